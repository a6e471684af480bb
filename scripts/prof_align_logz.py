"""Transcript likelihood on a bench corpus: log Z_a of every video for the transcript of its own Viterbi decode
(smm_align_logz_f64) and its gradient (smm_align_logz_bwd_f64), beside the alignment (smm_align_f64) and log Z with its gradient
(smm_logz_f64 / smm_logz_bwd_f64) of the same corpus.  HIP events here; run under `rocprofv3 --kernel-trace --stats` for the
per-kernel times (the six smm_align_logz_* kernels).  The summary line is printed and appended to
profiles/align_logz_kernel_times.txt (or to the file given as the second argument).
usage: python scripts/prof_align_logz.py [cfg2|cfg4|cfg3|refdef] [out.txt]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from action_segmentation_amd import ops, synth
from action_segmentation_amd.semimarkov_utils import spans_to_transcripts

workload = sys.argv[1] if len(sys.argv) > 1 else 'cfg2'
a = bench.parse(['--workload', workload])
dev = torch.device('cuda:0')
cfg = synth.CONFIGS[a.workload]
data = synth.SynthDatasplit(a.workload, seed=a.seed, device=dev, scale=a.scale)
_, model = bench.fit_model(a, cfg, data, dev, None, 1)
pc = model.prepare(data)
t, B = pc.tables, pc.batch
elp, _ = ops.emission(B, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
vit = ops.viterbi(B, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, want_labels=False)   # (local ids in the spans)
torch.cuda.synchronize()
ops.check_decoded(B, vit)
tr = spans_to_transcripts(vit['spans'], B.lengths)
ms_len = np.array([len(x) for x in tr])
assert ms_len.max() <= ops.MAX_TRANSCRIPT, "a Viterbi path with more than %d segments" % ops.MAX_TRANSCRIPT
ids, off = ops._transcript_arrays(B, tr)
tr_dev = (torch.from_numpy(ids).to(dev), off)
ws = torch.empty(ops.align_logz_workspace_bytes(B, off), dtype=torch.uint8, device=dev)
ws_z = torch.empty(B.workspace_bytes(), dtype=torch.uint8, device=dev)
ws_a = torch.empty(ops.align_workspace_bytes(B, off), dtype=torch.uint8, device=dev)
tabs = (t['trans'], t['init'], t['len'])


def fwd():
    return ops.align_logz(B, elp, *tabs, tr_dev, endpen=pc.endpen, ws=ws)


def bwd(z):
    return ops.align_logz_bwd(B, elp, *tabs, tr_dev, z, endpen=pc.endpen, ws=ws)


za = fwd()
g = bwd(za)
z = ops.logz(B, elp, *tabs, endpen=pc.endpen, ws=ws_z, with_backward=True)
torch.cuda.synchronize()
best = vit['best']
ok = bool(torch.isfinite(za).all() and (best <= za + 1e-9 * za.abs()).all() and (za <= z + 1e-9 * z.abs()).all())
rows = torch.cat([g['elp'][o:o + n].sum(1) for o, n in zip(B.frame_offset, B.lengths)])
ok_rows = float((rows - 1.0).abs().max())
ms = {k: [] for k in ('fwd', 'bwd', 'align', 'logz', 'logz_bwd')}
for rep in range(5):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    e[0].record()
    za = fwd()
    e[1].record()
    bwd(za)
    e[2].record()
    ops.align(B, elp, *tabs, tr, endpen=pc.endpen, ws=ws_a, want_labels=False)
    e[3].record()
    z = ops.logz(B, elp, *tabs, endpen=pc.endpen, ws=ws_z, with_backward=True)
    e[4].record()
    ops.logz_bwd(B, elp, *tabs, z, endpen=pc.endpen, ws=ws_z, with_backward=True)
    e[5].record()
    torch.cuda.synchronize()
    for j, k in enumerate(('fwd', 'bwd', 'align', 'logz', 'logz_bwd')):
        ms[k].append(e[j].elapsed_time(e[j + 1]))
med = {k: float(np.median(v)) for k, v in ms.items()}
line = ('%s: %d videos, %d frames, longest %d; transcripts: median %d, longest %d entries; align_logz call %.3f ms, '
        'align_logz_bwd call %.3f ms; align call %.3f ms, logz call (both directions) %.3f ms, logz_bwd call %.3f ms (medians of '
        '5); best <= log Z_a <= log Z: %s; max |sum_c g_elp - 1|: %.2e'
        % (workload, pc.n_videos, pc.n_frames, int(max(pc.lengths)), int(np.median(ms_len)), int(ms_len.max()), med['fwd'],
           med['bwd'], med['align'], med['logz'], med['logz_bwd'], ok, ok_rows))
print(line)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              'profiles', 'align_logz_kernel_times.txt')
with open(out_path, 'a') as f:
    f.write(line + '\n')
