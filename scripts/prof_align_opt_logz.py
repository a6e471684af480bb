"""Transcript likelihood with optional entries on a bench corpus (smm_align_opt_logz_f64 / smm_align_opt_logz_bwd_f64), every
video with the transcript of its own Viterbi decode:
  (i)   no flag set, beside smm_align_logz_f64 / smm_align_logz_bwd_f64 on the same inputs (the same values);
  (ii)  the same transcripts with an optional entry of a random class between every two entries and at both ends (the
        transcripts of scripts/prof_align_optional.py: M -> 2 M + 1).
HIP events here; run under `rocprofv3 --kernel-trace --stats` for the per-kernel times (the five smm_align_opt_logz_* kernels).
The summary line is printed and appended to profiles/align_opt_logz_kernel_times.txt (or to the file given as the second
argument).
usage: python scripts/prof_align_opt_logz.py [cfg2|cfg4|cfg3|refdef] [out.txt]"""
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
group = B.group if B.group is not None else np.zeros(B.b, np.int32)
rng = np.random.default_rng(0)
tabs = (t['trans'], t['init'], t['len'])
fl1 = [np.zeros(len(x), bool) for x in tr]
tr2, fl2 = [], []
for i, x in enumerate(tr):
    y = rng.integers(0, B.n_states[group[i]], size=2 * len(x) + 1)
    y[1::2] = x
    tr2.append(y)
    fl2.append(np.arange(len(y)) % 2 == 0)
ms1, ms2 = np.array([len(x) for x in tr]), np.array([len(x) for x in tr2])
assert ms2.max() <= ops.MAX_TRANSCRIPT, "a Viterbi path with more than %d segments" % ((ops.MAX_TRANSCRIPT - 1) // 2)


class Side:
    """One set of transcripts and flags, staged once: the calls copy nothing from the host."""

    def __init__(self, ids, flags):
        self.ids, self.flags = ids, flags
        _, off = ops._transcript_arrays(B, ids)
        self.ws = torch.empty(ops.align_opt_logz_workspace_bytes(B, off), dtype=torch.uint8, device=dev)
        self.staged = ops.align_opt_logz(B, elp, *tabs, ids, flags, endpen=pc.endpen, ws=self.ws)['_staged']

    def fwd(self):
        return ops.align_opt_logz(B, elp, *tabs, self.ids, self.flags, endpen=pc.endpen, ws=self.ws, staged=self.staged)['logz']

    def bwd(self, z):
        return ops.align_opt_logz_bwd(B, elp, *tabs, self.ids, self.flags, z, endpen=pc.endpen, ws=self.ws, staged=self.staged,
                                      want_entry_prob=True)


s1, s2 = Side(tr, fl1), Side(tr2, fl2)
ids, off = ops._transcript_arrays(B, tr)
tr_dev = (torch.from_numpy(ids).to(dev), off)
ws_a = torch.empty(ops.align_logz_workspace_bytes(B, off), dtype=torch.uint8, device=dev)


def exact_fwd():
    return ops.align_logz(B, elp, *tabs, tr_dev, endpen=pc.endpen, ws=ws_a)


def exact_bwd(z):
    return ops.align_logz_bwd(B, elp, *tabs, tr_dev, z, endpen=pc.endpen, ws=ws_a)


za, z1, z2 = exact_fwd(), s1.fwd(), s2.fwd()
ga, g1, g2 = exact_bwd(za), s1.bwd(z1), s2.bwd(z2)
best2 = ops.align_optional(B, elp, *tabs, tr2, fl2, endpen=pc.endpen, want_labels=False, want_spans=False)['best']
torch.cuda.synchronize()
same = float(((z1 - za).abs() / za.abs().clamp(min=1.0)).max())
same_g = max(float((g1[k] - ga[k]).abs().max()) for k in ('elp', 'trans', 'init', 'len'))
ok = bool(torch.isfinite(z2).all() and (best2 <= z2 + 1e-9 * z2.abs()).all() and (za <= z2 + 1e-9 * z2.abs()).all())
rows = torch.cat([g2['elp'][o:o + n].sum(1) for o, n in zip(B.frame_offset, B.lengths)])
p2 = torch.cat(g2['entry_prob'])
ms = {k: [] for k in ('exact_fwd', 'exact_bwd', 'fwd1', 'bwd1', 'fwd2', 'bwd2')}
for rep in range(5):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    e[0].record()
    za = exact_fwd()
    e[1].record()
    exact_bwd(za)
    e[2].record()
    z1 = s1.fwd()
    e[3].record()
    s1.bwd(z1)
    e[4].record()
    z2 = s2.fwd()
    e[5].record()
    s2.bwd(z2)
    e[6].record()
    torch.cuda.synchronize()
    for j, k in enumerate(('exact_fwd', 'exact_bwd', 'fwd1', 'bwd1', 'fwd2', 'bwd2')):
        ms[k].append(e[j].elapsed_time(e[j + 1]))
med = {k: float(np.median(v)) for k, v in ms.items()}
line = ('%s: %d videos, %d frames, longest %d; Viterbi transcripts: median %d, longest %d entries; (i) no flags: align_logz call '
        '%.3f ms, align_logz_bwd call %.3f ms; align_opt_logz call %.3f ms, align_opt_logz_bwd call %.3f ms; max rel |logZ_o - '
        'logZ_a| %.1e, max |gradient difference| %.1e; (ii) an optional entry between every two and at both ends (median %d '
        'entries): align_opt_logz call %.3f ms, align_opt_logz_bwd call %.3f ms; best <= log Z_o and log Z_a <= log Z_o: %s; '
        'max |sum_c g_elp - 1| %.2e; entry posteriors in [%.3g, %.9g] (medians of 5)'
        % (workload, pc.n_videos, pc.n_frames, int(max(pc.lengths)), int(np.median(ms1)), int(ms1.max()), med['exact_fwd'],
           med['exact_bwd'], med['fwd1'], med['bwd1'], same, same_g, int(np.median(ms2)), med['fwd2'], med['bwd2'], ok,
           float((rows - 1.0).abs().max()), float(p2.min()), float(p2.max())))
print(line)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              'profiles', 'align_opt_logz_kernel_times.txt')
with open(out_path, 'a') as f:
    f.write(line + '\n')
