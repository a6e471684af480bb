"""The MBR decode on a bench corpus: the pipeline (emission, smm_logz_f64 with the time-reversed recursion, smm_logz_bwd_f64 for
the frame posteriors, smm_mbr_f64) and, on the same substituted inputs (elp = the posteriors, zero length scores, binary tables),
one smm_viterbi_f64 launch for comparison, a few times (HIP events here; run under `rocprofv3 --kernel-trace --stats` for the
per-kernel times: smm_mbr_kernel beside smm_viterbi_kernel and the log Z / marginals launches).
usage: python scripts/prof_mbr.py [cfg3|cfg2|cfg4|refdef]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from action_segmentation_amd import ops, synth

workload = sys.argv[1] if len(sys.argv) > 1 else 'cfg3'
a = bench.parse(['--workload', workload])
dev = torch.device('cuda:0')
cfg = synth.CONFIGS[a.workload]
data = synth.SynthDatasplit(a.workload, seed=a.seed, device=dev, scale=a.scale)
_, model = bench.fit_model(a, cfg, data, dev, None, 1)
pc = model.prepare(data)
t = pc.tables
ws = torch.empty(max(pc.batch.workspace_bytes(), ops.mbr_workspace_bytes(pc.batch)), dtype=torch.uint8, device=dev)


def substituted(x):
    return torch.where(x <= -5e8, torch.full_like(x, -1e9), torch.zeros_like(x))


mt, mi = substituted(t['trans']), substituted(t['init'])
me = None if pc.endpen is None else substituted(pc.endpen)
lz = torch.zeros_like(t['len'])


def pipeline():
    elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
    z = ops.logz(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, ws=ws, with_backward=True)
    g = ops.logz_bwd(pc.batch, elp, t['trans'], t['init'], t['len'], z, endpen=pc.endpen, ws=ws, with_backward=True)
    return g['elp']


gain = pipeline()
out = ops.mbr(pc.batch, gain, t['trans'], t['init'], endpen=pc.endpen, class_map=t['class_map'], ws=ws, want_spans=False)
vit = ops.viterbi(pc.batch, gain, mt, mi, lz, endpen=me, class_map=t['class_map'], want_spans=False)
torch.cuda.synchronize()
ops.check_decoded(pc.batch, out)
ops.check_decoded(pc.batch, vit)
ms_p, ms_m, ms_v = [], [], []
for rep in range(5):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    gain = pipeline()
    e[1].record()
    out = ops.mbr(pc.batch, gain, t['trans'], t['init'], endpen=pc.endpen, class_map=t['class_map'], ws=ws, want_spans=False)
    e[2].record()
    vit = ops.viterbi(pc.batch, gain, mt, mi, lz, endpen=me, class_map=t['class_map'], want_spans=False)
    e[3].record()
    torch.cuda.synchronize()
    ms_p.append(e[0].elapsed_time(e[1]))
    ms_m.append(e[1].elapsed_time(e[2]))
    ms_v.append(e[2].elapsed_time(e[3]))
same = bool(torch.equal(out['labels'], vit['labels']) and torch.equal(out['best'], vit['best']))
ec = out['gain_sum'].cpu().numpy()
print('%s: %d videos, %d frames, longest %d: posterior (emission + log Z + marginals) %.3f ms, mbr call %.3f ms, viterbi call '
      'on the substituted inputs %.3f ms (medians of 5); mbr == viterbi(substituted): %s; expected correct frames / frames %.4f'
      % (workload, pc.n_videos, pc.n_frames, int(max(pc.lengths)), float(np.median(ms_p)), float(np.median(ms_m)),
         float(np.median(ms_v)), same, float(ec.sum()) / pc.n_frames))
