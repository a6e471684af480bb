"""The entropy's gradient on a bench corpus: one smm_logz_f64 launch, one smm_entropy_f64 launch (which runs the time-reversed
recursion), then smm_entropy_bwd_f64 on the same workspace, a few times (HIP events here; run under
`rocprofv3 --kernel-trace --stats` for the per-kernel times: smm_ebwd_eta_kernel, the serial pass, beside the assembly kernels;
one smm_logz_bwd_f64 per repetition puts smm_marginals_kernel / smm_glen_kernel beside them).
usage: python scripts/prof_entropy_grad.py [cfg3|cfg2|cfg4] [repetitions]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from action_segmentation_amd import ops, synth

workload = sys.argv[1] if len(sys.argv) > 1 else 'cfg3'
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
a = bench.parse(['--workload', workload])
dev = torch.device('cuda:0')
cfg = synth.CONFIGS[a.workload]
data = synth.SynthDatasplit(a.workload, seed=a.seed, device=dev, scale=a.scale)
_, model = bench.fit_model(a, cfg, data, dev, None, 1)
pc = model.prepare(data)
t = pc.tables
elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
ws = torch.empty(pc.batch.workspace_bytes(), dtype=torch.uint8, device=dev)
tabs = (t['trans'], t['init'], t['len'])
z = ops.logz(pc.batch, elp, *tabs, endpen=pc.endpen, ws=ws)
h = ops.entropy(pc.batch, elp, *tabs, z, endpen=pc.endpen, ws=ws)
g = ops.entropy_bwd(pc.batch, elp, *tabs, z, endpen=pc.endpen, ws=ws, with_backward=True, want_value=True)
torch.cuda.synchronize()
assert ops.error_flag(pc.batch, ws=ws) == 0
hv, v = h.cpu().numpy(), g['value'].cpu().numpy()
ms_b, ms_m = [], []
for rep in range(reps):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    g2 = ops.entropy_bwd(pc.batch, elp, *tabs, z, endpen=pc.endpen, ws=ws, with_backward=True)
    e[1].record()
    ops.logz_bwd(pc.batch, elp, *tabs, z, endpen=pc.endpen, ws=ws, with_backward=True)
    e[2].record()
    torch.cuda.synchronize()
    ms_b.append(e[0].elapsed_time(e[1]))
    ms_m.append(e[1].elapsed_time(e[2]))
    assert all(torch.equal(g2[k], g[k]) for k in ('elp', 'trans', 'init', 'len')), 'not bit-identical run to run'
d01 = np.abs(v[:, 0] - v[:, 1]) / np.maximum(1.0, v[:, 0])
dh = np.abs(v[:, 0] - hv) / np.maximum(1.0, hv)
print('%s: %d videos, %d frames: entropy_bwd call %.3f ms (median of %d), logz_bwd call %.3f ms; the two decompositions of H '
      'differ by <= %.3g, from smm_entropy_f64 by <= %.3g (relative to max(1, H)); max |g_elp| %.4g; finite: %s'
      % (workload, pc.n_videos, pc.n_frames, float(np.median(ms_b)), reps, float(np.median(ms_m)), d01.max(), dh.max(),
         float(g['elp'].abs().max()), bool(all(torch.isfinite(g[k]).all() for k in ('elp', 'trans', 'init', 'len')))))
