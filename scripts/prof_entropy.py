"""The posterior entropy on a bench corpus: one smm_logz_f64 launch and one smm_entropy_f64 launch (which runs the time-reversed
recursion itself, then smm_entropy_kernel), a few times (HIP events here; run under `rocprofv3 --kernel-trace --stats` for the
per-kernel times, smm_logz_kernel beside smm_entropy_kernel; one smm_logz_bwd_f64 per repetition puts smm_marginals_kernel
beside them).  usage: python scripts/prof_entropy.py [cfg3|cfg2|cfg4]"""
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
elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
ws = torch.empty(pc.batch.workspace_bytes(), dtype=torch.uint8, device=dev)
tabs = (t['trans'], t['init'], t['len'])
z = ops.logz(pc.batch, elp, *tabs, endpen=pc.endpen, ws=ws)
h = ops.entropy(pc.batch, elp, *tabs, z, endpen=pc.endpen, ws=ws)
torch.cuda.synchronize()
assert ops.error_flag(pc.batch, ws=ws) == 0
ms_z, ms_h = [], []
for rep in range(5):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    z = ops.logz(pc.batch, elp, *tabs, endpen=pc.endpen, ws=ws)
    e[1].record()
    h = ops.entropy(pc.batch, elp, *tabs, z, endpen=pc.endpen, ws=ws)
    e[2].record()
    ops.logz_bwd(pc.batch, elp, *tabs, z, endpen=pc.endpen, ws=ws, with_backward=True)
    torch.cuda.synchronize()
    ms_z.append(e[0].elapsed_time(e[1]))
    ms_h.append(e[1].elapsed_time(e[2]))
hv = h.cpu().numpy()
print('%s: %d videos, %d frames: logz call %.3f ms (median), entropy call (reversed recursion + entropy) %.3f ms (median); '
      'H per video: min %.4g, median %.4g, max %.4g nats; per frame: median %.4g; finite: %s'
      % (workload, pc.n_videos, pc.n_frames, float(np.median(ms_z)), float(np.median(ms_h)), hv.min(), np.median(hv), hv.max(),
         float(np.median(hv / np.asarray(pc.lengths))), bool(np.isfinite(hv).all())))
