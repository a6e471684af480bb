"""The posterior sampler on a bench corpus: one smm_logz_f64 launch and one smm_sample_f64 launch of 16 samples per video, a
few times (HIP events here; run under `rocprofv3 --kernel-trace --stats` for the per-kernel times, smm_logz_kernel beside
smm_sample_kernel).  usage: python scripts/prof_sample.py [cfg3|cfg2] [n_samples]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from action_segmentation_amd import ops, synth

workload = sys.argv[1] if len(sys.argv) > 1 else 'cfg3'
n_samples = int(sys.argv[2]) if len(sys.argv) > 2 else 16
a = bench.parse(['--workload', workload])
dev = torch.device('cuda:0')
cfg = synth.CONFIGS[a.workload]
data = synth.SynthDatasplit(a.workload, seed=a.seed, device=dev, scale=a.scale)
_, model = bench.fit_model(a, cfg, data, dev, None, 1)
pc = model.prepare(data)
t = pc.tables
elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
ws = torch.empty(pc.batch.workspace_bytes(), dtype=torch.uint8, device=dev)
kw = dict(endpen=pc.endpen, class_map=t['class_map'], ws=ws, want_spans=False, want_labels=True)
z = ops.logz(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, ws=ws)
out = ops.sample(pc.batch, elp, t['trans'], t['init'], t['len'], z, n_samples, 0, **kw)
torch.cuda.synchronize()
ops.check_decoded(pc.batch, out)
ms_z, ms_s = [], []
for rep in range(5):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    z = ops.logz(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, ws=ws)
    e[1].record()
    out = ops.sample(pc.batch, elp, t['trans'], t['init'], t['len'], z, n_samples, rep, **kw)
    e[2].record()
    torch.cuda.synchronize()
    ms_z.append(e[0].elapsed_time(e[1]))
    ms_s.append(e[1].elapsed_time(e[2]))
lp = out['logp'].cpu().numpy()
lab = out['labels'].cpu().numpy()
n_seg = [int((np.diff(lab[s, o:o + ln]) != 0).sum()) + 1 for s in range(n_samples) for o, ln in zip(pc.frame_offset, pc.lengths)]
print('%s: %d videos, %d frames, %d samples per video: logz call %.3f ms (median), sample call %.3f ms (median); '
      'label runs per sampled video: mean %.0f, max %d; log p finite: %s'
      % (workload, pc.n_videos, pc.n_frames, n_samples, float(np.median(ms_z)), float(np.median(ms_s)),
         float(np.mean(n_seg)), max(n_seg), bool(np.isfinite(lp).all())))
