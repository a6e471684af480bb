"""KL divergence and cross-entropy on a bench corpus: p is the bench's fitted model; q is the same workload fitted on a second
draw (seed + 1) where that draw has the same class inventory, else p with every parameter scaled by (1 + 0.05 N(0, 1)) from a
generator seeded with seed + 1 (the synthetic corpora of two seeds can differ in their number of classes, and KL needs one
lattice).  Both posteriors on p's corpus.  Per repetition one kl_packed, one cross_entropy_packed and one entropy_packed (HIP
events here; run under `rocprofv3 --kernel-trace --stats` for the per-kernel times, smm_kl_kernel beside smm_entropy_kernel on
the same corpus).  usage: python scripts/prof_kl.py [cfg3|cfg2|cfg4]"""
import copy
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from action_segmentation_amd import synth

workload = sys.argv[1] if len(sys.argv) > 1 else 'cfg3'
a = bench.parse(['--workload', workload])
a2 = bench.parse(['--workload', workload, '--seed', str(a.seed + 1)])
dev = torch.device('cuda:0')
cfg = synth.CONFIGS[a.workload]
data = synth.SynthDatasplit(a.workload, seed=a.seed, device=dev, scale=a.scale)
data2 = synth.SynthDatasplit(a.workload, seed=a2.seed, device=dev, scale=a.scale)
_, model = bench.fit_model(a, cfg, data, dev, None, 1)
_, model_q = bench.fit_model(a2, cfg, data2, dev, None, 1)
p, q = model.model, model_q.model
if (q.n_classes, q.input_feature_dim, q.max_k) != (p.n_classes, p.input_feature_dim, p.max_k):
    print('second draw: %d classes against %d; q = p perturbed' % (q.n_classes, p.n_classes))
    q = copy.deepcopy(p)
    g = torch.Generator().manual_seed(a2.seed)
    with torch.no_grad():
        for prm in (q.poisson_log_rates, q.gaussian_means, q.transition_logits, q.init_logits):
            prm.mul_(1.0 + 0.05 * torch.randn(prm.shape, generator=g).to(prm))
pc = model.prepare(data)
kl = p.kl_packed(q, pc)
torch.cuda.synchronize()
ms_kl, ms_x, ms_h = [], [], []
for rep in range(5):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    kl = p.kl_packed(q, pc)
    e[1].record()
    xe = p.cross_entropy_packed(q, pc)
    e[2].record()
    h = p.entropy_packed(pc)
    e[3].record()
    torch.cuda.synchronize()
    ms_kl.append(e[0].elapsed_time(e[1]))
    ms_x.append(e[1].elapsed_time(e[2]))
    ms_h.append(e[2].elapsed_time(e[3]))
kv, xv, hv = kl.cpu().numpy(), xe.cpu().numpy(), h.cpu().numpy()
print('%s: %d videos, %d frames: kl_packed %.3f ms, cross_entropy_packed %.3f ms, entropy_packed %.3f ms (medians; each with its '
      'emission and log Z launches); KL per video: min %.4g, median %.4g, max %.4g nats; per frame: median %.4g; '
      'max |H(p, q) - H(p) - KL| / H(p, q): %.3g; finite: %s'
      % (workload, pc.n_videos, pc.n_frames, float(np.median(ms_kl)), float(np.median(ms_x)), float(np.median(ms_h)), kv.min(),
         np.median(kv), kv.max(), float(np.median(kv / np.asarray(pc.lengths))), float(np.max(np.abs(xv - hv - kv) / xv)),
         bool(np.isfinite(kv).all())))
