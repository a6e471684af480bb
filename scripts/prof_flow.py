"""The feature projection on a bench corpus' feature shape: smm_flow_f32, smm_flow_bwd_f32 (+ its reduce) and the same flow as
plain torch fp32 modules on the same GPU, a few times each (HIP events here; run under `rocprofv3 --kernel-trace --stats` for
the per-kernel times: smm_flow_fwd_kernel, smm_flow_bwd_kernel, smm_flow_reduce_kernel beside torch's GEMM kernels), then
decode_packed with the projector against decode_packed of a plain module on pre-projected features.
usage: python scripts/prof_flow.py [cfg2|cfg4|cfg3] [hidden_units] [hidden_layers] [couple_layers]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from action_segmentation_amd import ops, synth
from action_segmentation_amd.flow import FeatureProjector

workload = sys.argv[1] if len(sys.argv) > 1 else 'cfg2'
h, hl, cl = (int(sys.argv[i]) if len(sys.argv) > i else v for i, v in ((2, 100), (3, 1), (4, 4)))
a = bench.parse(['--workload', workload])
dev = torch.device('cuda:0')
cfg = synth.CONFIGS[a.workload]
data = synth.SynthDatasplit(a.workload, seed=a.seed, device=dev, scale=a.scale)
_, model = bench.fit_model(a, cfg, data, dev, None, 1)
pc = model.prepare(data)
x = pc.x
n, d = x.shape
torch.manual_seed(0)
fp = FeatureProjector(d, h, hl, cl).to(dev)
shape, packed = fp.shape, fp.packed()
g_y = torch.randn_like(x)
flop = 2.0 * n * cl * sum(i * o for i, o in shape.layer_sizes)


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def torch_flow(xi):
    """The reference's NICETrans.forward on fp32 modules (what a user would run without the fused kernels)."""
    dh = d // 2
    h1, h2 = xi[:, :dh], xi[:, dh:]
    for i in range(cl):
        net = getattr(fp, 'cell%d' % i)
        src = h1 if i % 2 == 0 else h2
        t = src
        lins = net.linears()
        for lin in lins[:-1]:
            t = torch.relu(lin(t))
        t = lins[-1](t)
        if i % 2 == 0:
            h2 = h2 + t
        else:
            h1 = h1 + t
    return torch.cat([h1, h2], dim=1)


ms_f = timed(lambda: ops.flow(x, packed, shape))
ms_b = timed(lambda: ops.flow_bwd(x, g_y, packed, shape))
print('%s: %d rows x D = %d, H = %d, %d hidden, %d coupling layers (%.1f GFLOP per pass)' % (workload, n, d, h, hl, cl, flop / 1e9))
print('  smm_flow_f32      %.3f ms  = %.1f TFLOP/s = %.3f of the 157 TF fp32 matrix peak' % (ms_f, flop / ms_f / 1e9, flop / ms_f / 1e9 / 157))
print('  smm_flow_bwd_f32  %.3f ms  (the tile recomputed + the chain rule; the zero fill and the reduce kernel included)' % ms_b)
try:
    with torch.no_grad():
        y_t = torch_flow(x)
        err = float((y_t - ops.flow(x, packed, shape)).abs().max())
        ms_tf = timed(lambda: torch_flow(x))

    def torch_step():
        for p in fp.parameters():
            p.grad = None
        (torch_flow(x) * g_y).sum().backward()

    ms_tb = timed(torch_step)
    print('  torch fp32 modules: forward %.3f ms, forward + backward %.3f ms (max |y_torch - y_kernel| = %.2e)' % (ms_tf, ms_tb, err))
except RuntimeError as e:                                  # (a box whose torch has no usable GEMM back-end)
    print('  torch fp32 modules: not measured (%s)' % str(e).splitlines()[0])

# decode with the projector against the plain decode on pre-projected features
plain = model.model
y = ops.flow(x, packed, shape)
ms_plain = timed(lambda: plain.decode_packed(pc, x=y))
plain.feature_projector = fp
ms_cached = timed(lambda: plain.decode_packed(pc))


def fresh():
    pc.__dict__.pop('_projected', None)
    return plain.decode_packed(pc)


ms_fresh = timed(fresh)
plain.feature_projector = None
print('  decode_packed: plain on pre-projected features %.3f ms; with the projector %.3f ms (projection kept on the corpus), '
      '%.3f ms (projected again every call)' % (ms_plain, ms_cached, ms_fresh))
