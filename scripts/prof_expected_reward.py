"""The expected reward and its gradient on a bench corpus: one smm_logz_f64 launch with SMM_SHAPE_LOGZ_BOTH, then per repetition
one smm_expected_reward_f64 and one smm_expected_reward_bwd_f64 with reward = onehot(ground truth) and seg_reward = 1, and on the
same inputs one smm_entropy_bwd_f64 (its six kernels beside the new ones) and one smm_segment_posteriors_f64
(smm_segpost_dense_kernel beside the value kernel).  HIP events here; run under `rocprofv3 --kernel-trace --stats` for the
per-kernel times.  Every repetition is checked bit-identical to the first.
usage: python scripts/prof_expected_reward.py [cfg2|cfg4|cfg3] [repetitions]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from action_segmentation_amd import ops, synth

workload = sys.argv[1] if len(sys.argv) > 1 else 'cfg2'
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
a = bench.parse(['--workload', workload])
dev = torch.device('cuda:0')
cfg = synth.CONFIGS[a.workload]
data = synth.SynthDatasplit(a.workload, seed=a.seed, device=dev, scale=a.scale)
_, model = bench.fit_model(a, cfg, data, dev, None, 1)
pc = model.prepare(data)
t = pc.tables
batch = pc.batch
elp, _ = ops.emission(batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
# reward = onehot(ground truth) on local states, seg_reward = 1
cmap = t['class_map'].cpu().numpy()
group = np.zeros(batch.b, np.int64) if batch.group is None else batch.group
reward = np.zeros((batch.total_frames, batch.c_max))
for name, task, off, n, g in zip(pc.video_names, pc.task_names, pc.frame_offset, batch.lengths.tolist(), group):
    gt = np.asarray(data[(task, name)]['gt_single'].cpu()).reshape(-1)[:n]
    hit = gt[:, None] == cmap[g, :batch.n_states[g]][None]
    reward[int(off):int(off) + n, :batch.n_states[g]] = hit
reward = torch.from_numpy(reward).to(dev)
seg = torch.ones((batch.n_groups, batch.c_max), dtype=torch.float64, device=dev)
ws = torch.empty(batch.workspace_bytes(), dtype=torch.uint8, device=dev)
tabs = (t['trans'], t['init'], t['len'])
kw = dict(endpen=pc.endpen, ws=ws, with_backward=True)
z = ops.logz(batch, elp, *tabs, **kw)
v = ops.expected_reward(batch, elp, *tabs, z, reward=reward, seg_reward=seg, **kw)
g = ops.expected_reward_bwd(batch, elp, *tabs, z, reward=reward, seg_reward=seg, want_value=True, **kw)
torch.cuda.synchronize()
assert ops.error_flag(batch, ws=ws) == 0
names = ('elp', 'trans', 'init', 'len')
ms = {k: [] for k in ('value', 'grad', 'entropy_bwd', 'segpost')}
for rep in range(reps):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    e[0].record()
    v2 = ops.expected_reward(batch, elp, *tabs, z, reward=reward, seg_reward=seg, **kw)
    e[1].record()
    g2 = ops.expected_reward_bwd(batch, elp, *tabs, z, reward=reward, seg_reward=seg, want_value=True, **kw)
    e[2].record()
    ops.entropy_bwd(batch, elp, *tabs, z, **kw)
    e[3].record()
    ops.segment_posteriors(batch, elp, *tabs, z, **kw)
    e[4].record()
    torch.cuda.synchronize()
    for i, k in enumerate(('value', 'grad', 'entropy_bwd', 'segpost')):
        ms[k].append(e[i].elapsed_time(e[i + 1]))
    assert torch.equal(v2, v), 'the value is not bit-identical run to run'
    assert all(torch.equal(g2[k], g[k]) for k in names + ('value',)), 'the gradient is not bit-identical run to run'
vh, vv = v.cpu().numpy(), g['value'].cpu().numpy()
frames = batch.lengths.astype(np.float64)
d01 = np.abs(vv[:, 0] - vv[:, 1]) / np.maximum(1.0, np.abs(vv[:, 0]))
dv = np.abs(vv[:, 0] - vh) / np.maximum(1.0, np.abs(vh))
med = {k: float(np.median(x)) for k, x in ms.items()}
print('%s: %d videos, %d frames: expected_reward call %.3f ms, expected_reward_bwd call %.3f ms (medians of %d); on the same inputs '
      'entropy_bwd call %.3f ms, segment_posteriors call %.3f ms; expected accuracy + segments / frames: mean %.4f; V- and V+ differ '
      'by <= %.3g, from the value call by <= %.3g (relative to max(1, |V|)); max |g_elp| %.4g; finite: %s'
      % (workload, pc.n_videos, pc.n_frames, med['value'], med['grad'], reps, med['entropy_bwd'], med['segpost'],
         float((vh / frames).mean()), d01.max(), dv.max(), float(g['elp'].abs().max()),
         bool(all(torch.isfinite(g[k]).all() for k in names))))
