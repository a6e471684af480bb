"""The segment and boundary posteriors on a bench corpus: one smm_logz_f64 launch (forward and time-reversed) and one
smm_segment_posteriors_f64 launch on the Viterbi spans, a few times (HIP events here; run under `rocprofv3 --kernel-trace --stats`
for the per-kernel times, smm_segpost_dense_kernel and smm_segpost_spans_kernel beside smm_logz_kernel; one smm_logz_bwd_f64 per
repetition puts smm_marginals_kernel beside them).  Then the transcript-graph family on every video's own Viterbi transcript as
a chain graph: one forward call, one backward call and one smm_align_graph_segment_posteriors_f64 launch on the best alignment
per repetition (smm_align_graph_segpost_nodes_kernel and smm_align_graph_segpost_sets_kernel beside
smm_align_graph_logz_bwd_kernel).  profiles/segment_posterior_kernel_times.txt holds one such run.
usage: python scripts/prof_segment_posterior.py [cfg3|cfg2|cfg4]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from action_segmentation_amd import ops, synth

workload = sys.argv[1] if len(sys.argv) > 1 else 'cfg2'
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
spans = ops.viterbi(pc.batch, elp, *tabs, endpen=pc.endpen, class_map=t['class_map'], want_labels=False)['spans']
kw = dict(endpen=pc.endpen, ws=ws, with_backward=True)
ms_z, ms_p = [], []
for rep in range(6):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record()
    z = ops.logz(pc.batch, elp, *tabs, **kw)
    e[1].record()
    out = ops.segment_posteriors(pc.batch, elp, *tabs, z, spans=spans, class_map=t['class_map'], **kw)
    e[2].record()
    ops.logz_bwd(pc.batch, elp, *tabs, z, **kw)
    torch.cuda.synchronize()
    ms_z.append(e[0].elapsed_time(e[1]))
    ms_p.append(e[1].elapsed_time(e[2]))
assert ops.error_flag(pc.batch, out) == 0
sp = spans.cpu().numpy()
p = np.exp(out['seg_logp'].cpu().numpy())
starts = np.zeros_like(sp, dtype=bool)
for i, n in enumerate(pc.batch.lengths.tolist()):
    starts[i, :n] = sp[i, :n] != -1
ps = p[starts]
print('%s: %d videos, %d frames, %d decoded segments: logz call (both directions) %.3f ms (median), segment-posterior call %.3f ms '
      '(median); P(decoded segment): min %.3g, median %.3g, max %.6g; finite: %s'
      % (workload, pc.n_videos, pc.n_frames, int(starts.sum()), float(np.median(ms_z[1:])), float(np.median(ms_p[1:])), ps.min(),
         np.median(ps), ps.max(), bool(np.isfinite(ps).all())))

# ---- the transcript-graph family: every video's own Viterbi transcript as a chain graph (local ids), its best alignment as the
# given alignment; per repetition one forward call, the backward call (smm_align_graph_logz_bwd_kernel beside the new kernels)
# and the segment-posterior call
from action_segmentation_amd.semimarkov_utils import spans_to_transcripts

B = pc.batch
vit = ops.viterbi(B, elp, *tabs, endpen=pc.endpen, want_labels=False)             # (no class map: local ids)
tr = [np.asarray(x, np.int64) for x in spans_to_transcripts(vit['spans'], B.lengths)]
keep = np.flatnonzero(np.array([len(x) for x in tr]) <= ops.MAX_TRANSCRIPT)
group = B.group if B.group is not None else np.zeros(B.b, np.int32)
kp = B.kp if B.kp is not None else np.full(B.b, min(B.k_rows, B.t_max), np.int32)
gb = ops.Batch(B.lengths[keep], B.n_states, B.k_rows, c_max=B.c_max, frame_offset=B.frame_offset[keep], group=group[keep],
               kp=kp[keep], t_max=B.t_max, total_frames=B.total_frames)
graphs = [ops.TranscriptGraph.chain(tr[i]) for i in keep]
ep = None if pc.endpen is None else pc.endpen[torch.as_tensor(keep, device=dev)].contiguous()
best = ops.align_graph(gb, elp, *tabs, graphs, endpen=ep, want_labels=False, want_used=True)
staged, ms_g = None, []
for rep in range(6):
    z = ops.align_graph_logz(gb, elp, *tabs, graphs, endpen=ep, staged=staged)
    staged = z['_staged']
    ops.align_graph_logz_bwd(gb, elp, *tabs, graphs, z['logz'], endpen=ep, ws=z['ws'], staged=staged)
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    g = ops.align_graph_segment_posteriors(gb, elp, *tabs, graphs, z['logz'], spans=best['spans'], used=best['used'], endpen=ep,
                                           ws=z['ws'], staged=staged)
    e[1].record()
    torch.cuda.synchronize()
    ms_g.append(e[0].elapsed_time(e[1]))
assert ops.error_flag(gb, g) == 0
pn = np.exp(torch.cat(g['node_logp']).cpu().numpy())
sd = torch.cat(g['end_sd']).cpu().numpy()
print('%s, chains of the Viterbi transcripts: %d videos, %d nodes: segment-posterior call %.3f ms (median); P(aligned segment): min '
      '%.3g, median %.3g; end_sd: median %.3g, max %.3g frames'
      % (workload, len(keep), len(pn), float(np.median(ms_g[1:])), pn.min(), np.median(pn), np.median(sd), sd.max()))
