"""Forced alignment to a transcript graph on a bench corpus, timed as scripts/prof_align_optional.py times (HIP events around
the calls, medians of 5; the graphs are on the device from a first call, so a timed call copies nothing from the host; run
under `rocprofv3 --kernel-trace --stats` for the per-kernel times):
  (i)   every video's own Viterbi transcript as a chain graph, through smm_align_graph_f64, beside smm_align_f64 on the same
        inputs;
  (ii)  the same transcripts with an optional entry of a random class between every two entries and at both ends
        (M -> 2 M + 1) as a graph, beside smm_align_opt_f64 on the same transcripts and flags;
  (iii) per video the trie of its own transcript and 7 perturbed copies (one entry replaced or dropped each): one
        smm_align_graph_f64 call beside the 8 smm_align_f64 calls it replaces.
The summary line is printed and appended to profiles/align_graph_kernel_times.txt (or to the file given as the second
argument).
usage: python scripts/prof_align_graph.py [cfg3|cfg2|cfg4|refdef] [out.txt]"""
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
vit = ops.viterbi(B, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, want_labels=False)   # (no class map: local ids)
torch.cuda.synchronize()
ops.check_decoded(B, vit)
tr = [np.asarray(x, np.int64) for x in spans_to_transcripts(vit['spans'], B.lengths)]
group = B.group if B.group is not None else np.zeros(B.b, np.int32)
kp = B.kp if B.kp is not None else np.full(B.b, min(B.k_rows, B.t_max), np.int32)
rng = np.random.default_rng(0)
TG = ops.TranscriptGraph


def sub(keep, graphs):
    """The launch of the videos `keep`: batch, graphs, endpen rows, a workspace large enough for every entry point."""
    batch = ops.Batch(B.lengths[keep], B.n_states, B.k_rows, c_max=B.c_max, frame_offset=B.frame_offset[keep], group=group[keep],
                      kp=kp[keep], t_max=B.t_max, total_frames=B.total_frames)
    gs = [graphs[i] for i in keep]
    ep = None if pc.endpen is None else pc.endpen[torch.as_tensor(keep, device=dev)].contiguous()
    off = np.concatenate([[0], np.cumsum([len(g) for g in gs])]).astype(np.int64)
    ws = torch.empty(max(ops.align_graph_workspace_bytes(batch, off), ops.align_opt_workspace_bytes(batch, off)),
                     dtype=torch.uint8, device=dev)
    return dict(batch=batch, graphs=gs, keep=keep, endpen=ep, ws=ws, staged=None)


def graph(s):
    out = ops.align_graph(s['batch'], elp, t['trans'], t['init'], t['len'], s['graphs'], endpen=s['endpen'], ws=s['ws'],
                          want_labels=False, staged=s['staged'])
    s['staged'] = out['_staged']
    return out


def align(s, transcripts):
    return ops.align(s['batch'], elp, t['trans'], t['init'], t['len'], [transcripts[i] for i in s['keep']], endpen=s['endpen'],
                     ws=s['ws'], want_labels=False)


def align_opt(s, transcripts, flags, staged=None):
    return ops.align_optional(s['batch'], elp, t['trans'], t['init'], t['len'], [transcripts[i] for i in s['keep']],
                              [flags[i] for i in s['keep']], endpen=s['endpen'], ws=s['ws'], want_labels=False, staged=staged)


def perturbed(x, n_states):
    y = x.copy()
    if len(y) > 1 and rng.random() < 0.5:
        return np.delete(y, int(rng.integers(0, len(y))))
    y[int(rng.integers(0, len(y)))] = int(rng.integers(0, n_states))
    return y


# (i) chains
ms1 = np.array([len(x) for x in tr])
s1 = sub(np.flatnonzero(ms1 <= ops.MAX_TRANSCRIPT), [TG.chain(x[:ops.MAX_TRANSCRIPT]) for x in tr])
# (ii) an optional entry of a random class of the video between every two entries and at both ends
tr2, fl2 = [], []
for i, x in enumerate(tr):
    y = rng.integers(0, B.n_states[group[i]], size=2 * len(x) + 1)
    y[1::2] = x
    tr2.append(y)
    fl2.append(np.arange(len(y)) % 2 == 0)
ms2 = np.array([len(x) for x in tr2])
s2 = sub(np.flatnonzero(ms2 <= ops.MAX_TRANSCRIPT), [TG.from_optional(y[:ops.MAX_TRANSCRIPT], f[:ops.MAX_TRANSCRIPT])
                                                     for y, f in zip(tr2, fl2)])
# (iii) the trie of the transcript and 7 perturbed copies
cands = [[x] + [perturbed(x, int(B.n_states[group[i]])) for _ in range(7)] for i, x in enumerate(tr)]
ok3 = np.array([TG.trie_nodes(c) <= ops.MAX_TRANSCRIPT and max(len(y) for y in c) <= ops.MAX_TRANSCRIPT for c in cands])
s3 = sub(np.flatnonzero(ok3), [TG.from_candidates(c) if k else None for c, k in zip(cands, ok3)])
per = [[c[j] for c in cands] for j in range(8)]

o0, o1 = align(s1, tr), graph(s1)
p2 = align_opt(s2, tr2, fl2)
o2, o3 = graph(s2), graph(s3)
each = [align(s3, per[j]) for j in range(8)]
torch.cuda.synchronize()
for s, o in ((s1, o0), (s1, o1), (s2, p2), (s2, o2), (s3, o3)):
    ops.check_decoded(s['batch'], o)
same1 = bool(torch.equal(o0['best'], o1['best']) and torch.equal(o0['spans'], o1['spans']))
same2 = bool(torch.equal(p2['best'], o2['best']) and torch.equal(p2['spans'], o2['spans']))
same3 = bool(torch.equal(torch.stack([e['best'] for e in each]).max(0).values, o3['best']))
times = [[] for _ in range(6)]
for rep in range(5):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    e[0].record()
    align(s1, tr)
    e[1].record()
    graph(s1)
    e[2].record()
    align_opt(s2, tr2, fl2, staged=p2['_staged'])
    e[3].record()
    graph(s2)
    e[4].record()
    for j in range(8):
        align(s3, per[j])
    e[5].record()
    graph(s3)
    e[6].record()
    torch.cuda.synchronize()
    for q in range(6):
        times[q].append(e[q].elapsed_time(e[q + 1]))
med = [float(np.median(x)) for x in times]
m3 = np.array([len(g) for g in s3['graphs']])
line = ('%s: %d videos, %d frames, longest %d; Viterbi transcripts: median %d, longest %d entries; (i) chains, %d videos: align '
        'call %.3f ms, align_graph call %.3f ms (x%.2f), equal: %s; (ii) an optional entry between every two and at both ends '
        '(median %d nodes), %d videos: align_optional call %.3f ms, align_graph call %.3f ms (x%.2f), equal: %s; (iii) the trie '
        'of the transcript and 7 perturbed copies (median %d nodes), %d videos: 8 align calls %.3f ms, one align_graph call '
        '%.3f ms (x%.2f), best equal: %s (medians of 5)'
        % (workload, pc.n_videos, pc.n_frames, int(max(pc.lengths)), int(np.median(ms1)), int(ms1.max()), len(s1['graphs']),
           med[0], med[1], med[1] / med[0], same1, int(np.median(ms2)), len(s2['graphs']), med[2], med[3], med[3] / med[2], same2,
           int(np.median(m3)), len(s3['graphs']), med[4], med[5], med[5] / med[4], same3))
print(line)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              'profiles', 'align_graph_kernel_times.txt')
with open(out_path, 'a') as f:
    f.write(line + '\n')
