"""The expected reward under the transcript-graph posterior and its gradient on a bench corpus, on
scripts/prof_align_graph_entropy.py's three workloads and timed as that script times (HIP events around the calls, medians of 5;
the graphs' classes, masks and flags are on the device from a first call; run under `rocprofv3 --kernel-trace --stats`, in a run
of its own, for the per-kernel times):
  (i)   every video's own Viterbi transcript as a chain graph;
  (ii)  the same transcripts with an optional entry of a random class between every two entries and at both ends
        (M -> 2 M + 1) as a graph;
  (iii) per video the trie of its own transcript and 7 perturbed copies (one entry replaced or dropped each).
reward = one-hot of the ground truth labels, node_reward = 1: the expected number of correct frames plus the expected number of
segments.  Per repetition and workload: one forward call, then five calls on its workspace, each of which launches
smm_align_graph_logz_bwd_kernel first: the value call (prefix, value, sum), the gradient call (prefix, eta-, eta+, assembly, then
the entropy gradient's g_elp and reduce kernels), and the yardsticks: the entropy call (one kernel), the entropy-gradient call
(five kernels) and the backward call (g_elp, g_len, reduce), the by-hand route to the value.  Every repetition, the warm-up one
included, issues the same kernels in the same order, which is how the second mode tells the launches of one kernel apart.  The
summary line is printed and appended to profiles/align_graph_expected_reward_kernel_times.txt (or to the file given as the second
argument).
usage: python scripts/prof_align_graph_expected_reward.py [cfg2|cfg4|cfg3|refdef] [out.txt]
       python scripts/prof_align_graph_expected_reward.py --trace KERNEL_TRACE.csv     (the per-kernel table of a traced run)"""
import csv
import os
import sys

import numpy as np

REPS = 5
FWD, BWD = 'smm_align_graph_logz_fwd_kernel', 'smm_align_graph_logz_bwd_kernel'
OCC, REDUCE = 'smm_align_graph_entropy_bwd_occ_kernel', 'smm_align_graph_entropy_bwd_reduce_kernel'
PREFIX = 'smm_align_graph_er_prefix_kernel'
# the calls of one workload of one repetition behind the forward call, in order: (name, its kernels)
CALLS = (('value', (BWD, PREFIX, 'smm_align_graph_er_value_kernel', 'smm_align_graph_er_sum_kernel')),
         ('gradient', (BWD, PREFIX, 'smm_align_graph_er_eta_minus_kernel', 'smm_align_graph_er_eta_plus_kernel',
                       'smm_align_graph_er_bwd_kernel', OCC, REDUCE)),
         ('entropy', (BWD, 'smm_align_graph_entropy_kernel')),
         ('entropy gradient', (BWD, 'smm_align_graph_eta_minus_kernel', 'smm_align_graph_eta_plus_kernel',
                               'smm_align_graph_entropy_bwd_kernel', OCC, REDUCE)),
         ('backward', (BWD, 'smm_align_opt_logz_occ_kernel', 'smm_align_opt_logz_glen_kernel', 'smm_align_opt_logz_reduce_kernel')))
SEQ = (FWD,) + tuple(k for _, ks in CALLS for k in ks)
ORDER = [('(i)', 'chains'), ('(ii)', '2 M + 1'), ('(iii)', 'tries of 8')]


def summarize(path):
    """The kernel trace of one run -> per workload the time of every kernel of SEQ, avg / min / max over the repetitions after
    the warm-up one, and each call's kernel time; the gradient call against the entropy-gradient call, the value call against
    the entropy call and the backward call."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r['Kernel_Name'].split('(')[0]
            if name in SEQ:
                rows.append((int(r['Start_Timestamp']), name, (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6))
    rows.sort()
    assert len(rows) == (REPS + 1) * len(ORDER) * len(SEQ), (len(rows), len(SEQ))
    out = []
    for w, (wl, what) in enumerate(ORDER):
        t = [[] for _ in SEQ]
        for rep in range(1, REPS + 1):
            for q, k in enumerate(SEQ):
                row = rows[(rep * len(ORDER) + w) * len(SEQ) + q]
                assert row[1] == k, (row, k)
                t[q].append(row[2])
        q, total = 1, {}
        out.append('  %-5s %-12s %-62s avg %.3f ms  min %.3f  max %.3f' % (wl, what, FWD, np.mean(t[0]), min(t[0]), max(t[0])))
        for call, ks in CALLS:
            for k in ks:
                out.append('  %-5s %-12s %-62s avg %.3f ms  min %.3f  max %.3f'
                           % (wl, what, '%s (%s call)' % (k, call), np.mean(t[q]), min(t[q]), max(t[q])))
                q += 1
            total[call] = sum(np.mean(x) for x in t[q - len(ks):q])
        out.append('  %-5s %-12s gradient call %.3f ms: x%.2f of the entropy-gradient call (%.3f ms); value call %.3f ms: x%.2f of '
                   'the entropy call (%.3f ms), x%.2f of the backward call (%.3f ms)'
                   % (wl, what, total['gradient'], total['gradient'] / total['entropy gradient'], total['entropy gradient'],
                      total['value'], total['value'] / total['entropy'], total['entropy'], total['value'] / total['backward'],
                      total['backward']))
    return '\n'.join(out)


if len(sys.argv) > 2 and sys.argv[1] == '--trace':
    print(summarize(sys.argv[2]))
    sys.exit(0)

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
tabs = (t['trans'], t['init'], t['len'])
reward = model.model._onehot_labels_packed(pc, model._packed_labels(pc, data, None, 'prof_align_graph_expected_reward')).contiguous()


def sub(keep, graphs):
    """The launch of the videos `keep`: batch, graphs, endpen rows, the forward call's workspace, the nodes' rewards."""
    batch = ops.Batch(B.lengths[keep], B.n_states, B.k_rows, c_max=B.c_max, frame_offset=B.frame_offset[keep], group=group[keep],
                      kp=kp[keep], t_max=B.t_max, total_frames=B.total_frames)
    gs = [graphs[i] for i in keep]
    ep = None if pc.endpen is None else pc.endpen[torch.as_tensor(keep, device=dev)].contiguous()
    off = np.concatenate([[0], np.cumsum([len(g) for g in gs])]).astype(np.int64)
    ws = torch.empty(ops.align_graph_logz_workspace_bytes(batch, off), dtype=torch.uint8, device=dev)
    return dict(batch=batch, graphs=gs, endpen=ep, ws=ws, staged=None, node_reward=torch.ones(int(off[-1]), dtype=torch.float64, device=dev))


def calls(s):
    """-> (log Z_g, the five calls' results in CALLS' order, the events between the calls)."""
    z = ops.align_graph_logz(s['batch'], elp, *tabs, s['graphs'], endpen=s['endpen'], ws=s['ws'], staged=s['staged'])
    s['staged'] = z['_staged']
    args = (s['batch'], elp, *tabs, s['graphs'], z['logz'])
    kw = dict(endpen=s['endpen'], ws=s['ws'], staged=s['staged'])
    rw = dict(reward=reward, node_reward=s['node_reward'])
    mids = [torch.cuda.Event(enable_timing=True) for _ in range(len(CALLS))]
    out = []
    for ev, f in zip(mids, (lambda: ops.align_graph_expected_reward(*args, **rw, **kw),
                            lambda: ops.align_graph_expected_reward_bwd(*args, **rw, want_value=True, **kw),
                            lambda: ops.align_graph_entropy(*args, **kw), lambda: ops.align_graph_entropy_bwd(*args, **kw),
                            lambda: ops.align_graph_logz_bwd(*args, **kw))):
        ev.record()
        out.append(f())
    return z['logz'], out, mids


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
g2 = []
for i, x in enumerate(tr):
    y = rng.integers(0, B.n_states[group[i]], size=2 * len(x) + 1)
    y[1::2] = x
    g2.append(TG.from_optional(y[:ops.MAX_TRANSCRIPT], (np.arange(len(y)) % 2 == 0)[:ops.MAX_TRANSCRIPT]))
ms2 = 2 * ms1 + 1
s2 = sub(np.flatnonzero(ms2 <= ops.MAX_TRANSCRIPT), g2)
# (iii) the trie of the transcript and 7 distinct perturbed copies
cands = []
for i, x in enumerate(tr):
    mine = [x]
    while len(mine) < 8:
        y = perturbed(x, int(B.n_states[group[i]]))
        if not any(np.array_equal(y, z) for z in mine):
            mine.append(y)
    cands.append(mine)
ok3 = np.array([TG.trie_nodes(c) <= ops.MAX_TRANSCRIPT and max(len(y) for y in c) <= ops.MAX_TRANSCRIPT for c in cands])
s3 = sub(np.flatnonzero(ok3), [TG.from_candidates(c) if k else None for c, k in zip(cands, ok3)])

n_calls = 1 + len(CALLS)
times = [[] for _ in range(3 * n_calls)]
total, gmax, gap = [0.0] * 3, [0.0] * 3, [0.0] * 3
for rep in range(REPS + 1):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    mids, outs = [], []
    e[0].record()
    for q, s in enumerate((s1, s2, s3)):
        z, out, mid = calls(s)
        e[q + 1].record()
        mids.append(mid)
        outs.append((z, out))
    torch.cuda.synchronize()
    if rep == 0:                                                  # the warm-up repetition: the values, once
        for q, (z, out) in enumerate(outs):
            s = (s1, s2, s3)[q]
            v, g = out[0], out[1]
            assert ops.error_flag(s['batch'], v) == 0 and ops.error_flag(s['batch'], g) == 0
            assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(v['value']).all()) and bool(torch.isfinite(g['elp']).all())
            total[q], gmax[q] = float(v['value'].sum()), float(g['elp'].abs().max())
            gap[q] = float(torch.maximum((g['value'] - v['value']).abs(), (g['value_plus'] - v['value']).abs()).max())
        continue
    for q in range(3):
        ev = [e[q]] + mids[q] + [e[q + 1]]
        for c in range(n_calls):
            times[n_calls * q + c].append(ev[c].elapsed_time(ev[c + 1]))
med = [float(np.median(x)) for x in times]
m3 = np.array([len(g) for g in s3['graphs']])
what = ['(i) chains', '(ii) an optional entry between every two and at both ends (median %d nodes)' % int(np.median(ms2)),
        '(iii) the trie of the transcript and 7 perturbed copies (median %d nodes)' % int(np.median(m3))]
line = ('%s: %d videos, %d frames, longest %d; Viterbi transcripts: median %d, longest %d entries; reward = one-hot ground truth, '
        'node_reward = 1; one forward call, then the value, gradient, entropy, entropy-gradient and backward calls'
        % (workload, pc.n_videos, pc.n_frames, int(max(pc.lengths)), int(np.median(ms1)), int(ms1.max())))
for q, s in enumerate((s1, s2, s3)):
    f, v, g, h, hg, b = med[n_calls * q:n_calls * (q + 1)]
    line += ('; %s, %d videos: forward %.3f ms, value %.3f ms (x%.2f of the entropy call %.3f ms, x%.2f of the backward call %.3f ms), '
             'gradient %.3f ms (x%.2f of the entropy-gradient call %.3f ms); sum of V %.6f, worst |V- - V|, |V+ - V| %.1e, '
             'max |dV / d elp| %.3e' % (what[q], len(s['graphs']), f, v, v / h, h, v / b, b, g, g / hg, hg, total[q], gap[q], gmax[q]))
line += ' (medians of %d)' % REPS
print(line)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              'profiles', 'align_graph_expected_reward_kernel_times.txt')
with open(out_path, 'a') as f:
    f.write(line + '\n')
