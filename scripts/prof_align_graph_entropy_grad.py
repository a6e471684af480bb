"""The gradient of the transcript-graph entropy on a bench corpus, on scripts/prof_align_graph_entropy.py's three workloads and
timed as that script times (HIP events around the calls, medians of 5; the graphs' classes, masks and flags are on the device
from a first call; run under `rocprofv3 --kernel-trace --stats`, in a run of its own, for the per-kernel times):
  (i)   every video's own Viterbi transcript as a chain graph;
  (ii)  the same transcripts with an optional entry of a random class between every two entries and at both ends
        (M -> 2 M + 1) as a graph;
  (iii) per video the trie of its own transcript and 7 perturbed copies (one entry replaced or dropped each).
Per repetition and workload: one forward call, the entropy-gradient call (smm_align_graph_logz_bwd_kernel, then the eta-, eta+,
assembly, g_elp and reduce kernels of smm_align_graph_entropy_bwd.hip) and, beside it, the backward call (that first kernel again,
then the g_elp, g_len and reduce kernels): the yardstick.  Every repetition, the warm-up one included, issues the same kernels in
the same order, which is how the second mode tells the launches of one kernel apart.  The summary line is printed and appended
to profiles/align_graph_entropy_grad_kernel_times.txt (or to the file given as the second argument).
usage: python scripts/prof_align_graph_entropy_grad.py [cfg2|cfg4|cfg3|refdef] [out.txt]
       python scripts/prof_align_graph_entropy_grad.py --trace KERNEL_TRACE.csv     (the per-kernel table of a traced run)"""
import csv
import os
import sys

import numpy as np

REPS = 5
FWD, BWD = 'smm_align_graph_logz_fwd_kernel', 'smm_align_graph_logz_bwd_kernel'
OWN = ('smm_align_graph_eta_minus_kernel', 'smm_align_graph_eta_plus_kernel', 'smm_align_graph_entropy_bwd_kernel',
       'smm_align_graph_entropy_bwd_occ_kernel', 'smm_align_graph_entropy_bwd_reduce_kernel')
TAIL = ('smm_align_opt_logz_occ_kernel', 'smm_align_opt_logz_glen_kernel', 'smm_align_opt_logz_reduce_kernel')
CALL = (FWD, BWD) + OWN + (BWD,) + TAIL                  # the kernels of one workload of one repetition, in order
ORDER = [('(i)', 'chains'), ('(ii)', '2 M + 1'), ('(iii)', 'tries of 8')]


def summarize(path):
    """The kernel trace of one run -> per workload the time of every kernel of CALL, avg / min / max over the repetitions after
    the warm-up one, and the entropy-gradient call's six kernels against the backward call's four."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r['Kernel_Name'].split('(')[0]
            if name in CALL:
                rows.append((int(r['Start_Timestamp']), name, (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6))
    rows.sort()
    assert len(rows) == (REPS + 1) * len(ORDER) * len(CALL), (len(rows), len(CALL))
    out = []
    n_own = 1 + len(OWN)
    for w, (wl, what) in enumerate(ORDER):
        t = [[] for _ in CALL]
        for rep in range(1, REPS + 1):
            for q, k in enumerate(CALL):
                row = rows[(rep * len(ORDER) + w) * len(CALL) + q]
                assert row[1] == k, (row, k)
                t[q].append(row[2])
        for q, k in enumerate(CALL):
            whose = ' (entropy-gradient call)' if q == 1 else ' (backward call)' if q == 1 + n_own else ''
            out.append('  %-5s %-12s %-62s avg %.3f ms  min %.3f  max %.3f' % (wl, what, k + whose, np.mean(t[q]), min(t[q]), max(t[q])))
        grad, bwd = sum(np.mean(x) for x in t[1:1 + n_own]), sum(np.mean(x) for x in t[1 + n_own:])
        out.append('  %-5s %-12s entropy-gradient call %.3f ms: x%.2f of the backward call (%.3f ms); per kernel against the backward '
                   'call: %s' % (wl, what, grad, grad / bwd, bwd,
                                 ', '.join('%s x%.2f' % (k.replace('smm_align_graph_', ''), np.mean(x) / bwd) for k, x in zip(CALL[1:1 + n_own], t[1:1 + n_own]))))
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


def sub(keep, graphs):
    """The launch of the videos `keep`: batch, graphs, endpen rows, the forward call's workspace."""
    batch = ops.Batch(B.lengths[keep], B.n_states, B.k_rows, c_max=B.c_max, frame_offset=B.frame_offset[keep], group=group[keep],
                      kp=kp[keep], t_max=B.t_max, total_frames=B.total_frames)
    gs = [graphs[i] for i in keep]
    ep = None if pc.endpen is None else pc.endpen[torch.as_tensor(keep, device=dev)].contiguous()
    off = np.concatenate([[0], np.cumsum([len(g) for g in gs])]).astype(np.int64)
    ws = torch.empty(ops.align_graph_logz_workspace_bytes(batch, off), dtype=torch.uint8, device=dev)
    return dict(batch=batch, graphs=gs, endpen=ep, ws=ws, staged=None)


def forward_gradient_backward(s):
    """-> (log Z_g, the entropy-gradient call's result, the backward call's, the events between the three calls)."""
    z = ops.align_graph_logz(s['batch'], elp, *tabs, s['graphs'], endpen=s['endpen'], ws=s['ws'], staged=s['staged'])
    s['staged'] = z['_staged']
    mids = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    mids[0].record()
    h = ops.align_graph_entropy_bwd(s['batch'], elp, *tabs, s['graphs'], z['logz'], endpen=s['endpen'], ws=s['ws'], staged=s['staged'])
    mids[1].record()
    g = ops.align_graph_logz_bwd(s['batch'], elp, *tabs, s['graphs'], z['logz'], endpen=s['endpen'], ws=s['ws'], staged=s['staged'])
    return z['logz'], h, g, mids


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

times = [[] for _ in range(9)]
total, gmax = [0.0] * 3, [0.0] * 3
for rep in range(REPS + 1):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    mids, outs = [], []
    e[0].record()
    for q, s in enumerate((s1, s2, s3)):
        z, h, g, mid = forward_gradient_backward(s)
        e[q + 1].record()
        mids.append(mid)
        outs.append((z, h, g))
    torch.cuda.synchronize()
    if rep == 0:                                                  # the warm-up repetition: the values, once
        for q, (z, h, g) in enumerate(outs):
            s = (s1, s2, s3)[q]
            assert ops.error_flag(s['batch'], h) == 0 and bool(torch.isfinite(z).all()) and bool(torch.isfinite(h['value']).all())
            assert bool(torch.isfinite(h['elp']).all())
            total[q], gmax[q] = float(h['value'].sum()), float(h['elp'].abs().max())
        continue
    for q in range(3):
        times[3 * q].append(e[q].elapsed_time(mids[q][0]))
        times[3 * q + 1].append(mids[q][0].elapsed_time(mids[q][1]))
        times[3 * q + 2].append(mids[q][1].elapsed_time(e[q + 1]))
med = [float(np.median(x)) for x in times]
m3 = np.array([len(g) for g in s3['graphs']])
what = ['(i) chains', '(ii) an optional entry between every two and at both ends (median %d nodes)' % int(np.median(ms2)),
        '(iii) the trie of the transcript and 7 perturbed copies (median %d nodes)' % int(np.median(m3))]
line = ('%s: %d videos, %d frames, longest %d; Viterbi transcripts: median %d, longest %d entries; one forward call, the '
        'entropy-gradient call, the backward call'
        % (workload, pc.n_videos, pc.n_frames, int(max(pc.lengths)), int(np.median(ms1)), int(ms1.max())))
for q, s in enumerate((s1, s2, s3)):
    line += ('; %s, %d videos: forward %.3f ms, entropy gradient %.3f ms (x%.2f of the backward call), backward %.3f ms; sum of H '
             '%.6f nats, max |dH / d elp| %.3e'
             % (what[q], len(s['graphs']), med[3 * q], med[3 * q + 1], med[3 * q + 1] / med[3 * q + 2], med[3 * q + 2], total[q], gmax[q]))
line += ' (medians of %d)' % REPS
print(line)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              'profiles', 'align_graph_entropy_grad_kernel_times.txt')
with open(out_path, 'a') as f:
    f.write(line + '\n')
