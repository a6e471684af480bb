"""Transcript-graph likelihood (forward + backward) on a bench corpus, on scripts/prof_align_graph.py's three workloads, timed
as that script times (HIP events around the calls, medians of 5; the graphs, ids and flags are on the device from a first call
wherever the entry point can take them staged; run under `rocprofv3 --kernel-trace --stats` for the per-kernel times):
  (i)   every video's own Viterbi transcript as a chain graph, through smm_align_graph_logz_f64 / _bwd_f64, beside
        smm_align_logz_f64 / _bwd_f64 on the same inputs;
  (ii)  the same transcripts with an optional entry of a random class between every two entries and at both ends
        (M -> 2 M + 1) as a graph, beside smm_align_opt_logz_f64 / _bwd_f64 on the same transcripts and flags;
  (iii) per video the trie of its own transcript and 7 perturbed copies (one entry replaced or dropped each): one forward and
        one backward call on the trie beside the 8 smm_align_logz_f64 / _bwd_f64 pairs they replace.
Every repetition, the warm-up one included, issues the same kernels in the same order, which is how the second mode tells the
launches of one kernel apart.  The summary line is printed and appended to profiles/align_graph_logz_kernel_times.txt (or to
the file given as the second argument).
usage: python scripts/prof_align_graph_logz.py [cfg3|cfg2|cfg4|refdef] [out.txt]
       python scripts/prof_align_graph_logz.py --trace KERNEL_TRACE.csv     (the per-kernel table of a traced run)"""
import csv
import os
import sys

import numpy as np

REPS = 5
# the kernels of one repetition in launch order: (workload, what, kernel names)
LOGZ = ['smm_align_logz_fwd_kernel', 'smm_align_logz_bwd_kernel', 'smm_align_logz_occ_kernel', 'smm_align_logz_glen_kernel',
        'smm_align_logz_reduce_kernel', 'smm_align_logz_counts_kernel']
TAIL = ['smm_align_opt_logz_occ_kernel', 'smm_align_opt_logz_glen_kernel', 'smm_align_opt_logz_reduce_kernel']
OPT = ['smm_align_opt_logz_fwd_kernel', 'smm_align_opt_logz_bwd_kernel'] + TAIL
GRAPH = ['smm_align_graph_logz_fwd_kernel', 'smm_align_graph_logz_bwd_kernel'] + TAIL
ORDER = [('(i)', 'align_logz', LOGZ), ('(i)', 'align_graph_logz, chains', GRAPH), ('(ii)', 'align_opt_logz, 2 M + 1', OPT),
         ('(ii)', 'align_graph_logz, 2 M + 1', GRAPH), ('(iii)', 'align_logz, 8 launch sets', LOGZ * 8),
         ('(iii)', 'align_graph_logz, tries', GRAPH)]


def summarize(path):
    """The kernel trace of one run -> per workload and entry point the time of each kernel (8 launches of one kernel added),
    avg / min / max over the repetitions after the warm-up one, and the ratios graph / family member."""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r['Kernel_Name'].split('(')[0]
            if name.startswith('smm_align_'):
                rows.append((int(r['Start_Timestamp']), name, (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e6))
    rows.sort()
    seq = [k for _, _, ks in ORDER for k in ks]
    assert len(rows) == (REPS + 1) * len(seq), (len(rows), len(seq))
    table = {}
    for rep in range(1, REPS + 1):
        at = rep * len(seq)
        for wl, what, ks in ORDER:
            per = {}
            for k in ks:
                assert rows[at][1] == k, (rows[at], k)
                per[k] = per.get(k, 0.0) + rows[at][2]
                at += 1
            for k, v in per.items():
                table.setdefault((wl, what, k), []).append(v)
            table.setdefault((wl, what, 'all kernels'), []).append(sum(per.values()))
    out = []
    for wl, what, ks in ORDER:
        for k in list(dict.fromkeys(ks)) + ['all kernels']:
            v = table[(wl, what, k)]
            out.append('  %-5s %-28s %-36s avg %.3f ms  min %.3f  max %.3f' % (wl, what, k, np.mean(v), min(v), max(v)))
    for wl, (base, graph) in (('(i)', (0, 1)), ('(ii)', (2, 3)), ('(iii)', (4, 5))):
        b, g = ORDER[base], ORDER[graph]
        pairs = [('forward', b[2][0], g[2][0]), ('backward', b[2][1], g[2][1]), ('all kernels', 'all kernels', 'all kernels')]
        out.append('  %-5s graph / %s: ' % (wl, b[1]) + ', '.join(
            '%s x%.2f' % (n, np.mean(table[(wl, g[1], kg)]) / np.mean(table[(wl, b[1], kb)])) for n, kb, kg in pairs))
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
    """The launch of the videos `keep`: batch, graphs, endpen rows, a workspace large enough for every entry point."""
    batch = ops.Batch(B.lengths[keep], B.n_states, B.k_rows, c_max=B.c_max, frame_offset=B.frame_offset[keep], group=group[keep],
                      kp=kp[keep], t_max=B.t_max, total_frames=B.total_frames)
    gs = [graphs[i] for i in keep]
    ep = None if pc.endpen is None else pc.endpen[torch.as_tensor(keep, device=dev)].contiguous()
    off = np.concatenate([[0], np.cumsum([len(g) for g in gs])]).astype(np.int64)
    ws = torch.empty(max(ops.align_graph_logz_workspace_bytes(batch, off), ops.align_opt_logz_workspace_bytes(batch, off)),
                     dtype=torch.uint8, device=dev)
    return dict(batch=batch, graphs=gs, keep=keep, endpen=ep, ws=ws, staged=None, opt_staged=None)


def graph(s):
    out = ops.align_graph_logz(s['batch'], elp, *tabs, s['graphs'], endpen=s['endpen'], ws=s['ws'], staged=s['staged'])
    s['staged'] = out['_staged']
    g = ops.align_graph_logz_bwd(s['batch'], elp, *tabs, s['graphs'], out['logz'], endpen=s['endpen'], ws=s['ws'],
                                 staged=s['staged'])
    return out['logz'], g


def logz(s, transcripts):
    out = ops.align_logz_ex(s['batch'], elp, *tabs, [transcripts[i] for i in s['keep']], endpen=s['endpen'], ws=s['ws'])
    g = ops.align_logz_bwd(s['batch'], elp, *tabs, out['transcript'], out['logz'], endpen=s['endpen'], ws=s['ws'])
    return out['logz'], g


def opt_logz(s, transcripts, flags):
    ids, fl = [transcripts[i] for i in s['keep']], [flags[i] for i in s['keep']]
    out = ops.align_opt_logz(s['batch'], elp, *tabs, ids, fl, endpen=s['endpen'], ws=s['ws'], staged=s['opt_staged'])
    s['opt_staged'] = out['_staged']
    g = ops.align_opt_logz_bwd(s['batch'], elp, *tabs, ids, fl, out['logz'], endpen=s['endpen'], ws=s['ws'], staged=s['opt_staged'])
    return out['logz'], g


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
per = [[c[j] for c in cands] for j in range(8)]


def rel(x, y):
    x, y = x.cpu().numpy(), y.cpu().numpy()
    fin = np.isfinite(y)
    return float((np.abs(x[fin] - y[fin]) / np.maximum(1.0, np.abs(y[fin]))).max()) if np.array_equal(np.isfinite(x), fin) else np.inf


times = [[] for _ in range(6)]
worst = [0.0, 0.0, 0.0]
for rep in range(REPS + 1):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
    e[0].record()
    z0, _ = logz(s1, tr)
    e[1].record()
    z1, _ = graph(s1)
    e[2].record()
    zo, _ = opt_logz(s2, tr2, fl2)
    e[3].record()
    z2, _ = graph(s2)
    e[4].record()
    each = [logz(s3, per[j])[0] for j in range(8)]
    e[5].record()
    z3, _ = graph(s3)
    e[6].record()
    torch.cuda.synchronize()
    if rep == 0:                                                  # the warm-up repetition: the values, once
        worst = [rel(z1, z0), rel(z2, zo), rel(z3, torch.logsumexp(torch.stack(each), 0))]
        continue
    for q in range(6):
        times[q].append(e[q].elapsed_time(e[q + 1]))
med = [float(np.median(x)) for x in times]
m3 = np.array([len(g) for g in s3['graphs']])
line = ('%s: %d videos, %d frames, longest %d; Viterbi transcripts: median %d, longest %d entries; forward + backward calls; '
        '(i) chains, %d videos: align_logz pair %.3f ms, align_graph_logz pair %.3f ms (x%.2f), logZ rel. diff %.1e; (ii) an '
        'optional entry between every two and at both ends (median %d nodes), %d videos: align_opt_logz pair %.3f ms, '
        'align_graph_logz pair %.3f ms (x%.2f), logZ rel. diff %.1e; (iii) the trie of the transcript and 7 perturbed copies '
        '(median %d nodes), %d videos: 8 align_logz pairs %.3f ms, one align_graph_logz pair %.3f ms (x%.2f), logZ against '
        'their logsumexp rel. diff %.1e (medians of %d)'
        % (workload, pc.n_videos, pc.n_frames, int(max(pc.lengths)), int(np.median(ms1)), int(ms1.max()), len(s1['graphs']),
           med[0], med[1], med[1] / med[0], worst[0], int(np.median(ms2)), len(s2['graphs']), med[2], med[3], med[3] / med[2],
           worst[1], int(np.median(m3)), len(s3['graphs']), med[4], med[5], med[5] / med[4], worst[2], REPS))
print(line)
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                              'profiles', 'align_graph_logz_kernel_times.txt')
with open(out_path, 'a') as f:
    f.write(line + '\n')
