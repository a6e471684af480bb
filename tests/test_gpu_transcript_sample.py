"""Alignments sampled from the transcript-graph posterior on the GPU (smm_align_graph_sample_f64) against the enumeration of
tests/transcript_sample_ref.py, the fp64 numpy posteriors of tests/transcript_graph_ref.py and the library's own node / end
posteriors.

Bars: test_gpu_sample.py's.  Exact distribution: total variation <= 0.01 at 100 000 draws, where the enumerated posterior
itself keeps a perfect sampler's expected TV <= 0.007 (test_transcript_sample_host.py checks that of these very cases without
a GPU); nothing outside the enumeration and nothing below 1e-12 drawn; every distinct sample's logp within
1e-6 max(1, |log Z|) of its enumerated score minus log Z.  Frequencies at real sizes: at most 2 * expected + 10 entries outside
6 sqrt(p (1 - p) / n) + 2e-3 (``_exceedances``)."""
import functools

import numpy as np
import pytest
import torch

import align_graph_ref as AG
import test_gpu_transcript_graph as GT
import transcript_graph_ref as TG
import transcript_sample_ref as TS
from test_gpu_transcript_graph import Case, _lists, _ops, _tables, _tuple

pytestmark = pytest.mark.gpu
N_EXACT = 100000
LOGP_BAR = 1e-6


# ------------------------------------------------------------------------------------------------ launching
def _node_offsets(case):
    return np.concatenate([[0], np.cumsum([len(g) for g in case.graphs])]).astype(np.int64)


def _forward(case, fill=None):
    """The forward launch on a workspace of exactly the size the header asks for (``fill``: every byte set to it first)."""
    ops = _ops()
    batch, d = case.device_inputs()
    ws = torch.empty(ops.align_graph_logz_workspace_bytes(batch, _node_offsets(case)), dtype=torch.uint8, device='cuda:0')
    if fill is not None:
        ws.fill_(fill)
    fwd = ops.align_graph_logz(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, endpen=d['endpen'], ws=ws)
    assert fwd['ws'] is ws
    return batch, d, fwd


def _draw(case, batch, d, fwd, n, seed=0, **kw):
    return _ops().align_graph_sample(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, fwd['logz'], n, seed=seed,
                                     endpen=d['endpen'], ws=fwd['ws'], staged=fwd['_staged'], **kw)


def _host(out):
    return dict(spans=out['spans'].cpu().numpy(), labels=out['labels'].cpu().numpy(), logp=out['logp'].cpu().numpy(),
                n_segs=out['n_segs'].cpu().numpy(), used=[u.cpu().numpy() for u in out['used']])


def _sample(case, n, seed=0, fill=None):
    """-> (numpy outputs, logZ_g [b] numpy, error word)."""
    batch, d, fwd = _forward(case, fill)
    out = _draw(case, batch, d, fwd, n, seed)
    return _host(out), fwd['logz'].cpu().numpy(), _ops().error_flag(batch, out)


def _same(a, b):
    return (all(torch.equal(a[k], b[k]) for k in ('spans', 'labels', 'n_segs')) and torch.equal(torch.cat(a['used'], 1), torch.cat(b['used'], 1))
            and torch.equal(a['logp'].view(torch.int64), b['logp'].view(torch.int64)))


def _agree(case, h, i):
    """spans, labels, n_segs and used of video i agree with each other in every sample (a video with an alignment): as many
    segment starts as used nodes as n_segs, the first at 0, the EOS id (local id C) at T and -1 behind it, the frame labels
    the spans filled forward.  -> (rows [n, T + 1], used [n, M])."""
    T, C = case.lengths[i], case.n_states[case.vids[i][2]]
    rows, used = h['spans'][:, i, :], h['used'][i]
    n = rows.shape[0]
    starts = rows[:, :T] >= 0
    assert starts[:, 0].all() and (rows[:, T] == C).all() and (rows[:, T + 1:] == -1).all()
    assert np.array_equal(starts.sum(1), h['n_segs'][:, i]) and np.array_equal(used.sum(1), h['n_segs'][:, i])
    assert set(np.unique(used).tolist()) <= {0, 1}
    at = np.maximum.accumulate(np.where(starts, np.arange(T)[None, :], 0), axis=1)
    filled = rows[np.arange(n)[:, None], at]
    assert np.array_equal(filled, h['labels'][:, case.off[i]:case.off[i + 1]])
    return rows[:, :T + 1], used


def _degenerate(h, case, i):
    """The outputs of a video without an alignment."""
    T = case.lengths[i]
    return ((h['spans'][:, i, :] == -1).all() and (h['labels'][:, case.off[i]:case.off[i] + T] == -1).all()
            and not h['n_segs'][:, i].any() and not h['used'][i].any() and np.isnan(h['logp'][:, i]).all())


def _frame_freq(labels, c):
    return np.stack([(labels == j).mean(0) for j in range(c)], axis=1)


def _exceed(freq, ref, n):
    from test_gpu_sample import _exceedances
    bad, expected = _exceedances(freq, ref, n)
    return bad, expected, float(np.abs(freq - ref).max())


# ------------------------------------------------------------------------------------------------ 1. exact distribution
@functools.lru_cache(None)
def exact_cases():
    """k_rows 4: a chain of 3, a from_optional graph, a trie of 3 candidates one of which is a prefix of another (an end node
    with a successor), a diamond with equal arms (ambiguous: alignments count per path), a random graph with dead nodes, and
    two starts / two ends under end penalties; T in {5, 6, 7}, 3 classes.  k_rows 8 > T: the chain and the trie again.  Scales
    and seeds are chosen so that the enumeration alone keeps a perfect sampler's expected TV under 0.007
    (test_transcript_sample_host.py)."""
    G = _ops().TranscriptGraph
    rng = np.random.default_rng(2026)
    C = 3
    while True:                                                  # a random graph with a node on no start -> end path
        rg = TG.random_graph(rng, 6, C, p_edge=0.4)
        on = {m for p in AG.paths(*[np.asarray(x) for x in rg[1:]]) for m in p}
        if 0 < len(on) < 6 and TG.has_alignment_by_count(5, C, rg, 4):
            break
    named = [('chain of 3', G.chain([0, 2, 1]), 7),
             ('from_optional', G.from_optional([0, 1, 2, 0], [1, 0, 1, 0]), 6),
             ('trie, a prefix among 3', G.from_candidates([[0, 1], [0, 1, 2], [2, 0]]), 6),
             ('diamond, equal arms', _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 1, 2]), 7),
             ('random graph, dead nodes', G(*rg), 5),
             ('two starts, two ends, endpen', _lists(5, [[], [], [0, 1], [2], [2]], [0, 1], [3, 4], ids=[0, 1, 2, 0, 1]), 6)]
    tab = _tables(rng, C, 4, 1.2)
    endpen = np.zeros((len(named), C))
    endpen[-1] = rng.normal(size=C) * 2
    short = Case([(rng.normal(size=(T, C)) * 1.2, g, 0) for _, g, T in named], [tab], 4, endpen=endpen)
    tab8 = _tables(rng, C, 8, 1.5)
    long = Case([(rng.normal(size=(6, C)) * 1.5, named[0][1], 0), (rng.normal(size=(5, C)) * 1.5, named[2][1], 0)], [tab8], 8)
    return [('k_rows 4', short, [n for n, _, _ in named]), ('k_rows 8 > T', long, [named[0][0], named[2][0]])]


def enumerated(case, i):
    """-> (alignments {key: score}, log Z_g, {key: probability}) of video i of a case."""
    e, g, j = case.vids[i]
    t = case.tabs[j]
    aligns = TS.enumerate_alignments(e, _tuple(g), t['trans'], t['init'], t['len'], case.kp(i), case.ep(i))
    return (aligns,) + TS.posterior(aligns)


@pytest.mark.parametrize('which', [0, 1], ids=['k_rows4', 'k_rows8'])
def test_exact_distribution_on_tiny_graphs(which):
    _, case, names = exact_cases()[which]
    n = N_EXACT
    h, z, err = _sample(case, n, seed=7)
    assert err == 0
    for i, name in enumerate(names):
        aligns, lz, p = enumerated(case, i)
        T, graph, kp = case.lengths[i], _tuple(case.graphs[i]), case.kp(i)
        C, M = case.n_states[0], len(case.graphs[i])
        assert np.isfinite(lz) and abs(z[i] - lz) <= 1e-6 * max(1.0, abs(lz)), name
        assert TS.expected_tv(p.values(), n) <= 0.007, name
        rows, used = _agree(case, h, i)
        uniq, first, cnt = np.unique(np.concatenate([used, rows], axis=1), axis=0, return_index=True, return_counts=True)
        tol = LOGP_BAR * max(1.0, abs(lz))
        freq = {}
        for row, j, c in zip(uniq, first, cnt):
            key = TS.alignment_of(graph, T, kp, row[:M], row[M:], eos=C)
            assert key in p, (name, key)                         # nothing outside the enumeration
            assert p[key] >= 1e-12, (name, key, p[key])
            freq[key] = c / n
            assert abs(h['logp'][j, i] - (aligns[key] - lz)) <= tol, (name, key, h['logp'][j, i], aligns[key] - lz)
        tv = 0.5 * sum(abs(freq.get(k, 0.0) - pk) for k, pk in p.items())
        print('\n[transcript-sample] %-30s %3d alignments, %3d drawn, TV %.4f (bar 0.01, a perfect sampler %.4f)'
              % (name, len(p), len(freq), tv, TS.expected_tv(p.values(), n)))
        assert tv <= 0.01, (name, tv)
    if which == 0:                                               # the ambiguous diamond: both arms are drawn, as two alignments
        arms = h['used'][3][:, 1:3]
        assert (arms.sum(1) == 1).all() and 0 < arms[:, 0].sum() < n


# ------------------------------------------------------------------------------------------------ 2. the span draw's sixteen slots
@functools.lru_cache(None)
def _k1024():
    rng = np.random.default_rng(5)
    C, K, T = 4, 1024, 1500
    G = _ops().TranscriptGraph
    tab = _tables(rng, C, K, 0.3)
    case = Case([(rng.normal(size=(T, C)) * 0.05, G.chain([1, 3]), 0), (rng.normal(size=(T, C)) * 0.05, G.chain([0, 2, 1]), 0)], [tab], K)
    occ = [TG.forward_backward(e, _tuple(g), tab['trans'], tab['init'], tab['len'], case.kp(i))['elp']
           for i, (e, g, _) in enumerate(case.vids)]
    return case, occ


def test_span_lengths_up_to_1023_match_the_frame_posteriors():
    """k_rows 1024, T = 1500, a chain of 2 and a chain of 3: every one of the sixteen candidate slots of a lane holds span
    lengths with mass.  256 samples per video against the frame occupancy of the fp64 numpy forward-backward."""
    case, occ = _k1024()
    n = 256
    h, z, err = _sample(case, n, seed=3)
    assert err == 0 and np.isfinite(h['logp']).all()
    longest = 0
    for i, T in enumerate(case.lengths):
        rows, _ = _agree(case, h, i)
        for row in rows:
            longest = max(longest, int(np.diff(np.flatnonzero(row >= 0)).max()))
        bad, expected, worst = _exceed(_frame_freq(h['labels'][:, case.off[i]:case.off[i + 1]], 4), occ[i], n)
        print('\n[transcript-sample] k1024 video %d: %d entries outside the bound (%.1f expected), worst |freq - p| %.3f'
              % (i, bad, expected, worst))
        assert bad <= 2 * expected + 10, (i, bad, expected, worst)
    assert 64 * 15 < longest <= 1023, longest                   # (the last slot was drawn from; no span beyond the limit)


# ------------------------------------------------------------------------------------------------ 3. the node draws' four slots
def _wide(kind, rng):
    M = 256
    ids = rng.integers(0, 3, M)
    if kind == 'fan':                                            # 255 start nodes that all precede one end node
        return _lists(M, [[] for _ in range(M - 1)] + [list(range(M - 1))], list(range(M - 1)), [M - 1], ids=ids)
    return _lists(M, [[]] + [[m - 1] for m in range(1, M)], list(range(M)), list(range(M)), ids=ids)   # every run of the chain


@pytest.mark.parametrize('kind', ['fan', 'runs'])
def test_256_nodes_match_the_node_and_end_posteriors(kind):
    """M = 256, T = 10, k_rows 10: the end draw and the predecessor draw over all four candidate slots and all eight mask
    words.  4096 samples: the frequency of every node on the path and as its end against smm_align_graph_logz_bwd_f64's
    node_prob / end_prob."""
    ops = _ops()
    rng = np.random.default_rng(41)
    C, K, T, n = 3, 10, 10, 4096
    tab = _tables(rng, C, K, 0.5)
    case = Case([(rng.normal(size=(T, C)) * 0.3, _wide(kind, rng), 0)], [tab], K)
    batch, d, fwd = _forward(case)
    out = _draw(case, batch, d, fwd, n, seed=9)
    h = _host(out)
    assert ops.error_flag(batch, out) == 0 and np.isfinite(h['logp']).all()
    g = ops.align_graph_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, fwd['logz'], endpen=d['endpen'],
                                 ws=fwd['ws'], staged=fwd['_staged'], want_node_prob=True, want_end_prob=True)
    p_used, p_end = g['node_prob'][0].cpu().numpy(), g['end_prob'][0].cpu().numpy()
    _, used = _agree(case, h, 0)
    last = 255 - np.argmax(used[:, ::-1], axis=1)
    f_end = np.bincount(last, minlength=256) / n
    for what, freq, ref in (('used', used.mean(0), p_used), ('end', f_end, p_end)):
        bad, expected, worst = _exceed(freq, ref, n)
        print('\n[transcript-sample] M = 256 %s, %s: %d outside (%.1f expected), worst %.3f, %d nodes drawn'
              % (kind, what, bad, expected, worst, int((freq > 0).sum())))
        assert bad <= 2 * expected + 10, (kind, what, bad, expected, worst)
    if kind == 'fan':
        assert (last == 255).all() and (used.sum(1) == 2).all()
        first = np.argmax(used, axis=1)
        assert all(((first >> 6) == q).any() for q in range(4))  # a start node from every slot of the predecessor draw
    else:
        assert all(((last >> 6) == q).any() for q in range(4))   # an end node from every slot of the end draw


# ------------------------------------------------------------------------------------------------ 4. ranges
def test_reads_stay_inside_the_recorded_ranges():
    """The workspace holds 0xFF bytes (NaNs) wherever the forward kernel does not write.  A graph with dead nodes and skipped
    path lengths, and a chain with T == M: its one alignment is drawn every time, with logp 0."""
    ops = _ops()
    rng = np.random.default_rng(17)
    C, K = 3, 4
    tab = _tables(rng, C, K, 1.5)
    G = ops.TranscriptGraph
    gap_dead = _lists(8, [[], [0], [1], [2], [3], [0, 4], [], [6]], [0], [5], ids=[0, 1, 2, 0, 1, 2, 1, 0])   # paths of 2 or 6; 6, 7 dead
    full = G.chain([0, 1, 2, 0, 1, 2])
    case = Case([(rng.normal(size=(7, C)), gap_dead, 0), (rng.normal(size=(6, C)), full, 0),
                 (rng.normal(size=(4, C)), gap_dead, 0)], [tab], K, kps=[3, 4, 3])
    n = 512
    h, z, err = _sample(case, n, seed=1, fill=0xFF)
    assert err == 0 and np.isfinite(z).all() and np.isfinite(h['logp']).all()
    for i in range(3):
        rows, used = _agree(case, h, i)
        aligns, lz, p = enumerated(case, i)
        for row, u, lp in zip(rows, used, h['logp'][:, i]):
            key = TS.alignment_of(_tuple(case.graphs[i]), case.lengths[i], case.kp(i), u, row, eos=C)
            assert key in p and abs(lp - (aligns[key] - lz)) <= LOGP_BAR * max(1.0, abs(lz)), (i, key)
        assert i == 1 or not used[:, 6:].any()                   # (the dead nodes)
    batch, d = case.device_inputs()
    best = ops.align_graph(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, endpen=d['endpen'])
    lab = best['labels'].cpu().numpy()[case.off[1]:case.off[2]]
    assert (h['labels'][:, case.off[1]:case.off[2]] == lab[None, :]).all() and (h['used'][1] == 1).all()
    assert np.abs(h['logp'][:, 1]).max() <= LOGP_BAR * max(1.0, abs(z[1]))


# ------------------------------------------------------------------------------------------------ 5. degenerate videos
def test_degenerate_videos_beside_healthy_ones():
    """Behind two healthy videos: no start -> end path, M > T, every path cut by -inf entries -- log Z_g = -inf: spans and
    labels -1, n_segs 0, used 0, logp NaN, the error word clear -- and, in a second launch, a NaN in elp: the same outputs and
    the error word.  The healthy videos' samples are those of a launch without the others, bit for bit."""
    ops = _ops()
    rng = np.random.default_rng(23)
    C, K = 4, 6
    tab = _tables(rng, C, K, 1.5)
    tab['trans'][1, 0] = tab['trans'][2, 0] = -np.inf             # 0 -> 1 and 0 -> 2: both arms of the diamond
    G = ops.TranscriptGraph
    healthy = [(rng.normal(size=(9, C)), G.chain([1, 2, 3]), 0),
               (rng.normal(size=(10, C)), G.from_candidates([[3, 2], [3, 0, 3], [1, 0]]), 0)]
    no_path = (rng.normal(size=(8, C)), _lists(3, [[], [0], []], [0], [2], ids=[0, 1, 2]), 0)
    too_many = (rng.normal(size=(5, C)), G.chain([0, 3, 2, 1, 3, 2, 0]), 0)
    cut = (rng.normal(size=(10, C)), _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 2, 3]), 0)
    bad_elp = rng.normal(size=(8, C))
    bad_elp[3, 1] = np.nan
    nan_video = (bad_elp, G.chain([1, 2]), 0)
    n = 64
    alone, _, err = _sample(Case(healthy, [tab], K), n, seed=5)
    assert err == 0
    case = Case(healthy + [no_path, too_many, cut], [tab], K)
    h, z, err = _sample(case, n, seed=5)
    assert err == 0 and np.isfinite(z[:2]).all() and (z[2:] == -np.inf).all()
    case2 = Case(healthy + [no_path, nan_video, cut], [tab], K)
    h2, z2, err2 = _sample(case2, n, seed=5)
    assert err2 != 0 and np.isnan(z2[3]) and (z2[[2, 4]] == -np.inf).all()
    for hh, cc in ((h, case), (h2, case2)):
        for i in (2, 3, 4):
            assert _degenerate(hh, cc, i), i
        for i in (0, 1):
            _agree(cc, hh, i)
            assert np.isfinite(hh['logp'][:, i]).all()
            assert np.array_equal(hh['spans'][:, i, :], np.pad(alone['spans'][:, i, :], ((0, 0), (0, hh['spans'].shape[2] - alone['spans'].shape[2])),
                                                               constant_values=-1))
            assert np.array_equal(hh['labels'][:, cc.off[i]:cc.off[i + 1]], alone['labels'][:, cc.off[i]:cc.off[i + 1]])
            assert np.array_equal(hh['used'][i], alone['used'][i])
            assert np.array_equal(hh['logp'][:, i].view(np.int64), alone['logp'][:, i].view(np.int64))


# ------------------------------------------------------------------------------------------------ 6. determinism
def test_determinism_and_independence_of_the_backward_call():
    """The same seed gives the same bits; the first 4 of 16 samples are a call's 4; another seed differs; samples taken after
    smm_align_graph_logz_bwd_f64 has run on the workspace are those taken before it."""
    ops = _ops()
    case, _ = GT._ragged(kind='trie')
    batch, d, fwd = _forward(case)
    a = _draw(case, batch, d, fwd, 16, seed=123)
    b = _draw(case, batch, d, fwd, 16, seed=123)
    c = _draw(case, batch, d, fwd, 4, seed=123)
    e = _draw(case, batch, d, fwd, 16, seed=124)
    assert ops.error_flag(batch, a) == 0 and bool(torch.isfinite(a['logp']).all())
    assert _same(a, b)
    assert all(torch.equal(a[k][:4], c[k]) for k in ('spans', 'labels', 'logp', 'n_segs'))
    assert torch.equal(torch.cat(a['used'], 1)[:4], torch.cat(c['used'], 1))
    assert not torch.equal(a['labels'], e['labels'])
    g = ops.align_graph_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, fwd['logz'], grad_logz=d['u'],
                                 endpen=d['endpen'], ws=fwd['ws'], staged=fwd['_staged'], want_node_prob=True, want_end_prob=True)
    after = _draw(case, batch, d, fwd, 16, seed=123)
    assert _same(a, after)
    # ... and the backward call is not disturbed by the sampler either: a fresh forward + backward gives its bits
    _, d2, fwd2 = _forward(case)
    g2 = ops.align_graph_logz_bwd(batch, d2['elp'], d2['trans'], d2['init'], d2['len'], case.graphs, fwd2['logz'], grad_logz=d2['u'],
                                  endpen=d2['endpen'], ws=fwd2['ws'], staged=fwd2['_staged'], want_node_prob=True, want_end_prob=True)
    assert all(torch.equal(g[k], g2[k]) for k in ('elp', 'trans', 'init', 'len'))


def test_forward_and_sampler_capture_into_a_hip_graph():
    """Forward + sampler captured once with ``staged=`` and replayed on fresh inputs of the ragged shape: the replay
    reproduces the eager pair on those inputs bit for bit."""
    ops = _ops()
    case, _ = GT._ragged(kind='trie')
    batch, d = case.device_inputs()
    graphs = case.graphs
    ws = torch.empty(ops.align_graph_logz_workspace_bytes(batch, _node_offsets(case)), dtype=torch.uint8, device='cuda:0')
    staged = ops.align_graph_logz(batch, d['elp'], d['trans'], d['init'], d['len'], graphs, endpen=d['endpen'], ws=ws)['_staged']

    def step():
        z = ops.align_graph_logz(batch, d['elp'], d['trans'], d['init'], d['len'], graphs, endpen=d['endpen'], ws=ws,
                                 staged=staged)['logz']
        s = ops.align_graph_sample(batch, d['elp'], d['trans'], d['init'], d['len'], graphs, z, 8, seed=31, endpen=d['endpen'],
                                   ws=ws, staged=staged)
        return z, s['spans'], s['labels'], s['logp'], s['n_segs'], torch.cat(s['used'], 1)

    step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    fresh, _ = GT._ragged(values=1, kind='trie')
    _, f = fresh.device_inputs()
    for k in ('elp', 'trans', 'init', 'len', 'endpen'):
        d[k].copy_(f[k])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = [v.clone() for v in out]
    eager = step()
    torch.cuda.synchronize()
    for name, a, e in zip(('logz', 'spans', 'labels', 'logp', 'n_segs', 'used'), got, eager):
        assert torch.equal(a, e), name
    assert bool(torch.isfinite(got[3]).all())


# ------------------------------------------------------------------------------------------------ 7. module, packed, model
def _runs(seq):
    seq = np.asarray(seq)
    return seq[np.concatenate([[True], seq[1:] != seq[:-1]])].tolist()


def _keeps_mandatory(transcript, optional, runs):
    """``runs`` (the label runs of a sample) spell ``transcript`` with only optional entries dropped; kept neighbours of one
    class may have merged into one run."""
    reach = {(0, 0)}
    for i, (e, opt) in enumerate(zip(transcript, optional)):
        nxt = set()
        for (_, r) in reach:
            if opt:
                nxt.add((i + 1, r))
            if r < len(runs) and runs[r] == e:
                nxt.add((i + 1, r + 1))
            if r > 0 and runs[r - 1] == e:
                nxt.add((i + 1, r))
        reach = nxt
    return (len(transcript), len(runs)) in reach


def test_packed_two_groups_return_global_ids():
    """sample_alignments_packed on a packed corpus of two class sets: frame labels in GLOBAL ids that spell each video's
    chain, every node used, finite logp; sample_alignments on one padded batch gives spans of the same classes."""
    from action_segmentation_amd.batching import pack_batches
    G = _ops().TranscriptGraph
    m, rb, vc, _ = GT._module_case()
    x, lengths = rb.features, rb.lengths.tolist()
    vc2 = [1, 3, 5]
    batches = [dict(task_name=['a'] * 2, task_indices=[torch.tensor(vc)] * 2, lengths=torch.tensor(lengths[:2]),
                    features=x[:2, :max(lengths[:2])].contiguous(), video_name=['a0', 'a1']),
               dict(task_name=['b'], task_indices=[torch.tensor(vc2)], lengths=torch.tensor(lengths[2:]),
                    features=x[2:, :lengths[2]].contiguous(), video_name=['b0'])]
    pc = pack_batches(batches, torch.device('cuda:0'), m.max_k)
    chains = {'a0': [4, 0, 2, 5, 0], 'a1': [5, 2, 4], 'b0': [3, 1, 5, 3]}
    graphs = [G.chain(chains[name]) for name in pc.video_names]
    n = 32
    lab, logp, used = m.sample_alignments_packed(pc, graphs, n, seed=4)
    lab = lab.cpu().numpy()
    assert lab.shape == (n, pc.batch.total_frames) and bool(torch.isfinite(logp).all()) and logp.shape == (n, 3)
    for name, o, t, u in zip(pc.video_names, pc.frame_offset, pc.lengths, used):
        assert bool((u == 1).all()) and u.shape == (n, len(chains[name]))
        for s in range(n):
            assert _runs(lab[s, o:o + t]) == chains[name], (name, s)
    assert len({tuple(r) for r in lab.tolist()}) > 1             # (boundaries vary between the samples)
    dev = torch.device('cuda:0')
    sp, lp, us = m.sample_alignments(x[:2].to(dev), rb.lengths[:2].to(dev), [torch.tensor(vc)] * 2,
                                     [G.chain(chains['a0']), G.chain(chains['a1'])], n_samples=5, seed=4)
    assert sp.shape == (5, 2, x.shape[1] + 1) and not sp.is_cuda and bool(torch.isfinite(lp).all())
    for i, name in enumerate(('a0', 'a1')):
        for s in range(5):
            row = sp[s, i, :lengths[i]].numpy()
            assert row[row >= 0].tolist() == chains[name] and int(sp[s, i, lengths[i]]) == m.n_classes


def test_model_layer_candidates_and_optional_classes():
    """SemiMarkovModel.sample_candidates: the frequencies of the drawn candidate index against candidate_posteriors (4096
    samples, 4 candidates one of which comes twice: the repeat is never drawn), the labels spell the drawn candidate.
    sample_alignments with optional_classes drops only optional entries."""
    from action_segmentation_amd import ops, synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts
    data = synth.SynthDatasplit('tiny', seed=11)
    fitted = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    fitted.fit(data, use_labels=True)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=True, batch_size=2), data)
    model.model.load_state_dict(fitted.model.state_dict(), strict=False)
    model.model.cuda()
    pc = model.prepare(data)
    t = pc.tables
    elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
    out = ops.viterbi(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    names = list(pc.video_names)
    tr = dict(zip(names, ([int(v) for v in a] for a in spans_to_transcripts(out['spans'], pc.lengths))))
    cands = {v: [a, a[:-1] if len(a) > 1 else a + a, a, a + a[-1:]] for v, a in tr.items()}
    n = 4096
    labels, chosen = model.sample_candidates(data, cands, n, seed=2)
    post = model.candidate_posteriors(data, cands)
    freq = np.stack([np.bincount(chosen[v], minlength=4) / n for v in names])
    ref = np.stack([post[v] for v in names])
    assert (freq[:, 2] == 0).all()                               # the repeated candidate maps to its first index
    bad, expected, worst = _exceed(freq, ref, n)
    print('\n[transcript-sample] candidates: %d outside (%.1f expected), worst %.3f' % (bad, expected, worst))
    assert bad <= 2 * expected + 10, (bad, expected, worst)
    for v, T in zip(names, pc.lengths):
        assert labels[v].shape == (n, T) and chosen[v].shape == (n,) and chosen[v].dtype == np.int64
        for s in range(0, n, 97):
            assert _runs(labels[v][s]) == _runs(cands[v][int(chosen[v][s])]), (v, s)
    # optional background: every sample keeps the mandatory entries, in order
    bg = set(int(c) for c in data.corpus._background_indices)
    got = model.sample_alignments(data, tr, 16, seed=3, optional_classes=bg)
    plain = model.sample_alignments(data, tr, 16, seed=3)
    dropped = 0
    for v in names:
        opt = [c in bg for c in tr[v]]
        for s in range(16):
            runs = _runs(got[v][s])
            assert _keeps_mandatory(tr[v], opt, runs), (v, s, tr[v], runs)
            dropped += len(runs) < len(_runs(tr[v]))
            assert _runs(plain[v][s]) == _runs(tr[v]), (v, s)
    print('\n[transcript-sample] optional background: %d of %d samples drop an entry' % (dropped, 16 * len(names)))
