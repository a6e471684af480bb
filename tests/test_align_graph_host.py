"""Host-side checks of the forced alignment to a transcript graph: the reference restatement tests/align_graph_ref.py against
the C twin on the expanded lattice, against tests/align_optional_ref.py on graphs built from optional flags, against
tests/align_ref.py on chains and against a brute force over every path and composition; the rule that decides by counting
whether there is an alignment; ops.TranscriptGraph; the seeds of the GPU test's shapes; the C entry points' refusals (no GPU:
every call is refused before anything is staged) and the Python-level argument checks."""
import ctypes
import re
import os

import numpy as np
import pytest

import align_graph_ref as G
import align_optional_ref as O
import align_ref as R
from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)


def _tables(rng, ties, T, C, kp, with_endpen=None):
    K = kp + int(rng.integers(0, 3))
    if ties:
        draw = lambda *s: rng.integers(-3, 4, size=s).astype(np.float64)
    else:
        draw = lambda *s: rng.normal(size=s) * 3.0
    with_endpen = rng.random() < 0.5 if with_endpen is None else with_endpen
    return dict(elp=draw(T, C), trans=draw(C, C), init=draw(C), len_scores=draw(K, C), kp=kp,
                endpen=rng.integers(-3, 4, size=C).astype(np.float64) if with_endpen else None)


def _random_graph(rng, M, C, density):
    """a random DAG: every pair j < m is an edge with probability `density`; random start and end flags, at least one each"""
    pred = np.tril(rng.random((M, M)) < density, -1)
    start, end = rng.random(M) < 0.3, rng.random(M) < 0.3
    start[int(rng.integers(0, M))] = True
    end[int(rng.integers(0, M))] = True
    return rng.integers(0, C, size=M), pred, start, end


def _case(rng, ties, density, feasible=True):
    """A random video and graph, T < 30, M < 12, kp < 10, C <= 5; with an alignment by counting unless told otherwise."""
    C = int(rng.integers(1, 6))
    for _ in range(10000):
        T, kp, M = int(rng.integers(1, 30)), int(rng.integers(2, 10)), int(rng.integers(1, 12))
        graph = _random_graph(rng, M, C, density)
        if G.feasible_by_count(T, *graph[1:], kp) or not feasible:
            break
    else:
        raise AssertionError("no video with an alignment drawn")
    return dict(_tables(rng, ties, T, C, kp), graph=graph)


def _valid(c, segs):
    """The segments walk a start -> end path of the graph within the span limit."""
    T = c['elp'].shape[0]
    _, pred, start, end = c['graph']
    starts, nodes = [s for s, _ in segs], [j for _, j in segs]
    assert starts[0] == 0 and all(0 < e - s < c['kp'] for s, e in zip(starts, starts[1:] + [T]))
    assert start[nodes[0]] and end[nodes[-1]] and all(pred[m, j] for j, m in zip(nodes, nodes[1:]))


def _score(c, segs):
    """The score of a segmentation, summed term by term."""
    T, a = c['elp'].shape[0], c['graph'][0]
    ends = [s for s, _ in segs[1:]] + [T]
    sc = c['init'][a[segs[0][1]]] + (0.0 if c['endpen'] is None else c['endpen'][a[segs[-1][1]]])
    for i, ((s, j), e) in enumerate(zip(segs, ends)):
        sc += c['elp'][s:e, a[j]].sum() + c['len_scores'][e - s, a[j]]
        if i:
            sc += c['trans'][a[j], a[segs[i - 1][1]]]
    return sc


def test_the_reference_equals_the_twin_on_the_expanded_lattice():
    rng = np.random.default_rng(20261019)
    n = branching = 0
    for i in range(300):
        c = _case(rng, ties=i % 2 == 0, density=(0.15, 0.3, 0.6, 1.0)[(i // 2) % 4])
        best, segs = G.align_graph_ref(**c)
        if segs is None:                                               # (the count rule passed, the path lengths have a gap)
            assert best == -np.inf and G.align_graph_ref(count_rule=False, **c)[0] == -np.inf
            continue
        v, tw = G.twin_align(**c)
        assert best == v and segs == tw, (i, best, v, segs, tw)
        _valid(c, segs)
        branching += len(G.paths(*c['graph'][1:])) > 1
        n += 1
    assert n >= 200 and branching > 100


def test_the_reference_equals_the_optional_reference_on_graphs_from_flags():
    rng = np.random.default_rng(5)
    from action_segmentation_amd import ops
    for i in range(160):
        C, M = int(rng.integers(1, 6)), int(rng.integers(1, 13))
        opt = rng.random(M) < (0.0, 0.3, 0.6, 1.0)[i % 4]
        a = rng.integers(0, C, size=M)
        T, kp = int(rng.integers(1, 40)), int(rng.integers(1, 10))
        t = _tables(rng, i % 2 == 0, T, C, max(kp, 1))
        graph = G.from_optional(a, opt)
        tg = ops.TranscriptGraph.from_optional(a, opt)
        assert all(np.array_equal(x, y) for x, y in zip(graph, (tg.ids, tg.pred, tg.start, tg.end)))
        # the count rules agree, so the precedence of "none" over "error" does
        assert G.feasible_by_count(T, *graph[1:], kp) == O.feasible_by_count(T, opt, kp)
        for count_rule in (True, False):
            assert G.align_graph_ref(graph=graph, count_rule=count_rule, **t) == O.align_optional_ref(a=a, opt=opt, count_rule=count_rule, **t), i
    c = dict(_tables(rng, False, 9, 3, 5), graph=G.from_optional([0, 1, 2], [1, 0, 1]))
    c['elp'][2, 0] = np.nan
    assert np.isnan(G.align_graph_ref(**c)[0])


def test_the_reference_equals_align_ref_on_chains():
    rng = np.random.default_rng(4)
    from action_segmentation_amd import ops
    for i in range(120):
        C, M = int(rng.integers(1, 6)), int(rng.integers(1, 13))
        a = rng.integers(0, C, size=M)
        T, kp = int(rng.integers(1, 40)), int(rng.integers(2, 10))
        t = _tables(rng, i % 2 == 0, T, C, kp)
        tg = ops.TranscriptGraph.chain(a)
        assert all(np.array_equal(x, y) for x, y in zip(G.chain(a), (tg.ids, tg.pred, tg.start, tg.end)))
        best, segs = G.align_graph_ref(graph=G.chain(a), **t)
        closing = 0.0 if t['endpen'] is None else float(t['endpen'][a[-1]])
        want, starts = R.align_ref(t['elp'], a, t['trans'], t['init'], t['len_scores'], kp, closing=closing)
        assert best == want and (segs is None) == (starts is None), i
        if segs is not None:
            assert segs == list(zip(starts, range(M))), i
    t = _tables(rng, False, 6, 3, 4)
    assert G.align_graph_ref(graph=G.chain([0, 9, 0]), **t) == (-np.inf, None)          # an id that is no state


SMALL = {
    # name: (ids, predecessor lists, start nodes, end nodes)
    'diamond': ([0, 1, 2, 0], [[], [0], [0], [1, 2]], [0], [3]),
    'skip edge': ([0, 1, 2, 1, 0], [[], [0], [1], [2], [1, 3]], [0], [4]),
    'trie of 3': ([0, 1, 2, 2, 1, 0], [[], [0], [1], [0], [3], [3]], [0], [2, 4, 5]),
    'two starts, two ends': ([1, 0, 2, 1], [[], [], [0, 1], [1, 2]], [0, 1], [2, 3]),
    'free order': ([0, 1, 2, 2, 1, 0], [[], [0], [1], [0], [3], [2, 4]], [0], [5]),
}


def _small(name):
    ids, preds, start, end = SMALL[name]
    M = len(ids)
    pred = np.zeros((M, M), bool)
    for m, js in enumerate(preds):
        pred[m, js] = True
    return np.array(ids, np.int64), pred, np.isin(np.arange(M), start), np.isin(np.arange(M), end)


@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
@pytest.mark.parametrize('name', list(SMALL))
def test_the_reference_equals_the_brute_force(name, ties):
    """T <= 8, M <= 6: the best of every start -> end path and every composition.  Integer inputs: every score is exact in any
    order, and the reference's segmentation is one of the maximal ones.  Real inputs: a score is a sum of at most
    2 T + 2 M + 2 <= 30 terms of magnitude < 20; compared to 1e-9."""
    rng = np.random.default_rng(12 + ties)
    graph = _small(name)
    n = 0
    for T in range(1, 9):
        for kp in (2, 3, 4, 6):
            c = dict(_tables(rng, ties, T, 3, kp), graph=graph)
            best, segs = G.align_graph_ref(**c)
            want, args = G.brute_force(all_maximal=True, **c)
            assert (segs is None) == (want == -np.inf), (T, kp)
            if segs is None:
                assert best == -np.inf
                continue
            _valid(c, segs)
            if ties:
                assert best == want == _score(c, segs) and segs in args, (T, kp, best, want)
            else:
                assert abs(best - want) < 1e-9 and abs(_score(c, segs) - want) < 1e-9, (T, kp, best, want)
            n += 1
    assert n > 12


def test_the_count_rule_is_the_recursions_own_answer_where_it_says_none():
    """All T <= 10, kp <= 5, random graphs of M <= 7 nodes: where the rule (no path, Lmin > T, kp - 1 < 1, Lmax (kp - 1) < T)
    says "none", the recursion left to itself finds nothing; where the recursion finds something, the rule has let it pass.
    Lmin and Lmax are the extremes over the enumerated paths."""
    rng = np.random.default_rng(2)
    len_scores, trans, init = rng.normal(size=(8, 2)), rng.normal(size=(2, 2)), rng.normal(size=2)
    n_inf = n_fin = n_gap = 0
    for T in range(1, 11):
        elp = rng.normal(size=(T, 2))
        for M in range(1, 8):
            for rep in range(12):
                a, pred, start, end = _random_graph(rng, M, 2, (0.2, 0.5, 0.9)[rep % 3])
                if rep % 4 == 3:
                    start[:] = False if rep % 8 == 3 else start          # (no start node at all / flags as drawn)
                ps = G.paths(pred, start, end)
                L = G.path_lengths(pred, start, end)
                assert (L is None) == (not ps) and (L is None or L == (min(map(len, ps)), max(map(len, ps))))
                for kp in range(1, 6):
                    rule = G.feasible_by_count(T, pred, start, end, kp)
                    assert rule == (bool(ps) and kp >= 2 and L[0] <= T and L[1] * (kp - 1) >= T)
                    best, segs = G.align_graph_ref(elp, (a, pred, start, end), trans, init, len_scores, kp, count_rule=False)
                    exact = any(len(p) <= T <= len(p) * (kp - 1) for p in ps)
                    assert np.isfinite(best) == exact and (rule or not exact), (T, M, kp, best)
                    assert G.align_graph_ref(elp, (a, pred, start, end), trans, init, len_scores, kp)[0] == best
                    n_inf += not rule
                    n_fin += exact
                    n_gap += rule and not exact
    assert n_inf > 500 and n_fin > 500 and n_gap > 0


# ------------------------------------------------------------------------------------------------ ops.TranscriptGraph
def test_from_candidates_is_the_prefix_trie():
    from action_segmentation_amd import ops
    rng = np.random.default_rng(3)
    for _ in range(40):
        cands = [tuple(int(x) for x in rng.integers(0, 3, size=int(rng.integers(1, 6)))) for _ in range(int(rng.integers(1, 9)))]
        g = ops.TranscriptGraph.from_candidates(cands)
        got = {tuple(int(g.ids[m]) for m in p) for p in G.paths(g.pred, g.start, g.end)}
        assert got == set(cands)                                        # every candidate is a path and vice versa
        assert len(G.paths(g.pred, g.start, g.end)) == len(set(cands))  # ... once: identical candidates collapse
        assert len(g) == len({c[:n] for c in cands for n in range(1, len(c) + 1)}) == ops.TranscriptGraph.trie_nodes(cands)
        assert not np.triu(g.pred).any() and (g.pred.sum(1) == ~g.start).all()
        for p in G.paths(g.pred, g.start, g.end):
            seq = tuple(int(g.ids[m]) for m in p)
            assert g.end_candidate[p[-1]] == cands.index(seq)          # the lowest index of that candidate
            used = np.zeros(len(g), np.int32)
            used[list(p)] = 1
            assert g.candidate_of(used) == cands.index(seq)
        assert (g.end_candidate[~g.end] == -1).all() and g.candidate_of(np.zeros(len(g))) == -1
    g = ops.TranscriptGraph.from_candidates([[1, 2, 3], [1, 2], [1, 4, 3], [1, 2, 3]])
    assert list(g.ids) == [1, 2, 3, 4, 3] and list(g.end_candidate) == [-1, 1, 0, -1, 2]
    assert list(g.start) == [True, False, False, False, False] and list(g.end) == [False, True, True, False, True]


def test_mask_packing_and_flags():
    from action_segmentation_amd import ops
    M = 70
    preds = [[j for j in (m - 1, m - 33, m - 65, 0) if 0 <= j < m] for m in range(M)]
    g = ops.TranscriptGraph(np.zeros(M, np.int64), preds, np.arange(M) < 2, np.arange(M) >= M - 3)
    w = g.packed_masks()
    assert w.dtype == np.uint32 and w.shape == (M, 8)
    for m in range(M):
        bits = {j for j in range(256) if (int(w[m, j // 32]) >> (j % 32)) & 1}
        assert bits == set(preds[m]), m
    assert list(g.node_flags()[:3]) == [1, 1, 0] and list(g.node_flags()[-3:]) == [2, 2, 2]
    one = ops.TranscriptGraph([4], [[]], [True], [True])
    assert one.node_flags()[0] == 3 and not one.packed_masks().any()
    # the matrix form gives the same graph
    g2 = ops.TranscriptGraph(g.ids, g.pred, g.start, g.end)
    assert np.array_equal(g2.packed_masks(), w)


def test_transcript_graph_value_errors():
    from action_segmentation_amd import ops
    TG = ops.TranscriptGraph
    ok = TG.chain(np.zeros(256, np.int64))
    assert len(ok) == 256 == ops.MAX_TRANSCRIPT
    with pytest.raises(ValueError):
        TG.chain(np.zeros(257, np.int64))                               # more than 256 nodes
    with pytest.raises(ValueError):
        TG.chain([])
    with pytest.raises(ValueError):
        TG.from_candidates([np.arange(200), np.arange(200) + 1])        # a trie of 400 nodes
    with pytest.raises(ValueError):
        TG([0, 1], [[1], []], [True, False], [False, True])             # an edge j >= m
    with pytest.raises(ValueError):
        TG([0, 1], [[], [1]], [True, False], [False, True])             # ... a loop
    with pytest.raises(ValueError):
        TG([0, 1], np.array([[0, 1], [0, 0]]), [True, False], [False, True])
    with pytest.raises(ValueError):
        TG([0, 1], [[], [0]], [False, False], [False, True])            # no start node
    with pytest.raises(ValueError):
        TG([0, 1], [[], [0]], [True, False], [False, False])            # no end node
    with pytest.raises(ValueError):
        TG([0, 1], [[]], [True, False], [False, True])                  # one predecessor list short
    with pytest.raises(ValueError):
        TG.from_optional([0, 1], [True])
    with pytest.raises(ValueError):
        TG.from_candidates([[0, 1], []])


def test_the_gpu_tests_shapes_have_alignments_and_node_ties():
    """What tests/test_gpu_align_graph.py relies on, asserted here with the reference alone: with its seeds every video of
    every shape has an alignment but the ones it names, and the integer run of every shape has a video on which the
    back-trace meets two different nodes at the maximum (but the chain and the gap graph, which cannot)."""
    import test_gpu_align_graph as T
    for name in T.SHAPES:
        if name in ('kp=1024', 'M=256'):                                # (seconds of numpy; the GPU test runs them)
            continue
        for ties in (False, True):
            h, batch, graphs = T._case(name, ties)
            feasible, tied = [], 0
            for i, g in enumerate(graphs):
                found = []
                best, segs = G.align_graph_ref(node_ties=found, **T._video_inputs(h, batch, i, g)[4])
                feasible.append(segs is not None)
                tied += bool(found)
            assert feasible == T.NOT_ALL_FEASIBLE.get(name, [True] * len(graphs)), (name, ties)
            assert tied or not ties or name in ('chain', 'gap'), name


# ------------------------------------------------------------------------------------------------ the C entry points
def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _ws(lengths, ms, entry='smm_align_graph_workspace_bytes', **kw):
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    kw.setdefault('total', int(lengths.max()) * len(lengths))
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), **kw)
    return getattr(_lib.load(), entry)(ctypes.byref(shape), _p(lengths), _p(off))


_UNSET = object()


def _call(shape=None, off=_UNSET, elp=POISON, trans=POISON, init=POISON, len_scores=POISON, node_class=POISON, pred_mask=POISON,
          node_flags=POISON, best=POISON, spans=None, used=None, ws=POISON, ws_bytes=1 << 40, lengths=_UNSET, n_states=_UNSET,
          frame_off=_UNSET):
    lib = _lib.load()
    lengths = np.array([6], np.int64) if lengths is _UNSET else lengths
    frame_off = np.array([0], np.int64) if frame_off is _UNSET else frame_off
    n_states = np.array([3], np.int32) if n_states is _UNSET else n_states
    off = np.array([0, 2], np.int64) if off is _UNSET else off
    shape = shape or _shape()
    return lib.smm_align_graph_f64(ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), elp, trans, init,
                                   len_scores, None, None, node_class, pred_mask, node_flags, _p(off), spans, None, best, None,
                                   used, ws, ctypes.c_size_t(ws_bytes), POISON)


def test_the_new_symbols_are_exported():
    lib = _lib.load()
    for name in ('smm_align_graph_f64', 'smm_align_graph_workspace_bytes'):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'smmdp.h')).read()
    assert re.search(r'int smm_align_graph_f64\(', header) and re.search(r'size_t smm_align_graph_workspace_bytes\(', header)


def test_refuses_bad_arguments_before_staging():
    for name in ('elp', 'trans', 'init', 'len_scores', 'node_class', 'pred_mask', 'node_flags', 'ws', 'off', 'lengths',
                 'n_states', 'frame_off'):
        assert _call(**{name: None}) == ARG, name
    assert _call(best=None) == ARG                                      # every output NULL (`used` is none of the four)
    assert _call(best=None, used=POISON) == ARG
    assert _call(best=None, spans=POISON, ws_bytes=0) == WORKSPACE      # (one output is enough to get further)
    assert _call(shape=_shape(b=0)) == ARG
    assert _call(off=np.array([0, 0], np.int64)) == ARG                 # a video without nodes
    assert _call(off=np.array([2, 1], np.int64)) == ARG                 # non-monotone
    two = dict(shape=_shape(b=2), lengths=np.array([6, 6], np.int64), frame_off=np.array([0, 6], np.int64))
    assert _call(off=np.array([0, 3, 2], np.int64), **two) == ARG
    assert _call(off=np.array([0, 3, 3], np.int64), **two) == ARG
    assert _call(off=np.array([0, 3, 5], np.int64), ws_bytes=0, **two) == WORKSPACE


def test_refuses_unsupported_shapes_before_staging():
    assert _call(shape=_shape(flags=_lib.SHAPE_NO_EOS)) == UNSUPPORTED
    assert _call(shape=_shape(c=33)) == UNSUPPORTED
    assert _call(shape=_shape(k_rows=1025)) == UNSUPPORTED
    assert _call(off=np.array([0, 257], np.int64)) == UNSUPPORTED
    assert _call(off=np.array([0, 256], np.int64), ws_bytes=0) == WORKSPACE


def test_refuses_a_short_workspace_before_staging():
    need = _ws([6], [2])
    assert need > 0
    assert _call(ws_bytes=need - 1) == WORKSPACE
    assert _call(ws_bytes=0) == WORKSPACE
    assert _call(ws_bytes=_ws([6], [2], entry='smm_align_workspace_bytes')) == WORKSPACE   # (the plain alignment's is too small)


def test_workspace_bytes():
    lib = _lib.load()
    plain = lambda lengths, ms, **kw: _ws(lengths, ms, entry='smm_align_workspace_bytes', **kw)
    # the header's formula: the plain alignment's plus the gam columns, M (T + 1) doubles per video
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'smmdp.h')).read()
    assert 'smm_align_graph_workspace_bytes = smm_align_workspace_bytes(shape, lengths_host, node_offset_host)' in header
    assert '+ 8 * sum_i M_i (T_i + 1) bytes' in header
    for lengths, ms, kw in (([6], [2], {}), ([6, 60], [2, 3], dict(c=5)), ([600, 7, 33], [256, 1, 40], dict(c=7, k_rows=40))):
        extra = 8 * sum(m * (t + 1) for t, m in zip(lengths, ms))
        assert _ws(lengths, ms, **kw) == plain(lengths, ms, **kw) + extra
        assert _ws(lengths, ms, **kw) >= plain(lengths, ms, **kw)
    assert _ws([6], [1]) < _ws([6], [2]) < _ws([6], [6]) < _ws([6], [256])
    assert _ws([6], [3]) < _ws([7], [3]) < _ws([60], [3]) < _ws([600], [3])
    # 0 on what the call refuses
    assert _ws([6], [0]) == 0 and _ws([6], [257]) == 0 and _ws([0], [1]) == 0
    assert _ws([6], [2], flags=_lib.SHAPE_NO_EOS) == 0
    assert _ws([6], [2], c=33) == 0 and _ws([6], [2], k_rows=1025) == 0 and _ws([6], [2], k_rows=1) == 0
    lengths, off = np.array([6], np.int64), np.array([0, 2], np.int64)
    assert lib.smm_align_graph_workspace_bytes(ctypes.byref(_shape(t_max=4)), _p(lengths), _p(off)) == 0   # longer than t_max
    assert lib.smm_align_graph_workspace_bytes(ctypes.byref(_shape()), None, _p(off)) == 0
    assert lib.smm_align_graph_workspace_bytes(ctypes.byref(_shape()), _p(lengths), None) == 0
    assert lib.smm_align_graph_workspace_bytes(None, _p(lengths), _p(off)) == 0


# ------------------------------------------------------------------------------------------------ Python-level argument checks
def test_ops_align_graph_value_errors():
    import torch
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 5], [3], 4)
    graphs = [ops.TranscriptGraph.chain([0, 1]), ops.TranscriptGraph.from_candidates([[2, 2, 1], [2, 0]])]
    off = np.array([0, 2, 6], np.int64)
    assert ops.align_graph_workspace_bytes(batch, off) == ops.align_workspace_bytes(batch, off) + 8 * (2 * 7 + 4 * 6)
    with pytest.raises(ValueError):
        ops.align_graph_workspace_bytes(batch, off[:-1])
    z = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.align_graph(batch, z, z, z, z, graphs[:1])                  # one graph short, before a device is touched
    with pytest.raises(ValueError):
        ops.align_graph(batch, z, z, z, z, graphs + graphs[:1])
    with pytest.raises(ValueError):
        ops.align_graph(ops.Batch([6, 5], [3], 4, no_eos=True), z, z, z, z, graphs)     # add_eos=False


def test_module_align_graph_value_errors():
    import torch
    from action_segmentation_amd import ops, synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    data = synth.SynthDatasplit('tiny', seed=11)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    g = ops.TranscriptGraph.chain([0, 1])
    x, lengths = torch.zeros(2, 6, 8), torch.tensor([6, 5])
    with pytest.raises(ValueError):
        model.model.align_graph(x, lengths, torch.tensor([0, 1]), [g, g], add_eos=False)
    with pytest.raises(ValueError):
        model.model.align_graph(x, lengths, torch.tensor([0, 1]), [g])  # one graph short
