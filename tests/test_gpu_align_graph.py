"""Forced alignment to a transcript graph (smm_align_graph_f64 / ops.align_graph / SemiMarkovModule.align_graph,
align_graph_packed / SemiMarkovModel.align_candidates) on the GPU.

spans, labels, best, n_segs and used are compared bit for bit with tests/align_graph_ref.py (the definition in numpy) on every
video and, on videos that have an alignment, with the C twin's Viterbi on the lattice whose states are the nodes -- on
real-valued inputs and on small-integer inputs, where many alignments tie exactly and the back-trace's tie rule decides.
endpen is NULL or small integers, so no allowed end sits at the twin's -1e9.

The seeds are fixed so that every video of every shape not named "infeasible" or "gap" has an alignment, and that in the
integer run of every shape the reference's back-trace meets, on at least one video, a step at which two different nodes attain
the maximum: two maximal alignments through different nodes (``align_graph_ref(node_ties=...)``;
test_align_graph_host.py asserts both on the host).  The chain and the gap graph are exempt: a chain has one node set, and no
length fits both paths of the gap graph."""
import numpy as np
import pytest
import torch

import align_graph_ref as G
import test_gpu_align as A
import test_gpu_align_optional as AO

pytestmark = pytest.mark.gpu
P = A.P
_t, _h = A._t, A._h


# ------------------------------------------------------------------------------------------------ graphs (host only)
def _tg():
    from action_segmentation_amd import ops
    return ops.TranscriptGraph


def _lists(M, preds, start, end):
    """(structure without ids): predecessor lists, start nodes, end nodes"""
    return preds, np.isin(np.arange(M), start), np.isin(np.arange(M), end)


def _diamond():
    return _lists(4, [[], [0], [0], [1, 2]], [0], [3])


def _diamond_tail():
    return _lists(5, [[], [0], [0], [1, 2], [3]], [0], [4])


def _free_order():
    """s -> x -> y -> e and s -> y' -> x' -> e, sharing s and e"""
    return _lists(6, [[], [0], [1], [0], [3], [2, 4]], [0], [5])


def _skip_edge():
    """0 -> 1 -> 2 -> 3 -> 4 plus 1 -> 4"""
    return _lists(5, [[], [0], [1], [2], [1, 3]], [0], [4])


def _gap():
    """paths of 2 or 6 nodes only: 0 -> 5 and 0 -> 1 -> 2 -> 3 -> 4 -> 5"""
    return _lists(6, [[], [0], [1], [2], [3], [0, 4]], [0], [5])


def _dead_parts():
    """node 3 has no predecessor and is no start node (dead), so node 4, an end node, is reached by no start node; node 5
    is reached through 2 only"""
    return _lists(6, [[], [0], [1], [], [3], [2, 3]], [0], [2, 4, 5])


def _random_dag(rng, M, max_pred, starts=1, ends=1):
    """m - 1 -> m always (so the longest path has M nodes), up to max_pred - 1 random earlier nodes more; the first `starts`
    nodes may start and the last `ends` may end"""
    preds = [[]]
    for m in range(1, M):
        extra = rng.choice(m, size=min(m, int(rng.integers(0, max_pred))), replace=False) if m > 1 else []
        preds.append(sorted(set([m - 1]) | set(int(j) for j in extra)))
    return _lists(M, preds, list(range(starts)), list(range(M - ends, M)))


def _skip_one(M):
    return _lists(M, [[j for j in (m - 2, m - 1) if j >= 0] for m in range(M)], [0], [M - 1])


def _complete(M):
    return _lists(M, [list(range(m)) for m in range(M)], [0], [M - 1])


def _trie(cands):
    g = _tg().from_candidates(cands)
    return g


def _trie5(rng):
    """5 candidates of lengths 2..9 over 4 classes"""
    return [rng.integers(0, 4, size=int(n)) for n in (2, 4, 6, 8, 9)]


def _chain_struct(M):
    return _lists(M, [[m - 1] if m else [] for m in range(M)], [0], [M - 1])


def _opt_struct(opt):
    _, pred, first, end = G.from_optional(np.zeros(len(opt), np.int64), opt)
    return pred, first, end


def _shapes():
    """name -> (videos [(T, kp, M, group)], structures per video (or TranscriptGraphs with their own local ids), states per
    group, c_max, k_rows)"""
    r = np.random.default_rng(20261)
    alt = AO._alt
    t5 = _trie(_trie5(r))
    k3, k7 = _trie([[0, 1], [0, 2]]), _trie([[0, 1, 2, 3], [0, 1, 3, 2], [0, 2]])
    ragged = A.SHAPES['ragged, three groups']
    return {
        'chain': ([(40, 9, 7, 0)], [_chain_struct(7)], [4], 4, 9),
        'from optional, alternating': ([(60, 9, 11, 0), (9, 9, 11, 0), (5, 9, 11, 0)], [_opt_struct(alt(11))] * 3, [4], 4, 9),
        'from optional, all optional': ([(30, 6, 12, 0)], [_opt_struct(np.ones(12, bool))], [4], 4, 6),
        'diamond': ([(13, 7, 4, 0)], [_diamond()], [3], 3, 7),
        'free order': ([(20, 7, 6, 0)], [_free_order()], [4], 4, 7),
        'skip edge': ([(25, 9, 5, 0), (5, 9, 5, 0)], [_skip_edge()] * 2, [4], 4, 9),
        'trie of 5': ([(50, 9, len(t5), 0)], [t5], [4], 4, 9),
        'two starts, three ends': ([(30, 7, 9, 0), (12, 7, 9, 0)], [_random_dag(r, 9, 3, starts=2, ends=3)] * 2, [4], 4, 7),
        'dead node, unreachable end': ([(20, 7, 6, 0), (12, 7, 6, 0), (3, 7, 6, 0)], [_dead_parts()] * 3, [4], 4, 7),
        'gap': ([(5, 3, 6, 0), (7, 3, 6, 0), (4, 3, 6, 0)], [_gap()] * 3, [3], 3, 3),
        'T around the tile, span limit below it': (
            [(P - 1, 40, 25, 0), (P, 40, 25, 0), (P + 1, 40, 45, 0), (2 * P + 3, 40, 45, 0)],
            [_random_dag(r, 25, 4), _random_dag(r, 25, 4), _random_dag(r, 45, 4), _random_dag(r, 45, 4)], [5], 5, 40),
        'kp=1024': ([(P + 1, 1024, 3, 0), (2 * P + 3, 1024, 7, 0), (2100, 1024, 5, 0)], [k3, k7, _diamond_tail()], [4], 4, 1024),
        'M=256': ([(300, 6, 256, 0), (300, 3, 256, 0)], [_random_dag(r, 256, 8), _skip_one(256)], [7], 7, 9),
        'M=64, every pair an edge': ([(100, 6, 64, 0)], [_complete(64)], [5], 5, 6),
        'infeasible beside feasible': (
            [(13, 7, 4, 0), (3, 7, 5, 0), (12, 7, 6, 0), (40, 7, 6, 0), (9, 7, 4, 0)],
            [_diamond(), _chain_struct(5), _free_order(), _free_order(), _diamond()], [4], 4, 7),
        'ragged, three groups': (ragged[0], [_random_dag(r, v[2], 4, starts=min(2, v[2]), ends=min(2, v[2])) for v in ragged[0]])
        + ragged[1:],
    }


SHAPES = _shapes()
NOT_ALL_FEASIBLE = {'gap': [False, True, True], 'infeasible beside feasible': [True, False, True, False, True]}


def _make(seed, videos, cs, cm, k_rows, ties, structs, with_endpen=True, **kw):
    """videos: [(T, kp, M, group)], structs: per video (pred, start, end) over random local ids, or a TranscriptGraph that
    brings its ids.  endpen: small integers or None.  -> host arrays, the Batch, one TranscriptGraph per video."""
    if 'transcripts' not in kw:
        rng = np.random.default_rng(seed + 7)
        kw['transcripts'] = [s.ids if isinstance(s, _tg()) else rng.integers(0, cs[v[3]], size=v[2]) for s, v in zip(structs, videos)]
    h, batch, tr = A._make(seed, videos, cs, cm, k_rows, ties, with_endpen=False, **kw)
    if with_endpen:
        h['endpen'] = np.random.default_rng(seed + 1000).integers(-3, 4, size=(len(videos), cm)).astype(np.float64)
    graphs = [s if isinstance(s, _tg()) else _tg()(a, *s) for s, a in zip(structs, tr)]
    assert all(len(g) == v[2] for g, v in zip(graphs, videos))
    return h, batch, graphs


# (chosen on the host so that the integer run of the shape has a video with two maximal alignments through different nodes)
SEED_SHIFT = {'from optional, alternating': 1, 'diamond': 10, 'skip edge': 24, 'trie of 5': 3, 'two starts, three ends': 3,
              'dead node, unreachable end': 7, 'T around the tile, span limit below it': 23, 'kp=1024': 1,
              'ragged, three groups': 3}


def _case(name, ties):
    videos, structs, cs, cm, k_rows = SHAPES[name]
    return _make(sum(map(ord, name)) + ties + 2 * SEED_SHIFT.get(name, 0), videos, cs, cm, k_rows, ties, structs)


def _tuple(g):
    return g.ids, g.pred, g.start, g.end


def _run(h, batch, graphs):
    from action_segmentation_amd import ops
    out = ops.align_graph(batch, _t(h['elp']), _t(h['trans']), _t(h['init']), _t(h['len']), graphs,
                          endpen=None if h['endpen'] is None else _t(h['endpen']),
                          class_map=None if h['cmap'] is None else _t(h['cmap'], torch.int64), want_used=True)
    torch.cuda.synchronize()
    res = {k: _h(out[k]) for k in ('spans', 'labels', 'best', 'n_segs')}
    res['used'] = [_h(u) for u in out['used']]
    res['err'] = ops.error_flag(batch, out)
    return res


def _video_inputs(h, batch, i, g):
    gr = int(batch.group[i]) if batch.group is not None else 0
    C, T, o = int(batch.n_states[gr]), int(batch.lengths[i]), int(batch.frame_offset[i])
    kp = int(batch.kp[i]) if batch.kp is not None else min(batch.k_rows, batch.t_max)
    return gr, C, T, o, dict(elp=h['elp'][o:o + T, :C], graph=_tuple(g), trans=h['trans'][gr, :C, :C], init=h['init'][gr, :C],
                             len_scores=h['len'][gr, :, :C], kp=kp, endpen=None if h['endpen'] is None else h['endpen'][i, :C])


_refs = {}


def _reference(key, h, batch, graphs, twin=True):
    """Per video (best, segs) of the reference, once per case, checked against the twin where there is an alignment."""
    if key is not None and key in _refs:
        return _refs[key]
    out = []
    for i, g in enumerate(graphs):
        kw = _video_inputs(h, batch, i, g)[4]
        best, segs = G.align_graph_ref(**kw)
        if twin and segs is not None:
            v, tw = G.twin_align(**kw)
            assert best == v and segs == tw, (i, best, v)
        out.append((best, segs))
    if key is not None:
        _refs[key] = out
    return out


def _check(h, batch, graphs, twin=True, expect_err=0, res=None, key=None):
    """ops.align_graph against the reference on every video, the reference against the twin on those that have an alignment."""
    res = res or _run(h, batch, graphs)
    assert (res['err'] != 0) == bool(expect_err)
    feasible = []
    for i, (g, (best, segs)) in enumerate(zip(graphs, _reference(key, h, batch, graphs, twin))):
        gr, C, T, o, _ = _video_inputs(h, batch, i, g)
        a = g.ids
        gid = (lambda c: c) if h['cmap'] is None else (lambda c, gr=gr: int(h['cmap'][gr, c]))
        assert res['best'][i] == best or (np.isnan(best) and np.isnan(res['best'][i])), (i, res['best'][i], best)
        assert np.array_equal(res['spans'][i], G.span_row(segs, a, T, batch.t_max, gid, gid(C))), i
        assert np.array_equal(res['labels'][o:o + T], G.frame_labels(segs, a, T, gid)), i
        assert res['n_segs'][i] == (0 if segs is None else len(segs)), i
        assert np.array_equal(res['used'][i], G.used_flags(segs, len(a))), i
        feasible.append(segs is not None)
    covered = np.zeros(batch.total_frames, bool)
    for i in range(batch.b):
        covered[int(batch.frame_offset[i]):int(batch.frame_offset[i] + batch.lengths[i])] = True
    assert (res['labels'][~covered] == -1).all()
    return res, feasible


def _same(r1, r2, keys=('best', 'spans', 'labels', 'n_segs')):
    for k in keys:
        assert np.array_equal(r1[k], r2[k]), k
    if 'used' in r1 and 'used' in r2:
        assert all(np.array_equal(x, y) for x, y in zip(r1['used'], r2['used']))


# ------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_bit_exact_against_the_reference_and_the_twin(name, ties):
    from action_segmentation_amd import ops
    h, batch, graphs = _case(name, ties)
    res, feasible = _check(h, batch, graphs, key=(name, ties))
    assert res['err'] == 0
    assert feasible == NOT_ALL_FEASIBLE.get(name, [True] * batch.b)
    tr = [g.ids for g in graphs]
    if name == 'chain':
        _same(A._run(h, batch, tr), res)
        assert res['used'][0].all()
    if name.startswith('from optional'):
        flags = [AO._alt(11)] * 3 if 'alternating' in name else [np.ones(12, bool)]
        assert all(np.array_equal(_tuple(_tg().from_optional(a, f))[k], _tuple(g)[k]) for a, f, g in zip(tr, flags, graphs)
                   for k in range(4))
        _same(AO._run(h, batch, tr, flags), res)
    if name == 'gap':
        # paths of 2 or 6 nodes, segments of at most 2 frames: 5 frames pass the count rule (2 <= 5 <= 12) and have no
        # alignment; 7 frames take the long path, 4 the short one
        assert res['best'][0] == -np.inf and res['n_segs'][0] == 0 and (res['spans'][0] == -1).all() and not res['used'][0].any()
        assert G.feasible_by_count(5, *_tuple(graphs[0])[1:], 3)
        assert res['n_segs'][1] == 6 and res['n_segs'][2] == 2
    if name == 'dead node, unreachable end':
        assert not any(u[3:5].any() for u in res['used'])
    if name == 'infeasible beside feasible':
        assert (res['best'][[1, 3]] == -np.inf).all() and (res['spans'][[1, 3]] == -1).all()
        assert not res['used'][1].any() and not res['used'][3].any()
        keep = [0, 2, 4]                                                # the neighbours alone: the same results
        b2 = ops.Batch(batch.lengths[keep], [4], 7, c_max=4, frame_offset=batch.frame_offset[keep], group=batch.group[keep],
                       kp=batch.kp[keep], t_max=batch.t_max, total_frames=batch.total_frames)
        r2 = _run(dict(h, endpen=h['endpen'][keep]), b2, [graphs[i] for i in keep])
        assert r2['err'] == 0
        for k in ('best', 'spans', 'n_segs'):
            assert np.array_equal(r2[k], res[k][keep]), k
        assert all(np.array_equal(r2['used'][j], res['used'][i]) for j, i in enumerate(keep))
        cover = np.zeros(batch.total_frames, bool)
        for i in keep:
            cover[int(batch.frame_offset[i]):int(batch.frame_offset[i] + batch.lengths[i])] = True
        assert np.array_equal(r2['labels'][cover], res['labels'][cover]) and (r2['labels'][~cover] == -1).all()


@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
def test_endpen_null_and_no_class_map(ties):
    videos, structs, cs, cm, k_rows = SHAPES['ragged, three groups']
    h, batch, graphs = _make(71 + ties, videos, cs, cm, k_rows, ties, structs, with_endpen=False, with_cmap=False, gaps=False)
    _, feasible = _check(h, batch, graphs)
    assert all(feasible)


def test_two_calls_give_the_same_bits():
    h, batch, graphs = _case('T around the tile, span limit below it', False)
    _same(_run(h, batch, graphs), _run(h, batch, graphs))


def test_an_id_outside_the_states_or_an_edge_to_a_later_node_leaves_no_alignment():
    """... with the error word clear and the neighbour untouched; the masks go to the C entry point as they are."""
    from action_segmentation_amd import ops
    h, batch, graphs = _make(12, [(13, 7, 4, 0), (13, 7, 4, 0), (13, 7, 4, 0)], [3], 3, 7, False, [_diamond()] * 3)
    clean, _ = _check(h, batch, graphs)
    bad_id = graphs[1].with_ids([0, 3, 1, 2])
    upward = _tg()(graphs[2].ids, graphs[2].pred, graphs[2].start, graphs[2].end)
    upward.pred = upward.pred.copy()
    upward.pred[1, 2] = True                                            # (behind the constructor's back)
    res, feasible = _check(h, batch, [graphs[0], bad_id, upward])
    assert feasible == [True, False, False] and res['err'] == 0
    assert res['best'][0] == clean['best'][0] and np.array_equal(res['spans'][0], clean['spans'][0])
    assert ops.MAX_TRANSCRIPT == 256


# ------------------------------------------------------------------------------------------------ 2. candidate sets
def _candidate_case():
    """6 videos in 2 groups, 8 candidates each; the last video's candidates all need more frames than it has."""
    rng = np.random.default_rng(77)
    cs = [5, 4]
    videos = [(40, 9, 0, 0), (33, 9, 0, 1), (50, 12, 0, 0), (21, 9, 0, 1), (64, 12, 0, 0), (3, 9, 0, 1)]
    cands = []
    for (T, kp, _, g) in videos:
        base = rng.integers(0, cs[g], size=int(rng.integers(5, 9)))
        mine = [base]
        while len(mine) < 8:
            c = base.copy()
            if rng.random() < 0.5:
                c[int(rng.integers(0, len(c)))] = int(rng.integers(0, cs[g]))
            else:
                c = np.delete(c, int(rng.integers(0, len(c))))
            if not any(np.array_equal(c, m) for m in mine):
                mine.append(c)
        cands.append(mine)
    graphs = [_tg().from_candidates(c) for c in cands]
    videos = [(T, kp, len(g), gr) for (T, kp, _, gr), g in zip(videos, graphs)]
    h, batch, graphs = _make(505, videos, cs, 5, 12, False, graphs)
    return h, batch, graphs, cands


def test_a_candidate_set_is_the_best_of_its_candidates():
    h, batch, graphs, cands = _candidate_case()
    res, feasible = _check(h, batch, graphs)
    assert feasible == [True] * 5 + [False]
    per = [A._run(h, batch, [c[j] for c in cands]) for j in range(8)]
    bests = np.stack([p['best'] for p in per])                          # [candidate, video]
    for i in range(batch.b - 1):
        top = np.flatnonzero(bests[:, i] == bests[:, i].max())
        assert top.size == 1, (i, bests[:, i])                          # (the seeds make the arg-max unique)
        j = int(top[0])
        o, T = int(batch.frame_offset[i]), int(batch.lengths[i])
        assert res['best'][i] == bests[j, i]
        assert np.array_equal(res['labels'][o:o + T], per[j]['labels'][o:o + T])
        assert np.array_equal(res['spans'][i], per[j]['spans'][i])
        assert graphs[i].candidate_of(res['used'][i]) == j
    assert (bests[:, -1] == -np.inf).all() and graphs[-1].candidate_of(res['used'][-1]) == -1


# ------------------------------------------------------------------------------------------------ 3. smm_viterbi_f64, expanded
def test_equals_smm_viterbi_f64_on_the_expanded_lattice():
    """Graphs of at most 32 nodes, one group per video on the expanded side: the states are the nodes."""
    from action_segmentation_amd import ops
    rng = np.random.default_rng(31)
    T, K = 30, 12
    structs = [_diamond(), _free_order(), _skip_edge(), _random_dag(rng, 32, 4, starts=2, ends=2), _random_dag(rng, 17, 4),
               _complete(12), _trie(_trie5(rng))]
    videos = [(T, K, len(s) if isinstance(s, _tg()) else len(s[0]), 0) for s in structs]
    h, batch, graphs = _make(8, videos, [4], 4, K, False, structs, gaps=False)
    res = _run(h, batch, graphs)
    assert res['err'] == 0 and np.isfinite(res['best']).all()
    b = batch.b
    ms = np.array([len(g) for g in graphs], np.int32)
    M = int(ms.max())
    assert M <= 32
    e2 = np.zeros((b * T, M))
    t2, i2, l2, p2 = np.full((b, M, M), A.BIG_NEG), np.full((b, M), A.BIG_NEG), np.zeros((b, K, M)), np.full((b, M), A.BIG_NEG)
    for i, g in enumerate(graphs):
        kw = _video_inputs(h, batch, i, g)[4]
        ee, tt, ii, ll, pp = G.expanded_lattice(**kw)
        m = len(g)
        e2[i * T:(i + 1) * T, :m], t2[i, :m, :m], i2[i, :m], l2[i, :, :m], p2[i, :m] = ee, tt, ii, ll, pp
    bl = ops.Batch(batch.lengths, ms, K, c_max=M, group=np.arange(b, dtype=np.int32), t_max=T, total_frames=b * T)
    v2 = ops.viterbi(bl, _t(e2), _t(t2), _t(i2), _t(l2), endpen=_t(p2))
    torch.cuda.synchronize()
    assert ops.error_flag(bl, v2) == 0
    assert np.array_equal(_h(v2['best']), res['best'])
    sp = _h(v2['spans'])
    for i in range(b):
        pos = np.flatnonzero(sp[i, :T] >= 0)
        assert np.array_equal(pos, np.flatnonzero(res['spans'][i, :T] >= 0)), i
        assert np.array_equal(np.flatnonzero(res['used'][i]), sp[i, pos]), i          # the states are the nodes


# ------------------------------------------------------------------------------------------------ 4. errors
def test_a_nan_in_elp_sets_the_error_word_and_leaves_the_other_videos():
    videos = [(30, 9, 6, 0), (33, 9, 5, 0), (28, 9, 6, 0), (21, 9, 4, 0)]
    h, batch, graphs = _make(21, videos, [5], 5, 9, False, [_free_order(), _skip_edge(), _free_order(), _diamond()])
    clean, feasible = _check(h, batch, graphs)
    assert all(feasible)
    h2 = dict(h, elp=h['elp'].copy())
    h2['elp'][int(batch.frame_offset[2]) + 7, int(graphs[2].ids[0])] = np.nan
    res = _run(h2, batch, graphs)
    assert res['err'] != 0
    assert np.isnan(res['best'][2]) and res['n_segs'][2] == 0 and (res['spans'][2] == -1).all() and not res['used'][2].any()
    _check(h2, batch, graphs, twin=False, expect_err=1, res=res)
    for k in ('best', 'spans', 'n_segs'):
        assert np.array_equal(res[k][[0, 1, 3]], clean[k][[0, 1, 3]]), k
    assert _run(h, batch, graphs)['err'] == 0                          # the next call on clean inputs clears it


def test_an_inf_in_a_transition_only_a_skip_edge_reads():
    """trans[a_4][a_1] is read by the skip edge 1 -> 4 alone; trans[a_4][a_0] by no edge."""
    videos = [(30, 9, 5, 0), (30, 9, 5, 1)]
    ids = [[0, 1, 2, 3, 4], [0, 1, 2, 3, 4]]
    h, batch, graphs = _make(43, videos, [5, 5], 5, 9, False, [_skip_edge()] * 2, transcripts=ids)
    clean, feasible = _check(h, batch, graphs)
    assert all(feasible)
    h2 = dict(h, trans=h['trans'].copy())
    h2['trans'][1, 4, 0] = np.inf
    res, _ = _check(h2, batch, graphs)
    _same(res, clean, ('best', 'spans', 'n_segs'))
    h2['trans'][1, 4, 1] = np.inf
    res = _run(h2, batch, graphs)
    assert res['err'] != 0 and np.isnan(res['best'][1]) and res['n_segs'][1] == 0 and (res['spans'][1] == -1).all()
    assert res['best'][0] == clean['best'][0] and np.array_equal(res['spans'][0], clean['spans'][0])
    _check(h2, batch, graphs, twin=False, expect_err=1, res=res)


def test_a_bad_table_entry_of_a_node_off_every_path_sets_the_error_word():
    """Every node and every edge counts: the dead node's length scores and its edge's transition."""
    ids = [[0, 1, 2, 3, 1, 2]]
    h, batch, graphs = _make(9, [(20, 7, 6, 0)], [4], 4, 7, False, [_dead_parts()], transcripts=ids)
    assert all(_check(h, batch, graphs)[1])
    h2 = dict(h, len=h['len'].copy())
    h2['len'][0, 3, 3] = np.nan                                         # class 3: the dead node alone
    _check(h2, batch, graphs, twin=False, expect_err=1)
    h3 = dict(h, trans=h['trans'].copy())
    h3['trans'][0, 1, 3] = np.inf                                       # the edge 3 -> 4
    _check(h3, batch, graphs, twin=False, expect_err=1)
    h4 = dict(h, len=h['len'].copy())
    h4['len'][0, 2, 1] = -np.inf                                        # -inf is an ordinary "impossible"
    _check(h4, batch, graphs, twin=False)


# ------------------------------------------------------------------------------------------------ 5. layers
def test_call_paths_agree():
    """SemiMarkovModule.align_graph / align_graph_packed = ops.align_graph in local ids; a class outside the video's task
    leaves that video without an alignment; SemiMarkovModel.align_candidates = the best of SemiMarkovModel.align per
    candidate, also when the candidates are split over several tries."""
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts
    data, model = A._tiny_model()
    pc = model.prepare(data)
    t = pc.tables
    elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
    out = ops.viterbi(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    base = spans_to_transcripts(out['spans'], pc.lengths)
    cmap = _h(t['class_map'])
    group = pc.batch.group if pc.batch.group is not None else np.zeros(pc.batch.b, np.int64)
    rng = np.random.default_rng(2)
    cands = {}
    for i, (name, a) in enumerate(zip(pc.video_names, base)):
        valid = cmap[group[i], :pc.batch.n_states[group[i]]]
        a = np.asarray(a, np.int64)[:40]
        mine = [a]
        for _ in range(3):
            c = a.copy()
            c[int(rng.integers(0, len(c)))] = int(rng.choice(valid))
            mine.append(c)
        cands[name] = mine
    graphs = [ops.TranscriptGraph.from_candidates(cands[name]) for name in pc.video_names]
    local = [g.with_ids([list(cmap[group[i], :pc.batch.n_states[group[i]]]).index(c) for c in g.ids])
             for i, g in enumerate(graphs)]
    o2 = ops.align_graph(pc.batch, elp, t['trans'], t['init'], t['len'], local, endpen=pc.endpen, class_map=t['class_map'],
                         want_used=True)
    torch.cuda.synchronize()
    assert ops.error_flag(pc.batch, o2) == 0
    labels, best, used = model.model.align_graph_packed(pc, graphs)
    assert np.array_equal(_h(labels), _h(o2['labels'])) and np.array_equal(_h(best), _h(o2['best']))
    assert all(np.array_equal(_h(u), _h(v)) for u, v in zip(used, o2['used']))
    assert (_h(best) >= _h(out['best'])).all() and np.isfinite(_h(best)).all()    # (the Viterbi path is a candidate)
    with pytest.raises(ValueError):
        model.model.align_graph_packed(pc, graphs[:-1])
    # a class that is no class of the model's: that video has no alignment, the others keep theirs
    alien = [graphs[0].with_ids(np.where(np.arange(len(graphs[0])) == 0, 10 ** 6, graphs[0].ids))] + graphs[1:]
    l3, b3, u3 = model.model.align_graph_packed(pc, alien)
    assert _h(b3)[0] == -np.inf and not _h(u3[0]).any() and np.array_equal(_h(b3)[1:], _h(best)[1:])
    # the model: the best of its align per candidate
    per = [model.align(data, {name: cands[name][j] for name in pc.video_names}) for j in range(4)]
    per_best = np.stack([_h(model.model.align_packed(pc, [cands[name][j] for name in pc.video_names])[1]) for j in range(4)])
    got, chosen = model.align_candidates(data, cands)
    for i, name in enumerate(pc.video_names):
        top = np.flatnonzero(per_best[:, i] == per_best[:, i].max())
        assert chosen[name] in top, name
        assert per_best[chosen[name], i] == _h(best)[i]
        if top.size == 1:
            assert np.array_equal(got[name], per[int(top[0])][name]), name
    # ... split over several tries: five candidates as long as the video (at most 120) in front of the four above
    long = {}
    for i, name in enumerate(pc.video_names):
        valid = cmap[group[i], :pc.batch.n_states[group[i]]]
        T = int(pc.lengths[i])
        mk = lambda first: np.concatenate([[valid[first % len(valid)]], rng.choice(valid, size=min(T, 120) - 1)])
        long[name] = [mk(j) for j in range(5)] + list(cands[name])
    assert any(ops.TranscriptGraph.trie_nodes(c) > ops.MAX_TRANSCRIPT for c in long.values())
    got2, chosen2 = model.align_candidates(data, long)
    per2 = np.stack([_h(model.model.align_packed(pc, [long[name][j] for name in pc.video_names])[1]) for j in range(9)])
    for i, name in enumerate(pc.video_names):
        assert per2[chosen2[name], i] == per2[:, i].max(), name
        lab = model.align(data, {n: long[n][chosen2[n]] for n in pc.video_names})[name]
        top = np.flatnonzero(per2[:, i] == per2[:, i].max())
        if top.size == 1:
            assert np.array_equal(got2[name], lab), name
    with pytest.raises(ValueError):
        model.align_candidates(data, {name: [np.zeros(300, np.int64)] for name in pc.video_names})
    # per batch, padded
    from action_segmentation_amd.batching import make_data_loader
    from action_segmentation_amd.semimarkov_utils import spans_to_labels
    by_video = dict(zip(pc.video_names, graphs))
    pos = {name: j for j, name in enumerate(pc.video_names)}
    cons_fn = model._test_constraints(data)
    for batch in make_data_loader(model.args, data, shuffle=False, batch_by_task=True, batch_size=model.args.batch_size):
        feats, lengths = batch['features'].to(A.DEV), batch['lengths']
        spans, sc, us = model.model.align_graph(
            feats, lengths, batch['task_indices'], [by_video[v] for v in batch['video_name']],
            additional_allowed_ends_per_instance=model.make_additional_allowed_ends(batch['task_name'], lengths),
            constraints=cons_fn(batch) if cons_fn else None)
        lb = model.model.trim(spans_to_labels(spans), lengths, check_eos=True)
        for i, name in enumerate(batch['video_name']):
            assert np.array_equal(lb[i].numpy(), _h(o2['labels'])[pc.frame_offset[pos[name]]:][:int(lengths[i])]), name
            assert float(sc[i]) == _h(best)[pos[name]], name
            assert np.array_equal(_h(us[i]), _h(used[pos[name]])), name
