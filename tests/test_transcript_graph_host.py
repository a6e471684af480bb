"""Host-side checks of the transcript-graph likelihood: the references of tests/transcript_graph_ref.py against each other and
against the chain / optional-entry references, the header's identities, a trie against its candidates, the ambiguity predicate
against enumeration, the C entry points' refusals (no GPU: every call is refused before anything is staged) and the
Python-level argument checks."""
import ctypes
import types

import numpy as np
import pytest
import torch

import align_graph_ref as AG
import transcript_graph_ref as TG
import transcript_optional_ref as TO
import transcript_ref as TR
from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)


def _tables(rng, C, kp, i):
    return dict(trans=rng.normal(size=(C, C)) * 2, init=rng.normal(size=C) * 2, len_scores=rng.normal(size=(kp + i % 2, C)) * 2,
                kp=kp, endpen=rng.normal(size=C) if i % 3 == 0 else None)


def _case(rng, i, with_holes=False):
    """A random tiny video on a random DAG with an alignment by counting: T <= 7, M <= 6, kp <= 5, C <= 3."""
    while True:
        T, C, M, kp = int(rng.integers(1, 8)), int(rng.integers(1, 4)), int(rng.integers(1, 7)), int(rng.integers(2, 6))
        graph = TG.random_graph(rng, M, C, p_edge=(0.3, 0.6, 0.9)[i % 3])
        if TG.has_alignment_by_count(T, C, graph, kp):
            break
    c = dict(elp=rng.normal(size=(T, C)) * 2, graph=graph, **_tables(rng, C, kp, i))
    if with_holes:
        c['trans'][int(rng.integers(0, C)), int(rng.integers(0, C))] = -np.inf
        c['len_scores'][int(rng.integers(1, kp)), int(rng.integers(0, C))] = -np.inf
    return c


@pytest.fixture(scope='module')
def tiny_cases():
    """300 random tiny cases with each route's answer, computed once."""
    rng = np.random.default_rng(20261019)
    out = []
    for i in range(300):
        c = _case(rng, i)
        out.append((c, TG.brute_logz_graph(**c), TG.torch_grads_graph(**c), TG.twin_grads_graph(**c), TG.forward_backward(**c)))
    return out


def test_the_four_references_agree(tiny_cases):
    """(a) torch + autograd, (b) numpy forward-backward, (c) the C twin on the expanded lattice, (d) brute force: 1e-9."""
    worst, n_fin = 0.0, 0
    for c, (zb, occ, pu, pe), (zt, gt), (zw, gw), fb in tiny_cases:
        if not np.isfinite(zb):                    # a path by counting, but the graph skips the lengths that fit
            assert not np.isfinite(zt) and not np.isfinite(fb['logz']) and zw < -1e8, c
            continue
        n_fin += 1
        errs = [abs(zb - zt), abs(zb - zw), abs(zb - fb['logz']), np.abs(gt['elp'] - occ).max(), np.abs(gw['p_used'] - pu).max(),
                np.abs(fb['p_used'] - pu).max(), np.abs(fb['p_end'] - pe).max()]
        errs += [np.abs(gt[k] - gw[k]).max() for k in ('elp', 'trans', 'init', 'len')]
        errs += [np.abs(gt[k] - fb[k]).max() for k in ('elp', 'trans', 'init', 'len')]
        worst = max(worst, max(errs))
    assert n_fin > 200 and worst <= 1e-9, (n_fin, worst)


def test_identity_and_node_posteriors(tiny_cases):
    """lse_start(h[0] + bh[0]) = logZ_g; p_used from S equals p_used from E; p_end and g_init add up to 1."""
    n = 0
    for c, (zb, occ, pu, pe), _, _, fb in tiny_cases:
        if not np.isfinite(zb):
            continue
        assert abs(fb['ident'] - fb['logz']) <= 1e-9
        assert np.abs(fb['p_used'] - fb['p_used_S']).max() <= 1e-9
        assert abs(fb['p_end'].sum() - 1.0) <= 1e-9 and abs(fb['init'].sum() - 1.0) <= 1e-9
        assert fb['p_used'].min() >= -1e-12 and fb['p_used'].max() <= 1.0 + 1e-9
        n += 1
    assert n > 200


def test_minus_infinity_tables_against_enumeration():
    rng = np.random.default_rng(8)
    n_fin = n_inf = 0
    for i in range(150):
        c = _case(rng, i, with_holes=True)
        zb, occ, pu, pe = TG.brute_logz_graph(**c)
        zt, gt = TG.torch_grads_graph(**c)
        fb = TG.forward_backward(**c)
        assert np.isfinite(zb) == np.isfinite(zt) == np.isfinite(fb['logz'])
        if np.isfinite(zb):
            assert abs(zb - zt) <= 1e-9 and abs(zb - fb['logz']) <= 1e-9
            assert np.abs(gt['elp'] - occ).max() <= 1e-9 and np.abs(fb['p_used'] - pu).max() <= 1e-9
            n_fin += 1
        else:
            assert all(not v.any() for v in gt.values())
            n_inf += 1
    assert n_fin > 50 and n_inf > 5


def test_chains_and_optional_graphs_are_the_family_members():
    rng = np.random.default_rng(4)
    for i in range(40):
        T, C, M, kp = int(rng.integers(3, 8)), 3, int(rng.integers(1, 4)), 4
        a = [int(v) for v in rng.integers(0, C, M)]
        tab = _tables(rng, C, kp, i)
        elp = rng.normal(size=(T, C))
        closing = 0.0 if tab['endpen'] is None else float(tab['endpen'][a[-1]])
        z, g = TG.torch_grads_graph(elp, AG.chain(a), **tab)
        zr, gr = TR.torch_grads(elp, a, tab['trans'], tab['init'], tab['len_scores'], kp, closing)
        assert (np.isfinite(z) == np.isfinite(zr)) and (not np.isfinite(z) or abs(z - zr) <= 1e-12 * max(1.0, abs(zr)))
        assert all(np.abs(g[k] - gr[k]).max() <= 1e-12 for k in g)
        opt = [bool(v) for v in rng.random(M) < 0.5]
        fo = TO.forward_backward(elp, a, opt, **tab)
        fg = TG.forward_backward(elp, AG.from_optional(a, opt), **tab)
        assert np.isfinite(fo['logz']) == np.isfinite(fg['logz'])
        if np.isfinite(fo['logz']):
            assert abs(fo['logz'] - fg['logz']) <= 1e-12 * max(1.0, abs(fo['logz']))
            assert np.abs(fo['p_used'] - fg['p_used']).max() <= 1e-12


def test_a_trie_is_the_lse_of_its_candidates_and_p_end_their_softmax():
    from action_segmentation_amd import ops
    rng = np.random.default_rng(17)
    for i in range(25):
        T, C, kp = int(rng.integers(4, 8)), 3, 4
        cands = [[int(v) for v in rng.integers(0, C, int(rng.integers(1, 4)))] for _ in range(int(rng.integers(2, 6)))]
        tg = ops.TranscriptGraph.from_candidates(cands)
        assert not tg.is_ambiguous()
        tab = _tables(rng, C, kp, i)
        elp = rng.normal(size=(T, C))
        fb = TG.forward_backward(elp, (tg.ids, tg.pred, tg.start, tg.end), **tab)
        distinct = sorted({tuple(c) for c in cands})
        parts = {}
        for cand in distinct:
            closing = 0.0 if tab['endpen'] is None else float(tab['endpen'][cand[-1]])
            parts[cand] = float(TR.torch_logz(torch.tensor(elp), list(cand), torch.tensor(tab['trans']), torch.tensor(tab['init']),
                                              torch.tensor(tab['len_scores']), kp, closing))
        vals = np.array([parts[c] for c in distinct])
        if not np.isfinite(vals).any():
            assert not np.isfinite(fb['logz'])
            continue
        want = float(TO._lse(vals))
        assert abs(fb['logz'] - want) <= 1e-9 * max(1.0, abs(want))
        soft = np.exp(vals - want)
        for node in np.flatnonzero(tg.end):
            cand = tuple(cands[int(tg.end_candidate[node])])
            assert abs(fb['p_end'][node] - soft[distinct.index(cand)]) <= 1e-9


# ------------------------------------------------------------------------------------------------ ambiguity
def test_is_ambiguous_against_enumeration():
    from action_segmentation_amd import ops
    rng = np.random.default_rng(99)
    n_amb = 0
    for i in range(4000):
        M, C = int(rng.integers(1, 9)), int(rng.integers(1, 4))
        a, pred, start, end = TG.random_graph(rng, M, C, p_edge=(0.2, 0.4, 0.7)[i % 3])
        want = TG.is_ambiguous_brute((a, pred, start, end))
        assert ops.TranscriptGraph(a, pred, start, end).is_ambiguous() == want, (a, pred, start, end)
        n_amb += want
    assert 500 < n_amb < 3500, n_amb
    G = ops.TranscriptGraph
    assert G.from_optional([0, 1, 0], [1, 1, 1]).is_ambiguous()                 # [x?, y?, x?]: either x alone
    assert not G.from_optional([0, 1, 0], [1, 0, 1]).is_ambiguous()
    assert not G.from_candidates([[0, 1], [0, 2], [0, 1, 2]]).is_ambiguous()    # a trie
    assert not G.chain([0, 0, 0]).is_ambiguous()
    assert G([0, 1, 1, 2], [[], [0], [0], [1, 2]], [1, 0, 0, 0], [0, 0, 0, 1]).is_ambiguous()      # a diamond, equal arms
    assert not G([0, 1, 2, 2], [[], [0], [0], [1, 2]], [1, 0, 0, 0], [0, 0, 0, 1]).is_ambiguous()  # ... different arms
    assert G([1, 1], [[], []], [1, 1], [1, 1]).is_ambiguous()                   # two one-node paths of one class
    for ids, opt in (([0, 1, 0, 1], [1, 1, 1, 1]), ([2, 0, 2], [0, 1, 0]), ([0, 0], [1, 1])):
        from action_segmentation_amd.ops import transcript_is_ambiguous
        assert G.from_optional(ids, opt).is_ambiguous() == transcript_is_ambiguous(ids, opt)


# ------------------------------------------------------------------------------------------------ the C entry points
def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _ws(lengths, ms, entry='smm_align_graph_logz_workspace_bytes', **kw):
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    kw.setdefault('total', int(lengths.max()) * len(lengths))
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), **kw)
    return getattr(_lib.load(), entry)(ctypes.byref(shape), _p(lengths), _p(off))


_UNSET = object()


def _call(bwd=False, shape=None, off=_UNSET, elp=POISON, trans=POISON, init=POISON, len_scores=POISON, node_class=POISON,
          pred_mask=POISON, node_flags=POISON, logz=POISON, g_elp=POISON, g_trans=POISON, g_init=POISON, g_len=POISON,
          p_used=None, p_end=None, ws=POISON, ws_bytes=1 << 40, lengths=_UNSET, n_states=_UNSET, frame_off=_UNSET):
    lib = _lib.load()
    lengths = np.array([6], np.int64) if lengths is _UNSET else lengths
    frame_off = np.array([0], np.int64) if frame_off is _UNSET else frame_off
    n_states = np.array([3], np.int32) if n_states is _UNSET else n_states
    off = np.array([0, 2], np.int64) if off is _UNSET else off
    shape = shape or _shape()
    head = (ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), elp, trans, init, len_scores, None,
            node_class, pred_mask, node_flags, _p(off), logz)
    if not bwd:
        return lib.smm_align_graph_logz_f64(*head, ws, ctypes.c_size_t(ws_bytes), POISON)
    return lib.smm_align_graph_logz_bwd_f64(*head, None, g_elp, g_trans, g_init, g_len, p_used, p_end, ws,
                                            ctypes.c_size_t(ws_bytes), POISON)


def test_the_new_symbols_are_exported():
    lib = _lib.load()
    for name in ('smm_align_graph_logz_workspace_bytes', 'smm_align_graph_logz_f64', 'smm_align_graph_logz_bwd_f64'):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None


@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
def test_refuses_bad_arguments_before_staging(bwd):
    names = ['elp', 'trans', 'init', 'len_scores', 'node_class', 'pred_mask', 'node_flags', 'logz', 'ws', 'off', 'lengths',
             'n_states', 'frame_off']
    if bwd:
        names += ['g_elp', 'g_trans', 'g_init', 'g_len']
    for name in names:
        assert _call(bwd, **{name: None}) == ARG, name
    assert _call(bwd, ws_bytes=0) == WORKSPACE                          # (p_used, p_end and grad_logz may be NULL)
    assert _call(bwd, shape=_shape(b=0)) == ARG
    assert _call(bwd, off=np.array([0, 0], np.int64)) == ARG            # M = 0
    assert _call(bwd, off=np.array([2, 1], np.int64)) == ARG            # non-monotone
    two = dict(shape=_shape(b=2), lengths=np.array([6, 6], np.int64), frame_off=np.array([0, 6], np.int64))
    assert _call(bwd, off=np.array([0, 3, 2], np.int64), **two) == ARG
    assert _call(bwd, off=np.array([0, 3, 5], np.int64), ws_bytes=0, **two) == WORKSPACE


@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
def test_refuses_unsupported_shapes_and_short_workspaces_before_staging(bwd):
    assert _call(bwd, shape=_shape(flags=_lib.SHAPE_NO_EOS)) == UNSUPPORTED
    assert _call(bwd, shape=_shape(c=33)) == UNSUPPORTED
    assert _call(bwd, shape=_shape(k_rows=1025)) == UNSUPPORTED
    assert _call(bwd, off=np.array([0, 257], np.int64)) == UNSUPPORTED
    assert _call(bwd, off=np.array([0, 256], np.int64), ws_bytes=0) == WORKSPACE
    need = _ws([6], [2])
    assert need > 0 and _call(bwd, ws_bytes=need - 1) == WORKSPACE      # one byte short
    assert _call(bwd, ws_bytes=_ws([6], [2], entry='smm_align_graph_workspace_bytes')) == WORKSPACE   # (the alignment's is too small)


def test_workspace_bytes():
    """The header's formula: smm_workspace_bytes, the metadata, then 8 (3 M + 4 M (T + 1)) bytes of ranges and columns and
    8 (min(k_rows, T + 1) c_max + c_max^2 + c_max + 1) bytes of parts per video, each area on a multiple of 256."""
    lib = _lib.load()

    def formula(lengths, ms, c=3, k_rows=4):
        lengths = np.asarray(lengths, np.int64)
        b = len(lengths)
        shape = _shape(b=b, c=c, k_rows=k_rows, t_max=int(lengths.max()), total=int(lengths.max()) * b)
        up = lambda x: (x + 255) // 256 * 256
        cur = up(lib.smm_workspace_bytes(ctypes.byref(shape), _p(lengths)))
        cur += 8 * (b + 1) + 8 * b + 8 * b                               # the node, column and part offsets
        cur = up(cur + 4 * b)                                            # the launch order
        cur += 8 * sum(3 * m + 4 * m * (t + 1) for m, t in zip(ms, lengths.tolist()))
        cur = up(cur)
        return cur + 8 * sum(min(k_rows, t + 1) * c + c * c + c + 1 for t in lengths.tolist())

    for lengths, ms, kw in (([6], [2], {}), ([6, 60], [2, 3], dict(c=5)), ([600], [256], {}), ([7, 3, 9], [1, 2, 6], dict(k_rows=9))):
        assert _ws(lengths, ms, **kw) == formula(lengths, ms, **kw), (lengths, ms)
    assert _ws([6], [1]) < _ws([6], [2]) < _ws([6], [6]) < _ws([6], [256])
    assert _ws([6], [3]) < _ws([7], [3]) < _ws([60], [3]) < _ws([600], [3])
    assert _ws([6], [2]) > _ws([6], [2], entry='smm_align_graph_workspace_bytes')
    # 0 on bad arguments
    assert _ws([6], [0]) == 0 and _ws([6], [257]) == 0 and _ws([0], [1]) == 0
    assert _ws([6], [2], flags=_lib.SHAPE_NO_EOS) == 0
    assert _ws([6], [2], c=33) == 0 and _ws([6], [2], k_rows=1025) == 0 and _ws([6], [2], k_rows=1) == 0
    lengths, off = np.array([6], np.int64), np.array([0, 2], np.int64)
    assert lib.smm_align_graph_logz_workspace_bytes(ctypes.byref(_shape(t_max=4)), _p(lengths), _p(off)) == 0
    assert lib.smm_align_graph_logz_workspace_bytes(ctypes.byref(_shape()), None, _p(off)) == 0
    assert lib.smm_align_graph_logz_workspace_bytes(ctypes.byref(_shape()), _p(lengths), None) == 0
    assert lib.smm_align_graph_logz_workspace_bytes(None, _p(lengths), _p(off)) == 0


# ------------------------------------------------------------------------------------------------ Python-level argument checks
def test_ops_value_errors_before_a_device_is_touched():
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 5], [3], 4)
    G = ops.TranscriptGraph
    graphs = [G.chain([0, 1]), G.from_candidates([[2, 2, 1], [2, 0]])]
    off = np.array([0, 2, 6], np.int64)
    assert ops.align_graph_logz_workspace_bytes(batch, off) > ops.align_graph_workspace_bytes(batch, off)
    with pytest.raises(ValueError):
        ops.align_graph_logz_workspace_bytes(batch, off[:-1])
    z = torch.zeros(1, dtype=torch.float64)                                     # (a CPU tensor: no call gets as far as using it)
    with pytest.raises(ValueError, match="1 graphs for 2 videos"):
        ops.align_graph_logz(batch, z, z, z, z, graphs[:1])
    with pytest.raises(ValueError, match="1 graphs for 2 videos"):
        ops.align_graph_logz_bwd(batch, z, z, z, z, graphs[:1], z, ws=z)
    with pytest.raises(ValueError, match="add_eos"):
        ops.align_graph_logz(ops.Batch([6, 5], [3], 4, no_eos=True), z, z, z, z, graphs)
    staged = (torch.zeros(5, dtype=torch.int32), torch.zeros(40, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="staged"):
        ops.align_graph_logz(batch, z, z, z, z, graphs, staged=staged)


def test_module_checks_fire_before_a_device_is_touched():
    """The number of graphs, their type and ambiguous='raise' are host arithmetic: a corpus whose features sit on the CPU gets
    as far as them and no further (the next check would refuse the CPU tensor with another message)."""
    from module_util import make_args
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    G = ops.TranscriptGraph
    m = SemiMarkovModule(make_args(6), 4, 3, allow_self_transitions=True)
    pc = types.SimpleNamespace(video_names=['v0', 'v1'], batch=None, x=torch.zeros(1))
    amb = G.from_optional([0, 1, 0], [1, 1, 1])
    ok = G.from_candidates([[2, 3], [2, 1]])
    for fn in (m.transcript_graph_log_partition_packed, m.transcript_graph_scores_packed):
        with pytest.raises(ValueError, match="'v0'"):
            fn(pc, [amb, ok])
        with pytest.raises(ValueError, match="1 graphs for 2 videos"):
            fn(pc, [ok])
        with pytest.raises(ValueError, match="ambiguous"):
            fn(pc, [ok, ok], ambiguous='maybe')
        with pytest.raises(ValueError, match="'v1'"):
            fn(pc, [ok, [2, 3]])
    with pytest.raises(ValueError, match="1 graphs for 2 videos"):
        m.transcript_node_posteriors_packed(pc, [ok])
    x = torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="video 0"):
        m.transcript_graph_log_partition(x, torch.tensor([5, 5]), None, [amb, ok])
    with pytest.raises(ValueError, match="add_eos"):
        m.transcript_graph_log_partition(x, torch.tensor([5, 5]), None, [ok, ok], add_eos=False)
    with pytest.raises(ValueError, match="transcript_graphs alone"):
        m.log_likelihood(x, torch.tensor([5, 5]), None, transcripts=[[0], [1]], transcript_graphs=[ok, ok])


def test_candidate_chunks_drop_duplicates_across_chunks():
    """Candidates are de-duplicated before they are split into tries of at most MAX_TRANSCRIPT nodes: a class sequence that
    comes again behind a split is in no later trie, and every trie fits."""
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    chunk = SemiMarkovModel._candidate_chunks
    assert chunk([[0, 1], [0, 1], [0, 2]], 'v', 'f') == [[(0, (0, 1)), (2, (0, 2))]]
    long = lambda c: [c] * 100                                                   # 100 trie nodes each, no shared prefix
    cands = [long(0), long(1), [5, 6], long(2), long(0), [5, 6], long(3), torch.tensor(long(1))]
    got = chunk(cands, 'v', 'f')
    assert [[ci for ci, _ in part] for part in got] == [[0, 1, 2], [3, 6]]
    for part in got:
        assert ops.TranscriptGraph.trie_nodes([seq for _, seq in part]) <= ops.MAX_TRANSCRIPT
    assert len({seq for part in got for _, seq in part}) == sum(len(part) for part in got) == 5
    for bad in ([], [[]], [[0] * 257]):
        with pytest.raises(ValueError, match="'v'"):
            chunk(bad, 'v', 'f')
