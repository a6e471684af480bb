"""Segment and boundary posteriors (smm_segment_posteriors_f64) without a GPU: the two statements of the numpy reference
against each other and against the C twin, the identities that tie them to the log-partition gradient, the exported symbol,
every refusal of the entry point (one fault per call, poison device pointers: a refused call touches none), and the Python
layer's checks, which fire before a device is touched."""
import ctypes

import numpy as np
import pytest
import torch

from action_segmentation_amd import _lib
from oracle import factored as F

import segment_posterior_ref as R

TOL = 1e-9                     # between two exact fp64 statements: the host tests' bar
NEG_INF = float('-inf')


def _random_lattice(seed):
    g = np.random.default_rng(seed)
    c = int(g.integers(1, 4))
    no_eos = bool(g.integers(0, 2))
    frames = int(g.integers(2, 8))
    kp = min(int(g.integers(2, 5)), frames)
    elp = g.normal(size=(frames, c))
    trans = g.normal(size=(c, c))
    init = g.normal(size=c)
    lens = g.normal(size=(kp, c))
    ep = None if no_eos or g.integers(0, 2) else g.normal(size=c)
    # -inf entries: a few cells of each table (not of elp: the recursions take differences of its prefix sums)
    for a, p in ((trans, 0.15), (init, 0.15), (lens[1:], 0.12)):
        a[g.random(a.shape) < p] = NEG_INF
    if ep is not None:
        ep[g.random(c) < 0.2] = NEG_INF
    return elp, trans, init, lens, ep, no_eos


CASES = [_random_lattice(s) for s in range(300)]


def test_recursions_agree_with_enumeration_on_300_lattices():
    finite = 0
    for elp, trans, init, lens, ep, no_eos in CASES:
        a = R.Recursions(elp, trans, init, lens, ep, no_eos)
        b = R.enumerate_posteriors(elp, trans, init, lens, ep, no_eos)
        if b['logz'] == NEG_INF:
            assert a.logz == NEG_INF
            continue
        if b['logz'] < -1e8:                   # all mass on the -1e9 closing alternative: sums carry ulp(1e9) = 1.2e-7
            continue
        finite += 1
        assert abs(a.logz - b['logz']) <= TOL
        np.testing.assert_allclose(a.start_post, b['start_post'], rtol=0, atol=TOL)
        np.testing.assert_allclose(a.end_post, b['end_post'], rtol=0, atol=TOL)
        np.testing.assert_allclose(a.bnd_post, b['bnd_post'], rtol=0, atol=TOL)
        assert abs(a.bnd_post[0] - 1.0) <= TOL
        frames, c = elp.shape
        t = frames - (1 if no_eos else 0)
        for j in range(c):
            for s in range(t):
                for e in range(s + 1, t + 1):
                    pa = R._exp(a.span_logp(j, s, e))
                    assert abs(pa - b['spans'].get((j, s, e), 0.0)) <= TOL, (j, s, e)
        if no_eos:
            for to in range(c):
                assert abs(R._exp(a.closing_logp(to)) - b['closing'][to]) <= TOL
        # every path's spans as one row of a span encoding: both statements of seg_logp
        segs, to, _ = b['paths'][len(b['paths']) // 2]
        row = np.full(frames + 1, -1, np.int64)
        for (j, s, e) in segs:
            row[s] = j
        row[t] = to if no_eos else c
        la, lb = R.spans_logp(a, row, frames, no_eos, frames + 1), R.spans_logp(b, row, frames, no_eos, frames + 1)
        np.testing.assert_allclose(np.exp(la), np.exp(lb), rtol=0, atol=TOL)
    assert finite >= 200, finite


def _twin(elp, trans, init, lens, ep, no_eos):
    frames = elp.shape[0]
    return F.logz(elp[None], np.array([frames]), trans, init, lens, endpen=None if ep is None else ep[None], grad=True,
                  starts=True, no_eos=no_eos)


def test_twin_start_posteriors_and_identities():
    """The C twin's g['start'] is (a)'s start_post; the occupancy is cumsum(start) - cumsum(end) shifted by one frame; the
    expected number of segments is sum(start_post) = sum(g_len)."""
    finite = 0
    for elp, trans, init, lens, ep, no_eos in CASES:
        a = R.Recursions(elp, trans, init, lens, ep, no_eos)
        if a.logz < -1e8:                      # -inf, or all mass on the -1e9 closing alternative (ulp(1e9) = 1.2e-7)
            continue
        finite += 1
        z, g = _twin(elp, trans, init, lens, ep, no_eos)
        frames = elp.shape[0]
        t = frames - (1 if no_eos else 0)
        assert abs(z[0] - a.logz) <= TOL
        np.testing.assert_allclose(g['start'][0, :t], a.start_post[:t], rtol=0, atol=TOL)
        cs = np.cumsum(a.start_post[:t], axis=0)
        ce = np.concatenate([np.zeros((1, elp.shape[1])), np.cumsum(a.end_post[:t], axis=0)[:-1]])
        np.testing.assert_allclose(g['elp'][0, :t], cs - ce, rtol=0, atol=TOL)
        np.testing.assert_allclose(a.occupancy[:t], cs - ce, rtol=0, atol=TOL)
        if no_eos:
            np.testing.assert_allclose(g['elp'][0, t], a.start_post[t], rtol=0, atol=TOL)
        assert abs(a.start_post[:t].sum() - g['len'].sum()) <= TOL
        np.testing.assert_allclose(a.g_len, g['len'], rtol=0, atol=TOL)
    assert finite >= 200, finite


def test_symbol_is_exported():
    assert 'smm_segment_posteriors_f64' in _lib.SYMBOLS
    assert _lib.load().smm_segment_posteriors_f64 is not None


# ---------------------------------------------------------------------------------------------------------------- refusals
P = ctypes.c_void_p(16)                           # (never dereferenced: the arguments are refused first)
ARG = -1


def _call(shape_kw=None, shape_null=False, **fault):
    host = dict(lengths=np.array([6], np.int64), frame_off=np.array([0], np.int64), n_states=np.array([3], np.int32))
    sk = dict(b=1, d=0, n_groups=1, c_max=3, k_rows=4, t_max=6, flags=0, total_frames=6)
    sk.update(shape_kw or {})
    shape = _lib.SmmShape(*[sk[f] for f in ('b', 'd', 'n_groups', 'c_max', 'k_rows', 't_max', 'flags', 'total_frames')])
    for name in list(fault):
        if name in host:
            host[name] = fault.pop(name)
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    v = dict(elp=P, trans=P, init=P, len_scores=P, endpen=None, class_map=None, logz=P, spans_in=P, n_sets=2, start_post=P,
             end_post=P, bnd_post=P, seg_logp=P, ws=P)
    assert set(fault) <= set(v), sorted(fault)
    v.update(fault)
    return _lib.load().smm_segment_posteriors_f64(
        None if shape_null else ctypes.byref(shape), ptr(host['lengths']), ptr(host['frame_off']), None, None,
        ptr(host['n_states']), v['elp'], v['trans'], v['init'], v['len_scores'], v['endpen'], v['class_map'], v['logz'],
        v['spans_in'], ctypes.c_int32(v['n_sets']), v['start_post'], v['end_post'], v['bnd_post'], v['seg_logp'], v['ws'],
        ctypes.c_size_t(1 << 40), None)


REFUSALS = [
    dict(elp=None), dict(trans=None), dict(init=None), dict(len_scores=None), dict(logz=None),
    dict(start_post=None, end_post=None, bnd_post=None, seg_logp=None),
    dict(start_post=None, end_post=None, bnd_post=None, seg_logp=None, spans_in=None),
    dict(spans_in=None),                                    # seg_logp without spans_in
    dict(n_sets=0), dict(n_sets=-3),
    dict(shape_null=True), dict(shape_kw=dict(b=0)), dict(shape_kw=dict(k_rows=1)),
    dict(lengths=None), dict(frame_off=None), dict(n_states=None), dict(ws=None),
]


@pytest.mark.parametrize('fault', REFUSALS, ids=['-'.join(sorted(f)) + str(i) for i, f in enumerate(REFUSALS)])
def test_single_fault_is_refused(fault):
    assert _call(**fault) == ARG


# ------------------------------------------------------------------------------------------------------------ Python layer
def test_python_checks_fire_before_a_device_is_touched(monkeypatch):
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 4], [3], 4)
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail("the library was loaded before the arguments were checked"))
    f = lambda *s: torch.zeros(*s, dtype=torch.float64)
    elp, trans, init, lens, z = f(12, 3), f(1, 3, 3), f(1, 3), f(1, 4, 3), f(2)
    with pytest.raises(TypeError):
        ops.segment_posteriors(batch, elp, trans, init, lens, z, spans=torch.zeros(2, 7, dtype=torch.int32))
    with pytest.raises(ValueError):
        ops.segment_posteriors(batch, elp, trans, init, lens, z, spans=torch.zeros(2, 6, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.segment_posteriors(batch, elp, trans, init, lens, z, spans=torch.zeros(3, 3, 7, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.segment_posteriors(batch, elp, trans, init, lens, z, spans=torch.zeros(0, 2, 7, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.segment_posteriors(batch, f(11, 3), trans, init, lens, z)


# ================================================================================================ the transcript-graph family
import transcript_graph_ref as TG                                  # noqa: E402
import transcript_segment_posterior_ref as TR                      # noqa: E402


def _random_dag_case(seed):
    g = np.random.default_rng(1000 + seed)
    c = int(g.integers(1, 4))
    t = int(g.integers(2, 8))
    m = int(g.integers(1, 7))
    kp = int(g.integers(2, 5))
    graph = TG.random_graph(g, m, c)
    elp = g.normal(size=(t, c))
    trans, init, lens = g.normal(size=(c, c)), g.normal(size=c), g.normal(size=(kp, c))
    ep = None if g.integers(0, 2) else g.normal(size=c)
    return elp, graph, trans, init, lens, kp, ep


def test_graph_references_agree_on_300_dags():
    """(b) forward-backward against (d) brute force on 300 random DAGs that admit an alignment (the others: both say -inf): E, S,
    every segment's marginal; and per node sum_n E = p_used."""
    finite = 0
    for seed in range(2000):
        if finite == 300:
            break
        elp, graph, trans, init, lens, kp, ep = _random_dag_case(seed)
        a = TR.from_forward_backward(elp, graph, trans, init, lens, kp, ep)
        b = TR.brute_force(elp, graph, trans, init, lens, kp, ep)
        f = TR.from_forward_backward(elp, graph, trans, init, lens, kp, ep, fast=True)     # the array statement of (b)
        assert np.isfinite(f['logz']) == np.isfinite(a['logz'])
        if np.isfinite(f['logz']):
            np.testing.assert_allclose(f['E'], a['E'], rtol=0, atol=TOL)
            np.testing.assert_allclose(f['S'], a['S'], rtol=0, atol=TOL)
        if not np.isfinite(b['logz']):
            assert not np.isfinite(a['logz'])
            continue
        finite += 1
        t, m = elp.shape[0], len(graph[0])
        assert abs(a['logz'] - b['logz']) <= TOL
        np.testing.assert_allclose(a['E'], b['E'], rtol=0, atol=TOL)
        np.testing.assert_allclose(a['S'], b['S'], rtol=0, atol=TOL)
        np.testing.assert_allclose(a['E'].sum(axis=0), a['p_used'], rtol=0, atol=TOL)
        np.testing.assert_allclose(b['E'].sum(axis=0), a['S'].sum(axis=0), rtol=0, atol=TOL)
        for node in range(m):
            for s in range(t):
                for e in range(s + 1, t + 1):
                    assert abs(R._exp(a['seg'](node, s, e)) - b['segs'].get((node, s, e), 0.0)) <= TOL, (seed, node, s, e)
            for col in ('E', 'S'):
                ma, mb = TR.moments(a[col][:, node]), TR.moments(b[col][:, node])
                if b[col][:, node].sum() > 1e-6:
                    assert abs(ma[0] - mb[0]) <= 1e-6 and abs(ma[1] - mb[1]) <= 1e-6
    assert finite == 300, finite


def test_graph_symbol_is_exported():
    assert 'smm_align_graph_segment_posteriors_f64' in _lib.SYMBOLS
    assert _lib.load().smm_align_graph_segment_posteriors_f64 is not None


def _gcall(shape_kw=None, shape_null=False, **fault):
    host = dict(lengths=np.array([6], np.int64), frame_off=np.array([0], np.int64), n_states=np.array([3], np.int32),
                noff=np.array([0, 2], np.int64))
    sk = dict(b=1, d=0, n_groups=1, c_max=3, k_rows=4, t_max=6, flags=0, total_frames=6)
    sk.update(shape_kw or {})
    shape = _lib.SmmShape(*[sk[f] for f in ('b', 'd', 'n_groups', 'c_max', 'k_rows', 't_max', 'flags', 'total_frames')])
    for name in list(fault):
        if name in host:
            host[name] = fault.pop(name)
    ptr = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    outs = ('seg_logp', 'node_logp', 'end_mean', 'end_sd', 'start_mean', 'start_sd', 'node_end_post', 'node_start_post')
    v = dict(elp=P, trans=P, init=P, len_scores=P, endpen=None, class_map=None, node_class=P, pred_mask=P, node_flags=P, logz_g=P,
             spans_in=P, used_in=P, n_sets=2, ws=P, **{k: P for k in outs})
    assert set(fault) <= set(v), sorted(fault)
    v.update(fault)
    return _lib.load().smm_align_graph_segment_posteriors_f64(
        None if shape_null else ctypes.byref(shape), ptr(host['lengths']), ptr(host['frame_off']), None, None,
        ptr(host['n_states']), v['elp'], v['trans'], v['init'], v['len_scores'], v['endpen'], v['class_map'], v['node_class'],
        v['pred_mask'], v['node_flags'], ptr(host['noff']), v['logz_g'], v['spans_in'], v['used_in'], ctypes.c_int32(v['n_sets']),
        *[v[k] for k in outs], v['ws'], ctypes.c_size_t(1 << 40), None)


_NO_OUT = dict(seg_logp=None, node_logp=None, end_mean=None, end_sd=None, start_mean=None, start_sd=None, node_end_post=None,
               node_start_post=None)
GRAPH_REFUSALS = [
    dict(_NO_OUT), dict(spans_in=None, used_in=None),              # every output NULL; seg_logp without its alignments
    dict(spans_in=None), dict(used_in=None), dict(n_sets=0),
    dict(elp=None), dict(trans=None), dict(init=None), dict(len_scores=None), dict(logz_g=None), dict(node_class=None),
    dict(pred_mask=None), dict(node_flags=None), dict(noff=None), dict(lengths=None), dict(frame_off=None), dict(n_states=None),
    dict(ws=None), dict(shape_null=True), dict(shape_kw=dict(b=0)), dict(shape_kw=dict(flags=_lib.SHAPE_NO_EOS)),
]


@pytest.mark.parametrize('fault', GRAPH_REFUSALS, ids=[str(i) + '-' + '-'.join(sorted(f))[:40] for i, f in enumerate(GRAPH_REFUSALS)])
def test_graph_single_fault_is_refused(fault):
    assert _gcall(**fault) in (-1, -2)                             # SMM_ERR_ARG; NO_EOS: SMM_ERR_UNSUPPORTED as its siblings


def test_graph_python_checks_fire_before_a_device_is_touched(monkeypatch):
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 4], [3], 4)
    monkeypatch.setattr(_lib, 'load', lambda: pytest.fail("the library was loaded before the arguments were checked"))
    f = lambda *s: torch.zeros(*s, dtype=torch.float64)
    elp, trans, init, lens, z = f(12, 3), f(1, 3, 3), f(1, 3), f(1, 4, 3), f(2)
    graphs = [ops.TranscriptGraph.chain([0, 1]), ops.TranscriptGraph.chain([2])]
    spans, used = torch.zeros(2, 7, dtype=torch.int64), torch.zeros(3, dtype=torch.int32)
    call = lambda **kw: ops.align_graph_segment_posteriors(batch, elp, trans, init, lens, graphs, z, **kw)
    with pytest.raises(ValueError):
        call(spans=spans)                                          # spans without used
    with pytest.raises(ValueError):
        call(want_moments=False)                                   # nothing asked for
    with pytest.raises(TypeError):
        call(spans=spans, used=used.long())
    with pytest.raises(ValueError):
        call(spans=spans[:, :6], used=used)
    with pytest.raises(ValueError):
        call(spans=spans, used=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError):
        call(spans=spans, used=used)                               # no workspace of the forward call
