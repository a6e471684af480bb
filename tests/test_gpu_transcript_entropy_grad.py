"""Gradients of the entropy, cross-entropy and KL of transcript-graph posteriors on the GPU (smm_align_graph_entropy_bwd_f64,
smm_align_graph_kl_bwd_f64) against the three routes of tests/transcript_entropy_grad_ref.py: (a) autograd through the
enumeration on the tiny graphs, (b) log Z_g differentiated twice on the shapes that cross a work split.  q's gradient is
mu_q - mu_p from two align_graph_logz_bwd calls.

Bars: 1e-4 of max(1, max |ref|) per table, and 1e-5 max(1, |V|) for ``value`` against align_graph_entropy / align_graph_kl: the
family's own bars.  Every test prints its figures ("[transcript-entropy-grad] ...") before it asserts."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_transcript_graph as GT
import test_gpu_transcript_kl as GK
import test_gpu_transcript_sample as GS
import transcript_entropy_grad_ref as R
from test_gpu_transcript_graph import Case, _lists, _ops, _tables, _tuple

pytestmark = pytest.mark.gpu
TAB_BAR, VAL_BAR, NEAR_BAR = 1e-4, 1e-5, 1e-3
KEYS = R.KEYS


# ------------------------------------------------------------------------------------------------ launching
def _launch(pc, qc, mode, batch, dp, fp, dq=None, fq=None, u='case', scratch=None):
    ops = _ops()
    grad_out = dp['u'] if isinstance(u, str) else u
    if mode == 'entropy':
        return ops.align_graph_entropy_bwd(batch, dp['elp'], dp['trans'], dp['init'], dp['len'], pc.graphs, fp['logz'],
                                           grad_out=grad_out, endpen=dp['endpen'], ws=fp['ws'], staged=fp['_staged'], scratch=scratch)
    return ops.align_graph_kl_bwd(batch, GK._p_side(dp, fp), GK._q_side(dq, fq), pc.graphs, grad_out=grad_out,
                                  staged=fp['_staged'], cross_entropy=mode == 'xent', scratch=scratch)


def _host(batch, out):
    h = {k: out[k].cpu().numpy() for k in KEYS + ('value', 'value_plus')}
    h['err'] = _ops().error_flag(batch, out)
    return h


def _run(pc, qc, mode, fill=None):
    batch, dp, fp = GS._forward(pc, fill)
    dq = fq = None
    if mode != 'entropy':
        _, dq, fq = GS._forward(qc, fill)
    return _host(batch, _launch(pc, qc, mode, batch, dp, fp, dq, fq))


def _value_call(pc, qc, mode):
    """The value by the value calls: align_graph_entropy, or align_graph_kl's KL / cross-entropy."""
    batch, dp, fp = GS._forward(pc)
    if mode == 'entropy':
        return GK._entropy(pc, batch, dp, fp)['entropy'].cpu().numpy()
    _, dq, fq = GS._forward(qc)
    out = GK._kl(pc, batch, dp, fp, dq, fq)
    return out['kl' if mode == 'kl' else 'cross_entropy'].cpu().numpy()


def reference(pc, qc, mode, route):
    """-> (V [b], dict(elp [total, cm], trans, init, len [g, ...])) by ``route`` per video, times u, summed per group."""
    g_n, cm = len(pc.tabs), pc.cm
    val = np.zeros(len(pc.vids))
    g = dict(elp=np.zeros((int(pc.off[-1]), cm)), trans=np.zeros((g_n, cm, cm)), init=np.zeros((g_n, cm)),
             len=np.zeros((g_n, pc.k_rows, cm)))
    for i, (e, gr, j) in enumerate(pc.vids):
        c = pc.n_states[j]
        r = route(GK.side(pc, i), None if qc is None else GK.side(qc, i), _tuple(gr), pc.kp(i), mode)
        val[i], gi = r[0], r[1]
        u = 1.0 if pc.u is None else float(pc.u[i])
        g['elp'][pc.off[i]:pc.off[i + 1], :c] += u * gi['elp']
        g['trans'][j, :c, :c] += u * gi['trans']
        g['init'][j, :c] += u * gi['init']
        g['len'][j, :, :c] += u * gi['len']
    return val, g


def _errors(h, val, ref):
    return {k: float(np.abs(h[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())) for k in KEYS}


def _check(what, h, val, ref, value_ref=None, zero=(), premise=True):
    """The bars; and the premise of the relative bar, from the reference alone: every reference table has an entry of at least
    1e-2, but for the tables ``zero`` declares zero by structure."""
    e = _errors(h, val, ref)
    ev = float((np.abs(h['value'] - val) / np.maximum(1.0, np.abs(val))).max())
    ep = float((np.abs(h['value'] - h['value_plus']) / np.maximum(1.0, np.abs(val))).max())
    ec = 0.0 if value_ref is None else float((np.abs(h['value'] - value_ref) / np.maximum(1.0, np.abs(value_ref))).max())
    print('\n[transcript-entropy-grad] %-44s elp %.1e trans %.1e init %.1e len %.1e (bar %.0e)  V against ref %.1e, the value '
          'call %.1e, V+ %.1e (bar %.0e)  max|ref| %s' % (what, e['elp'], e['trans'], e['init'], e['len'], TAB_BAR, ev, ec, ep, VAL_BAR,
                                                         ' '.join('%.2g' % np.abs(ref[k]).max() for k in KEYS)))
    assert h['err'] == 0
    assert not premise or all(np.abs(ref[k]).max() >= 1e-2 for k in KEYS if k not in zero), what
    assert max(e.values()) <= TAB_BAR and max(ev, ec, ep) <= VAL_BAR
    return e


# ------------------------------------------------------------------------------------------------ 1. tiny graphs
@functools.lru_cache(None)
def tiny_reference(which, mode, near):
    _, pc, far, nr, names, _, _ = GK.tiny_pairs()[which]
    qc = nr if near else far
    return reference(pc, qc, mode, R.enumeration_grads)


@pytest.mark.parametrize('mode,near', [('entropy', False), ('xent', False), ('xent', True), ('kl', False), ('kl', True)],
                         ids=['entropy', 'xent-far', 'xent-near', 'kl-far', 'kl-near'])
@pytest.mark.parametrize('which', [0, 1], ids=['k_rows4', 'k_rows8'])
def test_tiny_graphs_against_enumeration(which, mode, near):
    """The sampler's tiny graphs (one of them under end penalties): p's four gradients and V against autograd through the
    enumerated value; q an independent draw, or p moved by 1e-3 sigma."""
    _, pc, far, nr, names, _, _ = GK.tiny_pairs()[which]
    qc = nr if near else far
    val, ref = tiny_reference(which, mode, near)
    h = _run(pc, qc, mode)
    small = mode == 'kl' and near
    _check('tiny %s %s %s' % (('k_rows4', 'k_rows8')[which], mode, 'near' if near else 'far'), h, val, ref, _value_call(pc, qc, mode),
           premise=not small)
    if small:
        # a gradient of the size of the move (max |ref| 2e-4 .. 2e-3): the absolute bar would pass a wrong table, so these
        # tables are held to NEAR_BAR of their own largest entry.  1e-3: the forward kernel's fp32 exponentials leave about
        # 6e-8 relative in p(o) per column, a few 1e-8 absolute in a table whose terms are of order 1 before they
        # cancel, against entries of 2e-4: 1e-4 .. 5e-4 relative; it is also the family's bar for near-identical sides (4q)
        rel = {k: float(np.abs(h[k] - ref[k]).max() / np.abs(ref[k]).max()) for k in KEYS}
        print('\n[transcript-entropy-grad] ... relative to max |ref|: %s (bar %.0e)' % (rel, NEAR_BAR))
        assert max(rel.values()) <= NEAR_BAR


@pytest.mark.parametrize('which', [0, 1], ids=['k_rows4', 'k_rows8'])
def test_q_s_gradient_is_the_difference_of_the_marginals(which):
    """dH(p, q) / d theta_q = dKL / d theta_q = mu_q - mu_p from two align_graph_logz_bwd calls, against autograd through the
    enumeration."""
    _, pc, qc, _, names, _, _ = GK.tiny_pairs()[which]
    mu = []
    for c in (pc, qc):
        batch, d, f = GS._forward(c)
        g = GK._backward(c, batch, d, f)
        mu.append({k: g[k].cpu().numpy() for k in KEYS})
    for mode in ('xent', 'kl'):
        g_n, cm = len(pc.tabs), pc.cm
        ref = dict(elp=np.zeros((int(pc.off[-1]), cm)), trans=np.zeros((g_n, cm, cm)), init=np.zeros((g_n, cm)),
                   len=np.zeros((g_n, pc.k_rows, cm)))
        for i, (e, gr, j) in enumerate(pc.vids):
            c = pc.n_states[j]
            gq = R.enumeration_grads(GK.side(pc, i), GK.side(qc, i), _tuple(gr), pc.kp(i), mode)[2]
            ref['elp'][pc.off[i]:pc.off[i + 1], :c] += gq['elp']
            ref['trans'][j, :c, :c] += gq['trans']
            ref['init'][j, :c] += gq['init']
            ref['len'][j, :, :c] += gq['len']
        err = {k: float(np.abs((mu[1][k] - mu[0][k]) - ref[k]).max() / max(1.0, np.abs(ref[k]).max())) for k in KEYS}
        print('\n[transcript-entropy-grad] q side, %s: %s (bar %.0e)' % (mode, err, TAB_BAR))
        assert max(err.values()) <= TAB_BAR


@pytest.mark.parametrize('mask', [-1e9, -np.inf], ids=['m1e9', 'minf'])
@pytest.mark.parametrize('mode', R.MODES)
def test_masked_entries_against_enumeration(mode, mask):
    """A diamond and a trie with one arm cut on BOTH sides by a -1e9 or -inf transition: the twice-differentiated identity is
    wrong by tens of nats here, the enumeration is not."""
    G = _ops().TranscriptGraph
    rng = np.random.default_rng(39)
    C, K = 3, 5
    vids = [(rng.normal(size=(7, C)) * 1.2, _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 2, 0]), 0),
            (rng.normal(size=(6, C)) * 1.2, G.from_candidates([[0, 1, 2], [0, 2, 1], [1, 0]]), 1)]

    def cut(seed):
        r = np.random.default_rng(seed)
        t1, t2 = _tables(r, C, K, 1.2), _tables(r, C, K, 1.2)
        t1['trans'][1, 0] = mask
        t2['trans'][2, 0] = mask
        return [t1, t2]

    pc = Case(vids, cut(40), K, kps=[5, 5])
    qc = Case([(rng.normal(size=e.shape), g, j) for e, g, j in vids], cut(41), K, kps=[5, 5])
    val, ref = reference(pc, qc, mode, R.enumeration_grads)
    h = _run(pc, qc, mode)
    _check('masked %s %s' % (mode, mask), h, val, ref, _value_call(pc, qc, mode))
    assert h['trans'][0, 1, 0] == 0.0 and h['trans'][1, 2, 0] == 0.0


# ------------------------------------------------------------------------------------------------ 2. work splits
def _two_start_classes(g, C):
    """The graph with node 1 of another class than node 0 (both are start nodes of a branching graph): g_init is not zero."""
    ids = np.array(g.ids).copy()
    ids[1] = (ids[0] + 1) % C
    return _ops().TranscriptGraph(ids, g.pred, g.start, g.end)


def _tile(T, seed):
    """T around the family's tile of 768 positions with kp = 64 and M = 20 on a branching graph."""
    rng = np.random.default_rng(seed)
    C, K = 4, 64
    return Case([(rng.normal(size=(T, C)) * 0.3, _two_start_classes(GT._branching(rng, 20, C), C), 0)], [_tables(rng, C, K, 0.5)], K)


def _halo():
    """T = 1100, kp = 1024, M = 3: two start nodes into one end node."""
    rng = np.random.default_rng(HALO_SEED)
    C, K = 4, 1024
    graph = _lists(3, [[], [], [0, 1]], [0, 1], [2], ids=[0, 1, 2])
    return Case([(rng.normal(size=(1100, C)) * HALO_SCALES[0], graph, 0)], [_tables(rng, C, K, HALO_SCALES[1])], K)


def _fan():
    """M = 256: 255 start nodes into one end node at T = 10."""
    rng = np.random.default_rng(41)
    return Case([(rng.normal(size=(10, 3)) * 0.3, GS._wide('fan', rng), 0)], [_tables(rng, 3, 10, 0.5)], 10)


def _chain():
    """M = 256: a chain of 256 at T = 300, kp = 8."""
    rng = np.random.default_rng(21)
    C, K = 5, 8
    return Case([(rng.normal(size=(300, C)) * 2.0, _ops().TranscriptGraph.chain(rng.integers(0, C, 256)), 0)], [_tables(rng, C, K, 1.0)], K)


def _dense():
    """M = 64 with every pair an edge, every node a start and an end, at T = 80: 2016 edges through the g_trans block sums."""
    rng = np.random.default_rng(1)
    C, K = 5, 8
    graph = _ops().TranscriptGraph(rng.integers(0, C, 64), np.tril(np.ones((64, 64), bool), k=-1), np.ones(64, bool), np.ones(64, bool))
    return Case([(rng.normal(size=(80, C)), graph, 0)], [_tables(rng, C, K, 1.0)], K)


def _states32():
    """32 states: 1024 class pairs."""
    rng = np.random.default_rng(1)
    C, K = 32, 12
    return Case([(rng.normal(size=(90, C)) * 0.5, _two_start_classes(GT._branching(rng, 40, C), C), 0)], [_tables(rng, C, K, 0.5)], K)


HALO_SEED, HALO_SCALES = 2, (0.05, 1.0)
# name -> (builder, modes, the tables that are zero by structure); seeds chosen so that every other reference table has an entry
# of at least 1e-2 (tests/test_transcript_entropy_grad_host.py holds that)
BIG_CASES = {
    'T767': (lambda: _tile(767, 6), ('kl',), ()),
    'T768': (lambda: _tile(768, 5), ('kl',), ()),
    'T769': (lambda: _tile(769, 4), R.MODES, ()),
    'T771': (lambda: _tile(771, 6), ('kl',), ()),
    'halo': (_halo, ('kl',), ()),
    'fan': (_fan, ('entropy', 'kl'), ()),
    'chain': (_chain, ('entropy', 'kl'), ('trans', 'init')),
    'dense': (_dense, ('entropy', 'kl'), ()),
    'states32': (_states32, ('entropy', 'kl'), ()),
}


@pytest.mark.parametrize('name', list(BIG_CASES))
def test_work_splits_against_the_identity(name):
    """The smallest shapes that cross each boundary, against log Z_g differentiated twice; q an independent draw.  A table that
    is zero by structure (the chain's g_trans and g_init) is held to the same absolute 1e-4; what is left in it is printed."""
    build, modes, zero = BIG_CASES[name]
    pc = build()
    qc = GK.other_side(pc, 5)
    for mode in modes:
        val, ref = reference(pc, qc, mode, R.identity_grads)
        h = _run(pc, qc, mode)
        _check('%s %s' % (name, mode), h, val, ref, _value_call(pc, qc, mode), zero=zero)
        for k in zero:
            print('\n[transcript-entropy-grad] ... %s is zero by structure: max |g| %.1e' % (k, np.abs(h[k]).max()))
            assert np.abs(h[k]).max() <= TAB_BAR


# ------------------------------------------------------------------------------------------------ 3. a packed corpus
def _corpus(bad, u):
    """Two class sets (6 and 17 states under c_max 17), ragged lengths, per-video span limits; with ``bad`` a video without an
    alignment (a chain of 5 over 3 frames) and one whose elp holds a NaN sit between the healthy ones."""
    G = _ops().TranscriptGraph
    rng = np.random.default_rng(91)
    tabs = [_tables(rng, 6, 12, 1.0), _tables(rng, 17, 12, 1.0)]
    vids = [(rng.normal(size=(23, 6)), GT._branching(rng, 7, 6), 0), (rng.normal(size=(31, 17)), GT._branching(rng, 9, 17), 1),
            (rng.normal(size=(17, 6)), G.from_candidates([[0, 1, 2], [3, 4], [5, 0, 1, 2]]), 0),
            (rng.normal(size=(40, 17)), GT._branching(rng, 12, 17), 1)]
    kps = [9, 12, 7, 11]
    if bad:
        nan = rng.normal(size=(9, 17))
        nan[4, 2] = np.nan
        vids = [vids[0], (rng.normal(size=(3, 6)), G.chain([0, 1, 2, 3, 4]), 0), vids[1], vids[2], (nan, GT._branching(rng, 4, 17), 1),
                vids[3]]
        kps = [9, 4, 12, 7, 6, 11]
        u = None if u is None else np.insert(np.insert(np.asarray(u, np.float64), 1, 1.0), 4, 1.0)
    return Case(vids, tabs, 12, kps=kps, u=u)


@pytest.mark.parametrize('mode', R.MODES)
def test_a_packed_corpus_with_an_upstream_zero_and_bad_videos(mode):
    u = [0.7, 0.0, -1.3, 2.0]
    good = _corpus(False, u)
    qgood = GK.other_side(good, 3)
    val, ref = reference(good, qgood, mode, R.identity_grads)
    h = _run(good, qgood, mode)
    _check('packed corpus %s' % mode, h, val, ref, _value_call(good, qgood, mode))
    o = good.off
    assert not h['elp'][o[1]:o[2]].any() and not np.signbit(h['elp'][o[1]:o[2]]).any()      # (u = 0: exact zeros)
    bad = _corpus(True, u)
    qbad = GK.other_side(bad, 3)
    for (e, _, _), (eq, _, _), i in zip(good.vids, qgood.vids, (0, 2, 3, 5)):                    # (the same healthy inputs on both sides)
        qbad.vids[i] = (eq, qbad.vids[i][1], qbad.vids[i][2])
        assert np.array_equal(bad.vids[i][0], e)
    qbad.tabs = qgood.tabs
    hb = _run(bad, qbad, mode)
    ob = bad.off
    print('\n[transcript-entropy-grad] bad videos, %s: values %s, error word %d' % (mode, hb['value'], hb['err']))
    assert hb['err'] != 0 and np.isnan(hb['value'][1]) and np.isnan(hb['value'][4])
    assert not hb['elp'][ob[1]:ob[2]].any() and not hb['elp'][ob[4]:ob[5]].any()
    for i, j in zip(range(4), (0, 2, 3, 5)):
        assert np.array_equal(h['elp'][o[i]:o[i + 1]], hb['elp'][ob[j]:ob[j + 1]])
        assert h['value'][i] == hb['value'][j]
    for k in ('trans', 'init', 'len'):
        assert np.array_equal(h[k], hb[k]), k


def _degenerate_cases():
    """Five videos over one diamond (video 3 alone in group 1); the three healthy ones as a launch of their own."""
    rng = np.random.default_rng(13)
    C, K = 3, 4
    tab, tq = _tables(rng, C, K, 1.5), _tables(rng, C, K, 1.5)
    good = _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 2, 0])
    other = _lists(4, [[], [0], [1], [0, 2]], [0], [3], ids=[0, 1, 2, 0])     # the same node count, other edges
    Ts = [6, 6, 7, 6, 5]
    ep, eq = [rng.normal(size=(T, C)) for T in Ts], [rng.normal(size=(T, C)) for T in Ts]
    return tab, tq, good, other, ep, eq


def _neighbours_keep_their_bits(h, a, off, off_a, healthy):
    for i, j in enumerate(healthy):
        assert np.array_equal(h['elp'][off[j]:off[j + 1]].view(np.int64), a['elp'][off_a[i]:off_a[i + 1]].view(np.int64)), j
        assert h['value'][j] == a['value'][i] and h['value_plus'][j] == a['value_plus'][i]


@pytest.mark.parametrize('mode', ['xent', 'kl'])
def test_a_q_workspace_written_for_other_graphs_is_refused_per_video(mode):
    """q's forward call ran on graphs of the same node counts but other edges for video 3: the recorded ranges differ.  The
    ranges are compared BEFORE the q / bh kernel runs on q's workspace: that video gets NaN, zero rows and the error word, what
    the call writes into q's workspace is a strict part of what q's own backward call writes (that video's columns are
    missing), and the videos beside it keep the bits of a launch of their own."""
    tab, tq, good, other, ep, eq = _degenerate_cases()
    healthy = [0, 1, 2, 4]
    hp = Case([(ep[i], good, 0) for i in healthy], [tab], 4)
    a = _run(hp, Case([(eq[i], good, 0) for i in healthy], [tq], 4), mode)
    assert a['err'] == 0 and np.isfinite(a['value']).all()
    pc = Case([(e, good, 0) for e in ep], [tab], 4)
    qo = Case([(e, other if i == 3 else good, 0) for i, e in enumerate(eq)], [tq], 4)
    batch, dp, fp = GS._forward(pc)
    _, dq, fq = GS._forward(qo)
    torch.cuda.synchronize()
    before = fq['ws'].clone()
    h = _host(batch, _launch(pc, qo, mode, batch, dp, fp, dq, fq))
    print('\n[transcript-entropy-grad] other graphs, %s: values %s, error word %d' % (mode, h['value'], h['err']))
    assert h['err'] != 0 and np.isnan(h['value'][3]) and np.isfinite(np.delete(h['value'], 3)).all()
    assert not h['elp'][pc.off[3]:pc.off[4]].any()
    _neighbours_keep_their_bits(h, a, pc.off, hp.off, healthy)
    for k in ('trans', 'init', 'len'):
        assert np.array_equal(h[k].view(np.int64), a[k].view(np.int64)), k
    # what the call wrote into q's workspace is part of what q's own backward call writes there, bit for bit, and less of it:
    # video 3's q and bh columns are missing
    after = fq['ws'].clone()
    own = before.clone()
    GK._backward(qo, batch, dq, dict(fq, ws=own))
    torch.cuda.synchronize()
    mine, theirs = after != before, own != before
    assert bool(mine.any()) and bool((theirs | ~mine).all()) and torch.equal(after[mine], own[mine])
    assert int(theirs.sum()) > int(mine.sum())


@pytest.mark.parametrize('mode', ['xent', 'kl'])
def test_a_value_of_plus_infinity_gives_nan_rows_and_nan_tables_for_its_group(mode):
    """Video 3 (alone in group 1): q cuts the arm 0 -> 1 of the diamond, which has mass under p.  Its value is +inf, its g_elp
    rows and its group's tables are NaN, the error word stays clear; with an upstream weight of 0 it contributes exact zeros
    instead.  The videos beside it, and their group's tables, keep the bits of a launch of their own."""
    tab, tq, good, _, ep, eq = _degenerate_cases()
    cut = dict(tq, trans=tq['trans'].copy())
    cut['trans'][1, 0] = -np.inf
    healthy = [0, 1, 2, 4]
    hp = Case([(ep[i], good, 0) for i in healthy], [tab], 4)
    a = _run(hp, Case([(eq[i], good, 0) for i in healthy], [tq], 4), mode)
    assert a['err'] == 0
    for u3 in (1.0, 0.0):
        u = np.array([1.0, 1.0, 1.0, u3, 1.0])
        pc = Case([(e, good, int(i == 3)) for i, e in enumerate(ep)], [tab, tab], 4, u=u)
        qc = Case([(e, good, int(i == 3)) for i, e in enumerate(eq)], [tq, cut], 4)
        h = _run(pc, qc, mode)
        print('\n[transcript-entropy-grad] q cuts an arm p uses, %s, u = %g: values %s, error word %d' % (mode, u3, h['value'], h['err']))
        assert h['err'] == 0 and np.isposinf(h['value'][3]) and np.isposinf(h['value_plus'][3])
        rows = h['elp'][pc.off[3]:pc.off[4]]
        if u3:
            assert np.isnan(rows[:, :3]).all()
            assert all(np.isnan(h[k][1][..., :3]).all() for k in ('init',)) and np.isnan(h['trans'][1][:3, :3]).all()
            assert np.isnan(h['len'][1][:, :3]).all()
        else:
            assert not rows.any() and not any(h[k][1].any() for k in ('trans', 'init', 'len'))
        _neighbours_keep_their_bits(h, a, pc.off, hp.off, healthy)
        for k in ('trans', 'init', 'len'):
            assert np.array_equal(h[k][0].view(np.int64), a[k][0].view(np.int64)), k


# ------------------------------------------------------------------------------------------------ 4. exactness
@pytest.mark.parametrize('which', [0, 1, 2], ids=['k_rows4', 'k_rows8', 'T769'])
def test_identical_sides_give_exact_zeros_in_kl_mode(which):
    case = GK._zero_case(which)
    batch, dp, fp = GS._forward(case)
    _, dq, fq = GS._forward(case)
    assert fq['ws'].data_ptr() != fp['ws'].data_ptr()
    h = _host(batch, _launch(case, case, 'kl', batch, dp, fp, dq, fq))
    assert h['err'] == 0
    for k in KEYS + ('value', 'value_plus'):
        assert (h[k] == 0.0).all(), k


@pytest.mark.parametrize('which', [0, 1, 2], ids=['k_rows4', 'k_rows8', 'T769'])
def test_cross_entropy_of_p_with_itself_is_the_entropy_call(which):
    case = GK._zero_case(which)
    batch, dp, fp = GS._forward(case)
    _, dq, fq = GS._forward(case)
    x = _host(batch, _launch(case, case, 'xent', batch, dp, fp, dq, fq))
    e = _host(batch, _launch(case, None, 'entropy', batch, dp, fp))
    rel = {k: float(np.abs(x[k] - e[k]).max() / max(1.0, np.abs(e[k]).max())) for k in KEYS + ('value',)}
    print('\n[transcript-entropy-grad] H(p, p) against H(p): %s (bar 1e-9)' % rel)
    assert max(rel.values()) <= 1e-9 and np.abs(e['elp']).max() > 1e-2


def test_a_chain_with_one_frame_per_node_has_no_gradient():
    rng = np.random.default_rng(4)
    C, K, M = 4, 6, 9
    case = Case([(rng.normal(size=(M, C)) * 2, _ops().TranscriptGraph.chain(rng.integers(0, C, M)), 0)], [_tables(rng, C, K, 2.0)], K)
    for mode in R.MODES:
        h = _run(case, GK.other_side(case, 8), mode)
        worst = max(float(np.abs(h[k]).max()) for k in KEYS)
        print('\n[transcript-entropy-grad] chain with T = M, %s: max |g| %.1e (bar 1e-12), V %.3e' % (mode, worst, h['value'][0]))
        assert h['err'] == 0 and worst <= 1e-12


def test_all_zero_tables_have_no_gradient():
    """Uniform posteriors are stationary points of the entropy: the chain of 5 over 40 frames at a span limit of 15 (N = 30381
    alignments) and the trie of three candidates over 12 frames."""
    G = _ops().TranscriptGraph
    C, K = 3, 16
    graphs = [G.chain([0, 1, 2, 0, 1]), G.from_candidates([[0, 1, 2], [0, 1, 0, 2], [2, 1]])]
    zero = dict(trans=np.zeros((C, C)), init=np.zeros(C), len=np.zeros((K, C)))
    case = Case([(np.zeros((40, C)), graphs[0], 0), (np.zeros((12, C)), graphs[1], 0)], [zero], K, endpen=np.zeros((2, C)))
    h = _run(case, None, 'entropy')
    worst = max(float(np.abs(h[k]).max()) for k in KEYS)
    print('\n[transcript-entropy-grad] all-zero tables: H %s, max |g| %.1e (bar %.0e max(1, H))' % (h['value'], worst, TAB_BAR))
    assert h['err'] == 0 and abs(h['value'][0] - np.log(30381)) <= VAL_BAR * np.log(30381)
    assert worst <= TAB_BAR * max(1.0, h['value'].max())


# ------------------------------------------------------------------------------------------------ 5. non-interference, determinism
def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in KEYS + ('value', 'value_plus'))


@pytest.mark.parametrize('mode', R.MODES)
def test_two_calls_and_poisoned_workspaces_and_scratch_give_the_same_bits(mode):
    """Both forward workspaces AND the caller's scratch filled with 0x00 or 0xFF bytes before the calls: no kernel reads an eta,
    D or part cell (or a column cell) that was not written first, so every output has the same bits; so have two calls."""
    _, pc, qc, _, _, _, _ = GK.tiny_pairs()[0]
    ops = _ops()
    outs = []
    for fill in (0, 0xFF, 0):
        batch, dp, fp = GS._forward(pc, fill)
        _, dq, fq = GS._forward(qc, fill)
        need = ops.align_graph_entropy_bwd_scratch_bytes(batch, GS._node_offsets(pc))
        for _ in range(2):
            scratch = torch.full((need,), fill, dtype=torch.uint8, device='cuda:0')
            out = _launch(pc, qc, mode, batch, dp, fp, dq, fq, scratch=scratch)
            assert out['_keep'][-1] is scratch and out['value_plus'].data_ptr() == scratch.data_ptr() + need - 8 * batch.b
            outs.append({k: out[k].clone() for k in KEYS + ('value', 'value_plus')})
    assert bool(torch.isfinite(outs[0]['elp']).all()) and float(outs[0]['elp'].abs().max()) > 1e-2
    assert all(_same(outs[0], o) for o in outs[1:])


def test_the_call_changes_nothing_of_either_side_s_other_results():
    """A backward call, sampler draws and the entropy and KL values of both sides, bit for bit, before and after."""
    _, pc, qc, _, _, _, _ = GK.tiny_pairs()[0]
    batch, dp, fp = GS._forward(pc)
    _, dq, fq = GS._forward(qc)

    def everything():
        out = []
        for c, d, f in ((pc, dp, fp), (qc, dq, fq)):
            g = GK._backward(c, batch, d, f)
            out += [g[k] for k in KEYS] + [torch.cat(g['node_prob']), torch.cat(g['end_prob'])]
            s = GS._draw(c, batch, d, f, 16, seed=3)
            out += [s['spans'], s['logp']]
            out.append(GK._entropy(c, batch, d, f)['entropy'])
        out.append(GK._kl(pc, batch, dp, fp, dq, fq)['kl'])
        out.append(GK._kl(qc, batch, dq, fq, dp, fp)['kl'])
        return [t.clone() for t in out]

    before = everything()
    for mode in R.MODES:
        _launch(pc, qc, mode, batch, dp, fp, dq, fq)
    after = everything()
    for x, y in zip(before, after):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def test_a_captured_graph_replays_the_same_bits():
    _, pc, qc, _, _, _, _ = GK.tiny_pairs()[0]
    batch, dp, fp = GS._forward(pc)
    _, dq, fq = GS._forward(qc)
    eager = _launch(pc, qc, 'kl', batch, dp, fp, dq, fq)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _launch(pc, qc, 'kl', batch, dp, fp, dq, fq)               # (warm-up on the capture stream)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            captured = _launch(pc, qc, 'kl', batch, dp, fp, dq, fq)
    torch.cuda.current_stream().wait_stream(side)
    for k in KEYS + ('value',):
        captured[k].fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert _same(eager, captured)
