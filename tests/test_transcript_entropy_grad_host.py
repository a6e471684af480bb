"""Host-side checks of the transcript-graph entropy / cross-entropy / KL gradients: the three entry points are declared, listed
and exported; the C calls' refusals (no GPU: every call is refused before anything is staged); the scratch query; the ops
layer's argument checks; the three references of tests/transcript_entropy_grad_ref.py against each other; and the premises of
the GPU tests, from the references alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import transcript_entropy_grad_ref as R
import transcript_graph_ref as TG
from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)
POISON_Q = ctypes.c_void_p(0xbeef0000)            # (q's workspace: another address than p's)
NAMES = ('smm_align_graph_entropy_bwd_scratch_bytes', 'smm_align_graph_entropy_bwd_f64', 'smm_align_graph_kl_bwd_f64')
_UNSET = object()
REF_BAR = 1e-9
BIG = 1 << 40


def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _meta(kw):
    lengths = kw.pop('lengths', np.array([6], np.int64))
    frame_off = kw.pop('frame_off', np.array([0], np.int64))
    n_states = kw.pop('n_states', np.array([3], np.int32))
    off = kw.pop('off', np.array([0, 2], np.int64))
    shape = kw.pop('shape', None) or _shape()
    return shape, lengths, frame_off, n_states, off


def _entropy(**kw):
    shape, lengths, frame_off, n_states, off = _meta(kw)
    a = dict(elp=POISON, trans=POISON, init=POISON, len_scores=POISON, node_class=POISON, pred_mask=POISON, node_flags=POISON,
             logz=POISON, grad_out=POISON, g_elp=POISON, g_trans=POISON, g_init=POISON, g_len=POISON, value=POISON, scratch=POISON,
             scratch_bytes=BIG, ws=POISON, ws_bytes=BIG)
    a.update(kw)
    return _lib.load().smm_align_graph_entropy_bwd_f64(
        ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), a['elp'], a['trans'], a['init'], a['len_scores'],
        None, a['node_class'], a['pred_mask'], a['node_flags'], _p(off), a['logz'], a['grad_out'], a['g_elp'], a['g_trans'],
        a['g_init'], a['g_len'], a['value'], a['scratch'], ctypes.c_size_t(a['scratch_bytes']), a['ws'],
        ctypes.c_size_t(a['ws_bytes']), POISON)


def _kl(**kw):
    shape, lengths, frame_off, n_states, off = _meta(kw)
    a = dict(elp=POISON, trans=POISON, init=POISON, len_scores=POISON, logz_p=POISON, ws_p=POISON, ws_p_bytes=BIG, trans_q=POISON,
             len_q=POISON, logz_q=POISON, ws_q=POISON_Q, ws_q_bytes=BIG, node_class=POISON, pred_mask=POISON, node_flags=POISON,
             mode=_lib.KL_BWD_KL, grad_out=POISON, g_elp=POISON, g_trans=POISON, g_init=POISON, g_len=POISON, value=POISON,
             scratch=POISON, scratch_bytes=BIG)
    a.update(kw)
    return _lib.load().smm_align_graph_kl_bwd_f64(
        ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), a['elp'], a['trans'], a['init'], a['len_scores'],
        None, a['logz_p'], a['ws_p'], ctypes.c_size_t(a['ws_p_bytes']), a['trans_q'], a['len_q'], None, a['logz_q'], a['ws_q'],
        ctypes.c_size_t(a['ws_q_bytes']), a['node_class'], a['pred_mask'], a['node_flags'], _p(off), ctypes.c_int32(a['mode']),
        a['grad_out'], a['g_elp'], a['g_trans'], a['g_init'], a['g_len'], a['value'], a['scratch'],
        ctypes.c_size_t(a['scratch_bytes']), POISON)


def _scratch(lengths, ms, **kw):
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), total=int(lengths.sum()), **kw)
    return _lib.load().smm_align_graph_entropy_bwd_scratch_bytes(ctypes.byref(shape), _p(lengths), _p(off))


def _ws_bytes(lengths, ms):
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), total=int(lengths.sum()))
    return _lib.load().smm_align_graph_logz_workspace_bytes(ctypes.byref(shape), _p(lengths), _p(off))


# ------------------------------------------------------------------------------------------------ the symbols
def test_the_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'smmdp.h')).read()
    for name in NAMES:
        assert re.search(r'^(int|size_t) %s\(' % name, header, re.M), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.load(), name) is not None
    from action_segmentation_amd import _build
    assert 'smm_align_graph_entropy_bwd.hip' in _build.SOURCES


# ------------------------------------------------------------------------------------------------ the C entry points
@pytest.mark.parametrize('call', [_entropy, _kl], ids=['entropy', 'kl'])
def test_refuses_bad_arguments_before_staging(call):
    ws = 'ws_bytes' if call is _entropy else 'ws_p_bytes'
    logz = 'logz' if call is _entropy else 'logz_p'
    wsp = 'ws' if call is _entropy else 'ws_p'
    assert call(**{ws: 0}) == WORKSPACE                                 # (the poisoned call gets as far as the size checks)
    assert call(scratch_bytes=0) == WORKSPACE
    for name in ('elp', 'trans', 'init', 'len_scores', logz, wsp, 'node_class', 'pred_mask', 'node_flags', 'g_elp', 'g_trans',
                 'g_init', 'g_len', 'scratch', 'off', 'lengths', 'n_states', 'frame_off'):
        assert call(**{name: None}) == ARG, name
    assert call(grad_out=None, value=None, scratch_bytes=0) == WORKSPACE   # the upstream weights and the value are optional
    assert call(shape=_shape(b=0)) == ARG
    assert call(off=np.array([0, 0], np.int64)) == ARG                  # a video without nodes
    assert call(off=np.array([2, 1], np.int64)) == ARG                  # non-monotone
    assert call(shape=_shape(flags=_lib.SHAPE_NO_EOS)) == UNSUPPORTED
    assert call(shape=_shape(c=33)) == UNSUPPORTED
    assert call(shape=_shape(k_rows=1025)) == UNSUPPORTED
    assert call(off=np.array([0, 257], np.int64)) == UNSUPPORTED
    need, sneed = _ws_bytes([6], [2]), _scratch([6], [2])
    assert need > 0 and sneed > 0
    assert call(**{ws: need - 1}) == WORKSPACE
    assert call(**{ws: need, 'scratch_bytes': sneed - 1}) == WORKSPACE


def test_the_kl_call_refuses_its_own_arguments_before_staging():
    for name in ('trans_q', 'len_q', 'logz_q', 'ws_q'):
        assert _kl(**{name: None}) == ARG, name
    assert _kl(mode=2) == ARG and _kl(mode=-1) == ARG
    assert _kl(ws_q_bytes=0) == WORKSPACE
    assert _kl(ws_q=POISON, ws_p=POISON) == ARG                         # one workspace for both sides: the entropy call's case
    assert _kl(ws_p_bytes=_ws_bytes([6], [2]), ws_q_bytes=_ws_bytes([6], [2]) - 1) == WORKSPACE


def test_the_scratch_query_is_zero_where_the_calls_refuse_and_grows_with_the_video():
    assert _scratch([6], [0]) == 0 and _scratch([6], [257]) == 0
    assert _scratch([6], [2], flags=_lib.SHAPE_NO_EOS) == 0 and _scratch([6], [2], c=33) == 0 and _scratch([6], [2], k_rows=1025) == 0
    lib = _lib.load()
    assert lib.smm_align_graph_entropy_bwd_scratch_bytes(None, None, None) == 0
    sizes_t = [_scratch([t], [5], k_rows=4) for t in range(1, 40)]
    sizes_m = [_scratch([12], [m], k_rows=4) for m in range(1, 257)]
    assert all(b > a > 0 for a, b in zip(sizes_t, sizes_t[1:])) and all(b > a > 0 for a, b in zip(sizes_m, sizes_m[1:]))
    # four eta blocks and the occupancy differences of M (T + 1) doubles, the video's parts, q's log Z as used, its V+
    assert _scratch([6], [2], c=3, k_rows=4) == 8 * (5 * 2 * 7 + (4 * 3 + 3 * 3 + 3 + 2) + 2)
    assert _scratch([6, 9], [2, 4], c=3, k_rows=4) == _scratch([6], [2], c=3, k_rows=4) + _scratch([9], [4], c=3, k_rows=4)


# ------------------------------------------------------------------------------------------------ Python-level argument checks
def test_ops_value_errors_before_a_device_is_touched():
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 5], [3], 4)
    G = ops.TranscriptGraph
    graphs = [G.chain([0, 1]), G.from_candidates([[2, 2, 1], [2, 0]])]
    z = torch.zeros(1, dtype=torch.float64)                                     # (a CPU tensor: no call gets as far as using it)
    p, q = (z, z, z, z, None, z, z), (z, z, None, z, z)
    short = torch.zeros(16, dtype=torch.uint8)
    staged = (torch.zeros(5, dtype=torch.int32), torch.zeros(40, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="align_graph_kl_bwd: 1 graphs for 2 videos"):
        ops.align_graph_kl_bwd(batch, p, q, graphs[:1])
    with pytest.raises(ValueError, match="align_graph_kl_bwd: add_eos"):
        ops.align_graph_kl_bwd(ops.Batch([6, 5], [3], 4, no_eos=True), p, q, graphs)
    with pytest.raises(ValueError, match="align_graph_kl_bwd: staged"):
        ops.align_graph_kl_bwd(batch, p, q, graphs, staged=staged)
    for bad_p, bad_q in ((p[:6] + (None,), q), (p, q[:4] + (None,)), (p[:6] + (short,), q), (p, q[:4] + (short,))):
        with pytest.raises(ValueError, match="align_graph_kl_bwd: pass the workspace"):
            ops.align_graph_kl_bwd(batch, bad_p, bad_q, graphs)
    with pytest.raises(ValueError, match="align_graph_entropy_bwd: 1 graphs for 2 videos"):
        ops.align_graph_entropy_bwd(batch, z, z, z, z, graphs[:1], z, ws=z)
    with pytest.raises(ValueError, match="align_graph_entropy_bwd: staged"):
        ops.align_graph_entropy_bwd(batch, z, z, z, z, graphs, z, ws=z, staged=staged)
    big = torch.zeros(ops.align_graph_logz_workspace_bytes(batch, np.array([0, 2, 7], np.int64)), dtype=torch.uint8)
    with pytest.raises(ValueError, match="align_graph_kl_bwd: the two sides need a workspace each"):
        ops.align_graph_kl_bwd(batch, p[:6] + (big,), q[:4] + (big,), graphs)
    for ws in (None, short):
        with pytest.raises(ValueError, match="align_graph_entropy_bwd: pass the workspace"):
            ops.align_graph_entropy_bwd(batch, z, z, z, z, graphs, z, ws=ws)
    off = np.array([0, 2, 7], np.int64)
    assert ops.align_graph_entropy_bwd_scratch_bytes(batch, off) == 8 * (5 * (2 * 7 + 5 * 6) + 2 * (4 * 3 + 3 * 3 + 3 + 2) + 4)


# ------------------------------------------------------------------------------------------------ the references
def _random_pair(rng, i, mask=None):
    """A random DAG with an alignment and two independent sides over it, every other one under end penalties; ``mask``: one
    transition of each side is set to it."""
    while True:
        T, C, M, kp = int(rng.integers(2, 8)), 3, int(rng.integers(1, 6)), int(rng.integers(2, 6))
        graph = TG.random_graph(rng, M, C, p_edge=(0.3, 0.6, 0.9)[i % 3])
        if TG.has_alignment_by_count(T, C, graph, kp):
            break
    sides = [[rng.normal(size=(T, C)) * 2, rng.normal(size=(C, C)) * 2, rng.normal(size=C) * 2, rng.normal(size=(kp + i % 2, C)) * 2,
              rng.normal(size=C) if i % 2 == 0 else None] for _ in range(2)]
    if mask is not None:
        to, frm = int(rng.integers(0, C)), int(rng.integers(0, C))
        for s in sides:
            s[1][to, frm] = mask
    return tuple(sides[0]), tuple(sides[1]), graph, kp


def _gap(x, y):
    return max(float(np.abs(x[k] - y[k]).max()) for k in R.KEYS)


def test_enumeration_identity_and_formulas_agree():
    """120 random DAGs (M <= 5, T <= 7, C = 3, random span limits, every other one under end penalties, an independent q), all
    three modes: the value, V-, V+ and the four gradients by autograd through the enumeration, by log Z_g differentiated twice
    and by the header's formulas agree to 1e-9."""
    rng = np.random.default_rng(20261020)
    worst = np.zeros(3)
    for i in range(120):
        p, q, graph, kp = _random_pair(rng, i)
        for mode in R.MODES:
            va, ga, _ = R.enumeration_grads(p, q, graph, kp, mode)
            vb, gb = R.identity_grads(p, q, graph, kp, mode)
            f = R.formula_grads(p, q, graph, kp, mode)
            bar = REF_BAR * max(1.0, abs(va))
            errs = (max(abs(va - vb), _gap(ga, gb)), max(abs(va - f['value']), _gap(ga, f)), abs(f['value'] - f['value_plus']))
            assert max(errs) <= bar, (i, mode, errs)
            assert min(f[k].min() for k in ('eta_ms', 'eta_me', 'eta_pe', 'eta_ps')) >= 0.0
            worst = np.maximum(worst, errs)
    print('\n[transcript-entropy-grad] references, 120 graphs x 3 modes: identity %.1e, formulas %.1e, V- against V+ %.1e (bar %.0e)'
          % (*worst, REF_BAR))


def test_enumeration_and_formulas_agree_under_masks():
    """-1e9 and -inf transitions on both sides: (a) and (c) agree; (b) is not asked (it subtracts terms of 1e9)."""
    rng = np.random.default_rng(77)
    n, worst = 0, 0.0
    for i in range(60):
        p, q, graph, kp = _random_pair(rng, i, mask=(-1e9, -np.inf)[i % 2])
        if min(TG.forward_backward(s[0], graph, s[1], s[2], s[3], kp, s[4])['logz'] for s in (p, q)) < -1e8:
            continue                                                            # (every alignment crosses the mask: scores of 1e9)
        for mode in R.MODES:
            va, ga, _ = R.enumeration_grads(p, q, graph, kp, mode)
            f = R.formula_grads(p, q, graph, kp, mode)
            if f is None:
                assert np.isnan(va)
                continue
            if not np.isfinite(va):                                             # (q excludes what p has)
                continue
            n += 1
            err = max(abs(va - f['value']), abs(va - f['value_plus']), _gap(ga, f))
            assert err <= REF_BAR * max(1.0, abs(va)), (i, mode, err)
            worst = max(worst, err)
    print('\n[transcript-entropy-grad] masked references: %d cases, worst %.1e (bar %.0e)' % (n, worst, REF_BAR))
    assert n >= 100


def test_q_s_gradient_is_the_difference_of_the_marginals():
    rng = np.random.default_rng(5)
    for i in range(10):
        p, q, graph, kp = _random_pair(rng, i)
        mu_p, mu_q = R.mu_grads(p, graph, kp), R.mu_grads(q, graph, kp)
        for mode in ('xent', 'kl'):
            gq = R.enumeration_grads(p, q, graph, kp, mode)[2]
            assert max(float(np.abs(gq[k] - (mu_q[k] - mu_p[k])).max()) for k in R.KEYS) <= REF_BAR


# ------------------------------------------------------------------------------------------------ premises of the GPU tests
def test_the_gpu_cases_have_gradients_to_measure():
    """From the references alone: every reference table of every GPU case that is held to the relative bar has an entry of at
    least 1e-2 -- except the tables that are zero by structure (a chain reads every transition once on every alignment and has
    one start node: g_trans = g_init = 0), which the GPU tests hold to an absolute bar instead, and the KL against a q moved by
    1e-3 sigma, whose gradient is of that size and which the GPU test holds to 1e-3 of its own largest entry.  The masked cases,
    the packed corpus and the module cases are built on the GPU tests' side: there the shared check asserts the same premise
    from the reference before it looks at the kernels' output."""
    import test_gpu_transcript_entropy_grad as GG
    for which in (0, 1):
        for mode, near in (('entropy', False), ('xent', False), ('xent', True), ('kl', False)):
            _, ref = GG.tiny_reference(which, mode, near)
            low = {k: float(np.abs(ref[k]).max()) for k in R.KEYS}
            print('\n[transcript-entropy-grad] premise, tiny %d %s %s: %s' % (which, mode, near, low))
            assert min(low.values()) >= 1e-2
    for name, (build, modes, zero) in GG.BIG_CASES.items():
        pc = build()
        qc = GG.GK.other_side(pc, 5)
        for mode in modes:
            _, ref = GG.reference(pc, qc, mode, R.identity_grads)
            low = {k: float(np.abs(ref[k]).max()) for k in R.KEYS}
            print('\n[transcript-entropy-grad] premise, %s %s: %s' % (name, mode, low))
            assert all((low[k] <= 1e-8) if k in zero else (low[k] >= 1e-2) for k in R.KEYS), (name, mode, low)


# ------------------------------------------------------------------------------------------------ the module layer
def test_the_module_methods_take_differentiable_and_check_before_a_device_is_touched():
    import inspect
    import types
    from module_util import make_args
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    names = ('alignment_entropy', 'alignment_entropy_packed', 'alignment_kl', 'alignment_kl_packed', 'alignment_cross_entropy',
             'alignment_cross_entropy_packed')
    for name in names:
        par = inspect.signature(getattr(SemiMarkovModule, name)).parameters['differentiable']
        assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY, name
    G = ops.TranscriptGraph
    m = SemiMarkovModule(make_args(6), 4, 3, allow_self_transitions=True)
    wider = SemiMarkovModule(make_args(6), 5, 3, allow_self_transitions=True)
    ok = G.from_candidates([[2, 3], [2, 1]])
    x, ln = torch.zeros(2, 5, 3), torch.tensor([5, 5])
    pc = types.SimpleNamespace(video_names=['v0', 'v1'], batch=None, x=torch.zeros(1))
    with pytest.raises(ValueError, match="1 graphs for 2 videos"):
        m.alignment_entropy(x, ln, None, [ok], differentiable=True)
    with pytest.raises(ValueError, match="alignment_entropy: add_eos"):
        m.alignment_entropy(x, ln, None, [ok, ok], add_eos=False, differentiable=True)
    with pytest.raises(ValueError, match="1 graphs for 2 videos"):
        m.alignment_entropy_packed(pc, [ok], differentiable=True)
    for padded, packed in ((m.alignment_kl, m.alignment_kl_packed), (m.alignment_cross_entropy, m.alignment_cross_entropy_packed)):
        what = padded.__name__
        with pytest.raises(TypeError, match="%s: other must be a SemiMarkovModule" % what):
            padded(None, x, ln, None, [ok, ok], differentiable=True)
        with pytest.raises(ValueError, match="%s: the two posteriors must share the lattice" % what):
            padded(wider, x, ln, None, [ok, ok], differentiable=True)
        with pytest.raises(ValueError, match="video 1"):
            padded(m, x, ln, None, [ok, [2, 3]], differentiable=True)
        with pytest.raises(ValueError, match="1 graphs for 2 videos"):
            packed(m, pc, [ok], differentiable=True)
