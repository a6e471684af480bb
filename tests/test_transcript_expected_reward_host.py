"""Host-side checks of the expected reward under the transcript-graph posterior: the entry points are declared, listed and
exported; the C calls' refusals (no GPU: every call is refused before anything is staged); the scratch queries; the two
references of tests/transcript_expected_reward_ref.py against each other and against the identities the value obeys; and the
premises of the GPU tests, from the references alone."""
import ctypes
import os
import re

import numpy as np
import pytest

import transcript_expected_reward_ref as R
import transcript_graph_ref as TG
from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)
NAMES = ('smm_align_graph_expected_reward_scratch_bytes', 'smm_align_graph_expected_reward_bwd_scratch_bytes',
         'smm_align_graph_expected_reward_f64', 'smm_align_graph_expected_reward_bwd_f64')
REF_BAR = 1e-9
BIG = 1 << 40
SETTINGS = ('frames', 'nodes', 'both')


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


def _value(**kw):
    shape, lengths, frame_off, n_states, off = _meta(kw)
    a = dict(elp=POISON, trans=POISON, init=POISON, len_scores=POISON, node_class=POISON, pred_mask=POISON, node_flags=POISON,
             logz=POISON, reward=POISON, node_reward=POISON, value=POISON, parts=POISON, scratch=POISON, scratch_bytes=BIG, ws=POISON,
             ws_bytes=BIG)
    a.update(kw)
    return _lib.load().smm_align_graph_expected_reward_f64(
        ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), a['elp'], a['trans'], a['init'], a['len_scores'],
        None, a['node_class'], a['pred_mask'], a['node_flags'], _p(off), a['logz'], a['reward'], a['node_reward'], a['value'],
        a['parts'], a['scratch'], ctypes.c_size_t(a['scratch_bytes']), a['ws'], ctypes.c_size_t(a['ws_bytes']), POISON)


def _bwd(**kw):
    shape, lengths, frame_off, n_states, off = _meta(kw)
    a = dict(elp=POISON, trans=POISON, init=POISON, len_scores=POISON, node_class=POISON, pred_mask=POISON, node_flags=POISON,
             logz=POISON, reward=POISON, node_reward=POISON, grad_out=POISON, g_elp=POISON, g_trans=POISON, g_init=POISON,
             g_len=POISON, value=POISON, scratch=POISON, scratch_bytes=BIG, ws=POISON, ws_bytes=BIG)
    a.update(kw)
    return _lib.load().smm_align_graph_expected_reward_bwd_f64(
        ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), a['elp'], a['trans'], a['init'], a['len_scores'],
        None, a['node_class'], a['pred_mask'], a['node_flags'], _p(off), a['logz'], a['reward'], a['node_reward'], a['grad_out'],
        a['g_elp'], a['g_trans'], a['g_init'], a['g_len'], a['value'], a['scratch'], ctypes.c_size_t(a['scratch_bytes']), a['ws'],
        ctypes.c_size_t(a['ws_bytes']), POISON)


def _query(name, lengths, ms, **kw):
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), total=int(lengths.sum()), **kw)
    return getattr(_lib.load(), name)(ctypes.byref(shape), _p(lengths), _p(off))


def _scratch(lengths, ms, **kw):
    return _query('smm_align_graph_expected_reward_scratch_bytes', lengths, ms, **kw)


def _scratch_bwd(lengths, ms, **kw):
    return _query('smm_align_graph_expected_reward_bwd_scratch_bytes', lengths, ms, **kw)


# ------------------------------------------------------------------------------------------------ the symbols
def test_the_symbols_are_declared_listed_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'smmdp.h')).read()
    for name in NAMES:
        assert re.search(r'^(int|size_t) %s\(' % name, header, re.M), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.load(), name) is not None
    from action_segmentation_amd import _build
    assert 'smm_align_graph_expected_reward.hip' in _build.SOURCES


def test_no_new_kernel_has_a_private_segment_or_a_spill():
    from action_segmentation_amd import _build
    res = {k: v for k, v in _build.kernel_resources().items() if 'smm_align_graph_er_' in k}
    if not res:
        pytest.skip('no code object metadata to read')
    assert len(res) == 6
    for name, r in res.items():
        assert r['private_segment_fixed_size'] == 0 and r['vgpr_spill_count'] == 0, (name, r)


# ------------------------------------------------------------------------------------------------ the C entry points
@pytest.mark.parametrize('call', [_value, _bwd], ids=['value', 'gradient'])
def test_refuses_bad_arguments_before_staging(call):
    query = _scratch if call is _value else _scratch_bwd
    assert call(ws_bytes=0) == WORKSPACE                                # (the poisoned call gets as far as the size checks)
    assert call(scratch_bytes=0) == WORKSPACE
    required = ('value',) if call is _value else ('g_elp', 'g_trans', 'g_init', 'g_len')
    for name in ('elp', 'trans', 'init', 'len_scores', 'logz', 'ws', 'node_class', 'pred_mask', 'node_flags', 'scratch', 'off',
                 'lengths', 'n_states', 'frame_off') + required:
        assert call(**{name: None}) == ARG, name
    assert call(reward=None, node_reward=None) == ARG                   # nothing to expect
    assert call(reward=None, scratch_bytes=0) == WORKSPACE and call(node_reward=None, scratch_bytes=0) == WORKSPACE
    optional = dict(parts=None) if call is _value else dict(grad_out=None, value=None)
    assert call(scratch_bytes=0, **optional) == WORKSPACE
    assert call(shape=_shape(b=0)) == ARG
    assert call(off=np.array([0, 0], np.int64)) == ARG                  # a video without nodes
    assert call(off=np.array([2, 1], np.int64)) == ARG                  # non-monotone
    assert call(shape=_shape(flags=_lib.SHAPE_NO_EOS)) == UNSUPPORTED
    assert call(shape=_shape(c=33)) == UNSUPPORTED
    assert call(shape=_shape(k_rows=1025)) == UNSUPPORTED
    assert call(off=np.array([0, 257], np.int64)) == UNSUPPORTED
    lengths, off = np.array([6], np.int64), np.array([0, 2], np.int64)
    need = _lib.load().smm_align_graph_logz_workspace_bytes(ctypes.byref(_shape()), _p(lengths), _p(off))
    sneed = query([6], [2])
    assert need > 0 and sneed > 0
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert call(ws_bytes=need, scratch_bytes=sneed - 1) == WORKSPACE


def test_the_scratch_queries_are_zero_where_the_calls_refuse_and_state_their_layout():
    lib = _lib.load()
    for q in (_scratch, _scratch_bwd):
        assert q([6], [0]) == 0 and q([6], [257]) == 0
        assert q([6], [2], flags=_lib.SHAPE_NO_EOS) == 0 and q([6], [2], c=33) == 0 and q([6], [2], k_rows=1025) == 0
        sizes_t = [q([t], [5], k_rows=4) for t in range(1, 40)]
        sizes_m = [q([12], [m], k_rows=4) for m in range(1, 257)]
        assert all(b > a > 0 for a, b in zip(sizes_t, sizes_t[1:])) and all(b > a > 0 for a, b in zip(sizes_m, sizes_m[1:]))
    assert lib.smm_align_graph_expected_reward_scratch_bytes(None, None, None) == 0
    assert lib.smm_align_graph_expected_reward_bwd_scratch_bytes(None, None, None) == 0
    # the value call: the videos' cumW offsets, cumW ((T + 1) c_max per video), two partials per node
    assert _scratch([6], [2], c=3, k_rows=4) == 8 * (1 + 7 * 3 + 2 * 2)
    assert _scratch([6, 9], [2, 4], c=3, k_rows=4) == 8 * (2 + (7 + 10) * 3 + 2 * 6)
    # the gradient call: the entropy gradient's scratch, then the offsets and cumW
    ent = _query('smm_align_graph_entropy_bwd_scratch_bytes', [6, 9], [2, 4], c=3, k_rows=4)
    assert _scratch_bwd([6, 9], [2, 4], c=3, k_rows=4) == ent + 8 * (2 + (7 + 10) * 3)


# ------------------------------------------------------------------------------------------------ the Python layers
def test_the_methods_take_differentiable_and_check_before_a_device_is_touched():
    import inspect
    import types
    import torch
    from module_util import make_args
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    for name in ('alignment_expected_reward', 'alignment_expected_reward_packed', 'alignment_expected_accuracy',
                 'alignment_expected_accuracy_packed'):
        par = inspect.signature(getattr(SemiMarkovModule, name)).parameters['differentiable']
        assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY, name
    assert callable(SemiMarkovModel.alignment_expected_accuracy) and callable(SemiMarkovModel.candidate_expected_accuracy)
    G = ops.TranscriptGraph
    m = SemiMarkovModule(make_args(6), 4, 3, allow_self_transitions=True)
    ok = G.from_candidates([[2, 3], [2, 1]])
    x, ln = torch.zeros(2, 5, 3), torch.tensor([5, 5])
    seg = torch.ones(4, dtype=torch.float64)
    pc = types.SimpleNamespace(video_names=['v0', 'v1'], batch=None, x=torch.zeros(1))
    for d in (False, True):
        with pytest.raises(ValueError, match="1 graphs for 2 videos"):
            m.alignment_expected_reward(x, ln, None, [ok], seg_reward=seg, differentiable=d)
        with pytest.raises(ValueError, match="alignment_expected_reward: add_eos"):
            m.alignment_expected_reward(x, ln, None, [ok, ok], seg_reward=seg, add_eos=False, differentiable=d)
        with pytest.raises(ValueError, match="1 graphs for 2 videos"):
            m.alignment_expected_reward_packed(pc, [ok], seg_reward=seg, differentiable=d)
    batch = ops.Batch([6, 5], [3], 4)
    off = np.array([0, 2, 7], np.int64)
    assert ops.align_graph_expected_reward_scratch_bytes(batch, off) == 8 * (2 + (7 + 6) * 3 + 2 * 7)
    assert ops.align_graph_expected_reward_bwd_scratch_bytes(batch, off) == ops.align_graph_entropy_bwd_scratch_bytes(batch, off) \
        + 8 * (2 + (7 + 6) * 3)


# ------------------------------------------------------------------------------------------------ the references
def _random_case(rng, i):
    """A random DAG with an alignment, a side over it (every other one under end penalties), N(0, 1) rewards."""
    while True:
        T, C, M, kp = int(rng.integers(2, 8)), 3, int(rng.integers(1, 6)), int(rng.integers(2, 6))
        graph = TG.random_graph(rng, M, C, p_edge=(0.3, 0.6, 0.9)[i % 3])
        if TG.has_alignment_by_count(T, C, graph, kp):
            break
    side = (rng.normal(size=(T, C)) * 2, rng.normal(size=(C, C)) * 2, rng.normal(size=C) * 2, rng.normal(size=(kp + i % 2, C)) * 2,
            rng.normal(size=C) if i % 2 == 0 else None)
    return side, graph, kp, rng.normal(size=(T, C)), rng.normal(size=M)


def _pick(setting, w, nr):
    return (w if setting != 'nodes' else None), (nr if setting != 'frames' else None)


def _gap(x, y):
    return max(float(np.abs(x[k] - y[k]).max()) for k in R.KEYS)


def test_enumeration_and_identity_agree():
    """100 random DAGs (M <= 5, T <= 7, C = 3, random span limits, every other one under end penalties), frame rewards, node
    rewards and both: the value and the four gradients by autograd through the enumeration and by log Z_g differentiated twice
    with a class per node agree to 1e-9."""
    rng = np.random.default_rng(20261021)
    worst = 0.0
    for i in range(100):
        side, graph, kp, w, nr = _random_case(rng, i)
        for setting in SETTINGS:
            va, ga = R.enumeration_reward(side, graph, kp, *_pick(setting, w, nr))
            vb, gb = R.identity_reward(side, graph, kp, *_pick(setting, w, nr))
            err = max(abs(va - vb), _gap(ga, gb))
            assert err <= REF_BAR * max(1.0, abs(va)), (i, setting, err)
            worst = max(worst, err)
    print('\n[transcript-expected-reward] references, 100 graphs x 3 settings: enumeration against identity %.1e (bar %.0e)' % (worst, REF_BAR))


def test_the_value_identities_hold_in_the_references():
    """reward = 1: V = T and no gradient; node_reward = 1 on a chain: V = M and no gradient; onehot(end node j) on a trie: p_end[j];
    onehot(column c): sum_t of the frame posteriors; V is linear in the rewards; accuracy + errors = T."""
    rng = np.random.default_rng(3)
    for i in range(20):
        side, graph, kp, w, nr = _random_case(rng, i)
        T, C = side[0].shape
        for route in (R.enumeration_reward, R.identity_reward):
            v, g = route(side, graph, kp, np.ones((T, C)), None)
            assert abs(v - T) <= REF_BAR * T and max(np.abs(g[k]).max() for k in R.KEYS) <= REF_BAR
        fb = TG.forward_backward(side[0], graph, side[1], side[2], side[3], kp, side[4])
        for c in range(C):
            onehot = np.zeros((T, C))
            onehot[:, c] = 1.0
            assert abs(R.enumeration_reward(side, graph, kp, onehot, None)[0] - fb['elp'][:, c].sum()) <= REF_BAR * T
        assert abs(R.enumeration_reward(side, graph, kp, None, nr)[0] - float((fb['p_used'] * nr).sum())) <= REF_BAR * np.abs(nr).sum()
        w2, nr2 = rng.normal(size=w.shape), rng.normal(size=nr.shape)
        va, vb = R.enumeration_reward(side, graph, kp, w, nr)[0], R.enumeration_reward(side, graph, kp, w2, nr2)[0]
        vm = R.enumeration_reward(side, graph, kp, 0.7 * w - 1.9 * w2, 0.7 * nr - 1.9 * nr2)[0]
        assert abs(vm - (0.7 * va - 1.9 * vb)) <= REF_BAR * (np.abs(w).sum() + np.abs(w2).sum() + np.abs(nr).sum() + np.abs(nr2).sum())
        hit = np.eye(C)[rng.integers(0, C, T)]
        assert abs(R.enumeration_reward(side, graph, kp, hit, None)[0] + R.enumeration_reward(side, graph, kp, 1.0 - hit, None)[0] - T) <= REF_BAR * T
    # a chain crosses every node
    a = rng.integers(0, 3, 4)
    chain = (a, np.eye(4, k=-1, dtype=bool), np.arange(4) == 0, np.arange(4) == 3)
    side = (rng.normal(size=(7, 3)), rng.normal(size=(3, 3)), rng.normal(size=3), rng.normal(size=(5, 3)), None)
    for route in (R.enumeration_reward, R.identity_reward):
        v, g = route(side, chain, 5, None, np.ones(4))
        assert abs(v - 4) <= REF_BAR and max(np.abs(g[k]).max() for k in R.KEYS) <= REF_BAR
    # the end nodes of a trie: the candidates' posteriors
    from action_segmentation_amd import ops
    trie = ops.TranscriptGraph.from_candidates([[0, 1, 2], [0, 2, 1], [1, 0]])
    tg = (trie.ids, trie.pred, trie.start, trie.end)
    fb = TG.forward_backward(side[0], tg, side[1], side[2], side[3], 5, None)
    for j in np.flatnonzero(np.asarray(trie.end)):
        onehot = np.zeros(len(trie))
        onehot[j] = 1.0
        assert abs(R.enumeration_reward(side, tg, 5, None, onehot)[0] - fb['p_end'][j]) <= REF_BAR
        assert abs(R.identity_reward(side, tg, 5, None, onehot)[0] - fb['p_end'][j]) <= REF_BAR


# ------------------------------------------------------------------------------------------------ premises of the GPU tests
def test_the_gpu_cases_have_gradients_to_measure():
    """From the references alone: every reference table of every GPU case that is held to the relative bar has an entry of at
    least 1e-2 -- except the tables that are zero by structure (a chain reads every transition once on every alignment and has
    one start node: g_trans = g_init = 0), which are at most 1e-8 in the reference and which the GPU test holds to an absolute
    bar instead."""
    import test_gpu_transcript_expected_reward as GE
    for which in (0, 1):
        for setting in SETTINGS:
            _, _, (_, ref) = GE.tiny_reference(which, setting)
            low = {k: float(np.abs(ref[k]).max()) for k in R.KEYS}
            print('\n[transcript-expected-reward] premise, tiny %d %s: %s' % (which, setting, low))
            assert min(low.values()) >= 1e-2
    for mask in (-1e9, -np.inf):
        case = GE.masked_case(mask)
        _, ref = GE.reference(case, GE.draw_rewards(case, 41), R.enumeration_reward)
        assert min(float(np.abs(ref[k]).max()) for k in R.KEYS) >= 1e-2
    for name, zero in GE.BIG_CASES.items():
        case, rewards = GE.big_case(name)
        _, ref = GE.reference(case, rewards, R.identity_reward)
        low = {k: float(np.abs(ref[k]).max()) for k in R.KEYS}
        print('\n[transcript-expected-reward] premise, %s: %s' % (name, low))
        assert all((low[k] <= 1e-8) if k in zero else (low[k] >= 1e-2) for k in R.KEYS), (name, low)
    good = GE.GG._corpus(False, [0.7, 0.0, -1.3, 2.0])
    _, ref = GE.reference(good, GE._corpus_rewards(good, False), R.identity_reward)
    assert min(float(np.abs(ref[k]).max()) for k in R.KEYS) >= 1e-2
