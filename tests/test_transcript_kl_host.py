"""Host-side checks of the transcript-graph KL: the entry point is declared, listed and exported; the C call's refusals (no
GPU: every call is refused before anything is staged); the Python layers' argument checks; the three references of
tests/transcript_kl_ref.py against each other; and the premises of the GPU test of the tiny graphs."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import transcript_graph_ref as TG
import transcript_kl_ref as TK
from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)
NAME = 'smm_align_graph_kl_f64'
_UNSET = object()
REF_BAR = 1e-9


def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _call(shape=None, off=_UNSET, elp=POISON, trans=POISON, init=POISON, len_scores=POISON, logz_p=POISON, ws_p=POISON,
          ws_p_bytes=1 << 40, trans_q=POISON, len_q=POISON, logz_q=POISON, ws_q=POISON, ws_q_bytes=1 << 40, node_class=POISON,
          pred_mask=POISON, node_flags=POISON, kl_out=POISON, xent_out=POISON, kl_parts=POISON, lengths=_UNSET, n_states=_UNSET,
          frame_off=_UNSET):
    lengths = np.array([6], np.int64) if lengths is _UNSET else lengths
    frame_off = np.array([0], np.int64) if frame_off is _UNSET else frame_off
    n_states = np.array([3], np.int32) if n_states is _UNSET else n_states
    off = np.array([0, 2], np.int64) if off is _UNSET else off
    shape = shape or _shape()
    return _lib.load().smm_align_graph_kl_f64(
        ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), elp, trans, init, len_scores, None, logz_p,
        ws_p, ctypes.c_size_t(ws_p_bytes), trans_q, len_q, None, logz_q, ws_q, ctypes.c_size_t(ws_q_bytes), node_class, pred_mask,
        node_flags, _p(off), kl_out, xent_out, kl_parts, POISON)


def _ws_bytes(lengths, ms, **kw):
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), total=int(lengths.max()) * len(lengths), **kw)
    return _lib.load().smm_align_graph_logz_workspace_bytes(ctypes.byref(shape), _p(lengths), _p(off))


# ------------------------------------------------------------------------------------------------ the symbol
def test_the_symbol_is_declared_listed_and_exported():
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'smmdp.h')).read()
    assert re.search(r'^int %s\(' % NAME, header, re.M)
    assert NAME in _lib.SYMBOLS
    assert getattr(_lib.load(), NAME) is not None
    from action_segmentation_amd import _build
    assert 'smm_align_graph_kl.hip' in _build.SOURCES


# ------------------------------------------------------------------------------------------------ the C entry point
def test_refuses_bad_arguments_before_staging():
    assert _call(ws_p_bytes=0) == WORKSPACE                             # (the poisoned call gets as far as the size checks)
    assert _call(ws_q_bytes=0) == WORKSPACE
    for name in ('elp', 'trans', 'init', 'len_scores', 'logz_p', 'ws_p', 'trans_q', 'len_q', 'logz_q', 'ws_q', 'node_class',
                 'pred_mask', 'node_flags', 'kl_out', 'off', 'lengths', 'n_states', 'frame_off'):
        assert _call(**{name: None}) == ARG, name
    assert _call(xent_out=None, kl_parts=None, ws_p_bytes=0) == WORKSPACE   # the cross-entropy and the parts are optional
    assert _call(shape=_shape(b=0)) == ARG
    assert _call(off=np.array([0, 0], np.int64)) == ARG                 # a video without nodes
    assert _call(off=np.array([2, 1], np.int64)) == ARG                 # non-monotone
    two = dict(shape=_shape(b=2), lengths=np.array([6, 6], np.int64), frame_off=np.array([0, 6], np.int64))
    assert _call(off=np.array([0, 3, 2], np.int64), **two) == ARG
    assert _call(off=np.array([0, 3, 5], np.int64), ws_q_bytes=0, **two) == WORKSPACE


def test_refuses_unsupported_shapes_and_short_workspaces_before_staging():
    assert _call(shape=_shape(flags=_lib.SHAPE_NO_EOS)) == UNSUPPORTED
    assert _call(shape=_shape(c=33)) == UNSUPPORTED
    assert _call(shape=_shape(k_rows=1025)) == UNSUPPORTED
    assert _call(off=np.array([0, 257], np.int64)) == UNSUPPORTED
    assert _call(off=np.array([0, 256], np.int64), ws_p_bytes=0) == WORKSPACE
    need = _ws_bytes([6], [2])
    assert need > 0
    assert _call(ws_p_bytes=need - 1) == WORKSPACE                      # one byte short of the forward call's size, either side
    assert _call(ws_p_bytes=need, ws_q_bytes=need - 1) == WORKSPACE


# ------------------------------------------------------------------------------------------------ Python-level argument checks
def test_ops_value_errors_before_a_device_is_touched():
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 5], [3], 4)
    G = ops.TranscriptGraph
    graphs = [G.chain([0, 1]), G.from_candidates([[2, 2, 1], [2, 0]])]
    z = torch.zeros(1, dtype=torch.float64)                                     # (a CPU tensor: no call gets as far as using it)
    p, q = (z, z, z, z, None, z, z), (z, z, None, z, z)
    with pytest.raises(ValueError, match="align_graph_kl: 1 graphs for 2 videos"):
        ops.align_graph_kl(batch, p, q, graphs[:1])
    with pytest.raises(ValueError, match="align_graph_kl: add_eos"):
        ops.align_graph_kl(ops.Batch([6, 5], [3], 4, no_eos=True), p, q, graphs)
    staged = (torch.zeros(5, dtype=torch.int32), torch.zeros(40, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="align_graph_kl: staged"):
        ops.align_graph_kl(batch, p, q, graphs, staged=staged)
    short = torch.zeros(16, dtype=torch.uint8)
    for bad_p, bad_q in ((p[:6] + (None,), q), (p, q[:4] + (None,)), (p[:6] + (short,), q), (p, q[:4] + (short,))):
        with pytest.raises(ValueError, match="align_graph_kl: pass the workspace"):   # missing, or too small to be the forward call's
            ops.align_graph_kl(batch, bad_p, bad_q, graphs)


def test_module_and_model_checks_fire_before_a_device_is_touched():
    from module_util import make_args
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    G = ops.TranscriptGraph
    m = SemiMarkovModule(make_args(6), 4, 3, allow_self_transitions=True)
    wider = SemiMarkovModule(make_args(6), 5, 3, allow_self_transitions=True)
    ok = G.from_candidates([[2, 3], [2, 1]])
    x, ln = torch.zeros(2, 5, 3), torch.tensor([5, 5])
    pc = types.SimpleNamespace(video_names=['v0', 'v1'], batch=None, x=torch.zeros(1))
    for padded, packed in ((m.alignment_kl, m.alignment_kl_packed), (m.alignment_cross_entropy, m.alignment_cross_entropy_packed)):
        what = padded.__name__
        with pytest.raises(TypeError, match="%s: other must be a SemiMarkovModule" % what):
            padded(None, x, ln, None, [ok, ok])
        with pytest.raises(ValueError, match="%s: the two posteriors must share the lattice" % what):
            padded(wider, x, ln, None, [ok, ok])
        with pytest.raises(ValueError, match="%s: add_eos" % what):
            padded(m, x, ln, None, [ok, ok], add_eos=False)
        with pytest.raises(ValueError, match="1 graphs for 2 videos"):
            padded(m, x, ln, None, [ok])
        with pytest.raises(ValueError, match="video 1"):
            padded(m, x, ln, None, [ok, [2, 3]])
        with pytest.raises(TypeError, match="%s_packed: other must be a SemiMarkovModule" % what):
            packed(None, pc, [ok, ok])
        with pytest.raises(ValueError, match="1 graphs for 2 videos"):
            packed(m, pc, [ok])
        with pytest.raises(ValueError, match="'v1'"):
            packed(m, pc, [ok, [2, 3]])
    nobody = SemiMarkovModel                                                    # (refused before the models are looked at)
    wide = [[c] * 100 for c in range(3)]                                        # a trie of 300 nodes
    with pytest.raises(ValueError, match="candidate_kl.*'v'.*300 nodes"):
        SemiMarkovModel.candidate_kl(nobody, None, None, {'v': wide})
    with pytest.raises(ValueError, match="candidate_kl: no candidates"):
        SemiMarkovModel.candidate_kl(nobody, None, None, {'v': []})
    with pytest.raises(TypeError, match="candidate_kl: other must be a SemiMarkovModel"):
        SemiMarkovModel.candidate_kl(nobody, m, None, {'v': [[0]]})
    with pytest.raises(ValueError, match="alignment_kl.*not both"):
        SemiMarkovModel.alignment_kl(nobody, None, None, {'v': [0]}, optional_by_video={}, optional_classes=[0])
    with pytest.raises(TypeError, match="alignment_kl: other must be a SemiMarkovModel"):
        SemiMarkovModel.alignment_kl(nobody, m, None, {'v': [0]})


# ------------------------------------------------------------------------------------------------ the references
def _random_pair(rng, i):
    """A random DAG with an alignment and two independent sides over it, every other one under end penalties."""
    while True:
        T, C, M, kp = int(rng.integers(1, 8)), int(rng.integers(1, 4)), int(rng.integers(1, 7)), int(rng.integers(2, 6))
        graph = TG.random_graph(rng, M, C, p_edge=(0.3, 0.6, 0.9)[i % 3])
        if TG.has_alignment_by_count(T, C, graph, kp):
            break
    sides = [(rng.normal(size=(T, C)) * 2, rng.normal(size=(C, C)) * 2, rng.normal(size=C) * 2, rng.normal(size=(kp + i % 2, C)) * 2,
              rng.normal(size=C) if i % 2 == 0 else None) for _ in range(2)]
    return sides[0], sides[1], graph, kp


def test_enumeration_chain_rule_and_identity_agree():
    """130 random DAGs (M <= 6, T <= 7, every other one under end penalties, an independent q): sum p log(p / q) over the
    enumerated alignments, the chain rule over the sampler's decisions and the identity agree in KL and in H(p, q); KL_end is
    the KL of the two p_end vectors; every part is >= 0."""
    rng = np.random.default_rng(20261020)
    n_fin, worst = 0, np.zeros(4)
    for i in range(130):
        p, q, graph, kp = _random_pair(rng, i)
        kl, xe, lzp, lzq, n = TK.enumeration_kl(p, q, graph, kp)
        parts = TK.chain_rule_kl(p, q, graph, kp)
        assert (parts is None) == (n == 0)
        if parts is None:
            continue
        n_fin += 1
        fp, fq = (TG.forward_backward(s[0], graph, s[1], s[2], s[3], kp, s[4]) for s in (p, q))
        ident = TK.identity_kl(fp['logz'], fq['logz'], fp, p, q, TG._graph(graph)[0], fp['p_end'])
        bar = REF_BAR * max(1.0, kl)
        assert min(parts[0]) >= 0.0 and min(parts[1]) >= 0.0 and kl >= -1e-14    # (the enumeration's own rounding)
        errs = (abs(sum(parts[0]) - kl), abs(ident - kl), abs(parts[0][0] - TK.kl_of(fp['p_end'], fq['p_end'])),
                abs(sum(parts[1]) - xe))
        assert max(errs) <= bar, (i, kl, parts, ident)
        worst = np.maximum(worst, errs)
    print('\n[transcript-kl] references, %d graphs: chain rule %.1e, identity %.1e, KL_end against p_end %.1e, H(p,q) %.1e (bar %.0e)'
          % (n_fin, *worst, REF_BAR))
    assert n_fin >= 100


def test_identical_sides_give_exact_zeros_and_a_cut_gives_infinity():
    rng = np.random.default_rng(3)
    for i in range(20):
        p, _, graph, kp = _random_pair(rng, i)
        parts = TK.chain_rule_kl(p, p, graph, kp)
        if parts is not None:
            assert parts[0] == (0.0, 0.0, 0.0) and TK.enumeration_kl(p, p, graph, kp)[0] == 0.0
    # a diamond whose arm 0 -> 1 q cuts: +inf; the other way round it is log Z_q - log Z_p
    diamond = (np.array([0, 1, 2, 0]), np.array([[0, 0, 0, 0], [1, 0, 0, 0], [1, 0, 0, 0], [0, 1, 1, 0]], bool),
               np.arange(4) == 0, np.arange(4) == 3)
    e, tr, ini, ln = rng.normal(size=(6, 3)), rng.normal(size=(3, 3)), rng.normal(size=3), rng.normal(size=(5, 3))
    cut = tr.copy()
    cut[1, 0] = -np.inf
    whole, less = (e, tr, ini, ln, None), (e, cut, ini, ln, None)
    assert TK.enumeration_kl(whole, less, diamond, 5)[0] == np.inf and sum(TK.chain_rule_kl(whole, less, diamond, 5)[0]) == np.inf
    kl, _, lzp, lzq, _ = TK.enumeration_kl(less, whole, diamond, 5)
    assert abs(kl - (lzq - lzp)) <= REF_BAR and abs(sum(TK.chain_rule_kl(less, whole, diamond, 5)[0]) - kl) <= REF_BAR and kl > 0


def test_a_trie_splits_into_candidate_and_boundary_kl():
    """total = KL(posteriors over the candidates) + sum_c p_c KL(chain of candidate c), and KL_end is the first term."""
    from action_segmentation_amd import ops
    G = ops.TranscriptGraph
    rng = np.random.default_rng(8)
    C, kp, T = 3, 5, 7
    draw = lambda ep: (rng.normal(size=(T, C)), rng.normal(size=(C, C)), rng.normal(size=C), rng.normal(size=(kp, C)),
                       rng.normal(size=C) if ep else None)
    for ep in (False, True):
        p, q = draw(ep), draw(ep)
        cands = [[0, 1], [0, 1, 2], [2, 0], [2, 0, 1, 1]]
        trie = G.from_candidates(cands)
        tup = (trie.ids, trie.pred, trie.start, trie.end)
        total = TK.chain_rule_kl(p, q, tup, kp)[0]
        chains = [(np.array(c), np.eye(len(c), k=-1, dtype=bool), np.arange(len(c)) == 0, np.arange(len(c)) == len(c) - 1) for c in cands]
        each = [TK.enumeration_kl(p, q, ch, kp) for ch in chains]
        post = lambda z: np.exp(z - (z.max() + np.log(np.exp(z - z.max()).sum())))
        pp, pq = post(np.array([e[2] for e in each])), post(np.array([e[3] for e in each]))
        want = TK.kl_of(pp, pq) + float(sum(pc * e[0] for pc, e in zip(pp, each)))
        assert abs(sum(total) - want) <= REF_BAR * max(1.0, want) and abs(total[0] - TK.kl_of(pp, pq)) <= REF_BAR
        assert abs(sum(total) - TK.enumeration_kl(p, q, tup, kp)[0]) <= REF_BAR * max(1.0, want)


# ------------------------------------------------------------------------------------------------ premises of the GPU test
def test_the_exact_cases_have_kl_to_measure():
    """What the GPU tests of the tiny graphs assume of test_gpu_transcript_kl.tiny_pairs(), from the enumeration alone: against
    the independent q every one of the 8 videos has KL >= 0.1; against the near q at least 6 of the 8 have KL >= 1e-7 (those
    are held to the relative bar, the others to an absolute one)."""
    import test_gpu_transcript_kl as GK
    far, near = [], []
    for _, _, _, _, names, ref_far, ref_near in GK.tiny_pairs():
        far += [r[0] for r in ref_far]
        near += [r[0] for r in ref_near]
    print('\n[transcript-kl] premises: independent q KL %s; near q KL %s' % (np.array2string(np.array(far), precision=3),
                                                                             np.array2string(np.array(near), precision=3)))
    assert len(far) == 8 and np.isfinite(far).all() and min(far) >= 0.1
    assert np.isfinite(near).all() and min(near) >= 0.0 and sum(k >= GK.SMALL for k in near) >= 6
