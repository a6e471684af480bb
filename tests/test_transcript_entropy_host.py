"""Host-side checks of the transcript-graph entropy: the entry point is declared, listed and exported; the C call's refusals
(no GPU: every call is refused before anything is staged); the Python layers' argument checks; the three references of
tests/transcript_entropy_ref.py against each other; and the premises of the GPU test of the tiny graphs."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import transcript_entropy_ref as TE
import transcript_graph_ref as TG
import transcript_sample_ref as TS
from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)
NAME = 'smm_align_graph_entropy_f64'
_UNSET = object()
REF_BAR = 1e-9


def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _call(shape=None, off=_UNSET, elp=POISON, trans=POISON, init=POISON, len_scores=POISON, node_class=POISON, pred_mask=POISON,
          node_flags=POISON, logz=POISON, h_out=POISON, h_parts=POISON, ws=POISON, ws_bytes=1 << 40, lengths=_UNSET,
          n_states=_UNSET, frame_off=_UNSET):
    lengths = np.array([6], np.int64) if lengths is _UNSET else lengths
    frame_off = np.array([0], np.int64) if frame_off is _UNSET else frame_off
    n_states = np.array([3], np.int32) if n_states is _UNSET else n_states
    off = np.array([0, 2], np.int64) if off is _UNSET else off
    shape = shape or _shape()
    return _lib.load().smm_align_graph_entropy_f64(
        ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), elp, trans, init, len_scores, None,
        node_class, pred_mask, node_flags, _p(off), logz, h_out, h_parts, ws, ctypes.c_size_t(ws_bytes), POISON)


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


# ------------------------------------------------------------------------------------------------ the C entry point
def test_refuses_bad_arguments_before_staging():
    assert _call(ws_bytes=0) == WORKSPACE                               # (the poisoned call gets as far as the size check)
    for name in ('elp', 'trans', 'init', 'len_scores', 'node_class', 'pred_mask', 'node_flags', 'logz', 'h_out', 'ws', 'off',
                 'lengths', 'n_states', 'frame_off'):
        assert _call(**{name: None}) == ARG, name
    assert _call(h_parts=None, ws_bytes=0) == WORKSPACE                 # the parts are optional
    assert _call(shape=_shape(b=0)) == ARG
    assert _call(off=np.array([0, 0], np.int64)) == ARG                 # a video without nodes
    assert _call(off=np.array([2, 1], np.int64)) == ARG                 # non-monotone
    two = dict(shape=_shape(b=2), lengths=np.array([6, 6], np.int64), frame_off=np.array([0, 6], np.int64))
    assert _call(off=np.array([0, 3, 2], np.int64), **two) == ARG
    assert _call(off=np.array([0, 3, 5], np.int64), ws_bytes=0, **two) == WORKSPACE


def test_refuses_unsupported_shapes_and_short_workspaces_before_staging():
    assert _call(shape=_shape(flags=_lib.SHAPE_NO_EOS)) == UNSUPPORTED
    assert _call(shape=_shape(c=33)) == UNSUPPORTED
    assert _call(shape=_shape(k_rows=1025)) == UNSUPPORTED
    assert _call(off=np.array([0, 257], np.int64)) == UNSUPPORTED
    assert _call(off=np.array([0, 256], np.int64), ws_bytes=0) == WORKSPACE
    need = _ws_bytes([6], [2])
    assert need > 0 and _call(ws_bytes=need - 1) == WORKSPACE           # one byte short of the forward call's size


# ------------------------------------------------------------------------------------------------ Python-level argument checks
def test_ops_value_errors_before_a_device_is_touched():
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 5], [3], 4)
    G = ops.TranscriptGraph
    graphs = [G.chain([0, 1]), G.from_candidates([[2, 2, 1], [2, 0]])]
    z = torch.zeros(1, dtype=torch.float64)                                     # (a CPU tensor: no call gets as far as using it)
    with pytest.raises(ValueError, match="align_graph_entropy: 1 graphs for 2 videos"):
        ops.align_graph_entropy(batch, z, z, z, z, graphs[:1], z, ws=z)
    with pytest.raises(ValueError, match="align_graph_entropy: add_eos"):
        ops.align_graph_entropy(ops.Batch([6, 5], [3], 4, no_eos=True), z, z, z, z, graphs, z, ws=z)
    staged = (torch.zeros(5, dtype=torch.int32), torch.zeros(40, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="align_graph_entropy: staged"):
        ops.align_graph_entropy(batch, z, z, z, z, graphs, z, ws=z, staged=staged)
    with pytest.raises(ValueError, match="align_graph_entropy: pass the workspace"):   # no workspace: not the forward call's
        ops.align_graph_entropy(batch, z, z, z, z, graphs, z)
    with pytest.raises(ValueError, match="align_graph_entropy: pass the workspace"):   # ... or one too small to be it
        ops.align_graph_entropy(batch, z, z, z, z, graphs, z, ws=torch.zeros(16, dtype=torch.uint8))


def test_module_and_model_checks_fire_before_a_device_is_touched():
    from module_util import make_args
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    G = ops.TranscriptGraph
    m = SemiMarkovModule(make_args(6), 4, 3, allow_self_transitions=True)
    ok = G.from_candidates([[2, 3], [2, 1]])
    x, ln = torch.zeros(2, 5, 3), torch.tensor([5, 5])
    with pytest.raises(ValueError, match="alignment_entropy: add_eos"):
        m.alignment_entropy(x, ln, None, [ok, ok], add_eos=False)
    with pytest.raises(ValueError, match="1 graphs for 2 videos"):
        m.alignment_entropy(x, ln, None, [ok])
    with pytest.raises(ValueError, match="video 1"):
        m.alignment_entropy(x, ln, None, [ok, [2, 3]])
    pc = types.SimpleNamespace(video_names=['v0', 'v1'], batch=None, x=torch.zeros(1))
    with pytest.raises(ValueError, match="1 graphs for 2 videos"):
        m.alignment_entropy_packed(pc, [ok])
    with pytest.raises(ValueError, match="'v1'"):
        m.alignment_entropy_packed(pc, [ok, [2, 3]])
    nobody = SemiMarkovModel                                                    # (refused before the model is looked at)
    wide = [[c] * 100 for c in range(3)]                                        # a trie of 300 nodes
    with pytest.raises(ValueError, match="candidate_entropy.*'v'.*300 nodes"):
        SemiMarkovModel.candidate_entropy(nobody, None, {'v': wide})
    with pytest.raises(ValueError, match="candidate_entropy: no candidates"):
        SemiMarkovModel.candidate_entropy(nobody, None, {'v': []})
    with pytest.raises(ValueError, match="alignment_entropy.*not both"):
        SemiMarkovModel.alignment_entropy(nobody, None, {'v': [0]}, optional_by_video={}, optional_classes=[0])


# ------------------------------------------------------------------------------------------------ the references
def _random_video(rng, i):
    while True:
        T, C, M, kp = int(rng.integers(1, 8)), int(rng.integers(1, 4)), int(rng.integers(1, 7)), int(rng.integers(2, 6))
        graph = TG.random_graph(rng, M, C, p_edge=(0.3, 0.6, 0.9)[i % 3])
        if TG.has_alignment_by_count(T, C, graph, kp):
            break
    elp, trans, init = rng.normal(size=(T, C)) * 2, rng.normal(size=(C, C)) * 2, rng.normal(size=C) * 2
    lens, ep = rng.normal(size=(kp + i % 2, C)) * 2, (rng.normal(size=C) if i % 2 == 0 else None)
    return elp, graph, trans, init, lens, kp, ep


def test_enumeration_chain_rule_and_identity_agree():
    """130 random DAGs (M <= 6, T <= 7, every other one under end penalties): -sum p log p over the enumerated alignments, the
    chain rule over the sampler's decisions and log Z_g - E[score] agree; the first part is the entropy of p_end; every part
    is >= 0."""
    rng = np.random.default_rng(20261020)
    n_fin, worst = 0, np.zeros(3)
    for i in range(130):
        elp, graph, trans, init, lens, kp, ep = _random_video(rng, i)
        h, lz, n = TE.enumeration_entropy(elp, graph, trans, init, lens, kp, ep)
        parts = TE.chain_rule(elp, graph, trans, init, lens, kp, ep)
        assert (parts is None) == (n == 0)
        if parts is None:
            continue
        n_fin += 1
        fb = TG.forward_backward(elp, graph, trans, init, lens, kp, ep)
        ident = TE.identity_entropy(fb['logz'], fb, elp, trans, init, lens, TG._graph(graph)[0], fb['p_end'], ep)
        bar = REF_BAR * max(1.0, h)
        assert min(parts) >= 0.0 and abs(fb['logz'] - lz) <= REF_BAR * max(1.0, abs(lz))
        errs = (abs(sum(parts) - h), abs(ident - h), abs(parts[0] - TE.entropy_of(fb['p_end'])))
        assert max(errs) <= bar, (i, h, parts, ident)
        assert n > 1 or h == 0.0
        worst = np.maximum(worst, errs)
    print('\n[transcript-entropy] references, %d graphs: chain rule %.1e, identity %.1e, H_end against p_end %.1e (bar %.0e)'
          % (n_fin, *worst, REF_BAR))
    assert n_fin >= 100


def test_a_trie_splits_into_candidate_and_boundary_entropy():
    """total = H(posterior over the candidates) + sum_c p_c H(chain of candidate c), and H_end is the first term."""
    from action_segmentation_amd import ops
    G = ops.TranscriptGraph
    rng = np.random.default_rng(8)
    C, kp, T = 3, 5, 7
    elp, trans, init, lens = rng.normal(size=(T, C)), rng.normal(size=(C, C)), rng.normal(size=C), rng.normal(size=(kp, C))
    for ep in (None, rng.normal(size=C)):
        cands = [[0, 1], [0, 1, 2], [2, 0], [2, 0, 1, 1]]
        trie = G.from_candidates(cands)
        tup = (trie.ids, trie.pred, trie.start, trie.end)
        total = TE.chain_rule(elp, tup, trans, init, lens, kp, ep)
        each = [TE.enumeration_entropy(elp, (np.array(c), np.eye(len(c), k=-1, dtype=bool), np.arange(len(c)) == 0,
                                             np.arange(len(c)) == len(c) - 1), trans, init, lens, kp, ep) for c in cands]
        z = np.array([e[1] for e in each])
        p = np.exp(z - (z.max() + np.log(np.exp(z - z.max()).sum())))
        want = TE.entropy_of(p) + float(sum(pc * e[0] for pc, e in zip(p, each)))
        assert abs(sum(total) - want) <= REF_BAR * max(1.0, want) and abs(total[0] - TE.entropy_of(p)) <= REF_BAR
        assert abs(sum(total) - TE.enumeration_entropy(elp, tup, trans, init, lens, kp, ep)[0]) <= REF_BAR * max(1.0, want)


def test_one_alignment_has_no_entropy_and_zero_tables_count():
    chain = (np.array([0, 1, 2]), np.eye(3, k=-1, dtype=bool), np.arange(3) == 0, np.arange(3) == 2)
    rng = np.random.default_rng(2)
    elp, trans, init, lens = rng.normal(size=(3, 3)), rng.normal(size=(3, 3)), rng.normal(size=3), rng.normal(size=(4, 3))
    assert TE.chain_rule(elp, chain, trans, init, lens, 4) == (0.0, 0.0, 0.0)
    assert TE.enumeration_entropy(elp, chain, trans, init, lens, 4) [0] == 0.0 and TE.count_alignments(3, chain, 4) == 1
    # all-zero tables: every alignment has the same mass, and the exact count is the enumeration's
    for i in range(30):
        _, graph, _, _, _, kp, _ = _random_video(rng, i)
        T, C = int(rng.integers(1, 8)), 3
        zeros = (np.zeros((T, C)), graph, np.zeros((C, C)), np.zeros(C), np.zeros((kp, C)), kp)
        h, _, n = TE.enumeration_entropy(*zeros)
        assert n == TE.count_alignments(T, graph, kp)
        if n:
            assert abs(h - np.log(n)) <= REF_BAR and abs(sum(TE.chain_rule(*zeros)) - np.log(n)) <= REF_BAR
    # C(39, 4) compositions of 40 frames into 5 segments, of which those with a segment over 15 frames are left out
    big = (np.zeros(5, np.int64), np.eye(5, k=-1, dtype=bool), np.arange(5) == 0, np.arange(5) == 4)
    assert TE.count_alignments(40, big, 41) == 82251 and 0 < TE.count_alignments(40, big, 16) < 82251


# ------------------------------------------------------------------------------------------------ premises of the GPU test
def test_the_exact_cases_have_entropy_to_measure():
    """What the GPU test of the tiny graphs assumes of test_gpu_transcript_sample.exact_cases(): every video has at least 4
    alignments and H > 0.1 nats."""
    import test_gpu_transcript_sample as GS
    for _, case, names in GS.exact_cases():
        for i, name in enumerate(names):
            _, lz, p = GS.enumerated(case, i)
            assert np.isfinite(lz) and len(p) >= 4 and TE.entropy_of(p.values()) > 0.1, (name, len(p))
