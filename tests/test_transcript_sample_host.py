"""Host-side checks of the transcript-graph sampler: the entry point is declared, listed and exported; the C call's refusals
(no GPU: every call is refused before anything is staged); the Python layers' argument checks; the enumeration of
tests/transcript_sample_ref.py against the family's other references; and the premise of the GPU test of the exact
distribution -- its enumerated posteriors keep a perfect sampler's expected total variation under 0.007."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import transcript_graph_ref as TG
import transcript_sample_ref as TS
from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)
NAME = 'smm_align_graph_sample_f64'
_UNSET = object()


def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _call(shape=None, off=_UNSET, elp=POISON, trans=POISON, init=POISON, len_scores=POISON, node_class=POISON, pred_mask=POISON,
          node_flags=POISON, logz=POISON, n_samples=4, outs=(POISON,) * 5, ws=POISON, ws_bytes=1 << 40, lengths=_UNSET,
          n_states=_UNSET, frame_off=_UNSET):
    lengths = np.array([6], np.int64) if lengths is _UNSET else lengths
    frame_off = np.array([0], np.int64) if frame_off is _UNSET else frame_off
    n_states = np.array([3], np.int32) if n_states is _UNSET else n_states
    off = np.array([0, 2], np.int64) if off is _UNSET else off
    shape = shape or _shape()
    return _lib.load().smm_align_graph_sample_f64(
        ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), elp, trans, init, len_scores, None, None,
        node_class, pred_mask, node_flags, _p(off), logz, ctypes.c_int32(n_samples), ctypes.c_uint64(1), *outs, ws,
        ctypes.c_size_t(ws_bytes), POISON)


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
    for name in ('elp', 'trans', 'init', 'len_scores', 'node_class', 'pred_mask', 'node_flags', 'logz', 'ws', 'off', 'lengths',
                 'n_states', 'frame_off'):
        assert _call(**{name: None}) == ARG, name
    assert _call(n_samples=0) == ARG and _call(n_samples=-3) == ARG
    assert _call(outs=(None,) * 5) == ARG                               # every output NULL
    for keep in range(5):                                               # ... any single one will do
        assert _call(outs=tuple(POISON if i == keep else None for i in range(5)), ws_bytes=0) == WORKSPACE, keep
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
    with pytest.raises(ValueError, match="n_samples"):
        ops.align_graph_sample(batch, z, z, z, z, graphs, z, 0, ws=z)
    with pytest.raises(ValueError, match="1 graphs for 2 videos"):
        ops.align_graph_sample(batch, z, z, z, z, graphs[:1], z, 4, ws=z)
    with pytest.raises(ValueError, match="add_eos"):
        ops.align_graph_sample(ops.Batch([6, 5], [3], 4, no_eos=True), z, z, z, z, graphs, z, 4, ws=z)
    staged = (torch.zeros(5, dtype=torch.int32), torch.zeros(40, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="staged"):
        ops.align_graph_sample(batch, z, z, z, z, graphs, z, 4, ws=z, staged=staged)
    with pytest.raises(ValueError, match="workspace"):                          # no workspace: not the forward call's
        ops.align_graph_sample(batch, z, z, z, z, graphs, z, 4)


def test_module_and_model_checks_fire_before_a_device_is_touched():
    from module_util import make_args
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    G = ops.TranscriptGraph
    m = SemiMarkovModule(make_args(6), 4, 3, allow_self_transitions=True)
    ok = G.from_candidates([[2, 3], [2, 1]])
    x, ln = torch.zeros(2, 5, 3), torch.tensor([5, 5])
    with pytest.raises(ValueError, match="add_eos"):
        m.sample_alignments(x, ln, None, [ok, ok], add_eos=False)
    with pytest.raises(ValueError, match="n_samples"):
        m.sample_alignments(x, ln, None, [ok, ok], n_samples=0)
    with pytest.raises(ValueError, match="1 graphs for 2 videos"):
        m.sample_alignments(x, ln, None, [ok])
    with pytest.raises(ValueError, match="video 1"):
        m.sample_alignments(x, ln, None, [ok, [2, 3]])
    pc = types.SimpleNamespace(video_names=['v0', 'v1'], batch=None, x=torch.zeros(1))
    with pytest.raises(ValueError, match="1 graphs for 2 videos"):
        m.sample_alignments_packed(pc, [ok], 4)
    with pytest.raises(ValueError, match="n_samples"):
        m.sample_alignments_packed(pc, [ok, ok], 0)
    with pytest.raises(ValueError, match="'v1'"):
        m.sample_alignments_packed(pc, [ok, [2, 3]], 4)
    nobody = SemiMarkovModel                                                    # (refused before the model is looked at)
    wide = [[c] * 100 for c in range(3)]                                        # a trie of 300 nodes
    with pytest.raises(ValueError, match="'v'.*300 nodes"):
        SemiMarkovModel.sample_candidates(nobody, None, {'v': wide}, 4)
    with pytest.raises(ValueError, match="no candidates"):
        SemiMarkovModel.sample_candidates(nobody, None, {'v': []}, 4)
    with pytest.raises(ValueError, match="n_samples"):
        SemiMarkovModel.sample_candidates(nobody, None, {'v': [[0]]}, 0)
    with pytest.raises(ValueError, match="n_samples"):
        SemiMarkovModel.sample_alignments(nobody, None, {'v': [0]}, 0)
    with pytest.raises(ValueError, match="not both"):
        SemiMarkovModel.sample_alignments(nobody, None, {'v': [0]}, 2, optional_by_video={}, optional_classes=[0])


# ------------------------------------------------------------------------------------------------ the enumeration
def test_enumeration_against_the_graph_references():
    """log Z_g, the frame occupancy, p_used and p_end of the enumerated alignments equal transcript_graph_ref's brute force;
    a key survives the round trip through (used nodes, span row) and rescore gives its score."""
    rng = np.random.default_rng(20261019)
    n_fin = 0
    for i in range(120):
        while True:
            T, C, M, kp = int(rng.integers(1, 8)), int(rng.integers(1, 4)), int(rng.integers(1, 7)), int(rng.integers(2, 6))
            graph = TG.random_graph(rng, M, C, p_edge=(0.3, 0.6, 0.9)[i % 3])
            if TG.has_alignment_by_count(T, C, graph, kp):
                break
        elp, trans, init = rng.normal(size=(T, C)) * 2, rng.normal(size=(C, C)) * 2, rng.normal(size=C) * 2
        lens, ep = rng.normal(size=(kp + i % 2, C)) * 2, (rng.normal(size=C) if i % 3 == 0 else None)
        aligns = TS.enumerate_alignments(elp, graph, trans, init, lens, kp, ep)
        lz, p = TS.posterior(aligns)
        zb, occ, pu, pe = TG.brute_logz_graph(elp, graph, trans, init, lens, kp, ep)
        assert np.isfinite(lz) == np.isfinite(zb)
        if not np.isfinite(lz):
            continue
        n_fin += 1
        assert abs(lz - zb) <= 1e-9 * max(1.0, abs(zb)) and abs(sum(p.values()) - 1.0) <= 1e-9
        mine_occ, mine_pu, mine_pe = np.zeros((T, C)), np.zeros(M), np.zeros(M)
        for key, pk in p.items():
            lab = TS.labels_of(graph, T, key)
            mine_occ[np.arange(T), lab] += pk
            mine_pu[list(key[0])] += pk
            mine_pe[key[0][-1]] += pk
            used = np.zeros(M, np.int32)
            used[list(key[0])] = 1
            row = np.full(T + 3, -1, np.int64)
            row[[0] + list(key[1])] = [graph[0][m] for m in key[0]]
            row[T] = C
            back, sc = TS.rescore(elp, graph, trans, init, lens, kp, ep, used, row)
            assert back == key and sc == aligns[key]
        assert max(np.abs(mine_occ - occ).max(), np.abs(mine_pu - pu).max(), np.abs(mine_pe - pe).max()) <= 1e-9
    assert n_fin > 80


def test_inconsistent_samples_are_caught():
    graph = (np.array([0, 1, 2]), np.eye(3, k=-1, dtype=bool), np.arange(3) == 0, np.arange(3) == 2)
    good = np.array([0, -1, 1, 2, -1, 3, -1], np.int64)                          # T = 5, EOS id 3
    assert TS.alignment_of(graph, 5, 4, [1, 1, 1], good, eos=3) == ((0, 1, 2), (2, 3))
    for used, row in (([1, 0, 1], good),                                         # fewer nodes than segments
                      ([1, 1, 1], np.array([0, -1, 2, 1, -1, 3, -1])),           # a class that is not its node's
                      ([1, 1, 1], np.array([0, -1, 1, 2, -1, 3, 0])),            # something behind T
                      ([1, 1, 1], np.array([-1, 0, 1, 2, -1, 3, -1]))):          # no segment starts at 0
        with pytest.raises(AssertionError):
            TS.alignment_of(graph, 5, 4, used, np.asarray(row, np.int64), eos=3)
    with pytest.raises(AssertionError):
        TS.alignment_of(graph, 5, 3, [1, 1, 1], np.array([0, 1, 2, -1, -1, 3, -1], np.int64), eos=3)   # a segment of 3 > kp - 1


def test_the_exact_cases_leave_room_under_the_bar():
    """What the GPU test of the exact distribution assumes of its own cases: every video has alignments, their enumerated
    posterior keeps E[TV] of 100 000 perfect draws <= 0.007 (the test's bar is 0.01), the diamond is ambiguous with mass on both
    arms, the trie has an end node with a successor, the random graph a dead node."""
    import align_graph_ref as AG
    import test_gpu_transcript_sample as GS
    cases = GS.exact_cases()
    assert [len(c.vids) for _, c, _ in cases] == [6, 2] and [c.k_rows for _, c, _ in cases] == [4, 8]
    assert {t for _, c, _ in cases for t in c.lengths} == {5, 6, 7} and all(c.k_rows > max(c.lengths) for _, c, _ in cases[1:])
    for _, case, names in cases:
        for i, name in enumerate(names):
            aligns, lz, p = GS.enumerated(case, i)
            assert np.isfinite(lz) and len(p) >= 4, name
            assert TS.expected_tv(p.values(), GS.N_EXACT) <= 0.007, (name, TS.expected_tv(p.values(), GS.N_EXACT))
    short = cases[0][1]
    assert short.graphs[3].is_ambiguous()
    _, _, p = GS.enumerated(short, 3)
    arms = [sum(pk for k, pk in p.items() if arm in k[0]) for arm in (1, 2)]
    assert min(arms) > 0.01, arms
    trie = short.graphs[2]
    assert any(trie.end[j] and trie.pred[:, j].any() for j in range(len(trie)))
    rg = short.graphs[4]
    assert len({m for path in AG.paths(rg.pred, rg.start, rg.end) for m in path}) < len(rg)
    assert short.endpen[-1].any() and not short.endpen[:-1].any()
