"""Host-side checks of the forced alignment: the C entry points' refusals (no GPU: every call is refused before anything is
staged), the reference restatement tests/align_ref.py against the C twin on the expanded lattice and against the twin's Viterbi,
and the Python-level argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import align_ref as R
from action_segmentation_amd import _lib
from oracle import factored as F

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)


def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _ws(lengths, ms, **kw):
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    kw.setdefault('total', int(lengths.max()) * len(lengths))
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), **kw)
    return _lib.load().smm_align_workspace_bytes(ctypes.byref(shape), _p(lengths), _p(off))


_UNSET = object()


def _call(shape=None, off=_UNSET, elp=POISON, trans=POISON, init=POISON, len_scores=POISON, transcript=POISON, best=POISON,
          spans=None, ws=POISON, ws_bytes=1 << 40, lengths=_UNSET, n_states=_UNSET, frame_off=_UNSET):
    lib = _lib.load()
    lengths = np.array([6], np.int64) if lengths is _UNSET else lengths
    frame_off = np.array([0], np.int64) if frame_off is _UNSET else frame_off
    n_states = np.array([3], np.int32) if n_states is _UNSET else n_states
    off = np.array([0, 2], np.int64) if off is _UNSET else off
    shape = shape or _shape()
    return lib.smm_align_f64(ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), elp, trans, init,
                             len_scores, None, None, transcript, _p(off), spans, None, best, None, ws,
                             ctypes.c_size_t(ws_bytes), POISON)


def test_align_symbols_are_exported():
    lib = _lib.load()
    for name in ('smm_align_f64', 'smm_align_workspace_bytes'):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    assert _lib.MAX_TRANSCRIPT == 256
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'smmdp.h')).read()
    assert re.search(r'#define\s+SMM_MAX_TRANSCRIPT\s+256\b', header)


def test_align_refuses_bad_arguments_before_staging():
    for name in ('elp', 'trans', 'init', 'len_scores', 'transcript', 'ws', 'off', 'lengths', 'n_states', 'frame_off'):
        assert _call(**{name: None}) == ARG, name
    assert _call(best=None) == ARG                                      # every output NULL
    assert _call(best=None, spans=POISON, ws_bytes=0) == WORKSPACE      # (one output is enough to get further)
    assert _call(shape=_shape(b=0)) == ARG
    assert _call(off=np.array([0, 0], np.int64)) == ARG                 # M = 0
    assert _call(off=np.array([2, 1], np.int64)) == ARG                 # non-monotone
    two = dict(shape=_shape(b=2), lengths=np.array([6, 6], np.int64), frame_off=np.array([0, 6], np.int64))
    assert _call(off=np.array([0, 3, 2], np.int64), **two) == ARG
    assert _call(off=np.array([0, 3, 3], np.int64), **two) == ARG
    assert _call(off=np.array([0, 3, 5], np.int64), ws_bytes=0, **two) == WORKSPACE


def test_align_refuses_unsupported_shapes_before_staging():
    assert _call(shape=_shape(flags=_lib.SHAPE_NO_EOS)) == UNSUPPORTED
    assert _call(shape=_shape(c=33)) == UNSUPPORTED
    assert _call(shape=_shape(k_rows=1025)) == UNSUPPORTED
    assert _call(off=np.array([0, 257], np.int64)) == UNSUPPORTED
    assert _call(off=np.array([0, 256], np.int64), ws_bytes=0) == WORKSPACE


def test_align_refuses_a_short_workspace_before_staging():
    need = _ws([6], [2])
    assert need > 0
    assert _call(ws_bytes=need - 1) == WORKSPACE
    assert _call(ws_bytes=0) == WORKSPACE


def test_align_workspace_bytes():
    lib = _lib.load()
    lengths = np.array([6], np.int64)
    base = lib.smm_workspace_bytes(ctypes.byref(_shape()), _p(lengths))
    assert _ws([6], [1]) > base                                          # the h columns lie behind the common workspace
    # monotone in T and in M
    assert _ws([6], [1]) < _ws([6], [2]) < _ws([6], [6]) < _ws([6], [256])
    assert _ws([6], [3]) < _ws([7], [3]) < _ws([60], [3]) < _ws([600], [3])
    assert _ws([6, 6], [2, 2]) < _ws([6, 60], [2, 2]) < _ws([6, 60], [2, 3])
    # 0 on bad arguments
    assert _ws([6], [0]) == 0 and _ws([6], [257]) == 0 and _ws([0], [1]) == 0
    assert _ws([6], [2], flags=_lib.SHAPE_NO_EOS) == 0
    assert _ws([6], [2], c=33) == 0 and _ws([6], [2], k_rows=1025) == 0 and _ws([6], [2], k_rows=1) == 0
    off = np.array([0, 2], np.int64)
    assert lib.smm_align_workspace_bytes(ctypes.byref(_shape(t_max=4)), _p(lengths), _p(off)) == 0   # longer than t_max
    assert lib.smm_align_workspace_bytes(ctypes.byref(_shape()), None, _p(off)) == 0
    assert lib.smm_align_workspace_bytes(ctypes.byref(_shape()), _p(lengths), None) == 0
    assert lib.smm_align_workspace_bytes(None, _p(lengths), _p(off)) == 0
    assert lib.smm_align_workspace_bytes(ctypes.byref(_shape()), _p(lengths), _p(np.array([1, 0], np.int64))) == 0


def test_the_tile_size_the_gpu_tests_assume():
    """tests/test_gpu_align.py places its lengths around the kernel's tile: SMM_ALIGN_THREADS x SMM_ALIGN_R positions."""
    src = open(os.path.join(_lib.HERE, 'csrc', 'smm_align.hip')).read()
    threads = int(re.search(r'#define\s+SMM_ALIGN_THREADS\s+(\d+)', src).group(1))
    r = int(re.search(r'#define\s+SMM_ALIGN_R\s+(\d+)', src).group(1))
    assert threads * r == 768


# ------------------------------------------------------------------------------------------------ the reference and the twin
def _case(rng, ties, T=None, C=None, kp=None, M=None, repeats=False):
    C = C or int(rng.integers(1, 6))
    T = T or int(rng.integers(1, 40))
    kp = kp or int(rng.integers(2, 12))
    lo, hi = -(-T // (kp - 1)), T                                        # feasible M
    M = M or int(rng.integers(lo, min(hi, lo + 12) + 1))
    a = rng.integers(0, C, size=M)
    if repeats and M >= 3:
        a[1] = a[2] = a[0]
    K = kp + int(rng.integers(0, 3))
    if ties:
        draw = lambda *s: rng.integers(-3, 4, size=s).astype(np.float64)
    else:
        draw = lambda *s: rng.normal(size=s) * 3.0
    return dict(elp=draw(T, C), a=a, trans=draw(C, C), init=draw(C), len_scores=draw(K, C), kp=kp,
                closing=float(draw(1)[0]) if rng.random() < 0.5 else 0.0)


def test_align_ref_equals_the_twin_on_the_expanded_lattice():
    rng = np.random.default_rng(20261018)
    n = 0
    for i in range(240):
        c = _case(rng, ties=i % 2 == 0, repeats=i % 3 == 0)
        best, starts = R.align_ref(**c)
        v, tw = R.twin_align(**c)
        assert best == v and starts == tw, (i, best, v, starts, tw)
        assert starts[0] == 0 and all(0 < starts[m + 1] - starts[m] < c['kp'] for m in range(len(starts) - 1))
        n += 1
    assert n >= 200


def test_align_ref_with_forbidden_transitions_stays_finite():
    rng = np.random.default_rng(5)
    for i in range(20):
        c = _case(rng, ties=False, T=25, C=3, kp=9, M=6)
        for m in range(1, 6):
            c['trans'][c['a'][m], c['a'][m - 1]] = R.BIG_NEG if m % 2 else c['trans'][c['a'][m], c['a'][m - 1]]
        best, starts = R.align_ref(**c)
        assert np.isfinite(best) and best < -1e9 and starts is not None


def test_align_ref_is_minus_inf_exactly_on_the_count_infeasible_cases():
    rng = np.random.default_rng(9)
    for T in range(1, 14):
        for kp in range(1, 7):
            for M in range(1, 16):
                c = _case(rng, ties=False, T=T, C=2, kp=max(kp, 2), M=M)
                c['kp'] = kp
                c['len_scores'] = rng.normal(size=(8, 2))
                best, starts = R.align_ref(**c)
                ok = M <= T and M * (kp - 1) >= T
                assert R.feasible_by_count(T, M, kp) == ok
                assert (best == -np.inf and starts is None) if not ok else (np.isfinite(best) and len(starts) == M)
    # an id that is no state of the video: no alignment either
    c = _case(rng, ties=False, T=6, C=2, kp=4, M=3)
    c['a'][1] = 2
    assert R.align_ref(**c) == (-np.inf, None)


def test_align_ref_reproduces_the_twins_viterbi_on_its_own_transcript():
    rng = np.random.default_rng(77)
    for i in range(200):
        C, T, kp = int(rng.integers(1, 6)), int(rng.integers(1, 45)), int(rng.integers(2, 14))
        K = kp
        elp, trans, init, ls = rng.normal(size=(T, C)) * 2, rng.normal(size=(C, C)), rng.normal(size=C), rng.normal(size=(K, C))
        ep = np.where(rng.random(C) < 0.3, R.BIG_NEG, 0.0)
        ep[int(rng.integers(0, C))] = 0.0
        tm = max(T, kp)
        pad = np.zeros((1, tm, C))
        pad[0, :T] = elp
        spans, v = F.viterbi(pad, np.array([T], np.int64), trans, init, ls, ep[None])
        row = spans[0, :T]
        if spans[0, T] != C:
            continue                                                    # (closed on a real class at -1e9: no EOS path)
        pos = np.flatnonzero(row >= 0)
        a = row[pos]
        best, starts = R.align_ref(elp, a, trans, init, ls, kp, closing=float(ep[a[-1]]))
        assert best == v[0] and starts == [int(p) for p in pos], i


def test_spans_to_transcripts_round_trip():
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts
    rng = np.random.default_rng(3)
    for _ in range(20):
        b, t_max = 4, 12
        lengths = rng.integers(1, t_max + 1, size=b)
        spans = np.full((b, t_max + 1), -1, np.int64)
        want = []
        for i in range(b):
            T = int(lengths[i])
            M = int(rng.integers(1, T + 1))
            starts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, T), size=M - 1, replace=False))]).astype(int)
            a = rng.integers(0, 3, size=M)                              # (consecutive repeats occur)
            spans[i, starts] = a
            spans[i, T] = 7                                             # EOS
            want.append(a)
            assert np.array_equal(R.span_row(list(starts), a, T, t_max, eos=7), spans[i])
        got = spans_to_transcripts(spans, lengths)
        assert len(got) == b and all(np.array_equal(g, w) for g, w in zip(got, want))
        import torch
        got = spans_to_transcripts(torch.from_numpy(spans), torch.from_numpy(lengths))
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


# ------------------------------------------------------------------------------------------------ Python-level argument checks
def test_local_transcripts_and_their_value_errors():
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    cmap = np.array([[5, 2, 9, 11], [4, 7, 11, 0]], np.int64)           # two groups: 3 and 2 valid classes, then EOS, padding
    loc = SemiMarkovModule._local_transcripts([[9, 9, 5], [7]], cmap, [3, 2], [0, 1])
    assert [list(x) for x in loc] == [[2, 2, 0], [1]]
    with pytest.raises(ValueError):
        SemiMarkovModule._local_transcripts([[9, 4], [7]], cmap, [3, 2], [0, 1])      # 4 is valid for group 1 only
    with pytest.raises(ValueError):
        SemiMarkovModule._local_transcripts([[11], [7]], cmap, [3, 2], [0, 1])        # EOS is no class of the video
    with pytest.raises(ValueError):
        SemiMarkovModule._local_transcripts([[9], []], cmap, [3, 2], [0, 1])          # empty
    with pytest.raises(ValueError):
        SemiMarkovModule._local_transcripts([[9]], cmap, [3, 2], [0, 1])              # one transcript short


def test_module_align_refuses_add_eos_false():
    import torch
    from action_segmentation_amd import synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    data = synth.SynthDatasplit('tiny', seed=11)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    feats = torch.zeros((1, 4, model.model.n_dims if hasattr(model.model, 'n_dims') else 1))
    with pytest.raises(ValueError):
        model.model.align(feats, torch.tensor([4]), None, [[0]], add_eos=False)


def test_ops_align_value_errors():
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 5], [3], 4)
    with pytest.raises(ValueError):
        ops._transcript_arrays(batch, [[0, 1]])
    with pytest.raises(ValueError):
        ops._transcript_arrays(batch, [[0, 1], []])
    with pytest.raises(ValueError):
        ops._transcript_arrays(batch, [[0, 1], [0] * 257])
    ids, off = ops._transcript_arrays(batch, [[0, 1], np.array([2, 2, 1])])
    assert ids.dtype == np.int32 and list(ids) == [0, 1, 2, 2, 1] and list(off) == [0, 2, 5]
    assert ops.align_workspace_bytes(batch, off) > batch.workspace_bytes()
