"""Host-side checks of the forced alignment with optional transcript entries: the reference restatement
tests/align_optional_ref.py against the C twin on the expanded lattice, against tests/align_ref.py when no flag is set and
against a brute force over every subset and composition; the rule that decides by counting whether there is an alignment; the
C entry points' refusals (no GPU: every call is refused before anything is staged) and the Python-level argument checks."""
import ctypes
import itertools

import numpy as np
import pytest

import align_optional_ref as O
import align_ref as R
from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)
DENSITIES = (0.0, 0.3, 0.6, 1.0)


def _case(rng, ties, density, T=None, C=None, kp=None, M=None, with_endpen=None):
    """A random video that has an alignment by counting: T < 40, M < 14, kp < 12, C <= 5."""
    C = C or int(rng.integers(1, 6))
    for _ in range(10000):
        t, k, m = T or int(rng.integers(1, 40)), kp or int(rng.integers(2, 12)), M or int(rng.integers(1, 14))
        opt = rng.random(m) < density
        if O.feasible_by_count(t, opt, k):
            break
    else:
        raise AssertionError("no video with an alignment drawn")
    T, kp = t, k
    a = rng.integers(0, C, size=m)
    K = kp + int(rng.integers(0, 3))
    if ties:
        draw = lambda *s: rng.integers(-3, 4, size=s).astype(np.float64)
    else:
        draw = lambda *s: rng.normal(size=s) * 3.0
    with_endpen = rng.random() < 0.5 if with_endpen is None else with_endpen
    return dict(elp=draw(T, C), a=a, opt=opt, trans=draw(C, C), init=draw(C), len_scores=draw(K, C), kp=kp,
                endpen=rng.integers(-3, 4, size=C).astype(np.float64) if with_endpen else None)


def _valid(c, segs):
    """The segments name a sub-sequence of the transcript that keeps every mandatory entry, within the span limit."""
    T = c['elp'].shape[0]
    starts, entries = [s for s, _ in segs], [j for _, j in segs]
    assert starts[0] == 0 and all(0 < e - s < c['kp'] for s, e in zip(starts, starts[1:] + [T]))
    assert all(x < y for x, y in zip(entries, entries[1:]))
    assert all(c['opt'][m] or m in entries for m in range(len(c['a'])))


def _score(c, segs):
    """The score of a segmentation, summed term by term."""
    T, a = c['elp'].shape[0], c['a']
    ends = [s for s, _ in segs[1:]] + [T]
    sc = c['init'][a[segs[0][1]]] + (0.0 if c['endpen'] is None else c['endpen'][a[segs[-1][1]]])
    for i, ((s, j), e) in enumerate(zip(segs, ends)):
        sc += c['elp'][s:e, a[j]].sum() + c['len_scores'][e - s, a[j]]
        if i:
            sc += c['trans'][a[j], a[segs[i - 1][1]]]
    return sc


def test_the_reference_equals_the_twin_on_the_expanded_lattice():
    rng = np.random.default_rng(20261019)
    n = skipped = taken = 0
    for i in range(256):
        c = _case(rng, ties=i % 2 == 0, density=DENSITIES[(i // 2) % 4])
        best, segs = O.align_optional_ref(**c)
        v, tw = O.twin_align(**c)
        assert best == v and segs == tw, (i, best, v, segs, tw)
        _valid(c, segs)
        u = O.used_flags(segs, len(c['a']))
        skipped += int((u[c['opt']] == 0).sum())
        taken += int((u[c['opt']] == 1).sum())
        n += 1
    assert n >= 200 and skipped > 100 and taken > 100


def test_the_reference_equals_align_ref_when_no_flag_is_set():
    rng = np.random.default_rng(4)
    for i in range(120):
        c = _case(rng, ties=i % 2 == 0, density=0.0)
        best, segs = O.align_optional_ref(**c)
        closing = 0.0 if c['endpen'] is None else float(c['endpen'][c['a'][-1]])
        want, starts = R.align_ref(c['elp'], c['a'], c['trans'], c['init'], c['len_scores'], c['kp'], closing=closing)
        assert best == want and segs == list(zip(starts, range(len(starts)))), i
    # ... also on what has no alignment, and on a NaN
    c = _case(rng, ties=False, density=0.0, T=6, kp=4, M=3)
    for a, kp in ((list(c['a']) * 3, 4), (c['a'], 2), ([0, 9, 0], 4)):
        assert O.align_optional_ref(c['elp'], a, [0] * len(a), c['trans'], c['init'], c['len_scores'], kp) == (-np.inf, None)
        assert R.align_ref(c['elp'], a, c['trans'], c['init'], c['len_scores'], kp) == (-np.inf, None)
    c['elp'][2, 0] = np.nan
    assert np.isnan(O.align_optional_ref(**c)[0])


@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
def test_the_reference_equals_the_brute_force(ties):
    """T <= 8, M <= 5: the best of every subset of the optional entries left out and every composition.  Integer inputs:
    every score is exact in any order.  Real inputs: a score is a sum of at most 2 T + 2 M + 2 terms of magnitude < 20, no
    longer than in tests/test_gpu_align.py, whose bound 4e-12 holds here as it does there."""
    rng = np.random.default_rng(12 + ties)
    n = 0
    for T in range(1, 9):
        for M in range(1, 6):
            for density in DENSITIES:
                kp = int(rng.integers(2, 7))
                opt = rng.random(M) < density
                if not O.feasible_by_count(T, opt, kp):
                    continue
                c = _case(rng, ties, density, T=T, C=3, kp=kp, M=M)
                best, segs = O.align_optional_ref(**c)
                want, arg = O.brute_force(**c)
                _valid(c, segs)
                if ties:
                    assert best == want == _score(c, segs), (T, M, best, want)
                else:
                    assert abs(best - want) < 4e-12 and abs(_score(c, segs) - want) < 4e-12, (T, M, best, want)
                n += 1
    assert n > 60


def test_the_count_rule_is_the_recursions_own_answer():
    """All T <= 12, kp <= 6, M <= 8, every flag pattern for M <= 6 (a sample of them beyond): the rule "mandatory count > T,
    M (kp - 1) < T or kp - 1 < 1" names exactly the videos for which the recursion, left to itself, finds nothing."""
    rng = np.random.default_rng(2)
    len_scores, trans, init = rng.normal(size=(8, 2)), rng.normal(size=(2, 2)), rng.normal(size=2)
    n_inf = n_fin = 0
    for T in range(1, 13):
        elp = rng.normal(size=(T, 2))
        for M in range(1, 9):
            a = rng.integers(0, 2, size=M)
            patterns = (list(itertools.product((0, 1), repeat=M)) if M <= 6
                        else [tuple(rng.integers(0, 2, size=M)) for _ in range(12)] + [(0,) * M, (1,) * M])
            for opt in patterns:
                for kp in range(1, 7):
                    rule = O.feasible_by_count(T, opt, kp)
                    mand = M - sum(opt)
                    assert rule == (kp >= 2 and mand <= T and M * (kp - 1) >= T)
                    best, segs = O.align_optional_ref(elp, a, opt, trans, init, len_scores, kp, count_rule=False)
                    assert np.isfinite(best) == rule, (T, M, opt, kp, best)
                    assert O.align_optional_ref(elp, a, opt, trans, init, len_scores, kp)[0] == best
                    n_inf += not rule
                    n_fin += rule
    assert n_inf > 1000 and n_fin > 1000


# ------------------------------------------------------------------------------------------------ the C entry points
def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _ws(lengths, ms, entry='smm_align_opt_workspace_bytes', **kw):
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    kw.setdefault('total', int(lengths.max()) * len(lengths))
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), **kw)
    return getattr(_lib.load(), entry)(ctypes.byref(shape), _p(lengths), _p(off))


_UNSET = object()


def _call(shape=None, off=_UNSET, elp=POISON, trans=POISON, init=POISON, len_scores=POISON, transcript=POISON, optional=POISON,
          best=POISON, spans=None, used=None, ws=POISON, ws_bytes=1 << 40, lengths=_UNSET, n_states=_UNSET, frame_off=_UNSET):
    lib = _lib.load()
    lengths = np.array([6], np.int64) if lengths is _UNSET else lengths
    frame_off = np.array([0], np.int64) if frame_off is _UNSET else frame_off
    n_states = np.array([3], np.int32) if n_states is _UNSET else n_states
    off = np.array([0, 2], np.int64) if off is _UNSET else off
    shape = shape or _shape()
    return lib.smm_align_opt_f64(ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), elp, trans, init,
                                 len_scores, None, None, transcript, optional, _p(off), spans, None, best, None, used, ws,
                                 ctypes.c_size_t(ws_bytes), POISON)


def test_the_new_symbols_are_exported():
    lib = _lib.load()
    for name in ('smm_align_opt_f64', 'smm_align_opt_workspace_bytes'):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None


def test_refuses_bad_arguments_before_staging():
    for name in ('elp', 'trans', 'init', 'len_scores', 'transcript', 'optional', 'ws', 'off', 'lengths', 'n_states',
                 'frame_off'):
        assert _call(**{name: None}) == ARG, name
    assert _call(best=None) == ARG                                      # every output NULL (`used` is none of the four)
    assert _call(best=None, used=POISON) == ARG
    assert _call(best=None, spans=POISON, ws_bytes=0) == WORKSPACE      # (one output is enough to get further)
    assert _call(shape=_shape(b=0)) == ARG
    assert _call(off=np.array([0, 0], np.int64)) == ARG                 # M = 0
    assert _call(off=np.array([2, 1], np.int64)) == ARG                 # non-monotone
    two = dict(shape=_shape(b=2), lengths=np.array([6, 6], np.int64), frame_off=np.array([0, 6], np.int64))
    assert _call(off=np.array([0, 3, 2], np.int64), **two) == ARG
    assert _call(off=np.array([0, 3, 3], np.int64), **two) == ARG
    assert _call(off=np.array([0, 3, 5], np.int64), ws_bytes=0, **two) == WORKSPACE


def test_refuses_unsupported_shapes_before_staging():
    assert _call(shape=_shape(flags=_lib.SHAPE_NO_EOS)) == UNSUPPORTED
    assert _call(shape=_shape(c=33)) == UNSUPPORTED
    assert _call(shape=_shape(k_rows=1025)) == UNSUPPORTED
    assert _call(off=np.array([0, 257], np.int64)) == UNSUPPORTED
    assert _call(off=np.array([0, 256], np.int64), ws_bytes=0) == WORKSPACE


def test_refuses_a_short_workspace_before_staging():
    need = _ws([6], [2])
    assert need > 0
    assert _call(ws_bytes=need - 1) == WORKSPACE
    assert _call(ws_bytes=0) == WORKSPACE
    assert _call(ws_bytes=_ws([6], [2], entry='smm_align_workspace_bytes')) == WORKSPACE   # (the plain alignment's is too small)


def test_workspace_bytes():
    lib = _lib.load()
    plain = lambda lengths, ms, **kw: _ws(lengths, ms, entry='smm_align_workspace_bytes', **kw)
    # the running maxima: c_max columns per video behind the h columns
    assert _ws([6], [2]) >= plain([6], [2]) + 8 * 3 * 7
    assert _ws([6, 60], [2, 3], c=5) >= plain([6, 60], [2, 3], c=5) + 8 * 5 * (7 + 61)
    assert _ws([6], [1]) < _ws([6], [2]) < _ws([6], [6]) < _ws([6], [256])
    assert _ws([6], [3]) < _ws([7], [3]) < _ws([60], [3]) < _ws([600], [3])
    # 0 on bad arguments
    assert _ws([6], [0]) == 0 and _ws([6], [257]) == 0 and _ws([0], [1]) == 0
    assert _ws([6], [2], flags=_lib.SHAPE_NO_EOS) == 0
    assert _ws([6], [2], c=33) == 0 and _ws([6], [2], k_rows=1025) == 0 and _ws([6], [2], k_rows=1) == 0
    lengths, off = np.array([6], np.int64), np.array([0, 2], np.int64)
    assert lib.smm_align_opt_workspace_bytes(ctypes.byref(_shape(t_max=4)), _p(lengths), _p(off)) == 0   # longer than t_max
    assert lib.smm_align_opt_workspace_bytes(ctypes.byref(_shape()), None, _p(off)) == 0
    assert lib.smm_align_opt_workspace_bytes(ctypes.byref(_shape()), _p(lengths), None) == 0
    assert lib.smm_align_opt_workspace_bytes(None, _p(lengths), _p(off)) == 0


# ------------------------------------------------------------------------------------------------ Python-level argument checks
def test_ops_align_value_errors():
    import torch
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 5], [3], 4)
    ids, off = ops._transcript_arrays(batch, [[0, 1], [2, 2, 1]])
    flags = ops._optional_flags(off, [[True, False], np.array([0, 1, 1])])
    assert flags.dtype == np.uint8 and list(flags) == [1, 0, 0, 1, 1]
    assert list(ops._optional_flags(off, [torch.tensor([False, False]), [False] * 3])) == [0] * 5
    with pytest.raises(ValueError):
        ops._optional_flags(off, [[True, False]])                               # one sequence short
    with pytest.raises(ValueError):
        ops._optional_flags(off, [[True, False], [False, True]])                # one flag short
    with pytest.raises(ValueError):
        ops._optional_flags(off, [[True, False, False], [False, True, True]])   # one flag too many
    assert ops.align_opt_workspace_bytes(batch, off) > ops.align_workspace_bytes(batch, off)
    with pytest.raises(ValueError):
        ops.align_opt_workspace_bytes(batch, off[:-1])
    # ops.align_optional checks the flags before it touches a device
    z = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.align_optional(batch, z, z, z, z, [[0, 1], [2, 2, 1]], [[True, False]])
    with pytest.raises(ValueError):
        ops.align_optional(batch, z, z, z, z, [[0, 1], [2, 2, 1]], [[True, False], [True]])
    with pytest.raises(ValueError):
        ops.align_optional(batch, z, z, z, z, [[0, 1], [2, 2, 1]], None)                    # no flags: that is ops.align


def test_model_align_refuses_both_kinds_of_flags():
    from action_segmentation_amd import synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    data = synth.SynthDatasplit('tiny', seed=11)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    with pytest.raises(ValueError):
        model.align(data, {}, optional_by_video={}, optional_classes=[0])
