"""Host-side checks of the transcript likelihood: the references of tests/transcript_ref.py against each other and against
enumeration, the C entry points' refusals (no GPU: every call is refused before anything is staged), the workspace query and the
Python-level argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

import align_ref as R
import transcript_ref as TR
from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)
_UNSET = object()


def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _ws(lengths, ms, **kw):
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    kw.setdefault('total', int(lengths.max()) * len(lengths))
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), **kw)
    return _lib.load().smm_align_logz_workspace_bytes(ctypes.byref(shape), _p(lengths), _p(off))


FWD_PTRS = ('elp', 'trans', 'init', 'len_scores', 'transcript', 'logz', 'ws')
BWD_PTRS = FWD_PTRS + ('g_elp', 'g_trans', 'g_init', 'g_len')


def _call(bwd, shape=None, off=_UNSET, ws_bytes=1 << 40, lengths=_UNSET, n_states=_UNSET, frame_off=_UNSET, **ptrs):
    lib = _lib.load()
    lengths = np.array([6], np.int64) if lengths is _UNSET else lengths
    frame_off = np.array([0], np.int64) if frame_off is _UNSET else frame_off
    n_states = np.array([3], np.int32) if n_states is _UNSET else n_states
    off = np.array([0, 2], np.int64) if off is _UNSET else off
    shape = shape or _shape()
    q = {name: ptrs.get(name, POISON) for name in BWD_PTRS}
    head = (ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), q['elp'], q['trans'], q['init'],
            q['len_scores'], None, q['transcript'], _p(off))
    tail = (q['ws'], ctypes.c_size_t(ws_bytes), POISON)
    if not bwd:
        return lib.smm_align_logz_f64(*head, q['logz'], *tail)
    return lib.smm_align_logz_bwd_f64(*head, q['logz'], None, q['g_elp'], q['g_trans'], q['g_init'], q['g_len'], *tail)


def test_the_three_symbols_are_exported():
    lib = _lib.load()
    for name in ('smm_align_logz_workspace_bytes', 'smm_align_logz_f64', 'smm_align_logz_bwd_f64'):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    header = open(os.path.join(os.path.dirname(_lib.HERE), 'include', 'smmdp.h')).read()
    for name in ('smm_align_logz_workspace_bytes', 'smm_align_logz_f64', 'smm_align_logz_bwd_f64'):
        assert re.search(r'\b%s\(' % name, header)


def test_the_tile_size_the_ops_layer_states():
    from action_segmentation_amd import ops
    src = open(os.path.join(_lib.HERE, 'csrc', 'smm_align_logz.hip')).read()
    threads = int(re.search(r'#define\s+SMM_ALIGN_THREADS\s+(\d+)', src).group(1))
    r = int(re.search(r'#define\s+SMM_ALIGN_R\s+(\d+)', src).group(1))
    assert threads * r == ops.ALIGN_LOGZ_TILE


@pytest.mark.parametrize('bwd', [False, True])
def test_refusals_before_staging(bwd):
    for name in (BWD_PTRS if bwd else FWD_PTRS) + ('off', 'lengths', 'n_states', 'frame_off'):
        assert _call(bwd, **{name: None}) == ARG, name
    assert _call(bwd, shape=_shape(b=0)) == ARG
    assert _call(bwd, off=np.array([0, 0], np.int64)) == ARG                 # an empty transcript
    assert _call(bwd, off=np.array([2, 1], np.int64)) == ARG                 # non-monotone
    two = dict(shape=_shape(b=2), lengths=np.array([6, 6], np.int64), frame_off=np.array([0, 6], np.int64))
    assert _call(bwd, off=np.array([0, 3, 2], np.int64), **two) == ARG
    assert _call(bwd, off=np.array([0, 3, 3], np.int64), **two) == ARG
    assert _call(bwd, off=np.array([0, 3, 5], np.int64), ws_bytes=0, **two) == WORKSPACE
    assert _call(bwd, shape=_shape(flags=_lib.SHAPE_NO_EOS)) == UNSUPPORTED
    assert _call(bwd, shape=_shape(c=33)) == UNSUPPORTED
    assert _call(bwd, shape=_shape(k_rows=1025)) == UNSUPPORTED
    assert _call(bwd, off=np.array([0, 257], np.int64)) == UNSUPPORTED
    assert _call(bwd, off=np.array([0, 256], np.int64), ws_bytes=0) == WORKSPACE
    need = _ws([6], [2])
    assert need > 0
    assert _call(bwd, ws_bytes=need - 1) == WORKSPACE
    assert _call(bwd, ws_bytes=0) == WORKSPACE


def test_workspace_bytes():
    lib = _lib.load()
    lengths = np.array([6], np.int64)
    base = lib.smm_workspace_bytes(ctypes.byref(_shape()), _p(lengths))
    off = np.array([0, 1], np.int64)
    assert _ws([6], [1]) > lib.smm_align_workspace_bytes(ctypes.byref(_shape()), _p(lengths), _p(off)) > base
    # grows with T and with M
    assert _ws([6], [1]) < _ws([6], [2]) < _ws([6], [6]) < _ws([6], [256])
    assert _ws([6], [3]) < _ws([7], [3]) < _ws([60], [3]) < _ws([600], [3])
    assert _ws([6, 6], [2, 2]) < _ws([6, 60], [2, 2]) < _ws([6, 60], [2, 3])
    # 0 on whatever the calls refuse
    assert _ws([6], [0]) == 0 and _ws([6], [257]) == 0 and _ws([0], [1]) == 0
    assert _ws([6], [2], flags=_lib.SHAPE_NO_EOS) == 0
    assert _ws([6], [2], c=33) == 0 and _ws([6], [2], k_rows=1025) == 0 and _ws([6], [2], k_rows=1) == 0
    off = np.array([0, 2], np.int64)
    f = lib.smm_align_logz_workspace_bytes
    assert f(ctypes.byref(_shape(t_max=4)), _p(lengths), _p(off)) == 0   # longer than t_max
    assert f(ctypes.byref(_shape()), None, _p(off)) == 0
    assert f(ctypes.byref(_shape()), _p(lengths), None) == 0
    assert f(None, _p(lengths), _p(off)) == 0
    assert f(ctypes.byref(_shape()), _p(lengths), _p(np.array([1, 0], np.int64))) == 0


# ------------------------------------------------------------------------------------------------ the references
def _case(rng, T=None, C=None, kp=None, M=None, repeats=False):
    C = C or int(rng.integers(1, 6))
    T = T or int(rng.integers(1, 40))
    kp = kp or int(rng.integers(2, 12))
    lo, hi = -(-T // (kp - 1)), T                                        # feasible M
    M = M or int(rng.integers(lo, min(hi, lo + 12) + 1))
    a = rng.integers(0, C, size=M)
    if repeats and M >= 3:
        a[1] = a[2] = a[0]
    K = kp + int(rng.integers(0, 3))
    draw = lambda *s: rng.normal(size=s) * 3.0
    return dict(elp=draw(T, C), a=a, trans=draw(C, C), init=draw(C), len_scores=draw(K, C), kp=kp,
                closing=float(draw(1)[0]) if rng.random() < 0.5 else 0.0)


def test_the_two_references_agree_on_random_cases():
    rng = np.random.default_rng(20261019)
    for i in range(60):
        c = _case(rng, repeats=i % 3 == 0)
        zt, gt = TR.torch_grads(**c)
        zw, gw = TR.twin_grads(**c)
        assert abs(zt - zw) <= 1e-10 * max(1.0, abs(zw)), (i, zt, zw)
        for k in ('elp', 'trans', 'init', 'len'):
            assert np.abs(gt[k] - gw[k]).max() <= 1e-9, (i, k)
        tr, st, n = TR.counts(c['a'], c['elp'].shape[1])
        assert np.abs(gt['trans'] - tr).max() <= 1e-12 and np.abs(gt['init'] - st).max() <= 1e-12
        assert np.abs(gt['elp'].sum(1) - 1.0).max() <= 1e-9               # every frame lies in one segment
        assert np.abs(gt['len'].sum(0) - n).max() <= 1e-9                 # every entry has one length
        best, _ = R.align_ref(**c)
        assert best <= zt + 1e-9


def test_the_references_equal_enumeration_on_small_cases():
    rng = np.random.default_rng(8)
    n = 0
    for T in range(1, 9):
        for M in range(1, T + 1):
            kp = int(rng.integers(2, 6))
            if M * (kp - 1) < T:
                continue
            c = _case(rng, T=T, C=2, kp=kp, M=M)
            zb, occ = TR.brute_logz(**c)
            zt, gt = TR.torch_grads(**c)
            zw, gw = TR.twin_grads(**c)
            assert abs(zt - zb) <= 1e-12 * max(1.0, abs(zb)) and abs(zw - zb) <= 1e-12 * max(1.0, abs(zb))
            assert np.abs(gt['elp'] - occ).max() <= 1e-12 and np.abs(gw['elp'] - occ).max() <= 1e-12
            n += 1
    assert n >= 20


def test_the_torch_reference_on_count_infeasible_and_forbidden_cases():
    rng = np.random.default_rng(4)
    c = _case(rng, T=6, C=2, kp=4, M=1)                                  # one segment of at most 3 frames
    z, g = TR.torch_grads(**c)
    assert z == -np.inf and all(not v.any() for v in g.values())
    c = _case(rng, T=6, C=2, kp=4, M=3)
    c['a'][1] = 2                                                        # no state of the video
    assert TR.torch_grads(**c)[0] == -np.inf
    c = _case(rng, T=9, C=3, kp=5, M=3)
    c['len_scores'][2, :] = -np.inf                                      # some alignments are left
    z, g = TR.torch_grads(**c)
    assert np.isfinite(z) and all(np.isfinite(v).all() for v in g.values())
    c['len_scores'][1:, c['a'][0]] = -np.inf                             # none is left
    z, g = TR.torch_grads(**c)
    assert z == -np.inf and all(not v.any() for v in g.values())


# ------------------------------------------------------------------------------------------------ Python-level argument checks
def _tiny_model():
    from action_segmentation_amd import synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    data = synth.SynthDatasplit('tiny', seed=11)
    return SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data).model


def test_module_refuses_add_eos_false_spans_with_transcripts_and_a_foreign_class():
    import torch
    m = _tiny_model()
    feats = torch.zeros((1, 4, m.input_feature_dim))
    lengths = torch.tensor([4])
    with pytest.raises(ValueError):
        m.transcript_log_partition(feats, lengths, None, [[0]], add_eos=False)
    with pytest.raises(ValueError):
        m.log_likelihood(feats, lengths, None, spans=torch.zeros((1, 4), dtype=torch.long), transcripts=[[0]])
    with pytest.raises(ValueError):
        m.log_likelihood(feats, lengths, None, transcripts=[[0]], add_eos=False)
    valid = [torch.tensor([0, 1])]
    with pytest.raises(ValueError):
        m.transcript_log_partition(feats, lengths, valid, [[0, m.n_classes - 1]])        # not a class of this video
    with pytest.raises(ValueError):
        m.transcript_log_partition(feats, lengths, valid, [[m.n_classes]])               # EOS is no class
    with pytest.raises(ValueError):
        m.transcript_log_partition(feats, lengths, valid, [[]])
    with pytest.raises(ValueError):
        m.transcript_log_partition(feats, lengths, valid, [[0], [1]])                    # one transcript too many


def test_ops_workspace_query_and_value_errors():
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 5], [3], 4)
    ids, off = ops._transcript_arrays(batch, [[0, 1], np.array([2, 2, 1])])
    assert ops.align_logz_workspace_bytes(batch, off) > ops.align_workspace_bytes(batch, off)
    with pytest.raises(ValueError):
        ops.align_logz_workspace_bytes(batch, off[:-1])
    with pytest.raises(_lib.SmmError):
        ops.align_logz_workspace_bytes(batch, np.array([0, 2, 2], np.int64))
