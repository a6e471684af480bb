"""Host-side checks of the MBR decode's C entry points and of its switches (no GPU: the calls are refused before anything is
staged)."""
import ctypes

import numpy as np
import pytest

from action_segmentation_amd import _lib


def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _ws(lengths, **kw):
    lengths = np.asarray(lengths, np.int64)
    kw.setdefault('total', int(lengths.max()) * len(lengths))
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), **kw)
    return _lib.load().smm_mbr_workspace_bytes(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data))


def _call(shape=None, gain=ctypes.c_void_p(16), trans=ctypes.c_void_p(16), init=ctypes.c_void_p(16),
          best=ctypes.c_void_p(16), gain_sum=None, ws=ctypes.c_void_p(4096), ws_bytes=1 << 30):
    lib = _lib.load()
    lengths = np.array([6], np.int64)
    offsets = np.array([0], np.int64)
    n_states = np.array([3], np.int32)
    shape = shape or _shape()
    p = ctypes.c_void_p(16)                       # (never dereferenced: the arguments are refused first)
    return lib.smm_mbr_f64(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data), ctypes.c_void_p(offsets.ctypes.data),
                           None, None, ctypes.c_void_p(n_states.ctypes.data), gain, trans, init, None, None,
                           None, None, best, gain_sum, None, ws, ctypes.c_size_t(ws_bytes), p)


def test_mbr_symbols_are_exported():
    lib = _lib.load()
    for name in ('smm_mbr_f64', 'smm_mbr_workspace_bytes'):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None


def test_mbr_refuses_null_inputs_and_outputs():
    assert _call(gain=None) == -1                 # SMM_ERR_ARG
    assert _call(trans=None) == -1
    assert _call(init=None) == -1
    assert _call(ws=None) == -1
    assert _call(best=None) == -1                 # every output NULL
    assert _call(shape=_shape(b=0)) == -1


def test_mbr_refuses_unsupported_shapes():
    assert _call(shape=_shape(c=33)) == -2        # SMM_ERR_UNSUPPORTED
    assert _call(shape=_shape(k_rows=1025)) == -2


def test_mbr_refuses_a_short_workspace_before_staging():
    need = _ws([6])
    assert need > 0
    assert _call(ws_bytes=need - 1) == -3         # SMM_ERR_WORKSPACE
    assert _call(ws_bytes=0, best=None, gain_sum=ctypes.c_void_p(16)) == -3


def test_mbr_workspace_bytes():
    lib = _lib.load()
    lengths = np.array([6], np.int64)
    base = lib.smm_workspace_bytes(ctypes.byref(_shape()), ctypes.c_void_p(lengths.ctypes.data))
    # the decode keeps its rows in the history area every entry point has: the same size, growing with the frames
    assert _ws([6]) == base
    assert _ws([6, 6]) < _ws([6, 60]) < _ws([600, 60])
    assert _ws([6], flags=1) == _ws([6])                         # add_eos=False
    # 0 on bad arguments
    assert _ws([0]) == 0                                         # an empty video
    assert _ws([6], c=33) == 0 and _ws([6], k_rows=1025) == 0 and _ws([6], k_rows=1) == 0
    shape = _shape(t_max=4)                                      # a video longer than t_max
    assert lib.smm_mbr_workspace_bytes(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data)) == 0
    assert lib.smm_mbr_workspace_bytes(ctypes.byref(_shape()), None) == 0
    assert lib.smm_mbr_workspace_bytes(None, ctypes.c_void_p(lengths.ctypes.data)) == 0


def test_decoder_flag_and_its_default():
    from action_segmentation_amd import cli
    args = cli.build_parser().parse_args(['--classifier', 'semimarkov'])
    assert args.sm_decoder == 'viterbi'
    args = cli.build_parser().parse_args(['--classifier', 'semimarkov', '--sm_decoder', 'mbr'])
    assert args.sm_decoder == 'mbr'
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(['--classifier', 'semimarkov', '--sm_decoder', 'argmax'])


def test_predict_refuses_an_unknown_decoder():
    from action_segmentation_amd import synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    data = synth.SynthDatasplit('tiny', seed=11)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    assert model.args.sm_decoder == 'viterbi'
    with pytest.raises(ValueError):
        model.predict(data, decoder='argmax')
