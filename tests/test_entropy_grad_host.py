"""Host-side argument checks of the entropy / cross-entropy / KL gradient entry points and their scratch-size query (no GPU:
every refused call returns before anything is staged or launched)."""
import ctypes

import numpy as np

from action_segmentation_amd import _lib

P = ctypes.c_void_p(16)                           # (never dereferenced: the arguments are refused first)


def _shape(lengths, c=3, k_rows=4, flags=0):
    return _lib.SmmShape(len(lengths), 0, 1, c, k_rows, int(max(lengths)), flags, int(sum(lengths)))


def _scratch_bytes(shape, lengths):
    return _lib.load().smm_entropy_bwd_scratch_bytes(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data))


def _entropy_bwd(tables=P, logz=P, outs=(P, P, P, P), scratch=P, scratch_bytes=1 << 30, lengths=np.array([6], np.int64)):
    shape = _shape(lengths)
    return _lib.load().smm_entropy_bwd_f64(
        ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data), None, None, None, None,
        P, tables, P, tables, None, logz, None, *outs, None, scratch, ctypes.c_size_t(scratch_bytes), P,
        ctypes.c_size_t(0), None)


def _kl_bwd(mode=1, tables_p=P, tables_q=P, ws_q=P, ws_q_bytes=1 << 30, outs=(P, P, P, P), scratch=P, scratch_bytes=1 << 30,
            lengths=np.array([6], np.int64)):
    shape = _shape(lengths)
    return _lib.load().smm_kl_bwd_f64(
        ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data), None, None, None, None,
        P, tables_p, P, tables_p, None, P, P, ctypes.c_size_t(0),
        P, tables_q, P, tables_q, None, P, ws_q, ctypes.c_size_t(ws_q_bytes), mode,
        None, *outs, None, scratch, ctypes.c_size_t(scratch_bytes), None)


def test_symbols_are_exported():
    lib = _lib.load()
    for name in ('smm_entropy_bwd_scratch_bytes', 'smm_entropy_bwd_f64', 'smm_kl_bwd_f64'):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None


def test_scratch_query_is_consistent():
    c, k_rows = 3, 4
    lengths = np.array([6, 4, 9], np.int64)
    fixed = (k_rows * c + c * c + 2 * c + 4 + 3) // 4 * 4       # per video: len | trans | init | closing | values
    want = 8 * (sum(6 * c * (int(t) + 1) for t in lengths) + len(lengths) * fixed)
    assert _scratch_bytes(_shape(lengths, c, k_rows), lengths) == want
    # it grows with every video's length, and the workspace query is untouched by it
    longer = lengths.copy()
    longer[1] += 1
    assert _scratch_bytes(_shape(longer, c, k_rows), longer) == want + 8 * 6 * c
    lib = _lib.load()
    ws = lib.smm_workspace_bytes(ctypes.byref(_shape(lengths, c, k_rows)), ctypes.c_void_p(lengths.ctypes.data))
    assert ws > 0
    # invalid shapes: 0
    assert _scratch_bytes(_shape(lengths, 33, k_rows), lengths) == 0                   # c_max > SMM_MAX_STATES
    assert _scratch_bytes(_shape(lengths, c, 1025), lengths) == 0                      # k_rows > SMM_MAX_K_ROWS
    bad = np.array([6, 0], np.int64)
    assert _scratch_bytes(_shape(bad, c, k_rows), bad) == 0


def test_entropy_bwd_refuses_null_arguments():
    assert _entropy_bwd(tables=None) == -1                      # SMM_ERR_ARG
    assert _entropy_bwd(logz=None) == -1
    assert _entropy_bwd(scratch=None) == -1
    for i in range(4):
        outs = [P] * 4
        outs[i] = None
        assert _entropy_bwd(outs=tuple(outs)) == -1


def test_entropy_bwd_refuses_a_short_scratch():
    lengths = np.array([6], np.int64)
    need = _scratch_bytes(_shape(lengths), lengths)
    assert need > 0
    assert _entropy_bwd(scratch_bytes=need - 1, lengths=lengths) == -3   # SMM_ERR_WORKSPACE


def test_kl_bwd_refuses_bad_mode_and_null_arguments():
    assert _kl_bwd(mode=2) == -1
    assert _kl_bwd(mode=-1) == -1
    assert _kl_bwd(tables_p=None) == -1
    assert _kl_bwd(tables_q=None) == -1
    assert _kl_bwd(ws_q=None) == -1
    assert _kl_bwd(scratch=None) == -1
    for i in range(4):
        outs = [P] * 4
        outs[i] = None
        assert _kl_bwd(outs=tuple(outs)) == -1


def test_kl_bwd_refuses_short_buffers():
    lengths = np.array([6], np.int64)
    shape = _shape(lengths)
    need = _lib.load().smm_workspace_bytes(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data))
    assert _kl_bwd(ws_q_bytes=need - 1, lengths=lengths) == -3
    sneed = _scratch_bytes(shape, lengths)
    assert _kl_bwd(ws_q_bytes=need, scratch_bytes=sneed - 1, lengths=lengths) == -3
