"""Host-side argument checks of the KL divergence's C entry point (no GPU: the call is refused before anything is staged)."""
import ctypes

import numpy as np

from action_segmentation_amd import _lib


def _call(out=ctypes.c_void_p(16), tables_p=ctypes.c_void_p(16), tables_q=ctypes.c_void_p(16), logz_q=ctypes.c_void_p(16),
          ws_q=ctypes.c_void_p(16)):
    lib = _lib.load()
    lengths = np.array([6], np.int64)
    shape = _lib.SmmShape(1, 0, 1, 3, 4, 6, 0, 6)
    p = ctypes.c_void_p(16)                       # (never dereferenced: the arguments are refused first)
    return lib.smm_kl_f64(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data), None, None, None, None,
                          p, tables_p, p, tables_p, None, p, None, ctypes.c_size_t(0),
                          p, tables_q, p, tables_q, None, logz_q, ws_q, ctypes.c_size_t(1 << 30),
                          out, None, None)


def test_kl_symbol_is_exported():
    lib = _lib.load()
    assert 'smm_kl_f64' in _lib.SYMBOLS
    assert lib.smm_kl_f64 is not None


def test_kl_refuses_null_output_and_tables():
    assert _call(out=None) == -1                  # SMM_ERR_ARG
    assert _call(tables_p=None) == -1
    assert _call(tables_q=None) == -1
    assert _call(logz_q=None) == -1
    assert _call(ws_q=None) == -1


def test_kl_refuses_a_short_workspace_of_q_before_staging():
    lib = _lib.load()
    lengths = np.array([6], np.int64)
    shape = _lib.SmmShape(1, 0, 1, 3, 4, 6, 0, 6)
    need = lib.smm_workspace_bytes(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data))
    p = ctypes.c_void_p(16)
    rc = lib.smm_kl_f64(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data), None, None, None, None,
                        p, p, p, p, None, p, p, ctypes.c_size_t(need), p, p, p, p, None, p, p, ctypes.c_size_t(need - 1),
                        p, None, None)
    assert rc == -3                               # SMM_ERR_WORKSPACE
