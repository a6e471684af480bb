"""Host-side argument checks of the posterior entropy's C entry point (no GPU: the call is refused before anything is staged)."""
import ctypes

import numpy as np

from action_segmentation_amd import _lib


def _call(out=ctypes.c_void_p(16), tables=ctypes.c_void_p(16), logz=ctypes.c_void_p(16)):
    lib = _lib.load()
    lengths = np.array([6], np.int64)
    shape = _lib.SmmShape(1, 0, 1, 3, 4, 6, 0, 6)
    p = ctypes.c_void_p(16)                       # (never dereferenced: the arguments are refused first)
    return lib.smm_entropy_f64(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data), None, None, None, None, p, tables,
                               p, tables, None, logz, out, None, ctypes.c_size_t(0), None)


def test_entropy_symbol_is_exported():
    lib = _lib.load()
    assert 'smm_entropy_f64' in _lib.SYMBOLS
    assert lib.smm_entropy_f64 is not None


def test_entropy_refuses_null_output_and_tables():
    assert _call(out=None) == -1                  # SMM_ERR_ARG
    assert _call(tables=None) == -1
    assert _call(logz=None) == -1
