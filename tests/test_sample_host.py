"""Host-side argument checks of the posterior sampler's C entry point (no GPU: the call is refused before anything is staged)."""
import ctypes

import numpy as np

from action_segmentation_amd import _lib


def _call(n_samples, spans=None, labels=None, logp=None):
    lib = _lib.load()
    lengths = np.array([6], np.int64)
    shape = _lib.SmmShape(1, 0, 1, 3, 4, 6, 0, 6)
    p = ctypes.c_void_p(16)                       # (never dereferenced: the arguments are refused first)
    return lib.smm_sample_f64(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data), None, None, None, None, p, p, p, p,
                              None, None, p, ctypes.c_int32(n_samples), ctypes.c_uint64(0), spans, labels, logp, None,
                              ctypes.c_size_t(0), None)


def test_sample_refuses_no_outputs_and_non_positive_counts():
    assert _call(4) == -1                                        # every output NULL
    assert _call(0, logp=ctypes.c_void_p(16)) == -1              # n_samples = 0
    assert _call(-3, spans=ctypes.c_void_p(16)) == -1
