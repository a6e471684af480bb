"""Refusal table of the C ABI (include/smmdp.h): for every entry point, each single fault that is refused before any HIP call,
with its status.  No GPU: a refused call touches neither a device pointer nor the runtime, so device pointers are a poison
value.  One fault per call; the precedence among simultaneous faults is not pinned.

Entry points whose own checks come first (entropy, KL, both gradients, k-best, MBR, align, dense) refuse more than the ones that
go straight to staging, which share stage()'s checks: a null shape, an invalid shape, a null length / offset / n_states array,
a null workspace.  What staging refuses later (limits, lengths, a short workspace) follows HIP calls and is not in this table.

Rows that another host test already asserts are listed in COVERED, not repeated.
"""
import ctypes
import importlib

import numpy as np
import pytest

from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = ctypes.c_void_p(16)                           # (never dereferenced: the arguments are refused first)
BIG = 1 << 40
NO_EOS = _lib.SHAPE_NO_EOS

# per entry point: its parameters in ABI order (shape ... stream); `meta` stands for the five (or, `meta4`, four: no kp) host arrays
_TABLES = ('elp', 'trans', 'init', 'len_scores', 'endpen')
_SIDE_P = tuple(n + '_p' for n in _TABLES) + ('logz_p', 'ws_p', 'ws_p_bytes')
_SIDE_Q = tuple(n + '_q' for n in _TABLES) + ('logz_q', 'ws_q', 'ws_q_bytes')
_GRADS = ('g_elp', 'g_trans', 'g_init', 'g_len')
_WS = ('ws', 'ws_bytes', 'stream')
SIGNATURES = {
    'smm_emission_f64': ('meta4', 'x', 'w', 'cst', 'inv_var', 'cons', 'elp64', 'elp32') + _WS,
    'smm_emission_bwd_f64': ('meta4', 'x', 'g_elp', 'g_w', 'g_cst', 'g_inv_var') + _WS,
    'smm_viterbi_f64': ('meta',) + _TABLES + ('class_map', 'spans', 'labels', 'best', 'n_segs') + _WS,
    'smm_viterbi_f32': ('meta',) + _TABLES + ('class_map', 'spans', 'labels', 'best', 'n_segs') + _WS,
    'smm_decode_f32': ('meta', 'x', 'w', 'cst', 'inv_var', 'cons', 'trans', 'init', 'len_scores', 'endpen', 'class_map', 'spans',
                       'labels', 'best', 'n_segs', 'elp32') + _WS,
    'smm_logz_f64': ('meta',) + _TABLES + ('logz',) + _WS,
    'smm_logz_bwd_f64': ('meta',) + _TABLES + ('logz', 'grad_logz') + _GRADS + _WS,
    'smm_sample_f64': ('meta',) + _TABLES + ('class_map', 'logz', 'n_samples', 'seed', 'spans', 'labels', 'logp') + _WS,
    'smm_entropy_f64': ('meta',) + _TABLES + ('logz', 'entropy_out') + _WS,
    'smm_kl_f64': ('meta',) + _SIDE_P + _SIDE_Q + ('kl_out', 'xent_out', 'stream'),
    'smm_entropy_bwd_f64': ('meta',) + _TABLES + ('logz', 'grad_out') + _GRADS + ('value_out', 'scratch', 'scratch_bytes') + _WS,
    'smm_kl_bwd_f64': ('meta',) + _SIDE_P + _SIDE_Q + ('mode', 'grad_out') + _GRADS + ('value_out', 'scratch', 'scratch_bytes',
                                                                                    'stream'),
    'smm_kbest_f64': ('meta',) + _TABLES + ('class_map', 'k', 'spans', 'labels', 'score', 'n_segs') + _WS,
    'smm_mbr_f64': ('meta', 'gain', 'trans', 'init', 'endpen', 'class_map', 'spans', 'labels', 'best', 'gain_sum', 'n_segs') + _WS,
    'smm_align_f64': ('meta',) + _TABLES + ('class_map', 'transcript', 'toff', 'spans', 'labels', 'best', 'n_segs') + _WS,
    'smm_dense_dp_f32': ('scores', 'dlengths', 'db', 'n1', 'dk', 'dc', 'semiring', 'v', 'dspans', 'dws', 'dws_bytes', 'stream'),
    'smm_dense_marginals_f32': ('scores', 'dlengths', 'db', 'n1', 'dk', 'dc', 'v', 'grad_v', 'marginals', 'dws', 'dws_bytes',
                                'stream'),
}
NULL_BY_DEFAULT = ('endpen', 'endpen_p', 'endpen_q', 'class_map', 'cons', 'grad_logz', 'grad_out', 'grad_v', 'value_out',
                   'xent_out', 'stream')
INTS = dict(n_samples=ctypes.c_int32, seed=ctypes.c_uint64, k=ctypes.c_int32, mode=ctypes.c_int32, db=ctypes.c_int32,
            n1=ctypes.c_int32, dk=ctypes.c_int32, dc=ctypes.c_int32, semiring=ctypes.c_int32)
INT_DEFAULTS = dict(n_samples=2, seed=1, k=4, mode=1, db=2, n1=5, dk=4, dc=3, semiring=0)


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def call(fn, **fault):
    """The valid call of `fn` on one video of 6 frames, 3 states, 4 length rows -- with the given slots replaced.  Slots: the
    parameter names of SIGNATURES; `shape` (keyword arguments of the smm_shape, or None), `lengths`, `frame_off`, `group`, `kp`,
    `n_states` (host arrays, or None)."""
    host = dict(lengths=np.array([6], np.int64), frame_off=np.array([0], np.int64), group=None, kp=None,
                n_states=np.array([3], np.int32), toff=np.array([0, 2], np.int64), dlengths=np.array([6, 3], np.int64))
    sk = dict(b=1, d=4, n_groups=1, c_max=3, k_rows=4, t_max=6, flags=0, total_frames=6)
    shape_fault = fault.pop('shape', {})
    shape = None
    if shape_fault is not None:
        sk.update(shape_fault)
        shape = _lib.SmmShape(*[sk[f] for f in ('b', 'd', 'n_groups', 'c_max', 'k_rows', 't_max', 'flags', 'total_frames')])
    for name in list(fault):
        if name in host:
            host[name] = fault.pop(name)
    args = []
    for name in SIGNATURES[fn]:
        if name in ('meta', 'meta4'):
            args.append(None if shape is None else ctypes.byref(shape))
            args += [_ptr(host[n]) for n in ('lengths', 'frame_off', 'group') + (('kp',) if name == 'meta' else ()) + ('n_states',)]
        elif name in ('toff', 'dlengths'):
            args.append(_ptr(host[name]))
        elif name in INTS:
            args.append(INTS[name](fault.pop(name, INT_DEFAULTS[name])))
        elif name.endswith('_bytes'):
            args.append(ctypes.c_size_t(fault.pop(name, BIG)))
        else:
            args.append(fault.pop(name, None if name in NULL_BY_DEFAULT else P))
    assert not fault, "unknown slots: %s" % sorted(fault)
    return getattr(_lib.load(), fn)(*args)


def _bytes(query, *extra, **shape):
    sk = dict(b=1, d=4, n_groups=1, c_max=3, k_rows=4, t_max=6, flags=0, total_frames=6)
    sk.update(shape)
    s = _lib.SmmShape(*[sk[f] for f in ('b', 'd', 'n_groups', 'c_max', 'k_rows', 't_max', 'flags', 'total_frames')])
    lengths = np.array([6], np.int64)
    fn = getattr(_lib.load(), query)
    fn.restype = ctypes.c_size_t
    n = fn(ctypes.byref(s), _ptr(lengths), *extra)
    assert n > 0
    return n


def _rows():
    rows = []

    def add(fn, status, **fault):
        rows.append(pytest.param(fn, status, fault, id="%d-%s-%s" % (len(rows), fn[4:], "-".join(sorted(fault)))))

    # what stage() refuses before it asks the runtime anything: every entry point that takes a shape
    for fn, sig in SIGNATURES.items():
        if sig[0] not in ('meta', 'meta4') or fn in ('smm_align_f64', 'smm_mbr_f64'):     # (those two: COVERED, their own checks)
            continue
        add(fn, ARG, shape=None)
        add(fn, ARG, shape=dict(b=0))
        add(fn, ARG, shape=dict(k_rows=1))
        for slot in ('lengths', 'frame_off', 'n_states'):
            add(fn, ARG, **{slot: None})
        add(fn, ARG, **{'ws_p' if 'ws_p' in sig else 'ws': None})
    # the emission gradient: its pointers and d, in front of staging
    for slot in ('x', 'g_elp', 'g_w', 'g_cst', 'g_inv_var'):
        add('smm_emission_bwd_f64', ARG, **{slot: None})
    add('smm_emission_bwd_f64', ARG, shape=dict(d=0))
    # entropy: each table by itself (COVERED has trans and len_scores together)
    for slot in ('elp', 'trans', 'init', 'len_scores'):
        add('smm_entropy_f64', ARG, **{slot: None})
    # KL and its gradient: each table and log Z of each side by itself; q's workspace is checked against the plan first
    for fn in ('smm_kl_f64', 'smm_kl_bwd_f64'):
        for side in 'pq':
            for slot in ('elp', 'trans', 'init', 'len_scores', 'logz'):
                add(fn, ARG, **{slot + '_' + side: None})
        add(fn, ARG, lengths=np.array([0], np.int64))
        add(fn, ARG, lengths=np.array([7], np.int64))
    # the gradients: each table by itself, the scratch query's refusals (it knows the kernels' limits: ARG, not UNSUPPORTED)
    for slot in ('elp', 'trans', 'init', 'len_scores'):
        add('smm_entropy_bwd_f64', ARG, **{slot: None})
    for fn in ('smm_entropy_bwd_f64', 'smm_kl_bwd_f64'):
        add(fn, ARG, shape=dict(c_max=33))
        add(fn, ARG, shape=dict(k_rows=1025))
    add('smm_entropy_bwd_f64', ARG, lengths=np.array([0], np.int64))
    # k best: limits, lengths, the workspace pointer (k, the outputs and a short workspace: COVERED)
    add('smm_kbest_f64', UNSUPPORTED, shape=dict(c_max=33))
    add('smm_kbest_f64', UNSUPPORTED, shape=dict(k_rows=1025))
    add('smm_kbest_f64', ARG, lengths=np.array([0], np.int64))
    add('smm_kbest_f64', ARG, lengths=np.array([7], np.int64))
    add('smm_kbest_f64', WORKSPACE, ws_bytes=_bytes('smm_kbest_workspace_bytes', ctypes.c_int32(4)) - 1)
    # MBR and align: what COVERED leaves
    add('smm_mbr_f64', ARG, shape=None)
    for slot in ('lengths', 'frame_off', 'n_states'):
        add('smm_mbr_f64', ARG, **{slot: None})
    add('smm_mbr_f64', ARG, lengths=np.array([0], np.int64))
    add('smm_mbr_f64', ARG, lengths=np.array([7], np.int64))
    add('smm_align_f64', ARG, shape=None)
    add('smm_align_f64', ARG, lengths=np.array([0], np.int64))
    add('smm_align_f64', ARG, lengths=np.array([7], np.int64))
    add('smm_align_f64', ARG, toff=np.array([-1, 1], np.int64))
    # dense boundary DP
    for fn, outs in (('smm_dense_dp_f32', ('v',)), ('smm_dense_marginals_f32', ('v', 'marginals'))):
        for slot in ('scores', 'dlengths', 'dws') + outs:
            add(fn, ARG, **{slot: None})
        for slot in ('db', 'n1', 'dk', 'dc'):
            add(fn, ARG, **{slot: 0})
        add(fn, UNSUPPORTED, dc=256)
        add(fn, UNSUPPORTED, dk=65536)
        add(fn, ARG, dlengths=np.array([6, 0], np.int64))
        add(fn, ARG, dlengths=np.array([6, 7], np.int64))          # more than n1 + 1 boundaries
        add(fn, WORKSPACE, dws_bytes=_lib.load().smm_dense_workspace_bytes(2, 5, 4, 3) - 1)
    return rows


@pytest.mark.parametrize("fn,status,fault", _rows())
def test_single_fault_is_refused(fn, status, fault):
    assert call(fn, **fault) == status


# rows asserted elsewhere: entry point -> (test module, test, the faults it covers)
COVERED = {
    'smm_sample_f64': [('test_sample_host', 'test_sample_refuses_no_outputs_and_non_positive_counts', 'n_samples <= 0; every output NULL')],
    'smm_entropy_f64': [('test_entropy_host', 'test_entropy_refuses_null_output_and_tables', 'NULL entropy_out, logz')],
    'smm_kl_f64': [('test_kl_host', 'test_kl_refuses_null_output_and_tables', 'NULL kl_out, ws_q'),
                   ('test_kl_host', 'test_kl_refuses_a_short_workspace_of_q_before_staging', 'ws_q one byte short')],
    'smm_entropy_bwd_f64': [('test_entropy_grad_host', 'test_entropy_bwd_refuses_null_arguments', 'NULL logz, scratch, each output'),
                            ('test_entropy_grad_host', 'test_entropy_bwd_refuses_a_short_scratch', 'scratch one byte short')],
    'smm_kl_bwd_f64': [('test_entropy_grad_host', 'test_kl_bwd_refuses_bad_mode_and_null_arguments',
                        'mode; NULL ws_q, scratch, each output'),
                       ('test_entropy_grad_host', 'test_kl_bwd_refuses_short_buffers', 'ws_q, scratch one byte short')],
    'smm_kbest_f64': [('test_kbest_host', 'test_kbest_refuses_bad_k_and_no_outputs', 'k 0, 17, -2; every output NULL'),
                      ('test_kbest_host', 'test_kbest_refuses_a_small_workspace', 'workspace one byte short')],
    'smm_mbr_f64': [('test_mbr_host', 'test_mbr_refuses_null_inputs_and_outputs', 'NULL gain, trans, init, ws; outputs; b = 0'),
                    ('test_mbr_host', 'test_mbr_refuses_unsupported_shapes', 'c_max 33, k_rows 1025'),
                    ('test_mbr_host', 'test_mbr_refuses_a_short_workspace_before_staging', 'workspace one byte short')],
    'smm_align_f64': [('test_align_host', 'test_align_refuses_bad_arguments_before_staging',
                       'every NULL pointer; outputs; b = 0; empty and non-monotone transcripts'),
                      ('test_align_host', 'test_align_refuses_unsupported_shapes_before_staging',
                       'NO_EOS, c_max 33, k_rows 1025, 257 entries'),
                      ('test_align_host', 'test_align_refuses_a_short_workspace_before_staging', 'workspace one byte short')],
}


def test_the_referenced_rows_exist():
    for fn, refs in COVERED.items():
        assert fn in SIGNATURES
        for module, test, _ in refs:
            assert callable(getattr(importlib.import_module(module), test)), (module, test)
