"""The expected-reward entry points (smm_expected_reward_f64 / smm_expected_reward_bwd_f64) without a GPU: the two statements of
the torch reference agree on the enumerable lattices, the scratch query, and every refusal that returns before a HIP call (the
pattern of tests/test_api_refusals_host.py: device pointers are a poison value that is never dereferenced)."""
import ctypes

import numpy as np
import pytest

import expected_reward_ref as E
from action_segmentation_amd import _lib
from entropy_grad_cases import SMALL, _small_case

P = ctypes.c_void_p(16)                           # (never dereferenced: the arguments are refused first)
ARG, WORKSPACE = -1, -3
BIG = 1 << 40


# ------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize('setting', E.SETTINGS)
@pytest.mark.parametrize('k,add_eos,masked,additional,narration', SMALL)
def test_enumeration_and_polynomial_reference_agree(k, add_eos, masked, additional, narration, setting):
    """(a) and (b) of tests/expected_reward_ref.py on every enumerable lattice: value, both parts and all four tables to 1e-9."""
    (elp, lengths, trans, init, lens, ep), _ = _small_case(k, add_eos, masked, additional, narration, 'draw')
    b, tmax, c = elp.shape
    reward, seg = E.small_rewards(1000 + k, b, tmax, c, setting)
    kp, up = min(k, max(lengths)), np.array([1.0, -0.5, 2.0])
    va, pa, ga = E.batch_reference(E.video_enumeration, elp, lengths, trans, init, lens, kp, not add_eos, ep, reward, seg, up)
    vb, pb, gb = E.batch_reference(E.video_polynomial, elp, lengths, trans, init, lens, kp, not add_eos, ep, reward, seg, up)
    np.testing.assert_allclose(va, vb, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(pa, pb, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(pa.sum(1), va, rtol=1e-12, atol=1e-12)
    if setting == 'reward':
        assert (pa[:, 1] == 0.0).all()
    if setting == 'seg_reward':
        assert (pa[:, 0] == 0.0).all()
    for name in E.NAMES:
        np.testing.assert_allclose(ga[name].numpy(), gb[name].numpy(), rtol=1e-9, atol=1e-9, err_msg=name)
    assert max(float(ga[name].abs().max()) for name in E.NAMES) > 1e-3          # (not a degenerate case)


def test_reference_closed_forms():
    """reward = 1 for every class: V is the frame count and the gradient 0; seg_reward = 1: V is the expected number of spans,
    sum of d log Z / d len (+ 1 for the closing label without EOS)."""
    import entropy_grad_dp_ref as D
    for k, add_eos in ((4, True), (3, False)):
        (elp, lengths, trans, init, lens, ep), _ = _small_case(k, add_eos, True, False, True, 'draw')
        kp = min(k, max(lengths))
        for i, fr in enumerate(lengths):
            t = dict(elp=elp[i, :fr], trans=trans, init=init, len=lens)
            e = None if ep is None else ep[i]
            v, vf, vs, g = E.video_enumeration(t, np.ones((fr, 3)), None, kp, not add_eos, e)
            assert abs(v - fr) <= 1e-12 and vs == 0.0
            assert max(float(g[n].abs().max()) for n in E.NAMES) <= 1e-12
            v, vf, vs, g = E.video_polynomial(t, None, np.ones(3), kp, not add_eos, e)
            want = float(D.length_marginals(t, kp, not add_eos, e).sum()) + (0 if add_eos else 1)
            assert abs(v - want) <= 1e-10 and vf == 0.0


# ------------------------------------------------------------------------------------------------------- the C ABI
def _shape(lengths, c=3, k_rows=4, flags=0):
    return _lib.SmmShape(len(lengths), 0, 1, c, k_rows, int(max(lengths)), flags, int(sum(lengths)))


def _scratch_bytes(shape, lengths):
    return _lib.load().smm_expected_reward_bwd_scratch_bytes(ctypes.byref(shape),
                                                             None if lengths is None else ctypes.c_void_p(lengths.ctypes.data))


_VALUE_SLOTS = ('elp', 'trans', 'init', 'len_scores', 'endpen', 'logz', 'reward', 'seg_reward', 'value_out', 'parts_out')
_BWD_SLOTS = ('elp', 'trans', 'init', 'len_scores', 'endpen', 'logz', 'reward', 'seg_reward', 'grad_out', 'g_elp', 'g_trans',
              'g_init', 'g_len', 'value_out')
_NULL_BY_DEFAULT = ('endpen', 'parts_out', 'grad_out')


def _call(fn, lengths=np.array([6], np.int64), scratch=P, scratch_bytes=BIG, ws=P, ws_bytes=BIG, shape=None, null_shape=False,
          **fault):
    """The valid call on one video of 6 frames, 3 states, 4 length rows, with the given slots replaced."""
    shape = _shape(lengths) if shape is None else shape
    bwd = fn == 'smm_expected_reward_bwd_f64'
    slots = _BWD_SLOTS if bwd else _VALUE_SLOTS
    null = _NULL_BY_DEFAULT + (('value_out',) if bwd else ())
    args = [fault.pop(n, None if n in null else P) for n in slots]
    assert not fault, sorted(fault)
    tail = ([scratch, ctypes.c_size_t(scratch_bytes)] if bwd else []) + [ws, ctypes.c_size_t(ws_bytes), None]
    return getattr(_lib.load(), fn)(None if null_shape else ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data), None, None,
                                    None, None, *args, *tail)


def test_symbols_are_exported():
    lib = _lib.load()
    for name in ('smm_expected_reward_bwd_scratch_bytes', 'smm_expected_reward_f64', 'smm_expected_reward_bwd_f64'):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None


def test_scratch_query_grows_with_the_batch_and_is_zero_on_bad_arguments():
    c, k_rows = 3, 4
    lengths = np.array([6, 4, 9], np.int64)
    base = _scratch_bytes(_shape(lengths, c, k_rows), lengths)
    assert base > 0 and base % 8 == 0
    longer = lengths.copy()
    longer[1] += 1
    assert _scratch_bytes(_shape(longer, c, k_rows), longer) > base                    # grows with T ...
    assert _scratch_bytes(_shape(lengths, c + 1, k_rows), lengths) > base              # ... and with c_max
    # enough for the four eta blocks, the occupancy differences and the per-video tables
    assert base >= 8 * (sum(5 * c * (int(t) + 1) for t in lengths) + len(lengths) * (k_rows * c + c * c + 2 * c + 2))
    # the workspace query does not change
    lib = _lib.load()
    assert lib.smm_workspace_bytes(ctypes.byref(_shape(lengths, c, k_rows)), ctypes.c_void_p(lengths.ctypes.data)) > 0
    # bad arguments: 0
    assert _scratch_bytes(_shape(lengths, 33, k_rows), lengths) == 0                   # c_max > SMM_MAX_STATES
    assert _scratch_bytes(_shape(lengths, c, 1025), lengths) == 0                      # k_rows > SMM_MAX_K_ROWS
    assert _scratch_bytes(_shape(lengths, c, k_rows), None) == 0
    bad = np.array([6, 0], np.int64)
    assert _scratch_bytes(_shape(bad, c, k_rows), bad) == 0
    assert lib.smm_expected_reward_bwd_scratch_bytes(None, ctypes.c_void_p(lengths.ctypes.data)) == 0


@pytest.mark.parametrize('slot', ['elp', 'trans', 'init', 'len_scores', 'logz', 'value_out'])
def test_value_call_refuses_a_null_argument(slot):
    assert _call('smm_expected_reward_f64', **{slot: None}) == ARG


@pytest.mark.parametrize('slot', ['elp', 'trans', 'init', 'len_scores', 'logz', 'g_elp', 'g_trans', 'g_init', 'g_len'])
def test_gradient_call_refuses_a_null_argument(slot):
    assert _call('smm_expected_reward_bwd_f64', **{slot: None}) == ARG


@pytest.mark.parametrize('fn', ['smm_expected_reward_f64', 'smm_expected_reward_bwd_f64'])
def test_both_rewards_null_is_refused(fn):
    assert _call(fn, reward=None, seg_reward=None) == ARG


@pytest.mark.parametrize('fn', ['smm_expected_reward_f64', 'smm_expected_reward_bwd_f64'])
def test_staging_refusals_come_before_any_hip_call(fn):
    lengths = np.array([6], np.int64)
    assert _call(fn, ws=None) == ARG
    assert _call(fn, null_shape=True) == ARG
    assert _call(fn, shape=_lib.SmmShape(0, 0, 1, 3, 4, 6, 0, 6)) == ARG               # b = 0
    assert _call(fn, shape=_shape(lengths, k_rows=1)) == ARG


def test_gradient_call_refuses_null_and_short_scratch():
    lengths = np.array([6], np.int64)
    assert _call('smm_expected_reward_bwd_f64', scratch=None) == ARG
    need = _scratch_bytes(_shape(lengths), lengths)
    assert need > 0
    assert _call('smm_expected_reward_bwd_f64', scratch_bytes=need - 1, lengths=lengths) == WORKSPACE
    # what the scratch query refuses is an argument error here too
    assert _call('smm_expected_reward_bwd_f64', shape=_shape(lengths, c=33)) == ARG
    assert _call('smm_expected_reward_bwd_f64', lengths=np.array([0], np.int64), shape=_shape(np.array([6]))) == ARG
