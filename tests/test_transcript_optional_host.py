"""Host-side checks of the transcript likelihood with optional entries: the three references of
tests/transcript_optional_ref.py against each other, the header's identities, the ambiguity predicate against enumeration, the
C entry points' refusals (no GPU: every call is refused before anything is staged) and the Python-level argument checks."""
import ctypes
import types

import numpy as np
import pytest
import torch

import align_optional_ref as AO
import transcript_optional_ref as TO
import transcript_ref as TR
from action_segmentation_amd import _lib

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
POISON = ctypes.c_void_p(0xdead0000)              # (never dereferenced: the arguments are refused first)
DENSITIES = (0.0, 0.3, 0.6, 1.0)


def _case(rng, i, with_holes=False):
    """A random tiny video with an alignment by counting: T <= 7, M <= 5, kp <= 5, C <= 3."""
    while True:
        T, C, M, kp = int(rng.integers(1, 8)), int(rng.integers(1, 4)), int(rng.integers(1, 6)), int(rng.integers(2, 6))
        opt = [bool(v) for v in rng.random(M) < DENSITIES[i % 4]]
        if AO.feasible_by_count(T, opt, kp):
            break
    c = dict(elp=rng.normal(size=(T, C)) * 2, a=[int(v) for v in rng.integers(0, C, size=M)], opt=opt,
             trans=rng.normal(size=(C, C)) * 2, init=rng.normal(size=C) * 2, len_scores=rng.normal(size=(kp + i % 2, C)) * 2, kp=kp,
             endpen=rng.normal(size=C) if i % 3 == 0 else None)
    if with_holes:
        c['trans'][int(rng.integers(0, C)), int(rng.integers(0, C))] = -np.inf
        c['len_scores'][int(rng.integers(1, kp)), int(rng.integers(0, C))] = -np.inf
    return c


@pytest.fixture(scope='module')
def tiny_cases():
    """400 random tiny cases with each route's answer, computed once."""
    rng = np.random.default_rng(20261019)
    out = []
    for i in range(400):
        c = _case(rng, i)
        out.append((c, TO.brute_logz_opt(**c), TO.torch_grads_opt(**c), TO.twin_grads_opt(**c), TO.forward_backward(**c)))
    return out


def test_the_three_references_agree(tiny_cases):
    worst, n = 0.0, 0
    for c, (zb, occ, pu), (zt, gt), (zw, gw), fb in tiny_cases:
        assert np.isfinite(zb), c                                            # (finite tables: a path by counting has a score)
        errs = [abs(zb - zt), abs(zb - zw), abs(zb - fb['logz']), np.abs(gt['elp'] - occ).max(), np.abs(gw['p_used'] - pu).max()]
        errs += [np.abs(gt[k] - gw[k]).max() for k in ('elp', 'trans', 'init', 'len')]
        worst = max(worst, max(errs))
        n += 1
    assert n == 400 and worst <= 1e-9, worst


def test_identity_and_entry_posteriors(tiny_cases):
    """lse_first(h[0] + bh[0]) = logZ_o; p_used from S and from E agree with the enumeration; 1 on mandatory entries; occ from
    S and E is the enumeration's frame occupancy; g_init is the start posterior."""
    n_opt = 0
    for c, (zb, occ, pu), (zt, gt), _, fb in tiny_cases:
        assert abs(fb['ident'] - fb['logz']) <= 1e-9
        assert np.abs(fb['p_used'] - pu).max() <= 1e-9 and np.abs(fb['p_used_S'] - pu).max() <= 1e-9
        mand = ~np.asarray(c['opt'], bool)
        assert np.abs(fb['p_used'][mand] - 1.0).max(initial=0.0) <= 1e-9
        assert fb['p_used'].min() >= -1e-12 and fb['p_used'].max() <= 1.0 + 1e-9
        n_opt += int((~mand).sum())
        by_class = np.zeros_like(occ)
        for m, cls in enumerate(c['a']):
            by_class[:, cls] += fb['occ'][:, m]
        assert np.abs(by_class - occ).max() <= 1e-9
        _, first, _, _ = AO.structure(c['opt'])
        gi = np.zeros(len(c['init']))
        for m, cls in enumerate(c['a']):
            if first[m]:
                gi[cls] += fb['S'][0, m]
        assert np.abs(gi - gt['init']).max() <= 1e-9 and abs(gi.sum() - 1.0) <= 1e-9
    assert n_opt > 300


def test_minus_infinity_tables_torch_against_enumeration():
    """-inf table entries kill some alignments or all of them: the torch route and the forward-backward know -inf."""
    rng = np.random.default_rng(8)
    n_fin = n_inf = 0
    for i in range(200):
        c = _case(rng, i, with_holes=True)
        zb, occ, pu = TO.brute_logz_opt(**c)
        zt, gt = TO.torch_grads_opt(**c)
        fb = TO.forward_backward(**c)
        assert np.isfinite(zb) == np.isfinite(zt) == np.isfinite(fb['logz'])
        if np.isfinite(zb):
            assert abs(zb - zt) <= 1e-9 and abs(zb - fb['logz']) <= 1e-9
            assert np.abs(gt['elp'] - occ).max() <= 1e-9 and np.abs(fb['p_used'] - pu).max() <= 1e-9
            n_fin += 1
        else:
            assert all(not v.any() for v in gt.values())
            n_inf += 1
    assert n_fin > 50 and n_inf > 5


def test_no_flag_is_the_exact_transcript_likelihood():
    rng = np.random.default_rng(4)
    for i in range(40):
        c = _case(rng, 0)
        assert not any(c['opt'])
        closing = 0.0 if c['endpen'] is None else float(c['endpen'][c['a'][-1]])
        z, g = TO.torch_grads_opt(**c)
        zr, gr = TR.torch_grads(c['elp'], c['a'], c['trans'], c['init'], c['len_scores'], c['kp'], closing)
        assert abs(z - zr) <= 1e-12 * max(1.0, abs(zr))
        assert all(np.abs(g[k] - gr[k]).max() <= 1e-12 for k in g)


# ------------------------------------------------------------------------------------------------ ambiguity
def test_transcript_is_ambiguous_against_enumeration():
    from action_segmentation_amd import ops
    rng = np.random.default_rng(99)
    n_amb = 0
    for i in range(6000):
        M, C = int(rng.integers(1, 10)), int(rng.integers(1, 4))
        a = rng.integers(0, C, size=M)
        opt = rng.random(M) < DENSITIES[1 + i % 3]
        want = TO.is_ambiguous_brute(a, opt)
        assert ops.transcript_is_ambiguous(a, opt) == want, (a, opt)
        n_amb += want
    assert 1000 < n_amb < 5000
    assert ops.transcript_is_ambiguous([0, 1, 0], [1, 1, 1]) and not ops.transcript_is_ambiguous([0, 1, 0], [1, 0, 1])
    assert not ops.transcript_is_ambiguous([0, 1, 0], [0, 0, 0]) and not ops.transcript_is_ambiguous([2], [1])
    assert ops.transcript_is_ambiguous(torch.tensor([1, 1]), torch.tensor([True, True]))
    with pytest.raises(ValueError):
        ops.transcript_is_ambiguous([0, 1], [1])


def test_the_crosstask_forms():
    """bg, step_1, bg, ..., step_S, bg: unambiguous with only the backgrounds optional and with only the steps optional,
    ambiguous with everything optional."""
    from action_segmentation_amd import ops
    for steps in ([1], [1, 2], [1, 2, 3, 4], [3, 1, 3, 2]):
        for bg_opt, step_opt, want in ((True, False, False), (False, True, False), (True, True, True)):
            a, f = TO.crosstask(steps, 0, bg_opt, step_opt)
            assert TO.is_ambiguous_brute(a, f) == want and ops.transcript_is_ambiguous(a, f) == want, (steps, bg_opt, step_opt)


def test_unambiguous_logz_is_the_lse_over_the_reduced_transcripts():
    rng = np.random.default_rng(17)
    n = 0
    while n < 60:
        c = _case(rng, 1 + n % 3)
        if TO.is_ambiguous_brute(c['a'], c['opt']):
            continue
        z = float(TO.torch_logz_opt(*[torch.tensor(c[k]) if isinstance(c[k], np.ndarray) else c[k]
                                       for k in ('elp', 'a', 'opt', 'trans', 'init', 'len_scores', 'kp')],
                                    None if c['endpen'] is None else torch.tensor(c['endpen'])))
        parts = []
        for red in TO.reduced_transcripts(c['a'], c['opt']):
            closing = 0.0 if c['endpen'] is None else float(c['endpen'][red[-1]])
            parts.append(float(TR.torch_logz(torch.tensor(c['elp']), red, torch.tensor(c['trans']), torch.tensor(c['init']),
                                             torch.tensor(c['len_scores']), c['kp'], closing)))
        parts = np.array(parts)
        parts = parts[np.isfinite(parts)]
        want = parts.max() + np.log(np.exp(parts - parts.max()).sum())
        assert abs(z - want) <= 1e-9 * max(1.0, abs(want))
        n += 1


# ------------------------------------------------------------------------------------------------ the C entry points
def _shape(b=1, c=3, k_rows=4, t_max=6, flags=0, total=None):
    return _lib.SmmShape(b, 0, 1, c, k_rows, t_max, flags, total if total is not None else b * t_max)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _ws(lengths, ms, entry='smm_align_opt_logz_workspace_bytes', **kw):
    lengths = np.asarray(lengths, np.int64)
    off = np.concatenate([[0], np.cumsum(ms)]).astype(np.int64)
    kw.setdefault('total', int(lengths.max()) * len(lengths))
    shape = _shape(b=len(lengths), t_max=int(lengths.max()), **kw)
    return getattr(_lib.load(), entry)(ctypes.byref(shape), _p(lengths), _p(off))


_UNSET = object()


def _call(bwd=False, shape=None, off=_UNSET, elp=POISON, trans=POISON, init=POISON, len_scores=POISON, transcript=POISON,
          optional=POISON, logz=POISON, g_elp=POISON, g_trans=POISON, g_init=POISON, g_len=POISON, p_used=None, ws=POISON,
          ws_bytes=1 << 40, lengths=_UNSET, n_states=_UNSET, frame_off=_UNSET):
    lib = _lib.load()
    lengths = np.array([6], np.int64) if lengths is _UNSET else lengths
    frame_off = np.array([0], np.int64) if frame_off is _UNSET else frame_off
    n_states = np.array([3], np.int32) if n_states is _UNSET else n_states
    off = np.array([0, 2], np.int64) if off is _UNSET else off
    shape = shape or _shape()
    head = (ctypes.byref(shape), _p(lengths), _p(frame_off), None, None, _p(n_states), elp, trans, init, len_scores, None,
            transcript, optional, _p(off), logz)
    if not bwd:
        return lib.smm_align_opt_logz_f64(*head, ws, ctypes.c_size_t(ws_bytes), POISON)
    return lib.smm_align_opt_logz_bwd_f64(*head, None, g_elp, g_trans, g_init, g_len, p_used, ws, ctypes.c_size_t(ws_bytes), POISON)


def test_the_new_symbols_are_exported():
    lib = _lib.load()
    for name in ('smm_align_opt_logz_workspace_bytes', 'smm_align_opt_logz_f64', 'smm_align_opt_logz_bwd_f64'):
        assert name in _lib.SYMBOLS
        assert getattr(lib, name) is not None


@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
def test_refuses_bad_arguments_before_staging(bwd):
    names = ['elp', 'trans', 'init', 'len_scores', 'transcript', 'optional', 'logz', 'ws', 'off', 'lengths', 'n_states', 'frame_off']
    if bwd:
        names += ['g_elp', 'g_trans', 'g_init', 'g_len']
    for name in names:
        assert _call(bwd, **{name: None}) == ARG, name
    assert _call(bwd, ws_bytes=0) == WORKSPACE                          # (p_used and grad_logz may be NULL)
    assert _call(bwd, shape=_shape(b=0)) == ARG
    assert _call(bwd, off=np.array([0, 0], np.int64)) == ARG            # M = 0
    assert _call(bwd, off=np.array([2, 1], np.int64)) == ARG            # non-monotone
    two = dict(shape=_shape(b=2), lengths=np.array([6, 6], np.int64), frame_off=np.array([0, 6], np.int64))
    assert _call(bwd, off=np.array([0, 3, 2], np.int64), **two) == ARG
    assert _call(bwd, off=np.array([0, 3, 5], np.int64), ws_bytes=0, **two) == WORKSPACE


@pytest.mark.parametrize('bwd', [False, True], ids=['fwd', 'bwd'])
def test_refuses_unsupported_shapes_and_short_workspaces_before_staging(bwd):
    assert _call(bwd, shape=_shape(flags=_lib.SHAPE_NO_EOS)) == UNSUPPORTED
    assert _call(bwd, shape=_shape(c=33)) == UNSUPPORTED
    assert _call(bwd, shape=_shape(k_rows=1025)) == UNSUPPORTED
    assert _call(bwd, off=np.array([0, 257], np.int64)) == UNSUPPORTED
    assert _call(bwd, off=np.array([0, 256], np.int64), ws_bytes=0) == WORKSPACE
    need = _ws([6], [2])
    assert need > 0 and _call(bwd, ws_bytes=need - 1) == WORKSPACE
    assert _call(bwd, ws_bytes=_ws([6], [2], entry='smm_align_logz_workspace_bytes')) == WORKSPACE   # (the exact one's is too small)


def test_workspace_bytes():
    lib = _lib.load()
    exact = lambda lengths, ms, **kw: _ws(lengths, ms, entry='smm_align_logz_workspace_bytes', **kw)
    # a fourth column per entry and c_max columns of running sums per video
    assert _ws([6], [2]) >= exact([6], [2]) + 8 * (2 + 3) * 7
    assert _ws([6, 60], [2, 3], c=5) >= exact([6, 60], [2, 3], c=5) + 8 * ((2 + 5) * 7 + (3 + 5) * 61)
    assert _ws([6], [1]) > exact([6], [1]) and _ws([600], [256]) > exact([600], [256])
    assert _ws([6], [1]) < _ws([6], [2]) < _ws([6], [6]) < _ws([6], [256])
    assert _ws([6], [3]) < _ws([7], [3]) < _ws([60], [3]) < _ws([600], [3])
    # 0 on bad arguments
    assert _ws([6], [0]) == 0 and _ws([6], [257]) == 0 and _ws([0], [1]) == 0
    assert _ws([6], [2], flags=_lib.SHAPE_NO_EOS) == 0
    assert _ws([6], [2], c=33) == 0 and _ws([6], [2], k_rows=1025) == 0 and _ws([6], [2], k_rows=1) == 0
    lengths, off = np.array([6], np.int64), np.array([0, 2], np.int64)
    assert lib.smm_align_opt_logz_workspace_bytes(ctypes.byref(_shape(t_max=4)), _p(lengths), _p(off)) == 0   # longer than t_max
    assert lib.smm_align_opt_logz_workspace_bytes(ctypes.byref(_shape()), None, _p(off)) == 0
    assert lib.smm_align_opt_logz_workspace_bytes(ctypes.byref(_shape()), _p(lengths), None) == 0
    assert lib.smm_align_opt_logz_workspace_bytes(None, _p(lengths), _p(off)) == 0


# ------------------------------------------------------------------------------------------------ Python-level argument checks
def test_ops_value_errors_before_a_device_is_touched():
    from action_segmentation_amd import ops
    batch = ops.Batch([6, 5], [3], 4)
    _, off = ops._transcript_arrays(batch, [[0, 1], [2, 2, 1]])
    assert ops.align_opt_logz_workspace_bytes(batch, off) > ops.align_logz_workspace_bytes(batch, off)
    with pytest.raises(ValueError):
        ops.align_opt_logz_workspace_bytes(batch, off[:-1])
    z = torch.zeros(1, dtype=torch.float64)                                     # (a CPU tensor: no call gets as far as using it)
    ids = [[0, 1], [2, 2, 1]]
    for flags in ([[True, False]], [[True, False], [True]], None):
        with pytest.raises(ValueError):
            ops.align_opt_logz(batch, z, z, z, z, ids, flags)
        with pytest.raises(ValueError):
            ops.align_opt_logz_bwd(batch, z, z, z, z, ids, flags, z, ws=z)
    with pytest.raises(ValueError):
        ops.align_opt_logz(batch, z, z, z, z, [[0, 1]], [[True, False]])        # one transcript short
    with pytest.raises(ValueError):
        ops.align_opt_logz(batch, z, z, z, z, [[0, 1], []], [[True, False], []])   # an empty transcript


def test_module_checks_fire_before_a_device_is_touched():
    """The flags' shape and ambiguous='raise' are host arithmetic: a corpus whose features sit on the CPU gets as far as them
    and no further (the next check would refuse the CPU tensor with another message)."""
    from module_util import make_args
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    m = SemiMarkovModule(make_args(6), 4, 3, allow_self_transitions=True)
    pc = types.SimpleNamespace(video_names=['v0', 'v1'], batch=None, x=torch.zeros(1))
    tr = [[0, 1, 0], [2, 3]]
    for fn in (m.transcript_log_partition_packed, m.transcript_scores_packed):
        with pytest.raises(ValueError, match="'v0'"):
            fn(pc, tr, optional=[[1, 1, 1], [0, 1]])                            # [x?, y?, x?]
        with pytest.raises(ValueError, match="flags"):
            fn(pc, tr, optional=[[1, 1], [0, 1]])
        with pytest.raises(ValueError, match="ambiguous"):
            fn(pc, tr, optional=[[0, 1, 0], [0, 1]], ambiguous='maybe')
    with pytest.raises(ValueError, match="'v0'"):
        m.transcript_entry_posteriors_packed(pc, tr, [[1, 1, 1], [0, 1]])
    with pytest.raises(ValueError):
        m.transcript_entry_posteriors_packed(pc, tr, None)
    x = torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="video 0"):
        m.transcript_log_partition(x, torch.tensor([5, 5]), None, tr, optional=[[1, 1, 1], [0, 1]])
    with pytest.raises(ValueError, match="transcript_optional"):
        m.log_likelihood(x, torch.tensor([5, 5]), None, transcript_optional=[[0, 1, 0], [0, 1]])


def test_model_refuses_both_kinds_of_flags_and_ambiguous_transcripts():
    from action_segmentation_amd import synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    data = synth.SynthDatasplit('tiny', seed=11)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    for fn in (model.transcript_log_likelihood, model.transcript_entry_posteriors):
        with pytest.raises(ValueError, match="not both"):
            fn(data, {}, optional_by_video={}, optional_classes=[0])
        with pytest.raises(ValueError, match="'clip'"):
            fn(data, {'clip': [0, 1, 0]}, optional_classes=[0, 1])
        with pytest.raises(ValueError, match="'clip'"):
            fn(data, {'clip': [0, 1, 0]}, optional_by_video={'clip': [1, 1, 1]})
    with pytest.raises(ValueError):
        model.transcript_entry_posteriors(data, {})
