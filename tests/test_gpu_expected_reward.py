"""Expected frame- and segment-additive reward and its gradient (smm_expected_reward_f64 / smm_expected_reward_bwd_f64,
ops.expected_reward / ops.expected_reward_bwd) on the GPU.

References are tests/expected_reward_ref.py's: (a) torch fp64 autograd through sum_y p(y) R(y) over every segmentation of the
enumerable lattices, (b) a second autograd pass through d log Z / d theta . rho at the mid sizes that cross every work split of
csrc/smm_expected_reward.hip; at real sizes identities that need no reference (the symmetry of the Hessian of log Z, linearity,
constant rewards, the two decompositions, the MBR gain, the span-start and frame posteriors) and central differences of the
existing marginals.  Every seed is fixed."""
import functools

import numpy as np
import pytest
import torch

import entropy_grad_cases as C
import expected_reward_ref as E
from entropy_grad_cases import SMALL, _small_case
from test_gpu_entropy import _batch_tables
from test_gpu_entropy_grad import _close, _entries, _mid_launch, _padding_is_zero

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TABLES = ('elp', 'trans', 'init', 'len')
# The bar of every gradient here is the project's: |error| <= 1e-4 max(1, max |ref|) per table, the stated accuracy of the
# log-partition histories the kernels read (_close's default).  Values: rtol = atol = 1e-6.
BAR = 1e-4
WORST = {}


def _t(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV).contiguous()


def _launch(batch, tabs, both=True):
    """log Z on a private workspace -> the keyword arguments of ops.expected_reward / ops.expected_reward_bwd."""
    from action_segmentation_amd import ops
    elp, trans, init, lens, ep = tabs
    ws = torch.empty(batch.workspace_bytes(), dtype=torch.uint8, device=DEV)
    z = ops.logz(batch, elp, trans, init, lens, endpen=ep, ws=ws, with_backward=both)
    return dict(elp=elp, trans=trans, init=init, len_scores=lens, logz_val=z, endpen=ep, ws=ws, with_backward=both)


def _value(batch, kw, reward, seg):
    from action_segmentation_amd import ops
    v, parts = ops.expected_reward(batch, reward=reward, seg_reward=seg, want_parts=True, **kw)
    torch.cuda.synchronize()
    return v.cpu().numpy(), parts.cpu().numpy()


def _grad(batch, kw, reward, seg, up=None):
    from action_segmentation_amd import ops
    g = ops.expected_reward_bwd(batch, reward=reward, seg_reward=seg, grad_out=up, want_value=True, **kw)
    torch.cuda.synchronize()
    return g


# ----------------------------------------------------------------------------------------------- 1. enumerable lattices
# Measured on one MI355X, worst over the nine lattices, |error| / max(1, max |ref|) over the four tables / |value - reference|:
#   both rewards 2.3e-7 / 7.6e-7      reward only 2.3e-7 / 3.4e-7      seg_reward only 1.7e-7 / 5.4e-7
@pytest.mark.parametrize('setting', E.SETTINGS)
@pytest.mark.parametrize('k,add_eos,masked,additional,narration', SMALL)
def test_exact_on_enumerable_lattices(k, add_eos, masked, additional, narration, setting):
    """Value (smm_expected_reward_f64, its two parts, V-, V+) and all four tables against the enumeration of every segmentation,
    with both rewards, the frame reward only and the segment reward only; upstream weights [1, -0.5, 2]."""
    from action_segmentation_amd import ops
    (elp, lengths, trans, init, lens, ep), _ = _small_case(k, add_eos, masked, additional, narration, 'draw')
    b, tmax, c = elp.shape
    no_eos = not add_eos
    reward, seg = E.small_rewards(1000 + k, b, tmax, c, setting)
    up = np.array([1.0, -0.5, 2.0])
    vals, parts, ref = E.batch_reference(E.video_enumeration, elp, lengths, trans, init, lens, min(k, max(lengths)), no_eos, ep,
                                         reward, seg, up)
    batch, *tabs = _batch_tables(elp, lengths, trans, init, lens, ep, no_eos=no_eos)
    rw = None if reward is None else _t(reward.reshape(b * tmax, c))
    sg = None if seg is None else _t(seg[None])
    kw = _launch(batch, tabs)
    v, pt = _value(batch, kw, rw, sg)
    g = _grad(batch, kw, rw, sg, _t(up))
    assert ops.error_flag(batch, ws=kw['ws']) == 0
    np.testing.assert_allclose(v, vals, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(pt, parts, rtol=1e-6, atol=1e-6)
    vv = g['value'].cpu().numpy()
    np.testing.assert_allclose(vv[:, 0], vals, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(vv[:, 1], vals, rtol=1e-6, atol=1e-6)
    w = _close(g, ref, ('small', setting), BAR)
    WORST[('small', setting)] = max(WORST.get(('small', setting), 0.0), w)
    print('small lattice K=%d eos=%s %s: worst |error| / max(1, max |ref|) %.3g; values off by %.3g'
          % (k, add_eos, setting, w, float(np.abs(v - vals).max())))


# ------------------------------------------------------------------------------------ 2. mid sizes, entry by entry
# entropy_grad_cases.MID crosses the splits of smm_expected_reward.hip, which are smm_entropy_bwd.hip's: several trips of the
# 32-lane length loop (k_trips), the second block of the length kernel (k_blocks: k = 300, T = 330), all 32 class groups and a
# one-frame video (states_32), 23 states without EOS at T = 128 / 64 / 1 (states_23_no_eos), packed groups with padded states,
# per-video kp and a zero upstream weight (packed_groups); the prefix kernel's 32 chunks are crossed by every T > 32.
# V- and V+ come out of self-normalised local distributions and are held to 1e-6, as test_gpu_entropy_grad.py holds its
# value_out.  The value kernel multiplies node posteriors read off the histories (exp(F + B - log Z), the fp32 sums of
# smm_logz_kernel: the segment-posterior tests measure them to 2e-5), so at these sizes it is held to the histories' stated
# accuracy, the bar, as test_gpu_entropy_grad.py holds smm_entropy_f64 there.
# Measured on one MI355X, worst |error| / max(1, max |ref|) over the four tables / V- and V+ / the value call:
#   k_trips            1.3e-6 / 3.8e-8 / 5.3e-7
#   k_blocks           4.6e-6 / 2.1e-8 / 5.5e-6
#   states_32          2.5e-6 / 1.8e-7 / 8.4e-7
#   states_23_no_eos   3.0e-7 / 3.7e-8 / 9.7e-7
#   packed_groups      6.3e-7 / 1.0e-7 / 6.1e-6
# No case needs a bar of its own.
@functools.lru_cache(maxsize=None)
def _mid_reference(name):
    """(reward, seg_reward, values, parts, grads) of mid_case(name) by reference (b).  Computed once; leave it unchanged."""
    case = C.mid_case(name)
    rng = np.random.default_rng(case['total_frames'] + 17)
    reward = rng.normal(size=(case['total_frames'], case['c_max']))
    seg = rng.normal(size=(len(case['n_states']), case['c_max']))
    p = case['p']
    vals, parts, g = E.batch_reference(E.video_polynomial, p[0], case['lengths'], p[1], p[2], p[3], case['kp'], case['no_eos'], p[4],
                                       reward, seg, case['up'], group=case['group'], n_states=case['n_states'],
                                       frame_offset=case['frame_offset'])
    return reward, seg, vals, parts, g


@pytest.mark.parametrize('name', list(C.MID))
def test_entry_by_entry_at_mid_sizes(name):
    from action_segmentation_amd import ops
    case = C.mid_case(name)
    reward, seg, vals, parts, ref = _mid_reference(name)
    (batch, *tabs), rows = _mid_launch(case, 'p')
    if case['single']:                                      # (padded rows: the reward of video i at i * tmax)
        tmax = max(case['lengths'])
        rw = np.zeros((len(rows) * tmax, case['c_max']))
        for r, o, n in zip(rows, case['frame_offset'], case['lengths']):
            rw[r] = reward[o:o + n]
        # NaN where no video reads: padded frames change nothing
        covered = np.zeros(rw.shape[0], bool)
        covered[np.concatenate(rows)] = True
        rw[~covered] = np.nan
    else:
        rw = reward.copy()
        rw[-C.MID_TAIL:] = np.nan                           # frames no video covers
        for i, (o, n) in enumerate(zip(case['frame_offset'], case['lengths'])):
            rw[o:o + n, case['n_states'][case['group'][i]]:] = np.nan       # padded columns
    kw = _launch(batch, tabs)
    v, pt = _value(batch, kw, _t(rw), _t(seg))
    g = _grad(batch, kw, _t(rw), _t(seg), _t(case['up']))
    assert ops.error_flag(batch, ws=kw['ws']) == 0
    failures = []
    scale = np.maximum(1.0, np.abs(vals))
    vv = g['value'].cpu().numpy()
    rv = max(float((np.abs(vv[:, j] - vals) / scale).max()) for j in (0, 1))
    rd = float((np.abs(v - vals) / scale).max())
    w = _entries(g, ref, case, rows, (name, 'expected reward'), BAR, failures)
    WORST[('mid', name)] = w
    print('mid %s: values %s; V-/V+ off by %.3g, the value kernel by %.3g; worst |error| / max(1, max |ref|) %.3g'
          % (name, vals, rv, rd, w))
    if not (np.isfinite(vv).all() and rv <= 1e-6):
        failures.append('%s: value_out %s, reference %s: off by %.3g > 1e-6' % (name, vv.tolist(), vals, rv))
    if not rd <= BAR:
        failures.append('%s: the value kernel gives %s, reference %s: off by %.3g > %.3g' % (name, v, vals, rd, BAR))
    if not (np.abs(pt - parts) <= BAR * np.maximum(1.0, np.abs(parts))).all():
        failures.append('%s: parts %s, reference %s' % (name, pt, parts))
    _padding_is_zero(g, case, rows, name)
    assert not failures, '\n'.join(failures)


# ------------------------------------------------------------------------------------------- 3. identities, real sizes
# Measured on one MI355X, 16 states T = 2048 span limit 255 / 23 states T = 1500 span limit 1023:
#   symmetry of the Hessian                       3.8e-5 / 3.4e-6 of the larger side
#   linearity, gradients                          7e-13 / 6e-14
#   reward = 1: |V - T| / T, worst |gradient|     2.3e-7, 2.6e-12 / 2.1e-7, 6.2e-13
#   V- against V+ (one-hot; N(0, 1))              4.9e-10, 1.7e-8 / 4.0e-10, 5.3e-7 of max(1, |V|)
#   the value call against V- (one-hot)           3.9e-7 / 1.1e-5 of V
#   the value call against V- (N(0, 1)), absolute 3.6e-5 / 5.3e-4 (1e-6 sum |reward| = 0.026 / 0.028)
#   <posteriors, reward> against the value call   4.9e-5 / 6.7e-4 absolute (N(0, 1)); 1.4e-7 / 3.4e-6 of V (one-hot)
#   expected segment count against sum(start)     0 / 0
#   MBR gain against the value call               1.4e-7 / 3.4e-6 of the gain; against V-: 5.2e-7 / 1.5e-5
BIG = dict(
    s16=dict(states=[16], k=256, lengths=[2048], eos=True, runs=(20, 200), seed=8100),       # span limit 255
    s23=dict(states=[23], k=1024, lengths=[1500], eos=True, runs=(50, 600), seed=8200),      # span limit 1023
)


@functools.lru_cache(maxsize=None)
def _big(name):
    """-> ((elp, lengths, trans, init, lens, endpen) of one video, the labels its emissions were drawn around)."""
    cfg = BIG[name]
    rng = np.random.default_rng(cfg['seed'])
    labels = [C._labels(rng, t, cfg['runs'], cfg['states'][0]) for t in cfg['lengths']]
    elp, trans, init, lens, ep = C._mid_side(cfg, labels, cfg['seed'] + 1)
    t, c = cfg['lengths'][0], cfg['states'][0]
    return (elp[:t].reshape(1, t, c), cfg['lengths'], trans[0], init[0], lens[0], ep), labels[0]


@pytest.mark.parametrize('name', list(BIG))
def test_identities_at_real_sizes(name):
    """Identities that need no reference, each inside the bar (the docstring of every block says which)."""
    from action_segmentation_amd import ops
    (elp, lengths, trans, init, lens, ep), lab = _big(name)
    T, c = lengths[0], elp.shape[2]
    batch, *tabs = _batch_tables(elp, lengths, trans, init, lens, ep)
    kw = _launch(batch, tabs)
    rng = np.random.default_rng(5)
    v_, w_ = rng.normal(size=(T, c)), rng.normal(size=(T, c))
    sg = rng.normal(size=(1, c))
    gv, gw = _grad(batch, kw, _t(v_), None), _grad(batch, kw, _t(w_), None)
    # symmetry of the Hessian of log Z: <v, g_elp(w)> = <w, g_elp(v)>
    a, b = float((_t(v_) * gw['elp']).sum()), float((_t(w_) * gv['elp']).sum())
    sym = abs(a - b) / max(1.0, abs(a), abs(b))
    print('%s symmetry: %.12g against %.12g: %.3g' % (name, a, b, sym))
    assert sym <= BAR
    # linearity in the reward
    gl = _grad(batch, kw, _t(2.0 * v_ - 3.0 * w_), None)
    lin = 0.0
    for k in TABLES:
        want = 2.0 * gv[k] - 3.0 * gw[k]
        lin = max(lin, float((gl[k] - want).abs().max()) / max(1.0, float(want.abs().max())))
    lv = float((gl['value'] - (2.0 * gv['value'] - 3.0 * gw['value'])).abs().max()) / max(1.0, float(gl['value'].abs().max()))
    print('%s linearity: gradients %.3g, values %.3g' % (name, lin, lv))
    assert lin <= BAR and lv <= BAR
    # reward = 1 for every class: V is the frame count, every gradient 0 within the bar x max(1, T)
    ones = _t(np.ones((T, c)))
    v1, _ = _value(batch, kw, ones, None)
    g1 = _grad(batch, kw, ones, None)
    z = max(float(g1[k].abs().max()) for k in TABLES)
    print('%s reward = 1: V %.12g (T = %d), worst |gradient| %.3g' % (name, v1[0], T, z))
    assert abs(v1[0] - T) <= 1e-6 * T and z <= BAR * max(1, T)
    # V- = V+ = the value call's value.  V- and V+ come out of self-normalised local distributions: inside the bar of each
    # other for any reward.  The value call is <node posteriors, prefix sums>: against V- it is inside the bar for the rewards
    # the entry point is for (the one-hot ground truth -- the labels the emissions were drawn around -- and a segment reward
    # of 1, every term >= 0); for zero-mean N(0, 1) rewards V is the cancelled total of T terms, and the call is held to what
    # tests/test_gpu_mbr.py holds each frame posterior to, 1e-6, times sum |reward|
    onehot = np.zeros((T, c))
    onehot[np.arange(T), lab] = 1.0
    for what, rw, s_rw in (('one-hot', onehot, np.ones((1, c))), ('N(0, 1)', v_, sg)):
        vb, _ = _value(batch, kw, _t(rw), _t(s_rw))
        gb = _grad(batch, kw, _t(rw), _t(s_rw))['value'].cpu().numpy()[0]
        scale = max(1.0, abs(vb[0]))
        d01, dv = abs(gb[0] - gb[1]) / scale, max(abs(gb[0] - vb[0]), abs(gb[1] - vb[0]))
        print('%s %s rewards: V %.12g, V- %.12g, V+ %.12g: V- against V+ %.3g, the value call off by %.3g (absolute)'
              % (name, what, vb[0], gb[0], gb[1], d01, dv))
        assert d01 <= BAR
        assert dv <= (BAR * scale if what == 'one-hot' else 1e-6 * float(np.abs(rw).sum()) + BAR * scale)
    # the value equals <frame posteriors, reward>; the segment count equals the sum of the span-start posteriors
    tb = {k: kw[k] for k in ('elp', 'trans', 'init', 'len_scores', 'logz_val', 'endpen', 'ws', 'with_backward')}
    post = ops.logz_bwd(batch, **tb)['elp']
    want = float((post * _t(v_)).sum())
    vf, _ = _value(batch, kw, _t(v_), None)
    print('%s <posteriors, reward> %.12g, value %.12g' % (name, want, vf[0]))
    # (two orders of summation over the same node posteriors, a zero-mean reward: the bound of the N(0, 1) case above)
    assert abs(vf[0] - want) <= 1e-6 * float(np.abs(v_).sum()) + BAR * max(1.0, abs(want))
    want = float((post * _t(onehot)).sum())
    vf, _ = _value(batch, kw, _t(onehot), None)
    print('%s <posteriors, one-hot labels> %.12g, value %.12g' % (name, want, vf[0]))
    assert abs(vf[0] - want) <= BAR * max(1.0, abs(want))
    sp = ops.segment_posteriors(batch, **tb)
    vs, _ = _value(batch, kw, None, _t(np.ones((1, c))))
    want = float(sp['start'].sum())
    print('%s sum of start posteriors %.12g, expected segment count %.12g' % (name, want, vs[0]))
    assert abs(vs[0] - want) <= 1e-6 * max(1.0, want)
    # expected_reward(onehot(labels of the MBR decode)) is the expected gain smm_mbr_f64 reports.  The gain is the frame
    # posteriors summed along the labels -- to 1e-12 T, tests/test_gpu_mbr.py's tolerance for that sum -- so what is left is the
    # identity above: the value call against <posteriors, one-hot>, inside the bar.  (V- and V+ of the same reward, which agree
    # to 1e-9, say how far both gathers are from the truth at these sizes: the figures are printed.)
    mb = ops.mbr(batch, post, kw['trans'], kw['init'], endpen=kw['endpen'], ws=kw['ws'], want_spans=False, want_labels=True)
    mlab = mb['labels'][:T]
    gain = float(mb['gain_sum'][0])
    assert abs(gain - float(post[torch.arange(T, device=DEV), mlab].sum())) <= 1e-12 * T
    moh = torch.zeros((T, c), dtype=torch.float64, device=DEV)
    moh[torch.arange(T, device=DEV), mlab] = 1.0
    kw2 = _launch(batch, tabs)                             # (the MBR decode took the workspace's history area)
    vm, _ = _value(batch, kw2, moh, None)
    vmm = _grad(batch, kw2, moh, None)['value'].cpu().numpy()[0]
    print('%s MBR gain %.12g, expected accuracy of its labels %.12g (V- %.12g, V+ %.12g)' % (name, gain, vm[0], vmm[0], vmm[1]))
    assert abs(vm[0] - gain) <= BAR * max(1.0, gain)
    assert abs(vmm[0] - gain) <= BAR * max(1.0, gain) and abs(vmm[1] - gain) <= BAR * max(1.0, gain)


# ----------------------------------------------------------------------------- 4. central differences of the marginals
# Measured on one MI355X, <w, g_elp(w)>: kernel / differences at 1e-2 / at 5e-3, then the same along u:
#   16 states, T = 2048   18.0959 / 18.0936 / 18.0904      1.4288 / 1.4259 / 1.4267
#   23 states, T = 1500    3.3043 /  3.3046 /  3.3021      0.0128 / 0.0151 / 0.0339
@pytest.mark.parametrize('name', list(BIG))
def test_directional_derivative_against_central_differences_of_the_marginals(name):
    """g_elp(w) = d/d eps mu(elp + eps w): central differences of smm_logz_bwd_f64's marginals, projected on w itself (the
    quadratic form <w, g_elp(w)> = Var_p(R_w) >= 0) and on a second random direction.  Step sizes and bar as in
    test_gpu_entropy_grad.py's test_directional_derivatives_against_central_differences -- two steps, one half the other, whose
    disagreement bounds the differences' own error -- with steps ten times its 1e-3 / 5e-4: those differenced the C twin's fp64
    value, these difference marginals that carry the histories' ~1e-6 per entry over T x C entries."""
    from action_segmentation_amd import ops
    (elp, lengths, trans, init, lens, ep), _ = _big(name)
    T, c = lengths[0], elp.shape[2]
    rng = np.random.default_rng(11)
    w_ = rng.normal(size=(T, c)) * (elp[0] > -1e8)         # (masks stay masks)
    batch, *tabs = _batch_tables(elp, lengths, trans, init, lens, ep)
    g = _grad(batch, _launch(batch, tabs), _t(w_), None)
    mus = {}
    for eps in (1e-2, 5e-3):
        for sgn in (1.0, -1.0):
            b2, *t2 = _batch_tables(elp + sgn * eps * w_[None], lengths, trans, init, lens, ep)
            kw = _launch(b2, t2)
            kw = {k: kw[k] for k in ('elp', 'trans', 'init', 'len_scores', 'logz_val', 'endpen', 'ws', 'with_backward')}
            mus[(eps, sgn)] = ops.logz_bwd(b2, **kw)['elp']
    for what, u_ in (('w', _t(w_)), ('u', _t(rng.normal(size=(T, c))))):
        dirv = float((g['elp'] * u_).sum())
        fd = [float(((mus[(eps, 1.0)] - mus[(eps, -1.0)]) * u_).sum()) / (2 * eps) for eps in (1e-2, 5e-3)]
        noise = abs(fd[0] - fd[1]) + 1e-7 * max(1.0, abs(dirv))
        err = abs(dirv - fd[1])
        print('%s <%s, g_elp(w)>: kernel %.9g, differences %.9g / %.9g' % (name, what, dirv, fd[0], fd[1]))
        assert err <= 4 * noise + 1e-4 * max(1.0, abs(fd[1])), (what, dirv, fd)
        if what == 'w':
            assert dirv > 0.0 and noise <= 0.05 * dirv, (dirv, fd)          # (the differences resolve the variance)


# ------------------------------------------------------------------------------------------------- 5. same bits twice
def test_two_calls_are_bit_identical():
    (elp, lengths, trans, init, lens, ep), _ = _small_case(4, True, True, True, True, 'draw')
    b, tmax, c = elp.shape
    reward, seg = E.small_rewards(3, b, tmax, c, 'both')
    small = _batch_tables(elp, lengths, trans, init, lens, ep)
    packed, _ = _mid_launch(C.mid_case('packed_groups'), 'p')
    mid_reward, mid_seg = _mid_reference('packed_groups')[:2]
    for (batch, *tabs), rw, sg in ((small, _t(reward.reshape(b * tmax, c)), _t(seg[None])), (packed, _t(mid_reward), _t(mid_seg))):
        kw = _launch(batch, tabs)
        v0, p0 = _value(batch, kw, rw, sg)
        v1, p1 = _value(batch, kw, rw, sg)
        assert np.array_equal(v0.view(np.int64), v1.view(np.int64)) and np.array_equal(p0.view(np.int64), p1.view(np.int64))
        a, b2 = _grad(batch, kw, rw, sg), _grad(batch, kw, rw, sg)
        for k in TABLES + ('value',):
            assert torch.equal(a[k], b2[k]), k
        # the value call leaves the histories as they were: the gradient after it gives the same bits
        _value(batch, kw, rw, sg)
        c2 = _grad(batch, kw, rw, sg)
        for k in TABLES + ('value',):
            assert torch.equal(a[k], c2[k]), k


def test_without_logz_both_the_call_runs_the_reversed_recursion_itself():
    (elp, lengths, trans, init, lens, ep), _ = _small_case(4, False, True, False, True, 'draw')
    b, tmax, c = elp.shape
    reward, seg = E.small_rewards(4, b, tmax, c, 'both')
    batch, *tabs = _batch_tables(elp, lengths, trans, init, lens, ep, no_eos=True)
    rw, sg = _t(reward.reshape(b * tmax, c)), _t(seg[None])
    kw1, kw0 = _launch(batch, tabs, both=True), _launch(batch, tabs, both=False)
    v1, _ = _value(batch, kw1, rw, sg)
    v0, _ = _value(batch, kw0, rw, sg)
    np.testing.assert_allclose(v0, v1, rtol=1e-12, atol=1e-12)
    g1 = _grad(batch, kw1, rw, sg)
    g0 = _grad(batch, _launch(batch, tabs, both=False), rw, sg)
    for k in TABLES:
        torch.testing.assert_close(g0[k], g1[k], rtol=1e-12, atol=1e-12)


# -------------------------------------------------------------------------------------------------------- 6. errors
def test_errors():
    """A NaN in a covered reward entry: NaN for that video only, and the error word; a video whose log Z is -inf: NaN rows and
    group tables; a NaN in a padded column or an uncovered frame changes nothing."""
    from action_segmentation_amd import ops
    case = C.mid_case('packed_groups')
    reward, seg, vals, parts, ref = _mid_reference('packed_groups')
    (batch, *tabs), rows = _mid_launch(case, 'p')
    up = _t(case['up'])
    kw = _launch(batch, tabs)
    v_clean, _ = _value(batch, kw, _t(reward), _t(seg))
    g_clean = _grad(batch, kw, _t(reward), _t(seg), up)
    assert ops.error_flag(batch, ws=kw['ws']) == 0
    # a NaN in a padded column (video 0: group 0 has 6 of 17 states) and in a frame no video covers: the same bits
    pad = reward.copy()
    pad[case['frame_offset'][0] + 3, 10] = np.nan
    pad[-1, 0] = np.nan
    kw = _launch(batch, tabs)
    v, _ = _value(batch, kw, _t(pad), _t(seg))
    g = _grad(batch, kw, _t(pad), _t(seg), up)
    assert ops.error_flag(batch, ws=kw['ws']) == 0
    assert np.array_equal(v.view(np.int64), v_clean.view(np.int64))
    for k in TABLES + ('value',):
        assert torch.equal(g[k], g_clean[k]), k
    # a NaN in a covered entry of video 3 (group 0)
    bad = reward.copy()
    bad[case['frame_offset'][3] + 5, 2] = np.nan
    kw = _launch(batch, tabs)
    v, pt = _value(batch, kw, _t(bad), _t(seg))
    assert ops.error_flag(batch, ws=kw['ws']) != 0
    assert np.isnan(v[3]) and np.isnan(pt[3]).all()
    others = [0, 1, 2, 4]
    assert np.array_equal(v[others].view(np.int64), v_clean[others].view(np.int64))
    kw = _launch(batch, tabs)
    g = _grad(batch, kw, _t(bad), _t(seg), up)
    assert ops.error_flag(batch, ws=kw['ws']) != 0
    vv = g['value'].cpu().numpy()
    assert np.isnan(vv[3]).all() and np.array_equal(vv[others].view(np.int64), g_clean['value'].cpu().numpy()[others].view(np.int64))
    ge, gc = g['elp'].cpu().numpy(), g_clean['elp'].cpu().numpy()
    c0 = case['n_states'][0]
    assert np.isnan(ge[rows[3]][:, :c0]).all()
    for i in others:
        assert np.array_equal(ge[rows[i]].view(np.int64), gc[rows[i]].view(np.int64)), i
    assert torch.isnan(g['trans'][0, :c0, :c0]).all() and torch.isnan(g['init'][0, :c0]).all()
    for k in ('trans', 'init', 'len'):
        assert torch.equal(g[k][1], g_clean[k][1]), k           # the other group's tables
    # a video whose log Z is -inf (video 1, group 1)
    for fn in ('value', 'grad'):
        kw = _launch(batch, tabs)
        kw['logz_val'] = kw['logz_val'].clone()
        kw['logz_val'][1] = float('-inf')
        if fn == 'value':
            v, _ = _value(batch, kw, _t(reward), _t(seg))
            assert np.isnan(v[1]) and np.isfinite(v[[0, 2, 3, 4]]).all()
        else:
            g = _grad(batch, kw, _t(reward), _t(seg), up)
            c1 = case['n_states'][1]
            assert torch.isnan(g['elp'][torch.as_tensor(rows[1], device=DEV)][:, :c1]).all()
            assert torch.isnan(g['trans'][1, :c1, :c1]).all() and torch.isnan(g['init'][1, :c1]).all()
            assert torch.isfinite(g['trans'][0]).all() and torch.isfinite(g['elp'][torch.as_tensor(rows[0], device=DEV)]).all()
        assert ops.error_flag(batch, ws=kw['ws']) != 0
    # the wrappers refuse what the library would
    with pytest.raises(ValueError):
        ops.expected_reward(batch, **_launch(batch, tabs))
    with pytest.raises(ValueError):
        ops.expected_reward(batch, reward=_t(reward[:-1]), **_launch(batch, tabs))
