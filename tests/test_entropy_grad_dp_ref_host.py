"""The polynomial-time reference of the entropy / cross-entropy / KL gradients (tests/entropy_grad_dp_ref.py) is pinned here, on
the CPU, before any kernel is compared with it: against the enumeration on the small lattices, against the C twin's log Z and
entropy at the mid sizes, and the conditions under which the mid-size cases of test_gpu_entropy_grad.py exercise what they are
there for."""
import numpy as np
import pytest

import entropy_grad_cases as C
import entropy_grad_dp_ref as D
import entropy_grad_ref as R
from oracle import factored as F
from test_gpu_entropy import _twin_entropy

TABLES = ('elp', 'trans', 'init', 'len')
MODES = ('entropy', 'cross_entropy', 'kl')


@pytest.mark.parametrize('k,add_eos,masked,additional,narration', C.SMALL + [(3, False, False, False, False)])
def test_against_enumeration(k, add_eos, masked, additional, narration):
    """Values and every gradient entry of both sides, all three modes: <= 1e-10 max(1, max |ref|) from the enumeration."""
    p, q = C._small_case(k, add_eos, masked, additional, narration, 'draw')
    elp, lengths, trans, init, lens, ep = p
    kp, up = min(k, max(lengths)), np.array([1.0, -0.5, 2.0])
    got = D.batch_reference(elp, lengths, trans, init, lens, kp, not add_eos, ep, q, None, up)
    worst = 0.0
    for mode in MODES:
        vals, rp, rq = R.batch_reference(elp, lengths, trans, init, lens, kp, not add_eos, ep, q, mode, up)
        gv, gp, gq = got[mode]
        assert gv.shape == vals.shape and np.abs(gv - vals).max() <= 1e-10 * max(1.0, np.abs(vals).max()), (mode, gv, vals)
        for side, a, r in (('p', gp, rp), ('q', gq, rq)):
            for t in TABLES:
                assert a[t].shape == r[t].shape, (mode, side, t)
                err = float((a[t] - r[t]).abs().max()) / max(1.0, float(r[t].abs().max()))
                worst = max(worst, err)
                assert err <= 1e-10, (mode, side, t, err)
    print('K %d eos %s: worst |dp - enumeration| / max(1, max |ref|) %.3g' % (k, add_eos, worst))


def test_single_mode_is_the_same_pass():
    p, q = C._small_case(4, True, True, False, False, 'draw')
    elp, lengths, trans, init, lens, ep = p
    up = np.array([1.0, -0.5, 2.0])
    every = D.batch_reference(elp, lengths, trans, init, lens, 4, False, ep, q, None, up)
    one = D.batch_reference(elp, lengths, trans, init, lens, 4, False, ep, q, 'kl', up)
    assert np.array_equal(one[0], every['kl'][0])
    for t in TABLES:
        assert (one[1][t] == every['kl'][1][t]).all() and (one[2][t] == every['kl'][2][t]).all()


def _padded(case, i, rows):
    """Video i's tables for the twin: its elp in a row of `rows` frames, the real states of its group.  The twin takes a span's
    emissions from one prefix sum, which behind ten -1e9 entries carries ulp(1e10) ~ 2e-6 (measured: 2.3e-6 of log Z on k_trips);
    it gets the window at -1e4 instead -- exp(-1e4) is 0 as well, so log Z and H are those of the case -- while the reference
    under test keeps the case's own -1e9."""
    side, ep = C.video_side(case, i)
    t, c = side['elp'].shape
    e = np.zeros((1, max(rows, t), c))
    e[0, :t] = np.where(side['elp'] > -1e8, side['elp'], -1e4)
    return e, side, (None if ep is None else ep[None])


@pytest.mark.parametrize('name', list(C.MID))
def test_mid_sizes_against_the_twin(name):
    """log Z of every video against oracle.factored.logz, and with EOS the entropy against log Z - E[score] of the twin's
    marginals: 1e-9 relative.  (Without EOS _twin_entropy has no closing term: log Z only.)"""
    case = C.mid_case(name)
    ref = C.mid_reference(name)['entropy'][0]
    for i, t in enumerate(case['lengths']):
        kp = case['kp'][i]
        e, side, ep = _padded(case, i, kp)                       # (the twin's span limit is min(K, frames of the row))
        z = F.logz(e, [t], side['trans'], side['init'], side['len'][:kp], endpen=ep, no_eos=case['no_eos'])[0]
        mine = D.logz(side, kp, case['no_eos'], None if ep is None else ep[0])
        assert abs(mine - z) <= 1e-9 * max(1.0, abs(z)), (name, i, mine, z)
        if not case['no_eos']:
            h = _twin_entropy(e, [t], side['trans'], side['init'], side['len'][:kp], ep, tmax=kp)[0]
            assert abs(ref[i] - h) <= 1e-9 * max(1.0, abs(h)), (name, i, ref[i], h)


# (case, video, spans at least this long, their share of the video's expected spans under p)
LONG_SPANS = [('k_trips', 0, 33, 0.15), ('k_trips', 0, 65, 0.05), ('k_blocks', 0, 257, 0.10), ('states_23_no_eos', 0, 33, 0.15)]


@pytest.mark.parametrize('name,video,at_least,share', LONG_SPANS)
def test_long_spans_carry_probability(name, video, at_least, share):
    """The trips of the length loop and the blocks of the length kernel beyond the first see spans that matter."""
    got = C.long_span_share(name, video, at_least)
    print('%s video %d: %.3f of the expected spans are >= %d long' % (name, video, got, at_least))
    assert got >= share


@pytest.mark.parametrize('name', list(C.MID))
def test_gradients_are_not_small(name):
    """max |ref| of g_elp and g_len >= 0.1 in every mode (the tolerance is relative to max(1, max |ref|))."""
    ref = C.mid_reference(name)
    for mode in MODES:
        for t in ('elp', 'len'):
            m = float(ref[mode][1][t].abs().max())
            print('%s %s: max |g_%s| %.3g' % (name, mode, t, m))
            assert m >= 0.1, (name, mode, t, m)
