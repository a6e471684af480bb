"""tests/decode_corpus.py checked on the host: the conditions that tests/test_gpu_decode_plans.py leans on.  The time-split
planner cuts exactly the three long videos; the corpus holds no decision that the emission kernel's rounding could flip (so
"labels equal the twin's" is a fair demand of the GPU); and the decode it asks for is a sensible one (the twin recovers the
sampled labels).  If the planner or the builder changes, this fails here instead of the GPU test quietly going easy."""
import numpy as np
import pytest

import decode_corpus as DC


@pytest.mark.parametrize('dressing', DC.DRESSINGS)
def test_time_split_plan_cuts_exactly_the_three_long_videos(dressing):
    cp = DC.corpus(dressing)
    units = DC.time_split_units(cp)
    cut = [i for i, u in enumerate(units) if u]
    assert cut == sorted(DC.LONG), cut
    ov = 512 + (DC.K - 1)
    for i in cut:
        t = int(cp['lengths'][i])
        assert t >= ov + 2 * (DC.K - 1)
        assert len(units[i]) >= 2, units[i]
        assert units[i][0] == (0, units[i][0][1], 0)
        for first, n, front in units[i][1:]:
            assert front == ov and n - front >= DC.K - 1
        assert units[i][-1][0] + units[i][-1][1] == t                        # the last unit ends the video
    assert all(cp['lengths'][i] < ov + 2 * (DC.K - 1) for i in range(cp['b']) if i not in DC.LONG)


@pytest.mark.parametrize('dressing', DC.DRESSINGS)
def test_stream_split_threshold_separates_the_same_three_videos(dressing):
    """choose_split (smm_api.hip) with SMM_SPLIT_MIN_US=0 and the default margin: the critical part is what lies within
    em_us / split_ns + 400 frames of the longest video, em_us the emission's modelled time.  Restated here from its formula."""
    cp = DC.corpus(dressing)
    b, lengths = cp['b'], cp['lengths']
    em_us = cp['total'] * (4.0 * DC.D + 8.0 * DC.C_MAX) / 4.0e6
    split_ns = 1.75 * (145.0 + 2.0 * DC.C_MAX)
    thr = int(lengths.max()) - int(em_us * 1000.0 / split_ns) - 400
    critical = np.flatnonzero(lengths >= thr).tolist()
    assert critical == sorted(DC.LONG), (thr, critical)
    assert b >= 24 and len(critical) <= b // 3 and b - len(critical) >= 16


@pytest.mark.parametrize('dressing', DC.DRESSINGS)
def test_no_decision_within_reach_of_the_emission_kernels_rounding(dressing):
    """The twin's decode does not change when every emission score moves by up to 1e-7 -- 100 x the fp64 emission tolerance
    (rtol 1e-12 of |elp| <= 1e4, atol 1e-9)."""
    cp, tw = DC.corpus(dressing), DC.twin(dressing)
    for seed in range(3):
        g = np.random.default_rng(1000 + seed)
        noisy = [e + g.uniform(-1e-7, 1e-7, size=e.shape) for e in tw['elp']]
        spans, best = DC.twin_viterbi(cp, noisy)
        for i in range(cp['b']):
            np.testing.assert_array_equal(spans[i], tw['spans'][i], err_msg='seed %d, video %d' % (seed, i))
        np.testing.assert_allclose(best, tw['best'], rtol=1e-9)


@pytest.mark.parametrize('dressing', DC.DRESSINGS)
def test_twin_recovers_the_sampled_labels(dressing):
    cp, tw = DC.corpus(dressing), DC.twin(dressing)
    same = sum(int((a == b).sum()) for a, b in zip(tw['labels'], cp['labs']))
    assert same > 0.95 * int(cp['lengths'].sum()), same / cp['lengths'].sum()
    for i in range(cp['b']):
        t, c = int(cp['lengths'][i]), DC.STATES[cp['group'][i]]
        assert tw['spans'][i][t] == c and np.isfinite(tw['best'][i]) and tw['best'][i] > -1e8    # a path no hard penalty touched
        if cp['endpen'] is not None:
            assert cp['endpen'][i, tw['labels'][i][-1]] == 0.0
            assert 2 <= int((cp['endpen'][i] == 0.0).sum()) <= 3


def test_the_dressings_differ_where_they_should():
    plain, dressed = DC.corpus('plain'), DC.corpus('dressed')
    assert plain['cons'] is None and plain['endpen'] is None and plain['class_map'] is None
    assert plain['total'] == int(plain['lengths'].sum()) and DC.covered(plain).all()
    assert dressed['total'] > int(dressed['lengths'].sum()) and not DC.covered(dressed).all()
    assert (dressed['cons'] == -1e4).any() and (dressed['cons'][~DC.covered(dressed)] == 0).all()
    assert int(plain['kp'].max()) == DC.K > 512 and int(plain['kp'].min()) == 9
