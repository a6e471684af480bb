"""The feedback planner (csrc/smm_plan_feedback.h) through its C entry, on synthetic per-video times: no GPU.

The planner gets measured DP times per video and the plan they were measured under, replays the split decode from them and
returns the first part -- the videos with the largest measured times -- whose replay ends first.  Checked here: on cfg3's own
(frames, states) structure with times the model misses by up to 15 %; on equal times (the plan stays); on launches the guards
of choose_split do not admit (the plan stays); and that the same input gives the same plan."""
import functools

import numpy as np
import pytest

N_CU = 256


@functools.lru_cache(maxsize=None)
def cfg3():
    """cfg3 seed 2, structure only: frames and states by video, the emission pass's modelled time, and the shipped plan --
    launch order by modelled time, the first part what choose_split's threshold (restated from its formula) takes."""
    from action_segmentation_amd import synth, _lib, _build
    _build.build()
    lib = _lib.load()
    data = synth.SynthDatasplit('cfg3', seed=2, keep=set())
    frames, states = [], []
    for (task, name), v in data._videos.items():
        frames.append(int(v['features'].shape[0]))
        states.append(len(v['task_indices']))
    frames, states = np.array(frames, np.int32), np.array(states)
    d, c_max = data.feature_dim, int(states.max())
    ns = np.array([lib.smm_band_frame_ns(int(c)) for c in states])
    em_us = float(frames.sum()) * (4.0 * d + 8.0 * c_max) / 4.0e6
    split_ns = 1.75 * lib.smm_band_frame_ns(c_max)
    thr = int(frames.max()) - int(em_us * 1000.0 / split_ns) - 400
    order = np.argsort(-(frames * ns), kind='stable').astype(np.int32)
    order = np.concatenate([order[frames[order] >= thr], order[frames[order] < thr]]).astype(np.int32)
    return dict(frames=frames, ns=ns, em_us=em_us, order=order, n1=int((frames >= thr).sum()))


def guards(b, n1, n_cu=N_CU):
    return b >= 24 and 1 <= n1 <= b // 3 and n1 <= n_cu // 2 and b - n1 >= 16


def test_cfg3_structure_with_times_off_the_model_by_15_percent():
    from action_segmentation_amd import ops
    c = cfg3()
    b = len(c['frames'])
    assert b == 360 and int(c['frames'].sum()) == 2452712 and guards(b, c['n1'])
    for seed in range(3):
        g = np.random.default_rng(100 + seed)
        dur = c['frames'] * c['ns'] * 1e-3 * g.uniform(0.85, 1.15, size=b)
        changed, order, n1, end_cur, end_new = ops.plan_feedback_plan(dur, c['frames'], c['order'], c['n1'], N_CU, c['em_us'])
        assert sorted(order.tolist()) == list(range(b))
        assert guards(b, n1)
        assert 0.0 < end_new <= end_cur
        if changed:
            # the first part is exactly the n1 largest times (distinct here), both parts longest first
            assert len(set(dur.tolist())) == b
            assert set(order[:n1].tolist()) == set(np.argsort(-dur)[:n1].tolist())
            assert (np.diff(dur[order[:n1]]) <= 0).all() and (np.diff(dur[order[n1:]]) <= 0).all()
        else:
            assert n1 == c['n1'] and (order == c['order']).all() and end_new == end_cur
        # the forced plan has the planner's form whatever it gains
        _, order, n1, _, _ = ops.plan_feedback_plan(dur, c['frames'], c['order'], c['n1'], N_CU, c['em_us'], force=True)
        assert guards(b, n1) and set(order[:n1].tolist()) == set(np.argsort(-dur)[:n1].tolist())


def test_equal_times_leave_the_plan_alone():
    """200 videos on 256 CUs: every video of the rest starts when the emission pass ends, whatever the first part's size, so
    with equal times every plan replays to the same end -- em_us + the common time -- and the plan must stay."""
    from action_segmentation_amd import ops
    g = np.random.default_rng(7)
    b, n1 = 200, 20
    frames = g.integers(500, 14001, size=b).astype(np.int32)
    order = np.argsort(-frames, kind='stable').astype(np.int32)
    dur = np.full(b, 1234.5)
    changed, new_order, new_n1, end_cur, end_new = ops.plan_feedback_plan(dur, frames, order, n1, N_CU, 600.0)
    assert not changed and new_n1 == n1 and (new_order == order).all()
    assert end_cur == end_new == 600.0 + 1234.5


@pytest.mark.parametrize('b, n1, n_cu', [(23, 4, 256), (30, 15, 256), (30, 8, 8), (360, 30, 40)])
def test_a_launch_the_guards_do_not_admit_keeps_its_plan(b, n1, n_cu):
    """Fewer than 24 videos; a first part over a third of the launch with fewer than 16 videos beside it; a first part over
    half of the GPU's CUs."""
    from action_segmentation_amd import ops
    assert not guards(b, n1, n_cu)
    g = np.random.default_rng(b)
    frames = g.integers(100, 5000, size=b).astype(np.int32)
    order = g.permutation(b).astype(np.int32)
    dur = frames * 0.2 * g.uniform(0.85, 1.15, size=b)
    for force in (False, True):
        changed, new_order, new_n1, end_cur, end_new = ops.plan_feedback_plan(dur, frames, order, n1, n_cu, 50.0, force=force)
        assert not changed and new_n1 == n1 and (new_order == order).all() and end_cur == end_new


def test_the_same_input_gives_the_same_plan():
    from action_segmentation_amd import ops
    c = cfg3()
    g = np.random.default_rng(3)
    dur = np.round(c['frames'] * c['ns'] * 1e-3 * g.uniform(0.85, 1.15, size=len(c['frames'])), -1)    # (with ties)
    plans = [ops.plan_feedback_plan(dur, c['frames'], c['order'], c['n1'], N_CU, c['em_us']) for _ in range(3)]
    for p in plans[1:]:
        assert p[0] == plans[0][0] and (p[1] == plans[0][1]).all() and p[2:] == plans[0][2:]


def test_arguments_are_checked():
    from action_segmentation_amd import ops, _lib
    with pytest.raises(_lib.SmmError):
        ops.plan_feedback_plan([1.0, 2.0], [10, 20], [0, 0], 1, N_CU, 1.0)        # not a permutation
