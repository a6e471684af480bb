"""The emission scorer with MIXED class sets in one launch.  The kernel is compiled for the launch's largest class set (NT state
tiles, NG four-state groups behind the first 16 states); the smaller groups of the launch run in that kernel through run-time
clamps -- ng1 < NG, the column clamp of the 4x4x4 operands, c < C on the LDS fill and on the stores, cm - 1 on the constraint
loads.  Every video is compared with the fp64 direct form lognorm - 1/2 sum_d (x - mu)^2 / sigma^2 + cons under ITS group's
parameters (oracle/smm_oracle.c through oracle.factored.emission, group by group), at the tolerances of
test_gpu_viterbi.test_emission_matches_oracle; and nothing may be stored on a frame no video covers or in a column past the
video's class set."""
import functools

import numpy as np
import pytest
import torch

from oracle import factored as F

pytestmark = pytest.mark.gpu

SENTINEL = -7.25

# states per group, c_max, D
SMALL_LAUNCHES = {
    'ng2': ((23, 9, 17, 16, 20, 13), 24, 24),      # NG = 2 kernel with ng1 in {0, 1, 2}, a padded column past every group
    'ng4': ((32, 5, 21, 28, 25), 32, 40),          # NG = 4 with ng1 in {0, 2, 3, 4}
    'nt1_scalar': ((16, 3, 11, 1), 16, 33),        # NT = 1 on the scalar-load path (D % 4 != 0)
    'ng1_scalar': ((19, 7), 19, 17),               # NG = 1 on the scalar-load path
}
PAIR_LAUNCH = ((27, 12, 18), 28, 8)                # >= 131 072 frames, tpw >= 2: pair kernel without constraints, one-tile with


def _layout(g, lengths):
    """The frame axis of test_emission_chain_rule_matches_torch: a leading offset of 3, 0..4 unused frames between videos."""
    gap = g.integers(0, 5, size=len(lengths))
    frame_off = np.concatenate([[0], np.cumsum(lengths + gap)[:-1]]) + 3
    return frame_off, int(frame_off[-1] + lengths[-1] + 2)


@functools.lru_cache(maxsize=None)
def make_launch(name):
    """Inputs of one launch (host arrays; finite values in the gaps and in the padded columns too) and the fp64 reference of
    every video, without and with constraints.  Built once per launch and shared: nothing here is changed by a test."""
    if name == 'pair':
        states, cm, d = PAIR_LAUNCH
        g = np.random.default_rng(2718)
        lengths = g.integers(2800, 3001, size=47)
        lengths[1], lengths[2], lengths[3] = 9, 16 * 181, 16 * 182 + 1             # < 1 tile; 181 and 183 tiles
        group = (np.arange(47) % len(states)).astype(np.int32)
        assert ((lengths[2] + 15) // 16) % 2 == 1 and ((lengths[3] + 15) // 16) % 2 == 1
    else:
        states, cm, d = SMALL_LAUNCHES[name]
        g = np.random.default_rng(sum(states) * 100 + d)
        lengths = np.concatenate([[1, 15, 16, 17, 31, 33], g.integers(100, 301, size=6)])
        lengths = lengths[g.permutation(12)]
        group = (g.permutation(12) % len(states)).astype(np.int32)              # every group at least once
        assert set(group.tolist()) == set(range(len(states)))
    lengths = lengths.astype(np.int64)
    frame_off, total = _layout(g, lengths)
    if name == 'pair':
        assert int(lengths.sum()) >= 131072
    x = g.standard_normal((total, d)).astype(np.float32)
    var = 0.5 + g.random(d)
    lognorm = float(-0.5 * d * np.log(2 * np.pi) - 0.5 * np.log(var).sum())
    mus = [g.standard_normal((c, d)) * 0.5 for c in states]
    cons = ((g.random((total, cm)) < 0.1) * -1e4).astype(np.float32)
    # tables padded to c_max columns; what stands in the padding is never to be read as a state's
    w = np.full((len(states), d, cm), 3.0)
    cst = np.full((len(states), cm), -11.0)
    for gi, (c, mu) in enumerate(zip(states, mus)):
        w[gi, :, :c] = (mu / var).T
        cst[gi, :c] = lognorm - 0.5 * (mu * mu / var).sum(1)
    refs = {}
    for with_cons in (False, True):
        ref = [None] * len(lengths)
        for gi, c in enumerate(states):
            idx = np.flatnonzero(group == gi)
            tg = int(lengths[idx].max())
            xp = np.zeros((len(idx), tg, d), np.float32)
            cn = np.zeros((len(idx), tg, c))
            for j, i in enumerate(idx):
                f0, t = int(frame_off[i]), int(lengths[i])
                xp[j, :t] = x[f0:f0 + t]
                cn[j, :t] = cons[f0:f0 + t, :c]
            e = F.emission(xp, lengths[idx], mus[gi], 1.0 / var, lognorm, cn if with_cons else None)
            for j, i in enumerate(idx):
                ref[i] = e[j, :lengths[i]].copy()
        refs[with_cons] = ref
    return dict(states=states, cm=cm, d=d, lengths=lengths, group=group, frame_off=frame_off, total=total, x=x, inv_var=1.0 / var,
                w=w, cst=cst, cons=cons, refs=refs)


def run_launch(L, with_cons, perm=None):
    """ops.emission with want64 and want32 on; elp64 starts from the sentinel, elp32 from the zeros ops.emission allocates.
    ``perm``: the groups' order in the tables (new group j = old group perm[j]), group[] changed to match."""
    from action_segmentation_amd import ops
    dev = torch.device('cuda:0')
    states, group, w, cst = np.asarray(L['states']), L['group'], L['w'], L['cst']
    if perm is not None:
        perm = np.asarray(perm)
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        states, w, cst, group = states[perm], w[perm], cst[perm], inv[group].astype(np.int32)
    t64 = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    batch = ops.Batch(L['lengths'], states, 4, c_max=L['cm'], frame_offset=L['frame_off'], group=group, t_max=int(L['lengths'].max()),
                      total_frames=L['total'], d=L['d'])
    out64 = torch.full((L['total'], L['cm']), SENTINEL, dtype=torch.float64, device=dev)
    e64, e32 = ops.emission(batch, torch.tensor(L['x'], device=dev), t64(w), t64(cst), t64(L['inv_var']),
                            torch.tensor(L['cons'], device=dev) if with_cons else None, True, True, out64=out64)
    torch.cuda.synchronize()
    assert e64 is out64
    return e64.cpu().numpy(), e32.cpu().numpy()


def check_launch(L, with_cons, e64, e32):
    covered = np.zeros(L['total'], bool)
    for i, t in enumerate(L['lengths']):
        f0, c = int(L['frame_off'][i]), L['states'][L['group'][i]]
        ref = L['refs'][with_cons][i]
        msg = 'video %d: %d frames, %d states' % (i, t, c)
        np.testing.assert_allclose(e64[f0:f0 + t, :c], ref, rtol=1e-12, atol=1e-9, err_msg=msg)
        np.testing.assert_allclose(e32[f0:f0 + t, :c], ref, rtol=2e-7, atol=1e-6, err_msg=msg)
        # no store past the video's class set
        assert (e64[f0:f0 + t, c:] == SENTINEL).all(), msg
        assert (e32[f0:f0 + t, c:] == 0).all(), msg
        covered[f0:f0 + t] = True
    assert not covered.all()
    # ... and none on a frame no video covers
    assert (e64[~covered] == SENTINEL).all()
    assert (e32[~covered] == 0).all()


@pytest.mark.parametrize('with_cons', [False, True])
@pytest.mark.parametrize('name', list(SMALL_LAUNCHES))
def test_emission_of_mixed_groups_matches_oracle(name, with_cons):
    """Twelve videos of 1..300 frames (1, 15, 16, 17, 31, 33: around the 16-frame tile) from up to six parameter groups of
    different sizes in ONE launch, on a frame axis with gaps."""
    L = make_launch(name)
    check_launch(L, with_cons, *run_launch(L, with_cons))


@pytest.mark.parametrize('with_cons', [False, True])
def test_emission_of_mixed_groups_on_pairs_of_tiles_matches_oracle(with_cons):
    """27, 12 and 18 states round-robin over 47 videos of >= 131 072 frames (two tiles per wave): the pair kernel with NG = 3 and
    ng1 in {0, 1, 3} without constraints, the one-tile kernel with them; odd tile counts and a video shorter than a tile."""
    L = make_launch('pair')
    check_launch(L, with_cons, *run_launch(L, with_cons))


@pytest.mark.parametrize('with_cons', [False, True])
def test_emission_does_not_depend_on_the_order_of_the_groups(with_cons):
    """The same launch with the groups' tables in another order (and group[] renamed to match): the same bits, everywhere."""
    L = make_launch('ng2')
    a64, a32 = run_launch(L, with_cons)
    b64, b32 = run_launch(L, with_cons, perm=[3, 5, 0, 2, 1, 4])
    np.testing.assert_array_equal(a64, b64)
    np.testing.assert_array_equal(a32, b32)
