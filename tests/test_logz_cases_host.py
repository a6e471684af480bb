"""The premise of test_gpu_logz_grid.py, on the host: the planted lattices of tests/logz_cases.py keep their posterior mass on
the segment lengths that smm_logz_kernel's chain wave does NOT evaluate (k > K0: the pusher waves' rings forward,
smm_glen_kernel's tiles backward), for every state and up to the longest slot -- asserted from the C twin alone, so that a
kernel with a dead, mis-rotated or mis-indexed ring could not pass the GPU test's bars.  Also asserted: the blind spot itself
(an i.i.d. normal lattice puts nothing there), and that the case table covers what it claims to cover."""
import numpy as np
import pytest

import logz_cases as L

RING_CASES = tuple(cs['name'] for cs in L.CASES if not cs['edge'])


@pytest.fixture(scope='module')
def at_upstream_one():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = L.twin(L.planted(name), np.ones(4))
        return cache[name]
    return get


@pytest.mark.parametrize('name', RING_CASES)
def test_posterior_mass_lies_on_the_rings(at_upstream_one, name):
    p = L.planted(name)
    kp, c, K0 = p['k'], p['c'], L.k0(p['k'])
    z, g = at_upstream_one(name)
    g_len = g['len']
    assert g_len.shape == (kp, c)
    assert g_len[K0 + 1:].sum() >= 0.3 * g_len.sum()                           # mass beyond the chain wave
    assert (g_len[K0 + 1:].sum(0) >= 0.05).all(), g_len[K0 + 1:].sum(0)        # every state's ring carries mass
    assert g_len[kp - 1].max() >= 0.05                                          # the longest slot
    assert g_len[kp // 2:].sum() >= 1.0                                         # the upper half
    # a dead ring moves log Z by at least a nat per video (the videos of at most K0 positions have no ring length to lose)
    dead = L.twin(p, lens=L.dead_ring_table(p), grad=False)
    reach = p['dp_lengths'] > K0
    assert reach.sum() >= 3
    assert (z[reach] - dead[reach] >= 1.0).all(), z - dead
    np.testing.assert_array_equal(dead[~reach], z[~reach])


@pytest.mark.parametrize('name', L.CASE_NAMES)
def test_planted_videos_are_what_the_table_claims(name):
    cs, p = L.case(name), L.planted(name)
    kp, c = cs['kp'], cs['c']
    t = p['dp_lengths']
    assert len(t) == 4 and set(int(x) % 4 for x in t) == {0, 1, 2, 3}          # every block tail
    assert (p['lengths'] >= (2 if p['no_eos'] else 1)).all()
    if not cs['edge']:
        assert (t[2:] < kp).all()                                              # two videos shorter than the span limit
        assert (t[:2] > kp).all()
        for y in p['labels'][:2]:
            assert set(y.tolist()) == set(range(c))                            # every state in every long video
        runs = [n for s, n in p['segs'][0]]
        assert runs.count(kp - 1) == 1                                         # video 0: one segment of exactly kp - 1
    for want, got in zip((cs['t_long'] or (None, None)) + (cs['t_short'] or (None, None)), t):
        assert want is None or want == got                                     # the named lengths are the DP's
    assert p['lens'].shape == (kp, c) and np.isfinite(p['lens'][1:]).all()


def test_the_table_covers_the_grid():
    ring = [cs for cs in L.CASES if not cs['edge']]
    seen = set(L.instantiation(cs['kp'], cs['c']) for cs in ring)
    assert seen == L.ALL_INSTANTIATIONS and len(seen) == 30
    by = lambda f: {key: set(cs['eos'] for cs in ring if f(cs) == key) for key in set(map(f, ring))}
    assert all(v == set(L.EOS_MODES) for v in by(lambda cs: L.ring_regs(cs['kp'])).values())       # every R, every class:
    assert all(v == set(L.EOS_MODES) for v in by(lambda cs: (L.spw(cs['c']), L.hf(cs['c']))).values())   # all three closings
    for lo, hi in L.STATE_CLASSES:
        assert set(L.ring_regs(cs['kp']) for cs in ring if cs['c'] == hi) == set(L.RINGS)
        assert len(set(L.ring_regs(cs['kp']) for cs in ring if cs['c'] == lo)) >= 2
    kps = set(cs['kp'] for cs in L.CASES)
    assert {64, 65, 128, 129, 256, 257, 512, 513, 1024} <= kps                 # ring-size boundaries
    assert {2, 5, 9} <= kps                                                     # no (or hardly a) ring length
    assert {33, 34, 65, 66, 129, 130, 257, 258, 514, 770} <= kps               # smm_glen's tiles: kp - 1 on both sides of each
    ts = set(int(t) for cs in L.CASES for t in L.planted(cs['name'])['dp_lengths'])
    assert {31, 33, 511, 512, 513, 1024, 1025} <= ts                            # marginals' slabs and chunks
    for b in (2, 4):                                                            # one to three positions, per block size
        tiny = set(int(t) for cs in ring if L.block(cs['kp']) == b for t in L.planted(cs['name'])['dp_lengths'] if t <= 3)
        assert tiny == {1, 2, 3}, (b, tiny)
    for name in L.CASE_NAMES:
        up = L.upstream(name)
        assert (up == 0).any() and (up < 0).any()


def test_rings_wrap_in_every_instantiation():
    """T past 64 R plus two blocks: some case of every instantiation has a long video whose ring wraps."""
    wraps = set()
    for cs in L.CASES:
        t = L.planted(cs['name'])['dp_lengths']
        if t.max() > 64 * L.ring_regs(cs['kp']) + 2 * L.block(cs['kp']):
            wraps.add(L.instantiation(cs['kp'], cs['c']))
    assert wraps == L.ALL_INSTANTIATIONS


def test_iid_normal_lattices_never_reach_the_rings():
    """The blind spot the grid closes: test_gpu_viterbi.make_problem (i.i.d. normal emissions, transitions and length rows) at two
    videos, T = 1100, 23 states, K = 1024, scale 1.5, with the seed test_log_partition_gradients_match_oracle would give the
    shape -- of more than a thousand expected segments, fewer than 1e-6 are longer than the 8 lengths the chain wave evaluates
    itself, and none reaches the upper half of the ring.  (Seeds 0..5: 5e-9 .. 3e-5.)  These shapes are no ring coverage."""
    from test_gpu_viterbi import make_problem
    shape = (2, 1100, 23, 1024)
    p = make_problem(hash(shape) % 1000 + 11, *shape, scale=1.5)
    _, grad = L.F.logz(p['elp'], p['lengths'], p['trans'], p['init'], p['lens'], None, grad=True, upstream=np.ones(2))
    assert grad['len'].sum() > 1000
    assert grad['len'][9:].sum() < 1e-6
    assert grad['len'][512:].sum() < 1e-20


@pytest.mark.parametrize('name', L.MIXED_NAMES)
def test_mixed_launches_are_what_the_table_claims(name):
    m = L.mixed(name)
    big, small = m['states']
    kp_max = int(m['kp'].max())
    assert kp_max == m['k'] and m['c_max'] >= big > small
    assert m['c_max'] > big or big == 32                                       # padded columns (the library stops at 32)
    assert (L.spw(big), L.hf(big)) != (L.spw(small), L.hf(small))              # the smaller group rides in another kernel's
    assert m['kp'].min() <= L.k0(kp_max) + 1                                   # a video without a ring length beside kp_max
    np.testing.assert_array_equal(m['frame_offset'][1:], np.cumsum(m['lengths'])[:-1])   # packed
    assert sorted(i for part in m['parts'] for i in part['videos']) == list(range(len(m['lengths'])))
    z, g, _ = L.mixed_reference(name)
    assert np.isfinite(z).all()
    K0 = L.k0(kp_max)
    for gi, c in enumerate(m['states']):                                        # both groups' rings carry mass in every state
        assert (np.abs(g['len'][gi, K0 + 1:, :c]).sum(0) >= 0.05).all()
