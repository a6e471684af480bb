"""Transcript likelihood with optional entries on the GPU (smm_align_opt_logz_f64 / smm_align_opt_logz_bwd_f64) against
tests/transcript_optional_ref.py.

Bars (tests/test_gpu_transcript.py's): |logZ_o - ref| <= 1e-6 max(1, |ref|); g_elp and p_used within 2e-5 absolute; g_len,
g_trans and g_init within 2e-5 (1 + videos of the group) -- the last two are sums of posteriors over a group's videos here, as
g_len is.  With no flag set: smm_align_logz_*'s values and gradients to 1e-12 (relative to max(1, |value|): the gradients are
probabilities and their sums).  Every reference is computed once per case and shared."""
import functools
import itertools

import numpy as np
import pytest
import torch

import transcript_optional_ref as TO
import train_ref as R

pytestmark = pytest.mark.gpu
Z_BAR, ELP_BAR, LEN_BAR, SAME_BAR, ROW_BAR = 1e-6, 2e-5, 2e-5, 1e-12, 2e-5


def _ops():
    from action_segmentation_amd import ops
    return ops


class Case:
    """A launch: videos (elp [T, C_g], transcript, flags, group), per-group tables, span limits, end penalties, upstream u."""

    def __init__(self, vids, tabs, k_rows, kps=None, endpen=None, u=None):
        self.vids, self.tabs, self.k_rows, self.kps, self.u = vids, tabs, k_rows, kps, u
        self.n_states = [t['init'].shape[0] for t in tabs]
        self.cm = max(self.n_states)
        self.lengths = [v[0].shape[0] for v in vids]
        self.endpen = endpen                                  # [b, cm] numpy or None
        self.off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)

    def kp(self, i):
        return int(self.kps[i]) if self.kps is not None else min(self.k_rows, max(self.lengths))

    def ep(self, i):
        return None if self.endpen is None else self.endpen[i, :self.n_states[self.vids[i][3]]]

    def device_inputs(self):
        ops = _ops()
        dev = torch.device('cuda:0')
        cm, g = self.cm, len(self.tabs)
        elp = np.zeros((int(self.off[-1]), cm))
        for i, v in enumerate(self.vids):
            elp[self.off[i]:self.off[i + 1], :v[0].shape[1]] = v[0]
        trans, init, lens = np.zeros((g, cm, cm)), np.zeros((g, cm)), np.zeros((g, self.k_rows, cm))
        for j, t in enumerate(self.tabs):
            c = self.n_states[j]
            trans[j, :c, :c], init[j, :c], lens[j, :, :c] = t['trans'], t['init'], t['len']
        batch = ops.Batch(self.lengths, self.n_states, self.k_rows, c_max=cm, frame_offset=self.off[:-1],
                          group=[v[3] for v in self.vids], kp=self.kps, total_frames=int(self.off[-1]))
        t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        return batch, dict(elp=t(elp), trans=t(trans), init=t(init), len=t(lens), endpen=t(self.endpen), u=t(self.u))

    def run(self, bwd=True):
        """-> (logZ_o [b], dict of the four gradients and p_used (list per video), numpy; error word)."""
        ops = _ops()
        batch, d = self.device_inputs()
        ids, flags = [v[1] for v in self.vids], [v[2] for v in self.vids]
        out = ops.align_opt_logz(batch, d['elp'], d['trans'], d['init'], d['len'], ids, flags, endpen=d['endpen'])
        err = ops.error_flag(batch, out)
        g = None
        if bwd:
            r = ops.align_opt_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], ids, flags, out['logz'],
                                       grad_logz=d['u'], endpen=d['endpen'], ws=out['ws'], want_entry_prob=True)
            g = {k: r[k].cpu().numpy() for k in ('elp', 'trans', 'init', 'len')}
            g['p_used'] = [p.cpu().numpy() for p in r['entry_prob']]
        return out['logz'].cpu().numpy(), g, err

    def reference(self, route):
        """-> (logZ_o [b], dict(elp [total, cm], trans, init, len [g, ...], p_used list or None)) by ``route`` per video,
        weighted by u and summed."""
        g_n, cm = len(self.tabs), self.cm
        z = np.zeros(len(self.vids))
        g = dict(elp=np.zeros((int(self.off[-1]), cm)), trans=np.zeros((g_n, cm, cm)), init=np.zeros((g_n, cm)),
                 len=np.zeros((g_n, self.k_rows, cm)), p_used=[None] * len(self.vids))
        for i, (e, a, opt, j) in enumerate(self.vids):
            t, c = self.tabs[j], self.n_states[j]
            z[i], gi = route(e, a, opt, t['trans'], t['init'], t['len'], self.kp(i), self.ep(i))
            u = 1.0 if self.u is None else float(self.u[i])
            if not np.isfinite(z[i]):
                g['p_used'][i] = np.zeros(len(a))
                continue
            g['elp'][self.off[i]:self.off[i + 1], :c] = u * gi['elp']
            g['trans'][j, :c, :c] += u * gi['trans']
            g['init'][j, :c] += u * gi['init']
            g['len'][j, :, :c] += u * gi['len']
            g['p_used'][i] = gi.get('p_used')
        return z, g

    def group_sizes(self):
        return np.bincount([v[3] for v in self.vids], minlength=len(self.tabs))


def torch_route(e, a, opt, trans, init, lens, kp, ep):
    """torch_logz_opt's autograd, with p_used from the reference's own forward-backward."""
    z, g = TO.torch_grads_opt(e, a, opt, trans, init, lens, kp, ep)
    if np.isfinite(z):
        g['p_used'] = TO.forward_backward(e, a, opt, trans, init, lens, kp, ep)['p_used']
    return z, g


def _tables(rng, c, k_rows, scale=3.0):
    return dict(trans=rng.normal(size=(c, c)) * scale, init=rng.normal(size=c) * scale, len=rng.normal(size=(k_rows, c)) * scale)


def _check(case, z, g, zr, gr, what):
    fin = np.isfinite(zr)
    assert np.array_equal(np.isfinite(z), fin), (what, z, zr)
    sizes = 1.0 + case.group_sizes()
    err_z = np.abs(z[fin] - zr[fin]) / np.maximum(1.0, np.abs(zr[fin]))
    err_e = np.abs(g['elp'] - gr['elp']).max()
    err_l = (np.abs(g['len'] - gr['len']).max(axis=(1, 2)) / sizes).max()
    err_t = (np.abs(g['trans'] - gr['trans']).max(axis=(1, 2)) / sizes).max()
    err_i = (np.abs(g['init'] - gr['init']).max(axis=1) / sizes).max()
    err_p = 0.0
    for i, (_, a, opt, _) in enumerate(case.vids):
        p = g['p_used'][i]
        assert p.shape == (len(a),)
        if gr['p_used'][i] is not None:
            err_p = max(err_p, float(np.abs(p - gr['p_used'][i]).max()))
        if fin[i]:                                            # a mandatory entry has a segment in every alignment
            mand = ~np.asarray(opt, bool)
            assert np.abs(p[mand] - 1.0).max(initial=0.0) <= ELP_BAR, (what, i)
            assert p.min() >= -ELP_BAR and p.max() <= 1.0 + ELP_BAR, (what, i)
        else:
            assert not p.any(), (what, i)
    print('\n[transcript-opt] %-40s logZ %.2e (bar %.0e)  g_elp %.2e p_used %.2e (%.0e)  g_len %.2e g_trans %.2e g_init %.2e (%.0e)'
          % (what, err_z.max() if err_z.size else 0.0, Z_BAR, err_e, err_p, ELP_BAR, err_l, err_t, err_i, LEN_BAR))
    assert (err_z <= Z_BAR).all(), (what, 'logZ_o', err_z.max())
    assert err_e <= ELP_BAR, (what, 'g_elp', err_e)
    assert err_p <= ELP_BAR, (what, 'p_used', err_p)
    assert err_l <= LEN_BAR, (what, 'g_len', err_l)
    assert err_t <= LEN_BAR, (what, 'g_trans', err_t)
    assert err_i <= LEN_BAR, (what, 'g_init', err_i)


# ------------------------------------------------------------------------------------------------ 1. tiny exhaustive
@functools.lru_cache(None)
def _tiny():
    rng = np.random.default_rng(1)
    T, C, kp = 7, 3, 5
    elp, tab = rng.normal(size=(T, C)) * 2, _tables(rng, C, kp, 1.5)
    seqs = [[2], [0, 1], [0, 1, 0], [0, 0, 0], [1, 0, 0, 1], [2, 1, 1, 2]]   # (0, 0 / 1, 1 inside one optional run: G folds two entries)
    vids = [(elp, a, list(f), 0) for a in seqs for f in itertools.product((0, 1), repeat=len(a))]
    case = Case(vids, [tab], kp)
    brute = [TO.brute_logz_opt(elp, a, f, tab['trans'], tab['init'], tab['len'], kp) for _, a, f, _ in vids]
    return case, brute, case.reference(torch_route)


def test_tiny_every_flag_pattern_against_enumeration():
    """Every flag pattern of six transcripts of 1 - 4 entries over 3 classes on one video of 7 frames, span limit 5, as 62
    videos of one launch: log Z_o, the frame occupancy and p_used against the enumeration over subsets and compositions, the
    launch's gradients against autograd through the torch recursion."""
    case, brute, ref = _tiny()
    assert len(case.vids) == 2 + 4 + 8 + 8 + 16 + 16
    z, g, err = case.run()
    assert err == 0
    n_fin = 0
    for i, ((_, a, f, _), (zb, occ, pu)) in enumerate(zip(case.vids, brute)):
        rows = g['elp'][case.off[i]:case.off[i + 1]]
        if not np.isfinite(zb):
            assert z[i] == -np.inf and not rows.any() and not g['p_used'][i].any(), (a, f)
            continue
        assert abs(z[i] - zb) <= Z_BAR * max(1.0, abs(zb)), (a, f, z[i], zb)
        assert np.abs(rows - occ).max() <= ELP_BAR, (a, f)
        assert np.abs(g['p_used'][i] - pu).max() <= ELP_BAR, (a, f)
        n_fin += 1
    assert n_fin >= 50
    _check(case, z, g, *ref, 'tiny, every flag pattern')


# ------------------------------------------------------------------------------------------------ 2. no flag set
def _ragged(with_endpen, values=0, density=0.0):
    """3 groups of 3, 11 and 32 states, 8 videos with their own span limits (tests/test_gpu_transcript.py's shape); ``values``:
    the seed of the scores alone; ``density``: the share of optional entries."""
    rng, val = np.random.default_rng(77), np.random.default_rng(500 + values)
    n_states, k_rows = [3, 11, 32], 24
    tabs = [_tables(val, c, k_rows) for c in n_states]
    vids, kps = [], []
    for i, (T, j) in enumerate([(5, 0), (90, 2), (33, 1), (61, 0), (17, 2), (48, 1), (24, 2), (80, 1)]):
        kp = int(rng.integers(4, k_rows + 1))
        lo = -(-T // (kp - 1))
        M = int(rng.integers(lo, min(T, lo + 9) + 1))
        a = rng.integers(0, n_states[j], size=M)
        if M >= 3:
            a[1] = a[2] = a[0]                                # consecutive repeats are separate segments
        opt = [bool(v) for v in rng.random(M) < density]
        vids.append((val.normal(size=(T, n_states[j])) * 3, [int(v) for v in a], opt, j))
        kps.append(kp)
    endpen = val.normal(size=(len(vids), 32)) * 2 if with_endpen else None
    u = np.array([1.0, 0.0, -0.75, 2.5, 0.3, 1.0, -1.25, 0.5])
    return Case(vids, tabs, k_rows, kps=kps, endpen=endpen, u=u)


@pytest.mark.parametrize('with_endpen', [False, True])
def test_no_flag_set_is_the_exact_transcript_likelihood(with_endpen):
    """Every flag 0 on a ragged batch: smm_align_logz_f64 / _bwd_f64 on the same inputs, values and all four gradients."""
    ops = _ops()
    case = _ragged(with_endpen)
    z, g, err = case.run()
    batch, d = case.device_inputs()
    out = ops.align_logz_ex(batch, d['elp'], d['trans'], d['init'], d['len'], [v[1] for v in case.vids], endpen=d['endpen'])
    want = ops.align_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], out['transcript'], out['logz'],
                              grad_logz=d['u'], endpen=d['endpen'], ws=out['ws'])
    zw = out['logz'].cpu().numpy()
    assert err == 0 and np.isfinite(zw).all()
    worst = dict(logz=float((np.abs(z - zw) / np.maximum(1.0, np.abs(zw))).max()))
    for k in ('elp', 'trans', 'init', 'len'):
        w = want[k].cpu().numpy()
        worst[k] = float((np.abs(g[k] - w) / np.maximum(1.0, np.abs(w))).max())
    print('\n[transcript-opt] no flag, endpen=%s: %s' % (with_endpen, worst))
    assert all(v <= SAME_BAR for v in worst.values()), worst
    for p in g['p_used']:
        assert np.abs(p - 1.0).max() <= SAME_BAR


# ------------------------------------------------------------------------------------------------ 3. against the existing kernel
def test_unambiguous_transcripts_are_the_lse_over_their_reduced_transcripts():
    """Transcripts with <= 6 optional entries no two subsets of which give the same class sequence: log Z_o = the lse over the
    2^r reduced transcripts of ops.align_logz, run as one batch of replicated videos."""
    ops = _ops()
    rng = np.random.default_rng(31)
    C, K = 6, 9
    tab = _tables(rng, C, K)
    specs = [TO.crosstask([1, 2, 3], 0, True, False),                      # the CrossTask form, backgrounds optional
             TO.crosstask([1, 2, 3, 4, 5], 0, False, True),                # ... steps optional
             ([0, 1, 2, 3, 4, 5, 0, 1], [1, 0, 1, 1, 0, 1, 1, 1]),         # all different within reach
             ([3, 3, 4, 4], [1, 0, 0, 1])]
    vids = []
    for a, f in specs:
        assert sum(f) <= 6 and not TO.is_ambiguous_brute(a, f) and not ops.transcript_is_ambiguous(a, f)
        vids.append((rng.normal(size=(int(rng.integers(20, 31)), C)) * 2, a, [bool(v) for v in f], 0))   # (4 entries of <= 8 frames reach 30)
    endpen = rng.normal(size=(len(vids), C))
    case = Case(vids, [tab], K, endpen=endpen)
    z, _, err = case.run(bwd=False)
    assert err == 0
    # the replicated batch
    rep, owner, ep = [], [], []
    for i, (e, a, f, _) in enumerate(vids):
        for red in TO.reduced_transcripts(a, f):
            rep.append((e, red, [False] * len(red), 0))
            owner.append(i)
            ep.append(endpen[i])
    big = Case(rep, [tab], K, endpen=np.array(ep))
    batch, d = big.device_inputs()
    zr = ops.align_logz(batch, d['elp'], d['trans'], d['init'], d['len'], [v[1] for v in rep], endpen=d['endpen']).cpu().numpy()
    owner = np.array(owner)
    for i in range(len(vids)):
        part = zr[owner == i]
        part = part[np.isfinite(part)]
        want = part.max() + np.log(np.exp(part - part.max()).sum())
        assert abs(z[i] - want) <= Z_BAR * max(1.0, abs(want)), (i, z[i], want)


# ------------------------------------------------------------------------------------------------ 4. tile geometry
@pytest.mark.parametrize('name', ['over_one_tile', 'halo_longer_than_a_tile', 'longest_transcript'])
def test_tile_geometry_against_the_twin(name):
    """T = 771 (a tile of 768 and 3 more), kp = 64, M = 20 with alternating flags; T = 1100, k_rows = 1024 (the halo is longer
    than a tile), M = 3 with the middle entry optional; M = 256, T = 300, kp = 8, every second entry optional."""
    P = _ops().ALIGN_LOGZ_TILE
    T, M, k_rows, flags = {'over_one_tile': (P + 3, 20, 64, [m % 2 for m in range(20)]),
                           'halo_longer_than_a_tile': (1100, 3, 1024, [0, 1, 0]),
                           'longest_transcript': (300, 256, 8, [m % 2 for m in range(256)])}[name]
    rng = np.random.default_rng(1000 + M)
    C = 4
    a = [int(v) for v in rng.integers(0, C, size=M)]
    case = Case([(rng.normal(size=(T, C)) * 2, a, [bool(v) for v in flags], 0)], [_tables(rng, C, k_rows, 2.0)], k_rows)
    z, g, err = case.run()
    assert err == 0
    _check(case, z, g, *case.reference(TO.twin_grads_opt), name)


# ------------------------------------------------------------------------------------------------ 5. runs
@functools.lru_cache(None)
def _runs():
    rng = np.random.default_rng(55)
    C, K = 3, 12
    tab = _tables(rng, C, K, 2.0)
    e = lambda T: rng.normal(size=(T, C)) * 2
    run40 = [int(v) for v in rng.integers(0, C, size=40)]
    vids = [
        # optional runs at both ends: several first(m) and end(j)
        (e(30), [0, 1, 2, 0, 1, 2, 0], [True, True, True, False, True, True, True], 0),
        # a run of 40 optional entries over 3 classes between two mandatory ones
        (e(60), [0] + run40 + [1], [False] + [True] * 40 + [False], 0),
        # two entries of one class whose cones are disjoint (kp = 3: entry 1 ends within [1, 4], entry 7 within [12, 16]),
        # the gap the interval bookkeeping exists for
        (e(16), [0, 1, 2, 2, 0, 2, 0, 1, 2, 0], [True] * 10, 0),
        # everything optional
        (e(25), [2, 1, 0, 1, 2, 0], [True] * 6, 0),
        (e(9), [1, 1, 1], [True] * 3, 0),
    ]
    case = Case(vids, [tab], K, kps=[12, 7, 3, 12, 6], endpen=rng.normal(size=(len(vids), C)), u=np.array([1.0, -0.5, 2.0, 1.0, 0.25]))
    return case, case.reference(TO.twin_grads_opt)


def test_optional_runs_against_the_twin():
    case, ref = _runs()
    z, g, err = case.run()
    assert err == 0 and np.isfinite(z).all()
    _check(case, z, g, *ref, 'runs')


# ------------------------------------------------------------------------------------------------ 6. dynamic range
def test_dynamic_range_against_the_twin():
    """T = 2000, kp = 1024; the elp columns differ by +-50 per frame in runs of 100 - 300 frames, the length scores are Poisson
    log-pmfs with rates 50 - 400 (tests/test_gpu_transcript.py's case), 9 entries of which 5 are optional."""
    rng = np.random.default_rng(5)
    T, C, K = 2000, 4, 1024
    elp = rng.normal(size=(T, C))
    t = 0
    while t < T:
        run = int(rng.integers(100, 301))
        elp[t:t + run] += rng.choice([-50.0, 50.0], size=C)
        t += run
    rates = rng.uniform(50, 400, size=C)
    k = np.arange(K)[:, None]
    tab = dict(trans=rng.normal(size=(C, C)), init=rng.normal(size=C),
               len=k * np.log(rates) - rates - torch.lgamma(torch.arange(K, dtype=torch.float64) + 1).numpy()[:, None])
    a, f = [0, 1, 2, 3, 1, 0, 2, 3, 1], [1, 0, 1, 1, 0, 0, 1, 0, 1]
    case = Case([(elp, a, [bool(v) for v in f], 0)], [tab], K)
    z, g, err = case.run()
    assert err == 0
    _check(case, z, g, *case.reference(TO.twin_grads_opt), 'dynamic range')


# ------------------------------------------------------------------------------------------------ 7. degenerate inputs
def test_degenerate_videos_beside_healthy_ones():
    rng = np.random.default_rng(12)
    C, K = 3, 6
    healthy, holes = _tables(rng, C, K), _tables(rng, C, K)
    holes['trans'][2, 0] = -np.inf                            # kills the subsets that keep 0 directly before 2
    holes['init'][1] = -np.inf
    e = lambda T: rng.normal(size=(T, C)) * 2
    nan_elp = e(10)
    nan_elp[4, 2] = np.nan                                    # in a class its transcript never names
    vids = [(e(14), [0, 1, 2, 1], [0, 1, 0, 1], 0),           # 0 healthy
            (e(3), [0, 1, 0, 1, 2], [0, 0, 1, 0, 0], 0),      # 1 four mandatory entries, three frames
            (e(12), [0, 1], [0, 1], 0),                       # 2 M kw = 10 < T
            (e(9), [0, 7, 1], [0, 1, 0], 0),                  # 3 an id out of range
            (nan_elp, [0, 1, 0], [0, 1, 0], 0),               # 4 NaN in elp
            (e(11), [0, 1, 2, 0], [0, 1, 0, 0], 1),           # 5 trans[2][0] = -inf: only the subsets that keep entry 1 are left
            (e(9), [1, 0, 2], [0, 1, 0], 1),                  # 6 init[1] = -inf kills every subset
            (e(7), [2, 2], [1, 1], 0)]                        # 7 healthy
    u = np.array([1.0, 2.0, 1.0, 1.0, 1.0, 2.0, 1.0, -0.5])
    case = Case(vids, [healthy, holes], K, u=u)
    z, g, err = case.run()
    assert err != 0
    assert np.isfinite(z[[0, 5, 7]]).all() and (z[[1, 2, 3, 6]] == -np.inf).all() and np.isnan(z[4])
    for i in (1, 2, 3, 4, 6):
        assert not g['elp'][case.off[i]:case.off[i + 1]].any() and not g['p_used'][i].any()
    # the reference: the same launch without the video that sets the error word (torch route: it knows -inf)
    vids_ok = [v if i != 4 else (np.zeros((10, C)), [0] * 11, [0] * 11, 0) for i, v in enumerate(vids)]   # (-inf by counting)
    ok = Case(vids_ok, [healthy, holes], K, u=u)
    zr, gr = ok.reference(torch_route)
    assert zr[4] == -np.inf and np.isfinite(zr[5]) and zr[6] == -np.inf
    z2 = np.where(np.isnan(z), -np.inf, z)
    g2 = dict(g, p_used=[p if i != 4 else np.zeros(11) for i, p in enumerate(g['p_used'])])
    _check(ok, z2, g2, zr, gr, 'degenerate beside healthy')
    # the error word alone: without the NaN it stays clear
    _, _, err_ok = Case([v for i, v in enumerate(vids) if i != 4], [healthy, holes], K).run(bwd=False)
    assert err_ok == 0


# ------------------------------------------------------------------------------------------------ 8. determinism
def test_two_calls_give_the_same_bits():
    case = _ragged(True, density=0.5)
    z1, g1, _ = case.run()
    z2, g2, _ = case.run()
    assert np.isfinite(z1).all() and np.array_equal(z1, z2)
    for k in ('elp', 'trans', 'init', 'len'):
        assert np.array_equal(g1[k], g2[k]), k
    assert all(np.array_equal(p, q) for p, q in zip(g1['p_used'], g2['p_used']))


def test_a_ragged_batch_with_flags_against_both_references():
    case = _ragged(True, density=0.5)
    z, g, err = case.run()
    assert err == 0
    _check(case, z, g, *case.reference(torch_route), 'ragged with flags vs torch')
    _check(case, z, g, *case.reference(TO.twin_grads_opt), 'ragged with flags vs twin')
    batch, d = case.device_inputs()
    best = _ops().align_optional(batch, d['elp'], d['trans'], d['init'], d['len'], [v[1] for v in case.vids],
                                 [v[2] for v in case.vids], endpen=d['endpen'])['best'].cpu().numpy()
    assert (best <= z + 1e-9 * np.maximum(1.0, np.abs(z))).all()


# ------------------------------------------------------------------------------------------------ 9. module and model
def _module_case(seed=3, n=6, d=8, k=12, lengths=(40, 25, 33)):
    from module_util import make_args
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    m = SemiMarkovModule(make_args(k), n, d, allow_self_transitions=True)
    mu = rng.normal(0, 1.0, size=(n, d))
    with torch.no_grad():
        m.gaussian_means.copy_(torch.as_tensor(mu, dtype=torch.float32))
        m.gaussian_cov.copy_(torch.diag(torch.as_tensor(rng.uniform(0.7, 1.3, size=d), dtype=torch.float32)))
        m.transition_logits.copy_(torch.randn(n, n, generator=gen))
        m.init_logits.copy_(torch.randn(n, generator=gen))
        m.poisson_log_rates.copy_(torch.log(torch.rand(n, generator=gen) * 8 + 3))
    vc = [4, 0, 2, 5]
    tmax = max(lengths)
    x = np.zeros((len(lengths), tmax, d), np.float32)
    transcripts, optional = [], []
    for i, t in enumerate(lengths):
        M = int(rng.integers(-(-t // (k - 1)) + 2, 9))
        opt = [bool(m % 3 == 1) for m in range(M)]
        while True:                                           # (log_likelihood keeps ambiguous='raise')
            a = [vc[int(v)] for v in rng.integers(0, len(vc), size=M)]
            if not TO.is_ambiguous_brute(a, opt):
                break
        cuts = np.sort(rng.choice(np.arange(1, t), size=M - 1, replace=False))
        lab = np.repeat(np.array(a), np.diff(np.concatenate([[0], cuts, [t]])))
        x[i, :t] = mu[lab] + rng.standard_normal((t, d))
        transcripts.append(a)
        optional.append(opt)
    rb = R.RefBatch(x, list(lengths), vc)
    return m.cuda(), rb, vc, transcripts, optional


@pytest.mark.parametrize('discriminative', [False, True])
def test_module_values_and_parameter_gradients(discriminative):
    """transcript_log_partition(optional=...) and log_likelihood(transcripts=..., transcript_optional=...) against autograd
    through torch_logz_opt on train_ref's tables; discriminative: minus log Z, held to the size of its two parts."""
    m, rb, vc, transcripts, optional = _module_case()
    m.args.sm_train_discriminatively = discriminative
    dev = torch.device('cuda:0')
    x, lengths, vcs = rb.features.to(dev), rb.lengths.to(dev), [rb.valid_classes] * len(transcripts)
    q, leaves = R.params_from_module(m)
    trans, init, lens, merged = R.tables(q, rb.valid_classes)
    elp = R.emission(q, merged, rb)
    kp = R.kp_of(lens, rb)
    loc = {c: j for j, c in enumerate(vc)}
    za = torch.stack([TO.torch_logz_opt(elp[i, :int(t)], [loc[c] for c in transcripts[i]], optional[i], trans, init, lens, kp)
                      for i, t in enumerate(rb.lengths.tolist())])
    value = za.mean().item()
    ref = R.grads(leaves, za.mean())
    models = None
    if discriminative:
        zl = R.logz_factored(q, rb)
        value -= zl.mean().item()
        gl = R.grads(leaves, zl.mean())
        models = {n: dict(size=np.abs(ref[n]) + np.abs(gl[n])) for n in ref}
        ref = {n: ref[n] - gl[n] for n in ref}
    z = m.transcript_log_partition(x, lengths, vcs, transcripts, optional=optional, ambiguous='allow')
    assert z.dtype == torch.float64 and z.requires_grad
    np.testing.assert_allclose(z.detach().cpu().numpy(), za.detach().numpy(), rtol=Z_BAR)
    m.zero_grad()
    ll, _ = m.log_likelihood(x, lengths, vcs, transcripts=transcripts, transcript_optional=optional)
    ll.backward()
    assert abs(ll.item() - value) <= Z_BAR * max(1.0, abs(za.mean().item()))
    got = R.module_grads(m)
    assert all(np.abs(v).max() > 0 for v in got.values())
    R.assert_grads_close(got, ref, ROW_BAR, 'transcript optional discriminative=%s' % discriminative, models)


def test_packed_and_model_layers():
    """The packed and model layers on the tiny synthetic corpus with each video's Viterbi transcript in the CrossTask reading
    (``optional_classes``: every entry of those classes may be missing): log Z_o >= the best optional alignment and >= log Z_a
    of the full transcript; the entry posteriors are 1 on mandatory entries, within [0, 1] elsewhere and the reference's;
    ambiguous='raise' names the video, 'allow' computes."""
    from action_segmentation_amd import ops, synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts
    data = synth.SynthDatasplit('tiny', seed=11)
    fitted = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    fitted.fit(data, use_labels=True)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=True, batch_size=2), data)
    model.model.load_state_dict(fitted.model.state_dict(), strict=False)
    mod = model.model.cuda()
    pc = model.prepare(data)
    t = pc.tables
    elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
    out = ops.viterbi(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    tr = [np.asarray(a, np.int64) for a in spans_to_transcripts(out['spans'], pc.lengths)]
    by_video = dict(zip(pc.video_names, tr))
    # one optional entry per video: the second (no two subsets of one optional entry agree unless the neighbours repeat)
    flags = [np.arange(len(a)) == 1 for a in tr]
    flags_by_video = dict(zip(pc.video_names, flags))
    assert not any(ops.transcript_is_ambiguous(a, f) for a, f in zip(tr, flags))
    za = mod.transcript_log_partition_packed(pc, tr).detach().cpu().numpy()
    zo = mod.transcript_log_partition_packed(pc, tr, optional=flags)
    assert zo.requires_grad and zo.dtype == torch.float64 and zo.shape == (len(tr),)
    zoh = zo.detach().cpu().numpy()
    _, best = mod.align_packed(pc, tr, optional=flags)
    best = best.cpu().numpy()
    tol = 1e-9 * np.maximum(1.0, np.abs(zoh))
    assert np.isfinite(zoh).all() and (best <= zoh + tol).all() and (za <= zoh + tol).all()
    mod.zero_grad()
    zo.sum().backward()
    assert all(getattr(mod, n).grad is not None and bool(getattr(mod, n).grad.abs().max() > 0) for n in R.PARAMS)
    scores = mod.transcript_scores_packed(pc, tr, optional=flags).numpy()
    assert np.abs(scores - zoh).max() <= 1e-9 * np.abs(zoh).max()
    got = model.transcript_log_likelihood(data, by_video, optional_by_video=flags_by_video, ambiguous='allow')
    for i, n in enumerate(pc.video_names):
        assert abs(got[n] - zoh[i]) <= 1e-9 * max(1.0, abs(zoh[i])), n
    # entry posteriors: the reference's own forward-backward on the same tables
    post = mod.transcript_entry_posteriors_packed(pc, tr, flags, ambiguous='allow')
    by_name = model.transcript_entry_posteriors(data, by_video, optional_by_video=flags_by_video, ambiguous='allow')
    elp_h, cmap = elp.cpu().numpy(), t['class_map'].cpu().numpy()
    tabs = [v.detach().cpu().numpy() for v in (t['trans'], t['init'], t['len'])]
    group = pc.batch.group if pc.batch.group is not None else np.zeros(pc.batch.b, np.int64)
    ep = None if pc.endpen is None else pc.endpen.cpu().numpy()
    for i, n in enumerate(pc.video_names):
        p = post[i]
        assert p.dtype == np.float64 and p.shape == (len(tr[i]),) and np.array_equal(p, by_name[n])
        assert np.abs(p[~flags[i]] - 1.0).max() <= ELP_BAR and p.min() >= -ELP_BAR and p.max() <= 1.0 + ELP_BAR
        gi, c = int(group[i]), int(pc.batch.n_states[group[i]])
        loc = {int(v): j for j, v in enumerate(cmap[gi, :c])}
        f0, T = int(pc.batch.frame_offset[i]), int(pc.batch.lengths[i])
        kp = int(pc.batch.kp[i]) if pc.batch.kp is not None else min(pc.batch.shape.k_rows, pc.batch.shape.t_max)
        fb = TO.forward_backward(elp_h[f0:f0 + T, :c], [loc[int(v)] for v in tr[i]], flags[i], tabs[0][gi, :c, :c], tabs[1][gi, :c],
                                 tabs[2][gi, :, :c], kp, None if ep is None else ep[i, :c])
        assert abs(fb['logz'] - zoh[i]) <= Z_BAR * max(1.0, abs(zoh[i])), n
        assert np.abs(p - fb['p_used']).max() <= ELP_BAR, n
    # ambiguous='raise': a transcript two subsets of which agree is refused by name before anything is launched
    k = int(np.argmax([len(a) for a in tr]))
    bad_t, bad_f = list(tr), list(flags)
    bad_t[k] = np.array([tr[k][0], tr[k][1], tr[k][0]], np.int64)                # [x?, y?, x?]
    bad_f[k] = np.array([True, True, True])
    with pytest.raises(ValueError, match=str(pc.video_names[k])):
        mod.transcript_log_partition_packed(pc, bad_t, optional=bad_f)
    with pytest.raises(ValueError, match=str(pc.video_names[k])):
        model.transcript_log_likelihood(data, dict(zip(pc.video_names, bad_t)), optional_by_video=dict(zip(pc.video_names, bad_f)))
    z_allow = mod.transcript_scores_packed(pc, bad_t, optional=bad_f, ambiguous='allow').numpy()
    others = [i for i in range(len(tr)) if i != k]
    assert np.abs(z_allow[others] - zoh[others]).max() <= 1e-9 * np.abs(zoh).max() and not np.isnan(z_allow[k])


# ------------------------------------------------------------------------------------------------ 10. stream capture
def test_forward_and_backward_capture_into_a_hip_graph():
    """The pair captured once with ``staged=`` and replayed twice on fresh inputs of the ragged shape: every replay reproduces
    the eager call on those inputs bit for bit."""
    ops = _ops()
    case = _ragged(True, density=0.5)
    batch, d = case.device_inputs()
    ids, flags = [v[1] for v in case.vids], [v[2] for v in case.vids]
    _, off = ops._transcript_arrays(batch, ids)
    ws = torch.empty(ops.align_opt_logz_workspace_bytes(batch, off), dtype=torch.uint8, device='cuda:0')
    staged = ops.align_opt_logz(batch, d['elp'], d['trans'], d['init'], d['len'], ids, flags, endpen=d['endpen'], ws=ws)['_staged']

    def step():
        z = ops.align_opt_logz(batch, d['elp'], d['trans'], d['init'], d['len'], ids, flags, endpen=d['endpen'], ws=ws,
                               staged=staged)['logz']
        g = ops.align_opt_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], ids, flags, z, grad_logz=d['u'],
                                   endpen=d['endpen'], ws=ws, staged=staged, want_entry_prob=True)
        return z, g['elp'], g['trans'], g['init'], g['len'], torch.cat(g['entry_prob'])

    step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for rep in (1, 2):
        fresh = _ragged(True, values=rep, density=0.5)
        _, f = fresh.device_inputs()
        for k in ('elp', 'trans', 'init', 'len', 'endpen'):
            d[k].copy_(f[k])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [v.clone() for v in out]
        eager = step()
        torch.cuda.synchronize()
        for name, a, e in zip(('logz', 'g_elp', 'g_trans', 'g_init', 'g_len', 'p_used'), got, eager):
            assert torch.equal(a, e), (rep, name)
        assert bool(torch.isfinite(got[0]).all())
