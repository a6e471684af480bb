"""Transcript likelihood on the GPU (smm_align_logz_f64 / smm_align_logz_bwd_f64) against tests/transcript_ref.py.

Bars (the project's own for the log-partition path): |logZ_a - ref| <= 1e-6 max(1, |ref|); g_elp within 2e-5 absolute; g_len
within 2e-5 (1 + videos of the group); g_trans and g_init equal the counts times u to 1e-12 relative; parameter gradients through
the module by train_ref.assert_rows_close at 2e-5.  Every reference is computed once per case and shared."""
import functools
import itertools

import numpy as np
import pytest
import torch

import transcript_ref as TR
import train_ref as R

pytestmark = pytest.mark.gpu
Z_BAR, ELP_BAR, LEN_BAR, COUNT_BAR, ROW_BAR = 1e-6, 2e-5, 2e-5, 1e-12, 2e-5


def _ops():
    from action_segmentation_amd import ops
    return ops


def _tile():
    return _ops().ALIGN_LOGZ_TILE


class Case:
    """A launch: videos (elp [T, C_g], transcript, group), per-group tables, span limits, end penalties, upstream u."""

    def __init__(self, vids, tabs, k_rows, kps=None, endpen=None, u=None):
        self.vids, self.tabs, self.k_rows, self.kps, self.u = vids, tabs, k_rows, kps, u
        self.n_states = [t['init'].shape[0] for t in tabs]
        self.cm = max(self.n_states)
        self.lengths = [v[0].shape[0] for v in vids]
        self.endpen = endpen                                  # [b, cm] numpy or None
        self.off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)

    def kp(self, i):
        return int(self.kps[i]) if self.kps is not None else min(self.k_rows, max(self.lengths))

    def closing(self, i):
        return 0.0 if self.endpen is None else float(self.endpen[i, self.vids[i][1][-1]])

    def device_inputs(self):
        ops = _ops()
        dev = torch.device('cuda:0')
        b, cm, g = len(self.vids), self.cm, len(self.tabs)
        elp = np.zeros((int(self.off[-1]), cm))
        for i, (e, _, _) in enumerate(self.vids):
            elp[self.off[i]:self.off[i + 1], :e.shape[1]] = e
        trans, init, lens = np.zeros((g, cm, cm)), np.zeros((g, cm)), np.zeros((g, self.k_rows, cm))
        for j, t in enumerate(self.tabs):
            c = self.n_states[j]
            trans[j, :c, :c], init[j, :c], lens[j, :, :c] = t['trans'], t['init'], t['len']
        batch = ops.Batch(self.lengths, self.n_states, self.k_rows, c_max=cm, frame_offset=self.off[:-1],
                          group=[v[2] for v in self.vids], kp=self.kps, total_frames=int(self.off[-1]))
        t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        return batch, dict(elp=t(elp), trans=t(trans), init=t(init), len=t(lens), endpen=t(self.endpen), u=t(self.u))

    def run(self, bwd=True):
        """-> (logZ_a [b], dict of the four gradients (numpy), error word)."""
        ops = _ops()
        batch, d = self.device_inputs()
        out = ops.align_logz_ex(batch, d['elp'], d['trans'], d['init'], d['len'], [v[1] for v in self.vids], endpen=d['endpen'])
        err = ops.error_flag(batch, out)
        g = None
        if bwd:
            g = ops.align_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], out['transcript'], out['logz'],
                                   grad_logz=d['u'], endpen=d['endpen'], ws=out['ws'])
            g = {k: v.cpu().numpy() for k, v in g.items()}
        return out['logz'].cpu().numpy(), g, err

    def reference(self, route):
        """-> (logZ_a [b], dict(elp [total, cm], trans, init, len [g, ...])) by ``route`` per video, weighted by u and summed."""
        g_n, cm = len(self.tabs), self.cm
        z = np.zeros(len(self.vids))
        g = dict(elp=np.zeros((int(self.off[-1]), cm)), trans=np.zeros((g_n, cm, cm)), init=np.zeros((g_n, cm)),
                 len=np.zeros((g_n, self.k_rows, cm)))
        for i, (e, a, j) in enumerate(self.vids):
            t, c = self.tabs[j], self.n_states[j]
            z[i], gi = route(e, a, t['trans'], t['init'], t['len'], self.kp(i), self.closing(i))
            u = 1.0 if self.u is None else float(self.u[i])
            if not np.isfinite(z[i]):
                continue
            g['elp'][self.off[i]:self.off[i + 1], :c] = u * gi['elp']
            g['trans'][j, :c, :c] += u * gi['trans']
            g['init'][j, :c] += u * gi['init']
            g['len'][j, :, :c] += u * gi['len']
        return z, g

    def group_sizes(self):
        return np.bincount([v[2] for v in self.vids], minlength=len(self.tabs))


def _tables(rng, c, k_rows, scale=3.0):
    return dict(trans=rng.normal(size=(c, c)) * scale, init=rng.normal(size=c) * scale, len=rng.normal(size=(k_rows, c)) * scale)


def _check(case, z, g, zr, gr, what):
    fin = np.isfinite(zr)
    assert np.array_equal(np.isfinite(z), fin), (what, z, zr)
    err_z = np.abs(z[fin] - zr[fin]) / np.maximum(1.0, np.abs(zr[fin]))
    err_e = np.abs(g['elp'] - gr['elp']).max()
    err_l = (np.abs(g['len'] - gr['len']).max(axis=(1, 2)) / (1.0 + case.group_sizes())).max()
    # g_trans and g_init are counts times u: held to the exact counts, not to a reference's posterior sums
    want_t, want_i = np.zeros_like(g['trans']), np.zeros_like(g['init'])
    for i, (_, a, j) in enumerate(case.vids):
        if fin[i]:
            c = case.n_states[j]
            tr, st, _ = TR.counts(a, c)
            u = 1.0 if case.u is None else float(case.u[i])
            want_t[j, :c, :c] += u * tr
            want_i[j, :c] += u * st
    assert np.abs(gr['trans'] - want_t).max() <= 1e-9 and np.abs(gr['init'] - want_i).max() <= 1e-9, what
    err_t = np.abs(g['trans'] - want_t).max() / max(np.abs(want_t).max(), 1.0)
    err_i = np.abs(g['init'] - want_i).max() / max(np.abs(want_i).max(), 1.0)
    print('\n[transcript] %-44s logZ %.2e (bar %.0e)  g_elp %.2e (%.0e)  g_len %.2e (%.0e)  g_trans %.1e  g_init %.1e'
          % (what, err_z.max() if err_z.size else 0.0, Z_BAR, err_e, ELP_BAR, err_l, LEN_BAR, err_t, err_i))
    assert (err_z <= Z_BAR).all(), (what, 'logZ_a', err_z.max())
    assert err_e <= ELP_BAR, (what, 'g_elp', err_e)
    assert err_l <= LEN_BAR, (what, 'g_len', err_l)
    assert err_t <= COUNT_BAR and err_i <= COUNT_BAR, (what, 'counts', err_t, err_i)


# ------------------------------------------------------------------------------------------------ a. tiny exhaustive
@functools.lru_cache(None)
def _tiny():
    rng = np.random.default_rng(1)
    T, C, kp = 6, 2, 4
    elp, tab = rng.normal(size=(T, C)) * 2, _tables(rng, C, kp, 1.5)
    seqs = [list(a) for M in range(1, T + 1) for a in itertools.product(range(C), repeat=M)]
    case = Case([(elp, a, 0) for a in seqs], [tab], kp)
    brute = [TR.brute_logz(elp, a, tab['trans'], tab['init'], tab['len'], kp) for a in seqs]
    return case, seqs, brute


def test_tiny_exhaustive_against_enumeration():
    """All 126 transcripts of 1 - 6 entries over 2 classes on one video of 6 frames, span limit 4, as 126 videos of one launch."""
    ops = _ops()
    case, seqs, brute = _tiny()
    assert len(seqs) == 126
    z, g, err = case.run()
    assert err == 0
    n_ok = 0
    for i, (a, (zb, occ)) in enumerate(zip(seqs, brute)):
        rows = g['elp'][case.off[i]:case.off[i + 1]]
        if len(a) == 1:                                       # one segment of at most 3 frames cannot cover 6
            assert z[i] == -np.inf and not rows.any()
            continue
        assert abs(z[i] - zb) <= Z_BAR * max(1.0, abs(zb)), (a, z[i], zb)
        assert np.abs(rows - occ).max() <= ELP_BAR, a
        n_ok += 1
    assert n_ok == 124
    # every segmentation of the video has exactly one of the transcripts
    one = Case(case.vids[:1], case.tabs, case.k_rows)
    batch, d = one.device_inputs()
    z_all = float(ops.logz(batch, d['elp'], d['trans'], d['init'], d['len']).cpu()[0])
    fin = z[np.isfinite(z)]
    lse = fin.max() + np.log(np.exp(fin - fin.max()).sum())
    assert abs(lse - z_all) <= Z_BAR * max(1.0, abs(z_all)), (lse, z_all)
    # g_trans, g_init, g_len of the launch: the 124 videos' references summed
    zr, gr = case.reference(TR.torch_grads)
    _check(case, z, g, zr, gr, 'tiny exhaustive')


# ------------------------------------------------------------------------------------------------ b. one alignment only
@pytest.mark.parametrize('T,M,kp', [(9, 9, 5), (6, 1, 7), (12, 3, 5)])
def test_a_single_alignment_is_the_alignment(T, M, kp):
    """M = T, M = 1 with T = kp - 1, M (kp - 1) = T: the sum has one term, the best alignment."""
    ops = _ops()
    rng = np.random.default_rng(T * 100 + M)
    C = 3
    a = [int(v) for v in rng.integers(0, C, size=M)]
    case = Case([(rng.normal(size=(T, C)) * 2, a, 0)], [_tables(rng, C, kp)], kp, kps=[kp])
    z, g, err = case.run()
    batch, d = case.device_inputs()
    al = ops.align(batch, d['elp'], d['trans'], d['init'], d['len'], [a])
    best, labels = float(al['best'].cpu()[0]), al['labels'].cpu().numpy()
    assert err == 0 and abs(z[0] - best) <= 1e-12 * max(1.0, abs(best))
    onehot = np.zeros((T, C))
    onehot[np.arange(T), labels] = 1.0
    assert np.abs(g['elp'] - onehot).max() <= 1e-12
    want = np.zeros((kp, C))
    seg = T // M
    for c in a:
        want[seg, c] += 1.0
    assert np.abs(g['len'][0] - want).max() <= 1e-12
    tr, st, _ = TR.counts(a, C)
    assert np.abs(g['trans'][0] - tr).max() <= 1e-12 and np.abs(g['init'][0] - st).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ c. random ragged batches
def _ragged(with_endpen, values=0):
    """3 groups of 3, 11 and 32 states, 8 videos with their own span limits; ``values``: the seed of the scores alone (the
    shape -- lengths, span limits, transcripts -- does not depend on it)."""
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
        vids.append((val.normal(size=(T, n_states[j])) * 3, [int(v) for v in a], j))
        kps.append(kp)
    endpen = val.normal(size=(len(vids), 32)) * 2 if with_endpen else None
    u = np.array([1.0, 0.0, -0.75, 2.5, 0.3, 1.0, -1.25, 0.5])
    return Case(vids, tabs, k_rows, kps=kps, endpen=endpen, u=u)


@functools.lru_cache(None)
def _ragged_refs(with_endpen):
    case = _ragged(with_endpen)
    return case, case.reference(TR.torch_grads), case.reference(TR.twin_grads)


@pytest.mark.parametrize('with_endpen', [False, True])
def test_random_ragged_batches_bounds_identities_and_both_references(with_endpen):
    ops = _ops()
    case, ref_torch, ref_twin = _ragged_refs(with_endpen)
    z, g, err = case.run()
    assert err == 0
    batch, d = case.device_inputs()
    best = ops.align(batch, d['elp'], d['trans'], d['init'], d['len'], [v[1] for v in case.vids],
                     endpen=d['endpen'])['best'].cpu().numpy()
    assert (best <= z + 1e-9 * np.maximum(1.0, np.abs(z))).all()
    for i in range(len(case.vids)):                           # every frame lies in exactly one segment
        rows = g['elp'][case.off[i]:case.off[i + 1]]
        assert np.abs(rows.sum(1) - case.u[i]).max() <= ELP_BAR
    for j, c in enumerate(case.n_states):                     # every entry has exactly one length
        want = np.zeros(case.cm)
        for i, (_, a, jj) in enumerate(case.vids):
            if jj == j:
                want[:c] += case.u[i] * TR.counts(a, c)[2]
        assert np.abs(g['len'][j].sum(0) - want).max() <= LEN_BAR * (1 + case.group_sizes()[j])
    _check(case, z, g, *ref_torch, 'ragged endpen=%s vs torch' % with_endpen)
    _check(case, z, g, *ref_twin, 'ragged endpen=%s vs twin' % with_endpen)


# ------------------------------------------------------------------------------------------------ d. tile edges
def _edge_case(T, M, k_rows, C=4, seed=0):
    rng = np.random.default_rng(1000 + seed)
    a = [int(v) for v in rng.integers(0, C, size=M)]
    return Case([(rng.normal(size=(T, C)) * 2, a, 0)], [_tables(rng, C, k_rows, 2.0)], k_rows)


def test_tile_edge_T_just_over_a_tile_M5_kp64_has_no_path_by_counting():
    """T = P + 37, M = 5, kp = 64 as the issue states it: 5 segments of at most 63 frames cannot cover P + 37 > 315 frames, so
    by the definition the video gets -inf, zero gradients and a clear error word (the twin has no -inf to compare with)."""
    case = _edge_case(_tile() + 37, 5, 64)
    z, g, err = case.run()
    assert err == 0 and z[0] == -np.inf and all(not v.any() for v in g.values())
    assert TR.torch_grads(*case.vids[0][:2], case.tabs[0]['trans'], case.tabs[0]['init'], case.tabs[0]['len'], 64)[0] == -np.inf


@pytest.mark.parametrize('name', ['over_one_tile', 'halo_longer_than_a_tile', 'longest_transcript'])
def test_tile_edges_against_the_twin(name):
    """T = P + 37 at kp = 64 with the fewest entries that give the sum more than a handful of terms (M = 16: the case above with
    a path); T = 2 P + 11, M = 3, k_rows = 1024: the halo is longer than a tile and the span limit is clipped to T; T = 300,
    M = 256, kp = 8: the longest transcript, a narrow cone."""
    P = _tile()
    T, M, k_rows = {'over_one_tile': (P + 37, 16, 64), 'halo_longer_than_a_tile': (2 * P + 11, 3, 1024),
                    'longest_transcript': (300, 256, 8)}[name]
    case = _edge_case(T, M, k_rows, seed=M)
    z, g, err = case.run()
    assert err == 0
    _check(case, z, g, *case.reference(TR.twin_grads), name)


# ------------------------------------------------------------------------------------------------ e. dynamic range
def test_dynamic_range_against_the_twin():
    """T = 2000, M = 6, kp = 1024; the elp columns differ by +-50 per frame in runs of 100 - 300 frames, the length scores are
    Poisson log-pmfs with rates 50 - 400: h moves by thousands of nats across a tile, so a shared linear-domain reference
    would underflow the dominant terms."""
    rng = np.random.default_rng(5)
    T, M, C, K = 2000, 6, 4, 1024
    elp = rng.normal(size=(T, C))
    t = 0
    while t < T:
        run = int(rng.integers(100, 301))
        elp[t:t + run] += rng.choice([-50.0, 50.0], size=C)
        t += run
    rates = rng.uniform(50, 400, size=C)
    k = np.arange(K)[:, None]
    tab = dict(trans=rng.normal(size=(C, C)), init=rng.normal(size=C), len=k * np.log(rates) - rates - torch.lgamma(torch.arange(K, dtype=torch.float64) + 1).numpy()[:, None])
    a = [0, 1, 2, 3, 1, 0]
    case = Case([(elp, a, 0)], [tab], K)
    z, g, err = case.run()
    assert err == 0
    _check(case, z, g, *case.reference(TR.twin_grads), 'dynamic range')


# ------------------------------------------------------------------------------------------------ f. degenerate inputs
def test_degenerate_videos_beside_healthy_ones():
    rng = np.random.default_rng(12)
    C, K = 3, 6
    healthy, holes = _tables(rng, C, K), _tables(rng, C, K)
    holes['len'][2, :] = -np.inf                              # some alignments are left
    holes['init'][1] = -np.inf
    holes['trans'][2, 0] = -np.inf
    e = lambda T: rng.normal(size=(T, C)) * 2
    nan_elp = e(10)
    nan_elp[4, 2] = np.nan                                    # in a class its transcript never names
    vids = [(e(14), [0, 1, 2, 1], 0), (e(11), [0, 1, 0], 1), (e(9), [1, 0], 1), (e(9), [0, 2], 1), (nan_elp, [0, 1, 0], 0),
            (e(7), [2, 2], 0)]
    u = np.array([1.0, 2.0, 1.0, 1.0, 1.0, -0.5])
    case = Case(vids, [healthy, holes], K, u=u)
    z, g, err = case.run()
    assert err != 0
    assert np.isfinite(z[[0, 1, 5]]).all() and z[2] == -np.inf and z[3] == -np.inf and np.isnan(z[4])
    for i in (2, 3, 4):
        assert not g['elp'][case.off[i]:case.off[i + 1]].any()
    # the reference: the same launch without the video that sets the error word (torch route: it knows -inf)
    vids_ok = [v if i != 4 else (np.zeros((10, C)), [0] * 11, 0) for i, v in enumerate(vids)]     # (-inf by counting: zeros)
    ok = Case(vids_ok, [healthy, holes], K, u=u)
    zr, gr = ok.reference(TR.torch_grads)
    assert zr[4] == -np.inf
    z2 = np.where(np.isnan(z), -np.inf, z)
    _check(ok, z2, g, zr, gr, 'degenerate beside healthy')
    # ... and the healthy videos alone give the same bits
    alone = Case([vids[0], vids[5]], [healthy, holes], K, u=u[[0, 5]])
    za, ga, erra = alone.run()
    assert erra == 0 and np.array_equal(za, z[[0, 5]])
    assert np.array_equal(ga['elp'][:14], g['elp'][:14]) and np.array_equal(ga['len'][0], g['len'][0])
    assert np.array_equal(ga['trans'][0], g['trans'][0]) and np.array_equal(ga['init'][0], g['init'][0])


# ------------------------------------------------------------------------------------------------ g. determinism
def test_two_calls_give_the_same_bits():
    case = _ragged(True)
    z1, g1, _ = case.run()
    z2, g2, _ = case.run()
    assert np.array_equal(z1, z2)
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), k


# ------------------------------------------------------------------------------------------------ h. module and model
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
    transcripts = []
    for i, t in enumerate(lengths):
        M = int(rng.integers(-(-t // (k - 1)) + 1, 8))
        a = [vc[int(v)] for v in rng.integers(0, len(vc), size=M)]
        cuts = np.sort(rng.choice(np.arange(1, t), size=M - 1, replace=False))
        lab = np.repeat(np.array(a), np.diff(np.concatenate([[0], cuts, [t]])))
        x[i, :t] = mu[lab] + rng.standard_normal((t, d))
        transcripts.append(a)
    rb = R.RefBatch(x, list(lengths), vc)
    return m.cuda(), rb, vc, transcripts


def _module_reference(m, rb, vc, transcripts):
    """(log Z_a per video, log Z per video) as differentiable torch values of train_ref's leaves."""
    q, leaves = R.params_from_module(m)
    trans, init, lens, merged = R.tables(q, rb.valid_classes)
    elp = R.emission(q, merged, rb)
    kp = R.kp_of(lens, rb)
    loc = {c: j for j, c in enumerate(vc)}
    za = torch.stack([TR.torch_logz(elp[i, :int(t)], [loc[c] for c in transcripts[i]], trans, init, lens, kp)
                      for i, t in enumerate(rb.lengths.tolist())])
    return q, leaves, za


@pytest.mark.parametrize('discriminative', [False, True])
def test_module_values_and_parameter_gradients(discriminative):
    """transcript_log_partition and log_likelihood(transcripts=...) against the torch recursion chained through train_ref's
    tables; discriminative: minus log Z (the twin), the difference held to the size of its two parts."""
    m, rb, vc, transcripts = _module_case()
    m.args.sm_train_discriminatively = discriminative
    dev = torch.device('cuda:0')
    x, lengths, vcs = rb.features.to(dev), rb.lengths.to(dev), [rb.valid_classes] * len(transcripts)
    q, leaves, za = _module_reference(m, rb, vc, transcripts)
    value = za.mean().item()
    ref = R.grads(leaves, za.mean())
    models = None
    if discriminative:
        zl = R.logz_factored(q, rb)
        value -= zl.mean().item()
        gl = R.grads(leaves, zl.mean())
        models = {n: dict(size=np.abs(ref[n]) + np.abs(gl[n])) for n in ref}
        ref = {n: ref[n] - gl[n] for n in ref}
    z = m.transcript_log_partition(x, lengths, vcs, transcripts)
    assert z.dtype == torch.float64 and z.requires_grad
    np.testing.assert_allclose(z.detach().cpu().numpy(), za.detach().numpy(), rtol=Z_BAR)
    m.zero_grad()
    ll, _ = m.log_likelihood(x, lengths, vcs, transcripts=transcripts)
    ll.backward()
    assert abs(ll.item() - value) <= Z_BAR * max(1.0, abs(za.mean().item()))
    got = R.module_grads(m)
    assert all(np.abs(v).max() > 0 for v in got.values())
    R.assert_grads_close(got, ref, ROW_BAR, 'transcript discriminative=%s' % discriminative, models)


def test_module_packed_model_and_the_viterbi_transcript():
    """transcript_log_partition on padded batches = _packed on the same videos = SemiMarkovModel.transcript_log_likelihood by
    video name; with each video's own Viterbi transcript log Z_a - log Z <= 0; .backward() fills the four parameter gradients."""
    from action_segmentation_amd import ops, synth
    from action_segmentation_amd.batching import make_data_loader
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
    tr = spans_to_transcripts(out['spans'], pc.lengths)
    by_video = dict(zip(pc.video_names, tr))
    za = mod.transcript_log_partition_packed(pc, tr)
    assert za.requires_grad and za.dtype == torch.float64 and za.shape == (len(tr),)
    zl = mod.log_partition_packed(pc)
    best = out['best'].cpu().numpy()
    zah, zlh = za.detach().cpu().numpy(), zl.detach().cpu().numpy()
    tol = 1e-9 * np.maximum(1.0, np.abs(zlh))
    assert np.isfinite(zah).all() and (best <= zah + tol).all() and (zah <= zlh + tol).all()
    got = model.transcript_log_likelihood(data, by_video)
    cond = model.transcript_log_likelihood(data, by_video, conditional=True)
    assert sorted(got) == sorted(pc.video_names)
    for i, n in enumerate(pc.video_names):
        assert abs(got[n] - zah[i]) <= 1e-9 * max(1.0, abs(zah[i])), n
        assert abs(cond[n] - (zah[i] - zlh[i])) <= 1e-9 * max(1.0, abs(zah[i])), n
    mod.zero_grad()
    za.sum().backward()
    assert all(getattr(mod, n).grad is not None and bool(getattr(mod, n).grad.abs().max() > 0) for n in R.PARAMS)
    # per batch, padded
    pos = {name: j for j, name in enumerate(pc.video_names)}
    n_seen = 0
    for batch in make_data_loader(model.args, data, shuffle=False, batch_by_task=True, batch_size=model.args.batch_size):
        feats, lengths = batch['features'].to('cuda:0'), batch['lengths']
        addl = model.make_additional_allowed_ends(batch['task_name'], lengths)
        z = mod.transcript_log_partition(feats, lengths, batch['task_indices'], [by_video[v] for v in batch['video_name']],
                                         additional_allowed_ends_per_instance=addl).detach().cpu().numpy()
        for i, name in enumerate(batch['video_name']):
            assert abs(z[i] - zah[pos[name]]) <= 1e-9 * max(1.0, abs(zah[pos[name]])), name
            n_seen += 1
    assert n_seen == len(pc.video_names)
    # a transcript no segmentation of its video has: the differentiable entry point names the video, the model returns -inf
    first = pc.video_names[0]
    bad = dict(by_video)
    bad[first] = np.array(list(by_video[first][:1]), np.int64)           # one segment cannot cover the video (K = 12 < T)
    with pytest.raises(ValueError, match=str(first)):
        mod.transcript_log_partition_packed(pc, [bad[n] for n in pc.video_names])
    assert model.transcript_log_likelihood(data, bad)[first] == -np.inf


# ------------------------------------------------------------------------------------------------ i. stream capture
def test_forward_and_backward_capture_into_a_hip_graph():
    """The pair captured once and replayed twice on fresh inputs of the ragged shape: every replay reproduces the eager call
    on those inputs bit for bit."""
    ops = _ops()
    case = _ragged(True)
    batch, d = case.device_inputs()
    ids, off = ops._transcript_arrays(batch, [v[1] for v in case.vids])
    tr = (torch.from_numpy(ids).cuda(), off)
    ws = torch.empty(ops.align_logz_workspace_bytes(batch, off), dtype=torch.uint8, device='cuda:0')

    def step():
        z = ops.align_logz(batch, d['elp'], d['trans'], d['init'], d['len'], tr, endpen=d['endpen'], ws=ws)
        g = ops.align_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], tr, z, grad_logz=d['u'], endpen=d['endpen'], ws=ws)
        return z, g['elp'], g['trans'], g['init'], g['len']

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
        fresh = _ragged(True, values=rep)
        _, f = fresh.device_inputs()
        for k in ('elp', 'trans', 'init', 'len', 'endpen'):
            d[k].copy_(f[k])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = [v.clone() for v in out]
        eager = step()
        torch.cuda.synchronize()
        for name, a, e in zip(('logz', 'g_elp', 'g_trans', 'g_init', 'g_len'), got, eager):
            assert torch.equal(a, e), '%s, replay %d' % (name, rep)
