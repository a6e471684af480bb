"""Posterior samples (smm_sample_f64 / SemiMarkovModule.sample*) and frame posteriors on the GPU.

A sampler's outputs depend on its generator, so the tests pin the DISTRIBUTION: exactly (total variation against every
segmentation enumerated on the dense reference lattice) on small lattices, and through the per-frame posteriors of the C
twin (oracle.factored) at real sizes.  Every seed is fixed: the tests are deterministic."""
import ctypes
from collections import Counter

import numpy as np
import pytest
import torch

from oracle import dense_ref as O
from oracle import factored as F
from module_util import make_args

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _module(n_classes, d, k, seed, constrained=False, scale=1.0):
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    g = torch.Generator().manual_seed(seed)
    kw = {}
    if constrained:
        # a chain 0 -> 1 -> ... with a side branch; self transitions allowed
        trans = {s: {s, s + 1} for s in range(n_classes - 1)}
        trans[n_classes - 1] = {n_classes - 1}
        trans[0].add(min(2, n_classes - 1))
        kw = dict(allowed_starts={0, 1}, allowed_transitions=trans, allowed_ends={n_classes - 1, n_classes - 2})
    m = SemiMarkovModule(make_args(k), n_classes, d, allow_self_transitions=True, **kw)
    with torch.no_grad():
        m.poisson_log_rates.copy_(torch.rand(n_classes, generator=g) * 1.5 + 0.2)
        m.gaussian_means.copy_(torch.randn(n_classes, d, generator=g) * scale)
        m.gaussian_cov.copy_(torch.diag(1.0 + torch.rand(d, generator=g)))
        m.transition_logits.copy_(torch.randn(n_classes, n_classes, generator=g))
        m.init_logits.copy_(torch.randn(n_classes, generator=g))
    return m.to(DEV), g


def _ref_params(m):
    ic, tc = getattr(m, 'init_constraints', None), getattr(m, 'transition_constraints', None)
    return O.RefParams(m.n_classes, m.poisson_log_rates.detach().cpu(), m.gaussian_means.detach().cpu(),
                       torch.diagonal(m.gaussian_cov.detach().cpu()).clone(), m.transition_logits.detach().cpu(),
                       m.init_logits.detach().cpu(), m.max_k, True, None if ic is None else ic.cpu(),
                       None if tc is None else tc.cpu(), m.allowed_ends).to(torch.float64)


def _features(m, g, b, lengths, d, noise=1.5):
    tmax = max(lengths)
    lab = torch.randint(0, m.n_classes, (b, tmax), generator=g)
    x = m.gaussian_means.detach().cpu()[lab] + torch.randn(b, tmax, d, generator=g) * noise
    for i, t in enumerate(lengths):
        x[i, t:] = 0
    return x


def _enumerate(edge, pos_len):
    """Every segmentation of one instance of a dense lattice: {local span encoding (tuple, length pos_len): score}."""
    e = edge.numpy()
    n_1, k_all, c, _ = e.shape
    last = pos_len - 1
    out = {}

    def rec(n, cur, acc, seq):
        if n == last:
            out[tuple(seq)] = acc
            return
        for k in range(1, k_all):
            if n + k > last:
                break
            for nxt in range(c):
                s2 = seq[:]
                s2[n + k] = nxt
                rec(n + k, nxt, acc + float(e[n, k, nxt, cur]), s2)

    for c0 in range(c):
        seq = [-1] * pos_len
        seq[0] = c0
        rec(0, c0, 0.0, seq)
    return out


# evidence strong enough that the posterior of every small lattice is concentrated on at most a few hundred segmentations:
# the total variation of n = 100 000 draws of a PERFECT sampler is ~0.5 sum sqrt(2 p / (pi n)), which exceeds 0.01 on
# lattices whose posterior spreads over a thousand segmentations or more
EXACT_SCALE, EXACT_NOISE = 1.5, 0.9
SMALL = [
    # (K, add_eos, constrained, additional ends, narration constraints)
    (2, True, False, False, False),
    (4, True, False, False, False),
    (4, False, False, False, False),
    (2, False, False, False, False),
    (4, True, True, False, False),
    (4, False, True, False, False),
    (4, True, True, True, False),
    (4, True, False, False, True),
    (2, True, True, False, True),
]


@pytest.mark.parametrize('k,add_eos,constrained,additional,narration', SMALL)
def test_exact_distribution_on_small_lattices(k, add_eos, constrained, additional, narration):
    """100 000 samples per video against the exact posterior over every segmentation (dense reference lattice):
    total variation <= 0.01, no segmentation below 1e-12 drawn, and every sample's log_prob equal to its dense-path
    rescore minus log Z."""
    d, c = 6, 3
    m, g = _module(c, d, k, seed=100 + k + 10 * add_eos + 20 * constrained + 40 * narration, constrained=constrained,
                   scale=EXACT_SCALE)
    lengths = [7, 5, 6]
    b = len(lengths)
    x = _features(m, g, b, lengths, d, noise=EXACT_NOISE)
    valid = torch.arange(c)
    add = [[0], [], [1]] if additional else None
    cons = None
    if narration:
        cons = torch.zeros(b, max(lengths), c, dtype=torch.float64)
        cons[0, 2, 1] = -1e9                       # frame 2 of video 0 may not be class 1
        cons[1, 0:2, 2] = -1e9
        cons += torch.randn(b, max(lengths), c, generator=g).double() * 0.3
    n = 100000
    spans, logp = m.sample(x.float().to(DEV), torch.tensor(lengths).to(DEV), [valid] * b, n_samples=n, seed=7,
                           add_eos=add_eos, additional_allowed_ends_per_instance=add,
                           constraints=None if cons is None else cons.float().to(DEV))
    logp = logp.cpu().numpy()
    p = _ref_params(m)
    scores, _ = O.score_features(p, x.double(), torch.tensor(lengths), valid, add_eos, add,
                                 None if cons is None else cons.float().double())
    pos = torch.tensor(lengths) + (1 if add_eos else 0)
    z_ref = O.log_partition(p, x.double(), torch.tensor(lengths), valid, add_eos, add,
                            None if cons is None else cons.float().double())
    sp = spans.numpy()
    assert sp.shape == (n, b, max(lengths) + (1 if add_eos else 0))
    for i in range(b):
        pl = int(pos[i])
        paths = _enumerate(scores[i, :pl - 1], pl)
        allv = np.array(list(paths.values()))
        lz = float(torch.logsumexp(torch.from_numpy(allv), 0))
        assert abs(lz - float(z_ref[i])) <= 1e-9 * max(1.0, abs(lz))
        rows = sp[:, i, :pl].copy()
        if add_eos:
            assert (rows[:, pl - 1] == m.n_classes).all()
            rows[:, pl - 1] = c                        # EOS -> local id C of the augmented lattice
        assert (sp[:, i, pl:] == -1).all()
        cnt = Counter(map(tuple, rows.tolist()))
        tv = 0.0
        for path, sc in paths.items():
            pr = np.exp(sc - lz)
            f = cnt.get(path, 0) / n
            tv += abs(f - pr)
            if pr < 1e-12:
                assert f == 0, (path, sc - lz)
        assert set(cnt) <= set(paths), "a sampled segmentation outside the lattice"
        tv *= 0.5
        # (the bar must stand above the noise of n draws from the exact distribution itself: E[TV] of a perfect sampler)
        pr = np.exp(np.array(list(paths.values())) - lz)
        assert 0.5 * np.sum(np.sqrt(2 * pr * (1 - pr) / (np.pi * n))) <= 0.007
        assert tv <= 0.01, tv
        # log-probabilities: every distinct sample against the dense rescore - log Z
        tol = 1e-6 * max(1.0, abs(lz))
        first = {}
        for j, r in enumerate(map(tuple, rows.tolist())):
            first.setdefault(r, j)
        for path, j in first.items():
            assert abs(logp[j, i] - (paths[path] - lz)) <= tol, (path, logp[j, i], paths[path] - lz)


def test_log_prob_equals_gold_score_minus_log_partition():
    """A constrained batch of cfg4's shape: log_prob = gold_score(spans[..., :Tmax]) - log_partition."""
    d, c, k = 16, 7, 64
    m, g = _module(c, d, k, seed=3, constrained=True, scale=0.7)
    lengths = [900, 640, 1200, 333]
    b = len(lengths)
    x = _features(m, g, b, lengths, d).float().to(DEV)
    ln = torch.tensor(lengths).to(DEV)
    valid = torch.arange(c)
    spans, logp = m.sample(x, ln, [valid] * b, n_samples=6, seed=11)
    z = m.log_partition(x, ln, valid).detach()
    tmax = max(lengths)
    for s in range(spans.shape[0]):
        gs = m.gold_score(x, ln, valid, spans[s, :, :tmax].to(DEV)).detach()
        ref = (gs - z).cpu().numpy()
        got = logp[s].cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6 * max(1.0, float(z.abs().max())))
    assert np.isfinite(logp.cpu().numpy()).all()


def _frequencies(labels, lengths, offs, c, n):
    out = []
    for t, o in zip(lengths, offs):
        lab = labels[:, o:o + t]
        out.append(np.stack([(lab == j).mean(0) for j in range(c)], axis=1))
    return out


def _exceedances(freq, ref, n):
    """Entries whose frequency of n draws lies outside 6 sqrt(p (1 - p) / n) + 2e-3 of the posterior p, and how many of them
    a PERFECT sampler is expected to give: with 1e5 entries, most at p in (1e-4, 0.05), the binomial tails put dozens of
    entries outside such a bound at n = 256 (k1024: 66 expected).  The expectation is exact (sum of binomial tail
    probabilities) whatever the correlations between frames."""
    from scipy.stats import binom
    p = np.clip(ref, 0.0, 1.0)
    bound = 6 * np.sqrt(p * (1 - p) / n) + 2e-3
    bad = int((np.abs(freq - p) > bound).sum())
    hi, lo = np.floor((p + bound) * n), np.ceil((p - bound) * n)
    expected = float((binom.sf(hi, n, p) + binom.cdf(lo - 1, n, p)).sum())
    return bad, expected


@pytest.mark.parametrize('shape', ['cfg2', 'k1024'])
def test_frequencies_match_posteriors_at_real_sizes(shape):
    """256 samples per video: per-frame class frequencies within 6 sqrt(p(1-p)/N) + 2e-3 of the C twin's posteriors, but for
    as many entries as binomial noise puts outside (_exceedances); frame_posteriors within 2e-5 of them."""
    if shape == 'cfg2':
        c, k, d, lengths = 16, 256, 24, [2048, 2048, 2048]
    else:
        c, k, d, lengths = 23, 1024, 24, [8192]
    m, g = _module(c, d, k, seed=21, scale=0.4)
    b = len(lengths)
    x = _features(m, g, b, lengths, d)
    valid = torch.arange(c)
    n = 256
    xd, ln = x.float().to(DEV), torch.tensor(lengths).to(DEV)
    spans, logp = m.sample(xd, ln, [valid] * b, n_samples=n, seed=5)
    post = m.frame_posteriors(xd, ln, [valid] * b).cpu().numpy()
    p = _ref_params(m)
    trans, init, lens, merged = O.factor_tables(p, valid)
    elp = O.emission_log_probs(x.float().double(), p.gaussian_means[merged], p.gaussian_cov_diag)
    _, gr = F.logz(elp.numpy(), np.array(lengths), trans.numpy(), init.numpy(), lens.numpy(), grad=True)
    assert np.isfinite(logp.cpu().numpy()).all()
    for i, t in enumerate(lengths):
        ref = gr['elp'][i, :t]
        np.testing.assert_allclose(post[i, :t], ref, rtol=0, atol=2e-5)
        lab = O.spans_to_labels(spans[:, i, :t].numpy())       # local == global ids here (valid = arange)
        freq = np.stack([(lab == j).mean(0) for j in range(c)], axis=1)
        bad, expected = _exceedances(freq, ref, n)
        assert bad <= 2 * expected + 10, (bad, expected, float(np.abs(freq - ref).max()))


def test_validity_on_constrained_data():
    """Samples of a constrained model (masks on starts / transitions / ends, cfg4's span limit): no forbidden transition,
    allowed first and last labels, no span longer than K - 1, spans consistent with the per-frame labels of sample_packed."""
    from action_segmentation_amd.batching import pack_batches
    d, c, k = 16, 7, 64
    m, g = _module(c, d, k, seed=9, constrained=True, scale=0.7)
    lengths = [700, 512, 1500, 901, 64]
    b = len(lengths)
    x = _features(m, g, b, lengths, d)
    valid = torch.arange(c)
    n = 8
    spans, logp = m.sample(x.float().to(DEV), torch.tensor(lengths).to(DEV), [valid] * b, n_samples=n, seed=2)
    tc, ic = m.transition_constraints.cpu(), m.init_constraints.cpu()          # True = forbidden, [to, from]
    allowed_t = {(f, t) for f in range(c) for t in range(c) if not bool(tc[t, f])}
    starts = {j for j in range(c) if not bool(ic[j])}
    for s in range(n):
        for i, t in enumerate(lengths):
            row = spans[s, i].numpy()
            assert row[t] == m.n_classes and (row[t + 1:] == -1).all()
            st = np.flatnonzero(row[:t] != -1)
            assert st[0] == 0
            labs = row[st]
            seglen = np.diff(np.append(st, t))
            assert seglen.max() <= k - 1
            assert int(labs[0]) in starts and int(labs[-1]) in m.allowed_ends
            for a, bb in zip(labs[:-1], labs[1:]):
                assert (int(a), int(bb)) in allowed_t, (a, bb)
    # the packed path: frame labels consistent with its spans' run structure and with the masks
    batch = dict(task_name=['t'] * b, task_indices=[valid] * b, lengths=torch.tensor(lengths), features=x,
                 video_name=['v%d' % i for i in range(b)])
    pc = pack_batches([batch], DEV, m.max_k)
    lab, lp = m.sample_packed(pc, n, seed=2)
    lab = lab.cpu().numpy()
    assert lab.shape == (n, sum(lengths)) and (lab >= 0).all() and (lab < c).all()
    for s in range(n):
        for i, (t, o) in enumerate(zip(pc.lengths, pc.frame_offset)):
            seq = lab[s, o:o + t]
            assert int(seq[0]) in starts and int(seq[-1]) in m.allowed_ends
            ch = np.flatnonzero(seq[1:] != seq[:-1])
            for p0 in ch:
                assert (int(seq[p0]), int(seq[p0 + 1])) in allowed_t


def test_determinism_and_packed_agreement():
    """Same seed -> same outputs; the first 4 of 16 samples = 4 samples; another seed differs; sample_packed draws from the
    same distribution as sample, and gives identical spans the same log-probability."""
    from action_segmentation_amd.batching import pack_batches
    d, c, k = 12, 9, 48
    m, g = _module(c, d, k, seed=13, scale=0.3)
    lengths = [600, 450, 600]
    b = len(lengths)
    x = _features(m, g, b, lengths, d)
    valid = torch.tensor([0, 1, 2, 4, 5, 6, 7, 8])
    cl = len(valid)
    xd, ln = x.float().to(DEV), torch.tensor(lengths).to(DEV)
    s1, l1 = m.sample(xd, ln, [valid] * b, n_samples=16, seed=123)
    s2, l2 = m.sample(xd, ln, [valid] * b, n_samples=16, seed=123)
    s3, l3 = m.sample(xd, ln, [valid] * b, n_samples=4, seed=123)
    s4, _ = m.sample(xd, ln, [valid] * b, n_samples=16, seed=124)
    assert torch.equal(s1, s2) and torch.equal(l1, l2)
    assert torch.equal(s1[:4], s3) and torch.equal(l1[:4], l3)
    assert not torch.equal(s1, s4)
    # class ids are global (the class map is applied)
    ids = set(np.unique(s1.numpy()).tolist()) - {-1, m.n_classes}
    assert ids <= set(valid.tolist())
    # packed: one group, the same videos
    batch = dict(task_name=['t'] * b, task_indices=[valid] * b, lengths=torch.tensor(lengths), features=x,
                 video_name=['v%d' % i for i in range(b)])
    pc = pack_batches([batch], DEV, m.max_k)
    n = 256
    lab_p, lp_p = m.sample_packed(pc, n, seed=77)
    sp, lp = m.sample(xd, ln, [valid] * b, n_samples=n, seed=77)
    post = m.frame_posteriors_packed(pc).cpu().numpy()
    post_pad = m.frame_posteriors(xd, ln, [valid] * b).cpu().numpy()
    lab_p = lab_p.cpu().numpy()
    vmap = {int(v): j for j, v in enumerate(valid.tolist())}
    for i, (t, o) in enumerate(zip(pc.lengths, pc.frame_offset)):
        np.testing.assert_allclose(post[o:o + t, :cl], post_pad[i, :t], rtol=0, atol=1e-9)
        ref = post[o:o + t, :cl]
        for labs in (lab_p[:, o:o + t], O.spans_to_labels(sp[:, i, :t].numpy())):
            loc = np.vectorize(vmap.get)(labs)
            freq = np.stack([(loc == j).mean(0) for j in range(cl)], axis=1)
            bad, expected = _exceedances(freq, ref, n)
            assert bad <= 2 * expected + 10, (bad, expected)
        # identical segmentations (as frame labels) get the same log-probability from both paths
        pad_labels = {tuple(O.spans_to_labels(sp[s:s + 1, i, :t].numpy())[0].tolist()): float(lp[s, i]) for s in range(n)}
        for s in range(n):
            key = tuple(lab_p[s, o:o + t].tolist())
            if key in pad_labels:
                assert abs(pad_labels[key] - float(lp_p[s, i])) <= 1e-6 * max(1.0, abs(pad_labels[key]))


def test_errors():
    """n_samples = 0 raises; smm_sample_f64 with every output NULL returns SMM_ERR_ARG."""
    from action_segmentation_amd import _lib
    d, c, k = 4, 3, 4
    m, g = _module(c, d, k, seed=1)
    x = _features(m, g, 1, [6], d).float().to(DEV)
    with pytest.raises(ValueError):
        m.sample(x, torch.tensor([6]).to(DEV), None, n_samples=0)
    lib = _lib.load()
    lengths = np.array([6], np.int64)
    shape = _lib.SmmShape(1, 0, 1, c, k, 6, 0, 6)
    dummy = torch.zeros(64, dtype=torch.float64, device=DEV)
    p = ctypes.c_void_p(dummy.data_ptr())
    rc = lib.smm_sample_f64(ctypes.byref(shape), ctypes.c_void_p(lengths.ctypes.data), None, None, None, None, p, p, p, p,
                            None, None, p, ctypes.c_int32(4), ctypes.c_uint64(0), None, None, None, None, ctypes.c_size_t(0),
                            None)
    assert rc == -1
