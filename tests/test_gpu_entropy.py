"""Exact posterior entropy H(y | x) of each video (smm_entropy_f64 / ops.entropy / SemiMarkovModule.entropy*) on the GPU.

References are computed here: -sum p log p over every segmentation of the dense reference lattice (small lattices),
log Z - E[score] from the C twin's exact fp64 marginals (real sizes; the identity itself is checked against the enumeration
first), and log N in closed form on the uniform lattice (N counted exactly with Python integers).  Every seed is fixed."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import dense_ref as O
from oracle import factored as F
from module_util import make_args

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NEG_INF = float('-inf')


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


def _entropy_of_scores(scores):
    """-sum p log p of the distribution exp(scores) / Z; zero-probability paths contribute nothing."""
    v = np.array(scores, dtype=np.float64)
    lz = float(torch.logsumexp(torch.from_numpy(v), 0))
    lp = v - lz
    p = np.exp(lp)
    keep = p > 0
    return float(-(p[keep] * lp[keep]).sum()), lz


def _twin_entropy(elp, lengths, trans, init, lens, endpen=None, tmax=None):
    """log Z - E[score] per video from the C twin's exact fp64 marginals (EOS mode).  E[score] sums every marginal times its
    potential; the closing term is the last frame's occupancy times the end penalty.  Terms of zero marginal are skipped, and
    so are masked potentials (<= -1e8): their exact marginal is exp(-1e9) = 0, but the twin's occupancies are differences of
    sums, whose rounding residue (~1e-17) times the mask would add ~1e-8 nats.  `tmax`: each video keeps that many frames of
    its padded row, so that the span limit is min(K, tmax) as in its batch (default: its own length)."""
    out = []
    for i, t in enumerate(lengths):
        ep = None if endpen is None else endpen[i:i + 1]
        e = elp[i:i + 1, :max(t, tmax or t)]
        z, g = F.logz(e, np.array([t]), trans, init, lens, endpen=ep, grad=True)
        kp = g['len'].shape[0]

        def dot(gr, x):
            gr, x = np.asarray(gr, np.float64), np.asarray(x, np.float64)
            nz = (gr != 0) & (x > -1e8)
            return float((gr[nz] * x[nz]).sum())

        es = dot(g['elp'], e) + dot(g['trans'], trans) + dot(g['init'], init) + dot(g['len'], np.asarray(lens)[:kp])
        if ep is not None:
            es += dot(g['elp'][0, t - 1], ep[0])
        out.append(float(z[0]) - es)
    return np.array(out)


def _batch_tables(elp_bt, lengths, trans, init, lens, endpen=None, no_eos=False):
    """Padded single-group batch for ops.* from host arrays: (Batch, elp, trans, init, len, endpen) on the device."""
    from action_segmentation_amd import ops
    b, tmax, c = elp_bt.shape
    k = lens.shape[0]
    batch = ops.Batch(lengths, [c], k, c_max=c, t_max=tmax, total_frames=b * tmax, no_eos=no_eos)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV).contiguous()
    return (batch, t(np.asarray(elp_bt).reshape(b * tmax, c)), t(np.asarray(trans)[None]), t(np.asarray(init)[None]),
            t(np.asarray(lens)[None]), None if endpen is None else t(endpen))


def _ops_entropy(batch, elp, trans, init, lens, endpen, with_backward=False):
    from action_segmentation_amd import ops
    ws = torch.empty(batch.workspace_bytes(), dtype=torch.uint8, device=DEV)
    z = ops.logz(batch, elp, trans, init, lens, endpen=endpen, ws=ws, with_backward=with_backward)
    h = ops.entropy(batch, elp, trans, init, lens, z, endpen=endpen, ws=ws, with_backward=with_backward)
    torch.cuda.synchronize()
    return h.cpu().numpy(), z.cpu().numpy(), ops.error_flag(batch, ws=ws)


def _count_segmentations(frames, kp, c, no_eos):
    """Exact number of segmentations of the uniform lattice (the kernel's conventions: spans of 1 .. kp - 1 positions; without
    EOS the last frame only carries the closing label, c choices)."""
    t = frames - 1 if no_eos else frames
    a = [1] + [0] * t
    win = 0                                   # sum of a[n - k] over k = 1 .. min(kp - 1, n)
    for n in range(1, t + 1):
        win += a[n - 1]
        if n - kp >= 0:
            win -= a[n - kp]
        a[n] = c * win
    return a[t] * (c if no_eos else 1)


def _log_int(n):
    return math.log(n) if n > 0 else NEG_INF


# ----------------------------------------------------------------------------------------------------------- 1. exact
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


def _small_case(k, add_eos, constrained, additional, narration):
    d, c = 6, 3
    m, g = _module(c, d, k, seed=300 + k + 10 * add_eos + 20 * constrained + 40 * narration, constrained=constrained,
                   scale=0.6)
    lengths = [7, 5, 6]
    b = len(lengths)
    x = _features(m, g, b, lengths, d, noise=EXACT_NOISE)
    valid = torch.arange(c)
    add = [[0], [], [1]] if additional else None
    cons = None
    if narration:
        cons = torch.zeros(b, max(lengths), c, dtype=torch.float64)
        cons[0, 2, 1] = -1e9
        cons[1, 0:2, 2] = -1e9
        cons += torch.randn(b, max(lengths), c, generator=g).double() * 0.3
    p = _ref_params(m)
    scores, elp = O.score_features(p, x.double(), torch.tensor(lengths), valid, add_eos, add,
                                   None if cons is None else cons.float().double())
    pos = torch.tensor(lengths) + (1 if add_eos else 0)
    ref = []
    for i in range(b):
        pl = int(pos[i])
        paths = _enumerate(scores[i, :pl - 1], pl)
        ref.append(_entropy_of_scores(list(paths.values()))[0])
    return m, x, lengths, valid, add, cons, p, elp, np.array(ref)


@pytest.mark.parametrize('k,add_eos,constrained,additional,narration', SMALL)
def test_exact_on_enumerable_lattices(k, add_eos, constrained, additional, narration):
    """SemiMarkovModule.entropy against -sum p log p over every segmentation of the dense reference lattice."""
    m, x, lengths, valid, add, cons, _, _, ref = _small_case(k, add_eos, constrained, additional, narration)
    b = len(lengths)
    h = m.entropy(x.float().to(DEV), torch.tensor(lengths).to(DEV), [valid] * b, add_eos=add_eos,
                  additional_allowed_ends_per_instance=add, constraints=None if cons is None else cons.float().to(DEV))
    assert h.dtype == torch.float64 and h.device.type == 'cuda' and h.shape == (b,)
    h = h.cpu().numpy()
    assert (ref > 0.05).any()                      # (the lattices are not trivially confident)
    for i in range(b):
        assert abs(h[i] - ref[i]) <= 1e-5 * max(1.0, ref[i]), (i, h[i], ref[i])


# ------------------------------------------------------------------------------------------------ 2. real sizes vs twin
@pytest.mark.parametrize('k,constrained,additional,narration', [(2, False, False, False), (4, False, False, False),
                                                                (4, True, False, False), (4, True, True, False),
                                                                (4, False, False, True)])
def test_twin_identity_on_small_lattices(k, constrained, additional, narration):
    """The reference of the real-size test (log Z - E[score] from the C twin) equals the enumeration (EOS mode)."""
    m, x, lengths, valid, add, cons, p, elp, ref = _small_case(k, True, constrained, additional, narration)
    trans, init, lens, _ = O.factor_tables(p, valid)
    ends = O.allowed_ends_for_batch(p, valid, add, len(lengths))
    ep = F.endpen_from_allowed_ends(ends, len(lengths), len(valid))
    twin = _twin_entropy(elp.numpy(), lengths, trans.numpy(), init.numpy(), lens.numpy(), ep)
    # (a prefix sum across a -1e9 cell carries ulp(1e9) ~ 1.2e-7 nats: the twin's sums do, the enumeration's do not)
    np.testing.assert_allclose(twin, ref, rtol=0, atol=1e-6 if narration else 1e-9)


def _real_case(shape):
    if shape == 'cfg2':
        c, k, d, lengths, constrained, scale = 16, 256, 24, [2048, 2048, 2048], False, 0.4
    elif shape == 'cfg1':
        c, k, d, lengths, constrained, scale = 20, 1024, 24, [10000], False, 0.4
    else:
        c, k, d, lengths, constrained, scale = 7, 64, 16, [900, 640, 1200, 333], True, 0.5
    m, g = _module(c, d, k, seed=41, constrained=constrained, scale=scale)
    b = len(lengths)
    x = _features(m, g, b, lengths, d)
    p = _ref_params(m)
    valid = torch.arange(c)
    trans, init, lens, merged = O.factor_tables(p, valid)
    cons = None
    if constrained:
        # narration-style -1e9 masks: in two windows of 40 frames per video one class may not occur
        cons = torch.randn(b, max(lengths), c, generator=g).double() * 0.3
        for i, t in enumerate(lengths):
            for _ in range(2):
                t0 = int(torch.randint(0, t - 40, (1,), generator=g))
                cons[i, t0:t0 + 40, int(torch.randint(0, c, (1,), generator=g))] = -1e9
    elp = O.emission_log_probs(x.float().double(), p.gaussian_means[merged], p.gaussian_cov_diag, cons)
    ends = O.allowed_ends_for_batch(p, valid, None, b)
    ep = F.endpen_from_allowed_ends(ends, b, c)
    return elp.numpy(), lengths, trans.numpy(), init.numpy(), lens.numpy(), ep


REAL_ERR = {}


@pytest.mark.parametrize('shape', ['cfg2', 'cfg1', 'cfg4'])
def test_real_sizes_against_twin(shape):
    """ops.entropy on the twin's own inputs against log Z - E[score] of its exact fp64 marginals: <= 1e-4 max(1, H)."""
    elp, lengths, trans, init, lens, ep = _real_case(shape)
    ref = _twin_entropy(elp, lengths, trans, init, lens, ep)
    h, _, err = _ops_entropy(*_batch_tables(elp, lengths, trans, init, lens, ep))
    assert err == 0
    rel = np.abs(h - ref) / np.maximum(1.0, ref)
    REAL_ERR[shape] = float(rel.max())
    print('entropy %s: H %s, worst relative error %.3g' % (shape, np.array2string(h, precision=4), rel.max()))
    assert (rel <= 1e-4).all(), (h, ref, rel)


# ------------------------------------------------------------------------------------------------ 3. uniform lattice
@pytest.mark.parametrize('frames,k,c', [(3, 3, 2), (4, 3, 2), (5, 3, 2), (6, 3, 3), (5, 4, 2)])
@pytest.mark.parametrize('no_eos', [False, True])
def test_segmentation_count_against_enumeration(frames, k, c, no_eos):
    """The closed-form count of the uniform lattice equals the finite-weight paths of the dense reference lattice."""
    z = torch.zeros
    scores = O.log_hsmm(z(c, c, dtype=torch.float64), z(1, frames, c, dtype=torch.float64), z(c, dtype=torch.float64),
                        z(k, c, dtype=torch.float64), torch.tensor([frames]), add_eos=not no_eos)
    pl = frames if no_eos else frames + 1
    paths = _enumerate(scores[0, :pl - 1], pl)
    n = sum(1 for v in paths.values() if v > -1e8)
    assert n == _count_segmentations(frames, min(k, frames), c, no_eos)


@pytest.mark.parametrize('no_eos', [False, True])
def test_uniform_lattice_is_log_count(no_eos):
    """All-zero emissions, tables and end penalties: the posterior is uniform and H = log N (1e-4 relative), up to T = 14 000,
    K = 1024, 23 states.  No oracle involved."""
    c, k = 23, 1024
    lengths = [14000, 3001, 1024, 700, 50, 2]
    b, tmax = len(lengths), max(lengths)
    zeros = np.zeros
    args = _batch_tables(zeros((b, tmax, c)), lengths, zeros((c, c)), zeros(c), zeros((k, c)),
                         None if no_eos else zeros((b, c)), no_eos=no_eos)
    h, _, err = _ops_entropy(*args)
    assert err == 0
    kp = min(k, tmax)
    ref = np.array([_log_int(_count_segmentations(t, kp, c, no_eos)) for t in lengths])
    rel = np.abs(h - ref) / np.maximum(1.0, ref)
    REAL_ERR['uniform' + ('_no_eos' if no_eos else '')] = float(rel.max())
    print('uniform lattice (no_eos=%s): worst relative error %.3g' % (no_eos, rel.max()))
    assert (rel <= 1e-4).all(), (h, ref)


# ------------------------------------------------------------------------------------------------ 4. zero entropy
def _one_path_tables(mask, no_eos):
    """3 states, spans of exactly 2 positions, init only 0, transitions only 0 -> 1 -> 2, ends only in 2 (EOS): one
    segmentation of 6 positions has finite weight (a mask is `mask`: -inf or -1e9)."""
    c, k, t = 3, 4, 6
    g = np.random.default_rng(5)
    frames = t + (1 if no_eos else 0)
    elp = g.normal(size=(1, frames, c)) * 2.0
    trans = np.full((c, c), mask)
    trans[1, 0] = trans[2, 1] = 0.3
    if no_eos:
        trans[2, 2] = -0.2                 # (the closing label: only 2 after 2)
    init = np.full(c, mask)
    init[0] = -0.1
    lens = np.full((k, c), mask)
    lens[2, :] = -0.7
    ep = None if no_eos else np.array([[mask, mask, 0.0]])
    return elp, [frames], trans, init, lens, ep, no_eos


@pytest.mark.parametrize('no_eos', [False, True])
def test_zero_entropy(no_eos):
    """One segmentation of finite weight: H = 0 within 1e-9 under true -inf masks (no NaN), H <= 1e-6 under -1e9 masks."""
    elp, lengths, trans, init, lens, ep, ne = _one_path_tables(NEG_INF, no_eos)
    h, z, err = _ops_entropy(*_batch_tables(elp, lengths, trans, init, lens, ep, no_eos=ne))
    assert np.isfinite(z).all() and err == 0
    assert np.isfinite(h).all() and abs(h[0]) <= 1e-9, h
    elp, lengths, trans, init, lens, ep, ne = _one_path_tables(-1e9, no_eos)
    h, z, err = _ops_entropy(*_batch_tables(elp, lengths, trans, init, lens, ep, no_eos=ne))
    assert err == 0 and np.isfinite(h).all() and 0.0 <= h[0] <= 1e-6, h


# ------------------------------------------------------------------------------------------------ 5, 6. corpus
def _corpus():
    """Two tasks (different class subsets, lengths), one module: (module, padded batches, PackedCorpus)."""
    from action_segmentation_amd.batching import pack_batches
    d, c, k = 10, 9, 40
    m, g = _module(c, d, k, seed=61, scale=0.5)
    batches = []
    for task, valid, lengths in (('a', torch.tensor([0, 1, 2, 4, 5]), [300, 180, 260]),
                                 ('b', torch.tensor([1, 3, 5, 6, 7, 8]), [150, 220])):
        x = _features(m, g, len(lengths), lengths, d, noise=2.0)
        batches.append(dict(task_name=[task] * len(lengths), task_indices=[valid] * len(lengths),
                            lengths=torch.tensor(lengths), features=x,
                            video_name=['%s%d' % (task, i) for i in range(len(lengths))]))
    pc = pack_batches(batches, DEV, m.max_k)
    return m, batches, pc


def test_agreement_with_sampler():
    """entropy_packed against the sample mean of -log p(y | x) of 4096 draws per video: within 5 sd / sqrt(n) + 1e-4 max(1, H)."""
    m, _, pc = _corpus()
    h = m.entropy_packed(pc).cpu().numpy()
    n = 4096
    _, lp = m.sample_packed(pc, n, seed=17)
    nl = -lp.cpu().numpy()
    assert h.shape == (len(pc.video_names),) and nl.shape == (n, len(pc.video_names))
    for i in range(len(h)):
        mean, sd = float(nl[:, i].mean()), float(nl[:, i].std(ddof=1))
        assert abs(h[i] - mean) <= 5 * sd / math.sqrt(n) + 1e-4 * max(1.0, h[i]), (pc.video_names[i], h[i], mean, sd)
    assert (h > 1.0).any()                         # (not a degenerate corpus)


def test_consistency_across_paths():
    """entropy_packed = entropy on each single-task batch; with_backward on / off; two calls bit-identical; H >= 0."""
    m, batches, pc = _corpus()
    hp = m.entropy_packed(pc).cpu().numpy()
    hp2 = m.entropy_packed(pc).cpu().numpy()
    assert np.array_equal(hp, hp2)
    pos = {name: j for j, name in enumerate(pc.video_names)}
    for bt in batches:
        valid = bt['task_indices']
        h = m.entropy(bt['features'].float().to(DEV), bt['lengths'].to(DEV), valid).cpu().numpy()
        h2 = m.entropy(bt['features'].float().to(DEV), bt['lengths'].to(DEV), valid).cpu().numpy()
        assert np.array_equal(h, h2)
        for i, name in enumerate(bt['video_name']):
            ref = hp[pos[name]]
            assert abs(h[i] - ref) <= 1e-12 * max(1.0, abs(ref)), (name, h[i], ref)
    assert (hp >= 0).all() and np.isfinite(hp).all()


@pytest.mark.parametrize('no_eos', [False, True])
def test_with_backward_and_bounds(no_eos):
    """ops.entropy with the reversed recursion in the log Z launch or in its own: the same to 1e-12; 0 <= H <= log N on the
    uniform lattice's sizes, with random tables."""
    c, k = 23, 1024
    lengths = [3001, 1024, 700, 50]
    b, tmax = len(lengths), max(lengths)
    g = np.random.default_rng(7)
    elp = g.normal(size=(b, tmax, c)) * 0.5
    trans = g.normal(size=(c, c)) - 3.0
    init = g.normal(size=c)
    lens = g.normal(size=(k, c)) * 0.5 - 6.0
    ep = None if no_eos else np.zeros((b, c))
    args = _batch_tables(elp, lengths, trans, init, lens, ep, no_eos=no_eos)
    h0, _, e0 = _ops_entropy(*args, with_backward=False)
    h1, _, e1 = _ops_entropy(*args, with_backward=True)
    assert e0 == 0 and e1 == 0
    np.testing.assert_allclose(h1, h0, rtol=1e-12, atol=0)
    kp = min(k, tmax)
    bound = np.array([_log_int(_count_segmentations(t, kp, c, no_eos)) for t in lengths])
    assert (h0 >= 0).all() and (h0 <= bound).all(), (h0, bound)


# ------------------------------------------------------------------------------------------------ 7. errors
def test_errors():
    """A NaN in elp: the error word is set and the video's value is NaN (ops level); SemiMarkovModule.entropy raises.  A
    workspace below smm_workspace_bytes: SMM_ERR_WORKSPACE."""
    from action_segmentation_amd import _lib, ops
    c, k = 5, 8
    lengths = [40, 33]
    g = np.random.default_rng(3)
    elp = g.normal(size=(2, 40, c))
    elp[1, 10, 2] = np.nan
    args = _batch_tables(elp, lengths, g.normal(size=(c, c)), g.normal(size=c), g.normal(size=(k, c)) - 2, np.zeros((2, c)))
    h, _, err = _ops_entropy(*args)
    assert err != 0 and np.isnan(h[1]) and np.isfinite(h[0])
    m, gen = _module(c, 4, k, seed=2)
    x = _features(m, gen, 2, lengths, 4)
    x[0, 5, 1] = float('nan')
    with pytest.raises(_lib.SmmError):
        m.entropy(x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(c)] * 2)
    batch, elp_d, tr, ini, ln, ep = args
    small = torch.empty(batch.workspace_bytes() // 2, dtype=torch.uint8, device=DEV)
    out = torch.empty(batch.b, dtype=torch.float64, device=DEV)
    z = torch.zeros(batch.b, dtype=torch.float64, device=DEV)
    lib = _lib.load()
    lh, fo, gr, kp, ns = batch.host_ptrs()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.smm_entropy_f64(ctypes.byref(batch.shape), lh, fo, gr, kp, ns, p(elp_d), p(tr), p(ini), p(ln), p(ep), p(z),
                             p(out), p(small), small.numel(), ops._raw_stream())
    assert rc == -3                                # SMM_ERR_WORKSPACE
    torch.cuda.synchronize()
