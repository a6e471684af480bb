"""Training gradients through the whole HIP chain -- fp32 parameters -> smm_factor_tables_f64 -> smm_emission_f64 ->
smm_logz_f64 / smm_logz_bwd_f64 -> smm_emission_bwd_f64 -> smm_factor_tables_bwd_f64 -> fp32 .grad -- against the
independent fp64 reference of tests/train_ref.py (dense_ref tables by autograd, the C twin's exact forward-backward),
at the shapes training runs at.  Every parameter row is held to its own size (train_ref.assert_rows_close) at 2e-5,
the bar the log Z backward kernels hold on their own (test_gpu_fullsize.py: _logz_both).

Error models, where the plain row bar cannot hold (measured on MI355X; every other parameter and test is held to it):
* Means where log Z enters at real sizes.  smm_logz_f64 / smm_logz_bwd_f64 keep their running sums in fp32 rings
  (csrc/smm_logz.hip, "Accuracy": a slot sums up to kp terms, relative error <= kp * 2^-24).  A mean gradient
  sum_t p_t(c) (x_td - mu_cd) / var_d cancels -- a class mean its frames sit around gives ~sqrt(n) from n terms of
  size ~1 -- and the kernels form p_t(c) as spans started minus spans ended up to t, so the posteriors' relative error
  reaches the gradient multiplied by a condition sum (train_ref.means_condition).  Without a model the means miss
  the row bar by 1.3x at cfg4 (13 states) and 6-16x on the long rings; rates, transitions and initial logits stay
  within 0.23 of it, and the packed step (T <= 300) within 0.75.  So cfg4 and the long rings allow the means
  ring_eps(kp) = kp * 2^-24 / 12 times that sum on top of the row bar (the measured need is at most 1/25 of kp * 2^-24).
* gold - log Z (--sm_train_discriminatively) at cfg4: the gold labels are what the posterior follows, so the two parts
  cancel to a remainder far below either (the means: 6e5x the row bar of the remainder).  The remainder's error is
  the log Z part's, so its bar scales with the size of the log Z part's gradient (``size``).
Both are capped at the bar these gradients were held to before, 5e-4 x (|ref| + max(1, max|ref|))."""
import numpy as np
import pytest
import torch

import train_ref as R
from golden_util import CASES, case_inputs
from module_util import make_args, module_from_golden
from oracle import dense_ref as O

pytestmark = pytest.mark.gpu
BAR = 2e-5


def _module(n_classes, d, k, mu, var, seed, **kw):
    """A SemiMarkovModule on the device holding the given means / variances and random logits / rates -> (module, the
    structure sets it was constructed with, for the reference to build its own masks from)."""
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    g = torch.Generator().manual_seed(seed)
    rate_hi = kw.pop('rate_hi', 60)
    m = SemiMarkovModule(make_args(k), n_classes, d, allow_self_transitions=True, **kw)
    with torch.no_grad():
        m.gaussian_means.copy_(torch.as_tensor(mu, dtype=torch.float32))
        m.gaussian_cov.copy_(torch.diag(torch.as_tensor(var, dtype=torch.float32)))
        m.transition_logits.copy_(torch.randn(n_classes, n_classes, generator=g))
        m.init_logits.copy_(torch.randn(n_classes, generator=g))
        m.poisson_log_rates.copy_(torch.log(torch.rand(n_classes, generator=g) * (rate_hi - 3) + 3))
    return m.cuda(), kw


def _pad(arrs, tmax, repeat_last=False):
    """Zero-padded batch [b, tmax, ...] (``repeat_last``: the tail repeats each row's last entry instead)."""
    out = np.zeros((len(arrs), tmax) + arrs[0].shape[1:], dtype=arrs[0].dtype)
    for i, a in enumerate(arrs):
        out[i, :a.shape[0]] = a
        if repeat_last:
            out[i, a.shape[0]:] = a[-1]
    return out


# ------------------------------------------------------------------------------------------------ cfg4 shape
def _cfg4(c, seed, lengths=(2048, 900, 1500, 200, 640), d=200, k=64):
    """BASELINE configs[3]'s shape: T <= 2048, K = 64, D = 200; a task of c states (a subset of c + 3 classes, in
    shuffled order) constrained to one left-to-right pass (allowed starts / transitions / ends), narration constraints
    of -1e4 outside each step's window (semimarkov.py:149-157), labels that follow the chain.
    -> (module, its structure sets, RefBatch with gold spans, the task's classes)."""
    g = np.random.default_rng(seed)
    n = c + 3
    vc = [int(v) for v in g.permutation(n)[:c]]
    sigma = g.uniform(0.7, 1.3, size=d)
    mu = g.normal(0, 0.3, size=(n, d))
    xs, labs, cons = [], [], []
    for t in lengths:
        cuts = np.sort(g.choice(np.arange(1, t), size=c - 1, replace=False))
        lab = np.repeat(np.arange(c), np.diff(np.concatenate([[0], cuts, [t]])))
        xs.append((mu[np.array(vc)[lab]] + sigma * g.standard_normal((t, d))).astype(np.float32))
        labs.append(np.array(vc)[lab])
        cn = np.zeros((t, c), np.float32)
        for j in range(1, c, 2):                                       # odd states = steps
            pos = np.flatnonzero(lab == j)
            lo, hi = max(0, pos.min() - int(g.integers(0, 20))), min(t, pos.max() + 1 + int(g.integers(0, 20)))
            cn[:lo, j] = -1e4
            cn[hi:, j] = -1e4
        cons.append(cn)
    trans = {v: {v} for v in range(n)}
    for j in range(c - 1):
        trans[vc[j]].add(vc[j + 1])
    m, st = _module(n, d, k, mu + g.normal(0, 0.02, size=mu.shape), sigma ** 2, seed, allowed_starts={vc[0]},
                allowed_transitions=trans, allowed_ends={vc[-1]})
    from action_segmentation_amd import semimarkov_utils as U
    tmax = max(lengths)
    spans = U.labels_to_spans(torch.from_numpy(_pad(labs, tmax, repeat_last=True)), max_k=k)
    rb = R.RefBatch(_pad(xs, tmax), list(lengths), vc, _pad(cons, tmax), None, True, spans)
    return m, st, rb, vc


def _on_device(rb):
    dev = torch.device('cuda:0')
    return (rb.features.to(dev), rb.lengths.to(dev), [rb.valid_classes] * rb.features.shape[0],
            None if rb.constraints is None else rb.constraints.to(dev))


@pytest.mark.parametrize('c', [7, 13])
def test_cfg4_log_likelihood_gradients(c):
    """log_likelihood(spans=None) at cfg4's shape: log Z per video to 1e-6 relative, the four parameter gradients of
    the batch mean at the 2e-5 row bar (the means with the ring model of the module docstring); the three classes
    outside the task get exactly no gradient."""
    m, st, rb, vc = _cfg4(c, 40 + c)
    x, lengths, vcs, cons = _on_device(rb)
    with torch.no_grad():
        z_gpu = m.log_partition(x, lengths, rb.valid_classes, constraints=cons).cpu().numpy()
    m.zero_grad()
    ll, _ = m.log_likelihood(x, lengths, vcs, spans=None, constraints=cons)
    ll.backward()
    q, leaves = R.params_from_module(m, **st)
    z = R.logz_factored(q, rb)
    ref = R.grads(leaves, z.mean())
    np.testing.assert_allclose(z_gpu, z.detach().numpy(), rtol=1e-6)
    np.testing.assert_allclose(ll.item(), z.mean().item(), rtol=1e-6)
    got = R.module_grads(m)
    b = rb.features.shape[0]
    means = dict(cond=R.means_condition(q, [rb], [np.full(b, 1.0 / b)]), eps=R.ring_eps(min(m.max_k, rb.features.shape[1])))
    R.assert_grads_close(got, ref, BAR, 'cfg4 c=%d' % c, {'gaussian_means': means})
    outside = sorted(set(range(m.n_classes)) - set(vc))
    assert not got['gaussian_means'][outside].any() and not got['transition_logits'][outside].any()


@pytest.mark.parametrize('discriminative', [False, True])
def test_cfg4_gold_score_gradients(discriminative):
    """Supervised gradient training: log_likelihood(spans=labels_to_spans(ground truth)) is the gold joint score
    (gold_score); with --sm_train_discriminatively it is gold - log Z.  Values and gradients against the factored gold
    score (sums along the spans on dense_ref's tables) and the twin's log Z."""
    m, st, rb, vc = _cfg4(13, 77)
    m.args.sm_train_discriminatively = discriminative
    x, lengths, vcs, cons = _on_device(rb)
    m.zero_grad()
    ll, _ = m.log_likelihood(x, lengths, vcs, spans=rb.spans.cuda(), constraints=cons)
    ll.backward()
    q, leaves = R.params_from_module(m, **st)
    gold = R.gold_factored(q, rb)
    if not discriminative:
        ref = R.grads(leaves, gold.mean())
        np.testing.assert_allclose(ll.item(), gold.mean().item(), rtol=1e-9)
        # the gold score alone never leaves fp64 before the .grad conversion: fp32 rounding of the exact result (1e-6)
        R.assert_grads_close(R.module_grads(m), ref, 1e-6, 'cfg4 gold')
        return
    ref_gold = R.grads(leaves, gold.mean())
    z = R.logz_factored(q, rb)
    ref_z = R.grads(leaves, z.mean())
    ref = {n: ref_gold[n] - ref_z[n] for n in R.PARAMS}
    np.testing.assert_allclose(ll.item(), (gold - z).mean().item(), rtol=1e-6)
    # the two parts cancel: the remainder is held at the bar of the log Z part it carries the error of
    R.assert_grads_close(R.module_grads(m), ref, BAR, 'cfg4 gold - logZ', {n: dict(size=ref_z[n]) for n in R.PARAMS})


# ------------------------------------------------------------------------------------------------ the long ring (K > 512)
def _ring(k, c, seed, lengths, d=32):
    """HSMM-sampled labels with long segments (rates 20..400), K = 520 / 1024, next to short videos of the same task."""
    g = np.random.default_rng(seed)
    n = c + 2
    vc = sorted(int(v) for v in g.permutation(n)[:c])
    sigma = g.uniform(0.7, 1.3, size=d)
    mu = g.normal(0, 0.3, size=(n, d))
    rates = g.uniform(20, 400, size=c)
    xs = []
    for t in lengths:
        out, cur, tot = [], int(g.integers(0, c)), 0
        while tot < t:
            ln = int(np.clip(g.poisson(rates[cur]), 1, k - 1))
            out.append(np.full(ln, cur)); tot += ln; cur = (cur + 1) % c
        lab = np.concatenate(out)[:t]
        xs.append((mu[np.array(vc)[lab]] + sigma * g.standard_normal((t, d))).astype(np.float32))
    m, st = _module(n, d, k, mu + g.normal(0, 0.02, size=mu.shape), sigma ** 2, seed, rate_hi=400)
    return m, st, xs, vc


@pytest.mark.parametrize('k,c,add_eos', [(520, 21, True), (1024, 23, True), (1024, 22, False)])
def test_long_ring_log_likelihood_gradients(k, c, add_eos):
    """K > 512 (the long-ring log Z kernels), T ~ 3000 next to short videos, 21-23 states; and add_eos=False.  The row
    bar, the means with the ring model of the module docstring."""
    lengths = [3000, 700, 2900, 160]
    m, st, xs, vc = _ring(k, c, 500 + k + c, lengths)
    tmax = max(lengths)
    rb = R.RefBatch(_pad(xs, tmax), lengths, vc, None, None, add_eos)
    x, lens, vcs, _ = _on_device(rb)
    with torch.no_grad():
        z_gpu = m.log_partition(x, lens, rb.valid_classes, no_eos=not add_eos).cpu().numpy()
    m.zero_grad()
    ll, _ = m.log_likelihood(x, lens, vcs, spans=None, add_eos=add_eos)
    ll.backward()
    q, leaves = R.params_from_module(m, **st)
    z = R.logz_factored(q, rb)
    ref = R.grads(leaves, z.mean())
    np.testing.assert_allclose(z_gpu, z.detach().numpy(), rtol=1e-6)
    b = len(lengths)
    means = dict(cond=R.means_condition(q, [rb], [np.full(b, 1.0 / b)]), eps=R.ring_eps(min(k, max(lengths))))
    R.assert_grads_close(R.module_grads(m), ref, BAR, 'ring K=%d c=%d eos=%d' % (k, c, add_eos), {'gaussian_means': means})


# ------------------------------------------------------------------------------------------------ the packed training step
def _packed_corpus(seed=9, n_classes=40, d=24, k=40):
    """Seven tasks with overlapping class subsets (three classes merged onto one parameter row, present in several
    tasks), transition constraints with allowed starts / ends (each video's last state added as an allowed end),
    narration-style emission constraints on some batches; 1-2 source batches per task, 2-3 videos each."""
    g = np.random.default_rng(seed)
    merge = {i: (3 if i in (3, 17, 29) else i) for i in range(n_classes)}
    allowed = {i: {j for j in range(n_classes) if g.random() > 0.25} | {i} for i in range(n_classes)}
    mu = g.normal(0, 0.5, size=(n_classes, d))
    sigma = g.uniform(0.7, 1.3, size=d)
    m, st = _module(n_classes, d, k, mu, sigma ** 2, seed, merge_classes=merge,
                allowed_starts=set(range(2, n_classes)), allowed_transitions=allowed,
                allowed_ends=set(range(0, n_classes, 2)))
    tasks = []
    for ti in range(7):
        vc = set(g.choice(n_classes, size=int(g.integers(5, 15)), replace=False).tolist())
        vc |= {3, 17} if ti % 2 == 0 else {29, 5}
        vc = [int(v) for v in g.permutation(sorted(vc))]
        tasks.append(('task%d' % ti, vc))
    batches = []
    for name, vc in tasks:
        for _ in range(int(g.integers(1, 3))):
            b = int(g.integers(2, 4))
            lengths = [int(v) for v in g.integers(50, 300, size=b)]
            tmax = max(lengths)
            xs, cons = [], []
            for t in lengths:
                lab = np.repeat(g.integers(0, len(vc), size=t // 20 + 1), 20)[:t]
                xs.append((mu[[merge[vc[j]] for j in lab]] + sigma * g.standard_normal((t, d))).astype(np.float32))
                cn = np.zeros((t, len(vc)), np.float32)
                j = int(g.integers(0, len(vc)))
                cn[t // 2:, j] = -1e4
                cons.append(cn)
            batches.append(dict(task_name=[name] * b, task_indices=[torch.tensor(vc)] * b, video_name=['%s_%d' % (name, i) for i in range(b)],
                                features=torch.from_numpy(_pad(xs, tmax)), lengths=torch.tensor(lengths),
                                constraints=torch.from_numpy(_pad(cons, tmax)) if g.random() < 0.6 else None,
                                additional=[[vc[-1]] for _ in range(b)]))
    return m, st, batches


@pytest.mark.parametrize('by_index', [False, True])
def test_packed_training_step_against_reference(by_index, monkeypatch):
    """log_likelihood_packed: many tasks in one launch, the parameter gradients scattered into shared rows, the per-batch
    means as one dense product or (BATCH_MEAN_DENSE_MAX = 0) sums by index -- the loss semimarkov.py's packed_group
    backpropagates, -sum(per-batch means) / n_batches, against the reference batch by batch."""
    from action_segmentation_amd.batching import pack_batches
    from action_segmentation_amd import semimarkov_modules
    if by_index:
        monkeypatch.setattr(semimarkov_modules, 'BATCH_MEAN_DENSE_MAX', 0)
    m, st, batches = _packed_corpus()
    assert len({b['task_name'][0] for b in batches}) >= 6
    dev = torch.device('cuda:0')
    pc = pack_batches(batches, dev, m.max_k, constraints_fn=lambda b: b['constraints'],
                      additional_ends_fn=lambda b: b['additional'])
    m.zero_grad()
    ll_p = m.log_likelihood_packed(pc)
    (-ll_p.sum() / len(batches)).backward()
    q, leaves = R.params_from_module(m, **st)
    means, rbs = [], []
    for b in batches:
        rb = R.RefBatch(b['features'], b['lengths'], b['task_indices'][0], b['constraints'], b['additional'], True)
        means.append(R.logz_factored(q, rb).mean())
        rbs.append(rb)
    means = torch.stack(means)
    ref = R.grads(leaves, -means.sum() / len(batches))
    np.testing.assert_allclose(ll_p.detach().cpu().numpy(), means.detach().numpy(), rtol=1e-6)
    got = R.module_grads(m)
    R.assert_grads_close(got, ref, BAR, 'packed by_index=%d' % by_index)
    # the merged row collects the three classes' lengths and means; classes in no task get nothing
    unused = sorted(set(range(m.n_classes)) - {v for b in batches for v in b['task_indices'][0].tolist()} - {3})
    assert not got['gaussian_means'][unused].any() and not got['poisson_log_rates'][unused].any()
    assert not got['gaussian_means'][[17, 29]].any() and got['gaussian_means'][3].any()


# ------------------------------------------------------------------------------------------------ gold scores, golden cases
GOLD_CASES = [(c, True) for c in CASES if CASES[c].get('add_eos', True)] + [('no_eos', False), ('tiny', False)]


@pytest.mark.parametrize('case,add_eos', GOLD_CASES)
@pytest.mark.parametrize('discriminative', [False, True])
def test_gold_score_gradients_on_golden_cases(golden, case, add_eos, discriminative):
    """log_likelihood(spans=...) on the golden cases (with and without EOS): the gold score and gold - log Z, values and
    gradients, against the dense route (sum(scores * to_parts(spans)) and the restated DP, by autograd)."""
    dev = torch.device('cuda:0')
    m = module_from_golden(golden, case).to(dev)
    m.args.sm_train_discriminatively = discriminative
    p, feats, lengths, valid, cons, cfg = case_inputs(golden, case, torch.float64)
    addl = cfg.get('additional') if add_eos else None
    r = O.viterbi_full(p, feats, lengths, valid, add_eos, addl, cons)
    spans = r['spans'][:, :feats.shape[1]]
    rb = R.RefBatch(feats.float(), lengths, valid, None if cons is None else cons.float(), addl, add_eos, spans)
    vcs = None if valid is None else [valid] * feats.shape[0]
    m.zero_grad()
    ll, _ = m.log_likelihood(feats.float().to(dev), lengths.to(dev), vcs, spans=spans.to(dev), add_eos=add_eos,
                             additional_allowed_ends_per_instance=addl,
                             constraints=None if cons is None else cons.float().to(dev))
    ll.backward()
    q, leaves = R.with_leaves(p)              # (the fixture's parameters and masks: what the module was loaded from)
    loss = R.gold_dense(q, rb)
    if discriminative:
        loss = loss - R.logz_dense(q, rb)
    ref = R.grads(leaves, loss.mean())
    np.testing.assert_allclose(ll.item(), loss.mean().item(), rtol=1e-9, atol=1e-6)
    R.assert_grads_close(R.module_grads(m), ref, BAR if discriminative else 1e-6,
                         '%s eos=%d gold%s' % (case, add_eos, ' - logZ' if discriminative else ''))
