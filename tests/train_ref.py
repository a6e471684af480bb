"""Independent fp64 training reference (TEST INFRASTRUCTURE ONLY).

For the module's parameters and a list of single-task batches: log Z per video, gold-span scores, and -- by autograd
-- the gradient of any loss built from them with respect to ``poisson_log_rates``, ``gaussian_means``,
``transition_logits`` and ``init_logits``.  Nothing here reads the package's torch statement of the tables or calls a
HIP op:

* parameters -> tables: fp64 autograd through ``oracle/dense_ref.py`` (``factor_tables``, ``emission_log_probs``,
  ``allowed_ends_for_batch``), on the fp32 values the module holds, converted to fp64;
* the DP, two routes: ``dense`` (``log_hsmm`` + ``semimarkov_dp(LogSemiring)`` with autograd; small lattices only) and
  ``factored`` (the C twin's exact forward-backward, ``oracle.factored.logz(grad=True)``, any size), whose elp / trans /
  init / len gradients are chained back into the parameters by autograd;
* gold scores: ``sum(scores * to_parts(spans))`` on the dense route, sums of table entries and emissions along the spans
  on the factored route.

``assert_rows_close`` is the one comparator the gradient tests use (see its docstring for the bar).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from torch.utils.checkpoint import checkpoint

from oracle import dense_ref as O
from oracle import factored as F

PARAMS = ('poisson_log_rates', 'gaussian_means', 'transition_logits', 'init_logits')
F64 = torch.float64


class RefBatch:
    """One single-task batch as the module is handed it.

    features  b x Tmax x D (fp32 values; Tmax = the batch's longest video: it sets kp = min(K, Tmax))
    lengths   b
    valid_classes  global ids of the task's states (None: all classes)
    constraints    b x Tmax x C additive emission constraints (or None)
    additional_ends  per instance, global ids added to the module's allowed ends (or None)
    add_eos   False: the reference's add_eos=False
    spans     gold span encoding, b x Tmax global ids (-1 = continuation), or None
    """

    def __init__(self, features, lengths, valid_classes=None, constraints=None, additional_ends=None, add_eos=True,
                 spans=None):
        self.features = torch.as_tensor(features).float()
        self.lengths = torch.as_tensor(lengths).long()
        self.valid_classes = None if valid_classes is None else torch.as_tensor(valid_classes).long().cpu()
        self.constraints = None if constraints is None else torch.as_tensor(constraints).float()
        self.additional_ends = additional_ends
        self.add_eos = add_eos
        self.spans = None if spans is None else torch.as_tensor(spans).long().cpu()
        assert int(self.lengths.max()) == self.features.shape[1]


# --------------------------------------------------------------------------------------------------- parameters
def with_leaves(p):
    """A copy of RefParams ``p`` in fp64 whose four trained parameters are fresh autograd leaves -> (params, leaves)."""
    q = p.to(F64)
    leaves = {n: getattr(q, n).detach().clone().requires_grad_(True) for n in PARAMS}
    for n, v in leaves.items():
        setattr(q, n, v)
    q.gaussian_cov_diag = q.gaussian_cov_diag.detach().clone()
    return q, leaves


def masks_from_sets(n_classes, allowed_starts, allowed_transitions):
    """(init mask [n], transition mask [n, n] [to, from]; True = forbidden) from the sets a module is constructed with,
    as the reference builds them (semimarkov_modules.py:169-191): everything forbidden, then the listed starts and
    every listed (src -> tgt) allowed."""
    ic = torch.ones(n_classes, dtype=torch.bool)
    ic[sorted(int(v) for v in allowed_starts)] = False
    tc = torch.ones(n_classes, n_classes, dtype=torch.bool)
    for src, targets in allowed_transitions.items():
        for tgt in targets:
            tc[int(tgt), int(src)] = False
    return ic, tc


def params_from_module(m, allowed_starts=None, allowed_transitions=None, allowed_ends=None, merge_classes=None):
    """RefParams holding the module's fp32 parameter values (what its kernels read) converted to fp64, as leaves.
    The structure -- masks, allowed ends, merged rows -- comes from the same sets the test gave the module's
    constructor, built here (``masks_from_sets``), not read back from the module: the module's own mask building is
    under test too.  A module carrying structure the caller did not name is an error."""
    assert (getattr(m, 'transition_constraints', None) is None) == (allowed_transitions is None), \
        "pass the module's allowed starts / transitions / ends"
    assert (m.merge_classes is None) == (merge_classes is None), "pass the module's merge_classes"
    get = lambda t: t.detach().cpu()
    ic = tc = None
    if allowed_transitions is not None:
        ic, tc = masks_from_sets(m.n_classes, allowed_starts, allowed_transitions)
    p = O.RefParams(m.n_classes, get(m.poisson_log_rates), get(m.gaussian_means),
                    torch.diagonal(get(m.gaussian_cov)).clone(), get(m.transition_logits), get(m.init_logits), m.max_k,
                    bool(m.allow_self_transitions), ic, tc, None if allowed_ends is None else set(allowed_ends),
                    None if merge_classes is None else dict(merge_classes))
    return with_leaves(p)


def tables(p, valid_classes):
    """(trans C x C [to, from], init C, len K x C, merged parameter rows) by autograd through dense_ref."""
    return O.factor_tables(p, valid_classes)


def emission(p, merged, rb, chunk=256):
    """elp b x Tmax x C (fp64, constraints added) by dense_ref.emission_log_probs, in checkpointed slabs of frames so that
    the b x T x C x D intermediate is never held whole (cfg4: D = 200)."""
    x = rb.features.to(F64)
    cons = None if rb.constraints is None else rb.constraints.to(F64)
    mu, var = p.gaussian_means[merged], p.gaussian_cov_diag
    out = []
    for t0 in range(0, x.shape[1], chunk):
        c = None if cons is None else cons[:, t0:t0 + chunk]
        if torch.is_grad_enabled() and mu.requires_grad:
            out.append(checkpoint(O.emission_log_probs, x[:, t0:t0 + chunk], mu, var, c, use_reentrant=False))
        else:
            out.append(O.emission_log_probs(x[:, t0:t0 + chunk], mu, var, c))
    return torch.cat(out, 1)


def allowed_ends(p, rb):
    if not rb.add_eos:
        return None
    return O.allowed_ends_for_batch(p, rb.valid_classes, rb.additional_ends, rb.features.shape[0])


# --------------------------------------------------------------------------------------------------- log Z
def logz_dense(p, rb):
    """log Z per video: dense potentials (log_hsmm) + the restated pytorch-struct DP, differentiable."""
    trans, init, lens, merged = tables(p, rb.valid_classes)
    elp = emission(p, merged, rb)
    scores = O.log_hsmm(trans, elp, init, lens, rb.lengths, add_eos=rb.add_eos, allowed_ends_per_instance=allowed_ends(p, rb))
    z, _ = O.semimarkov_dp(scores, rb.lengths + 1 if rb.add_eos else rb.lengths, O.LogSemiring)
    return z


def _twin(elp, trans, init, lens, lengths, endpen, no_eos, starts=False):
    """[(logZ [1], gradients with upstream 1)] per video: one twin call each on ``host_cores()`` threads."""
    e, tr, ini, ln = (t.detach().numpy() for t in (elp, trans, init, lens))
    lengths = np.asarray(lengths, np.int64)

    def one(i):
        ep = None if endpen is None else endpen[i:i + 1]
        return F.logz(e[i:i + 1], lengths[i:i + 1], tr, ini, ln, ep, grad=True, no_eos=no_eos, starts=starts)
    with ThreadPoolExecutor(max_workers=max(1, min(F.host_cores(), len(lengths)))) as ex:
        return list(ex.map(one, range(len(lengths))))


class _TwinLogZ(torch.autograd.Function):
    """log Z of every video by the C twin; backward = the twin's exact posteriors times the upstream gradient.
    One twin call per video on a pool of ``host_cores()`` threads (ctypes drops the GIL; the twin's log Z is serial),
    each with upstream 1; the backward weights and sums them."""

    @staticmethod
    def forward(ctx, elp, trans, init, lens, lengths, endpen, no_eos):
        ctx.res = res = _twin(elp, trans, init, lens, lengths, endpen, no_eos)
        return torch.tensor([float(z[0]) for z, _ in res], dtype=F64)

    @staticmethod
    def backward(ctx, gz):
        gz = gz.detach().numpy()
        g0 = ctx.res[0][1]
        ge = np.concatenate([gz[i] * g['elp'] for i, (_, g) in enumerate(ctx.res)], 0)
        gt, gi, gl = np.zeros_like(g0['trans']), np.zeros_like(g0['init']), np.zeros_like(g0['len'])
        for i, (_, g) in enumerate(ctx.res):
            gt += gz[i] * g['trans']
            gi += gz[i] * g['init']
            gl += gz[i] * g['len']
        return torch.from_numpy(ge), torch.from_numpy(gt), torch.from_numpy(gi), torch.from_numpy(gl), None, None, None


def kp_of(lens, rb):
    """Rows of the length table the DP reads: kp = min(K, Tmax of the batch) (the twin's ``len_scores[:tmax]``)."""
    return min(lens.shape[0], rb.features.shape[1])


def logz_factored(p, rb):
    """log Z per video on the C twin, differentiable (the tables' gradients chained back by autograd)."""
    trans, init, lens, merged = tables(p, rb.valid_classes)
    elp = emission(p, merged, rb)
    b, c = elp.shape[0], elp.shape[2]
    ep = F.endpen_from_allowed_ends(allowed_ends(p, rb), b, c)
    return _TwinLogZ.apply(elp, trans, init, lens[:kp_of(lens, rb)], rb.lengths.numpy(), ep, not rb.add_eos)


def logz(p, rb, route):
    return {'dense': logz_dense, 'factored': logz_factored}[route](p, rb)


def means_condition(p, batches, weights):
    """Condition sum of the mean gradients of  L = sum_b sum_i weights[b][i] * logZ_bi  ([n_classes, D]):

        cond[m, d] = sum |w_i| (p_t(c) + 2 started_t(c)) |x_td - mu_md| / var_d   over videos, frames, states c on row m

    with the twin's exact posteriors: p_t(c) the occupancy, started_t(c) the expected number of spans of c started up
    to t.  A mean gradient sum_t p_t(c) (x_td - mu_cd) / var_d cancels (a class mean its frames sit around: ~sqrt(n)
    from n terms of size ~1), and the kernels form p_t(c) as spans started minus spans ended up to t
    (csrc/smm_logz_bwd.hip), so a relative error eps of the span posteriors moves the entry by up to eps * cond."""
    n, d = p.gaussian_means.shape
    cond = np.zeros((n, d))
    var = p.gaussian_cov_diag.detach().numpy()
    for rb, w in zip(batches, weights):
        with torch.no_grad():
            trans, init, lens, merged = tables(p, rb.valid_classes)
            elp = emission(p, merged, rb)
            b, _, c = elp.shape
            ep = F.endpen_from_allowed_ends(allowed_ends(p, rb), b, c)
            res = _twin(elp, trans, init, lens[:kp_of(lens, rb)], rb.lengths.numpy(), ep, not rb.add_eos, starts=True)
        mv = merged.numpy()
        mu = p.gaussian_means.detach().numpy()[mv]                                  # C x D
        for i, t in enumerate(rb.lengths.tolist()):
            g = res[i][1]
            weight = g['elp'][0, :t] + 2.0 * np.cumsum(g['start'][0, :t], axis=0)  # T x C
            x = rb.features[i, :t].double().numpy()
            for j in range(c):
                cond[mv[j]] += abs(float(w[i])) * (weight[:, j] @ np.abs(x - mu[j])) / var
    return cond


def ring_eps(kp):
    """Relative error of the log Z kernels' span posteriors the means model allows: 1/12 of the fp32 ring sums' documented
    worst case kp * 2^-24 (csrc/smm_logz.hip, "Accuracy": a slot sums up to kp terms).  Calibrated on MI355X: cfg4
    (kp = 64) needs 1/105 of it, the long rings (kp = 520, 1024) up to 1/25."""
    return kp * 2.0 ** -24 / 12


# --------------------------------------------------------------------------------------------------- gold scores
def _local_spans(rb, c):
    """Gold spans as local state ids; with EOS, the EOS label (local C) at each video's end (as the module adds it)."""
    vc = None if rb.valid_classes is None else rb.valid_classes.tolist()
    loc = {(i if vc is None else g): i for i, g in enumerate(range(c) if vc is None else vc)}
    b, tmax = rb.spans.shape
    out = torch.full((b, tmax + 1), -1, dtype=torch.int64)
    for i, t in enumerate(rb.lengths.tolist()):
        for n in range(t):
            s = int(rb.spans[i, n])
            out[i, n] = -1 if s == -1 else loc[s]
        if rb.add_eos:
            out[i, t] = c
    return out if rb.add_eos else out[:, :tmax]


def gold_dense(p, rb):
    """sum(scores * to_parts(spans)) per video on the dense potentials (torch_struct ``score``), differentiable."""
    trans, init, lens, merged = tables(p, rb.valid_classes)
    elp = emission(p, merged, rb)
    scores = O.log_hsmm(trans, elp, init, lens, rb.lengths, add_eos=rb.add_eos, allowed_ends_per_instance=allowed_ends(p, rb))
    return O.rescore(scores, _local_spans(rb, trans.shape[0]), rb.lengths + 1 if rb.add_eos else rb.lengths)


def gold_factored(p, rb):
    """The same score as sums along the spans: init of the first label; per span its length entry and the emissions of
    its frames; the transition into each next label; with EOS the end penalty of the last label; without EOS the last
    span has no edge (to_parts), only its label's emission of the last frame when it starts there."""
    trans, init, lens, merged = tables(p, rb.valid_classes)
    elp = emission(p, merged, rb)
    c = trans.shape[0]
    kp = kp_of(lens, rb)
    ends = allowed_ends(p, rb)
    sp = _local_spans(rb, c)
    out = []
    for i, t in enumerate(rb.lengths.tolist()):
        row = sp[i, :t].tolist()
        starts = [n for n, s in enumerate(row) if s != -1]
        assert starts and starts[0] == 0
        labs = [row[s] for s in starts]
        bounds = starts + [t]
        n_scored = len(labs) - 1 if not rb.add_eos else len(labs)
        terms = [elp.new_zeros(())]
        if n_scored > 0:
            terms.append(init[labs[0]])
        for j in range(n_scored):
            k = bounds[j + 1] - bounds[j]
            assert 1 <= k <= kp - 1, (k, kp)
            terms.append(lens[k, labs[j]] + elp[i, bounds[j]:bounds[j + 1], labs[j]].sum())
            if j + 1 < len(labs):
                terms.append(trans[labs[j + 1], labs[j]])
        if not rb.add_eos:
            if bounds[-2] == t - 1:
                terms.append(elp[i, t - 1, labs[-1]])
        elif ends is not None and labs[-1] not in ends[i]:
            terms.append(elp.new_tensor(O.BIG_NEG))
        out.append(torch.stack(terms).sum())
    return torch.stack(out)


def gold(p, rb, route):
    return {'dense': gold_dense, 'factored': gold_factored}[route](p, rb)


# --------------------------------------------------------------------------------------------------- gradients
def grads(leaves, loss):
    """d loss / d leaves as numpy fp64 (zeros where the loss does not depend on a parameter)."""
    for v in leaves.values():
        v.grad = None
    loss.backward()
    return {n: (v.grad.numpy().copy() if v.grad is not None else np.zeros(tuple(v.shape))) for n, v in leaves.items()}


def module_grads(m):
    """The module's .grad of the four trained parameters as numpy fp64 (zeros where none was formed)."""
    return {n: (getattr(m, n).grad.detach().cpu().double().numpy() if getattr(m, n).grad is not None
                else np.zeros(tuple(getattr(m, n).shape))) for n in PARAMS}


# --------------------------------------------------------------------------------------------------- the comparator
OLD_BAR = 5e-4       # what the module gradient tests held before: rtol 5e-4, atol 5e-4 * max(1, max|ref|)


def row_errors(got, ref, bar, cond=None, eps=0.0, size=None):
    """-> (worst |got - ref| / allowed over all entries, list of (row, why) failures).

    Rows are the first axis (a 1-D tensor: every entry its own row).  An entry passes when
        |got - ref| <= bar * (|ref| + max(max|ref[row]|, 1e-2 * max|ref|)),
    i.e. each row is held to its own size, not the largest entry of the tensor: a rarely used class or a rarely taken
    transition is checked as tightly as a busy one, down to 1e-2 of the largest.  A row whose reference is exactly zero
    (a class in no group, a row no path reaches) must be exactly zero.

    ``size``: the magnitudes the bar scales with, where they are not the reference's own (default |ref|): a difference
    of two gradients that cancel (gold - log Z) is held to the size of the part the kernels compute.
    ``cond`` / ``eps``: an error model on top (``means_condition``): + eps * cond per entry, for gradients formed from
    posteriors that are themselves only accurate to eps relative.  Never looser than OLD_BAR * (|ref| + max(1, max|ref|)),
    the bar the module gradient tests held before."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    g2 = got.reshape(got.shape[0], -1) if got.ndim > 1 else got.reshape(-1, 1)
    r2 = ref.reshape(ref.shape[0], -1) if ref.ndim > 1 else ref.reshape(-1, 1)
    bad = []
    if not np.all(np.isfinite(g2)):
        bad.append((int(np.flatnonzero(~np.isfinite(g2).all(1))[0]), 'not finite'))
        return float('inf'), bad
    gmax = float(np.abs(r2).max()) if r2.size else 0.0
    rowmax = np.abs(r2).max(1, keepdims=True)
    zero = rowmax[:, 0] == 0
    zero_bad = np.flatnonzero(zero & (g2 != 0).any(1)).tolist()
    for r in zero_bad:
        bad.append((r, 'reference row is exactly zero, got max |%.3e|' % np.abs(g2[r]).max()))
    s2 = np.abs(r2) if size is None else np.abs(np.asarray(size, np.float64).reshape(r2.shape))
    allowed = bar * (s2 + np.maximum(s2.max(1, keepdims=True), 1e-2 * s2.max()))
    if cond is not None:
        allowed = allowed + eps * np.asarray(cond, np.float64).reshape(r2.shape)
    if size is not None or cond is not None:
        allowed = np.minimum(allowed, OLD_BAR * (np.abs(r2) + max(1.0, gmax)))
    ratio = np.where(zero[:, None], 0.0, np.abs(g2 - r2) / np.where(allowed > 0, allowed, 1.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    for r in np.flatnonzero((ratio > 1.0).any(1)).tolist():
        j = int(np.argmax(ratio[r]))
        bad.append((r, 'entry %d: got %.9e ref %.9e (%.3g of the bar)' % (j, g2[r, j], r2[r, j], ratio[r, j])))
    if zero_bad:
        worst = float('inf')
    return worst, bad


def assert_rows_close(got, ref, bar, name='', cond=None, eps=0.0, size=None):
    """The comparator of every gradient test (see ``row_errors``).  Returns the worst error as a fraction of the bar;
    with an error model, also printed: the worst as a fraction of the plain row bar."""
    worst, bad = row_errors(got, ref, bar, cond, eps, size)
    extra = ''
    if cond is not None or size is not None:
        extra = ' (plain row bar: %.3g; model:%s%s)' % (row_errors(got, ref, bar)[0], ' size' if size is not None else '',
                                                     ' + %.2e cond' % eps if cond is not None else '')
    print('\n[train_ref] %-50s worst %.3g of bar %.0e%s' % (name, worst, bar, extra))
    assert not bad, '%s (bar %g): %d rows fail, first %s' % (name, bar, len(bad), bad[:4])
    return worst


def assert_grads_close(got, ref, bar, label='', models=None):
    """assert_rows_close over the four parameters -> {name: worst fraction of the bar}.  ``models``: {name: dict(cond=,
    eps=, size=)} for the parameters an error model applies to (every other one is held to the plain row bar)."""
    models = models or {}
    return {n: assert_rows_close(got[n], ref[n], bar, '%s %s' % (label, n), **models.get(n, {})) for n in PARAMS}
