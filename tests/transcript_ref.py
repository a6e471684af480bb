"""Transcript likelihood log Z_a = log sum_{y : classes(y) = a} exp score(y) and its gradients (include/smmdp.h:
smm_align_logz_f64), by three routes that share no code with the kernels or with each other:

  torch_logz   the recursion of the header restated in fp64 torch on the CPU with torch.logsumexp, every cell of every column;
               autograd through it gives the four gradients.
  twin_logz    the C twin's exact forward-backward (oracle.factored.logz(grad=True)) on the expanded lattice of
               tests/align_ref.py -- states = transcript positions, every entry -1e9 except the transcript's own (exp(-1e9) is
               0 in fp64: the other paths add nothing) -- with column m of its gradients scattered back to class a_m.
  brute_logz   the sum over every composition of T into M parts of 1 .. kp - 1 (tiny cases)."""
import itertools

import numpy as np
import torch

import align_ref as R

NEG_INF = float('-inf')


def _lse_rows(x):
    """logsumexp over dim 1 whose rows of only -inf give -inf AND pass no NaN back (torch's own backward forms inf - inf)."""
    dead = torch.isinf(x.max(dim=1).values) & (x.max(dim=1).values < 0)
    safe = torch.where(dead.unsqueeze(1), torch.zeros_like(x), x)
    return torch.where(dead, torch.full_like(x[:, 0], NEG_INF), torch.logsumexp(safe, dim=1))


def torch_logz(elp, a, trans, init, len_scores, kp, closing=0.0):
    """One video, torch fp64 tensors (with requires_grad where a gradient is wanted): elp [T, C], a: local ids, trans [C, C]
    ([to][from]), init [C], len_scores [K, C], kp: lengths 1 .. kp - 1 are usable.  -> log Z_a, a 0-d tensor (-inf without a
    segmentation)."""
    T, C = elp.shape
    a = [int(v) for v in a]
    M = len(a)
    if not R.feasible_by_count(T, M, kp) or any(v < 0 or v >= C for v in a):
        return torch.tensor(NEG_INF, dtype=torch.float64)
    kw = min(kp - 1, T)
    cum = torch.cat([torch.zeros((1, C), dtype=torch.float64), torch.cumsum(elp, dim=0)])
    pad = torch.full((kw,), NEG_INF, dtype=torch.float64)
    h = torch.cat([init[a[0]].reshape(1), torch.full((T,), NEG_INF, dtype=torch.float64)])
    gam = None
    for m in range(M):
        c = a[m]
        # window n = h[n - kw .. n - 1]: entry j is the source at distance k = kw - j
        win = torch.cat([pad, h]).unfold(0, kw, 1)[:T + 1]
        gam = cum[:, c] + _lse_rows(win + len_scores[1:kw + 1, c].flip(0).unsqueeze(0))
        if m + 1 < M:
            cn = a[m + 1]
            inner = gam[1:T] + trans[cn, c] - cum[1:T, cn]
            edge = torch.full((1,), NEG_INF, dtype=torch.float64)
            h = torch.cat([edge, inner, edge])
    return gam[T] + closing


def torch_grads(elp, a, trans, init, len_scores, kp, closing=0.0):
    """numpy in -> (log Z_a, dict(elp, trans, init, len)): autograd through ``torch_logz``; zeros when log Z_a = -inf."""
    t = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in (elp, trans, init, len_scores)]
    z = torch_logz(t[0], a, t[1], t[2], t[3], kp, closing)
    if not bool(torch.isfinite(z)):
        return float(z.detach()), dict(elp=np.zeros(t[0].shape), trans=np.zeros(t[1].shape), init=np.zeros(t[2].shape),
                              len=np.zeros(t[3].shape))
    z.backward()
    g = [np.zeros(v.shape) if v.grad is None else v.grad.numpy() for v in t]
    return float(z.detach()), dict(elp=g[0], trans=g[1], init=g[2], len=g[3])


def twin_grads(elp, a, trans, init, len_scores, kp, closing=0.0):
    """numpy in -> (log Z_a, dict(elp [T, C], trans [C, C], init [C], len [K, C])) from the C twin on the expanded lattice.
    Finite tables only (the twin's "impossible" is -1e9)."""
    from oracle import factored as F
    elp = np.asarray(elp, np.float64)
    a = np.asarray(a, np.int64)
    T, C = elp.shape
    M = len(a)
    e2, t2, i2, l2, ep = R.expanded_lattice(elp, a, trans, init, len_scores, kp, closing)
    tm = max(T, kp)                                           # (the twin clips its length table to its Tmax)
    pad = np.zeros((1, tm, M))
    pad[0, :T] = e2
    z, g2 = F.logz(pad, np.array([T], np.int64), t2, i2, l2, ep[None], grad=True)
    K = np.asarray(len_scores).shape[0]
    g = dict(elp=np.zeros((T, C)), trans=np.zeros((C, C)), init=np.zeros(C), len=np.zeros((K, C)))
    for m in range(M):
        g['elp'][:, a[m]] += g2['elp'][0, :T, m]
        g['len'][:g2['len'].shape[0], a[m]] += g2['len'][:, m]
        if m > 0:
            g['trans'][a[m], a[m - 1]] += g2['trans'][m, m - 1]
    g['init'][a[0]] += g2['init'][0]
    return float(z[0]), g


def compositions(T, M, kp):
    for cuts in itertools.combinations(range(1, T), M - 1):
        b = (0,) + cuts + (T,)
        if all(b[m + 1] - b[m] <= kp - 1 for m in range(M)):
            yield b


def brute_logz(elp, a, trans, init, len_scores, kp, closing=0.0):
    """-> (log Z_a, frame occupancy [T, C]) by enumeration; (-inf, zeros) without a segmentation."""
    elp = np.asarray(elp, np.float64)
    T, C = elp.shape
    M = len(a)
    scores, occs = [], []
    if 1 <= M <= T:
        for b in compositions(T, M, kp):
            s = init[a[0]] + closing
            occ = np.zeros((T, C))
            for m in range(M):
                s += elp[b[m]:b[m + 1], a[m]].sum() + len_scores[b[m + 1] - b[m], a[m]]
                occ[b[m]:b[m + 1], a[m]] = 1.0
                if m > 0:
                    s += trans[a[m], a[m - 1]]
            scores.append(s)
            occs.append(occ)
    if not scores or not np.isfinite(np.max(scores)):
        return -np.inf, np.zeros((T, C))
    scores = np.array(scores)
    mx = scores.max()
    w = np.exp(scores - mx)
    z = mx + np.log(w.sum())
    return float(z), np.tensordot(w / w.sum(), np.array(occs), axes=1)


def counts(a, C):
    """(transition counts [C, C] ([to][from]), start indicator [C], entries per class [C]) of a transcript."""
    tr, st, n = np.zeros((C, C)), np.zeros(C), np.zeros(C)
    st[a[0]] = 1.0
    for m, c in enumerate(a):
        n[c] += 1.0
        if m > 0:
            tr[c, a[m - 1]] += 1.0
    return tr, st, n
