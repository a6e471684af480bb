"""Transcript likelihood with optional entries, log Z_o, and its gradients (include/smmdp.h: smm_align_opt_logz_f64), by routes
that share no code with the kernels or with each other:

  torch_logz_opt   the forward recursion of the header restated in fp64 torch on the CPU with torch.logsumexp, every cell of
                   every column; autograd through it gives the four gradients.
  forward_backward the header's forward AND backward recursions in fp64 numpy, every cell: S, E, p_used, the identity.
  twin_grads_opt   the C twin's exact forward-backward (oracle.factored.logz(grad=True)) on the expanded lattice of
                   tests/align_optional_ref.py -- states = transcript positions, every entry -1e9 except those the transcript
                   allows -- with its gradients scattered back to classes.  Finite tables only.
  brute_logz_opt   the sum over every subset of the optional entries and every composition of T into the kept entries.
  is_ambiguous_brute  two different subsets with the same non-empty class sequence, by enumeration."""
import itertools

import numpy as np
import torch

import align_optional_ref as AO
from transcript_ref import _lse_rows

NEG_INF = float('-inf')


def _closing(endpen, c):
    return 0.0 if endpen is None else endpen[c]


def torch_logz_opt(elp, a, opt, trans, init, len_scores, kp, endpen=None):
    """One video, torch fp64 tensors (with requires_grad where a gradient is wanted): elp [T, C], a: local ids, opt: one flag
    per entry, trans [C, C] ([to][from]), init [C], len_scores [K, C], kp: lengths 1 .. kp - 1 are usable, endpen [C] or None.
    -> log Z_o, a 0-d tensor (-inf without an alignment)."""
    T, C = elp.shape
    a = [int(v) for v in a]
    M = len(a)
    if not AO.feasible_by_count(T, opt, kp) or any(v < 0 or v >= C for v in a):
        return torch.tensor(NEG_INF, dtype=torch.float64)
    pred_lo, first, end, _ = AO.structure(opt)
    kw = min(kp - 1, T)
    cum = torch.cat([torch.zeros((1, C), dtype=torch.float64), torch.cumsum(elp, dim=0)])
    pad = torch.full((kw,), NEG_INF, dtype=torch.float64)
    edge = torch.full((1,), NEG_INF, dtype=torch.float64)
    gams = []
    for m in range(M):
        c = a[m]
        h0 = init[c].reshape(1) if first[m] else edge
        if m > 0 and T > 1:
            terms = torch.stack([gams[j][1:T] + trans[c, a[j]] for j in range(pred_lo[m], m)], dim=1)
            inner = _lse_rows(terms) - cum[1:T, c]
        else:
            inner = torch.full((T - 1,), NEG_INF, dtype=torch.float64)
        h = torch.cat([h0, inner, edge])
        # window n = h[n - kw .. n - 1]: entry j is the source at distance k = kw - j
        win = torch.cat([pad, h]).unfold(0, kw, 1)[:T + 1]
        gams.append(cum[:, c] + _lse_rows(win + len_scores[1:kw + 1, c].flip(0).unsqueeze(0)))
    last = torch.stack([gams[j][T] + _closing(endpen, a[j]) for j in range(M) if end[j]])
    return _lse_rows(last.unsqueeze(0))[0]


def torch_grads_opt(elp, a, opt, trans, init, len_scores, kp, endpen=None):
    """numpy in -> (log Z_o, dict(elp, trans, init, len)): autograd through ``torch_logz_opt``; zeros when log Z_o = -inf."""
    t = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in (elp, trans, init, len_scores)]
    ep = None if endpen is None else torch.tensor(np.asarray(endpen, np.float64))
    z = torch_logz_opt(t[0], a, opt, t[1], t[2], t[3], kp, ep)
    if not bool(torch.isfinite(z)):
        return float(z.detach()), dict(elp=np.zeros(t[0].shape), trans=np.zeros(t[1].shape), init=np.zeros(t[2].shape),
                                       len=np.zeros(t[3].shape))
    z.backward()
    g = [np.zeros(v.shape) if v.grad is None else v.grad.numpy() for v in t]
    return float(z.detach()), dict(elp=g[0], trans=g[1], init=g[2], len=g[3])


def _lse(x, axis=None):
    x = np.asarray(x, np.float64)
    mx = np.max(x, axis=axis, keepdims=True)
    ref = np.where(np.isfinite(mx), mx, 0.0)
    with np.errstate(divide='ignore'):
        out = ref + np.log(np.sum(np.exp(x - ref), axis=axis, keepdims=True))
    return out.reshape(()) if axis is None else np.squeeze(out, axis=axis)


def forward_backward(elp, a, opt, trans, init, len_scores, kp, endpen=None):
    """The header's two recursions, every cell, in numpy -> dict(logz, ident (lse_first(h[0] + bh[0])), h, gam, bh, bg, S, E
    (each [T + 1, M]), p_used [M] = sum_n E, p_used_S [M] = sum_s S, occ [T, M]); logz -inf: the rest is None."""
    elp = np.asarray(elp, np.float64)
    T, C = elp.shape
    a = [int(v) for v in a]
    M = len(a)
    if not AO.feasible_by_count(T, opt, kp) or any(v < 0 or v >= C for v in a):
        return dict(logz=-np.inf)
    pred_lo, first, end, _ = AO.structure(opt)
    succ = [[m for m in range(j + 1, M) if pred_lo[m] <= j] for j in range(M)]
    kw = min(kp - 1, T)
    cum = np.concatenate([np.zeros((1, C)), np.cumsum(elp, axis=0)])
    h = np.full((T + 1, M), -np.inf)
    gam = np.full((T + 1, M), -np.inf)
    for m in range(M):
        c = a[m]
        if first[m]:
            h[0, m] = init[c]
        for n in range(1, T):
            if m > 0:
                h[n, m] = _lse([gam[n, j] + trans[c, a[j]] for j in range(pred_lo[m], m)]) - cum[n, c]
        for n in range(1, T + 1):
            gam[n, m] = cum[n, c] + _lse([h[n - k, m] + len_scores[k, c] for k in range(1, min(kw, n) + 1)])
    logz = float(_lse([gam[T, j] + _closing(endpen, a[j]) for j in range(M) if end[j]]))
    if not np.isfinite(logz):
        return dict(logz=logz)
    bg = np.full((T + 1, M), -np.inf)
    bh = np.full((T + 1, M), -np.inf)
    for j in range(M):
        if end[j]:
            bg[T, j] = _closing(endpen, a[j])
    for m in range(M - 1, -1, -1):                            # succ(m) lies behind m: its bh columns are complete
        c = a[m]
        if succ[m]:
            for n in range(1, T):
                bg[n, m] = _lse([trans[a[q], c] - cum[n, a[q]] + bh[n, q] for q in succ[m]])
        for s in range(T):
            bh[s, m] = _lse([len_scores[k, c] + cum[s + k, c] + bg[s + k, m] for k in range(1, min(kw, T - s) + 1)])
    S = np.exp(h + bh - logz)
    E = np.exp(gam + bg - logz)
    occ = np.cumsum(S[:T], axis=0) - np.cumsum(E[:T], axis=0)
    ident = float(_lse([h[0, m] + bh[0, m] for m in range(M) if first[m]]))
    return dict(logz=logz, ident=ident, h=h, gam=gam, bh=bh, bg=bg, S=S, E=E, p_used=E.sum(axis=0), p_used_S=S.sum(axis=0),
                occ=occ)


def twin_grads_opt(elp, a, opt, trans, init, len_scores, kp, endpen=None):
    """numpy in -> (log Z_o, dict(elp [T, C], trans [C, C], init [C], len [K, C], p_used [M])) from the C twin on the expanded
    lattice.  Finite tables only (the twin's "impossible" is -1e9)."""
    from oracle import factored as F
    elp = np.asarray(elp, np.float64)
    a = np.asarray(a, np.int64)
    T, C = elp.shape
    M = len(a)
    pred_lo, first, _, _ = AO.structure(opt)
    e2, t2, i2, l2, ep = AO.expanded_lattice(elp, a, opt, trans, init, len_scores, kp, endpen)
    tm = max(T, kp)                                           # (the twin clips its length table to its Tmax)
    pad = np.zeros((1, tm, M))
    pad[0, :T] = e2
    z, g2 = F.logz(pad, np.array([T], np.int64), t2, i2, l2, ep[None], grad=True)
    K = np.asarray(len_scores).shape[0]
    g = dict(elp=np.zeros((T, C)), trans=np.zeros((C, C)), init=np.zeros(C), len=np.zeros((K, C)), p_used=np.zeros(M))
    for m in range(M):
        g['elp'][:, a[m]] += g2['elp'][0, :T, m]
        g['len'][:g2['len'].shape[0], a[m]] += g2['len'][:, m]
        for j in range(pred_lo[m], m):
            g['trans'][a[m], a[j]] += g2['trans'][m, j]
            g['p_used'][m] += g2['trans'][m, j]
        if first[m]:
            g['init'][a[m]] += g2['init'][m]
            g['p_used'][m] += g2['init'][m]
    return float(z[0]), g


def subsets(opt):
    """Every choice of kept entries: tuples of indices (the empty one included)."""
    M = len(opt)
    for keep in itertools.product(*[(False, True) if opt[m] else (True,) for m in range(M)]):
        yield tuple(m for m in range(M) if keep[m])


def brute_logz_opt(elp, a, opt, trans, init, len_scores, kp, endpen=None):
    """-> (log Z_o, frame occupancy [T, C], p_used [M]) by enumeration over subsets x compositions; (-inf, zeros, zeros)
    without an alignment."""
    elp = np.asarray(elp, np.float64)
    T, C = elp.shape
    M = len(a)
    scores, occs, useds = [], [], []
    for idx in subsets(opt):
        S = len(idx)
        if not 1 <= S <= T:
            continue
        for cuts in itertools.combinations(range(1, T), S - 1):
            b = (0,) + cuts + (T,)
            if any(b[i + 1] - b[i] > kp - 1 for i in range(S)):
                continue
            s = init[a[idx[0]]] + _closing(endpen, a[idx[-1]])
            occ, used = np.zeros((T, C)), np.zeros(M)
            for i, m in enumerate(idx):
                s += elp[b[i]:b[i + 1], a[m]].sum() + len_scores[b[i + 1] - b[i], a[m]]
                occ[b[i]:b[i + 1], a[m]] = 1.0
                used[m] = 1.0
                if i > 0:
                    s += trans[a[m], a[idx[i - 1]]]
            scores.append(s)
            occs.append(occ)
            useds.append(used)
    if not scores or not np.isfinite(np.max(scores)):
        return -np.inf, np.zeros((T, C)), np.zeros(M)
    scores = np.array(scores)
    mx = scores.max()
    w = np.exp(scores - mx)
    p = w / w.sum()
    return float(mx + np.log(w.sum())), np.tensordot(p, np.array(occs), axes=1), np.tensordot(p, np.array(useds), axes=1)


def reduced_transcripts(a, opt):
    """The class sequences of every non-empty subset, as lists (with repeats where two subsets agree)."""
    return [[int(a[m]) for m in idx] for idx in subsets(opt) if idx]


def is_ambiguous_brute(a, opt):
    seqs = [tuple(s) for s in reduced_transcripts(a, opt)]
    return len(set(seqs)) != len(seqs)


def crosstask(steps, bg, bg_optional, steps_optional):
    """bg, step_1, bg, ..., step_S, bg -> (ids, flags)."""
    ids, flags = [bg], [bg_optional]
    for s in steps:
        ids += [s, bg]
        flags += [steps_optional, bg_optional]
    return ids, flags
