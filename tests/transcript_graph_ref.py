"""Transcript-graph likelihood, log Z_g, its gradients and the node / end posteriors (include/smmdp.h:
smm_align_graph_logz_f64), by routes that share no code with the kernels or with each other.  A graph is
(a, pred, start, end): ids [M], bool [M, M] strictly lower triangular, bool [M], bool [M] (tests/align_graph_ref.py).

  torch_logz_graph   (a) the forward recursion of the header restated in fp64 torch on the CPU with torch.logsumexp, every cell
                     of every column; autograd through it gives the four gradients.
  forward_backward   (b) the header's forward AND backward recursions in fp64 numpy, every cell: S, E, p_used, p_end, the
                     identity, the gradients as sums of posteriors.
  twin_grads_graph   (c) the C twin's exact forward-backward (oracle.factored.logz(grad=True)) on
                     align_graph_ref.expanded_lattice -- states = nodes, every entry -1e9 except those the graph allows -- with
                     its gradients scattered back to classes.  Finite tables only.
  brute_logz_graph   (d) the sum over every start -> end path and every composition of T into its nodes.
  is_ambiguous_brute (e) two different start -> end paths with the same class sequence, by enumeration."""
import itertools

import numpy as np
import torch

import align_graph_ref as AG
from transcript_optional_ref import _lse
from transcript_ref import _lse_rows

NEG_INF = float('-inf')


def _closing(endpen, c):
    return 0.0 if endpen is None else endpen[c]


def _graph(graph):
    a, pred, start, end = graph
    return [int(v) for v in a], np.asarray(pred) != 0, np.asarray(start) != 0, np.asarray(end) != 0


def has_alignment_by_count(T, C, graph, kp):
    a, pred, start, end = _graph(graph)
    return AG.structure_ok(a, pred, C) and AG.feasible_by_count(T, pred, start, end, kp)


def torch_logz_graph(elp, graph, trans, init, len_scores, kp, endpen=None):
    """One video, torch fp64 tensors (with requires_grad where a gradient is wanted): elp [T, C], trans [C, C] ([to][from]),
    init [C], len_scores [K, C], kp: lengths 1 .. kp - 1 are usable, endpen [C] or None.  -> log Z_g, a 0-d tensor (-inf
    without an alignment)."""
    T, C = elp.shape
    a, pred, start, end = _graph(graph)
    M = len(a)
    if not has_alignment_by_count(T, C, graph, kp):
        return torch.tensor(NEG_INF, dtype=torch.float64)
    kw = min(kp - 1, T)
    cum = torch.cat([torch.zeros((1, C), dtype=torch.float64), torch.cumsum(elp, dim=0)])
    pad = torch.full((kw,), NEG_INF, dtype=torch.float64)
    edge = torch.full((1,), NEG_INF, dtype=torch.float64)
    gams = []
    for m in range(M):
        c = a[m]
        h0 = init[c].reshape(1) if start[m] else edge
        p = [j for j in range(m) if pred[m, j]]
        if p and T > 1:
            terms = torch.stack([gams[j][1:T] + trans[c, a[j]] for j in p], dim=1)
            inner = _lse_rows(terms) - cum[1:T, c]
        else:
            inner = torch.full((T - 1,), NEG_INF, dtype=torch.float64)
        h = torch.cat([h0, inner, edge])
        win = torch.cat([pad, h]).unfold(0, kw, 1)[:T + 1]    # window n = h[n - kw .. n - 1]
        gams.append(cum[:, c] + _lse_rows(win + len_scores[1:kw + 1, c].flip(0).unsqueeze(0)))
    last = torch.stack([gams[j][T] + _closing(endpen, a[j]) for j in range(M) if end[j]])
    return _lse_rows(last.unsqueeze(0))[0]


def torch_grads_graph(elp, graph, trans, init, len_scores, kp, endpen=None):
    """numpy in -> (log Z_g, dict(elp, trans, init, len)): autograd through ``torch_logz_graph``; zeros when log Z_g = -inf."""
    t = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in (elp, trans, init, len_scores)]
    ep = None if endpen is None else torch.tensor(np.asarray(endpen, np.float64))
    z = torch_logz_graph(t[0], graph, t[1], t[2], t[3], kp, ep)
    if not bool(torch.isfinite(z)):
        return float(z.detach()), dict(elp=np.zeros(t[0].shape), trans=np.zeros(t[1].shape), init=np.zeros(t[2].shape),
                                       len=np.zeros(t[3].shape))
    z.backward()
    g = [np.zeros(v.shape) if v.grad is None else v.grad.numpy() for v in t]
    return float(z.detach()), dict(elp=g[0], trans=g[1], init=g[2], len=g[3])


def forward_backward(elp, graph, trans, init, len_scores, kp, endpen=None):
    """The header's two recursions, every cell, in numpy -> dict(logz, ident (lse_start(h[0] + bh[0])), h, gam, bh, bg, S, E
    (each [T + 1, M]), p_used [M] = sum_n E, p_used_S [M] = sum_s S, p_end [M], occ [T, M], and the gradients as the header
    sums them: elp [T, C], trans [C, C], init [C], len [K, C]); logz -inf: only logz."""
    elp = np.asarray(elp, np.float64)
    trans, init, len_scores = (np.asarray(x, np.float64) for x in (trans, init, len_scores))
    T, C = elp.shape
    a, pred, start, end = _graph(graph)
    M = len(a)
    if not has_alignment_by_count(T, C, graph, kp):
        return dict(logz=-np.inf)
    succ = [[m for m in range(j + 1, M) if pred[m, j]] for j in range(M)]
    kw = min(kp - 1, T)
    cum = np.concatenate([np.zeros((1, C)), np.cumsum(elp, axis=0)])
    h = np.full((T + 1, M), -np.inf)
    gam = np.full((T + 1, M), -np.inf)
    for m in range(M):
        c = a[m]
        p = [j for j in range(m) if pred[m, j]]
        if start[m]:
            h[0, m] = init[c]
        if p:
            for n in range(1, T):
                h[n, m] = _lse([gam[n, j] + trans[c, a[j]] for j in p]) - cum[n, c]
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
    ident = float(_lse([h[0, m] + bh[0, m] for m in range(M) if start[m]]))
    p_end = np.array([np.exp(gam[T, j] + _closing(endpen, a[j]) - logz) if end[j] else 0.0 for j in range(M)])
    g_elp, g_trans, g_init, g_len = np.zeros((T, C)), np.zeros((C, C)), np.zeros(C), np.zeros(len_scores.shape)
    for m in range(M):
        c = a[m]
        g_elp[:, c] += occ[:, m]
        if start[m]:
            g_init[c] += S[0, m]
        for j in range(m):
            if pred[m, j] and T > 1:
                g_trans[c, a[j]] += np.exp(gam[1:T, j] + trans[c, a[j]] - cum[1:T, c] + bh[1:T, m] - logz).sum()
        for k in range(1, kw + 1):
            g_len[k, c] += np.exp(h[:T + 1 - k, m] + len_scores[k, c] + cum[k:, c] + bg[k:, m] - logz).sum()
    return dict(logz=logz, ident=ident, h=h, gam=gam, bh=bh, bg=bg, S=S, E=E, p_used=E.sum(axis=0), p_used_S=S.sum(axis=0),
                p_end=p_end, occ=occ, elp=g_elp, trans=g_trans, init=g_init, len=g_len)


def twin_grads_graph(elp, graph, trans, init, len_scores, kp, endpen=None):
    """numpy in -> (log Z_g, dict(elp [T, C], trans [C, C], init [C], len [K, C], p_used [M])) from the C twin on the expanded
    lattice.  Finite tables only (the twin's "impossible" is -1e9)."""
    from oracle import factored as F
    elp = np.asarray(elp, np.float64)
    a, pred, start, end = _graph(graph)
    T, C = elp.shape
    M = len(a)
    e2, t2, i2, l2, ep = AG.expanded_lattice(elp, (np.asarray(a, np.int64), pred, start, end), trans, init, len_scores, kp, endpen)
    tm = max(T, kp)                                           # (the twin clips its length table to its Tmax)
    pad = np.zeros((1, tm, M))
    pad[0, :T] = e2
    z, g2 = F.logz(pad, np.array([T], np.int64), t2, i2, l2, ep[None], grad=True)
    K = np.asarray(len_scores).shape[0]
    g = dict(elp=np.zeros((T, C)), trans=np.zeros((C, C)), init=np.zeros(C), len=np.zeros((K, C)), p_used=np.zeros(M))
    for m in range(M):
        g['elp'][:, a[m]] += g2['elp'][0, :T, m]
        g['len'][:g2['len'].shape[0], a[m]] += g2['len'][:, m]
        for j in range(m):
            if pred[m, j]:
                g['trans'][a[m], a[j]] += g2['trans'][m, j]
                g['p_used'][m] += g2['trans'][m, j]
        if start[m]:
            g['init'][a[m]] += g2['init'][m]
            g['p_used'][m] += g2['init'][m]
    return float(z[0]), g


def brute_logz_graph(elp, graph, trans, init, len_scores, kp, endpen=None):
    """-> (log Z_g, frame occupancy [T, C], p_used [M], p_end [M]) by enumeration over paths x compositions; (-inf, zeros ...)
    without an alignment."""
    elp = np.asarray(elp, np.float64)
    T, C = elp.shape
    a, pred, start, end = _graph(graph)
    M = len(a)
    scores, occs, useds, ends = [], [], [], []
    for idx in AG.paths(pred, start, end):
        S = len(idx)
        if not 1 <= S <= T:
            continue
        for cuts in itertools.combinations(range(1, T), S - 1):
            b = (0,) + cuts + (T,)
            if any(b[i + 1] - b[i] > kp - 1 for i in range(S)):
                continue
            s = init[a[idx[0]]] + _closing(endpen, a[idx[-1]])
            occ, used, ended = np.zeros((T, C)), np.zeros(M), np.zeros(M)
            for i, m in enumerate(idx):
                s += elp[b[i]:b[i + 1], a[m]].sum() + len_scores[b[i + 1] - b[i], a[m]]
                occ[b[i]:b[i + 1], a[m]] = 1.0
                used[m] = 1.0
                if i > 0:
                    s += trans[a[m], a[idx[i - 1]]]
            ended[idx[-1]] = 1.0
            scores.append(s)
            occs.append(occ)
            useds.append(used)
            ends.append(ended)
    if not scores or not np.isfinite(np.max(scores)):
        return -np.inf, np.zeros((T, C)), np.zeros(M), np.zeros(M)
    scores = np.array(scores)
    mx = scores.max()
    w = np.exp(scores - mx)
    p = w / w.sum()
    return (float(mx + np.log(w.sum())), np.tensordot(p, np.array(occs), axes=1), np.tensordot(p, np.array(useds), axes=1),
            np.tensordot(p, np.array(ends), axes=1))


def is_ambiguous_brute(graph):
    a, pred, start, end = _graph(graph)
    seqs = [tuple(a[m] for m in idx) for idx in AG.paths(pred, start, end)]
    return len(set(seqs)) != len(seqs)


def random_graph(rng, M, C, p_edge=0.5):
    """A random DAG with at least one start and one end node (dead nodes and skipped path lengths allowed)."""
    a = rng.integers(0, C, M)
    pred = np.tril(rng.random((M, M)) < p_edge, k=-1)
    start = rng.random(M) < 0.4
    end = rng.random(M) < 0.4
    start[rng.integers(0, M)] = True
    end[rng.integers(0, M)] = True
    return a.astype(np.int64), pred, start, end
