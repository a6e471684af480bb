"""fp64 numpy reference of the transcript-graph segment posteriors (smm_align_graph_segment_posteriors_f64), built on
tests/transcript_graph_ref.py: from (b), its forward-backward (S, E, h, bg), and from (d), the brute force over paths and
compositions, restated here with what it has to return per segment.

One video: elp [T, C], graph = (ids, pred, start, end) in local ids, trans [to][from], init [C], lens [K, C], kp (lengths
1 .. kp - 1 are usable), endpen [C] or None.  Positions: a segment of node m on the frames [s, e) starts at s and ends at e."""
import itertools

import numpy as np

import align_graph_ref as AG
import transcript_graph_ref as TG

NEG_INF = float('-inf')


def _lse_rows(a):
    """Row-wise LSE of a 2-d array; -inf for a row without a finite entry."""
    m = a.max(axis=1)
    safe = np.where(np.isfinite(m), m, 0.0)
    with np.errstate(divide='ignore'):
        return np.where(m == NEG_INF, NEG_INF, safe + np.log(np.exp(a - safe[:, None]).sum(axis=1)))


def fast_forward_backward(elp, graph, trans, init, lens, kp, endpen=None):
    """TG.forward_backward's h, gam, bh, bg, S, E, p_used and logz with the loops over positions and lengths as array
    operations (the same recursions; for the sizes the every-cell loops are too slow for).  Finite tables assumed."""
    elp = np.asarray(elp, np.float64)
    trans, init, lens = (np.asarray(x, np.float64) for x in (trans, init, lens))
    T, C = elp.shape
    a, pred, start, end = TG._graph(graph)
    M = len(a)
    if not TG.has_alignment_by_count(T, C, graph, kp):
        return dict(logz=-np.inf)
    win = np.lib.stride_tricks.sliding_window_view
    kw = min(kp - 1, T)
    cum = np.concatenate([np.zeros((1, C)), np.cumsum(elp, axis=0)])
    h = np.full((T + 1, M), NEG_INF)
    gam = np.full((T + 1, M), NEG_INF)
    pad = np.full(kw, NEG_INF)
    for m in range(M):
        c = a[m]
        p = [j for j in range(m) if pred[m, j]]
        if start[m]:
            h[0, m] = init[c]
        if p and T > 1:
            h[1:T, m] = _lse_rows(np.stack([gam[1:T, j] + trans[c, a[j]] for j in p], axis=1)) - cum[1:T, c]
        w = win(np.concatenate([pad, h[:, m]]), kw)[:T + 1]           # row n: h[n - kw .. n - 1]
        gam[:, m] = cum[:, c] + _lse_rows(w + lens[1:kw + 1, c][::-1][None])
        gam[0, m] = NEG_INF
    logz = float(_lse_rows(np.array([[gam[T, j] + TG._closing(endpen, a[j]) for j in range(M) if end[j]]]))[0])
    if not np.isfinite(logz):
        return dict(logz=logz)
    succ = [[q for q in range(j + 1, M) if pred[q, j]] for j in range(M)]
    bg = np.full((T + 1, M), NEG_INF)
    bh = np.full((T + 1, M), NEG_INF)
    for j in range(M):
        if end[j]:
            bg[T, j] = TG._closing(endpen, a[j])
    for m in range(M - 1, -1, -1):
        c = a[m]
        if succ[m] and T > 1:
            bg[1:T, m] = _lse_rows(np.stack([trans[a[q], c] - cum[1:T, a[q]] + bh[1:T, q] for q in succ[m]], axis=1))
        x = np.concatenate([cum[:, c] + bg[:, m], pad])
        bh[:T, m] = _lse_rows(win(x[1:], kw)[:T] + lens[1:kw + 1, c][None])   # row s: x[s + 1 .. s + kw]
    with np.errstate(invalid='ignore'):
        S = np.where((h == NEG_INF) | (bh == NEG_INF), 0.0, np.exp(h + bh - logz))
        E = np.where((gam == NEG_INF) | (bg == NEG_INF), 0.0, np.exp(gam + bg - logz))
    return dict(logz=logz, h=h, gam=gam, bh=bh, bg=bg, S=S, E=E, p_used=E.sum(axis=0))


def from_forward_backward(elp, graph, trans, init, lens, kp, endpen=None, fast=False):
    """(b) -> dict(logz, E, S [T + 1, M], p_used [M], seg(m, s, e) -> log posterior of node m on [s, e)); logz -inf: only logz.
    ``fast``: the recursions as array operations (``fast_forward_backward``)."""
    fb = (fast_forward_backward if fast else TG.forward_backward)(elp, graph, trans, init, lens, kp, endpen)
    if not np.isfinite(fb['logz']):
        return dict(logz=fb['logz'])
    elp = np.asarray(elp, np.float64)
    lens = np.asarray(lens, np.float64)
    T, C = elp.shape
    a = [int(v) for v in graph[0]]
    cum = np.concatenate([np.zeros((1, C)), np.cumsum(elp, axis=0)])
    kw = min(kp - 1, T)

    def seg(m, s, e):
        k = e - s
        if k < 1 or k > kw or e > T or s < 0:
            return NEG_INF
        c = a[m]
        lp = fb['h'][s, m] + lens[k, c] + (cum[e, c] + fb['bg'][e, m])
        return NEG_INF if lp == NEG_INF else float(lp - fb['logz'])

    return dict(logz=fb['logz'], E=fb['E'], S=fb['S'], p_used=fb['p_used'], seg=seg)


def brute_force(elp, graph, trans, init, lens, kp, endpen=None):
    """(d) -> dict(logz, E, S [T + 1, M], p_used [M], segs {(m, s, e): probability}); logz -inf: only logz."""
    elp = np.asarray(elp, np.float64)
    trans, init, lens = (np.asarray(x, np.float64) for x in (trans, init, lens))
    T, C = elp.shape
    a, pred, start, end = TG._graph(graph)
    M = len(a)
    scores, aligns = [], []
    for idx in AG.paths(pred, start, end):
        n = len(idx)
        if not 1 <= n <= T:
            continue
        for cuts in itertools.combinations(range(1, T), n - 1):
            b = (0,) + cuts + (T,)
            if any(b[i + 1] - b[i] > kp - 1 for i in range(n)):
                continue
            s = init[a[idx[0]]] + TG._closing(endpen, a[idx[-1]])
            for i, m in enumerate(idx):
                s += elp[b[i]:b[i + 1], a[m]].sum() + lens[b[i + 1] - b[i], a[m]]
                if i > 0:
                    s += trans[a[m], a[idx[i - 1]]]
            scores.append(s)
            aligns.append([(m, b[i], b[i + 1]) for i, m in enumerate(idx)])
    if not scores or not np.isfinite(np.max(scores)):
        return dict(logz=-np.inf)
    scores = np.array(scores)
    mx = scores.max()
    w = np.exp(scores - mx)
    p = w / w.sum()
    E, S, segs = np.zeros((T + 1, M)), np.zeros((T + 1, M)), {}
    for pi, al in zip(p, aligns):
        for (m, s, e) in al:
            S[s, m] += pi
            E[e, m] += pi
            segs[(m, s, e)] = segs.get((m, s, e), 0.0) + pi
    return dict(logz=float(mx + np.log(w.sum())), E=E, S=S, p_used=E.sum(axis=0), segs=segs)


def moments(col):
    """Mean and standard deviation of the position n under the weights col[n] (the variance about the mean); NaN for no mass."""
    col = np.asarray(col, np.float64)
    mass = col.sum()
    if not mass > 0:
        return float('nan'), float('nan')
    n = np.arange(col.shape[0], dtype=np.float64)
    mean = float((col * n).sum() / mass)
    return mean, float(np.sqrt((col * (n - mean) ** 2).sum() / mass))


def alignment_logp(ref, spans_row, used, ids, T, kp, class_of=None):
    """What seg_logp and node_logp hold for one alignment: ``spans_row`` [>= T + 1] in the ids ``class_of`` maps to local ones
    (default: local already), ``used`` [M] -> (seg [len(spans_row)], node [M]); everything -inf for an alignment the graph does
    not admit by the header's three faults."""
    row = np.asarray(spans_row)
    M = len(ids)
    seg, node = np.full(row.shape[0], NEG_INF), np.full(M, NEG_INF)
    starts = [q for q in range(T) if row[q] != -1]
    nodes = [m for m in range(M) if used[m]]
    if len(starts) != len(nodes):
        return seg, node
    ends = starts[1:] + [T]
    loc = (lambda v: int(v)) if class_of is None else class_of
    if any(e - s > kp - 1 or loc(row[s]) != int(ids[m]) for s, e, m in zip(starts, ends, nodes)):
        return seg, node
    for s, e, m in zip(starts, ends, nodes):
        if 'seg' in ref:
            v = ref['seg'](m, s, e)
        else:
            pr = ref['segs'].get((m, s, e), 0.0)
            v = np.log(pr) if pr > 0 else NEG_INF
        seg[s] = node[m] = v
    seg[T] = 0.0
    return seg, node
