"""Forced alignment to a transcript graph, restated directly from its definition (include/smmdp.h: smm_align_graph_f64) in
fp64 numpy -- the authority the tests compare against -- its twin, the C oracle's Viterbi on the lattice whose states are the
nodes, and a brute force over every start -> end path and every composition.

    pred(m)   = the nodes j < m that may directly precede node m
    h[0][m]   = init[a_m] if start(m), else -inf
    h[n][m]   = max_{j in pred(m)} ( gam[n][j] + trans[a_m][a_j] ) - cum[n][a_m]        0 < n < T   (-inf for an empty pred(m))
    gam[n][m] = cum[n][a_m] + max_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )        n = 1..T
    best      = max_{j : end(j)} ( gam[T][j] + closing_j )                              closing_j = endpen[a_j] or 0.0

Every + and - above is one numpy fp64 operation in that association; max is exact.  Nothing here is specific to any kernel:
every cell of every column is evaluated.  A graph is (a, pred, start, end): ids [M], bool [M, M] strictly lower triangular,
bool [M], bool [M]."""
import itertools

import numpy as np

from align_optional_ref import BIG_NEG, frame_labels, span_row, used_flags  # noqa: F401  (re-exported for the tests)


def from_optional(a, opt):
    """smm_align_opt_f64's pred / first / end as a graph."""
    import align_optional_ref as R
    pred_lo, first, end, _ = R.structure(opt)
    M = len(a)
    pred = np.zeros((M, M), bool)
    for m in range(M):
        pred[m, pred_lo[m]:m] = True
    return np.asarray(a, np.int64), pred, np.array(first, bool), np.array(end, bool)


def chain(a):
    M = len(a)
    return np.asarray(a, np.int64), np.eye(M, k=-1, dtype=bool), np.arange(M) == 0, np.arange(M) == M - 1


def path_lengths(pred, start, end):
    """(Lmin, Lmax): the fewest and the most nodes on any start -> end path, by a plain DP over the nodes; None without one."""
    M = len(start)
    lo, hi = [None] * M, [None] * M
    for m in range(M):
        cl = [lo[j] + 1 for j in range(m) if pred[m, j] and lo[j] is not None]
        ch = [hi[j] + 1 for j in range(m) if pred[m, j] and hi[j] is not None]
        if start[m]:
            cl.append(1)
            ch.append(1)
        if cl:
            lo[m], hi[m] = min(cl), max(ch)
    ends = [m for m in range(M) if end[m] and lo[m] is not None]
    if not ends:
        return None
    return min(lo[m] for m in ends), max(hi[m] for m in ends)


def structure_ok(a, pred, C):
    """Every id is a state of the video and every edge j -> m has j < m."""
    return all(0 <= int(x) < C for x in a) and not np.triu(np.asarray(pred)).any()


def feasible_by_count(T, pred, start, end, kp):
    """A start -> end path exists, the shortest fits into T frames, and the longest at the span limit reaches T."""
    L = path_lengths(pred, start, end)
    return L is not None and kp - 1 >= 1 and L[0] <= T and L[1] * (kp - 1) >= T


def columns(elp, a, pred, start, trans, init, len_scores, kp):
    """Every cell of the recursion -> (cum, h, gam), each [T + 1, .]."""
    T, M = elp.shape[0], len(a)
    cum = np.zeros((T + 1, elp.shape[1]))
    for n in range(1, T + 1):
        cum[n] = cum[n - 1] + elp[n - 1]
    h = np.full((T + 1, M), -np.inf)
    gam = np.full((T + 1, M), -np.inf)
    for m in range(M):
        c = a[m]
        if start[m]:
            h[0, m] = init[c]
        p = np.flatnonzero(pred[m, :m])
        if p.size and T > 1:
            h[1:T, m] = np.max(gam[1:T][:, p] + trans[c, a[p]][None, :], axis=1) - cum[1:T, c]
        acc = np.full(T + 1, -np.inf)
        for k in range(1, min(kp - 1, T) + 1):                # positions n = k .. T: source n - k
            np.maximum(acc[k:], h[:T + 1 - k, m] + len_scores[k, c], out=acc[k:])
        gam[1:, m] = cum[1:, c] + acc[1:]
    return cum, h, gam


def _bad(x):
    x = np.asarray(x, np.float64)
    return bool(np.any(np.isnan(x) | (x == np.inf)))


def tables_read_are_bad(a, pred, start, end, trans, init, len_scores, kp, endpen):
    """A NaN or +inf in a table entry the recursion reads (the error word's second condition): every node and every edge
    counts, on a start -> end path or not."""
    M = len(a)
    return (any(_bad(init[a[m]]) for m in range(M) if start[m])
            or any(_bad(trans[a[m], a[j]]) for m in range(M) for j in range(m) if pred[m, j])
            or any(_bad(len_scores[1:kp, a[m]]) for m in range(M))
            or (endpen is not None and any(_bad(endpen[a[j]]) for j in range(M) if end[j])))


def align_graph_ref(elp, graph, trans, init, len_scores, kp, endpen=None, count_rule=True, node_ties=None):
    """One video.  elp [T, C], graph = (a, pred, start, end) in local ids, trans [C, C] ([to][from]), init [C], len_scores
    [K, C] (row = length), kp: lengths 1 .. kp - 1 are usable, endpen [C] or None.  -> (best, segs): segs = [(start, node)] in
    time order; (-inf, None) without an alignment (by counting, an id outside [0, C), an edge j >= m, path lengths the graph
    skips, or -inf tables); (nan, None) when the error word's conditions hold.  ``count_rule=False``: the recursion decides
    alone whether there is an alignment.  ``node_ties``: a list that receives every position at which two different nodes attain
    the back-trace's maximum (two maximal alignments through different nodes)."""
    elp = np.asarray(elp, np.float64)
    T, C = elp.shape
    a, pred, start, end = graph
    a = np.asarray([int(x) for x in a], np.int64)
    pred, start, end = np.asarray(pred) != 0, np.asarray(start) != 0, np.asarray(end) != 0
    M = len(a)
    if not structure_ok(a, pred, C) or (count_rule and not feasible_by_count(T, pred, start, end, kp)):
        return -np.inf, None
    trans, init, len_scores = (np.asarray(x, np.float64) for x in (trans, init, len_scores))
    closing = np.zeros(C) if endpen is None else np.asarray(endpen, np.float64)
    with np.errstate(invalid='ignore'):
        cum, h, gam = columns(elp, a, pred, start, trans, init, len_scores, kp)
        if not np.isfinite(cum[T]).all() or tables_read_are_bad(a, pred, start, end, trans, init, len_scores, kp, endpen):
            return np.nan, None
        cand = np.flatnonzero(end)
        if cand.size == 0:
            return -np.inf, None
        w = closing[a[cand]]
        best = np.max(gam[T, cand] + w)
        if np.isnan(best):
            return np.nan, None
        if best == -np.inf:
            return best, None
        segs = []
        n = T
        while n > 0:
            kmax = min(kp - 1, n)
            k = np.arange(1, kmax + 1)[:, None]                                           # [k, j]: the smallest k, then j
            c = a[cand][None, :]
            val = (cum[n, c] + (h[n - k, cand[None, :]] + len_scores[k, c])) + w[None, :]
            hit = np.argwhere(val == np.max(val))
            assert hit.size, "no candidate attains the maximum"
            kk, j = int(k[hit[0][0], 0]), int(cand[hit[0][1]])
            if node_ties is not None and len(set(hit[:, 1].tolist())) > 1:
                node_ties.append(n)
            n -= kk
            segs.append((n, j))
            cand = np.flatnonzero(pred[j, :j])
            w = trans[a[j], a[cand]]
            assert n == 0 or cand.size, "the back-trace ran out of nodes"
        assert start[segs[-1][1]]
    return float(best), segs[::-1]


def expanded_lattice(elp, graph, trans, init, len_scores, kp, endpen=None):
    """The inputs of the twin: states = nodes (include/smmdp.h)."""
    a, pred, start, end = graph
    a = np.asarray(a, np.int64)
    M = len(a)
    e2 = np.ascontiguousarray(np.asarray(elp, np.float64)[:, a])
    l2 = np.ascontiguousarray(np.asarray(len_scores, np.float64)[:kp][:, a])
    t2 = np.full((M, M), BIG_NEG)
    i2 = np.full(M, BIG_NEG)
    ep = np.full(M, BIG_NEG)
    for m in range(M):
        for j in range(m):
            if pred[m, j]:
                t2[m, j] = trans[a[m], a[j]]
        if start[m]:
            i2[m] = init[a[m]]
        if end[m]:
            ep[m] = 0.0 if endpen is None else endpen[a[m]]
    return e2, t2, i2, l2, ep


def twin_align(elp, graph, trans, init, len_scores, kp, endpen=None):
    """oracle/smm_oracle.c's Viterbi on the expanded lattice -> (best, segs)."""
    from oracle import factored as F
    e2, t2, i2, l2, ep = expanded_lattice(elp, graph, trans, init, len_scores, kp, endpen)
    T, M = e2.shape
    tm = max(T, kp)                                           # (the twin clips its length table to its Tmax)
    pad = np.zeros((1, tm, M))
    pad[0, :T] = e2
    spans, v = F.viterbi(pad, np.array([T], np.int64), t2, i2, l2, ep[None])
    row = spans[0]
    pos = np.flatnonzero(row[:T] >= 0)
    assert row[T] == M and (np.diff(row[pos]) > 0).all(), "the twin left the graph"
    return float(v[0]), [(int(p), int(row[p])) for p in pos]


def paths(pred, start, end):
    """Every start -> end path as a tuple of nodes."""
    M = len(start)
    out = []

    def walk(path):
        m = path[-1]
        if end[m]:
            out.append(tuple(path))
        for nxt in range(m + 1, M):
            if pred[nxt, m]:
                walk(path + [nxt])

    for m in range(M):
        if start[m]:
            walk([m])
    return out


def brute_force(elp, graph, trans, init, len_scores, kp, endpen=None, all_maximal=False):
    """max over every start -> end path and every composition of T into its nodes, parts of 1 .. kp - 1, each score summed
    in real arithmetic (fp64, any order) -> (best, segs); ``all_maximal``: -> (best, every maximal segs)."""
    elp = np.asarray(elp, np.float64)
    a, pred, start, end = graph
    T = elp.shape[0]
    best, arg = -np.inf, []
    for idx in paths(pred, start, end):
        S = len(idx)
        if not 1 <= S <= T:
            continue
        for cuts in itertools.combinations(range(1, T), S - 1):
            b = (0,) + cuts + (T,)
            if any(b[i + 1] - b[i] > kp - 1 for i in range(S)):
                continue
            s = init[a[idx[0]]] + (0.0 if endpen is None else endpen[a[idx[-1]]])
            for i, m in enumerate(idx):
                s += elp[b[i]:b[i + 1], a[m]].sum() + len_scores[b[i + 1] - b[i], a[m]]
                if i > 0:
                    s += trans[a[m], a[idx[i - 1]]]
            if s > best:
                best, arg = s, [list(zip(b[:-1], idx))]
            elif s == best:
                arg.append(list(zip(b[:-1], idx)))
    if all_maximal:
        return best, arg
    return best, (arg[0] if arg else None)
