"""Forced alignment, restated directly from its definition (include/smmdp.h: smm_align_f64) in fp64 numpy -- the authority the
alignment tests compare against -- and its twin: the C oracle's Viterbi on the lattice whose states are the transcript positions.

    cum[0][c] = 0;  cum[n][c] = cum[n-1][c] + elp[n-1][c]
    h[0][0] = init[a_0];  h[0][m>0] = -inf
    gam[n][m] = cum[n][a_m] + max_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )
    h[n][m]   = ( gam[n][m-1] + trans[a_m][a_{m-1}] ) - cum[n][a_m]          0 < n < T, m >= 1;  h[n>0][0] = -inf
    best      = gam[T][M-1] + closing                                        closing = endpen[a_{M-1}] or 0.0

Every + above is one numpy fp64 add in that association; max is exact, so the order in which it is taken is free (it is taken
over k, one vector of positions at a time).  Nothing here is specific to any kernel: every cell of every column is evaluated."""
import itertools

import numpy as np

BIG_NEG = -1e9


def feasible_by_count(T, M, kp):
    return 1 <= M <= T and M * (kp - 1) >= T


def _columns(elp, a, trans, init, len_scores, kp):
    T, M = elp.shape[0], len(a)
    cum = np.zeros((T + 1, elp.shape[1]))
    for n in range(1, T + 1):
        cum[n] = cum[n - 1] + elp[n - 1]
    h = np.full((T + 1, M), -np.inf)
    gam = np.full((T + 1, M), -np.inf)
    h[0, 0] = init[a[0]]
    for m in range(M):
        c = a[m]
        acc = np.full(T + 1, -np.inf)
        for k in range(1, min(kp - 1, T) + 1):                # positions n = k .. T: source n - k
            np.maximum(acc[k:], h[:T + 1 - k, m] + len_scores[k, c], out=acc[k:])
        gam[1:, m] = cum[1:, c] + acc[1:]
        if m + 1 < M:
            cn = a[m + 1]
            h[1:T, m + 1] = (gam[1:T, m] + trans[cn, c]) - cum[1:T, cn]
    return cum, h, gam


def align_ref(elp, a, trans, init, len_scores, kp, closing=0.0):
    """One video.  elp [T, C], a: local ids, trans [C, C] ([to][from]), init [C], len_scores [K, C] (row = length), kp: lengths
    1 .. kp - 1 are usable, closing: the closing term.  -> (best, starts): starts[m] = first frame of segment m; (-inf, None)
    without an alignment (by counting, an id outside [0, C), or -inf tables); (nan, None) when a NaN reached the DP."""
    elp = np.asarray(elp, np.float64)
    T, C = elp.shape
    a = [int(x) for x in a]
    M = len(a)
    if not feasible_by_count(T, M, kp) or any(x < 0 or x >= C for x in a):
        return -np.inf, None
    with np.errstate(invalid='ignore'):
        cum, h, gam = _columns(elp, a, np.asarray(trans, np.float64), np.asarray(init, np.float64),
                               np.asarray(len_scores, np.float64), kp)
        best = gam[T, M - 1] + closing
        if np.isnan(best) or not np.isfinite(cum[T]).all():
            return np.nan, None
        if best == -np.inf:
            return best, None
        starts = [0] * M
        n, w = T, closing
        for m in range(M - 1, -1, -1):
            c = a[m]
            kmax = min(kp - 1, n)
            k = np.arange(1, kmax + 1)
            val = (cum[n, c] + (h[n - k, m] + len_scores[k, c])) + w
            hit = np.flatnonzero(val == np.max(val))
            if hit.size == 0:
                return np.nan, None
            n -= int(k[hit[0]])
            starts[m] = n
            if m > 0:
                w = trans[c, a[m - 1]]
    assert n == 0
    return float(best), starts


def span_row(starts, a, T, t_max, gid=None, eos=None):
    """The span encoding of an alignment: the (global) class at every segment start, the EOS id at T, -1 elsewhere."""
    row = np.full(t_max + 1, -1, np.int64)
    if starts is None:
        return row
    for s, c in zip(starts, a):
        row[s] = c if gid is None else gid(int(c))
    row[T] = eos
    return row


def frame_labels(starts, a, T, gid=None):
    lab = np.full(T, -1, np.int64)
    if starts is None:
        return lab
    ends = list(starts[1:]) + [T]
    for s, e, c in zip(starts, ends, a):
        lab[s:e] = c if gid is None else gid(int(c))
    return lab


def expanded_lattice(elp, a, trans, init, len_scores, kp, closing=0.0):
    """The inputs of the twin: states = transcript positions (include/smmdp.h)."""
    a = np.asarray(a, np.int64)
    M = len(a)
    e2 = np.ascontiguousarray(np.asarray(elp, np.float64)[:, a])
    l2 = np.ascontiguousarray(np.asarray(len_scores, np.float64)[:kp][:, a])
    t2 = np.full((M, M), BIG_NEG)
    for m in range(1, M):
        t2[m, m - 1] = trans[a[m], a[m - 1]]
    i2 = np.full(M, BIG_NEG)
    i2[0] = init[a[0]]
    ep = np.full(M, BIG_NEG)
    ep[M - 1] = closing
    return e2, t2, i2, l2, ep


def twin_align(elp, a, trans, init, len_scores, kp, closing=0.0):
    """oracle/smm_oracle.c's Viterbi on the expanded lattice -> (best, starts)."""
    from oracle import factored as F
    e2, t2, i2, l2, ep = expanded_lattice(elp, a, trans, init, len_scores, kp, closing)
    T, M = e2.shape
    tm = max(T, kp)                                           # (the twin clips its length table to its Tmax)
    pad = np.zeros((1, tm, M))
    pad[0, :T] = e2
    spans, v = F.viterbi(pad, np.array([T], np.int64), t2, i2, l2, ep[None])
    row = spans[0]
    pos = np.flatnonzero(row[:T] >= 0)
    assert row[T] == M and np.array_equal(row[pos], np.arange(M)), "the twin left the transcript"
    return float(v[0]), [int(p) for p in pos]


def brute_force(elp, a, trans, init, len_scores, kp, closing=0.0):
    """max over every composition of T into len(a) parts of 1 .. kp - 1, each score summed in real arithmetic (fp64, any
    order): the VALUE of the best alignment up to rounding, and the set of compositions within `tol` of it."""
    elp = np.asarray(elp, np.float64)
    T, M = elp.shape[0], len(a)
    best, arg = -np.inf, None
    for cuts in itertools.combinations(range(1, T), M - 1):
        b = (0,) + cuts + (T,)
        if any(b[m + 1] - b[m] > kp - 1 for m in range(M)):
            continue
        s = init[a[0]] + closing
        for m in range(M):
            s += elp[b[m]:b[m + 1], a[m]].sum() + len_scores[b[m + 1] - b[m], a[m]]
            if m > 0:
                s += trans[a[m], a[m - 1]]
        if s > best:
            best, arg = s, list(b[:-1])
    return best, arg
