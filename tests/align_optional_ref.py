"""Forced alignment with optional transcript entries, restated directly from its definition (include/smmdp.h:
smm_align_opt_f64) in fp64 numpy -- the authority the tests compare against -- its twin, the C oracle's Viterbi on the lattice
whose states are the transcript positions, and a brute force over every subset of the optional entries and every composition.

    pred(m)   = m-1, m-2, ... down to and including the nearest mandatory entry (to 0 when there is none)
    first(m)  = every entry before m is optional;  end(j) = every entry after j is optional
    h[0][m]   = init[a_m] if first(m), else -inf
    h[n][m]   = max_{j in pred(m)} ( gam[n][j] + trans[a_m][a_j] ) - cum[n][a_m]        0 < n < T
    gam[n][m] = cum[n][a_m] + max_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )        n = 1..T
    best      = max_{j : end(j)} ( gam[T][j] + closing_j )                              closing_j = endpen[a_j] or 0.0

Every + and - above is one numpy fp64 operation in that association; max is exact.  Nothing here is specific to any kernel:
every cell of every column is evaluated."""
import itertools

import numpy as np

BIG_NEG = -1e9


def structure(opt):
    """-> (pred_lo, first, end, mand): pred(m) = range(pred_lo[m], m); first[m], end[m] as above; the mandatory count."""
    opt = [bool(x) for x in opt]
    M = len(opt)
    pred_lo, head = [], 0
    for m in range(M):
        pred_lo.append(head)
        if not opt[m]:
            head = m
    first = [all(opt[:m]) for m in range(M)]
    end = [all(opt[m + 1:]) for m in range(M)]
    return pred_lo, first, end, M - sum(opt)


def feasible_by_count(T, opt, kp):
    """The mandatory entries need a frame each, and all M entries at their longest must reach T."""
    M = len(opt)
    return M >= 1 and kp - 1 >= 1 and M - sum(bool(x) for x in opt) <= T and M * (kp - 1) >= T


def columns(elp, a, opt, trans, init, len_scores, kp):
    """Every cell of the recursion -> (cum, h, gam), each [T + 1, .]."""
    T, M = elp.shape[0], len(a)
    pred_lo, first, _, _ = structure(opt)
    cum = np.zeros((T + 1, elp.shape[1]))
    for n in range(1, T + 1):
        cum[n] = cum[n - 1] + elp[n - 1]
    h = np.full((T + 1, M), -np.inf)
    gam = np.full((T + 1, M), -np.inf)
    for m in range(M):
        c = a[m]
        if first[m]:
            h[0, m] = init[c]
        if m > 0 and T > 1:
            p = np.arange(pred_lo[m], m)
            h[1:T, m] = np.max(gam[1:T][:, p] + trans[c, a[p]][None, :], axis=1) - cum[1:T, c]
        acc = np.full(T + 1, -np.inf)
        for k in range(1, min(kp - 1, T) + 1):                # positions n = k .. T: source n - k
            np.maximum(acc[k:], h[:T + 1 - k, m] + len_scores[k, c], out=acc[k:])
        gam[1:, m] = cum[1:, c] + acc[1:]
    return cum, h, gam


def _bad(x):
    x = np.asarray(x, np.float64)
    return bool(np.any(np.isnan(x) | (x == np.inf)))


def tables_read_are_bad(a, opt, trans, init, len_scores, kp, endpen):
    """A NaN or +inf in a table entry the recursion reads (the error word's second condition)."""
    pred_lo, first, end, _ = structure(opt)
    M = len(a)
    return (any(_bad(init[a[m]]) for m in range(M) if first[m])
            or any(_bad(trans[a[m], a[j]]) for m in range(M) for j in range(pred_lo[m], m))
            or any(_bad(len_scores[1:kp, a[m]]) for m in range(M))
            or (endpen is not None and any(_bad(endpen[a[j]]) for j in range(M) if end[j])))


def align_optional_ref(elp, a, opt, trans, init, len_scores, kp, endpen=None, count_rule=True):
    """One video.  elp [T, C], a: local ids, opt: one flag per entry, trans [C, C] ([to][from]), init [C], len_scores [K, C]
    (row = length), kp: lengths 1 .. kp - 1 are usable, endpen [C] or None.  -> (best, segs): segs = [(start, entry)] in
    time order; (-inf, None) without an alignment (by counting, an id outside [0, C), or -inf tables); (nan, None) when the
    error word's conditions hold.  ``count_rule=False``: the recursion decides alone whether there is an alignment."""
    elp = np.asarray(elp, np.float64)
    T, C = elp.shape
    a = np.asarray([int(x) for x in a], np.int64)
    M = len(a)
    if (count_rule and not feasible_by_count(T, opt, kp)) or any(x < 0 or x >= C for x in a):
        return -np.inf, None
    trans, init, len_scores = (np.asarray(x, np.float64) for x in (trans, init, len_scores))
    closing = np.zeros(C) if endpen is None else np.asarray(endpen, np.float64)
    pred_lo, first, end, _ = structure(opt)
    with np.errstate(invalid='ignore'):
        cum, h, gam = columns(elp, a, opt, trans, init, len_scores, kp)
        if not np.isfinite(cum[T]).all() or tables_read_are_bad(a, opt, trans, init, len_scores, kp, endpen):
            return np.nan, None
        cand = np.array([j for j in range(M) if end[j]])
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
            n -= kk
            segs.append((n, j))
            cand = np.arange(pred_lo[j], j)
            w = trans[a[j], a[cand]]
            assert n == 0 or cand.size, "the back-trace ran out of entries"
        assert first[segs[-1][1]]
    return float(best), segs[::-1]


def used_flags(segs, M):
    u = np.zeros(M, np.int32)
    if segs is not None:
        u[[j for _, j in segs]] = 1
    return u


def span_row(segs, a, T, t_max, gid=None, eos=None):
    """The span encoding of an alignment: the (global) class at every segment start, the EOS id at T, -1 elsewhere."""
    row = np.full(t_max + 1, -1, np.int64)
    if segs is None:
        return row
    for s, j in segs:
        row[s] = a[j] if gid is None else gid(int(a[j]))
    row[T] = eos
    return row


def frame_labels(segs, a, T, gid=None):
    lab = np.full(T, -1, np.int64)
    if segs is None:
        return lab
    ends = [s for s, _ in segs[1:]] + [T]
    for (s, j), e in zip(segs, ends):
        lab[s:e] = a[j] if gid is None else gid(int(a[j]))
    return lab


def expanded_lattice(elp, a, opt, trans, init, len_scores, kp, endpen=None):
    """The inputs of the twin: states = transcript positions (include/smmdp.h)."""
    a = np.asarray(a, np.int64)
    M = len(a)
    pred_lo, first, end, _ = structure(opt)
    e2 = np.ascontiguousarray(np.asarray(elp, np.float64)[:, a])
    l2 = np.ascontiguousarray(np.asarray(len_scores, np.float64)[:kp][:, a])
    t2 = np.full((M, M), BIG_NEG)
    i2 = np.full(M, BIG_NEG)
    ep = np.full(M, BIG_NEG)
    for m in range(M):
        for j in range(pred_lo[m], m):
            t2[m, j] = trans[a[m], a[j]]
        if first[m]:
            i2[m] = init[a[m]]
        if end[m]:
            ep[m] = 0.0 if endpen is None else endpen[a[m]]
    return e2, t2, i2, l2, ep


def twin_align(elp, a, opt, trans, init, len_scores, kp, endpen=None):
    """oracle/smm_oracle.c's Viterbi on the expanded lattice -> (best, segs)."""
    from oracle import factored as F
    e2, t2, i2, l2, ep = expanded_lattice(elp, a, opt, trans, init, len_scores, kp, endpen)
    T, M = e2.shape
    tm = max(T, kp)                                           # (the twin clips its length table to its Tmax)
    pad = np.zeros((1, tm, M))
    pad[0, :T] = e2
    spans, v = F.viterbi(pad, np.array([T], np.int64), t2, i2, l2, ep[None])
    row = spans[0]
    pos = np.flatnonzero(row[:T] >= 0)
    assert row[T] == M and (np.diff(row[pos]) > 0).all(), "the twin left the transcript"
    return float(v[0]), [(int(p), int(row[p])) for p in pos]


def brute_force(elp, a, opt, trans, init, len_scores, kp, endpen=None):
    """max over every subset of the optional entries left out and every composition of T into the kept entries, parts of
    1 .. kp - 1, each score summed in real arithmetic (fp64, any order) -> (best, segs)."""
    elp = np.asarray(elp, np.float64)
    T, M = elp.shape[0], len(a)
    best, arg = -np.inf, None
    for keep in itertools.product(*[(False, True) if opt[m] else (True,) for m in range(M)]):
        idx = [m for m in range(M) if keep[m]]
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
                best, arg = s, list(zip(b[:-1], idx))
    return best, arg
