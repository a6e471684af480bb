"""fp64 numpy reference of the segment and boundary posteriors (smm_segment_posteriors_f64), two independent statements.

(a) ``recursions``: the forward and backward recursions of include/smmdp.h's definitions on the factored tables of ONE video
    (oracle/smm_oracle.c states the same lattice in C): start / end / boundary posteriors, the marginal of any one span, and the
    identities' other sides (g_len, the frame occupancies).
(b) ``enumerate_posteriors``: every segmentation of the video with its probability, summed into the same quantities.

Conventions (both): elp [frames][C], trans [to][from], init [C], lens [kp][C] (row k = a span of k frames, k = 1 .. kp - 1),
endpen [C] or None.  T = the DP positions: ``frames`` with EOS, ``frames - 1`` without, where the closing label of frame T counts
as a one-frame span of its class.  The outputs cover the video's frames: [frames][C] and [frames]."""
import numpy as np

NEG_INF = float('-inf')
BIG_NEG = -1e9


def _lse(v):
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.size == 0:
        return NEG_INF
    m = v.max()
    if m == NEG_INF:
        return NEG_INF
    return float(m + np.log(np.exp(v - m).sum()))


def _lse0(a):
    """Column-wise LSE of a [n][C] array -> [C]; -inf for a column without a finite entry (or n = 0)."""
    a = np.asarray(a, dtype=np.float64)
    if a.shape[0] == 0:
        return np.full(a.shape[1], NEG_INF)
    m = a.max(axis=0)
    safe = np.where(m == NEG_INF, 0.0, m)
    with np.errstate(divide='ignore'):
        return np.where(m == NEG_INF, NEG_INF, safe + np.log(np.exp(a - safe).sum(axis=0)))


def _exp(lp):
    return 0.0 if lp == NEG_INF else float(np.exp(lp))


def _closing(trans, endpen, c):
    """EOS: the closing log-weight of a last span of class j: LSE(endpen[j], LSE_to(trans[to][j]) - 1e9)."""
    return np.array([_lse([0.0 if endpen is None else endpen[j], _lse(trans[:, j]) + BIG_NEG]) for j in range(c)])


class Recursions:
    """(a).  Attributes: logz, start_post / end_post [frames][C], bnd_post [frames], g_len [kp][C], occupancy [frames][C];
    ``span_logp(c, s, e)``: log P(a span of c covers exactly the frames [s, e)); ``closing_logp(to)`` without EOS."""

    def __init__(self, elp, trans, init, lens, endpen=None, no_eos=False):
        elp, trans, init, lens = (np.asarray(a, dtype=np.float64) for a in (elp, trans, init, lens))
        frames, c = elp.shape
        t = frames - (1 if no_eos else 0)
        kp = lens.shape[0]                      # (the caller clips the table to the video's span limit)
        self.t, self.c, self.kp, self.no_eos, self.lens = t, c, kp, no_eos, lens
        cum = np.zeros((t + 1, c))
        cum[1:] = np.cumsum(elp[:t], axis=0)
        start = np.full((t + 1, c), NEG_INF)
        gam = np.full((t + 1, c), NEG_INF)
        start[0] = init
        for n in range(1, t + 1):
            km = min(kp - 1, n)                 # rows n - 1 .. n - km stand for k = 1 .. km
            gam[n] = _lse0(start[n - km:n][::-1] + lens[1:km + 1] + (cum[n] - cum[n - km:n][::-1]))
            if n < t:
                for to in range(c):
                    start[n, to] = _lse(gam[n] + trans[to])
        if no_eos:
            fin = np.array([_lse(gam[t] + trans[to]) + elp[t, to] for to in range(c)])
            wend = np.array([_lse(trans[:, j] + elp[t]) for j in range(c)])
            z = _lse(fin)
        else:
            wend = _closing(trans, endpen, c)
            fin = None
            z = _lse(gam[t] + wend)
        bend = np.full((t + 1, c), NEG_INF)
        bstart = np.full((t + 1, c), NEG_INF)
        bend[t] = wend
        for s in range(t - 1, -1, -1):
            km = min(kp - 1, t - s)
            bstart[s] = _lse0(lens[1:km + 1] + (cum[s + 1:s + km + 1] - cum[s]) + bend[s + 1:s + km + 1])
            if s > 0:
                for j in range(c):
                    bend[s, j] = _lse(trans[:, j] + bstart[s])
        self.logz, self.cum, self.start, self.gam, self.bend, self.bstart, self.fin = z, cum, start, gam, bend, bstart, fin
        self.start_post = np.zeros((frames, c))
        self.end_post = np.zeros((frames, c))
        if z == NEG_INF:                        # no segmentation has finite weight: nothing below is defined
            self.start_post[:], self.end_post[:] = np.nan, np.nan
            self.bnd_post = np.full(frames, np.nan)
            return
        self.start_post[:t] = np.exp(start[:t] + bstart[:t] - z)
        self.end_post[:t] = np.exp(gam[1:] + bend[1:] - z)
        if no_eos:
            for to in range(c):
                self.start_post[t, to] = self.end_post[t, to] = _exp(fin[to] - z)
        self.bnd_post = self.start_post.sum(axis=1)
        self.g_len = np.zeros((kp, c))
        occ = np.zeros((frames + 1, c))
        for s in range(t):
            km = min(kp - 1, t - s)
            p = np.exp(start[s] + lens[1:km + 1] + (cum[s + 1:s + km + 1] - cum[s]) + bend[s + 1:s + km + 1] - z)
            self.g_len[1:km + 1] += p
            occ[s] += p.sum(axis=0)
            occ[s + 1:s + km + 1] -= p
        self.occupancy = np.cumsum(occ, axis=0)[:frames]
        if no_eos:
            self.occupancy[t] = self.start_post[t]

    def span_logp(self, c, s, e):
        k = e - s
        if k < 1 or k > self.kp - 1 or e > self.t or not 0 <= c < self.c:
            return NEG_INF
        lp = self.start[s, c] + self.lens[k, c] + (self.cum[e, c] - self.cum[s, c]) + self.bend[e, c]
        return NEG_INF if lp == NEG_INF else lp - self.logz

    def closing_logp(self, to):
        return NEG_INF if self.fin[to] == NEG_INF else self.fin[to] - self.logz


def enumerate_segmentations(elp, trans, init, lens, endpen=None, no_eos=False):
    """(b).  -> [(segments, closing label or None, score)]: ``segments`` a tuple of (class, start, end) that tiles the frames
    [0, T), the score summed term by term from the tables; with EOS the closing weight of ``_closing``."""
    elp, trans, init, lens = (np.asarray(a, dtype=np.float64) for a in (elp, trans, init, lens))
    frames, c = elp.shape
    t = frames - (1 if no_eos else 0)
    kp = lens.shape[0]                      # (the caller clips the table to the video's span limit)
    wend = None if no_eos else _closing(trans, endpen, c)
    out = []

    def rec(n, prev, acc, segs):
        if n == t:
            if no_eos:
                for to in range(c):
                    out.append((tuple(segs), to, acc + trans[to, prev] + elp[t, to]))
            else:
                out.append((tuple(segs), None, acc + wend[prev]))
            return
        for k in range(1, kp):
            if n + k > t:
                break
            for j in range(c):
                w = (init[j] if n == 0 else trans[j, prev]) + lens[k, j] + elp[n:n + k, j].sum()
                rec(n + k, j, acc + w, segs + [(j, n, n + k)])

    rec(0, -1, 0.0, [])
    return out


def enumerate_posteriors(elp, trans, init, lens, endpen=None, no_eos=False):
    """(b) summed: dict(logz, start_post, end_post, bnd_post, spans {(class, start, end): probability}, closing [C] without
    EOS, paths [(segments, closing, probability)])."""
    elp = np.asarray(elp, dtype=np.float64)
    frames, c = elp.shape
    t = frames - (1 if no_eos else 0)
    paths = enumerate_segmentations(elp, trans, init, lens, endpen, no_eos)
    z = _lse([p[2] for p in paths])
    start = np.zeros((frames, c))
    end = np.zeros((frames, c))
    spans = {}
    closing = np.zeros(c)
    listed = []
    for segs, to, score in paths:
        p = _exp(score - z) if z > NEG_INF else float('nan')
        listed.append((segs, to, p))
        for (j, s, e) in segs:
            start[s, j] += p
            end[e - 1, j] += p
            spans[(j, s, e)] = spans.get((j, s, e), 0.0) + p
        if to is not None:
            closing[to] += p
    if no_eos:
        start[t] = end[t] = closing
    return dict(logz=z, start_post=start, end_post=end, bnd_post=start.sum(axis=1), spans=spans, closing=closing, paths=listed)


def spans_logp(ref, row, frames, no_eos, n_cols):
    """What seg_logp holds for one row of a span encoding in LOCAL ids (EOS id = C): from (a) (``ref`` a Recursions) or from (b)
    (``ref`` the dict of enumerate_posteriors).  -> fp64 [n_cols]."""
    t = frames - (1 if no_eos else 0)
    out = np.full(n_cols, NEG_INF)
    starts = [q for q in range(t) if row[q] != -1]
    for i, s in enumerate(starts):
        e = starts[i + 1] if i + 1 < len(starts) else t
        c = int(row[s])
        if isinstance(ref, Recursions):
            out[s] = ref.span_logp(c, s, e)
        else:
            p = ref['spans'].get((c, s, e), 0.0)
            out[s] = np.log(p) if p > 0 else NEG_INF
    if no_eos:
        to = int(row[t])
        if isinstance(ref, Recursions):
            out[t] = ref.closing_logp(to) if 0 <= to < ref.c else NEG_INF
        else:
            p = ref['closing'][to] if 0 <= to < len(ref['closing']) else 0.0
            out[t] = np.log(p) if p > 0 else NEG_INF
    else:
        out[t] = 0.0
    return out
