"""Lattices built against the time-split decode's certificate (csrc/smm_chunk.hip), and a plain fp64 model of the
max-plus recursion that the host test and the GPU tests use to check that a lattice does what it was built for.

The MIRROR lattice: 2c states in two groups, A = 0..c-1 and B = c..2c-1, with the same emissions, the same init and the same
transitions inside each group (-50 between the groups: no path changes group).  A's length table is B's plus a constant phi_q
per class, so in the one-piece decode h_A - h_B = D(n) = the sum of phi over the segments of the path that end by n.  A unit
that starts from h = 0 at a_j sees D(n) - D(a_j) instead: the cut j lets the spread D(a_j) - D(a_{j-1}) through.  One segment of
the DRIFT class (phi < 0) ends between a_{j-1} and a_j for every cut, each within half the certificate's tolerance, and the
video's last segment is of the FINAL class (phi > 0), chosen so that D(T) = -delta: the one-piece decode ends in group B while
the last unit sees group A ahead by -D(a_J) - delta.  With drifting=1 the roles of the groups are swapped (B's table carries
phi): the spread at every cut then has the other sign relative to the cut's reference state, which is a group-A state."""
import numpy as np

DRIFT, FINAL = 0, 1


def unit_layout(lengths, c, k, unit=1):
    """The planner's units of a single-group batch as run_gpu launches it, with SMM_CHUNK=1 and SMM_CHUNK_P=unit:
    per video, a list of (first position a_j, positions T_j, positions in front of the own part)."""
    import os
    from action_segmentation_amd import ops, _lib, _build
    _build.build()                                             # (the planner is host code of libsmmdp.so: built if missing or stale)
    saved = {n: os.environ.get(n) for n in ('SMM_CHUNK', 'SMM_CHUNK_P', 'SMM_CHUNK_WC', 'SMM_CHUNK_LMIN')}
    try:
        os.environ['SMM_CHUNK'] = '1'
        os.environ['SMM_CHUNK_P'] = str(unit)
        for n in ('SMM_CHUNK_WC', 'SMM_CHUNK_LMIN'):
            os.environ.pop(n, None)
        _lib.reload_env()
        lengths = np.asarray(lengths)
        b = ops.Batch(lengths, [c], k, c_max=c, t_max=int(lengths.max()), total_frames=len(lengths) * int(lengths.max()))
        plan = ops.time_split_plan(b, n_cu=256)
    finally:
        for n, v in saved.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
        _lib.reload_env()
    out = [[] for _ in lengths]
    for vid, first, n, ov in plan:
        out[vid].append((first, n, ov))
    return out


def tol_floor(cum_r):
    """The certificate's tolerance at a cut, at its smallest: 2^-32 (|cumE[r][0]| + 1) (the kernel adds |h| of both units)."""
    return 2.0 ** -32 * (abs(cum_r[0]) + 1.0)


def tau_of(gamma, cum):
    """The stitch's margin for a decision among the states at a position: 2^-30 (|best| + max |cumE| + 1)."""
    return 2.0 ** -30 * (abs(np.max(gamma)) + np.max(np.abs(cum)) + 1.0)


def forward(p, start, stop, kp, h_start=None):
    """fp64 model of the Viterbi forward pass of video 0 over positions start..stop: h[start] = init (start = 0) or h_start,
    nothing older; -> (cumE, h, gamma), rows by position - start.  cumE is the serial prefix sum from position 0."""
    elp = p['elp'][0, :, :p['c']]
    lens, trans = p['lens'][:, :p['c']], p['trans'][:p['c'], :p['c']]
    cum_all = np.concatenate([np.zeros((1, elp.shape[1])), np.cumsum(elp[:stop], axis=0)])
    cum = cum_all[start:stop + 1]
    n_pos = stop - start
    h = np.empty((n_pos + 1, elp.shape[1]))
    gamma = np.full((n_pos + 1, elp.shape[1]), -np.inf)
    h[0] = p['init'][:p['c']] if h_start is None else h_start
    for i in range(1, n_pos + 1):
        km = min(kp - 1, i)
        best = np.max(h[i - km:i][::-1] + lens[1:km + 1], axis=0)
        gamma[i] = cum[i] + best
        h[i] = np.max(gamma[i][None, :] + trans, axis=1) - cum[i]
    return cum, h, gamma


def mirror_problem(seed, t, c, k, units, frac=0.48, magnitude=1e8, delta_tau=0.25, mean_len=None, noise=2.0, drifting=0):
    """The mirror lattice of one video of t frames, c classes per group (2c states), span limit k, cut as `units` (unit_layout
    of this shape).  Every cut lets frac x the certificate's tolerance through; the last unit sees A ahead by about
    (sum of the spreads) - delta_tau x tau while the one-piece decode ends in B.  magnitude: a constant added to every state's
    emission at frame 0 (it raises every |cumE| and with it tol and tau, and changes no decision); it is kept small enough
    (and the emission noise low enough) that tau stays far below the margins of the lattice's own decisions (a boundary moved
    by one frame costs ~18 +- noise): at 1e9 and noise 6 boundaries fall inside tau and the video is repaired for that."""
    from scipy.special import gammaln
    g = np.random.default_rng(seed)
    kp = min(k, t)
    mean_len = mean_len or min(60, (kp - 1) // 2)
    lo, hi = max(8, mean_len // 2), min(kp - 2, (3 * mean_len) // 2)
    a = [u[0] for u in units]                                  # a_0 = 0, a_1, ..., a_J
    r = [u[0] + u[2] for u in units]                           # r_j = a_j + OV (j >= 1)
    n_cuts = len(units) - 1
    # the label sequence: fillers (classes 2..c-1, never one class twice in a row), one DRIFT segment ending well inside every
    # (a_{j-1}, a_j], one FINAL segment ending at t, inside the last unit's own part
    segs, pos = [], 0

    def fill(stop):                                            # fillers from pos to stop, lengths in [lo, hi]
        nonlocal pos
        gap = stop - pos
        if gap <= 0:
            return
        n = -(-gap // hi)
        assert gap >= n * lo, (gap, n, lo)
        parts = [gap // n + (q < gap % n) for q in range(n)]
        for q in range(n - 1):                                 # (jitter, sums and bounds kept)
            x = int(g.integers(-min(parts[q] - lo, hi - parts[q + 1]), min(hi - parts[q], parts[q + 1] - lo) + 1))
            parts[q] += x; parts[q + 1] -= x
        for ln in parts:
            prev = segs[-1][0] if segs else -1
            segs.append((int(g.choice([x for x in range(2, c) if x != prev])), int(ln)))
            pos += int(ln)

    for j in range(1, n_cuts + 1):
        mid = (a[j - 1] + a[j]) // 2
        end_j = mid + int(g.integers(-(a[j] - a[j - 1]) // 8, (a[j] - a[j - 1]) // 8 + 1))
        dl = int(g.integers(lo, hi + 1))
        if 0 < end_j - dl - pos < lo:                          # (no filler fits: the drift segment takes the gap)
            dl = end_j - pos if end_j - pos <= hi else dl + lo
        fill(end_j - dl)
        segs.append((DRIFT, end_j - pos)); pos = end_j
    final_len = int(g.integers(lo, hi + 1))
    fill(t - final_len)
    segs.append((FINAL, final_len)); pos += final_len
    assert pos == t and all(lo <= ln <= hi for _, ln in segs), segs
    assert all(x != y for (x, _), (y, _) in zip(segs, segs[1:]))
    assert t - final_len > r[-1]                               # the FINAL segment ends the last unit's own part
    lab = np.concatenate([np.full(ln, q) for q, ln in segs])

    cs = 2 * c
    margin = 18.0
    e = -290.0 - margin + noise * g.standard_normal((t, c))
    e[np.arange(t), lab] += margin
    e[0] -= magnitude
    elp = np.concatenate([e, e], axis=1)[None]
    kk = np.arange(k)[:, None]
    lam = float(mean_len)
    lens_b = np.repeat(kk * np.log(lam) - lam - gammaln(kk + 1), c, axis=1)
    tr = np.log(g.dirichlet(np.ones(c) * 0.5, size=c).T + 1e-3)
    tr -= np.log(np.exp(tr).sum(0, keepdims=True))
    trans = np.full((cs, cs), -50.0)
    trans[:c, :c] = tr
    trans[c:, c:] = tr
    init = np.tile(np.log(g.dirichlet(np.ones(c))), 2)
    # phi: the DRIFT class spends frac x the smallest tolerance of the cuts per cut
    cum = np.concatenate([np.zeros((1, cs)), np.cumsum(elp[0], axis=0)])
    tol_min = min(tol_floor(cum[r[j]]) for j in range(1, n_cuts + 1))
    phi_drift = -frac * tol_min
    d_last = phi_drift * n_cuts                                 # D(a_J)
    # D(t) = d_last + phi_final = -delta; tau at t: |best| and |cumE| are both about |cumE[t]|
    tau_t = 2.0 ** -30 * (2.0 * np.max(np.abs(cum[t])) + 1.0)
    phi_final = -d_last - delta_tau * tau_t
    lens = np.concatenate([lens_b, lens_b], axis=1)
    lens[:, drifting * c + DRIFT] += phi_drift
    lens[:, drifting * c + FINAL] += phi_final
    return dict(elp=elp, lengths=np.asarray([t]), trans=trans, init=init, lens=lens, endpen=None, c=cs, c_max=cs, k=k,
                labels=lab, segs=segs, phi=(phi_drift, phi_final), drifting=drifting)


def certificate_report(p, units):
    """The fp64 model run the way the split decode runs video 0: once in one piece, once per unit from h = 0 at a_j.
    -> dict: per cut, the spread of h(unit j) - h(unit j-1) over the certified window and tol there; at t, the one-piece and
    the last unit's margins of the drifting group's best state over the other group's, and tau."""
    t, kp = int(p['lengths'][0]), min(p['k'], int(p['lengths'][0]))
    cs = p['c']
    half = cs // 2
    whole = forward(p, 0, t, kp)
    hs = []
    for j, (a0, n, ov) in enumerate(units):
        hs.append(forward(p, a0, a0 + n, kp, None if j == 0 else np.zeros(cs)))
    spreads, tols = [], []
    for j in range(1, len(units)):
        a1, a0 = units[j][0], units[j - 1][0]
        r = a1 + units[j][2]
        s = np.arange(r - (kp - 1), r + 1)
        d = hs[j][1][s - a1] - hs[j - 1][1][s - a0]
        spreads.append(float(d.max() - d.min()))
        tols.append(tol_floor(hs[j][0][r - a1]))

    def margin(cum, gamma):
        gt = gamma[-1]
        m = float(gt[:half].max() - gt[half:].max())
        return (-m if p.get('drifting', 0) else m), tau_of(gt, cum[-1])
    m_whole, tau_whole = margin(whole[0], whole[2])
    m_unit, tau_unit = margin(hs[-1][0], hs[-1][2])
    return dict(spreads=np.asarray(spreads), tols=np.asarray(tols), margin_whole=m_whole, tau_whole=tau_whole,
                margin_unit=m_unit, tau_unit=tau_unit)


def near_tie_problem(seed, t, c, k, units, m, cut=None):
    """A converged lattice of c states with one decision whose one-piece margin is m x tau: the segment [s, n) that crosses the
    cut r_j (s inside the certified window in front of r_j, n in unit j's own part) and its rival [s - 1, n), made as good but
    for m x tau (frame s - 1 explained by both classes, len[n - s + 1] of the class set so).  -> (problem, s, n, margin / tau
    as modelled)."""
    p = mirror_problem(seed, t, c, k, units, frac=0.0, magnitude=0.0, delta_tau=0.0)
    cs = c
    q = dict(p)
    q['elp'] = np.ascontiguousarray(p['elp'][:, :, c:])
    q['trans'] = np.ascontiguousarray(p['trans'][c:, c:])
    q['init'] = p['init'][c:].copy()
    q['lens'] = np.ascontiguousarray(p['lens'][:, c:])
    q['c'] = q['c_max'] = cs
    kp = min(k, t)
    j = cut if cut is not None else len(units) // 2
    r = units[j][0] + units[j][2]
    starts = np.cumsum([0] + [ln for _, ln in p['segs']])
    i = int(np.searchsorted(starts, r, side='right')) - 1           # the segment that holds frame r: [starts[i], starts[i + 1])
    s, n = int(starts[i]), int(starts[i + 1])
    assert r - (kp - 1) < s - 1 and s <= r < n and i >= 1 and i + 1 < len(p['segs'])
    cls, prv, nxt = p['segs'][i][0], p['segs'][i - 1][0], p['segs'][i + 1][0]
    q['elp'][0, s - 1, cls] = q['elp'][0, s - 1, prv]
    cum, h, gamma = forward(q, 0, n, kp)
    kk = n - s
    margin0 = (h[s][cls] + q['lens'][kk][cls]) - (h[s - 1][cls] + q['lens'][kk + 1][cls])
    tau = tau_of(gamma[n] + q['trans'][nxt], cum[n])
    q['lens'][kk + 1][cls] += margin0 - m * tau
    cum, h, gamma = forward(q, 0, n, kp)
    got = ((h[s][cls] + q['lens'][kk][cls]) - (h[s - 1][cls] + q['lens'][kk + 1][cls])) / tau_of(gamma[n] + q['trans'][nxt], cum[n])
    return q, s, n, got


def three_span_problem(seed, t, c, k, units, cut=None, mean_len=60):
    """A converged lattice of c states (every class's length table Poisson(mean_len)) with ONE run of a single class, 3 mean_len + 1
    frames long, that starts inside the certified window in front of the cut r_j and crosses it: one span cannot hold it (span
    limit k), two spans of ~1.5 mean_len cost more than a third span, so it is decoded as three spans (mean_len, mean_len,
    mean_len + 1) in some order -- the three orders tie to within rounding.  -> (problem, run start, run end)."""
    g = np.random.default_rng(seed)
    kp = min(k, t)
    lo, hi = max(8, mean_len // 2), min(kp - 2, (3 * mean_len) // 2)
    j = cut if cut is not None else len(units) // 2
    r = units[j][0] + units[j][2]
    run_len = 3 * mean_len + 1
    assert run_len > kp - 1
    s0 = r - int(g.integers(10, min(kp - 2, run_len - 10)))   # the run's first frame: inside the window, the run crosses r
    segs, pos = [], 0

    run_cls = int(g.integers(0, c))

    def fill(stop):                                            # fillers (never the run's class) from pos to stop
        nonlocal pos
        gap = stop - pos
        n = -(-gap // hi)
        assert gap >= n * lo, (gap, n, lo)
        parts = [gap // n + (q < gap % n) for q in range(n)]
        for q, ln in enumerate(parts):
            prev = segs[-1][0] if segs else -1
            bad = {prev, run_cls}
            segs.append((int(g.choice([x for x in range(c) if x not in bad])), int(ln)))
            pos += int(ln)
    fill(s0)
    segs.append((run_cls, run_len)); pos += run_len
    fill(t)
    assert pos == t and r - (kp - 1) < s0 <= r < s0 + run_len
    lab = np.concatenate([np.full(ln, q) for q, ln in segs])
    from scipy.special import gammaln
    e = -290.0 - 18.0 + 2.0 * g.standard_normal((t, c))
    e[np.arange(t), lab] += 18.0
    kk = np.arange(k)[:, None]
    lens = np.repeat(kk * np.log(mean_len) - mean_len - gammaln(kk + 1), c, axis=1)
    tr = np.full((c, c), -4.0) + g.uniform(-0.5, 0.5, size=(c, c))
    np.fill_diagonal(tr, -8.0)
    tr[run_cls, run_cls] = -1.5                                 # the run's class may follow itself
    tr -= np.log(np.exp(tr).sum(0, keepdims=True))
    init = np.log(g.dirichlet(np.ones(c)))
    return dict(elp=e[None], lengths=np.asarray([t]), trans=tr, init=init, lens=lens, endpen=None, c=c, c_max=c, k=k,
                labels=lab, segs=segs), s0, s0 + run_len
