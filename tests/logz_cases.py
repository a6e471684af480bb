"""Host-side inputs of the log-partition grid (tests/test_gpu_logz_grid.py; numpy + scipy only, no GPU): lattices whose
posterior LIVES on long segments, and the table of cases that crosses every work split of csrc/smm_logz.hip and
csrc/smm_logz_bwd.hip.  Every seed is fixed.

smm_logz_kernel's chain wave evaluates the K0 = 2B shortest segment lengths of a position itself; every longer length sits in
the pusher waves' fp32 ring slots (forward) and in smm_glen_kernel's tiles (backward).  On i.i.d. normal lattices
(test_gpu_viterbi.make_problem) the posterior never uses a length beyond K0, so a dead ring passes every bar.  Here a
segmentation is PLANTED per video: every state has a length rate (one kp - 1, one near 0.6 kp, the rest spread over
(K0 + 2, 30]), the length table is a flattened Poisson log-pmf around the rate, the emissions carry a per-frame bonus on the
planted label.  tests/test_logz_cases_host.py asserts from the C twin alone that the posterior mass of every ring-reaching
case lies where the rings are."""
import functools

import numpy as np
from scipy.special import gammaln

from oracle import factored as F

BONUS = 2.0          # per frame, on the planted label
FLAT = 0.5           # the Poisson log-pmf is multiplied by this: neighbouring lengths stay in reach
EOS_MODES = ('ends', 'eos', 'no_eos')        # add_eos with end penalties / without them / add_eos=False


def ring_regs(kp):
    """R of smm_launch_logz: ring registers per lane, 64 R >= kp_max."""
    r = 1
    while 64 * r < kp:
        r *= 2
    return r


def block(kp):
    """B: positions per hand-over block (2 on rings of up to 128 slots)."""
    return 2 if ring_regs(kp) <= 2 else 4


def k0(kp):
    """Lengths 1..K0 stay with the chain wave."""
    return 2 * block(kp)


def spw(c):
    return (c + 6) // 7


def hf(c):
    return 4 if c <= 16 else 16


def instantiation(kp, c):
    """(R, SPW, HF): the template arguments smm_launch_logz picks for a launch of kp_max = kp and at most c states."""
    return ring_regs(kp), spw(c), hf(c)


STATE_CLASSES = ((1, 7), (8, 14), (15, 16), (17, 21), (22, 28), (29, 32))
RINGS = (1, 2, 4, 8, 16)
ALL_INSTANTIATIONS = frozenset((r,) + instantiation(64, hi)[1:] for r in RINGS for _, hi in STATE_CLASSES)


# ------------------------------------------------------------------------------------------------------------ the case table
def _case(name, kp, c, eos, t_long=None, t_short=None, edge=False):
    return dict(name=name, kp=kp, c=c, eos=eos, t_long=t_long, t_short=t_short, edge=edge)


def _grid():
    # one case per (R, state class) at the class's upper bound.  kp per (R, class): the ring-size boundaries 64, 65, 128, 129,
    # 256, 257, 512, 513, 1024 and the backward's tile edges kp - 1 in {32, 33, 64, 65, 128, 129, 256, 257, 513, 769}, rotated
    # over the classes.  EOS handling alternates: every R and every class sees all three.
    kps = {1: (64, 33, 34, 64, 40, 64), 2: (65, 128, 66, 128, 100, 65), 4: (129, 256, 130, 200, 256, 129),
           8: (257, 512, 258, 400, 512, 257), 16: (513, 1024, 514, 770, 640, 600)}
    # video lengths where they are named: the marginals' slabs of 512 positions and 32-chunk scan, smm_glen's s tiles
    named = {
        (1, 7): dict(t_short=(31, 33)), (2, 7): dict(t_short=(33, 2)), (4, 7): dict(t_short=(31, 1)),
        (8, 7): dict(t_long=(1024, None), t_short=(33, 3)), (16, 7): dict(t_long=(1025, 1024), t_short=(511, 2)),
        (16, 16): dict(t_short=(513, 512)), (16, 14): dict(t_short=(1023, 513)), (8, 14): dict(t_short=(511, 33)),
        (1, 14): dict(t_short=(30, 3)), (2, 16): dict(t_short=(31, 1)), (4, 16): dict(t_short=(33, 3)),
    }
    out = []
    for ri, r in enumerate(RINGS):
        for ci, (_, hi) in enumerate(STATE_CLASSES):
            out.append(_case('R%d-c%d-kp%d' % (r, hi, kps[r][ci]), kps[r][ci], hi, EOS_MODES[(ri + ci) % 3],
                             **named.get((r, hi), {})))
    # the classes' lower bounds, each at two ring sizes
    lows = ((1, 64, 0), (1, 1024, 1), (8, 128, 2), (8, 512, 0), (15, 256, 1), (15, 34, 2), (17, 66, 0), (17, 513, 1),
            (22, 257, 2), (22, 130, 0), (29, 64, 1), (29, 520, 2))
    for c, kp, e in lows:
        out.append(_case('R%d-c%d-kp%d' % (ring_regs(kp), c, kp), kp, c, EOS_MODES[e]))
    # no ring length in reach (kp - 1 <= K0), or hardly any: exempt from the mass conditions
    out.append(_case('edge-kp2', 2, 4, 'eos', edge=True))
    out.append(_case('edge-kp5', 5, 9, 'ends', edge=True))
    out.append(_case('edge-kp9', 9, 3, 'no_eos', edge=True))
    return tuple(out)


CASES = _grid()
CASE_NAMES = tuple(cs['name'] for cs in CASES)
assert len(set(CASE_NAMES)) == len(CASE_NAMES)


def case(name):
    return CASES[CASE_NAMES.index(name)]


# ------------------------------------------------------------------------------------------------------------ the generator
def rates_of(g, kp, c):
    """Length rate per state: one state kp - 1, one near 0.6 kp, the rest spread over (K0 + 2, ~30] (all within 1..kp - 1)."""
    top = max(1, kp - 1)
    lo = min(top, k0(kp) + 3)
    rest = np.round(np.linspace(lo, max(lo, min(30, kp - 2)), max(c - 2, 1))).astype(int)[:max(c - 2, 0)]
    rates = np.concatenate([[top], [max(1, min(top, int(round(0.6 * kp))))], g.permutation(rest)])[:c]
    return rates[g.permutation(c)] if c > 1 else rates


def length_table(rates, kp):
    """[kp][c]: flattened Poisson log-pmf around each state's rate; a single state gets two sharp peaks (kp - 1 and ~0.6 kp),
    because nothing but the table can select a length there."""
    kk = np.arange(kp, dtype=np.float64)[:, None]
    if len(rates) == 1:
        m = max(1, int(round(0.6 * kp)))
        return np.logaddexp(-0.7 * np.abs(kk - (kp - 1)), -0.7 * np.abs(kk - m))
    r = np.asarray(rates, dtype=np.float64)[None, :]
    return FLAT * (kk * np.log(r) - r - gammaln(kk + 1))


def _labels(segs):
    return np.concatenate([np.full(n, s, dtype=np.int64) for s, n in segs])


def _plant_long(g, rates, c, shrink, t_target):
    """Every state once, at its rate (the kp - 1 state `shrink` frames shorter); then short states until t_target."""
    a = int(np.argmax(rates))
    order = g.permutation(c)
    segs = [(int(s), int(rates[s]) - (shrink if s == a else 0)) for s in order]
    segs = [(s, max(1, n)) for s, n in segs]
    if c == 1:                                             # (a second segment: a video of kp - 1 frames has span limit kp - 1)
        segs.append((0, max(1, int(round(0.6 * (rates[0] + 1))))))
    if t_target is not None:
        short = [int(s) for s in np.argsort(rates)[:max(1, c - 2)]]
        assert len(short) >= 2, 'a named length needs two short states to alternate'
        i = 0
        while sum(n for _, n in segs) < t_target:
            s = short[i % len(short)]
            if s == segs[-1][0]:
                i += 1
                continue
            segs.append((s, min(int(rates[s]), t_target - sum(n for _, n in segs))))
            i += 1
        assert sum(n for _, n in segs) == t_target, 'the planted states do not fit %d frames' % t_target
    return segs


def _plant_short(g, rates, c, t):
    """t frames: the shorter states in turn (the ~0.6 kp state first where it fits), the last segment cut at t."""
    by_rate = [int(s) for s in np.argsort(rates)]
    turn = by_rate[:-1] if c > 1 else by_rate
    if c > 2 and rates[turn[-1]] <= t:
        turn = [turn[-1]] + turn[:-1]
    segs, i = [], int(g.integers(0, len(turn)))
    while sum(n for _, n in segs) < t:
        s = turn[i % len(turn)]
        segs.append((s, min(int(rates[s]), t - sum(n for _, n in segs))))
        i += 1
    return segs


def _spread_residues(ts, fixed, limit):
    """Video lengths that cover every residue mod 4: the lengths not `fixed` grow by up to 3 frames (below `limit`)."""
    seen = set(ts[i] % 4 for i in range(len(ts)) if fixed[i])
    assert len(seen) == sum(fixed), 'the named video lengths repeat a residue mod 4: %r' % (ts,)
    for i in range(len(ts)):
        if not fixed[i]:
            while ts[i] % 4 in seen:
                ts[i] += 1
            assert limit[i] is None or ts[i] < limit[i]
            seen.add(ts[i] % 4)
    return ts


@functools.lru_cache(maxsize=None)
def planted(name):
    """The lattice of a case: dict(elp [4][tmax][c], lengths, trans, init, lens [kp][c], endpen, no_eos, labels, rates, ...).
    Four videos: two hold every state (video 0 one segment of exactly kp - 1 frames), two are shorter than kp."""
    cs = case(name)
    kp, c, eos = cs['kp'], cs['c'], cs['eos']
    g = np.random.default_rng(1000 + CASE_NAMES.index(name))
    rates = rates_of(g, kp, c)
    no_eos = eos == 'no_eos'
    tl, tsh = cs['t_long'] or (None, None), cs['t_short'] or (None, None)
    segs = [_plant_long(g, rates, c, 0, tl[0]), _plant_long(g, rates, c, min(2, kp - 2), tl[1])]
    ts = [sum(n for _, n in s) for s in segs]
    ts += [tsh[0] or max(2, min(kp - 4, int(0.8 * kp))), tsh[1] or max(2, min(kp - 4, int(0.45 * kp)))]
    fixed = [tl[0] is not None, tl[1] is not None, tsh[0] is not None, tsh[1] is not None]
    ts = _spread_residues(ts, fixed, [None, None, kp if kp > 8 else None, kp if kp > 8 else None])
    # a long video that grew for its residue: the frames go to a state that is not the kp - 1 one
    for i in (0, 1):
        grow = ts[i] - sum(n for _, n in segs[i])
        if grow:
            a = int(np.argmax(rates))
            j = next((j for j, (s, _) in enumerate(segs[i]) if s != a), 0)
            segs[i][j] = (segs[i][j][0], segs[i][j][1] + grow)
    segs += [_plant_short(g, rates, c, ts[2]), _plant_short(g, rates, c, ts[3])]
    labels = [_labels(s) for s in segs]
    # (no EOS: the DP covers the frames before the last one; the last frame's label only emits)
    if no_eos:
        labels = [np.concatenate([y, y[-1:]]) for y in labels]
    lengths = np.asarray([len(y) for y in labels], dtype=np.int64)
    b, tmax = len(labels), int(lengths.max())
    elp = g.standard_normal((b, tmax, c)) - 2.0            # (rows past a video's end are noise: nothing may read them)
    for i, y in enumerate(labels):
        elp[i, np.arange(len(y)), y] += BONUS
    trans = g.standard_normal((c, c)) - 1.0
    init = g.standard_normal(c) - 1.0
    lens = length_table(rates, kp)
    endpen = None
    if eos == 'ends':
        endpen = np.full((b, c), -1e9)
        for i, y in enumerate(labels):
            endpen[i, int(y[-1])] = 0.0
            endpen[i, int(g.integers(0, c))] = 0.0
    return dict(elp=elp, lengths=lengths, trans=trans, init=init, lens=lens, endpen=endpen, no_eos=no_eos, c=c, c_max=c,
                k=kp, labels=labels, rates=rates, segs=segs, dp_lengths=lengths - (1 if no_eos else 0))


def upstream(name):
    """Non-uniform upstream weights of the four videos, with a zero and a negative entry (which videos get them alternates)."""
    up = (1.25, -0.75, 0.5, 0.0) if CASE_NAMES.index(name) % 2 == 0 else (-0.75, 1.25, 0.0, 0.5)
    return np.asarray(up)


def twin(p, upstream=None, lens=None, grad=True):
    """The C twin on a planted lattice: (log Z [b], gradients) -- the reference of the GPU test."""
    return F.logz(p['elp'], p['lengths'], p['trans'], p['init'], p['lens'] if lens is None else lens, p['endpen'], grad=grad,
                  upstream=upstream, no_eos=p['no_eos'])


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once per case and shared (never modified): the twin's log Z and gradients at upstream(name)."""
    z, g = twin(planted(name), upstream(name))
    for a in (z,) + tuple(g.values()):
        a.setflags(write=False)
    return z, g


def dead_ring_table(p):
    """The length table with every ring length (k > K0) out of reach."""
    lens = p['lens'].copy()
    lens[k0(p['k']) + 1:] = -1e9
    return lens


# ------------------------------------------------------------------------------------------------------------ mixed launches
# (states of the group that picks the kernel, states of the group that rides in it, kp_max, the small kp, c_max).  c_max is
# larger than every group's state count wherever the library's limit of 32 columns leaves room.
MIXED = ((32, 3, 129, 9, 32), (17, 16, 65, 5, 20), (23, 9, 600, 9, 27), (8, 7, 257, 9, 11))
MIXED_NAMES = tuple('mixed-%d+%d-kp%d' % m[:3] for m in MIXED)


@functools.lru_cache(maxsize=None)
def mixed(name):
    """Two parameter groups in one launch, packed frame axis, padded columns (filled with noise: nothing may read them), kp per
    video: the first group's videos at kp_max and at a smaller kp, the second's at kp_max, one in between and one at
    kp <= K0 + 1.  -> dict(elp [total][c_max], lengths, frame_offset, group, kp, states, trans / init / lens [2][..], endpen,
    parts): `parts` lists, per (group, kp), the videos and the unpadded problem of one twin call."""
    big, small, kp_max, kp_small, cm = MIXED[MIXED_NAMES.index(name)]
    g = np.random.default_rng(7000 + MIXED_NAMES.index(name))
    states = (big, small)
    assert kp_small <= k0(kp_max) + 1 and cm >= big
    kp_mid = kp_max // 2 + 2
    plan = ((0, kp_max, None), (1, kp_max, None), (0, kp_mid, None), (1, kp_mid, None), (1, kp_small, 3 * kp_small + 1),
            (0, kp_max, kp_max - 3))
    trans = g.standard_normal((2, cm, cm)) - 1.0
    init = g.standard_normal((2, cm)) - 1.0
    lens = g.standard_normal((2, kp_max, cm))
    rates = [rates_of(g, kp_max, c) for c in states]
    for gi, c in enumerate(states):
        lens[gi, :, :c] = length_table(rates[gi], kp_max)
    labels = []
    for gi, kp, t in plan:
        c = states[gi]
        r = np.minimum(rates[gi], kp - 1)                  # (what a video of span limit kp can hold in one segment)
        labels.append(_labels(_plant_long(g, r, c, 0, None)) if t is None else _labels(_plant_short(g, r, c, t)))
    lengths = np.asarray([len(y) for y in labels], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    elp = g.standard_normal((int(lengths.sum()), cm)) - 2.0
    endpen = g.standard_normal((len(plan), cm))            # (padded columns: noise)
    for i, ((gi, kp, _), y) in enumerate(zip(plan, labels)):
        c = states[gi]
        elp[offs[i] + np.arange(len(y)), y] += BONUS
        endpen[i, :c] = -1e9
        endpen[i, int(y[-1])] = 0.0
        endpen[i, int(g.integers(0, c))] = 0.0
    parts = []
    for key in sorted(set((gi, kp) for gi, kp, _ in plan)):
        vids = [i for i, (gi, kp, _) in enumerate(plan) if (gi, kp) == key]
        gi, kp = key
        c = states[gi]
        tmax = int(lengths[vids].max())
        e = np.zeros((len(vids), tmax, c))
        for j, i in enumerate(vids):
            e[j, :lengths[i]] = elp[offs[i]:offs[i] + lengths[i], :c]
        parts.append(dict(group=gi, kp=kp, videos=vids, elp=e, lengths=lengths[vids], trans=trans[gi, :c, :c], init=init[gi, :c],
                          lens=lens[gi, :kp, :c], endpen=endpen[vids, :c]))
    return dict(elp=elp, lengths=lengths, frame_offset=offs, group=np.asarray([p[0] for p in plan], dtype=np.int32),
                kp=np.asarray([p[1] for p in plan], dtype=np.int32), states=states, c_max=cm, k=kp_max, trans=trans, init=init,
                lens=lens, endpen=endpen, parts=parts, upstream=np.asarray([1.25, -0.75, 0.5, 1.0, 0.0, 0.8]))


@functools.lru_cache(maxsize=None)
def mixed_reference(name):
    """One twin call per (group, kp): log Z per video, elp gradients per video, table gradients summed per group."""
    m = mixed(name)
    cm, kp_max = m['c_max'], m['k']
    z = np.zeros(len(m['lengths']))
    g_elp = np.zeros_like(m['elp'])
    tabs = dict(trans=np.zeros((2, cm, cm)), init=np.zeros((2, cm)), len=np.zeros((2, kp_max, cm)))
    for part in m['parts']:
        gi, c, vids = part['group'], part['trans'].shape[0], part['videos']
        zz, gg = F.logz(part['elp'], part['lengths'], part['trans'], part['init'], part['lens'], part['endpen'], grad=True,
                        upstream=m['upstream'][vids])
        z[vids] = zz
        for j, i in enumerate(vids):
            o, t = m['frame_offset'][i], m['lengths'][i]
            g_elp[o:o + t, :c] = gg['elp'][j, :t]
        tabs['trans'][gi, :c, :c] += gg['trans']
        tabs['init'][gi, :c] += gg['init']
        tabs['len'][gi, :gg['len'].shape[0], :c] += gg['len']
    g_elp_mask = np.zeros_like(m['elp'], dtype=bool)
    for i, gi in enumerate(m['group']):
        g_elp_mask[m['frame_offset'][i]:m['frame_offset'][i] + m['lengths'][i], :m['states'][gi]] = True
    return z, dict(elp=g_elp, **tabs), g_elp_mask
