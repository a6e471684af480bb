"""Host-side inputs of the entropy / cross-entropy / KL gradient tests (numpy only; no GPU): the enumerable lattices of
test_gpu_entropy_grad.py and the mid-size cases that are compared entry by entry with tests/entropy_grad_dp_ref.py.  Every seed
is fixed."""
import functools

import numpy as np

SMALL = [
    # (K, add_eos, masks, extra allowed ends, narration constraints)
    (2, True, False, False, False),
    (4, True, False, False, False),
    (4, False, False, False, False),
    (2, False, False, False, False),
    (4, True, True, False, False),
    (4, False, True, False, False),
    (4, True, True, True, False),
    (4, True, False, False, True),
    (3, False, True, False, True),
]


def _lsm(a, ax):
    return a - np.log(np.exp(a - a.max(ax, keepdims=True)).sum(ax, keepdims=True)) - a.max(ax, keepdims=True)


def _small_tables(k, add_eos, masked, additional, narration, seed, like=None, shift=None):
    """One small padded batch of 3 states and 3 videos: (elp_bt, lengths, trans, init, lens, endpen) as numpy.  `like` with
    `shift`: the same tables with elp moved by shift x N(0, 1) (a q near p); `like` alone: the same masks, other values."""
    rng = np.random.default_rng(seed)
    c, lengths = 3, [7, 5, 6]
    b, tmax = len(lengths), max(lengths)
    if like is not None and shift is not None:
        elp = like[0] + shift * rng.normal(size=like[0].shape) * (like[0] > -1e8)
        return (elp,) + tuple(like[1:])
    lsm = _lsm
    trans = lsm(rng.normal(size=(c, c)), 0)
    init = lsm(rng.normal(size=c), 0)
    lens = np.zeros((k, c))
    lens[1:] = lsm(rng.normal(size=(k - 1, c)), 0)
    elp = rng.normal(size=(b, tmax, c)) * 1.5
    for i, t in enumerate(lengths):
        elp[i, t:] = 0.0
    if masked:
        trans[2, 0] = trans[0, 2] = -1e9
        init[2] = -1e9
    if narration:
        elp[0, 2, 1] = -1e9
        elp[1, 0:2, 2] = -1e9
    ep = None
    if add_eos and (masked or additional):
        ep = np.zeros((b, c))
        ep[:, 0] = -1e9
        if additional:
            ep[1, 0] = 0.0
    return elp, lengths, trans, init, lens, ep


def _small_case(k, add_eos, masked, additional, narration, q_kind):
    seed = 500 + k + 10 * add_eos + 20 * masked + 40 * additional + 80 * narration
    p = _small_tables(k, add_eos, masked, additional, narration, seed)
    if q_kind == 'draw':
        q = _small_tables(k, add_eos, masked, additional, narration, seed + 1)
    else:
        q = _small_tables(k, add_eos, masked, additional, narration, seed + 2, like=p, shift=1e-3)
    return p, q


# ------------------------------------------------------------------------------------------------------- mid sizes
# Each case crosses work splits of csrc/smm_entropy_bwd.hip that the enumerable lattices leave in their trivial regime.
#   states: per group;  runs: label run lengths, uniform in [lo, hi) or given;  up: upstream weight per video
MID = dict(
    # three trips of the 32-lane length loop; three node slabs, n0 + 64 == T (64 frames); elp chunks of 5 frames
    k_trips=dict(states=[5], k=70, lengths=[150, 64, 65], eos=True, runs=(20, 70), up=[1.0, -0.5, 2.0], seed=7102),
    # second block of the length kernel (k > 256); ten trips of the lane loop
    k_blocks=dict(states=[3], k=300, lengths=[330], eos=True, runs=[20, 280, 30], up=[1.5], seed=7200),
    # all 32 class groups; 1024 pairs; the 64-lane last decision half full; a one-frame video
    states_32=dict(states=[32], k=12, lengths=[128, 127, 1], eos=True, runs=(3, 12), up=[1.0, -0.5, 2.0], seed=7300),
    # one slice of the boundaries per pair; the closing transition and the closing elp row; T = 128, 64, 1
    states_23_no_eos=dict(states=[23], k=40, lengths=[129, 65, 2], eos=False, runs=(8, 40), up=[1.0, -0.5, 2.0], seed=7400),
    # group sums in video order; padded states; per-video kp; a zero upstream weight
    packed_groups=dict(states=[6, 17], k=40, lengths=[70, 64, 129, 33, 2], eos=True, runs=(8, 40), group=[0, 1, 1, 0, 1],
                       kp=[40, 40, 20, 40, 3], up=[1.0, -0.5, 2.0, 0.0, 0.25], seed=7500),
)
MID_TAIL = 3                                  # frames of the packed axis behind the last video (no video covers them)


def _labels(rng, frames, runs, c):
    """A label per frame, in runs (neighbouring runs differ)."""
    out, prev, i = [], -1, 0
    while len(out) < frames:
        n = runs[i] if isinstance(runs, list) else int(rng.integers(runs[0], runs[1]))
        lab = int(rng.integers(0, c - 1)) if prev >= 0 else int(rng.integers(0, c))
        lab += 0 <= prev <= lab
        out += [lab] * n
        prev, i = lab, i + 1
    return np.array(out[:frames])


def _mid_side(cfg, labels, seed):
    """One side's tables of a mid-size case, stacked per group and zero-padded to c_max columns (as ops.factor_tables and the
    module's packed path fill them): (elp [total_frames, c_max], trans [g, c_max, c_max], init, lens, endpen [b, c_max] or None).
    Emissions 2 x onehot(label) + N(0, 1); -1e9 masks per group: the transitions 0 <-> 2, the initial state 2, frames 30 .. 39
    of state 1 in the group's first video, with EOS the end in state 0."""
    rng = np.random.default_rng(seed)
    states, k, lengths = cfg['states'], cfg['k'], cfg['lengths']
    group = cfg.get('group', [0] * len(lengths))
    cm, ng, b = max(states), len(states), len(lengths)
    trans, init, lens = np.zeros((ng, cm, cm)), np.zeros((ng, cm)), np.zeros((ng, k, cm))
    for g, c in enumerate(states):
        trans[g, :c, :c] = _lsm(rng.normal(size=(c, c)), 0)
        init[g, :c] = _lsm(rng.normal(size=c), 0)
        lens[g, 1:, :c] = _lsm(rng.normal(size=(k - 1, c)), 0)
        trans[g, 2, 0] = trans[g, 0, 2] = -1e9
        init[g, 2] = -1e9
    off = np.concatenate([[0], np.cumsum(lengths)])
    elp = np.zeros((int(off[-1]) + MID_TAIL, cm))
    windowed = set()
    for i, t in enumerate(lengths):
        c = states[group[i]]
        e = rng.normal(size=(t, c))
        e[np.arange(t), labels[i]] += 2.0
        if group[i] not in windowed and t >= 40:
            e[30:40, 1] = -1e9
            windowed.add(group[i])
        elp[off[i]:off[i] + t, :c] = e
    ep = None
    if cfg['eos']:
        ep = np.full((b, cm), -1e9)               # (padded states may not end a video)
        for i in range(b):
            ep[i, 1:states[group[i]]] = 0.0
    return elp, trans, init, lens, ep


@functools.lru_cache(maxsize=None)
def mid_case(name):
    """-> dict(p, q: _mid_side tuples -- q a fresh draw of every value on p's videos (the same label runs) with p's masks;
    lengths, frame_offset, group, n_states, kp (per video, as the kernels clamp it), k, c_max, no_eos, up, total_frames,
    single: one group and no per-video arguments)."""
    cfg = MID[name]
    lengths, states = cfg['lengths'], cfg['states']
    group = cfg.get('group', [0] * len(lengths))
    rng = np.random.default_rng(cfg['seed'])
    labels = [_labels(rng, t, cfg['runs'], states[g]) for t, g in zip(lengths, group)]
    off = np.concatenate([[0], np.cumsum(lengths)])
    kp = cfg.get('kp', [min(cfg['k'], max(lengths))] * len(lengths))
    return dict(p=_mid_side(cfg, labels, cfg['seed'] + 1), q=_mid_side(cfg, labels, cfg['seed'] + 2), lengths=lengths,
                frame_offset=[int(v) for v in off[:-1]], group=group, n_states=states, kp=kp, k=cfg['k'], c_max=max(states),
                no_eos=not cfg['eos'], up=np.array(cfg['up']), total_frames=int(off[-1]) + MID_TAIL,
                single='group' not in cfg)


def video_side(case, i, which='p'):
    """Video i of a mid_case alone: (dict(elp [frames, c], trans, init, len) of its group's real states, endpen [c] or None)."""
    t, g, o, fr = case[which], case['group'][i], case['frame_offset'][i], case['lengths'][i]
    c = case['n_states'][g]
    return (dict(elp=t[0][o:o + fr, :c], trans=t[1][g, :c, :c], init=t[2][g, :c], len=t[3][g, :, :c]),
            None if t[4] is None else t[4][i, :c])


@functools.lru_cache(maxsize=None)
def mid_reference(name):
    """{mode: (values, p's grads, q's grads)} of mid_case(name) by tests/entropy_grad_dp_ref.py, in the packed, grouped layouts
    (elp [total_frames, c_max], trans [g, c_max, c_max], init [g, c_max], len [g, k, c_max]).  Computed once per process and
    shared: leave it unchanged."""
    import entropy_grad_dp_ref as D
    case = mid_case(name)
    p, q = case['p'], case['q']
    qa = (q[0], case['lengths'], q[1], q[2], q[3], q[4])
    return D.batch_reference(p[0], case['lengths'], p[1], p[2], p[3], case['kp'], case['no_eos'], p[4], qa, None, case['up'],
                             group=case['group'], n_states=case['n_states'], frame_offset=case['frame_offset'])


def long_span_share(name, video, at_least):
    """Share of the expected spans of one video of mid_case(name), under p, that are at least `at_least` positions long."""
    import entropy_grad_dp_ref as D
    case = mid_case(name)
    side, ep = video_side(case, video)
    mu = D.length_marginals(side, case['kp'][video], case['no_eos'], ep).numpy()
    return float(mu[at_least:].sum() / mu.sum())
