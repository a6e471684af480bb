"""One small feature-driven decode corpus with SEVERAL parameter groups, for the tests of smm_decode_f32's plan features in
composition (tests/test_gpu_decode_plans.py) and the host test of the conditions those lean on (tests/test_decode_plans_host.py).

In the style of test_gpu_fullsize.make_corpus: labels are HSMM-sampled, x = mu[label] + sigma * eps, the length tables are
Poisson, the parameters are the truth slightly perturbed.  D = 24, K = 520 (kp_max > 512: BAND mode), per-video kp = min(K, T);
groups of 23, 9, 17, 13 and 16 states in tables padded to c_max = 24; 28 videos: three long ones of 3100, 2950 and 2800 frames
(23, 9 and 17 states) and 25 of 9..1500 frames over all groups.

Sizing.  With SMM_CHUNK_P=1 and the default warm-up a unit of a video with kp = 520 needs ov = 512 + 519 positions in front of an
own part of at least lmin = 519, so a video is cut from ov + 2 lmin = 2069 frames on: the three long videos, no other.  With
SMM_CHUNK=0, SMM_SPLIT_MIN_US=0 and the default margin of 400 choose_split's threshold is about tmax - 404 = 2696: the same three
videos are the critical part (3 <= 28 / 3 and 25 >= 16 beside them).

Two dressings:
  plain    packed frame axis, nothing else
  dressed  narration-style constraints (-1e4 outside a window around a step's true frames), end penalties (-1e9 but on two or
           three states per video), a class map to arbitrary ids, gaps on the frame axis

The C twin's results (oracle.factored: the fp64 direct-form emission and the Viterbi decode, per video with its group's tables)
are computed once per dressing and kept; nothing a test gets from here is to be changed."""
import functools
import os

import numpy as np

from oracle import dense_ref as O
from oracle import factored as F

D, K, C_MAX = 24, 520, 24
STATES = (23, 9, 17, 13, 16)
LONG = {5: (3100, 0), 12: (2950, 1), 20: (2800, 2)}        # position in the batch -> (frames, group)
SHORT = (9, 33, 120, 519, 520, 521, 1500)                   # among the other 25 lengths: one tile, around kp = K, the longest
EOS_ID, N_IDS = 200, 200
DRESSINGS = ('plain', 'dressed')


def _sample_labels(g, t, c, rates):
    out, cur, tot = [], int(g.integers(0, c)), 0
    while tot < t:
        ln = int(np.clip(g.poisson(rates[cur]), 1, K - 1))
        out.append(np.full(ln, cur)); tot += ln; cur = (cur + 1) % c
    return np.concatenate(out)[:t]


@functools.lru_cache(maxsize=None)
def corpus(dressing, seed=5):
    """Host arrays of the launch: lengths, group, kp, frame_off, total, x [total, D] fp32, the tables of every group padded to
    C_MAX (w, cst, inv_var, trans, init, lens), cons / endpen / class_map (None when plain), the sampled labels per video, and
    the unpadded per-group parameters for the twin."""
    from scipy.special import gammaln
    assert dressing in DRESSINGS
    dressed = dressing == 'dressed'
    g = np.random.default_rng(seed)
    b, n_groups = 28, len(STATES)
    lengths = np.zeros(b, np.int64)
    group = np.zeros(b, np.int32)
    rest = [i for i in range(b) if i not in LONG]
    others = np.concatenate([SHORT, g.integers(60, 1401, size=len(rest) - len(SHORT))])
    others = others[g.permutation(len(others))]
    for j, i in enumerate(rest):
        lengths[i], group[i] = others[j], j % n_groups                       # five videos per group
    for i, (t, gi) in LONG.items():
        lengths[i], group[i] = t, gi
    n_small = int(sum(STATES[group[i]] <= 16 for i in rest))
    assert n_small >= 8 and len(rest) - n_small >= 6 and lengths[rest].max() == 1500 and lengths.min() == 9
    kp = np.minimum(K, lengths).astype(np.int32)
    if dressed:
        gap = g.integers(0, 5, size=b)
        frame_off = np.concatenate([[0], np.cumsum(lengths + gap)[:-1]]) + 3
        total = int(frame_off[-1] + lengths[-1] + 2)
    else:
        frame_off = np.concatenate([[0], np.cumsum(lengths)[:-1]])
        total = int(lengths.sum())
    sigma = g.uniform(0.7, 1.3, size=D)
    var = sigma ** 2
    lognorm = float(-0.5 * np.log(var).sum() - 0.5 * D * np.log(2 * np.pi))
    kk = np.arange(K)[:, None]
    par = []
    for c in STATES:
        mu = g.normal(0, 0.9, size=(c, D))
        rates = g.uniform(20, 400, size=c)                                    # well below K, as structured_problem's
        trans = np.log(g.dirichlet(np.ones(c) * 0.5, size=c).T + 1e-3)
        trans -= np.log(np.exp(trans).sum(0, keepdims=True))
        par.append(dict(c=c, mu=mu, rates=rates, mu_hat=mu + g.normal(0, 0.02, size=mu.shape), trans=trans,
                        init=np.log(g.dirichlet(np.ones(c))), lens=kk * np.log(rates) - rates - gammaln(kk + 1)))
    x = g.standard_normal((total, D)).astype(np.float32)                      # (finite in the gaps too)
    labs = []
    for i in range(b):
        p = par[group[i]]
        lab = _sample_labels(g, int(lengths[i]), p['c'], p['rates'])
        labs.append(lab)
        x[frame_off[i]:frame_off[i] + lengths[i]] = (p['mu'][lab] + sigma * g.standard_normal((len(lab), D))).astype(np.float32)
    # the tables, padded to C_MAX columns
    w = np.zeros((n_groups, D, C_MAX)); cst = np.zeros((n_groups, C_MAX))
    trans = np.full((n_groups, C_MAX, C_MAX), -1e9); init = np.full((n_groups, C_MAX), -1e9)
    lens = np.full((n_groups, K, C_MAX), -1e9)
    for gi, p in enumerate(par):
        c = p['c']
        w[gi, :, :c] = (p['mu_hat'] / var).T
        cst[gi, :c] = lognorm - 0.5 * (p['mu_hat'] ** 2 / var).sum(1)
        trans[gi, :c, :c], init[gi, :c], lens[gi, :, :c] = p['trans'], p['init'], p['lens']
    cons = endpen = class_map = None
    if dressed:
        cons = np.zeros((total, C_MAX), np.float32)
        endpen = np.full((b, C_MAX), -1e9)
        for i, lab in enumerate(labs):
            t, c = len(lab), STATES[group[i]]
            for j in range(1, c, 2):                                          # odd states = steps (test_gpu_fullsize._constrained_corpus)
                pos = np.flatnonzero(lab == j)
                lo, hi = (0, t) if len(pos) == 0 else (max(0, pos.min() - int(g.integers(0, 20))),
                                                       min(t, pos.max() + 1 + int(g.integers(0, 20))))
                cons[frame_off[i]:frame_off[i] + lo, j] = -1e4
                cons[frame_off[i] + hi:frame_off[i] + t, j] = -1e4
            # two or three states, the true last one among them
            ends = [int(lab[-1])] + [int(e) for e in g.choice([s for s in range(c) if s != lab[-1]], size=int(g.integers(1, 3)), replace=False)]
            endpen[i, ends] = 0.0
        class_map = np.zeros((n_groups, C_MAX + 1), np.int64)
        for gi, c in enumerate(STATES):
            class_map[gi, :c] = g.permutation(N_IDS)[:c]
            class_map[gi, c] = EOS_ID
    return dict(dressing=dressing, b=b, lengths=lengths, group=group, kp=kp, frame_off=frame_off, total=total, x=x, w=w, cst=cst,
                inv_var=1.0 / var, lognorm=lognorm, trans=trans, init=init, lens=lens, cons=cons, endpen=endpen,
                class_map=class_map, labs=labs, par=par)


def covered(cp):
    """bool [total]: the frames some video covers."""
    m = np.zeros(cp['total'], bool)
    for f0, t in zip(cp['frame_off'], cp['lengths']):
        m[f0:f0 + t] = True
    return m


def reference_emission(cp):
    """The fp64 direct form lognorm - 1/2 sum_d (x - mu)^2 / sigma^2 + cons of every video under its group's parameters:
    a list of [T_i, c_i] arrays."""
    ref = [None] * cp['b']
    for gi, p in enumerate(cp['par']):
        idx = np.flatnonzero(cp['group'] == gi)
        tg, c = int(cp['lengths'][idx].max()), p['c']
        xp = np.zeros((len(idx), tg, D), np.float32)
        cn = None if cp['cons'] is None else np.zeros((len(idx), tg, c))
        for j, i in enumerate(idx):
            f0, t = int(cp['frame_off'][i]), int(cp['lengths'][i])
            xp[j, :t] = cp['x'][f0:f0 + t]
            if cn is not None:
                cn[j, :t] = cp['cons'][f0:f0 + t, :c]
        e = F.emission(xp, cp['lengths'][idx], p['mu_hat'], cp['inv_var'], cp['lognorm'], cn)
        for j, i in enumerate(idx):
            ref[i] = e[j, :cp['lengths'][i]].copy()
    return ref


def twin_viterbi(cp, elp):
    """The C twin's decode of every video on ``elp`` (a list of [T_i, c_i] arrays) with its group's tables, its kp = min(K, T_i)
    and its end penalties -> (spans: list of int64 [T_i + 1] in LOCAL ids with EOS = c_i, best fp64 [b])."""
    spans, best = [], np.empty(cp['b'])
    for i in range(cp['b']):
        p = cp['par'][cp['group'][i]]
        t, c = int(cp['lengths'][i]), p['c']
        ep = None if cp['endpen'] is None else cp['endpen'][i:i + 1, :c]
        s, v = F.viterbi(elp[i][None], [t], p['trans'], p['init'], p['lens'][:cp['kp'][i]], ep)
        spans.append(s[0]); best[i] = v[0]
    return spans, best


def global_ids(cp, i, local):
    """Local state ids of video i (-1 stays -1, c_i = EOS) as the launch reports them: through the class map, if there is one."""
    local = np.asarray(local)
    if cp['class_map'] is None:
        return local
    return np.append(cp['class_map'][cp['group'][i]], -1)[local]


@functools.lru_cache(maxsize=None)
def twin(dressing):
    """The twin on the reference emission: dict(elp, spans, best, labels) -- labels: local ids per frame, a list of [T_i]."""
    cp = corpus(dressing)
    elp = reference_emission(cp)
    spans, best = twin_viterbi(cp, elp)
    labels = [O.spans_to_labels(s[None, :-1])[0] for s in spans]
    return dict(elp=elp, spans=spans, best=best, labels=labels)


def make_batch(cp):
    from action_segmentation_amd import ops
    return ops.Batch(cp['lengths'], STATES, K, c_max=C_MAX, frame_offset=cp['frame_off'], group=cp['group'], kp=cp['kp'], d=D,
                     t_max=int(cp['lengths'].max()), total_frames=cp['total'])


def time_split_units(cp, unit=1, n_cu=256):
    """The planner's units of this launch under SMM_CHUNK=1 and SMM_CHUNK_P=unit (host logic of libsmmdp.so, built if missing
    or stale; the caller's switches are put back): per video, a list of (first position, positions, positions in front of the
    own part) -- empty for a video that is decoded in one piece."""
    from action_segmentation_amd import ops, _lib, _build
    _build.build()
    names = ('SMM_CHUNK', 'SMM_CHUNK_P', 'SMM_CHUNK_WC', 'SMM_CHUNK_LMIN')
    saved = {n: os.environ.get(n) for n in names}
    try:
        os.environ['SMM_CHUNK'], os.environ['SMM_CHUNK_P'] = '1', str(unit)
        for n in names[2:]:
            os.environ.pop(n, None)
        _lib.reload_env()
        plan = ops.time_split_plan(make_batch(cp), n_cu=n_cu)
    finally:
        for n, v in saved.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
        _lib.reload_env()
    out = [[] for _ in range(cp['b'])]
    for vid, first, n, ov in plan:
        out[vid].append((first, n, ov))
    return out
