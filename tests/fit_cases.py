"""Host-side inputs of the fit-statistics tests that cross the work splits of csrc/smm_fit.hip (numpy only; no GPU), and a
numpy restatement of smm_span_stats_kernel's chunked rule with the carry as a parameter.  Every seed is fixed.

The restatement serves ONE purpose (test_fit_cases_host.py): to show that the run lists below make the carry into a chunk
observable -- that a kernel which handed a wrong run start across a chunk boundary would count other spans than
oracle.dense_ref.sufficient_stats.  What the GPU test expects is the oracle's answer, never the restatement's."""
import functools

import numpy as np

CHUNK = 2048                     # SMM_FIT_CHUNK: frames per work item of both kernels
SCAN = 256                       # labels per trip of the backward scan for the run open at a chunk's first frame
N_CLASSES = 5
D = 4
MAX_KS = (None, 2, 20, 64, 1025)         # None and 2: no cut / a cut at every frame -- the carry cannot matter (control)
CARRY_MAX_KS = (20, 64, 1025)            # the settings at which a wrong carry must show
WRONG_CARRIES = ('zero', 'last')         # s_carry left at 0;  c_begin - 1 (the hit taken for granted in the first lane)

# (label, run length) lists.  Positions are frames of the video; chunk boundaries lie at 2048 and 4096.
CARRY_RUNS = {
    # a run opens at 1700, 348 frames before 2048 (second trip of the scan); a label change falls exactly at 4096
    'straddle': ((0, 1700), (1, 700), (3, 1696), (0, 300)),
    # no change anywhere: chunk 1 is entered and left inside one run, and both scans end at p == 0
    'whole': ((2, 2 * CHUNK + 5),),
    # the open run starts at c_begin - 1 = 2047: found by the first lane of the first trip
    'tid0': ((1, 2047), (0, 10), (3, 1783), (1, 600)),
    # the open run starts 256 frames before 2048 (first frame of the second trip) and 257 before 4096 (its second frame)
    'trip_edge': ((0, 1792), (1, 300), (3, 1747), (0, 400)),
}
CARRY_NAMES = tuple(CARRY_RUNS)


def labels_of(runs):
    return np.concatenate([np.full(n, c, dtype=np.int64) for c, n in runs])


def features_of(rng, labels, d):
    return (rng.normal(size=(len(labels), d)) + labels[:, None] * 0.1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def carry_batch():
    """The four videos of CARRY_RUNS in one batch: (features, labels), lists in CARRY_NAMES' order."""
    rng = np.random.default_rng(4396)
    labels = [labels_of(CARRY_RUNS[name]) for name in CARRY_NAMES]
    return [features_of(rng, y, D) for y in labels], labels


def run_start_before(y, c_begin):
    """Start of the run that contains frame c_begin - 1: the largest p < c_begin with p == 0 or y[p] != y[p - 1]."""
    p = c_begin - 1
    while p > 0 and y[p] == y[p - 1]:
        p -= 1
    return p


def chunked_span_stats(label_list, n_classes, max_k, carry='true'):
    """smm_span_stats_kernel restated: every video in chunks of CHUNK frames, the start of the run containing frame t is
    max(carry, last label change inside the chunk at or before t), a span starts at a change or where
    (t - run start) % (max_k - 1) == 0.  ``carry``: 'true' (run_start_before), 'zero' or 'last' (c_begin - 1).
    Returns the oracle's four integer statistics (float32 like the oracle's)."""
    spans = np.zeros(n_classes, np.float32)
    frames = np.zeros(n_classes, np.float32)
    starts = np.zeros(n_classes, np.float32)
    trans = np.zeros((n_classes, n_classes), np.float32)
    do_cut = max_k is not None and max_k > 0
    cut = max_k - 1 if do_cut and max_k > 1 else 1
    for y in label_list:
        y = np.asarray(y)
        for c_begin in range(0, len(y), CHUNK):
            c_end = min(len(y), c_begin + CHUNK)
            if c_begin == 0:
                cr = 0
            else:
                cr = {'true': run_start_before(y, c_begin), 'zero': 0, 'last': c_begin - 1}[carry]
            t = np.arange(c_begin, c_end)
            before = np.where(t > 0, y[np.maximum(t - 1, 0)], -1)
            change = (t == 0) | (y[t] != before)
            rs = np.maximum(np.maximum.accumulate(np.where(change, t, -1)), cr)
            start = change | ((t - rs) % cut == 0 if do_cut else False)
            np.add.at(frames, y[t], 1)
            np.add.at(spans, y[t][start], 1)
            first = start & (t == 0)
            np.add.at(starts, y[t][first], 1)
            later = start & (t > 0)
            np.add.at(trans, (y[t][later], before[later]), 1)
    return dict(span_counts=spans, span_lengths=frames, span_start_counts=starts, span_transition_counts=trans)


INT_KEYS = ('span_counts', 'span_lengths', 'span_start_counts', 'span_transition_counts')


def same_counts(a, b):
    return all(np.array_equal(a[k], b[k]) for k in INT_KEYS)


# ---------------------------------------------------------------------------------------------------- many work items
MANY_CLASSES = 9
MANY_ABSENT = 2                   # a class without a frame
MANY_MAX_K = 20
MANY_LONG = {0: 2500, 333: 2048, 666: 2049, 999: 513}


@functools.lru_cache(maxsize=None)
def many_items_labels():
    """1000 videos: T uniform in 1..30 but for four long ones at MANY_LONG's positions; label runs of Poisson(11) frames.
    1002 chunks = 4008 quarter-chunk work items for smm_class_sums_kernel's 768 workgroups: five to six items each, and three
    of the four items of every short video lie past its end (the `continue` in front of a live item)."""
    rng = np.random.default_rng(1000)
    classes = [c for c in range(MANY_CLASSES) if c != MANY_ABSENT]
    out = []
    for i in range(1000):
        t = MANY_LONG.get(i, int(rng.integers(1, 31)))
        y = []
        while len(y) < t:
            y += [int(rng.choice(classes))] * int(max(1, rng.poisson(11)))
        out.append(np.asarray(y[:t], dtype=np.int64))
    return out


def many_items_features(d):
    rng = np.random.default_rng(2000 + d)
    return [features_of(rng, y, d) for y in many_items_labels()]
