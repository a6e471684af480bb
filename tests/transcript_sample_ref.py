"""The transcript-graph posterior over ALIGNMENTS by enumeration (include/smmdp.h: smm_align_graph_sample_f64), sharing no
code with the kernels: an alignment is a start -> end path of the graph and the boundaries of its nodes' segments, so two paths
that spell the same class sequence are two alignments.  A graph is (a, pred, start, end) as in tests/align_graph_ref.py.

  enumerate_alignments   every (path, cuts) of a tiny video -> its score, each summed in fp64 from init, the elp of every
                         segment, len, trans and the closing term (the enumeration idea of transcript_graph_ref.brute_logz_graph).
  posterior              log Z_g and each alignment's probability from that map.
  alignment_of           a sample's (used nodes, span row) -> its (path, cuts) key, with every consistency check on the way.
  rescore                the score of a given (used nodes, span row), summed as above.
  expected_tv            E[total variation] of n draws of a PERFECT sampler from p (tests/test_gpu_sample.py's bound)."""
import itertools

import numpy as np

import align_graph_ref as AG


def _graph(graph):
    a, pred, start, end = graph
    return [int(v) for v in a], np.asarray(pred) != 0, np.asarray(start) != 0, np.asarray(end) != 0


def _score(elp, a, trans, init, len_scores, endpen, path, bounds):
    s = init[a[path[0]]] + (0.0 if endpen is None else endpen[a[path[-1]]])
    for i, m in enumerate(path):
        s += elp[bounds[i]:bounds[i + 1], a[m]].sum() + len_scores[bounds[i + 1] - bounds[i], a[m]]
        if i > 0:
            s += trans[a[m], a[path[i - 1]]]
    return float(s)


def enumerate_alignments(elp, graph, trans, init, len_scores, kp, endpen=None):
    """-> {(path, cuts): score}: path a tuple of nodes, cuts the tuple of the interior boundaries (segment i covers frames
    [b_i, b_{i+1}) with b = (0,) + cuts + (T,)); segments of 1 .. kp - 1 frames.  Alignments of score -inf are left out."""
    elp = np.asarray(elp, np.float64)
    T = elp.shape[0]
    a, pred, start, end = _graph(graph)
    out = {}
    for path in AG.paths(pred, start, end):
        S = len(path)
        if not 1 <= S <= T:
            continue
        for cuts in itertools.combinations(range(1, T), S - 1):
            b = (0,) + cuts + (T,)
            if any(b[i + 1] - b[i] > kp - 1 for i in range(S)):
                continue
            s = _score(elp, a, trans, init, len_scores, endpen, path, b)
            if s > -np.inf:
                out[(tuple(int(m) for m in path), tuple(int(c) for c in cuts))] = s
    return out


def posterior(aligns):
    """{key: score} -> (log Z_g, {key: probability}); (-inf, {}) for an empty map."""
    if not aligns:
        return -np.inf, {}
    keys = list(aligns)
    sc = np.array([aligns[k] for k in keys])
    mx = sc.max()
    w = np.exp(sc - mx)
    lz = float(mx + np.log(w.sum()))
    return lz, {k: float(np.exp(aligns[k] - lz)) for k in keys}


def alignment_of(graph, T, kp, used, span_row, eos=None):
    """A sample as the sampler hands it out -- ``used`` [M] 0/1 and ``span_row`` [>= T + 1] (the class at every segment start,
    -1 elsewhere, the EOS id at T) -- -> its (path, cuts) key.  AssertionError unless the used nodes form a start -> end path
    (their index order is the path's: the numbering is topological), as many of them as segments, each segment's class its
    node's, no segment longer than kp - 1, and nothing written behind position T."""
    a, pred, start, end = _graph(graph)
    path = tuple(int(m) for m in np.flatnonzero(np.asarray(used) != 0))
    row = np.asarray(span_row)
    starts = np.flatnonzero(row[:T] >= 0)
    assert len(path) >= 1 and len(path) == len(starts), (path, row)
    assert starts[0] == 0 and (row[T + 1:] == -1).all()
    if eos is not None:
        assert row[T] == eos, row
    b = tuple(int(s) for s in starts) + (T,)
    assert start[path[0]] and end[path[-1]], path
    for i, m in enumerate(path):
        assert row[b[i]] == a[m], (path, row)
        assert 1 <= b[i + 1] - b[i] <= kp - 1, (b, kp)
        if i > 0:
            assert pred[m, path[i - 1]], path
    return path, b[1:-1]


def rescore(elp, graph, trans, init, len_scores, kp, endpen, used, span_row):
    """-> ((path, cuts), score) of a given (used nodes, span row)."""
    elp = np.asarray(elp, np.float64)
    T = elp.shape[0]
    a = _graph(graph)[0]
    path, cuts = alignment_of(graph, T, kp, used, span_row)
    return (path, cuts), _score(elp, a, trans, init, len_scores, endpen, path, (0,) + cuts + (T,))


def labels_of(graph, T, key):
    """The frame labels [T] of an alignment."""
    a = _graph(graph)[0]
    path, cuts = key
    b = (0,) + tuple(cuts) + (T,)
    out = np.empty(T, np.int64)
    for i, m in enumerate(path):
        out[b[i]:b[i + 1]] = a[m]
    return out


def expected_tv(p, n):
    """0.5 sum sqrt(2 p (1 - p) / (pi n)): what n draws of a perfect sampler are expected to show."""
    p = np.asarray(list(p), np.float64)
    return float(0.5 * np.sum(np.sqrt(2 * p * (1 - p) / (np.pi * n))))
