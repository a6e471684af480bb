"""The entropy of the transcript-graph posterior over ALIGNMENTS (include/smmdp.h: smm_align_graph_entropy_f64) by routes that
share no code with the kernels.  A graph is (a, pred, start, end) as in tests/align_graph_ref.py; an alignment is a
start -> end path and the boundaries of its nodes' segments, so two paths that spell one class sequence are two alignments.

  enumeration_entropy   -sum p log p over transcript_sample_ref.enumerate_alignments / posterior.
  chain_rule            the header's H_end, H_span, H_pred in numpy over transcript_graph_ref.forward_backward (every cell).
  identity_entropy      log Z_g - E[score]: E[score] = <tables, fp64 gradients of log Z_g> + <p_end, endpen>.  Finite tables only
                        (0 * -inf otherwise).
  count_alignments      the number of alignments in Python integers: H = log N when every table is zero."""
import numpy as np

import transcript_graph_ref as TG
import transcript_sample_ref as TS


def entropy_of(p):
    """-sum p log p of a probability vector (zeros have no part)."""
    p = np.asarray(list(p), np.float64)
    p = p[p > 0]
    return float(-(p * np.log(p)).sum())


def enumeration_entropy(elp, graph, trans, init, len_scores, kp, endpen=None):
    """-> (H, log Z_g, number of alignments of finite score); (nan, -inf, 0) without one."""
    aligns = TS.enumerate_alignments(elp, graph, trans, init, len_scores, kp, endpen)
    lz, p = TS.posterior(aligns)
    if not p:
        return float('nan'), -np.inf, 0
    return entropy_of(p.values()), lz, len(p)


def hloc(w):
    """log Z - A / Z over the finite weights of a list, the largest as the reference; exactly 0 for a single one."""
    w = np.asarray(list(w), np.float64)
    w = w[np.isfinite(w)]
    assert w.size, "a decision without a candidate"
    x = w - w.max()
    e = np.exp(x)
    return float(np.log(e.sum()) - (e * x).sum() / e.sum())


def chain_rule(elp, graph, trans, init, len_scores, kp, endpen=None):
    """-> (H_end, H_span, H_pred) as the header defines them, every cell of the lattice; None when log Z_g = -inf.  A
    decision of posterior weight 0 is not evaluated."""
    fb = TG.forward_backward(elp, graph, trans, init, len_scores, kp, endpen)
    if not np.isfinite(fb['logz']):
        return None
    trans, len_scores = np.asarray(trans, np.float64), np.asarray(len_scores, np.float64)
    a, pred, start, end = TG._graph(graph)
    T, M = np.asarray(elp).shape[0], len(a)
    kw = min(kp - 1, T)
    h, gam, S, E = fb['h'], fb['gam'], fb['S'], fb['E']
    h_end = hloc(gam[T, j] + (0.0 if endpen is None else endpen[a[j]]) for j in range(M) if end[j])
    h_span = h_pred = 0.0
    for j in range(M):
        p = [i for i in range(j) if pred[j, i]]
        for n in range(1, T + 1):
            if E[n, j] > 0:
                h_span += E[n, j] * hloc(h[n - k, j] + len_scores[k, a[j]] for k in range(1, min(kw, n) + 1))
        for s in range(1, T):
            if p and S[s, j] > 0:
                h_pred += S[s, j] * hloc(gam[s, i] + trans[a[j], a[i]] for i in p)
    return h_end, h_span, h_pred


def identity_entropy(logz, g, elp, trans, init, len_scores, a=None, p_end=None, endpen=None):
    """log Z_g - E[score] from fp64 gradients g = dict(elp [T, C], trans, init, len) of log Z_g and, under end penalties, the
    end posteriors p_end [M] of the nodes of classes a."""
    score = sum(float((np.asarray(g[k], np.float64) * np.asarray(t, np.float64)).sum())
                for k, t in (('elp', elp), ('trans', trans), ('init', init), ('len', len_scores)))
    if endpen is not None:
        score += float(sum(p_end[j] * endpen[a[j]] for j in range(len(a)) if p_end[j] > 0))
    return float(logz - score)


def count_alignments(T, graph, kp):
    """The number of (path, boundaries) pairs of a video of T frames with segments of 1 .. kp - 1 frames, exactly."""
    a, pred, start, end = TG._graph(graph)
    M = len(a)
    kw = min(kp - 1, T)
    ch = [[0] * M for _ in range(T + 1)]                      # alignments of a prefix in front of a segment of m that starts at n
    cg = [[0] * M for _ in range(T + 1)]                      # ... of a prefix whose last segment, of node m, ends at n
    for m in range(M):
        ch[0][m] = 1 if start[m] else 0
        for n in range(1, T + 1):
            if n < T:
                ch[n][m] = sum(cg[n][j] for j in range(m) if pred[m, j])
            cg[n][m] = sum(ch[n - k][m] for k in range(1, min(kw, n) + 1))
    return sum(cg[T][j] for j in range(M) if end[j])
