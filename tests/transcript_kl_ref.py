"""KL(p || q) and the cross-entropy H(p, q) between two transcript-graph posteriors over ALIGNMENTS (include/smmdp.h:
smm_align_graph_kl_f64) by routes that share no code with the kernels.  A graph is (a, pred, start, end) as in
tests/align_graph_ref.py; a side is (elp, trans, init, len_scores, endpen or None); both sides share graph, T and kp.

  enumeration_kl   sum p log(p / q) over transcript_sample_ref.enumerate_alignments of both sides.
  chain_rule_kl    the header's KL_end, KL_span, KL_pred (and the same sums of Hloc_p + KLloc) in numpy over
                   transcript_graph_ref.forward_backward of both sides, every cell.
  identity_kl      log Z_q - log Z_p + <mu_p, theta_p - theta_q> (+ <p_end, endpen_p - endpen_q>) from fp64 gradients of p's
                   log Z_g and both log Z_g.  Finite tables only (0 * -inf otherwise)."""
import numpy as np

import transcript_graph_ref as TG
import transcript_sample_ref as TS


def kl_of(p, q):
    """sum p log(p / q) of two probability vectors over the same support order (zeros of p have no part; +inf where q is 0
    and p is not)."""
    p, q = np.asarray(list(p), np.float64), np.asarray(list(q), np.float64)
    on = p > 0
    if (q[on] <= 0).any():
        return float('inf')
    return float((p[on] * (np.log(p[on]) - np.log(q[on]))).sum())


def enumeration_kl(p, q, graph, kp):
    """-> (KL, H(p, q), log Z_p, log Z_q, number of p's alignments); (nan, nan, -inf, ., 0) when p has none."""
    ap = TS.enumerate_alignments(p[0], graph, p[1], p[2], p[3], kp, p[4])
    aq = TS.enumerate_alignments(q[0], graph, q[1], q[2], q[3], kp, q[4])
    lzp, pp = TS.posterior(ap)
    lzq, _ = TS.posterior(aq)
    if not pp:
        return float('nan'), float('nan'), lzp, lzq, 0
    kl = xe = 0.0
    for key, pr in pp.items():
        if pr <= 0:
            continue
        if key not in aq:
            return float('inf'), float('inf'), lzp, lzq, len(pp)
        lq = aq[key] - lzq
        kl += pr * ((ap[key] - lzp) - lq)
        xe -= pr * lq
    return float(kl), float(xe), lzp, lzq, len(pp)


def loc(wp, wq):
    """(KLloc, Hloc_p) of one decision from the candidates' weights on both sides, as the header defines them."""
    wp, wq = np.asarray(list(wp), np.float64), np.asarray(list(wq), np.float64)
    assert wp.size and np.isfinite(wp).any(), "a decision without a candidate under p"
    mp = wp[np.isfinite(wp)].max()
    mq = wq[np.isfinite(wq)].max() if np.isfinite(wq).any() else 0.0
    with np.errstate(invalid='ignore'):
        ep, eq = np.exp(wp - mp), np.exp(wq - mq)
    on = ep > 0
    sp, sq = ep.sum(), eq.sum()
    hl = float(np.log(sp) - (ep[on] * (wp[on] - mp)).sum() / sp)
    if np.isneginf(wq[on]).any():
        return float('inf'), hl
    y = (ep[on] * (wq[on] - wp[on])).sum()
    return max(0.0, float((mq - mp) + np.log(sq) - np.log(sp) - y / sp)), hl


def chain_rule_kl(p, q, graph, kp):
    """-> ((KL_end, KL_span, KL_pred), (X_end, X_span, X_pred)): the parts of KL(p || q) and of H(p, q), every cell of the
    lattice; None when p's log Z_g = -inf; all +inf when q's is and p's is not.  A decision of weight 0 under p is not
    evaluated."""
    fp = TG.forward_backward(p[0], graph, p[1], p[2], p[3], kp, p[4])
    if not np.isfinite(fp['logz']):
        return None
    fq = TG.forward_backward(q[0], graph, q[1], q[2], q[3], kp, q[4])
    if not np.isfinite(fq['logz']):
        return (float('inf'),) * 3, (float('inf'),) * 3
    tp, lp, tq, lq = (np.asarray(x, np.float64) for x in (p[1], p[3], q[1], q[3]))
    a, pred, start, end = TG._graph(graph)
    T, M = np.asarray(p[0]).shape[0], len(a)
    kw = min(kp - 1, T)
    cp = lambda c: 0.0 if p[4] is None else p[4][c]
    cq = lambda c: 0.0 if q[4] is None else q[4][c]
    ends = [j for j in range(M) if end[j]]
    k_end, h_end = loc([fp['gam'][T, j] + cp(a[j]) for j in ends], [fq['gam'][T, j] + cq(a[j]) for j in ends])
    kl, xe = [k_end, 0.0, 0.0], [h_end + k_end, 0.0, 0.0]
    for j in range(M):
        pj = [i for i in range(j) if pred[j, i]]
        for n in range(1, T + 1):
            if fp['E'][n, j] > 0:
                ks = range(1, min(kw, n) + 1)
                k, h = loc([fp['h'][n - d, j] + lp[d, a[j]] for d in ks], [fq['h'][n - d, j] + lq[d, a[j]] for d in ks])
                kl[1] += fp['E'][n, j] * k
                xe[1] += fp['E'][n, j] * (h + k)
        for s in range(1, T):
            if pj and fp['S'][s, j] > 0:
                k, h = loc([fp['gam'][s, i] + tp[a[j], a[i]] for i in pj], [fq['gam'][s, i] + tq[a[j], a[i]] for i in pj])
                kl[2] += fp['S'][s, j] * k
                xe[2] += fp['S'][s, j] * (h + k)
    return tuple(kl), tuple(xe)


def identity_kl(logz_p, logz_q, g, p, q, a=None, p_end=None):
    """log Z_q - log Z_p + <mu_p, theta_p - theta_q> from fp64 gradients g = dict(elp [T, C], trans, init, len) of p's log Z_g
    and, under end penalties, p's end posteriors p_end [M] of the nodes of classes a."""
    dot = sum(float((np.asarray(g[k], np.float64) * (np.asarray(tp, np.float64) - np.asarray(tq, np.float64))).sum())
              for k, tp, tq in (('elp', p[0], q[0]), ('trans', p[1], q[1]), ('init', p[2], q[2]), ('len', p[3], q[3])))
    if p[4] is not None or q[4] is not None:
        zero = np.zeros(np.asarray(p[2]).shape[0])
        ep, eq = (zero if p[4] is None else p[4]), (zero if q[4] is None else q[4])
        dot += float(sum(p_end[j] * (ep[a[j]] - eq[a[j]]) for j in range(len(a)) if p_end[j] > 0))
    return float(logz_q - logz_p + dot)
