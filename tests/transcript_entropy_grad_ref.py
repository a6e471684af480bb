"""Gradients of the entropy H(p), the cross-entropy H(p, q) and KL(p || q) of transcript-graph posteriors over ALIGNMENTS with
respect to the tables (include/smmdp.h: smm_align_graph_entropy_bwd_f64, smm_align_graph_kl_bwd_f64), by three routes that share
no code with the kernels.  A graph is (a, pred, start, end) as in tests/align_graph_ref.py; a side is (elp, trans, init,
len_scores, endpen or None) in numpy; both sides share graph, T and kp.  ``mode``: 'entropy' (q is ignored), 'xent' or 'kl'.

  enumeration_grads  (a) torch fp64 autograd through the value summed over transcript_sample_ref.enumerate_alignments: robust to
                     -1e9 entries, alignments of score -inf are left out.  Gradients for both sides.
  identity_grads     (b) transcript_graph_ref.torch_logz_graph differentiated twice: H = logZ_p - <mu_p, theta_p> - <p_end, endpen_p>,
                     H(p, q) = logZ_q - <mu_p, theta_q> - <p_end, endpen_q>.  Finite tables and masks at -1e4 only: at -1e9 the
                     identity subtracts terms of 1e9 and is wrong by tens of nats.
  formula_grads      (c) the header's formulas in numpy over transcript_graph_ref.forward_backward of both sides, every cell:
                     eta-, eta+, V-, V+ and the four gradients -- the executable statement of what the kernels compute."""
import numpy as np
import torch

import transcript_graph_ref as TG
import transcript_sample_ref as TS

MODES = ('entropy', 'xent', 'kl')
KEYS = ('elp', 'trans', 'init', 'len')


def _torch_side(side):
    t = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in side[:4]]
    ep = None if side[4] is None else torch.tensor(np.asarray(side[4], np.float64))
    return t, ep


def _grads(t):
    return {k: (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.numpy().copy()) for k, v in zip(KEYS, t)}


def _scores(keys, T, a, t, ep):
    elp, trans, init, len_scores = t
    cum = torch.cat([torch.zeros((1, elp.shape[1]), dtype=torch.float64), torch.cumsum(elp, dim=0)])
    out = []
    for path, cuts in keys:
        b = (0,) + cuts + (T,)
        s = init[a[path[0]]] + (0.0 if ep is None else ep[a[path[-1]]])
        for i, m in enumerate(path):
            s = s + (cum[b[i + 1], a[m]] - cum[b[i], a[m]]) + len_scores[b[i + 1] - b[i], a[m]]
            if i > 0:
                s = s + trans[a[m], a[path[i - 1]]]
        out.append(s)
    return torch.stack(out)


def enumeration_grads(p, q, graph, kp, mode):
    """-> (V, p's gradients dict(elp, trans, init, len), q's gradients or None); (nan, zeros, None) when p has no alignment,
    (inf, None, None) when q excludes an alignment that has mass under p."""
    assert mode in MODES
    a = TG._graph(graph)[0]
    T = np.asarray(p[0]).shape[0]
    ap = TS.enumerate_alignments(p[0], graph, p[1], p[2], p[3], kp, p[4])
    if not ap:
        return float('nan'), {k: np.zeros(np.asarray(v).shape) for k, v in zip(KEYS, p[:4])}, None
    keys = list(ap)
    tp, epp = _torch_side(p)
    lp = torch.log_softmax(_scores(keys, T, a, tp, epp), dim=0)
    pr = torch.exp(lp)
    if mode == 'entropy':
        v = -(pr * lp).sum()
        v.backward()
        return float(v.detach()), _grads(tp), None
    aq = TS.enumerate_alignments(q[0], graph, q[1], q[2], q[3], kp, q[4])
    if any(k not in aq for k, x in zip(keys, pr.detach().numpy()) if x > 0):
        return float('inf'), None, None
    tq, epq = _torch_side(q)
    qkeys = list(aq)
    lzq = torch.logsumexp(_scores(qkeys, T, a, tq, epq), dim=0)
    on = [i for i, k in enumerate(keys) if k in aq]
    lq = _scores([keys[i] for i in on], T, a, tq, epq) - lzq
    v = -(pr[on] * lq).sum() if mode == 'xent' else (pr[on] * (lp[on] - lq)).sum()
    v.backward()
    return float(v.detach()), _grads(tp), _grads(tq)


def identity_grads(p, q, graph, kp, mode):
    """-> (V, p's gradients): the value as log Z_g differentiated once, its gradient by differentiating again."""
    assert mode in MODES
    C = np.asarray(p[0]).shape[1]

    def side(s):
        t = [torch.tensor(np.asarray(v, np.float64), requires_grad=True) for v in s[:4]]
        ep = torch.tensor(np.zeros(C) if s[4] is None else np.asarray(s[4], np.float64), requires_grad=True)
        return t + [ep]

    tp = side(p)
    zp = TG.torch_logz_graph(tp[0], graph, tp[1], tp[2], tp[3], kp, tp[4])
    mu = torch.autograd.grad(zp, tp, create_graph=True, allow_unused=True)
    mu = [torch.zeros_like(t) if m is None else m for m, t in zip(mu, tp)]
    h_p = zp - sum((m * t).sum() for m, t in zip(mu, tp))
    if mode == 'entropy':
        v = h_p
    else:
        tq = [torch.tensor(np.zeros(C) if x is None else np.asarray(x, np.float64)) for x in q]
        zq = TG.torch_logz_graph(tq[0], graph, tq[1], tq[2], tq[3], kp, tq[4])
        x_pq = zq - sum((m * t).sum() for m, t in zip(mu, tq))
        v = x_pq if mode == 'xent' else x_pq - h_p
    g = torch.autograd.grad(v, tp[:4], allow_unused=True)
    return float(v.detach()), {k: (np.zeros(tuple(t.shape)) if x is None else x.numpy()) for k, x, t in zip(KEYS, g, tp)}


def _decide(wp, wq, eta, kl):
    """sum_c p_loc(c) [ L(c) + eta(c) ] of one decision; 0 without mass under p; +inf where q excludes what p has."""
    wp, wq, eta = (np.asarray(x, np.float64) for x in (wp, wq, eta))
    if not wp.size or not np.isfinite(wp).any():
        return 0.0
    lp = wp - TG._lse(wp)
    on = np.exp(lp) > 0
    if np.isneginf(wq[on]).any():
        return float('inf')
    lq = wq[on] - TG._lse(wq)
    loc = (np.exp(lp[on]) * ((lp[on] - lq) if kl else -lq)).sum()
    return max(0.0, float(loc)) + float((np.exp(lp[on]) * eta[on]).sum())


def formula_grads(p, q, graph, kp, mode):
    """-> dict(value (V-), value_plus (V+), elp, trans, init, len, eta_ms, eta_me, eta_pe, eta_ps (each [T + 1, M])); None
    when p has no alignment; dict(value=inf) when q has none or excludes what p has."""
    assert mode in MODES
    if mode == 'entropy':
        q = p
    kl = mode == 'kl'
    fp = TG.forward_backward(p[0], graph, p[1], p[2], p[3], kp, p[4])
    if not np.isfinite(fp['logz']):
        return None
    fq = TG.forward_backward(q[0], graph, q[1], q[2], q[3], kp, q[4])
    if not np.isfinite(fq['logz']):
        return dict(value=float('inf'))
    a, pred, start, end = TG._graph(graph)
    T, C = np.asarray(p[0]).shape
    M = len(a)
    kw = min(kp - 1, T)
    tabs = []
    for s in (p, q):
        elp, trans, init, ln = (np.asarray(x, np.float64) for x in s[:4])
        cum = np.concatenate([np.zeros((1, C)), np.cumsum(elp, axis=0)])
        tabs.append((cum, trans, init, ln, np.zeros(C) if s[4] is None else np.asarray(s[4], np.float64)))
    (cp, trp, inp, lnp, cep), (cq, trq, inq, lnq, ceq) = tabs
    preds = [[i for i in range(j) if pred[j, i]] for j in range(M)]
    succs = [[m for m in range(j + 1, M) if pred[m, j]] for j in range(M)]
    hp, gp, bhp, bgp, hq, gq, bhq, bgq = (f[k] for f in (fp, fq) for k in ('h', 'gam', 'bh', 'bg'))

    ems, eme = np.zeros((T + 1, M)), np.zeros((T + 1, M))
    for j in range(M):
        for s in range(1, T):
            ems[s, j] = _decide([gp[s, i] + trp[a[j], a[i]] for i in preds[j]], [gq[s, i] + trq[a[j], a[i]] for i in preds[j]],
                                [eme[s, i] for i in preds[j]], kl)
        for n in range(1, T + 1):
            ks = range(1, min(kw, n) + 1)
            eme[n, j] = _decide([hp[n - k, j] + lnp[k, a[j]] for k in ks], [hq[n - k, j] + lnq[k, a[j]] for k in ks],
                                [ems[n - k, j] for k in ks], kl)
    ends = [j for j in range(M) if end[j]]
    v_minus = _decide([gp[T, j] + cep[a[j]] for j in ends], [gq[T, j] + ceq[a[j]] for j in ends], [eme[T, j] for j in ends], kl)
    if not np.isfinite(v_minus):
        return dict(value=float('inf'))

    epe, eps = np.zeros((T + 1, M)), np.zeros((T + 1, M))
    for j in range(M - 1, -1, -1):
        for n in range(1, T):
            epe[n, j] = _decide([trp[a[m], a[j]] - cp[n, a[m]] + bhp[n, m] for m in succs[j]],
                                [trq[a[m], a[j]] - cq[n, a[m]] + bhq[n, m] for m in succs[j]], [eps[n, m] for m in succs[j]], kl)
        for s in range(T):
            ks = range(1, min(kw, T - s) + 1)
            eps[s, j] = _decide([lnp[k, a[j]] + cp[s + k, a[j]] + bgp[s + k, j] for k in ks],
                                [lnq[k, a[j]] + cq[s + k, a[j]] + bgq[s + k, j] for k in ks], [epe[s + k, j] for k in ks], kl)
    starts = [m for m in range(M) if start[m]]
    v_plus = _decide([inp[a[m]] + bhp[0, m] for m in starts], [inq[a[m]] + bhq[0, m] for m in starts], [eps[0, m] for m in starts], kl)

    lzp, lzq = fp['logz'], fq['logz']

    def term(wp, wq, eta):
        lp = wp - lzp
        po = np.exp(lp)
        if not po > 0:
            return 0.0
        lq = wq - lzq
        return po * (eta + ((lp - lq) if kl else -lq) - v_minus)

    g = dict(elp=np.zeros((T, C)), trans=np.zeros((C, C)), init=np.zeros(C), len=np.zeros(np.asarray(p[3]).shape))
    for j in range(M):
        c = a[j]
        for s in range(T):
            for k in range(1, min(kw, T - s) + 1):
                n = s + k
                x = term(hp[s, j] + lnp[k, c] + cp[n, c] + bgp[n, j], hq[s, j] + lnq[k, c] + cq[n, c] + bgq[n, j],
                         ems[s, j] + epe[n, j])
                g['elp'][s:n, c] += x
                g['len'][k, c] += x
        for i in preds[j]:
            for s in range(1, T):
                g['trans'][c, a[i]] += term(gp[s, i] + trp[c, a[i]] - cp[s, c] + bhp[s, j], gq[s, i] + trq[c, a[i]] - cq[s, c] + bhq[s, j],
                                            eme[s, i] + eps[s, j])
        if start[j]:
            g['init'][c] += term(inp[c] + bhp[0, j], inq[c] + bhq[0, j], eps[0, j])
    return dict(g, value=v_minus, value_plus=v_plus, eta_ms=ems, eta_me=eme, eta_pe=epe, eta_ps=eps)


def mu_grads(side, graph, kp):
    """The posterior marginals mu of one side as gradients of its log Z_g (transcript_graph_ref.torch_grads_graph): q's gradient
    of H(p, q) and of KL(p || q) is mu_q - mu_p."""
    return TG.torch_grads_graph(side[0], graph, side[1], side[2], side[3], kp, side[4])[1]
