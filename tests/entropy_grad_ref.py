"""fp64 references of the gradients of H(p), H(p, q) and KL(p || q) with respect to the factor tables, by enumeration: every
segmentation of a small factored lattice is listed with its occurrence counts phi(y) (spans, their frames and lengths,
transitions, the initial class; without EOS the closing label), its score is phi(y) . theta plus the EOS closing constant, and
torch autograd differentiates -sum p log p, -sum p log q and sum p (log p - log q).  Independent of the kernels and of the C
twin: only the lattice's definition (include/smmdp.h, csrc/smm_logz.hip) is shared."""
import numpy as np
import torch

BIG_NEG = -1e9


def segmentations(positions, c, kp, no_eos):
    """Every segmentation of `positions` DP positions: (spans [(start, length, class)], closing label or None)."""
    out = []

    def rec(n, spans):
        if n == positions:
            for to in (range(c) if no_eos else [None]):
                out.append((list(spans), to))
            return
        for k in range(1, kp):
            if n + k > positions:
                break
            for cl in range(c):
                spans.append((n, k, cl))
                rec(n + k, spans)
                spans.pop()

    rec(0, [])
    return out


def occurrences(frames, c, k_rows, kp, no_eos):
    """phi [paths, frames*c + c*c + c + k_rows*c] (elp | trans [to][from] | init | len) and each path's last span class."""
    positions = frames - (1 if no_eos else 0)
    o_tr, o_in, o_len = frames * c, frames * c + c * c, frames * c + c * c + c
    paths = segmentations(positions, c, kp, no_eos)
    phi = np.zeros((len(paths), o_len + k_rows * c))
    last = np.zeros(len(paths), np.int64)
    for i, (spans, to) in enumerate(paths):
        row = phi[i]
        row[o_in + spans[0][2]] += 1
        prev = None
        for s, k, cl in spans:
            row[o_len + k * c + cl] += 1
            for t in range(s, s + k):
                row[t * c + cl] += 1
            if prev is not None:
                row[o_tr + cl * c + prev] += 1
            prev = cl
        if to is not None:
            row[o_tr + to * c + prev] += 1
            row[positions * c + to] += 1
        last[i] = prev
    return torch.from_numpy(phi), torch.from_numpy(last)


def _flat(t):
    return torch.cat([t['elp'].reshape(-1), t['trans'].reshape(-1), t['init'].reshape(-1), t['len'].reshape(-1)])


def _unflat(g, frames, c, k_rows):
    o = [frames * c, c * c, c, k_rows * c]
    e, tr, ini, ln = torch.split(g, o)
    return dict(elp=e.view(frames, c), trans=tr.view(c, c), init=ini, len=ln.view(k_rows, c))


def _wend(trans, endpen):
    """EOS closing weight of each last class (a constant of the tables: the kernels' convention)."""
    alt = torch.logsumexp(trans.detach(), dim=0)
    ep = torch.zeros_like(alt) if endpen is None else torch.as_tensor(endpen, dtype=torch.float64)
    return torch.logaddexp(ep, alt + BIG_NEG)


def video_reference(tp, tq, kp, no_eos, endpen_p=None, endpen_q=None):
    """One video: tp / tq dicts of fp64 CPU tensors elp [frames, c], trans [c, c], init [c], len [k_rows, c].
    -> {mode: (value, grads of p's tables, grads of q's tables)} for mode in entropy, cross_entropy, kl."""
    frames, c = tp['elp'].shape
    k_rows = tp['len'].shape[0]
    phi, last = occurrences(frames, c, k_rows, kp, no_eos)
    thp = _flat(tp).clone().requires_grad_(True)
    thq = _flat(tq).clone().requires_grad_(True)
    sp, sq = phi @ thp, phi @ thq
    if not no_eos:
        sp = sp + _wend(tp['trans'], endpen_p)[last]
        sq = sq + _wend(tq['trans'], endpen_q)[last]
    lp, lq = torch.log_softmax(sp, 0), torch.log_softmax(sq, 0)
    p = lp.exp()
    vals = dict(entropy=-(p * lp).sum(), cross_entropy=-(p * lq).sum(), kl=(p * (lp - lq)).sum())
    out = {}
    for name, v in vals.items():
        gp, gq = torch.autograd.grad(v, (thp, thq), retain_graph=True, allow_unused=True)
        gq = torch.zeros_like(thq) if gq is None else gq
        out[name] = (float(v.detach()), _unflat(gp.detach(), frames, c, k_rows), _unflat(gq.detach(), frames, c, k_rows))
    return out


def batch_reference(elp_bt, lengths, trans, init, lens, kp, no_eos, endpen, q, mode, up):
    """Sum over the videos of a padded single-group batch of up[i] x the gradient of video i, in the layouts of the kernels:
    (values [b], p's grads dict(elp [b*tmax, c], trans, init, len), q's grads alike).  q = (elp_bt, lengths, trans, init, lens,
    endpen), the layout of p's arguments."""
    b, tmax, c = elp_bt.shape
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    gp = dict(elp=torch.zeros(b * tmax, c, dtype=torch.float64), trans=torch.zeros(c, c, dtype=torch.float64),
              init=torch.zeros(c, dtype=torch.float64), len=torch.zeros(lens.shape, dtype=torch.float64))
    gq = {k: v.clone() for k, v in gp.items()}
    vals = []
    for i, fr in enumerate(lengths):
        tp = dict(elp=t(elp_bt[i, :fr]), trans=t(trans), init=t(init), len=t(lens))
        tq = dict(elp=t(q[0][i, :fr]), trans=t(q[2]), init=t(q[3]), len=t(q[4]))
        r = video_reference(tp, tq, kp, no_eos, None if endpen is None else endpen[i], None if q[5] is None else q[5][i])
        v, a, bq = r[mode]
        vals.append(v)
        for g, src in ((gp, a), (gq, bq)):
            g['elp'][i * tmax:i * tmax + fr] += up[i] * src['elp']
            for k in ('trans', 'init', 'len'):
                g[k] += up[i] * src[k]
    return np.array(vals), gp, gq
