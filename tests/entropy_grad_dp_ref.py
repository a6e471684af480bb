"""fp64 references of the gradients of H(p), H(p, q) and KL(p || q) with respect to the factor tables in polynomial time, for
lattices too large to enumerate.  The conventions are those of tests/entropy_grad_ref.py (table layouts, kp, no_eos, the
closing label without EOS, the EOS closing weight `_wend` as a constant of the tables); nothing is shared with the kernels or
with the C twin.

log Z is a plain torch forward recursion over the positions,
    alpha[n][c] = LSE_{k = 1 .. min(kp - 1, n)} ( h[n - k][c] + len[k][c] + sum of elp[n - k .. n - 1][c] ),   h[0] = init,
    h[n][c]     = LSE_c' ( alpha[n][c'] + trans[c][c'] ),
closed by LSE_c(alpha[P][c] + w[c]) with EOS (w a leaf that holds _wend(trans, endpen): no gradient reaches trans through it,
and d log Z / d w[c] = P(last = c)) and by LSE_{to, c}(alpha[P][c] + trans[to][c] + elp[P][to]) without.  With mu_p = d log Z_p /
d (theta_p, w_p) kept differentiable, E_p[s_r] = mu_p . theta_r + mu_w . w_r, and
    H(p) = log Z_p - E_p[s_p],     H(p, q) = log Z_q - E_p[s_q],     KL = H(p, q) - H(p);
a second autograd pass differentiates them with respect to both sides' tables.

Two traps, each worth ~1e-7 when ignored:
  * Prefix sums across -1e9 entries.  A span's emission sum taken as cum[n] - cum[n - k] loses ulp(1e9) ~ 1.2e-7 once a -1e9
    entry lies anywhere in front of the span.  Two prefix sums are kept instead -- one over the entries above -1e8 (the others
    replaced by 0), one over the entries at or below -1e8 (the others replaced by 0) -- and their differences are added.
  * Masked potentials in mu . theta.  The exact marginal of a potential at or below -1e8 is exp(-1e9) = 0, but autograd leaves a
    rounding residue of ~1e-16 there, which the mask would multiply by 1e9: such potentials are left out of the sum."""
import numpy as np
import torch

from entropy_grad_ref import BIG_NEG, _wend

MASKED = BIG_NEG / 10                       # potentials at or below this are masks
NAMES = ('elp', 'trans', 'init', 'len')
MODES = ('entropy', 'cross_entropy', 'kl')
F64 = torch.float64


def _leaves(t):
    return {k: torch.as_tensor(np.asarray(t[k]), dtype=F64).clone().requires_grad_(True) for k in NAMES}


def _logz(th, w, kp, no_eos):
    """log Z of one video from differentiable tables th (elp [frames, c], trans, init, len) and the closing leaf w (EOS)."""
    elp, trans, init, lens = (th[k] for k in NAMES)
    frames, c = elp.shape
    pos = frames - (1 if no_eos else 0)
    body = elp[:pos]
    free = body > MASKED
    zero = torch.zeros_like(body)
    head = torch.zeros(1, c, dtype=F64)
    cum_free = torch.cat([head, torch.cumsum(torch.where(free, body, zero), 0)])
    cum_mask = torch.cat([head, torch.cumsum(torch.where(free, zero, body), 0)])
    h = [init]
    alpha = None
    for n in range(1, pos + 1):
        m = min(kp - 1, n)
        # rows j = n - m .. n - 1 are the span starts: lengths k = n - j = m .. 1
        span = (cum_free[n] - cum_free[n - m:n]) + (cum_mask[n] - cum_mask[n - m:n])
        alpha = torch.logsumexp(torch.stack(h[n - m:n]) + lens[1:m + 1].flip(0) + span, 0)
        if n < pos:
            h.append(torch.logsumexp(alpha.unsqueeze(0) + trans, 1))
    if no_eos:
        return torch.logsumexp((alpha.unsqueeze(0) + trans + elp[pos].unsqueeze(1)).reshape(-1), 0)
    return torch.logsumexp(alpha + w, 0)


def _dot(mu, theta):
    """sum of mu x theta over the potentials that are no masks."""
    t = theta.detach()
    return (mu * torch.where(t > MASKED, theta, torch.zeros_like(theta))).sum()


def _side(t, kp, no_eos, endpen):
    """Leaves of one side, its log Z and its differentiable marginals: (leaves + [w], log Z, mu)."""
    th = _leaves(t)
    w = None
    if not no_eos:
        w = _wend(th['trans'], endpen).detach().clone().requires_grad_(True)
    lz = _logz(th, w, kp, no_eos)
    wrt = [th[k] for k in NAMES] + ([] if w is None else [w])
    mu = torch.autograd.grad(lz, wrt, create_graph=True, allow_unused=True)        # (one position: no transition is read)
    mu = tuple(torch.zeros_like(x) if m is None else m for x, m in zip(wrt, mu))
    return wrt, lz, mu


def logz(t, kp, no_eos, endpen=None):
    """log Z of one video (t: dict of elp [frames, c], trans, init, len)."""
    return float(_side(t, kp, no_eos, endpen)[1].detach())


def length_marginals(t, kp, no_eos, endpen=None):
    """Expected number of spans of each (length, class) of one video under its posterior: d log Z / d len, [k_rows, c]."""
    wrt, _, mu = _side(t, kp, no_eos, endpen)
    return mu[3].detach()


def video_reference(tp, tq, kp, no_eos, endpen_p=None, endpen_q=None):
    """One video: tp / tq dicts of fp64 CPU arrays elp [frames, c], trans [c, c], init [c], len [k_rows, c].
    -> {mode: (value, grads of p's tables, grads of q's tables)} for mode in entropy, cross_entropy, kl."""
    lp, zp, mp = _side(tp, kp, no_eos, endpen_p)
    lq, zq, _ = _side(tq, kp, no_eos, endpen_q)
    ent = zp - sum(_dot(m, x) for m, x in zip(mp, lp))
    xent = zq - sum(_dot(m, x) for m, x in zip(mp, lq))
    vals = dict(entropy=ent, cross_entropy=xent, kl=xent - ent)
    leaves, grads = lp[:4] + lq[:4], {}
    for mode in ('entropy', 'cross_entropy'):
        g = torch.autograd.grad(vals[mode], leaves, retain_graph=True, allow_unused=True)
        grads[mode] = [torch.zeros_like(x) if gg is None else gg.detach() for x, gg in zip(leaves, g)]
    grads['kl'] = [a - b for a, b in zip(grads['cross_entropy'], grads['entropy'])]      # (the derivative is linear)
    out = {}
    for mode in MODES:
        g = grads[mode]
        out[mode] = (float(vals[mode].detach()), dict(zip(NAMES, g[:4])), dict(zip(NAMES, g[4:])))
    return out


def batch_reference(elp_bt, lengths, trans, init, lens, kp, no_eos, endpen, q, mode, up, group=None, n_states=None,
                    frame_offset=None):
    """Sum over the videos of a batch of up[i] x the gradient of video i, in the layouts of the kernels: (values [b], p's grads
    dict(elp, trans, init, len), q's grads alike); `mode` None: {mode: that triple} for all three from one pass.  q = (elp_bt,
    lengths, trans, init, lens, endpen), the layout of p's arguments.

    Without the optional arguments: a padded single-group batch, elp_bt [b, tmax, c] (grads' elp [b * tmax, c]), trans [c, c],
    init [c], lens [k_rows, c], kp one number.  With `group` (per video) and `n_states` (per group) the tables are stacked per
    group and padded to c_max columns -- trans [g, c_max, c_max], init [g, c_max], lens [g, k_rows, c_max], endpen [b, c_max] --
    and only the leading n_states[g] states of a video's group are read; `kp` may be one number per video; with `frame_offset`
    elp is packed, [total_frames, c_max], video i at rows frame_offset[i] .. + lengths[i].  The gradients keep these layouts."""
    b = len(lengths)
    packed = frame_offset is not None
    elp_p, elp_q = np.asarray(elp_bt), np.asarray(q[0])
    cm = elp_p.shape[-1]
    if not packed:
        tmax = elp_p.shape[1]
        frame_offset = [i * tmax for i in range(b)]
        elp_p, elp_q = elp_p.reshape(b * tmax, cm), elp_q.reshape(b * tmax, cm)
    grouped = group is not None
    group = [0] * b if group is None else list(group)
    kps = [int(kp)] * b if np.ndim(kp) == 0 else [int(v) for v in kp]
    tab = lambda a: np.asarray(a, dtype=np.float64) if grouped else np.asarray(a, dtype=np.float64)[None]
    tabs_p, tabs_q = [tab(a) for a in (trans, init, lens)], [tab(a) for a in (q[2], q[3], q[4])]
    n_states = [cm] * tabs_p[0].shape[0] if n_states is None else list(n_states)
    zeros = lambda: dict(elp=torch.zeros(elp_p.shape, dtype=F64), trans=torch.zeros(tabs_p[0].shape, dtype=F64),
                         init=torch.zeros(tabs_p[1].shape, dtype=F64), len=torch.zeros(tabs_p[2].shape, dtype=F64))
    acc = {m: (np.zeros(b), zeros(), zeros()) for m in MODES}
    for i, fr in enumerate(lengths):
        g, o = group[i], int(frame_offset[i])
        c = n_states[g]
        side = lambda e, t: dict(elp=e[o:o + fr, :c], trans=t[0][g, :c, :c], init=t[1][g, :c], len=t[2][g, :, :c])
        ep = lambda a: None if a is None else np.asarray(a)[i, :c]
        r = video_reference(side(elp_p, tabs_p), side(elp_q, tabs_q), kps[i], no_eos, ep(endpen), ep(q[5]))
        for m in MODES:
            v, a, bq = r[m]
            acc[m][0][i] = v
            for dst, src in ((acc[m][1], a), (acc[m][2], bq)):
                dst['elp'][o:o + fr, :c] += up[i] * src['elp']
                dst['trans'][g, :c, :c] += up[i] * src['trans']
                dst['init'][g, :c] += up[i] * src['init']
                dst['len'][g, :, :c] += up[i] * src['len']
    if not grouped:
        for m in MODES:
            for dst in acc[m][1:]:
                for k in ('trans', 'init', 'len'):
                    dst[k] = dst[k][0]
    return acc if mode is None else acc[mode]
