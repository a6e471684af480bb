"""fp64 references of the expected frame- and segment-additive reward V = E_p[R(y)] and of its gradient with respect to the factor
tables (smm_expected_reward_f64 / smm_expected_reward_bwd_f64), two independent statements in torch; nothing is shared with the
kernels or with the C twin.  The conventions are those of tests/entropy_grad_ref.py (table layouts, kp, no_eos, the closing
label without EOS, the EOS closing weight `_wend` as a constant of the tables).

R(y) = phi(y) . rho with phi the occurrence counts of y: on the elp block rho holds `reward`, on every len[k][c] entry and, without
EOS, on the closing elp row it holds seg_reward[c] (the closing label counts as a one-frame span), on trans and init 0.

(a) `video_enumeration`: every segmentation listed, V = sum_y softmax(s)(y) R(y), the gradient by autograd.
(b) `video_polynomial`: mu = d log Z / d theta kept differentiable through entropy_grad_dp_ref._logz, V = mu . rho, the gradient
    by a second autograd pass (a Hessian-vector product)."""
import numpy as np
import torch

import entropy_grad_dp_ref as D
import entropy_grad_ref as R

F64 = torch.float64
NAMES = ('elp', 'trans', 'init', 'len')


def _rho(frames, c, k_rows, no_eos, reward, seg_reward):
    """(rho_elp [frames, c] without the closing label's segment, the closing row's segment reward [frames, c], rho_len [k_rows, c])."""
    rw = torch.zeros(frames, c, dtype=F64) if reward is None else torch.as_tensor(np.asarray(reward), dtype=F64)
    sg = torch.zeros(c, dtype=F64) if seg_reward is None else torch.as_tensor(np.asarray(seg_reward), dtype=F64)
    close = torch.zeros(frames, c, dtype=F64)
    if no_eos:
        close[frames - 1] = sg
    return rw, close, sg.unsqueeze(0).expand(k_rows, c).clone()


def video_enumeration(t, reward, seg_reward, kp, no_eos, endpen=None):
    """One video by enumeration: t dict of fp64 arrays elp [frames, c], trans [c, c], init [c], len [k_rows, c].
    -> (V, frame part, segment part, grads dict of the four tables)."""
    tt = {k: torch.as_tensor(np.asarray(t[k]), dtype=F64) for k in NAMES}
    frames, c = tt['elp'].shape
    k_rows = tt['len'].shape[0]
    phi, last = R.occurrences(frames, c, k_rows, kp, no_eos)
    th = R._flat(tt).clone().requires_grad_(True)
    s = phi @ th
    if not no_eos:
        s = s + R._wend(tt['trans'], endpen)[last]
    p = torch.softmax(s, 0)
    rw, close, rl = _rho(frames, c, k_rows, no_eos, reward, seg_reward)
    zt = dict(trans=torch.zeros(c, c, dtype=F64), init=torch.zeros(c, dtype=F64))
    r_frame = phi @ R._flat(dict(elp=rw, len=torch.zeros_like(rl), **zt))
    r_seg = phi @ R._flat(dict(elp=close, len=rl, **zt))
    vf, vs = (p * r_frame).sum(), (p * r_seg).sum()
    g, = torch.autograd.grad(vf + vs, th)
    return float((vf + vs).detach()), float(vf.detach()), float(vs.detach()), R._unflat(g.detach(), frames, c, k_rows)


def video_polynomial(t, reward, seg_reward, kp, no_eos, endpen=None):
    """One video in polynomial time: V = d log Z / d theta . rho, its gradient a second autograd pass.  Same result layout."""
    th = D._leaves(t)
    frames, c = th['elp'].shape
    k_rows = th['len'].shape[0]
    w = None if no_eos else R._wend(th['trans'], endpen).detach().clone().requires_grad_(True)
    lz = D._logz(th, w, kp, no_eos)
    mu_elp, mu_len = torch.autograd.grad(lz, (th['elp'], th['len']), create_graph=True, allow_unused=True)
    mu_len = torch.zeros_like(th['len']) if mu_len is None else mu_len
    rw, close, rl = _rho(frames, c, k_rows, no_eos, reward, seg_reward)
    vf = (mu_elp * rw).sum()
    vs = (mu_elp * close).sum() + (mu_len * rl).sum()
    leaves = [th[k] for k in NAMES]
    g = torch.autograd.grad(vf + vs, leaves, allow_unused=True)
    g = [torch.zeros_like(x) if gg is None else gg.detach() for x, gg in zip(leaves, g)]
    return float((vf + vs).detach()), float(vf.detach()), float(vs.detach()), dict(zip(NAMES, g))


def batch_reference(video_fn, elp, lengths, trans, init, lens, kp, no_eos, endpen, reward, seg_reward, up, group=None,
                    n_states=None, frame_offset=None):
    """Sum over the videos of a batch of up[i] x the gradient of video i, in the layouts of the kernels: (values [b], parts
    [b, 2], grads dict(elp, trans, init, len)).  Layout rules as entropy_grad_dp_ref.batch_reference: without the optional
    arguments a padded single-group batch (elp, reward [b, tmax, c]; trans [c, c]; seg_reward [c]); with `group`, `n_states` and
    `frame_offset` packed and stacked per group (elp, reward [total_frames, c_max]; seg_reward [g, c_max])."""
    b = len(lengths)
    packed = frame_offset is not None
    elp = np.asarray(elp)
    cm = elp.shape[-1]
    rw = None if reward is None else np.asarray(reward)
    if not packed:
        tmax = elp.shape[1]
        frame_offset = [i * tmax for i in range(b)]
        elp = elp.reshape(b * tmax, cm)
        rw = None if rw is None else rw.reshape(b * tmax, cm)
    grouped = group is not None
    group = [0] * b if group is None else list(group)
    kps = [int(kp)] * b if np.ndim(kp) == 0 else [int(v) for v in kp]
    tab = lambda a: np.asarray(a, dtype=np.float64) if grouped else np.asarray(a, dtype=np.float64)[None]
    tabs = [tab(a) for a in (trans, init, lens)]
    sg = None if seg_reward is None else tab(seg_reward)
    n_states = [cm] * tabs[0].shape[0] if n_states is None else list(n_states)
    g_out = dict(elp=torch.zeros(elp.shape, dtype=F64), trans=torch.zeros(tabs[0].shape, dtype=F64),
                 init=torch.zeros(tabs[1].shape, dtype=F64), len=torch.zeros(tabs[2].shape, dtype=F64))
    vals, parts = np.zeros(b), np.zeros((b, 2))
    for i, fr in enumerate(lengths):
        g, o = group[i], int(frame_offset[i])
        c = n_states[g]
        side = dict(elp=elp[o:o + fr, :c], trans=tabs[0][g, :c, :c], init=tabs[1][g, :c], len=tabs[2][g, :, :c])
        v, vf, vs, gr = video_fn(side, None if rw is None else rw[o:o + fr, :c], None if sg is None else sg[g, :c], kps[i], no_eos,
                                 None if endpen is None else np.asarray(endpen)[i, :c])
        vals[i], parts[i] = v, (vf, vs)
        g_out['elp'][o:o + fr, :c] += up[i] * gr['elp']
        g_out['trans'][g, :c, :c] += up[i] * gr['trans']
        g_out['init'][g, :c] += up[i] * gr['init']
        g_out['len'][g, :, :c] += up[i] * gr['len']
    if not grouped:
        for k in ('trans', 'init', 'len'):
            g_out[k] = g_out[k][0]
    return vals, parts, g_out


SETTINGS = ('both', 'reward', 'seg_reward')


def small_rewards(seed, b, tmax, c, setting):
    """The rewards of an enumerable lattice: N(0, 1) draws; `setting` says which of the two is given."""
    rng = np.random.default_rng(seed)
    reward, seg = rng.normal(size=(b, tmax, c)), rng.normal(size=c)
    return (reward if setting != 'seg_reward' else None), (seg if setting != 'reward' else None)
