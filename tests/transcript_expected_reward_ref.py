"""The expected reward V = E[R(y)] under the transcript-graph posterior over ALIGNMENTS and its gradient with respect to the
tables (include/smmdp.h: smm_align_graph_expected_reward_f64, smm_align_graph_expected_reward_bwd_f64), by two routes in fp64
torch that share no code with the kernels.  A graph is (a, pred, start, end) as in tests/align_graph_ref.py; a side is (elp,
trans, init, len_scores, endpen or None) in numpy.  ``reward`` [T, C] and ``node_reward`` [M] numpy, either may be None:
    R(y) = sum over the segments (node j, frames s .. n-1) of y of  node_reward[j] + sum_t reward[t, a_j]

  enumeration_reward  (a) V = sum_y p(y) R(y) over transcript_sample_ref.enumerate_alignments, the gradient by autograd through
                      the softmax of the enumerated scores.  Robust to -1e9 and -inf entries.
  identity_reward     (b) transcript_graph_ref.torch_logz_graph differentiated twice.  Every node gets a class of its own
                      (C' = M: elp'[:, m] = elp[:, a_m], len'[:, m] = len[:, a_m], trans'[m][j] = trans[a_m][a_j],
                      init'[m] = init[a_m]), so that the posterior that node m covers frame t is d log Z_g / d elp'[t, m] and
                      the posterior that the path crosses m is sum_k d log Z_g / d len'[k, m]:
                          V = <d log Z_g / d elp', reward'> + <sum_k d log Z_g / d len'[k, .], node_reward>
                      and autograd folds the second derivative back over the nodes of each class.  Finite tables only."""
import numpy as np
import torch

import transcript_graph_ref as TG
import transcript_sample_ref as TS
from transcript_entropy_grad_ref import KEYS, _grads, _scores, _torch_side


def _zeros(side):
    return {k: np.zeros(np.asarray(v).shape) for k, v in zip(KEYS, side[:4])}


def reward_of(key, a, T, reward, node_reward):
    """R(y) of one enumerated alignment (path, cuts)."""
    path, cuts = key
    b = (0,) + tuple(cuts) + (T,)
    r = 0.0
    for i, m in enumerate(path):
        if node_reward is not None:
            r += float(node_reward[m])
        if reward is not None:
            r += float(np.asarray(reward, np.float64)[b[i]:b[i + 1], a[m]].sum())
    return r


def enumeration_reward(side, graph, kp, reward=None, node_reward=None):
    """-> (V, dict(elp, trans, init, len)); (nan, zeros) when the video has no alignment."""
    a = TG._graph(graph)[0]
    T = np.asarray(side[0]).shape[0]
    aligns = TS.enumerate_alignments(side[0], graph, side[1], side[2], side[3], kp, side[4])
    if not aligns:
        return float('nan'), _zeros(side)
    keys = list(aligns)
    t, ep = _torch_side(side)
    pr = torch.softmax(_scores(keys, T, a, t, ep), dim=0)
    r = torch.tensor([reward_of(k, a, T, reward, node_reward) for k in keys], dtype=torch.float64)
    v = (pr * r).sum()
    v.backward()
    return float(v.detach()), _grads(t)


def identity_reward(side, graph, kp, reward=None, node_reward=None):
    """-> (V, dict(elp, trans, init, len)); (nan, zeros) when the video has no alignment."""
    a, pred, start, end = TG._graph(graph)
    M = len(a)
    idx = torch.tensor(a, dtype=torch.long)
    t, ep = _torch_side(side)
    elp2, len2 = t[0][:, idx], t[3][:, idx]
    trans2, init2 = t[1][idx][:, idx], t[2][idx]
    ep2 = None if ep is None else ep[idx]
    z = TG.torch_logz_graph(elp2, (np.arange(M), pred, start, end), trans2, init2, len2, kp, ep2)
    if not bool(torch.isfinite(z)):
        return float('nan'), _zeros(side)
    mu_elp, mu_len = torch.autograd.grad(z, [elp2, len2], create_graph=True)
    v = torch.zeros((), dtype=torch.float64)
    if reward is not None:
        v = v + (mu_elp * torch.tensor(np.asarray(reward, np.float64))[:, idx]).sum()
    if node_reward is not None:
        v = v + (mu_len.sum(dim=0) * torch.tensor(np.asarray(node_reward, np.float64))).sum()
    g = torch.autograd.grad(v, t, allow_unused=True)
    return float(v.detach()), {k: (np.zeros(tuple(x.shape)) if gx is None else gx.numpy()) for k, gx, x in zip(KEYS, g, t)}


def abs_reward(graph, T, n_states, reward=None, node_reward=None):
    """sum |reward| over the entries a video covers + sum |node_reward|: what the value's rounding scales with."""
    s = 0.0
    if reward is not None:
        s += float(np.abs(np.asarray(reward, np.float64)[:T, :n_states]).sum())
    if node_reward is not None:
        s += float(np.abs(np.asarray(node_reward, np.float64)).sum())
    return s
