"""``SemiMarkovModule``: the reference's HSMM parameter container and decode entry points, MI355X back-end.

Mirrors reference ``src/models/semimarkov/semimarkov_modules.py`` (``SemiMarkovModule`` :52) -- same constructor,
parameter names (picklable / ``state_dict``-compatible: ``poisson_log_rates, gaussian_means, gaussian_cov,
transition_logits, init_logits, init_constraints, transition_constraints``), same method names, arguments and
return conventions -- for the decode path only.  What differs is *how* ``viterbi`` / ``log_likelihood`` compute:
the reference materialises dense ``b x N x K x C x C`` potentials (``log_hsmm`` :416-523) and hands them to
pytorch-struct; here the factors (emission scores, transition / initial / length tables) go straight to the HIP
kernels of ``libsmmdp.so`` (include/smmdp.h) and no dense tensor exists.

There is no CPU path: ``viterbi`` / ``log_likelihood`` need CUDA(HIP) tensors and raise otherwise.
``log_hsmm`` / ``score_features`` (the dense potentials) are kept as plain torch code for API compatibility and
small-shape inspection; nothing in this package's decode path calls them.
"""
import math
import pickle
import types
from typing import Dict, Set

import contextlib
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .flow import FeatureProjector
from .semimarkov_utils import semimarkov_sufficient_stats, semimarkov_sufficient_stats_device

BIG_NEG = -1e9  # reference semimarkov_modules.py:20


def all_equal(xs):
    xs = list(xs)
    return all(x == xs[0] for x in xs[1:])


def sliding_sum(inputs, k):
    """out[b,t,c] = sum_{j=t}^{t+k-1} inputs[b,j,c] (terms past the end dropped).  Reference :26-39."""
    assert k > 0
    out = inputs.clone()
    n = inputs.size(1)
    for j in range(1, min(k, n)):       # direct accumulation: no prefix-sum cancellation in fp32
        out[:, :n - j] += inputs[:, j:]
    return out


BATCH_MEAN_DENSE_MAX = 1 << 22     # log_likelihood_packed: entries of the [batches, videos] mean matrix; beyond that, sums by index


TABLE_NAMES = ('w', 'cst', 'trans', 'init', 'len')


def _one_group(tab):
    """The cached tables of one class set as a stack of ONE group -> (w, cst, trans, init, len, class_map), built on first use
    (ten views less per call)."""
    g1 = tab.get('_one_group')
    if g1 is None:
        g1 = tab['_one_group'] = tuple(tab[k].unsqueeze(0).contiguous() for k in TABLE_NAMES) + (tab['class_map'].view(1, -1),)
    return g1


def _emit(batch, x, cons, endpen, g, inv_var):
    """The emission launch of a staged batch, padded or packed; ``g``: (w, cst, trans, init, len, class_map) stacked per group.
    -> the record every operation below reads: dict(batch, elp, trans, init, len, class_map, endpen, x)."""
    elp, _ = ops.emission(batch, x, g[0], g[1], inv_var, cons=cons)
    return dict(batch=batch, elp=elp, trans=g[2], init=g[3], len=g[4], class_map=g[5], endpen=endpen, x=x)


def _emit_logz(batch, x, cons, endpen, g, inv_var, with_backward):
    """``_emit`` + log Z on a private workspace, for the launches that read the forward (and backward) histories afterwards:
    the record gains ``ws`` and ``logz``.  ``with_backward``: the log Z launch also runs the time-reversed recursion
    (SMM_SHAPE_LOGZ_BOTH), one more workgroup per video."""
    r = _emit(batch, x, cons, endpen, g, inv_var)
    r['ws'] = torch.empty(batch.workspace_bytes(), dtype=torch.uint8, device=x.device)
    r['logz'] = ops.logz(batch, r['elp'], r['trans'], r['init'], r['len'], endpen=endpen, ws=r['ws'], with_backward=with_backward)
    return r


def _side(r):
    """A launched posterior as one side of ops.kl / ops.kl_bwd."""
    return r['elp'], r['trans'], r['init'], r['len'], r['endpen'], r['logz'], r['ws']


def _after_logz(r):
    """The same seven as the keyword arguments of the launchers that follow a log Z launch on its workspace."""
    return dict(elp=r['elp'], trans=r['trans'], init=r['init'], len_scores=r['len'], logz_val=r['logz'], endpen=r['endpen'],
                ws=r['ws'])


def _paths(batch, out, want_spans):
    """A path launch's result as its entry point hands it out: spans on the CPU for a padded batch (without the EOS column for
    add_eos=False, as ``viterbi`` returns them), frame labels on the device for a packed one.  Raises SmmError when a NaN
    reached the DP."""
    paths = out['spans'].cpu() if want_spans else out['labels']
    ops.check_decoded(batch, out)
    if want_spans and batch.no_eos:
        paths = paths[..., :batch.t_max].contiguous()
    return paths


def _check_workspace(r):
    ops.check_decoded(r['batch'], dict(_err=ops._err_copy(r['batch'], r['ws'])))


def _sample(r, n_samples, seed, want_spans):
    out = ops.sample(r['batch'], n_samples=n_samples, seed=seed, class_map=r['class_map'], want_spans=want_spans,
                     want_labels=not want_spans, **_after_logz(r))
    return _paths(r['batch'], out, want_spans), out['logp']


def _marginals(r, with_backward=False):
    """Posterior class occupancy of every frame: the d log Z / d elp of smm_logz_bwd_f64, fp64 [total_frames, c_max]."""
    return ops.logz_bwd(r['batch'], with_backward=with_backward, **_after_logz(r))['elp']


def _mbr(r, want_spans):
    out = ops.mbr(r['batch'], _marginals(r, with_backward=True), r['trans'], r['init'], endpen=r['endpen'],
                  class_map=r['class_map'], ws=r['ws'], want_spans=want_spans, want_labels=not want_spans)
    return _paths(r['batch'], out, want_spans), out['gain_sum']


def _entropy(r, with_backward):
    """-> (H, p's launch, None): what _PosteriorValue's ``launch`` returns.  ``with_backward``: as given to the log Z launch;
    without it the entropy launch runs the time-reversed recursion itself, into ``ws``, where the backward finds both."""
    h = ops.entropy(r['batch'], with_backward=with_backward, **_after_logz(r))
    _check_workspace(r)
    return h, r, None


def _expected_reward(r, reward, seg_reward, with_backward):
    """-> (V, p's launch, None): what _PosteriorValue's ``launch`` returns; the launch keeps the rewards for the backward."""
    r['reward'], r['seg_reward'] = reward, seg_reward
    v = ops.expected_reward(r['batch'], reward=reward, seg_reward=seg_reward, with_backward=with_backward, **_after_logz(r))
    _check_workspace(r)
    return v, r, None


def _reward_tensor(t, shape, dev, what):
    """A reward as the launch takes it: fp64, contiguous, on the device, of the given shape; one that requires grad is refused."""
    if t is None:
        return None
    t = torch.as_tensor(t)
    if t.requires_grad:
        raise ValueError("%s requires grad: the expected reward is differentiable with respect to the model's parameters "
                         "only (d V / d reward is the frame posterior, ``frame_posteriors``)" % what)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: shape %s expected, got %s" % (what, tuple(shape), tuple(t.shape)))
    return t.detach().to(device=dev, dtype=torch.float64).contiguous()


def _segment_posteriors(r, spans, with_backward, want_spans=True):
    """Boundary posteriors of a launched posterior and the posterior of each segment of ``spans`` ([n_sets, b, t_max+1] or
    [b, t_max+1], any device; a row of t_max entries -- ``viterbi``'s add_eos=False format -- gets its last column back; None:
    the Viterbi decode on the same emissions).  -> dict(start, end, boundary, seg_logp, spans), all on the device."""
    batch = r['batch']
    if want_spans and spans is None:
        out = ops.viterbi(batch, r['elp'], r['trans'], r['init'], r['len'], endpen=r['endpen'], class_map=r['class_map'],
                          want_spans=True, want_labels=False)
        ops.check_decoded(batch, out)
        spans = out['spans']
    if spans is not None:
        spans = torch.as_tensor(spans).to(device=r['elp'].device, dtype=torch.int64)
        if spans.size(-1) == batch.t_max:
            spans = torch.nn.functional.pad(spans, (0, 1), value=-1)
        spans = spans.contiguous()
    out = ops.segment_posteriors(batch, spans=spans, class_map=r['class_map'], with_backward=with_backward, **_after_logz(r))
    _check_workspace(r)
    out['spans'] = spans
    del out['_err']
    return out


def _kl(r, q, what, with_backward, want_cross_entropy):
    """-> (KL(p || q) or H(p, q), p's launch, q's launch).  ``with_backward``: as given to p's log Z launch."""
    SemiMarkovModule._check_same_batch(r['batch'], q['batch'], what)
    out = ops.kl(r['batch'], _side(r), _side(q), with_backward=with_backward, want_cross_entropy=want_cross_entropy)
    _check_workspace(r)
    return (out[1] if want_cross_entropy else out), r, q


def _kbest(r, k, want_spans):
    out = ops.kbest(r['batch'], r['elp'], r['trans'], r['init'], r['len'], k, endpen=r['endpen'], class_map=r['class_map'],
                    want_spans=want_spans, want_labels=not want_spans)
    return _paths(r['batch'], out, want_spans), out['score']


# The ``ops`` launchers of the transcript family by the kind of supervision: alignment, likelihood as the backward needs it,
# that backward, likelihood as a value.  A supervision is (kind, what the launchers take behind the tables): ('chain',
# (transcripts,)), ('optional', (transcripts, flags)) or ('graph', (graphs,)), all in LOCAL state ids.
_ALIGN, _LOGZ, _LOGZ_BWD, _SCORE = range(4)
_TRANSCRIPT_OPS = {'chain': ('align', 'align_logz_ex', 'align_logz_bwd', 'align_logz'),
                   'optional': ('align_optional', 'align_opt_logz', 'align_opt_logz_bwd', 'align_opt_logz'),
                   'graph': ('align_graph', 'align_graph_logz', 'align_graph_logz_bwd', 'align_graph_logz')}


def _supervised(which, r, sup, *more, **kw):
    """The launcher ``which`` of the supervision's kind on the record of ``_emit``."""
    kind, given = sup
    return getattr(ops, _TRANSCRIPT_OPS[kind][which])(r['batch'], r['elp'], r['trans'], r['init'], r['len'], *given, *more,
                                                      endpen=r['endpen'], **kw)


def _align(r, sup, want_spans):
    """-> (spans or labels, scores); for graphs the per-video ``used`` flags of the nodes as a third result."""
    graphs = sup[0] == 'graph'
    out = _supervised(_ALIGN, r, sup, class_map=r['class_map'], want_spans=want_spans, want_labels=not want_spans,
                      **(dict(want_used=True) if graphs else {}))
    paths = _paths(r['batch'], out, want_spans)
    return (paths, out['best'], out['used']) if graphs else (paths, out['best'])


def _sample_alignments(r, sup, n_samples, seed, want_spans):
    """The forward launch over the graphs of ``sup`` on a private workspace, then the sampler on it: (spans or labels, logp,
    used).  A video without an alignment is no error: rows of -1 and logp NaN."""
    b = r['batch']
    z = _supervised(_LOGZ, r, sup)
    out = ops.align_graph_sample(b, r['elp'], r['trans'], r['init'], r['len'], sup[1][0], z['logz'], n_samples, seed=seed,
                                 endpen=r['endpen'], class_map=r['class_map'], ws=z['ws'], staged=z['_staged'],
                                 want_spans=want_spans, want_labels=not want_spans)
    return _paths(b, out, want_spans), out['logp'], out['used']


def _alignment_entropy(r, sup, want_parts):
    """The forward launch over the graphs of ``sup`` on a private workspace, then the entropy launch on it: (H, parts or None,
    (the forward launch,)).  A video without an alignment is no error: NaN."""
    b = r['batch']
    z = _supervised(_LOGZ, r, sup)
    out = ops.align_graph_entropy(b, r['elp'], r['trans'], r['init'], r['len'], sup[1][0], z['logz'], endpen=r['endpen'],
                                  ws=z['ws'], staged=z['_staged'], want_parts=want_parts)
    ops.check_decoded(b, out)
    return out['entropy'], out['parts'], (z,)


def _node_rewards(sup, node_reward, seg_reward, group, dev, what):
    """The rewards of the nodes as the launch takes them: fp64 [n_nodes] on the device, or None.  ``node_reward``: one tensor
    over all nodes or one sequence per video, laid out like the graphs' nodes; ``seg_reward``: n_groups x c_max on LOCAL states,
    broadcast over each node's class and added (a node whose class is no valid class of its video -- it leaves the video without
    an alignment -- gets none)."""
    graphs = sup[1][0]
    n = sum(len(g) for g in graphs)
    if isinstance(node_reward, (list, tuple)):
        if len(node_reward) != len(graphs):
            raise ValueError("%s: %d sequences of node rewards for %d videos" % (what, len(node_reward), len(graphs)))
        node_reward = torch.cat([torch.as_tensor(v, dtype=torch.float64).reshape(-1) for v in node_reward])
    nr = _reward_tensor(node_reward, (n,), dev, 'node_reward')
    if seg_reward is None:
        return nr
    ids = np.concatenate([np.asarray(g.ids, np.int64) for g in graphs])
    grp = np.concatenate([np.full(len(g), int(j), np.int64) for g, j in zip(graphs, group)])
    valid = torch.as_tensor(ids >= 0, device=dev)
    per_node = seg_reward[torch.as_tensor(grp, device=dev), torch.as_tensor(np.maximum(ids, 0), device=dev)]
    per_node = torch.where(valid, per_node, torch.zeros_like(per_node))
    return per_node.contiguous() if nr is None else nr + per_node


def _alignment_expected_reward(r, sup, want_parts):
    """The forward launch over the graphs of ``sup`` on a private workspace, then the expected-reward launch on it with the
    rewards the record holds: (V, parts or None, (the forward launch,)).  A video without an alignment is no error: NaN."""
    b = r['batch']
    z = _supervised(_LOGZ, r, sup)
    out = ops.align_graph_expected_reward(b, r['elp'], r['trans'], r['init'], r['len'], sup[1][0], z['logz'], reward=r['reward'],
                                          node_reward=r['node_reward'], endpen=r['endpen'], ws=z['ws'], staged=z['_staged'],
                                          want_parts=want_parts)
    ops.check_decoded(b, out)
    return out['value'], out['parts'], (z,)


def _alignment_segment_posteriors(r, sup, spans=None, used=None, want_alignment=True, want_dense=False):
    """The forward launch over the graphs of ``sup`` on a private workspace, then the segment-posterior launch on it, for the
    alignments ``spans`` / ``used`` (None with ``want_alignment``: the best alignment, one launch more, in front).  -> the dict of
    ``ops.align_graph_segment_posteriors`` with the alignments under ``spans`` and ``used``.  A video without an alignment is no
    error: NaN."""
    b = r['batch']
    graphs = sup[1][0]
    if want_alignment and spans is None:
        best = ops.align_graph(b, r['elp'], r['trans'], r['init'], r['len'], graphs, endpen=r['endpen'], class_map=r['class_map'],
                               want_spans=True, want_labels=False, want_used=True)
        ops.check_decoded(b, best)
        spans, used = best['spans'], best['used']
    if spans is not None:
        spans = torch.as_tensor(spans).to(device=r['elp'].device, dtype=torch.int64).contiguous()
    z = _supervised(_LOGZ, r, sup)
    out = ops.align_graph_segment_posteriors(b, r['elp'], r['trans'], r['init'], r['len'], graphs, z['logz'], spans=spans, used=used,
                                             endpen=r['endpen'], class_map=r['class_map'], ws=z['ws'], staged=z['_staged'],
                                             want_dense=want_dense)
    ops.check_decoded(b, out)
    out['spans'], out['used'], out['logz'] = spans, used, z['logz']
    for key in ('_err', '_staged'):
        del out[key]
    return out


def _alignment_kl(r, q, sup, what, want_cross_entropy, want_parts):
    """One forward launch per side over the graphs of ``sup``, each on a private workspace, then the KL launch on both
    (smm_align_graph_kl_f64): (KL(p || q) or H(p, q), parts or None, (p's forward launch, q's)).  A video p cannot align is no
    error: NaN."""
    b = r['batch']
    SemiMarkovModule._check_same_batch(b, q['batch'], what)
    zq = _supervised(_LOGZ, q, sup)
    zp = _supervised(_LOGZ, r, sup, staged=zq['_staged'])
    out = ops.align_graph_kl(b, (r['elp'], r['trans'], r['init'], r['len'], r['endpen'], zp['logz'], zp['ws']),
                             (q['trans'], q['len'], q['endpen'], zq['logz'], zq['ws']), sup[1][0], staged=zp['_staged'],
                             want_cross_entropy=want_cross_entropy, want_parts=want_parts)
    ops.check_decoded(b, out)
    ops.check_decoded(b, zq)                                   # (the KL launch leaves q's error word as q's forward launch set it)
    return (out['cross_entropy'] if want_cross_entropy else out['kl']), out['parts'], (zp, zq)


def _transcript_scores(r, sup, conditional, what):
    """Without autograd: the likelihood of the supervision per video (``conditional``: minus log Z) as a CPU fp64 tensor."""
    z = _supervised(_SCORE, r, sup)
    z = z if torch.is_tensor(z) else z['logz']
    if conditional:
        z = z - ops.logz(r['batch'], r['elp'], r['trans'], r['init'], r['len'], endpen=r['endpen'])
    return _check_transcript_logz(z, None, what, allow_none=True)


def _transcript_posteriors(r, sup, what, **want):
    """The forward and the backward launch of an 'optional' or 'graph' supervision for the posteriors ``want`` names."""
    out = _supervised(_LOGZ, r, sup)
    grads = _supervised(_LOGZ_BWD, r, sup, out['logz'], ws=out['ws'], staged=out['_staged'], **want)
    _check_transcript_logz(out['logz'], None, what, allow_none=True)
    return grads


def _feature_grad_inputs(ctx, slot, w, inv_var):
    """What the backward of a likelihood Function keeps beside its own tensors when the features (input ``slot``) want a
    gradient -- they are a feature projection's output then: the emission factors smm_emission_bwd_x_f64 reads."""
    return (w, inv_var) if ctx.needs_input_grad[slot] else ()


def _feature_grad(ctx, slot, x, g_elp, kept):
    """d L / d x from d L / d elp (smm_emission_bwd_x_f64), or None when the features carry no gradient."""
    if not ctx.needs_input_grad[slot]:
        return None
    w, inv_var = kept
    g_x = ops.emission_bwd_x(ctx.batch, x, g_elp, w.detach().contiguous(), inv_var.detach().contiguous(), ws=ctx.ws)
    if g_x.size(0) != x.size(0):                                  # (features longer than the launch's frame axis: no gradient there)
        g_x = torch.cat([g_x, g_x.new_zeros((x.size(0) - g_x.size(0), g_x.size(1)))])
    return g_x


class _LogPartition(torch.autograd.Function):
    """log Z of every video of one launch as a differentiable function of the fp64 factor tables (emission factors w,
    cst; transition, initial and length tables; stacked per parameter group).  Forward: smm_emission_f64 +
    smm_logz_f64; backward: smm_logz_bwd_f64 (posterior marginals) + smm_emission_bwd_f64 (the chain rule through
    elp = cst + x.w - 0.5 x^2.inv_var, one pass over the features)."""

    @staticmethod
    def forward(ctx, batch, x, cons, endpen, w, cst, inv_var, trans, init, len_scores):
        # a gradient will be asked for: the time-reversed recursion (independent of the forward one) rides in the same
        # launch; the private workspace survives until backward
        both = any(ctx.needs_input_grad)
        r = _emit_logz(batch, x, cons, endpen, (w, cst, trans, init, len_scores, None), inv_var, with_backward=both)
        ctx.batch, ctx.endpen, ctx.ws, ctx.both = batch, endpen, r['ws'], both
        ctx.save_for_backward(x, r['elp'], trans, init, len_scores, r['logz'], *_feature_grad_inputs(ctx, 1, w, inv_var))
        return r['logz']

    @staticmethod
    def backward(ctx, gz):
        r = dict(zip(('x', 'elp', 'trans', 'init', 'len', 'logz'), ctx.saved_tensors), endpen=ctx.endpen, ws=ctx.ws)
        g = ops.logz_bwd(ctx.batch, grad_logz=gz.to(torch.float64).contiguous(), with_backward=ctx.both, **_after_logz(r))
        # chain rule through elp = cst + x.w - 0.5 x^2.inv_var: one pass over x (smm_emission_bwd_f64)
        g_w, g_cst, g_iv = ops.emission_bwd(ctx.batch, r['x'], g['elp'], ws=ctx.ws)
        g_x = _feature_grad(ctx, 1, r['x'], g['elp'], ctx.saved_tensors[6:])
        return None, g_x, None, None, g_w, g_cst, g_iv, g['trans'], g['init'], g['len']


class _AlignmentLogPartition(torch.autograd.Function):
    """The likelihood of every video's supervision in one launch, as a differentiable function of the fp64 factor tables,
    beside ``_LogPartition``: log Z_a -- the sum over the segmentations whose class sequence is the video's transcript --, log
    Z_o -- over every alignment with any subset of the optional entries left out -- or log Z_g -- over every alignment to
    every start -> end path of the video's graph --, by the kind of ``sup`` (``_TRANSCRIPT_OPS``).  Forward: smm_emission_f64 +
    the kind's forward launch on a private workspace that survives until backward; backward: the kind's backward launch (the
    posterior of the alignments) + smm_emission_bwd_f64."""

    @staticmethod
    def forward(ctx, batch, x, cons, endpen, sup, w, cst, inv_var, trans, init, len_scores):
        r = _emit(batch, x, cons, endpen, (w, cst, trans, init, len_scores, None), inv_var)
        out = _supervised(_LOGZ, r, sup)
        if sup[0] == 'chain':       # the backward launch takes a plain transcript as the forward's (ids on the device, offsets)
            ctx.sup, ctx.staged = ('chain', (out['transcript'],)), {}
        else:                       # ... and the other kinds as they came, beside what the forward launch staged of them
            ctx.sup, ctx.staged = sup, dict(staged=out['_staged'])
        ctx.batch, ctx.endpen, ctx.ws = batch, endpen, out['ws']
        ctx.save_for_backward(x, r['elp'], trans, init, len_scores, out['logz'], *_feature_grad_inputs(ctx, 1, w, inv_var))
        return out['logz']

    @staticmethod
    def backward(ctx, gz):
        x, elp, trans, init, len_scores, logz = ctx.saved_tensors[:6]
        r = dict(batch=ctx.batch, elp=elp, trans=trans, init=init, len=len_scores, endpen=ctx.endpen)
        g = _supervised(_LOGZ_BWD, r, ctx.sup, logz, grad_logz=gz.to(torch.float64).contiguous(), ws=ctx.ws, **ctx.staged)
        g_w, g_cst, g_iv = ops.emission_bwd(ctx.batch, x, g['elp'], ws=ctx.ws)
        g_x = _feature_grad(ctx, 1, x, g['elp'], ctx.saved_tensors[6:])
        return None, g_x, None, None, None, g_w, g_cst, g_iv, g['trans'], g['init'], g['len']


def _alignment_log_partition(staged, sup):
    """``_AlignmentLogPartition`` on what ``_packed_stage`` returns (differentiable tables)."""
    batch, x, cons, endpen, g, inv_var = staged
    return _AlignmentLogPartition.apply(batch, x, cons, endpen, sup, g[0], g[1], inv_var, g[2], g[3], g[4])


def _check_ambiguous(ambiguous, what):
    if ambiguous not in ('raise', 'allow'):
        raise ValueError("%s: ambiguous must be 'raise' or 'allow'" % what)
    return ambiguous == 'raise'


def _video(names, i):
    """How a refusal names video ``i``: by its name in a corpus, by its index in a padded batch."""
    return i if names is None else names[i]


def _checked_graphs(graphs, n_videos, ambiguous, names, what):
    """The graphs of a launch, checked on the host before a device is touched: one ``ops.TranscriptGraph`` per video;
    ``ambiguous='raise'``: ValueError naming the first video two start -> end paths of whose graph spell the same class
    sequence (``TranscriptGraph.is_ambiguous``), ``'allow'``: the sum over paths and boundaries as defined."""
    refuse = _check_ambiguous(ambiguous, what)
    if len(graphs) != n_videos:
        raise ValueError("%s: %d graphs for %d videos" % (what, len(graphs), n_videos))
    for i, g in enumerate(graphs):
        if not isinstance(g, ops.TranscriptGraph):
            raise ValueError("%s: an ops.TranscriptGraph expected for video %r" % (what, _video(names, i)))
        if refuse and g.is_ambiguous():
            raise ValueError("%s: two start -> end paths of the graph of video %r spell the same class sequence, so its "
                             "segmentations would be counted once per path; pass ambiguous='allow' for that sum over "
                             "alignments" % (what, _video(names, i)))
    return list(graphs)


def _checked_optional(transcripts, optional, ambiguous, names, what):
    """The flags of a launch as boolean arrays, checked on the host before a device is touched (``transcripts`` in global or
    local ids: the map between them is one-to-one within a video): one sequence per video, as long as its transcript;
    ``ambiguous='raise'``: ValueError naming the first video two subsets of whose optional entries give the same class
    sequence (``ops.transcript_is_ambiguous``), ``'allow'``: the sum over alignments as defined."""
    refuse = _check_ambiguous(ambiguous, what)
    if len(optional) != len(transcripts):
        raise ValueError("%s: %d sequences of optional flags for %d videos" % (what, len(optional), len(transcripts)))
    flags = [np.asarray(f.detach().cpu() if torch.is_tensor(f) else f).reshape(-1) != 0 for f in optional]
    ids = [np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=np.int64).reshape(-1) for a in transcripts]
    for i, (a, f) in enumerate(zip(ids, flags)):
        if f.size != len(a):
            raise ValueError("%s: %d optional flags for the %d transcript entries of video %r"
                             % (what, f.size, len(a), _video(names, i)))
        if refuse and ops.transcript_is_ambiguous(a, f):
            raise ValueError("%s: two subsets of the optional entries of video %r give the same class sequence, so its "
                             "segmentations would be counted once per subset; pass ambiguous='allow' for that sum over "
                             "alignments" % (what, _video(names, i)))
    return flags


def _check_transcript_logz(z, names, what, allow_none=False):
    """The host's look at a launch's log Z_a (synchronises): SmmError for a NaN, ValueError -- naming the video -- for -inf."""
    zh = z.detach().cpu()
    if bool(torch.isnan(zh).any()):
        raise ops._lib.SmmError("libsmmdp: NaN (or +inf) in the DP inputs of %s" % what)
    bad = torch.nonzero(torch.isinf(zh)).reshape(-1).tolist()
    if bad and not allow_none:
        i = bad[0]
        raise ValueError("%s: no segmentation of video %r has its transcript (more entries than frames, too few for the span "
                         "limit, or forbidden by the tables): log Z_a = -inf cannot be trained on" % (what, _video(names, i)))
    return zh


def _table_grads(batch, x, g, ws):
    """(g_w, g_cst, g_trans, g_init, g_len) from the gradients of the tables and elp: the emission chain rule, one pass over x."""
    g_w, g_cst, _ = ops.emission_bwd(batch, x, g['elp'], ws=ws)
    return g_w, g_cst, g['trans'], g['init'], g['len']


class _PosteriorValue(torch.autograd.Function):
    """The entropy H(p), the expected reward E_p[R], the cross-entropy H(p, q) or KL(p || q) of every video as a differentiable
    function of the fp64 factor tables (w, cst, trans, init, len) of p, and of q for the two-sided values.  ``launch()`` computes the value exactly as the
    non-differentiable method does and returns (value, p's launch, q's launch or None); each launch keeps its private workspace
    (forward and time-reversed histories) until the backward runs.  Backward: smm_entropy_bwd_f64 / smm_expected_reward_bwd_f64 /
    smm_kl_bwd_f64 for p's tables, mu_q - mu_p (two smm_logz_bwd_f64) for q's, then the emission chain rule of each side."""

    @staticmethod
    def forward(ctx, kind, launch, *tables):
        value, r, q = launch()
        ctx.kind, ctx.r, ctx.q = kind, r, q
        return value

    @staticmethod
    def backward(ctx, gv):
        up = gv.to(torch.float64).contiguous()
        r, q = ctx.r, ctx.q
        b = r['batch']
        if ctx.kind == 'entropy':
            g = ops.entropy_bwd(b, grad_out=up, with_backward=True, **_after_logz(r))
            return (None, None) + _table_grads(b, r['x'], g, r['ws'])
        if ctx.kind == 'expected_reward':
            g = ops.expected_reward_bwd(b, reward=r['reward'], seg_reward=r['seg_reward'], grad_out=up, with_backward=True,
                                        **_after_logz(r))
            return (None, None) + _table_grads(b, r['x'], g, r['ws'])
        # (kl_bwd runs both sides' time-reversed recursions: q's launch ran only the forward one)
        g = ops.kl_bwd(b, _side(r), _side(q), grad_out=up, cross_entropy=ctx.kind == 'cross_entropy')
        mq = ops.logz_bwd(b, grad_logz=up, with_backward=True, **_after_logz(q))
        mp = ops.logz_bwd(b, grad_logz=up, with_backward=True, **_after_logz(r))
        gq = {k: mq[k] - mp[k] for k in ('elp', 'trans', 'init', 'len')}
        return (None, None) + _table_grads(b, r['x'], g, r['ws']) + _table_grads(b, q['x'], gq, q['ws'])


class _AlignmentValue(torch.autograd.Function):
    """``_PosteriorValue`` for the transcript-graph posteriors: the entropy, expected reward, cross-entropy or KL of every video's
    posterior over its ALIGNMENTS as a differentiable function of the fp64 factor tables of p, and of q for the two-sided values.  ``launch()``
    computes the value exactly as the non-differentiable method does and returns (value, [p's record, q's], the supervision,
    (p's forward launch, q's)); the forward launches keep their workspaces until the backward runs.  Backward:
    smm_align_graph_entropy_bwd_f64 / smm_align_graph_expected_reward_bwd_f64 / smm_align_graph_kl_bwd_f64 for p's tables,
    mu_q - mu_p (two smm_align_graph_logz_bwd_f64) for q's, then the emission chain rule of each side."""

    @staticmethod
    def forward(ctx, kind, launch, *tables):
        value, ctx.recs, ctx.sup, ctx.fwd = launch()
        ctx.kind = kind
        return value

    @staticmethod
    def backward(ctx, gv):
        up = gv.to(torch.float64).contiguous()
        r, zp, graphs = ctx.recs[0], ctx.fwd[0], ctx.sup[1][0]
        b = r['batch']
        side = (r['elp'], r['trans'], r['init'], r['len'], r['endpen'], zp['logz'], zp['ws'])
        if ctx.kind == 'entropy':
            g = ops.align_graph_entropy_bwd(b, *side[:4], graphs, zp['logz'], grad_out=up, endpen=r['endpen'], ws=zp['ws'],
                                            staged=zp['_staged'])
            return (None, None) + _table_grads(b, r['x'], g, zp['ws'])
        if ctx.kind == 'expected_reward':
            g = ops.align_graph_expected_reward_bwd(b, *side[:4], graphs, zp['logz'], reward=r['reward'], node_reward=r['node_reward'],
                                                    grad_out=up, endpen=r['endpen'], ws=zp['ws'], staged=zp['_staged'])
            return (None, None) + _table_grads(b, r['x'], g, zp['ws'])
        q, zq = ctx.recs[1], ctx.fwd[1]
        g = ops.align_graph_kl_bwd(b, side, (q['trans'], q['len'], q['endpen'], zq['logz'], zq['ws']), graphs, grad_out=up,
                                   staged=zp['_staged'], cross_entropy=ctx.kind == 'cross_entropy')
        mq = _supervised(_LOGZ_BWD, q, ctx.sup, zq['logz'], grad_logz=up, ws=zq['ws'], staged=zq['_staged'])
        mp = _supervised(_LOGZ_BWD, r, ctx.sup, zp['logz'], grad_logz=up, ws=zp['ws'], staged=zp['_staged'])
        gq = {k: mq[k] - mp[k] for k in ('elp', 'trans', 'init', 'len')}
        return (None, None) + _table_grads(b, r['x'], g, zp['ws']) + _table_grads(b, q['x'], gq, zq['ws'])


def _alignment_value(kind, what, names, sides, tables, want_parts):
    """The differentiable route of the ``alignment_*`` methods.  ``sides``: what ``_supervised_padded`` / ``_supervised_packed``
    return (the record of ``_emit``, the supervision), p's first, then q's for the two-sided values; ``tables``: each side's
    (w, cst, trans, init, len) with autograd history, which the gradients go to.  The value comes from the launches of the
    non-differentiable route, bit for bit; the parts carry no gradient.  A video without an alignment is refused here, by its
    name: a NaN cannot be trained on."""
    sup = sides[0][1]
    parts = []

    def launch():
        recs = [r for r, _ in sides]
        if kind == 'entropy':
            value, pt, fwd = _alignment_entropy(recs[0], sup, want_parts)
        elif kind == 'expected_reward':
            value, pt, fwd = _alignment_expected_reward(recs[0], sup, want_parts)
        else:
            value, pt, fwd = _alignment_kl(recs[0], recs[1], sup, what, kind == 'cross_entropy', want_parts)
        for z in fwd:
            _check_transcript_logz(z['logz'], names, what)
        parts.append(pt)
        return value, recs, sup, fwd

    value = _AlignmentValue.apply(kind, launch, *tables)
    return (value, parts[0]) if want_parts else value


class _FactorTables(torch.autograd.Function):
    """The fp64 factor tables of every parameter group of a launch as ONE differentiable node: smm_factor_tables_f64
    forward, smm_factor_tables_bwd_f64 backward (csrc/smm_tables.hip), instead of ~45 small torch ops each way.
    Returns (trans, init, len, w, cst, inv_var); inv_var carries no gradient (the covariance is not trained,
    reference :149)."""

    @staticmethod
    def forward(ctx, meta, init_cons, trans_cons, init_logits, transition_logits, poisson_log_rates, gaussian_means,
                gaussian_cov):
        t = ops.factor_tables(meta, init_logits, transition_logits, poisson_log_rates, gaussian_means, gaussian_cov,
                              init_cons, trans_cons)
        ctx.meta, ctx.init_cons, ctx.trans_cons = meta, init_cons, trans_cons
        ctx.save_for_backward(poisson_log_rates, gaussian_means, gaussian_cov, t['trans'], t['init'])
        ctx.mark_non_differentiable(t['inv_var'])
        return t['trans'], t['init'], t['len'], t['w'], t['cst'], t['inv_var']

    @staticmethod
    def backward(ctx, g_trans, g_init, g_len, g_w, g_cst, _g_iv):
        log_rates, means, cov, trans, init = ctx.saved_tensors
        cont = lambda t: None if t is None else t.contiguous()
        # the emission chain rule hands g_w over as a transposed view of its class-major buffer: undo the view
        g_w_cm = None if g_w is None else g_w.transpose(1, 2).contiguous()
        gi, gt, gr, gm, flat = ops.factor_tables_bwd(ctx.meta, log_rates, means, cov, trans, init, cont(g_trans), cont(g_init),
                                                     cont(g_len), g_w_cm, cont(g_cst), ctx.init_cons, ctx.trans_cons)
        # the four gradients are views of one fp64 buffer: one conversion launch for all of them
        f = flat.to(torch.float32)
        n, d = gi.numel(), gm.size(1)
        return (None, None, None, f[:n], f[n:n + n * n].view(n, n), f[n + n * n:2 * n + n * n], f[2 * n + n * n:].view(n, d), None)


class SemiMarkovModule(nn.Module):
    @classmethod
    def add_args(cls, parser):
        # reference :54-65, and the flags of the flow behind --sm_feature_projection (reference src/models/flow.py)
        parser.add_argument('--sm_max_span_length', type=int, default=20)
        parser.add_argument('--sm_supervised_state_smoothing', type=float, default=1e-2)
        parser.add_argument('--sm_supervised_length_smoothing', type=float, default=1e-1)
        parser.add_argument('--sm_supervised_method',
                            choices=['closed-form', 'gradient-based', 'closed-then-gradient'],
                            default='closed-form')
        parser.add_argument('--sm_feature_projection', action='store_true', help='use a flow')
        parser.add_argument('--sm_init_non_projection_parameters_from')
        parser.add_argument('--flow_hidden_layers', type=int, default=1)
        parser.add_argument('--flow_hidden_units', type=int, default=100)
        parser.add_argument('--flow_couple_layers', type=int, default=4)
        parser.add_argument('--flow_scale', action='store_true')
        parser.add_argument('--flow_scale_no_zero', action='store_true')

    def __init__(self, args, n_classes, n_dims, allow_self_transitions=False, allowed_starts: Set[int] = None,
                 allowed_transitions: Dict[int, Set[int]] = None, allowed_ends: Set[int] = None,
                 merge_classes: Dict[int, int] = None):
        super().__init__()
        self.args = args
        self.n_classes = n_classes
        self.input_feature_dim = n_dims
        self.feature_dim = n_dims
        self.allow_self_transitions = allow_self_transitions
        self.init_params()
        if allowed_starts is not None:
            assert allowed_transitions is not None
            self.set_transition_constraints(allowed_starts, allowed_transitions, allowed_ends)
        else:
            self.remove_transition_constraints()
        if getattr(args, 'sm_init_non_projection_parameters_from', None) is not None:
            with open(args.sm_init_non_projection_parameters_from, 'rb') as f:
                self.init_nonproject_parameters(pickle.load(f).model)
        self.init_projector()
        self.max_k = args.sm_max_span_length
        self._merge_classes = merge_classes
        self.kl = None

    # ------------------------------------------------------------------ parameters (reference :142-193)
    @property
    def merge_classes(self):
        return getattr(self, '_merge_classes', None)

    def init_nonproject_parameters(self, model):
        inc = self.load_state_dict(model.state_dict(), strict=False)
        assert not inc.unexpected_keys, inc.unexpected_keys
        assert all(k.startswith('feature_projector') for k in inc.missing_keys), inc.missing_keys

    def init_projector(self):
        """reference :131-140.  The additive flow (log det = 0) is built; --flow_scale, whose log-determinant the reference sums
        over padded frames as well, is not."""
        self.feature_projector = None
        if getattr(self.args, 'sm_feature_projection', False):
            if getattr(self.args, 'flow_scale', False):
                raise NotImplementedError("--flow_scale (the multiplicative coupling flow, with a non-zero log-determinant) is not "
                                          "built: --sm_feature_projection runs the additive flow only")
            self.feature_projector = FeatureProjector.from_args(self.args, self.feature_dim)

    def _project(self, x, projected=False):
        """Features fp32 [rows, D] on the device as the emission scorer sees them: through the feature projection when the
        module has one (smm_flow_f32; with gradients enabled the result carries the flow's autograd node), else as they are.
        ``projected``: x already IS the projection (``log_likelihood`` projects once for everything it calls)."""
        fp = getattr(self, 'feature_projector', None)
        return x if fp is None or projected else fp(x)

    def _project_packed(self, pc, x, differentiable=False):
        """``_project`` for the features of a PackedCorpus.  The projection of the resident ``pc.x`` is made once per parameter
        state and kept on the corpus -- one more copy of the features -- while ``pc.x`` (identity, version) and the flow's
        parameters (versions) stay what they were; ``differentiable`` with gradients enabled: a fresh autograd node instead.  A
        slab passed beside the corpus (``predict_host``) is projected and not kept."""
        fp = getattr(self, 'feature_projector', None)
        if fp is None:
            return x
        if differentiable and torch.is_grad_enabled():
            return fp(x)
        with torch.no_grad():
            # a slab beside the corpus is not kept; under stream capture the kept copy is neither read nor written: the captured
            # graph must hold the flow launch (a replay projects what pc.x holds then), and a buffer from the graph's pool is
            # not filled until the first replay
            if x is not pc.x or (x.is_cuda and torch.cuda.is_current_stream_capturing()):
                return fp(x)
            key = (x.data_ptr(), x._version, tuple(x.shape), fp.version_key())
            kept = pc.__dict__.get('_projected')
            if kept is None or kept[0] != key:
                kept = pc.__dict__['_projected'] = (key, fp(x))
            return kept[1]

    def _no_projected_gradient(self, *others):
        """The differentiable posterior values (entropy, KL, cross-entropy, expected reward, and their alignment forms) stop at
        the factor tables: with a feature projection they would silently leave the flow untrained."""
        if any(getattr(m, 'feature_projector', None) is not None for m in (self,) + others):
            raise NotImplementedError("differentiable=True does not reach through --sm_feature_projection: the gradients of the "
                                      "posterior values with respect to the flow's parameters are not built (log_likelihood's are)")

    def init_params(self):
        self.poisson_log_rates = nn.Parameter(torch.zeros(self.n_classes), requires_grad=True)
        self.gaussian_means = nn.Parameter(torch.zeros(self.n_classes, self.feature_dim), requires_grad=True)
        # shared, tied, diagonal covariance (stored as a dense D x D matrix like the reference)
        self.gaussian_cov = nn.Parameter(torch.eye(self.feature_dim), requires_grad=False)
        self.transition_logits = nn.Parameter(torch.zeros(self.n_classes, self.n_classes), requires_grad=True)  # to x from
        self.init_logits = nn.Parameter(torch.zeros(self.n_classes), requires_grad=True)
        torch.nn.init.uniform_(self.init_logits, 0, 1)

    def flatten_parameters(self):
        pass

    def remove_transition_constraints(self):
        self.transition_constraints = None
        self.init_constraints = None
        self.allowed_ends = None

    def set_transition_constraints(self, allowed_starts, allowed_transitions, allowed_ends):
        init_c = torch.ones(self.n_classes, dtype=torch.bool)           # True = forbidden
        assert all(x >= 0 for x in allowed_starts)
        init_c[torch.tensor(sorted(allowed_starts), dtype=torch.long)] = False
        trans_c = torch.ones(self.n_classes, self.n_classes, dtype=torch.bool)
        for src, targets in allowed_transitions.items():
            for tgt in targets:
                trans_c[tgt, src] = False
        # parameters so that .cuda() / state_dict carry them (reference :176-187)
        self.init_constraints = nn.Parameter(init_c, requires_grad=False)
        self.transition_constraints = nn.Parameter(trans_c, requires_grad=False)
        self.allowed_ends = allowed_ends

    # ------------------------------------------------------------------ closed-form supervised fit (:195-256)
    def fit_supervised(self, feature_list, label_list):
        if getattr(self, 'feature_projector', None) is not None:
            raise NotImplementedError("fit_supervised closed form with feature projector")
        if self.transition_constraints is not None or self.init_constraints is not None:
            raise NotImplementedError("fit_supervised closed form with constrained state transitions")
        a = self.args
        # module on the GPU: one HIP pass over the features (csrc/smm_fit.hip); module on the host: the reference's
        # host statement.  The placement decides, nothing falls back.
        if self.gaussian_means.is_cuda:
            stats_fn = lambda f, l: semimarkov_sufficient_stats_device(f, l, 'tied_diag', self.n_classes, self.max_k,
                                                                       device=self.gaussian_means.device)
        else:
            stats_fn = lambda f, l: semimarkov_sufficient_stats(f, l, 'tied_diag', self.n_classes, self.max_k)
        em, st = stats_fn(feature_list, label_list)
        if self.merge_classes is not None:
            table = torch.as_tensor([self.merge_classes[i] for i in range(self.n_classes)], dtype=torch.long)
            merged = [table.to(torch.as_tensor(labels).device)[torch.as_tensor(labels).long()] for labels in label_list]
            em_m, st_m = stats_fn(feature_list, merged)
        else:
            em_m, st_m = em, st
        with np.errstate(divide='ignore', invalid='ignore'):
            init_probs = (st['span_start_counts'] + a.sm_supervised_state_smoothing) / float(
                st['instance_count'] + a.sm_supervised_state_smoothing * self.n_classes)
            init_probs[np.isnan(init_probs)] = 0
            smoothed = st['span_transition_counts'] + a.sm_supervised_state_smoothing
            trans_probs = smoothed / smoothed.sum(axis=0)[None, :]
            trans_probs[np.isnan(trans_probs)] = 0
            mean_lengths = (st_m['span_lengths'] + a.sm_supervised_length_smoothing) / (
                st_m['span_counts'] + a.sm_supervised_length_smoothing)
        dev = self.init_logits.device
        with torch.no_grad():
            self.init_logits.copy_(torch.from_numpy(init_probs).to(dev).log())
            self.transition_logits.copy_(torch.from_numpy(trans_probs).to(dev).log())
            self.poisson_log_rates.copy_(torch.from_numpy(mean_lengths).to(dev).log())
            self.gaussian_means.copy_(torch.from_numpy(em_m.means_).to(dev).float())
            self.gaussian_cov.copy_(torch.diag(torch.from_numpy(em_m.covariances_[0]).to(dev).float()))

    def initialize_gaussian_from_feature_list(self, features):
        feats = torch.cat(features, dim=0)
        if getattr(self, 'feature_projector', None) is not None:
            with torch.no_grad():
                feats = self._project(feats.to(device=self.gaussian_means.device, dtype=torch.float32))
        assert feats.dim() == 2 and feats.size(1) == self.feature_dim
        with torch.no_grad():
            self.gaussian_means.copy_(feats.mean(dim=0, keepdim=True).expand(self.n_classes, self.feature_dim))
            self.gaussian_cov.data = torch.diag(feats.var(dim=0))

    def initialize_gaussian(self, data, lengths):
        self.initialize_gaussian_from_feature_list([data[i, :lengths[i]] for i in range(data.size(0))])

    # ------------------------------------------------------------------ scorers (:284-414); dtype follows the parameters
    def _merged(self, valid_classes):
        idx = valid_classes if valid_classes is not None else torch.arange(self.n_classes)
        if self.merge_classes is not None:
            idx = torch.as_tensor([self.merge_classes[int(ix)] for ix in idx], dtype=torch.long)
        return idx

    def _dev_index(self, kind, valid_classes, device):
        """Index tensors of a class set on the device, built once: ``vc`` (the class ids), ``merged`` (after
        merge_classes), ``class_map`` (ids + EOS).  A host -> device copy of a few integers per table and call is a
        stream synchronisation each; the training step builds six tables per class set."""
        cache = self.__dict__.setdefault('_index_cache', {})
        key = (kind, None if valid_classes is None else tuple(int(v) for v in valid_classes), str(device),
               id(getattr(self, 'merge_classes', None)))
        t = cache.get(key)
        if t is None:
            if len(cache) > 256:
                cache.clear()
            if kind == 'vc':
                t = valid_classes.to(device)
            elif kind == 'merged':
                t = self._merged(valid_classes).to(device)
            else:
                ids = list(range(self.n_classes)) if valid_classes is None else [int(v) for v in valid_classes]
                t = torch.tensor(ids + [self.n_classes], dtype=torch.int64, device=device)
            cache[key] = t
        return t

    def initial_log_probs(self, valid_classes, dtype=None):
        logits = self.init_logits if dtype is None else self.init_logits.to(dtype)
        if self.init_constraints is not None:
            logits = logits.masked_fill(self.init_constraints, BIG_NEG)
        if valid_classes is not None:
            logits = logits[self._dev_index('vc', valid_classes, logits.device)]
        return F.log_softmax(logits, dim=0)

    def transition_log_probs(self, valid_classes, dtype=None):
        t = self.transition_logits if dtype is None else self.transition_logits.to(dtype)
        if self.transition_constraints is not None:
            t = t.masked_fill(self.transition_constraints, BIG_NEG)
        if valid_classes is not None:
            vc = self._dev_index('vc', valid_classes, t.device)
            t = t[vc][:, vc]
        if not self.allow_self_transitions:
            t = t.masked_fill(torch.eye(t.size(0), device=t.device, dtype=torch.bool), BIG_NEG)
        return F.log_softmax(t, dim=0)   # [to, from]: every column normalised

    def _emission_log_probs_with_means(self, features, class_means):
        """Plain-torch Gaussian log density (API compatibility; the decode path uses smm_emission_f64)."""
        var = torch.diagonal(self.gaussian_cov).to(features.dtype)
        d = features.size(-1)
        z2 = ((features.unsqueeze(-2) - class_means.to(features.dtype)) ** 2 / var).sum(-1)
        return -0.5 * (d * math.log(2 * math.pi) + z2) - 0.5 * var.log().sum()

    def emission_log_probs(self, features, valid_classes, constraints):
        idx = self._merged(valid_classes).to(self.gaussian_means.device)
        elp = self._emission_log_probs_with_means(features, self.gaussian_means[idx])
        return elp if constraints is None else elp + constraints

    def _length_log_probs_with_rates(self, log_rates):
        n_classes = log_rates.size(-1)
        if self.max_k == 1:   # reference :389-391
            return torch.tensor([0.0, -1000.0], dtype=log_rates.dtype, device=log_rates.device
                                ).unsqueeze(-1).expand(2, n_classes)
        k = torch.arange(self.max_k, device=log_rates.device, dtype=log_rates.dtype).unsqueeze(-1)
        rate = torch.exp(log_rates)
        return torch.xlogy(k, rate) - rate - torch.lgamma(k + 1)   # Poisson(rate).log_prob(k); row == length

    def length_log_probs(self, valid_classes, dtype=None):
        idx = self._dev_index('merged', valid_classes, self.poisson_log_rates.device)
        rates = self.poisson_log_rates if dtype is None else self.poisson_log_rates.to(dtype)
        return self._length_log_probs_with_rates(rates[idx])

    # ------------------------------------------------------------------ dense potentials (compat only; :416-523)
    @staticmethod
    def log_hsmm(transition, emission_scores, init, length_scores, lengths, add_eos, all_batched=False,
                 allowed_ends_per_instance=None):
        """Dense ``scores[b, n, k, c_to, c_from]`` exactly as the reference defines them (memory b*N*K*C*C!)."""
        assert not all_batched, "per-instance parameter batches (compound model) are not built"
        b, n1, c1 = emission_scores.shape
        kk = min(length_scores.shape[0], n1)
        length_scores = length_scores[:kk]
        kw = dict(device=emission_scores.device, dtype=emission_scores.dtype)
        if add_eos:
            n, c = n1 + 1, c1 + 1
            trans = torch.full((b, c, c), BIG_NEG, **kw)
            trans[:, :c1, :c1] = transition
            if allowed_ends_per_instance is None:
                trans[:, c1, :] = 0
            else:
                for i, ends in enumerate(allowed_ends_per_instance):
                    assert len(ends) > 0
                    trans[i, c1, list(ends)] = 0
            ini = torch.full((b, c), BIG_NEG, **kw)
            ini[:, :c1] = init
            ls = torch.full((b, kk, c), BIG_NEG, **kw)
            ls[:, :, :c1] = length_scores
            ls[:, 1 if kk > 1 else 0, c1] = 0
            em = torch.full((b, n, c), BIG_NEG, **kw)
            for i, t in enumerate(lengths.tolist()):
                em[i, :t, :c1] = emission_scores[i, :t]
                em[i, t, c1] = 0
            lens = lengths + 1
        else:
            n, c = n1, c1
            trans = transition.unsqueeze(0).expand(b, c, c)
            ini = init.unsqueeze(0).expand(b, c)
            ls = length_scores.unsqueeze(0).expand(b, kk, c)
            em, lens = emission_scores, lengths
        scores = trans.view(b, 1, 1, c, c) + ls.view(b, 1, kk, 1, c) + torch.zeros(b, n - 1, kk, c, c, **kw)
        scores[:, 0] += ini.view(b, 1, 1, c)
        summed = None
        for k in range(1, kk):
            if summed is None:
                summed = em.clone()                          # window sums grow by one shifted copy per k
            elif k - 1 < n:
                summed[:, :n - (k - 1)] += em[:, k - 1:]
            for i in range(b):
                li = int(lens[i])
                scores[i, :li - 1, k] += summed[i, :li - 1].view(li - 1, 1, c)
                scores[i, li - 1 - k, k] += em[i, li - 1].view(c, 1)
        return scores

    def add_eos(self, spans, lengths):
        b = spans.size(0)
        aug = torch.cat([spans, torch.full([b, 1], -1, device=spans.device, dtype=torch.long)], dim=1)
        aug[torch.arange(b), lengths] = self.n_classes
        return aug

    def trim(self, spans, lengths, check_eos=False):
        return [spans[i, :lengths[i]] for i in range(spans.size(0))]

    @property
    def batched_scores(self):
        return False

    def set_z(self, features, lengths, use_mean=False):
        self.kl = torch.zeros(features.size(0), device=features.device)

    def _allowed_ends_per_instance(self, valid_classes, additional_allowed_ends_per_instance, b):
        """Local positions (in valid_classes) of allowed_ends | additional, per instance.  Reference :566-577."""
        if self.allowed_ends is None:
            return None
        vc = list(range(self.n_classes)) if valid_classes is None else [int(v) for v in valid_classes]
        if additional_allowed_ends_per_instance is None:
            additional_allowed_ends_per_instance = [set() for _ in range(b)]
        res = [[i for i, ix in enumerate(vc) if ix in (set(self.allowed_ends) | set(add))]
               for add in additional_allowed_ends_per_instance]
        assert all(res), res
        return res

    def score_features(self, features, lengths, valid_classes, add_eos, use_mean_z,
                       additional_allowed_ends_per_instance=None, constraints=None, return_elp=False):
        """Dense potentials like the reference (:553-595).  Compatibility API -- O(b*N*K*C*C) memory."""
        self.set_z(features, lengths, use_mean=use_mean_z)
        log_det = torch.zeros(features.size(0), device=features.device)
        if getattr(self, 'feature_projector', None) is not None:      # reference :560-563 (device only, like the projector)
            self._require_device(features, 'score_features')
            features = self._project(features.to(torch.float32).contiguous()).to(features.dtype)
        ends = self._allowed_ends_per_instance(valid_classes, additional_allowed_ends_per_instance, features.size(0))
        elp = self.emission_log_probs(features, valid_classes, constraints)
        scores = self.log_hsmm(self.transition_log_probs(valid_classes), elp, self.initial_log_probs(valid_classes),
                               self.length_log_probs(valid_classes), lengths, add_eos=add_eos,
                               allowed_ends_per_instance=ends)
        return (scores, log_det, elp) if return_elp else (scores, log_det)

    # ------------------------------------------------------------------ factor tables for the HIP path
    def _check_valid_classes(self, valid_classes_per_instance):
        if valid_classes_per_instance is None:
            return None
        first = valid_classes_per_instance[0]
        # (the collate hands over the task's ONE index tensor b times: identity first -- the element-wise comparison of the
        # reference, :600-601, walks every tensor in Python, 80 us of a 240 us call)
        if not all(vc is first for vc in valid_classes_per_instance):
            # ... then element-wise (one torch.equal per instance: the loader hands over equal COPIES of the task's indices),
            # and only then as sets, like the reference
            if not all(vc.shape == first.shape and torch.equal(vc, first) for vc in valid_classes_per_instance):
                assert all_equal(set(int(v) for v in vc) for vc in valid_classes_per_instance), \
                    "must have same valid_classes for all instances in the batch"
        return first.detach().cpu().long()

    def factor_tables(self, valid_classes, device=None):
        """fp64 factors of the potentials for one class set (no EOS row: the kernels handle EOS in closed form).

        Returns dict(trans C x C [to,from], init C, len K x C, w D x C, cst C, inv_var D, class_map C+1 int64).
        Built with differentiable torch ops on the parameters' device.
        """
        f64 = torch.float64
        dev = device or self.gaussian_means.device
        vc = valid_classes
        if vc is not None:      # checked on the host: an out-of-range id in a device gather is a GPU trap, not an exception
            bad = [int(v) for v in vc if not 0 <= int(v) < self.n_classes]
            if bad:
                raise IndexError("valid_classes %s outside the model's %d classes" % (bad, self.n_classes))
        idx = self._dev_index('merged', vc, dev)
        var = torch.diagonal(self.gaussian_cov).to(f64)
        mu = self.gaussian_means.to(f64)[idx]                                   # C x D
        d = mu.size(1)
        w = (mu / var).t().contiguous()                                         # D x C  (feature-major)
        cst = -0.5 * (mu * mu / var).sum(1) - 0.5 * var.log().sum() - 0.5 * d * math.log(2 * math.pi)
        ids = list(range(self.n_classes)) if vc is None else [int(v) for v in vc]
        assert len(set(ids)) == len(ids), "valid_classes must be unique"
        return dict(
            trans=self.transition_log_probs(vc, f64).contiguous(), init=self.initial_log_probs(vc, f64).contiguous(),
            len=self.length_log_probs(vc, f64).contiguous(), w=w, cst=cst.contiguous(),
            inv_var=(1.0 / var).contiguous(), class_map=self._dev_index('class_map', vc, dev))

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_table_cache', None)          # device tensors derived from the parameters: rebuilt on demand
        state.pop('_index_cache', None)
        state.pop('_endpen_cache', None)
        state.pop('_single_group', None)         # (index tensors + the ctypes shape of the table kernels)
        return state

    def _decode_tables(self, valid_classes, device):
        """factor_tables for decoding (no gradient), cached per class set: the reference decodes batch after batch with
        the same few class sets, and building the tables is a dozen small torch ops (half of a small batch's latency).
        The key includes the parameters' version counters, so any in-place update (an optimiser step, load_state_dict,
        fit_supervised) invalidates the entry."""
        key = (self._class_key(valid_classes), str(device), self.max_k, self._param_key(), self._constraint_key())
        cache = self.__dict__.setdefault('_table_cache', {})
        tab = cache.get(key)
        if tab is None:
            if len(cache) > 64:
                cache.clear()
            with torch.no_grad():
                tab = self.factor_tables(valid_classes, device)
            cache[key] = tab
        return tab

    def _hard_masks(self):
        """The tables carry -1e9 masks (--sm_constrain_transitions: allowed starts / transitions / ends): decodes ask the library
        not to split long videos along the time axis -- a unit that starts mid-video from a uniform guess ignores the masks'
        history and would not certify against the one-piece decode (profiles/round5_time_split.txt: cfg4)."""
        return (getattr(self, 'init_constraints', None) is not None or getattr(self, 'transition_constraints', None) is not None
                or self.allowed_ends is not None)

    def _param_key(self):
        """Identity + version of the five parameters: any in-place update changes it."""
        return tuple((p.data_ptr(), p._version) for p in (self.poisson_log_rates, self.gaussian_means, self.gaussian_cov,
                                                          self.transition_logits, self.init_logits))

    @staticmethod
    def _class_key(valid_classes):
        if isinstance(valid_classes, torch.Tensor):
            return tuple(valid_classes.tolist())         # (iterating a tensor costs ~1 us per element)
        return None if valid_classes is None else tuple(int(v) for v in valid_classes)

    def _constraint_key(self):
        """Identity of everything besides the five parameters that factor_tables reads."""
        ic = getattr(self, 'init_constraints', None)
        tc = getattr(self, 'transition_constraints', None)
        return (None if ic is None else (ic.data_ptr(), ic._version), None if tc is None else (tc.data_ptr(), tc._version),
                id(getattr(self, 'merge_classes', None)), bool(getattr(self, 'allow_self_transitions', True)))

    def _endpen(self, valid_classes, additional_allowed_ends_per_instance, b, c, device):
        """fp64 [b, c] end penalties on the device (0 for an allowed end state, -1e9 otherwise; reference :462-471).
        Cached per (class set, additional ends of the batch): the reference's call pattern asks for the same few
        tables batch after batch, and building one is a python loop plus a host-to-device copy."""
        if self.allowed_ends is None:
            return None
        add = additional_allowed_ends_per_instance
        key = (self._class_key(valid_classes), b, c, str(device),
               tuple(sorted(self.allowed_ends)), None if add is None else tuple(tuple(int(x) for x in a) for a in add))
        cache = self.__dict__.setdefault('_endpen_cache', {})
        hit = cache.get(key)
        if hit is not None:
            return hit
        ends = self._allowed_ends_per_instance(valid_classes, additional_allowed_ends_per_instance, b)
        ep = torch.full((b, c), BIG_NEG, dtype=torch.float64)
        for i, e in enumerate(ends):
            ep[i, e] = 0.0
        if len(cache) > 256:
            cache.clear()
        cache[key] = ep = ep.to(device)
        return ep

    @staticmethod
    def _require_device(t, what):
        if not t.is_cuda:
            raise ops._lib.SmmError("SemiMarkovModule.%s runs on the MI355X only: move the module and the batch to "
                                    "the device (--cuda); there is no CPU decode path" % what)

    # ------------------------------------------------------------------ decode (:660-696)
    def viterbi(self, features, lengths, valid_classes_per_instance, add_eos=True, use_mean_z=False,
                additional_allowed_ends_per_instance=None, constraints=None, predict_single=False, return_elp=False):
        """Viterbi segmentation of a zero-padded single-task batch.

        features b x Tmax x D (device fp32), lengths b, valid_classes_per_instance list of b identical LongTensors
        or None.  Returns pred_spans: CPU int64 b x (Tmax+1) -- global class id at every span start, -1 for a
        continuation, ``n_classes`` (EOS) at position lengths[i], -1 after it [, elp b x Tmax x C fp32 on device].
        """
        return self.viterbi_launch(features, lengths, valid_classes_per_instance, add_eos, use_mean_z,
                                   additional_allowed_ends_per_instance, constraints, predict_single, return_elp)()

    def viterbi_launch(self, features, lengths, valid_classes_per_instance, add_eos=True, use_mean_z=False,
                       additional_allowed_ends_per_instance=None, constraints=None, predict_single=False, return_elp=False,
                       slot=0, stream=None):
        """``viterbi`` in two halves: this one enqueues the decode and returns at once; calling the returned function waits
        for it and hands out what ``viterbi`` returns.  ONE launch may be outstanding per device AND ``slot`` (the spans land
        in a pinned host buffer that the next launch with the same slot reuses): a caller can collate and launch its next
        batch on the other slot in between (``SemiMarkovModel.predict(fused=False)`` does: the GPU decodes batch i + 1 while
        the host unpacks batch i).  ``stream``: decode on this stream instead of the current one (it first waits for the
        current stream, which produced the batch): a batch of five videos occupies five of 256 CUs for as long as its longest
        video takes, so batches launched on different streams decode side by side."""
        self._require_device(features, 'viterbi')
        valid_classes = self._check_valid_classes(valid_classes_per_instance)
        ctx = contextlib.nullcontext()
        if stream is not None:
            # tables that are not cached yet are built HERE, on the caller's stream, which `stream` then waits for: the
            # next batch of the same task finds them cached and may run on a third stream that waited for this point too
            self._decode_tables(valid_classes, features.device)
            stream.wait_stream(torch.cuda.current_stream(features.device))
            ctx = torch.cuda.stream(stream)
        with ctx:
            self.set_z(features, lengths, use_mean=use_mean_z)
            # (the spans land in pinned host memory, the error words follow by an asynchronous copy: ONE synchronisation, no
            # blocking device -> host copy -- this call is host latency at the reference's batch size)
            out = self._decode(features, lengths, valid_classes, additional_allowed_ends_per_instance, constraints,
                               want_elp=return_elp, want_labels=False, no_eos=not add_eos, spans_on_host=True, host_slot=slot)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(features.device))
        if stream is not None:
            for t in (features, constraints):                # (allocated on the caller's stream, read on this one)
                if t is not None and t.is_cuda:
                    t.record_stream(stream)
        tmax = features.size(1)
        b = features.size(0)

        def result():
            done.synchronize()
            pred_spans = out['spans'].clone()                  # (the pinned buffer is reused by the next launch)
            if not add_eos:
                pred_spans = pred_spans[:, :tmax].contiguous()  # b x Tmax: no EOS position (reference :679)
            ops.check_decoded(out['_batch'], out)
            if return_elp:
                return pred_spans, out['elp'].view(b, tmax, -1)
            return pred_spans
        return result

    viterbi_decode = viterbi   # name used by BASELINE.json's north star

    def decode_ragged_launch(self, feature_list, lengths, valid_classes_per_instance, additional_allowed_ends_per_instance=None,
                             slot=0, stream=None):
        """One single-task batch of the reference's call pattern WITHOUT its padded layout (round 5): ``feature_list`` holds
        the videos' own T_i x D device tensors, the decode runs on their concatenation (one gather instead of ``pad_sequence``'s
        zero fill + b copies) and hands back FRAME LABELS -- what ``predict`` makes of ``viterbi``'s spans with
        ``spans_to_labels`` + ``trim`` (reference semimarkov.py:397-409) is what the DP kernel writes anyway.  The batch keeps
        its one batch-dependent quantity, K clipped to its longest video (:450-452).  Returns at once; calling the result
        waits and gives the list of int64 numpy label arrays (views of a pinned buffer that the next launch with the same
        ``slot`` reuses: copy what you keep).  ``stream``: as in ``viterbi_launch``."""
        x0 = feature_list[0]
        self._require_device(x0, 'decode_ragged_launch')
        valid_classes = self._check_valid_classes(valid_classes_per_instance)
        dev = x0.device
        lengths_host = lengths.detach().cpu().numpy().astype(np.int64)
        b, d, tmax, total = len(feature_list), x0.size(1), int(lengths_host.max()), int(lengths_host.sum())
        ctx = contextlib.nullcontext()
        if stream is not None:
            self._decode_tables(valid_classes, dev)           # (built on the caller's stream: see viterbi_launch)
            stream.wait_stream(torch.cuda.current_stream(dev))
            ctx = torch.cuda.stream(stream)
        with ctx:
            self.kl = torch.zeros(b, device=dev)
            tab = self._decode_tables(valid_classes, dev)
            c = tab['init'].numel()
            off = np.concatenate([[0], np.cumsum(lengths_host)[:-1]])
            batch = ops.Batch(lengths_host, [c], tab['len'].size(0), c_max=c, t_max=tmax, total_frames=total, d=d,
                              frame_offset=off, kp=[min(tab['len'].size(0), tmax)] * b, no_time_split=self._hard_masks())
            x = torch.cat([f.detach().to(torch.float32) for f in feature_list]) if b > 1 else x0.detach().to(torch.float32).contiguous()
            with torch.no_grad():
                x = self._project(x)                          # (the third place features meet the scorer: this decode stages itself)
            endpen = self._endpen(valid_classes, additional_allowed_ends_per_instance, b, c, dev)
            g1 = _one_group(tab)
            labels = ops.pinned_labels(('ragged', slot), dev, total)
            out = ops.decode(batch, x, g1[0], g1[1], tab['inv_var'], g1[2], g1[3], g1[4], endpen=endpen, class_map=g1[5],
                             want_spans=False, want_labels=True, labels_out=labels, spans_on_host=True, host_slot=('ragged', slot))
            out['_keep'] = (tab, g1, endpen, x)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))
        if stream is not None:
            for f in feature_list:
                f.record_stream(stream)

        def result():
            done.synchronize()
            ops.check_decoded(batch, out)
            lab = labels.numpy()
            return [lab[o:o + t] for o, t in zip(off.tolist(), lengths_host.tolist())]
        return result

    @staticmethod
    def _check_no_eos_lengths(lengths_host, no_eos):
        if no_eos and int(lengths_host.min()) < 2:
            raise ValueError("add_eos=False needs at least two frames per video (a one-frame video has no edge at all "
                             "in the reference's lattice)")

    def _stage_padded(self, features, lengths, valid_classes, additional_allowed_ends_per_instance, constraints, no_eos=False,
                      no_time_split=False, check_no_eos=True, tables=None, projected=False):
        """A zero-padded single-task batch as the launchers take it -> (batch, x, cons, endpen, tab, g1): the ``ops.Batch``, the
        features fp32 [b * Tmax, D], the constraints fp32 [b * Tmax, C] or None, the end penalties (None with ``no_eos``), the
        factor tables and their stack of one group.
        ``no_time_split``: ``self._hard_masks()`` from the callers that ask the library to decode long videos in one piece.
        ``check_no_eos``: False from ``align``, which refuses add_eos=False itself and stages with ``no_eos`` off.
        ``tables``: the stacked differentiable tables of ``log_partition`` instead of the decode cache's (``g1`` is None then)."""
        b, tmax, d = features.shape
        dev = features.device
        lengths_host = lengths.detach().cpu().numpy().astype(np.int64)
        spans_tmax = int(lengths_host.max()) == tmax
        if tables is None:
            assert spans_tmax, "one instance must span the padded length (padding_colate)"
        assert spans_tmax                               # (log_partition: without a message)
        if check_no_eos:
            self._check_no_eos_lengths(lengths_host, no_eos)
        tab = self._decode_tables(valid_classes, dev) if tables is None else tables
        c = tab['init'].numel()
        batch = ops.Batch(lengths_host, [c], tab['len'].size(-2), c_max=c, t_max=tmax, total_frames=b * tmax, d=d, no_eos=no_eos,
                          no_time_split=no_time_split)
        # The likelihoods (``tables``: theirs, with autograd history) give their features a gradient (smm_emission_bwd_x_f64): the
        # projection then carries the flow's autograd node, and features that ask for a gradient themselves -- another module's
        # output -- keep theirs.  Every other entry point computes values: no node, nothing kept alive.
        if tables is not None and torch.is_grad_enabled():
            x = self._project((features if features.requires_grad else features.detach()).to(torch.float32).contiguous()
                              .view(b * tmax, d), projected)
        else:
            with torch.no_grad():
                x = self._project(features.detach().to(torch.float32).contiguous().view(b * tmax, d), projected)
        cons = None
        if constraints is not None:
            cons = constraints.detach().to(device=dev, dtype=torch.float32).contiguous().view(b * tmax, c)
        endpen = None if no_eos else self._endpen(valid_classes, additional_allowed_ends_per_instance, b, c, dev)
        return batch, x, cons, endpen, tab, _one_group(tab) if tables is None else None

    def _decode(self, features, lengths, valid_classes, additional_allowed_ends_per_instance, constraints,
                want_elp=False, want_labels=True, want_spans=True, no_eos=False, spans_on_host=False, host_slot=0):
        batch, x, cons, endpen, tab, g1 = self._stage_padded(features, lengths, valid_classes,
                                                             additional_allowed_ends_per_instance, constraints, no_eos=no_eos,
                                                             no_time_split=self._hard_masks())
        out = ops.decode(batch, x, g1[0], g1[1], tab['inv_var'], g1[2], g1[3], g1[4], cons=cons, endpen=endpen,
                         class_map=g1[5], want_spans=want_spans, want_labels=want_labels,
                         want_elp=want_elp, spans_on_host=spans_on_host, host_slot=host_slot)
        out['_batch'] = batch
        # the cached tables and end penalties are read by kernels that may run on a side stream (viterbi_launch) long after
        # this call has returned, and the caches evict (`cache.clear()` above 64 / 256 entries): the pending result keeps what
        # its launch reads alive until the caller has synchronised on it
        out['_keep'] = (tab, g1, endpen, x, cons)
        return out

    # ------------------------------------------------------------------ posterior samples and marginals (smm_sample_f64)
    def _posterior_launch(self, features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
                          constraints, what, with_backward=False):
        """emission + log Z of a zero-padded single-task batch on a private workspace -> the record of ``_emit_logz``:
        dict(batch, elp, tables as one group, class_map, endpen, logz, ws, x)."""
        self._require_device(features, what)
        batch, x, cons, endpen, tab, g1 = self._stage_padded(
            features, lengths, self._check_valid_classes(valid_classes_per_instance), additional_allowed_ends_per_instance,
            constraints, no_eos=not add_eos, no_time_split=self._hard_masks())
        return _emit_logz(batch, x, cons, endpen, g1, tab['inv_var'], with_backward)

    @torch.no_grad()
    def sample(self, features, lengths, valid_classes_per_instance, n_samples=1, seed=0, add_eos=True,
               additional_allowed_ends_per_instance=None, constraints=None):
        """Segmentations drawn from the posterior p(y | x) of a zero-padded single-task batch (argument conventions of
        ``viterbi``): one emission launch, one log Z launch, one sampling launch.  Sample j depends on (seed, video, j) only.

        Returns (spans, log_prob): spans CPU int64 n_samples x b x (Tmax+1) in ``viterbi``'s pred_spans format (n_samples x b x
        Tmax with add_eos=False, as ``viterbi`` then returns), log_prob fp64 n_samples x b on the device: the exact
        log p(spans | x) of each sample.  No autograd."""
        r = self._posterior_launch(features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
                                   constraints, 'sample')
        return _sample(r, n_samples, seed, want_spans=True)

    @torch.no_grad()
    def frame_posteriors(self, features, lengths, valid_classes_per_instance, add_eos=True,
                         additional_allowed_ends_per_instance=None, constraints=None):
        """Posterior class occupancy of every frame, P(frame t has label c | x): fp64 b x Tmax x C on the device, columns in
        the order of the batch's valid classes (0 on padded frames).  The d log Z / d elp of smm_logz_bwd_f64 -- what the
        label frequencies of ``sample`` converge to."""
        r = self._posterior_launch(features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
                                   constraints, 'frame_posteriors')
        b, tmax = features.shape[:2]
        return _marginals(r).view(b, tmax, -1)

    def entropy(self, features, lengths, valid_classes_per_instance, add_eos=True, additional_allowed_ends_per_instance=None,
                constraints=None, *, differentiable=False):
        """Exact entropy H(y | x) = -sum_y p(y | x) log p(y | x) of each video's segmentation posterior, in nats: fp64 b on the
        device (argument conventions of ``viterbi``).  One emission launch, one log Z launch (forward and time-reversed), one
        entropy launch (smm_entropy_f64); the value keeps its relative accuracy on confident videos (H -> 0).  Raises
        SmmError when a NaN reached the DP.
        ``differentiable``: the same value (bit for bit), differentiable with respect to the module's parameters: the backward
        runs smm_entropy_bwd_f64 and the chain rule through the emission scorer and the factor tables (``log_partition``'s)."""
        launch = lambda: _entropy(self._posterior_launch(
            features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance, constraints, 'entropy',
            with_backward=True), with_backward=True)
        if not differentiable:
            with torch.no_grad():
                return launch()[0]
        self._require_device(features, 'entropy')
        self._no_projected_gradient()
        tabs = self._differentiable_tables(self._check_valid_classes(valid_classes_per_instance), features.device)
        return _PosteriorValue.apply('entropy', launch, *tabs)

    def _packed_stage(self, pc, what, differentiable=False):
        """``_stage_padded`` for a PackedCorpus, prepared for this module here: (batch, x, cons, endpen, tables stacked per
        group, inv_var) -- the arguments of ``_emit`` / ``_emit_logz``.  ``differentiable``: tables with autograd history."""
        self._require_device(pc.x, what)
        self.prepare_packed(pc, differentiable)
        t = pc.tables
        return pc.batch, self._project_packed(pc, pc.x, differentiable), pc.cons, pc.endpen, tuple(t[k] for k in TABLE_NAMES) + (t['class_map'],), t['inv_var']

    def _packed_posterior_launch(self, pc, what, with_backward=False):
        return _emit_logz(*self._packed_stage(pc, what), with_backward)

    @torch.no_grad()
    def sample_packed(self, pc, n_samples, seed=0):
        """``sample`` for a whole PackedCorpus: one emission launch, one smm_logz_f64 and one sampling launch.
        Returns (labels, log_prob): device int64 n_samples x total_frames (global class ids on the packed frame axis) and fp64
        n_samples x n_videos in the order of ``pc.video_names``."""
        return _sample(self._packed_posterior_launch(pc, 'sample_packed'), n_samples, seed, want_spans=False)

    @torch.no_grad()
    def frame_posteriors_packed(self, pc):
        """``frame_posteriors`` for a whole PackedCorpus: fp64 total_frames x c_max on the device; column c of a frame is local
        state c of its video's group (``pc.tables['class_map']`` maps it to a global id)."""
        return _marginals(self._packed_posterior_launch(pc, 'frame_posteriors_packed'))

    def entropy_packed(self, pc, *, differentiable=False):
        """``entropy`` for a whole PackedCorpus: fp64 n_videos on the device, in the order of ``pc.video_names``.
        ``differentiable``: as ``entropy``'s; the tables are ``stacked_tables(pc, differentiable=True)``."""
        launch = lambda: _entropy(self._packed_posterior_launch(pc, 'entropy_packed'), with_backward=False)
        if not differentiable:
            with torch.no_grad():
                return launch()[0]
        self._require_device(pc.x, 'entropy_packed')
        self._no_projected_gradient()
        st = self.stacked_tables(pc, differentiable=True)[0]
        return _PosteriorValue.apply('entropy', launch, *(st[k] for k in TABLE_NAMES))

    # ------------------------------------------------------------------ expected reward (smm_expected_reward_f64)
    def expected_reward(self, features, lengths, valid_classes_per_instance, reward=None, seg_reward=None, add_eos=True,
                        additional_allowed_ends_per_instance=None, constraints=None, *, differentiable=False):
        """Posterior expectation E_{p(y | x)}[R(y)] of a reward that is additive over frames and segments, exactly: fp64 b on the
        device (argument conventions of ``viterbi``).  R(y) = sum over the segments (class c) of y of seg_reward[c] + the sum
        of reward[t, c] over the segment's frames.  ``reward``: b x Tmax x C, columns in the order of the batch's valid classes
        (the layout ``frame_posteriors`` returns; padded frames are ignored); ``seg_reward``: length C; either may be None.
        reward = one-hot labels: the expected number of correct frames (``expected_accuracy``); seg_reward = 1: the expected
        number of segments (``expected_segment_count``); reward[:, :, c] = 1: the expected time in class c.  One emission
        launch, one log Z launch (forward and time-reversed), one smm_expected_reward_f64 launch.  Raises SmmError when a NaN
        reached the DP or a reward is not finite.
        ``differentiable``: the same value (bit for bit), differentiable with respect to the module's parameters (not the
        rewards: one that requires grad is refused): the backward runs smm_expected_reward_bwd_f64, a Hessian-vector product
        of log Z, and the chain rule through the emission scorer and the factor tables (``log_partition``'s)."""
        self._require_device(features, 'expected_reward')
        b, tmax = features.shape[:2]
        dev = features.device
        vc = self._check_valid_classes(valid_classes_per_instance)
        c = self.n_classes if vc is None else int(vc.numel())
        rw = _reward_tensor(reward, (b, tmax, c), dev, 'reward')
        sg = _reward_tensor(seg_reward, (c,), dev, 'seg_reward')
        if rw is None and sg is None:
            raise ValueError("expected_reward: at least one of reward and seg_reward is needed")
        rw = None if rw is None else rw.view(b * tmax, c)
        sg = None if sg is None else sg.view(1, c)
        launch = lambda: _expected_reward(self._posterior_launch(
            features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance, constraints,
            'expected_reward', with_backward=True), rw, sg, with_backward=True)
        if not differentiable:
            with torch.no_grad():
                return launch()[0]
        self._no_projected_gradient()
        return _PosteriorValue.apply('expected_reward', launch, *self._differentiable_tables(vc, dev))

    def expected_reward_packed(self, pc, reward=None, seg_reward=None, *, differentiable=False):
        """``expected_reward`` for a whole PackedCorpus: fp64 n_videos on the device, in the order of ``pc.video_names``.
        ``reward``: total_frames x c_max on local states (the layout of ``frame_posteriors_packed``), ``seg_reward``:
        n_groups x c_max.  ``differentiable``: as ``expected_reward``'s; the tables are ``stacked_tables(pc,
        differentiable=True)``."""
        self._require_device(pc.x, 'expected_reward_packed')
        self.prepare_packed(pc)
        batch = pc.batch
        rw = _reward_tensor(reward, (batch.total_frames, batch.c_max), pc.x.device, 'reward')
        sg = _reward_tensor(seg_reward, (batch.n_groups, batch.c_max), pc.x.device, 'seg_reward')
        if rw is None and sg is None:
            raise ValueError("expected_reward_packed: at least one of reward and seg_reward is needed")
        launch = lambda: _expected_reward(self._packed_posterior_launch(pc, 'expected_reward_packed'), rw, sg, with_backward=False)
        if not differentiable:
            with torch.no_grad():
                return launch()[0]
        self._no_projected_gradient()
        st = self.stacked_tables(pc, differentiable=True)[0]
        return _PosteriorValue.apply('expected_reward', launch, *(st[k] for k in TABLE_NAMES))

    def expected_accuracy(self, features, lengths, valid_classes_per_instance, labels, add_eos=True,
                          additional_allowed_ends_per_instance=None, constraints=None, normalize=False, *, differentiable=False):
        """Expected number of frames of each video on which a segmentation drawn from p(y | x) agrees with ``labels`` (b x Tmax,
        GLOBAL class ids; padded frames are ignored; an id outside the batch's class set, or a negative one, is never
        correct): fp64 b on the device; with ``normalize`` the fraction of the video's frames.  ``expected_reward`` with
        reward = one-hot(labels): the quantity ``mbr_decode`` maximises over segmentations, here as a training signal for
        the given labels (``differentiable``) or as a quality estimate of a decode."""
        self._require_device(features, 'expected_accuracy')
        dev = features.device
        onehot = self._onehot_labels(features, valid_classes_per_instance, labels)
        v = self.expected_reward(features, lengths, valid_classes_per_instance, reward=onehot, add_eos=add_eos,
                                 additional_allowed_ends_per_instance=additional_allowed_ends_per_instance,
                                 constraints=constraints, differentiable=differentiable)
        return v / lengths.to(device=dev, dtype=torch.float64) if normalize else v

    def expected_accuracy_packed(self, pc, labels, normalize=False, *, differentiable=False):
        """``expected_accuracy`` for a whole PackedCorpus.  ``labels``: int64 total_frames, global class ids on the packed frame
        axis (what ``decode_packed`` returns); fp64 n_videos in the order of ``pc.video_names``."""
        self._require_device(pc.x, 'expected_accuracy_packed')
        self.prepare_packed(pc)
        batch, dev = pc.batch, pc.x.device
        v = self.expected_reward_packed(pc, reward=self._onehot_labels_packed(pc, labels), differentiable=differentiable)
        return v / torch.as_tensor(batch.lengths, device=dev).to(torch.float64) if normalize else v

    def _onehot_labels(self, features, valid_classes_per_instance, labels):
        """``labels`` (b x Tmax, GLOBAL class ids) as a reward: fp64 b x Tmax x C, 1 where the frame's label is the column's
        class; an id outside the batch's class set, or a negative one, matches no column."""
        dev = features.device
        vc = self._check_valid_classes(valid_classes_per_instance)
        ids = self._decode_tables(vc, dev)['class_map']
        c = self.n_classes if vc is None else int(vc.numel())
        lab = torch.as_tensor(labels).to(device=dev, dtype=torch.int64)
        if tuple(lab.shape) != tuple(features.shape[:2]):
            raise ValueError("labels: shape %s expected, got %s" % (tuple(features.shape[:2]), tuple(lab.shape)))
        return ((lab.unsqueeze(-1) == ids[:c].view(1, 1, c)) & (lab.unsqueeze(-1) >= 0)).to(torch.float64)

    @staticmethod
    def _onehot_labels_packed(pc, labels):
        """``labels`` (int64 total_frames, GLOBAL class ids on the packed frame axis of a prepared corpus) as a reward: fp64
        total_frames x c_max on local states; frames no video covers match no column."""
        batch, dev = pc.batch, pc.x.device
        lab = torch.as_tensor(labels).to(device=dev, dtype=torch.int64)
        if tuple(lab.shape) != (batch.total_frames,):
            raise ValueError("labels: shape %s expected, got %s" % ((batch.total_frames,), tuple(lab.shape)))
        group = np.zeros(batch.b, dtype=np.int64) if batch.group is None else batch.group.astype(np.int64)
        cmap = pc.tables['class_map'][:, :batch.c_max]                         # n_groups x c_max global ids
        live = torch.arange(batch.c_max, device=dev).view(1, -1) < torch.as_tensor(batch.n_states, device=dev).view(-1, 1)
        frame_group = torch.zeros(batch.total_frames, dtype=torch.int64, device=dev)
        covered = torch.zeros(batch.total_frames, dtype=torch.bool, device=dev)
        for off, t, g in zip(batch.frame_offset.tolist(), batch.lengths.tolist(), group.tolist()):
            frame_group[off:off + t] = g
            covered[off:off + t] = True
        onehot = (lab.view(-1, 1) == cmap[frame_group]) & live[frame_group] & (lab.view(-1, 1) >= 0) & covered.view(-1, 1)
        return onehot.to(torch.float64)

    def expected_segment_count(self, features, lengths, valid_classes_per_instance, add_eos=True,
                               additional_allowed_ends_per_instance=None, constraints=None, *, differentiable=False):
        """Expected number of segments of each video under p(y | x): fp64 b on the device.  ``expected_reward`` with
        seg_reward = 1 -- differentiable, it is an over-segmentation penalty.  With add_eos=False the closing label of the last
        frame counts as a segment (``segment_posteriors``' convention)."""
        vc = self._check_valid_classes(valid_classes_per_instance)
        c = self.n_classes if vc is None else int(vc.numel())
        return self.expected_reward(features, lengths, valid_classes_per_instance,
                                    seg_reward=torch.ones(c, dtype=torch.float64, device=features.device), add_eos=add_eos,
                                    additional_allowed_ends_per_instance=additional_allowed_ends_per_instance,
                                    constraints=constraints, differentiable=differentiable)

    def expected_segment_count_packed(self, pc, *, differentiable=False):
        """``expected_segment_count`` for a whole PackedCorpus: fp64 n_videos in the order of ``pc.video_names``."""
        self._require_device(pc.x, 'expected_segment_count_packed')
        self.prepare_packed(pc)
        ones = torch.ones((pc.batch.n_groups, pc.batch.c_max), dtype=torch.float64, device=pc.x.device)
        return self.expected_reward_packed(pc, seg_reward=ones, differentiable=differentiable)

    # ------------------------------------------------------------------ segment and boundary posteriors (smm_segment_posteriors_f64)
    @torch.no_grad()
    def segment_posteriors(self, features, lengths, valid_classes_per_instance, spans=None, add_eos=True,
                           additional_allowed_ends_per_instance=None, constraints=None):
        """How sure the posterior is of each segment of ``spans`` and of each boundary, exactly (argument conventions of
        ``viterbi``).  ``spans``: b x (Tmax+1) or n_sets x b x (Tmax+1) in ``viterbi``'s pred_spans format (Tmax columns with
        add_eos=False), on any device; None: the Viterbi decode.  One emission launch, one log Z launch (forward and
        time-reversed), one smm_segment_posteriors_f64 launch.

        Returns a dict of device tensors: ``seg_logp`` fp64 shaped like the spans (Tmax+1 columns): at each span start the log
        posterior that exactly this segment -- class, start, end -- is part of the segmentation, 0 at the EOS position, -inf
        elsewhere and for a segment the lattice does not have; ``start`` / ``end`` fp64 b x Tmax x C: P(a span of class c starts
        at / has as its last frame the frame), columns in the order of the batch's valid classes; ``boundary`` fp64 b x Tmax:
        P(a span starts at the frame); ``spans`` int64: the segmentations ``seg_logp`` speaks of.  Padded frames are 0.  Raises
        SmmError when a NaN reached the DP.  Values, not differentiable."""
        r = self._posterior_launch(features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
                                   constraints, 'segment_posteriors', with_backward=True)
        out = _segment_posteriors(r, spans, with_backward=True)
        b, tmax = features.shape[:2]
        out['start'], out['end'] = out['start'].view(b, tmax, -1), out['end'].view(b, tmax, -1)
        out['boundary'] = out['boundary'].view(b, tmax)
        return out

    @torch.no_grad()
    def segment_posteriors_packed(self, pc, spans=None):
        """``segment_posteriors`` for a whole PackedCorpus.  ``spans``: int64 n_videos x (t_max+1) or n_sets x n_videos x
        (t_max+1) in the span encoding ``decode_packed(want_spans=True)`` returns, videos in the order of ``pc.video_names``;
        None: the Viterbi decode of ``pc``.  ``start`` / ``end`` are fp64 total_frames x c_max and ``boundary`` fp64
        total_frames on the packed frame axis; column c of a frame is local state c of its video's group
        (``pc.tables['class_map']`` maps it to a global id).  Values, not differentiable."""
        return _segment_posteriors(self._packed_posterior_launch(pc, 'segment_posteriors_packed'), spans, with_backward=False)

    @torch.no_grad()
    def boundary_posteriors(self, features, lengths, valid_classes_per_instance, add_eos=True,
                            additional_allowed_ends_per_instance=None, constraints=None):
        """P(a segment starts at the frame | x), exactly: fp64 b x Tmax on the device (1 at frame 0, 0 on padded frames).
        Argument conventions of ``viterbi``; the launches of ``segment_posteriors``.  Values, not differentiable."""
        r = self._posterior_launch(features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
                                   constraints, 'boundary_posteriors', with_backward=True)
        return _segment_posteriors(r, None, with_backward=True, want_spans=False)['boundary'].view(features.shape[:2])

    @torch.no_grad()
    def boundary_posteriors_packed(self, pc):
        """``boundary_posteriors`` for a whole PackedCorpus: fp64 total_frames on the packed frame axis."""
        return _segment_posteriors(self._packed_posterior_launch(pc, 'boundary_posteriors_packed'), None, with_backward=False,
                                   want_spans=False)['boundary']

    # ------------------------------------------------------------------ KL divergence and cross-entropy (smm_kl_f64)
    def _check_same_lattice(self, other, what):
        if not isinstance(other, SemiMarkovModule):
            raise TypeError("%s: other must be a SemiMarkovModule" % what)
        mine = (self.n_classes, self.input_feature_dim, self.max_k)
        theirs = (other.n_classes, other.input_feature_dim, other.max_k)
        if mine != theirs:
            raise ValueError("%s: the two posteriors must share the lattice: (n_classes, n_dims, max_k) %s against %s"
                             % (what, mine, theirs))

    @staticmethod
    def _check_same_batch(bp, bq, what):
        same = (bp.c_max == bq.c_max and bp.k_rows == bq.k_rows and bp.no_eos == bq.no_eos
                and np.array_equal(bp.lengths, bq.lengths) and np.array_equal(bp.n_states, bq.n_states)
                and np.array_equal(bp.frame_offset, bq.frame_offset)
                and (bp.kp is None) == (bq.kp is None) and (bp.kp is None or np.array_equal(bp.kp, bq.kp))
                and (bp.group is None) == (bq.group is None) and (bp.group is None or np.array_equal(bp.group, bq.group)))
        if not same:
            raise ValueError("%s: the two posteriors' batches differ (states, span limit or lengths)" % what)

    def _kl(self, other, features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
            constraints, other_constraints, what, want_cross_entropy):
        self._check_same_lattice(other, what)
        q = other._posterior_launch(features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
                                    other_constraints, what)
        r = self._posterior_launch(features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
                                   constraints, what, with_backward=True)
        return _kl(r, q, what, True, want_cross_entropy)

    def _kl_value(self, other, args, what, want_cross_entropy, differentiable):
        if not differentiable:
            with torch.no_grad():
                return self._kl(other, *args, what, want_cross_entropy)[0]
        self._check_same_lattice(other, what)
        features = args[0]
        self._require_device(features, what)
        valid = self._check_valid_classes(args[2])
        self._no_projected_gradient(other)
        tabs = self._differentiable_tables(valid, features.device) + other._differentiable_tables(valid, features.device)
        return _PosteriorValue.apply(what, lambda: self._kl(other, *args, what, want_cross_entropy), *tabs)

    def kl_divergence(self, other, features, lengths, valid_classes_per_instance, add_eos=True,
                      additional_allowed_ends_per_instance=None, constraints=None, other_constraints=None, *,
                      differentiable=False):
        """Exact KL(p || q) = sum_y p(y | x) log(p(y | x) / q(y | x)) per video, in nats: fp64 b on the device (argument
        conventions of ``viterbi``).  p is this module's posterior under ``constraints``, q is ``other``'s under
        ``other_constraints`` (``other`` may be ``self``); each side builds its tables, emissions and end penalties from its own
        parameters and allowed ends.  Two emission launches, two log Z launches (p's forward and time-reversed), one KL launch
        (smm_kl_f64); the value keeps its relative accuracy as q -> p and is exactly 0 for the same inputs.  +inf where q gives
        probability 0 to a segmentation p does not.  Raises ValueError when the two modules' lattices differ (n_classes,
        n_dims, max_k), SmmError when a NaN reached the DP.
        ``differentiable``: the same value (bit for bit), differentiable with respect to both modules' parameters: p's side by
        smm_kl_bwd_f64, q's as mu_q - mu_p (two smm_logz_bwd_f64); a video whose KL is +inf gets NaN gradients."""
        args = (features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance, constraints,
                other_constraints)
        return self._kl_value(other, args, 'kl_divergence', False, differentiable)

    def cross_entropy(self, other, features, lengths, valid_classes_per_instance, add_eos=True,
                      additional_allowed_ends_per_instance=None, constraints=None, other_constraints=None, *,
                      differentiable=False):
        """Exact cross-entropy H(p, q) = -sum_y p(y | x) log q(y | x) = H(p) + KL(p || q) per video, in nats: fp64 b on the
        device.  Arguments and launches as ``kl_divergence``; with ``other`` = ``self`` and the same constraints it is
        ``entropy``'s value.  ``differentiable``: as ``kl_divergence``'s."""
        args = (features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance, constraints,
                other_constraints)
        return self._kl_value(other, args, 'cross_entropy', True, differentiable)

    def _kl_packed(self, other, pc, what, want_cross_entropy):
        self._check_same_lattice(other, what)
        # q first, on a copy of the corpus' cached state that is put back afterwards: prepare_packed keeps one module's
        # tables, end penalties and launch metadata on the corpus, and `pc` is left prepared for `self`
        saved = dict(pc.__dict__)
        try:
            q = other._packed_posterior_launch(pc, what)
        finally:
            pc.__dict__.clear()
            pc.__dict__.update(saved)
        return _kl(self._packed_posterior_launch(pc, what), q, what, False, want_cross_entropy)[0]

    @torch.no_grad()
    def kl_packed(self, other, pc):
        """``kl_divergence`` for a whole PackedCorpus: fp64 n_videos on the device, in the order of ``pc.video_names``.  q's
        stacked tables and end penalties are built on ``pc``'s layout; ``pc`` is left prepared for ``self``."""
        return self._kl_packed(other, pc, 'kl_packed', False)

    @torch.no_grad()
    def cross_entropy_packed(self, other, pc):
        """``cross_entropy`` for a whole PackedCorpus: fp64 n_videos on the device, in the order of ``pc.video_names``."""
        return self._kl_packed(other, pc, 'cross_entropy_packed', True)

    # ------------------------------------------------------------------ the k best segmentations (smm_kbest_f64)
    @torch.no_grad()
    def viterbi_kbest(self, features, lengths, valid_classes_per_instance, k, add_eos=True,
                      additional_allowed_ends_per_instance=None, constraints=None):
        """The k highest-scoring segmentations of a zero-padded single-task batch (argument conventions of ``viterbi``): one
        emission launch, one k-best launch.  Rank 0 is the Viterbi segmentation (up to ties within rounding).

        Returns (spans, scores): spans CPU int64 k x b x (Tmax+1) in ``viterbi``'s pred_spans format (k x b x Tmax with
        add_eos=False), scores fp64 k x b on the device, non-increasing over the ranks (two scores within rounding of each
        other may come in either order).  A video with fewer than k segmentations gets score -inf and a row of -1 on the ranks
        past its last.  No autograd."""
        self._require_device(features, 'viterbi_kbest')
        # (no_time_split stays off on this entry point, hard masks or not)
        batch, x, cons, endpen, tab, g1 = self._stage_padded(
            features, lengths, self._check_valid_classes(valid_classes_per_instance), additional_allowed_ends_per_instance,
            constraints, no_eos=not add_eos)
        return _kbest(_emit(batch, x, cons, endpen, g1, tab['inv_var']), k, want_spans=True)

    @torch.no_grad()
    def kbest_packed(self, pc, k):
        """``viterbi_kbest`` for a whole PackedCorpus: one emission launch and one k-best launch.  Returns (labels, scores):
        device int64 k x total_frames (global class ids on the packed frame axis) and fp64 k x n_videos in the order of
        ``pc.video_names``."""
        return _kbest(_emit(*self._packed_stage(pc, 'kbest_packed')), k, want_spans=False)

    # ------------------------------------------------------------------ minimum-Bayes-risk decode (smm_mbr_f64)
    @torch.no_grad()
    def mbr_decode(self, features, lengths, valid_classes_per_instance, add_eos=True, additional_allowed_ends_per_instance=None,
                   constraints=None):
        """The segmentation with the most expected correct frames (minimum-Bayes-risk decode under frame loss) of a zero-padded
        single-task batch (argument conventions of ``viterbi``): among the segmentations the posterior gives non-zero mass, the
        one that maximises sum_t P(y_t = label_t | x).  Unlike the per-frame argmax of ``frame_posteriors`` it obeys the span
        limit, the transition, start and end constraints and the narration masks.  One emission launch, one log Z launch
        (forward and time-reversed), one marginals launch (smm_logz_bwd_f64), one MBR launch (smm_mbr_f64).

        Returns (pred_spans, expected_correct): pred_spans CPU int64 b x (Tmax+1) in ``viterbi``'s format (b x Tmax with
        add_eos=False), expected_correct fp64 b on the device: sum_t P(y_t = label_t | x) along the result.  Raises SmmError
        when a NaN reached the DP.  No autograd."""
        r = self._posterior_launch(features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
                                   constraints, 'mbr_decode', with_backward=True)
        return _mbr(r, want_spans=True)

    @torch.no_grad()
    def mbr_decode_packed(self, pc):
        """``mbr_decode`` for a whole PackedCorpus: one emission, one log Z (both directions), one marginals and one MBR launch.
        Returns (labels, expected_correct): device int64 total_frames (global class ids on the packed frame axis, -1 on frames
        no video covers) and fp64 n_videos in the order of ``pc.video_names``."""
        return _mbr(self._packed_posterior_launch(pc, 'mbr_decode_packed', with_backward=True), want_spans=False)

    # ------------------------------------------------------------------ the transcript family: its supervision, staged
    @staticmethod
    def _local_ids(class_map_host, n_states, group):
        """Per video the look-up GLOBAL class id -> local state id: the position of the id among the video's valid classes."""
        lookup = [{int(c): j for j, c in reversed(list(enumerate(class_map_host[g, :n_states[g]])))} for g in range(len(n_states))]
        return [lookup[int(g)] for g in group]

    @staticmethod
    def _local_transcripts(transcripts, class_map_host, n_states, group):
        """Transcripts in GLOBAL class ids -> local state ids: the position of each id among its video's valid classes."""
        if len(transcripts) != len(group):
            raise ValueError("align: %d transcripts for %d videos" % (len(transcripts), len(group)))
        out = []
        for i, (t, lk) in enumerate(zip(transcripts, SemiMarkovModule._local_ids(class_map_host, n_states, group))):
            ids = np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.int64).reshape(-1)
            if ids.size == 0:
                raise ValueError("align: the transcript of video %d is empty" % i)
            bad = [int(c) for c in ids if int(c) not in lk]
            if bad:
                raise ValueError("align: class %d in the transcript of video %d is not a valid class of that video" % (bad[0], i))
            out.append(np.array([lk[int(c)] for c in ids], np.int64))
        return out

    @staticmethod
    def _local_graphs(graphs, class_map_host, n_states, group):
        """Graphs in GLOBAL class ids -> local state ids, as ``_local_transcripts`` maps transcripts; a class that is no valid
        class of the video becomes -1, which leaves that video without an alignment."""
        if len(graphs) != len(group):
            raise ValueError("align_graph: %d graphs for %d videos" % (len(graphs), len(group)))
        return [gr.with_ids([lk.get(int(c), -1) for c in gr.ids])
                for gr, lk in zip(graphs, SemiMarkovModule._local_ids(class_map_host, n_states, group))]

    @staticmethod
    def _checked_supervision(given, optional, graphs, n_videos, ambiguous, names, what):
        """What supervises a launch -- transcripts (with ``optional``: one boolean sequence each) or ``graphs`` --, checked on
        the host -> (given, optional).  ``ambiguous``: 'raise' / 'allow' from the likelihoods and the sampler
        (``_checked_graphs`` / ``_checked_optional``); None from the alignments, which hand flags and graphs to the launcher as
        they came."""
        if ambiguous is not None and graphs:
            given = _checked_graphs(given, n_videos, ambiguous, names, what)
        elif ambiguous is not None and optional is not None:
            optional = _checked_optional(given, optional, ambiguous, names, what)
        return given, optional

    def _local_supervision(self, given, optional, graphs, class_map_host, n_states, group):
        """The same in LOCAL state ids, as the launch helpers take it (``_TRANSCRIPT_OPS``)."""
        if graphs:
            return 'graph', (self._local_graphs(given, class_map_host, n_states, group),)
        local = self._local_transcripts(given, class_map_host, n_states, group)
        return ('chain', (local,)) if optional is None else ('optional', (local, optional))

    def _supervised_padded(self, what, features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
                           constraints, given, optional=None, graphs=False, ambiguous=None, differentiable=False, projected=False):
        """Stage a transcript-family launch on a zero-padded single-task batch -> (the record of ``_emit``, supervision); with
        ``differentiable`` the first is (batch, x, cons, endpen, tables with autograd history, inv_var) for
        ``_alignment_log_partition``, which emits itself.  Every check on the host comes before a device is touched.  (Staged
        without no_time_split and, add_eos=False being refused, without the length check.)"""
        if not add_eos:
            raise ValueError("%s: add_eos=False is not supported" % what)
        b = features.size(0)
        given, optional = self._checked_supervision(given, optional, graphs, b, ambiguous, None, what)
        valid_classes = self._check_valid_classes(valid_classes_per_instance)
        ids = list(range(self.n_classes)) if valid_classes is None else [int(v) for v in valid_classes]
        sup = self._local_supervision(given, optional, graphs, np.array([ids + [self.n_classes]], np.int64), [len(ids)],
                                      np.zeros(b, np.int64))
        self._require_device(features, what)
        st = self._one_group_tables(valid_classes, features.device) if differentiable else None
        batch, x, cons, endpen, tab, g1 = self._stage_padded(features, lengths, valid_classes, additional_allowed_ends_per_instance,
                                                             constraints, check_no_eos=False, tables=st, projected=projected)
        if differentiable:
            return (batch, x, cons, endpen, tuple(st[k] for k in TABLE_NAMES) + (None,), st['inv_var']), sup
        return _emit(batch, x, cons, endpen, g1, tab['inv_var']), sup

    def _supervised_packed(self, pc, what, given, optional=None, graphs=False, ambiguous=None, differentiable=False):
        """``_supervised_padded`` for a PackedCorpus, prepared for this module here; the supervision in the order of
        ``pc.video_names``, which its refusals name the videos by."""
        no_eos = "%s: add_eos=False is not supported" % what
        if getattr(pc, 'batch', None) is not None and pc.batch.no_eos:
            raise ValueError(no_eos)
        names = list(pc.video_names)
        given, optional = self._checked_supervision(given, optional, graphs, len(names), ambiguous, names, what)
        staged = self._packed_stage(pc, what, differentiable)
        batch = staged[0]
        if batch.no_eos:                                           # (a corpus this call prepared)
            raise ValueError(no_eos)
        group = batch.group if batch.group is not None else np.zeros(batch.b, np.int64)
        sup = self._local_supervision(given, optional, graphs, staged[4][5].cpu().numpy(), batch.n_states, group)
        return (staged if differentiable else _emit(*staged)), sup

    # ------------------------------------------------------------------ forced alignment (smm_align_f64)
    @torch.no_grad()
    def align(self, features, lengths, valid_classes_per_instance, transcripts, add_eos=True,
              additional_allowed_ends_per_instance=None, constraints=None, optional=None):
        """Forced alignment of a zero-padded single-task batch (argument conventions of ``viterbi``): ``transcripts[i]`` is the
        class sequence of video i in GLOBAL class ids, one entry per segment (consecutive repeats are two segments); the result
        is the best segmentation with exactly that sequence.  One emission launch, one alignment launch (smm_align_f64).

        Returns (pred_spans, scores): pred_spans CPU int64 b x (Tmax+1) in ``viterbi``'s format, scores fp64 b on the device.
        A transcript that cannot be laid over its video (more entries than frames, or too few for the span limit) gives a row
        of -1 and score -inf.  ValueError for an id that is not valid for the video, an empty transcript or add_eos=False.
        Raises SmmError when a NaN reached the DP.  No autograd.

        ``optional``: one boolean sequence per video, as long as its transcript; the flagged entries may be left out and the
        result is the best over every subset of them (smm_align_opt_f64; ``ops.align_optional``).  ValueError when their count or a
        length differs from the transcripts'."""
        r, sup = self._supervised_padded('align', features, lengths, valid_classes_per_instance, add_eos,
                                         additional_allowed_ends_per_instance, constraints, transcripts, optional)
        return _align(r, sup, want_spans=True)

    @torch.no_grad()
    def align_packed(self, pc, transcripts, optional=None):
        """``align`` for a whole PackedCorpus: one emission launch and one alignment launch.  ``transcripts``: one sequence of
        GLOBAL class ids per video, in the order of ``pc.video_names``.  Returns (labels, scores): device int64 total_frames
        (global class ids on the packed frame axis, -1 on frames no video covers and on videos without an alignment) and fp64
        n_videos.  ``optional``: as in ``align``."""
        return _align(*self._supervised_packed(pc, 'align_packed', transcripts, optional), want_spans=False)

    # ------------------------------------------------------------------ alignment to a transcript graph (smm_align_graph_f64)
    @torch.no_grad()
    def align_graph(self, features, lengths, valid_classes_per_instance, graphs, add_eos=True,
                    additional_allowed_ends_per_instance=None, constraints=None):
        """Alignment of a zero-padded single-task batch to transcript graphs (argument conventions of ``align``):
        ``graphs[i]`` is an ``ops.TranscriptGraph`` in GLOBAL class ids -- a candidate set as its trie, alternatives, a free
        order, long skips -- and the result is the best segmentation whose class sequence is one of its start -> end paths.
        One emission launch, one alignment launch (smm_align_graph_f64).

        Returns (pred_spans, scores, used): ``align``'s pair and a list of per-video int32 device tensors, 1 for the nodes of
        the path (``graph.candidate_of(used[i])`` names the candidate of a trie).  A video none of whose paths can be laid over
        it, or whose graph names a class that is not valid for it, gives a row of -1, score -inf and no used node.  ValueError
        for a wrong number of graphs or add_eos=False; SmmError when a NaN reached the DP.  No autograd."""
        if len(graphs) != len(lengths):
            raise ValueError("align_graph: %d graphs for %d videos" % (len(graphs), len(lengths)))
        r, sup = self._supervised_padded('align_graph', features, lengths, valid_classes_per_instance, add_eos,
                                         additional_allowed_ends_per_instance, constraints, graphs, graphs=True)
        return _align(r, sup, want_spans=True)

    @torch.no_grad()
    def align_graph_packed(self, pc, graphs):
        """``align_graph`` for a whole PackedCorpus: one emission launch and one alignment launch.  ``graphs``: one
        ``ops.TranscriptGraph`` in GLOBAL class ids per video, in the order of ``pc.video_names``.  Returns (labels, scores,
        used): device int64 total_frames (-1 on frames no video covers and on videos without an alignment), fp64 n_videos and
        the per-video flags of the nodes on the path."""
        return _align(*self._supervised_packed(pc, 'align_graph_packed', graphs, graphs=True), want_spans=False)

    # ------------------------------------------------------------------ segment posteriors under a transcript graph
    @torch.no_grad()
    def alignment_segment_posteriors(self, features, lengths, valid_classes_per_instance, graphs, spans=None, used=None,
                                     add_eos=True, additional_allowed_ends_per_instance=None, constraints=None, want_dense=False):
        """How sure the transcript-graph posterior is of each segment of an alignment, and where each node's segment starts and
        ends, exactly (argument conventions of ``align_graph``).  ``spans`` (b x (Tmax+1) or n_sets x b x (Tmax+1)) and ``used``
        (the per-video int32 flags, [M_i] or [n_sets, M_i]): alignments as ``align_graph`` / ``sample_alignments`` return them;
        None: ``align_graph``'s own result.  One emission launch, the forward launch and one
        smm_align_graph_segment_posteriors_f64 launch (one alignment launch more for the default).

        Returns the dict of ``ops.align_graph_segment_posteriors`` (``seg_logp``, ``node_logp``, ``end_mean``, ``end_sd``,
        ``start_mean``, ``start_sd``; with ``want_dense`` ``node_end_post`` / ``node_start_post``) with ``spans``, ``used`` and
        ``logz``.  A video without an alignment gets NaN; an alignment its graph does not admit gets -inf.  Values, not
        differentiable."""
        if len(graphs) != len(lengths):
            raise ValueError("alignment_segment_posteriors: %d graphs for %d videos" % (len(graphs), len(lengths)))
        r, sup = self._supervised_padded('alignment_segment_posteriors', features, lengths, valid_classes_per_instance, add_eos,
                                         additional_allowed_ends_per_instance, constraints, graphs, graphs=True)
        return _alignment_segment_posteriors(r, sup, spans, used, want_dense=want_dense)

    @torch.no_grad()
    def alignment_segment_posteriors_packed(self, pc, graphs, spans=None, used=None, want_dense=False):
        """``alignment_segment_posteriors`` for a whole PackedCorpus; ``graphs``, ``spans`` and ``used`` in the order of
        ``pc.video_names``; None means ``align_graph_packed``'s alignment.  Values, not differentiable."""
        r, sup = self._supervised_packed(pc, 'alignment_segment_posteriors_packed', graphs, graphs=True)
        return _alignment_segment_posteriors(r, sup, spans, used, want_dense=want_dense)

    @torch.no_grad()
    def alignment_boundaries_packed(self, pc, graphs):
        """Where each node's segment starts and ends under the transcript-graph posterior of a whole PackedCorpus: dict(end_mean,
        end_sd, start_mean, start_sd), lists of per-video fp64 [M_i] device tensors in frames, given that the path crosses the
        node (NaN for a node without mass or a video without an alignment).  Values, not differentiable."""
        r, sup = self._supervised_packed(pc, 'alignment_boundaries_packed', graphs, graphs=True)
        out = _alignment_segment_posteriors(r, sup, want_alignment=False)
        return {key: out[key] for key in ('end_mean', 'end_sd', 'start_mean', 'start_sd')}

    # ------------------------------------------------------------------ transcript likelihood (smm_align_logz_f64)
    def transcript_log_partition(self, features, lengths, valid_classes_per_instance, transcripts, add_eos=True,
                                 additional_allowed_ends_per_instance=None, constraints=None, optional=None, ambiguous='raise',
                                 projected=False):
        """log Z_a per video of a zero-padded single-task batch (argument conventions of ``align``): the log of the sum over
        every segmentation whose class sequence is ``transcripts[i]`` (GLOBAL class ids, one entry per segment, consecutive
        repeats are two segments) -- the joint log-likelihood of frames and transcript; minus ``log_partition`` it is the
        conditional likelihood of the transcript.  fp64 b on the device, differentiable w.r.t. the module's parameters
        (smm_emission_f64 + smm_align_logz_f64 forward, smm_align_logz_bwd_f64 + smm_emission_bwd_f64 backward).
        ValueError for add_eos=False, an id that is not valid for the video, an empty transcript, and for a video no
        segmentation of which has its transcript (log Z_a = -inf); SmmError when a NaN reached the DP.

        ``optional`` (``align``'s conventions: one boolean sequence per video, as long as its transcript): the flagged entries
        may be missing, and the value is log Z_o, the sum over every alignment with any subset of them left out
        (smm_align_opt_logz_f64 / _bwd_f64) -- the likelihood of the set of class sequences when no two subsets give the same
        one.  ``ambiguous``: 'raise' (ValueError naming the first video with two such subsets) or 'allow' (the sum over
        alignments as defined, a segmentation counted once per subset that yields its class sequence)."""
        if len(transcripts) != features.size(0):
            raise ValueError("transcript_log_partition: %d transcripts for %d videos" % (len(transcripts), features.size(0)))
        z = _alignment_log_partition(*self._supervised_padded(
            'transcript_log_partition', features, lengths, valid_classes_per_instance, add_eos, additional_allowed_ends_per_instance,
            constraints, transcripts, optional, ambiguous=ambiguous, differentiable=True, projected=projected))
        _check_transcript_logz(z, None, 'transcript_log_partition')
        return z

    def transcript_log_partition_packed(self, pc, transcripts, optional=None, ambiguous='raise'):
        """``transcript_log_partition`` for a whole PackedCorpus in one launch of each kernel: ``transcripts`` holds one sequence
        of GLOBAL class ids per video, in the order of ``pc.video_names``.  fp64 [n_videos], differentiable.  ``optional``,
        ``ambiguous``: as in ``transcript_log_partition``."""
        z = _alignment_log_partition(*self._supervised_packed(pc, 'transcript_log_partition_packed', transcripts, optional,
                                                              ambiguous=ambiguous, differentiable=True))
        _check_transcript_logz(z, list(pc.video_names), 'transcript_log_partition_packed')
        return z

    @torch.no_grad()
    def transcript_scores_packed(self, pc, transcripts, conditional=False, optional=None, ambiguous='raise'):
        """Without autograd, on the cached decode tables: log Z_a of every video of a PackedCorpus (``conditional``: minus its
        log Z) as a CPU fp64 tensor; -inf for a video no segmentation of which has its transcript.  One emission launch, then
        the DP launches.  SmmError when a NaN reached the DP.  ``optional``, ``ambiguous``: as in ``transcript_log_partition``
        (log Z_o in place of log Z_a)."""
        r, sup = self._supervised_packed(pc, 'transcript_scores_packed', transcripts, optional, ambiguous=ambiguous)
        return _transcript_scores(r, sup, conditional, 'transcript_scores_packed')

    @torch.no_grad()
    def transcript_entry_posteriors_packed(self, pc, transcripts, optional, ambiguous='raise'):
        """Per video of a PackedCorpus the posterior probability that each entry of its transcript has a segment, given the
        frames and the transcript with its ``optional`` flags (p_used of smm_align_opt_logz_bwd_f64: 1 for a mandatory entry):
        a list of fp64 CPU arrays in the order of ``pc.video_names``; zeros for a video without an alignment.  One emission
        launch, then the forward and the backward launches.  SmmError when a NaN reached the DP."""
        if optional is None:
            raise ValueError("transcript_entry_posteriors_packed: one sequence of optional flags per video expected")
        r, sup = self._supervised_packed(pc, 'transcript_entry_posteriors_packed', transcripts, optional, ambiguous=ambiguous)
        grads = _transcript_posteriors(r, sup, 'transcript_entry_posteriors_packed', want_entry_prob=True)
        return [p.cpu().numpy() for p in grads['entry_prob']]

    # ------------------------------------------------------------------ transcript-graph likelihood (smm_align_graph_logz_f64)
    def transcript_graph_log_partition(self, features, lengths, valid_classes_per_instance, graphs, add_eos=True,
                                       additional_allowed_ends_per_instance=None, constraints=None, ambiguous='raise',
                                       projected=False):
        """log Z_g per video of a zero-padded single-task batch (argument conventions of ``align_graph``): the log of the sum
        over every segmentation whose class sequence is a start -> end path of ``graphs[i]`` (an ``ops.TranscriptGraph`` in
        GLOBAL class ids) -- for a candidate set (``TranscriptGraph.from_candidates``) the joint log-likelihood of the frames and
        "one of these transcripts"; minus ``log_partition`` the conditional one.  fp64 b on the device, differentiable w.r.t.
        the module's parameters (smm_emission_f64 + smm_align_graph_logz_f64 forward, smm_align_graph_logz_bwd_f64 +
        smm_emission_bwd_f64 backward).  ``ambiguous``: 'raise' (ValueError naming the first video two paths of whose graph
        spell the same class sequence) or 'allow' (such a sequence's segmentations count once per path).  ValueError for
        add_eos=False, a wrong number of graphs, and for a video none of whose paths can be laid over it (log Z_g = -inf; a
        class that is not valid for the video does that); SmmError when a NaN reached the DP."""
        z = _alignment_log_partition(*self._supervised_padded(
            'transcript_graph_log_partition', features, lengths, valid_classes_per_instance, add_eos,
            additional_allowed_ends_per_instance, constraints, graphs, graphs=True, ambiguous=ambiguous, differentiable=True,
            projected=projected))
        _check_transcript_logz(z, None, 'transcript_graph_log_partition')
        return z

    def transcript_graph_log_partition_packed(self, pc, graphs, ambiguous='raise'):
        """``transcript_graph_log_partition`` for a whole PackedCorpus in one launch of each kernel: ``graphs`` holds one
        ``ops.TranscriptGraph`` in GLOBAL class ids per video, in the order of ``pc.video_names``.  fp64 [n_videos],
        differentiable."""
        z = _alignment_log_partition(*self._supervised_packed(pc, 'transcript_graph_log_partition_packed', graphs, graphs=True,
                                                              ambiguous=ambiguous, differentiable=True))
        _check_transcript_logz(z, list(pc.video_names), 'transcript_graph_log_partition_packed')
        return z

    @torch.no_grad()
    def transcript_graph_scores_packed(self, pc, graphs, conditional=False, ambiguous='raise'):
        """Without autograd, on the cached decode tables: log Z_g of every video of a PackedCorpus (``conditional``: minus its
        log Z) as a CPU fp64 tensor; -inf for a video none of whose paths can be laid over it.  One emission launch, then the
        DP launches.  SmmError when a NaN reached the DP.  ``ambiguous``: as in ``transcript_graph_log_partition``."""
        r, sup = self._supervised_packed(pc, 'transcript_graph_scores_packed', graphs, graphs=True, ambiguous=ambiguous)
        return _transcript_scores(r, sup, conditional, 'transcript_graph_scores_packed')

    @torch.no_grad()
    def transcript_node_posteriors_packed(self, pc, graphs):
        """Per video of a PackedCorpus the posterior probability, given the frames and "the class sequence is a path of the
        graph", that the path crosses each node and that it ends in it (p_used and p_end of smm_align_graph_logz_bwd_f64):
        (p_used, p_end), two lists of fp64 CPU arrays in the order of ``pc.video_names``; zeros for a video without an
        alignment, p_end adds up to 1 otherwise.  Paths that spell the same class sequence share its mass as they share its
        segmentations.  One emission launch, then the forward and the backward launches.  SmmError when a NaN reached the DP."""
        r, sup = self._supervised_packed(pc, 'transcript_node_posteriors_packed', graphs, graphs=True, ambiguous='allow')
        grads = _transcript_posteriors(r, sup, 'transcript_node_posteriors_packed', want_node_prob=True, want_end_prob=True)
        return [p.cpu().numpy() for p in grads['node_prob']], [p.cpu().numpy() for p in grads['end_prob']]

    # ------------------------------------------------------------------ samples of the graph posterior (smm_align_graph_sample_f64)
    @torch.no_grad()
    def sample_alignments(self, features, lengths, valid_classes_per_instance, graphs, n_samples=1, seed=0, add_eos=True,
                          additional_allowed_ends_per_instance=None, constraints=None):
        """Alignments drawn from the posterior of transcript supervision, p(alignment | x, "the class sequence is a
        start -> end path of ``graphs[i]``"), for a zero-padded single-task batch (argument conventions of ``align_graph``;
        graphs in GLOBAL class ids): one emission launch, the forward launch (smm_align_graph_logz_f64) and the sampler
        (smm_align_graph_sample_f64).  Sample j depends on (seed, video, j) only.

        Returns (spans, log_prob, used): spans CPU int64 n_samples x b x (Tmax+1) in ``viterbi``'s pred_spans format, log_prob
        fp64 n_samples x b on the device -- the exact log-probability of each drawn alignment (path and boundaries) --, used a
        list of per-video int32 device tensors n_samples x M_i, 1 for the nodes of the sampled path.  A video none of whose
        paths can be laid over it gives rows of -1, log_prob NaN and no used node.  ValueError for a wrong number of graphs,
        n_samples < 1 or add_eos=False; SmmError when a NaN reached the DP.  No autograd."""
        if int(n_samples) < 1:
            raise ValueError("sample_alignments: n_samples must be positive, got %d" % int(n_samples))
        r, sup = self._supervised_padded('sample_alignments', features, lengths, valid_classes_per_instance, add_eos,
                                         additional_allowed_ends_per_instance, constraints, graphs, graphs=True, ambiguous='allow')
        return _sample_alignments(r, sup, n_samples, seed, want_spans=True)

    @torch.no_grad()
    def sample_alignments_packed(self, pc, graphs, n_samples, seed=0):
        """``sample_alignments`` for a whole PackedCorpus: one emission launch, the forward launch and the sampler.  ``graphs``:
        one ``ops.TranscriptGraph`` in GLOBAL class ids per video, in the order of ``pc.video_names``.  Returns (labels,
        log_prob, used): device int64 n_samples x total_frames (global class ids on the packed frame axis, -1 on frames no
        video covers and on videos without an alignment), fp64 n_samples x n_videos and the per-video flags of the sampled
        paths' nodes."""
        if int(n_samples) < 1:
            raise ValueError("sample_alignments_packed: n_samples must be positive, got %d" % int(n_samples))
        r, sup = self._supervised_packed(pc, 'sample_alignments_packed', graphs, graphs=True, ambiguous='allow')
        return _sample_alignments(r, sup, n_samples, seed, want_spans=False)

    # ------------------------------------------------------------------ entropy of the graph posterior (smm_align_graph_entropy_f64)
    def alignment_entropy(self, features, lengths, valid_classes_per_instance, graphs, add_eos=True,
                          additional_allowed_ends_per_instance=None, constraints=None, want_parts=False, *, differentiable=False):
        """The exact entropy, in nats, of the posterior ``sample_alignments`` draws from, p(alignment | x, "the class sequence
        is a start -> end path of ``graphs[i]``"), for a zero-padded single-task batch (argument conventions of
        ``align_graph``; graphs in GLOBAL class ids): one emission launch, the forward launch (smm_align_graph_logz_f64) and the
        entropy launch (smm_align_graph_entropy_f64).  An alignment is a path and its boundaries: on an ambiguous graph two
        paths that spell one class sequence are two alignments.

        Returns fp64 b on the device, or with ``want_parts`` the pair (entropy, parts): parts fp64 b x 3, the entropy of the
        end node (for a trie: of the posterior over the candidates), of the segments' starts and of the predecessors, which
        add up to the entropy.  A video none of whose paths can be laid over it gives NaN.  ValueError for a wrong number of
        graphs or add_eos=False; SmmError when a NaN reached the DP.
        ``differentiable``: the same value (bit for bit, from the same launches), differentiable with respect to the module's
        parameters: the backward runs smm_align_graph_entropy_bwd_f64 and the chain rule through the emission scorer and the
        factor tables; the parts carry no gradient.  A video without an alignment is then a ValueError that names it
        (``transcript_graph_log_partition``'s): a NaN cannot be trained on."""
        with torch.no_grad():
            side = self._supervised_padded('alignment_entropy', features, lengths, valid_classes_per_instance, add_eos,
                                           additional_allowed_ends_per_instance, constraints, graphs, graphs=True, ambiguous='allow')
            if not differentiable:
                h, parts, _ = _alignment_entropy(*side, want_parts)
                return (h, parts) if want_parts else h
        self._no_projected_gradient()
        tabs = self._differentiable_tables(self._check_valid_classes(valid_classes_per_instance), features.device)
        return _alignment_value('entropy', 'alignment_entropy', None, [side], tabs, want_parts)

    def alignment_entropy_packed(self, pc, graphs, want_parts=False, *, differentiable=False):
        """``alignment_entropy`` for a whole PackedCorpus: one emission launch, the forward launch and the entropy launch.
        ``graphs``: one ``ops.TranscriptGraph`` in GLOBAL class ids per video, in the order of ``pc.video_names``.  Returns fp64
        n_videos on the device, or with ``want_parts`` (entropy, parts fp64 n_videos x 3).  ``differentiable``: as
        ``alignment_entropy``'s; the tables are ``stacked_tables(pc, differentiable=True)``."""
        with torch.no_grad():
            side = self._supervised_packed(pc, 'alignment_entropy_packed', graphs, graphs=True, ambiguous='allow')
            if not differentiable:
                h, parts, _ = _alignment_entropy(*side, want_parts)
                return (h, parts) if want_parts else h
        self._no_projected_gradient()
        st = self.stacked_tables(pc, differentiable=True)[0]
        return _alignment_value('entropy', 'alignment_entropy_packed', list(pc.video_names), [side], tuple(st[k] for k in TABLE_NAMES),
                                want_parts)

    # ------------------------------------------------------------------ expected reward under the graph posterior (smm_align_graph_expected_reward_f64)
    def _alignment_reward_value(self, what, names, side, rw, node_reward, sg, tables, want_parts, differentiable):
        """Both ``alignment_expected_reward`` methods behind their staging: the rewards into the record, the node rewards (with
        the per-class ``sg`` broadcast into them), then the value, or the autograd Function on it.  ``tables``: a callable
        that returns the differentiable tables."""
        r, sup = side
        batch = r['batch']
        group = batch.group if batch.group is not None else np.zeros(batch.b, np.int64)
        with torch.no_grad():
            r['reward'], r['node_reward'] = rw, _node_rewards(sup, node_reward, sg, group, r['elp'].device, what)
            if r['reward'] is None and r['node_reward'] is None:
                raise ValueError("%s: at least one of reward, node_reward and seg_reward is needed" % what)
            if not differentiable:
                v, parts, _ = _alignment_expected_reward(r, sup, want_parts)
                return (v, parts) if want_parts else v
        self._no_projected_gradient()
        return _alignment_value('expected_reward', what, names, [side], tables(), want_parts)

    def alignment_expected_reward(self, features, lengths, valid_classes_per_instance, graphs, reward=None, node_reward=None,
                                  seg_reward=None, add_eos=True, additional_allowed_ends_per_instance=None, constraints=None,
                                  want_parts=False, *, differentiable=False):
        """The expectation, under the posterior ``sample_alignments`` draws from, of a reward that is additive over the frames
        and the nodes of an alignment, exactly: fp64 b on the device (argument conventions of ``alignment_entropy``; graphs in
        GLOBAL class ids).  R(y) = sum over the segments (node j of class c) of y of node_reward[j] + seg_reward[c] + the sum of
        reward[t, c] over the segment's frames.  ``reward``: b x Tmax x C, columns in the order of the batch's valid classes
        (``expected_reward``'s convention; padded frames are ignored); ``node_reward``: one sequence per video, one entry per
        node of its graph (or one tensor over all nodes); ``seg_reward``: length C, a convenience that is broadcast into the node
        rewards over each node's class; at least one of the three.  reward = one-hot labels: the expected number of correct
        frames of an alignment (``alignment_expected_accuracy``); node_reward = 1: the expected number of segments, which says
        how many optional entries are used; node_reward = one-hot of an end node of a trie: that candidate's posterior.  One
        emission launch, the forward launch (smm_align_graph_logz_f64) and the smm_align_graph_expected_reward_f64 launch.  With
        ``want_parts`` the pair (value, parts fp64 b x 2: the frame part and the node part).  A video none of whose paths can be
        laid over it gives NaN.  Raises SmmError when a NaN reached the DP or a reward is not finite.
        ``differentiable``: the same value (bit for bit, from the same launches), differentiable with respect to the module's
        parameters (not the rewards: one that requires grad is refused): the backward runs
        smm_align_graph_expected_reward_bwd_f64, a Hessian-vector product of log Z_g, and the chain rule through the emission
        scorer and the factor tables; the parts carry no gradient.  A video without an alignment is then a ValueError that
        names it (``transcript_graph_log_partition``'s)."""
        what = 'alignment_expected_reward'
        with torch.no_grad():
            side = self._supervised_padded(what, features, lengths, valid_classes_per_instance, graphs=True, ambiguous='allow',
                                           add_eos=add_eos, additional_allowed_ends_per_instance=additional_allowed_ends_per_instance,
                                           constraints=constraints, given=graphs)
        b, tmax = features.shape[:2]
        dev = features.device
        vc = self._check_valid_classes(valid_classes_per_instance)
        c = self.n_classes if vc is None else int(vc.numel())
        rw = _reward_tensor(reward, (b, tmax, c), dev, 'reward')
        sg = _reward_tensor(seg_reward, (c,), dev, 'seg_reward')
        return self._alignment_reward_value(what, None, side, None if rw is None else rw.view(b * tmax, c), node_reward,
                                            None if sg is None else sg.view(1, c), lambda: self._differentiable_tables(vc, dev),
                                            want_parts, differentiable)

    def alignment_expected_reward_packed(self, pc, graphs, reward=None, node_reward=None, seg_reward=None, want_parts=False, *,
                                         differentiable=False):
        """``alignment_expected_reward`` for a whole PackedCorpus: fp64 n_videos on the device, in the order of
        ``pc.video_names``.  ``graphs``: one ``ops.TranscriptGraph`` in GLOBAL class ids per video; ``reward``: total_frames x
        c_max on local states (the layout of ``frame_posteriors_packed``); ``node_reward``: as the padded method's;
        ``seg_reward``: n_groups x c_max.  ``differentiable``: as ``alignment_expected_reward``'s; the tables are
        ``stacked_tables(pc, differentiable=True)``."""
        what = 'alignment_expected_reward_packed'
        with torch.no_grad():
            side = self._supervised_packed(pc, what, graphs, graphs=True, ambiguous='allow')
        batch, dev = pc.batch, pc.x.device
        rw = _reward_tensor(reward, (batch.total_frames, batch.c_max), dev, 'reward')
        sg = _reward_tensor(seg_reward, (batch.n_groups, batch.c_max), dev, 'seg_reward')
        tables = lambda: tuple(self.stacked_tables(pc, differentiable=True)[0][k] for k in TABLE_NAMES)
        return self._alignment_reward_value(what, list(pc.video_names), side, rw, node_reward, sg, tables, want_parts, differentiable)

    def alignment_expected_accuracy(self, features, lengths, valid_classes_per_instance, graphs, labels, normalize=False,
                                    add_eos=True, additional_allowed_ends_per_instance=None, constraints=None, *,
                                    differentiable=False):
        """Expected number of frames of each video on which an alignment drawn from the transcript-graph posterior agrees with
        ``labels`` (b x Tmax, GLOBAL class ids; ``expected_accuracy``'s conventions): fp64 b on the device; with ``normalize``
        the fraction of the video's frames.  ``alignment_expected_reward`` with reward = one-hot(labels): against held-out
        labels a quality estimate of the weak supervision, against pseudo-labels or a teacher (``differentiable``) risk
        training from transcripts; with a few annotated frames (every other label negative) the expected number of
        timestamps hit."""
        self._require_device(features, 'alignment_expected_accuracy')
        onehot = self._onehot_labels(features, valid_classes_per_instance, labels)
        v = self.alignment_expected_reward(features, lengths, valid_classes_per_instance, graphs, reward=onehot, add_eos=add_eos,
                                           additional_allowed_ends_per_instance=additional_allowed_ends_per_instance,
                                           constraints=constraints, differentiable=differentiable)
        return v / lengths.to(device=features.device, dtype=torch.float64) if normalize else v

    def alignment_expected_accuracy_packed(self, pc, graphs, labels, normalize=False, *, differentiable=False):
        """``alignment_expected_accuracy`` for a whole PackedCorpus.  ``labels``: int64 total_frames, global class ids on the
        packed frame axis; fp64 n_videos in the order of ``pc.video_names``."""
        self._require_device(pc.x, 'alignment_expected_accuracy_packed')
        self.prepare_packed(pc)
        v = self.alignment_expected_reward_packed(pc, graphs, reward=self._onehot_labels_packed(pc, labels),
                                                  differentiable=differentiable)
        return v / torch.as_tensor(pc.batch.lengths, device=pc.x.device).to(torch.float64) if normalize else v

    # ------------------------------------------------------------------ KL of two graph posteriors (smm_align_graph_kl_f64)
    def _alignment_kl_padded(self, other, what, features, lengths, valid_classes_per_instance, graphs, add_eos,
                             additional_allowed_ends_per_instance, constraints, other_constraints, want_cross_entropy, want_parts,
                             differentiable=False):
        self._check_same_lattice(other, what)
        stage = lambda m, c: m._supervised_padded(what, features, lengths, valid_classes_per_instance, add_eos,
                                                  additional_allowed_ends_per_instance, c, graphs, graphs=True, ambiguous='allow')
        with torch.no_grad():
            q = stage(other, other_constraints)
            p = stage(self, constraints)
            if not differentiable:
                value, parts, _ = _alignment_kl(p[0], q[0], p[1], what, want_cross_entropy, want_parts)
                return (value, parts) if want_parts else value
        valid = self._check_valid_classes(valid_classes_per_instance)
        self._no_projected_gradient(other)
        tabs = self._differentiable_tables(valid, features.device) + other._differentiable_tables(valid, features.device)
        return _alignment_value('cross_entropy' if want_cross_entropy else 'kl', what, None, [p, q], tabs, want_parts)

    def _alignment_kl_packed(self, other, pc, graphs, what, want_cross_entropy, want_parts, differentiable=False):
        self._check_same_lattice(other, what)
        with torch.no_grad():
            saved = dict(pc.__dict__)                              # (q first, `pc` left prepared for `self`: as _kl_packed)
            try:
                q = other._supervised_packed(pc, what, graphs, graphs=True, ambiguous='allow')
            finally:
                pc.__dict__.clear()
                pc.__dict__.update(saved)
            p = self._supervised_packed(pc, what, graphs, graphs=True, ambiguous='allow')
            if not differentiable:
                value, parts, _ = _alignment_kl(p[0], q[0], p[1], what, want_cross_entropy, want_parts)
                return (value, parts) if want_parts else value
        self._no_projected_gradient(other)
        tabs = tuple(m.stacked_tables(pc, differentiable=True)[0][k] for m in (self, other) for k in TABLE_NAMES)
        return _alignment_value('cross_entropy' if want_cross_entropy else 'kl', what, list(pc.video_names), [p, q], tabs, want_parts)

    def alignment_kl(self, other, features, lengths, valid_classes_per_instance, graphs, add_eos=True,
                     additional_allowed_ends_per_instance=None, constraints=None, other_constraints=None, want_parts=False, *,
                     differentiable=False):
        """The exact KL(p || q), in nats, between two posteriors over the alignments of each video to ``graphs[i]`` (argument
        conventions of ``alignment_entropy``; graphs in GLOBAL class ids): p is this module's under ``constraints``, q is
        ``other``'s under ``other_constraints`` (``other`` may be ``self``); each side builds its tables, emissions and end
        penalties from its own parameters.  Two emission launches, two forward launches (smm_align_graph_logz_f64), one KL
        launch (smm_align_graph_kl_f64); the value keeps its relative accuracy as q -> p and is exactly 0 for the same inputs.

        Returns fp64 b on the device, or with ``want_parts`` the pair (kl, parts): parts fp64 b x 3, the KL of the end node
        (for a trie: between the two posteriors over the candidates), of the segments' starts and of the predecessors, which
        add up to the KL.  NaN for a video p cannot align, +inf where q excludes an alignment p does not.  TypeError when
        ``other`` is no SemiMarkovModule, ValueError when the lattices differ, for a wrong number of graphs or add_eos=False;
        SmmError when a NaN reached the DP.
        ``differentiable``: the same value (bit for bit), differentiable with respect to both modules' parameters: the backward
        runs smm_align_graph_kl_bwd_f64 for p's tables, mu_q - mu_p (two smm_align_graph_logz_bwd_f64) for q's, and each side's
        chain rule through the emission scorer and the factor tables.  A video either side cannot align is then a ValueError."""
        return self._alignment_kl_padded(other, 'alignment_kl', features, lengths, valid_classes_per_instance, graphs, add_eos,
                                         additional_allowed_ends_per_instance, constraints, other_constraints, False, want_parts,
                                         differentiable)

    def alignment_cross_entropy(self, other, features, lengths, valid_classes_per_instance, graphs, add_eos=True,
                                additional_allowed_ends_per_instance=None, constraints=None, other_constraints=None,
                                want_parts=False, *, differentiable=False):
        """The exact cross-entropy H(p, q) = -sum p log q = H(p) + KL(p || q) of the same two posteriors, in nats: arguments,
        launches and refusals as ``alignment_kl`` (the parts are the KL's); with ``other`` = ``self`` and the same constraints
        it is ``alignment_entropy``'s value to that kernel's fp32 rounding.  ``differentiable``: as ``alignment_kl``'s."""
        return self._alignment_kl_padded(other, 'alignment_cross_entropy', features, lengths, valid_classes_per_instance, graphs,
                                         add_eos, additional_allowed_ends_per_instance, constraints, other_constraints, True,
                                         want_parts, differentiable)

    def alignment_kl_packed(self, other, pc, graphs, want_parts=False, *, differentiable=False):
        """``alignment_kl`` for a whole PackedCorpus: fp64 n_videos on the device in the order of ``pc.video_names``, or with
        ``want_parts`` (kl, parts fp64 n_videos x 3).  q's tables and end penalties are built on ``pc``'s layout; ``pc`` is left
        prepared for ``self``.  ``differentiable``: as ``alignment_kl``'s."""
        return self._alignment_kl_packed(other, pc, graphs, 'alignment_kl_packed', False, want_parts, differentiable)

    def alignment_cross_entropy_packed(self, other, pc, graphs, *, differentiable=False):
        """``alignment_cross_entropy`` for a whole PackedCorpus: fp64 n_videos on the device.  ``differentiable``: as
        ``alignment_kl``'s."""
        return self._alignment_kl_packed(other, pc, graphs, 'alignment_cross_entropy_packed', True, False, differentiable)

    # ------------------------------------------------------------------ packed multi-task decode
    def stacked_tables(self, pc, differentiable=False):
        """fp64 factor tables of every group of a PackedCorpus stacked to [groups, ...] and zero-padded to c_max columns.
        ``differentiable``: built from the parameters with autograd history (training); otherwise the cached decode
        tables."""
        dev = pc.device or pc.x.device
        if differentiable and self.max_k > 1:
            return self._stacked_tables_batched(pc, dev)
        if differentiable:
            tabs = [self.factor_tables(g['valid_classes'], dev) for g in pc.groups]
        else:
            # the stack of a corpus is good while the parameters (and what else the tables read) have not changed: one key
            # for the corpus, looked at before the per-group tables (whose keys list the classes of a group: a device ->
            # host copy per group when the corpus is resident -- 18 of them were 0.3 ms of a 3.2 ms predict() on cfg3)
            key = (self._param_key(), self._constraint_key(), str(dev), self.max_k)
            hit = getattr(pc, '_stacked', None)
            if hit is not None and hit[0] == key:
                return hit[1]
            tabs = [self._decode_tables(g['valid_classes'], dev) for g in pc.groups]
        n_states = [int(t['init'].numel()) for t in tabs]
        cm = max(n_states)
        pad = lambda t, c, rows=False: F.pad(t, (0, cm - c) + ((0, cm - c) if rows else ()))
        st = dict(trans=torch.stack([pad(t['trans'], c, True) for t, c in zip(tabs, n_states)]).contiguous(),
                  init=torch.stack([pad(t['init'], c) for t, c in zip(tabs, n_states)]).contiguous(),
                  len=torch.stack([pad(t['len'], c) for t, c in zip(tabs, n_states)]).contiguous(),
                  w=torch.stack([pad(t['w'], c) for t, c in zip(tabs, n_states)]).contiguous(),
                  cst=torch.stack([pad(t['cst'], c) for t, c in zip(tabs, n_states)]).contiguous(),
                  inv_var=tabs[0]['inv_var'],
                  class_map=torch.stack([F.pad(t['class_map'], (0, cm - c)) for t, c in zip(tabs, n_states)]).contiguous())
        out = (st, n_states, cm, tabs[0]['len'].size(0))
        if not differentiable:
            pc._stacked = (key, out, tabs)          # (tabs: keeps the ids alive)
        return out

    def _stacked_tables_batched(self, pc, dev, use_hip=None):
        """The differentiable tables of ALL groups of a launch.  fp32 parameters on the GPU: one HIP launch forward and
        one backward (``_FactorTables``, csrc/smm_tables.hip).  Otherwise (``use_hip=False``: the statement the HIP
        kernels are tested against) ~25 batched torch ops instead of a dozen small ops per group.  Same
        formulas as ``factor_tables`` / reference :284-414 -- masks before the softmax, columns normalised over `to`,
        Poisson length table, expanded Gaussian -- on index tensors padded to c_max (padded entries are excluded from
        every normalisation and come out as 0; the kernels never read them)."""
        f64 = torch.float64
        ix = getattr(pc, '_group_index', None)
        if ix is None or ix['dev'] != str(dev) or ix['merge'] != id(self.merge_classes):
            n_states = [self.n_classes if g['valid_classes'] is None else len(g['valid_classes']) for g in pc.groups]
            cm, ng = max(n_states), len(pc.groups)
            vcp = torch.zeros((ng, cm), dtype=torch.long)
            mvp = torch.zeros((ng, cm), dtype=torch.long)
            valid = torch.zeros((ng, cm), dtype=torch.bool)
            cmap = torch.zeros((ng, cm + 1), dtype=torch.long)
            for i, (g, c) in enumerate(zip(pc.groups, n_states)):
                vc = torch.arange(self.n_classes) if g['valid_classes'] is None else g['valid_classes'].long()
                bad = [int(v) for v in vc if not 0 <= int(v) < self.n_classes]
                if bad:
                    raise IndexError("valid_classes %s outside the model's %d classes" % (bad, self.n_classes))
                assert len(set(vc.tolist())) == c, "valid_classes must be unique"
                vcp[i, :c] = vc
                mvp[i, :c] = self._merged(vc)
                valid[i, :c] = True
                cmap[i, :c] = vc
                cmap[i, c] = self.n_classes
            ix = pc._group_index = dict(dev=str(dev), merge=id(self.merge_classes), n_states=n_states, cm=cm,
                                        vcp=vcp.to(dev), mvp=mvp.to(dev), valid=valid.to(dev), cmap=cmap.to(dev))
        vcp, mvp, valid, cm = ix['vcp'], ix['mvp'], ix['valid'], ix['cm']
        params = (self.init_logits, self.transition_logits, self.poisson_log_rates, self.gaussian_means, self.gaussian_cov)
        if use_hip is None:
            use_hip = dev.type == 'cuda' and cm <= 32 and all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()
                                                              for p in params)
        if use_hip:
            meta = ix.get('meta')
            if meta is None:
                meta = ix['meta'] = ops.TablesMeta(vcp, mvp, torch.tensor(ix['n_states'], dtype=torch.int32).to(dev),
                                                   self.n_classes, self.feature_dim, self.max_k,
                                                   self.allow_self_transitions)
            ic, tc = self.init_constraints, self.transition_constraints
            trans, init, lens, w, cst, inv_var = _FactorTables.apply(
                meta, None if ic is None else ic.detach().contiguous(), None if tc is None else tc.detach().contiguous(),
                *params)
            st = dict(trans=trans, init=init, len=lens, w=w, cst=cst, inv_var=inv_var, class_map=ix['cmap'])
            return st, ix['n_states'], cm, self.max_k
        neg_inf = float('-inf')
        # initial (reference :284-296)
        il = self.init_logits.to(f64)
        if self.init_constraints is not None:
            il = il.masked_fill(self.init_constraints, BIG_NEG)
        init = F.log_softmax(il[vcp].masked_fill(~valid, neg_inf), dim=1).masked_fill(~valid, 0.0)
        # transitions [to, from] (reference :298-322): every column normalised over the valid `to`
        tl = self.transition_logits.to(f64)
        if self.transition_constraints is not None:
            tl = tl.masked_fill(self.transition_constraints, BIG_NEG)
        tm = tl[vcp.unsqueeze(2), vcp.unsqueeze(1)]                           # [G, to, from]
        if not self.allow_self_transitions:
            tm = tm.masked_fill(torch.eye(cm, device=dev, dtype=torch.bool).unsqueeze(0), BIG_NEG)
        tm = tm.masked_fill(~valid.unsqueeze(2), neg_inf)
        trans = F.log_softmax(tm, dim=1).masked_fill(~(valid.unsqueeze(2) & valid.unsqueeze(1)), 0.0)
        # lengths (reference :383-414): Poisson(rate).log_prob(k), row == length
        lr = self.poisson_log_rates.to(f64)[mvp]                                # [G, cm]
        k = torch.arange(self.max_k, device=dev, dtype=f64).view(1, -1, 1)
        rate = torch.exp(lr).unsqueeze(1)
        lens = (torch.xlogy(k, rate) - rate - torch.lgamma(k + 1)).masked_fill(~valid.unsqueeze(1), 0.0)
        # emission factors (reference :324-381 in expanded form)
        var = torch.diagonal(self.gaussian_cov).to(f64)
        mu = self.gaussian_means.to(f64)[mvp]                                   # [G, cm, D]
        d = mu.size(2)
        w = (mu / var).transpose(1, 2).masked_fill(~valid.unsqueeze(1), 0.0).contiguous()          # [G, D, cm]
        cst = (-0.5 * (mu * mu / var).sum(2) - 0.5 * var.log().sum() - 0.5 * d * math.log(2 * math.pi)).masked_fill(~valid, 0.0)
        st = dict(trans=trans.contiguous(), init=init.contiguous(), len=lens.contiguous(), w=w, cst=cst.contiguous(),
                  inv_var=(1.0 / var).contiguous(), class_map=ix['cmap'])
        return st, ix['n_states'], cm, self.max_k

    def prepare_packed(self, pc, differentiable=False):
        """Stack the fp64 factor tables of every group of a PackedCorpus (batching.py), padded to c_max columns, and
        build the per-video end penalties / constraint block / launch metadata."""
        dev = pc.device or pc.x.device
        d = pc.x.size(1)
        if pc.n_videos == 0:                # an empty shard: nothing to launch (predict_packed returns {})
            pc.tables, pc.batch, pc.cons, pc.endpen = {}, None, None, None
            return pc
        st, n_states, cm, k_rows = self.stacked_tables(pc, differentiable)
        pc.tables, pc.n_states, pc.c_max, pc.k_rows = st, n_states, cm, k_rows
        if getattr(pc, '_static', None) == (cm, k_rows, id(self)):
            return pc                                # end penalties, constraints and launch metadata do not change
        pc.kp = [min(k, k_rows) for k in pc.kp]
        pc.endpen = None
        if self.allowed_ends is not None:
            ep = torch.full((pc.n_videos, cm), BIG_NEG, dtype=torch.float64)
            for i in range(pc.n_videos):
                vc = pc.groups[pc.group[i]]['valid_classes']
                add = pc.additional_ends[i]
                ends = self._allowed_ends_per_instance(vc, None if add is None else [add], 1)[0]
                ep[i, ends] = 0.0
            pc.endpen = ep.to(dev)
        pc.cons = None
        if getattr(pc, 'cons_list', None) is not None:
            cons = torch.zeros(pc.x.size(0), cm, dtype=torch.float32, device=dev)
            for i, cl in enumerate(pc.cons_list):
                if cl is not None:
                    o = pc.frame_offset[i]
                    cons[o:o + pc.lengths[i], :cl.size(1)] = cl.to(device=dev, dtype=torch.float32)
            pc.cons = cons
        pc.batch = ops.Batch(pc.lengths, n_states, k_rows, c_max=cm, frame_offset=pc.frame_offset, group=pc.group,
                             kp=pc.kp, d=d, total_frames=pc.x.size(0), no_time_split=self._hard_masks())
        pc._static = (cm, k_rows, id(self))
        return pc

    def decode_packed(self, pc, want_spans=False, want_labels=True, want_elp=False, labels_on_host=False, x=None,
                      labels_out=None):
        """One emission launch + one DP launch for a whole PackedCorpus.  Returns the dict of ops.decode
        (``labels``: int64 [total_frames] global class ids; ``spans``: [n_videos, t_max+1]).
        ``x``: the corpus' features on the device when ``pc.x`` itself lives on the host (predict_host uploads them slab by
        slab); ``labels_out``: where the frame labels go (a device tensor, or pinned host memory)."""
        x = pc.x if x is None else x
        self._require_device(x, 'decode_packed')
        x = self._project_packed(pc, x)
        if pc.tables is None:
            self.prepare_packed(pc)
        t = pc.tables
        if want_labels and not want_spans and not want_elp:
            # the common call -- frame labels of a resident corpus -- with its arguments marshalled once (ops.ResidentDecode);
            # rebuilt when the tables were (a parameter update) or the features moved (predict_host's device buffers)
            args = (x, t['w'], t['cst'], t['inv_var'], t['trans'], t['init'], t['len'], pc.cons, pc.endpen, t['class_map'])
            key = tuple(None if a is None else (a.data_ptr(), a._version) for a in args)
            calls = pc.__dict__.setdefault('_resident_calls', {})
            call = calls.get(x.data_ptr())
            if call is None or call.key != key:
                if len(calls) > 4:
                    calls.clear()
                call = calls[x.data_ptr()] = ops.ResidentDecode(pc.batch, *args[:7], cons=pc.cons, endpen=pc.endpen, class_map=t['class_map'])
            return call(labels_on_host=labels_on_host, labels_out=labels_out)
        return ops.decode(pc.batch, x, t['w'], t['cst'], t['inv_var'], t['trans'], t['init'], t['len'],
                          cons=pc.cons, endpen=pc.endpen, class_map=t['class_map'], want_spans=want_spans,
                          want_labels=want_labels, want_elp=want_elp, labels_on_host=labels_on_host, labels_out=labels_out)

    # ------------------------------------------------------------------ likelihoods (reference :597-658)
    def gold_score(self, features, lengths, valid_classes, spans, additional_allowed_ends_per_instance=None,
                   constraints=None, no_eos=False, projected=False):
        """Joint score of given span encodings = sum(potentials * to_parts(spans)) of the reference (:641-655),
        evaluated on the factors (differentiable torch ops, O(T*C); no dense tensor).  spans: b x Tmax global ids.
        ``no_eos`` (add_eos=False): ``to_parts`` has an edge per span START after the first, so the last span is not
        scored, except that its label's emission of the last frame counts when it starts there (modules:519-521)."""
        tab = self.factor_tables(valid_classes, features.device)
        f64 = torch.float64
        if getattr(self, 'feature_projector', None) is not None:     # (the reference scores the projected features: :560-563;
            self._require_device(features, 'gold_score')             # from ``log_likelihood`` they already are)
            features = self._project(features.to(torch.float32).contiguous(), projected)
        x = features.to(f64)
        elp = tab['cst'] + x @ tab['w'] - 0.5 * (x * x) @ tab['inv_var'].unsqueeze(1)
        if constraints is not None:
            elp = elp + constraints.to(elp)
        b, tmax, c = elp.shape
        cum = torch.cat([elp.new_zeros(b, 1, c), elp.cumsum(1)], dim=1)
        ids = list(range(self.n_classes)) if valid_classes is None else [int(v) for v in valid_classes]
        local = {g: i for i, g in enumerate(ids)}
        ends = self._allowed_ends_per_instance(valid_classes, additional_allowed_ends_per_instance, b)
        k_rows = tab['len'].size(0)
        kp = min(k_rows, tmax)
        # Segment list on the host (integers only), then ONE gather + segment-sum on the device: no per-segment device
        # scalars (a Python loop of tiny tensor ops per segment was the cost of --sm_supervised_method gradient-based).
        sp = spans.detach().cpu().numpy()
        seg_i, seg_s0, seg_s1, seg_c, tr_i, tr_to, tr_from, init_i, init_c, pen_i, last_i, last_c = ([] for _ in range(12))
        for i in range(b):
            t = int(lengths[i])
            row = sp[i, :t]
            starts = np.flatnonzero(row != -1).tolist()
            assert starts and starts[0] == 0, "a span encoding starts with a label"
            bounds = starts + [t]
            labs = [local[int(row[s])] for s in starts]
            n_scored = len(labs) - 1 if no_eos else len(labs)     # no EOS: the last span has no edge (to_parts)
            if n_scored > 0:
                init_i.append(i); init_c.append(labs[0])
            for j in range(n_scored):
                kk = bounds[j + 1] - bounds[j]
                assert 1 <= kk <= kp - 1, "span longer than the model's max span length"
                seg_i.append(i); seg_s0.append(bounds[j]); seg_s1.append(bounds[j + 1]); seg_c.append(labs[j])
                if j + 1 < len(labs):
                    tr_i.append(i); tr_to.append(labs[j + 1]); tr_from.append(labs[j])
            if no_eos:
                if bounds[-2] == t - 1:                            # the closing label's emission of the last frame
                    last_i.append(i); last_c.append(labs[-1])
            elif ends is not None and labs[-1] not in ends[i]:
                pen_i.append(i)
        dev = elp.device
        li = lambda v: torch.as_tensor(v, dtype=torch.long, device=dev)
        total = torch.zeros(b, dtype=f64, device=dev)
        if seg_i:
            si, s0, s1, sc = li(seg_i), li(seg_s0), li(seg_s1), li(seg_c)
            total = total.index_add(0, si, tab['len'][s1 - s0, sc] + (cum[si, s1, sc] - cum[si, s0, sc]))
        if tr_i:
            total = total.index_add(0, li(tr_i), tab['trans'][li(tr_to), li(tr_from)])
        if init_i:
            total = total.index_add(0, li(init_i), tab['init'][li(init_c)])
        if last_i:
            ii = li(last_i)
            total = total.index_add(0, ii, elp[ii, li([int(lengths[i]) - 1 for i in last_i]), li(last_c)])
        if pen_i:
            total = total.index_add(0, li(pen_i), torch.full((len(pen_i),), BIG_NEG, dtype=f64, device=dev))
        return total

    def _one_group_tables(self, valid_classes, dev):
        """The fp64 tables of one class set as a stack of one group, with autograd history."""
        if self.max_k > 1:
            # one-group stack (HIP table kernels for fp32 parameters on the GPU); the index tensors are kept per class set
            cache = self.__dict__.setdefault('_single_group', {})
            key = None if valid_classes is None else tuple(int(v) for v in valid_classes)
            one = cache.get(key)
            if one is None:
                one = cache[key] = types.SimpleNamespace(groups=[dict(valid_classes=valid_classes)])
            return self._stacked_tables_batched(one, dev)[0]
        tab = self.factor_tables(valid_classes, dev)
        st = {n: tab[n].unsqueeze(0).contiguous() for n in TABLE_NAMES}
        st['inv_var'] = tab['inv_var'].contiguous()
        return st

    def _differentiable_tables(self, valid_classes, dev):
        """(w, cst, trans, init, len) of one class set with autograd history: the inputs of _PosteriorValue."""
        st = self._one_group_tables(valid_classes, dev)
        return tuple(st[k] for k in TABLE_NAMES)

    def log_partition(self, features, lengths, valid_classes, additional_allowed_ends_per_instance=None,
                      constraints=None, no_eos=False, projected=False):
        """log Z per instance on the device, differentiable w.r.t. the module's parameters
        (smm_emission_f64 + smm_logz_f64 forward, smm_logz_bwd_f64 backward)."""
        self._require_device(features, 'log_partition')
        st = self._one_group_tables(valid_classes, features.device)
        batch, x, cons, endpen, _, _ = self._stage_padded(features, lengths, valid_classes, additional_allowed_ends_per_instance,
                                                          constraints, no_eos=no_eos, no_time_split=self._hard_masks(), tables=st,
                                                          projected=projected)
        return _LogPartition.apply(batch, x, cons, endpen, st['w'], st['cst'], st['inv_var'], st['trans'], st['init'], st['len'])

    def log_partition_packed(self, pc):
        """log Z of every video of a PackedCorpus (any number of single-task batches, any mix of tasks) in ONE launch
        of each kernel, differentiable w.r.t. the parameters: the unsupervised objective of reference
        semimarkov.py:259-286 for many batches at once (gradient accumulation, or the E-step over a whole corpus).
        Returns fp64 [n_videos] in the order of ``pc.video_names``."""
        self._require_device(pc.x, 'log_partition_packed')
        self.prepare_packed(pc, differentiable=True)
        t = pc.tables
        return _LogPartition.apply(pc.batch, self._project_packed(pc, pc.x, differentiable=True), pc.cons, pc.endpen, t['w'], t['cst'], t['inv_var'], t['trans'], t['init'],
                                   t['len'])

    def log_likelihood_packed(self, pc):
        """Per source batch the mean log-likelihood the reference's ``log_likelihood(spans=None)`` returns for it
        (semimarkov_modules.py:657: ``dist.partition.mean()``): fp64 [n_batches], differentiable."""
        z = self.log_partition_packed(pc)
        # the means per source batch as ONE product with a [n_batches, n_videos] matrix of 1 / count entries -- a property of the
        # packed corpus, made once (a zero fill, an index_add and a multiplication each way before: six launches per training step)
        nb = int(max(pc.batch_index)) + 1
        if nb * z.numel() > BATCH_MEAN_DENSE_MAX:
            # (a corpus of many thousands of videos: the dense matrix would be tens of megabytes and more; the sums by index)
            bi = getattr(pc, '_batch_index_dev', None)
            if bi is None or bi.device != z.device:
                bi = pc._batch_index_dev = torch.as_tensor(pc.batch_index, device=z.device)
            inv = getattr(pc, '_batch_inv_count_dev', None)
            if inv is None or inv.device != z.device or inv.dtype != z.dtype:
                cnt = torch.zeros(nb, dtype=z.dtype, device=z.device).index_add(0, bi, torch.ones_like(z))
                inv = pc._batch_inv_count_dev = (1.0 / cnt).detach()
            return torch.zeros(nb, dtype=z.dtype, device=z.device).index_add(0, bi, z) * inv
        mean_of = getattr(pc, '_batch_mean_matrix_dev', None)
        if mean_of is None or mean_of.device != z.device or mean_of.dtype != z.dtype:
            bi = torch.as_tensor(pc.batch_index, device=z.device)
            cnt = torch.zeros(nb, dtype=z.dtype, device=z.device).index_add(0, bi, torch.ones_like(z))
            mean_of = torch.zeros((nb, z.numel()), dtype=z.dtype, device=z.device)
            mean_of[bi, torch.arange(z.numel(), device=z.device)] = (1.0 / cnt)[bi]
            pc._batch_mean_matrix_dev = mean_of.detach()
        return torch.mv(mean_of, z)

    def log_likelihood(self, features, lengths, valid_classes_per_instance, spans=None, add_eos=True, use_mean_z=False,
                       additional_allowed_ends_per_instance=None, constraints=None, transcripts=None, transcript_optional=None,
                       transcript_graphs=None):
        """(mean log-likelihood, mean log_det) like the reference (:597-658).

        spans given: joint score p(x, y) (differentiable), or with --sm_train_discriminatively the conditional
        score - log Z.  spans=None: the log-partition (marginal likelihood) from the HIP forward kernel; its gradient
        (posterior marginals chained into the parameters) comes from the HIP backward kernels.
        transcripts given (and no spans): only the order of each video's actions is known -- the mean of log Z_a
        (``transcript_log_partition``), or with --sm_train_discriminatively of log Z_a - log Z.  ``transcript_optional``: one
        boolean sequence per transcript, the flagged entries may be missing (log Z_o; ValueError for an ambiguous transcript).
        transcript_graphs given (and neither spans nor transcripts): one ``ops.TranscriptGraph`` per video, e.g. the trie of its
        candidate transcripts -- the mean of log Z_g (``transcript_graph_log_partition``; ValueError for an ambiguous graph),
        or with --sm_train_discriminatively of log Z_g - log Z.
        """
        if spans is not None and transcripts is not None:
            raise ValueError("log_likelihood: give spans (full supervision) or transcripts (the order only), not both")
        if transcript_graphs is not None and (spans is not None or transcripts is not None):
            raise ValueError("log_likelihood: give transcript_graphs alone, without spans or transcripts")
        if transcript_optional is not None and transcripts is None:
            raise ValueError("log_likelihood: transcript_optional goes with transcripts")
        no_eos = not add_eos
        valid_classes = self._check_valid_classes(valid_classes_per_instance)
        self.set_z(features, lengths, use_mean=use_mean_z)
        log_det = torch.zeros(features.size(0), device=features.device)
        if getattr(self, 'feature_projector', None) is not None:
            # project ONCE: the gold score and the likelihood launches of one step read the same y, and the flow runs forward and
            # backward once per step
            self._require_device(features, 'log_likelihood')
            features = self._project((features if features.requires_grad else features.detach()).to(torch.float32).contiguous())
            return self._log_likelihood_value(features, lengths, valid_classes, valid_classes_per_instance, spans, add_eos,
                                              additional_allowed_ends_per_instance, constraints, transcripts,
                                              transcript_optional, transcript_graphs, True), log_det.mean()
        return self._log_likelihood_value(features, lengths, valid_classes, valid_classes_per_instance, spans, add_eos,
                                          additional_allowed_ends_per_instance, constraints, transcripts, transcript_optional,
                                          transcript_graphs, False), log_det.mean()

    def _log_likelihood_value(self, features, lengths, valid_classes, valid_classes_per_instance, spans, add_eos,
                              additional_allowed_ends_per_instance, constraints, transcripts, transcript_optional,
                              transcript_graphs, projected):
        """The mean of ``log_likelihood``; ``projected``: the features are the projection already, and every call below is told."""
        no_eos = not add_eos
        if transcripts is not None:
            ll = self.transcript_log_partition(features, lengths, valid_classes_per_instance, transcripts, add_eos=add_eos,
                                               additional_allowed_ends_per_instance=additional_allowed_ends_per_instance,
                                               constraints=constraints, optional=transcript_optional, projected=projected)
            if getattr(self.args, 'sm_train_discriminatively', False):
                ll = ll - self.log_partition(features, lengths, valid_classes, additional_allowed_ends_per_instance,
                                             constraints, projected=projected)
        elif transcript_graphs is not None:
            ll = self.transcript_graph_log_partition(features, lengths, valid_classes_per_instance, transcript_graphs,
                                                     add_eos=add_eos,
                                                     additional_allowed_ends_per_instance=additional_allowed_ends_per_instance,
                                                     constraints=constraints, projected=projected)
            if getattr(self.args, 'sm_train_discriminatively', False):
                ll = ll - self.log_partition(features, lengths, valid_classes, additional_allowed_ends_per_instance,
                                             constraints, projected=projected)
        elif spans is not None:
            ll = self.gold_score(features, lengths, valid_classes, spans, additional_allowed_ends_per_instance, constraints,
                                 no_eos=no_eos, projected=projected)
            if getattr(self.args, 'sm_train_discriminatively', False):
                ll = ll - self.log_partition(features, lengths, valid_classes, additional_allowed_ends_per_instance,
                                             constraints, no_eos=no_eos, projected=projected)
        else:
            ll = self.log_partition(features, lengths, valid_classes, additional_allowed_ends_per_instance, constraints,
                                    no_eos=no_eos, projected=projected)
        return ll.mean()
