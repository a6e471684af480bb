"""Golden trace of the module layer: which launchers of ``ops`` every entry point of ``SemiMarkovModule`` calls, in which order
and with which arguments.

    python tests/golden/make_golden_module_trace.py            ->  tests/golden/module_launch_trace.json   (committed)
    python tests/golden/make_golden_module_trace.py --show ID  ->  the full trace of one case on stdout (for a diff)

No GPU: ``semimarkov_modules.ops`` is replaced by a recording stand-in whose launchers return CPU tensors of the real shapes,
each filled with a serial number, so the arguments of a later call show which earlier output they consumed.  Everything else
of ``ops`` stays real (``Batch``, ``TablesMeta``, ``_lib``, ``workspace``; ``Batch.workspace_bytes`` is a host call into the
library).  The committed table was made from the module in front of the refactor that gave the padded staging, the one-group
stack and each posterior operation one statement; the rows of the transcript family (alignment with optional entries and to a
graph, the three transcript likelihoods with their backward passes, the graph sampler) were made from ``ops.py``,
``semimarkov_modules.py`` and ``semimarkov.py`` exactly as they stood in front of the refactor that gave that family one
statement of its supervision, its autograd function and its staging.  tests/test_module_trace_host.py holds every later module
to it.

What a call keeps: the launcher's name; every argument under its parameter name, after binding to the real launcher's
signature (a default left out and the same value spelled out are one call); a ``Batch`` as its fields and ``shape.flags``;
a tensor as dtype, shape, strides, device type and a digest of its bytes (floating values rounded to 8 decimals first: the
last bit of an exp or a log differs between CPUs); a uint8 tensor -- a workspace, or the staged flags of a transcript -- as its
index by first appearance within the entry point; an ``ops.TranscriptGraph`` as its classes, edges, start and end flags and
candidate indices.  The entry point's return value (and the parameters' gradients after a backward) are kept the same way.
The table stores the launcher names of each case and an 8-digit digest per call.
"""
import hashlib
import inspect
import itertools
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "module_launch_trace.json")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAUNCHERS = ('emission', 'emission_bwd', 'decode', 'viterbi', 'logz', 'logz_bwd', 'sample', 'entropy', 'entropy_bwd', 'kl',
             'kl_bwd', 'kbest', 'mbr', 'align', 'check_decoded', '_err_copy', 'pinned_labels', 'align_optional', 'align_graph',
             'align_logz', 'align_logz_ex', 'align_logz_bwd', 'align_opt_logz', 'align_opt_logz_bwd', 'align_graph_logz',
             'align_graph_logz_bwd', 'align_graph_sample')
BATCH_FIELDS = ('b', 'd', 'n_groups', 'c_max', 'k_rows', 't_max', 'total_frames', 'lengths', 'frame_offset', 'group', 'kp',
                'n_states')


def _sha(data):
    return hashlib.sha1(data).hexdigest()[:12]


class Recorder:
    """Stands in for the ``ops`` module: the launchers record and return serial-numbered CPU tensors, the rest is real."""

    def __init__(self, real):
        self._real = real
        self.calls = []
        self._serial = 0
        self._ws = []            # the workspaces seen, in order of first appearance (kept alive: an address is not reused)

    def __getattr__(self, name):
        return getattr(self._real, name)

    # ---------------------------------------------------------------- what is kept of a value
    def rec(self, v):
        real = self._real
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, real.Batch):
            out = {f: self.rec(getattr(v, f)) for f in BATCH_FIELDS}
            out['flags'] = int(v.shape.flags)
            return {'Batch': out}
        if torch.is_tensor(v):
            if v.dtype == torch.uint8:
                for i, w in enumerate(self._ws):
                    if w is v or (w.data_ptr() == v.data_ptr() and w.numel() == v.numel()):
                        return {'ws': i}
                self._ws.append(v)
                return {'ws': len(self._ws) - 1}
            a = v.detach().contiguous().numpy()
            if a.dtype.kind == 'f':
                a = np.round(a.astype(np.float64), 8) + 0.0
            return {'dtype': str(v.dtype), 'shape': list(v.shape), 'stride': list(v.stride()), 'device': v.device.type,
                    'sha': _sha(np.ascontiguousarray(a).tobytes())}
        if isinstance(v, np.ndarray):
            return {'np': str(v.dtype), 'v': v.tolist()}
        if isinstance(v, np.generic):
            return v.item()
        if isinstance(v, (tuple, list)):
            return {type(v).__name__: [self.rec(e) for e in v]}
        if isinstance(v, dict):
            return {'dict': {str(k): self.rec(e) for k, e in v.items()}}
        if isinstance(v, torch.device):
            return str(v)
        if isinstance(v, real.TranscriptGraph):
            return {'TranscriptGraph': {k: getattr(v, k).tolist() for k in ('ids', 'pred', 'start', 'end', 'end_candidate')}}
        if type(v).__name__ == 'PackedCorpus':
            return {'PackedCorpus': {k: self.rec(getattr(v, k, None)) for k in
                                     ('tables', 'n_states', 'c_max', 'k_rows', 'kp', 'endpen', 'cons', 'batch')}}
        return {'object': type(v).__name__}

    def _note(self, name, args, kwargs):
        bound = inspect.signature(getattr(self._real, name)).bind(*args, **kwargs)
        bound.apply_defaults()
        self.calls.append({'launcher': name, 'args': {k: self.rec(v) for k, v in bound.arguments.items()}})
        return bound.arguments

    def _new(self, shape, dtype=torch.float64):
        self._serial += 1
        return torch.full(tuple(int(s) for s in shape), self._serial % 251 if dtype == torch.uint8 else self._serial, dtype=dtype)

    def _err(self):
        return self._new((8,), torch.int32)

    def _like(self, elp, trans, init, len_scores):
        return dict(elp=self._new(elp.shape), trans=self._new(trans.shape), init=self._new(init.shape),
                    len=self._new(len_scores.shape))

    def _paths(self, batch, want_spans, want_labels, lead=()):
        i64 = torch.int64
        return (self._new(lead + (batch.b, batch.t_max + 1), i64) if want_spans else None,
                self._new(lead + (batch.total_frames,), i64) if want_labels else None,
                self._new(lead + (batch.b,)), self._new(lead + (batch.b,), torch.int32))

    # ---------------------------------------------------------------- the launchers (shapes: ops.py)
    def emission(self, *args, **kwargs):
        a = self._note('emission', args, kwargs)
        b = a['batch']
        elp64 = a['out64'] if a['out64'] is not None else (self._new((b.total_frames, b.c_max)) if a['want64'] else None)
        return elp64, (self._new((b.total_frames, b.c_max), torch.float32) if a['want32'] else None)

    def emission_bwd(self, *args, **kwargs):
        a = self._note('emission_bwd', args, kwargs)
        b, d = a['batch'], int(a['x'].size(1))
        return self._new((b.n_groups, b.c_max, d)).transpose(1, 2), self._new((b.n_groups, b.c_max)), self._new((d,))

    def _decode_like(self, name, args, kwargs):
        a = self._note(name, args, kwargs)
        b = a['batch']
        spans, labels, best, n_segs = self._paths(b, a['want_spans'], a['want_labels'])
        if a['labels_out'] is not None:
            labels = a['labels_out']
        out = dict(spans=spans, labels=labels, best=best, n_segs=n_segs)
        if name == 'decode':
            out['elp'] = self._new((b.total_frames, b.c_max), torch.float32) if a['want_elp'] else None
        out['_err'] = self._err()
        return out

    def decode(self, *args, **kwargs):
        return self._decode_like('decode', args, kwargs)

    def viterbi(self, *args, **kwargs):
        return self._decode_like('viterbi', args, kwargs)

    def logz(self, *args, **kwargs):
        return self._new((self._note('logz', args, kwargs)['batch'].b,))

    def logz_bwd(self, *args, **kwargs):
        a = self._note('logz_bwd', args, kwargs)
        return self._like(a['elp'], a['trans'], a['init'], a['len_scores'])

    def sample(self, *args, **kwargs):
        a = self._note('sample', args, kwargs)
        spans, labels, logp, _ = self._paths(a['batch'], a['want_spans'], a['want_labels'], (int(a['n_samples']),))
        return dict(spans=spans, labels=labels, logp=logp, _err=self._err())

    def entropy(self, *args, **kwargs):
        return self._new((self._note('entropy', args, kwargs)['batch'].b,))

    def kl(self, *args, **kwargs):
        a = self._note('kl', args, kwargs)
        out = self._new((a['batch'].b,))
        return (out, self._new((a['batch'].b,))) if a['want_cross_entropy'] else out

    def entropy_bwd(self, *args, **kwargs):
        a = self._note('entropy_bwd', args, kwargs)
        return dict(self._like(a['elp'], a['trans'], a['init'], a['len_scores']), value=None)

    def kl_bwd(self, *args, **kwargs):
        p = self._note('kl_bwd', args, kwargs)['p']
        return dict(self._like(p[0], p[1], p[2], p[3]), value=None)

    def kbest(self, *args, **kwargs):
        a = self._note('kbest', args, kwargs)
        spans, labels, score, n_segs = self._paths(a['batch'], a['want_spans'], a['want_labels'], (int(a['k']),))
        return dict(spans=spans, labels=labels, score=score, n_segs=n_segs, _err=self._err())

    def mbr(self, *args, **kwargs):
        a = self._note('mbr', args, kwargs)
        spans, labels, best, n_segs = self._paths(a['batch'], a['want_spans'], a['want_labels'])
        return dict(spans=spans, labels=labels, best=best, gain_sum=self._new((a['batch'].b,)), n_segs=n_segs, _err=self._err())

    def align(self, *args, **kwargs):
        a = self._note('align', args, kwargs)
        spans, labels, best, n_segs = self._paths(a['batch'], a['want_spans'], a['want_labels'])
        return dict(spans=spans, labels=labels, best=best, n_segs=n_segs, _err=self._err(), _keep=())

    # ---------------------------------------------------------------- the transcript family
    def _entries(self, supervision):
        """Transcript entries / graph nodes per video; ``supervision`` may be the (ids, offsets) pair of ``align_logz_ex``."""
        if isinstance(supervision, tuple) and len(supervision) == 2 and torch.is_tensor(supervision[0]):
            return np.diff(supervision[1]).tolist()
        return [len(s) if isinstance(s, self._real.TranscriptGraph) else int(np.asarray(s).size) for s in supervision]

    def _staged(self, kind, n, given=None):
        """What a launcher keeps of its supervision on the device: chain (ids,), optional (ids, flags), graph (ids, masks,
        flags); ``given``: the caller's ``staged``, handed on as it came."""
        if given is not None:
            return given
        i32, u8 = torch.int32, torch.uint8
        return {'chain': lambda: (self._new((n,), i32),), 'optional': lambda: (self._new((n,), i32), self._new((n,), u8)),
                'graph': lambda: (self._new((n,), i32), self._new((n * 8,), i32), self._new((n,), u8))}[kind]()

    def _own_ws(self, given):
        return given if given is not None else torch.zeros(16, dtype=torch.uint8)

    def _per_video(self, t, sizes, dim=0):
        return list(torch.split(t, [int(n) for n in sizes], dim=dim))

    def _align_like(self, name, kind, args, kwargs):
        a = self._note(name, args, kwargs)
        sizes = self._entries(a['graphs'] if kind == 'graph' else a['transcripts'])
        spans, labels, best, n_segs = self._paths(a['batch'], a['want_spans'], a['want_labels'])
        used = self._per_video(self._new((sum(sizes),), torch.int32), sizes) if a['want_used'] else None
        return dict(spans=spans, labels=labels, best=best, n_segs=n_segs, used=used, _err=self._err(),
                    _staged=self._staged(kind, sum(sizes), a['staged']), _keep=(self._own_ws(a['ws']),))

    def align_optional(self, *args, **kwargs):
        return self._align_like('align_optional', 'optional', args, kwargs)

    def align_graph(self, *args, **kwargs):
        return self._align_like('align_graph', 'graph', args, kwargs)

    def align_logz(self, *args, **kwargs):
        return self._new((self._note('align_logz', args, kwargs)['batch'].b,))

    def align_logz_ex(self, *args, **kwargs):
        a = self._note('align_logz_ex', args, kwargs)
        sizes = self._entries(a['transcripts'])
        off = np.zeros(len(sizes) + 1, np.int64)
        np.cumsum(sizes, out=off[1:])
        return dict(logz=self._new((a['batch'].b,)), ws=self._own_ws(a['ws']),
                    transcript=(self._staged('chain', sum(sizes))[0], off), _err=self._err())

    def _logz_like(self, name, kind, args, kwargs):
        a = self._note(name, args, kwargs)
        n = sum(self._entries(a['graphs'] if kind == 'graph' else a['transcripts']))
        ws = self._own_ws(a['ws'])
        out = dict(logz=self._new((a['batch'].b,)), ws=ws, _staged=self._staged(kind, n, a['staged']), _err=self._err())
        if kind == 'graph':
            out['_keep'] = (ws,)
        return out

    def align_opt_logz(self, *args, **kwargs):
        return self._logz_like('align_opt_logz', 'optional', args, kwargs)

    def align_graph_logz(self, *args, **kwargs):
        return self._logz_like('align_graph_logz', 'graph', args, kwargs)

    def align_logz_bwd(self, *args, **kwargs):
        a = self._note('align_logz_bwd', args, kwargs)
        return self._like(a['elp'], a['trans'], a['init'], a['len_scores'])

    def _logz_bwd_like(self, name, kind, wanted, args, kwargs):
        a = self._note(name, args, kwargs)
        sizes = self._entries(a['graphs'] if kind == 'graph' else a['transcripts'])
        g = self._like(a['elp'], a['trans'], a['init'], a['len_scores'])
        for want, key in wanted:
            if a[want]:
                g[key] = self._per_video(self._new((sum(sizes),)), sizes)
        g['_keep'] = self._staged(kind, sum(sizes), a['staged'])
        return g

    def align_opt_logz_bwd(self, *args, **kwargs):
        return self._logz_bwd_like('align_opt_logz_bwd', 'optional', (('want_entry_prob', 'entry_prob'),), args, kwargs)

    def align_graph_logz_bwd(self, *args, **kwargs):
        return self._logz_bwd_like('align_graph_logz_bwd', 'graph', (('want_node_prob', 'node_prob'), ('want_end_prob', 'end_prob')),
                                   args, kwargs)

    def align_graph_sample(self, *args, **kwargs):
        a = self._note('align_graph_sample', args, kwargs)
        n, sizes = int(a['n_samples']), self._entries(a['graphs'])
        spans, labels, logp, n_segs = self._paths(a['batch'], a['want_spans'], a['want_labels'], (n,))
        used = self._per_video(self._new((n, sum(sizes)), torch.int32), sizes, dim=1) if a['want_used'] else None
        return dict(spans=spans, labels=labels, logp=logp, n_segs=n_segs, used=used, _err=self._err(),
                    _staged=self._staged('graph', sum(sizes), a['staged']), _keep=(self._own_ws(a['ws']),))

    def check_decoded(self, *args, **kwargs):
        self._note('check_decoded', args, kwargs)

    def _err_copy(self, *args, **kwargs):
        self._note('_err_copy', args, kwargs)
        return self._err()

    def pinned_labels(self, *args, **kwargs):
        return self._new((self._note('pinned_labels', args, kwargs)['numel'],), torch.int64)


def trace(smm, fn):
    """Run ``fn()`` with the recording ``ops`` and CPU tensors allowed -> {'calls': [...], 'result': ...}.
    ``fn`` returns the entry point's value, or (value, parameters) after a backward: their gradients are kept too."""
    rec = Recorder(smm.ops)
    saved = smm.ops, smm.SemiMarkovModule.__dict__['_require_device']
    smm.ops = rec
    smm.SemiMarkovModule._require_device = staticmethod(lambda t, what: None)
    try:
        out = fn()
    finally:
        smm.ops = saved[0]
        smm.SemiMarkovModule._require_device = saved[1]
    res = {'calls': rec.calls}
    if isinstance(out, Grads):
        res['result'] = rec.rec(out.value)
        res['grads'] = [None if p.grad is None else rec.rec(p.grad) for p in out.params]
    else:
        res['result'] = rec.rec(out)
    return res


class Grads:
    def __init__(self, value, modules):
        self.value = value
        self.params = [p for m in modules for _, p in sorted(m.named_parameters())]


# -------------------------------------------------------------------------------------------------- the cases
B, TMAX, D, C, K = 3, 6, 3, 4, 4
LENGTHS = [6, 3, 2]
SUBSET = [0, 1, 3]


def _args(max_k):
    import argparse
    return argparse.Namespace(sm_max_span_length=max_k, sm_supervised_state_smoothing=1e-2, sm_supervised_length_smoothing=1e-1,
                              sm_supervised_method='closed-form', sm_feature_projection=False,
                              sm_init_non_projection_parameters_from=None, sm_train_discriminatively=False)


def padded_module(smm, hard, seed, max_k=K):
    kw = {}
    if hard:
        kw = dict(allowed_starts={0, 1}, allowed_transitions={0: {1, 3}, 1: {0, 3}, 2: {3}, 3: {0, 1, 2}}, allowed_ends={3})
    torch.manual_seed(seed)
    m = smm.SemiMarkovModule(_args(max_k), C, D, allow_self_transitions=False, **kw)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        m.gaussian_means.copy_(torch.randn(C, D, generator=g) * 0.5)
        m.poisson_log_rates.copy_(torch.rand(C, generator=g) + 0.5)
        m.transition_logits.copy_(torch.randn(C, C, generator=g))
        m.init_logits.copy_(torch.rand(C, generator=g))
    return m


def padded_inputs(vc, cons, addl):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, TMAX, D, generator=g)
    c = len(SUBSET) if vc else C
    cons1 = torch.randn(B, TMAX, c, generator=g)
    cons2 = torch.randn(B, TMAX, c, generator=g)
    ids = torch.tensor(SUBSET)
    ids_list = SUBSET if vc else list(range(C))
    spans = torch.full((B, TMAX), -1, dtype=torch.long)
    spans[0, 0], spans[0, 3], spans[0, 5] = ids_list[0], ids_list[1], ids_list[-1]
    spans[1, 0], spans[1, 2] = ids_list[1], ids_list[-1]
    spans[2, 0], spans[2, 1] = ids_list[0], ids_list[-1]
    a, b, d = ids_list[0], ids_list[1], ids_list[-1]
    return types.SimpleNamespace(
        x=x, lengths=torch.tensor(LENGTHS), vcpi=[ids] * B if vc else None, cons=cons1 if cons else None,
        cons2=cons2 if cons else None, addl=[{1}, set(), {0}] if addl else None, spans=spans,
        transcripts=[[a, b, d], [b, d], [a, d]], optional=[[0, 1, 0], torch.tensor([1, 0]), [False, False]],
        graphs=lambda ops: _graphs(ops, a, b, d, 2))


def _graphs(ops, a, b, d, other):
    """A candidate trie, a transcript with an optional entry and a chain, none ambiguous.  ``other``: a class of one candidate
    of the trie -- with ``SUBSET`` as the valid classes, or past the classes of a packed video's task, it is no valid class of
    the video (local id -1)."""
    G = ops.TranscriptGraph
    return [G.from_candidates([[a, b, d], [a, d], [a, b, d], [other, d]]), G.from_optional([b, a, d], [0, 1, 0]), G.chain([a, d])]


def _backward(value, *modules):
    for m in modules:
        m.zero_grad(set_to_none=True)
    value.sum().backward()
    return Grads(value, modules)


def padded_entry_points():
    """name -> (the options it accepts, fn(m, other, i, add_eos)).  ``i``: padded_inputs; ``other``: a second module."""
    std = lambda i, eos: (i.x, i.lengths, i.vcpi, eos, i.addl, i.cons)
    checked = lambda m, i: m._check_valid_classes(i.vcpi)
    ep = {}
    all_opts = ('vc', 'eos', 'cons', 'addl')
    ep['_decode.launch'] = (all_opts, lambda m, o, i, eos: m._decode(
        i.x, i.lengths, checked(m, i), i.addl, i.cons, want_elp=True, want_labels=False, no_eos=not eos, spans_on_host=True,
        host_slot=1))
    ep['_decode.probe'] = (('vc', 'cons', 'addl'), lambda m, o, i, eos: m._decode(i.x, i.lengths, checked(m, i), i.addl, i.cons,
                                                                                 want_labels=False))
    ep['_decode.default'] = (('vc', 'cons', 'addl'), lambda m, o, i, eos: m._decode(i.x, i.lengths, checked(m, i), i.addl, i.cons))
    ep['sample'] = (all_opts, lambda m, o, i, eos: m.sample(i.x, i.lengths, i.vcpi, 2, 5, eos, i.addl, i.cons))
    ep['frame_posteriors'] = (all_opts, lambda m, o, i, eos: m.frame_posteriors(*std(i, eos)))
    ep['entropy'] = (all_opts, lambda m, o, i, eos: m.entropy(*std(i, eos)))
    ep['entropy.grad'] = (all_opts, lambda m, o, i, eos: _backward(m.entropy(*std(i, eos), differentiable=True), m))
    for name in ('kl_divergence', 'cross_entropy'):
        for who in ('other', 'self'):
            pick = (lambda m, o: o) if who == 'other' else (lambda m, o: m)
            ep['%s.%s' % (name, who)] = (all_opts, lambda m, o, i, eos, name=name, pick=pick: getattr(m, name)(
                pick(m, o), *std(i, eos), i.cons2))
            ep['%s.%s.grad' % (name, who)] = (all_opts, lambda m, o, i, eos, name=name, pick=pick: _backward(
                getattr(m, name)(pick(m, o), *std(i, eos), i.cons2, differentiable=True), m, o))
    ep['viterbi_kbest'] = (all_opts, lambda m, o, i, eos: m.viterbi_kbest(i.x, i.lengths, i.vcpi, 3, eos, i.addl, i.cons))
    ep['mbr_decode'] = (all_opts, lambda m, o, i, eos: m.mbr_decode(*std(i, eos)))
    ep['align'] = (('vc', 'cons', 'addl'), lambda m, o, i, eos: m.align(i.x, i.lengths, i.vcpi, i.transcripts, True, i.addl, i.cons))
    from action_segmentation_amd import ops
    sup = ('vc', 'cons', 'addl')                 # (the transcript family refuses add_eos=False)
    tail = lambda i: (True, i.addl, i.cons)
    ep['align.optional'] = (sup, lambda m, o, i, eos: m.align(i.x, i.lengths, i.vcpi, i.transcripts, *tail(i), optional=i.optional))
    ep['align_graph'] = (sup, lambda m, o, i, eos: m.align_graph(i.x, i.lengths, i.vcpi, i.graphs(ops), *tail(i)))
    for tag, opt in (('', lambda i: None), ('.optional', lambda i: i.optional)):
        tlp = lambda m, o, i, eos, opt=opt: m.transcript_log_partition(i.x, i.lengths, i.vcpi, i.transcripts, *tail(i),
                                                                       optional=opt(i))
        ep['transcript_log_partition' + tag] = (sup, tlp)
        ep['transcript_log_partition%s.grad' % tag] = (sup, lambda m, o, i, eos, tlp=tlp: _backward(tlp(m, o, i, eos), m))
    tglp = lambda m, o, i, eos: m.transcript_graph_log_partition(i.x, i.lengths, i.vcpi, i.graphs(ops), *tail(i))
    ep['transcript_graph_log_partition'] = (sup, tglp)
    ep['transcript_graph_log_partition.grad'] = (sup, lambda m, o, i, eos: _backward(tglp(m, o, i, eos), m))
    ep['sample_alignments'] = (sup, lambda m, o, i, eos: m.sample_alignments(i.x, i.lengths, i.vcpi, i.graphs(ops), 2, 5, *tail(i)))
    ep['log_partition'] = (all_opts, lambda m, o, i, eos: m.log_partition(i.x, i.lengths, checked(m, i), i.addl, i.cons,
                                                                         no_eos=not eos))
    ep['log_partition.grad'] = (all_opts, lambda m, o, i, eos: _backward(
        m.log_partition(i.x, i.lengths, checked(m, i), i.addl, i.cons, no_eos=not eos), m))
    ep['log_likelihood'] = (all_opts, lambda m, o, i, eos: m.log_likelihood(i.x, i.lengths, i.vcpi, None, eos, False, i.addl, i.cons))
    ep['log_likelihood.spans'] = (all_opts, lambda m, o, i, eos: m.log_likelihood(i.x, i.lengths, i.vcpi, i.spans, eos, False,
                                                                                 i.addl, i.cons))
    ep['log_likelihood.spans.discriminative'] = (all_opts, lambda m, o, i, eos: _discriminative(m, lambda: m.log_likelihood(
        i.x, i.lengths, i.vcpi, i.spans, eos, False, i.addl, i.cons)))
    return ep


def _discriminative(m, fn):
    m.args.sm_train_discriminatively = True
    try:
        return fn()
    finally:
        m.args.sm_train_discriminatively = False


def packed_setup(smm, hard):
    from action_segmentation_amd import synth
    from action_segmentation_amd.batching import make_data_loader, pack_batches
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    data = synth.SynthDatasplit('tiny', seed=12)
    args = synth.make_args(data.max_k, cuda=False, batch_size=2, sm_constrain_transitions=hard,
                           annotate_background_with_previous=hard)
    mods = []
    for seed in (3, 4):
        torch.manual_seed(seed)
        m = SemiMarkovModel.from_args(args, data).model
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            m.gaussian_means.copy_(torch.randn(m.gaussian_means.shape, generator=g) * 0.3)
            m.poisson_log_rates.copy_(torch.rand(m.n_classes, generator=g) + 1.0)
            m.transition_logits.copy_(torch.randn(m.n_classes, m.n_classes, generator=g))
            m.init_logits.copy_(torch.rand(m.n_classes, generator=g))
        mods.append(m)
    batches = list(make_data_loader(args, data, shuffle=False, batch_by_task=True, batch_size=2))
    by_task = {}
    for b in batches:
        by_task.setdefault(b['task_name'][0], b)
    two = [by_task[t] for t in sorted(by_task)[:2]]

    def pack():
        pc = pack_batches(two, 'cpu', mods[0].max_k)
        assert len(pc.groups) == 2
        return pc
    return mods[0], mods[1], pack


def _transcripts(m, pc):
    out = []
    for g in pc.group:
        vc = pc.groups[g]['valid_classes']
        ids = list(range(m.n_classes)) if vc is None else [int(v) for v in vc]
        out.append([ids[0], ids[1], ids[0]])
    return out


def _kl_packed_keeps_pc(m, o, pc, name):
    """(the value, whether ``pc`` is left prepared for ``m`` by the very objects it held before the call)"""
    m.prepare_packed(pc)
    before = (pc.batch, pc.tables, pc.endpen)
    v = getattr(m, name)(o, pc)
    return {'value': v, 'pc_kept': all(a is b for a, b in zip(before, (pc.batch, pc.tables, pc.endpen)))}


def _optional(m, pc):
    return [[0, 1, 0]] * len(pc.group)


def _packed_graphs(m, pc):
    """``_graphs`` over the corpus, turn by turn; the class no video of the task has is one past its valid classes, or past
    every class of the model."""
    from action_segmentation_amd import ops
    out = []
    for v, (g, t) in enumerate(zip(pc.group, _transcripts(m, pc))):
        vc = pc.groups[g]['valid_classes']
        valid = set(range(m.n_classes)) if vc is None else {int(c) for c in vc}
        other = min(c for c in range(m.n_classes + 2) if c not in valid and c != m.n_classes)
        out.append(_graphs(ops, t[0], t[1], t[1], other)[v % 3])
    return out


def _transcript_packed_entry_points():
    """The packed entry points of the transcript family, on a prepared corpus as ``align_packed`` above (all but one read
    ``pc.batch`` before they prepare the corpus)."""
    ep = {}
    pre = lambda m, pc: m.prepare_packed(pc)
    ep['align_packed.optional'] = lambda m, o, pc: m.align_packed(pre(m, pc), _transcripts(m, pc), optional=_optional(m, pc))
    ep['align_graph_packed'] = lambda m, o, pc: m.align_graph_packed(pre(m, pc), _packed_graphs(m, pc))
    for tag, opt in (('', lambda m, pc: None), ('.optional', _optional)):
        tlp = lambda m, o, pc, opt=opt: m.transcript_log_partition_packed(pre(m, pc), _transcripts(m, pc), optional=opt(m, pc))
        ep['transcript_log_partition_packed' + tag] = tlp
        ep['transcript_log_partition_packed%s.grad' % tag] = lambda m, o, pc, tlp=tlp: _backward(tlp(m, o, pc), m)
        for ctag, cond in (('', False), ('.conditional', True)):
            ep['transcript_scores_packed%s%s' % (tag, ctag)] = lambda m, o, pc, opt=opt, cond=cond: m.transcript_scores_packed(
                pre(m, pc), _transcripts(m, pc), conditional=cond, optional=opt(m, pc))
    ep['transcript_entry_posteriors_packed'] = lambda m, o, pc: m.transcript_entry_posteriors_packed(
        pre(m, pc), _transcripts(m, pc), _optional(m, pc))
    tglp = lambda m, o, pc: m.transcript_graph_log_partition_packed(pre(m, pc), _packed_graphs(m, pc))
    ep['transcript_graph_log_partition_packed'] = tglp
    ep['transcript_graph_log_partition_packed.grad'] = lambda m, o, pc: _backward(tglp(m, o, pc), m)
    for ctag, cond in (('', False), ('.conditional', True)):
        ep['transcript_graph_scores_packed' + ctag] = lambda m, o, pc, cond=cond: m.transcript_graph_scores_packed(
            pre(m, pc), _packed_graphs(m, pc), conditional=cond)
    ep['transcript_node_posteriors_packed'] = lambda m, o, pc: m.transcript_node_posteriors_packed(pre(m, pc), _packed_graphs(m, pc))
    ep['sample_alignments_packed'] = lambda m, o, pc: m.sample_alignments_packed(pre(m, pc), _packed_graphs(m, pc), 2, 5)
    return ep


def packed_entry_points():
    ep = {}
    for name, fn in _core_packed_entry_points().items():
        ep[name] = fn
        if name == 'align_packed':                      # (the rest of its family follows it)
            ep.update(_transcript_packed_entry_points())
    return ep


def _core_packed_entry_points():
    return {
        'prepare_packed': lambda m, o, pc: m.prepare_packed(pc),
        'decode_packed.spans': lambda m, o, pc: m.decode_packed(pc, want_spans=True),
        'sample_packed': lambda m, o, pc: m.sample_packed(pc, 2, 5),
        'frame_posteriors_packed': lambda m, o, pc: m.frame_posteriors_packed(pc),
        'entropy_packed': lambda m, o, pc: m.entropy_packed(pc),
        'entropy_packed.grad': lambda m, o, pc: _backward(m.entropy_packed(pc, differentiable=True), m),
        'kl_packed': lambda m, o, pc: _kl_packed_keeps_pc(m, o, pc, 'kl_packed'),
        'cross_entropy_packed': lambda m, o, pc: _kl_packed_keeps_pc(m, o, pc, 'cross_entropy_packed'),
        'kbest_packed': lambda m, o, pc: m.kbest_packed(pc, 3),
        'mbr_decode_packed': lambda m, o, pc: m.mbr_decode_packed(pc),
        # (align_packed reads pc.batch.no_eos before it prepares the corpus: the corpus comes prepared)
        'align_packed': lambda m, o, pc: m.align_packed(m.prepare_packed(pc), _transcripts(m, pc)),
        'log_partition_packed': lambda m, o, pc: m.log_partition_packed(pc),
        'log_partition_packed.grad': lambda m, o, pc: _backward(m.log_partition_packed(pc), m),
    }


def cases(smm):
    """[(case id, thunk)]: every entry point over the product of the options it accepts, on a module with hard masks (H1) and
    one without (H0); ``log_partition`` also on a max_k = 1 module (K1); the packed entry points on a two-group corpus."""
    out = []
    mods = {h: (padded_module(smm, h, 1), padded_module(smm, h, 2)) for h in (False, True)}
    k1 = padded_module(smm, False, 1, max_k=1)
    for name, (opts, fn) in padded_entry_points().items():
        axes = [(False, True) if o in opts else (None,) for o in ('vc', 'eos', 'cons', 'addl')]
        runs = [('H%d' % h,) + mods[h] for h in (False, True)]
        if name.startswith('log_partition'):
            runs.append(('K1', k1, k1))
        for (tag, m, o), (vc, eos, cons, addl) in itertools.product(runs, itertools.product(*axes)):
            if addl and m.allowed_ends is None:
                continue                # (additional ends are read only next to the module's own allowed ends: a duplicate case)
            cid = '%s|%s|%s' % (name, tag, ''.join('%s%s' % (k, '-' if v is None else int(v)) for k, v in
                                                   (('v', vc), ('e', eos), ('c', cons), ('a', addl))))
            i = padded_inputs(bool(vc), bool(cons), bool(addl))
            out.append((cid, lambda fn=fn, m=m, o=o, i=i, eos=True if eos is None else eos: fn(m, o, i, eos)))
    for hard in (False, True):
        m, o, pack = packed_setup(smm, hard)
        for name, fn in packed_entry_points().items():
            out.append(('%s|H%d' % (name, hard), lambda fn=fn, m=m, o=o, pack=pack: fn(m, o, pack())))
    return out


def row(cid, tr):
    """What the table keeps of one case's trace."""
    dig = lambda v: _sha(json.dumps(v, sort_keys=True, separators=(',', ':')).encode())[:8]
    r = {'case': cid, 'calls': ['%s:%s' % (c['launcher'], dig(c)) for c in tr['calls']], 'result': dig(tr['result'])}
    if 'grads' in tr:
        r['grads'] = dig(tr['grads'])
    return r


def main():
    from action_segmentation_amd import semimarkov_modules as smm
    if len(sys.argv) > 2 and sys.argv[1] == '--show':
        thunk = dict(cases(smm))[sys.argv[2]]
        print(json.dumps(trace(smm, thunk), indent=1, sort_keys=True))
        return
    table = [row(cid, trace(smm, thunk)) for cid, thunk in cases(smm)]
    with open(OUT, 'w') as f:
        f.write('[\n' + ',\n'.join(json.dumps(r, separators=(',', ':')) for r in table) + '\n]\n')
    print('%d cases -> %s' % (len(table), OUT))


if __name__ == '__main__':
    main()
