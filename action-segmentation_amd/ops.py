"""Tensor-level wrappers of the libsmmdp C ABI (include/smmdp.h).

Every function takes CUDA(=HIP) tensors for bulk data and host sequences for the per-video / per-group
metadata, enqueues on torch's current stream and returns CUDA tensors.  Nothing here computes on the CPU.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import SmmShape


class Batch:
    """Metadata of one ragged decode batch (host side).

    lengths        frames per video
    frame_offset   first frame of each video on the packed frame axis (default: padded, i * t_max)
    group          parameter group per video (default 0)
    kp             per-video min(K, Tmax of its reference batch) (reference semimarkov_modules.py:450-452)
    n_states       states per group
    no_eos         add_eos=False of the reference: no EOS label, the last frame's label only emits
    no_time_split  the tables carry hard masks (ordering constraints): long videos are decoded in one piece
                   (include/smmdp.h: SMM_SHAPE_NO_TIME_SPLIT)
    """

    def __init__(self, lengths, n_states, k_rows, c_max=None, frame_offset=None, group=None, kp=None, d=0,
                 t_max=None, total_frames=None, no_eos=False, no_time_split=False):
        self.lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
        self.b = int(self.lengths.shape[0])
        self.n_states = np.ascontiguousarray(np.asarray(n_states, dtype=np.int32).reshape(-1))
        self.n_groups = int(self.n_states.shape[0])
        self.c_max = int(c_max if c_max is not None else self.n_states.max())
        self.k_rows = int(k_rows)
        self.t_max = int(t_max if t_max is not None else self.lengths.max())
        if frame_offset is None:
            frame_offset = np.arange(self.b, dtype=np.int64) * self.t_max
        self.frame_offset = np.ascontiguousarray(np.asarray(frame_offset, dtype=np.int64).reshape(-1))
        self.group = None if group is None else np.ascontiguousarray(np.asarray(group, dtype=np.int32).reshape(-1))
        self.kp = None if kp is None else np.ascontiguousarray(np.asarray(kp, dtype=np.int32).reshape(-1))
        if total_frames is None:
            total_frames = int((self.frame_offset + self.lengths).max())
        self.total_frames = int(total_frames)
        self.d = int(d)
        self.no_eos = bool(no_eos)     # add_eos=False of the reference (include/smmdp.h: SMM_SHAPE_NO_EOS)
        self.shape = SmmShape(self.b, self.d, self.n_groups, self.c_max, self.k_rows, self.t_max,
                              (_lib.SHAPE_NO_EOS if self.no_eos else 0) | (_lib.SHAPE_NO_TIME_SPLIT if no_time_split else 0),
                              self.total_frames)

    def workspace_bytes(self):
        n = _lib.load().smm_workspace_bytes(ctypes.byref(self.shape), self.lengths.ctypes.data)
        if n == 0:
            raise _lib.SmmError("libsmmdp: invalid batch shape")
        return n

    def host_ptrs(self):
        return (self.lengths.ctypes.data, self.frame_offset.ctypes.data,
                None if self.group is None else self.group.ctypes.data,
                None if self.kp is None else self.kp.ctypes.data, self.n_states.ctypes.data)

    def head(self, extra_flags=0, with_kp=True):
        """The leading arguments of an entry point as ctypes values: the smm_shape -- with extra SMM_SHAPE_* bits for this one
        call -- and the host arrays (lengths, frame_offset, group, kp, n_states; the emission pair takes no kp)."""
        s = self.shape
        if extra_flags:
            s = SmmShape(s.b, s.d, s.n_groups, s.c_max, s.k_rows, s.t_max, s.flags | extra_flags, s.total_frames)
        ln, fo, gr, kp, ns = self.host_ptrs()
        p = ctypes.c_void_p
        return (ctypes.byref(s), p(ln), p(fo), p(gr)) + ((p(kp),) if with_kp else ()) + (p(ns),)


def _dev(t, dtype, name):
    if t is None:
        return None
    if not t.is_cuda and not (name in ('labels', 'spans') and t.is_pinned()):
        raise _lib.SmmError("libsmmdp: %s must be a CUDA/HIP tensor (there is no CPU path)" % name)
    if t.dtype != dtype:
        raise TypeError("%s: expected %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return ctypes.c_void_p(t.data_ptr())


def _ws_args(ws):
    """A workspace (or scratch) tensor as the C ABI takes it: pointer, bytes."""
    return ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(ws.numel())


def _raw_stream():
    """Handle of torch's current stream on the current device, by the C-level getters (torch.cuda.current_stream() builds a
    Stream object and resolves the device through three python layers: ~10 us, twice per call, of a 150 us viterbi())."""
    get = getattr(torch._C, '_cuda_getCurrentRawStream', None)
    if get is None:                                    # (a torch build without the C-level getter)
        return torch.cuda.current_stream().cuda_stream
    return get(torch._C._cuda_getDevice())


def _stream():
    return ctypes.c_void_p(_raw_stream())


_ws_cache = {}


def workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream).  (Caller-owned from the library's point of view.)"""
    key = (device.index, _raw_stream())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


_host_labels = {}


def _labels_on_host(batch, device):
    """Pinned host buffer the DP kernel writes the frame labels into directly (host-pinned memory is mapped into the
    GPU's address space on ROCm; the stores go over PCIe while the kernel is still decoding other videos, so there is
    no separate device -> host copy at the end).  Valid after the stream has been synchronised, until the next call."""
    buf = _host_labels.get(device.index)
    if buf is None or buf.numel() < batch.total_frames:
        buf = torch.empty(int(batch.total_frames * 1.25) + 16, dtype=torch.int64, pin_memory=True)
        _host_labels[device.index] = buf
    out = buf[:batch.total_frames]
    if int(batch.lengths.sum()) != batch.total_frames:
        out.fill_(-1)                                  # frames no video covers (padded layouts) keep the -1 filler
    return out


_host_small = {}


def _pinned_small(kind, device, numel, dtype):
    """Small pinned host buffers the kernels (spans) or an async copy (error words) write into: the reference's call
    pattern -- one viterbi() per batch of five videos -- is host latency, and every blocking device -> host copy is ~50 us
    of it.  Valid after the stream has been synchronised, until the next call."""
    key = (kind, device.index, dtype)
    buf = _host_small.get(key)
    if buf is None or buf.numel() < numel:
        buf = torch.empty(int(numel * 1.5) + 16, dtype=dtype, pin_memory=True)
        _host_small[key] = buf
    return buf[:numel]


def pinned_labels(kind, device, numel):
    """A pinned int64 label buffer per (kind, device): the DP kernel's label stores land in it (see _labels_on_host); valid after
    the launch's stream has been synchronised, until the next launch that asks for the same kind."""
    return _pinned_small(('labels',) + tuple(kind), device, numel, torch.int64)


_label_leases = {}
LABEL_LEASES = 3      # pinned label buffers per device that can be out on lease at once


def _storage_users(t):
    """How many tensors (and numpy arrays made from them) share ``t``'s storage, ``t`` included; None if this torch build
    cannot tell (then nothing is ever leased)."""
    fn = getattr(torch._C, '_storage_Use_Count', None)
    return None if fn is None else fn(t.untyped_storage()._cdata)


def lease_host_labels(batch, device):
    """A pinned int64 [total_frames] label buffer that belongs to the CALLER for as long as the returned tensor -- or
    anything that shares its storage, such as the numpy arrays of ``SemiMarkovModel.predict`` -- is alive; pass it as
    ``labels_out``.  The buffer is free again when the last of them has died (the storage's use count tells: a numpy array
    made from a tensor keeps a NEW tensor object alive, not the one it was made from, so a weak reference would not), i.e. a
    caller that drops its result before the next decode keeps reusing one buffer and never copies 8 bytes per frame out of a
    staging buffer (cfg3: 20 MB).  At most LABEL_LEASES buffers per device are out at once: None when all are (the caller
    then decodes into the shared staging buffer and copies, as before)."""
    pool = _label_leases.setdefault(device.index, [])
    n = batch.total_frames
    entry = None
    for e in pool:
        if _storage_users(e[0]) == e[1]:               # nobody but the pool holds it
            entry = e
            if e[0].numel() >= n:
                break
    if entry is None or entry[0].numel() < n:
        if entry is None and len(pool) >= LABEL_LEASES:
            return None
        buf = torch.empty(int(n * 1.25) + 16, dtype=torch.int64, pin_memory=True)
        users = _storage_users(buf)
        if users is None:
            return None
        if entry is None:
            entry = [buf, users]
            pool.append(entry)
        else:
            entry[0], entry[1] = buf, users
    out = entry[0][:n]
    if int(batch.lengths.sum()) != n:
        out.fill_(-1)                                  # frames no video covers (padded layouts) keep the -1 filler
    return out


def _outputs(batch, device, want_spans, want_labels, labels_on_host=False, labels_out=None, spans_on_host=False, host_slot=0):
    if want_spans and spans_on_host:
        spans = _pinned_small(('spans', host_slot), device, batch.b * (batch.t_max + 1), torch.int64).view(batch.b, batch.t_max + 1)
    else:
        spans = torch.empty((batch.b, batch.t_max + 1), dtype=torch.int64, device=device) if want_spans else None
    if labels_out is not None:
        labels = labels_out
    elif want_labels and labels_on_host:
        labels = _labels_on_host(batch, device)
    else:
        labels = torch.full((batch.total_frames,), -1, dtype=torch.int64, device=device) if want_labels else None
    best = torch.empty(batch.b, dtype=torch.float64, device=device)
    n_segs = torch.empty(batch.b, dtype=torch.int32, device=device)
    return spans, labels, best, n_segs


def _device_outputs(batch, device, want_spans, want_labels, lead=()):
    """spans / labels (-1 on frames no video covers) / an fp64 and an int32 value per video, all on the device, of ``sample``,
    ``kbest``, ``mbr`` and ``align``; ``lead``: the leading [n_samples] / [k] dimension."""
    spans = torch.empty(lead + (batch.b, batch.t_max + 1), dtype=torch.int64, device=device) if want_spans else None
    labels = torch.full(lead + (batch.total_frames,), -1, dtype=torch.int64, device=device) if want_labels else None
    best = torch.empty(lead + (batch.b,), dtype=torch.float64, device=device)
    n_segs = torch.empty(lead + (batch.b,), dtype=torch.int32, device=device)
    return spans, labels, best, n_segs


def _grad_outputs(elp, trans, init, len_scores):
    return dict(elp=torch.empty_like(elp), trans=torch.empty_like(trans), init=torch.empty_like(init),
                len=torch.empty_like(len_scores))


def _own_workspace(ws, need, device):
    """``ws`` if the caller gave one that is large enough, else a private one of ``need`` bytes for this call."""
    if ws is None or ws.numel() < need:
        ws = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def emission(batch, x, w, cst, inv_var, cons=None, want64=True, want32=False, out64=None):
    """x fp32 [total_frames, d] -> elp fp64 and/or fp32 [total_frames, c_max].  (smm_emission_f64)
    ``out64``: write into this [total_frames, c_max] tensor (sub-batches of one packed frame axis share it)."""
    lib = _lib.load()
    dev = x.device
    elp64 = out64 if out64 is not None else (
        torch.empty((batch.total_frames, batch.c_max), dtype=torch.float64, device=dev) if want64 else None)
    elp32 = torch.zeros((batch.total_frames, batch.c_max), dtype=torch.float32, device=dev) if want32 else None
    ws = workspace(batch.workspace_bytes(), dev)
    _lib.check(lib.smm_emission_f64(
        *batch.head(with_kp=False), _dev(x, torch.float32, 'x'), _dev(w, torch.float64, 'w'), _dev(cst, torch.float64, 'cst'),
        _dev(inv_var, torch.float64, 'inv_var'), _dev(cons, torch.float32, 'cons'),
        _dev(elp64, torch.float64, 'elp64'), _dev(elp32, torch.float32, 'elp32'), *_ws_args(ws), _stream()))
    return elp64, elp32


def emission_bwd(batch, x, g_elp, ws=None):
    """Chain rule through the emission scorer (smm_emission_bwd_f64): g_elp fp64 [total_frames, c_max] ->
    (g_w [n_groups, d, c_max] (a transposed view of the kernel's class-major output), g_cst [n_groups, c_max],
    g_inv_var [d]), all fp64."""
    lib = _lib.load()
    dev = x.device
    f64 = torch.float64
    g, cm, d = batch.n_groups, batch.c_max, int(x.size(1))
    if d != batch.d or x.size(0) < batch.total_frames or tuple(g_elp.shape) != (batch.total_frames, cm):
        raise ValueError("emission_bwd: x [>= total_frames, batch.d] and g_elp [total_frames, c_max] expected")
    g_w = torch.empty((g, cm, d), dtype=f64, device=dev)
    g_cst = torch.empty((g, cm), dtype=f64, device=dev)
    g_iv = torch.empty(d, dtype=f64, device=dev)
    if ws is None:
        ws = workspace(batch.workspace_bytes(), dev)
    _lib.check(lib.smm_emission_bwd_f64(
        *batch.head(with_kp=False), _dev(x, torch.float32, 'x'), _dev(g_elp, f64, 'g_elp'), _dev(g_w, f64, 'g_w'),
        _dev(g_cst, f64, 'g_cst'), _dev(g_iv, f64, 'g_inv_var'), *_ws_args(ws), _stream()))
    return g_w.transpose(1, 2), g_cst, g_iv


def emission_bwd_x(batch, x, g_elp, w, inv_var, ws=None):
    """The gradient of the emission scores with respect to the features (smm_emission_bwd_x_f64): g_elp fp64
    [total_frames, c_max], w fp64 [n_groups, d, c_max] and inv_var fp64 [d] (``emission``'s) -> g_x fp32 [total_frames, d];
    rows no video covers are 0."""
    lib = _lib.load()
    dev = x.device
    f64 = torch.float64
    g, cm, d = batch.n_groups, batch.c_max, int(x.size(1))
    if d != batch.d or x.size(0) < batch.total_frames or tuple(g_elp.shape) != (batch.total_frames, cm) or \
            tuple(w.shape) != (g, d, cm) or tuple(inv_var.shape) != (d,):
        raise ValueError("emission_bwd_x: x [>= total_frames, batch.d], g_elp [total_frames, c_max], w [n_groups, d, c_max] and "
                         "inv_var [d] expected")
    g_x = torch.empty((batch.total_frames, d), dtype=torch.float32, device=dev)
    if ws is None:
        ws = workspace(batch.workspace_bytes(), dev)
    _lib.check(lib.smm_emission_bwd_x_f64(
        *batch.head(with_kp=False), _dev(x, torch.float32, 'x'), _dev(g_elp, f64, 'g_elp'), _dev(w, f64, 'w'),
        _dev(inv_var, f64, 'inv_var'), _dev(g_x, torch.float32, 'g_x'), *_ws_args(ws), _stream()))
    return g_x


class FlowShape:
    """Sizes of a NICE coupling flow (include/smmdp.h: smm_flow_shape, without the row count): feature dimension ``d``,
    ``hidden_units``, ``hidden_layers`` and ``couple_layers``."""

    def __init__(self, d, hidden_units=100, hidden_layers=1, couple_layers=4):
        self.d, self.hidden_units = int(d), int(hidden_units)
        self.hidden_layers, self.couple_layers = int(hidden_layers), int(couple_layers)

    @property
    def layer_sizes(self):
        """(in_features, out_features) of the linear layers of one coupling layer, in packing order."""
        dh, h = self.d // 2, self.hidden_units
        return [(dh, h)] + [(h, h)] * self.hidden_layers + [(h, dh)]

    @property
    def n_params(self):
        return self.couple_layers * sum(i * o + o for i, o in self.layer_sizes)

    def c_shape(self, n_rows):
        return _lib.SmmFlowShape(int(n_rows), self.d, self.hidden_units, self.hidden_layers, self.couple_layers)


def _flow_operands(x, packed, shape, what):
    if x.dim() != 2 or int(x.size(1)) != shape.d:
        raise ValueError("%s: x [n_rows, %d] expected, got %s" % (what, shape.d, tuple(x.shape)))
    if packed.dim() != 1 or packed.numel() != shape.n_params:
        raise ValueError("%s: %d packed parameters expected, got %s" % (what, shape.n_params, tuple(packed.shape)))


def flow(x, packed, shape):
    """y = flow(x) row by row (smm_flow_f32): x fp32 [n_rows, d], ``packed`` the flow's parameters in the ABI's layout
    (flow.FeatureProjector.packed), ``shape`` a FlowShape -> y fp32 [n_rows, d]."""
    lib = _lib.load()
    _flow_operands(x, packed, shape, 'flow')
    px, pp = _dev(x, torch.float32, 'x'), _dev(packed, torch.float32, 'packed')
    y = torch.empty_like(x)
    if x.size(0) == 0:
        return y
    _lib.check(lib.smm_flow_f32(ctypes.byref(shape.c_shape(x.size(0))), px, pp, _dev(y, torch.float32, 'y'),
                                None, ctypes.c_size_t(0), _stream()))
    return y


def flow_bwd(x, g_y, packed, shape, want_g_x=False):
    """Chain rule through ``flow`` (smm_flow_bwd_f32; the activations are computed again): g_y fp32 [n_rows, d] ->
    (g_packed fp64 [n_params] in the packed layout, g_x fp32 [n_rows, d] or None)."""
    lib = _lib.load()
    _flow_operands(x, packed, shape, 'flow_bwd')
    if tuple(g_y.shape) != tuple(x.shape):
        raise ValueError("flow_bwd: g_y of x's shape expected")
    px, pg, pp = _dev(x, torch.float32, 'x'), _dev(g_y, torch.float32, 'g_y'), _dev(packed, torch.float32, 'packed')
    dev = x.device
    g_packed = torch.empty(shape.n_params, dtype=torch.float64, device=dev)
    g_x = torch.empty_like(x) if want_g_x else None
    if x.size(0) == 0:
        return g_packed.zero_(), g_x
    cs = shape.c_shape(x.size(0))
    need = lib.smm_flow_bwd_scratch_bytes(ctypes.byref(cs))
    if need == 0:
        raise _lib.SmmError("libsmmdp: flow shape not supported (include/smmdp.h: smm_flow_shape)")
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    _lib.check(lib.smm_flow_bwd_f32(ctypes.byref(cs), px, pg, pp, _dev(g_packed, torch.float64, 'g_params'),
                                    _dev(g_x, torch.float32, 'g_x'), *_ws_args(scratch), _stream()))
    return g_packed, g_x


class TablesMeta:
    """Which class sets a launch's parameter groups are (device index tensors, built once per PackedCorpus):
    classes / merged int64 [g, c_max], n_states int32 [g]; plus the scalars of smm_tables_shape."""

    def __init__(self, classes, merged, n_states, n_classes, d, k_rows, allow_self_transitions):
        self.classes, self.merged, self.n_states = classes, merged, n_states
        g, cm = classes.shape
        self.g, self.cm, self.n, self.d, self.k_rows = int(g), int(cm), int(n_classes), int(d), int(k_rows)
        self.shape = _lib.SmmTablesShape(self.n, self.d, self.g, self.cm, self.k_rows, 1 if allow_self_transitions else 0)


def _u8(t, name):
    if t is None:
        return None
    if not t.is_cuda or not t.is_contiguous() or t.element_size() != 1:
        raise ValueError("%s: a contiguous 1-byte device tensor is expected" % name)
    return ctypes.c_void_p(t.data_ptr())


def factor_tables(meta, init_logits, transition_logits, poisson_log_rates, gaussian_means, gaussian_cov,
                  init_constraints=None, transition_constraints=None):
    """fp32 parameters -> fp64 tables of every group (smm_factor_tables_f64):
    dict(trans [g,cm,cm], init [g,cm], len [g,K,cm], w [g,d,cm], cst [g,cm], inv_var [d])."""
    lib = _lib.load()
    dev, f64, f32 = init_logits.device, torch.float64, torch.float32
    g, cm, d, k = meta.g, meta.cm, meta.d, meta.k_rows
    if tuple(gaussian_means.shape) != (meta.n, d) or tuple(gaussian_cov.shape) != (d, d) or \
            tuple(transition_logits.shape) != (meta.n, meta.n):
        raise ValueError("factor_tables: parameter shapes do not match the TablesMeta")
    t = dict(trans=torch.empty((g, cm, cm), dtype=f64, device=dev), init=torch.empty((g, cm), dtype=f64, device=dev),
             len=torch.empty((g, k, cm), dtype=f64, device=dev), w=torch.empty((g, d, cm), dtype=f64, device=dev),
             cst=torch.empty((g, cm), dtype=f64, device=dev), inv_var=torch.empty(d, dtype=f64, device=dev))
    _lib.check(lib.smm_factor_tables_f64(
        ctypes.byref(meta.shape), _dev(init_logits, f32, 'init_logits'), _dev(transition_logits, f32, 'transition_logits'),
        _dev(poisson_log_rates, f32, 'poisson_log_rates'), _dev(gaussian_means, f32, 'gaussian_means'),
        _dev(gaussian_cov, f32, 'gaussian_cov'), _u8(init_constraints, 'init_constraints'),
        _u8(transition_constraints, 'transition_constraints'), _dev(meta.classes, torch.int64, 'classes'),
        _dev(meta.merged, torch.int64, 'merged'), _dev(meta.n_states, torch.int32, 'n_states'),
        _dev(t['trans'], f64, 'trans'), _dev(t['init'], f64, 'init'), _dev(t['len'], f64, 'len'), _dev(t['w'], f64, 'w'),
        _dev(t['cst'], f64, 'cst'), _dev(t['inv_var'], f64, 'inv_var'), _stream()))
    return t


def factor_tables_bwd(meta, poisson_log_rates, gaussian_means, gaussian_cov, trans, init, g_trans, g_init, g_len,
                      g_w_class_major, g_cst, init_constraints=None, transition_constraints=None):
    """Gradients of the tables -> fp64 gradients of (init_logits [n], transition_logits [n,n], poisson_log_rates [n],
    gaussian_means [n,d])  (smm_factor_tables_bwd_f64).  g_w_class_major: [g, c_max, d]."""
    lib = _lib.load()
    dev, f64, f32 = trans.device, torch.float64, torch.float32
    n, d = meta.n, meta.d
    # (one flat buffer, four views: the caller converts the gradients to the parameters' dtype in ONE launch -- flat_of)
    flat = torch.empty(2 * n + n * n + n * d, dtype=f64, device=dev)
    out = (flat[:n], flat[n:n + n * n].view(n, n), flat[n + n * n:2 * n + n * n], flat[2 * n + n * n:].view(n, d))
    _lib.check(lib.smm_factor_tables_bwd_f64(
        ctypes.byref(meta.shape), _dev(poisson_log_rates, f32, 'poisson_log_rates'), _dev(gaussian_means, f32, 'gaussian_means'),
        _dev(gaussian_cov, f32, 'gaussian_cov'), _u8(init_constraints, 'init_constraints'),
        _u8(transition_constraints, 'transition_constraints'), _dev(meta.classes, torch.int64, 'classes'),
        _dev(meta.merged, torch.int64, 'merged'), _dev(meta.n_states, torch.int32, 'n_states'),
        _dev(trans, f64, 'trans'), _dev(init, f64, 'init'), _dev(g_trans, f64, 'g_trans'), _dev(g_init, f64, 'g_init'),
        _dev(g_len, f64, 'g_len'), _dev(g_w_class_major, f64, 'g_w'), _dev(g_cst, f64, 'g_cst'),
        _dev(out[0], f64, 'g_init_logits'), _dev(out[1], f64, 'g_transition_logits'), _dev(out[2], f64, 'g_poisson_log_rates'),
        _dev(out[3], f64, 'g_gaussian_means'), _stream()))
    return out + (flat,)


def viterbi(batch, elp, trans, init, len_scores, endpen=None, class_map=None, want_spans=True, want_labels=True,
            labels_on_host=False, labels_out=None):
    """Viterbi on emission scores.  elp fp64 (smm_viterbi_f64) or fp32 (smm_viterbi_f32, tables fp32 too).
    ``labels_on_host``: the kernel writes the frame labels straight into pinned host memory (see _labels_on_host);
    synchronise the stream before reading them."""
    lib = _lib.load()
    dev = elp.device
    dt = elp.dtype
    fn = lib.smm_viterbi_f64 if dt == torch.float64 else lib.smm_viterbi_f32
    spans, labels, best, n_segs = _outputs(batch, dev, want_spans, want_labels, labels_on_host, labels_out)
    ws = workspace(batch.workspace_bytes(), dev)
    _lib.check(fn(
        *batch.head(), _dev(elp, dt, 'elp'), _dev(trans, dt, 'trans'), _dev(init, dt, 'init'),
        _dev(len_scores, dt, 'len_scores'), _dev(endpen, dt, 'endpen'), _dev(class_map, torch.int64, 'class_map'),
        _dev(spans, torch.int64, 'spans'), _dev(labels, torch.int64, 'labels'), _dev(best, torch.float64, 'best'),
        _dev(n_segs, torch.int32, 'n_segs'), *_ws_args(ws), _stream()))
    return dict(spans=spans, labels=labels, best=best, n_segs=n_segs, _err=_err_copy(batch, ws))


def decode(batch, x, w, cst, inv_var, trans, init, len_scores, cons=None, endpen=None, class_map=None,
           want_spans=True, want_labels=True, want_elp=False, labels_on_host=False, labels_out=None, spans_on_host=False,
           host_slot=0):
    """Features -> spans / labels in one call (smm_decode_f32): emission kernel + DP kernel on the current stream.
    ``labels_on_host`` / ``labels_out``: see ``viterbi``.  ``spans_on_host``: the kernel writes the span encoding into
    pinned host memory and the error words follow by an asynchronous copy (small batches: the reference's per-batch call
    pattern); both are valid once the stream has been synchronised, until the next such call with the same ``host_slot``
    (a caller that keeps two decodes in flight alternates two slots)."""
    lib = _lib.load()
    dev = x.device
    spans, labels, best, n_segs = _outputs(batch, dev, want_spans, want_labels, labels_on_host, labels_out, spans_on_host,
                                           host_slot)
    elp32 = torch.zeros((batch.total_frames, batch.c_max), dtype=torch.float32, device=dev) if want_elp else None
    ws = workspace(batch.workspace_bytes(), dev)
    f64 = torch.float64
    _lib.check(lib.smm_decode_f32(
        *batch.head(), _dev(x, torch.float32, 'x'), _dev(w, f64, 'w'), _dev(cst, f64, 'cst'),
        _dev(inv_var, f64, 'inv_var'), _dev(cons, torch.float32, 'cons'), _dev(trans, f64, 'trans'),
        _dev(init, f64, 'init'), _dev(len_scores, f64, 'len_scores'), _dev(endpen, f64, 'endpen'),
        _dev(class_map, torch.int64, 'class_map'), _dev(spans, torch.int64, 'spans'),
        _dev(labels, torch.int64, 'labels'), _dev(best, f64, 'best'), _dev(n_segs, torch.int32, 'n_segs'),
        _dev(elp32, torch.float32, 'elp32'), *_ws_args(ws), _stream()))
    if spans_on_host:
        err = _pinned_small(('err', host_slot), dev, 8, torch.int32)
        err.copy_(_err_view(batch, ws), non_blocking=True)
    else:
        err = _err_copy(batch, ws)
    return dict(spans=spans, labels=labels, best=best, n_segs=n_segs, elp=elp32, _err=err)


class ResidentDecode:
    """``decode`` for a packed corpus that is decoded again and again (the training loop's per-epoch decode, bench.py's step):
    the call's FIXED arguments -- shape, the five metadata arrays, features, tables, constraints, end penalties, class map --
    are validated and turned into ctypes values once; a call then marshals three pointers (labels, workspace, stream) instead
    of eighteen (round 4 measured 25-35 us of python per ``decode`` call in front of the library's own 10-36 us).  Frame
    labels only (no spans, no emission copy); ``best`` / ``n_segs`` are the object's own buffers, overwritten by every call.
    The tensors are kept referenced; ``key`` lets the owner notice that the tables were rebuilt."""

    def __init__(self, batch, x, w, cst, inv_var, trans, init, len_scores, cons=None, endpen=None, class_map=None):
        self.lib = _lib.load()
        self.batch = batch
        dev = x.device
        f64 = torch.float64
        self.keep = (x, w, cst, inv_var, trans, init, len_scores, cons, endpen, class_map)
        self.key = tuple(None if t is None else (t.data_ptr(), t._version) for t in self.keep)
        self.best = torch.empty(batch.b, dtype=f64, device=dev)
        self.n_segs = torch.empty(batch.b, dtype=torch.int32, device=dev)
        self.head = (*batch.head(), _dev(x, torch.float32, 'x'), _dev(w, f64, 'w'), _dev(cst, f64, 'cst'),
                     _dev(inv_var, f64, 'inv_var'), _dev(cons, torch.float32, 'cons'), _dev(trans, f64, 'trans'),
                     _dev(init, f64, 'init'), _dev(len_scores, f64, 'len_scores'), _dev(endpen, f64, 'endpen'),
                     _dev(class_map, torch.int64, 'class_map'), None)
        self.tail = (_dev(self.best, f64, 'best'), _dev(self.n_segs, torch.int32, 'n_segs'), None)
        self.ws_bytes = batch.workspace_bytes()
        self.dev = dev

    def __call__(self, labels_on_host=False, labels_out=None):
        batch = self.batch
        if labels_out is not None:
            labels = labels_out
        elif labels_on_host:
            labels = _labels_on_host(batch, self.dev)
        else:
            labels = torch.full((batch.total_frames,), -1, dtype=torch.int64, device=self.dev)
        ws = workspace(self.ws_bytes, self.dev)
        _lib.check(self.lib.smm_decode_f32(*self.head, _dev(labels, torch.int64, 'labels'), *self.tail, *_ws_args(ws), _stream()))
        return dict(spans=None, labels=labels, best=self.best, n_segs=self.n_segs, elp=None, _err=_err_copy(batch, ws))


def logz(batch, elp, trans, init, len_scores, endpen=None, ws=None, with_backward=False):
    """Log-partition per video (smm_logz_f64).  elp fp64 [total_frames, c_max] -> logZ fp64 [b].
    ``ws``: a private uint8 workspace tensor (keep it for ``logz_bwd``); default: the shared per-stream one.
    ``with_backward``: run the time-reversed recursion in the same launch (SMM_SHAPE_LOGZ_BOTH); pass the same to
    ``logz_bwd``."""
    lib = _lib.load()
    head = batch.head(_lib.SHAPE_LOGZ_BOTH if with_backward else 0)
    dev = elp.device
    f64 = torch.float64
    out = torch.empty(batch.b, dtype=f64, device=dev)
    if ws is None:
        ws = workspace(batch.workspace_bytes(), dev)
    _lib.check(lib.smm_logz_f64(
        *head, *_tables(elp, trans, init, len_scores, endpen), _dev(out, f64, 'logz'), *_ws_args(ws), _stream()))
    return out


def logz_bwd(batch, elp, trans, init, len_scores, logz_val, grad_logz=None, endpen=None, ws=None, with_backward=False):
    """Gradient of sum_i grad_logz[i] * logZ_i (smm_logz_bwd_f64).  Must follow ``logz`` for the same batch with the
    same workspace (same device + stream).  -> dict(elp [total_frames, c_max], trans, init, len) fp64.
    ``with_backward``: ``logz`` was called with it (the backward messages are already in the workspace)."""
    lib = _lib.load()
    head = batch.head(_lib.SHAPE_LOGZ_BOTH if with_backward else 0)
    dev = elp.device
    f64 = torch.float64
    g = _grad_outputs(elp, trans, init, len_scores)
    if ws is None:
        ws = workspace(batch.workspace_bytes(), dev)
    _lib.check(lib.smm_logz_bwd_f64(
        *head, *_tables(elp, trans, init, len_scores, endpen), _dev(logz_val, f64, 'logz'), _dev(grad_logz, f64, 'grad_logz'),
        _dev(g['elp'], f64, 'g_elp'), _dev(g['trans'], f64, 'g_trans'), _dev(g['init'], f64, 'g_init'), _dev(g['len'], f64, 'g_len'),
        *_ws_args(ws), _stream()))
    return g


def sample(batch, elp, trans, init, len_scores, logz_val, n_samples, seed=0, endpen=None, class_map=None, ws=None,
           want_spans=True, want_labels=False, with_backward=False):
    """Segmentations drawn from the posterior p(y | x) (smm_sample_f64).  Must follow ``logz`` for the same batch and tables
    with the same workspace (``with_backward``: as passed to ``logz``); ``logz_val`` = its output.  Returns dict(spans int64
    [n_samples, b, t_max+1] (span encoding, class map applied) or None, labels int64 [n_samples, total_frames] (global ids, -1
    on frames no video covers) or None, logp fp64 [n_samples, b]: exact log p(sample | x)).  Sample j depends on
    (seed, video, j) only."""
    lib = _lib.load()
    n_samples = int(n_samples)
    if n_samples <= 0:
        raise ValueError("n_samples must be positive, got %d" % n_samples)
    head = batch.head(_lib.SHAPE_LOGZ_BOTH if with_backward else 0)
    dev = elp.device
    f64 = torch.float64
    spans, labels, logp, _ = _device_outputs(batch, dev, want_spans, want_labels, (n_samples,))
    if ws is None:
        ws = workspace(batch.workspace_bytes(), dev)
    _lib.check(lib.smm_sample_f64(
        *head, *_tables(elp, trans, init, len_scores, endpen), _dev(class_map, torch.int64, 'class_map'), _dev(logz_val, f64, 'logz'),
        ctypes.c_int32(n_samples), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _dev(spans, torch.int64, 'spans'),
        _dev(labels, torch.int64, 'labels'), _dev(logp, f64, 'logp'), *_ws_args(ws), _stream()))
    return dict(spans=spans, labels=labels, logp=logp, _err=_err_copy(batch, ws))



def entropy(batch, elp, trans, init, len_scores, logz_val, endpen=None, ws=None, with_backward=False):
    """Exact entropy H(y | x) of each video's segmentation posterior in nats (smm_entropy_f64): fp64 [b].  Must follow
    ``logz`` for the same batch and tables with the same workspace (``with_backward``: as passed to ``logz``; without it the
    call runs the time-reversed recursion itself); ``logz_val`` = its output.  A video whose log Z is not finite, or whose
    histories a NaN reached, gets NaN and sets the error word (``error_flag(batch, ws=ws)``).  Bit-identical run to run.
    Its gradient: ``entropy_bwd``."""
    lib = _lib.load()
    head = batch.head(_lib.SHAPE_LOGZ_BOTH if with_backward else 0)
    dev = elp.device
    f64 = torch.float64
    out = torch.empty(batch.b, dtype=f64, device=dev)
    if ws is None:
        ws = workspace(batch.workspace_bytes(), dev)
    _lib.check(lib.smm_entropy_f64(
        *head, *_tables(elp, trans, init, len_scores, endpen), _dev(logz_val, f64, 'logz'), _dev(out, f64, 'entropy'),
        *_ws_args(ws), _stream()))
    return out


def segment_posteriors(batch, elp, trans, init, len_scores, logz_val, spans=None, endpen=None, class_map=None, ws=None,
                       with_backward=False):
    """Exact posterior of every segment boundary, and of each segment of given segmentations (smm_segment_posteriors_f64).
    Must follow ``logz`` for the same batch and tables with the same workspace (``with_backward``: as passed to ``logz``;
    without it the call runs the time-reversed recursion itself); ``logz_val`` = its output.  ``spans``: int64 [n_sets, b,
    t_max+1] or [b, t_max+1] on the device, segmentations in the span encoding ``viterbi`` / ``kbest`` / ``sample`` / ``mbr``
    return (``class_map`` applied, if one is given).  Returns dict(start fp64 [total_frames, c_max]: P(a span of c starts at the
    frame), end: P(a span of c has it as its last frame), boundary fp64 [total_frames]: P(a span starts at the frame), seg_logp
    fp64 shaped like ``spans`` or None: the log posterior of each given span at its start, 0 at the EOS position, -inf at
    continuations, past the video and for a span the lattice does not have).  Padded columns and frames no video covers are 0.
    A video whose log Z is not finite, or whose histories a NaN reached, gets NaN and sets the error word
    (``error_flag(batch, ws=ws)``).  Bit-identical run to run; values, not differentiable."""
    n_sets = 0
    if spans is not None:
        if spans.dtype != torch.int64:
            raise TypeError("spans: expected torch.int64, got %s" % spans.dtype)
        if spans.dim() not in (2, 3) or tuple(spans.shape[-2:]) != (batch.b, batch.t_max + 1):
            raise ValueError("spans: [n_sets, b, t_max+1] or [b, t_max+1] = [.., %d, %d] expected, got %s"
                             % (batch.b, batch.t_max + 1, tuple(spans.shape)))
        n_sets = int(spans.shape[0]) if spans.dim() == 3 else 1
        if n_sets <= 0:
            raise ValueError("spans: at least one set of segmentations is expected")
    if tuple(elp.shape) != (batch.total_frames, batch.c_max):
        raise ValueError("elp: [total_frames, c_max] = [%d, %d] expected, got %s"
                         % (batch.total_frames, batch.c_max, tuple(elp.shape)))
    lib = _lib.load()
    head = batch.head(_lib.SHAPE_LOGZ_BOTH if with_backward else 0)
    dev = elp.device
    f64 = torch.float64
    start = torch.empty((batch.total_frames, batch.c_max), dtype=f64, device=dev)
    end = torch.empty_like(start)
    bnd = torch.empty(batch.total_frames, dtype=f64, device=dev)
    seg = None if spans is None else torch.empty(spans.shape, dtype=f64, device=dev)
    if ws is None:
        ws = workspace(batch.workspace_bytes(), dev)
    _lib.check(lib.smm_segment_posteriors_f64(
        *head, *_tables(elp, trans, init, len_scores, endpen), _dev(class_map, torch.int64, 'class_map'), _dev(logz_val, f64, 'logz'),
        _dev(spans, torch.int64, 'spans'), ctypes.c_int32(n_sets), _dev(start, f64, 'start'), _dev(end, f64, 'end'),
        _dev(bnd, f64, 'boundary'), _dev(seg, f64, 'seg_logp'), *_ws_args(ws), _stream()))
    return dict(start=start, end=end, boundary=bnd, seg_logp=seg, _err=_err_copy(batch, ws))


def _kl_side(t, tag):
    """One side of ``kl`` / ``kl_bwd`` -- (elp, trans, init, len_scores, endpen, logz_val, ws) -- as the C ABI takes it."""
    f64 = torch.float64
    elp, trans, init, len_scores, endpen, logz_val, ws = t
    return [_dev(elp, f64, 'elp_' + tag), _dev(trans, f64, 'trans_' + tag), _dev(init, f64, 'init_' + tag),
            _dev(len_scores, f64, 'len_scores_' + tag), _dev(endpen, f64, 'endpen_' + tag), _dev(logz_val, f64, 'logz_' + tag),
            *_ws_args(ws)]


def kl(batch, p, q, with_backward=False, want_cross_entropy=False):
    """Exact KL divergence KL(p || q) = sum_y p(y | x) log(p(y | x) / q(y | x)) between two segmentation posteriors of the same
    lattice, in nats (smm_kl_f64): fp64 [b]; with ``want_cross_entropy`` the pair (KL, H(p, q) = H(p) + KL).  ``p`` and ``q``
    are each ``(elp, trans, init, len_scores, endpen, logz_val, ws)``: the tables of that side, and the workspace and output of
    its own ``logz`` on ``batch`` (``with_backward``: as passed to p's ``logz``; without it the call runs p's time-reversed
    recursion itself; q needs only its forward histories and its workspace is only read).  +inf, without an error, where q gives
    probability 0 to what p does not.  A video whose log Z_p is not finite, or whose histories a NaN reached on either side,
    gets NaN and sets the error word of p's workspace (``error_flag(batch, ws=p[6])``).  Exactly 0 for bit-identical sides;
    bit-identical run to run.  Its gradient: ``kl_bwd``."""
    lib = _lib.load()
    head = batch.head(_lib.SHAPE_LOGZ_BOTH if with_backward else 0)
    f64 = torch.float64
    dev = p[0].device
    out = torch.empty(batch.b, dtype=f64, device=dev)
    xent = torch.empty(batch.b, dtype=f64, device=dev) if want_cross_entropy else None
    _lib.check(lib.smm_kl_f64(*head, *_kl_side(p, 'p'), *_kl_side(q, 'q'), _dev(out, f64, 'kl'), _dev(xent, f64, 'cross_entropy'),
                              _stream()))
    return (out, xent) if want_cross_entropy else out


def entropy_bwd_scratch_bytes(batch):
    """Bytes of the caller's scratch ``entropy_bwd`` / ``kl_bwd`` need (smm_entropy_bwd_scratch_bytes; host only)."""
    n = _lib.load().smm_entropy_bwd_scratch_bytes(ctypes.byref(batch.shape), batch.lengths.ctypes.data)
    if n == 0:
        raise _lib.SmmError("libsmmdp: invalid batch shape for the entropy gradient")
    return n


def _ebwd_outputs(batch, elp, trans, init, len_scores, want_value, scratch_bytes=entropy_bwd_scratch_bytes):
    """The gradients, ``value`` and the caller's scratch of a gradient unit; ``scratch_bytes``: the unit's scratch query."""
    f64 = torch.float64
    dev = elp.device
    g = _grad_outputs(elp, trans, init, len_scores)
    g['value'] = torch.empty((batch.b, 2), dtype=f64, device=dev) if want_value else None
    scratch = torch.empty(scratch_bytes(batch), dtype=torch.uint8, device=dev)
    return g, scratch


def entropy_bwd(batch, elp, trans, init, len_scores, logz_val, grad_out=None, endpen=None, ws=None, with_backward=False,
                want_value=False):
    """Gradient of sum_i grad_out[i] * H_i, H = ``entropy``, with respect to the tables (smm_entropy_bwd_f64).  Must follow
    ``logz`` for the same batch and tables with the same workspace (``with_backward``: its time-reversed recursion already ran,
    in ``logz`` or in ``entropy``).  -> dict(elp [total_frames, c_max], trans, init, len) fp64 in ``logz_bwd``'s layouts, and
    ``value`` fp64 [b, 2] (H by the two decompositions) with ``want_value``.  A video whose H is not finite gets NaN rows.
    Bit-identical run to run."""
    lib = _lib.load()
    head = batch.head(_lib.SHAPE_LOGZ_BOTH if with_backward else 0)
    f64 = torch.float64
    g, scratch = _ebwd_outputs(batch, elp, trans, init, len_scores, want_value)
    if ws is None:
        ws = workspace(batch.workspace_bytes(), elp.device)
    _lib.check(lib.smm_entropy_bwd_f64(
        *head, *_tables(elp, trans, init, len_scores, endpen), _dev(logz_val, f64, 'logz'), _dev(grad_out, f64, 'grad_out'),
        _dev(g['elp'], f64, 'g_elp'), _dev(g['trans'], f64, 'g_trans'), _dev(g['init'], f64, 'g_init'), _dev(g['len'], f64, 'g_len'),
        _dev(g['value'], f64, 'value'), *_ws_args(scratch), *_ws_args(ws), _stream()))
    return g


def kl_bwd(batch, p, q, grad_out=None, with_backward=False, cross_entropy=False, want_value=False):
    """Gradient of sum_i grad_out[i] * V_i with respect to p's tables (smm_kl_bwd_f64): V = KL(p || q), or H(p, q) with
    ``cross_entropy``.  ``p`` and ``q`` as for ``kl``; ``with_backward``: both sides' time-reversed recursions already ran
    (else the call runs both, and q's workspace is written).  -> dict as ``entropy_bwd``.  q's gradient is mu_q - mu_p: two
    ``logz_bwd`` calls.  Exactly 0 for bit-identical sides (KL); bit-identical run to run."""
    lib = _lib.load()
    head = batch.head(_lib.SHAPE_LOGZ_BOTH if with_backward else 0)
    f64 = torch.float64
    g, scratch = _ebwd_outputs(batch, p[0], p[1], p[2], p[3], want_value)
    mode = _lib.KL_BWD_CROSS_ENTROPY if cross_entropy else _lib.KL_BWD_KL
    _lib.check(lib.smm_kl_bwd_f64(
        *head, *_kl_side(p, 'p'), *_kl_side(q, 'q'), ctypes.c_int32(mode), _dev(grad_out, f64, 'grad_out'),
        _dev(g['elp'], f64, 'g_elp'), _dev(g['trans'], f64, 'g_trans'), _dev(g['init'], f64, 'g_init'),
        _dev(g['len'], f64, 'g_len'), _dev(g['value'], f64, 'value'), *_ws_args(scratch), _stream()))
    return g


def _check_rewards(batch, reward, seg_reward):
    if reward is None and seg_reward is None:
        raise ValueError("expected_reward: at least one of reward and seg_reward is needed")
    if reward is not None and tuple(reward.shape) != (batch.total_frames, batch.c_max):
        raise ValueError("reward: [total_frames, c_max] = [%d, %d] expected, got %s"
                         % (batch.total_frames, batch.c_max, tuple(reward.shape)))
    if seg_reward is not None and tuple(seg_reward.shape) != (batch.n_groups, batch.c_max):
        raise ValueError("seg_reward: [n_groups, c_max] = [%d, %d] expected, got %s"
                         % (batch.n_groups, batch.c_max, tuple(seg_reward.shape)))


def expected_reward(batch, elp, trans, init, len_scores, logz_val, reward=None, seg_reward=None, endpen=None, ws=None,
                    with_backward=False, want_parts=False):
    """Posterior expectation V = E_p[R(y)] of a reward that is additive over frames and segments (smm_expected_reward_f64):
    R(y) = sum over the spans (s, k, c) of y of seg_reward[c] + sum of reward[t][c] over the span's frames.  fp64 [b]; with
    ``want_parts`` the pair (V, parts fp64 [b, 2]: the frame part and the segment part).  ``reward``: fp64 [total_frames, c_max]
    on local states, ``seg_reward``: fp64 [n_groups, c_max]; either may be None.  Must follow ``logz`` for the same batch and
    tables with the same workspace (``with_backward``: as passed to ``logz``; without it the call runs the time-reversed
    recursion itself); ``logz_val`` = its output.  Padded columns and frames no video covers are ignored.  A video whose log Z
    is not finite, or with a non-finite reward in a covered entry, gets NaN and sets the error word
    (``error_flag(batch, ws=ws)``).  Bit-identical run to run.  Its gradient: ``expected_reward_bwd``."""
    _check_rewards(batch, reward, seg_reward)
    lib = _lib.load()
    head = batch.head(_lib.SHAPE_LOGZ_BOTH if with_backward else 0)
    dev = elp.device
    f64 = torch.float64
    out = torch.empty(batch.b, dtype=f64, device=dev)
    parts = torch.empty((batch.b, 2), dtype=f64, device=dev) if want_parts else None
    if ws is None:
        ws = workspace(batch.workspace_bytes(), dev)
    _lib.check(lib.smm_expected_reward_f64(
        *head, *_tables(elp, trans, init, len_scores, endpen), _dev(logz_val, f64, 'logz'), _dev(reward, f64, 'reward'),
        _dev(seg_reward, f64, 'seg_reward'), _dev(out, f64, 'value'), _dev(parts, f64, 'parts'), *_ws_args(ws), _stream()))
    return (out, parts) if want_parts else out


def expected_reward_bwd_scratch_bytes(batch):
    """Bytes of the caller's scratch ``expected_reward_bwd`` needs (smm_expected_reward_bwd_scratch_bytes; host only)."""
    n = _lib.load().smm_expected_reward_bwd_scratch_bytes(ctypes.byref(batch.shape), batch.lengths.ctypes.data)
    if n == 0:
        raise _lib.SmmError("libsmmdp: invalid batch shape for the expected-reward gradient")
    return n


def expected_reward_bwd(batch, elp, trans, init, len_scores, logz_val, reward=None, seg_reward=None, grad_out=None, endpen=None,
                        ws=None, with_backward=False, want_value=False):
    """Gradient of sum_i grad_out[i] * V_i, V = ``expected_reward``, with respect to the tables (smm_expected_reward_bwd_f64): a
    Hessian-vector product of log Z.  Call order as ``expected_reward``.  -> dict(elp [total_frames, c_max], trans, init, len)
    fp64 in ``logz_bwd``'s layouts, and ``value`` fp64 [b, 2] (V by the two decompositions) with ``want_value``.  The rewards
    get no gradient.  A video whose V is not finite gets NaN rows.  Bit-identical run to run."""
    _check_rewards(batch, reward, seg_reward)
    lib = _lib.load()
    head = batch.head(_lib.SHAPE_LOGZ_BOTH if with_backward else 0)
    f64 = torch.float64
    g, scratch = _ebwd_outputs(batch, elp, trans, init, len_scores, want_value, expected_reward_bwd_scratch_bytes)
    if ws is None:
        ws = workspace(batch.workspace_bytes(), elp.device)
    _lib.check(lib.smm_expected_reward_bwd_f64(
        *head, *_tables(elp, trans, init, len_scores, endpen), _dev(logz_val, f64, 'logz'), _dev(reward, f64, 'reward'),
        _dev(seg_reward, f64, 'seg_reward'), _dev(grad_out, f64, 'grad_out'), _dev(g['elp'], f64, 'g_elp'),
        _dev(g['trans'], f64, 'g_trans'), _dev(g['init'], f64, 'g_init'), _dev(g['len'], f64, 'g_len'),
        _dev(g['value'], f64, 'value'), *_ws_args(scratch), *_ws_args(ws), _stream()))
    return g


MAX_KBEST = 16


def kbest_workspace_bytes(batch, k):
    """Bytes of workspace smm_kbest_f64 needs for this batch and k (more than ``batch.workspace_bytes()``)."""
    n = _lib.load().smm_kbest_workspace_bytes(ctypes.byref(batch.shape), batch.lengths.ctypes.data, ctypes.c_int32(int(k)))
    if n == 0:
        raise _lib.SmmError("libsmmdp: invalid batch shape or k (1 <= k <= %d)" % MAX_KBEST)
    return n


def kbest(batch, elp, trans, init, len_scores, k, endpen=None, class_map=None, ws=None, want_spans=True, want_labels=True):
    """The k highest-scoring segmentations of every video (smm_kbest_f64).  Returns dict(spans int64 [k, b, t_max+1] (span
    encoding, class map applied) or None, labels int64 [k, total_frames] (global ids, -1 on frames no video covers) or None,
    score fp64 [k, b]: each result's score re-evaluated in fp64 along its path, non-increasing over the ranks, n_segs int32
    [k, b]).  Ranks past a video's last segmentation: score -inf, n_segs 0, spans -1, labels -1.  ``ws``: a uint8 workspace
    of at least ``kbest_workspace_bytes(batch, k)`` (default: a private one for this call)."""
    lib = _lib.load()
    k = int(k)
    if not 1 <= k <= MAX_KBEST:
        raise ValueError("k must be in 1..%d, got %d" % (MAX_KBEST, k))
    dev = elp.device
    f64 = torch.float64
    spans, labels, score, n_segs = _device_outputs(batch, dev, want_spans, want_labels, (k,))
    if ws is None:
        ws = torch.empty(kbest_workspace_bytes(batch, k), dtype=torch.uint8, device=dev)
    _lib.check(lib.smm_kbest_f64(
        *batch.head(), *_tables(elp, trans, init, len_scores, endpen), _dev(class_map, torch.int64, 'class_map'),
        ctypes.c_int32(k), _dev(spans, torch.int64, 'spans'), _dev(labels, torch.int64, 'labels'), _dev(score, f64, 'score'),
        _dev(n_segs, torch.int32, 'n_segs'), *_ws_args(ws), _stream()))
    return dict(spans=spans, labels=labels, score=score, n_segs=n_segs, _err=_err_copy(batch, ws))


def mbr_workspace_bytes(batch):
    """Bytes of workspace smm_mbr_f64 needs for this batch (host only)."""
    n = _lib.load().smm_mbr_workspace_bytes(ctypes.byref(batch.shape), batch.lengths.ctypes.data)
    if n == 0:
        raise _lib.SmmError("libsmmdp: invalid batch shape for the MBR decode")
    return n


def mbr(batch, gain, trans, init, endpen=None, class_map=None, ws=None, want_spans=True, want_labels=True):
    """Minimum-Bayes-risk decode under frame loss (smm_mbr_f64): per video the feasible segmentation that maximises
    sum_t gain[t][y_t] -- with gain = the frame posteriors (``logz_bwd``'s ``elp``), the expected number of correct frames.  It is
    ``viterbi`` on the substituted inputs elp = gain, zero length scores, and trans / init / endpen made binary (-1e9 where the
    table is <= -5e8, else 0).  gain fp64 [total_frames, c_max].  Returns dict(spans int64 [b, t_max+1] (span encoding, class
    map applied) or None, labels int64 [total_frames] (global ids, -1 on frames no video covers) or None, best fp64 [b] (the DP
    value), gain_sum fp64 [b] (sum_t gain[t][y_t], in frame order), n_segs int32 [b]).  ``ws``: a uint8 workspace of at least
    ``mbr_workspace_bytes(batch)`` (default: a private one for this call)."""
    lib = _lib.load()
    dev = gain.device
    f64 = torch.float64
    spans, labels, best, n_segs = _device_outputs(batch, dev, want_spans, want_labels)
    gain_sum = torch.empty(batch.b, dtype=f64, device=dev)
    ws = _own_workspace(ws, mbr_workspace_bytes(batch), dev)
    _lib.check(lib.smm_mbr_f64(
        *batch.head(), _dev(gain, f64, 'gain'), _dev(trans, f64, 'trans'), _dev(init, f64, 'init'),
        _dev(endpen, f64, 'endpen'), _dev(class_map, torch.int64, 'class_map'), _dev(spans, torch.int64, 'spans'),
        _dev(labels, torch.int64, 'labels'), _dev(best, f64, 'best'), _dev(gain_sum, f64, 'gain_sum'),
        _dev(n_segs, torch.int32, 'n_segs'), *_ws_args(ws), _stream()))
    return dict(spans=spans, labels=labels, best=best, gain_sum=gain_sum, n_segs=n_segs, _err=_err_copy(batch, ws))


MAX_TRANSCRIPT = _lib.MAX_TRANSCRIPT


def _transcript_arrays(batch, transcripts):
    """Per-video sequences of local state ids -> (ids int32 [sum M], offsets int64 [b + 1]) on the host."""
    if len(transcripts) != batch.b:
        raise ValueError("align: %d transcripts for %d videos" % (len(transcripts), batch.b))
    seqs = [np.asarray(t.detach().cpu() if torch.is_tensor(t) else t, dtype=np.int64).reshape(-1) for t in transcripts]
    for i, q in enumerate(seqs):
        if q.size == 0:
            raise ValueError("align: the transcript of video %d is empty" % i)
        if q.size > MAX_TRANSCRIPT:
            raise ValueError("align: the transcript of video %d has %d entries (at most %d)" % (i, q.size, MAX_TRANSCRIPT))
    off = np.zeros(batch.b + 1, np.int64)
    np.cumsum([q.size for q in seqs], out=off[1:])
    return np.ascontiguousarray(np.concatenate(seqs).astype(np.int32)), off


def _transcript_offsets(batch, transcript_offset, what):
    off = np.ascontiguousarray(np.asarray(transcript_offset, dtype=np.int64).reshape(-1))
    if off.shape[0] != batch.b + 1:
        raise ValueError("%s: b + 1 transcript offsets expected" % what)
    return off


def _transcript_workspace_bytes(batch, transcript_offset, what, of):
    """The ``*_workspace_bytes`` of the transcript entry points below: libsmmdp's ``smm_<what>`` on the checked offsets; 0 is its refusal."""
    off = _transcript_offsets(batch, transcript_offset, what)
    n = getattr(_lib.load(), 'smm_' + what)(ctypes.byref(batch.shape), ctypes.c_void_p(batch.lengths.ctypes.data),
                                            ctypes.c_void_p(off.ctypes.data))
    if n == 0:
        raise _lib.SmmError("libsmmdp: invalid batch shape or transcript offsets for the %s (add_eos=True only, 1..%d entries "
                            "per video)" % (of, MAX_TRANSCRIPT))
    return n


def align_workspace_bytes(batch, transcript_offset):
    """Bytes of workspace smm_align_f64 needs for this batch and these transcript offsets (int64 [b + 1]; host only)."""
    return _transcript_workspace_bytes(batch, transcript_offset, 'align_workspace_bytes', 'alignment')


def align_opt_workspace_bytes(batch, transcript_offset):
    """Bytes of workspace smm_align_opt_f64 needs for this batch and these transcript offsets (int64 [b + 1]; host only)."""
    return _transcript_workspace_bytes(batch, transcript_offset, 'align_opt_workspace_bytes', 'alignment')


def _optional_flags(off, optional):
    """One boolean sequence per video, as long as its transcript -> uint8 [sum M] on the host."""
    b = off.shape[0] - 1
    if len(optional) != b:
        raise ValueError("align: %d sequences of optional flags for %d videos" % (len(optional), b))
    flags = [np.asarray(f.detach().cpu() if torch.is_tensor(f) else f).reshape(-1) != 0 for f in optional]
    for i, f in enumerate(flags):
        if f.size != off[i + 1] - off[i]:
            raise ValueError("align: %d optional flags for the %d transcript entries of video %d" % (f.size, off[i + 1] - off[i], i))
    return np.ascontiguousarray(np.concatenate(flags).astype(np.uint8))


class TranscriptGraph:
    """What smm_align_graph_f64 aligns a video to: a DAG whose nodes carry a class id, numbered in topological order.
    ``ids`` int64 [M]; ``pred`` bool [M, M], strictly lower triangular: pred[m, j] -- node j may directly precede node m;
    ``start`` / ``end`` bool [M]: the node may be the first / the last segment.  The allowed class sequences are those of the
    start -> end paths.  ``pred`` may also be given as a list of predecessor lists.  ``end_candidate`` int64 [M]: for a graph
    from ``from_candidates`` the lowest index of a candidate that ends at the node, else -1.  ValueError for no node or more
    than ``MAX_TRANSCRIPT`` of them, an edge j >= m, no start node or no end node."""

    def __init__(self, ids, pred, start, end, end_candidate=None):
        ids = np.asarray(ids.detach().cpu() if torch.is_tensor(ids) else ids, dtype=np.int64).reshape(-1)
        M = ids.size
        if M < 1 or M > MAX_TRANSCRIPT:
            raise ValueError("TranscriptGraph: %d nodes (1 to %d)" % (M, MAX_TRANSCRIPT))
        if isinstance(pred, (list, tuple)):                 # predecessor lists (an array or a tensor: the matrix)
            if len(pred) != M:
                raise ValueError("TranscriptGraph: %d predecessor lists for %d nodes" % (len(pred), M))
            p = np.zeros((M, M), bool)
            for m, js in enumerate(pred):
                for j in js:
                    if not 0 <= int(j) < m:
                        raise ValueError("TranscriptGraph: edge %d -> %d (the numbering must be topological: j < m)" % (int(j), m))
                    p[m, int(j)] = True
        else:
            p = np.asarray(pred.detach().cpu() if torch.is_tensor(pred) else pred) != 0
            if p.shape != (M, M):
                raise ValueError("TranscriptGraph: pred must be [M, M] or M predecessor lists")
            if np.triu(p).any():
                m, j = (int(x) for x in np.argwhere(np.triu(p))[0])
                raise ValueError("TranscriptGraph: edge %d -> %d (the numbering must be topological: j < m)" % (j, m))
        start = np.asarray(start.detach().cpu() if torch.is_tensor(start) else start).reshape(-1) != 0
        end = np.asarray(end.detach().cpu() if torch.is_tensor(end) else end).reshape(-1) != 0
        if start.size != M or end.size != M:
            raise ValueError("TranscriptGraph: start and end take one flag per node")
        if not start.any():
            raise ValueError("TranscriptGraph: no start node")
        if not end.any():
            raise ValueError("TranscriptGraph: no end node")
        self.ids, self.pred, self.start, self.end = ids, p, start, end
        self._trie = False                                  # from_candidates: no two paths spell the same labels
        self.end_candidate = (np.full(M, -1, np.int64) if end_candidate is None
                              else np.asarray(end_candidate, dtype=np.int64).reshape(-1))
        if self.end_candidate.size != M:
            raise ValueError("TranscriptGraph: end_candidate takes one index per node")

    def __len__(self):
        return int(self.ids.size)

    @classmethod
    def chain(cls, ids):
        """A plain transcript: pred(m) = {m - 1}, start = {0}, end = {M - 1} (smm_align_f64's results)."""
        ids = np.asarray(ids.detach().cpu() if torch.is_tensor(ids) else ids, dtype=np.int64).reshape(-1)
        M = ids.size
        return cls(ids, np.eye(M, k=-1, dtype=bool), np.arange(M) == 0, np.arange(M) == M - 1)

    @classmethod
    def from_optional(cls, ids, optional):
        """A transcript with optional entries: pred(m) = m-1, m-2, ... down to and including the nearest mandatory entry;
        start(m): every entry before m is optional; end(m): every entry after it is (smm_align_opt_f64's results)."""
        ids = np.asarray(ids.detach().cpu() if torch.is_tensor(ids) else ids, dtype=np.int64).reshape(-1)
        opt = np.asarray(optional.detach().cpu() if torch.is_tensor(optional) else optional).reshape(-1) != 0
        M = ids.size
        if opt.size != M:
            raise ValueError("TranscriptGraph.from_optional: %d flags for %d entries" % (opt.size, M))
        pred = np.zeros((M, M), bool)
        head = 0
        for m in range(M):
            pred[m, head:m] = True
            if not opt[m]:
                head = m
        start = np.array([opt[:m].all() for m in range(M)], bool)
        end = np.array([opt[m + 1:].all() for m in range(M)], bool)
        return cls(ids, pred, start, end)

    @classmethod
    def from_candidates(cls, candidates):
        """"One of these transcripts": the prefix trie of the candidates (sequences of class ids, none empty).  Nodes are
        created in insertion order, which is topological; candidates with a common prefix share its nodes, identical
        candidates collapse.  ``end_candidate[m]``: the lowest index of a candidate that ends at node m."""
        ids, parent, endc, child = [], [], [], {}
        for ci, cand in enumerate(candidates):
            seq = np.asarray(cand.detach().cpu() if torch.is_tensor(cand) else cand, dtype=np.int64).reshape(-1)
            if seq.size == 0:
                raise ValueError("TranscriptGraph.from_candidates: candidate %d is empty" % ci)
            at = -1
            for c in seq.tolist():
                nxt = child.get((at, c))
                if nxt is None:
                    nxt = len(ids)
                    child[(at, c)] = nxt
                    ids.append(c)
                    parent.append(at)
                    endc.append(-1)
                at = nxt
            if endc[at] < 0:
                endc[at] = ci
        M = len(ids)
        if M < 1 or M > MAX_TRANSCRIPT:
            raise ValueError("TranscriptGraph.from_candidates: the trie has %d nodes (1 to %d)" % (M, MAX_TRANSCRIPT))
        par = np.array(parent, np.int64)
        pred = np.zeros((M, M), bool)
        inner = np.flatnonzero(par >= 0)
        pred[inner, par[inner]] = True
        endc = np.array(endc, np.int64)
        g = cls(ids, pred, par < 0, endc >= 0, end_candidate=endc)
        g._trie = True
        return g

    @staticmethod
    def trie_nodes(candidates):
        """The number of nodes ``from_candidates`` would create."""
        seen = set()
        for cand in candidates:
            seq = np.asarray(cand.detach().cpu() if torch.is_tensor(cand) else cand, dtype=np.int64).reshape(-1).tolist()
            seen.update(tuple(seq[:n]) for n in range(1, len(seq) + 1))
        return len(seen)

    def with_ids(self, ids):
        """The same structure over other class ids (global -> local)."""
        return TranscriptGraph(ids, self.pred, self.start, self.end, self.end_candidate)

    def packed_masks(self):
        """-> uint32 [M, 8]: bit j of node m's 256-bit mask (word j // 32, bit j % 32) is pred[m, j]."""
        M = len(self)
        bits = np.zeros((M, MAX_TRANSCRIPT), np.uint8)
        bits[:, :M] = self.pred
        return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder='little')).view('<u4').astype(np.uint32)

    def node_flags(self):
        """-> uint8 [M]: bit 0 = start, bit 1 = end."""
        return (self.start.astype(np.uint8) | (self.end.astype(np.uint8) << 1)).astype(np.uint8)

    def is_ambiguous(self):
        """Host only, exact: True when two different start -> end paths spell the same class sequence --
        ``align_graph_logz`` then counts the segmentations with that class sequence once per path.  Over the pairs (i, j) of
        equal class, in topological order, `same[i, j]` says that a path from a start node ending in i and one ending in j
        spell the same labels, `diff[i, j]` that two such paths differ (always when i != j); each row is one boolean
        pred[i] @ R @ pred[j].T, O(M^3) bit operations at worst.  Ambiguous iff diff holds for a pair of end nodes (i = j
        included).  A graph from ``from_candidates`` is unambiguous by construction."""
        if self._trie:
            return False
        M = len(self)
        pred = self.pred.astype(np.int64)
        eq = self.ids[:, None] == self.ids[None, :]
        same = np.zeros((M, M), np.int64)
        diff = np.zeros((M, M), np.int64)
        for t in range(M):
            lower = pred[:t + 1]
            row = eq[t, :t + 1] & ((self.start[t] & self.start[:t + 1]) | (lower @ (pred[t] @ same) > 0))
            same[t, :t + 1] = row
            same[:t + 1, t] = row
            drow = row.copy()
            drow[t] = row[t] and bool(pred[t] @ diff @ pred[t] > 0)
            diff[t, :t + 1] = drow
            diff[:t + 1, t] = drow
        ends = np.flatnonzero(self.end)
        return bool(diff[np.ix_(ends, ends)].any())

    def candidate_of(self, used):
        """The candidate an alignment chose: ``end_candidate`` of the last used node (``used``: the call's per-node flags of
        this video); -1 without an alignment."""
        u = np.flatnonzero(np.asarray(used.detach().cpu() if torch.is_tensor(used) else used).reshape(-1) != 0)
        return int(self.end_candidate[u[-1]]) if u.size else -1


def align_graph_workspace_bytes(batch, node_offset):
    """Bytes of workspace smm_align_graph_f64 needs for this batch and these node offsets (int64 [b + 1]; host only)."""
    return _transcript_workspace_bytes(batch, node_offset, 'align_graph_workspace_bytes', 'graph alignment')


ALIGN_LOGZ_TILE = _lib.ALIGN_LOGZ_TILE


def align_logz_workspace_bytes(batch, transcript_offset):
    """Bytes of workspace smm_align_logz_f64 / smm_align_logz_bwd_f64 need for this batch and these transcript offsets (int64
    [b + 1]; host only)."""
    return _transcript_workspace_bytes(batch, transcript_offset, 'align_logz_workspace_bytes', 'transcript likelihood')


def align_opt_logz_workspace_bytes(batch, transcript_offset):
    """Bytes of workspace smm_align_opt_logz_f64 / smm_align_opt_logz_bwd_f64 need for this batch and these transcript offsets
    (int64 [b + 1]; host only)."""
    return _transcript_workspace_bytes(batch, transcript_offset, 'align_opt_logz_workspace_bytes', 'transcript likelihood')


def align_graph_logz_workspace_bytes(batch, node_offset):
    """Bytes of workspace smm_align_graph_logz_f64 / smm_align_graph_logz_bwd_f64 need for this batch and these node offsets
    (int64 [b + 1]; host only)."""
    return _transcript_workspace_bytes(batch, node_offset, 'align_graph_logz_workspace_bytes', 'transcript-graph likelihood')


# (kind of supervision, what is computed) -> (the forward launch's symbol in the library, its workspace size, its value's name)
_TRANSCRIPT_LAUNCH = {
    ('chain', 'alignment'): ('smm_align_f64', align_workspace_bytes, 'best'),
    ('optional', 'alignment'): ('smm_align_opt_f64', align_opt_workspace_bytes, 'best'),
    ('graph', 'alignment'): ('smm_align_graph_f64', align_graph_workspace_bytes, 'best'),
    ('chain', 'likelihood'): ('smm_align_logz_f64', align_logz_workspace_bytes, 'logz_a'),
    ('optional', 'likelihood'): ('smm_align_opt_logz_f64', align_opt_logz_workspace_bytes, 'logz_o'),
    ('graph', 'likelihood'): ('smm_align_graph_logz_f64', align_graph_logz_workspace_bytes, 'logz_g'),
}


class _Supervision:
    """What one launch of the transcript family is supervised by, staged.  ``kind``: 'chain' (a transcript per video),
    'optional' (a transcript and one flag per entry) or 'graph' (a ``TranscriptGraph`` per video); ``off``: int64 [b + 1] on
    the host, the videos' entry / node offsets; ``dev``: the device tensors -- (ids,), (ids, flags) or (classes, masks, flags),
    what a launcher returns as ``_staged``; ``need``: the bytes of workspace the launch takes."""
    FIELDS = {'chain': (('transcript', torch.int32),),
              'optional': (('transcript', torch.int32), ('optional', torch.uint8)),
              'graph': (('node_class', torch.int32), ('pred_mask', torch.int32), ('node_flags', torch.uint8))}

    def __init__(self, kind, off, dev, need):
        self.kind, self.off, self.dev, self.need = kind, off, dev, need
        self.n = int(off[-1])

    def args(self):
        """The library call's pointer arguments: the device arrays, then the offsets."""
        return tuple(_dev(t, dtype, name) for t, (name, dtype) in zip(self.dev, self.FIELDS[self.kind])) + (
            ctypes.c_void_p(self.off.ctypes.data),)

    def per_video(self, t, dim=0):
        """One view per video of a device tensor that has one column per entry / node."""
        return list(torch.split(t, np.diff(self.off).tolist(), dim=dim))


def _supervision(kind, computed, what, batch, dev, given, optional=None, staged=None):
    """The supervision of the launch ``what``: ``given`` -- per-video sequences of local ids (with ``optional``: one boolean
    sequence per video) or one ``TranscriptGraph`` per video -- checked on the host, sized, and then taken from ``staged``
    (an earlier call's ``_staged``) or copied to ``dev``.  Every check on the host arrays, the workspace size among them,
    comes before a device is touched.  A 'chain' likelihood also takes the (ids on the device, offsets on the host) pair an
    earlier call returned as ``transcript``."""
    pair = (computed == 'likelihood' and kind == 'chain' and isinstance(given, tuple) and len(given) == 2
            and torch.is_tensor(given[0]))
    if kind == 'graph':
        if len(given) != batch.b:
            raise ValueError("%s: %d graphs for %d videos" % (what, len(given), batch.b))
        if batch.no_eos:
            raise ValueError("%s: add_eos=False is not supported" % what)
        off = np.zeros(batch.b + 1, np.int64)
        np.cumsum([len(g) for g in given], out=off[1:])
    elif pair:
        staged, off = (given[0],), given[1]
    else:
        if kind == 'optional' and optional is None:
            raise ValueError("%s: one sequence of flags per video expected (no flags: %s)"
                             % (what, 'align' if computed == 'alignment' else 'align_logz'))
        ids, off = _transcript_arrays(batch, given)
        host = (ids, _optional_flags(off, optional)) if kind == 'optional' else (ids,)
    need = _TRANSCRIPT_LAUNCH[kind, computed][1](batch, off)
    if staged is None:
        if kind == 'graph':
            host = (np.concatenate([g.ids for g in given]).astype(np.int32),
                    np.concatenate([g.packed_masks() for g in given]).reshape(-1).view(np.int32),   # (the bits of the uint32 words)
                    np.concatenate([g.node_flags() for g in given]))
        staged = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in host)
    elif kind == 'graph' and staged[0].shape[0] != off[-1]:
        raise ValueError("%s: staged classes, masks and flags of other graphs" % what)
    elif kind == 'optional' and (staged[0].shape[0] != off[-1] or staged[1].shape[0] != off[-1]):
        raise ValueError("%s: staged ids and flags of another transcript" % what)
    return _Supervision(kind, off, tuple(staged), need)


def _tables(elp, trans, init, len_scores, endpen):
    f64 = torch.float64
    return (_dev(elp, f64, 'elp'), _dev(trans, f64, 'trans'), _dev(init, f64, 'init'), _dev(len_scores, f64, 'len_scores'),
            _dev(endpen, f64, 'endpen'))


def _align_launch(kind, what, batch, elp, trans, init, len_scores, given, optional, endpen, class_map, ws, want_spans, want_labels,
                  want_used, staged):
    """smm_align_f64, smm_align_opt_f64 or smm_align_graph_f64 by ``kind``; the plain transcript's call has no ``used``."""
    lib = _lib.load()
    dev = elp.device
    sup = _supervision(kind, 'alignment', what, batch, dev, given, optional, staged)
    spans, labels, best, n_segs = _device_outputs(batch, dev, want_spans, want_labels)
    ws = _own_workspace(ws, sup.need, dev)
    used = torch.empty(sup.n, dtype=torch.int32, device=dev) if want_used else None
    _lib.check(getattr(lib, _TRANSCRIPT_LAUNCH[kind, 'alignment'][0])(
        *batch.head(), *_tables(elp, trans, init, len_scores, endpen), _dev(class_map, torch.int64, 'class_map'), *sup.args(),
        _dev(spans, torch.int64, 'spans'), _dev(labels, torch.int64, 'labels'), _dev(best, torch.float64, 'best'),
        _dev(n_segs, torch.int32, 'n_segs'), *(() if kind == 'chain' else (_dev(used, torch.int32, 'used'),)), *_ws_args(ws),
        _stream()))
    out = dict(spans=spans, labels=labels, best=best, n_segs=n_segs, _err=_err_copy(batch, ws))
    if kind == 'chain':
        return dict(out, _keep=sup.dev + (ws,))
    return dict(out, used=None if used is None else sup.per_video(used), _staged=sup.dev, _keep=(ws,))


def align(batch, elp, trans, init, len_scores, transcripts, endpen=None, class_map=None, ws=None, want_spans=True,
          want_labels=True):
    """Forced alignment (smm_align_f64): per video the best segmentation whose class sequence is its transcript -- a sequence
    of LOCAL state ids, one per segment, consecutive repeats allowed -- so only the boundaries are free.  Bit for bit
    ``viterbi`` on the lattice whose states are the transcript positions; with the transcript of the Viterbi path, the Viterbi
    decode.  Returns dict(spans int64 [b, t_max+1] (span encoding, class map applied) or None, labels int64 [total_frames]
    (global ids, -1 on frames no video covers) or None, best fp64 [b], n_segs int32 [b] (the transcript's length)).  A video
    whose transcript cannot be laid over its frames (more entries than frames, too few for the span limit, an id that is no
    state of the video) gets best -inf, n_segs 0, spans and labels -1.  ``ws``: a uint8 workspace of at least
    ``align_workspace_bytes`` (default: a private one for this call).  Optional entries: ``align_optional``."""
    return _align_launch('chain', 'align', batch, elp, trans, init, len_scores, transcripts, None, endpen, class_map, ws, want_spans,
                         want_labels, False, None)


def align_optional(batch, elp, trans, init, len_scores, transcripts, optional, endpen=None, class_map=None, ws=None,
                   want_spans=True, want_labels=True, want_used=False, staged=None):
    """``align`` with optional transcript entries (smm_align_opt_f64, also when no flag is set): ``optional`` is one boolean
    sequence per video, as long as its transcript; the flagged entries may be left out, and the result is the best over every
    subset of them.  ValueError when their count or a length differs from the transcripts'.  Returns ``align``'s dict, n_segs
    counting the entries that got a segment, plus ``used``: None, or with ``want_used`` a list of per-video int32 views of one
    device tensor, 1 for an entry that has a segment, else 0.  More MANDATORY entries than frames is what leaves no alignment.
    ``ws``: at least ``align_opt_workspace_bytes``.  ``staged``: the ``_staged`` entry of an earlier call's result for the same
    transcripts and flags -- the ids and flags on the device: the call then copies nothing from the host itself and can be
    captured into a graph (keep that earlier result alive as long as the graph)."""
    return _align_launch('optional', 'align_optional', batch, elp, trans, init, len_scores, transcripts, optional, endpen, class_map,
                         ws, want_spans, want_labels, want_used, staged)


def align_graph(batch, elp, trans, init, len_scores, graphs, endpen=None, class_map=None, ws=None, want_spans=True,
                want_labels=True, want_used=False, staged=None):
    """Forced alignment to a transcript graph (smm_align_graph_f64): per video the best segmentation whose class sequence is
    a start -> end path of its ``TranscriptGraph`` (LOCAL state ids) -- a candidate set as its trie, alternatives, a free
    order, long skips; a chain gives ``align``'s results and ``TranscriptGraph.from_optional`` gives ``align_optional``'s, bit
    for bit.  Returns ``align_optional``'s dict: n_segs counts the nodes of the path, ``used`` (with ``want_used``) is a list
    of per-video int32 views of one device tensor, 1 for the nodes of the path.  A video no path of whose graph can be laid
    over its frames gets best -inf, n_segs 0, spans and labels -1.  ValueError when the number of graphs differs from the
    videos'.  ``ws``: at least ``align_graph_workspace_bytes``.  ``staged``: the ``_staged`` entry of an earlier call's result
    for the same graphs -- classes, masks and flags on the device -- as in ``align_optional``."""
    return _align_launch('graph', 'align_graph', batch, elp, trans, init, len_scores, graphs, None, endpen, class_map, ws,
                         want_spans, want_labels, want_used, staged)


def _logz_launch(kind, what, batch, elp, trans, init, len_scores, given, optional, endpen, ws, staged):
    """smm_align_logz_f64, smm_align_opt_logz_f64 or smm_align_graph_logz_f64 by ``kind`` -> (dict(logz, ws, _staged, _err),
    the supervision)."""
    lib = _lib.load()
    symbol, _, name = _TRANSCRIPT_LAUNCH[kind, 'likelihood']
    sup = _supervision(kind, 'likelihood', what, batch, elp.device, given, optional, staged)
    args = _tables(elp, trans, init, len_scores, endpen) + sup.args()
    ws = _own_workspace(ws, sup.need, elp.device)
    out = torch.empty(batch.b, dtype=torch.float64, device=elp.device)
    _lib.check(getattr(lib, symbol)(*batch.head(), *args, _dev(out, torch.float64, name), *_ws_args(ws), _stream()))
    return dict(logz=out, ws=ws, _staged=sup.dev, _err=_err_copy(batch, ws)), sup


def align_logz(batch, elp, trans, init, len_scores, transcripts, endpen=None, ws=None):
    """Transcript likelihood (smm_align_logz_f64): per video log Z_a, the log of the sum over every segmentation whose class
    sequence is its transcript -- LOCAL state ids, one per segment, consecutive repeats allowed.  -> fp64 [b]: -inf for a
    video without such a segmentation, NaN (and the error word) when a NaN reached the DP.  ``ws``: a uint8 workspace of at
    least ``align_logz_workspace_bytes`` -- keep it for ``align_logz_bwd`` (default: a private one, then use ``align_logz_ex``)."""
    return align_logz_ex(batch, elp, trans, init, len_scores, transcripts, endpen=endpen, ws=ws)['logz']


def align_logz_ex(batch, elp, trans, init, len_scores, transcripts, endpen=None, ws=None):
    """``align_logz`` with what a backward call needs: dict(logz, ws, transcript (ids on the device, offsets on the host),
    _err (the launch's error words, copied))."""
    out, sup = _logz_launch('chain', 'align_logz', batch, elp, trans, init, len_scores, transcripts, None, endpen, ws, None)
    return dict(logz=out['logz'], ws=out['ws'], transcript=(sup.dev[0], sup.off), _err=out['_err'])


def align_opt_logz(batch, elp, trans, init, len_scores, transcripts, optional, endpen=None, ws=None, staged=None):
    """Transcript likelihood with optional entries (smm_align_opt_logz_f64, also when no flag is set): per video log Z_o, the
    log of the sum over every ALIGNMENT -- which of the flagged entries get a segment, and where the boundaries lie.  Where no
    two subsets of the flagged entries give the same class sequence (``transcript_is_ambiguous``) that is the likelihood of
    the set of class sequences; else a segmentation counts once per subset that yields its class sequence.  ``transcripts``
    and ``optional`` as in ``align_optional``.  -> dict(logz fp64 [b] (-inf: no alignment; NaN and the error word: a NaN
    reached the DP), ws (keep it for ``align_opt_logz_bwd``), _staged (ids and flags on the device), _err).  ``ws``: at least
    ``align_opt_logz_workspace_bytes``.  ``staged``: the ``_staged`` entry of an earlier call for the same transcripts and
    flags: the call then copies nothing from the host itself and can be captured into a graph."""
    return _logz_launch('optional', 'align_opt_logz', batch, elp, trans, init, len_scores, transcripts, optional, endpen, ws, staged)[0]


def align_graph_logz(batch, elp, trans, init, len_scores, graphs, endpen=None, ws=None, staged=None):
    """Transcript-graph likelihood (smm_align_graph_logz_f64): per video log Z_g, the log of the sum over every ALIGNMENT of
    the video to its ``TranscriptGraph`` (LOCAL state ids) -- a start -> end path and the boundaries of its nodes' segments.
    For a candidate set (``TranscriptGraph.from_candidates``) that is the likelihood of "one of these transcripts"; where two
    paths spell the same class sequence (``TranscriptGraph.is_ambiguous``) its segmentations count once per path.
    -> dict(logz fp64 [b] (-inf: no alignment; NaN and the error word: a NaN reached the DP), ws (keep it for
    ``align_graph_logz_bwd``), _staged (classes, masks and flags on the device), _err, _keep).  ``ws``: at least
    ``align_graph_logz_workspace_bytes``.  ``staged``: the ``_staged`` entry of an earlier call for the same graphs: the call
    then copies nothing from the host itself and can be captured into a graph."""
    out = _logz_launch('graph', 'align_graph_logz', batch, elp, trans, init, len_scores, graphs, None, endpen, ws, staged)[0]
    return dict(out, _keep=(out['ws'],))


def _logz_bwd_launch(kind, what, batch, elp, trans, init, len_scores, given, optional, logz_val, grad_logz, endpen, ws, staged,
                     **posteriors):
    """smm_align_logz_bwd_f64, smm_align_opt_logz_bwd_f64 or smm_align_graph_logz_bwd_f64 by ``kind``.  ``posteriors``: the
    kind's optional outputs in the library's order (p_used, p_end), each under the key of the result it goes to and with
    whether it is wanted."""
    lib = _lib.load()
    f64 = torch.float64
    symbol, _, name = _TRANSCRIPT_LAUNCH[kind, 'likelihood']
    sup = _supervision(kind, 'likelihood', what, batch, elp.device, given, optional, staged)
    args = _tables(elp, trans, init, len_scores, endpen) + sup.args()
    if ws is None or ws.numel() < sup.need:
        raise ValueError("%s: pass the workspace the %s call wrote" % (what, what[:-len('_bwd')]))
    g = _grad_outputs(elp, trans, init, len_scores)
    post = {key: torch.empty(sup.n, dtype=f64, device=elp.device) if want else None for key, want in posteriors.items()}
    _lib.check(getattr(lib, symbol.replace('_f64', '_bwd_f64'))(
        *batch.head(), *args, _dev(logz_val, f64, name), _dev(grad_logz, f64, 'grad_logz'), _dev(g['elp'], f64, 'g_elp'),
        _dev(g['trans'], f64, 'g_trans'), _dev(g['init'], f64, 'g_init'), _dev(g['len'], f64, 'g_len'),
        *[_dev(t, f64, p) for t, p in zip(post.values(), ('p_used', 'p_end'))], *_ws_args(ws), _stream()))
    g.update((key, sup.per_video(t)) for key, t in post.items() if t is not None)
    if kind != 'chain':
        g['_keep'] = sup.dev
    return g


def align_logz_bwd(batch, elp, trans, init, len_scores, transcripts, logz_a, grad_logz=None, endpen=None, ws=None):
    """Gradient of sum_i grad_logz[i] * log Z_a(i) (smm_align_logz_bwd_f64).  Must follow ``align_logz`` for the same batch,
    tables and transcripts with the same workspace ``ws`` on the same stream; ``logz_a`` = its output.
    -> dict(elp [total_frames, c_max], trans, init, len) fp64; videos whose log Z_a is -inf or NaN contribute zeros."""
    return _logz_bwd_launch('chain', 'align_logz_bwd', batch, elp, trans, init, len_scores, transcripts, None, logz_a, grad_logz,
                            endpen, ws, None)


def align_opt_logz_bwd(batch, elp, trans, init, len_scores, transcripts, optional, logz_o, grad_logz=None, endpen=None, ws=None,
                       staged=None, want_entry_prob=False):
    """Gradient of sum_i grad_logz[i] * log Z_o(i) (smm_align_opt_logz_bwd_f64).  Must follow ``align_opt_logz`` for the same
    batch, tables, transcripts and flags with the same workspace ``ws`` on the same stream; ``logz_o`` = its output.
    -> dict(elp [total_frames, c_max], trans, init, len) fp64, plus with ``want_entry_prob`` entry_prob: a list of per-video
    fp64 views of one device tensor, the posterior probability that the entry has a segment (1 for a mandatory entry).  Videos
    whose log Z_o is -inf or NaN contribute zeros."""
    return _logz_bwd_launch('optional', 'align_opt_logz_bwd', batch, elp, trans, init, len_scores, transcripts, optional, logz_o,
                            grad_logz, endpen, ws, staged, entry_prob=want_entry_prob)


def align_graph_logz_bwd(batch, elp, trans, init, len_scores, graphs, logz_g, grad_logz=None, endpen=None, ws=None, staged=None,
                         want_node_prob=False, want_end_prob=False):
    """Gradient of sum_i grad_logz[i] * log Z_g(i) (smm_align_graph_logz_bwd_f64).  Must follow ``align_graph_logz`` for the
    same batch, tables and graphs with the same workspace ``ws`` on the same stream; ``logz_g`` = its output.
    -> dict(elp [total_frames, c_max], trans, init, len) fp64, plus with ``want_node_prob`` node_prob and with
    ``want_end_prob`` end_prob: lists of per-video fp64 views of one device tensor each, the posterior probability that the
    path crosses the node / ends in it (end_prob sums to 1 over a video's nodes).  Videos whose log Z_g is -inf or NaN
    contribute zeros."""
    return _logz_bwd_launch('graph', 'align_graph_logz_bwd', batch, elp, trans, init, len_scores, graphs, None, logz_g, grad_logz,
                            endpen, ws, staged, node_prob=want_node_prob, end_prob=want_end_prob)


def _after_graph_logz(what, batch, dev, graphs, staged, *workspaces):
    """What a call that follows ``align_graph_logz`` checks on the host: every workspace is there, the supervision, every
    workspace holds the layout.  -> the supervision."""
    if any(ws is None for ws in workspaces):
        raise ValueError("%s: pass the workspace the align_graph_logz call wrote" % what)
    sup = _supervision('graph', 'likelihood', what, batch, dev, graphs, None, staged)
    if any(ws.numel() < sup.need for ws in workspaces):
        raise ValueError("%s: pass the workspace the align_graph_logz call wrote" % what)
    return sup


def _q_side(q):
    """``q`` = (trans, len_scores, endpen or None, logz_g, ws) of a two-sided call, as the library takes it."""
    trans_q, len_q, endpen_q, logz_q, ws_q = q
    f64 = torch.float64
    return (_dev(trans_q, f64, 'trans'), _dev(len_q, f64, 'len_scores'), _dev(endpen_q, f64, 'endpen'), _dev(logz_q, f64, 'logz_g'),
            *_ws_args(ws_q))


def align_graph_sample(batch, elp, trans, init, len_scores, graphs, logz_g, n_samples, seed=0, endpen=None, class_map=None,
                       ws=None, staged=None, want_spans=True, want_labels=True, want_used=True):
    """Alignments drawn from the transcript-graph posterior (smm_align_graph_sample_f64): per video ``n_samples`` independent
    draws of a start -> end path of its ``TranscriptGraph`` (LOCAL state ids) and the boundaries of its nodes' segments, from
    the distribution whose normaliser ``align_graph_logz`` returns.  Must follow ``align_graph_logz`` for the same batch,
    tables and graphs with the same workspace ``ws`` on the same stream (``ws`` and ``staged``: its ``ws`` and ``_staged``
    entries); ``logz_g`` = its output.  ``align_graph_logz_bwd`` may run in between: the samples do not change.
    -> dict(spans int64 [n_samples, b, t_max+1] or None, labels int64 [n_samples, total_frames] (-1 on frames no video covers)
    or None, logp fp64 [n_samples, b]: the exact log-probability of the drawn alignment -- on an ambiguous graph of the path
    and its boundaries, not of the class sequence --, n_segs int32 [n_samples, b], used: a list of per-video int32
    [n_samples, M_i] views of one device tensor, 1 for the nodes of the sampled path, or None, _err, _keep).  A video without
    an alignment (log Z_g = -inf) gets spans and labels -1, n_segs 0, used 0 and logp NaN.  Sample j depends on
    (seed, video, j) only."""
    lib = _lib.load()
    n_samples = int(n_samples)
    if n_samples <= 0:
        raise ValueError("align_graph_sample: n_samples must be positive, got %d" % n_samples)
    f64 = torch.float64
    dev = elp.device
    sup = _after_graph_logz('align_graph_sample', batch, dev, graphs, staged, ws)
    tables = _tables(elp, trans, init, len_scores, endpen)
    spans, labels, logp, n_segs = _device_outputs(batch, dev, want_spans, want_labels, (n_samples,))
    used = torch.empty((n_samples, sup.n), dtype=torch.int32, device=dev) if want_used else None
    _lib.check(lib.smm_align_graph_sample_f64(
        *batch.head(), *tables, _dev(class_map, torch.int64, 'class_map'), *sup.args(), _dev(logz_g, f64, 'logz_g'),
        ctypes.c_int32(n_samples), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), _dev(spans, torch.int64, 'spans'),
        _dev(labels, torch.int64, 'labels'), _dev(logp, f64, 'logp'), _dev(n_segs, torch.int32, 'n_segs'),
        _dev(used, torch.int32, 'used'), *_ws_args(ws), _stream()))
    return dict(spans=spans, labels=labels, logp=logp, n_segs=n_segs, used=None if used is None else sup.per_video(used, dim=1),
                _err=_err_copy(batch, ws), _staged=sup.dev, _keep=(ws,))


def align_graph_entropy(batch, elp, trans, init, len_scores, graphs, logz_g, endpen=None, ws=None, staged=None, want_parts=False):
    """The exact entropy of the transcript-graph posterior (smm_align_graph_entropy_f64): per video H = -sum p log p in nats
    over the ALIGNMENTS of the video to its ``TranscriptGraph`` -- the distribution ``align_graph_sample`` draws from, whose
    normaliser ``align_graph_logz`` returns.  Must follow ``align_graph_logz`` for the same batch, tables and graphs with the
    same workspace ``ws`` on the same stream (``ws`` and ``staged``: its ``ws`` and ``_staged`` entries); ``logz_g`` = its
    output.  ``align_graph_logz_bwd`` and ``align_graph_sample`` may run before or after it: neither's results change.
    -> dict(entropy fp64 [b], parts fp64 [b, 3] (with ``want_parts``: the entropy of the end node -- for a trie of the
    posterior over the candidates --, of the segments' starts, and of the predecessors; they add up to ``entropy``) or None,
    _err, _staged, _keep).  A video without an alignment (log Z_g = -inf) gets NaN.  Gradient: ``align_graph_entropy_bwd``."""
    lib = _lib.load()
    f64 = torch.float64
    dev = elp.device
    sup = _after_graph_logz('align_graph_entropy', batch, dev, graphs, staged, ws)
    tables = _tables(elp, trans, init, len_scores, endpen)
    entropy = torch.empty(batch.b, dtype=f64, device=dev)
    parts = torch.empty((batch.b, 3), dtype=f64, device=dev) if want_parts else None
    _lib.check(lib.smm_align_graph_entropy_f64(
        *batch.head(), *tables, *sup.args(), _dev(logz_g, f64, 'logz_g'), _dev(entropy, f64, 'entropy'), _dev(parts, f64, 'parts'),
        *_ws_args(ws), _stream()))
    return dict(entropy=entropy, parts=parts, _err=_err_copy(batch, ws), _staged=sup.dev, _keep=(ws,))


def align_graph_segment_posteriors(batch, elp, trans, init, len_scores, graphs, logz_g, spans=None, used=None, endpen=None,
                                   class_map=None, ws=None, staged=None, want_moments=True, want_dense=False):
    """The exact posterior of each segment of given alignments under the transcript-graph posterior, and where each node's
    segment starts and ends (smm_align_graph_segment_posteriors_f64).  Must follow ``align_graph_logz`` for the same batch,
    tables and graphs with the same workspace ``ws`` on the same stream (``ws`` and ``staged``: its ``ws`` and ``_staged``
    entries); ``logz_g`` = its output.  ``align_graph_logz_bwd``, ``align_graph_sample`` and ``align_graph_entropy`` may run
    before or after it: none's results change.  ``spans`` int64 [n_sets, b, t_max+1] or [b, t_max+1] and ``used`` int32
    [n_sets, n_nodes] or [n_nodes] (or the list of per-video views ``align_graph`` / ``align_graph_sample`` return), both on the
    device: alignments as those two write them, the k-th span of a video standing for its k-th used node; ``class_map`` as
    given to them.  -> dict(seg_logp fp64 shaped like ``spans`` or None: at each span start the log posterior that this node
    covers exactly these frames, 0 at the EOS position, -inf elsewhere; node_logp: a list of per-video fp64 views ([n_sets,] M_i),
    the same value per used node, -inf for the others, or None; end_mean, end_sd, start_mean, start_sd (``want_moments``):
    lists of per-video fp64 [M_i] views, mean and standard deviation in frames of the node's end and start position given that
    the path crosses it, NaN for a node without mass; node_end_post, node_start_post (``want_dense``) fp64 [n_nodes, t_max+1]:
    P(node m's segment ends / starts at position n), 8 (t_max+1) bytes per node each; _err, _staged, _keep).  An alignment the
    graph does not admit -- its spans and used nodes differ in number, a span's class is not its node's, a span is longer than
    the span limit -- gets -inf everywhere, without an error.  A video without an alignment (log Z_g = -inf) gets NaN.  Values,
    not differentiable."""
    f64 = torch.float64
    dev = elp.device
    if (spans is None) != (used is None):
        raise ValueError("align_graph_segment_posteriors: pass spans and used together")
    if spans is None and not want_moments and not want_dense:
        raise ValueError("align_graph_segment_posteriors: nothing is asked for")
    n_sets = 0
    if spans is not None:
        if isinstance(used, (list, tuple)):
            used = torch.cat(list(used), dim=-1)
        if spans.dtype != torch.int64 or used.dtype != torch.int32:
            raise TypeError("align_graph_segment_posteriors: spans int64 and used int32 expected, got %s and %s" % (spans.dtype, used.dtype))
        if spans.dim() not in (2, 3) or tuple(spans.shape[-2:]) != (batch.b, batch.t_max + 1):
            raise ValueError("align_graph_segment_posteriors: spans [n_sets, b, t_max+1] or [b, t_max+1] = [.., %d, %d] expected, "
                             "got %s" % (batch.b, batch.t_max + 1, tuple(spans.shape)))
        n_sets = int(spans.shape[0]) if spans.dim() == 3 else 1
        n_nodes = sum(len(g) for g in graphs)
        if n_sets <= 0 or tuple(used.shape) != ((n_sets, n_nodes) if spans.dim() == 3 else (n_nodes,)):
            raise ValueError("align_graph_segment_posteriors: used [n_sets, %d] to go with spans %s expected, got %s"
                             % (n_nodes, tuple(spans.shape), tuple(used.shape)))
        used = used.contiguous()
    sup = _after_graph_logz('align_graph_segment_posteriors', batch, dev, graphs, staged, ws)
    lib = _lib.load()
    tables = _tables(elp, trans, init, len_scores, endpen)
    seg = None if spans is None else torch.empty(spans.shape, dtype=f64, device=dev)
    node = None if spans is None else torch.empty(used.shape, dtype=f64, device=dev)
    mom = [torch.empty(sup.n, dtype=f64, device=dev) if want_moments else None for _ in range(4)]
    dense = [torch.empty((sup.n, batch.t_max + 1), dtype=f64, device=dev) if want_dense else None for _ in range(2)]
    _lib.check(lib.smm_align_graph_segment_posteriors_f64(
        *batch.head(), *tables, _dev(class_map, torch.int64, 'class_map'), *sup.args(), _dev(logz_g, f64, 'logz_g'),
        _dev(spans, torch.int64, 'spans'), _dev(used, torch.int32, 'used'), ctypes.c_int32(n_sets), _dev(seg, f64, 'seg_logp'),
        _dev(node, f64, 'node_logp'), *[_dev(t, f64, 'moments') for t in mom], *[_dev(t, f64, 'dense') for t in dense],
        *_ws_args(ws), _stream()))
    per = lambda t, dim=0: None if t is None else sup.per_video(t, dim=dim)
    return dict(seg_logp=seg, node_logp=per(node, node.dim() - 1 if node is not None else 0),
                end_mean=per(mom[0]), end_sd=per(mom[1]), start_mean=per(mom[2]), start_sd=per(mom[3]),
                node_end_post=dense[0], node_start_post=dense[1], _err=_err_copy(batch, ws), _staged=sup.dev, _keep=(ws,))


def align_graph_kl(batch, p, q, graphs, staged=None, want_cross_entropy=False, want_parts=False):
    """The exact KL divergence KL(p || q) between two transcript-graph posteriors over the ALIGNMENTS of the same videos to the
    same ``TranscriptGraph``s (smm_align_graph_kl_f64), in nats, and with ``want_cross_entropy`` H(p, q) = -sum p log q.
    ``p`` = (elp, trans, init, len_scores, endpen or None, logz_g, ws) and ``q`` = (trans, len_scores, endpen or None, logz_g, ws):
    each side's tables and the ``logz`` and ``ws`` entries of its own ``align_graph_logz`` call for this batch and these graphs,
    both on the current stream.  q's workspace is only read (its elp and init entered through it); p's is used as
    ``align_graph_entropy`` uses it, so p's backward, sampler and entropy results do not change.  ``staged``: either call's
    ``_staged`` entry.  -> dict(kl fp64 [b], cross_entropy fp64 [b] or None, parts fp64 [b, 3] (with ``want_parts``: the KL of
    the end node -- for a trie the KL between the posteriors over the candidates --, of the segments' starts, and of the
    predecessors; they add up to ``kl``) or None, _err, _staged, _keep).  Bit-identical sides give exactly 0.  A video p cannot
    align (log Z_g = -inf) gets NaN; one p can align and q cannot gets +inf, as does one where p puts mass on an alignment q
    excludes.  Gradient: ``align_graph_kl_bwd``."""
    lib = _lib.load()
    elp, trans, init, len_scores, endpen, logz_p, ws_p = p
    ws_q = tuple(q)[4:]                                           # (a malformed q fails in _q_side's unpacking)
    f64 = torch.float64
    dev = elp.device
    sup = _after_graph_logz('align_graph_kl', batch, dev, graphs, staged, ws_p, *ws_q)
    tables = _tables(elp, trans, init, len_scores, endpen)
    kl = torch.empty(batch.b, dtype=f64, device=dev)
    xent = torch.empty(batch.b, dtype=f64, device=dev) if want_cross_entropy else None
    parts = torch.empty((batch.b, 3), dtype=f64, device=dev) if want_parts else None
    _lib.check(lib.smm_align_graph_kl_f64(
        *batch.head(), *tables, _dev(logz_p, f64, 'logz_g'), *_ws_args(ws_p), *_q_side(q), *sup.args(), _dev(kl, f64, 'kl'),
        _dev(xent, f64, 'cross_entropy'), _dev(parts, f64, 'parts'), _stream()))
    return dict(kl=kl, cross_entropy=xent, parts=parts, _err=_err_copy(batch, ws_p), _staged=sup.dev, _keep=(ws_p, *ws_q))


def align_graph_entropy_bwd_scratch_bytes(batch, node_offset):
    """Bytes of scratch smm_align_graph_entropy_bwd_f64 / smm_align_graph_kl_bwd_f64 need for this batch and these node
    offsets (int64 [b + 1]; host only); raises ValueError for what the calls refuse."""
    off = np.ascontiguousarray(node_offset, dtype=np.int64)
    n = _lib.load().smm_align_graph_entropy_bwd_scratch_bytes(ctypes.byref(batch.shape), ctypes.c_void_p(batch.lengths.ctypes.data),
                                                              ctypes.c_void_p(off.ctypes.data))
    if n == 0:
        raise ValueError("align_graph_entropy_bwd: the library refuses this batch and these node offsets")
    return int(n)


def _graph_value_bwd(what, batch, p, q, graphs, grad_out, staged, mode, scratch=None):
    """smm_align_graph_entropy_bwd_f64 (``q`` None) or smm_align_graph_kl_bwd_f64 with ``mode``.  Every check on the host
    arrays comes before a device is touched.  ``scratch``: a uint8 tensor of at least
    ``align_graph_entropy_bwd_scratch_bytes`` (its contents do not matter); default: a private one."""
    lib = _lib.load()
    elp, trans, init, len_scores, endpen, logz_p, ws_p = p
    f64 = torch.float64
    dev = elp.device
    ws_q = () if q is None else tuple(q)[4:]                      # (a malformed q fails in _q_side's unpacking)
    sup = _after_graph_logz(what, batch, dev, graphs, staged, ws_p, *ws_q)
    if ws_q and ws_q[0].data_ptr() == ws_p.data_ptr():
        raise ValueError("%s: the two sides need a workspace each (one posterior against itself: align_graph_entropy_bwd)" % what)
    need = align_graph_entropy_bwd_scratch_bytes(batch, sup.off)
    tables = _tables(elp, trans, init, len_scores, endpen)
    g = _grad_outputs(elp, trans, init, len_scores)
    value = torch.empty(batch.b, dtype=f64, device=dev)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif scratch.dtype != torch.uint8 or scratch.numel() < need:
        raise ValueError("%s: scratch must be a uint8 tensor of at least %d bytes" % (what, need))
    outs = (_dev(grad_out, f64, 'grad_out'), _dev(g['elp'], f64, 'g_elp'), _dev(g['trans'], f64, 'g_trans'),
            _dev(g['init'], f64, 'g_init'), _dev(g['len'], f64, 'g_len'), _dev(value, f64, 'value'), *_ws_args(scratch))
    if q is None:
        _lib.check(lib.smm_align_graph_entropy_bwd_f64(
            *batch.head(), *tables, *sup.args(), _dev(logz_p, f64, 'logz_g'), *outs, *_ws_args(ws_p), _stream()))
        keep = (ws_p, scratch)
    else:
        _lib.check(lib.smm_align_graph_kl_bwd_f64(
            *batch.head(), *tables, _dev(logz_p, f64, 'logz_g'), *_ws_args(ws_p), *_q_side(q), *sup.args(), ctypes.c_int32(mode),
            *outs, _stream()))
        keep = (ws_p, *ws_q, scratch)
    g.update(value=value, value_plus=scratch[:need].view(f64)[-batch.b:], _err=_err_copy(batch, ws_p), _staged=sup.dev, _keep=keep)
    return g


def align_graph_entropy_bwd(batch, elp, trans, init, len_scores, graphs, logz_g, grad_out=None, endpen=None, ws=None, staged=None,
                            scratch=None):
    """Gradient of sum_i grad_out[i] * H_i, the entropy ``align_graph_entropy`` returns, with respect to the tables
    (smm_align_graph_entropy_bwd_f64).  Must follow ``align_graph_logz`` for the same batch, tables and graphs with the same
    workspace ``ws`` on the same stream; ``logz_g`` = its output.  The backward, sampler, entropy and KL results on that
    workspace do not change.  -> dict(elp [total_frames, c_max], trans, init, len fp64, value fp64 [b]: H by the message pass
    over the sampler's decisions (value_plus: by the time-forward walk's), _err, _staged, _keep).  A video without an
    alignment contributes zeros and gets the value NaN.  ``scratch``: the caller's, of ``align_graph_entropy_bwd_scratch_bytes``
    (uint8; it need not be initialised); default: a private one."""
    return _graph_value_bwd('align_graph_entropy_bwd', batch, (elp, trans, init, len_scores, endpen, logz_g, ws), None, graphs,
                            grad_out, staged, 0, scratch)


def align_graph_kl_bwd(batch, p, q, graphs, grad_out=None, staged=None, cross_entropy=False, scratch=None):
    """Gradient of sum_i grad_out[i] * KL_i(p || q), or with ``cross_entropy`` of H_i(p, q), with respect to p's tables
    (smm_align_graph_kl_bwd_f64).  ``p`` and ``q`` as ``align_graph_kl`` takes them.  q's workspace receives what q's own
    ``align_graph_logz_bwd`` would write first, so neither side's later results change.  The gradient with respect to q's
    tables is mu_q - mu_p from two ``align_graph_logz_bwd`` calls.  -> dict(elp, trans, init, len, value, value_plus, _err,
    _staged, _keep) as ``align_graph_entropy_bwd``.  Bit-identical sides give exactly 0 everywhere in the KL mode; a video
    whose value is +inf gets NaN rows and makes its group's tables NaN; a q workspace written for other graphs (the columns'
    recorded ranges differ) gives that video NaN, zeros and the error word, and is not written.  The two sides need a workspace
    each.  ``scratch``: as ``align_graph_entropy_bwd``'s."""
    return _graph_value_bwd('align_graph_kl_bwd', batch, p, q, graphs, grad_out, staged,
                            _lib.KL_BWD_CROSS_ENTROPY if cross_entropy else _lib.KL_BWD_KL, scratch)


def _graph_reward_scratch_bytes(symbol, batch, node_offset):
    off = np.ascontiguousarray(node_offset, dtype=np.int64)
    n = getattr(_lib.load(), symbol)(ctypes.byref(batch.shape), ctypes.c_void_p(batch.lengths.ctypes.data),
                                     ctypes.c_void_p(off.ctypes.data))
    if n == 0:
        raise ValueError("align_graph_expected_reward: the library refuses this batch and these node offsets")
    return int(n)


def align_graph_expected_reward_scratch_bytes(batch, node_offset):
    """Bytes of scratch smm_align_graph_expected_reward_f64 needs for this batch and these node offsets (int64 [b + 1]; host
    only); raises ValueError for what the call refuses."""
    return _graph_reward_scratch_bytes('smm_align_graph_expected_reward_scratch_bytes', batch, node_offset)


def align_graph_expected_reward_bwd_scratch_bytes(batch, node_offset):
    """... smm_align_graph_expected_reward_bwd_f64 needs."""
    return _graph_reward_scratch_bytes('smm_align_graph_expected_reward_bwd_scratch_bytes', batch, node_offset)


def _graph_reward_call(what, batch, elp, graphs, reward, node_reward, ws, staged, scratch, need_of):
    """What both expected-reward calls check before a device is touched: the workspace and the supervision as every call behind
    ``align_graph_logz``, the rewards' shapes, the scratch.  ``node_reward``: one fp64 tensor over all nodes or a list of
    per-video ones.  -> (supervision, reward, node_reward, scratch, bytes needed)."""
    dev = elp.device
    if reward is None and node_reward is None:
        raise ValueError("%s: pass reward, node_reward or both" % what)
    sup = _after_graph_logz(what, batch, dev, graphs, staged, ws)
    if reward is not None and (reward.dtype != torch.float64 or tuple(reward.shape) != tuple(elp.shape)):
        raise ValueError("%s: reward must be fp64 %s like elp, got %s %s" % (what, tuple(elp.shape), reward.dtype, tuple(reward.shape)))
    if isinstance(node_reward, (list, tuple)):
        node_reward = torch.cat([r.reshape(-1) for r in node_reward])
    if node_reward is not None and (node_reward.dtype != torch.float64 or tuple(node_reward.shape) != (sup.n,)):
        raise ValueError("%s: node_reward must be fp64 [%d], one entry per node, got %s %s"
                         % (what, sup.n, node_reward.dtype, tuple(node_reward.shape)))
    need = need_of(batch, sup.off)
    if scratch is not None and (scratch.dtype != torch.uint8 or scratch.numel() < need):
        raise ValueError("%s: scratch must be a uint8 tensor of at least %d bytes" % (what, need))
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    return sup, reward, node_reward, scratch, need


def align_graph_expected_reward(batch, elp, trans, init, len_scores, graphs, logz_g, reward=None, node_reward=None, endpen=None,
                                ws=None, staged=None, scratch=None, want_parts=False):
    """The expectation of a frame- and node-additive reward under the transcript-graph posterior
    (smm_align_graph_expected_reward_f64): per video V = E[ sum over the segments (node j, frames s .. n-1) of the alignment of
    node_reward[j] + sum_t reward[t, a_j] ].  ``reward`` fp64 [total_frames, c_max] (local states as columns) and/or
    ``node_reward`` fp64 [n_nodes] (or a list of per-video tensors), laid out like the graphs' nodes.  Must follow
    ``align_graph_logz`` for the same batch, tables and graphs with the same workspace ``ws`` on the same stream (``ws`` and
    ``staged``: its ``ws`` and ``_staged`` entries); ``logz_g`` = its output.  The backward, sampler, entropy, segment-posterior
    and KL results on that workspace do not change.  -> dict(value fp64 [b], parts fp64 [b, 2] (with ``want_parts``: the frame
    part and the node part) or None, _err, _staged, _keep).  A video without an alignment (log Z_g = -inf) gets NaN; a reward
    that is not finite gives its video NaN and sets the error word.  ``scratch``: the caller's, of
    ``align_graph_expected_reward_scratch_bytes`` (uint8; it need not be initialised); default: a private one.
    Gradient: ``align_graph_expected_reward_bwd``."""
    what = 'align_graph_expected_reward'
    sup, reward, node_reward, scratch, _ = _graph_reward_call(what, batch, elp, graphs, reward, node_reward, ws, staged, scratch,
                                                              align_graph_expected_reward_scratch_bytes)
    lib = _lib.load()
    f64 = torch.float64
    dev = elp.device
    tables = _tables(elp, trans, init, len_scores, endpen)
    value = torch.empty(batch.b, dtype=f64, device=dev)
    parts = torch.empty((batch.b, 2), dtype=f64, device=dev) if want_parts else None
    _lib.check(lib.smm_align_graph_expected_reward_f64(
        *batch.head(), *tables, *sup.args(), _dev(logz_g, f64, 'logz_g'), _dev(reward, f64, 'reward'),
        _dev(node_reward, f64, 'node_reward'), _dev(value, f64, 'value'), _dev(parts, f64, 'parts'), *_ws_args(scratch),
        *_ws_args(ws), _stream()))
    return dict(value=value, parts=parts, _err=_err_copy(batch, ws), _staged=sup.dev, _keep=(ws, scratch, reward, node_reward))


def align_graph_expected_reward_bwd(batch, elp, trans, init, len_scores, graphs, logz_g, reward=None, node_reward=None,
                                    grad_out=None, endpen=None, ws=None, staged=None, scratch=None, want_value=False):
    """Gradient of sum_i grad_out[i] * V_i, the value ``align_graph_expected_reward`` returns, with respect to the tables
    (smm_align_graph_expected_reward_bwd_f64): a Hessian-vector product of log Z_g.  Arguments and call order as
    ``align_graph_expected_reward``.  -> dict(elp [total_frames, c_max], trans, init, len fp64, value fp64 [b] (with
    ``want_value``, else None): V by the message pass over the sampler's decisions, value_plus: by the time-forward walk's,
    _err, _staged, _keep).  There is no gradient for the rewards: V is linear in them (``align_graph_logz_bwd``'s elp and
    node_prob).  A video without an alignment contributes zeros; ``grad_out[i] = 0`` gives exact zeros.  ``scratch``: the
    caller's, of ``align_graph_expected_reward_bwd_scratch_bytes``."""
    what = 'align_graph_expected_reward_bwd'
    sup, reward, node_reward, scratch, _ = _graph_reward_call(what, batch, elp, graphs, reward, node_reward, ws, staged, scratch,
                                                              align_graph_expected_reward_bwd_scratch_bytes)
    lib = _lib.load()
    f64 = torch.float64
    dev = elp.device
    tables = _tables(elp, trans, init, len_scores, endpen)
    g = _grad_outputs(elp, trans, init, len_scores)
    both = torch.empty((batch.b, 2), dtype=f64, device=dev) if want_value else None
    _lib.check(lib.smm_align_graph_expected_reward_bwd_f64(
        *batch.head(), *tables, *sup.args(), _dev(logz_g, f64, 'logz_g'), _dev(reward, f64, 'reward'),
        _dev(node_reward, f64, 'node_reward'), _dev(grad_out, f64, 'grad_out'), _dev(g['elp'], f64, 'g_elp'),
        _dev(g['trans'], f64, 'g_trans'), _dev(g['init'], f64, 'g_init'), _dev(g['len'], f64, 'g_len'), _dev(both, f64, 'value'),
        *_ws_args(scratch), *_ws_args(ws), _stream()))
    g.update(value=None if both is None else both[:, 0], value_plus=None if both is None else both[:, 1],
             _err=_err_copy(batch, ws), _staged=sup.dev, _keep=(ws, scratch, reward, node_reward))
    return g


def transcript_is_ambiguous(ids, optional):
    """Host only: True when two different subsets of the optional entries of this transcript give the same non-empty class
    sequence -- ``align_opt_logz`` then counts the segmentations with that class sequence once per subset.  Exact: over the
    pairs (i, j) with ids[i] == ids[j], `reach` says that a kept-entry path ending in i and one ending in j spell the same
    labels, `diff` that two such paths differ somewhere; each is one rectangle query on a 2-D prefix sum over
    pred(i) x pred(j), O(M^2) in all."""
    a = np.asarray(ids.detach().cpu() if torch.is_tensor(ids) else ids, dtype=np.int64).reshape(-1)
    opt = np.asarray(optional.detach().cpu() if torch.is_tensor(optional) else optional).reshape(-1) != 0
    M = a.shape[0]
    if opt.shape[0] != M:
        raise ValueError("transcript_is_ambiguous: %d flags for %d entries" % (opt.shape[0], M))
    if M == 0:
        return False
    plo, head = np.zeros(M, np.int64), 0
    for m in range(M):
        plo[m] = head
        if not opt[m]:
            head = m
    first = [bool(opt[:m].all()) for m in range(M)]
    end = [bool(opt[m + 1:].all()) for m in range(M)]
    reach = np.zeros((M + 1, M + 1), np.int64)      # 2-D inclusive prefix sums, shifted by one
    diff = np.zeros((M + 1, M + 1), np.int64)

    def rect(p, i0, i1, j0, j1):                    # the sum over [i0, i1) x [j0, j1)
        return p[i1, j1] - p[i0, j1] - p[i1, j0] + p[i0, j0]

    for i in range(M):
        for j in range(M):
            r = d = 0
            if a[i] == a[j]:
                r = int((first[i] and first[j]) or rect(reach, plo[i], i, plo[j], j) > 0)
                d = int(r and (i != j or rect(diff, plo[i], i, plo[j], j) > 0))
                if d and end[i] and end[j]:
                    return True
            reach[i + 1, j + 1] = r + reach[i, j + 1] + reach[i + 1, j] - reach[i, j]
            diff[i + 1, j + 1] = d + diff[i, j + 1] + diff[i + 1, j] - diff[i, j]
    return False


_pinned = {}


def to_host(t):
    """Device -> host copy through a cached pinned staging buffer (pageable copies are staged by the runtime and
    run at a fraction of the PCIe rate).  Returns a CPU tensor that is valid until the next call for the same dtype."""
    key = (t.dtype, t.device.index)
    buf = _pinned.get(key)
    if buf is None or buf.numel() < t.numel():
        buf = torch.empty(int(t.numel() * 1.25) + 16, dtype=t.dtype, pin_memory=True)
        _pinned[key] = buf
    out = buf[:t.numel()].view(t.shape)
    out.copy_(t, non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return out


def _err_view(batch, ws):
    """int32 view of the error word inside the workspace a launch was given (the kernels of that launch write it)."""
    off = _lib.load().smm_error_word_offset(ctypes.byref(batch.shape))
    return ws[off:off + 32].view(torch.int32)      # [error, 0, band-0 sources pushed, band-blocks evaluated, videos split in time, of those decoded again in one piece, why (bits), one-class-run ties resolved]


def _err_copy(batch, ws):
    """The launch's error words COPIED out of the workspace (32 bytes, stream-ordered behind the kernels, graph-capturable):
    the per-stream workspace is shared, and the next launch on the stream re-stages it and zeroes these words."""
    # (an elementwise kernel, not clone(): torch copies device -> device with hipMemcpyAsync, and memset / memcpy nodes are
    # what replayed wrongly from a captured hipGraph on ROCm 7.2 -- tests/test_gpu_graph.py; kernel nodes replay correctly)
    return torch.add(_err_view(batch, ws), 0)


def error_flag(batch, out=None, ws=None):
    """The kernels' error word of a decode (synchronises): non-zero means a NaN (or inf - inf) reached the DP and the
    decode of that video stopped early.  ``out``: the dict the launch returned (its ``_err`` entry views the workspace
    that launch wrote to -- the per-stream cache may have been regrown or switched since); without it the current
    (device, stream) workspace is read, which is only right directly after the launch."""
    return error_words(batch, out, ws)[0]


def error_words(batch, out=None, ws=None):
    """[error word, 0, sources pushed into band 0, delayed band-blocks evaluated (words 2 and 3: diagnostics of the Viterbi
    kernel's BAND mode, smm_viterbi.hip: DOM and the band skip test), videos decoded as several units along the time axis, of
    those the ones that were decoded again in one piece, why (a bit mask: 1 a cut did not certify, 2 the closing step, 4 two
    states within the margin, 8 two lengths within the margin, 16 NaN or too many segments, 32 a decision clear of the rounding
    margin but not of the spread the cuts in front of it let through), one-class-run ties the stitch resolved (words 4..7:
    csrc/smm_chunk.hip)] of a decode (synchronises).
    (Words 1 and 2 counted gang time-outs in rounds 1-3.)"""
    if out is not None and out.get('_err') is not None:
        return [int(v) for v in out['_err'].tolist()]
    if ws is None:
        ws = workspace(batch.workspace_bytes(), torch.device('cuda', torch.cuda.current_device()))
    return [int(v) for v in _err_view(batch, ws).tolist()]


def check_decoded(batch, out=None):
    """Call after the decode's outputs have reached the host (the stream is idle then): raises SmmError when the DP
    kernel flagged the run: a NaN / inf - inf reached the DP of some video and its decode stopped early."""
    flag = error_words(batch, out)[0]
    if flag != 0:
        raise _lib.SmmError("libsmmdp: NaN (or inf - inf) in the DP inputs; decode stopped early (error word %d)" % flag)


# ------------------------------------------------------------------------------------------------ evaluation counters
class EvalBatch:
    """Host metadata of one evaluation call: videos on the packed frame axis, their task and index inside the task."""

    def __init__(self, lengths, frame_offset, group, n_groups, c_max, n_labels, gt_width=1, video_key=None,
                 total_frames=None):
        self.lengths = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
        self.b = int(self.lengths.shape[0])
        self.frame_offset = np.ascontiguousarray(np.asarray(frame_offset, dtype=np.int64).reshape(-1))
        self.group = np.ascontiguousarray(np.asarray(group, dtype=np.int32).reshape(-1))
        self.video_key = None if video_key is None else np.ascontiguousarray(np.asarray(video_key, dtype=np.int32).reshape(-1))
        self.n_groups, self.c_max, self.n_labels, self.gt_width = int(n_groups), int(c_max), int(n_labels), int(gt_width)
        if self.c_max > _lib.EVAL_MAX_LABELS:
            raise _lib.SmmError("libsmmdp: a task with %d labels exceeds SMM_EVAL_MAX_LABELS" % self.c_max)
        if total_frames is None:
            total_frames = int((self.frame_offset + self.lengths).max())
        self.total_frames = int(total_frames)
        self.shape = _lib.SmmEvalShape(self.b, self.n_groups, self.c_max, self.n_labels, self.gt_width,
                                       int(self.lengths.max()), self.total_frames)

    def workspace_bytes(self):
        n = _lib.load().smm_eval_workspace_bytes(ctypes.byref(self.shape), self.lengths.ctypes.data)
        if n == 0:
            raise _lib.SmmError("libsmmdp: invalid evaluation batch shape")
        return n


def _eval_check(eb, pred, gt):
    if pred.numel() < eb.total_frames or gt.numel() < eb.total_frames * eb.gt_width:
        raise ValueError("pred / gt shorter than the packed frame axis")


def eval_confusion(eb, pred, gt, local_of):
    """(first gt label, predicted label) frame counts per task: int64 [n_groups, c_max+1, c_max+1].  (smm_eval_confusion_i64)"""
    lib = _lib.load()
    _eval_check(eb, pred, gt)
    dev = pred.device
    conf = torch.empty((eb.n_groups, eb.c_max + 1, eb.c_max + 1), dtype=torch.int64, device=dev)
    ws = workspace(eb.workspace_bytes(), dev)
    _lib.check(lib.smm_eval_confusion_i64(
        ctypes.byref(eb.shape), ctypes.c_void_p(eb.lengths.ctypes.data), ctypes.c_void_p(eb.frame_offset.ctypes.data),
        ctypes.c_void_p(eb.group.ctypes.data), _dev(pred, torch.int64, 'pred'), _dev(gt, torch.int64, 'gt'),
        _dev(local_of, torch.int32, 'local_of'), _dev(conf, torch.int64, 'confusion'),
        *_ws_args(ws), _stream()))
    return conf


def eval_videos(eb, pred, gt, local_of, cluster_of, gt_is_bg, pred_is_bg, seed=0):
    """Per-video counters int64 [b, EVAL_COUNTERS] (columns: _lib.EVAL_COUNTER_NAMES).  (smm_eval_videos_i64)"""
    lib = _lib.load()
    _eval_check(eb, pred, gt)
    dev = pred.device
    out = torch.empty((eb.b, _lib.EVAL_COUNTERS), dtype=torch.int64, device=dev)
    ws = workspace(eb.workspace_bytes(), dev)
    _lib.check(lib.smm_eval_videos_i64(
        ctypes.byref(eb.shape), ctypes.c_void_p(eb.lengths.ctypes.data), ctypes.c_void_p(eb.frame_offset.ctypes.data),
        ctypes.c_void_p(eb.group.ctypes.data),
        ctypes.c_void_p(None if eb.video_key is None else eb.video_key.ctypes.data),
        _dev(pred, torch.int64, 'pred'), _dev(gt, torch.int64, 'gt'), _dev(local_of, torch.int32, 'local_of'),
        _dev(cluster_of, torch.int32, 'cluster_of'), _dev(gt_is_bg, torch.uint8, 'gt_is_bg'),
        _dev(pred_is_bg, torch.uint8, 'pred_is_bg'), ctypes.c_uint32(int(seed) & 0xFFFFFFFF),
        _dev(out, torch.int64, 'counters'), *_ws_args(ws), _stream()))
    return out


# ------------------------------------------------------------------------------------------------ closed-form fit
def fit_stats(x, labels, lengths, frame_offset, n_classes, max_k):
    """Sufficient statistics of the supervised fit for videos on the packed frame axis (smm_fit_stats_f64).

    x cuda fp32 [F, D], labels cuda int64 [F] -> dict of cuda tensors: sum_x fp64 [n_classes, D], sum_x2 fp64 [D],
    frame_counts / span_counts / span_start_counts int64 [n_classes], span_transition_counts int64 [to, from].
    """
    lib = _lib.load()
    dev = x.device
    ln = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    fo = np.ascontiguousarray(np.asarray(frame_offset, dtype=np.int64).reshape(-1))
    b, d = int(ln.shape[0]), int(x.shape[1])
    n = int(n_classes)
    out = dict(sum_x=torch.empty((n, d), dtype=torch.float64, device=dev),
               sum_x2=torch.empty(d, dtype=torch.float64, device=dev),
               frame_counts=torch.empty(n, dtype=torch.int64, device=dev),
               span_counts=torch.empty(n, dtype=torch.int64, device=dev),
               span_start_counts=torch.empty(n, dtype=torch.int64, device=dev),
               span_transition_counts=torch.empty((n, n), dtype=torch.int64, device=dev))
    ws = workspace(lib.smm_fit_workspace_bytes(b), dev)
    _lib.check(lib.smm_fit_stats_f64(
        ctypes.c_int32(b), ctypes.c_void_p(ln.ctypes.data), ctypes.c_void_p(fo.ctypes.data),
        ctypes.c_int64(int(x.shape[0])), ctypes.c_int32(d), ctypes.c_int32(n),
        ctypes.c_int32(0 if max_k is None else int(max_k)), _dev(x, torch.float32, 'x'),
        _dev(labels, torch.int64, 'labels'), _dev(out['sum_x'], torch.float64, 'sum_x'),
        _dev(out['sum_x2'], torch.float64, 'sum_x2'), _dev(out['frame_counts'], torch.int64, 'frame_counts'),
        _dev(out['span_counts'], torch.int64, 'span_counts'),
        _dev(out['span_start_counts'], torch.int64, 'span_start_counts'),
        _dev(out['span_transition_counts'], torch.int64, 'span_transition_counts'),
        *_ws_args(ws), _stream()))
    off = lib.smm_fit_error_word_offset(b)
    out['_err'] = ws[off:off + 4].view(torch.int32).clone()     # (a copy, stream-ordered behind the kernels: the shared
    return out                                                   #  workspace may be reused by the next call)


def dp_timing(on):
    """Measurement aid (smmdp.h: smm_dp_timing_enable): HIP event pairs around every DP kernel launch the library makes."""
    _lib.load().smm_dp_timing_enable(1 if on else 0)


def dp_timing_read(cap=4096, tagged=False):
    """Durations (ms, launch order) of the DP kernel launches recorded since the last read; waits for them.
    ``tagged``: (ms, tag) pairs -- tag 0: the only DP launch of its call, 1: the critical videos of a split decode
    (caller's stream), 2: the rest of a split decode (the library's second stream), 3: the <= 16-state videos of a CU-time-bound
    part in four-wave workgroups, two per CU, on the library's side stream (beside a launch of tag 0 or 2)."""
    buf = (ctypes.c_float * cap)()
    tags = (ctypes.c_int32 * cap)()
    n = _lib.load().smm_dp_timing_read_tagged(buf, tags, cap)
    if tagged:
        return [(float(buf[i]), int(tags[i])) for i in range(min(n, cap))]
    return [float(buf[i]) for i in range(min(n, cap))]


def plan_feedback_info():
    """What plan feedback (smmdp.h: smm_plan_feedback_info) has done to the resident plan the last decode call of this thread ran
    from: re-plans, the first part's size before and now, the replayed ends (us), the measured (start, end) ticks of each video's
    DP workgroup -- int64 [b, 2], 100 MHz, or None -- and the plan's launch order.  Copies: they outlive the plan."""
    import numpy as np
    info = _lib.SmmPlanFeedbackInfo()
    _lib.check(_lib.load().smm_plan_feedback_info(ctypes.byref(info)))
    n = int(info.n_videos)
    stamps = np.ctypeslib.as_array(info.stamps, shape=(n, 2)).astype(np.int64) if n > 0 and info.stamps else None
    order = np.ctypeslib.as_array(info.order, shape=(n,)).copy() if n > 0 and info.order else None
    return {'n_replans': int(info.n_replans), 'n1_before': int(info.n1_before), 'n1_after': int(info.n1_after), 'n_videos': n,
            'end_before_us': float(info.end_before_us), 'end_after_us': float(info.end_after_us), 'stamps': stamps, 'order': order}


def plan_feedback_plan(dur_us, frames, cur_order, cur_n1, n_cu, em_us, force=False):
    """The feedback planner alone, on the host (smmdp.h: smm_plan_feedback_plan) -> (changed, order, n1, replayed end of the
    current plan, of the chosen one; us)."""
    import numpy as np
    dur = np.ascontiguousarray(dur_us, dtype=np.float64)
    fr = np.ascontiguousarray(frames, dtype=np.int32)
    cur = np.ascontiguousarray(cur_order, dtype=np.int32)
    b = len(dur)
    if len(fr) != b or len(cur) != b:
        raise ValueError("dur_us, frames and cur_order must have one entry per video")
    order = np.zeros(b, dtype=np.int32)
    n1 = ctypes.c_int32(0)
    e0, e1 = ctypes.c_double(0.0), ctypes.c_double(0.0)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = _lib.load().smm_plan_feedback_plan(b, int(n_cu), float(em_us), ptr(dur), ptr(fr), ptr(cur), int(cur_n1), 1 if force else 0,
                                            ptr(order), ctypes.cast(ctypes.byref(n1), ctypes.c_void_p),
                                            ctypes.cast(ctypes.byref(e0), ctypes.c_void_p), ctypes.cast(ctypes.byref(e1), ctypes.c_void_p))
    if rc < 0:
        _lib.check(rc)
    return bool(rc), order, int(n1.value), float(e0.value), float(e1.value)


def time_split_plan(batch, n_cu=256):
    """The time-split plan the library would make for this batch's Viterbi launch on a GPU of ``n_cu`` compute units (host logic
    only: include/smmdp.h, smm_time_split_plan) -> list of (video, first position, positions, positions in front of its own part)."""
    import numpy as np
    lib = _lib.load()
    ln, fo, gr, kp, ns = batch.host_ptrs()
    cap = int(batch.total_frames // 128 + 2 * batch.b + 8)
    arrs = [np.zeros(cap, dtype=np.int32) for _ in range(4)]
    n = lib.smm_time_split_plan(ctypes.byref(batch.shape), ctypes.c_void_p(ln), ctypes.c_void_p(gr), ctypes.c_void_p(kp), ctypes.c_void_p(ns),
                                int(n_cu), *[ctypes.c_void_p(a.ctypes.data) for a in arrs], cap)
    if n < 0:
        raise _lib.SmmError("smm_time_split_plan: %s" % lib.smm_strerror(n).decode())
    return [tuple(int(a[i]) for a in arrs) for i in range(min(n, cap))]


def reload_env():
    """Make the library read its SMM_* tuning switches again (it reads them once, at first use)."""
    _lib.reload_env()


def release_cached_plans():
    """smm_release_cached_plans(): frees the library's resident plans, second streams and pooled events; returns the
    device bytes given back.  Only when no call is in flight and no captured graph of a call will be replayed."""
    torch.cuda.synchronize()
    return int(_lib.load().smm_release_cached_plans())


def cached_plan_bytes():
    return int(_lib.load().smm_cached_plan_bytes())
