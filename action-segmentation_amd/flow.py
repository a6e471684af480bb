"""Feature projection of --sm_feature_projection: the NICE additive coupling flow (reference src/models/flow.py, NICETrans
without --flow_scale) in front of the emission scorer, on the GPU.

``FeatureProjector`` holds the parameters under the reference's names and shapes, so state dicts travel both ways; its forward
is ``smm_flow_f32`` and its backward ``smm_flow_bwd_f32`` (csrc/smm_flow.hip) on the parameters packed into the ABI's one
buffer.  There is no CPU path: a module on the host raises SmmError like every other device entry point.
"""
import torch
import torch.nn as nn

from . import ops


class _ReLUNet(nn.Module):
    """The MLP of one coupling layer, by the reference's names: in_layer, cell0 .. cell{hidden_layers-1}, out_layer."""

    def __init__(self, in_features, hidden_units, hidden_layers, out_features):
        super().__init__()
        self.in_layer = nn.Linear(in_features, hidden_units, bias=True)
        self.out_layer = nn.Linear(hidden_units, out_features, bias=True)
        for i in range(hidden_layers):
            setattr(self, 'cell%d' % i, nn.Linear(hidden_units, hidden_units, bias=True))
        self.hidden_layers = hidden_layers

    def linears(self):
        return [self.in_layer] + [getattr(self, 'cell%d' % i) for i in range(self.hidden_layers)] + [self.out_layer]


class _Flow(torch.autograd.Function):
    """y = flow(x) row by row as a function of x and of the flow's parameters (weight, bias of every linear layer in packing
    order).  Nothing but x is kept for the backward: smm_flow_bwd_f32 computes the activations again."""

    @staticmethod
    def forward(ctx, projector, x, *params):
        ctx.projector = projector
        ctx.packed = projector.packed()
        ctx.save_for_backward(x)
        return ops.flow(x, ctx.packed, projector.shape)

    @staticmethod
    def backward(ctx, g_y):
        x, = ctx.saved_tensors
        p = ctx.projector
        g_packed, g_x = ops.flow_bwd(x, g_y.to(torch.float32).contiguous(), ctx.packed, p.shape, want_g_x=ctx.needs_input_grad[1])
        return (None, g_x) + tuple(p.unpack_gradients(g_packed))


class FeatureProjector(nn.Module):
    """``couple_layers`` additive coupling layers over rows of ``features`` (even) entries: layer i copies one half of the row
    (the first for even i, the second for odd i) and adds a ReLU MLP of that half to the other.  log det = 0."""

    def __init__(self, features, hidden_units=100, hidden_layers=1, couple_layers=4):
        super().__init__()
        if features < 2 or features % 2:
            raise ValueError("--sm_feature_projection needs an even feature dimension, got %d" % features)
        self.shape = ops.FlowShape(features, hidden_units, hidden_layers, couple_layers)
        for i in range(couple_layers):
            setattr(self, 'cell%d' % i, _ReLUNet(features // 2, hidden_units, hidden_layers, features // 2))

    @classmethod
    def from_args(cls, args, features):
        return cls(features, getattr(args, 'flow_hidden_units', 100), getattr(args, 'flow_hidden_layers', 1),
                   getattr(args, 'flow_couple_layers', 4))

    def linears(self):
        return [lin for i in range(self.shape.couple_layers) for lin in getattr(self, 'cell%d' % i).linears()]

    def packing_order(self):
        """The parameters in the ABI buffer's order: weight, bias of every linear layer."""
        return [p for lin in self.linears() for p in (lin.weight, lin.bias)]

    def version_key(self):
        """Identity + version of every parameter: any in-place update changes it."""
        return tuple((p.data_ptr(), p._version) for p in self.packing_order())

    def packed(self):
        """The parameters as smm_flow_f32 takes them (include/smmdp.h: weights input-major), rebuilt when one has changed."""
        key = self.version_key()
        cached = self.__dict__.get('_packed')
        if cached is None or cached[0] != key:
            with torch.no_grad():
                flat = torch.cat([(p.t() if p.dim() == 2 else p).to(torch.float32).reshape(-1) for p in self.packing_order()])
            cached = self.__dict__['_packed'] = (key, flat.contiguous())
        return cached[1]

    def unpack_gradients(self, g_packed):
        """smm_flow_bwd_f32's fp64 gradients in packing order, in the parameters' shapes and dtypes."""
        out, o = [], 0
        for p in self.packing_order():
            n = p.numel()
            g = g_packed[o:o + n]
            out.append((g.view(p.size(1), p.size(0)).t() if p.dim() == 2 else g).to(p.dtype))
            o += n
        return out

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop('_packed', None)               # a device tensor derived from the parameters: rebuilt on demand
        return state

    def forward(self, x):
        """x fp32 [..., features] on the device -> the projected features, same shape; (y, log det = 0 per leading row) is what
        the reference's NICETrans returns -- the zero is the caller's to add."""
        flat = x.to(torch.float32).contiguous().view(-1, self.shape.d)
        return _Flow.apply(self, flat, *self.packing_order()).view(x.shape)
