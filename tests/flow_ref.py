"""The NICE additive coupling flow restated in plain torch for the tests: the oracle of the GPU tests, pinned to the reference
itself by tests/test_flow_host.py (it reproduces the golden fp64 outputs and gradients to 1e-12).

``state``: {name: tensor} by the reference's parameter names (``cell{i}.in_layer.weight`` ...), any dtype and device; the
computation follows the dtype of ``x``'s and the parameters' (give both fp64 for the oracle, both fp32 for the size of fp32's
own error).  Differentiable: give tensors that require grad.
"""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'flow_vectors.npz')


def mlp(state, i, hidden_layers, h):
    pre = 'cell%d.' % i
    h = torch.relu(h @ state[pre + 'in_layer.weight'].t() + state[pre + 'in_layer.bias'])
    for j in range(hidden_layers):
        h = torch.relu(h @ state[pre + 'cell%d.weight' % j].t() + state[pre + 'cell%d.bias' % j])
    return h @ state[pre + 'out_layer.weight'].t() + state[pre + 'out_layer.bias']


def flow(x, state, hidden_layers, couple_layers):
    """y = flow(x) over the last dimension of x."""
    dh = x.size(-1) // 2
    a, b = x[..., :dh], x[..., dh:]
    for i in range(couple_layers):
        if i % 2 == 0:
            b = b + mlp(state, i, hidden_layers, a)
        else:
            a = a + mlp(state, i, hidden_layers, b)
    return torch.cat([a, b], dim=-1)


def random_state(d, h, hidden_layers, couple_layers, seed, scale=2.0, dtype=torch.float64):
    """nn.Linear-like uniform parameters (widened by ``scale`` so that the ReLUs switch), by the reference's names."""
    g = torch.Generator().manual_seed(seed)
    dh = d // 2
    state = {}
    for i in range(couple_layers):
        sizes = [('in_layer', dh, h)] + [('cell%d' % j, h, h) for j in range(hidden_layers)] + [('out_layer', h, dh)]
        for name, fin, fout in sizes:
            bound = scale / np.sqrt(fin)
            state['cell%d.%s.weight' % (i, name)] = ((torch.rand(fout, fin, generator=g, dtype=torch.float64) * 2 - 1) * bound).to(dtype)
            state['cell%d.%s.bias' % (i, name)] = ((torch.rand(fout, generator=g, dtype=torch.float64) * 2 - 1) * bound).to(dtype)
    return state


def gradients(x, g_y, state, hidden_layers, couple_layers, dtype=torch.float64):
    """(y, g_x, {name: gradient}) of (flow(x) * g_y).sum() by torch autograd, computed in ``dtype`` on the CPU."""
    st = {k: v.detach().to(device='cpu', dtype=dtype).requires_grad_(True) for k, v in state.items()}
    xi = x.detach().to(device='cpu', dtype=dtype).requires_grad_(True)
    y = flow(xi, st, hidden_layers, couple_layers)
    (y * g_y.detach().to(device='cpu', dtype=dtype)).sum().backward()
    return y.detach(), xi.grad, {k: v.grad for k, v in st.items()}


def golden_cases():
    """[(shape (D, H, hidden, coupling), {field: array})] of tests/golden/flow_vectors.npz."""
    z = np.load(GOLDEN)
    cases = {}
    for key in z.files:
        c, field = key.split('/', 1)
        cases.setdefault(c, {})[field] = z[key]
    return [(tuple(int(v) for v in cases[c]['shape']), cases[c]) for c in sorted(cases)]


def golden_state(fields, prefix='state/', dtype=torch.float64):
    return {k[len(prefix):]: torch.from_numpy(v).to(dtype) for k, v in fields.items() if k.startswith(prefix)}
