"""Golden vectors of the feature projection, made by IMPORTING the reference's NICETrans (src/models/flow.py) where the
reference is at hand:

    python tests/golden/make_golden_flow.py --reference <reference>/src

The tests only read the committed ``flow_vectors.npz``.  Per case ``c<i>`` (sizes in ``c<i>/shape`` = D, H, hidden layers,
coupling layers):

* ``c<i>/state/<name>``: the module's state dict, fp32, by the reference's parameter names;
* ``c<i>/x``, ``c<i>/g_y``: an input (|x| <= 10) and an upstream gradient, fp32;
* ``c<i>/y32``, ``c<i>/y64``: the reference's own output in fp32, and with the module cast by ``.double()``;
* ``c<i>/g32/<name>``, ``c<i>/g64/<name>`` (and ``.../x``): torch autograd's gradients of ``(y * g_y).sum()`` with respect
  to every parameter and to the input, in fp32 and in fp64.

The default-shape case stores H = 24 instead of 100: at H = 100 its weights and gradients alone are 1.9 MB.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(2, 1, 0, 1, 9), (6, 5, 0, 3, 9), (34, 17, 2, 2, 9), (200, 24, 1, 4, 40)]      # D, H, hidden, coupling, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help="the reference's src directory")
    ap.add_argument('--out', default=os.path.join(HERE, 'flow_vectors.npz'))
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    sys.path.insert(0, a.reference)
    from models.flow import NICETrans

    out = {}
    for ci, (d, h, hl, cl, rows) in enumerate(CASES):
        torch.manual_seed(1000 + ci)
        args = types.SimpleNamespace(flow_hidden_layers=hl, flow_hidden_units=h, flow_couple_layers=cl, flow_scale=False,
                                     flow_scale_no_zero=False)
        net = NICETrans(args, d)
        # nn.Linear's initialisation leaves a D = 2 flow nearly linear: widen the weights so that the ReLUs switch
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(2.0)
        x = (torch.rand(1, rows, d) * 2 - 1) * 10
        g_y = torch.randn(1, rows, d)
        key = 'c%d/' % ci
        out[key + 'shape'] = np.array([d, h, hl, cl], np.int64)
        out[key + 'x'] = x[0].numpy().copy()
        out[key + 'g_y'] = g_y[0].numpy().copy()
        for name, t in net.state_dict().items():
            out[key + 'state/' + name] = t.numpy().copy()
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            m = NICETrans(args, d).to(dt)
            m.load_state_dict({k: v.to(dt) for k, v in net.state_dict().items()})
            xi = x.to(dt).clone().requires_grad_(True)
            y, log_det = m(xi)
            assert float(log_det.abs().max()) == 0.0
            (y * g_y.to(dt)).sum().backward()
            out[key + 'y' + tag] = y[0].detach().numpy().copy()
            out[key + 'g' + tag + '/x'] = xi.grad[0].numpy().copy()
            for name, p in m.named_parameters():
                out[key + 'g' + tag + '/' + name] = p.grad.numpy().copy()
    np.savez_compressed(a.out, **out)
    print('%s: %d arrays, %d bytes' % (a.out, len(out), os.path.getsize(a.out)))


if __name__ == '__main__':
    main()
