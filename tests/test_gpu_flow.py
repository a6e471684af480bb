"""The feature projection's kernels on the GPU (csrc/smm_flow.hip): smm_flow_f32, smm_flow_bwd_f32 and smm_emission_bwd_x_f64
against the reference's stored numbers (tests/golden/flow_vectors.npz) and against the tests' fp64 restatement of the flow
(tests/flow_ref.py, pinned to the reference by tests/test_flow_host.py).

Tolerances.  Forward: per case, 4 x the largest absolute difference between the REFERENCE's own fp32 and fp64 outputs (stored
for the golden cases; for the others measured here with the restatement in fp32 on the CPU).  Both the reference's fp32 run and
the kernel are fp32 chains with different summation orders (BLAS against the MFMA's k-ordered fma chain), so neither one's
error bounds the other's; a factor of 4 over one of them leaves room for that without hiding a wrong tile.  Backward: the same
with the fp32-against-fp64 autograd discrepancy, every tensor relative to its own max |ref|, the case's largest, times 4.
"""
import numpy as np
import pytest
import torch

import flow_ref as R
from action_segmentation_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TILES = (16, 32, 64)                      # rows per workgroup tile, by what fits the LDS (csrc/smm_flow.hip: smm_flow_plan)
GOLDEN = R.golden_cases()
GOLDEN_IDS = ['D%d-H%d-L%d-C%d' % s for s, _ in GOLDEN]
# every (D, H) of {2, 6, 34, 200, 300, 512} x {1, 17, 100, 256}, with 0..2 hidden and 1..4 coupling layers dealt over them
SWEEP = [(d, h, i % 3, 1 + (i + i // 4) % 4) for i, (d, h) in enumerate((d, h) for d in (2, 6, 34, 200, 300, 512)
                                                                         for h in (1, 17, 100, 256))]
SWEEP_ROWS = 70                           # 64 + 6, 2 x 32 + 6, 4 x 16 + 6: the last tile nearly empty at every tile size


def _pack(state, shape):
    """The ABI's buffer from a state dict by the reference's names (the module's packing, restated)."""
    parts = []
    for i in range(shape.couple_layers):
        for name in ['in_layer'] + ['cell%d' % j for j in range(shape.hidden_layers)] + ['out_layer']:
            parts += [state['cell%d.%s.weight' % (i, name)].t().reshape(-1), state['cell%d.%s.bias' % (i, name)]]
    return torch.cat(parts).to(device=DEV, dtype=torch.float32).contiguous()


def _unpack(g_packed, state, shape):
    out, o = {}, 0
    for i in range(shape.couple_layers):
        for name in ['in_layer'] + ['cell%d' % j for j in range(shape.hidden_layers)] + ['out_layer']:
            w = state['cell%d.%s.weight' % (i, name)]
            out['cell%d.%s.weight' % (i, name)] = g_packed[o:o + w.numel()].view(w.size(1), w.size(0)).t().cpu()
            o += w.numel()
            out['cell%d.%s.bias' % (i, name)] = g_packed[o:o + w.size(0)].cpu()
            o += w.size(0)
    assert o == g_packed.numel()
    return out


def _case(d, h, hl, cl, rows, seed):
    g = torch.Generator().manual_seed(seed)
    state = R.random_state(d, h, hl, cl, seed, dtype=torch.float32)
    x = ((torch.rand(rows, d, generator=g) * 2 - 1) * 10).float()
    g_y = torch.randn(rows, d, generator=g).float()
    return state, x, g_y


def _relative(got, ref):
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.double().abs().max()), 1e-300)


def _check_backward(g_packed, g_x, state, shape, ref_gx, ref_gp, own_gx, own_gp, what):
    """Entry by entry, relative to each tensor's max |ref|, against 4 x the fp32 autograd's own largest such discrepancy."""
    got = _unpack(g_packed, state, shape)
    bar = 4 * max([_relative(own_gx, ref_gx)] + [_relative(own_gp[k], ref_gp[k]) for k in ref_gp])
    worst = max([(_relative(g_x.cpu(), ref_gx), 'x')] + [(_relative(got[k], ref_gp[k]), k) for k in ref_gp])
    print('%s: backward worst %.3g (%s), bar %.3g, ratio %.2f' % (what, worst[0], worst[1], bar, worst[0] / max(bar, 1e-300)))
    assert worst[0] <= bar, (what, worst, bar)


# ------------------------------------------------------------------------------------------------ forward, exact properties
def test_zeroed_out_layers_give_the_identity_bit_for_bit():
    shape = ops.FlowShape(34, 17, 2, 3)
    state, x, _ = _case(34, 17, 2, 3, 77, 1)
    for k in state:
        if '.out_layer.' in k:
            state[k].zero_()
    y = ops.flow(x.to(DEV), _pack(state, shape), shape)
    assert torch.equal(y.cpu().view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize('d,h,hl,cl', [(200, 100, 1, 4), (512, 256, 2, 3), (6, 5, 0, 2)])
def test_a_row_gives_the_same_bits_wherever_it_sits(d, h, hl, cl):
    shape = ops.FlowShape(d, h, hl, cl)
    state, x, _ = _case(d, h, hl, cl, 3 * 64 + 7, 2)
    packed = _pack(state, shape)
    row = x[5].clone()
    alone = ops.flow(row.view(1, d).to(DEV), packed, shape).cpu()[0]
    places = sorted({0} | {t - 1 for t in TILES} | set(TILES) | {x.size(0) - 1})
    for at in places:
        xs = x.clone()
        xs[at] = row
        y = ops.flow(xs.to(DEV), packed, shape).cpu()
        assert torch.equal(y[at].view(torch.int32), alone.view(torch.int32)), at
    # permuting the rows permutes the output; two runs give the same bits
    perm = torch.randperm(x.size(0), generator=torch.Generator().manual_seed(3))
    y0 = ops.flow(x.to(DEV), packed, shape)
    y1 = ops.flow(x[perm].to(DEV), packed, shape)
    assert torch.equal(y1.view(torch.int32), y0[perm.to(DEV)].view(torch.int32))
    assert torch.equal(ops.flow(x.to(DEV), packed, shape).view(torch.int32), y0.view(torch.int32))


@pytest.mark.parametrize('rows', sorted({1, 3 * 64 + 7} | {t + o for t in TILES for o in (-1, 0, 1)}))
def test_row_counts_around_the_tile(rows):
    shape = ops.FlowShape(34, 17, 1, 2)
    state, x, _ = _case(34, 17, 1, 2, 3 * 64 + 7, 4)
    packed = _pack(state, shape)
    whole = ops.flow(x.to(DEV), packed, shape)
    y = ops.flow(x[:rows].contiguous().to(DEV), packed, shape)
    assert y.shape == (rows, 34)
    assert torch.equal(y.view(torch.int32), whole[:rows].view(torch.int32))
    ref = R.flow(x[:rows].double(), {k: v.double() for k, v in state.items()}, 1, 2)
    own = R.flow(x[:rows], state, 1, 2)
    assert float((y.cpu().double() - ref).abs().max()) <= 4 * float((own.double() - ref).abs().max())


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize('shp,f', GOLDEN, ids=GOLDEN_IDS)
def test_golden_cases_forward_and_backward(shp, f):
    d, h, hl, cl = shp
    shape = ops.FlowShape(d, h, hl, cl)
    state = R.golden_state(f, dtype=torch.float32)
    packed = _pack(state, shape)
    x, g_y = torch.from_numpy(f['x']).to(DEV), torch.from_numpy(f['g_y']).to(DEV)
    y = ops.flow(x, packed, shape).cpu()
    bar = 4 * float(np.abs(f['y32'].astype(np.float64) - f['y64']).max())
    err = float((y.double() - torch.from_numpy(f['y64'])).abs().max())
    print('golden %s: forward error %.3g, bar %.3g, ratio %.2f' % (shp, err, bar, err / bar))
    assert err <= bar
    if cl == 1:
        assert torch.equal(y[:, :d // 2].view(torch.int32), x.cpu()[:, :d // 2].view(torch.int32))
    g_packed, g_x = ops.flow_bwd(x, g_y, packed, shape, want_g_x=True)
    names = [k[len('g64/'):] for k in f if k.startswith('g64/') and k != 'g64/x']
    _check_backward(g_packed, g_x, state, shape, torch.from_numpy(f['g64/x']), {k: torch.from_numpy(f['g64/' + k]) for k in names},
                    torch.from_numpy(f['g32/x']), {k: torch.from_numpy(f['g32/' + k]) for k in names}, 'golden %s' % (shp,))
    again, g_x2 = ops.flow_bwd(x, g_y, packed, shape, want_g_x=True)
    assert torch.equal(again.view(torch.int64), g_packed.view(torch.int64)) and torch.equal(g_x2.view(torch.int32), g_x.view(torch.int32))
    only, none = ops.flow_bwd(x, g_y, packed, shape)
    assert none is None and torch.equal(only.view(torch.int64), g_packed.view(torch.int64))


def _forward_and_backward_against_the_restatement(d, h, hl, cl, rows):
    shape = ops.FlowShape(d, h, hl, cl)
    state, x, g_y = _case(d, h, hl, cl, rows, 100 + d + h)
    packed = _pack(state, shape)
    ref_y, ref_gx, ref_gp = R.gradients(x, g_y, state, hl, cl)
    own_y, own_gx, own_gp = R.gradients(x, g_y, state, hl, cl, dtype=torch.float32)
    y = ops.flow(x.to(DEV), packed, shape).cpu()
    bar = 4 * float((own_y.double() - ref_y).abs().max())
    err = float((y.double() - ref_y).abs().max())
    print('sweep %s: forward error %.3g, bar %.3g, ratio %.2f' % ((d, h, hl, cl), err, bar, err / max(bar, 1e-300)))
    assert err <= bar
    if cl == 1:        # one coupling layer leaves the first half untouched
        assert torch.equal(y[:, :d // 2].view(torch.int32), x[:, :d // 2].view(torch.int32))
    g_packed, g_x = ops.flow_bwd(x.to(DEV), g_y.to(DEV), packed, shape, want_g_x=True)
    _check_backward(g_packed, g_x, state, shape, ref_gx, ref_gp, own_gx, own_gp, 'sweep %s' % ((d, h, hl, cl),))
    again, g_x2 = ops.flow_bwd(x.to(DEV), g_y.to(DEV), packed, shape, want_g_x=True)
    assert torch.equal(again.view(torch.int64), g_packed.view(torch.int64)) and torch.equal(g_x2.view(torch.int32), g_x.view(torch.int32))


@pytest.mark.parametrize('d,h,hl,cl', SWEEP, ids=['D%d-H%d-L%d-C%d' % s for s in SWEEP])
def test_sweep_forward_and_backward_against_the_restatement(d, h, hl, cl):
    _forward_and_backward_against_the_restatement(d, h, hl, cl, SWEEP_ROWS)


# the sizes whose backward tile leaves no room in LDS for the coupling layers' input halves: they are kept in the workgroup's
# slice of the scratch (smm_flow_plan); the last one with more tiles (50) than workgroups (the 256 MB of partials allow 42), so
# that a slice is used again
SCRATCH_KEPT = [(512, 256, 2, 3, SWEEP_ROWS), (512, 256, 2, 4, SWEEP_ROWS), (512, 100, 1, 6, SWEEP_ROWS), (512, 256, 3, 2, 33),
                (512, 256, 4, 2, 16 * 50)]


@pytest.mark.parametrize('d,h,hl,cl,rows', SCRATCH_KEPT, ids=['D%d-H%d-L%d-C%d-%drows' % s for s in SCRATCH_KEPT])
def test_forward_and_backward_where_the_input_halves_are_kept_in_scratch(d, h, hl, cl, rows):
    import ctypes
    from action_segmentation_amd import _lib
    need = _lib.load().smm_flow_bwd_scratch_bytes(ctypes.byref(ops.FlowShape(d, h, hl, cl).c_shape(rows)))
    assert need % (8 * ops.FlowShape(d, h, hl, cl).n_params) != 0           # (more than whole fp64 partials: the halves)
    _forward_and_backward_against_the_restatement(d, h, hl, cl, rows)


def test_default_shape_backward_over_many_tiles():
    """D = 200, H = 100 (the golden stores H = 24): 5000 rows, so every workgroup of the backward grid sums several tiles."""
    d, h, hl, cl = 200, 100, 1, 4
    shape = ops.FlowShape(d, h, hl, cl)
    state, x, g_y = _case(d, h, hl, cl, 5000 - 9, 7)
    packed = _pack(state, shape)
    ref_y, ref_gx, ref_gp = R.gradients(x, g_y, state, hl, cl)
    own_y, own_gx, own_gp = R.gradients(x, g_y, state, hl, cl, dtype=torch.float32)
    g_packed, g_x = ops.flow_bwd(x.to(DEV), g_y.to(DEV), packed, shape, want_g_x=True)
    _check_backward(g_packed, g_x, state, shape, ref_gx, ref_gp, own_gx, own_gp, 'default shape, 4991 rows')
    again, _ = ops.flow_bwd(x.to(DEV), g_y.to(DEV), packed, shape)
    assert torch.equal(again.view(torch.int64), g_packed.view(torch.int64))


# ------------------------------------------------------------------------------------------------ d elp / d x
def _emission_case(n_states, lengths, frame_offset, total, d, seed, with_cons):
    g = torch.Generator().manual_seed(seed)
    cm, groups = max(n_states), len(n_states)
    group = [i % groups for i in range(len(lengths))]
    batch = ops.Batch(lengths, n_states, 8, c_max=cm, frame_offset=frame_offset, group=group, d=d, t_max=max(lengths),
                      total_frames=total)
    x = torch.randn(total, d, generator=g)
    w = torch.randn(groups, d, cm, generator=g, dtype=torch.float64)
    inv_var = torch.rand(d, generator=g, dtype=torch.float64) + 0.5
    cst = torch.randn(groups, cm, generator=g, dtype=torch.float64)
    for gi, c in enumerate(n_states):
        w[gi, :, c:] = 0
        cst[gi, c:] = 0
    g_elp = torch.randn(total, cm, generator=g, dtype=torch.float64)
    cons = torch.randn(total, cm, generator=g) if with_cons else None
    return batch, group, x, w, cst, inv_var, g_elp, cons


@pytest.mark.parametrize('n_states,d', [([5], 34), ([3, 17, 32], 200), ([9, 24, 2], 300)])
@pytest.mark.parametrize('with_cons', [False, True])
def test_emission_bwd_x_against_the_formula(n_states, d, with_cons):
    """g_x = g_elp . w^T - x * inv_var * rowsum(g_elp) in torch fp64 (the constraints are added to elp and do not depend on x:
    with them the same gradient, from torch autograd on the scorer's formula)."""
    lengths = [300, 7, 257, 64, 1, 90]
    offs, o = [], 3                                       # ragged, with rows no video covers in front, between and behind
    for t in lengths:
        offs.append(o)
        o += t + (5 if t % 2 else 0)
    total = o + 4
    batch, group, x, w, cst, inv_var, g_elp, cons = _emission_case(n_states, lengths, offs, total, d, 11, with_cons)
    got = ops.emission_bwd_x(batch, x.to(DEV), g_elp.to(DEV), w.to(DEV), inv_var.to(DEV))
    assert got.dtype == torch.float32 and got.shape == (total, d)
    ref = torch.zeros(total, d, dtype=torch.float64)
    for i, (t, o) in enumerate(zip(lengths, offs)):
        gi, c = group[i], n_states[group[i]]
        xi = x[o:o + t].double().requires_grad_(True)
        elp = cst[gi, :c] + xi @ w[gi, :, :c] - 0.5 * (xi * xi) @ inv_var.unsqueeze(1)
        if cons is not None:
            elp = elp + cons[o:o + t, :c].double()
        (elp * g_elp[o:o + t, :c]).sum().backward()
        ref[o:o + t] = xi.grad
    covered = torch.zeros(total, dtype=torch.bool)
    for t, o in zip(lengths, offs):
        covered[o:o + t] = True
    assert float(got.cpu()[~covered].abs().max()) == 0.0 and (~covered).sum() > 0
    err = float((got.cpu().double() - ref).abs().max())
    assert err <= 1e-6 * float(ref.abs().max()), err
    assert torch.equal(ops.emission_bwd_x(batch, x.to(DEV), g_elp.to(DEV), w.to(DEV), inv_var.to(DEV)).view(torch.int32),
                       got.view(torch.int32))
