"""Feature projection (--sm_feature_projection), what holds without a GPU: the tests' restatement against the reference's own
numbers, the parameter names, the flag surface, the refusals of the C ABI before a device is touched."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import flow_ref as R
from action_segmentation_amd import _lib, cli, ops
from action_segmentation_amd.flow import FeatureProjector
from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
from module_util import make_args

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
P = ctypes.c_void_p(16)                           # (never dereferenced: the arguments are refused first)
CASES = R.golden_cases()
IDS = ['D%d-H%d-L%d-C%d' % s for s, _ in CASES]


def test_the_golden_cases_are_the_ones_the_kernels_are_checked_on():
    assert [s for s, _ in CASES] == [(2, 1, 0, 1), (6, 5, 0, 3), (34, 17, 2, 2), (200, 24, 1, 4)]
    assert CASES[3][1]['x'].shape == (40, 200)
    for _, f in CASES:
        assert float(np.abs(f['x']).max()) <= 10.0


@pytest.mark.parametrize('shape,f', CASES, ids=IDS)
def test_restatement_reproduces_the_reference_in_fp64(shape, f):
    """tests/flow_ref.py is the oracle of the GPU tests: here it is pinned to the reference's own fp64 outputs and autograd
    gradients (tests/golden/make_golden_flow.py)."""
    d, h, hl, cl = shape
    y, g_x, g_p = R.gradients(torch.from_numpy(f['x']), torch.from_numpy(f['g_y']), R.golden_state(f), hl, cl)
    np.testing.assert_allclose(y.numpy(), f['y64'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(g_x.numpy(), f['g64/x'], rtol=0, atol=1e-12)
    assert set(g_p) == {k[len('g64/'):] for k in f if k.startswith('g64/') and k != 'g64/x'}
    for name, g in g_p.items():
        np.testing.assert_allclose(g.numpy(), f['g64/' + name], rtol=0, atol=1e-12, err_msg=name)


def _flow_module(d, h, hl, cl, k=6, n_classes=3, **kw):
    args = make_args(k, sm_feature_projection=True, flow_hidden_units=h, flow_hidden_layers=hl, flow_couple_layers=cl, **kw)
    return SemiMarkovModule(args, n_classes, d, allow_self_transitions=True)


@pytest.mark.parametrize('shape,f', CASES, ids=IDS)
def test_state_dict_carries_the_reference_names_and_loads_a_reference_checkpoint(shape, f):
    d, h, hl, cl = shape
    m = _flow_module(d, h, hl, cl)
    ref = {'feature_projector.' + k[len('state/'):]: v for k, v in f.items() if k.startswith('state/')}
    mine = {k: v for k, v in m.state_dict().items() if k.startswith('feature_projector.')}
    assert list(mine) == list(ref)                              # (names, and the order the reference registers them in)
    assert {k: tuple(v.shape) for k, v in mine.items()} == {k: v.shape for k, v in ref.items()}
    sd = dict(m.state_dict())
    sd.update({k: torch.from_numpy(v) for k, v in ref.items()})
    m.load_state_dict(sd, strict=True)
    np.testing.assert_array_equal(m.feature_projector.cell0.in_layer.weight.detach().numpy(), f['state/cell0.in_layer.weight'])
    # the packing of the C ABI: per coupling layer, per linear layer, the weight input-major, then the bias
    packed = m.feature_projector.packed()
    assert packed.dtype == torch.float32 and packed.numel() == m.feature_projector.shape.n_params
    np.testing.assert_array_equal(packed[:(d // 2) * h].view(d // 2, h).numpy(), f['state/cell0.in_layer.weight'].T)
    np.testing.assert_array_equal(packed[(d // 2) * h:(d // 2) * h + h].numpy(), f['state/cell0.in_layer.bias'])
    np.testing.assert_array_equal(packed[-(d // 2):].numpy(), f['state/cell%d.out_layer.bias' % (cl - 1)])


def test_packed_parameters_follow_in_place_updates():
    fp = FeatureProjector(6, 5, 1, 2)
    a = fp.packed()
    assert fp.packed() is a
    with torch.no_grad():
        fp.cell1.cell0.bias.add_(1.0)
    b = fp.packed()
    assert b is not a and float((b - a).abs().sum()) == 5.0
    grads = fp.unpack_gradients(torch.arange(fp.shape.n_params, dtype=torch.float64))
    assert [tuple(g.shape) for g in grads] == [tuple(p.shape) for p in fp.packing_order()]
    assert grads[0].dtype == torch.float32 and grads[0][1, 0] == 1.0 and grads[0][0, 1] == 5.0     # input-major -> [out][in]


def test_initialisation_is_nn_linears():
    torch.manual_seed(5)
    fp = FeatureProjector(6, 5, 1, 1)
    torch.manual_seed(5)
    lin = torch.nn.Linear(3, 5)
    assert torch.equal(fp.cell0.in_layer.weight, lin.weight) and torch.equal(fp.cell0.in_layer.bias, lin.bias)


def test_pickle_keeps_the_projector():
    m = _flow_module(6, 5, 1, 2)
    m.feature_projector.packed()
    m2 = pickle.loads(pickle.dumps(m))
    assert list(m2.state_dict()) == list(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(v, m2.state_dict()[k]), k
    assert m2.feature_projector.shape.couple_layers == 2 and '_packed' not in m2.feature_projector.__dict__


def test_a_module_without_the_flag_has_no_projector_and_todays_keys():
    m = SemiMarkovModule(make_args(6), 3, 6, allow_self_transitions=True)
    assert m.feature_projector is None
    assert set(m.state_dict()) == {'poisson_log_rates', 'gaussian_means', 'gaussian_cov', 'transition_logits', 'init_logits'}
    m.set_transition_constraints({0}, {0: {1}}, {1})
    assert set(m.state_dict()) == {'poisson_log_rates', 'gaussian_means', 'gaussian_cov', 'transition_logits', 'init_logits',
                                   'init_constraints', 'transition_constraints'}
    x = torch.zeros(4, 6)
    assert m._project(x) is x


def test_non_projection_parameters_load_into_a_module_with_a_projector():
    plain = SemiMarkovModule(make_args(6), 3, 6, allow_self_transitions=True)
    with torch.no_grad():
        plain.gaussian_means.normal_()
    m = _flow_module(6, 5, 1, 2)
    m.init_nonproject_parameters(plain)
    assert torch.equal(m.gaussian_means, plain.gaussian_means)
    with pytest.raises(AssertionError):
        del plain._parameters['init_logits']
        m.init_nonproject_parameters(plain)


def test_flags_parse_with_the_reference_command_lines():
    import test_cli_flags as T
    for argv in (T.README_S6, T.README_U7, T.DECODE):
        a = cli.build_parser().parse_args(argv + ['--sm_feature_projection', '--flow_couple_layers', '2'])
        assert a.sm_feature_projection and a.flow_couple_layers == 2
        assert a.flow_hidden_units == 100 and a.flow_hidden_layers == 1 and not a.flow_scale and not a.flow_scale_no_zero
    a = cli.build_parser().parse_args(T.README_S6)
    assert not a.sm_feature_projection and a.flow_couple_layers == 4


def test_flow_scale_and_the_closed_form_fit_are_refused():
    with pytest.raises(NotImplementedError, match='flow_scale'):
        _flow_module(6, 5, 1, 2, flow_scale=True)
    with pytest.raises(ValueError, match='even'):
        _flow_module(7, 5, 1, 2)
    m = _flow_module(6, 5, 1, 2)
    with pytest.raises(NotImplementedError, match='feature projector'):
        m.fit_supervised([torch.zeros(4, 6)], [torch.zeros(4, dtype=torch.long)])


def test_a_module_on_the_host_has_no_cpu_path():
    m = _flow_module(6, 5, 1, 2)
    x, lengths = torch.randn(2, 5, 6), torch.tensor([5, 4])
    with pytest.raises(_lib.SmmError):
        m.viterbi(x, lengths, None)
    with pytest.raises(_lib.SmmError):
        m.log_likelihood(x, lengths, None)
    with pytest.raises(_lib.SmmError):
        m.feature_projector(x)
    with pytest.raises(_lib.SmmError):
        ops.flow(x[0], m.feature_projector.packed(), m.feature_projector.shape)
    with pytest.raises(_lib.SmmError):
        ops.flow_bwd(x[0], x[0], m.feature_projector.packed(), m.feature_projector.shape)


# ------------------------------------------------------------------------------------------------ C ABI
def _shape(**kw):
    s = dict(n_rows=40, d=200, hidden_units=100, hidden_layers=1, couple_layers=4)
    s.update(kw)
    return _lib.SmmFlowShape(s['n_rows'], s['d'], s['hidden_units'], s['hidden_layers'], s['couple_layers'])


def _fwd(shape, x=P, params=P, y=P):
    return _lib.load().smm_flow_f32(None if shape is None else ctypes.byref(shape), x, params, y, None, 0, None)


def _bwd(shape, x=P, g_y=P, params=P, g_params=P, g_x=None, scratch=P, scratch_bytes=1 << 40):
    return _lib.load().smm_flow_bwd_f32(None if shape is None else ctypes.byref(shape), x, g_y, params, g_params, g_x, scratch,
                                        ctypes.c_size_t(scratch_bytes), None)


BAD_SHAPES = [(dict(d=201), ARG), (dict(d=3), ARG), (dict(n_rows=0), ARG), (dict(d=0), UNSUPPORTED), (dict(d=514), UNSUPPORTED),
              (dict(hidden_units=0), UNSUPPORTED), (dict(hidden_units=257), UNSUPPORTED), (dict(hidden_layers=-1), UNSUPPORTED),
              (dict(hidden_layers=5), UNSUPPORTED), (dict(couple_layers=0), UNSUPPORTED), (dict(couple_layers=17), UNSUPPORTED)]


@pytest.mark.parametrize('fault,status', BAD_SHAPES, ids=['-'.join('%s=%d' % kv for kv in f.items()) for f, _ in BAD_SHAPES])
def test_flow_refuses_sizes_outside_the_supported_ones(fault, status):
    lib = _lib.load()
    s = _shape(**fault)
    assert _fwd(s) == status and _bwd(s) == status
    assert lib.smm_flow_bwd_scratch_bytes(ctypes.byref(s)) == 0
    assert lib.smm_strerror(status) not in (b'ok', b'unknown smm_status')


def test_flow_refuses_null_pointers_and_a_short_scratch():
    lib = _lib.load()
    s = _shape()
    assert _fwd(None) == ARG and _bwd(None) == ARG
    for slot in ('x', 'params', 'y'):
        assert _fwd(s, **{slot: None}) == ARG, slot
    for slot in ('x', 'g_y', 'params', 'g_params', 'scratch'):
        assert _bwd(s, **{slot: None}) == ARG, slot
    need = lib.smm_flow_bwd_scratch_bytes(ctypes.byref(s))
    assert need > 0 and need % (8 * ops.FlowShape(200).n_params) == 0       # fp64 partials of every parameter, per workgroup
    assert _bwd(s, scratch_bytes=need - 1) == WORKSPACE
    assert lib.smm_flow_scratch_bytes(ctypes.byref(s)) == 0


def test_the_input_halves_go_to_the_scratch_only_where_lds_has_no_room():
    lib = _lib.load()
    for (d, h, hl, cl), in_scratch in (((200, 100, 1, 4), False), ((512, 256, 2, 2), False), ((512, 256, 2, 3), True),
                                       ((512, 100, 1, 4), False), ((512, 100, 1, 6), True), ((512, 256, 4, 1), True)):
        need = lib.smm_flow_bwd_scratch_bytes(ctypes.byref(_shape(d=d, hidden_units=h, hidden_layers=hl, couple_layers=cl, n_rows=70)))
        assert (need % (8 * ops.FlowShape(d, h, hl, cl).n_params) != 0) == in_scratch, (d, h, hl, cl)


@pytest.mark.parametrize('d,h,hl,cl', [(2, 1, 0, 1), (512, 256, 4, 16), (512, 256, 2, 4), (200, 100, 1, 4), (300, 17, 3, 2)])
def test_every_supported_size_has_a_backward_plan(d, h, hl, cl):
    """The backward tile (two row tiles, every activation of one MLP, a weight slab) fits the LDS at every supported size."""
    s = _shape(d=d, hidden_units=h, hidden_layers=hl, couple_layers=cl, n_rows=5000)
    need = _lib.load().smm_flow_bwd_scratch_bytes(ctypes.byref(s))
    # the fp64 partials (at most 256 MB, one workgroup's at the least) and, where LDS has no room, the kept halves of the tiles in
    # flight (couple_layers x 64 rows x d / 2 floats per workgroup at the most, 256 workgroups)
    assert 0 < need <= (256 << 20) + 8 * ops.FlowShape(d, h, hl, cl).n_params + 256 * cl * 64 * (d // 2) * 4


def test_emission_bwd_x_refusals():
    import test_api_refusals_host as T
    T.SIGNATURES['smm_emission_bwd_x_f64'] = ('meta4', 'x', 'g_elp', 'w', 'inv_var', 'g_x') + T._WS
    try:
        for slot in ('x', 'g_elp', 'w', 'inv_var', 'g_x', 'lengths', 'frame_off', 'n_states', 'ws'):
            assert T.call('smm_emission_bwd_x_f64', **{slot: None}) == ARG, slot
        for fault in (None, dict(d=0), dict(b=0), dict(k_rows=1)):
            assert T.call('smm_emission_bwd_x_f64', shape=fault) == ARG, fault
    finally:
        del T.SIGNATURES['smm_emission_bwd_x_f64']


def test_the_new_symbols_are_declared_listed_and_exported():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'smmdp.h')).read()
    declared = set(re.findall(r'\b(smm_[a-z0-9_]+)\s*\(', header))
    lib = _lib.load()
    for name in ('smm_flow_f32', 'smm_flow_bwd_f32', 'smm_emission_bwd_x_f64', 'smm_flow_scratch_bytes', 'smm_flow_bwd_scratch_bytes'):
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
