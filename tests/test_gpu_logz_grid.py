"""smm_logz_kernel and its backward across their work splits, on lattices whose posterior lives on LONG segments.

The chain wave of smm_logz_kernel evaluates the K0 = 2B shortest segment lengths; every longer one sits in the pusher waves'
fp32 (M, S, L) ring slots -- slot rotation, the ref / lmx rescaling, the hand-over of A' through LDS, the wrap at 64 R slots --
and, backward, in smm_glen_kernel's tiles.  The i.i.d. normal lattices of test_gpu_viterbi.make_problem never use such a length
(tests/test_logz_cases_host.py asserts that), so here every case brings a planted segmentation (tests/logz_cases.py): the same
host test proves from the C twin alone that at least 0.3 of the expected segments are ring lengths, that every state's ring
carries mass, the longest slot too, and that log Z moves by more than a nat per video when the ring is dead.

Forward log Z and the four gradients go through ops.logz / ops.logz_bwd, in both launch forms (the reversed recursion as its
own launch; both directions in one launch), against oracle.factored.logz(grad=True, upstream=...), computed once per case.
Bars are the project's: log Z rtol 1e-6 / atol 1e-4 (test_log_partition_matches_oracle), gradients rtol = atol = 2e-5
(test_log_partition_gradients_match_oracle); the two launch forms against each other as in
test_logz_both_directions_in_one_launch.  Every test prints its measured worst errors as one JSON line (pytest -rP)."""
import json

import numpy as np
import pytest
import torch

import logz_cases as L
from oracle import factored as F
from test_gpu_viterbi import masked_problem

pytestmark = pytest.mark.gpu

Z_BAR = dict(rtol=1e-6, atol=1e-4)
G_BAR = dict(rtol=2e-5, atol=2e-5)
KEYS = ('elp', 'trans', 'init', 'len')


def _ops():
    from action_segmentation_amd import ops
    return ops


def _launch(batch, elp, trans, init, lens, endpen, up):
    """log Z and gradients in both launch forms -> [(z, grads as numpy), (z, grads)]; the forms agree to the order of their
    atomic sums."""
    ops = _ops()
    dev = torch.device('cuda:0')
    t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    args = (t(elp), t(trans), t(init), t(lens))
    ep, upt = t(endpen), t(up)
    res = []
    for both in (False, True):
        ws = torch.empty(batch.workspace_bytes(), dtype=torch.uint8, device=dev)
        z = ops.logz(batch, *args, endpen=ep, ws=ws, with_backward=both)
        g = ops.logz_bwd(batch, *args, z, grad_logz=upt, endpen=ep, ws=ws, with_backward=both)
        torch.cuda.synchronize()
        res.append((z.cpu().numpy(), {k: v.cpu().numpy() for k, v in g.items()}))
    np.testing.assert_array_equal(res[0][0], res[1][0])
    for k in KEYS:
        np.testing.assert_allclose(res[1][1][k], res[0][1][k], rtol=1e-12, atol=1e-15, err_msg=k)
    return res


def _err(got, ref):
    """max |got - ref| / max(1, |ref|): the figure of test_logz_gradient_error_does_not_grow_with_the_lattice."""
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


@pytest.mark.parametrize('name', L.CASE_NAMES)
def test_planted_lattices_match_the_twin(name):
    """Every (R, SPW, HF) instantiation of smm_logz_kernel, the ring-size boundaries, block tails (four videos, every residue of
    T mod 4, two shorter than the span limit, one to three positions), the three closings, the backward's tiles."""
    ops = _ops()
    p = L.planted(name)
    b, tmax, c = p['elp'].shape
    kp, up = p['k'], L.upstream(name)
    ref_z, ref = L.reference(name)
    batch = ops.Batch(p['lengths'], [c], kp, c_max=c, t_max=tmax, total_frames=b * tmax, no_eos=p['no_eos'])
    res = _launch(batch, p['elp'].reshape(b * tmax, c), p['trans'][None], p['init'][None], p['lens'][None], p['endpen'], up)
    worst = dict(case=name, R=L.ring_regs(kp), logz=0.0, **{k: 0.0 for k in KEYS})
    for z, g in res:
        ge = g['elp'].reshape(b, tmax, c)
        got = dict(elp=np.concatenate([ge[i, :t].ravel() for i, t in enumerate(p['lengths'])]), trans=g['trans'][0],
                   init=g['init'][0], len=g['len'][0])
        want = dict(elp=np.concatenate([ref['elp'][i, :t].ravel() for i, t in enumerate(p['lengths'])]), trans=ref['trans'],
                    init=ref['init'], len=ref['len'])
        worst['logz'] = max(worst['logz'], _err(z, ref_z))
        for k in KEYS:
            worst[k] = max(worst[k], _err(got[k], want[k]))
    print(json.dumps(worst))
    for z, g in res:
        np.testing.assert_allclose(z, ref_z, **Z_BAR)
        ge = g['elp'].reshape(b, tmax, c)
        for i, t in enumerate(p['lengths']):
            np.testing.assert_allclose(ge[i, :t], ref['elp'][i, :t], **G_BAR, err_msg='video %d' % i)
            assert np.all(ge[i, t:] == 0)                           # rows past a video's end: exactly 0
        assert g['len'].shape == (1, kp, c)
        np.testing.assert_allclose(g['trans'][0], ref['trans'], **G_BAR)
        np.testing.assert_allclose(g['init'][0], ref['init'], **G_BAR)
        np.testing.assert_allclose(g['len'][0], ref['len'], **G_BAR)


@pytest.mark.parametrize('name', L.MIXED_NAMES)
def test_mixed_launches_match_the_twin(name):
    """Two parameter groups in one launch: the larger picks the kernel, the smaller rides in it (3 states beside 32, 16 beside
    17, 9 beside 23, 7 beside 8); padded columns full of noise, packed frame offsets, kp per video with one video at
    kp <= K0 + 1 beside kp_max.  Reference: one twin call per (group, kp); table gradients per group."""
    ops = _ops()
    m = L.mixed(name)
    ref_z, ref, live = L.mixed_reference(name)
    batch = ops.Batch(m['lengths'], list(m['states']), m['k'], c_max=m['c_max'], frame_offset=m['frame_offset'], group=m['group'],
                      kp=m['kp'])
    res = _launch(batch, m['elp'], m['trans'], m['init'], m['lens'], m['endpen'], m['upstream'])
    worst = dict(case=name, R=L.ring_regs(m['k']), logz=0.0, **{k: 0.0 for k in KEYS})
    for z, g in res:
        worst['logz'] = max(worst['logz'], _err(z, ref_z))
        for k in KEYS:
            worst[k] = max(worst[k], _err(g[k], ref[k]))
    print(json.dumps(worst))
    for z, g in res:
        np.testing.assert_allclose(z, ref_z, **Z_BAR)
        assert np.all(g['elp'][~live] == 0)                         # padded columns: exactly 0
        for k in KEYS:                                              # (the reference is 0 in every padded row and column)
            np.testing.assert_allclose(g[k], ref[k], **G_BAR, err_msg=k)


MASKED = [(5, 8, (31, 20, 17)), (16, 40, (97, 64, 50)), (23, 70, (139, 92, 71)), (11, 600, (1100, 700, 650))]


@pytest.mark.parametrize('c,k,lengths', MASKED)
@pytest.mark.parametrize('neg_inf', [False, True])
def test_masked_lattices_match_the_twin(c, k, lengths, neg_inf):
    """The constrained path's lattices (test_gpu_viterbi.masked_problem: chain-masked transitions, one start, one end, -1e4
    narration penalties; every second video cycles through the chain and is explained through penalties only) with the masks at
    -1e9 and at true -inf: no NaN anywhere, log Z and the gradients are the twin's.  (The twin's own gradient is finite under
    true -inf -- asserted here; its masked entries carry no mass, as under -1e9.)"""
    ops = _ops()
    p = masked_problem(60 + c, list(lengths), c, k, neg_inf=neg_inf)
    b, tmax, _ = p['elp'].shape
    up = np.asarray([1.25, -0.75, 0.5])
    with np.errstate(all='ignore'):
        ref_z, ref = F.logz(p['elp'], p['lengths'], p['trans'], p['init'], p['lens'], p['endpen'], grad=True, upstream=up)
    assert np.isfinite(ref_z).all() and all(np.isfinite(v).all() for v in ref.values())
    batch = ops.Batch(p['lengths'], [c], k, c_max=c, t_max=tmax, total_frames=b * tmax)
    res = _launch(batch, p['elp'].reshape(b * tmax, c), p['trans'][None], p['init'][None], p['lens'][None], p['endpen'], up)
    kp = min(k, tmax)
    worst = dict(case='masked-%d-%d-%s' % (c, k, 'inf' if neg_inf else '1e9'), R=L.ring_regs(kp), logz=0.0, **{k_: 0.0 for k_ in KEYS})
    for z, g in res:
        ge = g['elp'].reshape(b, tmax, c)
        worst['logz'] = max(worst['logz'], _err(z, ref_z))
        worst['elp'] = max([worst['elp']] + [_err(ge[i, :t], ref['elp'][i, :t]) for i, t in enumerate(p['lengths'])])
        for k_, got in (('trans', g['trans'][0]), ('init', g['init'][0]), ('len', g['len'][0, :kp])):
            worst[k_] = max(worst[k_], _err(got, ref[k_]))
    print(json.dumps(worst))
    for z, g in res:
        assert not np.isnan(z).any() and not any(np.isnan(v).any() for v in g.values())
        np.testing.assert_allclose(z, ref_z, **Z_BAR)
        ge = g['elp'].reshape(b, tmax, c)
        for i, t in enumerate(p['lengths']):
            np.testing.assert_allclose(ge[i, :t], ref['elp'][i, :t], **G_BAR, err_msg='video %d' % i)
            assert np.all(ge[i, t:] == 0)
        np.testing.assert_allclose(g['trans'][0], ref['trans'], **G_BAR)
        np.testing.assert_allclose(g['init'][0], ref['init'], **G_BAR)
        np.testing.assert_allclose(g['len'][0, :kp], ref['len'], **G_BAR)
        assert np.all(g['len'][0, kp:] == 0)
        forbidden = p['trans'] < -1e8
        assert np.all(np.abs(g['trans'][0][forbidden]) <= 2e-5)     # the masked transitions carry no mass
