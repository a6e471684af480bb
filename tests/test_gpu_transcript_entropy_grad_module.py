"""``SemiMarkovModule.alignment_entropy`` / ``alignment_kl`` / ``alignment_cross_entropy`` and their ``_packed`` twins with
``differentiable=True``: parameter gradients against autograd through the enumerated value (route (a) of
tests/transcript_entropy_grad_ref.py) on ``factor_tables``' differentiable fp64 tables, both modules, at 1e-4 max(1, max |ref|)
per parameter; the value is bit-identical to ``differentiable=False``, which has no ``grad_fn``."""
import numpy as np
import pytest
import torch

import transcript_entropy_grad_ref as R
import transcript_sample_ref as TS
from test_gpu_entropy import _corpus, _features, _module
from test_gpu_entropy_grad import _param_grads

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BAR = 1e-4


def _ops():
    from action_segmentation_amd import ops
    return ops


def _case():
    m, g = _module(3, 5, 4, seed=904, scale=0.6)
    m2 = _module(3, 5, 4, seed=901, scale=0.6)[0]
    lengths = [7, 5, 6]
    x = _features(m, g, len(lengths), lengths, 5, noise=0.9)
    G = _ops().TranscriptGraph
    graphs = [G.from_candidates([[0, 1], [0, 1, 2], [2, 0]]), G.chain([1, 0, 2]), G.from_optional([0, 1, 2, 0], [1, 0, 1, 0])]
    return m, m2, x, lengths, graphs


def _ref_value(m, m2, x, lengths, graphs, mode, up):
    """sum_i up[i] V_i by enumeration on differentiable fp64 tables (factor_tables, the emission in torch)."""
    valid = torch.arange(m.n_classes)
    tot = 0.0
    for i, fr in enumerate(lengths):
        sides = []
        for mod in (m, m2):
            t = mod.factor_tables(valid, DEV)
            xe = x[i, :fr].to(DEV).double()
            elp = t['cst'] + xe @ t['w'] - 0.5 * (xe * xe) @ t['inv_var'].unsqueeze(1)
            ep = mod._endpen(valid, None, len(lengths), elp.shape[1], DEV)
            sides.append(((elp.cpu(), t['trans'].cpu(), t['init'].cpu(), t['len'].cpu()), None if ep is None else ep[i].cpu()))
        (tp, epp), (tq, epq) = sides
        g = graphs[i]
        a = [int(v) for v in g.ids]
        kp = min(tp[3].shape[0], max(lengths))
        npv = lambda v: v.detach().numpy()
        keys = list(TS.enumerate_alignments(npv(tp[0]), (g.ids, g.pred, g.start, g.end), npv(tp[1]), npv(tp[2]), npv(tp[3]), kp,
                                            None if epp is None else npv(epp)))
        lp = torch.log_softmax(R._scores(keys, fr, a, tp, epp), 0)
        lq = torch.log_softmax(R._scores(keys, fr, a, tq, epq), 0)
        pp = lp.exp()
        tot = tot + up[i] * dict(entropy=-(pp * lp).sum(), cross_entropy=-(pp * lq).sum(), kl=(pp * (lp - lq)).sum())[mode]
    return tot


def _close(got, want, what):
    worst = 0.0
    for a, r in zip(got, want):
        scale = max(1.0, float(r.abs().max()))
        worst = max(worst, float((a.double() - r.double()).abs().max()) / scale)
    print('\n[transcript-entropy-grad] module, %s: worst %.1e of max(1, max |ref|) (bar %.0e); max |ref| %s'
          % (what, worst, BAR, ['%.2g' % float(r.abs().max()) for r in want]))
    assert worst <= BAR
    assert min(float(r.abs().max()) for r in want) >= 1e-2                  # (the premise of the relative bar, per parameter)


@pytest.mark.parametrize('mode', ['entropy', 'cross_entropy', 'kl'])
def test_module_gradients_against_enumeration(mode):
    m, m2, x, lengths, graphs = _case()
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(3)] * len(lengths), graphs)
    up = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64, device=DEV)
    if mode == 'entropy':
        f = lambda d, **kw: m.alignment_entropy(*args, differentiable=d, **kw)
        other = m
    else:
        meth = m.alignment_cross_entropy if mode == 'cross_entropy' else m.alignment_kl
        f = lambda d, **kw: meth(m2, *args, differentiable=d, **kw)
        other = m2
    v0 = f(False)
    assert v0.grad_fn is None and not v0.requires_grad
    v1, parts = f(True, want_parts=True)
    assert v1.grad_fn is not None and torch.equal(v0, v1.detach())
    assert parts.shape == (3, 3) and parts.grad_fn is None and torch.equal(parts, f(False, want_parts=True)[1])
    _close(_param_grads(m, (v1 * up).sum()), _param_grads(m, _ref_value(m, other, x, lengths, graphs, mode, up.cpu())), mode + ', p')
    if other is not m:
        _close(_param_grads(other, (f(True) * up).sum()), _param_grads(other, _ref_value(m, other, x, lengths, graphs, mode, up.cpu())),
               mode + ', q')


def test_kl_with_itself_reaches_the_module_twice():
    m, _, x, lengths, graphs = _case()
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(3)] * len(lengths), graphs)
    v = m.alignment_kl(m, *args, differentiable=True)
    assert (v.detach() == 0.0).all()
    for gg in _param_grads(m, v.sum()):
        assert float(gg.abs().max()) <= 1e-9


def test_a_video_without_an_alignment_is_refused_by_name():
    m, m2, x, lengths, graphs = _case()
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(3)] * len(lengths))
    long = _ops().TranscriptGraph.chain([0, 1, 2, 0, 1, 2, 0])               # 7 nodes over the 5 frames of video 1
    bad = [graphs[0], long, graphs[2]]
    assert torch.isnan(m.alignment_entropy(*args, bad)[1])
    with pytest.raises(ValueError, match="alignment_entropy: .*video 1"):
        m.alignment_entropy(*args, bad, differentiable=True)
    with pytest.raises(ValueError, match="alignment_kl: .*video 1"):
        m.alignment_kl(m2, *args, bad, differentiable=True)


@pytest.mark.parametrize('mode', ['entropy', 'kl', 'cross_entropy'])
def test_packed_gradient_is_the_sum_of_batch_gradients(mode):
    """The ``_packed`` twins on a two-task corpus: the value is the non-differentiable one's, bit for bit, and the parameter
    gradient is the sum of the per-batch gradients of the padded methods."""
    m, batches, pc = _corpus()
    m2 = _module(9, 10, 40, seed=62, scale=0.5)[0]
    G = _ops().TranscriptGraph
    rng = np.random.default_rng(12)
    per_batch = [[G.from_candidates([rng.choice(bt['task_indices'][0].numpy(), size=6), rng.choice(bt['task_indices'][0].numpy(), size=9)])
                  for _ in bt['video_name']] for bt in batches]
    by_name = {n: g for bt, gs in zip(batches, per_batch) for n, g in zip(bt['video_name'], gs)}
    graphs = [by_name[n] for n in pc.video_names]
    if mode == 'entropy':
        packed = lambda d: m.alignment_entropy_packed(pc, graphs, differentiable=d)
        padded = lambda bt, gs: m.alignment_entropy(bt['features'].float().to(DEV), bt['lengths'].to(DEV), bt['task_indices'], gs,
                                                    differentiable=True)
    else:
        pk = m.alignment_kl_packed if mode == 'kl' else m.alignment_cross_entropy_packed
        pd = m.alignment_kl if mode == 'kl' else m.alignment_cross_entropy
        packed = lambda d: pk(m2, pc, graphs, differentiable=d)
        padded = lambda bt, gs: pd(m2, bt['features'].float().to(DEV), bt['lengths'].to(DEV), bt['task_indices'], gs, differentiable=True)
    h0 = packed(False)
    h1 = packed(True)
    assert h0.grad_fn is None and h1.grad_fn is not None and torch.equal(h0, h1.detach()) and bool(torch.isfinite(h0).all())
    mods = (m,) if mode == 'entropy' else (m, m2)
    got = [_param_grads(mod, packed(True).sum()) for mod in mods]
    for mod, gp in zip(mods, got):
        want = None
        for bt, gs in zip(batches, per_batch):
            gb = _param_grads(mod, padded(bt, gs).sum())
            want = gb if want is None else [a + b for a, b in zip(want, gb)]
        for a, r in zip(gp, want):
            scale = max(1.0, float(r.abs().max()))
            assert float((a - r).abs().max()) <= 1e-5 * scale, (a, r)
