"""``SemiMarkovModule.alignment_expected_reward`` / ``alignment_expected_accuracy`` and their ``_packed`` twins, and the model
layer's ``alignment_expected_accuracy`` / ``candidate_expected_accuracy``.  With ``differentiable=True``: parameter gradients
against autograd through the enumerated expectation (route (a) of tests/transcript_expected_reward_ref.py) on ``factor_tables``'
differentiable fp64 tables, both modules of the sibling entropy test, at 1e-4 max(1, max |ref|) per parameter; the value is
bit-identical to ``differentiable=False``, which has no ``grad_fn``."""
import numpy as np
import pytest
import torch

import transcript_entropy_grad_ref as RG
import transcript_expected_reward_ref as R
import transcript_sample_ref as TS
from test_gpu_entropy import _corpus, _module
from test_gpu_entropy_grad import _param_grads
from test_gpu_transcript_entropy_grad_module import _case, _ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BAR, VAL_BAR = 1e-4, 1e-5


def _rewards(lengths, graphs, c, seed):
    """N(0, 1): reward b x Tmax x C (zeros on the padding), one node-reward vector per video, a per-class reward."""
    rng = np.random.default_rng(seed)
    w = np.zeros((len(lengths), max(lengths), c))
    for i, t in enumerate(lengths):
        w[i, :t] = rng.normal(size=(t, c))
    return torch.tensor(w), [torch.tensor(rng.normal(size=len(g))) for g in graphs], torch.tensor(rng.normal(size=c))


def _ref_value(m, x, lengths, graphs, reward, node_reward, up):
    """sum_i up[i] V_i by enumeration on differentiable fp64 tables (factor_tables, the emission in torch)."""
    valid = torch.arange(m.n_classes)
    tot = 0.0
    for i, fr in enumerate(lengths):
        t = m.factor_tables(valid, DEV)
        xe = x[i, :fr].to(DEV).double()
        elp = (t['cst'] + xe @ t['w'] - 0.5 * (xe * xe) @ t['inv_var'].unsqueeze(1)).cpu()
        ep = m._endpen(valid, None, len(lengths), elp.shape[1], DEV)
        ep = None if ep is None else ep[i].cpu()
        tabs = (elp, t['trans'].cpu(), t['init'].cpu(), t['len'].cpu())
        g = graphs[i]
        a = [int(v) for v in g.ids]
        kp = min(tabs[3].shape[0], max(lengths))
        npv = lambda v: v.detach().numpy()
        keys = list(TS.enumerate_alignments(npv(tabs[0]), (g.ids, g.pred, g.start, g.end), npv(tabs[1]), npv(tabs[2]), npv(tabs[3]), kp,
                                            None if ep is None else npv(ep)))
        pr = torch.softmax(RG._scores(keys, fr, a, tabs, ep), 0)
        w = None if reward is None else reward[i, :fr].numpy()
        nr = None if node_reward is None else node_reward[i].numpy()
        r = torch.tensor([R.reward_of(k, a, fr, w, nr) for k in keys], dtype=torch.float64)
        tot = tot + up[i] * (pr * r).sum()
    return tot


def _close(got, want, what):
    worst = 0.0
    for a, r in zip(got, want):
        scale = max(1.0, float(r.abs().max()))
        worst = max(worst, float((a.double() - r.double()).abs().max()) / scale)
    print('\n[transcript-expected-reward] module, %s: worst %.1e of max(1, max |ref|) (bar %.0e); max |ref| %s'
          % (what, worst, BAR, ['%.2g' % float(r.abs().max()) for r in want]))
    assert worst <= BAR
    assert min(float(r.abs().max()) for r in want) >= 1e-2                  # (the premise of the relative bar, per parameter)


@pytest.mark.parametrize('which', [0, 1], ids=['m', 'm2'])
def test_module_gradients_against_enumeration(which):
    """The sibling's first module, and a second draw of it (seed 906: the sibling's own second module has a decided initial
    class, an init gradient of 3e-4 whatever the reward, below the premise of the relative bar)."""
    m, _, x, lengths, graphs = _case()
    if which:
        m = _module(3, 5, 4, seed=906, scale=0.6)[0]
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(3)] * len(lengths), graphs)
    up = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64, device=DEV)
    reward, node_reward, _ = _rewards(lengths, graphs, 3, 5)
    f = lambda d, **kw: m.alignment_expected_reward(*args, reward=reward, node_reward=node_reward, differentiable=d, **kw)
    v0 = f(False)
    assert v0.grad_fn is None and not v0.requires_grad and v0.dtype == torch.float64 and v0.shape == (3,)
    v1, parts = f(True, want_parts=True)
    assert v1.grad_fn is not None and torch.equal(v0, v1.detach())
    assert parts.shape == (3, 2) and parts.grad_fn is None and torch.equal(parts, f(False, want_parts=True)[1])
    want = _ref_value(m, x, lengths, graphs, reward, node_reward, up.cpu())
    ref = _ref_value(m, x, lengths, graphs, reward, node_reward, torch.eye(3, dtype=torch.float64))
    scale = reward.abs().sum(dim=(1, 2)) + torch.stack([r.abs().sum() for r in node_reward])
    err = float(((v0.cpu() - ref.detach()).abs() / scale.clamp(min=1.0)).max())
    print('\n[transcript-expected-reward] module value against enumeration: %.1e of sum |r| (bar %.0e)' % (err, VAL_BAR))
    assert err <= VAL_BAR
    _close(_param_grads(m, (v1 * up).sum()), _param_grads(m, want), 'expected reward, module %d' % which)
    # labels: the expected number of correct frames
    labels = torch.tensor(np.random.default_rng(6).integers(-1, 4, size=(3, max(lengths))))      # (-1 and 3: never correct)
    a0 = m.alignment_expected_accuracy(*args, labels)
    a1 = m.alignment_expected_accuracy(*args, labels, differentiable=True)
    assert a0.grad_fn is None and a1.grad_fn is not None and torch.equal(a0, a1.detach())
    onehot = torch.stack([(labels == c) for c in range(3)], dim=-1).double()
    for i, t in enumerate(lengths):
        onehot[i, t:] = 0
    assert torch.equal(a0, m.alignment_expected_reward(*args, reward=onehot))
    frac = m.alignment_expected_accuracy(*args, labels, normalize=True)
    assert torch.equal(frac, a0 / torch.tensor(lengths, dtype=torch.float64, device=DEV)) and float(frac.max()) <= 1.0
    _close(_param_grads(m, (a1 * up).sum()), _param_grads(m, _ref_value(m, x, lengths, graphs, onehot, None, up.cpu())),
           'expected accuracy, module %d' % which)


def test_seg_reward_is_the_broadcast_node_reward():
    m, _, x, lengths, graphs = _case()
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(3)] * len(lengths), graphs)
    _, node_reward, seg = _rewards(lengths, graphs, 3, 7)
    by_class = [seg[torch.as_tensor(np.asarray(g.ids, np.int64))] for g in graphs]
    a = m.alignment_expected_reward(*args, seg_reward=seg)
    b = m.alignment_expected_reward(*args, node_reward=by_class)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    both = m.alignment_expected_reward(*args, node_reward=node_reward, seg_reward=seg)
    assert torch.equal(both, m.alignment_expected_reward(*args, node_reward=[n + c for n, c in zip(node_reward, by_class)]))
    ones = m.alignment_expected_reward(*args, seg_reward=torch.ones(3, dtype=torch.float64))
    assert abs(float(ones[1]) - 3.0) <= VAL_BAR * 3                       # (video 1 is a chain of three)
    with pytest.raises(ValueError, match="at least one of reward, node_reward and seg_reward"):
        m.alignment_expected_reward(*args)
    with pytest.raises(ValueError, match="requires grad"):
        m.alignment_expected_reward(*args, seg_reward=seg.clone().requires_grad_())


def test_a_video_without_an_alignment_is_refused_by_name():
    m, _, x, lengths, graphs = _case()
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(3)] * len(lengths))
    long = _ops().TranscriptGraph.chain([0, 1, 2, 0, 1, 2, 0])               # 7 nodes over the 5 frames of video 1
    bad = [graphs[0], long, graphs[2]]
    seg = torch.ones(3, dtype=torch.float64)
    assert torch.isnan(m.alignment_expected_reward(*args, bad, seg_reward=seg)[1])
    with pytest.raises(ValueError, match="alignment_expected_reward: .*video 1"):
        m.alignment_expected_reward(*args, bad, seg_reward=seg, differentiable=True)
    with pytest.raises(ValueError, match="1 graphs for 3 videos"):
        m.alignment_expected_reward(*args, graphs[:1], seg_reward=seg)
    with pytest.raises(ValueError, match="alignment_expected_reward: add_eos"):
        m.alignment_expected_reward(*args, graphs, seg_reward=seg, add_eos=False)


def test_packed_gradient_is_the_sum_of_batch_gradients():
    """The ``_packed`` twins on a two-task corpus: the value is the non-differentiable one's, bit for bit, and the parameter
    gradient is the sum of the per-batch gradients of the padded methods."""
    m, batches, pc = _corpus()
    G = _ops().TranscriptGraph
    rng = np.random.default_rng(12)
    per_batch = [[G.from_candidates([rng.choice(bt['task_indices'][0].numpy(), size=6), rng.choice(bt['task_indices'][0].numpy(), size=9)])
                  for _ in bt['video_name']] for bt in batches]
    by_name = {n: g for bt, gs in zip(batches, per_batch) for n, g in zip(bt['video_name'], gs)}
    graphs = [by_name[n] for n in pc.video_names]
    m.prepare_packed(pc)
    batch = pc.batch
    lab_by_name = {n: rng.integers(0, m.n_classes, size=int(t)) for bt in batches for n, t in zip(bt['video_name'], bt['lengths'])}
    labels = torch.full((batch.total_frames,), -1, dtype=torch.int64)
    for n, off in zip(pc.video_names, batch.frame_offset.tolist()):
        labels[off:off + len(lab_by_name[n])] = torch.as_tensor(lab_by_name[n])
    node_by_name = {n: torch.tensor(rng.normal(size=len(by_name[n]))) for n in by_name}
    nodes = [node_by_name[n] for n in pc.video_names]

    def padded(bt, gs, differentiable):
        lab = torch.full((len(gs), int(bt['lengths'].max())), -1, dtype=torch.int64)
        for i, n in enumerate(bt['video_name']):
            lab[i, :len(lab_by_name[n])] = torch.as_tensor(lab_by_name[n])
        args = (bt['features'].float().to(DEV), bt['lengths'].to(DEV), bt['task_indices'], gs)
        return (m.alignment_expected_accuracy(*args, lab, differentiable=differentiable)
                + m.alignment_expected_reward(*args, node_reward=[node_by_name[n] for n in bt['video_name']], differentiable=differentiable))

    packed = lambda d: (m.alignment_expected_accuracy_packed(pc, graphs, labels, differentiable=d)
                        + m.alignment_expected_reward_packed(pc, graphs, node_reward=nodes, differentiable=d))
    h0, h1 = packed(False), packed(True)
    assert h0.grad_fn is None and h1.grad_fn is not None and torch.equal(h0, h1.detach()) and bool(torch.isfinite(h0).all())
    value = {n: float(v) for bt, gs in zip(batches, per_batch) for n, v in zip(bt['video_name'], padded(bt, gs, False))}
    for n, v in zip(pc.video_names, h0.tolist()):
        assert abs(v - value[n]) <= 1e-9 * max(1.0, abs(value[n])), n
    got = _param_grads(m, h1.sum())
    want = None
    for bt, gs in zip(batches, per_batch):
        gb = _param_grads(m, padded(bt, gs, True).sum())
        want = gb if want is None else [a + b for a, b in zip(want, gb)]
    for a, r in zip(got, want):
        scale = max(1.0, float(r.abs().max()))
        assert float((a - r).abs().max()) <= 1e-5 * scale, (a, r)
    assert max(float(r.abs().max()) for r in want) >= 1e-2


def test_model_layer_expected_accuracies():
    """SemiMarkovModel.alignment_expected_accuracy on a tiny datasplit equals the module's value; candidate_expected_accuracy
    equals the candidate_posteriors-weighted sum of the candidates' own expected accuracies, within the value bar of T."""
    from action_segmentation_amd import ops, synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts
    data = synth.SynthDatasplit('tiny', seed=11)
    fitted = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    fitted.fit(data, use_labels=True)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=True, batch_size=2), data)
    model.model.load_state_dict(fitted.model.state_dict(), strict=False)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(5)
        model.model.gaussian_means.add_((0.3 * torch.randn(model.model.gaussian_means.shape, generator=gen)).to(model.model.gaussian_means.device))
    model.model.cuda()
    pc = model.prepare(data)
    t = pc.tables
    elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
    out = ops.viterbi(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    names = list(pc.video_names)
    tr = dict(zip(names, ([int(v) for v in a] for a in spans_to_transcripts(out['spans'], pc.lengths))))
    got = model.alignment_expected_accuracy(data, tr)
    assert set(got) == set(names)
    packed = model._packed_labels(pc, data, None, 'test')
    want = model.model.alignment_expected_accuracy_packed(pc, [ops.TranscriptGraph.chain(tr[n]) for n in names], packed).tolist()
    lengths = dict(zip(names, pc.batch.lengths.tolist()))
    for n, w in zip(names, want):
        assert got[n] == w and 0.0 < got[n] <= lengths[n] * (1 + VAL_BAR), n
    never = model.alignment_expected_accuracy(data, tr, {n: np.full(lengths[n], -1) for n in names})
    assert all(v == 0.0 for v in never.values())                              # (labels that are never correct)
    with pytest.raises(ValueError, match="alignment_expected_accuracy: no transcript for video"):
        model.alignment_expected_accuracy(data, {})
    cands = {v: [a, a[:-1] if len(a) > 1 else a + a, a + a[-1:]] for v, a in tr.items()}
    joint = model.candidate_expected_accuracy(data, cands)
    post = model.candidate_posteriors(data, cands)
    for k in range(3):
        each = model.alignment_expected_accuracy(data, {v: c[k] for v, c in cands.items()})
        for n in names:
            if post[n][k] > 0:
                joint[n] -= post[n][k] * each[n]
    worst = max(abs(joint[n]) / lengths[n] for n in names)
    print('\n[transcript-expected-reward] candidate_expected_accuracy against the weighted sum: %.1e of T (bar %.0e)' % (worst, VAL_BAR))
    assert worst <= VAL_BAR
