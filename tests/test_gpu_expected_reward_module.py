"""The expected reward at the module and model layers (SemiMarkovModule.expected_reward / expected_accuracy /
expected_segment_count and their packed forms, SemiMarkovModel.expected_accuracy / expected_segment_counts) on the GPU: parameter
gradients against autograd through the enumerated value on the module's own differentiable tables, the packed gradient against
the per-batch ones, the bit-identity of the differentiable and the plain value, refusals, and the model-level conveniences on a
synthetic datasplit.  Every seed is fixed."""
import numpy as np
import pytest
import torch

import entropy_grad_ref as R
from test_gpu_entropy import _corpus
from test_gpu_entropy_grad import _module_case, _param_grads

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _enumerated_accuracy(m, x, lengths, labels, add_eos, up, seg_weight=0.0):
    """sum_i up[i] (E_p[correct frames of video i] + seg_weight E_p[segments]) by enumeration on differentiable fp64 tables
    (factor_tables, the emission in torch): test_gpu_entropy_grad._ref_module_value's construction."""
    valid = torch.arange(m.n_classes)
    tot = 0.0
    for i, fr in enumerate(lengths):
        t = m.factor_tables(valid, DEV)
        xe = x[i, :fr].to(DEV).double()
        elp = t['cst'] + xe @ t['w'] - 0.5 * (xe * xe) @ t['inv_var'].unsqueeze(1)
        tp = dict(elp=elp.cpu(), trans=t['trans'].cpu(), init=t['init'].cpu(), len=t['len'].cpu())
        frames, c = tp['elp'].shape
        k_rows = tp['len'].shape[0]
        kp = min(k_rows, max(lengths))
        phi, last = R.occurrences(frames, c, k_rows, kp, not add_eos)
        s = phi @ R._flat(tp)
        if add_eos:
            ep = m._endpen(valid, None, len(lengths), c, DEV)
            s = s + R._wend(tp['trans'], None if ep is None else ep[i].cpu())[last]
        onehot = torch.zeros(frames, c, dtype=torch.float64)
        for f in range(fr):
            if 0 <= int(labels[i, f]) < c:
                onehot[f, int(labels[i, f])] = 1.0
        close = torch.zeros(frames, c, dtype=torch.float64)
        if not add_eos:
            close[frames - 1] = seg_weight
        rho = R._flat(dict(elp=onehot + close, trans=torch.zeros(c, c, dtype=torch.float64), init=torch.zeros(c, dtype=torch.float64),
                           len=torch.full((k_rows, c), seg_weight, dtype=torch.float64)))
        tot = tot + up[i] * (torch.softmax(s, 0) * (phi @ rho)).sum()
    return tot


# Measured on one MI355X, worst |error| / max(1, max |ref|) over the parameters: 1.1e-7 (EOS), 1.3e-7 (no EOS), 1.0e-7 (constrained)
@pytest.mark.parametrize('add_eos,constrained', [(True, False), (False, False), (True, True)])
def test_module_gradients_against_enumeration(add_eos, constrained):
    """Parameter gradients of expected_accuracy(differentiable=True) -- labels with an id outside the class set and a negative
    one, which are never correct -- and of expected_reward with both rewards against autograd through the enumerated value:
    <= 1e-4 max(1, max |ref|) per parameter (test_gpu_entropy_grad.test_module_gradients_against_enumeration's tolerance).  The
    value is bit-identical to differentiable=False, which has no grad_fn."""
    m, g, x, lengths = _module_case(4, add_eos, constrained)
    b, tmax = len(lengths), max(lengths)
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(3)] * b)
    up = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64, device=DEV)
    labels = torch.randint(0, 3, (b, tmax), generator=g)
    labels[0, 1], labels[1, 2] = 7, -1
    f = lambda d: m.expected_accuracy(*args, labels, add_eos=add_eos, differentiable=d)
    v0 = f(False)
    assert v0.grad_fn is None
    v1 = f(True)
    assert v1.grad_fn is not None and torch.equal(v0, v1.detach())
    assert (v0.cpu() >= 0).all() and (v0.cpu() <= torch.tensor(lengths) + 1e-9).all()
    got = _param_grads(m, (v1 * up).sum())
    ref = _enumerated_accuracy(m, x, lengths, labels, add_eos, up.cpu())
    assert abs(float((v0 * up).sum()) - float(ref.detach())) <= 1e-6 * max(1.0, abs(float(ref.detach())))
    want = _param_grads(m, ref)
    worst = 0.0
    for a, r in zip(got, want):
        scale = max(1.0, float(r.abs().max()))
        worst = max(worst, float((a.double() - r.double()).abs().max()) / scale)
        assert float((a.double() - r.double()).abs().max()) <= 1e-4 * scale, (a, r)
    print('module expected_accuracy eos=%s constrained=%s: worst |error| / max(1, max |ref|) %.3g' % (add_eos, constrained, worst))
    assert max(float(r.abs().max()) for r in want) > 1e-3          # (a gradient worth the name)
    # normalize: the fraction of the video's frames
    vn = m.expected_accuracy(*args, labels, add_eos=add_eos, normalize=True)
    torch.testing.assert_close(vn, v0 / torch.tensor(lengths, dtype=torch.float64, device=DEV), rtol=1e-12, atol=1e-12)
    # both rewards at once: accuracy + 0.25 segments
    onehot = torch.nn.functional.one_hot(labels.clamp(0, 2), 3).double()
    onehot[0, 1], onehot[1, 2] = 0.0, 0.0
    v2 = m.expected_reward(*args, reward=onehot, seg_reward=torch.full((3,), 0.25), add_eos=add_eos, differentiable=True)
    cnt = m.expected_segment_count(*args, add_eos=add_eos)
    torch.testing.assert_close(v2.detach(), v0 + 0.25 * cnt, rtol=1e-9, atol=1e-9)
    got = _param_grads(m, (v2 * up).sum())
    want = _param_grads(m, _enumerated_accuracy(m, x, lengths, labels, add_eos, up.cpu(), seg_weight=0.25))
    for a, r in zip(got, want):
        scale = max(1.0, float(r.abs().max()))
        assert float((a.double() - r.double()).abs().max()) <= 1e-4 * scale, (a, r)


def test_rewards_that_require_grad_are_refused():
    m, g, x, lengths = _module_case()
    b, tmax = len(lengths), max(lengths)
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(3)] * b)
    reward = torch.zeros(b, tmax, 3, dtype=torch.float64, requires_grad=True)
    with pytest.raises(ValueError, match='requires grad'):
        m.expected_reward(*args, reward=reward, differentiable=True)
    with pytest.raises(ValueError, match='requires grad'):
        m.expected_reward(*args, seg_reward=torch.ones(3, requires_grad=True))
    with pytest.raises(ValueError):
        m.expected_reward(*args)                                  # no reward at all
    with pytest.raises(ValueError):
        m.expected_reward(*args, reward=torch.zeros(b, tmax, 2))  # the wrong shape


def test_packed_gradient_is_the_sum_of_batch_gradients():
    """expected_accuracy_packed(differentiable=True) on a two-task corpus: its value is the plain call's, bit for bit, each
    video's value is its padded batch's, and its parameter gradient is the sum of the per-batch gradients (1e-5, the
    tolerance of test_gpu_entropy_grad's packed test); expected_segment_count_packed agrees with the padded call."""
    m, batches, pc = _corpus()
    m.prepare_packed(pc)
    gen = torch.Generator().manual_seed(3)
    labels = torch.full((pc.batch.total_frames,), -1, dtype=torch.int64)
    per_batch, o = [], 0
    offs = [int(v) for v in pc.frame_offset]
    for bt in batches:
        valid, lens = bt['task_indices'][0], bt['lengths'].tolist()
        lab = valid[torch.randint(0, len(valid), (len(lens), max(lens)), generator=gen)]
        lab[0, 0] = 0 if 0 not in valid.tolist() else 3           # (an id outside this task's class set)
        per_batch.append(lab)
        for i, t in enumerate(lens):
            labels[offs[o]:offs[o] + t] = lab[i, :t]
            o += 1
    v0 = m.expected_accuracy_packed(pc, labels)
    v1 = m.expected_accuracy_packed(pc, labels, differentiable=True)
    assert v0.grad_fn is None and torch.equal(v0, v1.detach())
    got = _param_grads(m, v1.sum())
    want, vals, cnts = None, [], []
    for bt, lab in zip(batches, per_batch):
        a = (bt['features'].float().to(DEV), bt['lengths'].to(DEV), bt['task_indices'])
        vb = m.expected_accuracy(*a, lab, differentiable=True)
        vals.append(vb.detach())
        cnts.append(m.expected_segment_count(*a))
        gb = _param_grads(m, vb.sum())
        want = gb if want is None else [p + q for p, q in zip(want, gb)]
    torch.testing.assert_close(v0, torch.cat(vals), rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(m.expected_segment_count_packed(pc), torch.cat(cnts), rtol=1e-9, atol=1e-9)
    for a, r in zip(got, want):
        scale = max(1.0, float(r.abs().max()))
        assert float((a - r).abs().max()) <= 1e-5 * scale, (a, r)


def test_model_level_conveniences_on_a_synthetic_datasplit():
    """SemiMarkovModel.expected_accuracy: values in [0, frames], equal to the module-level call; against the ground truth when
    no labels are given; expected_segment_counts in [1, frames]; labels of the wrong length are refused."""
    from action_segmentation_amd import synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    data = synth.SynthDatasplit('tiny', seed=11)
    fitted = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    fitted.fit(data, use_labels=True)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=True, batch_size=2), data)
    model.model.load_state_dict(fitted.model.state_dict(), strict=False)
    model.model.cuda()
    pred = model.predict(data)
    acc = model.expected_accuracy(data, pred)
    pc = model.prepare(data)
    assert set(acc) == set(pc.video_names)
    packed = np.full(pc.batch.total_frames, -1, np.int64)
    for name, off, t in zip(pc.video_names, pc.frame_offset, pc.batch.lengths.tolist()):
        packed[int(off):int(off) + t] = np.asarray(pred[name])
        assert 0.0 <= acc[name] <= t + 1e-6
    direct = model.model.expected_accuracy_packed(pc, torch.from_numpy(packed)).cpu().numpy()
    assert [acc[n] for n in pc.video_names] == [float(v) for v in direct]
    gt = {name: data[(task, name)]['gt_single'].numpy() for (task, name) in data._videos}
    against_gt = model.expected_accuracy(data)
    assert against_gt == model.expected_accuracy(data, gt)
    # a fitted model on its own training labels: most frames are expected to be right
    frames = sum(pc.batch.lengths.tolist())
    assert sum(against_gt.values()) > 0.5 * frames
    counts = model.expected_segment_counts(data)
    for name, t in zip(pc.video_names, pc.batch.lengths.tolist()):
        assert 1.0 - 1e-9 <= counts[name] <= t + 1e-9
    with pytest.raises(ValueError):
        model.expected_accuracy(data, {name: v[:-1] for name, v in pred.items()})
