"""The minimum-Bayes-risk decode under frame loss (smm_mbr_f64 / ops.mbr / SemiMarkovModule.mbr_decode, mbr_decode_packed /
SemiMarkovModel.predict(decoder='mbr')) on the GPU.

Its definition is the Viterbi DP on substituted inputs (include/smmdp.h): elp = the gain (the frame posteriors), zero length
scores, binary tables M(x) = -1e9 where x <= -5e8, else 0.  Checked bit for bit against the C twin's Viterbi and against
smm_viterbi_f64 on those inputs; against every segmentation of small lattices; and on the bench workloads for what users want of
it: at least as many expected correct frames as the Viterbi path, under the same constraints."""
import numpy as np
import pytest
import torch

from oracle import factored as F

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BIG_NEG = -1e9


def _M(x):
    return np.where(np.asarray(x, np.float64) <= BIG_NEG / 2, BIG_NEG, 0.0)


def _t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _h(t):
    return None if t is None else t.detach().cpu().numpy()


def _kp_of(batch):
    return batch.kp if batch.kp is not None else np.full(batch.b, min(batch.k_rows, batch.t_max), np.int32)


def _group_of(batch):
    return batch.group if batch.group is not None else np.zeros(batch.b, np.int32)


def _labels_from_spans(row, nf):
    """Per-frame local labels of frames 0..nf-1 from a span row (a start at every position where row >= 0)."""
    lab = np.empty(nf, np.int64)
    cur = -1
    for t in range(nf):
        if row[t] >= 0:
            cur = row[t]
        lab[t] = cur
    return lab


def _serial_sum(vals):
    return float(np.cumsum(np.asarray(vals, np.float64))[-1]) if len(vals) else 0.0


def _twin(batch, gain_h, trans_h, init_h, endpen_h, videos):
    """The C twin's Viterbi on the substituted inputs, per (group, kp) class of videos -> {video: (local span row, best)}."""
    kps, groups = _kp_of(batch), _group_of(batch)
    out = {}
    classes = {}
    for i in videos:
        classes.setdefault((int(groups[i]), int(kps[i])), []).append(i)
    for (g, kp), vids in classes.items():
        C = int(batch.n_states[g])
        lens = np.array([batch.lengths[i] for i in vids], np.int64)
        tm = max(int(lens.max()), kp)                       # (the twin clips its length table to its Tmax)
        elp = np.zeros((len(vids), tm, C))
        for r, i in enumerate(vids):
            o = int(batch.frame_offset[i])
            elp[r, :lens[r]] = gain_h[o:o + lens[r], :C]
        ep = None if endpen_h is None or batch.no_eos else _M(np.stack([endpen_h[i, :C] for i in vids]))
        spans, v = F.viterbi(elp, lens, _M(trans_h[g, :C, :C]), _M(init_h[g, :C]), np.zeros((kp, C)), ep, no_eos=batch.no_eos)
        for r, i in enumerate(vids):
            out[i] = (spans[r], v[r])
    return out


def _check(batch, gain, trans, init, endpen=None, class_map=None, videos=None, with_viterbi=True):
    """ops.mbr against the twin and (with_viterbi) against ops.viterbi on the substituted inputs; gain_sum against a host sum
    along the labels.  Returns the ops.mbr outputs on the host."""
    from action_segmentation_amd import ops
    out = ops.mbr(batch, gain, trans, init, endpen=endpen, class_map=class_map)
    torch.cuda.synchronize()
    assert ops.error_flag(batch, out) == 0
    res = {k: _h(out[k]) for k in ('spans', 'labels', 'best', 'gain_sum', 'n_segs')}
    if with_viterbi:
        lz = torch.zeros((batch.n_groups, batch.k_rows, batch.c_max), dtype=torch.float64, device=DEV)
        mt, mi = torch.from_numpy(_M(_h(trans))).to(DEV), torch.from_numpy(_M(_h(init))).to(DEV)
        me = None if endpen is None else torch.from_numpy(_M(_h(endpen))).to(DEV)
        vit = ops.viterbi(batch, gain, mt, mi, lz, endpen=me, class_map=class_map)
        torch.cuda.synchronize()
        assert ops.error_flag(batch, vit) == 0
        for k in ('spans', 'labels', 'best', 'n_segs'):
            assert np.array_equal(_h(vit[k]), res[k]), k
    gain_h, trans_h, init_h, endpen_h = _h(gain), _h(trans), _h(init), _h(endpen)
    cmap = _h(class_map)
    groups = _group_of(batch)
    videos = range(batch.b) if videos is None else videos
    twin = _twin(batch, gain_h, trans_h, init_h, endpen_h, videos)
    for i in videos:
        g, nf, o = int(groups[i]), int(batch.lengths[i]), int(batch.frame_offset[i])
        C = int(batch.n_states[g])
        sp_local, v = twin[i]
        assert res['best'][i] == v, (i, res['best'][i], v)
        gid = (lambda c: c) if cmap is None else (lambda c: int(cmap[g, c]))
        want = np.full(batch.t_max + 1, -1, np.int64)
        for n in range(nf + 1):
            if n < len(sp_local) and sp_local[n] >= 0:
                want[n] = gid(int(sp_local[n]))
        assert np.array_equal(res['spans'][i], want), i
        lab = _labels_from_spans(sp_local, nf)
        assert (lab >= 0).all() and (lab < C).all()
        assert np.array_equal(res['labels'][o:o + nf], np.array([gid(int(c)) for c in lab])), i
        assert res['n_segs'][i] == int((sp_local[:nf] >= 0).sum()), i
        assert res['gain_sum'][i] == _serial_sum(gain_h[o + np.arange(nf), lab]), i
    return res


# ------------------------------------------------------------------------------------------------ 1. bit-exact, random shapes
def _random_case(seed, b, cs, cm, k_rows, t_max, no_eos=False, self_trans=True, masks=False, quant=False, gaps=True):
    from action_segmentation_amd import ops
    rng = np.random.default_rng(seed)
    G = len(cs)
    lengths = rng.integers(2, t_max + 1, size=b)
    lengths[0] = t_max
    group = rng.integers(0, G, size=b).astype(np.int32)
    kp = rng.integers(2, k_rows + 1, size=b).astype(np.int32)
    kp[0] = k_rows
    gap = rng.integers(0, 5, size=b) if gaps else np.zeros(b, np.int64)
    off = np.concatenate([[0], np.cumsum(lengths + gap)[:-1]]).astype(np.int64)
    total = int(off[-1] + lengths[-1] + gap[-1])
    gain = rng.random((total, cm))
    if quant:
        gain = np.floor(gain * 4) / 4                    # many exact ties
    trans = rng.normal(size=(G, cm, cm))
    init = rng.normal(size=(G, cm))
    endpen = np.where(rng.random((b, cm)) < 0.3, BIG_NEG, 0.0)
    endpen[:, 0] = 0.0
    if masks:
        trans[rng.random(trans.shape) < 0.35] = -np.inf
        trans[rng.random(trans.shape) < 0.1] = BIG_NEG
        init[rng.random(init.shape) < 0.4] = -np.inf
        init[:, 0] = 0.5
    if not self_trans:
        for c in range(cm):
            trans[:, c, c] = -np.inf
    cmap = np.zeros((G, cm + 1), np.int64)
    for g, c in enumerate(cs):
        cmap[g, :c] = rng.permutation(40)[:c]
        cmap[g, c] = 40                                   # EOS id
    batch = ops.Batch(lengths, cs, k_rows, c_max=cm, frame_offset=off, group=group, kp=kp, t_max=t_max, total_frames=total,
                      no_eos=no_eos)
    return batch, _t(gain), _t(trans), _t(init), (None if no_eos else _t(endpen)), _t(cmap, torch.int64)


RANDOM = [
    # seed, b, states per group, c_max, k_rows, t_max, no_eos, self transitions, masks, quantised gains
    (1, 5, [2], 2, 2, 40, False, True, False, False),
    (2, 6, [3, 5], 6, 7, 90, False, True, True, False),
    (3, 7, [7, 4, 6], 8, 33, 300, False, False, False, True),
    (4, 4, [11], 11, 64, 500, True, True, True, False),
    (5, 6, [16, 9], 17, 130, 700, False, False, True, True),
    (6, 5, [23, 21, 13], 23, 1024, 2600, False, True, False, False),
    (7, 4, [32], 32, 1024, 3100, False, False, True, False),
    (8, 6, [31, 5], 32, 257, 1200, True, False, False, True),
    (9, 8, [1, 4], 5, 5, 30, False, True, False, True),
    (10, 3, [19], 20, 2, 400, True, False, True, False),
]


@pytest.mark.parametrize('case', RANDOM, ids=[str(c[0]) for c in RANDOM])
def test_bit_exact_on_random_shapes(case):
    """Ragged lengths and per-video span limits, several groups with padded c_max, masks of -inf / -1e9, self-transitions
    allowed or not, add_eos=False, ties: spans, labels, n_segs and best equal the twin's and smm_viterbi_f64's on the substituted
    inputs; gain_sum is the serial host sum along the labels."""
    seed, b, cs, cm, k_rows, t_max, no_eos, self_trans, masks, quant = case
    _check(*_random_case(seed, b, cs, cm, k_rows, t_max, no_eos, self_trans, masks, quant))


# ------------------------------------------------------------------------------------------------ posteriors of real models
_WL = {}


@pytest.fixture(scope='module', autouse=True)
def _release_workloads():
    yield
    _WL.clear()


def _workload(name):
    """(data, model, packed corpus) of a bench workload (bench.py's corpus and closed-form fit).  '<cfg>_t<s>': the same with
    the fitted covariance scaled by s -- emissions s times flatter, a posterior spread over many segmentations (the fitted
    models of the synthetic corpora are nearly certain of theirs)."""
    if name not in _WL:
        import bench
        from action_segmentation_amd import synth
        base, _, temper = name.partition('_t')
        a = bench.parse(['--workload', base])
        data = synth.SynthDatasplit(base, seed=a.seed, device=DEV, scale=a.scale)
        _, model = bench.fit_model(a, synth.CONFIGS[base], data, DEV, None, 1)
        if temper:
            with torch.no_grad():
                model.model.gaussian_cov.mul_(float(temper))
        _WL[name] = (data, model, model.prepare(data))
    return _WL[name]


def _posterior(pc):
    """emission -> log Z (both directions) -> marginals on the corpus: the gain the MBR decode of the corpus uses."""
    from action_segmentation_amd import ops
    t = pc.tables
    ws = torch.empty(pc.batch.workspace_bytes(), dtype=torch.uint8, device=DEV)
    elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
    z = ops.logz(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, ws=ws, with_backward=True)
    g = ops.logz_bwd(pc.batch, elp, t['trans'], t['init'], t['len'], z, endpen=pc.endpen, ws=ws, with_backward=True)
    return elp, g['elp']


@pytest.mark.parametrize('name', ['cfg4', 'cfg2', 'cfg3', 'cfg4_t40'])
def test_bit_exact_on_bench_workloads(name):
    """The corpus' own posterior (narration constraints and ordering masks on cfg4, K = 256 on cfg2, K = 1024 and up to 23
    states per task on cfg3, all videos in one launch; a spread posterior on the tempered cfg4) against the twin and
    smm_viterbi_f64 on the substituted inputs.  The twin
    checks every video of cfg4 and cfg2 and every second video of cfg3 (all of them take ~10 s on 16 threads)."""
    _, _, pc = _workload(name)
    t = pc.tables
    _, gain = _posterior(pc)
    videos = range(0, pc.batch.b, 2) if name == 'cfg3' else None
    _check(pc.batch, gain, t['trans'], t['init'], endpen=pc.endpen, class_map=t['class_map'], videos=videos)


def _count_masked(seq, g, C, trans_h, init_h, endpen_row, no_eos):
    """Masked terms of a segment class sequence (in EOS mode the last entry is the EOS id C)."""
    cnt = int(_M(init_h[g, seq[0]]) != 0)
    body = seq if no_eos else seq[:-1]
    for a, b in zip(body[:-1], body[1:]):
        cnt += int(_M(trans_h[g, b, a]) != 0)
    if not no_eos:
        last = body[-1]
        if seq[-1] == C:
            cnt += int(endpen_row is not None and _M(endpen_row[last]) != 0)
        else:
            cnt += 1 + int(_M(trans_h[g, seq[-1], last]) != 0)
    return cnt


def _local_rows(spans, cmap_h, groups, n_states):
    out = np.full(spans.shape, -1, np.int64)
    for i in range(spans.shape[0]):
        g = int(groups[i])
        inv = {int(cmap_h[g, c]): c for c in range(int(n_states[g]) + 1)}
        for n in np.nonzero(spans[i] >= 0)[0]:
            out[i, n] = inv[int(spans[i, n])]
    return out


@pytest.mark.parametrize('name', ['cfg4', 'cfg2', 'cfg3', 'cfg4_t40', 'cfg2_t40'])
def test_more_expected_correct_frames_than_viterbi(name):
    """With the same posterior, every video: expected correct frames of the MBR result >= those of the Viterbi path minus
    1e-9 T, and the Viterbi path uses no more masked terms than the MBR result (so it is among the paths the MBR decode
    maximises over).  (The bench corpora's posteriors are sharp: the two decodes often coincide.)"""
    from action_segmentation_amd import ops
    _, _, pc = _workload(name)
    t, batch = pc.tables, pc.batch
    elp, gain = _posterior(pc)
    mb = ops.mbr(batch, gain, t['trans'], t['init'], endpen=pc.endpen, class_map=t['class_map'])
    vit = ops.viterbi(batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    ops.check_decoded(batch, mb)
    ops.check_decoded(batch, vit)
    gain_h, trans_h, init_h, endpen_h, cmap_h = _h(gain), _h(t['trans']), _h(t['init']), _h(pc.endpen), _h(t['class_map'])
    groups = _group_of(batch)
    sm, sv = _local_rows(_h(mb['spans']), cmap_h, groups, batch.n_states), _local_rows(_h(vit['spans']), cmap_h, groups,
                                                                                       batch.n_states)
    ec = _h(mb['gain_sum'])
    gains = []
    for i in range(batch.b):
        g, nf, o = int(groups[i]), int(batch.lengths[i]), int(batch.frame_offset[i])
        C = int(batch.n_states[g])
        lab_v = _labels_from_spans(sv[i], nf)
        ev = _serial_sum(gain_h[o + np.arange(nf), lab_v])
        assert ec[i] >= ev - 1e-9 * nf, (i, ec[i], ev)
        ep = None if endpen_h is None else endpen_h[i]
        seq_m = [int(c) for c in sm[i, :nf + 1] if c >= 0]
        seq_v = [int(c) for c in sv[i, :nf + 1] if c >= 0]
        mm = _count_masked(seq_m, g, C, trans_h, init_h, ep, batch.no_eos)
        mv = _count_masked(seq_v, g, C, trans_h, init_h, ep, batch.no_eos)
        assert mv <= mm, (i, mv, mm)
        gains.append(ec[i] - ev)
    print('%s: expected correct frames, MBR - Viterbi: mean %.3f, max %.3f frames over %d videos'
          % (name, float(np.mean(gains)), float(np.max(gains)), len(gains)))


def test_valid_segmentations_where_the_frame_argmax_is_not():
    """Constrained cfg4 (tempered: a spread posterior): the MBR labels obey the span limit, the ordering masks, the allowed starts
    and the allowed ends (no masked term at all); the per-frame argmax of the posterior breaks them on at least one video."""
    from action_segmentation_amd import ops
    _, _, pc = _workload('cfg4_t40')
    t, batch = pc.tables, pc.batch
    _, gain = _posterior(pc)
    mb = ops.mbr(batch, gain, t['trans'], t['init'], endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    ops.check_decoded(batch, mb)
    gain_h, trans_h, init_h, endpen_h, cmap_h = _h(gain), _h(t['trans']), _h(t['init']), _h(pc.endpen), _h(t['class_map'])
    groups, kps = _group_of(batch), _kp_of(batch)
    sm = _local_rows(_h(mb['spans']), cmap_h, groups, batch.n_states)
    assert _M(trans_h).min() == BIG_NEG                  # (the tables do carry masks)
    broken = 0
    for i in range(batch.b):
        g, nf, o, kp = int(groups[i]), int(batch.lengths[i]), int(batch.frame_offset[i]), int(kps[i])
        C = int(batch.n_states[g])
        starts = [n for n in range(nf + 1) if sm[i, n] >= 0]
        assert starts[0] == 0 and starts[-1] == nf and sm[i, nf] == C
        assert all(0 < b - a <= kp - 1 for a, b in zip(starts[:-1], starts[1:]))
        seq = [int(sm[i, n]) for n in starts]
        ep = None if endpen_h is None else endpen_h[i]
        assert _count_masked(seq, g, C, trans_h, init_h, ep, False) == 0, i
        # the argmax: a run of one class may be several segments only where the class may follow itself
        am = np.argmax(gain_h[o:o + nf, :C], axis=1)
        cuts = [0] + [f for f in range(1, nf) if am[f] != am[f - 1]] + [nf]
        bad = _M(init_h[g, am[0]]) != 0 or (ep is not None and _M(ep[am[-1]]) != 0)
        for a, b in zip(cuts[:-1], cuts[1:]):
            c = int(am[a])
            if a > 0:
                bad |= _M(trans_h[g, c, int(am[a - 1])]) != 0
            if b - a > kp - 1:
                bad |= _M(trans_h[g, c, c]) != 0
        broken += int(bad)
    print('cfg4: the per-frame argmax breaks the constraints on %d of %d videos' % (broken, batch.b))
    assert broken >= 1


# ------------------------------------------------------------------------------------------------ 2. brute force
def _module(n_classes, d, k, seed, constrained=False, scale=1.0):
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    from module_util import make_args
    g = torch.Generator().manual_seed(seed)
    kw = {}
    if constrained:
        trans = {s: {s, s + 1} for s in range(n_classes - 1)}
        trans[n_classes - 1] = {n_classes - 1}
        trans[0].add(min(2, n_classes - 1))
        kw = dict(allowed_starts={0, 1}, allowed_transitions=trans, allowed_ends={n_classes - 1, n_classes - 2})
    m = SemiMarkovModule(make_args(k), n_classes, d, allow_self_transitions=True, **kw)
    with torch.no_grad():
        m.poisson_log_rates.copy_(torch.rand(n_classes, generator=g) * 1.5 + 0.2)
        m.gaussian_means.copy_(torch.randn(n_classes, d, generator=g) * scale)
        m.gaussian_cov.copy_(torch.diag(1.0 + torch.rand(d, generator=g)))
        m.transition_logits.copy_(torch.randn(n_classes, n_classes, generator=g))
        m.init_logits.copy_(torch.randn(n_classes, generator=g))
    return m.to(DEV), g


def _enumerate(T, C, kp, no_eos):
    """Every segmentation of positions 0..T-1 (segments of 1..kp-1 frames), as (starts, classes); no EOS: plus the closing
    label of the last frame."""
    out = []

    def rec(n, starts, classes):
        if n == T:
            if no_eos:
                for c in range(C):
                    out.append((starts, classes + [c]))
            else:
                out.append((starts, classes))
            return
        for k in range(1, kp):
            if n + k > T:
                break
            for c in range(C):
                rec(n + k, starts + [n], classes + [c])

    rec(0, [], [])
    return out


def _score(elp, trans, init, lens, ep, T, starts, classes, no_eos):
    s = init[classes[0]]
    bounds = starts + [T]
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        c = classes[i]
        if i > 0:
            s += trans[c, classes[i - 1]]
        s += lens[b - a, c] + elp[a:b, c].sum()
    if no_eos:
        s += trans[classes[-1], classes[-2]] + elp[T, classes[-1]]
    elif ep is not None:
        s += ep[classes[-1]]
    return s


@pytest.mark.parametrize('k,add_eos,constrained,narration', [
    (3, True, False, False), (4, True, True, False), (4, False, False, False), (3, False, True, False), (4, True, False, True),
])
def test_against_every_segmentation_of_small_lattices(k, add_eos, constrained, narration):
    """mbr_decode on videos small enough to enumerate: the marginals formed from every segmentation match the GPU's (1e-6: the
    log Z kernels' exponentials; measured ~1e-7);
    expected_correct is the maximum of sum_t P(y_t) over the segmentations of non-zero mass (1e-12), and the returned labels
    attain it (a different segmentation may only be returned when it is within rounding of the best)."""
    from action_segmentation_amd import ops
    c, d = 3, 5
    m, g = _module(c, d, k, seed=70 + k + 10 * add_eos + 20 * constrained, constrained=constrained, scale=1.2)
    lengths = [7, 5, 6, 4]
    b, tmax = len(lengths), max(lengths)
    lab = torch.randint(0, c, (b, tmax), generator=g)
    x = m.gaussian_means.detach().cpu()[lab] + torch.randn(b, tmax, d, generator=g) * 0.9
    for i, t in enumerate(lengths):
        x[i, t:] = 0
    valid = torch.arange(c)
    cons = None
    if narration:
        cons = torch.randn(b, tmax, c, generator=g).double() * 0.3
        cons[0, 2, 1] = -1e9
        cons[1, 0:2, 2] = -1e9
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [valid] * b)
    kw = dict(add_eos=add_eos, constraints=None if cons is None else cons.to(DEV))
    spans, ec = m.mbr_decode(*args, **kw)
    ec = _h(ec)
    post = _h(m.frame_posteriors(*args, **kw))
    r = m._posterior_launch(*args, add_eos, None, kw['constraints'], 'test')
    elp = _h(r['elp']).reshape(b, tmax, -1)
    trans, init, lens = _h(r['trans'])[0], _h(r['init'])[0], _h(r['len'])[0]
    ep = None if r['endpen'] is None else _h(r['endpen'])
    kp = min(lens.shape[0], tmax)
    for i, nf in enumerate(lengths):
        T = nf - (0 if add_eos else 1)
        segs = _enumerate(T, c, kp, not add_eos)
        sc = np.array([_score(elp[i], trans, init, lens, None if ep is None else ep[i], T, s, cl, not add_eos) for s, cl in segs])
        p = np.exp(sc - sc.max())
        p /= p.sum()
        labs = []
        for s, cl in segs:
            bounds = s + [T]
            row = np.concatenate([np.full(bb - a, cl[j]) for j, (a, bb) in enumerate(zip(bounds[:-1], bounds[1:]))]
                                 + ([[cl[-1]]] if not add_eos else []))
            labs.append(row.astype(np.int64))
        labs = np.stack(labs)
        marg = np.zeros((nf, c))
        for j in range(c):
            marg[:, j] = (p[:, None] * (labs == j)).sum(0)
        np.testing.assert_allclose(post[i, :nf], marg, rtol=0, atol=1e-6)
        # the candidates of the definition: the fewest masked table terms (none here: every video has an unmasked path)
        masked = np.array([_count_masked(cl if not add_eos else cl + [c], 0, c, trans[None], init[None],
                                         None if ep is None else ep[i], not add_eos) for _, cl in segs])
        assert masked.min() == 0
        feasible = masked == 0
        obj = np.array([_serial_sum(post[i, np.arange(nf), row]) for row in labs])
        best = obj[feasible].max()
        assert abs(ec[i] - best) <= 1e-12 * max(1.0, abs(best)), (i, ec[i], best)
        got = _labels_from_spans(spans[i].numpy(), nf)
        assert got.min() >= 0
        hits = [j for j in np.nonzero(feasible)[0] if np.array_equal(labs[j], got)]
        assert hits, i
        assert max(obj[j] for j in hits) >= best - 1e-12 * max(1.0, abs(best))


# ------------------------------------------------------------------------------------------------ 5. layers
def _tiny_model(seed=11):
    from action_segmentation_amd import synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    data = synth.SynthDatasplit('tiny', seed=seed)
    fitted = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    fitted.fit(data, use_labels=True)
    args = synth.make_args(data.max_k, cuda=True, batch_size=2, sm_constrain_transitions=True,
                           sm_constrain_with_narration=['test'])
    model = SemiMarkovModel.from_args(args, data)
    model.model.load_state_dict(fitted.model.state_dict(), strict=False)
    model.model.cuda()
    return data, model


def test_call_paths_agree_and_feed_the_evaluation():
    """predict(decoder='mbr') fused (mbr_decode_packed) and per batch (mbr_decode) give the same labels and expected correct
    frames; the labels feed accuracy_corpus; decoder='viterbi' -- and the default -- is the Viterbi decode as before;
    --sm_decoder mbr switches the default."""
    from action_segmentation_amd import evaluation
    from action_segmentation_amd.batching import make_data_loader
    data, model = _tiny_model()
    base = model.predict(data)
    vit = model.predict(data, decoder='viterbi')
    assert sorted(base) == sorted(vit) and all(np.array_equal(base[k], vit[k]) for k in base)
    fused = model.predict(data, decoder='mbr')
    loop = model.predict(data, decoder='mbr', fused=False)
    assert sorted(fused) == sorted(loop) == sorted(base)
    for k in fused:
        assert np.array_equal(fused[k], loop[k]), k
    stats = evaluation.accuracy_corpus(data, fused, False, seed=3)
    assert stats
    model.args.sm_decoder = 'mbr'
    again = model.predict(data)
    assert all(np.array_equal(again[k], fused[k]) for k in fused)
    model.args.sm_decoder = 'viterbi'
    # expected correct frames: packed against per batch
    pc = model.prepare(data)
    _, ec_packed = model.model.mbr_decode_packed(pc)
    ec_packed = _h(ec_packed)
    pos = {name: j for j, name in enumerate(pc.video_names)}
    cons_fn = model._test_constraints(data)
    n = 0
    for batch in make_data_loader(model.args, data, shuffle=False, batch_by_task=True, batch_size=model.args.batch_size):
        feats, lengths = batch['features'].to(DEV), batch['lengths']
        addl = model.make_additional_allowed_ends(batch['task_name'], lengths)
        spans, ec = model.model.mbr_decode(feats, lengths, batch['task_indices'], additional_allowed_ends_per_instance=addl,
                                           constraints=cons_fn(batch) if cons_fn else None)
        for i, name in enumerate(batch['video_name']):
            ref = ec_packed[pos[name]]
            assert abs(float(ec[i]) - ref) <= 1e-12 * max(1.0, ref), (name, float(ec[i]), ref)
            assert 0 < ref <= int(lengths[i])
            n += 1
    assert n == len(pc.video_names)


def test_gain_sum_is_the_posterior_summed_along_the_labels():
    """The module's expected_correct equals frame_posteriors gathered along the returned labels and summed on the host."""
    from action_segmentation_amd import ops
    m, g = _module(6, 8, 12, seed=5, scale=0.8)
    lengths = [60, 45, 33]
    b, tmax = len(lengths), max(lengths)
    lab = torch.randint(0, 6, (b, tmax), generator=g)
    x = m.gaussian_means.detach().cpu()[lab] + torch.randn(b, tmax, 8, generator=g) * 1.2
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(6)] * b)
    spans, ec = m.mbr_decode(*args)
    post = _h(m.frame_posteriors(*args))
    for i, nf in enumerate(lengths):
        got = _labels_from_spans(spans[i].numpy(), nf)
        ref = _serial_sum(post[i, np.arange(nf), got])
        assert abs(float(ec[i]) - ref) <= 1e-12 * nf, (i, float(ec[i]), ref)
    # add_eos=False: b x Tmax spans, as viterbi returns them
    sp2, ec2 = m.mbr_decode(*args, add_eos=False)
    assert tuple(sp2.shape) == (b, tmax) and np.isfinite(_h(ec2)).all()


# ------------------------------------------------------------------------------------------------ 6. errors
def test_nan_in_one_video_sets_the_error_word():
    from action_segmentation_amd import _lib, ops
    batch, gain, trans, init, endpen, cmap = _random_case(21, 4, [5], 5, 9, 120)
    gh = _h(gain)
    o = int(batch.frame_offset[2])
    gh[o + 7, 3] = np.nan
    out = ops.mbr(batch, _t(gh), trans, init, endpen=endpen, class_map=cmap)
    torch.cuda.synchronize()
    assert ops.error_flag(batch, out) != 0
    best, gs = _h(out['best']), _h(out['gain_sum'])
    assert np.isnan(best[2]) and np.isnan(gs[2])
    assert np.isfinite(best[[0, 1, 3]]).all() and np.isfinite(gs[[0, 1, 3]]).all()
    with pytest.raises(_lib.SmmError):
        ops.check_decoded(batch, out)
    # the next call on clean inputs clears it
    out = ops.mbr(batch, gain, trans, init, endpen=endpen, class_map=cmap)
    torch.cuda.synchronize()
    assert ops.error_flag(batch, out) == 0
