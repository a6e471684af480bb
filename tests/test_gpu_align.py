"""Forced alignment (smm_align_f64 / ops.align / SemiMarkovModule.align, align_packed / SemiMarkovModel.align) on the GPU.

spans, labels, best and n_segs are compared bit for bit with tests/align_ref.py (the definition in numpy) and, on videos that
have an alignment, with the C twin's Viterbi on the lattice whose states are the transcript positions -- on real-valued inputs
and on small-integer inputs, where many alignments tie exactly and the back-trace's tie rule decides."""
import numpy as np
import pytest
import torch

import align_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BIG_NEG = -1e9
P = 768                      # the kernel's tile (tests/test_align_host.py checks it against csrc/smm_align.hip)


def _t(a, dtype=torch.float64):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _h(t):
    return None if t is None else t.detach().cpu().numpy()


def _draw(rng, ties, *shape):
    return rng.integers(-3, 4, size=shape).astype(np.float64) if ties else rng.normal(size=shape) * 3.0


def _make(seed, videos, cs, cm, k_rows, ties, with_endpen=True, with_cmap=True, gaps=True, transcripts=None):
    """videos: [(T, kp, M, group)].  -> dict of host arrays, the Batch, and per-video transcripts (local ids, random unless
    given)."""
    from action_segmentation_amd import ops
    rng = np.random.default_rng(seed)
    G, b = len(cs), len(videos)
    lengths = np.array([v[0] for v in videos], np.int64)
    kp = np.array([v[1] for v in videos], np.int32)
    group = np.array([v[3] for v in videos], np.int32)
    gap = rng.integers(0, 4, size=b) if gaps else np.zeros(b, np.int64)
    off = np.concatenate([[0], np.cumsum(lengths + gap)[:-1]]).astype(np.int64)
    total = int(off[-1] + lengths[-1] + gap[-1])
    t_max = int(lengths.max())
    h = dict(elp=_draw(rng, ties, total, cm), trans=_draw(rng, ties, G, cm, cm), init=_draw(rng, ties, G, cm),
             len=_draw(rng, ties, G, k_rows, cm), endpen=None, cmap=None)
    if with_endpen:
        h['endpen'] = np.where(rng.random((b, cm)) < 0.3, BIG_NEG, 0.0) if not ties else _draw(rng, True, b, cm)
    if with_cmap:
        h['cmap'] = np.zeros((G, cm + 1), np.int64)
        for g, c in enumerate(cs):
            h['cmap'][g, :c] = rng.permutation(40)[:c]
            h['cmap'][g, c] = 40
    if transcripts is None:
        transcripts = [rng.integers(0, cs[v[3]], size=v[2]) for v in videos]
    transcripts = [np.asarray(a, np.int64) for a in transcripts]
    if with_endpen and not ties:
        # the twin on the expanded lattice is the alignment only while scores stay far from its -1e9 fill: the transcript's
        # last class is an allowed end
        for i, a in enumerate(transcripts):
            h['endpen'][i, a[-1]] = 0.0
    batch = ops.Batch(lengths, cs, k_rows, c_max=cm, frame_offset=off, group=group, kp=kp, t_max=t_max, total_frames=total)
    return h, batch, transcripts


def _run(h, batch, transcripts):
    from action_segmentation_amd import ops
    out = ops.align(batch, _t(h['elp']), _t(h['trans']), _t(h['init']), _t(h['len']), transcripts,
                    endpen=None if h['endpen'] is None else _t(h['endpen']),
                    class_map=None if h['cmap'] is None else _t(h['cmap'], torch.int64))
    torch.cuda.synchronize()
    res = {k: _h(out[k]) for k in ('spans', 'labels', 'best', 'n_segs')}
    res['err'] = ops.error_flag(batch, out)
    return res


def _video_inputs(h, batch, i, a):
    g = int(batch.group[i]) if batch.group is not None else 0
    C, T, o = int(batch.n_states[g]), int(batch.lengths[i]), int(batch.frame_offset[i])
    kp = int(batch.kp[i]) if batch.kp is not None else min(batch.k_rows, batch.t_max)
    closing = 0.0 if h['endpen'] is None or not (0 <= a[-1] < C) else float(h['endpen'][i, a[-1]])
    return g, C, T, o, dict(elp=h['elp'][o:o + T, :C], a=a, trans=h['trans'][g, :C, :C], init=h['init'][g, :C],
                            len_scores=h['len'][g, :, :C], kp=kp, closing=closing)


def _check(h, batch, transcripts, twin=True, expect_err=0):
    """ops.align against align_ref on every video and against the twin on the videos that have an alignment."""
    res = _run(h, batch, transcripts)
    assert res['err'] == expect_err
    feasible = []
    for i, a in enumerate(transcripts):
        g, C, T, o, kw = _video_inputs(h, batch, i, a)
        best, starts = R.align_ref(**kw)
        gid = (lambda c: c) if h['cmap'] is None else (lambda c, g=g: int(h['cmap'][g, c]))
        assert res['best'][i] == best or (np.isnan(best) and np.isnan(res['best'][i])), (i, res['best'][i], best)
        assert np.array_equal(res['spans'][i], R.span_row(starts, a, T, batch.t_max, gid, gid(C))), i
        assert np.array_equal(res['labels'][o:o + T], R.frame_labels(starts, a, T, gid)), i
        assert res['n_segs'][i] == (0 if starts is None else len(a)), i
        feasible.append(starts is not None)
        if twin and starts is not None:
            v, tw = R.twin_align(**kw)
            assert res['best'][i] == v and starts == tw, (i, res['best'][i], v)
    covered = np.zeros(batch.total_frames, bool)
    for i in range(batch.b):
        covered[int(batch.frame_offset[i]):int(batch.frame_offset[i] + batch.lengths[i])] = True
    assert (res['labels'][~covered] == -1).all()
    return res, feasible


# ------------------------------------------------------------------------------------------------ 1. shapes
SHAPES = {
    # name: (videos [(T, kp, M, group)], states per group, c_max, k_rows)
    'M=1': ([(7, 9, 1, 0), (1, 9, 1, 0), (8, 9, 1, 0)], [3], 3, 9),
    'M=T': ([(11, 4, 11, 0), (1, 4, 1, 0), (30, 4, 30, 0)], [4], 4, 4),
    'kp=2': ([(9, 2, 9, 0), (2, 2, 2, 0)], [3], 3, 5),
    'every segment at the span limit': ([(24, 7, 4, 0), (6, 7, 1, 0), (60, 7, 10, 0)], [2], 2, 7),
    'infeasible beside feasible': ([(13, 7, 3, 0), (25, 7, 4, 0), (12, 7, 4, 0), (5, 7, 6, 0), (9, 7, 2, 0)], [3], 3, 7),
    'T around the tile, span limit below it': ([(P - 1, 40, 25, 0), (P, 40, 25, 0), (P + 1, 40, 30, 0), (2 * P + 3, 40, 45, 0)],
                                               [5], 5, 40),
    'T around the tile, span limit above it': ([(P - 1, 1024, 2, 0), (P, 1024, 1, 0), (P + 1, 1024, 3, 0), (2 * P + 3, 1024, 2, 0),
                                                (2 * P + 3, 1024, 7, 0)], [4], 4, 1024),
    'kp=1024, T=2100, M=3': ([(2100, 1024, 3, 0), (2046, 1024, 2, 0)], [6], 6, 1024),
    'M=256, T=300': ([(300, 6, 256, 0), (300, 3, 150, 0), (256, 9, 256, 0)], [7], 7, 9),
    'ragged, three groups': ([(50, 9, 8, 0), (120, 33, 5, 1), (33, 5, 11, 2), (77, 20, 9, 1), (5, 33, 2, 0), (64, 17, 4, 2)],
                             [3, 11, 6], 13, 33),
}


@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_bit_exact_against_the_reference_and_the_twin(name, ties):
    videos, cs, cm, k_rows = SHAPES[name]
    h, batch, tr = _make(sum(map(ord, name)) + ties, videos, cs, cm, k_rows, ties)
    res, feasible = _check(h, batch, tr)
    if name == 'infeasible beside feasible':
        assert feasible == [True, False, True, False, True]
        assert (res['best'][[1, 3]] == -np.inf).all() and (res['spans'][[1, 3]] == -1).all()
        # the neighbours alone: the same results
        keep = [0, 2, 4]
        h2 = dict(h, endpen=h['endpen'][keep])
        from action_segmentation_amd import ops
        b2 = ops.Batch(batch.lengths[keep], cs, k_rows, c_max=cm, frame_offset=batch.frame_offset[keep], group=batch.group[keep],
                       kp=batch.kp[keep], t_max=batch.t_max, total_frames=batch.total_frames)
        r2 = _run(h2, b2, [tr[i] for i in keep])
        assert r2['err'] == 0
        assert np.array_equal(r2['best'], res['best'][keep]) and np.array_equal(r2['spans'], res['spans'][keep])
        assert np.array_equal(r2['n_segs'], res['n_segs'][keep])
    else:
        assert all(feasible)


@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
def test_endpen_null_and_no_class_map(ties):
    videos, cs, cm, k_rows = SHAPES['ragged, three groups']
    h, batch, tr = _make(71 + ties, videos, cs, cm, k_rows, ties, with_endpen=False, with_cmap=False, gaps=False)
    _check(h, batch, tr)


@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
def test_the_same_class_three_times_in_a_row(ties):
    videos = [(40, 9, 7, 0), (23, 9, 3, 0)]
    h, batch, tr = _make(5 + ties, videos, [4], 4, 9, ties, transcripts=[[2, 1, 1, 1, 3, 3, 0], [0, 0, 0]])
    res, _ = _check(h, batch, tr)
    assert (res['n_segs'] == [7, 3]).all()
    row = res['spans'][1]
    assert (row[:23] >= 0).sum() == 3                                  # three starts of one class


@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
def test_forbidden_transitions_on_the_transcript_are_finite_scores(ties):
    videos = [(30, 9, 5, 0), (18, 9, 4, 0)]
    h, batch, tr = _make(31 + ties, videos, [4], 4, 9, ties, transcripts=[[0, 1, 2, 1, 3], [3, 2, 2, 0]])
    h['trans'][0, 1, 0] = h['trans'][0, 1, 2] = h['trans'][0, 2, 2] = BIG_NEG
    res, _ = _check(h, batch, tr, twin=False)      # (the twin's own -1e9 fill competes at that level: align_ref is the authority)
    assert np.isfinite(res['best']).all() and (res['best'] < -0.9e9).all()


# ------------------------------------------------------------------------------------------------ 2. brute force
@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
def test_against_every_composition_of_small_videos(ties):
    """T <= 9: the best of every composition of T into M parts of 1 .. kp - 1.  Integer inputs: every score is exact in any
    order, so best is equal and the returned boundaries attain it.  Real inputs: a score is a sum of at most 2 T + 2 M + 2 terms
    of magnitude < 20, so two orders of summation differ by less than 40 * 2^-53 * 40 * 20 < 4e-12."""
    videos = [(T, kp, M, 0) for T in (1, 4, 7, 9) for kp in (3, 5, 10) for M in (1, 2, 3, 5) if M <= T <= M * (kp - 1)]
    h, batch, tr = _make(11 + ties, videos, [3], 3, 10, ties, with_endpen=ties)   # (real: no -1e9 closing term in the sums)
    res, _ = _check(h, batch, tr, twin=False)
    for i, a in enumerate(tr):
        g, C, T, o, kw = _video_inputs(h, batch, i, a)
        want, arg = R.brute_force(**kw)
        starts = [int(p) for p in np.flatnonzero(res['spans'][i][:T] >= 0)]
        bounds = starts + [T]
        sc = kw['init'][a[0]] + kw['closing'] + sum(
            kw['elp'][bounds[m]:bounds[m + 1], a[m]].sum() + kw['len_scores'][bounds[m + 1] - bounds[m], a[m]]
            + (kw['trans'][a[m], a[m - 1]] if m else 0.0) for m in range(len(a)))
        if ties:
            assert res['best'][i] == want == sc, (i, res['best'][i], want, sc)
        else:
            assert abs(res['best'][i] - want) < 4e-12 and abs(sc - want) < 4e-12, (i, res['best'][i], want, sc)


# ------------------------------------------------------------------------------------------------ 3. Viterbi
def _cfg2_like(seed, b=12, T=512, C=16, K=256):
    """A cfg2-shaped batch (16 states, K = 256, one group) cut to T = 512: block-structured real-valued emissions."""
    from action_segmentation_amd import ops
    rng = np.random.default_rng(seed)
    elp = rng.normal(size=(b * T, C))
    for i in range(b):
        t = 0
        while t < T:
            n = int(rng.integers(10, 120))
            elp[i * T + t:i * T + min(T, t + n), int(rng.integers(0, C))] += 2.5
            t += n
    # (a transition costs about 20: the Viterbi paths have tens of segments, not one per frame)
    h = dict(elp=elp, trans=rng.normal(size=(1, C, C)) - 20.0, init=rng.normal(size=(1, C)),
             len=-0.02 * np.abs(np.arange(K)[None, :, None] - 60.0) + 0.1 * rng.normal(size=(1, K, C)),
             endpen=np.where(rng.random((b, C)) < 0.3, BIG_NEG, 0.0), cmap=None)
    batch = ops.Batch(np.full(b, T, np.int64), [C], K, c_max=C, t_max=T, total_frames=b * T)
    return h, batch


@pytest.fixture(scope='module')
def viterbi_case():
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts
    h, batch = _cfg2_like(2026)
    dev = {k: _t(h[k]) for k in ('elp', 'trans', 'init', 'len', 'endpen')}
    vit = ops.viterbi(batch, dev['elp'], dev['trans'], dev['init'], dev['len'], endpen=dev['endpen'])
    torch.cuda.synchronize()
    assert ops.error_flag(batch, vit) == 0
    vit = {k: _h(vit[k]) for k in ('spans', 'labels', 'best', 'n_segs')}
    tr = spans_to_transcripts(vit['spans'], batch.lengths)
    assert all(1 <= len(a) <= 256 for a in tr)
    return h, batch, vit, tr


def test_the_viterbi_paths_transcript_reproduces_the_viterbi_decode(viterbi_case):
    h, batch, vit, tr = viterbi_case
    res = _run(h, batch, tr)
    assert res['err'] == 0
    assert np.array_equal(res['best'], vit['best'])
    assert np.array_equal(res['spans'], vit['spans'])
    assert np.array_equal(res['labels'], vit['labels'])
    # (smm_viterbi_f64 counts the EOS entry among its segments or not: compare with the transcript's length)
    assert np.array_equal(res['n_segs'], [len(a) for a in tr])


def test_no_other_transcript_beats_viterbi(viterbi_case):
    h, batch, vit, tr = viterbi_case
    rng = np.random.default_rng(8)
    for trial in range(3):
        other = []
        for a in tr:
            a = a.copy()
            if trial == 0:
                a[int(rng.integers(0, len(a)))] = int(rng.integers(0, 16))
            elif trial == 1:
                a = np.concatenate([a, [int(rng.integers(0, 16))]])
            else:
                a = rng.integers(0, 16, size=int(rng.integers(3, 40)))
            other.append(a)
        res = _run(h, batch, other)
        assert res['err'] == 0
        assert (res['best'] <= vit['best']).all()


# ------------------------------------------------------------------------------------------------ 4. layers
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


def test_call_paths_agree():
    """ops.align = SemiMarkovModule.align = align_packed = SemiMarkovModel.align on one small corpus, with the transcripts of
    its Viterbi decode -- which they all reproduce."""
    from action_segmentation_amd import ops
    from action_segmentation_amd.batching import make_data_loader
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts, spans_to_labels
    data, model = _tiny_model()
    pc = model.prepare(data)
    t = pc.tables
    elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
    out = ops.viterbi(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    assert ops.error_flag(pc.batch, out) == 0
    vlab = _h(out['labels'])
    pred = {name: vlab[off:off + n] for name, off, n in zip(pc.video_names, pc.frame_offset, pc.lengths)}
    tr = spans_to_transcripts(out['spans'], pc.lengths)
    by_video = dict(zip(pc.video_names, tr))
    # the model
    got = model.align(data, by_video)
    assert sorted(got) == sorted(pred)
    for k in pred:
        assert np.array_equal(got[k], pred[k]), k
    # the packed corpus
    labels, best = model.model.align_packed(pc, tr)
    labels, best = _h(labels), _h(best)
    assert np.array_equal(best, _h(out['best']))
    for name, off, nf in zip(pc.video_names, pc.frame_offset, pc.lengths):
        assert np.array_equal(labels[off:off + nf], pred[name]), name
    # ops, with local ids
    cmap = _h(t['class_map'])
    group = pc.batch.group if pc.batch.group is not None else np.zeros(pc.batch.b, np.int64)
    local = [[list(cmap[group[i], :pc.batch.n_states[group[i]]]).index(c) for c in a] for i, a in enumerate(tr)]
    o2 = ops.align(pc.batch, elp, t['trans'], t['init'], t['len'], local, endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    assert ops.error_flag(pc.batch, o2) == 0
    assert np.array_equal(_h(o2['labels']), labels) and np.array_equal(_h(o2['best']), best)
    assert np.array_equal(_h(o2['n_segs']), [len(a) for a in tr])
    # per batch, padded
    pos = {name: j for j, name in enumerate(pc.video_names)}
    cons_fn = model._test_constraints(data)
    n = 0
    for batch in make_data_loader(model.args, data, shuffle=False, batch_by_task=True, batch_size=model.args.batch_size):
        feats, lengths = batch['features'].to(DEV), batch['lengths']
        addl = model.make_additional_allowed_ends(batch['task_name'], lengths)
        spans, sc = model.model.align(feats, lengths, batch['task_indices'], [by_video[v] for v in batch['video_name']],
                                      additional_allowed_ends_per_instance=addl,
                                      constraints=cons_fn(batch) if cons_fn else None)
        lab = model.model.trim(spans_to_labels(spans), lengths, check_eos=True)
        for i, name in enumerate(batch['video_name']):
            assert np.array_equal(lab[i].numpy(), pred[name]), name
            # (its own emission launch on the padded layout: the same arithmetic per frame)
            assert float(sc[i]) == best[pos[name]], name
            n += 1
    assert n == len(pc.video_names)
    # an id that is not valid for the video
    bad = dict(by_video)
    first = pc.video_names[0]
    bad[first] = np.concatenate([by_video[first], [model.model.n_classes + 3]])
    with pytest.raises(ValueError):
        model.align(data, bad)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_nan_in_one_video_sets_the_error_word():
    from action_segmentation_amd import _lib, ops
    videos = [(40, 9, 6, 0), (33, 9, 5, 0), (50, 9, 8, 0), (21, 9, 3, 0)]
    h, batch, tr = _make(21, videos, [5], 5, 9, False)
    clean, _ = _check(h, batch, tr)
    o = int(batch.frame_offset[2])
    h2 = dict(h, elp=h['elp'].copy())
    h2['elp'][o + 7, int(tr[2][0])] = np.nan
    res = _run(h2, batch, tr)
    assert res['err'] != 0
    assert np.isnan(res['best'][2]) and res['n_segs'][2] == 0 and (res['spans'][2] == -1).all()
    for k in ('best', 'spans', 'n_segs'):
        assert np.array_equal(res[k][[0, 1, 3]], clean[k][[0, 1, 3]]), k
    out = ops.align(batch, _t(h2['elp']), _t(h['trans']), _t(h['init']), _t(h['len']), tr)
    torch.cuda.synchronize()
    with pytest.raises(_lib.SmmError):
        ops.check_decoded(batch, out)
    # the next call on clean inputs clears it
    assert _run(h, batch, tr)['err'] == 0


def test_an_id_out_of_range_is_an_infeasible_video():
    videos = [(40, 9, 6, 0), (33, 9, 5, 1), (50, 9, 8, 0)]
    h, batch, tr = _make(23, videos, [5, 3], 5, 9, False)
    clean, _ = _check(h, batch, tr)
    for bad_id in (3, 5, 1 << 20, -1):                                  # (3: a state of group 0, not of video 1's group)
        tr2 = [tr[0], tr[1].copy(), tr[2]]
        tr2[1][2] = bad_id
        res, feasible = _check(h, batch, tr2)
        assert feasible == [True, False, True] and res['best'][1] == -np.inf and res['n_segs'][1] == 0
        for k in ('best', 'spans', 'n_segs'):
            assert np.array_equal(res[k][[0, 2]], clean[k][[0, 2]]), k


def test_an_alignment_call_leaves_the_viterbi_path_alone():
    """smm_workspace_bytes and an ops.viterbi call made afterwards do not depend on whether an alignment ran before."""
    from action_segmentation_amd import ops
    videos = [(90, 17, 8, 0), (64, 17, 6, 0), (120, 17, 9, 0)]
    h, batch, tr = _make(29, videos, [6], 6, 17, False)
    dev = {k: _t(h[k]) for k in ('elp', 'trans', 'init', 'len', 'endpen')}
    need = batch.workspace_bytes()
    before = ops.viterbi(batch, dev['elp'], dev['trans'], dev['init'], dev['len'], endpen=dev['endpen'])
    torch.cuda.synchronize()
    before = {k: _h(before[k]) for k in ('spans', 'labels', 'best', 'n_segs')}
    _check(h, batch, tr)
    assert batch.workspace_bytes() == need
    after = ops.viterbi(batch, dev['elp'], dev['trans'], dev['init'], dev['len'], endpen=dev['endpen'])
    torch.cuda.synchronize()
    assert ops.error_flag(batch, after) == 0
    for k in before:
        assert np.array_equal(_h(after[k]), before[k]), k


# ------------------------------------------------------------------------------------------------ 6. the table detectors
@pytest.mark.parametrize('where', ['init', 'trans', 'len', 'endpen'])
@pytest.mark.parametrize('value', [np.nan, np.inf], ids=['nan', 'inf'])
def test_a_nan_or_inf_in_a_table_entry_the_transcript_reads_sets_the_error_word(where, value):
    """The DP's max drops a NaN, so each table the transcript reads has a detector of its own (include/smmdp.h).  One group
    per video: only the video whose group's table is poisoned fails; the others are unchanged."""
    videos = [(40, 9, 6, 0), (33, 9, 5, 1), (50, 9, 8, 2)]
    h, batch, tr = _make(41, videos, [5, 5, 5], 5, 9, False)
    clean, _ = _check(h, batch, tr)
    a = tr[1]
    h2 = {k: (None if v is None else v.copy()) for k, v in h.items()}
    if where == 'init':
        h2['init'][1, a[0]] = value
    elif where == 'trans':
        h2['trans'][1, a[3], a[2]] = value
    elif where == 'len':
        h2['len'][1, 4, a[2]] = value
    else:
        h2['endpen'][1, a[-1]] = value
    res = _run(h2, batch, tr)
    assert res['err'] != 0
    assert np.isnan(res['best'][1]) and res['n_segs'][1] == 0 and (res['spans'][1] == -1).all()
    o = int(batch.frame_offset[1])
    assert (res['labels'][o:o + 33] == -1).all()
    if np.isnan(value):
        g, C, T, o, kw = _video_inputs(h2, batch, 1, a)
        best, starts = R.align_ref(**kw)
        assert np.isnan(best) and starts is None
    for k in ('best', 'spans', 'n_segs'):
        assert np.array_equal(res[k][[0, 2]], clean[k][[0, 2]]), k
    # an entry the transcript does not read changes nothing
    h3 = {k: (None if v is None else v.copy()) for k, v in h.items()}
    h3["len"][1, 0, :] = value                                          # row 0 is no segment length
    res = _run(h3, batch, tr)
    assert res['err'] == 0
    for k in ('best', 'spans', 'n_segs'):
        assert np.array_equal(res[k], clean[k]), k


# ------------------------------------------------------------------------------------------------ 7. smm_viterbi_f64, expanded
@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
def test_equals_smm_viterbi_f64_on_the_expanded_lattice(ties):
    """Transcripts of at most 32 entries: smm_viterbi_f64 on the lattice whose states are the transcript positions (one
    parameter group per video) returns the same best and the same boundaries."""
    from action_segmentation_amd import ops
    videos, cs, cm, k_rows = SHAPES['ragged, three groups']
    videos = videos + [(700, 33, 32, 1), (90, 9, 31, 0)]
    h, batch, tr = _make(91 + ties, videos, cs, cm, k_rows, ties)
    res, feasible = _check(h, batch, tr, twin=False)
    assert all(feasible)
    b = len(videos)
    ms = np.array([len(a) for a in tr], np.int32)
    M = int(ms.max())
    assert M == 32
    lengths = batch.lengths
    off = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    e2 = np.zeros((int(lengths.sum()), M))
    t2, i2, l2, p2 = np.full((b, M, M), BIG_NEG), np.full((b, M), BIG_NEG), np.zeros((b, k_rows, M)), np.full((b, M), BIG_NEG)
    for i, a in enumerate(tr):
        g, C, T, o, kw = _video_inputs(h, batch, i, a)
        ee, tt, ii, ll, pp = R.expanded_lattice(kw['elp'], a, kw['trans'], kw['init'], h['len'][g, :, :C], k_rows, kw['closing'])
        m = len(a)
        e2[off[i]:off[i] + T, :m], t2[i, :m, :m], i2[i, :m], l2[i, :, :m], p2[i, :m] = ee, tt, ii, ll, pp
    bl = ops.Batch(lengths, ms, k_rows, c_max=M, frame_offset=off, group=np.arange(b, dtype=np.int32), kp=batch.kp,
                   t_max=batch.t_max, total_frames=int(lengths.sum()))
    vit = ops.viterbi(bl, _t(e2), _t(t2), _t(i2), _t(l2), endpen=_t(p2))
    torch.cuda.synchronize()
    assert ops.error_flag(bl, vit) == 0
    assert np.array_equal(_h(vit['best']), res['best'])
    sp = _h(vit['spans'])
    for i, a in enumerate(tr):
        T = int(lengths[i])
        pos = np.flatnonzero(sp[i, :T] >= 0)
        assert np.array_equal(sp[i, pos], np.arange(len(a))) and sp[i, T] == len(a), i      # position m at segment m's start, EOS
        assert np.array_equal(pos, np.flatnonzero(res['spans'][i, :T] >= 0)), i
