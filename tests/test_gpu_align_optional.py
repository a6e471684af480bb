"""Forced alignment with optional transcript entries (smm_align_opt_f64 / ops.align_optional / SemiMarkovModule.align,
align_packed / SemiMarkovModel.align) on the GPU.

spans, labels, best, n_segs and used are compared bit for bit with tests/align_optional_ref.py (the definition in numpy) on
every video and, on videos that have an alignment, with the C twin's Viterbi on the lattice whose states are the transcript
positions -- on real-valued inputs and on small-integer inputs, where many alignments tie exactly and the back-trace's tie
rule decides.  endpen is NULL or small integers, so no allowed end sits at the twin's -1e9."""
import numpy as np
import pytest
import torch

import align_optional_ref as O
import test_gpu_align as A

pytestmark = pytest.mark.gpu
P = A.P
_t, _h = A._t, A._h


def _flags(s):
    return np.array([ch == '1' for ch in s])


def _alt(M, first=True):
    """alternating, starting with an optional entry: "bg, step, bg, ..." """
    return np.array([(m % 2 == 0) == first for m in range(M)])


def _make(seed, videos, cs, cm, k_rows, ties, flags, with_endpen=True, **kw):
    """videos: [(T, kp, M, group)], flags: one boolean array per video.  endpen: small integers or None."""
    h, batch, tr = A._make(seed, videos, cs, cm, k_rows, ties, with_endpen=False, **kw)
    if with_endpen:
        h['endpen'] = np.random.default_rng(seed + 1000).integers(-3, 4, size=(len(videos), cm)).astype(np.float64)
    assert all(len(f) == len(a) for f, a in zip(flags, tr))
    return h, batch, tr, [np.asarray(f, bool) for f in flags]


def _run(h, batch, tr, flags):
    from action_segmentation_amd import ops
    out = ops.align_optional(batch, _t(h['elp']), _t(h['trans']), _t(h['init']), _t(h['len']), tr, flags,
                             endpen=None if h['endpen'] is None else _t(h['endpen']),
                             class_map=None if h['cmap'] is None else _t(h['cmap'], torch.int64), want_used=True)
    torch.cuda.synchronize()
    res = {k: _h(out[k]) for k in ('spans', 'labels', 'best', 'n_segs')}
    res['used'] = [_h(u) for u in out['used']]
    res['err'] = ops.error_flag(batch, out)
    return res


def _video_inputs(h, batch, i, a, opt):
    g = int(batch.group[i]) if batch.group is not None else 0
    C, T, o = int(batch.n_states[g]), int(batch.lengths[i]), int(batch.frame_offset[i])
    kp = int(batch.kp[i]) if batch.kp is not None else min(batch.k_rows, batch.t_max)
    return g, C, T, o, dict(elp=h['elp'][o:o + T, :C], a=a, opt=opt, trans=h['trans'][g, :C, :C], init=h['init'][g, :C],
                            len_scores=h['len'][g, :, :C], kp=kp, endpen=None if h['endpen'] is None else h['endpen'][i, :C])


def _check(h, batch, tr, flags, twin=True, expect_err=0, res=None):
    """ops.align_optional against the reference on every video and against the twin on those that have an alignment."""
    res = res or _run(h, batch, tr, flags)
    assert (res['err'] != 0) == bool(expect_err)
    feasible = []
    for i, (a, opt) in enumerate(zip(tr, flags)):
        g, C, T, o, kw = _video_inputs(h, batch, i, a, opt)
        best, segs = O.align_optional_ref(**kw)
        gid = (lambda c: c) if h['cmap'] is None else (lambda c, g=g: int(h['cmap'][g, c]))
        assert res['best'][i] == best or (np.isnan(best) and np.isnan(res['best'][i])), (i, res['best'][i], best)
        assert np.array_equal(res['spans'][i], O.span_row(segs, a, T, batch.t_max, gid, gid(C))), i
        assert np.array_equal(res['labels'][o:o + T], O.frame_labels(segs, a, T, gid)), i
        assert res['n_segs'][i] == (0 if segs is None else len(segs)), i
        assert np.array_equal(res['used'][i], O.used_flags(segs, len(a))), i
        feasible.append(segs is not None)
        if twin and segs is not None:
            v, tw = O.twin_align(**kw)
            assert res['best'][i] == v and segs == tw, (i, res['best'][i], v)
    return res, feasible


def _skipped_and_taken(res, flags):
    u, f = np.concatenate(res['used']), np.concatenate(flags)
    return int((u[f] == 0).sum()), int((u[f] == 1).sum())


# ------------------------------------------------------------------------------------------------ 1. shapes
def _ragged_flags():
    rng = np.random.default_rng(404)
    return [rng.random(v[2]) < 0.4 for v in A.SHAPES['ragged, three groups'][0]]


SHAPES = {
    # name: (videos [(T, kp, M, group)], flags per video, states per group, c_max, k_rows)
    'alternating': ([(60, 9, 11, 0), (9, 9, 11, 0), (5, 9, 11, 0)], [_alt(11)] * 3, [4], 4, 9),
    'all optional': ([(30, 6, 12, 0), (1, 6, 12, 0), (60, 6, 12, 0)], [np.ones(12, bool)] * 3, [4], 4, 6),
    'all mandatory': ([(40, 9, 7, 0)], [np.zeros(7, bool)], [4], 4, 9),
    'runs of three at both ends': ([(50, 9, 10, 0)], [_flags('1110010111')], [4], 4, 9),
    'the optional entries are needed': ([(13, 7, 3, 0)], [_flags('101')], [3], 3, 7),
    'no room for the optional entries': ([(2, 7, 5, 0)], [_flags('10101')], [3], 3, 7),
    'T around the tile, span limit below it': ([(P - 1, 40, 25, 0), (P, 40, 25, 0), (P + 1, 40, 45, 0), (2 * P + 3, 40, 45, 0)],
                                               [_alt(25), _alt(25), _alt(45), _alt(45)], [5], 5, 40),
    'kp=1024': ([(P + 1, 1024, 3, 0), (2 * P + 3, 1024, 7, 0), (2100, 1024, 5, 0)], [_alt(3), _alt(7), _alt(5)], [4], 4, 1024),
    'M=256': ([(300, 6, 256, 0), (300, 3, 256, 0), (256, 9, 256, 0)],
              [_alt(256), np.ones(256, bool), np.arange(256) >= 128], [7], 7, 9),
    'infeasible beside feasible': ([(13, 7, 3, 0), (5, 7, 8, 0), (12, 7, 4, 0), (25, 7, 4, 0), (9, 7, 2, 0)],
                                   [_flags('010'), _flags('00000011'), _flags('0101'), _flags('1010'), _flags('01')], [3], 3, 7),
    'ragged, three groups': (A.SHAPES['ragged, three groups'][0], _ragged_flags()) + A.SHAPES['ragged, three groups'][1:],
}
MIXED = ('alternating', 'all optional', 'M=256')
_seen = {}


@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
@pytest.mark.parametrize('name', list(SHAPES))
def test_bit_exact_against_the_reference_and_the_twin(name, ties):
    videos, flags, cs, cm, k_rows = SHAPES[name]
    h, batch, tr, flags = _make(sum(map(ord, name)) + ties, videos, cs, cm, k_rows, ties, flags)
    res, feasible = _check(h, batch, tr, flags)
    if name in MIXED:
        _seen[name, ties] = _skipped_and_taken(res, flags)
    if name == 'infeasible beside feasible':
        assert feasible == [True, False, True, False, True]
        assert (res['best'][[1, 3]] == -np.inf).all() and (res['spans'][[1, 3]] == -1).all()
        assert not res['used'][1].any() and not res['used'][3].any()
        # the neighbours alone: the same results
        from action_segmentation_amd import ops
        keep = [0, 2, 4]
        b2 = ops.Batch(batch.lengths[keep], cs, k_rows, c_max=cm, frame_offset=batch.frame_offset[keep], group=batch.group[keep],
                       kp=batch.kp[keep], t_max=batch.t_max, total_frames=batch.total_frames)
        r2 = _run(dict(h, endpen=h['endpen'][keep]), b2, [tr[i] for i in keep], [flags[i] for i in keep])
        assert r2['err'] == 0
        for k in ('best', 'spans', 'n_segs'):
            assert np.array_equal(r2[k], res[k][keep]), k
        assert all(np.array_equal(r2['used'][j], res['used'][i]) for j, i in enumerate(keep))
        cover = np.zeros(batch.total_frames, bool)
        for i in keep:
            cover[int(batch.frame_offset[i]):int(batch.frame_offset[i] + batch.lengths[i])] = True
        assert np.array_equal(r2['labels'][cover], res['labels'][cover]) and (r2['labels'][~cover] == -1).all()
    else:
        assert all(feasible)
    if name == 'all mandatory':
        plain = A._run(h, batch, tr)
        assert plain['err'] == 0
        for k in ('best', 'spans', 'labels', 'n_segs'):
            assert np.array_equal(plain[k], res[k]), k
        assert res['used'][0].all()
    if name == 'alternating':
        assert np.array_equal(res['used'][2], ~flags[2])               # T = 5: only the mandatory entries fit
    if name == 'the optional entries are needed':
        assert res['used'][0].all()
    if name == 'no room for the optional entries':
        assert np.array_equal(res['used'][0], ~flags[0])


def test_some_optional_entries_are_skipped_and_some_are_taken():
    """... over the alternating, all-optional and M = 256 shapes (the results of the test above, computed here when it did not
    run)."""
    for name in MIXED:
        for ties in (False, True):
            if (name, ties) not in _seen:
                videos, flags, cs, cm, k_rows = SHAPES[name]
                h, batch, tr, flags = _make(sum(map(ord, name)) + ties, videos, cs, cm, k_rows, ties, flags)
                _seen[name, ties] = _skipped_and_taken(_run(h, batch, tr, flags), flags)
            skipped, taken = _seen[name, ties]
            assert skipped > 0 and taken > 0, (name, ties, skipped, taken)


@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
def test_endpen_null_and_no_class_map(ties):
    videos, flags, cs, cm, k_rows = SHAPES['ragged, three groups']
    h, batch, tr, flags = _make(71 + ties, videos, cs, cm, k_rows, ties, flags, with_endpen=False, with_cmap=False, gaps=False)
    _check(h, batch, tr, flags)


@pytest.mark.parametrize('ties', [False, True], ids=['real', 'ties'])
def test_one_class_optional_twice_in_a_row_and_repeated_across_a_skipped_entry(ties):
    videos = [(40, 9, 7, 0), (23, 9, 5, 0), (6, 4, 3, 0)]
    tr = [[2, 1, 1, 1, 3, 3, 0], [0, 2, 0, 2, 0], [1, 0, 1]]
    flags = [_flags('0110110'), _flags('01010'), _flags('010')]
    h, batch, tr, flags = _make(5 + ties, videos, [4], 4, 9, ties, flags, transcripts=tr)
    _check(h, batch, tr, flags)
    # the third video: the entry between the two 1s is skipped when it is made too expensive
    h['elp'][int(batch.frame_offset[2]):int(batch.frame_offset[2]) + 6, 0] = -50.0
    res, _ = _check(h, batch, tr, flags)
    assert list(res['used'][2]) == [1, 0, 1] and res['n_segs'][2] == 2


def test_two_calls_give_the_same_bits():
    videos, flags, cs, cm, k_rows = SHAPES['T around the tile, span limit below it']
    h, batch, tr, flags = _make(3, videos, cs, cm, k_rows, False, flags)
    r1, r2 = _run(h, batch, tr, flags), _run(h, batch, tr, flags)
    for k in ('best', 'spans', 'labels', 'n_segs'):
        assert np.array_equal(r1[k], r2[k]), k
    assert all(np.array_equal(x, y) for x, y in zip(r1['used'], r2['used']))


def test_captures_into_a_graph_and_replays_bit_exactly():
    """tests/test_gpu_graph.py's pattern: eager, a warm-up on a side stream, one capture, one replay into overwritten outputs.
    The ids and flags are on the device from the eager call (``staged``), so the captured call copies nothing from the host;
    one stream, so the graph has no parallel branches."""
    from action_segmentation_amd import ops
    videos, flags, cs, cm, k_rows = SHAPES['T around the tile, span limit below it']
    h, batch, tr, flags = _make(17, videos, cs, cm, k_rows, False, flags)
    tabs = (_t(h['elp']), _t(h['trans']), _t(h['init']), _t(h['len']))
    endpen, cmap = _t(h['endpen']), _t(h['cmap'], torch.int64)
    ws = torch.empty(ops.align_opt_workspace_bytes(batch, ops._transcript_arrays(batch, tr)[1]), dtype=torch.uint8, device=A.DEV)

    def call(staged=None):
        return ops.align_optional(batch, *tabs, tr, flags, endpen=endpen, class_map=cmap, ws=ws, want_used=True, staged=staged)

    eager = call()
    torch.cuda.synchronize()
    assert ops.error_flag(batch, eager) == 0
    keys = ('spans', 'labels', 'best', 'n_segs')
    ref = {k: eager[k].clone() for k in keys}
    ref_used = [u.clone() for u in eager['used']]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(eager['_staged'])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(eager['_staged'])
    for k in keys:
        out[k].fill_(-9)
    for u in out['used']:
        u.fill_(-9)
    graph.replay()
    torch.cuda.synchronize()
    assert out['_err'].tolist()[0] == 0
    for k in keys:
        assert torch.equal(out[k], ref[k]), k
    assert all(torch.equal(u, v) for u, v in zip(out['used'], ref_used))


# ------------------------------------------------------------------------------------------------ 2. errors
def test_a_nan_in_elp_sets_the_error_word_and_leaves_the_other_videos():
    videos = [(40, 9, 6, 0), (33, 9, 5, 0), (50, 9, 8, 0), (21, 9, 3, 0)]
    flags = [_alt(6), _alt(5), _alt(8), _alt(3)]
    h, batch, tr, flags = _make(21, videos, [5], 5, 9, False, flags)
    clean, _ = _check(h, batch, tr, flags)
    h2 = dict(h, elp=h['elp'].copy())
    h2['elp'][int(batch.frame_offset[2]) + 7, int(tr[2][0])] = np.nan
    res = _run(h2, batch, tr, flags)
    assert res['err'] != 0
    assert np.isnan(res['best'][2]) and res['n_segs'][2] == 0 and (res['spans'][2] == -1).all() and not res['used'][2].any()
    _check(h2, batch, tr, flags, twin=False, expect_err=1, res=res)
    for k in ('best', 'spans', 'n_segs'):
        assert np.array_equal(res[k][[0, 1, 3]], clean[k][[0, 1, 3]]), k
    assert _run(h, batch, tr, flags)['err'] == 0                       # the next call on clean inputs clears it


def test_an_inf_in_a_transition_only_a_skipping_pair_reads():
    """trans[a_2][a_0] is read because entry 1 may be left out; trans[a_3][a_0] is read by no pair (entry 2 is mandatory)."""
    videos = [(30, 9, 4, 0), (30, 9, 4, 1)]
    tr = [[0, 1, 2, 3], [0, 1, 2, 3]]
    flags = [_flags('0100'), _flags('0100')]
    h, batch, tr, flags = _make(43, videos, [4, 4], 4, 9, False, flags, transcripts=tr)
    clean, _ = _check(h, batch, tr, flags)
    h2 = dict(h, trans=h['trans'].copy())
    h2['trans'][1, 3, 0] = np.inf
    res, _ = _check(h2, batch, tr, flags)
    for k in ('best', 'spans', 'n_segs'):
        assert np.array_equal(res[k], clean[k]), k
    h2['trans'][1, 2, 0] = np.inf
    res = _run(h2, batch, tr, flags)
    assert res['err'] != 0 and np.isnan(res['best'][1]) and res['n_segs'][1] == 0 and (res['spans'][1] == -1).all()
    assert res['best'][0] == clean['best'][0] and np.array_equal(res['spans'][0], clean['spans'][0])
    _check(h2, batch, tr, flags, twin=False, expect_err=1, res=res)


# ------------------------------------------------------------------------------------------------ 3. smm_viterbi_f64, expanded
def test_equals_smm_viterbi_f64_on_the_expanded_lattice():
    """One cfg2-like launch; the transcript is each video's own Viterbi transcript with an optional entry of a random class
    inserted after every entry, kept to the videos where that stays within smm_viterbi_f64's 32 states."""
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts
    h, batch = A._cfg2_like(2026)
    h['endpen'] = np.random.default_rng(6).integers(-3, 4, size=h['endpen'].shape).astype(np.float64)
    dev = {k: _t(h[k]) for k in ('elp', 'trans', 'init', 'len', 'endpen')}
    vit = ops.viterbi(batch, dev['elp'], dev['trans'], dev['init'], dev['len'], endpen=dev['endpen'])
    torch.cuda.synchronize()
    rng = np.random.default_rng(9)
    b, T, K = batch.b, int(batch.lengths[0]), batch.k_rows
    tr, flags = [], []
    for a in spans_to_transcripts(_h(vit['spans']), batch.lengths):
        a = a[:16]                                                      # (a prefix of the path is a transcript as well)
        x = np.empty(2 * len(a), np.int64)
        x[0::2], x[1::2] = a, rng.integers(0, 16, size=len(a))
        tr.append(x)
        flags.append(np.arange(len(x)) % 2 == 1)
    res = _run(h, batch, tr, flags)
    assert res['err'] == 0 and np.isfinite(res['best']).all()
    ms = np.array([len(a) for a in tr], np.int32)
    M = int(ms.max())
    assert M <= 32
    e2 = np.zeros((b * T, M))
    t2, i2, l2, p2 = np.full((b, M, M), A.BIG_NEG), np.full((b, M), A.BIG_NEG), np.zeros((b, K, M)), np.full((b, M), A.BIG_NEG)
    for i, (a, opt) in enumerate(zip(tr, flags)):
        g, C, _, o, kw = _video_inputs(h, batch, i, a, opt)
        kw['kp'] = K
        ee, tt, ii, ll, pp = O.expanded_lattice(**kw)
        m = len(a)
        e2[i * T:(i + 1) * T, :m], t2[i, :m, :m], i2[i, :m], l2[i, :, :m], p2[i, :m] = ee, tt, ii, ll, pp
    bl = ops.Batch(batch.lengths, ms, K, c_max=M, group=np.arange(b, dtype=np.int32), t_max=T, total_frames=b * T)
    v2 = ops.viterbi(bl, _t(e2), _t(t2), _t(i2), _t(l2), endpen=_t(p2))
    torch.cuda.synchronize()
    assert ops.error_flag(bl, v2) == 0
    assert np.array_equal(_h(v2['best']), res['best'])
    sp = _h(v2['spans'])
    for i, a in enumerate(tr):
        pos = np.flatnonzero(sp[i, :T] >= 0)
        assert np.array_equal(pos, np.flatnonzero(res['spans'][i, :T] >= 0)), i
        assert np.array_equal(np.flatnonzero(res['used'][i]), sp[i, pos]), i          # the states are the entries


# ------------------------------------------------------------------------------------------------ 4. layers
def test_call_paths_agree():
    """SemiMarkovModule.align / align_packed with flags = ops.align_optional; SemiMarkovModel.align(optional_classes) =
    optional_by_video built by hand; without either, today's align."""
    from action_segmentation_amd import ops
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts
    data, model = A._tiny_model()
    pc = model.prepare(data)
    t = pc.tables
    elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
    out = ops.viterbi(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    base = spans_to_transcripts(out['spans'], pc.lengths)
    cmap = _h(t['class_map'])
    group = pc.batch.group if pc.batch.group is not None else np.zeros(pc.batch.b, np.int64)
    rng = np.random.default_rng(1)
    tr, flags = [], []
    for i, a in enumerate(base):
        # an optional entry of a random valid class of the video in front of every entry
        valid = cmap[group[i], :pc.batch.n_states[group[i]]]
        x = np.empty(2 * len(a), np.int64)
        x[1::2], x[0::2] = a, rng.choice(valid, size=len(a))
        tr.append(x[:256])
        flags.append((np.arange(len(x)) % 2 == 0)[:256])
    local = [[list(cmap[group[i], :pc.batch.n_states[group[i]]]).index(c) for c in a] for i, a in enumerate(tr)]
    o2 = ops.align_optional(pc.batch, elp, t['trans'], t['init'], t['len'], local, flags, endpen=pc.endpen,
                            class_map=t['class_map'])
    torch.cuda.synchronize()
    assert ops.error_flag(pc.batch, o2) == 0 and o2['used'] is None
    labels, best = model.model.align_packed(pc, tr, optional=flags)
    assert np.array_equal(_h(labels), _h(o2['labels'])) and np.array_equal(_h(best), _h(o2['best']))
    assert (_h(best) >= _h(out['best'])).all()                          # (leaving every inserted entry out is the Viterbi path)
    with pytest.raises(ValueError):
        model.model.align_packed(pc, tr, optional=flags[:-1])
    # the model: flags per video, and by class
    by_video, opt_by_video = dict(zip(pc.video_names, tr)), dict(zip(pc.video_names, flags))
    got = model.align(data, by_video, optional_by_video=opt_by_video)
    lab = _h(o2['labels'])
    for name, off, n in zip(pc.video_names, pc.frame_offset, pc.lengths):
        assert np.array_equal(got[name], lab[off:off + n]), name
    classes = [int(c) for c in np.unique(np.concatenate(tr))[::2]]
    by_class = model.align(data, by_video, optional_classes=classes)
    by_hand = model.align(data, by_video, optional_by_video={k: np.isin(v, classes) for k, v in by_video.items()})
    plain = model.align(data, by_video)
    none = model.align(data, by_video, optional_classes=[])
    for name in pc.video_names:
        assert np.array_equal(by_class[name], by_hand[name]), name
        assert np.array_equal(plain[name], none[name]), name
    # per batch, padded
    from action_segmentation_amd.batching import make_data_loader
    from action_segmentation_amd.semimarkov_utils import spans_to_labels
    pos = {name: j for j, name in enumerate(pc.video_names)}
    cons_fn = model._test_constraints(data)
    for batch in make_data_loader(model.args, data, shuffle=False, batch_by_task=True, batch_size=model.args.batch_size):
        feats, lengths = batch['features'].to(A.DEV), batch['lengths']
        spans, sc = model.model.align(feats, lengths, batch['task_indices'], [by_video[v] for v in batch['video_name']],
                                      additional_allowed_ends_per_instance=model.make_additional_allowed_ends(
                                          batch['task_name'], lengths),
                                      constraints=cons_fn(batch) if cons_fn else None,
                                      optional=[opt_by_video[v] for v in batch['video_name']])
        lb = model.model.trim(spans_to_labels(spans), lengths, check_eos=True)
        for i, name in enumerate(batch['video_name']):
            assert np.array_equal(lb[i].numpy(), got[name]), name
            assert float(sc[i]) == _h(best)[pos[name]], name
