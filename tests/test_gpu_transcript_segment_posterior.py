"""Segment posteriors under a transcript graph (smm_align_graph_segment_posteriors_f64 / ops.align_graph_segment_posteriors /
SemiMarkovModule.alignment_segment_posteriors* / SemiMarkovModel.alignment_confidence) on the GPU, against
tests/transcript_segment_posterior_ref.py: (d) the brute force on the tiny graphs, (b) the forward-backward elsewhere.

Bars: probabilities -- exp of the log outputs, the dense E and S -- at rtol = atol = 2e-5, the family's bar for g_elp / p_used /
p_end; row sums of E against the backward call's p_used at the same bar.  Moments (mean and standard deviation of a node's end
and start position, in frames) are a ratio of sums for which the per-entry bar gives no bound: they were measured against the
reference's values from its own E and S on the nodes whose reference p_used >= 0.01 (each case asserts that at least 90 % of
its nodes pass that cut), and are asserted at 4 x the worst measured value, MOMENT_BAR below; the margin is for other seeds of
the same generators.  Every test prints its line, "[transcript-segment-posterior] ..."."""
import math

import numpy as np
import pytest
import torch

import transcript_segment_posterior_ref as TR
from test_gpu_transcript_graph import Case, _lists, _ops, _tables, _tuple

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
NEG_INF = float('-inf')
BAR = 2e-5
P_CUT = 0.01
# worst |mean - ref| and |sd - ref| in frames over every case below on an MI355X, 1.20e-07 (chain, M = 65): 4 x that
MOMENT_BAR = 4.8e-7


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref)
    worst = float(err.max()) if err.size else 0.0
    assert np.isfinite(got).all(), what
    assert (err <= BAR + BAR * np.abs(ref)).all(), (what, worst)
    return worst


def _run(case, spans=None, used=None, class_map=None, want_dense=True, sample=0, seed=3):
    """forward launch + the segment-posterior launch -> (numpy dict, the raw ops results).  ``sample`` > 0 and spans None: the
    sets are the best alignment followed by ``sample`` sampler draws."""
    ops = _ops()
    batch, d = case.device_inputs()
    tabs = (d['elp'], d['trans'], d['init'], d['len'])
    if spans is None:
        best = ops.align_graph(batch, *tabs, case.graphs, endpen=d['endpen'], class_map=class_map, want_labels=False, want_used=True)
        spans, used = best['spans'][None], torch.cat(best['used'])[None]
    z = ops.align_graph_logz(batch, *tabs, case.graphs, endpen=d['endpen'])
    if sample:
        smp = ops.align_graph_sample(batch, *tabs, case.graphs, z['logz'], sample, seed=seed, endpen=d['endpen'], class_map=class_map,
                                     ws=z['ws'], staged=z['_staged'], want_labels=False)
        spans = torch.cat([spans, smp['spans']])
        used = torch.cat([used, torch.cat(smp['used'], dim=1)])
    out = ops.align_graph_segment_posteriors(batch, *tabs, case.graphs, z['logz'], spans=spans, used=used, endpen=d['endpen'],
                                             class_map=class_map, ws=z['ws'], staged=z['_staged'], want_dense=want_dense)
    torch.cuda.synchronize()
    n = lambda t: None if t is None else t.cpu().numpy()
    res = dict(seg=n(out['seg_logp']), node=[n(t) for t in out['node_logp']], spans=n(spans), used=n(used), logz=n(z['logz']),
               E=n(out['node_end_post']), S=n(out['node_start_post']), err=ops.error_flag(batch, out))
    for key in ('end_mean', 'end_sd', 'start_mean', 'start_sd'):
        res[key] = [n(t) for t in out[key]]
    return res, (batch, d, z, out)


def _refs(case, fast=True, brute=False):
    out = []
    for i, (e, gr, j) in enumerate(case.vids):
        t = case.tabs[j]
        fn = TR.brute_force if brute else (lambda *a: TR.from_forward_backward(*a, fast=fast))
        out.append(fn(e, _tuple(gr), t['trans'], t['init'], t['len'], case.kp(i), case.ep(i)))
    return out


def _check(case, res, refs, what, class_of=None):
    """Everything the call returned against the references -> the worst errors: (seg, E, S, moments)."""
    noff = np.concatenate([[0], np.cumsum([len(g) for g in case.graphs])])
    w_seg = w_e = w_s = w_m = 0.0
    nodes = cut = 0
    for i, (e, gr, _) in enumerate(case.vids):
        T, M, r = e.shape[0], len(gr), refs[i]
        assert np.isfinite(r['logz']), (what, i)
        for s in range(res['seg'].shape[0]):
            used = res['used'][s, noff[i]:noff[i + 1]]
            seg, node = TR.alignment_logp(r, res['spans'][s, i], used, gr.ids, T, case.kp(i), class_of)
            w_seg = max(w_seg, _close(np.exp(res['seg'][s, i]), np.exp(seg), what + ' seg_logp'),
                        _close(np.exp(res['node'][i][s]), np.exp(node), what + ' node_logp'))
        if res['E'] is not None:
            E, S = res['E'][noff[i]:noff[i + 1]], res['S'][noff[i]:noff[i + 1]]
            w_e = max(w_e, _close(E[:, :T + 1], r['E'].T, what + ' E'))
            w_s = max(w_s, _close(S[:, :T + 1], r['S'].T, what + ' S'))
            assert not E[:, T + 1:].any() and not S[:, T + 1:].any()
            assert not E[:, :T + 1][r['E'].T == 0].any() and not S[:, :T + 1][r['S'].T == 0].any()   # outside the ranges: exactly 0
        for m in range(M):
            nodes += 1
            if r['p_used'][m] < P_CUT:
                continue
            cut += 1
            for col, mean, sd in (('E', 'end_mean', 'end_sd'), ('S', 'start_mean', 'start_sd')):
                rm, rs = TR.moments(r[col][:, m])
                w_m = max(w_m, abs(res[mean][i][m] - rm), abs(res[sd][i][m] - rs))
    assert cut >= 0.9 * nodes, (what, cut, nodes)               # (the cut hides no more than a tenth of the case's nodes)
    print('\n[transcript-segment-posterior] %-28s seg %.2e  E %.2e  S %.2e (bar %.0e)  moments %.2e frames (%d of %d nodes)'
          % (what, w_seg, w_e, w_s, BAR, w_m, cut, nodes))
    assert res['err'] == 0
    if MOMENT_BAR is not None:
        assert w_m <= MOMENT_BAR, (what, w_m)
    return w_seg, w_e, w_s, w_m


def _chain(ids):
    return _ops().TranscriptGraph.chain(list(ids))


# ------------------------------------------------------------------------------------------------ 1. tiny graphs vs brute force
def _tiny_case():
    rng = np.random.default_rng(5)
    C, kp = 3, 4
    tab = _tables(rng, C, kp, 1.0)
    G = _ops().TranscriptGraph
    graphs = [_chain([0, 1, 2]), G.from_candidates([[0, 1, 2], [0, 2], [1, 2, 0]]), G.from_optional([0, 1, 2, 1], [False, True, False, True]),
              _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 2, 0])]
    vids = [(rng.normal(size=(t, C)), g, 0) for t, g in zip([6, 7, 6, 7], graphs)]
    return Case(vids, [tab], kp, endpen=rng.normal(size=(4, C)) * 0.5)


def test_tiny_graphs_against_brute_force():
    """A chain, a trie of 3, from_optional and an alternative pair; one align_graph output and four sampler draws in one call."""
    case = _tiny_case()
    res, _ = _run(case, sample=4)
    assert res['seg'].shape[0] == 5
    _check(case, res, _refs(case, brute=True), 'tiny graphs vs (d)')
    _check(case, res, _refs(case, fast=False), 'tiny graphs vs (b)')


def test_module_defaults_are_the_best_alignment():
    """alignment_segment_posteriors with spans and used None gives align_graph's alignment and its values in the explicit call."""
    from test_gpu_entropy import _features, _module
    m, g = _module(4, 5, 12, seed=8, scale=0.8)                # (span limit 11: three nodes cover 20 frames)
    lengths = [20, 17]
    x = _features(m, g, 2, lengths, 5).float().to(DEV)
    ln, vc = torch.tensor(lengths).to(DEV), [torch.arange(4)] * 2
    G = _ops().TranscriptGraph
    graphs = [G.from_candidates([[0, 1, 2], [0, 3, 2]]), G.chain([1, 0, 3])]
    spans, _, used = m.align_graph(x, ln, vc, graphs)
    dflt = m.alignment_segment_posteriors(x, ln, vc, graphs)
    given = m.alignment_segment_posteriors(x, ln, vc, graphs, spans=spans, used=used)
    assert torch.equal(dflt['spans'].cpu(), spans)
    assert torch.equal(dflt['seg_logp'], given['seg_logp'])
    for a, b in zip(dflt['node_logp'], given['node_logp']):
        assert torch.equal(a, b)
    p = torch.exp(dflt['seg_logp'][spans.to(DEV) != -1])
    assert bool(((p >= 0) & (p <= 1 + BAR)).all())


# ------------------------------------------------------------------------------------------------ 2. closed forms
def test_chain_with_as_many_frames_as_nodes():
    """T = M: one alignment.  Every node_logp is 0 within the bar; end_mean[m] = m + 1 and end_sd = 0 within 1e-9."""
    rng = np.random.default_rng(7)
    C, M = 3, 9
    case = Case([(rng.normal(size=(M, C)), _chain(rng.integers(0, C, M)), 0)], [_tables(rng, C, 5, 1.0)], 5)
    res, _ = _run(case)
    _close(np.exp(res['node'][0][0]), np.ones(M), 'chain T = M')
    np.testing.assert_allclose(res['end_mean'][0], np.arange(1, M + 1), rtol=0, atol=1e-9)
    np.testing.assert_allclose(res['start_mean'][0], np.arange(M), rtol=0, atol=1e-9)
    np.testing.assert_allclose(res['end_sd'][0], 0.0, rtol=0, atol=1e-9)
    np.testing.assert_allclose(res['start_sd'][0], 0.0, rtol=0, atol=1e-9)


def test_single_node():
    """One node covers the video: end_mean = T, start_mean = 0, both deviations 0, probability 1."""
    rng = np.random.default_rng(9)
    C, T = 3, 7
    case = Case([(rng.normal(size=(T, C)), _chain([1]), 0)], [_tables(rng, C, 9, 1.0)], 9, kps=[9])   # (kw = 8 >= T)
    res, _ = _run(case)
    assert abs(res['end_mean'][0][0] - T) <= 1e-9 and abs(res['start_mean'][0][0]) <= 1e-9
    assert abs(res['end_sd'][0][0]) <= 1e-9 and abs(res['start_sd'][0][0]) <= 1e-9
    _close(np.exp(res['node'][0][0]), np.ones(1), 'single node')


# ------------------------------------------------------------------------------------------------ 3. word, wave and tile edges
@pytest.mark.parametrize('M', [32, 33, 64, 65])
def test_chain_across_word_and_wave_edges(M):
    rng = np.random.default_rng(M)
    C, k = 4, 8
    T = M + 40
    tab = _tables(rng, C, k, 0.5)
    case = Case([(rng.normal(size=(T, C)) * 0.5, _chain(rng.integers(0, C, M)), 0)], [tab], k)
    res, _ = _run(case, sample=2)
    _check(case, res, _refs(case), 'chain M = %d' % M)


@pytest.mark.parametrize('T', [767, 768, 769])
def test_tile_edge(T):
    rng = np.random.default_rng(T)
    C, k = 3, 300
    tab = _tables(rng, C, k, 0.3)
    tab['len'] = tab['len'] - np.abs(np.arange(k) - 250.0)[:, None] * 0.02       # (segments of about 250 frames: three cover the video)
    case = Case([(rng.normal(size=(T, C)) * 0.1, _chain([0, 1, 2]), 0)], [tab], k)
    res, _ = _run(case, sample=2)
    _check(case, res, _refs(case), 'tile edge T = %d' % T)


def test_wide_ranges():
    """M = 4, T = 769, kp = 256, flat emissions: every column's range is wide, the moments sum many small terms."""
    rng = np.random.default_rng(17)
    C, k, T = 3, 256, 769
    tab = dict(trans=np.zeros((C, C)), init=np.zeros(C), len=np.zeros((k, C)))
    case = Case([(np.zeros((T, C)), _chain([0, 1, 2, 0]), 0)], [tab], k)
    res, _ = _run(case, sample=2)
    _check(case, res, _refs(case), 'wide ranges')


# ------------------------------------------------------------------------------------------------ 4. ragged, class map
def test_ragged_groups_with_tries():
    rng = np.random.default_rng(21)
    ns, k = [2, 3, 4], 9
    tabs = [_tables(rng, c, k, 0.3) for c in ns]                # (flat tables: every candidate of a trie keeps mass)
    G = _ops().TranscriptGraph
    graphs = [G.from_candidates([[0, 1, 0], [1, 0]]), G.from_candidates([[0, 1, 2], [0, 2, 1], [2, 1]]),
              G.from_candidates([[3, 0, 1, 2], [3, 1, 0], [0, 3, 2]])]
    vids = [(rng.normal(size=(t, c)) * 0.3, g, j) for j, (t, c, g) in enumerate(zip([10, 11, 13], ns, graphs))]
    case = Case(vids, tabs, k)
    cmap = np.array([[10, 11, 99, -7, -7], [20, 21, 22, 99, -7], [30, 31, 32, 33, 99]], np.int64)
    res, _ = _run(case, class_map=torch.from_numpy(cmap).to(DEV), sample=3)
    inv = {int(v): c for row in cmap for c, v in enumerate(row) if v not in (99, -7)}
    _check(case, res, _refs(case, fast=False), 'ragged, three groups, tries', class_of=lambda v: inv.get(int(v), -1))


# ------------------------------------------------------------------------------------------------ 5. dense rows vs p_used
def test_dense_rows_sum_to_the_backward_calls_p_used():
    """Row sums of node_end_post and node_start_post against the p_used of smm_align_graph_logz_bwd_f64 on the same workspace."""
    ops = _ops()
    case = _tiny_case()
    res, (batch, d, z, _) = _run(case)
    g = ops.align_graph_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, z['logz'], endpen=d['endpen'],
                                 ws=z['ws'], staged=z['_staged'], want_node_prob=True)
    p_used = torch.cat(g['node_prob']).cpu().numpy()
    _close(res['E'].sum(axis=1), p_used, 'dense E rows')
    _close(res['S'].sum(axis=1), p_used, 'dense S rows')


# ------------------------------------------------------------------------------------------------ 6. alignments the graph does not admit
def test_alignment_faults():
    """A span of the wrong class, one span too many and a span longer than kw: that set's video is -inf everywhere, no error, the
    neighbours untouched."""
    rng = np.random.default_rng(31)
    C, k = 3, 5
    tab = _tables(rng, C, k, 0.7)
    vids = [(rng.normal(size=(9, C)), _chain([0, 1, 2]), 0) for _ in range(2)]
    case = Case(vids, [tab], k)
    good, _ = _run(case)
    sp, us = good['spans'][0], good['used'][0]
    sets, useds = [sp], [us]
    wrong = sp.copy()
    wrong[0, 0] = 2                                             # node 0 is class 0
    extra = sp.copy()
    extra[0, int(np.flatnonzero(sp[0, :9] == -1)[0])] = 1       # a fourth span for three used nodes
    long_ = np.full_like(sp, -1)
    long_[:, 9] = sp[:, 9]
    long_[0, [0, 5, 7]] = [0, 1, 2]                             # 5 frames > kw = 4
    long_[1] = sp[1]
    for bad in (wrong, extra, long_):
        sets.append(bad)
        useds.append(us)
    res, _ = _run(case, spans=torch.from_numpy(np.stack(sets)).to(DEV), used=torch.from_numpy(np.stack(useds)).to(DEV))
    assert res['err'] == 0
    for s in (1, 2, 3):
        assert (res['seg'][s, 0] == NEG_INF).all() and (res['node'][0][s] == NEG_INF).all(), s
        assert np.array_equal(res['seg'][s, 1].view(np.int64), res['seg'][0, 1].view(np.int64))
        assert np.array_equal(res['node'][1][s].view(np.int64), res['node'][1][0].view(np.int64))
    assert np.array_equal(res['seg'][0].view(np.int64), good['seg'][0].view(np.int64))
    assert np.isfinite(res['seg'][0, 0][sp[0] != -1]).all()


# ------------------------------------------------------------------------------------------------ 7. in between other calls
def test_entropy_and_sampler_do_not_notice_the_call():
    """Entropy and sampler outputs are bit-equal with and without this call in between; two calls give the same bits."""
    ops = _ops()
    case = _tiny_case()
    batch, d = case.device_inputs()
    tabs = (d['elp'], d['trans'], d['init'], d['len'])

    def after(between):
        z = ops.align_graph_logz(batch, *tabs, case.graphs, endpen=d['endpen'])
        kw = dict(endpen=d['endpen'], ws=z['ws'], staged=z['_staged'])
        first = ops.align_graph_sample(batch, *tabs, case.graphs, z['logz'], 3, seed=1, want_labels=False, **kw)
        sp = None
        if between:
            sp = ops.align_graph_segment_posteriors(batch, *tabs, case.graphs, z['logz'], spans=first['spans'],
                                                    used=torch.cat(first['used'], dim=1), want_dense=True, **kw)
        h = ops.align_graph_entropy(batch, *tabs, case.graphs, z['logz'], want_parts=True, **kw)
        if between:
            ops.align_graph_segment_posteriors(batch, *tabs, case.graphs, z['logz'], **kw)
        s = ops.align_graph_sample(batch, *tabs, case.graphs, z['logz'], 3, seed=2, want_labels=False, **kw)
        torch.cuda.synchronize()
        return h['entropy'].cpu(), h['parts'].cpu(), s['spans'].cpu(), s['logp'].cpu(), sp

    a, b = after(False), after(True)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
    c = after(True)
    for key in ('seg_logp', 'node_end_post', 'node_start_post'):
        assert torch.equal(b[4][key].view(torch.int64), c[4][key].view(torch.int64)), key
    for key in ('end_mean', 'end_sd', 'start_mean', 'start_sd'):
        assert torch.equal(torch.cat(b[4][key]).view(torch.int64), torch.cat(c[4][key]).view(torch.int64)), key


def test_video_without_an_alignment():
    """log Z_g = -inf (more nodes than frames): NaN with the error word clear; the video beside it is what it is alone."""
    rng = np.random.default_rng(41)
    C, k = 3, 5
    tab = _tables(rng, C, k, 0.7)
    e0, e1 = rng.normal(size=(3, C)), rng.normal(size=(8, C))
    case = Case([(e0, _chain([0, 1, 2, 0]), 0), (e1, _chain([0, 1, 2]), 0)], [tab], k)
    res, _ = _run(case)
    assert res['err'] == 0 and res['logz'][0] == NEG_INF
    assert np.isnan(res['end_mean'][0]).all() and np.isnan(res['node'][0]).all() and np.isnan(res['seg'][0, 0, :4]).all()
    assert np.isnan(res['E'][:4, :4]).all() and not res['E'][:4, 4:].any()
    alone, _ = _run(Case([(e1, _chain([0, 1, 2]), 0)], [tab], k, kps=[case.kp(1)]))
    np.testing.assert_allclose(res['end_mean'][1], alone['end_mean'][0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(np.exp(res['node'][1]), np.exp(alone['node'][0]), rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ 8. model layer
def test_alignment_confidence_on_a_small_corpus():
    """SemiMarkovModel.alignment_confidence on each video's Viterbi transcript: one row per entry, starts and ends that tile the
    video, probabilities in [0, 1 + bar]; candidate_confidence on a set that holds that transcript names trie nodes."""
    from action_segmentation_amd import ops, synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts
    data = synth.SynthDatasplit('tiny', seed=11)
    fitted = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    fitted.fit(data, use_labels=True)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=True, batch_size=2), data)
    model.model.load_state_dict(fitted.model.state_dict(), strict=False)
    model.model.cuda()
    pc = model.prepare(data)
    t = pc.tables
    elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
    out = ops.viterbi(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    names = list(pc.video_names)
    tr = dict(zip(names, ([int(v) for v in a] for a in spans_to_transcripts(out['spans'], pc.lengths))))
    conf = model.alignment_confidence(data, tr)
    for name, n in zip(names, pc.batch.lengths.tolist()):
        rows = conf[name]
        assert [r[0] for r in rows] == list(range(len(tr[name]))) and [r[1] for r in rows] == tr[name]
        assert rows[0][2] == 0 and rows[-1][3] == n and all(a[3] == b[2] for a, b in zip(rows, rows[1:]))
        for (_, _, s, e, p, mean, sd) in rows:
            assert 0.0 <= p <= 1.0 + BAR and s < e and 0.0 < mean <= n and sd >= 0.0
        assert abs(rows[-1][5] - n) <= 1e-9 and rows[-1][6] <= 1e-9          # the last entry ends with the video
    cands = {v: [a, a + a[-1:]] for v, a in tr.items()}
    cc = model.candidate_confidence(data, cands)
    for name, n in zip(names, pc.batch.lengths.tolist()):
        rows = cc[name]
        assert rows and rows[0][2] == 0 and rows[-1][3] == n and all(a[3] == b[2] for a, b in zip(rows, rows[1:]))
        assert all(0.0 <= r[4] <= 1.0 + BAR for r in rows)
    assert math.isfinite(sum(r[4] for rows in conf.values() for r in rows))
