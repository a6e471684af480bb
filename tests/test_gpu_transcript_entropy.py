"""The exact entropy of the transcript-graph posterior on the GPU (smm_align_graph_entropy_f64) against the enumeration, the
numpy chain rule and the identity H = log Z_g - E[score] of tests/transcript_entropy_ref.py, the library's own end posteriors
and the sampler's log-probabilities.

Bars: tests/test_gpu_entropy.py's for the value -- |H - ref| <= 1e-5 max(1, ref) against enumeration and exact counts,
1e-4 max(1, H) against the identity on the fp64 gradients of tests/test_gpu_transcript_graph.py's references at its shapes --;
DESIGN 4n's 2e-5 for a posterior (H_end against the entropy of end_prob); the parts add up to H within 1e-12 relative (two
fp64 additions); the mean of -logp over n draws within 5 sd / sqrt(n) + 1e-4 max(1, H).  Every test prints its figures
("[transcript-entropy] ...") before it asserts.

Worst measured error per case on an MI355X:

    case                                         reference                      worst              bar
    tiny graphs, k_rows 4 / 8                    enumeration                    5.8e-08 / 2.2e-08  1e-5 max(1, H)
      parts against H; H_end against end_prob    -; smm_align_graph_logz_bwd    0; 2.2e-16         1e-12 rel; 2e-5
    all-zero tables, N = 30381 / 231             log N                          2.2e-09 / 1.1e-09  1e-5 max(1, H)
    T = 767 / 768 / 769 / 771                    identity, the twin's gradients 1.9e-08            1e-4 max(1, H)
    T = 1100, kp = 1024, M = 3                   the same                       3.4e-08            1e-4 max(1, H)
    M = 256 fan / M = 256 chain / M = 64 dense   the same                       4.9e-09 / 3.3e-08 / 1.4e-08   1e-4 max(1, H)
    mean of -logp, 4096 draws, six tiny graphs   the sampler                    <= 3.6e-02         5.8e-02 .. 1.1e-01
    candidate_entropy: boundaries, candidates    the model layer                <= 1e-06           2e-5 max(1, total)"""
import numpy as np
import pytest
import torch

import test_gpu_transcript_graph as GT
import test_gpu_transcript_sample as GS
import transcript_entropy_ref as TE
import transcript_graph_ref as TG
from test_gpu_transcript_graph import Case, _lists, _ops, _tables, _tuple

pytestmark = pytest.mark.gpu
H_BAR, IDENT_BAR, SUM_BAR, END_BAR = 1e-5, 1e-4, 1e-12, 2e-5


# ------------------------------------------------------------------------------------------------ launching
def _entropy(case, batch, d, fwd, want_parts=True):
    return _ops().align_graph_entropy(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, fwd['logz'],
                                      endpen=d['endpen'], ws=fwd['ws'], staged=fwd['_staged'], want_parts=want_parts)


def _backward(case, batch, d, fwd):
    return _ops().align_graph_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, fwd['logz'], grad_logz=d['u'],
                                       endpen=d['endpen'], ws=fwd['ws'], staged=fwd['_staged'], want_node_prob=True,
                                       want_end_prob=True)


def _run(case, fill=None):
    """Forward on a workspace of exactly the header's size, then the entropy -> (H [b], parts [b, 3], log Z_g [b], error word)."""
    batch, d, fwd = GS._forward(case, fill)
    out = _entropy(case, batch, d, fwd)
    return out['entropy'].cpu().numpy(), out['parts'].cpu().numpy(), fwd['logz'].cpu().numpy(), _ops().error_flag(batch, out)


def _parts_add_up(h, parts):
    fin = np.isfinite(h)
    assert (parts[fin] >= 0.0).all()
    return float((np.abs(parts[fin].sum(axis=1) - h[fin]) / np.maximum(1.0, h[fin])).max(initial=0.0))


def _bits(t):
    return t.contiguous().view(torch.int64)


# ------------------------------------------------------------------------------------------------ 1. tiny graphs
@pytest.mark.parametrize('which', [0, 1], ids=['k_rows4', 'k_rows8'])
def test_tiny_graphs_against_enumeration(which):
    """test_gpu_transcript_sample.exact_cases(): chain, from_optional, a trie with an end node that has a successor, the
    ambiguous diamond, a random graph with dead nodes, two ends under end penalties.  H against -sum p log p over the
    enumerated alignments, the parts against H, H_end against the entropy of the backward call's end_prob."""
    _, case, names = GS.exact_cases()[which]
    batch, d, fwd = GS._forward(case)
    out = _entropy(case, batch, d, fwd)
    h, parts = out['entropy'].cpu().numpy(), out['parts'].cpu().numpy()
    assert _ops().error_flag(batch, out) == 0 and np.isfinite(h).all()
    end_prob = [p.cpu().numpy() for p in _backward(case, batch, d, fwd)['end_prob']]
    worst = np.zeros(2)
    for i, name in enumerate(names):
        ref = TE.entropy_of(GS.enumerated(case, i)[2].values())
        errs = (abs(h[i] - ref) / max(1.0, ref), abs(parts[i, 0] - TE.entropy_of(end_prob[i])))
        print('\n[transcript-entropy] %-30s H %.6f (ref %.6f, rel %.1e, bar %.0e)  parts %s  H_end against end_prob %.1e (bar %.0e)'
              % (name, h[i], ref, errs[0], H_BAR, np.array2string(parts[i], precision=4), errs[1], END_BAR))
        worst = np.maximum(worst, errs)
    add = _parts_add_up(h, parts)
    print('\n[transcript-entropy] tiny graphs: worst H %.1e, H_end %.1e, parts against H %.1e (bar %.0e)'
          % (worst[0], worst[1], add, SUM_BAR))
    assert worst[0] <= H_BAR and worst[1] <= END_BAR and add <= SUM_BAR
    assert parts[0, 0] == 0.0 and parts[0, 2] == 0.0            # (video 0 is a chain)


# ------------------------------------------------------------------------------------------------ 2. exact zeros
def test_exact_zeros():
    """A chain has H_end and H_pred exactly 0; a chain with T == M has H exactly 0; -inf entries that leave one alignment
    (the arm 0 -> 1 of a diamond at T = 3; all span lengths but 2 of a chain of two at T = 4) give 0 <= H <= 1e-9."""
    G = _ops().TranscriptGraph
    rng = np.random.default_rng(29)
    C, K = 3, 4
    tab = _tables(rng, C, K, 1.5)
    no_arm, one_len = dict(tab, trans=tab['trans'].copy()), dict(tab, len=tab['len'].copy())
    no_arm['trans'][1, 0] = -np.inf
    one_len['len'][1] = one_len['len'][3] = -np.inf
    diamond = _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 2, 0])
    case = Case([(rng.normal(size=(9, C)), G.chain([0, 2, 1, 1]), 0), (rng.normal(size=(5, C)), G.chain([2, 0, 1, 0, 2]), 0),
                 (rng.normal(size=(3, C)), diamond, 1), (rng.normal(size=(4, C)), G.chain([2, 1]), 2)],
                [tab, no_arm, one_len], K, kps=[4, 4, 4, 4])
    for i in (2, 3):                                             # (the premise: one alignment of finite score each)
        assert len(GS.enumerated(case, i)[0]) == 1, i
    h, parts, z, err = _run(case)
    print('\n[transcript-entropy] exact zeros: H %s parts %s' % (h, parts.tolist()))
    assert err == 0 and np.isfinite(z).all() and not np.isnan(h).any() and not np.isnan(parts).any()
    assert h[0] > 0.1 and parts[0, 0] == 0.0 and parts[0, 2] == 0.0 and parts[0, 1] == h[0]
    assert h[1] == 0.0 and not parts[1].any()
    assert 0.0 <= h[2] <= 1e-9 and 0.0 <= h[3] <= 1e-9 and (parts[2:] >= 0.0).all()


# ------------------------------------------------------------------------------------------------ 3. uniform posteriors
def test_all_zero_tables_give_the_log_of_the_exact_count():
    """Zero elp, tables and penalties: every alignment has the same mass, H = log N with N counted in Python integers.  A
    chain of 5 over 40 frames at a span limit of 15 and a trie of three candidates over 12 frames."""
    G = _ops().TranscriptGraph
    C, K = 3, 16
    tab = dict(trans=np.zeros((C, C)), init=np.zeros(C), len=np.zeros((K, C)))
    graphs = [G.chain([0, 1, 2, 0, 1]), G.from_candidates([[0, 1, 2], [0, 1, 0, 2], [2, 1]])]
    case = Case([(np.zeros((40, C)), graphs[0], 0), (np.zeros((12, C)), graphs[1], 0)], [tab], K, endpen=np.zeros((2, C)))
    h, parts, z, err = _run(case)
    assert err == 0
    for i, g in enumerate(graphs):
        n = TE.count_alignments(case.lengths[i], _tuple(g), case.kp(i))
        ref = float(np.log(n))
        print('\n[transcript-entropy] uniform, video %d: N = %d, H %.9f, log N %.9f, rel %.1e (bar %.0e), log Z_g - log N %.1e'
              % (i, n, h[i], ref, abs(h[i] - ref) / max(1.0, ref), H_BAR, z[i] - ref))
        assert n > 1 and abs(h[i] - ref) <= H_BAR * max(1.0, ref)
    assert _parts_add_up(h, parts) <= SUM_BAR


# ------------------------------------------------------------------------------------------------ 4. - 6. real sizes
def _against_the_identity(case, what):
    """One video, finite tables, no end penalties: H against log Z_g - E[score] on the twin's fp64 gradients."""
    h, parts, z, err = _run(case)
    zr, gr = case.reference(TG.twin_grads_graph)
    e, _, _ = case.vids[0]
    t = case.tabs[0]
    ref = TE.identity_entropy(zr[0], dict(elp=gr['elp'], trans=gr['trans'][0], init=gr['init'][0], len=gr['len'][0]), e,
                              t['trans'], t['init'], t['len'])
    rel, add = abs(h[0] - ref) / max(1.0, ref), _parts_add_up(h, parts)
    print('\n[transcript-entropy] %-34s H %.6f (identity %.6f, rel %.1e, bar %.0e)  parts %s (sum %.1e)  logZ rel %.1e'
          % (what, h[0], ref, rel, IDENT_BAR, np.array2string(parts[0], precision=4), add, abs(z[0] - zr[0]) / max(1.0, abs(zr[0]))))
    assert err == 0 and np.isfinite(h[0]) and ref > 0.1
    assert rel <= IDENT_BAR and add <= SUM_BAR
    return h, parts


@pytest.mark.parametrize('T', [767, 768, 769, 771])
def test_tile_edges_against_the_identity(T):
    """T around the tile of 768 positions with kp = 64 and M = 20 on a branching graph (test_gpu_transcript_graph's shape)."""
    rng = np.random.default_rng(1000 + T)
    C, k_rows = 4, 64
    case = Case([(rng.normal(size=(T, C)) * 2, GT._branching(rng, 20, C), 0)], [_tables(rng, C, k_rows, 2.0)], k_rows)
    _against_the_identity(case, 'tile edge T=%d' % T)


def test_halo_longer_than_a_tile_against_the_identity():
    """T = 1100, kp = 1024, M = 3: the halo of a column is longer than its tile."""
    rng = np.random.default_rng(7)
    C, k_rows = 4, 1024
    graph = _lists(3, [[], [0], [0, 1]], [0], [1, 2], ids=[0, 1, 2])
    case = Case([(rng.normal(size=(1100, C)) * 2, graph, 0)], [_tables(rng, C, k_rows, 2.0)], k_rows)
    _against_the_identity(case, 'halo T=1100 kp=1024')


@pytest.mark.parametrize('kind', ['fan', 'chain', 'dense'])
def test_large_and_dense_graphs_against_the_identity(kind):
    """M = 256: 255 start nodes into one end node at T = 10 (every slot of the predecessor list, every mask word), and a chain
    of 256 at T = 300, kp = 8 (H_end and H_pred exactly 0); M = 64 with every pair an edge, every node a start and an end."""
    rng = np.random.default_rng(dict(fan=41, chain=21, dense=22)[kind])
    if kind == 'fan':
        C, K, T = 3, 10, 10
        graph, scale = GS._wide('fan', rng), 0.3
    elif kind == 'chain':
        C, K, T = 5, 8, 300
        graph, scale = _ops().TranscriptGraph.chain(rng.integers(0, C, 256)), 2.0
    else:
        C, K, T = 5, 8, 80
        graph = _ops().TranscriptGraph(rng.integers(0, C, 64), np.tril(np.ones((64, 64), bool), k=-1), np.ones(64, bool), np.ones(64, bool))
        scale = 2.0
    case = Case([(rng.normal(size=(T, C)) * scale, graph, 0)], [_tables(rng, C, K, 1.0 if kind != 'fan' else 0.5)], K)
    h, parts = _against_the_identity(case, 'M=%d %s' % (len(graph), kind))
    if kind == 'chain':
        assert parts[0, 0] == 0.0 and parts[0, 2] == 0.0
    else:
        assert parts[0, 2] > 0.0


# ------------------------------------------------------------------------------------------------ 7. the sampler
def test_the_mean_of_minus_logp_of_the_sampler_is_the_entropy():
    """4096 draws per video of the tiny graphs: H against the mean of -logp, within 5 standard errors + 1e-4 max(1, H)."""
    _, case, names = GS.exact_cases()[0]
    n = 4096
    batch, d, fwd = GS._forward(case)
    h = _entropy(case, batch, d, fwd)['entropy'].cpu().numpy()
    logp = GS._draw(case, batch, d, fwd, n, seed=11, want_spans=False, want_labels=False, want_used=False)['logp'].cpu().numpy()
    assert np.isfinite(logp).all()
    for i, name in enumerate(names):
        mean, sd = float(-logp[:, i].mean()), float(logp[:, i].std(ddof=1))
        bar = 5 * sd / np.sqrt(n) + 1e-4 * max(1.0, h[i])
        print('\n[transcript-entropy] %-30s H %.5f, mean -logp %.5f, difference %.1e (bar %.1e)' % (name, h[i], mean, abs(mean - h[i]), bar))
        assert abs(mean - h[i]) <= bar, name


# ------------------------------------------------------------------------------------------------ 8. ranges
def test_reads_stay_inside_the_recorded_ranges():
    """A workspace of 0xFF bytes (NaNs wherever no kernel writes) gives the bits of a zeroed one: a graph with dead nodes and
    skipped path lengths at two lengths, and a chain with T == M."""
    rng = np.random.default_rng(17)
    C, K = 3, 4
    tab = _tables(rng, C, K, 1.5)
    gap_dead = _lists(8, [[], [0], [1], [2], [3], [0, 4], [], [6]], [0], [5], ids=[0, 1, 2, 0, 1, 2, 1, 0])   # paths of 2 or 6; 6, 7 dead
    full = _ops().TranscriptGraph.chain([0, 1, 2, 0, 1, 2])
    case = Case([(rng.normal(size=(7, C)), gap_dead, 0), (rng.normal(size=(6, C)), full, 0),
                 (rng.normal(size=(4, C)), gap_dead, 0)], [tab], K, kps=[3, 4, 3])
    h0, p0, _, e0 = _run(case, fill=0)
    h1, p1, _, e1 = _run(case, fill=0xFF)
    ref = [TE.entropy_of(GS.enumerated(case, i)[2].values()) for i in range(3)]
    print('\n[transcript-entropy] poisoned workspace: H %s against %s, enumeration %s' % (h1, h0, ref))
    assert e0 == 0 and e1 == 0 and np.isfinite(h1).all()
    assert np.array_equal(h0.view(np.int64), h1.view(np.int64)) and np.array_equal(p0.view(np.int64), p1.view(np.int64))
    assert h1[1] == 0.0 and all(abs(h1[i] - ref[i]) <= H_BAR * max(1.0, ref[i]) for i in range(3))


# ------------------------------------------------------------------------------------------------ 9. degenerate videos
def test_degenerate_videos_beside_healthy_ones():
    """test_gpu_transcript_graph's five kinds -- no start -> end path, Lmin > T, Lmax kw < T, an id out of range, the gap graph
    at T = 5 -- between healthy videos: H and the parts NaN, the error word clear; with a NaN in the elp of one more video, the
    same and the error word.  The healthy videos keep the bits of a launch of their own."""
    G = _ops().TranscriptGraph
    rng = np.random.default_rng(13)
    C, K = 3, 4
    tab = _tables(rng, C, K, 1.5)
    good = _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 2, 0])
    graphs = [good, _lists(3, [[], [0], []], [0], [2], ids=[0, 1, 2]), G.chain([0, 1, 2, 0, 1, 2, 0]), good, G.chain([0, 1]),
              G.chain([0, 3]), GT._gap(), good]
    Ts, kps = [6, 6, 6, 7, 6, 6, 5, 5], [4, 4, 4, 4, 3, 4, 3, 4]
    vids = [(rng.normal(size=(T, C)), g, 0) for T, g in zip(Ts, graphs)]
    healthy = [0, 3, 7]
    ha, pa, _, err = _run(Case([vids[i] for i in healthy], [tab], K, kps=[kps[i] for i in healthy]))
    assert err == 0 and np.isfinite(ha).all() and (ha > 0.1).all()
    h, parts, z, err = _run(Case(vids, [tab], K, kps=kps))
    print('\n[transcript-entropy] degenerate videos: log Z_g %s, H %s, error word %d' % (z, h, err))
    assert err == 0
    bad_elp = rng.normal(size=(6, C))                            # (two segments of at most 3 frames cover it)
    bad_elp[3, 1] = np.nan
    h2, parts2, z2, err2 = _run(Case(vids + [(bad_elp, G.chain([1, 2]), 0)], [tab], K, kps=kps + [4]))
    print('\n[transcript-entropy] ... and a NaN video: log Z_g %s, H %s, error word %d' % (z2, h2, err2))
    assert err2 != 0 and np.isnan(z2[8]) and np.isnan(h2[8]) and np.isnan(parts2[8]).all()
    for hh, pp, zz in ((h, parts, z), (h2, parts2, z2)):
        for i in range(8):
            if i in healthy:
                continue
            assert zz[i] == -np.inf and np.isnan(hh[i]) and np.isnan(pp[i]).all(), i
        assert np.array_equal(hh[healthy].view(np.int64), ha.view(np.int64))
        assert np.array_equal(pp[healthy].view(np.int64), pa.view(np.int64))


# ------------------------------------------------------------------------------------------------ 10. determinism, call order
def test_two_calls_give_the_same_bits_and_disturb_no_other_call():
    """Two entropy calls give equal bits; a backward call issued after them gives the gradients, node_prob and end_prob of one
    issued on a fresh forward call without them; the sampler's draws before and after are the same."""
    case, _ = GT._ragged(kind='trie')
    batch, d, fwd = GS._forward(case)
    before = GS._draw(case, batch, d, fwd, 8, seed=123)
    a = _entropy(case, batch, d, fwd)
    b = _entropy(case, batch, d, fwd)
    assert _ops().error_flag(batch, a) == 0 and bool(torch.isfinite(a['entropy']).all())
    assert torch.equal(_bits(a['entropy']), _bits(b['entropy'])) and torch.equal(_bits(a['parts']), _bits(b['parts']))
    g = _backward(case, batch, d, fwd)
    after = GS._draw(case, batch, d, fwd, 8, seed=123)
    c = _entropy(case, batch, d, fwd)                            # ... and behind a whole backward call and a sampler call
    assert torch.equal(_bits(a['entropy']), _bits(c['entropy'])) and torch.equal(_bits(a['parts']), _bits(c['parts']))
    assert GS._same(before, after)
    _, d2, fwd2 = GS._forward(case)
    g2 = _backward(case, batch, d2, fwd2)
    for k in ('elp', 'trans', 'init', 'len'):
        assert torch.equal(_bits(g[k]), _bits(g2[k])), k
    for k in ('node_prob', 'end_prob'):
        assert torch.equal(_bits(torch.cat(g[k])), _bits(torch.cat(g2[k]))), k


def test_forward_and_entropy_capture_into_a_hip_graph():
    """Forward + entropy captured once with ``staged=`` and replayed on fresh inputs of the ragged shape: the replay
    reproduces the eager pair on those inputs bit for bit."""
    ops = _ops()
    case, _ = GT._ragged(kind='trie')
    batch, d = case.device_inputs()
    graphs = case.graphs
    ws = torch.empty(ops.align_graph_logz_workspace_bytes(batch, GS._node_offsets(case)), dtype=torch.uint8, device='cuda:0')
    staged = ops.align_graph_logz(batch, d['elp'], d['trans'], d['init'], d['len'], graphs, endpen=d['endpen'], ws=ws)['_staged']

    def step():
        z = ops.align_graph_logz(batch, d['elp'], d['trans'], d['init'], d['len'], graphs, endpen=d['endpen'], ws=ws,
                                 staged=staged)['logz']
        e = ops.align_graph_entropy(batch, d['elp'], d['trans'], d['init'], d['len'], graphs, z, endpen=d['endpen'], ws=ws,
                                    staged=staged, want_parts=True)
        return z, e['entropy'], e['parts']

    step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    fresh, _ = GT._ragged(values=1, kind='trie')
    _, f = fresh.device_inputs()
    for k in ('elp', 'trans', 'init', 'len', 'endpen'):
        d[k].copy_(f[k])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = [v.clone() for v in out]
    eager = step()
    torch.cuda.synchronize()
    for name, a, e in zip(('logz', 'entropy', 'parts'), got, eager):
        assert torch.equal(_bits(a), _bits(e)), name
    assert bool(torch.isfinite(got[1]).all()) and bool((got[1] > 0).all())


# ------------------------------------------------------------------------------------------------ 11. module, packed, model
def test_packed_two_groups_take_global_ids():
    """alignment_entropy_packed on a packed corpus of two class sets, chains in GLOBAL ids: each video's value is that of a
    padded call on its own group's batch (the same kernels on the same frames: 1e-9 relative), H_end and H_pred are 0."""
    from action_segmentation_amd.batching import pack_batches
    G = _ops().TranscriptGraph
    m, rb, vc, _ = GT._module_case()
    x, lengths = rb.features, rb.lengths.tolist()
    vc2 = [1, 3, 5]
    batches = [dict(task_name=['a'] * 2, task_indices=[torch.tensor(vc)] * 2, lengths=torch.tensor(lengths[:2]),
                    features=x[:2, :max(lengths[:2])].contiguous(), video_name=['a0', 'a1']),
               dict(task_name=['b'], task_indices=[torch.tensor(vc2)], lengths=torch.tensor(lengths[2:]),
                    features=x[2:, :lengths[2]].contiguous(), video_name=['b0'])]
    pc = pack_batches(batches, torch.device('cuda:0'), m.max_k)
    chains = {'a0': [4, 0, 2, 5, 0], 'a1': [5, 2, 4], 'b0': [3, 1, 5, 3]}
    h, parts = m.alignment_entropy_packed(pc, [G.chain(chains[name]) for name in pc.video_names], want_parts=True)
    assert h.shape == (3,) and parts.shape == (3, 3) and h.dtype == torch.float64 and not h.requires_grad
    h, parts = h.cpu().numpy(), parts.cpu().numpy()
    dev = torch.device('cuda:0')
    ha = m.alignment_entropy(x[:2].to(dev), rb.lengths[:2].to(dev), [torch.tensor(vc)] * 2, [G.chain(chains['a0']), G.chain(chains['a1'])])
    hb = m.alignment_entropy(x[2:, :lengths[2]].contiguous().to(dev), rb.lengths[2:].to(dev), [torch.tensor(vc2)], [G.chain(chains['b0'])])
    want = dict(zip(('a0', 'a1', 'b0'), torch.cat([ha, hb]).cpu().numpy()))
    for i, name in enumerate(pc.video_names):
        print('\n[transcript-entropy] packed %s: H %.9f, padded %.9f' % (name, h[i], want[name]))
        assert h[i] > 0.0 and abs(h[i] - want[name]) <= 1e-9 * max(1.0, want[name]), name
    assert not parts[:, 0].any() and not parts[:, 2].any()


def test_model_layer_candidates_and_optional_classes():
    """SemiMarkovModel.candidate_entropy: boundaries = total - candidates is the candidate_posteriors-weighted mean of the
    candidates' alignment_entropy, and candidates the entropy of candidate_posteriors.  alignment_entropy with
    optional_classes is the packed call on the from_optional graphs."""
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
    cands = {v: [a, a[:-1] if len(a) > 1 else a + a, a, a + a[-1:]] for v, a in tr.items()}
    got = model.candidate_entropy(data, cands)
    post = model.candidate_posteriors(data, cands)
    each = [model.alignment_entropy(data, {v: cands[v][j] for v in names}) for j in range(4)]
    for v in names:
        g, p = got[v], post[v]
        assert set(g) == {'total', 'candidates', 'boundaries'} and g['boundaries'] == g['total'] - g['candidates']
        want = float(sum(p[j] * each[j][v] for j in range(4) if p[j] > 0))
        bar = END_BAR * max(1.0, g['total'])
        print('\n[transcript-entropy] candidates of %s: total %.6f = candidates %.6f + boundaries %.6f (weighted mean %.6f, '
              'H(posteriors) %.6f, bar %.1e)' % (v, g['total'], g['candidates'], g['boundaries'], want, TE.entropy_of(p), bar))
        assert abs(g['boundaries'] - want) <= bar and abs(g['candidates'] - TE.entropy_of(p)) <= bar, v
    bg = set(int(c) for c in data.corpus._background_indices)
    mine = model.alignment_entropy(data, tr, optional_classes=bg)
    graphs = [ops.TranscriptGraph.from_optional(tr[v], [c in bg for c in tr[v]]) for v in names]
    packed = model.model.alignment_entropy_packed(model.prepare(data), graphs).cpu().numpy()
    plain = model.alignment_entropy(data, tr)
    print('\n[transcript-entropy] optional background: H %s, without the flags %s' % ([mine[v] for v in names], [plain[v] for v in names]))
    assert all(isinstance(mine[v], float) for v in names)
    assert np.array_equal(np.array([mine[v] for v in names]).view(np.int64), packed.view(np.int64))
    assert all(mine[v] >= 0.0 and plain[v] >= 0.0 for v in names)
    # a transcript that cannot be laid over its video: NaN, and no error
    long = dict(tr)
    long[names[0]] = [tr[names[0]][0]] * min(int(pc.lengths[0]) + 1, ops.MAX_TRANSCRIPT)
    if len(long[names[0]]) > int(pc.lengths[0]):
        assert np.isnan(model.alignment_entropy(data, long)[names[0]])
