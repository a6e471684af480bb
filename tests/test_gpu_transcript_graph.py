"""Transcript-graph likelihood on the GPU (smm_align_graph_logz_f64 / smm_align_graph_logz_bwd_f64) against
tests/transcript_graph_ref.py and against the family's other members.

Bars (tests/test_gpu_transcript_optional.py's): |logZ_g - ref| <= 1e-6 max(1, |ref|); g_elp, p_used and p_end within 2e-5
absolute; g_len, g_trans and g_init within 2e-5 (1 + videos of the group).  Chains against smm_align_logz_f64: 1e-12 relative
on logZ (the h, gam and q columns are formed in that unit's association), the gradients at the family bars (a chain's g_trans
and g_init are sums of posteriors here, counts there).  Every reference is computed once per case and shared.

Worst measured error per case on an MI355X (each test prints its line, "[transcript-graph] ..."; "-": no reference for it):

    case                                  logZ      g_elp     p_used    p_end     g_len     g_trans   g_init
    tiny graphs vs (d) and (b)            2.9e-09   1.6e-08   2.7e-08   3.0e-10   4.5e-09   1.2e-09   3.7e-11
    chains vs ops.align_logz              0 (bits)  3.6e-14   3.5e-08   1.8e-15   0         4.1e-08   0
    from_optional vs ops.align_opt_logz   1.7e-16   2.9e-14   4.1e-08   -         0         5.1e-09   6.7e-27
    trie of 8 vs 8 x ops.align_logz       0         3.6e-08   -         7.5e-19   5.5e-08   3.1e-08   1.4e-15
    T = 767 / 768 / 769 / 771 vs (c)      3.9e-10   4.2e-08   3.0e-08   -         4.0e-08   3.7e-08   9.4e-13
    T = 1100, kp = 1024, M = 3 vs (c)     1.1e-10   1.4e-08   8.7e-09   -         1.0e-08   4.3e-09   1.4e-14
    M = 256, word / wave boundaries       6.1e-10   6.3e-08   3.8e-08   -         4.8e-07   6.9e-08   5.1e-13
    M = 64, every pair an edge            7.0e-10   4.8e-08   4.8e-08   -         4.5e-08   5.7e-08   4.4e-10
    ragged, three groups, tries           3.1e-09   1.2e-07   4.6e-08   -         4.9e-08   8.8e-08   4.8e-10
    dynamic range, T = 2000               1.5e-12   4.2e-08   3.8e-08   -         7.5e-09   3.0e-08   7.3e-12
    -inf entries cut one arm              2.7e-09   1.4e-08   1.4e-08   0         5.8e-09   4.5e-09   3.7e-17

Chains: logZ is bit-equal to smm_align_logz_f64's, with and without end penalties.  The from_optional comparison sums in two
orders (per-class running sums there, the edges here)."""
import functools

import numpy as np
import pytest
import torch

import align_graph_ref as AG
import transcript_graph_ref as TG

pytestmark = pytest.mark.gpu
Z_BAR, ELP_BAR, LEN_BAR, SAME_BAR = 1e-6, 2e-5, 2e-5, 1e-12


def _ops():
    from action_segmentation_amd import ops
    return ops


def _tg(graph):
    return graph if isinstance(graph, _ops().TranscriptGraph) else _ops().TranscriptGraph(*graph)


def _tuple(g):
    return g.ids, g.pred, g.start, g.end


class Case:
    """A launch: videos (elp [T, C_g], TranscriptGraph, group), per-group tables, span limits, end penalties, upstream u."""

    def __init__(self, vids, tabs, k_rows, kps=None, endpen=None, u=None):
        self.vids = [(e, _tg(g), j) for e, g, j in vids]
        self.tabs, self.k_rows, self.kps, self.u = tabs, k_rows, kps, u
        self.n_states = [t['init'].shape[0] for t in tabs]
        self.cm = max(self.n_states)
        self.lengths = [v[0].shape[0] for v in self.vids]
        self.endpen = endpen                                  # [b, cm] numpy or None
        self.off = np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)
        self.graphs = [v[1] for v in self.vids]

    def kp(self, i):
        return int(self.kps[i]) if self.kps is not None else min(self.k_rows, max(self.lengths))

    def ep(self, i):
        return None if self.endpen is None else self.endpen[i, :self.n_states[self.vids[i][2]]]

    def device_inputs(self):
        ops = _ops()
        dev = torch.device('cuda:0')
        cm, g = self.cm, len(self.tabs)
        elp = np.zeros((int(self.off[-1]), cm))
        for i, v in enumerate(self.vids):
            elp[self.off[i]:self.off[i + 1], :v[0].shape[1]] = v[0]
        trans, init, lens = np.zeros((g, cm, cm)), np.zeros((g, cm)), np.zeros((g, self.k_rows, cm))
        for j, t in enumerate(self.tabs):
            c = self.n_states[j]
            trans[j, :c, :c], init[j, :c], lens[j, :, :c] = t['trans'], t['init'], t['len']
        batch = ops.Batch(self.lengths, self.n_states, self.k_rows, c_max=cm, frame_offset=self.off[:-1],
                          group=[v[2] for v in self.vids], kp=self.kps, total_frames=int(self.off[-1]))
        t = lambda a: None if a is None else torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        return batch, dict(elp=t(elp), trans=t(trans), init=t(init), len=t(lens), endpen=t(self.endpen), u=t(self.u))

    def run(self, bwd=True, raw=False):
        """-> (logZ_g [b], dict of the four gradients, p_used and p_end (lists per video), numpy; error word)."""
        ops = _ops()
        batch, d = self.device_inputs()
        out = ops.align_graph_logz(batch, d['elp'], d['trans'], d['init'], d['len'], self.graphs, endpen=d['endpen'])
        err = ops.error_flag(batch, out)
        g = None
        if bwd:
            r = ops.align_graph_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], self.graphs, out['logz'],
                                         grad_logz=d['u'], endpen=d['endpen'], ws=out['ws'], want_node_prob=True,
                                         want_end_prob=True)
            if raw:
                return out['logz'], r, err
            g = {k: r[k].cpu().numpy() for k in ('elp', 'trans', 'init', 'len')}
            g['p_used'] = [p.cpu().numpy() for p in r['node_prob']]
            g['p_end'] = [p.cpu().numpy() for p in r['end_prob']]
        return out['logz'].cpu().numpy(), g, err

    def reference(self, route):
        """-> (logZ_g [b], dict(elp [total, cm], trans, init, len [g, ...], p_used / p_end lists or None)) by ``route`` per
        video, weighted by u and summed."""
        g_n, cm = len(self.tabs), self.cm
        z = np.zeros(len(self.vids))
        g = dict(elp=np.zeros((int(self.off[-1]), cm)), trans=np.zeros((g_n, cm, cm)), init=np.zeros((g_n, cm)),
                 len=np.zeros((g_n, self.k_rows, cm)), p_used=[None] * len(self.vids), p_end=[None] * len(self.vids))
        for i, (e, gr, j) in enumerate(self.vids):
            t, c = self.tabs[j], self.n_states[j]
            z[i], gi = route(e, _tuple(gr), t['trans'], t['init'], t['len'], self.kp(i), self.ep(i))
            u = 1.0 if self.u is None else float(self.u[i])
            if not np.isfinite(z[i]) or z[i] < -1e8:
                z[i] = -np.inf
                g['p_used'][i] = g['p_end'][i] = np.zeros(len(gr))
                continue
            g['elp'][self.off[i]:self.off[i + 1], :c] = u * gi['elp']
            g['trans'][j, :c, :c] += u * gi['trans']
            g['init'][j, :c] += u * gi['init']
            g['len'][j, :, :c] += u * gi['len']
            g['p_used'][i], g['p_end'][i] = gi.get('p_used'), gi.get('p_end')
        return z, g

    def group_sizes(self):
        return np.bincount([v[2] for v in self.vids], minlength=len(self.tabs))


def numpy_route(e, graph, trans, init, lens, kp, ep):
    """(b): the header's forward-backward, every cell."""
    fb = TG.forward_backward(e, graph, trans, init, lens, kp, ep)
    return fb['logz'], fb


def _tables(rng, c, k_rows, scale=3.0):
    return dict(trans=rng.normal(size=(c, c)) * scale, init=rng.normal(size=c) * scale, len=rng.normal(size=(k_rows, c)) * scale)


def _errors(case, z, g, zr, gr):
    fin = np.isfinite(zr)
    assert np.array_equal(np.isfinite(z), fin), (z, zr)
    sizes = 1.0 + case.group_sizes()
    e = dict(logz=float((np.abs(z[fin] - zr[fin]) / np.maximum(1.0, np.abs(zr[fin]))).max(initial=0.0)),
             g_elp=float(np.abs(g['elp'] - gr['elp']).max()),
             g_len=float((np.abs(g['len'] - gr['len']).max(axis=(1, 2)) / sizes).max()),
             g_trans=float((np.abs(g['trans'] - gr['trans']).max(axis=(1, 2)) / sizes).max()),
             g_init=float((np.abs(g['init'] - gr['init']).max(axis=1) / sizes).max()), p_used=0.0, p_end=0.0)
    for i, (_, graph, _) in enumerate(case.vids):
        for k in ('p_used', 'p_end'):
            p = g[k][i]
            assert p.shape == (len(graph),)
            if gr[k][i] is not None:
                e[k] = max(e[k], float(np.abs(p - gr[k][i]).max()))
            if fin[i]:
                assert p.min() >= -ELP_BAR and p.max() <= 1.0 + ELP_BAR, (k, i)
            else:
                assert not p.any(), (k, i)
        if fin[i]:                                           # the path ends somewhere, and only in end nodes
            assert abs(g['p_end'][i].sum() - 1.0) <= ELP_BAR and not g['p_end'][i][~graph.end].any(), i
    return e


def _check(case, z, g, zr, gr, what):
    e = _errors(case, z, g, zr, gr)
    print('\n[transcript-graph] %-34s logZ %.2e (bar %.0e)  g_elp %.2e p_used %.2e p_end %.2e (%.0e)  g_len %.2e g_trans %.2e '
          'g_init %.2e (%.0e)' % (what, e['logz'], Z_BAR, e['g_elp'], e['p_used'], e['p_end'], ELP_BAR, e['g_len'], e['g_trans'],
                                 e['g_init'], LEN_BAR))
    assert e['logz'] <= Z_BAR, (what, e)
    assert max(e['g_elp'], e['p_used'], e['p_end']) <= ELP_BAR, (what, e)
    assert max(e['g_len'], e['g_trans'], e['g_init']) <= LEN_BAR, (what, e)
    return e


def _lists(M, preds, starts, ends, ids=None, C=3, seed=0):
    ids = np.random.default_rng(seed).integers(0, C, M) if ids is None else ids
    return _ops().TranscriptGraph(ids, preds, np.isin(np.arange(M), starts), np.isin(np.arange(M), ends))


def _gap():
    """paths of 2 or 6 nodes only: 0 -> 5 and 0 -> 1 -> 2 -> 3 -> 4 -> 5"""
    return _lists(6, [[], [0], [1], [2], [3], [0, 4]], [0], [5], seed=3)


# ------------------------------------------------------------------------------------------------ 1. tiny exhaustive
@functools.lru_cache(None)
def _tiny():
    rng = np.random.default_rng(1)
    C, kp = 3, 4
    tab = _tables(rng, C, kp, 1.5)
    graphs = {
        'diamond': _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 2, 0]),
        'diamond, equal arms': _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 1, 2]),
        'free order of two': _lists(4, [[], [], [1], [0]], [0, 1], [2, 3], ids=[0, 1, 0, 1]),
        'skip edge': _lists(4, [[], [0], [1], [0, 2]], [0], [3], ids=[2, 1, 0, 2]),
        'two starts, two ends': _lists(5, [[], [], [0, 1], [2], [2]], [0, 1], [3, 4], ids=[0, 1, 2, 0, 1]),
        'dead nodes': _lists(6, [[], [0], [1], [], [3], [3]], [0], [2, 4], ids=[0, 1, 2, 0, 1, 2]),
        'one node': _lists(1, [[]], [0], [0], ids=[1]),
    }
    vids = [(rng.normal(size=(T, C)) * 2, g, 0) for g in graphs.values() for T in (3, 6, 7)]
    vids += [(rng.normal(size=(T, C)) * 2, _gap(), 0) for T in (5, 7, 4)]
    kps = [4] * (len(vids) - 3) + [3] * 3
    case = Case(vids, [tab], kp, kps=kps, endpen=rng.normal(size=(len(vids), C)), u=rng.normal(size=len(vids)))
    brute = [TG.brute_logz_graph(e, _tuple(g), tab['trans'], tab['init'], tab['len'], case.kp(i), case.ep(i))
             for i, (e, g, _) in enumerate(case.vids)]
    return case, brute, case.reference(numpy_route)


def test_tiny_graphs_against_enumeration():
    """Diamond, free order of two, skip edge, two start and two end nodes, dead nodes, one node, each at T = 3, 6, 7 with
    kp = 4, and the path-length-gap graph at kp = 3 (-inf at T = 5, finite at T = 7 and 4): log Z_g, the frame occupancy,
    p_used and p_end against the enumeration over paths and compositions, the gradients against the header's recursions."""
    case, brute, ref = _tiny()
    z, g, err = case.run()
    assert err == 0
    n_fin = 0
    for i, ((_, graph, _), (zb, occ, pu, pe)) in enumerate(zip(case.vids, brute)):
        rows = g['elp'][case.off[i]:case.off[i + 1]]
        u = float(case.u[i])
        if not np.isfinite(zb):
            assert z[i] == -np.inf and not rows.any() and not g['p_used'][i].any() and not g['p_end'][i].any(), i
            continue
        assert abs(z[i] - zb) <= Z_BAR * max(1.0, abs(zb)), (i, z[i], zb)
        assert np.abs(rows - u * occ).max() <= ELP_BAR * max(1.0, abs(u)), i
        assert np.abs(g['p_used'][i] - pu).max() <= ELP_BAR and np.abs(g['p_end'][i] - pe).max() <= ELP_BAR, i
        n_fin += 1
    gap = len(case.vids) - 3
    assert z[gap] == -np.inf and np.isfinite(z[gap + 1]) and np.isfinite(z[gap + 2])
    assert AG.feasible_by_count(5, *_tuple(case.graphs[gap])[1:], 3)
    assert n_fin >= 15
    _check(case, z, g, *ref, 'tiny graphs')


# ------------------------------------------------------------------------------------------------ 2. chains, optional entries
def _ragged(values=0, kind='chain', with_endpen=True):
    """3 groups of 3, 11 and 32 states, 8 videos with their own span limits (tests/test_gpu_transcript.py's shape)."""
    ops = _ops()
    rng, val = np.random.default_rng(77), np.random.default_rng(500 + values)
    n_states, k_rows = [3, 11, 32], 24
    tabs = [_tables(val, c, k_rows) for c in n_states]
    vids, kps, plain = [], [], []
    for i, (T, j) in enumerate([(5, 0), (90, 2), (33, 1), (61, 0), (17, 2), (48, 1), (24, 2), (80, 1)]):
        kp = int(rng.integers(4, k_rows + 1))
        lo = -(-T // (kp - 1))
        M = int(rng.integers(lo, min(T, lo + 9) + 1))
        a = rng.integers(0, n_states[j], size=M)
        if M >= 3:
            a[1] = a[2] = a[0]                                # consecutive repeats are separate segments
        opt = rng.random(M) < 0.5
        e = val.normal(size=(T, n_states[j])) * 3
        if kind == 'chain':
            graph = ops.TranscriptGraph.chain(a)
        elif kind == 'optional':
            graph = ops.TranscriptGraph.from_optional(a, opt)
        else:                                                 # a trie of the transcript and three variations of it
            cands = [a.tolist(), a[:max(1, M - 1)].tolist(), a[:M // 2].tolist() + a[M // 2:][::-1].tolist(),
                     np.roll(a, 1).tolist()]
            graph = ops.TranscriptGraph.from_candidates(cands)
        vids.append((e, graph, j))
        plain.append(([int(v) for v in a], [bool(v) for v in opt]))
        kps.append(kp)
    endpen = val.normal(size=(len(vids), 32)) * 2 if with_endpen else None
    u = np.array([1.0, 0.0, -0.75, 2.5, 0.3, 1.0, -1.25, 0.5])
    return Case(vids, tabs, k_rows, kps=kps, endpen=endpen, u=u), plain


@pytest.mark.parametrize('with_endpen', [False, True])
def test_chains_are_the_exact_transcript_likelihood(with_endpen):
    """Chains on a ragged batch of three groups against smm_align_logz_f64 / _bwd_f64 on the same inputs: logZ to 1e-12
    relative (measured: bit-equal, printed), the gradients at the family bars."""
    ops = _ops()
    case, plain = _ragged(kind='chain', with_endpen=with_endpen)
    z, g, err = case.run()
    batch, d = case.device_inputs()
    out = ops.align_logz_ex(batch, d['elp'], d['trans'], d['init'], d['len'], [p[0] for p in plain], endpen=d['endpen'])
    want = ops.align_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], out['transcript'], out['logz'],
                              grad_logz=d['u'], endpen=d['endpen'], ws=out['ws'])
    zw = out['logz'].cpu().numpy()
    assert err == 0 and np.isfinite(zw).all()
    rel = float((np.abs(z - zw) / np.maximum(1.0, np.abs(zw))).max())
    print('\n[transcript-graph] chains, endpen=%s: logZ rel %.2e, bit-equal: %s' % (with_endpen, rel, np.array_equal(z, zw)))
    assert rel <= SAME_BAR
    gr = {k: want[k].cpu().numpy() for k in ('elp', 'trans', 'init', 'len')}
    gr['p_used'] = [np.ones(len(gph)) for gph in case.graphs]
    gr['p_end'] = [gph.end.astype(np.float64) for gph in case.graphs]
    _check(case, z, g, zw, gr, 'chains vs align_logz')


def test_optional_graphs_are_the_optional_transcript_likelihood():
    """``from_optional`` graphs against smm_align_opt_logz_f64 / _bwd_f64, p_used included (the two sides sum in different
    orders: per-class running sums there, the edges themselves here)."""
    ops = _ops()
    case, plain = _ragged(kind='optional')
    z, g, err = case.run()
    batch, d = case.device_inputs()
    ids, flags = [p[0] for p in plain], [p[1] for p in plain]
    out = ops.align_opt_logz(batch, d['elp'], d['trans'], d['init'], d['len'], ids, flags, endpen=d['endpen'])
    want = ops.align_opt_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], ids, flags, out['logz'], grad_logz=d['u'],
                                  endpen=d['endpen'], ws=out['ws'], want_entry_prob=True)
    zw = out['logz'].cpu().numpy()
    assert err == 0 and np.isfinite(zw).all()
    gr = {k: want[k].cpu().numpy() for k in ('elp', 'trans', 'init', 'len')}
    gr['p_used'] = [p.cpu().numpy() for p in want['entry_prob']]
    gr['p_end'] = [None] * len(ids)
    _check(case, z, g, zw, gr, 'from_optional vs align_opt_logz')


# ------------------------------------------------------------------------------------------------ 3. a trie of 8 candidates
def test_a_trie_of_eight_is_the_lse_of_eight_transcript_likelihoods():
    """One video, 8 candidates that share prefixes: logZ_g against the logsumexp of 8 ops.align_logz calls (one launch of 8
    replicated videos), p_end against their softmax, the gradients against the posterior-weighted sum of the 8
    ops.align_logz_bwd results."""
    ops = _ops()
    rng = np.random.default_rng(31)
    C, K, T = 6, 12, 70
    tab = _tables(rng, C, K)
    base = [int(v) for v in rng.integers(0, C, 9)]
    cands = [base, base[:7], base[:4] + [5, 1, 2, 0], base[:4] + [5, 1, 3], base[:2] + base[4:] + [2], [int(v) for v in rng.integers(0, C, 8)],
             base[:8] + [0, 1], base[:1] + base[:6] + [4]]
    assert len({tuple(c) for c in cands}) == 8
    e = rng.normal(size=(T, C)) * 2
    trie = ops.TranscriptGraph.from_candidates(cands)
    endpen = rng.normal(size=(1, C))
    case = Case([(e, trie, 0)], [tab], K, endpen=endpen, u=np.array([1.5]))
    z, g, err = case.run()
    assert err == 0 and np.isfinite(z[0])
    rep = Case([(e, ops.TranscriptGraph.chain(c), 0) for c in cands], [tab], K, endpen=np.repeat(endpen, 8, axis=0))
    batch, d = rep.device_inputs()
    out = ops.align_logz_ex(batch, d['elp'], d['trans'], d['init'], d['len'], cands, endpen=d['endpen'])
    zc = out['logz'].cpu().numpy()
    assert np.isfinite(zc).all()
    want = zc.max() + np.log(np.exp(zc - zc.max()).sum())
    post = np.exp(zc - want)
    w = torch.tensor(1.5 * post, dtype=torch.float64, device='cuda:0')
    gw = ops.align_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], out['transcript'], out['logz'], grad_logz=w,
                            endpen=d['endpen'], ws=out['ws'])
    gr = {k: gw[k].cpu().numpy() for k in ('trans', 'init', 'len')}
    gr['elp'] = gw['elp'].cpu().numpy().reshape(8, T, C).sum(axis=0)
    pe = np.zeros(len(trie))
    for node in np.flatnonzero(trie.end):
        pe[node] = post[int(trie.end_candidate[node])]
    gr['p_used'], gr['p_end'] = [None], [pe]
    e_ = _errors(case, z, g, np.array([want]), gr)
    print('\n[transcript-graph] trie of 8: %s' % e_)
    assert e_['logz'] <= Z_BAR and max(e_['g_elp'], e_['p_end']) <= ELP_BAR
    assert max(e_['g_len'], e_['g_trans'], e_['g_init']) <= LEN_BAR


# ------------------------------------------------------------------------------------------------ 4. tile geometry
def _branching(rng, M, C, width=3):
    """A DAG in which every node takes the node before it and up to width - 1 more of the four before it: skips that meet again."""
    preds = [[]] + [sorted({m - 1} | set(int(v) for v in rng.integers(max(0, m - 4), m, int(rng.integers(0, width)))))
                    for m in range(1, M)]
    return _ops().TranscriptGraph(rng.integers(0, C, M), preds, np.arange(M) < 2, np.arange(M) >= M - 2)


@pytest.mark.parametrize('T', [767, 768, 769, 771])
def test_tile_edges_against_the_twin(T):
    """T around the tile of 768 positions with kp = 64 and M = 20 on a branching graph."""
    assert _ops().ALIGN_LOGZ_TILE == 768
    rng = np.random.default_rng(1000 + T)
    C, k_rows = 4, 64
    case = Case([(rng.normal(size=(T, C)) * 2, _branching(rng, 20, C), 0)], [_tables(rng, C, k_rows, 2.0)], k_rows)
    z, g, err = case.run()
    assert err == 0 and np.isfinite(z[0])
    _check(case, z, g, *case.reference(TG.twin_grads_graph), 'tile edge T=%d' % T)


def test_halo_longer_than_a_tile_against_the_twin():
    """T = 1100, kp = 1024, M = 3: a diamond's first three nodes, the halo of a column is longer than its tile."""
    rng = np.random.default_rng(7)
    C, k_rows = 4, 1024
    graph = _lists(3, [[], [0], [0, 1]], [0], [1, 2], ids=[0, 1, 2])
    case = Case([(rng.normal(size=(1100, C)) * 2, graph, 0)], [_tables(rng, C, k_rows, 2.0)], k_rows)
    z, g, err = case.run()
    assert err == 0 and np.isfinite(z[0])
    _check(case, z, g, *case.reference(TG.twin_grads_graph), 'halo T=1100 kp=1024')


# ------------------------------------------------------------------------------------------------ 5. ballot compaction
def test_wave_and_mask_word_boundaries_against_the_twin():
    """M = 256, T = 300, kp = 8.  A chain 0 -> 1 -> ... -> 255 (its edges 31 -> 32, 63 -> 64, ... cross every mask word and wave)
    with the edge 0 -> 255 and a node, 59, whose successors are 60 .. 70 and 190 .. 200: its list straddles three waves."""
    rng = np.random.default_rng(21)
    M, T, C, k_rows = 256, 300, 5, 8
    preds = [[]] + [[m - 1] for m in range(1, M)]
    for m in list(range(61, 71)) + list(range(190, 201)):
        preds[m].append(59)
    preds[255].append(0)
    graph = _ops().TranscriptGraph(rng.integers(0, C, M), preds, np.arange(M) == 0, np.arange(M) >= 250)
    case = Case([(rng.normal(size=(T, C)) * 2, graph, 0)], [_tables(rng, C, k_rows, 1.0)], k_rows)
    z, g, err = case.run()
    assert err == 0 and np.isfinite(z[0])
    _check(case, z, g, *case.reference(TG.twin_grads_graph), 'M=256, word and wave boundaries')


def test_dense_graph_against_the_twin():
    """64 nodes, every pair an edge, every node a start and an end node; T = 80, kp = 8."""
    rng = np.random.default_rng(22)
    M, T, C, k_rows = 64, 80, 5, 8
    graph = _ops().TranscriptGraph(rng.integers(0, C, M), np.tril(np.ones((M, M), bool), k=-1), np.ones(M, bool), np.ones(M, bool))
    case = Case([(rng.normal(size=(T, C)) * 2, graph, 0)], [_tables(rng, C, k_rows, 1.0)], k_rows)
    z, g, err = case.run()
    assert err == 0 and np.isfinite(z[0])
    _check(case, z, g, *case.reference(TG.twin_grads_graph), 'M=64, every pair an edge')


# ------------------------------------------------------------------------------------------------ 6. ragged batch, ranges
def test_ragged_batch_of_tries_against_the_twin():
    """Three groups in one launch, every video a trie of four candidates, its own span limit, end penalties and weights."""
    case, _ = _ragged(kind='trie')
    z, g, err = case.run()
    assert err == 0
    _check(case, z, g, *case.reference(TG.twin_grads_graph), 'ragged, three groups, tries')


def test_dynamic_range_against_the_twin():
    """T = 2000, kp = 1024; the elp columns differ by +-50 per frame in runs of 100 - 300 frames, the length scores are Poisson
    log-pmfs with rates 50 - 400 (tests/test_gpu_transcript.py's case), on a graph of 9 nodes with alternatives and skips."""
    rng = np.random.default_rng(5)
    T, C, K = 2000, 4, 1024
    elp = rng.normal(size=(T, C))
    t = 0
    while t < T:
        run = int(rng.integers(100, 301))
        elp[t:t + run] += rng.choice([-50.0, 50.0], size=C)
        t += run
    rates = rng.uniform(50, 400, size=C)
    k = np.arange(K)[:, None]
    tab = dict(trans=rng.normal(size=(C, C)), init=rng.normal(size=C),
               len=k * np.log(rates) - rates - torch.lgamma(torch.arange(K, dtype=torch.float64) + 1).numpy()[:, None])
    graph = _lists(9, [[], [0], [0], [1, 2], [3], [3, 4], [5], [5, 6], [6, 7]], [0], [7, 8], ids=[0, 1, 2, 3, 1, 0, 2, 3, 1])
    case = Case([(elp, graph, 0)], [tab], K)
    z, g, err = case.run()
    assert err == 0 and np.isfinite(z[0])
    _check(case, z, g, *case.reference(TG.twin_grads_graph), 'dynamic range')


# ------------------------------------------------------------------------------------------------ 7. tables, degenerate videos
def _diamond_case(rng, mutate):
    C, K, T = 4, 6, 10
    tab = _tables(rng, C, K, 1.5)
    graph = _lists(5, [[], [0], [0], [1, 2], []], [0], [3], ids=[0, 1, 2, 3, 3])     # node 4: off every path
    mutate(tab)
    return Case([(rng.normal(size=(T, C)), graph, 0), (rng.normal(size=(T, C)), _ops().TranscriptGraph.chain([1, 2]), 0)], [tab], K)


def test_minus_infinity_entries_that_cut_all_but_one_path():
    def cut(tab):
        tab['trans'][1, 0] = -np.inf                           # 0 -> 1: the diamond keeps its arm through node 2

    case = _diamond_case(np.random.default_rng(3), cut)
    z, g, err = case.run()
    assert err == 0 and np.isfinite(z).all()
    assert g['p_used'][0][1] == 0.0 and abs(g['p_used'][0][2] - 1.0) <= ELP_BAR and g['p_used'][0][4] == 0.0
    _check(case, z, g, *case.reference(numpy_route), '-inf cuts one arm')


def test_minus_infinity_entries_that_cut_every_path():
    def cut(tab):
        tab['trans'][1, 0] = tab['trans'][2, 0] = -np.inf

    case = _diamond_case(np.random.default_rng(3), cut)
    z, g, err = case.run()
    assert err == 0 and z[0] == -np.inf and np.isfinite(z[1])
    assert not g['elp'][:case.off[1]].any() and not g['p_used'][0].any() and not g['p_end'][0].any()
    _check(case, z, g, *case.reference(numpy_route), '-inf cuts every path')


def test_nan_in_a_table_entry_of_a_node_off_every_path_sets_the_error_word():
    """trans[3][3] is NaN.  The diamond with a dead node of class 3 has no edge between two nodes of class 3: the word stays
    clear.  With a second dead node behind the first (the edge 4 -> 5 reads trans[3][3], on no start -> end path) the word is
    set, the video's logZ_g is NaN and its contributions zero; the clean video beside it keeps its bits."""
    rng = np.random.default_rng(3)
    C, K, T = 4, 6, 10
    tab = _tables(rng, C, K, 1.5)
    tab['trans'][3, 3] = np.nan
    clean = _lists(5, [[], [0], [0], [1, 2], []], [0], [3], ids=[0, 1, 2, 3, 3])
    dead_edge = _lists(6, [[], [0], [0], [1, 2], [], [4]], [0], [3], ids=[0, 1, 2, 3, 3, 3])   # 4 -> 5 reads trans[3][3]
    e = rng.normal(size=(T, C))
    case = Case([(e, clean, 0)], [tab], K)
    z, g, err = case.run()
    assert err == 0 and np.isfinite(z[0])
    case = Case([(e, dead_edge, 0), (e, clean, 0)], [tab], K)
    z2, g2, err = case.run()
    assert err != 0 and np.isnan(z2[0]) and z2[1] == z[0]
    assert not g2['elp'][:T].any() and not g2['p_used'][0].any() and not g2['p_end'][0].any()
    assert np.array_equal(g2['elp'][T:], g['elp']) and np.array_equal(g2['trans'], g['trans'])


def test_degenerate_videos_beside_healthy_ones():
    """No start -> end path, Lmin > T, Lmax kw < T, an id out of range, the gap graph at T = 5: logZ_g -inf, exactly zero
    rows and posteriors, the error word clear; the healthy videos between them are unaffected."""
    ops = _ops()
    rng = np.random.default_rng(13)
    C, K = 3, 4
    tab = _tables(rng, C, K, 1.5)
    G = ops.TranscriptGraph
    good = _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 2, 0])
    graphs = [good,
              _lists(3, [[], [0], []], [0], [2], ids=[0, 1, 2]),              # no start -> end path
              G.chain([0, 1, 2, 0, 1, 2, 0]),                                 # Lmin = 7 > T = 6
              good,
              G.chain([0, 1]),                                                # Lmax kw = 2 * 2 < 6 at kp = 3
              G.chain([0, 3]),                                                # an id out of range
              _gap(),                                                         # T = 5, kp = 3: passes the count rule, no alignment
              good]
    Ts = [6, 6, 6, 7, 6, 6, 5, 5]
    kps = [4, 4, 4, 4, 3, 4, 3, 4]
    case = Case([(rng.normal(size=(T, C)), g, 0) for T, g in zip(Ts, graphs)], [tab], K, kps=kps)
    z, g, err = case.run()
    assert err == 0
    healthy = [0, 3, 7]
    for i in range(len(graphs)):
        rows = g['elp'][case.off[i]:case.off[i + 1]]
        if i in healthy:
            assert np.isfinite(z[i]) and rows.any()
        else:
            assert z[i] == -np.inf and not rows.any() and not g['p_used'][i].any() and not g['p_end'][i].any(), i
    alone = Case([case.vids[i] for i in healthy], [tab], K, kps=[kps[i] for i in healthy])
    za, ga, _ = alone.run()
    assert np.array_equal(za, z[healthy])
    for k in ('trans', 'init', 'len'):
        assert np.array_equal(ga[k], g[k]), k


def test_two_calls_give_the_same_bits():
    case, _ = _ragged(kind='trie')
    z1, r1, _ = case.run(raw=True)
    z2, r2, _ = case.run(raw=True)
    assert torch.equal(z1, z2)
    for k in ('elp', 'trans', 'init', 'len'):
        assert torch.equal(r1[k], r2[k]), k
    for k in ('node_prob', 'end_prob'):
        assert torch.equal(torch.cat(r1[k]), torch.cat(r2[k])), k


# ------------------------------------------------------------------------------------------------ 8. stream capture
def test_forward_and_backward_capture_into_a_hip_graph():
    """The pair captured once with ``staged=`` and replayed once on fresh inputs of the ragged shape: the replay reproduces
    the eager call on those inputs bit for bit."""
    ops = _ops()
    case, _ = _ragged(kind='trie')
    batch, d = case.device_inputs()
    graphs = case.graphs
    off = np.concatenate([[0], np.cumsum([len(g) for g in graphs])]).astype(np.int64)
    ws = torch.empty(ops.align_graph_logz_workspace_bytes(batch, off), dtype=torch.uint8, device='cuda:0')
    staged = ops.align_graph_logz(batch, d['elp'], d['trans'], d['init'], d['len'], graphs, endpen=d['endpen'], ws=ws)['_staged']

    def step():
        z = ops.align_graph_logz(batch, d['elp'], d['trans'], d['init'], d['len'], graphs, endpen=d['endpen'], ws=ws,
                                 staged=staged)['logz']
        g = ops.align_graph_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], graphs, z, grad_logz=d['u'],
                                     endpen=d['endpen'], ws=ws, staged=staged, want_node_prob=True, want_end_prob=True)
        return z, g['elp'], g['trans'], g['init'], g['len'], torch.cat(g['node_prob']), torch.cat(g['end_prob'])

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
    fresh, _ = _ragged(values=1, kind='trie')
    _, f = fresh.device_inputs()
    for k in ('elp', 'trans', 'init', 'len', 'endpen'):
        d[k].copy_(f[k])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = [v.clone() for v in out]
    eager = step()
    torch.cuda.synchronize()
    for name, a, e in zip(('logz', 'g_elp', 'g_trans', 'g_init', 'g_len', 'p_used', 'p_end'), got, eager):
        assert torch.equal(a, e), name
    assert bool(torch.isfinite(got[0]).all())


# ------------------------------------------------------------------------------------------------ 9. module, packed, model
def _module_case(seed=3, n=6, d=8, k=12, lengths=(40, 25, 33)):
    """A module with random parameters, a padded batch of three videos over four valid classes, and per video the trie of its
    true transcript and three variations (GLOBAL class ids)."""
    import train_ref as R
    from module_util import make_args
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    rng = np.random.default_rng(seed)
    gen = torch.Generator().manual_seed(seed)
    m = SemiMarkovModule(make_args(k), n, d, allow_self_transitions=True)
    mu = rng.normal(0, 1.0, size=(n, d))
    with torch.no_grad():
        m.gaussian_means.copy_(torch.as_tensor(mu, dtype=torch.float32))
        m.gaussian_cov.copy_(torch.diag(torch.as_tensor(rng.uniform(0.7, 1.3, size=d), dtype=torch.float32)))
        m.transition_logits.copy_(torch.randn(n, n, generator=gen))
        m.init_logits.copy_(torch.randn(n, generator=gen))
        m.poisson_log_rates.copy_(torch.log(torch.rand(n, generator=gen) * 8 + 3))
    vc = [4, 0, 2, 5]
    x = np.zeros((len(lengths), max(lengths), d), np.float32)
    graphs = []
    for i, t in enumerate(lengths):
        M = int(rng.integers(-(-t // (k - 1)) + 2, 9))
        a = [vc[int(v)] for v in rng.integers(0, len(vc), size=M)]
        cuts = np.sort(rng.choice(np.arange(1, t), size=M - 1, replace=False))
        x[i, :t] = mu[np.repeat(np.array(a), np.diff(np.concatenate([[0], cuts, [t]])))] + rng.standard_normal((t, d))
        cands = [a, a[:-1] + [vc[(vc.index(a[-1]) + 1) % 4]], a[:M // 2] + a[M // 2:][::-1], a + [vc[0]]]
        graphs.append(_ops().TranscriptGraph.from_candidates(cands))
    return m.cuda(), R.RefBatch(x, list(lengths), vc), vc, graphs


@pytest.mark.parametrize('discriminative', [False, True])
def test_module_values_and_parameter_gradients(discriminative):
    """transcript_graph_log_partition and log_likelihood(transcript_graphs=...) against autograd through torch_logz_graph
    (reference (a)) on train_ref's tables; discriminative: minus log Z, held to the size of its two parts."""
    import train_ref as R
    m, rb, vc, graphs = _module_case()
    m.args.sm_train_discriminatively = discriminative
    dev = torch.device('cuda:0')
    x, lengths, vcs = rb.features.to(dev), rb.lengths.to(dev), [rb.valid_classes] * len(graphs)
    q, leaves = R.params_from_module(m)
    trans, init, lens, merged = R.tables(q, rb.valid_classes)
    elp = R.emission(q, merged, rb)
    kp = R.kp_of(lens, rb)
    loc = {c: j for j, c in enumerate(vc)}
    local = [([loc[int(c)] for c in g.ids], g.pred, g.start, g.end) for g in graphs]
    zg = torch.stack([TG.torch_logz_graph(elp[i, :int(t)], local[i], trans, init, lens, kp) for i, t in enumerate(rb.lengths.tolist())])
    value = zg.mean().item()
    ref = R.grads(leaves, zg.mean())
    models = None
    if discriminative:
        zl = R.logz_factored(q, rb)
        value -= zl.mean().item()
        gl = R.grads(leaves, zl.mean())
        models = {n: dict(size=np.abs(ref[n]) + np.abs(gl[n])) for n in ref}
        ref = {n: ref[n] - gl[n] for n in ref}
    z = m.transcript_graph_log_partition(x, lengths, vcs, graphs)
    assert z.dtype == torch.float64 and z.requires_grad
    np.testing.assert_allclose(z.detach().cpu().numpy(), zg.detach().numpy(), rtol=Z_BAR)
    m.zero_grad()
    ll, _ = m.log_likelihood(x, lengths, vcs, transcript_graphs=graphs)
    ll.backward()
    assert abs(ll.item() - value) <= Z_BAR * max(1.0, abs(zg.mean().item()))
    got = R.module_grads(m)
    assert all(np.abs(v).max() > 0 for v in got.values())
    R.assert_grads_close(got, ref, ELP_BAR, 'transcript graph discriminative=%s' % discriminative, models)


def test_packed_and_model_layers():
    """The packed and model layers on the tiny synthetic corpus, every video with its Viterbi transcript among four candidates
    (one of them twice): the trie's log Z_g is the logsumexp of the distinct candidates' log Z_a, the candidate posteriors are
    their softmax, add up to 1 and give a repeated candidate's mass to its first index; candidates no one of which fits give
    -inf and zeros; ambiguous='raise' names the video."""
    from action_segmentation_amd import ops, synth
    from action_segmentation_amd.semimarkov import SemiMarkovModel
    from action_segmentation_amd.semimarkov_utils import spans_to_transcripts
    import train_ref as R
    data = synth.SynthDatasplit('tiny', seed=11)
    fitted = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=False, batch_size=2), data)
    fitted.fit(data, use_labels=True)
    model = SemiMarkovModel.from_args(synth.make_args(data.max_k, cuda=True, batch_size=2), data)
    model.model.load_state_dict(fitted.model.state_dict(), strict=False)
    mod = model.model.cuda()
    pc = model.prepare(data)
    t = pc.tables
    elp, _ = ops.emission(pc.batch, pc.x, t['w'], t['cst'], t['inv_var'], cons=pc.cons)
    out = ops.viterbi(pc.batch, elp, t['trans'], t['init'], t['len'], endpen=pc.endpen, class_map=t['class_map'])
    torch.cuda.synchronize()
    tr = [[int(v) for v in a] for a in spans_to_transcripts(out['spans'], pc.lengths)]
    cands = {n: [a, a[:-1] if len(a) > 1 else a + a, a, a + a[-1:], a[::-1] + a[:1]] for n, a in zip(pc.video_names, tr)}
    names = list(pc.video_names)
    # the distinct candidates one by one
    each = {}
    for j in range(5):
        zj = mod.transcript_scores_packed(pc, [cands[n][j] for n in names]).numpy()
        for i, n in enumerate(names):
            each.setdefault(n, []).append(zj[i])
    graphs = [ops.TranscriptGraph.from_candidates(cands[n]) for n in names]
    zg = mod.transcript_graph_log_partition_packed(pc, graphs)
    assert zg.requires_grad and zg.dtype == torch.float64 and zg.shape == (len(names),)
    mod.zero_grad()
    zg.sum().backward()
    assert all(getattr(mod, n).grad is not None and bool(getattr(mod, n).grad.abs().max() > 0) for n in R.PARAMS)
    got = model.candidate_log_likelihood(data, cands)
    cond = model.candidate_log_likelihood(data, cands, conditional=True)
    post = model.candidate_posteriors(data, cands)
    zgh = zg.detach().cpu().numpy()
    for i, n in enumerate(names):
        z = np.array(each[n])
        first = [j for j in range(5) if cands[n].index(cands[n][j]) == j]
        fin = [j for j in first if np.isfinite(z[j])]
        want = z[fin].max() + np.log(np.exp(z[fin] - z[fin].max()).sum())
        assert abs(zgh[i] - want) <= Z_BAR * max(1.0, abs(want)) and abs(got[n] - zgh[i]) <= 1e-9 * max(1.0, abs(want)), n
        assert cond[n] <= 1e-6 and np.isfinite(cond[n]), n
        p = post[n]
        assert p.dtype == np.float64 and p.shape == (5,) and abs(p.sum() - 1.0) <= 1e-9, n
        soft = np.zeros(5)
        soft[fin] = np.exp(z[fin] - want)
        assert np.abs(p - soft).max() <= ELP_BAR and all(p[j] == 0.0 for j in range(5) if j not in first), (n, p, soft)
    # no candidate fits: more entries than frames
    none = dict(cands)
    none[names[0]] = [[tr[0][0]] * (int(pc.lengths[0]) + 1)] if int(pc.lengths[0]) < ops.MAX_TRANSCRIPT else cands[names[0]]
    if int(pc.lengths[0]) < ops.MAX_TRANSCRIPT:
        assert model.candidate_log_likelihood(data, none)[names[0]] == -np.inf
        assert not model.candidate_posteriors(data, none)[names[0]].any()
    # ambiguous='raise' on the host, by name
    bad = list(graphs)
    bad[1] = ops.TranscriptGraph.from_optional([tr[1][0], tr[1][-1], tr[1][0]], [1, 1, 1])
    with pytest.raises(ValueError, match=str(names[1])):
        mod.transcript_graph_log_partition_packed(pc, bad)
    z_allow = mod.transcript_graph_scores_packed(pc, bad, ambiguous='allow').numpy()
    others = [i for i in range(len(names)) if i != 1]
    assert np.abs(z_allow[others] - zgh[others]).max() <= 1e-9 * np.abs(zgh).max() and not np.isnan(z_allow[1])
    p_used, p_end = mod.transcript_node_posteriors_packed(pc, graphs)
    for i, g in enumerate(graphs):
        assert p_used[i].shape == p_end[i].shape == (len(g),) and abs(p_end[i].sum() - 1.0) <= 1e-9
        assert p_used[i].max() <= 1.0 + ELP_BAR and abs(p_used[i][g.start].sum() - 1.0) <= ELP_BAR
