"""The expected reward under the transcript-graph posterior and its gradient on the GPU (smm_align_graph_expected_reward_f64,
smm_align_graph_expected_reward_bwd_f64) against the two routes of tests/transcript_expected_reward_ref.py: (a) autograd through
the enumeration on the tiny graphs, (b) log Z_g differentiated twice on the shapes that cross a work split.

Bars.  Gradients: worst |error| / max(1, max |ref|) over the four tables <= 1e-4, the project's bar.  Values (the value call,
V- and V+): 1e-5 max(1, sum |reward| over the covered entries + sum |node_reward|) against the reference: the rounding of a sum
of posteriors times rewards scales with the sum of |reward|, and the forward columns carry about 6e-8 relative per
column.  Every test prints its figures ("[transcript-expected-reward] ...") before it asserts; DESIGN 4v lists them."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_transcript_entropy_grad as GG
import test_gpu_transcript_graph as GT
import test_gpu_transcript_kl as GK
import test_gpu_transcript_sample as GS
import transcript_expected_reward_ref as R
from test_gpu_transcript_graph import Case, _lists, _ops, _tables, _tuple

pytestmark = pytest.mark.gpu
TAB_BAR, VAL_BAR = 1e-4, 1e-5
KEYS = R.KEYS
SETTINGS = ('frames', 'nodes', 'both')


# ------------------------------------------------------------------------------------------------ rewards
def draw_rewards(case, seed, setting='both'):
    """N(0, 1) rewards per video: [(reward [T, C_g] or None, node_reward [M] or None)]."""
    rng = np.random.default_rng(seed)
    out = []
    for e, g, _ in case.vids:
        w, nr = rng.normal(size=e.shape), rng.normal(size=len(g))
        out.append((w if setting != 'nodes' else None, nr if setting != 'frames' else None))
    return out


def device_rewards(case, rewards):
    """-> (reward fp64 [total_frames, c_max] or None, node_reward fp64 [n_nodes] or None) on the device."""
    dev = torch.device('cuda:0')
    reward = node = None
    if rewards[0][0] is not None:
        w = np.zeros((int(case.off[-1]), case.cm))
        for i, (r, _) in enumerate(rewards):
            w[case.off[i]:case.off[i + 1], :r.shape[1]] = r
        reward = torch.tensor(w, dtype=torch.float64, device=dev)
    if rewards[0][1] is not None:
        node = torch.tensor(np.concatenate([nr for _, nr in rewards]), dtype=torch.float64, device=dev)
    return reward, node


def scales(case, rewards):
    return np.array([R.abs_reward(None, case.lengths[i], case.n_states[case.vids[i][2]], *rewards[i]) for i in range(len(case.vids))])


# ------------------------------------------------------------------------------------------------ launching
def _value(case, rewards, batch, d, f, scratch=None):
    w, nr = device_rewards(case, rewards) if isinstance(rewards, list) else rewards      # (a list: one pair per video)
    return _ops().align_graph_expected_reward(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, f['logz'], reward=w,
                                              node_reward=nr, endpen=d['endpen'], ws=f['ws'], staged=f['_staged'], scratch=scratch,
                                              want_parts=True)


def _grad(case, rewards, batch, d, f, u='case', scratch=None):
    w, nr = device_rewards(case, rewards) if isinstance(rewards, list) else rewards      # (a list: one pair per video)
    return _ops().align_graph_expected_reward_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, f['logz'], reward=w,
                                                  node_reward=nr, grad_out=d['u'] if isinstance(u, str) else u, endpen=d['endpen'],
                                                  ws=f['ws'], staged=f['_staged'], scratch=scratch, want_value=True)


def _run(case, rewards, fill=None):
    """One forward launch, the value call, the gradient call -> numpy dict(elp, trans, init, len, value (V-), value_plus, call
    (the value call's), parts, err)."""
    batch, d, f = GS._forward(case, fill)
    v = _value(case, rewards, batch, d, f)
    err_v = _ops().error_flag(batch, v)
    g = _grad(case, rewards, batch, d, f)
    h = {k: g[k].cpu().numpy() for k in KEYS + ('value', 'value_plus')}
    h.update(call=v['value'].cpu().numpy(), parts=v['parts'].cpu().numpy(), err=max(err_v, _ops().error_flag(batch, g)))
    return h


def reference(case, rewards, route):
    """-> (V [b], dict(elp [total, cm], trans, init, len [g, ...])) by ``route`` per video, times u, summed per group."""
    g_n, cm = len(case.tabs), case.cm
    val = np.zeros(len(case.vids))
    g = dict(elp=np.zeros((int(case.off[-1]), cm)), trans=np.zeros((g_n, cm, cm)), init=np.zeros((g_n, cm)),
             len=np.zeros((g_n, case.k_rows, cm)))
    for i, (e, gr, j) in enumerate(case.vids):
        c = case.n_states[j]
        val[i], gi = route(GK.side(case, i), _tuple(gr), case.kp(i), *rewards[i])
        u = 1.0 if case.u is None else float(case.u[i])
        g['elp'][case.off[i]:case.off[i + 1], :c] += u * gi['elp']
        g['trans'][j, :c, :c] += u * gi['trans']
        g['init'][j, :c] += u * gi['init']
        g['len'][j, :, :c] += u * gi['len']
    return val, g


def _check(what, case, rewards, h, val, ref, zero=(), premise=True):
    """The bars; and the premise of the relative bar, from the reference alone: every reference table has an entry of at least
    1e-2, but for the tables ``zero`` declares zero by structure."""
    e = {k: float(np.abs(h[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())) for k in KEYS}
    sc = np.maximum(1.0, scales(case, rewards))
    ev = {k: float((np.abs(h[k] - val) / sc).max()) for k in ('call', 'value', 'value_plus')}
    ep = float(np.abs(h['parts'].sum(axis=1) - h['call']).max())
    print('\n[transcript-expected-reward] %-40s elp %.1e trans %.1e init %.1e len %.1e (bar %.0e)  V: the value call %.1e, V- %.1e, '
          'V+ %.1e (bar %.0e of sum |r| <= %.3g)  max|ref| %s' % (what, e['elp'], e['trans'], e['init'], e['len'], TAB_BAR, ev['call'],
                                                                ev['value'], ev['value_plus'], VAL_BAR, sc.max(),
                                                                ' '.join('%.2g' % np.abs(ref[k]).max() for k in KEYS)))
    assert h['err'] == 0
    assert not premise or all(np.abs(ref[k]).max() >= 1e-2 for k in KEYS if k not in zero), what
    assert max(e.values()) <= TAB_BAR and max(ev.values()) <= VAL_BAR
    assert ep <= 1e-12 * sc.max()
    return e


# ------------------------------------------------------------------------------------------------ 1. tiny graphs
TINY_SEED = 7


@functools.lru_cache(None)
def tiny_reference(which, setting):
    case = GS.exact_cases()[which][1]
    rewards = draw_rewards(case, TINY_SEED + which, setting)
    return case, rewards, reference(case, rewards, R.enumeration_reward)


@pytest.mark.parametrize('setting', SETTINGS)
@pytest.mark.parametrize('which', [0, 1], ids=['k_rows4', 'k_rows8'])
def test_tiny_graphs_against_enumeration(which, setting):
    """The sampler's tiny graphs (eight videos, one of them under end penalties): V by the value call, V-, V+ and the four
    gradients against autograd through the enumerated expectation; frame rewards, node rewards, both."""
    case, rewards, (val, ref) = tiny_reference(which, setting)
    _check('tiny %s %s' % (('k_rows4', 'k_rows8')[which], setting), case, rewards, _run(case, rewards), val, ref)


def masked_case(mask):
    """A diamond and a trie with one arm cut by a -1e9 or -inf transition."""
    G = _ops().TranscriptGraph
    rng = np.random.default_rng(39)
    C, K = 3, 5
    vids = [(rng.normal(size=(7, C)) * 1.2, _lists(4, [[], [0], [0], [1, 2]], [0], [3], ids=[0, 1, 2, 0]), 0),
            (rng.normal(size=(6, C)) * 1.2, G.from_candidates([[0, 1, 2], [0, 2, 1], [1, 0]]), 1)]
    r = np.random.default_rng(40)
    t1, t2 = _tables(r, C, K, 1.2), _tables(r, C, K, 1.2)
    t1['trans'][1, 0] = mask
    t2['trans'][2, 0] = mask
    return Case(vids, [t1, t2], K, kps=[5, 5])


@pytest.mark.parametrize('mask', [-1e9, -np.inf], ids=['m1e9', 'minf'])
def test_masked_entries_against_enumeration(mask):
    """The cut entries carry no occurrence with mass: exactly 0.0."""
    case = masked_case(mask)
    rewards = draw_rewards(case, 41)
    val, ref = reference(case, rewards, R.enumeration_reward)
    h = _run(case, rewards)
    _check('masked %s' % mask, case, rewards, h, val, ref)
    assert h['trans'][0, 1, 0] == 0.0 and h['trans'][1, 2, 0] == 0.0


# ------------------------------------------------------------------------------------------------ 2. work splits
BIG_SEED = 11
# name -> the tables that are zero by structure; the builders and their seeds are the entropy gradient's
BIG_CASES = {name: zero for name, (_, _, zero) in GG.BIG_CASES.items()}


def big_case(name):
    case = GG.BIG_CASES[name][0]()
    return case, draw_rewards(case, BIG_SEED)


@pytest.mark.parametrize('name', list(BIG_CASES))
def test_work_splits_against_the_identity(name):
    """The smallest shapes that cross each boundary, against log Z_g differentiated twice with a class per node; frame and node
    rewards together.  A table that is zero by structure (the chain's g_trans and g_init) is held to the same absolute 1e-4;
    what is left in it is printed."""
    zero = BIG_CASES[name]
    case, rewards = big_case(name)
    val, ref = reference(case, rewards, R.identity_reward)
    h = _run(case, rewards)
    _check(name, case, rewards, h, val, ref, zero=zero)
    for k in zero:
        print('\n[transcript-expected-reward] ... %s is zero by structure: max |g| %.1e' % (k, np.abs(h[k]).max()))
        assert np.abs(h[k]).max() <= TAB_BAR


# ------------------------------------------------------------------------------------------------ 3. a packed corpus
def _corpus_rewards(case, bad):
    """The healthy videos' rewards are the same draws in both corpora."""
    good = draw_rewards(GG._corpus(False, None), 17)
    if not bad:
        return good
    rng = np.random.default_rng(18)
    extra = [(rng.normal(size=case.vids[i][0].shape), rng.normal(size=len(case.graphs[i]))) for i in (1, 4)]
    return [good[0], extra[0], good[1], good[2], extra[1], good[3]]


def test_a_packed_corpus_with_an_upstream_zero_and_bad_videos():
    """6 and 17 states under c_max 17, ragged, per-video span limits, u = (0.7, 0, -1.3, 2); then the same corpus with a video
    without an alignment and a NaN video between the healthy ones; then with a reward that is not finite."""
    u = [0.7, 0.0, -1.3, 2.0]
    good = GG._corpus(False, u)
    rewards = _corpus_rewards(good, False)
    val, ref = reference(good, rewards, R.identity_reward)
    h = _run(good, rewards)
    _check('packed corpus', good, rewards, h, val, ref)
    o = good.off
    assert not h['elp'][o[1]:o[2]].any() and not np.signbit(h['elp'][o[1]:o[2]]).any()      # (u = 0: exact zeros)
    bad = GG._corpus(True, u)
    hb = _run(bad, _corpus_rewards(bad, True))
    ob = bad.off
    print('\n[transcript-expected-reward] bad videos: values %s / %s, error word %d' % (hb['call'], hb['value'], hb['err']))
    assert hb['err'] != 0
    for k in ('call', 'value', 'value_plus'):
        assert np.isnan(hb[k][1]) and np.isnan(hb[k][4]), k
    assert not hb['elp'][ob[1]:ob[2]].any() and not hb['elp'][ob[4]:ob[5]].any()
    for i, j in zip(range(4), (0, 2, 3, 5)):
        assert np.array_equal(h['elp'][o[i]:o[i + 1]].view(np.int64), hb['elp'][ob[j]:ob[j + 1]].view(np.int64))
        assert all(h[k][i] == hb[k][j] for k in ('call', 'value', 'value_plus'))
        assert np.array_equal(h['parts'][i], hb['parts'][j])
    for k in ('trans', 'init', 'len'):
        assert np.array_equal(h[k].view(np.int64), hb[k].view(np.int64)), k
    # the error word is the NaN video's alone: without it the word stays clear
    only = Case([bad.vids[i] for i in (0, 1, 2)], bad.tabs, 12, kps=[bad.kps[i] for i in (0, 1, 2)])
    ho = _run(only, _corpus_rewards(bad, True)[:3])
    assert ho['err'] == 0 and np.isnan(ho['call'][1]) and np.isnan(ho['value'][1]) and not ho['elp'][only.off[1]:only.off[2]].any()


@pytest.mark.parametrize('where', ['frame', 'node'])
def test_a_reward_that_is_not_finite_poisons_its_video_alone(where):
    """Video 2 (group 0) carries an inf in a covered reward entry, or a NaN on one of its nodes: its values are NaN, its g_elp rows
    and its group's tables are NaN, the error word is set.  The other videos keep their values and rows, the other group its
    tables, bit for bit.  An inf in a column past the video's state count is not read."""
    u = [0.7, 0.0, -1.3, 2.0]
    good = GG._corpus(False, u)
    rewards = _corpus_rewards(good, False)
    h = _run(good, rewards)
    batch, d, f = GS._forward(good)
    w, nr = device_rewards(good, rewards)
    w[good.off[2] + 3, 6:] = float('inf')                        # (video 2 has 6 states: columns 6 .. 16 are not its own)
    clean = _value(good, (w, nr), batch, d, f)
    assert torch.equal(clean['value'].cpu(), torch.tensor(h['call'])) and _ops().error_flag(batch, clean) == 0
    if where == 'frame':
        w[good.off[2] + 3, 2] = float('inf')
    else:
        nr[GS._node_offsets(good)[2] + 1] = float('nan')
    v = _value(good, (w, nr), batch, d, f)
    err_v = _ops().error_flag(batch, v)
    g = _grad(good, (w, nr), batch, d, f)
    err_g = _ops().error_flag(batch, g)
    hb = {k: g[k].cpu().numpy() for k in KEYS + ('value', 'value_plus')}
    hb['call'] = v['value'].cpu().numpy()
    print('\n[transcript-expected-reward] a reward that is not finite (%s): values %s / %s, error words %d %d'
          % (where, hb['call'], hb['value'], err_v, err_g))
    assert err_v != 0 and err_g != 0
    o = good.off
    for k in ('call', 'value', 'value_plus'):
        assert np.isnan(hb[k][2]) and all(hb[k][i] == h[k][i] for i in (0, 1, 3)), k
    assert np.isnan(hb['elp'][o[2]:o[3], :6]).all()
    for i in (0, 1, 3):
        assert np.array_equal(h['elp'][o[i]:o[i + 1]].view(np.int64), hb['elp'][o[i]:o[i + 1]].view(np.int64))
    for k in ('trans', 'init', 'len'):
        assert np.array_equal(h[k][1].view(np.int64), hb[k][1].view(np.int64)), k
    assert np.isnan(hb['trans'][0][:6, :6]).all() and np.isnan(hb['init'][0][:6]).all() and np.isnan(hb['len'][0][:, :6]).all()


# ------------------------------------------------------------------------------------------------ 4. identities
def _backward(case, batch, d, f, u=None):
    return _ops().align_graph_logz_bwd(batch, d['elp'], d['trans'], d['init'], d['len'], case.graphs, f['logz'], grad_logz=u,
                                       endpen=d['endpen'], ws=f['ws'], staged=f['_staged'], want_node_prob=True, want_end_prob=True)


def test_a_reward_of_one_on_every_class_counts_the_frames():
    """V = T whatever the alignment, so the gradient vanishes: held to 1e-4 absolute."""
    for which in (0, 1):
        case = GS.exact_cases()[which][1]
        rewards = [(np.ones(e.shape), None) for e, _, _ in case.vids]
        h = _run(case, rewards)
        T = np.array(case.lengths, np.float64)
        ev = max(float((np.abs(h[k] - T) / T).max()) for k in ('call', 'value', 'value_plus'))
        worst = max(float(np.abs(h[k]).max()) for k in KEYS)
        print('\n[transcript-expected-reward] reward = 1, %d: V against T %.1e (bar %.0e), max |g| %.1e (bar %.0e)'
              % (which, ev, VAL_BAR, worst, TAB_BAR))
        assert h['err'] == 0 and ev <= VAL_BAR and worst <= TAB_BAR


def test_a_node_reward_of_one_on_a_chain_counts_its_nodes():
    """Every alignment of a chain crosses every node: V = M and there is no gradient."""
    rng = np.random.default_rng(4)
    C, K, M = 4, 6, 9
    case = Case([(rng.normal(size=(21, C)) * 2, _ops().TranscriptGraph.chain(rng.integers(0, C, M)), 0)], [_tables(rng, C, K, 2.0)], K)
    h = _run(case, [(None, np.ones(M))])
    ev = max(abs(float(h[k][0]) - M) / M for k in ('call', 'value', 'value_plus'))
    worst = max(float(np.abs(h[k]).max()) for k in KEYS)
    print('\n[transcript-expected-reward] node_reward = 1 on a chain of %d: V against M %.1e (bar %.0e), max |g| %.1e (bar %.0e)'
          % (M, ev, VAL_BAR, worst, TAB_BAR))
    assert h['err'] == 0 and ev <= VAL_BAR and worst <= TAB_BAR


def test_one_hot_rewards_are_the_backward_call_s_posteriors():
    """On a trie none of whose candidates is a prefix of another, node_reward = onehot(end node j): V = p_end[j], that
    candidate's posterior (an end node with a successor is crossed by longer candidates too: its V is node_prob[j]).
    reward = onehot(column c): V = sum_t g_elp[t][c]."""
    one = masked_case(-1.0)                                          # (an ordinary entry: nothing is cut)
    one = Case([(e, g, 0) for e, g, _ in one.vids[1:]], one.tabs[1:], one.k_rows, kps=[5])
    graph = one.graphs[0]
    batch, d, f = GS._forward(one)
    bw = _backward(one, batch, d, f)
    p_end, p_used, g_elp = bw['end_prob'][0].cpu().numpy(), bw['node_prob'][0].cpu().numpy(), bw['elp'].cpu().numpy()
    ends = np.flatnonzero(np.asarray(graph.end))
    assert len(ends) == 3 and not np.asarray(graph.pred)[:, ends].any() and p_end[ends].min() > 1e-3
    for j in range(len(graph)):
        nr = np.zeros(len(graph))
        nr[j] = 1.0
        v = float(_value(one, [(None, nr)], batch, d, f)['value'][0])
        print('\n[transcript-expected-reward] onehot(node %d): V %.12f against p_used %.12f, p_end %.12f' % (j, v, p_used[j], p_end[j]))
        assert abs(v - p_used[j]) <= VAL_BAR and (j not in ends or abs(v - p_end[j]) <= VAL_BAR)
    for c in range(one.n_states[0]):
        w = np.zeros(one.vids[0][0].shape)
        w[:, c] = 1.0
        v = float(_value(one, [(w, None)], batch, d, f)['value'][0])
        print('\n[transcript-expected-reward] onehot(column %d): V %.12f against sum_t g_elp %.12f' % (c, v, g_elp[:, c].sum()))
        assert abs(v - g_elp[:, c].sum()) <= VAL_BAR * one.lengths[0]


def test_the_value_is_linear_in_the_rewards_and_the_hessian_is_symmetric():
    """V(a r1 + b r2) = a V(r1) + b V(r2) to 1e-9 of the scale; <w1, g_elp(w2)> = <w2, g_elp(w1)> within the gradient bar times
    ||w||: g_elp(w) is the Hessian of log Z_g applied to w."""
    case = GS.exact_cases()[0][1]
    batch, d, f = GS._forward(case)
    r1, r2 = draw_rewards(case, 51), draw_rewards(case, 52)
    a, b = 0.7, -1.9
    mix = [(a * w1 + b * w2, a * n1 + b * n2) for (w1, n1), (w2, n2) in zip(r1, r2)]
    v1, v2, vm = (_value(case, r, batch, d, f)['value'].cpu().numpy() for r in (r1, r2, mix))
    sc = np.maximum(1.0, abs(a) * scales(case, r1) + abs(b) * scales(case, r2))
    lin = float((np.abs(vm - (a * v1 + b * v2)) / sc).max())
    print('\n[transcript-expected-reward] linearity: %.1e of the scale (bar 1e-9)' % lin)
    assert lin <= 1e-9
    f1, f2 = [(w, None) for w, _ in r1], [(w, None) for w, _ in r2]
    g1, g2 = (_grad(case, r, batch, d, f, u=None)['elp'].cpu().numpy() for r in (f1, f2))
    w1, w2 = (device_rewards(case, r)[0].cpu().numpy() for r in (f1, f2))
    lhs, rhs = float((w1 * g2).sum()), float((w2 * g1).sum())
    norm = float(np.sqrt((w1 ** 2).sum()) * np.sqrt((w2 ** 2).sum()))
    print('\n[transcript-expected-reward] Hessian symmetry: %.10f against %.10f, |difference| %.1e (bar %.0e ||w1|| ||w2|| = %.1e)'
          % (lhs, rhs, abs(lhs - rhs), TAB_BAR, TAB_BAR * norm))
    assert abs(lhs - rhs) <= TAB_BAR * norm and abs(lhs) > 1e-2


def test_expected_accuracy_and_expected_errors_add_up_to_the_frames():
    case = GS.exact_cases()[0][1]
    batch, d, f = GS._forward(case)
    rng = np.random.default_rng(5)
    hit, miss = [], []
    for e, _, _ in case.vids:
        onehot = np.eye(e.shape[1])[rng.integers(0, e.shape[1], e.shape[0])]
        hit.append((onehot, None))
        miss.append((1.0 - onehot, None))
    va, vb = (_value(case, r, batch, d, f)['value'].cpu().numpy() for r in (hit, miss))
    T = np.array(case.lengths, np.float64)
    err = float((np.abs(va + vb - T) / T).max())
    print('\n[transcript-expected-reward] accuracy + errors against T: %.1e (bar %.0e)' % (err, VAL_BAR))
    assert err <= VAL_BAR and (va > 0).all() and (vb > 0).all()


# ------------------------------------------------------------------------------------------------ 5. bits
def _bits(t):
    return t.contiguous().view(torch.int64)


def _same(a, b, keys):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in keys)


def test_two_calls_and_poisoned_workspaces_and_scratch_give_the_same_bits():
    """The forward workspace AND the caller's scratch filled with 0x00 or 0xFF bytes before the calls: no kernel reads an eta, D,
    part, prefix-sum or partial cell (or a column cell) that was not written first; two calls give the same bits."""
    case = GS.exact_cases()[0][1]
    rewards = draw_rewards(case, 61)
    ops = _ops()
    vals, grads = [], []
    for fill in (0, 0xFF, 0):
        batch, d, f = GS._forward(case, fill)
        off = GS._node_offsets(case)
        need_v, need_g = ops.align_graph_expected_reward_scratch_bytes(batch, off), ops.align_graph_expected_reward_bwd_scratch_bytes(batch, off)
        for _ in range(2):
            sv = torch.full((need_v,), fill, dtype=torch.uint8, device='cuda:0')
            sg = torch.full((need_g,), fill, dtype=torch.uint8, device='cuda:0')
            v = _value(case, rewards, batch, d, f, scratch=sv)
            g = _grad(case, rewards, batch, d, f, scratch=sg)
            assert v['_keep'][1] is sv and g['_keep'][1] is sg
            vals.append({k: v[k].clone() for k in ('value', 'parts')})
            grads.append({k: g[k].clone() for k in KEYS + ('value', 'value_plus')})
    assert bool(torch.isfinite(grads[0]['elp']).all()) and float(grads[0]['elp'].abs().max()) > 1e-2
    assert all(_same(vals[0], o, ('value', 'parts')) for o in vals[1:])
    assert all(_same(grads[0], o, KEYS + ('value', 'value_plus')) for o in grads[1:])


def test_the_calls_change_nothing_of_the_other_calls_results():
    """A backward call, sampler draws, the entropy, the segment posteriors and the KL, bit for bit, before and after."""
    _, pc, qc, _, _, _, _ = GK.tiny_pairs()[0]
    batch, dp, fp = GS._forward(pc)
    _, dq, fq = GS._forward(qc)
    rewards = draw_rewards(pc, 62)

    def everything():
        g = GK._backward(pc, batch, dp, fp)
        out = [g[k] for k in KEYS] + [torch.cat(g['node_prob']), torch.cat(g['end_prob'])]
        s = GS._draw(pc, batch, dp, fp, 16, seed=3)
        out += [s['spans'], s['logp']]
        out.append(GK._entropy(pc, batch, dp, fp)['entropy'])
        sp = _ops().align_graph_segment_posteriors(batch, dp['elp'], dp['trans'], dp['init'], dp['len'], pc.graphs, fp['logz'],
                                                  spans=s['spans'], used=s['used'], endpen=dp['endpen'], ws=fp['ws'],
                                                  staged=fp['_staged'], want_dense=True)
        out += [sp['seg_logp'], sp['node_end_post'], sp['node_start_post'], torch.cat(sp['end_mean'])]
        out.append(GK._kl(pc, batch, dp, fp, dq, fq)['kl'])
        e = GG._launch(pc, None, 'entropy', batch, dp, fp)
        out += [e[k] for k in KEYS]
        return [t.clone() for t in out]

    before = everything()
    _value(pc, rewards, batch, dp, fp)
    _grad(pc, rewards, batch, dp, fp)
    after = everything()
    for x, y in zip(before, after):
        assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))


def test_a_captured_graph_replays_the_same_bits():
    case = GS.exact_cases()[0][1]
    batch, d, f = GS._forward(case)
    rewards = device_rewards(case, draw_rewards(case, 63))
    keys_v, keys_g = ('value', 'parts'), KEYS + ('value', 'value_plus')
    eager_v, eager_g = _value(case, rewards, batch, d, f), _grad(case, rewards, batch, d, f)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _value(case, rewards, batch, d, f)                          # (warm-up on the capture stream)
        _grad(case, rewards, batch, d, f)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            cap_v = _value(case, rewards, batch, d, f)
            cap_g = _grad(case, rewards, batch, d, f)
    torch.cuda.current_stream().wait_stream(side)
    for k in keys_v:
        cap_v[k].fill_(float('nan'))
    for k in KEYS:
        cap_g[k].fill_(float('nan'))
    graph.replay()
    torch.cuda.synchronize()
    assert _same(eager_v, cap_v, keys_v) and _same(eager_g, cap_g, keys_g)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_come_before_a_device_is_touched():
    """Every tensor is a CPU tensor: no call gets as far as using one."""
    ops = _ops()
    batch = ops.Batch([6, 5], [3], 4)
    G = ops.TranscriptGraph
    graphs = [G.chain([0, 1]), G.from_candidates([[2, 2, 1], [2, 0]])]
    z = torch.zeros(1, dtype=torch.float64)
    n = sum(len(g) for g in graphs)
    w, nr = torch.zeros((11, 3), dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    e = torch.zeros((11, 3), dtype=torch.float64)
    big = torch.zeros(ops.align_graph_logz_workspace_bytes(batch, np.array([0, 2, n], np.int64)), dtype=torch.uint8)
    short = torch.zeros(16, dtype=torch.uint8)
    staged = (torch.zeros(n - 1, dtype=torch.int32), torch.zeros(8 * (n - 1), dtype=torch.int32), torch.zeros(n - 1, dtype=torch.uint8))
    good = (torch.zeros(n, dtype=torch.int32), torch.zeros(8 * n, dtype=torch.int32), torch.zeros(n, dtype=torch.uint8))
    for name in ('align_graph_expected_reward', 'align_graph_expected_reward_bwd'):
        call = getattr(ops, name)
        with pytest.raises(ValueError, match="%s: pass reward, node_reward or both" % name):
            call(batch, e, z, z, z, graphs, z, ws=big, staged=good)
        with pytest.raises(ValueError, match="%s: scratch must be a uint8 tensor of at least" % name):
            call(batch, e, z, z, z, graphs, z, reward=w, node_reward=nr, ws=big, staged=good, scratch=short)
        with pytest.raises(ValueError, match="%s: add_eos" % name):
            call(ops.Batch([6, 5], [3], 4, no_eos=True), e, z, z, z, graphs, z, reward=w, ws=big, staged=good)
        with pytest.raises(ValueError, match="%s: staged" % name):
            call(batch, e, z, z, z, graphs, z, reward=w, ws=big, staged=staged)
        with pytest.raises(ValueError, match="%s: 1 graphs for 2 videos" % name):
            call(batch, e, z, z, z, graphs[:1], z, reward=w, ws=big)
        for ws in (None, short):
            with pytest.raises(ValueError, match="%s: pass the workspace" % name):
                call(batch, e, z, z, z, graphs, z, reward=w, ws=ws, staged=good)
        with pytest.raises(ValueError, match="%s: node_reward must be fp64 \\[%d\\]" % (name, n)):
            call(batch, e, z, z, z, graphs, z, node_reward=nr[:n - 1], ws=big, staged=good)
        with pytest.raises(ValueError, match="%s: reward must be fp64" % name):
            call(batch, e, z, z, z, graphs, z, reward=w[:5], ws=big, staged=good)
