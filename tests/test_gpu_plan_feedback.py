"""Plan feedback of smm_decode_f32 (csrc/smm_api.hip, "Plan feedback"): a resident plan with a stream split is re-planned from
the start and end stamps its DP workgroups leave, and nothing but the schedule changes.

Two small launches that choose_split splits under SMM_SPLIT_MIN_US=0 (threshold: the longest video - 400 frames, the emission
term is a frame or two at these sizes; both corpora keep 50 frames clear of it):
  ring   40 videos of 24..600 frames, groups of 3 and 6 states, D = 8, span limit 16 (ring kernel, window back-trace);
         10 videos of 250 frames and more are the first part
  band   24 videos of 700..2400 frames, groups of 5 and 17 states, D = 16, K = 1024 (BAND mode); 6 videos of 2050 frames and more
Each is decoded four times from one resident plan with SMM_PLAN_FEEDBACK=2: the first call is the first sighting, the second admits
the plan and is measured, the third takes the measurement and re-plans behind its own launches, the fourth runs the new plan."""
import functools

import numpy as np
import pytest
import torch

from oracle import dense_ref as O
from oracle import factored as F

pytestmark = pytest.mark.gpu

SWITCHES = ('SMM_NO_SPLIT', 'SMM_SPLIT_MIN_US', 'SMM_CHUNK', 'SMM_CHUNK_P', 'SMM_SMALL_WG', 'SMM_PLAN_CACHE', 'SMM_SPLIT_NS',
            'SMM_SPLIT_MARGIN', 'SMM_CHUNK_WC', 'SMM_CHUNK_LMIN', 'SMM_PLAN_FEEDBACK')
CASES = {
    #        b   long videos (first part)   the others        states   D   K
    'ring': (40, 10, (250, 600),            (24, 150),        (3, 6),  8,  16),
    'band': (24, 6,  (2050, 2400),          (700, 1900),      (5, 17), 16, 1024),
}


@functools.lru_cache(maxsize=None)
def corpus(case):
    """Host arrays of the launch, HSMM-sampled as tests/decode_corpus.py does it: the lengths hit both ends of both ranges."""
    from scipy.special import gammaln
    b, n_long, long_t, short_t, states, d, k = CASES[case]
    g = np.random.default_rng(11 + b)
    lengths = np.concatenate([[long_t[0], long_t[1]], g.integers(long_t[0], long_t[1] + 1, size=n_long - 2),
                              [short_t[0], short_t[1]], g.integers(short_t[0], short_t[1] + 1, size=b - n_long - 2)])
    lengths = lengths[g.permutation(b)].astype(np.int64)
    group = (np.arange(b) % len(states)).astype(np.int32)
    c_max = max(states)
    kp = np.minimum(k, lengths).astype(np.int32)
    frame_off = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    total = int(lengths.sum())
    sigma = g.uniform(0.7, 1.3, size=d)
    var = sigma ** 2
    lognorm = float(-0.5 * np.log(var).sum() - 0.5 * d * np.log(2 * np.pi))
    kk = np.arange(k)[:, None]
    par = []
    for c in states:
        mu = g.normal(0, 0.9, size=(c, d))
        rates = g.uniform(3, 12, size=c) if k <= 64 else g.uniform(20, 400, size=c)
        trans = np.log(g.dirichlet(np.ones(c) * 0.5, size=c).T + 1e-3)
        trans -= np.log(np.exp(trans).sum(0, keepdims=True))
        par.append(dict(c=c, mu=mu, rates=rates, mu_hat=mu + g.normal(0, 0.02, size=mu.shape), trans=trans,
                        init=np.log(g.dirichlet(np.ones(c))), lens=kk * np.log(rates) - rates - gammaln(kk + 1)))
    x = np.zeros((total, d), np.float32)
    for i in range(b):
        p = par[group[i]]
        lab, cur = [], int(g.integers(0, p['c']))
        while sum(map(len, lab)) < lengths[i]:
            lab.append(np.full(int(np.clip(g.poisson(p['rates'][cur]), 1, k - 1)), cur))
            cur = (cur + 1) % p['c']
        lab = np.concatenate(lab)[:lengths[i]]
        x[frame_off[i]:frame_off[i] + lengths[i]] = (p['mu'][lab] + sigma * g.standard_normal((len(lab), d))).astype(np.float32)
    n_groups = len(states)
    w = np.zeros((n_groups, d, c_max)); cst = np.zeros((n_groups, c_max))
    trans = np.full((n_groups, c_max, c_max), -1e9); init = np.full((n_groups, c_max), -1e9)
    lens = np.full((n_groups, k, c_max), -1e9)
    for gi, p in enumerate(par):
        c = p['c']
        w[gi, :, :c] = (p['mu_hat'] / var).T
        cst[gi, :c] = lognorm - 0.5 * (p['mu_hat'] ** 2 / var).sum(1)
        trans[gi, :c, :c], init[gi, :c], lens[gi, :, :c] = p['trans'], p['init'], p['lens']
    return dict(b=b, lengths=lengths, group=group, kp=kp, frame_off=frame_off, total=total, states=states, c_max=c_max, d=d, k=k,
                x=x, w=w, cst=cst, inv_var=1.0 / var, trans=trans, init=init, lens=lens, par=par, n_long=n_long)


def test_the_shipped_threshold_takes_the_long_videos():
    """choose_split's rule restated (as tests/test_decode_plans_host.py does): what the cases above promise about the first plan."""
    for case in CASES:
        cp = corpus(case)
        em_us = cp['total'] * (4.0 * cp['d'] + 8.0 * cp['c_max']) / 4.0e6
        thr = int(cp['lengths'].max()) - int(em_us * 1000.0 / (1.75 * (145.0 + 2.0 * cp['c_max']))) - 400
        n1 = int((cp['lengths'] >= thr).sum())
        assert n1 == cp['n_long'] and n1 <= cp['b'] // 3 and cp['b'] - n1 >= 16 and cp['b'] >= 24, (case, thr, n1)
        assert np.abs(cp['lengths'] - thr).min() >= 50


def run_calls(case, monkeypatch, feedback, n_calls=4):
    from action_segmentation_amd import ops
    cp = corpus(case)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('SMM_SPLIT_MIN_US', '0')
    monkeypatch.setenv('SMM_PLAN_FEEDBACK', feedback)
    ops.reload_env()
    ops.release_cached_plans()
    assert ops.cached_plan_bytes() == 0
    dev = torch.device('cuda:0')
    t64 = lambda a: torch.tensor(a, dtype=torch.float64, device=dev).contiguous()
    batch = ops.Batch(cp['lengths'], cp['states'], cp['k'], c_max=cp['c_max'], frame_offset=cp['frame_off'], group=cp['group'],
                      kp=cp['kp'], d=cp['d'], t_max=int(cp['lengths'].max()), total_frames=cp['total'])
    args = (torch.tensor(cp['x'], device=dev), t64(cp['w']), t64(cp['cst']), t64(cp['inv_var']), t64(cp['trans']), t64(cp['init']),
            t64(cp['lens']))
    calls = []
    for _ in range(n_calls):
        ops.dp_timing_read()
        ops.dp_timing(True)
        try:
            out = ops.decode(batch, *args)
            torch.cuda.synchronize()
        finally:
            ops.dp_timing(False)
        tags = sorted(t for _, t in ops.dp_timing_read(tagged=True))
        info = ops.plan_feedback_info()
        ops.check_decoded(batch, out)
        calls.append(({k: out[k].cpu().numpy() for k in ('spans', 'labels', 'best', 'n_segs', '_err')}, tags, info))
    # the GPU's own fp64 emission, for the twin
    e64 = torch.zeros((cp['total'], cp['c_max']), dtype=torch.float64, device=dev)
    ops.emission(batch, *args[:4], out64=e64)
    torch.cuda.synchronize()
    return calls, e64.cpu().numpy()


@pytest.mark.parametrize('case', list(CASES))
def test_replanned_decode_keeps_every_bit(case, monkeypatch):
    from action_segmentation_amd import ops
    cp = corpus(case)
    b, lengths, off = cp['b'], cp['lengths'], cp['frame_off']
    plain, e64 = run_calls(case, monkeypatch, '0', n_calls=2)
    for out, tags, info in plain:
        assert tags == [1, 2], tags
        assert info['n_replans'] == 0 and info['stamps'] is None
    base = plain[0][0]
    assert base['_err'][0] == 0 and base['_err'][4] == 0, base['_err']
    # the C twin on the GPU's emission: best and spans bit for bit, labels and segment counts as the spans say
    for i in range(b):
        p, t = cp['par'][cp['group'][i]], int(lengths[i])
        s, v = F.viterbi(e64[off[i]:off[i] + t, :p['c']][None], [t], p['trans'], p['init'], p['lens'][:cp['kp'][i]], None)
        assert base['best'][i] == v[0]
        np.testing.assert_array_equal(base['spans'][i, :t + 1], s[0], err_msg='video %d' % i)
        assert (base['spans'][i, t + 1:] == -1).all()
        np.testing.assert_array_equal(base['labels'][off[i]:off[i] + t], O.spans_to_labels(s[0][None, :-1])[0], err_msg='video %d' % i)
        assert base['n_segs'][i] == (s[0][:t] != -1).sum()
    calls, _ = run_calls(case, monkeypatch, '2')
    try:
        for n, (out, tags, info) in enumerate(calls):
            assert tags == [1, 2], (n, tags)
            assert out['_err'][0] == 0 and out['_err'][4] == 0, (n, out['_err'])
            for key in ('spans', 'labels', 'best', 'n_segs'):
                np.testing.assert_array_equal(out[key], base[key], err_msg='call %d: %s' % (n, key))
        info = calls[-1][2]
        assert info['n_replans'] >= 1, info
        assert [c[2]['n_replans'] for c in calls[:2]] == [0, 0]          # (nothing to go by before the admitting call is through)
        assert info['n_videos'] == b and info['n1_before'] == cp['n_long']
        stamps, order, n1 = info['stamps'], info['order'], info['n1_after']
        assert stamps is not None and stamps.shape == (b, 2)
        assert (stamps[:, 0] > 0).all() and (stamps[:, 1] >= stamps[:, 0]).all()
        assert sorted(order.tolist()) == list(range(b))
        assert 1 <= n1 <= b // 3 and b - n1 >= 16
        # the first part: the n1 videos with the largest measured times (the clock ticks every 10 ns: times may tie)
        dur = stamps[:, 1] - stamps[:, 0]
        assert dur[order[:n1]].min() >= dur[order[n1:]].max(), (dur[order[:n1]], dur[order[n1:]].max())
        assert (np.diff(dur[order[:n1]]) <= 0).all() and (np.diff(dur[order[n1:]]) <= 0).all()
        assert info['end_before_us'] > 0.0 and info['end_after_us'] > 0.0
        assert ops.cached_plan_bytes() > 0
    finally:
        ops.release_cached_plans()
    assert ops.cached_plan_bytes() == 0
    zero = ops.plan_feedback_info()
    assert zero['n_replans'] == 0 and zero['n_videos'] == 0 and zero['stamps'] is None
