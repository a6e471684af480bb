"""Randomised soak of the posterior sampler (smm_sample_f64 through SemiMarkovModule.sample): random modules (2..32 states, span
limits 2..1024, ordering masks on and off, EOS and no EOS), ragged batches.  Every pass checks each sample's log-probability against
the rescoring of its spans (gold_score - log_partition, to 1e-6 of max(1, |log Z|)), and, in EOS mode, the per-frame class
frequencies of 64 samples against the C twin's posteriors (oracle.factored.logz(grad=True)): the entries outside
6 sqrt(p(1-p)/N) + 2e-3 may not exceed twice what binomial noise alone puts there, plus 10 (tests/test_gpu_sample.py).
usage: soak_sample.py [seconds] [seed] [summary file]     (a line every ~20 s; the summary goes to profiles/ by default)"""
import os
import sys
import time

sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import numpy as np
import torch

import test_gpu_sample as ts
from oracle import dense_ref as O
from oracle import factored as F

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
seed0 = int(sys.argv[2]) if len(sys.argv) > 2 else 0
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join('profiles', 'soak_sample.txt')
g = np.random.default_rng(seed0)
dev = ts.DEV
t0, last, n, samples, frames, worst_lp, worst_ratio = time.time(), time.time(), 0, 0, 0, 0.0, 0.0
while time.time() - t0 < budget:
    c = int(g.integers(2, 33))
    k = int(g.choice([2, 3, 5, 8, 20, 64, 65, 130, 256, 300, 520, 1024]))
    b = int(g.integers(1, 5))
    tmax = int(g.choice([30, 200, 700, 2048]))
    add_eos = bool(g.random() < 0.75)
    constrained = bool(g.random() < 0.3) and c >= 3
    d = 8
    m, tg = ts._module(c, d, k, seed=int(g.integers(0, 10 ** 6)), constrained=constrained, scale=float(g.choice([0.3, 0.7])))
    lengths = [int(x) for x in g.integers(max(2, tmax // 3), tmax + 1, size=b)]
    lengths[0] = tmax
    x = ts._features(m, tg, b, lengths, d)
    xd, ln, valid = x.float().to(dev), torch.tensor(lengths).to(dev), torch.arange(c)
    ns = 64
    spans, logp = m.sample(xd, ln, [valid] * b, n_samples=ns, seed=int(g.integers(0, 2 ** 63)), add_eos=add_eos)
    z = m.log_partition(xd, ln, valid, no_eos=not add_eos).detach()
    tol = 1e-6 * max(1.0, float(z.abs().max()))
    for s in range(ns):
        gs = m.gold_score(xd, ln, valid, spans[s, :, :tmax].to(dev), no_eos=not add_eos).detach()
        err = float((logp[s] - (gs - z)).abs().max())
        worst_lp = max(worst_lp, err / tol)
        assert err <= tol, (c, k, b, tmax, add_eos, constrained, s, err)
    if add_eos and not constrained:
        p = ts._ref_params(m)
        trans, init, lens, merged = O.factor_tables(p, valid)
        elp = O.emission_log_probs(x.float().double(), p.gaussian_means[merged], p.gaussian_cov_diag)
        _, gr = F.logz(elp.numpy(), np.array(lengths), trans.numpy(), init.numpy(), lens.numpy(), grad=True)
        for i, t in enumerate(lengths):
            lab = O.spans_to_labels(spans[:, i, :t].numpy())
            freq = np.stack([(lab == j).mean(0) for j in range(c)], axis=1)
            bad, expected = ts._exceedances(freq, gr['elp'][i, :t], ns)
            worst_ratio = max(worst_ratio, bad / (2 * expected + 10))
            assert bad <= 2 * expected + 10, (c, k, b, tmax, i, bad, expected)
    n += 1
    samples += ns * b
    frames += ns * sum(lengths)
    if time.time() - last > 20:
        last = time.time()
        print('%6.0f s: %d batches, %d samples, %.1f M sampled frames; worst log-p error / bar %.3f, worst exceedances / bar %.3f'
              % (last - t0, n, samples, frames / 1e6, worst_lp, worst_ratio), flush=True)
line = ('soak_sample seed %d, %.0f s: %d batches, %d samples (%.1f M frames), every log-p within its bar (worst %.3f of it), '
        'frequency exceedances within their bar (worst %.3f of it)' % (seed0, time.time() - t0, n, samples, frames / 1e6, worst_lp,
                                                                        worst_ratio))
print(line)
os.makedirs(os.path.dirname(out_path) or '.', exist_ok=True)
with open(out_path, 'w') as f:
    f.write(line + '\n')
