"""The training reference (tests/train_ref.py) on the host: its two DP routes agree, values and gradients, and its
comparator rejects what a subtly wrong training kernel would produce."""
import numpy as np
import pytest
import torch

from oracle import dense_ref as O
import train_ref as R
from golden_util import CASES, case_inputs

# every golden case with EOS, each also without it (the reference's add_eos=False; no end penalties then), and no_eos
ROUTE_CASES = ([(c, True) for c in CASES if CASES[c].get('add_eos', True)] +
               [(c, False) for c in CASES])


def _batch(golden, case, add_eos, with_gold=False):
    p, feats, lengths, valid, cons, cfg = case_inputs(golden, case, torch.float64)
    spans = None
    if with_gold:
        # a gold segmentation the model can score: the reference path's own Viterbi spans (global ids)
        r = O.viterbi_full(p, feats, lengths, valid, add_eos, cfg.get('additional') if add_eos else None, cons)
        spans = r['spans'][:, :feats.shape[1]]
    rb = R.RefBatch(feats.float(), lengths, valid, None if cons is None else cons.float(),
                    cfg.get('additional') if add_eos else None, add_eos, spans)
    return p, rb


def _upstream(b):
    return torch.linspace(0.5, 1.5, b, dtype=torch.float64)


def _close(got, ref, tol, what):
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * max(1e-300, float(np.abs(ref).max())), err_msg=what)


@pytest.mark.parametrize('case,add_eos', ROUTE_CASES)
def test_factored_route_equals_dense_route(golden, case, add_eos):
    """log Z per video and the gradients of sum_i u_i log Z_i (u_i != 1: the twin's per-video upstream weighting) agree
    between the dense potentials + restated DP and the C twin's forward-backward, to 1e-10."""
    p, rb = _batch(golden, case, add_eos)
    out = {}
    for route in ('dense', 'factored'):
        q, leaves = R.with_leaves(p)
        z = R.logz(q, rb, route)
        out[route] = (z.detach().numpy(), R.grads(leaves, (z * _upstream(z.numel())).sum()))
    _close(out['factored'][0], out['dense'][0], 1e-10, 'logZ')
    for n in R.PARAMS:
        ref = out['dense'][1][n]
        _close(out['factored'][1][n], ref, 1e-10, n)
    for n in ('gaussian_means', 'transition_logits'):
        assert np.abs(out['dense'][1][n]).max() > 0, n
    if case == 'subset_merge':
        # merged classes share a parameter row: exactly the rows the set's states map to get a mean gradient
        merged_rows = {CASES[case]['merge'][int(v)] for v in rb.valid_classes}
        g = out['dense'][1]['gaussian_means']
        for row in range(g.shape[0]):
            assert (np.abs(g[row]).max() > 0) == (row in merged_rows), (row, merged_rows)


@pytest.mark.parametrize('case,add_eos', ROUTE_CASES)
def test_gold_score_routes_agree(golden, case, add_eos):
    """Gold-span joint score: sum(scores * to_parts(spans)) on the dense potentials == the sums along the spans on the
    factored tables, values and gradients; and (no gold penalty on these spans) never above log Z."""
    p, rb = _batch(golden, case, add_eos, with_gold=True)
    out = {}
    for route in ('dense', 'factored'):
        q, leaves = R.with_leaves(p)
        s = R.gold(q, rb, route)
        out[route] = (s.detach().numpy(), R.grads(leaves, (s * _upstream(s.numel())).sum()))
    _close(out['factored'][0], out['dense'][0], 1e-12, 'gold score')
    for n in R.PARAMS:
        _close(out['factored'][1][n], out['dense'][1][n], 1e-12, n)
    q, _ = R.with_leaves(p)
    with torch.no_grad():
        z = R.logz(q, rb, 'factored').numpy()
    assert np.all(out['dense'][0] <= z + 1e-9)


def test_discriminative_loss_routes_agree(golden):
    """gold - log Z (--sm_train_discriminatively) through both routes, with a constrained, end-restricted case."""
    p, rb = _batch(golden, 'constrained', True, with_gold=True)
    out = {}
    for route in ('dense', 'factored'):
        q, leaves = R.with_leaves(p)
        out[route] = R.grads(leaves, (R.gold(q, rb, route) - R.logz(q, rb, route)).mean())
    for n in R.PARAMS:
        _close(out['factored'][n], out['dense'][n], 1e-10, n)


def test_no_eos_twin_rejects_one_frame_videos():
    from oracle import factored as F
    elp = np.zeros((1, 3, 2))
    with pytest.raises(AssertionError):
        F.logz(elp, np.array([1]), np.zeros((2, 2)), np.zeros(2), np.zeros((3, 2)), no_eos=True)


# ------------------------------------------------------------------------------------------------ the comparator's teeth
def _reference_grads(golden):
    p, rb = _batch(golden, 'subset_merge', True)
    q, leaves = R.with_leaves(p)
    return R.grads(leaves, R.logz(q, rb, 'factored').mean())


def _small_row(ref):
    """A row well below the tensor's largest (so a bar scaled by max|ref| would not see it), above the 1e-2 floor."""
    r2 = np.abs(ref.reshape(ref.shape[0], -1))
    rowmax, gmax = r2.max(1), r2.max()
    cand = [r for r in range(len(rowmax)) if 2e-2 * gmax < rowmax[r] < 0.5 * gmax]
    assert cand, rowmax / gmax
    return min(cand, key=lambda r: rowmax[r])


@pytest.mark.parametrize('name', ['gaussian_means', 'transition_logits'])
def test_comparator_has_teeth(golden, name):
    ref = _reference_grads(golden)[name]
    bar = 2e-5
    assert R.row_errors(ref.copy(), ref, bar)[1] == []
    # fp32 rounding of the exact result passes at the tightest bar the tests use
    assert R.row_errors(ref.astype(np.float32), ref, 1e-6)[1] == []
    r = _small_row(ref)
    # 1e-4 relative in one small row: 5x the bar, invisible to a bar scaled by the whole tensor's largest entry
    bad = ref.copy()
    bad[r] *= 1 + 1e-4
    assert R.row_errors(bad, ref, bar)[1], 'a 1e-4 relative error in row %d passed' % r
    np.testing.assert_allclose(bad, ref, rtol=5e-4, atol=5e-4 * np.abs(ref).max())     # (the old bar lets it through)
    # a flipped sign in that row
    bad = ref.copy()
    bad[r] = -bad[r]
    assert R.row_errors(bad, ref, bar)[1]
    # a missing row (its contribution dropped: zeros)
    bad = ref.copy()
    bad[r] = 0.0
    assert R.row_errors(bad, ref, bar)[1]
    # anything in a row whose reference is exactly zero
    ref0 = ref.copy()
    ref0[r] = 0.0
    bad = ref0.copy()
    bad[r].flat[0] = 1e-30
    worst, fails = R.row_errors(bad, ref0, bar)
    assert fails and worst == float('inf')
    assert R.row_errors(ref0, ref0, bar)[1] == []
    # and a NaN anywhere
    bad = ref.copy()
    bad.flat[-1] = np.nan
    assert R.row_errors(bad, ref, bar)[1]


def test_comparator_on_one_dimensional_tensors():
    ref = np.array([3.0, -0.5, 0.04, 0.0, 1e-6])
    assert R.row_errors(ref, ref, 2e-5)[1] == []
    # every entry is its own row; below 1e-2 of the largest, the floor 1e-2 * max applies
    got = ref + np.array([0, 0, 0, 0, 2e-5 * 1e-2 * 3.0 * 0.9])
    assert R.row_errors(got, ref, 2e-5)[1] == []
    got = ref.copy(); got[2] *= 1 + 1e-4
    assert R.row_errors(got, ref, 2e-5)[1]
    got = ref.copy(); got[3] = 1e-300
    assert R.row_errors(got, ref, 2e-5)[1]


@pytest.mark.parametrize('case', ['subset_merge', 'constrained', 'k_gt_t'])
def test_means_condition_bounds_the_mean_gradients(golden, case):
    """means_condition sums the absolute values of (more than) the terms each mean gradient adds up: it bounds
    |gradient| entry by entry, and is zero exactly on the rows no state of the set maps to."""
    p, rb = _batch(golden, case, True)
    q, leaves = R.with_leaves(p)
    g = R.grads(leaves, R.logz(q, rb, 'factored').mean())['gaussian_means']
    cond = R.means_condition(q, [rb], [np.full(len(rb.lengths), 1.0 / len(rb.lengths))])
    assert np.all(cond >= np.abs(g) * (1 - 1e-12))
    used = set(range(p.n_classes)) if rb.valid_classes is None else set(int(v) for v in rb.valid_classes)
    if case == 'subset_merge':
        used = {CASES[case]['merge'][v] for v in used}
    rows = np.abs(cond).max(1) > 0
    assert set(np.flatnonzero(rows).tolist()) == used


def test_comparator_size_and_cap():
    """``size``: the bar follows the magnitudes given (a cancelling difference held at the size of its parts); with a
    model the allowance never exceeds the old bar 5e-4 * (|ref| + max(1, max|ref|))."""
    ref = np.array([[1e-4, -2e-4], [3e-4, 1e-5]])
    size = np.array([[10.0, 20.0], [5.0, 1.0]])
    got = ref + 1e-5
    assert R.row_errors(got, ref, 2e-5)[1]                          # against the remainder's own size: fails
    assert R.row_errors(got, ref, 2e-5, size=size)[1] == []          # against its parts' size: 1e-5 <= 2e-5 * 20
    got = ref + 1e-3
    assert R.row_errors(got, ref, 2e-5, size=size * 100)[1]          # 1e-3 > the old bar 5e-4 * (|ref| + 1)


def test_reference_masks_equal_the_modules():
    """masks_from_sets (what the reference builds from the constructor's sets, reference semimarkov_modules.py:169-191)
    equals the module's own init / transition masks."""
    from action_segmentation_amd.semimarkov_modules import SemiMarkovModule
    from module_util import make_args
    g = np.random.default_rng(4)
    n = 12
    starts = {0, 3, 7}
    allowed = {i: {int(j) for j in g.choice(n, size=int(g.integers(0, 5)), replace=False)} for i in range(n) if i != 5}
    m = SemiMarkovModule(make_args(8), n, 3, allow_self_transitions=False, allowed_starts=starts,
                         allowed_transitions=allowed, allowed_ends={1, 2})
    ic, tc = R.masks_from_sets(n, starts, allowed)
    assert torch.equal(m.init_constraints.detach().cpu(), ic) and torch.equal(m.transition_constraints.detach().cpu(), tc)
    q, _ = R.params_from_module(m, allowed_starts=starts, allowed_transitions=allowed, allowed_ends={1, 2})
    assert q.allowed_ends == {1, 2} and not q.allow_self_transitions
    with pytest.raises(AssertionError):
        R.params_from_module(m)                                      # structure the caller did not name
