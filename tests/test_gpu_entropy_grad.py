"""Gradients of the posterior entropy, cross-entropy and KL divergence (smm_entropy_bwd_f64 / smm_kl_bwd_f64, ops.entropy_bwd /
ops.kl_bwd, SemiMarkovModule.entropy / entropy_packed / cross_entropy / kl_divergence(differentiable=True)) on the GPU.

References are computed here: torch fp64 autograd through -sum p log p, -sum p log q and sum p log(p / q) over every
segmentation of small lattices (tests/entropy_grad_ref.py), central differences of the C twin's fp64 entropy at real sizes,
exact invariants of the occurrence counts, closed forms (the uniform lattice, bit-identical sides) and Monte Carlo.  Every seed
is fixed.  Every gradient entry is compared with a reference in two regimes: on the enumerable lattices (3 states, K <= 4, T <= 7:
each kernel's work split in its first lane, slab, block and slice only) and at the mid sizes (up to 32 states, 300 length rows
and 330 frames, packed groups: every split crossed, against the forward recursion of tests/entropy_grad_dp_ref.py, which
tests/test_entropy_grad_dp_ref_host.py pins on the CPU); the real sizes are covered by invariants, values and one directional
derivative per table."""
import numpy as np
import pytest
import torch

import entropy_grad_cases as C
import entropy_grad_ref as R
from entropy_grad_cases import SMALL, _small_case
from oracle import dense_ref as O
from oracle import factored as F
from test_gpu_entropy import _batch_tables, _corpus, _features, _module, _ref_params, _twin_entropy

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
TABLES = ('elp', 'trans', 'init', 'len')
WORST = {}


def _ws(batch):
    return torch.empty(batch.workspace_bytes(), dtype=torch.uint8, device=DEV)


def _side(batch, elp, trans, init, lens, endpen, both=True):
    from action_segmentation_amd import ops
    ws = _ws(batch)
    z = ops.logz(batch, elp, trans, init, lens, endpen=endpen, ws=ws, with_backward=both)
    return (elp, trans, init, lens, endpen, z, ws)


def _grads(batch, P, Q, mode, up=None):
    """p's gradients (and value_out) from the kernels; q's as mu_q - mu_p.  P / Q: _side tuples."""
    from action_segmentation_amd import ops
    if mode == 'entropy':
        g = ops.entropy_bwd(batch, *P[:4], P[5], grad_out=up, endpen=P[4], ws=P[6], with_backward=True, want_value=True)
        gq = None
    else:
        g = ops.kl_bwd(batch, P, Q, grad_out=up, cross_entropy=mode == 'cross_entropy', want_value=True)
        mq = ops.logz_bwd(batch, *Q[:4], Q[5], grad_logz=up, endpen=Q[4], ws=Q[6], with_backward=True)
        mp = ops.logz_bwd(batch, *P[:4], P[5], grad_logz=up, endpen=P[4], ws=P[6], with_backward=True)
        gq = {k: mq[k] - mp[k] for k in TABLES}
    torch.cuda.synchronize()
    return g, gq


def _close(got, ref, what, bar=1e-4):
    """|got - ref| <= bar max(1, max |ref|) per table; returns the worst ratio."""
    worst = 0.0
    for k in TABLES:
        a = got[k].detach().double().cpu().reshape(ref[k].shape)
        scale = max(1.0, float(ref[k].abs().max()))
        err = float((a - ref[k]).abs().max()) / scale
        worst = max(worst, err)
        assert err <= bar, (what, k, err, a, ref[k])
    return worst


# ----------------------------------------------------------------------------------------------- 1. enumerable lattices
@pytest.mark.parametrize('q_kind', ['draw', 'near'])
@pytest.mark.parametrize('k,add_eos,masked,additional,narration', SMALL)
def test_exact_on_enumerable_lattices(k, add_eos, masked, additional, narration, q_kind):
    """Every mode, both sides, against torch fp64 autograd over every segmentation: <= 1e-4 max(1, max |ref|) per table (an
    upstream gradient of a different weight per video); the two values the kernel reports are the enumerated value."""
    p, q = _small_case(k, add_eos, masked, additional, narration, q_kind)
    elp, lengths, trans, init, lens, ep = p
    no_eos = not add_eos
    batch, *tp = _batch_tables(elp, lengths, trans, init, lens, ep, no_eos=no_eos)
    _, *tq = _batch_tables(q[0], lengths, q[2], q[3], q[4], q[5], no_eos=no_eos)
    up = np.array([1.0, -0.5, 2.0])
    upd = torch.tensor(up, dtype=torch.float64, device=DEV)
    kp = min(k, max(lengths))
    for mode in ('entropy', 'cross_entropy', 'kl'):
        P, Q = _side(batch, *tp), _side(batch, *tq, both=False)
        g, gq = _grads(batch, P, Q, mode, upd)
        vals, rp, rq = R.batch_reference(elp, lengths, trans, init, lens, kp, no_eos, ep, q if mode != 'entropy' else p,
                                         mode, up)
        w = _close(g, rp, (mode, 'p'))
        if gq is not None:
            w = max(w, _close(gq, rq, (mode, 'q')))
        WORST[('small', mode, q_kind)] = max(WORST.get(('small', mode, q_kind), 0.0), w)
        print('small lattice %s, q %s: worst |error| / max(1, max |ref|) %.3g' % (mode, q_kind, w))
        v = g['value'].cpu().numpy()
        assert np.isfinite(v).all()
        np.testing.assert_allclose(v[:, 0], vals, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(v[:, 1], vals, rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------------------------ 1b. mid sizes, entry by entry
# The bar is the stated accuracy of the log-partition path whose histories (smm_logz_kernel, fp32 sums) the gradient is read
# from: 1e-4, _close's default.  Measured on one MI355X, worst |error| / max(1, max |ref|) over the four tables, p's side (the
# kernels) / q's side (mu_q - mu_p), for entropy, cross-entropy, KL:
#   k_trips            2.9e-6        3.4e-6 / 3.9e-6    1.9e-6 / 3.9e-6
#   k_blocks           5.5e-6        6.6e-6 / 1.1e-5    1.5e-5 / 1.1e-5
#   states_32          3.3e-6        2.0e-6 / 1.7e-6    1.0e-6 / 1.7e-6
#   states_23_no_eos   6.4e-7        2.4e-7 / 7.0e-7    4.6e-7 / 7.0e-7
#   packed_groups      1.2e-6        3.0e-6 / 4.3e-6    4.2e-6 / 4.3e-6
# (smm_logz_bwd_f64's marginals alone against the C twin's on the same lattices: 1.2e-6, 4.0e-6, 1.5e-6, 5.8e-7, 8.0e-7; the
# kernel's two values are within 1.8e-7 of the reference value, smm_entropy_f64 / smm_kl_f64 within 2.9e-6.)  No case needs a
# bar of its own.
MID_BAR = 1e-4


def _mid_launch(case, side):
    """(Batch, elp, trans, init, len, endpen) on the device and the rows of each video's frames in the kernels' elp layout: a
    padded single-group batch without per-video arguments, or (packed_groups) ops.Batch with frame_offset, group and kp."""
    from action_segmentation_amd import ops
    elp, trans, init, lens, ep = case[side]
    lengths, off = case['lengths'], case['frame_offset']
    if case['single']:
        b, tmax, c = len(lengths), max(lengths), case['c_max']
        pad = np.zeros((b, tmax, c))
        for i, t in enumerate(lengths):
            pad[i, :t] = elp[off[i]:off[i] + t]
        rows = [np.arange(i * tmax, i * tmax + t) for i, t in enumerate(lengths)]
        return _batch_tables(pad, lengths, trans[0], init[0], lens[0], ep, no_eos=case['no_eos']), rows
    batch = ops.Batch(lengths, case['n_states'], case['k'], c_max=case['c_max'], frame_offset=off, group=case['group'],
                      kp=case['kp'], total_frames=case['total_frames'], no_eos=case['no_eos'])
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(DEV).contiguous()
    return (batch, t(elp), t(trans), t(init), t(lens), None if ep is None else t(ep)), [np.arange(o, o + n) for o, n in
                                                                                         zip(off, lengths)]


def _entries(got, ref, case, rows, what, bar, failures):
    """Every entry of every table: |got - ref| <= bar max(1, max |ref|); a table beyond it adds a line to `failures` that names
    its worst entry's index (elp: video, frame, state; the tables: group, [row,] state).  Returns the worst ratio."""
    worst = 0.0
    for k in TABLES:
        a = got[k].detach().double().cpu()
        if k == 'elp':
            r = torch.cat([ref[k][o:o + n] for o, n in zip(case['frame_offset'], case['lengths'])])
            a = a.reshape(-1, r.shape[1])[np.concatenate(rows)]
        else:
            r = ref[k]
            a = a.reshape(r.shape)
        err = (a - r).abs()
        scale = max(1.0, float(r.abs().max()))
        at = np.unravel_index(int(err.argmax()), err.shape)
        where = tuple(int(v) for v in at)
        if k == 'elp':
            ends = np.cumsum(case['lengths'])
            vid = int(np.searchsorted(ends, where[0], side='right'))
            where = (vid, where[0] - int(ends[vid] - case['lengths'][vid]), where[1])
        ratio = float(err.max()) / scale
        worst = max(worst, ratio)
        if not ratio <= bar:
            failures.append('%s: g_%s%s is %.12g, reference %.12g: |error| / max(1, max |ref|) %.3g > %.3g' % (
                what, k, list(where), float(a[at]), float(r[at]), ratio, bar))
    return worst


def _padding_is_zero(g, case, rows, what):
    """Exactly 0.0: frames no video covers, the states a group does not have (columns of elp, init and len, rows and columns of
    trans), len's row 0 and its rows from the group's largest span limit on, the frames of a video of upstream weight 0."""
    cm = case['c_max']
    ge = g['elp'].detach().cpu().reshape(-1, cm)
    covered = np.zeros(ge.shape[0], bool)
    covered[np.concatenate(rows)] = True
    assert (ge[~covered] == 0.0).all(), (what, 'elp rows of no video')
    for i, r in enumerate(rows):
        c = case['n_states'][case['group'][i]]
        assert (ge[r][:, c:] == 0.0).all(), (what, 'elp', i, 'padded states')
        if case['up'][i] == 0.0:
            assert (ge[r] == 0.0).all(), (what, 'elp', i, 'upstream weight 0')
    for gi, c in enumerate(case['n_states']):
        tr, ini, ln = (g[k].detach().cpu()[gi] for k in ('trans', 'init', 'len'))
        assert (tr[c:] == 0.0).all() and (tr[:, c:] == 0.0).all(), (what, 'trans', gi)
        assert (ini[c:] == 0.0).all(), (what, 'init', gi)
        kmax = max(kp for kp, gv in zip(case['kp'], case['group']) if gv == gi)
        assert (ln[:, c:] == 0.0).all() and (ln[0] == 0.0).all() and (ln[kmax:] == 0.0).all(), (what, 'len', gi)


@pytest.mark.parametrize('name', list(C.MID))
def test_entry_by_entry_at_mid_sizes(name):
    """Every mode, both sides, every entry against the fp64 forward recursion of tests/entropy_grad_dp_ref.py at sizes that
    cross each kernel's work split (entropy_grad_cases.MID says which): <= MID_BAR = 1e-4 max(1, max |ref|) per table; the kernel's
    two values within 1e-6, smm_entropy_f64 / smm_kl_f64 within 1e-4 of the reference value; padding exactly 0."""
    from action_segmentation_amd import ops
    case, ref = C.mid_case(name), C.mid_reference(name)
    (batch, *tp), rows = _mid_launch(case, 'p')
    (_, *tq), _ = _mid_launch(case, 'q')
    upd = torch.tensor(case['up'], dtype=torch.float64, device=DEV)
    failures = []
    for mode in ('entropy', 'cross_entropy', 'kl'):
        vals, rp, rq = ref[mode]
        P, Q = _side(batch, *tp), _side(batch, *tq, both=False)
        if mode == 'entropy':
            direct = ops.entropy(batch, *tp[:4], P[5], endpen=tp[4], ws=P[6], with_backward=True)
        else:
            kl, xe = ops.kl(batch, P, Q, with_backward=True, want_cross_entropy=True)
            direct = xe if mode == 'cross_entropy' else kl
        g, gq = _grads(batch, P, Q, mode, upd)
        assert ops.error_flag(batch, ws=P[6]) == 0
        v, direct = g['value'].cpu().numpy(), direct.cpu().numpy()
        scale = np.maximum(1.0, np.abs(vals))
        rv = max(float((np.abs(v[:, j] - vals) / scale).max()) for j in (0, 1))
        rd = float((np.abs(direct - vals) / scale).max())
        print('mid %s %s: value %s; value_out off by %.3g, the value kernel by %.3g' % (name, mode, vals, rv, rd))
        w = _entries(g, rp, case, rows, (name, mode, 'p'), MID_BAR, failures)
        wq = 0.0 if gq is None else _entries(gq, rq, case, rows, (name, mode, 'q'), MID_BAR, failures)
        WORST[('mid', name, mode)] = (w, wq)
        print('mid %s %s: worst |error| / max(1, max |ref|) %.3g (p), %.3g (q)' % (name, mode, w, wq))
        if not (np.isfinite(v).all() and rv <= 1e-6):
            failures.append('%s %s: value_out %s, reference %s: off by %.3g > 1e-6' % (name, mode, v.tolist(), vals, rv))
        if not rd <= 1e-4:
            failures.append('%s %s: the value kernel gives %s, reference %s: off by %.3g > 1e-4' % (name, mode, direct, vals, rd))
        _padding_is_zero(g, case, rows, (name, mode))
    assert not failures, '\n'.join(failures)


# ------------------------------------------------------------------------------------------------------- 2. closed forms
@pytest.mark.parametrize('add_eos', [True, False])
def test_kl_of_identical_sides_is_exactly_zero(add_eos):
    """KL(p || p) with bit-identical inputs on two workspaces: every gradient entry is exactly 0.0 on p's side (any batch) and
    on q's (one video: logz_bwd's sums are then deterministic), and so are both values."""
    p, _ = _small_case(4, add_eos, True, False, True, 'draw')
    elp, lengths, trans, init, lens, ep = p
    batch, *tp = _batch_tables(elp, lengths, trans, init, lens, ep, no_eos=not add_eos)
    P, Q = _side(batch, *tp), _side(batch, *tp, both=False)
    g, _ = _grads(batch, P, Q, 'kl')
    for k in TABLES:
        assert (g[k] == 0.0).all(), (k, g[k])
    assert (g['value'] == 0.0).all()
    one, *t1 = _batch_tables(elp[:1, :lengths[0]], lengths[:1], trans, init, lens, None if ep is None else ep[:1],
                             no_eos=not add_eos)
    g, gq = _grads(one, _side(one, *t1), _side(one, *t1, both=False), 'kl')
    for k in TABLES:
        assert (g[k] == 0.0).all() and (gq[k] == 0.0).all(), k


@pytest.mark.parametrize('add_eos', [True, False])
def test_cross_entropy_with_itself_is_the_entropy_gradient(add_eos):
    """H(p, q) with q = p (bit-identical, its own workspace) gives smm_entropy_bwd_f64's gradient and values."""
    p, _ = _small_case(4, add_eos, True, True, False, 'draw')
    batch, *tp = _batch_tables(*p, no_eos=not add_eos)
    ge, _ = _grads(batch, _side(batch, *tp), None, 'entropy')
    gx, _ = _grads(batch, _side(batch, *tp), _side(batch, *tp, both=False), 'cross_entropy')
    for k in TABLES + ('value',):
        torch.testing.assert_close(gx[k], ge[k], rtol=1e-12, atol=1e-12)


def _uniform(no_eos, lengths, c=23, k=1024):
    b, tmax = len(lengths), max(lengths)
    z = np.zeros
    return _batch_tables(z((b, tmax, c)), lengths, z((c, c)), z(c), z((k, c)), None if no_eos else z((b, c)), no_eos=no_eos)


@pytest.mark.parametrize('no_eos', [False, True])
def test_uniform_lattice_gradient_is_zero(no_eos):
    """All tables 0: the posterior is uniform, s(y) = 0 for every y, so d H = -Cov(s, phi) = 0: every entry is 0 to rounding
    (<= 1e-6 max(1, H)) up to T = 14 000, K = 1024, 23 states; the values are log N."""
    from action_segmentation_amd import ops
    batch, *t = _uniform(no_eos, [14000, 3001, 700, 2])
    P = _side(batch, *t)
    g, _ = _grads(batch, P, None, 'entropy')
    h = ops.entropy(batch, *t[:4], P[5], endpen=t[4], ws=P[6], with_backward=True)
    scale = max(1.0, float(h.max()))
    worst = max(float(g[k].abs().max()) for k in TABLES) / scale
    WORST['uniform' + ('_no_eos' if no_eos else '')] = worst
    print('uniform lattice (no_eos=%s): H max %.6g, worst |grad| / H %.3g' % (no_eos, float(h.max()), worst))
    assert worst <= 1e-6
    torch.testing.assert_close(g['value'][:, 0], h, rtol=1e-6, atol=1e-9)
    torch.testing.assert_close(g['value'][:, 1], h, rtol=1e-6, atol=1e-9)


# ----------------------------------------------------------------------------------------- 3. real sizes: invariants, FD
def _real(shape, no_eos=False):
    if shape == 'cfg2':
        c, k, d, lengths, constrained, scale = 16, 256, 24, [2048, 2048, 2048], False, 0.4
    elif shape == 'cfg1':
        c, k, d, lengths, constrained, scale = 20, 1024, 24, [10000], False, 0.4
    else:
        c, k, d, lengths, constrained, scale = 7, 64, 16, [900, 640, 1200, 333], True, 0.5
    m, g = _module(c, d, k, seed=43, constrained=constrained, scale=scale)
    b = len(lengths)
    x = _features(m, g, b, lengths, d)
    p = _ref_params(m)
    valid = torch.arange(c)
    trans, init, lens, merged = O.factor_tables(p, valid)
    cons = torch.randn(b, max(lengths), c, generator=g).double() * 0.3
    for i, t in enumerate(lengths):           # narration-style -1e9 masks: two windows of 40 frames per video
        for _ in range(2):
            t0 = int(torch.randint(0, t - 40, (1,), generator=g))
            cons[i, t0:t0 + 40, int(torch.randint(0, c, (1,), generator=g))] = -1e9
    elp = O.emission_log_probs(x.float().double(), p.gaussian_means[merged], p.gaussian_cov_diag, cons).numpy()
    ep = None
    if not no_eos:
        ep = F.endpen_from_allowed_ends(O.allowed_ends_for_batch(p, valid, None, b), b, c)
    return elp, lengths, trans.numpy(), init.numpy(), lens.numpy(), ep


# the q side (mu_q - mu_p: smm_logz_bwd_f64's marginals alone) measures up to 2.5e-4 on these lattices; p's side is of the same
# order (2.9e-4 worst, cfg1): the invariants hold to the accuracy of the histories both are read from
INVARIANT_BAR = 1e-3


def _invariants(batch, g, lengths, tmax, c, what, bar=INVARIANT_BAR, len_bar=INVARIANT_BAR):
    """Per frame sum_c g_elp = 0 (one class per frame), sum_c g_init = 0, sum_{k,c} k g_len = 0 (the spans cover T frames):
    each residual <= bar max(1, sum of |its terms|).  Returns the three worst ratios."""
    ge = g['elp'].view(len(lengths), tmax, c)
    r_elp = 0.0
    for i, t in enumerate(lengths):
        row = ge[i, :t]
        r_elp = max(r_elp, float((row.sum(1).abs() / row.abs().sum(1).clamp(min=1.0)).max()))
    gi = g['init'][0]
    r_init = abs(float(gi.sum())) / max(1.0, float(gi.abs().sum()))
    kk = torch.arange(g['len'].shape[1], dtype=torch.float64, device=DEV).view(-1, 1)
    s = kk * g['len'][0]
    r_len = abs(float(s.sum())) / max(1.0, float(s.abs().sum()))
    print('%s invariants: elp %.3g init %.3g len %.3g' % (what, r_elp, r_init, r_len))
    assert max(r_elp, r_init) <= bar and r_len <= len_bar, (what, r_elp, r_init, r_len)
    return r_elp, r_init, r_len


@pytest.mark.parametrize('shape', ['cfg4', 'cfg2', 'cfg1'])
def test_real_size_invariants(shape):
    """Invariants of every mode at real sizes with -1e9 masks; the two values against smm_entropy_f64 / smm_kl_f64."""
    from action_segmentation_amd import ops
    elp, lengths, trans, init, lens, ep = _real(shape)
    b, tmax, c = elp.shape
    batch, *tp = _batch_tables(elp, lengths, trans, init, lens, ep)
    rng = np.random.default_rng(7)
    elq = elp + 0.05 * rng.normal(size=elp.shape) * (elp > -1e8)
    _, *tq = _batch_tables(elq, lengths, trans, init, lens, ep)
    for mode in ('entropy', 'cross_entropy', 'kl'):
        P, Q = _side(batch, *tp), _side(batch, *tq, both=False)
        if mode == 'entropy':
            ref = ops.entropy(batch, *tp[:4], P[5], endpen=tp[4], ws=P[6], with_backward=True)
        else:
            kl, xe = ops.kl(batch, P, Q, with_backward=True, want_cross_entropy=True)
            ref = xe if mode == 'cross_entropy' else kl
        g, gq = _grads(batch, P, Q, mode)
        # (KL of a q near p: the gradient is small, and its length sums carry the histories' error of log p(o) - log q(o) --
        # as q's side, mu_q - mu_p, does: 1.3e-2 of sum |k g_len| on cfg1)
        WORST[(shape, mode, 'invariants')] = _invariants(batch, g, lengths, tmax, c, (shape, mode, 'p'),
                                                         len_bar=5e-2 if mode == 'kl' else INVARIANT_BAR)
        if gq is not None:
            # (q's length sums are smm_glen_kernel's, on v_exp_f32: 1.4e-2 of sum |k g_len| measured on cfg1)
            _invariants(batch, gq, lengths, tmax, c, (shape, mode, 'q'), len_bar=5e-2)
        v, ref = g['value'].cpu().numpy(), ref.cpu().numpy()
        # the two decompositions agree far below the path's bar; the value kernels' K loops run on v_exp_f32 (smm_entropy.hip)
        d01 = np.abs(v[:, 0] - v[:, 1]) / np.maximum(1.0, v[:, 0])
        print('%s %s: the two decompositions differ by %.3g' % (shape, mode, d01.max()))
        assert (d01 <= 1e-5).all(), v
        rel = np.abs(v[:, 0] - ref) / np.maximum(1.0, ref)
        WORST[(shape, mode, 'value')] = float(rel.max())
        print('%s %s: value %s, worst relative difference to the value kernel %.3g' % (shape, mode, v[:, 0], rel.max()))
        assert (rel <= 2e-4).all(), (mode, v, ref)
        if mode == 'entropy':
            twin = _twin_h(elp, lengths, trans, init, lens, ep)
            rt = np.abs(v[:, 0] - twin) / np.maximum(1.0, twin)
            print('%s entropy: worst relative difference to the twin %.3g (value kernel: %.3g)'
                  % (shape, rt.max(), (np.abs(ref - twin) / np.maximum(1.0, twin)).max()))
            assert (rt <= 1e-4).all(), (v, twin)


def _twin_h(elp, lengths, trans, init, lens, ep):
    return _twin_entropy(elp, lengths, trans, init, lens, ep)


@pytest.mark.parametrize('shape', ['cfg4', 'cfg2'])
def test_directional_derivatives_against_central_differences(shape):
    """sum_i dH_i along random directions of elp, trans, init and len against central differences of the C twin's fp64 H (log
    Z - E[s]); the step sizes 1e-3 and 5e-4 bound the differences' own error."""
    elp, lengths, trans, init, lens, ep = _real(shape)
    b, tmax, c = elp.shape
    batch, *tp = _batch_tables(elp, lengths, trans, init, lens, ep)
    g, _ = _grads(batch, _side(batch, *tp), None, 'entropy')
    gh = {k: g[k].cpu().numpy() for k in TABLES}
    rng = np.random.default_rng(11)
    kp = min(lens.shape[0], tmax)
    for which in ('elp', 'trans', 'init', 'len'):
        base = dict(elp=elp, trans=trans, init=init, len=lens)
        d = rng.normal(size=base[which].shape) * (np.asarray(base[which]) > -1e8)      # (masks stay masks)
        if which == 'elp':
            for i, t in enumerate(lengths):
                d[i, t:] = 0.0
        elif which == 'len':
            d[0] = 0.0
            d[kp:] = 0.0
        dirv = float((gh[which].reshape(d.shape) * d).sum() if which != 'elp'
                     else (gh['elp'].reshape(b, tmax, c) * d).sum())
        fd = []
        for eps in (1e-3, 5e-4):
            hs = []
            for sgn in (1.0, -1.0):
                t = {k: np.array(v, copy=True) for k, v in base.items()}
                t[which] = t[which] + sgn * eps * d
                hs.append(_twin_h(t['elp'], lengths, t['trans'], t['init'], t['len'], ep).sum())
            fd.append((hs[0] - hs[1]) / (2 * eps))
        noise = abs(fd[0] - fd[1]) + 1e-7 * max(1.0, abs(dirv))
        err = abs(dirv - fd[1])
        WORST[(shape, 'fd', which)] = err / max(1.0, abs(fd[1]))
        print('%s d%s: kernel %.9g, differences %.9g / %.9g' % (shape, which, dirv, fd[0], fd[1]))
        assert err <= 4 * noise + 1e-4 * max(1.0, abs(fd[1])), (which, dirv, fd)


# -------------------------------------------------------------------------------------------------------- 4. errors
def test_errors():
    """A NaN in elp: the error word is set and the video's rows are NaN; a q that rules out what p allows: KL = +inf, NaN rows,
    no error word; a short scratch: SMM_ERR_WORKSPACE."""
    import ctypes
    from action_segmentation_amd import _lib, ops
    p, _ = _small_case(4, True, False, False, False, 'draw')
    elp, lengths, trans, init, lens, ep = p
    bad = np.array(elp, copy=True)
    bad[1, 2, 0] = np.nan
    batch, *tp = _batch_tables(bad, lengths, trans, init, lens, ep)
    P = _side(batch, *tp)
    g, _ = _grads(batch, P, None, 'entropy')
    assert ops.error_flag(batch, ws=P[6]) != 0
    tmax = max(lengths)
    rows = g['elp'].view(len(lengths), tmax, -1).cpu()
    assert torch.isnan(rows[1, :lengths[1]]).all()
    assert torch.isfinite(rows[0, :lengths[0]]).all() and torch.isfinite(rows[2, :lengths[2]]).all()
    # q: transition 1 -> 0 impossible (-inf) where p allows it
    tq = np.array(trans, copy=True)
    tq[0, 1] = -np.inf
    batch, *tp = _batch_tables(elp, lengths, trans, init, lens, ep)
    _, *tqq = _batch_tables(elp, lengths, tq, init, lens, ep)
    P, Q = _side(batch, *tp), _side(batch, *tqq, both=False)
    g, _ = _grads(batch, P, Q, 'kl')
    assert ops.error_flag(batch, ws=P[6]) == 0
    assert torch.isinf(g['value']).all()
    assert torch.isnan(g['trans']).all() and torch.isnan(g['elp'].view(len(lengths), tmax, -1)[0, :lengths[0]]).all()
    # a short scratch
    lib = _lib.load()
    scratch = torch.empty(ops.entropy_bwd_scratch_bytes(batch) - 8, dtype=torch.uint8, device=DEV)
    f = lambda t: ctypes.c_void_p(t.data_ptr())
    ln, fo, gr, kp, ns = batch.host_ptrs()
    out = [torch.empty_like(x) for x in tp[:4]]
    rc = lib.smm_entropy_bwd_f64(ctypes.byref(batch.shape), *(ctypes.c_void_p(v) for v in (ln, fo, gr, kp, ns)),
                                 *(f(x) for x in tp[:4]), None, f(P[5]), None, *(f(x) for x in out), None,
                                 f(scratch), ctypes.c_size_t(scratch.numel()), f(P[6]), ctypes.c_size_t(P[6].numel()), None)
    assert rc == -3


# ------------------------------------------------------------------------------------------------- 5. consistency, module
def test_two_calls_are_bit_identical():
    p, q = _small_case(4, True, True, True, True, 'draw')
    elp, lengths, trans, init, lens, ep = p
    batch, *tp = _batch_tables(elp, lengths, trans, init, lens, ep)
    _, *tq = _batch_tables(q[0], lengths, q[2], q[3], q[4], q[5])
    for mode in ('entropy', 'cross_entropy', 'kl'):
        P, Q = _side(batch, *tp), _side(batch, *tq, both=False)
        a, _ = _grads(batch, P, Q, mode)
        b, _ = _grads(batch, P, Q, mode)
        for k in TABLES + ('value',):
            assert torch.equal(a[k], b[k]), (mode, k)


def _module_case(k=4, add_eos=True, constrained=False):
    m, g = _module(3, 5, k, seed=900 + k, constrained=constrained, scale=0.6)
    lengths = [7, 5, 6]
    x = _features(m, g, len(lengths), lengths, 5, noise=0.9)
    return m, g, x, lengths


def _param_grads(m, v):
    prm = (m.init_logits, m.transition_logits, m.poisson_log_rates, m.gaussian_means)
    gs = torch.autograd.grad(v, prm, allow_unused=True)
    return [torch.zeros_like(p) if gg is None else gg for p, gg in zip(prm, gs)]


def _ref_module_value(m, m2, x, lengths, add_eos, mode, up):
    """The module's value by enumeration on differentiable fp64 tables (factor_tables, the emission in torch)."""
    valid = torch.arange(m.n_classes)
    tot = 0.0
    for i, fr in enumerate(lengths):
        sides = []
        for mod in (m, m2):
            t = mod.factor_tables(valid, DEV)
            xe = x[i, :fr].to(DEV).double()
            elp = t['cst'] + xe @ t['w'] - 0.5 * (xe * xe) @ t['inv_var'].unsqueeze(1)
            sides.append(dict(elp=elp.cpu(), trans=t['trans'].cpu(), init=t['init'].cpu(), len=t['len'].cpu()))
        tp, tq = sides
        frames, c = tp['elp'].shape
        kp = min(tp['len'].shape[0], max(lengths))
        phi, last = R.occurrences(frames, c, tp['len'].shape[0], kp, not add_eos)
        sp, sq = phi @ R._flat(tp), phi @ R._flat(tq)
        if add_eos:
            ep = m._endpen(valid, None, len(lengths), c, DEV)
            ep = None if ep is None else ep[i].cpu()
            ep2 = m2._endpen(valid, None, len(lengths), c, DEV)
            ep2 = None if ep2 is None else ep2[i].cpu()
            sp = sp + R._wend(tp['trans'], ep)[last]
            sq = sq + R._wend(tq['trans'], ep2)[last]
        lp, lq = torch.log_softmax(sp, 0), torch.log_softmax(sq, 0)
        pp = lp.exp()
        v = dict(entropy=-(pp * lp).sum(), cross_entropy=-(pp * lq).sum(), kl=(pp * (lp - lq)).sum())[mode]
        tot = tot + up[i] * v
    return tot


@pytest.mark.parametrize('mode', ['entropy', 'cross_entropy', 'kl'])
@pytest.mark.parametrize('add_eos,constrained', [(True, False), (False, False), (True, True)])
def test_module_gradients_against_enumeration(mode, add_eos, constrained):
    """Parameter gradients of entropy / cross_entropy / kl_divergence(differentiable=True) against autograd through the
    enumerated value on factor_tables' differentiable fp64 tables: <= 1e-4 max(1, max |ref|) per parameter, both modules.
    The value is bit-identical to differentiable=False, which has no grad_fn."""
    m, g, x, lengths = _module_case(4, add_eos, constrained)
    m2 = _module(3, 5, 4, seed=901, constrained=constrained, scale=0.6)[0]
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(3)] * len(lengths))
    up = torch.tensor([1.0, -0.5, 2.0], dtype=torch.float64, device=DEV)
    if mode == 'entropy':
        f = lambda d: m.entropy(*args, add_eos=add_eos, differentiable=d)
        other = m
    else:
        meth = m.cross_entropy if mode == 'cross_entropy' else m.kl_divergence
        f = lambda d: meth(m2, *args, add_eos=add_eos, differentiable=d)
        other = m2
    v0 = f(False)
    assert v0.grad_fn is None
    v1 = f(True)
    assert v1.grad_fn is not None and torch.equal(v0, v1.detach())
    got = _param_grads(m, (v1 * up).sum())
    got2 = _param_grads(other, (f(True) * up).sum()) if other is not m else None
    ref = _ref_module_value(m, other, x, lengths, add_eos, mode, up.cpu())
    want = _param_grads(m, ref)
    for a, r in zip(got, want):
        scale = max(1.0, float(r.abs().max()))
        assert float((a.double() - r.double()).abs().max()) <= 1e-4 * scale, (a, r)
    if got2 is not None:
        want2 = _param_grads(other, _ref_module_value(m, other, x, lengths, add_eos, mode, up.cpu()))
        for a, r in zip(got2, want2):
            scale = max(1.0, float(r.abs().max()))
            assert float((a.double() - r.double()).abs().max()) <= 1e-4 * scale, (a, r)


def test_kl_with_itself_reaches_the_module_twice():
    """kl_divergence(self, differentiable=True): 0.0 and a gradient of 0 to rounding (p's side exactly 0, q's mu_q - mu_p)."""
    m, g, x, lengths = _module_case()
    args = (x.float().to(DEV), torch.tensor(lengths).to(DEV), [torch.arange(3)] * len(lengths))
    v = m.kl_divergence(m, *args, differentiable=True)
    assert (v.detach() == 0.0).all()
    for gg in _param_grads(m, v.sum()):
        assert float(gg.abs().max()) <= 1e-9


def test_packed_gradient_is_the_sum_of_batch_gradients():
    """entropy_packed(differentiable=True) on a two-task corpus: its value is entropy_packed's, bit for bit, and its parameter
    gradient is the sum of the per-batch entropy(differentiable=True) gradients."""
    m, batches, pc = _corpus()
    h0 = m.entropy_packed(pc)
    h1 = m.entropy_packed(pc, differentiable=True)
    assert h0.grad_fn is None and torch.equal(h0, h1.detach())
    got = _param_grads(m, h1.sum())
    want = None
    for bt in batches:
        hb = m.entropy(bt['features'].float().to(DEV), bt['lengths'].to(DEV), bt['task_indices'], differentiable=True)
        gb = _param_grads(m, hb.sum())
        want = gb if want is None else [a + b for a, b in zip(want, gb)]
    for a, r in zip(got, want):
        scale = max(1.0, float(r.abs().max()))
        assert float((a - r).abs().max()) <= 1e-5 * scale, (a, r)


def test_monte_carlo_covariance():
    """-Cov_p(s, phi) of init and trans from 4096 posterior samples against entropy_bwd: within 5 standard errors + 1e-6."""
    from action_segmentation_amd import ops
    p, _ = _small_case(4, True, False, False, False, 'draw')
    elp, lengths, trans, init, lens, ep = p
    batch, *tp = _batch_tables(elp[:1, :lengths[0]], lengths[:1], trans, init, lens, None)
    P = _side(batch, *tp)
    g, _ = _grads(batch, P, None, 'entropy')
    n = 4096
    out = ops.sample(batch, *tp[:4], P[5], n, seed=3, endpen=None, ws=P[6], want_spans=True, with_backward=True)
    spans = out['spans'].cpu().numpy()[:, 0]
    s = out['logp'].cpu().numpy()[:, 0]                         # log p(y) = s(y) - log Z: the same covariance
    c = trans.shape[0]
    T = lengths[0]
    phi_i = np.zeros((n, c))
    phi_t = np.zeros((n, c, c))
    for j in range(n):
        labs = [int(v) for v in spans[j, :T] if v >= 0]
        phi_i[j, labs[0]] = 1
        for a, b2 in zip(labs[:-1], labs[1:]):
            phi_t[j, b2, a] += 1
    for phi, gk in ((phi_i, g['init'][0]), (phi_t.reshape(n, -1), g['trans'][0].reshape(-1))):
        sc = s - s.mean()
        cov = (sc[:, None] * (phi - phi.mean(0))).mean(0)
        se = (sc[:, None] * (phi - phi.mean(0))).std(0) / np.sqrt(n)
        got = gk.cpu().numpy()
        assert (np.abs(got + cov) <= 5 * se + 1e-6).all(), (got, -cov, se)
