"""Same bits from two builds of libsmmdp.so on the posterior calls of the unconstrained lattice whose kernels or entry points
csrc/smm_posterior_grad.h and the host preamble of csrc/smm_api.hip state once: the cases of tests/test_gpu_entropy_grad.py
and tests/test_gpu_expected_reward.py (the enumerable lattices, the mid sizes with the packed two-group corpus, identical sides, q near p)
and small ones on the skeletons' edges run through action-segmentation_amd/libsmmdp_prev.so and
action-segmentation_amd/libsmmdp.so, one fresh child process per library (SMM_LIB_PATH), each under its own time limit; the
second child starts only if the first exited 0.  Every output array is compared byte for byte: the four gradients, value (both
decompositions) and the error word of entropy_bwd, of kl_bwd in both modes and of expected_reward_bwd (frame reward only,
segment reward only, both); value and parts of expected_reward; entropy, kl with the cross-entropy, and segment_posteriors.
Workspaces and scratch are pre-filled with 0xFF bytes.  Prints the counts; exit status 1 on a difference.
usage: python scripts/ab_posterior_grad_bits.py              (the driver)
       python scripts/ab_posterior_grad_bits.py --child OUT.npz   (one library's run)"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'action-segmentation_amd')
LIMIT = 400                                                  # seconds per child


def driver():
    out = os.environ.get('SMM_OUT') or os.path.join(ROOT, 'bench_out')
    os.makedirs(out, exist_ok=True)
    files = []
    for lib in ('libsmmdp_prev.so', 'libsmmdp.so'):
        path = os.path.join(out, 'ab_posterior_grad_bits_%s.npz' % lib[:-3])
        rc = subprocess.call(['timeout', '-k', '10', str(LIMIT), sys.executable, os.path.abspath(__file__), '--child', path],
                             env=dict(os.environ, SMM_LIB_PATH=os.path.join(PKG, lib)))
        if rc != 0:
            print('%s: exit status %d' % (lib, rc))
            return 1
        files.append(path)
    a, b = (np.load(f) for f in files)
    assert sorted(a.files) == sorted(b.files), 'the two runs made different calls'
    calls = {k.rsplit('|', 1)[0] for k in a.files}
    differ = [k for k in a.files if a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    print('%d calls, %d output arrays, %d bytes compared: %d arrays differ' % (len(calls), len(a.files), sum(a[k].nbytes for k in a.files),
                                                                       len(differ)))
    for k in differ:
        print('  differs: %s (%d of %d bytes)' % (k, int((a[k].reshape(-1).view(np.uint8) != b[k].reshape(-1).view(np.uint8)).sum()),
                                                  a[k].nbytes))
    return 1 if differ else 0


def _tables(rng, c, k):
    lsm = lambda a: a - np.log(np.exp(a).sum(0, keepdims=True))
    lens = np.zeros((k, c))
    lens[1:] = lsm(rng.normal(size=(k - 1, c)))
    return lsm(rng.normal(size=(c, c))), lsm(rng.normal(size=c)), lens


def _edge(seed, lengths, c, k, eos=True):
    """A padded single-group lattice of random tables: (elp_bt, lengths, trans, init, lens, endpen) as numpy."""
    rng = np.random.default_rng(seed)
    b, tmax = len(lengths), max(lengths)
    elp = rng.normal(size=(b, tmax, c)) * 1.5
    for i, t in enumerate(lengths):
        elp[i, t:] = 0.0
    trans, init, lens = _tables(rng, c, k)
    return elp, lengths, trans, init, lens, (rng.normal(size=(b, c)) if eos else None)


def child(path):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import entropy_grad_cases as C
    from action_segmentation_amd import _lib, ops
    from test_gpu_entropy import _batch_tables
    from test_gpu_entropy_grad import _mid_launch
    assert os.path.samefile(_lib.LIB_PATH, os.environ['SMM_LIB_PATH'])
    dev = torch.device('cuda:0')
    out = {}
    outputs = ops._ebwd_outputs

    def filled_outputs(*a, **k):                             # the gradient calls' scratch: 0xFF like the workspaces
        g, scratch = outputs(*a, **k)
        return g, scratch.fill_(0xFF)
    ops._ebwd_outputs = filled_outputs

    def keep(call, err, **arrays):
        for k, v in dict(arrays, err=torch.tensor([err])).items():
            if v is not None:
                out['%s|%s' % (call, k)] = v.detach().cpu().numpy()

    def side(batch, t, both):
        ws = torch.full((batch.workspace_bytes(),), 0xFF, dtype=torch.uint8, device=dev)
        z = ops.logz(batch, *t[:4], endpen=t[4], ws=ws, with_backward=both)
        return (*t, z, ws)

    def run(name, launch_p, launch_q, up=None, reward=None, seg=None, both=False):
        """Every call on one pair of launches (batch, elp, trans, init, len, endpen); both: log Z runs the reversed recursion."""
        batch, tp, tq = launch_p[0], launch_p[1:], launch_q[1:]
        name = '%s, both %d' % (name, both)
        t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev).contiguous()
        up, reward, seg = t(up), t(reward), t(seg)
        err = lambda s: ops.error_flag(batch, ws=s[6])
        P = side(batch, tp, both)
        kw = dict(endpen=P[4], ws=P[6], with_backward=both)
        keep(name + ' logz', err(P), logz=P[5])
        h = ops.entropy(batch, *P[:4], P[5], **kw)
        keep(name + ' entropy', err(P), entropy=h)
        s = ops.segment_posteriors(batch, *P[:4], P[5], **kw)
        keep(name + ' segment_posteriors', err(P), start=s['start'], end=s['end'], boundary=s['boundary'])
        g = ops.entropy_bwd(batch, *P[:4], P[5], grad_out=up, want_value=True, **kw)
        keep(name + ' entropy_bwd', err(P), **g)
        for what, r, sg in (('both', reward, seg), ('frames', reward, None), ('segments', None, seg)):
            v, parts = ops.expected_reward(batch, *P[:4], P[5], reward=r, seg_reward=sg, want_parts=True, **kw)
            keep('%s expected_reward %s' % (name, what), err(P), value=v, parts=parts)
            g = ops.expected_reward_bwd(batch, *P[:4], P[5], reward=r, seg_reward=sg, grad_out=up, want_value=True, **kw)
            keep('%s expected_reward_bwd %s' % (name, what), err(P), **g)
        for xent in (False, True):                           # (kl_bwd writes q's workspace: a fresh pair per call)
            P, Q = side(batch, tp, both), side(batch, tq, both)
            d, x = ops.kl(batch, P, Q, with_backward=both, want_cross_entropy=True)
            keep('%s kl %d' % (name, xent), err(P), kl=d, xent=x)
            g = ops.kl_bwd(batch, P, Q, grad_out=up, with_backward=both, cross_entropy=xent, want_value=True)
            keep('%s kl_bwd xent %d' % (name, xent), err(P), **g)
        torch.cuda.synchronize()

    def rewards(seed, launch, n_groups=1):
        rng = np.random.default_rng(seed)
        return rng.normal(size=(launch[0].total_frames, launch[0].c_max)), rng.normal(size=(n_groups, launch[0].c_max))

    # ---- the test files' cases: the enumerable lattices (also with identical sides), the mid sizes, the packed corpus
    up3 = [1.0, -0.5, 2.0]
    for k, add_eos, masked, additional, narration in C.SMALL:
        p, q = C._small_case(k, add_eos, masked, additional, narration, 'draw')
        lp, lq = _batch_tables(*p, no_eos=not add_eos), _batch_tables(*q, no_eos=not add_eos)
        r, sg = rewards(1000 + k, lp)
        for both in (False, True):
            run('small %s' % ((k, add_eos, masked, additional, narration),), lp, lq, up3, r, sg, both)
        run('small %s, identical sides' % ((k, add_eos, masked, additional, narration),), lp, lp, up3, r, sg)
        near = C._small_case(k, add_eos, masked, additional, narration, 'near')[1]     # (q = p with elp moved by 1e-3 sigma)
        run('small %s, q near p' % ((k, add_eos, masked, additional, narration),), lp, _batch_tables(*near, no_eos=not add_eos),
            up3, r, sg)
    for name in C.MID:
        case = C.mid_case(name)
        lp, lq = _mid_launch(case, 'p')[0], _mid_launch(case, 'q')[0]
        r, sg = rewards(case['total_frames'] + 17, lp, len(case['n_states']))
        run('mid ' + name, lp, lq, case['up'], r, sg)
    # ---- the skeletons' edges
    def edge(seed, name, lengths, c, k, eos=True, up=None, both=False, mark=None):
        p, q = _edge(seed, lengths, c, k, eos), _edge(seed + 1, lengths, c, k, eos)
        lp, lq = _batch_tables(*p, no_eos=not eos), _batch_tables(*q, no_eos=not eos)
        r, sg = rewards(seed + 2, lp)
        if mark:
            lp, lq, r = mark(lp, lq, r)
        run('%s, eos %d' % (name, eos), lp, lq, up if up is not None else [1.0, 0.0, -0.5, 2.0][:len(lengths)], r, sg, both)

    for eos in (True, False):
        first = 1 - eos                                      # (without EOS the last frame carries the closing label only)
        edge(9000, 'T = 1', [1 + first, 2 + first], 3, 4, eos)
        edge(9010, 'the slab rule', [63 + first, 64 + first, 65 + first, 129 + first], 3, 9, eos)
        edge(9020, 'one state', [40, 7], 1, 6, eos)
        edge(9030, '23 states: one slice, idle threads past P', [70, 20], 23, 8, eos)
        edge(9040, '32 states: P = 1024', [40, 9], 32, 6, eos)
        edge(9050, 'kp = 2', [30, 5], 4, 2, eos)
        edge(9060, 'kp - 1 > T', [3 + first, 2 + first], 3, 12, eos)
        edge(9070, 'a second block of lengths', [275], 2, 262, eos, up=[1.5])

        def bad_reward(lp, lq, r):
            r = r.copy()
            r[lp[0].t_max + 3, 1] = np.inf                   # (video 1, frame 3; video 0 stays clean)
            return lp, lq, r
        edge(9080, 'a non-finite reward', [20, 18, 9], 3, 5, eos, mark=bad_reward)

        def no_path(lp, lq, r):
            elp = lp[1].clone()
            elp[2 * lp[0].t_max + 1] = -np.inf               # (video 2: no segmentation has a finite score)
            return (lp[0], elp) + tuple(lp[2:]), lq, r
        edge(9090, 'a video whose log Z is -inf', [20, 18, 9], 3, 5, eos, mark=no_path)

        def q_cuts(lp, lq, r):
            trans = lq[2].clone()
            trans[0, 1, 0] = -np.inf
            return lp, lq[:2] + (trans,) + tuple(lq[3:]), r
        edge(9100, 'q excludes a transition p uses', [20, 18, 9], 3, 5, eos, mark=q_cuts)

        def q_span(lp, lq, r):
            lens = lq[4].clone()
            lens[0, 2, 1] = -np.inf                          # (spans of two positions of state 1: p weighs them in every video)
            return lp, lq[:4] + (lens,) + tuple(lq[5:]), r
        edge(9110, 'q excludes a span p uses', [20, 18, 9], 3, 5, eos, mark=q_span)
    np.savez(path, **out)
    print('%s: %d calls, %d arrays' % (os.path.basename(os.environ['SMM_LIB_PATH']), len({k.rsplit('|', 1)[0] for k in out}), len(out)))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--child':
        child(sys.argv[2])
    else:
        sys.exit(driver())
