"""Same bits from two builds of libsmmdp.so on the transcript-graph posterior calls: the cases of
tests/test_gpu_transcript_{graph,sample,entropy,kl,entropy_grad,expected_reward}.py and a few of its own run through
action-segmentation_amd/libsmmdp_prev.so and action-segmentation_amd/libsmmdp.so, one fresh child process per library
(SMM_LIB_PATH), each under its own time limit; the second child starts only if the first exited 0.  Every output array is
compared byte for byte: log Z and the backward gradients with p_used / p_end; samples (spans, labels, logp, n_segs, used);
entropy and parts; KL, cross-entropy and parts; the four gradients, value and value_plus in the three gradient modes; value
and parts of the expected reward, and the four gradients, value and value_plus of its gradient call; the error word of every call that returns one (the backward call of log Z does not).  Workspaces and scratch are pre-filled with 0xFF bytes.  Prints the counts; exit status 1 on a difference.
usage: python scripts/ab_align_graph_bits.py              (the driver)
       python scripts/ab_align_graph_bits.py --child OUT.npz   (one library's run)"""
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
        path = os.path.join(out, 'ab_align_graph_bits_%s.npz' % lib[:-3])
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
        print('  differs: %s (%d of %d elements)' % (k, int((a[k].view(np.uint8) != b[k].view(np.uint8)).sum()), a[k].nbytes))
    return 1 if differ else 0


def child(path):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_gpu_transcript_entropy_grad as GG
    import test_gpu_transcript_expected_reward as GR
    import test_gpu_transcript_graph as GT
    import test_gpu_transcript_kl as GK
    import test_gpu_transcript_sample as GS
    from action_segmentation_amd import _lib, ops
    from test_gpu_transcript_graph import Case, _tables
    assert os.path.samefile(_lib.LIB_PATH, os.environ['SMM_LIB_PATH'])
    G = ops.TranscriptGraph
    out = {}

    def keep(call, **arrays):
        for k, v in arrays.items():
            if isinstance(v, (list, tuple)):
                v = torch.cat([x.reshape(-1) for x in v])
            if v is not None:
                out['%s|%s' % (call, k)] = v.detach().cpu().numpy()

    def run(name, pc, qc):
        """Every call of the family on one pair of launches (qc's graphs may differ from pc's: a q workspace for other graphs)."""
        batch, dp, fp = GS._forward(pc, 0xFF)
        _, dq, fq = GS._forward(qc, 0xFF)
        err = lambda o: torch.tensor([ops.error_flag(batch, o)])
        keep(name + ' logz p', logz=fp['logz'], err=err(fp))
        keep(name + ' logz q', logz=fq['logz'], err=err(fq))
        r = GK._backward(pc, batch, dp, fp)
        keep(name + ' logz_bwd', elp=r['elp'], trans=r['trans'], init=r['init'], len=r['len'], p_used=r['node_prob'], p_end=r['end_prob'])
        s = GS._draw(pc, batch, dp, fp, 5, seed=11)
        keep(name + ' sample', spans=s['spans'], labels=s['labels'], logp=s['logp'], n_segs=s['n_segs'], used=s['used'], err=err(s))
        h = GK._entropy(pc, batch, dp, fp)
        keep(name + ' entropy', entropy=h['entropy'], parts=h['parts'], err=err(h))
        k = GK._kl(pc, batch, dp, fp, dq, fq)
        keep(name + ' kl', kl=k['kl'], xent=k['cross_entropy'], parts=k['parts'], err=err(k))
        need = ops.align_graph_entropy_bwd_scratch_bytes(batch, GS._node_offsets(pc))
        for mode in ('entropy', 'xent', 'kl'):
            scratch = torch.full((need,), 0xFF, dtype=torch.uint8, device='cuda:0')
            g = GG._launch(pc, qc, mode, batch, dp, fp, dq, fq, scratch=scratch)
            keep('%s grad %s' % (name, mode), err=err(g), **{key: g[key] for key in GG.KEYS + ('value', 'value_plus')})
        rewards = GR.device_rewards(pc, GR.draw_rewards(pc, 31))
        fill = lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device='cuda:0')
        v = GR._value(pc, rewards, batch, dp, fp, scratch=fill(ops.align_graph_expected_reward_scratch_bytes(batch, GS._node_offsets(pc))))
        keep(name + ' expected reward', value=v['value'], parts=v['parts'], err=err(v))
        g = GR._grad(pc, rewards, batch, dp, fp, scratch=fill(ops.align_graph_expected_reward_bwd_scratch_bytes(batch, GS._node_offsets(pc))))
        keep(name + ' expected reward grad', err=err(g), **{key: g[key] for key in GR.KEYS + ('value', 'value_plus')})
        torch.cuda.synchronize()

    # ---- the test files' cases
    for k, (name, case, _) in enumerate(GS.exact_cases()):
        run('tiny ' + name, case, GK.other_side(case, 100 + k))
        run('tiny ' + name + ', identical sides', case, case)
    for name, (build, _, _) in GG.BIG_CASES.items():               # (chain: M = 256, T = 300, kp = 8)
        pc = build()
        run(name, pc, GK.other_side(pc, 5))
    run('T769, identical sides', GK._zero_case(2), GK._zero_case(2))
    run('gap, dead nodes, T below the shortest path', *GK._gap_pair())
    u = [0.7, 0.0, -1.3, 2.0]
    for bad in (False, True):                                      # (two groups; bad: no alignment, a NaN in elp)
        pc = GG._corpus(bad, u)
        run('packed corpus, bad %d' % bad, pc, GK.other_side(pc, 3))
    tab, tq, good, other, ep, eq = GG._degenerate_cases()
    cut = dict(tq, trans=tq['trans'].copy())
    cut['trans'][1, 0] = -np.inf
    dead, nan = dict(tq, len=np.full((4, 3), -np.inf)), dict(tq, trans=tq['trans'].copy())
    nan['trans'][1, 0] = np.nan
    for name, tab3 in (('q cuts an arm p uses', cut), ('q without an alignment', dead), ('a NaN in q\'s table', nan)):
        run(name, Case([(e, good, int(i == 3)) for i, e in enumerate(ep)], [tab, tab], 4),
            Case([(e, good, int(i == 3)) for i, e in enumerate(eq)], [tq, tab3], 4))
    run('q\'s workspace written for other graphs', Case([(e, good, 0) for e in ep], [tab], 4),
        Case([(e, other if i == 3 else good, 0) for i, e in enumerate(eq)], [tq], 4))
    # ---- and a few more: a trie that crosses a wave in graph_compact, skip edges, T = 257 under kp > T, closing scores
    rng = np.random.default_rng(7)
    C = 5
    while True:
        cands = [rng.integers(0, C, int(rng.integers(4, 9))) for _ in range(14)]
        if 66 <= G.trie_nodes(cands) <= 100:
            break
    trie = G.from_candidates(cands)
    opt = G.from_optional(rng.integers(0, C, 31), np.arange(31) % 2 == 0)
    for name, ep2 in (('closing scores null', None), ('closing scores given', rng.normal(size=(3, C)))):
        pc = Case([(rng.normal(size=(257, C)), trie, 0), (rng.normal(size=(280, C)), opt, 0),
                   (rng.normal(size=(90, C)), GT._branching(rng, 70, C), 0)], [_tables(rng, C, 280, 1.0)], 280, endpen=ep2)
        run('trie of %d nodes, from_optional, kp 280 > T, %s' % (len(trie), name), pc, GK.other_side(pc, 9))
    np.savez(path, **out)
    print('%s: %d calls, %d arrays' % (os.path.basename(os.environ['SMM_LIB_PATH']), len({k.rsplit('|', 1)[0] for k in out}), len(out)))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--child':
        child(sys.argv[2])
    else:
        sys.exit(driver())
