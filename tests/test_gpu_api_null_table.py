"""The entry points that look at their table pointers only AFTER staging (smm_logz_f64, smm_logz_bwd_f64, smm_sample_f64,
smm_viterbi_f32, smm_kbest_f64): a null ``trans`` is SMM_ERR_ARG, and the refused call leaves the workspace fit for the valid
call that follows -- its outputs are bit-equal to the same call on a fresh workspace."""
import ctypes

import pytest
import torch

from action_segmentation_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ERR_ARG = -1
K_BEST, N_SAMPLES, SEED = 3, 4, 7


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _call(fn, batch, ws, *args):
    ln, fo, gr, kp, ns = batch.host_ptrs()
    return getattr(_lib.load(), fn)(ctypes.byref(batch.shape), ctypes.c_void_p(ln), ctypes.c_void_p(fo), ctypes.c_void_p(gr),
                                    ctypes.c_void_p(kp), ctypes.c_void_p(ns), *args, _ptr(ws), ctypes.c_size_t(ws.numel()),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return torch.equal(a.view(torch.uint8), b.view(torch.uint8))             # bit-equal (NaN and -0.0 included)


def test_null_trans_after_staging_is_refused_and_leaves_the_workspace_usable():
    batch = ops.Batch([5, 3], [3], 4)
    g = torch.Generator().manual_seed(3)
    f64 = torch.float64
    elp = torch.randn(batch.total_frames, 3, generator=g, dtype=f64).to(DEV)
    trans = torch.randn(1, 3, 3, generator=g, dtype=f64).to(DEV)
    init = torch.randn(1, 3, generator=g, dtype=f64).to(DEV)
    lens = torch.randn(1, 4, 3, generator=g, dtype=f64).to(DEV)
    need = ops.kbest_workspace_bytes(batch, K_BEST)
    assert need >= batch.workspace_bytes()
    b, tf = batch.b, batch.total_frames

    def run(refuse):
        """Every entry point's valid call on one fresh workspace; with `refuse`, each behind its refused twin."""
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        out = {}

        def both(fn, pre, post):
            if refuse:
                assert _call(fn, batch, ws, *pre(None), *post) == ERR_ARG, fn
            assert _call(fn, batch, ws, *pre(trans), *post) == 0, fn

        tables = lambda e, i, l: (lambda t: (_ptr(e), _ptr(t), _ptr(i), _ptr(l), None))
        logz = torch.empty(b, dtype=f64, device=DEV)
        both('smm_logz_f64', tables(elp, init, lens), (_ptr(logz),))
        out['logz'] = logz
        grads = [torch.empty_like(t) for t in (elp, trans, init, lens)]
        both('smm_logz_bwd_f64', tables(elp, init, lens), (_ptr(logz), None) + tuple(_ptr(t) for t in grads))
        out.update(zip(('g_elp', 'g_trans', 'g_init', 'g_len'), grads))
        spans = torch.full((N_SAMPLES, b, batch.t_max + 1), -7, dtype=torch.int64, device=DEV)
        logp = torch.empty((N_SAMPLES, b), dtype=f64, device=DEV)
        both('smm_sample_f64', tables(elp, init, lens),
             (None, _ptr(logz), ctypes.c_int32(N_SAMPLES), ctypes.c_uint64(SEED), _ptr(spans), None, _ptr(logp)))
        out.update(sample_spans=spans, logp=logp)
        vspans = torch.full((b, batch.t_max + 1), -7, dtype=torch.int64, device=DEV)
        vlabels = torch.full((tf,), -1, dtype=torch.int64, device=DEV)
        best = torch.empty(b, dtype=f64, device=DEV)
        n_segs = torch.empty(b, dtype=torch.int32, device=DEV)
        both('smm_viterbi_f32', tables(elp.float(), init.float(), lens.float()),
             (None, _ptr(vspans), _ptr(vlabels), _ptr(best), _ptr(n_segs)))
        out.update(spans=vspans, labels=vlabels, best=best, n_segs=n_segs)
        kspans = torch.full((K_BEST, b, batch.t_max + 1), -7, dtype=torch.int64, device=DEV)
        klabels = torch.full((K_BEST, tf), -1, dtype=torch.int64, device=DEV)
        score = torch.empty((K_BEST, b), dtype=f64, device=DEV)
        kn = torch.empty((K_BEST, b), dtype=torch.int32, device=DEV)
        both('smm_kbest_f64', tables(elp, init, lens), (None, ctypes.c_int32(K_BEST), _ptr(kspans), _ptr(klabels), _ptr(score), _ptr(kn)))
        out.update(kbest_spans=kspans, kbest_labels=klabels, score=score, kbest_n_segs=kn)
        torch.cuda.synchronize()
        assert ops.error_flag(batch, ws=ws) == 0
        return out

    fresh, after = run(False), run(True)
    assert torch.isfinite(fresh['logz']).all() and torch.isfinite(fresh['best']).all() and int(fresh['n_segs'].min()) >= 1
    for name in fresh:
        assert _same(fresh[name], after[name]), name
