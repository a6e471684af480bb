// smm_align_lse.h -- the log-semiring span loop of the transcript-likelihood kernels (smm_align_logz.hip: exact transcripts;
// smm_align_opt_logz.hip: optional entries; smm_align_graph_logz.hip: the paths of a graph): one column of lse_k( src(p - k) + len[k] ) over smm_align_tile.h's tiles,
// the same column for the entropy of each cell's distribution over k (smm_align_graph_entropy.hip), and for the KL between two
// sides' distributions over k (smm_align_graph_kl.hip).
// Include after smm_align_tile.h.
#pragma once

// One column in the walk coordinate: every target p in [lo, hi] gets lse over the sources p - k, k = 1 .. kw, that lie in
// [slo, shi]: out(p, lse_k( src(p - k) + len[k] )).  s_len holds the column's length scores (align_stage_len).  Every cell takes
// two sweeps over its sources: the alignment's add + max, then the sum of exp(term - max).
template <class Src, class Out>
__device__ __forceinline__ void alogz_column(int lo, int hi, int slo, int shi, int d_all, double *s_h, const double *s_len,
                                             int tid, Src src, Out out)
{
    align_tiles(lo, hi, slo, shi, d_all, s_h, tid, src, [&](int n0, int d_from, int d_end, const double *hp) {
        double acc[SMM_ALIGN_R], sum[SMM_ALIGN_R];
        // (d_from >= d_end: no source is in reach of this tile -- a graph's column can have one -- and its cells are -inf)
        const int d_first = d_from < d_end ? d_from : d_end;
        // sweep 1: the largest term of each cell
        align_sweep_max(d_first, d_end, hp, s_len, acc);
        // sweep 2: sum exp(term - max); a cell without a finite term takes the reference 0 and sums zeros
#pragma unroll
        for (int r = 0; r < SMM_ALIGN_R; ++r) {
            acc[r] = align_nonfinite_bits(acc[r]) ? 0.0 : acc[r];
            sum[r] = 0.0;
        }
        align_sweep(d_first, d_end, hp, s_len, [&](int r, double t) { sum[r] = sum[r] + (double)__expf((float)(t - acc[r])); });
#pragma unroll
        for (int r = 0; r < SMM_ALIGN_R; ++r)
            if (n0 + r <= hi) out(n0 + r, acc[r] + log(sum[r]));
    });
}

// The same column for the entropy of each cell's distribution over its sources, p_k ~ exp(src(p - k) + len[k])
// (smm_align_graph_entropy.hip): out(p, log Z - A / Z) with Z = sum exp(term - max) and A = sum exp(term - max) (term - max),
// the second sweep carrying both.  A term of -inf has no mass (0, not 0 * -inf); a cell with one finite term gives exactly 0
// (log 1 - 0 / 1); one with none gives NaN: the caller gives it no weight.  Never negative: Z >= 1 and A <= 0.
template <class Src, class Out>
__device__ __forceinline__ void alogz_entropy_column(int lo, int hi, int slo, int shi, int d_all, double *s_h, const double *s_len,
                                                     int tid, Src src, Out out)
{
    align_tiles(lo, hi, slo, shi, d_all, s_h, tid, src, [&](int n0, int d_from, int d_end, const double *hp) {
        double acc[SMM_ALIGN_R], sum[SMM_ALIGN_R], dot[SMM_ALIGN_R];
        const int d_first = d_from < d_end ? d_from : d_end;
        align_sweep_max(d_first, d_end, hp, s_len, acc);
#pragma unroll
        for (int r = 0; r < SMM_ALIGN_R; ++r) {
            acc[r] = align_nonfinite_bits(acc[r]) ? 0.0 : acc[r];
            sum[r] = 0.0;
            dot[r] = 0.0;
        }
        align_sweep(d_first, d_end, hp, s_len, [&](int r, double t) {
            const double x = t - acc[r];
            const double e = (double)__expf((float)x);
            sum[r] = sum[r] + e;
            dot[r] = dot[r] + (e > 0.0 ? e * x : 0.0);
        });
#pragma unroll
        for (int r = 0; r < SMM_ALIGN_R; ++r)
            if (n0 + r <= hi) out(n0 + r, log(sum[r]) - dot[r] / sum[r]);
    });
}

// ---- two sides of one decision (smm_align_graph_kl.hip): the candidates' weights wp under p and wq under q, mp and mq the
// largest finite weight of each side (0 where a side has none).  Over the candidates that have mass under p (ep > 0):
//   Sp = sum ep,  Sq = sum exp(wq - mq) (over every candidate: q's normaliser),  Y = sum ep (wq - wp),  Ap = sum ep (wp - mp)
//   KLloc = (mq - mp) + log Sq - log Sp - Y / Sp  clamped at 0,   Hloc = log Sp - Ap / Sp
// Every exponential in fp64 on both sides: what is left of log Sq - log Sp between two near-identical sides is the whole value.
// Both sides run the same operations: bit-identical sides give exactly 0.0.  A candidate with mass under p and wq = -inf (cut)
// makes KLloc +inf; one without mass under p contributes to Sq only (0, never 0 * inf).
// The second pass's step:
__device__ __forceinline__ void akl_add(double wp, double wq, double mp, double mq, double &sp, double &sq, double &y, double &ap,
                                        bool &cut)
{
    const double xp = wp - mp;
    const double ep = exp(xp);
    sp = sp + ep;
    sq = sq + exp(wq - mq);
    if (ep > 0.0) {
        const double dw = wq - wp;
        ap = ap + ep * xp;
        if (dw == SMM_NEG_INF) cut = true; else y = y + ep * dw;
    }
}

// ... and what the sums give.  A decision without mass under p (Sp = 0) gives NaN: the caller gives it no weight.
__device__ __forceinline__ void akl_loc(double mp, double mq, double sp, double sq, double y, double ap, bool cut, double &kl,
                                        double &hl)
{
    const double lsp = log(sp);
    const double k = (((mq - mp) + log(sq)) - lsp) - y / sp;
    kl = cut ? __builtin_huge_val() : (k > 0.0 ? k : (k == k ? 0.0 : k));   // (NaN stays NaN: not reached with mass under p)
    hl = lsp - ap / sp;
}

// The column of alogz_entropy_column for both sides at once: the same tiles hold p's sources in s_hp and q's in s_hq, sweep 1
// takes both maxima, sweep 2 carries Sp, Sq, Y, Ap; out(p, KLloc, Hloc) per cell.
template <class SrcP, class SrcQ, class Out>
__device__ __forceinline__ void alogz_kl_column(int lo, int hi, int slo, int shi, int d_all, double *s_hp, double *s_hq,
                                                const double *s_lenp, const double *s_lenq, int tid, SrcP srcp, SrcQ srcq, Out out)
{
    align_tiles2(lo, hi, slo, shi, d_all, s_hp, s_hq, tid, srcp, srcq,
                 [&](int n0, int d_from, int d_end, const double *hp, const double *hq) {
        double mp[SMM_ALIGN_R], mq[SMM_ALIGN_R], sp[SMM_ALIGN_R], sq[SMM_ALIGN_R], y[SMM_ALIGN_R], ap[SMM_ALIGN_R];
        bool cut[SMM_ALIGN_R];
        const int d_first = d_from < d_end ? d_from : d_end;
#pragma unroll
        for (int r = 0; r < SMM_ALIGN_R; ++r) mp[r] = mq[r] = SMM_NEG_INF;
        align_sweep2(d_first, d_end, hp, hq, s_lenp, s_lenq, [&](int r, double tp, double tq) {
            mp[r] = align_max(mp[r], tp);
            mq[r] = align_max(mq[r], tq);
        });
#pragma unroll
        for (int r = 0; r < SMM_ALIGN_R; ++r) {
            mp[r] = align_nonfinite_bits(mp[r]) ? 0.0 : mp[r];
            mq[r] = align_nonfinite_bits(mq[r]) ? 0.0 : mq[r];
            sp[r] = sq[r] = y[r] = ap[r] = 0.0;
            cut[r] = false;
        }
        align_sweep2(d_first, d_end, hp, hq, s_lenp, s_lenq, [&](int r, double tp, double tq) {
            akl_add(tp, tq, mp[r], mq[r], sp[r], sq[r], y[r], ap[r], cut[r]);
        });
#pragma unroll
        for (int r = 0; r < SMM_ALIGN_R; ++r)
            if (n0 + r <= hi) {
                double kl, hl;
                akl_loc(mp[r], mq[r], sp[r], sq[r], y[r], ap[r], cut[r], kl, hl);
                out(n0 + r, kl, hl);
            }
    });
}
