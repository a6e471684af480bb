// smm_align_lse.h -- the log-semiring span loop of the transcript-likelihood kernels (smm_align_logz.hip: exact transcripts;
// smm_align_opt_logz.hip: optional entries; smm_align_graph_logz.hip: the paths of a graph): one column of lse_k( src(p - k) + len[k] ) over smm_align_tile.h's tiles,
// and the same column for the entropy of each cell's distribution over k (smm_align_graph_entropy.hip).
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
