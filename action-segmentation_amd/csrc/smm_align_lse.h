// smm_align_lse.h -- the log-semiring span loop of the transcript-likelihood kernels (smm_align_logz.hip: exact transcripts;
// smm_align_opt_logz.hip: optional entries): one column of lse_k( src(p - k) + len[k] ) over smm_align_tile.h's tiles, and the
// staging of a column's length scores.  Include after smm_align_tile.h.
#pragma once

// One column in the walk coordinate: every target p in [lo, hi] gets lse over the sources p - k, k = 1 .. kw, that lie in
// [slo, shi]: out(p, lse_k( src(p - k) + len[k] )).  s_len holds the column's length scores at index k + R (-inf outside
// 1 .. kw), written by the caller without a barrier behind them.  Tile and distance bounds as in smm_align_kernel.
template <class Src, class Out>
__device__ __forceinline__ void alogz_column(int lo, int hi, int slo, int shi, int d_all, double *s_h, const double *s_len,
                                             int tid, Src src, Out out)
{
    for (int tb = lo; tb <= hi; tb += SMM_ALIGN_P) {
        // distances that can meet a source: tb - shi <= d <= tb + P - R - slo; whole steps of R, from -R (cell r at d has k = d + r)
        const int x = tb - shi, y = tb + SMM_ALIGN_P - SMM_ALIGN_R - slo + 1;
        const int d_first = x <= 0 ? -SMM_ALIGN_R : x / SMM_ALIGN_R * SMM_ALIGN_R;
        const int y_up = (y + SMM_ALIGN_R - 1) / SMM_ALIGN_R * SMM_ALIGN_R;
        const int d_end = y_up < d_all ? y_up : d_all;
        // LDS index i <-> position tb - OFF + i, for the positions tb - (d_end - 1) .. tb + P - R - d_first
        const int i_first = SMM_ALIGN_OFF - (d_end - 1), i_last = SMM_ALIGN_OFF + SMM_ALIGN_P - SMM_ALIGN_R - d_first;
        __syncthreads();                                       // the previous tile's readers
        for (int i = i_first + tid; i <= i_last; i += SMM_ALIGN_THREADS) {
            const int s = tb - SMM_ALIGN_OFF + i;
            s_h[i] = (s >= slo && s <= shi) ? src(s) : SMM_NEG_INF;
        }
        __syncthreads();
        const int n0 = tb + tid * SMM_ALIGN_R;
        if (n0 <= hi) {
            double acc[SMM_ALIGN_R], sum[SMM_ALIGN_R], lw[SMM_ALIGN_R];
            const double *hp = s_h + SMM_ALIGN_OFF + tid * SMM_ALIGN_R;
            // sweep 1: the largest term of each cell (lw[(d + r) % R] = len[d + r]; d_first is a multiple of R)
#pragma unroll
            for (int r = 0; r < SMM_ALIGN_R; ++r) acc[r] = SMM_NEG_INF;
#pragma unroll
            for (int q = 0; q < SMM_ALIGN_R - 1; ++q) lw[q] = s_len[d_first + q + SMM_ALIGN_R];
            for (int d0 = d_first; d0 < d_end; d0 += SMM_ALIGN_R) {
#pragma unroll
                for (int j = 0; j < SMM_ALIGN_R; ++j) {
                    const int d = d0 + j;
                    const double hv = hp[-d];
                    lw[(j + SMM_ALIGN_R - 1) % SMM_ALIGN_R] = s_len[d + 2 * SMM_ALIGN_R - 1];
#pragma unroll
                    for (int r = 0; r < SMM_ALIGN_R; ++r)
                        acc[r] = align_max(acc[r], hv + lw[(j + r) % SMM_ALIGN_R]);
                }
            }
            // sweep 2: sum exp(term - max); a cell without a finite term takes the reference 0 and sums zeros
#pragma unroll
            for (int r = 0; r < SMM_ALIGN_R; ++r) {
                acc[r] = align_nonfinite_bits(acc[r]) ? 0.0 : acc[r];
                sum[r] = 0.0;
            }
#pragma unroll
            for (int q = 0; q < SMM_ALIGN_R - 1; ++q) lw[q] = s_len[d_first + q + SMM_ALIGN_R];
            for (int d0 = d_first; d0 < d_end; d0 += SMM_ALIGN_R) {
#pragma unroll
                for (int j = 0; j < SMM_ALIGN_R; ++j) {
                    const int d = d0 + j;
                    const double hv = hp[-d];
                    lw[(j + SMM_ALIGN_R - 1) % SMM_ALIGN_R] = s_len[d + 2 * SMM_ALIGN_R - 1];
#pragma unroll
                    for (int r = 0; r < SMM_ALIGN_R; ++r)
                        sum[r] = sum[r] + (double)__expf((float)((hv + lw[(j + r) % SMM_ALIGN_R]) - acc[r]));
                }
            }
#pragma unroll
            for (int r = 0; r < SMM_ALIGN_R; ++r)
                if (n0 + r <= hi) out(n0 + r, acc[r] + log(sum[r]));
        }
    }
}

// the column's length scores -> s_len (index k + R); true where one of them is NaN or +inf
__device__ __forceinline__ bool alogz_stage_len(const double *len, int cm, int c, int kw, int d_all, double *s_len, int tid)
{
    bool bad = false;
    for (int j = tid; j < d_all + 3 * SMM_ALIGN_R; j += SMM_ALIGN_THREADS) {
        const int k = j - SMM_ALIGN_R;
        double v = SMM_NEG_INF;
        if (k >= 1 && k <= kw) {
            v = len[(size_t)k * cm + c];
            bad |= align_bad_bits(v);
        }
        s_len[j] = v;
    }
    return bad;
}
