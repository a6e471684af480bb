// smm_align_logz.hip -- transcript likelihood: the sum over every segmentation of a video whose class sequence is its transcript
// a[0..M-1] (local state ids), and the gradient of that sum (include/smmdp.h: smm_align_logz_f64, smm_align_logz_bwd_f64).
//
//   forward   h[0][0] = init[a_0];  h[0][m>0] = -inf
//             gam[n][m] = cum[n][a_m] + lse_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )
//             h[n][m]   = ( gam[n][m-1] + trans[a_m][a_{m-1}] ) - cum[n][a_m]                       (0 < n < T, m >= 1)
//             logZ_a    = gam[T][M-1] + closing
//   backward  q[T][M-1] = cum[T][a_{M-1}] + closing                       (q[n][m] = cum[n][a_m] + bg[n][m]: what is stored)
//             bh[s][m]  = lse_{k=1..min(kp-1,T-s)} ( q[s+k][m] + len[k][a_m] )
//             q[n][m]   = cum[n][a_m] + ( ( trans[a_{m+1}][a_m] - cum[n][a_{m+1}] ) + bh[n][m+1] )  (0 < n < T, m < M-1)
//   E[n][m]   = exp( gam[n][m] + (q[n][m] - cum[n][a_m]) - logZ_a )       segment m ends at n; segment m + 1 starts there, so
//   occ[t][m] = P[t][m-1] - P[t][m],  P[t][m] = sum_{n <= t} E[n][m],  P[.][-1] = 1                frame t lies in segment m
//
// The column structure is smm_align.hip's (smm_align_tile.h): one workgroup per video, column m reads column m - 1 only, the
// cells off every complete alignment are skipped, tiles of SMM_ALIGN_P positions with the kp - 1 sources before them in LDS.
// The backward pass is the same loop in the walk coordinate p = T - n, from column M - 1 down to 0: its sources lie ahead in time.
//
// Numerics: every cell takes two sweeps over its sources.  The first is the alignment's add + max; the second sums
// exp(term - max): the difference is <= 0 and formed in fp64, exponentiated by v_exp_f32 and accumulated in fp64, so each cell
// has its own reference and no term of any dynamic range is lost (h holds -cum and moves by tens of nats per frame).
//
// Kernels, each one workgroup per video unless said otherwise; no atomics, no private segment, every sum in a fixed order:
//   smm_align_logz_fwd_kernel     prefix sums, the h and gam columns, logZ_a
//   smm_align_logz_bwd_kernel     the q columns
//   smm_align_logz_occ_kernel     g_elp: per tile of frames one block scan of E per transcript entry, the entries of one class
//                                 added in entry order (an LDS row per frame)
//   smm_align_logz_glen_kernel    the video's part of g_len: thread k owns length k and walks the segment starts
//   smm_align_logz_reduce_kernel  g_len: the videos' parts of a group summed in video order (one thread per (group, k, c))
//   smm_align_logz_counts_kernel  g_trans, g_init: the transcripts' transition and start counts (one workgroup per group)
// A video without an alignment (logZ_a -inf) or with the error word set (NaN) is skipped by all of the backward kernels.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3                                            // positions per thread (odd: smm_align_tile.h)
#include "smm_align_tile.h"
#include "smm_align_lse.h"

#define SMM_ALOGZ_OCC_THREADS 128
#define SMM_ALOGZ_OCC_LD (SMM_MAX_STATES_DEV + 1)               // doubles per frame row in LDS: odd, one row per thread

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_logz_fwd_kernel(SmmAlignLogzArgs a)
{
    __shared__ double s_h[SMM_ALIGN_HS];
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ double s_gam;
    __shared__ int s_flag[2];                                  // [0] an id out of range, [1] a NaN / +inf reached the DP

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const double *trans = v.trans, *len = v.len, *cum = v.cum;
    const size_t T1 = v.T1;
    double *hcol = a.cols + a.hoff[vid];                       // [M][T+1]
    double *gcol = hcol + (size_t)M * T1;                      // [M][T+1]

    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    // no alignment by counting (M segments of 1 .. kp - 1 frames each), or an id that is no state of this video
    if (!align_ids_ok(a, v, s_a, s_flag, tid, SMM_ALIGN_THREADS) || M > T || kw < 1 || (int64_t)M * kw < T) {
        if (tid == 0) a.logz[vid] = SMM_NEG_INF;
        return;
    }

    if (align_tables_bad(v, s_a, tid)) s_flag[1] = 1;
    if (align_prefix_sums(v.elp, v.cum, v.C, cm, T, s_h, tid)) s_flag[1] = 1;
    if (tid == 0) hcol[0] = v.init[s_a[0]];
    __threadfence_block();
    __syncthreads();

    // ---- columns
    int slo = 0, shi = 0;                                      // the positions of column m's sources (h[.][m])
    const int d_all = align_d_all(kw);
    for (int m = 0; m < M; ++m) {
        const int c = s_a[m];
        const bool last = m == M - 1;
        const int cn = last ? c : s_a[m + 1];
        const double tr = last ? 0.0 : trans[(size_t)cn * cm + c];
        const double *hm = hcol + (size_t)m * T1, *cumc = cum + (size_t)c * T1, *cumn = cum + (size_t)cn * T1;
        double *hn = hcol + (size_t)(m + 1) * T1;              // (never written by the last column)
        double *gm = gcol + (size_t)m * T1;
        int lo, hi;
        align_range(m, M, T, kw, lo, hi);
        __syncthreads();                                       // the previous column's readers of s_len, s_h
        if (align_stage_len(len, cm, c, kw, d_all, s_len, tid)) s_flag[1] = 1;
        alogz_column(lo, hi, slo, shi, d_all, s_h, s_len, tid,
                     [&](int s) { return hm[s]; },
                     [&](int n, double lse) {
                         const double gam = cumc[n] + lse;
                         gm[n] = gam;
                         if (last) s_gam = gam;                // (the last column is the one cell n = T)
                         else hn[n] = (gam + tr) - cumn[n];
                     });
        slo = lo;
        shi = hi;
        __threadfence_block();
    }
    __syncthreads();

    if (tid == 0) {
        const double w_end = v.endpen ? v.endpen[s_a[M - 1]] : 0.0;
        const double z = s_gam + w_end;
        const bool bad = s_flag[1] != 0 || align_bad_bits(z);
        if (bad) a.err[0] = 1;
        a.logz[vid] = bad ? __builtin_nan("") : z;
    }
}

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_logz_bwd_kernel(SmmAlignLogzArgs a)
{
    __shared__ double s_h[SMM_ALIGN_HS];
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_flag[2];

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const double lz = a.logz[vid];
    if (align_nonfinite_bits(lz)) {                            // no alignment, or the error word: nothing to differentiate
        if (tid == 0 && smm_nan_bits(lz)) a.err[0] = 1;        // (staging cleared the word the forward call had set)
        return;
    }
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const double *trans = v.trans, *len = v.len;
    const size_t T1 = v.T1;
    const double *cum = v.cum;                                 // [C][T+1], the forward call's
    double *qcol = a.cols + a.hoff[vid] + 2 * (size_t)M * T1;  // [M][T+1]

    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    if (!align_ids_ok(a, v, s_a, s_flag, tid, SMM_ALIGN_THREADS)) return;   // (a finite logZ_a had valid ids)
    if (tid == 0) {
        const int c = s_a[M - 1];
        const double w_end = v.endpen ? v.endpen[c] : 0.0;
        qcol[(size_t)(M - 1) * T1 + T] = cum[(size_t)c * T1 + T] + w_end;
    }
    __threadfence_block();
    __syncthreads();

    // ---- columns M - 1 .. 0 in the walk coordinate p = T - n: the targets are the starts of segment m, the sources its ends
    const int d_all = align_d_all(kw);
    for (int m = M - 1; m >= 0; --m) {
        const int c = s_a[m];
        const int cp = m > 0 ? s_a[m - 1] : c;
        const double tr = m > 0 ? trans[(size_t)c * cm + cp] : 0.0;
        const double *qm = qcol + (size_t)m * T1, *cumc = cum + (size_t)c * T1, *cump = cum + (size_t)cp * T1;
        double *qp = qcol + (size_t)(m > 0 ? m - 1 : 0) * T1;  // (never written by column 0)
        int lo, hi, sl, sh;
        align_range(m, M, T, kw, lo, hi);
        align_start_range(m, M, T, kw, sl, sh);
        __syncthreads();                                       // the previous column's readers of s_len, s_h
        align_stage_len(len, cm, c, kw, d_all, s_len, tid);
        alogz_column(T - sh, T - sl, T - hi, T - lo, d_all, s_h, s_len, tid,
                     [&](int p) { return qm[T - p]; },
                     [&](int p, double bh) {
                         const int s = T - p;
                         if (m > 0) qp[s] = cump[s] + ((tr - cumc[s]) + bh);
                     });
        __threadfence_block();
    }
}

// g_elp of one video.  Thread j of a tile owns frame t = f0 + j and an LDS row of class sums; per transcript entry one block scan
// of E[t][m] over the tile on top of the entry's running total gives P[t][m], and occ[t][m] = P[t][m-1] - P[t][m] goes to the
// row's class a_m.  Frames beside the video's and the rows of a skipped video keep the zeros of the call's zero fill.
__global__ void __launch_bounds__(SMM_ALOGZ_OCC_THREADS) smm_align_logz_occ_kernel(SmmAlignLogzArgs a)
{
    __shared__ double s_acc[SMM_ALOGZ_OCC_THREADS * SMM_ALOGZ_OCC_LD];
    __shared__ double s_carry[SMM_MAX_TRANSCRIPT];
    __shared__ double s_wave[2][SMM_ALOGZ_OCC_THREADS / 64];
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_flag[2];

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const double lz = a.logz[vid];
    if (align_nonfinite_bits(lz)) return;
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, C = v.C, M = v.M;
    const size_t T1 = v.T1;
    const double *cum = v.cum;
    const double *gcol = a.cols + a.hoff[vid] + (size_t)M * T1;
    const double *qcol = gcol + (size_t)M * T1;
    const double u = a.grad ? a.grad[vid] : 1.0;
    double *g_elp = a.g_elp + (size_t)v.frame_off * cm;

    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    if (!align_ids_ok(a, v, s_a, s_flag, tid, SMM_ALOGZ_OCC_THREADS)) return;
    for (int m = tid; m < M; m += SMM_ALOGZ_OCC_THREADS) s_carry[m] = 0.0;
    __syncthreads();

    double *row = s_acc + tid * SMM_ALOGZ_OCC_LD;
    for (int f0 = 0; f0 < T; f0 += SMM_ALOGZ_OCC_THREADS) {
        const int t = f0 + tid;
        for (int c = 0; c < C; ++c) row[c] = 0.0;
        double prev = 1.0;                                     // P[t][-1]: segment 0 has started
        for (int m = 0; m < M; ++m) {
            const int c = s_a[m];
            int lo, hi;
            align_range(m, M, T, kw, lo, hi);
            // E[t][m]: the last segment ends at T, behind every frame
            double e = 0.0;
            if (m < M - 1 && t >= lo && t <= hi && t < T) {
                const size_t i = (size_t)m * T1 + t;
                e = exp((gcol[i] + (qcol[i] - cum[(size_t)c * T1 + t])) - lz);
            }
            // inclusive scan over the tile on top of the entry's running total
            const double p = align_block_scan(e, s_carry[m], s_wave[m & 1], tid);
            if (tid == SMM_ALOGZ_OCC_THREADS - 1) s_carry[m] = p;
            row[c] = row[c] + (prev - p);
            prev = p;
        }
        __syncthreads();
        const int nr = T - f0 < SMM_ALOGZ_OCC_THREADS ? T - f0 : SMM_ALOGZ_OCC_THREADS;
        align_store_rows(g_elp + (size_t)f0 * cm, s_acc, SMM_ALOGZ_OCC_LD, nr, cm, C, u, tid, SMM_ALOGZ_OCC_THREADS);
        __syncthreads();
    }
}

// The video's part of g_len, [rows][c_max] at part + poff[vid] with rows = min(k_rows, T + 1), without the factor u:
//   part[k][c] = sum_{m: a_m = c} sum_s exp( h[s][m] + len[k][c] + q[s+k][m] - logZ_a )
// Thread k owns row k (k = tid + 1, + THREADS, ...): the entries in order, the starts in order.  The exponent is the log of an
// edge's posterior probability, <= 0 up to rounding, formed in fp64.
__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_logz_glen_kernel(SmmAlignLogzArgs a)
{
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_flag[2];

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const double lz = a.logz[vid];
    if (align_nonfinite_bits(lz)) return;                      // (the reduction skips this video's part)
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, M = v.M;
    const int kw = v.kw < T ? v.kw : T;                        // (a segment is no longer than the video)
    const int kw_cone = v.kw;
    const int rows = a.k_rows < T + 1 ? a.k_rows : T + 1;
    const double *len = v.len;
    const size_t T1 = v.T1;
    const double *hcol = a.cols + a.hoff[vid];
    const double *qcol = hcol + 2 * (size_t)M * T1;
    double *part = a.part + a.poff[vid];

    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    if (!align_ids_ok(a, v, s_a, s_flag, tid, SMM_ALIGN_THREADS)) return;
    for (int e = tid; e < rows * cm; e += SMM_ALIGN_THREADS) part[e] = 0.0;
    __threadfence_block();
    __syncthreads();

    for (int k = tid + 1; k <= kw && k < rows; k += SMM_ALIGN_THREADS) {
        double *prow = part + (size_t)k * cm;
        for (int m = 0; m < M; ++m) {
            const int c = s_a[m];
            int lo, hi, sl, sh;
            align_range(m, M, T, kw_cone, lo, hi);
            align_start_range(m, M, T, kw_cone, sl, sh);
            const int s_first = sl > lo - k ? sl : lo - k, s_last = sh < hi - k ? sh : hi - k;
            const double base = len[(size_t)k * cm + c] - lz;
            const double *hm = hcol + (size_t)m * T1, *qm = qcol + (size_t)m * T1 + k;
            double acc = 0.0;
            for (int s = s_first; s <= s_last; ++s)
                acc = acc + (double)__expf((float)((hm[s] + qm[s]) + base));
            prow[c] = prow[c] + acc;
        }
    }
}

// g_len[g][k][c] = sum over the group's videos, in video order, of u_i * part_i[k][c]; rows a video does not have add nothing
__global__ void __launch_bounds__(256) smm_align_logz_reduce_kernel(SmmAlignLogzArgs a)
{
    const int cm = a.c_max, g = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.k_rows * cm) return;
    const int k = e / cm;
    double sum = 0.0;
    for (int i = 0; i < a.b; ++i) {
        const SmmVideo mv = a.videos[i];
        if (mv.group != g || align_nonfinite_bits(a.logz[i])) continue;
        const int rows = a.k_rows < mv.T + 1 ? a.k_rows : mv.T + 1;
        if (k >= rows) continue;
        const double u = a.grad ? a.grad[i] : 1.0;
        sum = sum + u * a.part[a.poff[i] + e];
    }
    a.g_len[(size_t)g * a.k_rows * cm + e] = sum;
}

// g_trans[g][c][c'] = sum_i u_i #{m >= 1: a_m = c, a_{m-1} = c'},  g_init[g][c] = sum_i u_i [a_0 = c], in video order
__global__ void __launch_bounds__(256) smm_align_logz_counts_kernel(SmmAlignLogzArgs a)
{
    const int cm = a.c_max, g = blockIdx.x;
    for (int e = threadIdx.x; e < cm * cm; e += 256) {
        const int c = e / cm, cp = e - c * cm;
        double gt = 0.0, gi = 0.0;
        for (int i = 0; i < a.b; ++i) {
            if (a.videos[i].group != g || align_nonfinite_bits(a.logz[i])) continue;
            const double u = a.grad ? a.grad[i] : 1.0;
            const int64_t t0 = a.toff[i], t1 = a.toff[i + 1];
            int n = 0;
            int before = a.transcript[t0];
            if (cp == 0 && before == c) gi = gi + u;
            for (int64_t j = t0 + 1; j < t1; ++j) {
                const int id = a.transcript[j];
                n += (id == c && before == cp) ? 1 : 0;
                before = id;
            }
            gt = gt + u * (double)n;
        }
        a.g_trans[(size_t)g * cm * cm + e] = gt;
        if (cp == 0) a.g_init[(size_t)g * cm + c] = gi;
    }
}

void smm_launch_align_logz_fwd(const SmmAlignLogzArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_logz_fwd_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}

void smm_launch_align_logz_bwd(const SmmAlignLogzArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_logz_bwd_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_align_logz_occ_kernel, dim3((unsigned)a.b), dim3(SMM_ALOGZ_OCC_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_align_logz_glen_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
    const unsigned cells = (unsigned)(a.k_rows * a.c_max);
    hipLaunchKernelGGL(smm_align_logz_reduce_kernel, dim3((cells + 255) / 256, (unsigned)a.n_groups), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(smm_align_logz_counts_kernel, dim3((unsigned)a.n_groups), dim3(256), 0, stream, a);
}
