// smm_align.hip -- forced alignment: the best segmentation of a video whose class sequence (its transcript a[0..M-1], local
// state ids, consecutive repeats allowed) is given; only the boundaries are free (include/smmdp.h: smm_align_f64).
//
//   cum[0][c] = 0;  cum[n][c] = cum[n-1][c] + elp[n-1][c]                        (serial fp64 prefix sums, as the C twin's)
//   h[0][0] = init[a_0];  h[0][m>0] = -inf
//   gam[n][m] = cum[n][a_m] + max_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )
//   h[n][m]   = ( gam[n][m-1] + trans[a_m][a_{m-1}] ) - cum[n][a_m]               (0 < n < T, m >= 1)
//   best      = gam[T][M-1] + (endpen ? endpen[a_{M-1}] : 0.0)
// Every add is one IEEE fp64 add in this association (max is exact), so best and the boundaries are what
// smm_oracle_viterbi_ex (oracle/smm_oracle.c) returns on the lattice whose states are the transcript positions.
//
// smm_align_kernel: one workgroup per video.  There is no serial chain over T: column m ("segment m ends at n") depends on
// column m - 1 only, and inside a column every position is independent.  Phases, a workgroup barrier between them:
//   - prefix sums: elp tiles go through LDS; one lane per class adds serially; cum is kept class-major [C][T+1];
//   - columns m = 0 .. M-1 over the cells that lie on a complete alignment,
//       max(m+1, T - (M-1-m)(kp-1)) <= n <= min(T - (M-1-m), (m+1)(kp-1))
//     (cells outside are -inf or cannot reach (T, M-1): skipping them changes nothing), in tiles of SMM_ALIGN_P positions: the
//     tile's h values and the kp - 1 before it sit in LDS, the column's length scores too.  A thread owns SMM_ALIGN_R
//     consecutive positions and walks the distance d = (its first position) - (source position) upward: one LDS read of h
//     serves its R cells, the length scores slide through R registers (one broadcast read per step), one add and one max
//     per cell.  R is odd: the threads' h reads are R doubles apart, which spreads a half-wave over all 64 banks.
//     The column writes h[.][m+1] straight from its gam; the h columns stay in the workspace, column-major [M][T+1];
//   - back-trace (wave 0): M decisions, each the twin's rule -- the smallest k whose (cum[n] + (h[n-k][m] + len[k])) + w equals
//     the maximum of that expression over k;
//   - outputs: every span position and frame finds its segment by bisection over the segment starts in LDS.
// The tile walk, the sweep over the distances, the prologue and the output phase are smm_align_tile.h's.
// No atomics, no private segment; NaN / +inf detection on the bits (smm_nan_bits' reasoning).
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3                                            // positions per thread (odd: see above)
#include "smm_align_tile.h"                                      // the tile geometry that follows from the two, and the shared phases

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_kernel(SmmAlignArgs a)
{
    __shared__ double s_h[SMM_ALIGN_HS];
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_start[SMM_MAX_TRANSCRIPT + 1];
    __shared__ double s_gam;
    __shared__ int s_flag[2];                                  // [0] an id out of range, [1] a NaN / +inf reached the DP

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const double *trans = v.trans, *len = v.len, *cum = v.cum;
    const size_t T1 = v.T1;
    double *hcol = a.hcols + a.hoff[vid];                      // [M][T+1]

    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    // no alignment by counting (M segments of 1 .. kp - 1 frames each), or an id that is no state of this video
    if (!align_ids_ok(a, v, s_a, s_flag, tid, SMM_ALIGN_THREADS) || M > T || kw < 1 || (int64_t)M * kw < T) {
        align_write_none(a, v, vid, tid);
        return;
    }

    if (align_tables_bad(v, s_a, tid)) s_flag[1] = 1;
    // ---- prefix sums (smm_align_tile.h): tiles of frames through LDS, lane c adds class c serially, cum[c][n] class-major
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
        int lo, hi;
        align_range(m, M, T, kw, lo, hi);
        __syncthreads();                                       // the previous column's readers of s_len, s_h
        if (align_stage_len(len, cm, c, kw, d_all, s_len, tid)) s_flag[1] = 1;
        // (d_first < d_end on every tile: tb <= hi <= shi + kw gives tb - shi <= kw < d_all)
        align_tiles(lo, hi, slo, shi, d_all, s_h, tid, [&](int s) { return hm[s]; },
                    [&](int n0, int d_first, int d_end, const double *hp) {
                        double acc[SMM_ALIGN_R];
                        align_sweep_max(d_first, d_end, hp, s_len, acc);
#pragma unroll
                        for (int r = 0; r < SMM_ALIGN_R; ++r) {
                            const int n = n0 + r;
                            if (n <= hi) {
                                const double gam = cumc[n] + acc[r];
                                if (last) s_gam = gam;         // (the last column is the one cell n = T)
                                else hn[n] = (gam + tr) - cumn[n];
                            }
                        }
                    });
        slo = lo;
        shi = hi;
        __threadfence_block();
    }
    __syncthreads();

    // ---- closing step and back-trace (wave 0)
    const int c_last = s_a[M - 1];
    const double w_end = v.endpen ? v.endpen[c_last] : 0.0;
    const double best = s_gam + w_end;
    const bool bad = s_flag[1] != 0 || align_bad_bits(best);
    const bool none = !bad && align_nonfinite_bits(best);     // -inf: the tables leave no alignment
    if (!bad && !none && tid < 64) {
        int n = T;
        double w = w_end;
        bool fail = false;
        for (int m = M - 1; m >= 0; --m) {
            const int c = s_a[m];
            int lo, hi;
            align_start_range(m, M, T, kw, lo, hi);
            const double *hm = hcol + (size_t)m * T1;
            const double cn = cum[(size_t)c * T1 + n];
            const int kmax = kw < n ? kw : n;
            const int k_lo = n - hi > 1 ? n - hi : 1, k_hi = n - lo < kmax ? n - lo : kmax;
            double mx = SMM_NEG_INF;
            for (int k = k_lo + tid; k <= k_hi; k += 64)
                mx = align_max(mx, (cn + (hm[n - k] + len[(size_t)k * cm + c])) + w);
            mx = align_wave_max(mx);
            int kb = 0x7fffffff;
            for (int k = k_lo + tid; k <= k_hi; k += 64) {
                const double val = (cn + (hm[n - k] + len[(size_t)k * cm + c])) + w;
                if (val == mx && k < kb) kb = k;
            }
            kb = align_wave_min(kb);
            if (kb == 0x7fffffff || align_nonfinite_bits(mx)) { fail = true; break; }
            n -= kb;
            if (tid == 0) s_start[m] = n;
            if (m > 0) w = trans[(size_t)c * cm + s_a[m - 1]];
        }
        if (fail || n != 0) {
            if (tid == 0) s_flag[1] = 1;
        }
    }
    __syncthreads();
    const bool failed = s_flag[1] != 0;

    // ---- outputs (smm_align_tile.h): segment m carries entry m
    align_write_result(a, v, vid, s_start, [&](int l) { return s_a[l]; }, 0, failed, failed || none, best, tid);
}

void smm_launch_align(const SmmAlignArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}
