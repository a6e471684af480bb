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
// No atomics, no private segment; NaN / +inf detection on the bits (smm_nan_bits' reasoning).
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3                                            // positions per thread (odd: see above)
#include "smm_align_tile.h"                                      // the tile geometry that follows from the two, and the shared phases
#include "smm_launch.h"

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
    const SmmVideo mv = a.videos[vid];
    const int T = mv.T, g = mv.group, cm = a.c_max, kw = mv.kp - 1;
    const int C = a.n_states[g];
    const int64_t t0 = a.toff[vid];
    const int M = (int)(a.toff[vid + 1] - t0);
    const double *elp = a.elp + (size_t)mv.frame_off * cm;
    const double *trans = a.trans + (size_t)g * cm * cm;
    const double *len = a.len + (size_t)g * a.k_rows * cm;
    const int64_t *cmap = a.class_map ? a.class_map + (size_t)g * (cm + 1) : nullptr;
    const size_t T1 = (size_t)T + 1;
    double *cum = a.hist + mv.hist_off;                        // [C][T+1]
    double *hcol = a.hcols + a.hoff[vid];                      // [M][T+1]
    int64_t *spans = a.spans ? a.spans + (size_t)vid * (a.t_max + 1) : nullptr;
    int64_t *labels = a.labels ? a.labels + mv.frame_off : nullptr;

    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    for (int m = tid; m < M; m += SMM_ALIGN_THREADS) {
        const int id = a.transcript[t0 + m];
        const bool ok = id >= 0 && id < C;
        s_a[m] = ok ? id : 0;                                  // (never used as an index when the flag is up)
        if (!ok) s_flag[0] = 1;
    }
    __syncthreads();
    // no alignment by counting (M segments of 1 .. kp - 1 frames each), or an id that is no state of this video
    if (s_flag[0] || M > T || kw < 1 || (int64_t)M * kw < T) {
        if (spans)
            for (int q = tid; q <= a.t_max; q += SMM_ALIGN_THREADS) spans[q] = -1;
        if (labels)
            for (int f = tid; f < T; f += SMM_ALIGN_THREADS) labels[f] = -1;
        if (tid == 0) {
            if (a.best) a.best[vid] = SMM_NEG_INF;
            if (a.n_segs) a.n_segs[vid] = 0;
        }
        return;
    }

    // ---- the tables this transcript reads: a NaN or +inf among them reaches the DP
    if (tid < M) {
        const int c = s_a[tid];
        double v = tid == 0 ? a.init[(size_t)g * cm + c] : trans[(size_t)c * cm + s_a[tid - 1]];
        bool bad = align_bad_bits(v);
        if (tid == M - 1 && a.endpen) bad |= align_bad_bits(a.endpen[(size_t)vid * cm + c]);
        if (bad) s_flag[1] = 1;
    }

    // ---- prefix sums (smm_align_tile.h): tiles of frames through LDS, lane c adds class c serially, cum[c][n] class-major
    if (align_prefix_sums(elp, cum, C, cm, T, s_h, tid)) s_flag[1] = 1;
    if (tid == 0) hcol[0] = a.init[(size_t)g * cm + s_a[0]];
    __threadfence_block();
    __syncthreads();

    // ---- columns
    int slo = 0, shi = 0;                                      // the positions of column m's sources (h[.][m])
    const int d_all = (kw + 1 + SMM_ALIGN_R - 1) / SMM_ALIGN_R * SMM_ALIGN_R;   // distances -R .. d_all - 1 cover k = 1 .. kw
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
        for (int j = tid; j < d_all + 3 * SMM_ALIGN_R; j += SMM_ALIGN_THREADS) {
            const int k = j - SMM_ALIGN_R;
            double v = SMM_NEG_INF;
            if (k >= 1 && k <= kw) {
                v = len[(size_t)k * cm + c];
                if (align_bad_bits(v)) s_flag[1] = 1;
            }
            s_len[j] = v;
        }
        for (int tb = lo; tb <= hi; tb += SMM_ALIGN_P) {
            // distances that can meet a source: tb - shi <= d <= tb + P - R - slo; whole steps of R, from -R (cell r at d has k = d + r)
            const int x = tb - shi, y = tb + SMM_ALIGN_P - SMM_ALIGN_R - slo + 1;
            const int d_first = x <= 0 ? -SMM_ALIGN_R : x / SMM_ALIGN_R * SMM_ALIGN_R;
            const int y_up = (y + SMM_ALIGN_R - 1) / SMM_ALIGN_R * SMM_ALIGN_R;
            const int d_end = y_up < d_all ? y_up : d_all;
            // LDS index i <-> position tb - OFF + i, for the positions tb - (d_end - 1) .. tb + P - R - d_first
            const int i_first = SMM_ALIGN_OFF - (d_end - 1), i_last = SMM_ALIGN_OFF + SMM_ALIGN_P - SMM_ALIGN_R - d_first;
            __syncthreads();                                   // the previous tile's readers
            for (int i = i_first + tid; i <= i_last; i += SMM_ALIGN_THREADS) {
                const int s = tb - SMM_ALIGN_OFF + i;
                s_h[i] = (s >= slo && s <= shi) ? hm[s] : SMM_NEG_INF;
            }
            __syncthreads();
            const int n0 = tb + tid * SMM_ALIGN_R;
            // d_first < d_end on every tile: tb <= hi <= shi + kw gives tb - shi <= kw < d_all, and y > x.  (If it were not, the
            // loop below would not run and the cells would be -inf, which is what "no source in reach" means.)
            if (n0 <= hi) {
                double acc[SMM_ALIGN_R], lw[SMM_ALIGN_R];
#pragma unroll
                for (int r = 0; r < SMM_ALIGN_R; ++r) acc[r] = SMM_NEG_INF;
                // lw[(d + r) % R] = len[d + r]; d_first is a multiple of R
#pragma unroll
                for (int q = 0; q < SMM_ALIGN_R - 1; ++q) lw[q] = s_len[d_first + q + SMM_ALIGN_R];
                const double *hp = s_h + SMM_ALIGN_OFF + tid * SMM_ALIGN_R;
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
#pragma unroll
                for (int r = 0; r < SMM_ALIGN_R; ++r) {
                    const int n = n0 + r;
                    if (n <= hi) {
                        const double gam = cumc[n] + acc[r];
                        if (last) s_gam = gam;                 // (the last column is the one cell n = T)
                        else hn[n] = (gam + tr) - cumn[n];
                    }
                }
            }
        }
        slo = lo;
        shi = hi;
        __threadfence_block();
    }
    __syncthreads();

    // ---- closing step and back-trace (wave 0)
    const int c_last = s_a[M - 1];
    const double w_end = a.endpen ? a.endpen[(size_t)vid * cm + c_last] : 0.0;
    const double best = s_gam + w_end;
    const bool bad = s_flag[1] != 0 || align_bad_bits(best);
    const bool none = !bad && align_nonfinite_bits(best);     // -inf: the tables leave no alignment
    if (!bad && !none && tid < 64) {
        int n = T;
        double w = w_end;
        bool fail = false;
        for (int m = M - 1; m >= 0; --m) {
            const int c = s_a[m];
            int lo = 0, hi = 0;
            if (m > 0) align_range(m - 1, M, T, kw, lo, hi);
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
                const double v = (cn + (hm[n - k] + len[(size_t)k * cm + c])) + w;
                if (v == mx && k < kb) kb = k;
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
    const bool empty = failed || none;

    // ---- outputs: the segment of position q is the last one that starts at or before it
    const int64_t eos = cmap ? cmap[C] : (int64_t)C;
    const int q_end = a.t_max > T - 1 ? a.t_max : T - 1;
    for (int q = tid; q <= q_end; q += SMM_ALIGN_THREADS) {
        int64_t sp = -1, lb = -1;
        if (!empty && q < T) {
            int l = 0, r = M - 1;                              // s_start[0] = 0 <= q
            while (l < r) {
                const int mid = (l + r + 1) >> 1;
                if (s_start[mid] <= q) l = mid; else r = mid - 1;
            }
            const int id = s_a[l];
            lb = cmap ? cmap[id] : (int64_t)id;
            if (s_start[l] == q) sp = lb;
        } else if (!empty && q == T) {
            sp = eos;
        }
        if (spans && q <= a.t_max) spans[q] = sp;
        if (labels && q < T) labels[q] = lb;
    }
    if (tid == 0) {
        if (failed) a.err[0] = 1;
        if (a.best) a.best[vid] = failed ? __builtin_nan("") : best;
        if (a.n_segs) a.n_segs[vid] = empty ? 0 : M;
    }
}

void smm_launch_align(const SmmAlignArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}
