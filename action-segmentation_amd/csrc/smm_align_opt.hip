// smm_align_opt.hip -- forced alignment to a transcript whose entries may be optional: the best segmentation whose class
// sequence is the transcript a[0..M-1] with any subset of the optional entries left out (include/smmdp.h: smm_align_opt_f64).
//
//   pred(m)   = the entries that may directly precede entry m: m-1, m-2, ... down to and including the nearest mandatory one
//   first(m)  = every entry before m is optional;  end(j) = every entry after j is optional
//   h[0][m]   = init[a_m] if first(m), else -inf
//   h[n][m]   = max_{j in pred(m)} ( gam[n][j] + trans[a_m][a_j] ) - cum[n][a_m]        (0 < n < T)
//   gam[n][m] = cum[n][a_m] + max_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )
//   best      = max_{j : end(j)} ( gam[T][j] + closing_j )
// Every add is one IEEE fp64 add in this association (max is exact): the twin's Viterbi on the lattice whose states are the
// transcript positions, with trans'[m][j] = trans[a_m][a_j] for j in pred(m).
//
// smm_align_opt_kernel: one workgroup per video, smm_align_kernel's phases (smm_align.hip) and its span loop; what differs:
//   - the cells of column m that lie on a complete alignment count the mandatory entries before (nb) and after (na) it:
//       max(nb + 1, T - (M-1-m)(kp-1)) <= n <= min(T - na, (m+1)(kp-1));
//     an optional entry has none when the mandatory ones fill the video;
//   - behind a mandatory entry the column writes h[.][m+1] straight from its gam, as smm_align_kernel does.  Behind an optional
//     entry h[.][m+1] is formed from G[c][n] = max{ gam[n][j] : j in pred(m+1), a_j = c }, a running maximum per class that
//     every column of a run updates and a mandatory entry resets: max_c ( G[c][n] + trans[a_m][c] ) - cum[n][a_m], at most
//     n_states terms however long the run (x -> x + t is monotone in fp64, so the maximum may be taken first).  G sits behind
//     the h columns, [C][T+1]; per class only the positions [glo, ghi] hold values (the hull of the cones that wrote it: both
//     bounds grow along a run; a gap between two cones is filled with -inf by the column that opens it);
//   - gam[T][j] is kept for every end(j);
//   - the back-trace (wave 0) decides over the pairs (k, j), j among the candidates (first the end(j), then pred of the entry
//     just placed): the smallest k, then the smallest j, whose value equals the maximum.  It records start and entry of every
//     segment from the top of two LDS arrays down; the output phase bisects over the recorded starts and writes `used`.
// No atomics, no private segment; every output word has one writer.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3                                            // positions per thread (odd: smm_align_tile.h)
#include "smm_align_tile.h"
#include "smm_launch.h"

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_opt_kernel(SmmAlignArgs a)
{
    __shared__ double s_h[SMM_ALIGN_HS];
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ double s_gamT[SMM_MAX_TRANSCRIPT];              // gam[T][j] (-inf where (T, j) is no cell)
    __shared__ double s_tr[SMM_MAX_STATES_DEV];                // trans[a_m][s_act[i]]
    __shared__ double s_best;
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_opt[SMM_MAX_TRANSCRIPT];
    __shared__ int s_nb[SMM_MAX_TRANSCRIPT + 1];               // mandatory entries before m; [M]: all of them
    __shared__ int s_plo[SMM_MAX_TRANSCRIPT + 1];              // the first entry of pred(m); [M]: of the entries that may end
    __shared__ int s_slo[SMM_MAX_TRANSCRIPT], s_shi[SMM_MAX_TRANSCRIPT];   // the positions > 0 that hold column m's sources
    __shared__ int s_start[SMM_MAX_TRANSCRIPT], s_entry[SMM_MAX_TRANSCRIPT];   // the segments, filled from the top down
    __shared__ int s_used[SMM_MAX_TRANSCRIPT];
    __shared__ int s_glo[SMM_MAX_STATES_DEV], s_ghi[SMM_MAX_STATES_DEV], s_act[SMM_MAX_STATES_DEV];
    __shared__ int s_nact, s_first_seg;
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
    const double *endpen = a.endpen ? a.endpen + (size_t)vid * cm : nullptr;
    const int64_t *cmap = a.class_map ? a.class_map + (size_t)g * (cm + 1) : nullptr;
    const size_t T1 = (size_t)T + 1;
    double *cum = a.hist + mv.hist_off;                        // [C][T+1]
    double *hcol = a.hcols + a.hoff[vid];                      // [M][T+1]
    double *G = hcol + (size_t)M * T1;                         // [C][T+1]
    int64_t *spans = a.spans ? a.spans + (size_t)vid * (a.t_max + 1) : nullptr;
    int64_t *labels = a.labels ? a.labels + mv.frame_off : nullptr;
    int32_t *used = a.used ? a.used + t0 : nullptr;

    if (tid < 2) s_flag[tid] = 0;
    if (tid < SMM_MAX_STATES_DEV) { s_glo[tid] = 1; s_ghi[tid] = 0; }
    if (tid == 0) s_nact = 0;
    __syncthreads();
    for (int m = tid; m < M; m += SMM_ALIGN_THREADS) {
        const int id = a.transcript[t0 + m];
        const bool ok = id >= 0 && id < C;
        s_a[m] = ok ? id : 0;                                  // (never used as an index when the flag is up)
        s_opt[m] = a.optional[t0 + m] != 0;
        s_gamT[m] = SMM_NEG_INF;
        s_used[m] = 0;
        if (!ok) s_flag[0] = 1;
    }
    __syncthreads();
    if (tid == 0) {
        int nb = 0, head = 0;
        for (int m = 0; m < M; ++m) {
            s_nb[m] = nb;
            s_plo[m] = head;
            if (!s_opt[m]) { ++nb; head = m; }
        }
        s_nb[M] = nb;
        s_plo[M] = head;
    }
    __syncthreads();
    const int mand = s_nb[M];
    // no alignment by counting (the mandatory entries need a frame each; M segments of at most kp - 1 frames), or an id that is
    // no state of this video
    if (s_flag[0] || mand > T || kw < 1 || (int64_t)M * kw < T) {
        if (spans)
            for (int q = tid; q <= a.t_max; q += SMM_ALIGN_THREADS) spans[q] = -1;
        if (labels)
            for (int f = tid; f < T; f += SMM_ALIGN_THREADS) labels[f] = -1;
        if (used && tid < M) used[tid] = 0;
        if (tid == 0) {
            if (a.best) a.best[vid] = SMM_NEG_INF;
            if (a.n_segs) a.n_segs[vid] = 0;
        }
        return;
    }

    // ---- the tables this transcript reads: a NaN or +inf among them reaches the DP
    if (tid < M) {
        const int c = s_a[tid];
        bool bad = false;
        if (s_nb[tid] == 0) {                                  // first(m)
            const double v = a.init[(size_t)g * cm + c];
            hcol[(size_t)tid * T1] = v;
            bad |= align_bad_bits(v);
        }
        for (int j = s_plo[tid]; j < tid; ++j) bad |= align_bad_bits(trans[(size_t)c * cm + s_a[j]]);
        if (endpen && tid >= s_plo[M]) bad |= align_bad_bits(endpen[c]);   // end(m)
        if (bad) s_flag[1] = 1;
    }

    // ---- prefix sums (smm_align_tile.h): tiles of frames through LDS, lane c adds class c serially, cum[c][n] class-major
    if (align_prefix_sums(elp, cum, C, cm, T, s_h, tid)) s_flag[1] = 1;
    __threadfence_block();
    __syncthreads();

    // ---- columns
    int ulo = 1, uhi = 0;                                      // the hull of the cones of pred(m): column m's sources besides 0
    const int d_all = (kw + 1 + SMM_ALIGN_R - 1) / SMM_ALIGN_R * SMM_ALIGN_R;   // distances -R .. d_all - 1 cover k = 1 .. kw
    for (int m = 0; m < M; ++m) {
        const int c = s_a[m];
        const bool optm = s_opt[m] != 0, has_next = m + 1 < M, first = s_nb[m] == 0;
        const int na = mand - s_nb[m] - (optm ? 0 : 1);
        const bool direct = !optm && has_next;                 // pred(m + 1) = {m}: h[.][m+1] straight from this column's gam
        const bool to_g = has_next && (optm || s_opt[m + 1] != 0);   // a later column reads this one through G
        const int cn = has_next ? s_a[m + 1] : c;
        const double tr = direct ? trans[(size_t)cn * cm + c] : 0.0;
        double *hm = hcol + (size_t)m * T1;
        const double *cumc = cum + (size_t)c * T1, *cumn = cum + (size_t)cn * T1;
        double *hn = hcol + (size_t)(m + 1) * T1;              // (written under `direct` only)
        double *gc = G + (size_t)c * T1;
        int lo, hi;
        align_opt_range(m, M, T, kw, s_nb[m], na, lo, hi);
        __syncthreads();                                       // the previous column's readers of s_len, s_h; its update of G's ranges
        const int nact = s_nact;
        // G[c] as this column finds it: emptied by a mandatory entry, which starts the next run
        const int glo = optm ? s_glo[c] : 1, ghi = optm ? s_ghi[c] : 0;
        if (tid == 0) { s_slo[m] = ulo; s_shi[m] = uhi; }
        if (lo > hi || (!first && ulo > uhi)) continue;        // an optional entry the mandatory ones leave no frame for
        for (int j = tid; j < d_all + 3 * SMM_ALIGN_R; j += SMM_ALIGN_THREADS) {
            const int k = j - SMM_ALIGN_R;
            double v = SMM_NEG_INF;
            if (k >= 1 && k <= kw) {
                v = len[(size_t)k * cm + c];
                if (align_bad_bits(v)) s_flag[1] = 1;
            }
            s_len[j] = v;
        }
        if (m > 0 && s_opt[m - 1] && ulo <= uhi) {
            // ---- h[.][m] from the running maxima of the run before it
            if (tid < nact) s_tr[tid] = trans[(size_t)c * cm + s_act[tid]];
            __syncthreads();
            for (int n = ulo + tid; n <= uhi; n += SMM_ALIGN_THREADS) {
                double v = SMM_NEG_INF;
                for (int i = 0; i < nact; ++i) {
                    const int cc = s_act[i];
                    if (n >= s_glo[cc] && n <= s_ghi[cc]) v = align_max(v, G[(size_t)cc * T1 + n] + s_tr[i]);
                }
                hm[n] = v - cumc[n];
            }
            __threadfence_block();
        }
        const int s_lo = ulo <= uhi ? ulo : 0, s_hi = ulo <= uhi ? uhi : 0;
        for (int tb = lo; tb <= hi; tb += SMM_ALIGN_P) {
            // distances that can meet a source: tb - shi <= d <= tb + P - R - slo; whole steps of R, from -R (cell r at d has k = d + r)
            const int slo = first && tb <= kw ? 0 : s_lo;
            const int x = tb - s_hi, y = tb + SMM_ALIGN_P - SMM_ALIGN_R - slo + 1;
            const int d_first = x <= 0 ? -SMM_ALIGN_R : x / SMM_ALIGN_R * SMM_ALIGN_R;
            const int y_up = (y + SMM_ALIGN_R - 1) / SMM_ALIGN_R * SMM_ALIGN_R;
            const int d_end = y_up < d_all ? y_up : d_all;
            // LDS index i <-> position tb - OFF + i, for the positions tb - (d_end - 1) .. tb + P - R - d_first
            const int i_first = SMM_ALIGN_OFF - (d_end - 1), i_last = SMM_ALIGN_OFF + SMM_ALIGN_P - SMM_ALIGN_R - d_first;
            __syncthreads();                                   // the previous tile's readers; h[.][m] formed above
            if (d_first < d_end)
                for (int i = i_first + tid; i <= i_last; i += SMM_ALIGN_THREADS) {
                    const int s = tb - SMM_ALIGN_OFF + i;
                    s_h[i] = ((s >= ulo && s <= uhi) || (first && s == 0)) ? hm[s] : SMM_NEG_INF;
                }
            __syncthreads();
            const int n0 = tb + tid * SMM_ALIGN_R;
            if (n0 <= hi) {
                double acc[SMM_ALIGN_R], lw[SMM_ALIGN_R];
#pragma unroll
                for (int r = 0; r < SMM_ALIGN_R; ++r) acc[r] = SMM_NEG_INF;
                if (d_first < d_end) {                         // (else no source is in reach of this tile: its cells are -inf)
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
                }
#pragma unroll
                for (int r = 0; r < SMM_ALIGN_R; ++r) {
                    const int n = n0 + r;
                    if (n <= hi) {
                        const double gam = cumc[n] + acc[r];
                        if (n == T) s_gamT[m] = gam;           // (read for end(m) only)
                        if (direct) hn[n] = (gam + tr) - cumn[n];
                        if (to_g) gc[n] = (n >= glo && n <= ghi) ? align_max(gc[n], gam) : gam;
                    }
                }
            }
        }
        if (to_g) {
            // the positions between this class's last cone and this one hold no cell
            if (glo <= ghi)
                for (int n = ghi + 1 + tid; n < lo; n += SMM_ALIGN_THREADS) gc[n] = SMM_NEG_INF;
            __syncthreads();                                   // every reader of G's ranges in this column
            if (tid == 0) {
                int na2 = nact;
                if (!optm) {
                    for (int i = 0; i < nact; ++i) { s_glo[s_act[i]] = 1; s_ghi[s_act[i]] = 0; }
                    na2 = 0;
                }
                if (glo > ghi) { s_act[na2++] = c; s_glo[c] = lo; }
                s_ghi[c] = hi;
                s_nact = na2;
            }
        }
        if (!optm || ulo > uhi) ulo = lo;
        uhi = hi;
        __threadfence_block();
    }
    __syncthreads();

    // ---- closing step and back-trace (wave 0)
    bool none = false;
    if (tid < 64) {
        double best = SMM_NEG_INF;
        for (int j = s_plo[M] + tid; j < M; j += 64) best = align_max(best, s_gamT[j] + (endpen ? endpen[s_a[j]] : 0.0));
        best = align_wave_max(best);
        if (tid == 0) s_best = best;
        const bool bad = s_flag[1] != 0 || align_bad_bits(best);
        none = !bad && align_nonfinite_bits(best);             // -inf: the tables leave no alignment
        if (!bad && !none) {
            int n = T, cur = M, idx = M;
            bool fail = false;
            while (n > 0) {
                // candidates: pred(cur) (cur = M: the entries that may end), each with every length
                const int p_lo = s_plo[cur], kmax = kw < n ? kw : n;
                const int total = (cur - p_lo) * kmax;
                const double *trow = trans + (size_t)(cur < M ? s_a[cur] : 0) * cm;
                double mx = SMM_NEG_INF;
                int key = 0x7fffffff;                          // k * SMM_MAX_TRANSCRIPT + j: the smallest k, then the smallest j
                for (int e = tid; e < total; e += 64) {
                    const int ci = e / kmax, k = 1 + (e - ci * kmax), i = p_lo + ci, s = n - k;
                    const int nbi = s_nb[i];
                    int lo, hi;
                    align_opt_range(i, M, T, kw, nbi, mand - nbi - (s_opt[i] ? 0 : 1), lo, hi);
                    if (n < lo || n > hi) continue;
                    if (s == 0 ? nbi != 0 : (s < s_slo[i] || s > s_shi[i])) continue;
                    const int c = s_a[i];
                    const double w = cur < M ? trow[c] : (endpen ? endpen[c] : 0.0);
                    const double v = (cum[(size_t)c * T1 + n] + (hcol[(size_t)i * T1 + s] + len[(size_t)k * cm + c])) + w;
                    const int kk = k * SMM_MAX_TRANSCRIPT + i;
                    if (v > mx || (v == mx && kk < key)) { mx = v; key = kk; }
                }
                const double top = align_wave_max(mx);
                key = align_wave_min(mx == top ? key : 0x7fffffff);
                if (key == 0x7fffffff || align_nonfinite_bits(top)) { fail = true; break; }
                cur = key % SMM_MAX_TRANSCRIPT;
                n -= key / SMM_MAX_TRANSCRIPT;
                --idx;
                if (tid == 0) { s_start[idx] = n; s_entry[idx] = cur; s_used[cur] = 1; }
            }
            if (tid == 0) {
                s_first_seg = idx;
                if (fail) s_flag[1] = 1;
            }
        }
    }
    __syncthreads();
    const double best = s_best;
    const bool failed = s_flag[1] != 0 || align_bad_bits(best);
    const bool empty = failed || align_nonfinite_bits(best);

    // ---- outputs: the segment of position q is the last one that starts at or before it
    const int seg0 = empty ? M : s_first_seg;
    const int64_t eos = cmap ? cmap[C] : (int64_t)C;
    const int q_end = a.t_max > T - 1 ? a.t_max : T - 1;
    for (int q = tid; q <= q_end; q += SMM_ALIGN_THREADS) {
        int64_t sp = -1, lb = -1;
        if (!empty && q < T) {
            int l = seg0, r = M - 1;                           // s_start[seg0] = 0 <= q
            while (l < r) {
                const int mid = (l + r + 1) >> 1;
                if (s_start[mid] <= q) l = mid; else r = mid - 1;
            }
            const int id = s_a[s_entry[l]];
            lb = cmap ? cmap[id] : (int64_t)id;
            if (s_start[l] == q) sp = lb;
        } else if (!empty && q == T) {
            sp = eos;
        }
        if (spans && q <= a.t_max) spans[q] = sp;
        if (labels && q < T) labels[q] = lb;
    }
    if (used && tid < M) used[tid] = empty ? 0 : s_used[tid];
    if (tid == 0) {
        if (failed) a.err[0] = 1;
        if (a.best) a.best[vid] = failed ? __builtin_nan("") : best;
        if (a.n_segs) a.n_segs[vid] = empty ? 0 : M - seg0;
    }
}

void smm_launch_align_opt(const SmmAlignArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_opt_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}
