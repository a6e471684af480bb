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
// smm_align_opt_kernel: one workgroup per video, smm_align_kernel's phases (smm_align.hip) and its span loop, both from
// smm_align_tile.h; what differs:
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
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const double *trans = v.trans, *len = v.len, *endpen = v.endpen, *cum = v.cum;
    const size_t T1 = v.T1;
    double *hcol = a.hcols + a.hoff[vid];                      // [M][T+1]
    double *G = hcol + (size_t)M * T1;                         // [C][T+1]
    int32_t *used = a.used ? a.used + v.t0 : nullptr;

    if (tid < 2) s_flag[tid] = 0;
    if (tid < SMM_MAX_STATES_DEV) { s_glo[tid] = 1; s_ghi[tid] = 0; }
    if (tid == 0) s_nact = 0;
    for (int m = tid; m < M; m += SMM_ALIGN_THREADS) {
        s_gamT[m] = SMM_NEG_INF;
        s_used[m] = 0;
    }
    __syncthreads();
    const bool ids_ok = align_load_opt(a, v, s_a, s_opt, s_nb, s_plo, s_flag, tid, SMM_ALIGN_THREADS);
    const int mand = s_nb[M];
    // no alignment by counting (the mandatory entries need a frame each; M segments of at most kp - 1 frames), or an id that is
    // no state of this video
    if (!ids_ok || mand > T || kw < 1 || (int64_t)M * kw < T) {
        align_write_none(a, v, vid, tid);
        if (used && tid < M) used[tid] = 0;
        return;
    }

    if (align_opt_tables_bad(v, s_a, s_nb, s_plo, tid)) s_flag[1] = 1;
    if (tid < M && s_nb[tid] == 0) hcol[(size_t)tid * T1] = v.init[s_a[tid]];   // first(m)
    // ---- prefix sums (smm_align_tile.h): tiles of frames through LDS, lane c adds class c serially, cum[c][n] class-major
    if (align_prefix_sums(v.elp, v.cum, v.C, cm, T, s_h, tid)) s_flag[1] = 1;
    __threadfence_block();
    __syncthreads();

    // ---- columns
    int ulo = 1, uhi = 0;                                      // the hull of the cones of pred(m): column m's sources besides 0
    const int d_all = align_d_all(kw);
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
        if (align_stage_len(len, cm, c, kw, d_all, s_len, tid)) s_flag[1] = 1;
        if (m > 0 && s_opt[m - 1] && ulo <= uhi) {
            // ---- h[.][m] from the running maxima of the run before it
            if (tid < nact) s_tr[tid] = trans[(size_t)c * cm + s_act[tid]];
            __syncthreads();
            for (int n = ulo + tid; n <= uhi; n += SMM_ALIGN_THREADS)
                hm[n] = align_class_max(G, T1, n, nact, s_act, s_glo, s_ghi, s_tr) - cumc[n];
            __threadfence_block();
        }
        align_tiles(lo, hi, first ? 0 : ulo, ulo <= uhi ? uhi : 0, d_all, s_h, tid,
                    [&](int s) { return ((s >= ulo && s <= uhi) || (first && s == 0)) ? hm[s] : SMM_NEG_INF; },
                    [&](int n0, int d_first, int d_end, const double *hp) {
                        double acc[SMM_ALIGN_R];
                        // (d_first >= d_end: no source is in reach of this tile, its cells are -inf)
                        align_sweep_max(d_first < d_end ? d_first : d_end, d_end, hp, s_len, acc);
#pragma unroll
                        for (int r = 0; r < SMM_ALIGN_R; ++r) {
                            const int n = n0 + r;
                            if (n <= hi) {
                                const double gam = cumc[n] + acc[r];
                                if (n == T) s_gamT[m] = gam;   // (read for end(m) only)
                                if (direct) hn[n] = (gam + tr) - cumn[n];
                                if (to_g) gc[n] = (n >= glo && n <= ghi) ? align_max(gc[n], gam) : gam;
                            }
                        }
                    });
        if (to_g) {
            // the positions between this class's last cone and this one hold no cell
            if (glo <= ghi)
                for (int n = ghi + 1 + tid; n < lo; n += SMM_ALIGN_THREADS) gc[n] = SMM_NEG_INF;
            __syncthreads();                                   // every reader of G's ranges in this column
            if (tid == 0) align_hull(s_glo, s_ghi, s_act, &s_nact, !optm, c, lo, hi);
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
                    const double val = (cum[(size_t)c * T1 + n] + (hcol[(size_t)i * T1 + s] + len[(size_t)k * cm + c])) + w;
                    const int kk = k * SMM_MAX_TRANSCRIPT + i;
                    if (val > mx || (val == mx && kk < key)) { mx = val; key = kk; }
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

    // ---- outputs (smm_align_tile.h): the recorded segments carry the entries that got one
    const int seg0 = empty ? M : s_first_seg;
    align_write_result(a, v, vid, s_start, [&](int l) { return s_a[s_entry[l]]; }, seg0, failed, empty, best, tid);
    if (used && tid < M) used[tid] = empty ? 0 : s_used[tid];
}

void smm_launch_align_opt(const SmmAlignArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_opt_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}
