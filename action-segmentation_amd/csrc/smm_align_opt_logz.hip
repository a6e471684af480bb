// smm_align_opt_logz.hip -- transcript likelihood with optional entries: the sum over every alignment of a video to the
// transcript a[0..M-1] with any subset of its optional entries left out, and the gradient of that sum (include/smmdp.h:
// smm_align_opt_logz_f64, smm_align_opt_logz_bwd_f64).  The log-semiring counterpart of smm_align_opt.hip.
//
//   pred(m), first(m), end(j), nb, na: smm_align_opt.hip's;  succ(j) = { m : j in pred(m) }: j+1, j+2, ... up to and including
//   the next mandatory entry
//   forward   h[0][m]   = init[a_m] if first(m), else -inf
//             h[n][m]   = lse_{j in pred(m)} ( gam[n][j] + trans[a_m][a_j] ) - cum[n][a_m]                      (0 < n < T)
//             gam[n][m] = cum[n][a_m] + lse_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )
//             logZ_o    = lse_{j : end(j)} ( gam[T][j] + closing_j )
//   backward  q[n][j]   = cum[n][a_j] + bg[n][j]                                                           (what is stored)
//             bg[T][j]  = closing_j if end(j), else -inf
//             bh[s][m]  = lse_{k=1..min(kp-1,T-s)} ( q[s+k][m] + len[k][a_m] )
//             bg[n][j]  = lse_{m in succ(j)} ( trans[a_m][a_j] - cum[n][a_m] + bh[n][m] )                        (0 < n < T)
//   S[s][m] = exp( h[s][m] + bh[s][m] - logZ_o )  entry m has a segment that starts at s
//   E[n][m] = exp( gam[n][m] + bg[n][m] - logZ_o )  ... that ends at n;   occ[t][m] = sum_{s<=t} S[s][m] - sum_{n<=t} E[n][m]
//
// Columns.  One workgroup per video; column m is smm_align_logz.hip's span loop (smm_align_lse.h) over the cells that lie on a
// complete alignment (align_opt_range).  Where pred(m) = {m-1} the column before writes h[.][m] straight from its gam, and where
// succ(m-1) = {m} column m writes q[.][m-1] straight from its bh: in smm_align_logz.hip's association, so a transcript without
// flags gives that unit's h and q columns bit for bit.  Elsewhere the columns go through a running log-sum per class:
//   forward   G[c][n] = lse{ gam[n][j] : j in pred(m), a_j = c },   h[n][m] = lse_c ( G[c][n] + trans[a_m][c] ) - cum[n][a_m]
//   backward  B[c][n] = lse{ bh[n][m] - cum[n][a_m] : m in succ(j), a_m = c },   bg[n][j] = lse_c ( B[c][n] + trans[c][a_j] )
// at most n_states terms per position however long the run; a mandatory entry empties the sums and then adds itself.  Both use
// the same [C][T+1] area behind the columns.  Per class only the hull [glo, ghi] of the cones that were added holds values; the
// positions between two cones are filled with -inf by the column that opens the gap, so the area needs no fill.  A running sum
// is kept as its fp64 logarithm: lse(a, b) = max + log1p(exp(min - max)), exact for any dynamic range.
//
// Gradients.  g_trans needs no loop over pairs: the posterior of "entry j is followed by an entry of class c" is
// sum_n exp( gam[n][j] + trans[c][a_j] + B[c][n] - logZ_o ), formed by the backward kernel while B holds succ(j); where
// succ(j) is one entry it is p_used[j] = sum_n E[n][j].  g_init adds S[0][m] of the entries that may come first.
// What the structure decides is not summed, as smm_align_logz.hip counts instead of summing posteriors (a sum of fp32-
// exponentiated terms is 1 only to ~1e-7): p_used of a mandatory entry is 1; where pred(m) = {m-1} and succ(m-1) = {m},
// S[.][m] is E[.][m-1]; the start posteriors S[0][m] are normalised by their own total lse_first( h[0][m] + bh[0][m] ), the
// backward pass's value of logZ_o (kept behind the video's parts), so they add up to 1.
//
// Kernels, one workgroup per video unless said otherwise; no atomics, no private segment, every sum in a fixed order:
//   smm_align_opt_logz_fwd_kernel     prefix sums, the h and gam columns, the columns' ranges, logZ_o
//   smm_align_opt_logz_bwd_kernel     the q and bh columns, p_used, the video's parts of g_trans and g_init
//   smm_align_opt_logz_occ_kernel     g_elp: per tile of frames one block scan of S - E per transcript entry
//   smm_align_opt_logz_glen_kernel    the video's part of g_len: thread k owns length k and walks the segment starts
//   smm_align_opt_logz_reduce_kernel  g_len, g_trans, g_init: the videos' parts of a group summed in video order
// A video without an alignment (logZ_o -inf) or with the error word set (NaN) is skipped by all of the backward kernels.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3                                            // positions per thread (odd: smm_align_tile.h)
#include "smm_align_tile.h"
#include "smm_align_lse.h"

#define SMM_AOL_OCC_THREADS 128
#define SMM_AOL_OCC_LD (SMM_MAX_STATES_DEV + 1)                 // doubles per frame row in LDS: odd, one row per thread
#define SMM_AOL_RNG 5                                            // ints per column: its cells [elo, ehi], its sources [ulo, uhi], z

// log( exp(a) + exp(b) ); -inf where both are
__device__ __forceinline__ double aol_add(double a, double b)
{
    const double hi = align_max(a, b), lo = __builtin_fmin(a, b);
    if (align_nonfinite_bits(hi)) return hi;
    return hi + log1p(exp(lo - hi));
}

// Add val(n), n in [lo, hi], to the running log-sum gc[.] of one class, whose values so far sit at [glo, ghi] (glo > ghi:
// none); the positions between the two ranges get -inf.  Every thread calls it; the caller updates the hull behind a barrier.
template <class Val>
__device__ __forceinline__ void aol_fold(double *gc, int glo, int ghi, int lo, int hi, int tid, Val val)
{
    for (int n = lo + tid; n <= hi; n += SMM_ALIGN_THREADS) {
        const double v = val(n);
        gc[n] = (n >= glo && n <= ghi) ? aol_add(gc[n], v) : v;
    }
    if (glo <= ghi) {
        for (int n = ghi + 1 + tid; n < lo; n += SMM_ALIGN_THREADS) gc[n] = SMM_NEG_INF;
        for (int n = hi + 1 + tid; n < glo; n += SMM_ALIGN_THREADS) gc[n] = SMM_NEG_INF;
    }
}

// lse_i ( G[act_i][n] + tr[i] ) over the classes whose hull holds n
__device__ __forceinline__ double aol_class_lse(const double *G, size_t T1, int n, int nact, const int *s_act, const int *s_glo,
                                                const int *s_ghi, const double *s_tr)
{
    const double mx = align_class_max(G, T1, n, nact, s_act, s_glo, s_ghi, s_tr);
    const double ref = align_nonfinite_bits(mx) ? 0.0 : mx;
    double sum = 0.0;
    for (int i = 0; i < nact; ++i) {
        const int cc = s_act[i];
        if (n >= s_glo[cc] && n <= s_ghi[cc]) sum = sum + exp((G[(size_t)cc * T1 + n] + s_tr[i]) - ref);
    }
    return ref + log(sum);
}

// the sum of x over the workgroup, in every thread: a butterfly per wave, the waves in order
__device__ __forceinline__ double aol_block_sum(double x, double *s_red, int tid)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off);
    __syncthreads();                                           // the readers of the sum before this one
    if ((tid & 63) == 0) s_red[tid >> 6] = x;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < SMM_ALIGN_THREADS / 64; ++w) s = s + s_red[w];
    return s;
}

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_opt_logz_fwd_kernel(SmmAlignLogzArgs a)
{
    __shared__ double s_h[SMM_ALIGN_HS];
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ double s_gamT[SMM_MAX_TRANSCRIPT];              // gam[T][j] (-inf where (T, j) is no cell)
    __shared__ double s_tr[SMM_MAX_STATES_DEV];                // trans[a_m][s_act[i]]
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_opt[SMM_MAX_TRANSCRIPT];
    __shared__ int s_nb[SMM_MAX_TRANSCRIPT + 1];
    __shared__ int s_plo[SMM_MAX_TRANSCRIPT + 1];
    __shared__ int s_glo[SMM_MAX_STATES_DEV], s_ghi[SMM_MAX_STATES_DEV], s_act[SMM_MAX_STATES_DEV];
    __shared__ int s_nact;
    __shared__ int s_flag[2];                                  // [0] an id out of range, [1] a NaN / +inf reached the DP

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const double *trans = v.trans, *len = v.len, *endpen = v.endpen, *cum = v.cum;
    const size_t T1 = v.T1;
    int *rng = reinterpret_cast<int *>(a.cols + a.hoff[vid]);  // [M][SMM_AOL_RNG], in 3 M doubles
    double *hcol = a.cols + a.hoff[vid] + 3 * (size_t)M;       // [M][T+1]
    double *gcol = hcol + (size_t)M * T1;                      // [M][T+1]
    double *G = hcol + 4 * (size_t)M * T1;                     // [C][T+1], behind h | gam | q | bh

    if (tid < 2) s_flag[tid] = 0;
    if (tid < SMM_MAX_STATES_DEV) { s_glo[tid] = 1; s_ghi[tid] = 0; }
    if (tid == 0) s_nact = 0;
    for (int m = tid; m < M; m += SMM_ALIGN_THREADS) s_gamT[m] = SMM_NEG_INF;
    __syncthreads();
    const bool ids_ok = align_load_opt(a, v, s_a, s_opt, s_nb, s_plo, s_flag, tid, SMM_ALIGN_THREADS);
    const int mand = s_nb[M];
    // no alignment by counting (the mandatory entries need a frame each; M segments of at most kp - 1 frames), or an id that is
    // no state of this video
    if (!ids_ok || mand > T || kw < 1 || (int64_t)M * kw < T) {
        if (tid == 0) a.logz[vid] = SMM_NEG_INF;
        return;
    }

    if (align_opt_tables_bad(v, s_a, s_nb, s_plo, tid)) s_flag[1] = 1;
    if (tid < M && s_nb[tid] == 0) hcol[(size_t)tid * T1] = v.init[s_a[tid]];   // first(m)
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
        double *hn = hcol + (size_t)(has_next ? m + 1 : m) * T1;   // (written under `direct` only)
        double *gm = gcol + (size_t)m * T1;
        int lo, hi;
        align_opt_range(m, M, T, kw, s_nb[m], na, lo, hi);
        __syncthreads();                                       // the previous column's readers of s_len, s_h; its update of G's hulls
        const int nact = s_nact;
        const int glo = optm ? s_glo[c] : 1, ghi = optm ? s_ghi[c] : 0;   // G[c] as this column finds it: a mandatory entry empties it
        const bool active = lo <= hi && (first || ulo <= uhi); // (else: an optional entry the mandatory ones leave no frame for)
        if (tid == 0) {
            int *r = rng + SMM_AOL_RNG * m;
            r[0] = active ? lo : 1;
            r[1] = active ? hi : 0;
            r[2] = active ? ulo : 1;
            r[3] = active ? uhi : 0;
            r[4] = active && first ? 1 : 0;
        }
        if (!active) continue;
        if (align_stage_len(len, cm, c, kw, d_all, s_len, tid)) s_flag[1] = 1;
        if (m > 0 && s_opt[m - 1] && ulo <= uhi) {
            // ---- h[.][m] from the running sums of the run before it
            if (tid < nact) s_tr[tid] = trans[(size_t)c * cm + s_act[tid]];
            __syncthreads();
            for (int n = ulo + tid; n <= uhi; n += SMM_ALIGN_THREADS)
                hm[n] = aol_class_lse(G, T1, n, nact, s_act, s_glo, s_ghi, s_tr) - cumc[n];
            __threadfence_block();
        }
        alogz_column(lo, hi, first ? 0 : ulo, ulo <= uhi ? uhi : 0, d_all, s_h, s_len, tid,
                     [&](int s) { return ((s >= ulo && s <= uhi) || (first && s == 0)) ? hm[s] : SMM_NEG_INF; },
                     [&](int n, double lse) {
                         const double gam = cumc[n] + lse;
                         gm[n] = gam;
                         if (n == T) s_gamT[m] = gam;          // (read for end(m) only)
                         if (direct) hn[n] = (gam + tr) - cumn[n];
                     });
        if (to_g) {
            __threadfence_block();
            __syncthreads();                                   // the column's gam; every reader of G's hulls in this column
            aol_fold(G + (size_t)c * T1, glo, ghi, lo, hi, tid, [&](int n) { return gm[n]; });
            if (tid == 0) align_hull(s_glo, s_ghi, s_act, &s_nact, !optm, c, lo, hi);
        }
        if (!optm || ulo > uhi) ulo = lo;
        uhi = hi;
        __threadfence_block();
    }
    __syncthreads();

    // ---- closing step: the entries that may end, in order
    if (tid == 0) {
        double mx = SMM_NEG_INF;
        for (int j = s_plo[M]; j < M; ++j) mx = align_max(mx, s_gamT[j] + (endpen ? endpen[s_a[j]] : 0.0));
        const double ref = align_nonfinite_bits(mx) ? 0.0 : mx;
        double sum = 0.0;
        for (int j = s_plo[M]; j < M; ++j) sum = sum + exp((s_gamT[j] + (endpen ? endpen[s_a[j]] : 0.0)) - ref);
        const double z = ref + log(sum);
        const bool bad = s_flag[1] != 0 || align_bad_bits(z);
        if (bad) a.err[0] = 1;
        a.logz[vid] = bad ? __builtin_nan("") : z;
    }
}

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_opt_logz_bwd_kernel(SmmAlignLogzArgs a)
{
    __shared__ double s_h[SMM_ALIGN_HS];
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ double s_tr[SMM_MAX_STATES_DEV];                // trans[s_act[i]][a_m]
    __shared__ double s_red[SMM_ALIGN_THREADS / 64];
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_opt[SMM_MAX_TRANSCRIPT];
    __shared__ int s_nb[SMM_MAX_TRANSCRIPT + 1];
    __shared__ int s_plo[SMM_MAX_TRANSCRIPT + 1];
    __shared__ int s_glo[SMM_MAX_STATES_DEV], s_ghi[SMM_MAX_STATES_DEV], s_act[SMM_MAX_STATES_DEV];
    __shared__ int s_nact;
    __shared__ int s_flag[2];

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const int64_t t0 = a.toff[vid];
    const int M = (int)(a.toff[vid + 1] - t0);
    const double lz = a.logz[vid];
    if (align_nonfinite_bits(lz)) {                            // no alignment, or the error word: nothing to differentiate
        if (tid == 0 && smm_nan_bits(lz)) a.err[0] = 1;        // (staging cleared the word the forward call had set)
        if (a.p_used)
            for (int m = tid; m < M; m += SMM_ALIGN_THREADS) a.p_used[t0 + m] = 0.0;
        return;
    }
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, kw = v.kw;
    const double *trans = v.trans, *len = v.len, *endpen = v.endpen;
    const size_t T1 = v.T1;
    const double *cum = v.cum;                                 // [C][T+1], the forward call's
    const int *rng = reinterpret_cast<const int *>(a.cols + a.hoff[vid]);
    const double *hcol = a.cols + a.hoff[vid] + 3 * (size_t)M;
    const double *gcol = hcol + (size_t)M * T1;
    double *qcol = a.cols + a.hoff[vid] + 3 * (size_t)M + 2 * (size_t)M * T1;   // [M][T+1]
    double *bhcol = qcol + (size_t)M * T1;                     // [M][T+1]
    double *B = bhcol + (size_t)M * T1;                        // [C][T+1]: the forward kernel's G area
    const int rows = a.k_rows < T + 1 ? a.k_rows : T + 1;
    double *tpart = a.part + a.poff[vid] + (size_t)rows * cm;  // [c_max][c_max], then [c_max], then the backward pass's logZ_o
    double *ipart = tpart + (size_t)cm * cm;
    double *p_used = a.p_used ? a.p_used + t0 : nullptr;

    if (tid < 2) s_flag[tid] = 0;
    if (tid < SMM_MAX_STATES_DEV) { s_glo[tid] = 1; s_ghi[tid] = 0; }
    if (tid == 0) s_nact = 0;
    for (int e = tid; e < cm * cm + cm; e += SMM_ALIGN_THREADS) tpart[e] = 0.0;
    __syncthreads();
    if (!align_load_opt(a, v, s_a, s_opt, s_nb, s_plo, s_flag, tid, SMM_ALIGN_THREADS)) return;   // (a finite logZ_o had valid ids)
    __threadfence_block();
    __syncthreads();

    // ---- columns M - 1 .. 0 in the walk coordinate p = T - n: the targets are the starts of entry m, the sources its ends
    const int d_all = align_d_all(kw);
    for (int m = M - 1; m >= 0; --m) {
        const int *r = rng + SMM_AOL_RNG * m;
        const int elo = r[0], ehi = r[1], ulo = r[2], uhi = r[3], z = r[4];
        const int c = s_a[m];
        const bool optm = s_opt[m] != 0;
        __syncthreads();                                       // the previous column's readers of s_len, s_h; its update of B's hulls
        if (elo > ehi) {                                       // an entry without a cell
            if (tid == 0 && p_used) p_used[m] = 0.0;
            continue;
        }
        const bool endm = m >= s_plo[M];
        const bool q_direct = m + 1 < M && !s_opt[m + 1] && s_plo[m + 1] == m;   // succ(m) = {m+1}: column m + 1 wrote q[.][m]
        const bool p_direct = m > 0 && !optm && s_plo[m] == m - 1;               // pred(m) = {m-1} and succ(m-1) = {m}
        const int cp = m > 0 ? s_a[m - 1] : c;
        const double tr = p_direct ? trans[(size_t)c * cm + cp] : 0.0;
        const double *hm = hcol + (size_t)m * T1, *gm = gcol + (size_t)m * T1;
        const double *cumc = cum + (size_t)c * T1, *cump = cum + (size_t)cp * T1;
        double *qm = qcol + (size_t)m * T1, *bhm = bhcol + (size_t)m * T1;
        double *qp = qcol + (size_t)(m > 0 ? m - 1 : 0) * T1;  // (written under `p_direct` only)
        const int nact = s_nact;
        if (!q_direct) {
            // ---- q[.][m] from the running sums over succ(m), and what entry m hands to each class behind it
            if (tid < nact) s_tr[tid] = trans[(size_t)s_act[tid] * cm + c];
            __syncthreads();
            for (int n = elo + tid; n <= ehi; n += SMM_ALIGN_THREADS) {
                double bg;
                if (n == T) bg = endm ? (endpen ? endpen[c] : 0.0) : SMM_NEG_INF;
                else bg = aol_class_lse(B, T1, n, nact, s_act, s_glo, s_ghi, s_tr);
                qm[n] = cumc[n] + bg;
            }
            for (int i = 0; i < nact; ++i) {
                const int cc = s_act[i];
                const int l2 = elo > s_glo[cc] ? elo : s_glo[cc];
                int h2 = ehi < s_ghi[cc] ? ehi : s_ghi[cc];
                h2 = h2 < T - 1 ? h2 : T - 1;
                const double *bc = B + (size_t)cc * T1;
                double x = 0.0;
                for (int n = l2 + tid; n <= h2; n += SMM_ALIGN_THREADS) x = x + exp(((gm[n] + s_tr[i]) + bc[n]) - lz);
                const double tot = aol_block_sum(x, s_red, tid);
                if (tid == 0) tpart[(size_t)cc * cm + c] += tot;
            }
            __threadfence_block();
        }
        __syncthreads();
        // ---- p_used[m] = sum_n E[n][m]
        {
            double x = 0.0;
            if (optm)
                for (int n = elo + tid; n <= ehi; n += SMM_ALIGN_THREADS) x = x + exp((gm[n] + (qm[n] - cumc[n])) - lz);
            const double pu = optm ? aol_block_sum(x, s_red, tid) : 1.0;   // (a mandatory entry has a segment in every alignment)
            if (tid == 0) {
                if (p_used) p_used[m] = pu;
                if (q_direct) tpart[(size_t)s_a[m + 1] * cm + c] += pu;
            }
        }
        // ---- bh[.][m]
        const int smin = z ? 0 : ulo, smax = ulo <= uhi ? uhi : 0;
        align_stage_len(len, cm, c, kw, d_all, s_len, tid);
        alogz_column(T - smax, T - smin, T - ehi, T - elo, d_all, s_h, s_len, tid,
                     [&](int p) { return qm[T - p]; },
                     [&](int p, double bh) {
                         const int s = T - p;
                         if (s >= ulo && s <= uhi) {
                             bhm[s] = bh;
                             if (p_direct) qp[s] = cump[s] + ((tr - cumc[s]) + bh);
                         } else if (z && s == 0) {
                             bhm[0] = bh;
                         }
                     });
        __threadfence_block();
        __syncthreads();
        // ---- entry m joins the running sums that the entries before it read
        if (m > 0 && !p_direct) {
            const int glo = optm ? s_glo[c] : 1, ghi = optm ? s_ghi[c] : 0;
            if (ulo <= uhi) aol_fold(B + (size_t)c * T1, glo, ghi, ulo, uhi, tid, [&](int n) { return bhm[n] - cumc[n]; });
            __syncthreads();                                   // every reader of B's hulls in this column
            if (tid == 0) align_hull(s_glo, s_ghi, s_act, &s_nact, !optm, c, ulo, uhi);
        }
        __threadfence_block();
    }
    __syncthreads();

    // ---- the start posteriors, normalised by their own total: the entries that may come first, in order
    if (tid == 0) {
        double mx = SMM_NEG_INF;
        for (int m = 0; m < M && s_nb[m] == 0; ++m)
            if (rng[SMM_AOL_RNG * m + 4]) mx = align_max(mx, hcol[(size_t)m * T1] + bhcol[(size_t)m * T1]);
        const double ref = align_nonfinite_bits(mx) ? 0.0 : mx;
        double sum = 0.0;
        for (int m = 0; m < M && s_nb[m] == 0; ++m)
            if (rng[SMM_AOL_RNG * m + 4]) sum = sum + exp((hcol[(size_t)m * T1] + bhcol[(size_t)m * T1]) - ref);
        const double lzb = ref + log(sum);
        for (int m = 0; m < M && s_nb[m] == 0; ++m)
            if (rng[SMM_AOL_RNG * m + 4]) ipart[s_a[m]] += exp((hcol[(size_t)m * T1] + bhcol[(size_t)m * T1]) - lzb);
        ipart[cm] = lzb;
    }
}

// g_elp of one video.  Thread j of a tile owns frame t = f0 + j and an LDS row of class sums; per transcript entry one block scan
// of S[t][m] - E[t][m] over the tile on top of the entry's running total gives occ[t][m], which goes to the row's class a_m.
// Frames beside the video's and the rows of a skipped video keep the zeros of the call's zero fill.
__global__ void __launch_bounds__(SMM_AOL_OCC_THREADS) smm_align_opt_logz_occ_kernel(SmmAlignLogzArgs a)
{
    __shared__ double s_acc[SMM_AOL_OCC_THREADS * SMM_AOL_OCC_LD];
    __shared__ double s_carry[SMM_MAX_TRANSCRIPT];
    __shared__ double s_wave[2][SMM_AOL_OCC_THREADS / 64];
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_dir[SMM_MAX_TRANSCRIPT];                  // pred(m) = {m-1} and succ(m-1) = {m}: S[.][m] is E[.][m-1] (no flags: never)

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const double lz = a.logz[vid];
    if (align_nonfinite_bits(lz)) return;
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, C = v.C, M = v.M;
    const int64_t t0 = v.t0;
    const size_t T1 = v.T1;
    const double *cum = v.cum;
    const int *rng = reinterpret_cast<const int *>(a.cols + a.hoff[vid]);
    const double *hcol = a.cols + a.hoff[vid] + 3 * (size_t)M;
    const double *gcol = hcol + (size_t)M * T1;
    const double *qcol = gcol + (size_t)M * T1;
    const double *bhcol = qcol + (size_t)M * T1;
    const double u = a.grad ? a.grad[vid] : 1.0;
    double *g_elp = a.g_elp + (size_t)v.frame_off * cm;
    const int rows = a.k_rows < T + 1 ? a.k_rows : T + 1;
    const double lzb = a.part[a.poff[vid] + (size_t)rows * cm + (size_t)cm * cm + cm];   // the backward kernel's

    align_load_ids(a, v, s_a, tid, SMM_AOL_OCC_THREADS, [&](int m, bool) {   // (a finite logZ_o had valid ids)
        s_dir[m] = a.optional && m > 0 && a.optional[t0 + m] == 0 && (m == 1 || a.optional[t0 + m - 1] == 0);
        s_carry[m] = 0.0;
    });
    __syncthreads();

    double *row = s_acc + tid * SMM_AOL_OCC_LD;
    for (int f0 = 0; f0 < T; f0 += SMM_AOL_OCC_THREADS) {
        const int t = f0 + tid;
        for (int c = 0; c < C; ++c) row[c] = 0.0;
        for (int m = 0; m < M; ++m) {
            const int c = s_a[m];
            const int *r = rng + SMM_AOL_RNG * m;
            const int elo = r[0], ehi = r[1], ulo = r[2], uhi = r[3], z = r[4];
            // S[t][m] - E[t][m]: a segment ends at T behind every frame
            double e = 0.0;
            if (t < T) {
                const size_t i = (size_t)m * T1 + t;
                if (z && t == 0) {
                    e = exp((hcol[i] + bhcol[i]) - lzb);
                } else if (t >= ulo && t <= uhi) {
                    if (s_dir[m]) e = exp((gcol[i - T1] + (qcol[i - T1] - cum[(size_t)s_a[m - 1] * T1 + t])) - lz);
                    else e = exp((hcol[i] + bhcol[i]) - lz);
                }
                if (t >= elo && t <= ehi) e = e - exp((gcol[i] + (qcol[i] - cum[(size_t)c * T1 + t])) - lz);
            }
            // inclusive scan over the tile on top of the entry's running total
            const double p = align_block_scan(e, s_carry[m], s_wave[m & 1], tid);
            if (tid == SMM_AOL_OCC_THREADS - 1) s_carry[m] = p;
            row[c] = row[c] + p;
        }
        __syncthreads();
        const int nr = T - f0 < SMM_AOL_OCC_THREADS ? T - f0 : SMM_AOL_OCC_THREADS;
        align_store_rows(g_elp + (size_t)f0 * cm, s_acc, SMM_AOL_OCC_LD, nr, cm, C, u, tid, SMM_AOL_OCC_THREADS);
        __syncthreads();
    }
}

// The video's part of g_len, [rows][c_max] at part + poff[vid] with rows = min(k_rows, T + 1), without the factor u:
//   part[k][c] = sum_{m: a_m = c} sum_s exp( h[s][m] + len[k][c] + q[s+k][m] - logZ_o )
// Thread k owns row k (k = tid + 1, + THREADS, ...): the entries in order, the starts in order (0 first).
__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_opt_logz_glen_kernel(SmmAlignLogzArgs a)
{
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const double lz = a.logz[vid];
    if (align_nonfinite_bits(lz)) return;                      // (the reduction skips this video's part)
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, M = v.M;
    const int kw = v.kw < T ? v.kw : T;                        // (a segment is no longer than the video)
    const int rows = a.k_rows < T + 1 ? a.k_rows : T + 1;
    const double *len = v.len;
    const size_t T1 = v.T1;
    const int *rng = reinterpret_cast<const int *>(a.cols + a.hoff[vid]);
    const double *hcol = a.cols + a.hoff[vid] + 3 * (size_t)M;
    const double *qcol = hcol + 2 * (size_t)M * T1;
    double *part = a.part + a.poff[vid];

    align_load_ids(a, v, s_a, tid, SMM_ALIGN_THREADS, [](int, bool) {});   // (a finite logZ_o had valid ids)
    for (int e = tid; e < rows * cm; e += SMM_ALIGN_THREADS) part[e] = 0.0;
    __threadfence_block();
    __syncthreads();

    for (int k = tid + 1; k <= kw && k < rows; k += SMM_ALIGN_THREADS) {
        double *prow = part + (size_t)k * cm;
        for (int m = 0; m < M; ++m) {
            const int c = s_a[m];
            const int *r = rng + SMM_AOL_RNG * m;
            const int elo = r[0], ehi = r[1], ulo = r[2], uhi = r[3], z = r[4];
            if (elo > ehi) continue;
            const int s_first = ulo > elo - k ? ulo : elo - k, s_last = uhi < ehi - k ? uhi : ehi - k;
            const double base = len[(size_t)k * cm + c] - lz;
            const double *hm = hcol + (size_t)m * T1, *qm = qcol + (size_t)m * T1 + k;
            double acc = 0.0;
            if (z && k >= elo && k <= ehi) acc = acc + (double)__expf((float)((hm[0] + qm[0]) + base));
            for (int s = s_first; s <= s_last; ++s)
                acc = acc + (double)__expf((float)((hm[s] + qm[s]) + base));
            prow[c] = prow[c] + acc;
        }
    }
}

// g_len[g][k][c], g_trans[g][c][c'], g_init[g][c] = sum over the group's videos, in video order, of u_i * the video's part;
// rows a video does not have add nothing.  One thread per element: k_rows c_max of g_len, then c_max^2, then c_max.
__global__ void __launch_bounds__(256) smm_align_opt_logz_reduce_kernel(SmmAlignLogzArgs a)
{
    const int cm = a.c_max, g = blockIdx.y;
    const int n_len = a.k_rows * cm, n_tab = cm * cm + cm;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_len + n_tab) return;
    const int k = e / cm;
    double sum = 0.0;
    for (int i = 0; i < a.b; ++i) {
        const SmmVideo mv = a.videos[i];
        if (mv.group != g || align_nonfinite_bits(a.logz[i])) continue;
        const int rows = a.k_rows < mv.T + 1 ? a.k_rows : mv.T + 1;
        const double u = a.grad ? a.grad[i] : 1.0;
        if (e < n_len) {
            if (k < rows) sum = sum + u * a.part[a.poff[i] + e];
        } else {
            sum = sum + u * a.part[a.poff[i] + (size_t)rows * cm + (e - n_len)];
        }
    }
    if (e < n_len) a.g_len[(size_t)g * n_len + e] = sum;
    else if (e < n_len + cm * cm) a.g_trans[(size_t)g * cm * cm + (e - n_len)] = sum;
    else a.g_init[(size_t)g * cm + (e - n_len - cm * cm)] = sum;
}

void smm_launch_align_opt_logz_fwd(const SmmAlignLogzArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_opt_logz_fwd_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}

void smm_launch_align_opt_logz_bwd(const SmmAlignLogzArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_opt_logz_bwd_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
    smm_launch_align_opt_logz_tail(a, stream);
}

// g_elp, the videos' parts of g_len, the sums over the videos: from the columns, ranges and parts a backward kernel left
void smm_launch_align_opt_logz_tail(const SmmAlignLogzArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_opt_logz_occ_kernel, dim3((unsigned)a.b), dim3(SMM_AOL_OCC_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_align_opt_logz_glen_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
    const unsigned cells = (unsigned)(a.k_rows * a.c_max + a.c_max * a.c_max + a.c_max);
    hipLaunchKernelGGL(smm_align_opt_logz_reduce_kernel, dim3((cells + 255) / 256, (unsigned)a.n_groups), dim3(256), 0, stream, a);
}
