// smm_align_graph_logz.hip -- transcript-graph likelihood: the sum over every alignment of a video to every start -> end path
// of a transcript graph, its gradient and the node / end posteriors (include/smmdp.h: smm_align_graph_logz_f64,
// smm_align_graph_logz_bwd_f64).  The log-semiring counterpart of smm_align_graph.hip.
//
//   pred(m), start(m), end(j): smm_align_graph.hip's;  succ(j) = { m : j in pred(m) }
//   forward   h[0][m]   = init[a_m] if start(m), else -inf
//             h[n][m]   = lse_{j in pred(m)} ( gam[n][j] + trans[a_m][a_j] ) - cum[n][a_m]                      (0 < n < T)
//             gam[n][m] = cum[n][a_m] + lse_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )
//             logZ_g    = lse_{j : end(j)} ( gam[T][j] + closing_j )
//   backward  q[n][j]   = cum[n][a_j] + bg[n][j]                                                           (what is stored)
//             bg[T][j]  = closing_j if end(j), else -inf
//             bh[s][m]  = lse_{k=1..min(kp-1,T-s)} ( q[s+k][m] + len[k][a_m] )
//             bg[n][j]  = lse_{m in succ(j)} ( ( trans[a_m][a_j] - cum[n][a_m] ) + bh[n][m] )                    (0 < n < T)
//   S, E, occ: smm_align_opt_logz.hip's
//
// Forward kernel: smm_align_graph.hip's structure load, path-length walks, cell ranges and pull over the edges (all from
// smm_align_graph.h), with smm_align_logz.hip's two-sweep log-semiring cell (smm_align_lse.h) in place of the max-plus one.  The
// pull over the staged predecessor list is a max pass and a sum pass, SMM_GRAPH_U positions per thread in flight; the terms are
// exponentiated in fp64 (a column has few predecessors beside its kp - 1 span terms).  A single predecessor comes out as
// (gam + tr) - cum exactly: the maximum is the term, the sum exp(0) = 1, its logarithm 0.  Each column's cells [lo, hi], the
// positions > 0 that hold its h values [slo, shi] and whether it has an h[0] are recorded for the backward kernels in
// smm_align_opt_logz.hip's five ints per column.
//
// Backward kernel: the columns from M - 1 down to 0 in the walk coordinate p = T - n.  Column j needs succ(j): thread m > j tests
// bit j of its own mask and a ballot compacts the list (smm_align_graph.h: graph_compact), as the forward kernel lists
// predecessors; no transposed masks.  The successors are then put in (class, index) order -- each counts the listed nodes that
// come before it -- so that the edge posteriors of one successor class are a contiguous run: one block sum per (node,
// successor class), the waves in order, gives the video's part of g_trans.  The same column forms q[.][j] over the list from
// the bh columns kept in the workspace, p_used[j] and p_end[j], then bh[.][j] by the span loop.
//
// The workspace block of a video and its parts have smm_align_opt_logz.hip's layout without the per-class running sums, so
// the g_elp (occ), g_len and reduce kernels are that unit's own (smm_launch_align_opt_logz_tail): a graph has no entry whose
// start posterior is another's end posterior, which is what a null `optional` says to them.
//
// Static LDS, forward: s_h 14.1 KB, s_len 8.1 KB, the masks 8 KB, s_gamT and s_tr 4 KB, eleven int arrays of a node each 11 KB:
// 45.3 KB.  Backward: s_h, s_len, the masks, s_tr 2 KB, nine int arrays 9 KB: 41.3 KB.  Of the 64 KB a workgroup may declare.
// No atomics, no private segment, every sum in a fixed order.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3                                            // positions per thread (odd: smm_align_tile.h)
#include "smm_align_tile.h"
#include "smm_align_lse.h"
#include "smm_align_graph.h"

#define SMM_GRAPH_U 4                                            // positions per thread and round when h is formed

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_logz_fwd_kernel(SmmAlignLogzArgs a)
{
    __shared__ double s_h[SMM_ALIGN_HS];
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ double s_gamT[SMM_MAX_TRANSCRIPT];              // gam[T][j] (-inf where (T, j) is no cell)
    __shared__ double s_tr[SMM_MAX_TRANSCRIPT];                // trans[a_m][a_j], j = s_pl[i]
    __shared__ uint32_t s_mask[SMM_MAX_TRANSCRIPT * SMM_GRAPH_WORDS];
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_fl[SMM_MAX_TRANSCRIPT];                   // bit 0: start(m), bit 1: end(m)
    __shared__ int s_bmin[SMM_MAX_TRANSCRIPT], s_bmax[SMM_MAX_TRANSCRIPT];   // nodes before m on a path from a start node
    __shared__ int s_amin[SMM_MAX_TRANSCRIPT], s_amax[SMM_MAX_TRANSCRIPT];   // nodes after m on a path to an end node
    __shared__ int s_lo[SMM_MAX_TRANSCRIPT], s_hi[SMM_MAX_TRANSCRIPT];       // column m's cells (lo > hi: none)
    __shared__ int s_pl[SMM_MAX_TRANSCRIPT];                   // the predecessors of the column
    __shared__ int s_wcnt[4], s_wlo[4], s_whi[4];              // per wave: predecessors with cells, the hull of their cells
    __shared__ int s_len2[2];                                  // the fewest and most nodes on a start -> end path
    __shared__ int s_flag[2];                                  // [0] an id or a mask bit out of range, [1] a NaN / +inf reached the DP

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const double *trans = v.trans, *len = v.len, *endpen = v.endpen, *cum = v.cum;
    const size_t T1 = v.T1;
    int *rng = reinterpret_cast<int *>(a.cols + a.hoff[vid]);  // [M][SMM_GRAPH_RNG]: this kernel is their only writer
    const GraphCols<double> col = graph_cols(a.cols + a.hoff[vid], M, T1);
    double *hcol = col.h, *gcol = col.g;

    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    graph_load<true>(a, v, s_a, s_fl, s_mask, s_flag, tid);
    if (tid < M) s_gamT[tid] = SMM_NEG_INF;
    __syncthreads();
    if (s_flag[0] != 0 || kw < 1) {
        if (tid == 0) a.logz[vid] = SMM_NEG_INF;
        return;
    }
    if (tid < 64) graph_path_lengths(s_mask, s_fl, M, s_bmin, s_bmax, s_amin, s_amax, s_len2, tid);
    __syncthreads();
    graph_cells(M, T, kw, s_bmin, s_bmax, s_amin, s_amax, s_lo, s_hi, tid);
    if (graph_no_path(s_len2, T, kw)) {
        if (tid == 0) a.logz[vid] = SMM_NEG_INF;
        return;
    }

    if (graph_tables_bad(v, s_a, s_fl, s_mask, tid)) s_flag[1] = 1;
    if (tid < M && (s_fl[tid] & 1)) hcol[(size_t)tid * T1] = v.init[s_a[tid]];
    if (align_prefix_sums(v.elp, v.cum, v.C, cm, T, s_h, tid)) s_flag[1] = 1;
    __threadfence_block();
    __syncthreads();

    // ---- columns
    const int d_all = align_d_all(kw);
    for (int m = 0; m < M; ++m) {
        const int c = s_a[m];
        const bool first = (s_fl[m] & 1) != 0;
        const int lo = s_lo[m], hi = s_hi[m];
        double *hm = hcol + (size_t)m * T1, *gm = gcol + (size_t)m * T1;
        const double *cumc = cum + (size_t)c * T1;
        __syncthreads();                                       // the previous column's readers of s_len, s_h, s_pl, s_tr, s_w*
        if (lo > hi) {                                         // a node without cells: of its tables the length scores remain
            for (int k = 1 + tid; k <= kw; k += SMM_ALIGN_THREADS)
                if (align_bad_bits(len[(size_t)k * cm + c])) s_flag[1] = 1;
            if (tid == 0) {
                int *r = rng + SMM_GRAPH_RNG * m;
                r[0] = 1; r[1] = 0; r[2] = 1; r[3] = 0; r[4] = 0;
            }
            continue;
        }
        if (align_stage_len(len, cm, c, kw, d_all, s_len, tid)) s_flag[1] = 1;
        // ---- the predecessors that have cells -> s_pl, their transitions -> s_tr; the hull of their cells
        const bool is = tid < m && graph_edge(s_mask, m, tid) && s_lo[tid] <= s_hi[tid];
        int slot, np, ulo, uhi;
        graph_compact(is, is ? s_lo[tid] : 0, is ? s_hi[tid] : 0, s_wcnt, s_wlo, s_whi, tid, slot, np, ulo, uhi);
        if (is) {
            s_pl[slot] = tid;
            s_tr[slot] = trans[(size_t)c * cm + s_a[tid]];
        }
        // column m's sources besides 0: what its cells reach of that hull (slo > shi: none)
        int slo = ulo > lo - kw ? ulo : lo - kw, shi = uhi < hi - 1 ? uhi : hi - 1;
        if (np == 0 || slo > shi) { slo = 1; shi = 0; }
        if (tid == 0) {
            int *r = rng + SMM_GRAPH_RNG * m;
            r[0] = lo; r[1] = hi; r[2] = slo; r[3] = shi; r[4] = first ? 1 : 0;
        }
        __syncthreads();
        // ---- h[.][m] over the edges: the largest term, then the sum of exp(term - max)
        // (SMM_GRAPH_U positions per thread at a time: their loads are in flight together, the stores follow)
        for (int nb = slo + tid; nb <= shi; nb += SMM_GRAPH_U * SMM_ALIGN_THREADS) {
            double mx[SMM_GRAPH_U], sum[SMM_GRAPH_U], cu[SMM_GRAPH_U];
#pragma unroll
            for (int u = 0; u < SMM_GRAPH_U; ++u) {
                const int n = nb + u * SMM_ALIGN_THREADS;
                mx[u] = SMM_NEG_INF;
                sum[u] = 0.0;
                cu[u] = n <= shi ? cumc[n] : 0.0;
            }
            for (int i = 0; i < np; ++i) {
                const int j = s_pl[i], jl = s_lo[j], jh = s_hi[j];
                const double *gj = gcol + (size_t)j * T1;
                const double tr = s_tr[i];
                double g[SMM_GRAPH_U];
#pragma unroll
                for (int u = 0; u < SMM_GRAPH_U; ++u) {
                    const int n = nb + u * SMM_ALIGN_THREADS;
                    g[u] = (n <= shi && n >= jl && n <= jh) ? gj[n] : SMM_NEG_INF;   // (-inf + tr = -inf: no cell of j)
                }
#pragma unroll
                for (int u = 0; u < SMM_GRAPH_U; ++u) mx[u] = align_max(mx[u], g[u] + tr);
            }
#pragma unroll
            for (int u = 0; u < SMM_GRAPH_U; ++u) mx[u] = align_nonfinite_bits(mx[u]) ? 0.0 : mx[u];   // (no finite term: sums zeros)
            for (int i = 0; i < np; ++i) {
                const int j = s_pl[i], jl = s_lo[j], jh = s_hi[j];
                const double *gj = gcol + (size_t)j * T1;
                const double tr = s_tr[i];
                double g[SMM_GRAPH_U];
#pragma unroll
                for (int u = 0; u < SMM_GRAPH_U; ++u) {
                    const int n = nb + u * SMM_ALIGN_THREADS;
                    g[u] = (n <= shi && n >= jl && n <= jh) ? gj[n] : SMM_NEG_INF;
                }
#pragma unroll
                for (int u = 0; u < SMM_GRAPH_U; ++u) sum[u] = sum[u] + exp((g[u] + tr) - mx[u]);
            }
#pragma unroll
            for (int u = 0; u < SMM_GRAPH_U; ++u) {
                const int n = nb + u * SMM_ALIGN_THREADS;
                if (n <= shi) hm[n] = (mx[u] + log(sum[u])) - cu[u];
            }
        }
        __threadfence_block();
        alogz_column(lo, hi, first ? 0 : slo, shi, d_all, s_h, s_len, tid,
                     [&](int s) { return ((s >= slo && s <= shi) || (first && s == 0)) ? hm[s] : SMM_NEG_INF; },
                     [&](int n, double lse) {
                         const double gam = cumc[n] + lse;
                         gm[n] = gam;
                         if (n == T) s_gamT[m] = gam;          // (read for end(m) only)
                     });
        __threadfence_block();
    }
    __syncthreads();

    // ---- closing step: the end nodes, in index order
    if (tid == 0) {
        double mx = SMM_NEG_INF;
        for (int j = 0; j < M; ++j)
            if (s_fl[j] & 2) mx = align_max(mx, s_gamT[j] + (endpen ? endpen[s_a[j]] : 0.0));
        const double ref = align_nonfinite_bits(mx) ? 0.0 : mx;
        double sum = 0.0;
        for (int j = 0; j < M; ++j)
            if (s_fl[j] & 2) sum = sum + exp((s_gamT[j] + (endpen ? endpen[s_a[j]] : 0.0)) - ref);
        const double z = ref + log(sum);
        const bool bad = s_flag[1] != 0 || align_bad_bits(z);
        if (bad) a.err[0] = 1;
        a.logz[vid] = bad ? __builtin_nan("") : z;
    }
}

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_logz_bwd_kernel(SmmAlignLogzArgs a)
{
    __shared__ double s_h[SMM_ALIGN_HS];
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ double s_tr[SMM_MAX_TRANSCRIPT];                // trans[a_m][a_j], m = s_ps[i]
    __shared__ double s_red[SMM_ALIGN_THREADS / 64];
    __shared__ uint32_t s_mask[SMM_MAX_TRANSCRIPT * SMM_GRAPH_WORDS];
    __shared__ int s_ps[SMM_MAX_TRANSCRIPT];                   // the successors of the column in (class, index) order
    GRAPH_SHARED_NODES;                                        // (s_pl: ... in index order)

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const int64_t t0 = a.toff[vid];
    const int M = (int)(a.toff[vid + 1] - t0);
    const double lz = a.logz[vid];
    if (align_nonfinite_bits(lz)) {                            // no alignment, or the error word: nothing to differentiate
        if (tid == 0 && smm_nan_bits(lz)) a.err[0] = 1;        // (staging cleared the word the forward call had set)
        for (int m = tid; m < M; m += SMM_ALIGN_THREADS) {
            if (a.p_used) a.p_used[t0 + m] = 0.0;
            if (a.p_end) a.p_end[t0 + m] = 0.0;
        }
        return;
    }
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, kw = v.kw;
    const double *trans = v.trans, *len = v.len, *endpen = v.endpen;
    const size_t T1 = v.T1;
    const double *cum = v.cum;                                 // [C][T+1], the forward call's
    const GraphCols<double> col = graph_cols(a.cols + a.hoff[vid], M, T1);
    const double *hcol = col.h, *gcol = col.g;
    double *qcol = col.q, *bhcol = col.bh;                     // (written here)
    const int rows = a.k_rows < T + 1 ? a.k_rows : T + 1;
    double *tpart = a.part + a.poff[vid] + (size_t)rows * cm;  // [c_max][c_max], then [c_max], then the backward pass's logZ_g
    double *ipart = tpart + (size_t)cm * cm;
    double *p_used = a.p_used ? a.p_used + t0 : nullptr;
    double *p_end = a.p_end ? a.p_end + t0 : nullptr;

    if (tid < 2) s_flag[tid] = 0;
    for (int e = tid; e < cm * cm + cm; e += SMM_ALIGN_THREADS) tpart[e] = 0.0;
    __syncthreads();
    graph_load<true>(a, v, s_a, s_fl, s_mask, s_flag, tid);          // (a finite logZ_g had a valid structure)
    graph_load_ranges(graph_rng(a.cols + a.hoff[vid]), nd, M, tid);
    __threadfence_block();
    __syncthreads();
    if (s_flag[0] != 0) return;

    // ---- columns M - 1 .. 0 in the walk coordinate p = T - n: the targets are the starts of node m, the sources its ends
    const int d_all = align_d_all(kw);
    for (int m = M - 1; m >= 0; --m) {
        const int elo = s_lo[m], ehi = s_hi[m], slo = s_slo[m], shi = s_shi[m], z = s_z[m];
        const int c = s_a[m];
        __syncthreads();                                       // the previous column's readers of s_len, s_h, s_pl, s_ps, s_tr, s_w*
        if (elo > ehi) {                                       // a node without a cell
            if (tid == 0) {
                if (p_used) p_used[m] = 0.0;
                if (p_end) p_end[m] = 0.0;
            }
            continue;
        }
        const bool endm = (s_fl[m] & 2) != 0;
        const double *gm = gcol + (size_t)m * T1, *cumc = cum + (size_t)c * T1;
        double *qm = qcol + (size_t)m * T1, *bhm = bhcol + (size_t)m * T1;
        // ---- succ(m): the later nodes that name m in their own mask and hold bh values, first in index order ...
        bool is = false;
        const int np = graph_list<true>(s_mask, m, M, nd, tid, [&](int, int) { is = true; });
        __syncthreads();
        // ... then by class: a successor's place is the number of listed nodes of a smaller class, or of its class before it
        if (is) {
            const int mine = s_a[tid];
            int at = 0;
            for (int i = 0; i < np; ++i) {
                const int t = s_pl[i], ct = s_a[t];
                at += (ct < mine || (ct == mine && t < tid)) ? 1 : 0;
            }
            s_ps[at] = tid;
            s_tr[at] = trans[(size_t)mine * cm + c];
        }
        __syncthreads();
        // ---- q[.][m] over the edges
        for (int n = elo + tid; n <= ehi; n += SMM_ALIGN_THREADS) {
            double bg;
            if (n == T) {
                bg = endm ? (endpen ? endpen[c] : 0.0) : SMM_NEG_INF;
            } else {
                double mx = SMM_NEG_INF;
                for (int i = 0; i < np; ++i) {
                    const int t = s_ps[i];
                    if (n >= s_slo[t] && n <= s_shi[t])
                        mx = align_max(mx, (s_tr[i] - cum[(size_t)s_a[t] * T1 + n]) + bhcol[(size_t)t * T1 + n]);
                }
                const double ref = align_nonfinite_bits(mx) ? 0.0 : mx;
                double sum = 0.0;
                for (int i = 0; i < np; ++i) {
                    const int t = s_ps[i];
                    if (n >= s_slo[t] && n <= s_shi[t])
                        sum = sum + exp(((s_tr[i] - cum[(size_t)s_a[t] * T1 + n]) + bhcol[(size_t)t * T1 + n]) - ref);
                }
                bg = ref + log(sum);
            }
            qm[n] = cumc[n] + bg;
        }
        // ---- the video's part of g_trans: per successor class one block sum of the edge posteriors
        for (int i0 = 0; i0 < np;) {
            const int cc = s_a[s_ps[i0]];
            int i1 = i0 + 1;
            while (i1 < np && s_a[s_ps[i1]] == cc) ++i1;
            const double *cumn = cum + (size_t)cc * T1;
            const int last = ehi < T - 1 ? ehi : T - 1;
            double x = 0.0;
            for (int n = elo + tid; n <= last; n += SMM_ALIGN_THREADS) {
                const double g = gm[n], cu = cumn[n];
                for (int i = i0; i < i1; ++i) {
                    const int t = s_ps[i];
                    if (n >= s_slo[t] && n <= s_shi[t]) x = x + exp((g + ((s_tr[i] - cu) + bhcol[(size_t)t * T1 + n])) - lz);
                }
            }
            const double tot = graph_block_sum(x, s_red, tid);
            if (tid == 0) tpart[(size_t)cc * cm + c] += tot;
            i0 = i1;
        }
        __threadfence_block();
        __syncthreads();
        // ---- p_used[m] = sum_n E[n][m];  p_end[m] = E[T][m]  (asked for by the posterior calls, not by training)
        if (p_used || p_end) {
            double x = 0.0;
            for (int n = elo + tid; n <= ehi; n += SMM_ALIGN_THREADS) x = x + exp((gm[n] + (qm[n] - cumc[n])) - lz);
            const double pu = graph_block_sum(x, s_red, tid);
            if (tid == 0) {
                if (p_used) p_used[m] = pu;
                if (p_end) p_end[m] = (endm && ehi == T) ? exp((gm[T] + (qm[T] - cumc[T])) - lz) : 0.0;
            }
        }
        // ---- bh[.][m]
        const int smin = z ? 0 : slo, smax = slo <= shi ? shi : 0;
        align_stage_len(len, cm, c, kw, d_all, s_len, tid);
        alogz_column(T - smax, T - smin, T - ehi, T - elo, d_all, s_h, s_len, tid,
                     [&](int p) { return qm[T - p]; },
                     [&](int p, double bh) {
                         const int s = T - p;
                         if ((s >= slo && s <= shi) || (z && s == 0)) bhm[s] = bh;
                     });
        __threadfence_block();
    }
    __syncthreads();

    // ---- the start posteriors, normalised by their own total: the start nodes that have cells, in index order
    if (tid == 0) {
        double mx = SMM_NEG_INF;
        for (int m = 0; m < M; ++m)
            if (s_z[m]) mx = align_max(mx, hcol[(size_t)m * T1] + bhcol[(size_t)m * T1]);
        const double ref = align_nonfinite_bits(mx) ? 0.0 : mx;
        double sum = 0.0;
        for (int m = 0; m < M; ++m)
            if (s_z[m]) sum = sum + exp((hcol[(size_t)m * T1] + bhcol[(size_t)m * T1]) - ref);
        const double lzb = ref + log(sum);
        for (int m = 0; m < M; ++m)
            if (s_z[m]) ipart[s_a[m]] += exp((hcol[(size_t)m * T1] + bhcol[(size_t)m * T1]) - lzb);
        ipart[cm] = lzb;
    }
}

void smm_launch_align_graph_logz_fwd(const SmmAlignLogzArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_graph_logz_fwd_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}

void smm_launch_align_graph_logz_bwd_columns(const SmmAlignLogzArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_graph_logz_bwd_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}

void smm_launch_align_graph_logz_bwd(const SmmAlignLogzArgs &a, hipStream_t stream)
{
    smm_launch_align_graph_logz_bwd_columns(a, stream);
    smm_launch_align_opt_logz_tail(a, stream);                 // g_elp, the videos' parts of g_len, the sums over the videos
}
