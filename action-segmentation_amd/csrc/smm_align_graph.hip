// smm_align_graph.hip -- forced alignment to a transcript graph: the best segmentation whose class sequence is a start -> end
// path of a DAG whose nodes carry a class (include/smmdp.h: smm_align_graph_f64).  A plain transcript is a chain, an optional
// transcript a special DAG, a set of candidate transcripts their prefix trie.
//
//   pred(m)   = the nodes j < m whose bit is set in node m's mask (the numbering is topological)
//   h[0][m]   = init[a_m] if start(m), else -inf
//   h[n][m]   = max_{j in pred(m)} ( gam[n][j] + trans[a_m][a_j] ) - cum[n][a_m]        (0 < n < T; -inf for an empty pred(m))
//   gam[n][m] = cum[n][a_m] + max_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )
//   best      = max_{j : end(j)} ( gam[T][j] + closing_j )
// Every add is one IEEE fp64 add in this association (max is exact): the twin's Viterbi on the lattice whose states are the
// nodes, with trans'[m][j] = trans[a_m][a_j] for j in pred(m).
//
// smm_align_graph_kernel: one workgroup per video, smm_align_opt_kernel's phases (smm_align_opt.hip) and its span loop, both
// from smm_align_tile.h; what differs:
//   - the structure sits in LDS (this item and the next: smm_align_graph.h, shared with smm_align_graph_logz.hip): classes,
//     flags and the 8-word masks.  Wave 0 walks the nodes once up and once down for the
//     fewest / most nodes before a node on a path from a start node (bmin, bmax) and after it on a path to an end node (amin,
//     amax); Lmin and Lmax, the count rule's path lengths, come from the same walk.  A node no start -> end path crosses has no
//     cells;
//   - the cells of column m that lie on a complete alignment: max(bmin + 1, T - amax (kp-1)) <= n <= min(T - amin, (bmax+1)(kp-1))
//     (align_opt_range with nb -> bmin, na -> amin, m -> bmax, M-1-m -> amax; the same cells for a graph built from flags);
//   - pred(m) is no contiguous run, so h[.][m] is PULLED over the edges themselves: the gam columns stay in the workspace, a
//     second [M][T+1] area behind the h columns, and the head of column m lists its predecessors that have cells, stages
//     trans[a_m][a_j] for them in LDS and forms h[n][m] over the hull of their cells (clipped to what column m's cells can
//     reach); a cell outside a predecessor's own range counts as -inf.  The subtraction follows the maximum, as the definition
//     has it.  A column costs (cells) x (kp - 1 + |pred|);
//   - gam[T][j] is kept for every end(j);
//   - the back-trace (wave 0) is smm_align_opt_kernel's loop over the pairs (k, j), the candidates walked from the set bits of
//     a mask (first the end(j), then pred of the node just placed) instead of an interval.
// No atomics, no private segment; every output word has one writer.
//
// Static LDS: s_h and s_len 22.7 KB, the masks 8 KB, s_gamT and s_tr 4 KB, fourteen int arrays of a node each 14 KB: 49 KB of
// the 64 KB a workgroup may declare.  (Pull keeps no successor masks.)
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3                                            // positions per thread (odd: smm_align_tile.h)
#include "smm_align_tile.h"
#include "smm_align_graph.h"

#define SMM_GRAPH_U 4                                            // positions per thread and round when h is formed

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_kernel(SmmAlignArgs a)
{
    __shared__ double s_h[SMM_ALIGN_HS];
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ double s_gamT[SMM_MAX_TRANSCRIPT];              // gam[T][j] (-inf where (T, j) is no cell)
    __shared__ double s_tr[SMM_MAX_TRANSCRIPT];                // trans[a_m][a_j], j = s_pl[i]
    __shared__ double s_best;
    __shared__ uint32_t s_mask[SMM_MAX_TRANSCRIPT * SMM_GRAPH_WORDS];
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_fl[SMM_MAX_TRANSCRIPT];                   // bit 0: start(m), bit 1: end(m)
    __shared__ int s_bmin[SMM_MAX_TRANSCRIPT], s_bmax[SMM_MAX_TRANSCRIPT];   // nodes before m on a path from a start node
    __shared__ int s_amin[SMM_MAX_TRANSCRIPT], s_amax[SMM_MAX_TRANSCRIPT];   // nodes after m on a path to an end node
    __shared__ int s_lo[SMM_MAX_TRANSCRIPT], s_hi[SMM_MAX_TRANSCRIPT];       // column m's cells (lo > hi: none)
    __shared__ int s_slo[SMM_MAX_TRANSCRIPT], s_shi[SMM_MAX_TRANSCRIPT];     // the positions > 0 that hold column m's sources
    __shared__ int s_pl[SMM_MAX_TRANSCRIPT];                   // the predecessors of the column, the candidates of the back-trace
    __shared__ int s_start[SMM_MAX_TRANSCRIPT], s_entry[SMM_MAX_TRANSCRIPT];   // the segments, filled from the top down
    __shared__ int s_used[SMM_MAX_TRANSCRIPT];
    __shared__ int s_wcnt[4], s_wlo[4], s_whi[4];              // per wave: predecessors with cells, the hull of their cells
    __shared__ int s_len2[2], s_first_seg;                     // [0], [1]: the fewest and most nodes on a start -> end path
    __shared__ int s_flag[2];                                  // [0] an id or a mask bit out of range, [1] a NaN / +inf reached the DP

    const int tid = threadIdx.x;
    const int vid = a.order[blockIdx.x];
    const AlignVideo v = align_video(a, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const double *trans = v.trans, *len = v.len, *endpen = v.endpen, *cum = v.cum;
    const size_t T1 = v.T1;
    double *hcol = a.hcols + a.hoff[vid];                      // [M][T+1]
    double *gcol = hcol + (size_t)M * T1;                      // [M][T+1]: the gam columns
    int32_t *used = a.used ? a.used + v.t0 : nullptr;

    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    // ---- the structure -> LDS (smm_align_graph.h)
    graph_load<true>(a, v, s_a, s_fl, s_mask, s_flag, tid);
    if (tid < M) {
        s_gamT[tid] = SMM_NEG_INF;
        s_used[tid] = 0;
    }
    __syncthreads();
    if (s_flag[0] != 0 || kw < 1) {
        align_write_none(a, v, vid, tid);
        if (used && tid < M) used[tid] = 0;
        return;
    }

    // ---- path lengths (wave 0), the columns' cells, the count rule
    if (tid < 64) graph_path_lengths(s_mask, s_fl, M, s_bmin, s_bmax, s_amin, s_amax, s_len2, tid);
    __syncthreads();
    graph_cells(M, T, kw, s_bmin, s_bmax, s_amin, s_amax, s_lo, s_hi, tid);
    if (graph_no_path(s_len2, T, kw)) {
        align_write_none(a, v, vid, tid);
        if (used && tid < M) used[tid] = 0;
        return;
    }

    // ---- the tables the structure reads; h[0][m] of the start nodes
    if (graph_tables_bad(v, s_a, s_fl, s_mask, tid)) s_flag[1] = 1;
    if (tid < M && (s_fl[tid] & 1)) hcol[(size_t)tid * T1] = v.init[s_a[tid]];
    // ---- prefix sums (smm_align_tile.h): tiles of frames through LDS, lane c adds class c serially, cum[c][n] class-major
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
        if (tid == 0) { s_slo[m] = slo; s_shi[m] = shi; }
        __syncthreads();
        // ---- h[.][m] over the edges
        // (SMM_GRAPH_U positions per thread at a time: their loads are in flight together, the stores follow)
        for (int nb = slo + tid; nb <= shi; nb += SMM_GRAPH_U * SMM_ALIGN_THREADS) {
            double mx[SMM_GRAPH_U], cu[SMM_GRAPH_U];
#pragma unroll
            for (int u = 0; u < SMM_GRAPH_U; ++u) {
                const int n = nb + u * SMM_ALIGN_THREADS;
                mx[u] = SMM_NEG_INF;
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
            for (int u = 0; u < SMM_GRAPH_U; ++u) {
                const int n = nb + u * SMM_ALIGN_THREADS;
                if (n <= shi) hm[n] = mx[u] - cu[u];
            }
        }
        __threadfence_block();
        align_tiles(lo, hi, first ? 0 : slo, shi, d_all, s_h, tid,
                    [&](int s) { return ((s >= slo && s <= shi) || (first && s == 0)) ? hm[s] : SMM_NEG_INF; },
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
                                gm[n] = gam;
                            }
                        }
                    });
        __threadfence_block();
    }
    __syncthreads();

    // ---- closing step and back-trace (wave 0)
    if (tid < 64) {
        double best = SMM_NEG_INF;
        for (int j = tid; j < M; j += 64)
            if (s_fl[j] & 2) best = align_max(best, s_gamT[j] + (endpen ? endpen[s_a[j]] : 0.0));
        best = align_wave_max(best);
        if (tid == 0) s_best = best;
        const bool bad = s_flag[1] != 0 || align_bad_bits(best);
        const bool none = !bad && align_nonfinite_bits(best);  // -inf: the tables, or the path lengths, leave no alignment
        if (!bad && !none) {
            int n = T, cur = M, idx = M;
            bool fail = false;
            while (n > 0) {
                // candidates: pred(cur) (cur = M: the nodes that may end) that have a cell at n, each with every length
                int nc = 0;
                for (int j0 = 0; j0 < cur; j0 += 64) {
                    const int j = j0 + tid;
                    const bool is = j < cur && (cur < M ? graph_edge(s_mask, cur, j) : (s_fl[j] & 2) != 0) && n >= s_lo[j] && n <= s_hi[j];
                    const unsigned long long ballot = __ballot(is);
                    if (is) s_pl[nc + graph_rank(ballot, tid)] = j;
                    nc += __popcll(ballot);
                }
                __threadfence_block();
                const int kmax = kw < n ? kw : n;
                const int total = nc * kmax;
                const double *trow = trans + (size_t)(cur < M ? s_a[cur] : 0) * cm;
                double mx = SMM_NEG_INF;
                int key = 0x7fffffff;                          // k * SMM_MAX_TRANSCRIPT + j: the smallest k, then the smallest j
                for (int e = tid; e < total; e += 64) {
                    const int ci = e / kmax, k = 1 + (e - ci * kmax), i = s_pl[ci], s = n - k;
                    if (s == 0 ? (s_fl[i] & 1) == 0 : (s < s_slo[i] || s > s_shi[i])) continue;
                    const int c = s_a[i];
                    const double w = cur < M ? trow[c] : (endpen ? endpen[c] : 0.0);
                    const double val = (cum[(size_t)c * T1 + n] + (hcol[(size_t)i * T1 + s] + len[(size_t)k * cm + c])) + w;
                    const int kk = k * SMM_MAX_TRANSCRIPT + i;
                    if (val > mx || (val == mx && kk < key)) { mx = val; key = kk; }
                }
                const double top = align_wave_max(mx);
                key = align_wave_min(mx == top ? key : 0x7fffffff);
                __threadfence_block();                         // the readers of s_pl before the next round's writers
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

    // ---- outputs (smm_align_tile.h): the recorded segments carry the nodes of the path
    const int seg0 = empty ? M : s_first_seg;
    align_write_result(a, v, vid, s_start, [&](int l) { return s_a[s_entry[l]]; }, seg0, failed, empty, best, tid);
    if (used && tid < M) used[tid] = empty ? 0 : s_used[tid];
}

void smm_launch_align_graph(const SmmAlignArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_graph_kernel, dim3((unsigned)a.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}
