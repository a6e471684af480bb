// smm_align_graph_entropy.hip -- the exact entropy of the transcript-graph posterior over ALIGNMENTS, H = -sum_y p(y) log p(y)
// (include/smmdp.h: smm_align_graph_entropy_f64): forward by smm_align_graph_logz_fwd_kernel, the q and bh columns by
// smm_align_graph_logz_bwd_kernel, one more pass here.  What smm_entropy.hip is to smm_logz_kernel.
//
// The chain rule of entropy over the decisions of smm_align_graph_sample.hip's walk: an alignment is drawn by an end node, then
// per segment its start and, unless that is 0, the node in front of it; H is the sum over every decision the walk can come to
// of the probability that it comes to it times the entropy of its draw.  With, for a list of weights w,
//   Hloc(w) = log Z - A / Z,   Z = sum exp(w - max w),  A = sum exp(w - max w) (w - max w)      (>= 0 term by term: Z >= 1, A <= 0)
// and the posteriors of "a segment of node j ends at n" and "a segment of node j starts at s",
//   E[n][j] = exp(gam[n][j] + (q[n][j] - cum[n][a_j]) - logZ_g),   S[s][j] = exp(h[s][j] + bh[s][j] - logZ_g):
//   H_end  = Hloc( gam[T][j] + closing_j : end(j) )
//   H_span = sum_j sum_{n in [lo_j, hi_j]}   E[n][j] Hloc( h[n-k][j] + len[k][a_j] : k = 1 .. min(kw, n) )
//   H_pred = sum_j sum_{s in [slo_j, shi_j]} S[s][j] Hloc( gam[s][i] + trans[a_j][a_i] : i in pred(j) )
//   H      = (H_end + H_span) + H_pred
// A candidate of weight -inf has no mass (0, never 0 * -inf); a decision with a single candidate gives exactly 0, so a chain has
// H_end = H_pred = 0 and a chain with T = M has H = 0.  A decision nobody comes to (E or S = 0) is not evaluated.
//
// Inputs are what the two kernels before it leave in the video's block of the workspace (smm_align_graph_logz.hip has the layout):
// the h, gam, q and bh columns and five ints per column, lo, hi, slo, shi, z: gam[.][m] and q[.][m] hold values on [lo, hi] only,
// h[.][m] and bh[.][m] on [slo, shi] and, when z, at 0.  Everything else in the block is uninitialised memory: every read is
// gated by these ranges BEFORE the load, as in the sampler.
//
// One workgroup per video, the columns one after another (they do not depend on each other).  Per column: the span part by
// smm_align_lse.h's alogz_entropy_column over the forward kernel's tiles, E-weighted per cell; the predecessors listed as the
// forward kernel lists them (graph_compact), one position s per thread, a max pass and a sum pass in fp64.  A thread adds its
// cells in a fixed order; the three totals are block sums, a butterfly per wave and the waves in order.  No atomics, no
// private segment.  Static LDS: s_h 14.1 KB, s_len 8.1 KB, the masks 8 KB, s_tr 2 KB, eight int arrays of a node each 8 KB:
// 40.3 KB of the 64 KB a workgroup may declare.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3
#include "smm_align_tile.h"
#include "smm_align_lse.h"
#include "smm_align_graph.h"

// Hloc of the weights cand(f) hands to f(w): log Z and A / Z are two passes over them
__device__ __forceinline__ void age_add(double w, double ref, double &z, double &a)
{
    const double x = w - ref;
    const double e = exp(x);
    z = z + e;
    a = a + (e > 0.0 ? e * x : 0.0);
}

template <class Cand>
__device__ __forceinline__ double age_decide(Cand cand)
{
    double mx = SMM_NEG_INF;
    cand([&](double w) { mx = align_max(mx, w); });
    const double ref = align_nonfinite_bits(mx) ? 0.0 : mx;
    double z = 0.0, dot = 0.0;
    cand([&](double w) { age_add(w, ref, z, dot); });
    return log(z) - dot / z;
}

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_entropy_kernel(SmmAlignEntropyArgs a)
{
    __shared__ double s_h[SMM_ALIGN_HS];
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ double s_tr[SMM_MAX_TRANSCRIPT];                // trans[a_m][a_j], j = s_pl[i]
    __shared__ double s_red[SMM_ALIGN_THREADS / 64];
    __shared__ uint32_t s_mask[SMM_MAX_TRANSCRIPT * SMM_GRAPH_WORDS];
    GRAPH_SHARED_NODES;

    const int tid = threadIdx.x;
    const int vid = a.g.order[blockIdx.x];
    double *parts = a.h_parts ? a.h_parts + 3 * (size_t)vid : nullptr;
    const double lz = a.g.logz[vid];
    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    const AlignVideo v = align_video(a.g, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    bool ok = !align_nonfinite_bits(lz);       // (-inf: no alignment, an ordinary "impossible"; a finite logZ_g had a valid structure)
    if (ok) {
        graph_load<true>(a.g, v, s_a, s_fl, s_mask, s_flag, tid);
        __syncthreads();
        ok = s_flag[0] == 0;
    }
    if (!ok) {
        if (tid == 0) {
            if (align_bad_bits(lz) || !align_nonfinite_bits(lz)) a.g.err[0] = 1;   // (staging cleared the word the forward call had set)
            a.h_out[vid] = __builtin_nan("");
            if (parts) parts[0] = parts[1] = parts[2] = __builtin_nan("");
        }
        return;
    }
    const double *trans = v.trans, *len = v.len, *cum = v.cum;
    const size_t T1 = v.T1;
    const double *block = a.g.cols + a.g.hoff[vid];
    const GraphCols<const double> p = graph_cols(block, M, T1);
    graph_load_ranges(graph_rng(block), nd, M, tid);
    __threadfence_block();
    __syncthreads();

    // ---- the end node
    double h_end = 0.0;
    if (tid == 0)
        h_end = age_decide([&](auto f) {
            graph_each_end(nd, M, T, [&](int j) { f(p.g[(size_t)j * T1 + T] + graph_closing(v.endpen, s_a[j])); });
        });

    // ---- columns
    double x_span = 0.0, x_pred = 0.0;                         // this thread's cells, in the order it comes to them
    const int d_all = align_d_all(kw);
    for (int m = 0; m < M; ++m) {
        const int lo = s_lo[m], hi = s_hi[m], slo = s_slo[m], shi = s_shi[m];
        const bool first = s_z[m] != 0;
        const int c = s_a[m];
        __syncthreads();                                       // the previous column's readers of s_len, s_h, s_pl, s_tr, s_w*
        if (lo > hi) continue;                                 // a node without a cell
        const double *hm = p.h + (size_t)m * T1, *gm = p.g + (size_t)m * T1;
        const double *qm = p.q + (size_t)m * T1, *bhm = p.bh + (size_t)m * T1;
        const double *cumc = cum + (size_t)c * T1;
        align_stage_len(len, cm, c, kw, d_all, s_len, tid);
        // ---- the node in front: pred(m) as the forward kernel lists it, one start s per thread
        const int np = graph_list<false>(s_mask, m, M, nd, tid, [&](int slot, int j) { s_tr[slot] = trans[(size_t)c * cm + s_a[j]]; });
        __syncthreads();
        if (np > 1)                                            // (a single predecessor: exactly 0)
            for (int s = slo + tid; s <= shi; s += SMM_ALIGN_THREADS) {
                const double ps = exp((hm[s] + bhm[s]) - lz);
                if (!(ps > 0.0)) continue;                     // (nobody starts here: its candidates may all be -inf)
                x_pred = x_pred + ps * age_decide([&](auto f) {
                    graph_each_pred(nd, np, s, [&](int i, int j) { f(p.g[(size_t)j * T1 + s] + s_tr[i]); });
                });
            }
        // ---- the start of the segment: the forward kernel's column again
        alogz_entropy_column(lo, hi, first ? 0 : slo, shi, d_all, s_h, s_len, tid,
                             [&](int s) { return ((s >= slo && s <= shi) || (first && s == 0)) ? hm[s] : SMM_NEG_INF; },
                             [&](int n, double hloc) {
                                 const double pe = exp((gm[n] + (qm[n] - cumc[n])) - lz);
                                 if (pe > 0.0) x_span = x_span + pe * hloc;   // (nobody ends here: hloc may be NaN)
                             });
    }
    const double h_span = graph_block_sum(x_span, s_red, tid);
    const double h_pred = graph_block_sum(x_pred, s_red, tid);
    if (tid == 0) {
        const double h = (h_end + h_span) + h_pred;
        if (align_nonfinite_bits(h)) a.g.err[0] = 1;           // (a posterior that does not add up: not reached from a finite logZ_g)
        a.h_out[vid] = h;
        if (parts) { parts[0] = h_end; parts[1] = h_span; parts[2] = h_pred; }
    }
}

void smm_launch_align_graph_entropy(const SmmAlignEntropyArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_graph_entropy_kernel, dim3((unsigned)a.g.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}
