// smm_align_graph_kl.hip -- the exact KL divergence KL(p || q) = sum_y p(y) log( p(y) / q(y) ) and the cross-entropy
// H(p, q) = -sum_y p(y) log q(y) between two transcript-graph posteriors over ALIGNMENTS of the same videos to the same graphs
// (include/smmdp.h: smm_align_graph_kl_f64): one forward call per side, the q and bh columns of p by
// smm_align_graph_logz_bwd_kernel, one more pass here.  What smm_kl.hip is to smm_entropy.hip.
//
// The chain rule of relative entropy over the decisions of smm_align_graph_sample.hip's walk, in smm_align_graph_entropy.hip's
// notation: the KL is the sum over every decision the walk can come to of the probability UNDER p that it comes to it times
// the KL of its draw.  With KLloc and Hloc of smm_align_lse.h (akl_add, akl_loc) over the candidates' weights on both sides,
//   KL_end  = KLloc( gam[T][j] + closing_j : end(j) )
//   KL_span = sum_j sum_{n in [lo_j, hi_j]}   E[n][j] KLloc( h[n-k][j] + len[k][a_j] : k = 1 .. min(kw, n) )
//   KL_pred = sum_j sum_{s in [slo_j, shi_j]} S[s][j] KLloc( gam[s][i] + trans[a_j][a_i] : i in pred(j) )
//   KL      = (KL_end + KL_span) + KL_pred;      H(p, q) = the same three sums of weight * (Hloc + KLloc)
// E and S are p's posteriors, exactly as the entropy kernel forms them.  q enters through its h and gam columns, its
// transitions, length scores and closing scores: no backward pass of q, and neither its elp nor its init is read.  Every term
// is >= 0 (KLloc is clamped), every exponential is fp64 on both sides, and both sides run the same operations: bit-identical
// sides give exactly 0.0 in every part.  A candidate that has mass under p and none under q gives +inf: an answer.
//
// The two sides share the videos, lengths, span limit and graphs, so the ranges the forward calls recorded per column are the
// same five ints: thread m compares q's with p's before anything of q's columns is read (a mismatch: the workspace was written
// for other graphs -> NaN and the error word), and every read of either side's columns is gated by p's ranges BEFORE the load.
//
// One workgroup per video, the columns one after another, as smm_align_graph_entropy_kernel; the span part by
// alogz_kl_column, whose tiles hold both sides' sources.  Two s_h and two s_len leave no room for the 8 KB of masks in LDS:
// the structure is tested without storing them (graph_load_sides) and a column reads its own mask row from global memory, one
// word per thread.  A thread adds its cells in a fixed order; each total is one block sum.  No atomics, no private segment.
// Static LDS: s_h 2 x 14.1 KB, s_len 2 x 8.1 KB, s_tr 2 x 2 KB, eight int arrays of a node each 8 KB: 56.4 KB of the 64 KB.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3
#include "smm_align_tile.h"
#include "smm_align_lse.h"
#include "smm_align_graph.h"

// KLloc and Hloc of the weights cand(f) hands to f(wp, wq): two passes over them (smm_align_lse.h: akl_add, akl_loc)
template <class Cand>
__device__ __forceinline__ void akl_decide(Cand cand, double &kl, double &hl)
{
    double mp = SMM_NEG_INF, mq = SMM_NEG_INF;
    cand([&](double wp, double wq) {
        mp = align_max(mp, wp);
        mq = align_max(mq, wq);
    });
    mp = align_nonfinite_bits(mp) ? 0.0 : mp;
    mq = align_nonfinite_bits(mq) ? 0.0 : mq;
    double sp = 0.0, sq = 0.0, y = 0.0, ap = 0.0;
    bool cut = false;
    cand([&](double wp, double wq) { akl_add(wp, wq, mp, mq, sp, sq, y, ap, cut); });
    akl_loc(mp, mq, sp, sq, y, ap, cut, kl, hl);
}

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_kl_kernel(SmmAlignKlArgs a)
{
    __shared__ double s_hp[SMM_ALIGN_HS], s_hq[SMM_ALIGN_HS];
    __shared__ double s_red[SMM_ALIGN_THREADS / 64];
    GRAPH_SHARED_SIDES;                                        // (s_flag[1]: q's ranges are not p's)

    const int tid = threadIdx.x;
    const int vid = a.g.order[blockIdx.x];
    double *parts = a.kl_parts ? a.kl_parts + 3 * (size_t)vid : nullptr;
    const double lz = a.g.logz[vid];
    const AlignVideo v = align_video(a.g, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const size_t T1 = v.T1;
    const double *block = a.g.cols + a.g.hoff[vid], *blockq = a.q.cols + a.g.hoff[vid];
    const GraphVerdict vd = graph_verdict(lz, a.q.logz[vid]);
    if (!vd.both || !graph_load_sides(a.g, v, graph_rng(block), graph_rng(blockq), nd, s_flag, tid)) {
        if (tid == 0) {
            if (vd.error()) a.g.err[0] = 1;
            a.kl_out[vid] = vd.answer();
            if (a.xent_out) a.xent_out[vid] = vd.answer();
            if (parts) parts[0] = parts[1] = parts[2] = vd.answer();
        }
        return;
    }
    const double *len = v.len, *cum = v.cum;
    const SmmAlignSideQ sq = graph_side_q(a.q, v, a.g.k_rows, vid);
    const GraphCols<const double> p = graph_cols(block, M, T1), q = graph_cols(blockq, M, T1);
    const uint32_t *masks = a.g.pred_mask + (size_t)v.t0 * SMM_GRAPH_WORDS;

    // ---- the end node
    double kl_end = 0.0, h_end = 0.0;
    if (tid == 0)
        akl_decide([&](auto f) {
            graph_each_end(nd, M, T, [&](int j) {
                f(p.g[(size_t)j * T1 + T] + graph_closing(v.endpen, s_a[j]), q.g[(size_t)j * T1 + T] + graph_closing(sq.endpen, s_a[j]));
            });
        }, kl_end, h_end);

    // ---- columns
    double k_span = 0.0, k_pred = 0.0, h_span = 0.0, h_pred = 0.0;   // this thread's cells, in the order it comes to them
    const int d_all = align_d_all(kw);
    for (int m = 0; m < M; ++m) {
        const int lo = s_lo[m], hi = s_hi[m], slo = s_slo[m], shi = s_shi[m];
        const bool first = s_z[m] != 0;
        const int c = s_a[m];
        __syncthreads();                                       // the previous column's readers of s_len*, s_h*, s_pl, s_tr*, s_w*
        if (lo > hi) continue;                                 // a node without a cell
        const double *hm = p.h + (size_t)m * T1, *gm = p.g + (size_t)m * T1;
        const double *qm = p.q + (size_t)m * T1, *bhm = p.bh + (size_t)m * T1;
        const double *hmq = q.h + (size_t)m * T1;
        const double *cumc = cum + (size_t)c * T1;
        align_stage_len(len, cm, c, kw, d_all, s_lenp, tid);
        align_stage_len(sq.len, cm, c, kw, d_all, s_lenq, tid);
        // ---- the node in front: pred(m) as the forward kernel lists it, one start s per thread
        const int np = graph_list<false>(masks, m, M, nd, tid, [&](int slot, int j) {
            s_trp[slot] = v.trans[(size_t)c * cm + s_a[j]];
            s_trq[slot] = sq.trans[(size_t)c * cm + s_a[j]];
        });
        __syncthreads();
        if (np > 0)                                            // (a single predecessor: exactly 0, or +inf where q cuts it)
            for (int s = slo + tid; s <= shi; s += SMM_ALIGN_THREADS) {
                const double ps = exp((hm[s] + bhm[s]) - lz);
                if (!(ps > 0.0)) continue;                     // (nobody starts here: its candidates may all be -inf)
                double kl, hl;
                akl_decide([&](auto f) {
                    graph_each_pred(nd, np, s, [&](int i, int j) {
                        f(p.g[(size_t)j * T1 + s] + s_trp[i], q.g[(size_t)j * T1 + s] + s_trq[i]);
                    });
                }, kl, hl);
                k_pred = k_pred + ps * kl;
                h_pred = h_pred + ps * (hl + kl);
            }
        // ---- the start of the segment: the forward kernel's column again, both sides' sources in one tile walk
        alogz_kl_column(lo, hi, first ? 0 : slo, shi, d_all, s_hp, s_hq, s_lenp, s_lenq, tid,
                        [&](int s) { return ((s >= slo && s <= shi) || (first && s == 0)) ? hm[s] : SMM_NEG_INF; },
                        [&](int s) { return ((s >= slo && s <= shi) || (first && s == 0)) ? hmq[s] : SMM_NEG_INF; },
                        [&](int n, double kl, double hl) {
                            const double pe = exp((gm[n] + (qm[n] - cumc[n])) - lz);
                            if (pe > 0.0) {                    // (nobody ends here: kl and hl may be NaN)
                                k_span = k_span + pe * kl;
                                h_span = h_span + pe * (hl + kl);
                            }
                        });
    }
    const double kl_span = graph_block_sum(k_span, s_red, tid);
    const double kl_pred = graph_block_sum(k_pred, s_red, tid);
    const double x_span = graph_block_sum(h_span, s_red, tid);
    const double x_pred = graph_block_sum(h_pred, s_red, tid);
    if (tid == 0) {
        const double kl = (kl_end + kl_span) + kl_pred;
        const double xe = ((h_end + kl_end) + x_span) + x_pred;
        if (kl != kl || xe != xe) a.g.err[0] = 1;              // (a posterior that does not add up: not reached from finite logZ_g)
        a.kl_out[vid] = kl;
        if (a.xent_out) a.xent_out[vid] = xe;
        if (parts) { parts[0] = kl_end; parts[1] = kl_span; parts[2] = kl_pred; }
    }
}

void smm_launch_align_graph_kl(const SmmAlignKlArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_graph_kl_kernel, dim3((unsigned)a.g.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
}
