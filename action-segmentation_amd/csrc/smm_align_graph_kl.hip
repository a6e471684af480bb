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
// the structure is tested without storing them (graph_load_nodes) and a column reads its own mask row from global memory, one
// word per thread.  A thread adds its cells in a fixed order; each total is one block sum.  No atomics, no private segment.
// Static LDS: s_h 2 x 14.1 KB, s_len 2 x 8.1 KB, s_tr 2 x 2 KB, eight int arrays of a node each 8 KB: 56.4 KB of the 64 KB.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3
#include "smm_align_tile.h"
#include "smm_align_lse.h"
#include "smm_align_graph.h"

#define SMM_AGK_RNG 5              // ints per column (smm_align_graph_logz.hip: SMM_AGL_RNG)

__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_kl_kernel(SmmAlignKlArgs a)
{
    __shared__ double s_hp[SMM_ALIGN_HS], s_hq[SMM_ALIGN_HS];
    __shared__ double s_lenp[SMM_ALIGN_LEN], s_lenq[SMM_ALIGN_LEN];
    __shared__ double s_trp[SMM_MAX_TRANSCRIPT], s_trq[SMM_MAX_TRANSCRIPT];   // trans[a_m][a_j], j = s_pl[i], of each side
    __shared__ double s_red[SMM_ALIGN_THREADS / 64];
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];
    __shared__ int s_fl[SMM_MAX_TRANSCRIPT];
    __shared__ int s_lo[SMM_MAX_TRANSCRIPT], s_hi[SMM_MAX_TRANSCRIPT];       // column m's cells
    __shared__ int s_slo[SMM_MAX_TRANSCRIPT], s_shi[SMM_MAX_TRANSCRIPT];     // the positions > 0 that hold h[.][m] and bh[.][m]
    __shared__ int s_z[SMM_MAX_TRANSCRIPT];                    // column m has an h[0]
    __shared__ int s_pl[SMM_MAX_TRANSCRIPT];                   // the predecessors of the column
    __shared__ int s_wcnt[4], s_wlo[4], s_whi[4];
    __shared__ int s_flag[2];                                  // [0] an id or a mask bit out of range, [1] q's ranges are not p's

    const int tid = threadIdx.x;
    const int vid = a.g.order[blockIdx.x];
    double *parts = a.kl_parts ? a.kl_parts + 3 * (size_t)vid : nullptr;
    const double lz = a.g.logz[vid], lzq = a.logz_q[vid];
    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    const AlignVideo v = align_video(a.g, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const size_t T1 = v.T1;
    const int *rng = reinterpret_cast<const int *>(a.g.cols + a.g.hoff[vid]);
    const int *rngq = reinterpret_cast<const int *>(a.cols_q + a.g.hoff[vid]);
    const bool bad = align_bad_bits(lz) || align_bad_bits(lzq);
    const bool both = !bad && !align_nonfinite_bits(lz) && !align_nonfinite_bits(lzq);   // (-inf: an ordinary "impossible")
    bool ok = both;
    if (ok) {                                                  // (a finite logZ_g had a valid structure and wrote its ranges)
        graph_load_nodes(a.g, v, s_a, s_fl, s_flag, tid);
        if (tid < M) {
            const int *r = rng + SMM_AGK_RNG * tid, *rq = rngq + SMM_AGK_RNG * tid;
            s_lo[tid] = r[0]; s_hi[tid] = r[1]; s_slo[tid] = r[2]; s_shi[tid] = r[3]; s_z[tid] = r[4];
            if (rq[0] != r[0] || rq[1] != r[1] || rq[2] != r[2] || rq[3] != r[3] || rq[4] != r[4]) s_flag[1] = 1;
        }
        __threadfence_block();
        __syncthreads();
        ok = s_flag[0] == 0 && s_flag[1] == 0;
    }
    if (!ok) {
        if (tid == 0) {
            // p without an alignment: NaN; p with one and q without: +inf; a NaN on either side, or a finite pair whose
            // structure or ranges failed: NaN and the error word (staging cleared the word p's forward call had set)
            const bool q_none = !bad && !align_nonfinite_bits(lz) && align_nonfinite_bits(lzq);
            const double out = q_none ? __builtin_huge_val() : __builtin_nan("");
            if (bad || both) a.g.err[0] = 1;
            a.kl_out[vid] = out;
            if (a.xent_out) a.xent_out[vid] = out;
            if (parts) parts[0] = parts[1] = parts[2] = out;
        }
        return;
    }
    const double *trans = v.trans, *len = v.len, *cum = v.cum;
    const double *transq = a.trans_q + (size_t)v.g * cm * cm, *lenq = a.len_q + (size_t)v.g * a.g.k_rows * cm;
    const double *endpenq = a.endpen_q ? a.endpen_q + (size_t)vid * cm : nullptr;
    const double *hcol = a.g.cols + a.g.hoff[vid] + 3 * (size_t)M;
    const double *gcol = hcol + (size_t)M * T1;
    const double *qcol = gcol + (size_t)M * T1;
    const double *bhcol = qcol + (size_t)M * T1;
    const double *hcolq = a.cols_q + a.g.hoff[vid] + 3 * (size_t)M;
    const double *gcolq = hcolq + (size_t)M * T1;
    const uint32_t *masks = a.g.pred_mask + (size_t)v.t0 * SMM_GRAPH_WORDS;

    // ---- the end node: the end nodes that have the cell (T, j), in index order
    double kl_end = 0.0, h_end = 0.0;
    if (tid == 0) {
        double mp = SMM_NEG_INF, mq = SMM_NEG_INF;
        for (int j = 0; j < M; ++j)
            if ((s_fl[j] & 2) && s_lo[j] <= T && T <= s_hi[j]) {
                mp = align_max(mp, gcol[(size_t)j * T1 + T] + (v.endpen ? v.endpen[s_a[j]] : 0.0));
                mq = align_max(mq, gcolq[(size_t)j * T1 + T] + (endpenq ? endpenq[s_a[j]] : 0.0));
            }
        mp = align_nonfinite_bits(mp) ? 0.0 : mp;
        mq = align_nonfinite_bits(mq) ? 0.0 : mq;
        double sp = 0.0, sq = 0.0, y = 0.0, ap = 0.0;
        bool cut = false;
        for (int j = 0; j < M; ++j)
            if ((s_fl[j] & 2) && s_lo[j] <= T && T <= s_hi[j])
                akl_add(gcol[(size_t)j * T1 + T] + (v.endpen ? v.endpen[s_a[j]] : 0.0),
                        gcolq[(size_t)j * T1 + T] + (endpenq ? endpenq[s_a[j]] : 0.0), mp, mq, sp, sq, y, ap, cut);
        akl_loc(mp, mq, sp, sq, y, ap, cut, kl_end, h_end);
    }

    // ---- columns
    double k_span = 0.0, k_pred = 0.0, h_span = 0.0, h_pred = 0.0;   // this thread's cells, in the order it comes to them
    const int d_all = align_d_all(kw);
    for (int m = 0; m < M; ++m) {
        const int lo = s_lo[m], hi = s_hi[m], slo = s_slo[m], shi = s_shi[m];
        const bool first = s_z[m] != 0;
        const int c = s_a[m];
        __syncthreads();                                       // the previous column's readers of s_len*, s_h*, s_pl, s_tr*, s_w*
        if (lo > hi) continue;                                 // a node without a cell
        const double *hm = hcol + (size_t)m * T1, *gm = gcol + (size_t)m * T1;
        const double *qm = qcol + (size_t)m * T1, *bhm = bhcol + (size_t)m * T1;
        const double *hmq = hcolq + (size_t)m * T1;
        const double *cumc = cum + (size_t)c * T1;
        align_stage_len(len, cm, c, kw, d_all, s_lenp, tid);
        align_stage_len(lenq, cm, c, kw, d_all, s_lenq, tid);
        // ---- the node in front: pred(m) as the forward kernel lists it, one start s per thread
        const bool is = tid < m && graph_edge_row(masks + (size_t)m * SMM_GRAPH_WORDS, tid) && s_lo[tid] <= s_hi[tid];
        int slot, np, ulo, uhi;
        graph_compact(is, is ? s_lo[tid] : 0, is ? s_hi[tid] : 0, s_wcnt, s_wlo, s_whi, tid, slot, np, ulo, uhi);
        if (is) {
            s_pl[slot] = tid;
            s_trp[slot] = trans[(size_t)c * cm + s_a[tid]];
            s_trq[slot] = transq[(size_t)c * cm + s_a[tid]];
        }
        __syncthreads();
        if (np > 0)                                            // (a single predecessor: exactly 0, or +inf where q cuts it)
            for (int s = slo + tid; s <= shi; s += SMM_ALIGN_THREADS) {
                const double ps = exp((hm[s] + bhm[s]) - lz);
                if (!(ps > 0.0)) continue;                     // (nobody starts here: its candidates may all be -inf)
                double mp = SMM_NEG_INF, mq = SMM_NEG_INF;
                for (int i = 0; i < np; ++i) {
                    const int j = s_pl[i];
                    if (s >= s_lo[j] && s <= s_hi[j]) {
                        mp = align_max(mp, gcol[(size_t)j * T1 + s] + s_trp[i]);
                        mq = align_max(mq, gcolq[(size_t)j * T1 + s] + s_trq[i]);
                    }
                }
                mp = align_nonfinite_bits(mp) ? 0.0 : mp;
                mq = align_nonfinite_bits(mq) ? 0.0 : mq;
                double sp = 0.0, sq = 0.0, y = 0.0, ap = 0.0;
                bool cut = false;
                for (int i = 0; i < np; ++i) {
                    const int j = s_pl[i];
                    if (s >= s_lo[j] && s <= s_hi[j])
                        akl_add(gcol[(size_t)j * T1 + s] + s_trp[i], gcolq[(size_t)j * T1 + s] + s_trq[i], mp, mq, sp, sq, y, ap, cut);
                }
                double kl, hl;
                akl_loc(mp, mq, sp, sq, y, ap, cut, kl, hl);
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
