// smm_align_graph_entropy_bwd.hip -- the gradients of the entropy H(p), the cross-entropy H(p, q) and KL(p || q) of
// transcript-graph posteriors with respect to p's tables (include/smmdp.h: smm_align_graph_entropy_bwd_f64,
// smm_align_graph_kl_bwd_f64).  What smm_entropy_bwd.hip is to smm_entropy.hip and smm_kl.hip, for this family.
//
// Notation: smm_align_graph_logz.hip's (h, gam, q = cum + bg, bh, the five ints per column).  An occurrence o is a span
// (node j, start s, end n = s + k), an edge (i -> j at s) or a start (node m at 0); w_x(o) its log-weight under side x:
//   span   h[s][j] + len[k][a_j] + q[n][j]
//   edge   gam[s][i] + trans[a_j][a_i] - cum[s][a_j] + bh[s][j]
//   start  h[0][m] + bh[0][m]                                   (h[0][m] = init[a_m])
// p(o) = exp(w_p(o) - logZ_p);  l(o) = -(w_q(o) - logZ_q), and for the KL (w_p(o) - logZ_p) - (w_q(o) - logZ_q).
//   dV / d theta = sum over the occurrences o that read the entry of  p(o) ( l(o) + eta-(S_o) + eta+(E_o) - V )
// eta- is the chain rule of smm_align_graph_entropy.hip / smm_align_graph_kl.hip as a message pass over the sampler's decisions:
// with L(c) = -log q_loc(c) of a candidate (KL: log p_loc(c) - log q_loc(c)) and p_loc the softmax of p's weights,
//   eta-S(0, j) = 0;   eta-S(s, j) = sum_{i in pred(j)} p_loc(i) [ L(i) + eta-E(s, i) ]       weights gam[s][i] + trans[a_j][a_i]
//   eta-E(n, j) = sum_k p_loc(k) [ L(k) + eta-S(n-k, j) ]                                      weights h[n-k][j] + len[k][a_j]
//   V-          = sum_{end(j)} p_loc(j) [ L(j) + eta-E(T, j) ]                                 weights gam[T][j] + closing_j
// eta+ is the same over the decisions of the time-forward walk, read from the backward columns:
//   eta+E(T, j) = 0;   eta+E(n, j) = sum_{m in succ(j)} p_loc(m) [ L(m) + eta+S(n, m) ]       weights trans[a_m][a_j] - cum[n][a_m] + bh[n][m]
//   eta+S(s, m) = sum_k p_loc(k) [ L(k) + eta+E(s+k, m) ]                                      weights len[k][a_m] + q[s+k][m]
//   V+          = sum_{start(m)} p_loc(m) [ L(m) + eta+S(0, m) ]                               weights h[0][m] + bh[0][m]
// sum p_loc L of one decision is formed from the sums S_p, S_q, Y, A_p of smm_align_lse.h (clamped at 0): every exponential is
// fp64 on both sides, both sides run the same operations, so bit-identical sides give L = 0, eta = 0, l = 0, V = 0 and exactly
// 0.0 in every output of the KL mode.  The entropy is the cross-entropy with q's pointers equal to p's.
//
// In front of the q-side launch of the q / bh kernel, the check kernel (below): the two sides' recorded ranges, per video.  Then
// five kernels, the first three one workgroup per video in the family's launch order, a column at a time, one position per thread:
//   eta-      columns 0 .. M-1: eta-S over the predecessor list (graph_compact), then eta-E over the span lengths; V-
//   eta+      columns M-1 .. 0: eta+E over the successor list, then eta+S over the span lengths; V+
//   assembly  per column: one block sum per edge -> the video's part of g_trans; per position f the sum of the span terms that
//             start at f minus the sum of those that end at f -> D[f][j]; thread k the span terms of length k -> the video's part
//             of g_len; the start nodes -> its part of g_init
//   occ       g_elp[f][a_j] += u * (running sum of D[.][j] up to f): a span's term lies on each of its frames
//   reduce    g_trans, g_init, g_len = sum over the group's videos, in video order, of u times the video's part
// Every read of a column is gated by its recorded range before the load; a decision without mass under p is not evaluated
// (its eta is 0), a term of p(o) = 0 neither.  The spans are read from global memory (L2), not from LDS tiles: see DESIGN 4r.
// The caller's scratch: per video five [M][T+1] blocks (eta-S, eta-E, eta+E, eta+S, D) in the order of the workspace's column
// blocks, then per video its parts (g_len [k_rows][c_max], g_trans [c_max][c_max], g_init [c_max], V-, state), then the log Z of q the call
// uses [b] (the check kernel's), then V+ [b].  The videos' five blocks lie in the order and at 5/4 of the cell offsets of the
// workspace's column blocks (smm_launch.h: smm_graph_cells_before).
// No atomics, no private segment, every sum in a fixed order.  Static LDS: two s_len 16.2 KB, two s_tr 4 KB, eight int arrays 8 KB.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3
#include "smm_align_tile.h"
#include "smm_align_lse.h"
#include "smm_align_graph.h"

#define SMM_AGB_OCC_THREADS 256

// (a video's state in its parts, SMM_AGB_RUN / _SKIP / _NAN, and the size of the parts: smm_launch.h)
__host__ __device__ inline size_t agb_part_doubles(int cm, int k_rows) { return smm_agb_part_doubles(cm, k_rows); }

// the two sides' columns, q's tables (p's are the AlignVideo's) and the scratch blocks (smm_align_graph.h) of one video
struct AgbVideo : GraphGradScratch {
    const int *rng, *rngq;                                     // the columns' recorded ranges
    GraphCols<const double> p, q;
    SmmAlignSideQ tq;                                          // (trans, len, endpen: the video's)
    const double *cumq;
    const uint32_t *masks;
    double lzp, lzq;
};

__device__ __forceinline__ AgbVideo agb_video(const SmmAlignEntBwdArgs &a, const AlignVideo &v, int vid)
{
    AgbVideo x;
    static_cast<GraphGradScratch &>(x) = graph_grad_scratch(a, v, vid);
    const int64_t ho = a.g.hoff[vid];
    x.rng = graph_rng(a.g.cols + ho); x.rngq = graph_rng(a.q.cols + ho);
    x.p = graph_cols<const double>(a.g.cols + ho, v.M, v.T1);
    x.q = graph_cols<const double>(a.q.cols + ho, v.M, v.T1);
    x.tq = graph_side_q(a.q, v, a.g.k_rows, vid);
    x.cumq = a.q.hist + a.g.videos[vid].hist_off;
    x.masks = a.g.pred_mask + (size_t)v.t0 * SMM_GRAPH_WORDS;
    x.lzp = a.g.logz[vid]; x.lzq = a.q.logz[vid];
    return x;
}

// ---- one decision: the sums of its second pass (smm_align_lse.h: akl_add) and the expected eta of the chosen candidate
struct AgbAcc {
    double sp, sq, y, ap, e;
    bool cut;
};

__device__ __forceinline__ void agb_add(double wp, double wq, const double *eta, double mp, double mq, AgbAcc &c)
{
    const double xp = wp - mp;
    const double ep = exp(xp);
    c.sp = c.sp + ep;
    c.sq = c.sq + exp(wq - mq);
    if (ep > 0.0) {
        const double xq = wq - mq;
        c.ap = c.ap + ep * xp;
        if (xq == SMM_NEG_INF) c.cut = true; else c.y = c.y + ep * xq;
        if (eta) c.e = c.e + ep * eta[0];
    }
}

// sum_c p_loc(c) [ L(c) + eta(c) ] over the candidates cand(f) hands to f(wp, wq, eta or null); 0 for a decision without mass
// under p.  The local sum is clamped at 0 as KLloc is; +inf where q excludes a candidate that has mass under p.
template <class Cand>
__device__ __forceinline__ double agb_decide(int kl, Cand cand)
{
    double mp = SMM_NEG_INF, mq = SMM_NEG_INF;
    cand([&](double wp, double wq, const double *) {
        mp = align_max(mp, wp);
        mq = align_max(mq, wq);
    });
    if (align_nonfinite_bits(mp)) return 0.0;
    mq = align_nonfinite_bits(mq) ? 0.0 : mq;
    AgbAcc c;
    c.sp = c.sq = c.y = c.ap = c.e = 0.0;
    c.cut = false;
    cand([&](double wp, double wq, const double *eta) { agb_add(wp, wq, eta, mp, mq, c); });
    const double lsp = log(c.sp), lsq = log(c.sq);
    const double loc = kl ? (c.ap - c.y) / c.sp + (lsq - lsp) : lsq - c.y / c.sp;
    const double lc = c.cut ? __builtin_huge_val() : (loc > 0.0 ? loc : (loc == loc ? 0.0 : loc));
    return lc + c.e / c.sp;
}

// p(o) ( l(o) + eta - V ) of one occurrence: xp = w_p(o), xq = w_q(o) without their log Z; 0 where p(o) = 0
__device__ __forceinline__ double agb_term(double xp, double xq, double eta, double lzp, double lzq, double val, int kl)
{
    const double lp = xp - lzp;
    const double po = exp(lp);
    if (!(po > 0.0)) return 0.0;
    const double lq = xq - lzq;
    const double l = kl ? lp - lq : -lq;
    return po * ((eta + l) - val);
}

// ---- q's workspace, before anything in it is read or written through p's offsets: thread m compares the five ints the two
// forward calls recorded for column m (a function of graph, T and span limit only).  out[vid] is the log Z of q that every later
// kernel of the call sees, the q-side launch of smm_align_graph_logz_bwd_kernel included, which skips a video whose log Z is not
// finite: q's own where the ranges agree; NaN (-> the error word, the value NaN) where they differ: the workspace was written
// for other graphs; -inf (skipped silently) where p has no finite log Z and so no ranges to compare with.  A log Z of q that is
// not finite passes as it is.  The reads stay inside q's workspace whatever it holds: its size was checked against the layout.
__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_entropy_bwd_check_kernel(SmmAlignEntBwdArgs a, const double *logz_q,
                                                                                             double *out)
{
    __shared__ int s_diff;
    const int tid = threadIdx.x, vid = blockIdx.x;
    const double lzp = a.g.logz[vid], lzq = logz_q[vid];
    if (align_nonfinite_bits(lzq) || align_nonfinite_bits(lzp)) {
        if (tid == 0) out[vid] = align_nonfinite_bits(lzq) ? lzq : SMM_NEG_INF;
        return;
    }
    if (tid == 0) s_diff = 0;
    __syncthreads();
    const int M = (int)(a.g.toff[vid + 1] - a.g.toff[vid]);
    if (tid < M && graph_range_differs(graph_rng(a.g.cols + a.g.hoff[vid]), graph_rng(a.q.cols + a.g.hoff[vid]), tid)) s_diff = 1;
    __syncthreads();
    if (tid == 0) out[vid] = s_diff ? __builtin_nan("") : lzq;
}

// ---- eta-, V-, and each video's state
__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_eta_minus_kernel(SmmAlignEntBwdArgs a)
{
    GRAPH_SHARED_SIDES;
    const int tid = threadIdx.x;
    const int vid = a.g.order[blockIdx.x];
    const AlignVideo v = align_video(a.g, vid);
    const AgbVideo x = agb_video(a, v, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M, kl = a.kl;
    const size_t T1 = v.T1;
    const GraphVerdict vd = graph_verdict(x.lzp, x.lzq);
    if (!vd.both || !graph_load_sides(a.g, v, x.rng, x.rngq, nd, s_flag, tid)) {
        if (tid == 0) {                                        // (p without an alignment: nothing to differentiate)
            if (vd.error()) a.g.err[0] = 1;
            if (a.value) a.value[vid] = vd.answer();
            x.vals[0] = vd.answer();
            x.vals[1] = vd.q_none ? SMM_AGB_NAN : SMM_AGB_SKIP;
        }
        return;
    }

    const int d_all = align_d_all(kw);
    for (int m = 0; m < M; ++m) {
        const GraphRange r = graph_range(nd, m);
        const int c = s_a[m];
        __syncthreads();                                       // the previous column's readers of s_len*, s_pl, s_tr*, s_w*
        if (r.lo > r.hi) continue;                             // a node without a cell
        const double *hmp = x.p.h + (size_t)m * T1, *hmq = x.q.h + (size_t)m * T1;
        double *es = x.em_s + (size_t)m * T1, *ee = x.em_e + (size_t)m * T1;
        align_stage_len(v.len, cm, c, kw, d_all, s_lenp, tid);
        align_stage_len(x.tq.len, cm, c, kw, d_all, s_lenq, tid);
        // ---- the node in front: pred(m) as the forward kernel lists it, one start s per thread
        const int np = graph_list<false>(x.masks, m, M, nd, tid, [&](int slot, int j) {
            s_trp[slot] = v.trans[(size_t)c * cm + s_a[j]];
            s_trq[slot] = x.tq.trans[(size_t)c * cm + s_a[j]];
        });
        __syncthreads();
        for (int s = r.slo + tid; s <= r.shi; s += SMM_ALIGN_THREADS)
            es[s] = agb_decide(kl, [&](auto f) {
                graph_each_pred(nd, np, s, [&](int i, int j) {
                    const size_t at = (size_t)j * T1 + s;
                    f(x.p.g[at] + s_trp[i], x.q.g[at] + s_trq[i], x.em_e + at);
                });
            });
        if (r.z && tid == 0) es[0] = 0.0;
        __threadfence_block();
        __syncthreads();
        // ---- the start of the segment: the starts > 0 by rising k, then 0, which adds no eta (a loop of its own: through an
        // enumerator shared with the assembly kernel this kernel measured 0.3 % slower, the assembly up to 2.6 %)
        for (int n = r.lo + tid; n <= r.hi; n += SMM_ALIGN_THREADS)
            ee[n] = agb_decide(kl, [&](auto f) {
                const int kmax = kw < n ? kw : n;
                const int k0 = n - r.shi > 1 ? n - r.shi : 1, k1 = n - r.slo < kmax ? n - r.slo : kmax;
                for (int k = k0; k <= k1; ++k)
                    f(hmp[n - k] + s_lenp[k + SMM_ALIGN_R], hmq[n - k] + s_lenq[k + SMM_ALIGN_R], es + (n - k));
                if (r.z && n <= kw) f(hmp[0] + s_lenp[n + SMM_ALIGN_R], hmq[0] + s_lenq[n + SMM_ALIGN_R], nullptr);
            });
        __threadfence_block();
    }
    __syncthreads();

    // ---- the end node
    if (tid == 0) {
        const double val = agb_decide(kl, [&](auto f) {
            graph_each_end(nd, M, T, [&](int j) {
                const size_t at = (size_t)j * T1 + T;
                f(x.p.g[at] + graph_closing(v.endpen, s_a[j]), x.q.g[at] + graph_closing(x.tq.endpen, s_a[j]), x.em_e + at);
            });
        });
        if (val != val) a.g.err[0] = 1;                        // (a posterior that does not add up: not reached from finite logZ_g)
        if (a.value) a.value[vid] = val;
        x.vals[0] = val;
        x.vals[1] = graph_grad_state(val);
    }
}

// ---- eta+ and V+
__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_eta_plus_kernel(SmmAlignEntBwdArgs a)
{
    GRAPH_SHARED_SIDES;
    const int tid = threadIdx.x;
    const int vid = a.g.order[blockIdx.x];
    const AlignVideo v = align_video(a.g, vid);
    const AgbVideo x = agb_video(a, v, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M, kl = a.kl;
    const size_t T1 = v.T1;
    if (x.vals[1] != SMM_AGB_RUN) {                            // (nothing to walk: V+ is what the eta- kernel answered)
        if (tid == 0) x.vplus[0] = x.vals[0];
        return;
    }
    graph_load_sides(a.g, v, x.rng, x.rngq, nd, s_flag, tid);

    const int d_all = align_d_all(kw);
    for (int m = M - 1; m >= 0; --m) {
        const GraphRange r = graph_range(nd, m);
        const int c = s_a[m];
        __syncthreads();
        if (r.lo > r.hi) continue;
        const double *qmp = x.p.q + (size_t)m * T1, *qmq = x.q.q + (size_t)m * T1;
        double *es = x.ep_s + (size_t)m * T1, *ee = x.ep_e + (size_t)m * T1;
        align_stage_len(v.len, cm, c, kw, d_all, s_lenp, tid);
        align_stage_len(x.tq.len, cm, c, kw, d_all, s_lenq, tid);
        // ---- the node behind: succ(m) as the backward kernel lists it, one end n per thread
        // (graph_list<true>'s statements with the mask row's address formed first, as a copy: through the helper this kernel
        // measured 0.4 % slower on cfg4)
        const bool is = tid > m && tid < M && graph_edge(x.masks + (size_t)tid * SMM_GRAPH_WORDS, 0, m) && s_slo[tid] <= s_shi[tid];
        int slot, np, ulo, uhi;
        graph_compact(is, is ? s_slo[tid] : 0, is ? s_shi[tid] : 0, s_wcnt, s_wlo, s_whi, tid, slot, np, ulo, uhi);
        if (is) {
            s_pl[slot] = tid;
            s_trp[slot] = v.trans[(size_t)s_a[tid] * cm + c];
            s_trq[slot] = x.tq.trans[(size_t)s_a[tid] * cm + c];
        }
        __syncthreads();
        for (int n = r.lo + tid; n <= r.hi; n += SMM_ALIGN_THREADS)
            ee[n] = n == T ? 0.0 : agb_decide(kl, [&](auto f) {
                for (int i = 0; i < np; ++i) {
                    const int t = s_pl[i];
                    if (n >= s_slo[t] && n <= s_shi[t]) {
                        const size_t at = (size_t)t * T1 + n, cu = (size_t)s_a[t] * T1 + n;
                        f((s_trp[i] - v.cum[cu]) + x.p.bh[at], (s_trq[i] - x.cumq[cu]) + x.q.bh[at], x.ep_s + at);
                    }
                }
            });
        __threadfence_block();
        __syncthreads();
        // ---- the end of the segment
        const int smin = r.z ? 0 : r.slo;
        for (int s = smin + tid; s <= r.shi; s += SMM_ALIGN_THREADS) {
            if (s != 0 && s < r.slo) continue;                 // (between an h[0] and the column's other starts)
            es[s] = agb_decide(kl, [&](auto f) {
                const int kmax = kw < T - s ? kw : T - s;
                const int k0 = r.lo - s > 1 ? r.lo - s : 1, k1 = r.hi - s < kmax ? r.hi - s : kmax;
                for (int k = k0; k <= k1; ++k)
                    f(s_lenp[k + SMM_ALIGN_R] + qmp[s + k], s_lenq[k + SMM_ALIGN_R] + qmq[s + k], ee + (s + k));
            });
        }
        __threadfence_block();
    }
    __syncthreads();

    // ---- the start node: the start nodes that have cells, in index order
    if (tid == 0)
        x.vplus[0] = agb_decide(kl, [&](auto f) {
            for (int m = 0; m < M; ++m)
                if (s_z[m]) {
                    const size_t at = (size_t)m * T1;
                    f(x.p.h[at] + x.p.bh[at], x.q.h[at] + x.q.bh[at], x.ep_s + at);
                }
        });
}

// ---- the video's parts of g_trans, g_init and g_len, and D
__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_entropy_bwd_kernel(SmmAlignEntBwdArgs a)
{
    GRAPH_SHARED_SIDES;
    __shared__ double s_red[SMM_ALIGN_THREADS / 64];
    const int tid = threadIdx.x;
    const int vid = a.g.order[blockIdx.x];
    const AlignVideo v = align_video(a.g, vid);
    const AgbVideo x = agb_video(a, v, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M, kl = a.kl;
    const size_t T1 = v.T1;
    if (x.vals[1] != SMM_AGB_RUN) return;
    const double val = x.vals[0], lzp = x.lzp, lzq = x.lzq;
    double *lpart = x.part, *tpart = x.part + (size_t)a.g.k_rows * cm, *ipart = tpart + (size_t)cm * cm;
    for (int e = tid; e < a.g.k_rows * cm + cm * cm + cm; e += SMM_ALIGN_THREADS) lpart[e] = 0.0;
    graph_load_sides(a.g, v, x.rng, x.rngq, nd, s_flag, tid);  // (its barriers: the zeros before the sums)

    const int d_all = align_d_all(kw);
    for (int m = 0; m < M; ++m) {
        const int lo = s_lo[m], hi = s_hi[m], slo = s_slo[m], shi = s_shi[m];
        const bool first = s_z[m] != 0;
        const int c = s_a[m];
        __syncthreads();
        if (lo > hi) continue;
        const size_t col = (size_t)m * T1;
        const double *hmp = x.p.h + col, *hmq = x.q.h + col, *qmp = x.p.q + col, *qmq = x.q.q + col;
        const double *bhmp = x.p.bh + col, *bhmq = x.q.bh + col;
        const double *cump = v.cum + (size_t)c * T1, *cumq = x.cumq + (size_t)c * T1;
        const double *es = x.em_s + col, *ee = x.ep_e + col, *ps = x.ep_s + col;
        double *dm = x.dd + col;
        align_stage_len(v.len, cm, c, kw, d_all, s_lenp, tid);
        align_stage_len(x.tq.len, cm, c, kw, d_all, s_lenq, tid);
        // (graph_list's statements with the mask row's address formed first, as a copy: see the span loops below)
        const bool is = tid < m && graph_edge(x.masks + (size_t)m * SMM_GRAPH_WORDS, 0, tid) && s_lo[tid] <= s_hi[tid];
        int slot, np, ulo, uhi;
        graph_compact(is, is ? s_lo[tid] : 0, is ? s_hi[tid] : 0, s_wcnt, s_wlo, s_whi, tid, slot, np, ulo, uhi);
        if (is) {
            s_pl[slot] = tid;
            s_trp[slot] = v.trans[(size_t)c * cm + s_a[tid]];
            s_trq[slot] = x.tq.trans[(size_t)c * cm + s_a[tid]];
        }
        __syncthreads();
        // ---- the edges into m: one block sum each, in the list's order
        for (int i = 0; i < np; ++i) {
            const int j = s_pl[i];
            const int e0 = slo > s_lo[j] ? slo : s_lo[j], e1 = shi < s_hi[j] ? shi : s_hi[j];
            const double trp = s_trp[i], trq = s_trq[i];
            double acc = 0.0;
            for (int s = e0 + tid; s <= e1; s += SMM_ALIGN_THREADS) {
                const size_t at = (size_t)j * T1 + s;
                acc = acc + agb_term(x.p.g[at] + ((trp - cump[s]) + bhmp[s]), x.q.g[at] + ((trq - cumq[s]) + bhmq[s]),
                                     x.em_e[at] + ps[s], lzp, lzq, val, kl);
            }
            const double tot = graph_block_sum(acc, s_red, tid);
            if (tid == 0) tpart[(size_t)c * cm + s_a[j]] += tot;
        }
        // ---- D[f][m]: the span terms that start at f minus those that end at f
        // (eta+'s and eta-'s span loops again, as copies: through shared enumerators this kernel measured 1.5 % / 2.6 % slower
        // on cfg2 / cfg4 at the same 120 VGPRs)
        const int dlo = first ? 0 : (slo <= shi && slo < lo ? slo : lo);
        for (int f = dlo + tid; f <= hi; f += SMM_ALIGN_THREADS) {
            double st = 0.0, en = 0.0;
            if ((f >= slo && f <= shi) || (first && f == 0)) {
                const double hp = hmp[f], hq = hmq[f], eta = es[f];
                const int kmax = kw < T - f ? kw : T - f;
                const int k0 = lo - f > 1 ? lo - f : 1, k1 = hi - f < kmax ? hi - f : kmax;
                for (int k = k0; k <= k1; ++k)
                    st = st + agb_term((hp + s_lenp[k + SMM_ALIGN_R]) + qmp[f + k], (hq + s_lenq[k + SMM_ALIGN_R]) + qmq[f + k],
                                       eta + ee[f + k], lzp, lzq, val, kl);
            }
            if (f >= lo) {
                const double qp = qmp[f], qq = qmq[f], eta = ee[f];
                const int kmax = kw < f ? kw : f;
                const int k0 = f - shi > 1 ? f - shi : 1, k1 = f - slo < kmax ? f - slo : kmax;
                for (int k = k0; k <= k1; ++k)
                    en = en + agb_term((hmp[f - k] + s_lenp[k + SMM_ALIGN_R]) + qp, (hmq[f - k] + s_lenq[k + SMM_ALIGN_R]) + qq,
                                       es[f - k] + eta, lzp, lzq, val, kl);
                if (first && f <= kw)
                    en = en + agb_term((hmp[0] + s_lenp[f + SMM_ALIGN_R]) + qp, (hmq[0] + s_lenq[f + SMM_ALIGN_R]) + qq,
                                       es[0] + eta, lzp, lzq, val, kl);
            }
            dm[f] = st - en;
        }
        // ---- the video's part of g_len: thread k owns row k, the starts in order (0 first)
        const int kt = kw < T ? kw : T;
        for (int k = tid + 1; k <= kt && k < a.g.k_rows; k += SMM_ALIGN_THREADS) {
            const double lp = s_lenp[k + SMM_ALIGN_R], lq = s_lenq[k + SMM_ALIGN_R];
            const int s0 = slo > lo - k ? slo : lo - k, s1 = shi < hi - k ? shi : hi - k;
            double acc = 0.0;
            if (first && k >= lo && k <= hi)
                acc = acc + agb_term((hmp[0] + lp) + qmp[k], (hmq[0] + lq) + qmq[k], es[0] + ee[k], lzp, lzq, val, kl);
            for (int s = s0; s <= s1; ++s)
                acc = acc + agb_term((hmp[s] + lp) + qmp[s + k], (hmq[s] + lq) + qmq[s + k], es[s] + ee[s + k], lzp, lzq, val, kl);
            lpart[(size_t)k * cm + c] += acc;
        }
        __threadfence_block();
    }
    __syncthreads();

    // ---- the start nodes, in index order
    if (tid == 0)
        for (int m = 0; m < M; ++m)
            if (s_z[m]) {
                const size_t at = (size_t)m * T1;
                ipart[s_a[m]] += agb_term(x.p.h[at] + x.p.bh[at], x.q.h[at] + x.q.bh[at], x.ep_s[at], lzp, lzq, val, kl);
            }
}

// ---- g_elp of one video: thread j of a tile owns frame f0 + j and its row; per node one block scan of D over the tile on top
// of the node's running total.  Frames beside the video's, and the rows of a video that contributes nothing, keep the zeros
// of the call's zero fill; a video whose value is not finite gets NaN rows.
__global__ void __launch_bounds__(SMM_AGB_OCC_THREADS) smm_align_graph_entropy_bwd_occ_kernel(SmmAlignEntBwdArgs a)
{
    __shared__ double s_carry[SMM_MAX_TRANSCRIPT];
    __shared__ double s_wave[2][SMM_AGB_OCC_THREADS / 64];
    __shared__ int s_a[SMM_MAX_TRANSCRIPT];

    const int tid = threadIdx.x;
    const int vid = a.g.order[blockIdx.x];
    const AlignVideo v = align_video(a.g, vid);
    const AgbVideo x = agb_video(a, v, vid);
    const int T = v.T, cm = v.cm, C = v.C, M = v.M;
    const size_t T1 = v.T1;
    const double u = a.g.grad ? a.g.grad[vid] : 1.0;
    const double state = x.vals[1];
    double *g_elp = a.g.g_elp + (size_t)v.frame_off * cm;
    if (state == SMM_AGB_SKIP || u == 0.0) return;
    if (state == SMM_AGB_NAN) {
        for (int e = tid; e < T * cm; e += SMM_AGB_OCC_THREADS)
            if (e % cm < C) g_elp[e] = __builtin_nan("");
        return;
    }
    align_load_ids(a.g, v, s_a, tid, SMM_AGB_OCC_THREADS, [&](int m, bool) { s_carry[m] = 0.0; });
    __syncthreads();
    int set = 0;                                               // (two scans in a row never share their wave slots)
    for (int f0 = 0; f0 < T; f0 += SMM_AGB_OCC_THREADS) {
        const int t = f0 + tid;
        double *row = g_elp + (size_t)t * cm;
        for (int m = 0; m < M; ++m) {
            const GraphRange r = graph_range(x.rng, m);
            if (r.lo > r.hi) continue;
            const double e = (t < T && t >= r.dlo() && t <= r.hi) ? x.dd[(size_t)m * T1 + t] : 0.0;
            const double p = align_block_scan(e, s_carry[m], s_wave[set], tid);
            set ^= 1;
            if (tid == SMM_AGB_OCC_THREADS - 1) s_carry[m] = p;
            if (t < T) row[s_a[m]] += u * p;
        }
        __syncthreads();
    }
}

// g_len[g][k][c], g_trans[g][c][c'], g_init[g][c] = sum over the group's videos, in video order, of u_i * the video's part; a
// video whose value is not finite makes them NaN.  One thread per element: k_rows c_max of g_len, then c_max^2, then c_max.
__global__ void __launch_bounds__(256) smm_align_graph_entropy_bwd_reduce_kernel(SmmAlignEntBwdArgs a)
{
    const int cm = a.g.c_max, g = blockIdx.y;
    const int n_len = a.g.k_rows * cm, n_tab = cm * cm + cm;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_len + n_tab) return;
    const size_t pf = agb_part_doubles(cm, a.g.k_rows);
    double sum = 0.0;
    for (int i = 0; i < a.g.b; ++i) {
        if (a.g.videos[i].group != g) continue;
        const double *part = a.scratch + a.pv_base + (size_t)i * pf;
        const double u = a.g.grad ? a.g.grad[i] : 1.0;
        const double state = part[pf - 1];
        if (state == SMM_AGB_SKIP || u == 0.0) continue;
        sum = sum + (state == SMM_AGB_NAN ? __builtin_nan("") : u * part[e]);
    }
    if (e < n_len) a.g.g_len[(size_t)g * n_len + e] = sum;
    else if (e < n_len + cm * cm) a.g.g_trans[(size_t)g * cm * cm + (e - n_len)] = sum;
    else a.g.g_init[(size_t)g * cm + (e - n_len - cm * cm)] = sum;
}

size_t smm_align_graph_entropy_bwd_part_doubles(int c_max, int k_rows) { return agb_part_doubles(c_max, k_rows); }

void smm_launch_align_graph_entropy_bwd_check(const SmmAlignEntBwdArgs &a, const double *logz_q, double *out, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_graph_entropy_bwd_check_kernel, dim3((unsigned)a.g.b), dim3(SMM_ALIGN_THREADS), 0, stream, a, logz_q, out);
}

void smm_launch_align_graph_entropy_bwd(const SmmAlignEntBwdArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)a.g.b), block(SMM_ALIGN_THREADS);
    hipLaunchKernelGGL(smm_align_graph_eta_minus_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(smm_align_graph_eta_plus_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(smm_align_graph_entropy_bwd_kernel, grid, block, 0, stream, a);
    smm_launch_align_graph_entropy_bwd_tail(a, stream);
}

void smm_launch_align_graph_entropy_bwd_tail(const SmmAlignEntBwdArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_graph_entropy_bwd_occ_kernel, dim3((unsigned)a.g.b), dim3(SMM_AGB_OCC_THREADS), 0, stream, a);
    const unsigned cells = (unsigned)(a.g.k_rows * a.g.c_max + a.g.c_max * a.g.c_max + a.g.c_max);
    hipLaunchKernelGGL(smm_align_graph_entropy_bwd_reduce_kernel, dim3((cells + 255) / 256, (unsigned)a.g.n_groups),
                       dim3(256), 0, stream, a);
}
