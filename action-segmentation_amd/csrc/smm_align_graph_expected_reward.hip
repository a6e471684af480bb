// smm_align_graph_expected_reward.hip -- the expectation V = E[R(y)] of a reward that is additive over the frames and the nodes of
// an alignment under the transcript-graph posterior, and its gradient with respect to the tables (include/smmdp.h:
// smm_align_graph_expected_reward_f64, smm_align_graph_expected_reward_bwd_f64).  What smm_expected_reward.hip is to the
// unconstrained posterior, for this family; the decisions are smm_align_graph_entropy_bwd.hip's.
//
// Notation: smm_align_graph_logz.hip's (h, gam, q = cum + bg, bh, the five ints per column).
//   R(y) = sum over the segments (node j, start s, end n) of y of  r(j, s, n) = node_reward[j] + cumW[n][a_j] - cumW[s][a_j]
// with cumW[n][c] = sum_{t < n} reward[t][c], one prefix sum per video, class-major like cum.  The EOS step carries no reward.
//
// The value gathers (no recursion).  With smm_align_graph_segpost.hip's E[n][j] and S[s][j] (a segment of node j ends at n,
// starts at s), every segment contributes cumW at its end, minus cumW at its start, plus its node's reward:
//   V = sum_j ( sum_n E[n][j] cumW[n][a_j] - sum_s S[s][j] cumW[s][a_j] )  +  sum_j node_reward[j] sum_n E[n][j]
//
// The gradient is a Hessian-vector product of log Z_g.  An occurrence o is a span (node j, start s, end n = s + k), an edge
// (i -> j at s) or a start (node m at 0), w(o) its log-weight as smm_align_graph_entropy_bwd.hip lists them, p(o) = exp(w(o) - logZ_g):
//   dV / d theta = sum over the occurrences o that read the entry of  p(o) ( r(o) + eta-(S_o) + eta+(E_o) - V )
// r(o) = 0 for edges and starts.  eta- is the expected reward in front of a decision node, eta+ behind it, message passes over
// the sampler's decisions with p_loc the softmax of the weights:
//   eta-S(0, j) = 0;   eta-S(s, j) = sum_{i in pred(j)} p_loc(i) eta-E(s, i)                   weights gam[s][i] + trans[a_j][a_i]
//   eta-E(n, j) = sum_k p_loc(k) [ r(j, n-k, n) + eta-S(n-k, j) ]                              weights h[n-k][j] + len[k][a_j]
//   V-          = sum_{end(j)} p_loc(j) eta-E(T, j)                                            weights gam[T][j] + closing_j
//   eta+E(T, j) = 0;   eta+E(n, j) = sum_{m in succ(j)} p_loc(m) eta+S(n, m)                   weights trans[a_m][a_j] - cum[n][a_m] + bh[n][m]
//   eta+S(s, m) = sum_k p_loc(k) [ r(m, s, s+k) + eta+E(s+k, m) ]                              weights len[k][a_m] + q[s+k][m]
//   V+          = sum_{start(m)} p_loc(m) eta+S(0, m)                                          weights h[0][m] + bh[0][m]
// V- = V+ = V up to rounding, by independent decompositions.  One side, no logarithms: the candidates of a decision are read
// once, a maximum pass and a pass of fp64 exponentials; nothing is rescaled.
// The stored span-side values carry the prefix sum of their position -- eta-S(s, j) - cumW[s][a_j] in the eta-S block,
// eta+E(n, j) + cumW[n][a_j] in the eta+E block -- so a span's frame reward, a difference of two prefix sums, costs no load per
// candidate in the message passes and none in the assembly (smm_expected_reward.hip's fold).
//
// Work split.
//   prefix    one workgroup per video: where its cumW lies (the (T + 1) c_max doubles of every video in front of it), then
//             cumW, threads = (state, one of eight chunks of frames), two passes in a fixed order.  A non-finite reward in a
//             covered entry or on one of the video's nodes poisons the video's cumW with NaN and sets the error word.
//   value     one wave per (video, node) over the node's recorded range (smm_align_graph_segpost_nodes_kernel's shape):
//             lane-strided fp64 partials and a butterfly -> (frame part, node part) per node
//   sum       one wave per video: its nodes' partials, lane-strided in index order and a butterfly
//   eta-, eta+, assembly   one workgroup per video in the family's launch order, a column at a time, one position per thread:
//             smm_align_graph_entropy_bwd.hip's three kernels with one set of columns.  The assembly leaves D[f][j] (the span
//             terms that start at f minus those that end at f) and the video's parts of g_trans, g_init, g_len
//   then smm_align_graph_entropy_bwd_occ_kernel (g_elp as the running sum of D) and smm_align_graph_entropy_bwd_reduce_kernel
//   (the groups' tables) as they are: the scratch layout in front of cumW is SmmAlignEntBwdArgs'.
// Every read of a column is gated by its recorded range before the load; a decision without mass is not evaluated, a term of
// p(o) = 0 neither.  No atomics, no private segment, every sum in a fixed order: two calls give the same bits.
// A video whose log Z_g is not finite: NaN for its value and no contribution (the error word for a NaN or +inf).  A poisoned
// video: NaN for its value, its g_elp rows and its group's tables.
// Static LDS of the three column kernels: s_len 8.1 KB, s_tr 2 KB, eight int arrays 8 KB.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3
#include "smm_align_tile.h"
#include "smm_align_lse.h"
#include "smm_align_graph.h"

#define SMM_AGER_CHUNKS (SMM_ALIGN_THREADS / SMM_MAX_STATES_DEV)  // the prefix kernel's chunks of frames per state

// the columns, the scratch blocks (smm_align_graph.h; here em_s holds eta-S - cumW and ep_e eta+E + cumW), the prefix sums and
// the node rewards of one video
struct AgerVideo : GraphGradScratch {
    const int *rng;                                            // the columns' recorded ranges
    GraphCols<const double> p;
    const double *cw;                                          // cumW [C][T+1]
    const double *nr;                                          // the rewards of the video's nodes, or null
    const uint32_t *masks;
    double lz;
};

__device__ __forceinline__ AgerVideo ager_video(const SmmAlignExpRewardArgs &a, const AlignVideo &v, int vid)
{
    AgerVideo x;
    static_cast<GraphGradScratch &>(x) = graph_grad_scratch(a.e, v, vid);
    const int64_t ho = a.e.g.hoff[vid];
    x.rng = graph_rng(a.e.g.cols + ho);
    x.p = graph_cols<const double>(a.e.g.cols + ho, v.M, v.T1);
    x.cw = a.cumw + a.cw_off[vid];
    x.nr = a.node_reward ? a.node_reward + v.t0 : nullptr;
    x.masks = a.e.g.pred_mask + (size_t)v.t0 * SMM_GRAPH_WORDS;
    x.lz = a.e.g.logz[vid];
    return x;
}

// classes, flags and the ranges -> LDS, the masks stay in global memory; false where the structure is invalid.  Every thread
// calls it, once log Z_g is finite; its barriers are the caller's too.
__device__ __forceinline__ bool ager_load(const SmmAlignLogzArgs &g, const AlignVideo &v, const int *rng, const GraphNodes &s,
                                          int *s_flag, int tid)
{
    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    graph_load<false>(g, v, s.a, s.fl, nullptr, s_flag, tid);
    graph_load_ranges(rng, s, v.M, tid);
    __threadfence_block();
    __syncthreads();
    return s_flag[0] == 0;
}

// sum_c p_loc(c) eta(c) over the candidates cand(f) hands to f(w, eta or null: 0); 0 for a decision without mass
template <class Cand>
__device__ __forceinline__ double ager_decide(Cand cand)
{
    double mx = SMM_NEG_INF;
    cand([&](double w, const double *) { mx = align_max(mx, w); });
    if (align_nonfinite_bits(mx)) return 0.0;
    double z = 0.0, e = 0.0;
    cand([&](double w, const double *eta) {
        const double ew = exp(w - mx);
        z = z + ew;
        if (eta && ew > 0.0) e = e + ew * eta[0];
    });
    return e / z;
}

// p(o) ( cond - V ) of one occurrence: w = w(o), cond = r(o) + eta-(S_o) + eta+(E_o); 0 where p(o) = 0
__device__ __forceinline__ double ager_term(double w, double cond, double lz, double val)
{
    const double po = exp(w - lz);
    if (!(po > 0.0)) return 0.0;
    return po * (cond - val);
}

// the video of flat node index `node`: the last i with toff[i] <= node
__device__ __forceinline__ int ager_video_of(const int64_t *toff, int b, int64_t node)
{
    int lo = 0, hi = b - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (toff[mid] <= node) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------ prefix sums
__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_er_prefix_kernel(SmmAlignExpRewardArgs a)
{
    __shared__ double s_part[SMM_MAX_STATES_DEV][SMM_AGER_CHUNKS + 1];
    __shared__ double s_red[SMM_ALIGN_THREADS / 64];
    const int tid = threadIdx.x, vid = blockIdx.x;
    const AlignVideo v = align_video(a.e.g, vid);
    const int T = v.T, cm = v.cm, C = v.C < SMM_MAX_STATES_DEV ? v.C : SMM_MAX_STATES_DEV;
    // where the video's cumW lies: positions are counted exactly in fp64
    double cnt = 0.0;
    for (int i = tid; i < vid; i += SMM_ALIGN_THREADS) cnt = cnt + (double)(a.e.g.videos[i].T + 1);
    const int64_t off = (int64_t)graph_block_sum(cnt, s_red, tid) * cm;
    if (tid == 0) a.cw_off[vid] = off;
    double *cw = a.cumw + off;
    const int c = tid % SMM_MAX_STATES_DEV, j = tid / SMM_MAX_STATES_DEV;
    const int cs = (T + SMM_AGER_CHUNKS - 1) / SMM_AGER_CHUNKS;
    const int t0 = j * cs < T ? j * cs : T, t1 = t0 + cs < T ? t0 + cs : T;
    const bool act = c < C;
    const double *rw = a.reward ? a.reward + (size_t)v.frame_off * cm + c : nullptr;
    double sum = 0.0;
    int bad = 0;
    if (act && rw)
        for (int t = t0; t < t1; ++t) {
            const double r = rw[(size_t)t * cm];
            bad |= align_nonfinite_bits(r);
            sum = sum + r;
        }
    if (a.node_reward)
        for (int m = tid; m < v.M; m += SMM_ALIGN_THREADS) bad |= align_nonfinite_bits(a.node_reward[v.t0 + m]);
    s_part[c][j] = sum;
    bad = __syncthreads_or(bad);
    if (bad && tid == 0) a.e.g.err[0] = 1;
    if (!act) return;
    const double nan = __builtin_nan("");
    double run = 0.0;
    for (int q = 0; q < j; ++q) run = run + s_part[c][q];
    double *cwc = cw + (size_t)c * v.T1;
    for (int t = t0; t < t1; ++t) {
        cwc[t] = bad ? nan : run;
        if (rw) run = run + rw[(size_t)t * cm];
    }
    if (t0 < t1 && t1 == T) cwc[T] = bad ? nan : run;
}

// ------------------------------------------------------------------------------------------------ the value
__global__ void __launch_bounds__(256) smm_align_graph_er_value_kernel(SmmAlignExpRewardArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t node = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (node >= a.n_nodes) return;
    const int vid = ager_video_of(a.e.g.toff, a.e.g.b, node);
    const AlignVideo v = align_video(a.e.g, vid);
    const int m = (int)(node - v.t0);
    const double lz = a.e.g.logz[vid];
    const size_t T1 = v.T1;
    const double *cw = a.cumw + a.cw_off[vid];
    double fr = 0.0, nv = 0.0;
    if (align_nonfinite_bits(lz)) {                            // no alignment (-inf), or a log Z that is no number: NaN
        if (lane == 0 && align_bad_bits(lz)) a.e.g.err[0] = 1; // (staging cleared the word the forward call had set)
        fr = nv = __builtin_nan("");
    } else if (cw[0] != cw[0]) {                               // (a non-finite reward: the prefix kernel set the word)
        fr = nv = __builtin_nan("");
    } else {
        const double *block = a.e.g.cols + a.e.g.hoff[vid];
        const GraphCols<const double> p = graph_cols(block, v.M, T1);
        const GraphRange r = graph_range(graph_rng(block), m);
        const int c = a.e.g.transcript[v.t0 + m];              // (a finite logZ_g had a valid structure)
        const double *hm = p.h + (size_t)m * T1, *gm = p.g + (size_t)m * T1;
        const double *qm = p.q + (size_t)m * T1, *bhm = p.bh + (size_t)m * T1;
        const double *cumc = v.cum + (size_t)c * T1, *cwc = cw + (size_t)c * T1;
        if (r.lo <= r.hi) {
            double mass = 0.0;
            for (int n = r.lo + lane; n <= r.hi; n += 64) {
                const double pe = exp((gm[n] + (qm[n] - cumc[n])) - lz);
                mass = mass + pe;
                fr = fr + pe * cwc[n];
            }
            // (a start at 0 carries cumW[0] = 0)
            for (int s = r.slo + lane; s <= r.shi; s += 64) fr = fr - exp((hm[s] + bhm[s]) - lz) * cwc[s];
            fr = smm_group_sum<64>(fr);
            mass = smm_group_sum<64>(mass);
            if (a.node_reward) nv = a.node_reward[node] * mass;
        }
    }
    if (lane == 0) {
        a.partial[2 * node] = fr;
        a.partial[2 * node + 1] = nv;
    }
}

// one wave per video: the partials of its nodes, lane-strided in index order and a butterfly
__global__ void __launch_bounds__(256) smm_align_graph_er_sum_kernel(SmmAlignExpRewardArgs a)
{
    const int lane = threadIdx.x & 63;
    const int vid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (vid >= a.e.g.b) return;
    const int64_t t0 = a.e.g.toff[vid];
    const int M = (int)(a.e.g.toff[vid + 1] - t0);
    double fr = 0.0, nv = 0.0;
    for (int m = lane; m < M; m += 64) {
        fr = fr + a.partial[2 * (t0 + m)];
        nv = nv + a.partial[2 * (t0 + m) + 1];
    }
    fr = smm_group_sum<64>(fr);
    nv = smm_group_sum<64>(nv);
    if (lane == 0) {
        a.value[vid] = fr + nv;
        if (a.parts) {
            a.parts[2 * vid] = fr;
            a.parts[2 * vid + 1] = nv;
        }
    }
}

// ------------------------------------------------------------------------------------------------ eta-, V-, each video's state
__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_er_eta_minus_kernel(SmmAlignExpRewardArgs a)
{
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ double s_tr[SMM_MAX_TRANSCRIPT];                // trans[a_m][a_j], j = s_pl[i]
    GRAPH_SHARED_NODES;
    const int tid = threadIdx.x;
    const int vid = a.e.g.order[blockIdx.x];
    const AlignVideo v = align_video(a.e.g, vid);
    const AgerVideo x = ager_video(a, v, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const size_t T1 = v.T1;
    const bool none = align_nonfinite_bits(x.lz);
    const bool ok = !none && ager_load(a.e.g, v, x.rng, nd, s_flag, tid);
    const bool poisoned = ok && x.cw[0] != x.cw[0];            // (a non-finite reward: the prefix kernel set the word)
    if (!ok || poisoned) {
        if (tid == 0) {                                        // (no alignment: nothing to differentiate)
            if (align_bad_bits(x.lz) || (!none && !ok)) a.e.g.err[0] = 1;
            x.vals[0] = __builtin_nan("");
            x.vals[1] = poisoned ? SMM_AGB_NAN : SMM_AGB_SKIP;
            if (a.vpm) a.vpm[2 * vid] = __builtin_nan("");
        }
        return;
    }

    const int d_all = align_d_all(kw);
    for (int m = 0; m < M; ++m) {
        const GraphRange r = graph_range(nd, m);
        const int c = s_a[m];
        __syncthreads();                                       // the previous column's readers of s_len, s_pl, s_tr, s_w*
        if (r.lo > r.hi) continue;                             // a node without a cell
        const double *hm = x.p.h + (size_t)m * T1, *cwc = x.cw + (size_t)c * T1;
        double *es = x.em_s + (size_t)m * T1, *ee = x.em_e + (size_t)m * T1;
        const double nrm = x.nr ? x.nr[m] : 0.0;
        align_stage_len(v.len, cm, c, kw, d_all, s_len, tid);
        // ---- the node in front: pred(m) as the forward kernel lists it, one start s per thread
        const int np = graph_list<false>(x.masks, m, M, nd, tid, [&](int slot, int j) { s_tr[slot] = v.trans[(size_t)c * cm + s_a[j]]; });
        __syncthreads();
        for (int s = r.slo + tid; s <= r.shi; s += SMM_ALIGN_THREADS)
            es[s] = ager_decide([&](auto f) {
                graph_each_pred(nd, np, s, [&](int i, int j) {
                    const size_t at = (size_t)j * T1 + s;
                    f(x.p.g[at] + s_tr[i], x.em_e + at);
                });
            }) - cwc[s];
        if (r.z && tid == 0) es[0] = 0.0;                      // (cumW[0] = 0)
        __threadfence_block();
        __syncthreads();
        // ---- the start of the segment: the starts > 0 by rising k, then 0, which adds no eta
        for (int n = r.lo + tid; n <= r.hi; n += SMM_ALIGN_THREADS)
            ee[n] = (nrm + cwc[n]) + ager_decide([&](auto f) {
                const int kmax = kw < n ? kw : n;
                const int k0 = n - r.shi > 1 ? n - r.shi : 1, k1 = n - r.slo < kmax ? n - r.slo : kmax;
                for (int k = k0; k <= k1; ++k) f(hm[n - k] + s_len[k + SMM_ALIGN_R], es + (n - k));
                if (r.z && n <= kw) f(hm[0] + s_len[n + SMM_ALIGN_R], nullptr);
            });
        __threadfence_block();
    }
    __syncthreads();

    // ---- the end node
    if (tid == 0) {
        const double val = ager_decide([&](auto f) {
            graph_each_end(nd, M, T, [&](int j) {
                const size_t at = (size_t)j * T1 + T;
                f(x.p.g[at] + graph_closing(v.endpen, s_a[j]), x.em_e + at);
            });
        });
        if (val != val) a.e.g.err[0] = 1;                      // (a posterior that does not add up: not reached from finite logZ_g)
        if (a.vpm) a.vpm[2 * vid] = val;
        x.vals[0] = val;
        x.vals[1] = graph_grad_state(val);
    }
}

// ------------------------------------------------------------------------------------------------ eta+ and V+
__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_er_eta_plus_kernel(SmmAlignExpRewardArgs a)
{
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ double s_tr[SMM_MAX_TRANSCRIPT];                // trans[a_t][a_m], t = s_pl[i]
    GRAPH_SHARED_NODES;
    const int tid = threadIdx.x;
    const int vid = a.e.g.order[blockIdx.x];
    const AlignVideo v = align_video(a.e.g, vid);
    const AgerVideo x = ager_video(a, v, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const size_t T1 = v.T1;
    if (x.vals[1] != SMM_AGB_RUN) {                            // (nothing to walk: V+ is what the eta- kernel answered)
        if (tid == 0) {
            x.vplus[0] = x.vals[0];
            if (a.vpm) a.vpm[2 * vid + 1] = x.vals[0];
        }
        return;
    }
    ager_load(a.e.g, v, x.rng, nd, s_flag, tid);

    const int d_all = align_d_all(kw);
    for (int m = M - 1; m >= 0; --m) {
        const GraphRange r = graph_range(nd, m);
        const int c = s_a[m];
        __syncthreads();
        if (r.lo > r.hi) continue;
        const double *qm = x.p.q + (size_t)m * T1, *cwc = x.cw + (size_t)c * T1;
        double *es = x.ep_s + (size_t)m * T1, *ee = x.ep_e + (size_t)m * T1;
        const double nrm = x.nr ? x.nr[m] : 0.0;
        align_stage_len(v.len, cm, c, kw, d_all, s_len, tid);
        // ---- the node behind: succ(m) as the backward kernel lists it, one end n per thread
        const int np = graph_list<true>(x.masks, m, M, nd, tid, [&](int slot, int t) { s_tr[slot] = v.trans[(size_t)s_a[t] * cm + c]; });
        __syncthreads();
        for (int n = r.lo + tid; n <= r.hi; n += SMM_ALIGN_THREADS)
            ee[n] = (n == T ? 0.0 : ager_decide([&](auto f) {
                for (int i = 0; i < np; ++i) {
                    const int t = s_pl[i];
                    if (n >= s_slo[t] && n <= s_shi[t]) {
                        const size_t at = (size_t)t * T1 + n, cu = (size_t)s_a[t] * T1 + n;
                        f((s_tr[i] - v.cum[cu]) + x.p.bh[at], x.ep_s + at);
                    }
                }
            })) + cwc[n];
        __threadfence_block();
        __syncthreads();
        // ---- the end of the segment
        const int smin = r.z ? 0 : r.slo;
        for (int s = smin + tid; s <= r.shi; s += SMM_ALIGN_THREADS) {
            if (s != 0 && s < r.slo) continue;                 // (between an h[0] and the column's other starts)
            es[s] = (nrm - cwc[s]) + ager_decide([&](auto f) {
                const int kmax = kw < T - s ? kw : T - s;
                const int k0 = r.lo - s > 1 ? r.lo - s : 1, k1 = r.hi - s < kmax ? r.hi - s : kmax;
                for (int k = k0; k <= k1; ++k) f(s_len[k + SMM_ALIGN_R] + qm[s + k], ee + (s + k));
            });
        }
        __threadfence_block();
    }
    __syncthreads();

    // ---- the start node: the start nodes that have cells, in index order
    if (tid == 0) {
        const double val = ager_decide([&](auto f) {
            for (int m = 0; m < M; ++m)
                if (s_z[m]) {
                    const size_t at = (size_t)m * T1;
                    f(x.p.h[at] + x.p.bh[at], x.ep_s + at);
                }
        });
        x.vplus[0] = val;
        if (a.vpm) a.vpm[2 * vid + 1] = val;
    }
}

// ------------------------------------------------------------------------------------------------ assembly
// the video's parts of g_trans, g_init and g_len, and D
__global__ void __launch_bounds__(SMM_ALIGN_THREADS) smm_align_graph_er_bwd_kernel(SmmAlignExpRewardArgs a)
{
    __shared__ double s_len[SMM_ALIGN_LEN];
    __shared__ double s_tr[SMM_MAX_TRANSCRIPT];                // trans[a_m][a_j], j = s_pl[i]
    __shared__ double s_red[SMM_ALIGN_THREADS / 64];
    GRAPH_SHARED_NODES;
    const int tid = threadIdx.x;
    const int vid = a.e.g.order[blockIdx.x];
    const AlignVideo v = align_video(a.e.g, vid);
    const AgerVideo x = ager_video(a, v, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M, k_rows = a.e.g.k_rows;
    const size_t T1 = v.T1;
    if (x.vals[1] != SMM_AGB_RUN) return;
    const double val = x.vals[0], lz = x.lz;
    double *lpart = x.part, *tpart = x.part + (size_t)k_rows * cm, *ipart = tpart + (size_t)cm * cm;
    for (int e = tid; e < k_rows * cm + cm * cm + cm; e += SMM_ALIGN_THREADS) lpart[e] = 0.0;
    ager_load(a.e.g, v, x.rng, nd, s_flag, tid);               // (its barriers: the zeros before the sums)

    const int d_all = align_d_all(kw);
    for (int m = 0; m < M; ++m) {
        const GraphRange r = graph_range(nd, m);
        const int lo = r.lo, hi = r.hi, slo = r.slo, shi = r.shi;
        const bool first = r.z != 0;
        const int c = s_a[m];
        __syncthreads();
        if (lo > hi) continue;
        const size_t col = (size_t)m * T1;
        const double *hm = x.p.h + col, *qm = x.p.q + col, *bhm = x.p.bh + col, *cumc = v.cum + (size_t)c * T1;
        const double *es = x.em_s + col, *ee = x.ep_e + col, *ps = x.ep_s + col;   // (the prefix sums are inside es and ee)
        double *dm = x.dd + col;
        const double nrm = x.nr ? x.nr[m] : 0.0;
        align_stage_len(v.len, cm, c, kw, d_all, s_len, tid);
        const int np = graph_list<false>(x.masks, m, M, nd, tid, [&](int slot, int j) { s_tr[slot] = v.trans[(size_t)c * cm + s_a[j]]; });
        __syncthreads();
        // ---- the edges into m: one block sum each, in the list's order
        for (int i = 0; i < np; ++i) {
            const int j = s_pl[i];
            const int e0 = slo > s_lo[j] ? slo : s_lo[j], e1 = shi < s_hi[j] ? shi : s_hi[j];
            const double tr = s_tr[i];
            double acc = 0.0;
            for (int s = e0 + tid; s <= e1; s += SMM_ALIGN_THREADS) {
                const size_t at = (size_t)j * T1 + s;
                acc = acc + ager_term(x.p.g[at] + ((tr - cumc[s]) + bhm[s]), x.em_e[at] + ps[s], lz, val);
            }
            const double tot = graph_block_sum(acc, s_red, tid);
            if (tid == 0) tpart[(size_t)c * cm + s_a[j]] += tot;
        }
        // ---- D[f][m]: the span terms that start at f minus those that end at f
        const int dlo = r.dlo();
        for (int f = dlo + tid; f <= hi; f += SMM_ALIGN_THREADS) {
            double st = 0.0, en = 0.0;
            if ((f >= slo && f <= shi) || (first && f == 0)) {
                const double hv = hm[f], eta = nrm + es[f];
                const int kmax = kw < T - f ? kw : T - f;
                const int k0 = lo - f > 1 ? lo - f : 1, k1 = hi - f < kmax ? hi - f : kmax;
                for (int k = k0; k <= k1; ++k) st = st + ager_term((hv + s_len[k + SMM_ALIGN_R]) + qm[f + k], eta + ee[f + k], lz, val);
            }
            if (f >= lo) {
                const double qv = qm[f], eta = nrm + ee[f];
                const int kmax = kw < f ? kw : f;
                const int k0 = f - shi > 1 ? f - shi : 1, k1 = f - slo < kmax ? f - slo : kmax;
                for (int k = k0; k <= k1; ++k) en = en + ager_term((hm[f - k] + s_len[k + SMM_ALIGN_R]) + qv, es[f - k] + eta, lz, val);
                if (first && f <= kw) en = en + ager_term((hm[0] + s_len[f + SMM_ALIGN_R]) + qv, es[0] + eta, lz, val);
            }
            dm[f] = st - en;
        }
        // ---- the video's part of g_len: thread k owns row k, the starts in order (0 first)
        const int kt = kw < T ? kw : T;
        for (int k = tid + 1; k <= kt && k < k_rows; k += SMM_ALIGN_THREADS) {
            const double lk = s_len[k + SMM_ALIGN_R];
            const int s0 = slo > lo - k ? slo : lo - k, s1 = shi < hi - k ? shi : hi - k;
            double acc = 0.0;
            if (first && k >= lo && k <= hi) acc = acc + ager_term((hm[0] + lk) + qm[k], (nrm + es[0]) + ee[k], lz, val);
            for (int s = s0; s <= s1; ++s) acc = acc + ager_term((hm[s] + lk) + qm[s + k], (nrm + es[s]) + ee[s + k], lz, val);
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
                ipart[s_a[m]] += ager_term(x.p.h[at] + x.p.bh[at], x.ep_s[at], lz, val);
            }
}

void smm_launch_align_graph_expected_reward(const SmmAlignExpRewardArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_align_graph_er_prefix_kernel, dim3((unsigned)a.e.g.b), dim3(SMM_ALIGN_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_align_graph_er_value_kernel, dim3((unsigned)((a.n_nodes + 3) / 4)), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(smm_align_graph_er_sum_kernel, dim3((unsigned)((a.e.g.b + 3) / 4)), dim3(256), 0, stream, a);
}

void smm_launch_align_graph_expected_reward_bwd(const SmmAlignExpRewardArgs &a, hipStream_t stream)
{
    const dim3 grid((unsigned)a.e.g.b), block(SMM_ALIGN_THREADS);
    hipLaunchKernelGGL(smm_align_graph_er_prefix_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(smm_align_graph_er_eta_minus_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(smm_align_graph_er_eta_plus_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(smm_align_graph_er_bwd_kernel, grid, block, 0, stream, a);
    smm_launch_align_graph_entropy_bwd_tail(a.e, stream);
}
