// smm_align_graph_segpost.hip -- the posterior of each segment of given alignments under the transcript-graph posterior, and
// where each node's segment starts and ends (include/smmdp.h: smm_align_graph_segment_posteriors_f64): forward by
// smm_align_graph_logz_fwd_kernel, the q and bh columns by smm_align_graph_logz_bwd_kernel, gathers here.
//
// With smm_align_graph_entropy.hip's E and S, the posteriors of "a segment of node m ends at n" and "... starts at s",
//   E[n][m] = exp(gam[n][m] + (q[n][m] - cum[n][a_m]) - logZ_g),  n in [lo_m, hi_m]
//   S[s][m] = exp(h[s][m] + bh[s][m] - logZ_g),                   s in [slo_m, shi_m] and, when z_m, s = 0
// and, from gam = cum + LSE(h + len), the posterior that node m covers exactly the frames [s, e):
//   P(m on [s, e)) = exp(h[s][m] + len[e-s][a_m] + q[e][m] - logZ_g),   1 <= e - s <= kw.
// Everything outside a column's recorded range is uninitialised memory: every load is gated by the range BEFORE it, as in the
// sampler; a cell outside the range has probability 0.
//
//   smm_align_graph_segpost_nodes_kernel  one wave per (video, node) over the node's range: the dense rows E[.][m] and S[.][m]
//       (0.0 outside the range), and mean and standard deviation of the end and the start position given that the path
//       crosses m: mass and first moment in one pass, the variance about the mean in a second one, lane-strided partial sums
//       and a butterfly, all in fp64.  Bounded by the column loads: four doubles per cell and pass.
//   smm_align_graph_segpost_sets_kernel   one wave per (set, video).  The used nodes are listed in index order by ballots over
//       64 nodes at a time; the span starts are found by ballots over 64 positions at a time and matched to the list by prefix
//       counts; a start finds its end by a forward scan over at most kw + 1 positions.  A first pass finds what makes the
//       alignment impossible (the counts differ, a class is not its node's, a span is longer than kw): such a (set, video) is
//       -inf everywhere.  Bounded by the reads of the span rows, twice.
// No atomics, and only the error word is written beside the outputs; every sum is in a fixed order.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3
#include "smm_align_tile.h"
#include "smm_align_graph.h"

// the video of flat node index `node`: the last i with toff[i] <= node
__device__ __forceinline__ int agsp_video_of(const int64_t *toff, int b, int64_t node)
{
    int lo = 0, hi = b - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (toff[mid] <= node) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// mean and standard deviation of the position under the weights w(n), n = lo .. hi (and, with `zero`, n = 0): all 64 lanes call
// it; NaN where the mass is 0.  row (or null): the dense row, which gets w(n) on the range
template <class W>
__device__ __forceinline__ void agsp_moments(int lo, int hi, bool zero, int lane, W w, double *row, double *mean_out, double *sd_out)
{
    double mass = 0.0, m1 = 0.0;
    if (zero && lane == 0) {
        const double e = w(0);
        mass = e;                                              // (position 0 adds nothing to the first moment)
        if (row) row[0] = e;
    }
    for (int n = (lo & ~63) + lane; n <= hi; n += 64) {        // lane n & 63 owns cell n of the row, as in the caller's fill
        if (n < lo) continue;
        const double e = w(n);
        mass += e;
        m1 += e * (double)n;
        if (row) row[n] = e;
    }
    mass = smm_group_sum<64>(mass);
    m1 = smm_group_sum<64>(m1);
    const double mean = m1 / mass;
    double var = 0.0;
    if (zero && lane == 0) var = w(0) * mean * mean;
    for (int n = (lo & ~63) + lane; n <= hi; n += 64) {
        if (n < lo) continue;
        const double d = (double)n - mean;
        var += w(n) * d * d;
    }
    var = smm_group_sum<64>(var);
    if (lane == 0) {
        const bool ok = mass > 0.0;
        if (mean_out) *mean_out = ok ? mean : __builtin_nan("");
        if (sd_out) *sd_out = ok ? sqrt(var / mass) : __builtin_nan("");
    }
}

__global__ void __launch_bounds__(256) smm_align_graph_segpost_nodes_kernel(SmmAlignSegPostArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t node = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (node >= a.n_nodes) return;
    const int vid = agsp_video_of(a.g.toff, a.g.b, node);
    const AlignVideo v = align_video(a.g, vid);
    const int m = (int)(node - v.t0), T = v.T;
    const double lz = a.g.logz[vid];
    const size_t T1 = v.T1, W = (size_t)a.t_max + 1;
    double *erow = a.node_end_post ? a.node_end_post + (size_t)node * W : nullptr;
    double *srow = a.node_start_post ? a.node_start_post + (size_t)node * W : nullptr;
    if (align_nonfinite_bits(lz)) {                            // no alignment (-inf), or a log Z that is no number: NaN
        const double nan = __builtin_nan("");
        if (lane == 0) {
            if (align_bad_bits(lz)) a.g.err[0] = 1;            // (staging cleared the word the forward call had set)
            if (a.end_mean) a.end_mean[node] = nan;
            if (a.end_sd) a.end_sd[node] = nan;
            if (a.start_mean) a.start_mean[node] = nan;
            if (a.start_sd) a.start_sd[node] = nan;
        }
        for (size_t n = lane; n < W; n += 64) {
            if (erow) erow[n] = n <= (size_t)T ? nan : 0.0;
            if (srow) srow[n] = n <= (size_t)T ? nan : 0.0;
        }
        return;
    }
    const double *block = a.g.cols + a.g.hoff[vid];
    const GraphCols<const double> p = graph_cols(block, v.M, T1);
    const GraphRange r = graph_range(graph_rng(block), m);
    const int c = a.g.transcript[v.t0 + m];                    // (a finite logZ_g had a valid structure)
    const double *hm = p.h + (size_t)m * T1, *gm = p.g + (size_t)m * T1;
    const double *qm = p.q + (size_t)m * T1, *bhm = p.bh + (size_t)m * T1;
    const double *cumc = v.cum + (size_t)c * T1;
    // the dense rows outside the ranges; a lane's zero and its value of the same cell are stores of one thread, in order
    for (size_t n = lane; n < W; n += 64) {
        if (erow) erow[n] = 0.0;
        if (srow) srow[n] = 0.0;
    }
    const bool has = r.lo <= r.hi;
    agsp_moments(has ? r.lo : 1, has ? r.hi : 0, false, lane,
                 [&](int n) { return exp((gm[n] + (qm[n] - cumc[n])) - lz); }, erow,
                 a.end_mean ? a.end_mean + node : nullptr, a.end_sd ? a.end_sd + node : nullptr);
    const bool hs = has && r.slo <= r.shi;
    const bool zero = has && r.z != 0 && !(hs && r.slo == 0);
    // (lane 0 owns cell 0 of the row: its zero above and its value are one thread's stores)
    agsp_moments(hs ? r.slo : 1, hs ? r.shi : 0, zero, lane, [&](int s) { return exp((hm[s] + bhm[s]) - lz); }, srow,
                 a.start_mean ? a.start_mean + node : nullptr, a.start_sd ? a.start_sd + node : nullptr);
}

// local state of a global class id (the video's class-map row, in index order); -1 when the id is not in the set
__device__ __forceinline__ int agsp_local(const int64_t *cmap, int C, int64_t id)
{
    if (!cmap) return (id >= 0 && id < C) ? (int)id : -1;
    for (int c = 0; c < C; ++c)
        if (cmap[c] == id) return c;
    return -1;
}

__global__ void __launch_bounds__(64) smm_align_graph_segpost_sets_kernel(SmmAlignSegPostArgs a)
{
    __shared__ int s_node[SMM_MAX_TRANSCRIPT];                 // the used nodes in index order
    const int lane = threadIdx.x;
    const int set = blockIdx.x / a.g.b, vid = blockIdx.x - set * a.g.b;
    const AlignVideo v = align_video(a.g, vid);
    const int T = v.T, M = v.M, kw = v.kw;
    const size_t W = (size_t)a.t_max + 1;
    const int64_t *sp = a.spans_in + ((size_t)set * a.g.b + vid) * W;
    const int32_t *us = a.used_in + (size_t)set * a.n_nodes + v.t0;
    double *seg = a.seg_logp ? a.seg_logp + ((size_t)set * a.g.b + vid) * W : nullptr;
    double *nlp = a.node_logp ? a.node_logp + (size_t)set * a.n_nodes + v.t0 : nullptr;
    const double lz = a.g.logz[vid];
    if (align_nonfinite_bits(lz)) {                            // no alignment (-inf), or a log Z that is no number: NaN
        if (lane == 0 && align_bad_bits(lz)) a.g.err[0] = 1;
        if (seg)
            for (size_t q = lane; q < W; q += 64) seg[q] = q <= (size_t)T ? __builtin_nan("") : SMM_NEG_INF;
        if (nlp)
            for (int m = lane; m < M; m += 64) nlp[m] = __builtin_nan("");
        return;
    }
    // ---- the used nodes, in index order
    int n_used = 0;
    for (int m0 = 0; m0 < M; m0 += 64) {
        const int m = m0 + lane;
        const bool is = m < M && us[m] != 0;
        const unsigned long long ballot = __ballot(is);
        if (is) s_node[n_used + graph_rank(ballot, lane)] = m;
        n_used += __popcll(ballot);
    }
    __syncthreads();
    const double *block = a.g.cols + a.g.hoff[vid];
    const GraphCols<const double> p = graph_cols(block, M, v.T1);
    const int *rng = graph_rng(block);
    const int64_t *cmap = a.class_map ? a.class_map + (size_t)v.g * (v.cm + 1) : nullptr;
    // ---- two passes over the span row: what makes the alignment impossible, then the values
    bool fault = false;
    for (int pass = 0; pass < 2; ++pass) {
        int k0 = 0;                                            // span starts in front of this chunk
        for (int q0 = 0; q0 <= a.t_max; q0 += 64) {
            const int q = q0 + lane;
            const bool is = q < T && sp[q] != -1;
            const unsigned long long ballot = __ballot(is);
            const int k = k0 + graph_rank(ballot, lane);
            k0 += __popcll(ballot);
            double out = SMM_NEG_INF;
            if (is && k < n_used) {
                int e = 0;                                     // the next position that is no continuation, at most kw + 1 on
                for (int j = 1; j <= kw + 1 && q + j <= T; ++j)
                    if (sp[q + j] != -1) { e = q + j; break; }
                const int m = s_node[k];
                const int c = a.g.transcript[v.t0 + m];
                if (pass == 0) {
                    fault |= e == 0 || e - q > kw || agsp_local(cmap, v.C, sp[q]) != c;
                } else if (!fault) {
                    const GraphRange r = graph_range(rng, m);
                    const bool hs = (q >= r.slo && q <= r.shi) || (r.z != 0 && q == 0);
                    if (r.lo <= r.hi && hs && e >= r.lo && e <= r.hi)
                        out = p.h[(size_t)m * v.T1 + q] + v.len[(size_t)(e - q) * v.cm + c] + p.q[(size_t)m * v.T1 + e] - lz;
                    if (nlp) nlp[m] = out;
                }
            }
            if (pass == 1 && seg && q <= a.t_max) seg[q] = (q == T && !fault) ? 0.0 : out;
        }
        if (pass == 0) fault = __any(fault) || k0 != n_used;
    }
    // the nodes no span stands for (under a fault: every node)
    if (nlp)
        for (int m = lane; m < M; m += 64)
            if (fault || us[m] == 0) nlp[m] = SMM_NEG_INF;
}

void smm_launch_align_graph_segpost(const SmmAlignSegPostArgs &a, hipStream_t stream)
{
    if (a.end_mean || a.end_sd || a.start_mean || a.start_sd || a.node_end_post || a.node_start_post)
        hipLaunchKernelGGL(smm_align_graph_segpost_nodes_kernel, dim3((unsigned)((a.n_nodes + 3) / 4)), dim3(256), 0, stream, a);
    if (a.seg_logp || a.node_logp)
        hipLaunchKernelGGL(smm_align_graph_segpost_sets_kernel, dim3((unsigned)a.g.b * (unsigned)a.n_sets), dim3(64), 0, stream, a);
}
