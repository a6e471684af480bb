// smm_expected_reward.hip -- the posterior expectation V = E_p[R(y)] of a reward that is additive over the frames and segments of
// a segmentation, and its gradient with respect to p's factor tables (elp, trans, init, len).
//
//   R(y) = sum over the spans (s, k, c) of y of r(s, k, c),   r(s, k, c) = seg_reward[c] + cumW[s + k][c] - cumW[s][c]
// with cumW[n][c] = sum_{t < n} reward[t][c], one prefix sum per video.  Without EOS the closing label `to` of frame T counts as
// a one-frame span (smm_segpost.hip's convention): it carries reward[T][to] + seg_reward[to], and row T is not part of cumW.
//
// The value gathers (no recursion).  With the node probabilities of smm_posterior.h,
//   V = sum_{n, c} P(end (n, c)) cumW[n][c] - P(start (n, c)) cumW[n][c] + P(start (n, c)) seg_reward[c]   (+ the closing label)
// because every span contributes cumW at its end, minus cumW at its start, plus seg_reward at its start.
//
// The gradient is a Hessian-vector product of log Z: dV / d theta_o = Cov_p(R, phi_o) for every occurrence o (a span, a
// transition at a boundary, the initial class, without EOS the closing transition).  Given o, the part of y in front of o
// depends on o only through the decision node S it starts from and the part behind only through the node E it ends in (the
// lattice is Markov in its decision nodes), so E[R | o] = r(o) + eta-(S) + eta+(E) and
//   Cov_p(R, phi_o) = p(o) * ( r(o) + eta-(S_o) + eta+(E_o) - V )
//   eta-(end (n, c))   = sum_k  p(k | end (n, c))    [ r(n - k, k, c) + eta-(start (n - k, c)) ]
//   eta-(start (s, c)) = sum_c' p(c' | start (s, c))  eta-(end (s, c')),          eta-(start (0, c)) = 0
// with the local distributions of smm_sample.hip's backward walk (smm_entropy.hip's header lists them) and eta+ the same
// recursion on the time-reversed histories; its boundary is 0 with EOS and, without, the closing label's reward averaged over
// p(to | end (T, c)).  r(o) = 0 for a transition and the initial class; the closing transition from -> to carries the closing
// label's reward.  The last decision of each direction closes the sum: V- (the sampler's final decision) and V+ (the initial
// class) are both V, by independent decompositions.  What smm_entropy_bwd.hip does for s_q, with one side, no logarithms and
// O(1) rewards in place of 1e6-nat scores.
//
// Work split.
//   smm_er_prefix_kernel   one workgroup per video: cumW, threads = (state, chunk of frames), two passes in a fixed order
//                          (smm_ebwd_elp_kernel's pattern).  A non-finite reward in a covered entry poisons the video's cumW
//                          with NaN and sets the error word.  cumW lives in the video's second scratch row block (hT1 of
//                          smm_logz_bwd.hip), the value's slab partials in the first (smm_entropy.hip's place).
//   smm_expected_reward_kernel   grid (video, slab of SMM_POST_SLAB positions), thread = node (n, c), c fastest
//                          (smm_segpost_dense_kernel's split): six history loads, one cumW load, two fp64 exp per node; one
//                          (frame part, segment part) pair of fp64 partials per workgroup, summed per video in a fixed order
//                          by smm_er_sum_kernel.  Bounded by the history loads.
//   smm_er_eta_kernel, smm_er_nodes_kernel, smm_er_pairs_kernel, smm_er_len_kernel   smm_posterior_grad.h's skeletons (the
//                          work split is described there) under this file's policy: one side, an expectation per decision
//                          (smm_er_decide: maxima, then fp64 exponentials and sums, nothing rescaled).  The start-node values
//                          the walk stores carry the prefix sum of their position (eta- - cumW, eta+ + cumW): a span's frame
//                          reward then costs no load per candidate, and none in the assembly.
//   then smm_ebwd_elp_kernel (g_elp = running sum of D over t, x the upstream gradient) and smm_ebwd_group_kernel (the
//   per-video tables summed over each group's videos in video order) as they are: the scratch layout is SmmEntBwdArgs'.
// No atomics but the error word: the results are bit-identical run to run.  A video whose log Z is not finite, or with a
// non-finite reward in a covered entry, gets NaN for its value, its g_elp rows and its group's tables.
#include "smm_posterior_grad.h"
#include "../../include/smmdp.h"

#define SMM_ER_VAL_THREADS 256

__device__ __forceinline__ bool smm_er_finite(double x) { return x > SMM_NEG_INF && x < -SMM_NEG_INF; }

// exp of a log-probability: 0 for -inf, NaN for NaN
__device__ __forceinline__ double smm_er_p(double lp) { return lp == SMM_NEG_INF ? 0.0 : exp(lp); }

// the video's cumW [T+1][c_max]: the second scratch row block of its histories
__device__ __forceinline__ double *smm_er_cum(const SmmExpRewardArgs &a, const SmmVideo &mv, int cm, int T)
{
    return smm_hist(a.e.p.hist, mv, cm, T).scratch + (size_t)cm * (T + 1);
}

// reward of the closing label `to` of frame T (no EOS): its frame and its segment
__device__ __forceinline__ double smm_er_close_frame(const SmmExpRewardArgs &a, const SmmVideo &mv, int cm, int T, int to)
{
    return a.reward ? a.reward[(size_t)(mv.frame_off + T) * cm + to] : 0.0;
}
__device__ __forceinline__ double smm_er_seg(const SmmExpRewardArgs &a, int g, int cm, int c)
{
    return a.seg_reward ? a.seg_reward[(size_t)g * cm + c] : 0.0;
}

// ------------------------------------------------------------------------------------------------ prefix sums
__global__ void __launch_bounds__(1024) smm_er_prefix_kernel(SmmExpRewardArgs a)
{
    __shared__ double part[32][33];
    const int vid = blockIdx.x;
    const SmmVideo mv = a.e.h.videos[vid];
    const int T = mv.T - a.e.h.no_eos, g = mv.group, cm = a.e.h.c_max;
    const int C = a.e.h.n_states[g];
    if (T <= 0 || C <= 0) return;
    double *cw = smm_er_cum(a, mv, cm, T);
    const int tid = threadIdx.x, c = tid & 31, j = tid >> 5, nj = blockDim.x >> 5;
    const int cs = (T + nj - 1) / nj;
    const int t0 = j * cs, t1 = (t0 + cs < T) ? t0 + cs : T;
    const bool act = c < C, col = c < cm;
    const double *rw = a.reward ? a.reward + (size_t)mv.frame_off * cm + c : nullptr;
    double sum = 0.0;
    int bad = 0;
    if (act && rw)
        for (int t = t0; t < t1; ++t) {
            const double r = rw[(size_t)t * cm];
            bad |= !smm_er_finite(r);
            sum += r;
        }
    if (act && j == 0) {
        if (a.seg_reward) bad |= !smm_er_finite(a.seg_reward[(size_t)g * cm + c]);
        if (a.e.h.no_eos && rw) bad |= !smm_er_finite(rw[(size_t)T * cm]);
    }
    part[c][j] = sum;
    bad = __syncthreads_or(bad);
    if (bad && tid == 0) atomicExch(a.e.h.err, 1);
    if (!col) return;
    const double nan = __builtin_nan("");
    double run = 0.0;
    if (act)
        for (int q = 0; q < j; ++q) run += part[c][q];
    for (int t = t0; t < t1; ++t) {
        cw[(size_t)t * cm + c] = bad ? nan : run;
        if (act && rw) run += rw[(size_t)t * cm];
    }
    if (t0 < t1 && t1 == T) cw[(size_t)T * cm + c] = bad ? nan : run;
}

// ------------------------------------------------------------------------------------------------ the value
__global__ void __launch_bounds__(SMM_ER_VAL_THREADS) smm_expected_reward_kernel(SmmExpRewardArgs a)
{
    __shared__ double s_part[2][SMM_ER_VAL_THREADS / 64];
    const int vid = blockIdx.x, y = blockIdx.y;
    const SmmVideo mv = a.e.h.videos[vid];
    const int T = mv.T - a.e.h.no_eos, g = mv.group, cm = a.e.h.c_max;
    const int C = a.e.h.n_states[g];
    if (T <= 0 || C <= 0) return;                       // (the reduction flags it)
    const int n0 = y * SMM_POST_SLAB;
    if (n0 > T) return;                                 // positions 0 .. T
    const SmmHist H = smm_hist(a.e.p.hist, mv, cm, T);  // (scratch: [2][n_slabs] partials, then cumW)
    const double *cw = smm_er_cum(a, mv, cm, T);
    const double lz = a.e.p.logz[vid];
    const int tid = threadIdx.x;
    double fr = 0.0, sg = 0.0;
    if (smm_er_finite(lz)) {
        const int nodes = (smm_post_slab_end(n0, T) - n0) * cm;
        for (int i = tid; i < nodes; i += SMM_ER_VAL_THREADS) {
            const int dn = i / cm, c = i - dn * cm, n = n0 + dn;
            if (c >= C) continue;
            const double w = cw[(size_t)n * cm + c];
            const double pe = n >= 1 ? smm_er_p(smm_post_lp_end(H, T, cm, n, c, lz)) : 0.0;
            const double ps = n < T ? smm_er_p(smm_post_lp_start(H, T, cm, n, c, lz)) : 0.0;
            fr += pe * w - ps * w;
            sg += ps * smm_er_seg(a, g, cm, c);
        }
        // slab 0: without EOS the closing label of frame T (wave 0, lane = to)
        if (y == 0 && tid < C && a.e.h.no_eos) {
            const double pt = smm_er_p(smm_post_final_weight(a.e.h, a.e.p, mv, vid, T, C, H.F.g + (size_t)T * cm, tid) - lz);
            fr += pt * smm_er_close_frame(a, mv, cm, T, tid);
            sg += pt * smm_er_seg(a, g, cm, tid);
        }
    } else {
        fr = sg = __builtin_nan("");
    }
    smm_post_block_sum(fr, sg, s_part, H.scratch, smm_post_slabs(T), y);
}

// one wave per video: the partials of its slabs in a fixed order; NaN (and the error word) for anything not finite
__global__ void __launch_bounds__(256) smm_er_sum_kernel(SmmExpRewardArgs a)
{
    const int lane = threadIdx.x & 63;
    const int vid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (vid >= a.e.h.b) return;
    const SmmVideo mv = a.e.h.videos[vid];
    const int T = mv.T - a.e.h.no_eos;
    double v[2] = {__builtin_nan(""), __builtin_nan("")};
    if (T > 0 && a.e.h.n_states[mv.group] > 0)
        smm_post_video_sum(smm_hist(a.e.p.hist, mv, a.e.h.c_max, T).scratch, smm_post_slabs(T), lane, v);
    if (lane == 0) {
        const double t = v[0] + v[1];
        const bool ok = smm_er_finite(t);
        if (!ok) atomicExch(a.e.h.err, 1);
        a.value[vid] = ok ? t : __builtin_nan("");
        if (a.parts) {
            a.parts[2 * vid] = ok ? v[0] : __builtin_nan("");
            a.parts[2 * vid + 1] = ok ? v[1] : __builtin_nan("");
        }
    }
}

// ------------------------------------------------------------------------------------------------ the serial pass
// One decision shared by the W lanes of a group: E[x] under the distribution exp(w(i)) over the candidates i = i0, i0 + step, ..
// < n of this lane.  Every lane of the group must call it (butterflies); the result is group-uniform.  0 for a node without a
// finite candidate (it is never weighed), NaN for a NaN or +inf weight.  A candidate of probability 0 does not read its x.
template <int W, class Wf, class Xf>
__device__ double smm_er_decide(int i0, int n, int step, Wf w, Xf x)
{
    double m = SMM_NEG_INF;
    int nan = 0;
    for (int i = i0; i < n; i += step) {
        const double wi = w(i);
        nan |= (wi != wi) | (wi == -SMM_NEG_INF);
        m = fmax(m, wi);
    }
    m = smm_group_max<W>(m);
    nan = smm_group_or<W>(nan);
    double s = 0.0, acc = 0.0;
    if (!nan && m > SMM_NEG_INF) {
        for (int i = i0; i < n; i += step) {
            const double d = w(i) - m;
            const double e = (d > SMM_NEG_INF) ? exp(d) : 0.0;
            if (e > 0.0) {
                s += e;
                acc += e * x(i);
            }
        }
    }
    s = smm_group_sum<W>(s);
    acc = smm_group_sum<W>(acc);
    if (nan) return __builtin_nan("");
    if (!(s > 0.0)) return 0.0;
    return acc / s;
}

// ------------------------------------------------------------------------------------------------ assembly
// p(o) dev(o) of one occurrence: lp its log-probability, cond = E[R | o] = r(o) + eta-(S_o) + eta+(E_o), V the value
__device__ __forceinline__ double smm_er_term(double lp, double cond, double V)
{
    if (lp == SMM_NEG_INF) return 0.0;
    return exp(lp) * (cond - V);
}

// The policy of smm_posterior_grad.h's skeletons: one side.  The walk's S blocks hold eta at the start nodes with the prefix sum
// of the node's position folded in -- forward eta-(start (s, c)) - cumW[s][c], time-reversed (index j = T - s) eta+(end (s, c))
// + cumW[s][c] -- so a span's frame reward, a difference of two prefix sums, is the near end's cumW (position()) on the end
// node's value and nothing in the assembly; its segment reward rides on one end's eta (near())
struct SmmErPolicy {
    const SmmExpRewardArgs &a;
    const SmmVideo &mv;
    const int T, dir, cm;
    SmmPgSide p;
    const double *cw;              // (the walk's)
    double sg;
    static __device__ __forceinline__ const SmmEntBwdArgs &base(const SmmExpRewardArgs &a) { return a.e; }
    __device__ __forceinline__ SmmErPolicy(const SmmExpRewardArgs &a_, const SmmVideo &mv_, int vid, int T_, int dir_)
        : a(a_), mv(mv_), T(T_), dir(dir_), cm(a_.e.h.c_max), p(smm_pg_side(a_.e.h, a_.e.p, mv_, vid, T_, dir_)), cw(nullptr), sg(0.0)
    {
    }
    template <int W, class Wf, class Xf>
    __device__ __forceinline__ double decide(int i0, int n, int step, Wf w, Xf x) const
    {
        return smm_er_decide<W>(i0, n, step, [&](int i) { return w(p, i); }, x);
    }
    __device__ __forceinline__ bool walk_begin(bool ok, int c, bool act)
    {
        cw = ok ? smm_er_cum(a, mv, cm, T) : nullptr;
        if (ok && cw[0] != cw[0]) ok = false;               // (a non-finite reward: smm_er_prefix_kernel)
        sg = (ok && act) ? smm_er_seg(a, mv.group, cm, c) : 0.0;
        return ok;
    }
    // end node (n, c): forward the span covers [n - k, n) and earns cumW[n] - cumW[n - k], time-reversed [T - n, T - n + k) and
    // cumW[T - n + k] - cumW[T - n]: the far end's cumW is inside S
    __device__ __forceinline__ double position(int n, int c, bool act) const
    {
        return act ? (dir ? -cw[(size_t)(T - n) * cm + c] : cw[(size_t)n * cm + c]) : 0.0;
    }
    __device__ __forceinline__ double end_value(double v, double cw_n) const { return v + (sg + cw_n); }
    __device__ __forceinline__ double start_value(double v, double cw_n) const { return v - cw_n; }
    __device__ __forceinline__ double boundary(double b0, int c) const { return b0 + (dir ? cw[(size_t)T * cm + c] : -cw[c]); }
    __device__ __forceinline__ double closing(int to) const { return smm_er_close_frame(a, mv, cm, T, to) + smm_er_seg(a, mv.group, cm, to); }
    __device__ __forceinline__ double closed(int to, double x) const { return closing(to) + x; }
    __device__ __forceinline__ double near(double eta, int c) const { return eta + smm_er_seg(a, mv.group, cm, c); }
    template <class Lf>
    __device__ __forceinline__ double each(Lf lp) const
    {
        return lp(p);
    }
    template <class Lf>
    __device__ __forceinline__ double each(double v, Lf lp) const
    {
        return lp(p, v);
    }
    __device__ __forceinline__ double term(double lp, double eta, double V) const { return smm_er_term(lp, eta, V); }
};

__global__ void __launch_bounds__(SMM_PG_WALK_THREADS) smm_er_eta_kernel(SmmExpRewardArgs a) { smm_pg_walk<SmmErPolicy>(a); }
__global__ void __launch_bounds__(256) smm_er_nodes_kernel(SmmExpRewardArgs a) { smm_pg_nodes<SmmErPolicy>(a); }
__global__ void __launch_bounds__(1024) smm_er_pairs_kernel(SmmExpRewardArgs a) { smm_pg_pairs<SmmErPolicy>(a); }
__global__ void __launch_bounds__(256) smm_er_len_kernel(SmmExpRewardArgs a) { smm_pg_len<SmmErPolicy>(a); }

void smm_launch_expected_reward(const SmmExpRewardArgs &a, int t_max, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_er_prefix_kernel, dim3(a.e.h.b), dim3(1024), 0, stream, a);
    hipLaunchKernelGGL(smm_expected_reward_kernel, dim3(a.e.h.b, t_max / SMM_POST_SLAB + 1), dim3(SMM_ER_VAL_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_er_sum_kernel, dim3((a.e.h.b + 3) / 4), dim3(256), 0, stream, a);
}

void smm_launch_expected_reward_bwd(const SmmExpRewardArgs &a, int t_max, int kp_max, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_er_prefix_kernel, dim3(a.e.h.b), dim3(1024), 0, stream, a);
    hipLaunchKernelGGL(smm_er_eta_kernel, dim3(a.e.h.b, 2), dim3(SMM_PG_WALK_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_er_nodes_kernel, dim3(a.e.h.b, t_max / SMM_POST_SLAB + 1), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(smm_er_pairs_kernel, dim3(a.e.h.b), dim3(1024), 0, stream, a);
    if (kp_max >= 2)
        hipLaunchKernelGGL(smm_er_len_kernel, dim3(a.e.h.b * a.e.h.c_max, (kp_max - 1 + 255) / 256), dim3(256), 0, stream, a);
    smm_launch_entropy_bwd_tail(a.e, stream);
}
