// smm_entropy_bwd.hip -- gradients of the posterior entropy H(p), the cross-entropy H(p, q) and KL(p || q) with respect to p's
// factor tables (elp, trans, init, len), for the values smm_entropy.hip and smm_kl.hip compute.
//
// With s(y) the score of segmentation y and phi_o(y) = 1 when occurrence o (a span, a transition at a boundary, the initial class,
// without EOS the closing transition) is part of y,
//   dH(p, q) / d theta_o = -Cov_p(s_q, phi_o)          dKL(p || q) / d theta_o = Cov_p(s_p - s_q, phi_o)
// and a table entry's gradient is the sum over the occurrences that read it.  The covariance is never formed as E[s phi] - E[s] mu
// (s is ~1e6 nats of cumulative emissions).  Given o, the segmentation splits into the part in front of o, which depends on o only
// through the decision node S it starts from, and the part behind, through the node E it ends in (Markov), so
//   -Cov_p(s_q, phi_o) = p(o) * ( l(o) + eta-(S) + eta+(E) - V ),   l(o) = -log r(o)                (entropy, cross-entropy)
//    Cov_p(s_p - s_q, phi_o) = p(o) * ( l(o) + eta-(S) + eta+(E) - V ),  l(o) = log p(o) - log q(o)  (KL)
// r = q (cross-entropy; r = p for the entropy), V = the value itself, eta-(S) = E_p[ -log r(prefix | S) | S ] (KL: the prefix's
// KL) and eta+ the same for the suffix.  eta- follows the chain rule over the decisions of smm_sample.hip's backward walk, every
// local term >= 0:
//   eta-(end (n, c))   = sum_k  p(k | end (n, c))    [ L(k | end (n, c))    + eta-(start (n - k, c)) ]
//   eta-(start (s, c)) = sum_c' p(c' | start (s, c)) [ L(c' | start (s, c)) + eta-(end (s, c')) ],     eta-(start (0, c)) = 0
// with L = -log r (KL: log p - log q) of the local decision, the local distributions of smm_entropy.hip's header (the final
// decision's weights are smm_posterior.h's) on each side's own forward histories.  eta+ is the same recursion on the time-reversed lattice: smm_logz_bwd.hip's backward histories are the
// forward histories of that lattice (transposed transitions), so one kernel serves both directions; its boundary is 0 with EOS
// and, without, the local term of the closing label `to` given end (T, c).  The last decision of each direction closes the sum:
// V- (the sampler's final decision) and V+ (the initial class) are both the value, by independent decompositions.
//
// Work split.  The walk and two assembly kernels are smm_posterior_grad.h's skeletons (smm_ebwd_eta_kernel, _nodes_, _pairs_:
// the work split is described there; smm_ebwd_len_kernel is its own copy of the third, below) under this file's policy: two sides, l(o) = -log r(o) or log p(o) - log q(o),
// a node's value from both sides' sums (smm_eb_node).  Each node of the walk has two passes (maxima, then fp64 exponentials and
// sums) so that nothing is rescaled.  Then smm_ebwd_elp_kernel: g_elp as the running sum of D over t (the occupancy identity of
// smm_logz_bwd.hip), x the upstream gradient; smm_ebwd_group_kernel: the per-video tables summed over the videos of each group
// in video order.  No atomics: the result is bit-identical run to run.  A video whose value is not finite (+inf: q gives a
// segmentation of p probability 0; NaN) gets NaN rows, and so does its group's tables.
#include "smm_posterior_grad.h"
#include "../../include/smmdp.h"

// value of one decision from its candidates' sums: sum_i p_i (L_i + x_i).  A node no candidate of p reaches is never weighed (0);
// p-mass on a candidate r rules out gives +inf.
__device__ __forceinline__ double smm_eb_node(int kl, double mp, double sp, double mr, double sr, double a1, double a2, double a3,
                                              int rinf, int nan)
{
    if (nan) return __builtin_nan("");
    if (!(mp > SMM_NEG_INF) || !(sp > 0.0)) return 0.0;
    if (rinf || !(mr > SMM_NEG_INF)) return -SMM_NEG_INF;
    double loc = kl ? ((a1 / sp - log(sp)) - (a2 / sp - log(sr))) : (log(sr) - a2 / sp);
    loc = loc > 0.0 ? loc : (loc == loc ? 0.0 : loc);
    return loc + a3 / sp;
}

// One decision shared by the W lanes of a group: candidates i = i0, i0 + step, .. < n of this lane; w(i, wp, wr) their weights on
// p and r, x(i) what follows each.  Every lane of the group must call it (butterflies); the result is group-uniform.  W = 1
// (i0 = 0, step = 1): one thread alone, the butterflies have no steps.
template <int W, class Wf, class Xf>
__device__ double smm_eb_decide(int kl, int i0, int n, int step, Wf w, Xf x)
{
    double mp = SMM_NEG_INF, mr = SMM_NEG_INF;
    int nan = 0;
    for (int i = i0; i < n; i += step) {
        double wp, wr;
        w(i, wp, wr);
        nan |= (wp != wp) | (wr != wr) | (wp == -SMM_NEG_INF) | (wr == -SMM_NEG_INF);
        mp = fmax(mp, wp);
        mr = fmax(mr, wr);
    }
    mp = smm_group_max<W>(mp);
    mr = smm_group_max<W>(mr);
    nan = smm_group_or<W>(nan);
    double sp = 0.0, sr = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int rinf = 0;
    if (!nan && mp > SMM_NEG_INF) {
        for (int i = i0; i < n; i += step) {
            double wp, wr;
            w(i, wp, wr);
            const double dp = wp - mp;
            const double e = (dp > SMM_NEG_INF) ? exp(dp) : 0.0;
            if (e > 0.0) {
                sp += e;
                if (wr > SMM_NEG_INF) {
                    a1 += e * dp;
                    a2 += e * (wr - mr);
                } else {
                    rinf = 1;
                }
                a3 += e * x(i);
            }
            if (wr > SMM_NEG_INF) sr += exp(wr - mr);
        }
    }
    sp = smm_group_sum<W>(sp);
    sr = smm_group_sum<W>(sr);
    a1 = smm_group_sum<W>(a1);
    a2 = smm_group_sum<W>(a2);
    a3 = smm_group_sum<W>(a3);
    rinf = smm_group_or<W>(rinf);
    return smm_eb_node(kl, mp, sp, mr, sr, a1, a2, a3, rinf, nan);
}

// p(o) dev(o) of one occurrence: lp, lr its log-probabilities under p and r, eta the two sides' etas (prefix + suffix), V the value
__device__ __forceinline__ double smm_eb_term(int kl, double lp, double lr, double eta, double V)
{
    if (lp == SMM_NEG_INF) return 0.0;
    const double l = kl ? lp - lr : -lr;
    return exp(lp) * ((l + eta) - V);
}

// The policy of smm_posterior_grad.h's skeletons: two sides; nothing rides on a node's value and the closing label earns nothing
// of its own (its local term is inside the decision)
struct SmmEbPolicy {
    SmmPgSide p, r;
    int kl;
    static __device__ __forceinline__ const SmmEntBwdArgs &base(const SmmEntBwdArgs &a) { return a; }
    __device__ __forceinline__ SmmEbPolicy(const SmmEntBwdArgs &a, const SmmVideo &mv, int vid, int T, int dir)
        : p(smm_pg_side(a.h, a.p, mv, vid, T, dir)), r(smm_pg_side(a.h, a.r, mv, vid, T, dir)), kl(a.kl)
    {
    }
    template <int W, class Wf, class Xf>
    __device__ __forceinline__ double decide(int i0, int n, int step, Wf w, Xf x) const
    {
        return smm_eb_decide<W>(
            kl, i0, n, step,
            [&](int i, double &wp, double &wr) {
                wp = w(p, i);
                wr = w(r, i);
            },
            x);
    }
    __device__ __forceinline__ bool walk_begin(bool ok, int, bool) { return ok; }
    __device__ __forceinline__ SmmPgNone position(int, int, bool) const { return {}; }
    __device__ __forceinline__ double end_value(double v, SmmPgNone) const { return v; }
    __device__ __forceinline__ double start_value(double v, SmmPgNone) const { return v; }
    __device__ __forceinline__ double boundary(double b0, int) const { return b0; }
    __device__ __forceinline__ double closing(int) const { return 0.0; }
    __device__ __forceinline__ double closed(int, double x) const { return x; }
    __device__ __forceinline__ double near(double eta, int) const { return eta; }
    struct Two {
        double p, r;
    };
    template <class Lf>
    __device__ __forceinline__ Two each(Lf lp) const
    {
        return {lp(p), lp(r)};
    }
    template <class Lf>
    __device__ __forceinline__ Two each(Two v, Lf lp) const
    {
        return {lp(p, v.p), lp(r, v.r)};
    }
    __device__ __forceinline__ double term(Two lp, double eta, double V) const { return smm_eb_term(kl, lp.p, lp.r, eta, V); }
};

__global__ void __launch_bounds__(SMM_PG_WALK_THREADS) smm_ebwd_eta_kernel(SmmEntBwdArgs a) { smm_pg_walk<SmmEbPolicy>(a); }
__global__ void __launch_bounds__(256) smm_ebwd_nodes_kernel(SmmEntBwdArgs a) { smm_pg_nodes<SmmEbPolicy>(a); }
__global__ void __launch_bounds__(1024) smm_ebwd_pairs_kernel(SmmEntBwdArgs a) { smm_pg_pairs<SmmEbPolicy>(a); }

// per (video, state): the length sums, thread = k, loop over the span's start.  This unit's own copy of smm_pg_len's body:
// on the skeleton the loop was the same instruction for instruction, the code in front of it another, and the kernel measured
// +0.1 .. +1.2 % against the parent's in eight tables of eight (profiles/posterior_grad_shared_ab.txt)
__global__ void __launch_bounds__(256) smm_ebwd_len_kernel(SmmEntBwdArgs a)
{
    const int cm = a.h.c_max;
    const int vid = blockIdx.x / cm, c = blockIdx.x - vid * cm;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, kl = a.kl;
    const int C = a.h.n_states[g];
    if (T <= 0 || c >= C) return;
    const int k = 1 + blockIdx.y * blockDim.x + threadIdx.x;
    const int kmax = (mv.kp - 1 < T) ? mv.kp - 1 : T;
    if (k > kmax) return;
    const size_t blk = (size_t)cm * (T + 1);
    const SmmHist Hp = smm_hist(a.p.hist, mv, cm, T), Hr = smm_hist(a.r.hist, mv, cm, T);
    const double *lenp = a.p.len + (size_t)g * a.h.k_rows * cm, *lenr = a.r.len + (size_t)g * a.h.k_rows * cm;
    const double *sv = smm_eb_video(a, mv);
    const double *S0 = sv + blk, *S1 = sv + 3 * blk;
    double V;
    const bool fin = smm_eb_value(a, vid, &V);
    const double lzp = a.p.logz[vid], lzr = a.r.logz[vid];
    double acc = __builtin_nan("");
    if (fin) {
        acc = 0.0;
        for (int s = 0; s + k <= T; ++s) {
            const double lp = smm_pg_span(Hp, lenp, T, cm, s, k, c, lzp);
            const double lr = smm_pg_span(Hr, lenr, T, cm, s, k, c, lzr);
            acc += smm_eb_term(kl, lp, lr, S0[(size_t)s * cm + c] + S1[(size_t)(T - s - k) * cm + c], V);
        }
    }
    smm_eb_fixed(a, vid)[smm_eb_pv(cm, a.h.k_rows).len + (size_t)k * cm + c] = acc;
}

// g_elp of one video: running sums of D over t, threads = (state, chunk of frames), two passes (smm_marginals_kernel's (b))
__global__ void __launch_bounds__(1024) smm_ebwd_elp_kernel(SmmEntBwdArgs a)
{
    __shared__ double part[32][33];
    const int vid = blockIdx.x;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max;
    const int C = a.h.n_states[g];
    if (T <= 0 || C <= 0) return;
    const size_t blk = (size_t)cm * (T + 1);
    const double *D = smm_eb_video(a, mv) + 4 * blk;
    double V;
    const bool fin = smm_eb_value(a, vid, &V);
    const double up = a.grad_out ? a.grad_out[vid] : 1.0;
    const int tid = threadIdx.x, c = tid & 31, j = tid >> 5, nj = blockDim.x >> 5;
    const int cs = (T + nj - 1) / nj;
    const int t0 = j * cs, t1 = (t0 + cs < T) ? t0 + cs : T;
    double sum = 0.0;
    if (c < C)
        for (int t = t0; t < t1; ++t) sum += D[(size_t)t * cm + c];
    part[c][j] = sum;
    __syncthreads();
    if (c < C) {
        double run = 0.0;
        for (int q = 0; q < j; ++q) run += part[c][q];
        for (int t = t0; t < t1; ++t) {
            run += D[(size_t)t * cm + c];
            a.g_elp[(size_t)(mv.frame_off + t) * cm + c] = fin ? up * run : __builtin_nan("");
        }
        if (a.h.no_eos && j == 0) {
            const double cl = smm_eb_fixed(a, vid)[smm_eb_pv(cm, a.h.k_rows).close + c];
            a.g_elp[(size_t)(mv.frame_off + T) * cm + c] = fin ? up * cl : __builtin_nan("");
        }
    }
}

// the tables of each group: the per-video sums x the upstream gradient, over the videos of the group in video order
__global__ void __launch_bounds__(256) smm_ebwd_group_kernel(SmmEntBwdArgs a)
{
    const int cm = a.h.c_max;
    const SmmEbPv lo = smm_eb_pv(cm, a.h.k_rows);
    const int64_t per = lo.val;                         // len | trans | init
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= per * a.n_groups) return;
    const int g = (int)(i / per);
    const int64_t e = i - (int64_t)g * per;
    if (e >= lo.close) return;
    double acc = 0.0;
    for (int v = 0; v < a.h.b; ++v) {
        if (a.h.videos[v].group != g) continue;
        const double up = a.grad_out ? a.grad_out[v] : 1.0;
        acc += up * smm_eb_fixed(a, v)[e];
    }
    if (e < lo.trans) a.g_len[(size_t)g * a.h.k_rows * cm + e] = acc;
    else if (e < lo.init) a.g_trans[(size_t)g * cm * cm + (e - lo.trans)] = acc;
    else a.g_init[(size_t)g * cm + (e - lo.init)] = acc;
}

size_t smm_entropy_bwd_fixed_doubles(int c_max, int k_rows)
{
    return (size_t)smm_eb_pv(c_max, k_rows).stride;
}

void smm_launch_entropy_bwd_tail(const SmmEntBwdArgs &a, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_ebwd_elp_kernel, dim3(a.h.b), dim3(1024), 0, stream, a);
    const int64_t n = (int64_t)smm_eb_pv(a.h.c_max, a.h.k_rows).val * a.n_groups;
    hipLaunchKernelGGL(smm_ebwd_group_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, a);
}

void smm_launch_entropy_bwd(const SmmEntBwdArgs &a, int t_max, int kp_max, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_ebwd_eta_kernel, dim3(a.h.b, 2), dim3(SMM_PG_WALK_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_ebwd_nodes_kernel, dim3(a.h.b, t_max / SMM_POST_SLAB + 1), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(smm_ebwd_pairs_kernel, dim3(a.h.b), dim3(1024), 0, stream, a);
    if (kp_max >= 2)
        hipLaunchKernelGGL(smm_ebwd_len_kernel, dim3(a.h.b * a.h.c_max, (kp_max - 1 + 255) / 256), dim3(256), 0, stream, a);
    smm_launch_entropy_bwd_tail(a, stream);
}
