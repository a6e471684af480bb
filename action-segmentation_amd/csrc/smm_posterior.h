// smm_posterior.h -- what the posterior kernels (smm_entropy.hip, smm_kl.hip, smm_entropy_bwd.hip, the final decision of
// smm_sample.hip) share, each stated once: the history view, the local distributions of the sampler's decisions, p's entropy of
// the final decision, the end node's online normaliser, the node log-probabilities, and the slab partition with its fixed-order
// sums.  The cross-entropy of p with itself is the entropy, and KL(p || p) is 0, because both kernels run THESE operations.
#pragma once
#include "smm_device.h"
#include "smm_launch.h"

#define SMM_POST_SLAB 64           // positions per workgroup of the (video, slab) grids: one partition, the same sums

// ---- a video's histories (smm_logz_bwd.hip has the layout): three [T+1][c_max] blocks per direction, then the scratch rows
struct SmmHistDir {
    const double *cum, *h, *g;
};
struct SmmHist {
    SmmHistDir F, B;
    double *scratch;               // hT0, hT1
};

// one direction: 0 forward, 1 backward (the forward histories of the time-reversed lattice)
__device__ __forceinline__ SmmHistDir smm_hist_dir(const double *hist, const SmmVideo &mv, int cm, int T, int dir)
{
    const size_t blk = (size_t)cm * (T + 1);
    const double *b = hist + mv.hist_off + (dir ? 3 * blk : 0);
    return {b, b + blk, b + 2 * blk};
}

__device__ __forceinline__ SmmHist smm_hist(const double *hist, const SmmVideo &mv, int cm, int T)
{
    return {smm_hist_dir(hist, mv, cm, T, 0), smm_hist_dir(hist, mv, cm, T, 1),
            const_cast<double *>(hist + mv.hist_off + 6 * (size_t)cm * (T + 1))};
}

// ---- local distributions
__device__ __forceinline__ double smm_lse2_exact(double a, double b)
{
    const double m = fmax(a, b);
    if (m == SMM_NEG_INF) return m;
    return m + log(exp(a - m) + exp(b - m));
}

// log S - A / S, clamped at 0 (rounding); NaN when no candidate was finite
__device__ __forceinline__ double smm_post_ent_local(double m, double s, double a)
{
    if (!(m > SMM_NEG_INF)) return __builtin_nan("");
    const double h = log(s) - a / s;
    return h > 0.0 ? h : (h == h ? 0.0 : h);
}

// entropy of the distribution exp(w0[i * st] + w1[i]), i < n, fp64 throughout; NaN when no finite candidate
__device__ __forceinline__ double smm_post_ent_of(const double *w0, const double *w1, int n, int st)
{
    double m = SMM_NEG_INF;
    bool nan = false;
    for (int i = 0; i < n; ++i) {
        const double w = w0[(size_t)i * st] + w1[i];
        nan |= (w != w);
        m = fmax(m, w);
    }
    if (nan || !(m > SMM_NEG_INF) || m == -SMM_NEG_INF) return __builtin_nan("");
    double s = 0.0, a = 0.0;
    for (int i = 0; i < n; ++i) {
        const double d = w0[(size_t)i * st] + w1[i] - m;
        if (d > SMM_NEG_INF) {
            const double e = exp(d);
            s += e;
            a += e * d;
        }
    }
    return smm_post_ent_local(m, s, a);
}

// EOS closing weight of class j: LSE(endpen[j], LSE_to(trans[to][j]) - 1e9)
__device__ __forceinline__ double smm_post_wend(const double *trans, const double *endpen, int cm, int C, int j)
{
    double alt = SMM_NEG_INF;
    for (int to = 0; to < C; ++to) alt = smm_lse2_exact(alt, trans[(size_t)to * cm + j]);
    return smm_lse2_exact(endpen ? endpen[j] : 0.0, alt + SMM_BIG_NEG);
}

// no EOS: weight of the closing label `to`, LSE_c(F_g[T][c] + trans[to][c]) + elp[T][to] formed as mx + log s + elp; NaN for a
// NaN, -inf without a finite candidate.  With `hcond`: also the entropy of the span label in front given `to` (left alone when
// the weight carries no sum)
__device__ __forceinline__ double smm_post_to_weight(const double *Fg_T, const double *row, double elp_to, int C,
                                                     double *hcond = nullptr)
{
    double mx = SMM_NEG_INF;
    for (int c = 0; c < C; ++c) mx = fmax(mx, Fg_T[c] + row[c]);
    if (mx != mx) return mx;
    if (!(mx > SMM_NEG_INF && mx < -SMM_NEG_INF)) return SMM_NEG_INF;
    double s = 0.0, acc = 0.0;
    for (int c = 0; c < C; ++c) {
        const double d = Fg_T[c] + row[c] - mx;
        if (d > SMM_NEG_INF) {
            const double e = exp(d);
            s += e;
            acc += e * d;
        }
    }
    if (hcond) *hcond = smm_post_ent_local(mx, s, acc);
    return mx + log(s) + elp_to;
}

// weight of candidate j of the final decision on one side: EOS the class j, no EOS the closing label j
__device__ __forceinline__ double smm_post_final_weight(const SmmPostHead &h, const SmmPostSide &s, const SmmVideo &mv, int vid,
                                                        int T, int C, const double *Fg_T, int j, double *hcond = nullptr)
{
    const int cm = h.c_max;
    const double *trans = s.trans + (size_t)mv.group * cm * cm;
    if (!h.no_eos) return Fg_T[j] + smm_post_wend(trans, s.endpen ? s.endpen + (size_t)vid * cm : nullptr, cm, C, j);
    return smm_post_to_weight(Fg_T, trans + (size_t)j * cm, s.elp[(size_t)(mv.frame_off + T) * cm + j], C, hcond);
}

// Entropy of the final decision from the lanes' weights w (`on`: this lane has a candidate) and their finite wave maximum m;
// without EOS + sum_to P(to) H(j | to), a `to` of probability 0 not counting.  e, s: the lane's exp(w - m) and their sum.
// All 64 lanes must call it; the result is wave-uniform.
__device__ __forceinline__ double smm_post_final_entropy(double w, double m, bool on, int no_eos, double hcond, double &e, double &s)
{
    const double d = w - m;
    e = (on && d > SMM_NEG_INF) ? exp(d) : 0.0;
    s = smm_group_sum<64>(e);
    const double ad = smm_group_sum<64>(e > 0.0 ? e * d : 0.0);
    double h = smm_post_ent_local(m, s, ad);
    if (no_eos) h += smm_group_sum<64>((e > 0.0) ? (e / s) * hcond : 0.0);
    return h;
}

// One candidate of weight w into an end node's online (m, S, A): S = sum e^{w-m}, A = sum e^{w-m} (w - m), the exponentials
// through v_exp_f32 on fp64-shifted arguments.  (smm_kl_kernel's K loop holds the one copy of this step, with p's fp64 sums inside
// its two branches: a correction here is a correction there.)
__device__ __forceinline__ void smm_post_online(double w, double &m, double &s, double &ad)
{
    const double d = w - m;
    if (d > 0.0) {                                         // a new maximum (or the first finite one)
        const double r = (double)__expf((float)-d);        // (m = -inf: d = inf, r = 0)
        ad = r * (ad - (s > 0.0 ? s * d : 0.0));
        s = r * s + 1.0;
        m = w;
    } else if (w > SMM_NEG_INF) {
        const double e = (double)__expf((float)d);
        s += e;
        ad += e * d;
    }
}

// ---- node log-probabilities: P(a span of c ends at n), P(a span of c starts at n)
__device__ __forceinline__ double smm_post_lp_end(const SmmHist &H, int T, int cm, int n, int c, double lz)
{
    return H.F.g[(size_t)n * cm + c] + H.B.h[(size_t)(T - n) * cm + c] + H.B.cum[(size_t)(T - n) * cm + c] - lz;
}

__device__ __forceinline__ double smm_post_lp_start(const SmmHist &H, int T, int cm, int n, int c, double lz)
{
    return H.F.h[(size_t)n * cm + c] + H.F.cum[(size_t)n * cm + c] + H.B.g[(size_t)(T - n) * cm + c] - lz;
}

// ---- slabs: workgroup y of a video takes the positions n0 .. n1 - 1 of 0 .. T; ns slabs per video
__device__ __forceinline__ int smm_post_slab_end(int n0, int T) { return (n0 + SMM_POST_SLAB <= T) ? n0 + SMM_POST_SLAB : T + 1; }
__device__ __forceinline__ int smm_post_slabs(int T) { return T / SMM_POST_SLAB + 1; }

// One or two accumulators (NA; a1 is not read for one) of a workgroup of 64 NW threads, summed in a fixed order (butterfly
// within each wave, then the waves in order) into part[i * ns + y].  (By value: as an array by reference the accumulators cost
// smm_entropy_kernel and smm_kl_kernel 4 VGPRs each.)
template <int NA, int NW>
__device__ __forceinline__ void smm_post_block_sum(double a0, double a1, double (&s_part)[NA][NW], double *part, int ns, int y)
{
    const int tid = threadIdx.x;
    a0 = smm_group_sum<64>(a0);
    if (NA > 1) a1 = smm_group_sum<64>(a1);
    if ((tid & 63) == 0) {
        s_part[0][tid >> 6] = a0;
        if (NA > 1) s_part[NA - 1][tid >> 6] = a1;
    }
    __syncthreads();
    if (tid < NA) {
        double t = s_part[tid][0];
#pragma unroll
        for (int w = 1; w < NW; ++w) t += s_part[tid][w];
        part[(size_t)tid * ns + y] = t;
    }
}

// ... and the slab partials of one video summed by one wave, lane-strided, then the butterfly
template <int NA>
__device__ __forceinline__ void smm_post_video_sum(const double *part, int ns, int lane, double (&out)[NA])
{
    double t[NA] = {};
    for (int q = lane; q < ns; q += 64) {
#pragma unroll
        for (int i = 0; i < NA; ++i) t[i] += part[(size_t)i * ns + q];
    }
#pragma unroll
    for (int i = 0; i < NA; ++i) out[i] = smm_group_sum<64>(t[i]);
}

// ---- the caller's scratch of the gradient units (smm_entropy_bwd.hip, smm_expected_reward.hip), one layout for both
// per-video layout of the caller's scratch: 4 eta blocks and D, each [T+1][c_max], at 6/8 of the video's history offset; the
// fixed part (smm_eb_pv) behind all of them
struct SmmEbPv {
    int64_t len, trans, init, close, val, stride;
};
__device__ __host__ __forceinline__ SmmEbPv smm_eb_pv(int cm, int k_rows)
{
    SmmEbPv p;
    p.len = 0;
    p.trans = (int64_t)k_rows * cm;
    p.init = p.trans + (int64_t)cm * cm;
    p.close = p.init + cm;
    p.val = p.close + cm;
    p.stride = (p.val + 4 + 3) / 4 * 4;
    return p;
}

__device__ __forceinline__ double *smm_eb_video(const SmmEntBwdArgs &a, const SmmVideo &mv)
{
    return a.scratch + mv.hist_off / 8 * 6;
}

__device__ __forceinline__ double *smm_eb_fixed(const SmmEntBwdArgs &a, int vid)
{
    return a.scratch + a.pv_base + (int64_t)vid * smm_eb_pv(a.h.c_max, a.h.k_rows).stride;
}

// the value V- every assembly kernel subtracts; false when the video gets NaN rows
__device__ __forceinline__ bool smm_eb_value(const SmmEntBwdArgs &a, int vid, double *V)
{
    const double *f = smm_eb_fixed(a, vid) + smm_eb_pv(a.h.c_max, a.h.k_rows).val;
    *V = f[0];
    return f[0] > SMM_NEG_INF && f[0] < -SMM_NEG_INF && f[1] > SMM_NEG_INF && f[1] < -SMM_NEG_INF;
}
