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
// Work split.  (1) smm_ebwd_eta_kernel: one workgroup per (video, direction) walks the positions in order; 32 lanes per class
// share each node's candidates (K of an end node, C of a start node) and reduce them with butterflies; the local weights are
// recomputed from the histories (T K C of them do not fit anywhere).  Each node has two passes (maxima, then fp64 exponentials
// and sums) so that nothing is rescaled.  (2) smm_ebwd_nodes_kernel: grid (video, slab), thread = node (n, c): D[n][c] = the
// p(o) dev(o) of the spans starting at n minus those ending at n; (3) smm_ebwd_pairs_kernel: per video the transitions, the
// initial class and the closing transition; (4) smm_ebwd_len_kernel: per (video, state) the length sums, thread = k;
// (5) smm_ebwd_elp_kernel: g_elp as the running sum of D over t (the occupancy identity of smm_logz_bwd.hip), x the upstream
// gradient; (6) smm_ebwd_group_kernel: the per-video tables summed over the videos of each group in video order.  No atomics:
// the result is bit-identical run to run.  A video whose value is not finite (+inf: q gives a segmentation of p probability 0;
// NaN) gets NaN rows, and so does its group's tables.
#include "smm_posterior.h"
#include "../../include/smmdp.h"

#define SMM_EB_THREADS 1024        // serial pass: 32 classes x 32 lanes

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

__global__ void __launch_bounds__(SMM_EB_THREADS) smm_ebwd_eta_kernel(SmmEntBwdArgs a)
{
    __shared__ double s_end[SMM_MAX_STATES_DEV];
    const int vid = blockIdx.x, dir = blockIdx.y;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max, kl = a.kl;
    const int C = a.h.n_states[g];
    const int tid = threadIdx.x, c = tid >> 5, l = tid & 31;
    const bool act = c < C;
    const size_t blk = (size_t)cm * (T + 1);
    const SmmHistDir P = smm_hist_dir(a.p.hist, mv, cm, T, dir), R = smm_hist_dir(a.r.hist, mv, cm, T, dir);
    const double *trp = a.p.trans + (size_t)g * cm * cm, *trr = a.r.trans + (size_t)g * cm * cm;
    const double *lenp = a.p.len + (size_t)g * a.h.k_rows * cm, *lenr = a.r.len + (size_t)g * a.h.k_rows * cm;
    double *sv = smm_eb_video(a, mv);
    double *E = sv + (dir ? 2 * blk : 0), *S = E + blk;
    // transitions of this direction: from node class c to candidate c' (time-reversed: transposed)
    const int ts = dir ? 1 : cm, tt = dir ? cm : 1;
    const bool ok = T > 0 && C > 0 && C <= SMM_MAX_STATES_DEV;
    if (ok) {
        // boundary: eta at start (0, c)
        if (act && l == 0) {
            double b0 = 0.0;
            if (dir == 1 && a.h.no_eos) {
                const size_t fr = (size_t)(mv.frame_off + T) * cm;
                b0 = smm_eb_decide<1>(
                    kl, 0, C, 1,
                    [&](int to, double &wp, double &wr) {
                        wp = trp[(size_t)to * cm + c] + a.p.elp[fr + to];
                        wr = trr[(size_t)to * cm + c] + a.r.elp[fr + to];
                    },
                    [&](int) { return 0.0; });
            }
            S[c] = b0;
        }
        __syncthreads();
        for (int n = 1; n <= T; ++n) {
            // end nodes (n, c): the span's length
            const int kmax = (mv.kp - 1 < n) ? mv.kp - 1 : n;
            const double *hp = P.h + (size_t)n * cm + c, *hr = R.h + (size_t)n * cm + c, *sx = S + (size_t)n * cm + c;
            const double ve = smm_eb_decide<32>(
                kl, 1 + l, act ? kmax + 1 : 0, 32,
                [&](int k, double &wp, double &wr) {
                    wp = hp[-(ptrdiff_t)k * cm] + lenp[(size_t)k * cm + c];
                    wr = hr[-(ptrdiff_t)k * cm] + lenr[(size_t)k * cm + c];
                },
                [&](int k) { return sx[-(ptrdiff_t)k * cm]; });
            if (act && l == 0) {
                E[(size_t)n * cm + c] = ve;
                s_end[c] = ve;
            }
            __syncthreads();
            // start nodes (n, c), 0 < n < T: the class of the span on the other side
            if (n < T) {
                const double vs = smm_eb_decide<32>(
                    kl, l, (act && l < C) ? l + 1 : 0, 32,
                    [&](int cc, double &wp, double &wr) {
                        wp = P.g[(size_t)n * cm + cc] + trp[(size_t)c * ts + (size_t)cc * tt];
                        wr = R.g[(size_t)n * cm + cc] + trr[(size_t)c * ts + (size_t)cc * tt];
                    },
                    [&](int cc) { return s_end[cc]; });
                if (act && l == 0) S[(size_t)n * cm + c] = vs;
            }
            __syncthreads();
        }
    }
    // the last decision (wave 0): dir 0 the sampler's final decision, dir 1 the initial class
    if (tid >= 64) return;
    double v = __builtin_nan("");
    const double lzp = a.p.logz[vid];
    if (ok && lzp > SMM_NEG_INF && lzp < -SMM_NEG_INF) {
        const int lane = tid;
        if (dir == 1) {
            v = smm_eb_decide<64>(
                kl, lane, lane < C ? lane + 1 : 0, 64,
                [&](int j, double &wp, double &wr) {
                    wp = P.g[(size_t)T * cm + j] + a.p.init[(size_t)g * cm + j];
                    wr = R.g[(size_t)T * cm + j] + a.r.init[(size_t)g * cm + j];
                },
                [&](int j) { return E[(size_t)T * cm + j]; });
        } else {
            // the sampler's final decision: EOS the class j; no EOS the closing label `to`, then the span label j in front of it
            const double *FpT = P.g + (size_t)T * cm, *FrT = R.g + (size_t)T * cm;
            v = smm_eb_decide<64>(
                kl, lane, lane < C ? lane + 1 : 0, 64,
                [&](int j, double &wp, double &wr) {
                    wp = smm_post_final_weight(a.h, a.p, mv, vid, T, C, FpT, j);
                    wr = smm_post_final_weight(a.h, a.r, mv, vid, T, C, FrT, j);
                },
                [&](int to) {
                    if (!a.h.no_eos) return E[(size_t)T * cm + to];
                    return smm_eb_decide<1>(
                        kl, 0, C, 1,
                        [&](int j, double &wp, double &wr) {
                            wp = FpT[j] + trp[(size_t)to * cm + j];
                            wr = FrT[j] + trr[(size_t)to * cm + j];
                        },
                        [&](int j) { return E[(size_t)T * cm + j]; });
                });
        }
    }
    if (tid == 0) {
        if (v != v) atomicExch(a.h.err, 1);
        smm_eb_fixed(a, vid)[smm_eb_pv(cm, a.h.k_rows).val + dir] = v;
        if (a.value) a.value[2 * vid + dir] = v;
    }
}

// p(o) dev(o) of one occurrence: lp, lr its log-probabilities under p and r, eta the two sides' etas (prefix + suffix), V the value
__device__ __forceinline__ double smm_eb_term(int kl, double lp, double lr, double eta, double V)
{
    if (lp == SMM_NEG_INF) return 0.0;
    const double l = kl ? lp - lr : -lr;
    return exp(lp) * ((l + eta) - V);
}

// log p(span (s, k, c)) on one side: F_h[s][c] + len[k][c] + B_h[T-s-k][c] + cumE[T][c] - logZ
__device__ __forceinline__ double smm_eb_span(const SmmHist &H, const double *len, int T, int cm, int s, int k, int c, double lz)
{
    return H.F.h[(size_t)s * cm + c] + len[(size_t)k * cm + c] + H.B.h[(size_t)(T - s - k) * cm + c] + H.F.cum[(size_t)T * cm + c] - lz;
}

__global__ void __launch_bounds__(256) smm_ebwd_nodes_kernel(SmmEntBwdArgs a)
{
    const int vid = blockIdx.x, y = blockIdx.y;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max, kl = a.kl;
    const int C = a.h.n_states[g];
    if (T <= 0 || C <= 0) return;
    const int n0 = y * SMM_POST_SLAB;
    if (n0 > T) return;
    const size_t blk = (size_t)cm * (T + 1);
    const SmmHist Hp = smm_hist(a.p.hist, mv, cm, T), Hr = smm_hist(a.r.hist, mv, cm, T);
    const double *lenp = a.p.len + (size_t)g * a.h.k_rows * cm, *lenr = a.r.len + (size_t)g * a.h.k_rows * cm;
    double *sv = smm_eb_video(a, mv);
    const double *S0 = sv + blk, *S1 = sv + 3 * blk;
    double *D = sv + 4 * blk;
    double V;
    const bool fin = smm_eb_value(a, vid, &V);
    const double lzp = a.p.logz[vid], lzr = a.r.logz[vid];
    const int n1 = smm_post_slab_end(n0, T);
    for (int i = threadIdx.x; i < (n1 - n0) * cm; i += blockDim.x) {
        const int dn = i / cm, c = i - dn * cm, n = n0 + dn;
        double d = 0.0;
        if (c < C && fin) {
            // spans of c that start at n
            const int ks = (mv.kp - 1 < T - n) ? mv.kp - 1 : T - n;
            for (int k = 1; k <= ks; ++k) {
                const double lp = smm_eb_span(Hp, lenp, T, cm, n, k, c, lzp);
                const double lr = smm_eb_span(Hr, lenr, T, cm, n, k, c, lzr);
                d += smm_eb_term(kl, lp, lr, S0[(size_t)n * cm + c] + S1[(size_t)(T - n - k) * cm + c], V);
            }
            // ... minus those that end at n
            const int ke = (mv.kp - 1 < n) ? mv.kp - 1 : n;
            double e = 0.0;
            for (int k = 1; k <= ke; ++k) {
                const double lp = smm_eb_span(Hp, lenp, T, cm, n - k, k, c, lzp);
                const double lr = smm_eb_span(Hr, lenr, T, cm, n - k, k, c, lzr);
                e += smm_eb_term(kl, lp, lr, S0[(size_t)(n - k) * cm + c] + S1[(size_t)(T - n) * cm + c], V);
            }
            d -= e;
        }
        D[(size_t)n * cm + c] = d;
    }
}

// per video: the transitions (pair = (to, from), slices of the boundaries merged in a fixed order), the initial class, the closing
// transition without EOS
__global__ void __launch_bounds__(1024) smm_ebwd_pairs_kernel(SmmEntBwdArgs a)
{
    __shared__ double s_acc[1024];
    const int vid = blockIdx.x;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max, kl = a.kl;
    const int C = a.h.n_states[g];
    if (T <= 0 || C <= 0) return;
    const size_t blk = (size_t)cm * (T + 1);
    const SmmHist Hp = smm_hist(a.p.hist, mv, cm, T), Hr = smm_hist(a.r.hist, mv, cm, T);
    const double *trp = a.p.trans + (size_t)g * cm * cm, *trr = a.r.trans + (size_t)g * cm * cm;
    const double *sv = smm_eb_video(a, mv);
    const double *E0 = sv, *E1 = sv + 2 * blk;
    const SmmEbPv lo = smm_eb_pv(cm, a.h.k_rows);
    double *pv = smm_eb_fixed(a, vid);
    double V;
    const bool fin = smm_eb_value(a, vid, &V);
    const double lzp = a.p.logz[vid], lzr = a.r.logz[vid];
    const int tid = threadIdx.x, P = C * C, ng = blockDim.x / P;
    const int pair = tid % P, sl = tid / P;
    const int to = pair / C, from = pair - to * C;
    double acc = 0.0;
    if (sl < ng && fin) {
        const double twp = trp[(size_t)to * cm + from] - lzp, twr = trr[(size_t)to * cm + from] - lzr;
        for (int n = 1 + sl; n < T; n += ng) {
            const double lp = Hp.F.g[(size_t)n * cm + from] + twp + Hp.B.g[(size_t)(T - n) * cm + to];
            const double lr = Hr.F.g[(size_t)n * cm + from] + twr + Hr.B.g[(size_t)(T - n) * cm + to];
            acc += smm_eb_term(kl, lp, lr, E0[(size_t)n * cm + from] + E1[(size_t)(T - n) * cm + to], V);
        }
    }
    s_acc[tid] = acc;
    __syncthreads();
    double cl = 0.0;                                    // without EOS: the closing transition from -> to
    if (tid < P && a.h.no_eos && fin) {
        const size_t fr = (size_t)(mv.frame_off + T) * cm + to;
        const double lp = Hp.F.g[(size_t)T * cm + from] + trp[(size_t)to * cm + from] + a.p.elp[fr] - lzp;
        const double lr = Hr.F.g[(size_t)T * cm + from] + trr[(size_t)to * cm + from] + a.r.elp[fr] - lzr;
        cl = smm_eb_term(kl, lp, lr, E0[(size_t)T * cm + from], V);
    }
    if (tid < P) {
        double t = s_acc[tid];
        for (int q = 1; q < ng; ++q) t += s_acc[q * P + tid];
        pv[lo.trans + (size_t)to * cm + from] = fin ? t + cl : __builtin_nan("");
    }
    __syncthreads();
    s_acc[tid] = cl;
    __syncthreads();
    if (tid < C) {
        const int c = tid;
        double ini = __builtin_nan(""), cls = __builtin_nan("");
        if (fin) {
            const double lp = Hp.F.h[c] + Hp.F.cum[c] + Hp.B.g[(size_t)T * cm + c] - lzp;
            const double lr = Hr.F.h[c] + Hr.F.cum[c] + Hr.B.g[(size_t)T * cm + c] - lzr;
            ini = smm_eb_term(kl, lp, lr, E1[(size_t)T * cm + c], V);
            cls = 0.0;
            for (int f = 0; f < C; ++f) cls += s_acc[c * C + f];     // (pair = to * C + from: to = c)
        }
        pv[lo.init + c] = ini;
        pv[lo.close + c] = cls;
    }
}

// per (video, state): the length sums, thread = k, loop over the span's start
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
            const double lp = smm_eb_span(Hp, lenp, T, cm, s, k, c, lzp);
            const double lr = smm_eb_span(Hr, lenr, T, cm, s, k, c, lzr);
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
    hipLaunchKernelGGL(smm_ebwd_eta_kernel, dim3(a.h.b, 2), dim3(SMM_EB_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_ebwd_nodes_kernel, dim3(a.h.b, t_max / SMM_POST_SLAB + 1), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(smm_ebwd_pairs_kernel, dim3(a.h.b), dim3(1024), 0, stream, a);
    if (kp_max >= 2)
        hipLaunchKernelGGL(smm_ebwd_len_kernel, dim3(a.h.b * a.h.c_max, (kp_max - 1 + 255) / 256), dim3(256), 0, stream, a);
    smm_launch_entropy_bwd_tail(a, stream);
}
