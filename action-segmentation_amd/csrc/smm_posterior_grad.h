// smm_posterior_grad.h -- the skeletons of the gradient units of the unconstrained lattice (smm_entropy_bwd.hip: entropy,
// cross-entropy, KL; smm_expected_reward.hip: an additive reward), each stated once.  Both units form
//   d value / d theta_o = p(o) * ( l(o) + eta-(S_o) + eta+(E_o) - V )
// for every occurrence o (a span, a transition at a boundary, the initial class, without EOS the closing transition), S_o the
// decision node o starts from and E_o the one it ends in; they differ in what an occurrence earns (l(o)) and in the sum a
// decision node forms.  A unit states that in a policy; the indexing, the loop bounds, the slices and their merge, and the
// stores are here.  A policy is constructed per thread from (the unit's arguments, the video, vid, T, dir) and supplies
//   base(args)                 the SmmEntBwdArgs inside the unit's arguments (the scratch layout is smm_posterior.h's)
//   decide<W>(i0, n, step, w, x)   one decision shared by W lanes: candidates i0, i0 + step, .. < n of this lane, w(side, i)
//                              their weight on one side, x(i) what follows each; every lane of the group calls it, the result
//                              is group-uniform
//   walk_begin(ok, c, act)     the walk's per-video state; false: the video gets NaN values
//   position(n, c, act), end_value(v, at), start_value(v, at), boundary(b0, c)
//                              what rides on a node's value where it is stored (at: whatever position() returned)
//   closing(to), closed(to, x) what the closing label `to` of frame T earns (no EOS), alone and in front of x
//   near(eta, c)               what a span of c adds to the eta of one of its ends
//   each(lp), each(v, lp)      lp(side), an occurrence's log-probability on one side, for every side of the unit; with v, an
//                              earlier each()'s result, lp(side, v's entry of that side)
//   term(lps, eta, V)          p(o) dev(o) of an occurrence: lps = what each() returned, eta = the etas of its two ends (and what
//                              near / closed added)
// Every hook is inlined: a hook that returns its argument leaves no instruction, and each unit keeps its own order of additions.
//
// Work split.  smm_pg_walk: one workgroup per (video, direction) walks the positions in order; 32 lanes per class share each
// node's candidates (K of an end node, C of a start node) and reduce them with butterflies; the local weights are recomputed
// from the histories (T K C of them do not fit anywhere).  The time-reversed direction runs on the backward histories
// (smm_logz_bwd.hip: the forward histories of the reversed lattice) with transposed transitions.  Bounded by the serial chain:
// T steps of two dependent decisions each.  smm_pg_nodes: grid (video, slab of SMM_POST_SLAB positions), thread = node (n, c):
// D[n][c] = the p(o) dev(o) of the spans starting at n minus those ending at n; O(T K C) exponentials, the most arithmetic.
// smm_pg_pairs: per video the transitions (pair = (to, from), slices of the boundaries merged in a fixed order in LDS), the
// initial class and the closing transition.  smm_pg_len: per (video, state) the length sums, thread = k, blocks of 256 lengths.
// No atomics but the error word: the result is bit-identical run to run.
#pragma once
#include "smm_posterior.h"

#define SMM_PG_WALK_THREADS 1024   // 32 classes x 32 lanes

// one side (one posterior) as the skeletons read it: the video's histories, its group's tables, its log Z
struct SmmPgSide {
    const SmmPostSide &s;
    SmmHist H;
    SmmHistDir D;                  // the walk's direction
    const double *trans, *len;
    double lz;
};
__device__ __forceinline__ SmmPgSide smm_pg_side(const SmmPostHead &h, const SmmPostSide &s, const SmmVideo &mv, int vid, int T,
                                                 int dir)
{
    const int cm = h.c_max;
    return {s, smm_hist(s.hist, mv, cm, T), smm_hist_dir(s.hist, mv, cm, T, dir), s.trans + (size_t)mv.group * cm * cm,
            s.len + (size_t)mv.group * h.k_rows * cm, s.logz[vid]};
}

struct SmmPgNone {};               // position() of a policy with nothing riding on the node values

// log p(span (s, k, c)) on one side: F_h[s][c] + len[k][c] + B_h[T-s-k][c] + cumE[T][c] - logZ
__device__ __forceinline__ double smm_pg_span(const SmmHist &H, const double *len, int T, int cm, int s, int k, int c, double lz)
{
    return H.F.h[(size_t)s * cm + c] + len[(size_t)k * cm + c] + H.B.h[(size_t)(T - s - k) * cm + c] + H.F.cum[(size_t)T * cm + c] - lz;
}
__device__ __forceinline__ double smm_pg_span(const SmmPgSide &x, int T, int cm, int s, int k, int c)
{
    return smm_pg_span(x.H, x.len, T, cm, s, k, c, x.lz);
}

// ------------------------------------------------------------------------------------------------ the walk
// grid (video, direction), SMM_PG_WALK_THREADS threads.  Leaves eta at the end nodes (E) and the start nodes (S) of its
// direction in the video's scratch blocks, and the value by its direction's last decision: dir 0 V- (the sampler's final
// decision), dir 1 V+ (the initial class).
template <class Pol, class Args>
__device__ __forceinline__ void smm_pg_walk(const Args &args)
{
    __shared__ double s_end[SMM_MAX_STATES_DEV];
    const SmmEntBwdArgs &a = Pol::base(args);
    const int vid = blockIdx.x, dir = blockIdx.y;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max;
    const int C = a.h.n_states[g];
    const int tid = threadIdx.x, c = tid >> 5, l = tid & 31;
    const bool act = c < C;
    const size_t blk = (size_t)cm * (T + 1);
    Pol pol(args, mv, vid, T, dir);
    double *sv = smm_eb_video(a, mv);
    double *E = sv + (dir ? 2 * blk : 0), *S = E + blk;
    // transitions of this direction: from node class c to candidate c' (time-reversed: transposed)
    const int ts = dir ? 1 : cm, tt = dir ? cm : 1;
    const bool ok = pol.walk_begin(T > 0 && C > 0 && C <= SMM_MAX_STATES_DEV, c, act);
    if (ok) {
        // boundary: eta at start (0, c); time-reversed without EOS the closing label `to` given end (T, c)
        if (act && l == 0) {
            double b0 = 0.0;
            if (dir == 1 && a.h.no_eos) {
                const size_t fr = (size_t)(mv.frame_off + T) * cm;
                b0 = pol.template decide<1>(
                    0, C, 1, [&](const SmmPgSide &x, int to) { return x.trans[(size_t)to * cm + c] + x.s.elp[fr + to]; },
                    [&](int to) { return pol.closing(to); });
            }
            S[c] = pol.boundary(b0, c);
        }
        __syncthreads();
        for (int n = 1; n <= T; ++n) {
            // end nodes (n, c): the span's length
            const int kmax = (mv.kp - 1 < n) ? mv.kp - 1 : n;
            const double *sx = S + (size_t)n * cm + c;
            const auto at = pol.position(n, c, act);
            const double ve = pol.end_value(
                pol.template decide<32>(
                    1 + l, act ? kmax + 1 : 0, 32,
                    [&](const SmmPgSide &x, int k) {
                        return (x.D.h + (size_t)n * cm + c)[-(ptrdiff_t)k * cm] + x.len[(size_t)k * cm + c];
                    },
                    [&](int k) { return sx[-(ptrdiff_t)k * cm]; }),
                at);
            if (act && l == 0) {
                E[(size_t)n * cm + c] = ve;
                s_end[c] = ve;
            }
            __syncthreads();
            // start nodes (n, c), 0 < n < T: the class of the span on the other side
            if (n < T) {
                const double vs = pol.template decide<32>(
                    l, (act && l < C) ? l + 1 : 0, 32,
                    [&](const SmmPgSide &x, int cc) {
                        return x.D.g[(size_t)n * cm + cc] + x.trans[(size_t)c * ts + (size_t)cc * tt];
                    },
                    [&](int cc) { return s_end[cc]; });
                if (act && l == 0) S[(size_t)n * cm + c] = pol.start_value(vs, at);
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
        const double *ET = E + (size_t)T * cm;
        if (dir == 1) {
            v = pol.template decide<64>(
                lane, lane < C ? lane + 1 : 0, 64,
                [&](const SmmPgSide &x, int j) { return x.D.g[(size_t)T * cm + j] + x.s.init[(size_t)g * cm + j]; },
                [&](int j) { return ET[j]; });
        } else {
            // the sampler's final decision: EOS the class j; no EOS the closing label `to`, then the span label j in front of it
            v = pol.template decide<64>(
                lane, lane < C ? lane + 1 : 0, 64,
                [&](const SmmPgSide &x, int j) {
                    return smm_post_final_weight(a.h, x.s, mv, vid, T, C, x.D.g + (size_t)T * cm, j);
                },
                [&](int to) {
                    if (!a.h.no_eos) return ET[to];
                    return pol.closed(to, pol.template decide<1>(
                                              0, C, 1,
                                              [&](const SmmPgSide &x, int j) {
                                                  return x.D.g[(size_t)T * cm + j] + x.trans[(size_t)to * cm + j];
                                              },
                                              [&](int j) { return ET[j]; }));
                });
        }
    }
    if (tid == 0) {
        if (v != v) atomicExch(a.h.err, 1);
        smm_eb_fixed(a, vid)[smm_eb_pv(cm, a.h.k_rows).val + dir] = v;
        if (a.value) a.value[2 * vid + dir] = v;
    }
}

// ------------------------------------------------------------------------------------------------ assembly
// grid (video, slab), 256 threads, thread = node (n, c): D[n][c]
template <class Pol, class Args>
__device__ __forceinline__ void smm_pg_nodes(const Args &args)
{
    const SmmEntBwdArgs &a = Pol::base(args);
    const int vid = blockIdx.x, y = blockIdx.y;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max;
    const int C = a.h.n_states[g];
    if (T <= 0 || C <= 0) return;
    const int n0 = y * SMM_POST_SLAB;
    if (n0 > T) return;                                 // positions 0 .. T
    const size_t blk = (size_t)cm * (T + 1);
    const Pol pol(args, mv, vid, T, 0);
    double *sv = smm_eb_video(a, mv);
    const double *S0 = sv + blk, *S1 = sv + 3 * blk;
    double *D = sv + 4 * blk;
    double V;
    const bool fin = smm_eb_value(a, vid, &V);
    const int n1 = smm_post_slab_end(n0, T);
    for (int i = threadIdx.x; i < (n1 - n0) * cm; i += blockDim.x) {
        const int dn = i / cm, c = i - dn * cm, n = n0 + dn;
        double d = 0.0;
        if (c < C && fin) {
            // spans of c that start at n
            const int ks = (mv.kp - 1 < T - n) ? mv.kp - 1 : T - n;
            const double s0 = pol.near(S0[(size_t)n * cm + c], c);
            for (int k = 1; k <= ks; ++k)
                d += pol.term(pol.each([&](const SmmPgSide &x) { return smm_pg_span(x, T, cm, n, k, c); }),
                              s0 + S1[(size_t)(T - n - k) * cm + c], V);
            // ... minus those that end at n
            const int ke = (mv.kp - 1 < n) ? mv.kp - 1 : n;
            const double s1 = pol.near(S1[(size_t)(T - n) * cm + c], c);
            double e = 0.0;
            for (int k = 1; k <= ke; ++k)
                e += pol.term(pol.each([&](const SmmPgSide &x) { return smm_pg_span(x, T, cm, n - k, k, c); }),
                              s1 + S0[(size_t)(n - k) * cm + c], V);
            d -= e;
        }
        D[(size_t)n * cm + c] = d;
    }
}

// grid (video), 1024 threads: the transitions, the initial class, the closing transition without EOS
template <class Pol, class Args>
__device__ __forceinline__ void smm_pg_pairs(const Args &args)
{
    __shared__ double s_acc[1024];
    const SmmEntBwdArgs &a = Pol::base(args);
    const int vid = blockIdx.x;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max;
    const int C = a.h.n_states[g];
    if (T <= 0 || C <= 0) return;
    const size_t blk = (size_t)cm * (T + 1);
    const Pol pol(args, mv, vid, T, 0);
    const double *sv = smm_eb_video(a, mv);
    const double *E0 = sv, *E1 = sv + 2 * blk;
    const SmmEbPv lo = smm_eb_pv(cm, a.h.k_rows);
    double *pv = smm_eb_fixed(a, vid);
    double V;
    const bool fin = smm_eb_value(a, vid, &V);
    const int tid = threadIdx.x, P = C * C, ng = blockDim.x / P;
    const int pair = tid % P, sl = tid / P;             // (sl == ng: the idle threads past ng * P)
    const int to = pair / C, from = pair - to * C;
    double acc = 0.0;
    if (sl < ng && fin) {
        // (each side's tw in front of the loop by hand: left to the compiler, the second side's transition load and its
        // subtraction stay inside the loop, behind the first side's test -- measured so, smm_ebwd_pairs_kernel against the
        // parent's: 0.4055 / 0.3859 ms at cfg2, 0.1784 / 0.1673 ms at cfg4.  The two indices are stated once: without that
        // the two units' kernels take 80 / 69 VGPRs for the parent's 69 / 63)
        const auto tw = pol.each([&](const SmmPgSide &x) { return x.trans[(size_t)to * cm + from] - x.lz; });
        for (int n = 1 + sl; n < T; n += ng) {
            const size_t i0 = (size_t)n * cm + from, i1 = (size_t)(T - n) * cm + to;
            acc += pol.term(pol.each(tw, [&](const SmmPgSide &x, double tw_x) { return x.H.F.g[i0] + tw_x + x.H.B.g[i1]; }),
                            E0[i0] + E1[i1], V);
        }
    }
    s_acc[tid] = acc;
    __syncthreads();
    double cl = 0.0;                                    // without EOS: the closing transition from -> to
    if (tid < P && a.h.no_eos && fin) {
        const size_t fr = (size_t)(mv.frame_off + T) * cm + to;
        cl = pol.term(pol.each([&](const SmmPgSide &x) {
                          return x.H.F.g[(size_t)T * cm + from] + x.trans[(size_t)to * cm + from] + x.s.elp[fr] - x.lz;
                      }),
                      pol.closed(to, E0[(size_t)T * cm + from]), V);
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
            ini = pol.term(
                pol.each([&](const SmmPgSide &x) { return x.H.F.h[c] + x.H.F.cum[c] + x.H.B.g[(size_t)T * cm + c] - x.lz; }),
                E1[(size_t)T * cm + c], V);
            cls = 0.0;
            for (int f = 0; f < C; ++f) cls += s_acc[c * C + f];     // (pair = to * C + from: to = c)
        }
        pv[lo.init + c] = ini;
        pv[lo.close + c] = cls;
    }
}

// grid (video x state, blocks of 256 lengths), thread = k, loop over the span's start
template <class Pol, class Args>
__device__ __forceinline__ void smm_pg_len(const Args &args)
{
    const SmmEntBwdArgs &a = Pol::base(args);
    const int cm = a.h.c_max;
    const int vid = blockIdx.x / cm, c = blockIdx.x - vid * cm;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group;
    const int C = a.h.n_states[g];
    if (T <= 0 || c >= C) return;
    const int k = 1 + blockIdx.y * blockDim.x + threadIdx.x;
    const int kmax = (mv.kp - 1 < T) ? mv.kp - 1 : T;
    if (k > kmax) return;
    const size_t blk = (size_t)cm * (T + 1);
    const Pol pol(args, mv, vid, T, 0);
    const double *sv = smm_eb_video(a, mv);
    const double *S0 = sv + blk, *S1 = sv + 3 * blk;
    double V;
    const bool fin = smm_eb_value(a, vid, &V);
    double acc = __builtin_nan("");
    if (fin) {
        acc = 0.0;
        for (int s = 0; s + k <= T; ++s)
            acc += pol.term(pol.each([&](const SmmPgSide &x) { return smm_pg_span(x, T, cm, s, k, c); }),
                            pol.near(S0[(size_t)s * cm + c], c) + S1[(size_t)(T - s - k) * cm + c], V);
    }
    smm_eb_fixed(a, vid)[smm_eb_pv(cm, a.h.k_rows).len + (size_t)k * cm + c] = acc;
}
