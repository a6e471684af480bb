// smm_entropy.hip -- exact entropy H(y | x) = -sum_y p(y | x) log p(y | x) of each video's segmentation posterior.
//
// Inputs are the two histories smm_logz_bwd.hip's header lays out (forward F_cum, F_h, F_g; backward B_cum, B_h, B_g).
// y is in one-to-one correspondence with the decisions of the backward walk smm_sample.hip draws (its header lists them), a
// Markov chain over decision nodes, so by the chain rule of entropy
//   H(y | x) = H(final decision)
//            + sum_{n >= 1, c}   P(a span of c ends at n)   * H(start of that span | end (n, c))            O(T K C)
//            + sum_{0 < s, c}    P(a span of c starts at s) * H(class of the span in front | start (s, c))  O(T C^2)
// with the node probabilities (smm_logz_bwd.hip)
//   P(end (n, c))   = exp(F_g[n][c] + B_h[T-n][c] + B_cum[T-n][c] - logZ)
//   P(start (s, c)) = exp(F_h[s][c] + F_cum[s][c] + B_g[T-s][c] - logZ)
// and the sampler's local distributions
//   end (n, c)      k  ~ exp(F_h[n-k][c] + len[k][c]),  k = 1 .. min(kp-1, n)
//   start (s, c)    c' ~ exp(F_g[s][c'] + trans[c][c'])
//   final, EOS      j  ~ exp(F_g[T][j] + wend[j]),  wend[j] = LSE(endpen[j], LSE_to(trans[to][j]) - 1e9)
//   final, no EOS   to ~ exp(LSE_c(F_g[T][c] + trans[to][c]) + elp[T][to]),  then j ~ exp(F_g[T][j] + trans[to][j])
// Every term is >= 0 (node-local form): the rounding error of the sum scales with H itself, also where H -> 0.  Each local
// entropy is log S - A / S with its own normaliser, S = sum e^{w-m}, A = sum e^{w-m} (w - m), in fp64; a candidate of weight
// -inf contributes nothing.  A node of probability 0 is skipped; a node of non-zero probability without a finite candidate
// (or a NaN anywhere) makes the video's value NaN and sets the error word.
//
// Work split: grid (video, slab of SMM_POST_SLAB positions), thread = node (n, c), c fastest: at a fixed k the threads of a
// workgroup read consecutive doubles of F_h (a coalesced sliding window over the rows n - k), and every thread keeps an online
// (m, S, A) of its own end node: no cross-lane reduction inside the K loop.  The exponentials of that loop go through
// v_exp_f32 on fp64-shifted arguments (relative error ~1e-7 per weight); the O(T C^2) and final terms use fp64 exp.  Each
// workgroup writes one fp64 partial per video into the video's scratch rows (hT0 of smm_logz_bwd.hip, which only
// smm_marginals_kernel also uses as scratch); a second kernel sums them in a fixed order: the result is bit-identical run to run.
// The local entropies, the final decision, the node probabilities, the slabs and their sums are smm_posterior.h's: smm_kl.hip
// runs the same statements for p.
#include "smm_posterior.h"
#include "../../include/smmdp.h"

#define SMM_ENT_THREADS 256

// P(node) * H(node): 0 for a node of probability 0 (whatever its local distribution), NaN for a NaN
__device__ __forceinline__ double smm_ent_term(double lp, double h)
{
    if (lp == SMM_NEG_INF) return 0.0;
    return exp(lp) * h;
}

// H(final decision) of one video; wave-uniform result, all 64 lanes of the wave must call it
__device__ double smm_ent_final(const SmmEntropyArgs &a, const SmmVideo &mv, int vid, int T, int C, const double *F_g, int lane)
{
    // EOS: lane = the class j; no EOS: lane = to, the closing label of frame T, with the entropy of the span label in front of it
    double w = SMM_NEG_INF, hcond = 0.0, e, s;
    if (lane < C) w = smm_post_final_weight(a.h, a.p, mv, vid, T, C, F_g + (size_t)T * a.h.c_max, lane, &hcond);
    const double m = smm_group_max<64>(w);
    if (__any(w != w) || !(m > SMM_NEG_INF) || m == -SMM_NEG_INF) return __builtin_nan("");
    return smm_post_final_entropy(w, m, lane < C, a.h.no_eos, hcond, e, s);
}

__global__ void __launch_bounds__(SMM_ENT_THREADS) smm_entropy_kernel(SmmEntropyArgs a)
{
    __shared__ double s_part[1][SMM_ENT_THREADS / 64];
    const int vid = blockIdx.x, y = blockIdx.y;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max;
    const int C = a.h.n_states[g];
    if (T <= 0 || C <= 0) return;                       // (the reduction flags it)
    const int n0 = y * SMM_POST_SLAB;
    if (n0 > T) return;                                 // positions 0 .. T
    const SmmHist H = smm_hist(a.p.hist, mv, cm, T);    // (scratch: [n_slabs] partials)
    const double *trans = a.p.trans + (size_t)g * cm * cm;
    const double *len = a.p.len + (size_t)g * a.h.k_rows * cm;
    const double lz = a.p.logz[vid];
    const int tid = threadIdx.x, lane = tid & 63;
    double acc = 0.0;
    if (lz > SMM_NEG_INF && lz < -SMM_NEG_INF) {
        const int nodes = (smm_post_slab_end(n0, T) - n0) * cm;
        for (int i = tid; i < nodes; i += SMM_ENT_THREADS) {
            const int dn = i / cm, c = i - dn * cm, n = n0 + dn;
            if (c >= C) continue;
            // end node (n, c): which length the span has
            if (n >= 1) {
                const double lp = smm_post_lp_end(H, T, cm, n, c, lz);
                if (lp != SMM_NEG_INF) {
                    const int kmax = (mv.kp - 1 < n) ? mv.kp - 1 : n;
                    const double *hp = H.F.h + (size_t)n * cm + c;
                    const double *lk = len + c;
                    double m = SMM_NEG_INF, s = 0.0, ad = 0.0;
                    bool nan = false;
                    for (int k = 1; k <= kmax; ++k) {
                        const double w = hp[-(ptrdiff_t)k * cm] + lk[(size_t)k * cm];
                        nan |= (w != w);
                        smm_post_online(w, m, s, ad);
                    }
                    acc += smm_ent_term(lp, nan ? __builtin_nan("") : smm_post_ent_local(m, s, ad));
                }
            }
            // start node (n, c), 0 < n < T: which class the span in front has
            if (n >= 1 && n < T) {
                const double lp = smm_post_lp_start(H, T, cm, n, c, lz);
                if (lp != SMM_NEG_INF)
                    acc += smm_ent_term(lp, smm_post_ent_of(H.F.g + (size_t)n * cm, trans + (size_t)c * cm, C, 1));
            }
        }
        // slab 0: the final decision (wave 0)
        if (y == 0 && tid < 64) {
            const double hf = smm_ent_final(a, mv, vid, T, C, H.F.g, lane);
            if (lane == 0) acc += hf;
        }
    } else {
        acc = __builtin_nan("");
    }
    smm_post_block_sum(acc, 0.0, s_part, H.scratch, 0, y);
}

// one wave per video: the partials of its slabs in a fixed order; NaN (and the error word) for anything not finite
__global__ void __launch_bounds__(256) smm_entropy_sum_kernel(SmmEntropyArgs a)
{
    const int lane = threadIdx.x & 63;
    const int vid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (vid >= a.h.b) return;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos;
    double h[1] = {__builtin_nan("")};
    if (T > 0 && a.h.n_states[mv.group] > 0)
        smm_post_video_sum(smm_hist(a.p.hist, mv, a.h.c_max, T).scratch, smm_post_slabs(T), lane, h);
    if (lane == 0) {
        const bool ok = h[0] >= 0.0 && h[0] < -SMM_NEG_INF;
        if (!ok) atomicExch(a.h.err, 1);
        a.entropy[vid] = ok ? h[0] : __builtin_nan("");
    }
}

void smm_launch_entropy(const SmmEntropyArgs &a, int t_max, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_entropy_kernel, dim3(a.h.b, t_max / SMM_POST_SLAB + 1), dim3(SMM_ENT_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_entropy_sum_kernel, dim3((a.h.b + 3) / 4), dim3(256), 0, stream, a);
}
