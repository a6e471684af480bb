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
// Work split: grid (video, slab of SMM_ENT_SLAB positions), thread = node (n, c), c fastest: at a fixed k the threads of a
// workgroup read consecutive doubles of F_h (a coalesced sliding window over the rows n - k), and every thread keeps an online
// (m, S, A) of its own end node: no cross-lane reduction inside the K loop.  The exponentials of that loop go through
// v_exp_f32 on fp64-shifted arguments (relative error ~1e-7 per weight); the O(T C^2) and final terms use fp64 exp.  Each
// workgroup writes one fp64 partial per video into the video's scratch rows (hT0 of smm_logz_bwd.hip, which only
// smm_marginals_kernel also uses as scratch); a second kernel sums them in a fixed order: the result is bit-identical run to run.
#include "smm_device.h"
#include "smm_launch.h"
#include "../../include/smmdp.h"

#define SMM_ENT_SLAB 64            // positions per workgroup
#define SMM_ENT_THREADS 256

__device__ __forceinline__ double smm_ent_wave_max(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = fmax(x, __shfl_xor(x, off));
    return x;
}

__device__ __forceinline__ double smm_ent_wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// log S - A / S, clamped at 0 (rounding); NaN when no candidate was finite
__device__ __forceinline__ double smm_ent_local(double m, double s, double a)
{
    if (!(m > SMM_NEG_INF)) return __builtin_nan("");
    const double h = log(s) - a / s;
    return h > 0.0 ? h : (h == h ? 0.0 : h);
}

// entropy of the distribution exp(w[0..n)) (w[i] at stride `st`), fp64 throughout; NaN when no finite candidate
__device__ __forceinline__ double smm_ent_of(const double *w0, const double *w1, int n, int st)
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
    return smm_ent_local(m, s, a);
}

// P(node) * H(node): 0 for a node of probability 0 (whatever its local distribution), NaN for a NaN
__device__ __forceinline__ double smm_ent_term(double lp, double h)
{
    if (lp == SMM_NEG_INF) return 0.0;
    return exp(lp) * h;
}

// H(final decision) of one video; wave-uniform result, all 64 lanes of the wave must call it
__device__ double smm_ent_final(const SmmEntropyArgs &a, const SmmVideo &mv, int vid, int T, int C, const double *F_g, int lane)
{
    const int cm = a.c_max, g = mv.group;
    const double *trans = a.trans + (size_t)g * cm * cm;
    double w = SMM_NEG_INF, hcond = 0.0;
    bool nan = false;
    if (lane < C) {
        if (!a.no_eos) {
            double alt = SMM_NEG_INF;
            for (int to = 0; to < C; ++to) {
                const double t = trans[(size_t)to * cm + lane], mx = fmax(alt, t);
                alt = (mx == SMM_NEG_INF) ? mx : mx + log(exp(alt - mx) + exp(t - mx));
            }
            const double ep = a.endpen ? a.endpen[(size_t)vid * cm + lane] : 0.0, b2 = alt + SMM_BIG_NEG;
            const double mx = fmax(ep, b2);
            const double wend = (mx == SMM_NEG_INF) ? mx : mx + log(exp(ep - mx) + exp(b2 - mx));
            w = F_g[(size_t)T * cm + lane] + wend;
        } else {
            // lane = to: the closing label of frame T, and the entropy of the span label in front of it given `to`
            const double *row = trans + (size_t)lane * cm;
            double mx = SMM_NEG_INF;
            for (int c = 0; c < C; ++c) mx = fmax(mx, F_g[(size_t)T * cm + c] + row[c]);
            double s = 0.0, acc = 0.0;
            if (mx > SMM_NEG_INF && mx < -SMM_NEG_INF) {
                for (int c = 0; c < C; ++c) {
                    const double d = F_g[(size_t)T * cm + c] + row[c] - mx;
                    if (d > SMM_NEG_INF) {
                        const double e = exp(d);
                        s += e;
                        acc += e * d;
                    }
                }
                hcond = smm_ent_local(mx, s, acc);
                w = mx + log(s) + a.elp[(size_t)(mv.frame_off + T) * cm + lane];
            } else if (mx != mx) {
                nan = true;
            }
        }
        nan |= (w != w);
    }
    const double m = smm_ent_wave_max(w);
    const int any_nan = __any(nan);
    if (any_nan || !(m > SMM_NEG_INF) || m == -SMM_NEG_INF) return __builtin_nan("");
    const double d = w - m;
    const double e = (lane < C && d > SMM_NEG_INF) ? exp(d) : 0.0;
    const double s = smm_ent_wave_sum(e), ad = smm_ent_wave_sum(e > 0.0 ? e * d : 0.0);
    double h = smm_ent_local(m, s, ad);
    if (a.no_eos) {
        // + sum_to P(to) H(j | to); a `to` of probability 0 does not count
        const double t = (e > 0.0) ? (e / s) * hcond : 0.0;
        h += smm_ent_wave_sum(t);
    }
    return h;
}

__global__ void __launch_bounds__(SMM_ENT_THREADS) smm_entropy_kernel(SmmEntropyArgs a)
{
    __shared__ double s_part[SMM_ENT_THREADS / 64];
    const int vid = blockIdx.x, y = blockIdx.y;
    const SmmVideo mv = a.videos[vid];
    const int T = mv.T - a.no_eos, g = mv.group, cm = a.c_max;
    const int C = a.n_states[g];
    if (T <= 0 || C <= 0) return;                       // (the reduction flags it)
    const int n0 = y * SMM_ENT_SLAB;
    if (n0 > T) return;                                 // positions 0 .. T
    const size_t blk = (size_t)cm * (T + 1);
    const double *F_cum = a.hist + mv.hist_off, *F_h = F_cum + blk, *F_g = F_h + blk;
    const double *B_cum = F_g + blk, *B_h = B_cum + blk, *B_g = B_h + blk;
    double *part = const_cast<double *>(B_g + blk);    // [n_slabs] (hT0: scratch)
    const double *trans = a.trans + (size_t)g * cm * cm;
    const double *len = a.len + (size_t)g * a.k_rows * cm;
    const double lz = a.logz[vid];
    const int tid = threadIdx.x, lane = tid & 63;
    double acc = 0.0;
    if (lz > SMM_NEG_INF && lz < -SMM_NEG_INF) {
        const int n1 = (n0 + SMM_ENT_SLAB <= T) ? n0 + SMM_ENT_SLAB : T + 1;
        const int nodes = (n1 - n0) * cm;
        for (int i = tid; i < nodes; i += SMM_ENT_THREADS) {
            const int dn = i / cm, c = i - dn * cm, n = n0 + dn;
            if (c >= C) continue;
            // end node (n, c): which length the span has
            if (n >= 1) {
                const double lp = F_g[(size_t)n * cm + c] + B_h[(size_t)(T - n) * cm + c] + B_cum[(size_t)(T - n) * cm + c] - lz;
                if (lp != SMM_NEG_INF) {
                    const int kmax = (mv.kp - 1 < n) ? mv.kp - 1 : n;
                    const double *hp = F_h + (size_t)n * cm + c;
                    const double *lk = len + c;
                    double m = SMM_NEG_INF, s = 0.0, ad = 0.0;
                    bool nan = false;
                    for (int k = 1; k <= kmax; ++k) {
                        const double w = hp[-(ptrdiff_t)k * cm] + lk[(size_t)k * cm];
                        nan |= (w != w);
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
                    acc += smm_ent_term(lp, nan ? __builtin_nan("") : smm_ent_local(m, s, ad));
                }
            }
            // start node (n, c), 0 < n < T: which class the span in front has
            if (n >= 1 && n < T) {
                const double lp = F_h[(size_t)n * cm + c] + F_cum[(size_t)n * cm + c] + B_g[(size_t)(T - n) * cm + c] - lz;
                if (lp != SMM_NEG_INF)
                    acc += smm_ent_term(lp, smm_ent_of(F_g + (size_t)n * cm, trans + (size_t)c * cm, C, 1));
            }
        }
        // slab 0: the final decision (wave 0)
        if (y == 0 && tid < 64) {
            const double hf = smm_ent_final(a, mv, vid, T, C, F_g, lane);
            if (lane == 0) acc += hf;
        }
    } else {
        acc = __builtin_nan("");
    }
    // fixed-order reduction: butterfly within each wave, then the waves in order
    acc = smm_ent_wave_sum(acc);
    if (lane == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double t = s_part[0];
#pragma unroll
        for (int w = 1; w < SMM_ENT_THREADS / 64; ++w) t += s_part[w];
        part[y] = t;
    }
}

// one wave per video: the partials of its slabs in a fixed order; NaN (and the error word) for anything not finite
__global__ void __launch_bounds__(256) smm_entropy_sum_kernel(SmmEntropyArgs a)
{
    const int lane = threadIdx.x & 63;
    const int vid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (vid >= a.b) return;
    const SmmVideo mv = a.videos[vid];
    const int T = mv.T - a.no_eos, cm = a.c_max;
    const int C = a.n_states[mv.group];
    double h = __builtin_nan("");
    if (T > 0 && C > 0) {
        const size_t blk = (size_t)cm * (T + 1);
        const double *part = a.hist + mv.hist_off + 6 * blk;
        const int ns = T / SMM_ENT_SLAB + 1;
        double t = 0.0;
        for (int q = lane; q < ns; q += 64) t += part[q];
        h = smm_ent_wave_sum(t);
    }
    if (lane == 0) {
        const bool ok = h >= 0.0 && h < -SMM_NEG_INF;
        if (!ok) atomicExch(a.err, 1);
        a.entropy[vid] = ok ? h : __builtin_nan("");
    }
}

void smm_launch_entropy(const SmmEntropyArgs &a, int t_max, hipStream_t stream)
{
    const int slabs = t_max / SMM_ENT_SLAB + 1;
    hipLaunchKernelGGL(smm_entropy_kernel, dim3(a.b, slabs), dim3(SMM_ENT_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_entropy_sum_kernel, dim3((a.b + 3) / 4), dim3(256), 0, stream, a);
}
