// smm_kl.hip -- exact KL(p || q) = sum_y p(y | x) log(p(y | x) / q(y | x)) between two segmentation posteriors of the same
// lattice (same videos, lengths, class sets, span limit; other tables), and the cross-entropy H(p, q) = H(p) + KL(p || q).
//
// y is in one-to-one correspondence with the decisions of the backward walk smm_sample.hip draws; for p and q alike that walk
// is a Markov chain over the same decision nodes, so by the chain rule of relative entropy
//   KL(p || q) = KL(final decision)
//              + sum_{n >= 1, c}  P_p(a span of c ends at n)   * KL(p(k | end (n, c))    || q(k | end (n, c)))      O(T K C)
//              + sum_{0 < s, c}   P_p(a span of c starts at s) * KL(p(c' | start (s, c)) || q(c' | start (s, c)))  O(T C^2)
// The node probabilities are p's (smm_entropy.hip: p's forward and backward histories and log Z_p).  The local distributions
// are the sampler's, each side on its own forward histories and tables (q needs no backward pass; log Z_q does not enter):
//   end (n, c)      k  ~ exp(F_h[n-k][c] + len[k][c]),  k = 1 .. min(kp-1, n)
//   start (s, c)    c' ~ exp(F_g[s][c'] + trans[c][c'])
//   final, EOS      j  ~ exp(F_g[T][j] + wend[j])
//   final, no EOS   to ~ exp(LSE_c(F_g[T][c] + trans[to][c]) + elp[T][to]),  then j ~ exp(F_g[T][j] + trans[to][j])
// Each local KL is (m_q - m_p) + log S_q - log S_p - Y / S_p with S = sum e^{w-m} per side and Y = sum e^{w_p-m_p} (w_q - w_p)
// over the candidates finite on both sides: identically 0 when the two weight vectors are equal (both sides run the same
// operations), clamped at 0 against rounding otherwise.  Its exponentials are fp64: at a per-weight error of ~1e-7 (v_exp_f32)
// the difference log S_q - log S_p would carry ~1e-7 absolute per node, as large as the whole KL of two near-identical
// posteriors.  p's own local entropy is the entropy kernel's: both call smm_posterior.h (smm_post_ent_local, smm_post_ent_of,
// smm_post_final_weight / smm_post_final_entropy); only the K loop's online step with v_exp_f32 is written out here a second
// time, operation for operation, with the fp64 sums in its branches.  So the cross-entropy of p with itself is
// smm_entropy_f64's value.
// Support: a candidate finite under p and -inf under q makes the node's KL +inf (a legitimate value, no error); a node of
// probability 0 under p adds nothing whatever q says.  A NaN, a node of non-zero p-probability without a finite p-candidate, or a
// log Z_p that is not finite makes the video's values NaN and sets the error word.
//
// Work split as in smm_entropy.hip: grid (video, slab of SMM_POST_SLAB positions), thread = node (n, c), c fastest (the reads of
// both F_h at a fixed k are coalesced), one online normaliser per side and thread over the K loop.  Each workgroup writes one fp64
// partial per output into p's scratch rows (hT0: [KL partials | cross-entropy partials]); a second kernel sums them in a fixed
// order: the result is bit-identical run to run.
#include "smm_posterior.h"
#include "../../include/smmdp.h"

#define SMM_KL_THREADS 256

// the local KL from the two normalisers: NaN without a finite p-candidate, +inf for p-mass where q has none, else >= 0
__device__ __forceinline__ double smm_kl_local(double mp, double sp, double y, double mq, double sq, bool qinf)
{
    if (!(mp > SMM_NEG_INF)) return __builtin_nan("");
    if (qinf || !(mq > SMM_NEG_INF)) return -SMM_NEG_INF;
    const double kl = ((mq - mp) + (log(sq) - log(sp))) - y / sp;
    return kl > 0.0 ? kl : (kl == kl ? 0.0 : kl);
}

// KL of exp(p0[i*st] + p1[i]) against exp(q0[i*st] + q1[i]), i < n, fp64 throughout
__device__ __forceinline__ double smm_kl_of(const double *p0, const double *p1, const double *q0, const double *q1, int n, int st)
{
    double mp = SMM_NEG_INF, mq = SMM_NEG_INF;
    bool nan = false;
    for (int i = 0; i < n; ++i) {
        const double wp = p0[(size_t)i * st] + p1[i], wq = q0[(size_t)i * st] + q1[i];
        nan |= (wp != wp) | (wq != wq);
        mp = fmax(mp, wp);
        mq = fmax(mq, wq);
    }
    if (nan || mp == -SMM_NEG_INF || mq == -SMM_NEG_INF) return __builtin_nan("");
    double sp = 0.0, sq = 0.0, y = 0.0;
    bool qinf = false;
    for (int i = 0; i < n; ++i) {
        const double wp = p0[(size_t)i * st] + p1[i], wq = q0[(size_t)i * st] + q1[i];
        const double dp = wp - mp, dq = wq - mq;
        if (dp > SMM_NEG_INF) {
            const double e = exp(dp);
            sp += e;
            if (wq > SMM_NEG_INF) y += e * (wq - wp);
            else qinf = true;
        }
        if (dq > SMM_NEG_INF) sq += exp(dq);
    }
    return smm_kl_local(mp, sp, y, mq, sq, qinf);
}

// P(node) * local value: 0 for a node of probability 0 (whatever its local distributions), +inf for +inf, NaN for a NaN
__device__ __forceinline__ double smm_kl_term(double lp, double v)
{
    if (lp == SMM_NEG_INF) return 0.0;
    if (v == -SMM_NEG_INF && lp == lp) return v;
    return exp(lp) * v;
}

// H(final decision) of p and KL(final decision) of p against q, one video; wave-uniform results, all 64 lanes must call it
__device__ void smm_kl_final(const SmmKlArgs &a, const SmmVideo &mv, int vid, int T, int C, const double *Fp_g,
                             const double *Fq_g, int lane, double *h_out, double *kl_out)
{
    const int cm = a.h.c_max;
    const double *Fp = Fp_g + (size_t)T * cm, *Fq = Fq_g + (size_t)T * cm;
    double wp = SMM_NEG_INF, wq = SMM_NEG_INF, hcond = 0.0, kcond = 0.0;
    if (lane < C) {
        // EOS: lane = the class j; no EOS: lane = to, the closing label of frame T, with the entropy (p) and KL (p against q)
        // of the span label in front of it
        wp = smm_post_final_weight(a.h, a.p, mv, vid, T, C, Fp, lane, &hcond);
        wq = smm_post_final_weight(a.h, a.q, mv, vid, T, C, Fq, lane);
        if (a.h.no_eos && wp > SMM_NEG_INF) {           // (a `to` without p-mass is never weighed)
            const size_t row = ((size_t)mv.group * cm + lane) * cm;
            kcond = smm_kl_of(Fp, a.p.trans + row, Fq, a.q.trans + row, C, 1);
        }
    }
    const double mp = smm_group_max<64>(wp), mq = smm_group_max<64>(wq);
    if (__any((wp != wp) | (wq != wq)) || !(mp > SMM_NEG_INF) || mp == -SMM_NEG_INF || mq == -SMM_NEG_INF) {
        *h_out = *kl_out = __builtin_nan("");
        return;
    }
    double e, s;
    *h_out = smm_post_final_entropy(wp, mp, lane < C, a.h.no_eos, hcond, e, s);
    // its KL: the same weights e on p's side
    const double dq = wq - mq;
    const double eq = (lane < C && dq > SMM_NEG_INF) ? exp(dq) : 0.0;
    const double sq = smm_group_sum<64>(eq);
    const double y = smm_group_sum<64>((e > 0.0 && wq > SMM_NEG_INF) ? e * (wq - wp) : 0.0);
    const int qinf = __any(e > 0.0 && !(wq > SMM_NEG_INF));
    double kl = smm_kl_local(mp, s, y, mq, sq, qinf != 0);
    if (a.h.no_eos) {
        // + sum_to P_p(to) KL(j | to); a `to` of p-probability 0 does not count
        const double u = (e > 0.0) ? (kcond == -SMM_NEG_INF ? kcond : (e / s) * kcond) : 0.0;
        kl += smm_group_sum<64>(u);
    }
    *kl_out = kl;
}

__global__ void __launch_bounds__(SMM_KL_THREADS) smm_kl_kernel(SmmKlArgs a)
{
    __shared__ double s_part[2][SMM_KL_THREADS / 64];
    const int vid = blockIdx.x, y = blockIdx.y;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max;
    const int C = a.h.n_states[g];
    if (T <= 0 || C <= 0) return;                       // (the reduction flags it)
    const int n0 = y * SMM_POST_SLAB;
    if (n0 > T) return;                                 // positions 0 .. T
    const SmmHist H = smm_hist(a.p.hist, mv, cm, T);    // (scratch: [2][n_slabs], KL partials | cross-entropy partials)
    const SmmHistDir Q = smm_hist_dir(a.q.hist, mv, cm, T, 0);
    const double *trp = a.p.trans + (size_t)g * cm * cm, *trq = a.q.trans + (size_t)g * cm * cm;
    const double *lenp = a.p.len + (size_t)g * a.h.k_rows * cm, *lenq = a.q.len + (size_t)g * a.h.k_rows * cm;
    const double lz = a.p.logz[vid], lzq = a.q.logz[vid];
    const int tid = threadIdx.x, lane = tid & 63;
    const int nodes = (smm_post_slab_end(n0, T) - n0) * cm;
    double acc = 0.0, accx = 0.0;                       // KL, cross-entropy
    if (lz > SMM_NEG_INF && lz < -SMM_NEG_INF && lzq > SMM_NEG_INF && lzq < -SMM_NEG_INF) {
        for (int i = tid; i < nodes; i += SMM_KL_THREADS) {
            const int dn = i / cm, c = i - dn * cm, n = n0 + dn;
            if (c >= C) continue;
            // end node (n, c): which length the span has
            if (n >= 1) {
                const double lp = smm_post_lp_end(H, T, cm, n, c, lz);
                if (lp != SMM_NEG_INF) {
                    const int kmax = (mv.kp - 1 < n) ? mv.kp - 1 : n;
                    const double *hp = H.F.h + (size_t)n * cm + c, *hq = Q.h + (size_t)n * cm + c;
                    const double *lkp = lenp + c, *lkq = lenq + c;
                    double m = SMM_NEG_INF, s = 0.0, ad = 0.0;          // p, smm_post_online's normaliser (v_exp_f32) 
                    double sp = 0.0, yy = 0.0;                           // p, fp64 (same maximum m)
                    double mq = SMM_NEG_INF, sq = 0.0;                   // q, fp64
                    bool nan = false, qinf = false;
                    for (int k = 1; k <= kmax; ++k) {
                        const double w = hp[-(ptrdiff_t)k * cm] + lkp[(size_t)k * cm];
                        const double wq = hq[-(ptrdiff_t)k * cm] + lkq[(size_t)k * cm];
                        nan |= (w != w) | (wq != wq);
                        const bool both = wq > SMM_NEG_INF;
                        // p: smm_post_online's step with the fp64 sums in its branches (the one remaining copy: with the sums
                        // apart, under the same conditions, the kernel was 4 % slower)
                        const double d = w - m;
                        if (d > 0.0) {                                         // a new maximum (or the first finite one)
                            const double r = (double)__expf((float)-d);        // (m = -inf: d = inf, r = 0)
                            ad = r * (ad - (s > 0.0 ? s * d : 0.0));
                            s = r * s + 1.0;
                            const double r64 = exp(-d);
                            sp = r64 * sp + 1.0;
                            yy = r64 * yy + (both ? wq - w : 0.0);
                            qinf |= !both;
                            m = w;
                        } else if (w > SMM_NEG_INF) {
                            const double e = (double)__expf((float)d);
                            s += e;
                            ad += e * d;
                            const double e64 = exp(d);
                            sp += e64;
                            yy += both ? e64 * (wq - w) : 0.0;
                            qinf |= !both;
                        }
                        const double dq = wq - mq;
                        if (dq > 0.0) {
                            sq = exp(-dq) * sq + 1.0;
                            mq = wq;
                        } else if (wq > SMM_NEG_INF) {
                            sq += exp(dq);
                        }
                    }
                    const double h = nan ? __builtin_nan("") : smm_post_ent_local(m, s, ad);
                    const double kl = nan ? __builtin_nan("") : smm_kl_local(m, sp, yy, mq, sq, qinf);
                    acc += smm_kl_term(lp, kl);
                    accx += smm_kl_term(lp, h + kl);
                }
            }
            // start node (n, c), 0 < n < T: which class the span in front has
            if (n >= 1 && n < T) {
                const double lp = smm_post_lp_start(H, T, cm, n, c, lz);
                if (lp != SMM_NEG_INF) {
                    const double h = smm_post_ent_of(H.F.g + (size_t)n * cm, trp + (size_t)c * cm, C, 1);
                    const double kl = smm_kl_of(H.F.g + (size_t)n * cm, trp + (size_t)c * cm, Q.g + (size_t)n * cm,
                                                trq + (size_t)c * cm, C, 1);
                    acc += smm_kl_term(lp, kl);
                    accx += smm_kl_term(lp, h + kl);
                }
            }
        }
        // slab 0: the final decision (wave 0)
        if (y == 0 && tid < 64) {
            double hf, kf;
            smm_kl_final(a, mv, vid, T, C, H.F.g, Q.g, lane, &hf, &kf);
            if (lane == 0) {
                acc += kf;
                accx += hf + kf;
            }
        }
    } else if (lz > SMM_NEG_INF && lz < -SMM_NEG_INF && lzq == SMM_NEG_INF) {
        // q gives every segmentation probability 0: +inf, unless a NaN in q's inputs is why (the log Z recursion closes a NaN
        // to -inf; its histories keep it)
        bool nan = false;
        for (int i = tid; i < nodes; i += SMM_KL_THREADS) {
            const int dn = i / cm, c = i - dn * cm, n = n0 + dn;
            if (c >= C) continue;
            const double h = Q.h[(size_t)n * cm + c], gg = Q.g[(size_t)n * cm + c];
            nan |= (h != h) | (gg != gg);
        }
        acc = accx = nan ? __builtin_nan("") : -SMM_NEG_INF;
    } else {
        acc = accx = __builtin_nan("");
    }
    smm_post_block_sum(acc, accx, s_part, H.scratch, smm_post_slabs(T), y);
}

// one wave per video: the partials of its slabs in a fixed order; NaN (and the error word) for anything not in [0, +inf]
__global__ void __launch_bounds__(256) smm_kl_sum_kernel(SmmKlArgs a)
{
    const int lane = threadIdx.x & 63;
    const int vid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (vid >= a.h.b) return;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos;
    double v[2] = {__builtin_nan(""), __builtin_nan("")};         // KL, cross-entropy
    if (T > 0 && a.h.n_states[mv.group] > 0)
        smm_post_video_sum(smm_hist(a.p.hist, mv, a.h.c_max, T).scratch, smm_post_slabs(T), lane, v);
    if (lane == 0) {
        const bool ok = v[0] >= 0.0 && v[1] >= 0.0;     // (+inf included: p-mass where q has none)
        if (!ok) atomicExch(a.h.err, 1);
        a.kl[vid] = ok ? v[0] : __builtin_nan("");
        if (a.xent) a.xent[vid] = ok ? v[1] : __builtin_nan("");
    }
}

void smm_launch_kl(const SmmKlArgs &a, int t_max, hipStream_t stream)
{
    hipLaunchKernelGGL(smm_kl_kernel, dim3(a.h.b, t_max / SMM_POST_SLAB + 1), dim3(SMM_KL_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_kl_sum_kernel, dim3((a.h.b + 3) / 4), dim3(256), 0, stream, a);
}
