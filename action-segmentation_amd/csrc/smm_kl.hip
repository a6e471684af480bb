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
// posteriors.  p's own local entropy is the entropy kernel's, operation for operation (v_exp_f32 in the K loop), so that the
// cross-entropy of p with itself is smm_entropy_f64's value.
// Support: a candidate finite under p and -inf under q makes the node's KL +inf (a legitimate value, no error); a node of
// probability 0 under p adds nothing whatever q says.  A NaN, a node of non-zero p-probability without a finite p-candidate, or a
// log Z_p that is not finite makes the video's values NaN and sets the error word.
//
// Work split as in smm_entropy.hip: grid (video, slab of SMM_KL_SLAB positions), thread = node (n, c), c fastest (the reads of
// both F_h at a fixed k are coalesced), one online normaliser per side and thread over the K loop.  Each workgroup writes one fp64
// partial per output into p's scratch rows (hT0: [KL partials | cross-entropy partials]); a second kernel sums them in a fixed
// order: the result is bit-identical run to run.
#include "smm_device.h"
#include "smm_launch.h"
#include "../../include/smmdp.h"

#define SMM_KL_SLAB 64             // positions per workgroup (= smm_entropy.hip's: the same partition, the same sums)
#define SMM_KL_THREADS 256

__device__ __forceinline__ double smm_kl_wave_max(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = fmax(x, __shfl_xor(x, off));
    return x;
}

__device__ __forceinline__ double smm_kl_wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
    return x;
}

// (smm_entropy.hip's smm_ent_local) log S - A / S, clamped at 0; NaN when no candidate was finite
__device__ __forceinline__ double smm_kl_ent_local(double m, double s, double a)
{
    if (!(m > SMM_NEG_INF)) return __builtin_nan("");
    const double h = log(s) - a / s;
    return h > 0.0 ? h : (h == h ? 0.0 : h);
}

// (smm_entropy.hip's smm_ent_of) entropy of exp(w[0..n)), fp64 throughout; NaN when no finite candidate
__device__ __forceinline__ double smm_kl_ent_of(const double *w0, const double *w1, int n, int st)
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
    return smm_kl_ent_local(m, s, a);
}

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

// EOS closing weight of class j: LSE(endpen[j], LSE_to(trans[to][j]) - 1e9)  (smm_entropy.hip's smm_ent_final)
__device__ __forceinline__ double smm_kl_wend(const double *trans, const double *endpen, int cm, int C, int j)
{
    double alt = SMM_NEG_INF;
    for (int to = 0; to < C; ++to) {
        const double t = trans[(size_t)to * cm + j], mx = fmax(alt, t);
        alt = (mx == SMM_NEG_INF) ? mx : mx + log(exp(alt - mx) + exp(t - mx));
    }
    const double ep = endpen ? endpen[j] : 0.0, b2 = alt + SMM_BIG_NEG;
    const double mx = fmax(ep, b2);
    return (mx == SMM_NEG_INF) ? mx : mx + log(exp(ep - mx) + exp(b2 - mx));
}

// no EOS: weight of the closing label `to` on one side, mx + log s + elp[T][to] (as smm_ent_final forms it); NaN for a NaN
__device__ __forceinline__ double smm_kl_to_weight(const double *Fg_T, const double *row, double elp_to, int C)
{
    double mx = SMM_NEG_INF;
    for (int c = 0; c < C; ++c) mx = fmax(mx, Fg_T[c] + row[c]);
    if (mx != mx) return mx;
    if (!(mx > SMM_NEG_INF && mx < -SMM_NEG_INF)) return SMM_NEG_INF;
    double s = 0.0;
    for (int c = 0; c < C; ++c) {
        const double d = Fg_T[c] + row[c] - mx;
        if (d > SMM_NEG_INF) s += exp(d);
    }
    return mx + log(s) + elp_to;
}

// H(final decision) of p and KL(final decision) of p against q, one video; wave-uniform results, all 64 lanes must call it
__device__ void smm_kl_final(const SmmKlArgs &a, const SmmVideo &mv, int vid, int T, int C, const double *Fp_g,
                             const double *Fq_g, int lane, double *h_out, double *kl_out)
{
    const int cm = a.c_max, g = mv.group;
    const double *trp = a.trans_p + (size_t)g * cm * cm, *trq = a.trans_q + (size_t)g * cm * cm;
    double wp = SMM_NEG_INF, wq = SMM_NEG_INF, hcond = 0.0, kcond = 0.0;
    bool nan = false;
    if (lane < C) {
        if (!a.no_eos) {
            wp = Fp_g[(size_t)T * cm + lane] + smm_kl_wend(trp, a.endpen_p ? a.endpen_p + (size_t)vid * cm : nullptr, cm, C, lane);
            wq = Fq_g[(size_t)T * cm + lane] + smm_kl_wend(trq, a.endpen_q ? a.endpen_q + (size_t)vid * cm : nullptr, cm, C, lane);
        } else {
            // lane = to: the closing label of frame T; the entropy (p) and KL (p against q) of the span label in front of it
            const double *rp = trp + (size_t)lane * cm, *rq = trq + (size_t)lane * cm;
            const double *Fp = Fp_g + (size_t)T * cm, *Fq = Fq_g + (size_t)T * cm;
            const size_t fr = (size_t)(mv.frame_off + T) * cm + lane;
            // p: smm_ent_final's own operations (its conditional entropy and weight)
            double mx = SMM_NEG_INF;
            for (int c = 0; c < C; ++c) mx = fmax(mx, Fp[c] + rp[c]);
            double s = 0.0, acc = 0.0;
            if (mx > SMM_NEG_INF && mx < -SMM_NEG_INF) {
                for (int c = 0; c < C; ++c) {
                    const double d = Fp[c] + rp[c] - mx;
                    if (d > SMM_NEG_INF) {
                        const double e = exp(d);
                        s += e;
                        acc += e * d;
                    }
                }
                hcond = smm_kl_ent_local(mx, s, acc);
                wp = mx + log(s) + a.elp_p[fr];
                kcond = smm_kl_of(Fp, rp, Fq, rq, C, 1);
            } else if (mx != mx) {
                nan = true;
            }
            wq = smm_kl_to_weight(Fq, rq, a.elp_q[fr], C);
        }
        nan |= (wp != wp) | (wq != wq);
    }
    const double mp = smm_kl_wave_max(wp), mq = smm_kl_wave_max(wq);
    const int any_nan = __any(nan);
    if (any_nan || !(mp > SMM_NEG_INF) || mp == -SMM_NEG_INF || mq == -SMM_NEG_INF) {
        *h_out = *kl_out = __builtin_nan("");
        return;
    }
    // p's entropy of the decision: smm_ent_final's operations
    const double d = wp - mp;
    const double e = (lane < C && d > SMM_NEG_INF) ? exp(d) : 0.0;
    const double s = smm_kl_wave_sum(e), ad = smm_kl_wave_sum(e > 0.0 ? e * d : 0.0);
    double h = smm_kl_ent_local(mp, s, ad);
    // its KL: the same weights e on p's side
    const double dq = wq - mq;
    const double eq = (lane < C && dq > SMM_NEG_INF) ? exp(dq) : 0.0;
    const double sq = smm_kl_wave_sum(eq);
    const double y = smm_kl_wave_sum((e > 0.0 && wq > SMM_NEG_INF) ? e * (wq - wp) : 0.0);
    const int qinf = __any(e > 0.0 && !(wq > SMM_NEG_INF));
    double kl = smm_kl_local(mp, s, y, mq, sq, qinf != 0);
    if (a.no_eos) {
        // + sum_to P_p(to) H(j | to), + sum_to P_p(to) KL(j | to); a `to` of p-probability 0 does not count
        const double t = (e > 0.0) ? (e / s) * hcond : 0.0;
        h += smm_kl_wave_sum(t);
        const double u = (e > 0.0) ? (kcond == -SMM_NEG_INF ? kcond : (e / s) * kcond) : 0.0;
        kl += smm_kl_wave_sum(u);
    }
    *h_out = h;
    *kl_out = kl;
}

__global__ void __launch_bounds__(SMM_KL_THREADS) smm_kl_kernel(SmmKlArgs a)
{
    __shared__ double s_part[2][SMM_KL_THREADS / 64];
    const int vid = blockIdx.x, y = blockIdx.y;
    const SmmVideo mv = a.videos[vid];
    const int T = mv.T - a.no_eos, g = mv.group, cm = a.c_max;
    const int C = a.n_states[g];
    if (T <= 0 || C <= 0) return;                       // (the reduction flags it)
    const int n0 = y * SMM_KL_SLAB;
    if (n0 > T) return;                                 // positions 0 .. T
    const size_t blk = (size_t)cm * (T + 1);
    const double *F_cum = a.hist_p + mv.hist_off, *F_h = F_cum + blk, *F_g = F_h + blk;
    const double *B_cum = F_g + blk, *B_h = B_cum + blk, *B_g = B_h + blk;
    const double *Q_h = a.hist_q + mv.hist_off + blk, *Q_g = Q_h + blk;
    double *part = const_cast<double *>(B_g + blk);    // [2][n_slabs] (p's hT0: scratch)
    const int ns = T / SMM_KL_SLAB + 1;
    const double *trp = a.trans_p + (size_t)g * cm * cm, *trq = a.trans_q + (size_t)g * cm * cm;
    const double *lenp = a.len_p + (size_t)g * a.k_rows * cm, *lenq = a.len_q + (size_t)g * a.k_rows * cm;
    const double lz = a.logz_p[vid], lzq = a.logz_q[vid];
    const int tid = threadIdx.x, lane = tid & 63;
    double acc = 0.0, accx = 0.0;                       // KL, cross-entropy
    if (lz > SMM_NEG_INF && lz < -SMM_NEG_INF && lzq > SMM_NEG_INF && lzq < -SMM_NEG_INF) {
        const int n1 = (n0 + SMM_KL_SLAB <= T) ? n0 + SMM_KL_SLAB : T + 1;
        const int nodes = (n1 - n0) * cm;
        for (int i = tid; i < nodes; i += SMM_KL_THREADS) {
            const int dn = i / cm, c = i - dn * cm, n = n0 + dn;
            if (c >= C) continue;
            // end node (n, c): which length the span has
            if (n >= 1) {
                const double lp = F_g[(size_t)n * cm + c] + B_h[(size_t)(T - n) * cm + c] + B_cum[(size_t)(T - n) * cm + c] - lz;
                if (lp != SMM_NEG_INF) {
                    const int kmax = (mv.kp - 1 < n) ? mv.kp - 1 : n;
                    const double *hp = F_h + (size_t)n * cm + c, *hq = Q_h + (size_t)n * cm + c;
                    const double *lkp = lenp + c, *lkq = lenq + c;
                    double m = SMM_NEG_INF, s = 0.0, ad = 0.0;          // p, the entropy kernel's normaliser (v_exp_f32)
                    double sp = 0.0, yy = 0.0;                           // p, fp64 (same maximum m)
                    double mq = SMM_NEG_INF, sq = 0.0;                   // q, fp64
                    bool nan = false, qinf = false;
                    for (int k = 1; k <= kmax; ++k) {
                        const double w = hp[-(ptrdiff_t)k * cm] + lkp[(size_t)k * cm];
                        const double wq = hq[-(ptrdiff_t)k * cm] + lkq[(size_t)k * cm];
                        nan |= (w != w) | (wq != wq);
                        const bool both = wq > SMM_NEG_INF;
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
                    const double h = nan ? __builtin_nan("") : smm_kl_ent_local(m, s, ad);
                    const double kl = nan ? __builtin_nan("") : smm_kl_local(m, sp, yy, mq, sq, qinf);
                    acc += smm_kl_term(lp, kl);
                    accx += smm_kl_term(lp, h + kl);
                }
            }
            // start node (n, c), 0 < n < T: which class the span in front has
            if (n >= 1 && n < T) {
                const double lp = F_h[(size_t)n * cm + c] + F_cum[(size_t)n * cm + c] + B_g[(size_t)(T - n) * cm + c] - lz;
                if (lp != SMM_NEG_INF) {
                    const double h = smm_kl_ent_of(F_g + (size_t)n * cm, trp + (size_t)c * cm, C, 1);
                    const double kl = smm_kl_of(F_g + (size_t)n * cm, trp + (size_t)c * cm, Q_g + (size_t)n * cm,
                                                trq + (size_t)c * cm, C, 1);
                    acc += smm_kl_term(lp, kl);
                    accx += smm_kl_term(lp, h + kl);
                }
            }
        }
        // slab 0: the final decision (wave 0)
        if (y == 0 && tid < 64) {
            double hf, kf;
            smm_kl_final(a, mv, vid, T, C, F_g, Q_g, lane, &hf, &kf);
            if (lane == 0) {
                acc += kf;
                accx += hf + kf;
            }
        }
    } else if (lz > SMM_NEG_INF && lz < -SMM_NEG_INF && lzq == SMM_NEG_INF) {
        // q gives every segmentation probability 0: +inf, unless a NaN in q's inputs is why (the log Z recursion closes a NaN
        // to -inf; its histories keep it)
        const int n1 = (n0 + SMM_KL_SLAB <= T) ? n0 + SMM_KL_SLAB : T + 1;
        bool nan = false;
        for (int i = tid; i < (n1 - n0) * cm; i += SMM_KL_THREADS) {
            const int dn = i / cm, c = i - dn * cm, n = n0 + dn;
            if (c >= C) continue;
            const double h = Q_h[(size_t)n * cm + c], gg = Q_g[(size_t)n * cm + c];
            nan |= (h != h) | (gg != gg);
        }
        acc = accx = nan ? __builtin_nan("") : -SMM_NEG_INF;
    } else {
        acc = accx = __builtin_nan("");
    }
    // fixed-order reduction: butterfly within each wave, then the waves in order
    acc = smm_kl_wave_sum(acc);
    accx = smm_kl_wave_sum(accx);
    if (lane == 0) {
        s_part[0][tid >> 6] = acc;
        s_part[1][tid >> 6] = accx;
    }
    __syncthreads();
    if (tid < 2) {
        double t = s_part[tid][0];
#pragma unroll
        for (int w = 1; w < SMM_KL_THREADS / 64; ++w) t += s_part[tid][w];
        part[(size_t)tid * ns + y] = t;
    }
}

// one wave per video: the partials of its slabs in a fixed order; NaN (and the error word) for anything not in [0, +inf]
__global__ void __launch_bounds__(256) smm_kl_sum_kernel(SmmKlArgs a)
{
    const int lane = threadIdx.x & 63;
    const int vid = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (vid >= a.b) return;
    const SmmVideo mv = a.videos[vid];
    const int T = mv.T - a.no_eos, cm = a.c_max;
    const int C = a.n_states[mv.group];
    double kl = __builtin_nan(""), x = __builtin_nan("");
    if (T > 0 && C > 0) {
        const size_t blk = (size_t)cm * (T + 1);
        const double *part = a.hist_p + mv.hist_off + 6 * blk;
        const int ns = T / SMM_KL_SLAB + 1;
        double t = 0.0, u = 0.0;
        for (int q = lane; q < ns; q += 64) {
            t += part[q];
            u += part[ns + q];
        }
        kl = smm_kl_wave_sum(t);
        x = smm_kl_wave_sum(u);
    }
    if (lane == 0) {
        const bool ok = kl >= 0.0 && x >= 0.0;         // (+inf included: p-mass where q has none)
        if (!ok) atomicExch(a.err, 1);
        a.kl[vid] = ok ? kl : __builtin_nan("");
        if (a.xent) a.xent[vid] = ok ? x : __builtin_nan("");
    }
}

void smm_launch_kl(const SmmKlArgs &a, int t_max, hipStream_t stream)
{
    const int slabs = t_max / SMM_KL_SLAB + 1;
    hipLaunchKernelGGL(smm_kl_kernel, dim3(a.b, slabs), dim3(SMM_KL_THREADS), 0, stream, a);
    hipLaunchKernelGGL(smm_kl_sum_kernel, dim3((a.b + 3) / 4), dim3(256), 0, stream, a);
}
