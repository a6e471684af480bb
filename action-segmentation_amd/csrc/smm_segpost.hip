// smm_segpost.hip -- exact posterior of segment boundaries and of given segments under the semi-Markov posterior p(y | x).
//
// Inputs are the two histories smm_logz_bwd.hip's header lays out (forward F_cum, F_h, F_g; backward B_cum, B_h, B_g).  With
// them every quantity here is local (T = the video's DP positions, mv.T - no_eos; frame f = position f):
//   start_post[f][c] = P(a span of c starts at f)            = exp(smm_post_lp_start(f, c)),      f < T
//   end_post[f][c]   = P(a span of c has f as its last frame) = exp(smm_post_lp_end(f + 1, c)),    f < T
//   bnd_post[f]      = sum_c start_post[f][c], c in index order (1 at frame 0, up to rounding)
//   P(a span of c covers exactly [s, e)) = exp(F_h[s][c] + len[e-s][c] + B_h[T-e][c] + F_cum[T][c] - logZ)
// the last one being the summand of d logZ / d len[e-s][c] (smm_logz_bwd.hip).  Without EOS the closing label of frame T
// counts as a one-frame span of its class: its entry in all four outputs is P(closing label = to) =
// exp(smm_post_final_weight(to) - logZ).
//
// Nothing here is a recursion: both kernels gather.
//   smm_segpost_dense_kernel  grid (video, slab of SMM_POST_SLAB positions), thread = node (f, c), c fastest
//                             (smm_entropy_kernel's split): six history loads, two fp64 exp and two stores per node.  The
//                             slab's start posteriors also go through LDS, from where one thread per position sums them in
//                             index order into bnd_post.  Bounded by the history loads: 48 bytes in, 16 bytes out per node.
//   smm_segpost_spans_kernel  one thread per position of every given span row.  A span start finds its end by a forward scan
//                             over at most kp - 1 positions (a longer span has probability 0), then makes three history loads
//                             and one table load.  The class map is inverted by a search over the video's <= 32 states.
//                             Bounded by the scan: every position of a row is read twice.
// No atomics but the error word; no sum crosses a workgroup: two calls give the same bits.
//
// A video whose log Z is not finite gets NaN in every entry that would hold a probability and sets the error word; so does a
// NaN that reached the histories, in the entries it reaches.  The histories and the scratch rows are only read.
#include "smm_posterior.h"
#include "../../include/smmdp.h"

#define SMM_SEGPOST_THREADS 256

__device__ __forceinline__ bool smm_segpost_finite(double lz) { return lz > SMM_NEG_INF && lz < -SMM_NEG_INF; }

// exp of a log-probability: 0 for -inf, NaN for NaN
__device__ __forceinline__ double smm_segpost_p(double lp) { return lp == SMM_NEG_INF ? 0.0 : exp(lp); }

__global__ void __launch_bounds__(SMM_SEGPOST_THREADS) smm_segpost_dense_kernel(SmmSegPostArgs a)
{
    __shared__ double s_start[SMM_POST_SLAB][SMM_MAX_STATES_DEV + 1];
    const int vid = blockIdx.x, y = blockIdx.y;
    const SmmVideo mv = a.h.videos[vid];
    const int Tf = mv.T, T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max;
    const int C = a.h.n_states[g];
    const int n0 = y * SMM_POST_SLAB;
    if (n0 >= Tf) return;                               // frames 0 .. Tf - 1
    const int tid = threadIdx.x;
    if (T <= 0 || C <= 0) {
        if (tid == 0) atomicExch(a.h.err, 1);
        return;
    }
    const int n1 = (n0 + SMM_POST_SLAB < Tf) ? n0 + SMM_POST_SLAB : Tf;
    const SmmHist H = smm_hist(a.p.hist, mv, cm, T);
    const double lz = a.p.logz[vid];
    const bool ok = smm_segpost_finite(lz);
    const size_t row0 = (size_t)(mv.frame_off + n0);
    bool bad = !ok;
    const int nodes = (n1 - n0) * cm;
    for (int i = tid; i < nodes; i += SMM_SEGPOST_THREADS) {
        const int dn = i / cm, c = i - dn * cm, f = n0 + dn;
        if (c >= C) continue;                           // (padded columns keep the 0.0 of the fill)
        double ps, pe;
        if (!ok) {
            ps = pe = __builtin_nan("");
        } else if (f < T) {
            ps = smm_segpost_p(smm_post_lp_start(H, T, cm, f, c, lz));
            pe = smm_segpost_p(smm_post_lp_end(H, T, cm, f + 1, c, lz));
        } else {                                        // no EOS: the closing label of frame T
            ps = pe = smm_segpost_p(smm_post_final_weight(a.h, a.p, mv, vid, T, C, H.F.g + (size_t)T * cm, c) - lz);
        }
        bad |= (ps != ps) | (pe != pe);
        s_start[dn][c] = ps;
        const size_t o = (row0 + dn) * cm + c;
        if (a.start_post) a.start_post[o] = ps;
        if (a.end_post) a.end_post[o] = pe;
    }
    if (__any(bad) && (tid & 63) == 0) atomicExch(a.h.err, 1);
    if (!a.bnd_post) return;
    __syncthreads();
    if (tid < n1 - n0) {
        double s = 0.0;
        for (int c = 0; c < C; ++c) s += s_start[tid][c];
        a.bnd_post[row0 + tid] = s;
    }
}

// local state of a global class id: the video's class-map row searched in index order; -1 when the id is not in the set
__device__ __forceinline__ int smm_segpost_local(const int64_t *cmap, int C, int64_t id)
{
    if (!cmap) return (id >= 0 && id < C) ? (int)id : -1;
    for (int c = 0; c < C; ++c)
        if (cmap[c] == id) return c;
    return -1;
}

__global__ void __launch_bounds__(SMM_SEGPOST_THREADS) smm_segpost_spans_kernel(SmmSegPostArgs a)
{
    const int q = blockIdx.y * SMM_SEGPOST_THREADS + threadIdx.x;
    if (q > a.t_max) return;
    const int set = blockIdx.x / a.h.b, vid = blockIdx.x - set * a.h.b;
    const SmmVideo mv = a.h.videos[vid];
    const int T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max;
    const int C = a.h.n_states[g];
    const size_t row = ((size_t)set * a.h.b + vid) * (size_t)(a.t_max + 1);
    const int64_t *sp = a.spans_in + row;
    double out = SMM_NEG_INF;
    if (T > 0 && C > 0 && q <= T) {
        const double lz = a.p.logz[vid];
        const int64_t *cmap = a.class_map ? a.class_map + (size_t)g * (cm + 1) : nullptr;
        if (q == T) {
            if (!a.h.no_eos) {
                out = 0.0;                              // the EOS position
            } else {                                    // the closing label
                const int c = smm_segpost_local(cmap, C, sp[T]);
                const SmmHist H = smm_hist(a.p.hist, mv, cm, T);
                if (!smm_segpost_finite(lz)) out = __builtin_nan("");
                else if (c >= 0) out = smm_post_final_weight(a.h, a.p, mv, vid, T, C, H.F.g + (size_t)T * cm, c) - lz;
            }
        } else if (sp[q] != -1) {
            // a span start: its end is the next position that is no continuation, at most kp - 1 positions on
            const int kmax = (mv.kp - 1 < T - q) ? mv.kp - 1 : T - q;
            int k = 0;
            for (int j = 1; j <= kmax; ++j)
                if (sp[q + j] != -1) { k = j; break; }
            const int c = smm_segpost_local(cmap, C, sp[q]);
            if (!smm_segpost_finite(lz)) out = __builtin_nan("");
            else if (k > 0 && c >= 0) {
                const SmmHist H = smm_hist(a.p.hist, mv, cm, T);
                const double *len = a.p.len + (size_t)g * a.h.k_rows * cm;
                out = H.F.h[(size_t)q * cm + c] + len[(size_t)k * cm + c] + H.B.h[(size_t)(T - q - k) * cm + c]
                      + H.F.cum[(size_t)T * cm + c] - lz;
            }
        }
    }
    if (out != out) atomicExch(a.h.err, 1);
    a.seg_logp[row + q] = out;
}

void smm_launch_segpost(const SmmSegPostArgs &a, hipStream_t stream)
{
    if (a.start_post || a.end_post || a.bnd_post)
        hipLaunchKernelGGL(smm_segpost_dense_kernel, dim3(a.h.b, a.t_max / SMM_POST_SLAB + 1), dim3(SMM_SEGPOST_THREADS), 0,
                           stream, a);
    if (a.seg_logp)
        hipLaunchKernelGGL(smm_segpost_spans_kernel, dim3((unsigned)a.h.b * (unsigned)a.n_sets, a.t_max / SMM_SEGPOST_THREADS + 1),
                           dim3(SMM_SEGPOST_THREADS), 0, stream, a);
}
