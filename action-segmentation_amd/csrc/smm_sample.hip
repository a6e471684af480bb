// smm_sample.hip -- segmentations drawn from the semi-Markov posterior p(y | x) (forward filtering, backward sampling).
//
// Inputs are the forward histories smm_logz_kernel leaves in the workspace (smm_logz_bwd.hip has the layout):
//   F_cum[n][c] = cumE,   F_h[s][c] = start[s][c] - cumE[s][c]  (start: log-weight of "a span of c starts at s", init at 0),
//   F_g[n][c]   = gamma   (log-weight of "a span of c ends at n").
// One walk per (video, sample), from the end (oracle/smm_oracle.c: smm_oracle_logz has the plain statement of the weights):
//   last label   EOS:    j ~ exp(gamma[T][j] + wend[j]),  wend[j] = LSE(endpen[j], LSE_to(trans[to][j]) - 1e9)  (smm_post_wend)
//                no EOS: to ~ exp(LSE_c(gamma[T][c] + trans[to][c]) + elp[T][to]), then its predecessor as below
//   span start   a span of j that ends at n starts at n - k,  k ~ exp(F_h[n-k][j] + len[k][j]),  k = 1 .. min(kp-1, n)
//                (cumE[n][j] is the same for every k)
//   predecessor  a span of j that starts at s > 0 follows a span of j',  j' ~ exp(gamma[s][j'] + trans[j][j'])
// The distribution sampled is the one whose normaliser smm_logz_f64 returns.  The histories carry the log Z kernel's fp32-internal
// rounding (~1e-6 relative): they decide the draws, never the log-probability, which is summed in fp64 from the tables and elp
// (init, emissions of every span, len, trans, the closing term) minus log Z.
//
// Work split: one wave per (video, sample), grid-stride over the pairs.  A decision has at most 1023 candidates: lane l takes
// candidates l, l + 64, ...  (<= 16 per lane); the draw itself and the random numbers are smm_draw.h's, shared with
// smm_align_graph_sample.hip.  Counter = (decision number, sample, video, 0).
#include "smm_posterior.h"
#include "smm_draw.h"
#include "../../include/smmdp.h"

#define SMM_SAMPLE_NI 16           // candidates per lane: 16 x 64 >= SMM_MAX_K_ROWS - 1

__device__ void smm_sample_one(const SmmSampleArgs &a, int vid, int smp, int lane)
{
    const SmmVideo mv = a.h.videos[vid];
    const int Tf = mv.T, T = mv.T - a.h.no_eos, g = mv.group, cm = a.h.c_max;
    const int C = a.h.n_states[g];
    const SmmHistDir F = smm_hist_dir(a.p.hist, mv, cm, T, 0);
    const double *F_h = F.h, *F_g = F.g;
    const double *trans = a.p.trans + (size_t)g * cm * cm;
    const double *len = a.p.len + (size_t)g * a.h.k_rows * cm;
    const double *elp = a.p.elp + (size_t)mv.frame_off * cm;
    const int64_t *cmap = a.class_map ? a.class_map + (size_t)g * (cm + 1) : nullptr;
    int64_t *sp = a.spans ? a.spans + ((size_t)smp * a.h.b + vid) * (size_t)(a.t_max + 1) : nullptr;
    int64_t *lab = a.labels ? a.labels + (size_t)smp * a.total_frames + mv.frame_off : nullptr;
    // every span position is written by lane (position & 63): the -1 filler and the labels that follow are one thread's stores
    if (sp)
        for (int q = lane; q <= a.t_max; q += 64) sp[q] = -1;
    if (T <= 0 || C <= 0) {
        if (lane == 0) atomicExch(a.h.err, 1);
        return;
    }
    uint32_t dec = 0;
    double lp = 0.0;               // (wave-uniform)
    bool ok = true;
    int j, n = T;
    if (!a.h.no_eos) {
        double w[1] = {SMM_NEG_INF}, wend = SMM_NEG_INF;
        if (lane < C) {
            wend = smm_post_wend(trans, a.p.endpen ? a.p.endpen + (size_t)vid * cm : nullptr, cm, C, lane);
            w[0] = F_g[(size_t)T * cm + lane] + wend;
        }
        j = smm_draw<1>(w, smm_uniform53(a.seed, vid, smp, dec++, 0u), lane);
        if (j < 0) ok = false;
        else {
            lp += smm_readlane(wend, j);
            if (sp && lane == (Tf & 63)) sp[Tf] = smm_gid(cmap, C);
        }
    } else {
        // the closing label of frame T (it only emits), then the label of the span that ends at T
        double w[1] = {SMM_NEG_INF};
        if (lane < C) {
            double f = SMM_NEG_INF;
            for (int c = 0; c < C; ++c) f = smm_lse2_exact(f, F_g[(size_t)T * cm + c] + trans[(size_t)lane * cm + c]);
            w[0] = f + elp[(size_t)T * cm + lane];
        }
        const int to = smm_draw<1>(w, smm_uniform53(a.seed, vid, smp, dec++, 0u), lane);
        j = -1;
        if (to < 0) ok = false;
        else {
            lp += elp[(size_t)T * cm + to];
            const int64_t gid = smm_gid(cmap, to);
            if (sp && lane == (T & 63)) sp[T] = gid;
            if (lab && lane == 0) lab[T] = gid;
            double w1[1] = {lane < C ? F_g[(size_t)T * cm + lane] + trans[(size_t)to * cm + lane] : SMM_NEG_INF};
            j = smm_draw<1>(w1, smm_uniform53(a.seed, vid, smp, dec++, 0u), lane);
            if (j < 0) ok = false;
            else lp += trans[(size_t)to * cm + j];
        }
    }
    while (ok && n > 0) {
        // start of the span of j that ends at n
        const int kmax = (mv.kp - 1 < n) ? mv.kp - 1 : n;
        double w[SMM_SAMPLE_NI];
#pragma unroll
        for (int i = 0; i < SMM_SAMPLE_NI; ++i) {
            const int k = 1 + i * 64 + lane;
            w[i] = (k <= kmax) ? F_h[(size_t)(n - k) * cm + j] + len[(size_t)k * cm + j] : SMM_NEG_INF;
        }
        const int kc = smm_draw<SMM_SAMPLE_NI>(w, smm_uniform53(a.seed, vid, smp, dec++, 0u), lane);
        if (kc < 0 || kc + 1 > kmax) { ok = false; break; }
        const int k = kc + 1, s = n - k;
        const int64_t gid = smm_gid(cmap, j);
        double es = 0.0;
        for (int f = s + lane; f < n; f += 64) {
            es += elp[(size_t)f * cm + j];
            if (lab) lab[f] = gid;
        }
        lp += len[(size_t)k * cm + j] + smm_group_sum<64>(es);
        if (sp && lane == (s & 63)) sp[s] = gid;
        if (s == 0) {
            lp += a.p.init[(size_t)g * cm + j];
            break;
        }
        // the span in front of it
        double w1[1] = {lane < C ? F_g[(size_t)s * cm + lane] + trans[(size_t)j * cm + lane] : SMM_NEG_INF};
        const int jp = smm_draw<1>(w1, smm_uniform53(a.seed, vid, smp, dec++, 0u), lane);
        if (jp < 0 || jp >= C) { ok = false; break; }
        lp += trans[(size_t)j * cm + jp];
        j = jp;
        n = s;
    }
    if (!ok && lane == 0) atomicExch(a.h.err, 1);
    if (a.logp && lane == 0) a.logp[(size_t)smp * a.h.b + vid] = ok ? lp - a.p.logz[vid] : __builtin_nan("");
}

__global__ void __launch_bounds__(256) smm_sample_kernel(SmmSampleArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_pairs = (int64_t)a.h.b * a.n_samples;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < n_pairs; p += stride) {
        const int vid = __builtin_amdgcn_readfirstlane((int)(p / a.n_samples));
        const int smp = __builtin_amdgcn_readfirstlane((int)(p % a.n_samples));
        smm_sample_one(a, vid, smp, lane);
    }
}

void smm_launch_sample(const SmmSampleArgs &a, hipStream_t stream)
{
    const int64_t waves = (int64_t)a.h.b * a.n_samples;
    const int64_t blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(smm_sample_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, stream, a);
}
