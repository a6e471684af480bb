// smm_align_graph_sample.hip -- alignments drawn from the transcript-graph posterior p(alignment | x, "the class sequence is a
// start -> end path of this graph") (include/smmdp.h: smm_align_graph_sample_f64): forward filtering by
// smm_align_graph_logz_fwd_kernel, backward sampling here.  What smm_sample.hip is to smm_logz_kernel.
//
// Inputs are what the forward kernel leaves in the video's block of the workspace (smm_align_graph_logz.hip has the layout and the
// recursions): the h columns, h[s][m] = log-weight of "a segment of node m starts at s" - cum[s][a_m]; the gam columns,
// gam[n][m] = log-weight of "a segment of node m ends at n"; and five ints per column, lo, hi, slo, shi, z: gam[.][m] holds
// values on [lo, hi] only, h[.][m] on [slo, shi] and, when z, at 0.  Everything else in the block is uninitialised memory: a
// candidate is tested against these ranges BEFORE its value is loaded, and one outside them has no mass.
// One walk per (video, sample), from n = T:
//   end node     j ~ exp(gam[T][j] + closing_j) over the nodes with end(j)
//   span         a segment of node j that ends at n starts at n - k,  k ~ exp(h[n-k][j] + len[k][a_j]),  k = 1 .. min(kw, n)
//                (cum[n][a_j] is the same for every k)
//   predecessor  at s = n - k > 0,  i ~ exp(gam[s][i] + trans[a_j][a_i]) over i in pred(j)
//   stop         at s = 0: h[0][j] exists for a start node only
// The histories carry the forward kernel's rounding: they decide the draws, never the log-probability, which is summed in fp64
// from the tables and elp (init, the emissions of every segment, len, trans, the closing term) minus logZ_g.
//
// Work split: smm_sample.hip's.  One wave per (video, sample), grid-stride over the pairs; lane l takes candidates l, l + 64,
// ...: <= 16 per lane of the span draw (kw <= 1023), <= 4 per lane of the end and predecessor draws (M <= 256; the predecessor
// draw tests the candidate's bit of node j's mask).  Candidate number = k - 1, or the node index.  The draw and the random
// numbers are smm_draw.h's; counter = (decision number, sample, video, 1), and every decision takes one counter value.
// Every output position has one writing lane (position & 63), so the fillers and the values that replace them are one
// thread's stores in program order.  No LDS, no private segment, no atomics but the error word.
#define SMM_ALIGN_THREADS 256
#define SMM_ALIGN_R 3
#include "smm_align_tile.h"
#include "smm_align_graph.h"
#include "smm_draw.h"

#define SMM_AGS_NK 16              // span candidates per lane: 16 x 64 >= SMM_MAX_K_ROWS - 1
#define SMM_AGS_NM 4               // node candidates per lane: 4 x 64 = SMM_MAX_TRANSCRIPT
#define SMM_AGS_STREAM 1u          // the last counter word (smm_sample.hip: 0)

static_assert(SMM_AGS_NK * 64 >= SMM_MAX_K_ROWS - 1, "a lane holds its share of the span lengths");
static_assert(SMM_AGS_NM * 64 >= SMM_MAX_TRANSCRIPT, "a lane holds its share of the nodes");

__device__ void ags_sample_one(const SmmAlignSampleArgs &a, int vid, int smp, int lane)
{
    const AlignVideo v = align_video(a.g, vid);
    const int T = v.T, cm = v.cm, kw = v.kw, M = v.M;
    const size_t T1 = v.T1;
    const int b = a.g.b;
    int64_t *sp = a.spans ? a.spans + ((size_t)smp * b + vid) * (size_t)(a.t_max + 1) : nullptr;
    int64_t *lab = a.labels ? a.labels + (size_t)smp * a.total_frames + v.frame_off : nullptr;
    int32_t *us = a.used ? a.used + (size_t)smp * a.n_nodes + v.t0 : nullptr;
    if (sp)
        for (int q = lane; q <= a.t_max; q += 64) sp[q] = -1;
    if (us)
        for (int m = lane; m < M; m += 64) us[m] = 0;

    const double lz = a.g.logz[vid];
    bool ok = !align_nonfinite_bits(lz);       // (-inf: no alignment, an ordinary "impossible"; a finite logZ_g had a valid structure)
    const bool lz_nan = smm_nan_bits(lz);      // (staging cleared the word the forward call had set)
    double lp = 0.0;                           // (wave-uniform)
    int segs = 0;
    if (ok) {
        const int *rng = graph_rng(a.g.cols + a.g.hoff[vid]);
        const GraphCols<const double> col = graph_cols<const double>(a.g.cols + a.g.hoff[vid], M, T1);
        const double *hcol = col.h, *gcol = col.g;
        const int32_t *cls = a.g.transcript + v.t0;
        const uint8_t *fl = a.g.node_flags + v.t0;
        const uint32_t *mask = a.g.pred_mask + (size_t)v.t0 * SMM_GRAPH_WORDS;
        const int64_t *cmap = a.class_map ? a.class_map + (size_t)v.g * (cm + 1) : nullptr;
        uint32_t dec = 0;
        int n = T;
        // ---- the end node
        double we[SMM_AGS_NM];
#pragma unroll
        for (int i = 0; i < SMM_AGS_NM; ++i) {
            const int m = i * 64 + lane;
            we[i] = SMM_NEG_INF;
            if (m < M && (fl[m] & 2)) {
                const GraphRange r = graph_range(rng, m);
                if (r.lo <= T && T <= r.hi) we[i] = gcol[(size_t)m * T1 + T] + graph_closing(v.endpen, cls[m]);
            }
        }
        int j = smm_draw<SMM_AGS_NM>(we, smm_uniform53(a.seed, vid, smp, dec++, SMM_AGS_STREAM), lane);
        if (j < 0 || j >= M) ok = false;
        else lp += graph_closing(v.endpen, cls[j]);
        while (ok) {
            // ---- the start of the segment of node j that ends at n
            const int c = cls[j];
            const GraphRange rj = graph_range(rng, j);
            const int slo = rj.slo, shi = rj.shi, z = rj.z;
            const double *hj = hcol + (size_t)j * T1;
            const int kmax = kw < n ? kw : n;
            double w[SMM_AGS_NK];
#pragma unroll
            for (int i = 0; i < SMM_AGS_NK; ++i) {
                const int k = 1 + i * 64 + lane, s = n - k;
                const bool in = k <= kmax && ((s >= slo && s <= shi) || (z != 0 && s == 0));
                w[i] = in ? hj[s] + v.len[(size_t)k * cm + c] : SMM_NEG_INF;
            }
            const int kc = smm_draw<SMM_AGS_NK>(w, smm_uniform53(a.seed, vid, smp, dec++, SMM_AGS_STREAM), lane);
            if (kc < 0 || kc + 1 > kmax) { ok = false; break; }
            const int k = kc + 1, s = n - k;
            const int64_t gid = smm_gid(cmap, c);
            double es = 0.0;
            for (int f = (s & ~63) + lane; f < n; f += 64)
                if (f >= s) {
                    es += v.elp[(size_t)f * cm + c];
                    if (lab) lab[f] = gid;
                }
            lp += v.len[(size_t)k * cm + c] + smm_group_sum<64>(es);
            if (sp && lane == (s & 63)) sp[s] = gid;
            if (us && lane == (j & 63)) us[j] = 1;
            ++segs;
            if (s == 0) {
                lp += v.init[c];
                break;
            }
            // ---- the node in front of it
            double wp[SMM_AGS_NM];
#pragma unroll
            for (int i = 0; i < SMM_AGS_NM; ++i) {
                const int m = i * 64 + lane;
                wp[i] = SMM_NEG_INF;
                if (m < j && ((mask[(size_t)j * SMM_GRAPH_WORDS + (m >> 5)] >> (m & 31)) & 1u)) {
                    const GraphRange r = graph_range(rng, m);
                    if (s >= r.lo && s <= r.hi) wp[i] = gcol[(size_t)m * T1 + s] + v.trans[(size_t)c * cm + cls[m]];
                }
            }
            const int jp = smm_draw<SMM_AGS_NM>(wp, smm_uniform53(a.seed, vid, smp, dec++, SMM_AGS_STREAM), lane);
            if (jp < 0 || jp >= j) { ok = false; break; }
            lp += v.trans[(size_t)c * cm + cls[jp]];
            j = jp;
            n = s;
        }
        if (ok) {
            if (sp && lane == (T & 63)) sp[T] = smm_gid(cmap, v.C);
        } else {                               // a decision without a candidate of finite weight: take back what the walk wrote
            if (sp)
                for (int q = lane; q <= a.t_max; q += 64) sp[q] = -1;
            if (us)
                for (int m = lane; m < M; m += 64) us[m] = 0;
        }
    }
    if (!ok && lab)
        for (int f = lane; f < T; f += 64) lab[f] = -1;
    if ((lz_nan || (!ok && !align_nonfinite_bits(lz))) && lane == 0) atomicExch(a.g.err, 1);
    if (lane == 0) {
        if (a.logp) a.logp[(size_t)smp * b + vid] = ok ? lp - lz : __builtin_nan("");
        if (a.n_segs) a.n_segs[(size_t)smp * b + vid] = ok ? segs : 0;
    }
}

__global__ void __launch_bounds__(256) smm_align_graph_sample_kernel(SmmAlignSampleArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_pairs = (int64_t)a.g.b * a.n_samples;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < n_pairs; p += stride) {
        const int vid = __builtin_amdgcn_readfirstlane((int)(p / a.n_samples));
        const int smp = __builtin_amdgcn_readfirstlane((int)(p % a.n_samples));
        ags_sample_one(a, vid, smp, lane);
    }
}

void smm_launch_align_graph_sample(const SmmAlignSampleArgs &a, hipStream_t stream)
{
    const int64_t waves = (int64_t)a.g.b * a.n_samples;
    const int64_t blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(smm_align_graph_sample_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, stream, a);
}
