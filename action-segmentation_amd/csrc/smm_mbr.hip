// smm_mbr.hip -- minimum-Bayes-risk decode under frame (Hamming) loss: the feasible segmentation with the most expected
// correct frames, sum_t gain[t][y_t] with gain = the frame posteriors (include/smmdp.h: smm_mbr_f64).
//
// The DP is smm_oracle_viterbi_ex's (oracle/smm_oracle.c) on substituted inputs: elp' = gain, len' = 0, and the tables binary,
// M(x) = SMM_BIG_NEG where x <= SMM_BIG_NEG / 2, else 0.  With zero length scores the length dimension collapses:
//   gam[n][c] = cum[n][c] + max_{k=1..kmax} h[n-k][c]          a sliding-window max over the last kp - 1 values of h
//   h[n][to]  = max_j (gam[n][j] + trans'[to][j]) - cum[n][to]
// Every floating-point operation is the twin's (serial fp64 prefix sums, the same adds and subtractions in the same
// association; max is exact), so spans, labels and best are bit-identical to the twin and to smm_viterbi_f64 on the
// substituted inputs.
//
// smm_mbr_kernel: one wave per video, several videos per workgroup, no barrier.  Lane L owns state c = L & 31 (both halves of
// the wave carry the same state values; the lower half stores them).  Per position:
//   - the gain row comes from LDS (chunks of SMM_MBR_ROWS rows, staged through registers one chunk ahead);
//   - the window max is van Herk / Gil-Werman over blocks of w = kp - 1 positions: a running prefix max of h since the start of
//     the block that holds position n - 1, and the suffix max S[lo] of the block before it, which a backward scan over that
//     block's h rows wrote to the workspace when the block was complete.  S[lo] is first needed two positions after that, so
//     its load is issued one position ahead, in front of the position's stores (what that costs);
//   - the transition goes through LDS: gam is written once, and each lane takes the max over its half of the source states
//     (lane to: sources [half * H, half * H + H), H = ceil(C / 2)), then over the two halves;
//   - h, the transition value bt = h + cum before the subtraction, and cum are stored per position for the back-trace.
// The back-trace is the twin's rule -- at (n, to) the first (k ascending, then source ascending) whose (cum[n][j] + h[n-k][j]) +
// w(to, j) equals m = max_j (gam[n][j] + w(to, j)) -- as one stream over the rows p = n - k, which only ever go down: the lower
// half of the wave tests row p, the upper half row p - 1, against the current (n, to); a hit starts a segment and the next state's
// m is bt[p][j] (the forward's own max), its cum the row's.  Rows are loaded a batch ahead.  Then the frame labels go back to
// the workspace and one lane sums gain[t][label_t] in frame order (the expected number of correct frames).
#include "smm_device.h"
#include "smm_launch.h"
#include "../../include/smmdp.h"

#define SMM_MBR_WAVES 4                                         // videos per workgroup
#define SMM_MBR_ROWS 32                                         // gain rows per LDS chunk
#define SMM_MBR_STAGE (SMM_MBR_ROWS * SMM_MAX_STATES_DEV / 64)  // doubles per lane of a chunk staged in registers
#define SMM_MBR_SCAN 16                                         // h rows per load batch of the suffix-max scan
#define SMM_MBR_BT 8                                            // row pairs per load batch of the back-trace

// fmax: the operands are finite or -inf (a NaN in the gain is caught by its bits at the end of the forward pass); the results
// of arithmetic need no canonicalising, so this is a bare v_max_f64 in the loops
__device__ __forceinline__ double mbr_max(double a, double b) { return __builtin_fmax(a, b); }

// the binary table entry of the substituted inputs: SMM_BIG_NEG for a forbidden term (-inf included), else 0
__device__ __forceinline__ double mbr_mask(double x) { return x <= SMM_BIG_NEG / 2 ? SMM_BIG_NEG : 0.0; }

// (not smm_device.h's smm_group_max<64>: that one's fmax() is not mbr_max)
__device__ __forceinline__ double mbr_wave_max(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = mbr_max(x, __shfl_xor(x, off));
    return x;
}

__device__ __forceinline__ int64_t mbr_gid(int64_t gid_l, int c)
{
    const int lo = __builtin_amdgcn_readlane((int)(gid_l & 0xffffffff), c);
    const int hi = __builtin_amdgcn_readlane((int)(gid_l >> 32), c);
    return ((int64_t)hi << 32) | (uint32_t)lo;
}

__global__ void __launch_bounds__(64 * SMM_MBR_WAVES) smm_mbr_kernel(SmmMbrArgs a)
{
    __shared__ double s_gain[SMM_MBR_WAVES][SMM_MBR_ROWS * SMM_MAX_STATES_DEV];
    __shared__ double s_gam[SMM_MBR_WAVES][SMM_MAX_STATES_DEV];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int slot = blockIdx.x * SMM_MBR_WAVES + wv;
    if (slot >= a.b) return;
    const int vid = __builtin_amdgcn_readfirstlane(a.order[slot]);
    const SmmVideo mv = a.videos[vid];
    const int Tf = mv.T, T = mv.T - a.no_eos, g = mv.group, cm = a.c_max, kp = mv.kp;
    const int C = a.n_states[g];
    const int H = (C + 1) >> 1;
    const int wl = kp > 2 ? kp - 1 : 1;                      // window block length (kp <= 1: no usable length at all)
    const bool no_len = kp < 2;
    const int to = lane & 31, half = lane >> 5;
    const bool live = to < C;                                 // the lane's state exists
    const bool own = live && half == 0;                       // ... and this lane stores its rows
    const double *gain = a.gain + (size_t)mv.frame_off * cm;
    const double *trans = a.trans + (size_t)g * cm * cm;
    const int64_t *cmap = a.class_map ? a.class_map + (size_t)g * (cm + 1) : nullptr;
    const size_t N = (size_t)(Tf + 1) * cm;
    double *hcum = a.hist + mv.hist_off, *hh = hcum + N, *hbt = hh + N, *hs = hbt + N;
    int32_t *hlab = reinterpret_cast<int32_t *>(hs + N);
    double *sg = s_gain[wv], *sgam = s_gam[wv];

    // lane (half, to): trans'[to][j] of the sources of its half
    double tp[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = half * H + i;
        tp[i] = (i < H && j < C && live) ? mbr_mask(trans[(size_t)to * cm + j]) : SMM_NEG_INF;
    }
    // lane j: which targets may follow source j at no cost (bit t: trans'[t][j] == 0), its end weight, its global id
    uint32_t tcol = 0;
    if (live)
        for (int t = 0; t < C; ++t) tcol |= (mbr_mask(trans[(size_t)t * cm + to]) == 0.0 ? 1u : 0u) << t;
    const double epj = (live && a.endpen) ? mbr_mask(a.endpen[(size_t)vid * cm + to]) : 0.0;
    const int64_t gid_l = (lane <= C) ? (cmap ? cmap[lane] : (int64_t)lane) : 0;

    // gain chunks: registers one chunk ahead of the LDS copy the positions read
    double stg[SMM_MBR_STAGE];
    auto load_chunk = [&](int c) {
        const int rows = Tf - c * SMM_MBR_ROWS;
        const int ne = rows <= 0 ? 0 : (rows < SMM_MBR_ROWS ? rows : SMM_MBR_ROWS) * cm;
        const double *src = gain + (size_t)c * SMM_MBR_ROWS * cm;
#pragma unroll
        for (int q = 0; q < SMM_MBR_STAGE; ++q) {
            const int e = lane + 64 * q;
            stg[q] = e < ne ? src[e] : 0.0;
        }
    };
    auto put_chunk = [&]() {
#pragma unroll
        for (int q = 0; q < SMM_MBR_STAGE; ++q) sg[lane + 64 * q] = stg[q];
    };

    double h_prev = live ? mbr_mask(a.init[(size_t)g * cm + to]) : SMM_NEG_INF;     // h[0] = init'
    if (own) {
        hh[to] = h_prev;
        hcum[to] = 0.0;
    }
    load_chunk(0);
    put_chunk();
    load_chunk(1);
    int chunk = 1, row = 0;
    double cum = 0.0, P = SMM_NEG_INF, s_next = SMM_NEG_INF, gam = SMM_NEG_INF;
    int r = wl - 1, bn = -1;                                  // position n - 1 = bn * wl + r
    for (int n = 1; n <= T; ++n) {
        if (++r == wl) { r = 0; ++bn; }
        const double s_cur = s_next;
        {
            // the suffix max the next position needs: S[n + 1 - wl] of the block before that of position n
            const int r2 = (r + 1 == wl) ? 0 : r + 1, b2 = (r + 1 == wl) ? bn + 1 : bn;
            s_next = SMM_NEG_INF;
            if (n < T && b2 >= 1 && r2 < wl - 1 && live) s_next = hs[(size_t)(n + 1 - wl) * cm + to];
        }
        const double gv = sg[(size_t)row * cm + to];
        cum = cum + gv;
        const double hin = no_len ? SMM_NEG_INF : h_prev;
        P = (r == 0) ? hin : mbr_max(P, hin);
        gam = cum + mbr_max(P, s_cur);
        gam = live ? gam : SMM_NEG_INF;
        if (n == T) break;
        if (half == 0) sgam[to] = gam;
        __builtin_amdgcn_wave_barrier();
        double bt = SMM_NEG_INF;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i >= H) break;
            bt = mbr_max(bt, sgam[half * H + i] + tp[i]);
        }
        bt = smm_max_halves(bt);
        const double h = bt - cum;
        if (own) {
            hh[(size_t)n * cm + to] = h;
            hbt[(size_t)n * cm + to] = bt;
            hcum[(size_t)n * cm + to] = cum;
        }
        h_prev = h;
        if (++row == SMM_MBR_ROWS) {
            row = 0;
            put_chunk();
            load_chunk(++chunk);
        }
        // position n completes its block: the block's suffix maxima (needed from position n + 2 on)
        if (wl >= 2 && r == wl - 2 && n + 2 <= T) {
            __threadfence_block();
            double m = SMM_NEG_INF;
            const int p_lo = n - wl;                          // (exclusive)
            for (int p = n; p > p_lo; p -= SMM_MBR_SCAN) {
                double v[SMM_MBR_SCAN];
#pragma unroll
                for (int q = 0; q < SMM_MBR_SCAN; ++q) v[q] = (p - q > p_lo && live) ? hh[(size_t)(p - q) * cm + to] : SMM_NEG_INF;
#pragma unroll
                for (int q = 0; q < SMM_MBR_SCAN; ++q) {
                    m = mbr_max(m, v[q]);
                    if (own && p - q > p_lo) hs[(size_t)(p - q) * cm + to] = m;
                }
            }
            __threadfence_block();
        }
    }
    // ---- closing step at position T: per real target (EOS mode: + SMM_BIG_NEG; no EOS: + the last frame's gain), and EOS
    if (half == 0) sgam[to] = gam;
    __builtin_amdgcn_wave_barrier();
    double fpre = SMM_NEG_INF;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (i >= H) break;
        fpre = mbr_max(fpre, sgam[half * H + i] + tp[i]);
    }
    fpre = smm_max_halves(fpre);
    bool bad = smm_nan_bits(cum);
    double fin = SMM_NEG_INF;
    if (live) {
        if (a.no_eos) {
            const double gl = gain[(size_t)T * cm + to];
            bad |= smm_nan_bits(gl);
            fin = fpre + gl;
        } else {
            fin = fpre + SMM_BIG_NEG;
        }
    }
    const double fe = a.no_eos ? SMM_NEG_INF : mbr_wave_max((live && half == 0) ? gam + epj : SMM_NEG_INF);
    double best = mbr_wave_max(fin);
    if (!a.no_eos) best = mbr_max(best, fe);
    const unsigned long long hitf = __ballot(own && fin == best);
    const int best_to = hitf ? __ffsll(hitf) - 1 : C;
    bad = __ballot(live && bad) != 0;

    int64_t *spans = a.spans ? a.spans + (size_t)vid * (a.t_max + 1) : nullptr;
    int64_t *labels = a.labels ? a.labels + mv.frame_off : nullptr;
    // every span position is written by lane (position & 63): the -1 filler and the entries that follow are one thread's stores
    if (spans)
        for (int q = lane; q <= a.t_max; q += 64) spans[q] = -1;
    int nseg = 0;
    bool fail = bad;
    if (!bad) {
        const int64_t gl_to = mbr_gid(gid_l, best_to);
        if (spans && lane == (T & 63)) spans[T] = gl_to;
        if (a.no_eos && lane == 0) {
            if (labels) labels[T] = gl_to;
            hlab[T] = best_to;
        }
        // ---- back-trace
        __threadfence_block();
        int n = T;
        double m = (best_to == C) ? fe : smm_readlane(fpre, best_to);
        double cumn = cum;
        double wj = (best_to == C) ? epj : (((tcol >> best_to) & 1u) ? 0.0 : SMM_BIG_NEG);
        double bh[SMM_MBR_BT], bc[SMM_MBR_BT], bb[SMM_MBR_BT];
        double nh[SMM_MBR_BT], nc[SMM_MBR_BT], nb[SMM_MBR_BT];
        auto load_rows = [&](int p, double (&vh)[SMM_MBR_BT], double (&vc)[SMM_MBR_BT], double (&vb)[SMM_MBR_BT]) {
#pragma unroll
            for (int q = 0; q < SMM_MBR_BT; ++q) {
                const int rw = p - 2 * q - half;
                const bool ok = rw >= 0 && live;
                const size_t o = (size_t)(ok ? rw : 0) * cm + to;
                vh[q] = ok ? hh[o] : SMM_NEG_INF;
                vc[q] = ok ? hcum[o] : 0.0;
                vb[q] = ok ? hbt[o] : SMM_NEG_INF;
            }
        };
        int p = T - 1;
        load_rows(p, bh, bc, bb);
        while (n > 0) {
            load_rows(p - 2 * SMM_MBR_BT, nh, nc, nb);
#pragma unroll
            for (int q = 0; q < SMM_MBR_BT; ++q) {
                const int rw = p - 2 * q - half;
                while (n > 0) {
                    const int kmax = (kp - 1 < n) ? kp - 1 : n;
                    const bool cand = live && rw >= 0 && rw < n && n - rw <= kmax;
                    const double val = (cumn + bh[q]) + wj;
                    const unsigned long long hit = __ballot(cand && val == m);
                    if (!hit) break;
                    const int src = __ffsll(hit) - 1;        // the lower half's row (the shorter segment) first
                    const int jn = src & 31, s = p - 2 * q - (src >> 5);
                    const int64_t gv = mbr_gid(gid_l, jn);
                    for (int f = s + lane; f < n; f += 64) {
                        if (labels) labels[f] = gv;
                        hlab[f] = jn;
                    }
                    if (spans && lane == (s & 63)) spans[s] = gv;
                    ++nseg;
                    m = smm_readlane(bb[q], src);
                    const double oc = __shfl_xor(bc[q], 32);
                    cumn = ((src >> 5) == half) ? bc[q] : oc;
                    wj = ((tcol >> jn) & 1u) ? 0.0 : SMM_BIG_NEG;
                    n = s;
                }
            }
            p -= 2 * SMM_MBR_BT;
            // no row left within the span limit of (n, cur): a NaN / inf - inf reached the DP after all
            if (n > 0 && p < n - ((kp - 1 < n) ? kp - 1 : n)) { fail = true; break; }
#pragma unroll
            for (int q = 0; q < SMM_MBR_BT; ++q) { bh[q] = nh[q]; bc[q] = nc[q]; bb[q] = nb[q]; }
        }
    }
    double gsum = __builtin_nan("");
    if (!fail) {
        // ---- the expected number of correct frames: sum_t gain[t][label_t], serially in frame order
        __threadfence_block();
        double acc = 0.0;
        for (int t0 = 0; t0 < Tf; t0 += 64) {
            const int t = t0 + lane;
            double v = 0.0;
            if (t < Tf) v = gain[(size_t)t * cm + hlab[t]];
            const int cnt = (Tf - t0 < 64) ? Tf - t0 : 64;
            for (int i = 0; i < cnt; ++i) acc = acc + smm_readlane(v, i);
        }
        gsum = acc;
    }
    if (lane == 0) {
        if (fail) atomicExch(a.err, 1);
        if (a.best) a.best[vid] = fail ? __builtin_nan("") : best;
        if (a.gain_sum) a.gain_sum[vid] = gsum;
        if (a.n_segs) a.n_segs[vid] = fail ? 0 : nseg + a.no_eos;
    }
}

void smm_launch_mbr(const SmmMbrArgs &a, hipStream_t stream)
{
    const int blocks = (a.b + SMM_MBR_WAVES - 1) / SMM_MBR_WAVES;
    hipLaunchKernelGGL(smm_mbr_kernel, dim3((unsigned)blocks), dim3(64 * SMM_MBR_WAVES), 0, stream, a);
}
