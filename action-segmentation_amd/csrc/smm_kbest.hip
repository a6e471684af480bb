// smm_kbest.hip -- the k highest-scoring segmentations (k-best Viterbi: the DP in the k-max semiring).
//
// The lattice is smm_oracle_viterbi_ex's (oracle/smm_oracle.c), with every value of it turned into a sorted list of up to k
// entries, each with a back-pointer:
//   G[n][j][0..k)   top k over (l, r) of H[n-l][j][r] + len[l][j], plus cum[n][j]            back-pointer l * 16 + r
//   H[n][to][0..k)  top k over (j, r) of G[n][j][r] + trans[to][j], minus cum[n][to]         back-pointer j * 16 + r
//                   (H[0][to] = {init[to]})
//   closing         per to in {0..C-1, EOS}: top k over (j, r) of G[T][j][r] + w(to, j), then the per-to term (EOS mode: a real
//                   class + SMM_BIG_NEG; no EOS: + elp[T][to]); then top k over (to, r) of those lists.
// Each segmentation has one derivation, so the k best derivations are k distinct segmentations.  Every selection orders its
// candidates by (value descending, back-pointer ascending): a strict total order, so the top k are the first k of the top
// k' > k, and a launch is deterministic.
//
// smm_kbest_fwd_kernel: one workgroup per video, serial over positions, the classes dealt out to the waves (the wave that owns
// class j owns target j too, so the H lists a wave reads are the ones it wrote itself; the G lists go through LDS: one barrier
// per position).  The G step of (n, j) takes up to 1023 sorted lists: lane l owns the lengths l + 1, l + 65, ...; the top k of
// the lists' HEADS are found first (k wave arg-max rounds on registers), and only those lists can hold the top k entries (list i
// of them: its first k - i); their entries are read in one go and selected by k more rounds.  Two trips to memory per (n, j),
// none of them dependent on a selection round.
// smm_kbest_bt_kernel: one wave per (video, rank): follows the back-pointers to the front, then writes spans and labels and
// re-evaluates the score in fp64 from the tables and elp, segments left to right (init or trans, len, the emissions of the
// segment summed over the wave in a fixed order), then the closing term.
#include "smm_device.h"
#include "smm_launch.h"
#include "../../include/smmdp.h"

#define SMM_KB_WAVES 8          // waves per workgroup of the forward kernel
#define SMM_KB_EMPTY 0x7fffffff // key of "no candidate"

// (v, key) <- the better of itself and (ov, ok): larger value, then smaller key
__device__ __forceinline__ void kb_take(double &v, int &key, double ov, int ok)
{
    const bool t = ov > v || (ov == v && ok < key);
    v = t ? ov : v;
    key = t ? ok : key;
}

template <int CTRL>
__device__ __forceinline__ void kb_step(double &v, int &key)
{
    const double ov = smm_dpp<CTRL>(v);
    const int ok = __builtin_amdgcn_update_dpp(key, key, CTRL, 0xf, 0xf, false);
    kb_take(v, key, ov, ok);
}

// the best (v, key) of the wave, in every lane: within rows of 16 by DPP (xor 1, xor 2, half-row mirror, row mirror: each
// pairs a lane with one of the other half of the group it is made uniform over), then the four rows by readlane
__device__ __forceinline__ void kb_wave_best(double &v, int &key)
{
    kb_step<0xB1>(v, key);
    kb_step<0x4E>(v, key);
    kb_step<0x141>(v, key);
    kb_step<0x140>(v, key);
    double bv = smm_readlane(v, 0);
    int bk = __builtin_amdgcn_readlane(key, 0);
#pragma unroll
    for (int q = 1; q < 4; ++q) kb_take(bv, bk, smm_readlane(v, 16 * q), __builtin_amdgcn_readlane(key, 16 * q));
    v = bv;
    key = bk;
}

// a candidate value as selections see it: NaN flags the video and counts as no candidate, like -inf
__device__ __forceinline__ double kb_cand(double x, bool valid, bool &bad)
{
    if (!valid) return SMM_NEG_INF;
    bad |= (x != x);
    return (x > SMM_NEG_INF) ? x : SMM_NEG_INF;
}

// k rounds of selection over NI candidates per lane (value v[i], key keys(i)); lane r ends with the r-th best (-inf, EMPTY
// past the last).  Returns how many were found.
template <int NI, typename KeyF>
__device__ __forceinline__ int kb_select(double (&v)[NI], KeyF keys, int k, int lane, double &out_v, int &out_k)
{
    out_v = SMM_NEG_INF;
    out_k = SMM_KB_EMPTY;
    int found = 0;
    for (int r = 0; r < k; ++r) {
        double bv = SMM_NEG_INF;
        int bk = SMM_KB_EMPTY;
#pragma unroll
        for (int i = 0; i < NI; ++i) kb_take(bv, bk, v[i], v[i] > SMM_NEG_INF ? keys(i) : SMM_KB_EMPTY);
        kb_wave_best(bv, bk);
        if (!(bv > SMM_NEG_INF)) break;
        if (lane == r) { out_v = bv; out_k = bk; }
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (keys(i) == bk) v[i] = SMM_NEG_INF;
        ++found;
    }
    return found;
}

__global__ void __launch_bounds__(64 * SMM_KB_WAVES) smm_kbest_len_t_kernel(SmmKbestArgs a)
{
    // len[g][k_rows][c_max] -> len_t[g][c_max][k_rows] (the G step reads one class's lengths with consecutive lanes)
    const int64_t n = (int64_t)a.n_groups * a.c_max * a.k_rows;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = i % a.k_rows, gc = i / a.k_rows, c = gc % a.c_max, g = gc / a.c_max;
        a.len_t[i] = a.len[((size_t)g * a.k_rows + l) * a.c_max + c];
    }
}

__global__ void __launch_bounds__(64 * SMM_KB_WAVES) smm_kbest_fwd_kernel(SmmKbestArgs a)
{
    __shared__ double g_v[2][SMM_MAX_STATES_DEV][SMM_MAX_KBEST];          // G[n] lists, two positions in turn
    __shared__ double f_v[SMM_MAX_STATES_DEV + 1][SMM_MAX_KBEST];         // closing lists per target
    __shared__ int f_k[SMM_MAX_STATES_DEV + 1][SMM_MAX_KBEST];
    __shared__ double s_cum[SMM_MAX_STATES_DEV];
    __shared__ int s_bad;
    const int vid = blockIdx.x;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const SmmVideo mv = a.videos[vid];
    const int T = mv.T - a.no_eos, g = mv.group, cm = a.c_max, K = a.k, W = a.ring;
    const int C = a.n_states[g];
    const int64_t pos0 = mv.hist_off / (8 * (int64_t)cm);                // sum of (T_i + 1) over the videos in front
    const double *elp = a.elp + (size_t)mv.frame_off * cm;
    const double *trans = a.trans + (size_t)g * cm * cm;
    const double *len_t = a.len_t + (size_t)g * cm * a.k_rows;
    double *hh = a.hh + (size_t)vid * cm * W;                             // [c][W]       H[s][c][0]
    double *hr = a.hring + (size_t)vid * W * cm * K;                      // [W][c][k]    H[s][c][:]
    uint16_t *gbp = a.gbp + (size_t)pos0 * cm * K, *hbp = a.hbp + (size_t)pos0 * cm * K;
    if (threadIdx.x == 0) s_bad = 0;
    bool bad = false;
    // cum[n][j] of the wave's classes (each entry read and written by the wave that owns the class only)
    if (threadIdx.x < SMM_MAX_STATES_DEV) s_cum[threadIdx.x] = 0.0;
    __syncthreads();
    // position 0: H[0][to] = {init[to]}
    for (int to = w; to < C; to += SMM_KB_WAVES) {
        const double iv = a.init[(size_t)g * cm + to];
        if (lane < K) {
            hr[(size_t)to * K + lane] = lane == 0 ? iv : SMM_NEG_INF;
            hbp[(size_t)to * K + lane] = 0;
        }
        if (lane == 0) hh[(size_t)to * W] = iv;
    }
    __threadfence_block();
    int nm = 0;                                                           // n mod W
    for (int n = 1; n <= T; ++n) {
        nm = (nm + 1 == W) ? 0 : nm + 1;
        const int buf = n & 1;
        const int kmax = (mv.kp - 1 < n) ? mv.kp - 1 : n;
        // ---- G step of the wave's classes
        for (int j = w; j < C; j += SMM_KB_WAVES) {
            const double cj = s_cum[j] + elp[(size_t)(n - 1) * cm + j];
            // the heads of the lists l = lane + 1 + 64 i
            double hv[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int l = lane + 1 + 64 * i;
                double x = SMM_NEG_INF;
                if (l <= kmax) {
                    int sm = nm - l;
                    sm += sm < 0 ? W : 0;
                    x = hh[(size_t)j * W + sm] + len_t[(size_t)j * a.k_rows + l];
                }
                hv[i] = kb_cand(x, l <= kmax, bad);
            }
            double wl_v;
            int wl;                                   // lane i: the length whose head is the i-th best
            const int m = kb_select<16>(hv, [&](int i) { return lane + 1 + 64 * i; }, K, lane, wl_v, wl);
            double out_v = SMM_NEG_INF;
            int out_k = 0;
            if (K == 1) {
                out_v = wl_v;
                out_k = (lane == 0 && m > 0) ? wl * 16 : 0;
            } else if (m > 0) {
                // entries r < K - i of the list with the i-th best head: candidate q = i * 16 + r, lane q & 63, slot q >> 6
                double cv[4];
                int cl[4];
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int q = lane + 64 * s, i = q >> 4, r = q & 15;
                    const bool ok = i < m && r < K - i;
                    const int l = __shfl(wl, i & 63);
                    cl[s] = ok ? l : 0;
                    double x = SMM_NEG_INF;
                    if (ok) {
                        int sm = nm - l;
                        sm += sm < 0 ? W : 0;
                        x = hr[((size_t)sm * cm + j) * K + r] + len_t[(size_t)j * a.k_rows + l];
                    }
                    cv[s] = kb_cand(x, ok, bad);
                }
                kb_select<4>(cv, [&](int s) { return cl[s] * 16 + ((lane + 64 * s) & 15); }, K, lane, out_v, out_k);
            }
            if (lane == 0) s_cum[j] = cj;
            if (lane < K) {
                g_v[buf][j][lane] = out_v + cj;
                gbp[((size_t)n * cm + j) * K + lane] = (uint16_t)(out_v > SMM_NEG_INF ? out_k : 0);
            }
        }
        __syncthreads();
        if (n < T) {
            // ---- H step of the wave's targets
            for (int to = w; to < C; to += SMM_KB_WAVES) {
                double cv[8];
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int q = lane + 64 * s, jj = q >> 4, r = q & 15;
                    const bool ok = jj < C && r < K;
                    cv[s] = kb_cand(ok ? g_v[buf][jj][r] + trans[(size_t)to * cm + jj] : SMM_NEG_INF, ok, bad);
                }
                double out_v;
                int out_k;
                kb_select<8>(cv, [&](int s) { return lane + 64 * s; }, K, lane, out_v, out_k);
                const double h = out_v - s_cum[to];
                if (lane < K) {
                    hr[((size_t)nm * cm + to) * K + lane] = out_v > SMM_NEG_INF ? h : SMM_NEG_INF;
                    hbp[((size_t)n * cm + to) * K + lane] = (uint16_t)(out_v > SMM_NEG_INF ? out_k : 0);
                }
                if (lane == 0) hh[(size_t)to * W + nm] = out_v > SMM_NEG_INF ? h : SMM_NEG_INF;
            }
            // (the wave reads these lists itself at the next positions: its stores must be through first)
            __threadfence_block();
        }
    }
    // ---- closing step: per target (EOS = C in EOS mode), then over the targets
    const int buf = T & 1;
    const int n_to = a.no_eos ? C : C + 1;
    for (int to = w; to < n_to; to += SMM_KB_WAVES) {
        double cv[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int q = lane + 64 * s, jj = q >> 4, r = q & 15;
            const bool ok = jj < C && r < K;
            double x = SMM_NEG_INF;
            if (ok) {
                const double wt = (to == C) ? (a.endpen ? a.endpen[(size_t)vid * cm + jj] : 0.0) : trans[(size_t)to * cm + jj];
                x = g_v[buf][jj][r] + wt;
            }
            cv[s] = kb_cand(x, ok, bad);
        }
        double out_v;
        int out_k;
        kb_select<8>(cv, [&](int s) { return lane + 64 * s; }, K, lane, out_v, out_k);
        if (lane < K) {
            double f = out_v;
            if (out_v > SMM_NEG_INF) {
                if (a.no_eos) f = out_v + elp[(size_t)T * cm + to];
                else if (to < C) f = out_v + SMM_BIG_NEG;
            }
            f_v[to][lane] = kb_cand(f, true, bad);
            f_k[to][lane] = out_k;
        }
    }
    if (__ballot(bad)) {
        if (lane == 0) atomicOr(&s_bad, 1);
    }
    __syncthreads();
    if (w != 0) return;
    double cv[9];
#pragma unroll
    for (int s = 0; s < 9; ++s) {
        const int q = lane + 64 * s, to = q >> 4, r = q & 15;
        const bool ok = to < n_to && r < K;
        cv[s] = ok ? f_v[to][r] : SMM_NEG_INF;
    }
    double out_v;
    int out_k;
    kb_select<9>(cv, [&](int s) { return lane + 64 * s; }, K, lane, out_v, out_k);
    const bool nan_video = s_bad != 0;
    if (lane < K) {
        int key = 0;
        if (out_v > SMM_NEG_INF) key = ((out_k >> 4) << 9) | f_k[out_k >> 4][out_k & 15];   // to << 9 | j * 16 + r
        a.fin_v[(size_t)vid * K + lane] = nan_video ? __builtin_nan("") : out_v;
        a.fin_k[(size_t)vid * K + lane] = key;
    }
    if (nan_video && lane == 0) atomicExch(a.err, 1);
}

__device__ __forceinline__ int64_t kb_gid(const int64_t *cmap, int c) { return cmap ? cmap[c] : (int64_t)c; }

__device__ void smm_kbest_one(const SmmKbestArgs &a, int vid, int rank, int lane)
{
    const SmmVideo mv = a.videos[vid];
    const int Tf = mv.T, T = mv.T - a.no_eos, g = mv.group, cm = a.c_max, K = a.k;
    const int C = a.n_states[g];
    const int64_t pos0 = mv.hist_off / (8 * (int64_t)cm);
    const double *elp = a.elp + (size_t)mv.frame_off * cm;
    const double *trans = a.trans + (size_t)g * cm * cm;
    const double *len = a.len + (size_t)g * a.k_rows * cm;
    const uint16_t *gbp = a.gbp + (size_t)pos0 * cm * K, *hbp = a.hbp + (size_t)pos0 * cm * K;
    const int64_t *cmap = a.class_map ? a.class_map + (size_t)g * (cm + 1) : nullptr;
    int32_t *segs = a.segs + (size_t)rank * a.n_pos + pos0;
    int64_t *sp = a.spans ? a.spans + ((size_t)rank * a.b + vid) * (size_t)(a.t_max + 1) : nullptr;
    int64_t *lab = a.labels ? a.labels + (size_t)rank * a.total_frames + mv.frame_off : nullptr;
    const size_t out = (size_t)rank * a.b + vid;
    // every span position is written by lane (position & 63): the -1 filler and the entries that follow are one thread's stores
    if (sp)
        for (int q = lane; q <= a.t_max; q += 64) sp[q] = -1;
    const double fv = a.fin_v[(size_t)vid * K + rank];
    const int fk = a.fin_k[(size_t)vid * K + rank];
    bool ok = fv > SMM_NEG_INF;
    // back-pointers, from the end: segment c (from the back) = (length << 5) | class
    int cnt = 0;
    const int to = fk >> 9;
    if (ok) {
        int j = (fk >> 4) & 31, r = fk & 15, n = T;
        while (true) {
            if (j >= C || r >= K || cnt > T) { ok = false; break; }
            const int gb = gbp[((size_t)n * cm + j) * K + r];
            const int l = gb >> 4, s = n - l;
            if (l < 1 || s < 0) { ok = false; break; }
            if (lane == 0) segs[cnt] = (l << 5) | j;
            ++cnt;
            if (s == 0) break;
            const int hb = hbp[((size_t)s * cm + j) * K + (gb & 15)];
            j = hb >> 4;
            r = hb & 15;
            n = s;
        }
        if (!ok && lane == 0) atomicExch(a.err, 1);
    }
    if (!ok) {
        if (lab)
            for (int f = lane; f < Tf; f += 64) lab[f] = -1;
        if (lane == 0) {
            if (a.score) a.score[out] = (fv != fv || fv > SMM_NEG_INF) ? __builtin_nan("") : SMM_NEG_INF;
            if (a.n_segs) a.n_segs[out] = 0;
        }
        return;
    }
    __threadfence_block();
    // forward over the segments: spans, labels, the score in fp64
    double lp = 0.0;
    int s = 0, jprev = -1;
    for (int c = cnt - 1; c >= 0; --c) {
        const int e = segs[c], l = e >> 5, j = e & 31;
        lp = (jprev < 0) ? a.init[(size_t)g * cm + j] : lp + trans[(size_t)j * cm + jprev];
        lp += len[(size_t)l * cm + j];
        const int64_t gid = kb_gid(cmap, j);
        double es = 0.0;
        for (int f = s + lane; f < s + l; f += 64) {
            es += elp[(size_t)f * cm + j];
            if (lab) lab[f] = gid;
        }
        lp += smm_group_sum<64>(es);
        if (sp && lane == (s & 63)) sp[s] = gid;
        s += l;
        jprev = j;
    }
    if (a.no_eos) {
        lp += trans[(size_t)to * cm + jprev] + elp[(size_t)T * cm + to];
        const int64_t gid = kb_gid(cmap, to);
        if (sp && lane == (T & 63)) sp[T] = gid;
        if (lab && lane == 0) lab[T] = gid;
    } else {
        lp += (to == C) ? (a.endpen ? a.endpen[(size_t)vid * cm + jprev] : 0.0) : trans[(size_t)to * cm + jprev] + SMM_BIG_NEG;
        if (sp && lane == (T & 63)) sp[T] = kb_gid(cmap, to);
    }
    if (lane == 0) {
        if (a.score) a.score[out] = lp;
        if (a.n_segs) a.n_segs[out] = cnt;
    }
}

__global__ void __launch_bounds__(256) smm_kbest_bt_kernel(SmmKbestArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t n_pairs = (int64_t)a.b * a.k;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t p = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); p < n_pairs; p += stride) {
        const int vid = __builtin_amdgcn_readfirstlane((int)(p / a.k));
        const int rank = __builtin_amdgcn_readfirstlane((int)(p % a.k));
        smm_kbest_one(a, vid, rank, lane);
    }
}

void smm_launch_kbest(const SmmKbestArgs &a, hipStream_t stream)
{
    const int64_t nl = (int64_t)a.n_groups * a.c_max * a.k_rows;
    const int64_t lb = (nl + 511) / 512;
    hipLaunchKernelGGL(smm_kbest_len_t_kernel, dim3((unsigned)(lb < 1024 ? lb : 1024)), dim3(64 * SMM_KB_WAVES), 0, stream, a);
    hipLaunchKernelGGL(smm_kbest_fwd_kernel, dim3((unsigned)a.b), dim3(64 * SMM_KB_WAVES), 0, stream, a);
    const int64_t waves = (int64_t)a.b * a.k;
    const int64_t blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(smm_kbest_bt_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, stream, a);
}
