// smm_align_tile.h -- what the transcript kernels share (smm_align.hip: the best alignment; smm_align_opt.hip: the same with
// optional entries; smm_align_graph.hip: the same over the paths of a transcript graph, whose structure is in smm_align_graph.h;
// smm_align_logz.hip, smm_align_opt_logz.hip, smm_align_graph_logz.hip: the sums over all alignments): a video's header, its transcript
// in LDS, the tests on the bits and on the tables, the prefix-sum phase, the cells of a column that lie on a complete alignment,
// the tile walk of a column and the sweep of a thread's cells over the distances, the hulls of the per-class running values,
// the alignment's output phase, and the block scan and row store of the g_elp kernels.  What is log-semiring only is in
// smm_align_lse.h.  The including unit chooses its tile: SMM_ALIGN_THREADS threads, SMM_ALIGN_R positions per thread (odd: the
// threads' h reads are R doubles apart, which spreads a half-wave over all 64 banks).
#pragma once
#include "smm_device.h"
#include "smm_launch.h"
#include "../../include/smmdp.h"

#if !defined(SMM_ALIGN_THREADS) || !defined(SMM_ALIGN_R)
#error "define SMM_ALIGN_THREADS (threads per workgroup) and SMM_ALIGN_R (positions per thread) before this header"
#endif
#define SMM_ALIGN_P (SMM_ALIGN_THREADS * SMM_ALIGN_R)            // positions per tile
#define SMM_ALIGN_DMAX ((SMM_MAX_K_ROWS + SMM_ALIGN_R - 1) / SMM_ALIGN_R * SMM_ALIGN_R)   // distances walked, at most
#define SMM_ALIGN_OFF SMM_ALIGN_DMAX                             // LDS index of the tile's first position
#define SMM_ALIGN_HS (SMM_ALIGN_OFF + SMM_ALIGN_P + 8)           // h values in LDS: halo | tile | the R ahead
#define SMM_ALIGN_LEN (SMM_ALIGN_DMAX + 3 * SMM_ALIGN_R)         // length scores in LDS: index k + R, -inf outside 1 .. kp - 1

static_assert(SMM_ALIGN_R % 2 == 1, "an even stride puts a half-wave's h reads on a quarter of the banks");
static_assert(SMM_MAX_TRANSCRIPT <= SMM_ALIGN_THREADS, "one thread per transcript position checks its tables");

__device__ __forceinline__ double align_max(double a, double b) { return __builtin_fmax(a, b); }

// NaN or +-inf by the bits (exponent all ones)
__device__ __forceinline__ bool align_nonfinite_bits(double x)
{
    int hi = __double2hiint(x);
    asm volatile("" : "+v"(hi));
    return (hi & 0x7ff00000) == 0x7ff00000;
}
// NaN or +inf: what must not enter the DP (-inf is an ordinary "impossible")
__device__ __forceinline__ bool align_bad_bits(double x)
{
    return smm_nan_bits(x) || (align_nonfinite_bits(x) && __double2hiint(x) >= 0);
}

__device__ __forceinline__ double align_wave_max(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = align_max(x, __shfl_xor(x, off));
    return x;
}

__device__ __forceinline__ int align_wave_min(int x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int y = __shfl_xor(x, off);
        x = y < x ? y : x;
    }
    return x;
}

// the cells of column m that lie on a complete alignment (lo > hi: none)
__device__ __forceinline__ void align_range(int m, int M, int T, int kw, int &lo, int &hi)
{
    const int rest = M - 1 - m;
    const int a = m + 1, b = T - rest * kw;
    const int c = T - rest, d = (m + 1) * kw;
    lo = a > b ? a : b;
    hi = c < d ? c : d;
}

// ... and the positions at which segment m can start: {0} for m = 0, else the cells of column m - 1
__device__ __forceinline__ void align_start_range(int m, int M, int T, int kw, int &lo, int &hi)
{
    lo = hi = 0;
    if (m > 0) align_range(m - 1, M, T, kw, lo, hi);
}

// ... with optional entries (smm_align_opt.hip, smm_align_opt_logz.hip): nb / na: mandatory entries before / after m
__device__ __forceinline__ void align_opt_range(int m, int M, int T, int kw, int nb, int na, int &lo, int &hi)
{
    const int a = nb + 1, b = T - (M - 1 - m) * kw;
    const int c = T - na, d = (m + 1) * kw;
    lo = a > b ? a : b;
    hi = c < d ? c : d;
}

// Prefix sums of one video: tiles of `rows` frames through LDS (s_h: SMM_ALIGN_HS doubles), lane c adds class c serially,
// cum[c][n] class-major [C][T+1].  Every thread of the workgroup calls it; returns true in the threads whose class total is not
// finite.  The caller puts a barrier behind it before cum is read.
__device__ __forceinline__ bool align_prefix_sums(const double *elp, double *cum, int C, int cm, int T, double *s_h, int tid)
{
    const size_t T1 = (size_t)T + 1;
    const int ld = cm + 1;                                 // row stride in LDS: odd, so the transposing reads spread over the banks
    const int rows = SMM_ALIGN_HS / ld;
    double run = 0.0;
    if (tid < C) cum[(size_t)tid * T1] = 0.0;
    for (int f0 = 0; f0 < T; f0 += rows) {
        const int nr = T - f0 < rows ? T - f0 : rows;
        __syncthreads();
        for (int e = tid; e < nr * cm; e += SMM_ALIGN_THREADS) {
            const int r = e / cm, c = e - r * cm;
            s_h[r * ld + c] = elp[(size_t)f0 * cm + e];
        }
        __syncthreads();
        if (tid < C) {
#pragma unroll 8
            for (int r = 0; r < nr; ++r) {
                run = run + s_h[r * ld + tid];
                s_h[r * ld + tid] = run;
            }
        }
        __syncthreads();
        for (int e = tid; e < nr * C; e += SMM_ALIGN_THREADS) {
            const int c = e / nr, r = e - c * nr;
            cum[(size_t)c * T1 + f0 + 1 + r] = s_h[r * ld + c];
        }
    }
    return tid < C && align_nonfinite_bits(run);
}

// ---- a video and its transcript
struct AlignVideo {
    int T, g, cm, kw, C, M;                                // frames, group, row stride, span limit kp - 1, states, entries
    int64_t t0, frame_off;                                 // the transcript's and the frames' first index
    size_t T1;                                             // T + 1: the stride of cum's rows and of the columns
    const double *elp, *trans, *init, *len, *endpen;       // the video's frames, its group's tables, its closing row or null
    double *cum;                                           // [C][T+1] in the history area
};

template <class Args>
__device__ __forceinline__ AlignVideo align_video(const Args &a, int vid)
{
    const SmmVideo mv = a.videos[vid];
    AlignVideo v;
    v.T = mv.T; v.g = mv.group; v.cm = a.c_max; v.kw = mv.kp - 1;
    v.C = a.n_states[v.g];
    v.t0 = a.toff[vid];
    v.M = (int)(a.toff[vid + 1] - v.t0);
    v.frame_off = mv.frame_off;
    v.T1 = (size_t)v.T + 1;
    v.elp = a.elp + (size_t)mv.frame_off * v.cm;
    v.trans = a.trans + (size_t)v.g * v.cm * v.cm;
    v.init = a.init + (size_t)v.g * v.cm;
    v.len = a.len + (size_t)v.g * a.k_rows * v.cm;
    v.endpen = a.endpen ? a.endpen + (size_t)vid * v.cm : nullptr;
    v.cum = a.hist + mv.hist_off;
    return v;
}

// the transcript's ids -> s_a, and each(m, ok) per entry in the same pass; ok: the id is a state of the video (else its slot gets
// 0: never used as an index once the caller has raised its flag).  The caller puts a barrier behind it.
template <class Args, class Each>
__device__ __forceinline__ void align_load_ids(const Args &a, const AlignVideo &v, int *s_a, int tid, int nthreads, Each each)
{
    for (int m = tid; m < v.M; m += nthreads) {
        const int id = a.transcript[v.t0 + m];
        const bool ok = id >= 0 && id < v.C;
        s_a[m] = ok ? id : 0;
        each(m, ok);
    }
}

// ... with the flag (s_flag[0], cleared by the caller behind a barrier) and the barrier; false where an id is out of range
template <class Args>
__device__ __forceinline__ bool align_ids_ok(const Args &a, const AlignVideo &v, int *s_a, int *s_flag, int tid, int nthreads)
{
    align_load_ids(a, v, s_a, tid, nthreads, [&](int, bool ok) { if (!ok) s_flag[0] = 1; });
    __syncthreads();
    return s_flag[0] == 0;
}

// ... with optional entries: ids, flags, nb (mandatory entries before m; [M]: all of them) and plo (the first entry of
// pred(m); [M]: of the entries that may end) -> LDS; false where an id is out of range
template <class Args>
__device__ __forceinline__ bool align_load_opt(const Args &a, const AlignVideo &v, int *s_a, int *s_opt, int *s_nb, int *s_plo,
                                               int *s_flag, int tid, int nthreads)
{
    align_load_ids(a, v, s_a, tid, nthreads, [&](int m, bool ok) {
        s_opt[m] = a.optional[v.t0 + m] != 0;
        if (!ok) s_flag[0] = 1;
    });
    __syncthreads();
    if (tid == 0) {
        int nb = 0, head = 0;
        for (int m = 0; m < v.M; ++m) {
            s_nb[m] = nb;
            s_plo[m] = head;
            if (!s_opt[m]) { ++nb; head = m; }
        }
        s_nb[v.M] = nb;
        s_plo[v.M] = head;
    }
    __syncthreads();
    return s_flag[0] == 0;
}

// The tables this transcript reads: a NaN or +inf among them reaches the DP.  Thread m < M tests what entry m reads: init or
// the transition from the entry before it, and the last entry its closing score.
__device__ __forceinline__ bool align_tables_bad(const AlignVideo &v, const int *s_a, int tid)
{
    if (tid >= v.M) return false;
    const int c = s_a[tid];
    bool bad = align_bad_bits(tid == 0 ? v.init[c] : v.trans[(size_t)c * v.cm + s_a[tid - 1]]);
    if (tid == v.M - 1 && v.endpen) bad |= align_bad_bits(v.endpen[c]);
    return bad;
}

// ... with optional entries: init where first(m), the transitions from all of pred(m), the closing score where end(m)
__device__ __forceinline__ bool align_opt_tables_bad(const AlignVideo &v, const int *s_a, const int *s_nb, const int *s_plo, int tid)
{
    if (tid >= v.M) return false;
    const int c = s_a[tid];
    bool bad = s_nb[tid] == 0 && align_bad_bits(v.init[c]);
    for (int j = s_plo[tid]; j < tid; ++j) bad |= align_bad_bits(v.trans[(size_t)c * v.cm + s_a[j]]);
    if (v.endpen && tid >= s_plo[v.M]) bad |= align_bad_bits(v.endpen[c]);
    return bad;
}

// ---- a column
// the distances a column walks: -R .. d_all - 1 cover k = 1 .. kw
__device__ __forceinline__ int align_d_all(int kw) { return (kw + 1 + SMM_ALIGN_R - 1) / SMM_ALIGN_R * SMM_ALIGN_R; }

// the length scores of class c -> s_len (index k + R, -inf outside 1 .. kw); true where one of them is NaN or +inf.  No
// barrier behind them: align_tiles has one before any of its readers.
__device__ __forceinline__ bool align_stage_len(const double *len, int cm, int c, int kw, int d_all, double *s_len, int tid)
{
    bool bad = false;
    for (int j = tid; j < d_all + 3 * SMM_ALIGN_R; j += SMM_ALIGN_THREADS) {
        const int k = j - SMM_ALIGN_R;
        double v = SMM_NEG_INF;
        if (k >= 1 && k <= kw) {
            v = len[(size_t)k * cm + c];
            bad |= align_bad_bits(v);
        }
        s_len[j] = v;
    }
    return bad;
}

// The tile walk of one column: the targets [lo, hi] in tiles of SMM_ALIGN_P positions, the sources src(s), s in [slo, shi]
// (-inf outside), with the d_all - 1 before the tile in s_h.  A thread owns R consecutive targets from n0 and gets
// cells(n0, d_first, d_end, hp) once per tile: hp[-d] is the source at distance d = n0 - s, for the distances of the tile
// that can meet a source (whole steps of R; none, d_first >= d_end, for a tile out of every source's reach).
template <class Src, class Cells>
__device__ __forceinline__ void align_tiles(int lo, int hi, int slo, int shi, int d_all, double *s_h, int tid, Src src, Cells cells)
{
    for (int tb = lo; tb <= hi; tb += SMM_ALIGN_P) {
        // distances that can meet a source: tb - shi <= d <= tb + P - R - slo; whole steps of R, from -R (cell r at d has k = d + r)
        const int x = tb - shi, y = tb + SMM_ALIGN_P - SMM_ALIGN_R - slo + 1;
        const int y_up = (y + SMM_ALIGN_R - 1) / SMM_ALIGN_R * SMM_ALIGN_R;
        const int d_end = y_up < d_all ? y_up : d_all;
        const int d_first = x <= 0 ? -SMM_ALIGN_R : x / SMM_ALIGN_R * SMM_ALIGN_R;
        // LDS index i <-> position tb - OFF + i, for the positions tb - (d_end - 1) .. tb + P - R - d_first
        const int i_first = SMM_ALIGN_OFF - (d_end - 1), i_last = SMM_ALIGN_OFF + SMM_ALIGN_P - SMM_ALIGN_R - d_first;
        __syncthreads();                                       // the previous tile's readers; what the caller wrote for src
        for (int i = i_first + tid; i <= i_last; i += SMM_ALIGN_THREADS) {
            const int s = tb - SMM_ALIGN_OFF + i;
            s_h[i] = (s >= slo && s <= shi) ? src(s) : SMM_NEG_INF;
        }
        __syncthreads();
        const int n0 = tb + tid * SMM_ALIGN_R;
        if (n0 <= hi) cells(n0, d_first, d_end, s_h + SMM_ALIGN_OFF + tid * SMM_ALIGN_R);
    }
}

// ... of two columns with the same ranges at once (smm_align_graph_kl.hip: the two sides of a comparison): the same tiles, the
// same barriers, srcp -> s_hp and srcq -> s_hq; cells(n0, d_first, d_end, hp, hq).
template <class SrcP, class SrcQ, class Cells>
__device__ __forceinline__ void align_tiles2(int lo, int hi, int slo, int shi, int d_all, double *s_hp, double *s_hq, int tid,
                                             SrcP srcp, SrcQ srcq, Cells cells)
{
    for (int tb = lo; tb <= hi; tb += SMM_ALIGN_P) {
        const int x = tb - shi, y = tb + SMM_ALIGN_P - SMM_ALIGN_R - slo + 1;
        const int y_up = (y + SMM_ALIGN_R - 1) / SMM_ALIGN_R * SMM_ALIGN_R;
        const int d_end = y_up < d_all ? y_up : d_all;
        const int d_first = x <= 0 ? -SMM_ALIGN_R : x / SMM_ALIGN_R * SMM_ALIGN_R;
        const int i_first = SMM_ALIGN_OFF - (d_end - 1), i_last = SMM_ALIGN_OFF + SMM_ALIGN_P - SMM_ALIGN_R - d_first;
        __syncthreads();                                       // the previous tile's readers; what the caller wrote for the sources
        for (int i = i_first + tid; i <= i_last; i += SMM_ALIGN_THREADS) {
            const int s = tb - SMM_ALIGN_OFF + i;
            const bool in = s >= slo && s <= shi;
            s_hp[i] = in ? srcp(s) : SMM_NEG_INF;
            s_hq[i] = in ? srcq(s) : SMM_NEG_INF;
        }
        __syncthreads();
        const int n0 = tb + tid * SMM_ALIGN_R;
        if (n0 <= hi) cells(n0, d_first, d_end, s_hp + SMM_ALIGN_OFF + tid * SMM_ALIGN_R, s_hq + SMM_ALIGN_OFF + tid * SMM_ALIGN_R);
    }
}

// The sweep of a thread's R cells over the distances: f(r, h[n0 - d] + len[d + r]) for every d in [d_first, d_end) and cell r.
// One LDS read of h serves the R cells; the length scores slide through R registers, one broadcast read per step
// (lw[(d + r) % R] = len[d + r]; d_first is a multiple of R).
template <class F>
__device__ __forceinline__ void align_sweep(int d_first, int d_end, const double *hp, const double *s_len, F f)
{
    double lw[SMM_ALIGN_R];
#pragma unroll
    for (int q = 0; q < SMM_ALIGN_R - 1; ++q) lw[q] = s_len[d_first + q + SMM_ALIGN_R];
    for (int d0 = d_first; d0 < d_end; d0 += SMM_ALIGN_R) {
#pragma unroll
        for (int j = 0; j < SMM_ALIGN_R; ++j) {
            const int d = d0 + j;
            const double hv = hp[-d];
            lw[(j + SMM_ALIGN_R - 1) % SMM_ALIGN_R] = s_len[d + 2 * SMM_ALIGN_R - 1];
#pragma unroll
            for (int r = 0; r < SMM_ALIGN_R; ++r) f(r, hv + lw[(j + r) % SMM_ALIGN_R]);
        }
    }
}

// ... of two columns at once (align_tiles2): f(r, hp[n0 - d] + lenp[d + r], hq[n0 - d] + lenq[d + r])
template <class F>
__device__ __forceinline__ void align_sweep2(int d_first, int d_end, const double *hp, const double *hq, const double *s_lenp,
                                             const double *s_lenq, F f)
{
    double lp[SMM_ALIGN_R], lq[SMM_ALIGN_R];
#pragma unroll
    for (int q = 0; q < SMM_ALIGN_R - 1; ++q) {
        lp[q] = s_lenp[d_first + q + SMM_ALIGN_R];
        lq[q] = s_lenq[d_first + q + SMM_ALIGN_R];
    }
    for (int d0 = d_first; d0 < d_end; d0 += SMM_ALIGN_R) {
#pragma unroll
        for (int j = 0; j < SMM_ALIGN_R; ++j) {
            const int d = d0 + j;
            const double vp = hp[-d], vq = hq[-d];
            lp[(j + SMM_ALIGN_R - 1) % SMM_ALIGN_R] = s_lenp[d + 2 * SMM_ALIGN_R - 1];
            lq[(j + SMM_ALIGN_R - 1) % SMM_ALIGN_R] = s_lenq[d + 2 * SMM_ALIGN_R - 1];
#pragma unroll
            for (int r = 0; r < SMM_ALIGN_R; ++r) f(r, vp + lp[(j + r) % SMM_ALIGN_R], vq + lq[(j + r) % SMM_ALIGN_R]);
        }
    }
}

// the max-plus cells of a tile: acc[r] = max_d ( h[n0 + r - k] + len[k] )
__device__ __forceinline__ void align_sweep_max(int d_first, int d_end, const double *hp, const double *s_len, double *acc)
{
#pragma unroll
    for (int r = 0; r < SMM_ALIGN_R; ++r) acc[r] = SMM_NEG_INF;
    align_sweep(d_first, d_end, hp, s_len, [&](int r, double t) { acc[r] = align_max(acc[r], t); });
}

// One thread: the hulls of the per-class running values (maxima or log-sums, [C][T+1] behind a video's columns) after [lo, hi]
// was added to class c (lo > hi: nothing was); reset: a mandatory entry empties them first.  Per class only the hull
// [glo, ghi] of the cones that were added holds values; s_act lists the classes that hold any.
__device__ __forceinline__ void align_hull(int *s_glo, int *s_ghi, int *s_act, int *s_nact, bool reset, int c, int lo, int hi)
{
    int n = *s_nact;
    if (reset) {
        for (int i = 0; i < n; ++i) { s_glo[s_act[i]] = 1; s_ghi[s_act[i]] = 0; }
        n = 0;
    }
    if (lo <= hi) {
        if (s_glo[c] > s_ghi[c]) {
            s_act[n++] = c;
            s_glo[c] = lo;
            s_ghi[c] = hi;
        } else {
            s_glo[c] = lo < s_glo[c] ? lo : s_glo[c];
            s_ghi[c] = hi > s_ghi[c] ? hi : s_ghi[c];
        }
    }
    *s_nact = n;
}

// max_i ( G[act_i][n] + tr[i] ) over the classes whose hull holds n: what entry m reads at n from the run before it
__device__ __forceinline__ double align_class_max(const double *G, size_t T1, int n, int nact, const int *s_act, const int *s_glo,
                                                  const int *s_ghi, const double *s_tr)
{
    double mx = SMM_NEG_INF;
    for (int i = 0; i < nact; ++i) {
        const int cc = s_act[i];
        if (n >= s_glo[cc] && n <= s_ghi[cc]) mx = align_max(mx, G[(size_t)cc * T1 + n] + s_tr[i]);
    }
    return mx;
}

// ---- the alignment's outputs (smm_align.hip, smm_align_opt.hip, smm_align_graph.hip)
// a video without an alignment by counting, or with an id that is no state of it: no spans, no labels, best -inf
__device__ __forceinline__ void align_write_none(const SmmAlignArgs &a, const AlignVideo &v, int vid, int tid)
{
    if (a.spans)
        for (int q = tid; q <= a.t_max; q += SMM_ALIGN_THREADS) a.spans[(size_t)vid * (a.t_max + 1) + q] = -1;
    if (a.labels)
        for (int f = tid; f < v.T; f += SMM_ALIGN_THREADS) a.labels[v.frame_off + f] = -1;
    if (tid == 0) {
        if (a.best) a.best[vid] = SMM_NEG_INF;
        if (a.n_segs) a.n_segs[vid] = 0;
    }
}

// The segments seg0 .. M - 1 start at s_start[.] (s_start[seg0] = 0) and carry the state id_of(l): the segment of position q is
// the last one that starts at or before it.  failed: NaN and the error word; empty (failed, or the tables leave no
// alignment): -1 everywhere and no segments.
template <class IdOf>
__device__ __forceinline__ void align_write_result(const SmmAlignArgs &a, const AlignVideo &v, int vid, const int *s_start,
                                                   IdOf id_of, int seg0, bool failed, bool empty, double best, int tid)
{
    const int64_t *cmap = a.class_map ? a.class_map + (size_t)v.g * (v.cm + 1) : nullptr;
    int64_t *spans = a.spans ? a.spans + (size_t)vid * (a.t_max + 1) : nullptr;
    int64_t *labels = a.labels ? a.labels + v.frame_off : nullptr;
    const int64_t eos = cmap ? cmap[v.C] : (int64_t)v.C;
    const int q_end = a.t_max > v.T - 1 ? a.t_max : v.T - 1;
    for (int q = tid; q <= q_end; q += SMM_ALIGN_THREADS) {
        int64_t sp = -1, lb = -1;
        if (!empty && q < v.T) {
            int l = seg0, r = v.M - 1;
            while (l < r) {
                const int mid = (l + r + 1) >> 1;
                if (s_start[mid] <= q) l = mid; else r = mid - 1;
            }
            const int id = id_of(l);
            lb = cmap ? cmap[id] : (int64_t)id;
            if (s_start[l] == q) sp = lb;
        } else if (!empty && q == v.T) {
            sp = eos;
        }
        if (spans && q <= a.t_max) spans[q] = sp;
        if (labels && q < v.T) labels[q] = lb;
    }
    if (tid == 0) {
        if (failed) a.err[0] = 1;
        if (a.best) a.best[vid] = failed ? __builtin_nan("") : best;
        if (a.n_segs) a.n_segs[vid] = empty ? 0 : v.M - seg0;
    }
}

// ---- the g_elp kernels (smm_align_logz.hip, smm_align_opt_logz.hip), whose workgroups are their own size
// carry + the inclusive sum of x over the threads up to this one: within the wave by shuffles, the waves before this one through
// s_wave (a slot per wave; the caller alternates between two sets, the barrier here separates one call's writes from its reads)
__device__ __forceinline__ double align_block_scan(double x, double carry, double *s_wave, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double y = __shfl_up(x, off);
        if (lane >= off) x = x + y;
    }
    if (lane == 63) s_wave[wave] = x;
    __syncthreads();
    double before = carry;
    for (int w = 0; w < wave; ++w) before = before + s_wave[w];
    return before + x;
}

// a tile's rows of class sums (s_acc, ld doubles per frame) -> g_elp rows of nr frames, times u; the columns beyond C are zero
__device__ __forceinline__ void align_store_rows(double *g_elp, const double *s_acc, int ld, int nr, int cm, int C, double u,
                                                 int tid, int nthreads)
{
    for (int e = tid; e < nr * cm; e += nthreads) {
        const int r = e / cm, c = e - r * cm;
        g_elp[e] = c < C ? u * s_acc[r * ld + c] : 0.0;
    }
}
