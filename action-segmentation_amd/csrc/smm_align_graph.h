// smm_align_graph.h -- what the transcript-graph kernels share (smm_align_graph.hip: the best alignment over the paths of a
// graph; smm_align_graph_logz.hip: the sum over them; smm_align_graph_entropy.hip: the entropy of their posterior;
// smm_align_graph_kl.hip: the KL between two such posteriors): the
// structure in LDS, the path lengths, the cells of a column that lie
// on a complete alignment, the test of the tables the structure reads, the compaction of a ballot into a list, and the block
// sum of the posterior kernels (smm_align_graph_logz.hip, smm_align_graph_entropy.hip).
// Include after smm_align_tile.h.
#pragma once

#define SMM_GRAPH_WORDS (SMM_MAX_TRANSCRIPT / 32)                // mask words per node
#define SMM_GRAPH_FAR 0x3fffffff                                 // "no path": more nodes than any path has

static_assert(SMM_MAX_TRANSCRIPT == SMM_ALIGN_THREADS, "thread j stands for node j when a column lists its neighbours");

// node j may directly precede node m
__device__ __forceinline__ bool graph_edge(const uint32_t *s_mask, int m, int j)
{
    return (s_mask[m * SMM_GRAPH_WORDS + (j >> 5)] >> (j & 31)) & 1u;
}

__device__ __forceinline__ int graph_wave_max(int x) { return -align_wave_min(-x); }

// this lane's slot among the set lanes of a ballot
__device__ __forceinline__ int graph_rank(unsigned long long ballot, int lane)
{
    return __popcll(ballot & ((1ull << lane) - 1ull));
}

// The structure -> LDS: classes, flags and the 8-word masks.  An id must be a state of the video, a mask may name earlier
// nodes only: s_flag[0] (cleared by the caller behind a barrier) is raised otherwise.  The caller puts a barrier behind it.
template <class Args>
__device__ __forceinline__ void graph_load(const Args &a, const AlignVideo &v, int *s_a, int *s_fl, uint32_t *s_mask, int *s_flag,
                                           int tid)
{
    if (tid < v.M) {
        const int id = a.transcript[v.t0 + tid];
        bool ok = id >= 0 && id < v.C;
        s_a[tid] = ok ? id : 0;
        s_fl[tid] = a.node_flags[v.t0 + tid] & 3;
        const uint32_t *mask = a.pred_mask + (size_t)(v.t0 + tid) * SMM_GRAPH_WORDS;
#pragma unroll
        for (int w = 0; w < SMM_GRAPH_WORDS; ++w) {
            const uint32_t word = mask[w];
            const int below = tid - 32 * w;                    // bits of this word that name a node before tid
            const uint32_t allowed = below <= 0 ? 0u : below >= 32 ? 0xffffffffu : (1u << below) - 1u;
            ok &= (word & ~allowed) == 0;
            s_mask[tid * SMM_GRAPH_WORDS + w] = word;
        }
        if (!ok) s_flag[0] = 1;
    }
}

// ... without the masks in LDS (smm_align_graph_kl.hip, whose two sides' tiles leave no 8 KB for them): the same tests, classes
// and flags -> LDS; a column then reads its own mask row from global memory (graph_edge_row).
template <class Args>
__device__ __forceinline__ void graph_load_nodes(const Args &a, const AlignVideo &v, int *s_a, int *s_fl, int *s_flag, int tid)
{
    if (tid < v.M) {
        const int id = a.transcript[v.t0 + tid];
        bool ok = id >= 0 && id < v.C;
        s_a[tid] = ok ? id : 0;
        s_fl[tid] = a.node_flags[v.t0 + tid] & 3;
        const uint32_t *mask = a.pred_mask + (size_t)(v.t0 + tid) * SMM_GRAPH_WORDS;
#pragma unroll
        for (int w = 0; w < SMM_GRAPH_WORDS; ++w) {
            const int below = tid - 32 * w;
            const uint32_t allowed = below <= 0 ? 0u : below >= 32 ? 0xffffffffu : (1u << below) - 1u;
            ok &= (mask[w] & ~allowed) == 0;
        }
        if (!ok) s_flag[0] = 1;
    }
}

// node j < SMM_MAX_TRANSCRIPT may directly precede the node whose mask row this is (8 words in global memory)
__device__ __forceinline__ bool graph_edge_row(const uint32_t *row, int j)
{
    return (row[j >> 5] >> (j & 31)) & 1u;
}

// Path lengths (wave 0 calls it, tid < 64; serially in topological order; the fences order a lane's writes before the other
// lanes' reads): the fewest / most nodes before a node on a path from a start node (bmin, bmax; bmax < 0: no start node
// reaches it) and after it on a path to an end node (amin, amax; amax < 0: it reaches no end node); s_len2[0], [1]: the fewest
// and most nodes on a start -> end path ([1] < 0: there is none).  The caller puts a barrier behind it.
__device__ __forceinline__ void graph_path_lengths(const uint32_t *s_mask, const int *s_fl, int M, int *s_bmin, int *s_bmax,
                                                   int *s_amin, int *s_amax, int *s_len2, int tid)
{
    for (int m = 0; m < M; ++m) {
        int mn = SMM_GRAPH_FAR, mx = -1;
        for (int j = tid; j < m; j += 64) {
            const int bj = s_bmax[j];
            if (bj >= 0 && graph_edge(s_mask, m, j)) {
                const int t = s_bmin[j] + 1;
                mn = t < mn ? t : mn;
                mx = bj + 1 > mx ? bj + 1 : mx;
            }
        }
        mn = align_wave_min(mn);
        mx = graph_wave_max(mx);
        if (s_fl[m] & 1) { mn = 0; mx = mx > 0 ? mx : 0; }
        if (tid == 0) { s_bmin[m] = mn; s_bmax[m] = mx; }
        __threadfence_block();
    }
    for (int j = tid; j < M; j += 64) {
        const bool e = (s_fl[j] & 2) != 0;
        s_amin[j] = e ? 0 : SMM_GRAPH_FAR;
        s_amax[j] = e ? 0 : -1;
    }
    __threadfence_block();
    for (int m = M - 1; m > 0; --m) {                          // every successor of m has pushed: m is final, and pushes
        const int an = s_amin[m], ax = s_amax[m];
        if (ax >= 0)
            for (int j = tid; j < m; j += 64)
                if (graph_edge(s_mask, m, j)) {
                    if (an + 1 < s_amin[j]) s_amin[j] = an + 1;
                    if (ax + 1 > s_amax[j]) s_amax[j] = ax + 1;
                }
        __threadfence_block();
    }
    int lmin = SMM_GRAPH_FAR, lmax = -1;
    for (int j = tid; j < M; j += 64)
        if ((s_fl[j] & 2) && s_bmax[j] >= 0) {
            lmin = s_bmin[j] + 1 < lmin ? s_bmin[j] + 1 : lmin;
            lmax = s_bmax[j] + 1 > lmax ? s_bmax[j] + 1 : lmax;
        }
    lmin = align_wave_min(lmin);
    lmax = graph_wave_max(lmax);
    if (tid == 0) { s_len2[0] = lmin; s_len2[1] = lmax; }
}

// thread m < M: the cells of column m that lie on a complete alignment (lo > hi: none; a node off every start -> end path has
// none): align_opt_range with nb -> bmin, na -> amin, m -> bmax, M-1-m -> amax
__device__ __forceinline__ void graph_cells(int M, int T, int kw, const int *s_bmin, const int *s_bmax, const int *s_amin,
                                            const int *s_amax, int *s_lo, int *s_hi, int tid)
{
    if (tid < M) {
        int lo = 1, hi = 0;
        if (s_bmax[tid] >= 0 && s_amax[tid] >= 0) {
            const int p = s_bmin[tid] + 1, q = T - s_amax[tid] * kw;
            const int r = T - s_amin[tid], s = (s_bmax[tid] + 1) * kw;
            lo = p > q ? p : q;
            hi = r < s ? r : s;
            if (lo > hi) { lo = 1; hi = 0; }
        }
        s_lo[tid] = lo;
        s_hi[tid] = hi;
    }
}

// no alignment by counting: no start -> end path, the shortest needs more frames than there are, the longest at the span limit
// does not reach T
__device__ __forceinline__ bool graph_no_path(const int *s_len2, int T, int kw)
{
    return s_len2[1] < 0 || s_len2[0] > T || (int64_t)s_len2[1] * kw < T;
}

// The tables the structure reads, on a start -> end path or not: init where start(m), the transition of every edge, the closing
// score where end(m) (the length scores: as their column stages them).  Thread m < M tests what node m reads.
__device__ __forceinline__ bool graph_tables_bad(const AlignVideo &v, const int *s_a, const int *s_fl, const uint32_t *s_mask, int tid)
{
    if (tid >= v.M) return false;
    const int c = s_a[tid];
    bool bad = (s_fl[tid] & 1) && align_bad_bits(v.init[c]);
    for (int w = 0; w * 32 < tid; ++w) {
        uint32_t word = s_mask[tid * SMM_GRAPH_WORDS + w];
        while (word) {
            const int j = w * 32 + __builtin_ctz(word);
            word &= word - 1;
            bad |= align_bad_bits(v.trans[(size_t)c * v.cm + s_a[j]]);
        }
    }
    if (v.endpen && (s_fl[tid] & 2)) bad |= align_bad_bits(v.endpen[c]);
    return bad;
}

// The neighbours of a column (is: this thread's node is one; lo, hi: its positions) -> s_list in index order, the waves in
// order; slot: this thread's place in the list (for an `is` thread), np: their number, [ulo, uhi]: the hull of their positions.
// Every thread of the workgroup calls it; it holds one barrier; the caller puts one behind its own writes to the list's slots.
__device__ __forceinline__ void graph_compact(bool is, int lo, int hi, int *s_wcnt, int *s_wlo, int *s_whi, int tid, int &slot,
                                              int &np, int &ulo, int &uhi)
{
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long ballot = __ballot(is);
    const int wl = align_wave_min(is ? lo : SMM_GRAPH_FAR), wh = graph_wave_max(is ? hi : 0);
    if (lane == 0) { s_wcnt[wave] = __popcll(ballot); s_wlo[wave] = wl; s_whi[wave] = wh; }
    __syncthreads();
    int before = 0;
    np = 0; ulo = SMM_GRAPH_FAR; uhi = 0;
#pragma unroll
    for (int w = 0; w < SMM_ALIGN_THREADS / 64; ++w) {
        if (w < wave) before += s_wcnt[w];
        np += s_wcnt[w];
        ulo = s_wlo[w] < ulo ? s_wlo[w] : ulo;
        uhi = s_whi[w] > uhi ? s_whi[w] : uhi;
    }
    slot = before + graph_rank(ballot, lane);
}

// the sum of x over the workgroup, in every thread: a butterfly per wave, the waves in order
__device__ __forceinline__ double graph_block_sum(double x, double *s_red, int tid)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off);
    __syncthreads();                                           // the readers of the sum before this one
    if ((tid & 63) == 0) s_red[tid >> 6] = x;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < SMM_ALIGN_THREADS / 64; ++w) s = s + s_red[w];
    return s;
}
