// smm_align_graph.h -- what the six transcript-graph units share, each stated once.  The units:
//   smm_align_graph.hip              the best alignment over the paths of a graph
//   smm_align_graph_logz.hip         the sum over them, forward and backward
//   smm_align_graph_sample.hip       alignments drawn from their posterior
//   smm_align_graph_entropy.hip      the entropy of that posterior
//   smm_align_graph_kl.hip           the KL and cross-entropy between two such posteriors
//   smm_align_graph_entropy_bwd.hip  the gradients of the three
// First what the two forward kernels need: the structure in LDS, the path lengths, the cells of a column that lie on a complete
// alignment, the test of the tables the structure reads, the compaction of a ballot into a list.  Then what the readers of the
// forward kernel's workspace block share (from "the posterior" on): the recorded range of a column, the column blocks of a
// video, the neighbour lists of a column, the candidates of the end and predecessor decisions, what a video of a two-sided
// kernel answers that cannot be evaluated, q's side of such a call, the block sum, and the scratch view and the video states of
// the two gradient units (smm_align_graph_entropy_bwd.hip, smm_align_graph_expected_reward.hip).
// Include after smm_align_tile.h.
#pragma once

#define SMM_GRAPH_WORDS (SMM_MAX_TRANSCRIPT / 32)                // mask words per node
#define SMM_GRAPH_FAR 0x3fffffff                                 // "no path": more nodes than any path has

static_assert(SMM_MAX_TRANSCRIPT == SMM_ALIGN_THREADS, "thread j stands for node j when a column lists its neighbours");

// node j may directly precede node m (mask: the video's rows, in LDS or in global memory)
__device__ __forceinline__ bool graph_edge(const uint32_t *mask, int m, int j)
{
    return (mask[m * SMM_GRAPH_WORDS + (j >> 5)] >> (j & 31)) & 1u;
}

__device__ __forceinline__ int graph_wave_max(int x) { return -align_wave_min(-x); }

// this lane's slot among the set lanes of a ballot
__device__ __forceinline__ int graph_rank(unsigned long long ballot, int lane)
{
    return __popcll(ballot & ((1ull << lane) - 1ull));
}

// The structure -> LDS: classes, flags and the 8-word masks.  An id must be a state of the video, a mask may name earlier
// nodes only: s_flag[0] (cleared by the caller behind a barrier) is raised otherwise.  The caller puts a barrier behind it.
// MASKS false: the same tests without the masks in LDS (the two-sided kernels, whose two sides' tiles and length scores leave
// no 8 KB for them; s_mask null); a column then reads the mask rows in global memory (graph_edge on a.pred_mask's rows of the
// video).  A template flag: a null test of an LDS pointer stays in the code as eight branches and takes the 16-byte loads apart.
template <bool MASKS, class Args>
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
            if (MASKS) s_mask[tid * SMM_GRAPH_WORDS + w] = word;
        }
        if (!ok) s_flag[0] = 1;
    }
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

// ------------------------------------------------------------------------------------------------ the posterior
// What the readers of the block the forward kernel leaves per video share (smm_launch.h: smm_graph_block_doubles).

#define SMM_GRAPH_RNG 5                                          // ints per column at the head of the block
static_assert(SMM_GRAPH_RNG * sizeof(int) <= SMM_GRAPH_HEAD * sizeof(double), "a column's range fits its share of the head");

// The recorded range of column m: gam[.][m] and q[.][m] hold values on [lo, hi] (lo > hi: a node without a cell), h[.][m] and
// bh[.][m] on [slo, shi] and, when z, at 0.  Everything else in the block is uninitialised memory: every read of a column is
// gated by its range BEFORE the load.  smm_align_graph_logz_fwd_kernel is the only writer.
struct GraphRange {
    int lo, hi, slo, shi, z;
    // the first position that holds a D of the gradient's span terms (smm_align_graph_entropy_bwd.hip)
    __device__ __forceinline__ int dlo() const { return z ? 0 : (slo <= shi && slo < lo ? slo : lo); }
};

__device__ __forceinline__ const int *graph_rng(const double *block) { return reinterpret_cast<const int *>(block); }

__device__ __forceinline__ GraphRange graph_range(const int *rng, int m)
{
    const int *r = rng + SMM_GRAPH_RNG * m;
    return {r[0], r[1], r[2], r[3], r[4]};
}

// q's range of column m is p's.  It is a function of graph, T and span limit only: a difference says that q's workspace was
// written for other graphs, and nothing of its columns may be read through p's ranges.
__device__ __forceinline__ bool graph_range_differs(const int *rng, const int *rngq, int m)
{
    const int *r = rng + SMM_GRAPH_RNG * m, *rq = rngq + SMM_GRAPH_RNG * m;
    return rq[0] != r[0] || rq[1] != r[1] || rq[2] != r[2] || rq[3] != r[3] || rq[4] != r[4];
}

// The int arrays of a node each that a posterior kernel keeps in LDS, and one view of them for the helpers below
struct GraphNodes {
    int *a, *fl;                                               // class; bit 0: start(m), bit 1: end(m)
    int *lo, *hi, *slo, *shi, *z;                              // the columns' ranges
    int *pl;                                                   // the neighbours of the column
    int *wcnt, *wlo, *whi;                                     // graph_compact's
};
#define GRAPH_SHARED_NODES                                                                                                       \
    __shared__ int s_a[SMM_MAX_TRANSCRIPT], s_fl[SMM_MAX_TRANSCRIPT];                                                            \
    __shared__ int s_lo[SMM_MAX_TRANSCRIPT], s_hi[SMM_MAX_TRANSCRIPT], s_slo[SMM_MAX_TRANSCRIPT], s_shi[SMM_MAX_TRANSCRIPT];     \
    __shared__ int s_z[SMM_MAX_TRANSCRIPT], s_pl[SMM_MAX_TRANSCRIPT];                                                            \
    __shared__ int s_wcnt[4], s_wlo[4], s_whi[4];                                                                                \
    __shared__ int s_flag[2];                                  /* [0] an id or a mask bit out of range, [1] the kernel's own */  \
    const GraphNodes nd = {s_a, s_fl, s_lo, s_hi, s_slo, s_shi, s_z, s_pl, s_wcnt, s_wlo, s_whi}
// ... with the column's length scores and the listed transitions of both sides of a two-sided kernel
#define GRAPH_SHARED_SIDES                                                                                                       \
    __shared__ double s_lenp[SMM_ALIGN_LEN], s_lenq[SMM_ALIGN_LEN];                                                              \
    __shared__ double s_trp[SMM_MAX_TRANSCRIPT], s_trq[SMM_MAX_TRANSCRIPT];   /* trans[a_m][a_j], j = s_pl[i], of each side */   \
    GRAPH_SHARED_NODES

__device__ __forceinline__ GraphRange graph_range(const GraphNodes &s, int m) { return {s.lo[m], s.hi[m], s.slo[m], s.shi[m], s.z[m]}; }

// every column's range -> LDS, thread m its own.  The caller puts a fence and a barrier behind it.
__device__ __forceinline__ void graph_load_ranges(const int *rng, const GraphNodes &s, int M, int tid)
{
    if (tid < M) {
        const GraphRange r = graph_range(rng, tid);
        s.lo[tid] = r.lo; s.hi[tid] = r.hi; s.slo[tid] = r.slo; s.shi[tid] = r.shi; s.z[tid] = r.z;
    }
}

// A two-sided kernel's load: classes, flags and p's ranges -> LDS, the masks stay in global memory; false where the structure is
// invalid or q's ranges are not p's.  Every thread calls it, once both log Z are finite (they had a valid structure and wrote
// their ranges); its barriers are the caller's too.
template <class Args>
__device__ __forceinline__ bool graph_load_sides(const Args &a, const AlignVideo &v, const int *rng, const int *rngq,
                                                 const GraphNodes &s, int *s_flag, int tid)
{
    if (tid < 2) s_flag[tid] = 0;
    __syncthreads();
    graph_load<false>(a, v, s.a, s.fl, nullptr, s_flag, tid);
    graph_load_ranges(rng, s, v.M, tid);
    if (tid < v.M && graph_range_differs(rng, rngq, tid)) s_flag[1] = 1;
    __threadfence_block();
    __syncthreads();
    return s_flag[0] == 0 && s_flag[1] == 0;
}

// The column blocks of a video behind the head of its block, each [M][T+1] (D: double or const double)
template <class D>
struct GraphCols {
    D *h, *g, *q, *bh;
};

template <class D>
__device__ __forceinline__ GraphCols<D> graph_cols(D *block, int M, size_t T1)
{
    GraphCols<D> c;
    c.h = block + SMM_GRAPH_HEAD * (size_t)M;
    c.g = c.h + (size_t)M * T1;
    c.q = c.g + (size_t)M * T1;
    c.bh = c.q + (size_t)M * T1;
    return c;
}

// ---- the neighbours of column m -> s.pl in index order; tr(slot, node) per listed node, for the caller's transitions; -> their
// number.  SUCC false: pred(m), the nodes in front of m that have cells (the forward kernels, which also want the hull of those
// cells, keep their own statement of it); true: succ(m), the later nodes that name m in their own mask and hold bh values (no
// transposed masks).  Every thread calls it; graph_compact's barrier inside, the caller's behind it.
template <bool SUCC, class Tr>
__device__ __forceinline__ int graph_list(const uint32_t *mask, int m, int M, const GraphNodes &s, int tid, Tr tr)
{
    const int *lo = SUCC ? s.slo : s.lo, *hi = SUCC ? s.shi : s.hi;
    const bool is = (SUCC ? tid > m && tid < M && graph_edge(mask, tid, m) : tid < m && graph_edge(mask, m, tid)) && lo[tid] <= hi[tid];
    int slot, np, ulo, uhi;
    graph_compact(is, is ? lo[tid] : 0, is ? hi[tid] : 0, s.wcnt, s.wlo, s.whi, tid, slot, np, ulo, uhi);
    if (is) {
        s.pl[slot] = tid;
        tr(slot, tid);
    }
    return np;
}

// ---- the candidates of two decisions of smm_align_graph_sample.hip's walk, in the order in which every kernel sums them.  The
// caller's f forms the weights; how they are summed is its business (three different sums).
__device__ __forceinline__ double graph_closing(const double *endpen, int c) { return endpen ? endpen[c] : 0.0; }

// the end node: f(j) for the end nodes that hold the cell (T, j), in index order
template <class F>
__device__ __forceinline__ void graph_each_end(const GraphNodes &s, int M, int T, F f)
{
    for (int j = 0; j < M; ++j)
        if ((s.fl[j] & 2) && s.lo[j] <= T && T <= s.hi[j]) f(j);
}

// the node in front of a segment that starts at pos: f(i, j) for the listed j = s.pl[i] that hold the cell (pos, j)
template <class F>
__device__ __forceinline__ void graph_each_pred(const GraphNodes &s, int np, int pos, F f)
{
    for (int i = 0; i < np; ++i) {
        const int j = s.pl[i];
        if (pos >= s.lo[j] && pos <= s.hi[j]) f(i, j);
    }
}

// ---- what a video of a two-sided kernel answers whose two log Z do not allow an evaluation, or whose structure or ranges
// failed behind finite ones: p without an alignment: NaN, silently; p with one and q without: +inf; a NaN or +inf on
// either side, or the failure behind a finite pair: NaN and the error word (staging cleared the word the forward call had set)
struct GraphVerdict {
    bool bad, both, q_none;                                    // both: evaluate (-inf: no alignment, an ordinary "impossible")
    __device__ __forceinline__ double answer() const { return q_none ? __builtin_huge_val() : __builtin_nan(""); }
    __device__ __forceinline__ bool error() const { return bad || both; }
};

__device__ __forceinline__ GraphVerdict graph_verdict(double lzp, double lzq)
{
    GraphVerdict d;
    d.bad = align_bad_bits(lzp) || align_bad_bits(lzq);
    d.both = !d.bad && !align_nonfinite_bits(lzp) && !align_nonfinite_bits(lzq);
    d.q_none = !d.bad && !align_nonfinite_bits(lzp) && align_nonfinite_bits(lzq);
    return d;
}

// ---- q's side of a two-sided call for one video: trans and len of its group, its closing row (the rest as it is)
__device__ __forceinline__ SmmAlignSideQ graph_side_q(SmmAlignSideQ q, const AlignVideo &v, int k_rows, int vid)
{
    q.trans += (size_t)v.g * v.cm * v.cm;
    q.len += (size_t)v.g * k_rows * v.cm;
    q.endpen = q.endpen ? q.endpen + (size_t)vid * v.cm : nullptr;
    return q;
}

// ---- the caller's scratch of the gradient units, one layout for both (smm_launch.h: SmmAlignEntBwdArgs): per video five
// [M][T+1] blocks behind 5 x the cells in front of it; behind pv_base the videos' parts, [b] doubles of the entropy unit, V+ [b]
struct GraphGradScratch {
    double *em_s, *em_e, *ep_e, *ep_s, *dd;                    // eta-S, eta-E, eta+E, eta+S, D: each [M][T+1]
    double *part, *vals;                                       // the video's parts; vals[0] = V-, vals[1] = state
    double *vplus;
};

__device__ __forceinline__ GraphGradScratch graph_grad_scratch(const SmmAlignEntBwdArgs &a, const AlignVideo &v, int vid)
{
    GraphGradScratch x;
    const size_t MT = (size_t)v.M * v.T1;
    const int64_t cells = smm_graph_cells_before(a.g.hoff[vid], v.t0 - a.g.toff[0]);
    x.em_s = a.scratch + 5 * cells; x.em_e = x.em_s + MT; x.ep_e = x.em_e + MT; x.ep_s = x.ep_e + MT; x.dd = x.ep_s + MT;
    const size_t pf = smm_agb_part_doubles(v.cm, a.g.k_rows);
    x.part = a.scratch + a.pv_base + (size_t)vid * pf;
    x.vals = x.part + pf - 2;
    x.vplus = a.scratch + a.pv_base + (size_t)a.g.b * (pf + 1) + vid;
    return x;
}

// a video's state (smm_launch.h) from its V-: NaN: nothing to sum; +inf or -inf: NaN rows; finite: its terms are summed
__device__ __forceinline__ double graph_grad_state(double val)
{
    return align_nonfinite_bits(val) ? (val != val ? SMM_AGB_SKIP : SMM_AGB_NAN) : SMM_AGB_RUN;
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
