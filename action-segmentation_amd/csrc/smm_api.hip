// smm_api.hip -- host side of libsmmdp.so: argument checks, launch planning, C ABI (include/smmdp.h).
#include <algorithm>
#include <atomic>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>
#include <unordered_map>
#include <mutex>
#include <utility>
#include <string>

#include "../../include/smmdp.h"
#include "smm_device.h"
#include "smm_launch.h"
#include "smm_plan_feedback.h"

static thread_local int g_last_hip = 0;

// ------------------------------------------------------------------------------------------------ tuning switches
// Read ONCE, when the library is first used, and again whenever smm_env_reload() is called (tests and A/B scripts that
// flip a switch inside one process call it; nothing on the per-call path touches the environment).  Release builds know
// the switches of the first block only; the ones that change RESULTS (profiling stops, half-run splits) exist in
// -DSMM_DEV builds alone.
namespace {
struct SmmEnv {
    int spec = 1;             // SMM_SPEC=0: Viterbi without the speculative transition (A/B aid; same results)
    int no_split = 0;         // SMM_NO_SPLIT=1: smm_decode_f32 never splits a launch over two streams (same results)
    double split_min_us = 100.0, split_ns = 0.0;     // SMM_SPLIT_MIN_US, SMM_SPLIT_NS (0: from smm_band_frame_ns), SMM_SPLIT_MARGIN: choose_split's model
    int split_margin = 400;
    int plan_cache = 1;       // SMM_PLAN_CACHE=0: no resident plans
    int small_wg = 1;         // SMM_SMALL_WG=0: no four-wave workgroups for <= 16-state videos; 2: wherever they apply, whatever the part's size (tests; same results)
    int plan_feedback = 1;    // SMM_PLAN_FEEDBACK=0: a resident plan's stream split is never re-planned from measured times; 2: re-planned after the
                              // first complete measurement whatever the predicted gain (tests; same results)
    int chunk = 1;            // SMM_CHUNK=0: no time-split decode of long videos (same results)
    int chunk_p = 0;          // SMM_CHUNK_P: positions per unit of a time-split decode (0: from the launch's CU-time; tests force small ones)
    int chunk_lmin = 0;       // SMM_CHUNK_LMIN: least own part of a unit (0: SMM_CHUNK_LMIN below; never less than kp - 1 or 130)
    int chunk_wc = 512;       // SMM_CHUNK_WC: warm-up positions of a unit in front of the kp - 1 it is certified on (at most kp)
    int no_bt_window = 0;     // SMM_NO_BT_WINDOW=1: the general back-trace also for kp <= 64 (same results)
    int fit_grid = 0;         // SMM_FIT_GRID: workgroups of the class-sums kernel (tuning aid)
    int verbose = 0;          // SMM_VERBOSE
#ifdef SMM_DEV
    int debug_flags = 0;      // SMM_DEBUG_FLAGS: SmmDpArgs::flags bits (bit 0: stop after the forward pass -- outputs UNDEFINED)
    int split_debug = 0;      // SMM_SPLIT_DEBUG: leave parts of a split decode out (results INCOMPLETE)
    int upload_memcpy = 0;    // SMM_UPLOAD_MEMCPY: metadata by hipMemcpyAsync instead of kernel arguments
    int emission_v2 = 0;      // SMM_EMISSION_V2: the LDS-staged emission variant (slower)
#endif
    std::string key;          // what the planning functions depend on, for the resident plans' keys
};
// The current set of switches.  Other threads hold `const SmmEnv &` from env() across a whole call (plan_key reads
// env().key), so a reload never writes into a struct that has been published: it publishes a NEW one, and the old ones
// stay allocated (a few hundred bytes per smm_env_reload(), which only tests and A/B scripts call).
std::atomic<const SmmEnv *> g_env{nullptr};
std::once_flag g_env_once;

void env_read()
{
    SmmEnv e;
    struct Item { const char *name; int *i; double *d; };
    const Item items[] = {
        {"SMM_SPEC", &e.spec, nullptr}, {"SMM_NO_SPLIT", &e.no_split, nullptr}, {"SMM_SPLIT_MIN_US", nullptr, &e.split_min_us},
        {"SMM_SPLIT_NS", nullptr, &e.split_ns}, {"SMM_SPLIT_MARGIN", &e.split_margin, nullptr},
        {"SMM_PLAN_CACHE", &e.plan_cache, nullptr}, {"SMM_SMALL_WG", &e.small_wg, nullptr}, {"SMM_PLAN_FEEDBACK", &e.plan_feedback, nullptr}, {"SMM_CHUNK", &e.chunk, nullptr}, {"SMM_CHUNK_P", &e.chunk_p, nullptr},
        {"SMM_CHUNK_WC", &e.chunk_wc, nullptr}, {"SMM_CHUNK_LMIN", &e.chunk_lmin, nullptr}, {"SMM_NO_BT_WINDOW", &e.no_bt_window, nullptr},
        {"SMM_FIT_GRID", &e.fit_grid, nullptr}, {"SMM_VERBOSE", &e.verbose, nullptr},
#ifdef SMM_DEV
        {"SMM_DEBUG_FLAGS", &e.debug_flags, nullptr}, {"SMM_SPLIT_DEBUG", &e.split_debug, nullptr},
        {"SMM_UPLOAD_MEMCPY", &e.upload_memcpy, nullptr}, {"SMM_EMISSION_V2", &e.emission_v2, nullptr},
#endif
    };
    for (const Item &it : items) {
        const char *v = std::getenv(it.name);
        if (!v) continue;
        if (it.i) *it.i = (*v == 0) ? 1 : std::atoi(v);        // (a switch set to the empty string counts as set)
        if (it.d) *it.d = std::atof(v);
        e.key += it.name; e.key += '='; e.key += v; e.key += ';';
    }
    g_env.store(new SmmEnv(e), std::memory_order_release);
}
const SmmEnv &env()
{
    std::call_once(g_env_once, env_read);
    return *g_env.load(std::memory_order_acquire);
}
}  // namespace

extern "C" void smm_env_reload(void)
{
    (void)env();
    env_read();
}
int smm_env_fit_grid() { return env().fit_grid; }
int smm_env_emission_v2()
{
#ifdef SMM_DEV
    return env().emission_v2;
#else
    return 0;
#endif
}

#define SMM_HIP(call)                                                         \
    do {                                                                      \
        hipError_t e_ = (call);                                               \
        if (e_ != hipSuccess) { g_last_hip = (int)e_; return SMM_ERR_HIP; }   \
    } while (0)

extern "C" const char *smm_strerror(int status)
{
    switch (status) {
    case SMM_OK: return "ok";
    case SMM_ERR_ARG: return "invalid argument";
    case SMM_ERR_UNSUPPORTED: return "shape not supported by the compiled kernels";
    case SMM_ERR_WORKSPACE: return "workspace too small";
    case SMM_ERR_HIP: return "HIP runtime error";
    case SMM_ERR_NO_DEVICE: return "no gfx950 device";
    default: return "unknown smm_status";
    }
}

extern "C" int smm_last_hip_error(void) { return g_last_hip; }
extern "C" const char *smm_version(void) { return "smmdp 0.1 (gfx950)"; }

extern "C" int smm_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ------------------------------------------------------------------------------------------------ metadata upload
struct SmmMetaChunk { uint32_t w[512]; };

__global__ void __launch_bounds__(512) smm_meta_upload_kernel(SmmMetaChunk c, uint32_t *dst, int n)
{
    // the chunk is the first kernel argument: read it from the kernel-argument segment with a per-thread offset (indexing
    // the by-value struct would make the compiler copy all of it into scratch first)
    typedef const __attribute__((address_space(4))) uint32_t *smm_kernarg_ptr;
    (void)c;
#if defined(__HIP_DEVICE_COMPILE__)
    smm_kernarg_ptr ka = (smm_kernarg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    if ((int)threadIdx.x < n) dst[threadIdx.x] = ka[threadIdx.x];
#else
    (void)dst; (void)n;
#endif
}

int smm_upload_meta(void *dst_dev, const void *src_host, size_t bytes, hipStream_t stream)
{
#ifdef SMM_DEV
    if (env().upload_memcpy) return (int)hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, stream);
#endif
    const size_t words = (bytes + 3) / 4;                    // (every destination is padded to 256 B by the planners)
    const unsigned char *src = static_cast<const unsigned char *>(src_host);
    for (size_t off = 0; off < words; off += 512) {
        SmmMetaChunk c;
        const size_t n = std::min<size_t>(512, words - off);
        const size_t nb = std::min<size_t>(n * 4, bytes - off * 4);
        std::memset(&c, 0, sizeof(c));
        std::memcpy(c.w, src + off * 4, nb);
        hipLaunchKernelGGL(smm_meta_upload_kernel, dim3(1), dim3(512), 0, stream, c, static_cast<uint32_t *>(dst_dev) + off, (int)n);
    }
    return (int)hipGetLastError();
}

// Zero fill by a kernel of ours instead of hipMemsetAsync: a memset node captured into a hipGraph came back from the
// SECOND replay on with a 16-byte pattern of stale kernel arguments instead of zeros (ROCm 7.2, found by
// tests/test_gpu_graph.py: error words and gang counters full of pointers) -- kernel nodes replay correctly.
__global__ void __launch_bounds__(256) smm_zero_kernel(uint32_t *p, size_t nwords)
{
    const size_t head = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2;    // words before 16-byte alignment
    const size_t h = head < nwords ? head : nwords;
    const size_t nq = (nwords - h) >> 2;                                               // 16-byte pieces
    uint4 *q = reinterpret_cast<uint4 *>(p + h);
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nth = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < nq; i += nth) q[i] = make_uint4(0, 0, 0, 0);
    if (tid < h) p[tid] = 0;
    const size_t tail0 = h + 4 * nq;
    if (tid < nwords - tail0) p[tail0 + tid] = 0;
}

// Several regions in ONE launch (grid.y = region): the gradient buffers of a backward entry point were zeroed by three to six
// launches of ~4 us each back to back -- 15 per training step on cfg4, a quarter of everything that is not the DP there.
struct SmmZeroRegions { uint32_t *p[8]; size_t nwords[8]; };
__global__ void __launch_bounds__(256) smm_zero_multi_kernel(SmmZeroRegions r)
{
    uint32_t *p = r.p[blockIdx.y];
    const size_t nwords = r.nwords[blockIdx.y];
    const size_t head = ((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) >> 2;
    const size_t h = head < nwords ? head : nwords;
    const size_t nq = (nwords - h) >> 2;
    uint4 *q = reinterpret_cast<uint4 *>(p + h);
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nth = (size_t)gridDim.x * 256;
    for (size_t i = tid; i < nq; i += nth) q[i] = make_uint4(0, 0, 0, 0);
    if (tid < h) p[tid] = 0;
    const size_t tail0 = h + 4 * nq;
    if (tid < nwords - tail0) p[tail0 + tid] = 0;
}

int smm_zero_multi_async(void *const *dst_dev, const size_t *bytes, int n, hipStream_t stream)
{
    SmmZeroRegions r{};
    int m = 0;
    size_t most = 0;
    for (int i = 0; i < n; ++i) {
        if (bytes[i] == 0) continue;
        if (m == 8 || (bytes[i] & 3) || (reinterpret_cast<uintptr_t>(dst_dev[i]) & 3)) {       // (never: at most six word-made buffers here)
            const int rc = smm_zero_async(dst_dev[i], bytes[i], stream);
            if (rc != (int)hipSuccess) return rc;
            continue;
        }
        r.p[m] = static_cast<uint32_t *>(dst_dev[i]);
        r.nwords[m] = bytes[i] >> 2;
        most = r.nwords[m] > most ? r.nwords[m] : most;
        ++m;
    }
    if (m == 0) return (int)hipSuccess;
    size_t blocks = (most / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(smm_zero_multi_kernel, dim3((unsigned)blocks, (unsigned)m), dim3(256), 0, stream, r);
    return (int)hipGetLastError();
}

int smm_zero_async(void *dst_dev, size_t bytes, hipStream_t stream)
{
    if (bytes == 0) return (int)hipSuccess;
    if ((bytes & 3) || (reinterpret_cast<uintptr_t>(dst_dev) & 3)) return (int)hipMemsetAsync(dst_dev, 0, bytes, stream);   // (never: every buffer here is made of 4- or 8-byte words)
    const size_t nwords = bytes >> 2;
    size_t blocks = (nwords / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(smm_zero_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<uint32_t *>(dst_dev), nwords);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ planning
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct SmmPlan {
    size_t meta_bytes;     // SmmVideo[b] | order[b] | n_states[g] | emission block table[b+1] | err
    size_t o_order, o_nstates, o_emcum, o_err;
    size_t hist_doubles;   // sum over videos of 8*c_max*(T+1): forward cumE/h/gamma, backward cumE/h/gamma, 2 transposes
    size_t elp_doubles;    // total_frames*c_max  (smm_decode_f32 / smm_viterbi_f32)
    size_t tab_doubles;    // widened tables       (smm_viterbi_f32)
    size_t band_doubles;   // Viterbi BAND mode: state-major length table + skip-test bounds per (group, state)
    size_t b;              // videos
    size_t chunk_bytes;    // Viterbi, time-split videos: redo words | anchors | (not resident: the units' metadata); an upper bound
    size_t o_chunk;        // ... its offset in the workspace
    size_t total;
};

// Upper bounds of a time-split plan (the workspace is sized before anything is planned): a unit's own part is never shorter
// than SMM_CHUNK_LMIN positions, so a video of T frames has at most T / SMM_CHUNK_LMIN + 1 units
constexpr int SMM_CHUNK_LMIN = 512;                 // ... or 2 kp where that is less (kp > 64: at least 130)
constexpr int SMM_CHUNK_LMIN_FINE = 384;            // (plan_chunks: where one more unit per video still fits one round of workgroups)
static size_t chunk_units_max(const smm_shape *s) { return (size_t)(s->total_frames / 128) + 2 * (size_t)s->b; }
static size_t chunk_ext_meta_bytes(size_t b, size_t units, size_t n_cv)
{
    return align_up(sizeof(SmmVideo) * (b + units), 256) + align_up(sizeof(int32_t) * (b + units), 256) +
           align_up(sizeof(SmmChunkVideo) * n_cv, 256) + align_up(sizeof(int32_t) * n_cv, 256);
}

static bool shape_ok(const smm_shape *s)
{
    return s && s->b > 0 && s->n_groups > 0 && s->c_max > 0 && s->k_rows >= 2 && s->t_max > 0 && s->total_frames > 0;
}

// (of a shape that is shape_ok) within what the kernels are compiled for / every video has 1..t_max frames
static bool limits_ok(const smm_shape *s) { return s->c_max <= SMM_MAX_STATES && s->k_rows <= SMM_MAX_K_ROWS; }
static bool lengths_ok(const smm_shape *s, const int64_t *lengths)
{
    for (int i = 0; i < s->b; ++i)
        if (lengths[i] < 1 || lengths[i] > s->t_max) return false;
    return true;
}

// Regions of a workspace, one behind the other: take() rounds the next region's start up to 256 bytes, packed() does not
// (regions that go up in one upload)
struct Carver {
    size_t cur;
    size_t packed(size_t bytes) { const size_t o = cur; cur += bytes; return o; }
    size_t take(size_t bytes) { const size_t o = packed(bytes); cur = align_up(cur, 256); return o; }
};

// the metadata in front of a plan (what smm_error_word_offset tells python, too)
static void plan_meta(const smm_shape *s, SmmPlan *p)
{
    Carver c{0};
    c.take(sizeof(SmmVideo) * s->b);
    p->o_order = c.take(sizeof(int32_t) * s->b);
    p->o_nstates = c.take(sizeof(int32_t) * s->n_groups);
    p->o_emcum = c.take(sizeof(int32_t) * ((size_t)s->b + 1));
    p->o_err = c.cur;
    p->meta_bytes = p->o_err + 512;   // error word + diagnostic counters
}

static SmmPlan make_plan(const smm_shape *s, const int64_t *lengths)
{
    SmmPlan p{};
    p.b = (size_t)s->b;
    plan_meta(s, &p);
    size_t h = 0;
    for (int i = 0; i < s->b; ++i) h += 8 * (size_t)s->c_max * (size_t)(lengths[i] + 1);
    p.hist_doubles = h;
    p.elp_doubles = (size_t)s->total_frames * s->c_max;
    p.tab_doubles = (size_t)s->n_groups * s->c_max * ((size_t)s->c_max + 1 + s->k_rows) + (size_t)s->b * s->c_max;
    p.band_doubles = (size_t)s->n_groups * s->c_max * ((size_t)SMM_BAND_ROW + SMM_BAND_TAB + 64);   // len_t | band_tab | dmin_t
    {
        const size_t um = chunk_units_max(s);
        p.chunk_bytes = align_up(sizeof(int32_t) * s->b, 256) + align_up(sizeof(double) * um * s->c_max, 256) +
                        chunk_ext_meta_bytes(s->b, um, s->b);
    }
    p.o_chunk = align_up(p.meta_bytes + 8 * (p.hist_doubles + p.elp_doubles + p.tab_doubles + p.band_doubles), 256);
    p.total = p.o_chunk + p.chunk_bytes + 1024;
    return p;
}

extern "C" size_t smm_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host)
{
    if (!shape_ok(shape) || !lengths_host || !lengths_ok(shape, lengths_host)) return 0;
    return make_plan(shape, lengths_host).total;
}

extern "C" size_t smm_error_word_offset(const smm_shape *shape)
{
    if (!shape_ok(shape)) return 0;
    SmmPlan p{};
    plan_meta(shape, &p);
    return p.o_err;
}

struct Staged {
    SmmVideo *videos;
    int32_t *order;
    int32_t *n_states;
    int32_t *err;
    double *hist;
    double *elp;
    double *tabs;
    double *band;          // [g][c_max][k_rows] len_t | [g][c_max][16] band bounds
    bool band_mode;        // Viterbi at K > 512: BAND mode (smm_viterbi.hip)
    int32_t *em_cum;       // emission: workgroups before each video of `order` ([b + 1])
    std::vector<int32_t> em_cum_host;   // (decode split: the same table on the host)
    int em_tpw, em_blocks;
    int kp_max, c_need;
    int n_split;           // decode only: the first n_split videos of `order` are the launch's critical path (0: no split)
    // time-split videos (Viterbi; smm_chunk.hip).  n_cv = 0: none.  uvideos = [the b videos | the units]; uorder = the DP
    // launch's order over [unsplit videos, units] -- the units first (u_part1 of them: with a stream split they are its first part)
    SmmVideo *uvideos;
    int32_t *uorder, *porder;     // porder: the split videos, for the repair launch
    SmmChunkVideo *cvs;
    int32_t *redo;
    double *anchors;
    int n_cv, n_units, u_part1;
    // the LAST part of the DP launch order (the rest of a stream split, or the whole launch) ends with small_count units of <= 16
    // states that run in four-wave workgroups, two per CU, beside the others (smm_viterbi.hip: smm_launch_viterbi_small); 0: none
    int small_first, small_count;
    // plan feedback (below, "Plan feedback"): where this call's DP workgroups stamp their start and end (null: nowhere), the
    // event the call records behind its join, and the resident plan it runs from
    uint64_t *stamps = nullptr;
    hipEvent_t done = nullptr;
    void *fb_entry = nullptr;
    std::vector<int32_t> order_host, frames_host;   // (stream split, on the way to a new resident plan only: `order` and T by video)
};

static bool band_mode(int kp_max, int c_need);

// Validates the metadata, builds SmmVideo[] (+ longest-first block order) and stages it into the workspace.
// for_viterbi: the call launches the Viterbi kernel (part of a resident plan's key; rounds 1-3 planned gangs here: only
// the entry points that launch that kernel ask for it)
// Split of a decode (smm_decode_f32) into [critical videos | the rest].  The DP kernel's time is the time of the launch's
// longest videos (one workgroup each, ~0.3 us per frame), while the emission scorer in front of it streams EVERY video's
// features (0.6 ms on cfg3).  With the few longest videos scored first, their DP can start at once and the rest of the
// corpus is scored -- and then decoded -- on a second stream beside it: the second part must be through before the first
// is, i.e. its longest video has to be shorter than the launch's longest by the time the emission scorer takes.
// Returns how many videos of `order` (reordered: critical ones first, both parts keep their order) form the first part;
// 0: no split (few videos, a flat length distribution, or nothing to hide).
static int device_cus()
{
    static std::mutex mu;
    static int n_cu[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
    std::lock_guard<std::mutex> lock(mu);
    if (!n_cu[dev] && hipDeviceGetAttribute(&n_cu[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n_cu[dev] = 0;
    return n_cu[dev] > 0 ? n_cu[dev] : 0;
}

// ns per frame of one BAND-mode video on its CU (include/smmdp.h).  Measured, round 4's final kernels, CrossTask-like
// lattices of 64 x 4096 frames (profiles/round4_band_stamps.txt): 167 / 172 / 186 / 191 ns at 11 / 16 / 20 / 23 states.
// Re-fit these two numbers when the kernel changes; everything that needs the kernel's speed reads them from here.
constexpr double SMM_BAND_NS_BASE = 145.0, SMM_BAND_NS_PER_STATE = 2.0;
extern "C" double smm_band_frame_ns(int n_states)
{
    if (n_states < 1 || n_states > SMM_MAX_STATES) return 0.0;
    return SMM_BAND_NS_BASE + SMM_BAND_NS_PER_STATE * n_states;
}

// Modelled ns per frame of one video on its CU: BAND mode by the library's model, the ring kernels (span limits up to 512: cfg2's
// 16 states at K = 256 take 199 ns per frame) by theirs.  A DP launch is ordered by T x this, most work first.
static double dp_frame_ns(bool band, int c) { return band ? smm_band_frame_ns(c) : 150.0 + 3.0 * c; }

static int choose_split(const SmmVideo *hv, int32_t *order, int b, int d, int c_max, int64_t total_frames)
{
    const SmmEnv &ev = env();
    if (b < 24 || ev.no_split) return 0;
    const int n_cu = device_cus();
    if (n_cu <= 0) return 0;
    const double em_us = (double)total_frames * (4.0 * d + 8.0 * c_max) / 4.0e6;      // ~4 TB/s of algorithmic bytes
    if (em_us < ev.split_min_us) return 0;                                             // (SMM_SPLIT_MIN_US: test hook, split small launches too)
    int tmax = 0;
    for (int i = 0; i < b; ++i) tmax = std::max(tmax, hv[i].T);
    // a video of the second part starts em_us later than the critical ones and must not outlast them: the critical set is
    // the videos within em_us / split_ns + margin frames of the longest.  Same-box scan on cfg3 (scripts/gpu_ab_cfg3.sh,
    // BAND kernel of round 3, ~250 ns per frame beside a full GPU): 230 / 250 ns 3.72-3.74 ms per step, 300 3.58-3.62,
    // 400 3.59-3.62, 600 3.65-3.71, 1000+ 3.68-3.70 -- the em_us estimate below (4 TB/s) is already on the long side.
    // SMM_SPLIT_NS / SMM_SPLIT_MARGIN: tuning aids
    // (round 5: the slack per microsecond of emission follows the kernel's own speed -- split_slack x the modelled ns per
    // frame of the launch's largest class set, 1.75 x 191 = 334 at 23 states, the value the scans above settled on when it
    // was a literal -- instead of being re-fitted by hand each time the DP kernel gets faster; SMM_SPLIT_NS overrides)
    const double split_ns = ev.split_ns > 0.0 ? ev.split_ns : 1.75 * smm_band_frame_ns(std::min(c_max, (int)SMM_MAX_STATES));
    const int thr = tmax - (int)(em_us * 1000.0 / split_ns) - ev.split_margin;
    int n1 = 0;
    for (int i = 0; i < b; ++i) n1 += hv[i].T >= thr;
    // ... and only a launch that is bound by its longest videos: with more than two rounds of workgroups the DP is bound by
    // CU-time and the split only adds a second launch (scripts/sweep_split.py, round 4: 1000 videos of ~2000 frames lost
    // 3.8 % with it; every latency-bound distribution won 5..10 % or stayed level)
    if (thr <= 0 || n1 < 1 || n1 > b / 3 || n1 > n_cu / 2 || b - n1 < 16 || b > 2 * n_cu) return 0;
    std::stable_partition(order, order + b, [&](int32_t v) { return hv[v].T >= thr; });
    return n1;
}

// ---------------------------------------------------------------------------------------------------------------
// Resident plans.  Staging a call is host work (ordering the videos, the split, the emission grid) plus the upload of
// the metadata in 2 KB kernel-argument chunks -- about 0.2 ms in front of the first real kernel of a 360-video
// launch, every call, although a training loop decodes the SAME batches every epoch.  A staged call is therefore kept:
// the immutable part of the metadata (videos | order | n_states | emission block table) lives in a device buffer the
// LIBRARY owns -- nobody else can write to it, so a later call with bit-identical inputs (compared in full, not by hash)
// and the same planning environment points its kernels at that buffer and skips planning and upload.  The mutable
// part (the error words) stays in the caller's workspace and is cleared per call as before.
// Lifetime: a plan is ADMITTED the second time its inputs are seen (a training loop that packs shuffled batches shows a new
// key every step: those are staged the old way and leave nothing behind); plans live in slabs of the device they were
// made on, 64 MB at most per process, and stay until smm_release_cached_plans() frees them (the caller's promise: no
// call in flight and no captured graph that was captured from one of these calls still to be replayed).  With
// SMM_PLAN_CACHE=0, past the cap, or when a call with new inputs happens under stream capture (no allocation, no event
// query there), a call is staged into its workspace as before.
//
// Plan feedback.  The stream split of a decode is planned from a model -- (T, states) -> time -- that predicts a video's DP time
// to +-15 % (BAND mode skips what its bound tests exclude: the time depends on the lattice), and a launch ends with its slowest
// video.  A resident plan is decoded again and again, so the library MEASURES instead: a call that runs from (or admits) a
// resident plan with a stream split, no time-split videos and no small-workgroup tail hands the DP kernels a pinned host
// buffer, [b][2] ticks of the 100 MHz wall clock, and records an event behind its join.  A later call on that plan that
// finds the event complete (queried, never waited for; nothing of this under stream capture) takes the times and, once its
// own launches are queued, replays the step from them (smm_plan_feedback.h).  If a first part made of the videos that
// really are the slowest ends the replayed step at least 2 % sooner, the plan's launch order and emission block table are
// written into a FRESH region of the plan slabs and the entry's pointers are swapped on the host: the old region stays valid
// until smm_release_cached_plans(), so a call in flight or a captured graph never sees a buffer change under it.  Only who
// starts when changes: every video is decoded by the same kernel on the same inputs.  An entry is re-planned at most 4 times
// and stops measuring at the first measurement that offers no such gain.  SMM_PLAN_FEEDBACK=0: never; 2: tests.
namespace {
struct PlanFeedback {
    uint64_t *stamps = nullptr;              // pinned host memory, [b][2]: the DP workgroups write, the host reads behind `done`
    hipEvent_t done = nullptr;
    bool pending = false;                    // a stamping call has been queued and its stamps have not been looked at yet
    bool have = false;                       // `snap` is a complete measurement nobody has evaluated yet
    bool busy = false;                       // a thread is evaluating it
    int evals_left = 5, n_replans = 0;
    int b = 0, n1_first = 0;
    double em_us = 0.0, end_before_us = 0.0, end_after_us = 0.0;
    std::vector<uint64_t> snap, used;        // the latest complete measurement; the one the last evaluation was made from
    std::vector<int32_t> order, frames;      // host copies: the plan's current launch order, T by video
};
constexpr int SMM_FEEDBACK_MAX_REPLANS = 4;
constexpr double SMM_FEEDBACK_MIN_GAIN = 0.02;
struct PlanEntry {
    PlanFeedback *fb = nullptr;
    std::vector<char> key;
    int device = 0;
    char *dev_meta = nullptr;
    SmmPlan plan{};
    Staged st{};
    hipEvent_t ready = nullptr;
    hipStream_t stream = nullptr;
    bool settled = false;
};
struct PlanSlabs {                                                      // per device: metadata buffers are cut from 1 MB slabs
    char *cur = nullptr;
    size_t left = 0;
    std::vector<std::pair<char *, size_t>> all;                         // (slab, its real size: a plan larger than 1 MB gets its own)
};
struct PlanCache {
    std::mutex mu;
    std::unordered_map<uint64_t, std::vector<PlanEntry *>> entries;     // by FNV-1a of the key; compared in full on a hit
    std::unordered_map<uint64_t, uint32_t> seen_once;                   // keys seen once (hash only): admitted at the second sighting
    size_t n = 0, bytes = 0, key_bytes = 0;                            // plans, device bytes, host bytes of their keys
    size_t pinned_bytes = 0;                                           // pinned host bytes of the plans' stamp buffers
    uint64_t generation = 1;                                           // bumped by smm_release_cached_plans()
    PlanSlabs slabs[64];
} g_plans;
constexpr size_t SMM_PLAN_MAX_BYTES = (size_t)64 << 20, SMM_PLAN_MAX_ENTRIES = 8192, SMM_PLAN_SLAB = (size_t)1 << 20;

uint64_t plan_hash(const std::vector<char> &k)
{
    uint64_t h = 1469598103934665603ull;
    for (unsigned char c : k) { h ^= c; h *= 1099511628211ull; }
    return h;
}

// (called with the cache locked; `dev` is the current device: a plan's buffer lives on the device its kernels run on)
char *plan_alloc(size_t bytes, int dev)
{
    if (dev < 0 || dev >= 64) return nullptr;
    PlanSlabs &sl = g_plans.slabs[dev];
    bytes = align_up(bytes, 256);
    if (bytes > sl.left) {
        const size_t want = std::max(bytes, SMM_PLAN_SLAB);
        char *p = nullptr;
        if (hipMalloc(reinterpret_cast<void **>(&p), want) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        sl.all.emplace_back(p, want);      // (the rest of the previous slab is given up)
        sl.cur = p;
        sl.left = want;
    }
    char *r = sl.cur;
    sl.cur += bytes;
    sl.left -= bytes;
    return r;
}

void plan_key_append(std::vector<char> &k, const void *p, size_t n)
{
    const char *c = static_cast<const char *>(p);
    k.insert(k.end(), c, c + n);
}

std::vector<char> plan_key(const smm_shape *s, const int64_t *lengths, const int64_t *frame_off, const int32_t *group,
                           const int32_t *kp, const int32_t *n_states, bool for_viterbi, int cum_chunk, bool want_split)
{
    std::vector<char> k;
    k.reserve(sizeof(*s) + (size_t)s->b * 24 + (size_t)s->n_groups * 4 + 128);
    plan_key_append(k, s, sizeof(*s));
    plan_key_append(k, lengths, sizeof(int64_t) * s->b);
    plan_key_append(k, frame_off, sizeof(int64_t) * s->b);
    const char has[2] = {(char)(group != nullptr), (char)(kp != nullptr)};
    plan_key_append(k, has, 2);
    if (group) plan_key_append(k, group, sizeof(int32_t) * s->b);
    if (kp) plan_key_append(k, kp, sizeof(int32_t) * s->b);
    plan_key_append(k, n_states, sizeof(int32_t) * s->n_groups);
    const int32_t f[3] = {for_viterbi, cum_chunk, want_split};
    plan_key_append(k, f, sizeof(f));
    // the switches the planning functions read (smm_env_reload() may change them between calls)
    const std::string &ek = env().key;
    plan_key_append(k, ek.data(), ek.size() + 1);
    return k;
}

// (cache locked) a call is about to run from resident plan `e`: take a finished measurement, arm the next one
void feedback_arm(PlanEntry *e, Staged *out)
{
    PlanFeedback *fb = e->fb;
    if (!fb || !env().plan_feedback) return;
    out->fb_entry = e;
    if (fb->pending) {
        if (hipEventQuery(fb->done) != hipSuccess) { (void)hipGetLastError(); return; }      // (still running: this call does not stamp)
        fb->pending = false;
        bool complete = !fb->have && !fb->busy;
        for (int i = 0; complete && i < fb->b; ++i) complete = fb->stamps[2 * i] > 0 && fb->stamps[2 * i + 1] >= fb->stamps[2 * i];
        if (complete) { fb->snap.assign(fb->stamps, fb->stamps + 2 * (size_t)fb->b); fb->have = true; }
    }
    // (a measurement that waits for its evaluation at the end of this call may change the plan: nothing is measured beside it)
    if (fb->evals_left > 0 && !fb->have && !fb->busy) {
        std::memset(fb->stamps, 0, sizeof(uint64_t) * 2 * (size_t)fb->b);
        out->stamps = fb->stamps;
        out->done = fb->done;
        fb->pending = true;
    }
}

void plan_point(const SmmPlan &p, void *ws, Staged *out)
{
    char *base = static_cast<char *>(ws);
    out->err = reinterpret_cast<int32_t *>(base + p.o_err);
    out->hist = reinterpret_cast<double *>(base + p.meta_bytes);
    out->elp = out->hist + p.hist_doubles;
    out->tabs = out->elp + p.elp_doubles;
    out->band = out->tabs + p.tab_doubles;
    out->redo = reinterpret_cast<int32_t *>(base + p.o_chunk);
    out->anchors = reinterpret_cast<double *>(base + p.o_chunk + align_up(sizeof(int32_t) * p.b, 256));
}
}  // namespace

// meta_alloc(bytes): where the IMMUTABLE metadata of this call goes when it is to be kept as a resident plan (called once,
// with the exact size, after the host-side planning); nullptr result / no function: into the workspace
static int stage_uncached(const smm_shape *s, const int64_t *lengths, const int64_t *frame_off, const int32_t *group,
                          const int32_t *kp, const int32_t *n_states, void *ws, size_t ws_bytes, hipStream_t stream, Staged *out,
                          bool for_viterbi, int cum_chunk, bool want_split, const std::function<char *(size_t)> *meta_alloc,
                          SmmPlan *plan_out);

static int stage(const smm_shape *s, const int64_t *lengths, const int64_t *frame_off, const int32_t *group,
                 const int32_t *kp, const int32_t *n_states, void *ws, size_t ws_bytes, hipStream_t stream, Staged *out,
                 bool for_viterbi = false, int cum_chunk = 0, bool want_split = false)
{
    if (!shape_ok(s) || !lengths || !frame_off || !n_states || !ws) return SMM_ERR_ARG;
    if (!env().plan_cache) return stage_uncached(s, lengths, frame_off, group, kp, n_states, ws, ws_bytes, stream, out, for_viterbi, cum_chunk, want_split, nullptr, nullptr);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cap) != hipSuccess) cap = hipStreamCaptureStatusNone;
    const bool capturing = cap != hipStreamCaptureStatusNone;
    const std::vector<char> key = plan_key(s, lengths, frame_off, group, kp, n_states, for_viterbi, cum_chunk, want_split);
    const uint64_t hk = plan_hash(key) ^ (uint64_t)dev;
    PlanEntry *hit = nullptr;
    {
        std::lock_guard<std::mutex> lock(g_plans.mu);
        auto it = g_plans.entries.find(hk);
        if (it != g_plans.entries.end())
            for (PlanEntry *e : it->second)
                if (e->device == dev && e->key.size() == key.size() && std::memcmp(e->key.data(), key.data(), key.size()) == 0) { hit = e; break; }
        if (hit && !hit->settled) {
            // the upload was queued on another stream, maybe: usable once it is known to be through (or on that very
            // stream).  Under capture nothing is queried or waited for (an event query can invalidate a global-mode capture):
            // an unsettled plan is then simply not used.
            if (capturing) { if (hit->stream != stream) hit = nullptr; }
            else if (hipEventQuery(hit->ready) == hipSuccess) hit->settled = true;
            else if (hit->stream != stream && hipStreamWaitEvent(stream, hit->ready, 0) != hipSuccess) hit = nullptr;
        }
    }
    if (hit) {
        if (ws_bytes < hit->plan.total) return SMM_ERR_WORKSPACE;
        {
            std::lock_guard<std::mutex> lock(g_plans.mu);      // (a re-plan swaps the entry's pointers under this lock)
            *out = hit->st;
            if (!capturing && for_viterbi && want_split) feedback_arm(hit, out);
        }
        plan_point(hit->plan, ws, out);
        char *base = static_cast<char *>(ws);
        SMM_HIP((hipError_t)smm_zero_async(base + hit->plan.o_err, hit->plan.meta_bytes - hit->plan.o_err, stream));
        return SMM_OK;
    }
    // miss: stage, and keep the plan unless this is a capture (no allocation there) or the cache is full
    char *dev_meta = nullptr;
    bool keep = !capturing;
    if (keep) {
        std::lock_guard<std::mutex> lock(g_plans.mu);
        // admitted at the second sighting: one-off batches (shuffled training steps) never take a slot
        auto seen = g_plans.seen_once.find(hk);
        if (seen == g_plans.seen_once.end()) {
            if (g_plans.seen_once.size() >= 4 * SMM_PLAN_MAX_ENTRIES) g_plans.seen_once.clear();
            g_plans.seen_once.emplace(hk, 1u);
            keep = false;
        }
    }
    // (called by stage_uncached once the size of the immutable metadata is known: the videos, and the units of a time-split plan)
    const std::function<char *(size_t)> alloc = [&](size_t bytes) -> char * {
        std::lock_guard<std::mutex> lock(g_plans.mu);
        if (!(g_plans.bytes + bytes <= SMM_PLAN_MAX_BYTES && g_plans.n < SMM_PLAN_MAX_ENTRIES &&
              g_plans.key_bytes + key.size() <= SMM_PLAN_MAX_BYTES)) return nullptr;
        dev_meta = plan_alloc(bytes, dev);
        if (dev_meta) g_plans.bytes += align_up(bytes, 256);
        return dev_meta;
    };
    SmmPlan plan{};
    const int rc = stage_uncached(s, lengths, frame_off, group, kp, n_states, ws, ws_bytes, stream, out, for_viterbi, cum_chunk, want_split,
                                  keep ? &alloc : nullptr, &plan);
    keep = keep && dev_meta != nullptr;
    if (rc != SMM_OK || !keep) return rc;          // (a buffer cut for a call that failed stays cut: 64 MB bound the total)
    PlanEntry *e = new PlanEntry;
    e->key = key;
    e->device = dev;
    e->dev_meta = dev_meta;
    e->plan = plan;
    PlanFeedback *fb = nullptr;
    std::vector<int32_t> order_host = std::move(out->order_host), frames_host = std::move(out->frames_host);
    out->order_host.clear(); out->frames_host.clear();
    e->st = *out;
    e->stream = stream;
    // plan feedback: this call, the one that admits the plan, is the first to be measured
    if (for_viterbi && want_split && env().plan_feedback && out->n_split > 0 && out->n_cv == 0 && out->small_count == 0 &&
        (int)order_host.size() == s->b) {
        fb = new PlanFeedback;
        const size_t bytes = sizeof(uint64_t) * 2 * (size_t)s->b;
        if (hipHostMalloc(reinterpret_cast<void **>(&fb->stamps), bytes, hipHostMallocDefault) != hipSuccess) fb->stamps = nullptr;
        if (fb->stamps && hipEventCreateWithFlags(&fb->done, hipEventDisableTiming) != hipSuccess) fb->done = nullptr;
        if (!fb->stamps || !fb->done) {
            (void)hipGetLastError();
            if (fb->stamps) (void)hipHostFree(fb->stamps);
            delete fb;
            fb = nullptr;
        } else {
            fb->b = s->b;
            fb->n1_first = out->n_split;
            fb->em_us = (double)s->total_frames * (4.0 * s->d + 8.0 * s->c_max) / 4.0e6;      // choose_split's emission model
            fb->order = std::move(order_host);
            fb->frames = std::move(frames_host);
            std::memset(fb->stamps, 0, bytes);
            fb->pending = true;
            out->stamps = fb->stamps;
            out->done = fb->done;
        }
    }
    e->fb = fb;
    auto drop_fb = [&]() {
        if (!fb) return;
        out->stamps = nullptr; out->done = nullptr;             // (this call then runs unmeasured)
        (void)hipHostFree(fb->stamps);
        (void)hipEventDestroy(fb->done);
        delete fb;
    };
    if (hipEventCreateWithFlags(&e->ready, hipEventDisableTiming) != hipSuccess || hipEventRecord(e->ready, stream) != hipSuccess) {
        // (cannot tell later whether the upload is through: this call is fine -- same stream -- but the plan is not kept)
        if (e->ready) (void)hipEventDestroy(e->ready);
        drop_fb();
        delete e;
        return SMM_OK;     // dev_meta stays allocated: this call's kernels read it
    }
    std::lock_guard<std::mutex> lock(g_plans.mu);
    if (fb) { g_plans.pinned_bytes += sizeof(uint64_t) * 2 * (size_t)s->b; out->fb_entry = e; }
    g_plans.entries[hk].push_back(e);
    g_plans.seen_once.erase(hk);
    g_plans.n += 1;
    g_plans.key_bytes += key.size();
    return SMM_OK;
}

// Frees every resident plan and its device memory (all devices), the decode's second streams and the pooled events.
// The caller's promise: no libsmmdp call is in flight on any stream, and no hipGraph captured from one of these calls will
// be replayed again (a captured call points at its plan's buffer).  Returns the device bytes given back.
static void release_aux();
extern "C" size_t smm_release_cached_plans(void)
{
    release_aux();
    std::lock_guard<std::mutex> lock(g_plans.mu);
    int cur = 0;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    size_t freed = 0;
    for (auto &kv : g_plans.entries)
        for (PlanEntry *e : kv.second) {
            if (e->ready) (void)hipEventDestroy(e->ready);
            if (e->fb) {
                (void)hipHostFree(e->fb->stamps);
                (void)hipEventDestroy(e->fb->done);
                delete e->fb;
            }
            delete e;
        }
    freed += g_plans.pinned_bytes;
    g_plans.pinned_bytes = 0;
    g_plans.generation += 1;
    g_plans.entries.clear();
    g_plans.seen_once.clear();
    for (int d = 0; d < 64; ++d) {
        PlanSlabs &sl = g_plans.slabs[d];
        if (sl.all.empty()) continue;
        (void)hipSetDevice(d);
        for (auto &ps : sl.all) if (hipFree(ps.first) == hipSuccess) freed += ps.second;
        sl = PlanSlabs{};
    }
    if (have_cur) (void)hipSetDevice(cur);
    g_plans.n = g_plans.bytes = g_plans.key_bytes = 0;
    return freed;
}

extern "C" size_t smm_cached_plan_bytes(void)
{
    std::lock_guard<std::mutex> lock(g_plans.mu);
    size_t n = g_plans.pinned_bytes;                 // (the plans' stamp buffers: pinned host memory)
    for (int d = 0; d < 64; ++d)
        for (auto &ps : g_plans.slabs[d].all) n += ps.second;
    return n;
}

// ---- plan feedback: the evaluation, at the END of a decode call (its launches are queued: the host work hides behind them)
namespace {
struct FeedbackInfo {
    uint64_t generation = 0;
    smm_plan_feedback_info_t info{};
};
thread_local FeedbackInfo g_fb_info;

void feedback_info_set(const PlanFeedback *fb, int n1_now)        // (cache locked)
{
    g_fb_info.generation = g_plans.generation;
    smm_plan_feedback_info_t &o = g_fb_info.info;
    o.n_replans = fb->n_replans;
    o.n1_before = fb->n1_first;
    o.n1_after = n1_now;
    o.n_videos = fb->b;
    o.end_before_us = fb->end_before_us;
    o.end_after_us = fb->end_after_us;
    o.stamps = fb->used.empty() ? nullptr : fb->used.data();
    o.order = fb->order.data();
}

// st: what the call ran from; stream: the caller's (the new metadata is uploaded behind the call's own work)
void feedback_evaluate(const Staged &st, hipStream_t stream)
{
    PlanEntry *e = static_cast<PlanEntry *>(st.fb_entry);
    if (!e || !e->fb) return;
    PlanFeedback *fb = e->fb;
    std::vector<uint64_t> snap;
    std::vector<int32_t> order;
    int n1 = 0;
    {
        std::lock_guard<std::mutex> lock(g_plans.mu);
        if (!fb->have || fb->busy || fb->evals_left <= 0) { feedback_info_set(fb, e->st.n_split); return; }
        fb->busy = true;
        snap = fb->snap;
        order = fb->order;
        n1 = e->st.n_split;
    }
    const SmmEnv &ev = env();
    const int b = fb->b, n_cu = device_cus();
    std::vector<double> dur(b);
    for (int i = 0; i < b; ++i) dur[i] = (double)(snap[2 * i + 1] - snap[2 * i]) * 0.01;       // 100 MHz ticks -> us
    const bool force = ev.plan_feedback >= 2;
    // the emission pass's time, measured as well: the rest's first workgroup started (1 - the first part's share of the frames) of
    // it behind the first part's (the model's 4 TB/s are on the fast side: cfg3 603 us modelled, 690 measured); kept within a
    // factor of two of the model, so that a launch whose emission is a few microseconds is not planned around launch gaps
    double em_us = fb->em_us;
    {
        uint64_t s1 = ~0ull, s2 = ~0ull;
        double f1 = 0.0, f_all = 0.0;
        for (int i = 0; i < b; ++i) {
            const int v = order[i];
            (i < n1 ? s1 : s2) = std::min(i < n1 ? s1 : s2, snap[2 * (size_t)v]);
            f_all += fb->frames[v];
            if (i < n1) f1 += fb->frames[v];
        }
        if (s2 > s1 && f_all > f1) em_us = std::min(2.0 * fb->em_us, std::max(0.5 * fb->em_us, (double)(s2 - s1) * 0.01 * f_all / (f_all - f1)));
    }
    const SmmFeedbackPlan plan = smm_feedback_plan(dur.data(), fb->frames.data(), order.data(), b, n1, n_cu, em_us, force);
    const bool planned = smm_feedback_guards(b, n_cu, plan.n1) && plan.end_chosen_us > 0.0;
    bool replan = planned && (force || (plan.changed && plan.end_chosen_us <= (1.0 - SMM_FEEDBACK_MIN_GAIN) * plan.end_current_us));
    // the new metadata: launch order | emission block table, in the DP's new order
    const size_t o_cum = align_up(sizeof(int32_t) * (size_t)b, 256), bytes = o_cum + align_up(sizeof(int32_t) * ((size_t)b + 1), 256);
    std::vector<char> host(replan ? bytes : 0, 0);
    std::vector<int32_t> cum(replan ? b + 1 : 0);
    if (replan) {
        int64_t c = 0;
        for (int i = 0; i < b; ++i) { cum[i] = (int32_t)c; c += smm_emission_blocks(fb->frames[plan.order[i]], st.em_tpw); }
        cum[b] = (int32_t)c;
        if (c != st.em_blocks) replan = false;                      // (cannot happen: the same videos)
        else {
            std::memcpy(host.data(), plan.order.data(), sizeof(int32_t) * b);
            std::memcpy(host.data() + o_cum, cum.data(), sizeof(int32_t) * ((size_t)b + 1));
        }
    }
    std::lock_guard<std::mutex> lock(g_plans.mu);
    fb->busy = false;
    fb->have = false;
    fb->evals_left -= 1;
    fb->used = std::move(snap);
    if (fb->n_replans == 0) fb->end_before_us = plan.end_current_us;
    fb->end_after_us = plan.end_current_us;
    char *dst = nullptr;
    if (replan && g_plans.bytes + bytes <= SMM_PLAN_MAX_BYTES) dst = plan_alloc(bytes, e->device);
    if (dst && smm_upload_meta(dst, host.data(), bytes, stream) == (int)hipSuccess && hipEventRecord(e->ready, stream) == hipSuccess) {
        g_plans.bytes += align_up(bytes, 256);
        e->st.order = reinterpret_cast<int32_t *>(dst);
        e->st.em_cum = reinterpret_cast<int32_t *>(dst + o_cum);
        e->st.em_cum_host = cum;
        e->st.n_split = plan.n1;
        e->stream = stream;                                          // (another stream waits for `ready` before it uses the new region)
        e->settled = false;
        fb->order = plan.order;
        fb->n_replans += 1;
        fb->end_after_us = plan.end_chosen_us;
        if (force || fb->n_replans >= SMM_FEEDBACK_MAX_REPLANS) fb->evals_left = 0;
    } else {
        if (dst) (void)hipGetLastError();
        fb->evals_left = 0;                                          // nothing to gain (or no room): the plan is final, nothing more is measured
    }
    feedback_info_set(fb, e->st.n_split);
}
}  // namespace

extern "C" int smm_plan_feedback_info(smm_plan_feedback_info_t *out)
{
    if (!out) return SMM_ERR_ARG;
    std::lock_guard<std::mutex> lock(g_plans.mu);
    *out = g_fb_info.generation == g_plans.generation ? g_fb_info.info : smm_plan_feedback_info_t{};
    return SMM_OK;
}

// The planner alone (smm_plan_feedback.h), for the host tests: no device needed.
extern "C" int smm_plan_feedback_plan(int b, int n_cu, double em_us, const double *dur_us, const int32_t *frames,
                                      const int32_t *cur_order, int cur_n1, int force, int32_t *order_out, int32_t *n1_out,
                                      double *end_current_us, double *end_chosen_us)
{
    if (b < 1 || n_cu < 1 || !dur_us || !frames || !cur_order || cur_n1 < 0 || cur_n1 > b) return SMM_ERR_ARG;
    std::vector<char> seen(b, 0);
    for (int i = 0; i < b; ++i) {
        if (cur_order[i] < 0 || cur_order[i] >= b || seen[cur_order[i]]) return SMM_ERR_ARG;
        seen[cur_order[i]] = 1;
    }
    const SmmFeedbackPlan p = smm_feedback_plan(dur_us, frames, cur_order, b, cur_n1, n_cu, em_us, force != 0);
    if (order_out) std::memcpy(order_out, p.order.data(), sizeof(int32_t) * b);
    if (n1_out) *n1_out = p.n1;
    if (end_current_us) *end_current_us = p.end_current_us;
    if (end_chosen_us) *end_chosen_us = p.end_chosen_us;
    return p.changed ? 1 : 0;
}

// Time-split plan of a Viterbi launch (smm_chunk.hip).  A launch lasts as long as its longest video -- one serial chain -- while
// its CU-time may be a fraction of that: videos longer than P positions are cut into units of about P positions each (unit
// 0: the video's first P'; the others: OV = warm-up + kp - 1 positions in front of an own part of L' = P' - OV), P from the
// launch's CU-time (SMM_CHUNK_P overrides).  An own part is at least kp - 1 positions (the window a unit is certified on
// must lie inside the previous unit's own part) and at least SMM_CHUNK_LMIN; the units' histories live in the video's own
// history block (8 c_max (T + 1) doubles: a unit needs 3 C (T_u + 1)).
struct ChunkPlan {
    std::vector<SmmVideo> units;
    std::vector<SmmChunkVideo> cvs;
};

static void plan_chunks_lmin(const smm_shape *s, const SmmVideo *hv, const int32_t *n_states, int kp_max, bool band, ChunkPlan &out, int n_cu_given, int lmin_cfg)
{
    const SmmEnv &ev = env();
    if (!ev.chunk || (s->flags & (SMM_SHAPE_NO_EOS | SMM_SHAPE_NO_TIME_SPLIT)) || kp_max <= 64) return;      // (kp <= 64: the window back-trace's launches are left alone)
    const int n_cu = n_cu_given > 0 ? n_cu_given : device_cus();
    if (n_cu <= 0) return;
    auto ns = [&](int c) { return dp_frame_ns(band, c); };
    double t_cu = 0.0, t_long = 0.0;
    for (int i = 0; i < s->b; ++i) {
        const double t = (double)hv[i].T * ns(n_states[hv[i].group]);
        t_cu += t;
        t_long = std::max(t_long, t);
    }
    // the launch's CU-time: the DP's share per CU + what the emission pass in front of it (or beside it) takes of the chip
    t_cu = t_cu / n_cu + (s->d > 0 ? (double)s->total_frames * (4.0 * s->d + 8.0 * s->c_max) / 4.0e3 : 0.0);
    // Only a launch that is bound by its longest video is split.  Measured on cfg3 (360 videos, CU-time 2.3 ms against 2.3 ms
    // for its longest video; profiles/round5_time_split.txt): cutting its 46 longest videos shortens the critical launch from
    // 2.3 to 1.5 ms and the step not at all -- the other 314 videos keep 256 CUs busy for 2.1 ms either way -- while every
    // video that has to be repaired (2..4 per launch there: runs of one class decoded as two spans, whose (a, b) / (b, a) orders
    // tie to within rounding) costs a whole one-piece decode on top.  One long video on an idle GPU (cfg1) is the other end:
    // 1.70 -> 0.92 ms.  SMM_CHUNK_P forces the split (tests).
    if (ev.chunk_p <= 0 && t_long < 1.5 * t_cu) return;
    const size_t units_cap = chunk_units_max(s);
    for (int i = 0; i < s->b; ++i) {
        const int T = hv[i].T, C = n_states[hv[i].group], kpv = hv[i].kp;
        // warm-up: the recursion forgets its start behind the next segment boundary, and a segment is shorter than kp
        const int ov = std::max(std::min(ev.chunk_wc, kpv), 16) + kpv - 1;
        const int lmin = std::max(kpv - 1, std::min(lmin_cfg, 2 * kpv));
        const int pmin = ov + lmin;
        // positions per unit: what the launch's CU-time lasts on this video's state count (+ 10 %), at least pmin
        int P = ev.chunk_p > 0 ? ev.chunk_p : (int)(1.1 * t_cu / ns(C));
        P = std::max(P, pmin);
        if ((double)T < 1.05 * P || T < pmin + lmin) continue;                   // (not worth a second unit)
        int n_rest = (T - P + (P - ov) - 1) / (P - ov);
        int Pq = 0;
        for (; n_rest >= 1; --n_rest) {                                          // equal shares: P' + n_rest (P' - OV) = T
            Pq = (int)(((int64_t)T + (int64_t)n_rest * ov + n_rest) / (n_rest + 1));
            if (Pq - ov >= lmin) break;
        }
        if (n_rest < 1 || n_rest + 1 > SMM_CHUNK_MAX_UNITS) continue;
        const int L = Pq - ov;
        // unit j >= 1: own part (r_j, e_j], r_j = Pq + (j - 1) L, first position a_j = r_j - OV; the last one ends at T
        size_t need = (size_t)3 * C * ((size_t)Pq + 1);
        for (int j = 1; j <= n_rest; ++j) {
            const int r = Pq + (j - 1) * L, e = (j == n_rest) ? T : r + L;
            need += (size_t)3 * C * ((size_t)(e - (r - ov)) + 1);
        }
        if (need > (size_t)8 * s->c_max * ((size_t)T + 1) || Pq + (n_rest - 1) * L >= T) continue;
        if (out.units.size() + n_rest + 1 > units_cap) break;
        SmmChunkVideo cv{i, (int32_t)out.units.size(), n_rest + 1, ov};           // (first_unit: made absolute by the caller)
        size_t hoff = (size_t)hv[i].hist_off;
        for (int j = 0; j <= n_rest; ++j) {
            const int r = j ? Pq + (j - 1) * L : 0, a0 = j ? r - ov : 0, e = (j == n_rest) ? T : Pq + j * L;
            SmmVideo u = hv[i];
            u.frame_off = hv[i].frame_off + a0;
            u.hist_off = (int64_t)hoff;
            u.T = e - a0;
            u.pad = 1 | (j ? 2 : 0) | (a0 << 2);
            hoff += (size_t)3 * C * ((size_t)u.T + 1);
            out.units.push_back(u);
        }
        out.cvs.push_back(cv);
    }
}

// The least own part of a unit: SMM_CHUNK_LMIN, or the finer SMM_CHUNK_LMIN_FINE where the launch then still runs in ONE round of
// workgroups (units + unsplit videos <= CUs).  cfg2 (64 videos x 2048 frames, K = 256): four units per video on 256 CUs instead of
// three on 192, 0.378 -> 0.369 ms per step, two alternating runs on one box; five or six units per video (320 / 384 workgroups, a
// second round): 0.49-0.50 ms.  SMM_CHUNK_LMIN (environment) overrides both.
static void plan_chunks(const smm_shape *s, const SmmVideo *hv, const int32_t *n_states, int kp_max, bool band, ChunkPlan &out, int n_cu_given = 0)
{
    const SmmEnv &ev = env();
    if (ev.chunk_lmin > 0) { plan_chunks_lmin(s, hv, n_states, kp_max, band, out, n_cu_given, std::max(ev.chunk_lmin, 130)); return; }
    const int n_cu = n_cu_given > 0 ? n_cu_given : device_cus();
    ChunkPlan fine;
    plan_chunks_lmin(s, hv, n_states, kp_max, band, fine, n_cu_given, SMM_CHUNK_LMIN_FINE);
    if (!fine.cvs.empty() && (int)fine.units.size() + (s->b - (int)fine.cvs.size()) <= n_cu) { out = std::move(fine); return; }
    plan_chunks_lmin(s, hv, n_states, kp_max, band, out, n_cu_given, SMM_CHUNK_LMIN);
}

static int stage_uncached(const smm_shape *s, const int64_t *lengths, const int64_t *frame_off, const int32_t *group,
                          const int32_t *kp, const int32_t *n_states, void *ws, size_t ws_bytes, hipStream_t stream, Staged *out,
                          bool for_viterbi, int cum_chunk, bool want_split, const std::function<char *(size_t)> *meta_alloc,
                          SmmPlan *plan_out)
{
    if (!shape_ok(s) || !lengths || !frame_off || !n_states || !ws) return SMM_ERR_ARG;
    if (!limits_ok(s)) return SMM_ERR_UNSUPPORTED;
    int c_need = 0;
    for (int g = 0; g < s->n_groups; ++g) {
        if (n_states[g] < 1 || n_states[g] > s->c_max) return SMM_ERR_ARG;
        c_need = std::max(c_need, n_states[g]);
    }
    const bool no_eos = (s->flags & SMM_SHAPE_NO_EOS) != 0;
    for (int i = 0; i < s->b; ++i)
        if (lengths[i] < (no_eos ? 2 : 1) || lengths[i] > s->t_max) return SMM_ERR_ARG;
    const SmmPlan p = make_plan(s, lengths);
    if (ws_bytes < p.total) return SMM_ERR_WORKSPACE;

    std::vector<char> host(p.meta_bytes, 0);
    SmmVideo *hv = reinterpret_cast<SmmVideo *>(host.data());
    int32_t *ho = reinterpret_cast<int32_t *>(host.data() + p.o_order);
    int32_t *hn = reinterpret_cast<int32_t *>(host.data() + p.o_nstates);

    size_t hoff = 0;
    int kp_max = 2;
    for (int i = 0; i < s->b; ++i) {
        const int64_t t = lengths[i];
        if (frame_off[i] < 0 || frame_off[i] + t > s->total_frames) return SMM_ERR_ARG;
        const int g = group ? group[i] : 0;
        if (g < 0 || g >= s->n_groups) return SMM_ERR_ARG;
        const int k = kp ? kp[i] : std::min<int>(s->k_rows, s->t_max);
        if (k < 1 || k > s->k_rows) return SMM_ERR_ARG;
        hv[i].frame_off = frame_off[i];
        hv[i].hist_off = (int64_t)hoff;
        hv[i].T = (int32_t)t;                      // (no EOS: the DP kernels take T - 1, the emission kernel every frame)
        hv[i].group = g;
        hv[i].kp = k;
        hv[i].pad = 0;
        hoff += 8 * (size_t)s->c_max * (size_t)(t + 1);
        kp_max = std::max(kp_max, k);
    }
    std::iota(ho, ho + s->b, 0);
    out->band_mode = band_mode(kp_max, c_need);
    // most work first -- by modelled time, T x ns per frame at the video's state count -- so the tail of the grid is made of short videos
    const bool band = out->band_mode;
    std::stable_sort(ho, ho + s->b, [&](int a, int b) {
        return hv[a].T * dp_frame_ns(band, n_states[hv[a].group]) > hv[b].T * dp_frame_ns(band, n_states[hv[b].group]);
    });
    // (chunk table for the emission chain rule: by group, so that a workgroup's run of chunks rarely changes group)
    if (cum_chunk > 0) std::stable_sort(ho, ho + s->b, [&](int a, int b) { return hv[a].group < hv[b].group; });
    std::memcpy(hn, n_states, sizeof(int32_t) * s->n_groups);
    // time-split plan (Viterbi launches only): the split videos come FIRST in `order` -- with a stream split they are its
    // first part (their emission, the prefix sums at their units' starts and their units' DP on the caller's stream, the
    // rest beside them)
    ChunkPlan cp;
    if (for_viterbi && cum_chunk == 0) plan_chunks(s, hv, n_states, kp_max, out->band_mode, cp);
    const int n_cv = (int)cp.cvs.size(), n_un = (int)cp.units.size();
    out->n_cv = n_cv;
    out->n_units = s->b - n_cv + n_un;
    out->u_part1 = n_un;
    out->n_split = 0;
    if (n_cv > 0) {
        std::vector<char> is_cv(s->b, 0);
        for (const SmmChunkVideo &cv : cp.cvs) is_cv[cv.vid] = 1;
        std::stable_partition(ho, ho + s->b, [&](int32_t v) { return is_cv[v] != 0; });
        // the stream split of a decode: the split videos are its critical part, if there is enough beside them to be worth a second stream
        const SmmEnv &ev = env();
        const double em_us = (double)s->total_frames * (4.0 * s->d + 8.0 * s->c_max) / 4.0e6;
        if (want_split && !ev.no_split && s->b - n_cv >= 16 && em_us >= ev.split_min_us) out->n_split = n_cv;
    } else {
        out->n_split = want_split ? choose_split(hv, ho, s->b, s->d, s->c_max, s->total_frames) : 0;
    }
    // SMALL workgroups: the last part of the launch -- the rest of a stream split, or everything that is not a unit of a
    // time-split video -- when it is bound by CU-time through and through: at least three videos per CU (cfg3's rest, 340 videos
    // on 256 CUs, lost 15 % to them: its <= 16-state videos of up to 11 800 frames run 25..60 % longer in four waves and became
    // the part's critical path; cfg5's 2754 videos gained 11 %), and only videos that stay well inside the part's CU-time at the
    // four-wave speed.  Those go to the part's END (work order kept on both sides).
    out->small_first = out->small_count = 0;
    if (for_viterbi && cum_chunk == 0 && out->band_mode && env().small_wg && !(s->flags & SMM_SHAPE_NO_EOS)) {
        const bool force = env().small_wg >= 2;
        const int n_cu = device_cus();
        const int t0 = out->n_split > 0 ? out->n_split : n_cv;              // first video of the last part, in `order`
        const int n_tail = s->b - t0;
        if (n_cu > 0 && (force || n_tail >= 3 * n_cu)) {
            double t_cu = 0.0;                                              // the part's CU-time at the eight-wave speed, ns
            for (int i = t0; i < s->b; ++i) t_cu += (double)hv[ho[i]].T * smm_band_frame_ns(n_states[hv[ho[i]].group]);
            t_cu /= n_cu;
            auto small = [&](int32_t v) {
                return n_states[hv[v].group] <= 16 && (force || (double)hv[v].T * 1.6 * smm_band_frame_ns(n_states[hv[v].group]) <= 0.5 * t_cu);
            };
            const int n_small = (int)std::count_if(ho + t0, ho + s->b, small);
            if (n_small >= (force ? 1 : 64)) {
                std::stable_partition(ho + t0, ho + s->b, [&](int32_t v) { return !small(v); });
                out->small_count = n_small;
            }
        }
    }
    {
        // emission grid (flat): video order[i] gets smm_emission_blocks(T) workgroups; in the DP's final order
        int32_t *hc = reinterpret_cast<int32_t *>(host.data() + p.o_emcum);
        out->em_tpw = smm_emission_tiles_per_wave(s->total_frames, s->b);
        int64_t cum = 0;
        for (int i = 0; i < s->b; ++i) {
            hc[i] = (int32_t)cum;
            // (cum_chunk: the table counts chunks of that many frames instead -- smm_emission_bwd_f64)
            cum += cum_chunk > 0 ? (hv[ho[i]].T + cum_chunk - 1) / cum_chunk : smm_emission_blocks(hv[ho[i]].T, out->em_tpw);
        }
        if (cum > 0x7fffffff) return SMM_ERR_UNSUPPORTED;
        hc[s->b] = (int32_t)cum;
        out->em_blocks = (int)cum;
        if (out->n_split > 0) out->em_cum_host.assign(hc, hc + s->b + 1);
        if (out->n_split > 0 && meta_alloc) {
            out->order_host.assign(ho, ho + s->b);
            out->frames_host.resize(s->b);
            for (int i = 0; i < s->b; ++i) out->frames_host[i] = hv[i].T;
        }
    }
    // the units' metadata: [videos | units], the DP launch's order over [units (most work first) | unsplit videos (as in `order`)],
    // the split videos' table and -- for the repair launch -- their list
    std::vector<char> ext;
    size_t x_order = 0, x_cvs = 0, x_porder = 0;
    if (n_cv > 0) {
        x_order = align_up(sizeof(SmmVideo) * ((size_t)s->b + n_un), 256);
        x_cvs = x_order + align_up(sizeof(int32_t) * ((size_t)s->b + n_un), 256);
        x_porder = x_cvs + align_up(sizeof(SmmChunkVideo) * n_cv, 256);
        ext.assign(x_porder + align_up(sizeof(int32_t) * n_cv, 256), 0);
        SmmVideo *xv = reinterpret_cast<SmmVideo *>(ext.data());
        int32_t *xo = reinterpret_cast<int32_t *>(ext.data() + x_order);
        SmmChunkVideo *xc = reinterpret_cast<SmmChunkVideo *>(ext.data() + x_cvs);
        int32_t *xp = reinterpret_cast<int32_t *>(ext.data() + x_porder);
        std::memcpy(xv, hv, sizeof(SmmVideo) * s->b);
        std::memcpy(xv + s->b, cp.units.data(), sizeof(SmmVideo) * n_un);
        for (int i = 0; i < n_un; ++i) xo[i] = s->b + i;
        std::stable_sort(xo, xo + n_un, [&](int a, int b) {
            return xv[a].T * dp_frame_ns(band, n_states[xv[a].group]) > xv[b].T * dp_frame_ns(band, n_states[xv[b].group]);
        });
        for (int i = n_cv; i < s->b; ++i) xo[n_un + i - n_cv] = ho[i];
        for (int i = 0; i < n_cv; ++i) {
            xc[i] = cp.cvs[i];
            xc[i].first_unit += s->b;
            xp[i] = cp.cvs[i].vid;
        }
    }

    // (in the DP launch's order -- `order`, or with time-split videos [units | unsplit videos in `order`'s order] -- the small videos
    // are the last small_count entries)
    if (out->small_count > 0) out->small_first = out->n_units - out->small_count;

    char *base = static_cast<char *>(ws);
    // videos | order | n_states travel as kernel arguments (no pageable copy: the host never waits for the stream) -- into
    // the workspace, or into the resident plan's own buffer; the error words behind them (always in the workspace) start at zero
    const size_t o_ext = align_up(p.o_err, 256);
    char *meta_dst = meta_alloc ? (*meta_alloc)(o_ext + ext.size()) : nullptr;
    char *meta = meta_dst ? meta_dst : base;
    SMM_HIP((hipError_t)smm_upload_meta(meta, host.data(), p.o_err, stream));
    SMM_HIP((hipError_t)smm_zero_async(base + p.o_err, p.meta_bytes - p.o_err, stream));
    out->videos = reinterpret_cast<SmmVideo *>(meta);
    out->order = reinterpret_cast<int32_t *>(meta + p.o_order);
    out->n_states = reinterpret_cast<int32_t *>(meta + p.o_nstates);
    out->em_cum = reinterpret_cast<int32_t *>(meta + p.o_emcum);
    plan_point(p, ws, out);
    out->uvideos = nullptr; out->uorder = nullptr; out->porder = nullptr; out->cvs = nullptr;
    if (n_cv > 0) {
        // (workspace: behind the redo words and the anchors of the chunk region, whose size bounds every plan of this shape)
        char *xdst = meta_dst ? meta_dst + o_ext
                              : base + p.o_chunk + align_up(sizeof(int32_t) * s->b, 256) + align_up(sizeof(double) * chunk_units_max(s) * s->c_max, 256);
        SMM_HIP((hipError_t)smm_upload_meta(xdst, ext.data(), ext.size(), stream));
        out->uvideos = reinterpret_cast<SmmVideo *>(xdst);
        out->uorder = reinterpret_cast<int32_t *>(xdst + x_order);
        out->cvs = reinterpret_cast<SmmChunkVideo *>(xdst + x_cvs);
        out->porder = reinterpret_cast<int32_t *>(xdst + x_porder);
    }
    out->kp_max = kp_max;
    out->c_need = c_need;
    if (plan_out) *plan_out = p;
    return SMM_OK;
}

// The time-split plan of a Viterbi launch as the library would make it on a GPU of n_cu compute units (include/smmdp.h): host
// logic only, no device needed -- what the CPU tests look at.
extern "C" int smm_time_split_plan(const smm_shape *s, const int64_t *lengths, const int32_t *group, const int32_t *kp,
                                   const int32_t *n_states, int n_cu, int32_t *unit_video, int32_t *unit_first, int32_t *unit_len,
                                   int32_t *unit_overlap, int cap)
{
    if (!shape_ok(s) || !lengths || !n_states || n_cu < 1) return SMM_ERR_ARG;
    std::vector<SmmVideo> hv(s->b);
    size_t hoff = 0;
    int kp_max = 2, c_need = 0;
    for (int g = 0; g < s->n_groups; ++g) c_need = std::max(c_need, n_states[g]);
    for (int i = 0; i < s->b; ++i) {
        const int g = group ? group[i] : 0;
        if (g < 0 || g >= s->n_groups || lengths[i] < 1) return SMM_ERR_ARG;
        hv[i] = SmmVideo{0, (int64_t)hoff, (int32_t)lengths[i], g, kp ? kp[i] : std::min<int>(s->k_rows, s->t_max), 0};
        hoff += 8 * (size_t)s->c_max * (size_t)(lengths[i] + 1);
        kp_max = std::max(kp_max, hv[i].kp);
    }
    ChunkPlan cp;
    plan_chunks(s, hv.data(), n_states, kp_max, band_mode(kp_max, c_need), cp, n_cu);
    int n = 0;
    for (const SmmChunkVideo &cv : cp.cvs)
        for (int j = 0; j < cv.n_chunks; ++j, ++n) {
            if (n >= cap) continue;
            const SmmVideo &u = cp.units[cv.first_unit + j];
            if (unit_video) unit_video[n] = cv.vid;
            if (unit_first) unit_first[n] = u.pad >> 2;
            if (unit_len) unit_len[n] = u.T;
            if (unit_overlap) unit_overlap[n] = j ? cv.ov : 0;
        }
    return n;
}

// Viterbi at K > 512: BAND mode (smm_viterbi.hip), up to SMM_MAX_STATES states on one CU; also 29..32 states at K > 256
// (the 512-slot rings of five states per pusher wave do not fit the registers)
static bool band_mode(int kp_max, int c_need)
{
    return kp_max > 512 || (kp_max > 256 && c_need > 28);
}

static int ring_regs(int kp_max)
{
    int r = 1;
    while (64 * r < kp_max) r *= 2;
    return r;
}

// ------------------------------------------------------------------------------------------------ pieces
// One side's tables as an entry point was given them (host only: the kernels' argument structs are in smm_launch.h)
struct Tables {
    const double *elp, *trans, *init, *len, *endpen, *logz;
};

// what every DP launch is told: the staged videos, the tables, history and error words, the sizes, and add_eos=False
static SmmDpArgs dp_args(const smm_shape *s, const Staged &st, const Tables &t)
{
    SmmDpArgs a{};
    a.videos = st.videos; a.order = st.order; a.n_states = st.n_states;
    a.elp = t.elp; a.trans = t.trans; a.init = t.init; a.len = t.len; a.endpen = t.endpen;
    a.hist = st.hist; a.err = st.err;
    a.c_max = s->c_max; a.k_rows = s->k_rows; a.t_max = s->t_max; a.b = s->b;
    if (s->flags & SMM_SHAPE_NO_EOS) { a.flags |= 8; a.endpen = nullptr; }
    return a;
}

// what the posterior launches repeat (smm_launch.h): the head from the shape and the staged videos ...
static SmmPostHead post_head(const smm_shape *s, const Staged &st)
{
    return {st.videos, st.n_states, st.err, s->c_max, s->k_rows, s->b, (s->flags & SMM_SHAPE_NO_EOS) ? 1 : 0};
}
// ... and one side from the workspace its histories are in and its tables: endpen is null without EOS
static SmmPostSide post_side(int no_eos, const double *hist, const Tables &t)
{
    return {hist, t.elp, t.trans, t.init, t.len, no_eos ? nullptr : t.endpen, t.logz};
}

// The `tabs` area of a plan as the time-reversed recursion uses it
struct ReversedTabs {
    double *trans_t;       // [g][cm][cm] transposed
    double *logz_b;        // [b] log Z as closed by the backward recursion (consistency value)
};
static ReversedTabs reversed_tabs(const smm_shape *s, double *tabs)
{
    return {tabs, tabs + (size_t)s->n_groups * s->c_max * s->c_max};
}

// The time-reversed recursion of one side into `hist` (backward messages in the second history half): transposed transitions
// and closing values in `tabs`.  With SMM_SHAPE_LOGZ_BOTH smm_logz_f64 already ran it, in the forward run's launch.
static int run_reversed(const smm_shape *shape, const Staged &st, double *hist, double *tabs, const Tables &t, hipStream_t hs)
{
    if (shape->flags & SMM_SHAPE_LOGZ_BOTH) return SMM_OK;
    const ReversedTabs rt = reversed_tabs(shape, tabs);
    smm_launch_transpose(t.trans, rt.trans_t, shape->n_groups, shape->c_max, hs);
    SmmDpArgs a = dp_args(shape, st, t);
    a.trans = rt.trans_t;
    a.hist = hist;
    a.flags |= 2;                                  // time-reversed run
    return smm_launch_logz(a, rt.logz_b, ring_regs(st.kp_max), st.c_need, hs);
}

// What the calls that read both directions of p's lattice open with: the launch staged into the workspace, then p's
// time-reversed histories.  `held`: a refusal that ranks behind staging's own.
static int stage_both(const smm_shape *shape, const int64_t *lengths, const int64_t *frame_off, const int32_t *group,
                      const int32_t *kp, const int32_t *n_states, void *ws, size_t ws_bytes, const Tables &p, hipStream_t hs,
                      Staged *st, int held = SMM_OK)
{
    const int rc = stage(shape, lengths, frame_off, group, kp, n_states, ws, ws_bytes, hs, st);
    if (rc != SMM_OK) return rc;
    if (held != SMM_OK) return held;
    return run_reversed(shape, *st, st->hist, st->tabs, p, hs);
}

// a caller's buffer against the size its query returns: 0 is the query's refusal of the shape
static int room_ok(size_t need, size_t have) { return need == 0 ? SMM_ERR_ARG : have < need ? SMM_ERR_WORKSPACE : SMM_OK; }

static int run_emission(const smm_shape *s, const Staged &st, const float *x, const double *w, const double *cst,
                        const double *inv_var, const float *cons, double *elp64, float *elp32, hipStream_t stream,
                        int first = 0, int count = -1)
{
    if (!x || !w || !cst || !inv_var || s->d < 1 || (!elp64 && !elp32)) return SMM_ERR_ARG;
    if (smm_emission_lds_bytes(s->d, st.c_need) > 160 * 1024)
        return SMM_ERR_UNSUPPORTED;   // the group's weight table must fit the CU's LDS (D <= 544 at 32 states)
    SmmEmArgs a{st.videos, st.order, st.n_states, x, w, cst, inv_var, cons, elp64, elp32, s->d, s->c_max, s->b};
    if (count < 0) smm_launch_emission(a, st.c_need, st.em_tpw, st.em_blocks, st.em_cum, s->total_frames, stream);
    else smm_launch_emission(a, st.c_need, st.em_tpw, st.em_cum_host[first + count] - st.em_cum_host[first], st.em_cum,
                             s->total_frames, stream, st.em_cum_host[first], first, count);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// first / count: only the videos order[first .. first + count) (count < 0: all); prep: launch the band tables kernel (a
// split decode launches it once, in front of both parts)
// smm_dp_timing_*: event pairs around the DP kernel launches (measurement aid, smmdp.h)
namespace {
struct DpTiming {
    std::mutex mu;
    bool on = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> rec, pool;
    std::vector<int> tag;          // per record: 0 the only DP launch of its call, 1 the critical videos of a split decode
                                   // (caller's stream), 2 the rest of a split decode (second stream)
} g_dp_timing;

bool dp_timing_begin(hipStream_t stream, std::pair<hipEvent_t, hipEvent_t> &ev)
{
    std::lock_guard<std::mutex> lock(g_dp_timing.mu);
    if (!g_dp_timing.on) return false;
    if (!g_dp_timing.pool.empty()) { ev = g_dp_timing.pool.back(); g_dp_timing.pool.pop_back(); }
    else if (hipEventCreate(&ev.first) != hipSuccess || hipEventCreate(&ev.second) != hipSuccess) return false;
    return hipEventRecord(ev.first, stream) == hipSuccess;
}

void dp_timing_end(hipStream_t stream, const std::pair<hipEvent_t, hipEvent_t> &ev, int tag)
{
    (void)hipEventRecord(ev.second, stream);
    std::lock_guard<std::mutex> lock(g_dp_timing.mu);
    g_dp_timing.rec.push_back(ev);
    g_dp_timing.tag.push_back(tag);
}
}  // namespace

extern "C" void smm_dp_timing_enable(int on)
{
    std::lock_guard<std::mutex> lock(g_dp_timing.mu);
    g_dp_timing.on = on != 0;
}

extern "C" int smm_dp_timing_read_tagged(float *ms, int32_t *tags, int cap)
{
    std::vector<std::pair<hipEvent_t, hipEvent_t>> rec;
    std::vector<int> tag;
    {
        std::lock_guard<std::mutex> lock(g_dp_timing.mu);
        rec.swap(g_dp_timing.rec);
        tag.swap(g_dp_timing.tag);
    }
    int n = 0;
    for (auto &ev : rec) {
        float t = 0.f;
        if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&t, ev.first, ev.second) == hipSuccess && n < cap) {
            if (ms) ms[n] = t;
            if (tags) tags[n] = tag[n];
        }
        ++n;
    }
    std::lock_guard<std::mutex> lock(g_dp_timing.mu);
    for (auto &ev : rec) g_dp_timing.pool.push_back(ev);
    return n;
}

extern "C" int smm_dp_timing_read(float *ms, int cap) { return smm_dp_timing_read_tagged(ms, nullptr, cap); }

namespace {
// (defined with the split decode below) per device: second streams and pooled event pairs
hipStream_t aux_stream_n(int dev, int which);
bool aux_events_get(int dev, std::pair<hipEvent_t, hipEvent_t> &ev);
void aux_events_put(int dev, const std::pair<hipEvent_t, hipEvent_t> &ev);
}  // namespace

static int run_viterbi(const smm_shape *s, const Staged &st, const double *elp, const double *trans, const double *init,
                       const double *len_scores, const double *endpen, const int64_t *class_map, int64_t *spans,
                       int64_t *labels, double *best, int32_t *n_segs, hipStream_t stream, int first = 0, int count = -1,
                       bool prep = true, bool launch = true, int timing_tag = 0)
{
    if (!elp || !trans || !init || !len_scores) return SMM_ERR_ARG;
    SmmDpArgs a = dp_args(s, st, Tables{elp, trans, init, len_scores, endpen, nullptr});
    a.class_map = class_map;
    a.spans = spans; a.labels = labels; a.best = best; a.n_segs = n_segs;
    a.stamps = st.stamps;
    if (count >= 0) { a.order = st.order + first; a.b = count; }
    // time-split videos (smm_chunk.hip): the launch runs over UNITS -- [the split videos' units | the unsplit videos]; a stream
    // split's first part is exactly the units
    const bool with_units = st.n_cv > 0 && (count < 0 || first == 0);
    if (st.n_cv > 0) {
        a.videos = st.uvideos;
        a.b_videos = s->b;
        a.chunk_anchor = st.anchors;
        if (count < 0) { a.order = st.uorder; a.b = st.n_units; }
        else if (first == 0) { a.order = st.uorder; a.b = st.u_part1; }
        else { a.order = st.uorder + st.u_part1; a.b = st.n_units - st.u_part1; }
    }
#ifdef SMM_DEV
    a.flags |= env().debug_flags;                             // (SmmDpArgs::flags bit 0: profiling, outputs undefined)
#endif
    if (!env().spec) a.flags |= 256;                          // A/B aid: no speculative transition
    if (st.band_mode) {
        double *len_t = st.band, *band_tab = st.band + (size_t)s->n_groups * s->c_max * SMM_BAND_ROW;
        double *dmin_t = band_tab + (size_t)s->n_groups * s->c_max * SMM_BAND_TAB;
        if (prep) smm_launch_band_tables(len_scores, st.n_states, len_t, band_tab, dmin_t, s->n_groups, s->c_max, s->k_rows, stream);
        a.len_t = len_t;
        a.band_tab = band_tab;
        a.dmin_t = dmin_t;
        a.flags |= 128;
    }
    if (ring_regs(st.kp_max) == 1 && !env().no_bt_window) {
        // short segments: window back-trace (smm_viterbi.hip); W >= 2 kp keeps a window good for many segments
        // about 48 KB of window (three workgroups per CU stay possible), at least 2 kp positions, at most 512
        int w = (int)(48 * 1024 / (24 * (size_t)st.c_need)) & ~7;
        w = std::min(512, std::max(w, (2 * st.kp_max + 7) & ~7));
        const size_t bytes = sizeof(double) * ((size_t)3 * w + st.c_need + st.kp_max) * st.c_need;
        if (bytes <= 126 * 1024) { a.bt_window = w; a.bt_dyn_bytes = (int32_t)bytes; }
    }
    if (!launch) { SMM_HIP(hipGetLastError()); return SMM_OK; }      // (prep only)
    if (with_units) smm_launch_cum_anchors(a, st.cvs, st.n_cv, st.anchors, stream);   // cumE at the units' first positions, serially
    // SMALL workgroups (smm_viterbi.hip: smm_launch_viterbi_small): when this range of the launch order ends with the part's
    // <= 16-state videos (stage_uncached put them there), those run in four-wave workgroups, two per CU, on a side stream
    // BESIDE the eight-wave launch of the others -- forked behind everything this stream has queued so far (band tables,
    // this part's emission) and joined before the call goes on.  Not under stream capture (the side stream is shared).
    const int lo = (int)(a.order - (st.n_cv > 0 ? st.uorder : st.order));
    int n_small = (st.small_count > 0 && lo <= st.small_first && lo + a.b == st.small_first + st.small_count) ? st.small_count : 0;
    hipStream_t side = nullptr;
    std::pair<hipEvent_t, hipEvent_t> fj{nullptr, nullptr};
    int dev = 0;
    if (n_small > 0) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64 && hipStreamIsCapturing(stream, &cap) == hipSuccess &&
            cap == hipStreamCaptureStatusNone)
            side = aux_stream_n(dev, 1);
        if (side && !aux_events_get(dev, fj)) side = nullptr;
        if (!side) n_small = 0;
    }
    int rc_small = SMM_OK;
    if (n_small > 0) {
        SmmDpArgs as = a;
        as.order = a.order + (a.b - n_small);
        as.b = n_small;
        a.b -= n_small;
        if (hipEventRecord(fj.first, stream) != hipSuccess || hipStreamWaitEvent(side, fj.first, 0) != hipSuccess) rc_small = SMM_ERR_HIP;
        if (rc_small == SMM_OK) {
            std::pair<hipEvent_t, hipEvent_t> tev2;
            const bool timed2 = dp_timing_begin(side, tev2);
            rc_small = smm_launch_viterbi_small(as, side);
            if (timed2) dp_timing_end(side, tev2, 3);
        }
    }
    std::pair<hipEvent_t, hipEvent_t> tev;
    int rc = SMM_OK;
    if (a.b > 0) {
        const bool timed = dp_timing_begin(stream, tev);
        rc = smm_launch_viterbi(a, st.band_mode ? 16 : ring_regs(st.kp_max), st.c_need, stream);
        if (timed) dp_timing_end(stream, tev, timing_tag);
    }
    if (side) {
        // the join is made even after an error on the way, so that this stream never runs ahead of the side stream
        if (hipEventRecord(fj.second, side) != hipSuccess || hipStreamWaitEvent(stream, fj.second, 0) != hipSuccess) rc_small = SMM_ERR_HIP;
        aux_events_put(dev, fj);
    }
    if (rc != SMM_OK) return rc;
    if (rc_small != SMM_OK) return rc_small;
    if (with_units) {
        // certify the cuts, walk the path, write the split videos' outputs -- and decode again, in one piece, the ones that
        // could not be certified (one workgroup per split video; all but the flagged ones return at once)
        smm_launch_chunk_stitch(a, st.cvs, st.n_cv, st.redo, stream);
        SmmDpArgs ar = a;
        ar.order = st.porder;
        ar.b = st.n_cv;
        ar.redo = st.redo;
        // (BAND mode: the launch's own kernel under its second name, so that per-kernel statistics of the DP launch are not
        // diluted by a launch that nearly always returns at once; the ring kernels repair with themselves)
        const int rc2 = st.band_mode ? smm_launch_viterbi_repair(ar, st.c_need, stream)
                                     : smm_launch_viterbi(ar, ring_regs(st.kp_max), st.c_need, stream);
        if (rc2 != SMM_OK) return rc2;
    }
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int smm_emission_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                const int32_t *group_host, const int32_t *n_states_host, const float *x, const double *w,
                                const double *cst, const double *inv_var, const float *cons, double *elp64, float *elp32,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = stage(shape, lengths_host, frame_offset_host, group_host, nullptr, n_states_host, workspace, workspace_bytes,
                   hs, &st);
    if (rc != SMM_OK) return rc;
    return run_emission(shape, st, x, w, cst, inv_var, cons, elp64, elp32, hs);
}

extern "C" int smm_emission_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                    const int32_t *group_host, const int32_t *n_states_host, const float *x,
                                    const double *g_elp, double *g_w, double *g_cst, double *g_inv_var,
                                    void *workspace, size_t workspace_bytes, void *stream)
{
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    if (!x || !g_elp || !g_w || !g_cst || !g_inv_var || !shape || shape->d < 1) return SMM_ERR_ARG;
    int rc = stage(shape, lengths_host, frame_offset_host, group_host, nullptr, n_states_host, workspace, workspace_bytes,
                   hs, &st, false, smm_emission_bwd_chunk());
    if (rc != SMM_OK) return rc;
    const size_t g = shape->n_groups, cm = shape->c_max, d = shape->d;
    {
        void *const zp[3] = {g_w, g_cst, g_inv_var};
        const size_t zb[3] = {sizeof(double) * g * cm * d, sizeof(double) * g * cm, sizeof(double) * d};
        SMM_HIP((hipError_t)smm_zero_multi_async(zp, zb, 3, hs));
    }
    SmmEmBwdArgs a{st.videos, st.order, st.n_states, st.em_cum, x, g_elp, g_w, g_cst, g_inv_var,
                   shape->d, shape->c_max, shape->b, st.em_blocks};
    smm_launch_emission_bwd(a, st.c_need, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_viterbi_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                               const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                               const double *elp, const double *trans, const double *init, const double *len_scores,
                               const double *endpen, const int64_t *class_map, int64_t *spans, int64_t *labels,
                               double *best, int32_t *n_segs, void *workspace, size_t workspace_bytes, void *stream)
{
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = stage(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes,
                   hs, &st, true);
    if (rc != SMM_OK) return rc;
    return run_viterbi(shape, st, elp, trans, init, len_scores, endpen, class_map, spans, labels, best, n_segs, hs);
}

extern "C" int smm_viterbi_f32(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                               const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                               const float *elp, const float *trans, const float *init, const float *len_scores,
                               const float *endpen, const int64_t *class_map, int64_t *spans, int64_t *labels,
                               double *best, int32_t *n_segs, void *workspace, size_t workspace_bytes, void *stream)
{
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = stage(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes,
                   hs, &st, true);
    if (rc != SMM_OK) return rc;
    if (!elp || !trans || !init || !len_scores) return SMM_ERR_ARG;
    const size_t g = shape->n_groups, cm = shape->c_max;
    double *t64 = st.tabs, *i64 = t64 + g * cm * cm, *l64 = i64 + g * cm, *e64 = l64 + g * shape->k_rows * cm;
    smm_launch_widen(trans, t64, g * cm * cm, hs);
    smm_launch_widen(init, i64, g * cm, hs);
    smm_launch_widen(len_scores, l64, g * shape->k_rows * cm, hs);
    if (endpen) smm_launch_widen(endpen, e64, (size_t)shape->b * cm, hs);
    smm_launch_widen(elp, st.elp, (size_t)shape->total_frames * cm, hs);
    SMM_HIP(hipGetLastError());
    return run_viterbi(shape, st, st.elp, t64, i64, l64, endpen ? e64 : nullptr, class_map, spans, labels, best, n_segs, hs);
}

// The second stream of a split decode: one per device, created on first use with the lowest priority (the critical videos'
// DP on the caller's stream goes first); it lives until smm_release_cached_plans().  Every use is bracketed by a pooled
// event pair on the caller's stream, so from the caller's point of view the call is still ordered on ITS stream.  A call
// made under stream capture does NOT split (the one shared second stream would be pulled into the capture and a
// concurrent call from another thread would then enqueue onto a capturing stream): it runs as one launch pair.
namespace {
struct AuxDev {                       // per device: the second stream of a split decode, the side stream of the small workgroups,
    hipStream_t stream = nullptr, stream1 = nullptr;             // and the event pairs that bracket them
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;     // idle (fork, join) pairs
};
std::mutex g_aux_mu;
AuxDev g_aux[64];

hipStream_t aux_stream_n(int dev, int which)
{
    std::lock_guard<std::mutex> lock(g_aux_mu);
    AuxDev &d = g_aux[dev];
    hipStream_t &st = which ? d.stream1 : d.stream;
    if (!st) {
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        if (hipStreamCreateWithPriority(&st, hipStreamNonBlocking, least) != hipSuccess) st = nullptr;
    }
    return st;
}
hipStream_t aux_stream(int dev) { return aux_stream_n(dev, 0); }

bool aux_events_get(int dev, std::pair<hipEvent_t, hipEvent_t> &ev)
{
    {
        std::lock_guard<std::mutex> lock(g_aux_mu);
        AuxDev &d = g_aux[dev];
        if (!d.events.empty()) { ev = d.events.back(); d.events.pop_back(); return true; }
    }
    ev = {nullptr, nullptr};
    if (hipEventCreateWithFlags(&ev.first, hipEventDisableTiming) != hipSuccess) return false;
    if (hipEventCreateWithFlags(&ev.second, hipEventDisableTiming) != hipSuccess) { (void)hipEventDestroy(ev.first); return false; }
    return true;
}

void aux_events_put(int dev, const std::pair<hipEvent_t, hipEvent_t> &ev)
{
    // (an event that is re-recorded while an earlier wait on it is still queued keeps that wait's meaning: a wait
    // captures the record it follows)
    std::lock_guard<std::mutex> lock(g_aux_mu);
    g_aux[dev].events.push_back(ev);
}
}  // namespace

static void release_aux()
{
    std::lock_guard<std::mutex> lock(g_aux_mu);
    for (int d = 0; d < 64; ++d) {
        for (auto &ev : g_aux[d].events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
        g_aux[d].events.clear();
        if (g_aux[d].stream) { (void)hipStreamDestroy(g_aux[d].stream); g_aux[d].stream = nullptr; }
        if (g_aux[d].stream1) { (void)hipStreamDestroy(g_aux[d].stream1); g_aux[d].stream1 = nullptr; }
    }
    std::lock_guard<std::mutex> lock2(g_dp_timing.mu);
    for (auto &ev : g_dp_timing.pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    g_dp_timing.pool.clear();
}

extern "C" int smm_decode_f32(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                              const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                              const float *x, const double *w, const double *cst, const double *inv_var, const float *cons,
                              const double *trans, const double *init, const double *len_scores, const double *endpen,
                              const int64_t *class_map, int64_t *spans, int64_t *labels, double *best, int32_t *n_segs,
                              float *elp32, void *workspace, size_t workspace_bytes, void *stream)
{
    g_fb_info = FeedbackInfo{};        // (smm_plan_feedback_info: this thread's last decode call)
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = stage(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes,
                   hs, &st, true, 0, true);
    if (rc != SMM_OK) return rc;
    int dev = 0;
    hipStream_t aux = nullptr;
    if (st.n_split > 0 && hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < 64) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(hs, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone) aux = aux_stream(dev);
    }
    std::pair<hipEvent_t, hipEvent_t> fj{nullptr, nullptr};
    if (aux && !aux_events_get(dev, fj)) aux = nullptr;
    if (!aux) {
        rc = run_emission(shape, st, x, w, cst, inv_var, cons, st.elp, elp32, hs);
        if (rc != SMM_OK) return rc;
        rc = run_viterbi(shape, st, st.elp, trans, init, len_scores, endpen, class_map, spans, labels, best, n_segs, hs);
        if (st.stamps && hipEventRecord(st.done, hs) != hipSuccess) (void)hipGetLastError();
        return rc;
    }
    // split decode (choose_split): [band tables, emission of the critical videos] on the caller's stream, then their DP
    // there, while the second stream scores and decodes the rest; the caller's stream waits for it at the end
    const int n1 = st.n_split, n2 = shape->b - st.n_split;
    rc = run_viterbi(shape, st, st.elp, trans, init, len_scores, endpen, class_map, spans, labels, best, n_segs, hs, 0, n1, true, false);
    if (rc != SMM_OK) { aux_events_put(dev, fj); return rc; }
    const hipEvent_t fork = fj.first, join = fj.second;
    int rc2 = SMM_OK;
    rc = run_emission(shape, st, x, w, cst, inv_var, cons, st.elp, elp32, hs, 0, n1);
    if (rc != SMM_OK) { aux_events_put(dev, fj); return rc; }
    // (the fork sits BEHIND the critical videos' emission on purpose: forked in front of it, the rest's emission workgroups fill
    // the CUs the critical videos' DP workgroups need -- one per CU, 245 VGPRs -- and that launch starts late: cfg3 2.81 -> 2.89 ms
    // per step, critical launch 2.31 -> 2.65 ms, three alternating runs on one box, round 5)
    if (hipEventRecord(fork, hs) != hipSuccess || hipStreamWaitEvent(aux, fork, 0) != hipSuccess) rc2 = SMM_ERR_HIP;
#ifdef SMM_DEV
    const int dbg_split = env().split_debug;                  // (timing experiments: results INCOMPLETE)
#else
    const int dbg_split = 0;
#endif
    if (rc2 == SMM_OK && !(dbg_split & 2)) rc2 = run_emission(shape, st, x, w, cst, inv_var, cons, st.elp, elp32, aux, n1, n2);
    if (rc2 == SMM_OK && !(dbg_split & 1))
        rc2 = run_viterbi(shape, st, st.elp, trans, init, len_scores, endpen, class_map, spans, labels, best, n_segs, aux, n1, n2, false, true, 2);
    rc = run_viterbi(shape, st, st.elp, trans, init, len_scores, endpen, class_map, spans, labels, best, n_segs, hs, 0, n1, false, true, 1);
    // the join is made even after an error on the way, so that the caller's stream never runs ahead of the second one
    if (hipEventRecord(join, aux) != hipSuccess || hipStreamWaitEvent(hs, join, 0) != hipSuccess) rc2 = SMM_ERR_HIP;
    aux_events_put(dev, fj);
    // plan feedback: the stamps of this call are whole once `done` is; a measurement taken on the way in is evaluated now
    if (st.stamps && hipEventRecord(st.done, hs) != hipSuccess) (void)hipGetLastError();
    if (rc == SMM_OK && rc2 == SMM_OK) feedback_evaluate(st, hs);
    return rc != SMM_OK ? rc : rc2;
}

extern "C" int smm_logz_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                            const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                            const double *elp, const double *trans, const double *init, const double *len_scores,
                            const double *endpen, double *logz, void *workspace, size_t workspace_bytes, void *stream)
{
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = stage(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes,
                   hs, &st);
    if (rc != SMM_OK) return rc;
    if (!elp || !trans || !init || !len_scores || !logz) return SMM_ERR_ARG;
    SmmDpArgs a = dp_args(shape, st, Tables{elp, trans, init, len_scores, endpen, nullptr});
    if (shape->flags & SMM_SHAPE_LOGZ_BOTH) {
        // forward and time-reversed recursion in one launch: the transposed tables and the reversed runs' closing values
        // live where run_reversed keeps them
        const ReversedTabs rt = reversed_tabs(shape, st.tabs);
        smm_launch_transpose(trans, rt.trans_t, shape->n_groups, shape->c_max, hs);
        a.trans_t = rt.trans_t;
        a.logz_b = rt.logz_b;
        a.flags |= 64;
    }
    rc = smm_launch_logz(a, logz, ring_regs(st.kp_max), st.c_need, hs);
    if (rc != SMM_OK) return rc;
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_logz_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                const double *elp, const double *trans, const double *init, const double *len_scores,
                                const double *endpen, const double *logz, const double *grad_logz, double *g_elp,
                                double *g_trans, double *g_init, double *g_len, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = stage(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes,
                   hs, &st);
    if (rc != SMM_OK) return rc;
    if (!elp || !trans || !init || !len_scores || !logz || !g_elp || !g_trans || !g_init || !g_len) return SMM_ERR_ARG;
    const size_t g = shape->n_groups, cm = shape->c_max;
    const bool no_eos = (shape->flags & SMM_SHAPE_NO_EOS) != 0;
    rc = run_reversed(shape, st, st.hist, st.tabs, Tables{elp, trans, init, len_scores, endpen, logz}, hs);
    if (rc != SMM_OK) return rc;
    {
        void *const zp[4] = {g_trans, g_init, g_len, g_elp};
        const size_t zb[4] = {sizeof(double) * g * cm * cm, sizeof(double) * g * cm, sizeof(double) * g * shape->k_rows * cm,
                              sizeof(double) * (size_t)shape->total_frames * cm};
        SMM_HIP((hipError_t)smm_zero_multi_async(zp, zb, 4, hs));
    }
    SmmBwdArgs m{st.videos, st.n_states, trans, len_scores, st.hist, logz, grad_logz, g_elp, g_trans, g_init, g_len,
                 shape->c_max, shape->k_rows, shape->b, elp, no_eos ? 1 : 0};
    smm_launch_marginals(m, shape->t_max, st.kp_max, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_sample_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                              const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                              const double *elp, const double *trans, const double *init, const double *len_scores,
                              const double *endpen, const int64_t *class_map, const double *logz, int32_t n_samples,
                              uint64_t seed, int64_t *spans_out, int64_t *labels_out, double *logp_out, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    if (n_samples <= 0 || (!spans_out && !labels_out && !logp_out)) return SMM_ERR_ARG;
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = stage(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes,
                   hs, &st);
    if (rc != SMM_OK) return rc;
    if (!elp || !trans || !init || !len_scores || !logz) return SMM_ERR_ARG;
    const SmmPostHead h = post_head(shape, st);
    const SmmSampleArgs a{h, post_side(h.no_eos, st.hist, Tables{elp, trans, init, len_scores, endpen, logz}), class_map,
                          spans_out, labels_out, logp_out, shape->total_frames, seed, shape->t_max, n_samples};
    smm_launch_sample(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_entropy_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                               const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                               const double *elp, const double *trans, const double *init, const double *len_scores,
                               const double *endpen, const double *logz, double *entropy_out, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (!entropy_out || !elp || !trans || !init || !len_scores || !logz) return SMM_ERR_ARG;
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const Tables p{elp, trans, init, len_scores, endpen, logz};
    const int rc = stage_both(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace,
                              workspace_bytes, p, hs, &st);
    if (rc != SMM_OK) return rc;
    const SmmPostHead h = post_head(shape, st);
    smm_launch_entropy(SmmEntropyArgs{h, post_side(h.no_eos, st.hist, p), entropy_out}, shape->t_max, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_segment_posteriors_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                          const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                          const double *elp, const double *trans, const double *init, const double *len_scores,
                                          const double *endpen, const int64_t *class_map, const double *logz,
                                          const int64_t *spans_in, int32_t n_sets, double *start_post, double *end_post,
                                          double *bnd_post, double *seg_logp, void *workspace, size_t workspace_bytes,
                                          void *stream)
{
    if (!elp || !trans || !init || !len_scores || !logz) return SMM_ERR_ARG;
    if (!start_post && !end_post && !bnd_post && !seg_logp) return SMM_ERR_ARG;
    if (seg_logp && !spans_in) return SMM_ERR_ARG;
    if (spans_in && n_sets <= 0) return SMM_ERR_ARG;
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const Tables p{elp, trans, init, len_scores, endpen, logz};
    const int rc = stage_both(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace,
                              workspace_bytes, p, hs, &st,
                              (seg_logp && shape && (int64_t)shape->b * n_sets > 0x7fffffff) ? SMM_ERR_UNSUPPORTED : SMM_OK);
    if (rc != SMM_OK) return rc;
    {
        const size_t fr = (size_t)shape->total_frames;
        void *const zp[3] = {start_post, end_post, bnd_post};
        const size_t zb[3] = {start_post ? sizeof(double) * fr * shape->c_max : 0, end_post ? sizeof(double) * fr * shape->c_max : 0,
                              bnd_post ? sizeof(double) * fr : 0};
        SMM_HIP((hipError_t)smm_zero_multi_async(zp, zb, 3, hs));
    }
    const SmmPostHead h = post_head(shape, st);
    smm_launch_segpost(SmmSegPostArgs{h, post_side(h.no_eos, st.hist, p), class_map, spans_in, start_post, end_post, bnd_post,
                                      seg_logp, shape->t_max, spans_in ? n_sets : 0}, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// The second workspace of the KL calls (q's forward histories) is only read: checked against the plan, before p's is staged,
// and pointed into
static int point_q(const smm_shape *shape, const int64_t *lengths_host, void *ws_q, size_t ws_q_bytes, Staged *sq)
{
    const int rc = room_ok(smm_workspace_bytes(shape, lengths_host), ws_q_bytes);
    if (rc != SMM_OK) return rc;
    plan_point(make_plan(shape, lengths_host), ws_q, sq);
    return SMM_OK;
}

extern "C" int smm_kl_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                          const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                          const double *elp_p, const double *trans_p, const double *init_p, const double *len_p,
                          const double *endpen_p, const double *logz_p, void *ws_p, size_t ws_p_bytes,
                          const double *elp_q, const double *trans_q, const double *init_q, const double *len_q,
                          const double *endpen_q, const double *logz_q, void *ws_q, size_t ws_q_bytes,
                          double *kl_out, double *xent_out, void *stream)
{
    if (!kl_out || !elp_p || !trans_p || !init_p || !len_p || !logz_p || !elp_q || !trans_q || !init_q || !len_q || !logz_q ||
        !ws_q)
        return SMM_ERR_ARG;
    Staged sq;
    const int rq = point_q(shape, lengths_host, ws_q, ws_q_bytes, &sq);
    if (rq != SMM_OK) return rq;
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const Tables p{elp_p, trans_p, init_p, len_p, endpen_p, logz_p}, q{elp_q, trans_q, init_q, len_q, endpen_q, logz_q};
    const int rc = stage_both(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, ws_p, ws_p_bytes, p,
                              hs, &st);                              // (p's side only)
    if (rc != SMM_OK) return rc;
    const SmmPostHead h = post_head(shape, st);
    smm_launch_kl(SmmKlArgs{h, post_side(h.no_eos, st.hist, p), post_side(h.no_eos, sq.hist, q), kl_out, xent_out}, shape->t_max,
                  hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ------------------------------------------------------------------------------------------------ entropy / KL gradients
// The caller's scratch of smm_entropy_bwd_f64 / smm_kl_bwd_f64: per video six [T+1][c_max] blocks (the etas of both directions
// and the occupancy differences), then one fixed part per video (its tables and values)
static bool ebwd_layout(const smm_shape *s, const int64_t *lengths, size_t *pv_base, size_t *total_doubles)
{
    if (!shape_ok(s) || !lengths || !limits_ok(s) || !lengths_ok(s, lengths)) return false;
    size_t h = 0;
    for (int i = 0; i < s->b; ++i) h += 6 * (size_t)s->c_max * (size_t)(lengths[i] + 1);
    *pv_base = h;
    *total_doubles = h + (size_t)s->b * smm_entropy_bwd_fixed_doubles(s->c_max, s->k_rows);
    return true;
}

extern "C" size_t smm_entropy_bwd_scratch_bytes(const smm_shape *shape, const int64_t *lengths_host)
{
    size_t pv = 0, tot = 0;
    if (!ebwd_layout(shape, lengths_host, &pv, &tot)) return 0;
    return sizeof(double) * tot;
}

// what the gradient units launch on (the expected reward's too): g_elp and the scratch's fixed parts zeroed, and the argument
// block.  p's histories in st, r's in hist_r (r = p for the entropy and the reward)
static int ebwd_args(const smm_shape *shape, const int64_t *lengths_host, const Staged &st, const double *hist_r,
                     const Tables &p, const Tables &r, int kl, const double *grad_out, double *g_elp, double *g_trans,
                     double *g_init, double *g_len, double *value_out, void *scratch, hipStream_t hs, SmmEntBwdArgs *e)
{
    size_t pv_base = 0, tot = 0;
    ebwd_layout(shape, lengths_host, &pv_base, &tot);
    double *sc = static_cast<double *>(scratch);
    {
        void *const zp[2] = {g_elp, sc + pv_base};
        const size_t zb[2] = {sizeof(double) * (size_t)shape->total_frames * shape->c_max, sizeof(double) * (tot - pv_base)};
        SMM_HIP((hipError_t)smm_zero_multi_async(zp, zb, 2, hs));
    }
    const SmmPostHead h = post_head(shape, st);
    *e = SmmEntBwdArgs{h, post_side(h.no_eos, st.hist, p), post_side(h.no_eos, hist_r, r), grad_out, g_elp, g_trans, g_init,
                       g_len, value_out, sc, (int64_t)pv_base, shape->n_groups, kl};
    return SMM_OK;
}

// both entropy / KL entry points
static int ebwd_run(const smm_shape *shape, const int64_t *lengths_host, const Staged &st, const double *hist_r,
                    const Tables &p, const Tables &r, int kl, const double *grad_out, double *g_elp, double *g_trans,
                    double *g_init, double *g_len, double *value_out, void *scratch, hipStream_t hs)
{
    SmmEntBwdArgs e;
    const int rc = ebwd_args(shape, lengths_host, st, hist_r, p, r, kl, grad_out, g_elp, g_trans, g_init, g_len, value_out,
                             scratch, hs, &e);
    if (rc != SMM_OK) return rc;
    smm_launch_entropy_bwd(e, shape->t_max, st.kp_max, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_entropy_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                   const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                   const double *elp, const double *trans, const double *init, const double *len_scores,
                                   const double *endpen, const double *logz, const double *grad_out, double *g_elp,
                                   double *g_trans, double *g_init, double *g_len, double *value_out, void *scratch,
                                   size_t scratch_bytes, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!elp || !trans || !init || !len_scores || !logz || !g_elp || !g_trans || !g_init || !g_len || !scratch)
        return SMM_ERR_ARG;
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = room_ok(smm_entropy_bwd_scratch_bytes(shape, lengths_host), scratch_bytes);
    if (rc != SMM_OK) return rc;
    const Tables p{elp, trans, init, len_scores, endpen, logz};
    rc = stage_both(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes, p, hs,
                    &st);
    if (rc != SMM_OK) return rc;
    return ebwd_run(shape, lengths_host, st, st.hist, p, p, 0, grad_out, g_elp, g_trans, g_init, g_len, value_out, scratch, hs);
}

extern "C" int smm_kl_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                              const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                              const double *elp_p, const double *trans_p, const double *init_p, const double *len_p,
                              const double *endpen_p, const double *logz_p, void *ws_p, size_t ws_p_bytes,
                              const double *elp_q, const double *trans_q, const double *init_q, const double *len_q,
                              const double *endpen_q, const double *logz_q, void *ws_q, size_t ws_q_bytes, int32_t mode,
                              const double *grad_out, double *g_elp, double *g_trans, double *g_init, double *g_len,
                              double *value_out, void *scratch, size_t scratch_bytes, void *stream)
{
    if (mode != SMM_KL_BWD_CROSS_ENTROPY && mode != SMM_KL_BWD_KL) return SMM_ERR_ARG;
    if (!elp_p || !trans_p || !init_p || !len_p || !logz_p || !elp_q || !trans_q || !init_q || !len_q || !logz_q || !ws_q ||
        !g_elp || !g_trans || !g_init || !g_len || !scratch)
        return SMM_ERR_ARG;
    Staged sq;
    const int rq = point_q(shape, lengths_host, ws_q, ws_q_bytes, &sq);
    if (rq != SMM_OK) return rq;
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = room_ok(smm_entropy_bwd_scratch_bytes(shape, lengths_host), scratch_bytes);
    if (rc != SMM_OK) return rc;
    const Tables p{elp_p, trans_p, init_p, len_p, endpen_p, logz_p}, q{elp_q, trans_q, init_q, len_q, endpen_q, logz_q};
    rc = stage_both(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, ws_p, ws_p_bytes, p, hs,
                    &st);                                           // both sides' backward histories
    if (rc == SMM_OK && sq.hist != st.hist) rc = run_reversed(shape, st, sq.hist, sq.tabs, q, hs);
    if (rc != SMM_OK) return rc;
    return ebwd_run(shape, lengths_host, st, sq.hist, p, q, mode == SMM_KL_BWD_KL ? 1 : 0, grad_out, g_elp, g_trans, g_init,
                    g_len, value_out, scratch, hs);
}

// ------------------------------------------------------------------------------------------------ expected reward
// (smm_expected_reward.hip).  The gradient's scratch has smm_entropy_bwd_f64's layout: its last two kernels run as they are.
extern "C" size_t smm_expected_reward_bwd_scratch_bytes(const smm_shape *shape, const int64_t *lengths_host)
{
    return smm_entropy_bwd_scratch_bytes(shape, lengths_host);
}

extern "C" int smm_expected_reward_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                       const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                       const double *elp, const double *trans, const double *init, const double *len_scores,
                                       const double *endpen, const double *logz, const double *reward, const double *seg_reward,
                                       double *value_out, double *parts_out, void *workspace, size_t workspace_bytes,
                                       void *stream)
{
    if (!value_out || !elp || !trans || !init || !len_scores || !logz || (!reward && !seg_reward)) return SMM_ERR_ARG;
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const Tables p{elp, trans, init, len_scores, endpen, logz};
    const int rc = stage_both(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace,
                              workspace_bytes, p, hs, &st);
    if (rc != SMM_OK) return rc;
    SmmExpRewardArgs a{};
    a.e.h = post_head(shape, st);
    a.e.p = a.e.r = post_side(a.e.h.no_eos, st.hist, p);
    a.reward = reward; a.seg_reward = seg_reward; a.value = value_out; a.parts = parts_out;
    smm_launch_expected_reward(a, shape->t_max, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_expected_reward_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                           const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                           const double *elp, const double *trans, const double *init, const double *len_scores,
                                           const double *endpen, const double *logz, const double *reward,
                                           const double *seg_reward, const double *grad_out, double *g_elp, double *g_trans,
                                           double *g_init, double *g_len, double *value_out, void *scratch, size_t scratch_bytes,
                                           void *workspace, size_t workspace_bytes, void *stream)
{
    if (!elp || !trans || !init || !len_scores || !logz || (!reward && !seg_reward) || !g_elp || !g_trans || !g_init || !g_len ||
        !scratch)
        return SMM_ERR_ARG;
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = room_ok(smm_expected_reward_bwd_scratch_bytes(shape, lengths_host), scratch_bytes);
    if (rc != SMM_OK) return rc;
    const Tables p{elp, trans, init, len_scores, endpen, logz};
    rc = stage_both(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes, p, hs,
                    &st);
    if (rc != SMM_OK) return rc;
    SmmExpRewardArgs a{};
    rc = ebwd_args(shape, lengths_host, st, st.hist, p, p, 0, grad_out, g_elp, g_trans, g_init, g_len, value_out, scratch, hs,
                   &a.e);
    if (rc != SMM_OK) return rc;
    a.reward = reward; a.seg_reward = seg_reward;
    smm_launch_expected_reward_bwd(a, shape->t_max, st.kp_max, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ------------------------------------------------------------------------------------------------ k best
// Behind the plan's workspace (its `total`): the length table state-major, the H lists of the last `ring` positions (and their
// heads apart, class-major), the back-pointers of G and H at every position, the closing lists, the back-trace's scratch.
struct KbestLayout {
    size_t o_lent, o_hh, o_h, o_gbp, o_hbp, o_fv, o_fk, o_segs, total;
    int64_t n_pos;
    int ring;
};

static bool kbest_layout(const smm_shape *s, const int64_t *lengths, int32_t k, KbestLayout *lo)
{
    if (k < 1 || k > SMM_MAX_KBEST || !shape_ok(s) || !lengths || !limits_ok(s) || !lengths_ok(s, lengths)) return false;
    int64_t n_pos = 0;
    for (int i = 0; i < s->b; ++i) n_pos += lengths[i] + 1;
    const size_t cm = (size_t)s->c_max, kk = (size_t)k, b = (size_t)s->b;
    lo->n_pos = n_pos;
    lo->ring = std::min<int>(s->k_rows, s->t_max + 1);
    Carver c{align_up(make_plan(s, lengths).total, 256)};
    lo->o_lent = c.take(sizeof(double) * s->n_groups * cm * s->k_rows);
    lo->o_hh = c.take(sizeof(double) * b * cm * lo->ring);
    lo->o_h = c.take(sizeof(double) * b * lo->ring * cm * kk);
    lo->o_gbp = c.take(sizeof(uint16_t) * (size_t)n_pos * cm * kk);
    lo->o_hbp = c.take(sizeof(uint16_t) * (size_t)n_pos * cm * kk);
    lo->o_fv = c.take(sizeof(double) * b * kk);
    lo->o_fk = c.take(sizeof(int32_t) * b * kk);
    lo->o_segs = c.take(sizeof(int32_t) * kk * (size_t)n_pos);
    lo->total = c.cur;
    return true;
}

extern "C" size_t smm_kbest_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host, int32_t k)
{
    KbestLayout lo;
    return kbest_layout(shape, lengths_host, k, &lo) ? lo.total : 0;
}

extern "C" int smm_kbest_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                             const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                             const double *elp, const double *trans, const double *init, const double *len_scores,
                             const double *endpen, const int64_t *class_map, int32_t k, int64_t *spans_out,
                             int64_t *labels_out, double *score_out, int32_t *n_segs_out, void *workspace,
                             size_t workspace_bytes, void *stream)
{
    if (k < 1 || k > SMM_MAX_KBEST || (!spans_out && !labels_out && !score_out && !n_segs_out)) return SMM_ERR_ARG;
    if (!shape_ok(shape) || !lengths_host) return SMM_ERR_ARG;
    if (!limits_ok(shape)) return SMM_ERR_UNSUPPORTED;
    KbestLayout lo;
    if (!kbest_layout(shape, lengths_host, k, &lo)) return SMM_ERR_ARG;
    if (!workspace) return SMM_ERR_ARG;
    if (workspace_bytes < lo.total) return SMM_ERR_WORKSPACE;
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    int rc = stage(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes,
                   hs, &st);
    if (rc != SMM_OK) return rc;
    if (!elp || !trans || !init || !len_scores) return SMM_ERR_ARG;
    const bool no_eos = (shape->flags & SMM_SHAPE_NO_EOS) != 0;
    char *base = static_cast<char *>(workspace);
    SmmKbestArgs a{};
    a.videos = st.videos; a.n_states = st.n_states;
    a.elp = elp; a.trans = trans; a.init = init; a.len = len_scores; a.endpen = no_eos ? nullptr : endpen;
    a.class_map = class_map;
    a.len_t = reinterpret_cast<double *>(base + lo.o_lent);
    a.hh = reinterpret_cast<double *>(base + lo.o_hh);
    a.hring = reinterpret_cast<double *>(base + lo.o_h);
    a.gbp = reinterpret_cast<uint16_t *>(base + lo.o_gbp);
    a.hbp = reinterpret_cast<uint16_t *>(base + lo.o_hbp);
    a.fin_v = reinterpret_cast<double *>(base + lo.o_fv);
    a.fin_k = reinterpret_cast<int32_t *>(base + lo.o_fk);
    a.segs = reinterpret_cast<int32_t *>(base + lo.o_segs);
    a.spans = spans_out; a.labels = labels_out; a.score = score_out; a.n_segs = n_segs_out; a.err = st.err;
    a.total_frames = shape->total_frames; a.n_pos = lo.n_pos;
    a.c_max = shape->c_max; a.k_rows = shape->k_rows; a.t_max = shape->t_max; a.b = shape->b; a.n_groups = shape->n_groups;
    a.k = k; a.ring = lo.ring; a.no_eos = no_eos ? 1 : 0;
    smm_launch_kbest(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ------------------------------------------------------------------------------------------------ MBR decode
// The history area of the plan (8 c_max (T + 1) doubles per video) holds what the MBR kernel keeps per video: cum, h, bt and the
// suffix maxima of h, then the frame labels.  Nothing behind the plan's `total`.
static bool mbr_shape_ok(const smm_shape *s, const int64_t *lengths)
{
    return shape_ok(s) && lengths && limits_ok(s) && lengths_ok(s, lengths);
}

extern "C" size_t smm_mbr_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host)
{
    return mbr_shape_ok(shape, lengths_host) ? make_plan(shape, lengths_host).total : 0;
}

extern "C" int smm_mbr_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                           const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                           const double *gain, const double *trans, const double *init, const double *endpen,
                           const int64_t *class_map, int64_t *spans, int64_t *labels, double *best, double *gain_sum,
                           int32_t *n_segs, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!shape_ok(shape) || !lengths_host || !frame_offset_host || !n_states_host) return SMM_ERR_ARG;
    if (!limits_ok(shape)) return SMM_ERR_UNSUPPORTED;
    if (!gain || !trans || !init || !workspace) return SMM_ERR_ARG;
    if (!spans && !labels && !best && !gain_sum && !n_segs) return SMM_ERR_ARG;
    const size_t need = smm_mbr_workspace_bytes(shape, lengths_host);
    if (need == 0) return SMM_ERR_ARG;
    if (workspace_bytes < need) return SMM_ERR_WORKSPACE;
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    const int rc = stage(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes,
                         hs, &st);
    if (rc != SMM_OK) return rc;
    const bool no_eos = (shape->flags & SMM_SHAPE_NO_EOS) != 0;
    SmmMbrArgs a{};
    a.videos = st.videos; a.order = st.order; a.n_states = st.n_states;
    a.gain = gain; a.trans = trans; a.init = init; a.endpen = no_eos ? nullptr : endpen; a.class_map = class_map;
    a.hist = st.hist;
    a.spans = spans; a.labels = labels; a.best = best; a.gain_sum = gain_sum; a.n_segs = n_segs; a.err = st.err;
    a.c_max = shape->c_max; a.t_max = shape->t_max; a.b = shape->b; a.no_eos = no_eos ? 1 : 0;
    smm_launch_mbr(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ------------------------------------------------------------------------------------------------ forced alignment
// The transcript entry points (alignment, alignment with optional entries, transcript likelihood, the same with optional
// entries) share one layout behind the plan's workspace: the transcript offsets, the offsets of the videos' columns and, where
// the family has parts, of their parts, and the launch order (uploaded per call: they are no part of a resident plan), then the
// videos' columns, then their parts.  cum uses the history area.  A family says how many doubles a video takes:
struct AlignFamily {
    size_t (*cells)(const smm_shape *s, int64_t m, int64_t t);   // the columns of a video with m entries and t frames
    size_t (*part)(const smm_shape *s, int64_t t);               // its parts of the gradients; null: the family has none
};
static size_t glen_part(const smm_shape *s, int64_t t) { return (size_t)(std::min<int64_t>(s->k_rows, t + 1) * s->c_max); }
// alignment: M h columns; with optional entries c_max columns of running maxima more
static const AlignFamily ALIGN = {[](const smm_shape *, int64_t m, int64_t t) { return (size_t)(m * (t + 1)); }, nullptr};
static const AlignFamily ALIGN_OPT = {[](const smm_shape *s, int64_t m, int64_t t) { return (size_t)((m + s->c_max) * (t + 1)); },
                                      nullptr};
// to a transcript graph: the h columns and, for the pull over the edges, the gam columns
static const AlignFamily ALIGN_GRAPH = {[](const smm_shape *, int64_t m, int64_t t) { return (size_t)(2 * m * (t + 1)); }, nullptr};
// likelihood: the h, gam and q columns; the parts are g_len's rows, min(k_rows, T + 1) c_max doubles
static const AlignFamily ALIGN_LOGZ = {[](const smm_shape *, int64_t m, int64_t t) { return (size_t)(3 * m * (t + 1)); }, glen_part};
// ... with optional entries: the columns' ranges (3 M doubles), the h, gam, q and bh columns and c_max columns of running
// per-class sums; the parts hold g_len's rows, then c_max^2 + c_max doubles of g_trans and g_init and the backward pass's own
// logZ_o
static const AlignFamily ALIGN_OPT_LOGZ = {
    [](const smm_shape *s, int64_t m, int64_t t) { return (size_t)(3 * m + (4 * m + s->c_max) * (t + 1)); },
    [](const smm_shape *s, int64_t t) { return glen_part(s, t) + (size_t)((int64_t)s->c_max * s->c_max + s->c_max + 1); }};

// ... over the paths of a transcript graph: the same block without the running sums (a column reads its neighbours' columns)
static const AlignFamily ALIGN_GRAPH_LOGZ = {[](const smm_shape *, int64_t m, int64_t t) { return smm_graph_block_doubles(m, t); },
                                             ALIGN_OPT_LOGZ.part};

struct AlignLayout {
    size_t o_toff, o_hoff, o_poff, o_order, meta_end, o_cols, o_part, total;
};

// SMM_OK, or the refusal; everything here is host arithmetic on the caller's arrays
static int align_layout(const AlignFamily &f, const smm_shape *s, const int64_t *lengths, const int64_t *toff, AlignLayout *lo)
{
    if (!shape_ok(s) || !lengths || !toff) return SMM_ERR_ARG;
    if ((s->flags & SMM_SHAPE_NO_EOS) || !limits_ok(s)) return SMM_ERR_UNSUPPORTED;
    if (toff[0] < 0 || !lengths_ok(s, lengths)) return SMM_ERR_ARG;
    size_t cells = 0, part = 0;
    bool too_long = false;
    for (int i = 0; i < s->b; ++i) {
        const int64_t m = toff[i + 1] - toff[i];
        if (m < 1) return SMM_ERR_ARG;                      // non-monotone offsets, or an empty transcript
        too_long |= m > SMM_MAX_TRANSCRIPT;
        cells += f.cells(s, m, lengths[i]);
        if (f.part) part += f.part(s, lengths[i]);
    }
    if (too_long) return SMM_ERR_UNSUPPORTED;
    const size_t b = (size_t)s->b;
    Carver c{align_up(make_plan(s, lengths).total, 256)};
    lo->o_toff = c.packed(sizeof(int64_t) * (b + 1));      // (the arrays up to meta_end go up in one upload)
    lo->o_hoff = c.packed(sizeof(int64_t) * b);
    lo->o_poff = c.packed(f.part ? sizeof(int64_t) * b : 0);
    lo->o_order = c.take(sizeof(int32_t) * b);
    lo->meta_end = lo->o_order + sizeof(int32_t) * b;
    lo->o_cols = c.packed(sizeof(double) * cells);
    if (f.part) c.cur = align_up(c.cur, 256);
    lo->o_part = c.packed(sizeof(double) * part);
    lo->total = c.cur;
    return SMM_OK;
}

static size_t align_workspace_bytes(const AlignFamily &f, const smm_shape *s, const int64_t *lengths, const int64_t *toff)
{
    AlignLayout lo;
    return align_layout(f, s, lengths, toff, &lo) == SMM_OK ? lo.total : 0;
}

// what every transcript entry point has staged when it fills its kernel arguments
struct AlignStaged {
    Staged st;
    const int32_t *order;      // [b] most lattice cells (T x M x span limit) first
    const int64_t *toff, *hoff, *poff;   // poff: null in a family without parts
    double *cols, *part;
};

// The refusals of the layout and of the workspace size, the staging, and this call's own metadata
static int align_stage(const AlignFamily &f, const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                       const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                       const int64_t *transcript_offset_host, void *workspace, size_t workspace_bytes, hipStream_t hs,
                       AlignStaged *out)
{
    AlignLayout lo;
    int rc = align_layout(f, shape, lengths_host, transcript_offset_host, &lo);
    if (rc != SMM_OK) return rc;
    if (workspace_bytes < lo.total) return SMM_ERR_WORKSPACE;
    rc = stage(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, workspace, workspace_bytes, hs, &out->st);
    if (rc != SMM_OK) return rc;
    const int b = shape->b;
    std::vector<char> host(lo.meta_end - lo.o_toff, 0);
    int64_t *h_toff = reinterpret_cast<int64_t *>(host.data());
    int64_t *h_hoff = reinterpret_cast<int64_t *>(host.data() + (lo.o_hoff - lo.o_toff));
    int64_t *h_poff = reinterpret_cast<int64_t *>(host.data() + (lo.o_poff - lo.o_toff));
    int32_t *h_order = reinterpret_cast<int32_t *>(host.data() + (lo.o_order - lo.o_toff));
    std::vector<double> work(b);
    int64_t cells = 0, part = 0;
    for (int i = 0; i < b; ++i) {
        const int64_t m = transcript_offset_host[i + 1] - transcript_offset_host[i];
        const int k = kp_host ? kp_host[i] : std::min<int>(shape->k_rows, shape->t_max);
        h_toff[i] = transcript_offset_host[i];
        h_hoff[i] = cells;
        cells += (int64_t)f.cells(shape, m, lengths_host[i]);
        if (f.part) {
            h_poff[i] = part;
            part += (int64_t)f.part(shape, lengths_host[i]);
        }
        work[i] = (double)m * (double)lengths_host[i] * (double)std::min<int64_t>(k, lengths_host[i]);
    }
    h_toff[b] = transcript_offset_host[b];
    std::iota(h_order, h_order + b, 0);
    std::stable_sort(h_order, h_order + b, [&](int x, int y) { return work[x] > work[y]; });
    char *base = static_cast<char *>(workspace);
    SMM_HIP((hipError_t)smm_upload_meta(base + lo.o_toff, host.data(), host.size(), hs));
    out->order = reinterpret_cast<const int32_t *>(base + lo.o_order);
    out->toff = reinterpret_cast<const int64_t *>(base + lo.o_toff);
    out->hoff = reinterpret_cast<const int64_t *>(base + lo.o_hoff);
    out->poff = f.part ? reinterpret_cast<const int64_t *>(base + lo.o_poff) : nullptr;
    out->cols = reinterpret_cast<double *>(base + lo.o_cols);
    out->part = reinterpret_cast<double *>(base + lo.o_part);
    return SMM_OK;
}

// Both alignment entry points up to their launch: the refusals, the staging, the kernel arguments
static int align_prepare(const AlignFamily &f, const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                         const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                         const double *elp, const double *trans, const double *init, const double *len_scores,
                         const double *endpen, const int64_t *class_map, const int32_t *transcript,
                         const int64_t *transcript_offset_host, int64_t *spans, int64_t *labels, double *best,
                         int32_t *n_segs, void *workspace, size_t workspace_bytes, hipStream_t hs, SmmAlignArgs *out)
{
    if (!shape_ok(shape) || !lengths_host || !frame_offset_host || !n_states_host || !transcript_offset_host) return SMM_ERR_ARG;
    if (!elp || !trans || !init || !len_scores || !transcript || !workspace) return SMM_ERR_ARG;
    if (!spans && !labels && !best && !n_segs) return SMM_ERR_ARG;
    AlignStaged sg;
    const int rc = align_stage(f, shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host,
                               transcript_offset_host, workspace, workspace_bytes, hs, &sg);
    if (rc != SMM_OK) return rc;
    SmmAlignArgs a{};
    a.videos = sg.st.videos; a.n_states = sg.st.n_states; a.order = sg.order; a.toff = sg.toff; a.hoff = sg.hoff;
    a.elp = elp; a.trans = trans; a.init = init; a.len = len_scores; a.endpen = endpen; a.class_map = class_map;
    a.transcript = transcript;
    a.hist = sg.st.hist; a.hcols = sg.cols;
    a.spans = spans; a.labels = labels; a.best = best; a.n_segs = n_segs; a.err = sg.st.err;
    a.c_max = shape->c_max; a.k_rows = shape->k_rows; a.t_max = shape->t_max; a.b = shape->b;
    *out = a;
    return SMM_OK;
}

extern "C" size_t smm_align_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                            const int64_t *transcript_offset_host)
{
    return align_workspace_bytes(ALIGN, shape, lengths_host, transcript_offset_host);
}

extern "C" int smm_align_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                             const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                             const double *elp, const double *trans, const double *init, const double *len_scores,
                             const double *endpen, const int64_t *class_map, const int32_t *transcript,
                             const int64_t *transcript_offset_host, int64_t *spans, int64_t *labels, double *best,
                             int32_t *n_segs, void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignArgs a;
    const int rc = align_prepare(ALIGN, shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp, trans,
                                 init, len_scores, endpen, class_map, transcript, transcript_offset_host, spans, labels, best,
                                 n_segs, workspace, workspace_bytes, hs, &a);
    if (rc != SMM_OK) return rc;
    smm_launch_align(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ... with optional entries (smm_align_opt.hip).  (The family reads shape->c_max behind the layout's shape_ok only.)
extern "C" size_t smm_align_opt_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                const int64_t *transcript_offset_host)
{
    return align_workspace_bytes(ALIGN_OPT, shape, lengths_host, transcript_offset_host);
}

extern "C" int smm_align_opt_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                 const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                 const double *elp, const double *trans, const double *init, const double *len_scores,
                                 const double *endpen, const int64_t *class_map, const int32_t *transcript,
                                 const uint8_t *optional, const int64_t *transcript_offset_host, int64_t *spans,
                                 int64_t *labels, double *best, int32_t *n_segs, int32_t *used, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    if (!optional) return SMM_ERR_ARG;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignArgs a;
    const int rc = align_prepare(ALIGN_OPT, shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp,
                                 trans, init, len_scores, endpen, class_map, transcript, transcript_offset_host, spans, labels,
                                 best, n_segs, workspace, workspace_bytes, hs, &a);
    if (rc != SMM_OK) return rc;
    a.optional = optional; a.used = used;
    smm_launch_align_opt(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ... to a transcript graph (smm_align_graph.hip): the nodes stand where the transcript's entries do
extern "C" size_t smm_align_graph_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                  const int64_t *node_offset_host)
{
    return align_workspace_bytes(ALIGN_GRAPH, shape, lengths_host, node_offset_host);
}

extern "C" int smm_align_graph_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                   const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                   const double *elp, const double *trans, const double *init, const double *len_scores,
                                   const double *endpen, const int64_t *class_map, const int32_t *node_class,
                                   const uint32_t *pred_mask, const uint8_t *node_flags, const int64_t *node_offset_host,
                                   int64_t *spans, int64_t *labels, double *best, int32_t *n_segs, int32_t *used,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    if (!pred_mask || !node_flags) return SMM_ERR_ARG;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignArgs a;
    const int rc = align_prepare(ALIGN_GRAPH, shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp,
                                 trans, init, len_scores, endpen, class_map, node_class, node_offset_host, spans, labels, best,
                                 n_segs, workspace, workspace_bytes, hs, &a);
    if (rc != SMM_OK) return rc;
    a.pred_mask = pred_mask; a.node_flags = node_flags; a.used = used;
    smm_launch_align_graph(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ------------------------------------------------------------------------------------------------ transcript likelihood
// What the six likelihood entry points (forward and backward: exact, with optional entries, over a graph) share up to their launch:
// the refusals, the staging, the kernel arguments but for `optional` and what the backward call adds
static int align_logz_prepare(const AlignFamily &f, const smm_shape *shape, const int64_t *lengths_host,
                              const int64_t *frame_offset_host, const int32_t *group_host, const int32_t *kp_host,
                              const int32_t *n_states_host, const double *elp, const double *trans, const double *init,
                              const double *len_scores, const double *endpen, const int32_t *transcript,
                              const int64_t *transcript_offset_host, const double *logz, void *workspace, size_t workspace_bytes,
                              hipStream_t hs, SmmAlignLogzArgs *a)
{
    if (!shape_ok(shape) || !lengths_host || !frame_offset_host || !n_states_host || !transcript_offset_host) return SMM_ERR_ARG;
    if (!elp || !trans || !init || !len_scores || !transcript || !logz || !workspace) return SMM_ERR_ARG;
    AlignStaged sg;
    const int rc = align_stage(f, shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host,
                               transcript_offset_host, workspace, workspace_bytes, hs, &sg);
    if (rc != SMM_OK) return rc;
    *a = SmmAlignLogzArgs{};
    a->videos = sg.st.videos; a->n_states = sg.st.n_states; a->order = sg.order;
    a->toff = sg.toff; a->hoff = sg.hoff; a->poff = sg.poff;
    a->elp = elp; a->trans = trans; a->init = init; a->len = len_scores; a->endpen = endpen; a->transcript = transcript;
    a->hist = sg.st.hist; a->cols = sg.cols; a->part = sg.part;
    a->logz = const_cast<double *>(logz);                       // (the backward launches only read it)
    a->err = sg.st.err;
    a->c_max = shape->c_max; a->k_rows = shape->k_rows; a->b = shape->b; a->n_groups = shape->n_groups;
    return SMM_OK;
}

// ... and the backward calls behind it: the gradients' arguments, and g_elp's zeros -- frames no video covers and the rows of
// skipped videos stay zero; the other gradients are written whole by their kernels
static int align_logz_bwd_outputs(const smm_shape *shape, const double *grad_logz, double *g_elp, double *g_trans, double *g_init,
                                  double *g_len, hipStream_t hs, SmmAlignLogzArgs *a)
{
    a->grad = grad_logz;
    a->g_elp = g_elp; a->g_trans = g_trans; a->g_init = g_init; a->g_len = g_len;
    SMM_HIP((hipError_t)smm_zero_async(g_elp, sizeof(double) * (size_t)shape->total_frames * shape->c_max, hs));
    return SMM_OK;
}

extern "C" size_t smm_align_logz_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                 const int64_t *transcript_offset_host)
{
    return align_workspace_bytes(ALIGN_LOGZ, shape, lengths_host, transcript_offset_host);
}

extern "C" int smm_align_logz_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                  const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                  const double *elp, const double *trans, const double *init, const double *len_scores,
                                  const double *endpen, const int32_t *transcript, const int64_t *transcript_offset_host,
                                  double *logz_a, void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignLogzArgs a;
    const int rc = align_logz_prepare(ALIGN_LOGZ, shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp,
                                      trans, init, len_scores, endpen, transcript, transcript_offset_host, logz_a, workspace,
                                      workspace_bytes, hs, &a);
    if (rc != SMM_OK) return rc;
    smm_launch_align_logz_fwd(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_align_logz_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                      const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                      const double *elp, const double *trans, const double *init, const double *len_scores,
                                      const double *endpen, const int32_t *transcript, const int64_t *transcript_offset_host,
                                      const double *logz_a, const double *grad_logz, double *g_elp, double *g_trans,
                                      double *g_init, double *g_len, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!g_elp || !g_trans || !g_init || !g_len) return SMM_ERR_ARG;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignLogzArgs a;
    int rc = align_logz_prepare(ALIGN_LOGZ, shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp,
                                trans, init, len_scores, endpen, transcript, transcript_offset_host, logz_a, workspace,
                                workspace_bytes, hs, &a);
    if (rc == SMM_OK) rc = align_logz_bwd_outputs(shape, grad_logz, g_elp, g_trans, g_init, g_len, hs, &a);
    if (rc != SMM_OK) return rc;
    smm_launch_align_logz_bwd(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ------------------------------------------------------------------------------------------------ ... with optional entries
extern "C" size_t smm_align_opt_logz_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                     const int64_t *transcript_offset_host)
{
    return align_workspace_bytes(ALIGN_OPT_LOGZ, shape, lengths_host, transcript_offset_host);
}

extern "C" int smm_align_opt_logz_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                      const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                      const double *elp, const double *trans, const double *init, const double *len_scores,
                                      const double *endpen, const int32_t *transcript, const uint8_t *optional,
                                      const int64_t *transcript_offset_host, double *logz_o, void *workspace,
                                      size_t workspace_bytes, void *stream)
{
    if (!optional) return SMM_ERR_ARG;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignLogzArgs a;
    const int rc = align_logz_prepare(ALIGN_OPT_LOGZ, shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host,
                                      elp, trans, init, len_scores, endpen, transcript, transcript_offset_host, logz_o, workspace,
                                      workspace_bytes, hs, &a);
    if (rc != SMM_OK) return rc;
    a.optional = optional;
    smm_launch_align_opt_logz_fwd(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_align_opt_logz_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                          const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                          const double *elp, const double *trans, const double *init, const double *len_scores,
                                          const double *endpen, const int32_t *transcript, const uint8_t *optional,
                                          const int64_t *transcript_offset_host, const double *logz_o, const double *grad_logz,
                                          double *g_elp, double *g_trans, double *g_init, double *g_len, double *p_used,
                                          void *workspace, size_t workspace_bytes, void *stream)
{
    if (!optional || !g_elp || !g_trans || !g_init || !g_len) return SMM_ERR_ARG;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignLogzArgs a;
    int rc = align_logz_prepare(ALIGN_OPT_LOGZ, shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp,
                                trans, init, len_scores, endpen, transcript, transcript_offset_host, logz_o, workspace,
                                workspace_bytes, hs, &a);
    if (rc == SMM_OK) rc = align_logz_bwd_outputs(shape, grad_logz, g_elp, g_trans, g_init, g_len, hs, &a);
    if (rc != SMM_OK) return rc;
    a.optional = optional; a.p_used = p_used;
    smm_launch_align_opt_logz_bwd(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ------------------------------------------------------------------------------------------------ ... over a transcript graph
extern "C" size_t smm_align_graph_logz_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                       const int64_t *node_offset_host)
{
    return align_workspace_bytes(ALIGN_GRAPH_LOGZ, shape, lengths_host, node_offset_host);
}

// What the forward call and every call behind it (backward, sampler, entropy, KL, their gradients) share up to their launch: the
// graph pointers' null test, the likelihood family's refusals, staging and arguments (the same layout, so the same columns), the
// graph into them
static int align_graph_prepare(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                               const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host, const double *elp,
                               const double *trans, const double *init, const double *len_scores, const double *endpen,
                               const int32_t *node_class, const uint32_t *pred_mask, const uint8_t *node_flags,
                               const int64_t *node_offset_host, const double *logz_g, void *workspace, size_t workspace_bytes,
                               hipStream_t hs, SmmAlignLogzArgs *a)
{
    if (!pred_mask || !node_flags) return SMM_ERR_ARG;
    const int rc = align_logz_prepare(ALIGN_GRAPH_LOGZ, shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host,
                                      elp, trans, init, len_scores, endpen, node_class, node_offset_host, logz_g, workspace,
                                      workspace_bytes, hs, a);
    if (rc != SMM_OK) return rc;
    a->pred_mask = pred_mask; a->node_flags = node_flags;
    return SMM_OK;
}

extern "C" int smm_align_graph_logz_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                        const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                        const double *elp, const double *trans, const double *init, const double *len_scores,
                                        const double *endpen, const int32_t *node_class, const uint32_t *pred_mask,
                                        const uint8_t *node_flags, const int64_t *node_offset_host, double *logz_g,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignLogzArgs a;
    const int rc = align_graph_prepare(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp, trans, init,
                                       len_scores, endpen, node_class, pred_mask, node_flags, node_offset_host, logz_g, workspace,
                                       workspace_bytes, hs, &a);
    if (rc != SMM_OK) return rc;
    smm_launch_align_graph_logz_fwd(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_align_graph_logz_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                            const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                            const double *elp, const double *trans, const double *init, const double *len_scores,
                                            const double *endpen, const int32_t *node_class, const uint32_t *pred_mask,
                                            const uint8_t *node_flags, const int64_t *node_offset_host, const double *logz_g,
                                            const double *grad_logz, double *g_elp, double *g_trans, double *g_init,
                                            double *g_len, double *p_used, double *p_end, void *workspace, size_t workspace_bytes,
                                            void *stream)
{
    if (!g_elp || !g_trans || !g_init || !g_len) return SMM_ERR_ARG;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignLogzArgs a;
    int rc = align_graph_prepare(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp, trans, init,
                                 len_scores, endpen, node_class, pred_mask, node_flags, node_offset_host, logz_g, workspace,
                                 workspace_bytes, hs, &a);
    if (rc == SMM_OK) rc = align_logz_bwd_outputs(shape, grad_logz, g_elp, g_trans, g_init, g_len, hs, &a);
    if (rc != SMM_OK) return rc;
    a.p_used = p_used; a.p_end = p_end;
    smm_launch_align_graph_logz_bwd(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// alignments drawn from the graph posterior (smm_align_graph_sample.hip): the forward call's staging and arguments again, then
// the sampler's own outputs
extern "C" int smm_align_graph_sample_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                          const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                          const double *elp, const double *trans, const double *init, const double *len_scores,
                                          const double *endpen, const int64_t *class_map, const int32_t *node_class,
                                          const uint32_t *pred_mask, const uint8_t *node_flags, const int64_t *node_offset_host,
                                          const double *logz_g, int32_t n_samples, uint64_t seed, int64_t *spans_out,
                                          int64_t *labels_out, double *logp_out, int32_t *n_segs_out, int32_t *used_out,
                                          void *workspace, size_t workspace_bytes, void *stream)
{
    if (n_samples <= 0) return SMM_ERR_ARG;
    if (!spans_out && !labels_out && !logp_out && !n_segs_out && !used_out) return SMM_ERR_ARG;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignSampleArgs a{};
    const int rc = align_graph_prepare(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp, trans, init,
                                       len_scores, endpen, node_class, pred_mask, node_flags, node_offset_host, logz_g, workspace,
                                       workspace_bytes, hs, &a.g);
    if (rc != SMM_OK) return rc;
    a.class_map = class_map;
    a.spans = spans_out; a.labels = labels_out; a.logp = logp_out; a.n_segs = n_segs_out; a.used = used_out;
    a.total_frames = shape->total_frames; a.n_nodes = node_offset_host[shape->b];
    a.seed = seed; a.t_max = shape->t_max; a.n_samples = n_samples;
    smm_launch_align_graph_sample(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// the entropy of the graph posterior (smm_align_graph_entropy.hip): the backward call's staging and arguments without its
// outputs, its first kernel for the q and bh columns -- not the g_elp / g_len / reduce tail --, then the entropy kernel
extern "C" int smm_align_graph_entropy_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                           const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                           const double *elp, const double *trans, const double *init, const double *len_scores,
                                           const double *endpen, const int32_t *node_class, const uint32_t *pred_mask,
                                           const uint8_t *node_flags, const int64_t *node_offset_host, const double *logz_g,
                                           double *h_out, double *h_parts, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!h_out) return SMM_ERR_ARG;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignEntropyArgs a{};
    const int rc = align_graph_prepare(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp, trans, init,
                                       len_scores, endpen, node_class, pred_mask, node_flags, node_offset_host, logz_g, workspace,
                                       workspace_bytes, hs, &a.g);
    if (rc != SMM_OK) return rc;
    a.h_out = h_out; a.h_parts = h_parts;
    smm_launch_align_graph_logz_bwd_columns(a.g, hs);
    smm_launch_align_graph_entropy(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// segment posteriors of given alignments and the nodes' boundary distributions (smm_align_graph_segpost.hip): the entropy call's
// staging, arguments and first kernel, then the gathers
extern "C" int smm_align_graph_segment_posteriors_f64(
    const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host, const int32_t *group_host,
    const int32_t *kp_host, const int32_t *n_states_host, const double *elp, const double *trans, const double *init,
    const double *len_scores, const double *endpen, const int64_t *class_map, const int32_t *node_class, const uint32_t *pred_mask,
    const uint8_t *node_flags, const int64_t *node_offset_host, const double *logz_g, const int64_t *spans_in,
    const int32_t *used_in, int32_t n_sets, double *seg_logp, double *node_logp, double *end_mean, double *end_sd,
    double *start_mean, double *start_sd, double *node_end_post, double *node_start_post, void *workspace, size_t workspace_bytes,
    void *stream)
{
    if (!seg_logp && !node_logp && !end_mean && !end_sd && !start_mean && !start_sd && !node_end_post && !node_start_post)
        return SMM_ERR_ARG;
    if ((seg_logp || node_logp) && (!spans_in || !used_in)) return SMM_ERR_ARG;
    if ((spans_in != nullptr) != (used_in != nullptr)) return SMM_ERR_ARG;
    if (spans_in && n_sets <= 0) return SMM_ERR_ARG;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignSegPostArgs a{};
    const int rc = align_graph_prepare(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp, trans, init,
                                       len_scores, endpen, node_class, pred_mask, node_flags, node_offset_host, logz_g, workspace,
                                       workspace_bytes, hs, &a.g);
    if (rc != SMM_OK) return rc;
    if (spans_in && (int64_t)shape->b * n_sets > 0x7fffffff) return SMM_ERR_UNSUPPORTED;
    a.class_map = class_map; a.spans_in = spans_in; a.used_in = used_in;
    a.seg_logp = seg_logp; a.node_logp = node_logp;
    a.end_mean = end_mean; a.end_sd = end_sd; a.start_mean = start_mean; a.start_sd = start_sd;
    a.node_end_post = node_end_post; a.node_start_post = node_start_post;
    a.n_nodes = node_offset_host[shape->b]; a.t_max = shape->t_max; a.n_sets = spans_in ? n_sets : 0;
    smm_launch_align_graph_logz_bwd_columns(a.g, hs);
    smm_launch_align_graph_segpost(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// What the two-sided calls (KL, the gradients) refuse before anything is staged: the null tests, the layout, with `distinct`
// one workspace for both sides, both workspaces' sizes
static int align_graph_two_sides(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                 const int32_t *n_states_host, const int64_t *node_offset_host, const double *elp_p,
                                 const double *trans_p, const double *init_p, const double *len_p, const int32_t *node_class,
                                 const double *logz_p, const void *ws_p, size_t ws_p_bytes, const double *trans_q,
                                 const double *len_q, const double *logz_q, const void *ws_q, size_t ws_q_bytes, bool distinct,
                                 AlignLayout *lo)
{
    if (!trans_q || !len_q || !logz_q || !ws_q) return SMM_ERR_ARG;
    if (!shape_ok(shape) || !lengths_host || !frame_offset_host || !n_states_host || !node_offset_host) return SMM_ERR_ARG;
    if (!elp_p || !trans_p || !init_p || !len_p || !node_class || !logz_p || !ws_p) return SMM_ERR_ARG;
    const int rc = align_layout(ALIGN_GRAPH_LOGZ, shape, lengths_host, node_offset_host, lo);
    if (rc != SMM_OK) return rc;
    if (distinct && ws_q == ws_p) return SMM_ERR_ARG;          // (one posterior against itself is the entropy call's)
    if (ws_p_bytes < lo->total || ws_q_bytes < lo->total) return SMM_ERR_WORKSPACE;
    return SMM_OK;
}

// ... and q's side of such a call: its histories and columns lie where the same plan and layout put p's; nothing is staged in
// q's workspace
static SmmAlignSideQ align_graph_side_q(const smm_shape *shape, const int64_t *lengths_host, const AlignLayout &lo,
                                        const double *trans_q, const double *len_q, const double *endpen_q, const double *logz_q,
                                        void *ws_q)
{
    Staged sq;
    plan_point(make_plan(shape, lengths_host), ws_q, &sq);
    return {trans_q, len_q, endpen_q, logz_q, sq.hist, reinterpret_cast<double *>(static_cast<char *>(ws_q) + lo.o_cols)};
}

// KL and cross-entropy of two graph posteriors (smm_align_graph_kl.hip): the entropy call's staging, arguments and first kernel
// on p's workspace; q's workspace is only read
extern "C" int smm_align_graph_kl_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                      const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                      const double *elp_p, const double *trans_p, const double *init_p, const double *len_scores_p,
                                      const double *endpen_p, const double *logz_g_p, void *workspace_p, size_t workspace_p_bytes,
                                      const double *trans_q, const double *len_scores_q, const double *endpen_q,
                                      const double *logz_g_q, const void *workspace_q, size_t workspace_q_bytes,
                                      const int32_t *node_class, const uint32_t *pred_mask, const uint8_t *node_flags,
                                      const int64_t *node_offset_host, double *kl_out, double *xent_out, double *kl_parts,
                                      void *stream)
{
    if (!pred_mask || !node_flags || !kl_out) return SMM_ERR_ARG;
    AlignLayout lo;
    SmmAlignKlArgs a{};
    int rc = align_graph_two_sides(shape, lengths_host, frame_offset_host, n_states_host, node_offset_host, elp_p, trans_p, init_p,
                                   len_scores_p, node_class, logz_g_p, workspace_p, workspace_p_bytes, trans_q, len_scores_q,
                                   logz_g_q, workspace_q, workspace_q_bytes, false, &lo);
    if (rc != SMM_OK) return rc;
    a.q = align_graph_side_q(shape, lengths_host, lo, trans_q, len_scores_q, endpen_q, logz_g_q,
                             const_cast<void *>(workspace_q));   // (the KL kernel only reads it)
    hipStream_t hs = static_cast<hipStream_t>(stream);
    rc = align_graph_prepare(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp_p, trans_p, init_p,
                             len_scores_p, endpen_p, node_class, pred_mask, node_flags, node_offset_host, logz_g_p, workspace_p,
                             workspace_p_bytes, hs, &a.g);
    if (rc != SMM_OK) return rc;
    a.kl_out = kl_out; a.xent_out = xent_out; a.kl_parts = kl_parts;
    smm_launch_align_graph_logz_bwd_columns(a.g, hs);
    smm_launch_align_graph_kl(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// gradients of the entropy, cross-entropy and KL of graph posteriors (smm_align_graph_entropy_bwd.hip).  The caller's scratch:
// per video five [M][T+1] blocks in the order of the workspace's column blocks (smm_launch.h: smm_graph_cells_before), one part
// per video, q's log Z as the call uses it and V+ per video
static bool agbwd_layout(const smm_shape *s, const int64_t *lengths, const int64_t *noff, size_t *pv_base, size_t *total_doubles)
{
    AlignLayout lo;
    if (align_layout(ALIGN_GRAPH_LOGZ, s, lengths, noff, &lo) != SMM_OK) return false;
    int64_t blocks = 0;
    for (int i = 0; i < s->b; ++i) blocks += (int64_t)smm_graph_block_doubles(noff[i + 1] - noff[i], lengths[i]);
    *pv_base = 5 * (size_t)smm_graph_cells_before(blocks, noff[s->b] - noff[0]);
    *total_doubles = *pv_base + (size_t)s->b * (smm_align_graph_entropy_bwd_part_doubles(s->c_max, s->k_rows) + 2);
    return true;
}

extern "C" size_t smm_align_graph_entropy_bwd_scratch_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                            const int64_t *node_offset_host)
{
    size_t pv = 0, tot = 0;
    if (!agbwd_layout(shape, lengths_host, node_offset_host, &pv, &tot)) return 0;
    return sizeof(double) * tot;
}

// both entry points (`two` false: the entropy, q's arguments are p's): the refusals, p's staging, each side's q and bh columns,
// the launch
static int agbwd_run(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                     const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host, const double *elp_p,
                     const double *trans_p, const double *init_p, const double *len_p, const double *endpen_p,
                     const double *logz_p, void *ws_p, size_t ws_p_bytes, const double *trans_q, const double *len_q,
                     const double *endpen_q, const double *logz_q, void *ws_q, size_t ws_q_bytes, bool two,
                     const int32_t *node_class, const uint32_t *pred_mask, const uint8_t *node_flags,
                     const int64_t *node_offset_host, int kl, const double *grad_out, double *g_elp, double *g_trans,
                     double *g_init, double *g_len, double *value_out, void *scratch, size_t scratch_bytes, hipStream_t hs)
{
    if (!pred_mask || !node_flags || !g_elp || !g_trans || !g_init || !g_len || !scratch) return SMM_ERR_ARG;
    AlignLayout lo;
    SmmAlignEntBwdArgs a{};
    int rc = align_graph_two_sides(shape, lengths_host, frame_offset_host, n_states_host, node_offset_host, elp_p, trans_p, init_p,
                                   len_p, node_class, logz_p, ws_p, ws_p_bytes, trans_q, len_q, logz_q, ws_q, ws_q_bytes, two, &lo);
    if (rc != SMM_OK) return rc;
    size_t pv_base = 0, tot = 0;
    agbwd_layout(shape, lengths_host, node_offset_host, &pv_base, &tot);
    if (scratch_bytes < sizeof(double) * tot) return SMM_ERR_WORKSPACE;
    rc = align_graph_prepare(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp_p, trans_p, init_p,
                             len_p, endpen_p, node_class, pred_mask, node_flags, node_offset_host, logz_p, ws_p, ws_p_bytes, hs,
                             &a.g);
    if (rc == SMM_OK) rc = align_logz_bwd_outputs(shape, grad_out, g_elp, g_trans, g_init, g_len, hs, &a.g);
    if (rc != SMM_OK) return rc;
    smm_launch_align_graph_logz_bwd_columns(a.g, hs);
    a.scratch = static_cast<double *>(scratch);
    a.q = SmmAlignSideQ{trans_p, len_p, endpen_p, logz_p, a.g.hist, a.g.cols};
    if (two) {
        // First the recorded ranges of the two sides, video by video: a video whose ranges differ gets a NaN in place of q's
        // log Z, which the q-side launch below skips (and answers with the error word) as every later kernel does -- nothing of
        // q's workspace is read or written through ranges that were not compared.  Then q's q and bh columns and parts,
        // exactly as q's own backward call would write them first: p's staged metadata (the two sides share it), q's tables,
        // histories, columns and parts
        double *lzq = a.scratch + pv_base + (size_t)shape->b * smm_align_graph_entropy_bwd_part_doubles(shape->c_max, shape->k_rows);
        a.q = align_graph_side_q(shape, lengths_host, lo, trans_q, len_q, endpen_q, lzq, ws_q);
        smm_launch_align_graph_entropy_bwd_check(a, logz_q, lzq, hs);
        SmmAlignLogzArgs q = a.g;
        q.trans = trans_q; q.len = len_q; q.endpen = endpen_q; q.logz = lzq;
        q.hist = a.q.hist; q.cols = a.q.cols;
        q.part = reinterpret_cast<double *>(static_cast<char *>(ws_q) + lo.o_part);
        q.grad = nullptr; q.g_elp = q.g_trans = q.g_init = q.g_len = nullptr;
        smm_launch_align_graph_logz_bwd_columns(q, hs);
    }
    a.value = value_out;
    a.pv_base = (int64_t)pv_base;
    a.kl = kl;
    smm_launch_align_graph_entropy_bwd(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_align_graph_entropy_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                               const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                               const double *elp, const double *trans, const double *init, const double *len_scores,
                                               const double *endpen, const int32_t *node_class, const uint32_t *pred_mask,
                                               const uint8_t *node_flags, const int64_t *node_offset_host, const double *logz_g,
                                               const double *grad_out, double *g_elp, double *g_trans, double *g_init,
                                               double *g_len, double *value_out, void *scratch, size_t scratch_bytes,
                                               void *workspace, size_t workspace_bytes, void *stream)
{
    return agbwd_run(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp, trans, init, len_scores,
                     endpen, logz_g, workspace, workspace_bytes, trans, len_scores, endpen, logz_g, workspace, workspace_bytes,
                     false, node_class, pred_mask, node_flags, node_offset_host, 0, grad_out, g_elp, g_trans, g_init, g_len,
                     value_out, scratch, scratch_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int smm_align_graph_kl_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                          const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                          const double *elp_p, const double *trans_p, const double *init_p,
                                          const double *len_scores_p, const double *endpen_p, const double *logz_g_p,
                                          void *workspace_p, size_t workspace_p_bytes, const double *trans_q,
                                          const double *len_scores_q, const double *endpen_q, const double *logz_g_q,
                                          void *workspace_q, size_t workspace_q_bytes, const int32_t *node_class,
                                          const uint32_t *pred_mask, const uint8_t *node_flags, const int64_t *node_offset_host,
                                          int32_t mode, const double *grad_out, double *g_elp, double *g_trans, double *g_init,
                                          double *g_len, double *value_out, void *scratch, size_t scratch_bytes, void *stream)
{
    if (mode != SMM_KL_BWD_CROSS_ENTROPY && mode != SMM_KL_BWD_KL) return SMM_ERR_ARG;
    return agbwd_run(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp_p, trans_p, init_p,
                     len_scores_p, endpen_p, logz_g_p, workspace_p, workspace_p_bytes, trans_q, len_scores_q, endpen_q, logz_g_q,
                     workspace_q, workspace_q_bytes, true, node_class, pred_mask, node_flags, node_offset_host,
                     mode == SMM_KL_BWD_KL ? 1 : 0, grad_out, g_elp, g_trans, g_init, g_len, value_out, scratch, scratch_bytes,
                     static_cast<hipStream_t>(stream));
}

// expected reward under the graph posterior and its gradient (smm_align_graph_expected_reward.hip).  The caller's scratch, in
// doubles: the value call's is the videos' cumW offsets [b], cumW ((T + 1) c_max per video), two partials per node; the gradient
// call's is the entropy-gradient call's layout, then the offsets and cumW
struct AgerLayout {
    size_t pv_base, o_off, o_cumw, o_partial, total;
};

static bool ager_layout(const smm_shape *s, const int64_t *lengths, const int64_t *noff, bool bwd, AgerLayout *lo)
{
    size_t front = 0;
    lo->pv_base = 0;
    if (bwd) {
        if (!agbwd_layout(s, lengths, noff, &lo->pv_base, &front)) return false;
    } else {
        AlignLayout al;
        if (align_layout(ALIGN_GRAPH_LOGZ, s, lengths, noff, &al) != SMM_OK) return false;
    }
    size_t rows = 0;
    for (int i = 0; i < s->b; ++i) rows += (size_t)lengths[i] + 1;
    lo->o_off = front;
    lo->o_cumw = lo->o_off + (size_t)s->b;
    lo->o_partial = lo->o_cumw + rows * (size_t)s->c_max;
    lo->total = lo->o_partial + (bwd ? 0 : 2 * (size_t)(noff[s->b] - noff[0]));
    return true;
}

extern "C" size_t smm_align_graph_expected_reward_scratch_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                                const int64_t *node_offset_host)
{
    AgerLayout lo;
    return ager_layout(shape, lengths_host, node_offset_host, false, &lo) ? sizeof(double) * lo.total : 0;
}

extern "C" size_t smm_align_graph_expected_reward_bwd_scratch_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                                    const int64_t *node_offset_host)
{
    AgerLayout lo;
    return ager_layout(shape, lengths_host, node_offset_host, true, &lo) ? sizeof(double) * lo.total : 0;
}

// both entry points up to their launch: the entropy-gradient call's refusals, their own, the staging, the q and bh columns
static int ager_prepare(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                        const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host, const double *elp,
                        const double *trans, const double *init, const double *len_scores, const double *endpen,
                        const int32_t *node_class, const uint32_t *pred_mask, const uint8_t *node_flags,
                        const int64_t *node_offset_host, const double *logz_g, const double *reward, const double *node_reward,
                        bool outputs_ok, bool bwd, void *scratch, size_t scratch_bytes, void *workspace, size_t workspace_bytes,
                        hipStream_t hs, SmmAlignExpRewardArgs *a)
{
    if (!pred_mask || !node_flags || !outputs_ok || !scratch || (!reward && !node_reward)) return SMM_ERR_ARG;
    AlignLayout al;
    int rc = align_graph_two_sides(shape, lengths_host, frame_offset_host, n_states_host, node_offset_host, elp, trans, init,
                                   len_scores, node_class, logz_g, workspace, workspace_bytes, trans, len_scores, logz_g, workspace,
                                   workspace_bytes, false, &al);
    if (rc != SMM_OK) return rc;
    AgerLayout lo;
    ager_layout(shape, lengths_host, node_offset_host, bwd, &lo);
    if (scratch_bytes < sizeof(double) * lo.total) return SMM_ERR_WORKSPACE;
    *a = SmmAlignExpRewardArgs{};
    rc = align_graph_prepare(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp, trans, init,
                             len_scores, endpen, node_class, pred_mask, node_flags, node_offset_host, logz_g, workspace,
                             workspace_bytes, hs, &a->e.g);
    if (rc != SMM_OK) return rc;
    double *sc = static_cast<double *>(scratch);
    a->e.scratch = sc;
    a->e.pv_base = (int64_t)lo.pv_base;
    a->e.q = SmmAlignSideQ{trans, len_scores, endpen, logz_g, a->e.g.hist, a->e.g.cols};
    a->reward = reward; a->node_reward = node_reward;
    a->cw_off = reinterpret_cast<int64_t *>(sc + lo.o_off);
    a->cumw = sc + lo.o_cumw;
    a->partial = sc + lo.o_partial;
    a->n_nodes = node_offset_host[shape->b] - node_offset_host[0];
    return SMM_OK;
}

extern "C" int smm_align_graph_expected_reward_f64(const smm_shape *shape, const int64_t *lengths_host,
                                                   const int64_t *frame_offset_host, const int32_t *group_host,
                                                   const int32_t *kp_host, const int32_t *n_states_host, const double *elp,
                                                   const double *trans, const double *init, const double *len_scores,
                                                   const double *endpen, const int32_t *node_class, const uint32_t *pred_mask,
                                                   const uint8_t *node_flags, const int64_t *node_offset_host, const double *logz_g,
                                                   const double *reward, const double *node_reward, double *value_out,
                                                   double *parts_out, void *scratch, size_t scratch_bytes, void *workspace,
                                                   size_t workspace_bytes, void *stream)
{
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignExpRewardArgs a;
    const int rc = ager_prepare(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp, trans, init,
                                len_scores, endpen, node_class, pred_mask, node_flags, node_offset_host, logz_g, reward,
                                node_reward, value_out != nullptr, false, scratch, scratch_bytes, workspace, workspace_bytes, hs, &a);
    if (rc != SMM_OK) return rc;
    a.value = value_out; a.parts = parts_out;
    smm_launch_align_graph_logz_bwd_columns(a.e.g, hs);
    smm_launch_align_graph_expected_reward(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_align_graph_expected_reward_bwd_f64(const smm_shape *shape, const int64_t *lengths_host,
                                                       const int64_t *frame_offset_host, const int32_t *group_host,
                                                       const int32_t *kp_host, const int32_t *n_states_host, const double *elp,
                                                       const double *trans, const double *init, const double *len_scores,
                                                       const double *endpen, const int32_t *node_class, const uint32_t *pred_mask,
                                                       const uint8_t *node_flags, const int64_t *node_offset_host,
                                                       const double *logz_g, const double *reward, const double *node_reward,
                                                       const double *grad_out, double *g_elp, double *g_trans, double *g_init,
                                                       double *g_len, double *value_out, void *scratch, size_t scratch_bytes,
                                                       void *workspace, size_t workspace_bytes, void *stream)
{
    hipStream_t hs = static_cast<hipStream_t>(stream);
    SmmAlignExpRewardArgs a;
    int rc = ager_prepare(shape, lengths_host, frame_offset_host, group_host, kp_host, n_states_host, elp, trans, init, len_scores,
                          endpen, node_class, pred_mask, node_flags, node_offset_host, logz_g, reward, node_reward,
                          g_elp && g_trans && g_init && g_len, true, scratch, scratch_bytes, workspace, workspace_bytes, hs, &a);
    if (rc == SMM_OK) rc = align_logz_bwd_outputs(shape, grad_out, g_elp, g_trans, g_init, g_len, hs, &a.e.g);
    if (rc != SMM_OK) return rc;
    a.vpm = value_out;
    smm_launch_align_graph_logz_bwd_columns(a.e.g, hs);
    smm_launch_align_graph_expected_reward_bwd(a, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ------------------------------------------------------------------------------------------------ dense boundary
struct DenseLayout {
    size_t o_len, o_alpha, o_beta, o_bp_from, o_bp_k, o_rmsg, total;
};

static DenseLayout dense_layout(int32_t b, int32_t n1, int32_t k, int32_t c)
{
    DenseLayout lo;
    Carver cv{0};
    lo.o_len = cv.take(sizeof(int64_t) * b);
    lo.o_alpha = cv.take(sizeof(double) * (size_t)b * k * k * c);
    lo.o_beta = cv.take(sizeof(double) * (size_t)b * (n1 + 1) * c);
    lo.o_bp_from = cv.take((size_t)b * n1 * k * c);
    lo.o_bp_k = cv.take(sizeof(uint16_t) * (size_t)b * (n1 + 1) * c);
    lo.o_rmsg = cv.take(sizeof(double) * (size_t)b * (n1 + 1) * c);       // backward messages (smm_dense_marginals_f32)
    lo.total = cv.cur;
    return lo;
}

extern "C" size_t smm_dense_workspace_bytes(int32_t b, int32_t n1, int32_t k, int32_t c)
{
    if (b < 1 || n1 < 1 || k < 1 || c < 1) return 0;
    return dense_layout(b, n1, k, c).total;
}

// both entry points: the refusals (ptrs_ok: no required pointer is null), then what every launch is told
static int dense_args(bool ptrs_ok, const float *scores, const int64_t *lengths_host, int32_t b, int32_t n1, int32_t k, int32_t c,
                      void *workspace, size_t workspace_bytes, DenseLayout *lo, SmmDenseArgs *a)
{
    if (!ptrs_ok || !scores || !lengths_host || !workspace || b < 1 || n1 < 1 || k < 1 || c < 1) return SMM_ERR_ARG;
    if (c > 255 || k > 65535) return SMM_ERR_UNSUPPORTED;
    *lo = dense_layout(b, n1, k, c);
    if (workspace_bytes < lo->total) return SMM_ERR_WORKSPACE;
    for (int i = 0; i < b; ++i)
        if (lengths_host[i] < 1 || lengths_host[i] > n1 + 1) return SMM_ERR_ARG;
    char *base = static_cast<char *>(workspace);
    a->edge = scores;
    a->lengths = reinterpret_cast<int64_t *>(base + lo->o_len);
    a->alpha = reinterpret_cast<double *>(base + lo->o_alpha);
    a->beta = reinterpret_cast<double *>(base + lo->o_beta);
    a->b = b; a->n1 = n1; a->k = k; a->c = c;
    return SMM_OK;
}

extern "C" int smm_dense_dp_f32(const float *scores, const int64_t *lengths_host, int32_t b, int32_t n1, int32_t k,
                                int32_t c, int32_t semiring, double *v, int64_t *spans, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    DenseLayout lo;
    SmmDenseArgs a{};
    const int rc = dense_args(v != nullptr, scores, lengths_host, b, n1, k, c, workspace, workspace_bytes, &lo, &a);
    if (rc != SMM_OK) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    char *base = static_cast<char *>(workspace);
    a.bp_from = reinterpret_cast<uint8_t *>(base + lo.o_bp_from);
    a.bp_k = reinterpret_cast<uint16_t *>(base + lo.o_bp_k);
    SMM_HIP((hipError_t)smm_upload_meta(base + lo.o_len, lengths_host, sizeof(int64_t) * b, hs));
    a.v = v; a.spans = spans;
    smm_launch_dense(a, semiring != 0, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_dense_marginals_f32(const float *scores, const int64_t *lengths_host, int32_t b, int32_t n1, int32_t k,
                                       int32_t c, const double *v, const double *grad_v, float *marginals, void *workspace,
                                       size_t workspace_bytes, void *stream)
{
    DenseLayout lo;
    SmmDenseArgs a{};
    const int rc = dense_args(v && marginals, scores, lengths_host, b, n1, k, c, workspace, workspace_bytes, &lo, &a);
    if (rc != SMM_OK) return rc;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    double *rmsg = reinterpret_cast<double *>(static_cast<char *>(workspace) + lo.o_rmsg);
    a.v = const_cast<double *>(v);
    smm_launch_dense_marginals(a, rmsg, grad_v, marginals, hs);     // (lengths, beta: left by smm_dense_dp_f32, semiring 1)
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// ------------------------------------------------------------------------------------------------ feature projection (smm_flow.hip)
extern "C" int smm_emission_bwd_x_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                      const int32_t *group_host, const int32_t *n_states_host, const float *x,
                                      const double *g_elp, const double *w, const double *inv_var, float *g_x,
                                      void *workspace, size_t workspace_bytes, void *stream)
{
    Staged st;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    if (!x || !g_elp || !w || !inv_var || !g_x || !shape || shape->d < 1) return SMM_ERR_ARG;
    int rc = stage(shape, lengths_host, frame_offset_host, group_host, nullptr, n_states_host, workspace, workspace_bytes,
                   hs, &st, false, smm_emission_bwd_chunk());
    if (rc != SMM_OK) return rc;
    int64_t covered = 0;
    for (int i = 0; i < shape->b; ++i) covered += lengths_host[i];
    if (covered != shape->total_frames)                         // (a padded layout: the rows between the videos)
        SMM_HIP((hipError_t)smm_zero_async(g_x, sizeof(float) * (size_t)shape->total_frames * shape->d, hs));
    SmmEmBwdXArgs a{st.videos, st.order, st.n_states, st.em_cum, x, g_elp, w, inv_var, g_x,
                    shape->d, shape->c_max, shape->b, st.em_blocks, smm_emission_bwd_chunk()};
    smm_launch_emission_bwd_x(a, st.c_need, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

// SMM_OK and the launch plan, or the refusal: host logic only
static int flow_check(const smm_flow_shape *s, bool bwd, SmmFlowPlan *plan)
{
    if (!s || s->n_rows < 1 || (s->d & 1)) return SMM_ERR_ARG;
    if (s->d < 2 || s->d > 512 || s->hidden_units < 1 || s->hidden_units > 256 || s->hidden_layers < 0 || s->hidden_layers > 4 ||
        s->couple_layers < 1 || s->couple_layers > 16)
        return SMM_ERR_UNSUPPORTED;
    return smm_flow_plan(s->n_rows, s->d, s->hidden_units, s->hidden_layers, s->couple_layers, bwd, plan) ? SMM_OK : SMM_ERR_UNSUPPORTED;
}

static SmmFlowArgs flow_args(const smm_flow_shape *s, const SmmFlowPlan &p, const float *x, const float *g_y, const float *params,
                             float *out, double *partials)
{
    float *keep_global = p.keep == 2 ? reinterpret_cast<float *>(partials + p.n_params * (size_t)p.grid) : nullptr;
    return SmmFlowArgs{x, g_y, params, out, partials, keep_global, s->n_rows, (int64_t)p.n_params, s->d, s->hidden_units, s->hidden_layers,
                       s->couple_layers, p.strips, p.slab_rows, p.n_tiles, p.keep};
}

// the fp64 partials of every workgroup, then (keep = 2) every workgroup's kept halves
static size_t flow_bwd_bytes(const SmmFlowPlan &p)
{
    return sizeof(double) * p.n_params * (size_t)p.grid + sizeof(float) * p.keep_floats * (size_t)p.grid;
}

extern "C" size_t smm_flow_scratch_bytes(const smm_flow_shape *) { return 0; }

extern "C" size_t smm_flow_bwd_scratch_bytes(const smm_flow_shape *shape)
{
    SmmFlowPlan p{};
    if (flow_check(shape, true, &p) != SMM_OK) return 0;
    return flow_bwd_bytes(p);
}

extern "C" int smm_flow_f32(const smm_flow_shape *shape, const float *x, const float *params, float *y, void *scratch,
                            size_t scratch_bytes, void *stream)
{
    (void)scratch; (void)scratch_bytes;
    SmmFlowPlan p{};
    const int rc = flow_check(shape, false, &p);
    if (rc != SMM_OK) return rc;
    if (!x || !params || !y) return SMM_ERR_ARG;
    smm_launch_flow_fwd(flow_args(shape, p, x, nullptr, params, y, nullptr), p, static_cast<hipStream_t>(stream));
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}

extern "C" int smm_flow_bwd_f32(const smm_flow_shape *shape, const float *x, const float *g_y, const float *params,
                                double *g_params, float *g_x, void *scratch, size_t scratch_bytes, void *stream)
{
    SmmFlowPlan p{};
    const int rc = flow_check(shape, true, &p);
    if (rc != SMM_OK) return rc;
    if (!x || !g_y || !params || !g_params || !scratch) return SMM_ERR_ARG;
    const size_t need = flow_bwd_bytes(p);
    if (scratch_bytes < need) return SMM_ERR_WORKSPACE;
    hipStream_t hs = static_cast<hipStream_t>(stream);
    double *partials = static_cast<double *>(scratch);
    SMM_HIP((hipError_t)smm_zero_async(partials, sizeof(double) * p.n_params * (size_t)p.grid, hs));
    smm_launch_flow_bwd(flow_args(shape, p, x, g_y, params, g_x, partials), p, hs);
    smm_launch_flow_reduce(partials, p.grid, p.n_params, g_params, hs);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
}
