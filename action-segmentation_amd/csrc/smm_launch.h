// smm_launch.h -- launch wrappers shared between the kernel translation units and smm_api.hip.
#pragma once
#include "smm_device.h"

struct SmmEmArgs {
    const SmmVideo *videos;
    const int32_t *order;    // [b] block -> video (most work first)
    const int32_t *n_states;
    const float *x;          // [total_frames][d]
    const double *w;         // [g][d][c_max]
    const double *cst;       // [g][c_max]
    const double *inv_var;   // [d]
    const float *cons;       // [total_frames][c_max] or null
    double *elp64;           // [total_frames][c_max] or null
    float *elp32;            // [total_frames][c_max] or null
    int32_t d, c_max, b;
};

// Host metadata -> device, stream-ordered, WITHOUT a host-to-device copy: the bytes travel in the kernel-argument
// segment of tiny copy kernels (2 KB per launch).  A hipMemcpyAsync from pageable host memory makes the host wait until
// the stream has drained (and cannot be captured into a hipGraph); this does neither.  Returns a hipError_t as int.
int smm_upload_meta(void *dst_dev, const void *src_host, size_t bytes, hipStream_t stream);
// zero fill by a kernel (a hipMemsetAsync captured into a hipGraph does not replay reliably: smm_api.hip); hipError_t as int
int smm_zero_async(void *dst_dev, size_t bytes, hipStream_t stream);
// ... of up to eight regions in one launch
int smm_zero_multi_async(void *const *dst_dev, const size_t *bytes, int n, hipStream_t stream);

// flat grid: blk_cum[i] (device, [b + 1]) = workgroups of the videos order[0..i), built by the host from
// smm_emission_tiles_per_wave / smm_emission_blocks
int smm_emission_tiles_per_wave(int64_t total_frames, int b);
int smm_emission_blocks(int t, int tpw);
size_t smm_emission_lds_bytes(int d, int c_need);   // LDS of one workgroup: the largest class set's weight table + inv_var
void smm_launch_emission(const SmmEmArgs &a, int c_need, int tpw, int n_blocks, const int32_t *blk_cum, int64_t total_frames,
                         hipStream_t stream, int blk_base = 0, int vid0 = 0, int nvid = -1);
void smm_launch_widen(const float *src, double *dst, size_t n, hipStream_t stream);

// chain rule through the emission scorer (smm_emission.hip): outputs must be zero at launch
struct SmmEmBwdArgs {
    const SmmVideo *videos;
    const int32_t *order;    // [b]
    const int32_t *n_states;
    const int32_t *cum;      // [b + 1] chunks of smm_emission_bwd_chunk() frames before each video of `order`
    const float *x;          // [total_frames][d]
    const double *g_elp;     // [total_frames][c_max]
    double *g_w;             // [g][c_max][d]   (class-major)
    double *g_cst;           // [g][c_max]
    double *g_iv;            // [d]
    int32_t d, c_max, b, n_chunks;
};
int smm_emission_bwd_chunk();
void smm_launch_emission_bwd(const SmmEmBwdArgs &a, int c_need, hipStream_t stream);
// returns an smm_status; r = ring registers per lane (1,2,4,..,64), c_need = max states of any group
int smm_launch_viterbi(const SmmDpArgs &a, int r, int c_need, hipStream_t stream);
int smm_launch_viterbi_small(const SmmDpArgs &a, hipStream_t stream);   // BAND mode, <= 16 states, four-wave workgroups (two per CU)
int smm_launch_viterbi_repair(const SmmDpArgs &a, int c_need, hipStream_t stream);   // BAND mode (time-split decode: smm_chunk.hip)
// Viterbi BAND mode: the state-major length table and the skip-test bounds of every (group, state) (smm_viterbi.hip)
void smm_launch_band_tables(const double *len, const int32_t *n_states, double *len_t, double *band_tab, double *dmin_t,
                            int n_groups, int cm, int k_rows, hipStream_t stream);
// time-split Viterbi decode (smm_chunk.hip): serial prefix sums at the units' first positions; certification, back-trace and
// outputs of the split videos (redo[i] = 1: video i of `cvs` has to be decoded again in one piece)
void smm_launch_cum_anchors(const SmmDpArgs &a, const SmmChunkVideo *cvs, int n_split, double *anchors, hipStream_t stream);
void smm_launch_chunk_stitch(const SmmDpArgs &a, const SmmChunkVideo *cvs, int n_split, int32_t *redo, hipStream_t stream);
// tuning switches other translation units read (smm_api.hip: SmmEnv; read once, see smm_env_reload)
int smm_env_fit_grid();        // SMM_FIT_GRID (0: default)
int smm_env_emission_v2();     // SMM_EMISSION_V2 (-DSMM_DEV builds only)
// LogSemiring forward: logz[b]; same arguments as the Viterbi launch
int smm_launch_logz(const SmmDpArgs &a, double *logz, int r, int c_need, hipStream_t stream);

struct SmmBwdArgs {
    const SmmVideo *videos;
    const int32_t *n_states;
    const double *trans;       // forward tables [g][c_max][c_max], [g][k_rows][c_max]
    const double *len;
    const double *hist;        // per video: F_cum, F_h, F_g, B_cum, B_h, B_g, (scratch) hT0, hT1; each [T+1][c_max]
    const double *logz;        // [b]
    const double *grad_logz;   // [b] or null (= 1)
    double *g_elp;             // [total_frames][c_max]
    double *g_trans;           // [g][c_max][c_max]
    double *g_init;            // [g][c_max]
    double *g_len;             // [g][k_rows][c_max]
    int32_t c_max, k_rows, b;
    const double *elp;         // [total_frames][c_max]   (no_eos only: the closing label's emission)
    int32_t no_eos;            // add_eos=False (smmdp.h: SMM_SHAPE_NO_EOS)
};
void smm_launch_transpose(const double *src, double *dst, int g, int cm, hipStream_t stream);
void smm_launch_marginals(const SmmBwdArgs &a, int t_max, int kp_max, hipStream_t stream);

struct SmmDenseArgs {
    const float *edge;        // [b][n1][k][c][c]  (c_to, c_from)
    const int64_t *lengths;   // [b] positions (device)
    double *alpha;            // scratch [b][k][k][c]
    double *beta;             // scratch [b][n1+1][c]
    uint8_t *bp_from;         // scratch [b][n1][k][c]   (max semiring)
    uint16_t *bp_k;           // scratch [b][n1+1][c]
    double *v;                // [b]
    int64_t *spans;           // [b][n1+1] or null
    int32_t b, n1, k, c;
};
void smm_launch_dense(const SmmDenseArgs &a, bool log_semiring, hipStream_t stream);
// posterior edge marginals (x upstream gradient) from the beta a LogSemiring smm_launch_dense left in a.beta and a.v
void smm_launch_dense_marginals(const SmmDenseArgs &a, double *rmsg, const double *grad_v, float *out, hipStream_t stream);

// What the posterior units' argument structs repeat.  The head: the staged videos, the error word, the sizes, add_eos=False
struct SmmPostHead {
    const SmmVideo *videos;
    const int32_t *n_states;
    int32_t *err;              // sticky error word (p's workspace)
    int32_t c_max, k_rows, b, no_eos;
};
// ... and one side (one posterior): its histories in a workspace smm_launch_logz ran on, its tables, its log Z
struct SmmPostSide {
    const double *hist;        // per video: F_cum, F_h, F_g, B_cum, B_h, B_g, (scratch) hT0, hT1; each [T+1][c_max] (smm_logz_bwd.hip)
    const double *elp;         // [total_frames][c_max]
    const double *trans;       // [g][c_max][c_max]  [to][from]
    const double *init;        // [g][c_max]
    const double *len;         // [g][k_rows][c_max]
    const double *endpen;      // [b][c_max] or null (null without EOS)
    const double *logz;        // [b]
};

// posterior sampling (smm_sample.hip): after smm_launch_logz on the same workspace (forward histories)
struct SmmSampleArgs {
    SmmPostHead h;             // (err: a decision without a finite candidate)
    SmmPostSide p;
    const int64_t *class_map;  // [g][c_max+1] or null
    int64_t *spans;            // [n_samples][b][t_max+1] or null
    int64_t *labels;           // [n_samples][total_frames] or null
    double *logp;              // [n_samples][b] or null
    int64_t total_frames;
    uint64_t seed;
    int32_t t_max, n_samples;
};
void smm_launch_sample(const SmmSampleArgs &a, hipStream_t stream);

// k best segmentations (smm_kbest.hip): the lists and back-pointers live in the part of the workspace behind smm_workspace_bytes
struct SmmKbestArgs {
    const SmmVideo *videos;
    const int32_t *n_states;
    const double *elp;         // [total_frames][c_max]
    const double *trans;       // [g][c_max][c_max]  [to][from]
    const double *init;        // [g][c_max]
    const double *len;         // [g][k_rows][c_max]
    const double *endpen;      // [b][c_max] or null (EOS mode only)
    const int64_t *class_map;  // [g][c_max+1] or null
    double *len_t;             // [g][c_max][k_rows]     the length table, state-major
    double *hh;                // [b][c_max][ring]       H[s][c][0] of the last `ring` positions
    double *hring;             // [b][ring][c_max][k]    H[s][c][:] of the last `ring` positions
    uint16_t *gbp, *hbp;       // [n_pos][c_max][k]      back-pointers of G and H (video i from position sum_{i' < i} (T_i' + 1))
    double *fin_v;             // [b][k]                 the closing list
    int32_t *fin_k;            // [b][k]                 ... its back-pointers: to << 9 | j * 16 + r
    int32_t *segs;             // [k][n_pos]             back-trace scratch: (length << 5) | class per segment, last first
    int64_t *spans;            // [k][b][t_max+1] or null
    int64_t *labels;           // [k][total_frames] or null
    double *score;             // [k][b] or null
    int32_t *n_segs;           // [k][b] or null
    int32_t *err;              // sticky error word
    int64_t total_frames, n_pos;
    int32_t c_max, k_rows, t_max, b, n_groups, k, ring, no_eos;
};
void smm_launch_kbest(const SmmKbestArgs &a, hipStream_t stream);

// exact posterior entropy (smm_entropy.hip): after smm_launch_logz forward AND time-reversed on the same workspace
struct SmmEntropyArgs {
    SmmPostHead h;
    SmmPostSide p;
    double *entropy;           // [b] nats
};
void smm_launch_entropy(const SmmEntropyArgs &a, int t_max, hipStream_t stream);

// posteriors of segment boundaries and of given segments (smm_segpost.hip): after smm_launch_logz forward AND time-reversed on
// the same workspace; the dense outputs are zero at launch
struct SmmSegPostArgs {
    SmmPostHead h;
    SmmPostSide p;
    const int64_t *class_map;  // [g][c_max+1] or null
    const int64_t *spans_in;   // [n_sets][b][t_max+1] or null
    double *start_post;        // [total_frames][c_max] or null
    double *end_post;          // [total_frames][c_max] or null
    double *bnd_post;          // [total_frames] or null
    double *seg_logp;          // [n_sets][b][t_max+1] or null (needs spans_in)
    int32_t t_max, n_sets;
};
void smm_launch_segpost(const SmmSegPostArgs &a, hipStream_t stream);

// KL divergence and cross-entropy between two posteriors of one lattice (smm_kl.hip): after smm_launch_logz forward AND
// time-reversed on p's workspace and forward on q's (the same shape and metadata, so the same history offsets)
struct SmmKlArgs {
    SmmPostHead h;
    SmmPostSide p, q;          // (q: forward histories only)
    double *kl;                // [b] nats
    double *xent;              // [b] nats, or null
};
void smm_launch_kl(const SmmKlArgs &a, int t_max, hipStream_t stream);

// gradients of the entropy, cross-entropy and KL with respect to p's tables (smm_entropy_bwd.hip): after smm_launch_logz forward
// AND time-reversed on p's workspace and on r's (r = q; for the entropy r = p again)
struct SmmEntBwdArgs {
    SmmPostHead h;
    SmmPostSide p, r;
    const double *grad_out;               // [b] or null (= 1)
    double *g_elp, *g_trans, *g_init, *g_len;   // smm_logz_bwd_f64's layouts; g_elp zero at launch
    double *value;                        // [b][2] or null: the value by the two decompositions
    double *scratch;                      // caller's: per video 6 [T+1][c_max] blocks at 6/8 of hist_off, then the fixed parts
    int64_t pv_base;                      // doubles in front of the fixed parts (zero at launch)
    int32_t n_groups, kl;
};
size_t smm_entropy_bwd_fixed_doubles(int c_max, int k_rows);   // the fixed part of one video
void smm_launch_entropy_bwd(const SmmEntBwdArgs &a, int t_max, int kp_max, hipStream_t stream);
// ... its last two kernels alone (g_elp as the running sum of D, the groups' tables): what follows kernels that left D and the
// per-video sums in that unit's scratch layout (smm_expected_reward.hip does)
void smm_launch_entropy_bwd_tail(const SmmEntBwdArgs &a, hipStream_t stream);

// expected frame- and segment-additive reward and its gradient with respect to p's tables (smm_expected_reward.hip): after
// smm_launch_logz forward AND time-reversed on the same workspace.  The value launch reads e.h and e.p only; the gradient launch
// uses e as smm_launch_entropy_bwd does (e.r and e.kl unused; e.value: V-, V+)
struct SmmExpRewardArgs {
    SmmEntBwdArgs e;
    const double *reward;      // [total_frames][c_max] or null
    const double *seg_reward;  // [g][c_max] or null
    double *value;             // [b]               (value launch)
    double *parts;             // [b][2] or null: frame part, segment part   (value launch)
};
void smm_launch_expected_reward(const SmmExpRewardArgs &a, int t_max, hipStream_t stream);
void smm_launch_expected_reward_bwd(const SmmExpRewardArgs &a, int t_max, int kp_max, hipStream_t stream);

// minimum-Bayes-risk decode under frame loss (smm_mbr.hip): the Viterbi DP on the substituted inputs of smmdp.h (smm_mbr_f64);
// per video, behind hist_off: cum, h, bt (the transition max before - cum), the suffix maxima of h, each [T+1][c_max], then
// the frame labels (int32 [T+1])
struct SmmMbrArgs {
    const SmmVideo *videos;
    const int32_t *order;      // [b] wave -> video (most work first)
    const int32_t *n_states;
    const double *gain;        // [total_frames][c_max]
    const double *trans;       // [g][c_max][c_max]  [to][from] (made binary on load)
    const double *init;        // [g][c_max]
    const double *endpen;      // [b][c_max] or null (EOS mode only)
    const int64_t *class_map;  // [g][c_max+1] or null
    double *hist;              // the workspace's history area
    int64_t *spans;            // [b][t_max+1] or null
    int64_t *labels;           // [total_frames] or null
    double *best;              // [b] or null
    double *gain_sum;          // [b] or null
    int32_t *n_segs;           // [b] or null
    int32_t *err;              // sticky error word
    int32_t c_max, t_max, b, no_eos;
};
void smm_launch_mbr(const SmmMbrArgs &a, hipStream_t stream);

// forced alignment to a given transcript (smm_align.hip; with optional entries: smm_align_opt.hip; to a transcript graph:
// smm_align_graph.hip, whose nodes stand where the transcript's entries do).  cum sits class-major [C][T+1] at the video's
// hist_off; the h columns [M][T+1] of video i at hcols + hoff[i], smm_align_opt's running maxima [c_max][T+1] behind them, or
// smm_align_graph's gam columns [M][T+1]
struct SmmAlignArgs {
    const SmmVideo *videos;
    const int32_t *order;      // [b] workgroup -> video (most lattice cells first)
    const int32_t *n_states;
    const double *elp;         // [total_frames][c_max]
    const double *trans;       // [g][c_max][c_max]  [to][from]
    const double *init;        // [g][c_max]
    const double *len;         // [g][k_rows][c_max]
    const double *endpen;      // [b][c_max] or null
    const int64_t *class_map;  // [g][c_max+1] or null
    const int32_t *transcript; // [toff[b]] local state ids (caller's; checked against n_states on load)
    const uint8_t *optional;   // [toff[b]] non-zero: the entry may be left out            (smm_align_opt only)
    const uint32_t *pred_mask; // [8 * toff[b]] bit j of node m's 8 words: j may directly precede m   (smm_align_graph only)
    const uint8_t *node_flags; // [toff[b]] bit 0: may be the first segment, bit 1: the last          (smm_align_graph only)
    const int64_t *toff;       // [b + 1]
    const int64_t *hoff;       // [b] doubles
    double *hist;              // the workspace's history area
    double *hcols;             // behind the plan's workspace
    int64_t *spans;            // [b][t_max+1] or null
    int64_t *labels;           // [total_frames] or null
    double *best;              // [b] or null
    int32_t *n_segs;           // [b] or null
    int32_t *used;             // [toff[b]] or null: 1 for an entry that got a segment   (smm_align_opt, smm_align_graph)
    int32_t *err;              // sticky error word
    int32_t c_max, k_rows, t_max, b;
};
void smm_launch_align(const SmmAlignArgs &a, hipStream_t stream);
void smm_launch_align_opt(const SmmAlignArgs &a, hipStream_t stream);
void smm_launch_align_graph(const SmmAlignArgs &a, hipStream_t stream);

// transcript likelihood and its gradient (smm_align_logz.hip; with optional entries: smm_align_opt_logz.hip).  cum as for the
// alignment.  smm_align_logz: the columns of video i at cols + hoff[i]: h | gam | q, each [M][T+1]; its part of g_len at
// part + poff[i]: [min(k_rows, T + 1)][c_max].  smm_align_opt_logz: the block of video i at cols + hoff[i]: the columns' ranges
// (3 M doubles), then h | gam | q | bh, each [M][T+1], then the running per-class sums [c_max][T+1]; its parts at
// part + poff[i]: g_len [min(k_rows, T + 1)][c_max], g_trans [c_max][c_max], g_init [c_max], then the backward pass's logZ_o
struct SmmAlignLogzArgs {
    const SmmVideo *videos;
    const int32_t *order;      // [b] workgroup -> video (most lattice cells first)
    const int32_t *n_states;
    const double *elp;         // [total_frames][c_max]
    const double *trans;       // [g][c_max][c_max]  [to][from]
    const double *init;        // [g][c_max]
    const double *len;         // [g][k_rows][c_max]
    const double *endpen;      // [b][c_max] or null
    const int32_t *transcript; // [toff[b]] local state ids (caller's; checked against n_states on load)
    const uint8_t *optional;   // [toff[b]] non-zero: the entry may be left out   (smm_align_opt_logz only; null: no entry is optional
                               // and none takes its start posteriors from the entry before it)
    const uint32_t *pred_mask; // [8 * toff[b]] bit j of node m's 8 words: j may directly precede m   (smm_align_graph_logz only)
    const uint8_t *node_flags; // [toff[b]] bit 0: may be the first segment, bit 1: the last          (smm_align_graph_logz only)
    const int64_t *toff;       // [b + 1]
    const int64_t *hoff;       // [b] doubles
    const int64_t *poff;       // [b] doubles
    double *hist;              // the workspace's history area
    double *cols;              // behind the plan's workspace
    double *part;              // behind the columns
    double *logz;              // [b]: the forward launch writes it, the backward launches read it
    const double *grad;        // [b] or null (= 1)                      (backward only, as the five below)
    double *g_elp, *g_trans, *g_init, *g_len;   // smm_logz_bwd_f64's layouts; g_elp zero at launch
    double *p_used;            // [toff[b]] or null                      (smm_align_opt_logz, smm_align_graph_logz)
    double *p_end;             // [toff[b]] or null                      (smm_align_graph_logz only)
    int32_t *err;              // sticky error word
    int32_t c_max, k_rows, b, n_groups;
};
void smm_launch_align_logz_fwd(const SmmAlignLogzArgs &a, hipStream_t stream);
void smm_launch_align_logz_bwd(const SmmAlignLogzArgs &a, hipStream_t stream);
void smm_launch_align_opt_logz_fwd(const SmmAlignLogzArgs &a, hipStream_t stream);
void smm_launch_align_opt_logz_bwd(const SmmAlignLogzArgs &a, hipStream_t stream);
// the g_elp, g_len and reduce kernels of smm_align_opt_logz.hip alone: what follows a backward kernel that left that unit's
// columns, ranges and parts in the workspace (smm_align_graph_logz.hip does, with a null `optional`)
void smm_launch_align_opt_logz_tail(const SmmAlignLogzArgs &a, hipStream_t stream);
// ... over the paths of a transcript graph (smm_align_graph_logz.hip): the block of video i at cols + hoff[i]: the columns'
// ranges (3 M doubles), then h | gam | q | bh, each [M][T+1]; its parts as smm_align_opt_logz's
void smm_launch_align_graph_logz_fwd(const SmmAlignLogzArgs &a, hipStream_t stream);
void smm_launch_align_graph_logz_bwd(const SmmAlignLogzArgs &a, hipStream_t stream);
// ... its first kernel alone: the q and bh columns, the videos' parts of g_trans and g_init and, where asked for, p_used / p_end
void smm_launch_align_graph_logz_bwd_columns(const SmmAlignLogzArgs &a, hipStream_t stream);

// The block of video i at cols + hoff[i]: the columns' ranges in 3 M doubles, then h | gam | q | bh, each [M][T+1].  Its size,
// and from a video's offset and the nodes in front of it the [M][T+1] cells in front of it (smm_align_graph_entropy_bwd.hip keeps
// its scratch blocks in the same order)
#define SMM_GRAPH_HEAD 3           // doubles per node in front of the columns
__host__ __device__ inline size_t smm_graph_block_doubles(int64_t m, int64_t t) { return (size_t)(SMM_GRAPH_HEAD * m + 4 * m * (t + 1)); }
__host__ __device__ inline int64_t smm_graph_cells_before(int64_t hoff, int64_t nodes_before)
{
    return (hoff - SMM_GRAPH_HEAD * nodes_before) / 4;
}

// the second side of a call on two transcript-graph posteriors: q's tables and what its own forward call left
struct SmmAlignSideQ {
    const double *trans;       // [g][c_max][c_max]
    const double *len;         // [g][k_rows][c_max]
    const double *endpen;      // [b][c_max] or null
    const double *logz;        // [b]
    double *hist;              // q's history area: the same plan, so the videos' hist_off serve both
    double *cols;              // q's workspace at the offset of `cols` in p's: the same layout, so hoff serves both (the KL call
                               // only reads the two; the gradient calls' q-side launch of the q / bh kernel writes through them)
};

// the entropy of the transcript-graph posterior (smm_align_graph_entropy.hip): after smm_launch_align_graph_logz_fwd and
// smm_launch_align_graph_logz_bwd_columns on the same workspace -- it reads cum, the h, gam, q and bh columns and the columns'
// ranges, and writes the error word only
struct SmmAlignEntropyArgs {
    SmmAlignLogzArgs g;        // the forward launch's arguments (logz: read; the backward call's fields: unused)
    double *h_out;             // [b]
    double *h_parts;           // [b][3]: end node, span, predecessor; or null
};
void smm_launch_align_graph_entropy(const SmmAlignEntropyArgs &a, hipStream_t stream);

// segment posteriors of given alignments and the nodes' boundary distributions (smm_align_graph_segpost.hip): after
// smm_launch_align_graph_logz_fwd and smm_launch_align_graph_logz_bwd_columns on the same workspace -- it reads cum, the four
// column blocks and the columns' ranges, and writes the error word only
struct SmmAlignSegPostArgs {
    SmmAlignLogzArgs g;        // the forward launch's arguments (logz: read; the backward call's fields: unused)
    const int64_t *class_map;  // [g][c_max+1] or null
    const int64_t *spans_in;   // [n_sets][b][t_max+1] or null
    const int32_t *used_in;    // [n_sets][n_nodes] or null (with spans_in)
    double *seg_logp;          // [n_sets][b][t_max+1] or null
    double *node_logp;         // [n_sets][n_nodes] or null
    double *end_mean, *end_sd, *start_mean, *start_sd;   // [n_nodes] each, or null
    double *node_end_post;     // [n_nodes][t_max+1] or null
    double *node_start_post;   // [n_nodes][t_max+1] or null
    int64_t n_nodes;
    int32_t t_max, n_sets;
};
void smm_launch_align_graph_segpost(const SmmAlignSegPostArgs &a, hipStream_t stream);

// KL(p || q) and the cross-entropy H(p, q) of two transcript-graph posteriors over the same videos and graphs
// (smm_align_graph_kl.hip): after smm_launch_align_graph_logz_fwd per side and smm_launch_align_graph_logz_bwd_columns on p's
// workspace -- of p's it reads what the entropy kernel reads, of q's the h and gam columns and the columns' ranges only, and it
// writes p's error word only
struct SmmAlignKlArgs {
    SmmAlignLogzArgs g;        // p's forward launch's arguments (logz: read; the backward call's fields: unused)
    SmmAlignSideQ q;           // (hist: unused)
    double *kl_out;            // [b]
    double *xent_out;          // [b] or null
    double *kl_parts;          // [b][3]: end node, span, predecessor; or null
};
void smm_launch_align_graph_kl(const SmmAlignKlArgs &a, hipStream_t stream);

// gradients of the entropy, cross-entropy and KL of transcript-graph posteriors with respect to p's tables
// (smm_align_graph_entropy_bwd.hip): after smm_launch_align_graph_logz_fwd and smm_launch_align_graph_logz_bwd_columns per side
// (for the entropy q's pointers are p's) -- of both sides it reads cum, the four column blocks and the columns' ranges; it
// writes the caller's scratch, the gradients and p's error word
struct SmmAlignEntBwdArgs {
    SmmAlignLogzArgs g;        // p's backward launch's arguments (grad: the upstream weights; g_elp zero at launch)
    SmmAlignSideQ q;
    double *value;             // [b] or null: V-
    double *scratch;           // caller's: per video five [M][T+1] blocks, then the videos' parts at pv_base, then q's log Z as the
                               // call uses it [b], then V+ [b]
    int64_t pv_base;           // doubles in front of the parts
    int32_t kl;                // 0: cross-entropy (entropy), 1: KL
};
size_t smm_align_graph_entropy_bwd_part_doubles(int c_max, int k_rows);   // the parts of one video
// ... on the device: g_len [k_rows][c_max], g_trans [c_max][c_max], g_init [c_max], V-, state
__host__ __device__ inline size_t smm_agb_part_doubles(int cm, int k_rows) { return (size_t)k_rows * cm + (size_t)cm * cm + cm + 2; }
// a video's state in its parts: its terms are summed, it contributes nothing (no alignment under p, a NaN, other graphs), or
// its value is not finite (NaN rows, NaN tables for its group)
#define SMM_AGB_RUN 0.0
#define SMM_AGB_SKIP 1.0
#define SMM_AGB_NAN 2.0
void smm_launch_align_graph_entropy_bwd(const SmmAlignEntBwdArgs &a, hipStream_t stream);
// ... its last two kernels alone (g_elp as the running sum of D, the groups' tables): what follows kernels that left D, the
// videos' parts and their states in that unit's scratch layout (smm_align_graph_expected_reward.hip does)
void smm_launch_align_graph_entropy_bwd_tail(const SmmAlignEntBwdArgs &a, hipStream_t stream);
// ... before q's workspace is touched: out[i] = logz_q[i] where the two sides' recorded ranges agree, NaN where they differ
// (g.cols, g.hoff, g.toff, g.logz and cols_q are read)
void smm_launch_align_graph_entropy_bwd_check(const SmmAlignEntBwdArgs &a, const double *logz_q, double *out, hipStream_t stream);

// expected frame- and node-additive reward under the transcript-graph posterior and its gradient with respect to the tables
// (smm_align_graph_expected_reward.hip): after smm_launch_align_graph_logz_fwd and smm_launch_align_graph_logz_bwd_columns on
// the same workspace.  The value launch reads e.g only; the gradient launch uses e as smm_launch_align_graph_entropy_bwd does
// (e.q: p's own pointers; e.kl and e.value unused)
struct SmmAlignExpRewardArgs {
    SmmAlignEntBwdArgs e;
    const double *reward;      // [total_frames][c_max] or null
    const double *node_reward; // [toff[b]] or null
    int64_t *cw_off;           // [b] caller's scratch: the doubles in front of each video's cumW (the prefix kernel writes them)
    double *cumw;              // caller's scratch: per video cumW [C][T+1], (T+1) c_max doubles each
    double *partial;           // caller's scratch: [n_nodes][2] frame part, node part     (value launch)
    double *value;             // [b]                                                      (value launch)
    double *parts;             // [b][2] or null: frame part, node part                    (value launch)
    double *vpm;               // [b][2] or null: V-, V+                                   (gradient launch)
    int64_t n_nodes;
};
void smm_launch_align_graph_expected_reward(const SmmAlignExpRewardArgs &a, hipStream_t stream);
void smm_launch_align_graph_expected_reward_bwd(const SmmAlignExpRewardArgs &a, hipStream_t stream);

// alignments drawn from the transcript-graph posterior (smm_align_graph_sample.hip): after smm_launch_align_graph_logz_fwd on
// the same workspace -- it reads cum, the h and gam columns and the columns' ranges, and writes the error word only
struct SmmAlignSampleArgs {
    SmmAlignLogzArgs g;        // the forward launch's arguments (logz: read; the backward call's fields: unused)
    const int64_t *class_map;  // [g][c_max+1] or null
    int64_t *spans;            // [n_samples][b][t_max+1] or null
    int64_t *labels;           // [n_samples][total_frames] or null
    double *logp;              // [n_samples][b] or null
    int32_t *n_segs;           // [n_samples][b] or null
    int32_t *used;             // [n_samples][n_nodes] or null
    int64_t total_frames, n_nodes;
    uint64_t seed;
    int32_t t_max, n_samples;
};
void smm_launch_align_graph_sample(const SmmAlignSampleArgs &a, hipStream_t stream);

// NICE coupling flow in front of the emission scorer (smm_flow.hip).  A workgroup of four waves owns `strips` x 16 rows and
// carries them through every coupling layer in LDS; `slab_rows` k-rows of a weight matrix are staged through LDS at a time.
struct SmmFlowPlan {
    int32_t strips;            // 16-row MFMA strips per tile: 4, 2 or 1 (the largest whose tile fits the LDS)
    int32_t slab_rows;         // 16, or 8 where nothing else fits
    int32_t keep;              // backward: every coupling layer's active half as it came in is kept in LDS (1) or in the scratch (2)
    size_t keep_floats;        // keep = 2: floats of scratch per workgroup, behind the partials
    int32_t grid;              // workgroups (backward: each owns an fp64 partial of every parameter gradient)
    int32_t n_tiles;
    size_t lds_bytes;
    size_t n_params;           // floats of the packed parameter buffer
};
// false: no tile of this shape fits the LDS (never for the sizes smmdp.h admits); host only
bool smm_flow_plan(int64_t n_rows, int d, int h, int hidden_layers, int couple_layers, bool bwd, SmmFlowPlan *out);
struct SmmFlowArgs {
    const float *x;            // [n_rows][d]
    const float *g_y;          // [n_rows][d]                 (backward)
    const float *params;       // packed (smmdp.h: smm_flow_shape)
    float *out;                // forward: y [n_rows][d]; backward: g_x or null
    double *partials;          // backward: [grid][n_params], zero at launch
    float *keep_global;        // backward, keep = 2: [grid][couple_layers][rows of a tile][d / 2]
    int64_t n_rows, n_params;
    int32_t d, h, hidden_layers, couple_layers, strips, slab_rows, n_tiles, keep;
};
void smm_launch_flow_fwd(const SmmFlowArgs &a, const SmmFlowPlan &p, hipStream_t stream);
void smm_launch_flow_bwd(const SmmFlowArgs &a, const SmmFlowPlan &p, hipStream_t stream);
// g_params[i] = partials[0][i] + partials[1][i] + ... in that order
void smm_launch_flow_reduce(const double *partials, int grid, size_t n_params, double *g_params, hipStream_t stream);

// gradient of the emission scores with respect to the features (smm_flow.hip); rows no video covers are not written
struct SmmEmBwdXArgs {
    const SmmVideo *videos;
    const int32_t *order;    // [b]
    const int32_t *n_states;
    const int32_t *cum;      // [b + 1] chunks of smm_emission_bwd_chunk() frames before each video of `order`
    const float *x;          // [total_frames][d]
    const double *g_elp;     // [total_frames][c_max]
    const double *w;         // [g][d][c_max]
    const double *inv_var;   // [d]
    float *g_x;              // [total_frames][d]
    int32_t d, c_max, b, n_chunks, chunk;   // chunk: smm_emission_bwd_chunk()
};
void smm_launch_emission_bwd_x(const SmmEmBwdXArgs &a, int c_need, hipStream_t stream);
