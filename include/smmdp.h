/*
 * smmdp.h -- C ABI of libsmmdp.so: MI355X (gfx950) semi-Markov decode path.
 *
 * This library replaces, for the `--classifier semimarkov` path of dpfried/action-segmentation,
 * everything between "features are on the device" and "span encoding / frame labels are back":
 *
 *   smm_emission_f64        <- SemiMarkovModule.emission_log_probs / _emission_log_probs_with_means
 *                              (reference src/models/semimarkov/semimarkov_modules.py:324-381)
 *   smm_viterbi_f64/_f32    <- SemiMarkovModule.log_hsmm (modules:416-523) + torch_struct
 *                              SemiMarkovCRF(...).argmax + .struct.from_parts (modules:677-679) + class
 *                              un-mapping (modules:683-691) + semimarkov_utils.spans_to_labels
 *                              (semimarkov_utils.py:51-63) + SemiMarkovModule.trim (modules:532-543)
 *   smm_decode_f32          <- SemiMarkovModule.viterbi end to end (modules:660-696)
 *   smm_logz_f64 / _bwd     <- SemiMarkovCRF(...).partition (modules:657) and its autograd backward
 *                              (reference src/models/semimarkov/semimarkov.py:286)
 *   smm_sample_f64          <- pytorch-struct's SemiMarkovCRF(...).sample (posterior samples; the reference never calls it)
 *   smm_entropy_f64         <- pytorch-struct's SemiMarkovCRF(...).entropy (exact H(y | x) per video; the reference never
 *                              calls it)
 *   smm_segment_posteriors_f64 <- the exact posterior of each segment boundary and of each segment of given segmentations (what
 *                              pytorch-struct's marginals hold per dense edge; the reference never calls them)
 *   smm_kl_f64              <- pytorch-struct's SemiMarkovCRF(...).kl / cross_entropy (exact KL(p || q) and H(p, q) per
 *                              video between two posteriors of one lattice; the reference never calls them)
 *   smm_entropy_bwd_f64 /   <- autograd through pytorch-struct's entropy / kl / cross_entropy (the gradients of the three
 *   smm_kl_bwd_f64             values with respect to p's tables)
 *   smm_expected_reward_f64 / <- the posterior expectation of a frame- and segment-additive reward (expected correct frames,
 *   smm_expected_reward_bwd_f64  expected segment count, expected time in a class) and its gradient with respect to p's tables,
 *                              a Hessian-vector product of log Z (minimum-risk training; the reference has none)
 *   smm_kbest_f64           <- pytorch-struct's SemiMarkovCRF(...).kmax / topk (the k best segmentations; the reference never
 *                              calls it)
 *   smm_mbr_f64             <- minimum-Bayes-risk decode under frame loss: the feasible segmentation with the most expected
 *                              correct frames (the reference has none)
 *   smm_align_f64           <- forced alignment: the best segmentation whose class sequence is a given transcript (the
 *                              reference has none)
 *   smm_align_opt_f64       <- ... with optional transcript entries: the best over every subset of them left out (a CrossTask
 *                              task "bg, step, bg, ..." whose backgrounds or steps may be missing; the reference has none)
 *   smm_align_graph_f64     <- ... to a transcript graph: the best segmentation whose class sequence is a start -> end path of a
 *                              DAG of classes (candidate sets as a trie, alternatives, free order, long skips; the reference
 *                              has none)
 *   smm_align_logz_f64 /    <- transcript likelihood: the log of the sum over every segmentation with a given transcript,
 *   smm_align_logz_bwd_f64     and its gradient (the objective and the E-step of transcript supervision; the reference has none)
 *   smm_align_opt_logz_f64 / <- ... with optional transcript entries: the sum over every alignment, any subset of them left
 *   smm_align_opt_logz_bwd_f64   out, its gradient and each entry's posterior of being used (the reference has none)
 *   smm_align_graph_logz_f64 / <- ... over a transcript graph: the sum over every start -> end path's alignments ("one of these
 *   smm_align_graph_logz_bwd_f64   N transcripts" as a trie), its gradient and the node / end posteriors (the reference has none)
 *   smm_align_graph_sample_f64 <- ... and alignments drawn from that posterior: a path of the graph and its boundaries (pseudo-labels
 *                              for stochastic EM from transcripts, boundary uncertainty; the reference has none)
 *   smm_align_graph_entropy_f64 <- ... and the exact entropy of that posterior: how sure the model is of the alignment, of the
 *                              candidate and of the boundaries (the reference has none)
 *   smm_align_graph_segment_posteriors_f64 <- ... and the exact posterior of each segment of given alignments, with the mean and
 *                              deviation of every node's boundaries (the reference has none)
 *   smm_align_graph_kl_f64    <- ... and the exact KL divergence and cross-entropy between two such posteriors over the same
 *                              videos and graphs: teacher against student, one EM epoch against the next (the reference has none)
 *   smm_align_graph_entropy_bwd_f64 / <- ... and the gradients of those three values with respect to p's tables: entropy
 *   smm_align_graph_kl_bwd_f64   regularisation, distillation of an alignment posterior (the reference has none)
 *   smm_align_graph_expected_reward_f64 / <- ... and the expectation under that posterior of a frame- and node-additive reward
 *   smm_align_graph_expected_reward_bwd_f64  (expected correct frames of an alignment, expected segments, a candidate's posterior)
 *                              and its gradient with respect to the tables (the reference has none)
 *
 * The reference has no FFI: its boundary is the Python call SemiMarkovCRF(scores, lengths) on a dense
 * b x N x K x C x C tensor.  These entry points take the FACTORS of that tensor instead,
 * which is what a maintainer's binding passes (INTEGRATION.md shows the ctypes stub).
 *
 * Conventions
 *   - Plain C, no exceptions; every function returns SMM_OK (0) or a negative smm_status.
 *   - "dev" pointers are HIP device pointers owned by the caller; "host" pointers are small per-video /
 *     per-group metadata arrays in ordinary host memory (the library stages them itself; they may be reused
 *     as soon as the call returns).  Results never depend on earlier calls.  What the library keeps between calls is
 *     listed under "State" below; nothing else is allocated or retained.
 *   - All work is enqueued on `stream` (a hipStream_t passed as void*, NULL = default stream); no call
 *     synchronises.  Distinct streams may be used from distinct threads.
 *   - A "group" is a parameter set (one CrossTask task: its valid classes, transition/init/length tables).
 *     A reference-style batch (corpus.py:613-644: one task, padded) is n_groups = 1, group = NULL,
 *     frame_offset[i] = i * t_max.
 *   - Frames of all videos live on one packed frame axis; video i occupies frames
 *     [frame_offset[i], frame_offset[i] + lengths[i]).
 *   - Tables are fp64, padded to c_max columns: trans[g][to][from] (c_max x c_max), init[g][c_max],
 *     len_scores[g][k_rows][c_max] (row index == segment length, rows 1..k_rows-1 usable; modules:383-398),
 *     class_map[g][c_max + 1] int64: local state -> global class id, entry n_states[g] = EOS id (n_classes).
 *   - Per-video kp[i] = min(K, Tmax of the video's reference batch) reproduces modules:450-452 (NULL: min(k_rows, t_max)).
 *   - endpen[i][c_max] fp64 (dev, nullable): 0 for allowed end states, -1e9 otherwise (modules:462-471).
 *
 * State (all of it released by smm_release_cached_plans(); none of it changes a result)
 *   - resident plans: the staged, immutable metadata of a call whose inputs have been seen twice, in library-owned device
 *     memory (at most 64 MB per process; the entry points that take lengths_host / frame_offset_host stage through it);
 *   - measured times per resident plan of a split smm_decode_f32 ("Plan feedback" below): 16 bytes of pinned host memory
 *     per video and one event per plan;
 *   - one low-priority stream per device for smm_decode_f32's split decode, and pooled events around it;
 *   - the SMM_* tuning switches, read from the environment once, at first use (smm_env_reload() reads them again);
 *   - smm_dp_timing_*: the event pairs of the measurement aid while it is enabled.
 */
#ifndef SMMDP_H
#define SMMDP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum smm_status {
    SMM_OK = 0,
    SMM_ERR_ARG = -1,          /* null pointer / non-positive size / inconsistent metadata */
    SMM_ERR_UNSUPPORTED = -2,  /* shape outside the compiled kernels (c_max > 32, k_rows > 1024) */
    SMM_ERR_WORKSPACE = -3,    /* workspace too small */
    SMM_ERR_HIP = -4,          /* a HIP runtime call failed (smm_last_hip_error() has the code) */
    SMM_ERR_NO_DEVICE = -5     /* no gfx950 device visible */
} smm_status;

#define SMM_MAX_STATES 32
#define SMM_MAX_K_ROWS 1024

/* Shape of one decode call (plain data; passed by pointer). */
typedef struct smm_shape {
    int32_t b;         /* videos */
    int32_t d;         /* feature dim (emission only) */
    int32_t n_groups;  /* parameter groups */
    int32_t c_max;     /* table column stride, >= every n_states[g], <= SMM_MAX_STATES */
    int32_t k_rows;    /* rows of the length table (= --sm_max_span_length, or 2 for the K==1 HMM table) */
    int32_t t_max;     /* max lengths[i] */
    int32_t flags;     /* SMM_SHAPE_* bits, 0 = the reference's default (add_eos=True) */
    int64_t total_frames; /* extent of the packed frame axis (>= every frame_offset[i] + lengths[i]) */
} smm_shape;

/* add_eos=False of the reference (semimarkov_modules.py:494-505, :660): no EOS label is appended.  The DP positions
 * are the frames themselves: segments cover frames 0 .. T-2 and the video closes with a transition into the label of
 * frame T-1, which contributes its emission only (no length score); end penalties do not apply (endpen is ignored).
 * Viterbi: spans[i][T-1] holds that label and no EOS id is written; log Z and its gradient likewise.  lengths[i] >= 2. */
#define SMM_SHAPE_NO_EOS 1
/* smm_logz_f64 only: also run the time-reversed recursion (the backward messages smm_logz_bwd_f64 needs) in the SAME
 * launch, one extra workgroup per video.  The two directions are independent, so a batch that does not fill the GPU
 * gets its gradient's DP for free; pass the same flag to smm_logz_bwd_f64, which then skips its own reversed run. */
#define SMM_SHAPE_LOGZ_BOTH 2
/* Viterbi entry points: never split a video along the time axis ("Long videos" below).  For callers that know their tables
 * carry hard masks (ordering constraints: transitions / initial states / ends at -1e9): a unit that starts in the middle of
 * such a video from "every state equally good" reaches states the masks forbid there, its cuts do not certify, and every
 * split video would be decoded a second time in one piece -- correct as ever, and slower than not splitting. */
#define SMM_SHAPE_NO_TIME_SPLIT 4

const char *smm_strerror(int status);
int smm_last_hip_error(void);
const char *smm_version(void);
/* number of visible gfx950 devices (0 when none; never initialises a context on failure) */
int smm_device_count(void);

/* Bytes of device workspace any entry point below needs for this shape (lengths: host array [b]).
 * Returns 0 on invalid arguments.  The workspace is scratch: its contents are undefined after a call,
 * except between smm_logz_f64 and smm_logz_bwd_f64 / smm_sample_f64 / smm_entropy_f64 / smm_segment_posteriors_f64 / smm_kl_f64,
 * and between a transcript likelihood call and the calls its comment names (smm_align_graph_logz_f64:
 * smm_align_graph_logz_bwd_f64, smm_align_graph_sample_f64, smm_align_graph_entropy_f64,
 * smm_align_graph_segment_posteriors_f64 and smm_align_graph_kl_f64, in any order). */
size_t smm_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host);

/* Byte offset, inside the workspace, of the int32 error word the kernels set.  1: a NaN / inf-inf reached the DP of
 * some video and its decode stopped early.  It is cleared at the start of every call.  Returns 0 on invalid shape.
 * (The int32 word behind it is always 0: rounds 1-3 counted the time-outs of multi-workgroup "gangs" there, which no
 * longer exist; the third and fourth words are diagnostics of the Viterbi kernel's BAND mode: sources pushed into
 * band 0, delayed band-blocks evaluated; the fifth and sixth count the videos a Viterbi call decoded as several units
 * along the time axis and, of those, the ones it decoded again in one piece because a cut could not be certified or a
 * decision was closer than rounding can tell -- the outputs are the one-piece decode's either way, see "Long videos"
 * below.) */
size_t smm_error_word_offset(const smm_shape *shape);

/*
 * Long videos (Viterbi entry points, EOS mode, span limit > 64).  The decode of one video is one serial chain over its
 * frames; a launch whose CU-time is shorter than its longest video cuts that video along the TIME axis into units that
 * run on different CUs, each warmed up on the frames in front of its own part, and stitches them: the cuts are certified
 * against each other, every decision of the back-trace has to be clear of rounding, the best score is re-evaluated along
 * the path in the one-piece decode's association -- and a video that fails any of it is decoded again in one piece by the
 * same call (csrc/smm_chunk.hip).  spans / labels / best / n_segs are those of the one-piece decode, bit for bit; the
 * workspace bound of smm_workspace_bytes covers it.  SMM_CHUNK=0 in the environment switches the splitting off.
 */

/* The plan "Long videos" would make for this launch on a GPU of n_cu compute units -- host logic only, no device needed (tests;
 * capacity planning): for every unit of every video that would be split, in time order per video: its video, its first
 * position, its length in positions, and how many of those it runs in front of its own part (0 for a video's first unit).
 * Arrays of `cap` entries (any may be NULL); returns the number of units (may exceed cap), 0 when nothing would be split,
 * or a negative smm_status.  group / kp may be NULL as in the decode entry points. */
int smm_time_split_plan(const smm_shape *shape, const int64_t *lengths_host, const int32_t *group_host, const int32_t *kp_host,
                        const int32_t *n_states_host, int n_cu, int32_t *unit_video, int32_t *unit_first, int32_t *unit_len,
                        int32_t *unit_overlap, int cap);

/*
 * Measurement aid (bench.py's roofline; not part of the reference's interface): while enabled, every launch of the
 * Viterbi DP kernel made by smm_viterbi_* / smm_decode_f32 is bracketed by a pair of HIP events on the stream it is
 * launched on (smm_decode_f32 may launch the kernel twice per call, on two streams: smmdp.h / DESIGN.md "split decode").
 * smm_dp_timing_read waits for the recorded launches, writes their durations in milliseconds (launch order, at most
 * `cap`) and forgets them; it returns the number of launches recorded since the last read (which may exceed cap).
 * Not to be enabled around a stream capture.  The two event records cost a few microseconds per launch.
 */
void smm_dp_timing_enable(int on);
int smm_dp_timing_read(float *ms, int cap);
/* as smm_dp_timing_read, plus which launch each one was: tags[i] = 0 the only DP launch of its call, 1 the launch of the
 * critical (longest) videos of a split smm_decode_f32 on the caller's stream, 2 the rest of that call on the library's
 * second stream, 3 the <= 16-state videos of a launch part that holds more videos than the GPU has CUs, decoded in four-wave
 * workgroups (two per CU) on a side stream beside the launch of tag 0 / 2 (either array may be NULL) */
int smm_dp_timing_read_tagged(float *ms, int32_t *tags, int cap);

/*
 * Cost model of the shipped Viterbi kernel (not part of the reference's interface): nanoseconds per frame of ONE video
 * of `n_states` states decoded with segment lengths beyond 512 (BAND mode: the time of its serial chain, which hardly
 * depends on the span limit), as measured on an MI355X with this library's kernels (the constants sit next
 * to the kernel's dispatch and move with it).  ONE place for the number that two host-side decisions need: the split of
 * smm_decode_f32 (how much shorter than the launch's longest video a video must be to start behind the emission pass
 * of the whole corpus) and the balancing of video shards over ranks (batching.batch_cost).  Returns 0 for n_states
 * outside 1..32.
 */
double smm_band_frame_ns(int n_states);

/*
 * Library state (see "State" above).  smm_release_cached_plans frees every resident plan (all devices), the split
 * decode's second streams and all pooled events, and returns the device bytes it gave back.  The caller's promise: no
 * libsmmdp call is in flight on any stream, and no hipGraph captured from a call will be replayed afterwards (a captured
 * call points at its plan's buffer).  smm_cached_plan_bytes: device bytes currently held by resident plans, plus the
 * pinned host bytes of their measured times (both are given back, and counted in smm_release_cached_plans' result).
 * smm_env_reload: read the SMM_* tuning switches from the environment again (they are read once, at first use:
 * SMM_SPEC, SMM_NO_SPLIT, SMM_SPLIT_MIN_US / _NS / _MARGIN, SMM_PLAN_CACHE, SMM_PLAN_FEEDBACK, SMM_NO_BT_WINDOW, SMM_FIT_GRID, SMM_SMALL_WG,
 * SMM_CHUNK, SMM_CHUNK_P / _WC / _LMIN, SMM_VERBOSE --
 * none of them changes a result; switches that do exist only in -DSMM_DEV builds of the library).
 */
size_t smm_release_cached_plans(void);
size_t smm_cached_plan_bytes(void);
void smm_env_reload(void);

/*
 * Plan feedback (smm_decode_f32; not part of the reference's interface).  A split decode runs the launch's slowest videos
 * first, on the caller's stream, and everything else beside them.  Which videos are the slowest the library first takes
 * from a model of (frames, states); for a RESIDENT plan -- a launch it has seen twice and will see again -- it then measures:
 * the DP workgroups of a call that runs from (or admits) such a plan write their start and end, ticks of the 100 MHz wall
 * clock, into pinned host memory the library owns, the call records an event behind its last work, and a later call on the
 * plan that finds the event complete (it is queried, never waited for) replays the step from the measured times and, where
 * that ends at least 2 % sooner, moves videos between the two parts and re-orders them -- at most 4 times per plan.  The
 * plan's new metadata goes into a fresh buffer and the old one stays valid until smm_release_cached_plans, so a call in
 * flight and a captured graph are never touched; under stream capture nothing is measured and nothing re-planned; plans
 * with videos split in time or a four-wave tail are left alone.  Results do not change: every video is decoded by the same
 * kernel on the same inputs, only who starts when differs.  SMM_PLAN_FEEDBACK=0 switches it off (2: re-plan after the
 * first complete measurement whatever the predicted gain -- tests).
 *
 * smm_plan_feedback_info: what feedback has done to the plan the LAST smm_decode_f32 call of the calling thread ran from (all
 * zero when it ran from none, or since smm_release_cached_plans).  The pointers stay valid until smm_release_cached_plans.
 */
typedef struct smm_plan_feedback_info_t {
    int32_t n_replans;           /* times the plan has been re-planned */
    int32_t n1_before, n1_after; /* videos of the first part: as first planned, and now */
    int32_t n_videos;
    double end_before_us;        /* replayed end of the step under the first plan, from the first measurement */
    double end_after_us;         /* ... under the current plan: as predicted at the last re-plan, or as replayed from a later measurement */
    const uint64_t *stamps;      /* [n_videos][2] start and end of each video's workgroup, 100 MHz ticks: the measurement the last
                                    evaluation was made from (NULL: none yet) */
    const int32_t *order;        /* [n_videos] the plan's launch order: the first n1_after are the first part */
} smm_plan_feedback_info_t;
int smm_plan_feedback_info(smm_plan_feedback_info_t *out);

/* The planner alone, on the host (tests): measured times dur_us[b] and frames[b] by video, the current plan (cur_order[b], its
 * first cur_n1 videos the first part), the GPU's CU count and the emission pass's time em_us -> the plan feedback would make
 * (order_out[b], *n1_out) and the replayed ends of both; force != 0: the best plan of the planner's own form even where the
 * current one replays no later.  Returns 1 when the plan changes, 0 when it stays, or a negative smm_status. */
int smm_plan_feedback_plan(int b, int n_cu, double em_us, const double *dur_us, const int32_t *frames, const int32_t *cur_order,
                           int cur_n1, int force, int32_t *order_out, int32_t *n1_out, double *end_current_us,
                           double *end_chosen_us);

/*
 * Emission scorer.  elp[t][c] = cst[g][c] + sum_d x[t][d]*w[g][c][d] - 0.5*sum_d x[t][d]^2*inv_var[d] (+ cons[t][c])
 * which is the diagonal-Gaussian log density of modules:324-381 with w = mu/sigma^2,
 * cst = -0.5*sum mu^2/sigma^2 - sum log sigma - D/2 log 2pi.
 *   x        dev fp32 [total_frames][d]
 *   w        dev fp64 [n_groups][d][c_max]  (feature-major, so one frame step reads one contiguous row);
 *   cst      dev fp64 [n_groups][c_max];  inv_var dev fp64 [d]
 *   cons     dev fp32 [total_frames][c_max] or NULL (narration constraints, modules:379-380)
 *   elp64    dev fp64 [total_frames][c_max] or NULL   (frame-major, reference layout)
 *   elp32    dev fp32 [total_frames][c_max] or NULL   (what `return_elp=True` hands back)
 */
int smm_emission_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                     const int32_t *group_host, const int32_t *n_states_host,
                     const float *x, const double *w, const double *cst, const double *inv_var, const float *cons,
                     double *elp64, float *elp32, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Chain rule through the emission scorer (training): with g_elp = dL/d elp (smm_logz_bwd_f64's output),
 *   g_w[g][c][d] = sum_t x[t][d] g_elp[t][c]      g_cst[g][c] = sum_t g_elp[t][c]
 *   g_inv_var[d] = -0.5 sum_t x[t][d]^2 sum_c g_elp[t][c]              (t over the frames of the videos of group g)
 * -- what autograd does behind emission_log_probs (modules:324-381) in the reference's loss.backward()
 * (src/models/semimarkov/semimarkov.py:286).  Outputs are overwritten.
 *   g_w        dev fp64 [n_groups][c_max][d]   CLASS-major (the layout of the reference's gaussian_means; the
 *              transpose of smm_emission_f64's w)
 *   g_cst      dev fp64 [n_groups][c_max];   g_inv_var  dev fp64 [d]
 * Sums leave the workgroups through fp64 atomics: the last bits depend on the order of arrival.
 */
int smm_emission_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                         const int32_t *group_host, const int32_t *n_states_host,
                         const float *x, const double *g_elp, double *g_w, double *g_cst, double *g_inv_var,
                         void *workspace, size_t workspace_bytes, void *stream);

/*
 * The rest of that chain rule, the gradient with respect to the features (what a feature projection in front of the scorer
 * trains on; smm_flow_bwd_f32 reads it as g_y):
 *   g_x[t][d] = sum_c g_elp[t][c] w[g][d][c] - x[t][d] inv_var[d] sum_c g_elp[t][c]        (g the group of the frame's video)
 * computed in fp64 and rounded once.  w and inv_var are smm_emission_f64's (feature-major w).  Rows of g_x that no video covers
 * are 0.  One pass over x and g_elp, no atomics: two runs give the same bits.
 *   g_x        dev fp32 [total_frames][d]   (overwritten)
 */
int smm_emission_bwd_x_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                           const int32_t *group_host, const int32_t *n_states_host,
                           const float *x, const double *g_elp, const double *w, const double *inv_var, float *g_x,
                           void *workspace, size_t workspace_bytes, void *stream);

/*
 * Feature projection: the NICE additive coupling flow of the reference's --sm_feature_projection (src/models/flow.py,
 * NICETrans without --flow_scale), applied to every row of x on its own: y = flow(x), log det = 0.
 *
 * Coupling layer i (0-based) splits a row into halves (h1, h2) of d/2.  For even i the passive half is h1 and the active half h2,
 * for odd i the other way round.  The passive half is copied; the active half becomes active + t_i(passive), where t_i is a
 * ReLU MLP: in_layer (d/2 -> hidden_units), hidden_layers layers hidden_units -> hidden_units, out_layer (hidden_units -> d/2),
 * with ReLU behind every layer but the last.  Everything is fp32; every dot product is a fused-multiply-add chain in ascending
 * input index that starts from the bias, so a row's result does not depend on n_rows or on the row's place.
 *
 * params: ONE packed fp32 device buffer.  For coupling layer 0, 1, ... in turn: for its linear layers in_layer, cell0, cell1, ...,
 * out_layer in turn: the weight, then the bias.  A weight is stored INPUT-major, [in_features][out_features] (the transpose of
 * torch.nn.Linear.weight), unpadded; a bias is [out_features].  With dh = d/2, H = hidden_units, L = hidden_layers the buffer holds
 * couple_layers * (dh*H + H + L*(H*H + H) + H*dh + dh) floats.  smm_flow_bwd_f32 returns the gradients in the same layout, fp64.
 *
 * Supported: d even, 2 <= d <= 512; 1 <= hidden_units <= 256; 0 <= hidden_layers <= 4; 1 <= couple_layers <= 16; n_rows >= 1.
 * Anything else is SMM_ERR_UNSUPPORTED (an odd d, n_rows < 1 or a NULL shape: SMM_ERR_ARG), a NULL x / params / y / g_y /
 * g_params / scratch SMM_ERR_ARG, a short scratch SMM_ERR_WORKSPACE -- all before a device is touched.
 *
 * smm_flow_f32:      x dev fp32 [n_rows][d] -> y dev fp32 [n_rows][d] (y may be x).  The tile lives on chip, so the call needs no
 *                    scratch today: smm_flow_scratch_bytes is 0 and scratch may be NULL; a caller that passes what the query
 *                    returns stays correct if that changes.
 * smm_flow_bwd_f32:  x and g_y = dL/dy (dev fp32 [n_rows][d]) -> g_params dev fp64 (packed layout, overwritten) and, when g_x is
 *                    not NULL, g_x = dL/dx dev fp32 [n_rows][d].  Activations are recomputed, nothing is kept from the forward
 *                    call.  Products are fp32 within a tile of rows; sums across tiles are fp64, per workgroup, added in a fixed
 *                    order: two runs give the same bits.  scratch: smm_flow_bwd_scratch_bytes (0 for an invalid shape): the
 *                    partials and, at the sizes whose tile leaves no room for them in LDS, each coupling layer's input half of
 *                    the tiles in flight; its contents are undefined after the call.
 * Neither call synchronises or allocates; both run on `stream` and can be captured into a hipGraph.
 */
typedef struct smm_flow_shape {
    int64_t n_rows;
    int32_t d;
    int32_t hidden_units;
    int32_t hidden_layers;
    int32_t couple_layers;
} smm_flow_shape;
size_t smm_flow_scratch_bytes(const smm_flow_shape *shape);
size_t smm_flow_bwd_scratch_bytes(const smm_flow_shape *shape);
int smm_flow_f32(const smm_flow_shape *shape, const float *x, const float *params, float *y,
                 void *scratch, size_t scratch_bytes, void *stream);
int smm_flow_bwd_f32(const smm_flow_shape *shape, const float *x, const float *g_y, const float *params,
                     double *g_params, float *g_x, void *scratch, size_t scratch_bytes, void *stream);

/*
 * Viterbi decode on emission scores (fp64 path).
 *   elp       dev fp64 [total_frames][c_max]
 *   spans     dev int64 [b][t_max + 1]  span encoding of modules:679-691: global class id at each span start,
 *             -1 continuation, EOS id at position lengths[i], -1 after it           (nullable)
 *   labels    dev int64 [total_frames]  per-frame global class ids (spans_to_labels + trim)   (nullable)
 *   best      dev fp64 [b] Viterbi score (nullable);  n_segs dev int32 [b] (nullable)
 */
int smm_viterbi_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                    const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                    const double *elp, const double *trans, const double *init, const double *len_scores,
                    const double *endpen, const int64_t *class_map,
                    int64_t *spans, int64_t *labels, double *best, int32_t *n_segs,
                    void *workspace, size_t workspace_bytes, void *stream);

/* Same with the reference's dtypes at the boundary: fp32 elp [total_frames][c_max] and fp32 tables
 * (log_hsmm's inputs, modules:416-417); converted to fp64 on load, then the same DP. */
int smm_viterbi_f32(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                    const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                    const float *elp, const float *trans, const float *init, const float *len_scores,
                    const float *endpen, const int64_t *class_map,
                    int64_t *spans, int64_t *labels, double *best, int32_t *n_segs,
                    void *workspace, size_t workspace_bytes, void *stream);

/* Features -> decode in one call (emission kernel + DP kernel on `stream`); elp32 nullable. */
int smm_decode_f32(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                   const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                   const float *x, const double *w, const double *cst, const double *inv_var, const float *cons,
                   const double *trans, const double *init, const double *len_scores,
                   const double *endpen, const int64_t *class_map,
                   int64_t *spans, int64_t *labels, double *best, int32_t *n_segs, float *elp32,
                   void *workspace, size_t workspace_bytes, void *stream);

/*
 * Log-partition (LogSemiring forward) and its backward.
 *   logz   dev fp64 [b]
 *   bwd:   grad_logz dev fp64 [b] (upstream, NULL = ones), outputs g_elp dev fp64 [total_frames][c_max],
 *          g_trans dev fp64 [n_groups][c_max][c_max], g_init [n_groups][c_max], g_len [n_groups][k_rows][c_max]
 *          (all overwritten).  The workspace written by smm_logz_f64 must be passed unchanged to smm_logz_bwd_f64.
 */
int smm_logz_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                 const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                 const double *elp, const double *trans, const double *init, const double *len_scores,
                 const double *endpen, double *logz, void *workspace, size_t workspace_bytes, void *stream);

int smm_logz_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                     const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                     const double *elp, const double *trans, const double *init, const double *len_scores,
                     const double *endpen, const double *logz, const double *grad_logz,
                     double *g_elp, double *g_trans, double *g_init, double *g_len,
                     void *workspace, size_t workspace_bytes, void *stream);

/*
 * Segmentations drawn from the posterior p(y | x) whose normaliser smm_logz_f64 returns (forward filtering, backward
 * sampling on the forward histories; csrc/smm_sample.hip).  Must follow smm_logz_f64 on the same shape, tables and workspace
 * (with or without SMM_SHAPE_LOGZ_BOTH); logz = that call's output.  One walk per (video, sample); the random numbers are
 * Philox4x32-10 keyed by `seed`, one stream per (video, sample): sample j of a call does not depend on n_samples.
 *   spans_out   dev int64 [n_samples][b][t_max + 1]  the Viterbi entry points' span encoding (class map applied)   (nullable)
 *   labels_out  dev int64 [n_samples][total_frames]  per-frame global class ids; frames no video covers are not written
 *                                                                                                                 (nullable)
 *   logp_out    dev fp64 [n_samples][b]  exact log p(y | x) of each sample: its score summed in fp64 from the tables
 *               and elp, minus logz                                                                               (nullable)
 * SMM_ERR_ARG when n_samples <= 0 or every output is NULL.  The error word is set (and that sample's logp is NaN) when a
 * decision has no candidate of finite weight (NaN inputs, or log Z = -inf).
 */
int smm_sample_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                   const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                   const double *elp, const double *trans, const double *init, const double *len_scores,
                   const double *endpen, const int64_t *class_map, const double *logz, int32_t n_samples, uint64_t seed,
                   int64_t *spans_out, int64_t *labels_out, double *logp_out,
                   void *workspace, size_t workspace_bytes, void *stream);

/*
 * Exact entropy H(y | x) = -sum_y p(y | x) log p(y | x) of each video's segmentation posterior, in nats (csrc/smm_entropy.hip:
 * the chain rule over the decisions of smm_sample_f64's backward walk, every term >= 0, so the value keeps its relative
 * accuracy as H -> 0).  Must follow smm_logz_f64 on the same shape, tables and workspace; logz = that call's output.  Without
 * SMM_SHAPE_LOGZ_BOTH the call runs the time-reversed recursion itself (as smm_logz_bwd_f64 does); with it, smm_logz_f64 has.
 * The forward and backward histories are left as they were (smm_sample_f64 / smm_logz_bwd_f64 may follow); the per-video
 * partial sums are reduced in a fixed order, so the result is bit-identical run to run.  Gradient: smm_entropy_bwd_f64.
 *   entropy_out  dev fp64 [b]
 * SMM_ERR_ARG when entropy_out or a required input (elp, trans, init, len_scores, logz) is NULL, before anything is staged.
 * The error word is set (and that video's value is NaN) when log Z is not finite, a NaN reached the histories, or a node of
 * non-zero probability has no candidate of finite weight.
 */
int smm_entropy_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                    const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                    const double *elp, const double *trans, const double *init, const double *len_scores,
                    const double *endpen, const double *logz, double *entropy_out,
                    void *workspace, size_t workspace_bytes, void *stream);

/*
 * Exact posterior of each segment boundary and of each segment of given segmentations under p(y | x) (csrc/smm_segpost.hip:
 * gathers over the two histories, no recursion).  Call order as smm_entropy_f64: it must follow smm_logz_f64 on the same shape,
 * tables and workspace; without SMM_SHAPE_LOGZ_BOTH the call runs the time-reversed recursion itself; the histories are left as
 * they were (smm_sample_f64 / smm_entropy_f64 / smm_logz_bwd_f64 may follow, and give the bits they give without this call).
 * It has no size query of its own: the workspace is smm_workspace_bytes'.  T below is the number of DP positions of a video,
 * lengths[i] with EOS and lengths[i] - 1 under SMM_SHAPE_NO_EOS; frame f of video i is row frame_offset[i] + f.
 *   class_map   dev int64 [n_groups][c_max + 1], as in smm_sample_f64: the global ids spans_in is written in     (nullable: local ids)
 *   spans_in    dev int64 [n_sets][b][t_max + 1]  segmentations in the Viterbi entry points' span encoding, class map applied,
 *               as smm_viterbi_f64 / smm_kbest_f64 / smm_sample_f64 / smm_mbr_f64 write them                      (nullable)
 *   n_sets      segmentations per video in spans_in (ignored without spans_in)
 *   start_post  dev fp64 [total_frames][c_max]  P(a span of class c starts at frame f)                            (nullable)
 *   end_post    dev fp64 [total_frames][c_max]  P(a span of class c has frame f as its last frame)                (nullable)
 *   bnd_post    dev fp64 [total_frames]         sum over c of start_post, in index order: P(a span starts at f); 1 at frame 0
 *               up to rounding                                                                                    (nullable)
 *   seg_logp    dev fp64 [n_sets][b][t_max + 1] laid out like spans_in (and it needs spans_in): at every span start s < T the
 *               log posterior that exactly this span -- class, start, end = the next span start -- is part of y; 0.0 at the EOS
 *               position; -inf at continuations and past the video                                                (nullable)
 * Columns c >= n_states and frames no video covers are 0.0 in the three dense outputs.  Under SMM_SHAPE_NO_EOS the closing label
 * of frame T counts as a one-frame span of its class: its entry in the dense outputs and in seg_logp is P(closing label = c).
 * A span gets -inf, without an error, when it is longer than kp - 1 frames, when its class is not in the video's class set, or
 * when its posterior is 0.  A video whose log Z is -inf or NaN gets NaN in every probability (seg_logp: at its span starts) and
 * sets the error word; a NaN that reached the histories does the same in the entries it reaches.  No atomics but the error word
 * and no sum across workgroups: the outputs are bit-identical run to run.
 * SMM_ERR_ARG, before anything is staged, when a required input (elp, trans, init, len_scores, logz) is NULL, when every output
 * is NULL, when seg_logp is given without spans_in, or when spans_in is given with n_sets <= 0.
 */
int smm_segment_posteriors_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                               const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                               const double *elp, const double *trans, const double *init, const double *len_scores,
                               const double *endpen, const int64_t *class_map, const double *logz,
                               const int64_t *spans_in, int32_t n_sets,
                               double *start_post, double *end_post, double *bnd_post, double *seg_logp,
                               void *workspace, size_t workspace_bytes, void *stream);

/*
 * Exact KL divergence KL(p || q) = sum_y p(y | x) log(p(y | x) / q(y | x)) and cross-entropy H(p, q) = H(p) + KL(p || q) between
 * two segmentation posteriors of the same lattice (same shape, lengths, frame offsets, groups, kp, state counts; other tables),
 * in nats (csrc/smm_kl.hip: the chain rule of relative entropy over the decisions of smm_sample_f64's backward walk, every term
 * >= 0).  ws_p must follow smm_logz_f64 on this shape with p's tables, ws_q smm_logz_f64 on this shape with q's; logz_p / logz_q
 * are their outputs.  Without SMM_SHAPE_LOGZ_BOTH the call runs p's time-reversed recursion itself (as smm_entropy_f64 does);
 * with it, p's smm_logz_f64 has.  q needs only its forward histories, and ws_q is not written.  The value is exactly 0.0 when
 * p's and q's inputs are bit-identical; the per-video partial sums are reduced in a fixed order (bit-identical run to run).
 * xent_out of p with itself is smm_entropy_f64's value.  Gradient: smm_kl_bwd_f64.
 *   kl_out    dev fp64 [b]
 *   xent_out  dev fp64 [b] or NULL
 * +inf (no error) when q gives probability 0 to a segmentation p does not (a true -inf on q's side only, or log Z_q = -inf).
 * SMM_ERR_ARG when kl_out, a required input (elp, trans, init, len_scores, logz of either side) or ws_q is NULL, before
 * anything is staged; SMM_ERR_WORKSPACE when either workspace is shorter than smm_workspace_bytes.  The error word (in ws_p) is
 * set, and that video's values are NaN, when log Z_p is not finite, a NaN reached either side's histories or tables, or a node
 * of non-zero p-probability has no candidate of finite p-weight.
 */
int smm_kl_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
               const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
               const double *elp_p, const double *trans_p, const double *init_p, const double *len_p,
               const double *endpen_p, const double *logz_p, void *ws_p, size_t ws_p_bytes,
               const double *elp_q, const double *trans_q, const double *init_q, const double *len_q,
               const double *endpen_q, const double *logz_q, void *ws_q, size_t ws_q_bytes,
               double *kl_out, double *xent_out, void *stream);

/*
 * Gradients of the entropy, the cross-entropy and the KL divergence (csrc/smm_entropy_bwd.hip): d sum_i grad_out[i] V_i with
 * respect to p's tables, V = H(p) (smm_entropy_bwd_f64) or H(p, q) / KL(p || q) (smm_kl_bwd_f64, `mode`).  The covariance
 * -Cov_p(s_q, phi) (KL: Cov_p(s_p - s_q, phi)) of each occurrence is p(o) times its deviation, assembled from the prefix and
 * suffix values eta- and eta+ of the chain rule over the sampler's decisions (two serial passes per video, one per direction),
 * so every local term is >= 0 and nothing of the size of the scores cancels.  q's tables get no gradient here: it is
 * mu_q - mu_p, two smm_logz_bwd_f64 calls.  Sums run in a fixed order: bit-identical run to run.  KL of bit-identical sides:
 * exactly 0.0.
 *   grad_out   dev fp64 [b] upstream gradient (NULL = ones)
 *   g_elp, g_trans, g_init, g_len   smm_logz_bwd_f64's outputs and layouts (overwritten; padded rows and columns 0)
 *   value_out  dev fp64 [b][2] or NULL: V by the two decompositions (eta- at the sampler's final decision, eta+ at the initial
 *              class); both are the value smm_entropy_f64 / smm_kl_f64 returns, up to rounding
 *   scratch    dev, smm_entropy_bwd_scratch_bytes: the etas (4 c_max (T+1) doubles per video) and the per-video sums; its contents
 *              are undefined after the call.  smm_workspace_bytes does not change.
 * Inputs as smm_entropy_f64 / smm_kl_f64 (ws_p after smm_logz_f64 with p's tables, ws_q with q's).  Without SMM_SHAPE_LOGZ_BOTH
 * the call runs the time-reversed recursions itself (smm_kl_bwd_f64: of both sides; ws_q is written); with it, both sides'
 * smm_logz_f64 have.  A video whose value is +inf or NaN gets NaN rows in g_elp, and its group's tables are NaN; a NaN value also
 * sets the error word (in p's workspace).  SMM_ERR_ARG for a NULL output, table, logz or scratch, or a mode other than the two
 * below, before anything is staged; SMM_ERR_WORKSPACE for a short scratch or q workspace.
 */
#define SMM_KL_BWD_CROSS_ENTROPY 0
#define SMM_KL_BWD_KL 1
/* host only; 0 on invalid arguments (those of smm_workspace_bytes, c_max or k_rows too large) */
size_t smm_entropy_bwd_scratch_bytes(const smm_shape *shape, const int64_t *lengths_host);
int smm_entropy_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                        const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                        const double *elp, const double *trans, const double *init, const double *len_scores,
                        const double *endpen, const double *logz, const double *grad_out,
                        double *g_elp, double *g_trans, double *g_init, double *g_len, double *value_out,
                        void *scratch, size_t scratch_bytes, void *workspace, size_t workspace_bytes, void *stream);
int smm_kl_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                   const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                   const double *elp_p, const double *trans_p, const double *init_p, const double *len_p,
                   const double *endpen_p, const double *logz_p, void *ws_p, size_t ws_p_bytes,
                   const double *elp_q, const double *trans_q, const double *init_q, const double *len_q,
                   const double *endpen_q, const double *logz_q, void *ws_q, size_t ws_q_bytes, int32_t mode,
                   const double *grad_out, double *g_elp, double *g_trans, double *g_init, double *g_len, double *value_out,
                   void *scratch, size_t scratch_bytes, void *stream);

/*
 * Posterior expectation of a reward that is additive over frames and segments, and its gradient with respect to p's tables
 * (csrc/smm_expected_reward.hip):
 *   R(y) = sum over the spans (s, k, c) of y of ( seg_reward[c] + sum_{t = s .. s+k-1} reward[t][c] ),   V = E_{p(y | x)}[ R(y) ]
 * reward = onehot(labels) makes V the expected number of correct frames (smm_mbr_f64 decodes for it, this trains for it),
 * seg_reward = 1 the expected number of segments, reward[:, c] = 1 the expected time spent in class c.  The value gathers over
 * the two histories (<reward, frame posteriors> + <seg_reward, span-start posteriors>, no recursion).  The gradient
 * dV / d theta_o = Cov_p(R, phi_o) is a Hessian-vector product of log Z: each occurrence's probability times
 * r(o) + eta-(S_o) + eta+(E_o) - V, from the prefix and suffix expectations eta- and eta+ over the sampler's decisions (two serial
 * passes per video, one per direction; smm_entropy_bwd_f64's scheme with one side and no logarithms).  Sums run in a fixed
 * order: value and gradient are bit-identical run to run.  Under SMM_SHAPE_NO_EOS the closing label `to` of frame T counts as a
 * one-frame span, as in smm_segment_posteriors_f64: it carries reward[T][to] + seg_reward[to].
 * Call order and workspace as smm_entropy_f64 / smm_entropy_bwd_f64: the call must follow smm_logz_f64 on the same shape, tables
 * and workspace; without SMM_SHAPE_LOGZ_BOTH it runs the time-reversed recursion itself; the histories are left as they were
 * (the scratch rows behind them are written: smm_logz_bwd_f64's and smm_entropy_f64's, which rewrite them, may follow).
 *   reward      dev fp64 [total_frames][c_max], local states as columns                                        (nullable)
 *   seg_reward  dev fp64 [n_groups][c_max]                                                                    (nullable)
 *   value_out   smm_expected_reward_f64: dev fp64 [b], V
 *               smm_expected_reward_bwd_f64: dev fp64 [b][2] or NULL: V by the two decompositions, V- at the sampler's final
 *               decision and V+ at the initial class; both are smm_expected_reward_f64's value up to rounding
 *   parts_out   dev fp64 [b][2] or NULL: the frame part <reward, frame posteriors> and the segment part of V
 *   grad_out    dev fp64 [b] upstream gradient (NULL = ones)
 *   g_elp, g_trans, g_init, g_len   smm_logz_bwd_f64's outputs and layouts (overwritten; padded rows and columns 0)
 *   scratch     dev, smm_expected_reward_bwd_scratch_bytes; its contents are undefined after the call.  smm_workspace_bytes does
 *               not change.
 * Columns c >= n_states and frames no video covers are ignored in both rewards.  A masked potential has p(o) = 0 and
 * contributes 0 to the value and gets gradient 0.  The rewards get no gradient here (dV / d reward is the frame posterior,
 * smm_logz_bwd_f64's g_elp; dV / d seg_reward the span-start posterior, smm_segment_posteriors_f64's start_post).
 * A video whose log Z is not finite, or with a non-finite reward in a covered entry (or in its group's seg_reward), gets NaN:
 * its value, its g_elp rows and its group's tables; the error word is set.
 * Accuracy: a span's frame reward is a difference of prefix sums of `reward`, so it carries the rounding of sum_t |reward[t][c]|
 * in fp64: rewards are meant to be O(1) per frame.
 * SMM_ERR_ARG, before anything is staged, when a required input (elp, trans, init, len_scores, logz) or output (value_out of the
 * value call; g_elp, g_trans, g_init, g_len) is NULL, when both reward and seg_reward are NULL, or when scratch is NULL;
 * SMM_ERR_WORKSPACE for a short workspace or scratch.
 */
/* host only; 0 on invalid arguments (those of smm_entropy_bwd_scratch_bytes) */
size_t smm_expected_reward_bwd_scratch_bytes(const smm_shape *shape, const int64_t *lengths_host);
int smm_expected_reward_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                            const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                            const double *elp, const double *trans, const double *init, const double *len_scores,
                            const double *endpen, const double *logz, const double *reward, const double *seg_reward,
                            double *value_out, double *parts_out,
                            void *workspace, size_t workspace_bytes, void *stream);
int smm_expected_reward_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                const double *elp, const double *trans, const double *init, const double *len_scores,
                                const double *endpen, const double *logz, const double *reward, const double *seg_reward,
                                const double *grad_out,
                                double *g_elp, double *g_trans, double *g_init, double *g_len, double *value_out,
                                void *scratch, size_t scratch_bytes, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The k highest-scoring segmentations (k-best Viterbi: the DP in the k-max semiring; csrc/smm_kbest.hip).  The candidate set
 * is the one smm_viterbi_f64 maximises over, its closing step included (EOS mode: the last position may also close into a
 * real class, at trans + SMM_BIG_NEG); the k results are pairwise distinct segmentations in non-increasing order of score.
 * Inputs, layouts and error returns as smm_viterbi_f64; 1 <= k <= SMM_MAX_KBEST.  SMM_SHAPE_NO_TIME_SPLIT is accepted and
 * ignored: a video is never split.  The workspace is smm_kbest_workspace_bytes (more than smm_workspace_bytes: the lists and
 * back-pointers of every position); the error word sits at smm_error_word_offset as for the other entry points.
 *   spans_out   dev int64 [k][b][t_max + 1]  the Viterbi entry points' span encoding (class map applied)       (nullable)
 *   labels_out  dev int64 [k][total_frames]  per-frame global class ids; frames no video covers are not written (nullable)
 *   score_out   dev fp64 [k][b]  each segmentation's score, re-evaluated in fp64 along the path from the tables and elp
 *               (init, then per segment left to right: trans, len, its emissions; then the closing term)       (nullable)
 *   n_segs_out  dev int32 [k][b]  segments of each result (the closing position not counted)                    (nullable)
 * The ranking is decided by the DP's own sums: two results whose scores differ by no more than rounding may come in either
 * order.  A video with fewer than k segmentations gets score -inf, n_segs 0, a span row of -1 and labels -1 on the ranks past
 * its last.  A NaN that reaches the DP sets the error word and that video's scores are NaN.
 * SMM_ERR_ARG when k is outside 1..SMM_MAX_KBEST or every output is NULL; SMM_ERR_WORKSPACE below smm_kbest_workspace_bytes.
 */
#define SMM_MAX_KBEST 16
/* host only; 0 on invalid arguments (those of smm_workspace_bytes, k outside 1..SMM_MAX_KBEST, c_max or k_rows too large) */
size_t smm_kbest_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host, int32_t k);
int smm_kbest_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                  const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                  const double *elp, const double *trans, const double *init, const double *len_scores,
                  const double *endpen, const int64_t *class_map, int32_t k,
                  int64_t *spans_out, int64_t *labels_out, double *score_out, int32_t *n_segs_out,
                  void *workspace, size_t workspace_bytes, void *stream);

/*
 * Minimum-Bayes-risk (maximum expected accuracy) decode under frame (Hamming) loss (csrc/smm_mbr.hip): per video, the feasible
 * segmentation that maximises sum_t gain[t][y_t] -- with gain = the frame posteriors P(y_t = c | x) (the g_elp of
 * smm_logz_bwd_f64), the expected number of correct frames.  Exact definition: the result is what smm_viterbi_f64 returns on the
 * substituted inputs
 *   elp' = gain;   len'[k][c] = 0 for every usable row (the span limit k_rows / kp still applies);
 *   trans' = M(trans), init' = M(init), endpen' = M(endpen),   M(x) = SMM_BIG_NEG if x <= SMM_BIG_NEG / 2 (-inf included), else 0;
 * everything else unchanged: class map, groups, kp, SMM_SHAPE_NO_EOS, and the EOS closing step (a real class closes at
 * + SMM_BIG_NEG).  A term is forbidden exactly when the posterior gives it zero mass; the gains sum to at most T << 1e9, so the
 * result uses the fewest forbidden terms and, among those paths, has the most expected correct frames.  Ties: the C twin's rule
 * (oracle/smm_oracle.c: in the back-trace the shortest segment first, then the smallest source state; each value
 * re-evaluated as (cum + h) + w); spans, labels, n_segs and best are bit-identical to the twin and to smm_viterbi_f64 on the
 * substituted inputs.  A video is never split along the time axis (SMM_SHAPE_NO_TIME_SPLIT is accepted and ignored).
 *   gain        dev fp64 [total_frames][c_max]
 *   trans, init, endpen, class_map: as smm_viterbi_f64 reads them (made binary on load; endpen nullable); there is no length table
 *   spans, labels, best, n_segs: smm_viterbi_f64's outputs and layouts (best = the DP value)                           (nullable)
 *   gain_sum    dev fp64 [b]: sum_t gain[t][y_t] along the result, summed serially in frame order in fp64              (nullable)
 * Enqueued on `stream` only; never synchronises.  The workspace is smm_mbr_workspace_bytes; the error word sits at
 * smm_error_word_offset.  A NaN in a video's gain sets it (that video's best and gain_sum are NaN, its n_segs 0).
 * SMM_ERR_ARG for a NULL gain / trans / init / workspace, every output NULL or invalid metadata; SMM_ERR_UNSUPPORTED for c_max
 * or k_rows beyond the compiled kernels; SMM_ERR_WORKSPACE below smm_mbr_workspace_bytes -- all before anything is staged.
 */
/* host only; 0 on invalid arguments (those of smm_workspace_bytes, c_max or k_rows too large) */
size_t smm_mbr_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host);
int smm_mbr_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                const double *gain, const double *trans, const double *init, const double *endpen,
                const int64_t *class_map, int64_t *spans, int64_t *labels, double *best, double *gain_sum, int32_t *n_segs,
                void *workspace, size_t workspace_bytes, void *stream);

/*
 * Forced alignment (csrc/smm_align.hip): per video, the best segmentation whose class sequence is the given transcript
 * a[0..M-1] (local state ids, 1 <= M <= SMM_MAX_TRANSCRIPT; consecutive equal ids are two segments); only the boundaries are
 * free.  EOS mode only.  With kp the video's span limit (kp_host, NULL: min(k_rows, t_max)), every + one IEEE fp64 add in
 * this association:
 *   cum[0][c] = 0;  cum[n][c] = cum[n-1][c] + elp[n-1][c]                                    (serial prefix sums)
 *   h[0][0] = init[a_0];  h[0][m>0] = -inf
 *   gam[n][m] = cum[n][a_m] + max_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )              n = 1..T
 *   h[n][m]   = ( gam[n][m-1] + trans[a_m][a_{m-1}] ) - cum[n][a_m]                          0 < n < T, m >= 1; h[n>0][0] = -inf
 *   best      = gam[T][M-1] + (endpen ? endpen[i][a_{M-1}] : 0.0)
 * Back-trace from (n, m, w) = (T, M-1, the closing term): the smallest k whose (cum[n][a_m] + (h[n-k][m] + len[k][a_m])) + w
 * equals the maximum of that expression over k; segment m starts at n - k; on to (n - k, m - 1, trans[a_m][a_{m-1}]).
 * This is, bit for bit, what smm_viterbi_f64 and the C twin (oracle/smm_oracle.c: smm_oracle_viterbi_ex) return on the
 * expanded lattice -- states = transcript positions, elp'[t][m] = elp[t][a_m], len'[k][m] = len[k][a_m],
 * trans'[m][m-1] = trans[a_m][a_{m-1}], init'[0] = init[a_0], endpen'[M-1] = the closing term, every other entry -1e9 -- as
 * long as a path exists and its score stays far from -1e9; with the transcript of the Viterbi path it is the Viterbi decode.
 * Model-forbidden transitions (-1e9 in trans) are ordinary finite scores here.
 *   transcript              dev int32 [transcript_offset_host[b]]: video i's ids at [offset[i], offset[i+1])
 *   transcript_offset_host  host int64 [b + 1], non-decreasing; every video has at least one id
 *   elp, trans, init, len_scores, endpen, class_map: as smm_viterbi_f64 reads them (endpen, class_map nullable)
 *   spans, labels, best, n_segs: smm_viterbi_f64's outputs and layouts; n_segs = M                              (nullable)
 * A video without a path by counting (M > T or M (kp - 1) < T), or with an id outside [0, n_states), gets best = -inf,
 * n_segs = 0, spans and labels -1; the error word stays clear and no table is read with such an id.  The error word is set
 * (best NaN, n_segs 0, spans and labels -1) when the prefix sum cum[T][c] of ANY state c < n_states of the video is not finite
 * -- a NaN, +inf or -inf anywhere in the video's elp, also in a class the transcript never names: h = gam - cum has no value
 * then, as in the twin -- or when a table entry the transcript reads (init[a_0], trans[a_m][a_{m-1}], len[k][a_m] for
 * k < kp, endpen[a_{M-1}]) is a NaN or +inf; -inf in such a table entry is an ordinary "impossible".  Enqueued on `stream` only; never synchronises; a video is never split along the time axis.  The workspace is
 * smm_align_workspace_bytes; the error word sits at smm_error_word_offset.
 * SMM_ERR_ARG for a NULL required pointer, every output NULL, non-monotone offsets or an empty transcript;
 * SMM_ERR_UNSUPPORTED for SMM_SHAPE_NO_EOS, a transcript longer than SMM_MAX_TRANSCRIPT, c_max or k_rows beyond the compiled
 * kernels; SMM_ERR_WORKSPACE below smm_align_workspace_bytes -- all before anything is staged.
 */
#define SMM_MAX_TRANSCRIPT 256
/* host only; 0 on invalid arguments (whatever smm_align_f64 refuses for the shape, the lengths or the offsets) */
size_t smm_align_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host, const int64_t *transcript_offset_host);
int smm_align_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                  const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                  const double *elp, const double *trans, const double *init, const double *len_scores,
                  const double *endpen, const int64_t *class_map, const int32_t *transcript,
                  const int64_t *transcript_offset_host, int64_t *spans, int64_t *labels, double *best, int32_t *n_segs,
                  void *workspace, size_t workspace_bytes, void *stream);

/*
 * Forced alignment with optional transcript entries (csrc/smm_align_opt.hip): per video, the best segmentation whose class
 * sequence is the transcript a[0..M-1] with any subset of its optional entries left out.  opt[0..M-1] flags the entries
 * (0 = mandatory, non-zero = optional); kw = kp - 1.  With
 *   pred(m)  = the entries that may directly precede entry m: j = m-1, m-2, ... down to and including the nearest mandatory
 *              entry (down to 0 when no mandatory entry lies before m),
 *   first(m) = every entry before m is optional (entry m may be the first segment),
 *   end(j)   = every entry after j is optional (entry j may be the last segment),
 *   nb(m) / na(m) = the number of mandatory entries before / after m,
 * every + and - one IEEE fp64 operation in this association:
 *   cum as in smm_align_f64
 *   h[0][m]   = init[a_m] if first(m), else -inf
 *   h[n][m]   = max_{j in pred(m)} ( gam[n][j] + trans[a_m][a_j] ) - cum[n][a_m]              0 < n < T
 *   gam[n][m] = cum[n][a_m] + max_{k=1..min(kw,n)} ( h[n-k][m] + len[k][a_m] )                n = 1..T
 *   best      = max_{j : end(j)} ( gam[T][j] + closing_j )                  closing_j = endpen ? endpen[i][a_j] : 0.0
 * Back-trace: start from n = T with the candidates {j : end(j)} and the weights w_j = closing_j.  Among all (k, j) take the
 * smallest k, then the smallest j, whose (cum[n][a_j] + (h[n-k][j] + len[k][a_j])) + w_j equals the maximum of that
 * expression; the segment is entry j on [n-k, n); continue from n - k with the candidates pred(j) and w_i = trans[a_j][a_i];
 * stop at n = 0.  This is smm_oracle_viterbi_ex on the expanded lattice -- states = transcript positions,
 * trans'[m][j] = trans[a_m][a_j] for j in pred(m), init'[m] = init[a_m] for first(m), endpen'[j] = closing_j for end(j), every
 * other entry -1e9 -- bit for bit, the tie rule being the twin's "shortest segment, then smallest source state".
 * Only the cells max(nb(m)+1, T - (M-1-m) kw) <= n <= min(T - na(m), (m+1) kw) of column m lie on a complete alignment; the
 * kernel evaluates those.
 *   optional   dev uint8 [transcript_offset_host[b]], laid out like `transcript`                                   (required)
 *   used       dev int32, laid out like `transcript`: 1 for an entry that has a segment, else 0                     (nullable)
 *   spans, labels, best as smm_align_f64; n_segs = the number of entries that got a segment; every other argument as
 *   smm_align_f64.  With every flag 0 the results are bit-identical to smm_align_f64's.
 * A video whose mandatory entries outnumber its frames, or with M kw < T, kw < 1, or an id outside [0, n_states), gets
 * best = -inf, n_segs = 0, spans and labels -1, used 0; the error word stays clear.  The error word is set (best NaN, n_segs 0,
 * spans and labels -1, used 0) as by smm_align_f64: a prefix sum cum[T][c] of any state of the video that is not finite, or a
 * NaN or +inf in a table entry the recursion reads -- init[a_m] for first(m), trans[a_m][a_j] for j in pred(m), len[k][a_m]
 * for k < kp, endpen[a_j] for end(j); -inf there is an ordinary "impossible", -1e9 an ordinary finite score.
 * The workspace is smm_align_opt_workspace_bytes (smm_align_workspace_bytes plus c_max (T + 1) doubles per video: the running
 * maxima per class that keep a column's cost independent of the length of an optional run).  Refusals as smm_align_f64's,
 * plus SMM_ERR_ARG for a NULL `optional` -- all before anything is staged.
 */
size_t smm_align_opt_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host, const int64_t *transcript_offset_host);
int smm_align_opt_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                      const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                      const double *elp, const double *trans, const double *init, const double *len_scores,
                      const double *endpen, const int64_t *class_map, const int32_t *transcript, const uint8_t *optional,
                      const int64_t *transcript_offset_host, int64_t *spans, int64_t *labels, double *best, int32_t *n_segs,
                      int32_t *used, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Forced alignment to a transcript graph (csrc/smm_align_graph.hip): per video, the best segmentation whose class sequence is
 * a start -> end path of a DAG whose nodes carry a class.  A set of candidate transcripts is their prefix trie, "a or b" two
 * nodes with the same neighbours, a free order two branches, a long skip one more edge; a plain transcript is a chain and a
 * transcript with optional entries a special DAG.  A video's nodes are numbered 0..M-1 in TOPOLOGICAL order,
 * 1 <= M <= SMM_MAX_TRANSCRIPT; a_m is node m's local state id; pred(m) = the nodes that may directly precede node m, every
 * one of them < m; start(m) / end(m): node m may be the first / the last segment; kw = kp - 1.  Every + and - one IEEE fp64
 * operation in this association:
 *   cum as in smm_align_f64
 *   h[0][m]   = init[a_m] if start(m), else -inf
 *   h[n][m]   = max_{j in pred(m)} ( gam[n][j] + trans[a_m][a_j] ) - cum[n][a_m]              0 < n < T  (-inf for an empty pred(m))
 *   gam[n][m] = cum[n][a_m] + max_{k=1..min(kw,n)} ( h[n-k][m] + len[k][a_m] )                n = 1..T
 *   best      = max_{j : end(j)} ( gam[T][j] + closing_j )                  closing_j = endpen ? endpen[i][a_j] : 0.0
 * Back-trace: smm_align_opt_f64's.  Start from n = T with the candidates {j : end(j)} and the weights w_j = closing_j.  Among
 * all (k, j) take the smallest k, then the smallest j, whose (cum[n][a_j] + (h[n-k][j] + len[k][a_j])) + w_j equals the maximum
 * of that expression; the segment is node j on [n-k, n); continue from n - k with the candidates pred(j) and
 * w_i = trans[a_j][a_i]; stop at n = 0, where the node is a start node.  This is smm_oracle_viterbi_ex on the expanded lattice
 * -- states = nodes, trans'[m][j] = trans[a_m][a_j] for j in pred(m), init'[m] = init[a_m] for start(m), endpen'[j] = closing_j
 * for end(j), every other entry -1e9 -- bit for bit.
 *   With pred(m) = {m-1}, start = {0} and end = {M-1}, every output equals smm_align_f64's, bit for bit.
 *   With pred / start / end as smm_align_opt_f64 derives them from optional flags (start = its first), every output equals
 *   smm_align_opt_f64's, bit for bit, `used` included.
 * With bmin(m) / bmax(m) the fewest / most nodes before m on a path from a start node and amin(m) / amax(m) the fewest / most
 * after it on a path to an end node, only the cells max(bmin+1, T - amax kw) <= n <= min(T - amin, (bmax+1) kw) of column m
 * lie on a complete alignment; the kernel evaluates those (smm_align_opt_f64's cells for a graph built from flags).
 *   node_class        dev int32 [node_offset_host[b]]: video i's nodes at [offset[i], offset[i+1])              (required)
 *   pred_mask         dev uint32 [8 * node_offset_host[b]]: 8 words per node, laid out like node_class; bit j of node m's
 *                     256-bit mask (word j / 32, bit j % 32) is set when j is in pred(m)                         (required)
 *   node_flags        dev uint8, laid out like node_class: bit 0 = start(m), bit 1 = end(m)                      (required)
 *   node_offset_host  host int64 [b + 1], non-decreasing; every video has at least one node
 *   used              dev int32, laid out like node_class: 1 for the nodes of the path, else 0; the path is the used nodes
 *                     in index order                                                                            (nullable)
 *   spans, labels, best as smm_align_f64; n_segs = the number of nodes on the path; every other argument as smm_align_f64.
 * With Lmin / Lmax the fewest / most nodes on any start -> end path: a video without such a path, or with Lmin > T, kw < 1,
 * Lmax kw < T, an id outside [0, n_states) or a mask bit j >= m, gets best = -inf, n_segs = 0, spans and labels -1, used 0; the
 * error word stays clear and no table is read (for a graph built from optional flags this is smm_align_opt_f64's rule).  A
 * video that passes this rule but has no alignment of finite score (path lengths the graph skips, -inf table entries) gets
 * the same.  The error word is set (best NaN, n_segs 0, spans and labels -1, used 0) under smm_align_opt_f64's conditions read
 * structurally: a prefix sum cum[T][c] of any state of the video that is not finite, or a NaN or +inf in a table entry the
 * recursion reads -- init[a_m] for start(m), trans[a_m][a_j] for every edge, len[k][a_m] for k < kp and every node,
 * endpen[a_j] for end(j) -- every node and every edge, on a start -> end path or not.
 * Enqueued on `stream` only; never synchronises; a video is never split; the error word sits at smm_error_word_offset.
 * The workspace is smm_align_graph_workspace_bytes = smm_align_workspace_bytes(shape, lengths_host, node_offset_host)
 * + 8 * sum_i M_i (T_i + 1) bytes: the gam columns, which a column reads over its edges, behind the h columns.
 * SMM_ERR_ARG for a NULL required pointer, every output NULL, non-monotone offsets or a video without nodes;
 * SMM_ERR_UNSUPPORTED for SMM_SHAPE_NO_EOS, more than SMM_MAX_TRANSCRIPT nodes in a video, c_max or k_rows beyond the compiled
 * kernels; SMM_ERR_WORKSPACE below smm_align_graph_workspace_bytes -- all before anything is staged.
 */
size_t smm_align_graph_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host, const int64_t *node_offset_host);
int smm_align_graph_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                        const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                        const double *elp, const double *trans, const double *init, const double *len_scores,
                        const double *endpen, const int64_t *class_map, const int32_t *node_class, const uint32_t *pred_mask,
                        const uint8_t *node_flags, const int64_t *node_offset_host, int64_t *spans, int64_t *labels,
                        double *best, int32_t *n_segs, int32_t *used, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Transcript likelihood (csrc/smm_align_logz.hip): per video log Z_a = log sum_{y : classes(y) = a} exp score(y), the sum over
 * every segmentation whose class sequence is the transcript a[0..M-1], and the gradient of sum_i u_i log Z_a(i).  log Z_a is the
 * joint log-likelihood of frames and transcript, log Z_a - log Z (smm_logz_f64) the conditional one; the gradient is the E-step
 * of transcript-supervised training.  Conventions of smm_align_f64: EOS mode only, 1 <= M <= SMM_MAX_TRANSCRIPT local state
 * ids, consecutive equal ids are two segments, kp the video's span limit, cum the serial prefix sum of elp,
 * closing = endpen ? endpen[i][a_{M-1}] : 0; lse is log-sum-exp, and an lse over only -inf terms is -inf.
 *   forward   h[0][0] = init[a_0];  h[0][m>0] = -inf;  h[n>0][0] = -inf
 *             gam[n][m] = cum[n][a_m] + lse_{k=1..min(kp-1,n)} ( h[n-k][m] + len[k][a_m] )            n = 1..T
 *             h[n][m]   = gam[n][m-1] + trans[a_m][a_{m-1}] - cum[n][a_m]                             0 < n < T, m >= 1
 *             logZ_a    = gam[T][M-1] + closing
 *   backward  bg[T][M-1] = closing;  bg[T][m<M-1] = -inf
 *             bh[s][m]  = lse_{k=1..min(kp-1,T-s)} ( len[k][a_m] + cum[s+k][a_m] + bg[s+k][m] )       s = 0..T-1
 *             bg[n][m]  = trans[a_{m+1}][a_m] - cum[n][a_{m+1}] + bh[n][m+1]                          0 < n < T, m < M-1
 *             (identity: h[0][0] + bh[0][0] = logZ_a)
 *   marginals S[s][m] = exp(h[s][m] + bh[s][m] - logZ_a)      segment m starts at s   (= E[s][m-1] for m >= 1; S[0][0] = 1)
 *             E[n][m] = exp(gam[n][m] + bg[n][m] - logZ_a)    segment m ends at n
 *             occ[t][m] = sum_{s<=t} S[s][m] - sum_{n<=t} E[n][m]                                    frame t lies in segment m
 *   gradients of sum_i u_i logZ_a(i)   (u = grad_logz, NULL = ones):
 *             g_elp[t][c]    = u_i * sum_{m: a_m = c} occ[t][m]
 *             g_len[k][c]    = sum_i u_i * sum_{m: a_m = c} sum_s exp(h[s][m] + len[k][c] + cum[s+k][c] + bg[s+k][m] - logZ_a)
 *             g_trans[c][c'] = sum_i u_i * #{m >= 1 : a_m = c, a_{m-1} = c'}        (every alignment uses the same transitions)
 *             g_init[c]      = sum_i u_i * [a_0 = c]
 * Each lse takes its own maximum as the reference: the differences are formed in fp64, exponentiated in fp32 and summed in
 * fp64, so the values hold for any dynamic range of the scores (|logZ_a - exact| ~ 1e-7 per column).  Every sum -- over the
 * videos of a group, the transcript entries, the positions -- is taken in a fixed order without atomics: two calls on the same
 * inputs give the same bits.
 *   - A video without a path by counting (M > T or M (kp - 1) < T), or with an id outside [0, n_states), gets logZ_a = -inf
 *     and contributes exactly zero to every gradient (its g_elp rows are zeros); the error word stays clear and no table is
 *     read with such an id.
 *   - A video with a path by counting but none of finite score (-inf table entries, an ordinary "impossible") likewise gets
 *     -inf and zero gradients.
 *   - The error word is set, logZ_a is NaN and the gradient contributions are zero under smm_align_f64's conditions: cum[T][c]
 *     not finite for any state of the video, or a NaN or +inf in a table entry the transcript reads.
 * smm_align_logz_bwd_f64 must follow smm_align_logz_f64 for the same batch, tables and transcripts on the same workspace and
 * stream: it reads the cum, h and gam columns the forward call left there (and writes the bg columns and the videos' parts of
 * g_len beside them); logz_a is the forward call's output.  g_elp, g_trans, g_init, g_len have smm_logz_bwd_f64's layouts and
 * are overwritten entirely (zero fills are kernels).  The workspace is smm_align_logz_workspace_bytes -- the only size query
 * these entry points add to -- and the error word sits at smm_error_word_offset; staging the backward call clears the word,
 * and the backward call sets it again for every video whose logz_a is NaN.  Enqueued on `stream` only; never synchronises;
 * a video is never split over workgroups.
 * SMM_ERR_ARG for a NULL required pointer, non-monotone offsets or an empty transcript; SMM_ERR_UNSUPPORTED for
 * SMM_SHAPE_NO_EOS, a transcript longer than SMM_MAX_TRANSCRIPT, c_max or k_rows beyond the compiled kernels;
 * SMM_ERR_WORKSPACE below smm_align_logz_workspace_bytes -- all before anything is staged.
 */
/* host only; 0 on whatever the calls refuse for the shape, the lengths or the offsets */
size_t smm_align_logz_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host, const int64_t *transcript_offset_host);
int smm_align_logz_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                       const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                       const double *elp, const double *trans, const double *init, const double *len_scores,
                       const double *endpen, const int32_t *transcript, const int64_t *transcript_offset_host,
                       double *logz_a /* dev [b] */, void *workspace, size_t workspace_bytes, void *stream);
int smm_align_logz_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                           const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                           const double *elp, const double *trans, const double *init, const double *len_scores,
                           const double *endpen, const int32_t *transcript, const int64_t *transcript_offset_host,
                           const double *logz_a, const double *grad_logz /* nullable */, double *g_elp, double *g_trans,
                           double *g_init, double *g_len, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Transcript likelihood with optional entries (csrc/smm_align_opt_logz.hip): the log-semiring counterpart of smm_align_opt_f64,
 * with its gradient.  Per video log Z_o = log of the sum of exp score over every ALIGNMENT of the video to the transcript
 * a[0..M-1]: a choice of which optional entries get a segment, and of the boundaries.  Definitions of smm_align_opt_f64 (pred,
 * first, end, nb, na; closing_j = endpen ? endpen[i][a_j] : 0) and conventions of smm_align_logz_f64 (EOS mode only, local
 * state ids, kw = kp - 1, cum the serial prefix sum, lse of only -inf terms is -inf); succ(j) = { m : j in pred(m) }, that is
 * j+1, j+2, ... up to and including the next mandatory entry (to M-1 when there is none).
 *   forward   h[0][m]   = init[a_m] if first(m), else -inf
 *             h[n][m]   = lse_{j in pred(m)} ( gam[n][j] + trans[a_m][a_j] ) - cum[n][a_m]            0 < n < T
 *             gam[n][m] = cum[n][a_m] + lse_{k=1..min(kw,n)} ( h[n-k][m] + len[k][a_m] )              n = 1..T
 *             logZ_o    = lse_{j : end(j)} ( gam[T][j] + closing_j )
 *   backward  bg[T][j]  = closing_j if end(j), else -inf
 *             bh[s][m]  = lse_{k=1..min(kw,T-s)} ( len[k][a_m] + cum[s+k][a_m] + bg[s+k][m] )         s = 0..T-1
 *             bg[n][j]  = lse_{m in succ(j)} ( trans[a_m][a_j] - cum[n][a_m] + bh[n][m] )             0 < n < T
 *             (identity: lse_{m : first(m)} ( h[0][m] + bh[0][m] ) = logZ_o)
 *   marginals S[s][m]   = exp(h[s][m] + bh[s][m] - logZ_o)          entry m has a segment that starts at s
 *             E[n][m]   = exp(gam[n][m] + bg[n][m] - logZ_o)        ... that ends at n
 *             occ[t][m] = sum_{s<=t} S[s][m] - sum_{n<=t} E[n][m]   frame t lies in the segment of entry m
 *             p_used[m] = sum_n E[n][m]                             entry m has a segment at all (1 for a mandatory entry)
 *   gradients of sum_i u_i logZ_o(i)   (u = grad_logz, NULL = ones):
 *             g_elp[t][c]    = u_i sum_{m: a_m=c} occ[t][m]
 *             g_len[k][c]    = sum_i u_i sum_{m: a_m=c} sum_s exp(h[s][m] + len[k][c] + cum[s+k][c] + bg[s+k][m] - logZ_o)
 *             g_trans[c][c'] = sum_i u_i sum_{m: a_m=c} sum_{j in pred(m): a_j=c'} sum_{0<n<T}
 *                                      exp(gam[n][j] + trans[c][c'] - cum[n][c] + bh[n][m] - logZ_o)
 *             g_init[c]      = sum_i u_i sum_{m: first(m), a_m=c} S[0][m]
 *   g_trans and g_init are sums of posteriors here, not counts; there is no gradient for endpen.
 * What is summed: alignments, not class sequences.  Where no two subsets of the optional entries give the same class sequence
 * logZ_o is the log-likelihood of the SET of class sequences the transcript stands for.  Where two subsets do -- [x?, y?, x?]
 * without y, either x -- the segmentations with that class sequence are counted once per subset.  Whether a transcript is of
 * that kind is host arithmetic on the ids and the flags (the Python layer ships the predicate: ops.transcript_is_ambiguous).
 * With no flag set this is smm_align_logz_f64's value (the h, gam and bg columns are formed in its association).
 * What the structure decides is returned exactly, as smm_align_logz_bwd_f64 returns counts: p_used of a mandatory entry is 1;
 * where pred(m) = {m-1} and succ(m-1) = {m}, S[.][m] is taken as E[.][m-1] and the transition's posterior as p_used[m-1]; the
 * start posteriors S[0][m] are normalised by their own total (the identity's left side), so g_init adds up to u_i.
 * Numerics of smm_align_logz_f64 for the span sums; a sum over pred(m) or succ(j) is a running per-class log-sum kept as an fp64
 * logarithm (max + log1p(exp(min - max))), then one lse over at most n_states classes in fp64: exact for any dynamic range.
 * Every sum is taken in a fixed order without atomics: two calls on the same inputs give the same bits.
 *   - A video whose MANDATORY entries outnumber its frames, or with M kw < T, kw < 1, or an id outside [0, n_states), gets
 *     logZ_o = -inf, zero gradient contributions and p_used 0; the error word stays clear and no table is read with such an id.
 *   - A video with a path by counting but none of finite score (-inf table entries) likewise gets -inf, zeros and p_used 0.
 *   - The error word is set, logZ_o is NaN, the gradient contributions and p_used are zero under smm_align_opt_f64's
 *     conditions: cum[T][c] not finite for any state of the video, or a NaN or +inf in a table entry the recursion reads:
 *     init[a_m] for first(m), trans[a_m][a_j] for j in pred(m), len[k][a_m] for k < kp, endpen[i][a_j] for end(j).
 * smm_align_opt_logz_bwd_f64 must follow smm_align_opt_logz_f64 for the same batch, tables, transcripts and flags on the same
 * workspace and stream: it reads the cum, h and gam columns and the columns' ranges the forward call left there.  g_elp,
 * g_trans, g_init, g_len have smm_logz_bwd_f64's layouts and are overwritten entirely (zero fills are kernels); p_used
 * (nullable) is laid out like `transcript` and written for every entry.  The workspace is smm_align_opt_logz_workspace_bytes
 * (more than smm_align_logz_workspace_bytes: a fourth column per entry and n_states columns of running sums per video); the
 * error word sits at smm_error_word_offset; staging the backward call clears the word, and the backward call sets it again
 * for every video whose logz_o is NaN.  Enqueued on `stream` only; never synchronises; a video is never split over workgroups.
 * SMM_ERR_ARG for a NULL required pointer (`optional` is one), non-monotone offsets or an empty transcript;
 * SMM_ERR_UNSUPPORTED for SMM_SHAPE_NO_EOS, a transcript longer than SMM_MAX_TRANSCRIPT, c_max or k_rows beyond the compiled
 * kernels; SMM_ERR_WORKSPACE below smm_align_opt_logz_workspace_bytes -- all before anything is staged.
 */
/* host only; 0 on whatever the calls refuse for the shape, the lengths or the offsets */
size_t smm_align_opt_logz_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host, const int64_t *transcript_offset_host);
int smm_align_opt_logz_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                           const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                           const double *elp, const double *trans, const double *init, const double *len_scores,
                           const double *endpen, const int32_t *transcript, const uint8_t *optional /* dev, required */,
                           const int64_t *transcript_offset_host, double *logz_o /* dev [b] */, void *workspace,
                           size_t workspace_bytes, void *stream);
int smm_align_opt_logz_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                               const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                               const double *elp, const double *trans, const double *init, const double *len_scores,
                               const double *endpen, const int32_t *transcript, const uint8_t *optional,
                               const int64_t *transcript_offset_host, const double *logz_o, const double *grad_logz /* nullable */,
                               double *g_elp, double *g_trans, double *g_init, double *g_len,
                               double *p_used /* dev double, laid out like transcript, nullable */, void *workspace,
                               size_t workspace_bytes, void *stream);

/*
 * Transcript-graph likelihood (csrc/smm_align_graph_logz.hip): the log-semiring counterpart of smm_align_graph_f64, with its
 * gradient and the node / end posteriors.  Per video log Z_g = log of the sum of exp score over every ALIGNMENT of the video to
 * the graph: a start -> end path, and the boundaries of its nodes' segments.  With a candidate set as its prefix trie this is
 * the "one of these N transcripts" objective, and p_end the posterior over the candidates.  Nodes, pred, start, end, the mask /
 * flag / offset encodings and kw = kp - 1 are exactly smm_align_graph_f64's; lse, cum and closing_j as in
 * smm_align_opt_logz_f64; succ(j) = { m : j in pred(m) }.
 *   forward   h[0][m]   = init[a_m] if start(m), else -inf
 *             h[n][m]   = lse_{j in pred(m)} ( gam[n][j] + trans[a_m][a_j] ) - cum[n][a_m]            0 < n < T
 *             gam[n][m] = cum[n][a_m] + lse_{k=1..min(kw,n)} ( h[n-k][m] + len[k][a_m] )              n = 1..T
 *             logZ_g    = lse_{j : end(j)} ( gam[T][j] + closing_j )
 *   backward  bg[T][j]  = closing_j if end(j), else -inf
 *             bh[s][m]  = lse_{k=1..min(kw,T-s)} ( len[k][a_m] + cum[s+k][a_m] + bg[s+k][m] )         s = 0..T-1
 *             bg[n][j]  = lse_{m in succ(j)} ( trans[a_m][a_j] - cum[n][a_m] + bh[n][m] )             0 < n < T
 *             (identity: lse_{m : start(m)} ( h[0][m] + bh[0][m] ) = logZ_g)
 *   marginals S, E, occ as smm_align_opt_logz_f64;  p_used[m] = sum_n E[n][m]      node m lies on the path
 *             p_end[j]  = exp(gam[T][j] + closing_j - logZ_g) for end(j), else 0   the path ends in node j
 *   gradients of sum_i u_i logZ_g(i)   (u = grad_logz, NULL = ones): g_elp, g_len as smm_align_opt_logz_f64;
 *             g_trans[c][c'] = sum_i u_i sum_{edges j->m : a_m=c, a_j=c'} sum_{0<n<T}
 *                                      exp(gam[n][j] + trans[c][c'] - cum[n][c] + bh[n][m] - logZ_g)
 *             g_init[c]      = sum_i u_i sum_{m : start(m), a_m=c} S[0][m]
 * What is summed is paths times boundaries, not class sequences: two start -> end paths that spell the same class sequence
 * count its segmentations twice (the Python layer ships the predicate: TranscriptGraph.is_ambiguous).  A prefix trie never
 * has two such paths: for a trie logZ_g = lse over the distinct candidates of smm_align_logz_f64's logZ_a.
 * The start posteriors S[0][m] are normalised by the backward pass's own total (the identity's left side), so g_init of a video
 * adds up to u_i.  Nothing else is decided by the structure: every other posterior is a sum of exponentials, and a chain's
 * g_trans is 1 per transition only to the family's accuracy.
 * Numerics of smm_align_logz_f64 for the span sums; a sum over pred(m) or succ(j) takes its own maximum as the reference and
 * exponentiates in fp64; a single predecessor or successor comes out as (gam + trans) - cum, smm_align_logz_f64's
 * association, exactly.  Every sum is taken in a fixed order without atomics: two calls on the same inputs give the same bits.
 *   - Degenerate videos follow smm_align_graph_f64's rule: no start -> end path, Lmin > T, kw < 1, Lmax kw < T, an id outside
 *     [0, n_states) or a mask bit j >= m give logZ_g = -inf, exactly zero gradient contributions and p_used / p_end 0; the
 *     error word stays clear and no table is read.
 *   - A video that passes this rule but has no alignment of finite score gets the same.
 *   - The error word is set, logZ_g is NaN, the contributions, p_used and p_end are zero under smm_align_graph_f64's
 *     conditions: every node and every edge, on a start -> end path or not.
 * smm_align_graph_logz_bwd_f64 must follow smm_align_graph_logz_f64 for the same batch, tables and graphs on the same
 * workspace and stream: it reads the cum, h and gam columns and the columns' ranges the forward call left there.  g_elp,
 * g_trans, g_init, g_len have smm_logz_bwd_f64's layouts and are overwritten entirely; p_used and p_end (nullable) are laid out
 * like node_class and written for every node.  Staging the backward call clears the error word, and the backward call sets it
 * again for every video whose logz_g is NaN.  Enqueued on `stream` only; never synchronises; a video is never split.
 * The workspace is smm_align_graph_logz_workspace_bytes: smm_workspace_bytes (cum lives in its history area), the offsets and
 * the launch order, then per video 8 * (3 M + 4 M (T + 1)) bytes -- the columns' recorded ranges and the h, gam, q and bh
 * columns -- then per video 8 * (min(k_rows, T + 1) c_max + c_max^2 + c_max + 1) bytes: its parts of g_len, g_trans and g_init
 * and the backward pass's own logZ_g; each area starts on a multiple of 256 bytes.
 * Refusals as smm_align_graph_f64: SMM_ERR_ARG for a NULL required pointer, non-monotone offsets or a video without nodes;
 * SMM_ERR_UNSUPPORTED for SMM_SHAPE_NO_EOS, more than SMM_MAX_TRANSCRIPT nodes in a video, c_max or k_rows beyond the compiled
 * kernels; SMM_ERR_WORKSPACE below smm_align_graph_logz_workspace_bytes -- all before anything is staged.
 */
/* host only; 0 on whatever the calls refuse for the shape, the lengths or the offsets */
size_t smm_align_graph_logz_workspace_bytes(const smm_shape *shape, const int64_t *lengths_host, const int64_t *node_offset_host);
int smm_align_graph_logz_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                             const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                             const double *elp, const double *trans, const double *init, const double *len_scores,
                             const double *endpen, const int32_t *node_class, const uint32_t *pred_mask,
                             const uint8_t *node_flags, const int64_t *node_offset_host, double *logz_g /* dev [b] */,
                             void *workspace, size_t workspace_bytes, void *stream);
int smm_align_graph_logz_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                 const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                 const double *elp, const double *trans, const double *init, const double *len_scores,
                                 const double *endpen, const int32_t *node_class, const uint32_t *pred_mask,
                                 const uint8_t *node_flags, const int64_t *node_offset_host, const double *logz_g,
                                 const double *grad_logz /* nullable */, double *g_elp, double *g_trans, double *g_init,
                                 double *g_len, double *p_used /* dev double, laid out like node_class, nullable */,
                                 double *p_end /* the same layout, nullable */, void *workspace, size_t workspace_bytes,
                                 void *stream);

/*
 * Alignments drawn from the transcript-graph posterior (csrc/smm_align_graph_sample.hip): n_samples independent draws per video
 * from p(alignment | x, "the class sequence is a start -> end path of the graph"), the distribution whose normaliser
 * smm_align_graph_logz_f64 returns.  An ALIGNMENT is a start -> end path and the boundaries of its nodes' segments: on an
 * ambiguous graph two paths that spell the same class sequence are two alignments, each with its own probability, exactly as
 * they are two terms of log Z_g.  A chain samples the boundaries of a plain transcript, TranscriptGraph.from_optional which
 * optional entries are kept as well, a prefix trie which candidate.
 * Call order: the call must follow smm_align_graph_logz_f64 for the same batch, tables and graphs on the same workspace and
 * stream; logz_g is that call's output.  It reads cum, the h and gam columns and the columns' ranges, and writes NOTHING into
 * the workspace but the error word; there is no size query of its own (smm_align_graph_logz_workspace_bytes).
 * smm_align_graph_logz_bwd_f64 may run before or after it, or between two sampler calls: the backward call writes only the q
 * and bh columns and the per-video gradient parts, none of which the sampler reads, so the samples do not change by a bit.
 * The walk, one per (video, sample), from n = T, its weights taken from the forward histories only:
 *   end node     j ~ exp(gam[T][j] + closing_j) over the nodes with end(j)
 *   span         the segment of node j that ends at n starts at n - k,  k ~ exp(h[n-k][j] + len[k][a_j]),  k = 1..min(kw, n)
 *   predecessor  at s = n - k > 0,  i ~ exp(gam[s][i] + trans[a_j][a_i]) over i in pred(j);  the walk stops at s = 0
 * A candidate outside the ranges the forward call recorded for its column is never loaded and has no mass.
 * Random numbers: Philox4x32-10 keyed by `seed`, counter = (decision number, sample, video, 1) -- smm_sample_f64's last word is
 * 0, so the two samplers never share a stream under one seed; every decision takes one counter value, also one with a single
 * candidate.  Sample j depends on (seed, video, j) only: not on n_samples, the grid or the order the waves run in.
 * Outputs (each nullable, not all): spans_out and labels_out in smm_sample_f64's encodings (class map applied, the EOS id at
 * position T; labels_out frames no video covers are left alone); n_segs_out the number of nodes on the path; used_out 1 for the
 * nodes on the path, laid out like node_class per sample; logp_out the exact log-probability of the drawn alignment: its score
 * summed in fp64 from init, the elp of every segment, len, trans and the closing term, minus logz_g.  The histories carry the
 * forward kernel's rounding; they decide the draws, never this value.
 *   - A video whose logz_g is -inf has no alignment: spans and labels -1, n_segs 0, used 0, logp NaN; the error word stays clear.
 *   - A NaN logz_g, or a decision without a candidate of finite weight, sets the error word and gives the same outputs.
 * Enqueued on `stream` only; never synchronises; no atomics but the error word.
 * Refusals: SMM_ERR_ARG for a NULL required pointer (logz_g included), n_samples <= 0, every output NULL, non-monotone offsets or
 * a video without nodes; SMM_ERR_UNSUPPORTED for SMM_SHAPE_NO_EOS, more than SMM_MAX_TRANSCRIPT nodes in a video, c_max or k_rows
 * beyond the compiled kernels; SMM_ERR_WORKSPACE below smm_align_graph_logz_workspace_bytes -- all before anything is staged.
 */
int smm_align_graph_sample_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                               const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                               const double *elp, const double *trans, const double *init, const double *len_scores,
                               const double *endpen, const int64_t *class_map /* nullable */, const int32_t *node_class,
                               const uint32_t *pred_mask, const uint8_t *node_flags, const int64_t *node_offset_host,
                               const double *logz_g, int32_t n_samples, uint64_t seed,
                               int64_t *spans_out  /* dev [n_samples][b][t_max+1], nullable */,
                               int64_t *labels_out /* dev [n_samples][total_frames], nullable */,
                               double *logp_out    /* dev [n_samples][b], nullable */,
                               int32_t *n_segs_out /* dev [n_samples][b], nullable */,
                               int32_t *used_out   /* dev [n_samples][node_offset_host[b]], nullable */,
                               void *workspace, size_t workspace_bytes, void *stream);

/*
 * The exact entropy of the transcript-graph posterior (csrc/smm_align_graph_entropy.hip): per video
 * H = -sum_y p(y) log p(y) in nats over the ALIGNMENTS y of smm_align_graph_sample_f64's distribution -- "how sure is the model
 * of this alignment?".  On an ambiguous graph two paths that spell one class sequence are two alignments, exactly as in log Z_g
 * and in the sampler.  What smm_entropy_f64 is to smm_logz_f64.
 * The chain rule of entropy over the sampler's decisions, in smm_align_graph_logz_f64's notation (h, gam, q[n][j] =
 * cum[n][a_j] + bg[n][j], bh, closing_j, kw, and the ranges [lo_j, hi_j] of gam / q and [slo_j, shi_j] of h / bh the forward
 * call records per column).  For a list of weights w, of which only the finite, in-range ones count:
 *   Hloc(w) = log Z - A / Z,   Z = sum exp(w - max w),   A = sum exp(w - max w) (w - max w)        a single candidate: exactly 0
 *   E[n][j] = exp(gam[n][j] + (q[n][j] - cum[n][a_j]) - logZ_g)                a segment of node j ends at n
 *   S[s][j] = exp(h[s][j] + bh[s][j] - logZ_g)                                 a segment of node j starts at s
 *   H_end   = Hloc( gam[T][j] + closing_j : end(j) )
 *   H_span  = sum_j sum_{n in [lo_j, hi_j]}   E[n][j] Hloc( h[n-k][j] + len[k][a_j] : k = 1..min(kw, n) )
 *   H_pred  = sum_j sum_{s in [slo_j, shi_j]} S[s][j] Hloc( gam[s][i] + trans[a_j][a_i] : i in pred(j) )
 *   h_out   = (H_end + H_span) + H_pred;   h_parts (nullable) = H_end, H_span, H_pred per video; every term >= 0
 * H_end is the entropy of p_end: for a prefix trie the entropy of the posterior over the candidates, and h_out - H_end the
 * expected boundary entropy given the candidate.  A chain has H_end = H_pred = 0.0 exactly, and H = 0.0 when T = M.
 * Call order: the call must follow smm_align_graph_logz_f64 for the same batch, tables and graphs on the same workspace and
 * stream; logz_g is that call's output.  It launches smm_align_graph_logz_bwd_f64's first kernel itself for the q and bh
 * columns (without p_used / p_end, and without the g_elp / g_len / reduce kernels behind it: nothing of a gradient is
 * computed that the entropy does not read), then one kernel of its own, one workgroup per video.  It may run before, after or
 * between smm_align_graph_logz_bwd_f64 and smm_align_graph_sample_f64 calls: it writes what the backward call's first kernel
 * writes, which is a function of the forward call's columns alone, so a later backward call's outputs and the sampler's draws
 * do not change by a bit.  Staging is the backward call's and clears the error word; there is no size query of its own
 * (smm_align_graph_logz_workspace_bytes).
 * Numerics: the span sums as smm_align_logz_f64's second sweep (fp32 exponentials of fp64 differences, fp64 sums) with a second
 * accumulator; the sums over end nodes and predecessors exponentiate in fp64; E, S and every total in fp64.  Every sum is taken
 * in a fixed order, without atomics: two calls on the same inputs give the same bits.
 *   - A video whose logz_g is -inf has no alignment: h_out and its parts are NaN; the error word stays clear.
 *   - A NaN logz_g gives the same and sets the error word.  Videos beside such a video are not affected.
 * Enqueued on `stream` only; never synchronises; a video is never split.
 * Refusals: SMM_ERR_ARG for a NULL required pointer (logz_g and h_out included), non-monotone offsets or a video without nodes;
 * SMM_ERR_UNSUPPORTED for SMM_SHAPE_NO_EOS, more than SMM_MAX_TRANSCRIPT nodes in a video, c_max or k_rows beyond the compiled
 * kernels; SMM_ERR_WORKSPACE below smm_align_graph_logz_workspace_bytes -- all before anything is staged.
 */
int smm_align_graph_entropy_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                const double *elp, const double *trans, const double *init, const double *len_scores,
                                const double *endpen /* nullable */, const int32_t *node_class, const uint32_t *pred_mask,
                                const uint8_t *node_flags, const int64_t *node_offset_host, const double *logz_g /* dev [b] */,
                                double *h_out /* dev [b] */, double *h_parts /* dev [b][3]: end, span, pred; nullable */,
                                void *workspace, size_t workspace_bytes, void *stream);

/*
 * The exact posterior of each segment of given alignments under the transcript-graph posterior, and where each node's segment
 * starts and ends (csrc/smm_align_graph_segpost.hip: gathers over the columns, no recursion).  With the E and S of
 * smm_align_graph_entropy_f64 -- E[n][m], S[s][m]: the posteriors that a segment of node m ends at position n / starts at s --
 * the posterior that node m covers exactly the frames [s, e) is exp(h[s][m] + len[e-s][a_m] + q[e][m] - logZ_g).
 * Call order as smm_align_graph_entropy_f64: it follows smm_align_graph_logz_f64 on the same workspace and stream, launches the
 * backward call's first kernel itself for the q and bh columns, computes nothing of a gradient, and may run before, after or
 * between backward, sampler and entropy calls without changing a bit of theirs.  SMM_SHAPE_NO_EOS is refused as by its siblings.
 * It has no size query of its own: the workspace is smm_align_graph_logz_workspace_bytes'.
 *   class_map  dev int64 [n_groups][c_max + 1], the ids spans_in is written in                            (nullable: local ids)
 *   spans_in   dev int64 [n_sets][b][t_max + 1] and
 *   used_in    dev int32 [n_sets][node_offset_host[b]]: alignments as smm_align_graph_f64 and smm_align_graph_sample_f64 write
 *              them; the k-th span of a video belongs to its k-th used node in index order            (nullable, both or neither)
 *   seg_logp   dev fp64 [n_sets][b][t_max + 1]: at each span start log P(its node covers exactly [s, e)), e the next span
 *              start; 0.0 at the EOS position; -inf elsewhere                                          (nullable; needs spans_in)
 *   node_logp  dev fp64 [n_sets][node_offset_host[b]]: the same value per used node, -inf for the others (nullable; needs spans_in)
 *   end_mean, end_sd, start_mean, start_sd  dev fp64 [node_offset_host[b]], laid out like node_class: mean and standard
 *              deviation, in frames, of node m's end and start position under E[.][m] and S[.][m] given that the path crosses m;
 *              summed over the column's recorded range in a fixed order in fp64, the variance about the mean in a second pass;
 *              NaN where the node's mass is 0                                                          (each nullable)
 *   node_end_post, node_start_post  dev fp64 [node_offset_host[b]][t_max + 1]: the dense E and S, 0.0 outside a column's range.
 *              They cost 8 (t_max + 1) bytes per node each: 256 nodes at T = 10 000 are 20 MB per video  (each nullable)
 * An alignment the graph does not admit has probability 0: when a (set, video)'s number of spans differs from its number of
 * used nodes, when a span's class, after the class map, is not its node's, or when a span is longer than kw = kp - 1, that
 * set's video is -inf everywhere in seg_logp and node_logp, and no error is set.  A video whose logZ_g is -inf gets NaN (seg_logp:
 * at its positions 0 .. T) with the error word clear; a NaN logZ_g gives NaN with the error word set.
 * SMM_ERR_ARG when every output is NULL, when seg_logp or node_logp is given without spans_in and used_in, when only one of the
 * two is given, when n_sets <= 0 with them, and under smm_align_graph_entropy_f64's refusals.
 */
int smm_align_graph_segment_posteriors_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                           const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                           const double *elp, const double *trans, const double *init, const double *len_scores,
                                           const double *endpen /* nullable */, const int64_t *class_map /* nullable */,
                                           const int32_t *node_class, const uint32_t *pred_mask, const uint8_t *node_flags,
                                           const int64_t *node_offset_host, const double *logz_g /* dev [b] */,
                                           const int64_t *spans_in, const int32_t *used_in, int32_t n_sets,
                                           double *seg_logp, double *node_logp, double *end_mean, double *end_sd,
                                           double *start_mean, double *start_sd, double *node_end_post, double *node_start_post,
                                           void *workspace, size_t workspace_bytes, void *stream);

/*
 * The exact KL divergence and cross-entropy between two transcript-graph posteriors (csrc/smm_align_graph_kl.hip): per video
 * KL(p || q) = sum_y p(y) log( p(y) / q(y) ) and H(p, q) = -sum_y p(y) log q(y) in nats over the ALIGNMENTS y of the video to
 * its graph -- teacher against student, one EM epoch against the next, a model with narration constraints against one without.
 * What smm_kl_f64 is to smm_entropy_f64.  Both sides share the videos, lengths, class sets, span limit and graphs; each has its
 * own elp, tables and closing scores and the workspace of its own smm_align_graph_logz_f64 call.
 * The chain rule of relative entropy over the sampler's decisions, in smm_align_graph_entropy_f64's notation.  For a decision
 * with the candidates' weights w_p (p's columns and tables) and w_q (q's), m_. the largest finite weight of a side, and over
 * the candidates with e_p = exp(w_p - m_p) > 0:
 *   S_p = sum e_p,  S_q = sum exp(w_q - m_q) (every candidate: q's normaliser),  Y = sum e_p (w_q - w_p),  A_p = sum e_p (w_p - m_p)
 *   KLloc  = (m_q - m_p) + log S_q - log S_p - Y / S_p   clamped at 0;      Hloc_p = log S_p - A_p / S_p
 *   KL_end  = KLloc( gam[T][j] + closing_j : end(j) )
 *   KL_span = sum_j sum_{n in [lo_j, hi_j]}   E[n][j] KLloc( h[n-k][j] + len[k][a_j] : k = 1..min(kw, n) )
 *   KL_pred = sum_j sum_{s in [slo_j, shi_j]} S[s][j] KLloc( gam[s][i] + trans[a_j][a_i] : i in pred(j) )
 *   kl_out   = (KL_end + KL_span) + KL_pred;    kl_parts (nullable) = KL_end, KL_span, KL_pred per video; every term >= 0
 *   xent_out (nullable) = the same three sums of weight * (Hloc_p + KLloc)
 * E and S are p's posteriors exactly as the entropy kernel forms them.  A candidate with e_p > 0 whose w_q is -inf makes KLloc
 * +inf: an answer, not an error.  A candidate of p-weight 0 contributes nothing (never 0 * inf).  Both sides run the same
 * operations: bit-identical sides give exactly 0.0 in every part.  For a prefix trie KL_end is the KL between the two
 * posteriors over the candidates and kl_out - KL_end the expected KL of the boundaries given the candidate; a chain has
 * KL_end = KL_pred = 0.0 exactly.  q needs no backward pass; its elp and init are never read (they enter through its h and gam
 * columns only).
 * Call order: one smm_align_graph_logz_f64 per side on the same stream first, each on its own workspace; logz_g_p / logz_g_q
 * are their outputs.  The call stages p's workspace as the entropy call does (clearing its error word), launches
 * smm_align_graph_logz_bwd_f64's first kernel on it for p's q and bh columns, then one kernel of its own, one workgroup per
 * video.  q's workspace is ONLY READ: nothing is staged there and its error word is not touched.  Before any of q's columns
 * is read, the five ints each forward call recorded per column are compared: they are a function of graph, T and span limit
 * only, so a mismatch means that workspace_q belongs to other graphs -- that video gets NaN and the error word.  As the
 * entropy call, it may run before, after or between p's backward, sampler and entropy calls without changing a bit of theirs.
 * There is no size query of its own (smm_align_graph_logz_workspace_bytes, for either side).
 * Numerics: EVERY exponential is fp64, on both sides, the span sums included: fp32 exponentials leave about 1e-7 in
 * log S_q - log S_p, which is the whole value between two near-identical posteriors.  There is no fp32 path for Hloc_p, so
 * H(p, p) equals smm_align_graph_entropy_f64's value only to that kernel's own fp32 rounding (1e-5 relative).  Every sum is
 * taken in a fixed order, without atomics: two calls on the same inputs give the same bits.
 *   logz_g_p = -inf                      KL, cross-entropy and parts NaN; the error word stays clear
 *   logz_g_p or logz_g_q NaN             NaN; the error word (of p's workspace) is set
 *   logz_g_q = -inf, logz_g_p finite     +inf (q's columns are not read); the error word stays clear
 * Videos beside such a video are not affected.
 * Enqueued on `stream` only; never synchronises; a video is never split.
 * Refusals: SMM_ERR_ARG for a NULL required pointer (both logz_g, workspace_q and kl_out included), b = 0, non-monotone offsets
 * or a video without nodes; SMM_ERR_UNSUPPORTED for SMM_SHAPE_NO_EOS, more than SMM_MAX_TRANSCRIPT nodes in a video, c_max or
 * k_rows beyond the compiled kernels; SMM_ERR_WORKSPACE when either side is below smm_align_graph_logz_workspace_bytes -- all
 * before anything is staged.
 */
int smm_align_graph_kl_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                           const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                           const double *elp_p, const double *trans_p, const double *init_p, const double *len_scores_p,
                           const double *endpen_p /* nullable */, const double *logz_g_p /* dev [b] */,
                           void *workspace_p, size_t workspace_p_bytes,
                           const double *trans_q, const double *len_scores_q, const double *endpen_q /* nullable */,
                           const double *logz_g_q /* dev [b] */, const void *workspace_q, size_t workspace_q_bytes,
                           const int32_t *node_class, const uint32_t *pred_mask, const uint8_t *node_flags,
                           const int64_t *node_offset_host, double *kl_out /* dev [b] */, double *xent_out /* dev [b], nullable */,
                           double *kl_parts /* dev [b][3]: end, span, pred; nullable */, void *stream);

/*
 * The gradients of smm_align_graph_entropy_f64's and smm_align_graph_kl_f64's values with respect to p's tables
 * (csrc/smm_align_graph_entropy_bwd.hip): V = H(p) (smm_align_graph_entropy_bwd_f64) or H(p, q) / KL(p || q)
 * (smm_align_graph_kl_bwd_f64, `mode` = SMM_KL_BWD_CROSS_ENTROPY / SMM_KL_BWD_KL).  What smm_entropy_bwd_f64 and smm_kl_bwd_f64 are
 * to smm_entropy_f64 and smm_kl_f64.  Entropy regularisation of weakly supervised training, distillation of a teacher's
 * alignment posterior, cross-entropy against a constrained posterior.
 * In smm_align_graph_logz_f64's notation, an occurrence o is a span (node j, start s, end n = s + k), an edge (i -> j at
 * boundary s) or a start (node m at 0), with the log-weight under a side
 *   span   h[s][j] + len[k][a_j] + cum[n][a_j] + bg[n][j]
 *   edge   gam[s][i] + trans[a_j][a_i] - cum[s][a_j] + bh[s][j]
 *   start  init[a_m] + bh[0][m]
 * p(o) = exp(w_p(o) - logZ_p);  l(o) = -(w_q(o) - logZ_q) (the entropy: q = p), for the KL (w_p(o) - logZ_p) - (w_q(o) - logZ_q);
 *   dV / d theta = sum over the occurrences that read the entry of  p(o) ( l(o) + eta-(S_o) + eta+(E_o) - V )
 * S_o / E_o: the decision node in front of / behind o (span: start node (s, j) / end node (n, j); edge: end node (s, i) / start
 * node (s, j); start: none / start node (0, m)).  eta- is the chain rule of the value calls run as a message pass over the
 * sampler's decisions, eta+ the same over the decisions of the time-forward walk, read from the backward columns; with
 * L(c) = -log q_loc(c) of a candidate, for the KL log p_loc(c) - log q_loc(c):
 *   eta-S(0, j) = 0;  eta-S(s, j) = sum_{i in pred(j)} p(i | start (s, j)) [ L(i) + eta-E(s, i) ]
 *   eta-E(n, j) = sum_k p(k | end (n, j)) [ L(k) + eta-S(n-k, j) ];     V- = sum_{end(j)} p_end(j) [ L(j) + eta-E(T, j) ]
 *   eta+E(T, j) = 0;  eta+E(n, j) = sum_{m in succ(j)} p(m | end (n, j)) [ L(m) + eta+S(n, m) ]
 *   eta+S(s, m) = sum_k p(k | start (s, m)) [ L(k) + eta+E(s+k, m) ];   V+ = sum_{start(m)} p(start m) [ L(m) + eta+S(0, m) ]
 * V- = V+ = V.  Outputs: smm_align_graph_logz_bwd_f64's four layouts, times the upstream weight grad_out[i] (NULL: ones), summed
 * over each group's videos in video order; all four are overwritten entirely.  A span's term goes to g_elp on each of its
 * frames and to g_len[k][a_j], an edge's to g_trans[a_j][a_i], a start's to g_init[a_m]; there is no gradient for endpen.
 * value_out (nullable): V- per video.  The gradient with respect to q's tables needs no call of its own:
 * dH(p,q)/d theta_q = dKL/d theta_q = mu_q - mu_p from two smm_align_graph_logz_bwd_f64 calls.
 *   scratch   dev, smm_align_graph_entropy_bwd_scratch_bytes: per video five [M][T+1] blocks (the four etas and the occupancy
 *             differences), then the videos' parts of the tables, q's log Z as the call uses it, then V+ per video in its last
 *             b doubles; its contents need
 *             not be initialised.  The query is host arithmetic and returns 0 for whatever the calls refuse.
 * Call order: one smm_align_graph_logz_f64 per side on the same stream first, each on its own workspace.  The call stages p's
 * workspace as the backward call does (clearing its error word) and launches smm_align_graph_logz_bwd_f64's first kernel on it
 * (smm_launch_align_graph_logz_bwd_columns) for p's q and bh columns.  The gradient also needs q's q and bh columns, so
 * smm_align_graph_kl_bwd_f64 WRITES workspace_q: it launches that same kernel on it, with q's tables -- q's workspace receives
 * exactly what q's own smm_align_graph_logz_bwd_f64 call would write first, a function of q's forward columns alone; nothing is
 * staged there and its error word is not touched.  So q's later backward, sampler, entropy and KL results do not change by a
 * bit, nor do p's.  BEFORE that kernel runs on workspace_q, a kernel of one workgroup per video compares the five ints each
 * forward call recorded per column, as smm_align_graph_kl_f64 does: a video whose ranges differ (workspace_q was written for
 * other graphs) is skipped by the q-side launch and by every kernel behind it -- nothing of workspace_q is read or written
 * through ranges that were not compared --, gets the value NaN, contributes zeros, and sets the error word.  workspace_q must
 * not be workspace_p (SMM_ERR_ARG): one posterior against itself is smm_align_graph_entropy_bwd_f64.  Then five kernels of
 * its own: eta-, eta+, the assembly (one workgroup per video each), g_elp, and
 * the sums over the videos.
 * Numerics: every exponential is fp64 on both sides, in all three modes; every read of a column is gated by its recorded range;
 * a decision or an occurrence without mass under p is not evaluated.  No atomics, every sum in a fixed order: two calls give the
 * same bits.  Both sides run the same operations, so in KL mode bit-identical sides give exactly 0.0 in every output.
 *   logz_g_p = -inf                          value NaN, exactly zero contributions; the error word stays clear
 *   logz_g_p or logz_g_q NaN                 the same; the error word (of p's workspace) is set
 *   grad_out[i] = 0                          exactly 0.0 contributions
 *   a value of +inf (q excludes what p has)  NaN rows of g_elp for that video, NaN tables for its group
 * Videos beside such a video keep their bits.
 * Enqueued on `stream` only; never synchronises; a video is never split.
 * Refusals: as smm_align_graph_kl_f64's (a NULL gradient or scratch pointer included; an unknown `mode`; workspace_q equal to
 * workspace_p), and
 * SMM_ERR_WORKSPACE for a scratch below smm_align_graph_entropy_bwd_scratch_bytes -- all before anything is staged.
 */
size_t smm_align_graph_entropy_bwd_scratch_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                 const int64_t *node_offset_host);
int smm_align_graph_entropy_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                    const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                    const double *elp, const double *trans, const double *init, const double *len_scores,
                                    const double *endpen /* nullable */, const int32_t *node_class, const uint32_t *pred_mask,
                                    const uint8_t *node_flags, const int64_t *node_offset_host, const double *logz_g /* dev [b] */,
                                    const double *grad_out /* dev [b], nullable */, double *g_elp, double *g_trans, double *g_init,
                                    double *g_len, double *value_out /* dev [b], nullable */, void *scratch, size_t scratch_bytes,
                                    void *workspace, size_t workspace_bytes, void *stream);
int smm_align_graph_kl_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                               const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                               const double *elp_p, const double *trans_p, const double *init_p, const double *len_scores_p,
                               const double *endpen_p /* nullable */, const double *logz_g_p /* dev [b] */,
                               void *workspace_p, size_t workspace_p_bytes,
                               const double *trans_q, const double *len_scores_q, const double *endpen_q /* nullable */,
                               const double *logz_g_q /* dev [b] */, void *workspace_q, size_t workspace_q_bytes,
                               const int32_t *node_class, const uint32_t *pred_mask, const uint8_t *node_flags,
                               const int64_t *node_offset_host, int32_t mode, const double *grad_out /* dev [b], nullable */,
                               double *g_elp, double *g_trans, double *g_init, double *g_len,
                               double *value_out /* dev [b], nullable */, void *scratch, size_t scratch_bytes, void *stream);

/*
 * The expectation of a frame- and node-additive reward under the transcript-graph posterior, and its gradient with respect to
 * the tables (csrc/smm_align_graph_expected_reward.hip).  What smm_expected_reward_f64 / _bwd_f64 are to the unconstrained
 * posterior: the expected number of correct frames of an alignment against held-out labels or a teacher, the expected time in
 * a class, the expected number of segments (of optional entries used), a candidate's posterior on the end nodes of a trie --
 * each without committing to the best alignment, and each trainable.
 * For an alignment y (a start -> end path and the boundaries of its nodes' segments), in smm_align_graph_logz_f64's notation:
 *   R(y) = sum over the segments (node j, start s, end n) of y of ( node_reward[j] + sum_{t = s .. n-1} reward[t][a_j] )
 *   V    = E_{p(y | x, graph)}[ R(y) ]
 *   reward       dev fp64 [total_frames][c_max], local states as columns (the columns past a video's state count and the frames
 *                no video covers are not read); nullable
 *   node_reward  dev fp64, laid out like node_class; nullable -- but not both.  The EOS step carries no reward.
 * With cumW[n][c] = sum_{t < n} reward[t][c] per video, r(j, s, n) = node_reward[j] + cumW[n][a_j] - cumW[s][a_j], and the
 * value gathers smm_align_graph_segment_posteriors_f64's E (a segment of node j ends at n) and S (starts at s), no recursion:
 *   V = sum_j ( sum_n E[n][j] cumW[n][a_j] - sum_s S[s][j] cumW[s][a_j] )  +  sum_j node_reward[j] sum_n E[n][j]
 * value_out: dev [b]; parts_out (nullable): dev [b][2], the frame part and the node part.
 * The gradient is a Hessian-vector product of log Z_g, over smm_align_graph_entropy_bwd_f64's occurrences (span, edge, start):
 *   dV / d theta = sum over the occurrences o that read the entry of  p(o) ( r(o) + eta-(S_o) + eta+(E_o) - V )
 * r(o) = 0 for edges and starts; eta- / eta+ the expected reward in front of / behind a decision node, message passes over the
 * sampler's decisions and those of the time-forward walk:
 *   eta-S(0, j) = 0;  eta-S(s, j) = sum_{i in pred(j)} p(i | start (s, j)) eta-E(s, i)
 *   eta-E(n, j) = sum_k p(k | end (n, j)) [ r(j, n-k, n) + eta-S(n-k, j) ];     V- = sum_{end(j)} p_end(j) eta-E(T, j)
 *   eta+E(T, j) = 0;  eta+E(n, j) = sum_{m in succ(j)} p(m | end (n, j)) eta+S(n, m)
 *   eta+S(s, m) = sum_k p(k | start (s, m)) [ r(m, s, s+k) + eta+E(s+k, m) ];   V+ = sum_{start(m)} p(start m) eta+S(0, m)
 * V- = V+ = V up to rounding.  Outputs of the gradient call: smm_align_graph_logz_bwd_f64's four layouts, times the upstream
 * weight grad_out[i] (NULL: ones), summed over each group's videos in video order; all four are overwritten entirely.  There is
 * no gradient for endpen, and none for the rewards: V is linear in them, dV / d reward is smm_align_graph_logz_bwd_f64's g_elp
 * and dV / d node_reward its p_used.  value_out of the gradient call (nullable): dev [b][2], V- and V+.
 *   scratch   dev; its contents need not be initialised and are undefined after the call.
 *             smm_align_graph_expected_reward_scratch_bytes: the videos' cumW offsets [b], cumW ((T + 1) c_max doubles per
 *             video, class-major like cum), two partials per node.
 *             smm_align_graph_expected_reward_bwd_scratch_bytes: smm_align_graph_entropy_bwd_f64's layout (five [M][T+1] blocks
 *             per video, the videos' parts, V+), then the offsets and cumW.
 *             The queries are host arithmetic and return 0 for whatever the calls refuse.  smm_align_graph_logz_workspace_bytes
 *             does not change.
 * Call order: smm_align_graph_logz_f64 on the same workspace and stream first.  Both calls stage the workspace as the backward
 * call does (clearing its error word) and launch smm_align_graph_logz_bwd_f64's first kernel on it
 * (smm_launch_align_graph_logz_bwd_columns), which rewrites the q and bh columns with the same bits; they never launch its g_elp /
 * g_len / reduce kernels.  So they may run before, after or between the backward, sampler, entropy, segment-posterior, KL and
 * gradient calls without changing a bit of theirs.  Then the value call launches three kernels (prefix sums, one wave per node,
 * one wave per video), the gradient call the prefix sums, eta-, eta+, the assembly (one workgroup per video each) and
 * smm_align_graph_entropy_bwd_f64's last two kernels (g_elp, the sums over the videos).
 * Numerics: every exponential is fp64; each decision takes a maximum pass and a pass of exponentials, nothing is rescaled; every
 * read of a column is gated by its recorded range; a decision or an occurrence without mass is not evaluated.  No atomics,
 * every sum in a fixed order: two calls give the same bits.  The rounding of V scales with the sum of |reward| over the covered
 * entries plus the sum of |node_reward|.
 *   logz_g = -inf                            value NaN, exactly zero contributions; the error word stays clear
 *   logz_g NaN                               the same; the error word is set
 *   grad_out[i] = 0                          exactly 0.0 contributions
 *   a reward that is not finite, in a covered entry or on one of the video's nodes
 *                                            value NaN, NaN rows of g_elp for that video, NaN tables for its group; the error
 *                                            word is set
 * Videos beside such a video keep their bits.
 * Enqueued on `stream` only; never synchronises; a video is never split.
 * Refusals: smm_align_graph_entropy_bwd_f64's (SMM_SHAPE_NO_EOS: SMM_ERR_UNSUPPORTED), SMM_ERR_ARG when both rewards are NULL,
 * when value_out of the value call or a gradient pointer of the gradient call is NULL, or when the scratch is NULL, and
 * SMM_ERR_WORKSPACE for a scratch below its query -- all before anything is staged.
 */
size_t smm_align_graph_expected_reward_scratch_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                     const int64_t *node_offset_host);
size_t smm_align_graph_expected_reward_bwd_scratch_bytes(const smm_shape *shape, const int64_t *lengths_host,
                                                         const int64_t *node_offset_host);
int smm_align_graph_expected_reward_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                        const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                        const double *elp, const double *trans, const double *init, const double *len_scores,
                                        const double *endpen /* nullable */, const int32_t *node_class, const uint32_t *pred_mask,
                                        const uint8_t *node_flags, const int64_t *node_offset_host, const double *logz_g /* dev [b] */,
                                        const double *reward /* nullable */, const double *node_reward /* nullable */,
                                        double *value_out /* dev [b] */, double *parts_out /* dev [b][2], nullable */,
                                        void *scratch, size_t scratch_bytes, void *workspace, size_t workspace_bytes, void *stream);
int smm_align_graph_expected_reward_bwd_f64(const smm_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                                            const int32_t *group_host, const int32_t *kp_host, const int32_t *n_states_host,
                                            const double *elp, const double *trans, const double *init, const double *len_scores,
                                            const double *endpen /* nullable */, const int32_t *node_class,
                                            const uint32_t *pred_mask, const uint8_t *node_flags, const int64_t *node_offset_host,
                                            const double *logz_g /* dev [b] */, const double *reward /* nullable */,
                                            const double *node_reward /* nullable */, const double *grad_out /* dev [b], nullable */,
                                            double *g_elp, double *g_trans, double *g_init, double *g_len,
                                            double *value_out /* dev [b][2]: V-, V+; nullable */, void *scratch,
                                            size_t scratch_bytes, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Factor tables of every parameter group from the model parameters (training steps), and their chain rule.
 * One launch each instead of the differentiable torch ops behind initial_log_probs (modules:284-296),
 * transition_log_probs (:298-322), _length_log_probs_with_rates (:383-414) and the expanded emission_log_probs
 * (:324-381); layouts as the entry points above read them, columns past a group's state count are 0.
 * Every pointer is a DEVICE pointer; nothing is staged and the host never waits.
 *   parameters: init_logits [n], transition_logits [n][n] ([to][from]), poisson_log_rates [n], gaussian_means [n][d],
 *               gaussian_cov [d][d] (its diagonal: tied diagonal covariance), fp32 like the reference's nn.Parameters
 *   init_constraints [n] / transition_constraints [n][n]: bytes, 1 = forbidden (set_transition_constraints,
 *               modules:160-193), or NULL
 *   classes [g][c_max]: class id of each local state (valid_classes);  merged [g][c_max]: its parameter row after
 *               merge_classes;  n_states [g] int32
 * smm_factor_tables_bwd_f64: g_* of the tables in (NULL = no gradient through that table; g_w_class_major is
 * [g][c_max][d], smm_emission_bwd_f64's layout), fp64 gradients of the parameters out (overwritten; sums over groups
 * leave through fp64 atomics).  trans / init: the forward call's outputs.
 */
typedef struct smm_tables_shape {
    int32_t n_classes, d, n_groups, c_max, k_rows;
    int32_t allow_self_transitions;
} smm_tables_shape;
int smm_factor_tables_f64(const smm_tables_shape *shape, const float *init_logits, const float *transition_logits,
                          const float *poisson_log_rates, const float *gaussian_means, const float *gaussian_cov,
                          const uint8_t *init_constraints, const uint8_t *transition_constraints,
                          const int64_t *classes, const int64_t *merged, const int32_t *n_states,
                          double *trans, double *init, double *len_scores, double *w, double *cst, double *inv_var,
                          void *stream);
int smm_factor_tables_bwd_f64(const smm_tables_shape *shape, const float *poisson_log_rates, const float *gaussian_means,
                              const float *gaussian_cov, const uint8_t *init_constraints,
                              const uint8_t *transition_constraints, const int64_t *classes, const int64_t *merged,
                              const int32_t *n_states, const double *trans, const double *init,
                              const double *g_trans, const double *g_init, const double *g_len,
                              const double *g_w_class_major, const double *g_cst,
                              double *g_init_logits, double *g_transition_logits, double *g_poisson_log_rates,
                              double *g_gaussian_means, void *stream);

/*
 * The reference's inner boundary as it stands: semiring DP over DENSE potentials, for lattices small enough to be
 * materialised (reference defaults).  Replaces torch_struct.SemiMarkovCRF(scores, lengths).argmax + from_parts
 * (semiring = 0, max) and .partition (semiring = 1, log) -- call sites semimarkov_modules.py:624, 657, 677-679,
 * src/models/test_semimarkov.py:312-314.
 *   scores   dev fp32 [b][n1][k][c][c] indexed [n][k][c_to][c_from];  lengths_host[b] = positions (max == n1 + 1)
 *   v        dev fp64 [b];  spans dev int64 [b][n1 + 1] (max semiring only, nullable)
 */
size_t smm_dense_workspace_bytes(int32_t b, int32_t n1, int32_t k, int32_t c);
int smm_dense_dp_f32(const float *scores, const int64_t *lengths_host, int32_t b, int32_t n1, int32_t k, int32_t c,
                     int32_t semiring, double *v, int64_t *spans, void *workspace, size_t workspace_bytes, void *stream);
/* Posterior edge marginals of the dense lattice = d sum_i grad_v[i] * logZ_i / d scores -- the gradient the reference
 * obtains by autograd through torch_struct's LogSemiring DP (src/models/semimarkov/semimarkov.py:286 through
 * semimarkov_modules.py:624-657).  Must follow smm_dense_dp_f32(semiring = 1) on the same scores with the SAME
 * workspace (its forward messages are read from there); v = that call's output.
 *   grad_v     dev fp64 [b] upstream gradient (NULL = ones)
 *   marginals  dev fp32 [b][n1][k][c][c], overwritten (0 outside each instance's lattice) */
int smm_dense_marginals_f32(const float *scores, const int64_t *lengths_host, int32_t b, int32_t n1, int32_t k, int32_t c,
                            const double *v, const double *grad_v, float *marginals,
                            void *workspace, size_t workspace_bytes, void *stream);

/*
 * Evaluation counters of decoded frame labels against ground truth -- the per-frame loops of the reference's
 * src/evaluation/accuracy.py as driven by Datasplit.accuracy_corpus (src/data/corpus.py:486-565).  Integer work only;
 * the label assignment (identity / Hungarian on the confusion table) and the final ratios are the caller's.
 *   pred        dev int64 [total_frames]            global class ids (what smm_decode_f32 writes to `labels`)
 *   gt          dev int64 [total_frames][gt_width]  ground-truth ids, first column = "the" label, -1 = no further label
 *   local_of    dev int32 [n_groups][n_labels]      global id -> local id in [0, c_max) of the video's task, -1 = not
 *                                                   in the task (such frames are counted under local id c_max)
 * smm_eval_confusion_i64  (accuracy.py:232-283 voting table, :500-521 per-class masks)
 *   confusion   dev int64 [n_groups][c_max+1][c_max+1]  frames with (first gt label, predicted label); overwritten
 * smm_eval_videos_i64     (accuracy.py:538-576 frame loop, :21-37 + :364-408 run lengths and edit distance,
 *                          :410-472 step recall)
 *   video_key   host int32 [b] index of the video inside its task (seeds the random frame draw; NULL: i)
 *   cluster_of  dev int32 [n_groups][c_max+1]      local gt id -> predicted label that it owns after assignment, as a
 *                                                  local id, or c_max+1+j for an invented label j, or -1 (none)
 *   gt_is_bg    dev uint8 [n_groups][c_max+1]      local gt id is a background class
 *   pred_is_bg  dev uint8 [n_groups][2*(c_max+1)]  (extended) predicted id is owned by a background class
 *   seed        the frame drawn for `single_step_recall` is the candidate with the smallest hash(seed, key, t)
 *   counters    dev int64 [b][SMM_EVAL_COUNTERS]   per video, indexed by smm_eval_counter; overwritten
 */
#define SMM_EVAL_MAX_LABELS 63
#define SMM_EVAL_COUNTERS 32
typedef enum smm_eval_counter {
    SMM_EV_FRAMES = 0, SMM_EV_SEGS_GT = 1, SMM_EV_SEGS_PRED = 2, SMM_EV_SEGS_PRED_NON_BG = 3,
    SMM_EV_MULTI = 4,            /* frames with more than one gt label */
    SMM_EV_GT_LABELS = 5,        /* sum of gt labels per frame (recall denominator) */
    SMM_EV_TP = 6,               /* prediction owned by one of the frame's gt labels */
    SMM_EV_PRED_BG = 7, SMM_EV_TRUE_BG = 8,
    SMM_EV_IOU_DEN = 9, SMM_EV_IOU_NUM = 10,          /* frames not (gt bg and pred bg); of those, true positives */
    SMM_EV_GT_LABELS_NON_BG = 11, SMM_EV_FRAMES_NON_BG = 12, SMM_EV_TP_NON_BG = 13,
    SMM_EV_STEPS = 14, SMM_EV_STEPS_NON_BG = 15,      /* distinct (remapped) gt labels of the video */
    SMM_EV_DRAW_HIT = 16, SMM_EV_DRAW_HIT_NON_BG = 17, SMM_EV_MID_HIT = 18, SMM_EV_MID_HIT_NON_BG = 19,
    SMM_EV_TYPES = 20, SMM_EV_TYPES_NON_BG = 21,      /* distinct predicted labels */
    SMM_EV_OTHER = 22,           /* labels outside the task's table (must be 0 for the statistics to be meaningful) */
    SMM_EV_LEVENSHTEIN = 23
} smm_eval_counter;

typedef struct smm_eval_shape {
    int32_t b;          /* videos */
    int32_t n_groups;   /* tasks */
    int32_t c_max;      /* local label ids per task, <= SMM_EVAL_MAX_LABELS */
    int32_t n_labels;   /* size of the global label space */
    int32_t gt_width;   /* ground-truth labels per frame (>= 1) */
    int32_t t_max;      /* max lengths[i] */
    int64_t total_frames;
} smm_eval_shape;

size_t smm_eval_workspace_bytes(const smm_eval_shape *shape, const int64_t *lengths_host);
int smm_eval_confusion_i64(const smm_eval_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                           const int32_t *group_host, const int64_t *pred, const int64_t *gt, const int32_t *local_of,
                           int64_t *confusion, void *workspace, size_t workspace_bytes, void *stream);
int smm_eval_videos_i64(const smm_eval_shape *shape, const int64_t *lengths_host, const int64_t *frame_offset_host,
                        const int32_t *group_host, const int32_t *video_key_host, const int64_t *pred, const int64_t *gt,
                        const int32_t *local_of, const int32_t *cluster_of, const uint8_t *gt_is_bg,
                        const uint8_t *pred_is_bg, uint32_t seed, int64_t *counters,
                        void *workspace, size_t workspace_bytes, void *stream);

/*
 * Sufficient statistics of the closed-form supervised fit -- semimarkov_utils.semimarkov_sufficient_stats
 * (reference src/models/semimarkov/semimarkov_utils.py:74-126) as consumed by SemiMarkovModule.fit_supervised
 * (semimarkov_modules.py:195-256).  One pass over the features (HBM-bound).
 *   x        dev fp32 [total_frames][d];  labels dev int64 [total_frames] global class ids in [0, n_classes)
 *   max_k    --sm_max_span_length: a run of one label counts as spans of at most max_k - 1 frames
 *            (labels_to_spans, utils.py:6-23); <= 0: runs are never cut
 *   sum_x    dev fp64 [n_classes][d]  per-class feature sums;   sum_x2 dev fp64 [d]  sum of squares over all frames
 *   frame_counts / span_counts / span_start_counts dev int64 [n_classes];
 *   span_transition_counts dev int64 [n_classes][n_classes] indexed [to][from]            (all outputs overwritten)
 * The int32 at smm_fit_error_word_offset(b) in the workspace is non-zero when a label was outside [0, n_classes).
 */
size_t smm_fit_workspace_bytes(int32_t b);
size_t smm_fit_error_word_offset(int32_t b);
int smm_fit_stats_f64(int32_t b, const int64_t *lengths_host, const int64_t *frame_offset_host, int64_t total_frames,
                      int32_t d, int32_t n_classes, int32_t max_k, const float *x, const int64_t *labels,
                      double *sum_x, double *sum_x2, int64_t *frame_counts, int64_t *span_counts,
                      int64_t *span_start_counts, int64_t *span_transition_counts,
                      void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SMMDP_H */
