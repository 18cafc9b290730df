/* tip_hip.h — C-ABI of the MI355X-native TIP forward pass (libtip_hip.so).
 *
 * The reference has no FFI layer: its boundary for this path is the Python nn.Module
 * `TF_RNN_Past_State` (/root/reference/simple_transformer_with_state.py:8-102).  Each entry point below
 * names the piece of that interface it replaces; the Python host in
 * transformer-inertial-poser_amd/simple_transformer_with_state.py binds them with ctypes.
 *
 * Conventions: plain C, no torch types, no exceptions; every function returns 0 or a negative
 * tip_status; device pointers are caller-owned, contiguous, row-major fp32; tip_forward is asynchronous on
 * the caller's HIP stream; one handle per GPU, used from one thread at a time; the library allocates no
 * device memory (packed weights and workspace are caller-provided buffers; the one allocation is a 64-byte pinned HOST
 * block per handle, the hand-off error word of tip_check).  Arithmetic is fp32; the reference's `--double` switch
 * (train_model.py:84-85) is served by tip_forward_f64 (fp64 parameters and windows, every operation in IEEE double) for the
 * forward and by tip_train_forward_f64 / tip_train_backward_f64 for the training step.  Tensors are never converted silently.
 */
#ifndef TIP_HIP_H
#define TIP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TIP_ABI_VERSION 5 /* 2: packed image without the exploratory split-fp16 section unless asked for (TIP_CREATE_S16, tip_create_ex);
                             tip_max_batch; export list = this header (+ tip_hip_debug.h), everything else hidden
                             3: tip_forward_dropout, tip_draw_keep_mask, tip_train_input_grads; plan 9 (persistent latency kernel) and its 1 KiB of sync words in the packed image
                             removed; TIP_OPT_FUSE_HEAD reserved
                             4: plans 5 / 7 / 8 (pair-split, split-fp16) and TIP_OPT_PACK_SPLIT16 retired (and the split-fp16 trace hook of tip_hip_debug.h with them)
                             5: exact streaming reuse — tip_reuse_cache_bytes, tip_reuse_reset, tip_forward_reuse, tip_stream_frame_counter_offset,
                                tip_stream_ingest_newest; later, backward compatible: tip_forward_rows and the staggered streaming entry points
                                (tip_stream_attach, tip_stream_detach, tip_stream_ingest_staggered, tip_stream_consume_staggered,
                                tip_stream_ingest_mapped, tip_stream_consume_mapped); the model shapes of the streaming entry points
                                (tip_stream_reset_shaped) and the host override of the fed-back pose (tip_stream_history_override); the deployed forward at any
                                batch and its device seeds (tip_forward_live, tip_seeds_next); the streaming entry points at any window
                                length (the tip_stream_*_w family); device-fed replay of recordings (tip_replay_feed, tip_replay_collect) */

/* The library is built with -fvisibility=hidden: the functions declared here (and the measurement hooks of
 * tip_hip_debug.h) are its whole dynamic symbol table (tests/test_host_cpu.py compares `nm -D` with the two headers). */
#define TIP_API __attribute__((visibility("default")))

typedef struct tip_handle tip_handle;
typedef void* tip_stream_t; /* hipStream_t */

/* Constructor arguments of TF_RNN_Past_State (simple_transformer_with_state.py:9-17). */
typedef struct tip_config {
    int32_t input_size_imu;  /* 72 */
    int32_t size_s;          /* 131 */
    int32_t rnn_hid_size;    /* 512 */
    int32_t tf_hid_size;     /* 1024 (dim_feedforward) */
    int32_t tf_in_dim;       /* 256  (d_model) */
    int32_t n_heads;         /* 16 */
    int32_t tf_layers;       /* 4 */
    int32_t with_rnn;        /* :15 */
    int32_t with_acc_sum;    /* :16  (+18 input columns, :20-22) */
    int32_t t_max;           /* typical longest window (40; 80 for the scaled config): a sizing hint only — tip_forward serves any
                                T >= 1 (the reference builds its causal mask for any length, :56-58,85); T > 128 takes the key-tiled
                                attention of the general plan */
} tip_config;

typedef enum tip_status {
    TIP_OK = 0,
    TIP_ERR_INVALID_ARG = -1,
    TIP_ERR_UNSUPPORTED_CONFIG = -2,
    TIP_ERR_NOT_READY = -3,      /* tip_forward before tip_attach_packed */
    TIP_ERR_WORKSPACE = -4,      /* workspace too small / misaligned */
    TIP_ERR_HIP = -5,            /* a HIP runtime call failed; see tip_last_hip_error */
    TIP_ERR_NO_DEVICE = -6,
    TIP_ERR_ALLOC = -7,
    TIP_ERR_HANDOFF = -8         /* an inter-workgroup hand-off wait of an EARLIER launch gave up (see tip_check) */
} tip_status;

/* tip_forward flags */
#define TIP_FWD_LAST_ROW_ONLY 0x1 /* y is [B, size_s] = row T-1 of every window: what RTRunnerMin.step consumes
                                     (real_time_runner_minimal.py:150) */
#define TIP_FWD_KEEP_MASK     0x2 /* keep_mask [B,T,size_s] supplied: x_s * mask * keep_scale, replaces the Bernoulli
                                     draw of nn.Dropout(past_state_dropout) (simple_transformer_with_state.py:77) */

/* execution plans (tip_set_option(TIP_OPT_PLAN, ...)) */
#define TIP_PLAN_AUTO    0
#define TIP_PLAN_GENERAL 1 /* layer-by-layer MFMA GEMM kernels, any configuration */
#define TIP_PLAN_FUSED   2 /* one workgroup = one window through all encoder layers (paper configuration) */
#define TIP_PLAN_FUSED2  4 /* two windows per workgroup (80 rows = 5 MFMA row blocks, no padding); AUTO picks it for
                              B >= 2 x CUs; bit-identical results to TIP_PLAN_FUSED */
/* plan value 5 is RETIRED (rounds 1-5: TIP_PLAN_FUSED2S, a window pair on two co-resident workgroups; superseded by TIP_PLAN_FUSEDH
   and TIP_PLAN_FUSED1S, removed in round 6): tip_set_option answers TIP_ERR_UNSUPPORTED_CONFIG */
#define TIP_PLAN_FUSEDH  6 /* TIP_PLAN_FUSED with a hybrid row tiling: rows 0-31 on 16x16x4 MFMAs, rows 32-39 on 4x4x1 MFMAs fed by the
                              same weight fragments — no matrix-core work on the pad rows 40-47 outside the QKV projection.  No
                              inter-workgroup hand-off in the encoder.  Rows 0-31 bit-identical to TIP_PLAN_FUSED. */
/* plan values 7 and 8 are RETIRED (rounds 3-5: exploratory split-fp16 emulation of the fp32 GEMM operands — narrower arithmetic than the
   reference's fp32, never a default; removed in round 6): tip_set_option answers TIP_ERR_UNSUPPORTED_CONFIG */
#define TIP_PLAN_LATENCY 3 /* one window spread over up to 64 CUs per stage + GEMV-cluster RNN (paper config, B <= 64);
                              AUTO picks it for B <= 32 (up to 48 where four CUs per window are not to be had, and up to 64 where
                              TIP_PLAN_FUSED1S does not apply: T < 40) */

#define TIP_PLAN_FUSED1S 10 /* window-split: ONE window on TWO co-resident workgroups of one XCD — a column split with two partial-sum
                               hand-offs at 48 rows (3/5 of the matrix work per workgroup) — for batches that leave at least half of the
                               CUs idle: needs 2 B <= #CUs and B <= 128.  Its own summation order (K-halves of out-proj / linear2 summed
                               across the partners).  While 4 B <= #CUs (and B <= 64) the window is carried by FOUR workgroups instead (quads
                               of heads, quarters of the hidden units and of the RNN input projection; partial sums added p0 + p1 + p2 + p3
                               in every partner; TIP_OPT_F1S_PARTS pins the form) — the two forms differ in summation order, each is
                               deterministic.  AUTO picks it for 32 < B <= #CUs / 2 at T = 40 and for remainders of 33-128 windows behind
                               whole rounds. */
/* plan value 9 is RESERVED (rounds 4: TIP_PLAN_LATENCY1, the latency chain as one persistent kernel — bit-identical, measured slower
   than the launch chain at every batch size, removed in round 5): tip_set_option rejects it */

#define TIP_OPT_PLAN        1
#define TIP_OPT_PROFILE     2 /* 0 off; 1: bracket every stage with a HIP event pair; 2: only the dominant stage; 3: the dominant
                                 stage of every fourth forward (a pair costs ~7 us of queue barriers per step at B = 256: this is
                                 the form a timed region carries).  Setting it resets the accumulated times. */
#define TIP_OPT_RNN_CLUSTER 3 /* workgroups cooperating on one RNN window-tile (1,2,4,8,16); 0 = auto */
#define TIP_RNN_CLUSTER_ROWS4 0x44 /* TIP_OPT_RNN_CLUSTER value: 4-window tiles on 4-workgroup clusters (4x4x1 MFMAs; rnn_hidden 512 only) */
#define TIP_OPT_FAULT_INJECT 4 /* TESTS ONLY.  Bit 0: the window-split encoder drops one workgroup of its first window; bit 1: the clustered
                                 RNN drops member 1 of its first cluster; bit 2: the latency plan's GEMV RNN drops member 1 of
                                 stream 0.  The partners' waits then MUST give up (after a shortened spin): the error path of
                                 tip_check is exercised deterministically.  Bit 3: nobody is dropped, but every cooperating kernel
                                 treats its partners as sitting on DIFFERENT XCDs (agent-scope stores, L1-bypassing loads, paced
                                 polls) wherever they really are: the path a placement across XCDs takes, bit-identical results.
                                 Bit 4: in the one-launch few-stream form one producer of window 0 stamps its completion flag as a
                                 workgroup on ANOTHER XCD would (what kernels of a foreign stream running beside it can cause): its
                                 consumers give up at once and report TIP_OPT_HANDOFF_KIND = 2.  0 = off (default). */

#define TIP_OPT_FUSE_HEAD 5 /* RESERVED: accepted (0 / 1) and ignored.  Rounds 3-4: the output projection as the epilogue of the recurrence
                               kernel (measured neutral, removed in round 5); round 5: the projection inside the recurrence's hop wait
                               with an L2-ring hand-off (correct, measured slower than the separate kernels: CHANGELOG.md). */

/* option 6 is RETIRED (rounds 3-5: TIP_OPT_PACK_SPLIT16, the split-fp16 sections of the packed image): TIP_ERR_INVALID_ARG */
#define TIP_OPT_AUTO_DEMOTE 7 /* 1 (default): hosts may answer the first TIP_ERR_HANDOFF of this handle by demoting it (TIP_OPT_DEMOTED)
                                 and re-issuing the call; 0: they report the error.  A flag for the host layer (the library itself never
                                 re-issues a call); the Python host honours it. */
#define TIP_OPT_DEMOTED     8 /* 1: TIP_PLAN_AUTO and the automatic TIP_OPT_RNN_CLUSTER choose only kernels WITHOUT inter-workgroup hand-offs
                                 (hybrid one-window / two-window encoder or the general plan, single-workgroup recurrence tiles): no
                                 co-residency needed, a co-tenant costs throughput instead of frames.  Explicit plans / cluster sizes are
                                 still honoured.  The training step's two recurrences likewise run on single-workgroup tiles.  Default 0. */
#define TIP_OPT_NO_FLOW    10 /* 1: the few-stream plan never takes its ONE-launch form (B <= 24: stages, recurrence and projection as roles of one
                                 launch, every workgroup of a window on the window's XCD) but the launch chain for every batch it serves —
                                 what a host answers a placement loss with (TIP_OPT_HANDOFF_KIND = 2: kernels of another stream were
                                 dispatched beside the launch and broke the id mod 8 = XCD rule).  The chain needs co-residency only.
                                 Default 0. */
#define TIP_OPT_HANDOFF_KIND 11 /* READ ONLY (tip_get_option): what the sticky hand-off word of tip_check says.  0: nothing pending; 1: a
                                 cooperating kernel's wait gave up (co-residency lost: the answer is TIP_OPT_DEMOTED); 2: only the
                                 one-launch few-stream form found a producer on another XCD (the answer is TIP_OPT_NO_FLOW). */
#define TIP_OPT_NO_ROUND_LAUNCH 12 /* 1: a batch of at most one window per CU on the hybrid encoder (TIP_PLAN_FUSEDH chosen or pinned, rnn_hidden 512,
                                 state width 129..131, T <= 40) runs as the three launches encoder / recurrence / projection; 0: as ONE
                                 launch whose workgroups stay on as recurrence members and projection (same bits; needs the whole
                                 grid co-resident, else the three launches are taken; never on a demoted handle, and not under
                                 TIP_OPT_PROFILE = 1: a stage is a launch.  Under TIP_OPT_PROFILE = 2 / 3 the "fused_encoder" pair then
                                 brackets the whole launch, recurrence and projection phases included).  Default 0: B = 256, T = 40
                                 0.613-0.616 ms per step against 0.621-0.623 (CHANGELOG.md). */
#define TIP_OPT_F1S_PARTS   9 /* workgroups that share ONE window under TIP_PLAN_FUSED1S: 2, 4, or 0 (default) = four while 4 B <= #CUs and
                                 B <= 64, two otherwise.  An explicit 4 outside that range is TIP_ERR_UNSUPPORTED_CONFIG at the forward. */

/* ---- lifetime: replaces TF_RNN_Past_State.__init__ (simple_transformer_with_state.py:9-54) ---------------- */
TIP_API int tip_abi_version(void);
TIP_API int tip_create(const tip_config* cfg, tip_handle** out);
TIP_API void tip_destroy(tip_handle* h);
TIP_API const char* tip_strerror(int status);
TIP_API const char* tip_last_hip_error(const tip_handle* h);
TIP_API int tip_set_option(tip_handle* h, int option, int value);
TIP_API int tip_get_option(const tip_handle* h, int option, int* value);

/* ---- parameters: replaces state_dict()/load_state_dict() (train_model.py:109-111,220-225;
 *      offline_testing_simple.py:96).  Tensor i is the i-th entry of the reference's state_dict(), same shape. */
TIP_API int tip_num_tensors(const tip_handle* h);
TIP_API int tip_tensor_info(const tip_handle* h, int i, const char** name, int* rows, int* cols /* 0 for 1-D */);
/* size of the packed weight image (padded / permuted / folded copy the kernels read) */
TIP_API int tip_packed_bytes(const tip_handle* h, size_t* bytes);
/* host: build the packed image from the n state-dict tensors (host pointers, fp32, reference layout).
 * Folds applied here: channel shuffle :88-89 into in_linear rows; root-velocity zeroing :75 into in_linear
 * columns; 1/sqrt(d_head) into W_q/b_q when exact; b_ih + b_hh; MFMA-fragment ordering of W_hh. */
TIP_API int tip_pack_weights(const tip_handle* h, const float* const* host_tensors, int n, void* packed_host_out, size_t bytes);
/* device: point the handle at a packed image resident in HBM (caller-owned; e.g. the buffer every rank
 * receives from the one-time RCCL broadcast).  Must stay valid until the next attach / destroy. */
/* tip_pack_weights on the GPU: `tensors` are DEVICE pointers (the live parameters), `packed_dev` a device buffer of
 * tip_packed_bytes(); asynchronous on `stream`.  Bit-identical image; microseconds instead of a host pack + 27 MB upload. */
TIP_API int tip_pack_weights_device(const tip_handle* h, const float* const* tensors, int n, void* packed_dev, size_t bytes,
                            tip_stream_t stream);
TIP_API int tip_attach_packed(tip_handle* h, const void* packed_device, size_t bytes);

/* ---- forward: replaces TF_RNN_Past_State.forward(x_imu, x_s) (simple_transformer_with_state.py:60-102) ---- */
/* Scratch of one forward, 256-byte aligned, caller-owned; its contents need not survive between calls (the caller may reuse the
 * memory for anything).  Two forwards in flight must not share one (the library serialises forwards of different streams on the
 * device, but see the module's per-stream buffers).  For the paper configuration the first 1.06 MiB hold the completion flags and
 * launch counters of the one-launch few-stream plan (B <= 24): a flag counts as set only if it equals a 56-bit stamp (per-handle
 * nonce + a hash of the area's address + the counter kept in the same area), so stale or foreign contents are harmless — the same
 * handle's own flags of an earlier workspace at another address included (a host whose buffer grows moves it through recycled
 * memory); the area sits at offset 0 for every (B, T), so that a workspace used with changing batch sizes / window lengths keeps
 * its counters. */
TIP_API int tip_workspace_bytes(const tip_handle* h, int B, int T, size_t* bytes);
/* largest batch one tip_forward (fp64 = 0) / tip_forward_f64 (fp64 = 1) call serves at window length T (32-bit buffer offsets
 * and grid limits); beyond it the calls return TIP_ERR_UNSUPPORTED_CONFIG.  Windows are independent (:60-102 has no op across
 * batch elements): a host runs a larger batch as chunks of at most this size. */
TIP_API int tip_max_batch(const tip_handle* h, int T, int fp64, int* max_batch);
/* x_imu [B,T,input_size_imu(+18)], x_s [B,T,size_s] (NaNs allowed, :65), y [B,T,size_s] (or [B,size_s] with
 * TIP_FWD_LAST_ROW_ONLY).  Inputs are not modified (:63-64).  keep_mask may be NULL. */
TIP_API int tip_forward(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, int flags,
                const float* keep_mask, float keep_scale, void* workspace, size_t workspace_bytes,
                tip_stream_t stream);
/* One output row per window, chosen per window: y [B,size_s], y[b] = row rows[b] of window b, rows a DEVICE int [B] read once per
 * window.  Bit-identical to tip_forward(...)[b, rows[b]] on the same plan (and with rows[b] == T-1 everywhere to
 * TIP_FWD_LAST_ROW_ONLY): plan choice, chunking limit (tip_max_batch), keep mask, CU-masked streams, a demoted handle and HIP-graph
 * capture behave as in tip_forward; only the output projection's row addressing differs (flags as tip_forward's; the last-row flag
 * is implied).  rows[b] outside [0, T) gives an all-NaN row ("no value"); nothing outside the window is read for it.
 * Finite padding: attention is causal and the recurrence runs forward, so row r of a window depends on rows 0 .. r only — but only
 * while the later rows are FINITE.  The diagonal attention tile multiplies masked probabilities (exact 0) with the V rows of later
 * keys, and 0 * NaN = NaN: a NaN or Inf in a later row spreads into earlier ones.  Pad a short window with zeros (the staggered ingest
 * below does). */
TIP_API int tip_forward_rows(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, const int* rows, int flags,
                     const float* keep_mask, float keep_scale, void* workspace, size_t workspace_bytes, tip_stream_t stream);

/* The forward WITH the training step's encoder dropout and WITHOUT its activation stash: what a `.train()`-mode module computes when
 * nobody differentiates it — the unedited reference runner (offline_testing_simple.py:98 never calls .eval();
 * real_time_runner_minimal.py:149).  Few streams only: the configurations TIP_PLAN_LATENCY serves (paper configuration, B <= 64,
 * T <= 40), on that plan's kernels with the four dropout sites of every encoder layer live; TIP_ERR_UNSUPPORTED_CONFIG otherwise
 * (and on a demoted handle): the caller then takes tip_train_forward.  The keep decisions are tip_train_forward's for the same
 * (p_drop, seed) — same hash, same element indices — so a later tip_train_forward(same arguments) + tip_train_backward differentiates
 * exactly the function evaluated here (the Python module does that when .backward() is called after all).  Uses the ATTACHED packed
 * image like tip_forward; flags / workspace as tip_forward.  Past-state dropout (:77): an explicit keep_mask (TIP_FWD_KEEP_MASK), or
 * p_state > 0 with keep_mask NULL — the mask is then drawn inside the first kernel from (p_state, state_seed), the same decisions
 * tip_draw_keep_mask(p_state, state_seed, ...) writes out as a [B,T,size_s] tensor of 0 / 1 (for the tip_train_forward that a later
 * backward needs); kept values are scaled by keep_scale either way. */
TIP_API int tip_forward_dropout(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, int flags,
                        const float* keep_mask, float keep_scale, float p_state, unsigned long long state_seed, float p_drop,
                        unsigned long long seed, void* workspace, size_t workspace_bytes, tip_stream_t stream);
/* mask[i] = 1 (keep) or 0 for i < n: the counter-based hash of the training step at site 0xFFFFFFF0, drop probability p_state in [0, 1) */
TIP_API int tip_draw_keep_mask(float p_state, unsigned long long state_seed, float* mask, size_t n, tip_stream_t stream);

/* The deployed forward at ANY batch: the function tip_forward_dropout computes (encoder dropout at p_drop under `seed`, past-state keep
 * mask at p_state under `state_seed` or an explicit keep_mask, nothing stashed), for every B up to tip_max_batch and with
 * tip_forward_rows' output forms (rows NULL: flags decide between the full output and the last row; rows non-NULL: one chosen row per
 * window, NaN for an index outside [0, T)).  Every shipped loader of the reference builds the model with past_state_dropout = 0.8 and
 * never calls .eval(): this is what such a runner evaluates, whatever the size of its pool.
 * Plan: the few-stream latency plan where tip_forward_dropout takes it (B <= 64, T <= 40, handle not demoted); otherwise ONE launch
 * sequence — the one-window hybrid encoder in its live mode (the training instantiation's four dropout sites, the keep mask drawn in its
 * prologue, no stash), then the recurrence and the output projection of tip_forward.  A demoted handle is served by the second form (it
 * has no cooperating encoder).  Configurations the hybrid training forward does not serve: TIP_ERR_UNSUPPORTED_CONFIG.  The keep
 * decisions are a function of (seed, site, element index) alone: both plans, tip_train_forward and tip_draw_keep_mask agree on them.
 * seeds_dev (nullable): DEVICE unsigned long long [2] = {seed, state_seed}, read by the kernels at launch time INSTEAD of the two
 * arguments — so a captured HIP graph holding "tip_seeds_next, tip_forward_live" draws fresh masks at every replay with no kernel
 * argument changing.  p_state / p_drop (the thresholds) stay host arguments.
 * flags, workspace (tip_workspace_bytes), hand-off checks, CU-masked streams and HIP-graph capture as in tip_forward_rows. */
TIP_API int tip_forward_live(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, const int* rows, int flags,
                     const float* keep_mask, float keep_scale, float p_state, unsigned long long state_seed, float p_drop,
                     unsigned long long seed, const unsigned long long* seeds_dev, void* workspace, size_t workspace_bytes,
                     tip_stream_t stream);
/* One tiny launch: each of the two words of seeds_dev (DEVICE, 8-byte aligned) is replaced by its splitmix64 successor,
 *     z = s + 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *     next(s) = z ^ (z >> 31)                                                  (all arithmetic modulo 2^64) */
TIP_API int tip_seeds_next(unsigned long long* seeds_dev, tip_stream_t stream);

/* ---- forward in fp64: the module built under `--double` (train_model.py:62-63,84-85: torch.set_default_dtype(float64), fp64
 *      windows :161-164).  Same function as tip_forward (simple_transformer_with_state.py:60-102) with every operation in IEEE
 *      double on the fp64 matrix cores.  `params` = host array of n_params DEVICE pointers to the fp64 state-dict tensors in
 *      tip_tensor_info() order, RAW (nothing is packed, no tip_attach_packed needed); x_imu / x_s / keep_mask / y as in tip_forward
 *      but double; flags: TIP_FWD_LAST_ROW_ONLY; workspace of tip_forward_f64_bytes(), 256-byte aligned.  Any configuration and
 *      any T >= 1.  A debugging / verification path: layer-by-layer kernels, not tuned. */
TIP_API int tip_forward_f64_bytes(const tip_handle* h, int B, int T, size_t* bytes);
TIP_API int tip_forward_f64(tip_handle* h, const double* const* params, int n_params, const double* x_imu, const double* x_s, double* y,
                    int B, int T, int flags, const double* keep_mask, double keep_scale, void* workspace, size_t workspace_bytes,
                    tip_stream_t stream);

/* ---- measurement ------------------------------------------------------------------------------------------ */
/* number of tip_forward calls that launched HIP kernels since tip_create (lets tests prove the HIP path ran) */
TIP_API int tip_forward_count(const tip_handle* h, uint64_t* n);
/* after the stream is synchronised: per-stage totals accumulated since TIP_OPT_PROFILE was last set.
 * ms[i] = summed duration of stage names[i], launches[i] = event pairs summed.  Arrays of length `cap`;
 * returns the number of stages (<= cap) or a negative status. */
TIP_API int tip_profile_read(tip_handle* h, const char** names, float* ms, int* launches, int cap);
/* (synchronises the device) number of inter-workgroup hand-off waits that gave up since the library was loaded.
 * The cooperating kernels (RNN clusters) never spin forever; if a peer does not arrive within ~1 s they continue
 * and bump this counter: non-zero => the outputs of that launch are invalid.  Must be 0 in a healthy process. */
TIP_API int tip_spin_timeouts(unsigned* count);
/* Hand-off failures are ERRORS, not numbers.  The cooperating plans (pair-split encoder, clustered / GEMV RNN) rely on
 * all their workgroups being resident at once: the launchers refuse a grid the runtime's occupancy query says cannot be
 * (hipErrorCooperativeLaunchTooLarge -> TIP_ERR_HIP), but another process or stream holding CUs can still starve a
 * partner.  A wait that gives up (bounded spin, ~1 s) (a) makes that workgroup produce NaN from there on, which the rest of
 * the forward propagates into the affected output rows — never finite-but-wrong values; (b) sets a sticky word in the
 * handle's pinned host block.  While it is set, tip_forward / tip_train_forward / tip_train_backward return
 * TIP_ERR_HANDOFF at entry, i.e. the call AFTER the failed launch completed reports it.  tip_check(h, 0) returns
 * TIP_ERR_HANDOFF or TIP_OK without synchronising (synchronise the stream first for a definitive answer about launches in
 * flight); tip_check(h, 1) also clears the word.  The GPU must be exclusively this process's for the cooperating plans to
 * run at speed; TIP_PLAN_FUSED / TIP_PLAN_GENERAL with TIP_OPT_RNN_CLUSTER = 1 need no co-residency at all.
 * Inside one process the library helps: tip_forward / tip_forward_f64 / tip_train_forward / tip_train_backward calls issued on
 * DIFFERENT streams of the handle's device (any handle) are serialised on the device (one event wait per stream switch; streams
 * are told apart by handle value, so a destroyed stream whose handle the runtime recycles counts as the same stream; calls on a
 * CAPTURING stream are exempt — see the HIP-graph note below), and a stream created with a CU mask
 * (hipExtStreamCreateWithCUMask) gets plan, grid and cluster sizes for the CUs its mask leaves.
 * After a lost hand-off a host can keep going without co-residency: tip_check(h, 1), tip_set_option(h, TIP_OPT_DEMOTED, 1). */
TIP_API int tip_check(tip_handle* h, int clear);

/* ---- streaming front/back-end: the model-facing half of RTRunnerMin.step
 *      (real_time_runner_minimal.py:59-85 record_raw_imu / record_state_aa_and_c, :87-112 smooth_and_split_s_c,
 *      :131-167 window build + pose assembly) for n_streams lock-stepped streams, entirely on the device.
 *      `state` is a caller-owned device buffer of tip_stream_state_bytes(); frame / call counters are the caller's.
 *      Per frame f = 0,1,2,...:  T = tip_stream_window_len(f);
 *          tip_stream_ingest(state, raw_imu[n,72], n, f, x_imu[n,T,90], x_s[n,T,131], stream);
 *          if (T > 0) { tip_forward(..., TIP_FWD_LAST_ROW_ONLY) -> y_last[n,131];
 *                       tip_stream_consume(state, y_last, n, f - 5, s_rest[n,111] (= s_t[3:114]), c_t[n,20], stream); }
 *      (widths of the paper's model; x_imu [.., 72|90], x_s / y_last [.., 119|131], c_t [.., 8|20] by the buffer's shape: "model shapes" below)
 *      FK and the SBP root-translation correction (:169-194) are not part of the frame: tip_kin_track ("kinematics" below) consumes
 *      s_rest / c_t beside it.  RTRunner's terrain map and IK stay with the host.
 *      HIP graphs: kernel arguments are frozen at capture, so once the window is full (frame_idx >= 43 has been ingested, T = 40
 *      from then on) both calls accept TIP_STREAM_FRAME_AUTO for frame_idx / call_idx — "the frame after the last one ingested",
 *      read from a counter the ingest kernel keeps in `state`.  The triple ingest(AUTO) -> tip_forward -> consume(AUTO) can then be
 *      captured once (hipStreamBeginCapture) and replayed per frame: one graph launch instead of ~23 kernel launches
 *      (tip_amd.StreamingEngine(use_graph=True)).  Entry points called on a capturing stream skip the cross-stream serialisation
 *      and the CU-mask query (see tip_check above): replay such a graph when no other forward is in flight on the device.
 *      (tip_forward itself may be captured the same way for any batch; the clustered recurrence's per-launch XCC-exchange words are
 *      cleared by the kernels at their end for T >= 2, so a replay never reads a previous replay's words; capture T = 1 launches of
 *      more than 64 windows only if they are not replayed.) */
/* ---- model shapes.  The reference's runners serve four models: with or without the acc-sum feature (RTRunner / RTRunnerMin
 *      with_acc_sum) times five or two stationary body points (RTRunner five_sbp; real_time_runner.py:39).  A state buffer has ONE
 *      shape, fixed by its reset and kept until the next one (an attach keeps it); every streaming entry point reads it from the
 *      buffer, so none of them takes it as an argument.  Buffer widths per shape, wherever the comments of this section say 90, 131, 20:
 *          x_imu        [.., 72 | 90]     72 without acc-sum, 90 with
 *          x_s, y_last,
 *          y, y_slot    [.., 119 | 131]   108 + 3 + 4 * n_sbps: 119 with two SBPs, 131 with five
 *          c_t          [..,   8 |  20]   4 * n_sbps
 *          raw_imu [.., 72], s_init [.., 114], s_rest [.., 111]: the same at every shape
 *      tip_stream_state_bytes does not depend on the shape.  tip_stream_reset is tip_stream_reset_shaped with n_sbps = 5,
 *      with_acc_sum = 1 (the paper's model); n_sbps other than 2 or 5 gives TIP_ERR_INVALID_ARG. */
#define TIP_STREAM_FRAME_AUTO (-1)
TIP_API int tip_stream_state_bytes(int n_streams, size_t* bytes);
TIP_API int tip_stream_reset(void* state, const float* s_init /* [n,114] device */, int n_streams, tip_stream_t stream);
TIP_API int tip_stream_reset_shaped(void* state, const float* s_init /* [n,114] device */, int n_streams, int n_sbps, int with_acc_sum,
                            tip_stream_t stream);
/* Host override of the fed-back pose.  RTRunner with multi_sbp_terrain_and_correction feeds back a history row that is NOT the pose
 * it returns: its two-joint IK corrects hip / knee / ankle angles first (real_time_runner.py:334-382, 483-495).  For each j < count
 * the 6D pose columns 0 .. 107 of slot slots[j]'s NEWEST history row (the one its last consume wrote) are replaced by the 6D form
 * (data_utils.py:182-187) of the 18 axis-angle joints q_aa[j] (= s_t[3:57] of the corrected state).  Root-velocity and c_t columns of
 * that row, the pose average, the output filter and every other slot are untouched.  Call it after the consume of the frame it
 * corrects and before the next ingest, on the same stream; it addresses slots, so it serves lock-step, staggered and
 * position-mapped buffers alike, and runs between two replays of a captured frame.  slots / q_aa are DEVICE arrays; a slot outside
 * [0, n_streams) or one that has not consumed a frame yet is skipped. */
TIP_API int tip_stream_history_override(void* state, int n_streams, const int* slots /* [count] */, const float* q_aa /* [count,54] */,
                                int count, tip_stream_t stream);
TIP_API int tip_stream_window_len(int frame_idx); /* 0 while the 11-tap smoother primes (frames 0..4), then 1..40 */
TIP_API int tip_stream_ingest(void* state, const float* raw_imu, int n_streams, int frame_idx, float* x_imu, float* x_s,
                      tip_stream_t stream);
TIP_API int tip_stream_consume(void* state, const float* y_last, int n_streams, int call_idx, float* s_rest, float* c_t,
                       tip_stream_t stream);
/* tip_stream_ingest for a frame whose forward is tip_forward_reuse on FULL windows: the state is advanced exactly as by
 * tip_stream_ingest, but only row T-1 of x_imu / x_s [n,T,*] is written (rows 0 .. T-2 keep whatever they held) — the reuse forward
 * takes every older row from its ring, and at >= 1024 streams gathering the 35-KB windows is most of the ingest's time. */
TIP_API int tip_stream_ingest_newest(void* state, const float* raw_imu, int n_streams, int frame_idx, float* x_imu, float* x_s,
                             tip_stream_t stream);

/* ---- staggered streams: every slot of `state` starts, warms up and stops on its own (a server's connect / disconnect / restart),
 *      without touching the other slots.  Each slot keeps its own frame counter f_i (in `state`; no host frame index anywhere) and a
 *      flag, attached or detached; detached is the flag's zero value, so after tip_stream_reset every slot is detached.  A NEW state
 *      buffer goes through tip_stream_reset once before its first staggered call: freshly allocated memory holds garbage flags.
 *      Windows sit in fixed 40-row slots, x_imu [n,40,90] / x_s [n,40,131] (x_imu [n,40,72|90], x_s / y_last [n,40|-,119|131],
 *      c_t [n,8|20], s_rest [n,111] by the buffer's shape); per frame, on one stream:
 *          tip_stream_ingest_staggered(state, raw_imu[n,72], n, x_imu, x_s, rows[n], stream);
 *              attached slot i: f_i advances, T_i = tip_stream_window_len(f_i); rows 0 .. T_i-1 of its window are what
 *              tip_stream_ingest writes for frame f_i (bit for bit), rows T_i .. 39 are zero, rows[i] = T_i - 1 (-1 while priming);
 *              detached slot: zero window, rows[i] = -1, state untouched
 *          tip_forward_rows(h, x_imu, x_s, y_last[n,131], n, 40, rows, ...);      (NaN rows where rows[i] = -1)
 *          tip_stream_consume_staggered(state, y_last, rows, n, s_rest[n,111], c_t[n,20], stream);
 *              slot i with rows[i] >= 0 consumes y_last[i] as call f_i - 5; the others are skipped (state and output rows untouched)
 *      The three calls take no frame index, so they can be captured once (HIP graph) and replayed from the first frame on;
 *      tip_stream_attach / tip_stream_detach run between replays on the same stream.  slots / s_init are DEVICE arrays; slot indices
 *      outside [0, n) are ignored (the host rejects them, and duplicates, before the call).
 *      tip_stream_attach: the listed slots are reset as tip_stream_reset does (history row 0 from s_init row j for slots[j]) and
 *      marked attached: their next staggered ingest is their frame 0.  tip_stream_detach marks slots detached.
 *      Cost: every slot, warming up, priming or detached, occupies a T = 40 window in the forward — a freshly started staggered
 *      engine pays the steady-state price from its first frame on, where the lock-step entry points run shorter windows (the
 *      position-mapped entry points below run the forward on the attached slots only).  The lock-step entry points ignore the flag. */
TIP_API int tip_stream_attach(void* state, int n_streams, const int* slots, const float* s_init /* [count,114] */, int count,
                      tip_stream_t stream);
TIP_API int tip_stream_detach(void* state, int n_streams, const int* slots, int count, tip_stream_t stream);
TIP_API int tip_stream_ingest_staggered(void* state, const float* raw_imu, int n_streams, float* x_imu, float* x_s, int* rows,
                                tip_stream_t stream);
TIP_API int tip_stream_consume_staggered(void* state, const float* y_last, const int* rows, int n_streams, float* s_rest, float* c_t,
                                 tip_stream_t stream);

/* ---- staggered streams through a position map (compact pools): the forward runs on B <= n windows, not n.  slot_at is a DEVICE
 *      int [B]: window position p (0 <= p < B) carries slot slot_at[p], and -1 (any value outside [0, n)) marks an empty position.
 *      Each slot appears AT MOST ONCE in slot_at: that is the host's duty, it is not checked on the device (a slot listed twice would
 *      advance twice in one frame).  Indexing: raw_imu, state, s_rest, c_t, y_slot and rows_slot are by SLOT ([n, *]); x_imu, x_s,
 *      rows and y are by POSITION ([B, *]); x_imu [B,40,72|90], x_s [B,40,119|131], y / y_slot [.,119|131], c_t [n,8|20],
 *      s_rest [n,111] by the buffer's shape.  Per frame, on one stream:
 *          tip_stream_ingest_mapped(state, raw_imu[n,72], n, slot_at, B, x_imu[B,40,90], x_s[B,40,131], rows[B], stream);
 *              position p with slot s = slot_at[p]: window p and rows[p] are bit for bit what tip_stream_ingest_staggered writes for
 *              slot s (s's state, frame counter and attached flag); an empty position, or a detached slot: zero window, rows[p] = -1.
 *              Slots not listed are not touched (their frame counter does not advance).
 *          tip_forward_rows(h, x_imu, x_s, y[B,131], B, 40, rows, ...);
 *          tip_stream_consume_mapped(state, y, rows, slot_at, B, n, s_rest[n,111], c_t[n,20], y_slot[n,131], rows_slot[n], stream);
 *              tip_stream_consume_staggered's work for slot slot_at[p] on y[p]; y_slot[s] = y[p] (the NaN row included) and
 *              rows_slot[s] = rows[p] when those are given (both nullable); rows of slots not listed are not touched.
 *      One workgroup per position: both calls cost in proportion to B.  Position -> slot is free to change between frames (the ingest
 *      rebuilds every window from the slot's own state), so a host keeps the attached slots at positions 0 .. k-1 and runs the
 *      forward on the smallest cheap B >= k (tip_amd.streaming.StaggeredStreamingEngine(compact=True)).  Bits: tip_forward's plan
 *      under TIP_PLAN_AUTO depends on B, and AUTO splits a batch into whole rounds plus a remainder, so a window's output bits may
 *      change with B or with its position (within the parity bound of the fp64 reference); on a pinned plan whose per-window results
 *      do not depend on the batch (TIP_PLAN_FUSED) they do not.  B > n and null pointers (other than y_slot / rows_slot) give
 *      TIP_ERR_INVALID_ARG. */
TIP_API int tip_stream_ingest_mapped(void* state, const float* raw_imu, int n_streams, const int* slot_at, int B, float* x_imu,
                             float* x_s, int* rows, tip_stream_t stream);
TIP_API int tip_stream_consume_mapped(void* state, const float* y, const int* rows, const int* slot_at, int B, int n_streams,
                              float* s_rest, float* c_t, float* y_slot, int* rows_slot, tip_stream_t stream);

/* ---- any window length: the reference's RTRunnerMin(char, model, max_input_l, ...) / RTRunner take the window length W as an
 *      argument (real_time_runner_minimal.py:24,54,131,139; real_time_runner.py:29,413,421); the entry points above are W = 40.  The
 *      _w family is the same calls with `window` = W in [1, 128] in front of `stream` (anything else: TIP_ERR_INVALID_ARG); the host
 *      cannot read the device buffer, so every call is told.  What W changes, and nothing else:
 *        - the call for frame f has T = tip_stream_window_len_w(f, W) = min(max(f - 4, 0), W) rows: x_imu [n,T,72|90], x_s [n,T,119|131];
 *          the staggered and mapped windows sit in W-row slots ([n|B, W, *], rows T_i .. W-1 zero);
 *        - the local-frame, acc-sum and history rings are W deep; the raw ring (11) and the output filter (6) are not.  A block is
 *          11*72 + W*(72 + 18 + 131) + 6*131 + 54 + 3 floats rounded up to 64 (tip_stream_state_bytes_w; 10496 floats at W = 40);
 *        - the acc-sum feature still spans ACC_SUM_WIN_LEN = 40 rows (:136-141): the newest min(T, 40) rows of the window;
 *        - TIP_STREAM_FRAME_AUTO means full windows (T = W): valid once frame W + 3 has been ingested.
 *      window = 40 IS the call above: same kernels, same layout, same bits (and no layout check).  Every other W runs kernels that take
 *      W as a value, on a layout of its own: the three control words lead the block, and the shape word records W above the two
 *      shape bits (0 there — what tip_stream_reset(_shaped) writes — means 40).  A buffer is used with ONE W from tip_stream_reset_w
 *      to the next reset.  A _w call whose window (other than 40) is not the one the buffer's reset recorded never produces another
 *      layout's numbers and touches no state: tip_stream_ingest_w writes NaN window rows, the staggered and mapped ingest a NaN window
 *      and rows = -1; consume, attach, detach and override skip the block.  (The windows are filled at the buffer's shape; a buffer no
 *      _w reset ever wrote has no known shape, and the NaNs go to windows of the narrowest one, 119 / 72 columns.  block 0's words
 *      are read at the head of the buffer: it must hold at least one block, which every n_streams >= 1 gives.)
 *      tip_stream_ingest_newest, tip_stream_frame_counter_offset and tip_forward_reuse's ring stay at 40 only. */
TIP_API int tip_stream_state_bytes_w(int n_streams, int window, size_t* bytes);
TIP_API int tip_stream_window_len_w(int frame_idx, int window); /* T, or TIP_ERR_INVALID_ARG (< 0) for a window outside [1, 128] */
TIP_API int tip_stream_reset_w(void* state, const float* s_init /* [n,114] device */, int n_streams, int n_sbps, int with_acc_sum,
                       int window, tip_stream_t stream);
TIP_API int tip_stream_ingest_w(void* state, const float* raw_imu, int n_streams, int frame_idx, float* x_imu, float* x_s, int window,
                        tip_stream_t stream);
TIP_API int tip_stream_consume_w(void* state, const float* y_last, int n_streams, int call_idx, float* s_rest, float* c_t, int window,
                         tip_stream_t stream);
TIP_API int tip_stream_attach_w(void* state, int n_streams, const int* slots, const float* s_init /* [count,114] */, int count,
                        int window, tip_stream_t stream);
TIP_API int tip_stream_detach_w(void* state, int n_streams, const int* slots, int count, int window, tip_stream_t stream);
TIP_API int tip_stream_ingest_staggered_w(void* state, const float* raw_imu, int n_streams, float* x_imu, float* x_s, int* rows,
                                  int window, tip_stream_t stream);
TIP_API int tip_stream_consume_staggered_w(void* state, const float* y_last, const int* rows, int n_streams, float* s_rest, float* c_t,
                                   int window, tip_stream_t stream);
TIP_API int tip_stream_ingest_mapped_w(void* state, const float* raw_imu, int n_streams, const int* slot_at, int B, float* x_imu,
                               float* x_s, int* rows, int window, tip_stream_t stream);
TIP_API int tip_stream_consume_mapped_w(void* state, const float* y, const int* rows, const int* slot_at, int B, int n_streams,
                                float* s_rest, float* c_t, float* y_slot, int* rows_slot, int window, tip_stream_t stream);
TIP_API int tip_stream_history_override_w(void* state, int n_streams, const int* slots /* [count] */, const float* q_aa /* [count,54] */,
                                  int count, int window, tip_stream_t stream);

/* ---- device-fed replay: recorded IMU files through a compact pool with no per-frame host traffic (tip_amd.replay.ReplayPool; the
 *      reference replays a file by stepping its runner once per frame: offline_testing_simple.py:109-155).  The corpus — the frames of
 *      every recording back to back, corpus[n_rows,72] fp32 — and the corpus-shaped outputs s_out[n_rows,111], c_out[n_rows,8|20],
 *      y_out[n_rows,119|131] (nullable), valid[n_rows] (bytes) are DEVICE arrays that live for the whole run.  cur / end are DEVICE
 *      long long [n_slots] tables: cur[s] is the corpus row slot s is fed next (< 0: the slot is idle), end[s] the row after the last
 *      one it is fed.  A frame is, on one stream,
 *          tip_replay_feed(corpus, n_rows, cur, n, raw[n,72], stream);
 *              raw[s] = corpus[cur[s]]; an idle slot, or a cursor outside [0, n_rows): zeros (finite padding, as tip_forward_rows' empty windows)
 *          tip_stream_ingest_mapped(state, raw, ...) -> tip_forward_rows / tip_forward_live -> tip_stream_consume_mapped(..., y_slot, rows_slot, ...);
 *          tip_replay_collect(cur, end, n, n_rows, s_rest[n,111], c_t[n,8|20], y_slot[n,119|131], rows_slot[n], size_s, s_out, c_out, y_out, valid, stream);
 *              slot s with c = cur[s] >= 0 writes output row c + 1 — the step on frame t of a recording fills its row t + 1, as the
 *              reference's loop does (offline_testing_simple.py:123-134).  rows_slot[s] >= 0 (the slot produced a row this frame):
 *              s_out / c_out / y_out row c + 1 = s_rest[s] / c_t[s] / y_slot[s], valid = 1.  rows_slot[s] < 0 (the slot's smoother primes:
 *              its first five frames): s_out row c + 1 = s_out row c, c_out row = 0, y_out row = NaN, valid = 0 — the HOST writes
 *              row 0 of every recording (its start state) before the run, so every priming row is the start state, which is what the
 *              runner returns while it primes (real_time_runner_minimal.py:125-128).  Then cur[s] = c + 1, or -1 once c + 1 = end[s].
 *              A cursor with c + 1 >= n_rows writes nothing and goes idle; idle slots are not touched.
 *      Neither call takes a frame index or any argument that changes from frame to frame: the three steps are captured once (HIP
 *      graph) and replayed; the host rewrites cur / end entries between two replays when a slot takes its next recording.  One wave
 *      per slot, one writer per slot and per output row (the host keeps the recordings of different slots disjoint).  corpus, raw,
 *      c_t and c_out must be 16-byte aligned, cur / end 8-byte; size_s is 119 or 131; y_slot may be null only with y_out;
 *      anything else: TIP_ERR_INVALID_ARG. */
TIP_API int tip_replay_feed(const float* corpus, long long n_rows, const long long* cur, int n_slots, float* raw, tip_stream_t stream);
TIP_API int tip_replay_collect(long long* cur, const long long* end, int n_slots, long long n_rows, const float* s_rest, const float* c_t,
                       const float* y_slot, const int* rows_slot, int size_s, float* s_out, float* c_out, float* y_out,
                       unsigned char* valid, tip_stream_t stream);
/* The tracked frame (tip_amd.replay.ReplayPool(terrain=...)): the full runner's tail inside the pool's frame, so that the pose the leg
 * IK corrects reaches the model's history before the next frame, as RTRunner.step feeds it back (real_time_runner.py:483-495).  On one
 * stream, with nothing read by the host:
 *     tip_replay_feed(...); tip_stream_ingest_mapped -> forward -> tip_stream_consume_mapped;                 (as above)
 *     tip_replay_mask(cur, rows_slot, n, mask[n], stream);
 *         mask[s] = rows_slot[s] >= 0 && cur[s] >= 0: slot s produced a row this frame and feeds a recording
 *     tip_terrain_track(skel, blocks, n, ..., slots = null, begin = {0 .. n-1}, end = {1 .. n}, n, n, s_rest, c_t, nc, valid = mask, flags,
 *                       t_root[n,3], t_viz[n,5,3], t_q_hist[n,54], t_fire[n], stream);                 (one block and one row per slot)
 *     tip_stream_history_override[_w](state, n, t_fire, t_q_hist, n, stream);                          (entries < 0 are skipped)
 *     tip_replay_collect_tracked(... tip_replay_collect's arguments up to valid ..., t_root, t_viz, t_q_hist, t_fire, blocks, block_stride,
 *                                root_out[n_rows,3], viz_out[n_rows,5,3], q_hist_out[n_rows,54], fire_out[n_rows] (bytes),
 *                                counters_out[n_rows,2] (int), stream);
 *         for s_out / c_out / y_out / valid and the cursors: tip_replay_collect, bit for bit.  Beside it, for a slot that wrote row c + 1:
 *         rows_slot[s] >= 0: root_out / viz_out / q_hist_out row c + 1 = t_root[s] / t_viz[s] / t_q_hist[s], fire_out = (t_fire[s] >= 0),
 *         counters_out row = {off_map, regions_full} of block s (bytes 1208 and 1212 of blocks + s * block_stride: cumulative since the
 *         block's reset).  rows_slot[s] < 0 (priming): root_out, q_hist_out and counters_out rows c + 1 = their rows c, viz_out = 100,
 *         fire_out = 0 — so every row is what tip_terrain_track gives for it in a post-pass over the recording.  The HOST writes row 0 of
 *         every recording before the run (root s_init[:3], q_hist s_init[3:57], viz 100, fire 0, counters 0) and resets the slot's block
 *         (tip_terrain_reset) whenever the slot takes a recording.
 * block_stride is tip_terrain_state_bytes(n, ...) / n (a multiple of 8, at least 1280); blocks 8-byte aligned.  Null pointers (y_slot /
 * y_out as above), negative counts and size_s outside {119, 131} return TIP_ERR_INVALID_ARG; n_slots = 0 is TIP_OK without a launch. */
TIP_API int tip_replay_mask(const long long* cur, const int* rows_slot, int n_slots, unsigned char* mask, tip_stream_t stream);
TIP_API int tip_replay_collect_tracked(long long* cur, const long long* end, int n_slots, long long n_rows, const float* s_rest,
                               const float* c_t, const float* y_slot, const int* rows_slot, int size_s, float* s_out, float* c_out,
                               float* y_out, unsigned char* valid, const float* t_root, const float* t_viz, const float* t_q_hist,
                               const int* t_fire, const void* t_state, long long block_stride, float* root_out, float* viz_out,
                               float* q_hist_out, unsigned char* fire_out, int* counters_out, tip_stream_t stream);

/* ---- sensor front end: raw IMU packets and the per-slot calibration, in front of the `raw_imu` every ingest above takes — the
 *      arithmetic the reference's live demo does on the host between its socket reader and RTRunner.step (live_demo_new.py:97-112
 *      packet -> readings, :150-158 / :221-226 heading reset, :243-248 / :52-62 T-pose, :161-175 the per-frame transform).
 *      A packet is packets[n,42] fp32, row-major: per sensor q0 q1 q2 q3 ax ay az, the quaternion read as (x, y, z, w) and normalised
 *      — what the demo hands to fairmotion's Q2R, i.e. scipy's Rotation.from_quat(q).as_matrix() — and the acceleration in the
 *      sensor's frame.  `cal` is a caller-owned device buffer of tip_sensor_state_bytes() (8-byte aligned), one block per slot: the
 *      126-float TABLE R_Gn_Gp[6][9] | acc_offset[6][3] | R_B0_S0[6][9] (fp32), fp64 sums [72], a sample count, a phase word, and
 *      the fp64 form of R_Gn_Gp.  Phases: 0 uncalibrated, 1 accumulating heading, 2 heading done, 3 accumulating T-pose, 4 live.
 *      tip_sensor_reset: every block to phase 0 (required once: fresh memory holds garbage phases).
 *      tip_sensor_begin: for each j < count, slot slots[j] starts a hold: sums and count to zero, and with TIP_SENSOR_HEADING phase
 *        0 | 2 | 4 -> 1, with TIP_SENSOR_TPOSE phase 2 -> 3 (also how a T-pose is taken again after a finished heading).  A begin
 *        this rule does not allow leaves the block untouched.
 *      tip_sensor_accumulate: every slot in phase 1 or 3 adds its packet's six Q2R matrices (fp64, from the fp32 quaternion) and six
 *        raw accelerations to its sums and bumps its count; slots in any other phase are not written at all.
 *      tip_sensor_finish: a listed slot in phase 1: R_Gn_Gp = the mean matrices AS THEY ARE (the demo does not re-orthonormalise),
 *        acc_offset = the mean accelerations, phase 2.  In phase 3: R_B0_S0 = R_Gp_B0^T (R_Gn_Gp^T mean) in fp64, rounded once to
 *        fp32, phase 4.  R_Gp_B0: DEVICE double [6][9] (8-byte aligned), or null for the demo's aligned T-pose
 *        [[0,0,1],[1,0,0],[0,1,0]] for all six sensors.  A finish with count 0 writes NaN tables; a listed slot in any other phase
 *        is untouched.
 *      tip_sensor_set / tip_sensor_get: tables[count,126] into / out of the listed slots' blocks.  A set makes the slot live (phase
 *        4): a saved calibration is put back without the two holds.  A get does not look at the phase.
 *      tip_sensor_transform: the per-frame launch.  raw_out[n,72] by slot — a streaming engine's raw_imu — from packets[n,42], fp32:
 *        R_Gp_St = R_Gn_Gp^T Q2R(q), columns 9k .. 9k+8 = R_Gp_St R_B0_S0^T, columns 54+3k .. 54+3k+2 = clip(R_Gp_St acc -
 *        acc_offset, +-max_acc) (the demo's MAX_ACC is 10; max_acc < 0 or NaN: TIP_ERR_INVALID_ARG).  The clip is np.clip's: a NaN
 *        stays a NaN.  A zero or non-finite quaternion (scipy raises there) gives that sensor's nine rotation and three
 *        acceleration columns NaN and touches nothing else; a slot whose phase is not 4 gets a row of 72 NaN, never a finite row
 *        from an unfinished calibration.  One thread per (slot, sensor), no argument that changes from frame to frame.
 *      slots / tables / R_Gp_B0 are DEVICE arrays.  A listed slot outside [0, n_slots) is skipped (a get leaves its output row as it
 *      was); a slot listed twice is written twice with the same values.  Null buffers, a negative n_slots or count:
 *      TIP_ERR_INVALID_ARG; count = 0 or n_slots = 0 launches nothing.  Everything runs on `stream`, in order with the engine's frame:
 *      tip_sensor_transform(cal, packets, n, 10.f, raw, stream); tip_stream_ingest(state, raw, ...); a hold of one slot runs between
 *      the frames of the others (tip_amd.sensors.SensorFrontEnd; the engines' step_packets). */
#define TIP_SENSOR_HEADING 1
#define TIP_SENSOR_TPOSE   2
TIP_API int tip_sensor_state_bytes(int n_slots, size_t* bytes);
TIP_API int tip_sensor_reset(void* cal, int n_slots, tip_stream_t stream);
TIP_API int tip_sensor_begin(void* cal, int n_slots, const int* slots, int count, int which, tip_stream_t stream);
TIP_API int tip_sensor_accumulate(void* cal, const float* packets /* [n,42] */, int n_slots, tip_stream_t stream);
TIP_API int tip_sensor_finish(void* cal, int n_slots, const int* slots, int count, const double* R_Gp_B0 /* [6,9] or null */,
                      tip_stream_t stream);
TIP_API int tip_sensor_set(void* cal, int n_slots, const int* slots, int count, const float* tables /* [count,126] */,
                   tip_stream_t stream);
TIP_API int tip_sensor_get(const void* cal, int n_slots, const int* slots, int count, float* tables_out /* [count,126] */,
                   tip_stream_t stream);
TIP_API int tip_sensor_transform(const void* cal, const float* packets /* [n,42] */, int n_slots, float max_acc,
                         float* raw_out /* [n,72] */, tip_stream_t stream);

/* ---- missing IMU readings: the reference's answer to sensors that deliver nothing for a frame (preprocess_DIP_TC_new.py:112-136
 *      fill_in_nan_values, :160-180 get_real_imu_readings_ours_format_knee), for recorded files, for the live front end above and for
 *      recorded sessions.  A sensor's 9 rotation values and its 3 acceleration values are two independent PARTS of a row; a part is
 *      BAD when the sum of its values is NaN (one NaN element, or Inf - Inf), and a bad part is replaced as a whole.
 *      Rule R ("reference"), on a sequence known in full: the mask comes from the data as it came; walking t upwards, a bad part
 *        at t becomes, per value, (the sum in ascending row order of the values of that column that are not NaN) / (their number)
 *        over rows 0 .. min(10, L)-1 when t <= 10 and over rows t-5 .. t-1 otherwise — of the values as they are by then, earlier
 *        fills included; no such value gives NaN.
 *      Rule V ("live"), for a stream, which cannot look ahead: per part a ring of the last five rows AFTER filling, `have` of them
 *        valid, `run` consecutive fills and `total` fills.  A bad part with have >= 1 (and run < max_gap, when max_gap >= 0) becomes
 *        (the ring's rows summed oldest to newest, fp32) / have, is pushed, and run and total go up.  A bad part with have = 0, or
 *        past max_gap, becomes NaN in all its values and is not pushed.  A good part is pushed and sets run to 0.  max_gap = -1: no
 *        limit, as the reference has none.  V equals R on every row t > 10 when rows 0 .. 10 are good.
 *      tip_fill_real: rule R in fp64 on n_seq ragged sequences of one launch.  ori[n_rows, n_sensors, 9] and acc[n_rows, n_sensors, 3]
 *        (device), sequence r being rows offsets[r] .. offsets[r+1]-1 (device, clamped to [0, n_rows]); sel[6] and rot[9] are HOST
 *        arrays: the six sensors taken, in output order (each in [0, n_sensors)), and the row-major rotation.  out[n_rows, 72]
 *        (device): columns 9k .. 9k+8 = rot * (filled rotation of sensor sel[k]), 54+3k .. 54+3k+2 = rot * (filled acceleration),
 *        every value (r0 h0 + r1 h1) + r2 h2.  unfilled[n_seq] (device int): the parts of the sequence that are still bad.  Rows
 *        that no sequence owns are not written.
 *      tip_fill_rows: rule V on n_seq ragged sequences of frames[n_rows, 72] fp32 into out (which may be frames itself), each
 *        sequence starting from empty rings.  flags[n_rows, 12] bytes, part k < 6 the rotation of sensor k, part 6+k its
 *        acceleration: 0 good, 1 filled, 2 bad and left NaN.
 *      tip_fill_state_bytes / tip_fill_reset: the rings of n slots are a caller-owned device buffer (4-byte aligned).  A reset empties
 *        the rings and zeroes the counters of the listed slots, or of all n when slots is null (required once).
 *      tip_fill_live: rule V for one frame, in place on raw[n, 72] — what tip_sensor_transform has just written — and flags[n, 12].
 *        `cal` is the front end's buffer: a slot whose phase is not 4 is skipped, its NaN row stays, its rings are not touched and its
 *        flags are 0.  No argument changes from frame to frame.
 *      tip_fill_get: counts_out[count, 3, 12] (device int) = have | run | total of the listed slots.
 *      tip_fill_packets: tip_sensor_transform's arithmetic (the same device function, bit for bit) on packets[n_rows, 42] of recorded
 *        sessions, the rows of sequence r with tables[r, 126]; out[n_rows, 72].
 *      Null buffers, negative counts, max_gap < -1, a sel outside the sensors: TIP_ERR_INVALID_ARG; a count of 0 launches nothing. */
TIP_API int tip_fill_real(const double* ori, const double* acc, long long n_rows, int n_sensors, const long long* offsets /* [n_seq+1] */,
                  int n_seq, const int* sel /* host [6] */, const double* rot /* host [9] */, double* out /* [n_rows,72] */,
                  int* unfilled /* [n_seq] */, tip_stream_t stream);
TIP_API int tip_fill_rows(const float* frames /* [n_rows,72] */, float* out, long long n_rows, const long long* offsets /* [n_seq+1] */,
                  int n_seq, int max_gap, unsigned char* flags /* [n_rows,12] */, tip_stream_t stream);
TIP_API int tip_fill_state_bytes(int n_slots, size_t* bytes);
TIP_API int tip_fill_reset(void* state, int n_slots, const int* slots /* or null: all */, int count, tip_stream_t stream);
TIP_API int tip_fill_live(void* state, const void* cal, float* raw /* [n,72] */, int n_slots, int max_gap,
                  unsigned char* flags /* [n,12] */, tip_stream_t stream);
TIP_API int tip_fill_get(const void* state, int n_slots, const int* slots, int count, int* counts_out /* [count,3,12] */,
                 tip_stream_t stream);
TIP_API int tip_fill_packets(const float* tables /* [n_seq,126] */, const float* packets /* [n_rows,42] */, long long n_rows,
                     const long long* offsets /* [n_seq+1] */, int n_seq, float max_acc, float* out /* [n_rows,72] */,
                     tip_stream_t stream);

/* ---- timestamped packets: every wearer resampled to the pool's tick grid, in front of the sensor front end above, whose packets[n,42]
 *      must be one packet per slot per 60 Hz frame.  The reference serves its one wearer with a zero-order hold: the reader thread
 *      overwrites current_reading whenever a packet arrives (live_demo_new.py:82-115) and the loop takes what is there once per
 *      clock.tick(FREQ) (:161-162, :281-307).  Here a slot keeps its last packets with their stamps, and one launch per tick gives every
 *      slot its packet AT the tick — sensors at 100 or 120 Hz, a 50 Hz wearer beside a 60 Hz one, bursts, recorded sessions off the grid.
 *      Stamps and query times are fp64 seconds everywhere (an epoch-sized stamp, 1.7e9 s, still resolves 2.4e-7 s; fp32 resolves 128 s).
 *      `state` is a caller-owned device buffer of tip_resample_state_bytes() (8-byte aligned), one block of bytes / n_slots per slot: the
 *      ring index of the oldest entry, `have` (entries in the ring, 0 .. depth), `total` (packets taken) and `dropped` (packets refused),
 *      4-byte ints; depth fp64 stamps; depth packets [42] fp32.  depth is 2 .. 64 and is given to every call as the state was sized.
 *      tip_resample_reset: the blocks of the listed slots, or of all n when slots is null (required once), to zero: an empty ring.
 *      tip_resample_push: m arrivals, packets[m,42], slots[m], times[m] (device arrays).  The arrivals of one slot are taken in array
 *        order.  A slot outside [0, n) is skipped.  A stamp that is not finite, or (have > 0) not above the slot's newest stamp — a
 *        duplicate, an out-of-order packet — is refused: dropped += 1, nothing else changes.  Otherwise the packet is appended as it is,
 *        NaNs included, a full ring losing its oldest entry, and total += 1.  One wave per slot, and EVERY slot's wave reads the whole
 *        slot list: a push costs n_slots x m reads of slots[] (measured at m = 2 n_slots, the per-tick case: 3.3 us at 256 slots, 7.0 us
 *        at 1024).  A burst or a catch-up with m far above n_slots at a large n grows with the product: push it in pieces per tick,
 *        or use tip_resample_rows, which searches.
 *      tip_resample_emit: the per-tick launch.  t[n] is a DEVICE array (a captured frame freezes its arguments).  Per slot, with
 *        tau = t[slot] - delay (fp64) and the ring's stamps s_0 < ... < s_last, packets_out[slot] and flags[slot] are
 *          ring empty                                                              NaN                      3
 *          not (tau >= s_0)  (before the ring, or tau NaN)                         NaN                      4
 *          tau >= s_last and (max_hold < 0 or tau - s_last <= max_hold)            the newest packet        1
 *          tau >= s_last otherwise                                                 NaN                      2
 *          s_i <= tau < s_(i+1), HOLD: max_hold < 0 or tau - s_i <= max_hold       packet i                 1
 *                                      otherwise                                   NaN                      2
 *          s_i <= tau < s_(i+1), SLERP, max_hold >= 0 and s_(i+1) - s_i > max_hold as the two HOLD rows (nothing is interpolated across a dropout)
 *          s_i <= tau < s_(i+1), SLERP otherwise                                   interpolated at u = (tau - s_i) / (s_(i+1) - s_i), fp64    0
 *        A packet that is given is copied bit for bit.  HOLD with delay 0 is the reference's rule; SLERP needs delay > 0 to have a
 *        later packet at all (delay = one sensor period keeps tau inside the ring).  Every decision is an fp64 comparison of the
 *        expressions above.  One thread per (slot, sensor); tip_resample_tile answers the slots (or rows) of a workgroup.
 *      Interpolation of sensor k between a = q0 q1 q2 q3 ax ay az of packet i and b of packet i + 1, fp32 unless said, every sum left to
 *        right, nothing contracted:
 *          Ra = Q2R(a[0:4]), Rb = Q2R(b[0:4]): the sensor front end's (normalise, then scipy's polynomials).  A zero or non-finite
 *            quaternion on either side gives the sensor's seven output columns NaN and touches nothing else.
 *          qa = a[0:4] / sqrt(a0 a0 + a1 a1 + a2 a2 + a3 a3), qb likewise; dot = qa0 qb0 + qa1 qb1 + qa2 qb2 + qa3 qb3;
 *            dot < 0: qb = -qb, dot = -dot (the shorter arc).
 *          fp64: d = min(dot, 1); d > 1 - 1e-6: w0 = 1 - u, w1 = u; else th = acos(d), w0 = sin((1 - u) th) / sin(th),
 *            w1 = sin(u th) / sin(th); each rounded once to fp32.
 *          q = w0 qa + w1 qb per component, then q / sqrt(q0 q0 + q1 q1 + q2 q2 + q3 q3): unit, its sign the earlier packet's
 *            (a q of length zero or not finite: seven NaN).
 *          The acceleration is a lerp in the GLOBAL frame, where gravity is constant, not of sensor-frame numbers: uf = (float) u,
 *            vf = 1 - uf; ga_r = Ra[r,0] a4 + Ra[r,1] a5 + Ra[r,2] a6, gb_r from Rb and b; g_r = vf ga_r + uf gb_r; with Rq = Q2R(q),
 *            out[4 + c] = Rq[0,c] g_0 + Rq[1,c] g_1 + Rq[2,c] g_2.  A NaN acceleration component makes the sensor's three acceleration
 *            columns NaN and leaves its quaternion.
 *      tip_resample_get: counts_out[count, 3] (device int) = have | dropped | total of the listed slots; a slot outside [0, n) leaves
 *        its row as it was.  It runs on `stream` like every other *_get entry of this header.
 *      tip_resample_rows: the same for n_seq ragged recorded sequences in one launch.  Sequence j is rows in_offsets[j] ..
 *        in_offsets[j + 1] - 1 of packets[n_in, 42] and stamps[n_in] (strictly increasing within a sequence: the host checks), and
 *        its output rows out_offsets[j] .. out_offsets[j + 1] - 1 of packets_out[n_out, 42] and flags[n_out], taken at t_out[n_out]
 *        (all device arrays).  An output row sees what a live ring would hold at its tick — the packets of its sequence with a stamp
 *        <= t_out[row], of these the last `depth` — and then the rule of tip_resample_emit, bit for bit.  The sequence of a row and
 *        the packets before its tick are found by searches, not scans.  A row no sequence owns is NaN with flag 3; input offsets are
 *        clamped to [0, n_in] and to ascending order before they index anything.  out_offsets is trusted to ascend from 0 to n_out: it
 *        is only compared with the row's number and never used as an index, so a wrong one misplaces rows and reads nothing outside.
 *      Null buffers, misaligned state, negative counts, a depth outside 2 .. 64, a delay that is negative or not finite, a NaN max_hold
 *      and an unknown mode return TIP_ERR_INVALID_ARG before any launch; n_slots = 0, m = 0, count = 0, n_out = 0 launch nothing. */
#define TIP_RESAMPLE_HOLD  0
#define TIP_RESAMPLE_SLERP 1
TIP_API int tip_resample_tile(int* rows);
TIP_API int tip_resample_state_bytes(int n_slots, int depth, size_t* bytes);
TIP_API int tip_resample_reset(void* state, int n_slots, int depth, const int* slots /* or null: all */, int count, tip_stream_t stream);
TIP_API int tip_resample_push(void* state, int n_slots, int depth, const float* packets /* [m,42] */, const int* slots /* [m] */,
                      const double* times /* [m] */, int m, tip_stream_t stream);
TIP_API int tip_resample_emit(void* state, int n_slots, int depth, const double* t /* device [n] */, double delay, double max_hold,
                      int mode, float* packets_out /* [n,42] */, unsigned char* flags /* [n] */, tip_stream_t stream);
TIP_API int tip_resample_get(const void* state, int n_slots, int depth, const int* slots, int count, int* counts_out /* [count,3] */,
                     tip_stream_t stream);
TIP_API int tip_resample_rows(const float* packets /* [n_in,42] */, const double* stamps /* [n_in] */,
                      const long long* in_offsets /* [n_seq+1] */, long long n_in, const double* t_out /* [n_out] */,
                      const long long* out_offsets /* [n_seq+1] */, long long n_out, int n_seq, double delay, double max_hold, int mode,
                      int depth, float* packets_out /* [n_out,42] */, unsigned char* flags /* [n_out] */, tip_stream_t stream);

/* ---- clock sync and predicted ticks: in front of the resampler above, for hubs that stamp packets with a clock of their own (it starts
 *      at power-on and drifts by tens of ppm) while the server knows only arrival times, which carry the network's jitter; and a third
 *      emit rule that gives a packet AT the tick with delay 0, so that neither a sensor period of delay (SLERP) nor a packet of
 *      varying age (HOLD with delay 0) has to be chosen.  The reference keeps no stamps (live_demo_new.py:82-115).  Every time and every
 *      decision is fp64, the library is built with -ffp-contract=off, and the statements below give the same bits in numpy.
 *      CLOCK.  `state` is a caller-owned device buffer of tip_clock_state_bytes() (8-byte aligned), 32 bytes per slot, separate from the
 *      resampler's: double theta; double s_prev; int count; int rejected; 8 bytes reserved.  A reset block is all zero bits.
 *      The model: arrival a = s + theta + d, s the sensor's stamp, d >= 0 the network's delay, theta an offset that drifts by at most
 *      `leak` seconds per second.  The estimate is a lower envelope of a - s that may rise only as fast as a clock can drift and fall
 *      only as fast as keeps mapped times strictly increasing.  One slot, its arrivals (s, a) in array order, leak >= 0, 0 <= slew < 1:
 *          if s or a is not finite, or (count > 0 and s <= s_prev):   rejected += 1; mapped = NaN
 *          else:
 *              o = a - s
 *              if count == 0:   theta = o
 *              else:
 *                  d  = s - s_prev
 *                  up = theta + leak * d
 *                  dn = theta - slew * d
 *                  th = o if o < up else up
 *                  theta = th if th > dn else dn
 *              s_prev = s; count += 1; mapped = s + theta
 *      (TIP_CLOCK_LEAK, 200 ppm, is above any crystal; with TIP_CLOCK_SLEW 0.5 two mapped times are at least half as far apart as
 *      their stamps.)  A NaN mapped time is what tip_resample_push drops and counts.
 *      tip_clock_reset: the blocks of the listed slots, or of all n when slots is null (required once), to zero.
 *      tip_clock_get: theta_out[count] (device fp64) and counts_out[count, 2] (device int) = count | rejected of the listed slots; a
 *        slot outside [0, n) leaves its entries as they were.
 *      tip_clock_map: m arrivals, slots[m], stamps[m], arrivals[m] -> times_out[m] (device arrays).  One wave per slot scans the list 64
 *        entries at a time, as tip_resample_push does (and at the same n_slots x m reads of slots[]); times_out[j] of an arrival whose
 *        slot is outside [0, n) is not written.
 *      tip_clock_push: tip_clock_map and tip_resample_push in ONE launch: the same scan maps the stamp and inserts the packet at the
 *        mapped time.  Ring, counters and clock blocks are bit for bit what the two launches leave.  times_out may be null.
 *      tip_clock_rows: n_seq ragged recorded sequences in one launch, sequence j rows offsets[j] .. offsets[j + 1] - 1 of stamps[n_in]
 *        and arrivals[n_in] (offsets clamped to [0, n_in] and to ascending order), each from a reset block: bit for bit what the live
 *        rule gives when fed the sequence in any chunking.  The rule is a sequential scan: one wave per sequence loads 64 pairs at a
 *        time and steps them out of registers, so a launch takes as many dependent steps as its longest sequence has rows.
 *      PREDICTED TICKS.  tip_resample_emit and tip_resample_rows keep their two modes; prediction has entries of its own, with
 *      tip_resample_emit's and tip_resample_rows' arguments, max_predict (seconds, finite, >= 0) in the place of mode.  With
 *      tau = t - delay, the ring's stamps s_0 < ... < s_last and s_prev the one before s_last:
 *          fewer than 2 packets, or not (tau > s_last)                             the SLERP rule above: rows, flags and bits unchanged
 *          tau > s_last: h = tau - s_last, b = s_last - s_prev;
 *            h <= max_predict and h <= TIP_PREDICT_SPAN * b and (max_hold < 0 or b <= max_hold)
 *                                                                                  predicted at u = (tau - s_prev) / b > 1, fp64    5
 *            otherwise                                                             the SLERP rule above (the newest packet held, or stale)
 *        max_predict = 0 predicts no row: every row is then bit for bit SLERP's.
 *      A predicted sensor, a the packet at s_prev and b the one at s_last: the quaternion statements of the interpolation above with this
 *        u — the shorter arc, w0 = sin((1 - u) th) / sin(th) (negative), w1 = sin(u th) / sin(th), q = w0 qa + w1 qb normalised —
 *        which is the geodesic through the two packets continued past the newer one: a constant angular rate.  One statement
 *        differs: above d = 1 - 1e-6, where acos cannot tell arcs apart, th = 2 asin(|qb - qa| / 2) (fp64, the chord's four squares
 *        summed left to right) and the same two sines, not the linear weights, whose error of u (u^2 - 1) th^3 / 6 is a rate error
 *        once u is past 1; the weights are 1 - u and u only below th = 1e-5.  The result is unit, and its sign is the earlier packet's while u th < pi / 2 (q . qa = cos(u th)).
 *        The acceleration is HELD in the global frame, never extrapolated (that would amplify the sensor's noise): gb_r = Rb[r,0] b4 +
 *        Rb[r,1] b5 + Rb[r,2] b6, out[4 + c] = Rq[0,c] gb_0 + Rq[1,c] gb_1 + Rq[2,c] gb_2.  Only the newer packet's acceleration is
 *        read: a NaN in the older one's does not reach the row.  A zero or non-finite quaternion in either packet, or a q without a
 *        rotation, gives the sensor's seven columns NaN; a NaN in the newer packet's acceleration gives its three columns NaN.
 *      Null buffers, misaligned state, negative counts, a depth outside 2 .. 64, a leak, delay or max_predict that is negative or not
 *      finite, a slew outside [0, 1), a NaN max_hold return TIP_ERR_INVALID_ARG before any launch; n_slots = 0, m = 0, count = 0,
 *      n_in = 0, n_out = 0 launch nothing. */
#define TIP_CLOCK_LEAK    2e-4
#define TIP_CLOCK_SLEW    0.5
#define TIP_PREDICT_SPAN  2.0
#define TIP_RESAMPLE_PREDICTED 5
TIP_API int tip_clock_state_bytes(int n_slots, size_t* bytes);
TIP_API int tip_clock_reset(void* state, int n_slots, const int* slots /* or null: all */, int count, tip_stream_t stream);
TIP_API int tip_clock_get(const void* state, int n_slots, const int* slots, int count, double* theta_out /* [count] */,
                  int* counts_out /* [count,2] */, tip_stream_t stream);
TIP_API int tip_clock_map(void* state, int n_slots, const int* slots /* [m] */, const double* stamps /* [m] */,
                  const double* arrivals /* [m] */, int m, double leak, double slew, double* times_out /* [m] */, tip_stream_t stream);
TIP_API int tip_clock_push(void* resample_state, void* clock_state, int n_slots, int depth, const float* packets /* [m,42] */,
                   const int* slots /* [m] */, const double* stamps /* [m] */, const double* arrivals /* [m] */, int m, double leak,
                   double slew, double* times_out /* [m] or null */, tip_stream_t stream);
TIP_API int tip_clock_rows(const double* stamps /* [n_in] */, const double* arrivals /* [n_in] */, const long long* offsets /* [n_seq+1] */,
                   long long n_in, int n_seq, double leak, double slew, double* times_out /* [n_in] */, tip_stream_t stream);
TIP_API int tip_predict_emit(void* state, int n_slots, int depth, const double* t /* device [n] */, double delay, double max_hold,
                     double max_predict, float* packets_out /* [n,42] */, unsigned char* flags /* [n] */, tip_stream_t stream);
TIP_API int tip_predict_rows(const float* packets /* [n_in,42] */, const double* stamps /* [n_in] */,
                     const long long* in_offsets /* [n_seq+1] */, long long n_in, const double* t_out /* [n_out] */,
                     const long long* out_offsets /* [n_seq+1] */, long long n_out, int n_seq, double delay, double max_hold,
                     double max_predict, int depth, float* packets_out /* [n_out,42] */, unsigned char* flags /* [n_out] */,
                     tip_stream_t stream);

/* ---- kinematics: forward kinematics of the character, the root track with its SBP correction, and the evaluation script's seven
 *      metrics — what the reference does through PyBullet behind RTRunnerMin.step (real_time_runner_minimal.py:159-194;
 *      data_utils.py:262-306, 397-412, 473-548) and in offline_testing_simple.py --compare_gt (:422-453; data_utils.py:314-391).
 *      None of it feeds back into the model, so none of it is inside a streaming frame: these entries CONSUME s_rest / c_t, as a
 *      post-pass over whole recordings or as one more launch per live frame (tip_amd.kinematics).
 *      `skel` is a caller-owned device buffer of tip_kin_skel_bytes() that the host fills (4-byte words):
 *          int n_links (<= 32); int sbp[5] (body indices of lankle, rankle, lwrist, rwrist, root); int pad[2];
 *          per link i < 32: int parent (body index: 0 the root, j + 1 link j, always below i + 1); int state_col (column of the
 *          57-wide q where the link's axis-angle starts, -1 for a fixed joint); float joint_xyz[3], joint_q[4] (x, y, z, w: the joint
 *          origin in the parent's link frame); float com_xyz[3] (the inertial origin in the link frame).
 *      A pose is 7 floats, xyz + (x, y, z, w); a pose table is [rows, n_links + 1, 7], the root first, then the links in table order.
 *      tip_kin_fk: q[n, ldq >= 57] (root xyz, root axis-angle, joint axis-angles) -> pq_g (COM poses: getLinkState fields 0-1) and,
 *        when not null, pq_jf (link frames: fields 4-5).  Base at q[:3] with A2Q(q[3:6]); child frame = parent frame x joint origin x
 *        A2Q(axis-angle), the identity for a fixed joint.  A2Q is scipy's from_rotvec().as_quat(): exact at angle 0, a series below
 *        1e-3 rad.  fp32, one lane per pose.
 *      `carry` is a caller-owned device buffer of tip_kin_carry_bytes() (8-byte aligned), one block per sequence: the corrected root
 *        (fp64), the corrected pq_g of the last valid frame with positions about that root, and that frame's s_rest[54:57].
 *      tip_kin_track_reset: for each j < count, block slots[j] (null: j) <- root = s_init[j, :3], pq_prev = FK(s_init[j]) (:47-50).
 *      tip_kin_track: one kernel.  Sequence j < count uses block slots[j] (null: j) and rows begin[j] .. end[j] - 1 of s_rest[n_rows,111],
 *        c_t[n_rows,nc] (nc 8 | 20), valid[n_rows] (bytes; null: every row valid), in order, and leaves the block ready for the next
 *        chunk: a whole recording per call is the replay post-pass, one row per call the live frame, and any chunking gives the same
 *        bits.  A row that is not valid: root_out = the carry's root, viz_out = 100, carry unchanged.  A valid row: the runner's
 *        :159-194 — root_pre = root + v DT, FK, the residues of the active feet against pq_prev, nanmean, clip at +-0.5, the
 *        flat-ground z rule with its norm test taken literally, then root, the five locations and the poses shifted by -vel_res DT.
 *        v is the velocity :159 integrates, from BEFORE the pose averaging of :165-166, which s_rest[54:57] has been through:
 *        v = 2 s_rest[54:57] - (the previous valid row's), and s_rest[54:57] itself on a block's first valid row.
 *        FK is fp32 with the root at the origin; the scan and the root accumulator are fp64; the outputs root_out[n_rows,3] and
 *        viz_out[n_rows,5,3] are fp32.  A non-finite row makes its own sequence's root NaN from there on and touches no other.
 *      tip_kin_metrics: out[count,7] fp64 = angle, j_pos, root_2s, root_5s, root_10s, jerk, root_jerk of file j over rows
 *        offsets[j] + start .. offsets[j + 1] - end - 1 of pred_qdq / gt_qdq [.., 114] and of their pose tables pq_pred / pq_gt (tip_kin_fk
 *        of the same rows); i2, i5, i10 are the script's int(t / DT) - 1, clamped here to the rows in range.  A file with fewer than 4
 *        rows in range gets NaN.  One workgroup per file, fp64 sums in a fixed order.
 *      Null pointers and negative counts return TIP_ERR_INVALID_ARG; a zero count returns TIP_OK without a launch. */
TIP_API int tip_kin_skel_bytes(size_t* bytes);
TIP_API int tip_kin_carry_bytes(int n_slots, size_t* bytes);
TIP_API int tip_kin_fk(const void* skel, const float* q /* [n,ldq] */, int ldq, long long n, float* pq_g /* [n,L+1,7] */,
               float* pq_jf /* [n,L+1,7] or null */, tip_stream_t stream);
TIP_API int tip_kin_track_reset(const void* skel, void* carry, int n_slots, const int* slots /* [count] or null */, int count,
                        const float* s_init /* [count,114] */, tip_stream_t stream);
TIP_API int tip_kin_track(const void* skel, void* carry, int n_slots, const int* slots /* [count] or null */, const long long* begin,
                  const long long* end, int count, long long n_rows, const float* s_rest /* [n_rows,111] */,
                  const float* c_t /* [n_rows,nc] */, int nc, const unsigned char* valid /* [n_rows] or null */,
                  float* root_out /* [n_rows,3] */, float* viz_out /* [n_rows,5,3] */, tip_stream_t stream);
TIP_API int tip_kin_metrics(const void* skel, const float* pred_qdq, const float* gt_qdq, const float* pq_pred, const float* pq_gt,
                    const long long* offsets /* [count+1] */, int count, int start, int end, int i2, int i5, int i10,
                    double* out /* [count,7] */, tip_stream_t stream);

/* ---- kinematics, per-wearer body scale: the entries above for wearers of different body sizes.  The reference builds its character
 *      with scale = h / 1.6 (data-gen-and-viz-bullet-new.py:256-257; bullet_agent.py:47,67: PyBullet's globalScaling), and
 *      RTRunnerMin / RTRunner run on the character they are given.  For a wearer of scale s EVERY LINK'S joint_xyz AND com_xyz IS
 *      MULTIPLIED BY s BEFORE IT IS ROTATED, and nothing else is scaled: not the root xyz of q / s_init / the root accumulator (the
 *      wearer's metres already; tip_syn_poses scales the root too because it puts a reference motion on a scaled agent — the trackers
 *      must not), not the r vectors of c_t, not DT, the +-0.5 clip, the 0.2 m pelvis test, the IK thresholds, the map's bound, grid
 *      size or region epsilons.  Each entry takes what its unscaled form takes and, in front of the stream, `scale` (fp32, device):
 *        the FK entry: one entry PER ROW, so that rows of many wearers share a launch without a search;
 *        the reset and track entries: [n_slots], indexed by the BLOCK a sequence uses (slots[j], or j when slots is null), read once
 *        per sequence per launch.  The scale is not kept in the carry: the caller passes the same array to the reset and to every
 *        track, and changes an entry only together with a reset of that block (the carry's pq_prev was computed with it).
 *      A scale that is not finite or not above 0 makes its own rows NaN — pose tables; root_out, viz_out (and q_hist_out; fire_out -1)
 *      of the rows begin[j] .. end[j] - 1 — writes nothing to that block, the map included (a reset leaves its root NaN), touches no
 *      other sequence and still returns TIP_OK.  A null `scale` is TIP_ERR_INVALID_ARG.  The unscaled entries are unchanged, to the
 *      instruction: the scaled kernels are instantiations of their own (SCALED, csrc/tip_kin_fk.h), never a multiply by 1.
 *      (Declared with the name on a line of its own: the one-line declarations above are each family's unscaled surface.) */
TIP_API int
tip_kin_fk_scaled(const void* skel, const float* q /* [n,ldq] */, int ldq, long long n, float* pq_g /* [n,L+1,7] */,
                  float* pq_jf /* [n,L+1,7] or null */, const float* scale /* [n] */, tip_stream_t stream);
TIP_API int
tip_kin_track_reset_scaled(const void* skel, void* carry, int n_slots, const int* slots /* [count] or null */, int count,
                           const float* s_init /* [count,114] */, const float* scale /* [n_slots], by block */, tip_stream_t stream);
TIP_API int
tip_kin_track_scaled(const void* skel, void* carry, int n_slots, const int* slots /* [count] or null */, const long long* begin,
                     const long long* end, int count, long long n_rows, const float* s_rest /* [n_rows,111] */,
                     const float* c_t /* [n_rows,nc] */, int nc, const unsigned char* valid /* [n_rows] or null */,
                     float* root_out /* [n_rows,3] */, float* viz_out /* [n_rows,5,3] */,
                     const float* scale /* [n_slots], by block */, tip_stream_t stream);

/* ---- terrain: the full runner's tail — what RTRunner.step does behind the model (real_time_runner.py:451-496): the tracker above with
 *      the per-stream height-region map (:140-262), the "establishing height" ticks (:264-277), the vertical root correction from the
 *      map, and the two-joint leg IK (:334-382; data_utils.py:556-630) whose pose is fed back into the history.  A CONSUMER beside the
 *      engines, as the tracker is (tip_amd.terrain): it reads s_rest / c_t, and the pose it corrects goes back through
 *      tip_stream_history_override with fire_out as the slot list (entries < 0 are skipped there) — no engine kernel is involved.
 *      `skel` is the kinematics table above.  The leg chains are read from it: ankle = the SBP body, knee and hip its parent and
 *      grandparent, the hip's parent; the pose columns are those links' state columns (on the reference's character: ik_chain_map_bullet
 *      and ik_chain_map_nimble_joint).  A chain that is not three spherical links never fires.
 *      `state` is a caller-owned device buffer of tip_terrain_state_bytes() (8-byte aligned), one block per slot: what a tracker carry
 *        holds; c_locs_prev[5][3], ik_target_deltas of the two ankles (fp64); the ticks of lankle, rankle, root; n_regions; the
 *        counters off_map and regions_full; grid_num and max_regions as reset laid the block out; region_height[max_regions] and
 *        region_weight[max_regions] (fp64); the map [grid_num, grid_num] of 4-byte cells: region index << 16 | the squared integer
 *        distance to the centre of the update that wrote the cell (the reference's confidence is -sqrt of it; -100 is 10000, so
 *        "confidence_old > confidence_new" is d2_old < d2_new, exactly).  Byte offsets within a block: 0 carry (1024: as
 *        tip_kin_carry_bytes(1)), 1024 c_locs_prev, 1144 deltas, 1192 ticks, 1204 n_regions, 1208 off_map, 1212 regions_full, 1216
 *        grid_num, 1220 max_regions, 1280 region_height, 1280 + 8 max_regions region_weight, 1280 + 16 max_regions the map.
 *        grid_num (2 .. 4096) = int(map_bound / grid_size) * 2 and diffuse_region (1 .. 16) = round(0.5 / grid_size) are the
 *        reference's expressions, evaluated by the host; max_regions 1 .. 65535.
 *      tip_terrain_reset: for each j < count, block slots[j] (null: j) <- RTRunner.__init__: the carry as tip_kin_track_reset sets it,
 *        c_locs_prev 100, ticks -1, deltas 0, region 0 of height 0 and weight 10, every cell region 0 at confidence -100.  The only
 *        launch that touches a whole map.
 *      tip_terrain_track: one kernel.  Sequence j < count uses block slots[j] (null: j) and rows begin[j] .. end[j] - 1, in order, and
 *        leaves the block ready for the next chunk: any chunking gives the same bits.  flags bit 0 is
 *        multi_sbp_terrain_and_correction.  Per valid row, in the reference's order: (1) root_pre = root + v DT (v as tip_kin_track
 *        takes it), FK, c_locs and residues of the active SBPs against the previous frame's corrected poses, vel_res = clip(nanmean
 *        of the two feet), vel_res[2] = 0, c_locs -= vel_res DT; (2) the ticks; (3) update_height_map_new on c_locs_prev for lankle,
 *        then rankle, vel_res[2] += -20 d each; (4) with bit 0 and the pelvis more than 0.2 m (xy) from the mid-ankle point, the same
 *        update for root; (5) with bit 0, correct_joint_q_for_history_feedback for lankle, then rankle; (6) root = root_pre - vel_res
 *        DT, poses about the root, c_locs_prev = c_locs.  Outputs per row: root_out, viz_out (c_locs), q_hist_out = s_rest[:54] with the
 *        columns the IK rewrote, fire_out = the SLOT INDEX where the IK rewrote the pose and -1 elsewhere.  A row that is not valid:
 *        (the carry's root, 100s, s_rest[:54], -1), no state changed.
 *        Decisions the reference leaves open.  OFF-MAP: a patch [c - d, c + d)^2 not wholly inside the map (the reference raises):
 *        no map or region write, the update returns 0, the tick goes to -1, off_map counts it.  OVERFLOW: a new region is due and
 *        max_regions are in use: the same, regions_full counts it.  TIES: an exact tie of |height difference| between two regions of a
 *        patch goes to the lower region index.  TWO SBPS: with nc = 8 only the feet exist, and bit 0 is TIP_ERR_INVALID_ARG.
 *        NON-FINITE: a non-finite c_loc is inactive (the reference's norm < 100); an index is formed only from an active location after
 *        a range test in fp64; a non-finite row can spoil its own slot's root from there on, and nothing else.
 *        FK is fp32 with the root at the origin; everything behind it is fp64 on the fp32 poses; outputs are rounded to fp32 once.
 *        One wave per sequence; nothing waits on another workgroup; a block is written only by the wave whose sequence names it.
 *      Null pointers, negative counts and sizes out of range return TIP_ERR_INVALID_ARG; a zero count returns TIP_OK without a launch. */
TIP_API int tip_terrain_state_bytes(int n_slots, int grid_num, int max_regions, size_t* bytes);
TIP_API int tip_terrain_reset(const void* skel, void* state, int n_slots, int grid_num, int max_regions,
                      const int* slots /* [count] or null */, int count, const float* s_init /* [count,114] */, tip_stream_t stream);
TIP_API int tip_terrain_track(const void* skel, void* state, int n_slots, int grid_num, int max_regions, int diffuse_region,
                      double grid_size, const int* slots /* [count] or null */, const long long* begin, const long long* end,
                      int count, long long n_rows, const float* s_rest /* [n_rows,111] */, const float* c_t /* [n_rows,nc] */, int nc,
                      const unsigned char* valid /* [n_rows] or null */, int flags, float* root_out /* [n_rows,3] */,
                      float* viz_out /* [n_rows,5,3] */, float* q_hist_out /* [n_rows,54] */, int* fire_out /* [n_rows] */,
                      tip_stream_t stream);

/* ---- terrain, per-wearer body scale: tip_terrain_reset and tip_terrain_track for wearers of different body sizes, by the rule of
 *      "kinematics, per-wearer body scale" above: the FK of every row — the poses the residues are taken on, the pelvis test's, the link
 *      frames the leg IK solves on — is the wearer's, and nothing else is scaled.  The block's layout and every byte offset are the
 *      unscaled ones: the scale is not stored. */
TIP_API int
tip_terrain_reset_scaled(const void* skel, void* state, int n_slots, int grid_num, int max_regions,
                         const int* slots /* [count] or null */, int count, const float* s_init /* [count,114] */,
                         const float* scale /* [n_slots], by block */, tip_stream_t stream);
TIP_API int
tip_terrain_track_scaled(const void* skel, void* state, int n_slots, int grid_num, int max_regions, int diffuse_region,
                         double grid_size, const int* slots /* [count] or null */, const long long* begin, const long long* end,
                         int count, long long n_rows, const float* s_rest /* [n_rows,111] */, const float* c_t /* [n_rows,nc] */,
                         int nc, const unsigned char* valid /* [n_rows] or null */, int flags, float* root_out /* [n_rows,3] */,
                         float* viz_out /* [n_rows,5,3] */, float* q_hist_out /* [n_rows,54] */, int* fire_out /* [n_rows] */,
                         const float* scale /* [n_slots], by block */, tip_stream_t stream);

/* ---- hand-over: a live wearer's state moved between pools (tip_amd.handover).  Every per-wearer state above is a block of
 *      *_state_bytes(1, ...) bytes at slot * that in its buffer — tip_stream_state_bytes_w, tip_sensor_state_bytes, tip_fill_state_bytes,
 *      tip_resample_state_bytes, tip_clock_state_bytes, tip_kin_carry_bytes, tip_terrain_state_bytes, and tip_pose_state_bytes of the
 *      display-time poses below — so a wearer leaves one pool and
 *      enters another (of another n, on another device through the host, after a restart) as those bytes, and continues bit for bit.
 *      All lists are DEVICE arrays; every call is asynchronous on `stream`; nothing is read by the host.
 *      tip_handover_export: for each j < count, block slots[j] of `state` (n_slots blocks of block_bytes) -> out + j * out_stride.
 *      tip_handover_import: the other way.  An entry outside [0, n_slots) is skipped and its row (export) or block (import) left
 *        untouched — tip_stream_history_override's convention.  A slot listed twice in an import is the caller's error (either row may win).
 *      tip_handover_stream_import: tip_handover_import for stream blocks (40-row and any-length layout, window 1 .. 128 as the _w family).
 *        Words of a block that belong to the BUFFER, not to the wearer — the complete list, over all eight states: the stream block's
 *        shape word (float index 10474 at window 40, word 2 otherwise: model shape, and the window tag in bits 16-30).  It is not copied,
 *        and it is compared first: a block whose stored shape word differs from the destination block's (or, any-length layout, a
 *        destination whose block 0 does not confirm `window`) is skipped, the slot untouched.  refused (nullable, [count] device ints):
 *        entry j <- slots[j] where the block was skipped for that reason, -1 otherwise.  The frame counter and the attached flag travel
 *        with the block.  No other block stores its slot index or anything derived from n: the terrain block's grid_num and max_regions
 *        words are the wearer's map's, and the host refuses a destination that was built with others; per-slot arrays BESIDE the
 *        blocks (the trackers' scale [n], fire [n], whose entries are slot indices) are the host's to carry and rewrite.
 *      Refused with TIP_ERR_INVALID_ARG before any launch: null state / out / in, a null list with count > 0, negative counts,
 *        block_bytes 0 or not a multiple of 4, a stride below block_bytes or not a multiple of 4, a base or list that is not 4-byte
 *        aligned, a window outside [1, 128].  count = 0 returns TIP_OK without a launch.
 *      One workgroup per (entry, 16-KiB chunk); 16-byte loads and stores when block_bytes, the stride and both bases are multiples of
 *        16, 4-byte ones otherwise (chosen per launch); no LDS; nothing waits on another workgroup. */
TIP_API int tip_handover_export(const void* state, int n_slots, size_t block_bytes, const int* slots /* [count] */, int count,
                                void* out, size_t out_stride, tip_stream_t stream);
TIP_API int tip_handover_import(void* state, int n_slots, size_t block_bytes, const int* slots /* [count] */, int count,
                                const void* in, size_t in_stride, tip_stream_t stream);
TIP_API int tip_handover_stream_import(void* state, int n_streams, const int* slots /* [count] */, int count, const void* in,
                                       size_t in_stride, int window, int* refused /* [count] or null */, tip_stream_t stream);

/* ---- session recorder: the rows a live pool's wearers were served, logged on the device and handed to the host a page at a time
 *      (tip_amd.record.SessionRecorder) — the reference's is_recording buffer (live_demo_new.py:276-278, 312-323), for n wearers and
 *      without a host copy per frame.  A consumer BESIDE the frame, as tip_kin_track and tip_terrain_track are: one launch behind the
 *      engine's frame on the same stream, reading the engine's static buffers; no engine, front-end, tracker, replay or hand-over kernel
 *      is involved.  Every call is asynchronous on `stream`, all lists are DEVICE arrays, nothing is read by the host, and NOTHING
 *      WAITS: no kernel here polls a word another workgroup writes.  The calls on one state buffer are ordered by the stream they share.
 *      State: ONE buffer of tip_record_state_bytes(n, P, R, W) bytes, 16-byte aligned (n slots, P pages of R rows of W floats), int32
 *      words unless said otherwise:
 *          byte 0         header, 64 bytes: 0 magic, 1 n, 2 P, 3 R, 4 W, 5 free-ring head, 6 free-ring tail, 7 full-queue head,
 *                         8 full-queue tail (all four counters run on, taken modulo P as indices), 9 the drain's arrival count
 *          64             slot heads, 32 bytes per slot: 0 open flag, 1 session id, 2 rows written, 3 current page (-1: none),
 *                         4 rows in the current page, 5 rows dropped, 6 pages dropped (runs of dropped rows: page requests that were
 *                         refused behind a row that was stored), 7 rows dropped since the last stored row
 *          64 + 32 n      page records, 32 bytes per page: 0 slot, 1 session id, 2 sequence number within the session, 3 rows used,
 *                         4 rows dropped directly in front of this page's first row (> 0: the page FOLLOWS A GAP), 5-7 unused
 *          + 32 P         free ring int32[P] (padded to 16 bytes), then the full queue int32[P] (padded likewise): pages ready for the host
 *          + ...          the pages, P * R * W floats
 *      A page of a session is pushed onto the full queue the moment it fills, so every page of a session but its last is full and a
 *      page's first row is row seq * R of the session's stored rows.
 *      tip_record_reset: header, heads, records and rings for the stated shape; every page free, every slot closed.
 *      tip_record_open: for each j < count, slot slots[j] starts session sessions[j] with every counter at 0.  An entry outside
 *        [0, n_slots) is skipped (the hand-over's convention), an open slot is left as it is; a slot listed twice is the caller's error.
 *      tip_record_close: the listed slots stop: a partly filled page goes onto the full queue with its row count, the slot becomes closed
 *        (its head keeps the session's counters until the next open).  Closing a slot that is not open does nothing; a slot listed
 *        twice in one close is the caller's error (its page may be queued twice).
 *      tip_record_append: THE PER-FRAME LAUNCH.  srcs is a HOST table of n_srcs <= TIP_RECORD_MAX_SOURCES sources, passed to the kernel
 *        by value (the launch reads no table from memory, and the host can choose the copy's vector from it): a slot's row is row `slot`
 *        of every source, one behind the other, and the columns must add up to W (the kernel checks it against the buffer's header and
 *        writes nothing otherwise; likewise for another n_slots).  valid (nullable, device int32[n_slots]): a slot appends only where
 *        valid[slot] >= valid_min — valid_min = 1 for an array of window lengths T (a priming or detached slot has T = 0 and writes
 *        nothing), 0 for the engines' static arrays of T - 1; with valid null every open slot appends.  No argument changes from frame to
 *        frame, so the launch can sit inside a captured frame.  One wave per slot.  An open slot without a page pops one from the free
 *        ring: ONE device-scope atomic add on the ring's head, checked against its tail (and taken back when nothing was free); a page
 *        that fills is stamped and pushed onto the full queue with one atomic add on that queue's tail.  When no page is free the row is
 *        DROPPED AND COUNTED (head words 5-7) and written nowhere; the slot's next stored row starts a new page whose record word 4
 *        holds the rows dropped in front of it.  When FEWER pages are free than slots ask for one in the same frame, exactly as many
 *        slots get one as pages are free (successful claims take distinct ring entries; once a claim has failed none after it in the
 *        launch succeeds; the head ends where it belongs) and every other asking slot counts its row as dropped; only WHICH of them
 *        get one is not defined.  Rows are copied as 16-byte
 *        vectors when every source's columns and stride are multiples of 4 floats and every base is 16-byte aligned, 4 bytes at a
 *        time otherwise (chosen per launch).
 *      tip_record_drain: the first min(pages on the full queue, max_pages) pages of the queue -> staging, those pages back onto the free
 *        ring, the queue advanced.  staging (tip_record_staging_bytes(max_pages, R, W) bytes, 16-byte aligned): 16 int32 words — 0 pages
 *        gathered, 1 pages still queued, 2 pages in use after the drain (with slots or queued), 3 n, 4 P, 5 R, 6 W, 7 max_pages — then
 *        max_pages page records, then max_pages pages of R * W floats; entries from the gathered count on are left as they were.
 *        out_count (nullable, device int): <- word 0.  It runs in stream order behind an append and in front of the next: no pop is
 *        ever concurrent with a push onto the free ring.
 *      Refused with TIP_ERR_INVALID_ARG before any launch: a null or misaligned state / staging / bytes, a null list with count > 0,
 *        negative counts, pages < 1, page_rows < 1, width < 1 (W = 0), a null source table, n_srcs outside [1, 8], a source with a null
 *        or misaligned base, columns < 1 or a stride below its columns, max_pages < 1.  count = 0 and n_slots = 0 launch nothing. */
#define TIP_RECORD_MAX_SOURCES 8
typedef struct tip_record_source {
    const float* data; /* device, [n_slots] rows */
    int cols;          /* floats taken from each row */
    int stride;        /* floats from one row to the next (>= cols) */
} tip_record_source;
TIP_API int tip_record_state_bytes(int n_slots, int pages, int page_rows, int width, size_t* bytes);
TIP_API int tip_record_staging_bytes(int max_pages, int page_rows, int width, size_t* bytes);
TIP_API int tip_record_reset(void* state, int n_slots, int pages, int page_rows, int width, tip_stream_t stream);
TIP_API int tip_record_open(void* state, int n_slots, const int* slots /* [count] */, const int* sessions /* [count] */, int count,
                            tip_stream_t stream);
TIP_API int tip_record_close(void* state, int n_slots, const int* slots /* [count] */, int count, tip_stream_t stream);
TIP_API int tip_record_append(void* state, int n_slots, const tip_record_source* srcs /* HOST, [n_srcs] */, int n_srcs,
                              const int* valid /* [n_slots] or null */, int valid_min, tip_stream_t stream);
TIP_API int tip_record_drain(void* state, void* staging, int max_pages, int* out_count /* or null */, tip_stream_t stream);

/* ---- display-time poses: the pool's OUTPUT at the viewer's time (tip_amd.display.PoseResampler; csrc/tip_display.hip).  The input side
 *      of a pool is free of the 60 Hz grid (timestamped packets, clock sync and predicted ticks, above); its output is not, and it is late
 *      by construction: the pose a frame produces belongs to IMU_n_smooth = 5 frames before the packet that produced it (the centred
 *      11-tap acceleration average, real_time_runner.py:279-296, :391-393), and the reference shows it once per clock.tick(FREQ)
 *      (live_demo_new.py:281-307).  Here a slot keeps a ring of its last poses with their fp64 stamps, and one launch gives every slot
 *      its pose AT a time of the viewer's choosing — a headset at 72, 90 or 120 Hz, a renderer's next vsync, an export at 30 or 100 fps —
 *      held, interpolated, or predicted past the newest entry.  A consumer BESIDE the frame, as tip_kin_track and tip_record_append are:
 *      it reads the tracker's root [n,3] and the engine's s_rest [n,ld] (root axis-angle and 17 joint axis-angles in its first 54
 *      columns) where they lie; no engine, tracker, replay, hand-over or recorder kernel is involved.  Every call is asynchronous on
 *      `stream`, all arrays are DEVICE arrays, nothing waits on another workgroup and there are no atomics.
 *      `state` is a caller-owned device buffer of tip_pose_state_bytes() (8-byte aligned), one block of bytes / n_slots per slot: the
 *      packet ring's 16-byte header (the ring index of the oldest entry, have, total, dropped: 4-byte ints), depth fp64 stamps, depth
 *      rows [57] fp32 (root xyz, then 18 axis-angles: the q of tip_kin_fk), padded to a multiple of 8 bytes.  depth is 2 .. 64.  A row is
 *      stored exactly as pushed and quaternions are not stored: emit converts the two rows it reads, so a row that is given back is a
 *      bit-for-bit copy.  A block stores nothing derived from its slot index or from n: tip_handover_export / _import carry it unchanged.
 *      tip_pose_reset: the blocks of the listed slots, or of all n when slots is null (required once), to zero: an empty ring.
 *      tip_pose_get: counts_out[count, 3] (device int) = have | dropped | total of the listed slots, with tip_resample_get's conventions.
 *      tip_pose_push: for each listed slot (slots[count], or all n when slots is null) whose valid[slot] is set (valid null: every one),
 *        append (t[slot], root[slot, 0:3], s_rest[slot, 0:54]).  A stamp that is not finite, or (have > 0) not above the slot's newest
 *        stamp, is refused: dropped += 1, nothing else changes.  A slot outside [0, n) is skipped; a slot listed twice is the caller's
 *        error.  A full ring loses its oldest entry; total += 1.  Every argument is static, so a captured frame can hold the call.  One
 *        wave per listed slot.
 *      tip_pose_emit: the per-display-frame launch.  t[n] is a DEVICE array.  Per slot, with tau = t[slot] - delay (fp64) and the ring's
 *        stamps s_0 < ... < s_last, the decision in modes TIP_POSE_HOLD and TIP_POSE_SLERP is tip_resample_emit's table (timestamped
 *        packets, above: the kernel calls the same function), and flags[slot] keeps its numbering: 3 empty, 4 early, 1 held, 2 stale,
 *        0 interpolated.  TIP_POSE_PREDICT is SLERP except where have >= 2 and tau > s_last.  There, with b = min(baseline, have - 1),
 *        s_a the stamp b entries back from the newest and h = tau - s_last:
 *          h <= max_predict and (max_hold < 0 or s_last - s_a <= b * max_hold)      predicted at u = (tau - s_a) / (s_last - s_a) > 1, fp64    5
 *          otherwise                                                                the SLERP rule (the newest entry held, or stale)
 *        THERE IS NO SPAN RULE: the packet side's TIP_PREDICT_SPAN (at most two brackets past the newest packet) would refuse exactly
 *        the 5 .. 9 frames this entry exists for; max_predict alone bounds the horizon.  max_predict = 0 predicts no row: every row is
 *        then bit for bit SLERP's.  baseline > 1 takes the rate over a longer chord: less noise, more lag on a curved track.
 *        A held row is copied bit for bit; an empty, early or stale row is 57 NaN.  quat_out (nullable, [n,18,4]): the 18 rotations as
 *        quaternions x y z w — of a held row its conversion below, of an interpolated or predicted row the unit quaternion the
 *        axis-angle came from, its sign the earlier row's; NaN where the row's columns are.
 *      The arithmetic, per (slot, part), 18 rotation parts and the root, a the earlier row and b the later one.  fp32 unless said, every
 *        sum left to right, nothing contracted:
 *          Axis-angle a -> quaternion: t2 = a0 a0 + a1 a1 + a2 a2, t = sqrt(t2); s = 1/2 - t2 / 48 below t = 1e-3, else
 *            s = sin(t / 2) / t (fp64, rounded once); q = (s a0, s a1, s a2, cos(t / 2) (fp64, rounded once)).  t = 0 is the identity.
 *            A non-finite component makes that joint's three output columns (and its four quaternion columns) NaN and touches nothing else.
 *          dot = qa0 qb0 + qa1 qb1 + qa2 qb2 + qa3 qb3; not (|dot| > TIP_POSE_ANTIPODAL): the two rotations are pi apart, there is no
 *            shorter arc, and the joint is NaN (its neighbours are untouched).
 *          Between the rows (flag 0): the quaternion statements of the packet interpolation above — normalise, the shorter arc, fp64
 *            weights rounded once, q normalised; the kernel calls that function with a zero acceleration.  Past the newer row (flag 5):
 *            the predicted sensor's statements of "clock sync and predicted ticks" — the chord's asin above d = 1 - 1e-6, linear weights
 *            only below th = 1e-5 — likewise called.
 *          Quaternion q -> axis-angle: w < 0: q = -q.  v2 = x x + y y + z z, v = sqrt(v2); k = 2 + v2 / 3 below v = 1e-3, else
 *            k = 2 atan2(v, w) / v (fp64, rounded once); out = (k x, k y, k z): the angle is in [0, pi], so an axis-angle above pi comes
 *            back as its equivalent.
 *          Root position: uf = (float) u, vf = 1 - uf, p_c = vf pa_c + uf pb_c.  The same statement covers u in [0, 1) and u > 1: the
 *            root moves on at the finite-difference velocity of the two entries.  A non-finite component in either row makes the three
 *            root columns NaN.
 *        One thread per (slot, part), tip_pose_tile slots per workgroup; part 0 of a slot decides and the others read the decision from LDS.
 *      tip_pose_rows: tip_resample_rows for poses.  Sequence j is rows in_offsets[j] .. in_offsets[j + 1] - 1 of stamps[n_in] (strictly
 *        increasing within a sequence: the host checks), root[n_in,3] and rows[n_in,ld] (its first 54 columns), and its output rows
 *        out_offsets[j] .. out_offsets[j + 1] - 1 of q_out[n_out,57], quat_out (nullable, [n_out,18,4]) and flags[n_out], taken at
 *        t_out[n_out].  An output row sees what a live ring would hold at its time — the entries of its sequence with a stamp <=
 *        t_out[row], of these the last `depth`, found by searches — and then the rule of tip_pose_emit, bit for bit.  A row no sequence
 *        owns is NaN with flag 3; offsets are clamped and trusted as tip_resample_rows states.
 *      Null buffers, misaligned state or times, negative counts, a depth outside 2 .. 64, ld < 54, a baseline outside 1 .. depth - 1, a
 *      delay or max_predict that is negative or not finite, a NaN max_hold and an unknown mode return TIP_ERR_INVALID_ARG before any
 *      launch; n_slots = 0, count = 0 with a list, n_out = 0 launch nothing. */
#define TIP_POSE_HOLD      0
#define TIP_POSE_SLERP     1
#define TIP_POSE_PREDICT   2
#define TIP_POSE_ANTIPODAL 1e-6f
TIP_API int tip_pose_tile(int* slots);
TIP_API int tip_pose_state_bytes(int n_slots, int depth, size_t* bytes);
TIP_API int tip_pose_reset(void* state, int n_slots, int depth, const int* slots /* or null: all */, int count, tip_stream_t stream);
TIP_API int tip_pose_get(const void* state, int n_slots, int depth, const int* slots, int count, int* counts_out /* [count,3] */,
                 tip_stream_t stream);
TIP_API int tip_pose_push(void* state, int n_slots, int depth, const int* slots /* [count] or null: all */, int count,
                  const float* root /* [n,3] */, const float* s_rest /* [n,ld] */, int ld, const unsigned char* valid /* [n] or null */,
                  const double* t /* device [n] */, tip_stream_t stream);
TIP_API int tip_pose_emit(void* state, int n_slots, int depth, const double* t /* device [n] */, double delay, double max_hold,
                  double max_predict, int baseline, int mode, float* q_out /* [n,57] */, float* quat_out /* [n,18,4] or null */,
                  unsigned char* flags /* [n] */, tip_stream_t stream);
TIP_API int tip_pose_rows(const double* stamps /* [n_in] */, const float* root /* [n_in,3] */, const float* rows /* [n_in,ld] */, int ld,
                  const long long* in_offsets /* [n_seq+1] */, long long n_in, const double* t_out /* [n_out] */,
                  const long long* out_offsets /* [n_seq+1] */, long long n_out, int n_seq, double delay, double max_hold,
                  double max_predict, int baseline, int mode, int depth, float* q_out /* [n_out,57] */,
                  float* quat_out /* [n_out,18,4] or null */, unsigned char* flags /* [n_out] */, tip_stream_t stream);

/* ---- synthetic data: IMU readings and stationary-body-point (SBP) labels from pose sequences — the reference's offline generator
 *      (data-gen-and-viz-bullet-new.py:44-218 over data_utils.py:27-100 get_rot_center_sample_based; bullet_agent.py for the scale),
 *      for `count` ragged sequences held back to back: sequence j is rows offsets[j] .. offsets[j + 1] - 1 of every array, offsets
 *      [count + 1] a DEVICE array from 0 up to n.  fp64 end to end; it produces what tip_combine_sequence consumes
 *      (tip_amd.syndata.synthesize).  An offline producer beside the engines: no engine, graph or other kernel is involved.
 *      `skel` is a caller-owned device buffer of tip_syn_skel_bytes(), 8-byte aligned, that the host fills — the fp64 form of the
 *      kinematics table, with the IMU bodies:
 *          int n_links (<= 32); int sbp[5] (body indices of lankle, rankle, lwrist, rwrist, root); int imu[6] (body indices of root,
 *          lwrist, rwrist, lknee, rknee, upperneck; the first three are sbp[4], sbp[2], sbp[3]); int pad[4];
 *          per link i < 32, 88 bytes: int parent; int state_col; double joint_xyz[3], joint_q[4], com_xyz[3] (as in "kinematics").
 *      `grids` is a caller-owned device buffer of tip_syn_grid_bytes(), 8-byte aligned: the candidate points of the three body classes,
 *      0 feet (SBP slots 0-1), 1 wrists (slots 2-3), 2 pelvis (slot 4), each
 *          int n[3] (points per axis, <= 40); int pad; double axis[3][40] (the values of lp_x, lp_y, lp_z, built by the HOST with
 *          the reference's np.arange expressions: the device never regenerates them);
 *      point i of a class is (axis[0][ix], axis[1][iy], axis[2][iz]) with i = (iy n[0] + ix) n[2] + iz, the order of
 *      np.meshgrid(lp_x, lp_y, lp_z) ravelled.  The launches serve 9 x 6 x 33, 5 x 5 x 5 and 31 x 25 x 8 points (1782 / 125 / 6200);
 *      a class with more than 1792 / 128 / 6400 is cut there.
 *      The tracked-pose block `poses` is [n, 8, 7] doubles, xyz + (x, y, z, w) per slot: slots 0-4 the SBP bodies in sbp order, slots
 *      5-7 imu[3], imu[4], imu[5].  A slot whose body is the root (index 0) holds p + Q2R(Q) (0, 0.1, -0.1) with the root's Q — the
 *      root IMU's and the pelvis SBP's point, the offset not scaled — and every other slot the body's COM pose.
 *      tip_syn_poses: q[n, ldq >= 57] fp64 (as tip_kin_fk's) -> poses, FK in fp64 with every joint and COM offset and the root xyz of
 *        sequence j multiplied by scale[j] (a DEVICE array [count]).  One lane per row.
 *      tip_syn_imu: poses -> imu[n,72]: columns 0:54 six row-major Q2R matrices (scipy's as_matrix, the quaternion normalised first) of
 *        slots 4, 2, 3, 5, 6, 7; columns 54:72 (p[t+4] + p[t-4] - 2 p[t]) / (4/60)^2 of the same slots with t clamped to rows 4 .. L - 5 of
 *        the row's OWN sequence (rows 0-3 copy row 4, rows L-4 .. L-1 copy row L-5); NaN for a sequence of fewer than 9 rows.
 *      tip_syn_sbp: poses -> constrs[n,20], five blocks of (flag, r).  `frames` is caller-owned scratch of n x 5 x 15 doubles, 8-byte
 *        aligned: a first launch fills it with R, w, v per (row, slot) — what does not depend on the previous solution — and the chains
 *        read it.  One workgroup per (sequence, slot), frames in order.  Rows 0, 1,
 *        L-2, L-1 are zero.  Row t takes x1, q1 from row t-1 and x2, q2 from row t+1, dt = 2/60: v = (x2 - x1) / dt, w = (2 sub q2* / dt)[:3]
 *        with sub = q2 - q1 if |q2 - q1| < |q2 + q1| else q2 + q1, R = Q2R(q2); the residue of point p is
 *        |w x Rp + v| + 0.2 |Rp - (r_prev - v dt)| + 0.02 |Rp|, the middle term absent when row t-1 had no solution or t = 2.  The
 *        solution is the first point of least residue in the order above; the flag is 1 and r = Rp iff that residue is < 0.15, else the
 *        row is zero and the chain starts over.  A NaN residue never wins a comparison, so a non-finite row gives flag 0.
 *      Null pointers, negative counts and misaligned buffers return TIP_ERR_INVALID_ARG; n = 0 returns TIP_OK without a launch. */
TIP_API int tip_syn_skel_bytes(size_t* bytes);
TIP_API int tip_syn_grid_bytes(size_t* bytes);
TIP_API int tip_syn_poses(const void* skel, const double* q /* [n,ldq] */, int ldq, const long long* offsets /* [count+1] */, int count,
                  const double* scale /* [count] */, long long n, double* poses /* [n,8,7] */, tip_stream_t stream);
TIP_API int tip_syn_imu(const double* poses /* [n,8,7] */, const long long* offsets /* [count+1] */, int count, long long n,
                double* imu /* [n,72] */, tip_stream_t stream);
TIP_API int tip_syn_sbp(const void* grids, const double* poses /* [n,8,7] */, const long long* offsets /* [count+1] */, int count,
                long long n, double* frames /* [n,5,15] scratch */, double* constrs /* [n,20] */, tip_stream_t stream);

/* ---- motion: SMPL pose sequences -> nimble_qdq — the ground-truth half of the reference's preprocessing (data_utils.py:103-161
 *      get_raw_motion_info_nimble_q_dummy_dq over dip_loader.py:101-183, the root augmentation of preprocess_DIP_TC_new.py:98-107 and
 *      fairmotion's Motion.get_pose_by_time), for `count` ragged sequences held back to back, fp64, one launch.  It produces what
 *      tip_syn_poses and tip_combine_sequence consume (tip_amd.motion.qdq_from_smpl).  An offline producer beside the engines.
 *      Source sequence j is rows in_offsets[j] .. in_offsets[j + 1] - 1 of poses[n_in, ldp >= 66] (one axis-angle per SMPL joint, joints
 *      0 .. 21 read) and of trans[n_in, 3], at fps[j] frames per second; its output is rows out_offsets[j] .. out_offsets[j + 1] - 1 of
 *      qdq[n_out, 114].  in_offsets, out_offsets [count + 1], fps [count], has_trans [count] are DEVICE arrays.  A sequence has `trans`
 *      when trans is not null and has_trans is null or has_trans[j] != 0: its root is (A2R(pose[0:3]), trans[frame]); otherwise it is
 *      (rot_up_R A2R(pose[0:3]), (0, 0, 0.95)), rot_up_R = Q2R((.5, .5, .5, .5)) (constants.py:21-23).
 *      times [n_times] (device): t_0 = 0.0075, t_{k+1} = t_k + 1/60 as the HOST's running fp64 sum (np.cumsum: the reference's loop to
 *      the bit; the device never regenerates it).  Output row k of a sequence of n frames is taken at t_k, and exists while
 *      t_k < (n - 1) / fps — the caller sizes out_offsets by that rule.  The pose at a time: time clipped to [0, (n - 1) / fps],
 *      frame1 = int(time fps + 1e-5), frame2 = min(frame1 + 1, n - 1); frame1 == frame2: that frame; else alpha = clip((time -
 *      frame1 / fps) / (frame2 / fps - frame1 / fps), 0, 1), each rotation R1 A2R(alpha R2A(R1^T R2)), the root position linear.
 *      Row k: root p (0:3), root axis-angle (3:6), the 17 spherical joints' axis-angles (6:57; joints[18] (device int): the SMPL joint
 *      of the root, then of output columns 6, 9, ..., 54), v = (p(t_k + 1/60) - p) 60 (57:60), w = R2A(R^T R(t_k + 1/60)) 60 (60:63),
 *      zeros (63:114).  Every column of every row is written.  Axis-angles are rotation-vector logarithms with angle in [0, pi],
 *      taken through a quaternion (Shepperd, atan2).  A NaN or infinite source value makes what reads it NaN; rows that cannot be
 *      addressed (offsets outside the arrays, k >= n_times, fps <= 0, a joint outside 0 .. 21) are NaN, never an access outside.
 *      One lane per (row, slot): root, 17 joints, root at t + 1/60; tip_motion_tile answers the rows and slots of a workgroup.
 *      Negative counts, ldp < 66, misaligned buffers and null pointers with non-zero counts return TIP_ERR_INVALID_ARG before any
 *      launch; count = 0 or n_out = 0 returns TIP_OK without one. */
TIP_API int tip_motion_tile(int* rows, int* slots);
TIP_API int tip_motion_qdq(const double* poses /* [n_in,ldp] */, int ldp, const double* trans /* [n_in,3] or null */,
                   const int* has_trans /* [count] or null */, const long long* in_offsets /* [count+1] */,
                   const long long* out_offsets /* [count+1] */, const double* fps /* [count] */, int count, long long n_in,
                   long long n_out, const double* times /* [n_times] */, long long n_times, const int* joints /* [18] */,
                   double* qdq /* [n_out,114] */, tip_stream_t stream);

/* ---- exact streaming reuse: tip_forward for lock-stepped streams whose windows slide by one frame per call.
 *      In the runner a frame's model inputs never change once recorded (real_time_runner_minimal.py:74,85,137: raw_imu_buffer,
 *      s_and_c_in_buffer and imu_acc_sum_buffer are append-only), so with the stochastic parts off — past_state_dropout = 0, in_dropout = 0,
 *      module in .eval() — the frame's in_linear row (:79) and its layer-0 Q / K / V rows are the same numbers in each of the 40 windows
 *      it appears in (6.8 % of a window's FLOPs).  tip_forward_reuse keeps them per stream in `cache`, a caller-owned device ring of
 *      tip_reuse_cache_bytes() (256-byte aligned; 40 slots x 4 KiB per stream), and computes per call only the NEWEST row's:
 *        call k = 0, 1, 2, ... with frame_idx = f0 + k (consecutive; any f0 >= 0) and windows x_imu / x_s [B,T,*] whose rows 0 .. T-2
 *        are rows 1 .. T-1 of the previous call's windows (T growing 1 .. 40 while the history fills, then T = 40 and sliding);
 *        T < 40: the ring is written, the forward is tip_forward's; T = 40: layer 0 of the two-window encoder (TIP_PLAN_FUSED2, for any
 *        B) reads the ring instead of running prologue, in_linear and the QKV projection.  The results are BIT-IDENTICAL to
 *        tip_forward under TIP_PLAN_FUSED2 (AUTO's own choice for whole multiples of 2 x #CUs windows, e.g. 1024 streams) on the same
 *        windows: the ring's rows are produced by the same MFMA instruction over the same packed fragments in the same k order.
 *      frame_ctr (nullable): a DEVICE int holding the frame index, read by the kernels instead of frame_idx — what a captured HIP graph
 *        needs (arguments are frozen at capture); with the streaming front end: the counter tip_stream_ingest keeps at byte offset
 *        tip_stream_frame_counter_offset() of `state`.
 *      Every slot is tagged with the frame it was written for: a window whose 40 slots are not frames c-39 .. c (a skipped or repeated
 *      call, a ring that was reset or never primed) yields NaN rows, never another frame's numbers.  tip_reuse_reset clears the tags
 *      (required once before the first call, whenever the streams restart, and after tip_attach_packed of a new weight image: the
 *      ring's rows are functions of the weights — the Python host ties a ring to the image it was filled under and refuses a stale
 *      one).  flags: TIP_FWD_LAST_ROW_ONLY; a keep mask is refused
 *      (TIP_ERR_INVALID_ARG), other configurations than the paper's answer TIP_ERR_UNSUPPORTED_CONFIG.  Reference for what is reused:
 *      simple_transformer_with_state.py:63-79 (row-wise prologue + in_linear), torch functional.py:5785 (_in_projection_packed). */
TIP_API int tip_reuse_cache_bytes(const tip_handle* h, int n_streams, size_t* bytes);
TIP_API int tip_reuse_reset(void* cache, size_t cache_bytes, tip_stream_t stream);
TIP_API int tip_forward_reuse(tip_handle* h, const float* x_imu, const float* x_s, float* y, int B, int T, int flags, void* cache,
                      size_t cache_bytes, int frame_idx, const int* frame_ctr, void* workspace, size_t workspace_bytes,
                      tip_stream_t stream);
TIP_API int tip_stream_frame_counter_offset(size_t* bytes);

/* ---- training step: the model call of train_model.py:171-196 ---------------------
 * Replaces `y_pred = model(x_imu, x_s + noise)` in train mode (train_model.py:175) and the model part of
 * `loss.backward()` (train_model.py:192).  Loss, gradient clipping and the optimiser stay in PyTorch.
 *   params    host array of n_params device pointers: the state-dict tensors in tip_tensor_info() order, RAW (as the
 *             optimiser updates them; nothing is packed by the caller)
 *   keep_mask / keep_scale  as in tip_forward (past-state dropout :77); NULL = keep everything.  Input dropout :73 is
 *             applied by the caller to x_imu (no gradient flows to the inputs)
 *   p_drop, seed  dropout of the four nn.TransformerEncoderLayer sites (attention probabilities, after out_proj, after
 *             ReLU, after linear2; torch default p = 0.1, simple_transformer_with_state.py:26-29).  A mask is never
 *             stored: element idx of site s is kept iff  lowbias32((idx mod 2^32) * 0x9E3779B1 + key(seed, s)) >=
 *             floor(p * 2^32), where key = hi32(splitmix64_mix(seed + 0x9E3779B97F4A7C15 * (s + 1))) (once per site) and
 *             lowbias32(z): z ^= z>>16; z *= 0x7FEB352D; z ^= z>>15; z *= 0x846CA68B; z ^= z>>16 (all mod 2^32);
 *             site s = 4*layer + {0 attention P [B,H,T,T], 1 out_proj [M,D], 2 ffn hidden [M,F], 3 linear2 [M,D]},
 *             idx = row-major element index.
 *             Kept values are scaled by 1/(1-p).  p_drop = 0 switches it off.
 *   saved     activation stash written by the forward and read by the backward (tip_train_bytes: saved_bytes)
 *   scratch   backward workspace (scratch_bytes); grads = one flat buffer, tensors in tip_tensor_info() order.
 * Supported: with or without the RNN (:43-46), rnn_hid_size any multiple of 64 up to 512 (512: register-resident cluster kernels;
 * other widths: the streaming kernel in both directions), tf_in_dim 256/512/1024, head width 16/32/64, T <= 128 — else
 * TIP_ERR_UNSUPPORTED_CONFIG (the Python module then differentiates its torch-op composite instead).  A handle with
 * TIP_OPT_DEMOTED set runs both recurrences on single-workgroup tiles (no inter-workgroup hand-off). */
TIP_API int tip_train_bytes(const tip_handle* h, int B, int T, size_t* saved_bytes, size_t* scratch_bytes);
/* where one stashed activation of encoder layer `layer` lives inside `saved` (float offset, float count): */
#define TIP_SAVED_QKV  0 /* [M,3D] in-projection output (q | k | v)                                   */
#define TIP_SAVED_ATT  1 /* [M,D]  attention output before out_proj                                    */
#define TIP_SAVED_X1   2 /* [M,D]  LayerNorm1 output                                                    */
#define TIP_SAVED_HID  3 /* [M,F]  linear1 output after ReLU and dropout (> 0 exactly where the unit's gate is open) */
#define TIP_SAVED_XOUT 4 /* [M,D]  layer output (LayerNorm2)                                            */
#define TIP_SAVED_HALL 5 /* [M,R]  RNN states h_t (layer argument ignored but must be valid)           */
TIP_API int tip_train_saved_view(const tip_handle* h, int B, int T, int what, int layer, size_t* float_offset, size_t* floats);
TIP_API int tip_train_forward(tip_handle* h, const float* const* params, int n_params, const float* x_imu, const float* x_s,
                      const float* keep_mask, float keep_scale, float p_drop, unsigned long long seed, float* y, void* saved,
                      size_t saved_bytes, int B, int T, tip_stream_t stream);
TIP_API int tip_train_backward(tip_handle* h, const float* const* params, int n_params, const float* dy, const void* saved,
                       size_t saved_bytes, void* scratch, size_t scratch_bytes, float* grads, size_t grads_floats, float p_drop,
                       unsigned long long seed, int B, int T, tip_stream_t stream);

/* Gradients w.r.t. the step's INPUTS, to be called right after tip_train_backward on the same scratch (which still holds the gradient
 * w.r.t. in_linear's output): dx_imu [B,T,input_size_imu(+18)] and / or dx_s [B,T,size_s] (either may be NULL).  x_s, keep_mask and
 * keep_scale as given to tip_train_forward: d x_s carries the keep mask and is zero where x_s was NaN (:65) and in the root-velocity
 * columns (:75). */
TIP_API int tip_train_input_grads(tip_handle* h, const float* const* params, int n_params, const float* x_s, const float* keep_mask,
                          float keep_scale, void* scratch, size_t scratch_bytes, float* dx_imu, float* dx_s, int B, int T,
                          tip_stream_t stream);

/* ---- the same step for a module built under `--double` (train_model.py:84-85): fp64 parameters (raw, state-dict order), windows,
 *      keep mask, cotangent and gradients; same dropout decisions as the fp32 step for the same seed (kept values scaled by the fp32
 *      value of 1 / (1 - p), widened).  Any configuration tip_forward_f64 serves (with or without the RNN, any widths) with T <= 128 and
 *      (4 T d_head + 2 T^2) doubles of LDS <= 160 KB (attention backward: T <= 90 at head width 16) — else TIP_ERR_UNSUPPORTED_CONFIG.
 *      A debugging / verification path like tip_forward_f64: layer by layer, deterministic, not tuned.  saved / scratch: 256-byte
 *      aligned, tip_train_bytes_f64(); grads: one flat fp64 buffer, tensors in tip_tensor_info() order. */
TIP_API int tip_train_bytes_f64(const tip_handle* h, int B, int T, size_t* saved_bytes, size_t* scratch_bytes);
TIP_API int tip_train_forward_f64(tip_handle* h, const double* const* params, int n_params, const double* x_imu, const double* x_s,
                          const double* keep_mask, double keep_scale, float p_drop, unsigned long long seed, double* y, void* saved,
                          size_t saved_bytes, int B, int T, tip_stream_t stream);
TIP_API int tip_train_backward_f64(tip_handle* h, const double* const* params, int n_params, const double* dy, const void* saved,
                           size_t saved_bytes, void* scratch, size_t scratch_bytes, double* grads, size_t grads_doubles, float p_drop,
                           unsigned long long seed, int B, int T, tip_stream_t stream);

/* ---- train-set combiner and window gather -------------------------------------------------
 * tip_combine_sequence replaces the per-file body of store_imu_s_info (preprocess_and_combine_syn_amass.py:73-101):
 *   imu [L_imu,72], s = nimble_qdq [L_s,114], c = constrs [>=min(L),20]: fp64 DEVICE arrays as unpickled; bias [18] = the
 *   constant accelerometer bias the caller drew (:85); nan_root_vel = 1 for augmented-DIP files (:61-62).
 *   Writes float32 rows imu_out [n,72], sum_out [n,18], s_out [n,131] and returns n = min(L_imu, L_s) - 8, or 0 when the
 *   file is too short (min(L) <= 40, :68-70: nothing written), or a negative tip_status.
 * tip_gather_windows replaces TrainSubDataset's window slicing (training_data_loader.py:53-58,72-86): for each sampled
 *   end frame t_idx[i] (device int64, seq_length <= t < n_frames): x_imu[i] = [IMU[t-T:t] | SUM[t-T:t]] ([T,90]; [T,72]
 *   when sum_c is NULL), x_s[i] = S[t-T:t], y[i] = S[t-T+1:t+1]. */
TIP_API int tip_combine_frames(int L_imu, int L_s);
TIP_API int tip_combine_scratch_bytes(int L_imu, int L_s, size_t* bytes);
TIP_API int tip_combine_sequence(const double* imu, const double* s, const double* c, int L_imu, int L_s, const double* bias,
                         int nan_root_vel, float* imu_out, float* sum_out, float* s_out, void* scratch, size_t scratch_bytes,
                         tip_stream_t stream);
TIP_API int tip_gather_windows(const float* imu_c, const float* sum_c, const float* s_c, long long n_frames, const long long* t_idx,
                       int n, int T, float* x_imu, float* x_s, float* y, tip_stream_t stream);

/* ---- training losses and their gradient ---------------------------------------------------
 * Replaces learning_utils.py:13-78 as train_model.py:177-189 combines them: loss = loss_constr_multi + loss_q_only_2axis +
 * loss_jerk.  pred / gt: DEVICE fp32 rows [B*T, W], W = n_pose + n_vel + 4*n_sbp (reference: 108 + 3 + 20), row strides ld_*
 * in floats (so the reference's column slices can be passed as they are); n_vel is 3 or 0.  `terms` selects which of the
 * three functions are evaluated; a column group a term does not use may have width 0 (loss_jerk alone: n_vel = n_sbp = 0,
 * gt may be NULL).  Masking as the reference: rows whose GT root x/y are NaN leave the root-velocity terms, rows with any
 * NaN GT constraint leave the constraint terms; a mean over no rows is NaN.
 *   tip_loss_forward   stats[0..3] = total, loss_q, loss_c, loss_j (0 for a term not selected); the rest of stats
 *                      (TIP_LOSS_STATS floats, device) carries the normalisers the backward needs.
 *   tip_loss_backward  dpred[B*T, W] = gout * d total / d pred (gout: DEVICE scalar, NULL = 1); every column is written.
 * Deterministic: fixed-order fp64 reduction of per-workgroup partial sums.  W <= 256 (else TIP_ERR_UNSUPPORTED_CONFIG). */
#define TIP_LOSS_Q 1 /* loss_q_only_2axis (learning_utils.py:50-78) */
#define TIP_LOSS_C 2 /* loss_constr_multi (learning_utils.py:13-35) */
#define TIP_LOSS_J 4 /* loss_jerk         (learning_utils.py:38-47) */
#define TIP_LOSS_STATS 16
TIP_API int tip_loss_ws_bytes(int B, int T, size_t* bytes);
TIP_API int tip_loss_forward(const float* pred, long long ld_pred, const float* gt, long long ld_gt, int B, int T, int n_pose, int n_vel,
                     int n_sbp, int terms, float* stats, void* ws, size_t ws_bytes, tip_stream_t stream);
TIP_API int tip_loss_backward(const float* pred, long long ld_pred, const float* gt, long long ld_gt, int B, int T, int n_pose, int n_vel,
                      int n_sbp, int terms, const float* stats, const float* gout, float* dpred, long long ld_dpred,
                      tip_stream_t stream);

/* the same two passes for fp64 rows (train_model.py --double): pred / gt / stats / gout / dpred in double, everything else as above */
TIP_API int tip_loss_forward_f64(const double* pred, long long ld_pred, const double* gt, long long ld_gt, int B, int T, int n_pose, int n_vel,
                         int n_sbp, int terms, double* stats, void* ws, size_t ws_bytes, tip_stream_t stream);
TIP_API int tip_loss_backward_f64(const double* pred, long long ld_pred, const double* gt, long long ld_gt, int B, int T, int n_pose, int n_vel,
                          int n_sbp, int terms, const double* stats, const double* gout, double* dpred, long long ld_dpred,
                          tip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TIP_HIP_H */
