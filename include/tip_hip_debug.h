/* tip_hip_debug.h — measurement hooks of libtip_hip.so.  NOT part of the drop-in boundary (include/tip_hip.h is): these read
 * in-kernel time stamps and launch counters that the profiling scripts under tools/ and two launch-path assertions in tests/
 * use.  They are exported so that those scripts can reach them through ctypes; nothing in the product path calls them.
 * Every reader copies `n` 64-bit words from a __device__ trace array (filled only when the matching TIP_*_TRACE environment
 * switch was set at launch) and returns 0, -1 for a bad `n`, -5 for a HIP error.
 *
 * Environment switches of the MEASUREMENT BUILD (csrc: `make measure` -> libtip_hip_measure.so, -DTIP_MEASURE; the default library
 * reads none of them — its kernel selection depends on tip_set_option only).  csrc/tip_measure.h is the table (name, type, default,
 * meaning, one line each) and the library reads it in one place; this list repeats exactly its names:
 *   traces (fill the arrays the readers below copy): TIP_FUSEDH_TRACE, TIP_FUSED2_TRACE, TIP_BWD_TRACE, TIP_RNN_TRACE, TIP_HEAD_TRACE,
 *     TIP_FLOW_TRACE
 *   ablation (wrong results, timing only): TIP_RNN_ABLATE (bits: 1 polls never wait, 2 no MFMAs, 4 no row touches,
 *     16 A fragments of the first two batches only — a quarter of the LDS reads, 32 clamp instead of tanh; 128+ trace stamp selection)
 *   A/B selections: TIP_AUTO_SPLIT=0 (no rounds + remainder split), TIP_AUTO_MERGE=0 (no shared tail), TIP_RNN_ROWS4=0 / TIP_RNN_W4=0|1
 *     (recurrence variants), TIP_HEAD=old (streaming projection kernel), TIP_LAT_FLOW=n (largest batch of the few-stream plan's
 *     one-launch form; 0: launch chain), TIP_DW_GROUP=0 (training step: one launch per weight gradient)
 * A boolean switch is off exactly when its value starts with '0'; TIP_RNN_ABLATE, TIP_RNN_W4 and TIP_LAT_FLOW are read with atoi.
 */
#ifndef TIP_HIP_DEBUG_H
#define TIP_HIP_DEBUG_H

#include "tip_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

TIP_API int tip_debug_read_fh_wg(unsigned long long* out, int n);      /* hybrid encoder: per-workgroup start / end stamps (tools/fh_trace.py), n <= 2048.
                                                                          2048 < n <= 7168: behind those words the one-launch round's table (same switch;
                                                                          tools/round_trace.py) — [4 wg] entry, encoder published, recurrence done, exit in
                                                                          100-MHz ticks, then [4096 + wg] the workgroup's XCC id */
TIP_API int tip_debug_read_fh_trace(unsigned long long* out, int n);   /* hybrid encoder: phase stamps of workgroup 0 */
TIP_API int tip_debug_read_bwd_trace(unsigned long long* out, int n);  /* fused backward kernels: phase stamps (tools/bwd_trace.py) */
TIP_API int tip_debug_pgemm_launches(unsigned long long* out);         /* panel-GEMM launches since load, inference (pgemm_kernel) and
                                                                          training step (pgemm_tg_kernel) alike (tests: the scaled widths take it) */
TIP_API int tip_debug_read_f2s_cross_xcd(unsigned* out);               /* pair-split plan: pairs whose halves sat on different XCDs */
TIP_API int tip_debug_read_f2_trace(unsigned long long* out, int n);   /* two-window encoder phase stamps (tools/f2_trace.py) */
TIP_API int tip_debug_read_flow_trace(unsigned long long* out, int n);  /* few-stream dataflow kernel: (entry, inputs ready, stored, published) stamps per stage (tools/flow_trace.py) */
TIP_API int tip_debug_read_f2s_trace(unsigned long long* out, int n);  /* window-split hand-off stamps */
TIP_API int tip_debug_read_rnn_trace(unsigned long long* out, int n);  /* clustered recurrence hand-off stamps (tools/rnn_trace.py) */
TIP_API int tip_debug_clock_probe(unsigned long long* dev_out, void* stream); /* s_memtime / s_memrealtime pair (bench.py: clock under load) */
TIP_API int tip_debug_read_head_wg(unsigned long long* out, int n);    /* output projection: per-workgroup lifetimes (tools/head_trace.py) */
TIP_API int tip_debug_read_head_trace(unsigned long long* out, int n); /* output projection: tile stamps */
/* The schedule tip_forward would take for B windows of length T on `cus` CUs (<= 0: the handle's own count; a handle made without
 * a GPU reports 256), under the handle's options and a workspace of `workspace_bytes`; reuse_full: as tip_forward_reuse on full
 * windows.  Touches no device.  out (cap >= 9): nparts, shared_tail, rnn_cluster, then first / count / plan of part 0 and part 1
 * (zeros for an absent part), then (cap >= 10) 1 when the batch would run as the one-launch round; plan is resolved (never TIP_PLAN_AUTO).  nparts = 2: whole rounds + remainder, as two launch sequences,
 * or (shared_tail) two encoders with one recurrence and one output projection.  Returns the schedule's status (TIP_OK, or
 * TIP_ERR_UNSUPPORTED_CONFIG for a pinned plan that does not serve the shape), TIP_ERR_INVALID_ARG for bad arguments. */
TIP_API int tip_debug_schedule(const tip_handle* h, int B, int T, int cus, int reuse_full, size_t workspace_bytes, int* out, int cap);

#ifdef __cplusplus
}
#endif
#endif /* TIP_HIP_DEBUG_H */
