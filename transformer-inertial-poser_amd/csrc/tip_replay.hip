// tip_replay.hip — device side of offline replay (tip_amd.replay.ReplayPool): recorded IMU files run through the closed loop of a
// compact staggered pool with no per-frame host traffic.  The reference replays a recording by pretending it streams
// (offline_testing_simple.py:109-155: one RTRunnerMin.step per frame, one file after the other); here the whole corpus — every
// recording's frames, back to back, [n_rows, 72] — and the corpus-shaped outputs stay in HBM for the run, and two small kernels
// stand in front of and behind the engine's frame (ingest_mapped -> forward -> consume_mapped):
//
//   replay_feed_kernel     raw[slot] = corpus[cur[slot]]; an idle slot (cur < 0) gets zeros — finite padding, as the empty windows
//                          of tip_forward_rows
//   replay_collect_kernel  for a slot with a live cursor: output row cur + 1 <- the slot's s_rest / c_t / y_last rows and valid = 1, or,
//                          while the slot primes (rows_slot < 0), the start-state row (a copy of output row cur: row 0 of a
//                          recording is written by the host, and each priming row repeats the one before it); then cur += 1, and -1
//                          once the recording's last fed frame (corpus row end - 1) has been collected
//
// cur / end are per-slot int64 tables in HBM: a captured HIP graph freezes kernel arguments, a table does not, so the frame
// feed -> engine -> collect replays unchanged while every slot walks its own recording.  One wave per slot, four slots per
// workgroup; nothing waits on another workgroup; a slot is written by its own wave only, and a wave writes rows of its own
// recording only.  Corpus and raw rows are 288 B and 16-byte aligned: one float4 per lane, 18 lanes.  c_t rows (80 / 32 B) move as
// float4 too; s_rest (444 B) and y_last (524 / 476 B) rows are only 4-byte aligned and move one float per lane.
#include "tip_kin_track.h"   // TerHead: the tracked collect reads two counters of a terrain slot's block

namespace tip {

constexpr int kReplaySlotsPerBlock = 4;

__global__ __launch_bounds__(256) void replay_feed_kernel(const float* __restrict__ corpus, long long n_rows,
                                                          const long long* __restrict__ cur, int n_slots, float* __restrict__ raw) {
    const int slot = blockIdx.x * kReplaySlotsPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= n_slots || lane >= 18) return;
    const long long c = cur[slot];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c >= 0 && c < n_rows) v = reinterpret_cast<const float4*>(corpus + (size_t)c * 72)[lane];
    reinterpret_cast<float4*>(raw + (size_t)slot * 72)[lane] = v;
}

// One slot's collect, by the slot's own wave: what both collect kernels do for s_out / c_out / y_out / valid and the cursor.  Returns the
// output row it wrote (cur + 1), or -1 when the slot wrote nothing (idle, or a cursor past the corpus); *produced says whether the slot's
// engine row went there (rows_slot >= 0) or the start state did.
__device__ __forceinline__ long long replay_collect_slot(int slot, int lane, long long* __restrict__ cur, const long long* __restrict__ end,
                                                         long long n_rows, const float* __restrict__ s_rest,
                                                         const float* __restrict__ c_t, const float* __restrict__ y_slot,
                                                         const int* __restrict__ rows_slot, int ns, float* __restrict__ s_out,
                                                         float* __restrict__ c_out, float* __restrict__ y_out,
                                                         unsigned char* __restrict__ valid, bool* produced_out) {
    const long long c = cur[slot];
    if (c < 0) return -1;                                   // idle
    const long long o = c + 1, e = end[slot];
    if (o >= n_rows) {                                      // (a table that points past the corpus: never written through)
        if (lane == 0) cur[slot] = -1;
        return -1;
    }
    const int nc = ns - 111;                                // 20 | 8 SBP columns
    const bool produced = rows_slot[slot] >= 0;             // the slot's T - 1 of this frame; < 0 while its smoother primes
    // s_rest: the slot's row, or the row before (the start state)
    const float* s_src = produced ? s_rest + (size_t)slot * 111 : s_out + (size_t)c * 111;
    float* s_dst = s_out + (size_t)o * 111;
    for (int i = lane; i < 111; i += 64) s_dst[i] = s_src[i];
    if (lane < nc / 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (produced) v = reinterpret_cast<const float4*>(c_t + (size_t)slot * nc)[lane];
        reinterpret_cast<float4*>(c_out + (size_t)o * nc)[lane] = v;
    }
    if (y_out) {
        const float* y_src = y_slot + (size_t)slot * ns;
        float* y_dst = y_out + (size_t)o * ns;
        for (int i = lane; i < ns; i += 64) y_dst[i] = produced ? y_src[i] : __builtin_nanf("");
    }
    if (lane == 0) {
        valid[o] = produced ? 1 : 0;
        cur[slot] = (o >= e) ? -1 : o;                      // the frame at corpus row end - 1 was the last one fed
    }
    *produced_out = produced;
    return o;
}

__global__ __launch_bounds__(256) void replay_collect_kernel(long long* __restrict__ cur, const long long* __restrict__ end, int n_slots,
                                                             long long n_rows, const float* __restrict__ s_rest,
                                                             const float* __restrict__ c_t, const float* __restrict__ y_slot,
                                                             const int* __restrict__ rows_slot, int ns, float* __restrict__ s_out,
                                                             float* __restrict__ c_out, float* __restrict__ y_out,
                                                             unsigned char* __restrict__ valid) {
    const int slot = blockIdx.x * kReplaySlotsPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= n_slots) return;
    bool produced;
    replay_collect_slot(slot, lane, cur, end, n_rows, s_rest, c_t, y_slot, rows_slot, ns, s_out, c_out, y_out, valid, &produced);
}

// ---- the tracked frame (ReplayPool(terrain=...)): feed -> engine -> mask -> tip_terrain_track -> tip_stream_history_override -> this ----
//
//   replay_mask_kernel             mask[slot] = the slot produced a row this frame AND feeds a recording: rows_slot >= 0 && cur >= 0 — the
//                                  `valid` the terrain step takes, so that an idle slot's stale row never moves a map
//   replay_collect_tracked_kernel  replay_collect_slot, and beside it output row cur + 1 of root / viz / q_hist / fire / counters: from the
//                                  tracker's per-slot rows and the slot's block (off_map, regions_full at their documented byte offsets)
//                                  when the slot produced a row; while it primes, the row before (root, q_hist, counters), markers at 100,
//                                  fire 0 — what a terrain post-pass gives for a row that is not valid

static_assert(offsetof(TerHead, off_map) == 1208 && offsetof(TerHead, regions_full) == 1212,
              "include/tip_hip.h, \"terrain\": off_map, then regions_full");

__global__ __launch_bounds__(256) void replay_mask_kernel(const long long* __restrict__ cur, const int* __restrict__ rows_slot, int n_slots,
                                                          unsigned char* __restrict__ mask) {
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot < n_slots) mask[slot] = (rows_slot[slot] >= 0 && cur[slot] >= 0) ? 1 : 0;
}

__global__ __launch_bounds__(256) void replay_collect_tracked_kernel(
    long long* __restrict__ cur, const long long* __restrict__ end, int n_slots, long long n_rows, const float* __restrict__ s_rest,
    const float* __restrict__ c_t, const float* __restrict__ y_slot, const int* __restrict__ rows_slot, int ns, float* __restrict__ s_out,
    float* __restrict__ c_out, float* __restrict__ y_out, unsigned char* __restrict__ valid, const float* __restrict__ t_root,
    const float* __restrict__ t_viz, const float* __restrict__ t_q_hist, const int* __restrict__ t_fire,
    const unsigned char* __restrict__ t_state, long long t_stride, float* __restrict__ root_out, float* __restrict__ viz_out,
    float* __restrict__ q_hist_out, unsigned char* __restrict__ fire_out, int* __restrict__ counters_out) {
    const int slot = blockIdx.x * kReplaySlotsPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (slot >= n_slots) return;
    bool produced = false;
    const long long o = replay_collect_slot(slot, lane, cur, end, n_rows, s_rest, c_t, y_slot, rows_slot, ns, s_out, c_out, y_out, valid,
                                            &produced);
    if (o < 0) return;
    const long long c = o - 1;
    if (lane < 54) q_hist_out[(size_t)o * 54 + lane] = produced ? t_q_hist[(size_t)slot * 54 + lane] : q_hist_out[(size_t)c * 54 + lane];
    if (lane < 15) viz_out[(size_t)o * 15 + lane] = produced ? t_viz[(size_t)slot * 15 + lane] : 100.f;
    if (lane < 3) root_out[(size_t)o * 3 + lane] = produced ? t_root[(size_t)slot * 3 + lane] : root_out[(size_t)c * 3 + lane];
    if (lane >= 32 && lane < 34) {
        const int k = lane - 32;
        const int* words = reinterpret_cast<const int*>(t_state + (size_t)slot * (size_t)t_stride + offsetof(TerHead, off_map));
        counters_out[(size_t)o * 2 + k] = produced ? words[k] : counters_out[(size_t)c * 2 + k];
    }
    if (lane == 63) fire_out[o] = (produced && t_fire[slot] >= 0) ? 1 : 0;
}

hipError_t launch_replay_feed(const float* corpus, long long n_rows, const long long* cur, int n_slots, float* raw, hipStream_t s) {
    const int blocks = (n_slots + kReplaySlotsPerBlock - 1) / kReplaySlotsPerBlock;
    hipLaunchKernelGGL(replay_feed_kernel, dim3(blocks), dim3(256), 0, s, corpus, n_rows, cur, n_slots, raw);
    return hipGetLastError();
}

hipError_t launch_replay_collect(long long* cur, const long long* end, int n_slots, long long n_rows, const float* s_rest,
                                 const float* c_t, const float* y_slot, const int* rows_slot, int ns, float* s_out, float* c_out,
                                 float* y_out, unsigned char* valid, hipStream_t s) {
    const int blocks = (n_slots + kReplaySlotsPerBlock - 1) / kReplaySlotsPerBlock;
    hipLaunchKernelGGL(replay_collect_kernel, dim3(blocks), dim3(256), 0, s, cur, end, n_slots, n_rows, s_rest, c_t, y_slot, rows_slot,
                       ns, s_out, c_out, y_out, valid);
    return hipGetLastError();
}

hipError_t launch_replay_mask(const long long* cur, const int* rows_slot, int n_slots, unsigned char* mask, hipStream_t s) {
    hipLaunchKernelGGL(replay_mask_kernel, dim3((n_slots + 255) / 256), dim3(256), 0, s, cur, rows_slot, n_slots, mask);
    return hipGetLastError();
}

}  // namespace tip

using namespace tip;

extern "C" {

static bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

int tip_replay_feed(const float* corpus, long long n_rows, const long long* cur, int n_slots, float* raw, tip_stream_t stream) {
    if (!corpus || !cur || !raw || n_rows < 0 || n_slots < 0 || !aligned16(corpus) || !aligned16(raw) ||
        reinterpret_cast<uintptr_t>(cur) % 8)
        return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    return launch_replay_feed(corpus, n_rows, cur, n_slots, raw, static_cast<hipStream_t>(stream)) == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_replay_collect(long long* cur, const long long* end, int n_slots, long long n_rows, const float* s_rest, const float* c_t,
                       const float* y_slot, const int* rows_slot, int size_s, float* s_out, float* c_out, float* y_out,
                       unsigned char* valid, tip_stream_t stream) {
    if (!cur || !end || !s_rest || !c_t || !rows_slot || !s_out || !c_out || !valid || n_rows < 0 || n_slots < 0 ||
        (size_s != 119 && size_s != 131) || (y_out && !y_slot) || !aligned16(c_t) || !aligned16(c_out) ||
        reinterpret_cast<uintptr_t>(cur) % 8 || reinterpret_cast<uintptr_t>(end) % 8)
        return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    return launch_replay_collect(cur, end, n_slots, n_rows, s_rest, c_t, y_slot, rows_slot, size_s, s_out, c_out, y_out, valid,
                                 static_cast<hipStream_t>(stream)) == hipSuccess
               ? TIP_OK
               : TIP_ERR_HIP;
}

int tip_replay_mask(const long long* cur, const int* rows_slot, int n_slots, unsigned char* mask, tip_stream_t stream) {
    if (!cur || !rows_slot || !mask || n_slots < 0 || reinterpret_cast<uintptr_t>(cur) % 8) return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    return launch_replay_mask(cur, rows_slot, n_slots, mask, static_cast<hipStream_t>(stream)) == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_replay_collect_tracked(long long* cur, const long long* end, int n_slots, long long n_rows, const float* s_rest, const float* c_t,
                               const float* y_slot, const int* rows_slot, int size_s, float* s_out, float* c_out, float* y_out,
                               unsigned char* valid, const float* t_root, const float* t_viz, const float* t_q_hist, const int* t_fire,
                               const void* t_state, long long t_stride, float* root_out, float* viz_out, float* q_hist_out,
                               unsigned char* fire_out, int* counters_out, tip_stream_t stream) {
    if (!cur || !end || !s_rest || !c_t || !rows_slot || !s_out || !c_out || !valid || n_rows < 0 || n_slots < 0 ||
        (size_s != 119 && size_s != 131) || (y_out && !y_slot) || !aligned16(c_t) || !aligned16(c_out) ||
        reinterpret_cast<uintptr_t>(cur) % 8 || reinterpret_cast<uintptr_t>(end) % 8)
        return TIP_ERR_INVALID_ARG;
    if (!t_root || !t_viz || !t_q_hist || !t_fire || !t_state || !root_out || !viz_out || !q_hist_out || !fire_out || !counters_out ||
        t_stride < 1280 || t_stride % 8 || reinterpret_cast<uintptr_t>(t_state) % 8)
        return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    const int blocks = (n_slots + kReplaySlotsPerBlock - 1) / kReplaySlotsPerBlock;
    hipLaunchKernelGGL(replay_collect_tracked_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), cur, end, n_slots,
                       n_rows, s_rest, c_t, y_slot, rows_slot, size_s, s_out, c_out, y_out, valid, t_root, t_viz, t_q_hist, t_fire,
                       static_cast<const unsigned char*>(t_state), t_stride, root_out, viz_out, q_hist_out, fire_out, counters_out);
    return tip_launch_status();
}

}  // extern "C"
