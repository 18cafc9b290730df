// tip_resample.hip — timestamped packets: every wearer resampled to the pool's tick grid on the device, in front of the sensor front
// end (include/tip_hip.h, "timestamped packets").  The reference serves one wearer with a zero-order hold: its reader thread overwrites
// current_reading whenever a packet arrives (live_demo_new.py:82-115) and the loop takes what is there once per clock.tick(FREQ)
// (:161-162, :281-307).  Here a slot keeps a ring of its last `depth` packets with their fp64 stamps, and one launch per tick gives
// every slot its packet AT the tick: held (the reference's rule) or interpolated between the two packets around it.
//
//   resample_push_kernel   one wave per slot: the lanes scan the arrival list 64 entries at a time (ballot), the slot's arrivals are taken
//                          in array order, lanes 0-41 copy an accepted packet into the ring, lane 0 its stamp and the counters
//   resample_emit_kernel   one thread per (slot, sensor): the bracket by a search over the ring's stamps, then resample_sensor
//   resample_rows_kernel   the same for R ragged recorded sequences, one thread per (output row, sensor): the row's sequence by a search
//                          over the output offsets, what a live ring would hold at the row's tick by a search over the sequence's stamps
//                          (the packets not after the tick, of these the last `depth`), then the same decision and the same arithmetic
//   resample_reset_kernel / resample_get_kernel   the blocks of all or of the listed slots to zero; have / dropped / total copied out
//
// Every decision is an fp64 comparison of the expressions the header states; the arithmetic is fp32 except the two slerp weights.  Nothing
// waits on another workgroup, nothing reads the environment; a listed slot outside [0, n) is skipped, ring indices and offsets are
// clamped before they index anything, and a block is written only by the wave whose slot it is.  The ring's layout, the emit rule and
// resample_sensor are in tip_resample.h, which tip_clock.hip (clock sync, predicted ticks) shares.
#include "tip_resample.h"

namespace tip {

// ---- live ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void resample_push_kernel(void* state, int n, int depth, const float* __restrict__ packets,
                                                           const int* __restrict__ slots, const double* __restrict__ times, int m) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot >= n) return;
    const ResampleSlot st = resample_slot(state, slot, depth);
    int head = clamp_int(st.hdr[0], 0, depth - 1), have = clamp_int(st.hdr[1], 0, depth);
    int total = st.hdr[2], dropped = st.hdr[3];
    double newest = have > 0 ? st.stamp[(head + have - 1) % depth] : 0.0;
    bool any = false;
    for (int base = 0; base < m; base += 64) {
        const int j0 = base + lane;
        unsigned long long mask = __ballot(j0 < m && slots[j0] == slot);
        while (mask) {                                           // the slot's arrivals of this group, in array order (wave-uniform)
            const int j = base + __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            any = true;
            const double t = times[j];
            if (!__builtin_isfinite(t) || (have > 0 && t <= newest)) {
                dropped += 1;
                continue;
            }
            int at;
            if (have < depth) {
                at = (head + have) % depth;
                have += 1;
            } else {                                             // a full ring loses its oldest entry
                at = head;
                head = (head + 1) % depth;
            }
            if (lane < sn::PACKET) st.packet[(size_t)at * sn::PACKET + lane] = packets[(size_t)j * sn::PACKET + lane];
            if (lane == 0) st.stamp[at] = t;
            newest = t;
            total += 1;
        }
    }
    if (any && lane == 0) st.hdr[0] = head, st.hdr[1] = have, st.hdr[2] = total, st.hdr[3] = dropped;
}

__global__ __launch_bounds__(rs::THREADS) void resample_emit_kernel(void* state, int n, int depth, const double* __restrict__ t,
                                                                    double delay, double max_hold, int mode, float* __restrict__ out,
                                                                    unsigned char* __restrict__ flags) {
    const int slot = blockIdx.x * rs::TILE + threadIdx.x / sn::SENSORS, k = threadIdx.x % sn::SENSORS;
    if (slot >= n) return;
    const ResampleSlot st = resample_slot(state, slot, depth);
    const int head = clamp_int(st.hdr[0], 0, depth - 1), have = clamp_int(st.hdr[1], 0, depth);
    const double tau = t[slot] - delay;
    int i;
    double u;
    const int f = resample_decide([&](int j) { return st.stamp[(head + j) % depth]; }, have, tau, max_hold, mode, i, u);
    float* o = out + (size_t)slot * sn::PACKET + 7 * k;
    const float* a = st.packet + (size_t)((head + i) % depth) * sn::PACKET + 7 * k;
    if (f == rs::F_INTERP) resample_sensor(a, st.packet + (size_t)((head + i + 1) % depth) * sn::PACKET + 7 * k, u, o);
    else if (f == rs::F_HELD) resample_copy7(a, o);
    else resample_nan7(o);
    if (k == 0) flags[slot] = (unsigned char)f;
}

// blockIdx.x: a list entry (slots given) or a slot (slots null); 64 threads zero the block's words.
__global__ __launch_bounds__(64) void resample_reset_kernel(void* state, int n, int depth, const int* __restrict__ slots) {
    const int slot = slots ? slots[blockIdx.x] : (int)blockIdx.x;
    if (slot < 0 || slot >= n) return;
    const ResampleSlot st = resample_slot(state, slot, depth);
    const size_t words = rs::slot_bytes(depth) / 4;              // the ring too: a reset block has one bit pattern
    for (size_t w = threadIdx.x; w < words; w += 64) reinterpret_cast<unsigned*>(st.hdr)[w] = 0u;
}

__global__ __launch_bounds__(64) void resample_get_kernel(const void* state, int n, int depth, const int* __restrict__ slots, int count,
                                                          int* __restrict__ out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count) return;
    const int slot = slots[j];
    if (slot < 0 || slot >= n) return;
    const ResampleSlot st = resample_slot(const_cast<void*>(state), slot, depth);
    out[3 * (size_t)j] = st.hdr[1], out[3 * (size_t)j + 1] = st.hdr[3], out[3 * (size_t)j + 2] = st.hdr[2];
}

// ---- recorded sequences -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(rs::THREADS) void resample_rows_kernel(const float* __restrict__ packets, const double* __restrict__ stamps,
                                                                    const long long* __restrict__ in_off, long long N_in,
                                                                    const double* __restrict__ t_out, const long long* __restrict__ out_off,
                                                                    long long N_out, int R, double delay, double max_hold, int mode,
                                                                    int depth, float* __restrict__ out, unsigned char* __restrict__ flags) {
    const long long row = (long long)blockIdx.x * rs::TILE + threadIdx.x / sn::SENSORS;
    const int k = threadIdx.x % sn::SENSORS;
    if (row >= N_out) return;
    float* o = out + row * sn::PACKET + 7 * k;
    int lo = 0, hi = R;                                          // the last j with out_off[j] <= row
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (out_off[mid] <= row) lo = mid;
        else hi = mid;
    }
    if (R < 1 || row < out_off[lo] || row >= out_off[lo + 1]) {  // a row no sequence owns
        resample_nan7(o);
        if (k == 0) flags[row] = (unsigned char)rs::F_EMPTY;
        return;
    }
    const long long b0 = clamp_ll(in_off[lo], 0, N_in), b1 = clamp_ll(in_off[lo + 1], b0, N_in);
    const double tk = t_out[row];
    long long c0 = 0, c1 = b1 - b0;                              // the packets not after the tick: stamps[b0 + c] <= tk for c < c0
    while (c0 < c1) {
        const long long mid = (c0 + c1) >> 1;
        if (stamps[b0 + mid] <= tk) c0 = mid + 1;
        else c1 = mid;
    }
    const int cnt = c0 < depth ? (int)c0 : depth;                // of these the last `depth`
    const long long first = b0 + c0 - cnt;
    int i;
    double u;
    const int f = resample_decide([&](int j) { return stamps[first + j]; }, cnt, tk - delay, max_hold, mode, i, u);
    const float* a = packets + (first + i) * sn::PACKET + 7 * k;
    if (f == rs::F_INTERP) resample_sensor(a, a + sn::PACKET, u, o);
    else if (f == rs::F_HELD) resample_copy7(a, o);
    else resample_nan7(o);
    if (k == 0) flags[row] = (unsigned char)f;
}

}  // namespace tip

using namespace tip;

extern "C" {

static bool rs_bad_n(long long n) { return n < 0 || n > (1ll << 24); }
static bool rs_bad_rows(long long n) { return n < 0 || n > (1ll << 40); }
static bool rs_bad_depth(int depth) { return depth < rs::MIN_DEPTH || depth > rs::MAX_DEPTH; }
static bool rs_bad_state(const void* state) { return !state || reinterpret_cast<uintptr_t>(state) % 8; }
// delay: finite and >= 0 (nothing is extrapolated past the newest packet); max_hold: < 0 for no limit, never NaN; mode: HOLD or SLERP
static bool rs_bad_rule(double delay, double max_hold, int mode) {
    return !(delay >= 0.0) || !__builtin_isfinite(delay) || max_hold != max_hold || (mode != rs::HOLD && mode != rs::SLERP);
}

int tip_resample_tile(int* rows) {
    if (!rows) return TIP_ERR_INVALID_ARG;
    *rows = rs::TILE;
    return TIP_OK;
}

int tip_resample_state_bytes(int n_slots, int depth, size_t* bytes) {
    if (!bytes || rs_bad_n(n_slots) || rs_bad_depth(depth)) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)n_slots * rs::slot_bytes(depth);
    return TIP_OK;
}

int tip_resample_reset(void* state, int n_slots, int depth, const int* slots, int count, tip_stream_t stream) {
    if (rs_bad_state(state) || rs_bad_n(n_slots) || rs_bad_depth(depth) || count < 0) return TIP_ERR_INVALID_ARG;
    const int blocks = slots ? count : n_slots;
    if (blocks == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(resample_reset_kernel, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), state, n_slots, depth, slots);
    return tip_launch_status();
}

int tip_resample_push(void* state, int n_slots, int depth, const float* packets, const int* slots, const double* times, int m,
                      tip_stream_t stream) {
    if (rs_bad_state(state) || rs_bad_n(n_slots) || rs_bad_depth(depth) || m < 0 || (m > 0 && (!packets || !slots || !times)))
        return TIP_ERR_INVALID_ARG;
    if (m == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(resample_push_kernel, dim3(n_slots), dim3(64), 0, static_cast<hipStream_t>(stream), state, n_slots, depth, packets,
                       slots, times, m);
    return tip_launch_status();
}

int tip_resample_emit(void* state, int n_slots, int depth, const double* t, double delay, double max_hold, int mode, float* packets_out,
                      unsigned char* flags, tip_stream_t stream) {
    if (rs_bad_state(state) || rs_bad_n(n_slots) || rs_bad_depth(depth) || !t || !packets_out || !flags || rs_bad_rule(delay, max_hold, mode))
        return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(resample_emit_kernel, dim3((n_slots + rs::TILE - 1) / rs::TILE), dim3(rs::THREADS), 0,
                       static_cast<hipStream_t>(stream), state, n_slots, depth, t, delay, max_hold, mode, packets_out, flags);
    return tip_launch_status();
}

int tip_resample_get(const void* state, int n_slots, int depth, const int* slots, int count, int* counts_out, tip_stream_t stream) {
    if (rs_bad_state(state) || rs_bad_n(n_slots) || rs_bad_depth(depth) || count < 0 || (count > 0 && (!slots || !counts_out)))
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(resample_get_kernel, dim3((count + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), state, n_slots, depth,
                       slots, count, counts_out);
    return tip_launch_status();
}

int tip_resample_rows(const float* packets, const double* stamps, const long long* in_offsets, long long n_in, const double* t_out,
                      const long long* out_offsets, long long n_out, int n_seq, double delay, double max_hold, int mode, int depth,
                      float* packets_out, unsigned char* flags, tip_stream_t stream) {
    if (rs_bad_rows(n_in) || rs_bad_rows(n_out) || rs_bad_n(n_seq) || rs_bad_depth(depth) || rs_bad_rule(delay, max_hold, mode) ||
        !in_offsets || !out_offsets || (n_in > 0 && (!packets || !stamps)) || (n_out > 0 && (!t_out || !packets_out || !flags)))
        return TIP_ERR_INVALID_ARG;
    if (n_out == 0) return TIP_OK;
    const long long blocks = (n_out + rs::TILE - 1) / rs::TILE;
    if (blocks > 0x7fffffffll) return TIP_ERR_INVALID_ARG;
    hipLaunchKernelGGL(resample_rows_kernel, dim3((unsigned)blocks), dim3(rs::THREADS), 0, static_cast<hipStream_t>(stream), packets, stamps,
                       in_offsets, n_in, t_out, out_offsets, n_out, n_seq, delay, max_hold, mode, depth, packets_out, flags);
    return tip_launch_status();
}

}  // extern "C"
