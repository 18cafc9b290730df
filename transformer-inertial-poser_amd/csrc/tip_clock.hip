// tip_clock.hip — timestamped packets whose stamps are on the SENSOR's clock, and ticks that want a packet AT the tick (include/tip_hip.h,
// "clock sync and predicted ticks").  The reference has neither: its reader thread keeps no stamps at all (live_demo_new.py:82-115).
//
//   clock_map_kernel       one wave per slot, the arrival list scanned 64 entries at a time by ballot as resample_push_kernel scans it; the
//                          slot's arrivals step clock_step in array order and lane 0 writes the mapped time of each
//   clock_push_kernel      the same scan with resample_push_kernel's ring insert behind the mapping: one launch for what clock_map_kernel
//                          followed by resample_push_kernel leave, bit for bit
//   clock_rows_kernel      R ragged recorded sequences, one wave per sequence: 64 (stamp, arrival) pairs are loaded at once, stepped in order
//                          out of the lanes' registers, and 64 mapped times are written at once.  The rule is a sequential scan, so the step
//                          count of a launch is the longest sequence's length; what the wave saves is the memory round trip per step
//   clock_reset_kernel / clock_get_kernel   one thread per listed block
//   predict_emit_kernel / predict_rows_kernel   resample_emit_kernel / resample_rows_kernel with predict_decide in front of
//                          resample_decide and predict_sensor beside resample_sensor; every row that is not predicted goes through the
//                          shared functions of tip_resample.h with mode SLERP
//
// Every time and every decision is fp64 in the header's statement order (the library is built with -ffp-contract=off: no statement here is
// fused); packet arithmetic is fp32 as in resample_sensor.  Nothing waits on another workgroup, nothing reads the environment; a listed
// slot outside [0, n) is skipped, offsets are clamped before they index anything, a block is written only by the wave whose slot it is.
#include "tip_resample.h"

namespace tip {

namespace ck {
constexpr double PREDICT_SPAN = TIP_PREDICT_SPAN;            // a row is predicted at most this many brackets past the newest packet
constexpr int F_PREDICT = TIP_RESAMPLE_PREDICTED;
}  // namespace ck

// One slot's clock: 32 bytes, a reset block all zero bits.
struct ClockSlot {
    double theta;                                            // the offset estimate: mapped = stamp + theta
    double s_prev;                                           // the last accepted stamp
    int count, rejected;
    int pad[2];
};
static_assert(sizeof(ClockSlot) == 32, "ClockSlot layout");

// The header's rule, statement for statement: -> the mapped time, NaN for a rejected arrival.
__device__ __forceinline__ double clock_step(double& theta, double& s_prev, int& count, int& rejected, double s, double a, double leak,
                                             double slew) {
    if (!__builtin_isfinite(s) || !__builtin_isfinite(a) || (count > 0 && s <= s_prev)) {
        rejected += 1;
        return __builtin_nan("");
    }
    const double o = a - s;
    if (count == 0) {
        theta = o;
    } else {
        const double d = s - s_prev;
        const double up = theta + leak * d;
        const double dn = theta - slew * d;
        const double th = o < up ? o : up;
        theta = th > dn ? th : dn;
    }
    s_prev = s;
    count += 1;
    return s + theta;
}

// ---- live ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void clock_map_kernel(ClockSlot* __restrict__ clock, int n, const int* __restrict__ slots,
                                                       const double* __restrict__ stamps, const double* __restrict__ arrivals, int m,
                                                       double leak, double slew, double* __restrict__ times_out) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot >= n) return;
    ClockSlot& c = clock[slot];
    double theta = c.theta, s_prev = c.s_prev;
    int count = c.count, rejected = c.rejected;
    bool any = false;
    for (int base = 0; base < m; base += 64) {
        const int j0 = base + lane;
        unsigned long long mask = __ballot(j0 < m && slots[j0] == slot);
        while (mask) {                                           // the slot's arrivals of this group, in array order (wave-uniform)
            const int j = base + __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            any = true;
            const double t = clock_step(theta, s_prev, count, rejected, stamps[j], arrivals[j], leak, slew);
            if (lane == 0) times_out[j] = t;
        }
    }
    if (any && lane == 0) c.theta = theta, c.s_prev = s_prev, c.count = count, c.rejected = rejected;
}

// resample_push_kernel's text with the stamp mapped first; times_out may be null.
__global__ __launch_bounds__(64) void clock_push_kernel(void* state, ClockSlot* __restrict__ clock, int n, int depth,
                                                        const float* __restrict__ packets, const int* __restrict__ slots,
                                                        const double* __restrict__ stamps, const double* __restrict__ arrivals, int m,
                                                        double leak, double slew, double* __restrict__ times_out) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot >= n) return;
    const ResampleSlot st = resample_slot(state, slot, depth);
    int head = clamp_int(st.hdr[0], 0, depth - 1), have = clamp_int(st.hdr[1], 0, depth);
    int total = st.hdr[2], dropped = st.hdr[3];
    double newest = have > 0 ? st.stamp[(head + have - 1) % depth] : 0.0;
    ClockSlot& c = clock[slot];
    double theta = c.theta, s_prev = c.s_prev;
    int count = c.count, rejected = c.rejected;
    bool any = false;
    for (int base = 0; base < m; base += 64) {
        const int j0 = base + lane;
        unsigned long long mask = __ballot(j0 < m && slots[j0] == slot);
        while (mask) {
            const int j = base + __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            any = true;
            const double t = clock_step(theta, s_prev, count, rejected, stamps[j], arrivals[j], leak, slew);
            if (times_out && lane == 0) times_out[j] = t;
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
    if (any && lane == 0) {
        st.hdr[0] = head, st.hdr[1] = have, st.hdr[2] = total, st.hdr[3] = dropped;
        c.theta = theta, c.s_prev = s_prev, c.count = count, c.rejected = rejected;
    }
}

// One thread per list entry (slots given) or per slot (slots null).
__global__ __launch_bounds__(64) void clock_reset_kernel(ClockSlot* __restrict__ clock, int n, const int* __restrict__ slots, int blocks) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= blocks) return;
    const int slot = slots ? slots[j] : j;
    if (slot < 0 || slot >= n) return;
    unsigned long long* w = reinterpret_cast<unsigned long long*>(clock + slot);
    w[0] = 0ull, w[1] = 0ull, w[2] = 0ull, w[3] = 0ull;
}

__global__ __launch_bounds__(64) void clock_get_kernel(const ClockSlot* __restrict__ clock, int n, const int* __restrict__ slots, int count,
                                                       double* __restrict__ theta_out, int* __restrict__ counts_out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count) return;
    const int slot = slots[j];
    if (slot < 0 || slot >= n) return;
    theta_out[j] = clock[slot].theta;
    counts_out[2 * (size_t)j] = clock[slot].count, counts_out[2 * (size_t)j + 1] = clock[slot].rejected;
}

// ---- recorded sequences -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void clock_rows_kernel(const double* __restrict__ stamps, const double* __restrict__ arrivals,
                                                        const long long* __restrict__ off, long long N_in, int R, double leak, double slew,
                                                        double* __restrict__ times_out) {
    const int seq = blockIdx.x, lane = threadIdx.x;
    if (seq >= R) return;
    const long long b0 = clamp_ll(off[seq], 0, N_in), b1 = clamp_ll(off[seq + 1], b0, N_in);
    double theta = 0.0, s_prev = 0.0;                            // a reset block
    int count = 0, rejected = 0;
    for (long long base = b0; base < b1; base += 64) {
        const long long j = base + lane;
        const double s_l = j < b1 ? stamps[j] : 0.0, a_l = j < b1 ? arrivals[j] : 0.0;
        const int cnt = b1 - base < 64 ? (int)(b1 - base) : 64;
        double mine = 0.0;
        for (int k = 0; k < cnt; ++k) {                          // in order, every lane the same numbers
            const double t = clock_step(theta, s_prev, count, rejected, __shfl(s_l, k), __shfl(a_l, k), leak, slew);
            if (lane == k) mine = t;
        }
        if (j < b1) times_out[j] = mine;
    }
}

// ---- predicted ticks ----------------------------------------------------------------------------------------------------------------------
// The header's decision: tau past the newest of at least two packets, no further than max_predict and PREDICT_SPAN brackets, the bracket
// no longer than max_hold -> F_PREDICT, i = cnt - 2 and u = (tau - s_prev) / b > 1; anything else is resample_decide in mode SLERP.
template <typename Stamp>
__device__ __forceinline__ int predict_decide(Stamp stamp, int cnt, double tau, double max_hold, double max_predict, int& i, double& u) {
    if (cnt >= 2) {
        const double s_last = stamp(cnt - 1);
        if (tau > s_last) {
            const double s_prev = stamp(cnt - 2);
            const double h = tau - s_last, b = s_last - s_prev;
            if (h <= max_predict && h <= ck::PREDICT_SPAN * b && (max_hold < 0.0 || b <= max_hold)) {
                i = cnt - 2;
                u = (tau - s_prev) / b;
                return ck::F_PREDICT;
            }
        }
    }
    return resample_decide(stamp, cnt, tau, max_hold, rs::SLERP, i, u);
}

// predict_sensor, one sensor past the newer of two packets, is in tip_resample.h: the display-time poses (tip_display.hip) call it too.
__global__ __launch_bounds__(rs::THREADS) void predict_emit_kernel(void* state, int n, int depth, const double* __restrict__ t,
                                                                   double delay, double max_hold, double max_predict,
                                                                   float* __restrict__ out, unsigned char* __restrict__ flags) {
    const int slot = blockIdx.x * rs::TILE + threadIdx.x / sn::SENSORS, k = threadIdx.x % sn::SENSORS;
    if (slot >= n) return;
    const ResampleSlot st = resample_slot(state, slot, depth);
    const int head = clamp_int(st.hdr[0], 0, depth - 1), have = clamp_int(st.hdr[1], 0, depth);
    const double tau = t[slot] - delay;
    int i;
    double u;
    const int f = predict_decide([&](int j) { return st.stamp[(head + j) % depth]; }, have, tau, max_hold, max_predict, i, u);
    float* o = out + (size_t)slot * sn::PACKET + 7 * k;
    const float* a = st.packet + (size_t)((head + i) % depth) * sn::PACKET + 7 * k;
    const float* b = st.packet + (size_t)((head + i + 1) % depth) * sn::PACKET + 7 * k;
    if (f == ck::F_PREDICT) predict_sensor(a, b, u, o);
    else if (f == rs::F_INTERP) resample_sensor(a, b, u, o);
    else if (f == rs::F_HELD) resample_copy7(a, o);
    else resample_nan7(o);
    if (k == 0) flags[slot] = (unsigned char)f;
}

__global__ __launch_bounds__(rs::THREADS) void predict_rows_kernel(const float* __restrict__ packets, const double* __restrict__ stamps,
                                                                   const long long* __restrict__ in_off, long long N_in,
                                                                   const double* __restrict__ t_out, const long long* __restrict__ out_off,
                                                                   long long N_out, int R, double delay, double max_hold,
                                                                   double max_predict, int depth, float* __restrict__ out,
                                                                   unsigned char* __restrict__ flags) {
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
    const int f = predict_decide([&](int j) { return stamps[first + j]; }, cnt, tk - delay, max_hold, max_predict, i, u);
    const float* a = packets + (first + i) * sn::PACKET + 7 * k;
    if (f == ck::F_PREDICT) predict_sensor(a, a + sn::PACKET, u, o);
    else if (f == rs::F_INTERP) resample_sensor(a, a + sn::PACKET, u, o);
    else if (f == rs::F_HELD) resample_copy7(a, o);
    else resample_nan7(o);
    if (k == 0) flags[row] = (unsigned char)f;
}

}  // namespace tip

using namespace tip;

extern "C" {

static bool ck_bad_n(long long n) { return n < 0 || n > (1ll << 24); }
static bool ck_bad_rows(long long n) { return n < 0 || n > (1ll << 40); }
static bool ck_bad_depth(int depth) { return depth < rs::MIN_DEPTH || depth > rs::MAX_DEPTH; }
static bool ck_bad_state(const void* state) { return !state || reinterpret_cast<uintptr_t>(state) % 8; }
// leak: finite and >= 0; slew: in [0, 1) (at 1 two stamps could map to one time)
static bool ck_bad_rule(double leak, double slew) { return !(leak >= 0.0) || !__builtin_isfinite(leak) || !(slew >= 0.0) || !(slew < 1.0); }
// delay, max_predict: finite and >= 0; max_hold: < 0 for no limit, never NaN
static bool ck_bad_predict(double delay, double max_hold, double max_predict) {
    return !(delay >= 0.0) || !__builtin_isfinite(delay) || max_hold != max_hold || !(max_predict >= 0.0) || !__builtin_isfinite(max_predict);
}

int tip_clock_state_bytes(int n_slots, size_t* bytes) {
    if (!bytes || ck_bad_n(n_slots)) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)n_slots * sizeof(ClockSlot);
    return TIP_OK;
}

int tip_clock_reset(void* state, int n_slots, const int* slots, int count, tip_stream_t stream) {
    if (ck_bad_state(state) || ck_bad_n(n_slots) || count < 0) return TIP_ERR_INVALID_ARG;
    const int blocks = slots ? count : n_slots;
    if (blocks == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(clock_reset_kernel, dim3((blocks + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<ClockSlot*>(state), n_slots, slots, blocks);
    return tip_launch_status();
}

int tip_clock_get(const void* state, int n_slots, const int* slots, int count, double* theta_out, int* counts_out, tip_stream_t stream) {
    if (ck_bad_state(state) || ck_bad_n(n_slots) || count < 0 || (count > 0 && (!slots || !theta_out || !counts_out)))
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(clock_get_kernel, dim3((count + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<const ClockSlot*>(state), n_slots, slots, count, theta_out, counts_out);
    return tip_launch_status();
}

int tip_clock_map(void* state, int n_slots, const int* slots, const double* stamps, const double* arrivals, int m, double leak, double slew,
                  double* times_out, tip_stream_t stream) {
    if (ck_bad_state(state) || ck_bad_n(n_slots) || m < 0 || ck_bad_rule(leak, slew) || (m > 0 && (!slots || !stamps || !arrivals || !times_out)))
        return TIP_ERR_INVALID_ARG;
    if (m == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(clock_map_kernel, dim3(n_slots), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<ClockSlot*>(state), n_slots,
                       slots, stamps, arrivals, m, leak, slew, times_out);
    return tip_launch_status();
}

int tip_clock_push(void* rs_state, void* clock_state, int n_slots, int depth, const float* packets, const int* slots, const double* stamps,
                   const double* arrivals, int m, double leak, double slew, double* times_out, tip_stream_t stream) {
    if (ck_bad_state(rs_state) || ck_bad_state(clock_state) || ck_bad_n(n_slots) || ck_bad_depth(depth) || m < 0 || ck_bad_rule(leak, slew) ||
        (m > 0 && (!packets || !slots || !stamps || !arrivals)))
        return TIP_ERR_INVALID_ARG;
    if (m == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(clock_push_kernel, dim3(n_slots), dim3(64), 0, static_cast<hipStream_t>(stream), rs_state,
                       static_cast<ClockSlot*>(clock_state), n_slots, depth, packets, slots, stamps, arrivals, m, leak, slew, times_out);
    return tip_launch_status();
}

int tip_clock_rows(const double* stamps, const double* arrivals, const long long* offsets, long long n_in, int n_seq, double leak,
                   double slew, double* times_out, tip_stream_t stream) {
    if (ck_bad_rows(n_in) || ck_bad_n(n_seq) || ck_bad_rule(leak, slew) || !offsets || (n_in > 0 && (!stamps || !arrivals || !times_out)))
        return TIP_ERR_INVALID_ARG;
    if (n_in == 0 || n_seq == 0) return TIP_OK;
    hipLaunchKernelGGL(clock_rows_kernel, dim3(n_seq), dim3(64), 0, static_cast<hipStream_t>(stream), stamps, arrivals, offsets, n_in, n_seq,
                       leak, slew, times_out);
    return tip_launch_status();
}

int tip_predict_emit(void* state, int n_slots, int depth, const double* t, double delay, double max_hold, double max_predict,
                     float* packets_out, unsigned char* flags, tip_stream_t stream) {
    if (ck_bad_state(state) || ck_bad_n(n_slots) || ck_bad_depth(depth) || !t || !packets_out || !flags ||
        ck_bad_predict(delay, max_hold, max_predict))
        return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(predict_emit_kernel, dim3((n_slots + rs::TILE - 1) / rs::TILE), dim3(rs::THREADS), 0,
                       static_cast<hipStream_t>(stream), state, n_slots, depth, t, delay, max_hold, max_predict, packets_out, flags);
    return tip_launch_status();
}

int tip_predict_rows(const float* packets, const double* stamps, const long long* in_offsets, long long n_in, const double* t_out,
                     const long long* out_offsets, long long n_out, int n_seq, double delay, double max_hold, double max_predict, int depth,
                     float* packets_out, unsigned char* flags, tip_stream_t stream) {
    if (ck_bad_rows(n_in) || ck_bad_rows(n_out) || ck_bad_n(n_seq) || ck_bad_depth(depth) || ck_bad_predict(delay, max_hold, max_predict) ||
        !in_offsets || !out_offsets || (n_in > 0 && (!packets || !stamps)) || (n_out > 0 && (!t_out || !packets_out || !flags)))
        return TIP_ERR_INVALID_ARG;
    if (n_out == 0) return TIP_OK;
    const long long blocks = (n_out + rs::TILE - 1) / rs::TILE;
    if (blocks > 0x7fffffffll) return TIP_ERR_INVALID_ARG;
    hipLaunchKernelGGL(predict_rows_kernel, dim3((unsigned)blocks), dim3(rs::THREADS), 0, static_cast<hipStream_t>(stream), packets, stamps,
                       in_offsets, n_in, t_out, out_offsets, n_out, n_seq, delay, max_hold, max_predict, depth, packets_out, flags);
    return tip_launch_status();
}

}  // extern "C"
