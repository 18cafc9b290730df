// tip_fill.hip — missing IMU readings: the reference's answer to sensors that deliver nothing for a frame, on the device, for the
// recorded files (preprocess_DIP_TC_new.py), for the live front end and for recorded sessions.
//
//   :112-136   fill_in_nan_values: a sensor's rotation (9 values) or acceleration (3 values) of a row is BAD when the sum of its values
//              is NaN, and a bad part is replaced as a whole by the column-wise nanmean of rows 0..9 (t <= 10) or of the five rows before
//              it (t > 10) — of the values as they are by then, earlier fills included
//   :160-180   get_real_imu_readings_ours_format_knee: six of the recording's sensors, filled, rotated by ROT_MAT_OURS, as [L, 72]
//
// Rule R ("reference") is that, on a whole sequence.  Rule V ("live") is what a stream can do, which cannot look ahead: per part a
// ring of the last five rows AFTER filling; a bad part becomes the mean of the ring (fp32, oldest to newest, one correctly rounded
// division), is pushed and counted; a bad part with an empty ring, or after `max_gap` consecutive fills, becomes NaN as a whole and is
// not pushed.  V equals R on every row t > 10 when rows 0..10 are clean.  Kernels:
//
//   fill_real_kernel      rule R, fp64: one workgroup per sequence, one wave per selected sensor, tiles of 64 rows in LDS (five rows
//                         of the tile before in front); lanes 0-11, one per component, walk the tile's bad rows; all lanes rotate and
//                         store.  A tile without a bad part does no walk.
//   fill_rows_kernel      rule V on ragged sequences of frames [N, 72], one thread per (sequence, part), the ring in registers
//   fill_live_kernel      rule V for one frame of n slots, one thread per (slot, part), the ring in the caller's state buffer; a slot
//                         whose calibration is not live is skipped
//   fill_packets_kernel   tip_sensor_transform's arithmetic (tip_sensor.h: sensor_row) on N recorded packet rows, the table by sequence
//   fill_reset_kernel / fill_get_kernel     the state blocks of all or of the listed slots to zero; have / run / total copied out
//
// Nothing waits on another workgroup, nothing reads the environment; a listed slot outside [0, n) is skipped, offsets are clamped to
// [0, N] and to ascending order before they index anything.
#include "tip_sensor.h"

namespace tip {

namespace fl {
constexpr int PARTS = 12, RING = 5, TILE = 64, PITCH = 13;          // PITCH: 12 components + 1, odd in doubles
__device__ __forceinline__ int part_col(int p) { return p < 6 ? 9 * p : 54 + 3 * (p - 6); }
}  // namespace fl

// One slot's rings.  ring[j] is a whole 72-column row; part p's oldest row is ring[head[p]], its newest ring[(head[p] + 4) % 5], and the
// newest have[p] of them are valid.  1632 bytes.
struct FillSlot {
    float ring[fl::RING][sn::RAW];
    int have[fl::PARTS], head[fl::PARTS], run[fl::PARTS], total[fl::PARTS];
};
static_assert(sizeof(FillSlot) == 1632, "FillSlot layout");

struct FillRealArgs {
    int sel[6];
    double rot[9];
};

// ---- rule V: one part (W = 9 or 3 values), one row -------------------------------------------------------------------------------------
template <int W>
struct FillPart {
    float ring[fl::RING][W];                                     // ring[4] the newest; the last `have` are valid
    int have, run, total;
};

template <int W>
__device__ __forceinline__ void fill_push(FillPart<W>& s, const float* v) {
#pragma unroll
    for (int c = 0; c < W; ++c) {
#pragma unroll
        for (int j = 0; j < fl::RING - 1; ++j) s.ring[j][c] = s.ring[j + 1][c];
        s.ring[fl::RING - 1][c] = v[c];
    }
    if (s.have < fl::RING) s.have += 1;
}

// v[W] in and out.  Returns 0 (good: pushed), 1 (filled: pushed) or 2 (bad and left: all of v is NaN, nothing pushed).
template <int W>
__device__ __forceinline__ int fill_step(FillPart<W>& s, float* v, int max_gap) {
    float sum = 0.f;
#pragma unroll
    for (int c = 0; c < W; ++c) sum += v[c];
    if (!__builtin_isnan(sum)) {
        fill_push<W>(s, v);
        s.run = 0;
        return 0;
    }
    if (s.have < 1 || (max_gap >= 0 && s.run >= max_gap)) {
#pragma unroll
        for (int c = 0; c < W; ++c) v[c] = __builtin_nanf("");
        return 2;
    }
    const float cnt = (float)s.have;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < fl::RING; ++j)
            if (j >= fl::RING - s.have) m += s.ring[j][c];
        v[c] = __fdiv_rn(m, cnt);
    }
    fill_push<W>(s, v);
    s.run += 1;
    s.total += 1;
    return 1;
}

// offsets[r], offsets[r + 1] as a row range inside [0, N]
__device__ __forceinline__ void fill_range(const long long* __restrict__ offsets, int r, long long N, long long& b0, long long& b1) {
    long long a = offsets[r], b = offsets[r + 1];
    a = a < 0 ? 0 : (a > N ? N : a);
    b = b < a ? a : (b > N ? N : b);
    b0 = a, b1 = b;
}

template <int W>
__device__ __forceinline__ void fill_rows_part(const float* frames, float* out, long long b0, long long b1, int p, int col, int max_gap,
                                               unsigned char* __restrict__ flags) {
    FillPart<W> s;
    s.have = s.run = s.total = 0;
#pragma unroll
    for (int j = 0; j < fl::RING; ++j)
#pragma unroll
        for (int c = 0; c < W; ++c) s.ring[j][c] = 0.f;
    for (long long t = b0; t < b1; ++t) {
        float v[W];
#pragma unroll
        for (int c = 0; c < W; ++c) v[c] = frames[t * sn::RAW + col + c];
        const int f = fill_step<W>(s, v, max_gap);
        if (f != 0 || out != frames) {
#pragma unroll
            for (int c = 0; c < W; ++c) out[t * sn::RAW + col + c] = v[c];
        }
        flags[t * fl::PARTS + p] = (unsigned char)f;
    }
}

__global__ __launch_bounds__(256) void fill_rows_kernel(const float* frames, float* out, long long N, const long long* __restrict__ offsets,
                                                        int R, int max_gap, unsigned char* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int r = i / fl::PARTS, p = i - r * fl::PARTS;
    if (r >= R) return;
    long long b0, b1;
    fill_range(offsets, r, N, b0, b1);
    if (p < 6) fill_rows_part<9>(frames, out, b0, b1, p, fl::part_col(p), max_gap, flags);
    else fill_rows_part<3>(frames, out, b0, b1, p, fl::part_col(p), max_gap, flags);
}

template <int W>
__device__ __forceinline__ void fill_live_part(FillSlot& st, float* __restrict__ row, int p, int col, int max_gap,
                                               unsigned char* __restrict__ flag) {
    int head = st.head[p];
    head = head < 0 || head >= fl::RING ? 0 : head;
    FillPart<W> s;
    s.have = st.have[p], s.run = st.run[p], s.total = st.total[p];
    s.have = s.have < 0 ? 0 : (s.have > fl::RING ? fl::RING : s.have);
#pragma unroll
    for (int j = 0; j < fl::RING; ++j) {
        const int q = (head + j) % fl::RING;
#pragma unroll
        for (int c = 0; c < W; ++c) s.ring[j][c] = st.ring[q][col + c];
    }
    float v[W];
#pragma unroll
    for (int c = 0; c < W; ++c) v[c] = row[c];
    const int f = fill_step<W>(s, v, max_gap);
    if (f != 0) {
#pragma unroll
        for (int c = 0; c < W; ++c) row[c] = v[c];
    }
    if (f != 2) {                                               // pushed: the oldest row of the ring is the one that goes
#pragma unroll
        for (int c = 0; c < W; ++c) st.ring[head][col + c] = v[c];
        st.head[p] = (head + 1) % fl::RING;
        st.have[p] = s.have;
    }
    st.run[p] = s.run;
    st.total[p] = s.total;
    *flag = (unsigned char)f;
}

__global__ __launch_bounds__(256) void fill_live_kernel(FillSlot* __restrict__ state, const SensorCal* __restrict__ cal,
                                                        float* __restrict__ raw, int n, int max_gap, unsigned char* __restrict__ flags) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int slot = i / fl::PARTS, p = i - slot * fl::PARTS;
    if (slot >= n) return;
    unsigned char* flag = flags + (size_t)slot * fl::PARTS + p;
    if (cal[slot].phase != sn::LIVE) {                          // its NaN row stays, its rings are not touched
        *flag = 0;
        return;
    }
    const int col = fl::part_col(p);
    float* row = raw + (size_t)slot * sn::RAW + col;
    if (p < 6) fill_live_part<9>(state[slot], row, p, col, max_gap, flag);
    else fill_live_part<3>(state[slot], row, p, col, max_gap, flag);
}

// blockIdx.x: a list entry (slots given) or a slot (slots null); 128 threads zero the block's 408 words.
__global__ __launch_bounds__(128) void fill_reset_kernel(FillSlot* __restrict__ state, int n, const int* __restrict__ slots) {
    const int slot = slots ? slots[blockIdx.x] : (int)blockIdx.x;
    if (slot < 0 || slot >= n) return;
    unsigned* wds = reinterpret_cast<unsigned*>(state + slot);
    for (int t = threadIdx.x; t < (int)(sizeof(FillSlot) / 4); t += 128) wds[t] = 0u;
}

__global__ __launch_bounds__(64) void fill_get_kernel(const FillSlot* __restrict__ state, int n, const int* __restrict__ slots,
                                                      int* __restrict__ out) {
    const int slot = slots[blockIdx.x], t = threadIdx.x;
    if (slot < 0 || slot >= n || t >= 3 * fl::PARTS) return;
    const FillSlot& st = state[slot];
    const int which = t / fl::PARTS, p = t - which * fl::PARTS;
    out[(size_t)blockIdx.x * 3 * fl::PARTS + t] = which == 0 ? st.have[p] : (which == 1 ? st.run[p] : st.total[p]);
}

__global__ __launch_bounds__(256) void fill_packets_kernel(const float* __restrict__ tables, const float* __restrict__ packets, long long N,
                                                           const long long* __restrict__ offsets, int R, float max_acc,
                                                           float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = i / sn::SENSORS;
    const int k = (int)(i - row * sn::SENSORS);
    if (row >= N) return;
    int lo = 0, hi = R;                                          // the last r with offsets[r] <= row
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= row) lo = mid;
        else hi = mid;
    }
    if (row < offsets[lo] || row >= offsets[lo + 1]) return;     // a row no sequence owns is not written
    sensor_row(tables + (size_t)lo * sn::TABLE, true, packets + row * sn::PACKET + 7 * k, k, max_acc, out + row * sn::RAW + 9 * k,
               out + row * sn::RAW + 54 + 3 * k);
}

// ---- rule R ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool part_bad(const double* v, int w) {
    double s = 0.0;
    for (int c = 0; c < w; ++c) s += v[c];
    return __builtin_isnan(s);
}

__global__ __launch_bounds__(384) void fill_real_kernel(const double* __restrict__ ori, const double* __restrict__ acc, long long N, int S,
                                                        const long long* __restrict__ offsets, FillRealArgs args,
                                                        double* __restrict__ out, int* __restrict__ unfilled) {
    __shared__ double buf_all[6][(fl::RING + fl::TILE) * fl::PITCH];
    __shared__ int unf;
    const int seq = blockIdx.x, k = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double* buf = buf_all[k];                                    // rows 0..4: the last five rows of the tile before; 5..68: this tile
    if (threadIdx.x == 0) unf = 0;
    long long b0, b1;
    fill_range(offsets, seq, N, b0, b1);
    const long long L = b1 - b0;
    const int src = args.sel[k];
    const int first = L < 10 ? (int)L : 10;                      // rows 0 .. first-1 serve every t <= 10
    int left = 0;
    for (long long base = 0; base < L; base += fl::TILE) {
        const int rows = L - base < fl::TILE ? (int)(L - base) : fl::TILE;
        bool bad_r = false, bad_a = false;
        if (lane < rows) {
            double v[12];
            const size_t at = (size_t)(b0 + base + lane) * S + src;
            for (int c = 0; c < 9; ++c) v[c] = ori[at * 9 + c];
            for (int c = 0; c < 3; ++c) v[9 + c] = acc[at * 3 + c];
            bad_r = part_bad(v, 9), bad_a = part_bad(v + 9, 3);  // the mask: from the data as it came
            for (int c = 0; c < 12; ++c) buf[(fl::RING + lane) * fl::PITCH + c] = v[c];
        }
        const unsigned long long m_r = __ballot(bad_r), m_a = __ballot(bad_a);
        __syncthreads();
        if ((m_r | m_a) != 0ull && lane < 12) {
            unsigned long long m = lane < 9 ? m_r : m_a;
            while (m) {
                const int j = __ffsll((long long)m) - 1;
                m &= m - 1;
                double s = 0.0;
                int cnt = 0;
                if (base + j <= 10) {                            // (tile 0 only: its rows sit at 5 ..)
                    for (int q = 0; q < first; ++q) {
                        const double x = buf[(fl::RING + q) * fl::PITCH + lane];
                        if (!__builtin_isnan(x)) s += x, cnt += 1;
                    }
                } else {
                    for (int q = 0; q < fl::RING; ++q) {         // rows t-5 .. t-1
                        const double x = buf[(j + q) * fl::PITCH + lane];
                        if (!__builtin_isnan(x)) s += x, cnt += 1;
                    }
                }
                buf[(fl::RING + j) * fl::PITCH + lane] = cnt ? s / (double)cnt : __builtin_nan("");
            }
        }
        __syncthreads();
        if (lane < rows) {
            double v[12];
            for (int c = 0; c < 12; ++c) v[c] = buf[(fl::RING + lane) * fl::PITCH + c];
            left += (part_bad(v, 9) ? 1 : 0) + (part_bad(v + 9, 3) ? 1 : 0);
            double* o = out + (size_t)(b0 + base + lane) * sn::RAW;
            const double* Rm = args.rot;
            for (int j = 0; j < 3; ++j) {
                for (int q = 0; q < 3; ++q) o[9 * k + 3 * j + q] = (Rm[3 * j] * v[q] + Rm[3 * j + 1] * v[3 + q]) + Rm[3 * j + 2] * v[6 + q];
                o[54 + 3 * k + j] = (Rm[3 * j] * v[9] + Rm[3 * j + 1] * v[10]) + Rm[3 * j + 2] * v[11];
            }
        }
        if (base + fl::TILE < L) {                               // (a full tile) its last five rows go in front of the next
            double keep = 0.0;
            const int cr = lane / 12, cc = lane - cr * 12;
            if (lane < 60) keep = buf[(fl::TILE + cr) * fl::PITCH + cc];
            __syncthreads();
            if (lane < 60) buf[cr * fl::PITCH + cc] = keep;
        }
    }
    if (left) atomicAdd(&unf, left);
    __syncthreads();
    if (threadIdx.x == 0) unfilled[seq] = unf;
}

}  // namespace tip

using namespace tip;

extern "C" {

static bool fill_bad_n(long long n) { return n < 0 || n > (1ll << 24); }
static bool fill_bad_rows(long long n) { return n < 0 || n > (1ll << 40); }

int tip_fill_real(const double* ori, const double* acc, long long n_rows, int n_sensors, const long long* offsets, int n_seq,
                  const int* sel, const double* rot, double* out, int* unfilled, tip_stream_t stream) {
    if (!ori || !acc || !offsets || !sel || !rot || !out || !unfilled || fill_bad_rows(n_rows) || fill_bad_n(n_seq) || n_sensors < 1 ||
        n_sensors > 1024)
        return TIP_ERR_INVALID_ARG;
    FillRealArgs args;
    for (int i = 0; i < 6; ++i) {
        if (sel[i] < 0 || sel[i] >= n_sensors) return TIP_ERR_INVALID_ARG;
        args.sel[i] = sel[i];
    }
    for (int i = 0; i < 9; ++i) args.rot[i] = rot[i];
    if (n_seq == 0) return TIP_OK;
    hipLaunchKernelGGL(fill_real_kernel, dim3(n_seq), dim3(384), 0, static_cast<hipStream_t>(stream), ori, acc, n_rows, n_sensors, offsets,
                       args, out, unfilled);
    return tip_launch_status();
}

int tip_fill_rows(const float* frames, float* out, long long n_rows, const long long* offsets, int n_seq, int max_gap,
                  unsigned char* flags, tip_stream_t stream) {
    if (!frames || !out || !offsets || !flags || fill_bad_rows(n_rows) || fill_bad_n(n_seq) || max_gap < -1) return TIP_ERR_INVALID_ARG;
    if (n_seq == 0 || n_rows == 0) return TIP_OK;
    hipLaunchKernelGGL(fill_rows_kernel, dim3((n_seq * fl::PARTS + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), frames, out,
                       n_rows, offsets, n_seq, max_gap, flags);
    return tip_launch_status();
}

int tip_fill_state_bytes(int n_slots, size_t* bytes) {
    if (!bytes || fill_bad_n(n_slots)) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)n_slots * sizeof(FillSlot);
    return TIP_OK;
}

int tip_fill_reset(void* state, int n_slots, const int* slots, int count, tip_stream_t stream) {
    if (!state || fill_bad_n(n_slots) || count < 0 || reinterpret_cast<uintptr_t>(state) % 4) return TIP_ERR_INVALID_ARG;
    const int blocks = slots ? count : n_slots;
    if (blocks == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(fill_reset_kernel, dim3(blocks), dim3(128), 0, static_cast<hipStream_t>(stream), static_cast<FillSlot*>(state),
                       n_slots, slots);
    return tip_launch_status();
}

int tip_fill_live(void* state, const void* cal, float* raw, int n_slots, int max_gap, unsigned char* flags, tip_stream_t stream) {
    if (!state || !cal || !raw || !flags || fill_bad_n(n_slots) || max_gap < -1) return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(fill_live_kernel, dim3((n_slots * fl::PARTS + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<FillSlot*>(state), static_cast<const SensorCal*>(cal), raw, n_slots, max_gap, flags);
    return tip_launch_status();
}

int tip_fill_get(const void* state, int n_slots, const int* slots, int count, int* counts_out, tip_stream_t stream) {
    if (!state || fill_bad_n(n_slots) || count < 0 || (count > 0 && (!slots || !counts_out))) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(fill_get_kernel, dim3(count), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<const FillSlot*>(state),
                       n_slots, slots, counts_out);
    return tip_launch_status();
}

int tip_fill_packets(const float* tables, const float* packets, long long n_rows, const long long* offsets, int n_seq, float max_acc,
                     float* out, tip_stream_t stream) {
    if (!tables || !packets || !offsets || !out || fill_bad_rows(n_rows) || fill_bad_n(n_seq) || !(max_acc >= 0.f))
        return TIP_ERR_INVALID_ARG;
    if (n_seq == 0 || n_rows == 0) return TIP_OK;
    const long long blocks = (n_rows * sn::SENSORS + 255) / 256;
    if (blocks > 0x7fffffffll) return TIP_ERR_INVALID_ARG;
    hipLaunchKernelGGL(fill_packets_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), tables, packets, n_rows,
                       offsets, n_seq, max_acc, out);
    return tip_launch_status();
}

}  // extern "C"
