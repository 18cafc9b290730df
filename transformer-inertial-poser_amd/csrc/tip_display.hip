// tip_display.hip — display-time poses: the pool's OUTPUT resampled and predicted on the device (include/tip_hip.h, "display-time
// poses").  The reference shows the pose of a frame once per clock.tick(FREQ) (live_demo_new.py:281-307), and that pose belongs to
// IMU_n_smooth = 5 frames before the packet that produced it (real_time_runner.py:279-296, :391-393).  Here a slot keeps a ring of its
// last `depth` poses — the tracker's root and the 18 axis-angles of the engine's s_rest — with their fp64 stamps, and one launch gives
// every slot its pose at the viewer's time: held, interpolated between the two entries around it, or continued past the newest one at
// the angular rate and root velocity of two entries.  A consumer BESIDE the frame, as the trackers and the recorder are.
//
//   pose_push_kernel    one wave per listed slot: lanes 0-56 copy (root, s_rest[:54]) into the ring, lane 0 the stamp and the counters
//   pose_emit_kernel    one thread per (slot, part), 19 parts (18 rotations and the root), dp::TILE slots per workgroup: part 0 of a
//                       slot decides (pose_decide: resample_decide behind the prediction branch) and hands the decision to the other
//                       18 through LDS — the workgroup's one barrier — then every part converts the two rows it reads
//   pose_rows_kernel    the same for R ragged recorded tracks, one thread per (output row, part); part 0 finds the row's track and
//                       the entries a live ring would hold at the row's time by searches, as resample_rows_kernel does
//   pose_reset_kernel / pose_get_kernel   as the packet ring's
//
// Every decision is an fp64 comparison of the header's expressions.  Rotations go axis-angle -> quaternion -> resample_sensor /
// predict_sensor (tip_resample.h: the packet side's own functions, called with a zero acceleration) -> axis-angle; the sines, cosines
// and arctangents of the two conversions are fp64 rounded once, everything else fp32, nothing contracted.  Nothing waits on another
// workgroup, there are no atomics, nothing reads the environment; a listed slot outside [0, n) is skipped, ring indices and offsets
// are clamped before they index anything, and a block is written only by the wave whose slot it is.
#include "tip_resample.h"

namespace tip {

namespace dp {
constexpr int ROTS = 18, PARTS = ROTS + 1, ROW = 3 + 3 * ROTS, QUAT = 4 * ROTS;   // a row: root xyz, then 18 axis-angles
constexpr int TILE = 32, THREADS = TILE * PARTS;             // slots (or rows) of a workgroup, one thread per (slot, part): 608
constexpr int MIN_LD = 3 * ROTS;
enum : int { HOLD = TIP_POSE_HOLD, SLERP = TIP_POSE_SLERP, PREDICT = TIP_POSE_PREDICT };
constexpr int F_PREDICT = TIP_RESAMPLE_PREDICTED;
constexpr float AA_SERIES = 1e-3f;                           // below this angle sin(t / 2) / t is 1/2 - t^2 / 48
constexpr float Q_SERIES = 1e-3f;                            // below this |v| the angle over |v| is 2 + |v|^2 / 3
constexpr float ANTIPODAL = TIP_POSE_ANTIPODAL;              // |qa . qb| at or below this: the rotations are pi apart
static_assert(ROW == 57 && THREADS <= 1024, "layout");
// the packet ring's header, depth stamps, depth rows; padded so that the next block's stamps are 8-byte aligned at an odd depth
__host__ __device__ constexpr size_t slot_bytes(int depth) { return ((size_t)rs::HDR + (size_t)depth * (8 + 4 * ROW) + 7) & ~(size_t)7; }
}  // namespace dp

// One slot's block: int head (the ring index of the oldest entry), have, total, dropped; double stamp[depth]; float row[depth][57].
struct PoseSlot {
    int* hdr;
    double* stamp;
    float* row;
};
__device__ __forceinline__ PoseSlot pose_slot(void* state, int slot, int depth) {
    char* base = static_cast<char*>(state) + (size_t)slot * dp::slot_bytes(depth);
    PoseSlot s;
    s.hdr = reinterpret_cast<int*>(base);
    s.stamp = reinterpret_cast<double*>(base + rs::HDR);
    s.row = reinterpret_cast<float*>(base + rs::HDR + (size_t)depth * 8);
    return s;
}

// ---- the emit decision ------------------------------------------------------------------------------------------------------------------
// The header's: mode PREDICT with tau past the newest of at least two entries, no further than max_predict, and the `b` brackets back
// from the newest no longer than b max_hold -> F_PREDICT, the rows ia = cnt - 1 - b and ib = cnt - 1, u = (tau - s_a) / (s_last - s_a)
// > 1.  There is no span rule.  Anything else is resample_decide (HOLD as HOLD, SLERP and PREDICT as SLERP); ib = ia + 1 for F_INTERP.
template <typename Stamp>
__device__ __forceinline__ int pose_decide(Stamp stamp, int cnt, double tau, double max_hold, double max_predict, int baseline, int mode,
                                           int& ia, int& ib, double& u) {
    if (mode == dp::PREDICT && cnt >= 2) {
        const double s_last = stamp(cnt - 1);
        if (tau > s_last) {
            const int b = baseline < cnt - 1 ? baseline : cnt - 1;
            const double s_a = stamp(cnt - 1 - b);
            const double h = tau - s_last, span = s_last - s_a;
            if (h <= max_predict && (max_hold < 0.0 || span <= (double)b * max_hold)) {
                ia = cnt - 1 - b, ib = cnt - 1;
                u = (tau - s_a) / span;
                return dp::F_PREDICT;
            }
        }
    }
    const int f = resample_decide(stamp, cnt, tau, max_hold, mode == dp::HOLD ? rs::HOLD : rs::SLERP, ia, u);
    ib = f == rs::F_INTERP ? ia + 1 : ia;
    return f;
}

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
// Axis-angle -> quaternion x y z w (the header's statement); a non-finite component gives four NaN.
__device__ __forceinline__ void pose_aa2q(const float* __restrict__ a, float* __restrict__ q) {
    const float t2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    const float t = sqrtf(t2);
    float s;
    if (t < dp::AA_SERIES) s = 0.5f - t2 / 48.f;
    else s = (float)(sin(0.5 * (double)t) / (double)t);
    q[0] = s * a[0], q[1] = s * a[1], q[2] = s * a[2], q[3] = (float)cos(0.5 * (double)t);
}

// Quaternion (unit) -> axis-angle with its angle in [0, pi]; NaN in, NaN out.
__device__ __forceinline__ void pose_q2aa(const float* __restrict__ q, float* __restrict__ a) {
    float x = q[0], y = q[1], z = q[2], w = q[3];
    if (w < 0.f) x = -x, y = -y, z = -z, w = -w;
    const float v2 = x * x + y * y + z * z;
    const float v = sqrtf(v2);
    float k;
    if (v < dp::Q_SERIES) k = 2.f + v2 / 3.f;
    else k = (float)(2.0 * atan2((double)v, (double)w) / (double)v);
    a[0] = k * x, a[1] = k * y, a[2] = k * z;
}

// One part of one output row.  f the decision's flag, (a_root, a_rot) the earlier row's root [3] and axis-angles [54], (b_root, b_rot)
// the later one's (F_HELD reads only a), u the position; q_o the output row [57], quat_o the row's quaternions [18][4] or null.
__device__ __forceinline__ void pose_part(int f, const float* __restrict__ a_root, const float* __restrict__ a_rot,
                                          const float* __restrict__ b_root, const float* __restrict__ b_rot, double u, int part,
                                          float* __restrict__ q_o, float* __restrict__ quat_o) {
    const float nan = __builtin_nanf("");
    const bool two = f == rs::F_INTERP || f == dp::F_PREDICT;
    if (part == dp::ROTS) {                                      // the root: one statement between and past the two entries
        float p[3] = {nan, nan, nan};
        if (f == rs::F_HELD) {
            p[0] = a_root[0], p[1] = a_root[1], p[2] = a_root[2];
        } else if (two) {
            const float pa[3] = {a_root[0], a_root[1], a_root[2]}, pb[3] = {b_root[0], b_root[1], b_root[2]};
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) ok = ok && __builtin_isfinite(pa[c]) && __builtin_isfinite(pb[c]);
            const float uf = (float)u, vf = 1.f - uf;
            if (ok) {
#pragma unroll
                for (int c = 0; c < 3; ++c) p[c] = vf * pa[c] + uf * pb[c];
            }
        }
        q_o[0] = p[0], q_o[1] = p[1], q_o[2] = p[2];
        return;
    }
    float* o = q_o + 3 + 3 * part;
    float* qo = quat_o ? quat_o + 4 * part : nullptr;
    float Q[7] = {nan, nan, nan, nan, 0.f, 0.f, 0.f};
    if (f == rs::F_HELD) {                                       // the row as it was pushed, bit for bit
        const float a[3] = {a_rot[3 * part], a_rot[3 * part + 1], a_rot[3 * part + 2]};
        o[0] = a[0], o[1] = a[1], o[2] = a[2];
        if (qo) {
            pose_aa2q(a, Q);
            qo[0] = Q[0], qo[1] = Q[1], qo[2] = Q[2], qo[3] = Q[3];
        }
        return;
    }
    if (two) {
        const float a[3] = {a_rot[3 * part], a_rot[3 * part + 1], a_rot[3 * part + 2]};
        const float b[3] = {b_rot[3 * part], b_rot[3 * part + 1], b_rot[3 * part + 2]};
        float A[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, B[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // a packet's sensor, no acceleration
        pose_aa2q(a, A);
        pose_aa2q(b, B);
        const float dot = A[0] * B[0] + A[1] * B[1] + A[2] * B[2] + A[3] * B[3];
        if (fabsf(dot) > dp::ANTIPODAL) {                        // (false for a NaN too; pi apart: no shorter arc, the joint is NaN)
            if (f == rs::F_INTERP) resample_sensor(A, B, u, Q);
            else predict_sensor(A, B, u, Q);
        }
    }
    float r[3];
    pose_q2aa(Q, r);
    o[0] = r[0], o[1] = r[1], o[2] = r[2];
    if (qo) qo[0] = Q[0], qo[1] = Q[1], qo[2] = Q[2], qo[3] = Q[3];
}

// ---- live ---------------------------------------------------------------------------------------------------------------------------------
// blockIdx.x: a list entry (slots given) or a slot (slots null)
__global__ __launch_bounds__(64) void pose_push_kernel(void* state, int n, int depth, const int* __restrict__ slots,
                                                       const float* __restrict__ root, const float* __restrict__ s_rest, int ld,
                                                       const unsigned char* __restrict__ valid, const double* __restrict__ t) {
    const int slot = slots ? slots[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
    if (slot < 0 || slot >= n) return;
    if (valid && !valid[slot]) return;
    const PoseSlot st = pose_slot(state, slot, depth);
    int head = clamp_int(st.hdr[0], 0, depth - 1), have = clamp_int(st.hdr[1], 0, depth);
    const int total = st.hdr[2], dropped = st.hdr[3];
    const double ts = t[slot];
    if (!__builtin_isfinite(ts) || (have > 0 && ts <= st.stamp[(head + have - 1) % depth])) {
        if (lane == 0) st.hdr[3] = dropped + 1;
        return;
    }
    int at;
    if (have < depth) {
        at = (head + have) % depth;
        have += 1;
    } else {                                                     // a full ring loses its oldest entry
        at = head;
        head = (head + 1) % depth;
    }
    float* row = st.row + (size_t)at * dp::ROW;
    if (lane < 3) row[lane] = root[(size_t)slot * 3 + lane];
    else if (lane < dp::ROW) row[lane] = s_rest[(size_t)slot * ld + (lane - 3)];
    if (lane == 0) {
        st.stamp[at] = ts;
        st.hdr[0] = head, st.hdr[1] = have, st.hdr[2] = total + 1;
    }
}

__global__ __launch_bounds__(dp::THREADS) void pose_emit_kernel(void* state, int n, int depth, const double* __restrict__ t, double delay,
                                                                double max_hold, double max_predict, int baseline, int mode,
                                                                float* __restrict__ q_out, float* __restrict__ quat_out,
                                                                unsigned char* __restrict__ flags) {
    __shared__ double sh_u[dp::TILE];
    __shared__ int sh_f[dp::TILE], sh_a[dp::TILE], sh_b[dp::TILE];
    const int sl = threadIdx.x / dp::PARTS, part = threadIdx.x - sl * dp::PARTS;
    const int slot = blockIdx.x * dp::TILE + sl;
    const bool live = slot < n;
    if (live && part == 0) {
        const PoseSlot st = pose_slot(state, slot, depth);
        const int head = clamp_int(st.hdr[0], 0, depth - 1), have = clamp_int(st.hdr[1], 0, depth);
        const double tau = t[slot] - delay;
        int ia, ib;
        double u;
        const int f = pose_decide([&](int j) { return st.stamp[(head + j) % depth]; }, have, tau, max_hold, max_predict, baseline, mode, ia,
                                  ib, u);
        sh_f[sl] = f, sh_a[sl] = (head + ia) % depth, sh_b[sl] = (head + ib) % depth, sh_u[sl] = u;
        flags[slot] = (unsigned char)f;
    }
    __syncthreads();                                             // every thread of the workgroup arrives: nothing returned above
    if (!live) return;
    const PoseSlot st = pose_slot(state, slot, depth);
    const float* ra = st.row + (size_t)sh_a[sl] * dp::ROW;
    const float* rb = st.row + (size_t)sh_b[sl] * dp::ROW;
    pose_part(sh_f[sl], ra, ra + 3, rb, rb + 3, sh_u[sl], part, q_out + (size_t)slot * dp::ROW,
              quat_out ? quat_out + (size_t)slot * dp::QUAT : nullptr);
}

// blockIdx.x: a list entry (slots given) or a slot (slots null); 64 threads zero the block's words.
__global__ __launch_bounds__(64) void pose_reset_kernel(void* state, int n, int depth, const int* __restrict__ slots) {
    const int slot = slots ? slots[blockIdx.x] : (int)blockIdx.x;
    if (slot < 0 || slot >= n) return;
    const PoseSlot st = pose_slot(state, slot, depth);
    const size_t words = dp::slot_bytes(depth) / 4;              // the ring too: a reset block has one bit pattern
    for (size_t w = threadIdx.x; w < words; w += 64) reinterpret_cast<unsigned*>(st.hdr)[w] = 0u;
}

__global__ __launch_bounds__(64) void pose_get_kernel(const void* state, int n, int depth, const int* __restrict__ slots, int count,
                                                      int* __restrict__ out) {
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= count) return;
    const int slot = slots[j];
    if (slot < 0 || slot >= n) return;
    const PoseSlot st = pose_slot(const_cast<void*>(state), slot, depth);
    out[3 * (size_t)j] = st.hdr[1], out[3 * (size_t)j + 1] = st.hdr[3], out[3 * (size_t)j + 2] = st.hdr[2];
}

// ---- recorded tracks ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(dp::THREADS) void pose_rows_kernel(const double* __restrict__ stamps, const float* __restrict__ root,
                                                                const float* __restrict__ rows, int ld,
                                                                const long long* __restrict__ in_off, long long N_in,
                                                                const double* __restrict__ t_out, const long long* __restrict__ out_off,
                                                                long long N_out, int R, double delay, double max_hold, double max_predict,
                                                                int baseline, int mode, int depth, float* __restrict__ q_out,
                                                                float* __restrict__ quat_out, unsigned char* __restrict__ flags) {
    __shared__ double sh_u[dp::TILE];
    __shared__ long long sh_a[dp::TILE], sh_b[dp::TILE];
    __shared__ int sh_f[dp::TILE];
    const int sl = threadIdx.x / dp::PARTS, part = threadIdx.x - sl * dp::PARTS;
    const long long row = (long long)blockIdx.x * dp::TILE + sl;
    const bool live = row < N_out;
    if (live && part == 0) {
        int lo = 0, hi = R;                                      // the last j with out_off[j] <= row
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (out_off[mid] <= row) lo = mid;
            else hi = mid;
        }
        int f = rs::F_EMPTY, ia = 0, ib = 0;
        double u = 0.0;
        long long first = 0;
        if (!(R < 1 || row < out_off[lo] || row >= out_off[lo + 1])) {   // (else: a row no sequence owns)
            const long long b0 = clamp_ll(in_off[lo], 0, N_in), b1 = clamp_ll(in_off[lo + 1], b0, N_in);
            const double tk = t_out[row];
            long long c0 = 0, c1 = b1 - b0;                      // the entries not after the time: stamps[b0 + c] <= tk for c < c0
            while (c0 < c1) {
                const long long mid = (c0 + c1) >> 1;
                if (stamps[b0 + mid] <= tk) c0 = mid + 1;
                else c1 = mid;
            }
            const int cnt = c0 < depth ? (int)c0 : depth;        // of these the last `depth`
            first = b0 + c0 - cnt;
            f = pose_decide([&](int j) { return stamps[first + j]; }, cnt, tk - delay, max_hold, max_predict, baseline, mode, ia, ib, u);
        }
        sh_f[sl] = f, sh_a[sl] = first + ia, sh_b[sl] = first + ib, sh_u[sl] = u;
        flags[row] = (unsigned char)f;
    }
    __syncthreads();                                             // every thread of the workgroup arrives: nothing returned above
    if (!live) return;
    const long long ia = sh_a[sl], ib = sh_b[sl];                // (read only where the flag says there is an entry)
    pose_part(sh_f[sl], root + ia * 3, rows + ia * ld, root + ib * 3, rows + ib * ld, sh_u[sl], part, q_out + row * dp::ROW,
              quat_out ? quat_out + row * dp::QUAT : nullptr);
}

}  // namespace tip

using namespace tip;

extern "C" {

static bool dp_bad_n(long long n) { return n < 0 || n > (1ll << 24); }
static bool dp_bad_rows(long long n) { return n < 0 || n > (1ll << 40); }
static bool dp_bad_depth(int depth) { return depth < rs::MIN_DEPTH || depth > rs::MAX_DEPTH; }
static bool dp_bad_state(const void* state) { return !state || reinterpret_cast<uintptr_t>(state) % 8; }
// delay, max_predict: finite and >= 0; max_hold: < 0 for no limit, never NaN; baseline: 1 .. depth - 1; mode: HOLD, SLERP or PREDICT
static bool dp_bad_rule(double delay, double max_hold, double max_predict, int baseline, int mode, int depth) {
    return !(delay >= 0.0) || !__builtin_isfinite(delay) || max_hold != max_hold || !(max_predict >= 0.0) || !__builtin_isfinite(max_predict) ||
           baseline < 1 || baseline > depth - 1 || (mode != dp::HOLD && mode != dp::SLERP && mode != dp::PREDICT);
}

int tip_pose_tile(int* slots) {
    if (!slots) return TIP_ERR_INVALID_ARG;
    *slots = dp::TILE;
    return TIP_OK;
}

int tip_pose_state_bytes(int n_slots, int depth, size_t* bytes) {
    if (!bytes || dp_bad_n(n_slots) || dp_bad_depth(depth)) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)n_slots * dp::slot_bytes(depth);
    return TIP_OK;
}

int tip_pose_reset(void* state, int n_slots, int depth, const int* slots, int count, tip_stream_t stream) {
    if (dp_bad_state(state) || dp_bad_n(n_slots) || dp_bad_depth(depth) || count < 0) return TIP_ERR_INVALID_ARG;
    const int blocks = slots ? count : n_slots;
    if (blocks == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(pose_reset_kernel, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), state, n_slots, depth, slots);
    return tip_launch_status();
}

int tip_pose_get(const void* state, int n_slots, int depth, const int* slots, int count, int* counts_out, tip_stream_t stream) {
    if (dp_bad_state(state) || dp_bad_n(n_slots) || dp_bad_depth(depth) || count < 0 || (count > 0 && (!slots || !counts_out)))
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(pose_get_kernel, dim3((count + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), state, n_slots, depth, slots,
                       count, counts_out);
    return tip_launch_status();
}

int tip_pose_push(void* state, int n_slots, int depth, const int* slots, int count, const float* root, const float* s_rest, int ld,
                  const unsigned char* valid, const double* t, tip_stream_t stream) {
    if (dp_bad_state(state) || dp_bad_n(n_slots) || dp_bad_depth(depth) || count < 0 || ld < dp::MIN_LD || !root || !s_rest || !t ||
        reinterpret_cast<uintptr_t>(t) % 8)
        return TIP_ERR_INVALID_ARG;
    const int blocks = slots ? count : n_slots;
    if (blocks == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(pose_push_kernel, dim3(blocks), dim3(64), 0, static_cast<hipStream_t>(stream), state, n_slots, depth, slots, root,
                       s_rest, ld, valid, t);
    return tip_launch_status();
}

int tip_pose_emit(void* state, int n_slots, int depth, const double* t, double delay, double max_hold, double max_predict, int baseline,
                  int mode, float* q_out, float* quat_out, unsigned char* flags, tip_stream_t stream) {
    if (dp_bad_state(state) || dp_bad_n(n_slots) || dp_bad_depth(depth) || !t || reinterpret_cast<uintptr_t>(t) % 8 || !q_out || !flags ||
        dp_bad_rule(delay, max_hold, max_predict, baseline, mode, depth))
        return TIP_ERR_INVALID_ARG;
    if (n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(pose_emit_kernel, dim3((n_slots + dp::TILE - 1) / dp::TILE), dim3(dp::THREADS), 0, static_cast<hipStream_t>(stream),
                       state, n_slots, depth, t, delay, max_hold, max_predict, baseline, mode, q_out, quat_out, flags);
    return tip_launch_status();
}

int tip_pose_rows(const double* stamps, const float* root, const float* rows, int ld, const long long* in_offsets, long long n_in,
                  const double* t_out, const long long* out_offsets, long long n_out, int n_seq, double delay, double max_hold,
                  double max_predict, int baseline, int mode, int depth, float* q_out, float* quat_out, unsigned char* flags,
                  tip_stream_t stream) {
    if (dp_bad_rows(n_in) || dp_bad_rows(n_out) || dp_bad_n(n_seq) || dp_bad_depth(depth) || ld < dp::MIN_LD ||
        dp_bad_rule(delay, max_hold, max_predict, baseline, mode, depth) || !in_offsets || !out_offsets ||
        (n_in > 0 && (!stamps || !root || !rows)) || (n_out > 0 && (!t_out || !q_out || !flags)) ||
        reinterpret_cast<uintptr_t>(stamps) % 8 || reinterpret_cast<uintptr_t>(t_out) % 8)
        return TIP_ERR_INVALID_ARG;
    if (n_out == 0) return TIP_OK;
    const long long blocks = (n_out + dp::TILE - 1) / dp::TILE;
    if (blocks > 0x7fffffffll) return TIP_ERR_INVALID_ARG;
    hipLaunchKernelGGL(pose_rows_kernel, dim3((unsigned)blocks), dim3(dp::THREADS), 0, static_cast<hipStream_t>(stream), stamps, root, rows,
                       ld, in_offsets, n_in, t_out, out_offsets, n_out, n_seq, delay, max_hold, max_predict, baseline, mode, depth, q_out,
                       quat_out, flags);
    return tip_launch_status();
}

}  // extern "C"
