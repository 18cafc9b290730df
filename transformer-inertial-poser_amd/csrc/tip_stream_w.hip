// tip_stream_w.hip — the streaming front/back-end of tip_stream.hip at ANY window length W = 1 .. 128: the reference's
// RTRunnerMin(char, model, max_input_l = W, ...) / RTRunner (real_time_runner_minimal.py:24,54,131,139; real_time_runner.py:29,413,421).
// The _w entry points of include/tip_hip.h live here.  window = 40 IS tip_stream.hip (same kernels, same layout: the _w entry points
// hand the call over); every other length runs the kernels below, which take W as a value where the 40-row bodies have compile-time
// trip counts — the same arithmetic in the same order, restated (a kernel of tip_stream.hip that shares a body with one of these
// is no longer the kernel it was: its schedule changes), in a translation unit of their own for the same reason.
//
// What W changes (nothing else does): the call for frame f has T = min(max(f - 4, 0), W) rows; the local-frame, acc-sum and history
// rings are W deep (ring index j % W, j >= 0 throughout); the raw ring (11) and the output filter (6) are not.  The acc-sum feature
// still spans ACC_SUM_WIN_LEN = 40 rows (constants.py:17, :136): the newest min(T, 40) rows of the window, oldest first and this
// frame's row last; older rows of a longer window keep the value the acc-sum ring holds for them.
// W = 1: every ring has one slot.  The history slot is read by ingest k (entry k) and rewritten by consume k (entry k + 1), the
// local-frame slot is written by ingest k and read by consume k: stream order keeps both, as at every other length.
//
// State per stream (floats): frame counter | attached flag | shape word (ints) | raw[11][72] | loc[W][72] | accs[W][18] | hist[W][131] |
// outs[6][131] | last[54], padded to a multiple of 64 — the parts of the 40-row block with the three control words in FRONT: block 0's
// then sit at offset 0 of the buffer whatever W is, so a kernel that was handed another W than the buffer's reset finds the recorded
// length (and the shape) without leaving the buffer.  Shape word: (WTAG << 16) | (W << 2) | shape; in a 40-row buffer bits 2 and up
// are 0, what tip_stream_reset(_shaped) has always written.
// Layout guard (stream_check): a kernel whose W is not the buffer's touches no state; an ingest answers with NaN windows (and rows = -1),
// consume / attach / detach / override skip the block — NaN, never numbers read at another layout's offsets.  From a buffer no _w reset
// ever wrote, the shape is unknown and the NaNs go to windows of the narrowest shape (119 / 72 columns: inside every caller's buffers).
#include "tip_stream.h"

namespace tip {

namespace sz {
constexpr int WIN_MAX = 128;      // the longest window served (the training step's T limit)
constexpr int ACC_SUM_WIN = 40;   // ACC_SUM_WIN_LEN
constexpr int WTAG = 0x5457;      // bits 16-30 of the shape word
}  // namespace sz

struct StreamLay { int win, raw, loc, accs, hist, outs, last, stride; };   // the control words are floats 0 .. 2
__host__ __device__ constexpr StreamLay stream_lay(int W) {
    const int raw = 3, loc = raw + sz::RAWN * sz::NIMU, accs = loc + W * sz::NIMU, hist = accs + W * 18, outs = hist + W * sz::NS;
    const int last = outs + sz::OUTN * sz::NS;
    return {W, raw, loc, accs, hist, outs, last, (last + 54 + 63) / 64 * 64};
}
static_assert(stream_lay(sz::WIN).stride == sz::STRIDE, "a 40-row block is as large under either layout");

__host__ __device__ __forceinline__ int window_len_w(int frame_idx, int W) {   // T of the model call issued for frame `frame_idx`
    if (frame_idx < 5) return 0;
    const int t = frame_idx - 4;
    return t < W ? t : W;
}

struct StreamCheck { bool ok; int shape; };
// S: the workgroup's own block under L
__device__ __forceinline__ StreamCheck stream_check(const float* __restrict__ state, const float* __restrict__ S, const StreamLay L) {
    const int w0 = reinterpret_cast<const int*>(state)[2];   // block 0's shape word
    const bool tagged = (w0 >> 16) == sz::WTAG, ok0 = tagged && ((w0 >> 2) & 0x3fff) == L.win;
    // (this block's own word only once block 0 has confirmed the stride that leads to it)
    return {ok0 && reinterpret_cast<const int*>(S)[2] == w0, tagged ? (w0 & 3) : 3};
}

// ---- reset / attach (tip_stream.hip: stream_reset_kernel).  An attach to a buffer of another layout does nothing. ------------------
__global__ __launch_bounds__(64) void stream_reset_w_kernel(float* __restrict__ state, const float* __restrict__ s_init, int B,
                                                            const int* __restrict__ slots, int shape, int W) {
    const StreamLay L = stream_lay(W);
    const int tid = threadIdx.x;
    const int b = slots ? slots[blockIdx.x] : (int)blockIdx.x;
    if (b < 0 || b >= B) return;
    float* S = state + (size_t)b * L.stride;
    int* words = reinterpret_cast<int*>(S);
    if (slots) {
        if (!stream_check(state, S, L).ok) return;
        shape = words[2] & 3;
    }
    // (the shape word is written, never cleared: the other blocks of an attach are reading block 0's)
    for (int i = tid + 3; i < L.stride; i += 64) S[i] = 0.f;
    if (tid == 0) {
        words[0] = slots ? -1 : 0;   // "last ingested frame": an attached slot's next one is its frame 0
        words[1] = slots ? 1 : 0;
        words[2] = (sz::WTAG << 16) | (W << 2) | shape;
    }
    __syncthreads();
    const float* si = s_init + (size_t)blockIdx.x * 114;
    if (tid < 18) {
        float rv[3] = {si[3 + tid * 3], si[4 + tid * 3], si[5 + tid * 3]}, o[6];
        rotvec_to_6d(rv, o);
        for (int e = 0; e < 6; ++e) S[L.hist + tid * 6 + e] = o[e];
    }
    if (tid < 3) S[L.hist + 108 + tid] = si[57 + tid];
}

__global__ __launch_bounds__(64) void stream_detach_w_kernel(float* __restrict__ state, int B, const int* __restrict__ slots, int count,
                                                             int W) {
    const StreamLay L = stream_lay(W);
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const int b = slots[i];
    if (b < 0 || b >= B) return;
    float* S = state + (size_t)b * L.stride;
    if (!stream_check(state, S, L).ok) return;
    reinterpret_cast<int*>(S)[1] = 0;
}

// ---- ingest (tip_stream.hip: stream_ingest_body).  The window gather is plain strided loops. ---------------------------------------
template <int NS_, int NX_>
__device__ __forceinline__ void stream_ingest_body_w(float* __restrict__ sm, float* __restrict__ loc, float* __restrict__ S, int b,
                                                     bool listed, bool ok, const float* __restrict__ raw_in, int f,
                                                     float* __restrict__ x_imu, float* __restrict__ x_s, int T,
                                                     int* __restrict__ rows_out, const StreamLay L) {
    using namespace sz;
    constexpr int NS = NS_, NX = NX_;      // this shape's widths (they hide sz::NS / sz::NX, the widest shape's)
    constexpr bool ACC = NX_ > NIMU;
    const int p = blockIdx.x, tid = threadIdx.x, W = L.win;
    const int ldw = rows_out ? W : T;      // rows between two windows of x_imu / x_s
    float* xs = x_s + (size_t)p * ldw * NS;
    float* xi = x_imu + (size_t)p * ldw * NX;
    if (!ok) {   // another layout's buffer: NaN, and nothing of it is touched
        const float nan = __int_as_float(0x7fc00000);
        for (int i = tid; i < ldw * NS; i += 256) xs[i] = nan;
        for (int i = tid; i < ldw * NX; i += 256) xi[i] = nan;
        if (rows_out && tid == 0) rows_out[p] = -1;
        return;
    }
    int* words = reinterpret_cast<int*>(S);
    if (rows_out) {
        const bool attached = listed && words[1] != 0;
        f = attached ? words[0] + 1 : 0;
        __syncthreads();   // every thread reads before thread 0 writes
        T = attached ? window_len_w(f, W) : 0;
        for (int i = T * NS + tid; i < W * NS; i += 256) xs[i] = 0.f;
        for (int i = T * NX + tid; i < W * NX; i += 256) xi[i] = 0.f;
        if (tid == 0) rows_out[p] = T - 1;
        if (!attached) return;
    } else if (f < 0) {   // TIP_STREAM_FRAME_AUTO: the frame after the last one ingested (every thread reads before thread 0 writes)
        f = words[0] + 1;
        __syncthreads();
    }
    if (tid == 0) words[0] = f;
    const int k = f - 5;  // index of the smoothed frame produced now == index of this model call (f >= 5)
    float acc_old = 0.f;  // threads < 18: acc-sum over the older rows it spans, oldest first (:136)
    if (f >= 5) {
        for (int i = tid; i < T * NS; i += 256) {
            const int t = i / NS, c = i - t * NS, j = k + 1 - T + t;   // history entries k+1-T .. k (:144)
            xs[i] = S[L.hist + (j % W) * NS + c];
        }
        for (int i = tid; i < (T - 1) * NX; i += 256) {
            const int t = i / NX, c = i - t * NX, j = k - T + 1 + t;
            if (ACC && c >= NIMU)
                xi[i] = S[L.accs + (j % W) * 18 + (c - NIMU)] / 15.0f;   // :139-141
            else
                xi[i] = S[L.loc + (j % W) * NIMU + c];
        }
        if (ACC && tid < 18) {
            const int older = (T < ACC_SUM_WIN ? T : ACC_SUM_WIN) - 1;
            for (int j = k - older; j < k; ++j) acc_old += S[L.loc + (j % W) * NIMU + 54 + tid];
        }
    }
    // the smoothing chain, as in tip_stream.hip
    float vnew = 0.f;
    if (tid < NIMU) {
        vnew = raw_in[(size_t)b * NIMU + tid];
        if (f == 0) {
            for (int e = 0; e < 6; ++e) S[L.raw + e * NIMU + tid] = vnew;   // 5 priming copies + the frame itself (:61-66)
        } else {
            S[L.raw + ((f + 5) % RAWN) * NIMU + tid] = vnew;
        }
    }
    if (f < 5) return;   // fewer than 11 raw entries: the smoother is still priming (:68, :125-128)
    if (tid < 54) {
        sm[tid] = S[L.raw + (f % RAWN) * NIMU + tid];            // rotations of the frame 5 steps back (:71)
    } else if (tid < NIMU) {
        float acc = 0.f;
        for (int i = 0; i < RAWN - 1; ++i) acc += S[L.raw + ((f - 5 + i) % RAWN) * NIMU + tid];   // oldest -> newest (:72) ...
        acc += vnew;                                                                               // ... the newest is this call's frame
        sm[tid] = acc / (float)RAWN;
    }
    __syncthreads();
    if (tid < NIMU) {
        // general 3x3 inverse (np.linalg.inv at data_utils.py:200,211), adjugate / determinant
        float inv[9];
        {
            const float a = sm[0], bq = sm[1], c = sm[2], d = sm[3], e = sm[4], g = sm[5], h = sm[6], i9 = sm[7], j = sm[8];
            const float A = e * j - g * i9, Bc = -(d * j - g * h), Cc = d * i9 - e * h;
            const float det = a * A + bq * Bc + c * Cc;
            const float id = 1.f / det;
            inv[0] = A * id;  inv[1] = -(bq * j - c * i9) * id; inv[2] = (bq * g - c * e) * id;
            inv[3] = Bc * id; inv[4] = (a * j - c * h) * id;    inv[5] = -(a * g - c * d) * id;
            inv[6] = Cc * id; inv[7] = -(a * i9 - bq * h) * id; inv[8] = (a * e - bq * d) * id;
        }
        float lv;
        if (tid < 9) {
            lv = sm[tid];
        } else if (tid < 54) {
            const int s = (tid - 9) / 9, e = (tid - 9) % 9, i = e / 3, j = e % 3;
            const float* Rm = sm + 9 + s * 9;
            lv = inv[i * 3 + 0] * Rm[0 * 3 + j] + inv[i * 3 + 1] * Rm[1 * 3 + j] + inv[i * 3 + 2] * Rm[2 * 3 + j];
        } else if (tid < 57) {
            lv = sm[tid];
        } else {
            const int s = (tid - 57) / 3, i = (tid - 57) % 3;
            const float* am = sm + 57 + s * 3;
            lv = inv[i * 3 + 0] * am[0] + inv[i * 3 + 1] * am[1] + inv[i * 3 + 2] * am[2];
        }
        loc[tid] = lv;
    }
    __syncthreads();
    // this frame's row: to the state (next frames read it) and straight to the newest row of x_imu, both from LDS
    float* xin = xi + (size_t)(T - 1) * NX;
    if (tid < NIMU) {
        S[L.loc + (k % W) * NIMU + tid] = loc[tid];
        xin[tid] = loc[tid];
    }
    if (ACC && tid < 18) {   // the older rows' partial + this frame, added last (:136)
        const float acc = acc_old + loc[54 + tid];
        S[L.accs + (k % W) * 18 + tid] = acc;
        xin[NIMU + tid] = acc / 15.0f;                        // :139-141
    }
}

// f, T: the lock-step call's frame index and window length (the staggered and mapped calls keep both per slot); rows_out, slot_at:
// as stream_ingest_kernel's
__global__ __launch_bounds__(256) void stream_ingest_w_kernel(float* __restrict__ state, const float* __restrict__ raw_in, int n,
                                                              int f, float* __restrict__ x_imu, float* __restrict__ x_s, int T,
                                                              int* __restrict__ rows_out, const int* __restrict__ slot_at, int W) {
    __shared__ float sm[sz::NIMU], loc[sz::NIMU];
    const StreamLay L = stream_lay(W);
    const int b = slot_at ? slot_at[blockIdx.x] : (int)blockIdx.x;
    const bool listed = b >= 0 && b < n;
    float* S = state + (size_t)(listed ? b : 0) * L.stride;
    const StreamCheck c = stream_check(state, S, L);
    if (c.shape == 0) {
        stream_ingest_body_w<sz::NS, sz::NX>(sm, loc, S, b, listed, c.ok, raw_in, f, x_imu, x_s, T, rows_out, L);
    } else if (c.shape == 1) {
        stream_ingest_body_w<sz::NS2, sz::NX>(sm, loc, S, b, listed, c.ok, raw_in, f, x_imu, x_s, T, rows_out, L);
    } else if (c.shape == 2) {
        stream_ingest_body_w<sz::NS, sz::NIMU>(sm, loc, S, b, listed, c.ok, raw_in, f, x_imu, x_s, T, rows_out, L);
    } else {
        stream_ingest_body_w<sz::NS2, sz::NIMU>(sm, loc, S, b, listed, c.ok, raw_in, f, x_imu, x_s, T, rows_out, L);
    }
}

// ---- consume (tip_stream.hip: stream_consume_kernel; rows, slot_at, y_slot, rows_slot as there) -----------------------------------
template <int NS_>
__device__ __forceinline__ void stream_consume_filter_w(float* __restrict__ s, float* __restrict__ O, const float* __restrict__ y_row,
                                                        float* __restrict__ c_row, int k, int tid) {
    using namespace sz;
    constexpr int NS = NS_;
    const float coeff[OUTN] = {0.07776f, 0.1296f, 0.216f, 0.36f, 0.6f, 1.0f};   // 0.6^(5..0) (:57)
    const float csum = 0.07776f + 0.1296f + 0.216f + 0.36f + 0.6f + 1.0f;
    const int n = k + 1;
    if (tid < NS) {   // O: the block's output ring
        const float y = y_row[tid];
        O[(k % OUTN) * NS + tid] = y;
        float v;
        if (n >= OUTN) {
            float acc = 0.f;
            for (int i = 0; i < OUTN - 1; ++i) acc += O[((k - 5 + i) % OUTN) * NS + tid] * coeff[i];
            acc += y * coeff[OUTN - 1];
            v = acc / csum;
        } else {
            v = y;
        }
        if (tid >= 111) {
            const int ci = tid - 111;
            v = (ci & 3) == 0 ? (v > 0.f ? 1.f : 0.f) : v / 5.0f;      // :107-110
            // reference quirk: with fewer than 6 buffered rows the decode happens IN PLACE in the buffered row (:99)
            if (n < OUTN) O[(k % OUTN) * NS + tid] = v;
            c_row[ci] = v;
        }
        s[tid] = v;
    }
}

__global__ __launch_bounds__(192) void stream_consume_w_kernel(float* __restrict__ state, const float* __restrict__ y_last, int n_slots,
                                                               int k, float* __restrict__ s_rest, float* __restrict__ c_out,
                                                               const int* __restrict__ rows, const int* __restrict__ slot_at,
                                                               float* __restrict__ y_slot, int* __restrict__ rows_slot, int W) {
    using namespace sz;
    __shared__ float s[NS], aa[54], rootv[3];
    const StreamLay L = stream_lay(W);
    const int p = blockIdx.x, tid = threadIdx.x;
    const int b = slot_at ? slot_at[p] : p;
    if (slot_at && (b < 0 || b >= n_slots)) return;
    float* S = state + (size_t)b * L.stride;
    const StreamCheck chk = stream_check(state, S, L);
    if (!chk.ok) return;
    const int row = rows ? rows[p] : 0;
    const int ns = (chk.shape & 1) ? NS2 : NS;   // this buffer's state width; ns - 111 SBP columns (20 / 8)
    if (slot_at) {
        if (y_slot && tid < ns) y_slot[(size_t)b * ns + tid] = y_last[(size_t)p * ns + tid];
        if (rows_slot && tid == 0) rows_slot[b] = row;
    }
    if (row < 0) return;
    if (k < 0) k = reinterpret_cast<const int*>(S)[0] - 5;   // TIP_STREAM_FRAME_AUTO: the call that belongs to the last ingested frame
    float last3[3] = {0.f, 0.f, 0.f}, rr[9];
    if (tid >= 1 && tid < 18 && k > 0)
        for (int e = 0; e < 3; ++e) last3[e] = S[L.last + (tid - 1) * 3 + e];
    if (tid >= 64 && tid < 67 && k > 0) last3[0] = S[L.last + 51 + (tid - 64)];
    if (tid == 0)
        for (int e = 0; e < 9; ++e) rr[e] = S[L.loc + (k % W) * NIMU + e];
    if (ns == NS)
        stream_consume_filter_w<NS>(s, S + L.outs, y_last + (size_t)p * NS, c_out + (size_t)b * (NS - 111), k, tid);
    else
        stream_consume_filter_w<NS2>(s, S + L.outs, y_last + (size_t)p * NS2, c_out + (size_t)b * (NS2 - 111), k, tid);
    __syncthreads();
    float* hrow = S + L.hist + ((k + 1) % W) * ns;   // the history row this call feeds back
    if (tid < 18) {
        float rv[3];
        if (tid == 0) {   // root rotation comes from the IMU, not from the prediction (:160-162)
            float m[3][3] = {{rr[0], rr[1], rr[2]}, {rr[3], rr[4], rr[5]}, {rr[6], rr[7], rr[8]}};
            polar_newton(m);
            float q[4];
            mat_to_quat(m, q);
            quat_to_rotvec(q, rv);
        } else {          // 6D -> rotation (columns normalised with +1e-6, third by cross product; data_utils.py:171-176)
            const float* c6 = s + tid * 6;
            float a1[3] = {c6[0], c6[2], c6[4]}, a2[3] = {c6[1], c6[3], c6[5]};
            const float n1 = sqrtf(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]) + 1e-6f;
            const float n2 = sqrtf(a2[0] * a2[0] + a2[1] * a2[1] + a2[2] * a2[2]) + 1e-6f;
            for (int e = 0; e < 3; ++e) { a1[e] /= n1; a2[e] /= n2; }
            float m[3][3];
            polar_two_axis(a1, a2, m);
            float q[4];
            mat_to_quat(m, q);
            quat_to_rotvec(q, rv);
            if (k > 0) {  // averaged with the previous pose (:165-166)
                for (int e = 0; e < 3; ++e) rv[e] = (rv[e] + last3[e]) * 0.5f;
            }
            for (int e = 0; e < 3; ++e) S[L.last + (tid - 1) * 3 + e] = rv[e];
        }
        for (int e = 0; e < 3; ++e) aa[tid * 3 + e] = rv[e];
        float o6[6];
        rotvec_to_6d(rv, o6);   // :78-85
        for (int e = 0; e < 6; ++e) hrow[tid * 6 + e] = o6[e];
    } else if (tid >= 64 && tid < 67) {
        const int e = tid - 64;
        float v = s[108 + e];
        if (k > 0) v = (v + last3[0]) * 0.5f;
        S[L.last + 51 + e] = v;
        rootv[e] = v;
        hrow[108 + e] = v;
    } else if (tid >= 128 && tid < 128 + ns - 111) {
        hrow[111 + (tid - 128)] = s[111 + (tid - 128)];
    }
    __syncthreads();
    // s_t[3:114]: 54 axis-angles, root velocity, 54 zeros
    if (tid < 111) s_rest[(size_t)b * 111 + tid] = tid < 54 ? aa[tid] : (tid < 57 ? rootv[tid - 54] : 0.f);
}

// ---- host override of the fed-back pose (tip_stream.hip: stream_history_override_kernel) -------------------------------------------
__global__ __launch_bounds__(64) void stream_history_override_w_kernel(float* __restrict__ state, int B, const int* __restrict__ slots,
                                                                       const float* __restrict__ q_aa, int W) {
    using namespace sz;
    const StreamLay L = stream_lay(W);
    const int j = blockIdx.x, tid = threadIdx.x;
    const int b = slots[j];
    if (b < 0 || b >= B) return;
    float* S = state + (size_t)b * L.stride;
    const StreamCheck chk = stream_check(state, S, L);
    if (!chk.ok) return;
    const int ns = (chk.shape & 1) ? NS2 : NS;
    const int k = reinterpret_cast<const int*>(S)[0] - 5;
    if (k < 0 || tid >= 18) return;
    const float* q = q_aa + (size_t)j * 54 + tid * 3;
    const float rv[3] = {q[0], q[1], q[2]};
    float o6[6];
    rotvec_to_6d(rv, o6);
    for (int e = 0; e < 6; ++e) S[L.hist + ((k + 1) % W) * ns + tid * 6 + e] = o6[e];
}

}  // namespace tip

using namespace tip;

static bool bad_window(int window) { return window < 1 || window > sz::WIN_MAX; }

extern "C" {

int tip_stream_state_bytes_w(int n_streams, int window, size_t* bytes) {
    if (bad_window(window) || n_streams < 0 || !bytes) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)n_streams * stream_lay(window).stride * sizeof(float);
    return TIP_OK;
}

int tip_stream_window_len_w(int frame_idx, int window) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    return window_len_w(frame_idx, window);
}

int tip_stream_reset_w(void* state, const float* s_init, int n_streams, int n_sbps, int with_acc_sum, int window, tip_stream_t stream) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    if (window == sz::WIN) return tip_stream_reset_shaped(state, s_init, n_streams, n_sbps, with_acc_sum, stream);
    if (!state || !s_init || n_streams < 0 || (n_sbps != 2 && n_sbps != 5)) return TIP_ERR_INVALID_ARG;
    if (n_streams == 0) return TIP_OK;
    const int shape = (n_sbps == 2 ? 1 : 0) | (with_acc_sum ? 0 : 2);
    hipLaunchKernelGGL(stream_reset_w_kernel, dim3(n_streams), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(state), s_init, n_streams, nullptr, shape, window);
    return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_stream_history_override_w(void* state, int n_streams, const int* slots, const float* q_aa, int count, int window,
                                  tip_stream_t stream) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    if (window == sz::WIN) return tip_stream_history_override(state, n_streams, slots, q_aa, count, stream);
    if (!state || n_streams < 0 || count < 0 || (count > 0 && (!slots || !q_aa))) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_streams == 0) return TIP_OK;
    hipLaunchKernelGGL(stream_history_override_w_kernel, dim3(count), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(state), n_streams, slots, q_aa, window);
    return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_stream_ingest_w(void* state, const float* raw_imu, int n_streams, int frame_idx, float* x_imu, float* x_s, int window,
                        tip_stream_t stream) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    if (window == sz::WIN) return tip_stream_ingest(state, raw_imu, n_streams, frame_idx, x_imu, x_s, stream);
    if (!state || !raw_imu || n_streams < 0 || frame_idx < TIP_STREAM_FRAME_AUTO) return TIP_ERR_INVALID_ARG;
    const int T = frame_idx == TIP_STREAM_FRAME_AUTO ? window : window_len_w(frame_idx, window);
    if (T > 0 && (!x_imu || !x_s)) return TIP_ERR_INVALID_ARG;
    if (n_streams == 0) return TIP_OK;
    hipLaunchKernelGGL(stream_ingest_w_kernel, dim3(n_streams), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(state), raw_imu, n_streams, frame_idx, x_imu, x_s, T, nullptr, nullptr, window);
    return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_stream_consume_w(void* state, const float* y_last, int n_streams, int call_idx, float* s_rest, float* c_t, int window,
                         tip_stream_t stream) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    if (window == sz::WIN) return tip_stream_consume(state, y_last, n_streams, call_idx, s_rest, c_t, stream);
    if (!state || !y_last || !s_rest || !c_t || n_streams < 0 || call_idx < TIP_STREAM_FRAME_AUTO) return TIP_ERR_INVALID_ARG;
    if (n_streams == 0) return TIP_OK;
    hipLaunchKernelGGL(stream_consume_w_kernel, dim3(n_streams), dim3(192), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(state), y_last, n_streams, call_idx, s_rest, c_t, nullptr, nullptr, nullptr, nullptr, window);
    return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_stream_attach_w(void* state, int n_streams, const int* slots, const float* s_init, int count, int window, tip_stream_t stream) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    if (window == sz::WIN) return tip_stream_attach(state, n_streams, slots, s_init, count, stream);
    if (!state || n_streams < 0 || count < 0 || (count > 0 && (!slots || !s_init))) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_streams == 0) return TIP_OK;
    hipLaunchKernelGGL(stream_reset_w_kernel, dim3(count), dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<float*>(state),
                       s_init, n_streams, slots, 0, window);
    return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_stream_detach_w(void* state, int n_streams, const int* slots, int count, int window, tip_stream_t stream) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    if (window == sz::WIN) return tip_stream_detach(state, n_streams, slots, count, stream);
    if (!state || n_streams < 0 || count < 0 || (count > 0 && !slots)) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_streams == 0) return TIP_OK;
    hipLaunchKernelGGL(stream_detach_w_kernel, dim3((count + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(state), n_streams, slots, count, window);
    return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_stream_ingest_staggered_w(void* state, const float* raw_imu, int n_streams, float* x_imu, float* x_s, int* rows, int window,
                                  tip_stream_t stream) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    if (window == sz::WIN) return tip_stream_ingest_staggered(state, raw_imu, n_streams, x_imu, x_s, rows, stream);
    if (!state || !raw_imu || !x_imu || !x_s || !rows || n_streams < 0) return TIP_ERR_INVALID_ARG;
    if (n_streams == 0) return TIP_OK;
    hipLaunchKernelGGL(stream_ingest_w_kernel, dim3(n_streams), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(state), raw_imu, n_streams, 0, x_imu, x_s, window, rows, nullptr, window);
    return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_stream_consume_staggered_w(void* state, const float* y_last, const int* rows, int n_streams, float* s_rest, float* c_t,
                                   int window, tip_stream_t stream) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    if (window == sz::WIN) return tip_stream_consume_staggered(state, y_last, rows, n_streams, s_rest, c_t, stream);
    if (!state || !y_last || !rows || !s_rest || !c_t || n_streams < 0) return TIP_ERR_INVALID_ARG;
    if (n_streams == 0) return TIP_OK;
    hipLaunchKernelGGL(stream_consume_w_kernel, dim3(n_streams), dim3(192), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(state), y_last, n_streams, TIP_STREAM_FRAME_AUTO, s_rest, c_t, rows, nullptr, nullptr, nullptr,
                       window);
    return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_stream_ingest_mapped_w(void* state, const float* raw_imu, int n_streams, const int* slot_at, int B, float* x_imu, float* x_s,
                               int* rows, int window, tip_stream_t stream) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    if (window == sz::WIN) return tip_stream_ingest_mapped(state, raw_imu, n_streams, slot_at, B, x_imu, x_s, rows, stream);
    if (!state || !raw_imu || !slot_at || !x_imu || !x_s || !rows || n_streams < 0 || B < 0 || B > n_streams) return TIP_ERR_INVALID_ARG;
    if (B == 0) return TIP_OK;
    hipLaunchKernelGGL(stream_ingest_w_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(state), raw_imu, n_streams, 0, x_imu, x_s, window, rows, slot_at, window);
    return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

int tip_stream_consume_mapped_w(void* state, const float* y, const int* rows, const int* slot_at, int B, int n_streams, float* s_rest,
                                float* c_t, float* y_slot, int* rows_slot, int window, tip_stream_t stream) {
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    if (window == sz::WIN) return tip_stream_consume_mapped(state, y, rows, slot_at, B, n_streams, s_rest, c_t, y_slot, rows_slot, stream);
    if (!state || !y || !rows || !slot_at || !s_rest || !c_t || n_streams < 0 || B < 0 || B > n_streams) return TIP_ERR_INVALID_ARG;
    if (B == 0) return TIP_OK;
    hipLaunchKernelGGL(stream_consume_w_kernel, dim3(B), dim3(192), 0, static_cast<hipStream_t>(stream),
                       static_cast<float*>(state), y, n_streams, TIP_STREAM_FRAME_AUTO, s_rest, c_t, rows, slot_at, y_slot, rows_slot,
                       window);
    return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP;
}

}  // extern "C"
