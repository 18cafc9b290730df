// tip_stream.hip — on-device streaming front/back-end: the model-facing half of
// RTRunnerMin.step (/root/reference/real_time_runner_minimal.py) for B concurrent streams, so that a closed-loop
// frame costs ZERO host<->device round trips for the model inputs (the reference crosses PCIe twice per frame per
// stream at :146-150 and does ~7 ms of numpy per stream on the host).
//
//   stream_ingest_kernel   :59-76   raw-IMU ring (5-frame priming), 11-tap acceleration mean, rotations delayed 5
//                          :131-147 root-frame rotation of the 5 other IMUs (data_utils.py:190-219), acc-sum feature
//                                   over the <=40-frame window (/15, constants.py:17-18), window gather -> x_imu, x_s
//   stream_consume_kernel  :87-112  6-tap 0.6^k output filter (incl. the reference's in-place quirk on the first 5
//                                   rows), SBP flag threshold, offsets / 5
//                          :154-167 6D -> axis-angle (data_utils.py:164-179; scipy Rotation.from_matrix/as_rotvec
//                                   restated), root rotation from the IMU, averaging with the previous pose
//                          :78-85   axis-angle -> 6D history row (data_utils.py:182-187; from_rotvec/as_matrix)
// PyBullet FK and the SBP root-translation correction (:169-194) stay on the host, unchanged: they only touch the
// root translation, which is not a model input.
//
// State per stream (floats, caller-owned device buffer): raw[11][72] | loc[40][72] | accs[40][18] | hist[40][131] |
// outs[6][131] | last[54] | frame counter (int) | attached flag (int; the staggered entry points only, 0 = detached) | shape word
// (int).  Frame / call counters live on the host (all streams advance in lock step); the
// ingest kernel also leaves the frame index in the state, so that a call with TIP_STREAM_FRAME_AUTO continues from it — kernel
// arguments are frozen in a captured HIP graph, a counter in HBM is not.
//
// Shapes: the reference's runners serve four models — with or without the acc-sum feature (x_imu 90 / 72 columns; RTRunner(Min)'s
// with_acc_sum) times five or two stationary body points (state 131 / 119 columns, c_t 20 / 8; real_time_runner.py:39).  The
// smaller shapes live inside the same block at the same offsets (hist / outs rows are NS wide, accs is unused without acc-sum), so
// the block size does not depend on the shape.  The shape is ONE per state buffer: tip_stream_reset(_shaped) writes it into the
// shape word of every block (an attach keeps it), next to the frame counter and the attached flag — the three share a cache line, and
// a kernel asks for them together: read on its own, ahead of everything else, the word cost the one-stream frame 0.8 us per kernel.
// A workgroup reads its own block's word (block 0's for an empty position of a compact pool, which still zeroes a window of the
// right width) and branches once into its <NS, NX> body — the window loops have compile-time trip counts.  0 is (5 SBPs, acc-sum).
//
// Window length: the kernels of the first half are the paper's 40 rows; any other length (the runners' max_input_l; the _w entry
// points) runs the _w kernels of the second half, which take the length as a value.  The rule for what the two forms share: the 40-row
// ingest, consume, reset and detach kernels compile to the gfx950 instructions, registers and LDS they had as a file of their own
// (compared kernel by kernel on the device assembly); the _w kernels keep their output bits, not their schedule.
//   Shared (tip_stream.h, over a layout policy): the smoothing chain (stream_ingest_kernel unchanged: 50 664 bytes, 79 VGPRs); the
//   output filter (stream_consume_kernel unchanged: 14 036 bytes, 40 VGPRs); the 6D history row of a reset and of an override
//   (stream_reset_kernel unchanged; stream_history_override_kernel keeps its 2632 bytes and 23 VGPRs with the row index computed
//   earlier); the window length rule, as a function of the layout (of W as a value it changed the 40-row ingest: a signed minimum).
//   Not shared: the window gather (register-staged with compile-time trip counts here, strided loops there: two algorithms); the pose
//   half of a consume (as a function of the layout it changed stream_consume_kernel, 2506 -> 2499 instruction lines, and the _w
//   kernel is its only other user); the reset, detach and override prologues (control words in other places, and the layout
//   guard, which is any-length only).
#include "tip_stream.h"

namespace tip {

// ---- reset: history row 0 from s_init (:45, :78-85) ----------------------------------------------------------
// slots == nullptr: every stream b = blockIdx.x (tip_stream_reset: all detached).  Otherwise (tip_stream_attach) the block rebuilds
// stream slots[blockIdx.x] from s_init row blockIdx.x and marks it attached, its next staggered ingest being its frame 0.
// The shape word is set by the reset only (`shape`, the same in every block); an attach puts back what it found: a buffer has one
// shape from reset to reset.  History row 0 is 108 + 3 columns and zeros at every shape.
__global__ __launch_bounds__(64) void stream_reset_kernel(float* __restrict__ state, const float* __restrict__ s_init, int B,
                                                          const int* __restrict__ slots, int shape) {
    using namespace sz;
    const int tid = threadIdx.x;
    const int b = slots ? slots[blockIdx.x] : (int)blockIdx.x;
    if (b < 0 || b >= B) return;
    float* S = state + (size_t)b * STRIDE;
    if (slots) shape = reinterpret_cast<const int*>(S + SHP)[0];   // (one wave: read before its own zeroing below, put back after it)
    for (int i = tid; i < STRIDE; i += 64) S[i] = 0.f;
    __syncthreads();
    if (tid == 0) reinterpret_cast<int*>(S + SHP)[0] = shape;
    if (slots && tid == 0) {
        reinterpret_cast<int*>(S + CTR)[0] = -1;   // "last ingested frame": the next one is frame 0
        reinterpret_cast<int*>(S + ATT)[0] = 1;
    }
    const float* si = s_init + (size_t)blockIdx.x * 114;
    if (tid < 18) stream_hist_pose(S, HIST, si, 3, tid);
    if (tid < 3) S[HIST + 108 + tid] = si[57 + tid];
}

// ---- detach: the listed slots stop taking part in the staggered calls (their state is kept until the next attach) -----------
__global__ __launch_bounds__(64) void stream_detach_kernel(float* __restrict__ state, int B, const int* __restrict__ slots, int count) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const int b = slots[i];
    if (b < 0 || b >= B) return;
    reinterpret_cast<int*>(state + (size_t)b * sz::STRIDE + sz::ATT)[0] = 0;
}

// ---- ingest one raw frame per stream and emit the model inputs -----------------------------------------------
// newest != 0 (tip_stream_ingest_newest): only row T - 1 of every window is written — what the exact-reuse forward reads
// (tip_forward_reuse takes every older row from its ring).  At >= 1024 streams the window gather IS this kernel: 35 KB read and 35 KB
// written per stream, 18 us at 1024 streams and 53 us at 4096 against 8-9 us for the smoothing chain.
// rows_out != nullptr (tip_stream_ingest_staggered): every stream keeps its own frame counter and window length T_i, and its window
// sits in a 40-row slot: rows 0 .. T_i - 1 as the lock-step ingest writes them for frame f_i, rows T_i .. 39 zero, rows_out[b] = T_i - 1
// (-1 while priming).  A detached stream gets a zero window and -1, and its state is not touched.
// slot_at != nullptr (tip_stream_ingest_mapped, staggered only): block p builds window p (x_imu, x_s, rows_out by POSITION) for slot
// slot_at[p] (state, raw_in by SLOT); a position whose entry is outside [0, n) is empty: zero window, -1.  nullptr: slot = position.
template <int NS_, int NX_>
__device__ __forceinline__ void stream_ingest_body(float* __restrict__ sm, float* __restrict__ loc, float* __restrict__ S, int b,
                                                   bool listed, StreamWords w, const float* __restrict__ raw_in, int f,
                                                   float* __restrict__ x_imu, float* __restrict__ x_s, int T, int newest,
                                                   int* __restrict__ rows_out) {
    using namespace sz;
    constexpr int NS = NS_, NX = NX_;      // this shape's widths (they hide sz::NS / sz::NX, the widest shape's)
    constexpr bool ACC = NX_ > NIMU;       // the acc-sum feature: ring accs[40][18], columns 72-89
    const int p = blockIdx.x, tid = threadIdx.x;
    int* ctr = reinterpret_cast<int*>(S + CTR);
    int ldw = T;   // rows between two windows of x_imu / x_s
    if (rows_out) {
        const bool attached = listed && w.att != 0;
        f = attached ? w.ctr + 1 : 0;
        __syncthreads();   // every thread reads before thread 0 writes
        T = attached ? window_len(f, StreamLay40{}) : 0;
        ldw = WIN;
        float* xs0 = x_s + (size_t)p * WIN * NS;
        float* xi0 = x_imu + (size_t)p * WIN * NX;
        for (int i = T * NS + tid; i < WIN * NS; i += 256) xs0[i] = 0.f;
        for (int i = T * NX + tid; i < WIN * NX; i += 256) xi0[i] = 0.f;
        if (tid == 0) rows_out[p] = T - 1;
        if (!attached) return;
    } else if (f < 0) {   // TIP_STREAM_FRAME_AUTO: the frame after the last one ingested (every thread reads before thread 0 writes)
        f = w.ctr + 1;
        __syncthreads();
    }
    if (tid == 0) *ctr = f;
    // Everything that does not depend on THIS frame goes first, so that it runs under the latency of the smoothing chain below (five
    // dependent phases with a barrier and a global round trip each) instead of after it: the whole x_s window (history rows written by
    // earlier consume calls), rows 0 .. T-2 of x_imu (local-frame rows and acc-sums of earlier frames) and the acc-sum of the older
    // frames.  As one tail behind the chain these copies were two thirds of the kernel's 13 us at one stream.
    const int k = f - 5;  // index of the smoothed frame produced now == index of this model call (f >= 5)
    float acc_old = 0.f;  // threads < 18: acc-sum over the window's older frames, oldest first (:136)
    if (f >= 5) {
        // (compile-time trip counts, every load of a loop requested before its first store: 36 round trips in flight together)
        constexpr int XS_IT = (WIN * NS + 255) / 256, XI_IT = (WIN * NX + 255) / 256;
        float* xs = x_s + (size_t)p * ldw * NS;
        float* xi = x_imu + (size_t)p * ldw * NX;
        if (newest) {
            if (tid < NS) xs[(T - 1) * NS + tid] = S[HIST + (k % WIN) * NS + tid];     // history entry k (:144)
        } else {
        float vs[XS_IT];
#pragma unroll
        for (int u = 0; u < XS_IT; ++u) {
            const int i = tid + 256 * u, ic = i < T * NS ? i : 0;
            const int t = ic / NS, c = ic - t * NS, j = k + 1 - T + t;   // history entries k+1-T .. k (:144)
            vs[u] = S[HIST + (j % WIN) * NS + c];
        }
        float vi[XI_IT];
#pragma unroll
        for (int u = 0; u < XI_IT; ++u) {
            const int i = tid + 256 * u, ic = i < (T - 1) * NX ? i : 0;
            const int t = ic / NX, c = ic - t * NX, j = k - T + 1 + t;
            if constexpr (ACC) {
                const float* pv = c < NIMU ? S + LOC + (j % WIN) * NIMU + c : S + ACCS + (j % WIN) * 18 + (c - NIMU);
                const float x = *pv;
                vi[u] = c < NIMU ? x : x / 15.0f;                                                        // :139-141
            } else {
                vi[u] = S[LOC + (j % WIN) * NIMU + c];
            }
        }
#pragma unroll
        for (int u = 0; u < XS_IT; ++u)
            if (tid + 256 * u < T * NS) xs[tid + 256 * u] = vs[u];
#pragma unroll
        for (int u = 0; u < XI_IT; ++u)
            if (tid + 256 * u < (T - 1) * NX) xi[tid + 256 * u] = vi[u];
        }
        if (ACC && tid < 18) {   // all (up to 39) loads first, then the sum in the reference's order: one round trip, not one per frame
            float av[WIN - 1];
#pragma unroll
            for (int u = 0; u < WIN - 1; ++u) {
                const int j = k - T + 1 + u;
                av[u] = S[LOC + ((j < k ? j : k - 1 < 0 ? 0 : k - 1) % WIN) * NIMU + 54 + tid];
            }
#pragma unroll
            for (int u = 0; u < WIN - 1; ++u)
                if (k - T + 1 + u < k) acc_old += av[u];
        }
    }
    stream_ingest_chain<NX>(sm, loc, S, b, raw_in, f, x_imu, ldw, T, acc_old, StreamLay40{});
}

__global__ __launch_bounds__(256) void stream_ingest_kernel(float* __restrict__ state, const float* __restrict__ raw_in, int n,
                                                            int f, float* __restrict__ x_imu, float* __restrict__ x_s, int T, int newest,
                                                            int* __restrict__ rows_out, const int* __restrict__ slot_at) {
    __shared__ float sm[sz::NIMU], loc[sz::NIMU];
    const int b = slot_at ? slot_at[blockIdx.x] : (int)blockIdx.x;
    const bool listed = b >= 0 && b < n;
    float* S = state + (size_t)(listed ? b : 0) * sz::STRIDE;
    const StreamWords w = stream_words(S);
    // The paper's shape is tested on its own and marked likely, so that its body follows the prologue in the code, where the
    // instruction fetch already is: as one four-way switch the compiler put it behind a 13-KB jump, one more instruction miss for a
    // cold one-stream launch.  (The empty asm keeps the second test from being merged with the first into that switch again.)
    if (__builtin_expect(w.shape == 0, 1)) {
        stream_ingest_body<sz::NS, sz::NX>(sm, loc, S, b, listed, w, raw_in, f, x_imu, x_s, T, newest, rows_out);
        return;
    }
    int other = w.shape;
    asm volatile("" : "+s"(other));
    if (other == 1) {
        stream_ingest_body<sz::NS2, sz::NX>(sm, loc, S, b, listed, w, raw_in, f, x_imu, x_s, T, newest, rows_out);
    } else if (other == 2) {
        stream_ingest_body<sz::NS, sz::NIMU>(sm, loc, S, b, listed, w, raw_in, f, x_imu, x_s, T, newest, rows_out);
    } else {
        stream_ingest_body<sz::NS2, sz::NIMU>(sm, loc, S, b, listed, w, raw_in, f, x_imu, x_s, T, newest, rows_out);
    }
}

// ---- consume the model's last row: filter, decode, pose assembly, history feedback ----------------------------
// rows != nullptr (tip_stream_consume_staggered): a stream with rows[b] < 0 is skipped (state and output rows untouched); the others
// consume their row as call f_b - 5 of their own counter
// slot_at != nullptr (tip_stream_consume_mapped): block p consumes y_last[p] / rows[p] (by POSITION) for slot slot_at[p] (state,
// s_rest, c_out by SLOT), after copying them to y_slot[slot] / rows_slot[slot] when given; an empty position (entry outside
// [0, n_slots)) does nothing.  nullptr: slot = position.
// The kernel is one body for every shape except its first phase (stream_consume_filter: the NS-wide row, its ring and the SBP
// columns, where the width is a compile-time constant); the pose half behind the first barrier takes the width as a value — it
// enters one address computation — so that its rotation code, whose small matrices the compiler keeps in LDS, exists once.
__global__ __launch_bounds__(192) void stream_consume_kernel(float* __restrict__ state, const float* __restrict__ y_last, int n_slots,
                                                             int k, float* __restrict__ s_rest, float* __restrict__ c_out,
                                                             const int* __restrict__ rows, const int* __restrict__ slot_at,
                                                             float* __restrict__ y_slot, int* __restrict__ rows_slot) {
    using namespace sz;
    __shared__ float s[NS], aa[54], rootv[3];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int b = slot_at ? slot_at[p] : p;
    if (slot_at && (b < 0 || b >= n_slots)) return;
    float* S = state + (size_t)b * STRIDE;
    const StreamWords w = stream_words(S);
    const int row = rows ? rows[p] : 0;
    const int ns = (w.shape & 1) ? NS2 : NS;   // this buffer's state width; ns - 111 SBP columns (20 / 8)
    if (slot_at) {
        if (y_slot && tid < ns) y_slot[(size_t)b * ns + tid] = y_last[(size_t)p * ns + tid];
        if (rows_slot && tid == 0) rows_slot[b] = row;
    }
    if (row < 0) return;
    if (k < 0) k = w.ctr - 5;   // TIP_STREAM_FRAME_AUTO: the call that belongs to the last ingested frame
    // requested up front, with the prediction row: the previous pose / root velocity (the averaging below) and the root IMU rotation
    // — behind the first barrier each was one more exposed round trip
    float last3[3] = {0.f, 0.f, 0.f}, rr[9];
    if (tid >= 1 && tid < 18 && k > 0)
        for (int e = 0; e < 3; ++e) last3[e] = S[LAST + (tid - 1) * 3 + e];
    if (tid >= 64 && tid < 67 && k > 0) last3[0] = S[LAST + 51 + (tid - 64)];
    if (tid == 0)
        for (int e = 0; e < 9; ++e) rr[e] = S[LOC + (k % WIN) * NIMU + e];
    if (__builtin_expect(ns == NS, 1))
        stream_consume_filter<NS>(s, S, OUTS, y_last + (size_t)p * NS, c_out + (size_t)b * (NS - 111), k, tid);
    else
        stream_consume_filter<NS2>(s, S, OUTS, y_last + (size_t)p * NS2, c_out + (size_t)b * (NS2 - 111), k, tid);
    __syncthreads();
    float* hrow = S + HIST + ((k + 1) % WIN) * ns;   // the history row this call feeds back
    if (tid < 18) {
        float rv[3];
        if (tid == 0) {   // root rotation comes from the IMU, not from the prediction (:160-162)
            float m[3][3] = {{rr[0], rr[1], rr[2]}, {rr[3], rr[4], rr[5]}, {rr[6], rr[7], rr[8]}};
            polar_newton(m);
            float q[4];
            mat_to_quat(m, q);
            quat_to_rotvec(q, rv);
        } else {          // 6D -> rotation (columns normalised with +1e-6, third by cross product; data_utils.py:171-176)
            const float* p = s + tid * 6;
            float a1[3] = {p[0], p[2], p[4]}, a2[3] = {p[1], p[3], p[5]};
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
            for (int e = 0; e < 3; ++e) S[LAST + (tid - 1) * 3 + e] = rv[e];
        }
        for (int e = 0; e < 3; ++e) aa[tid * 3 + e] = rv[e];
        float o6[6];
        rotvec_to_6d(rv, o6);   // :78-85
        for (int e = 0; e < 6; ++e) hrow[tid * 6 + e] = o6[e];
    } else if (tid >= 64 && tid < 67) {
        const int e = tid - 64;
        float v = s[108 + e];
        if (k > 0) v = (v + last3[0]) * 0.5f;
        S[LAST + 51 + e] = v;
        rootv[e] = v;
        hrow[108 + e] = v;
    } else if (tid >= 128 && tid < 128 + ns - 111) {
        hrow[111 + (tid - 128)] = s[111 + (tid - 128)];
    }
    __syncthreads();
    // s_t[3:114]: 54 axis-angles, root velocity, 54 zeros
    if (tid < 111) s_rest[(size_t)b * 111 + tid] = tid < 54 ? aa[tid] : (tid < 57 ? rootv[tid - 54] : 0.f);
}

// ---- host override of the fed-back pose: columns 0-107 of the NEWEST history row of the listed slots ------------------------
// RTRunner with multi_sbp_terrain_and_correction feeds back a pose its two-joint IK corrected on the host, not the pose it returns
// (real_time_runner.py:483-495: record_state_aa_and_c(st_hist_copy, c_t)).  Block j rewrites, for slot slots[j], the 6D columns of
// the row the last consume wrote (call k = frame counter - 5 -> hist[(k + 1) % 40]) from the 18 axis-angle joints q_aa[j]
// (data_utils.py:182-187).  Root velocity and c_t columns, last[54], the output ring and every other slot are not touched; a slot
// that has not consumed a frame yet (k < 0) or lies outside [0, B) is skipped.
__global__ __launch_bounds__(64) void stream_history_override_kernel(float* __restrict__ state, int B, const int* __restrict__ slots,
                                                                     const float* __restrict__ q_aa) {
    using namespace sz;
    const int j = blockIdx.x, tid = threadIdx.x;
    const int b = slots[j];
    if (b < 0 || b >= B) return;
    float* S = state + (size_t)b * STRIDE;
    const StreamWords w = stream_words(S);
    const int ns = (w.shape & 1) ? NS2 : NS;
    const int k = w.ctr - 5;
    if (k < 0 || tid >= 18) return;
    stream_hist_pose(S, HIST + ((k + 1) % WIN) * ns, q_aa + (size_t)j * 54, 0, tid);
}

// ==== any window length W = 1 .. 128 (the _w entry points at window != 40) =====================================================
// The reference's RTRunnerMin(char, model, max_input_l = W, ...) / RTRunner (real_time_runner_minimal.py:24,54,131,139;
// real_time_runner.py:29,413,421).  What W changes (nothing else does): the call for frame f has T = min(max(f - 4, 0), W) rows; the
// local-frame, acc-sum and history rings are W deep (ring index j % W, j >= 0 throughout); the raw ring (11) and the output filter (6)
// are not.  The acc-sum feature still spans ACC_SUM_WIN_LEN = 40 rows (constants.py:17, :136): the newest min(T, 40) rows of the
// window, oldest first and this frame's row last; older rows of a longer window keep the value the acc-sum ring holds for them.
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
struct StreamCheck { bool ok; int shape; };
// S: the workgroup's own block under L
__device__ __forceinline__ StreamCheck stream_check(const float* __restrict__ state, const float* __restrict__ S, const StreamLay L) {
    const int w0 = reinterpret_cast<const int*>(state)[2];   // block 0's shape word
    const bool tagged = (w0 >> 16) == sz::WTAG, ok0 = tagged && ((w0 >> 2) & 0x3fff) == L.win;
    // (this block's own word only once block 0 has confirmed the stride that leads to it)
    return {ok0 && reinterpret_cast<const int*>(S)[2] == w0, tagged ? (w0 & 3) : 3};
}

// ---- reset / attach (as stream_reset_kernel).  An attach to a buffer of another layout does nothing. -------------------------------
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
    if (tid < 18) stream_hist_pose(S, L.hist, si, 3, tid);
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

// ---- ingest (as stream_ingest_body).  The window gather is plain strided loops. ----------------------------------------------------
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
        T = attached ? window_len(f, L) : 0;
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
    stream_ingest_chain<NX>(sm, loc, S, b, raw_in, f, x_imu, ldw, T, acc_old, L);
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

// ---- consume (as stream_consume_kernel; rows, slot_at, y_slot, rows_slot as there) -------------------------------------------------
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
        stream_consume_filter<NS>(s, S, L.outs, y_last + (size_t)p * NS, c_out + (size_t)b * (NS - 111), k, tid);
    else
        stream_consume_filter<NS2>(s, S, L.outs, y_last + (size_t)p * NS2, c_out + (size_t)b * (NS2 - 111), k, tid);
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

// ---- host override of the fed-back pose (as stream_history_override_kernel) --------------------------------------------------------
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
    stream_hist_pose(S, L.hist + ((k + 1) % W) * ns, q_aa + (size_t)j * 54, 0, tid);
}

}  // namespace tip

using namespace tip;

// ---- host side ------------------------------------------------------------------------------------------------------------------
// One launcher per kernel pair: it checks the arguments once (the pointers a form of the call cannot do without are checked by that
// form's entry point) and launches the 40-row kernel at window == 40, the any-length kernel otherwise.  The _w entry points call it
// with their window, the 40-row entry points with sz::WIN.  A call over no streams (slots, positions) returns TIP_OK without a launch.
static bool bad_window(int window) { return window < 1 || window > sz::WIN_MAX; }

// k40(state, args...) at 40 rows, kw(state, args..., window) at any other length
template <class K40, class KW, class... A>
static int launch(K40 k40, KW kw, int blocks, int threads, int window, tip_stream_t stream, void* state, A... args) {
    if (window == sz::WIN)
        hipLaunchKernelGGL(k40, dim3(blocks), dim3(threads), 0, static_cast<hipStream_t>(stream), static_cast<float*>(state), args...);
    else
        hipLaunchKernelGGL(kw, dim3(blocks), dim3(threads), 0, static_cast<hipStream_t>(stream), static_cast<float*>(state), args..., window);
    return tip_launch_status();
}

// reset (slots == nullptr: all n_streams, count == n_streams) / attach (the listed slots; shape ignored)
static int stream_reset(void* state, const float* s_init, int n_streams, const int* slots, int count, int shape, int window,
                        tip_stream_t stream) {
    if (bad_window(window) || !state || n_streams < 0 || count < 0 || (count > 0 && !s_init)) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_streams == 0) return TIP_OK;
    return launch(stream_reset_kernel, stream_reset_w_kernel, count, 64, window, stream, state, s_init, n_streams, slots, shape);
}

// ingest: B windows.  rows == nullptr: lock step at frame_idx (B == n_streams; newest: tip_stream_ingest_newest's, 40 rows only);
// otherwise every slot on its own counter, position p serving slot slot_at[p], or slot p without a map (B == n_streams)
static int stream_ingest(void* state, const float* raw_imu, int n_streams, int frame_idx, float* x_imu, float* x_s, int* rows,
                         const int* slot_at, int B, int window, int newest, tip_stream_t stream) {
    if (bad_window(window) || !state || !raw_imu || n_streams < 0 || B < 0 || B > n_streams || frame_idx < TIP_STREAM_FRAME_AUTO)
        return TIP_ERR_INVALID_ARG;
    const int T = rows || frame_idx == TIP_STREAM_FRAME_AUTO ? window : window_len(frame_idx, stream_lay(window));
    if (T > 0 && (!x_imu || !x_s)) return TIP_ERR_INVALID_ARG;
    if (B == 0) return TIP_OK;
    if (window == sz::WIN)   // (not through launch: `newest` is this kernel's alone)
        hipLaunchKernelGGL(stream_ingest_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<float*>(state),
                           raw_imu, n_streams, frame_idx, x_imu, x_s, T, newest, rows, slot_at);
    else
        hipLaunchKernelGGL(stream_ingest_w_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<float*>(state),
                           raw_imu, n_streams, frame_idx, x_imu, x_s, T, rows, slot_at, window);
    return tip_launch_status();
}

// consume: B rows of y.  rows == nullptr: lock step, call call_idx (B == n_streams); otherwise as stream_ingest's, call_idx AUTO
static int stream_consume(void* state, const float* y, const int* rows, const int* slot_at, int B, int n_streams, int call_idx,
                          float* s_rest, float* c_t, float* y_slot, int* rows_slot, int window, tip_stream_t stream) {
    if (bad_window(window) || !state || !y || !s_rest || !c_t || n_streams < 0 || B < 0 || B > n_streams || call_idx < TIP_STREAM_FRAME_AUTO)
        return TIP_ERR_INVALID_ARG;
    if (B == 0) return TIP_OK;
    return launch(stream_consume_kernel, stream_consume_w_kernel, B, 192, window, stream, state, y, n_streams, call_idx, s_rest, c_t, rows,
                  slot_at, y_slot, rows_slot);
}

extern "C" {

int tip_stream_state_bytes_w(int n_streams, int window, size_t* bytes) {
    if (bad_window(window) || n_streams < 0 || !bytes) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)n_streams * stream_lay(window).stride * sizeof(float);
    return TIP_OK;
}

int tip_stream_frame_counter_offset(size_t* bytes) {   // where stream 0's 40-row block keeps the index of the last ingested frame (an int)
    if (!bytes) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)sz::CTR * sizeof(float);
    return TIP_OK;
}

int tip_stream_window_len_w(int frame_idx, int window) {   // T of the model call issued for frame `frame_idx`; 0 while priming
    if (bad_window(window)) return TIP_ERR_INVALID_ARG;
    return window_len(frame_idx, stream_lay(window));
}

int tip_stream_reset_w(void* state, const float* s_init, int n_streams, int n_sbps, int with_acc_sum, int window, tip_stream_t stream) {
    if (!s_init || (n_sbps != 2 && n_sbps != 5)) return TIP_ERR_INVALID_ARG;
    return stream_reset(state, s_init, n_streams, nullptr, n_streams, (n_sbps == 2 ? 1 : 0) | (with_acc_sum ? 0 : 2), window, stream);
}

int tip_stream_attach_w(void* state, int n_streams, const int* slots, const float* s_init, int count, int window, tip_stream_t stream) {
    if (count > 0 && !slots) return TIP_ERR_INVALID_ARG;
    return stream_reset(state, s_init, n_streams, slots, count, 0, window, stream);
}

int tip_stream_detach_w(void* state, int n_streams, const int* slots, int count, int window, tip_stream_t stream) {
    if (bad_window(window) || !state || n_streams < 0 || count < 0 || (count > 0 && !slots)) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_streams == 0) return TIP_OK;
    return launch(stream_detach_kernel, stream_detach_w_kernel, (count + 63) / 64, 64, window, stream, state, n_streams, slots, count);
}

int tip_stream_history_override_w(void* state, int n_streams, const int* slots, const float* q_aa, int count, int window,
                                  tip_stream_t stream) {
    if (bad_window(window) || !state || n_streams < 0 || count < 0 || (count > 0 && (!slots || !q_aa))) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_streams == 0) return TIP_OK;
    return launch(stream_history_override_kernel, stream_history_override_w_kernel, count, 64, window, stream, state, n_streams, slots, q_aa);
}

int tip_stream_ingest_w(void* state, const float* raw_imu, int n_streams, int frame_idx, float* x_imu, float* x_s, int window,
                        tip_stream_t stream) {
    return stream_ingest(state, raw_imu, n_streams, frame_idx, x_imu, x_s, nullptr, nullptr, n_streams, window, 0, stream);
}

int tip_stream_ingest_staggered_w(void* state, const float* raw_imu, int n_streams, float* x_imu, float* x_s, int* rows, int window,
                                  tip_stream_t stream) {
    if (!rows) return TIP_ERR_INVALID_ARG;
    return stream_ingest(state, raw_imu, n_streams, 0, x_imu, x_s, rows, nullptr, n_streams, window, 0, stream);
}

int tip_stream_ingest_mapped_w(void* state, const float* raw_imu, int n_streams, const int* slot_at, int B, float* x_imu, float* x_s,
                               int* rows, int window, tip_stream_t stream) {
    if (!rows || !slot_at) return TIP_ERR_INVALID_ARG;
    return stream_ingest(state, raw_imu, n_streams, 0, x_imu, x_s, rows, slot_at, B, window, 0, stream);
}

int tip_stream_consume_w(void* state, const float* y_last, int n_streams, int call_idx, float* s_rest, float* c_t, int window,
                         tip_stream_t stream) {
    return stream_consume(state, y_last, nullptr, nullptr, n_streams, n_streams, call_idx, s_rest, c_t, nullptr, nullptr, window, stream);
}

int tip_stream_consume_staggered_w(void* state, const float* y_last, const int* rows, int n_streams, float* s_rest, float* c_t,
                                   int window, tip_stream_t stream) {
    if (!rows) return TIP_ERR_INVALID_ARG;
    return stream_consume(state, y_last, rows, nullptr, n_streams, n_streams, TIP_STREAM_FRAME_AUTO, s_rest, c_t, nullptr, nullptr, window,
                          stream);
}

int tip_stream_consume_mapped_w(void* state, const float* y, const int* rows, const int* slot_at, int B, int n_streams, float* s_rest,
                                float* c_t, float* y_slot, int* rows_slot, int window, tip_stream_t stream) {
    if (!rows || !slot_at) return TIP_ERR_INVALID_ARG;
    return stream_consume(state, y, rows, slot_at, B, n_streams, TIP_STREAM_FRAME_AUTO, s_rest, c_t, y_slot, rows_slot, window, stream);
}

// ---- the 40-row entry points ----------------------------------------------------------------------------------------------------
int tip_stream_state_bytes(int n_streams, size_t* bytes) { return tip_stream_state_bytes_w(n_streams, sz::WIN, bytes); }
int tip_stream_window_len(int frame_idx) { return window_len(frame_idx, StreamLay40{}); }
int tip_stream_reset_shaped(void* state, const float* s_init, int n_streams, int n_sbps, int with_acc_sum, tip_stream_t stream) {
    return tip_stream_reset_w(state, s_init, n_streams, n_sbps, with_acc_sum, sz::WIN, stream);
}
int tip_stream_reset(void* state, const float* s_init, int n_streams, tip_stream_t stream) {
    return tip_stream_reset_w(state, s_init, n_streams, 5, 1, sz::WIN, stream);
}
int tip_stream_history_override(void* state, int n_streams, const int* slots, const float* q_aa, int count, tip_stream_t stream) {
    return tip_stream_history_override_w(state, n_streams, slots, q_aa, count, sz::WIN, stream);
}
int tip_stream_ingest(void* state, const float* raw_imu, int n_streams, int frame_idx, float* x_imu, float* x_s, tip_stream_t stream) {
    return stream_ingest(state, raw_imu, n_streams, frame_idx, x_imu, x_s, nullptr, nullptr, n_streams, sz::WIN, 0, stream);
}
int tip_stream_ingest_newest(void* state, const float* raw_imu, int n_streams, int frame_idx, float* x_imu, float* x_s,
                             tip_stream_t stream) {
    return stream_ingest(state, raw_imu, n_streams, frame_idx, x_imu, x_s, nullptr, nullptr, n_streams, sz::WIN, 1, stream);
}
int tip_stream_consume(void* state, const float* y_last, int n_streams, int call_idx, float* s_rest, float* c_t, tip_stream_t stream) {
    return tip_stream_consume_w(state, y_last, n_streams, call_idx, s_rest, c_t, sz::WIN, stream);
}
int tip_stream_attach(void* state, int n_streams, const int* slots, const float* s_init, int count, tip_stream_t stream) {
    return tip_stream_attach_w(state, n_streams, slots, s_init, count, sz::WIN, stream);
}
int tip_stream_detach(void* state, int n_streams, const int* slots, int count, tip_stream_t stream) {
    return tip_stream_detach_w(state, n_streams, slots, count, sz::WIN, stream);
}
int tip_stream_ingest_staggered(void* state, const float* raw_imu, int n_streams, float* x_imu, float* x_s, int* rows, tip_stream_t stream) {
    return tip_stream_ingest_staggered_w(state, raw_imu, n_streams, x_imu, x_s, rows, sz::WIN, stream);
}
int tip_stream_consume_staggered(void* state, const float* y_last, const int* rows, int n_streams, float* s_rest, float* c_t,
                                 tip_stream_t stream) {
    return tip_stream_consume_staggered_w(state, y_last, rows, n_streams, s_rest, c_t, sz::WIN, stream);
}
int tip_stream_ingest_mapped(void* state, const float* raw_imu, int n_streams, const int* slot_at, int B, float* x_imu, float* x_s,
                             int* rows, tip_stream_t stream) {
    return tip_stream_ingest_mapped_w(state, raw_imu, n_streams, slot_at, B, x_imu, x_s, rows, sz::WIN, stream);
}
int tip_stream_consume_mapped(void* state, const float* y, const int* rows, const int* slot_at, int B, int n_streams, float* s_rest,
                              float* c_t, float* y_slot, int* rows_slot, tip_stream_t stream) {
    return tip_stream_consume_mapped_w(state, y, rows, slot_at, B, n_streams, s_rest, c_t, y_slot, rows_slot, sz::WIN, stream);
}

}  // extern "C"
