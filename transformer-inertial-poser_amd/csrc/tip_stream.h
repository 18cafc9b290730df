// tip_stream.h — the device code that the two forms of the streaming kernels in tip_stream.hip share (40-row windows with compile-time
// trip counts; any window length W as a value): the two block layouts as one policy, the control words, scipy's Rotation restated, the
// window length rule, and on top of the policy the pieces written once — the ingest's smoothing chain, the consume's output filter, the
// history row of a reset and of an override.  What is deliberately written twice, and why, is in the header of tip_stream.hip.
#pragma once
#include "tip_internal.h"

namespace tip {

namespace sz {
constexpr int NIMU = 72, NS = 131, NX = 90, WIN = 40, RAWN = 11, OUTN = 6;
constexpr int RAW = 0;
constexpr int LOC = RAW + RAWN * NIMU;        // 792
constexpr int ACCS = LOC + WIN * NIMU;        // 3672
constexpr int HIST = ACCS + WIN * 18;         // 4392
constexpr int OUTS = HIST + WIN * NS;         // 9632
constexpr int LAST = OUTS + OUTN * NS;        // 10418
constexpr int CTR = LAST + 54;                // 10472: frame index of the last ingest (int)
constexpr int ATT = CTR + 1;                  // 10473: staggered slots: 1 = attached (int); the lock-step entry points ignore it
constexpr int SHP = ATT + 1;                  // 10474: shape of the whole buffer (int): bit 0 = two SBPs (NS 119), bit 1 = no acc-sum (NX 72)
constexpr int STRIDE = 10496;                 // SHP + 1 = 10475, padded to a multiple of 64
constexpr int NS2 = 119;                      // 108 + 3 + 2 * 4
constexpr int WIN_MAX = 128;                  // the longest window served (the training step's T limit)
constexpr int ACC_SUM_WIN = 40;               // ACC_SUM_WIN_LEN: the rows the acc-sum feature spans at any window length
constexpr int WTAG = 0x5457;                  // bits 16-30 of an any-length buffer's shape word
}  // namespace sz

// The layout policy: where the parts of a block are, how deep its rings are, how large it is.  At 40 rows every member is a compile-time
// constant (the offsets above); at any other length they are values, the parts of the 40-row block behind the three control words,
// which then sit at floats 0 .. 2 (tip_stream.hip: "State per stream").
struct StreamLay40 {
    static constexpr int win = sz::WIN, raw = sz::RAW, loc = sz::LOC, accs = sz::ACCS, hist = sz::HIST, outs = sz::OUTS, last = sz::LAST,
                         stride = sz::STRIDE;
};
struct StreamLay { int win, raw, loc, accs, hist, outs, last, stride; };
__host__ __device__ constexpr StreamLay stream_lay(int W) {
    const int raw = 3, loc = raw + sz::RAWN * sz::NIMU, accs = loc + W * sz::NIMU, hist = accs + W * 18, outs = hist + W * sz::NS;
    const int last = outs + sz::OUTN * sz::NS;
    return {W, raw, loc, accs, hist, outs, last, (last + 54 + 63) / 64 * 64};
}
static_assert(stream_lay(sz::WIN).stride == sz::STRIDE, "a 40-row block is as large under either layout");

// the three control words of a block, requested together: frame counter, attached flag, shape
struct StreamWords { int ctr, att, shape; };
__device__ __forceinline__ StreamWords stream_words(const float* S) {
    const int* w = reinterpret_cast<const int*>(S + sz::CTR);
    return {w[0], w[1], w[2] & 3};
}

// ---- scipy.spatial.transform.Rotation restated (fp32) -------------------------------------------------------
// from_matrix() first replaces a non-orthogonal input by the NEAREST rotation (U V^T of its SVD), then extracts the
// quaternion.  The two inputs that occur here have closed forms for that polar factor:
//   * M = [a1 a2 a1 x a2] (data_utils.py:171-176, columns normalised but not orthogonalised): M^T M is block
//     diagonal, so R = [ [a1 a2] A^{-1/2} , a3/|a3| ] with the 2x2 A = [[a1.a1, a1.a2], [a1.a2, a2.a2]] and
//     A^{1/2} = (A + sqrt(det A) I) / sqrt(tr A + 2 sqrt(det A)).
//   * the root IMU rotation (orthonormal up to sensor round-off): two Newton steps X <- (X + X^{-T}) / 2.
__device__ __forceinline__ void polar_two_axis(const float a1[3], const float a2[3], float m[3][3]) {
    const float a3[3] = {a1[1] * a2[2] - a1[2] * a2[1], a1[2] * a2[0] - a1[0] * a2[2], a1[0] * a2[1] - a1[1] * a2[0]};
    const float p = a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2];
    const float q = a2[0] * a2[0] + a2[1] * a2[1] + a2[2] * a2[2];
    const float c = a1[0] * a2[0] + a1[1] * a2[1] + a1[2] * a2[2];
    const float d = sqrtf(fmaxf(p * q - c * c, 0.f));
    const float tau = sqrtf(p + q + 2.f * d);
    const float den = (p + d) * (q + d) - c * c;
    const float n3sq = a3[0] * a3[0] + a3[1] * a3[1] + a3[2] * a3[2];
    if (!(den > 1e-10f) || !(n3sq > 1e-12f)) {
        // (anti)parallel or vanishing predicted axes: M is singular, its polar factor is not unique (scipy's SVD returns SOME rotation
        // there) and the closed form above divides by zero — seen once in 300 k stream-frames of a random-weight closed loop, after
        // which the NaN lived on in the pose average.  Any orthonormal frame is as right as another: first axis along a1 (or x), the
        // second from the coordinate axis least aligned with it.
        float e1[3] = {a1[0], a1[1], a1[2]};
        float n1 = sqrtf(p);
        if (!(n1 > 1e-12f)) { e1[0] = 1.f; e1[1] = 0.f; e1[2] = 0.f; n1 = 1.f; }
        for (int i = 0; i < 3; ++i) e1[i] /= n1;
        const float ax = fabsf(e1[0]), ay = fabsf(e1[1]), az = fabsf(e1[2]);
        float h[3] = {0.f, 0.f, 0.f};
        h[(ax <= ay && ax <= az) ? 0 : (ay <= az ? 1 : 2)] = 1.f;
        const float hd = h[0] * e1[0] + h[1] * e1[1] + h[2] * e1[2];
        float e2[3] = {h[0] - hd * e1[0], h[1] - hd * e1[1], h[2] - hd * e1[2]};
        const float n2 = sqrtf(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
        for (int i = 0; i < 3; ++i) e2[i] /= n2;
        const float e3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        for (int i = 0; i < 3; ++i) { m[i][0] = e1[i]; m[i][1] = e2[i]; m[i][2] = e3[i]; }
        return;
    }
    const float f = tau / den;
    const float b00 = (q + d) * f, b01 = -c * f, b11 = (p + d) * f;
    const float n3 = 1.f / sqrtf(n3sq);
    for (int i = 0; i < 3; ++i) {
        m[i][0] = a1[i] * b00 + a2[i] * b01;
        m[i][1] = a1[i] * b01 + a2[i] * b11;
        m[i][2] = a3[i] * n3;
    }
}

__device__ __forceinline__ void polar_newton(float m[3][3]) {
    for (int it = 0; it < 2; ++it) {
        // inverse transpose = cofactor matrix / det
        float cof[3][3];
        cof[0][0] = m[1][1] * m[2][2] - m[1][2] * m[2][1];
        cof[0][1] = m[1][2] * m[2][0] - m[1][0] * m[2][2];
        cof[0][2] = m[1][0] * m[2][1] - m[1][1] * m[2][0];
        cof[1][0] = m[0][2] * m[2][1] - m[0][1] * m[2][2];
        cof[1][1] = m[0][0] * m[2][2] - m[0][2] * m[2][0];
        cof[1][2] = m[0][1] * m[2][0] - m[0][0] * m[2][1];
        cof[2][0] = m[0][1] * m[1][2] - m[0][2] * m[1][1];
        cof[2][1] = m[0][2] * m[1][0] - m[0][0] * m[1][2];
        cof[2][2] = m[0][0] * m[1][1] - m[0][1] * m[1][0];
        const float det = m[0][0] * cof[0][0] + m[0][1] * cof[0][1] + m[0][2] * cof[0][2];
        const float id = 1.f / det;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) m[i][j] = 0.5f * (m[i][j] + cof[i][j] * id);
    }
}

// quaternion of a rotation matrix by the largest-of-{diag, trace} rule, normalised (the extraction scipy uses).
__device__ __forceinline__ void mat_to_quat(const float m[3][3], float q[4]) {
    const float tr = m[0][0] + m[1][1] + m[2][2];
    int choice = 0;
    float best = m[0][0];
    if (m[1][1] > best) { best = m[1][1]; choice = 1; }
    if (m[2][2] > best) { best = m[2][2]; choice = 2; }
    if (tr > best) { choice = 3; }
    if (choice != 3) {
        const int i = choice, j = (i + 1) % 3, k = (j + 1) % 3;
        q[i] = 1.f - tr + 2.f * m[i][i];
        q[j] = m[j][i] + m[i][j];
        q[k] = m[k][i] + m[i][k];
        q[3] = m[k][j] - m[j][k];
    } else {
        q[0] = m[2][1] - m[1][2];
        q[1] = m[0][2] - m[2][0];
        q[2] = m[1][0] - m[0][1];
        q[3] = 1.f + tr;
    }
    const float n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}

// as_rotvec(): w >= 0 branch, small-angle series below 1e-3.
__device__ __forceinline__ void quat_to_rotvec(const float qi[4], float rv[3]) {
    float q[4] = {qi[0], qi[1], qi[2], qi[3]};
    if (q[3] < 0.f) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const float angle = 2.f * atan2f(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]), q[3]);
    float scale;
    if (angle <= 1e-3f) {
        const float a2 = angle * angle;
        scale = 2.f + a2 / 12.f + 7.f * a2 * a2 / 2880.f;
    } else {
        scale = angle / sinf(angle * 0.5f);
    }
    rv[0] = scale * q[0]; rv[1] = scale * q[1]; rv[2] = scale * q[2];
}

// from_rotvec().as_matrix()[:, :2] -> (3x2) row-major
__device__ __forceinline__ void rotvec_to_6d(const float rv[3], float out[6]) {
    const float angle = sqrtf(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    float scale;
    if (angle <= 1e-3f) {
        const float a2 = angle * angle;
        scale = 0.5f - a2 / 48.f + a2 * a2 / 3840.f;
    } else {
        scale = sinf(angle * 0.5f) / angle;
    }
    const float x = scale * rv[0], y = scale * rv[1], z = scale * rv[2], w = cosf(angle * 0.5f);
    const float x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const float xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    out[0] = x2 - y2 - z2 + w2;   // m00
    out[1] = 2.f * (xy - zw);     // m01
    out[2] = 2.f * (xy + zw);     // m10
    out[3] = -x2 + y2 - z2 + w2;  // m11
    out[4] = 2.f * (xz - yw);     // m20
    out[5] = 2.f * (yz + xw);     // m21
}

template <class Lay>   // (the layout, not its length: at 40 rows the bound then is a constant where the rule is compiled)
__host__ __device__ __forceinline__ int window_len(int frame_idx, const Lay L) {   // T of the model call issued for frame `frame_idx`
    if (frame_idx < 5) return 0;                                                    // 0 while priming
    const int t = frame_idx - 4;
    return t < L.win ? t : L.win;
}

// ---- ingest: the smoothing chain (:59-76, :131-141), from this call's raw frame to its row of x_imu ---------------------------
// Two LDS barriers.  The raw frame is used from its register (it also goes to the ring for the next ten calls), the ten older raw rows
// do not depend on this call, and every thread inverts the 3 x 3 root matrix for itself (40 flops) — with the frame stored, re-read
// behind a barrier, and the inverse computed by thread 0 between two more, the chain was five barriers with a global round trip each.
// b: the stream (its row of raw_in); ldw: rows between two windows of x_imu, of which this call's row is the T-th of window blockIdx.x;
// acc_old (threads < 18): the acc-sum over the older rows it spans.
template <int NX, class Lay>
__device__ __forceinline__ void stream_ingest_chain(float* sm, float* loc, float* S, int b, const float* raw_in, int f, float* x_imu, int ldw,
                                                    int T, float acc_old, const Lay L) {
    using namespace sz;
    constexpr bool ACC = NX > NIMU;
    const int p = blockIdx.x, tid = threadIdx.x, k = f - 5;
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
    float* xin = x_imu + (size_t)p * ldw * NX + (size_t)(T - 1) * NX;
    if (tid < NIMU) {
        S[L.loc + (k % L.win) * NIMU + tid] = loc[tid];
        xin[tid] = loc[tid];
    }
    if (ACC && tid < 18) {   // acc-sum feature: the older rows' partial + this frame, added last (:136)
        const float acc = acc_old + loc[54 + tid];
        S[L.accs + (k % L.win) * 18 + tid] = acc;
        xin[NIMU + tid] = acc / 15.0f;                        // :139-141
    }
}

// ---- consume: the 6-tap 0.6^k output filter over the block's output ring S + outs, SBP decode (:87-112) ------------------------------
// s: the filtered row (LDS); c_row: this stream's c_t.  The width is a compile-time constant here and nowhere else in a consume.
template <int NS>
__device__ __forceinline__ void stream_consume_filter(float* __restrict__ s, float* __restrict__ S, int outs, const float* __restrict__ y_row,
                                                      float* __restrict__ c_row, int k, int tid) {
    using namespace sz;
    const float coeff[OUTN] = {0.07776f, 0.1296f, 0.216f, 0.36f, 0.6f, 1.0f};   // 0.6^(5..0) (:57)
    const float csum = 0.07776f + 0.1296f + 0.216f + 0.36f + 0.6f + 1.0f;
    const int n = k + 1;
    if (tid < NS) {
        const float y = y_row[tid];
        S[outs + (k % OUTN) * NS + tid] = y;
        float v;
        if (n >= OUTN) {
            // the five older rows do not depend on this call's row: their loads go out with its load; the newest term is y itself
            // (the row just stored: same value, no store -> load round trip)
            float acc = 0.f;
            for (int i = 0; i < OUTN - 1; ++i) acc += S[outs + ((k - 5 + i) % OUTN) * NS + tid] * coeff[i];
            acc += y * coeff[OUTN - 1];
            v = acc / csum;
        } else {
            v = y;
        }
        if (tid >= 111) {
            const int ci = tid - 111;
            v = (ci & 3) == 0 ? (v > 0.f ? 1.f : 0.f) : v / 5.0f;      // :107-110 (real_time_runner.py:323-330: 4 columns per SBP)
            // reference quirk: with fewer than 6 buffered rows the decode happens IN PLACE in the buffered row (:99)
            if (n < OUTN) S[outs + (k % OUTN) * NS + tid] = v;
            c_row[ci] = v;
        }
        s[tid] = v;
    }
}

// ---- the 6D columns of history row S + h from 18 axis-angle joints (data_utils.py:182-187): thread tid < 18 writes joint tid ---------
// aa: joint j at aa[o + 3 j .. o + 3 j + 2] (a reset's s_init row, an override's q_aa row)
__device__ __forceinline__ void stream_hist_pose(float* S, int h, const float* aa, int o, int tid) {
    const float rv[3] = {aa[o + tid * 3], aa[o + 1 + tid * 3], aa[o + 2 + tid * 3]};
    float o6[6];
    rotvec_to_6d(rv, o6);
    for (int e = 0; e < 6; ++e) S[h + tid * 6 + e] = o6[e];
}

}  // namespace tip
