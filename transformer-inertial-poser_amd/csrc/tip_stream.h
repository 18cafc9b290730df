// tip_stream.h — what the streaming kernels of tip_stream.hip (40-row windows, compile-time trip counts) and tip_stream_w.hip (any
// window length, as a value) share: the block layout at 40 rows, the control words, scipy's Rotation restated, the window length rule.
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
}  // namespace sz

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

__host__ __device__ __forceinline__ int window_len(int frame_idx) {   // T of the model call issued for frame `frame_idx`; 0 while priming
    if (frame_idx < 5) return 0;
    const int t = frame_idx - 4;
    return t < sz::WIN ? t : sz::WIN;
}

}  // namespace tip
