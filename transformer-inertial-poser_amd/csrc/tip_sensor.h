// tip_sensor.h — what the sensor front end (tip_sensor.hip) and the gap filling (tip_fill.hip) share: the calibration block of a slot
// and the per-sensor arithmetic of the per-frame transform, one __device__ function that tip_sensor_transform and tip_fill_packets
// both call, so that a recorded packet session and the live launch agree bit for bit.
#pragma once
#include "tip_internal.h"

namespace tip {

namespace sn {
constexpr int SENSORS = 6, PACKET = 42, RAW = 72, TABLE = 126;
constexpr int T_GN_GP = 0, T_OFFSET = 54, T_B0_S0 = 72;       // float offsets inside the table
enum : int { UNCALIBRATED = 0, HEADING = 1, HEADING_DONE = 2, TPOSE = 3, LIVE = 4 };
}  // namespace sn

// One slot's calibration.  `table` is what the transform reads and what set / get move; `heading` is the fp64 mean the heading finish
// rounded into table[T_GN_GP ..], kept so that the T-pose finish is fp64 from the sums to its single rounding (a set writes the
// table's values there).  1536 bytes: a multiple of 64, the doubles 8-byte aligned.
struct SensorCal {
    float table[sn::TABLE];       // R_Gn_Gp [6][9] | acc_offset [6][3] | R_B0_S0 [6][9]
    double sums[sn::RAW];         // rotation sums [6][9] | acceleration sums [6][3]
    double heading[54];
    int count, phase;
    int pad[4];
};
static_assert(sizeof(SensorCal) == 1536, "SensorCal layout");

// scipy's Rotation.from_quat(q).as_matrix() on q = (x, y, z, w): normalise, then the nine polynomials.  A zero or non-finite
// quaternion has no rotation (scipy raises): `ok` is false and m is not written.
template <typename F>
__device__ __forceinline__ bool q2r(F x, F y, F z, F w, F* m) {
    const F n2 = x * x + y * y + z * z + w * w;
    if (!(n2 > F(0)) || !__builtin_isfinite(n2)) return false;  // zero, NaN (compares false), Inf or an overflowed norm
    F n;
    if constexpr (std::is_same<F, float>::value) n = sqrtf(n2);
    else n = sqrt(n2);
    x /= n, y /= n, z /= n, w /= n;
    const F x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const F xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    m[0] = x2 - y2 - z2 + w2, m[1] = F(2) * (xy - zw), m[2] = F(2) * (xz + yw);
    m[3] = F(2) * (xy + zw), m[4] = -x2 + y2 - z2 + w2, m[5] = F(2) * (yz - xw);
    m[6] = F(2) * (xz - yw), m[7] = F(2) * (yz + xw), m[8] = -x2 - y2 + z2 + w2;
    return true;
}

// np.clip(v, -m, m): a NaN stays a NaN (both comparisons are false).  fminf / fmaxf would return the finite operand.
__device__ __forceinline__ float clip_nan_transparent(float v, float m) { return v < -m ? -m : (v > m ? m : v); }

// One sensor of one packet row: p = q0 q1 q2 q3 ax ay az, `table` the 126 floats of the row's calibration, k the sensor.  Writes the
// sensor's 9 rotation columns to r_out and its 3 acceleration columns to a_out; `live` false (an unfinished calibration) or a
// quaternion without a rotation gives NaN in all twelve, never a finite value.
__device__ __forceinline__ void sensor_row(const float* __restrict__ table, bool live, const float* __restrict__ p, int k, float max_acc,
                                           float* __restrict__ r_out, float* __restrict__ a_out) {
    float S[9];                                                  // R_Gn_St
    const bool ok = live && q2r<float>(p[0], p[1], p[2], p[3], S);
    if (!ok) {                                                   // an unfinished calibration, or no rotation: never a finite row
        const float nan = __builtin_nanf("");
        for (int j = 0; j < 9; ++j) r_out[j] = nan;
        for (int j = 0; j < 3; ++j) a_out[j] = nan;
        return;
    }
    const float* G = table + sn::T_GN_GP + 9 * k;                // R_Gn_Gp
    const float* B = table + sn::T_B0_S0 + 9 * k;                // R_B0_S0
    float P[9];                                                  // R_Gp_St = R_Gn_Gp^T R_Gn_St
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) P[3 * r + q] = G[r] * S[q] + G[3 + r] * S[3 + q] + G[6 + r] * S[6 + q];
    for (int r = 0; r < 3; ++r)                                  // R_Gp_Bt = R_Gp_St R_B0_S0^T
        for (int q = 0; q < 3; ++q) r_out[3 * r + q] = P[3 * r] * B[3 * q] + P[3 * r + 1] * B[3 * q + 1] + P[3 * r + 2] * B[3 * q + 2];
    const float ax = p[4], ay = p[5], az = p[6];
    for (int r = 0; r < 3; ++r) {
        const float a = P[3 * r] * ax + P[3 * r + 1] * ay + P[3 * r + 2] * az - table[sn::T_OFFSET + 3 * k + r];
        a_out[r] = clip_nan_transparent(a, max_acc);
    }
}

}  // namespace tip
