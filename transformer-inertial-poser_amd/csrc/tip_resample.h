// tip_resample.h — what the resampler's kernels (tip_resample.hip), the clock-sync / predicted-tick kernels (tip_clock.hip) and the
// display-time poses (tip_display.hip) share: the layout of a slot's packet ring, the emit rule, the per-sensor interpolation and its
// continuation past the newer packet, each one __device__ function that the files call, so that a predicted tick that falls back to the
// slerp rule, a fused push, and a pose's rotation between or past two rows agree with the plain entries bit for bit.
#pragma once
#include "tip_sensor.h"

namespace tip {

namespace rs {
constexpr int TILE = 32, THREADS = TILE * sn::SENSORS;       // rows (or slots) of a workgroup, one thread per (row, sensor)
constexpr int MIN_DEPTH = 2, MAX_DEPTH = 64;
constexpr int HDR = 16;                                      // head, have, total, dropped
enum : int { HOLD = 0, SLERP = 1 };
enum : int { F_INTERP = 0, F_HELD = 1, F_STALE = 2, F_EMPTY = 3, F_EARLY = 4 };
constexpr double TINY_ARC = 1e-5;                            // predict_sensor: below this arc (rad, between the quaternions) the weights are 1 - u and u
__host__ __device__ constexpr size_t slot_bytes(int depth) { return (size_t)HDR + (size_t)depth * (8 + 4 * sn::PACKET); }
}  // namespace rs

// One slot's block: int head (the ring index of the oldest entry), have, total, dropped; double stamp[depth]; float packet[depth][42].
struct ResampleSlot {
    int* hdr;
    double* stamp;
    float* packet;
};
__device__ __forceinline__ ResampleSlot resample_slot(void* state, int slot, int depth) {
    char* base = static_cast<char*>(state) + (size_t)slot * rs::slot_bytes(depth);
    ResampleSlot s;
    s.hdr = reinterpret_cast<int*>(base);
    s.stamp = reinterpret_cast<double*>(base + rs::HDR);
    s.packet = reinterpret_cast<float*>(base + rs::HDR + (size_t)depth * 8);
    return s;
}
__device__ __forceinline__ int clamp_int(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ long long clamp_ll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the emit rule: which packets, and where between them -------------------------------------------------------------------------------
// stamp(i), i < cnt: strictly increasing.  Returns the flag; for F_HELD `i` is the packet copied, for F_INTERP i and i + 1 are the
// bracket and u the position in it.
template <typename Stamp>
__device__ __forceinline__ int resample_decide(Stamp stamp, int cnt, double tau, double max_hold, int mode, int& i, double& u) {
    i = 0, u = 0.0;
    if (cnt < 1) return rs::F_EMPTY;
    if (!(tau >= stamp(0))) return rs::F_EARLY;              // (a NaN tau: nothing is known to be before it)
    const double s_last = stamp(cnt - 1);
    if (tau >= s_last) {
        i = cnt - 1;
        return (max_hold < 0.0 || tau - s_last <= max_hold) ? rs::F_HELD : rs::F_STALE;
    }
    int lo = 0, hi = cnt - 1;                                // stamp(lo) <= tau < stamp(hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (stamp(mid) <= tau) lo = mid;
        else hi = mid;
    }
    i = lo;
    const double s0 = stamp(lo), s1 = stamp(lo + 1);
    if (mode == rs::HOLD || (max_hold >= 0.0 && s1 - s0 > max_hold))
        return (max_hold < 0.0 || tau - s0 <= max_hold) ? rs::F_HELD : rs::F_STALE;
    u = (tau - s0) / (s1 - s0);
    return rs::F_INTERP;
}

__device__ __forceinline__ void resample_nan7(float* __restrict__ o) {
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int j = 0; j < 7; ++j) o[j] = nan;
}
__device__ __forceinline__ void resample_copy7(const float* __restrict__ p, float* __restrict__ o) {
#pragma unroll
    for (int j = 0; j < 7; ++j) o[j] = p[j];
}

// One sensor between two packets: a = q0 q1 q2 q3 ax ay az of the earlier packet, b of the later one, u in [0, 1); o[7].  The order of
// every operation is the header's ("timestamped packets", interpolation).
__device__ __forceinline__ void resample_sensor(const float* __restrict__ a, const float* __restrict__ b, double u, float* __restrict__ o) {
    float Ra[9], Rb[9];
    const bool ok = q2r<float>(a[0], a[1], a[2], a[3], Ra) && q2r<float>(b[0], b[1], b[2], b[3], Rb);
    if (!ok) {
        resample_nan7(o);
        return;
    }
    const float na = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);
    const float nb = sqrtf(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
    float qa[4], qb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) qa[j] = a[j] / na, qb[j] = b[j] / nb;
    float dot = qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3];
    if (dot < 0.f) {
#pragma unroll
        for (int j = 0; j < 4; ++j) qb[j] = -qb[j];
        dot = -dot;
    }
    const double d = (double)dot < 1.0 ? (double)dot : 1.0;
    double w0, w1;
    if (d > 1.0 - 1e-6) {
        w0 = 1.0 - u, w1 = u;
    } else {
        const double th = acos(d), st = sin(th);
        w0 = sin((1.0 - u) * th) / st, w1 = sin(u * th) / st;
    }
    const float f0 = (float)w0, f1 = (float)w1;
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = f0 * qa[j] + f1 * qb[j];
    float Rq[9];
    if (!q2r<float>(q[0], q[1], q[2], q[3], Rq)) {           // (the two quaternions pi apart: no shortest arc)
        resample_nan7(o);
        return;
    }
    const float nq = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = q[j] / nq;
    const float uf = (float)u, vf = 1.f - uf;
    float g[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float ga = Ra[3 * r] * a[4] + Ra[3 * r + 1] * a[5] + Ra[3 * r + 2] * a[6];
        const float gb = Rb[3 * r] * b[4] + Rb[3 * r + 1] * b[5] + Rb[3 * r + 2] * b[6];
        g[r] = vf * ga + uf * gb;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[4 + c] = Rq[c] * g[0] + Rq[3 + c] * g[1] + Rq[6 + c] * g[2];
}

// One sensor past the newer of two packets: a the earlier packet's q0 q1 q2 q3 ax ay az, b the newer one's, u > 1; o[7].  The
// quaternion statements are resample_sensor's except above d = 1 - 1e-6: linear weights, which between two packets cost 1e-10, are a
// rate error once u is past 1 (u (u^2 - 1) th^3 / 6: 7e-9 at 0.3 rad/s and 100 Hz), so the arc is taken from the chord |qb - qa|
// and the same two sines are used.  The acceleration is the newer packet's alone, held in the global frame.
__device__ __forceinline__ void predict_sensor(const float* __restrict__ a, const float* __restrict__ b, double u, float* __restrict__ o) {
    float Ra[9], Rb[9];
    const bool ok = q2r<float>(a[0], a[1], a[2], a[3], Ra) && q2r<float>(b[0], b[1], b[2], b[3], Rb);
    if (!ok) {
        resample_nan7(o);
        return;
    }
    const float na = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]);
    const float nb = sqrtf(b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]);
    float qa[4], qb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) qa[j] = a[j] / na, qb[j] = b[j] / nb;
    float dot = qa[0] * qb[0] + qa[1] * qb[1] + qa[2] * qb[2] + qa[3] * qb[3];
    if (dot < 0.f) {
#pragma unroll
        for (int j = 0; j < 4; ++j) qb[j] = -qb[j];
        dot = -dot;
    }
    const double d = (double)dot < 1.0 ? (double)dot : 1.0;
    double th;
    if (d > 1.0 - 1e-6) {                                        // acos cannot tell arcs this short apart: the arc from its chord
        double c2 = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double e = (double)qb[j] - (double)qa[j];
            c2 = c2 + e * e;
        }
        th = 2.0 * asin(0.5 * sqrt(c2));
    } else {
        th = acos(d);
    }
    double w0, w1;
    if (th < rs::TINY_ARC) {                                     // (linear weights are exact to th^3 here, and sin(th) may be 0)
        w0 = 1.0 - u, w1 = u;
    } else {
        const double st = sin(th);
        w0 = sin((1.0 - u) * th) / st, w1 = sin(u * th) / st;
    }
    const float f0 = (float)w0, f1 = (float)w1;
    float q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = f0 * qa[j] + f1 * qb[j];
    float Rq[9];
    if (!q2r<float>(q[0], q[1], q[2], q[3], Rq)) {
        resample_nan7(o);
        return;
    }
    const float nq = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = q[j] / nq;
    float g[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) g[r] = Rb[3 * r] * b[4] + Rb[3 * r + 1] * b[5] + Rb[3 * r + 2] * b[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[4 + c] = Rq[c] * g[0] + Rq[3 + c] * g[1] + Rq[6 + c] * g[2];
}

}  // namespace tip
