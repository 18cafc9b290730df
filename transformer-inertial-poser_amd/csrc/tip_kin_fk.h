// tip_kin_fk.h — the forward-kinematics body of the character, once, for both scalar types: fp32 for tip_kin.hip (the root track, the
// metrics), fp64 for tip_syn.hip (the synthetic IMU readings and SBP labels).  The statements and their order are the same for both,
// so the fp32 instantiation gives the bits tip_kin.hip gave when these functions lived there.
//
//   data_utils.py:262-306      viz_current_frame_and_store_fk_info_include_fixed: base at q[:3] with A2Q(q[3:6]); per link the COM
//                              pose (getLinkState fields 0-1) and the link frame (fields 4-5)
//
// A2Q is fairmotion's, i.e. scipy's Rotation.from_rotvec(a).as_quat(): (x, y, z, w), series below 1e-3 rad, exact at 0.  Q_mult is the
// Hamilton product on (x, y, z, w).
#pragma once
#include "tip_internal.h"

namespace tip {

namespace kn {
constexpr int MAX_LINKS = 32, MAX_BODIES = 33, LANES = 64, COL = 65;      // COL: LDS column stride (odd: the transpose is conflict-free)
constexpr int QDQ = 114, REST = 111, NQ = 57, SBPS = 5;
constexpr double DT = 1.0 / 60;                                           // constants.py:7
}  // namespace kn

// One link of the skeleton table as the device reads it, in either scalar type (include/tip_hip.h has both layouts).
template <typename F>
struct KinLinkT {
    int parent;                  // body index of the parent: 0 the root, i + 1 link i; always below this link's own body index
    int state_col;               // column of the 57-wide q where the link's axis-angle starts, or -1 for a fixed joint
    F jxyz[3], jq[4];            // joint origin in the parent's link frame
    F com[3];                    // inertial origin in the link frame
};
static_assert(sizeof(KinLinkT<float>) == 48 && sizeof(KinLinkT<double>) == 88, "KinLinkT layout");

template <typename F> __device__ __forceinline__ F kin_sqrt(F x) {
    if constexpr (std::is_same<F, float>::value) return sqrtf(x);
    else return sqrt(x);
}

// scipy's from_rotvec(a).as_quat(): exact at angle 0 (x = y = z = 0, w = cos 0 = 1), the series of sin(t / 2) / t below 1e-3 rad.
template <typename F>
__device__ __forceinline__ void a2q(F ax, F ay, F az, F* q) {
    const F t2 = ax * ax + ay * ay + az * az;
    const F t = kin_sqrt<F>(t2);
    F s, w;
    if (t <= F(1e-3)) {
        s = F(0.5) - t2 / F(48) + t2 * t2 / F(3840);
    } else {
        if constexpr (std::is_same<F, float>::value) s = sinf(t * 0.5f) / t;
        else s = sin(t * 0.5) / t;
    }
    if constexpr (std::is_same<F, float>::value) w = cosf(t * 0.5f);
    else w = cos(t * 0.5);
    q[0] = ax * s, q[1] = ay * s, q[2] = az * s, q[3] = w;
}

// Hamilton product, (x, y, z, w)
template <typename F>
__device__ __forceinline__ void qmul(const F* a, const F* b, F* o) {
    const F x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    const F y = a[3] * b[1] - a[0] * b[2] + a[1] * b[3] + a[2] * b[0];
    const F z = a[3] * b[2] + a[0] * b[1] - a[1] * b[0] + a[2] * b[3];
    const F w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = x, o[1] = y, o[2] = z, o[3] = w;
}

// v rotated by the unit quaternion q: v + w t + u x t with t = 2 (u x v); exact for the identity
template <typename F>
__device__ __forceinline__ void qrot(const F* q, const F* v, F* o) {
    const F tx = F(2) * (q[1] * v[2] - q[2] * v[1]), ty = F(2) * (q[2] * v[0] - q[0] * v[2]), tz = F(2) * (q[0] * v[1] - q[1] * v[0]);
    o[0] = v[0] + q[3] * tx + (q[1] * tz - q[2] * ty);
    o[1] = v[1] + q[3] * ty + (q[2] * tx - q[0] * tz);
    o[2] = v[2] + q[3] * tz + (q[0] * ty - q[1] * tx);
}

// The link frames of one pose into this lane's LDS column Fc (Fc[(7 b + c) * COL]): base at (rx, ry, rz) with A2Q(rot[0:3]), a child's
// frame = the parent's frame x the joint origin x A2Q(its axis-angle) (identity for a fixed joint).  rot is q + 3: the 54 rotation
// columns.  A table entry outside its range reads as "root's child" / "fixed" and never as an address.  SCALED: every joint offset is
// multiplied by `scale` first (PyBullet's globalScaling); without it `scale` is not read.
template <typename F, bool SCALED>
__device__ __forceinline__ void fk_frames(const KinLinkT<F>* __restrict__ link, int L, const F* __restrict__ rot, F rx, F ry, F rz, F scale,
                                          F* Fc) {
    F q[4];
    a2q<F>(rot[0], rot[1], rot[2], q);
    Fc[0 * kn::COL] = rx, Fc[1 * kn::COL] = ry, Fc[2 * kn::COL] = rz;
    for (int c = 0; c < 4; ++c) Fc[(3 + c) * kn::COL] = q[c];
    for (int i = 0; i < L; ++i) {
        const KinLinkT<F>& lk = link[i];
        const int b = i + 1;
        const int pa = (lk.parent < 0 || lk.parent >= b) ? 0 : lk.parent;
        F pp[3], pq[4], o[3], qj[4];
        for (int c = 0; c < 3; ++c) pp[c] = Fc[(7 * pa + c) * kn::COL];
        for (int c = 0; c < 4; ++c) pq[c] = Fc[(7 * pa + 3 + c) * kn::COL];
        if constexpr (SCALED) {
            const F js[3] = {lk.jxyz[0] * scale, lk.jxyz[1] * scale, lk.jxyz[2] * scale};
            qrot<F>(pq, js, o);
        } else {
            qrot<F>(pq, lk.jxyz, o);
        }
        qmul<F>(pq, lk.jq, qj);
        const int col = lk.state_col;
        if (col >= 3 && col <= kn::NQ - 3) {
            F qa[4];
            a2q<F>(rot[col - 3], rot[col - 2], rot[col - 1], qa);
            qmul<F>(qj, qa, qj);
        }
        for (int c = 0; c < 3; ++c) Fc[(7 * b + c) * kn::COL] = pp[c] + o[c];
        for (int c = 0; c < 4; ++c) Fc[(7 * b + 3 + c) * kn::COL] = qj[c];
    }
}

// link frames -> COM poses, in place: position += R com (getLinkState fields 0-1; the inertial frames carry no rotation of their own)
template <typename F, bool SCALED>
__device__ __forceinline__ void fk_to_com(const KinLinkT<F>* __restrict__ link, int L, F scale, F* Fc) {
    for (int i = 0; i < L; ++i) {
        const int b = i + 1;
        F q[4], o[3];
        for (int c = 0; c < 4; ++c) q[c] = Fc[(7 * b + 3 + c) * kn::COL];
        if constexpr (SCALED) {
            const F cs[3] = {link[i].com[0] * scale, link[i].com[1] * scale, link[i].com[2] * scale};
            qrot<F>(q, cs, o);
        } else {
            qrot<F>(q, link[i].com, o);
        }
        for (int c = 0; c < 3; ++c) Fc[(7 * b + c) * kn::COL] += o[c];
    }
}

// ---- the fp32 table, carry and FK wrappers of tip_kin.hip and tip_terrain.hip ----------------------------------------------------
// The skeleton table as the device reads it (tip_amd.kinematics.Skeleton.pack writes it; include/tip_hip.h has the layout).
using KinLink = KinLinkT<float>;
struct KinSkel {
    int n_links;
    int sbp[kn::SBPS];           // body indices of lankle, rankle, lwrist, rwrist, root
    int pad[2];
    KinLink link[kn::MAX_LINKS];
};
static_assert(sizeof(KinLink) == 48 && sizeof(KinSkel) == 32 + 48 * kn::MAX_LINKS, "KinSkel layout");

// One sequence's carry between chunks: the corrected root; the corrected poses of the last valid frame with their positions taken
// about that root (pq_prev of the runner = pq + root); and that frame's root-velocity columns, s_rest[54:57].  Those columns are
// the runner's s_t[57:60] AFTER its pose averaging (:165-166 averages s_t[6:], the velocity included), while :159 integrates the
// velocity BEFORE it, so the scan takes it back out: v_t = 2 a_t - a_(t-1) from the second valid frame on, v = a on the first.
struct KinCarry {
    double root[3];
    float pq[kn::MAX_BODIES * 7];
    float vprev[3];
    int has_prev;
    int pad[15];
};
static_assert(sizeof(KinCarry) == 1024, "KinCarry layout");

__device__ __forceinline__ int kin_links(const KinSkel& sk) { return sk.n_links < 0 ? 0 : (sk.n_links > kn::MAX_LINKS ? kn::MAX_LINKS : sk.n_links); }

// the shared FK body (tip_kin_fk.h) in fp32 on this table, unscaled
__device__ __forceinline__ void fk_frames(const KinSkel& sk, int L, const float* __restrict__ rot, float rx, float ry, float rz, float* F) {
    fk_frames<float, false>(sk.link, L, rot, rx, ry, rz, 1.f, F);
}
__device__ __forceinline__ void fk_to_com(const KinSkel& sk, int L, float* F) { fk_to_com<float, false>(sk.link, L, 1.f, F); }

// ... and for a wearer of body scale `scale` (the _scaled entries): every joint and COM offset times `scale` before it is rotated, as
// PyBullet's globalScaling builds a SimAgent(scale=s) (bullet_agent.py:47,67).  SCALED = false is the two wrappers above, statement for
// statement: `scale` is not read and nothing is multiplied by 1.
template <bool SCALED>
__device__ __forceinline__ void fk_frames_of(const KinSkel& sk, int L, const float* __restrict__ rot, float rx, float ry, float rz, float scale,
                                             float* F) {
    if constexpr (SCALED) fk_frames<float, true>(sk.link, L, rot, rx, ry, rz, scale, F);
    else fk_frames(sk, L, rot, rx, ry, rz, F);
}
template <bool SCALED>
__device__ __forceinline__ void fk_to_com_of(const KinSkel& sk, int L, float scale, float* F) {
    if constexpr (SCALED) fk_to_com<float, true>(sk.link, L, scale, F);
    else fk_to_com(sk, L, F);
}

// A body scale the kernels accept: finite and above 0.  Any other makes its sequence's rows NaN and touches nothing else.
__device__ __forceinline__ bool kin_scale_ok(float s) { return s > 0.f && s <= 3.402823466e38f; }

// The kernels of tip_kin.hip and tip_terrain.hip are templates over (SCALED, S...): the scaled instantiation has one parameter more, the
// scale array, as the pack S... = const float*; the unscaled one has an empty pack, i.e. the parameter list it always had.
__device__ __forceinline__ const float* kin_scale_ptr() { return nullptr; }
__device__ __forceinline__ const float* kin_scale_ptr(const float* scale) { return scale; }

}  // namespace tip
