// tip_motion.hip — SMPL pose sequences to nimble_qdq: the ground-truth half of the reference's preprocessing, fp64, one launch over
// R ragged sequences held back to back.
//
//   dip_loader.py:151-181                    the source motion: n frames at fps, one axis-angle per SMPL joint, A2R of each
//   preprocess_DIP_TC_new.py:98-107          the root: (A2R(pose[0:3]), trans[frame]) with `trans`, else (rot_up_R A2R(pose[0:3]),
//                                            (0, 0, root_z_offset)) — constants.py:21-23
//   data_utils.py:103-161                    get_raw_motion_info_nimble_q_dummy_dq: rows at t_0 = 0.0075, t_{k+1} = t_k + DT while
//                                            t_k < (n - 1) / fps, each from the pose at t_k and the root at t_k + DT
//   fairmotion Motion.get_pose_by_time       time clipped to [0, length], frame1 = int(time fps + 1e-5), frame2 = min(frame1 + 1, n - 1),
//                                            alpha = clip((time - t1) / (t2 - t1), 0, 1), R = R1 A2R(alpha R2A(R1^T R2)), p linear
//
// Kernel:
//   motion_qdq_kernel   one lane per (output row, slot); a workgroup covers ROWS rows.  Slot 0 is the root at t_k (p and its
//                       axis-angle), slots 1-17 the spherical joints in output order, slot 18 the root at t_k + DT (v and w, with
//                       slot 0's rotation and position handed over through LDS: the workgroup's one barrier).  Every lane runs the
//                       same straight-line body — two A2R, one relative rotation, its logarithm, A2R of the scaled logarithm, a
//                       product and the logarithm of the result — on 3x3 matrices held in named registers; nothing is indexed
//                       dynamically, so nothing goes to scratch.  The 51 zero columns are written by the whole workgroup.
//                       The tile: 16 rows x 19 slots = 304 lanes (five waves, the last one 48 lanes wide).  The body is a few hundred
//                       fp64 VALU operations and six transcendental calls per lane on 12 doubles read and 3-6 written, so the launch is
//                       bound by the fp64 VALU and not by memory; at 72 VGPRs and no scratch a SIMD keeps seven waves (make
//                       resource-usage), more than the five of a workgroup, and a smaller tile would only add barriers.
//
// The logarithm goes through a quaternion (Shepperd's choice of the largest of trace and diagonal, then atan2): conditioning stays
// O(1) up to pi, where the trace / acos form loses half the digits.  Axis-angles come out with angle in [0, pi].
// The time table is data: the host builds it with np.cumsum (the reference's running sum to the bit) and uploads it.
// Plain HIP C++, vector stores only, no environment.
#include "tip_kin_fk.h"

namespace tip {

namespace mo {
constexpr int JOINTS = 17, SLOTS = JOINTS + 2, ROWS = 16, THREADS = 320;   // 304 lanes at work
constexpr int NQ = kn::NQ, QDQ = kn::QDQ, MIN_LDP = 66, SMPL_USED = 22;
constexpr double ROOT_Z = 0.95;                                           // constants.py:23
constexpr double T_EPS = 1e-5;                                            // get_pose_by_time's frame epsilon
static_assert(3 + 3 * (JOINTS + 1) == NQ && ROWS * SLOTS <= THREADS, "layout");
}  // namespace mo

struct Mat3 {
    double a, b, c, d, e, f, g, h, i;                                     // row-major
};

// scipy's Rotation.from_rotvec(v).as_matrix(): through the quaternion, the small-angle series below 1e-3
__device__ __forceinline__ Mat3 mo_a2r(double vx, double vy, double vz) {
    const double t2 = (vx * vx + vy * vy) + vz * vz;
    const double t = sqrt(t2);
    double s;
    if (t <= 1e-3) s = (0.5 - t2 / 48) + t2 * t2 / 3840;
    else s = sin(t * 0.5) / t;
    double x = s * vx, y = s * vy, z = s * vz, w = cos(t * 0.5);
    const double n = sqrt(((x * x + y * y) + z * z) + w * w);
    x /= n, y /= n, z /= n, w /= n;
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    Mat3 m;
    m.a = x2 - y2 - z2 + w2, m.b = 2 * (xy - zw), m.c = 2 * (xz + yw);
    m.d = 2 * (xy + zw), m.e = -x2 + y2 - z2 + w2, m.f = 2 * (yz - xw);
    m.g = 2 * (xz - yw), m.h = 2 * (yz + xw), m.i = -x2 - y2 + z2 + w2;
    return m;
}

// scipy's Rotation.from_matrix(m).as_rotvec(): Shepperd's quaternion, w made non-negative, angle = 2 atan2(|xyz|, w) in [0, pi]
__device__ __forceinline__ void mo_r2a(const Mat3& m, double& ox, double& oy, double& oz) {
    const double tr = (m.a + m.e) + m.i;
    double x, y, z, w;
    if (tr >= m.a && tr >= m.e && tr >= m.i) {
        x = m.h - m.f, y = m.c - m.g, z = m.d - m.b, w = 1 + tr;
    } else if (m.a >= m.e && m.a >= m.i) {
        x = (1 - tr) + 2 * m.a, y = m.d + m.b, z = m.g + m.c, w = m.h - m.f;
    } else if (m.e >= m.i) {
        x = m.d + m.b, y = (1 - tr) + 2 * m.e, z = m.h + m.f, w = m.c - m.g;
    } else {                                                              // (a NaN matrix ends here and stays NaN)
        x = m.g + m.c, y = m.h + m.f, z = (1 - tr) + 2 * m.i, w = m.d - m.b;
    }
    const double n = sqrt(((x * x + y * y) + z * z) + w * w);
    x /= n, y /= n, z /= n, w /= n;
    if (w < 0) x = -x, y = -y, z = -z, w = -w;
    const double sn = sqrt((x * x + y * y) + z * z);
    const double ang = 2 * atan2(sn, w);
    double s;
    if (ang <= 1e-3) {
        const double a2 = ang * ang;
        s = (2 + a2 / 12) + 7 * a2 * a2 / 2880;
    } else {
        s = ang / sin(ang * 0.5);
    }
    ox = s * x, oy = s * y, oz = s * z;
}

__device__ __forceinline__ Mat3 mo_mul(const Mat3& p, const Mat3& q) {
    Mat3 o;
    o.a = (p.a * q.a + p.b * q.d) + p.c * q.g, o.b = (p.a * q.b + p.b * q.e) + p.c * q.h, o.c = (p.a * q.c + p.b * q.f) + p.c * q.i;
    o.d = (p.d * q.a + p.e * q.d) + p.f * q.g, o.e = (p.d * q.b + p.e * q.e) + p.f * q.h, o.f = (p.d * q.c + p.e * q.f) + p.f * q.i;
    o.g = (p.g * q.a + p.h * q.d) + p.i * q.g, o.h = (p.g * q.b + p.h * q.e) + p.i * q.h, o.i = (p.g * q.c + p.h * q.f) + p.i * q.i;
    return o;
}

__device__ __forceinline__ Mat3 mo_t(const Mat3& p) {
    Mat3 o;
    o.a = p.a, o.b = p.d, o.c = p.g, o.d = p.b, o.e = p.e, o.f = p.h, o.g = p.c, o.h = p.f, o.i = p.i;
    return o;
}

// the sequence whose rows [offsets[s], offsets[s + 1]) hold `row` (0 <= row < offsets[R]; empty sequences are stepped over)
__device__ __forceinline__ int mo_seq_of(const long long* __restrict__ offsets, int R, long long row) {
    int lo = 0, hi = R;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(mo::THREADS) void motion_qdq_kernel(const double* __restrict__ poses, int ldp, const double* __restrict__ trans,
                                                                 const int* __restrict__ has_trans, const long long* __restrict__ in_off,
                                                                 const long long* __restrict__ out_off, const double* __restrict__ fps_seq,
                                                                 int R, long long n_in, long long n_out, const double* __restrict__ times,
                                                                 long long n_times, const int* __restrict__ joints, double* __restrict__ qdq) {
    __shared__ double root[mo::ROWS][12];                             // slot 0's rotation and position, for slot 18 of the same row
    const int tid = threadIdx.x, rl = tid / mo::SLOTS, slot = tid - rl * mo::SLOTS;
    const long long row0 = (long long)blockIdx.x * mo::ROWS, row = row0 + rl;
    const bool live = rl < mo::ROWS && row < n_out;
    const double nan = __builtin_nan("");
    Mat3 Rm = {nan, nan, nan, nan, nan, nan, nan, nan, nan};
    double px = nan, py = nan, pz = nan;
    const bool next = slot == mo::SLOTS - 1, is_root = slot == 0 || next;
    if (live) {
        const int seq = mo_seq_of(out_off, R, row);
        const long long k = row - out_off[seq], a = in_off[seq], n = in_off[seq + 1] - a;
        const double fps = fps_seq[seq];
        int j = joints[is_root ? 0 : slot];
        if (j < 0 || j >= mo::SMPL_USED) j = -1;
        // what cannot be addressed or timed gives a NaN row, never a read outside the arrays
        if (k >= 0 && k < n_times && a >= 0 && n >= 1 && a + n <= n_in && fps > 0 && fps <= 1e9 && j >= 0) {
            const double fps_inv = 1.0 / fps, length = (double)(n - 1) * fps_inv;
            double t = times[k];
            if (next) t = t + kn::DT;
            t = t < 0 ? 0 : (t > length ? length : t);                    // (NaN stays and is caught below)
            const double ff = t * fps + mo::T_EPS;
            long long f1 = ff >= (double)(n - 1) ? n - 1 : (ff >= 0 ? (long long)ff : 0);
            if (!(t == t)) f1 = 0;
            const long long f2 = f1 + 1 < n - 1 ? f1 + 1 : n - 1;
            const double* s1 = poses + (size_t)(a + f1) * ldp + 3 * j;
            const double* s2 = poses + (size_t)(a + f2) * ldp + 3 * j;
            const Mat3 R1 = mo_a2r(s1[0], s1[1], s1[2]);
            const bool with_trans = trans != nullptr && (has_trans == nullptr || has_trans[seq] != 0);
            double alpha = 0.0;
            if (f1 == f2) {
                Rm = R1;
            } else {
                const double t1 = (double)f1 * fps_inv, t2 = (double)f2 * fps_inv;
                alpha = (t - t1) / (t2 - t1);
                alpha = alpha < 0 ? 0 : (alpha > 1 ? 1 : alpha);
                const Mat3 R2 = mo_a2r(s2[0], s2[1], s2[2]);
                double lx, ly, lz;
                mo_r2a(mo_mul(mo_t(R1), R2), lx, ly, lz);
                Rm = mo_mul(R1, mo_a2r(alpha * lx, alpha * ly, alpha * lz));
            }
            if (is_root) {
                if (with_trans) {
                    const double* p1 = trans + (size_t)(a + f1) * 3;
                    const double* p2 = trans + (size_t)(a + f2) * 3;
                    if (f1 == f2) px = p1[0], py = p1[1], pz = p1[2];
                    else px = (1 - alpha) * p1[0] + alpha * p2[0], py = (1 - alpha) * p1[1] + alpha * p2[1], pz = (1 - alpha) * p1[2] + alpha * p2[2];
                    if (!(fabs(px) <= 1.79769313486231570e308)) px = nan;  // an infinite source value reads as NaN
                    if (!(fabs(py) <= 1.79769313486231570e308)) py = nan;
                    if (!(fabs(pz) <= 1.79769313486231570e308)) pz = nan;
                } else {                                                  // rot_up_R = Q2R((.5, .5, .5, .5)) is the row rotation (x, y, z) <- (z, x, y), exact
                    const Mat3 u = Rm;
                    Rm.a = u.g, Rm.b = u.h, Rm.c = u.i, Rm.d = u.a, Rm.e = u.b, Rm.f = u.c, Rm.g = u.d, Rm.h = u.e, Rm.i = u.f;
                    px = 0.0, py = 0.0, pz = mo::ROOT_Z;
                }
            }
        }
        double* o = qdq + (size_t)row * mo::QDQ;
        if (!next) {
            double ax, ay, az;
            mo_r2a(Rm, ax, ay, az);
            o[3 + 3 * slot] = ax, o[4 + 3 * slot] = ay, o[5 + 3 * slot] = az;
            if (slot == 0) {
                o[0] = px, o[1] = py, o[2] = pz;
                double* h = root[rl];
                h[0] = Rm.a, h[1] = Rm.b, h[2] = Rm.c, h[3] = Rm.d, h[4] = Rm.e, h[5] = Rm.f, h[6] = Rm.g, h[7] = Rm.h, h[8] = Rm.i;
                h[9] = px, h[10] = py, h[11] = pz;
            }
        }
    }
    __syncthreads();                                                     // every lane of the workgroup arrives: nothing returned above
    if (live && next) {
        const double* h = root[rl];
        Mat3 R0t;                                                         // the root's rotation at t_k, transposed
        R0t.a = h[0], R0t.b = h[3], R0t.c = h[6], R0t.d = h[1], R0t.e = h[4], R0t.f = h[7], R0t.g = h[2], R0t.h = h[5], R0t.i = h[8];
        double wx, wy, wz;
        mo_r2a(mo_mul(R0t, Rm), wx, wy, wz);
        double* o = qdq + (size_t)row * mo::QDQ + mo::NQ;
        o[0] = (px - h[9]) / kn::DT, o[1] = (py - h[10]) / kn::DT, o[2] = (pz - h[11]) / kn::DT;
        o[3] = wx / kn::DT, o[4] = wy / kn::DT, o[5] = wz / kn::DT;
    }
    constexpr int ZEROS = mo::QDQ - mo::NQ - 6;                           // the joints' velocities: the reference fills zeros
    const long long rows_here = n_out - row0 < mo::ROWS ? n_out - row0 : mo::ROWS;
    for (int e = tid; e < (int)rows_here * ZEROS; e += mo::THREADS) qdq[(size_t)(row0 + e / ZEROS) * mo::QDQ + (mo::NQ + 6) + e % ZEROS] = 0.0;
}

}  // namespace tip

using namespace tip;

extern "C" {

int tip_motion_tile(int* rows, int* slots) {
    if (!rows || !slots) return TIP_ERR_INVALID_ARG;
    *rows = mo::ROWS, *slots = mo::SLOTS;
    return TIP_OK;
}

int tip_motion_qdq(const double* poses, int ldp, const double* trans, const int* has_trans, const long long* in_offsets,
                   const long long* out_offsets, const double* fps, int count, long long n_in, long long n_out, const double* times,
                   long long n_times, const int* joints, double* qdq, tip_stream_t stream) {
    if (tip_bad_count(count) || tip_bad_rows(n_in) || tip_bad_rows(n_out) || tip_bad_rows(n_times) || ldp < mo::MIN_LDP)
        return TIP_ERR_INVALID_ARG;
    if (count > 0 && (!in_offsets || !out_offsets || !fps)) return TIP_ERR_INVALID_ARG;
    if (n_in > 0 && !poses) return TIP_ERR_INVALID_ARG;
    if (n_out > 0 && (!qdq || !times || !joints || !poses || count == 0 || n_in == 0 || n_times == 0)) return TIP_ERR_INVALID_ARG;
    if (has_trans && !trans) return TIP_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(poses) % 8 || reinterpret_cast<uintptr_t>(trans) % 8 || reinterpret_cast<uintptr_t>(qdq) % 8
        || reinterpret_cast<uintptr_t>(times) % 8 || reinterpret_cast<uintptr_t>(fps) % 8)
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_out == 0) return TIP_OK;
    hipLaunchKernelGGL(motion_qdq_kernel, dim3((unsigned)((n_out + mo::ROWS - 1) / mo::ROWS)), dim3(mo::THREADS), 0,
                       static_cast<hipStream_t>(stream), poses, ldp, trans, has_trans, in_offsets, out_offsets, fps, count, n_in, n_out,
                       times, n_times, joints, qdq);
    return tip_launch_status();
}

}  // extern "C"
