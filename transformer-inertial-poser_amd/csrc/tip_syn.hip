// tip_syn.hip — synthetic IMU readings and stationary-body-point (SBP) labels from pose sequences: the reference's offline data
// generator (data-gen-and-viz-bullet-new.py) as a handful of launches over R ragged sequences held back to back, fp64 end to end.
//
//   data-gen-and-viz-bullet-new.py:44-73     get_raw_motion_info: per frame the root's tracked point p + Q2R(Q) ROOT_COM_OFFSET with the
//                                            root's orientation, every other body's COM pose (getLinkState fields 0-1)
//   :147-218                                 get_imu_readings_from_raw_motion_info: six Q2R matrices, six centred second differences
//                                            over +-4 frames, the first and last four rows copied from their neighbours
//   :76-144, data_utils.py:27-100            get_link_contr_seq_from_raw_motion_info over get_rot_center_sample_based: per frame and
//                                            body the candidate point of least residue, chained through the previous solution
//   bullet_agent.py:47-78, 381-390           scale: globalScaling of every joint and COM offset, ref_scale on the root translation
//
// Kernels:
//   syn_pose_kernel     one lane per row, as kin_fk_kernel: the shared FK body (tip_kin_fk.h) in fp64 on the fp64 table, the sequence's
//                       scale on the offsets and the root xyz; only the eight tracked poses leave
//   syn_imu_kernel      one lane per (row, IMU body); the padding rows by clamping the row index into the sequence's own rows
//   syn_frame_kernel    one lane per (row, SBP body): R, w, v of that row's search from the tracked poses of rows t - 1 and t + 1 — what
//                       does not depend on the previous solution and is the same for every candidate, taken out of the chain
//                       (profiles/syn/syn_ab.txt: the SBP stage 37.4 -> 32.3 ms on 64 x 3000 frames, the same bits)
//   syn_sbp_kernel      the hot path.  One workgroup per (sequence, SBP body), frames in order.  A lane keeps its PTS candidate points
//                       in registers for the whole sequence; per frame every lane reads the row's 15 doubles (uniform loads, the next
//                       frame's issued a frame ahead), scores its points, and the workgroup takes the argmin on (residue, index),
//                       lowest index first: a butterfly inside the wave, then one LDS slot per wave, double-buffered by frame parity
//                       so that a frame costs ONE barrier.  A NaN residue never wins a comparison; if nothing finite is below
//                       V_THRES the flag is 0 and the chain restarts.
//
// Every wait is a workgroup barrier; nothing waits on another workgroup.  Plain HIP C++, vector stores only, no environment.
// The candidate grids are data: the host builds the three axes per body class with the reference's np.arange expressions and uploads
// them (SynGrid); nothing here regenerates them.
#include "tip_kin_fk.h"

namespace tip {

namespace sy {
constexpr int TRACKED = 8, IMUS = 6, AXIS = 40, CLASSES = 3;
constexpr int ACC_N = 4;                                                  // constants.py:8
constexpr double DT2 = 2 * kn::DT;                                        // the labels' dt (:129)
constexpr double DT_FIN_ACC = kn::DT * ACC_N;                             // constants.py:9
constexpr double V_THRES = 0.15;                                          // constants.py:12
constexpr size_t POSE_LDS = (size_t)kn::MAX_BODIES * 7 * kn::COL * sizeof(double);
}  // namespace sy

// The fp64 skeleton table (tip_amd.syndata writes it; include/tip_hip.h, "synthetic data", has the layout).
struct SynSkel {
    int n_links;
    int sbp[kn::SBPS];           // body indices of lankle, rankle, lwrist, rwrist, root
    int imu[sy::IMUS];           // body indices of root, lwrist, rwrist, lknee, rknee, upperneck
    int pad[4];
    KinLinkT<double> link[kn::MAX_LINKS];
};
static_assert(sizeof(SynSkel) == 64 + 88 * kn::MAX_LINKS, "SynSkel layout");

// One body class's candidate grid: point i = (axis[0][ix], axis[1][iy], axis[2][iz]) with i = (iy n[0] + ix) n[2] + iz, which is
// np.meshgrid(lp_x, lp_y, lp_z) ravelled (data_utils.py:70-71).  The grid table is three of these: feet, wrists, pelvis.
struct SynGrid {
    int n[3];
    int pad;
    double axis[3][sy::AXIS];
};
static_assert(sizeof(SynGrid) == 16 + 3 * sy::AXIS * 8, "SynGrid layout");

// scipy's Rotation.from_quat(q).as_matrix(): q normalised first, row-major
__device__ __forceinline__ void q2r(const double* qq, double* m) {
    const double n = sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
    const double x = qq[0] / n, y = qq[1] / n, z = qq[2] / n, w = qq[3] / n;
    const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
    const double xy = x * y, zw = z * w, xz = x * z, yw = y * w, yz = y * z, xw = x * w;
    m[0] = x2 - y2 - z2 + w2, m[1] = 2 * (xy - zw), m[2] = 2 * (xz + yw);
    m[3] = 2 * (xy + zw), m[4] = -x2 + y2 - z2 + w2, m[5] = 2 * (yz - xw);
    m[6] = 2 * (xz - yw), m[7] = 2 * (yz + xw), m[8] = -x2 - y2 + z2 + w2;
}

// the sequence whose rows [offsets[s], offsets[s + 1]) hold `row` (0 <= row < offsets[R]; empty sequences are stepped over)
__device__ __forceinline__ int syn_seq_of(const long long* __restrict__ offsets, int R, long long row) {
    int lo = 0, hi = R;                                              // offsets[lo] <= row < offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int syn_body(int b, int L) { return (b < 0 || b > L) ? 0 : b; }

__global__ __launch_bounds__(64) void syn_pose_kernel(const SynSkel* __restrict__ skp, const double* __restrict__ q, int ldq,
                                                      const long long* __restrict__ offsets, int R, const double* __restrict__ scale,
                                                      long long n, double* __restrict__ P) {
    extern __shared__ double syn_Fs[];                              // [MAX_BODIES * 7][COL]: one column per lane
    const SynSkel& sk = *skp;
    const int L = sk.n_links < 0 ? 0 : (sk.n_links > kn::MAX_LINKS ? kn::MAX_LINKS : sk.n_links), lane = threadIdx.x;
    const long long row = (long long)blockIdx.x * kn::LANES + lane;
    if (row >= n) return;                                            // (no barrier below: a lane reads only its own column)
    const double s = scale[syn_seq_of(offsets, R, row)];
    const double* qr = q + (size_t)row * ldq;
    double* Fc = syn_Fs + lane;
    fk_frames<double, true>(sk.link, L, qr + 3, qr[0] * s, qr[1] * s, qr[2] * s, s, Fc);
    double root_p[3], root_q[4];                                     // the base pose, before the COM step (which leaves body 0 alone)
    for (int c = 0; c < 3; ++c) root_p[c] = Fc[c * kn::COL];
    for (int c = 0; c < 4; ++c) root_q[c] = Fc[(3 + c) * kn::COL];
    fk_to_com<double, true>(sk.link, L, s, Fc);
    double* o = P + (size_t)row * (sy::TRACKED * 7);
    for (int k = 0; k < sy::TRACKED; ++k) {
        const int b = syn_body(k < kn::SBPS ? sk.sbp[k] : sk.imu[k - 2], L);
        if (b == 0) {                                                // p + Q2R(Q) ROOT_COM_OFFSET, the offset (0, 0.1, -0.1) unscaled
            double m[9];
            q2r(root_q, m);
            o[7 * k + 0] = root_p[0] + ((m[0] * 0.0 + m[1] * 0.1) + m[2] * -0.1);
            o[7 * k + 1] = root_p[1] + ((m[3] * 0.0 + m[4] * 0.1) + m[5] * -0.1);
            o[7 * k + 2] = root_p[2] + ((m[6] * 0.0 + m[7] * 0.1) + m[8] * -0.1);
            for (int c = 0; c < 4; ++c) o[7 * k + 3 + c] = root_q[c];
        } else {
            for (int c = 0; c < 7; ++c) o[7 * k + c] = Fc[(7 * b + c) * kn::COL];
        }
    }
}

__global__ __launch_bounds__(256) void syn_imu_kernel(const double* __restrict__ P, const long long* __restrict__ offsets, int R,
                                                      long long n, double* __restrict__ imu) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * sy::IMUS) return;
    const long long row = idx / sy::IMUS;
    const int j = (int)(idx - row * sy::IMUS);
    const int slot = j == 0 ? 4 : (j < 3 ? j + 1 : j + 2);           // root, lwrist, rwrist are SBP slots 4, 2, 3; the rest follow them
    const int seq = syn_seq_of(offsets, R, row);
    const long long a = offsets[seq], b = offsets[seq + 1];
    const double* p = P + (size_t)row * (sy::TRACKED * 7) + 7 * slot;
    double m[9];
    q2r(p + 3, m);
    double* o = imu + (size_t)row * 72;
    for (int c = 0; c < 9; ++c) o[9 * j + c] = m[c];
    const double nan = __builtin_nan("");
    double acc[3] = {nan, nan, nan};
    if (b - a >= 2 * sy::ACC_N + 1 && a >= 0 && b <= n) {                                // rows 0-3 copy row 4, rows L-4 .. L-1 copy row L-5 (:215-216)
        long long t = row < a + sy::ACC_N ? a + sy::ACC_N : row;
        if (t > b - sy::ACC_N - 1) t = b - sy::ACC_N - 1;
        const double* cur = P + (size_t)t * (sy::TRACKED * 7) + 7 * slot;
        const double* nxt = cur + (size_t)sy::ACC_N * (sy::TRACKED * 7);
        const double* prv = cur - (size_t)sy::ACC_N * (sy::TRACKED * 7);
        for (int c = 0; c < 3; ++c) acc[c] = ((-2 * cur[c] + nxt[c]) + prv[c]) / (sy::DT_FIN_ACC * sy::DT_FIN_ACC);
    }
    for (int c = 0; c < 3; ++c) o[54 + 3 * j + c] = acc[c];
}

// what a frame of a chain needs from its two neighbouring poses, the same in every lane
struct SynFrame {
    double R[9], w[3], v[3];
};

__device__ __forceinline__ void syn_frame(const double* p1, const double* p2, SynFrame& f) {
    for (int c = 0; c < 3; ++c) f.v[c] = (p2[c] - p1[c]) / sy::DT2;
    const double* q1 = p1 + 3;
    const double* q2 = p2 + 3;
    double dq[4], sq[4], sub[4], cj[4], dori[4], nd = 0.0, ns = 0.0;
    for (int c = 0; c < 4; ++c) {
        dq[c] = q2[c] - q1[c], sq[c] = q2[c] + q1[c];
        nd += dq[c] * dq[c], ns += sq[c] * sq[c];
    }
    const bool minus = sqrt(nd) < sqrt(ns);
    for (int c = 0; c < 4; ++c) sub[c] = minus ? dq[c] : sq[c];
    cj[0] = -q2[0], cj[1] = -q2[1], cj[2] = -q2[2], cj[3] = q2[3];
    qmul<double>(sub, cj, dori);
    for (int c = 0; c < 3; ++c) f.w[c] = 2 * dori[c] / sy::DT2;
    q2r(q2, f.R);
}

__device__ __forceinline__ void syn_frame_load(const double* __restrict__ o, SynFrame& f) {
    for (int c = 0; c < 9; ++c) f.R[c] = o[c];
    for (int c = 0; c < 3; ++c) f.w[c] = o[9 + c], f.v[c] = o[12 + c];
}

// frame-parallel form of syn_frame: one lane per (row, SBP slot), F[row, slot] = the 15 doubles R, w, v of the search at that row
__global__ __launch_bounds__(256) void syn_frame_kernel(const double* __restrict__ P, const long long* __restrict__ offsets, int R,
                                                        long long n, double* __restrict__ F) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * kn::SBPS) return;
    const long long row = idx / kn::SBPS;
    const int b = (int)(idx - row * kn::SBPS);
    const int seq = syn_seq_of(offsets, R, row);
    const long long a = offsets[seq], e = offsets[seq + 1];
    if (a < 0 || e > n || row - a < 2 || row >= e - 2) return;        // rows without a search are never read
    constexpr int STRIDE = sy::TRACKED * 7;
    double p1[7], p2[7];
    for (int c = 0; c < 7; ++c) p1[c] = P[(size_t)(row - 1) * STRIDE + 7 * b + c], p2[c] = P[(size_t)(row + 1) * STRIDE + 7 * b + c];
    SynFrame f;
    syn_frame(p1, p2, f);
    double* o = F + (size_t)idx * 15;
    for (int c = 0; c < 9; ++c) o[c] = f.R[c];
    for (int c = 0; c < 3; ++c) o[9 + c] = f.w[c], o[12 + c] = f.v[c];
}

template <int THREADS, int PTS>
__global__ __launch_bounds__(THREADS) void syn_sbp_kernel(const SynGrid* __restrict__ grids, int cls, int body0, int n_bodies,
                                                          const long long* __restrict__ offsets, long long n,
                                                          const double* __restrict__ Fr, double* __restrict__ constrs) {
    constexpr int WAVES = THREADS / 64;
    __shared__ double ax[3][sy::AXIS];
    __shared__ double red_r[2][WAVES];
    __shared__ int red_i[2][WAVES];
    const int tid = threadIdx.x;
    const int seq = blockIdx.x / n_bodies, body = body0 + blockIdx.x % n_bodies;      // body: SBP slot = tracked slot
    const long long a = offsets[seq], b = offsets[seq + 1];
    const long long len = b - a;
    if (len <= 0 || a < 0 || b > n) return;                          // (uniform over the workgroup; offsets outside the rows address nothing)
    const SynGrid& g = grids[cls];
    int nn[3];
    for (int k = 0; k < 3; ++k) nn[k] = g.n[k] < 1 ? 1 : (g.n[k] > sy::AXIS ? sy::AXIS : g.n[k]);
    const int cap = THREADS * PTS;
    const int npts = nn[0] * nn[1] * nn[2] < cap ? nn[0] * nn[1] * nn[2] : cap;
    for (int e = tid; e < 3 * sy::AXIS; e += THREADS) ax[e / sy::AXIS][e % sy::AXIS] = g.axis[e / sy::AXIS][e % sy::AXIS];
    double* out = constrs + (size_t)a * 20 + 4 * body;
    if (len < 5) {                                                   // (the host refuses L < 9) no row has both neighbours' neighbours
        for (long long e = tid; e < len * 4; e += THREADS) out[(e / 4) * 20 + (e % 4)] = 0.0;
        return;
    }
    if (tid < 16) {                                                  // rows 0, 1, L - 2, L - 1 stay zero (:113, :123)
        const long long r = (tid / 4) < 2 ? (tid / 4) : len - 4 + (tid / 4);
        out[r * 20 + (tid % 4)] = 0.0;
    }
    __syncthreads();
    double px[PTS], py[PTS], pz[PTS];
#pragma unroll
    for (int k = 0; k < PTS; ++k) {
        const int i = tid + k * THREADS;
        const int ii = i < npts ? i : 0;
        const int iz = ii % nn[2], ixy = ii / nn[2];
        px[k] = ax[0][ixy % nn[0]], py[k] = ax[1][ixy / nn[0]], pz[k] = ax[2][iz];
    }
    const double* Fb = Fr + ((size_t)a * kn::SBPS + body) * 15;
    SynFrame f, fn;                                                  // this frame's R, w, v and, loaded a frame ahead, the next one's
    syn_frame_load(Fb + (size_t)2 * kn::SBPS * 15, fn);
    bool has_prev = false;
    double rp[3] = {0.0, 0.0, 0.0};
    for (long long t = 2; t < len - 2; ++t) {
        f = fn;
        const long long tn = t + 1 < len - 2 ? t + 1 : t;               // the last frame reloads itself
        syn_frame_load(Fb + (size_t)tn * kn::SBPS * 15, fn);
        double cen[3];
        for (int c = 0; c < 3; ++c) cen[c] = rp[c] - f.v[c] * sy::DT2;
        double best = __builtin_inf();
        int besti = 0x7fffffff;
#pragma unroll
        for (int k = 0; k < PTS; ++k) {
            const double r0 = (f.R[0] * px[k] + f.R[1] * py[k]) + f.R[2] * pz[k];
            const double r1 = (f.R[3] * px[k] + f.R[4] * py[k]) + f.R[5] * pz[k];
            const double r2 = (f.R[6] * px[k] + f.R[7] * py[k]) + f.R[8] * pz[k];
            const double l0 = (f.w[1] * r2 - f.w[2] * r1) + f.v[0];
            const double l1 = (f.w[2] * r0 - f.w[0] * r2) + f.v[1];
            const double l2 = (f.w[0] * r1 - f.w[1] * r0) + f.v[2];
            double res = sqrt((l0 * l0 + l1 * l1) + l2 * l2);
            if (has_prev) {
                const double d0 = r0 - cen[0], d1 = r1 - cen[1], d2 = r2 - cen[2];
                res = res + 0.2 * sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            }
            res = res + 0.02 * sqrt((r0 * r0 + r1 * r1) + r2 * r2);
            const int i = tid + k * THREADS;
            // np.argmin answers the first NaN and NaN < V_THRES is false: flag 0.  Here a NaN never wins, which gives the same flags:
            // R, w, v and the previous solution are the same for every candidate and the grid is finite, so a frame's residues are all
            // NaN or none is — except inf x 0 beside inf, where the others are +inf and the minimum is not below V_THRES either.
            if (i < npts && res < best) best = res, besti = i;       // ascending i within the lane: the first minimum stays
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {                           // butterfly: every lane of the wave ends with the wave's best
            const double orr = __shfl_xor(best, m, 64);
            const int oi = __shfl_xor(besti, m, 64);
            if (orr < best || (orr == best && oi < besti)) best = orr, besti = oi;
        }
        if constexpr (WAVES > 1) {
            const int buf = (int)(t & 1);
            if ((tid & 63) == 0) red_r[buf][tid >> 6] = best, red_i[buf][tid >> 6] = besti;
            __syncthreads();                                         // the frame's one barrier; the other parity is next frame's
            best = red_r[buf][0], besti = red_i[buf][0];
#pragma unroll
            for (int wv = 1; wv < WAVES; ++wv) {
                const double orr = red_r[buf][wv];
                const int oi = red_i[buf][wv];
                if (orr < best || (orr == best && oi < besti)) best = orr, besti = oi;
            }
        }
        has_prev = best < sy::V_THRES && besti < npts;               // an all-NaN or infinite frame: no solution, the chain restarts
        if (has_prev) {
            const int iz = besti % nn[2], ixy = besti / nn[2];
            const double x = ax[0][ixy % nn[0]], y = ax[1][ixy / nn[0]], z = ax[2][iz];
            rp[0] = (f.R[0] * x + f.R[1] * y) + f.R[2] * z;
            rp[1] = (f.R[3] * x + f.R[4] * y) + f.R[5] * z;
            rp[2] = (f.R[6] * x + f.R[7] * y) + f.R[8] * z;
        }
        if (tid < 4) out[t * 20 + tid] = !has_prev ? 0.0 : (tid == 0 ? 1.0 : rp[tid - 1]);
    }
}

}  // namespace tip

using namespace tip;

extern "C" {


int tip_syn_skel_bytes(size_t* bytes) {
    if (!bytes) return TIP_ERR_INVALID_ARG;
    *bytes = sizeof(SynSkel);
    return TIP_OK;
}

int tip_syn_grid_bytes(size_t* bytes) {
    if (!bytes) return TIP_ERR_INVALID_ARG;
    *bytes = sy::CLASSES * sizeof(SynGrid);
    return TIP_OK;
}

int tip_syn_poses(const void* skel, const double* q, int ldq, const long long* offsets, int count, const double* scale, long long n,
                  double* poses, tip_stream_t stream) {
    if (!skel || tip_bad_count(count) || tip_bad_rows(n) || ldq < kn::NQ) return TIP_ERR_INVALID_ARG;
    if (n > 0 && (!q || !offsets || !scale || !poses || count == 0)) return TIP_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(skel) % 8 || reinterpret_cast<uintptr_t>(q) % 8 || reinterpret_cast<uintptr_t>(poses) % 8)
        return TIP_ERR_INVALID_ARG;
    if (n == 0) return TIP_OK;
    // 120 KB of dynamic LDS needs the opt-in, and the attribute belongs to the current device: set on every call (it is cheap)
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(syn_pose_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sy::POSE_LDS)
        != hipSuccess)
        return TIP_ERR_HIP;
    hipLaunchKernelGGL(syn_pose_kernel, dim3((unsigned)((n + kn::LANES - 1) / kn::LANES)), dim3(kn::LANES), sy::POSE_LDS,
                       static_cast<hipStream_t>(stream), static_cast<const SynSkel*>(skel), q, ldq, offsets, count, scale, n, poses);
    return tip_launch_status();
}

int tip_syn_imu(const double* poses, const long long* offsets, int count, long long n, double* imu, tip_stream_t stream) {
    if (tip_bad_count(count) || tip_bad_rows(n)) return TIP_ERR_INVALID_ARG;
    if (n > 0 && (!poses || !offsets || !imu || count == 0)) return TIP_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(poses) % 8 || reinterpret_cast<uintptr_t>(imu) % 8) return TIP_ERR_INVALID_ARG;
    if (n == 0) return TIP_OK;
    hipLaunchKernelGGL(syn_imu_kernel, dim3((unsigned)((n * sy::IMUS + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), poses,
                       offsets, count, n, imu);
    return tip_launch_status();
}

int tip_syn_sbp(const void* grids, const double* poses, const long long* offsets, int count, long long n, double* frames,
                double* constrs, tip_stream_t stream) {
    if (tip_bad_count(count) || tip_bad_rows(n)) return TIP_ERR_INVALID_ARG;
    if (n > 0 && (!grids || !poses || !offsets || !frames || !constrs || count == 0)) return TIP_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(grids) % 8 || reinterpret_cast<uintptr_t>(poses) % 8 || reinterpret_cast<uintptr_t>(constrs) % 8
        || reinterpret_cast<uintptr_t>(frames) % 8)
        return TIP_ERR_INVALID_ARG;
    if (n == 0) return TIP_OK;
    const SynGrid* g = static_cast<const SynGrid*>(grids);
    hipStream_t s = static_cast<hipStream_t>(stream);
    // SBP slots 0-1 (feet): 9 x 6 x 33 = 1782 points on 256 lanes; 2-3 (wrists): 5^3 = 125 on 64; 4 (pelvis): 31 x 25 x 8 = 6200 on 256.
    // The pelvis chains are the longest, so they start first.
    hipLaunchKernelGGL(syn_frame_kernel, dim3((unsigned)((n * kn::SBPS + 255) / 256)), dim3(256), 0, s, poses, offsets, count, n, frames);
    hipLaunchKernelGGL((syn_sbp_kernel<256, 25>), dim3(count), dim3(256), 0, s, g, 2, 4, 1, offsets, n, frames, constrs);
    hipLaunchKernelGGL((syn_sbp_kernel<256, 7>), dim3(2 * count), dim3(256), 0, s, g, 0, 0, 2, offsets, n, frames, constrs);
    hipLaunchKernelGGL((syn_sbp_kernel<64, 2>), dim3(2 * count), dim3(64), 0, s, g, 1, 2, 2, offsets, n, frames, constrs);
    return tip_launch_status();
}

}  // extern "C"
