// tip_kin.hip — forward kinematics of the character, the root track with its stationary-body-point (SBP) correction, and the
// evaluation script's seven metrics: what the reference does through PyBullet on the host, as consumers of the streaming engines'
// outputs.  Nothing here feeds back into the model (simple_transformer_with_state.py:75 zeroes the root translation), so none of it
// is inside an engine's frame: the replay post-pass and the live per-frame launch are the same kernel on different chunks.
//
//   data_utils.py:262-306      viz_current_frame_and_store_fk_info_include_fixed: base at q[:3] with A2Q(q[3:6]); per link the COM
//                              pose (getLinkState fields 0-1) and the link frame (fields 4-5)
//   real_time_runner_minimal.py:159-194   root_pre = root + v DT; FK; residues of the active SBPs against the previous frame's
//                              corrected poses; clip; the flat-ground z rule; root, SBP locations and poses shifted by -vel_res DT
//   data_utils.py:397-412, 473-548        get_residue_from_contr, get_cur_step_root_correction_from_all_constr
//   data_utils.py:314-391, offline_testing_simple.py:422-445   the seven metrics over rows start .. L - end - 1
//
// A2Q is fairmotion's, i.e. scipy's Rotation.from_rotvec(a).as_quat(): (x, y, z, w), series below 1e-3 rad, exact at 0.  Q_mult is the
// Hamilton product on (x, y, z, w).
//
// Kernels:
//   kin_fk_kernel       one lane per pose, link frames in LDS (one column per lane, root first, parents before children), fp32;
//                       the workgroup's rows leave through LDS so that the 7-float poses are written coalesced
//   kin_reset_kernel    one lane per listed slot: carry = (s_init[:3], FK(s_init) about the root)
//   kin_track_kernel    one wave per sequence: 64 rows of FK in parallel (root at the origin: FK does not depend on the root, and the
//                       scan only ever adds a root to a pose), then lane 0 steps through those rows in fp64, then the next 64
//   kin_metrics_kernel  one workgroup per file over the two FK'd trajectories, fp64 sums, a fixed-order tree reduction
//
// PRECISION.  FK is fp32.  The scan — root accumulator, residues, clip, z rule — is fp64 on the fp32 poses, and the carry keeps the
// root as fp64; outputs are rounded to fp32 once.  The metrics are fp64 on the fp32 poses.
//
// Nothing waits on another workgroup; a carry block is written by the one wave whose sequence names it.
#include "tip_kin_fk.h"      // KinLinkT, a2q, qmul, qrot, fk_frames, fk_to_com: one body for fp32 (here) and fp64 (tip_syn.hip);
                             // KinSkel, KinCarry and the fp32 FK wrappers, which tip_terrain.hip reads too

namespace tip {

// rows [first, first + cnt) of out[n, L + 1, 7] from the LDS columns 0 .. cnt - 1, consecutive lanes on consecutive floats
__device__ __forceinline__ void fk_store(const float* F, int per, long long first, int cnt, float* __restrict__ out, int lane) {
    float* o = out + (size_t)first * per;
    for (int e = lane; e < cnt * per; e += kn::LANES) {
        const int r = e / per, c = e - r * per;
        o[e] = F[c * kn::COL + r];
    }
}

__global__ __launch_bounds__(64) void kin_fk_kernel(const KinSkel* __restrict__ skp, const float* __restrict__ q, int ldq, long long n,
                                                    float* __restrict__ pq_g, float* __restrict__ pq_jf) {
    __shared__ float Fs[kn::MAX_BODIES * 7 * kn::COL];
    const KinSkel& sk = *skp;
    const int L = kin_links(sk), lane = threadIdx.x, per = (L + 1) * 7;
    const long long first = (long long)blockIdx.x * kn::LANES;
    const long long left = n - first;
    const int cnt = left < kn::LANES ? (int)left : kn::LANES;
    float* F = Fs + lane;
    if (lane < cnt) {
        const float* row = q + (size_t)(first + lane) * ldq;
        fk_frames(sk, L, row + 3, row[0], row[1], row[2], F);
    }
    __syncthreads();
    if (pq_jf) fk_store(Fs, per, first, cnt, pq_jf, lane);
    __syncthreads();
    if (lane < cnt) fk_to_com(sk, L, F);
    __syncthreads();
    fk_store(Fs, per, first, cnt, pq_g, lane);
}

__global__ __launch_bounds__(64) void kin_reset_kernel(const KinSkel* __restrict__ skp, KinCarry* __restrict__ carry, int n_slots,
                                                       const int* __restrict__ slots, int count, const float* __restrict__ s_init) {
    __shared__ float Fs[kn::MAX_BODIES * 7 * kn::COL];
    const KinSkel& sk = *skp;
    const int L = kin_links(sk), lane = threadIdx.x;
    const int j = blockIdx.x * kn::LANES + lane;
    if (j >= count) return;
    const int slot = slots ? slots[j] : j;
    if (slot < 0 || slot >= n_slots) return;
    float* F = Fs + lane;
    const float* row = s_init + (size_t)j * kn::QDQ;
    fk_frames(sk, L, row + 3, 0.f, 0.f, 0.f, F);
    fk_to_com(sk, L, F);
    KinCarry& c = carry[slot];
    for (int k = 0; k < 3; ++k) c.root[k] = (double)row[k], c.vprev[k] = 0.f;
    c.has_prev = 0;
    for (int e = 0; e < (L + 1) * 7; ++e) c.pq[e] = F[e * kn::COL];
}

// np.clip(v, -m, m): a NaN stays a NaN
__device__ __forceinline__ double clip_nan_transparent_d(double v, double m) { return v < -m ? -m : (v > m ? m : v); }

__global__ __launch_bounds__(64) void kin_track_kernel(const KinSkel* __restrict__ skp, KinCarry* __restrict__ carry, int n_slots,
                                                       const int* __restrict__ slots, const long long* __restrict__ begin,
                                                       const long long* __restrict__ end, long long n_rows,
                                                       const float* __restrict__ s_rest, const float* __restrict__ c_t, int nc,
                                                       const unsigned char* __restrict__ valid, float* __restrict__ root_out,
                                                       float* __restrict__ viz_out) {
    __shared__ float Fs[kn::MAX_BODIES * 7 * kn::COL];
    __shared__ int last_s;
    const KinSkel& sk = *skp;
    const int L = kin_links(sk), lane = threadIdx.x, per = (L + 1) * 7;
    const int seq = blockIdx.x;
    const int slot = slots ? slots[seq] : seq;
    if (slot < 0 || slot >= n_slots) return;                      // (uniform over the wave: every return below is)
    long long r0 = begin[seq], r1 = end[seq];
    if (r0 < 0) r0 = 0;
    if (r1 > n_rows) r1 = n_rows;
    if (r1 <= r0) return;
    KinCarry& cr = carry[slot];
    const int n_sbps = nc / 4;
    int body[kn::SBPS];
    for (int i = 0; i < kn::SBPS; ++i) body[i] = (sk.sbp[i] < 0 || sk.sbp[i] > L) ? 0 : sk.sbp[i];
    float* F = Fs + lane;

    // lane 0's scan state: the corrected root, and the previous valid frame's SBP-body poses about it
    double root[3] = {0.0, 0.0, 0.0};
    float x1r[2][3], q1[2][4], vprev[3] = {0.f, 0.f, 0.f};
    int has_prev = 0;
    if (lane == 0) {
        for (int k = 0; k < 3; ++k) root[k] = cr.root[k], vprev[k] = cr.vprev[k];
        has_prev = cr.has_prev;
        for (int i = 0; i < 2; ++i) {
            for (int k = 0; k < 3; ++k) x1r[i][k] = cr.pq[7 * body[i] + k];
            for (int k = 0; k < 4; ++k) q1[i][k] = cr.pq[7 * body[i] + 3 + k];
        }
    }
    for (long long t0 = r0; t0 < r1; t0 += kn::LANES) {
        const long long left = r1 - t0;
        const int cnt = left < kn::LANES ? (int)left : kn::LANES;
        if (lane == 0) last_s = -1;
        if (lane < cnt && (!valid || valid[t0 + lane])) {
            fk_frames(sk, L, s_rest + (size_t)(t0 + lane) * kn::REST, 0.f, 0.f, 0.f, F);
            fk_to_com(sk, L, F);
        }
        __syncthreads();
        if (lane == 0) {
            int last = -1;
            for (int j = 0; j < cnt; ++j) {
                const size_t row = (size_t)(t0 + j);
                float* ro = root_out + row * 3;
                float* vo = viz_out + row * 15;
                if (valid && !valid[row]) {                          // what the runner returns while it primes: the carry's root, 100s
                    for (int k = 0; k < 3; ++k) ro[k] = (float)root[k];
                    for (int k = 0; k < 15; ++k) vo[k] = 100.f;
                    continue;
                }
                const float* sr = s_rest + row * kn::REST;
                const float* ct = c_t + row * nc;
                double pre[3], cl[kn::SBPS][3], res[2][3];
                for (int k = 0; k < 3; ++k) {                        // :159, on the velocity from before the averaging
                    const double v = has_prev ? 2.0 * (double)sr[54 + k] - (double)vprev[k] : (double)sr[54 + k];
                    pre[k] = root[k] + v * kn::DT;
                }
                for (int i = 0; i < kn::SBPS; ++i)
                    for (int k = 0; k < 3; ++k) cl[i][k] = 100.0;
                const double nan = __builtin_nan("");
                for (int i = 0; i < 2; ++i)
                    for (int k = 0; k < 3; ++k) res[i][k] = nan;
                for (int i = 0; i < n_sbps; ++i) {
                    if (ct[4 * i] == 0.f) continue;                  // inactive: location 100, residue NaN
                    double x2[3], sol[3];
                    for (int k = 0; k < 3; ++k) {
                        x2[k] = (double)Fs[(7 * body[i] + k) * kn::COL + j] + pre[k];
                        sol[k] = (double)ct[4 * i + 1 + k];
                        cl[i][k] = x2[k] + sol[k];
                    }
                    if (i >= 2) continue;                            // only the two feet correct the root (:517-520)
                    double q2[4], dq[4], sq[4], sub[4], cj[4], dori[4];
                    double nd = 0.0, ns = 0.0;
                    for (int k = 0; k < 4; ++k) {
                        q2[k] = (double)Fs[(7 * body[i] + 3 + k) * kn::COL + j];
                        dq[k] = q2[k] - (double)q1[i][k], sq[k] = q2[k] + (double)q1[i][k];
                        nd += dq[k] * dq[k], ns += sq[k] * sq[k];
                    }
                    const bool minus = sqrt(nd) < sqrt(ns);
                    for (int k = 0; k < 4; ++k) sub[k] = minus ? dq[k] : sq[k];
                    cj[0] = -q2[0], cj[1] = -q2[1], cj[2] = -q2[2], cj[3] = q2[3];
                    qmul<double>(sub, cj, dori);
                    double w[3], v[3];
                    for (int k = 0; k < 3; ++k) {
                        w[k] = 2.0 * dori[k] / kn::DT;
                        v[k] = (x2[k] - ((double)x1r[i][k] + root[k])) / kn::DT;
                    }
                    res[i][0] = (w[1] * sol[2] - w[2] * sol[1]) + v[0];
                    res[i][1] = (w[2] * sol[0] - w[0] * sol[2]) + v[1];
                    res[i][2] = (w[0] * sol[1] - w[1] * sol[0]) + v[2];
                }
                bool all_nan = true;
                for (int i = 0; i < 2; ++i)
                    for (int k = 0; k < 3; ++k) all_nan = all_nan && (res[i][k] != res[i][k]);
                double vr[3];
                for (int k = 0; k < 3; ++k) {
                    if (all_nan) { vr[k] = 0.0; continue; }
                    const bool a = res[0][k] == res[0][k], b = res[1][k] == res[1][k];      // np.nanmean over the two feet
                    const double m = a && b ? (res[0][k] + res[1][k]) / 2.0 : (a ? res[0][k] : (b ? res[1][k] : nan));
                    vr[k] = clip_nan_transparent_d(m, 0.5);
                }
                vr[2] = 0.0;                                         // flat ground (:184-189), the norm test taken literally
                for (int i = 0; i < 2; ++i)
                    if (sqrt(cl[i][0] * cl[i][0] + cl[i][1] * cl[i][1] + cl[i][2] * cl[i][2]) < 100.0) vr[2] += cl[i][2] * 1.0;
                for (int k = 0; k < 3; ++k) {
                    const double d = vr[k] * kn::DT;
                    root[k] = pre[k] - d;
                    ro[k] = (float)root[k];
                    for (int i = 0; i < kn::SBPS; ++i) vo[3 * i + k] = (float)(cl[i][k] - d);
                }
                for (int i = 0; i < 2; ++i) {
                    for (int k = 0; k < 3; ++k) x1r[i][k] = Fs[(7 * body[i] + k) * kn::COL + j];
                    for (int k = 0; k < 4; ++k) q1[i][k] = Fs[(7 * body[i] + 3 + k) * kn::COL + j];
                }
                for (int k = 0; k < 3; ++k) vprev[k] = sr[54 + k];
                has_prev = 1;
                last = j;
            }
            last_s = last;
        }
        __syncthreads();
        const int last = last_s;
        if (last >= 0)
            for (int e = lane; e < per; e += kn::LANES) cr.pq[e] = Fs[e * kn::COL + last];
        __syncthreads();
    }
    if (lane == 0) {
        for (int k = 0; k < 3; ++k) cr.root[k] = root[k], cr.vprev[k] = vprev[k];
        cr.has_prev = has_prev;
    }
}

// fixed-order sum of one double per thread over a 256-thread workgroup
__device__ __forceinline__ double block_sum(double v, double* sh, int t) {
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(256) void kin_metrics_kernel(const KinSkel* __restrict__ skp, const float* __restrict__ pred,
                                                          const float* __restrict__ gt, const float* __restrict__ pq_p,
                                                          const float* __restrict__ pq_g, const long long* __restrict__ offsets,
                                                          int start, int end, int i2, int i5, int i10, double* __restrict__ out) {
    __shared__ double sh[256];
    const int L = kin_links(*skp), per = (L + 1) * 7, t = threadIdx.x;
    const long long a = offsets[blockIdx.x] + start, b = offsets[blockIdx.x + 1] - end;
    const long long n = b - a;                                     // rows in range
    double* o = out + (size_t)blockIdx.x * 7;
    if (n < 4) {                                                   // (the host refuses such a file; never an empty mean's garbage)
        if (t < 7) o[t] = __builtin_nan("");
        return;
    }
    double s_ang = 0.0, s_pos = 0.0, s_jerk = 0.0, s_rjerk = 0.0;
    for (long long r = t; r < n; r += 256) {
        const size_t row = (size_t)(a + r);
        const float* x1 = gt + row * kn::QDQ;
        const float* x2 = pred + row * kn::QDQ;
        for (int j = 0; j < 18; ++j) {                             // the geodesic angle between the 18 rotations (:314-327)
            double qa[4], qb[4], d[4];
            a2q<double>((double)x1[3 + 3 * j], (double)x1[4 + 3 * j], (double)x1[5 + 3 * j], qa);
            a2q<double>((double)x2[3 + 3 * j], (double)x2[4 + 3 * j], (double)x2[5 + 3 * j], qb);
            qa[0] = -qa[0], qa[1] = -qa[1], qa[2] = -qa[2];
            qmul<double>(qa, qb, d);
            s_ang += 2.0 * atan2(sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), fabs(d[3]));
        }
        const float* p1 = pq_g + row * per;
        const float* p2 = pq_p + row * per;
        for (int k = 1; k <= L; ++k) {                             // root-relative COM positions (:330-337)
            double e2 = 0.0;
            for (int c = 0; c < 3; ++c) {
                const double e = ((double)p2[7 * k + c] - (double)p2[c]) - ((double)p1[7 * k + c] - (double)p1[c]);
                e2 += e * e;
            }
            s_pos += sqrt(e2);
        }
        if (r + 3 < n) {                                           // third differences of the prediction (:359-378)
            for (int k = 0; k <= L; ++k) {
                double e2 = 0.0;
                for (int c = 0; c < 3; ++c) {
                    const double e = (double)p2[3 * per + 7 * k + c] - 3.0 * (double)p2[2 * per + 7 * k + c]
                                     + 3.0 * (double)p2[per + 7 * k + c] - (double)p2[7 * k + c];
                    e2 += e * e;
                }
                s_jerk += sqrt(e2);
                if (k == 0) s_rjerk += sqrt(e2);
            }
        }
    }
    s_ang = block_sum(s_ang, sh, t);
    s_pos = block_sum(s_pos, sh, t);
    s_jerk = block_sum(s_jerk, sh, t);
    s_rjerk = block_sum(s_rjerk, sh, t);
    if (t == 0) {
        o[0] = s_ang / (double)(n * 18) * 180 / 3.1416;            // the script's literal constant
        o[1] = s_pos / (double)(n * L) * 100.0;
        o[5] = s_jerk / (double)((n - 3) * (L + 1)) * 100.0;
        o[6] = s_rjerk / (double)(n - 3) * 100.0;
        const int idx[3] = {i2, i5, i10};
        for (int m = 0; m < 3; ++m) {                              // root displacement from row 0 to row idx (:381-391)
            long long ind = idx[m] < 0 ? 0 : idx[m];
            if (ind > n - 1) ind = n - 1;
            double e2 = 0.0;
            for (int c = 0; c < 3; ++c) {
                const double d1 = (double)pq_g[(size_t)(a + ind) * per + c] - (double)pq_g[(size_t)a * per + c];
                const double d2 = (double)pq_p[(size_t)(a + ind) * per + c] - (double)pq_p[(size_t)a * per + c];
                e2 += (d1 - d2) * (d1 - d2);
            }
            o[2 + m] = sqrt(e2);
        }
    }
}

}  // namespace tip

using namespace tip;

extern "C" {

static int kin_done() { return hipGetLastError() == hipSuccess ? TIP_OK : TIP_ERR_HIP; }
static bool kin_bad_rows(long long n) { return n < 0 || n > (1LL << 30); }
static bool kin_bad_slots(int n) { return n < 0 || n > (1 << 24); }

int tip_kin_skel_bytes(size_t* bytes) {
    if (!bytes) return TIP_ERR_INVALID_ARG;
    *bytes = sizeof(KinSkel);
    return TIP_OK;
}

int tip_kin_carry_bytes(int n_slots, size_t* bytes) {
    if (!bytes || kin_bad_slots(n_slots)) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)n_slots * sizeof(KinCarry);
    return TIP_OK;
}

int tip_kin_fk(const void* skel, const float* q, int ldq, long long n, float* pq_g, float* pq_jf, tip_stream_t stream) {
    if (!skel || !q || !pq_g || kin_bad_rows(n) || ldq < kn::NQ) return TIP_ERR_INVALID_ARG;
    if (n == 0) return TIP_OK;
    hipLaunchKernelGGL(kin_fk_kernel, dim3((unsigned)((n + kn::LANES - 1) / kn::LANES)), dim3(kn::LANES), 0,
                       static_cast<hipStream_t>(stream), static_cast<const KinSkel*>(skel), q, ldq, n, pq_g, pq_jf);
    return kin_done();
}

int tip_kin_track_reset(const void* skel, void* carry, int n_slots, const int* slots, int count, const float* s_init,
                        tip_stream_t stream) {
    if (!skel || !carry || kin_bad_slots(n_slots) || count < 0 || (count > 0 && !s_init) || reinterpret_cast<uintptr_t>(carry) % 8)
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL(kin_reset_kernel, dim3((count + kn::LANES - 1) / kn::LANES), dim3(kn::LANES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), static_cast<KinCarry*>(carry), n_slots, slots, count, s_init);
    return kin_done();
}

int tip_kin_track(const void* skel, void* carry, int n_slots, const int* slots, const long long* begin, const long long* end, int count,
                  long long n_rows, const float* s_rest, const float* c_t, int nc, const unsigned char* valid, float* root_out,
                  float* viz_out, tip_stream_t stream) {
    if (!skel || !carry || kin_bad_slots(n_slots) || count < 0 || kin_bad_rows(n_rows) || (nc != 8 && nc != 20)
        || reinterpret_cast<uintptr_t>(carry) % 8)
        return TIP_ERR_INVALID_ARG;
    if (count > 0 && (!begin || !end || !s_rest || !c_t || !root_out || !viz_out)) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0 || n_rows == 0) return TIP_OK;
    hipLaunchKernelGGL(kin_track_kernel, dim3(count), dim3(kn::LANES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), static_cast<KinCarry*>(carry), n_slots, slots, begin, end, n_rows, s_rest, c_t,
                       nc, valid, root_out, viz_out);
    return kin_done();
}

int tip_kin_metrics(const void* skel, const float* pred_qdq, const float* gt_qdq, const float* pq_pred, const float* pq_gt,
                    const long long* offsets, int count, int start, int end, int i2, int i5, int i10, double* out,
                    tip_stream_t stream) {
    if (!skel || count < 0 || start < 0 || end < 0 || reinterpret_cast<uintptr_t>(out) % 8) return TIP_ERR_INVALID_ARG;
    if (count > 0 && (!pred_qdq || !gt_qdq || !pq_pred || !pq_gt || !offsets || !out)) return TIP_ERR_INVALID_ARG;
    if (count == 0) return TIP_OK;
    hipLaunchKernelGGL(kin_metrics_kernel, dim3(count), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), pred_qdq, gt_qdq, pq_pred, pq_gt, offsets, start, end, i2, i5, i10, out);
    return kin_done();
}

}  // extern "C"
