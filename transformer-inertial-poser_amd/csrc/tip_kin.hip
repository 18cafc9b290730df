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
// The first three are templates over (SCALED, S...): SCALED = true is the kernel for wearers of different body sizes — every joint and
// COM offset times the wearer's scale before it is rotated (tip_kin_fk.h), the scale read from a device array, one entry per row in
// FK, one per block (slot) in the reset and the tracker — behind the *_scaled entries of tip_kin_scaled.hip.  The metrics need no
// such form: they read the pose tables, which the scaled FK makes.
//
// PRECISION.  FK is fp32.  The scan — root accumulator, residues, clip, z rule — is fp64 on the fp32 poses, and the carry keeps the
// root as fp64; outputs are rounded to fp32 once.  The metrics are fp64 on the fp32 poses.
//
// Nothing waits on another workgroup; a carry block is written by the one wave whose sequence names it.
//
// The scan's frame — root_pre, the SBP locations, the residues, the nanmean and the clip — the scan state's load, advance and store,
// and the carry's initialisation are tip_kin_track.h's: one body for this tracker and for tip_terrain.hip's.  What is written out
// below is this tracker's own: the flat-ground z rule and the shift of the outputs.
// SCALED = true is instantiated in a translation unit of its own (tip_kin_scaled.hip, which includes this file for the templates and
// defines TIP_KIN_SCALED_TU), so that the unscaled kernels are compiled alone, as they were before there was a scale: with both in
// one unit the inliner's choices for the unscaled ones moved (make resource-usage showed scratch where there was none).
#include "tip_kin_track.h"   // sbp_step and the carry; over tip_kin_fk.h: KinLinkT, a2q, qmul, qrot, fk_frames, fk_to_com, one body for
                             // fp32 (here) and fp64 (tip_syn.hip), KinSkel, KinCarry and the fp32 FK wrappers

namespace tip {

// rows [first, first + cnt) of out[n, L + 1, 7] from the LDS columns 0 .. cnt - 1, consecutive lanes on consecutive floats
__device__ __forceinline__ void fk_store(const float* F, int per, long long first, int cnt, float* __restrict__ out, int lane) {
    float* o = out + (size_t)first * per;
    for (int e = lane; e < cnt * per; e += kn::LANES) {
        const int r = e / per, c = e - r * per;
        o[e] = F[c * kn::COL + r];
    }
}

// SCALED: `scale` has one entry per row, so rows of many wearers share a launch; a row whose scale kin_scale_ok refuses is NaN whole.
template <bool SCALED, typename... S>
__global__ __launch_bounds__(64) void kin_fk_kernel(const KinSkel* __restrict__ skp, const float* __restrict__ q, int ldq, long long n,
                                                    float* __restrict__ pq_g, float* __restrict__ pq_jf, S... scale) {
    __shared__ float Fs[kn::MAX_BODIES * 7 * kn::COL];
    const KinSkel& sk = *skp;
    const int L = kin_links(sk), lane = threadIdx.x, per = (L + 1) * 7;
    const long long first = (long long)blockIdx.x * kn::LANES;
    const long long left = n - first;
    const int cnt = left < kn::LANES ? (int)left : kn::LANES;
    float* F = Fs + lane;
    float sc = 1.f;
    bool ok = true;
    if constexpr (SCALED)
        if (lane < cnt) sc = kin_scale_ptr(scale...)[first + lane], ok = kin_scale_ok(sc);
    if (lane < cnt) {
        const float* row = q + (size_t)(first + lane) * ldq;
        if (ok) fk_frames_of<SCALED>(sk, L, row + 3, row[0], row[1], row[2], sc, F);
        else
            for (int e = 0; e < per; ++e) F[e * kn::COL] = __builtin_nanf("");
    }
    __syncthreads();
    if (pq_jf) fk_store(Fs, per, first, cnt, pq_jf, lane);
    __syncthreads();
    if (lane < cnt && ok) fk_to_com_of<SCALED>(sk, L, sc, F);
    __syncthreads();
    fk_store(Fs, per, first, cnt, pq_g, lane);
}

// SCALED: `scale` is indexed by the block (slot), as the track kernel reads it.
template <bool SCALED, typename... S>
__global__ __launch_bounds__(64) void kin_reset_kernel(const KinSkel* __restrict__ skp, KinCarry* __restrict__ carry, int n_slots,
                                                       const int* __restrict__ slots, int count, const float* __restrict__ s_init,
                                                       S... scale) {
    __shared__ float Fs[kn::MAX_BODIES * 7 * kn::COL];
    const KinSkel& sk = *skp;
    const int L = kin_links(sk), lane = threadIdx.x;
    const int j = blockIdx.x * kn::LANES + lane;
    if (j >= count) return;
    const int slot = slots ? slots[j] : j;
    if (slot < 0 || slot >= n_slots) return;
    const float* row = s_init + (size_t)j * kn::QDQ;
    if constexpr (SCALED) carry_init<true>(sk, L, carry[slot], row, Fs + lane, kin_scale_ptr(scale...)[slot]);
    else carry_init(sk, L, carry[slot], row, Fs + lane);
    carry_init_pq(carry[slot], Fs + lane, L, 0, 1);
}

// SCALED: the sequence's body scale is scale[slot], read once per launch; one that kin_scale_ok refuses makes the sequence's rows NaN and
// leaves its carry alone.
template <bool SCALED, typename... S>
__global__ __launch_bounds__(64) void kin_track_kernel(const KinSkel* __restrict__ skp, KinCarry* __restrict__ carry, int n_slots,
                                                       const int* __restrict__ slots, const long long* __restrict__ begin,
                                                       const long long* __restrict__ end, long long n_rows,
                                                       const float* __restrict__ s_rest, const float* __restrict__ c_t, int nc,
                                                       const unsigned char* __restrict__ valid, float* __restrict__ root_out,
                                                       float* __restrict__ viz_out, S... scale) {
    __shared__ float Fs[kn::MAX_BODIES * 7 * kn::COL];
    __shared__ int last_s;
    const KinSkel& sk = *skp;
    const int L = kin_links(sk), lane = threadIdx.x, per = (L + 1) * 7;
    int slot;
    long long r0, r1;
    if (!track_range(slots, begin, end, blockIdx.x, n_slots, n_rows, slot, r0, r1)) return;      // (uniform over the wave)
    KinCarry& cr = carry[slot];
    float sc = 1.f;
    if constexpr (SCALED) {
        sc = kin_scale_ptr(scale...)[slot];
        if (!kin_scale_ok(sc)) {                                      // (uniform over the wave)
            const float nanf = __builtin_nanf("");
            for (long long e = r0 * 3 + lane; e < r1 * 3; e += kn::LANES) root_out[e] = nanf;
            for (long long e = r0 * 15 + lane; e < r1 * 15; e += kn::LANES) viz_out[e] = nanf;
            return;
        }
    }
    const int n_sbps = nc / 4;
    int body[kn::SBPS];
    sbp_bodies(sk, L, body);
    float* F = Fs + lane;

    SbpScan<2> st;                                                // lane 0's scan state
    if (lane == 0) sbp_scan_load(st, cr, body);
    for (long long t0 = r0; t0 < r1; t0 += kn::LANES) {
        const long long left = r1 - t0;
        const int cnt = left < kn::LANES ? (int)left : kn::LANES;
        if (lane == 0) last_s = -1;
        if (lane < cnt && (!valid || valid[t0 + lane])) {
            fk_frames_of<SCALED>(sk, L, s_rest + (size_t)(t0 + lane) * kn::REST, 0.f, 0.f, 0.f, sc, F);
            fk_to_com_of<SCALED>(sk, L, sc, F);
        }
        __syncthreads();
        if (lane == 0) {
            int last = -1;
            for (int j = 0; j < cnt; ++j) {
                const size_t row = (size_t)(t0 + j);
                float* ro = root_out + row * 3;
                float* vo = viz_out + row * 15;
                if (valid && !valid[row]) {                          // what the runner returns while it primes: the carry's root, 100s
                    for (int k = 0; k < 3; ++k) ro[k] = (float)st.root[k];
                    for (int k = 0; k < 15; ++k) vo[k] = 100.f;
                    continue;
                }
                const float* sr = s_rest + row * kn::REST;
                double pre[3], cl[kn::SBPS][3], res[2][3], vr[3];
                sbp_step<2>(st, body, sr, c_t + row * nc, n_sbps, Fs, j, pre, cl, res, vr);      // :159-183
                vr[2] = 0.0;                                         // flat ground (:184-189), the norm test taken literally
                for (int i = 0; i < 2; ++i)
                    if (sqrt(cl[i][0] * cl[i][0] + cl[i][1] * cl[i][1] + cl[i][2] * cl[i][2]) < 100.0) vr[2] += cl[i][2] * 1.0;
                for (int k = 0; k < 3; ++k) {
                    const double d = vr[k] * kn::DT;
                    st.root[k] = pre[k] - d;
                    ro[k] = (float)st.root[k];
                    for (int i = 0; i < kn::SBPS; ++i) vo[3 * i + k] = (float)(cl[i][k] - d);
                }
                sbp_advance(st, body, sr, Fs, j);
                last = j;
            }
            last_s = last;
        }
        __syncthreads();
        carry_store_pq(cr, Fs, per, last_s, lane);
        __syncthreads();
    }
    if (lane == 0) sbp_scan_store(st, cr);
}

#ifndef TIP_KIN_SCALED_TU
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

#endif  // TIP_KIN_SCALED_TU

}  // namespace tip

#ifndef TIP_KIN_SCALED_TU
using namespace tip;

extern "C" {

int tip_kin_skel_bytes(size_t* bytes) {
    if (!bytes) return TIP_ERR_INVALID_ARG;
    *bytes = sizeof(KinSkel);
    return TIP_OK;
}

int tip_kin_carry_bytes(int n_slots, size_t* bytes) {
    if (!bytes || tip_bad_count(n_slots)) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)n_slots * sizeof(KinCarry);
    return TIP_OK;
}

int tip_kin_fk(const void* skel, const float* q, int ldq, long long n, float* pq_g, float* pq_jf, tip_stream_t stream) {
    if (!skel || !q || !pq_g || tip_bad_rows(n) || ldq < kn::NQ) return TIP_ERR_INVALID_ARG;
    if (n == 0) return TIP_OK;
    hipLaunchKernelGGL((kin_fk_kernel<false>), dim3((unsigned)((n + kn::LANES - 1) / kn::LANES)), dim3(kn::LANES), 0,
                       static_cast<hipStream_t>(stream), static_cast<const KinSkel*>(skel), q, ldq, n, pq_g, pq_jf);
    return tip_launch_status();
}

int tip_kin_track_reset(const void* skel, void* carry, int n_slots, const int* slots, int count, const float* s_init,
                        tip_stream_t stream) {
    if (!skel || !carry || tip_bad_count(n_slots) || count < 0 || (count > 0 && !s_init) || reinterpret_cast<uintptr_t>(carry) % 8)
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL((kin_reset_kernel<false>), dim3((count + kn::LANES - 1) / kn::LANES), dim3(kn::LANES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), static_cast<KinCarry*>(carry), n_slots, slots, count, s_init);
    return tip_launch_status();
}

int tip_kin_track(const void* skel, void* carry, int n_slots, const int* slots, const long long* begin, const long long* end, int count,
                  long long n_rows, const float* s_rest, const float* c_t, int nc, const unsigned char* valid, float* root_out,
                  float* viz_out, tip_stream_t stream) {
    if (!skel || !carry || tip_bad_count(n_slots) || count < 0 || tip_bad_rows(n_rows) || (nc != 8 && nc != 20)
        || reinterpret_cast<uintptr_t>(carry) % 8)
        return TIP_ERR_INVALID_ARG;
    if (count > 0 && (!begin || !end || !s_rest || !c_t || !root_out || !viz_out)) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0 || n_rows == 0) return TIP_OK;
    hipLaunchKernelGGL((kin_track_kernel<false>), dim3(count), dim3(kn::LANES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), static_cast<KinCarry*>(carry), n_slots, slots, begin, end, n_rows, s_rest, c_t,
                       nc, valid, root_out, viz_out);
    return tip_launch_status();
}

int tip_kin_metrics(const void* skel, const float* pred_qdq, const float* gt_qdq, const float* pq_pred, const float* pq_gt,
                    const long long* offsets, int count, int start, int end, int i2, int i5, int i10, double* out,
                    tip_stream_t stream) {
    if (!skel || count < 0 || start < 0 || end < 0 || reinterpret_cast<uintptr_t>(out) % 8) return TIP_ERR_INVALID_ARG;
    if (count > 0 && (!pred_qdq || !gt_qdq || !pq_pred || !pq_gt || !offsets || !out)) return TIP_ERR_INVALID_ARG;
    if (count == 0) return TIP_OK;
    hipLaunchKernelGGL(kin_metrics_kernel, dim3(count), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), pred_qdq, gt_qdq, pq_pred, pq_gt, offsets, start, end, i2, i5, i10, out);
    return tip_launch_status();
}

}  // extern "C"
#endif  // TIP_KIN_SCALED_TU
