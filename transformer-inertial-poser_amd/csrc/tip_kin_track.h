// tip_kin_track.h — the SBP root-correction step of the two runners, once: what tip_kin.hip's flat-ground tracker (RTRunnerMin.step,
// real_time_runner_minimal.py:159-194) and tip_terrain.hip's full runner (RTRunner.step, real_time_runner.py:451-463) do alike for
// every frame, and what their reset kernels do alike for a carry.
//
//   root_pre = root + v DT on the velocity from before the averaging; the SBP locations; the residues of the active SBPs against the
//   previous frame's corrected poses (data_utils.py:397-412, 473-548: the quaternion difference with its sign choice, w x sol + v);
//   vel_res = clip(nanmean over the two feet, +-0.5)
//
// The two kernels differ in three things only, and those stay with them: which residues are read (NRES = 2: the feet; NRES = 3: the
// feet and the root, for the IK), what becomes of vel_res[2] after the clip, and who executes — lane 0 alone in kin_track_kernel, every
// lane on the same values in terrain_track_kernel.  Hence nothing here holds a barrier or a shuffle, and only the functions that say
// so store to memory.  All of it is fp64 on the fp32 poses; the library is built with -ffp-contract=off, so the statements give the
// same bits wherever they are inlined.
//
// Also here, because tip_replay.hip reads two of its words: the head of a terrain slot's block and the block's layout.
#pragma once
#include "tip_kin_fk.h"

namespace tip {

// np.clip(v, lo, hi): a NaN stays a NaN
__device__ __forceinline__ double kin_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ void kin_conj(const double* q, double* o) { o[0] = -q[0], o[1] = -q[1], o[2] = -q[2], o[3] = q[3]; }

// The SBP whose residue is kept as number m: lankle, rankle and, for NRES = 3, root; and the residue number of SBP i, or -1 (the
// wrists' residues are read by nobody).
__device__ __forceinline__ constexpr int sbp_of_res(int m) { return m < 2 ? m : 4; }
template <int NRES> __device__ __forceinline__ constexpr int res_of_sbp(int i) { return i < 2 ? i : (NRES == 3 && i == 4 ? 2 : -1); }

// The wave prologue: the sequence's slot and its rows [r0, r1) clamped to [0, n_rows]; false (uniform over the wave) for a slot outside
// the table or no rows.
__device__ __forceinline__ bool track_range(const int* __restrict__ slots, const long long* __restrict__ begin,
                                            const long long* __restrict__ end, int seq, int n_slots, long long n_rows, int& slot,
                                            long long& r0, long long& r1) {
    slot = slots ? slots[seq] : seq;
    if (slot < 0 || slot >= n_slots) return false;
    r0 = begin[seq], r1 = end[seq];
    if (r0 < 0) r0 = 0;
    if (r1 > n_rows) r1 = n_rows;
    return r1 > r0;
}

// body indices of the five SBPs; an entry outside the table reads as the root
__device__ __forceinline__ void sbp_bodies(const KinSkel& sk, int L, int* body) {
    for (int i = 0; i < kn::SBPS; ++i) body[i] = (sk.sbp[i] < 0 || sk.sbp[i] > L) ? 0 : sk.sbp[i];
}

// The scan state: the corrected root, the previous valid frame's poses of the NRES bodies about it, and that frame's velocity columns.
template <int NRES>
struct SbpScan {
    double root[3];
    float x1r[NRES][3], q1[NRES][4], vprev[3];
    int has_prev;
};

template <int NRES>
__device__ __forceinline__ void sbp_scan_load(SbpScan<NRES>& st, const KinCarry& cr, const int* body) {
    for (int k = 0; k < 3; ++k) st.root[k] = cr.root[k], st.vprev[k] = cr.vprev[k];
    st.has_prev = cr.has_prev;
    for (int m = 0; m < NRES; ++m) {
        for (int k = 0; k < 3; ++k) st.x1r[m][k] = cr.pq[7 * body[sbp_of_res(m)] + k];
        for (int k = 0; k < 4; ++k) st.q1[m][k] = cr.pq[7 * body[sbp_of_res(m)] + 3 + k];
    }
}

// (stores: one lane's)
template <int NRES>
__device__ __forceinline__ void sbp_scan_store(const SbpScan<NRES>& st, KinCarry& cr) {
    for (int k = 0; k < 3; ++k) cr.root[k] = st.root[k], cr.vprev[k] = st.vprev[k];
    cr.has_prev = st.has_prev;
}

// The shared half of a frame, on column j of the FK'd poses Fs (root at the origin): pre = root_pre, cl = the SBP locations (100 for an
// inactive point), res = the residues (NaN for an inactive point), vr = vel_res after the nanmean and the clip.  The caller applies its
// own z rule and its own shift of cl.
template <int NRES>
__device__ __forceinline__ void sbp_step(const SbpScan<NRES>& st, const int* body, const float* __restrict__ sr, const float* __restrict__ ct,
                                         int n_sbps, const float* Fs, int j, double* pre, double (*cl)[3], double (*res)[3], double* vr) {
    for (int k = 0; k < 3; ++k) {                        // on the velocity from before the averaging
        const double v = st.has_prev ? 2.0 * (double)sr[54 + k] - (double)st.vprev[k] : (double)sr[54 + k];
        pre[k] = st.root[k] + v * kn::DT;
    }
    for (int i = 0; i < kn::SBPS; ++i)
        for (int k = 0; k < 3; ++k) cl[i][k] = 100.0;
    const double nan = __builtin_nan("");
    for (int m = 0; m < NRES; ++m)
        for (int k = 0; k < 3; ++k) res[m][k] = nan;
    for (int i = 0; i < n_sbps; ++i) {
        if (ct[4 * i] == 0.f) continue;                  // inactive: location 100, residue NaN
        double x2[3], sol[3];
        for (int k = 0; k < 3; ++k) {
            x2[k] = (double)Fs[(7 * body[i] + k) * kn::COL + j] + pre[k];
            sol[k] = (double)ct[4 * i + 1 + k];
            cl[i][k] = x2[k] + sol[k];
        }
        const int m = res_of_sbp<NRES>(i);
        if (m < 0) continue;                             // only the two feet correct the root (:517-520)
        double q2[4], dq[4], sq[4], sub[4], cj[4], dori[4];
        double nd = 0.0, ns = 0.0;
        for (int k = 0; k < 4; ++k) {
            q2[k] = (double)Fs[(7 * body[i] + 3 + k) * kn::COL + j];
            dq[k] = q2[k] - (double)st.q1[m][k], sq[k] = q2[k] + (double)st.q1[m][k];
            nd += dq[k] * dq[k], ns += sq[k] * sq[k];
        }
        const bool minus = sqrt(nd) < sqrt(ns);
        for (int k = 0; k < 4; ++k) sub[k] = minus ? dq[k] : sq[k];
        kin_conj(q2, cj);
        qmul<double>(sub, cj, dori);
        double w[3], v[3];
        for (int k = 0; k < 3; ++k) {
            w[k] = 2.0 * dori[k] / kn::DT;
            v[k] = (x2[k] - ((double)st.x1r[m][k] + st.root[k])) / kn::DT;
        }
        res[m][0] = (w[1] * sol[2] - w[2] * sol[1]) + v[0];
        res[m][1] = (w[2] * sol[0] - w[0] * sol[2]) + v[1];
        res[m][2] = (w[0] * sol[1] - w[1] * sol[0]) + v[2];
    }
    bool all_nan = true;
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 3; ++k) all_nan = all_nan && (res[i][k] != res[i][k]);
    for (int k = 0; k < 3; ++k) {
        if (all_nan) { vr[k] = 0.0; continue; }
        const bool a = res[0][k] == res[0][k], b = res[1][k] == res[1][k];      // np.nanmean over the two feet
        const double m = a && b ? (res[0][k] + res[1][k]) / 2.0 : (a ? res[0][k] : (b ? res[1][k] : nan));
        vr[k] = kin_clip(m, -0.5, 0.5);
    }
}

// The advance after a valid frame: column j becomes the previous frame.
template <int NRES>
__device__ __forceinline__ void sbp_advance(SbpScan<NRES>& st, const int* body, const float* __restrict__ sr, const float* Fs, int j) {
    for (int m = 0; m < NRES; ++m) {
        for (int k = 0; k < 3; ++k) st.x1r[m][k] = Fs[(7 * body[sbp_of_res(m)] + k) * kn::COL + j];
        for (int k = 0; k < 4; ++k) st.q1[m][k] = Fs[(7 * body[sbp_of_res(m)] + 3 + k) * kn::COL + j];
    }
    for (int k = 0; k < 3; ++k) st.vprev[k] = sr[54 + k];
    st.has_prev = 1;
}

// The write-back after a 64-row chunk, by the whole wave: the carry's poses from the chunk's last valid column (none: nothing).
__device__ __forceinline__ void carry_store_pq(KinCarry& cr, const float* Fs, int per, int last, int lane) {
    if (last >= 0)
        for (int e = lane; e < per; e += kn::LANES) cr.pq[e] = Fs[e * kn::COL + last];
}

// A carry at its start: root = s_init[:3], no previous velocity, pq = FK(s_init) about the root.  carry_init, by one lane, fills the LDS
// column F with that FK and sets all but pq; carry_init_pq copies the column out, entries first, first + step, ... — by the same lane
// (0, 1) or, behind a barrier, by a workgroup (t, its size).  Entries of pq beyond (L + 1) * 7 and the pad are the caller's.
// SCALED: the FK of a wearer of body scale `scale` (the root of s_init is the wearer's metres already and is not scaled); a scale that
// kin_scale_ok refuses leaves a NaN root and NaN positions, which the track kernels never read: they test the scale first.
template <bool SCALED = false>
__device__ __forceinline__ void carry_init(const KinSkel& sk, int L, KinCarry& c, const float* __restrict__ row, float* F, float scale = 1.f) {
    if constexpr (SCALED) scale = kin_scale_ok(scale) ? scale : __builtin_nanf("");
    fk_frames_of<SCALED>(sk, L, row + 3, 0.f, 0.f, 0.f, scale, F);
    fk_to_com_of<SCALED>(sk, L, scale, F);
    for (int k = 0; k < 3; ++k) c.root[k] = (double)row[k], c.vprev[k] = 0.f;
    if constexpr (SCALED)
        if (scale != scale)
            for (int k = 0; k < 3; ++k) c.root[k] = __builtin_nan("");
    c.has_prev = 0;
}
__device__ __forceinline__ void carry_init_pq(KinCarry& c, const float* F, int L, int first, int step) {
    for (int e = first; e < (L + 1) * 7; e += step) c.pq[e] = F[e * kn::COL];
}

// One terrain slot's block: this head, region_height[max_regions], region_weight[max_regions] (fp64), the map [grid_num, grid_num].
struct TerHead {
    KinCarry carry;
    double c_prev[kn::SBPS][3];  // c_locs_prev
    double ik_delta[2][3];       // ik_target_deltas of lankle, rankle
    int tick[3];                 // establishing_height_phase_tick of lankle, rankle, root
    int n_regions;
    int off_map, regions_full;
    int grid_num, max_regions;   // as the reset laid the block out
    int pad[14];
};
static_assert(sizeof(TerHead) == 1280, "TerHead layout");

struct TerLay {
    size_t off_w, off_map, stride;
};
__host__ __device__ __forceinline__ TerLay ter_lay(int G, int M) {
    TerLay l;
    l.off_w = sizeof(TerHead) + (size_t)M * 8;
    l.off_map = l.off_w + (size_t)M * 8;
    l.stride = (l.off_map + (size_t)G * G * 4 + 7) & ~(size_t)7;
    return l;
}

}  // namespace tip
