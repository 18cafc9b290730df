// tip_terrain.hip — the full runner's tail on the device: what RTRunner.step does behind the model (real_time_runner.py:451-496), as a
// CONSUMER of the streaming engines' outputs beside them, as tip_kin.hip's tracker is for RTRunnerMin.  Per stream: the height-region
// map, the "establishing height" ticks, the vertical root correction from the map, and the two-joint leg IK whose pose is fed back
// into the model's history (through tip_stream_history_override, a launch of its own: no engine kernel is involved here).
//
//   real_time_runner.py:451-463   root_pre = root + v DT; FK; residues and c_locs of the active SBPs against the previous frame's
//                                 corrected poses (data_utils.py:397-412, 473-548); vel_res = clip(nanmean of the two feet);
//                                 vel_res[2] = 0; c_locs -= vel_res DT
//   :264-277                      update_sbp_establishing_height_ticks
//   :140-262                      update_height_map_new on c_locs_prev, for lankle, rankle (vel_res[2] += -20 d each) and, with
//                                 multi_sbp_terrain_and_correction and the pelvis more than 0.2 m (xy) from the mid-ankle point, root
//   :334-382, data_utils.py:556-630   correct_joint_q_for_history_feedback over leg_two_joint_ik_keep_foot_pointing; Q2A is scipy's
//                                 as_rotvec (normalise, w >= 0, 2 atan2, the series below 1e-3)
//   :489-496                      root = root_pre - vel_res DT, poses about the root, c_locs_prev = c_locs
//
// The leg chain is read from the skeleton table: ankle = the SBP body, knee and hip its parent and grandparent, "parent" the hip's
// parent; the pose columns are those links' state columns.  On the reference's character that is ik_chain_map_bullet ([-1, 0, 1, 2],
// [-1, 3, 4, 5]) and ik_chain_map_nimble_joint ([1, 2, 3], [15, 16, 17]).  A chain that is not three spherical links never fires.
//
// THE MAP.  One 4-byte cell: region index (high half) and the SQUARED integer distance to the centre of the update that wrote it (low
// half).  The reference's confidences are -sqrt(i^2 + j^2) of integers and -100 at the start, so confidence_old > confidence_new is
// d2_old < d2_new with 10000 for the start: exact, no square root.  A step touches a 2d x 2d patch, never a map.
//
// DECISIONS the reference leaves open:
//   off-map     a patch not wholly inside the map (the reference raises on the empty slice): no map or region write, the update
//               returns 0, the tick goes to -1, off_map counts it
//   overflow    a new region is due and the list is full (max_regions): the same, regions_full counts it
//   ties        an exact tie of |height difference| between two regions of the patch goes to the lower region index (CPython's set
//               order decides in the reference)
//   2 SBPs      c_t of 8 columns has only the feet; flags bit 0 is then TIP_ERR_INVALID_ARG
//   non-finite  a non-finite c_loc is inactive, as the reference's norm < 100 makes it; an index is formed only from an active (hence
//               finite) location after a range test in fp64.  A non-finite row can spoil its own slot's root, and nothing else.
//
// PRECISION, as the tracker's: FK in fp32 (root at the origin); everything behind it in fp64 on the fp32 poses — residues, deltas,
// region heights and weights, the IK's norms, arccos and quaternion products; outputs rounded to fp32 once.  Quaternions out of the
// fp32 FK are used as they are where the reference's Q2R would normalise them (a difference below the fp32 FK's own rounding).
//
// Kernels:
//   terrain_reset_kernel   one workgroup per listed slot: the carry (carry_init, as kin_reset_kernel's), RTRunner.__init__'s state, and the
//                          only pass over a whole map
//   terrain_track_kernel   one wave per sequence: 64 rows of FK in parallel, then the wave steps through those rows with every lane
//                          holding the same scan state (the same fp64 statements on the same values), so that the patch — the region
//                          search over it and its merge — is lane-parallel under wave-uniform control flow.  Stores of scan state are
//                          lane 0's; region heights and the map go through memory with a workgroup barrier between writer and reader.
//
// Both are templates over (SCALED, S...), as tip_kin.hip's: SCALED = true runs FK on the wearer's own body scale (read from a device
// array by block), behind the *_scaled entries of tip_terrain_scaled.hip; the block's layout is the same.
//
// Nothing waits on another workgroup; a slot's block is written only by the wave whose sequence names it.
//
// The first half of a frame — root_pre, the SBP locations, the residues, the nanmean and the clip — the scan state and the carry's
// initialisation are tip_kin_track.h's, shared with tip_kin.hip's tracker; so are TerHead and ter_lay, which tip_replay.hip reads.
// SCALED = true is instantiated in a translation unit of its own (tip_terrain_scaled.hip, which includes this file for the templates
// and defines TIP_TERRAIN_SCALED_TU), so that the unscaled kernels are compiled alone, as they were before there was a scale.
#include "tip_kin_track.h"

namespace tip {

namespace tr {
constexpr int MAX_D = 16, MAX_GRID = 4096, MAX_REGIONS = 65535, TICK_LEN = 50;      // :77
constexpr unsigned D2_INIT = 10000;                                                   // confidence -100 (:120)
constexpr double EPS_H = 0.1, FORCE = 20.0, PELVIS = 0.2, W0 = 10.0, IK_LO = 0.05, IK_HI = 0.5;      // :138, :124, :125, :122, :358, :353
}  // namespace tr

// The leg chains of the table: body indices of hip, knee, ankle and of the hip's parent, and the columns of s_rest the three joints
// occupy; ok = three spherical links below a parent.
struct TerChain {
    int pa, hip, knee, ank, col[3];
    bool ok;
};
__device__ __forceinline__ TerChain ter_chain(const KinSkel& sk, int L, int ank) {
    TerChain c;
    c.ank = ank, c.ok = false, c.pa = c.hip = c.knee = 0, c.col[0] = c.col[1] = c.col[2] = 0;
    if (ank < 1 || ank > L) return c;
    const int knee = sk.link[ank - 1].parent;
    if (knee < 1 || knee >= ank) return c;
    const int hip = sk.link[knee - 1].parent;
    if (hip < 1 || hip >= knee) return c;
    const int pa = sk.link[hip - 1].parent;
    if (pa < 0 || pa >= hip) return c;
    c.pa = pa, c.hip = hip, c.knee = knee;
    const int b[3] = {hip, knee, ank};
    for (int m = 0; m < 3; ++m) {
        const int col = sk.link[b[m] - 1].state_col;
        if (col < 3 || col > kn::NQ - 3) return c;
        c.col[m] = col - 3;
    }
    c.ok = true;
    return c;
}

// SCALED: the carry's FK is the wearer's, of body scale scale[slot] (by block, as the track kernel reads it).
template <bool SCALED, typename... S>
__global__ __launch_bounds__(256) void terrain_reset_kernel(const KinSkel* __restrict__ skp, unsigned char* __restrict__ state, int n_slots,
                                                            int G, int M, const int* __restrict__ slots, int count,
                                                            const float* __restrict__ s_init, S... scale) {
    __shared__ float Fs[kn::MAX_BODIES * 7 * kn::COL];
    const KinSkel& sk = *skp;
    const int L = kin_links(sk), t = threadIdx.x, j = blockIdx.x;
    if (j >= count) return;
    const int slot = slots ? slots[j] : j;
    if (slot < 0 || slot >= n_slots) return;
    const TerLay lay = ter_lay(G, M);
    unsigned char* blk = state + (size_t)slot * lay.stride;
    TerHead& h = *reinterpret_cast<TerHead*>(blk);
    double* rh = reinterpret_cast<double*>(blk + sizeof(TerHead));
    double* rw = reinterpret_cast<double*>(blk + lay.off_w);
    unsigned* map = reinterpret_cast<unsigned*>(blk + lay.off_map);
    const float* row = s_init + (size_t)j * kn::QDQ;
    if (t == 0) {
        if constexpr (SCALED) carry_init<true>(sk, L, h.carry, row, Fs, kin_scale_ptr(scale...)[slot]);
        else carry_init(sk, L, h.carry, row, Fs);
        for (int i = 0; i < kn::SBPS; ++i)
            for (int k = 0; k < 3; ++k) h.c_prev[i][k] = 100.0;     // :53-54
        for (int i = 0; i < 2; ++i)
            for (int k = 0; k < 3; ++k) h.ik_delta[i][k] = 0.0;
        for (int i = 0; i < 3; ++i) h.tick[i] = -1;
        h.n_regions = 1, h.off_map = 0, h.regions_full = 0, h.grid_num = G, h.max_regions = M;
        for (int i = 0; i < 14; ++i) h.pad[i] = 0;
    }
    __syncthreads();
    carry_init_pq(h.carry, Fs, L, t, 256);
    for (int e = (L + 1) * 7 + t; e < kn::MAX_BODIES * 7; e += 256) h.carry.pq[e] = 0.f;      // (the whole block is defined after a reset)
    for (int e = t; e < 15; e += 256) h.carry.pad[e] = 0;
    for (int e = t; e < M; e += 256) rh[e] = 0.0, rw[e] = e == 0 ? tr::W0 : 0.0;      // :121-122
    const size_t cells = (lay.stride - lay.off_map) / 4;
    for (size_t e = t; e < cells; e += 256) map[e] = tr::D2_INIT;   // region 0, confidence -100 (:119-120)
}

__device__ __forceinline__ double ter_norm3(const double* v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
__device__ __forceinline__ bool ter_active(const double* c) { return ter_norm3(c) < 100.0; }      // is_c_loc_active (:19-21); false for a NaN
__device__ __forceinline__ bool ter_all_nan(const double* v) { return v[0] != v[0] && v[1] != v[1] && v[2] != v[2]; }
__device__ __forceinline__ void ter_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
}
// data_utils.normalize (:551-553)
__device__ __forceinline__ void ter_unit(const double* v, double* o) {
    const double n = ter_norm3(v) + 1e-4;
    o[0] = v[0] / n, o[1] = v[1] / n, o[2] = v[2] / n;
}
__device__ __forceinline__ double ter_angle(const double* a, const double* b) {
    return acos(kin_clip(a[0] * b[0] + a[1] * b[1] + a[2] * b[2], -1.0, 1.0));
}
// scipy's Rotation.from_quat(q).as_rotvec()
__device__ __forceinline__ void ter_q2a(const double* qi, double* a) {
    const double n = sqrt(qi[0] * qi[0] + qi[1] * qi[1] + qi[2] * qi[2] + qi[3] * qi[3]);
    double q[4] = {qi[0] / n, qi[1] / n, qi[2] / n, qi[3] / n};
    if (q[3] < 0.0) q[0] = -q[0], q[1] = -q[1], q[2] = -q[2], q[3] = -q[3];
    const double ang = 2.0 * atan2(ter_norm3(q), q[3]);
    double s;
    if (ang <= 1e-3) {
        const double a2 = ang * ang;
        s = 2.0 + a2 / 12.0 + 7.0 * a2 * a2 / 2880.0;
    } else {
        s = ang / sin(ang / 2.0);
    }
    a[0] = s * q[0], a[1] = s * q[1], a[2] = s * q[2];
}

// leg_two_joint_ik_keep_foot_pointing over two_joint_ik (data_utils.py:556-630) on the link frames: positions a, b, c of hip, knee and
// ankle, their orientations and the parent's; out: the axis-angles of the three new local rotations.
__device__ void ter_leg_ik(const double* a, const double* b, const double* c, const double* qpa, const double* qa, const double* qb,
                           const double* qc, const double* c_delta, double* aa_out) {
    double pinv[4], qainv[4], target[3], ba[3], cb[3], ca[3], ta[3], ab[3];
    kin_conj(qpa, pinv);
    kin_conj(qa, qainv);
    for (int k = 0; k < 3; ++k) {
        target[k] = c[k] + c_delta[k];
        ba[k] = b[k] - a[k], cb[k] = c[k] - b[k], ca[k] = c[k] - a[k], ab[k] = a[k] - b[k];
    }
    for (int k = 0; k < 3; ++k) ta[k] = target[k] - a[k];
    const double eps = 0.01;
    const double lab = ter_norm3(ba), lcb = ter_norm3(cb);
    const double lat = kin_clip(ter_norm3(ta), eps, lab + lcb - eps);
    double n_ca[3], n_ba[3], n_ab[3], n_cb[3], n_ta[3];
    ter_unit(ca, n_ca), ter_unit(ba, n_ba), ter_unit(ab, n_ab), ter_unit(cb, n_cb), ter_unit(ta, n_ta);
    const double ac_ab_0 = ter_angle(n_ca, n_ba);
    const double ba_bc_0 = ter_angle(n_ab, n_cb);
    const double ac_at_0 = ter_angle(n_ca, n_ta);
    const double ac_ab_1 = acos(kin_clip((lcb * lcb - lab * lab - lat * lat) / (-2.0 * lab * lat), -1.0, 1.0));
    const double ba_bc_1 = acos(kin_clip((lat * lat - lab * lab - lcb * lcb) / (-2.0 * lab * lcb), -1.0, 1.0));
    const double up[3] = {0.0, 0.0, 1.0};
    double d[3], x0[3], x1[3], ax0g[3], ax1g[3], ax0l[3], ax1l[3];
    qrot<double>(qa, up, d);
    ter_cross(ca, d, x0);
    ter_unit(x0, ax0g);
    ter_cross(ca, ta, x1);
    ter_unit(x1, ax1g);
    qrot<double>(pinv, ax0g, ax0l);
    qrot<double>(qainv, ax1g, ax1l);
    double r0[4], r1[4], r2[4];
    const double t0 = ac_ab_1 - ac_ab_0, t1 = ba_bc_1 - ba_bc_0;
    a2q<double>(ax0l[0] * t0, ax0l[1] * t0, ax0l[2] * t0, r0);
    a2q<double>(ax0l[0] * t1, ax0l[1] * t1, ax0l[2] * t1, r1);
    a2q<double>(ax1l[0] * ac_at_0, ax1l[1] * ac_at_0, ax1l[2] * ac_at_0, r2);
    double a_l[4], b_l[4], r02[4], a_l1[4], b_l1[4], a_g1[4], b_g1[4], b_g1inv[4], c_l1[4];
    qmul<double>(pinv, qa, a_l);
    qmul<double>(qainv, qb, b_l);
    qmul<double>(r0, r2, r02);
    qmul<double>(a_l, r02, a_l1);
    qmul<double>(b_l, r1, b_l1);
    qmul<double>(qpa, a_l1, a_g1);
    qmul<double>(a_g1, b_l1, b_g1);
    kin_conj(b_g1, b_g1inv);
    qmul<double>(b_g1inv, qc, c_l1);
    ter_q2a(a_l1, aa_out), ter_q2a(b_l1, aa_out + 3), ter_q2a(c_l1, aa_out + 6);
}

// What the wave keeps of a slot's map state while it steps (the same values in every lane).
struct TerScan {
    double cp[kn::SBPS][3];
    int tick[3];
    int n_regions, off_map, regions_full;
};

// update_height_map_new (:140-262) for SBP `i` with tick `ti`, on c_locs_prev.  Called by the whole wave under uniform control flow.
__device__ double terrain_update(TerScan& s, double* rh, double* rw, unsigned* map, int G, int M, int D, double gs, int i, int ti,
                                 int lane) {
    const double* c = s.cp[i];
    if (!ter_active(c)) return 0.0;
    if (s.tick[ti] < 0) {
        s.tick[ti] = tr::TICK_LEN;
        return 0.0;
    }
    if (s.tick[ti] > 0) return 0.0;
    s.tick[ti] = -1;                                                // every way out from here leaves the tick at -1
    const double h = c[2];
    const double fx = rint(c[0] / gs) + (double)(G / 2), fy = rint(c[1] / gs) + (double)(G / 2);      // round(): half to even
    if (!(fx - D >= 0.0 && fx + D <= (double)G && fy - D >= 0.0 && fy + D <= (double)G)) {
        s.off_map += 1;
        return 0.0;
    }
    const int x0 = (int)fx - D, y0 = (int)fy - D, side = 2 * D;
    // check_neighboring_area_for_similar_height_region (:174-197)
    int r;
    if (h < rh[0] + tr::EPS_H) {
        r = 0;
    } else {
        double best = __builtin_inf();
        int bi = 0x7fffffff;
        for (int e = lane; e < side * side; e += kn::LANES) {
            const int a = e / side, b = e - a * side;
            const int reg = (int)(map[(size_t)(x0 + a) * G + (y0 + b)] >> 16);
            if (reg >= M) continue;
            const double diff = fabs(rh[reg] - h);
            if (diff < best || (diff == best && reg < bi)) best = diff, bi = reg;
        }
        for (int m = kn::LANES / 2; m > 0; m >>= 1) {
            const double ob = __shfl_xor(best, m, kn::LANES);
            const int oi = __shfl_xor(bi, m, kn::LANES);
            if (ob < best || (ob == best && oi < bi)) best = ob, bi = oi;
        }
        r = best < tr::EPS_H ? bi : -1;
    }
    double new_h;
    if (r < 0) {
        if (s.n_regions >= M) {
            s.regions_full += 1;
            return 0.0;
        }
        r = s.n_regions;
        s.n_regions += 1;
        new_h = h;
        __syncthreads();
        if (lane == 0) rh[r] = h, rw[r] = tr::W0;
    } else {
        const double old_h = rh[r], old_w = rw[r];
        new_h = (old_h * old_w * 1.0 + h * 1.0) / (old_w * 1.0 + 1.0);      // temporal_inertial = 1 (:123, :248-249)
        __syncthreads();
        if (lane == 0) rh[r] = new_h, rw[r] = old_w + 1.0;
    }
    // update_height_region_map_and_confidence_map (:148-172)
    for (int e = lane; e < side * side; e += kn::LANES) {
        const int a = e / side, b = e - a * side;
        const unsigned d2 = (unsigned)((a - D) * (a - D) + (b - D) * (b - D));
        unsigned* cell = map + (size_t)(x0 + a) * G + (y0 + b);
        if (!((*cell & 0xffffu) < d2)) *cell = ((unsigned)r << 16) | d2;
    }
    __syncthreads();
    return new_h - h;                                               // region_height[map[centre]] - h: the centre cell (d2 = 0) is r's
}

// SCALED: the sequence's body scale is scale[slot], read once per launch: the FK of every row — the poses the residues are taken on, the
// pelvis test's and the link frames the IK solves on — is the wearer's.  Nothing else is scaled.  A scale that kin_scale_ok refuses makes
// the sequence's rows NaN with fire -1 and leaves its block, the map included, alone.
template <bool SCALED, typename... S>
__global__ __launch_bounds__(64) void terrain_track_kernel(const KinSkel* __restrict__ skp, unsigned char* __restrict__ state, int n_slots,
                                                           int G, int M, int D, double gs, const int* __restrict__ slots,
                                                           const long long* __restrict__ begin, const long long* __restrict__ end,
                                                           long long n_rows, const float* __restrict__ s_rest,
                                                           const float* __restrict__ c_t, int nc, const unsigned char* __restrict__ valid,
                                                           int flags, float* __restrict__ root_out, float* __restrict__ viz_out,
                                                           float* __restrict__ q_hist, int* __restrict__ fire_out, S... scale) {
    __shared__ float Fs[kn::MAX_BODIES * 7 * kn::COL];
    __shared__ float Js[18 * kn::COL];                              // link-frame positions of hip, knee, ankle of both legs
    const KinSkel& sk = *skp;
    const int L = kin_links(sk), lane = threadIdx.x, per = (L + 1) * 7;
    int slot;
    long long r0, r1;
    if (!track_range(slots, begin, end, blockIdx.x, n_slots, n_rows, slot, r0, r1)) return;      // (uniform over the wave: every return is)
    const TerLay lay = ter_lay(G, M);
    unsigned char* blk = state + (size_t)slot * lay.stride;
    TerHead& hd = *reinterpret_cast<TerHead*>(blk);
    if (hd.grid_num != G || hd.max_regions != M) return;          // not the layout the reset gave this block
    float sc = 1.f;
    if constexpr (SCALED) {
        sc = kin_scale_ptr(scale...)[slot];
        if (!kin_scale_ok(sc)) {
            const float nanf = __builtin_nanf("");
            for (long long e = r0 * 3 + lane; e < r1 * 3; e += kn::LANES) root_out[e] = nanf;
            for (long long e = r0 * 15 + lane; e < r1 * 15; e += kn::LANES) viz_out[e] = nanf;
            for (long long e = r0 * 54 + lane; e < r1 * 54; e += kn::LANES) q_hist[e] = nanf;
            for (long long e = r0 + lane; e < r1; e += kn::LANES) fire_out[e] = -1;
            return;
        }
    }
    double* rh = reinterpret_cast<double*>(blk + sizeof(TerHead));
    double* rw = reinterpret_cast<double*>(blk + lay.off_w);
    unsigned* map = reinterpret_cast<unsigned*>(blk + lay.off_map);
    KinCarry& cr = hd.carry;
    const int n_sbps = nc / 4;
    const bool multi = (flags & 1) != 0;
    int body[kn::SBPS];
    sbp_bodies(sk, L, body);
    const TerChain chain[2] = {ter_chain(sk, L, body[0]), ter_chain(sk, L, body[1])};
    float* F = Fs + lane;

    // the scan state, the same in every lane: the residues read are the feet's and, for the IK, the root's
    SbpScan<3> st;
    double delta[2][3];
    TerScan s;
    sbp_scan_load(st, cr, body);
    for (int i = 0; i < kn::SBPS; ++i)
        for (int k = 0; k < 3; ++k) s.cp[i][k] = hd.c_prev[i][k];
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 3; ++k) delta[i][k] = hd.ik_delta[i][k];
    for (int i = 0; i < 3; ++i) s.tick[i] = hd.tick[i];
    s.n_regions = hd.n_regions, s.off_map = hd.off_map, s.regions_full = hd.regions_full;
    if (s.n_regions < 1) s.n_regions = 1;
    if (s.n_regions > M) s.n_regions = M;
    __syncthreads();

    for (long long t0 = r0; t0 < r1; t0 += kn::LANES) {
        const long long left = r1 - t0;
        const int cnt = left < kn::LANES ? (int)left : kn::LANES;
        if (lane < cnt && (!valid || valid[t0 + lane])) {
            fk_frames_of<SCALED>(sk, L, s_rest + (size_t)(t0 + lane) * kn::REST, 0.f, 0.f, 0.f, sc, F);
            for (int g = 0; g < 2; ++g) {
                const int b3[3] = {chain[g].hip, chain[g].knee, chain[g].ank};
                for (int m = 0; m < 3; ++m)
                    for (int k = 0; k < 3; ++k) Js[(9 * g + 3 * m + k) * kn::COL + lane] = F[(7 * b3[m] + k) * kn::COL];
            }
            fk_to_com_of<SCALED>(sk, L, sc, F);
        }
        __syncthreads();
        int last = -1;
        for (int j = 0; j < cnt; ++j) {
            const size_t row = (size_t)(t0 + j);
            float* ro = root_out + row * 3;
            float* vo = viz_out + row * 15;
            const float* sr = s_rest + row * kn::REST;
            if (valid && !valid[row]) {                              // what the runner returns while it primes: the carry's root, 100s
                for (int k = 0; k < 3; ++k)
                    if (lane == k) ro[k] = (float)st.root[k];
                if (lane < 15) vo[lane] = 100.f;
                if (lane < 54) q_hist[row * 54 + lane] = sr[lane];
                if (lane == 0) fire_out[row] = -1;
                continue;
            }
            double pre[3], cl[kn::SBPS][3], res[3][3], vr[3];
            sbp_step<3>(st, body, sr, c_t + row * nc, n_sbps, Fs, j, pre, cl, res, vr);      // :441-461
            vr[2] = 0.0;                                             // the terrain corrects the height, not the SBPs (:462)
            for (int i = 0; i < kn::SBPS; ++i)
                for (int k = 0; k < 3; ++k) cl[i][k] = cl[i][k] - vr[k] * kn::DT;      // :463, the inactive 100s included
            // update_sbp_establishing_height_ticks (:264-277)
            for (int ti = 0; ti < 3; ++ti) {
                if (s.tick[ti] < 0) continue;
                s.tick[ti] -= 1;
                if (!ter_active(cl[sbp_of_res(ti)]) && ter_active(s.cp[sbp_of_res(ti)])) s.tick[ti] = 0;
            }
            for (int ti = 0; ti < 2; ++ti) {                         // :467-472
                const double d = terrain_update(s, rh, rw, map, G, M, D, gs, sbp_of_res(ti), ti, lane);
                vr[2] += -d * tr::FORCE;
            }
            if (multi) {
                const double dx = (double)Fs[(7 * body[4] + 0) * kn::COL + j]
                                  - ((double)Fs[(7 * body[0] + 0) * kn::COL + j] + (double)Fs[(7 * body[1] + 0) * kn::COL + j]) / 2.0;
                const double dy = (double)Fs[(7 * body[4] + 1) * kn::COL + j]
                                  - ((double)Fs[(7 * body[0] + 1) * kn::COL + j] + (double)Fs[(7 * body[1] + 1) * kn::COL + j]) / 2.0;
                if (sqrt(dx * dx + dy * dy) > tr::PELVIS) terrain_update(s, rh, rw, map, G, M, D, gs, 4, 2, lane);      // :475-480
            }
            // correct_joint_q_for_history_feedback (:334-382) for lankle, then rankle
            double aa[2][9];
            bool fired[2] = {false, false};
            if (multi) {
                for (int g = 0; g < 2; ++g) {
                    if (ter_all_nan(res[g]) || ter_all_nan(res[2])) {
                        for (int k = 0; k < 3; ++k) delta[g][k] = 0.0;
                        continue;
                    }
                    double corr[3];
                    for (int k = 0; k < 3; ++k) {
                        delta[g][k] += (res[g][k] - res[2][k]) * kn::DT;
                        corr[k] = -delta[g][k];
                    }
                    const double nrm = ter_norm3(corr);
                    if (nrm > tr::IK_HI) {
                        for (int k = 0; k < 3; ++k) delta[g][k] = 0.0;
                        continue;
                    }
                    if (nrm > tr::IK_LO && chain[g].ok) {
                        const TerChain& ch = chain[g];
                        double pa[3], pb[3], pc[3], qpa[4], qa[4], qb[4], qc[4];
                        for (int k = 0; k < 3; ++k) {
                            pa[k] = (double)Js[(9 * g + k) * kn::COL + j];
                            pb[k] = (double)Js[(9 * g + 3 + k) * kn::COL + j];
                            pc[k] = (double)Js[(9 * g + 6 + k) * kn::COL + j];
                        }
                        for (int k = 0; k < 4; ++k) {
                            qpa[k] = (double)Fs[(7 * ch.pa + 3 + k) * kn::COL + j];
                            qa[k] = (double)Fs[(7 * ch.hip + 3 + k) * kn::COL + j];
                            qb[k] = (double)Fs[(7 * ch.knee + 3 + k) * kn::COL + j];
                            qc[k] = (double)Fs[(7 * ch.ank + 3 + k) * kn::COL + j];
                        }
                        ter_leg_ik(pa, pb, pc, qpa, qa, qb, qc, corr, aa[g]);
                        fired[g] = true;
                    }
                }
            }
            // :489-496
            for (int k = 0; k < 3; ++k) st.root[k] = pre[k] - vr[k] * kn::DT;
            for (int k = 0; k < 3; ++k)
                if (lane == k) ro[k] = (float)st.root[k];
            for (int i = 0; i < kn::SBPS; ++i)
                for (int k = 0; k < 3; ++k)
                    if (lane == 3 * i + k) vo[3 * i + k] = (float)cl[i][k];
            if (lane < 54) {
                float v = sr[lane];
                for (int g = 0; g < 2; ++g)
                    if (fired[g])
                        for (int m = 0; m < 3; ++m)
                            for (int k = 0; k < 3; ++k)
                                if (lane == chain[g].col[m] + k) v = (float)aa[g][3 * m + k];
                q_hist[row * 54 + lane] = v;
            }
            if (lane == 0) fire_out[row] = (fired[0] || fired[1]) ? slot : -1;
            for (int i = 0; i < kn::SBPS; ++i)
                for (int k = 0; k < 3; ++k) s.cp[i][k] = cl[i][k];
            sbp_advance(st, body, sr, Fs, j);
            last = j;
        }
        carry_store_pq(cr, Fs, per, last, lane);
        __syncthreads();
    }
    if (lane == 0) {
        sbp_scan_store(st, cr);
        for (int i = 0; i < kn::SBPS; ++i)
            for (int k = 0; k < 3; ++k) hd.c_prev[i][k] = s.cp[i][k];
        for (int i = 0; i < 2; ++i)
            for (int k = 0; k < 3; ++k) hd.ik_delta[i][k] = delta[i][k];
        for (int i = 0; i < 3; ++i) hd.tick[i] = s.tick[i];
        hd.n_regions = s.n_regions, hd.off_map = s.off_map, hd.regions_full = s.regions_full;
    }
}

}  // namespace tip

static bool ter_bad_shape(int n_slots, int grid_num, int max_regions) {
    using namespace tip;
    return tip_bad_count(n_slots) || grid_num < 2 || grid_num > tr::MAX_GRID || max_regions < 1 || max_regions > tr::MAX_REGIONS;
}

#ifndef TIP_TERRAIN_SCALED_TU
using namespace tip;

extern "C" {

int tip_terrain_state_bytes(int n_slots, int grid_num, int max_regions, size_t* bytes) {
    if (!bytes || ter_bad_shape(n_slots, grid_num, max_regions)) return TIP_ERR_INVALID_ARG;
    *bytes = (size_t)n_slots * ter_lay(grid_num, max_regions).stride;
    return TIP_OK;
}

int tip_terrain_reset(const void* skel, void* state, int n_slots, int grid_num, int max_regions, const int* slots, int count,
                      const float* s_init, tip_stream_t stream) {
    if (!skel || !state || ter_bad_shape(n_slots, grid_num, max_regions) || count < 0 || (count > 0 && !s_init)
        || reinterpret_cast<uintptr_t>(state) % 8)
        return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0) return TIP_OK;
    hipLaunchKernelGGL((terrain_reset_kernel<false>), dim3(count), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), static_cast<unsigned char*>(state), n_slots, grid_num, max_regions, slots, count,
                       s_init);
    return tip_launch_status();
}

int tip_terrain_track(const void* skel, void* state, int n_slots, int grid_num, int max_regions, int diffuse_region, double grid_size,
                      const int* slots, const long long* begin, const long long* end, int count, long long n_rows, const float* s_rest,
                      const float* c_t, int nc, const unsigned char* valid, int flags, float* root_out, float* viz_out,
                      float* q_hist_out, int* fire_out, tip_stream_t stream) {
    if (!skel || !state || ter_bad_shape(n_slots, grid_num, max_regions) || count < 0 || tip_bad_rows(n_rows)
        || (nc != 8 && nc != 20) || reinterpret_cast<uintptr_t>(state) % 8 || diffuse_region < 1 || diffuse_region > tr::MAX_D
        || !(grid_size > 0.0) || !(grid_size < 1e6) || (flags & ~1) || ((flags & 1) && nc != 20))
        return TIP_ERR_INVALID_ARG;
    if (count > 0 && (!begin || !end || !s_rest || !c_t || !root_out || !viz_out || !q_hist_out || !fire_out)) return TIP_ERR_INVALID_ARG;
    if (count == 0 || n_slots == 0 || n_rows == 0) return TIP_OK;
    hipLaunchKernelGGL((terrain_track_kernel<false>), dim3(count), dim3(kn::LANES), 0, static_cast<hipStream_t>(stream),
                       static_cast<const KinSkel*>(skel), static_cast<unsigned char*>(state), n_slots, grid_num, max_regions, diffuse_region,
                       grid_size, slots, begin, end, n_rows, s_rest, c_t, nc, valid, flags, root_out, viz_out, q_hist_out, fire_out);
    return tip_launch_status();
}

}  // extern "C"
#endif  // TIP_TERRAIN_SCALED_TU
