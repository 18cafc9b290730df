"""numpy restatement of what tip_amd.terrain runs on the device (csrc/tip_terrain.hip), in any dtype: the tail of RTRunner.step
(real_time_runner.py:451-496) — the root track of tests/kin_oracle.py with the height-region map (:140-262), the "establishing
height" ticks (:264-277), the vertical root correction and the two-joint leg IK (:334-382; data_utils.py:556-630) whose pose is fed
back.  fp64 is the oracle; float32 is the same statements in float32, which is what the GPU tests take their noise floor from.  It
imports nothing of tip_amd.

Beside the outputs it returns a TRACE: every decision taken (`events`, one tuple per decision, in order) and, per kind of decision, the
smallest distance of the deciding quantity from its threshold (`margins`), so that a fixture can show its decisions are not at the
mercy of rounding.  Where the reference leaves a case open, the choices are those of include/tip_hip.h ("terrain"): off-map and
region overflow write nothing, return 0, set the tick to -1 and are counted; a tie goes to the lower region index.

The leg chain comes from the skeleton table (ankle = the SBP body, knee and hip its parent and grandparent, then the hip's parent),
which on the reference's character is ik_chain_map_bullet / ik_chain_map_nimble_joint (:81-95)."""
import warnings

import numpy as np

import kin_oracle as ko

DT = ko.DT
TICK_LEN, EPS_H, FORCE, PELVIS, W0, IK_LO, IK_HI = 50, 0.1, 20.0, 0.2, 10.0, 0.05, 0.5      # :77, :138, :124, :125, :122, :358, :353
D2_INIT = 10000                                                                             # confidence -100 (:120)
LINKS = (("lankle", 0), ("rankle", 1), ("root", 4))                                         # tick order; SBP index (:56-62)
MARGINS = ("half", "eps", "tie", "ik_lo", "ik_hi", "h0", "dist")
BRANCHES = ("merge", "new", "region0", "expiry", "ik_fire", "ik_small", "ik_reset", "pelvis_near", "off_map", "regions_full")


def grid_num(map_bound, grid_size):
    return int(map_bound / grid_size) * 2                   # :115


def diffuse_region(grid_size):
    return round(0.5 / grid_size)                           # :128


def chains(table):
    """Per leg: (parent body, hip, knee, ankle bodies), (the three joints' first columns in s_rest[:54])."""
    out = []
    for i in range(2):
        ank = int(table["sbp"][i])
        knee = int(table["parent"][ank - 1])
        hip = int(table["parent"][knee - 1])
        pa = int(table["parent"][hip - 1])
        cols = [int(table["state_col"][b - 1]) - 3 for b in (hip, knee, ank)]
        assert ank > knee > hip > pa >= 0 and min(cols) >= 0, (pa, hip, knee, ank, cols)
        out.append(((pa, hip, knee, ank), cols))
    return out


def q2a(q, f):
    """scipy's Rotation.from_quat(q).as_rotvec(): normalise, w >= 0, 2 atan2, the series below 1e-3."""
    q = np.asarray(q, dtype=f)
    q = q / np.sqrt((q * q).sum())
    if q[3] < 0:
        q = -q
    ang = f(2) * np.arctan2(np.sqrt((q[:3] * q[:3]).sum()), q[3])
    if ang <= f(1e-3):
        a2 = ang * ang
        s = f(2) + a2 / f(12) + f(7) * a2 * a2 / f(2880)
    else:
        s = ang / np.sin(ang / f(2))
    return (s * q[:3]).astype(f)


def _norm(v):
    return np.sqrt((v * v).sum())


def _unit(v, f):
    return v / (_norm(v) + f(1e-4))                         # data_utils.normalize (:551-553)


def _angle(a, b, f):
    return np.arccos(np.clip((a * b).sum(), f(-1), f(1)))


def leg_ik(jf, chain, c_delta, f):
    """leg_two_joint_ik_keep_foot_pointing over two_joint_ik (data_utils.py:556-630) on the link frames jf [L + 1, 7]: the axis-angles
    of the new local rotations of hip, knee and ankle."""
    pa, hip, knee, ank = chain
    a, b, c = jf[hip, :3], jf[knee, :3], jf[ank, :3]
    qpa, qa, qb, qc = jf[pa, 3:], jf[hip, 3:], jf[knee, 3:], jf[ank, 3:]
    pinv, qainv = ko.qconj(qpa), ko.qconj(qa)
    target = c + c_delta
    eps = f(0.01)
    lab, lcb = _norm(b - a), _norm(c - b)
    lat = np.clip(_norm(target - a), eps, lab + lcb - eps)
    ac_ab_0 = _angle(_unit(c - a, f), _unit(b - a, f), f)
    ba_bc_0 = _angle(_unit(a - b, f), _unit(c - b, f), f)
    ac_at_0 = _angle(_unit(c - a, f), _unit(target - a, f), f)
    ac_ab_1 = np.arccos(np.clip((lcb * lcb - lab * lab - lat * lat) / (f(-2) * lab * lat), f(-1), f(1)))
    ba_bc_1 = np.arccos(np.clip((lat * lat - lab * lab - lcb * lcb) / (f(-2) * lab * lcb), f(-1), f(1)))
    d = ko.qrot(qa, np.array([0, 0, 1], dtype=f))
    ax0g = _unit(np.cross(c - a, d), f)
    ax1g = _unit(np.cross(c - a, target - a), f)
    ax0l, ax1l = ko.qrot(pinv, ax0g), ko.qrot(qainv, ax1g)
    r0, r1, r2 = ko.a2q(ax0l * (ac_ab_1 - ac_ab_0), f), ko.a2q(ax0l * (ba_bc_1 - ba_bc_0), f), ko.a2q(ax1l * ac_at_0, f)
    a_l, b_l = ko.qmul(pinv, qa), ko.qmul(qainv, qb)
    a_l1, b_l1 = ko.qmul(a_l, ko.qmul(r0, r2)), ko.qmul(b_l, r1)
    b_g1 = ko.qmul(ko.qmul(qpa, a_l1), b_l1)
    c_l1 = ko.qmul(ko.qconj(b_g1), qc)
    return np.concatenate([q2a(a_l1, f), q2a(b_l1, f), q2a(c_l1, f)])


class State:
    """One sequence's state: the tracker's carry and what RTRunner.__init__ sets (:53-138)."""

    def __init__(self, table, s_init, G, max_regions, dtype):
        f = dtype
        s_init = np.asarray(s_init, dtype=f)
        self.root = s_init[:3].copy()
        self.pq_prev = ko.fk(table, np.concatenate([np.zeros(3, dtype=f), s_init[3:57]])[None], f)[0][0]      # about the root
        self.a_prev, self.has_prev = np.zeros(3, dtype=f), False
        self.c_prev = np.full((5, 3), 100, dtype=f)
        self.ticks = [-1, -1, -1]
        self.ik_deltas = np.zeros((2, 3), dtype=f)
        self.region_height, self.region_weight = [f(0)], [f(W0)]
        self.region_map = np.zeros((G, G), dtype=np.int64)
        self.d2_map = np.full((G, G), D2_INIT, dtype=np.int64)
        self.off_map = self.regions_full = 0
        self.max_regions = max_regions

    @property
    def height_map(self):
        return np.asarray(self.region_height, dtype=np.float64)[self.region_map]


def _active(c):
    return bool(_norm(c) < 100)                             # is_c_loc_active (:19-21); False for a NaN


def _margin(tr, key, value):
    value = float(value)
    if np.isfinite(value):
        tr["margins"][key] = min(tr["margins"][key], value)


def _update(st, ti, sbp_i, G, D, gs, f, tr, row, by_expiry):
    """update_height_map_new (:140-262) on c_locs_prev."""
    c = st.c_prev[sbp_i]
    if not _active(c):
        return f(0)
    if st.ticks[ti] < 0:
        st.ticks[ti] = TICK_LEN
        return f(0)
    if st.ticks[ti] > 0:
        return f(0)
    st.ticks[ti] = -1
    if by_expiry:
        tr["counts"]["expiry"] += 1
    h = c[2]
    ux, uy = c[0] / f(gs), c[1] / f(gs)
    fx, fy = np.rint(ux) + G // 2, np.rint(uy) + G // 2
    for u in (ux, uy):
        _margin(tr, "half", abs(abs(float(u) - np.floor(float(u))) - 0.5))
    if not (fx - D >= 0 and fx + D <= G and fy - D >= 0 and fy + D <= G):
        st.off_map += 1
        tr["counts"]["off_map"] += 1
        tr["events"].append((row, ti, "off_map", -1, -1, -1))
        return f(0)
    x0, y0 = int(fx) - D, int(fy) - D
    old = st.region_map[x0:x0 + 2 * D, y0:y0 + 2 * D]
    _margin(tr, "h0", abs(float(h) - (float(st.region_height[0]) + EPS_H)))
    if h < st.region_height[0] + f(EPS_H):                  # :183-184
        r = 0
        tr["counts"]["region0"] += 1
    else:
        present = sorted(set(int(v) for v in old.flatten()))
        diffs = np.array([abs(st.region_height[p] - h) for p in present], dtype=f)
        k = int(np.argmin(diffs))                           # the first of equal minima: the lower index
        _margin(tr, "eps", abs(float(diffs[k]) - EPS_H))
        if len(present) > 1:
            _margin(tr, "tie", np.sort(diffs.astype(np.float64))[1] - float(diffs[k]))
        r = present[k] if diffs[k] < f(EPS_H) else -1
    if r < 0:
        if len(st.region_height) >= st.max_regions:
            st.regions_full += 1
            tr["counts"]["regions_full"] += 1
            tr["events"].append((row, ti, "regions_full", int(fx), int(fy), -1))
            return f(0)
        r = len(st.region_height)
        st.region_height.append(h)
        st.region_weight.append(f(W0))
        tr["counts"]["new"] += 1
        kind = "new"
    else:
        old_h, old_w = st.region_height[r], st.region_weight[r]
        st.region_weight[r] = old_w + f(1)
        st.region_height[r] = (old_h * old_w * f(1) + h * f(1)) / (old_w * f(1) + f(1))      # :242-249
        if r:
            tr["counts"]["merge"] += 1
        kind = "merge"
    i = np.arange(-D, D)
    d2 = i[:, None] ** 2 + i[None, :] ** 2
    keep = st.d2_map[x0:x0 + 2 * D, y0:y0 + 2 * D] < d2     # confidence_old > confidence_new (:156-161)
    st.region_map[x0:x0 + 2 * D, y0:y0 + 2 * D] = np.where(keep, old, r)
    st.d2_map[x0:x0 + 2 * D, y0:y0 + 2 * D] = np.minimum(st.d2_map[x0:x0 + 2 * D, y0:y0 + 2 * D], d2)
    tr["events"].append((row, ti, kind, int(fx), int(fy), r))
    return st.region_height[st.region_map[int(fx), int(fy)]] - h


def new_trace():
    return {"events": [], "margins": {k: np.inf for k in MARGINS}, "counts": {k: 0 for k in BRANCHES}}


def step(table, st, s_rest_row, c_t_row, G, D, gs, multi_sbp, f, tr, row=0):
    """One valid frame on `st`: (root [3], viz_locs [5, 3], q_hist [54], fired)."""
    sr, ct = np.asarray(s_rest_row, dtype=f), np.asarray(c_t_row, dtype=f)
    n_sbps, dt = ct.shape[0] // 4, f(DT)
    a = sr[54:57]
    v = f(2) * a - st.a_prev if st.has_prev else a
    pre = st.root + v * dt
    g, jf = ko.fk(table, np.concatenate([np.zeros(3, dtype=f), sr[:54]])[None], f)
    g, jf = g[0], jf[0]
    c_locs = np.full((5, 3), 100, dtype=f)
    res = np.full((5, 3), np.nan, dtype=f)
    for i in range(n_sbps):
        if ct[4 * i] == 0:
            continue
        b = int(table["sbp"][i])
        x1, q1 = st.pq_prev[b, :3] + st.root, st.pq_prev[b, 3:]
        x2, q2 = g[b, :3] + pre, g[b, 3:]
        sol = ct[4 * i + 1:4 * i + 4]
        c_locs[i] = x2 + sol
        sub = q2 - q1 if _norm(q2 - q1) < _norm(q2 + q1) else q2 + q1
        w = (f(2) * ko.qmul(sub, ko.qconj(q2)) / dt)[:3]
        res[i] = np.cross(w, sol) + (x2 - x1) / dt
    if np.isnan(res[:2]).all():
        vr = np.zeros(3, dtype=f)
    else:
        vr = np.clip(np.nanmean(res[:2], axis=0).astype(f), f(-0.5), f(0.5))
    vr[2] = 0                                               # :462
    c_locs = c_locs - vr * dt                               # :463
    expired = [False] * 3
    for ti, (_, i) in enumerate(LINKS):                     # :264-277
        if st.ticks[ti] < 0:
            continue
        st.ticks[ti] -= 1
        expired[ti] = st.ticks[ti] == 0
        if not _active(c_locs[i]) and _active(st.c_prev[i]):
            st.ticks[ti] = 0
            expired[ti] = False
    for ti in (0, 1):                                       # :467-472
        d = _update(st, ti, LINKS[ti][1], G, D, gs, f, tr, row, expired[ti])
        vr[2] += -d * f(FORCE)
    fired = False
    q_hist = sr[:54].copy()
    if multi_sbp:
        bl, br_, b0 = (int(table["sbp"][k]) for k in (0, 1, 4))
        dist = _norm(g[b0, :2] - (g[bl, :2] + g[br_, :2]) / f(2))      # :475-478
        _margin(tr, "dist", abs(float(dist) - PELVIS))
        if dist > f(PELVIS):
            _update(st, 2, 4, G, D, gs, f, tr, row, expired[2])
        else:
            tr["counts"]["pelvis_near"] += 1
        for leg, (chain, cols) in enumerate(chains(table)):            # :334-382
            if np.isnan(res[leg]).all() or np.isnan(res[4]).all():
                st.ik_deltas[leg] = 0
                continue
            st.ik_deltas[leg] = st.ik_deltas[leg] + (res[leg] - res[4]) * dt
            corr = -st.ik_deltas[leg]
            nrm = _norm(corr)
            _margin(tr, "ik_hi", abs(float(nrm) - IK_HI))
            _margin(tr, "ik_lo", abs(float(nrm) - IK_LO))
            if nrm > f(IK_HI):
                st.ik_deltas[leg] = 0
                tr["counts"]["ik_reset"] += 1
                tr["events"].append((row, leg, "ik_reset", -1, -1, -1))
                continue
            if nrm > f(IK_LO):
                aa = leg_ik(jf, chain, corr, f)
                for m in range(3):
                    q_hist[cols[m]:cols[m] + 3] = aa[3 * m:3 * m + 3]
                fired = True
                tr["counts"]["ik_fire"] += 1
                tr["events"].append((row, leg, "ik_fire", -1, -1, -1))
            else:
                tr["counts"]["ik_small"] += 1
    st.root = pre - vr * dt                                 # :489-496
    st.pq_prev = g
    st.a_prev, st.has_prev = a.copy(), True
    st.c_prev = c_locs.copy()
    return st.root.copy(), c_locs, q_hist, fired


def track(table, s_init, s_rest, c_t, valid, map_bound=5.0, grid_size=0.1, multi_sbp=False, max_regions=64, dtype=np.float64,
          state=None, trace=None):
    """One sequence: s_init [114], s_rest [n, 111], c_t [n, 8 | 20], valid [n] -> root [n, 3], viz_locs [n, 5, 3], q_hist [n, 54],
    fire [n] bool, the State (pass it back as `state` to go on), the trace."""
    f = dtype
    G, D = grid_num(map_bound, grid_size), diffuse_region(grid_size)
    s_rest, c_t = np.asarray(s_rest, dtype=f), np.asarray(c_t, dtype=f)
    if multi_sbp and c_t.shape[1] != 20:
        raise ValueError("terrain_oracle.track: multi_sbp needs the five-SBP model (c_t of 20 columns)")
    st = state if state is not None else State(table, s_init, G, max_regions, f)
    tr = trace if trace is not None else new_trace()
    n = s_rest.shape[0]
    root, viz = np.zeros((n, 3), dtype=f), np.full((n, 5, 3), 100, dtype=f)
    q_hist, fire = s_rest[:, :54].copy(), np.zeros(n, bool)
    ticks, n_regions = np.zeros((n, 3), dtype=np.int64), np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for t in range(n):
            if valid is None or valid[t]:
                root[t], viz[t], q_hist[t], fire[t] = step(table, st, s_rest[t], c_t[t], G, D, grid_size, multi_sbp, f, tr, t)
            else:
                root[t] = st.root
            ticks[t], n_regions[t] = st.ticks, len(st.region_height)
    tr["ticks"], tr["n_regions"] = ticks, n_regions
    return root, viz, q_hist, fire, st, tr
