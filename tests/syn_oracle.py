"""numpy restatement, in fp64, of what tip_amd.syndata runs on the device (csrc/tip_syn.hip): the reference's synthetic-data generator
(data-gen-and-viz-bullet-new.py:44-218 over data_utils.py:27-100) in its three stages — the tracked poses of a scaled character, the
six IMU readings, and the five stationary-body-point (SBP) label tracks.  FK is tests/kin_oracle.py's.  It imports nothing of
tip_amd.syndata, and has its own copy of the candidate grids.

A skeleton table is kin_oracle's dict of arrays plus imu [6]: the body indices of root, lwrist, rwrist, lknee, rknee, upperneck.
The tracked-pose block is [L, 8, 7]: slots 0-4 the SBP bodies (lankle, rankle, lwrist, rwrist, root), slots 5-7 imu[3:6]; a pose is
xyz + (x, y, z, w).  The slot of body 0 holds the root's tracked point p + Q2R(Q) ROOT_COM_OFFSET with the root's orientation."""
import numpy as np

import kin_oracle as ko

DT = 1.0 / 60                                   # constants.py:7
ACC_N = 4                                       # constants.py:8
DT_FIN_ACC = DT * ACC_N                         # constants.py:9
ROOT_COM_OFFSET = np.array([0.0, 0.1, -0.1])    # constants.py:10
NOMINAL_H = 1.7                                 # constants.py:11
V_THRES = 0.15                                  # constants.py:12
IMU_SLOTS = (4, 2, 3, 5, 6, 7)                  # root, lwrist, rwrist, lknee, rknee, upperneck among the tracked slots
SBP_CLASS = (0, 0, 1, 1, 2)                     # the grid of each SBP slot: feet, feet, wrists, wrists, pelvis


def q2r(q):
    """scipy's Rotation.from_quat(q).as_matrix() on [..., 4]: the quaternion normalised first; [..., 3, 3]."""
    q = np.asarray(q, dtype=np.float64)
    q = q / np.sqrt((q * q).sum(-1))[..., None]
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    m = np.stack([x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw),
                  2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw),
                  2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2], axis=-1)
    return m.reshape(q.shape[:-1] + (3, 3))


def grid_axes():
    """(feet, wrists, pelvis): the three axes of each class's candidate grid (data_utils.py:52-66)."""
    a = np.arange
    return ((a(-0.04, 0.05, 0.01), a(-0.04, 0.02, 0.01), a(-0.15, 0.18, 0.01)),
            (a(-0.02, 0.03, 0.01), a(-0.02, 0.03, 0.01), a(-0.02, 0.03, 0.01)),
            (a(-0.15, 0.16, 0.01), a(-0.1, 0.15, 0.01), a(-0.12, -0.04, 0.01)))


def grid_points(cls):
    """[n, 3]: np.meshgrid(lp_x, lp_y, lp_z) ravelled — point (iy nx + ix) nz + iz is (lp_x[ix], lp_y[iy], lp_z[iz])."""
    xx, yy, zz = np.meshgrid(*grid_axes()[cls])
    return np.stack((xx.ravel(), yy.ravel(), zz.ravel()), axis=1)


def scaled_table(table, scale):
    """PyBullet's globalScaling: every joint and COM offset times `scale`."""
    t = dict(table)
    t["joint_xyz"], t["com_xyz"] = np.asarray(table["joint_xyz"], dtype=np.float64) * scale, np.asarray(table["com_xyz"], dtype=np.float64) * scale
    return t


def tracked_poses(table, q, scale):
    """q [L, >= 57], one scale -> [L, 8, 7]: FK of the scaled character with the root xyz scaled too (ref_scale)."""
    q = np.array(np.asarray(q, dtype=np.float64)[:, :57])
    q[:, :3] = q[:, :3] * scale
    with np.errstate(all="ignore"):
        g = ko.fk(scaled_table(table, scale), q)[0]
        bodies = [int(b) for b in table["sbp"]] + [int(b) for b in table["imu"][3:]]
        P = g[:, bodies].copy()
        for k, b in enumerate(bodies):
            if b == 0:
                P[:, k, :3] = g[:, 0, :3] + q2r(g[:, 0, 3:]) @ ROOT_COM_OFFSET
    return P


def imu_readings(P):
    """[L, 8, 7] -> [L, 72]: six row-major rotation matrices, then six centred second differences over +-4 frames divided by
    DT_FIN_ACC^2 on rows 4 .. L - 5, the first four rows copying row 4 and the last four row L - 5."""
    L = P.shape[0]
    H = np.zeros((L, 72))
    with np.errstate(all="ignore"):
        for j, s in enumerate(IMU_SLOTS):
            H[:, 9 * j:9 * j + 9] = q2r(P[:, s, 3:]).reshape(L, 9)
            p = P[:, s, :3]
            H[ACC_N:L - ACC_N, 54 + 3 * j:57 + 3 * j] = (-2 * p[ACC_N:L - ACC_N] + p[2 * ACC_N:] + p[:L - 2 * ACC_N]) / (DT_FIN_ACC ** 2)
    H[:ACC_N, 54:] = H[ACC_N, 54:]
    H[L - ACC_N:, 54:] = H[L - ACC_N - 1, 54:]
    return H


def sbp_labels(P):
    """[L, 8, 7] -> constrs [L, 20] and a trace of [L, 5] arrays: "min" (the least residue), "gap" (the second-smallest residue minus
    it), "margin" (|min - V_THRES|); NaN on rows 0, 1, L - 2, L - 1, which carry no search.  Per frame t and body: the neighbours
    t - 1 and t + 1 give v, w (dt = 2 DT) and R = Q2R(q2); the residue of candidate p is |w x Rp + v| + 0.2 |Rp - (r_prev - v dt)| +
    0.02 |Rp|, the middle term absent without a previous solution; the first index of the least residue is the solution if that
    residue is below V_THRES, and no solution otherwise.  np.argmin answers the first NaN, and NaN < V_THRES is false."""
    L = P.shape[0]
    C = np.zeros((L, 20))
    tr = {k: np.full((L, 5), np.nan) for k in ("min", "gap", "margin")}
    dt = 2 * DT
    with np.errstate(all="ignore"):
        for b in range(5):
            lps = grid_points(SBP_CLASS[b])
            r_prev = None
            for t in range(2, L - 2):
                x1, q1, x2, q2 = P[t - 1, b, :3], P[t - 1, b, 3:], P[t + 1, b, :3], P[t + 1, b, 3:]
                v = (x2 - x1) / dt
                sub = q2 - q1 if np.linalg.norm(q2 - q1) < np.linalg.norm(q2 + q1) else q2 + q1
                w = (2 * ko.qmul(sub, ko.qconj(q2)) / dt)[:3]
                Rp = lps @ q2r(q2).T
                lv = np.cross(w[None], Rp) + v[None]
                dist = np.zeros_like(lps) if r_prev is None else Rp - (r_prev - v * dt)[None]
                res = np.linalg.norm(lv, axis=1) + 0.2 * np.linalg.norm(dist, axis=1) + 0.02 * np.linalg.norm(Rp, axis=1)
                i = int(np.argmin(res))
                two = np.partition(res, 1)[:2]
                tr["min"][t, b], tr["gap"][t, b], tr["margin"][t, b] = res[i], two[1] - two[0], abs(res[i] - V_THRES)
                if res[i] < V_THRES:
                    r_prev = Rp[i]
                    C[t, 4 * b], C[t, 4 * b + 1:4 * b + 4] = 1.0, r_prev
                else:
                    r_prev = None
    return C, tr


def synthesize(table, q, scale):
    """One sequence -> (imu [L, 72], constrs [L, 20], trace)."""
    P = tracked_poses(table, q, scale)
    C, tr = sbp_labels(P)
    return imu_readings(P), C, tr


def motion(n, seed, speed=1.0):
    """A smooth nimble_qdq sequence [n, 114] (columns 57: zero): sinusoidal joints and root about a standing pose, run on a clock whose
    speed alternates between slow and fast — d(phase)/dt = 0.02 + 0.6 sin^2(2 pi t / n) — so that every SBP body is stationary over
    some stretches and moving over others."""
    rng = np.random.RandomState(seed)
    k = np.arange(n)
    clock = np.cumsum(speed * (0.02 + 0.6 * np.sin(2 * np.pi * k / n) ** 2))[:, None] / 60.0 * 2.0
    q = np.zeros((n, 114))
    base, amp = rng.randn(54) * 0.15, rng.uniform(0.05, 0.4, 54)
    freq, ph = rng.uniform(0.3, 1.2, 54), rng.uniform(0, 2 * np.pi, 54)
    q[:, 3:57] = base + amp * np.sin(2 * np.pi * freq * clock + ph)
    q[:, :3] = np.array([0.0, 0.0, 0.95]) + rng.uniform(0.05, 0.3, 3) * np.sin(2 * np.pi * rng.uniform(0.2, 0.6, 3) * clock + rng.uniform(0, 6, 3))
    return q
