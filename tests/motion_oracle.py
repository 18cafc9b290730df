"""numpy / scipy restatement, in fp64, of what tip_amd.motion runs on the device (csrc/tip_motion.hip): the ground-truth half of the
reference's preprocessing, raw SMPL pose sequences to `nimble_qdq`.  It imports nothing of tip_amd.motion.

  dip_loader.py:151-181                    n frames at fps (60.0 without mocap_framerate / frame_rate), A2R of every SMPL joint's axis-angle
  preprocess_DIP_TC_new.py:98-107          the root: (A2R(pose[0:3]), trans[frame]) with `trans`; else (rot_up_R A2R(pose[0:3]),
                                           (0, 0, root_z_offset)), constants.py:21-23
  data_utils.py:103-161                    get_raw_motion_info_nimble_q_dummy_dq: t_0 = 0.015 / 2, t_{k+1} = t_k + DT while t_k < length;
                                           per row the pose at t_k (T2Qp, Q2A per joint) and the root at t_k + DT (v, and w through
                                           Q_mult of the conjugate); the joints' velocities are zeros
  amass_char_info.py                       bvh_map names the SMPL joint of a URDF joint (the names coincide with constants.SMPL_JOINTS);
                                           nimble_state_map orders the 17 spherical joints; the two fixed wrists are dropped
  fairmotion Motion.get_pose_by_time       (its published source; the library is not vendored, parity with it is UNPINNED): time clipped to
                                           [0, length], frame1 = int(time fps + 1e-5), frame2 = min(frame1 + 1, n - 1), alpha =
                                           clip((time - t1) / (t2 - t1), 0, 1), R = R1 A2R(alpha R2A(R1^T R2)), p linear

The rotation primitives are scipy's (Rotation.from_rotvec / from_matrix / as_rotvec), as the stand-ins of the golden's generator are;
the quaternion sign drops out of every output, so everything stays at the rotation level.  One statement beyond the reference, which
never sees such input: a non-finite root position reads as NaN (the device's rule for Inf)."""
import numpy as np
from scipy.spatial.transform import Rotation

DT = 1.0 / 60                                   # constants.py:7
T0 = 0.015 / 2.0                                # data_utils.py:112
ROOT_Z = 0.95                                   # constants.py:23
ROT_UP_Q = np.array([0.5, 0.5, 0.5, 0.5])       # constants.py:21
SMPL_JOINTS = ("root", "lhip", "rhip", "lowerback", "lknee", "rknee", "upperback", "lankle", "rankle", "chest", "ltoe", "rtoe", "lowerneck",
               "lclavicle", "rclavicle", "upperneck", "lshoulder", "rshoulder", "lelbow", "relbow", "lwrist", "rwrist", "lhand",
               "rhand")                          # constants.py:33-58
# amass_char_info.py:89-109 nimble_state_map, as names in state order 1 .. 17 (output columns 6, 9, ..., 54)
STATE_ORDER = ("lhip", "lknee", "lankle", "lowerback", "upperback", "chest", "lclavicle", "lshoulder", "lelbow", "lowerneck", "upperneck",
               "rclavicle", "rshoulder", "relbow", "rhip", "rknee", "rankle")
JOINTS = tuple(SMPL_JOINTS.index(n) for n in ("root",) + STATE_ORDER)       # [18]: the root, then the joints in output order


def time_table(count):
    """t_0 .. t_{count-1} as np.cumsum over [T0, DT, DT, ...]: the reference's running sum (data_utils.py:112,156), to the bit."""
    if count <= 0:
        return np.zeros(0)
    step = np.full(count, DT)
    step[0] = T0
    return np.cumsum(step)


def time_loop(length, cap=1 << 22):
    """The reference's own loop: every cur_time with cur_time < length."""
    out, t = [], 0.015 / 2.0
    while t < length and len(out) < cap:
        out.append(t)
        t += DT
    return np.array(out)


def output_rows(n, fps):
    """K: the number of k with t_k < (n - 1) / fps."""
    if n < 1:
        return 0
    length = (n - 1) * (1.0 / fps)
    cap = max(int(length / DT) + 4, 1)
    return int(np.count_nonzero(time_table(cap) < length))


def _a2r(a):
    """scipy's from_rotvec(a).as_matrix() on [..., 3]; a non-finite vector gives a NaN matrix (scipy refuses some of them)."""
    a = np.asarray(a, dtype=np.float64)
    flat = a.reshape(-1, 3)
    ok = np.isfinite(flat).all(axis=1)
    out = np.full((flat.shape[0], 3, 3), np.nan)
    if ok.any():
        out[ok] = Rotation.from_rotvec(flat[ok]).as_matrix()
    return out.reshape(a.shape[:-1] + (3, 3))


def _r2a(R):
    """scipy's from_matrix(R).as_rotvec() on [..., 3, 3]: angle in [0, pi]; a non-finite matrix gives a NaN vector."""
    R = np.asarray(R, dtype=np.float64)
    flat = R.reshape(-1, 3, 3)
    ok = np.isfinite(flat).all(axis=(1, 2))
    out = np.full((flat.shape[0], 3), np.nan)
    if ok.any():
        out[ok] = Rotation.from_matrix(flat[ok]).as_rotvec()
    return out.reshape(R.shape[:-2] + (3,))


def lookup(n, fps, time):
    """get_pose_by_time's indices: (frame1, frame2, alpha, unclipped, time fps + 1e-5)."""
    fps_inv = 1.0 / fps
    length = (n - 1) * fps_inv
    t = min(max(time, 0.0), length)
    ff = t * fps + 1e-5
    f1 = int(ff)
    f2 = min(f1 + 1, n - 1)
    if f1 == f2:
        return f1, f2, 0.0, t == time, ff
    t1, t2 = f1 * fps_inv, f2 * fps_inv
    return f1, f2, min(max((t - t1) / (t2 - t1), 0.0), 1.0), t == time, ff


def pose_at(poses, trans, fps, time, joints):
    """(R [len(joints), 3, 3], p [3]) of the listed SMPL joints at `time`; joints[0] is the root and carries the root rule."""
    n = poses.shape[0]
    f1, f2, alpha, _, _ = lookup(n, fps, time)
    with np.errstate(all="ignore"):
        a1 = np.stack([poses[f1, 3 * j:3 * j + 3] for j in joints])
        R1 = _a2r(a1)
        if f1 == f2:
            R = R1
        else:
            R2 = _a2r(np.stack([poses[f2, 3 * j:3 * j + 3] for j in joints]))
            R = R1 @ _a2r(alpha * _r2a(np.swapaxes(R1, 1, 2) @ R2))
        if trans is None:
            R[0] = Rotation.from_quat(ROT_UP_Q).as_matrix() @ R[0]
            p = np.array([0.0, 0.0, ROOT_Z])
        else:
            p = trans[f1].astype(np.float64) if f1 == f2 else (1 - alpha) * trans[f1] + alpha * trans[f2]
            p = np.where(np.isfinite(p), p, np.nan)
    return R, p


def qdq_from_smpl(poses, fps, trans=None, joints=JOINTS):
    """One sequence: poses [n, >= 66], trans [n, 3] or None -> nimble_qdq [K, 114]."""
    poses = np.asarray(poses, dtype=np.float64)
    trans = None if trans is None else np.asarray(trans, dtype=np.float64)
    n = poses.shape[0]
    K = output_rows(n, fps)
    T = time_table(K)
    out = np.zeros((K, 114))
    with np.errstate(all="ignore"):
        for k in range(K):
            R, p = pose_at(poses, trans, fps, T[k], joints)
            Rn, pn = pose_at(poses, trans, fps, T[k] + DT, joints[:1])
            out[k, 0:3] = p
            out[k, 3:57] = _r2a(R).reshape(-1)
            out[k, 57:60] = (pn - p) / DT
            out[k, 60:63] = _r2a(R[0].T @ Rn[0]) / DT
    return out


def rows_reading(n, fps, frame, root):
    """The output rows of a sequence that read source frame `frame`: through the pose at t_k, and for a root value (`root`: columns 0:3
    of poses, or trans) also through the root at t_k + DT.  A weight of 0 counts: 0 x NaN is NaN."""
    K = output_rows(n, fps)
    T = time_table(K)
    rows = []
    for k in range(K):
        hit = False
        for t in (T[k], T[k] + DT) if root else (T[k],):
            f1, f2, _, _, _ = lookup(n, fps, t)
            hit |= frame in (f1, f2)
        if hit:
            rows.append(k)
    return rows


def conditions(poses, fps, trans=None, joints=JOINTS):
    """What the fixture is held to, for one sequence: (largest emitted rotation angle, largest neighbouring-frame relative rotation
    angle over the joints read, smallest distance of time fps + 1e-5 from an integer over the unclipped lookups)."""
    poses = np.asarray(poses, dtype=np.float64)
    n = poses.shape[0]
    out = qdq_from_smpl(poses, fps, trans, joints)
    ang = out[:, 3:57].reshape(-1, 3)
    emitted = float(np.linalg.norm(ang, axis=1).max()) if ang.size else 0.0
    emitted = max(emitted, float(np.linalg.norm(out[:, 60:63], axis=1).max() * DT) if out.size else 0.0)
    rel = 0.0
    for f in range(n - 1):
        R1 = _a2r(np.stack([poses[f, 3 * j:3 * j + 3] for j in joints]))
        R2 = _a2r(np.stack([poses[f + 1, 3 * j:3 * j + 3] for j in joints]))
        rel = max(rel, float(np.linalg.norm(_r2a(np.swapaxes(R1, 1, 2) @ R2), axis=1).max()))
    frac = 1.0
    for t in time_table(out.shape[0]):
        for tt in (t, t + DT):
            _, _, _, unclipped, ff = lookup(n, fps, tt)
            if unclipped:
                frac = min(frac, abs(ff - round(ff)))
    return emitted, rel, frac


def source_motion(n, seed, width=72, with_trans=True, amp=0.5):
    """A smooth source motion: sinusoidal SMPL axis-angles [n, width] (columns beyond 66 carry values that nothing may read) and a
    sinusoidal root path [n, 3] or None."""
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None] / max(n, 2)
    poses = rng.randn(width) * 0.2 + rng.uniform(0.05, amp, width) * np.sin(2 * np.pi * rng.uniform(0.3, 1.5, width) * t + rng.uniform(0, 6, width))
    trans = None
    if with_trans:
        trans = np.array([0.1, -0.2, 0.9]) + rng.uniform(0.05, 0.4, 3) * np.sin(2 * np.pi * rng.uniform(0.3, 1.0, 3) * t + rng.uniform(0, 6, 3))
    return poses, trans
