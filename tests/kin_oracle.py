"""numpy restatement of what tip_amd.kinematics runs on the device (csrc/tip_kin.hip), in any dtype: forward kinematics of the
character, the root track with its stationary-body-point (SBP) correction (real_time_runner_minimal.py:159-194; data_utils.py:397-412,
473-548) and the evaluation script's seven metrics (offline_testing_simple.py:422-445; data_utils.py:314-391).  fp64 is the oracle;
float32 is the same statements in float32, which is what the GPU tests take their noise floor from.  It has its own URDF reading and
imports nothing of tip_amd.kinematics.

A skeleton table is a dict of arrays, the links in URDF (= PyBullet) order, bodies numbered 0 (the root) and i + 1 (link i):
    parent [L] int (body index)   joint_xyz [L,3]   joint_q [L,4] (x, y, z, w)   com_xyz [L,3]   state_col [L] int (-1: fixed)
    sbp [5] int (body indices of lankle, rankle, lwrist, rwrist, root)   names [L + 1]
A pose is xyz + (x, y, z, w); pose tables are [rows, L + 1, 7], the root first."""
import xml.etree.ElementTree as ET

import numpy as np

DT = 1.0 / 60                       # constants.py:7
SBP_BODIES = ("lankle", "rankle", "lwrist", "rwrist", "root")
METRICS = ("angle", "j_pos", "root_2s", "root_5s", "root_10s", "jerk", "root_jerk")


# ---- rotations -----------------------------------------------------------------------------------------------------------------------
def a2q(aa, dtype=np.float64):
    """scipy's Rotation.from_rotvec(aa).as_quat() — fairmotion's A2Q — on [..., 3]: exact at angle 0, the series below 1e-3 rad."""
    aa = np.asarray(aa, dtype=dtype)
    t2 = (aa * aa).sum(-1)
    t = np.sqrt(t2)
    small = t <= dtype(1e-3)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(small, dtype(0.5) - t2 / dtype(48) + t2 * t2 / dtype(3840), np.sin(t * dtype(0.5)) / t)
    return np.concatenate([aa * s[..., None], np.cos(t * dtype(0.5))[..., None]], axis=-1).astype(dtype)


def qmul(a, b):
    """Hamilton product on (x, y, z, w), [..., 4]."""
    x1, y1, z1, w1 = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    x2, y2, z2, w2 = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2,
                     w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2, w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2], axis=-1)


def qconj(q):
    return q * np.array([-1, -1, -1, 1], dtype=q.dtype)


def qrot(q, v):
    """v rotated by the unit quaternion q: v + w t + u x t, t = 2 (u x v).  Exact for the identity."""
    u, w = q[..., :3], q[..., 3:4]
    t = q.dtype.type(2) * np.cross(u, v)
    return v + w * t + np.cross(u, t)


def rpy_to_quat(rpy):
    """URDF roll-pitch-yaw (fixed axes x, y, z) -> (x, y, z, w), fp64."""
    r, p, y = (float(v) for v in rpy)
    qx = np.array([np.sin(r / 2), 0, 0, np.cos(r / 2)])
    qy = np.array([0, np.sin(p / 2), 0, np.cos(p / 2)])
    qz = np.array([0, 0, np.sin(y / 2), np.cos(y / 2)])
    return qmul(qz, qmul(qy, qx))


# ---- the URDF ------------------------------------------------------------------------------------------------------------------------
def _vec(el, attr, n=3):
    v = [float(x) for x in (el.get(attr, "0 0 0") if el is not None else "0 0 0").split()]
    assert len(v) == n, (attr, v)
    return np.array(v)


def read_urdf(path, char_info):
    """The skeleton table of a URDF whose joints are spherical or fixed, with the state columns of our_pose_2_bullet_format
    (data_utils.py:246-259) and the SBP bodies of get_cur_step_root_correction_from_all_constr (:502-508) from `char_info`."""
    robot = ET.parse(path).getroot()
    links = {ln.get("name"): ln for ln in robot.findall("link")}
    joints = robot.findall("joint")
    children = {j.find("child").get("link") for j in joints}
    root = [n for n in links if n not in children]
    assert len(root) == 1, root
    body = {root[0]: 0}
    parent, jxyz, jq, com, col, names = [], [], [], [], [], [root[0]]
    assert np.all(_vec(links[root[0]].find("inertial/origin"), "xyz") == 0) and np.all(_vec(links[root[0]].find("inertial/origin"), "rpy") == 0)
    for i, j in enumerate(joints):
        assert j.get("type") in ("spherical", "fixed"), j.get("type")
        child = j.find("child").get("link")
        parent.append(body[j.find("parent").get("link")])
        body[child] = i + 1
        names.append(child)
        o = j.find("origin")
        jxyz.append(_vec(o, "xyz"))
        jq.append(rpy_to_quat(_vec(o, "rpy")))
        io = links[child].find("inertial/origin")
        assert np.all(_vec(io, "rpy") == 0), child
        com.append(_vec(io, "xyz"))
        if j.get("type") == "fixed":
            col.append(-1)
        else:
            col.append((char_info.nimble_state_map[char_info.joint_idx[j.get("name")]] - 1) * 3 + 6)
        assert char_info.joint_idx[j.get("name")] == i, (j.get("name"), i)
    sbp = [getattr(char_info, n) + 1 for n in SBP_BODIES]
    return {"parent": np.array(parent, dtype=np.int32), "joint_xyz": np.array(jxyz), "joint_q": np.array(jq), "com_xyz": np.array(com),
            "state_col": np.array(col, dtype=np.int32), "sbp": np.array(sbp, dtype=np.int32), "names": np.array(names)}


# ---- forward kinematics --------------------------------------------------------------------------------------------------------------
def fk_quats(table, root_p, root_q, joint_q, dtype=np.float64):
    """(pq_g, pq_jf) [N, L + 1, 7] from the base pose and one quaternion per link ([N, L, 4]; a fixed link's is ignored): what
    PyBullet's getLinkState gives after resetBasePositionAndOrientation + resetJointStateMultiDof — fields 0-1 (the COM pose) and 4-5
    (the link frame).  child frame = parent frame x joint origin x joint rotation; COM = frame + R com_xyz."""
    root_p, root_q, joint_q = (np.asarray(a, dtype=dtype) for a in (root_p, root_q, joint_q))
    n, L = root_p.shape[0], len(table["parent"])
    jf = np.zeros((n, L + 1, 7), dtype=dtype)
    g = np.zeros((n, L + 1, 7), dtype=dtype)
    jf[:, 0, :3], jf[:, 0, 3:] = root_p, root_q
    g[:, 0] = jf[:, 0]
    for i in range(L):
        pa = int(table["parent"][i])
        pp, pq = jf[:, pa, :3], jf[:, pa, 3:]
        q = qmul(pq, np.broadcast_to(table["joint_q"][i].astype(dtype), (n, 4)))
        if table["state_col"][i] >= 0:
            q = qmul(q, joint_q[:, i])
        jf[:, i + 1, :3] = pp + qrot(pq, table["joint_xyz"][i].astype(dtype)[None])
        jf[:, i + 1, 3:] = q
        g[:, i + 1, :3] = jf[:, i + 1, :3] + qrot(q, table["com_xyz"][i].astype(dtype)[None])
        g[:, i + 1, 3:] = q
    return g, jf


def fk(table, q, dtype=np.float64):
    """(pq_g, pq_jf) of q [N, >= 57]: root xyz, root axis-angle, then the joints' axis-angles at their state columns."""
    q = np.asarray(q, dtype=dtype)
    L = len(table["parent"])
    jq = np.zeros((q.shape[0], L, 4), dtype=dtype)
    jq[..., 3] = 1
    for i in range(L):
        c = int(table["state_col"][i])
        if c >= 0:
            jq[:, i] = a2q(q[:, c:c + 3], dtype)
    return fk_quats(table, q[:, :3], a2q(q[:, 3:6], dtype), jq, dtype)


# ---- the root track ------------------------------------------------------------------------------------------------------------------
def track_batch(table, s_init, s_rest, c_t, valid, dtype=np.float64):
    """R sequences side by side through RTRunnerMin.step's tail (:159-194), one time step of all of them per pass: s_init [R, 114],
    s_rest [R, n, 111] (= the runner's s_t[3:114]), c_t [R, n, 8|20], valid [R, n] (shorter sequences padded with rows that are not
    valid) -> root [R, n, 3], viz_locs [R, n, 5, 3] and a trace {"flags" [R, n, 2] (-1 on rows that are not valid), "clip" [R, n] (the
    clip changed x or y), "margin" [R, n] (||q2 - q1| - |q2 + q1|| at its smallest over the active feet, inf when none is)}.
    The statements are the reference's, on arrays: get_residue_from_contr (data_utils.py:397-412), the nanmean / clip of :517-545, the
    flat-ground rule of the runner (:184-189) with its norm test taken literally, and the shifts of :191-194.
    The velocity :159 integrates is the one from before the pose averaging of :165-166, which s_rest[54:57] has been through:
    v = 2 s_rest[54:57] - the previous valid row's (s_rest[54:57] itself on a sequence's first valid row)."""
    import warnings
    f = dtype
    s_init, s_rest, c_t = (np.asarray(a, dtype=f) for a in (s_init, s_rest, c_t))
    valid = np.asarray(valid, dtype=bool)
    R, n = s_rest.shape[:2]
    n_sbps, dt = c_t.shape[2] // 4, f(DT)
    root = s_init[:, :3].copy()
    pq_prev = fk(table, s_init[:, :57], f)[0]
    a_prev, has_prev = np.zeros((R, 3), dtype=f), np.zeros(R, bool)
    roots, viz = np.zeros((R, n, 3), dtype=f), np.full((R, n, 5, 3), 100, dtype=f)
    flags, clip, margin = np.full((R, n, 2), -1), np.zeros((R, n), bool), np.full((R, n), np.inf)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for t in range(n):
            ok = valid[:, t]
            a = s_rest[:, t, 54:57]
            v = np.where(has_prev[:, None], f(2) * a - a_prev, a)
            q = np.concatenate([root + v * dt, s_rest[:, t, :54]], axis=1)
            pq = fk(table, q, f)[0]
            c_locs = np.full((R, 5, 3), 100, dtype=f)
            res = np.full((R, 2, 3), np.nan, dtype=f)
            for i in range(n_sbps):
                b = int(table["sbp"][i])
                x1, q1, x2, q2 = pq_prev[:, b, :3], pq_prev[:, b, 3:], pq[:, b, :3], pq[:, b, 3:]
                act = c_t[:, t, 4 * i] != 0
                sol = c_t[:, t, 4 * i + 1:4 * i + 4]
                c_locs[:, i] = np.where(act[:, None], x2 + sol, f(100))
                if i >= 2:
                    continue                                         # only the two feet correct the root (:517-520)
                nd, ns = np.linalg.norm(q2 - q1, axis=1), np.linalg.norm(q2 + q1, axis=1)
                sub = np.where((nd < ns)[:, None], q2 - q1, q2 + q1)
                w = (f(2) * qmul(sub, qconj(q2)) / dt)[:, :3]
                res[:, i] = np.where(act[:, None], np.cross(w, sol) + (x2 - x1) / dt, f(np.nan))
                flags[ok, t, i] = act[ok]
                margin[:, t] = np.where(ok & act, np.minimum(margin[:, t], np.abs(nd.astype(np.float64) - ns)), margin[:, t])
            all_nan = np.isnan(res).all(axis=(1, 2))
            m = np.nanmean(res, axis=1).astype(f)
            vr = np.where(all_nan[:, None], f(0), np.clip(m, f(-0.5), f(0.5))).astype(f)
            clip[:, t] = ok & ~all_nan & ((vr[:, :2] != m[:, :2]) & ~np.isnan(m[:, :2])).any(axis=1)
            vr[:, 2] = 0
            for i in range(2):
                vr[:, 2] += np.where(np.linalg.norm(c_locs[:, i], axis=1) < 100, c_locs[:, i, 2], f(0))
            d = vr * dt
            root = np.where(ok[:, None], q[:, :3] - d, root)
            shifted = pq.copy()
            shifted[:, :, :3] -= d[:, None]
            pq_prev = np.where(ok[:, None, None], shifted, pq_prev)
            a_prev, has_prev = np.where(ok[:, None], a, a_prev), has_prev | ok
            roots[:, t] = root
            viz[:, t] = np.where(ok[:, None, None], c_locs - d[:, None], f(100))
    return roots, viz, {"flags": flags, "clip": clip, "margin": margin}


def track(table, s_init, s_rest, c_t, valid, dtype=np.float64):
    """One sequence: s_init [114], s_rest [n, 111], c_t [n, 8|20], valid [n] -> root [n, 3], viz_locs [n, 5, 3], trace."""
    r, v, tr = track_batch(table, np.asarray(s_init)[None], np.asarray(s_rest)[None], np.asarray(c_t)[None], np.asarray(valid)[None], dtype)
    return r[0], v[0], {k: x[0] for k, x in tr.items()}


def track_ragged(table, s_init, s_rest, c_t, valid, offsets, dtype=np.float64):
    """R sequences back to back (rows offsets[i] .. offsets[i + 1] - 1): root [N, 3], viz_locs [N, 5, 3] and the traces, row for row."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    R, n = len(lens), int(lens.max())
    pad = lambda x: np.stack([np.concatenate([x[a:b], np.zeros((n - (b - a),) + x.shape[1:], dtype=x.dtype)])      # noqa: E731
                              for a, b in zip(offsets[:-1], offsets[1:])])
    r, v, tr = track_batch(table, s_init, pad(np.asarray(s_rest)), pad(np.asarray(c_t)), pad(np.asarray(valid, dtype=bool)), dtype)
    take = lambda x: np.concatenate([x[i, :lens[i]] for i in range(R)])      # noqa: E731
    return take(r), take(v), {k: take(x) for k, x in tr.items()}


# ---- the seven metrics ---------------------------------------------------------------------------------------------------------------
def root_indices(n):
    """loss_root_dist_pos's row for t = 2, 5, 10 s among n rows (data_utils.py:383-386), with its exact Python expression."""
    return [int(np.minimum(int(t / DT) - 1, n - 1)) for t in (2.0, 5.0, 10.0)]


def evaluate(table, pred_qdq, gt_qdq, start=30, end=6, dtype=np.float64):
    """One file: the script's seven numbers over rows start .. L - end - 1 (offline_testing_simple.py:244, :437-445), FK of both
    trajectories included.  Trajectory 1 is the ground truth, 2 the prediction."""
    f = dtype
    pred, gt = np.asarray(pred_qdq, dtype=f), np.asarray(gt_qdq, dtype=f)
    L = pred.shape[0]
    if L < start + end + 4:
        raise ValueError(f"kin_oracle.evaluate: {L} rows leave fewer than 4 in range")
    pred, gt = pred[start:L - end], gt[start:L - end]
    n = pred.shape[0]
    p1, p2 = fk(table, gt[:, :57], f)[0], fk(table, pred[:, :57], f)[0]
    d = qmul(qconj(a2q(gt[:, 3:57].reshape(-1, 3), f)), a2q(pred[:, 3:57].reshape(-1, 3), f))
    ang = f(2) * np.arctan2(np.linalg.norm(d[:, :3], axis=1), np.abs(d[:, 3]))
    out = np.zeros(7, dtype=np.float64)
    out[0] = ang.mean() * 180 / 3.1416
    r1, r2 = p1[:, 1:, :3] - p1[:, 0:1, :3], p2[:, 1:, :3] - p2[:, 0:1, :3]
    out[1] = np.linalg.norm((r2 - r1).reshape(-1, 3), axis=1).mean() * 100.0
    for k, ind in enumerate(root_indices(n)):
        out[2 + k] = np.linalg.norm((p1[ind, 0, :3] - p1[0, 0, :3]) - (p2[ind, 0, :3] - p2[0, 0, :3]))
    x = p2[:, :, :3]
    jerk = np.linalg.norm(x[3:] - f(3) * x[2:-1] + f(3) * x[1:-2] - x[:-3], axis=2)
    out[5] = jerk.mean(axis=1).mean() * 100.0
    out[6] = jerk[:, 0].mean() * 100.0
    return out


# ---- inputs like the golden tracks ---------------------------------------------------------------------------------------------------
def scripted_rows(n, seed, nc=20, speed=1.0):
    """Smooth runner outputs for n frames: s_rest [n, 111] (sinusoidal joints about a random pose and a sinusoidal root velocity, both
    under an envelope that is small at the ends of the sequence, so that the clip at +-0.5 binds on some rows and not on others) and c_t [n, nc] (foot flags on a schedule that passes through all four combinations, hand and
    root flags on another, sinusoidal contact offsets), plus s_init [114]."""
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None] / 60.0
    base, amp = rng.randn(54) * 0.25, rng.uniform(0.05, 0.35, 54) * speed
    freq, ph = rng.uniform(0.3, 1.6, 54), rng.uniform(0, 2 * np.pi, 54)
    s_rest = np.zeros((n, 111))
    env = 0.04 + 0.96 * np.sin(np.pi * np.arange(n)[:, None] / max(n, 40)) ** 2      # slow at the ends (the clip is idle), fast between
    s_rest[:, :54] = base + env * amp * np.sin(2 * np.pi * freq * t + ph)
    s_rest[:, 54:57] = env * rng.uniform(0.1, 0.6, 3) * np.sin(2 * np.pi * rng.uniform(0.2, 0.8, 3) * t + rng.uniform(0, 6, 3))
    c_t = np.zeros((n, nc))
    k = np.arange(n)
    sched = [(k // 5) % 2, (k // 10) % 2, (k // 7) % 2, (k // 9) % 2, (k // 13) % 2]
    for i in range(nc // 4):
        c_t[:, 4 * i] = sched[i]
        c_t[:, 4 * i + 1:4 * i + 4] = 0.06 * np.sin(2 * np.pi * rng.uniform(0.2, 1.0, 3) * t + rng.uniform(0, 6, 3))
    s_init = np.zeros(114)
    s_init[:3] = [0.1 * rng.randn(), 0.1 * rng.randn(), 0.95]
    s_init[3:57] = s_rest[0, :54]
    return s_rest, c_t, s_init
