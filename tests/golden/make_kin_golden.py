#!/usr/bin/env python3
"""Golden fixture of the REFERENCE's kinematic tail for tip_amd.kinematics: FK through data_utils.viz_current_frame_and_store_fk_info_
include_fixed, the root track and SBP locations of the real RTRunnerMin.step, and the evaluation script's seven metrics through the
reference's own loss_* functions.

Runs only in the build container (it reads the reference checkout).  The reference's data_utils and real_time_runner_minimal are
imported as they are; what is not installed is stood in at the module boundary:
  * fairmotion.ops.conversions / quaternion -> make_runner_golden.py's scipy stand-ins, plus Q_diff (q1^-1 q2) for the metrics;
  * bullet_agent.SimAgent (PyBullet)        -> KinChar below: the same accessors, REAL forward kinematics of data/amass.urdf through
    tests/kin_oracle.py (resetBasePositionAndOrientation + resetJointStateMultiDof + getLinkState fields 0-1 and 4-5).  PyBullet is
    not installed here, so PyBullet parity is UNPINNED and the fixture says so (`fk_impl`), as `conversions_impl` does for
    fairmotion.  --real-pybullet builds the reference's own SimAgent instead; regenerating the fixture and re-running
    tests/test_kin_cpu.py + tests/test_kin_gpu.py is then the whole pinning step.  --real-fairmotion as in make_runner_golden.py.
  * torch.Tensor.cuda                        -> identity.

tests/golden/tip_kin_golden.npz (data only):
  (a) table/*     the skeleton table derived from the URDF and amass_char_info (no text of either)
  (b) poses/*     32 poses (the zero pose, joint angles at the branch points of tip_rotation_branches.npz, random ones) and their
                  pq_g / pq_jf through the reference's viz_current_frame_and_store_fk_info_include_fixed
  (c) track{0,1}/* two tracks of 60 and 90 frames from RTRunnerMin.step with a scripted model (prepared rows: smooth sinusoidal
                  joints, root velocity and contact offsets, flags on a schedule); per step qdq, ct, viz_locs
  (d) track{0,1}/pred_qdq, gt_qdq, metrics: the script's trimmed prediction, a perturbed "ground truth", and the seven numbers of
                  offline_testing_simple.py:436-445 (rows 30 .. L - 7)

usage: python tests/golden/make_kin_golden.py [--real-fairmotion] [--real-pybullet]
"""
import os
import sys

import numpy as np
import torch
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
REF = "/root/reference"

import kin_oracle as ko                # noqa: E402
import make_runner_golden as mrg       # noqa: E402


def q_diff(q1, q2):
    """fairmotion's Q_diff stood in: q1^-1 q2 on (x, y, z, w), single or batched."""
    q1, q2 = np.asarray(q1, dtype=np.float64), np.asarray(q2, dtype=np.float64)
    return ko.qmul(ko.qconj(q1), q2)


class KinChar:
    """bullet_agent.SimAgent's accessors over real FK of the URDF (kin_oracle.fk_quats)."""

    def __init__(self, table, info):
        self._table, self._info = table, info
        L = len(table["parent"])
        self._joint_indices = range(L)
        self.non_root_active_idx = [j for j in info.joint_idx.values() if j != info.root and table["state_col"][j] >= 0]
        self._p, self._q = np.zeros(3), np.array([0.0, 0, 0, 1])
        self._jq = np.tile(np.array([0.0, 0, 0, 1]), (L, 1))

    def get_char_info(self):
        return self._info

    def set_root_pQvw(self, p, Q, v, w):
        self._p, self._q = np.array(p, dtype=float), np.array(Q, dtype=float)

    def set_joints_pv(self, idx, pos, vel):
        for j, q in zip(idx, pos):
            self._jq[j] = np.asarray(q, dtype=float)

    def get_root_pQ(self):
        return self._p.copy(), self._q.copy()

    def _fk(self):
        return ko.fk_quats(self._table, self._p[None], self._q[None], self._jq[None])

    def get_link_pQ(self, indices):
        g = self._fk()[0][0]
        return [g[i + 1, :3] for i in indices], [g[i + 1, 3:] for i in indices]

    def get_link_pQ_joint_frame(self, indices):
        jf = self._fk()[1][0]
        return [jf[i + 1, :3] for i in indices], [jf[i + 1, 3:] for i in indices]


def make_char(table, info, real_pybullet):
    if not real_pybullet:
        return KinChar(table, info), "kin_oracle.fk_quats stand-in (PyBullet absent: getLinkState parity UNPINNED)"
    import pybullet as pb
    import pybullet_utils.bullet_client as bc
    from bullet_agent import SimAgent
    client = bc.BulletClient(connection_mode=pb.DIRECT)
    return SimAgent(name="sim_agent_0", pybullet_client=client, model_file=os.path.join(REF, "data/amass.urdf"), char_info=info,
                    kinematic_only=True, self_collision=False), "pybullet (installed package)"


def poses_fixture(char, table, data_utils):
    """32 poses in our (nimble) column order and their FK through the reference."""
    rng = np.random.RandomState(7)
    br = np.load(os.path.join(HERE, "tip_rotation_branches.npz"))
    aa_branch = br["aa_in"][: int(br["n_real"][0])]
    q = np.zeros((32, 57))
    q[1:, :3] = rng.randn(31, 3) * 0.5 + [0, 0, 0.9]
    pick = aa_branch[np.linspace(0, len(aa_branch) - 1, 16 * 18).astype(int)].reshape(16, 54)       # 16 poses made of branch-point angles
    q[1:17, 3:] = pick
    q[17:, 3:] = rng.randn(15, 54) * 0.6
    g, jf = [], []
    for row in q:
        s = np.concatenate([row, np.zeros(57)])
        a, b = data_utils.viz_current_frame_and_store_fk_info_include_fixed(char, data_utils.our_pose_2_bullet_format(char, s),
                                                                            return_joint_frame_info=True)
        g.append(a)
        jf.append(b)
    return {"poses/q": q, "poses/pq_g": np.array(g), "poses/pq_jf": np.array(jf)}


class ScriptedModel:
    """model(x_imu, x_s) -> [1, T, 131] whose last row is the prepared row of the call."""

    def __init__(self, rows):
        self.rows, self.k = rows, 0

    def __call__(self, x_imu, x_s):
        y = torch.zeros((1, x_imu.shape[1], self.rows.shape[1]), dtype=torch.float64)
        y[0, -1] = torch.tensor(self.rows[self.k])
        self.k += 1
        return y


def prepared_rows(n, seed):
    """The model rows of n calls: 6D of smooth joints, root velocity, confidences on a schedule and contact offsets (x 5, as the
    network emits them: smooth_and_split_s_c divides by 5)."""
    s_rest, c_t, _ = ko.scripted_rows(n, seed, nc=20, speed=[0.35, 1.0][seed % 2])
    y = np.zeros((n, 131))
    R = Rotation.from_rotvec(s_rest[:, :54].reshape(-1, 3)).as_matrix()[:, :, :2]
    y[:, :108] = R.reshape(n, 108)
    y[:, 108:111] = s_rest[:, 54:57]
    y[:, 111:] = c_t
    y[:, 111::4] = np.where(c_t[:, 0::4] > 0, 1.0, -1.0)
    for k in (1, 2, 3):
        y[:, 111 + k::4] *= 5.0
    return y


def imu_sequence(n_frames, seed):
    """make_runner_golden's smooth IMU frames with a root sensor that turns slowly at the ends of the track and faster in the middle
    (the root orientation is the IMU's, :160-162: a fast turn alone sweeps the feet past the clip on every frame)."""
    out = mrg.smooth_imu_sequence(n_frames, seed)
    rng = np.random.RandomState(900 + seed)
    base, axis = Rotation.random(random_state=seed), rng.randn(3) * 0.8
    k = np.arange(n_frames)
    angle = np.cumsum(0.03 + 0.97 * np.sin(np.pi * k / n_frames) ** 2) / 60.0
    out[:, :9] = (Rotation.from_rotvec(angle[:, None] * axis[None]) * base).as_matrix().reshape(n_frames, 9)
    return out


def track_fixture(tag, n_frames, seed, char, table, info, data_utils, RTRunnerMin):
    rng = np.random.RandomState(500 + seed)
    s_init = np.zeros(114)
    s_init[3:57] = rng.randn(54) * 0.3
    s_init[:3] = [0.2, -0.1, 0.95]
    model = ScriptedModel(prepared_rows(n_frames, seed))
    runner = RTRunnerMin(char, model, 40, s_init, with_acc_sum=True)
    imu = imu_sequence(n_frames, seed)
    # the script's loop (offline_testing_simple.py:123-139)
    s_traj = np.zeros((n_frames, 114))
    s_traj[0] = s_init
    qdq, ct, viz, valid = [], [], [np.ones((5, 3)) * 100.0], []
    for t in range(n_frames - 1):
        calls = model.k
        res = runner.step(imu[t], s_traj[t, :3])
        s_traj[t + 1] = res["qdq"]
        qdq.append(np.array(res["qdq"]).copy())
        ct.append(np.array(res["ct"]).copy())
        viz.append(np.array(res["viz_locs"]).copy())
        valid.append(model.k > calls)
    viz = np.array(viz)
    out = {f"{tag}/s_init": s_init, f"{tag}/qdq": np.array(qdq), f"{tag}/ct": np.array(ct), f"{tag}/viz_locs": viz[1:],
           f"{tag}/valid": np.array(valid)}
    # the three properties the tests lean on, from the oracle's trace of the same rows
    _, _, tr = ko.track(table, s_init, out[f"{tag}/qdq"][:, 3:], out[f"{tag}/ct"], out[f"{tag}/valid"])
    fl = tr["flags"][out[f"{tag}/valid"]]
    combos = [int(((fl[:, 0] == a) & (fl[:, 1] == b)).sum()) for a in (0, 1) for b in (0, 1)]
    on = out[f"{tag}/valid"] & (tr["flags"].max(1) == 1)
    binds, free = int((tr["clip"] & on).sum()), int((~tr["clip"] & on).sum())
    gap = float(tr["margin"].min())
    print(tag, "frames", n_frames, "valid", int(out[f"{tag}/valid"].sum()), "flag combos", combos, "clip binds / not", binds, free,
          "min branch margin", round(gap, 3))
    assert min(combos) >= 5, combos
    assert binds >= 5 and free >= 20, (binds, free)
    assert gap > 0.1, gap
    # (d) the script's trim (:148-153), a perturbed ground truth, its FK loop (:228-260) and metrics (:436-445)
    trim = runner.IMU_n_smooth + 2
    pred = s_traj.copy()
    pred[0:-trim] = pred[trim:]
    pred[-trim:] = pred[-trim - 1]
    tt = np.arange(n_frames)[:, None] / 60.0
    gt = pred.copy()
    gt[:, :57] += 0.05 * np.sin(2 * np.pi * rng.uniform(0.2, 1.0, 57) * tt + rng.uniform(0, 6, 57))
    gt[:, :3] += tt * rng.uniform(-0.2, 0.2, 3)
    t1 = np.array([data_utils.our_pose_2_bullet_format(char, p) for p in gt])
    t2 = np.array([data_utils.our_pose_2_bullet_format(char, p) for p in pred])
    pq1, pq2 = [], []
    for t in range(30, n_frames - 6):
        pq2.append(data_utils.viz_current_frame_and_store_fk_info_include_fixed(char, t2[t]))
        pq1.append(data_utils.viz_current_frame_and_store_fk_info_include_fixed(char, t1[t]))
    res = (t1[30:n_frames - 6], t2[30:n_frames - 6], np.array(pq1), np.array(pq2))
    m = [data_utils.loss_angle(*res), data_utils.loss_j_pos(*res), data_utils.loss_root_dist_pos(*res, t=2.0),
         data_utils.loss_root_dist_pos(*res, t=5.0), data_utils.loss_root_dist_pos(*res, t=10.0), data_utils.loss_max_jerk(*res),
         data_utils.loss_root_jerk(*res)]
    out.update({f"{tag}/pred_qdq": pred, f"{tag}/gt_qdq": gt, f"{tag}/metrics": np.array(m, dtype=np.float64)})
    print(tag, "metrics", np.round(m, 4))
    return out


def main():
    real_fm, real_pb = "--real-fairmotion" in sys.argv, "--real-pybullet" in sys.argv
    mrg.install_stubs(real_fm)
    if not real_fm:
        sys.modules["fairmotion.ops.quaternion"].Q_diff = q_diff
    if real_pb:
        for name in ("pybullet", "bullet_agent"):
            sys.modules.pop(name, None)
    sys.path.insert(0, REF)
    import amass_char_info as info
    import data_utils
    from real_time_runner_minimal import RTRunnerMin
    torch.Tensor.cuda = lambda self, *a, **k: self      # harness only
    table = ko.read_urdf(os.path.join(REF, "data", "amass.urdf"), info)
    char, fk_impl = make_char(table, info, real_pb)
    out = {"table/" + k: v for k, v in table.items()}
    out.update(poses_fixture(char, table, data_utils))
    for tag, n, seed in (("track0", 60, 2), ("track1", 90, 5)):
        out.update(track_fixture(tag, n, seed, char, table, info, data_utils, RTRunnerMin))
    conv = "fairmotion (installed package)" if real_fm else "scipy stand-in (fairmotion fork absent: parity UNPINNED)"
    out["conversions_impl"] = np.frombuffer(conv.encode(), dtype=np.uint8).copy()
    out["fk_impl"] = np.frombuffer(fk_impl.encode(), dtype=np.uint8).copy()
    path = os.path.join(HERE, "tip_kin_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; FK:", fk_impl)


if __name__ == "__main__":
    main()
