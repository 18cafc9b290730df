#!/usr/bin/env python3
"""Golden fixture of the REFERENCE's ground-truth preprocessing for tip_amd.motion: the `nimble_qdq` arrays that
data_utils.get_raw_motion_info_nimble_q_dummy_dq computes from pose files, read by the reference's own dip_loader.load and given
their root by preprocess_DIP_TC_new.load_and_augment_dip_motion.

Runs only in the build container (it reads the reference checkout).  dip_loader and data_utils are imported as they are, and
preprocess_DIP_TC_new.py is EXECUTED as it is (runpy.run_path, as make_syn_golden.py executes the data-generation script): its working
directory is a scratch directory that holds only a link to amass_char_info.py, so its module-level gen_data_all_tc finds no file and
its load_and_augment_dip_motion is then called on the fixture's files — `augment_impl` records that the root augmentation (:98-107) ran
from the script itself.  What is not installed is stood in at the module boundary only:
  * fairmotion.ops.conversions / quaternion -> make_runner_golden.install_stubs' scipy stand-ins, plus T2Qp, T2Rp, Rp2T, R2T, p2T here;
    fairmotion.utils.constants.eye_T;
  * fairmotion.core.motion                  -> Motion, Skeleton, Joint and Pose below: what dip_loader, the augmentation and
    get_raw_motion_info_nimble_q_dummy_dq call, with get_pose_by_time and the pose interpolation written from fairmotion's published
    source (time clipped to [0, length], frame1 = int(time fps + 1e-5), frame2 = min(frame1 + 1, n - 1), alpha clipped to [0, 1], per
    joint R1 A2R(alpha R2A(R1^T R2)) and a linear position).  fairmotion is not installed here, so parity with its interpolation is
    UNPINNED and the fixture says so (`motion_impl`), as `conversions_impl` does for the conversions;
  * pybullet, pybullet_data, bullet_client  -> modules with the few names the script's module level touches (DIRECT, JOINT_FIXED,
    getDataPath, BulletClient);
  * bullet_agent.SimAgent                   -> MotionChar below: get_char_info, and get_joint_type answered from data/amass.urdf.
    PyBullet parity is UNPINNED.

tests/golden/tip_motion_golden.npz (data only):
  table/*   the kinematics table derived from the URDF and amass_char_info (names and state_col give the joint order), with imu
  A/*       40 frames, no frame rate (60), DIP-IMU layout (.pkl: gt [40, 72], imu_ori, imu_acc), no trans: the DIP root rule
  B/*       50 frames at mocap_framerate 120, AMASS layout (.npz: poses [50, 156], trans)
  C/*       37 frames at frame_rate 100, TotalCapture layout (.npz: poses [37, 72], trans)
  D/*       2 frames (one row), E/* 1 frame (no row)
  per sequence: poses, trans (where the file has it), fps, qdq [K, 114]
Smooth sinusoids (values on a 2^-16 grid, so that the file stays small) with planted cases: a joint that is exactly zero in every frame
(A), a joint at angle pi - 2e-3 (B), source axis-angles of norm above pi (C: they come back with norm <= pi), and a joint whose
neighbouring frames are 2 rad apart (C).  The generator ASSERTS, and tests/test_motion_cpu.py re-asserts: every emitted rotation angle
<= pi - 1e-3, every neighbouring-frame relative rotation <= pi - 1e-3, time fps + 1e-5 at least 1e-3 away from an integer on every
unclipped lookup — with them no comparison against the fixture has to leave a row out.

usage: python tests/golden/make_motion_golden.py
"""
import os
import pickle
import runpy
import sys
import tempfile
import types
import xml.etree.ElementTree as ET

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
REF = "/root/reference"

import kin_oracle as ko                # noqa: E402
import make_runner_golden as mrg       # noqa: E402
import motion_oracle as mo             # noqa: E402

ANGLE_GUARD, FRAME_GUARD = 1e-3, 1e-3
JOINT_FIXED, JOINT_SPHERICAL = 4, 2    # pybullet's constants


# ---- stand-ins -----------------------------------------------------------------------------------------------------------------------
def install_motion_stubs():
    """What make_runner_golden.install_stubs leaves out and this path calls."""
    mrg.install_stubs(False)
    conv = sys.modules["fairmotion.ops.conversions"]

    def Rp2T(R, p):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, p
        return T

    conv.Rp2T = Rp2T
    conv.R2T = lambda R: Rp2T(R, np.zeros(3))
    conv.p2T = lambda p: Rp2T(np.eye(3), p)
    conv.T2Rp = lambda T: (T[:3, :3].copy(), T[:3, 3].copy())
    conv.T2Qp = lambda T: (conv.R2Q(T[:3, :3]), T[:3, 3].copy())
    utils = types.ModuleType("fairmotion.utils")
    consts = types.ModuleType("fairmotion.utils.constants")
    consts.eye_T = lambda: np.eye(4)
    utils.constants = consts
    sys.modules["fairmotion"].utils = utils
    sys.modules["fairmotion.utils"], sys.modules["fairmotion.utils.constants"] = utils, consts

    class Joint:
        def __init__(self, name=None):
            self.name, self.info, self.parent_joint, self.index = name, {}, None, -1
            self.xform_from_parent_joint = np.eye(4)

    class Skeleton:
        def __init__(self, v_up=None, v_face=None, v_up_env=None):
            self.joints, self.index_joint, self.v_up, self.v_face, self.v_up_env = [], {}, v_up, v_face, v_up_env

        def add_joint(self, joint, parent_joint):
            joint.index = len(self.joints)
            joint.parent_joint = None if parent_joint is None else self.joints[self.index_joint[parent_joint]]
            self.index_joint[joint.name] = joint.index
            self.joints.append(joint)

        def get_index_joint(self, key):
            return self.index_joint[key]

        def get_joint(self, key):
            return self.joints[self.index_joint[key]]

    class Pose:
        def __init__(self, skel, data):
            self.skel, self.data = skel, [np.array(T, dtype=np.float64) for T in data]

        def get_transform(self, key, local):
            j = self.skel.get_joint(key)
            if local:
                return self.data[j.index]
            T = j.xform_from_parent_joint @ self.data[j.index]
            while j.parent_joint is not None:
                j = j.parent_joint
                T = j.xform_from_parent_joint @ self.data[j.index] @ T
            return T

        def set_transform(self, key, T, local):
            j = self.skel.get_joint(key)
            if not local and j.parent_joint is not None:
                raise NotImplementedError("stand-in: a global transform is set on the root only")
            self.data[j.index] = np.array(T, dtype=np.float64) if local else np.linalg.inv(j.xform_from_parent_joint) @ T

        @classmethod
        def interpolate(cls, pose1, pose2, alpha):
            data = []
            for T1, T2 in zip(pose1.data, pose2.data):
                R1, p1 = conv.T2Rp(T1)
                R2, p2 = conv.T2Rp(T2)
                R = R1 @ conv.A2R(alpha * conv.R2A(R1.T @ R2))
                data.append(conv.Rp2T(R, (1 - alpha) * p1 + alpha * p2))
            return cls(pose1.skel, data)

    class Motion:
        def __init__(self, name="motion", skel=None, fps=60):
            self.name, self.skel, self.poses = name, skel, []
            self.set_fps(fps)

        def set_fps(self, fps):
            self.fps, self.fps_inv = fps, 1.0 / fps

        def add_one_frame(self, pose_data):
            self.poses.append(Pose(self.skel, pose_data))

        def num_frames(self):
            return len(self.poses)

        def length(self):
            return (len(self.poses) - 1) * self.fps_inv

        def time_to_frame(self, time):
            return int(time * self.fps + 1e-05)

        def frame_to_time(self, frame):
            return min(max(frame, 0), len(self.poses) - 1) * self.fps_inv

        def get_pose_by_frame(self, frame):
            return self.poses[frame]

        def get_pose_by_time(self, time):
            time = min(max(time, 0), self.length())
            frame1 = self.time_to_frame(time)
            frame2 = min(frame1 + 1, self.num_frames() - 1)
            if frame1 == frame2:
                return self.get_pose_by_frame(frame1)
            t1, t2 = self.frame_to_time(frame1), self.frame_to_time(frame2)
            alpha = min(max((time - t1) / (t2 - t1), 0.0), 1.0)
            return Pose.interpolate(self.get_pose_by_frame(frame1), self.get_pose_by_frame(frame2), alpha)

    m = sys.modules["fairmotion.core.motion"]
    m.Motion, m.Skeleton, m.Joint, m.Pose = Motion, Skeleton, Joint, Pose
    pb = sys.modules["pybullet"]
    pb.JOINT_FIXED, pb.JOINT_SPHERICAL, pb.DIRECT = JOINT_FIXED, JOINT_SPHERICAL, 2
    for name in ("pybullet_data", "bullet_client"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pybullet_data"].getDataPath = lambda: ""

    class BulletClient:
        def __init__(self, connection_mode=None):
            pass

        def __getattr__(self, name):
            return lambda *a, **k: None

    sys.modules["bullet_client"].BulletClient = BulletClient

    class MotionChar:
        """bullet_agent.SimAgent as get_raw_motion_info_nimble_q_dummy_dq uses it: the character's module, and each joint's type
        from the URDF."""

        def __init__(self, name=None, pybullet_client=None, model_file=None, char_info=None, **kw):
            path = model_file if os.path.exists(model_file) else os.path.join(REF, model_file)
            self._info = char_info
            self._types = {}
            for j in ET.parse(path).getroot().findall("joint"):
                self._types[char_info.joint_idx[j.get("name")]] = {"fixed": JOINT_FIXED, "spherical": JOINT_SPHERICAL}[j.get("type")]

        def get_char_info(self):
            return self._info

        def get_joint_type(self, idx):
            return self._types[idx]

    sys.modules["bullet_agent"].SimAgent = MotionChar


def run_reference_script():
    """Execute preprocess_DIP_TC_new.py itself in a scratch directory; returns its globals (robot, load_and_augment_dip_motion, ...)."""
    sys.path.insert(0, REF)
    cwd, argv = os.getcwd(), sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        os.symlink(os.path.join(REF, "amass_char_info.py"), os.path.join(tmp, "amass_char_info.py"))
        os.chdir(tmp)
        sys.argv = ["preprocess_DIP_TC_new.py", "--data_version_tag", "golden"]
        try:
            return runpy.run_path(os.path.join(REF, "preprocess_DIP_TC_new.py"), run_name="__main__")
        finally:
            os.chdir(cwd)
            sys.argv = argv


# ---- the fixture's motions -----------------------------------------------------------------------------------------------------------
def grid(x):
    return np.round(np.asarray(x, dtype=np.float64) * 65536.0) / 65536.0


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def sequences():
    """[(tag, layout, poses, trans, fps or None)]; columns 66: are constants (nothing reads them; tests poison them)."""
    out = []
    p, _ = mo.source_motion(40, 21, 72, with_trans=False, amp=0.45)
    p[:, 0:3] *= 0.3                                                    # the DIP root is rot_up_R (120 degrees) times this
    p = grid(p)
    p[:, 12:15] = 0.0                                                   # lknee: exactly zero in every frame
    p[:, 66:] = 0.25
    out.append(("A", "dip", p, None, None))
    p, t = mo.source_motion(50, 22, 156, amp=0.45)
    p = grid(p)
    p[:, 48:51] = unit([0.3, -0.5, 0.8]) * (np.pi - 2e-3)               # lshoulder: at angle pi - 2e-3
    p[:, 66:] = 0.25
    out.append(("B", "amass", p, grid(t), 120.0))
    p, t = mo.source_motion(37, 23, 72, amp=0.3)
    p = grid(p)
    ax = unit([0.6, 0.2, -0.7])
    p[:, 3:6] = ax[None] * (np.pi + 1.0 + 0.3 * np.sin(np.arange(37) / 9.0))[:, None]         # lhip: norms above pi
    p[:, 54:57] = np.array([0.0, 0.0, 1.0])[None] * np.where(np.arange(37) % 2 == 0, 1.0, -1.0)[:, None]   # lelbow: 2 rad between neighbours
    p[:, 66:] = 0.25
    out.append(("C", "tc", p, grid(t), 100.0))
    p, t = mo.source_motion(2, 24, 72, amp=0.4)
    out.append(("D", "tc", grid(p), grid(t), 60.0))
    p, t = mo.source_motion(1, 25, 72, amp=0.4)
    out.append(("E", "tc", grid(p), grid(t), 60.0))
    return out


def write_source(tmp, tag, layout, poses, trans, fps):
    """One pose file in the key layout of its corpus."""
    n = poses.shape[0]
    if layout == "dip":                                                  # DIP-IMU: a latin1-readable pickle, no frame rate, no trans
        path = os.path.join(tmp, tag + ".pkl")
        with open(path, "wb") as f:
            pickle.dump({"gt": poses, "imu_ori": np.tile(np.eye(3), (n, 17, 1, 1)), "imu_acc": np.zeros((n, 17, 3))}, f, protocol=2)
        return path
    path = os.path.join(tmp, tag + "_poses.npz")
    if layout == "amass":
        np.savez(path, poses=poses, trans=trans, mocap_framerate=np.float64(fps), gender="neutral", betas=np.zeros(16))
    else:
        np.savez(path, poses=poses, trans=trans, frame_rate=np.float64(fps))
    return path


def main():
    install_motion_stubs()
    g = run_reference_script()
    import data_utils
    robot, info = g["robot"], g["char_info"]
    assert type(robot).__name__ == "MotionChar" and robot.get_joint_type(info.lwrist) == JOINT_FIXED
    table = ko.read_urdf(os.path.join(REF, "data", "amass.urdf"), info)
    table["imu"] = np.array([getattr(info, n) + 1 for n in ("root", "lwrist", "rwrist", "lknee", "rknee", "upperneck")], dtype=np.int32)
    out = {"table/" + k: v for k, v in table.items()}
    worst = [0.0, 0.0, 1.0]
    with tempfile.TemporaryDirectory() as tmp:
        for tag, layout, poses, trans, fps in sequences():
            path = write_source(tmp, tag, layout, poses, trans, fps)
            n = poses.shape[0]
            motion, imu_R, imu_acc = g["load_and_augment_dip_motion"](robot, path, path)
            assert motion.num_frames() == n and motion.fps == (60.0 if fps is None else fps)
            if n > 1:
                qdq = data_utils.get_raw_motion_info_nimble_q_dummy_dq(robot, motion)
            else:                                                        # length 0: the loop body never runs (np.array([]) fails the shape assert)
                assert not (0.015 / 2.0 < motion.length())
                qdq = np.zeros((0, 114))
            f = motion.fps
            ours = mo.qdq_from_smpl(poses, f, trans)
            err = float(np.abs(ours - qdq).max()) if qdq.size else 0.0
            emitted, rel, frac = mo.conditions(poses, f, trans)
            print(f"{tag}: {n} frames at {f} fps ({layout}) -> {qdq.shape[0]} rows; oracle - reference {err:.2e}; largest emitted angle "
                  f"{emitted:.6f}, largest neighbour rotation {rel:.6f}, frame-lookup margin {frac:.4f}")
            assert qdq.shape == ours.shape == (mo.output_rows(n, f), 114)
            assert np.all(np.abs(ours - qdq) <= 1e-12 * np.maximum(1.0, np.abs(qdq)))
            assert not qdq[:, 63:].any()
            worst = [max(worst[0], emitted), max(worst[1], rel), min(worst[2], frac)]
            out[f"{tag}/poses"], out[f"{tag}/fps"], out[f"{tag}/qdq"] = poses, np.float64(f), qdq
            out[f"{tag}/layout"] = np.frombuffer(layout.encode(), dtype=np.uint8).copy()
            if trans is not None:
                out[f"{tag}/trans"] = trans
    assert worst[0] <= np.pi - ANGLE_GUARD and worst[1] <= np.pi - ANGLE_GUARD and worst[2] >= FRAME_GUARD, worst
    # the planted cases are there
    assert not out["A/qdq"][:, 9:12].any()                                # lknee is state 2: columns 9:12
    assert np.abs(np.linalg.norm(out["B/qdq"][:, 27:30], axis=1) - (np.pi - 2e-3)).max() < 1e-9      # lshoulder is state 8
    assert np.linalg.norm(out["C/poses"][:, 3:6], axis=1).min() > np.pi and np.linalg.norm(out["C/qdq"][:, 6:9], axis=1).max() < np.pi
    assert abs(worst[1] - 2.0) < 1e-9
    assert out["D/qdq"].shape[0] == 1 and out["E/qdq"].shape[0] == 0
    for key, text in (("conversions_impl", "scipy stand-in (fairmotion fork absent: parity UNPINNED)"),
                      ("motion_impl", "stand-in (fairmotion absent: get_pose_by_time and the pose interpolation written from its published "
                                      "source, parity UNPINNED; PyBullet absent: joint types from the URDF, parity UNPINNED)"),
                      ("augment_impl", "preprocess_DIP_TC_new.py executed (runpy): its own load_and_augment_dip_motion")):
        out[key] = np.frombuffer(text.encode(), dtype=np.uint8).copy()
    path = os.path.join(HERE, "tip_motion_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 100 * 1024


if __name__ == "__main__":
    main()
