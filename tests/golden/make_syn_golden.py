#!/usr/bin/env python3
"""Golden fixture of the REFERENCE's synthetic-data generator for tip_amd.syndata: the `imu` and `constrs` arrays that
data-gen-and-viz-bullet-new.py computes from a motion, through the script's own get_imu_readings_from_raw_motion_info and
get_all_contr_seqs_from_raw_motion_info (and so through data_utils.get_rot_center_sample_based).

Runs only in the build container (it reads the reference checkout).  The script is EXECUTED as it is (runpy.run_path, cwd at the
reference, sys.argv naming an empty --src_dir and a scratch --save_dir, so its module-level gen_data_all finds nothing to do), and its
two functions are then called on a raw_info built the way its get_raw_motion_info builds one.  What is not installed is stood in at
the module boundary only:
  * fairmotion.ops.conversions / quaternion -> make_runner_golden.install_stubs' scipy stand-ins; fairmotion.data.amass -> an empty
    module (only load_motion_amass, which is not called, names it);
  * pybullet, pybullet_data, bullet_client   -> empty modules (the script only touches them inside gen_data_job_single_core);
  * bullet_agent.SimAgent                    -> SynChar below: get_char_info, get_root_state, get_root_local_point_p and
    get_link_states over REAL forward kinematics of data/amass.urdf (tests/kin_oracle.py) with PyBullet's globalScaling on every joint
    and COM offset and ref_scale on the root translation.  PyBullet is not installed here, so PyBullet parity is UNPINNED and the
    fixture says so (`fk_impl`), as `conversions_impl` does for fairmotion.

tests/golden/tip_syn_golden.npz (data only):
  table/*   the kinematics table derived from the URDF and amass_char_info, plus imu: the body indices of root, lwrist, rwrist,
            lknee, rknee, upperneck
  A/*       64 frames at scale 1.0:            q [64, 57], scale, imu [64, 72], constrs [64, 20]
  B/*       120 frames at scale 1.7 * 1.07 / 1.6
  C/*       24 frames of one fixed pose at scale 1.0: every flag on from row 2 to row L - 3, the offsets R x (the grid point nearest
            the origin)
A and B are syn_oracle.motion: smooth sinusoidal joints and root on a clock that alternates slow and fast.  The generator ASSERTS, over
A and B together and per SBP body: at least 5 on-frames, at least 20 off-frames, at least 2 switches; on every on-frame the gap between
the least and the second-least residue is at least 1e-8; on every frame |least residue - V_THRES| is at least 1e-5.  These are
conditions on the fixture: with them no comparison against it has to leave a frame out.

usage: python tests/golden/make_syn_golden.py
"""
import os
import runpy
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
REF = "/root/reference"

import kin_oracle as ko                # noqa: E402
import make_runner_golden as mrg       # noqa: E402
import syn_oracle as so                # noqa: E402

IMU_BODIES = ("root", "lwrist", "rwrist", "lknee", "rknee", "upperneck")
SEQS = (("A", 64, 11, 1.0), ("B", 120, 12, 1.7 * 1.07 / 1.6))


class SynChar:
    """bullet_agent.SimAgent's accessors, as the script's get_raw_motion_info uses them, over FK of the scaled URDF."""

    def __init__(self, table, info, scale, conversions):
        self._table, self._info, self._scale, self._conv = so.scaled_table(table, scale), info, scale, conversions
        self._g = None

    def get_char_info(self):
        return self._info

    def set_rows(self, q):
        """All frames at once: the root xyz times ref_scale, then FK; frame() picks one."""
        q = np.array(q[:, :57], dtype=np.float64)
        q[:, :3] = q[:, :3] * self._scale
        self._all = ko.fk(self._table, q)[0]

    def frame(self, t):
        self._g = self._all[t]

    def get_root_state(self):
        return self._g[0, :3].copy(), self._g[0, 3:].copy(), np.zeros(3), np.zeros(3)

    def get_root_local_point_p(self, offset):
        p, Q, _, _ = self.get_root_state()
        return p + self._conv.Q2R(Q).dot(offset)

    def get_link_states(self, indices=None):
        (i,) = indices
        return self._g[i + 1, :3].copy(), self._g[i + 1, 3:].copy(), np.zeros(3), np.zeros(3)


def raw_info_of(robot, n, cst):
    """raw_info as get_raw_motion_info leaves it: per frame {joint index: 7 numbers}, the root's from the tracked point."""
    info = robot.get_char_info()
    out = []
    for t in range(n):
        robot.frame(t)
        cur = {}
        for idx in info.joint_idx.values():
            if idx == info.root:
                _, Q, _, _ = robot.get_root_state()
                cur[idx] = list(robot.get_root_local_point_p(cst.ROOT_COM_OFFSET)) + list(Q)
            else:
                st = robot.get_link_states([idx])
                cur[idx] = list(st[0]) + list(st[1])
        out.append(cur)
    return out


def run_reference_script():
    """Execute data-gen-and-viz-bullet-new.py itself; returns its globals."""
    for name in ("pybullet_data", "bullet_client", "fairmotion.data", "fairmotion.data.amass"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pybullet_data"].getDataPath = lambda: ""
    sys.modules["fairmotion.data"].amass = sys.modules["fairmotion.data.amass"]
    sys.modules["fairmotion"].data = sys.modules["fairmotion.data"]
    sys.path.insert(0, REF)
    cwd, argv = os.getcwd(), sys.argv
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "src")
        os.makedirs(src)
        os.chdir(REF)
        sys.argv = ["data-gen-and-viz-bullet-new.py", "--src_dir", src, "--save_dir", os.path.join(tmp, "out"), "--n_proc", "1"]
        try:
            return runpy.run_path(os.path.join(REF, "data-gen-and-viz-bullet-new.py"), run_name="__main__")
        finally:
            os.chdir(cwd)
            sys.argv = argv


def main():
    mrg.install_stubs(False)
    g = run_reference_script()
    assert g["USE_KNEE_RATHER_ANKLE_IMU"] is True
    import constants as cst
    from fairmotion.ops import conversions
    info = g["char_info"]
    table = ko.read_urdf(os.path.join(REF, "data", "amass.urdf"), info)
    table["imu"] = np.array([getattr(info, n) + 1 for n in IMU_BODIES], dtype=np.int32)
    out = {"table/" + k: v for k, v in table.items()}
    fixed = np.tile(so.motion(64, 13)[20:21, :57], (24, 1))
    seqs = [(tag, so.motion(n, seed)[:, :57], scale) for tag, n, seed, scale in SEQS] + [("C", fixed, 1.0)]
    traces = {}
    for tag, q, scale in seqs:
        robot = SynChar(table, info, scale, conversions)
        robot.set_rows(q)
        raw = raw_info_of(robot, q.shape[0], cst)
        imu = g["get_imu_readings_from_raw_motion_info"](robot, raw)
        constrs = g["get_all_contr_seqs_from_raw_motion_info"](robot, raw)
        o_imu, o_c, tr = so.synthesize(table, q, scale)
        flags = constrs[:, 0::4]
        print(tag, "frames", q.shape[0], "scale", round(scale, 6), "on-frames per body", flags.sum(0).astype(int).tolist(),
              "| oracle - reference: imu %.2e, offsets %.2e, flags equal %s" % (np.abs(o_imu - imu).max(), np.abs(o_c - constrs).max(),
                                                                               np.array_equal(o_c[:, 0::4], flags)))
        assert np.array_equal(o_c[:, 0::4], flags) and np.abs(o_imu - imu).max() < 1e-12 and np.abs(o_c - constrs).max() < 1e-12
        traces[tag] = (flags, tr)
        out.update({f"{tag}/q": q, f"{tag}/scale": np.float64(scale), f"{tag}/imu": imu, f"{tag}/constrs": constrs})
    # the conditions on the fixture
    for b in range(5):
        on = sum(int(traces[t][0][2:-2, b].sum()) for t in "AB")
        off = sum(int((traces[t][0][2:-2, b] == 0).sum()) for t in "AB")
        sw = sum(int((np.diff(traces[t][0][2:-2, b]) != 0).sum()) for t in "AB")
        print("body", b, "on", on, "off", off, "switches", sw)
        assert on >= 5 and off >= 20 and sw >= 2, (b, on, off, sw)
    gaps, margins = [], []
    for tag, (flags, tr) in traces.items():
        inner = np.zeros(flags.shape, bool)
        inner[2:-2] = True
        gaps.append(tr["gap"][inner & (flags == 1)])
        margins.append(tr["margin"][inner])
    gap, margin = float(np.concatenate(gaps).min()), float(np.concatenate(margins).min())
    print("smallest on-frame argmin gap %.3e, smallest threshold margin %.3e" % (gap, margin))
    assert gap >= 1e-8 and margin >= 1e-5, (gap, margin)
    # C: one fixed pose — every searched row is on, at R x (the grid point nearest the origin)
    fc, P = traces["C"][0], so.tracked_poses(table, fixed, 1.0)
    assert fc[2:-2].all() and not fc[:2].any() and not fc[-2:].any()
    for b in range(5):
        lps = so.grid_points(so.SBP_CLASS[b])
        near = lps[int(np.argmin(np.linalg.norm(lps, axis=1)))]
        assert np.abs(out["C/constrs"][2:-2, 4 * b + 1:4 * b + 4] - so.q2r(P[0, b, 3:]) @ near).max() < 1e-12, b
    conv = "scipy stand-in (fairmotion fork absent: parity UNPINNED)"
    fk_impl = "kin_oracle.fk stand-in with scaled offsets (PyBullet absent: getLinkState / globalScaling parity UNPINNED)"
    out["conversions_impl"] = np.frombuffer(conv.encode(), dtype=np.uint8).copy()
    out["fk_impl"] = np.frombuffer(fk_impl.encode(), dtype=np.uint8).copy()
    path = os.path.join(HERE, "tip_syn_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; FK:", fk_impl)
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
