"""tip_amd.motion without a GPU: the oracle the GPU tests compare against (tests/motion_oracle.py) held to the reference-generated golden
(tests/golden/tip_motion_golden.npz: the reference's own nimble_qdq of five pose files), the conditions that fixture was built under,
the time table and the row-count rule, load_pose_file on each key layout, the C-ABI surface of tip_motion_*, and everything
qdq_from_smpl refuses before it touches the library or a device.

A row has 114 columns as the reference lays them out (data_utils.py:152-159): 57 of q (root xyz, root axis-angle, 17 spherical joints),
then the root's v and w (57:63) and 51 zeros for the joints' velocities."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

import motion_oracle as mo
from tip_amd import kinematics as kin
from tip_amd import lib as tlib
from tip_amd import motion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tip_motion_tile": 2, "tip_motion_qdq": 15}                     # name: arguments
TAGS = ("A", "B", "C", "D", "E")
FRAMES = {"A": (40, 60.0, 72, False), "B": (50, 120.0, 156, True), "C": (37, 100.0, 72, True), "D": (2, 60.0, 72, True), "E": (1, 60.0, 72, True)}
ANGLE_GUARD, FRAME_GUARD = 1e-3, 1e-3
RATES = (60.0, 100.0, 120.0, 250.0, 59.94, 30.0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "tip_motion_golden.npz"))


def _seq(golden, tag):
    return golden[f"{tag}/poses"], float(golden[f"{tag}/fps"]), golden[f"{tag}/trans"] if f"{tag}/trans" in golden.files else None


@pytest.fixture(scope="module")
def oracle_runs(golden):
    """The oracle on the fixture's five motions, once."""
    out = {}
    for t in TAGS:
        poses, fps, trans = _seq(golden, t)
        out[t] = mo.qdq_from_smpl(poses, fps, trans)
    return out


# ---- the oracle against the reference-generated golden ------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_oracle_matches_the_golden(golden, oracle_runs, tag):
    """Within 1e-12 max(1, |value|): both sides use the same scipy primitives in another operation order, and the largest values are
    w <= pi / DT ~ 188, where a few ulps are about 1e-13."""
    ours, ref = oracle_runs[tag], golden[f"{tag}/qdq"]
    n, fps, width, has_trans = FRAMES[tag]
    poses, f, trans = _seq(golden, tag)
    assert poses.shape == (n, width) and f == fps and (trans is not None) == has_trans
    assert ours.shape == ref.shape == (mo.output_rows(n, fps), 114)
    err = float(np.abs(ours - ref).max()) if ref.size else 0.0
    print(f"{tag}: oracle - golden {err:.2e} over {ref.shape[0]} rows")
    assert np.all(np.abs(ours - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref)))
    assert not ref[:, 63:].any() and not ours[:, 63:].any()
    if not has_trans:                                                    # the DIP root rule ((1 - a) 0.95 + a 0.95 is 0.95 to an ulp)
        assert (ref[:, 0:2] == 0).all() and np.abs(ref[:, 2] - 0.95).max() <= 2.3e-16 and np.abs(ref[:, 57:60]).max() <= 2.3e-16 * 60


def test_the_fixture_meets_its_conditions(golden, oracle_runs):
    """Every emitted rotation angle and every neighbouring-frame relative rotation <= pi - 1e-3, time fps + 1e-5 at least 1e-3 away
    from an integer on every unclipped lookup (the clipped end is exact by construction) — so no comparison has to leave a row out.
    And the planted cases are there."""
    worst = [0.0, 0.0, 1.0]
    for t in TAGS:
        poses, fps, trans = _seq(golden, t)
        emitted, rel, frac = mo.conditions(poses, fps, trans)
        worst = [max(worst[0], emitted), max(worst[1], rel), min(worst[2], frac)]
    print(f"largest emitted angle {worst[0]:.6f}, largest neighbour rotation {worst[1]:.6f}, smallest frame-lookup margin {worst[2]:.4f}")
    assert worst[0] <= np.pi - ANGLE_GUARD and worst[1] <= np.pi - ANGLE_GUARD and worst[2] >= FRAME_GUARD
    assert [golden[f"{t}/qdq"].shape[0] for t in TAGS] == [39, 25, 22, 1, 0]
    assert not golden["A/poses"][:, 12:15].any() and not golden["A/qdq"][:, 9:12].any()              # lknee: exactly zero throughout
    assert np.abs(np.linalg.norm(golden["B/qdq"][:, 27:30], axis=1) - (np.pi - 2e-3)).max() < 1e-9   # lshoulder at pi - 2e-3
    assert np.linalg.norm(golden["C/poses"][:, 3:6], axis=1).min() > np.pi                             # lhip: source norms above pi ...
    assert np.linalg.norm(golden["C/qdq"][:, 3:57].reshape(-1, 3), axis=1).max() <= np.pi             # ... come back within it
    assert abs(worst[1] - 2.0) < 1e-9                                                                   # lelbow: 2 rad between neighbours
    for key in ("conversions_impl", "motion_impl"):
        assert "UNPINNED" in bytes(golden[key]).decode()
    assert bytes(golden["motion_impl"]).decode().startswith("stand-in") and "executed" in bytes(golden["augment_impl"]).decode()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "tip_motion_golden.npz")) < 100 * 1024


def test_the_joint_order_is_the_characters(golden):
    sk = kin.Skeleton.from_table(golden)
    want = [0, 1, 4, 7, 3, 6, 9, 13, 16, 18, 12, 15, 14, 17, 19, 2, 5, 8]
    assert list(motion.joint_table(sk)) == list(motion.joint_table(None)) == list(mo.JOINTS) == want
    assert motion.SMPL_JOINTS == mo.SMPL_JOINTS and len(motion.SMPL_JOINTS) == 24


# ---- the time table and K ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fps", RATES)
def test_the_time_table_is_the_references_running_sum(fps):
    """np.cumsum over [0.0075, DT, DT, ...] equals the loop `cur_time += DT` bit for bit up to 40 000 rows, and so does the K it implies."""
    table = mo.time_table(40001)
    assert np.array_equal(table, motion.time_table(40001))
    loop = mo.time_loop(1e9, cap=40001)
    assert table.tobytes() == loop.tobytes()
    for n in (1, 2, 3, 37, 40, 50, 1001, int(40000 * fps / 60)):
        length = (n - 1) * (1.0 / fps)
        K = len(mo.time_loop(length))
        assert K == mo.output_rows(n, fps) == motion.output_rows(n, fps) == int(np.count_nonzero(table < length)), (n, fps)
        assert K <= 40000
    assert motion.output_rows(0, fps) == 0 and motion.output_rows(1, fps) == 0
    with pytest.raises(ValueError, match="positive"):
        motion.output_rows(10, 0.0)


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def test_load_pose_file_on_each_key_layout(tmp_path, golden):
    pa, _, _ = _seq(golden, "A")
    pb, fb, tb = _seq(golden, "B")
    pc, fc, tc = _seq(golden, "C")
    ori17, acc17 = np.random.RandomState(0).randn(40, 17, 3, 3), np.random.RandomState(1).randn(40, 17, 3)
    dip = tmp_path / "01.pkl"                                            # DIP-IMU: gt wider than 72, no frame rate, no trans
    with open(dip, "wb") as f:
        pickle.dump({"gt": np.concatenate([pa, np.ones((40, 3))], axis=1), "imu_ori": ori17, "imu_acc": acc17}, f, protocol=2)
    d = motion.load_pose_file(str(dip))
    assert np.array_equal(d["poses"], pa) and d["poses"].shape == (40, 72) and d["trans"] is None and d["fps"] == 60.0
    assert np.array_equal(d["ori"], ori17) and np.array_equal(d["acc"], acc17)
    amass = tmp_path / "B1_poses.npz"                                    # AMASS: poses [n, 156], trans, mocap_framerate
    np.savez(amass, poses=pb, trans=tb, mocap_framerate=np.float64(fb), gender="neutral")
    d = motion.load_pose_file(str(amass))
    assert np.array_equal(d["poses"], pb) and np.array_equal(d["trans"], tb) and d["fps"] == 120.0 and d["ori"] is None and d["acc"] is None
    tcg = tmp_path / "acting1_poses.npz"                                 # TotalCapture ground truth: frame_rate
    np.savez(tcg, poses=pc, trans=tc, frame_rate=np.float64(fc))
    d = motion.load_pose_file(str(tcg))
    assert np.array_equal(d["poses"], pc) and d["fps"] == 100.0 and np.array_equal(d["trans"], tc)
    tci = tmp_path / "s1_acting1.pkl"                                    # TotalCapture readings: ori / acc of six sensors
    with open(tci, "wb") as f:
        pickle.dump({"ori": ori17[:, :6], "acc": acc17[:, :6], "poses": pc}, f, protocol=2)
    d = motion.load_pose_file(str(tci))
    assert d["ori"].shape == (40, 6, 3, 3) and d["acc"].shape == (40, 6, 3) and d["fps"] == 60.0
    both = tmp_path / "both.npz"                                         # mocap_framerate wins over frame_rate, gt over poses
    np.savez(both, gt=pa, poses=pc, mocap_framerate=np.float64(30.0), frame_rate=np.float64(100.0))
    d = motion.load_pose_file(str(both))
    assert d["fps"] == 30.0 and np.array_equal(d["poses"], pa)
    with pytest.raises(ValueError, match="neither .npz nor .pkl"):
        motion.load_pose_file(str(tmp_path / "x.bvh"))
    np.savez(tmp_path / "empty.npz", trans=tb)
    with pytest.raises(ValueError, match="neither poses .* nor readings"):
        motion.load_pose_file(str(tmp_path / "empty.npz"))
    only = tmp_path / "readings.pkl"                                     # a file of readings only loads, and is refused as a pose file
    with open(only, "wb") as f:
        pickle.dump({"ori": ori17[:, :6], "acc": acc17[:, :6]}, f, protocol=2)
    assert motion.load_pose_file(str(only))["poses"] is None
    with pytest.raises(ValueError, match="has no poses"):
        motion.real_files([str(only)], [str(only)], np.eye(3), range(6))
    with pytest.raises(ValueError, match="has no IMU readings"):
        motion.real_files([str(amass)], [str(amass)], np.eye(3), range(6))
    with pytest.raises(ValueError, match="1 pose files for 2 IMU files"):
        motion.real_files([str(amass)], [str(amass), str(dip)], np.eye(3), range(6))


# ---- refusals, all before the library or a device is touched -------------------------------------------------------------------------
def test_qdq_from_smpl_refusals(golden, monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(tlib, "load", no_library)
    ok, tr = np.zeros((5, 72)), np.zeros((5, 3))
    with pytest.raises(ValueError, match="no sequences"):
        motion.qdq_from_smpl([], 60.0)
    with pytest.raises(ValueError, match=r"sequence 1 is \[n, >= 66\]"):
        motion.qdq_from_smpl([ok, np.zeros((5, 65))], 60.0)
    with pytest.raises(ValueError, match=r"sequence 0 is \[n, >= 66\]"):
        motion.qdq_from_smpl([np.zeros(72)], 60.0)
    with pytest.raises(ValueError, match="fps is positive and finite"):
        motion.qdq_from_smpl([ok], 0.0)
    with pytest.raises(ValueError, match="fps is positive and finite"):
        motion.qdq_from_smpl([ok, ok], [60.0, -1.0])
    with pytest.raises(ValueError, match="fps is positive and finite"):
        motion.qdq_from_smpl([ok], np.nan)
    with pytest.raises(ValueError, match="one number or one per sequence"):
        motion.qdq_from_smpl([ok, ok], [60.0, 60.0, 60.0])
    with pytest.raises(ValueError, match="one entry .* per sequence"):
        motion.qdq_from_smpl([ok, ok], 60.0, [tr])
    with pytest.raises(ValueError, match="5 pose frames and 4 trans frames"):
        motion.qdq_from_smpl([ok], 60.0, [tr[:4]])
    with pytest.raises(ValueError, match=r"trans of sequence 1 is \[n, 3\]"):
        motion.qdq_from_smpl([ok, ok], 60.0, [None, np.zeros((5, 4))])
    with pytest.raises(TypeError, match="Skeleton"):
        motion.qdq_from_smpl([ok], 60.0, skel={"names": []})
    table = {k[len("table/"):]: golden[k] for k in golden.files if k.startswith("table/")}
    names = [str(n) for n in table["names"]]
    names[3] = "ltoes"                                                   # a skeleton joint with no SMPL name
    with pytest.raises(ValueError, match="'ltoes' is none of the SMPL joints"):
        motion.qdq_from_smpl([ok], 60.0, skel=kin.Skeleton.from_table(dict(table, names=np.array(names))))
    names[3] = "lhand"                                                   # an SMPL joint beyond the 22 that the files share
    with pytest.raises(ValueError, match="'lhand' is none of the SMPL joints 0 .. 21"):
        motion.qdq_from_smpl([ok], 60.0, skel=kin.Skeleton.from_table(dict(table, names=np.array(names))))
    col = table["state_col"].copy()
    col[0] = col[1]                                                      # two joints in one column, one column empty
    with pytest.raises(ValueError, match="each once"):
        motion.qdq_from_smpl([ok], 60.0, skel=kin.Skeleton.from_table(dict(table, state_col=col)))
    col = table["state_col"].copy()
    col[0] = -1
    with pytest.raises(ValueError, match="17 spherical joints"):
        motion.qdq_from_smpl([ok], 60.0, skel=kin.Skeleton.from_table(dict(table, state_col=col)))
    with pytest.raises(RuntimeError, match="cuda device"):              # valid inputs: only now the device is looked at
        motion.qdq_from_smpl([ok], 60.0, [tr], device="cpu")


# ---- surface -------------------------------------------------------------------------------------------------------------------------
def test_c_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert set(re.findall(r"TIP_API int (tip_motion_\w+)\(", hdr)) == set(NAMES) == {n for n in tlib.EXPORTS if n.startswith("tip_motion_")}
    assert "---- motion:" in hdr
    raw = ctypes.CDLL(tlib.LIB_PATH)
    lib = tlib.load()
    for name, nargs in NAMES.items():
        m = re.search(r"TIP_API int " + name + r"\((.*?)\);", hdr, re.S)
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == nargs, name
        assert hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is lib.tip_forward.restype, name
    rows, slots = ctypes.c_int(), ctypes.c_int()
    assert lib.tip_motion_tile(ctypes.byref(rows), ctypes.byref(slots)) == 0 and slots.value == 19 and rows.value >= 1
    assert lib.tip_motion_tile(None, ctypes.byref(slots)) == -1 and lib.tip_motion_tile(ctypes.byref(rows), None) == -1
    src = open(os.path.join(tlib.CSRC, "tip_motion.hip")).read()
    assert "asm" not in src and "getenv" not in src and "tip_env" not in src          # plain C++, no environment
    mk = open(os.path.join(tlib.CSRC, "Makefile")).read()
    assert mk.count("tip_motion.hip") == 2                               # in SRCS and in the resource-usage report


def test_arguments_the_host_can_check_are_refused_before_any_launch():
    lib = tlib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)            # a non-null pointer: every call below returns before it would launch
    #      poses ldp trans flags in out fps count n_in n_out times n_times joints qdq stream
    ok = (p, 66, p, p, p, p, p, 1, 5, 3, p, 8, p, p, None)
    for k in (0, 4, 5, 6, 10, 12, 13):                                   # null pointers with non-zero counts
        args = list(ok)
        args[k] = None
        assert lib.tip_motion_qdq(*args) == -1, k
    for k, bad in ((1, 65), (1, 0), (7, -1), (8, -1), (9, -1), (11, -1), (7, 0), (8, 0), (11, 0), (0, p + 4), (13, p + 4), (10, p + 4)):
        args = list(ok)
        args[k] = bad
        assert lib.tip_motion_qdq(*args) == -1, (k, bad)
    args = list(ok)
    args[2] = None                                                       # per-sequence flags without a trans array
    assert lib.tip_motion_qdq(*args) == -1
    # zero sequences, and sequences that give no rows, are a successful no-op
    assert lib.tip_motion_qdq(None, 66, None, None, None, None, None, 0, 0, 0, None, 0, None, None, None) == 0
    assert lib.tip_motion_qdq(p, 72, None, None, p, p, p, 2, 2, 0, None, 0, None, None, None) == 0
