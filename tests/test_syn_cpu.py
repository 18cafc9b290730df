"""tip_amd.syndata without a GPU: the oracle the GPU tests compare against (tests/syn_oracle.py) held to the reference-generated golden
(tests/golden/tip_syn_golden.npz: the reference script's own imu and constrs of three motions), the conditions that fixture was built
under, the candidate grids, the C-ABI surface of tip_syn_*, and everything synthesize, Skeleton and combine_motions refuse before they
touch a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import syn_oracle as so
from tip_amd import kinematics as kin
from tip_amd import lib as tlib
from tip_amd import syndata as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tip_syn_skel_bytes": 1, "tip_syn_grid_bytes": 1, "tip_syn_poses": 9, "tip_syn_imu": 6, "tip_syn_sbp": 8}      # name: arguments
FP64_BOUND = 1e-12                              # the oracle against the reference's own arrays (the issue's figure)
GAP_GUARD, MARGIN_GUARD = 1e-8, 1e-5            # the fixture's conditions: argmin gap on on-frames, distance of the minimum from V_THRES


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "tip_syn_golden.npz"))


@pytest.fixture(scope="module")
def table(golden):
    return {k[len("table/"):]: golden[k] for k in golden.files if k.startswith("table/")}


@pytest.fixture(scope="module")
def oracle_runs(golden, table):
    """The oracle on the fixture's three motions, once."""
    return {t: so.synthesize(table, golden[f"{t}/q"], float(golden[f"{t}/scale"])) for t in "ABC"}


# ---- the oracle against the reference-generated golden ------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_oracle_matches_the_golden(golden, oracle_runs, tag):
    imu, constrs, _ = oracle_runs[tag]
    g_imu, g_c = golden[f"{tag}/imu"], golden[f"{tag}/constrs"]
    e_imu, e_off = float(np.abs(imu - g_imu).max()), float(np.abs(constrs - g_c).max())
    print(f"{tag}: oracle - golden imu {e_imu:.2e}, offsets {e_off:.2e}")
    assert imu.shape == g_imu.shape and constrs.shape == g_c.shape and g_c.shape[1] == 20 and g_imu.shape[1] == 72
    assert e_imu <= FP64_BOUND and e_off <= FP64_BOUND
    assert np.array_equal(constrs[:, 0::4], g_c[:, 0::4])
    assert not g_c[:2].any() and not g_c[-2:].any()                       # rows 0, 1, L - 2, L - 1 carry no search
    L = g_imu.shape[0]
    assert np.array_equal(g_imu[:4, 54:], np.tile(g_imu[4, 54:], (4, 1))) and np.array_equal(g_imu[L - 4:, 54:], np.tile(g_imu[L - 5, 54:], (4, 1)))


def test_the_fixture_meets_its_conditions(golden, oracle_runs):
    """Per SBP body over A and B: >= 5 on-frames, >= 20 off-frames, >= 2 switches; every on-frame's argmin gap >= 1e-8 and every
    frame's |min - V_THRES| >= 1e-5 (A, B and C) — so no comparison against the fixture has to leave a frame out."""
    assert golden["A/q"].shape == (64, 57) and golden["B/q"].shape == (120, 57) and golden["C/q"].shape == (24, 57)
    assert float(golden["A/scale"]) == 1.0 and float(golden["B/scale"]) == 1.7 * 1.07 / 1.6
    flags = {t: golden[f"{t}/constrs"][2:-2, 0::4] for t in "ABC"}
    for b in range(5):
        on = sum(int(flags[t][:, b].sum()) for t in "AB")
        off = sum(int((flags[t][:, b] == 0).sum()) for t in "AB")
        sw = sum(int((np.diff(flags[t][:, b]) != 0).sum()) for t in "AB")
        assert on >= 5 and off >= 20 and sw >= 2, (b, on, off, sw)
    gap = min(float(oracle_runs[t][2]["gap"][2:-2][flags[t] == 1].min()) for t in "ABC")
    margin = min(float(oracle_runs[t][2]["margin"][2:-2].min()) for t in "ABC")
    print(f"smallest on-frame argmin gap {gap:.3e}, smallest threshold margin {margin:.3e}")
    assert gap >= GAP_GUARD and margin >= MARGIN_GUARD
    for t in "ABC":                                                       # the trace covers exactly the searched rows
        tr = oracle_runs[t][2]
        assert np.isnan(tr["min"][:2]).all() and np.isnan(tr["min"][-2:]).all() and np.isfinite(tr["min"][2:-2]).all()
    assert bytes(golden["fk_impl"]).decode().count("UNPINNED") == 1 and "UNPINNED" in bytes(golden["conversions_impl"]).decode()


def test_the_fixed_pose_is_on_throughout_at_the_point_nearest_the_origin(golden, table):
    c = golden["C/constrs"]
    assert (golden["C/q"] == golden["C/q"][0]).all() and c[2:-2, 0::4].all()
    P = so.tracked_poses(table, golden["C/q"], 1.0)
    for b in range(5):
        lps = so.grid_points(so.SBP_CLASS[b])
        near = lps[int(np.argmin(np.linalg.norm(lps, axis=1)))]
        assert np.abs(c[2:-2, 4 * b + 1:4 * b + 4] - so.q2r(P[0, b, 3:]) @ near).max() <= FP64_BOUND, b


# ---- the grids -----------------------------------------------------------------------------------------------------------------------
def test_grids_have_the_references_points():
    assert [so.grid_points(c).shape[0] for c in range(3)] == [1782, 125, 6200]
    mine, theirs = syn.grid_axes(), so.grid_axes()
    assert [[len(a) for a in cls] for cls in mine] == [[9, 6, 33], [5, 5, 5], [31, 25, 8]]
    for cm, co in zip(mine, theirs):
        for a, b in zip(cm, co):
            assert np.array_equal(a, b)                                    # numpy's own values, to the bit
    raw = syn.pack_grids()
    n = ctypes.c_size_t()
    assert tlib.load().tip_syn_grid_bytes(ctypes.byref(n)) == 0 and raw.nbytes == n.value == 3 * (16 + 3 * 40 * 8)
    for c in range(3):
        rec = raw[c * 976:(c + 1) * 976]
        cnt = rec[:16].view("<i4")
        assert list(cnt[:3]) == [len(a) for a in mine[c]] and cnt[3] == 0
        ax = rec[16:].view("<f8").reshape(3, 40)
        for k in range(3):
            assert np.array_equal(ax[k, :cnt[k]], mine[c][k]) and not ax[k, cnt[k]:].any()
        # the ravel order the device decodes: i = (iy nx + ix) nz + iz
        pts = so.grid_points(c)
        i = np.arange(pts.shape[0])
        iz, ixy = i % cnt[2], i // cnt[2]
        assert np.array_equal(pts, np.stack([ax[0][ixy % cnt[0]], ax[1][ixy // cnt[0]], ax[2][iz]], axis=1))


# ---- surface -------------------------------------------------------------------------------------------------------------------------
def test_c_abi_surface(golden):
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert set(re.findall(r"TIP_API int (tip_syn_\w+)\(", hdr)) == set(NAMES)
    assert "synthetic data" in hdr and int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    raw = ctypes.CDLL(tlib.LIB_PATH)
    lib = tlib.load()
    for name, nargs in NAMES.items():
        m = re.search(r"TIP_API int " + name + r"\((.*?)\);", hdr, re.S)
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == nargs, name
        assert name in tlib.EXPORTS and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is lib.tip_forward.restype, name
    n = ctypes.c_size_t()
    assert lib.tip_syn_skel_bytes(ctypes.byref(n)) == 0 and n.value == 64 + 32 * 88 and lib.tip_syn_skel_bytes(None) == -1
    assert lib.tip_syn_grid_bytes(None) == -1
    sk = kin.Skeleton.from_table(golden)
    b = syn.pack_skeleton(sk)
    assert b.nbytes == n.value
    head = b[:64].view("<i4")
    assert head[0] == 19 and list(head[1:6]) == list(sk.sbp) and list(head[6:12]) == list(sk.imu) == [0, 15, 19, 2, 5, 11] and not head[12:].any()
    rec = b[64:].view(syn._SKEL_DTYPE)
    assert np.array_equal(rec["joint_xyz"][:19], sk.joint_xyz) and np.array_equal(rec["com_xyz"][:19], sk.com_xyz)        # fp64, unrounded
    assert np.array_equal(rec["joint_q"][:19], sk.joint_q) and list(rec["parent"][:19]) == list(sk.parent) and (rec["state_col"][19:] == -1).all()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)        # a non-null pointer: every call below returns before it would launch
    okp = (p, p, 57, p, 1, p, 9, p, None)
    for k in (0, 1, 3, 5, 7):
        args = list(okp)
        args[k] = None
        assert lib.tip_syn_poses(*args) == -1, k
    for k, bad in ((2, 56), (4, -1), (4, 0), (6, -1), (1, p + 4)):
        args = list(okp)
        args[k] = bad
        assert lib.tip_syn_poses(*args) == -1, k
    assert lib.tip_syn_poses(p, None, 57, None, 0, None, 0, None, None) == 0
    oki = (p, p, 1, 9, p, None)
    for k in (0, 1, 4):
        args = list(oki)
        args[k] = None
        assert lib.tip_syn_imu(*args) == -1, k
    assert lib.tip_syn_imu(p, p, -1, 9, p, None) == -1 and lib.tip_syn_imu(p, p, 1, -1, p, None) == -1 and lib.tip_syn_imu(None, None, 0, 0, None, None) == 0
    oks = (p, p, p, 1, 9, p, p, None)
    for k in (0, 1, 2, 5, 6):
        args = list(oks)
        args[k] = None
        assert lib.tip_syn_sbp(*args) == -1, k
    assert lib.tip_syn_sbp(p, p, p, -1, 9, p, p, None) == -1 and lib.tip_syn_sbp(p, p, p, 1, -1, p, p, None) == -1
    assert lib.tip_syn_sbp(None, None, None, 0, 0, None, None, None) == 0
    src = open(os.path.join(tlib.CSRC, "tip_syn.hip")).read()
    assert "asm" not in src and "getenv" not in src and "tip_env" not in src          # plain C++, no environment
    assert "tip_syn.hip" in open(os.path.join(tlib.CSRC, "Makefile")).read()


# ---- refusals, all before a device is touched ----------------------------------------------------------------------------------------
def test_skeleton_imu_bodies(golden, table):
    kin_golden = np.load(os.path.join(ROOT, "tests", "golden", "tip_kin_golden.npz"))
    plain = kin.Skeleton.from_table(kin_golden)                           # the kinematics fixture has no imu and still loads
    assert plain.imu is None and plain.n_links == 19
    with pytest.raises(ValueError, match="needs an `imu` array of six body indices"):
        syn.synthesize(plain, [np.zeros((9, 57))], [1.0], device="cpu")
    sk = kin.Skeleton.from_table(golden)
    assert list(sk.imu) == [0, 15, 19, 2, 5, 11] and [sk.names[i] for i in sk.imu[3:]] == ["lknee", "rknee", "upperneck"]
    assert np.array_equal(sk.pack(), plain.pack())                        # the fp32 table of tip_amd.kinematics does not change
    need = ("parent", "joint_xyz", "joint_q", "com_xyz", "state_col", "sbp")
    with pytest.raises(ValueError, match="imu is six body indices"):
        kin.Skeleton(*[table[k] for k in need], imu=[0, 15, 19, 2, 5])
    with pytest.raises(ValueError, match="imu is six body indices"):
        kin.Skeleton(*[table[k] for k in need], imu=[0, 15, 19, 2, 5, 20])
    q = [np.zeros((9, 57))]
    for imu, sbp, what in (([0, 15, 19, 2, 5, 5], None, "imu is 6 distinct"), ([0, 15, 19, 2, 5, 11], [3, 3, 15, 19, 0], "sbp is 5 distinct"),
                           ([0, 19, 15, 2, 5, 11], None, "are the bodies sbp"), ([0, 15, 19, 3, 5, 11], None, "are not SBP bodies")):
        bad = kin.Skeleton(*[table[k] if k != "sbp" or sbp is None else sbp for k in need], imu=imu)
        with pytest.raises(ValueError, match=what):
            syn.synthesize(bad, q, [1.0], device="cpu")


def test_from_urdf_reads_the_imu_bodies(tmp_path):
    import types
    names = ["a", "b", "c", "d", "e", "f", "g"]
    text = ['<robot name="toy"><link name="root"><inertial><origin xyz="0 0 0" rpy="0 0 0"/><mass value="1"/></inertial></link>']
    for i, n in enumerate(names):
        pa = "root" if i == 0 else names[i - 1]
        text.append(f'<link name="{n}"><inertial><origin xyz="0 0 0.1" rpy="0 0 0"/><mass value="1"/></inertial></link>')
        text.append(f'<joint name="{n}" type="fixed"><origin xyz="0 0 1" rpy="0 0 0"/><parent link="{pa}"/><child link="{n}"/></joint>')
    path = tmp_path / "toy.urdf"
    path.write_text("".join(text) + "</robot>")
    ci = types.SimpleNamespace(root=-1, joint_idx={"root": -1, **{n: i for i, n in enumerate(names)}}, nimble_state_map={},
                               lankle=0, rankle=1, lwrist=2, rwrist=3, lknee=4, rknee=5, upperneck=6)
    sk = kin.Skeleton.from_urdf(str(path), ci)
    assert list(sk.sbp) == [1, 2, 3, 4, 0] and list(sk.imu) == [0, 3, 4, 5, 6, 7]
    syn.check_skeleton(sk)
    del ci.upperneck                                                      # a char_info without them serves tip_amd.kinematics as before
    assert kin.Skeleton.from_urdf(str(path), ci).imu is None


def test_synthesize_refusals(golden):
    sk = kin.Skeleton.from_table(golden)
    ok = np.zeros((9, 57))
    with pytest.raises(ValueError, match="sequence 1 has 8 rows"):
        syn.synthesize(sk, [ok, np.zeros((8, 57))], [1.0, 1.0], device="cpu")
    with pytest.raises(ValueError, match=r"sequence 0 is \[L, >= 57\]"):
        syn.synthesize(sk, [np.zeros((9, 56))], [1.0], device="cpu")
    with pytest.raises(ValueError, match="one number per sequence"):
        syn.synthesize(sk, [ok, ok], [1.0], device="cpu")
    with pytest.raises(ValueError, match="no sequences"):
        syn.synthesize(sk, [], [], device="cpu")
    with pytest.raises(RuntimeError, match="cuda device"):              # valid inputs: only now the device is looked at
        syn.synthesize(sk, [ok], [1.0], device="cpu")
    rng = np.random.RandomState(0)
    s = [syn.body_scale(rng) for _ in range(200)]
    assert 1.7 * 0.9 / 1.6 <= min(s) < max(s) <= 1.7 * 1.1 / 1.6
    assert syn.body_scale(np.random.RandomState(5)) == 1.7 * np.random.RandomState(5).uniform(0.9, 1.1) / 1.6


def test_combine_motions_still_rejects_what_it_rejected():
    from tip_amd import data
    f = {"imu": np.zeros((50, 72)), "nimble_qdq": np.zeros((50, 114)), "constrs": np.zeros((50, 20))}
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        data.combine_motions([f], [1], device="cpu")
