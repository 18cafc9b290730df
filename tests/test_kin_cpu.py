"""tip_amd.kinematics without a GPU: the C-ABI surface of tip_kin_*, Skeleton.from_urdf (on the reference's URDF where it exists, on
a three-link URDF written here, and its refusals), the oracle the GPU tests compare against (tests/kin_oracle.py) held to the
reference-generated golden (tests/golden/tip_kin_golden.npz: FK, the teacher-forced root track, the seven metrics), and
track_replay's row conventions and refusals."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import kin_oracle as ko
from tip_amd import kinematics as kin
from tip_amd import lib as tlib
from tip_amd.replay import ReplayResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
NAMES = {"tip_kin_skel_bytes": 1, "tip_kin_carry_bytes": 2, "tip_kin_fk": 7, "tip_kin_track_reset": 7, "tip_kin_track": 15,
         "tip_kin_metrics": 14}                 # name: number of arguments
FP64_BOUND = 1e-11                              # the project's bound for an fp64 restatement against its reference


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "tip_kin_golden.npz"))


@pytest.fixture(scope="module")
def table(golden):
    return {k[len("table/"):]: golden[k] for k in golden.files if k.startswith("table/")}


# ---- surface -------------------------------------------------------------------------------------------------------------------------
def test_c_abi_surface():
    """Every tip_kin_* name is declared in the header, exported by the library and bound in lib.py; the ABI is still 5; null pointers
    and negative counts return -1 and a zero count returns 0, all before any launch."""
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert set(re.findall(r"TIP_API int (tip_kin_\w+)\(", hdr)) == set(NAMES)
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    raw = ctypes.CDLL(tlib.LIB_PATH)
    lib = tlib.load()
    for name, nargs in NAMES.items():
        m = re.search(r"TIP_API int " + name + r"\((.*?)\);", hdr, re.S)
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == nargs, name
        assert name in tlib.EXPORTS and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is lib.tip_forward.restype, name
    assert lib.tip_abi_version() == 5 and tlib.TIP_ABI_VERSION == 5
    n = ctypes.c_size_t()
    assert lib.tip_kin_skel_bytes(ctypes.byref(n)) == 0 and n.value == 32 + 32 * 48 and lib.tip_kin_skel_bytes(None) == -1
    assert lib.tip_kin_carry_bytes(3, ctypes.byref(n)) == 0 and n.value % 8 == 0 and n.value >= 3 * (24 + 33 * 7 * 4 + 16)
    one = ctypes.c_size_t()
    assert lib.tip_kin_carry_bytes(1, ctypes.byref(one)) == 0 and n.value == 3 * one.value
    assert lib.tip_kin_carry_bytes(-1, ctypes.byref(n)) == -1 and lib.tip_kin_carry_bytes(3, None) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)        # a non-null pointer: every call below returns before it would launch
    assert lib.tip_kin_fk(None, p, 57, 4, p, None, None) == -1 and lib.tip_kin_fk(p, None, 57, 4, p, None, None) == -1
    assert lib.tip_kin_fk(p, p, 57, 4, None, None, None) == -1 and lib.tip_kin_fk(p, p, 57, -1, p, None, None) == -1
    assert lib.tip_kin_fk(p, p, 56, 4, p, None, None) == -1 and lib.tip_kin_fk(p, p, 57, 0, p, None, None) == 0
    assert lib.tip_kin_track_reset(None, p, 4, None, 1, p, None) == -1 and lib.tip_kin_track_reset(p, None, 4, None, 1, p, None) == -1
    assert lib.tip_kin_track_reset(p, p, 4, None, -1, p, None) == -1 and lib.tip_kin_track_reset(p, p, 4, None, 1, None, None) == -1
    assert lib.tip_kin_track_reset(p, p, -1, None, 1, p, None) == -1 and lib.tip_kin_track_reset(p, p, 4, None, 0, None, None) == 0
    ok = (p, p, 4, None, p, p, 1, 8, p, p, 20, None, p, p, None)
    for k in (0, 1, 4, 5, 8, 9, 12, 13):           # each required pointer in turn
        args = list(ok)
        args[k] = None
        assert lib.tip_kin_track(*args) == -1, k
    for k, bad in ((2, -1), (6, -1), (7, -1), (10, 12)):      # n_slots, count, n_rows, a c_t width that is neither 8 nor 20
        args = list(ok)
        args[k] = bad
        assert lib.tip_kin_track(*args) == -1, k
    args = list(ok)
    args[6] = 0
    assert lib.tip_kin_track(*args) == 0
    okm = (p, p, p, p, p, p, 1, 30, 6, 119, 299, 599, p, None)
    for k in (0, 1, 2, 3, 4, 5, 12):
        args = list(okm)
        args[k] = None
        assert lib.tip_kin_metrics(*args) == -1, k
    for k in (6, 7, 8):
        args = list(okm)
        args[k] = -1
        assert lib.tip_kin_metrics(*args) == -1, k
    args = list(okm)
    args[6] = 0
    assert lib.tip_kin_metrics(*args) == 0
    # the kernels keep to plain C++: no assembly in the new source
    src = open(os.path.join(tlib.CSRC, "tip_kin.hip")).read()
    assert "asm" not in src and "getenv" not in src and "tip_env" not in src


def test_pack_is_the_layout_the_header_gives(golden):
    sk = kin.Skeleton.from_table(golden)
    b = sk.pack()
    n = ctypes.c_size_t()
    assert tlib.load().tip_kin_skel_bytes(ctypes.byref(n)) == 0 and b.nbytes == n.value
    head = b[:32].view("<i4")
    assert head[0] == 19 and list(head[1:6]) == [3, 6, 15, 19, 0] and list(head[6:]) == [0, 0]
    rec = b[32:].view("<i4").reshape(32, 12)
    assert list(rec[:19, 0]) == list(sk.parent) and list(rec[:19, 1]) == list(sk.state_col) and (rec[19:, 1] == -1).all()
    f = b[32:].view("<f4").reshape(32, 12)
    assert np.array_equal(f[:19, 2:5], sk.joint_xyz.astype(np.float32)) and np.array_equal(f[:19, 9:12], sk.com_xyz.astype(np.float32))
    assert np.array_equal(f[:, 5:9], np.tile(np.float32([0, 0, 0, 1]), (32, 1)))


# ---- from_urdf -----------------------------------------------------------------------------------------------------------------------
def _char_info(names, cols, sbp):
    """A char-info module for a toy URDF: joint_idx, nimble_state_map (from the wanted state columns) and the SBP bodies."""
    ci = types.SimpleNamespace(root=-1, joint_idx={"root": -1}, nimble_state_map={-1: 0})
    for i, (n, c) in enumerate(zip(names, cols)):
        ci.joint_idx[n] = i
        ci.nimble_state_map[i] = None if c is None else (c - 6) // 3 + 1
    for k, v in zip(ko.SBP_BODIES, sbp):
        setattr(ci, k, v)
    return ci


def _urdf(joints, root_inertial='<origin xyz="0 0 0" rpy="0 0 0"/>'):
    """joints: (name, type, parent, joint xyz, joint rpy, com xyz, inertial rpy)."""
    out = [f'<robot name="toy"><link name="root"><inertial>{root_inertial}<mass value="1"/></inertial></link>']
    for n, kind, pa, xyz, rpy, com, irpy in joints:
        out.append(f'<link name="{n}"><inertial><origin xyz="{com}" rpy="{irpy}"/><mass value="1"/></inertial></link>')
        out.append(f'<joint name="{n}" type="{kind}"><origin xyz="{xyz}" rpy="{rpy}"/><parent link="{pa}"/><child link="{n}"/></joint>')
    out.append("</robot>")
    return "".join(out)


THREE = [("a", "spherical", "root", "0 0 1", "0 0 0", "0.5 0 0", "0 0 0"),
         ("b", "fixed", "a", "1 0 0", "0 0 1.5707963267948966", "0 0.25 0", "0 0 0"),
         ("c", "spherical", "b", "0 2 0", "0 0 0", "0 0 0.125", "0 0 0")]
THREE_INFO = dict(names=["a", "b", "c"], cols=[6, None, 9], sbp=[0, 2, 1, 1, -1])


def test_from_urdf_on_a_three_link_urdf_by_hand(tmp_path):
    """root -a(spherical)-> a -b(fixed, turned 90 degrees about z)-> b -c(spherical)-> c, positions worked out by hand."""
    path = tmp_path / "toy.urdf"
    path.write_text(_urdf(THREE))
    sk = kin.Skeleton.from_urdf(str(path), _char_info(**THREE_INFO))
    assert sk.n_links == 3 and list(sk.parent) == [0, 1, 2] and list(sk.state_col) == [6, -1, 9] and list(sk.sbp) == [1, 3, 2, 2, 0]
    assert sk.names == ["root", "a", "b", "c"]
    s = np.sqrt(0.5)
    assert np.allclose(sk.joint_q, [[0, 0, 0, 1], [0, 0, s, s], [0, 0, 0, 1]], atol=1e-15)
    t = sk.table()
    # the zero pose at (10, 20, 30): a's frame at +z 1; b's at a + x 1, turned so that its x is the world's y; c's at b + (b's y) 2
    # = world -x 2.  COMs: a + x 0.5; b + (b's y 0.25 = world -x 0.25); c + z 0.125.
    q = np.zeros((2, 57))
    q[:, :3] = [10, 20, 30]
    q[1, 6:9] = [0, np.pi / 2, 0]               # a turned 90 degrees about y: its x points along world -z
    g, jf = ko.fk(t, q)
    assert np.allclose(jf[0, :, :3], [[10, 20, 30], [10, 20, 31], [11, 20, 31], [9, 20, 31]], atol=1e-14)
    assert np.allclose(g[0, :, :3], [[10, 20, 30], [10.5, 20, 31], [10.75, 20, 31], [9, 20, 31.125]], atol=1e-14)
    assert np.allclose(jf[0, :, 3:], [[0, 0, 0, 1], [0, 0, 0, 1], [0, 0, s, s], [0, 0, s, s]], atol=1e-15)
    # with a turned: a's x -> world -z, a's y stays, a's z -> world x.  b's frame at a + (-z) 1 = (10, 20, 30); b's y = a's -x = world z,
    # so c's frame = b + 2 z = (10, 20, 32); a's COM = a + 0.5 (-z); b's COM = b + 0.25 z; c's z = a's z = world x: COM = c + 0.125 x
    assert np.allclose(jf[1, :, :3], [[10, 20, 30], [10, 20, 31], [10, 20, 30], [10, 20, 32]], atol=1e-14)
    assert np.allclose(g[1, :, :3], [[10, 20, 30], [10, 20, 30.5], [10, 20, 30.25], [10.125, 20, 32]], atol=1e-14)
    # the oracle's own URDF reading gives the same table
    t2 = ko.read_urdf(str(path), _char_info(**THREE_INFO))
    for k in ("parent", "joint_xyz", "joint_q", "com_xyz", "state_col", "sbp"):
        assert np.allclose(t[k], t2[k], atol=1e-15), k


def test_from_urdf_refusals(tmp_path):
    def build(text, **info):
        p = tmp_path / "bad.urdf"
        p.write_text(text)
        return kin.Skeleton.from_urdf(str(p), _char_info(**(info or THREE_INFO)))

    turned = list(THREE)
    turned[2] = ("c", "spherical", "b", "0 2 0", "0 0 0", "0 0 0.125", "0 0.1 0")
    with pytest.raises(ValueError, match="non-zero inertial rpy"):
        build(_urdf(turned))
    with pytest.raises(ValueError, match="root's inertial origin is not zero"):
        build(_urdf(THREE, root_inertial='<origin xyz="0 0.01 0" rpy="0 0 0"/>'))
    with pytest.raises(ValueError, match="root's inertial origin is not zero"):
        build(_urdf(THREE, root_inertial='<origin xyz="0 0 0" rpy="0.2 0 0"/>'))
    hinge = list(THREE)
    hinge[0] = ("a", "revolute", "root", "0 0 1", "0 0 0", "0.5 0 0", "0 0 0")
    with pytest.raises(ValueError, match="'revolute'; only spherical and fixed"):
        build(_urdf(hinge))
    chain = [(f"l{i}", "fixed", "root" if i == 0 else f"l{i - 1}", "0 0 1", "0 0 0", "0 0 0", "0 0 0") for i in range(33)]
    with pytest.raises(ValueError, match="33 links; the device table holds 32"):
        build(_urdf(chain), names=[f"l{i}" for i in range(33)], cols=[None] * 33, sbp=[0, 1, 2, 3, -1])
    assert build(_urdf(chain[:32]), names=[f"l{i}" for i in range(32)], cols=[None] * 32, sbp=[0, 1, 2, 3, -1]).n_links == 32


@pytest.mark.skipif(not os.path.exists(os.path.join(REF, "data", "amass.urdf")), reason="the reference checkout is not here")
def test_from_urdf_on_the_reference_equals_the_golden_table(golden, table):
    import importlib.util
    spec = importlib.util.spec_from_file_location("kin_test_char_info", os.path.join(REF, "amass_char_info.py"))
    info = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(info)
    sk = kin.Skeleton.from_urdf(os.path.join(REF, "data", "amass.urdf"), info)
    assert sk.n_links == 19 and int((sk.state_col >= 0).sum()) == 17
    for k, v in sk.table().items():
        assert np.array_equal(v, table[k]), k
    assert np.array_equal(kin.Skeleton.from_table(golden).pack(), sk.pack())


# ---- the oracle against the reference-generated golden ------------------------------------------------------------------------------
def test_oracle_fk_matches_the_golden(golden, table):
    g, jf = ko.fk(table, golden["poses/q"])
    eg, ej = float(np.abs(g - golden["poses/pq_g"]).max()), float(np.abs(jf - golden["poses/pq_jf"]).max())
    print(f"oracle FK - golden: pq_g {eg:.2e}, pq_jf {ej:.2e}")
    assert eg <= FP64_BOUND and ej <= FP64_BOUND
    assert golden["poses/q"].shape == (32, 57) and not golden["poses/q"][0].any()
    assert np.array_equal(g[0, :, 3:], np.tile([0.0, 0, 0, 1], (20, 1)))            # the zero pose: A2Q is exact at angle 0
    g32 = ko.fk(table, golden["poses/q"], dtype=np.float32)[0]
    assert g32.dtype == np.float32 and 0 < np.abs(g32 - g).max() < 1e-5


@pytest.mark.parametrize("tag,frames", [("track0", 60), ("track1", 90)])
def test_oracle_track_matches_the_golden_teacher_forced(golden, table, tag, frames):
    """Inputs: the golden's qdq[3:114] and ct of every step; outputs: its qdq[:3] and viz_locs (the real RTRunnerMin.step)."""
    qdq, ct, valid = golden[tag + "/qdq"], golden[tag + "/ct"], golden[tag + "/valid"]
    assert qdq.shape == (frames - 1, 114) and ct.shape == (frames - 1, 20) and not valid[:5].any() and valid[5:].all()
    root, viz, tr = ko.track(table, golden[tag + "/s_init"], qdq[:, 3:], ct, valid)
    er, ev = float(np.abs(root - qdq[:, :3]).max()), float(np.abs(viz - golden[tag + "/viz_locs"]).max())
    print(f"{tag}: oracle root - golden {er:.2e}, viz_locs {ev:.2e}")
    assert er <= FP64_BOUND and ev <= FP64_BOUND
    # the case is sound: every flag combination, the clip both binding and idle, and clear of the one discontinuous branch
    fl = tr["flags"][valid]
    assert min(int(((fl[:, 0] == a) & (fl[:, 1] == b)).sum()) for a in (0, 1) for b in (0, 1)) >= 5
    on = valid & (tr["flags"].max(1) == 1)
    assert int((tr["clip"] & on).sum()) >= 5 and int((~tr["clip"] & on).sum()) >= 20 and tr["margin"].min() > 0.1


@pytest.mark.parametrize("tag", ["track0", "track1"])
def test_oracle_metrics_match_the_golden(golden, table, tag):
    m = ko.evaluate(table, golden[tag + "/pred_qdq"], golden[tag + "/gt_qdq"])
    err = np.abs(m - golden[tag + "/metrics"])
    print(tag, dict(zip(ko.METRICS, np.round(m, 5))), "max error", float(err.max()))
    assert (err <= FP64_BOUND).all() and (m > 0).all()
    assert ko.root_indices(1000) == [119, 299, 599] == kin.root_indices(1000) and ko.root_indices(100) == [99, 99, 99]
    with pytest.raises(ValueError):
        ko.evaluate(table, golden[tag + "/pred_qdq"][:39], golden[tag + "/gt_qdq"][:39])


# ---- track_replay and evaluate: conventions and refusals that need no device -------------------------------------------------------
def _fake_results(lengths, nc=20):
    rng = np.random.RandomState(0)
    out = []
    for n in lengths:
        valid = np.zeros(n, bool)
        valid[6:] = True
        out.append(ReplayResult(rng.randn(n, 111).astype(np.float32), rng.randn(n, nc).astype(np.float32), valid, None))
    return out


def test_track_replay_row_conventions(golden, monkeypatch):
    """track_replay concatenates the recordings, tracks them in one call and hands back the script's rows: qdq = root | s_rest.  The
    device call is replaced by a recorder here (the GPU tests run the real one)."""
    import torch
    sk = kin.Skeleton.from_table(golden)
    res = _fake_results([9, 1, 12])
    s0 = np.random.RandomState(1).randn(3, 114).astype(np.float32)
    seen = {}

    def fake_track(skel, s_init, s_rest, c_t, valid, offsets, device=None):
        seen.update(s_init=s_init, s_rest=s_rest, c_t=c_t, valid=valid, offsets=list(offsets))
        n = s_rest.shape[0]
        return torch.arange(n * 3, dtype=torch.float32).reshape(n, 3), torch.full((n, 5, 3), 100.0)

    monkeypatch.setattr(kin, "track", fake_track)
    out = kin.track_replay(sk, res, s0)
    assert seen["offsets"] == [0, 9, 10, 22] and seen["s_rest"].shape == (22, 111) and seen["valid"].dtype == bool
    assert np.array_equal(seen["s_init"], s0) and np.array_equal(seen["c_t"][9:10], res[1].c_t)
    assert [o[0].shape for o in out] == [(9, 114), (1, 114), (12, 114)] and [o[1].shape for o in out] == [(9, 5, 3), (1, 5, 3), (12, 5, 3)]
    assert np.array_equal(out[2][0][:, 3:], res[2].s_rest) and np.array_equal(out[2][0][:, :3], np.arange(30, 66).reshape(12, 3))
    assert out[0][0].dtype == np.float32


def test_track_replay_and_evaluate_refusals(golden):
    sk = kin.Skeleton.from_table(golden)
    res = _fake_results([9, 12])
    with pytest.raises(ValueError, match="no recordings"):
        kin.track_replay(sk, [], np.zeros((0, 114)))
    with pytest.raises(ValueError, match="s_init is \\[R, 114\\]"):
        kin.track_replay(sk, res, np.zeros((3, 114)))
    with pytest.raises(ValueError, match="c_t widths differ"):
        kin.track_replay(sk, [res[0], _fake_results([12], nc=8)[0]], np.zeros((2, 114)))
    bad = ReplayResult(res[0].s_rest, res[0].c_t[:5], res[0].valid, None)
    with pytest.raises(ValueError, match="not a ReplayResult of one length"):
        kin.track_replay(sk, [bad, res[1]], np.zeros((2, 114)))
    with pytest.raises(ValueError, match="sbp is five body indices"):
        kin.Skeleton([0], [[0, 0, 1]], [[0, 0, 0, 1]], [[0, 0, 0]], [6], [0, 1, 2, 0, 0])
    with pytest.raises(ValueError, match="parent comes before it"):
        kin.Skeleton([0, 3], np.zeros((2, 3)), np.tile([0, 0, 0, 1.0], (2, 1)), np.zeros((2, 3)), [6, 9], [0, 1, 2, 0, 0])
    with pytest.raises(ValueError, match="missing"):
        kin.Skeleton.from_table({"parent": [0]})
