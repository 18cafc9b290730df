"""tip_amd.motion on the device (csrc/tip_motion.hip) against the reference-generated golden (tests/golden/tip_motion_golden.npz) and
tests/motion_oracle.py.  The skeleton comes from the golden's table only.

THE BOUND is 1e-9 absolute, as tests/test_syn_gpu.py holds the same class of fp64 rotation chains to.  What to expect is about 1e-13:
the path is fp64 end to end on magnitudes <= pi through a few hundred operations, and the largest values are w <= pi / DT ~ 188 where an
ulp is 3e-14; tests/test_motion_cpu.py holds the fixture to rotation angles <= pi - 1e-3 and frame lookups 1e-3 away from an integer,
so no branch of either side can flip and no row is left out of any comparison.  Measured on an MI355X: 2.6e-14 against the golden,
8.9e-15 against the oracle on the fixture and on the tile-edge batch (CHANGELOG.md).

A row has 114 columns as the reference lays them out: 57 of q, the root's v and w (57:63) and 51 zeros.  Columns 0:63 are compared,
columns 63:114 must be exactly 0.0."""
import ctypes
import pickle

import numpy as np
import pytest
import torch

import motion_oracle as mo
import syn_oracle as so
from tip_amd import data
from tip_amd import kinematics as kin
from tip_amd import lib as tlib
from tip_amd import motion
from tip_amd import sensors
from tip_amd import syndata as syn

pytestmark = pytest.mark.gpu
BOUND = 1e-9
DATA_TOL = 2e-6                                  # tests/test_data_gpu.py: fp64 math on both sides, float32 storage
GAP_GUARD, MARGIN_GUARD = 1e-8, 1e-5             # tests/test_syn_gpu.py: the conditions under which SBP flags cannot flip
GOLDEN = np.load(__file__.replace("test_motion_gpu.py", "golden/tip_motion_golden.npz"))
TAGS = ("A", "B", "E", "C", "D")                 # the empty sequence in the middle of the batch
POSES = {t: GOLDEN[f"{t}/poses"] for t in TAGS}
FPS = {t: float(GOLDEN[f"{t}/fps"]) for t in TAGS}
TRANS = {t: GOLDEN[f"{t}/trans"] if f"{t}/trans" in GOLDEN.files else None for t in TAGS}
RATES = (60.0, 100.0, 120.0, 250.0)


@pytest.fixture(scope="module")
def skel():
    return kin.Skeleton.from_table(GOLDEN)


def _run(seqs, skel=None):
    """qdq_from_smpl on [(poses, fps, trans)] -> a list of numpy [K_i, 114]."""
    out = motion.qdq_from_smpl([s[0] for s in seqs], [s[1] for s in seqs], [s[2] for s in seqs], skel)
    base = out[0].untyped_storage().data_ptr()
    for o, s in zip(out, seqs):
        assert o.is_cuda and o.dtype == torch.float64 and tuple(o.shape) == (motion.output_rows(s[0].shape[0], s[1]), 114)
        assert o.untyped_storage().data_ptr() == base                      # views of one tensor
    return [o.cpu().numpy() for o in out]


@pytest.fixture(scope="module")
def clean(skel):
    """All five fixture sequences in ONE launch; every test below compares against these arrays and leaves them alone."""
    return dict(zip(TAGS, _run([(POSES[t], FPS[t], TRANS[t]) for t in TAGS], skel)))


@pytest.fixture(scope="module")
def edge_batch():
    """Sequences of tile - 1, tile, tile + 1 and 3 tile + 1 rows at 60 / 100 / 120 / 250 fps, and the oracle on them, once."""
    rows, slots = ctypes.c_int(), ctypes.c_int()
    assert tlib.load().tip_motion_tile(ctypes.byref(rows), ctypes.byref(slots)) == 0
    tile = rows.value
    seqs = []
    for i, (K, fps) in enumerate(((tile - 1, 60.0), (tile, 100.0), (tile + 1, 120.0), (tile, 250.0), (3 * tile + 1, 100.0), (tile - 1, 250.0))):
        n = 2
        while mo.output_rows(n, fps) < K:
            n += 1
        assert mo.output_rows(n, fps) == K
        p, tr = mo.source_motion(n, 40 + i, 72, with_trans=i != 1)
        seqs.append((p, fps, tr))
    return tile, seqs, [mo.qdq_from_smpl(*s) for s in seqs]


def _same(a, b):
    """Bit for bit, NaN included."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _compare(got, ref, what):
    assert got.shape == ref.shape and ref.shape[1] == 114, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    err = float(np.nanmax(np.abs(got[:, :63] - ref[:, :63]))) if ref.size and not np.isnan(ref[:, :63]).all() else 0.0
    print(f"{what}: {ref.shape[0]} rows, max |device - reference| {err:.2e}")
    assert err <= BOUND, what
    assert (got[:, 63:] == 0.0).all(), what
    return err


# ---- parity --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_parity_with_the_golden_and_the_oracle(clean, tag):
    _compare(clean[tag], GOLDEN[f"{tag}/qdq"], f"{tag} against the golden")
    _compare(clean[tag], mo.qdq_from_smpl(POSES[tag], FPS[tag], TRANS[tag]), f"{tag} against the oracle")
    if tag == "C":
        assert np.linalg.norm(clean[tag][:, 3:57].reshape(-1, 3), axis=1).max() <= np.pi      # source norms above pi come back within it
    if tag == "A":
        assert (clean[tag][:, 9:12] == 0.0).all() and (clean[tag][:, 0:3] == np.array([0.0, 0.0, 0.95])).all()


def test_the_default_joint_order_is_the_skeletons(clean):
    for t, q in zip(TAGS, _run([(POSES[t], FPS[t], TRANS[t]) for t in TAGS], None)):
        assert _same(q, clean[t]), t


# ---- independence --------------------------------------------------------------------------------------------------------------------
def test_each_sequence_alone_equals_its_rows_in_the_batch(skel, clean):
    for t in TAGS:
        (q,) = _run([(POSES[t], FPS[t], TRANS[t])], skel)
        assert _same(q, clean[t]), t
    # a scalar frame rate, device tensors, and a batch without any trans (the null pointer path)
    (q,) = _run([(torch.from_numpy(POSES["C"]).cuda(), 100.0, torch.from_numpy(TRANS["C"]).cuda())], skel)
    assert _same(q, clean["C"])
    a, a2 = (o.cpu().numpy() for o in motion.qdq_from_smpl([POSES["A"], POSES["A"]], 60.0))
    assert _same(a, clean["A"]) and _same(a2, clean["A"])


# ---- tile edges ----------------------------------------------------------------------------------------------------------------------
def test_tile_edges_at_mixed_frame_rates(edge_batch):
    tile, seqs, refs = edge_batch
    assert sorted({s[1] for s in seqs} | {60.0}) == sorted(RATES) and [r.shape[0] for r in refs] == [tile - 1, tile, tile + 1, tile, 3 * tile + 1, tile - 1]
    for i, (q, r) in enumerate(zip(_run(seqs), refs)):
        _compare(q, r, f"edge sequence {i} ({r.shape[0]} rows at {seqs[i][1]} fps)")


# ---- the row stride ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ldp", [66, 72, 156])
def test_the_stride_and_poison_in_the_unused_columns(skel, clean, ldp):
    seqs = []
    for t in TAGS:
        p = np.full((POSES[t].shape[0], ldp), np.nan)
        p[:, :66] = POSES[t][:, :66]
        seqs.append((p, FPS[t], TRANS[t]))
    for t, q in zip(TAGS, _run(seqs, skel)):
        assert _same(q, clean[t]), (t, ldp)


# ---- non-finite input ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["root", "joint", "trans", "inf"])
def test_a_nan_in_the_source_stays_in_the_rows_that_read_it(edge_batch, where):
    """One non-finite value in frame 9 of the 120 fps sequence: the rows the oracle says read that frame are NaN (in the columns that
    the value feeds), every other row of the batch keeps its bits."""
    tile, seqs, refs = edge_batch
    base = _run(seqs)
    p, fps, tr = seqs[2]
    p, tr = p.copy(), tr.copy()
    if where == "root":
        p[9, 1] = np.nan
    elif where == "joint":
        p[9, 3 * 13 + 2] = np.nan                                         # lclavicle
    elif where == "trans":
        tr[9, 0] = np.nan
    else:
        tr[9, 2] = np.inf
    ref = mo.qdq_from_smpl(p, fps, tr)
    hit = mo.rows_reading(p.shape[0], fps, 9, root=where != "joint")
    assert sorted(set(np.nonzero(np.isnan(ref))[0].tolist())) == hit and 1 <= len(hit) <= 4
    poisoned = list(seqs)
    poisoned[2] = (p, fps, tr)
    got = _run(poisoned)
    _compare(got[2], ref, f"non-finite {where}")
    assert not np.isinf(got[2]).any()
    keep = np.setdiff1d(np.arange(ref.shape[0]), hit)
    assert _same(got[2][keep], base[2][keep])
    for i in (0, 1, 3, 4, 5):
        assert _same(got[i], base[i]), i


# ---- the pipelines: pose files -> combine_motions without leaving the card ----------------------------------------------------------
def _guards(tr, flags, what):
    gap, mar = tr["gap"][2:-2], tr["margin"][2:-2]
    on = flags[2:-2] == 1
    g = float(gap[on].min()) if on.any() else np.inf
    m = float(mar[np.isfinite(mar)].min())
    print(f"{what}: oracle's smallest on-frame argmin gap {g:.2e}, smallest threshold margin {m:.2e}")
    assert g >= GAP_GUARD and m >= MARGIN_GUARD, what


def _combined_close(x, y):
    assert np.array_equal(x.info, y.info) and x.info.shape[0] == 2
    for k in ("IMU", "SUM", "S"):
        a, b = getattr(x, k).cpu().numpy(), getattr(y, k).cpu().numpy()
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), k
        err = float(np.nanmax(np.abs(a - b)))
        print(f"combined {k}: {a.shape}, max difference {err:.2e}")
        assert err < DATA_TOL, k


def test_syn_files_through_combine_motions(skel, tmp_path):
    """Two AMASS-layout files -> syn_files -> combine_motions, against the oracle's qdq through the same synthesize and combiner."""
    paths, qs, scales = [], [], [1.0, 1.7 * 1.05 / 1.6]
    for i, (n, fps) in enumerate(((100, 120.0), (95, 100.0))):
        p, tr = mo.source_motion(n, 70 + i, 156, amp=0.12)                # gentle: accelerations below 16, where a float32 ulp is 1e-6
        tr = np.array([0.0, 0.0, 0.9]) + 0.1 * (tr - tr.mean(0))
        path = tmp_path / f"m{i}_poses.npz"
        np.savez(path, poses=p, trans=tr, mocap_framerate=np.float64(fps))
        paths.append(str(path))
        qs.append(mo.qdq_from_smpl(p, fps, tr))
    assert [q.shape[0] for q in qs] == [50, 56]
    for q, s in zip(qs, scales):
        _, c, trace = so.synthesize({k[len("table/"):]: GOLDEN[k] for k in GOLDEN.files if k.startswith("table/")}, q, s)
        _guards(trace, c[:, 0::4], "syn_files")
    dev = motion.syn_files(skel, paths, scales)
    ref = syn.synthesize(skel, qs, scales)
    for d, r, q in zip(dev, ref, qs):
        assert d["nimble_qdq"].is_cuda and float((d["nimble_qdq"].cpu() - torch.from_numpy(q)).abs().max()) <= BOUND
        assert float((d["imu"] - r["imu"]).abs().max()) <= BOUND and float((d["constrs"] - r["constrs"]).abs().max()) <= BOUND
        assert torch.equal(d["constrs"][:, 0::4], r["constrs"][:, 0::4])
    bias = np.linspace(-0.1, 0.1, 36).reshape(2, 18)
    _combined_close(data.combine_motions(dev, [1, 2], biases=bias), data.combine_motions(ref, [1, 2], biases=bias))


def test_real_files_through_combine_motions(tmp_path):
    """A DIP-IMU pickle (readings and poses in one file, no trans) and a TotalCapture pair (poses .npz, readings .pkl) -> real_files ->
    combine_motions, against real_imu_frames with the oracle's qdq through the same combiner."""
    rng = np.random.RandomState(5)
    p0, _ = mo.source_motion(60, 80, 72, with_trans=False, amp=0.3)
    ori0, acc0 = rng.randn(60, 17, 3, 3), rng.randn(60, 17, 3)
    with open(tmp_path / "dip.pkl", "wb") as f:
        pickle.dump({"gt": p0, "imu_ori": ori0, "imu_acc": acc0}, f, protocol=2)
    dip = motion.real_files([str(tmp_path / "dip.pkl")], [str(tmp_path / "dip.pkl")], sensors.ROT_DIP, sensors.SEL_DIP17)
    p1, t1 = mo.source_motion(55, 81, 72, amp=0.3)
    ori1, acc1 = rng.randn(55, 6, 3, 3), rng.randn(55, 6, 3)
    np.savez(tmp_path / "tc_poses.npz", poses=p1, trans=t1, frame_rate=np.float64(60.0))
    with open(tmp_path / "tc.pkl", "wb") as f:
        pickle.dump({"ori": ori1, "acc": acc1}, f, protocol=2)
    tc = motion.real_files([str(tmp_path / "tc_poses.npz")], [str(tmp_path / "tc.pkl")], sensors.ROT_TC, sensors.SEL_TC6)
    dev = dip + tc
    refs = [{"imu": sensors.real_imu_frames([ori0], [acc0], sensors.ROT_DIP, sensors.SEL_DIP17)[0], "nimble_qdq": mo.qdq_from_smpl(p0, 60.0, None)},
            {"imu": sensors.real_imu_frames([ori1], [acc1], sensors.ROT_TC, sensors.SEL_TC6)[0], "nimble_qdq": mo.qdq_from_smpl(p1, 60.0, t1)}]
    for d, r in zip(dev, refs):
        assert set(d) == {"imu", "nimble_qdq"} and d["imu"].is_cuda and d["nimble_qdq"].is_cuda and d["nimble_qdq"].dtype == torch.float64
        assert torch.equal(d["imu"], r["imu"]) and tuple(d["imu"].shape) == (d["nimble_qdq"].shape[0] + 1, 72)
        assert float((d["nimble_qdq"].cpu() - torch.from_numpy(r["nimble_qdq"])).abs().max()) <= BOUND
        d["constrs"] = r["constrs"] = np.zeros((d["imu"].shape[0], 20))     # the reference adds DIP's SBP labels from another directory
    bias = np.linspace(-0.1, 0.1, 36).reshape(2, 18)
    _combined_close(data.combine_motions(dev, [1, 1], augmented_dip=[True, False], biases=bias),
                    data.combine_motions(refs, [1, 1], augmented_dip=[True, False], biases=bias))
