"""Gap filling without a GPU: the C-ABI surface of tip_fill_*, the oracle (tests/sensor_fill_oracle.py) against the reference's own
output (tests/golden/tip_fill_golden.npz, made by tests/golden/make_fill_golden.py), rule V against rule R, the TotalCapture selection
and the branches the fixture reaches."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import sensor_fill_oracle as fo
from tip_amd import lib as tlib
from tip_amd import sensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tip_fill_real": 11, "tip_fill_rows": 8, "tip_fill_state_bytes": 2, "tip_fill_reset": 5, "tip_fill_live": 7, "tip_fill_get": 6,
         "tip_fill_packets": 8}      # name: number of arguments


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "tip_fill_golden.npz"))


def test_c_abi_surface():
    """Every tip_fill_* name is declared in the header, exported by the library and bound in lib.py; the ABI is still 5; the argument
    checks that run before any launch."""
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert set(re.findall(r"TIP_API int (tip_fill_\w+)\(", hdr)) == set(NAMES)
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5 and tlib.TIP_ABI_VERSION == 5
    raw = ctypes.CDLL(tlib.LIB_PATH)
    lib = tlib.load()
    for name, nargs in NAMES.items():
        m = re.search(r"TIP_API int " + name + r"\((.*?)\);", hdr, re.S)
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == nargs, name
        assert name in tlib.EXPORTS and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is lib.tip_forward.restype, name
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)        # a non-null pointer: every call below returns before it would launch
    sel, rot = (ctypes.c_int * 6)(2, 7, 8, 11, 12, 0), (ctypes.c_double * 9)(*sensors.ROT_DIP.reshape(-1))
    INV = -1
    n = ctypes.c_size_t()
    assert lib.tip_fill_state_bytes(3, ctypes.byref(n)) == 0 and n.value >= 3 * (5 * 72 * 4 + 3 * 12 * 4) and n.value % 4 == 0
    one = ctypes.c_size_t()
    assert lib.tip_fill_state_bytes(1, ctypes.byref(one)) == 0 and n.value == 3 * one.value
    assert lib.tip_fill_state_bytes(-1, ctypes.byref(n)) == INV and lib.tip_fill_state_bytes(3, None) == INV
    assert lib.tip_fill_state_bytes(0, ctypes.byref(n)) == 0 and n.value == 0
    # tip_fill_real(ori, acc, n_rows, n_sensors, offsets, n_seq, sel, rot, out, unfilled, stream)
    ok = [p, p, 4, 17, p, 1, sel, rot, p, p, None]
    for i in (0, 1, 4, 6, 7, 8, 9):
        a = list(ok)
        a[i] = None
        assert lib.tip_fill_real(*a) == INV, i
    assert lib.tip_fill_real(p, p, -1, 17, p, 1, sel, rot, p, p, None) == INV and lib.tip_fill_real(p, p, 4, 0, p, 1, sel, rot, p, p, None) == INV
    assert lib.tip_fill_real(p, p, 4, 17, p, -1, sel, rot, p, p, None) == INV
    assert lib.tip_fill_real(p, p, 4, 6, p, 1, sel, rot, p, p, None) == INV                 # sel names sensor 12 of 6
    assert lib.tip_fill_real(p, p, 4, 17, p, 0, sel, rot, p, p, None) == 0
    # tip_fill_rows(frames, out, n_rows, offsets, n_seq, max_gap, flags, stream)
    ok = [p, p, 4, p, 1, -1, p, None]
    for i in (0, 1, 3, 6):
        a = list(ok)
        a[i] = None
        assert lib.tip_fill_rows(*a) == INV, i
    assert lib.tip_fill_rows(p, p, -1, p, 1, -1, p, None) == INV and lib.tip_fill_rows(p, p, 4, p, -1, -1, p, None) == INV
    assert lib.tip_fill_rows(p, p, 4, p, 1, -2, p, None) == INV
    assert lib.tip_fill_rows(p, p, 4, p, 0, -1, p, None) == 0 and lib.tip_fill_rows(p, p, 0, p, 1, 3, p, None) == 0
    # tip_fill_reset(state, n, slots | null, count, stream)
    assert lib.tip_fill_reset(None, 4, None, 0, None) == INV and lib.tip_fill_reset(p, -1, None, 0, None) == INV
    assert lib.tip_fill_reset(p, 4, p, -1, None) == INV
    assert lib.tip_fill_reset(p, 0, None, 0, None) == 0 and lib.tip_fill_reset(p, 4, p, 0, None) == 0
    # tip_fill_live(state, cal, raw, n, max_gap, flags, stream)
    ok = [p, p, p, 4, -1, p, None]
    for i in (0, 1, 2, 5):
        a = list(ok)
        a[i] = None
        assert lib.tip_fill_live(*a) == INV, i
    assert lib.tip_fill_live(p, p, p, -1, -1, p, None) == INV and lib.tip_fill_live(p, p, p, 4, -2, p, None) == INV
    assert lib.tip_fill_live(p, p, p, 0, -1, p, None) == 0
    # tip_fill_get(state, n, slots, count, counts_out, stream)
    assert lib.tip_fill_get(None, 4, p, 1, p, None) == INV and lib.tip_fill_get(p, 4, None, 1, p, None) == INV
    assert lib.tip_fill_get(p, 4, p, 1, None, None) == INV and lib.tip_fill_get(p, 4, p, -1, p, None) == INV
    assert lib.tip_fill_get(p, -1, p, 1, p, None) == INV and lib.tip_fill_get(p, 4, None, 0, None, None) == 0
    # tip_fill_packets(tables, packets, n_rows, offsets, n_seq, max_acc, out, stream)
    ok = [p, p, 4, p, 1, 10.0, p, None]
    for i in (0, 1, 3, 6):
        a = list(ok)
        a[i] = None
        assert lib.tip_fill_packets(*a) == INV, i
    assert lib.tip_fill_packets(p, p, -1, p, 1, 10.0, p, None) == INV and lib.tip_fill_packets(p, p, 4, p, -1, 10.0, p, None) == INV
    assert lib.tip_fill_packets(p, p, 4, p, 1, -1.0, p, None) == INV and lib.tip_fill_packets(p, p, 4, p, 1, float("nan"), p, None) == INV
    assert lib.tip_fill_packets(p, p, 4, p, 0, 10.0, p, None) == 0 and lib.tip_fill_packets(p, p, 0, p, 1, 10.0, p, None) == 0


def test_rotations_and_selections_are_the_references():
    """ROT_DIP is Q2R((.5, .5, .5, .5)) in its exact form and ROT_TC is A2R((pi / 2, 0, 0)) as scipy gives it; SEL_TC6 is the reference's
    scatter of TotalCapture's six sensors into 17 slots (preprocess_DIP_TC_new.py:89-90) followed by its selection (:166)."""
    q = Rotation.from_quat([0.5, 0.5, 0.5, 0.5]).as_matrix()
    assert np.abs(sensors.ROT_DIP - q).max() <= 1e-15 and np.array_equal(sensors.ROT_DIP, [[0, 0, 1], [1, 0, 0], [0, 1, 0]])
    assert np.array_equal(sensors.ROT_TC, Rotation.from_rotvec([np.pi / 2, 0, 0]).as_matrix())
    assert sensors.SEL_DIP17 == (2, 7, 8, 11, 12, 0)
    rng = np.random.RandomState(0)
    sub = rng.normal(size=(5, 6, 3))
    full = np.zeros((5, 17, 3))
    full[:, [11, 12, 7, 8, 0, 2]] = sub
    assert np.array_equal(full[:, list(sensors.SEL_DIP17)], sub[:, list(sensors.SEL_TC6)])
    assert sorted(sensors.SEL_TC6) == list(range(6))


def test_oracle_rule_r_equals_the_reference_bit_for_bit(golden):
    for i, L in enumerate(golden["lengths"]):
        ori, acc = golden[f"ori_{i}"], golden[f"acc_{i}"]
        assert ori.shape == (L, 17, 3, 3) and acc.shape == (L, 17, 3) and np.isnan(ori).any() and np.isnan(acc).any()
        for name, rot in (("dip", sensors.ROT_DIP), ("tc", sensors.ROT_TC)):
            out, unfilled = fo.real_frames(ori, acc, rot, sensors.SEL_DIP17)
            ref = golden[f"out_{name}_{i}"]
            assert unfilled == 0 and out.dtype == np.float64 and np.isfinite(ref).all()
            assert np.array_equal(out, ref), (name, L, float(np.abs(out - ref).max()))


def test_fixture_reaches_every_branch(golden):
    counts = dict(zip(golden["branch_names"].tolist(), golden["branch_counts"].tolist()))
    print(counts, golden["filled_parts"].tolist())
    assert set(counts) == {"t_lt_10", "t_eq_10", "t_gt_10", "in_long_run", "one_element", "rotation_only", "acceleration_only"}
    assert all(v >= 3 for v in counts.values()), counts
    assert list(golden["lengths"]) == [12, 37, 120]
    total = sum(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in ("tip_fill_golden.npz",))
    assert total < 500_000


def test_rule_v_equals_rule_r_after_clean_first_rows():
    """In float32, with rows 0 .. 10 good, the live rule gives what the reference's rule gives on every row, bit for bit: runs of up to
    15 bad rows, single-element NaNs, rotation and acceleration apart."""
    rng = np.random.RandomState(7)
    L = 120
    clean = rng.normal(0.0, 2.0, size=(L, 72)).astype(np.float32)
    frames = fo.gap_frames(rng, clean, p_bad=0.08, runs=[(0, 20, 35), (7, 40, 47), (3, 60, 69), (11, 100, 112)])
    frames[:11] = clean[:11]
    live, flags, state = fo.fill_live(frames)
    H_ori = fo.fill_reference(frames[:, :54].reshape(L, 6, 9))
    H_acc = fo.fill_reference(frames[:, 54:].reshape(L, 6, 3))
    ref = np.concatenate((H_ori.reshape(L, 54), H_acc.reshape(L, 18)), axis=1)
    assert ref.dtype == np.float32 and live.dtype == np.float32
    n_filled = int((flags == 1).sum())
    print(f"{n_filled} filled parts, longest run {int(state.total.max())} fills in a part")
    assert n_filled > 100 and (flags != 2).all() and np.isfinite(ref).all()
    assert np.array_equal(live, ref)
    assert np.array_equal(state.total, (flags == 1).sum(axis=0))
    # and where they part: a bad part in the first rows looks ahead under R, and has nothing to look at under V
    frames[0, :9] = np.nan
    live2, flags2, _ = fo.fill_live(frames)
    assert flags2[0, 0] == 2 and np.isnan(live2[0, :9]).all() and np.isfinite(live2[1:]).all()
    assert np.isfinite(fo.fill_reference(frames[:, :54].reshape(L, 6, 9))[0]).all()


def test_rule_v_max_gap_and_counters():
    rng = np.random.RandomState(3)
    frames = rng.normal(size=(12, 72)).astype(np.float32)
    frames[2:8, 54:57] = np.nan
    out, flags, state = fo.fill_live(frames, max_gap=3)
    assert list(flags[:, 6]) == [0, 0, 1, 1, 1, 2, 2, 2, 0, 0, 0, 0]
    assert np.isnan(out[5:8, 54:57]).all() and np.isfinite(out[2:5, 54:57]).all()
    assert out[2, 54] == np.float32(np.float32(frames[0, 54] + frames[1, 54]) / np.float32(2))
    assert state.total[6] == 3 and state.run[6] == 0 and state.have[6] == 5
    out, flags, state = fo.fill_live(frames)
    assert list(flags[:, 6]) == [0, 0, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0] and np.isfinite(out).all()
