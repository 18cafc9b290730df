"""Sensor front end without a GPU: the C-ABI surface of tip_sensor_*, the oracle the GPU tests compare against (tests/sensor_oracle.py:
its vectorised and per-stream forms, its Q2R formula, the aligned T-pose), the host mirror of the calibration phases, and the two
numpy / scipy facts the device rules rest on."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

import sensor_oracle as so
from tip_amd import lib as tlib
from tip_amd import sensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tip_sensor_state_bytes": 2, "tip_sensor_reset": 3, "tip_sensor_begin": 6, "tip_sensor_accumulate": 4, "tip_sensor_finish": 6,
         "tip_sensor_set": 6, "tip_sensor_get": 6, "tip_sensor_transform": 6}      # name: number of arguments


def test_c_abi_surface():
    """Every tip_sensor_* name is declared in the header, exported by the library and bound in lib.py; the ABI is still 5; the
    argument checks that run before any launch."""
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert set(re.findall(r"TIP_API int (tip_sensor_\w+)\(", hdr)) == set(NAMES)
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    assert re.search(r"#define TIP_SENSOR_HEADING 1\b", hdr) and re.search(r"#define TIP_SENSOR_TPOSE\s+2\b", hdr)
    assert (tlib.TIP_SENSOR_HEADING, tlib.TIP_SENSOR_TPOSE) == (1, 2)
    raw = ctypes.CDLL(tlib.LIB_PATH)
    lib = tlib.load()
    for name, nargs in NAMES.items():
        m = re.search(r"TIP_API int " + name + r"\((.*?)\);", hdr, re.S)
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")) == nargs, name
        assert name in tlib.EXPORTS and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is lib.tip_forward.restype, name
    assert lib.tip_abi_version() == 5
    n = ctypes.c_size_t()
    assert lib.tip_sensor_state_bytes(3, ctypes.byref(n)) == 0 and n.value >= 3 * (126 * 4 + 72 * 8 + 8) and n.value % 8 == 0
    one = ctypes.c_size_t()
    assert lib.tip_sensor_state_bytes(1, ctypes.byref(one)) == 0 and n.value == 3 * one.value
    assert lib.tip_sensor_state_bytes(-1, ctypes.byref(n)) == -1 and lib.tip_sensor_state_bytes(3, None) == -1
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)        # a non-null pointer: every call below returns before it would launch
    assert lib.tip_sensor_reset(None, 4, None) == -1 and lib.tip_sensor_reset(p, -1, None) == -1 and lib.tip_sensor_reset(p, 0, None) == 0
    assert lib.tip_sensor_begin(None, 4, p, 1, 1, None) == -1 and lib.tip_sensor_begin(p, 4, None, 1, 1, None) == -1
    assert lib.tip_sensor_begin(p, 4, p, -1, 1, None) == -1 and lib.tip_sensor_begin(p, 4, p, 1, 0, None) == -1
    assert lib.tip_sensor_begin(p, 4, p, 1, 3, None) == -1 and lib.tip_sensor_begin(p, 4, None, 0, 2, None) == 0
    assert lib.tip_sensor_accumulate(None, p, 4, None) == -1 and lib.tip_sensor_accumulate(p, None, 4, None) == -1
    assert lib.tip_sensor_accumulate(p, p, -1, None) == -1 and lib.tip_sensor_accumulate(p, p, 0, None) == 0
    assert lib.tip_sensor_finish(None, 4, p, 1, None, None) == -1 and lib.tip_sensor_finish(p, 4, None, 1, None, None) == -1
    assert lib.tip_sensor_finish(p, 4, p, -1, None, None) == -1 and lib.tip_sensor_finish(p, 4, None, 0, None, None) == 0
    assert lib.tip_sensor_set(p, 4, p, 1, None, None) == -1 and lib.tip_sensor_set(p, 4, None, 1, p, None) == -1
    assert lib.tip_sensor_set(None, 4, p, 1, p, None) == -1 and lib.tip_sensor_set(p, 4, None, 0, None, None) == 0
    assert lib.tip_sensor_get(p, 4, p, 1, None, None) == -1 and lib.tip_sensor_get(None, 4, p, 1, p, None) == -1
    assert lib.tip_sensor_get(p, 4, p, -1, p, None) == -1 and lib.tip_sensor_get(p, 4, None, 0, None, None) == 0
    assert lib.tip_sensor_transform(None, p, 4, 10.0, p, None) == -1 and lib.tip_sensor_transform(p, None, 4, 10.0, p, None) == -1
    assert lib.tip_sensor_transform(p, p, 4, 10.0, None, None) == -1 and lib.tip_sensor_transform(p, p, -1, 10.0, p, None) == -1
    assert lib.tip_sensor_transform(p, p, 4, -1.0, p, None) == -1 and lib.tip_sensor_transform(p, p, 4, float("nan"), p, None) == -1
    assert lib.tip_sensor_transform(p, p, 0, 10.0, p, None) == 0


def test_vectorised_oracle_equals_the_per_stream_one():
    rng = np.random.RandomState(0)
    n, K = 16, 5
    hp, tp = so.hold_packets(rng, K, n, 0.02), so.hold_packets(rng, K, n, 0.5)
    tables = so.calibrate_v(hp, tp)
    pk = so.frame_packets(rng, n)
    frames = so.transform_v(so.read_packet_v(pk), *so.unpack_tables(tables))
    worst_t = worst_f = 0.0
    for i in range(n):
        G, off = so.heading(so.mean_readings([so.read_packet(hp[t, i]) for t in range(K)]))
        B = so.tpose(so.mean_readings([so.read_packet(tp[t, i]) for t in range(K)]), G, so.aligned_t_pose())
        worst_t = max(worst_t, float(np.abs(so.pack_tables(G, off, B) - tables[i]).max()))
        worst_f = max(worst_f, float(np.abs(so.transform(so.read_packet(pk[i]), G, off, B) - frames[i]).max()))
    print(f"vectorised - per stream: tables {worst_t:.2e}, frames {worst_f:.2e}")
    assert worst_t <= 1e-15 and worst_f <= 1e-15
    # the float32 restatement the GPU test takes its noise from really runs in float32, and is close to the fp64 one
    t32 = tables.astype(np.float32)
    f32, f64 = so.frames_from_tables(pk, t32, dtype=np.float32), so.frames_from_tables(pk, t32)
    assert f32.dtype == np.float32 and f64.dtype == np.float64
    assert 0 < np.abs(f32 - f64)[:, :54].max() < 5e-6 and 0 < np.abs(f32 - f64)[:, 54:].max() < 1e-4


def test_q2r_formula_is_scipys_and_reads_xyzw():
    rng = np.random.RandomState(1)
    q = rng.normal(size=(2000, 4)) * rng.uniform(0.3, 3.0, size=(2000, 1))
    assert np.abs(so.q2r_formula(q) - Rotation.from_quat(q).as_matrix()).max() <= 1e-15
    # (x, y, z, w): a quarter turn about z is (0, 0, sin 45, cos 45), and it takes x to y
    s = np.sqrt(0.5)
    assert np.allclose(so.Q2R([0, 0, s, s]) @ [1, 0, 0], [0, 1, 0], atol=1e-15)
    assert np.allclose(so.Q2R([0, 0, 0, 2.0]), np.eye(3), atol=0)            # normalised first


def test_default_t_pose_is_the_demos_product_without_its_residues():
    """live_demo_new.py:52-62: A2R([0, 0, pi / 2]) @ [[1,0,0],[0,0,-1],[0,1,0]] for every sensor.  The device's default is its exact form;
    the fp64 product itself carries residues of cos(pi / 2) (2.2e-16 here)."""
    ref = Rotation.from_rotvec([0, 0, np.pi / 2]).as_matrix() @ np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])
    d = float(np.abs(sensors.ALIGNED_T_POSE - ref).max())
    print(f"|default - product| = {d:.3e}")
    assert 0 < d <= 1e-15
    assert np.array_equal(sensors.ALIGNED_T_POSE, [[0, 0, 1], [1, 0, 0], [0, 1, 0]])
    assert np.abs(so.aligned_t_pose() - ref).max() == 0 and so.aligned_t_pose().shape == (6, 3, 3)


def test_phase_mirror_transitions_and_refusals():
    U, H, HD, T, L = sensors.UNCALIBRATED, sensors.HEADING, sensors.HEADING_DONE, sensors.TPOSE, sensors.LIVE
    assert (U, H, HD, T, L) == (0, 1, 2, 3, 4)
    m = sensors.PhaseMirror(5)
    assert m.phase == [U] * 5 and not m.live().any()
    # every allowed transition: 0 -> 1 -> 2 -> 3 -> 4; 2 -> 1 and 4 -> 1 (heading again); 2 -> 3 after a new heading; load: any -> 4
    m.begin_heading([0, 1, 2])
    assert m.phase == [H, H, H, U, U]
    m.finish([0, 1, 2])
    assert m.phase == [HD, HD, HD, U, U]
    m.begin_heading([2])                       # 2 -> 1
    m.begin_tpose([0, 1])
    assert m.phase == [T, T, H, U, U]
    m.finish([0, 1, 2])                        # 3 -> 4 and 1 -> 2 in one call
    assert m.phase == [L, L, HD, U, U]
    assert list(m.live()) == [True, True, False, False, False] and list(m.live([1, 2])) == [True, False]
    m.begin_heading([0])                       # 4 -> 1: a live slot starts over
    m.finish([0])
    m.begin_tpose([0, 2])                      # the T-pose again after a finished heading
    m.finish([0, 2])
    assert m.phase == [L, L, L, U, U]
    for start in (U, H, HD, T, L):             # load makes any slot live
        m.phase[3] = start
        m.load([3])
        assert m.phase[3] == L
    # refusals: the mirror is left exactly as it was, for every listed slot
    for start in (U, H, T, L):                 # begin_tpose without a finished heading
        m.phase = [HD, start, U, U, U]
        with pytest.raises(RuntimeError, match="SensorFrontEnd.begin_tpose: slot 1 has no finished heading"):
            m.begin_tpose([0, 1])
        assert m.phase == [HD, start, U, U, U]
    for start in (U, HD, L):                   # finish on a slot that is not accumulating
        m.phase = [H, T, start, U, U]
        with pytest.raises(RuntimeError, match="SensorFrontEnd.finish: slot 2 is not accumulating"):
            m.finish([0, 1, 2])
        assert m.phase == [H, T, start, U, U]
    for start in (H, T):                       # begin_heading inside a hold (the device rule allows 0, 2, 4 only)
        m.phase = [U, start, U, U, U]
        with pytest.raises(RuntimeError, match="SensorFrontEnd.begin_heading: slot 1 is in a hold"):
            m.begin_heading([0, 1])
        assert m.phase == [U, start, U, U, U]


def test_np_clip_propagates_nan_and_scipy_refuses_the_zero_quaternion():
    """The two facts the device rules rest on: a NaN acceleration stays NaN through the clip (so must the kernel's), and scipy has no
    rotation for a zero quaternion (it raises; the kernel gives that sensor NaN columns)."""
    c = np.clip(np.array([np.nan, np.inf, -np.inf, 3.0]), -10.0, 10.0)
    assert np.isnan(c[0]) and list(c[1:]) == [10.0, -10.0, 3.0]
    with pytest.raises(ValueError, match="zero norm"):
        Rotation.from_quat([0.0, 0.0, 0.0, 0.0])
    G, off, B = so.unpack_tables(so.case(1, 3)[1].astype(np.float64)[0])
    reading = so.read_packet(so.case(1, 3)[0][0])
    reading[54 + 4] = np.nan                   # sensor 1, y
    out = so.transform(reading, G, off, B)
    assert np.isnan(out[54 + 3: 54 + 6]).all() and np.isfinite(np.delete(out, [57, 58, 59])).all()


def test_case_inputs_reach_both_clip_ends():
    """The GPU transform test's inputs at n = 1024 (24 576 sensor samples): about a fifth of the acceleration outputs sit on the clip,
    at both ends, both signs of w occur, and the quaternions are not unit length."""
    pk, tables = so.case(1024, 1024)
    f = so.frames_from_tables(pk, tables)
    acc = f[:, 54:]
    hi, lo = float((acc == 10.0).mean()), float((acc == -10.0).mean())
    print(f"on the clip: +10 {hi:.3f}, -10 {lo:.3f}")
    assert 0.07 < hi < 0.15 and 0.07 < lo < 0.15 and np.isfinite(f).all()
    q = pk.reshape(-1, 7)[:, :4]
    norm = np.linalg.norm(q, axis=1)
    assert (q[:, 3] > 0).any() and (q[:, 3] < 0).any() and norm.min() < 0.4 and norm.max() > 2.5
    assert (np.abs(pk.reshape(-1, 7)[:, 4:]) == 10.0).sum() > 100
