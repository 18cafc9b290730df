"""The timestamped-packet resampler without a GPU: the C-ABI surface of tip_resample_* and its refusals before any launch, the oracle's
fp64 interpolation (tests/resample_oracle.py) against scipy's Slerp and the global-frame lerp, the oracle's push / emit / rows rules
against each other, every refusal of the Python layer, and tick_times.

No fixture from the reference is needed: the reference has no resampling, and its one rule — the demo's zero-order hold,
live_demo_new.py:82-115 / :161-162 — is restated by numpy indexing in test_hold_is_the_demos_rule."""
import ctypes
import fnmatch
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation, Slerp

import resample_oracle as ro
from tip_amd import lib as tlib
from tip_amd import sensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tip_resample_tile": 1, "tip_resample_state_bytes": 3, "tip_resample_reset": 6, "tip_resample_push": 8, "tip_resample_emit": 10,
         "tip_resample_get": 7, "tip_resample_rows": 15}      # name: number of arguments
f32 = np.float32


def test_c_abi_surface_and_refusals_before_any_launch():
    """Every tip_resample_* name is declared in the header under "timestamped packets", matched by the export map, exported by the
    library and bound in lib.py; the ABI is still 5; every refusal returns before a launch (this machine has no GPU to launch on)."""
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert set(re.findall(r"TIP_API int (tip_resample_\w+)\(", hdr)) == set(NAMES) == {n for n in tlib.EXPORTS if n.startswith("tip_resample_")}
    section = hdr[hdr.index("/* ---- timestamped packets"):hdr.index("/* ---- kinematics:")]
    assert all(section.count(name + "(") >= 1 for name in NAMES)
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5 and tlib.TIP_ABI_VERSION == 5
    assert int(re.search(r"#define TIP_RESAMPLE_HOLD\s+(\d+)", hdr).group(1)) == tlib.TIP_RESAMPLE_HOLD == ro.HOLD == 0
    assert int(re.search(r"#define TIP_RESAMPLE_SLERP\s+(\d+)", hdr).group(1)) == tlib.TIP_RESAMPLE_SLERP == ro.SLERP == 1
    the_map = open(os.path.join(tlib.CSRC, "tip_exports.map")).read()
    globs = re.search(r"global:(.*?);", re.sub(r"/\*.*?\*/", "", the_map, flags=re.S), re.S).group(1).split()
    raw = ctypes.CDLL(tlib.LIB_PATH)
    lib = tlib.load()
    for name, nargs in NAMES.items():
        m = re.search(r"TIP_API int " + name + r"\((.*?)\);", hdr, re.S)
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == nargs, name
        assert any(fnmatch.fnmatchcase(name, g) for g in globs) and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is lib.tip_forward.restype, name
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(tlib.CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "tip_resample.hip" in srcs
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)        # a non-null, 8-byte aligned pointer: every call below returns before it would launch
    INV = -1
    rows = ctypes.c_int()
    assert lib.tip_resample_tile(ctypes.byref(rows)) == 0 and rows.value >= 1 and lib.tip_resample_tile(None) == INV
    n, one = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.tip_resample_state_bytes(3, 8, ctypes.byref(n)) == 0 and lib.tip_resample_state_bytes(1, 8, ctypes.byref(one)) == 0
    assert n.value == 3 * one.value and one.value >= 8 * (42 * 4 + 8) + 12 and one.value % 8 == 0
    for depth in (1, 65, -1, 0):
        assert lib.tip_resample_state_bytes(3, depth, ctypes.byref(n)) == INV, depth
    assert lib.tip_resample_state_bytes(-1, 8, ctypes.byref(n)) == INV and lib.tip_resample_state_bytes(3, 8, None) == INV
    assert lib.tip_resample_state_bytes(0, 2, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.tip_resample_state_bytes(1, 64, ctypes.byref(n)) == 0
    # tip_resample_reset(state, n, depth, slots | null, count, stream)
    assert lib.tip_resample_reset(None, 4, 8, None, 0, None) == INV and lib.tip_resample_reset(p + 4, 4, 8, None, 0, None) == INV
    assert lib.tip_resample_reset(p, -1, 8, None, 0, None) == INV and lib.tip_resample_reset(p, 4, 1, None, 0, None) == INV
    assert lib.tip_resample_reset(p, 4, 8, p, -1, None) == INV
    assert lib.tip_resample_reset(p, 0, 8, None, 0, None) == 0 and lib.tip_resample_reset(p, 4, 8, p, 0, None) == 0
    # tip_resample_push(state, n, depth, packets, slots, times, m, stream)
    ok = [p, 4, 8, p, p, p, 2, None]
    for i in (0, 3, 4, 5):
        a = list(ok)
        a[i] = None
        assert lib.tip_resample_push(*a) == INV, i
    for i, v in ((0, p + 4), (1, -1), (2, 65), (2, 1), (6, -1)):
        a = list(ok)
        a[i] = v
        assert lib.tip_resample_push(*a) == INV, (i, v)
    assert lib.tip_resample_push(p, 4, 8, None, None, None, 0, None) == 0 and lib.tip_resample_push(p, 0, 8, p, p, p, 2, None) == 0
    # tip_resample_emit(state, n, depth, t, delay, max_hold, mode, packets_out, flags, stream)
    ok = [p, 4, 8, p, 0.01, -1.0, 1, p, p, None]
    for i in (0, 3, 7, 8):
        a = list(ok)
        a[i] = None
        assert lib.tip_resample_emit(*a) == INV, i
    for i, v in ((0, p + 4), (1, -1), (2, 0), (4, -0.01), (4, float("nan")), (4, float("inf")), (5, float("nan")), (6, 2), (6, -1)):
        a = list(ok)
        a[i] = v
        assert lib.tip_resample_emit(*a) == INV, (i, v)
    assert lib.tip_resample_emit(p, 0, 8, p, 0.0, 0.5, 0, p, p, None) == 0
    # tip_resample_get(state, n, depth, slots, count, counts_out, stream)
    assert lib.tip_resample_get(None, 4, 8, p, 1, p, None) == INV and lib.tip_resample_get(p, 4, 8, None, 1, p, None) == INV
    assert lib.tip_resample_get(p, 4, 8, p, 1, None, None) == INV and lib.tip_resample_get(p, 4, 8, p, -1, p, None) == INV
    assert lib.tip_resample_get(p, 4, 99, p, 1, p, None) == INV and lib.tip_resample_get(p, 4, 8, None, 0, None, None) == 0
    # tip_resample_rows(packets, stamps, in_offsets, n_in, t_out, out_offsets, n_out, n_seq, delay, max_hold, mode, depth, out, flags, stream)
    ok = [p, p, p, 4, p, p, 3, 1, 0.01, -1.0, 1, 8, p, p, None]
    for i in (0, 1, 2, 4, 5, 12, 13):
        a = list(ok)
        a[i] = None
        assert lib.tip_resample_rows(*a) == INV, i
    for i, v in ((3, -1), (6, -1), (7, -1), (8, -1.0), (8, float("inf")), (9, float("nan")), (10, 3), (11, 1), (11, 65)):
        a = list(ok)
        a[i] = v
        assert lib.tip_resample_rows(*a) == INV, (i, v)
    a = list(ok)
    a[6] = 0
    assert lib.tip_resample_rows(*a) == 0


# ---- the interpolation -----------------------------------------------------------------------------------------------------------------
def _pairs(rng, N):
    """N sensor pairs [N, 7]: relative rotations 1e-7 .. 3.0 rad (log-uniform), either quaternion sign, norms 0.5 .. 2."""
    Ra = Rotation.random(N, random_state=rng)
    axis = rng.normal(size=(N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = np.exp(rng.uniform(np.log(1e-7), np.log(3.0), size=N))
    Rb = Ra * Rotation.from_rotvec(axis * angle[:, None])
    out = []
    for R in (Ra, Rb):
        q = R.as_quat() * rng.uniform(0.5, 2.0, size=(N, 1)) * rng.choice([-1.0, 1.0], size=(N, 1))
        out.append(np.concatenate((q, rng.normal(0.0, 3.0, size=(N, 3))), axis=1).astype(f32))
    return out[0], out[1], angle


def test_oracle_interpolation_is_slerp_and_a_global_frame_lerp():
    """20 000 random pairs in fp64: the rotation of the output quaternion against scipy's Slerp between the two packets' rotations (as
    matrices: the sign is free) within 1e-9 — the linear weights above 1 - 1e-6 cost 8.1e-11 here, the slerp branch 8e-16 — and the
    acceleration against R(u)^T ((1 - u) Ra a + u Rb b) within 1e-9 of the global vector's length (the rotation's error times what it
    turns).  The output quaternion is unit and keeps the earlier packet's sign."""
    rng = np.random.RandomState(5)
    N = 20000
    a, b, angle = _pairs(rng, N)
    u = rng.uniform(0.0, 1.0, size=N)
    u[:50] = 0.0
    got = ro.interp(a, b, u, np.float64)
    assert np.isfinite(got).all() and got.dtype == np.float64
    Ra, Rb = Rotation.from_quat(a[:, :4].astype(np.float64)), Rotation.from_quat(b[:, :4].astype(np.float64))
    ref = np.empty((N, 3, 3))
    for i in range(N):
        ref[i] = Slerp([0.0, 1.0], Rotation.concatenate([Ra[i], Rb[i]]))(u[i]).as_matrix()
    R_got = Rotation.from_quat(got[:, :4]).as_matrix()
    err = np.abs(R_got - ref).max(axis=(1, 2))
    small = angle < np.arccos(1 - 1e-6) * 2        # (quaternion dot above the switch: half the rotation angle below acos(1 - 1e-6))
    print(f"max |R - Slerp| {err.max():.3e} (linear branch: {int(small.sum())} pairs, {err[small].max():.3e}; slerp branch {err[~small].max():.3e})")
    assert small.sum() > 1000 and (~small).sum() > 1000
    assert err.max() <= 1e-9
    g = (1.0 - u)[:, None] * Ra.apply(a[:, 4:].astype(np.float64)) + u[:, None] * Rb.apply(b[:, 4:].astype(np.float64))
    a_ref = np.einsum("nji,nj->ni", ref, g)
    a_err = np.abs(got[:, 4:] - a_ref).max(axis=1) / np.maximum(1.0, np.linalg.norm(g, axis=1))
    print(f"max |a - lerp| / max(1, |g|) {a_err.max():.3e}")
    assert a_err.max() <= 1e-9
    assert np.abs(np.linalg.norm(got[:, :4], axis=1) - 1.0).max() <= 1e-15
    qa = a[:, :4].astype(np.float64)
    assert (np.einsum("ni,ni->n", got[:, :4], qa) > 0).all()
    # u = 0 gives the earlier packet's rotation and its own acceleration back
    assert np.abs(R_got[:50] - Ra[:50].as_matrix()).max() <= 1e-15 and np.abs(got[:50, 4:] - a[:50, 4:]).max() <= 1e-14


def test_oracle_float32_follows_the_same_formula():
    """The float32 evaluation is the same restatement: fp32 throughout (weights rounded once), within fp32 noise of the fp64 one, and a
    bad quaternion on either side, or a NaN acceleration, spoils exactly the stated columns."""
    rng = np.random.RandomState(6)
    a, b, _ = _pairs(rng, 4000)
    u = rng.uniform(0.0, 1.0, size=4000)
    lo, hi = ro.interp(a, b, u, f32), ro.interp(a, b, u, np.float64)
    assert lo.dtype == f32
    dR = np.abs(Rotation.from_quat(lo[:, :4].astype(np.float64)).as_matrix() - Rotation.from_quat(hi[:, :4]).as_matrix()).max()
    print(f"fp32 - fp64: rotation entries {dR:.3e}, accelerations {np.abs(lo[:, 4:] - hi[:, 4:]).max():.3e}")
    assert dR < 2e-6 and np.abs(lo[:, 4:] - hi[:, 4:]).max() < 2e-5
    bad_a, bad_b = a[:8].copy(), b[:8].copy()
    bad_a[0, :4] = 0.0
    bad_b[1, 2] = np.nan
    bad_a[2, 0] = np.inf
    bad_a[3, 5] = np.nan
    bad_b[4, 6] = np.nan
    for dtype in (f32, np.float64):
        got = ro.interp(bad_a, bad_b, u[:8], dtype)
        assert np.isnan(got[:3]).all() and np.isfinite(got[5:]).all()
        assert np.isfinite(got[3:5, :4]).all() and np.isnan(got[3:5, 4:]).all()


# ---- the rules -------------------------------------------------------------------------------------------------------------------------
def test_push_rule_and_counters():
    rng = np.random.RandomState(1)
    r = ro.Rings(3, depth=4)
    pk = rng.normal(size=(12, 42)).astype(f32)
    pk[5, 3] = np.nan                                             # NaNs are appended as they are
    slots = [0, 1, 0, 7, 0, 1, 0, -1, 0, 0, 1, 0]
    times = [1.0, 5.0, 2.0, 9.0, 2.0, 6.0, 1.5, 3.0, np.nan, 3.0, np.inf, 4.0]
    r.push(pk, slots, times)
    have, dropped, total = r.counts()
    assert list(have) == [4, 2, 0] and list(dropped) == [3, 1, 0] and list(total) == [4, 2, 0]
    assert r.stamps[0] == [1.0, 2.0, 3.0, 4.0] and r.stamps[1] == [5.0, 6.0]
    assert np.array_equal(np.stack(r.packets[0]), pk[[0, 2, 9, 11]]) and np.isnan(r.packets[1][1][3])
    r.push(pk[:2], [0, 0], [4.0, 4.5])                            # a duplicate of the newest is dropped; a full ring loses its oldest
    assert r.stamps[0] == [2.0, 3.0, 4.0, 4.5] and r.counts()[1][0] == 4 and r.counts()[2][0] == 5
    r.reset([0])
    assert r.stamps[0] == [] and [int(c[0]) for c in r.counts()] == [0, 0, 0] and r.stamps[1] == [5.0, 6.0]


def test_emit_rule_table():
    s = [1.0, 2.0, 2.5, 4.0]
    D = ro.decide
    assert D([], 3.0, None, ro.SLERP)[0] == ro.F_EMPTY
    assert D(s, 0.5, None, ro.SLERP)[0] == ro.F_EARLY and D(s, float("nan"), None, ro.HOLD)[0] == ro.F_EARLY
    assert D(s, 4.0, None, ro.SLERP) == (ro.F_HELD, 3, 0.0) and D(s, 9.0, None, ro.SLERP) == (ro.F_HELD, 3, 0.0)
    assert D(s, 4.5, 0.5, ro.SLERP) == (ro.F_HELD, 3, 0.0) and D(s, 4.6, 0.5, ro.SLERP)[0] == ro.F_STALE
    assert D(s, 2.25, None, ro.HOLD) == (ro.F_HELD, 1, 0.0) and D(s, 1.75, 0.5, ro.HOLD)[0] == ro.F_STALE
    assert D(s, 2.25, None, ro.SLERP) == (ro.F_INTERP, 1, 0.5) and D(s, 2.0, None, ro.SLERP) == (ro.F_INTERP, 1, 0.0)
    assert D(s, 3.0, 1.0, ro.SLERP) == (ro.F_HELD, 2, 0.0)        # a bracket of 1.5 s > max_hold: held while young enough ...
    assert D(s, 3.75, 1.0, ro.SLERP)[0] == ro.F_STALE             # ... then nothing
    assert D(s, 3.0, 1.5, ro.SLERP) == (ro.F_INTERP, 2, 0.5 / 1.5)


def test_rows_is_the_live_ring_at_every_tick():
    """The oracle's offline form against its live form: everything stamped up to the tick pushed before it, depth 4, a wrap."""
    rng = np.random.RandomState(2)
    L = 60
    pk, st = ro.motion_packets(rng, L), ro.stamps_at(rng, L, 100.0, t0=10.0)
    ticks = sensors.tick_times(10.005, 30)
    for mode, delay, hold in ((ro.SLERP, 0.012, None), (ro.SLERP, 0.012, 0.011), (ro.HOLD, 0.0, None)):
        off, off_f = ro.rows(pk, st, ticks, delay, hold, mode, depth=4)
        r, at = ro.Rings(1, 4), 0
        for k, t in enumerate(ticks):
            new = int(np.searchsorted(st, t, side="right"))
            r.push(pk[at:new], [0] * (new - at), st[at:new])
            at = new
            row, f = r.emit(t, delay, hold, mode)
            assert f[0] == off_f[k] and np.array_equal(row[0].view(np.int32), off[k].view(np.int32)), (mode, k)
        seen = set(int(f) for f in off_f)
        assert seen == {ro.F_HELD} if mode == ro.HOLD else ro.F_INTERP in seen, seen
        assert hold is None or seen & {ro.F_HELD, ro.F_STALE}, seen      # (brackets longer than max_hold are not interpolated)


def test_hold_is_the_demos_rule():
    """Mode HOLD with delay 0 and no limit is the demo's: whatever packet is the newest at the tick (numpy indexing)."""
    rng = np.random.RandomState(3)
    pk, st = ro.motion_packets(rng, 50), ro.stamps_at(rng, 50, 59.94, t0=0.0)
    ticks = sensors.tick_times(0.1, 40)
    got, flags = ro.rows(pk, st, ticks, 0.0, None, ro.HOLD, depth=64)
    idx = ro.newest_not_after(pk, st, ticks)
    assert (idx >= 0).all() and (flags == ro.F_HELD).all() and np.array_equal(got, pk[idx])


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_tick_times():
    t = sensors.tick_times(1.7e9, 1000)
    assert t.dtype == np.float64 and t.shape == (1000,) and t[0] == 1.7e9
    assert all(t[k] == 1.7e9 + k * (1.0 / 60.0) for k in (1, 7, 999))         # a product, not a running sum
    assert np.array_equal(sensors.tick_times(0.5, 4, 50), 0.5 + np.arange(4) * (1.0 / 50))
    assert sensors.tick_times(0.0, 0).shape == (0,)
    for bad in ((0.0, -1), (0.0, 2.5), (0.0, True), (float("nan"), 3)):
        with pytest.raises(ValueError, match="tick_times"):
            sensors.tick_times(*bad)
    for rate in (0.0, -60.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="rate_hz"):
            sensors.tick_times(0.0, 3, rate)
    st = np.array([2.0, 2.01, 2.02, 2.105])
    assert np.array_equal(sensors.sequence_ticks(st, 60.0, 0.01), sensors.tick_times(2.0 + 0.01, 7))    # 6 / 60 <= 0.105 < 7 / 60
    assert sensors.sequence_ticks(st, 60.0, 0.0, t_start=3.0).shape == (0,) and sensors.sequence_ticks([], 60.0).shape == (0,)


def test_times_are_float64_whatever_they_come_as():
    """Stamps and query times that are no tensor are read as float64: torch reads a list of Python floats as float32, in which two
    epoch-sized stamps 10 ms apart are the same number.  A float32 tensor or array has lost them already and is refused."""
    import torch
    a, b = 1.7e9 + 0.123, 1.7e9 + 0.133
    assert torch.as_tensor([a, b]).dtype == torch.float32                     # (what the conversion is there for)
    for given in ([a, b], (a, b), np.array([a, b]), torch.tensor([a, b], dtype=torch.float64)):
        t = sensors._times_f64(given, "x")
        assert t.dtype == torch.float64 and t.tolist() == [a, b]
    assert sensors._times_f64(a, "x").shape == () and float(sensors._times_f64(np.array(a), "x")) == a
    assert sensors._times_f64([1, 2], "x").tolist() == [1.0, 2.0] and sensors._times_f64(torch.tensor([1, 2]), "x").dtype == torch.float64
    assert sensors._times_f64([], "x").shape == (0,)
    for bad in (torch.tensor([a, b], dtype=torch.float32), np.array([a, b], dtype=np.float32), np.float32(1.0), torch.tensor([True])):
        with pytest.raises(ValueError, match="x are float64 seconds"):
            sensors._times_f64(bad, "x")
    with pytest.raises(ValueError, match="x are seconds"):
        sensors._times_f64(["a"], "x")


def test_sequence_ticks_checks_its_arguments():
    st = np.array([2.0, 2.01, 2.02, 2.105])
    for kw, what in (({"rate_hz": 0.0}, "rate_hz is"), ({"rate_hz": float("nan")}, "rate_hz is"), ({"delay": float("nan")}, "delay is"),
                     ({"delay": -0.01}, "delay is"), ({"delay": float("inf")}, "delay is"), ({"t_start": float("nan")}, "are finite")):
        with pytest.raises(ValueError, match="sequence_ticks: .*" + what):
            sensors.sequence_ticks(st, **kw)
    with pytest.raises(ValueError, match=r"sequence_ticks: times is \[L\]"):
        sensors.sequence_ticks(st.reshape(2, 2))
    with pytest.raises(ValueError, match="are finite"):
        sensors.sequence_ticks([0.0, float("inf")])
    assert len(sensors.sequence_ticks(st.tolist(), 60, 0)) == 7


def test_python_refusals_before_any_launch():
    """Every argument check of PacketResampler and resample_sequences comes before a device is chosen: on a machine without a GPU each
    is a ValueError in the caller's name, and only a good set of arguments gets as far as asking for the device."""
    P = sensors.PacketResampler
    for kw, what in (({"mode": "linear"}, "mode is"), ({"mode": 1}, "mode is"), ({"delay": -0.01}, "delay is"),
                     ({"delay": float("nan")}, "delay is"), ({"delay": float("inf")}, "delay is"), ({"delay": "x"}, "delay is"),
                     ({"max_hold": -1.0}, "max_hold is"), ({"max_hold": float("nan")}, "max_hold is"), ({"depth": 1}, "depth is"),
                     ({"depth": 65}, "depth is"), ({"depth": 8.0}, "depth is"), ({"depth": True}, "depth is")):
        with pytest.raises(ValueError, match="PacketResampler: " + what):
            P(2, "cpu", **kw)
    for n in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="n is the number of slots"):
            P(n, "cpu")
    with pytest.raises(RuntimeError, match="runs on an MI355X"):
        P(2, "cpu", mode="hold", delay=0.0, max_hold=0.5, depth=64)
    pk = np.zeros((5, 42), f32)
    t = np.arange(5) * 0.01
    R = sensors.resample_sequences
    for kw, what in (({"mode": "nearest"}, "mode is"), ({"delay": -1.0}, "delay is"), ({"max_hold": float("nan")}, "max_hold is"),
                     ({"depth": 0}, "depth is"), ({"rate_hz": 0.0}, "rate_hz is"), ({"t_start": [0.0, 1.0, 2.0]}, "t_start is")):
        with pytest.raises(ValueError, match="resample_sequences: " + what):
            R([pk, pk], [t, t], **kw)
    with pytest.raises(ValueError, match="no sequences"):
        R([], [])
    with pytest.raises(ValueError, match=r"packets_list\[1\] is \[L, 42\]"):
        R([pk, pk[:, :41]], [t, t])
    with pytest.raises(ValueError, match="2 packet arrays for 1 time arrays"):
        R([pk, pk], [t])
    with pytest.raises(ValueError, match=r"times_list\[1\] is \[5\]"):
        R([pk, pk], [t, t[:4]])
    bad = t.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match=r"times_list\[1\] row 3 is not finite"):
        R([pk, pk], [t, bad])
    bad = t.copy()
    bad[2] = bad[1]
    with pytest.raises(ValueError, match=r"times_list\[0\] row 2 is not after row 1"):
        R([pk, pk], [bad, t])
    bad = t.copy()
    bad[4] = 0.005
    with pytest.raises(ValueError, match=r"times_list\[1\] row 4 is not after row 3"):
        R([pk, pk], [t, bad])
