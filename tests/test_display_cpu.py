"""Display-time poses without a GPU: the C-ABI surface of tip_pose_* and its refusals before any launch, the oracle's fp64 form
(tests/display_oracle.py) against scipy's Slerp inside a bracket and against an analytic constant-rate spin past the newest entry, the
oracle's rules against each other and against the packet side's oracles, every refusal of the Python layer, and pose_time.

The reference has no display-time resampling; what it fixes is the pose's age — IMU_n_smooth = 5 frames (real_time_runner.py:391-393) —
which pose_time restates."""
import ctypes
import fnmatch
import os
import re
import types

import numpy as np
import pytest
import torch
from scipy.spatial.transform import Rotation, Slerp

import display_oracle as do
import resample_oracle as ro
import sync_oracle as so
from tip_amd import display, handover
from tip_amd import lib as tlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tip_pose_tile": 1, "tip_pose_state_bytes": 3, "tip_pose_reset": 6, "tip_pose_get": 7, "tip_pose_push": 11, "tip_pose_emit": 13,
         "tip_pose_rows": 20}      # name: number of arguments
f32 = np.float32


def test_c_abi_surface_and_refusals_before_any_launch():
    """Every tip_pose_* name is declared in the header under "display-time poses", matched by the export map, exported by the library and
    bound in lib.py; the ABI is still 5; every refusal returns before a launch (this machine has no GPU to launch on)."""
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert set(re.findall(r"TIP_API int (tip_pose_\w+)\(", hdr)) == set(NAMES) == {n for n in tlib.EXPORTS if n.startswith("tip_pose_")}
    section = hdr[hdr.index("/* ---- display-time poses"):hdr.index("/* ---- synthetic data")]
    assert all(section.count(name + "(") >= 1 for name in NAMES)
    assert "NO SPAN RULE" in section and "TIP_PREDICT_SPAN" in section
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5 and tlib.TIP_ABI_VERSION == 5
    for name, v in (("HOLD", do.HOLD), ("SLERP", do.SLERP), ("PREDICT", do.PREDICT)):
        assert int(re.search(r"#define TIP_POSE_" + name + r"\s+(\d+)", hdr).group(1)) == getattr(tlib, "TIP_POSE_" + name) == v
    assert float(re.search(r"#define TIP_POSE_ANTIPODAL\s+([\d.e+-]+)f", hdr).group(1)) == tlib.TIP_POSE_ANTIPODAL == do.ANTIPODAL
    the_map = open(os.path.join(tlib.CSRC, "tip_exports.map")).read()
    globs = re.search(r"global:(.*?);", re.sub(r"/\*.*?\*/", "", the_map, flags=re.S), re.S).group(1).split()
    raw = ctypes.CDLL(tlib.LIB_PATH)
    lib = tlib.load()
    for name, nargs in NAMES.items():
        m = re.search(r"TIP_API int " + name + r"\((.*?)\);", hdr, re.S)
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == nargs, name
        assert any(fnmatch.fnmatchcase(name, g) for g in globs) and hasattr(raw, name), name
        assert len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is lib.tip_forward.restype, name
    mk = open(os.path.join(tlib.CSRC, "Makefile")).read()
    assert "tip_display.hip" in re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split() and "-c tip_display.hip" in mk
    assert "-ffp-contract=off" in mk
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)        # a non-null, 8-byte aligned pointer: every call below returns before it would launch
    INV = -1
    tile = ctypes.c_int()
    assert lib.tip_pose_tile(ctypes.byref(tile)) == 0 and tile.value >= 1 and lib.tip_pose_tile(None) == INV
    n, one = ctypes.c_size_t(), ctypes.c_size_t()
    for depth in range(2, 65):       # the host's block size is the library's, odd depths (padded to 8) included
        assert lib.tip_pose_state_bytes(1, depth, ctypes.byref(one)) == 0 and lib.tip_pose_state_bytes(3, depth, ctypes.byref(n)) == 0
        assert one.value == display.block_bytes(depth) == do.block_bytes(depth) and n.value == 3 * one.value and one.value % 8 == 0
        assert 0 <= one.value - (16 + depth * (8 + 57 * 4)) < 8
    for depth in (1, 65, -1, 0):
        assert lib.tip_pose_state_bytes(3, depth, ctypes.byref(n)) == INV, depth
    assert lib.tip_pose_state_bytes(-1, 8, ctypes.byref(n)) == INV and lib.tip_pose_state_bytes(3, 8, None) == INV
    assert lib.tip_pose_state_bytes(0, 2, ctypes.byref(n)) == 0 and n.value == 0
    # tip_pose_reset(state, n, depth, slots | null, count, stream)
    assert lib.tip_pose_reset(None, 4, 8, None, 0, None) == INV and lib.tip_pose_reset(p + 4, 4, 8, None, 0, None) == INV
    assert lib.tip_pose_reset(p, -1, 8, None, 0, None) == INV and lib.tip_pose_reset(p, 4, 1, None, 0, None) == INV
    assert lib.tip_pose_reset(p, 4, 8, p, -1, None) == INV
    assert lib.tip_pose_reset(p, 0, 8, None, 0, None) == 0 and lib.tip_pose_reset(p, 4, 8, p, 0, None) == 0
    # tip_pose_get(state, n, depth, slots, count, counts_out, stream)
    assert lib.tip_pose_get(None, 4, 8, p, 1, p, None) == INV and lib.tip_pose_get(p, 4, 8, None, 1, p, None) == INV
    assert lib.tip_pose_get(p, 4, 8, p, 1, None, None) == INV and lib.tip_pose_get(p, 4, 8, p, -1, p, None) == INV
    assert lib.tip_pose_get(p, 4, 99, p, 1, p, None) == INV and lib.tip_pose_get(p, 4, 8, None, 0, None, None) == 0
    # tip_pose_push(state, n, depth, slots | null, count, root, s_rest, ld, valid | null, t, stream)
    ok = [p, 4, 8, p, 2, p, p, 111, None, p, None]
    for i in (0, 5, 6, 9):
        a = list(ok)
        a[i] = None
        assert lib.tip_pose_push(*a) == INV, i
    for i, v in ((0, p + 4), (1, -1), (2, 65), (2, 1), (4, -1), (7, 53), (7, 0), (9, p + 4)):
        a = list(ok)
        a[i] = v
        assert lib.tip_pose_push(*a) == INV, (i, v)
    assert lib.tip_pose_push(p, 4, 8, p, 0, p, p, 54, None, p, None) == 0 and lib.tip_pose_push(p, 0, 8, None, 0, p, p, 54, p, p, None) == 0
    # tip_pose_emit(state, n, depth, t, delay, max_hold, max_predict, baseline, mode, q_out, quat_out | null, flags, stream)
    ok = [p, 4, 8, p, 0.01, -1.0, 0.15, 1, 2, p, None, p, None]
    for i in (0, 3, 9, 11):
        a = list(ok)
        a[i] = None
        assert lib.tip_pose_emit(*a) == INV, i
    for i, v in ((0, p + 4), (1, -1), (2, 0), (4, -0.01), (4, float("nan")), (4, float("inf")), (5, float("nan")), (6, -0.1),
                 (6, float("nan")), (6, float("inf")), (7, 0), (7, 8), (7, -1), (8, 3), (8, -1)):
        a = list(ok)
        a[i] = v
        assert lib.tip_pose_emit(*a) == INV, (i, v)
    assert lib.tip_pose_emit(p, 0, 8, p, 0.0, 0.5, 0.0, 7, 0, p, p, p, None) == 0
    # tip_pose_rows(stamps, root, rows, ld, in_offsets, n_in, t_out, out_offsets, n_out, n_seq, delay, max_hold, max_predict, baseline,
    #               mode, depth, q_out, quat_out | null, flags, stream)
    ok = [p, p, p, 54, p, 4, p, p, 3, 1, 0.01, -1.0, 0.15, 1, 2, 8, p, None, p, None]
    for i in (0, 1, 2, 4, 6, 7, 16, 18):
        a = list(ok)
        a[i] = None
        assert lib.tip_pose_rows(*a) == INV, i
    for i, v in ((3, 53), (5, -1), (8, -1), (9, -1), (10, -1.0), (10, float("inf")), (11, float("nan")), (12, -1.0), (12, float("nan")),
                 (13, 0), (13, 8), (14, 3), (15, 1), (15, 65)):
        a = list(ok)
        a[i] = v
        assert lib.tip_pose_rows(*a) == INV, (i, v)
    a = list(ok)
    a[8] = 0
    assert lib.tip_pose_rows(*a) == 0


# ---- the arithmetic --------------------------------------------------------------------------------------------------------------------
def _pairs(rng, N):
    """N pairs of axis-angles: any start (angles up to pi), relative rotations 1e-7 .. 3.0 rad (log-uniform)."""
    Ra = Rotation.random(N, random_state=rng)
    axis = rng.normal(size=(N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = np.exp(rng.uniform(np.log(1e-7), np.log(3.0), size=N))
    Rb = Ra * Rotation.from_rotvec(axis * angle[:, None])
    return Ra.as_rotvec(), Rb.as_rotvec(), angle


def test_conversions_are_scipys():
    """aa2q and q2aa in fp64 against scipy on 20 000 axis-angles of 0 .. 2 pi (an angle above pi comes back as its equivalent), the
    series on both sides of their thresholds, the identity, and the stated NaN behaviour."""
    rng = np.random.RandomState(11)
    N = 20000
    axis = rng.normal(size=(N, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = np.concatenate((np.exp(rng.uniform(np.log(1e-9), np.log(2e-3), size=N // 2)), rng.uniform(0.0, 2 * np.pi - 1e-3, size=N // 2)))
    a = axis * ang[:, None]
    q = do.aa2q(a, np.float64)
    ref = Rotation.from_rotvec(a)
    dq = np.abs(np.abs(np.einsum("ni,ni->n", q, ref.as_quat())) - 1.0).max()
    err = np.abs(do.quat_rotations(q[:, None])[:, 0] - ref.as_matrix()).max()
    back = do.q2aa(q, np.float64)
    err_back = np.abs(Rotation.from_rotvec(back).as_matrix() - ref.as_matrix()).max()
    print(f"aa2q: |1 - |q . scipy|| {dq:.3e}, rotation entries {err:.3e}; q2aa(aa2q): {err_back:.3e}")
    assert dq <= 1e-15 and err <= 2e-15 and err_back <= 1e-14
    assert np.linalg.norm(back, axis=1).max() <= np.pi + 1e-15
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= 1e-15
    assert np.array_equal(do.aa2q(np.zeros(3), np.float64), [0.0, 0.0, 0.0, 1.0]) and np.array_equal(do.q2aa([0.0, 0.0, 0.0, 1.0]), np.zeros(3))
    assert np.array_equal(do.aa2q(np.zeros(3, f32), f32), np.array([0, 0, 0, 1], f32)) and do.aa2q(np.zeros(3, f32), f32).dtype == f32
    for bad in ([np.nan, 0.1, 0.2], [0.1, np.inf, 0.2]):
        assert np.isnan(do.aa2q(np.array(bad), np.float64)).all() and np.isnan(do.between(bad, [0.1, 0.2, 0.3], 0.5)[0]).all()
    # fp32: t carries 1.5 ulp of relative error from its three squares, two sums and root (9e-8), so t / 2 is off by up to 2.8e-7 at
    # 2 pi, and that is the error of cos(t / 2) where its slope is 1; one more rounding on top: 3.4e-7
    lo = do.aa2q(a.astype(f32), f32)
    assert lo.dtype == f32 and np.abs(lo - do.aa2q(a.astype(f32).astype(np.float64), np.float64)).max() < 3.4e-7


def test_oracle_interpolation_is_scipys_slerp():
    """The fp64 oracle inside a bracket against scipy's Slerp between the two rows' rotations, as matrices (an axis-angle above pi is
    its equivalent), 20 000 pairs: within 1e-10 — the order of the packet oracle's 8e-11, which is the linear weights above
    d = 1 - 1e-6.  The root is the lerp."""
    rng = np.random.RandomState(5)
    N = 20000
    a, b, angle = _pairs(rng, N)
    u = rng.uniform(0.0, 1.0, size=N)
    u[:50] = 0.0
    aa, q = do.between(a, b, u, np.float64, stored=np.float64)
    assert np.isfinite(aa).all() and aa.dtype == np.float64
    Ra, Rb = Rotation.from_rotvec(a), Rotation.from_rotvec(b)
    ref = np.empty((N, 3, 3))
    for i in range(N):
        ref[i] = Slerp([0.0, 1.0], Rotation.concatenate([Ra[i], Rb[i]]))(u[i]).as_matrix()
    err = np.abs(Rotation.from_rotvec(aa).as_matrix() - ref).max(axis=(1, 2))
    small = angle < np.arccos(1 - 1e-6) * 2
    print(f"max |R - Slerp| {err.max():.3e} (linear branch: {int(small.sum())} pairs, {err[small].max():.3e}; slerp branch {err[~small].max():.3e})")
    assert small.sum() > 1000 and (~small).sum() > 1000
    assert err.max() <= 1e-10
    assert np.abs(do.quat_rotations(q[:, None])[:, 0] - ref).max() <= 1e-10 and np.abs(np.linalg.norm(q, axis=1) - 1.0).max() <= 1e-15
    assert (np.einsum("ni,ni->n", q, do.aa2q(a, np.float64)) > 0).all()                     # the earlier row's sign
    assert np.abs(Rotation.from_rotvec(aa[:50]).as_matrix() - Ra[:50].as_matrix()).max() <= 1e-15
    pa, pb = rng.normal(size=(N, 3)), rng.normal(size=(N, 3))
    p = do.root(pa, pb, u, np.float64, stored=np.float64)
    assert np.abs(p - ((1 - u)[:, None] * pa + u[:, None] * pb)).max() <= 1e-15


def test_oracle_prediction_is_the_analytic_spin():
    """The fp64 oracle's predicted pose against an analytic constant-rate spin per joint and a constant-velocity root: rates 0.1 .. 8
    rad/s, u up to 10, baseline 1 .. 4, through decide and emit's own arithmetic on unrounded rows.  Bound 1e-12: a few dozen fp64
    operations on unit quantities with two orders of margin (the packet predictor's oracle measured 4e-15 on the same check at u <= 3)."""
    rng = np.random.RandomState(9)
    rates = np.concatenate((np.exp(np.linspace(np.log(0.1), np.log(8.0), do.ROTS - 2)), [0.1, 8.0]))
    worst_r, worst_p, seen = 0.0, 0.0, set()
    for baseline in (1, 2, 3, 4):
        stamps = ro.stamps_at(rng, 6, 60.0, t0=3.0, jitter=0.2)
        rt, aa, analytic = do.spin_track(rng, stamps, rates)
        span = stamps[-1] - stamps[-1 - baseline]
        for u_want in (1.0 + 1e-9, 1.3, 2.0, 4.7, 10.0):
            tau = stamps[-1 - baseline] + u_want * span
            f, ia, ib, u = do.decide(stamps, tau, None, 1.0, baseline, do.PREDICT)
            assert (f, ia, ib) == (do.F_PREDICT, 5 - baseline, 5) and abs(u - u_want) < 1e-9
            got, q = do.between(aa[ia], aa[ib], u, np.float64, past=True, stored=np.float64)
            R_ref, p_ref = analytic(tau)
            e_r = np.abs(Rotation.from_rotvec(got).as_matrix() - R_ref.as_matrix()).max(axis=(1, 2))
            e_p = np.abs(do.root(rt[ia], rt[ib], u, np.float64, stored=np.float64) - p_ref).max()
            worst_r, worst_p = max(worst_r, e_r.max()), max(worst_p, e_p)
            assert np.abs(do.quat_rotations(q) - R_ref.as_matrix()).max() <= 1e-12
            seen.add((baseline, u_want))
    print(f"predicted rotation entries vs the analytic spin: max {worst_r:.3e}; root: {worst_p:.3e}")
    assert len(seen) == 20
    assert worst_r <= 1e-12 and worst_p <= 1e-12


def test_oracle_slerp_is_the_packet_sides():
    """display_oracle.slerp restates the packet oracles' quaternion statements (it has to take unrounded fp64 rows, which they do not):
    on fp32 quaternions it gives resample_oracle.interp's and sync_oracle.predict's quaternion columns bit for bit, in both dtypes."""
    rng = np.random.RandomState(4)
    a, b, _ = _pairs(rng, 3000)
    qa, qb = do.aa2q(a.astype(f32), f32), do.aa2q(b.astype(f32), f32)
    A, B = (np.concatenate((q, np.zeros((len(q), 3), f32)), axis=1) for q in (qa, qb))
    u = rng.uniform(0.0, 1.0, size=len(a))
    for dtype in (f32, np.float64):
        mine = do.slerp(qa.astype(dtype), qb.astype(dtype), u, dtype)
        assert np.array_equal(mine, ro.interp(A, B, u, dtype)[:, :4])
        mine = do.slerp(qa.astype(dtype), qb.astype(dtype), 1.0 + 5 * u, dtype, past=True)
        assert np.array_equal(mine, so.predict(A, B, 1.0 + 5 * u, dtype)[:, :4])


def test_two_rotations_pi_apart_have_no_shorter_arc():
    for dtype in (f32, np.float64):
        a = np.array([[0.0, 0.0, 0.0], [0.3, 0.1, -0.2], [0.0, 0.0, 0.0]], dtype=f32)
        b = np.array([[np.pi, 0.0, 0.0], [0.35, 0.1, -0.2], [np.pi - 1e-3, 0.0, 0.0]], dtype=f32)
        aa, q = do.between(a, b, 0.5, dtype)
        assert np.isnan(aa[0]).all() and np.isnan(q[0]).all() and np.isfinite(aa[1:]).all() and np.isfinite(q[1:]).all()


# ---- the rules -------------------------------------------------------------------------------------------------------------------------
def test_decision_table():
    s = [1.0, 2.0, 2.5, 4.0]
    D = do.decide
    assert D([], 3.0)[0] == do.F_EMPTY and D(s, 0.5)[0] == do.F_EARLY and D(s, float("nan"))[0] == do.F_EARLY
    for mode in (do.SLERP, do.PREDICT):
        assert D(s, 2.25, None, 9.0, 1, mode) == (do.F_INTERP, 1, 2, 0.5) and D(s, 4.0, None, 9.0, 1, mode) == (do.F_HELD, 3, 3, 0.0)
        assert D(s, 3.0, 1.0, 9.0, 1, mode) == (do.F_HELD, 2, 2, 0.0) and D(s, 3.75, 1.0, 9.0, 1, mode)[0] == do.F_STALE
    assert D(s, 2.25, None, 9.0, 1, do.HOLD) == (do.F_HELD, 1, 1, 0.0) and D(s, 5.0, None, 9.0, 1, do.HOLD) == (do.F_HELD, 3, 3, 0.0)
    assert D(s, 5.0, None, 9.0, 1, do.SLERP) == (do.F_HELD, 3, 3, 0.0)
    assert D(s, 5.5, None, 9.0, 1) == (do.F_PREDICT, 2, 3, 2.0) and D(s, 5.5, None, 9.0, 3) == (do.F_PREDICT, 0, 3, 1.5)
    assert D(s, 5.5, None, 9.0, 7) == (do.F_PREDICT, 0, 3, 1.5)                     # have - 1 < baseline: the oldest entry
    assert D(s, 5.5, None, 1.5, 1)[0] == do.F_PREDICT and D(s, 5.5, None, 1.49, 1) == (do.F_HELD, 3, 3, 0.0)   # max_predict
    assert D(s, 5.5, None, 0.0, 1) == (do.F_HELD, 3, 3, 0.0)
    assert D(s, 5.5, 1.5, 9.0, 1)[0] == do.F_PREDICT and D(s, 5.5, 1.4, 9.0, 1)[0] == do.F_STALE      # the dropout rule, b = 1
    assert D(s, 5.0, 1.0, 9.0, 3)[0] == do.F_PREDICT and D(s, 4.5, 0.99, 9.0, 3)[0] == do.F_HELD      # span 3.0 <= 3 max_hold
    assert D(s[:1], 5.5, None, 9.0, 1) == (do.F_HELD, 0, 0, 0.0)
    # the packet side would refuse 6 brackets past the newest entry; there is no span rule here
    grid = [k / 60.0 for k in range(8)]
    assert D(grid, grid[-1] + 6.7 / 60.0, None, 9 / 60.0, 1)[0] == do.F_PREDICT
    assert so.decide(grid, grid[-1] + 6.7 / 60.0, None, 9 / 60.0)[0] == do.F_HELD


def test_rings_rows_and_the_image():
    """The oracle's offline form against its live form in all three modes; push's rules and counters; the ring image's layout."""
    rng = np.random.RandomState(2)
    L = 40
    rt, sr, t = do.smooth_track(rng, L)
    st = 10.0 + t - 5 * do.DT
    out_t = np.sort(rng.uniform(st[0] - 0.02, st[-1] + 0.2, size=90))
    for mode, delay, hold, base in ((do.PREDICT, 0.0, None, 1), (do.PREDICT, 0.0, 0.05, 3), (do.SLERP, 0.012, 0.02, 1), (do.HOLD, 0.0, None, 1)):
        off, off_q, off_f = do.rows(st, rt, sr, out_t, delay, hold, 9 * do.DT, base, mode, depth=4)
        r, at = do.Rings(1, 4), 0
        for k, tk in enumerate(out_t):
            new = int(np.searchsorted(st, tk, side="right"))
            for j in range(at, new):
                r.push(rt[j][None], sr[j][None], st[j])
            at = new
            row, quat, f = r.emit(tk, delay, hold, 9 * do.DT, base, mode)
            assert f[0] == off_f[k] and np.array_equal(row[0].view(np.int32), off[k].view(np.int32)), (mode, k)
            assert np.array_equal(quat[0].view(np.int32), off_q[k].view(np.int32))
        seen = set(int(f) for f in off_f)
        assert (do.F_PREDICT in seen) == (mode == do.PREDICT) and (do.F_INTERP in seen) == (mode != do.HOLD and delay > 0), (mode, seen)
        # (a row sees the entries up to its own time: without a delay there is no later entry to interpolate towards)
    r = do.Rings(3, depth=4)
    root_, s_rest = rng.normal(size=(3, 3)).astype(f32), rng.normal(size=(3, 111)).astype(f32)
    for tk in (1.0, 2.0, 2.0, 1.5, np.nan, 3.0, 4.0, 5.0):
        r.push(root_, s_rest, [tk, tk + 10, tk], valid=[True, True, False], slots=[0, 1, 7, -1])
    have, dropped, total = r.counts()
    assert list(have) == [4, 4, 0] and list(dropped) == [3, 3, 0] and list(total) == [5, 5, 0]
    assert r.stamps[0] == [2.0, 3.0, 4.0, 5.0] and np.array_equal(r.rows[0][0], np.concatenate((root_[0], s_rest[0, :54])))
    img = r.image()
    assert img.shape == (3, do.block_bytes(4)) and list(img[0, :16].view(np.int32)) == [1, 4, 5, 3] and not img[2].any()
    assert list(img[0, 16:48].view(np.float64)) == [5.0, 2.0, 3.0, 4.0]
    r.reset([0])
    assert r.stamps[0] == [] and r.counts()[2][1] == 5


# ---- the Python layer ------------------------------------------------------------------------------------------------------------------
def test_pose_time_and_the_default_horizon():
    assert display.IMU_N_SMOOTH == 5 and display.DT == 1.0 / 60
    assert display.pose_time(2.0) == 2.0 - 5 * (1.0 / 60) and isinstance(display.pose_time(2.0), float)
    assert display.pose_time(1.7e9 + 0.25) == (1.7e9 + 0.25) - 5 * (1.0 / 60)
    t = np.array([0.0, 1.0, 1.7e9])
    assert np.array_equal(display.pose_time(t), t - 5 * (1.0 / 60)) and display.pose_time(t).dtype == np.float64
    assert display.pose_time(torch.tensor([1.0], dtype=torch.float64)).dtype == torch.float64
    # the derived lag: 5 frames + the 0.6**k filter's mean delay + half a frame, under the cap of 9 frames with two frames of slack
    w = 0.6 ** np.arange(6)
    assert abs(display.FILTER_DELAY_FRAMES - (np.arange(6) * w).sum() / w.sum()) < 1e-12 and abs(display.FILTER_DELAY_FRAMES - 1.2064) < 1e-4
    lag = display.IMU_N_SMOOTH + display.FILTER_DELAY_FRAMES + display.AVERAGE_DELAY_FRAMES
    assert display.MAX_PREDICT == 9 * display.DT and lag + 2.0 <= 9.0 < lag + 3.0


def test_python_refusals_before_the_library_is_loaded(monkeypatch):
    """Every argument check of PoseResampler, push, emit, resample_poses and import_slots comes before the library is loaded or a device
    chosen: each is a ValueError in the caller's name, and only a good set of arguments gets as far as asking for the device."""
    def boom():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(tlib, "load", boom)
    P = display.PoseResampler
    for kw, what in (({"mode": "linear"}, "mode is"), ({"mode": 2}, "mode is"), ({"delay": -0.01}, "delay is"),
                     ({"delay": float("nan")}, "delay is"), ({"delay": float("inf")}, "delay is"), ({"delay": "x"}, "delay is"),
                     ({"max_hold": -1.0}, "max_hold is"), ({"max_hold": float("nan")}, "max_hold is"),
                     ({"max_predict": -0.1}, "max_predict is"), ({"max_predict": float("inf")}, "max_predict is"),
                     ({"max_predict": None}, "max_predict is"), ({"depth": 1}, "depth is"), ({"depth": 65}, "depth is"),
                     ({"depth": 8.0}, "depth is"), ({"depth": True}, "depth is"), ({"baseline": 0}, "baseline is"),
                     ({"baseline": 8}, "baseline is"), ({"baseline": 2, "depth": 2}, "baseline is"), ({"baseline": 1.0}, "baseline is")):
        with pytest.raises(ValueError, match="PoseResampler: " + what):
            P(2, "cpu", **kw)
    for n in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="n is the number of slots"):
            P(n, "cpu")
    with pytest.raises(RuntimeError, match="runs on an MI355X"):
        P(2, "cpu", mode="hold", delay=0.0, max_hold=0.5, depth=64, baseline=63, max_predict=0.0)
    # push and emit on an object that never got a device
    ps = object.__new__(P)
    ps.n, ps.depth, ps.device, ps._lists = 3, 8, torch.device("cpu"), {}
    ps.t = ps.t_push = torch.zeros(3, dtype=torch.float64)
    root, s_rest = torch.zeros((3, 3)), torch.zeros((3, 111))
    for args, what in (((np.zeros((3, 3), f32), s_rest, 0.0), "root is"), ((root, torch.zeros((3, 53)), 0.0), "s_rest is"),
                       ((root.double(), s_rest, 0.0), "root is"), ((torch.zeros((2, 3)), s_rest, 0.0), "root is"),
                       ((root, s_rest.t().contiguous().t(), 0.0), "s_rest is read where it lies"),
                       ((root, s_rest, torch.zeros(3)), "float64 seconds"), ((root, s_rest, np.zeros(3, f32)), "float64 seconds"),
                       ((root, s_rest, [0.0, 1.0]), r"t is a number or \[3\]"), ((root, s_rest, True), r"t is a number or \[3\]")):
        with pytest.raises(ValueError, match="PoseResampler.push: .*" + what):
            ps.push(*args)
    for kw, what in (({"valid": torch.zeros(3)}, "valid is"), ({"valid": torch.zeros(2, dtype=torch.bool)}, "valid is"),
                     ({"slots": [0, 0]}, "duplicate"), ({"slots": 3}, "slots is a list"), ({"slots": ["a"]}, "slots is a list")):
        with pytest.raises(ValueError, match="PoseResampler.push: .*" + what):
            ps.push(root, s_rest, 0.0, **kw)
    for args, what in (((torch.zeros(3),), "float64 seconds"), (([0.0] * 4,), r"t is a number or \[3\]"),
                       ((0.0, torch.zeros((3, 56))), "out is a contiguous float32"), ((0.0, torch.zeros((3, 57), dtype=torch.float64)), "out is")):
        with pytest.raises(ValueError, match="PoseResampler.emit: .*" + what):
            ps.emit(*args)
    # import_slots: another depth, another kind, another count
    ex = {"meta": {"kind": "poses", "depth": 8, "block_bytes": display.block_bytes(8)}, "per": {},
          "block": torch.zeros((2, display.block_bytes(8)), dtype=torch.uint8)}
    other = object.__new__(P)
    other.n, other.depth, other.device = 5, 4, torch.device("cpu")
    with pytest.raises(ValueError, match="display.PoseResampler.import_slots: depth= differs"):
        other.import_slots([0, 1], ex)
    other.depth = 8
    with pytest.raises(ValueError, match="export_slots of the same kind"):
        other.import_slots([0, 1], dict(ex, meta=dict(ex["meta"], kind="resampler")))
    with pytest.raises(ValueError, match="one row per listed slot"):
        other.import_slots([0, 1, 2], ex)
    with pytest.raises(ValueError, match="slot index outside"):
        other.import_slots([0, 5], ex)
    assert "poses" in handover.COMPONENTS
    w = handover.Wearers(2, {"poses": ex})
    with pytest.raises(ValueError, match="every component"):
        handover.import_wearers(w, [0, 1], clock=types.SimpleNamespace())
    other.depth = 4
    with pytest.raises(ValueError, match="depth= differs"):
        handover.import_wearers(w, [0, 1], poses=other)
    # resample_poses
    rt, rows, t = np.zeros((5, 3), f32), np.zeros((5, 111), f32), np.arange(5) * 0.01
    R = display.resample_poses
    for kw, what in (({"mode": "nearest"}, "mode is"), ({"delay": -1.0}, "delay is"), ({"max_hold": float("nan")}, "max_hold is"),
                     ({"depth": 0}, "depth is"), ({"baseline": 9}, "baseline is"), ({"max_predict": -1.0}, "max_predict is"),
                     ({"rate_hz": 0.0}, "rate_hz is"), ({"rate_hz": float("nan")}, "rate_hz is")):
        with pytest.raises(ValueError, match="resample_poses: " + what):
            R([rt, rt], [rows, rows], [t, t], **({"rate_hz": 90.0} | kw))
    with pytest.raises(ValueError, match="one of the two"):
        R([rt], [rows], [t])
    with pytest.raises(ValueError, match="one of the two"):
        R([rt], [rows], [t], [t], rate_hz=90.0)
    with pytest.raises(ValueError, match="no sequences"):
        R([], [], [], rate_hz=90.0)
    with pytest.raises(ValueError, match=r"rows_list\[1\] is \[L, >= 54\]"):
        R([rt, rt], [rows, rows[:, :53]], [t, t], rate_hz=90.0)
    with pytest.raises(ValueError, match=r"root_list\[0\] is \[5, 3\]"):
        R([rt[:4], rt], [rows, rows], [t, t], rate_hz=90.0)
    with pytest.raises(ValueError, match="1 root arrays for 2 row arrays"):
        R([rt], [rows, rows], [t, t], rate_hz=90.0)
    with pytest.raises(ValueError, match="2 row arrays for 1 stamp arrays"):
        R([rt, rt], [rows, rows], [t], rate_hz=90.0)
    with pytest.raises(ValueError, match=r"stamps_list\[1\] is \[5\]"):
        R([rt, rt], [rows, rows], [t, t[:4]], rate_hz=90.0)
    with pytest.raises(ValueError, match="float64 seconds"):
        R([rt, rt], [rows, rows], [t, t.astype(f32)], rate_hz=90.0)
    bad = t.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match=r"stamps_list\[1\] row 3 is not finite"):
        R([rt, rt], [rows, rows], [t, bad], rate_hz=90.0)
    bad = t.copy()
    bad[2] = bad[1]
    with pytest.raises(ValueError, match=r"stamps_list\[0\] row 2 is not after row 1"):
        R([rt, rt], [rows, rows], [bad, t], rate_hz=90.0)
    with pytest.raises(ValueError, match="1 output-time arrays for 2 sequences"):
        R([rt, rt], [rows, rows], [t, t], [t])
    with pytest.raises(ValueError, match=r"t_out_list\[1\] is \[K\]"):
        R([rt, rt], [rows, rows], [t, t], [t, t.reshape(5, 1)])
