"""GPU tests of the display-time poses (csrc/tip_display.hip; tip_amd.display.PoseResampler, resample_poses) against their numpy oracle
(tests/display_oracle.py): recorded tracks at the edges of the kernel's tile, every branch of the decision, of the ring and of the
rotation arithmetic, the live rings against the offline launch bit for bit in all three modes, chunking, epoch-sized stamps, reset,
hand-over, and the resampler beside an engine and a tracker, launch by launch and captured.

No fixture from the reference is needed: the reference has no display-time resampling; what it fixes is the pose's age (pose_time).

Bounds: flags and counters are equal (every decision is an fp64 comparison of stated expressions); a held row is the pushed row, bit
for bit; an interpolated or predicted row is within 3 x the oracle's own fp32 noise of the fp64 oracle — noise = max |oracle in fp32 -
oracle in fp64| on the same rows, the rule of tests/test_resample_gpu.py — measured per test on the rotation matrices of the output
axis-angles (an axis-angle above pi comes back as its equivalent: matrices, not vectors) and on the root separately."""
import ctypes

import numpy as np
import pytest
import torch

import display_oracle as do
import tip_amd
from tip_amd import display, handover, kinematics as kin
from tip_amd import lib as tlib
from test_resample_gpu import UNIT
from test_staggered_streams_gpu import paper  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE = {do.PREDICT: "predict", do.SLERP: "slerp", do.HOLD: "hold"}
S = tip_amd.streaming
EPS = float(np.finfo(f32).eps)


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tile():
    rows = ctypes.c_int()
    assert tlib.load().tip_pose_tile(ctypes.byref(rows)) == 0
    return rows.value


def _rows_dev(seqs, t_outs, rule, depth=8):
    """resample_poses on tracks [(stamps, root, rows)] -> (q [K, 57], quat [K, 18, 4], flags [K]), the sequences back to back."""
    mode, delay, hold, far, base = rule
    q, fl, qt = display.resample_poses([s[1] for s in seqs], [s[2] for s in seqs], [s[0] for s in seqs], t_outs, mode=MODE[mode],
                                       delay=delay, max_hold=hold, max_predict=far, baseline=base, depth=depth, device="cuda", host=True,
                                       quat=True)
    return np.concatenate(q), np.concatenate(qt), np.concatenate(fl)


def _oracle_rows(seqs, t_outs, rule, depth=8):
    mode, delay, hold, far, base = rule
    out = []
    for dtype in (f32, np.float64):
        parts = [do.rows(st, rt, rw, t, delay, hold, far, base, mode, depth, dtype) for (st, rt, rw), t in zip(seqs, t_outs)]
        out.append(tuple(np.concatenate([p[j] for p in parts]) for j in range(3)))
    assert np.array_equal(out[0][2], out[1][2])
    return out


def _hold_to_oracle(got, lo, hi, who):
    """got, lo (the oracle in fp32), hi (in fp64): (q, quat, flags).  Flags equal; held rows bit for bit, NaN rows NaN; interpolated and
    predicted rows within 3 x the measured fp32 noise as rotation matrices and root vectors, NaN where the oracle's are; quat unit and
    the same rotations as q.  Prints the figures before it asserts."""
    (q, quat, flags), (q32, quat32, f32_), (q64, quat64, _) = got, lo, hi
    assert np.array_equal(flags, f32_), (who, np.flatnonzero(flags != f32_)[:8])
    two = (flags == do.F_INTERP) | (flags == do.F_PREDICT)
    held = flags == do.F_HELD
    assert np.array_equal(_bits(q[held]), _bits(q32[held])), who
    assert np.isnan(q[~two & ~held]).all() and np.isnan(quat[~two & ~held]).all(), who
    with np.errstate(invalid="ignore"):
        if held.any():       # a held row's quaternions: the same fp32 statements, fp64 sines rounded once — an ulp where libm's last bit differs
            assert np.array_equal(np.isnan(quat[held]), np.isnan(quat32[held])), who
            assert float(np.nanmax(np.abs(quat[held] - quat32[held]), initial=0.0)) <= 2 * EPS, who
        if not two.any():
            print(f"{who}: {len(flags)} rows, none interpolated or predicted")
            return
        g, l, h = q[two], q32[two], q64[two]
        assert np.array_equal(np.isnan(g), np.isnan(h)) and np.array_equal(np.isnan(l), np.isnan(h)), who
        assert np.array_equal(np.isnan(quat[two]), np.isnan(quat64[two])), who
        Rh = do.rotations(h)
        noise_r, err_r = float(np.nanmax(np.abs(do.rotations(l) - Rh))), float(np.nanmax(np.abs(do.rotations(g) - Rh)))
        noise_p, err_p = float(np.nanmax(np.abs(l[:, :3] - h[:, :3]))), float(np.nanmax(np.abs(g[:, :3].astype(np.float64) - h[:, :3])))
        off_unit = float(np.nanmax(np.abs(np.linalg.norm(quat[two | held].astype(np.float64), axis=-1) - 1.0)))
        same = float(np.nanmax(np.abs(do.quat_rotations(quat[two]) - do.rotations(g))))
    print(f"{who}: {int((flags == 0).sum())} interpolated and {int((flags == 5).sum())} predicted rows of {len(flags)}; fp32 noise rot "
          f"{noise_r:.3e} root {noise_p:.3e}; device error rot {err_r:.3e} root {err_p:.3e}; | |quat| - 1 | {off_unit:.3e}; "
          f"R(quat) - R(q) {same:.3e}")
    assert err_r <= 3.0 * noise_r and err_p <= 3.0 * noise_p, who
    # q is quat through the header's quaternion -> axis-angle statement: v (three squares, two sums, a root: 1.5 ulp), k (one rounding)
    # and the product (one rounding) put at most four half-ulps of relative error on an angle of at most pi
    assert off_unit <= UNIT and same <= 2.0 * EPS * np.pi, who


# ---- (a) recorded tracks against the oracle ----------------------------------------------------------------------------------------------
RULES = [(do.PREDICT, 0.0, None, 9 * do.DT, 1), (do.PREDICT, 0.02, 0.03, 0.05, 3), (do.SLERP, 0.02, None, 0.0, 1), (do.HOLD, 0.0, 0.05, 0.0, 1)]


@pytest.mark.parametrize("depth", [2, 8])
@pytest.mark.parametrize("rule", RULES, ids=lambda r: f"{MODE[r[0]]}-{r[1]}-{r[2]}-b{r[4]}")
def test_rows_match_the_oracle(rule, depth):
    """Tracks of 1, 2, 17 and 80 rows at 30, 60 and 100 Hz, each taken at 0, 1, tile - 1, tile and tile + 1 times that start a little
    before its first row and run past its last: 60 ragged sequences, one launch."""
    rng = np.random.RandomState(17)
    tile = _tile()
    rule = rule[:4] + (min(rule[4], depth - 1),)
    seqs, t_outs = [], []
    for L in (1, 2, 17, 80):
        for rate in (30.0, 60.0, 100.0):
            for K in (0, 1, tile - 1, tile, tile + 1):
                rt, sr, t = do.smooth_track(rng, L, rate)
                st = 50.0 + rng.uniform(0.0, 1.0) + t + rng.uniform(-0.2, 0.2, size=L) / rate
                seqs.append((st, rt, sr))
                t_outs.append(np.sort(rng.uniform(st[0] - 0.03, st[-1] + 0.12, size=K)))
    got = _rows_dev(seqs, t_outs, rule, depth)
    lo, hi = _oracle_rows(seqs, t_outs, rule, depth)
    print({int(f): int((lo[2] == f).sum()) for f in range(6)})
    assert (lo[2] == do.F_EMPTY).sum() >= 3 and (lo[2] == do.F_HELD).sum() >= 3
    assert rule[0] != do.PREDICT or (lo[2] == do.F_PREDICT).sum() >= (60 if rule[1] == 0.0 else 5)
    assert not (rule[0] != do.HOLD and rule[1] > 0 and depth == 8) or (lo[2] == do.F_INTERP).sum() >= 60
    _hold_to_oracle(got, lo, hi, f"rows {MODE[rule[0]]} delay {rule[1]} max_hold {rule[2]} baseline {rule[4]} depth {depth}")


# ---- (b) every branch ------------------------------------------------------------------------------------------------------------------
B_RULE = (do.PREDICT, 0.02, 0.03, 0.05, 2)      # mode, delay, max_hold, max_predict, baseline
B_DEPTH = 8


@pytest.fixture(scope="module")
def branches():
    """Three tracks under up to 125 output times each (90 Hz), built to reach every branch of the decision and of the rotation arithmetic, and
    a live script that reaches every branch of the ring, with the number of output rows (or joints of output rows) that reach each.
    Track 0 and 1: 70 rows at 60 Hz; the output times start before the first row (EMPTY, then EARLY); row 20 is missing (a 33 ms
    gap, longer than max_hold: predicted across, then the dropout bracket held and stale); rows 40-41 and 43-44 are missing (row 42 alone between two gaps:
    prediction refused by the dropout rule, the newest row held, then stale); the output times run 0.2 s past the last row (predicted,
    then refused by max_predict).  Track 2: two rows (have - 1 < baseline).  Joint 5 never moves from 0 (theta = 0); joint 6 stays
    below the series thresholds; joints 7 and 8 turn about a fixed axis just under and just over pi; joint 9 of rows 30 and 31 is 0
    and (pi, 0, 0): pi apart; row 50 has a NaN in joint 10 and row 55 a NaN in the root."""
    rng = np.random.RandomState(29)
    seqs, t_outs = [], []
    for j in range(3):
        L = 70 if j < 2 else 2
        rt, sr, t = do.smooth_track(rng, L)
        st = 100.0 + 0.37 * j + t + rng.uniform(-0.001, 0.001, size=L)
        aa = sr[:, :54].reshape(L, 18, 3)
        aa[:, 5] = 0.0
        aa[:, 6] = 1e-4 * np.sin(3.0 * t + 0.5)[:, None] * np.array([0.6, -0.3, 0.7], f32)
        axis = np.array([0.48, -0.6, 0.64], f32)
        aa[:, 7] = axis * (np.pi - 0.02 + 0.005 * np.sin(4.0 * t))[:, None]
        aa[:, 8] = axis * (np.pi + 0.02 + 0.005 * np.sin(4.0 * t))[:, None]
        if j < 2:
            aa[30, 9], aa[31, 9] = 0.0, (np.pi, 0.0, 0.0)
            aa[50, 10, 1] = np.nan
            rt[55, 1] = np.nan
        sr[:, :54] = aa.reshape(L, 54)
        if j < 2:
            keep = np.ones(L, dtype=bool)
            keep[[20, 40, 41, 43, 44]] = False
            st, rt, sr = st[keep], rt[keep], sr[keep]
        seqs.append((st, rt, sr))
        t_outs.append(st[0] - 0.015 + np.arange(125) / 90.0 if j < 2 else st[-1] + 0.004 + np.arange(6) / 90.0)
    mode, delay, hold, far, base = B_RULE
    c = {k: 0 for k in ("empty", "early", "held_newest", "stale", "hold_in_bracket", "dropout_held", "dropout_stale", "interp", "predicted",
                        "refused_max_predict", "refused_dropout", "short_baseline", "theta_zero", "aa_series", "q_series", "under_pi",
                        "over_pi", "pi_apart", "nan_joint", "nan_root", "chord_branch")}
    for (st, rt, sr), tk in zip(seqs, t_outs):
        full = np.concatenate((rt, sr[:, :54]), axis=1)
        for t in tk:
            cnt = int(np.searchsorted(st, t, side="right"))
            lo = max(0, cnt - B_DEPTH)
            s, tau = st[lo:cnt], t - delay
            f, ia, ib, u = do.decide(s, tau, hold, far, base, mode)
            c["hold_in_bracket"] += int(do.decide(s, tau, hold, far, base, do.HOLD)[0] == do.F_HELD and len(s) > 1 and s[0] <= tau < s[-1])
            c["empty"] += int(f == do.F_EMPTY)
            c["early"] += int(f == do.F_EARLY)
            c["interp"] += int(f == do.F_INTERP)
            c["predicted"] += int(f == do.F_PREDICT)
            past = len(s) >= 2 and tau > s[-1]
            inside = len(s) >= 2 and s[0] <= tau < s[-1]
            c["held_newest"] += int(f == do.F_HELD and len(s) >= 1 and tau >= s[-1])
            c["stale"] += int(f == do.F_STALE and len(s) >= 1 and tau >= s[-1])
            c["dropout_held"] += int(f == do.F_HELD and inside)
            c["dropout_stale"] += int(f == do.F_STALE and inside)
            if past:
                b = min(base, len(s) - 1)
                c["short_baseline"] += int(b < base and f == do.F_PREDICT)
                c["refused_max_predict"] += int(tau - s[-1] > far)
                c["refused_dropout"] += int(tau - s[-1] <= far and f != do.F_PREDICT)
            if f not in (do.F_INTERP, do.F_PREDICT):
                continue
            a, bb = full[lo + ia, 3:].reshape(18, 3), full[lo + ib, 3:].reshape(18, 3)
            out, q = do.between(a, bb, u, f32, past=f == do.F_PREDICT)
            th = np.linalg.norm(a.astype(np.float64), axis=1)
            c["theta_zero"] += int(th[5] == 0.0)
            c["aa_series"] += int(0.0 < th[6] < do.AA_SERIES)
            with np.errstate(invalid="ignore"):
                c["q_series"] += int((0.0 < np.linalg.norm(q[6, :3])) and np.linalg.norm(q[6, :3]) < do.Q_SERIES)
            c["under_pi"] += int(np.pi - 0.05 < th[7] < np.pi)
            c["over_pi"] += int(np.pi < th[8] < np.pi + 0.05)
            fin = np.isfinite(a).all(axis=1) & np.isfinite(bb).all(axis=1)
            c["pi_apart"] += int(fin[9] and np.isnan(out[9]).all() and np.isfinite(out[8]).all() and np.isfinite(out[10]).all())
            c["nan_joint"] += int(not fin[10] and np.isnan(out[10]).all() and np.isfinite(out[9]).all() and np.isfinite(out[11]).all())
            c["nan_root"] += int(np.isnan(do.root(full[lo + ia, :3], full[lo + ib, :3], u, f32)).all())
            if f == do.F_PREDICT:
                qa, qb = do.aa2q(a[5:7].astype(f32), f32), do.aa2q(bb[5:7].astype(f32), f32)
                c["chord_branch"] += int((np.abs(do._dot4(qa, qb)) > 1 - 1e-6).any())
    return seqs, t_outs, c


def _live_script(rng, n, depth):
    """A push script on n slots that reaches every ring branch: depth + 3 good pushes (a wrap), a duplicate stamp, an earlier one, a
    NaN one, valid False, a slot outside [0, n).  -> list of (root, s_rest, t [n], valid or None, slots or None)."""
    steps = []
    for k in range(depth + 3):
        steps.append((rng.normal(size=(n, 3)).astype(f32), rng.normal(size=(n, 111)).astype(f32), 5.0 + k * do.DT + 0.001 * np.arange(n), None, None))
    bad = 5.0 + (depth + 2) * do.DT + 0.001 * np.arange(n)
    steps.append((steps[-1][0], steps[-1][1], bad, None, None))                                         # a duplicate of the newest
    steps.append((steps[-1][0], steps[-1][1], bad - 0.5, None, None))                                   # earlier
    t_nan = bad + do.DT
    t_nan[0] = np.nan
    steps.append((rng.normal(size=(n, 3)).astype(f32), rng.normal(size=(n, 111)).astype(f32), t_nan, None, None))   # slot 0: NaN
    valid = np.ones(n, dtype=bool)
    valid[1] = False
    steps.append((rng.normal(size=(n, 3)).astype(f32), rng.normal(size=(n, 111)).astype(f32), bad + 2 * do.DT, valid, None))
    steps.append((rng.normal(size=(n, 3)).astype(f32), rng.normal(size=(n, 111)).astype(f32), bad + 3 * do.DT, None, [n - 1, n + 4, -1, 0]))
    return steps


def _run_script(ps, ring, steps):
    for rt, sr, t, valid, slots in steps:
        ps.push(torch.from_numpy(rt).cuda(), torch.from_numpy(sr).cuda(), torch.from_numpy(np.asarray(t, dtype=np.float64)).cuda(),
                valid=None if valid is None else torch.from_numpy(valid).cuda(), slots=slots)
        ring.push(rt, sr, t, valid, slots)


def test_fixture_reaches_every_branch(branches):
    _, _, c = branches
    print(c)
    assert all(v > 0 for v in c.values()), c


def test_every_branch_matches_the_oracle(branches):
    """The fixture's rows in modes predict and hold.  That a joint pi apart, a NaN joint and a NaN root stay where they are is the
    NaN-mask equality of _hold_to_oracle on rows whose neighbours the fixture has counted finite."""
    seqs, t_outs, _ = branches
    for mode in (do.PREDICT, do.HOLD):
        rule = (mode,) + B_RULE[1:]
        got = _rows_dev(seqs, t_outs, rule, B_DEPTH)
        lo, hi = _oracle_rows(seqs, t_outs, rule, B_DEPTH)
        _hold_to_oracle(got, lo, hi, f"branches {MODE[mode]}")


@pytest.mark.parametrize("depth", [2, 8])
def test_ring_branches_and_counters(depth):
    """The live script on n = 3: counters, the ring image and the next emit equal the oracle's; a wrapped ring; refused stamps; valid
    False; a slot outside [0, n)."""
    rng = np.random.RandomState(31)
    n = 3
    steps = _live_script(rng, n, depth)
    ps = display.PoseResampler(n, "cuda", depth=depth, baseline=1)
    ring = do.Rings(n, depth)
    _run_script(ps, ring, steps)
    have, dropped, total = (c.cpu().numpy() for c in ps.counts())
    oh, od, ot = ring.counts()
    print(f"depth {depth}: have {have}, dropped {dropped}, total {total}")
    assert np.array_equal(have, oh) and np.array_equal(dropped, od) and np.array_equal(total, ot)
    assert (have == depth).all() and list(dropped) == [3, 2, 2] and list(total) == [depth + 5, depth + 4, depth + 6]
    assert np.array_equal(ps.state.cpu().numpy().reshape(n, -1), ring.image())
    assert [int(c[0]) for c in ps.counts([2])] == [depth, 2, depth + 6]
    t = float(steps[-1][2][0]) + 2.5 * do.DT
    q = ps.emit(t).cpu().numpy()
    got = (q, ps.quat.cpu().numpy(), ps.flags.cpu().numpy())
    lo = ring.emit(t, 0.0, None, display.MAX_PREDICT, 1, do.PREDICT, f32)
    hi = ring.emit(t, 0.0, None, display.MAX_PREDICT, 1, do.PREDICT, np.float64)
    assert (lo[2] == do.F_PREDICT).all()
    _hold_to_oracle(got, lo, hi, f"live script depth {depth}")


# ---- (c) chunking and selection ----------------------------------------------------------------------------------------------------------
def _pool_tracks(rng, n, F=40):
    """n tracks of F rows at 60 Hz on per-slot clocks -> stamps [n, F], root [n, F, 3], s_rest [n, F, 111]."""
    st, rt, sr = [], [], []
    for s in range(n):
        r, x, t = do.smooth_track(rng, F)
        st.append(20.0 + t + rng.uniform(0.0, 0.016) + rng.uniform(-0.003, 0.003, size=F))
        rt.append(r)
        sr.append(x)
    return np.stack(st), np.stack(rt), np.stack(sr)


def _live(ps, st, rt, sr, times):
    """Feed the pool as a server would: before each emit time, every slot's rows stamped up to it, one launch per round of due slots.
    -> (q [K, n, 57], quat, flags) as emitted."""
    n, F = st.shape
    rt_d, sr_d, st_d = torch.from_numpy(rt).cuda(), torch.from_numpy(sr).cuda(), torch.from_numpy(st).cuda()
    nxt = np.zeros(n, dtype=np.int64)
    ar = torch.arange(n, device="cuda")
    out = []
    for T in times:
        while True:
            due = (nxt < F) & (st[np.arange(n), np.minimum(nxt, F - 1)] <= T)
            if not due.any():
                break
            idx = torch.from_numpy(np.minimum(nxt, F - 1)).cuda()
            ps.push(rt_d[ar, idx].contiguous(), sr_d[ar, idx].contiguous(), st_d[ar, idx].contiguous(), valid=torch.from_numpy(due).cuda())
            nxt[due] += 1
        q = ps.emit(float(T))
        out.append((q.clone(), ps.quat.clone(), ps.flags.clone()))
    return tuple(torch.stack([o[j] for o in out]).cpu().numpy() for j in range(3))


@pytest.mark.parametrize("which", ["3", "tile-1", "tile", "tile+1"])
@pytest.mark.parametrize("mode", ["predict", "slerp", "hold"])
def test_live_equals_resample_poses_bit_for_bit(mode, which):
    """Push / emit frame by frame at 90 Hz equals resample_poses on the same tracks, bit for bit; and the ring image at the end equals
    the one that pushing every row in one go per frame leaves, and the oracle's."""
    tile = _tile()
    n = {"3": 3, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[which]
    rng = np.random.RandomState(41 + n)
    st, rt, sr = _pool_tracks(rng, n)
    times = 20.0 + np.arange(62) / 90.0
    kw = dict(mode=mode, delay=0.02 if mode == "slerp" else 0.0, max_hold=0.1, baseline=2, depth=8)
    kw.update({"max_predict": 0.07} if mode == "predict" else {"max_predict": 0.0})
    ps = display.PoseResampler(n, "cuda", **kw)
    q, quat, flags = _live(ps, st, rt, sr, times)
    rq, rf, rqt = display.resample_poses(list(rt), list(sr), list(st), [times] * n, device="cuda", host=True, quat=True, **kw)
    seen = set(int(f) for f in np.unique(flags))
    print(f"n {n} {mode}: flags seen {sorted(seen)}")
    assert {"predict": {do.F_PREDICT, do.F_EMPTY}, "slerp": {do.F_INTERP, do.F_EARLY}, "hold": {do.F_HELD}}[mode] <= seen
    for s in range(n):
        assert np.array_equal(flags[:, s], rf[s]) and np.array_equal(_bits(q[:, s]), _bits(rq[s])), (mode, s)
        assert np.array_equal(_bits(quat[:, s]), _bits(rqt[s])), (mode, s)
    # any chunking of pushes gives the same ring image: the rows again, one launch per frame for the whole pool
    due_end = (st <= times[-1]).sum(axis=1)
    again, ring = display.PoseResampler(n, "cuda", **kw), do.Rings(n, 8)
    for f in range(st.shape[1]):
        ok = f < due_end
        again.push(_dev(rt[:, f]), _dev(sr[:, f]), _dev(st[:, f]), valid=_dev(ok))
        ring.push(rt[:, f], sr[:, f], st[:, f], ok)
    assert torch.equal(again.state, ps.state) and np.array_equal(ps.state.cpu().numpy().reshape(n, -1), ring.image())


def test_max_predict_zero_is_slerp_and_the_baseline_is_read():
    rng = np.random.RandomState(7)
    rt, sr, t = do.smooth_track(rng, 60, speed=2.0)
    st = 3.0 + t
    out_t = np.sort(rng.uniform(st[0] - 0.01, st[-1] + 0.1, size=150))
    seqs = [(st, rt, sr)]
    a = _rows_dev(seqs, [out_t], (do.PREDICT, 0.01, None, 0.0, 1))
    b = _rows_dev(seqs, [out_t], (do.SLERP, 0.01, None, 0.0, 1))
    assert all(np.array_equal(x.view(np.int32) if x.dtype == f32 else x, y.view(np.int32) if y.dtype == f32 else y) for x, y in zip(a, b))
    assert set(np.unique(a[2])) >= {do.F_INTERP, do.F_HELD}
    one = _rows_dev(seqs, [out_t], (do.PREDICT, 0.0, None, 0.15, 1))
    three = _rows_dev(seqs, [out_t], (do.PREDICT, 0.0, None, 0.15, 3))
    p = (one[2] == do.F_PREDICT) & (three[2] == do.F_PREDICT)
    assert np.array_equal(one[2], three[2]) and p.sum() > 100
    diff = float(np.abs(do.rotations(one[0][p]) - do.rotations(three[0][p])).max())
    print(f"baseline 1 vs 3 on a curved track: rotation entries differ by up to {diff:.3e}")
    assert diff > 1e-3 and not np.array_equal(_bits(one[0][p][:, :3]), _bits(three[0][p][:, :3]))
    assert np.array_equal(_bits(one[0][~p]), _bits(three[0][~p]))


# ---- (d) stamps and slots ------------------------------------------------------------------------------------------------------------------
def test_epoch_sized_stamps():
    """Stamps of 1.7e9 s: fp64 resolves 2.4e-7 s there.  The rows equal the oracle's, and flags and u come out as on a clock that starts
    at 0 wherever the shift is exact."""
    rng = np.random.RandomState(13)
    rt, sr, t = do.smooth_track(rng, 50)
    k = np.arange(120) / 90.0 - 0.02
    for rule in ((do.PREDICT, 0.0, 0.05, 9 * do.DT, 2), (do.SLERP, 0.02, None, 0.0, 1)):
        seqs, t_outs = [(1.7e9 + t, rt, sr)], [1.7e9 + k]
        got = _rows_dev(seqs, t_outs, rule)
        lo, hi = _oracle_rows(seqs, t_outs, rule)
        assert {do.F_PREDICT if rule[0] == do.PREDICT else do.F_INTERP, do.F_HELD} <= set(np.unique(lo[2]))
        _hold_to_oracle(got, lo, hi, f"epoch {MODE[rule[0]]}")
    ps = display.PoseResampler(2, "cuda", depth=4)
    for f in range(6):
        ps.push(torch.from_numpy(np.stack([rt[f]] * 2)).cuda(), torch.from_numpy(np.stack([sr[f]] * 2)).cuda(), 1.7e9 + f * do.DT)
    ps.push(torch.from_numpy(np.stack([rt[6]] * 2)).cuda(), torch.from_numpy(np.stack([sr[6]] * 2)).cuda(), 1.7e9 + 5 * do.DT)   # refused
    assert [int(c[0]) for c in ps.counts()] == [4, 1, 6]
    ps.emit([1.7e9 + 5.5 * do.DT, 1.7e9 + 4.5 * do.DT])
    assert ps.flags.tolist() == [do.F_PREDICT, do.F_INTERP]


def test_reset_and_hand_over(tmp_path):
    """reset of one slot leaves the others' bytes alone; export_slots -> import_slots into a pool of another n (device to device, and
    through a file with the wearers' other components' conventions): the next emit equals the source's bit for bit."""
    rng = np.random.RandomState(19)
    n = 5
    st, rt, sr = _pool_tracks(rng, n, F=12)
    a = display.PoseResampler(n, "cuda", baseline=2)
    for f in range(12):
        a.push(_dev(rt[:, f]), _dev(sr[:, f]), _dev(st[:, f]))
    T = float(st.max()) + 0.03
    ref = a.emit(T).clone()
    ref_quat, ref_flags = a.quat.clone(), a.flags.clone()
    assert (ref_flags == do.F_PREDICT).all()
    src, dst = [4, 0, 2], [1, 6, 3]
    b = display.PoseResampler(7, "cuda", baseline=2)
    b.import_slots(dst, a.export_slots(src))
    got = b.emit(T)
    assert torch.equal(got[dst].view(torch.int32), ref[src].view(torch.int32)) and torch.equal(b.quat[dst].view(torch.int32), ref_quat[src].view(torch.int32))
    assert b.flags[dst].tolist() == [do.F_PREDICT] * 3 and b.flags[[0, 2, 4, 5]].tolist() == [do.F_EMPTY] * 4
    w = handover.export_wearers(src, poses=a).cpu()
    w.save(str(tmp_path / "w.npz"))
    c = display.PoseResampler(4, "cuda", baseline=2)
    handover.import_wearers(handover.Wearers.load(str(tmp_path / "w.npz")).to("cuda"), [3, 1, 0], poses=c)
    got = c.emit(T)
    assert torch.equal(got[[3, 1, 0]].view(torch.int32), ref[src].view(torch.int32)) and c.flags.tolist() == [5, 5, 3, 5]
    with pytest.raises(ValueError, match="depth= differs"):
        display.PoseResampler(4, "cuda", depth=4).import_slots([0, 1, 2], a.export_slots(src))
    before = a.state.clone().reshape(n, -1)
    a.reset([1])
    after = a.state.reshape(n, -1)
    assert torch.equal(after[[0, 2, 3, 4]], before[[0, 2, 3, 4]]) and not after[1].any()
    assert [int(c[0]) for c in a.counts([1])] == [0, 0, 0]
    a.emit(T)
    assert a.flags.tolist() == [5, do.F_EMPTY, 5, 5, 5]


# ---- (e) beside an engine ------------------------------------------------------------------------------------------------------------------
def _frames(n, F, seed):
    rng = np.random.RandomState(seed)
    raw = rng.randn(F, n, 72).astype(f32)
    raw[:, :, :54] = np.tile(np.eye(3, dtype=f32).reshape(9), 6) + 0.05 * raw[:, :, :54]
    return raw, (rng.randn(n, 114) * 0.2).astype(f32)


def test_beside_an_engine_launch_by_launch_and_captured(paper):
    """StaggeredStreamingEngine -> RootTracker.step -> push(pose_time(tick), valid) -> emit -> fk for 50 frames, n = 3, slot 2 taking a
    new wearer at frame 30.  The engine's outputs are bit-identical with and without the consumer; a slot that is still priming is flagged EMPTY;
    push + emit captured in one torch.cuda.graph (a single chain) and replayed equal launch mode bit for bit."""
    m, _ = paper
    skel = kin.Skeleton.from_table(np.load(__file__.replace("test_display_gpu.py", "golden/tip_kin_golden.npz")))
    n, F = 3, 50
    raw, s_init = _frames(n, F, 23)

    def run(consumer):
        eng = S.StaggeredStreamingEngine(m, s_init)
        rt = kin.RootTracker(skel, n, "cuda")
        rt.reset(None, s_init)
        ps = display.PoseResampler(n, "cuda") if consumer else None
        t_push = torch.zeros(n, dtype=torch.float64, device="cuda")
        t_emit = torch.zeros(n, dtype=torch.float64, device="cuda")
        valid = torch.zeros(n, dtype=torch.bool, device="cuda")
        q_out = torch.zeros((n, 57), device="cuda")
        graph, outs = None, []
        for f in range(F):
            if f == 30:
                eng.attach([2], s_init[[2]])
                rt.reset([2], s_init[[2]])
                if consumer:
                    ps.reset([2])
            out = eng.step(raw[f])
            root, _ = rt.step(out)
            rec = {k: out[k].clone() for k in ("s_rest", "c_t", "valid")}
            rec["root"] = root.clone()
            if consumer:
                tick = 100.0 + f * do.DT
                t_push.fill_(display.pose_time(tick))
                t_emit.fill_(tick + 0.004)
                valid.copy_(out["valid"])
                if consumer == "graph" and f >= 10:
                    if graph is None:                                   # (frames 0 .. 9 ran launch by launch: nothing is loaded inside the capture)
                        graph = torch.cuda.CUDAGraph()
                        with torch.cuda.graph(graph):
                            ps.push(root, out["s_rest"], t_push, valid=valid)
                            ps.emit(t_emit, out=q_out)
                    graph.replay()
                else:
                    ps.push(root, out["s_rest"], t_push, valid=valid)
                    ps.emit(t_emit, out=q_out)
                pq = kin.fk(skel, q_out, scale=rt.scale)
                rec.update(q=q_out.clone(), quat=ps.quat.clone(), flags=ps.flags.clone(), pq=pq.clone())
            outs.append(rec)
        torch.cuda.synchronize()
        return outs

    plain, beside, captured = run(None), run("launch"), run("graph")
    for f in range(F):
        for k in ("s_rest", "c_t", "root"):
            assert torch.equal(plain[f][k].view(torch.int32), beside[f][k].view(torch.int32)), (f, k)
        assert torch.equal(plain[f]["valid"], beside[f]["valid"])
        for k in ("q", "quat", "pq"):
            assert torch.equal(beside[f][k].view(torch.int32), captured[f][k].view(torch.int32)), (f, k)
        assert torch.equal(beside[f]["flags"], captured[f]["flags"])
    flags = torch.stack([o["flags"] for o in beside]).cpu().numpy()
    valid = torch.stack([o["valid"] for o in beside]).cpu().numpy()
    print(f"valid frames per slot {valid.sum(axis=0).tolist()}; flags of slot 2 {flags[:, 2].tolist()}")
    primes = np.zeros((F, n), dtype=bool)
    primes[:5] = True
    primes[30:35, 2] = True
    assert np.array_equal(valid, ~primes)
    want = np.full((F, n), do.F_PREDICT)                                    # 5 frames + 4 ms past the newest pose, every frame
    want[primes] = do.F_EMPTY                                                # priming: nothing pushed yet
    want[5], want[35, 2] = do.F_HELD, do.F_HELD                              # one entry: nothing to take a rate from
    assert np.array_equal(flags, want)
    last = beside[-1]
    assert torch.isfinite(last["q"]).all() and torch.isfinite(last["pq"]).all()
    # the predicted pose is the oracle's on the rows that were pushed
    ring = do.Rings(n, 8)
    for f in range(F):
        if f == 30:
            ring.reset([2])
        ring.push(beside[f]["root"].cpu().numpy(), beside[f]["s_rest"].cpu().numpy(), display.pose_time(100.0 + f * do.DT),
                  beside[f]["valid"].cpu().numpy())
    T = 100.0 + (F - 1) * do.DT + 0.004
    lo = ring.emit(T, 0.0, None, display.MAX_PREDICT, 1, do.PREDICT, f32)
    hi = ring.emit(T, 0.0, None, display.MAX_PREDICT, 1, do.PREDICT, np.float64)
    _hold_to_oracle((last["q"].cpu().numpy(), last["quat"].cpu().numpy(), last["flags"].cpu().numpy()), lo, hi, "beside an engine")
