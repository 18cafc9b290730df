"""No GPU: the host half of ReplayPool(terrain=...) (tip_amd.replay) — the composed closed-loop oracle (tests/replay_terrain_oracle.py)
held to the reference-generated tests/golden/tip_terrain_loop_golden.npz (the real RTRunner.step around the reference's own model,
IK feedback in the loop), the numpy specification replay_on_host(make_tracker=...), the refusals, and the C-ABI surface of
tip_replay_mask / tip_replay_collect_tracked."""
import os
import re

import numpy as np
import pytest

import replay_terrain_oracle as rto
from conftest import ROOT
from tip_amd import lib as tlib
from tip_amd import replay

GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "tip_terrain_loop_golden.npz")
ORACLE_BOUND = 1e-11              # oracle against golden: the bound of tests/test_kin_cpu.py


# ---- 1. the override's meaning, against the real reference ---------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(GOLDEN_PATH), reason="tests/golden/make_terrain_loop_golden.py found no qualifying seed")
def test_composed_oracle_reproduces_the_closed_loop_fixture():
    """Teacher-forced on the fixture's raw model rows, StreamOracle + terrain_oracle.step + the override as the device defines it (the
    newest history row's columns 0 .. 107 <- aa_to_rot6d of the fired pose) gives what RTRunner.step gave: qdq, ct, the fed-back pose
    and — the point — the history rows the next model call reads, within 1e-11; fire flags equal.
    Measured: qdq 2.2e-16, ct 0, q_hist 4.3e-15, hist 3.6e-15, viz_locs 6.7e-16 over F_cmp = 160 rows, 127 of them fired.  (Without the
    float32 "root_v * DT" of the runner's first five calls, which ClosedLoop restates, the root alone is 1.8e-9 off.)"""
    g = np.load(GOLDEN_PATH)
    table = {k[len("table/"):]: g[k] for k in g.files if k.startswith("table/")}
    F = int(g["F_cmp"][0])
    rows = iter(g["y_last"][g["valid"]])
    got = rto.run(table, g["raw_imu"][:F], g["s_init"], lambda x_imu, x_s: next(rows))
    assert np.array_equal(got["valid"], g["valid"][:F]) and np.array_equal(got["fire"], g["fire"][:F])
    assert got["fire"].sum() >= 3
    qdq = np.concatenate([got["root"], got["s_rest"]], axis=1)
    err = {"qdq": np.abs(qdq - g["qdq"][:F]).max(), "ct": np.abs(got["c_t"] - g["ct"][:F]).max(),
           "q_hist": np.abs(got["q_hist"] - g["q_hist"][:F]).max(), "hist": np.abs(got["hist"] - g["hist"][:F]).max(),
           "viz_locs": np.abs(got["viz_locs"] - g["viz_locs"][:F]).max()}
    print("composed oracle against the closed-loop golden:", {k: float(f"{v:.2e}") for k, v in err.items()}, "fired rows", int(got["fire"].sum()))
    for k, v in err.items():
        assert v < ORACLE_BOUND, (k, v)
    # the same through the specification: replay_on_host(make_tracker=...) steps the tracker, applies the fired pose to the stream and
    # lays the rows out.  It stores float32 rows and takes s_init as float32 (check_inputs), so: fire flags equal, values within 1e-6
    # (half a float32 ulp of |x| < 4 is 2.4e-7, s_init's rounding 6e-8, carried by the root; the markers of inactive SBPs sit at 100
    # less the frame's correction, where half an ulp is 3.8e-6: 5e-6 for viz_locs)
    rows = iter(g["y_last"][g["valid"]])
    make_stream, make_tracker = rto.spec_pair(table, lambda x_imu, x_s: next(rows))
    (r,), frames = replay.replay_on_host([g["raw_imu"][:F]], g["s_init"][None], 1, make_stream, make_tracker=make_tracker)
    assert frames == F - 1 and type(r) is replay.TrackedReplayResult
    assert np.array_equal(r.fire, g["fire"][:F]) and np.array_equal(r.valid, g["valid"][:F]) and (r.off_map, r.regions_full) == (0, 0)
    for name, a, b in (("qdq", r.qdq, g["qdq"][:F]), ("c_t", r.c_t, g["ct"][:F]), ("q_hist", r.q_hist, g["q_hist"][:F]),
                       ("viz_locs", r.viz_locs, g["viz_locs"][:F])):
        assert np.abs(a - b).max() < (5e-6 if name == "viz_locs" else 1e-6), (name, np.abs(a - b).max())
    # the override is not a no-op on this fixture: on fired rows the history row is NOT the row of the returned pose
    fired = np.nonzero(g["fire"][:F])[0]
    from oracle.streaming_oracle import aa_to_rot6d
    plain = np.stack([aa_to_rot6d(g["qdq"][r, 3:57]) for r in fired])
    assert np.abs(plain - g["hist"][fired, :108]).max() > 1e-3


# ---- 2. the specification with a tracker ----------------------------------------------------------------------------------------------
class ToyStream:
    """A deterministic stand-in for a slot's closed loop: primes for five frames, then rows that depend on every frame so far and on
    every override so far."""

    def __init__(self, s_init_row):
        self.h = float(np.asarray(s_init_row, dtype=np.float64).sum())
        self.f = 0
        self.overrides = 0

    def step(self, raw):
        self.f += 1
        self.h = np.sin(self.h + float(np.asarray(raw, dtype=np.float64).sum()))
        if self.f <= 5:
            return None
        k = np.arange(131, dtype=np.float64)
        y = np.cos(self.h * (1 + 0.01 * k)).astype(np.float32)
        c = y[111:].copy()
        c[0::4] = c[0::4] > 0
        return y[:111].copy(), c, y

    def override(self, q):
        self.overrides += 1
        self.h += 0.5 + float(np.asarray(q, dtype=np.float64).sum())


class ToyTracker:
    """A deterministic stand-in for a slot's TerrainTracker block: a root that integrates, a pose it rewrites when it fires, counters."""
    made = []

    def __init__(self, s_init_row, fires=True):
        s = np.asarray(s_init_row, dtype=np.float32)
        self.root, self.k, self.fires = s[:3].copy(), 0, fires
        self.off_map = self.regions_full = 0
        ToyTracker.made.append(s.copy())

    def step(self, s_rest, c_t):
        self.k += 1
        self.root = self.root + np.float32(1 / 60) * s_rest[54:57]
        fired = self.fires and self.k % 3 != 1
        q = s_rest[:54].copy()
        if fired:
            q[3:12] += np.float32(0.1) * self.root.sum()
        self.off_map += int(c_t[4] > 0)
        self.regions_full += int(self.k % 5 == 0)
        viz = np.full((5, 3), self.k, dtype=np.float32) + self.root
        return self.root.copy(), viz, q, fired, self.off_map, self.regions_full


LENGTHS = [9, 1, 14, 6, 5, 20, 7, 11, 2]          # more recordings than slots; L = 1; L <= 6 (no valid row); 2: one priming row


def _toy_recordings():
    rng = np.random.RandomState(3)
    return [rng.randn(L, 72).astype(np.float32) for L in LENGTHS], (rng.randn(len(LENGTHS), 114) * 0.3).astype(np.float32)


def _same_tracked(a, b, who):
    assert type(a) is type(b) is replay.TrackedReplayResult
    for k in a._fields:
        x, y = getattr(a, k), getattr(b, k)
        assert np.array_equal(x, y, equal_nan=isinstance(x, np.ndarray) and x.dtype.kind == "f"), (who, k)


@pytest.mark.parametrize("slots", [1, 2, 3])
def test_spec_with_a_tracker_every_recording_equals_itself_alone(slots):
    recs, s0 = _toy_recordings()
    ToyTracker.made = []
    out, frames = replay.replay_on_host(recs, s0, slots, ToyStream, make_tracker=ToyTracker)
    assert frames == replay.plan_replay(LENGTHS, slots).n_frames
    # a fresh tracker (and stream) whenever a slot takes a recording, from that recording's s_init: the reset on re-attach
    order = [i for i in sorted(range(len(LENGTHS)), key=lambda i: (replay.plan_replay(LENGTHS, slots).start[i], i)) if LENGTHS[i] > 1]
    assert len(ToyTracker.made) == len(order) and all(np.array_equal(m, s0[i]) for m, i in zip(ToyTracker.made, order))
    fired_total = 0
    for i, r in enumerate(out):
        alone, _ = replay.replay_on_host([recs[i]], s0[i:i + 1], 1, ToyStream, make_tracker=ToyTracker)
        _same_tracked(r, alone[0], (slots, i))
        L, prim = LENGTHS[i], min(LENGTHS[i], 6)
        # the row conventions of the new arrays: row 0 and the priming rows are the start state, markers at 100, nothing fired
        assert r.root.shape == (L, 3) and r.viz_locs.shape == (L, 5, 3) and r.q_hist.shape == (L, 54) and r.fire.shape == (L,)
        assert r.fire.dtype == bool and r.root.dtype == r.viz_locs.dtype == r.q_hist.dtype == np.float32
        assert np.array_equal(r.root[:prim], np.repeat(s0[i][None, :3], prim, 0)) and (r.viz_locs[:prim] == 100).all()
        assert np.array_equal(r.q_hist[:prim], np.repeat(s0[i][None, 3:57], prim, 0)) and not r.fire[:prim].any()
        assert not r.valid[:prim].any() and r.valid[prim:].all()
        assert np.array_equal(r.q_hist[~r.fire], r.s_rest[~r.fire, :54]) and (r.q_hist[r.fire] != r.s_rest[r.fire, :54]).any(axis=1).all()
        assert np.array_equal(r.qdq, np.concatenate([r.root, r.s_rest], axis=1)) and r.qdq.shape == (L, 114)
        assert isinstance(r.off_map, int) and isinstance(r.regions_full, int)
        assert r.regions_full == (L - prim) // 5 and (r.off_map == 0) == (L <= 6 or not (r.c_t[:, 4] > 0).any())
        fired_total += int(r.fire.sum())
    assert fired_total >= 5


def test_spec_feedback_reaches_the_stream():
    """Up to and including a recording's first fired row its rows are those of the run without feedback; behind it they are not."""
    recs, s0 = _toy_recordings()
    fed, _ = replay.replay_on_host(recs, s0, 2, ToyStream, make_tracker=ToyTracker)
    quiet, _ = replay.replay_on_host(recs, s0, 2, ToyStream, make_tracker=lambda row: ToyTracker(row, fires=False))
    hit = 0
    for a, b in zip(fed, quiet):
        assert not b.fire.any()
        if not a.fire.any():
            assert np.array_equal(a.s_rest, b.s_rest)
            continue
        t = int(np.nonzero(a.fire)[0][0])
        assert np.array_equal(a.s_rest[:t + 1], b.s_rest[:t + 1]) and np.array_equal(a.root[:t + 1], b.root[:t + 1])
        if t + 1 < a.s_rest.shape[0]:
            assert not np.array_equal(a.s_rest[t + 1:], b.s_rest[t + 1:])
            hit += 1
    assert hit >= 3


def test_spec_without_a_tracker_is_unchanged():
    """No make_tracker: ReplayResult (four fields), and the rows of a tracked run whose tracker never fires (nothing reaches the stream)."""
    recs, s0 = _toy_recordings()
    plain, frames = replay.replay_on_host(recs, s0, 2, ToyStream)
    again, _ = replay.replay_on_host(recs, s0, 2, ToyStream, n_c=20, n_y=131, make_tracker=None)
    quiet, frames_q = replay.replay_on_host(recs, s0, 2, ToyStream, make_tracker=lambda row: ToyTracker(row, fires=False))
    assert frames == frames_q
    for a, b, q in zip(plain, again, quiet):
        assert type(a) is replay.ReplayResult and a._fields == ("s_rest", "c_t", "valid", "y_last")
        for k in a._fields:
            assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True) and np.array_equal(getattr(a, k), getattr(q, k), equal_nan=True), k
    assert replay.ReplayResult._fields == ("s_rest", "c_t", "valid", "y_last")
    assert replay.TrackedReplayResult._fields == ("s_rest", "c_t", "valid", "y_last", "root", "viz_locs", "q_hist", "fire", "off_map",
                                                  "regions_full")


def test_trim_takes_the_tracked_rows():
    recs, s0 = _toy_recordings()
    out, _ = replay.replay_on_host(recs, s0, 3, ToyStream, make_tracker=ToyTracker)
    r = out[5]
    t = replay.trim_like_reference(r.qdq)
    assert t.shape == (20, 114) and np.array_equal(t[:13], r.qdq[7:]) and np.array_equal(t[13:], np.repeat(r.qdq[-1:], 7, 0))


# ---- 3. the C-ABI surface ---------------------------------------------------------------------------------------------------------------
def test_tracked_replay_c_abi_surface():
    """Header, bindings and exported symbols of tip_replay_mask / tip_replay_collect_tracked, and their argument checks (no launch)."""
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5
    for name, nargs in (("tip_replay_mask", 5), ("tip_replay_collect_tracked", 25)):
        m = re.search(r"TIP_API int " + name + r"\((.*?)\);", hdr, re.S)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in tlib.EXPORTS
    lib = tlib.load()
    assert len(lib.tip_replay_mask.argtypes) == 5 and len(lib.tip_replay_collect_tracked.argtypes) == 25
    assert lib.tip_abi_version() == 5
    assert lib.tip_replay_mask(64, 64, 0, 64, None) == 0                  # no slots: nothing to launch
    for bad in ((None, 64, 1, 64), (64, None, 1, 64), (64, 64, 1, None), (64, 64, -1, 64), (68, 64, 1, 64)):
        assert lib.tip_replay_mask(*bad, None) == -1, bad
    ok = dict(cur=64, end=64, n=0, rows=4, s_rest=64, c_t=64, y_slot=64, rows_slot=64, size_s=131, s_out=64, c_out=64, y_out=64, valid=64,
              t_root=64, t_viz=64, t_q=64, t_fire=64, t_state=64, stride=1280, root_out=64, viz_out=64, q_out=64, fire_out=64, cnt_out=64)
    call = lambda **k: lib.tip_replay_collect_tracked(*{**ok, **k}.values(), None)  # noqa: E731
    assert call() == 0 and call(y_out=None, y_slot=None) == 0 and call(size_s=119) == 0
    for bad in (dict(size_s=130), dict(cur=None), dict(end=68), dict(valid=None), dict(y_slot=None), dict(c_out=72), dict(n=-1), dict(rows=-1),
                dict(t_root=None), dict(t_viz=None), dict(t_q=None), dict(t_fire=None), dict(t_state=None), dict(stride=1279), dict(stride=-8),
                dict(root_out=None), dict(viz_out=None), dict(q_out=None), dict(fire_out=None), dict(cnt_out=None), dict(s_rest=None),
                dict(rows_slot=None)):
        assert call(**bad) == -1, bad


# ---- 4. refusals before anything is launched ----------------------------------------------------------------------------------------------
def test_pool_refuses_a_bad_terrain_dict_before_it_builds_anything():
    """ValueError from the dict alone: no model is touched (None stands in for it), nothing is allocated."""
    with pytest.raises(ValueError, match="terrain is dict"):
        replay.ReplayPool(None, slots=2, terrain=dict(skel=object(), map_bound=5.0, grid=0.1))
    with pytest.raises(ValueError, match="terrain is dict"):
        replay.ReplayPool(None, slots=2, terrain=dict(map_bound=5.0, grid_size=0.1))
