"""The closed loop of the full runner in numpy, for the tests of ReplayPool(terrain=...): oracle.streaming_oracle.StreamOracle (the
model-facing half of the runner) composed with terrain_oracle.step (RTRunner.step's tail) and the history override AS THE DEVICE
DEFINES IT (include/tip_hip.h, tip_stream_history_override): where the leg IK fired, columns 0 .. 107 of the stream's newest history
row are replaced by aa_to_rot6d of the fired pose; root velocity and c_t columns stay.  RTRunner.step does the same thing another way
— it builds the whole row from the corrected copy of the state (real_time_runner.py:483-495) — and tests/test_replay_terrain_cpu.py
holds the two to each other on the reference-generated tests/golden/tip_terrain_loop_golden.npz.

    loop = ClosedLoop(table, s_init, model_last_row, multi_sbp=True)      # model_last_row(x_imu [T, 90], x_s [T, 131]) -> y [131]
    out = loop.step(raw[72])              # None while the smoother primes, else a dict: s_rest, c_t, y_last, root, viz_locs, q_hist, fired
    loop.stream.hist[-1]                  # the newest history row, as the model sees it on the next frame
    make_stream, make_tracker = spec_pair(table, model_last_row)          # the same loop through tip_amd.replay.replay_on_host

It imports nothing of tip_amd."""
import warnings

import numpy as np

import terrain_oracle as to
from oracle.streaming_oracle import StreamOracle, aa_to_rot6d


def override(stream: StreamOracle, q_hist):
    """tip_stream_history_override on a StreamOracle: the pose columns of the newest history row <- the 6D form of q_hist [54]."""
    row = np.array(stream.hist[-1], dtype=np.float64)
    row[:108] = aa_to_rot6d(np.asarray(q_hist, dtype=np.float64))
    stream.hist[-1] = row


class ClosedLoop:
    """One stream: model -> tracker -> IK -> model history -> model.  dtype is the tracker's (fp64: the oracle; float32: the same
    statements in float32); the stream half is StreamOracle's fp64 either way.  rows_f32=True rounds s_rest / c_t to float32 before the
    tracker takes them, as the device's tracker reads the engine's float32 rows."""

    def __init__(self, table, s_init, model_last_row, map_bound=5.0, grid_size=0.1, multi_sbp=True, max_regions=64, dtype=np.float64,
                 window=40, rows_f32=False):
        self.table, self.model, self.f, self.multi = table, model_last_row, dtype, bool(multi_sbp)
        self.G, self.D, self.gs = to.grid_num(map_bound, grid_size), to.diffuse_region(grid_size), grid_size
        s_init = np.asarray(s_init, dtype=np.float64)
        self.stream = StreamOracle(s_init, max_len=window)
        self.state = to.State(table, s_init.astype(dtype), self.G, max_regions, dtype)
        self.trace = to.new_trace()
        self.rows_f32 = rows_f32
        self.row = 0

    def stream_step(self, raw):
        """The model-facing half: None while the smoother primes, else (s_rest [111], c_t [20], y_last [131])."""
        seen = {}

        def model(x_imu, x_s):
            seen["y"] = np.asarray(self.model(x_imu, x_s))
            return seen["y"]

        r = self.stream.step(np.asarray(raw, dtype=np.float64), model)
        self.row += 1
        if r is None:
            return None
        self.y = seen["y"]
        return r[0], r[1], seen["y"]

    def tracker_step(self, s_rest, c_t):
        """RTRunner.step's tail on the row the stream half just produced: (root, viz_locs, q_hist, fired).  No override."""
        if self.f is np.float64 and len(self.stream.outs) < 6:
            # The runner's first five calls filter nothing and work on the model's float32 row itself (StreamOracle.consume), so
            # "prev_root_xyz + root_v * DT" (real_time_runner.py:441) multiplies in float32 there.  The tracker cannot see that from
            # s_rest; put the 1e-9 of it into this step's root_pre from outside: the root moves, the previous poses (kept about the
            # root) move back, so that only root_pre = root + v DT changes.
            v32 = np.asarray(self.y, dtype=np.float32)[108:111]
            delta = (v32 * np.float32(to.DT)).astype(np.float64) - v32.astype(np.float64) * to.DT
            self.state.root = self.state.root + delta
            self.state.pq_prev = self.state.pq_prev.copy()
            self.state.pq_prev[:, :3] -= delta
        if self.rows_f32:
            s_rest, c_t = np.asarray(s_rest).astype(np.float32), np.asarray(c_t).astype(np.float32)
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return to.step(self.table, self.state, s_rest, c_t, self.G, self.D, self.gs, self.multi, self.f, self.trace, self.row)

    def step(self, raw):
        r = self.stream_step(raw)
        if r is None:
            return None
        s_rest, c_t, y = r
        if self.rows_f32:
            s_rest, c_t = s_rest.astype(np.float32), c_t.astype(np.float32)
        root, viz, q_hist, fired = self.tracker_step(s_rest, c_t)
        if fired:
            override(self.stream, q_hist)
        return {"s_rest": np.asarray(s_rest), "c_t": np.asarray(c_t), "y_last": y, "root": root, "viz_locs": viz, "q_hist": q_hist,
                "fired": bool(fired)}


def spec_pair(table, model_last_row, **kw):
    """(make_stream, make_tracker) for tip_amd.replay.replay_on_host: the two halves of one ClosedLoop per slot — the specification
    makes a slot's tracker right after its stream — with the override as the specification applies it (stream.override on fire)."""
    loops = []

    class Stream:
        def __init__(self, s_init_row):
            self.loop = ClosedLoop(table, s_init_row, model_last_row, **kw)
            loops.append(self.loop)

        def step(self, raw):
            return self.loop.stream_step(raw)

        def override(self, q_hist):
            override(self.loop.stream, q_hist)

    class Tracker:
        def __init__(self, s_init_row):
            self.loop = loops.pop()

        def step(self, s_rest, c_t):
            root, viz, q_hist, fired = self.loop.tracker_step(s_rest, c_t)
            return root, viz, q_hist, bool(fired), self.loop.state.off_map, self.loop.state.regions_full

    return Stream, Tracker


BIAS_INDEX, BIAS_SHIFT = (111, 115, 127), 0.5      # the fixture's departure from the synthetic weights: contacts of lankle, rankle, root held


def standing_recording(L, seed):
    """(imu [L, 72] float32, s_init [114] float32) of an upright character: the root sensor upright with a slow yaw, the other five
    turning smoothly, accelerations an AR(1) walk — the kind of recording the closed-loop fixture was made on.  With the contact
    logits shifted by BIAS_SHIFT the synthetic model holds its feet and the leg IK fires within a few frames of the first valid row."""
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(seed)
    base, w, acc = Rotation.random(6, random_state=seed), rng.randn(6, 3) * 0.6, rng.randn(6, 3)
    up = Rotation.from_rotvec([np.pi / 2, 0, 0])
    imu = np.zeros((L, 72))
    for t in range(L):
        acc = 0.9 * acc + 0.6 * rng.randn(6, 3)
        imu[t, :54] = (Rotation.from_rotvec(w * (t / 60.0)) * base).as_matrix().reshape(-1)
        imu[t, :9] = (Rotation.from_rotvec([0, 0, 0.3 * np.sin(2 * np.pi * 0.2 * t / 60.0 + seed)]) * up).as_matrix().reshape(-1)
        imu[t, 54:] = acc.reshape(-1)
    s_init = np.zeros(114)
    s_init[:3] = [0.2 + 0.01 * (seed % 7), -0.1, 0.93]
    s_init[3:6] = up.as_rotvec()
    return imu.astype(np.float32), s_init.astype(np.float32)


def run(table, raw, s_init, model_last_row, **kw):
    """One recording by the script's row conventions (row 0: the start state; the step on frame t fills row t + 1; the last frame is
    never fed): a dict of arrays s_rest [L, 111], c_t [L, 20], valid, y_last [L, 131], root, viz_locs, q_hist, fire, hist [L, 131] (the
    newest history row after the step), off_map, regions_full, and `loop`."""
    raw = np.asarray(raw)
    L = raw.shape[0]
    s_init = np.asarray(s_init, dtype=np.float64)
    loop = ClosedLoop(table, s_init, model_last_row, **kw)
    out = {"s_rest": np.repeat(s_init[None, 3:], L, 0), "c_t": np.zeros((L, 20)), "valid": np.zeros(L, bool),
           "y_last": np.full((L, 131), np.nan), "root": np.repeat(s_init[None, :3], L, 0), "viz_locs": np.full((L, 5, 3), 100.0),
           "q_hist": np.repeat(s_init[None, 3:57], L, 0), "fire": np.zeros(L, bool), "hist": np.zeros((L, 131))}
    out["hist"][0] = loop.stream.hist[-1]
    for t in range(L - 1):
        r = loop.step(raw[t])
        out["hist"][t + 1] = loop.stream.hist[-1]
        if r is None:
            continue
        out["valid"][t + 1] = True
        for k, key in (("s_rest", "s_rest"), ("c_t", "c_t"), ("y_last", "y_last"), ("root", "root"), ("viz_locs", "viz_locs"),
                       ("q_hist", "q_hist"), ("fire", "fired")):
            out[k][t + 1] = r[key]
    out["off_map"], out["regions_full"], out["loop"] = loop.state.off_map, loop.state.regions_full, loop
    return out
