"""Offline replay: recorded IMU files through the closed loop of a compact streaming pool, with no per-frame host traffic.

The reference has no offline mode: offline_testing_simple.py pretends each recorded file is streaming — for every file a fresh
RTRunnerMin and one step per frame (test_run_ours_gpt_v4_with_c_rt_minimal, :109-155; the per-file loop :360-399), one B = 1
forward per frame, one file after the other.  ReplayPool runs a set of recordings of any lengths through ONE
StaggeredStreamingEngine(compact=True): recordings take the pool's slots in turn, and a frame of the pool is a frame of every
recording in flight.

    pool = ReplayPool(model, slots=64, window=40, live_dropout=False, use_graph=True, keep_y=False)
    out = pool.run(recordings, s_init)      # recordings: list of [L_i, 72] float arrays; s_init [R, 114] (the script's s_gt[0] per file)
    out[i].s_rest [L_i, 111]   out[i].c_t [L_i, 20 | 8]   out[i].valid [L_i] bool   out[i].y_last [L_i, 131 | 119] (keep_y=True, else None)
    pool.frames (engine frames run)   pool.restarts (recordings restarted after a lost hand-off)

Row conventions — those of test_run_ours_gpt_v4_with_c_rt_minimal (:123-134):
  - row 0 is the start state: s_init[i, 3:114], c_t = 0, valid False (y_last NaN);
  - the step on imu[t] fills row t + 1, for t = 0 .. L_i - 2; the last frame is never fed, as in the script;
  - the five priming steps (t < 5) give s_init's rest, zero c_t, NaN y_last and valid False — what the runner returns while its
    smoother primes (real_time_runner_minimal.py:125-128);
  - so a recording with L_i <= 6 has no valid row, L_i = 1 runs nothing, and L_i = 0 is a ValueError.
s_rest is s_t[3:114] of the runner (54 axis-angles, root velocity, zeros).  Root translation, FK and the SBP root correction
(real_time_runner_minimal.py:159-194) are a post-pass over this result, also on the device: tip_amd.kinematics.track_replay gives the
script's s_traj_pred rows and viz_locs, kinematics.evaluate its seven metrics; neither touches the pool.  s_rest[:, 54:57] is the root
velocity after the runner's pose averaging (:165-166), not the one :159 integrates: the tracker takes the averaging back out.
trim_like_reference applies the script's shift by IMU_n_smooth + 2 rows (:148-151) to pose rows.

Device side (csrc/tip_replay.hip; include/tip_hip.h: tip_replay_feed, tip_replay_collect): the corpus — every recording's frames
back to back — and the corpus-shaped outputs live in HBM for the whole run, with a per-slot cursor table (cur: corpus row to feed
next, -1 idle; end).  A frame is feed -> the engine's mapped frame -> collect (StaggeredStreamingEngine._step_fed), captured once per
bucket with use_graph=True.  Lengths are known up front, so the whole schedule is (plan_replay): no frame of run() synchronises with
the device or reads anything back, and there is one synchronisation, at the end (the engine's capture of a bucket's frame, on the
bucket's first use in a run, synchronises once as it does for every compact pool).  Attaches and detaches go through the engine's
attach / detach on exactly the frames the plan names, and on those frames the cursor table is uploaded (one small non-blocking copy
from pinned memory, between two replays, in front of the engine's own staged attach copy).

The full runner (terrain=): ReplayPool(model, slots, ..., terrain=dict(skel=..., map_bound=5.0, grid_size=0.1, multi_sbp=True,
max_regions=64)) runs RTRunner.step's tail — terrain map, height correction, leg IK (tip_amd.terrain) — INSIDE the frame, one
TerrainTracker block per slot (pool.tracker), so that the pose the IK corrects reaches the model's history before the next frame as the
reference feeds it back (real_time_runner.py:483-495; live_demo_new.py ships multi_sbp_terrain_and_correction on).  A tracked frame is
feed -> the engine's mapped frame -> tip_replay_mask (valid = the slot produced a row and feeds a recording) -> tip_terrain_track over
the pool's slots -> tip_stream_history_override with the tracker's `fire` as the device slot list -> tip_replay_collect_tracked, all of
it inside the captured ("fed", B) frame: three launches more than the plain frame, nothing read by the host.  run() then returns
TrackedReplayResult per recording: the four arrays above and root [L, 3], viz_locs [L, 5, 3], q_hist [L, 54], fire [L] — row for row
what terrain.track_terrain gives in a post-pass (row 0 and the priming rows: s_init's root and pose, markers at 100, fire False) — and
the recording's off_map / regions_full totals; .qdq is root | s_rest, which trim_like_reference and kinematics.evaluate take.  The
tracker's blocks of the slots a frame attaches are reset from the recordings' s_init in front of that frame (pinned, non-blocking);
no synchronisation is added.  With multi_sbp=False nothing is fed back and the result is the plain pool's plus the post-pass, bit for
bit; RTRunnerMin needs no tracker in the pool (kinematics.track_replay is exact for it).  terrain=None changes nothing.

Model shapes, .train() / .eval() rules and every refusal are the engine's own; the shipped loaders (past_state_dropout = 0.8,
never .eval()) are served with live_dropout=True.

Lost hand-off: the engine re-primes every attached slot and raises TipHandoffError; run() catches it once, restarts the recordings
that were in flight from their frame 0 (their rows are overwritten), counts them in `restarts` and goes on.  The handle has demoted
itself by then, so a second loss is raised to the caller.  A recording that finished before the loss was noticed keeps its rows: a
row computed by the lost launch is NaN, never a finite wrong number — with valid True (ReplayResult: valid is not "finite").  With a
tracker the restarted recordings' blocks are reset as well and their rows, the tracker's included, are overwritten."""
from __future__ import annotations

import collections
import pickle
import random
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

IMU_N_SMOOTH = 5                    # RTRunnerMin.IMU_n_smooth (real_time_runner_minimal.py:34)
TRIM = IMU_N_SMOOTH + 2             # offline_testing_simple.py:149
DT = 1.0 / 60                       # constants.py:7
MIN_FILE_FRAMES = 2.5 / DT          # offline_testing_simple.py:371


class ReplayResult(NamedTuple):
    """One recording's rows.  valid says that a model call produced the row (it is the engine's T > 0), NOT that the row is finite: a
    non-finite input frame gives NaN rows with valid True, as in the live engines, and so does a lost hand-off that is noticed only
    after the recording finished (graph mode polls a host word: one or more frames late) — such a recording is not restarted and
    keeps the NaN rows the lost launch wrote.  A caller that needs finite rows tests np.isfinite(s_rest).all(1) beside valid."""
    s_rest: np.ndarray              # [L, 111] float32
    c_t: np.ndarray                 # [L, 20 | 8] float32
    valid: np.ndarray               # [L] bool
    y_last: Optional[np.ndarray]    # [L, 131 | 119] float32 (keep_y=True), else None


class TrackedReplayResult(NamedTuple):
    """One recording's rows from ReplayPool(terrain=...): ReplayResult's four and the full runner's tail, row for row what
    tip_amd.terrain.track_terrain gives for the recording in a post-pass — row 0 and the priming rows hold s_init's root and pose,
    markers at 100 and fire False.  q_hist is the pose the runner feeds back (s_rest[:, :54] with the columns the leg IK rewrote on
    rows where fire is True); with multi_sbp it HAS gone into the model's history, so s_rest behind a fired row is not the plain
    pool's.  off_map and regions_full are the recording's totals (map updates dropped off the map, or for want of a free region)."""
    s_rest: np.ndarray              # [L, 111] float32
    c_t: np.ndarray                 # [L, 20 | 8] float32
    valid: np.ndarray               # [L] bool
    y_last: Optional[np.ndarray]    # [L, 131 | 119] float32 (keep_y=True), else None
    root: np.ndarray                # [L, 3] float32: RTRunner.step's qdq[:3]
    viz_locs: np.ndarray            # [L, 5, 3] float32
    q_hist: np.ndarray              # [L, 54] float32
    fire: np.ndarray                # [L] bool
    off_map: int
    regions_full: int

    @property
    def qdq(self) -> np.ndarray:
        """[L, 114]: root | s_rest — the script's s_traj_pred rows before its trim, as kinematics.track_replay returns them."""
        return np.concatenate([self.root, self.s_rest], axis=1)


TERRAIN_KEYS = ("skel", "map_bound", "grid_size", "multi_sbp", "max_regions")


class ReplayPlan(NamedTuple):
    frames: list                    # per engine frame: (attaches [(slot, recording), ...], detaches [slot, ...]), applied BEFORE the frame
    n_frames: int                   # engine frames in total (= len(frames))
    final_detach: list              # slots still attached after the last frame
    slot: list                      # per recording: its slot (-1: nothing to run, L = 1)
    start: list                     # per recording: the engine frame that feeds its frame 0 (-1: nothing to run)


def _plan(lengths, slots, order, occupied) -> ReplayPlan:
    """plan_replay's rule on the recordings `order`, with the slots of `occupied` ({slot: recording}) already attached at frame 0 and
    feeding their recording from its frame 0 (no attach is emitted for them)."""
    busy = {int(s): (int(i), lengths[i] - 2) for s, i in occupied.items()}          # slot -> (recording, its last fed engine frame)
    slot_of, start = [-1] * len(lengths), [-1] * len(lengths)
    for s, (i, _) in busy.items():
        slot_of[i], start[i] = s, 0
    queue = collections.deque(i for i in order if lengths[i] > 1)
    frames, f = [], 0
    while True:
        ended = [s for s in sorted(busy) if busy[s][1] < f]
        for s in ended:
            del busy[s]
        att = []
        for s in range(slots):
            if not queue:
                break
            if s not in busy:
                i = queue.popleft()
                busy[s] = (i, f + lengths[i] - 2)
                slot_of[i], start[i] = s, f
                att.append((s, i))
        det = [s for s in ended if s not in busy]
        if not busy:
            return ReplayPlan(frames, len(frames), det, slot_of, start)
        frames.append((att, det))
        f += 1


def plan_replay(lengths: Sequence[int], slots: int) -> ReplayPlan:
    """The schedule of a replay, host only.  Recordings in the given order, each to the free slot of lowest index; a recording of L
    frames feeds L - 1 of them (the last one is never fed), one per engine frame, and a slot takes its next recording on the frame
    after its last fed frame — a re-attach, so the slot keeps its window position.  A slot with nothing left to take is detached on
    that frame (after the last frame: final_detach).  A recording with L = 1 takes no frame and no slot."""
    lengths = [int(n) for n in lengths]
    slots = int(slots)
    if slots < 1:
        raise ValueError(f"tip_amd.replay.plan_replay: slots must be at least 1; got {slots}")
    if any(n < 1 for n in lengths):
        raise ValueError("tip_amd.replay.plan_replay: a recording has at least one frame")
    return _plan(lengths, slots, range(len(lengths)), {})


def trim_like_reference(s_rest: np.ndarray) -> np.ndarray:
    """The script's alignment of a predicted trajectory (offline_testing_simple.py:148-151): rows move up by IMU_n_smooth + 2 = 7 — the
    smoother's delay plus the output filter's — and the last 7 repeat the row in front of them.  Pose rows only ([L, any width]): the
    script leaves c_t untrimmed.  Returns a new array.  L <= 7 leaves no row to repeat: the script's line :151 raises IndexError there
    (it never sees such a file: :371 skips anything under 150 frames); here it is a ValueError."""
    s = np.array(s_rest, copy=True)
    if s.ndim < 1 or s.shape[0] <= TRIM:
        raise ValueError(f"tip_amd.replay.trim_like_reference: the trim drops {TRIM} rows; a trajectory of {s.shape[0] if s.ndim else 0} "
                         "rows has none left")
    s[0:-TRIM] = s[TRIM:]
    s[-TRIM:] = s[-TRIM - 1]
    return s


def recordings_from_files(paths, test_len: int, seed=None):
    """The script's file handling (offline_testing_simple.py:366-387), host only: unpickle each file (keys 'imu' [L, 72] and
    'nimble_qdq' [L, 114]), skip files shorter than 2.5 / DT = 150 frames, crop longer ones to test_len frames from a
    random.randrange start (one generator seeded with `seed` for the whole list, drawn from in file order, as the script's module
    generator is), and lift the root by 5 cm (Y[:, 2] += 0.05).  Returns (recordings, s_init): the IMU arrays as float32 and the
    first qdq row of each kept file, [R, 114] float32 — what ReplayPool.run takes.  Missing files are the caller's business."""
    rng = random.Random(seed)
    recs, s0 = [], []
    for p in paths:
        with open(p, "rb") as fh:
            data = pickle.load(fh)
        X, Y = np.asarray(data["imu"]), np.array(data["nimble_qdq"], dtype=np.float64)
        if Y.shape[0] < MIN_FILE_FRAMES:
            continue
        if Y.shape[0] > test_len:
            start = rng.randrange(0, Y.shape[0] - test_len)
            end = start + test_len
        else:
            start, end = 0, Y.shape[0]
        X, Y = X[start:end, :], Y[start:end, :]
        Y[:, 2] += 0.05
        recs.append(np.ascontiguousarray(X, dtype=np.float32))
        s0.append(Y[0].astype(np.float32))
    return recs, (np.stack(s0) if s0 else np.zeros((0, 114), dtype=np.float32))


def check_inputs(recordings, s_init):
    """(recordings as contiguous float32 [L_i, 72] arrays, s_init as float32 [R, 114]); ValueError for anything else."""
    try:
        recs = [np.ascontiguousarray(r, dtype=np.float32) for r in recordings]
    except (TypeError, ValueError):
        raise ValueError("tip_amd.replay: recordings is a list of [L_i, 72] float arrays") from None
    if not recs:
        raise ValueError("tip_amd.replay: no recordings")
    for i, r in enumerate(recs):
        if r.ndim != 2 or r.shape[1] != 72:
            raise ValueError(f"tip_amd.replay: recording {i} is {r.shape}; a recording is [L, 72] (six IMUs: rotations, then accelerations)")
        if r.shape[0] == 0:
            raise ValueError(f"tip_amd.replay: recording {i} has no frames")
    s = np.ascontiguousarray(s_init, dtype=np.float32)
    if s.ndim == 1:
        s = s[None]
    if s.ndim != 2 or s.shape != (len(recs), 114):
        raise ValueError(f"tip_amd.replay: s_init is [R, 114] (q, dq: one start state per recording); got {s.shape} for {len(recs)} recordings")
    return recs, s


def replay_on_host(recordings, s_init, slots: int, make_stream, n_c: int = 20, n_y: int = 131, make_tracker=None):
    """ReplayPool.run's bookkeeping — the plan, the cursor tables, what the feed and collect kernels do with them — in plain numpy, with
    the device's per-slot closed loop replaced by make_stream(s_init_row) -> an object whose step(raw[72]) returns None while it primes
    and (s_rest[111], c_t[n_c], y_last[n_y]) afterwards (oracle.streaming_oracle.StreamOracle with a model bound in is one).  A
    SPECIFICATION, not the code path: ReplayPool.run shares plan_replay and check_inputs with it and nothing else — the cursor tables,
    feed and collect it restates run on the device there (csrc/tip_replay.hip), and only the GPU tests check those.  It exists so that
    the row conventions can be held against the script's loop without a device; returns (results, frames).
    make_tracker (ReplayPool(terrain=...)'s frame): make_tracker(s_init_row) -> an object whose step(s_rest[111], c_t[n_c]) returns
    (root[3], viz_locs[5, 3], q_hist[54], fired, off_map, regions_full) — one per slot, made anew whenever the slot takes a recording.
    It is stepped on every row a stream produced; where it fired, stream.override(q_hist) puts the pose into the stream's newest
    history row before the next frame; the results are TrackedReplayResult."""
    recs, s0 = check_inputs(recordings, s_init)
    lengths = [r.shape[0] for r in recs]
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    n_rows = int(offs[-1])
    corpus = np.concatenate(recs)
    s_out, c_out = np.zeros((n_rows, 111), np.float32), np.zeros((n_rows, n_c), np.float32)
    y_out, valid = np.full((n_rows, n_y), np.nan, np.float32), np.zeros(n_rows, bool)
    s_out[offs[:-1]] = s0[:, 3:]
    tracked = make_tracker is not None
    if tracked:
        root_out, viz_out = np.zeros((n_rows, 3), np.float32), np.full((n_rows, 5, 3), 100.0, np.float32)
        q_out, fire_out, cnt_out = np.zeros((n_rows, 54), np.float32), np.zeros(n_rows, bool), np.zeros((n_rows, 2), np.int32)
        root_out[offs[:-1]], q_out[offs[:-1]] = s0[:, :3], s0[:, 3:57]
    plan = plan_replay(lengths, slots)
    cur, end = np.full(slots, -1, np.int64), np.full(slots, -1, np.int64)
    stream, tracker = [None] * slots, [None] * slots
    for att, det in plan.frames:
        for s in det:
            stream[s] = None
        for s, i in att:
            stream[s] = make_stream(s0[i])
            tracker[s] = make_tracker(s0[i]) if tracked else None
            cur[s], end[s] = offs[i], offs[i] + lengths[i] - 1
        raw = np.zeros((slots, 72), np.float32)                      # feed
        live = cur >= 0
        raw[live] = corpus[cur[live]]
        res = [stream[s].step(raw[s]) if stream[s] is not None else None for s in range(slots)]      # the engine's frame
        trk = [None] * slots
        if tracked:                                                  # the terrain step and the override, for the slots that are valid
            for s in range(slots):
                if res[s] is not None and cur[s] >= 0:
                    trk[s] = tracker[s].step(res[s][0], res[s][1])
                    if trk[s][3]:
                        stream[s].override(np.asarray(trk[s][2]))
        for s in range(slots):                                       # collect
            c = cur[s]
            if c < 0:
                continue
            if res[s] is None:
                s_out[c + 1], c_out[c + 1], y_out[c + 1], valid[c + 1] = s_out[c], 0.0, np.nan, False
                if tracked:
                    root_out[c + 1], viz_out[c + 1], q_out[c + 1], fire_out[c + 1], cnt_out[c + 1] = root_out[c], 100.0, q_out[c], False, cnt_out[c]
            else:
                s_out[c + 1], c_out[c + 1], y_out[c + 1] = res[s]
                valid[c + 1] = True
                if tracked:
                    root_out[c + 1], viz_out[c + 1], q_out[c + 1], fire_out[c + 1] = trk[s][:4]
                    cnt_out[c + 1] = trk[s][4:6]
            cur[s] = -1 if c + 1 >= end[s] else c + 1
    assert (cur < 0).all()
    if tracked:
        return _split_tracked(offs, s_out, c_out, valid, y_out, root_out, viz_out, q_out, fire_out, cnt_out), plan.n_frames
    return _split(offs, s_out, c_out, valid, y_out), plan.n_frames


def _split(offs, s_out, c_out, valid, y_out) -> List[ReplayResult]:
    return [ReplayResult(s_out[a:b], c_out[a:b], valid[a:b], None if y_out is None else y_out[a:b])
            for a, b in zip(offs[:-1], offs[1:])]


def _split_tracked(offs, s_out, c_out, valid, y_out, root, viz, q_hist, fire, counters) -> List[TrackedReplayResult]:
    return [TrackedReplayResult(s_out[a:b], c_out[a:b], valid[a:b], None if y_out is None else y_out[a:b], root[a:b], viz[a:b],
                                q_hist[a:b], fire[a:b].astype(bool), int(counters[b - 1, 0]), int(counters[b - 1, 1]))
            for a, b in zip(offs[:-1], offs[1:])]


class ReplayPool:
    """See the module's docstring.  One StaggeredStreamingEngine(compact=True) with `slots` slots, owned by the pool (`engine`) and
    reused by every run(); window, live_dropout and use_graph are the engine's.  keep_y=True also returns the model's raw last rows.
    terrain=dict(skel=..., map_bound=..., grid_size=..., multi_sbp=..., max_regions=64) puts the full runner's tail into the frame
    (`tracker`: a TerrainTracker of `slots` blocks) and makes run() return TrackedReplayResult; unknown keys, a missing skel,
    multi_sbp with a two-SBP model or with leg chains the IK cannot serve are ValueErrors before anything is built.
    After a run: frames, restarts, and plan (the run's ReplayPlan: which slot and engine frame each recording started on)."""

    def __init__(self, model, slots: int = 64, window: int = 40, live_dropout: bool = False, use_graph: bool = True, keep_y: bool = False,
                 terrain=None):
        import torch
        from . import lib as _lib
        from .streaming import StaggeredStreamingEngine, stream_shape
        slots = int(slots)
        if slots < 1:
            raise ValueError(f"tip_amd.replay.ReplayPool: slots must be at least 1; got {slots}")
        if terrain is not None:          # every refusal before anything is allocated or launched
            from .terrain import _leg_chains_ok
            terrain = dict(terrain)
            extra = set(terrain) - set(TERRAIN_KEYS)
            if extra or terrain.get("skel") is None:
                raise ValueError("tip_amd.replay.ReplayPool: terrain is dict(skel=..., map_bound=..., grid_size=..., multi_sbp=..., "
                                 f"max_regions=...) with a skeleton; got {sorted(terrain)}")
            if terrain.get("multi_sbp"):
                if stream_shape(model)[0] != 5:
                    raise ValueError("tip_amd.replay.ReplayPool: terrain multi_sbp corrects by the root's SBP, which a two-SBP model "
                                     "does not have (tip_amd.terrain's rule)")
                if not _leg_chains_ok(terrain["skel"]):
                    raise ValueError("tip_amd.replay.ReplayPool: terrain multi_sbp needs both ankles below three spherical links "
                                     "(hip, knee, ankle)")
        self.slots, self.keep_y = slots, bool(keep_y)
        self.engine = StaggeredStreamingEngine(model, np.zeros((slots, 114), dtype=np.float32), use_graph=use_graph, compact=True,
                                               live_dropout=live_dropout, window=window)
        self.engine.detach(range(slots))          # (an engine is born with every slot attached; a pool is at rest between runs)
        self.lib = _lib.load()
        self._handoff_error = _lib.TipHandoffError
        self._torch = torch
        # cur (row 0) and end (row 1), one entry per slot: where the captured frames read them, for the pool's lifetime
        self._tbl = torch.full((2, slots), -1, dtype=torch.int64, device=self.engine.device)
        self._bufs = None           # the current run's corpus and outputs (what the engine's captured frames point at)
        self.frames = self.restarts = 0
        # terrain: the full runner's tail inside the frame — one TerrainTracker block per slot, stepped, fed back and collected by the
        # collect callable (_install), all of it inside the captured ("fed", B) frame
        self.tracker = None
        if terrain is not None:
            from .terrain import TerrainTracker
            skel = terrain.pop("skel")
            self.tracker = TerrainTracker(skel, slots, self.engine.device, **terrain)
            self._mask = torch.zeros(slots, dtype=torch.uint8, device=self.engine.device)

    # ---- the two launches around the engine's frame ----------------------------------------------------------------------------------
    def _install(self, corpus, s_out, c_out, y_out, valid, tracked=()):
        """tracked: a pool with a tracker passes its corpus-shaped (root_out, viz_out, q_hist_out, fire_out, counters_out)."""
        eng, lib, n, n_rows = self.engine, self.lib, self.slots, int(corpus.shape[0])
        cur, end = self._tbl[0].data_ptr(), self._tbl[1].data_ptr()
        p_corpus, p_raw = corpus.data_ptr(), eng.raw.data_ptr()
        p_out = (s_out.data_ptr(), c_out.data_ptr(), None if y_out is None else y_out.data_ptr(), valid.data_ptr())
        p_eng = (eng.s_rest.data_ptr(), eng.c_t.data_ptr(), eng.y_slot.data_ptr(), eng.rows_slot.data_ptr())

        def feed():
            eng._check(lib.tip_replay_feed(p_corpus, n_rows, cur, n, p_raw, eng._stream()))

        def collect():
            eng._check(lib.tip_replay_collect(cur, end, n, n_rows, *p_eng, eng.ns, *p_out, eng._stream()))

        if tracked:
            # the terrain step over the pool's slots (valid: the mask launch), the history override for the slots that fired (the
            # tracker's `fire` as the device slot list) and the tracked collect: three launches more, nothing read by the host
            tt = self.tracker
            p_trk = (tt.root.data_ptr(), tt.viz_locs.data_ptr(), tt.q_hist.data_ptr(), tt.fire.data_ptr(), tt._s.buf.data_ptr(), tt._s.stride)
            p_new = tuple(t.data_ptr() for t in tracked)
            frame = {"s_rest": eng.s_rest, "c_t": eng.c_t, "valid": self._mask}

            def collect_tracked():
                eng._check(lib.tip_replay_mask(cur, p_eng[3], n, self._mask.data_ptr(), eng._stream()))
                tt.step(frame)
                tt.feed_back(eng)
                eng._check(lib.tip_replay_collect_tracked(cur, end, n, n_rows, *p_eng, eng.ns, *p_out, *p_trk, *p_new, eng._stream()))

        self._bufs = (corpus, s_out, c_out, y_out, valid) + tuple(tracked)
        eng.set_feeder(feed, collect_tracked if tracked else collect)

    def _reset_tracker(self, pairs, s0, scales=None):
        """The tracker's blocks of the slots in `pairs` [(slot, recording), ...] start over from the recordings' s_init (pinned,
        non-blocking: TerrainTracker.reset) and, with scales, take the recordings' body scales, in stream order before the next frame."""
        if self.tracker is not None and pairs:
            pairs = sorted(pairs)
            kw = {} if scales is None else {"scales": scales[[i for _, i in pairs]]}
            self.tracker.reset([s for s, _ in pairs], s0[[i for _, i in pairs]], **kw)

    def _upload_table(self, in_flight, f, offs, lengths):
        """The cursor table as it stands before engine frame f — in_flight: {slot: (recording, the frame that fed its frame 0)} — in one
        non-blocking copy from pinned memory.  The device advances the cursors itself; the schedule is known, so the host knows them."""
        t = np.full((2, self.slots), -1, dtype=np.int64)
        for s, (i, f0) in in_flight.items():
            t[0, s], t[1, s] = offs[i] + (f - f0), offs[i] + lengths[i] - 1
        self._tbl.copy_(self._torch.from_numpy(t).pin_memory(), non_blocking=True)

    def run(self, recordings, s_init, scales=None) -> list:
        """scales [R] (pools with terrain= only): the recordings' body scales (tip_amd.kinematics.scale_of_height).  A recording's scale
        goes to its slot's block with the reset the pool issues at the recording's attach frame, and again on a restart after a lost
        hand-off; the captured frame reads the tracker's scale array where it lies, so a frame has no launch more and a run still one
        synchronisation.  scales=None is the unscaled frame."""
        recs, s0 = check_inputs(recordings, s_init)
        if scales is not None:          # refused before anything is allocated or launched
            from .kinematics import check_scales
            if self.tracker is None:
                raise ValueError("tip_amd.replay.ReplayPool.run: scales are the body scales the pool's tracker runs FK with; this pool "
                                 "has none (ReplayPool(terrain=dict(skel=..., ...)))")
            scales = check_scales(scales, len(recs), "replay.ReplayPool.run")
        torch = self._torch
        eng, n, dev = self.engine, self.slots, self.engine.device
        lengths = [r.shape[0] for r in recs]
        offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        n_rows = int(offs[-1])
        self.frames = self.restarts = 0
        fed0 = eng.fed_frames
        with torch.cuda.device(dev), torch.no_grad():
            # every slot detached and at rest, graphs of the previous run dropped
            eng.detach([i for i in range(n) if eng.attached[i]])
            eng.reset()
            if scales is None and self.tracker is not None:
                self.tracker._unscaled()          # (after a run with scales: back to the unscaled entries before the frame is captured)
            corpus = torch.from_numpy(np.concatenate(recs)).pin_memory().to(dev, non_blocking=True)
            s_out = torch.zeros((n_rows, 111), dtype=torch.float32, device=dev)
            c_out = torch.zeros((n_rows, eng.nc), dtype=torch.float32, device=dev)
            y_out = torch.full((n_rows, eng.ns), float("nan"), dtype=torch.float32, device=dev) if self.keep_y else None
            valid = torch.zeros(n_rows, dtype=torch.uint8, device=dev)
            # row 0 of every recording: its start state (what the priming rows repeat)
            start_rows = torch.from_numpy(offs[:-1].copy()).pin_memory().to(dev, non_blocking=True)
            s_out.index_copy_(0, start_rows, torch.from_numpy(s0[:, 3:].copy()).pin_memory().to(dev, non_blocking=True))
            tracked = ()
            if self.tracker is not None:
                # the tracker's corpus-shaped rows; row 0 of every recording is the host's: s_init's root and pose, markers at 100
                root_out = torch.zeros((n_rows, 3), dtype=torch.float32, device=dev)
                viz_out = torch.full((n_rows, 5, 3), 100.0, dtype=torch.float32, device=dev)
                q_out = torch.zeros((n_rows, 54), dtype=torch.float32, device=dev)
                fire_out = torch.zeros(n_rows, dtype=torch.uint8, device=dev)
                cnt_out = torch.zeros((n_rows, 2), dtype=torch.int32, device=dev)
                head = torch.from_numpy(s0[:, :57].copy()).pin_memory().to(dev, non_blocking=True)
                root_out.index_copy_(0, start_rows, head[:, :3].contiguous())
                q_out.index_copy_(0, start_rows, head[:, 3:].contiguous())
                tracked = (root_out, viz_out, q_out, fire_out, cnt_out)
            self._install(corpus, s_out, c_out, y_out, valid, tracked)

            plan = plan_replay(lengths, n)
            self.plan = plan
            in_flight, done_attach = {}, set()          # slot -> (recording, frame of its frame 0); recordings attached so far
            caught, f = False, 0                        # (frame 0 attaches, so it uploads the whole table: nothing of an earlier run stays)
            while f < plan.n_frames:
                att, det = plan.frames[f]
                if det:
                    eng.detach(det)
                    for s in det:
                        del in_flight[s]
                if att:
                    eng.attach([s for s, _ in att], s0[[i for _, i in att]])
                    for s, i in att:
                        in_flight[s] = (i, f)
                        done_attach.add(i)
                # (a slot whose recording ended and that takes no other was detached above; one that takes another was overwritten)
                in_flight = {s: v for s, v in in_flight.items() if f - v[1] < lengths[v[0]] - 1}
                if att:
                    self._upload_table(in_flight, f, offs, lengths)
                    self._reset_tracker(att, s0, scales)
                try:
                    eng._step_fed()
                except self._handoff_error:
                    if caught:
                        raise
                    # the engine re-primed every attached slot from the s_init it was attached with: those recordings start over
                    caught = True
                    self.restarts += len(in_flight)
                    occupied = {s: i for s, (i, _) in in_flight.items()}
                    plan = _plan(lengths, n, [i for i in range(len(recs)) if i not in done_attach], occupied)
                    in_flight, f = {s: (i, 0) for s, i in occupied.items()}, 0
                    self._upload_table(in_flight, 0, offs, lengths)
                    self._reset_tracker(list(occupied.items()), s0, scales)
                    continue
                f += 1
            eng.detach(plan.final_detach)
            torch.cuda.current_stream(dev).synchronize()          # the one synchronisation
            self.frames = eng.fed_frames - fed0
            y_host = None if y_out is None else y_out.cpu().numpy()
            if self.tracker is not None:
                return _split_tracked(offs, s_out.cpu().numpy(), c_out.cpu().numpy(), valid.cpu().numpy().astype(bool), y_host,
                                      root_out.cpu().numpy(), viz_out.cpu().numpy(), q_out.cpu().numpy(), fire_out.cpu().numpy(),
                                      cnt_out.cpu().numpy())
            return _split(offs, s_out.cpu().numpy(), c_out.cpu().numpy(), valid.cpu().numpy().astype(bool), y_host)
