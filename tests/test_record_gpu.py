"""GPU tests of the session recorder (csrc/tip_record.hip; tip_amd.record.SessionRecorder).  The recorder copies rows and counts them:
every comparison here is bit for bit — against the numpy restatement of the page machine (tests/record_oracle.py), against clones the
test takes of the engine's buffers, and against the replay of the recorded frames."""
import gc
import os
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch

import record_oracle as ro
import sensor_oracle as so
import tip_amd
from tip_amd import record, replay, sensors, synth
from test_host_cpu import make_model, load_synth

pytestmark = pytest.mark.gpu
f32 = np.float32
S = tip_amd.streaming
_models = {}


def _model():
    if "m" not in _models:
        m = make_model(dict(synth.PAPER))
        load_synth(m, dict(synth.PAPER), 0)
        _models["m"] = m.cuda().eval()
    return _models["m"]


@pytest.fixture(autouse=True)
def _leave_nothing_behind():
    """What a test here drops — recorders with pinned buffers and events, engines and a replay pool with captured graphs, some of it in
    reference cycles — is collected when the test ends, so that no later test's graph capture finds it."""
    yield
    gc.collect()


@pytest.fixture
def fused():
    m = _model()
    m.set_plan("fused")
    yield m
    m.set_plan("auto")


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


# ---- 1. append against the oracle ---------------------------------------------------------------------------------------------------------
WIDTHS = {72: [72], 191: [72, 111, 8], 203: [72, 111, 20], 8: [8]}


def _sources(n, widths, layout="dense"):
    """Static source tensors of the given widths.  layout: "dense"; "odd-stride" — the first source is a column slice of a [n, w + 3]
    tensor (a row stride that is no multiple of 4 floats); "offset" — a column slice that starts 8 bytes into 16-byte aligned rows."""
    src = OrderedDict()
    for k, w in enumerate(widths):
        if k == 0 and layout == "odd-stride":
            src["s0"] = torch.zeros((n, w + 3), device="cuda")[:, :w]
        elif k == 0 and layout == "offset":
            src["s0"] = torch.zeros((n, w + 8), device="cuda")[:, 2: 2 + w]
        else:
            src[f"s{k}"] = torch.zeros((n, w), device="cuda")
    return src


def _schedule(rng, n, F):
    """Ragged opens and closes: per frame a few slots change state; the lists also carry -1 and n now and then."""
    is_open, script = [False] * n, {}
    for f in range(F):
        ops = []
        if f == 0 or rng.rand() < 0.35:
            pick = [s for s in rng.permutation(n)[: max(1, n // 3)] if not is_open[s]]
            if pick or f == 0:
                pick = pick or [0]
                for s in pick:
                    is_open[s] = True
                ops.append(("open", [int(s) for s in pick] + ([-1, n] if rng.rand() < 0.5 else [])))
        if f > 2 and rng.rand() < 0.25:
            pick = [int(s) for s in rng.permutation(n)[: max(1, n // 4)]]          # (open or not: closing a closed slot does nothing)
            for s in pick:
                is_open[s] = False
            ops.append(("close", pick + ([n] if rng.rand() < 0.5 else [])))
        script[f] = ops
    return script


def _drive(rec, machine, src, script, F, drain_every, rng, valid_min=1):
    """The same schedule on the recorder and on the oracle; returns {name: session id of the oracle}."""
    n, W = rec.n, rec.width
    data = rng.randn(F, n, W).astype(f32)
    data[:, :, 0] = np.arange(F)[:, None]                          # column 0: the frame; column 1: the slot
    data[:, :, 1 % W] = np.arange(n)[None, :] if W > 1 else data[:, :, 0]
    mask = (rng.rand(F, n) < 0.7).astype(np.int32) * rng.randint(1, 41, size=(F, n)).astype(np.int32) + (valid_min - 1)
    d_data, d_mask = torch.from_numpy(data).cuda(), torch.from_numpy(mask).cuda()
    names, sid = {}, 0
    for f in range(F):
        for what, slots in script.get(f, ()):
            if what == "open":
                inside = [s for s in slots if 0 <= s < n]
                ids, nm = [], []
                for s in slots:
                    if 0 <= s < n:
                        sid += 1
                        ids.append(sid)
                        nm.append(f"w{sid}")
                        names[f"w{sid}"] = sid
                    else:
                        ids.append(0)
                        nm.append(f"out{f}_{s}")
                rec.open(slots, s_init_rows=np.full((len(slots), 114), f, f32), names=nm)
                machine.open(slots, ids)
                assert inside
            else:
                rec.close(slots)
                machine.close(slots)
        at = 0
        for t in src.values():
            t.copy_(d_data[f, :, at: at + t.shape[1]])
            at += t.shape[1]
        rec.valid.copy_(d_mask[f])
        rec.step()
        machine.append(data[f], mask[f], valid_min)
        if drain_every and f % drain_every == drain_every - 1:
            rec.drain()
            machine.drain(rec.staging_pages)
    return names


def _finish(rec, machine):
    rec.close(list(range(rec.n)))
    machine.close(list(range(rec.n)))
    rec.drain(wait=True)
    machine.drain(rec.staging_pages)
    while rec.queued:
        rec.drain(wait=True)
        machine.drain(rec.staging_pages)


def _same_as_truth(rec, machine, names):
    got = {s.name: s for s in rec.sessions()}
    assert set(got) == set(names)
    for name, sid in names.items():
        rows, gaps, dropped = machine.truth[sid].final()
        s = got[name]
        assert s.closed and s.complete, name
        assert s.slot == machine.truth[sid].slot and s.rows.shape == rows.shape and np.array_equal(_bits(s.rows), _bits(rows)), name
        assert s.gaps == gaps and s.dropped == dropped, (name, s.gaps, gaps)
    assert rec.counters(wait=True) == machine.totals()
    assert rec.guards_intact()


GRID = [(n, R, W) for n in (1, 5, 70) for R in (1, 3, 64) for W in (72, 191, 203, 8)]
EXTRA = [(5, 3, 72, "odd-stride"), (5, 3, 72, "offset"), (70, 64, 203, "odd-stride")]


@pytest.mark.parametrize("case", list(range(len(GRID) + len(EXTRA))))
def test_append_equals_the_oracle(case):
    """72 and 8 take the 16-byte path, 191 and 203 (odd widths) the 4-byte one, and so does a 72-wide source whose row stride is no
    multiple of 4 floats or whose rows start off a 16-byte boundary.  10 .. 140 frames of ragged open / close, a valid mask that
    changes every frame, lists that carry -1 and n, drains every 1 or 7 frames or never until the end: every session's rows, gap list
    and counters equal the oracle's, and the sentinel bytes around the state and staging buffers are untouched."""
    n, R, W, layout = (GRID[case] + ("dense",)) if case < len(GRID) else EXTRA[case - len(GRID)]
    rng = np.random.RandomState(100 + case)
    F = (10, 37, 64, 140)[case % 4] if n < 70 else (10, 33, 66)[case % 3]
    drain_every = (1, 7, 0)[(case // 4 + case) % 3]
    script = _schedule(rng, n, F)
    # ample (running dry is the next test's): a slot's full pages, one partly filled, and one for every session that a close leaves
    # on the queue until the next drain
    pages = n * (F // R + 2) + sum(len(slots) for ops in script.values() for what, slots in ops if what == "open")
    src = _sources(n, WIDTHS[W], layout)
    valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    rec = record.SessionRecorder(n, "cuda", src, pages=pages, page_rows=R, staging_pages=max(1, pages // 3), valid=valid)
    assert rec.width == W
    machine = ro.RecordOracle(n, pages, R, W)
    names = _drive(rec, machine, src, script, F, drain_every, rng)
    _finish(rec, machine)
    _same_as_truth(rec, machine, names)
    assert sum(len(s) for s in rec.sessions()) > 0 and not any(s.dropped for s in rec.sessions())


def test_valid_min_zero_reads_an_array_of_t_minus_one():
    """The engines keep T - 1 per slot (-1: priming or detached): valid_min = 0 appends exactly where T > 0."""
    n, R, W = 5, 3, 8
    src = _sources(n, [W])
    valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    rec = record.SessionRecorder(n, "cuda", src, pages=64, page_rows=R, valid=valid, valid_min=0)
    machine = ro.RecordOracle(n, 64, R, W)
    rng = np.random.RandomState(5)
    names = _drive(rec, machine, src, {0: [("open", [0, 1, 2, 3, 4])]}, 12, 4, rng, valid_min=0)
    _finish(rec, machine)
    _same_as_truth(rec, machine, names)


# ---- 2. exhaustion -----------------------------------------------------------------------------------------------------------------------
def test_a_dry_pool_drops_and_counts_and_resumes_after_a_drain():
    """3 pages of 5 rows, 5 open slots, no drain for 10 frames.  Slot k is valid from frame k on, so slots 0, 1, 2 take the three pages
    and fill them; slots 3 and 4 never get one, and from frame 5 on nobody does: every such row is counted, none is written.  The
    drain behind frame 9 frees three pages: slots 0, 3, 4 take them (the mask keeps the others out, so that as many ask as are free)
    and each session's first row behind the gap is reported at the right place; then slots 1 and 2 likewise.  (With fewer pages free
    than slots asking in one frame the device does not define who gets one — the oracle refuses such a schedule.)"""
    n, R, W = 5, 5, 8
    src = _sources(n, [W])
    valid = torch.zeros(n, dtype=torch.int32, device="cuda")
    rec = record.SessionRecorder(n, "cuda", src, pages=3, page_rows=R, staging_pages=3, valid=valid)
    machine = ro.RecordOracle(n, 3, R, W)
    F = 20
    mask = np.zeros((F, n), np.int32)
    for f in range(F):
        mask[f] = [f >= k for k in range(n)] if f < 10 else ([1, 0, 0, 1, 1] if f < 15 else [0, 1, 1, 0, 0])
    data = np.zeros((F, n, W), f32)
    data[:, :, 0], data[:, :, 1] = np.arange(F)[:, None], np.arange(n)[None, :]
    data[:, :, 2:] = np.random.RandomState(3).randn(F, n, W - 2)
    d_data, d_mask = torch.from_numpy(data).cuda(), torch.from_numpy(mask).cuda()
    rec.open(range(n), names=[f"w{k + 1}" for k in range(n)])
    machine.open(range(n), [k + 1 for k in range(n)])
    for f in range(F):
        src["s0"].copy_(d_data[f])
        valid.copy_(d_mask[f])
        rec.step()
        machine.append(data[f], mask[f])
        if f == 9:
            c = rec.counters(wait=True)
            assert c == machine.totals() and c["rows_written"] == 15 and c["pages_in_use"] == 3
            assert c["rows_dropped"] == 7 + 6 + 5 + 4 + 3                        # slots 3, 4 from their first frame; 0, 1, 2 once full
        if f in (9, 15):
            rec.drain()
            assert machine.drain(3)[3] == 0
    _finish(rec, machine)
    _same_as_truth(rec, machine, {f"w{k + 1}": k + 1 for k in range(n)})
    got = {s.slot: s for s in rec.sessions()}
    for k, s in got.items():                                                     # no row of one slot ever appears in another's session
        assert (s.rows[:, 1] == k).all() and np.array_equal(_bits(s.rows), _bits(data[s.rows[:, 0].astype(int), k]))
    assert got[3].gaps == [(0, 7)] and got[3].rows[0, 0] == 10 and len(got[3]) == 5 and got[3].dropped == 7
    assert got[0].gaps == [(5, 5)] and got[0].rows[:, 0].tolist() == [0, 1, 2, 3, 4, 10, 11, 12, 13, 14]
    assert got[1].rows[:, 0].tolist() == [1, 2, 3, 4, 5, 16, 17, 18, 19] and got[1].gaps == [(5, 5)] and got[1].dropped == 5


# ---- 3. captured ---------------------------------------------------------------------------------------------------------------------------
def test_step_captures_into_a_graph():
    """step() has static arguments: inside a torch.cuda.graph capture — behind the kernels that produce the frame's rows — and replayed
    50 times it files the sessions that 50 launches file on identical source contents."""
    n, R = 5, 4
    out = []
    for captured in (False, True):
        src = _sources(n, [72, 111, 8])
        valid = torch.ones(n, dtype=torch.int32, device="cuda")
        rec = record.SessionRecorder(n, "cuda", src, pages=80, page_rows=R, valid=valid)
        for k, t in enumerate(src.values()):
            t.copy_(torch.arange(t.numel(), device="cuda").reshape(t.shape) * 0.25 + k)

        def frame():
            for t in src.values():
                t.mul_(1.0009765625).add_(0.5)
            valid.add_(1).remainder_(4)                                           # (slots skip every fourth frame)
            rec.step()

        rec.open([0, 2, 3, -1], names=["a", "b", "c", "x"])
        frame()                                                                   # (both ways: one plain frame first)
        if captured:
            g = torch.cuda.CUDAGraph()
            steps = rec.steps
            gc.collect()
            gc.disable()                                                          # (no finalizer of a dead cycle inside the capture)
            try:
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    frame()
            finally:
                gc.enable()
            assert rec.steps == steps + 1                                         # (captured, not run)
        for f in range(50):
            if f == 20:
                rec.open([4], names=["d"])
                rec.close([0])
            g.replay() if captured else frame()
            if f % 7 == 6:
                rec.drain()
        rec.close(range(n))
        rec.drain(wait=True)
        assert rec.guards_intact() and rec.queued == 0
        out.append({s.name: s for s in rec.sessions()})
    a, b = out
    assert set(a) == set(b) == {"a", "b", "c", "d"}
    for k in a:
        assert a[k].complete and b[k].complete and len(a[k]) > 10 and a[k].gaps == b[k].gaps == []
        assert a[k].rows.shape == b[k].rows.shape and np.array_equal(_bits(a[k].rows), _bits(b[k].rows)), k
    assert len(a["b"]) == 38 and len(a["a"]) == 16


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------------------
def _imu_frames(n, F, seed):
    rng = np.random.RandomState(seed)
    raw = rng.randn(F, n, 72).astype(f32)
    raw[:, :, :54] = np.tile(np.eye(3, dtype=f32).reshape(9), 6) + 0.05 * raw[:, :, :54]
    return raw, (rng.randn(n, 114) * 0.2).astype(f32)


def _wearer_rows(clones, slot):
    """(imu, s_rest, c_t) of the frames on which `slot` was valid, from the test's own per-frame clones."""
    keep = [f for f, c in enumerate(clones) if bool(c["valid"][slot])]
    return keep, tuple(torch.stack([clones[f][k][slot] for f in keep]).cpu().numpy() for k in ("raw", "s_rest", "c_t"))


def test_a_live_pool_records_what_it_served_and_the_replay_agrees(fused, tmp_path):
    """A compact pool of 4 on the pinned fused plan, captured frames; wearer A in slot 2 from frame 0 to 49, wearer B in slot 0 from
    frame 9 on; 70 frames.  (a) Each session's imu rows are the clones of engine.raw[slot] at the slot's valid frames and its pose rows
    the returned s_rest / c_t, bit for bit.  (b) The .pkl files load; the full IMU sequences — priming frames included — replayed through
    ReplayPool(slots=2) on the same plan give, on their valid rows (row t + 1 is the step on frame t), the recorded pose rows bit for bit."""
    m = fused
    F = 70
    raw, s_init = _imu_frames(4, F, 23)
    eng = S.StaggeredStreamingEngine(m, np.zeros((4, 114), f32), compact=True, use_graph=True)
    eng.detach(range(4))
    eng.reset()
    rec = record.SessionRecorder.for_engine(eng, page_rows=8)
    assert list(rec.sources) == ["raw", "s_rest", "c_t"] and rec.width == 203 and rec.valid is eng.rows_slot and rec.valid_min == 0
    wearers = {"A": (2, 0, 50), "B": (0, 9, F)}                                   # slot, first frame, frame of the detach
    clones = []
    for f in range(F):
        for name, (slot, first, last) in wearers.items():
            if f == first:
                eng.attach([slot], s_init[[slot]])
                rec.open([slot], s_init_rows=s_init[[slot]], names=[name])
            if f == last:
                eng.detach([slot])
                rec.close([slot])
        out = eng.step(raw[f])
        rec.step()
        clones.append({"raw": eng.raw.clone(), "s_rest": out["s_rest"].clone(), "c_t": out["c_t"].clone(), "valid": out["valid"].clone()})
        if f % 5 == 4:
            rec.drain()
    rec.close([0, 2])
    rec.drain(wait=True)
    assert rec.guards_intact() and rec.counters(wait=True)["rows_dropped"] == 0
    paths, full, pose = [], [], []
    for name, (slot, first, last) in wearers.items():
        s = rec.pop(name)
        keep, (imu, s_rest, c_t) = _wearer_rows(clones, slot)
        assert keep == list(range(first + 5, last)) and s.complete and s.slot == slot and not s.gaps          # (five frames prime)
        assert np.array_equal(_bits(s.column("raw")), _bits(imu)) and np.array_equal(_bits(imu), _bits(raw[keep, slot]))
        assert np.array_equal(_bits(s.column("s_rest")), _bits(s_rest)) and np.array_equal(_bits(s.column("c_t")), _bits(c_t))
        assert np.array_equal(s.qdq_init, s_init[slot])
        paths.append(str(tmp_path / f"{name}.pkl"))
        s.save(paths[-1])
        full.append(np.concatenate([raw[first:last, slot], raw[last - 1:last, slot]]))          # (a replay never feeds its last frame)
        pose.append((s_rest, c_t))
    recs, s0 = record.load_sessions(paths)
    assert np.array_equal(s0, s_init[[2, 0]]) and [r.shape[0] for r in recs] == [45, 56]
    assert all(np.array_equal(_bits(r), _bits(f[5:-1])) for r, f in zip(recs, full))
    with open(paths[0], "rb") as fh:
        assert np.array_equal(_bits(pickle.load(fh)["pose"]), _bits(pose[0][0]))
    # (b)
    results = replay.ReplayPool(m, slots=2).run(full, s0)
    for res, (s_rest, c_t), name in zip(results, pose, wearers):
        v = np.asarray(res.valid, dtype=bool)
        assert v.sum() == s_rest.shape[0] and not v[:6].any() and v[6:].all(), name
        assert np.array_equal(_bits(res.s_rest[v]), _bits(s_rest)), name
        assert np.array_equal(_bits(res.c_t[v]), _bits(c_t)), name


# ---- 5. with the sensor front end in front -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["staggered", "lock"])
def test_sessions_behind_step_packets(fused, kind):
    """20 frames of raw packets through SensorFrontEnd + step_packets: the sessions' imu rows are the calibrated rows the front end put
    into engine.raw, and the pose rows what the engine returned.  The lock-step engine has no valid array: rec.step() follows exactly
    the frames for which step_packets returned a dict."""
    m = fused
    n, F = 3, 20
    rng = np.random.RandomState(9)
    _, tables = so.case(n, 5)
    front = sensors.SensorFrontEnd(n, "cuda")
    front.load(list(range(n)), tables)
    s_init = (rng.randn(n, 114) * 0.2).astype(f32)
    eng = (S.StreamingEngine if kind == "lock" else S.StaggeredStreamingEngine)(m, s_init)
    if kind == "lock":
        with pytest.raises(RuntimeError, match="say where the IMU rows lie"):
            record.SessionRecorder.for_engine(eng)
    # (step_packets always fills engine.raw: that is what a lock-step caller states with raw=engine.raw)
    rec = record.SessionRecorder.for_engine(eng, page_rows=4, pages=16, **({"raw": eng.raw} if kind == "lock" else {}))
    assert (rec.valid is None) == (kind == "lock")
    rec.open(range(n), s_init_rows=s_init)
    clones = []
    for f in range(F):
        out = eng.step_packets(front, so.frame_packets(rng, n))
        if out is not None:
            rec.step()
            ok = out["valid"].clone() if "valid" in out else torch.ones(n, dtype=torch.bool, device="cuda")
            clones.append({"raw": eng.raw.clone(), "s_rest": out["s_rest"].clone(), "c_t": out["c_t"].clone(), "valid": ok})
        if f % 6 == 5:
            rec.drain()
    rec.close(range(n))
    rec.drain(wait=True)
    got = {s.slot: s for s in rec.sessions()}
    assert rec.guards_intact() and len(got) == n
    for slot in range(n):
        keep, (imu, s_rest, c_t) = _wearer_rows(clones, slot)
        s = got[slot]
        assert len(keep) == 15 == len(s) and s.complete and not s.gaps and np.isfinite(s.rows).all()
        assert np.array_equal(_bits(s.column("raw")), _bits(imu)) and np.array_equal(_bits(s.column("s_rest")), _bits(s_rest))
        assert np.array_equal(_bits(s.column("c_t")), _bits(c_t))


def test_lock_step_step_records_the_tensor_the_caller_names(fused):
    """Launch mode, lock-step: step(raw) reads the caller's tensor and never fills engine.raw (poisoned here), so the recorder is told
    where the rows lie (raw=) and stores exactly what was fed."""
    m = fused
    n, F = 2, 12
    raw, s_init = _imu_frames(n, F, 31)
    eng = S.StreamingEngine(m, s_init)
    eng.raw.fill_(float("nan"))
    feed = torch.empty((n, 72), device="cuda")
    rec = record.SessionRecorder.for_engine(eng, raw=feed, page_rows=4, pages=8)
    assert rec.sources["raw"] is feed and rec.valid is None
    rec.open(range(n), s_init_rows=s_init)
    poses = []
    for f in range(F):
        feed.copy_(torch.from_numpy(raw[f]))
        out = eng.step(feed)
        if out is not None:
            rec.step()
            poses.append(out["s_rest"].clone())
    rec.close(range(n))
    rec.drain(wait=True)
    assert torch.isnan(eng.raw).all() and rec.guards_intact()
    for s in rec.sessions():
        assert s.complete and len(s) == F - 5 and np.array_equal(_bits(s.column("raw")), _bits(raw[5:, s.slot]))
        assert np.array_equal(_bits(s.column("s_rest")), _bits(torch.stack([p[s.slot] for p in poses]).cpu().numpy()))


def test_for_engine_with_y_and_a_tracker():
    """A compact pool's y_slot and a TerrainTracker's root and q_hist beside raw, s_rest and c_t: 391 columns, each equal to the test's
    clones on the slot's valid frames."""
    from tip_amd import kinematics as kin, terrain
    m = _model()
    n, F = 3, 14
    raw, s_init = _imu_frames(n, F, 37)
    skel = kin.Skeleton.from_table(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tip_terrain_golden.npz")))
    eng = S.StaggeredStreamingEngine(m, s_init, compact=True)
    tt = terrain.TerrainTracker(skel, n, "cuda")
    tt.reset(None, s_init)
    with pytest.raises(RuntimeError, match="only a compact pool"):
        record.SessionRecorder.for_engine(S.StaggeredStreamingEngine(m, s_init), y=True)
    rec = record.SessionRecorder.for_engine(eng, y=True, tracker=tt, page_rows=4, pages=12)
    assert list(rec.sources) == ["raw", "s_rest", "c_t", "y_last", "root", "q_hist"] and rec.width == 391
    assert rec.sources["y_last"] is eng.y_slot and rec.sources["root"] is tt.root and rec.sources["q_hist"] is tt.q_hist
    rec.open(range(n), s_init_rows=s_init)
    clones = []
    for f in range(F):
        out = eng.step(raw[f])
        tt.step(out)
        rec.step()
        clones.append({"valid": out["valid"].clone(), "y_last": out["y_last"].clone(), "root": tt.root.clone(), "q_hist": tt.q_hist.clone()})
        if f % 4 == 3:
            rec.drain()
    rec.close(range(n))
    rec.drain(wait=True)
    for s in rec.sessions():
        keep = [f for f, c in enumerate(clones) if bool(c["valid"][s.slot])]
        assert keep == list(range(5, F)) and s.complete and len(s) == len(keep) and np.isfinite(s.rows).all()
        for k in ("y_last", "root", "q_hist"):
            assert np.array_equal(_bits(s.column(k)), _bits(torch.stack([clones[f][k][s.slot] for f in keep]).cpu().numpy())), k
    assert rec.guards_intact()


def test_fewer_free_pages_than_askers_is_exact_in_its_counts():
    """5 slots ask for a page in the same frame and 3 are free: exactly 3 get one and store their own row, exactly 2 count theirs as
    dropped; which three is not defined, and not asserted."""
    n, W = 5, 8
    src = _sources(n, [W])
    rec = record.SessionRecorder(n, "cuda", src, pages=3, page_rows=4, staging_pages=3)
    src["s0"].copy_(torch.arange(n, device="cuda", dtype=torch.float32)[:, None] + torch.arange(W, device="cuda") * 0.125)
    rec.open(range(n))
    for _ in range(2):                                                            # (the second frame: the three write on, the two drop again)
        rec.step()
    c = rec.counters(wait=True)
    assert (c["rows_written"], c["rows_dropped"], c["gaps"], c["pages_in_use"]) == (6, 4, 2, 3)
    rec.close(range(n))
    rec.drain(wait=True)
    got = rec.sessions()
    assert all(s.complete for s in got) and sorted(len(s) for s in got) == [0, 0, 2, 2, 2] and rec.guards_intact()
    for s in got:
        assert (s.rows[:, 0] == s.slot).all() and (s.gaps, s.dropped) == (([], 0) if len(s) else ([(0, 2)], 2))
