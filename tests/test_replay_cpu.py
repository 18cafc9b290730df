"""No GPU: the host half of offline replay (tip_amd.replay) — the schedule, the row conventions of the reference's evaluation loop
(offline_testing_simple.py:109-155), its trim (:148-151) and its file handling (:366-387) — and the C-ABI surface of the two replay
kernels."""
import heapq
import os
import pickle
import random
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle.streaming_oracle import StreamOracle
from tip_amd import replay, synth
from tip_amd import lib as tlib

LENGTHS = [6, 7, 47, 12, 90, 1, 45]
SLOTS = [1, 3, 7, 10]                 # R > n, R > n, R = n, R < n


def _greedy_start_times(lengths, slots):
    """List scheduling on its own terms: a heap of (frame the slot is free, slot); a recording of L frames holds its slot L - 1 frames."""
    free = [(0, s) for s in range(slots)]
    heapq.heapify(free)
    start, slot, makespan = {}, {}, 0
    for i, L in enumerate(lengths):
        if L <= 1:
            continue
        t, s = heapq.heappop(free)
        start[i], slot[i] = t, s
        heapq.heappush(free, (t + L - 1, s))
        makespan = max(makespan, t + L - 1)
    return start, slot, makespan


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("lengths", [LENGTHS, [2, 2, 2, 2, 2], [1, 1], [30], [9, 1, 9, 1, 9, 9, 2, 40]], ids=str)
def test_plan_replay_properties(lengths, slots):
    plan = replay.plan_replay(lengths, slots)
    assert plan.n_frames == len(plan.frames)
    attached_at, slot_of = {}, {}
    occupant = {}                                             # slot -> (recording, last fed frame)
    for f, (att, det) in enumerate(plan.frames):
        for s in det:                                         # a detach: the frame after the slot's last fed frame, nothing to take
            assert s in occupant and occupant[s][1] == f - 1 and s not in [a for a, _ in att]
            del occupant[s]
        for s, i in att:
            assert 0 <= s < slots and i not in attached_at    # every recording exactly once
            if s in occupant:                                 # a turn-over: exactly the frame after the last fed frame
                assert occupant[s][1] == f - 1
            attached_at[i], slot_of[i] = f, s
            occupant[s] = (i, f + lengths[i] - 2)
        for s, (i, last) in occupant.items():
            assert last >= f, "a finished recording still occupies its slot"
        assert occupant, "a frame with nothing in flight"
        if att:                                               # the free slots of lowest index were the ones taken
            free = set(range(slots)) - set(occupant)
            assert not free or min(free) > max(s for s, _ in att)
    assert sorted(attached_at) == [i for i, n in enumerate(lengths) if n > 1]
    assert all(plan.slot[i] == -1 and plan.start[i] == -1 for i, n in enumerate(lengths) if n == 1)     # L = 1 takes no frame
    start, slot, makespan = _greedy_start_times(lengths, slots)
    assert plan.n_frames == makespan
    assert attached_at == start and slot_of == slot
    assert [plan.start[i] for i in start] == list(start.values()) and [plan.slot[i] for i in slot] == list(slot.values())
    # what is still attached after the last frame is handed back for detaching
    assert sorted(plan.final_detach) == sorted(s for s, (_, last) in occupant.items())
    # no two recordings overlap in a slot
    spans = sorted((slot_of[i], attached_at[i], attached_at[i] + lengths[i] - 2) for i in attached_at)
    for (s0, _, b0), (s1, a1, _) in zip(spans, spans[1:]):
        assert s0 != s1 or a1 == b0 + 1


def test_plan_replay_argument_errors():
    with pytest.raises(ValueError):
        replay.plan_replay([5, 0], 2)
    with pytest.raises(ValueError):
        replay.plan_replay([5], 0)
    assert replay.plan_replay([], 3).n_frames == 0


def _stand_in(x_imu, x_s):
    """A deterministic stand-in for the model's last row: a smooth function of the newest window row."""
    k = np.arange(131, dtype=np.float64)
    return np.tanh(0.3 * x_s[-1].astype(np.float64) + 0.05 * x_imu[-1].astype(np.float64).sum() + np.sin(0.37 * k + 0.01 * len(x_s))).astype(np.float32)


class _OracleSlot:
    def __init__(self, s_init_row):
        self.o = StreamOracle(np.asarray(s_init_row, dtype=np.float64))

    def step(self, raw):
        seen = {}

        def model(x_imu, x_s):
            seen["y"] = _stand_in(x_imu, x_s)
            return seen["y"]

        r = self.o.step(np.asarray(raw, dtype=np.float64), model)
        return None if r is None else (r[0].astype(np.float32), r[1].astype(np.float32), seen["y"])


def _script_loop(imu, s_gt0):
    """offline_testing_simple.py:118-134, literally, with StreamOracle as the runner's model-facing half (root translation left
    out: columns 0 .. 2): (s_traj_pred [L, 114], c_traj_pred [L, 20], which rows a model call produced)."""
    o = StreamOracle(s_gt0)
    m_len = imu.shape[0]
    s_traj_pred = np.zeros((m_len, 114))
    s_traj_pred[0] = s_gt0
    c_traj_pred = np.zeros((m_len, 20))
    produced = np.zeros(m_len, dtype=bool)
    for t in range(0, m_len - 1):
        r = o.step(imu[t, :].astype(np.float64), _stand_in)
        if r is None:                                           # real_time_runner_minimal.py:125-128
            res = {"qdq": s_gt0, "ct": np.zeros(20)}
        else:
            res = {"qdq": np.concatenate([np.zeros(3), r[0]]), "ct": r[1]}
            produced[t + 1] = True
        s_traj_pred[t + 1, :] = res["qdq"]
        c_traj_pred[t + 1, :] = res["ct"]
    return s_traj_pred, c_traj_pred, produced


@pytest.fixture(scope="module")
def recordings():
    recs, s0 = zip(*(synth.make_recording(L, seed=100 + i) for i, L in enumerate(LENGTHS)))
    return list(recs), np.stack(s0)


@pytest.fixture(scope="module")
def script_rows(recordings):
    recs, s0 = recordings
    return [_script_loop(r, s0[i].astype(np.float64)) for i, r in enumerate(recs)]


@pytest.mark.parametrize("slots", SLOTS)
def test_row_conventions_are_the_scripts(recordings, script_rows, slots):
    """The pool's bookkeeping (plan, cursor tables, feed / collect rules: replay_on_host) around the same per-stream closed loop gives the
    script's rows: row 0 and the priming rows are the start state with zero c_t and valid False, the step on imu[t] fills row t + 1, the
    last frame is never fed."""
    recs, s0 = recordings
    out, frames = replay.replay_on_host(recs, s0, slots, _OracleSlot)
    assert frames == replay.plan_replay(LENGTHS, slots).n_frames
    for i, (r, (s_ref, c_ref, produced)) in enumerate(zip(out, script_rows)):
        L = LENGTHS[i]
        assert r.s_rest.shape == (L, 111) and r.c_t.shape == (L, 20) and r.valid.shape == (L,) and r.y_last.shape == (L, 131)
        assert np.array_equal(r.s_rest, s_ref[:, 3:].astype(np.float32)), i
        assert np.array_equal(r.c_t, c_ref.astype(np.float32)), i
        assert np.array_equal(r.valid, produced), i
        prim = min(L, 6)
        assert not r.valid[:prim].any() and r.valid[prim:].all()
        assert np.array_equal(r.s_rest[:prim], np.repeat(s0[i][None, 3:], prim, 0)) and not r.c_t[:prim].any()
        assert np.isnan(r.y_last[:prim]).all() and np.isfinite(r.y_last[prim:]).all()
    assert not out[0].valid.any() and out[1].valid.sum() == 1 and LENGTHS[5] == 1 and out[5].s_rest.shape == (1, 111)


def test_trim_like_reference():
    rng = np.random.RandomState(3)
    for L in (1, 2, 6, 7, 8, 9, 15, 60):
        for width in (111, 114):
            s_traj_pred = rng.randn(L, width)
            want = s_traj_pred.copy()
            before = s_traj_pred.copy()
            trim = 5 + 2                                            # offline_testing_simple.py:149-151
            if L > trim:
                want[0:-trim, :] = want[trim:, :]
                want[-trim:, :] = want[-trim - 1, :]
                got = replay.trim_like_reference(s_traj_pred)
                assert np.array_equal(got, want), (L, width)
            else:
                # L <= 7: the script's line :151 reads row -8 of an array that has none and raises; here that is a ValueError
                with pytest.raises(IndexError):
                    want[0:-trim, :] = want[trim:, :]
                    want[-trim:, :] = want[-trim - 1, :]
                with pytest.raises(ValueError):
                    replay.trim_like_reference(s_traj_pred)
            assert np.array_equal(s_traj_pred, before)              # the argument is left alone
    assert replay.TRIM == 7


def test_recordings_from_files(tmp_path):
    rng = np.random.RandomState(11)
    paths, lens = [], [100, 149, 150, 260, 400, 200]
    for i, L in enumerate(lens):
        p = tmp_path / f"rec{i}.pkl"
        with open(p, "wb") as fh:
            pickle.dump({"imu": rng.randn(L, 72), "nimble_qdq": rng.randn(L, 114), "constrs": rng.randn(L, 20)}, fh)
        paths.append(str(p))
    TEST_LEN, seed = 200, 42
    recs, s_init = replay.recordings_from_files(paths, TEST_LEN, seed)
    # the script's loop (:366-387) under random.seed(seed)
    random.seed(seed)
    want_x, want_y0 = [], []
    for f in paths:
        data = pickle.load(open(f, "rb"))
        X = data["imu"]
        Y = data["nimble_qdq"]
        if Y.shape[0] < 2.5 / (1. / 60):
            continue
        if Y.shape[0] > TEST_LEN:
            rand_start = random.randrange(0, Y.shape[0] - TEST_LEN)
            start = rand_start
            end = rand_start + TEST_LEN
        else:
            start = 0
            end = Y.shape[0]
        X = X[start: end, :]
        Y = Y[start: end, :]
        Y[:, 2] += 0.05
        want_x.append(X)
        want_y0.append(Y[0])
    assert [r.shape[0] for r in recs] == [150, 200, 200, 200] == [x.shape[0] for x in want_x]
    for r, x in zip(recs, want_x):
        assert r.dtype == np.float32 and np.array_equal(r, x.astype(np.float32))
    assert s_init.shape == (4, 114) and s_init.dtype == np.float32 and np.array_equal(s_init, np.stack(want_y0).astype(np.float32))
    recs, s_init = replay.recordings_from_files(paths[:2], TEST_LEN, seed)
    assert recs == [] and s_init.shape == (0, 114)


def test_argument_errors(recordings):
    recs, s0 = recordings
    for bad_recs, bad_s in (([], s0[:0]),                                        # empty input
                            ([recs[0][:, :71]], s0[:1]),                         # wrong width
                            ([recs[0].reshape(-1)], s0[:1]),
                            ([recs[0][:0]], s0[:1]),                             # L = 0
                            (recs[:3], s0[:2]),                                  # s_init rows != R
                            (recs[:2], s0[:2, :113])):
        with pytest.raises(ValueError):
            replay.check_inputs(bad_recs, bad_s)
        with pytest.raises(ValueError):
            replay.replay_on_host(bad_recs, bad_s, 2, _OracleSlot)
    r, s = replay.check_inputs([recs[0].astype(np.float64)], s0[0])             # one recording, one [114] row
    assert r[0].dtype == np.float32 and s.shape == (1, 114)


def test_replay_c_abi_surface():
    """Header, bindings and exported symbols of tip_replay_feed / tip_replay_collect, and their argument checks (no launch)."""
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert re.search(r"TIP_API int tip_replay_feed\(const float\* corpus, long long n_rows, const long long\* cur, int n_slots, float\* raw, "
                     r"tip_stream_t stream\);", hdr)
    assert "TIP_API int tip_replay_collect(long long* cur, const long long* end, int n_slots, long long n_rows," in hdr
    assert "tip_replay_feed" in tlib.EXPORTS and "tip_replay_collect" in tlib.EXPORTS
    lib = tlib.load()
    assert len(lib.tip_replay_feed.argtypes) == 6 and len(lib.tip_replay_collect.argtypes) == 14
    assert lib.tip_abi_version() == 5
    assert lib.tip_replay_feed(None, 4, 64, 1, 64, None) == -1            # null corpus
    assert lib.tip_replay_feed(64, 4, 64, 1, 68, None) == -1              # raw not 16-byte aligned
    assert lib.tip_replay_feed(64, 4, 68, 1, 64, None) == -1              # cur not 8-byte aligned
    assert lib.tip_replay_feed(64, -1, 64, 1, 64, None) == -1
    assert lib.tip_replay_feed(64, 4, 64, 0, 64, None) == 0               # no slots: nothing to launch
    ok = dict(cur=64, end=64, n=0, rows=4, s_rest=64, c_t=64, y_slot=64, rows_slot=64, size_s=131, s_out=64, c_out=64, y_out=64, valid=64)
    call = lambda **k: lib.tip_replay_collect(*{**ok, **k}.values(), None)  # noqa: E731
    assert call() == 0 and call(y_out=None, y_slot=None) == 0
    for bad in (dict(size_s=130), dict(cur=None), dict(end=68), dict(valid=None), dict(y_slot=None), dict(c_out=72), dict(n=-1), dict(rows=-1)):
        assert call(**bad) == -1, bad
