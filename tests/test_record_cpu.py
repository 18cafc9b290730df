"""CPU tests of the session recorder (tip_amd.record; include/tip_hip.h, "session recorder"): the C-ABI surface, every refusal — raised
on the host, with no device and nothing launched — the numpy restatement of the page machine on a hand-written schedule, the filing of
pages into sessions, and the two file formats up to tip_amd.replay.check_inputs."""
import ctypes
import os
import pickle
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import record_oracle as ro
import tip_amd
from tip_amd import lib as tlib
from tip_amd import record, replay
from conftest import ROOT

NAMES = {"tip_record_state_bytes", "tip_record_staging_bytes", "tip_record_reset", "tip_record_open", "tip_record_close",
         "tip_record_append", "tip_record_drain"}
f32 = np.float32


def test_c_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert set(re.findall(r"TIP_API int (tip_record_\w+)\(", hdr)) == NAMES == {n for n in tlib.EXPORTS if n.startswith("tip_record_")}
    lib = tlib.load()
    assert all(hasattr(lib, n) for n in NAMES) and tlib.TIP_ABI_VERSION == 5 == lib.tip_abi_version()
    mk = open(os.path.join(tlib.CSRC, "Makefile")).read()
    assert "session recorder" in hdr and mk.count("tip_record.hip") == 2            # in SRCS and in the resource-usage report
    assert int(re.search(r"#define TIP_RECORD_MAX_SOURCES (\d+)", hdr).group(1)) == tlib.TIP_RECORD_MAX_SOURCES == record.MAX_SOURCES == 8
    assert ctypes.sizeof(tlib.RecordSource) == 16
    assert tip_amd.record is record                                               # re-exported lazily like the other modules


def _bytes(n, P, R, W):
    b = ctypes.c_size_t()
    assert tlib.load().tip_record_state_bytes(n, P, R, W, ctypes.byref(b)) == 0
    return b.value


def test_the_state_layout_is_the_header_s():
    up16 = lambda x: (x + 15) // 16 * 16
    for n, P, R, W in ((1, 1, 1, 1), (5, 3, 3, 191), (70, 13, 64, 203), (1024, 4096, 64, 203)):
        assert _bytes(n, P, R, W) == 64 + 32 * n + 32 * P + 2 * up16(4 * P) + 4 * P * R * W
    b = ctypes.c_size_t()
    assert tlib.load().tip_record_staging_bytes(7, 3, 191, ctypes.byref(b)) == 0 and b.value == 64 + 32 * 7 + 4 * 7 * 3 * 191
    assert record.default_pages(1024, 64) == 4096 and record.default_pages(1, 64) == 4 and record.default_pages(3, 100) == 9
    assert _bytes(1024, 4096, 64, 203) == 4096 * 51_968 + 196_672 == 213_057_600                           # the docstring's 213 MB


def test_entry_points_refuse_before_any_launch():
    """Null pointers, W == 0, more than 8 sources, pages < 1, page_rows < 1 and the rest of the header's list: TIP_ERR_INVALID_ARG with
    no device in the machine; count 0 and n 0 are TIP_OK without a launch."""
    lib = tlib.load()
    p, q, s = 4096, 8192, 1024             # (never dereferenced: every call here returns before a launch)
    b = ctypes.c_size_t()
    for args in ((4, 0, 64, 72), (4, -1, 64, 72), (4, 8, 0, 72), (4, 8, 64, 0), (-1, 8, 64, 72)):
        assert lib.tip_record_state_bytes(*args, ctypes.byref(b)) == -1, args
        assert lib.tip_record_reset(p, *args, None) == -1, args
    assert lib.tip_record_state_bytes(4, 8, 64, 72, None) == -1 and lib.tip_record_staging_bytes(0, 64, 72, ctypes.byref(b)) == -1
    assert lib.tip_record_staging_bytes(4, 64, 0, ctypes.byref(b)) == -1 and lib.tip_record_staging_bytes(4, 64, 72, None) == -1
    assert lib.tip_record_reset(None, 4, 8, 64, 72, None) == -1 and lib.tip_record_reset(p + 4, 4, 8, 64, 72, None) == -1
    # open / close
    for args in ((None, 4, s, s, 1), (p, 4, None, s, 1), (p, 4, s, None, 1), (p, 4, s, s, -1), (p, -1, s, s, 1), (p + 2, 4, s, s, 1), (p, 4, s + 1, s, 1)):
        assert lib.tip_record_open(*args, None) == -1, args
    for args in ((None, 4, s, 1), (p, 4, None, 1), (p, 4, s, -1), (p, -1, s, 1), (p, 4, s + 2, 1)):
        assert lib.tip_record_close(*args, None) == -1, args
    assert lib.tip_record_open(p, 4, None, None, 0, None) == 0 and lib.tip_record_close(p, 4, None, 0, None) == 0
    # append: the table is read on the host
    Src = tlib.RecordSource
    ok = (Src * 2)(Src(q, 72, 72), Src(q + 1024, 8, 8))
    assert lib.tip_record_append(p, 0, ok, 2, None, 1, None) == 0                 # n = 0: nothing to launch
    nine = (Src * 9)(*[Src(q, 4, 4)] * 9)
    for table, k in ((None, 1), (ok, 0), (ok, -1), (nine, 9), ((Src * 1)(Src(None, 72, 72)), 1), ((Src * 1)(Src(q, 0, 72)), 1),
                     ((Src * 1)(Src(q, 72, 71)), 1), ((Src * 1)(Src(q + 2, 72, 72)), 1), ((Src * 1)(Src(q, -4, 72)), 1)):
        assert lib.tip_record_append(p, 0, table, k, None, 1, None) == -1, k
    assert lib.tip_record_append(None, 0, ok, 2, None, 1, None) == -1 and lib.tip_record_append(p, -1, ok, 2, None, 1, None) == -1
    assert lib.tip_record_append(p, 0, ok, 2, s + 2, 1, None) == -1
    # drain
    for args in ((None, q, 4, None), (p, None, 4, None), (p, q, 0, None), (p, q, -1, None), (p + 4, q, 4, None), (p, q + 4, 4, None), (p, q, 4, s + 2)):
        assert lib.tip_record_drain(*args, None) == -1, args


def test_python_refusals():
    z = lambda *shape: torch.zeros(shape)
    good = OrderedDict(raw=z(4, 72), c_t=z(4, 20))
    assert [(k, w, st) for k, _, w, st in record.check_sources(4, good)] == [("raw", 72, 72), ("c_t", 20, 20)]
    wide = z(4, 100)
    assert record.check_sources(4, {"part": wide[:, 10:82]})[0][2:] == (72, 100)      # a column slice: stride 100
    for bad, match in (({}, "1 to 8 sources"), ({f"s{i}": z(4, 4) for i in range(9)}, "1 to 8 sources"), ({"raw": z(5, 72)}, r"\[4, w\]"),
                       ({"raw": z(4, 72).double()}, "float32"), ({"raw": z(4, 72, 1)}, r"\[4, w\]"), ({"raw": z(4, 0)}, r"\[4, w\]"),
                       ({"raw": z(72, 4).t()}, "unit column stride"), ({"raw": np.zeros((4, 72), f32)}, "float32 tensor"), ([1, 2], "ordered dict")):
        with pytest.raises(ValueError, match=match):
            record.check_sources(4, bad)
    for kw, match in ((dict(pages=0), "pages must be"), (dict(page_rows=0), "page_rows must be"), (dict(staging_pages=0), "staging_pages must be"),
                      (dict(valid=torch.zeros(4)), "int32 tensor")):
        with pytest.raises(ValueError, match=match):
            record.SessionRecorder(4, "cpu", good, **kw)
    with pytest.raises(ValueError, match="at least 1"):
        record.SessionRecorder(0, "cpu", good)
    with pytest.raises(RuntimeError, match="runs on an MI355X"):                  # every shape refusal comes first; then: no device, no recorder
        record.SessionRecorder(4, "cpu", good)
    # the host's book: double open, duplicates, names
    book = record.SessionBook(4, {"raw": (0, 72)}, 8)
    assert book.open([2, -1, 4, 0], names=["a", "x", "y", "b"]) == ([2, -1, 4, 0], [1, 0, 0, 2]) and book.open_slots == [0, 2]
    with pytest.raises(RuntimeError, match="slot 2 is already recording session 'a'"):
        book.open([1, 2])
    assert book.open_slots == [0, 2]                                              # (refused whole: slot 1 was not opened)
    for args, match in ((([1, 1],), "duplicate"), (([1], np.zeros((2, 114))), "one s_init row"), (([1], None, ["a"]), "already in use"),
                        (([1, 3], None, ["c"]), "one name per"), ((3,), "list of slot indices")):
        with pytest.raises(ValueError, match=match):
            book.open(*args)
    assert book.close([2, 3, 7]) == ([2, 3, 7], [1]) and book.open_slots == [0]
    with pytest.raises(RuntimeError, match="still open"):
        book.pop("b")
    with pytest.raises(KeyError):
        book.pop("nobody")
    with pytest.raises(RuntimeError, match="not complete"):                      # closed, but nothing of it has arrived yet
        book.pop("a")
    assert [s.name for s in book.sessions()] == ["a", "b"]
    heads = np.zeros((4, 8), np.int32)
    heads[2] = (0, 1, 3, -1, 0, 0, 0, 0)                                         # slot 2 after the close: session 1 wrote 3 rows
    book.file_heads(heads, closing=[1])
    with pytest.raises(RuntimeError, match="not complete"):                      # the final counters are here, the page is not
        book.pop("a")
    book.file_pages(np.array([[2, 1, 0, 3, 0, 0, 0, 0]], np.int32), np.arange(8 * 72, dtype=f32).reshape(1, 8, 72))
    a = book.pop("a")
    assert a.complete and a.rows.shape == (3, 72) and [s.name for s in book.sessions()] == ["b"]
    book.close([0])
    assert book.pop("b", partial=True).complete is False and not book.sessions()


def test_for_engine_refuses_what_it_cannot_record():
    """A lock-step engine fills engine.raw only through step_packets and on replayed frames: for_engine wants to be told where the
    IMU rows lie.  Only a compact pool keeps y_last in a static buffer.  Both refused before anything is built (no device here)."""
    import types
    lock = object.__new__(tip_amd.streaming.StreamingEngine)                      # (never initialised: the refusal reads only the class)
    with pytest.raises(RuntimeError, match="say where the IMU rows lie"):
        record.SessionRecorder.for_engine(lock)
    z = lambda *shape: torch.zeros(shape)
    plain = types.SimpleNamespace(n=4, device="cpu", raw=z(4, 72), s_rest=z(4, 111), c_t=z(4, 20), compact=False, rows=None)
    with pytest.raises(RuntimeError, match="only a compact pool"):
        record.SessionRecorder.for_engine(plain, y=True)
    with pytest.raises(ValueError, match="the tracker has 3 slots"):
        record.SessionRecorder.for_engine(plain, tracker=types.SimpleNamespace(n=3))
    with pytest.raises(RuntimeError, match="runs on an MI355X"):                  # everything else was accepted up to the device
        record.SessionRecorder.for_engine(plain)


def _run(machine, book, frames, script, drain_every, staging=2, W=3):
    """A schedule on the oracle with a SessionBook filing its pages: script {frame: [("open" | "close", slots)]}, one append per frame
    whose row of slot s is [frame, s, ...], a drain every drain_every frames (0: only at the end)."""
    for f in range(frames):
        for what, slots in script.get(f, ()):
            if what == "open":
                idx, sids = book.open(slots)
                machine.open(idx, sids)
            else:
                idx, closing = book.close(slots)
                machine.close(idx)
                book.file_heads(machine.heads.copy(), closing)
        rows = np.array([[f, s] + [0] * (W - 2) for s in range(machine.n)], f32)
        machine.append(rows, valid=np.array([(f + s) % 4 != 3 for s in range(machine.n)], np.int32))
        if drain_every and f % drain_every == drain_every - 1:
            book.file_pages(*machine.drain(staging)[:2])
    idx, closing = book.close(book.open_slots)
    machine.close(idx)
    book.file_heads(machine.heads.copy(), closing)
    while machine.full:
        book.file_pages(*machine.drain(staging)[:2])


def test_the_oracle_on_a_hand_written_schedule():
    """3 slots, 2 pages of 2 rows, no drain until frame 5.  Slot 0 opens at 0, fills page 0 at frames 0 and 1 (queued) and page 1 at
    frames 2 and 3; slot 1 opens at frame 3 and finds nothing free: its rows of frames 3 and 4 are dropped, and so is slot 0's of
    frame 4.  The drains at frame 5 free the pages; both slots resume on pages that say "follows a gap"."""
    m = ro.RecordOracle(3, 2, 2, 3)
    m.open([0, 5, -1], [7, 8, 9])                                                # entries outside [0, n) are skipped
    assert m.heads[0].tolist() == [1, 7, 0, -1, 0, 0, 0, 0] and list(m.truth) == [7]
    v1 = np.ones(3, np.int32)
    rows = lambda f: np.array([[f, s, 0] for s in range(3)], f32)
    m.append(rows(0), v1)
    m.append(rows(1), v1)                                                         # page 0 fills and is queued
    assert list(m.full) == [0] and m.heads[0].tolist() == [1, 7, 2, -1, 0, 0, 0, 0] and m.recs[0, :5].tolist() == [0, 7, 0, 2, 0]
    m.append(rows(2), np.array([0, 1, 1], np.int32))                              # masked: nothing happens
    m.append(rows(2), v1)
    assert m.heads[0].tolist() == [1, 7, 3, 1, 1, 0, 0, 0] and not m.free
    m.open([1], [11])
    m.append(rows(3), v1)                                                         # slot 0 fills page 1; slot 1 finds nothing free
    m.append(rows(4), v1)                                                         # both dropped
    assert m.heads[0].tolist() == [1, 7, 4, -1, 0, 1, 1, 1] and m.heads[1].tolist() == [1, 11, 0, -1, 0, 2, 1, 2]
    assert m.totals() == {"rows_written": 4, "rows_dropped": 3, "gaps": 2, "pages_in_use": 2, "pages": 2}
    recs, body, queued, in_use = m.drain(1)
    assert recs[0, :5].tolist() == [0, 7, 0, 2, 0] and body[0, :, 0].tolist() == [0, 1] and (queued, in_use) == (1, 1)
    with pytest.raises(ro.Contention):                                            # two slots ask, one page is free
        m.append(rows(5), v1)
    recs, body, queued, in_use = m.drain(4)
    assert recs[0, :5].tolist() == [0, 7, 1, 2, 0] and (queued, in_use) == (0, 0)
    m.append(rows(5), v1)                                                         # both resume on pages that say "follows a gap"
    assert sorted(m.recs[:, :5].tolist()) == [[0, 7, 2, 1, 1], [1, 11, 0, 1, 2]]
    m.close([0, 1, 2, 9])                                                         # slot 2 was never open, 9 is outside: nothing
    assert len(m.full) == 2 and not m.heads[:, S_OPEN].any()
    r7, g7, d7 = m.truth[7].final()
    r11, g11, d11 = m.truth[11].final()
    assert r7[:, 0].tolist() == [0, 1, 2, 3, 5] and g7 == [(4, 1)] and d7 == 1
    assert r11[:, 0].tolist() == [5] and g11 == [(0, 2)] and d11 == 2


S_OPEN = ro.S_OPEN


@pytest.mark.parametrize("drain_every", [1, 3, 0])
def test_filed_sessions_equal_the_truth(drain_every):
    """The host's filing (SessionBook) on the oracle's pages: sessions that open, close and reopen, a pool that runs dry when it is
    never drained — rows, gap lists and totals equal the truth kept without pages."""
    n, R, W = 4, 3, 5
    m = ro.RecordOracle(n, 64 if drain_every else 6, R, W)
    book = record.SessionBook(n, {"a": (0, 2), "b": (2, 5)}, R)
    script = {0: [("open", [0])], 2: [("open", [1, -1])], 9: [("close", [0, 2])], 10: [("open", [0, n])], 17: [("open", [3])], 21: [("close", [1])]}
    _run(m, book, 40, script, drain_every, W=W)
    got = {s.name: s for s in book.sessions()}
    assert len(got) == len(m.truth) == 4 and all(s.closed and s.complete for s in got.values())
    for sid, t in m.truth.items():
        rows, gaps, dropped = t.final()
        s = got[f"session{sid}"]
        assert s.slot == t.slot and np.array_equal(s.rows, rows) and s.gaps == gaps and s.dropped == dropped, sid
    assert any(s.dropped for s in got.values()) == (drain_every == 0)
    assert list(got["session1"].columns.items()) == [("a", (0, 2)), ("b", (2, 5))] and got["session1"].column("b").shape[1] == 3


def _session(L=9, pose=True, seed=0):
    rng = np.random.RandomState(seed)
    cols = OrderedDict(raw=(0, 72))
    if pose:
        cols.update(s_rest=(72, 183), c_t=(183, 203))
    W = 203 if pose else 72
    return record.Session("anna/1", 3, cols, rng.randn(L, W).astype(f32), rng.randn(114).astype(f32), [(4, 2)], 2)


@pytest.mark.parametrize("pose", [True, False])
def test_files_round_trip_and_feed_the_replay(tmp_path, pose):
    a, b = _session(9, pose, 1), _session(12, pose, 2)
    pkl, npz = str(tmp_path / "a.pkl"), str(tmp_path / "b.npz")
    a.save(pkl)
    b.save(npz)
    # the .pkl form: the demo's dictionary, read with nothing but pickle + numpy
    with open(pkl, "rb") as fh:
        d = pickle.load(fh)
    assert {"imu", "qdq_init"} <= set(d) and d["imu"].dtype == f32 and d["imu"].shape == (9, 72) and d["qdq_init"].shape == (114,)
    assert np.array_equal(d["imu"], a.rows[:, :72]) and np.array_equal(d["qdq_init"], a.qdq_init)
    assert (("pose" in d) and ("c_t" in d) and ("columns" in d)) == pose
    if pose:
        assert np.array_equal(d["pose"], a.rows[:, 72:183]) and np.array_equal(d["c_t"], a.rows[:, 183:]) and d["columns"][1] == ("s_rest", 72, 183)
    # the .npz form holds no pickled object
    with np.load(npz, allow_pickle=False) as z:
        assert all(z[k].dtype != object for k in z.files) and np.array_equal(z["rows"], b.rows)
    for s, path in ((a, pkl), (b, npz)):
        back = record.Session.load(path)
        assert back.name == s.name and back.slot == 3 and list(back.columns.items()) == list(s.columns.items()) and back.gaps == [(4, 2)]
        assert np.array_equal(back.rows, s.rows) and np.array_equal(back.qdq_init, s.qdq_init) and back.dropped == 2
    recs, s0 = record.load_sessions([pkl, npz])
    assert [r.shape for r in recs] == [(9, 72), (12, 72)] and s0.shape == (2, 114) and s0.dtype == f32
    assert np.array_equal(recs[0], a.rows[:, :72]) and np.array_equal(recs[1], b.rows[:, :72]) and np.array_equal(s0[1], b.qdq_init)
    r2, s2 = replay.check_inputs(recs, s0)                                        # exactly the form ReplayPool.run takes
    assert all(x is y or np.array_equal(x, y) for x, y in zip(r2, recs)) and np.array_equal(s2, s0)
    # the demo's own file (float64 rows, two keys) loads as well
    demo = str(tmp_path / "demo.pkl")
    with open(demo, "wb") as fh:
        pickle.dump({"imu": a.rows[:, :72].astype(np.float64), "qdq_init": a.qdq_init.astype(np.float64)}, fh)
    recs, s0 = record.load_sessions(demo)
    assert recs[0].dtype == f32 and np.array_equal(recs[0], a.rows[:, :72]) and s0.shape == (1, 114)
    with pytest.raises(ValueError, match="source named 'raw'"):
        record.Session("x", 0, {"c_t": (0, 20)}, np.zeros((2, 20), f32), np.zeros(114, f32), [], 0).save(pkl)
    np.savez(npz, a=np.zeros(3))
    with pytest.raises(ValueError, match="not a session file"):
        record.Session.load(npz)
