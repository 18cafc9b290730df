"""Session recorder: log what a live pool's wearers were served, on the device, and get it back as files the offline path reads.

The reference's live loop records (live_demo_new.py:276-278, 312-323, `is_recording`): it appends every calibrated IMU row to a list
and writes {"imu": [L, 72], "qdq_init": [114]} every 15 s — the file its offline script evaluates later.  Here the rows never visit the
host one by one.  `SessionRecorder` is a consumer BESIDE the frame, as RootTracker.step and TerrainTracker.step are: one launch behind
engine.step*() on the same stream (tip_record_append, csrc/tip_record.hip) copies every valid open slot's row — row `slot` of a few
static device buffers, one behind the other — into a page of a page pool in HBM; every few frames drain() gathers the pages that
filled, copies them to pinned memory without blocking and files those that have arrived under their session.

    rec = SessionRecorder.for_engine(engine)                 # raw (72) | s_rest (111) | c_t (20 | 8), valid = the engine's T
    rec.open([3], s_init_rows=s_init[[3]], names=["anna"])   # with engine.attach([3], ...)
    for frame in ...:
        out = engine.step(raw); rec.step()                   # ONE launch more; nothing is read by the host
        if frame % 16 == 0: rec.drain()                      # one launch + one non-blocking copy; never synchronises
    rec.close([3]); rec.drain(wait=True)                     # with engine.detach([3])
    rec.pop("anna").save("anna.pkl")                         # the demo's dictionary; tip_amd.replay reads it (load_sessions)

No engine, front-end, tracker, replay or hand-over code is involved or changed.  A recording does not move with
tip_amd.handover.export_wearers: the caller closes the session on the source pool and opens one on the destination (`names` lets the two
parts share a name with a part number)."""
from __future__ import annotations

import ctypes
import math
import pickle
from collections import OrderedDict
from typing import List, Optional, Sequence, Tuple

import numpy as np

HDR_WORDS, HEAD_WORDS, REC_WORDS = 16, 8, 8          # include/tip_hip.h, "session recorder": header, slot head, page record (int32 words)
MAX_SOURCES = 8                                       # TIP_RECORD_MAX_SOURCES
FPS = 60                                              # constants.py:7 (DT = 1 / 60)
DEFAULT_SECONDS = 4                                   # the default page pool holds this much of every slot
GUARD_BYTES = 256                                     # sentinel bytes in front of and behind the state and staging buffers
GUARD_BYTE = 0xA5
FILE_KEYS = {"raw": "imu", "s_rest": "pose", "c_t": "c_t"}      # source name -> key of the demo's dictionary


class Session:
    """One wearer's recording: `rows` [L, W] float32, one stored row per valid frame, `columns` {source name: (first, last + 1)} into W,
    `qdq_init` [114] float32 (the s_init row given to open(); zeros when none was), `gaps` [(row, dropped), ...] — `dropped` rows were
    lost in front of stored row `row` because no page was free (row = L: behind the last one) — and `dropped`, their total.  `closed`:
    close() was called; `complete`: closed, and every page and the final counters have arrived."""

    def __init__(self, name, slot, columns, rows, qdq_init, gaps, dropped, closed=True, complete=True):
        self.name, self.slot, self.columns = name, int(slot), OrderedDict(columns)
        self.rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.qdq_init = np.ascontiguousarray(qdq_init, dtype=np.float32).reshape(114)
        self.gaps = [(int(r), int(d)) for r, d in gaps]
        self.dropped, self.closed, self.complete = int(dropped), bool(closed), bool(complete)

    def __len__(self):
        return int(self.rows.shape[0])

    def column(self, name: str) -> np.ndarray:
        a, b = self.columns[name]
        return self.rows[:, a:b]

    def save(self, path: str):
        """A path ending in .pkl gets the demo's dictionary (live_demo_new.py:318-321), readable with nothing but pickle and numpy:
        {"imu": [L, 72], "qdq_init": [114]} plus, when they were recorded, "pose" [L, 111] (s_rest), "c_t" [L, 20 | 8] and "columns" (every
        other source under its own name, and the layout of `rows`).  "imu" is FLOAT32 — the rows the model was served, bit for bit; the
        demo writes its own in float64.  Any other path gets a plain .npz (no pickled objects: np.load(..., allow_pickle=False) reads
        it) with the whole of `rows`, the column table, the gaps and the name.  Both need a source named "raw" of 72 columns."""
        if "raw" not in self.columns or self.columns["raw"][1] - self.columns["raw"][0] != 72:
            raise ValueError("tip_amd.record.Session.save: the file formats hold the IMU rows — record a source named 'raw' [n, 72]")
        if str(path).endswith(".pkl"):
            d = {"imu": np.array(self.column("raw")), "qdq_init": np.array(self.qdq_init)}
            for src, (a, b) in self.columns.items():
                if src != "raw":
                    d[FILE_KEYS.get(src, src)] = np.array(self.rows[:, a:b])
            if len(self.columns) > 1:
                d["columns"] = [(k, int(a), int(b)) for k, (a, b) in self.columns.items()]
            d["gaps"], d["name"], d["slot"] = list(self.gaps), self.name, self.slot
            with open(path, "wb") as fh:
                pickle.dump(d, fh)
            return
        names = list(self.columns)
        np.savez(path, rows=self.rows, qdq_init=self.qdq_init, column_names=np.array(names),
                 column_bounds=np.array([self.columns[k] for k in names], dtype=np.int64).reshape(-1, 2),
                 gaps=np.array(self.gaps, dtype=np.int64).reshape(-1, 2), dropped=np.int64(self.dropped),
                 name=np.array(str(self.name)), slot=np.int64(self.slot))

    @staticmethod
    def load(path: str) -> "Session":
        """A file written by save(), either format."""
        if str(path).endswith(".pkl"):
            with open(path, "rb") as fh:
                d = pickle.load(fh)
            imu = np.asarray(d["imu"], dtype=np.float32)
            cols = d.get("columns") or [("raw", 0, 72)]
            rows = np.zeros((imu.shape[0], max(b for _, _, b in cols)), dtype=np.float32)
            for k, a, b in cols:
                rows[:, a:b] = imu if k == "raw" else d[FILE_KEYS.get(k, k)]
            gaps = d.get("gaps", [])
            return Session(d.get("name"), d.get("slot", -1), [(k, (a, b)) for k, a, b in cols], rows, d["qdq_init"], gaps,
                           sum(g for _, g in gaps))
        with np.load(path, allow_pickle=False) as z:
            if "rows" not in z.files or "column_names" not in z.files:
                raise ValueError(f"tip_amd.record.Session.load: {path} is not a session file")
            cols = [(str(k), (int(a), int(b))) for k, (a, b) in zip(z["column_names"], z["column_bounds"])]
            return Session(str(z["name"]), int(z["slot"]), cols, z["rows"], z["qdq_init"], [tuple(g) for g in z["gaps"]], int(z["dropped"]))


def load_sessions(paths) -> Tuple[List[np.ndarray], np.ndarray]:
    """Session files (either format of Session.save, or the demo's own pickles) as (recordings, s_init): a list of contiguous float32
    [L_i, 72] IMU arrays and float32 [R, 114], exactly what tip_amd.replay.ReplayPool.run and check_inputs take.  Nothing is cropped,
    skipped or lifted (tip_amd.replay.recordings_from_files does the script's file handling, on files that carry a ground truth)."""
    recs, s0 = [], []
    for p in ([paths] if isinstance(paths, str) else paths):
        if str(p).endswith(".pkl"):
            with open(p, "rb") as fh:
                d = pickle.load(fh)
            imu, q = d["imu"], d["qdq_init"]
        else:
            s = Session.load(p)
            imu, q = s.column("raw"), s.qdq_init
        imu = np.ascontiguousarray(imu, dtype=np.float32)
        if imu.ndim != 2 or imu.shape[1] != 72:
            raise ValueError(f"tip_amd.record.load_sessions: {p}: 'imu' is {imu.shape}; a recording is [L, 72]")
        recs.append(imu)
        s0.append(np.asarray(q, dtype=np.float32).reshape(114))
    return recs, (np.stack(s0) if s0 else np.zeros((0, 114), dtype=np.float32))


def default_pages(n: int, page_rows: int = 64) -> int:
    """Pages that hold DEFAULT_SECONDS = 4 s (240 frames) of every one of n slots: n * ceil(240 / page_rows) — 4 n at 64 rows."""
    return max(1, int(n)) * math.ceil(DEFAULT_SECONDS * FPS / int(page_rows))


def check_sources(n: int, sources) -> list:
    """`sources` (an ordered mapping name -> static tensor [n, w] float32) as [(name, tensor, w, row stride in floats)]; ValueError for
    anything the append launch cannot read: no source, more than 8, a tensor that is not float32 [n, w] with w >= 1 and unit column
    stride, tensors on different devices."""
    try:
        items = list(sources.items())
    except AttributeError:
        raise ValueError("tip_amd.record.SessionRecorder: sources is an ordered dict name -> device tensor [n, w] float32") from None
    if not 1 <= len(items) <= MAX_SOURCES:
        raise ValueError(f"tip_amd.record.SessionRecorder: 1 to {MAX_SOURCES} sources (TIP_RECORD_MAX_SOURCES); got {len(items)}")
    import torch
    out = []
    for name, t in items:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != n or t.shape[1] < 1:
            raise ValueError(f"tip_amd.record.SessionRecorder: source {name!r} must be a float32 tensor [{n}, w]; got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.stride(1) != 1 or (n > 1 and t.stride(0) < t.shape[1]):
            raise ValueError(f"tip_amd.record.SessionRecorder: source {name!r} must have unit column stride and rows that do not overlap")
        if t.device != items[0][1].device:
            raise ValueError(f"tip_amd.record.SessionRecorder: source {name!r} is on {t.device}, {items[0][0]!r} on {items[0][1].device}")
        out.append((str(name), t, int(t.shape[1]), int(t.stride(0)) if n > 1 else int(t.shape[1])))
    return out


class _Live:
    """A session the book still works on."""

    def __init__(self, sid, name, slot, qdq_init):
        self.sid, self.name, self.slot, self.qdq_init = sid, name, slot, qdq_init
        self.pages = {}                     # seq -> (rows [k, W], rows dropped in front)
        self.closed = False
        self.head = None                    # (rows written, rows dropped, rows dropped since the last stored row) of the newest snapshot
        self.final = False                  # that snapshot was taken behind the close


class SessionBook:
    """The host half of the recorder, numpy only: which slot records which session, and the filing of what the device hands back —
    page records with their contents (file_pages) and snapshots of the slot heads (file_heads).  SessionRecorder owns one; the tests
    drive it from the numpy restatement of the page machine as well."""

    def __init__(self, n: int, columns, page_rows: int):
        self.n, self.page_rows = int(n), int(page_rows)
        self.columns = OrderedDict(columns)
        self.width = max(b for _, b in self.columns.values())
        self._open = {}                     # slot -> session id
        self._live = OrderedDict()          # session id -> _Live
        self._next = 1

    def open(self, slots, s_init_rows=None, names=None):
        """-> (entries, session ids), one per list entry; an entry outside [0, n) is kept (the device skips it) with id 0.  RuntimeError
        for a slot that is open, ValueError for a slot listed twice, a name in use or rows / names that do not match the list."""
        try:
            idx = [int(i) for i in slots]
        except TypeError:
            raise ValueError("tip_amd.record.SessionRecorder.open: slots must be a list of slot indices") from None
        inside = [i for i in idx if 0 <= i < self.n]
        if len(set(inside)) != len(inside):
            raise ValueError("tip_amd.record.SessionRecorder.open: duplicate slot index")
        for i in inside:
            if i in self._open:
                raise RuntimeError(f"tip_amd.record.SessionRecorder.open: slot {i} is already recording session "
                                   f"{self._live[self._open[i]].name!r}; close it first")
        rows = None
        if s_init_rows is not None:
            rows = np.asarray(s_init_rows, dtype=np.float32).reshape(-1, 114) if len(idx) else np.zeros((0, 114), np.float32)
            if rows.shape[0] != len(idx):
                raise ValueError("tip_amd.record.SessionRecorder.open: one s_init row [114] per list entry")
        if names is not None:
            names = list(names)
            if len(names) != len(idx):
                raise ValueError("tip_amd.record.SessionRecorder.open: one name per list entry")
            used = {s.name for s in self._live.values()}
            given = [names[j] for j, i in enumerate(idx) if 0 <= i < self.n]
            if len(set(given)) != len(given) or used & set(given):
                raise ValueError("tip_amd.record.SessionRecorder.open: a session name is already in use")
        sids = []
        for j, i in enumerate(idx):
            if not 0 <= i < self.n:
                sids.append(0)
                continue
            sid, self._next = self._next, self._next + 1
            name = names[j] if names is not None else f"session{sid}"
            self._live[sid] = _Live(sid, name, i, np.zeros(114, np.float32) if rows is None else rows[j].copy())
            self._open[i] = sid
            sids.append(sid)
        return idx, sids

    def close(self, slots):
        """-> (entries, ids of the sessions this closes); entries outside [0, n) and slots that are not open stay in the list (the device
        skips them)."""
        try:
            idx = [int(i) for i in slots]
        except TypeError:
            raise ValueError("tip_amd.record.SessionRecorder.close: slots must be a list of slot indices") from None
        inside = [i for i in idx if 0 <= i < self.n]
        if len(set(inside)) != len(inside):
            raise ValueError("tip_amd.record.SessionRecorder.close: duplicate slot index")
        closing = []
        for i in inside:
            sid = self._open.pop(i, None)
            if sid is not None:
                self._live[sid].closed = True
                closing.append(sid)
        return idx, closing

    @property
    def open_slots(self):
        return sorted(self._open)

    def file_pages(self, records: np.ndarray, contents: np.ndarray):
        """records [k, 8] int32 (slot, session, sequence number, rows used, rows dropped in front), contents [k, page_rows, W]."""
        for r, page in zip(np.asarray(records).reshape(-1, REC_WORDS), np.asarray(contents).reshape(-1, self.page_rows, self.width)):
            s = self._live.get(int(r[1]))
            if s is not None:               # (a session that was popped before its last page arrived: the page has no owner)
                s.pages[int(r[2])] = (np.array(page[: int(r[3])], dtype=np.float32), int(r[4]))

    def file_heads(self, heads: np.ndarray, closing=()):
        """A snapshot of the slot heads [n, 8] int32, taken behind the close of the sessions in `closing`."""
        heads = np.asarray(heads).reshape(self.n, HEAD_WORDS)
        for i in range(self.n):
            s = self._live.get(int(heads[i, 1]))
            if s is not None and s.slot == i and not s.final:
                s.head = (int(heads[i, 2]), int(heads[i, 5]), int(heads[i, 7]))
                s.final = s.sid in closing
        self.totals = {"rows_written": int(heads[:, 2].sum()), "rows_dropped": int(heads[:, 5].sum()), "gaps": int(heads[:, 6].sum())}

    totals = {"rows_written": 0, "rows_dropped": 0, "gaps": 0}

    def _session(self, s: _Live) -> Session:
        parts, gaps, at, seq = [], [], 0, 0
        while seq in s.pages:               # (pages in order, up to the first that has not arrived)
            rows, gap = s.pages[seq]
            if gap:
                gaps.append((at, gap))
            parts.append(rows)
            at += rows.shape[0]
            seq += 1
        dropped = sum(g for _, g in gaps)
        complete = False
        if s.head is not None:
            written, total, trailing = s.head
            if trailing and at == written:
                gaps.append((at, trailing))
            dropped = max(total, dropped)
            complete = s.final and at == written and len(s.pages) == seq
        rows = np.concatenate(parts) if parts else np.zeros((0, self.width), np.float32)
        return Session(s.name, s.slot, self.columns, rows, s.qdq_init, gaps, dropped, s.closed, complete)

    def sessions(self) -> List[Session]:
        return [self._session(s) for s in self._live.values()]

    def pop(self, name, partial: bool = False) -> Session:
        for sid, s in self._live.items():
            if s.name == name:
                if not s.closed:
                    raise RuntimeError(f"tip_amd.record.SessionRecorder.pop: session {name!r} is still open (slot {s.slot}); close it first")
                out = self._session(s)
                if not (out.complete or partial):
                    raise RuntimeError(f"tip_amd.record.SessionRecorder.pop: session {name!r} is not complete — pages or its final counters "
                                       "are still on the device or on their way: drain(wait=True) first (while `queued` is not 0, again), or "
                                       "pop(name, partial=True) and lose what has not arrived")
                del self._live[sid]
                return out
        raise KeyError(name)


class SessionRecorder:
    """n slots beside an engine of n slots; `sources` an ordered dict name -> STATIC device tensor [n, w] float32 (at most 8; a row of a
    session is row `slot` of each, one behind the other, W floats in all).  valid: a static device int32 [n]; a slot appends only
    where valid[slot] >= valid_min (None: every open slot appends).

    Memory.  The page pool is `pages` pages of page_rows * W floats.  The default holds 4 s of every slot (default_pages: 4 n pages at
    page_rows = 64): 64 * 203 * 4 = 51 968 bytes per page for raw | s_rest | c_t of the paper's model, so 208 KB per slot — 213 MB at
    1024 slots, 53 MB at 256, 208 KB at 1 — plus 32 bytes per slot, 40 per page and 64 in all.  staging_pages is how many pages one
    drain() can take, and every drain() copies the WHOLE staging buffer (that many pages) to pinned memory whatever it gathered, so it
    is sized for the drain rhythm, not for the pool: n slots fill n / page_rows pages per frame, and the default, max(16, n / 4) (at
    most pages), is what a drain every 16 frames of 64-row pages takes on average — 13 MB at 1024 slots.  Slots that opened together
    fill their pages together: such a burst leaves pages on the queue (`queued`) for the next drains, well inside the head-room.

    When to drain.  A slot fills a page every page_rows valid frames, and a drain returns the full pages to the pool.  With `open`
    slots recording, pages * page_rows rows of head-room divided by the number of open slots is how many frames may pass between
    drains before rows are dropped — less one page per open slot for the pages that are partly filled: at the default, 240 - 64 = 176
    frames.  Call drain() every few frames (16, say): it is one launch and one copy, and it never blocks.  Rows that find no page are
    DROPPED AND COUNTED, never written anywhere, and reported per session (Session.gaps, Session.dropped) and in counters().

    step() has static arguments only — the state buffer, the sources' addresses, `valid` — so it may also be called inside a
    torch.cuda.graph capture, behind the engine's frame or on its own; no capture_into() is needed.

    Hand-over.  A recording does not move with tip_amd.handover.export_wearers, and tip_amd.handover knows nothing of it: close the
    session here, open one on the destination pool's recorder; `names` lets the two parts share a name with a part number."""

    def __init__(self, n: int, device, sources, pages: Optional[int] = None, page_rows: int = 64, staging_pages: Optional[int] = None,
                 valid=None, valid_min: int = 1):
        import torch
        from . import lib as _lib
        self.n, self.page_rows = int(n), int(page_rows)
        if self.n < 1:
            raise ValueError(f"tip_amd.record.SessionRecorder: n is the number of slots, at least 1; got {n!r}")
        if self.page_rows < 1:
            raise ValueError(f"tip_amd.record.SessionRecorder: page_rows must be at least 1; got {page_rows!r}")
        srcs = check_sources(self.n, sources)
        self.pages = default_pages(self.n, self.page_rows) if pages is None else int(pages)
        if self.pages < 1:
            raise ValueError(f"tip_amd.record.SessionRecorder: pages must be at least 1; got {pages!r}")
        self.staging_pages = min(self.pages, max(16, -(-self.n // 4))) if staging_pages is None else int(staging_pages)
        if not 1 <= self.staging_pages:
            raise ValueError(f"tip_amd.record.SessionRecorder: staging_pages must be at least 1; got {staging_pages!r}")
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:          # ("cuda": the current device, as the tensors name it)
            self.device = torch.device("cuda", torch.cuda.current_device())
        if valid is not None and not (isinstance(valid, torch.Tensor) and valid.dtype == torch.int32 and tuple(valid.shape) == (self.n,)
                                      and valid.is_contiguous()):
            raise ValueError(f"tip_amd.record.SessionRecorder: valid is a contiguous int32 tensor [{self.n}]")
        columns, at = OrderedDict(), 0
        for name, _, w, _ in srcs:
            columns[name] = (at, at + w)
            at += w
        self.width = at
        self.book = SessionBook(self.n, columns, self.page_rows)
        if self.device.type != "cuda" or any(t.device != self.device for _, t, _, _ in srcs) or (valid is not None and valid.device != self.device):
            raise RuntimeError("tip_amd.record.SessionRecorder runs on an MI355X: the sources (and valid) are static tensors on `device`")
        self._torch, self._lib, self.lib = torch, _lib, _lib.load()
        self.sources, self.valid, self.valid_min = OrderedDict((k, t) for k, t, _, _ in srcs), valid, int(valid_min)
        self._table = (_lib.RecordSource * len(srcs))(*[_lib.RecordSource(t.data_ptr(), w, st) for _, t, w, st in srcs])
        nb, sb = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(self.lib.tip_record_state_bytes(self.n, self.pages, self.page_rows, self.width, ctypes.byref(nb)))
        _lib.check(self.lib.tip_record_staging_bytes(self.staging_pages, self.page_rows, self.width, ctypes.byref(sb)))
        self.state_bytes, self.staging_bytes = nb.value, sb.value
        self._head_bytes = 4 * (HDR_WORDS + HEAD_WORDS * self.n)
        with torch.cuda.device(self.device):
            self._state_raw = torch.full((nb.value + 2 * GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=self.device)
            self._staging_raw = torch.full((sb.value + 2 * GUARD_BYTES,), GUARD_BYTE, dtype=torch.uint8, device=self.device)
            self.state = self._state_raw[GUARD_BYTES: GUARD_BYTES + nb.value]
            self.staging = self._staging_raw[GUARD_BYTES: GUARD_BYTES + sb.value]
            self._p_state, self._p_staging = self.state.data_ptr(), self.staging.data_ptr()
            self._p_valid = None if valid is None else valid.data_ptr()
            _lib.check(self.lib.tip_record_reset(self._p_state, self.n, self.pages, self.page_rows, self.width, self._stream()))
        self._pinned = {self.staging_bytes: [], self._head_bytes: []}      # pinned buffers at rest, by size
        self._pending = []                  # (event, kind, pinned buffer, closing ids), in stream order
        self._counters = {"rows_written": 0, "rows_dropped": 0, "gaps": 0, "pages_in_use": 0, "pages": self.pages}
        self.steps = self.drains = 0

    @classmethod
    def for_engine(cls, engine, pose: bool = True, y: bool = False, tracker=None, raw=None, **kw) -> "SessionRecorder":
        """The recorder of an engine's frame: the IMU row [n, 72] the model was served, then, with pose, s_rest [n, 111] and c_t
        [n, 20 | 8]; with y the model's raw last rows (a compact pool's y_slot — the other engines keep no static buffer for them:
        RuntimeError); with a RootTracker / TerrainTracker its root [n, 3] and, where it has one, q_hist [n, 54].
        StaggeredStreamingEngine: the IMU source is engine.raw, which step() and step_packets() fill every frame, and valid is the
        engine's T — it keeps T - 1 per slot in a static array (rows; a compact pool: rows_slot), read with valid_min = 0, so a priming
        or detached slot writes nothing.
        The lock-step StreamingEngine has no such array — every stream is valid once step() returns a dict: call rec.step() behind
        exactly those frames — and it does NOT always fill engine.raw: step(raw) reads the caller's tensor and copies it into
        engine.raw only on replayed frames (use_graph=True, steady state).  So for a lock-step engine `raw=` must say where the rows
        lie: raw=engine.raw by a caller who feeds it through step_packets (which always fills it), or the static [n, 72] device tensor
        the caller hands to step().  Without it: RuntimeError, before anything is built."""
        from .streaming import StreamingEngine
        if raw is None:
            if isinstance(engine, StreamingEngine):
                raise RuntimeError("tip_amd.record.SessionRecorder.for_engine: a lock-step StreamingEngine fills engine.raw only through "
                                   "step_packets and on replayed frames; say where the IMU rows lie — raw=engine.raw (step_packets), or the "
                                   "static [n, 72] device tensor you pass to step()")
            raw = engine.raw
        src = OrderedDict(raw=raw)
        if pose:
            src["s_rest"], src["c_t"] = engine.s_rest, engine.c_t
        if y:
            if not getattr(engine, "compact", False):
                raise RuntimeError("tip_amd.record.SessionRecorder.for_engine(y=True): only a compact pool keeps the model's last rows in a "
                                   "static buffer (y_slot); give any other static tensor through SessionRecorder(sources=...)")
            src["y_last"] = engine.y_slot
        if tracker is not None:
            if tracker.n != engine.n:
                raise ValueError(f"tip_amd.record.SessionRecorder.for_engine: the tracker has {tracker.n} slots, the engine {engine.n}")
            src["root"] = tracker.root
            if getattr(tracker, "q_hist", None) is not None:
                src["q_hist"] = tracker.q_hist
        valid = getattr(engine, "rows_slot", None) if getattr(engine, "compact", False) else getattr(engine, "rows", None)
        return cls(engine.n, engine.device, src, valid=valid, valid_min=0, **kw)

    def _stream(self):
        return self._lib.current_stream(self.device)

    def _list_dev(self, *rows):
        """Equal-length int lists as ONE pinned int32 array, on the device by one non-blocking copy."""
        host = self._torch.tensor(rows, dtype=self._torch.int32).reshape(len(rows), -1).pin_memory()
        return host.to(self.device, non_blocking=True)

    # ---- the device calls -----------------------------------------------------------------------------------------------------------------
    def open(self, slots, s_init_rows=None, names=None):
        """Start a session on each listed slot: the host keeps qdq_init (the slot's s_init row [114]; zeros when none is given), the name
        (default "session<id>") and a session id; one launch on the current stream.  Entries outside [0, n) are skipped, as the
        device skips them.  Opening a slot that is already open is a RuntimeError, raised before anything is launched."""
        idx, sids = self.book.open(slots, s_init_rows, names)
        if not idx:
            return
        with self._lib.on_device(self.device):
            t = self._list_dev(idx, sids)
            self._lib.check(self.lib.tip_record_open(self._p_state, self.n, t[0].data_ptr(), t[1].data_ptr(), len(idx), self._stream()))

    def close(self, slots):
        """Stop the listed slots' sessions: a partly filled page goes onto the full queue (the next drain() brings it), and a small
        non-blocking read brings the sessions' final counters.  Slots that are not open, and entries outside [0, n), do nothing."""
        idx, closing = self.book.close(slots)
        if not idx:
            return
        with self._lib.on_device(self.device):
            t = self._list_dev(idx)
            self._lib.check(self.lib.tip_record_close(self._p_state, self.n, t[0].data_ptr(), len(idx), self._stream()))
            self._snapshot(closing)

    def step(self):
        """THE per-frame call: one tip_record_append launch on the current stream, behind the engine's frame.  Every argument is static."""
        with self._lib.on_device(self.device):
            status = self.lib.tip_record_append(self._p_state, self.n, self._table, len(self._table), self._p_valid, self.valid_min,
                                                self._stream())
        if status < 0:
            self._lib.check(status)
        self.steps += 1

    def _pin(self, nbytes):
        free = self._pinned[nbytes]
        return free.pop() if free else self._torch.empty(nbytes, dtype=self._torch.uint8, pin_memory=True)

    def _enqueue(self, kind, src, closing=()):
        buf = self._pin(src.numel())
        buf.copy_(src, non_blocking=True)
        ev = self._torch.cuda.Event()
        ev.record()
        self._pending.append((ev, kind, buf, tuple(closing)))
        return ev

    def _snapshot(self, closing=()):
        return self._enqueue("heads", self.state[: self._head_bytes], closing)

    def _collect(self):
        """File everything whose copy has completed, in stream order; never blocks."""
        while self._pending and self._pending[0][0].query():
            _, kind, buf, closing = self._pending.pop(0)
            words = buf.numpy().view(np.int32)
            if kind == "heads":
                self.book.file_heads(words[HDR_WORDS:].reshape(self.n, HEAD_WORDS), closing)
                free = (int(words[6]) - int(words[5])) & 0xFFFFFFFF          # (free ring: tail - head, counters that run on)
                self._counters.update(self.book.totals, pages_in_use=self.pages - free)
            else:
                k = int(words[0])
                recs = words[HDR_WORDS: HDR_WORDS + REC_WORDS * k].reshape(k, REC_WORDS)
                body = buf.numpy()[4 * (HDR_WORDS + REC_WORDS * self.staging_pages):].view(np.float32)
                self.book.file_pages(recs, body[: k * self.page_rows * self.width].reshape(k, self.page_rows, self.width))
                self._counters["pages_in_use"] = int(words[2])
                self.queued = int(words[1])
            self._pinned[buf.numel()].append(buf)

    queued = 0      # pages that were still on the full queue behind the newest drain that has arrived (staging_pages was too small for them)

    def drain(self, wait: bool = False):
        """One tip_record_drain launch — the pages on the full queue into the staging buffer and back onto the free ring — plus ONE
        non-blocking copy of the staging buffer to pinned memory, with an event; then whatever has arrived (this copy or earlier ones)
        is filed under its session by sequence number.  Never synchronises; wait=True synchronises once, on the last event, so that
        everything launched so far is filed when it returns."""
        with self._lib.on_device(self.device):
            self._lib.check(self.lib.tip_record_drain(self._p_state, self._p_staging, self.staging_pages, None, self._stream()))
            ev = self._enqueue("pages", self.staging)
            self.drains += 1
            if wait:
                ev.synchronize()
        self._collect()

    def counters(self, wait: bool = False) -> dict:
        """rows_written and rows_dropped (over the slots' current or last sessions), gaps, pages_in_use and pages, as of the newest
        snapshot that has ARRIVED: the call starts a non-blocking read of the header and the slot heads (64 + 32 n bytes) and returns
        what earlier reads brought — it does not synchronise, so the numbers trail the device by a call.  wait=True waits for its own."""
        with self._lib.on_device(self.device):
            ev = self._snapshot()
            if wait:
                ev.synchronize()
        self._collect()
        return dict(self._counters)

    # ---- what has been filed ----------------------------------------------------------------------------------------------------------
    def sessions(self) -> List[Session]:
        """Every session that has not been popped, open ones included, with the rows that have arrived so far."""
        self._collect()
        return self.book.sessions()

    def pop(self, name, partial: bool = False) -> Session:
        """A closed, complete session, forgotten by the recorder (KeyError: no such name; RuntimeError: still open, or not complete —
        pages that arrive for a forgotten session have no owner and are lost, so that takes partial=True)."""
        self._collect()
        return self.book.pop(name, partial)

    def guards_intact(self) -> bool:
        """The sentinel bytes in front of and behind the state and the staging buffer are as they were written (synchronises: a check
        for tests and for debugging, never for the frame loop)."""
        ok = True
        for raw, nbytes in ((self._state_raw, self.state_bytes), (self._staging_raw, self.staging_bytes)):
            g = self._torch.cat([raw[:GUARD_BYTES], raw[GUARD_BYTES + nbytes:]])
            ok = ok and bool((g == GUARD_BYTE).all().item())
        return ok
