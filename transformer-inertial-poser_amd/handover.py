"""Wearer hand-over: a live wearer's whole state moved between pools (csrc/tip_handover.hip; include/tip_hip.h, "hand-over").

Everything around the model lives per wearer in HBM as "n fixed blocks in one buffer", n fixed when the object is built: the streaming
engine's block, the front end's calibration and fill blocks, the resampler's packet ring, the clock's envelope, a tracker's carry or
terrain block, the display side's ring of recent poses (display.PoseResampler, poses=).  A wearer could enter a pool only through attach(), at its frame 0.  Here it moves as it stands, and continues bit for bit:

    w = export_wearers([3, 7], engine=small, front=front_a, resampler=rs_a, clock=ck_a, tracker=tt_a)     # nothing is detached ...
    small.detach([3, 7])                                                                                  # ... that is the next call
    import_wearers(w, [0, 1], engine=big, front=front_b, resampler=rs_b, clock=ck_b, tracker=tt_b)        # the next step() goes on

    w.cpu().save("wearers.npz")                      # a restart: ... Wearers.load("wearers.npz").to(device), then import_wearers
    w.cpu().to("cuda:1")                             # another GPU: the host path (pinned memory, non-blocking)

Each object has export_slots(slots) -> {"meta": shape parameters, "per": per-wearer host values, tensors [count, ...]} and
import_slots(slots, exported); export_wearers / import_wearers run them over a chain, and Wearers carries the result with a header
(TIP_ABI_VERSION and per component the block size and shape parameters).  Every mismatch — window, model shape, depth, grid, fill,
skeleton, ABI version, block size, duplicate or out-of-range slots, an attached destination — is a ValueError / RuntimeError on the host
before anything is launched (the check_* functions below need no device).  The device-to-device path never synchronises: slot lists go
up from pinned memory, blocks move in one launch per buffer (tip_handover_export / _import / _stream_import), per-slot rows by gathers
and scatters, all on the current stream behind the previous frame.

Bits: against the project's own uninterrupted run, on a plan whose per-window result does not depend on the batch (set_plan("fused"),
the rule compact=True documents).  Trackers: between two trackers on the same entries (both given scales, or neither).  live_dropout:
the blocks move exactly, the engine's seeds do not (StaggeredStreamingEngine.export_slots)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import lib as _lib
from .streaming import slot_list

COMPONENTS = ("engine", "front", "resampler", "clock", "tracker", "poses")
_TRACKER_KINDS = {"RootTracker": 0, "TerrainTracker": 1}


# ---- host checks (no device) -------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def check_meta(who: str, mine: dict, theirs: dict, what: dict):
    """ValueError unless `theirs` (an export's meta) has every key of `mine` (the destination's) with an equal value; `what` names the
    keys in the message."""
    for k, v in mine.items():
        if k not in theirs or not _same(v, theirs[k]):
            got = theirs.get(k, "nothing")
            got = got if np.ndim(got) == 0 else "another"
            mine_v = v if np.ndim(v) == 0 else "its own"
            raise ValueError(f"tip_amd.{who}: {what.get(k, k)} differs — the wearers were exported with {got}, this object has {mine_v}")


def check_exported(who: str, exported, kind: str, count: int, rows: dict):
    """`exported` is an export of `kind` with `count` wearers and the tensors `rows` (name -> (dtype, shape tail)); ValueError otherwise."""
    if not isinstance(exported, dict) or not isinstance(exported.get("meta"), dict) or exported["meta"].get("kind") != kind:
        raise ValueError(f"tip_amd.{who}: `exported` is what export_slots of the same kind of object returned")
    for name, (dt, tail) in rows.items():
        t = exported.get(name)
        if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (count,) + tuple(tail):
            got = (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"tip_amd.{who}: exported[{name!r}] is {dt} [{count}{''.join(', ' + str(s) for s in tail)}] — one row per "
                             f"listed slot; got {got}")
    for k, v in exported.get("per", {}).items():
        if len(v) != count:
            raise ValueError(f"tip_amd.{who}: exported['per'][{k!r}] has {len(v)} entries for {count} slots")


_ENGINE_WHAT = {"window": "the window length", "nx": "the model shape (x_imu columns)", "ns": "the model shape (size_s)",
                "block_bytes": "the stream block size"}


def engine_rows(meta):
    ns = int(meta["ns"])
    return {"block": (torch.uint8, (int(meta["block_bytes"]),)), "s_rest": (torch.float32, (111,)), "c_t": (torch.float32, (ns - 111,)),
            "y": (torch.float32, (ns,)), "rows": (torch.int32, ()), "s_init": (torch.float32, (114,))}


def check_engine_import(meta: dict, n: int, attached, slots, exported, who="StaggeredStreamingEngine.import_slots"):
    """The host side of an engine import: the list (in range, no duplicates), the export (kind, one row per slot), the shapes (window,
    model shape, block size: ValueError) and the destination slots (attached: RuntimeError).  Returns the slots as ints."""
    idx = slot_list(slots, n, who)
    check_meta(who, {k: meta[k] for k in _ENGINE_WHAT}, exported.get("meta", {}) if isinstance(exported, dict) else {}, _ENGINE_WHAT)
    check_exported(who, exported, "engine", len(idx), engine_rows(meta))
    if "age" not in exported.get("per", {}):
        raise ValueError(f"tip_amd.{who}: exported['per']['age'] (each wearer's age in frames) is missing")
    for i in idx:
        if attached[i]:
            raise RuntimeError(f"tip_amd.{who}: slot {i} is attached (detach it first: an import never overwrites a live wearer)")
    return idx


_FRONT_WHAT = {"fill": "fill=", "block_bytes": "the calibration block size", "fill_block_bytes": "the fill block size"}
_SIMPLE_WHAT = {"depth": "depth=", "block_bytes": "the block size"}
_TRACKER_WHAT = {"tracker": "the kind of tracker", "grid_num": "grid_num (map_bound / grid_size)", "max_regions": "max_regions",
                 "multi_sbp": "multi_sbp", "skel": "the skeleton table", "block_bytes": "the block size"}      # (in the order checked)


def check_front_import(meta, n, slots, exported, who="SensorFrontEnd.import_slots"):
    idx = slot_list(slots, n, who)
    check_meta(who, {k: meta[k] for k in _FRONT_WHAT}, exported.get("meta", {}) if isinstance(exported, dict) else {}, _FRONT_WHAT)
    rows = {"cal": (torch.uint8, (int(meta["block_bytes"]),))}
    if meta["fill"]:
        rows["fill"] = (torch.uint8, (int(meta["fill_block_bytes"]),))
    check_exported(who, exported, "front", len(idx), rows)
    if "phase" not in exported.get("per", {}):
        raise ValueError(f"tip_amd.{who}: exported['per']['phase'] (the calibration phases) is missing")
    return idx


def check_simple_import(meta, n, slots, exported, kind, who):
    idx = slot_list(slots, n, who)
    check_meta(who, {k: meta[k] for k in _SIMPLE_WHAT if k in meta}, exported.get("meta", {}) if isinstance(exported, dict) else {},
               _SIMPLE_WHAT)
    check_exported(who, exported, kind, len(idx), {"block": (torch.uint8, (int(meta["block_bytes"]),))})
    return idx


def tracker_rows(meta):
    rows = {"block": (torch.uint8, (int(meta["block_bytes"]),)), "scale": (torch.float32, ()), "root": (torch.float32, (3,)),
            "viz_locs": (torch.float32, (5, 3))}
    if meta["tracker"] == 1:
        rows.update(q_hist=(torch.float32, (54,)), fire=(torch.int32, ()))
    return rows


def check_tracker_import(meta, n, scaled: bool, slots, exported, who):
    """As the others; and a destination that has never been given scales (scaled False: it runs the unscaled entries) refuses a wearer
    whose scale is not 1."""
    idx = slot_list(slots, n, who)
    check_meta(who, {k: meta[k] for k in _TRACKER_WHAT}, exported.get("meta", {}) if isinstance(exported, dict) else {}, _TRACKER_WHAT)
    check_exported(who, exported, "tracker", len(idx), tracker_rows(meta))
    sc = exported.get("per", {}).get("scale")
    if sc is None:
        raise ValueError(f"tip_amd.{who}: exported['per']['scale'] (the wearers' body scales) is missing")
    if not scaled and any(float(s) != 1.0 for s in sc):
        raise ValueError(f"tip_amd.{who}: a wearer's body scale is not 1 ({[float(s) for s in sc]}) and this tracker has never been given "
                         "scales (it runs the unscaled entries): reset(slots, rows, scales=...) on it first")
    return idx


# ---- device plumbing ---------------------------------------------------------------------------------------------------------------------
def _to(t, device):
    """A tensor on `device` without a synchronising copy: host tensors go through pinned memory, non-blocking."""
    device = torch.device(device)
    if t.device == device:
        return t
    if t.is_cuda:
        return t.to(device, non_blocking=True)
    return (t if t.is_pinned() else t.pin_memory()).to(device, non_blocking=True)


def _slots_dev(idx, device):
    """The list on the device as (int32, int64), one upload."""
    s64 = torch.tensor(idx, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
    return s64.to(torch.int32), s64


def _state_bytes(fn, *args) -> int:
    nbytes = ctypes.c_size_t()
    _lib.check(getattr(_lib.load(), fn)(*args, ctypes.byref(nbytes)))
    return int(nbytes.value)


def blocks_out(buf, n: int, block: int, s32, device):
    """tip_handover_export: block s32[j] of `buf` (n blocks of `block` bytes) -> row j of a new uint8 [count, block]."""
    out = torch.empty((int(s32.shape[0]), block), dtype=torch.uint8, device=device)
    if s32.shape[0]:
        _lib.check(_lib.load().tip_handover_export(buf.data_ptr(), n, block, s32.data_ptr(), int(s32.shape[0]), out.data_ptr(), block,
                                                   _lib.current_stream(device)))
    return out


def blocks_in(buf, n: int, block: int, s32, rows, device):
    """tip_handover_import: row j of `rows` (contiguous uint8 [count, block] on `device`) -> block s32[j] of `buf`."""
    if s32.shape[0]:
        _lib.check(_lib.load().tip_handover_import(buf.data_ptr(), n, block, s32.data_ptr(), int(s32.shape[0]), rows.data_ptr(), block,
                                                   _lib.current_stream(device)))


# ---- the streaming engine ----------------------------------------------------------------------------------------------------------------
def engine_meta(eng) -> dict:
    return {"kind": "engine", "window": eng.window, "nx": eng.nx, "ns": eng.ns,
            "block_bytes": _state_bytes("tip_stream_state_bytes_w", 1, eng.window)}


@torch.no_grad()
def export_engine(eng, slots) -> dict:
    who = "StaggeredStreamingEngine.export_slots"
    idx = slot_list(slots, eng.n, who)
    for i in idx:
        if not eng._attached[i]:
            raise RuntimeError(f"tip_amd.{who}: slot {i} is detached (a hand-over moves live wearers)")
    meta = engine_meta(eng)
    per = {"age": [int(eng.frame - eng._attach_frame[i]) for i in idx]}
    dev = eng.device
    with torch.cuda.device(dev):
        if eng.compact:
            eng._flush()                       # a pending attach of an exported slot runs first (and the map goes up)
        s32, s64 = _slots_dev(idx, dev)
        out = {"meta": meta, "per": per, "block": blocks_out(eng.state, eng.n, meta["block_bytes"], s32, dev),
               "s_rest": eng.s_rest.index_select(0, s64), "c_t": eng.c_t.index_select(0, s64)}
        if eng.compact:
            eng._s_host_settle()
            out["y"], out["rows"] = eng.y_slot.index_select(0, s64), eng.rows_slot.index_select(0, s64)
            out["s_init"] = _to(eng.s_host[idx].contiguous(), dev)
        else:
            y = eng._y_last
            out["y"] = (y.index_select(0, s64) if y is not None and y.shape[0] == eng.n
                        else torch.full((len(idx), eng.ns), float("nan"), dtype=torch.float32, device=dev))
            out["rows"] = (eng.rows.index_select(0, s64) if eng.frame else torch.full((len(idx),), -1, dtype=torch.int32, device=dev))
            out["s_init"] = eng.s_cur.index_select(0, s64)
    return out


def adopt_slots(eng, idx, ages):
    """The host bookkeeping of an engine import (no device): the slots are attached at the age they had, and a compact pool gives each a
    window position exactly as attach() does — SlotPositions.attach, the map uploaded by the next frame's flush."""
    for i, age in zip(idx, ages):
        eng._attached[i] = True
        eng._attach_frame[i] = eng.frame - int(age)
        if eng.compact:
            eng._map_dirty |= eng._positions.attach(i)


@torch.no_grad()
def import_engine(eng, slots, exported):
    idx = check_engine_import(engine_meta(eng), eng.n, eng._attached, slots, exported)
    if not idx:
        return
    dev, meta = eng.device, exported["meta"]
    with torch.cuda.device(dev):
        if eng.compact:
            eng._flush()                       # (a pending detach of a destination slot would wipe its y_last / T rows AFTER the import)
        s32, s64 = _slots_dev(idx, dev)
        block = _to(exported["block"], dev).contiguous()
        eng.handover_refused = torch.full((len(idx),), -1, dtype=torch.int32, device=dev)      # the kernel's own check, never read here
        _lib.check(eng.lib.tip_handover_stream_import(eng.state.data_ptr(), eng.n, s32.data_ptr(), len(idx), block.data_ptr(),
                                                      int(meta["block_bytes"]), eng.window, eng.handover_refused.data_ptr(), eng._stream()))
        eng.s_rest.index_copy_(0, s64, _to(exported["s_rest"], dev))
        eng.c_t.index_copy_(0, s64, _to(exported["c_t"], dev))
        s_init = _to(exported["s_init"], dev)
        eng.s_cur.index_copy_(0, s64, s_init)
        if eng.compact:
            eng.y_slot.index_copy_(0, s64, _to(exported["y"], dev))
            eng.rows_slot.index_copy_(0, s64, _to(exported["rows"], dev))
            eng._s_host_settle()
            if exported["s_init"].is_cuda:     # the rows reach s_host behind an event (StaggeredStreamingEngine._s_host_settle)
                pinned = torch.empty((len(idx), 114), dtype=torch.float32).pin_memory()
                pinned.copy_(s_init, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                eng._s_arriving.append((ev, idx, pinned))
            else:
                eng.s_host[idx] = exported["s_init"]
        else:
            eng.rows.index_copy_(0, s64, _to(exported["rows"], dev))
            if eng._y_last is not None and eng._y_last.shape[0] == eng.n:
                eng._y_last.index_copy_(0, s64, _to(exported["y"], dev))
    adopt_slots(eng, idx, exported["per"]["age"])


# ---- the sensor front end, the resampler, the clock --------------------------------------------------------------------------------------
def front_meta(front) -> dict:
    return {"kind": "front", "fill": bool(front.fill), "block_bytes": _state_bytes("tip_sensor_state_bytes", 1),
            "fill_block_bytes": _state_bytes("tip_fill_state_bytes", 1) if front.fill else 0}


@torch.no_grad()
def export_front(front, slots) -> dict:
    idx = slot_list(slots, front.n, "SensorFrontEnd.export_slots")
    meta, dev = front_meta(front), front.device
    out = {"meta": meta, "per": {"phase": [int(front.mirror.phase[i]) for i in idx]}}
    with torch.cuda.device(dev):
        s32, _ = _slots_dev(idx, dev)
        out["cal"] = blocks_out(front.cal, front.n, meta["block_bytes"], s32, dev)
        if front.fill:
            out["fill"] = blocks_out(front.fill_state, front.n, meta["fill_block_bytes"], s32, dev)
    return out


@torch.no_grad()
def import_front(front, slots, exported):
    meta = front_meta(front)
    idx = check_front_import(meta, front.n, slots, exported)
    if not idx:
        return
    dev = front.device
    with torch.cuda.device(dev):
        s32, _ = _slots_dev(idx, dev)
        blocks_in(front.cal, front.n, meta["block_bytes"], s32, _to(exported["cal"], dev).contiguous(), dev)
        if front.fill:
            blocks_in(front.fill_state, front.n, meta["fill_block_bytes"], s32, _to(exported["fill"], dev).contiguous(), dev)
    for i, ph in zip(idx, exported["per"]["phase"]):
        front.mirror.phase[i] = int(ph)


def simple_meta(obj, kind) -> dict:
    if kind == "resampler":
        return {"kind": kind, "depth": int(obj.depth), "block_bytes": _state_bytes("tip_resample_state_bytes", 1, int(obj.depth))}
    if kind == "poses":         # (display.block_bytes is tip_pose_state_bytes(1, depth) on the host: a refusal needs no library)
        from .display import block_bytes
        return {"kind": kind, "depth": int(obj.depth), "block_bytes": block_bytes(obj.depth)}
    return {"kind": kind, "block_bytes": _state_bytes("tip_clock_state_bytes", 1)}


_SIMPLE_NAME = {"resampler": "sensors.PacketResampler", "clock": "sensors.ClockSync", "poses": "display.PoseResampler"}


@torch.no_grad()
def export_simple(obj, slots, kind) -> dict:
    idx = slot_list(slots, obj.n, f"{_SIMPLE_NAME[kind]}.export_slots")
    meta, dev = simple_meta(obj, kind), obj.device
    with torch.cuda.device(dev):
        s32, _ = _slots_dev(idx, dev)
        return {"meta": meta, "per": {}, "block": blocks_out(obj.state, obj.n, meta["block_bytes"], s32, dev)}


@torch.no_grad()
def import_simple(obj, slots, exported, kind):
    meta = simple_meta(obj, kind)
    idx = check_simple_import(meta, obj.n, slots, exported, kind, f"{_SIMPLE_NAME[kind]}.import_slots")
    if not idx:
        return
    dev = obj.device
    with torch.cuda.device(dev):
        s32, _ = _slots_dev(idx, dev)
        blocks_in(obj.state, obj.n, meta["block_bytes"], s32, _to(exported["block"], dev).contiguous(), dev)


# ---- the trackers --------------------------------------------------------------------------------------------------------------------------
def tracker_meta(t) -> dict:
    kind = _TRACKER_KINDS[t._name]
    st = t._s
    if kind == 1:
        block, extra = _state_bytes("tip_terrain_state_bytes", 1, st.G, st.M), (st.G, st.M, int(st.flags) & 1)
    else:
        block, extra = _state_bytes("tip_kin_carry_bytes", 1), (0, 0, 0)
    return {"kind": "tracker", "tracker": kind, "block_bytes": block, "grid_num": extra[0], "max_regions": extra[1], "multi_sbp": extra[2],
            "skel": st.skel.pack()}


@torch.no_grad()
def export_tracker(t, slots) -> dict:
    idx = slot_list(slots, t.n, f"{t._slot_who}.export_slots")
    meta, dev = tracker_meta(t), t.device
    out = {"meta": meta, "per": {"scale": [float(t._scale_host[i]) for i in idx]}}
    with torch.cuda.device(dev):
        s32, s64 = _slots_dev(idx, dev)
        out["block"] = blocks_out(t._s.buf, t.n, meta["block_bytes"], s32, dev)
        out["scale"] = t.scale.index_select(0, s64)
        out["root"], out["viz_locs"] = t.root.index_select(0, s64), t.viz_locs.index_select(0, s64)
        if meta["tracker"] == 1:
            out["q_hist"], out["fire"] = t.q_hist.index_select(0, s64), t.fire.index_select(0, s64)
    return out


@torch.no_grad()
def import_tracker(t, slots, exported):
    meta = tracker_meta(t)
    idx = check_tracker_import(meta, t.n, t._s.scale is not None, slots, exported, f"{t._slot_who}.import_slots")
    if not idx:
        return
    dev = t.device
    with torch.cuda.device(dev):
        s32, s64 = _slots_dev(idx, dev)
        blocks_in(t._s.buf, t.n, meta["block_bytes"], s32, _to(exported["block"], dev).contiguous(), dev)
        if t._s.scale is not None:
            t.scale.index_copy_(0, s64, _to(exported["scale"], dev))
        t.root.index_copy_(0, s64, _to(exported["root"], dev))
        t.viz_locs.index_copy_(0, s64, _to(exported["viz_locs"], dev))
        if meta["tracker"] == 1:
            t.q_hist.index_copy_(0, s64, _to(exported["q_hist"], dev))
            fire = _to(exported["fire"], dev)          # its entries are SLOT indices (feed_back's list): rewritten to the new slots
            t.fire.index_copy_(0, s64, torch.where(fire >= 0, s32, torch.full_like(s32, -1)))
    for i, s in zip(idx, exported["per"]["scale"]):
        t._scale_host[i] = float(s)


# ---- a set of wearers ----------------------------------------------------------------------------------------------------------------------
def expected_block_bytes(meta: dict) -> dict:
    """What THIS library says the blocks of a component with `meta`'s shape parameters measure (host only): {meta key: bytes}."""
    kind = meta.get("kind")
    if kind == "engine":
        return {"block_bytes": _state_bytes("tip_stream_state_bytes_w", 1, int(meta["window"]))}
    if kind == "front":
        return {"block_bytes": _state_bytes("tip_sensor_state_bytes", 1),
                "fill_block_bytes": _state_bytes("tip_fill_state_bytes", 1) if meta["fill"] else 0}
    if kind == "resampler":
        return {"block_bytes": _state_bytes("tip_resample_state_bytes", 1, int(meta["depth"]))}
    if kind == "clock":
        return {"block_bytes": _state_bytes("tip_clock_state_bytes", 1)}
    if kind == "poses":
        return {"block_bytes": _state_bytes("tip_pose_state_bytes", 1, int(meta["depth"]))}
    if kind == "tracker":
        if int(meta["tracker"]) == 1:
            return {"block_bytes": _state_bytes("tip_terrain_state_bytes", 1, int(meta["grid_num"]), int(meta["max_regions"]))}
        return {"block_bytes": _state_bytes("tip_kin_carry_bytes", 1)}
    raise ValueError(f"tip_amd.handover: unknown component kind {kind!r}")


class Wearers:
    """A set of `count` wearers: per component of the chain (COMPONENTS) what its export_slots returned.  `header` is plain data:
    TIP_ABI_VERSION, the count, and per component the block size and shape parameters (its meta).
    to(device) / cpu() move every tensor through pinned memory without blocking (the host path is also how a wearer reaches another
    GPU); save(path) / load(path) keep them as a plain .npz of byte and number arrays — no pickled objects, loaded with
    allow_pickle=False; select(indices) takes some of the wearers."""

    def __init__(self, count: int, parts: dict, abi: int = _lib.TIP_ABI_VERSION):
        unknown = set(parts) - set(COMPONENTS)
        if unknown:
            raise ValueError(f"tip_amd.handover.Wearers: unknown components {sorted(unknown)} (known: {COMPONENTS})")
        self.count, self.parts, self.abi = int(count), dict(parts), int(abi)
        self._ready = None       # an event behind the last non-blocking copy to the host

    @property
    def header(self) -> dict:
        h = {"abi": self.abi, "count": self.count}
        h.update({name: dict(p["meta"]) for name, p in self.parts.items()})
        return h

    def _tensors(self):
        for name, p in self.parts.items():
            for k, v in p.items():
                if isinstance(v, torch.Tensor):
                    yield name, k, v

    @property
    def device(self):
        for _, _, v in self._tensors():
            return v.device
        return torch.device("cpu")

    def wait(self):
        """Block until a cpu() before this has landed (save(), select() and numpy readers call it; the device path never does)."""
        if self._ready is not None:
            self._ready.synchronize()
            self._ready = None
        return self

    def _moved(self, move):
        parts = {name: {k: (move(v) if isinstance(v, torch.Tensor) else v) for k, v in p.items()} for name, p in self.parts.items()}
        return Wearers(self.count, parts, self.abi)

    def to(self, device) -> "Wearers":
        device = torch.device(device)
        if device.type == "cpu":
            return self.cpu()
        self.wait()
        return self._moved(lambda t: _to(t, device))

    def cpu(self) -> "Wearers":
        src = self.device
        if src.type == "cpu":
            return self
        with torch.cuda.device(src):
            w = self._moved(lambda t: torch.empty(t.shape, dtype=t.dtype).pin_memory().copy_(t, non_blocking=True))
            w._ready = torch.cuda.Event()
            w._ready.record()
        return w

    def select(self, indices) -> "Wearers":
        idx = [int(i) for i in indices]
        if any(i < 0 or i >= self.count for i in idx):
            raise ValueError(f"tip_amd.handover.Wearers.select: index outside [0, {self.count})")
        self.wait()
        parts = {}
        for name, p in self.parts.items():
            q = {"meta": dict(p["meta"]), "per": {k: [v[i] for i in idx] for k, v in p.get("per", {}).items()}}
            for k, v in p.items():
                if isinstance(v, torch.Tensor):
                    q[k] = v.index_select(0, torch.tensor(idx, dtype=torch.int64, device=v.device))
            parts[name] = q
        return Wearers(len(idx), parts, self.abi)

    # ---- files: "header/abi", "header/count", "<component>/meta/<key>", "<component>/per/<key>", "<component>/<tensor>" ----------------
    def save(self, path):
        self.wait()
        arrays = {"header/abi": np.int64(self.abi), "header/count": np.int64(self.count)}
        for name, p in self.parts.items():
            for k, v in p["meta"].items():
                arrays[f"{name}/meta/{k}"] = np.frombuffer(v.encode(), dtype=np.uint8) if isinstance(v, str) else np.asarray(v)
            for k, v in p.get("per", {}).items():
                arrays[f"{name}/per/{k}"] = np.asarray(v)
            for k, v in p.items():
                if isinstance(v, torch.Tensor):
                    arrays[f"{name}/{k}"] = v.detach().cpu().numpy()
        bad = [k for k, a in arrays.items() if np.asarray(a).dtype == object]
        if bad:
            raise ValueError(f"tip_amd.handover.Wearers.save: {bad} are not plain numbers")
        with open(path, "wb") as f:
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path) -> "Wearers":
        """The wearers of a file save() wrote, on the host.  Refused (ValueError): a file written under another TIP_ABI_VERSION, and one
        whose header states a block size that this library does not give the same shape parameters — its blocks would be read at
        another layout's offsets."""
        who = "tip_amd.handover.Wearers.load"
        with np.load(path, allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        if "header/abi" not in arrays or "header/count" not in arrays:
            raise ValueError(f"{who}: {path} is not a wearers file (no header)")
        abi, count = int(arrays["header/abi"]), int(arrays["header/count"])
        if abi != _lib.TIP_ABI_VERSION:
            raise ValueError(f"{who}: the file was written under TIP_ABI_VERSION {abi}, this library is {_lib.TIP_ABI_VERSION}")
        parts = {}
        for key, a in arrays.items():
            name, _, rest = key.partition("/")
            if name == "header":
                continue
            p = parts.setdefault(name, {"meta": {}, "per": {}})
            if rest.startswith("meta/"):
                k = rest[5:]
                p["meta"][k] = bytes(a).decode() if k == "kind" else (a.item() if a.ndim == 0 else a)
            elif rest.startswith("per/"):
                p["per"][rest[4:]] = a.tolist()
            else:
                p[rest] = torch.from_numpy(np.ascontiguousarray(a))
        for name, p in parts.items():
            for k, v in expected_block_bytes(p["meta"]).items():
                if int(p["meta"].get(k, -1)) != v:
                    raise ValueError(f"{who}: the file's {name} blocks are {p['meta'].get(k)} bytes ({k}); this library lays the same shape "
                                     f"out in {v}")
            for k, v in p.items():
                if isinstance(v, torch.Tensor) and (v.dim() < 1 or v.shape[0] != count):
                    raise ValueError(f"{who}: {name}/{k} has {tuple(v.shape)} for {count} wearers")
        return cls(count, parts, abi)


def _chain(who, engine, front, resampler, clock, tracker, poses=None):
    given = {k: v for k, v in zip(COMPONENTS, (engine, front, resampler, clock, tracker, poses)) if v is not None}
    if not given:
        raise ValueError(f"tip_amd.handover.{who}: give at least one of engine=, front=, resampler=, clock=, tracker=, poses=")
    return given


def export_wearers(slots, engine=None, front=None, resampler=None, clock=None, tracker=None, poses=None) -> Wearers:
    """The wearers in `slots` of every object given — one chain serving the same slots — as they stand.  Nothing is detached or reset.
    poses: the chain's display.PoseResampler, whose rings of recent poses travel with the wearers."""
    given = _chain("export_wearers", engine, front, resampler, clock, tracker, poses)
    idx = [int(i) for i in slots]
    return Wearers(len(idx), {name: obj.export_slots(idx) for name, obj in given.items()})


def import_wearers(wearers: Wearers, slots, engine=None, front=None, resampler=None, clock=None, tracker=None, poses=None):
    """Put `wearers` into `slots` of the objects given: wearer j goes to slots[j] of each.  Every component the wearers hold must be
    given, and the reverse (ValueError); every object checks its part on the host before ANY of them launches."""
    who = "import_wearers"
    if not isinstance(wearers, Wearers):
        raise ValueError(f"tip_amd.handover.{who}: wearers is a handover.Wearers")
    given = _chain(who, engine, front, resampler, clock, tracker, poses)
    if set(given) != set(wearers.parts):
        raise ValueError(f"tip_amd.handover.{who}: the wearers hold {sorted(wearers.parts)}, the call gives {sorted(given)} — every component "
                         "of one must be in the other")
    if wearers.abi != _lib.TIP_ABI_VERSION:
        raise ValueError(f"tip_amd.handover.{who}: the wearers were exported under TIP_ABI_VERSION {wearers.abi}, this library is "
                         f"{_lib.TIP_ABI_VERSION}")
    idx = [int(i) for i in slots]
    if len(idx) != wearers.count:
        raise ValueError(f"tip_amd.handover.{who}: {len(idx)} slots for {wearers.count} wearers")
    wearers.wait()
    # the host checks of every component first: a refusal leaves every object as it was
    for name, obj in given.items():
        p = wearers.parts[name]
        if name == "engine":
            if not hasattr(obj, "_attached"):
                obj.import_slots(idx, p)      # (the lock-step engine: raises)
            check_engine_import(engine_meta(obj), obj.n, obj._attached, idx, p)
        elif name == "front":
            check_front_import(front_meta(obj), obj.n, idx, p)
        elif name == "tracker":
            check_tracker_import(tracker_meta(obj), obj.n, obj._s.scale is not None, idx, p, f"{obj._slot_who}.import_slots")
        else:
            check_simple_import(simple_meta(obj, name), obj.n, idx, p, name, f"{_SIMPLE_NAME[name]}.import_slots")
    for name, obj in given.items():
        obj.import_slots(idx, wearers.parts[name])
