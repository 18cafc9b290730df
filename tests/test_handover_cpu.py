"""CPU tests of wearer hand-over (tip_amd.handover; include/tip_hip.h, "hand-over"): the C-ABI surface, every refusal — raised on the
host, with no device and nothing launched — the wearers file, and the bookkeeping of a compact import."""
import os
import re
import types

import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import handover
from tip_amd import lib as tlib
from tip_amd.streaming import SlotPositions
from conftest import ROOT

NAMES = {"tip_handover_export", "tip_handover_import", "tip_handover_stream_import"}


def test_c_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    assert set(re.findall(r"TIP_API int (tip_handover_\w+)\(", hdr)) == NAMES == {n for n in tlib.EXPORTS if n.startswith("tip_handover_")}
    lib = tlib.load()
    assert all(hasattr(lib, n) for n in NAMES) and tlib.TIP_ABI_VERSION == 5 == lib.tip_abi_version()
    assert "hand-over" in hdr and "tip_handover.hip" in open(os.path.join(os.path.dirname(tlib.CSRC), "csrc", "Makefile")).read()
    assert "handover" in dir(tip_amd) or tip_amd.handover is handover           # re-exported lazily like the other modules


def test_entry_points_refuse_before_any_launch():
    """Null pointers, block_bytes 0 or no multiple of 4, a stride below the block or no multiple of 4, misaligned bases, negative counts,
    a window outside [1, 128]: TIP_ERR_INVALID_ARG with no device in the machine; count 0 is TIP_OK."""
    lib = tlib.load()
    p, q, s = 4096, 8192, 1024             # (never dereferenced: every call here returns before a launch)
    bad = [(None, 4, 32, s, 1, q, 32), (p, 4, 32, s, 1, None, 32), (p, 4, 32, None, 1, q, 32), (p, 4, 0, s, 1, q, 32),
           (p, 4, 30, s, 1, q, 32), (p, 4, 32, s, 1, q, 28), (p, 4, 32, s, 1, q, 34), (p + 2, 4, 32, s, 1, q, 32),
           (p, 4, 32, s, 1, q + 2, 32), (p, 4, 32, s + 1, 1, q, 32), (p, 4, 32, s, -1, q, 32), (p, -1, 32, s, 1, q, 32)]
    for fn in (lib.tip_handover_export, lib.tip_handover_import):
        for args in bad:
            assert fn(*args, None) == -1, args
        assert fn(p, 4, 32, None, 0, q, 32, None) == 0
    for W in (0, -3, 129):
        assert lib.tip_handover_stream_import(p, 4, s, 1, q, 64, W, None, None) == -1
    assert lib.tip_handover_stream_import(p, 4, s, 1, q, 41984 - 4, 40, None, None) == -1          # a stride below the 40-row block
    assert lib.tip_handover_stream_import(None, 4, s, 1, q, 41984, 40, None, None) == -1
    assert lib.tip_handover_stream_import(p, 4, None, 0, q, 41984, 40, None, None) == 0


# ---- fabricated exports: what export_slots returns, on the host ---------------------------------------------------------------------------------
def _engine_meta(window=40, nx=90, ns=131):
    return {"kind": "engine", "window": window, "nx": nx, "ns": ns, "block_bytes": handover.expected_block_bytes({"kind": "engine", "window": window})["block_bytes"]}


def _engine_export(count, seed=0, **kw):
    meta = _engine_meta(**kw)
    g = torch.Generator().manual_seed(seed)
    rows = handover.engine_rows(meta)
    out = {"meta": meta, "per": {"age": [3 + 17 * j for j in range(count)]}}
    for k, (dt, tail) in rows.items():
        shape = (count,) + tuple(tail)
        out[k] = (torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) if dt == torch.uint8 else
                  torch.randint(-1, 40, shape, generator=g, dtype=torch.int32) if dt == torch.int32 else torch.randn(shape, generator=g))
    return out


def test_engine_import_refusals():
    meta, w = _engine_meta(), _engine_export(2)
    free = [False] * 4
    assert handover.check_engine_import(meta, 4, free, [3, 1], w) == [3, 1]
    for slots, match in (([0, 0], "duplicate slot index"), ([0, 4], "slot index outside"), ([-1, 0], "slot index outside"), ([0], "one row per")):
        with pytest.raises(ValueError, match=match):
            handover.check_engine_import(meta, 4, free, slots, w)
    with pytest.raises(RuntimeError, match="slot 1 is attached"):
        handover.check_engine_import(meta, 4, [False, True, False, False], [3, 1], w)
    for other, match in ((dict(window=7), "window length differs"), (dict(ns=119), "model shape"), (dict(nx=72), "model shape")):
        with pytest.raises(ValueError, match=match):
            handover.check_engine_import(_engine_meta(**other), 4, free, [3, 1], w)
    small = dict(w, meta=dict(w["meta"], block_bytes=41980))
    with pytest.raises(ValueError, match="stream block size differs"):
        handover.check_engine_import(meta, 4, free, [3, 1], small)
    with pytest.raises(ValueError, match="export_slots of the same kind"):
        handover.check_engine_import(meta, 4, free, [3, 1], dict(w, meta=dict(w["meta"], kind="clock")))
    with pytest.raises(ValueError, match="exported\\['s_rest'\\]"):
        handover.check_engine_import(meta, 4, free, [3, 1], dict(w, s_rest=w["s_rest"][:, :100]))


def test_front_resampler_clock_tracker_refusals():
    cal, fill = torch.zeros((1, 1536), dtype=torch.uint8), torch.zeros((1, 1632), dtype=torch.uint8)
    on = {"kind": "front", "fill": True, "block_bytes": 1536, "fill_block_bytes": 1632}
    off = {"kind": "front", "fill": False, "block_bytes": 1536, "fill_block_bytes": 0}
    ex = {"meta": on, "per": {"phase": [3]}, "cal": cal, "fill": fill}
    assert handover.check_front_import(on, 2, [1], ex) == [1]
    with pytest.raises(ValueError, match="fill= differs"):
        handover.check_front_import(off, 2, [1], ex)
    with pytest.raises(ValueError, match="fill= differs"):
        handover.check_front_import(on, 2, [1], {"meta": off, "per": {"phase": [3]}, "cal": cal})
    with pytest.raises(ValueError, match="slot index outside"):
        handover.check_front_import(on, 2, [2], ex)
    rs = {"kind": "resampler", "depth": 8, "block_bytes": 1424}
    exr = {"meta": rs, "per": {}, "block": torch.zeros((2, 1424), dtype=torch.uint8)}
    assert handover.check_simple_import(rs, 4, [0, 2], exr, "resampler", "sensors.PacketResampler.import_slots") == [0, 2]
    with pytest.raises(ValueError, match="depth= differs"):
        handover.check_simple_import(dict(rs, depth=4, block_bytes=720), 4, [0, 2], exr, "resampler", "sensors.PacketResampler.import_slots")
    ck = {"kind": "clock", "block_bytes": 32}
    with pytest.raises(ValueError, match="export_slots of the same kind"):
        handover.check_simple_import(ck, 4, [0, 2], {"meta": dict(rs, block_bytes=32), "per": {}, "block": torch.zeros((2, 32), dtype=torch.uint8)},
                                     "clock", "sensors.ClockSync.import_slots")
    skel = np.arange(1568, dtype=np.uint8)
    tm = {"kind": "tracker", "tracker": 1, "block_bytes": 42304, "grid_num": 100, "max_regions": 64, "multi_sbp": 1, "skel": skel}
    ext = {"meta": tm, "per": {"scale": [0.875]}, "block": torch.zeros((1, 42304), dtype=torch.uint8), "scale": torch.ones(1),
           "root": torch.zeros((1, 3)), "viz_locs": torch.zeros((1, 5, 3)), "q_hist": torch.zeros((1, 54)),
           "fire": torch.zeros(1, dtype=torch.int32)}
    who = "terrain.TerrainTracker.import_slots"
    assert handover.check_tracker_import(tm, 3, True, [2], ext, who) == [2]
    with pytest.raises(ValueError, match="body scale is not 1"):
        handover.check_tracker_import(tm, 3, False, [2], ext, who)
    assert handover.check_tracker_import(tm, 3, False, [2], dict(ext, per={"scale": [1.0]}), who) == [2]
    for change, match in ((dict(grid_num=20, block_bytes=2304 + 1600), "grid_num"), (dict(max_regions=4), "max_regions"), (dict(multi_sbp=0), "multi_sbp"),
                          (dict(skel=skel[::-1].copy()), "skeleton table"), (dict(tracker=0), "kind of tracker")):
        with pytest.raises(ValueError, match=match):
            handover.check_tracker_import(dict(tm, **change), 3, True, [2], ext, who)


def test_import_wearers_asks_for_the_same_components():
    w = handover.Wearers(2, {"engine": _engine_export(2)})
    stub = types.SimpleNamespace()
    with pytest.raises(ValueError, match="every component"):
        handover.import_wearers(w, [0, 1], engine=stub, clock=stub)
    with pytest.raises(ValueError, match="every component"):
        handover.import_wearers(w, [0, 1], front=stub)
    with pytest.raises(ValueError, match="give at least one"):
        handover.import_wearers(w, [0, 1])
    with pytest.raises(ValueError, match="unknown components"):
        handover.Wearers(1, {"pool": {}})
    old = handover.Wearers(2, {"engine": _engine_export(2)}, abi=4)
    with pytest.raises(ValueError, match="TIP_ABI_VERSION 4"):
        handover.import_wearers(old, [0, 1], engine=stub)
    with pytest.raises(ValueError, match="3 slots for 2 wearers"):
        handover.import_wearers(w, [0, 1, 2], engine=stub)


# ---- the file -------------------------------------------------------------------------------------------------------------------------------------
def _resave(path, out, **changes):
    with np.load(path, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    arrays.update({k: np.asarray(v) for k, v in changes.items()})
    np.savez(out, **arrays)


def test_the_file_is_plain_arrays_and_checks_its_header(tmp_path):
    skel = np.arange(1568, dtype=np.uint8)
    tm = {"kind": "tracker", "tracker": 0, "block_bytes": 1024, "grid_num": 0, "max_regions": 0, "multi_sbp": 0, "skel": skel}
    parts = {"engine": _engine_export(3, window=7),
             "clock": {"meta": {"kind": "clock", "block_bytes": 32}, "per": {}, "block": torch.arange(96, dtype=torch.uint8).reshape(3, 32)},
             "tracker": {"meta": tm, "per": {"scale": [1.0, 0.875, 1.0625]}, "block": torch.ones((3, 1024), dtype=torch.uint8),
                         "scale": torch.tensor([1.0, 0.875, 1.0625]), "root": torch.zeros((3, 3)), "viz_locs": torch.zeros((3, 5, 3))}}
    w = handover.Wearers(3, parts)
    assert w.header["abi"] == tlib.TIP_ABI_VERSION and w.header["engine"]["window"] == 7 and w.header["clock"]["block_bytes"] == 32
    path = str(tmp_path / "w.npz")
    w.save(path)
    with np.load(path, allow_pickle=False) as z:                          # no pickled objects: every array loads, none is of dtype object
        assert all(z[k].dtype != object for k in z.files) and {"header/abi", "header/count", "engine/block", "engine/meta/window"} <= set(z.files)
    back = handover.Wearers.load(path)
    assert back.count == 3 and back.abi == w.abi and set(back.parts) == set(parts)
    for name, p in parts.items():
        q = back.parts[name]
        assert q["per"] == p["per"] and set(q["meta"]) == set(p["meta"])
        for k, v in p["meta"].items():
            assert np.array_equal(np.asarray(v), np.asarray(q["meta"][k])), (name, k)
        for k, v in p.items():
            if isinstance(v, torch.Tensor):
                assert q[k].dtype == v.dtype and torch.equal(q[k], v), (name, k)
    assert handover.check_engine_import(_engine_meta(window=7), 5, [False] * 5, [4, 0, 2], back.parts["engine"]) == [4, 0, 2]
    # select: wearers 2 and 0, in that order
    sel = back.select([2, 0])
    assert sel.count == 2 and sel.parts["engine"]["per"]["age"] == [37, 3] and sel.parts["tracker"]["per"]["scale"] == [1.0625, 1.0]
    assert torch.equal(sel.parts["clock"]["block"], parts["clock"]["block"][[2, 0]])
    with pytest.raises(ValueError, match="index outside"):
        back.select([3])
    assert back.cpu() is back and back.device.type == "cpu"
    # another ABI version, another block size: refused
    other = str(tmp_path / "other.npz")
    _resave(path, other, **{"header/abi": 4})
    with pytest.raises(ValueError, match="TIP_ABI_VERSION 4"):
        handover.Wearers.load(other)
    _resave(path, other, **{"clock/meta/block_bytes": 40})
    with pytest.raises(ValueError, match="clock blocks are 40 bytes"):
        handover.Wearers.load(other)
    _resave(path, other, **{"engine/meta/block_bytes": 41984})
    with pytest.raises(ValueError, match="engine blocks are 41984 bytes"):
        handover.Wearers.load(other)
    with pytest.raises(ValueError, match="not a wearers file"):
        np.savez(other, a=np.zeros(3))
        handover.Wearers.load(other)
    with pytest.raises(ValueError):                                       # a pickled object in the file is never unpickled
        np.savez(other, **{"header/abi": np.int64(5), "header/count": np.int64(1), "clock/meta/kind": np.array({"a": 1}, dtype=object)})
        handover.Wearers.load(other)


# ---- the bookkeeping of a compact import ------------------------------------------------------------------------------------------------------
def _pool(n, attached, frame):
    return types.SimpleNamespace(n=n, compact=True, frame=frame, _attached=[i in attached for i in range(n)], _attach_frame=[0] * n,
                                 _positions=SlotPositions(n, attached), _map_dirty=False)


def test_a_compact_import_keeps_the_books_of_an_attach():
    """Slots 5 and 1 enter a pool of 6 with slots 2 and 4 attached: window positions, position map and the attached list are what
    attach([5, 1]) leaves (SlotPositions.attach, the map marked for the next flush); only the age differs — the wearer's own."""
    a, b = _pool(6, [2, 4], 90), _pool(6, [2, 4], 90)
    handover.adopt_slots(a, [5, 1], [3, 47])
    for i in (5, 1):                                                     # StaggeredStreamingEngine.attach, compact: the host half
        b._attach_frame[i] = b.frame
        b._attached[i] = True
        b._map_dirty |= b._positions.attach(i)
    assert a._positions.slot_at == b._positions.slot_at == [2, 4, 5, 1] and a._positions.pos == b._positions.pos
    assert a._attached == b._attached and a._map_dirty and b._map_dirty and len(a._positions) == 4
    assert [a.frame - a._attach_frame[i] for i in (5, 1)] == [3, 47] and a._attach_frame[2] == 0
    # a detach behind it moves the last position into the hole, as ever
    assert a._positions.detach(2) and a._positions.slot_at == [1, 4, 5]
