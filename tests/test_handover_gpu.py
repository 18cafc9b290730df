"""GPU tests of wearer hand-over (csrc/tip_handover.hip; tip_amd.handover; export_slots / import_slots of the engines, the sensor front
end, the resampler, the clock and the trackers).  The contract is the project's own: a wearer that is handed over continues BIT FOR BIT
as in the uninterrupted run, on a plan whose per-window result does not depend on the batch (set_plan("fused"), compact=True's rule) —
so no test here has a tolerance."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sensor_oracle as so
import tip_amd
from tip_amd import handover, sensors, synth, terrain
from tip_amd import kinematics as kin
from tip_amd import lib as tlib
from test_host_cpu import make_model, load_synth
from test_terrain_cpu import golden_track

pytestmark = pytest.mark.gpu
f32 = np.float32
S = tip_amd.streaming
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tip_terrain_golden.npz"))
SHAPES = {"72x119": dict(synth.PAPER, size_s=119, with_acc_sum=False), "90x131": dict(synth.PAPER)}
_models = {}


def _model(tag="90x131", p_state=0.0):
    key = (tag, p_state)
    if key not in _models:
        m = make_model(SHAPES[tag], p_state=p_state)
        load_synth(m, SHAPES[tag], 0)
        _models[key] = m.cuda().eval()
    return _models[key]


@pytest.fixture
def fused():
    """Models pinned to the plan whose per-window bits do not depend on the batch; back to AUTO afterwards."""
    used = []

    def get(tag="90x131"):
        m = _model(tag)
        m.set_plan("fused")
        used.append(m)
        return m
    yield get
    for m in used:
        m.set_plan("auto")


def _frames(n, F, seed):
    """Random finite frames: near-identity rotation columns, unit-normal accelerations; s_init rows."""
    rng = np.random.RandomState(seed)
    raw = rng.randn(F, n, 72).astype(f32)
    raw[:, :, :54] = np.tile(np.eye(3, dtype=f32).reshape(9), 6) + 0.05 * raw[:, :, :54]
    return raw, (rng.randn(n, 114) * 0.2).astype(f32)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _snap(out, slots):
    sl = torch.tensor(slots, device="cuda")
    return {k: out[k].index_select(0, sl).clone() for k in ("s_rest", "c_t", "y_last", "T", "valid")}


def _same_rows(a, b, where):
    """Two snapshots of the same wearers: T, valid, s_rest and c_t equal bit for bit; y_last bit for bit where valid, NaN where not."""
    assert torch.equal(a["T"], b["T"]) and torch.equal(a["valid"], b["valid"]), where
    for k in ("s_rest", "c_t"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), (where, k)
    v = a["valid"]
    assert torch.equal(_bits(a["y_last"][v]), _bits(b["y_last"][v])), (where, "y_last")
    assert torch.isnan(a["y_last"][~v]).all() and torch.isnan(b["y_last"][~v]).all(), (where, "y_last of a slot without a row")


# ---- 1. continuation, stream only ----------------------------------------------------------------------------------------------------------
SRC, DST = [0, 2, 4], [2, 0, 1]
F0, F1 = 50, 45


def _engine_a(m, raw, s_init, W, compact):
    """n = 5 after F0 frames: slot 0 at age 3 (smoother priming), slot 2 at age 20 (short window), slot 4 at age W + 7 (full window),
    slot 1 detached with its state kept, slot 3 attached from the start."""
    a = S.StaggeredStreamingEngine(m, s_init, compact=compact, window=W)
    for f in range(F0):
        for slot, age in ((0, 3), (2, 20), (4, W + 7)):
            if f == F0 - age:
                a.attach([slot], s_init[[slot]])
        if f == 25:
            a.detach([1])
        a.step(raw[f])
    assert [a.frame - a._attach_frame[i] for i in SRC] == [3, 20, W + 7] and a.attached == [True, False, True, True, True]
    return a


def _handed_over(m, kind, graph, W, through=None):
    src_compact, dst_compact = kind == "compact->plain", kind == "plain->compact"
    raw, s_init = _frames(5, F0 + F1, 11)
    a = _engine_a(m, raw, s_init, W, src_compact)
    b = S.StaggeredStreamingEngine(m, np.zeros((3, 114), f32), compact=dst_compact, use_graph=graph, window=W)
    b.detach([0, 1, 2])
    b.reset()
    zero = np.zeros((3, 72), f32)
    for _ in range(2):                      # (plain + graph: captured and replayed before the import, which then lands between two replays)
        b.step(zero)
    caps = b.captures
    w = handover.export_wearers(SRC, engine=a)
    assert a.attached == [True, False, True, True, True]                 # exporting does not detach
    if through is not None:
        w = through(w)
    handover.import_wearers(w, DST, engine=b)
    assert b.attached == [True, True, True] and b.captures == caps
    return a, b, raw


def _run_on(a, b, raw, q=None):
    rb = np.zeros((3, 72), f32)
    for f in range(F0, F0 + F1):
        rb[DST] = raw[f][SRC]
        oa, ob = a.step(raw[f]), b.step(rb)
        _same_rows(_snap(oa, SRC), _snap(ob, DST), f)
        if f == F0 and q is not None:
            # override_history on a moved slot: at once where its age allows, refused by age exactly as in A
            for e, slot in ((a, SRC[0]), (b, DST[0])):
                with pytest.raises(RuntimeError, match="has not consumed a frame yet"):
                    e.override_history(q[:1], [slot])
            a.override_history(q, SRC[1:])
            b.override_history(q, DST[1:])
    torch.cuda.synchronize()
    return oa, ob


@pytest.mark.parametrize("tag", list(SHAPES))
@pytest.mark.parametrize("W", [40, 7])
@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graph"])
@pytest.mark.parametrize("kind", ["plain->plain", "plain->compact", "compact->plain"])
def test_a_moved_wearer_continues_bit_for_bit(fused, kind, graph, W, tag):
    """Engine A (n = 5) after 50 frames hands slots [0, 2, 4] — ages 3, 20 and W + 7 — to slots [2, 0, 1] of a fresh engine B (n = 3, every
    slot detached); A and B then run 45 more frames on the same rows and agree on s_rest, c_t, y_last, T and valid in every frame,
    the priming frames of the age-3 wearer included."""
    m = fused(tag)
    a, b, raw = _handed_over(m, kind, graph, W)
    q = (np.random.RandomState(5).randn(2, 54) * 0.3).astype(f32)
    oa, ob = _run_on(a, b, raw, q)
    assert bool(ob["valid"].all()) and (b.captures >= 1) == graph
    m.check_handoffs()


# ---- 4. the host round trip: the path that stands for another GPU ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain->compact", "compact->plain"])
def test_through_the_host_and_a_file(fused, tmp_path, kind):
    """Wearers.cpu().save() -> load() -> .to(device) -> import: the equality of the test above."""
    path = str(tmp_path / "wearers.npz")

    def through(w):
        h = w.cpu()
        h.save(path)
        assert all(not t.is_cuda for _, _, t in h._tensors())
        with np.load(path, allow_pickle=False) as z:
            assert all(z[k].dtype != object for k in z.files) and int(z["header/abi"]) == tlib.TIP_ABI_VERSION
        back = handover.Wearers.load(path)
        assert back.header["engine"]["block_bytes"] == w.header["engine"]["block_bytes"] and back.count == 3
        return back.to("cuda")

    m = fused()
    a, b, raw = _handed_over(m, kind, False, 40, through)
    _run_on(a, b, raw)


# ---- 5. live dropout: the blocks move, the seeds are the engine's ----------------------------------------------------------------------------
def test_live_dropout_engines_hand_over():
    m = _model("90x131", p_state=0.8)
    raw, s_init = _frames(4, 40, 17)
    a = S.StaggeredStreamingEngine(m, s_init, live_dropout=True)
    b = S.StaggeredStreamingEngine(m, np.zeros((2, 114), f32), live_dropout=True, compact=True)
    b.detach([0, 1])
    for f in range(30):
        a.step(raw[f])
    w = a.export_slots([1, 3])
    b.import_slots([1, 0], w)
    again = b.export_slots([1, 0])
    for k in ("block", "s_rest", "c_t", "s_init"):
        assert torch.equal(w[k], again[k]), k
    rb = np.zeros((2, 72), f32)
    for f in range(30, 40):
        rb[[1, 0]] = raw[f][[1, 3]]
        out = b.step(rb)
        assert bool(out["valid"].all()) and bool(torch.isfinite(out["y_last"]).all()) and bool(torch.isfinite(out["s_rest"]).all())
    m.check_handoffs()


# ---- 2. bytes ----------------------------------------------------------------------------------------------------------------------------------
def _stream_bytes(W):
    nb = ctypes.c_size_t()
    tlib.check(tlib.load().tip_stream_state_bytes_w(1, W, ctypes.byref(nb)))
    return nb.value


def _list(rng, n, count):
    """`count` distinct slots of n in random order, with a -1 and an n among them from three entries on."""
    sl = rng.permutation(n)[:count].astype(np.int32)
    if count >= 3:
        sl[1], sl[count - 1] = -1, n
    return sl


@pytest.mark.parametrize("count", [0, 1, 3, 65, 257])
@pytest.mark.parametrize("block", [32, 36, 1536, "stream"])
def test_generic_pair_moves_the_listed_blocks_and_nothing_else(block, count):
    """tip_handover_export / tip_handover_import on buffers of random bytes: rows of listed blocks equal the blocks, entries -1 and n
    leave their row / block as it was, every unlisted block and every byte between two rows keeps its sentinel — with strides that
    allow the 16-byte path and with one that is no multiple of 16 (and at 36 bytes) on the 4-byte path."""
    lib, rng = tlib.load(), np.random.RandomState(1000 + count)
    block = _stream_bytes(40) if block == "stream" else block
    n = 300
    src = torch.from_numpy(rng.randint(0, 256, size=(n, block)).astype(np.uint8)).cuda()
    sl = _list(rng, n, count)
    sl_d = torch.from_numpy(sl).cuda() if count else torch.zeros(1, dtype=torch.int32, device="cuda")
    ok = (sl >= 0) & (sl < n)
    for stride in (block, block + 16, block + 4):
        out = torch.full((max(count, 1), stride), 0xA5, dtype=torch.uint8, device="cuda")
        tlib.check(lib.tip_handover_export(src.data_ptr(), n, block, sl_d.data_ptr(), count, out.data_ptr(), stride, None))
        dst = torch.full((n + 1, block), 0x5A, dtype=torch.uint8, device="cuda")           # (one block more: a write past block n - 1 shows)
        tlib.check(lib.tip_handover_import(dst.data_ptr(), n, block, sl_d.data_ptr(), count, out.data_ptr(), stride, None))
        back = torch.full((max(count, 1), stride), 0xA5, dtype=torch.uint8, device="cuda")
        tlib.check(lib.tip_handover_export(dst.data_ptr(), n, block, sl_d.data_ptr(), count, back.data_ptr(), stride, None))
        torch.cuda.synchronize()
        o, d, s = out.cpu().numpy(), dst.cpu().numpy(), src.cpu().numpy()
        assert np.array_equal(o, back.cpu().numpy())                        # export -> import -> export: identical bytes
        if count == 0:
            assert (o == 0xA5).all() and (d == 0x5A).all()
            continue
        assert np.array_equal(o[ok, :block], s[sl[ok]]) and (o[~ok] == 0xA5).all() and (o[:, block:] == 0xA5).all()
        rest = np.ones(n + 1, bool)
        rest[sl[ok]] = False
        assert np.array_equal(d[sl[ok]], s[sl[ok]]) and (d[rest] == 0x5A).all()


def test_generic_pair_refusals():
    lib = tlib.load()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    sl = torch.zeros(4, dtype=torch.int32, device="cuda")
    p, s = buf.data_ptr(), sl.data_ptr()
    bad = [(None, 4, 32, s, 1, p + 1024, 32), (p, 4, 32, s, 1, None, 32), (p, 4, 32, None, 1, p + 1024, 32), (p, 4, 0, s, 1, p + 1024, 32),
           (p, 4, 30, s, 1, p + 1024, 32), (p, 4, 32, s, 1, p + 1024, 28), (p, 4, 32, s, 1, p + 1024, 34), (p + 2, 4, 32, s, 1, p + 1024, 32),
           (p, 4, 32, s, 1, p + 1026, 32), (p, 4, 32, s, -1, p + 1024, 32), (p, -1, 32, s, 1, p + 1024, 32)]
    for fn in (lib.tip_handover_export, lib.tip_handover_import):
        for args in bad:
            assert fn(*args, None) < 0, args
        assert fn(p, 4, 32, None, 0, p + 1024, 32, None) == 0
    for W in (0, 129):
        assert lib.tip_handover_stream_import(p, 4, s, 1, p + 1024, 64, W, None, None) < 0
    torch.cuda.synchronize()
    assert not buf.any()


@pytest.mark.parametrize("W", [40, 7])
def test_stream_import_keeps_the_shape_word_and_refuses_another_shape(W):
    """Blocks of a (5 SBPs, acc-sum) buffer into a buffer of the same shape: every byte but the shape word moves, unlisted blocks keep
    theirs; into a buffer reset for (2 SBPs, no acc-sum): skipped, reported in `refused`, the buffer untouched."""
    lib, rng = tlib.load(), np.random.RandomState(W)
    block, n = _stream_bytes(W), 6
    shp = 10474 if W == 40 else 2
    s_init = torch.zeros((n, 114), device="cuda")

    def buffer(n_sbps, acc):
        st = torch.empty(n * block, dtype=torch.uint8, device="cuda")
        tlib.check(lib.tip_stream_reset_w(st.data_ptr(), s_init.data_ptr(), n, n_sbps, acc, W, None))
        return st

    same, other = buffer(5, 1), buffer(2, 0)
    word = same.view(torch.int32)[shp].item()
    rows = rng.randint(0, 256, size=(3, block)).astype(np.uint8)
    rows.view(np.int32)[:, shp] = word                                   # recorded under `same`'s shape
    rows.view(np.int32)[2, shp] = other.view(torch.int32)[shp].item()    # ... but the third under the other
    rows_d = torch.from_numpy(rows).cuda()
    sl = torch.tensor([4, 1, 3, -1][:3], dtype=torch.int32, device="cuda")
    for dst, want in ((same, [-1, -1, 3]), (other, [4, 1, -1])):
        before = dst.clone()
        refused = torch.full((3,), 77, dtype=torch.int32, device="cuda")
        tlib.check(lib.tip_handover_stream_import(dst.data_ptr(), n, sl.data_ptr(), 3, rows_d.data_ptr(), block, W, refused.data_ptr(), None))
        torch.cuda.synchronize()
        assert refused.cpu().tolist() == want
        got, was = dst.cpu().numpy().reshape(n, block), before.cpu().numpy().reshape(n, block)
        for j, slot in enumerate([4, 1, 3]):
            if want[j] >= 0:
                assert np.array_equal(got[slot], was[slot])               # refused: the slot untouched
            else:
                exp = rows[j].copy()
                exp.view(np.int32)[shp] = was[slot].view(np.int32)[shp]   # the destination's own shape word stays
                assert np.array_equal(got[slot], exp)
        for slot in (0, 2, 5):
            assert np.array_equal(got[slot], was[slot])


@pytest.fixture(scope="module")
def skel():
    return kin.Skeleton.from_table(GOLDEN)


def _random_bytes(t, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t.copy_(torch.randint(0, 256, t.shape, generator=g, device="cuda", dtype=torch.uint8))


def test_every_component_round_trips_and_leaves_the_rest_alone(skel):
    """export -> import -> export gives identical bytes for the front end (fill=True), the resampler, the clock, both trackers — state
    buffers of random bytes, wearers 1 and 3 of n = 4 into slots 4 and 0 of n = 6 — and every other block of the destination is byte
    for byte what it was."""
    src, dst = [1, 3], [4, 0]

    def pair(make, buf):
        a, b = make(4), make(6)
        _random_bytes(buf(a), 1)
        _random_bytes(buf(b), 2)
        return a, b

    cases = [("front", *pair(lambda n: sensors.SensorFrontEnd(n, "cuda", fill=True), lambda o: o.cal), lambda o: (o.cal, o.fill_state)),
             ("resampler", *pair(lambda n: sensors.PacketResampler(n, "cuda", mode="predict", depth=4), lambda o: o.state), lambda o: (o.state,)),
             ("clock", *pair(lambda n: sensors.ClockSync(n, "cuda"), lambda o: o.state), lambda o: (o.state,)),
             ("tracker", *pair(lambda n: kin.RootTracker(skel, n, "cuda"), lambda o: o._s.buf), lambda o: (o._s.buf,)),
             ("tracker", *pair(lambda n: terrain.TerrainTracker(skel, n, "cuda", map_bound=1.0, multi_sbp=True), lambda o: o._s.buf),
              lambda o: (o._s.buf,))]
    for name, a, b, bufs in cases:
        if name == "front":
            _random_bytes(a.fill_state, 3)
            _random_bytes(b.fill_state, 4)
            a.mirror.phase[1], a.mirror.phase[3] = sensors.TPOSE, sensors.LIVE
        before = [t.clone() for t in bufs(b)]
        w = handover.export_wearers(src, **{name: a})
        handover.import_wearers(w, dst, **{name: b})
        again = handover.export_wearers(dst, **{name: b})
        torch.cuda.synchronize()
        for k, v in w.parts[name].items():
            if isinstance(v, torch.Tensor) and k != "fire":
                assert torch.equal(_bits(v), _bits(again.parts[name][k])), (name, k)
        for t, was, ta in zip(bufs(b), before, bufs(a)):
            blk = t.numel() // 6
            got, was, srcb = t.view(6, blk), was.view(6, blk), ta.view(4, blk)
            assert torch.equal(got[dst], srcb[src]), name
            assert torch.equal(got[[1, 2, 3, 5]], was[[1, 2, 3, 5]]), name
        if name == "front":
            assert [b.mirror.phase[i] for i in dst] == [sensors.TPOSE, sensors.LIVE]


def test_engine_round_trip_and_refusals(fused):
    """An engine's export -> import -> export is identical; the other slots' blocks keep their bytes; the refusals of an import come
    before anything is launched (the destination's state is what it was)."""
    m = fused()
    raw, s_init = _frames(4, 12, 23)
    a = S.StaggeredStreamingEngine(m, s_init, compact=True)
    for f in range(12):
        a.step(raw[f])
    b = S.StaggeredStreamingEngine(m, s_init[:3])
    b.detach([0, 2])
    torch.cuda.synchronize()
    before = b.state.clone()
    w = a.export_slots([3, 0])
    with pytest.raises(RuntimeError, match="slot 1 is attached"):
        b.import_slots([0, 1], w)
    with pytest.raises(ValueError, match="duplicate slot index"):
        b.import_slots([0, 0], w)
    with pytest.raises(ValueError, match="slot index outside"):
        b.import_slots([0, 3], w)
    with pytest.raises(ValueError, match="the window length differs"):
        S.StaggeredStreamingEngine(m, s_init[:3], window=7).import_slots([0, 2], w)
    with pytest.raises(ValueError, match="model shape"):
        S.StaggeredStreamingEngine(_model("72x119"), s_init[:3]).import_slots([0, 2], w)
    with pytest.raises(RuntimeError, match="slot 0 is detached"):
        b.export_slots([0])
    with pytest.raises(RuntimeError, match="StaggeredStreamingEngine"):
        S.StreamingEngine(m, s_init).export_slots([0])
    with pytest.raises(RuntimeError, match="StaggeredStreamingEngine"):
        S.StreamingEngine(m, s_init).import_slots([0], w)
    torch.cuda.synchronize()
    assert torch.equal(b.state, before) and b.attached == [False, True, False]
    b.import_slots([0, 2], w)
    again = b.export_slots([0, 2])
    torch.cuda.synchronize()
    for k in ("block", "s_rest", "c_t", "s_init"):
        assert torch.equal(_bits(w[k]), _bits(again[k])), k
    assert w["per"] == again["per"] and b.attached == [True, True, True]
    blk = b.state.numel() // 3
    assert torch.equal(b.state.view(3, blk)[1], before.view(3, blk)[1]) and bool((b.handover_refused == -1).all())
    m.check_handoffs()


# ---- 3. the whole chain, IK in the loop ------------------------------------------------------------------------------------------------------
class _Chain:
    """ClockSync + PacketResampler(mode="predict") + SensorFrontEnd(fill=True) + compact engine + TerrainTracker(multi_sbp=True)."""

    def __init__(self, m, skel, n):
        self.n = n
        self.clock = sensors.ClockSync(n, "cuda")
        self.rs = sensors.PacketResampler(n, "cuda", mode="predict", depth=4, max_hold=0.1)
        self.front = sensors.SensorFrontEnd(n, "cuda", fill=True)
        self.eng = S.StaggeredStreamingEngine(m, np.zeros((n, 114), f32), compact=True)
        self.eng.detach(list(range(n)))
        self.tt = terrain.TerrainTracker(skel, n, "cuda", multi_sbp=True)
        self.tt.reset(None, np.zeros((n, 114), f32), scales=[1.0] * n)        # (a tracker that has been given scales takes any wearer)
        self.fab_s = torch.zeros((n, 111), device="cuda")
        self.fab_c = torch.zeros((n, 20), device="cuda")
        self.mask = torch.zeros(n, dtype=torch.bool, device="cuda")

    def parts(self, engine=True):
        p = dict(front=self.front, resampler=self.rs, clock=self.clock)
        if engine:
            p.update(engine=self.eng, tracker=self.tt)
        return p

    def frame(self, t, arrivals, tracks):
        """One tick: `arrivals` {slot: (packets, stamps, arrival times)} pushed through the clock, the emitted rows through front end
        and engine, the tracker on fabricated rows (tracks: {slot: (s_rest row, c_t row)} of the golden tracks) and fed back.  Returns
        the per-slot tensors of the frame."""
        for slot, (pk, st, ar) in arrivals.items():
            self.rs.push(pk, [slot] * len(st), st, arrivals=ar, sync=self.clock)
        emitted = self.rs.emit(float(t))
        flags = self.rs.flags.clone()
        self.front.accumulate(emitted)                                        # a slot in a hold takes the reading; the others ignore it
        out = self.eng.step_packets(self.front, emitted)
        self.mask.zero_()
        for slot, (s, c) in tracks.items():
            self.fab_s[slot], self.fab_c[slot], self.mask[slot] = s, c, True
        self.tt.step({"s_rest": self.fab_s, "c_t": self.fab_c, "valid": out["valid"] & self.mask})
        self.tt.feed_back(self.eng)
        snap = {"packet": emitted, "flags": flags, "theta": self.clock.offsets(), "raw": self.eng.raw.clone(),
                "filled": self.front.filled.clone(), "s_rest": out["s_rest"].clone(), "c_t": out["c_t"].clone(),
                "y_last": out["y_last"].clone(), "T": out["T"].clone(), "root": self.tt.root.clone(), "viz_locs": self.tt.viz_locs.clone(),
                "q_hist": self.tt.q_hist.clone(), "fire": self.tt.fire.clone()}
        return snap


def _same_wearer(u, su, c, sc, where, live):
    """Wearer at slot su of snapshot u and slot sc of snapshot c: every per-slot output bit for bit (NaN rows as NaN rows)."""
    keys = ["packet", "flags", "theta"] + (["raw", "filled", "s_rest", "c_t", "y_last", "T", "root", "viz_locs", "q_hist"] if live else [])
    for k in keys:
        a, b = u[k][su], c[k][sc]
        if a.dtype.is_floating_point:
            nan = torch.isnan(a)
            assert torch.equal(nan, torch.isnan(b)), (where, k)
            a, b = a[~nan], b[~nan]
        assert torch.equal(a, b), (where, k)
    if live:
        assert (int(u["fire"][su]) >= 0) == (int(c["fire"][sc]) >= 0), (where, "fire")
        assert int(c["fire"][sc]) in (-1, sc) and int(u["fire"][su]) in (-1, su), (where, "fire holds the slot index")


def test_the_whole_chain_moves_with_the_ik_in_the_loop(fused, skel):
    """Two wearers (scales 0.875 and 1.0625) on an uninterrupted chain U (n = 3, slots 0 and 2) and on a chain A (n = 3) whose wearers
    move to a chain B (n = 4, slots 3 and 1) at frame 30: X is live and streaming, the IK firing on it; Y is in the middle of its
    T-pose hold and moves with the sums, count and phase of that hold, finishes it on B, attaches and streams.  From the hand-over
    on every output of both wearers is bit-identical to U's, the IK fires after it, and Y's finished tables equal the unmoved hold's."""
    m = fused()
    rng = np.random.RandomState(41)
    F, MOVE, Y_LIVE = 75, 30, 42
    sx, sy = 0.875, 1.0625
    tracks = {w: golden_track(GOLDEN, tag, True) for w, tag in (("x", "track2"), ("y", "track2"))}      # (the IK fires on rows 38 .. 57)
    base = {"x": 5, "y": 25}                                             # the track row a wearer's first valid frame is fed
    tracks = {w: (t[0].astype(f32), torch.from_numpy(t[1].astype(f32)).cuda(), torch.from_numpy(t[2].astype(f32)).cuda())
              for w, t in tracks.items()}
    _, tables = so.case(1, 5)
    # a 100 Hz hub per wearer whose clock is 3.2 s / 1.7 s behind the server's; ticks at 60 Hz; one packet of X lost on the way
    period, t0 = 0.01, 100.0
    ticks = t0 + 0.05 + np.arange(F) / 60.0
    hubs = {}
    for w, off in (("x", 3.2), ("y", 1.7)):
        K = int((ticks[-1] - t0) / period) + 2
        stamps = t0 - off + period * np.arange(K)
        arrive = stamps + off + 0.002 + 0.001 * rng.rand(K)
        pk = np.concatenate([so.frame_packets(rng, 1) for _ in range(K)]).astype(f32)
        if w == "y":                                                     # a steady pose for the holds (scatter as the demo's)
            pk = so.hold_packets(rng, K, 1, 0.01).reshape(K, 42).astype(f32)
        hubs[w] = (pk, stamps, arrive)
    hubs["x"][0][700 // 10 + 3, 7:14] = np.nan                            # one sensor's reading missing: the fill ring answers

    U, A, B = _Chain(m, skel, 3), _Chain(m, skel, 3), _Chain(m, skel, 4)
    where = {"U": {"x": 0, "y": 2}, "C": {"x": 0, "y": 2}}               # C: the chain the moved wearers are on (A, then B)
    C = A
    for ch in (U, A):
        ch.front.load([0], tables)
        ch.eng.attach([0], tracks["x"][0][None])
        ch.tt.reset([0], tracks["x"][0][None], scales=[sx])
        ch.front.begin_heading([2])
    at = {"x": 0, "y": 0}
    age = {"x": 0, "y": None}
    fired_after, k_hold = 0, 0
    for f in range(F):
        t = ticks[f]
        arr = {}
        for w, (pk, st, ar) in hubs.items():
            new = int(np.searchsorted(ar, t, side="right"))
            arr[w] = (pk[at[w]:new], st[at[w]:new], ar[at[w]:new])
            at[w] = new
        if f == 12:                                                      # Y: heading hold done, T-pose hold begins
            for ch in (U, C):
                ch.front.finish([where["U" if ch is U else "C"]["y"]])
                ch.front.begin_tpose([where["U" if ch is U else "C"]["y"]])
        if f == MOVE:                                                    # X live and streaming, Y mid T-pose hold: both move to B
            wx = handover.export_wearers([0], **A.parts())
            wy = handover.export_wearers([2], **A.parts(engine=False))
            A.eng.detach([0])
            handover.import_wearers(wx, [3], **B.parts())
            handover.import_wearers(wy, [1], **B.parts(engine=False))
            assert B.front.mirror.phase[1] == sensors.TPOSE and B.front.mirror.phase[3] == sensors.LIVE and B.eng.attached[3]
            C, where["C"] = B, {"x": 3, "y": 1}
        if f == Y_LIVE:                                                  # Y: T-pose hold done on both; it attaches and streams
            tabs = []
            for ch, key in ((U, "U"), (C, "C")):
                sl = where[key]["y"]
                ch.front.finish([sl])
                tabs.append(ch.front.tables([sl]))
                ch.eng.attach([sl], tracks["y"][0][None])
                ch.tt.reset([sl], tracks["y"][0][None], scales=[sy])
            assert torch.equal(tabs[0], tabs[1]) and bool(torch.isfinite(tabs[0]).all())      # the moved hold's tables == the unmoved one's
            age["y"] = 0
        snaps = []
        for ch, key in ((U, "U"), (C, "C")):
            rows = {}
            for w in ("x", "y"):
                if age[w] is not None and age[w] >= 5:
                    k = age[w] - 5
                    rows[where[key][w]] = (tracks[w][1][base[w] + k], tracks[w][2][base[w] + k])
            snaps.append(ch.frame(t, {where[key][w]: arr[w] for w in arr}, rows))
        torch.cuda.synchronize()
        for w in ("x", "y"):
            _same_wearer(snaps[0], where["U"][w], snaps[1], where["C"][w], (f, w), live=age[w] is not None)
            if f >= MOVE and age[w] is not None:
                fired_after += int(snaps[1]["fire"][where["C"][w]]) >= 0
            if age[w] is not None:
                age[w] += 1
    assert fired_after >= 3, fired_after                                 # the IK fired on moved wearers after the hand-over
    # the maps and every other byte of the terrain blocks; the calibration blocks
    for w in ("x", "y"):
        assert np.array_equal(U.tt.state_bytes()[where["U"][w]], B.tt.state_bytes()[where["C"][w]]), w
        blk = U.front.cal.numel() // U.n
        assert torch.equal(U.front.cal.view(U.n, blk)[where["U"][w]], B.front.cal.view(B.n, blk)[where["C"][w]]), w
    m.check_handoffs()
