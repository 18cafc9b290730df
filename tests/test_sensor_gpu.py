"""GPU tests of the sensor front end (csrc/tip_sensor.hip; tip_amd.sensors; the engines' step_packets) against the fp64 numpy / scipy
oracle of the reference's live demo (tests/sensor_oracle.py): the per-frame transform at the block edges of its thread mapping,
isolation of bad readings, the two calibration holds beside slots that must not be touched, saved tables, and step_packets against
step(front.transform(p)) bit for bit through every engine."""
import ctypes

import numpy as np
import pytest
import torch

import sensor_oracle as so
import tip_amd
from tip_amd import lib as tlib
from tip_amd import sensors, synth
from test_staggered_streams_gpu import paper  # noqa: F401

pytestmark = pytest.mark.gpu
Lock, Staggered = tip_amd.streaming.StreamingEngine, tip_amd.streaming.StaggeredStreamingEngine
f32 = np.float32


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def _front(n, **kw):
    return sensors.SensorFrontEnd(n, "cuda", **kw)


def _loaded(n, tables):
    fr = _front(n)
    fr.load(range(n), tables)
    return fr


def _noise(pk, tables):
    """(fp64 oracle, fp32 noise of the rotation columns, of the acceleration columns) on the device's inputs."""
    ref = so.frames_from_tables(pk, tables)
    d = np.abs(so.frames_from_tables(pk, tables, dtype=f32).astype(np.float64) - ref)
    return ref, float(d[:, :54].max()), float(d[:, 54:].max())


@pytest.fixture(scope="module")
def case1_bound():
    """The bound of case 1 on rotation columns at its largest size (CPU only): 3 x the fp32 restatement's own error."""
    return 3.0 * _noise(*so.case(1024, 1024))[1]


# ---- 1. the transform against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 42, 43, 128, 1024])
def test_transform_matches_the_oracle(n):
    """One thread per (slot, sensor), 256 threads per block: 42 slots are 252 threads, 43 straddle the first block edge, 128 fill three
    blocks exactly.  The device may differ from the fp64 oracle by at most 3 x the error of the same restatement in numpy float32 on
    the same inputs (the margin the conditioning tests give the forward), rotation and acceleration columns separately."""
    pk, tables = so.case(n, n)
    ref, noise_r, noise_a = _noise(pk, tables)
    guard = torch.full((n + 2, 72), 7.0, device="cuda")
    out = _loaded(n, tables).transform(pk, out=guard[1:-1])
    got = out.cpu().numpy().astype(np.float64)
    err_r, err_a = float(np.abs(got - ref)[:, :54].max()), float(np.abs(got - ref)[:, 54:].max())
    print(f"n={n}: fp32 noise rot {noise_r:.3e} acc {noise_a:.3e}; device error rot {err_r:.3e} acc {err_a:.3e}")
    assert np.isfinite(got).all()
    assert err_r <= 3.0 * noise_r and err_a <= 3.0 * noise_a
    assert (got[:, 54:] == 10.0).any() == (ref[:, 54:] == 10.0).any() and np.abs(got[:, 54:]).max() <= 10.0
    assert (guard[0] == 7.0).all() and (guard[-1] == 7.0).all()


# ---- 2. isolation -----------------------------------------------------------------------------------------------------------------
def test_bad_readings_stay_in_their_sensor():
    """n = 43.  A NaN acceleration component, an Inf acceleration component, a zero quaternion and a NaN quaternion, one sensor of
    four different slots.  A quaternion without a rotation gives exactly that sensor's 12 columns NaN.  A bad acceleration is stated
    from the oracle, which has no rule of its own for it: the NaN one makes the sensor's three acceleration columns NaN (never +-10),
    the Inf one (that slot's offset set to 0) NaN or a clipped +-10 exactly where np.clip gives them; the rotation columns of both
    sensors are the clean run's.  Every output outside the four sensors is bit-identical to the clean run."""
    n = 43
    pk, tables = so.case(n, 43)
    tables = tables.copy()
    tables[11, 54:72] = 0.0
    fr = _loaded(n, tables)
    clean = fr.transform(pk).cpu().numpy()
    assert np.isfinite(clean).all()
    bad = pk.copy().reshape(n, 6, 7)
    bad[5, 2, 5] = np.nan           # slot 5 sensor 2: a_y
    bad[11, 0, 4] = np.inf          # slot 11 sensor 0: a_x
    bad[20, 4, :4] = 0.0            # slot 20 sensor 4: the zero quaternion
    bad[30, 5, 1] = np.nan          # slot 30 sensor 5: a NaN quaternion component
    got = fr.transform(bad.reshape(n, 42)).cpu().numpy()
    where = [(5, 2), (11, 0), (20, 4), (30, 5)]

    def cols(k):
        return list(range(9 * k, 9 * k + 9)) + list(range(54 + 3 * k, 54 + 3 * k + 3))

    touched = np.zeros((n, 72), dtype=bool)
    for s, k in where:
        touched[s, cols(k)] = True
    assert np.array_equal(_bits(got)[~touched], _bits(clean)[~touched])
    for s, k in ((20, 4), (30, 5)):
        assert np.isnan(got[s, cols(k)]).all()
    # the oracle on the bad accelerations (the two bad quaternions, which scipy refuses or turns into NaN matrices, left clean)
    ok_q = bad.copy()
    ok_q[20, 4, :4], ok_q[30, 5, :4] = pk.reshape(n, 6, 7)[20, 4, :4], pk.reshape(n, 6, 7)[30, 5, :4]
    with np.errstate(invalid="ignore"):
        ref = so.frames_from_tables(ok_q.reshape(n, 42), tables)
    for s, k in ((5, 2), (11, 0)):
        assert np.array_equal(_bits(got[s, 9 * k: 9 * k + 9]), _bits(clean[s, 9 * k: 9 * k + 9]))
        a_got, a_ref = got[s, 54 + 3 * k: 57 + 3 * k], ref[s, 54 + 3 * k: 57 + 3 * k]
        assert np.array_equal(np.isnan(a_got), np.isnan(a_ref)), (s, a_got, a_ref)
        assert np.array_equal(a_got[~np.isnan(a_got)], a_ref[~np.isnan(a_ref)].astype(f32)), (s, a_got, a_ref)
    assert np.isnan(got[5, 54 + 6: 54 + 9]).all()
    a_inf = ref[11, 54:57]
    assert (np.isnan(a_inf) | (np.abs(a_inf) == 10.0)).all() and (np.abs(a_inf) == 10.0).any()


def test_unfinished_calibrations_give_nan_rows():
    """Phases 0 (uncalibrated), 1 and 3 (in a hold), 2 (heading done): 72 NaN, never a finite row; the live slot beside them is served."""
    rng = np.random.RandomState(7)
    pk, tables = so.case(5, 70)
    hold = so.hold_packets(rng, 2, 5, 0.02)
    fr = _front(5)
    fr.load([4], tables[4:5])
    fr.begin_heading([1, 2, 3])
    fr.accumulate(hold[0])
    fr.finish([2, 3])
    fr.begin_tpose([3])
    fr.accumulate(hold[1])
    assert fr.mirror.phase == [0, 1, 2, 3, 4] and list(fr.live()) == [False] * 4 + [True]
    got = fr.transform(pk).cpu().numpy()
    assert np.isnan(got[:4]).all() and np.isfinite(got[4]).all()
    assert np.array_equal(_bits(got[4]), _bits(_loaded(5, tables).transform(pk)[4]))


# ---- 3. calibration ---------------------------------------------------------------------------------------------------------------
def _within_one_ulp(got, ref64):
    ref = ref64.astype(f32)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64)


@pytest.mark.parametrize("K", [1, 2, 181])
def test_holds_beside_slots_that_are_not_touched(K, case1_bound):
    """Four slots in four situations at once — 0 accumulating its heading, 1 accumulating its T-pose (after a heading of 3 readings), 2
    live, 3 uncalibrated — through K accumulate calls of random packets.  After finish every table entry is within one fp32 ulp of the
    fp64 oracle's entry rounded to fp32 (the device sums, divides and multiplies in fp64: a double rounding costs at most that), and
    the blocks of slots 2 and 3 have not changed by a bit.  At K = 181 the readings scatter 0.5 rad, so the mean matrices are visibly
    not orthonormal: the device matches the oracle that keeps them as they are and misses, by more than the bound of case 1, the
    variant that re-orthonormalises them."""
    rng = np.random.RandomState(100 + K)
    scatter = 0.5 if K == 181 else 0.02
    n = 4
    first = so.hold_packets(rng, 3, n, 0.02)                   # slot 1's heading
    hold = so.hold_packets(rng, K, n, scatter)
    _, tables = so.case(n, 5)
    fr = _front(n)
    fr.load([2], tables[2:3])
    fr.begin_heading([1])
    for p in first:
        fr.accumulate(p)
    fr.finish([1])
    fr.begin_tpose([1])
    fr.begin_heading([0])
    block = fr.cal.numel() // n
    before = fr.cal.clone()
    for p in hold:
        fr.accumulate(torch.tensor(p) if K == 2 else p)        # (host tensors and arrays alike)
    mid = fr.cal.clone()
    assert torch.equal(mid[2 * block:], before[2 * block:])
    assert not torch.equal(mid[:block], before[:block]) and not torch.equal(mid[block: 2 * block], before[block: 2 * block])
    fr.finish([0, 1])
    assert fr.mirror.phase == [2, 4, 4, 0]
    got = fr.tables().cpu().numpy()
    assert torch.equal(fr.cal[2 * block:], before[2 * block:])
    # slot 0: the heading of `hold`
    G0, off0 = so.heading_v(so.read_packet_v(hold[:, 0]).mean(axis=0))
    assert _within_one_ulp(got[0, :54], G0.reshape(54)).all() and _within_one_ulp(got[0, 54:72], off0.reshape(18)).all()
    # slot 1: the heading of `first`, the T-pose of `hold`
    G1, off1 = so.heading_v(so.read_packet_v(first[:, 1]).mean(axis=0))
    B1 = so.tpose_v(so.read_packet_v(hold[:, 1]).mean(axis=0), G1)
    assert _within_one_ulp(got[1], so.pack_tables(G1, off1, B1)).all()
    assert np.array_equal(_bits(got[2]), _bits(tables[2]))
    if K == 181:
        dev = np.abs(G0 @ G0.transpose(0, 2, 1) - np.eye(3)).max()
        miss = float(np.abs(got[0, :54].astype(np.float64) - so.reorthonormalised(G0).reshape(54)).max())
        print(f"K=181, 0.5 rad: |G G^T - 1| = {dev:.3e}; device - re-orthonormalised = {miss:.3e}; bound of case 1 = {case1_bound:.3e}")
        assert miss > case1_bound
    # a custom R_Gp_B0 goes through the same finish
    R = so.Q2R(rng.normal(size=(6, 4)))
    fr2 = _front(1, r_gp_b0=R)
    for which, pk in ((fr2.begin_heading, first), (fr2.begin_tpose, hold[:3])):
        which()
        for p in pk:
            fr2.accumulate(p[1:2])
        fr2.finish()
    B2 = so.tpose_v(so.read_packet_v(hold[:3, 1]).mean(axis=0), G1, R)
    assert _within_one_ulp(fr2.tables().cpu().numpy()[0], so.pack_tables(G1, off1, B2)).all()


def test_finish_without_a_reading_gives_nan_tables():
    pk, tables = so.case(2, 9)
    fr = _front(2)
    fr.load([1], tables[1:2])
    fr.begin_heading([0])
    fr.finish([0])
    t = fr.tables([0]).cpu().numpy()[0]
    assert np.isnan(t[:72]).all()
    fr.begin_tpose([0])
    fr.finish([0])
    assert np.isnan(fr.tables([0]).cpu().numpy()).all() and list(fr.live()) == [True, True]
    got = fr.transform(pk).cpu().numpy()
    assert np.isnan(got[0]).all() and np.isfinite(got[1]).all()


def test_front_end_refusals():
    fr = _front(3)
    pk, _ = so.case(3, 1)
    with pytest.raises(RuntimeError, match="begin_tpose: slot 0 has no finished heading"):
        fr.begin_tpose([0])
    with pytest.raises(RuntimeError, match="finish: slot 2 is not accumulating"):
        fr.finish([2])
    for bad in (pk[:2], pk[:, :41], pk.reshape(-1)):
        with pytest.raises(ValueError, match=r"packets is \[3, 42\]"):
            fr.accumulate(bad)
        with pytest.raises(ValueError, match=r"packets is \[3, 42\]"):
            fr.transform(bad)
    with pytest.raises(ValueError, match="slot index outside"):
        fr.begin_heading([3])
    with pytest.raises(ValueError, match="tables is"):
        fr.load([0, 1], np.zeros((1, 126), f32))
    assert fr.mirror.phase == [0, 0, 0]
    torch.cuda.synchronize()


# ---- 4. tables round trip ---------------------------------------------------------------------------------------------------------
def test_tables_round_trip_and_harmless_slot_lists():
    """tables() -> load() on a fresh front end: the same tables and the same frames, bit for bit.  Through the C-ABI, a slot listed
    twice and slots outside [0, n) are harmless: nothing around the calibration buffer or around the listed rows is written."""
    rng = np.random.RandomState(11)
    n = 5
    a = _front(n)
    for begin in (a.begin_heading, a.begin_tpose):
        begin()
        for p in so.hold_packets(rng, 3, n, 0.1):
            a.accumulate(p)
        a.finish()
    saved = a.tables()
    b = _front(n)
    b.load(range(n), saved)
    pk = so.frame_packets(rng, n)
    assert np.array_equal(_bits(b.tables()), _bits(saved)) and np.isfinite(saved.cpu().numpy()).all()
    assert np.array_equal(_bits(b.transform(pk)), _bits(a.transform(pk)))

    lib, st = tlib.load(), torch.cuda.current_stream().cuda_stream
    nb = ctypes.c_size_t()
    assert lib.tip_sensor_state_bytes(n, ctypes.byref(nb)) == 0
    block = nb.value // n
    buf = torch.full(((n + 2) * block,), 0xCD, dtype=torch.uint8, device="cuda")       # one guard block on either side
    cal = buf.data_ptr() + block
    slots = torch.tensor([1, 3, 3, n, -1, 1 << 30, 0], dtype=torch.int32, device="cuda")
    rows = torch.full((9, 126), 5.0, device="cuda")                                    # rows 1 .. 7 are the call's
    rows[1:8] = saved[[1, 3, 3, 0, 0, 0, 0]]
    assert lib.tip_sensor_reset(cal, n, st) == 0
    assert lib.tip_sensor_set(cal, n, slots.data_ptr(), 7, rows[1:].data_ptr(), st) == 0
    out = torch.full((9, 126), 6.0, device="cuda")
    assert lib.tip_sensor_get(cal, n, slots.data_ptr(), 7, out[1:].data_ptr(), st) == 0
    assert (out[0] == 6.0).all() and (out[8] == 6.0).all() and (out[4:7] == 6.0).all()           # skipped: as they were
    assert np.array_equal(_bits(out[[1, 2, 3, 7]]), _bits(saved[[1, 3, 3, 0]]))
    # holds through the same list: slots 2 and 4 (phase 0) are not listed, 0 / 1 / 3 restart their heading
    assert lib.tip_sensor_begin(cal, n, slots.data_ptr(), 7, tlib.TIP_SENSOR_HEADING, st) == 0
    d_pk = torch.tensor(pk).cuda()
    assert lib.tip_sensor_accumulate(cal, d_pk.data_ptr(), n, st) == 0
    assert lib.tip_sensor_finish(cal, n, slots.data_ptr(), 7, None, st) == 0
    assert lib.tip_sensor_begin(cal, n, slots.data_ptr(), 7, tlib.TIP_SENSOR_TPOSE, st) == 0
    assert lib.tip_sensor_accumulate(cal, d_pk.data_ptr(), n, st) == 0
    assert lib.tip_sensor_finish(cal, n, slots.data_ptr(), 7, None, st) == 0
    raw = torch.full((n + 2, 72), 7.0, device="cuda")
    assert lib.tip_sensor_transform(cal, d_pk.data_ptr(), n, 10.0, raw[1:].data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert (buf[:block] == 0xCD).all() and (buf[-block:] == 0xCD).all()
    r = raw.cpu().numpy()
    assert (r[0] == 7.0).all() and (r[-1] == 7.0).all()
    assert np.isfinite(r[[1, 2, 4]]).all() and np.isnan(r[[3, 5]]).all()            # slots 0, 1, 3 live; 2, 4 never calibrated
    # a one-reading calibration against the oracle
    one = so.calibrate_v(pk[None], pk[None]).astype(f32)
    ref = so.frames_from_tables(pk, one)
    assert np.abs(r[[1, 2, 4]] - ref[[0, 1, 3]]).max() < 1e-4


# ---- 5. engines -------------------------------------------------------------------------------------------------------------------
FRAMES = 50


@pytest.fixture(scope="module")
def streams():
    """Four streams of FRAMES packets (a fixed pose per sensor with 0.05 rad of motion), their start states, and a front end whose
    slots 0 and 1 went through the holds (differently) and 2 and 3 are loaded."""
    rng = np.random.RandomState(21)
    n = 4
    pk = so.hold_packets(rng, FRAMES, n, 0.05, acc_sigma=3.0)
    s0 = np.stack([synth.make_recording(2, seed=300 + i)[1] for i in range(n)])
    holds = [so.hold_packets(rng, 3, n, s) for s in (0.02, 0.02, 0.2, 0.2)]
    tables = np.empty((n, 126), f32)
    tables[[0, 2]] = so.calibrate_v(holds[0], holds[1]).astype(f32)[[0, 2]]
    tables[[1, 3]] = so.calibrate_v(holds[2], holds[3]).astype(f32)[[1, 3]]
    return pk, s0, holds, tables


def _front3(streams, n=3):
    """n slots; 0 and 1 calibrated on the device from different holds, 2 put in through load; a fourth slot stays uncalibrated."""
    _, _, holds, tables = streams
    fr = _front(n)
    for slot, (h, t) in ((0, holds[:2]), (1, holds[2:])):
        fr.begin_heading([slot])
        for p in h:
            fr.accumulate(p[:n])
        fr.finish([slot])
        fr.begin_tpose([slot])
        for p in t:
            fr.accumulate(p[:n])
        fr.finish([slot])
    fr.load([2], tables[2:3])
    return fr


KEYS = ("s_rest", "c_t", "y_last")


def _snap(out):
    if out is None:
        return None
    d = {k: out[k].clone() for k in KEYS}
    d["T"] = out["T"].clone() if isinstance(out["T"], torch.Tensor) else out["T"]
    if "valid" in out:
        d["valid"] = out["valid"].clone()
    return d


def _same(a, b, who, rows=None):
    assert (a is None) == (b is None), who
    if a is None:
        return
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, torch.Tensor):
            if rows is not None:
                x, y = x[rows], y[rows]
            x, y = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (x, y))
            assert torch.equal(x, y), (who, k)
        else:
            assert x == y, (who, k)


@pytest.mark.parametrize("kind,kw", [("lock", {}), ("lock", {"use_graph": True}), ("staggered", {}), ("staggered", {"use_graph": True}),
                                     ("staggered", {"compact": True}), ("staggered", {"compact": True, "use_graph": True})])
def test_step_packets_is_step_of_the_transformed_frame(paper, streams, kind, kw):
    """n = 3, the paper's model, 50 frames (graph mode begins at frame 44): step_packets(front, p) against step(front.transform(p)) in a
    twin engine, bit for bit in s_rest, c_t, y_last and T / valid, with equal `captures`."""
    m, _ = paper
    pk, s0, _, _ = streams
    fr = _front3(streams)
    assert list(fr.live()) == [True] * 3
    Engine = Lock if kind == "lock" else Staggered
    a, b = Engine(m, s0[:3], **kw), Engine(m, s0[:3], **kw)
    produced = 0
    for f in range(FRAMES):
        p = pk[f, :3]
        oa = _snap(a.step_packets(fr, torch.tensor(p).cuda() if f % 3 == 0 else p))        # (CUDA tensors and host arrays alike)
        ob = _snap(b.step(fr.transform(torch.tensor(p) if f % 2 else p)))
        _same(oa, ob, (kind, kw, f))
        produced += oa is not None and bool(torch.isfinite(oa["y_last"]).all())
    assert produced == FRAMES - 5 and a.captures == b.captures == (1 if kw.get("use_graph") else 0)
    assert a.frame == b.frame == FRAMES
    torch.cuda.synchronize()


@pytest.mark.parametrize("use_graph", [False, True])
def test_a_newcomer_calibrates_while_the_pool_streams(paper, streams, use_graph):
    """A compact pool of four slots on a pinned plan, slot 3 detached and uncalibrated.  From frame 10 on it runs its two holds beside
    the others' frames (5 + 5 accumulate calls, one between two frames each) and is attached before frame 20.  Its rows equal the
    same stream run alone in a one-slot engine; the other slots' rows equal, bit for bit, a run in which it never shows up."""
    m, _ = paper
    pk, s0, holds, _ = streams
    m.set_plan("fused")
    try:
        def pool(newcomer):
            fr = _front3(streams, 4)
            eng = Staggered(m, s0, compact=True, use_graph=use_graph)
            eng.detach([3])
            outs = []
            for f in range(FRAMES):
                if newcomer:
                    if f == 10:
                        fr.begin_heading([3])
                    if f == 15:
                        fr.finish([3])
                        fr.begin_tpose([3])
                    if 10 <= f < 20:
                        fr.accumulate(holds[0][f % 3] if f < 15 else holds[1][f % 3])
                    if f == 20:
                        fr.finish([3])
                        eng.attach([3], s0[3:4])
                outs.append(_snap(eng.step_packets(fr, pk[f])))
            return fr, eng, outs

        fr, eng, with_new = pool(True)
        _, _, without = pool(False)
        assert list(fr.live()) == [True] * 4 and eng.attached == [True] * 4
        for f in range(FRAMES):
            _same({k: with_new[f][k] for k in KEYS + ("valid",)}, {k: without[f][k] for k in KEYS + ("valid",)}, ("others", f), rows=[0, 1, 2])
            assert bool(with_new[f]["valid"][3]) == (f >= 25)
        alone_front = _front(1)
        alone_front.load([0], fr.tables([3]))
        alone = Staggered(m, s0[3:4], use_graph=use_graph)
        for f in range(20, FRAMES):
            o = _snap(alone.step(alone_front.transform(pk[f, 3:4])))
            for k in KEYS + ("valid",):
                if k == "y_last" and f < 25:          # (priming: a NaN row in both, whose payload is not part of any contract)
                    assert torch.isnan(with_new[f][k][3]).all() and torch.isnan(o[k][0]).all()
                    continue
                x, y = with_new[f][k][3], o[k][0]
                x, y = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (x, y))
                assert torch.equal(x, y), ("newcomer", f, k)
        assert torch.isfinite(with_new[-1]["y_last"]).all()
        torch.cuda.synchronize()
    finally:
        m.set_plan("auto")


def test_step_packets_refusals_launch_nothing(paper, streams):
    m, _ = paper
    pk, s0, _, tables = streams
    fr = _front(4)
    fr.load([0, 1, 2], tables[:3])                     # slot 3 is not calibrated
    for eng in (Lock(m, s0), Staggered(m, s0), Staggered(m, s0, compact=True)):
        eng.raw.fill_(3.0)
        fr.packets.fill_(4.0)
        with pytest.raises(RuntimeError, match="step_packets: slot 3 is not calibrated"):
            eng.step_packets(fr, pk[0])
        with pytest.raises(ValueError, match="step_packets: the front end serves 3 slots"):
            eng.step_packets(_front(3), pk[0, :3])
        with pytest.raises(ValueError, match=r"step_packets: packets is \[4, 42\]"):
            eng.step_packets(_loaded(4, tables), pk[0, :3])
        assert eng.frame == 0 and (eng.raw == 3.0).all() and (fr.packets == 4.0).all() and eng.captures == 0
    # a detached slot may be uncalibrated: the staggered engines serve the others
    for eng in (Staggered(m, s0), Staggered(m, s0, compact=True)):
        eng.detach([3])
        out = eng.step_packets(fr, pk[0])
        assert eng.frame == 1 and not bool(out["valid"].any())
    torch.cuda.synchronize()
