"""Gap filling on the MI355X (csrc/tip_fill.hip, tip_amd.sensors): the reference's fixture and edge lengths through real_imu_frames, the
live rule through SensorFrontEnd(fill=True), recorded frames and packet sessions, the streaming engines, the untouched fill=False path
and the hand-over to combine_motions — against tests/sensor_fill_oracle.py, bit for bit (NaNs equal NaNs, signed zeros aside)."""
import os

import numpy as np
import pytest
import torch

import sensor_fill_oracle as fo
import sensor_oracle as so
import tip_amd
from tip_amd import sensors, synth
from test_staggered_streams_gpu import paper  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Lock, Staggered = tip_amd.streaming.StreamingEngine, tip_amd.streaming.StaggeredStreamingEngine
f32 = np.float32


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _equal(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "tip_fill_golden.npz"))


# ---- 1. the reference's fixture ------------------------------------------------------------------------------------------------------
def test_fixture_through_real_imu_frames(golden):
    """All three recordings in one call and each alone.  ROT_DIP: the golden bit for bit (a permutation: no rounding in the rotation).
    ROT_TC: within 8 * 2^-53 * max(1, M), M the largest finite input magnitude — the three-term dot's bound under either contraction."""
    n = len(golden["lengths"])
    oris, accs = [golden[f"ori_{i}"] for i in range(n)], [golden[f"acc_{i}"] for i in range(n)]
    M = max(float(np.nanmax(np.abs(a))) for a in oris + accs)
    bound = 8 * 2.0 ** -53 * max(1.0, M)
    for name, rot in (("dip", sensors.ROT_DIP), ("tc", sensors.ROT_TC)):
        both = sensors.real_imu_frames(oris, accs, rot)
        alone = [sensors.real_imu_frames([oris[i]], [accs[i]], rot, sel=sensors.SEL_DIP17, strict=True)[0] for i in range(n)]
        for i in range(n):
            ref = golden[f"out_{name}_{i}"]
            assert both[i].is_cuda and both[i].dtype == torch.float64 and tuple(both[i].shape) == ref.shape
            assert torch.equal(both[i], alone[i]), (name, i)
            err = float(np.abs(_np(both[i]) - ref).max())
            print(f"{name} L = {ref.shape[0]}: max |device - reference| = {err:.3e} (bound {bound:.3e})")
            if name == "dip":
                assert np.array_equal(_np(both[i]), ref), (i, err)
            else:
                assert err <= bound, (i, err, bound)


# ---- 2. edges ------------------------------------------------------------------------------------------------------------------------
EDGE_L = (1, 2, 7, 10, 11, 12, 63, 64, 65, 129)


@pytest.mark.parametrize("S,sel", [(17, sensors.SEL_DIP17), (6, sensors.SEL_TC6)])
def test_edge_lengths_in_one_call(S, sel):
    """66 sequences of every length around the rule's rows (10, 11) and the kernel's tile (64) in one launch: sequence 0 has no NaN;
    sequence 15 (L = 12) has a selected sensor that reads nothing in rows 0 .. 9, which stays NaN, is counted and refused."""
    rng = np.random.RandomState(100 + S)
    seqs = []
    for r in range(66):
        L = EDGE_L[r % len(EDGE_L)]
        whole = [(sel[1], 20, 31)] if L >= 63 else []
        ori, acc = fo.recording(rng, L, S, p_bad=0.0 if r == 0 else 0.15, whole=whole)
        for s in sel:                                            # a reading in rows 0 .. 9 for every selected sensor
            ori[0, s], acc[min(1, L - 1), s] = rng.normal(size=(3, 3)), rng.normal(size=3)
        seqs.append((ori, acc))
    BAD = 15
    assert seqs[BAD][0].shape[0] == 12
    seqs[BAD][0][:10, sel[2]] = np.nan
    want = [fo.real_frames(o, a, sensors.ROT_DIP, sel) for o, a in seqs]
    unf = [u for _, u in want]
    assert unf[BAD] > 0 and sum(u > 0 for u in unf) == 1 and not np.isnan(seqs[0][0]).any()
    oris, accs = [o for o, _ in seqs], [a for _, a in seqs]
    with pytest.raises(ValueError, match=rf"real_imu_frames: sequences {BAD} \({unf[BAD]} parts\) keep NaN"):
        sensors.real_imu_frames(oris, accs, sensors.ROT_DIP, sel=sel, strict=True)
    got = sensors.real_imu_frames(oris, accs, sensors.ROT_DIP, sel=sel, strict=False)
    assert len(got) == 66
    for r, (ref, _) in enumerate(want):
        assert tuple(got[r].shape) == ref.shape and _equal(got[r], ref), (r, ref.shape)
    assert np.isnan(_np(got[BAD])).any() and np.isfinite(_np(got[0])).all()
    # the same without the refused one: strict passes, and the kernel's own count is the oracle's
    ok = [r for r in range(66) if r != BAD]
    again = sensors.real_imu_frames([oris[r] for r in ok], [accs[r] for r in ok], sensors.ROT_DIP, sel=sel)
    assert all(torch.equal(again[j], got[r]) for j, r in enumerate(ok))


# ---- 3. the live front end -----------------------------------------------------------------------------------------------------------
def _live_case(n, frames, seed):
    """tables [n, 126] and packets [frames, n, 42] with gaps: slot 0 has none; every other slot loses whole sensors (a NaN quaternion)
    and accelerations (a NaN component) with its own probability; slot 1's sensor 0 reads nothing in frames 0 .. 2."""
    rng = np.random.RandomState(seed)
    tables = so.case(n, seed)[1]
    pk = np.stack([so.frame_packets(rng, n) for _ in range(frames)]).reshape(frames, n, 6, 7)
    for i in range(1, n):
        p = 0.05 + 0.25 * rng.rand()
        kind = rng.choice(3, size=(frames, 6), p=[1 - p, p / 2, p / 2])
        pk[:, i][kind == 1, 0] = np.nan
        pk[:, i][kind == 2, 4 + (i % 3)] = np.nan
        if i % 7 == 3:
            pk[20:33, i, 2, :4] = np.nan                         # a run of 13 frames
    if n > 1:
        pk[:3, 1, 0, :4] = np.nan
    return tables, pk.reshape(frames, n, 42)


def _loaded(n, tables, **kw):
    fr = sensors.SensorFrontEnd(n, "cuda", **kw)
    fr.load(range(n), tables)
    return fr


@pytest.mark.parametrize("n", [1, 3, 65])
def test_live_fill_is_rule_v_on_the_transformed_frames(n):
    FR = 60
    tables, pk = _live_case(n, FR, 40 + n)
    off, on = _loaded(n, tables), _loaded(n, tables, fill=True)
    assert off.fill_state is None and off.filled is None and tuple(on.filled.shape) == (n, 12) and on.filled.dtype == torch.uint8
    oracle = [fo.LiveFill() for _ in range(n)]
    n_filled = n_left = 0
    for t in range(FR):
        plain = _np(off.transform(pk[t]))
        got = on.transform(torch.tensor(pk[t]).cuda() if t % 2 else pk[t])
        want = [oracle[i].step(plain[i]) for i in range(n)]
        rows, flags = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
        assert _equal(got, rows), t
        assert np.array_equal(_np(on.filled), flags), t
        n_filled, n_left = n_filled + int((flags == 1).sum()), n_left + int((flags == 2).sum())
        if t == 0 and n > 1:                                     # a bad part before any good one stays NaN
            assert (flags[1, [0, 6]] == 2).all() and np.isnan(rows[1, :9]).all() and np.isnan(rows[1, 54:57]).all()
    have, run, total = (_np(c) for c in on.fill_counts())
    assert have.shape == (n, 12) and have.dtype == np.int32
    assert np.array_equal(have, np.stack([o.have for o in oracle]))
    assert np.array_equal(run, np.stack([o.run for o in oracle]))
    assert np.array_equal(total, np.stack([o.total for o in oracle]))
    print(f"n = {n}: {n_filled} parts filled, {n_left} left NaN")
    assert (total[0] == 0).all() and (n == 1 or (n_filled > 20 and n_left >= 2))
    h1 = on.fill_counts([n - 1])[0]
    assert tuple(h1.shape) == (1, 12) and h1.is_cuda


def test_live_max_gap_unlive_slots_and_resets():
    n, FR = 3, 24
    rng = np.random.RandomState(5)
    tables = so.case(n, 5)[1]
    pk = np.stack([so.frame_packets(rng, n) for _ in range(FR)]).reshape(FR, n, 6, 7)
    pk[10:17, 0, 3, :4] = np.nan                                 # slot 0, sensor 3: seven frames without a reading
    pk = pk.reshape(FR, n, 42)
    off = _loaded(n, tables)
    fr = sensors.SensorFrontEnd(n, "cuda", fill=True, max_gap=3)
    fr.load([0, 1], tables[:2])                                  # slot 2 stays uncalibrated
    oracle = [fo.LiveFill(max_gap=3) for _ in range(2)]
    for t in range(FR):
        plain = _np(off.transform(pk[t]))
        got = _np(fr.transform(pk[t]))
        for i in range(2):
            row, flags = oracle[i].step(plain[i])
            assert _equal(got[i], row) and np.array_equal(_np(fr.filled[i]), flags), (t, i)
        assert np.isnan(got[2]).all() and (_np(fr.filled[2]) == 0).all()          # not live: its NaN row, no flag
        want = 1 if 10 <= t < 13 else (2 if 13 <= t < 17 else 0)                   # the fourth frame goes through as NaN
        assert int(fr.filled[0, 3]) == want and int(fr.filled[0, 9]) == want, t
        assert bool(np.isnan(got[0, 27:36]).all()) == (want == 2) and bool(np.isfinite(got[0, 27:36]).all()) == (want != 2)
    have, run, total = (_np(c) for c in fr.fill_counts())
    assert (have[2] == 0).all() and (total[2] == 0).all() and (have[:2] == 5).all() and total[0, 3] == 3 and total[0, 9] == 3
    # load empties the listed slots' rings: the next bad part has nothing to be filled from
    fr.load([1, 2], tables[1:3])
    have, _, total = (_np(c) for c in fr.fill_counts())
    assert (have[0] == 5).all() and (have[1:] == 0).all() and (total[1:] == 0).all() and total[0, 3] == 3
    p = pk[0].reshape(n, 6, 7).copy()
    p[:, 1, :4] = np.nan
    got = _np(fr.transform(p.reshape(n, 42)))
    assert np.isfinite(got[0, 9:18]).all() and np.isnan(got[1, 9:18]).all() and np.isnan(got[2, 9:18]).all()
    assert [int(fr.filled[i, 1]) for i in range(3)] == [1, 2, 2]
    # begin_heading (a new wearer) and fill_reset do the same
    fr.fill_reset([0])
    assert (_np(fr.fill_counts([0])[0]) == 0).all()
    fr.transform(pk[1])
    fr.begin_heading([1])
    assert (_np(fr.fill_counts([1])[0]) == 0).all() and (_np(fr.fill_counts([0])[0]) == 1).all()
    with pytest.raises(RuntimeError, match="fill_counts: this front end was built without fill=True"):
        off.fill_counts()
    with pytest.raises(ValueError, match="max_gap"):
        sensors.SensorFrontEnd(2, "cuda", max_gap=3)
    with pytest.raises(ValueError, match="max_gap"):
        sensors.SensorFrontEnd(2, "cuda", fill=True, max_gap=-1)


# ---- 4. recorded frames and recorded packet sessions ---------------------------------------------------------------------------------
@pytest.mark.parametrize("max_gap", [None, 2])
def test_recorded_sessions_equal_the_live_front_end(max_gap):
    lens = (65, 12, 1)
    rng = np.random.RandomState(9)
    tables = so.case(3, 9)[1]
    sessions = []
    for r, L in enumerate(lens):
        pk = np.stack([so.frame_packets(rng, 1)[0] for _ in range(L)]).reshape(L, 6, 7)
        kind = rng.choice(3, size=(L, 6), p=[0.8, 0.1, 0.1])
        pk[kind == 1, 1] = np.nan
        pk[kind == 2, 5] = np.nan
        if L > 30:
            pk[20:29, 4, :4] = np.nan
        sessions.append(pk.reshape(L, 42))
    live, live_flags, plain = [], [], []
    for r, L in enumerate(lens):
        on, off = _loaded(1, tables[r:r + 1], fill=True, max_gap=max_gap), _loaded(1, tables[r:r + 1])
        rows, flags, raw = [], [], []
        for t in range(L):
            rows.append(on.transform(sessions[r][t:t + 1]).clone())
            flags.append(on.filled.clone())
            raw.append(off.transform(sessions[r][t:t + 1]).clone())
        live.append(torch.cat(rows)), live_flags.append(torch.cat(flags)), plain.append(torch.cat(raw))
    assert any(bool((f == 1).any()) for f in live_flags) and any(bool((f == 2).any()) for f in live_flags)
    recs = sensors.transform_sequences(sessions, tables)
    filled, flags = sensors.transform_sequences(sessions, tables, fill=True, max_gap=max_gap, return_flags=True)
    again, flags2 = sensors.fill_sequences(plain, rule="live", max_gap=max_gap, return_flags=True)
    host = sensors.fill_sequences([_np(p) for p in plain], max_gap=max_gap, host=True)
    for r, L in enumerate(lens):
        assert recs[r].is_cuda and recs[r].dtype == torch.float32 and tuple(recs[r].shape) == (L, 72)
        assert _equal(recs[r], plain[r]), r
        assert _equal(filled[r], live[r]) and torch.equal(flags[r], live_flags[r]), r
        assert _equal(again[r], live[r]) and torch.equal(flags2[r], live_flags[r]), r
        assert isinstance(host[r], np.ndarray) and host[r].dtype == f32 and _equal(host[r], live[r])
        assert _equal(plain[r], sensors.transform_sequences([sessions[r]], tables[r:r + 1])[0])
    with pytest.raises(ValueError, match='rule is "live"'):
        sensors.fill_sequences(plain, rule="reference")
    with pytest.raises(ValueError, match=r"tables is \[3, 126\]"):
        sensors.transform_sequences(sessions, tables[:2])


# ---- 5. engines ----------------------------------------------------------------------------------------------------------------------
FRAMES, DROP = 95, 50


@pytest.fixture(scope="module")
def streams():
    rng = np.random.RandomState(21)
    n = 3
    pk = so.hold_packets(rng, FRAMES, n, 0.05, acc_sigma=3.0)
    s0 = np.stack([synth.make_recording(2, seed=300 + i)[1] for i in range(n)])
    tables = so.calibrate_v(so.hold_packets(rng, 3, n, 0.02), so.hold_packets(rng, 3, n, 0.02)).astype(f32)
    dropped = pk.copy()
    dropped[DROP, 1] = np.nan                                    # stream 1 delivers nothing for one frame
    return pk, dropped, s0, tables


def _y(out):
    return None if out is None else out["y_last"].clone()


@pytest.mark.parametrize("use_graph", [False, True])
def test_a_dropped_packet_with_and_without_fill(paper, streams, use_graph):
    """Lock-step, n = 3, one packet of stream 1 dropped at frame 50.  With a fill=True front end step_packets equals step() on the filled
    frames bit for bit and stream 1's y_last is finite at every later frame; without, it is NaN while the window holds the frame (the
    behaviour as it was, asserted as the contrast); the streams without a gap are bit-identical between the two."""
    m, _ = paper
    _, pk, s0, tables = streams
    on, twin_front, off = _loaded(3, tables, fill=True), _loaded(3, tables, fill=True), _loaded(3, tables)
    a, b, c = (Lock(m, s0, use_graph=use_graph) for _ in range(3))
    window = a.window
    assert window == 40 and DROP + window < FRAMES
    for f in range(FRAMES):
        ya = _y(a.step_packets(on, pk[f]))
        yb = _y(b.step(twin_front.transform(pk[f])))
        yc = _y(c.step_packets(off, pk[f]))
        assert (ya is None) == (yb is None) == (yc is None), f
        if f == DROP:
            assert (_np(on.filled)[1] == 1).all() and (_np(on.filled)[[0, 2]] == 0).all() and torch.isfinite(a.raw).all()
            assert torch.isnan(c.raw[1]).all()
        if ya is None:
            continue
        assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), f
        assert torch.equal(ya[[0, 2]].view(torch.int32), yc[[0, 2]].view(torch.int32)), f
        if f >= 5:
            assert torch.isfinite(ya).all(), f
        if DROP <= f < DROP + window:
            assert torch.isnan(yc[1]).any(), f
        elif f < DROP:
            assert torch.equal(ya.view(torch.int32), yc.view(torch.int32)), f
    assert a.captures == b.captures == c.captures == (1 if use_graph else 0)
    torch.cuda.synchronize()


def test_a_newcomer_does_not_inherit_the_ring(paper, streams):
    """Staggered: slot 1 is detached, another wearer's calibration is loaded into it and it is attached again; the newcomer's first
    packet is bad and stays NaN (flag 2), whatever the slot's rings held before."""
    m, _ = paper
    pk, _, s0, tables = streams
    fr = _loaded(2, tables[:2], fill=True)
    eng = Staggered(m, s0[:2])
    for f in range(8):
        eng.step_packets(fr, pk[f, :2])
    assert (_np(fr.fill_counts()[0]) == 5).all()
    eng.detach([1])
    fr.load([1], tables[2:3])
    eng.attach([1], s0[2:3])
    p = pk[8, :2].copy()
    p[:] = np.nan
    eng.step_packets(fr, p)
    flags = _np(fr.filled)
    assert (flags[0] == 1).all() and (flags[1] == 2).all()
    assert torch.isfinite(eng.raw[0]).all() and torch.isnan(eng.raw[1]).all()
    have, _, total = (_np(c) for c in fr.fill_counts())
    assert (have[1] == 0).all() and (total[1] == 0).all() and (total[0] == 1).all()
    torch.cuda.synchronize()


# ---- 6. fill=False is the front end as it was ----------------------------------------------------------------------------------------
class _Counting:
    """The library with every tip_* call noted by name."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tip_") or name == "tip_strerror":
            return fn

        def call(*a):
            self._log.append(name)
            return fn(*a)
        return call


def test_fill_false_launches_and_computes_what_it_did():
    n = 5
    pk, tables = so.case(n, 77)
    pk[2, :4] = np.nan
    logs, outs = [], []
    for kw in ({}, {"fill": False}, {"fill": True}):
        log = []
        fr = sensors.SensorFrontEnd(n, "cuda", **kw)
        fr.lib = _Counting(fr.lib, log)
        fr.load(range(n), tables)
        del log[:]
        outs.append(fr.transform(pk).clone())
        logs.append(list(log))
        if not kw.get("fill"):
            assert fr.fill_state is None and fr.filled is None and fr.max_gap == -1
    assert logs[0] == logs[1] == ["tip_sensor_transform"] and logs[2] == ["tip_sensor_transform", "tip_fill_live"]
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert torch.isnan(outs[0][2, :9]).all() and torch.isnan(outs[2][2, :9]).all()          # (nothing to fill from yet)
    assert torch.isfinite(outs[0][[0, 1, 3, 4]]).all() and _equal(outs[0], outs[2])


# ---- 7. into the combiner -------------------------------------------------------------------------------------------------------------
def test_real_imu_frames_feed_combine_motions(golden):
    from make_data_golden import synth_motion
    files_dev, files_host = [], []
    oris, accs = [golden["ori_2"]], [golden["acc_2"]]
    rng = np.random.RandomState(3)
    for L in (65, 90):
        o, a = fo.recording(rng, L, 17, p_bad=0.1)
        for s in sensors.SEL_DIP17:
            o[0, s], a[0, s] = rng.normal(size=(3, 3)), rng.normal(size=3)
        oris.append(o), accs.append(a)
    imus = sensors.real_imu_frames(oris, accs, sensors.ROT_DIP)
    for i, (o, a) in enumerate(zip(oris, accs)):
        L = o.shape[0]
        _, s, c = synth_motion(L, 50 + i)
        ref, unfilled = fo.real_frames(o, a, sensors.ROT_DIP, sensors.SEL_DIP17)
        assert unfilled == 0
        files_dev.append({"imu": imus[i], "nimble_qdq": s, "constrs": c})
        files_host.append({"imu": ref, "nimble_qdq": s, "constrs": c})
    bias = np.linspace(-0.1, 0.1, 18 * 3).reshape(3, 18)
    x = tip_amd.data.combine_motions(files_dev, [2, 2, 2], biases=bias)
    y = tip_amd.data.combine_motions(files_host, [2, 2, 2], biases=bias)
    assert x.IMU.shape[0] > 100 and np.array_equal(x.info, y.info)
    for k in ("IMU", "SUM", "S"):
        assert _equal(getattr(x, k), getattr(y, k)), k
