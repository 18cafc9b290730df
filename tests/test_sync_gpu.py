"""GPU tests of clock sync and predicted ticks (csrc/tip_clock.hip; tip_amd.sensors.ClockSync, PacketResampler(mode="predict"),
push(arrivals=, sync=), sync_sequences, resample_sequences(mode="predict")) against their numpy oracle (tests/sync_oracle.py, whose own
properties tests/test_sync_cpu.py holds): the clock rule bit for bit at the edges of the 64-wide scan, the fused push against the two
launches it replaces, recorded sequences against the live rule, every flag of the predict rule, and the whole chain in front of an engine.

No fixture from the reference is needed: the reference keeps no stamps (live_demo_new.py:82-115).

Bounds: every time, offset, counter and flag is EQUAL to the oracle's as a bit pattern (fp64 statements in a stated order, nothing
fused); a held packet is the packet; an interpolated row is the slerp entry's row bit for bit; a predicted row is within 3 x the fp32
noise of the fp64 oracle, noise = max |oracle in fp32 - oracle in fp64| on the same inputs, on the rotation matrices of the output
quaternions and on the accelerations separately — the rule tests/test_resample_gpu.py uses for interpolated rows."""
import ctypes

import numpy as np
import pytest
import torch

import resample_oracle as ro
import sensor_oracle as so
import sync_oracle as sy
import tip_amd
from tip_amd import lib as tlib
from tip_amd import sensors, synth
from test_staggered_streams_gpu import paper  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
NAN = float("nan")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class _Clock:
    """A clock state of n blocks through the C ABI, a guard block of 0xCD on either side."""

    def __init__(self, n):
        self.n, self.lib = n, tlib.load()
        nb = ctypes.c_size_t()
        assert self.lib.tip_clock_state_bytes(n, ctypes.byref(nb)) == 0 and nb.value == 32 * n
        self.buf = torch.full(((n + 2) * 32,), 0xCD, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + 32
        assert self.lib.tip_clock_reset(self.ptr, n, None, 0, _st()) == 0

    def map(self, slots, stamps, arrivals, leak=sy.LEAK, slew=sy.SLEW):
        """-> times_out [m] as the launch left it over a fill of 7.0."""
        m = len(slots)
        out = torch.full((m + 2,), 7.0, dtype=torch.float64, device="cuda")
        if m:
            s, a, l = _dev(stamps, np.float64), _dev(arrivals, np.float64), _dev(slots, np.int32)
            assert self.lib.tip_clock_map(self.ptr, self.n, l.data_ptr(), s.data_ptr(), a.data_ptr(), m, leak, slew, out[1:].data_ptr(), _st()) == 0
        o = out.cpu().numpy()
        assert o[0] == 7.0 and o[-1] == 7.0
        return o[1:-1]

    def image(self):
        b = self.buf.cpu().numpy()
        assert (b[:32] == 0xCD).all() and (b[-32:] == 0xCD).all()
        return b[32:-32].reshape(self.n, 32)

    def get(self):
        sl = torch.arange(self.n, dtype=torch.int32, device="cuda")
        theta = torch.full((self.n,), 7.0, dtype=torch.float64, device="cuda")
        counts = torch.full((self.n, 2), 9, dtype=torch.int32, device="cuda")
        assert self.lib.tip_clock_get(self.ptr, self.n, sl.data_ptr(), self.n, theta.data_ptr(), counts.data_ptr(), _st()) == 0
        return theta.cpu().numpy(), counts.cpu().numpy()


def _arrivals(rng, n, m):
    """m arrivals for n hubs, each hub on a clock of its own (offsets 1.7e9 + 3 slot): stamps at 100 Hz per slot, and among them
    duplicates, out-of-order stamps, NaN and Inf stamps, NaN arrival times, and slots outside [0, n)."""
    slots = rng.randint(0, n, size=m)
    stamps, seen = np.empty(m), {}
    for j, s in enumerate(slots):
        seen[s] = seen.get(s, 0) + 1
        stamps[j] = 5.0 + 0.01 * seen[s] + rng.uniform(-0.002, 0.002)
    kind = rng.randint(0, 12, size=m)
    kind[:1] = 99                                                 # (the first arrival is a good one)
    for j in np.flatnonzero(kind == 0):
        stamps[j] = stamps[max(0, j - n)]                         # likely a duplicate of, or older than, the slot's last
    stamps[kind == 1] -= 0.05
    stamps[kind == 2] = NAN
    stamps[kind == 3] = np.inf
    arrivals = stamps + 1.7e9 + 3.0 * slots + 0.002 + rng.exponential(0.003, size=m)
    arrivals[kind == 4] = NAN
    slots = slots.copy()
    slots[kind == 5] = rng.choice([-1, n, n + 7, -(1 << 30), 1 << 30], size=int((kind == 5).sum()))
    return slots.astype(np.int64), stamps, arrivals


# ---- (a) the clock ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("m", [1, 64, 65, 130])
def test_clock_map_equals_the_oracle_bit_for_bit(n, m):
    """times_out, theta, s_prev, count and rejected equal the oracle's as bit patterns, fed at once and in 3 and 7 chunks; an arrival for
    a slot outside [0, n) writes nothing; nothing around the state or the output is written."""
    rng = np.random.RandomState(100 * n + m)
    slots, stamps, arrivals = _arrivals(rng, n, m)
    ref = sy.Clocks(n)
    want = ref.map(slots, stamps, arrivals)
    inside = (slots >= 0) & (slots < n)
    if m >= 64:
        cnt, rej = ref.counts()
        assert rej.sum() >= 6 and (~inside).sum() >= 2 and np.isnan(stamps).any() and np.isnan(arrivals[np.isfinite(stamps)]).any()
    images = []
    for chunks in (1, 3, 7):
        c = _Clock(n)
        got = np.concatenate([c.map(slots[i], stamps[i], arrivals[i]) for i in np.array_split(np.arange(m), chunks)])
        assert np.array_equal(_i64(got[inside]), _i64(want[inside])), chunks
        assert (got[~inside] == 7.0).all(), chunks
        images.append(c.image())
        assert np.array_equal(images[-1], ref.image()), chunks
        theta, counts = c.get()
        assert np.array_equal(_i64(theta), _i64(ref.theta())) and np.array_equal(counts, np.stack(ref.counts(), axis=1)), chunks
    assert np.isfinite(want[inside]).sum() >= 1


def test_clock_reset_of_one_slot_leaves_the_others_and_lists_that_name_no_slot():
    n = 33
    rng = np.random.RandomState(3)
    slots, stamps, arrivals = _arrivals(rng, n, 130)
    c = _Clock(n)
    c.map(slots, stamps, arrivals)
    before = c.image().copy()
    assert before[7].any() and before[32].any()
    lst = _dev([7, -1, n, 1 << 30], np.int32)
    assert c.lib.tip_clock_reset(c.ptr, n, lst.data_ptr(), 4, _st()) == 0
    after = c.image()
    keep = np.arange(n) != 7
    assert np.array_equal(after[keep], before[keep]) and not after[7].any()
    theta = torch.full((5,), 7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((5, 2), 9, dtype=torch.int32, device="cuda")
    lst = _dev([32, -1, n, 7], np.int32)
    assert c.lib.tip_clock_get(c.ptr, n, lst.data_ptr(), 4, theta.data_ptr(), counts.data_ptr(), _st()) == 0
    assert theta.cpu().tolist()[1:] == [7.0, 7.0, 0.0, 7.0] and counts.cpu().tolist()[1:] == [[9, 9], [9, 9], [0, 0], [9, 9]]
    assert theta.cpu().numpy()[:1].view(np.int64)[0] == before[32, :8].view(np.int64)[0]
    # the host class: the same numbers, NaN where nothing is mapped, counts and offsets by slot
    k = sensors.ClockSync(n, "cuda")
    ref = sy.Clocks(n)
    got = k.map(slots, stamps, arrivals)
    assert got.dtype == torch.float64 and got.is_cuda and np.array_equal(_i64(got.cpu().numpy()), _i64(ref.map(slots, stamps, arrivals)))
    got2 = k.map(torch.tensor(slots).cuda(), torch.tensor(stamps + 2.0).cuda(), arrivals + 2.0)       # CUDA tensors where they lie
    assert np.array_equal(_i64(got2.cpu().numpy()), _i64(ref.map(slots, stamps + 2.0, arrivals + 2.0)))
    assert np.array_equal(_i64(k.offsets().cpu().numpy()), _i64(ref.theta()))
    assert [c_.cpu().tolist() for c_ in k.counts()] == [list(c_) for c_ in ref.counts()]
    k.reset([0, 5])
    ref.reset([0, 5])
    assert np.array_equal(_i64(k.offsets([0, 5, 6]).cpu().numpy()), _i64(ref.theta()[[0, 5, 6]])) and k.map([], [], []).shape == (0,)
    for bad in (np.array([1.0], dtype=f32), torch.tensor([1.0], dtype=torch.float32)):
        with pytest.raises(ValueError, match="map: stamps are float64 seconds"):
            k.map([0], bad, [2.0])
        with pytest.raises(ValueError, match="map: arrivals are float64 seconds"):
            k.map([0], [1.0], bad)
    with pytest.raises(ValueError, match=r"map: slots, stamps and arrivals are \[m\]"):
        k.map([0, 1], [1.0], [2.0])
    torch.cuda.synchronize()


# ---- (b) the fused push ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("depth", [2, 8])
@pytest.mark.parametrize("m", [65, 130])
def test_fused_push_is_map_then_push(n, depth, m):
    """Two rounds of m arrivals (the second on rings that hold packets): ring bytes, the resampler's counters, the clock blocks and
    times_out of the one launch equal those of tip_clock_map followed by tip_resample_push on a second pair of states, and the oracle's."""
    lib = tlib.load()
    rng = np.random.RandomState(1000 * n + 10 * depth + m)
    nb = ctypes.c_size_t()
    assert lib.tip_resample_state_bytes(n, depth, ctypes.byref(nb)) == 0
    block = nb.value // n
    rings = [torch.full(((n + 2) * block,), 0xCD, dtype=torch.uint8, device="cuda") for _ in range(2)]
    ptr = [r.data_ptr() + block for r in rings]
    clocks = [_Clock(n), _Clock(n)]
    for p in ptr:
        assert lib.tip_resample_reset(p, n, depth, None, 0, _st()) == 0
    ref_c, ref_r = sy.Clocks(n), sy.Rings(n, depth)
    for rnd in range(2):
        slots, stamps, arrivals = _arrivals(rng, n, m)
        stamps = stamps + 2.0 * rnd
        arrivals = arrivals + 2.0 * rnd
        pk = ro.motion_packets(rng, m)
        d_pk, d_sl, d_st, d_ar = _dev(pk, f32), _dev(slots, np.int32), _dev(stamps, np.float64), _dev(arrivals, np.float64)
        two = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
        assert lib.tip_clock_map(clocks[0].ptr, n, d_sl.data_ptr(), d_st.data_ptr(), d_ar.data_ptr(), m, sy.LEAK, sy.SLEW, two.data_ptr(), _st()) == 0
        assert lib.tip_resample_push(ptr[0], n, depth, d_pk.data_ptr(), d_sl.data_ptr(), two.data_ptr(), m, _st()) == 0
        one = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
        assert lib.tip_clock_push(ptr[1], clocks[1].ptr, n, depth, d_pk.data_ptr(), d_sl.data_ptr(), d_st.data_ptr(), d_ar.data_ptr(), m,
                                  sy.LEAK, sy.SLEW, one.data_ptr() if rnd == 0 else None, _st()) == 0
        if rnd == 0:
            assert torch.equal(one.view(torch.int64), two.view(torch.int64))
        mapped = ref_c.map(slots, stamps, arrivals)
        ref_r.push(pk, slots, mapped)
        a, b = rings[0].cpu().numpy(), rings[1].cpu().numpy()
        assert (b[:block] == 0xCD).all() and (b[-block:] == 0xCD).all()
        assert np.array_equal(a, b), rnd
        assert np.array_equal(clocks[0].image(), clocks[1].image()) and np.array_equal(clocks[1].image(), ref_c.image()), rnd
        assert np.array_equal(b[block:-block].reshape(n, block), ref_r.image()), rnd
    have, dropped, total = ref_r.counts()
    assert dropped.sum() >= 6 and total.sum() >= m and (have.max() == depth if n == 1 else have.max() >= 2)      # (n = 1: the ring wraps)
    counts = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
    sl = torch.arange(n, dtype=torch.int32, device="cuda")
    assert lib.tip_resample_get(ptr[1], n, depth, sl.data_ptr(), n, counts.data_ptr(), _st()) == 0
    assert np.array_equal(counts.cpu().numpy(), np.stack([have, dropped, total], axis=1))


def test_push_with_arrivals_and_sync_is_the_one_launch():
    """PacketResampler.push(arrivals=, sync=) from host arrays and from CUDA tensors leaves what ClockSync.map + push leave; one of the
    two keywords alone, a sync of another size and float32 arrival times are refused and launch nothing."""
    n = 5
    rng = np.random.RandomState(9)
    a, b = sensors.PacketResampler(n, "cuda", depth=4), sensors.PacketResampler(n, "cuda", depth=4)
    ka, kb = sensors.ClockSync(n, "cuda"), sensors.ClockSync(n, "cuda")
    for rnd in range(3):
        slots, stamps, arrivals = _arrivals(rng, n, 40)
        stamps, arrivals = stamps + rnd, arrivals + rnd
        pk = ro.motion_packets(rng, 40)
        a.push(pk, slots, ka.map(slots, stamps, arrivals))
        if rnd == 1:
            b.push(torch.tensor(pk).cuda(), torch.tensor(slots).cuda(), torch.tensor(stamps).cuda(), arrivals=arrivals, sync=kb)
        else:
            b.push(pk, slots, stamps.tolist(), arrivals=arrivals, sync=kb)
        assert torch.equal(a.state, b.state) and torch.equal(ka.state, kb.state), rnd
    assert int(b.counts()[1].sum()) >= 3 and int(kb.counts()[1].sum()) >= 3
    before, kbefore = b.state.clone(), kb.state.clone()
    pk = ro.motion_packets(rng, 2)
    with pytest.raises(ValueError, match="arrivals and sync come together"):
        b.push(pk, [0, 1], [1.0, 2.0], arrivals=[3.0, 4.0])
    with pytest.raises(ValueError, match="arrivals and sync come together"):
        b.push(pk, [0, 1], [1.0, 2.0], sync=kb)
    with pytest.raises(ValueError, match="sync is a ClockSync of 5 slots"):
        b.push(pk, [0, 1], [1.0, 2.0], arrivals=[3.0, 4.0], sync=sensors.ClockSync(4, "cuda"))
    with pytest.raises(ValueError, match="push: arrivals are float64 seconds"):
        b.push(pk, [0, 1], [1.0, 2.0], arrivals=np.array([3.0, 4.0], dtype=f32), sync=kb)
    with pytest.raises(ValueError, match=r"arrivals is \[m\]"):
        b.push(pk, [0, 1], [1.0, 2.0], arrivals=[3.0], sync=kb)
    b.push(pk[:0], [], [], arrivals=[], sync=kb)
    assert torch.equal(b.state, before) and torch.equal(kb.state, kbefore)
    torch.cuda.synchronize()


# ---- (c) recorded sequences through the clock ------------------------------------------------------------------------------------------------
def test_sync_sequences_equal_the_live_rule_and_the_oracle():
    """Sequences of 1, 64 and 257 rows (the third with a duplicate stamp and a NaN arrival time): bit for bit the oracle's, and a live
    ClockSync fed the sequence in chunks of 50."""
    rng = np.random.RandomState(21)
    st, ar = [], []
    for i, L in enumerate((1, 64, 257)):
        s, a, _, _ = sy.hub(rng, L, rate_hz=(100.0, 120.0, 50.0)[i], offset=1.7e9 + 11.0 * i, drift=(40e-6, -25e-6, 0.0)[i])
        st.append(s)
        ar.append(a)
    st[2][100] = st[2][99]
    ar[2][200] = NAN
    got = sensors.sync_sequences(st, ar)
    assert [g.shape for g in got] == [(1,), (64,), (257,)] and all(isinstance(g, np.ndarray) and g.dtype == np.float64 for g in got)
    live = sensors.ClockSync(3, "cuda")
    for i in range(3):
        want, _ = sy.clock_sequence(st[i], ar[i])
        assert np.array_equal(_i64(got[i]), _i64(want)), i
        parts = [live.map(np.full(len(c), i), st[i][c], ar[i][c]).cpu().numpy() for c in np.array_split(np.arange(len(st[i])), max(1, len(st[i]) // 50))]
        assert np.array_equal(_i64(np.concatenate(parts)), _i64(want)), i
    assert np.isnan(got[2][[100, 200]]).all() and np.isfinite(np.delete(got[2], [100, 200])).all()
    other = sensors.sync_sequences(st, ar, leak=0.0, slew=0.25)
    assert np.array_equal(_i64(other[1]), _i64(sy.clock_sequence(st[1], ar[1], 0.0, 0.25)[0])) and not np.array_equal(other[1], got[1])


# ---- (d) predicted ticks: every flag -------------------------------------------------------------------------------------------------------------
GRID = 1.0 / 1024.0                   # every stamp and query time of the emit test is a multiple of this: exact at 0 and at 1.7e9
MAX_HOLD, MAX_PREDICT = 40 * GRID, 30 * GRID
# query times relative to the slot's newest stamp, in grid steps (stamps are 8 .. 12 steps apart): before the ring; inside it; at the
# newest stamp; a little past it (predicted); further than twice the bracket but young enough to hold; older than max_hold
OFFSETS = (-2000, -1500, -1001, -13, -7, -3, -1, 0, 1, 3, 6, 11, 16, 26, 29, 38, 41, 60, 500)


def _predict_case(n, depth, t0):
    """n rings of depth + 3 pushed packets each and the query times [len(OFFSETS), n].  Slot s % 4 == 3 is left empty.  In slot 0 the
    newest two packets carry a zero quaternion (older packet, sensor 1), a NaN quaternion (newer, sensor 2), a NaN acceleration in the
    newer (sensor 3) and in the older packet (sensor 4)."""
    rng = np.random.RandomState(7 * n + depth)
    L = depth + 3
    pk, st, sl = [], [], []
    for s in range(n):
        if s % 4 == 3:
            continue
        steps = rng.randint(8, 13, size=L)
        stamps = t0 + (1000 + 7 * s + np.cumsum(steps)) * GRID
        p = ro.motion_packets(rng, L).reshape(L, 6, 7)
        if s == 0:
            p[L - 2, 1, :4] = 0.0
            p[L - 1, 2, 1] = np.nan
            p[L - 1, 3, 5] = np.nan
            p[L - 2, 4, 6] = np.nan
        pk.append(p.reshape(L, 42))
        st.append(stamps)
        sl.append(np.full(L, s))
    order = np.argsort(np.concatenate(st), kind="stable")
    pk, st, sl = np.concatenate(pk)[order].astype(f32), np.concatenate(st)[order], np.concatenate(sl)[order]
    newest = np.full(n, t0 + 1100 * GRID)
    for s in range(n):
        if (sl == s).any():
            newest[s] = st[sl == s].max()
    return pk, st, sl, np.stack([newest + o * GRID for o in OFFSETS])


def _emit_all(pk, st, sl, queries, n, depth, max_predict, slerp=False):
    """Fresh rings, three emits on the empty pool, the push, one emit per query row -> (rows [3 + Q, n, 42], flags [3 + Q, n])."""
    rs = sensors.PacketResampler(n, "cuda", mode="slerp" if slerp else "predict", delay=0.0, max_hold=MAX_HOLD, depth=depth,
                                 max_predict=None if slerp else max_predict)
    rows, flags = [], []
    for k in range(3):
        rows.append(rs.emit(float(queries[0, 0]) + k).clone())
        flags.append(rs.flags.clone())
    rs.push(pk, sl, st)
    for q in queries:
        rows.append(rs.emit(q).clone())
        flags.append(rs.flags.clone())
    torch.cuda.synchronize()
    return torch.stack(rows).cpu().numpy(), torch.stack(flags).cpu().numpy()


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("depth", [2, 8])
def test_predict_emit_every_flag(n, depth):
    """tip_predict_emit on n slots (one tile and one slot of the next at 33) against the oracle, at stamps from 0 and from 1.7e9."""
    per_epoch = []
    for t0 in (0.0, 1.7e9):
        pk, st, sl, queries = _predict_case(n, depth, t0)
        assert np.array_equal((st - t0) / GRID, np.round((st - t0) / GRID)) and np.array_equal((queries - t0) / GRID, np.round((queries - t0) / GRID))
        got, got_flags = _emit_all(pk, st, sl, queries, n, depth, MAX_PREDICT)
        ref = sy.Rings(n, depth)
        lo, hi, flags = [], [], []
        for k in range(3):
            r32, f = ref.emit(queries[0, 0] + k, 0.0, MAX_HOLD, MAX_PREDICT, f32)
            lo.append(r32), hi.append(r32.astype(np.float64)), flags.append(f)
        ref.push(pk, sl, st)
        for q in queries:
            r32, f = ref.emit(q, 0.0, MAX_HOLD, MAX_PREDICT, f32)
            r64, f64_ = ref.emit(q, 0.0, MAX_HOLD, MAX_PREDICT, np.float64)
            assert np.array_equal(f, f64_)
            lo.append(r32), hi.append(r64), flags.append(f)
        lo, hi, flags = np.stack(lo), np.stack(hi), np.stack(flags)
        seen = {int(f): int((flags == f).sum()) for f in range(6)}
        print(f"n {n} depth {depth} t0 {t0:g}: oracle flags {seen}")
        assert all(v >= 3 for v in seen.values()), seen                       # an empty comparison cannot pass
        assert np.array_equal(got_flags, flags), np.argwhere(got_flags != flags)[:8]
        per_epoch.append(flags)
        pred, interp = flags == sy.F_PREDICT, flags == sy.F_INTERP
        rest = ~pred & ~interp
        assert np.array_equal(got[rest].view(np.int32), lo[rest].view(np.int32))              # held: the packet; stale, empty, early: NaN
        # interpolated rows: the slerp entry's on the same state, bit for bit; max_predict = 0: the slerp entry's everywhere
        slerp, slerp_flags = _emit_all(pk, st, sl, queries, n, depth, None, slerp=True)
        assert (slerp_flags[interp] == ro.F_INTERP).all() and np.array_equal(got[interp].view(np.int32), slerp[interp].view(np.int32))
        assert np.array_equal(slerp_flags[~pred], flags[~pred]) and (slerp_flags[pred] == ro.F_HELD).all()
        zero, zero_flags = _emit_all(pk, st, sl, queries, n, depth, 0.0)
        assert np.array_equal(zero_flags, slerp_flags) and np.array_equal(zero.view(np.int32), slerp.view(np.int32))
        # predicted rows: NaN where the fp64 oracle's are, within 3 x its fp32 noise, unit quaternions
        g, l, h = got[pred], lo[pred], hi[pred]
        assert np.array_equal(np.isnan(g), np.isnan(h)) and np.array_equal(np.isnan(l), np.isnan(h))
        with np.errstate(invalid="ignore"):
            noise_r = float(np.nanmax(np.abs(ro.rotations(l) - ro.rotations(h))))
            noise_a = float(np.nanmax(np.abs(ro.accelerations(l) - ro.accelerations(h))))
            err_r = float(np.nanmax(np.abs(ro.rotations(g) - ro.rotations(h))))
            err_a = float(np.nanmax(np.abs(ro.accelerations(g) - ro.accelerations(h))))
            norm = np.linalg.norm(g.reshape(-1, 6, 7)[..., :4].astype(np.float64), axis=-1)
        print(f"  {int(pred.sum())} predicted rows; fp32 noise rot {noise_r:.3e} acc {noise_a:.3e}; device error rot {err_r:.3e} "
              f"({err_r / noise_r:.2f} x) acc {err_a:.3e} ({err_a / noise_a:.2f} x)")
        assert err_r <= 3.0 * noise_r and err_a <= 3.0 * noise_a
        assert float(np.nanmax(np.abs(norm - 1.0))) <= 3.0 * float(np.finfo(f32).eps)
        # the NaN rules, stated from the inputs: slot 0's newest two packets
        r0 = got[:, 0][pred[:, 0]].reshape(-1, 6, 7)
        assert len(r0) >= 3
        want_nan = np.zeros((6, 7), dtype=bool)
        want_nan[1] = want_nan[2] = True                                      # a zero quaternion in the older, a NaN one in the newer packet
        want_nan[3, 4:] = True                                                # a NaN in the newer packet's acceleration
        assert all(np.array_equal(np.isnan(r), want_nan) for r in r0)         # (sensor 4, NaN in the older acceleration only: finite)
    assert np.array_equal(per_epoch[0], per_epoch[1])


# ---- (e) recorded sessions in predict mode -----------------------------------------------------------------------------------------------------
def test_predict_rows_equal_the_live_resampler_tick_by_tick():
    """Three ragged sessions at 100, 120 and 50 Hz through resample_sequences(mode="predict"): every row and flag equals what a live
    PacketResampler(mode="predict") emits at that tick after being pushed everything stamped up to it, bit for bit; flags equal the
    oracle's; most rows are predicted."""
    rng = np.random.RandomState(41)
    t0, K, depth = 7.0, 36, 4
    seqs = []
    for rate, secs in ((100.0, 0.9), (120.0, 0.75), (50.0, 1.0)):
        L = int(secs * rate)
        seqs.append((ro.motion_packets(rng, L), ro.stamps_at(rng, L, rate, t0=t0 + rng.uniform(0.0, 0.01))))
    ticks = sensors.tick_times(t0 + 0.03, K)
    kw = dict(mode="predict", delay=0.0, max_hold=0.03, depth=depth, max_predict=0.02)
    off, off_flags = sensors.resample_sequences([p for p, _ in seqs], [s for _, s in seqs], 60.0, t_start=float(ticks[0]), host=True, **kw)
    assert all(len(o) >= K for o in off)
    rs = sensors.PacketResampler(3, "cuda", **kw)
    at = [0, 0, 0]
    for k, t in enumerate(ticks):
        for s, (pk, st) in enumerate(seqs):
            new = int(np.searchsorted(st, t, side="right"))
            rs.push(pk[at[s]:new], [s] * (new - at[s]), st[at[s]:new])
            at[s] = new
        row, fl = rs.emit(float(t)).cpu().numpy(), rs.flags.cpu().numpy()
        for s in range(3):
            assert fl[s] == off_flags[s][k] and np.array_equal(row[s].view(np.int32), off[s][k].view(np.int32)), (k, s)
    for s, (pk, st) in enumerate(seqs):
        want = sy.rows(pk, st, ticks, 0.0, 0.03, 0.02, depth)[1]
        assert np.array_equal(off_flags[s][:K], want), s
        print(f"session {s}: flags {np.bincount(want, minlength=6).tolist()}")
        assert (want == sy.F_PREDICT).sum() >= K // 2
    assert min(at) > 2 * depth


# ---- (f) the whole chain in front of an engine ---------------------------------------------------------------------------------------------------
def test_clock_sync_and_predicted_ticks_in_front_of_an_engine(paper):
    """Two hubs on clocks of their own (100 and 120 Hz, started 100 s apart, 1.7e9 s behind the server, 40 / -25 ppm of drift) behind 2 ms + Exp(1 ms) of network:
    ClockSync + push(arrivals=, sync=) + emit in mode "predict" with delay 0 in front of StreamingEngine.step_packets, 50 ticks — once
    launch by launch, once with the emit replayed from a captured graph whose t is a CUDA float64 tensor.  The engine's outputs of
    the two runs match bit for bit; most rows are predicted."""
    m, _ = paper
    n, frames = 2, 50
    rng = np.random.RandomState(67)
    hubs = []
    for i, rate in enumerate((100.0, 120.0)):
        L = int((frames / 60.0 + 0.2) * rate)
        s, a, _, _ = sy.hub(rng, L, rate_hz=rate, offset=1.7e9 - 100.0 * i, drift=(40e-6, -25e-6)[i], mean_jitter=0.001, s0=12.5 + 100.0 * i)
        hubs.append((ro.motion_packets(rng, L), s, a))
    ticks = sensors.tick_times(min(a[0] for _, _, a in hubs) + 0.05, frames)
    _, tables = so.case(n, 71)
    s0 = np.stack([synth.make_recording(2, seed=310 + i)[1] for i in range(n)])

    def run(graphed):
        fr = sensors.SensorFrontEnd(n, "cuda")
        fr.load(range(n), tables)
        eng = tip_amd.streaming.StreamingEngine(m, s0, use_graph=False)
        rs = sensors.PacketResampler(n, "cuda", mode="predict", delay=0.0, max_hold=0.1)
        clk = sensors.ClockSync(n, "cuda")
        t_dev = torch.zeros(n, dtype=torch.float64, device="cuda")
        buf = torch.empty((n, 42), dtype=torch.float32, device="cuda")
        g = None
        outs, flags, at = [], [], [0] * n
        for k, t in enumerate(ticks):
            arr = []
            for s, (pk, st, ar) in enumerate(hubs):
                new = int(np.searchsorted(ar, t, side="right"))       # (arrival times ascend here: the jitter is below a period)
                arr += [(ar[j], s, j) for j in range(at[s], new)]
                at[s] = new
            arr.sort()
            if arr:
                rs.push(np.stack([hubs[s][0][j] for _, s, j in arr]), [s for _, s, _ in arr], np.array([hubs[s][1][j] for _, s, j in arr]),
                        arrivals=np.array([a for a, _, _ in arr]), sync=clk)
            t_dev.fill_(float(t))
            if not graphed:
                rs.emit(t_dev, out=buf)
            elif g is None:
                rs.emit(t_dev, out=buf)                               # (the first frame launches, and is captured for the others)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    rs.emit(t_dev, out=buf)
            else:
                g.replay()
            flags.append(rs.flags.clone())
            o = eng.step_packets(fr, buf)
            outs.append(None if o is None else {key: o[key].clone() for key in ("s_rest", "c_t", "y_last")})
        torch.cuda.synchronize()
        return outs, torch.stack(flags).cpu().numpy(), clk.counts()[0].cpu().tolist(), at

    for _, s, a in hubs:
        assert (np.diff(a) > 0).all()
    a_out, a_flags, a_counts, at = run(False)
    b_out, b_flags, b_counts, _ = run(True)
    assert np.array_equal(a_flags, b_flags) and a_counts == b_counts == at and min(at) > 60
    print(f"flags over {frames} ticks x {n} slots: {np.bincount(a_flags.reshape(-1), minlength=6).tolist()}")
    assert (a_flags == sy.F_PREDICT).sum() >= frames * n * 3 // 4
    produced = 0
    for k, (oa, ob) in enumerate(zip(a_out, b_out)):
        assert (oa is None) == (ob is None), k
        if oa is not None:
            for key in oa:
                assert torch.equal(oa[key].view(torch.int32), ob[key].view(torch.int32)), (k, key)
            produced += bool(torch.isfinite(oa["y_last"]).all())
    assert produced >= frames - 8
