"""GPU tests of the timestamped-packet resampler (csrc/tip_resample.hip; tip_amd.sensors.PacketResampler, resample_sequences) against
its numpy oracle (tests/resample_oracle.py): recorded sequences at the edges of the kernel's tile, every branch of the emit rule and of
the interpolation, the live rings against the offline launch bit for bit, the demo's hold, on-grid wearers, epoch-sized stamps, reset,
and the resampler in front of the engines and of recorded sessions.

No fixture from the reference is needed: the reference has no resampling.  Its one rule — the live demo's zero-order hold, the reader
thread overwriting current_reading (live_demo_new.py:82-115) and the loop taking it once per tick (:161-162) — is mode "hold" with
delay 0, restated by numpy indexing in test_hold_is_the_demos_rule.

Bounds: flags are equal (every decision is an fp64 comparison of stated expressions); a held packet is the packet, bit for bit; an
interpolated row is within 3 x the fp32 noise of the fp64 oracle, the rule of tests/test_sensor_gpu.py: noise = max |oracle in fp32 -
oracle in fp64| on the same inputs, measured per test, on the rotation matrices of the output quaternions (R, not q: the sign is free)
and on the accelerations separately."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import resample_oracle as ro
import sensor_oracle as so
import tip_amd
from tip_amd import lib as tlib
from tip_amd import sensors, synth
from test_staggered_streams_gpu import paper  # noqa: F401

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE = {ro.SLERP: "slerp", ro.HOLD: "hold"}
UNIT = 3.0 * float(np.finfo(f32).eps)        # |q| after q / sqrt(q.q) in fp32: the sum, the root and the division, half an ulp each and twice


def _bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=f32).view(np.int32)


def _tile():
    rows = ctypes.c_int()
    assert tlib.load().tip_resample_tile(ctypes.byref(rows)) == 0
    return rows.value


def _rows_dev(seqs, ticks, delay, hold, mode, depth):
    """tip_resample_rows on sequences [(packets, stamps)] at the given ticks (one array per sequence), with a guard row on either side
    of both outputs.  -> (list of [K_i, 42] float32, list of [K_i] uint8)."""
    lib, st = tlib.load(), torch.cuda.current_stream().cuda_stream
    lens, out_lens = [len(s) for _, s in seqs], [len(t) for t in ticks]
    pk = torch.tensor(np.concatenate([p.reshape(-1, 42) for p, _ in seqs]).astype(f32)).cuda()
    stamps = torch.tensor(np.concatenate([np.asarray(s, dtype=np.float64) for _, s in seqs])).cuda()
    t_out = torch.tensor(np.concatenate([np.asarray(t, dtype=np.float64) for t in ticks] + [np.zeros(1)])).cuda()
    in_off = torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int64).cuda()
    out_off = torch.tensor(np.concatenate(([0], np.cumsum(out_lens))), dtype=torch.int64).cuda()
    K = int(sum(out_lens))
    out = torch.full((K + 2, 42), 7.0, device="cuda")
    flags = torch.full((K + 2,), 9, dtype=torch.uint8, device="cuda")
    assert lib.tip_resample_rows(pk.data_ptr(), stamps.data_ptr(), in_off.data_ptr(), int(pk.shape[0]), t_out.data_ptr(), out_off.data_ptr(), K,
                                 len(seqs), float(delay), -1.0 if hold is None else float(hold), mode, depth, out[1:].data_ptr(),
                                 flags[1:].data_ptr(), st) == 0
    torch.cuda.synchronize()
    o, f = out.cpu().numpy(), flags.cpu().numpy()
    assert (o[0] == 7.0).all() and (o[-1] == 7.0).all() and f[0] == 9 and f[-1] == 9
    at = np.concatenate(([0], np.cumsum(out_lens))) + 1
    return [o[a:b] for a, b in zip(at[:-1], at[1:])], [f[a:b] for a, b in zip(at[:-1], at[1:])]


def _oracle(seqs, ticks, delay, hold, mode, depth):
    """The oracle in fp32 and in fp64 on the same inputs: ([K, 42] float32, [K, 42] float64, flags [K]), the sequences back to back."""
    lo = [ro.rows(p, s, t, delay, hold, mode, depth, f32) for (p, s), t in zip(seqs, ticks)]
    hi = [ro.rows(p, s, t, delay, hold, mode, depth, np.float64) for (p, s), t in zip(seqs, ticks)]
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(lo, hi))
    return np.concatenate([a[0] for a in lo]), np.concatenate([b[0] for b in hi]), np.concatenate([a[1] for a in lo])


def _hold_to_oracle(got, got_flags, ref32, ref64, flags, who):
    """Flags equal; held and NaN rows bit for bit; interpolated rows within 3 x the measured fp32 noise, their NaN columns where the
    oracle's are, their quaternions unit.  Prints the figures before it asserts."""
    assert np.array_equal(got_flags, flags), (who, np.flatnonzero(got_flags != flags)[:8])
    it = flags == ro.F_INTERP
    assert np.array_equal(_bits(got[~it]), _bits(ref32[~it])), who
    if not it.any():
        print(f"{who}: {len(flags)} rows, none interpolated")
        return
    g, lo, hi = got[it], ref32[it], ref64[it]
    assert np.array_equal(np.isnan(g), np.isnan(hi)) and np.array_equal(np.isnan(lo), np.isnan(hi)), who
    with np.errstate(invalid="ignore"):
        noise_r = float(np.nanmax(np.abs(ro.rotations(lo) - ro.rotations(hi))))
        noise_a = float(np.nanmax(np.abs(ro.accelerations(lo) - ro.accelerations(hi))))
        err_r = float(np.nanmax(np.abs(ro.rotations(g) - ro.rotations(hi))))
        err_a = float(np.nanmax(np.abs(ro.accelerations(g) - ro.accelerations(hi))))
        norm = np.linalg.norm(g.reshape(-1, 6, 7)[..., :4].astype(np.float64), axis=-1)
        off_unit = float(np.nanmax(np.abs(norm - 1.0)))
    print(f"{who}: {int(it.sum())} interpolated rows of {len(flags)}; fp32 noise rot {noise_r:.3e} acc {noise_a:.3e}; "
          f"device error rot {err_r:.3e} acc {err_a:.3e}; | |q| - 1 | {off_unit:.3e}")
    assert err_r <= 3.0 * noise_r and err_a <= 3.0 * noise_a, who
    assert off_unit <= UNIT, who


# ---- (a) recorded sequences against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,delay,hold", [(ro.SLERP, 0.02, None), (ro.SLERP, 0.02, 0.03), (ro.HOLD, 0.0, 0.05)])
def test_rows_match_the_oracle(mode, delay, hold):
    """Sequences of 1, 2, 17 and 130 packets, each at 30, 59.94, 100 and 120 Hz with a jitter of a fifth of a period, each taken at 0,
    1, tile - 1, tile and tile + 1 ticks of the 60 Hz grid that start a little before its first packet: 80 ragged sequences, one
    launch."""
    rng = np.random.RandomState(17)
    tile = _tile()
    seqs, ticks = [], []
    for L, rate, K in itertools.product((1, 2, 17, 130), (30.0, 59.94, 100.0, 120.0), (0, 1, tile - 1, tile, tile + 1)):
        t0 = 50.0 + rng.uniform(0.0, 1.0)
        seqs.append((ro.motion_packets(rng, L), ro.stamps_at(rng, L, rate, t0=t0)))
        ticks.append(sensors.tick_times(t0 - 0.021 if K > 1 else t0 + 0.5 / rate + delay, K))
    got, got_flags = _rows_dev(seqs, ticks, delay, hold, mode, depth=8)
    ref32, ref64, flags = _oracle(seqs, ticks, delay, hold, mode, 8)
    print({int(f): int((flags == f).sum()) for f in range(5)})
    assert (flags == ro.F_HELD).sum() >= 3 and (mode == ro.HOLD or (flags == ro.F_INTERP).sum() >= 60)
    _hold_to_oracle(np.concatenate(got), np.concatenate(got_flags), ref32, ref64, flags, f"rows {MODE[mode]} {delay} {hold}")


# ---- (b) every branch ------------------------------------------------------------------------------------------------------------------
DELAY, MAX_HOLD, DEPTH = 0.02, 0.03, 8


@pytest.fixture(scope="module")
def branches():
    """Four sequences of 55 packets at 100 Hz under 40 ticks each, built to reach every branch of the emit rule and of the interpolation, with
    the number of output rows (or sensors of output rows) that reach each; consecutive packets are about 0.15 rad apart (< 3.0 rad: at pi
    the shortest arc is ambiguous).  Per sequence: no packet before tick 3 (flag 3); tick 4 sees two packets, both after t - delay
    (flag 4); a packet stamped exactly at tick 10 - delay (u == 0); a packet stamped exactly at tick 20 - delay and then nothing for
    55 ms (tau == s_last, then a packet too old to hold, then a bracket longer than max_hold); the packets end before the ticks do
    (flag 1, then 2).  Sensor 5 of sequences 0 and 1 never moves (the small-angle switch); every quaternion has a random sign (the
    flip); packets 12, 35, 40 and 45 carry a zero, a NaN and an Inf quaternion and a NaN acceleration in sensors 1, 2, 3 and 4."""
    rng = np.random.RandomState(29)
    seqs, ticks, L = [], [], 55
    for j in range(4):
        t0 = 100.0 + 0.37 * j
        tk = sensors.tick_times(t0, 40)
        st = t0 + 0.0512 + 0.01 * np.arange(L) + rng.uniform(-0.0015, 0.0015, size=L)
        pk = ro.motion_packets(rng, L).reshape(L, 6, 7)
        if j < 2:
            still = pk[0, 5, :4] / np.linalg.norm(pk[0, 5, :4])
            pk[:, 5, :4] = still * rng.uniform(0.5, 2.0, size=(L, 1)) * rng.choice([-1.0, 1.0], size=(L, 1))
        pk[12, 1, :4] = 0.0
        pk[35, 2, 1] = np.nan
        pk[40, 3, 3] = np.inf
        pk[45, 4, 5] = np.nan
        exact_u0, exact_last = tk[10] - DELAY, tk[20] - DELAY
        i0, i1 = int(np.argmin(np.abs(st - exact_u0))), int(np.argmin(np.abs(st - exact_last)))
        st[i0], st[i1] = exact_u0, exact_last
        keep = ~((st > exact_last) & (st < exact_last + 0.055))
        st, pk = st[keep], pk[keep]
        assert (np.diff(st) > 0).all()
        seqs.append((pk.reshape(-1, 42).astype(f32), st))
        ticks.append(tk)
    counts = {k: 0 for k in ("flag0", "flag1", "flag2", "flag3", "flag4", "flip", "small_angle", "u_zero", "tau_is_last", "long_bracket",
                             "zero_q", "nan_q", "inf_q", "nan_acc")}
    for (pk, st), tk in zip(seqs, ticks):
        for t in tk:
            cnt = int(np.searchsorted(st, t, side="right"))
            lo = max(0, cnt - DEPTH)
            s, p, tau = st[lo:cnt], pk[lo:cnt].reshape(-1, 6, 7), t - DELAY
            f, i, u = ro.decide(s, tau, MAX_HOLD, ro.SLERP)
            counts[f"flag{f}"] += 1
            if f in (ro.F_HELD, ro.F_STALE) and len(s) and tau == s[-1]:
                counts["tau_is_last"] += 1
            if f != ro.F_INTERP:
                counts["long_bracket"] += int(len(s) > 0 and s[0] <= tau < s[-1])
                continue
            counts["u_zero"] += int(u == 0.0)
            a, b = p[i], p[i + 1]
            with np.errstate(all="ignore"):
                qa, qb = (q[:, :4] / np.sqrt((q[:, :4] * q[:, :4]).sum(-1, dtype=f32, keepdims=True)) for q in (a, b))
                dot = (qa * qb).sum(-1, dtype=f32)
            counts["flip"] += int((dot < 0).sum())
            counts["small_angle"] += int((np.abs(dot.astype(np.float64)) > 1 - 1e-6).sum())
            both = np.concatenate((a, b))
            counts["zero_q"] += int((both[:, :4] == 0).all(-1).sum())
            counts["nan_q"] += int(np.isnan(both[:, :4]).any(-1).sum())
            counts["inf_q"] += int(np.isinf(both[:, :4]).any(-1).sum())
            counts["nan_acc"] += int(np.isnan(both[:, 4:]).any(-1).sum())
    print("branches:", counts)
    return seqs, ticks, counts


def test_fixture_reaches_every_branch(branches):
    _, _, counts = branches
    assert all(v >= 3 for v in counts.values()), counts


def test_every_branch_matches_the_oracle(branches):
    """The fixture through tip_resample_rows against the oracle, and the bad readings stated from the inputs: in an interpolated row a
    sensor whose quaternion is zero, NaN or Inf in either packet of the bracket has exactly its seven columns NaN, a sensor with a NaN
    acceleration component in either packet exactly its three acceleration columns; nothing else in the row is NaN."""
    seqs, ticks, _ = branches
    got, got_flags = _rows_dev(seqs, ticks, DELAY, MAX_HOLD, ro.SLERP, DEPTH)
    ref32, ref64, flags = _oracle(seqs, ticks, DELAY, MAX_HOLD, ro.SLERP, DEPTH)
    _hold_to_oracle(np.concatenate(got), np.concatenate(got_flags), ref32, ref64, flags, "branches")
    checked = 0
    for (pk, st), tk, g in zip(seqs, ticks, got):
        for r, t in enumerate(tk):
            cnt = int(np.searchsorted(st, t, side="right"))
            lo = max(0, cnt - DEPTH)
            f, i, _ = ro.decide(st[lo:cnt], t - DELAY, MAX_HOLD, ro.SLERP)
            if f != ro.F_INTERP:
                continue
            pair = pk[lo + i: lo + i + 2].reshape(2, 6, 7)
            with np.errstate(all="ignore"):
                n2 = (pair[:, :, :4].astype(np.float64) ** 2).sum(-1)
            bad_q = (~(np.isfinite(n2) & (n2 > 0))).any(0)
            bad_a = np.isnan(pair[:, :, 4:]).any((0, 2))
            want = np.zeros((6, 7), dtype=bool)
            want[bad_q] = True
            want[bad_a, 4:] = True
            assert np.array_equal(np.isnan(g[r]).reshape(6, 7), want), (r, t)
            checked += int(want.any())
    assert checked >= 8


# ---- (c) live equals offline ---------------------------------------------------------------------------------------------------------------
def _drive(rs, seqs, ticks, extra=None, cuda_every=0):
    """The live loop: before tick k everything stamped <= t_k is pushed, the slots' arrivals interleaved in stamp order (`extra`:
    {tick: [(packet, slot, stamp)]} appended to that tick's push), then emit(t_k).  -> (rows [K, n, 42], flags [K, n]) and the number of
    arrivals per slot."""
    at, pushed = [0] * len(seqs), [0] * len(seqs)
    rows, flags = [], []
    for k, t in enumerate(ticks):
        arr = []
        for s, (pk, st) in enumerate(seqs):
            new = int(np.searchsorted(st, t, side="right"))
            arr += [(st[j], s, pk[j]) for j in range(at[s], new)]
            at[s] = new
        arr.sort(key=lambda a: a[0])
        arr += [(t_, s_, p_) for p_, s_, t_ in (extra or {}).get(k, [])]
        for _, s, _ in arr:
            pushed[s] += 1
        if arr:
            p = np.stack([a[2] for a in arr]).astype(f32)
            sl, tm = np.array([a[1] for a in arr], dtype=np.int64), np.array([a[0] for a in arr], dtype=np.float64)
            if cuda_every and k % cuda_every == 0:
                rs.push(torch.tensor(p).cuda(), torch.tensor(sl).cuda(), torch.tensor(tm).cuda())
            else:
                rs.push(p, sl, tm)
        rows.append(rs.emit(np.full(len(seqs), t) if k % 2 else float(t)).clone())
        flags.append(rs.flags.clone())
    torch.cuda.synchronize()
    return torch.stack(rows).cpu().numpy(), torch.stack(flags).cpu().numpy(), pushed


def _wearers(rng, rates, seconds, t0, jitter=0.2):
    out = []
    for rate in rates:
        L = int(seconds * rate)
        out.append((ro.motion_packets(rng, L), ro.stamps_at(rng, L, rate, t0=t0 + rng.uniform(0.0, 0.01), jitter=jitter)))
    return out


@pytest.mark.parametrize("mode,delay,hold", [("slerp", 0.022, None), ("slerp", 0.022, 0.021), ("hold", 0.0, None)])
def test_live_equals_offline_bit_for_bit(mode, delay, hold):
    """3 slots at 50, 100 and 120 Hz, depth 4, 40 ticks.  Before tick k everything stamped <= t_k is pushed — interleaved across the
    slots, several arrivals per slot, the rings wrapping many times, host arrays and CUDA tensors alike — and one push carries a packet
    of slot 1 with a stamp older than its newest, which is dropped and counted.  Every emitted row and flag equals, bit for bit, the
    row of resample_sequences on the same packets (without the dropped one) at the same tick; the flags equal the oracle's."""
    rng = np.random.RandomState(41)
    t0, K = 7.0, 40
    seqs = _wearers(rng, (50.0, 100.0, 120.0), 0.9, t0)
    ticks = sensors.tick_times(t0 + 0.03, K)
    late = (seqs[1][0][3], 1, seqs[1][1][5] - 0.004)             # pushed at tick 12: long after packet 5 went in
    rs = sensors.PacketResampler(3, "cuda", mode=mode, delay=delay, max_hold=hold, depth=4)
    live, live_flags, pushed = _drive(rs, seqs, ticks, extra={12: [late]}, cuda_every=3)
    have, dropped, total = (c.cpu().numpy() for c in rs.counts())
    assert list(dropped) == [0, 1, 0] and list(total) == [pushed[0], pushed[1] - 1, pushed[2]] and list(have) == [4, 4, 4]
    assert min(pushed) > 2 * 4
    off, off_flags = sensors.resample_sequences([p for p, _ in seqs], [s for _, s in seqs], 60.0, mode=mode, delay=delay, max_hold=hold,
                                                depth=4, t_start=float(ticks[0]), host=True)
    assert all(len(o) >= K for o in off)
    for s in range(3):
        assert np.array_equal(live_flags[:, s], off_flags[s][:K]), s
        assert np.array_equal(_bits(live[:, s]), _bits(off[s][:K])), s
        want = ro.rows(seqs[s][0], seqs[s][1], ticks, delay, hold, ro.SLERP if mode == "slerp" else ro.HOLD, 4)[1]
        assert np.array_equal(live_flags[:, s], want), s
    seen = set(live_flags.reshape(-1).tolist())
    print(f"live {mode} {delay} {hold}: flags seen {sorted(seen)}, pushed {pushed}")
    assert (ro.F_INTERP in seen) == (mode == "slerp") and (hold is None or ro.F_HELD in seen or ro.F_STALE in seen)


# ---- (d) HOLD ------------------------------------------------------------------------------------------------------------------------------
def test_hold_is_the_demos_rule():
    """mode "hold": every row is the newest packet not after t - delay, by numpy indexing — at delay 0 the demo's rule — live and
    through resample_sequences, array_equal on the bits."""
    rng = np.random.RandomState(43)
    t0, K = 3.0, 30
    seqs = _wearers(rng, (59.94, 100.0), 0.7, t0)
    ticks = sensors.tick_times(t0 + 0.05, K)
    for delay in (0.0, 0.03):
        rs = sensors.PacketResampler(2, "cuda", mode="hold", delay=delay, depth=8)
        live, flags, _ = _drive(rs, seqs, ticks)
        off, off_flags = sensors.resample_sequences([p for p, _ in seqs], [s for _, s in seqs], mode="hold", delay=delay,
                                                    t_start=float(ticks[0]), host=True)
        for s, (pk, st) in enumerate(seqs):
            idx = ro.newest_not_after(pk, st, ticks - delay)
            assert (idx >= 0).all() and len(set(idx.tolist())) > K // 2
            assert np.array_equal(_bits(live[:, s]), _bits(pk[idx])) and (flags[:, s] == ro.F_HELD).all(), (delay, s)
            assert np.array_equal(_bits(off[s][:K]), _bits(pk[idx])) and (off_flags[s][:K] == ro.F_HELD).all(), (delay, s)


# ---- (e) on the grid -----------------------------------------------------------------------------------------------------------------------
def test_a_wearer_on_the_grid_gets_its_own_packets_back():
    """A 60 Hz wearer whose stamps ARE the ticks, in slerp mode with delay 0: its own packets, bit for bit, flag 1 — live (beside a
    100 Hz wearer) and through resample_sequences."""
    rng = np.random.RandomState(47)
    K = 30
    ticks = sensors.tick_times(12.5, K)
    on_grid = (ro.motion_packets(rng, K), ticks.copy())
    other = _wearers(rng, (100.0,), 0.6, 12.5)[0]
    rs = sensors.PacketResampler(2, "cuda", mode="slerp", delay=0.0, max_hold=0.05)
    live, flags, _ = _drive(rs, [on_grid, other], ticks)
    assert np.array_equal(_bits(live[:, 0]), _bits(on_grid[0])) and (flags[:, 0] == ro.F_HELD).all()
    off, off_flags = sensors.resample_sequences([on_grid[0]], [on_grid[1]], mode="slerp", delay=0.0, max_hold=0.05, t_start=12.5, host=True)
    assert off[0].shape == (K, 42) and np.array_equal(_bits(off[0]), _bits(on_grid[0])) and (off_flags[0] == ro.F_HELD).all()


# ---- (f) epoch-sized stamps ----------------------------------------------------------------------------------------------------------------
def test_epoch_sized_stamps():
    """Stamps of 1.7e9 s + ...: the flags equal the oracle's and the values hold the bound.  At that size a float32 stamp resolves
    128 s; in fp64 u = (tau - s_i) / (s_(i+1) - s_i) is the same number on the device and in numpy."""
    rng = np.random.RandomState(53)
    t0 = 1.7e9 + 0.123
    seqs = _wearers(rng, (100.0, 120.0), 0.5, t0)
    off, off_flags = sensors.resample_sequences([p for p, _ in seqs], [s for _, s in seqs], 60.0, mode="slerp", delay=0.015, max_hold=0.05,
                                                host=True)
    ticks = [sensors.sequence_ticks(s, 60.0, 0.015) for _, s in seqs]
    assert [len(o) for o in off] == [len(t) for t in ticks] and min(len(t) for t in ticks) >= 25
    ref32, ref64, flags = _oracle(seqs, ticks, 0.015, 0.05, ro.SLERP, 8)
    assert (flags == ro.F_INTERP).sum() >= 40
    _hold_to_oracle(np.concatenate(off), np.concatenate(off_flags), ref32, ref64, flags, "epoch")


def test_epoch_sized_stamps_given_as_python_lists():
    """Stamps and query times as Python lists of floats, at 1.7e9 s: torch reads such a list as float32, in which every stamp here is
    the same number, so that every packet after a slot's first would be dropped as a duplicate and the query would be up to 128 s off.
    Flags, counts and rows equal the oracle's and what the same values give as numpy float64; a 0-d array and a 0-d tensor are a
    number; float32 times and a CUDA float64 [n] tensor that cannot be read where it lies are refused, and launch nothing."""
    rng = np.random.RandomState(83)
    t0 = 1.7e9 + 0.123
    seqs = _wearers(rng, (100.0, 120.0), 0.2, t0)
    K = 8
    ticks = sensors.tick_times(t0 + 0.05, K)
    a = sensors.PacketResampler(2, "cuda", delay=0.015, max_hold=0.05)
    b = sensors.PacketResampler(2, "cuda", delay=0.015, max_hold=0.05)
    ref = ro.Rings(2, 8)
    at = [0, 0]
    for k, t in enumerate(ticks):
        for s, (pk, st) in enumerate(seqs):
            new = int(np.searchsorted(st, t, side="right"))
            if new > at[s]:
                a.push(pk[at[s]:new].tolist(), [s] * (new - at[s]), [float(v) for v in st[at[s]:new]])
                b.push(pk[at[s]:new], np.full(new - at[s], s), st[at[s]:new])
                ref.push(pk[at[s]:new], [s] * (new - at[s]), st[at[s]:new])
            at[s] = new
        how = k % 4
        ta = [float(t), float(t)] if how == 0 else (float(t) if how == 1 else (np.array(t) if how == 2 else torch.tensor(float(t), dtype=torch.float64)))
        ra, fa = a.emit(ta).cpu().numpy(), a.flags.cpu().numpy()
        rb, fb = b.emit(np.full(2, t)).cpu().numpy(), b.flags.cpu().numpy()
        want, wf = ref.emit(t, 0.015, 0.05, ro.SLERP)
        assert np.array_equal(fa, wf) and np.array_equal(fb, wf), (k, fa, fb, wf)
        assert np.array_equal(_bits(ra), _bits(rb)), k
        assert (wf == ro.F_INTERP).all() and np.abs(ra - want).max() < 1e-4, k
    for got in (a.counts(), b.counts()):
        assert [c.cpu().tolist() for c in got] == [list(c) for c in ref.counts()]
    assert [int(v) for v in a.counts()[1]] == [0, 0] and min(int(v) for v in a.counts()[2]) > 8
    before, flags = a.state.clone(), a.flags.clone()
    pk = seqs[0][0][:2]
    for bad in (torch.tensor([t0 + 9.0, t0 + 9.01], dtype=torch.float32), np.array([t0 + 9.0, t0 + 9.01], dtype=np.float32),
                torch.tensor([t0 + 9.0, t0 + 9.01], dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError, match="push: times are float64 seconds"):
            a.push(pk, [0, 1], bad)
        with pytest.raises(ValueError, match="emit: t are float64 seconds"):
            a.emit(bad)
    strided = torch.zeros((2, 2), dtype=torch.float64, device="cuda")[:, 0]
    with pytest.raises(ValueError, match="read where it lies"):
        a.emit(strided)
    assert torch.equal(a.state, before) and torch.equal(a.flags, flags)
    lies = torch.full((2,), float(ticks[-1]), dtype=torch.float64, device="cuda")
    assert np.array_equal(_bits(a.emit(lies)), _bits(ra))
    torch.cuda.synchronize()


# ---- (g) reset, and lists that name no slot ------------------------------------------------------------------------------------------------
def test_reset_of_one_slot_leaves_the_others():
    rng = np.random.RandomState(59)
    t0 = 1.0
    seqs = _wearers(rng, (100.0, 100.0, 120.0), 0.6, t0)
    ticks = sensors.tick_times(t0 + 0.03, 30)
    a = sensors.PacketResampler(3, "cuda", delay=0.015, depth=4)
    b = sensors.PacketResampler(3, "cuda", delay=0.015, depth=4)
    _drive(a, seqs, ticks[:15])
    _drive(b, seqs, ticks[:15])
    block = a.state.numel() // 3
    before = a.state.clone()
    a.reset([1])
    after = a.state.clone()
    assert torch.equal(after[:block], before[:block]) and torch.equal(after[2 * block:], before[2 * block:])
    assert not torch.equal(after[block: 2 * block], before[block: 2 * block]) and not after[block: 2 * block].any()
    a.emit(float(ticks[14]))
    assert a.flags.cpu().tolist()[1] == ro.F_EMPTY and [int(c[1]) for c in a.counts()] == [0, 0, 0]
    assert [int(c[0]) for c in a.counts()] == [int(c[0]) for c in b.counts()]
    # from here slot 1 sees only what arrives after its reset; the others go on as in the twin that was never reset
    later = [(p[np.searchsorted(s, ticks[14], side="right"):], s[np.searchsorted(s, ticks[14], side="right"):]) for p, s in seqs]
    rows_a, flags_a, _ = _drive(a, later, ticks[15:])
    rows_b, flags_b, _ = _drive(b, later, ticks[15:])
    assert np.array_equal(_bits(rows_a[:, [0, 2]]), _bits(rows_b[:, [0, 2]])) and np.array_equal(flags_a[:, [0, 2]], flags_b[:, [0, 2]])
    alone, alone_flags = ro.rows(later[1][0], later[1][1], ticks[15:], 0.015, None, ro.SLERP, 4)
    assert np.array_equal(flags_a[:, 1], alone_flags) and (alone_flags == ro.F_INTERP).sum() >= 5
    assert not np.array_equal(flags_a[:, 1], flags_b[:, 1])


def test_lists_that_name_no_slot_are_harmless():
    """Through the C ABI: arrivals, reset and get entries for slots outside [0, n) are skipped, and nothing around the state buffer, the
    emitted rows or the counts is written."""
    lib, st = tlib.load(), torch.cuda.current_stream().cuda_stream
    n, depth = 3, 2
    nb = ctypes.c_size_t()
    assert lib.tip_resample_state_bytes(n, depth, ctypes.byref(nb)) == 0
    block = nb.value // n
    buf = torch.full(((n + 2) * block,), 0xCD, dtype=torch.uint8, device="cuda")
    state = buf.data_ptr() + block
    rng = np.random.RandomState(61)
    pk = torch.tensor(ro.motion_packets(rng, 6)).cuda()
    slots = torch.tensor([0, n, -1, 1 << 30, 0, 2], dtype=torch.int32, device="cuda")
    times = torch.tensor([1.0, 1.0, 1.0, 1.0, 2.0, float("nan")], dtype=torch.float64, device="cuda")
    assert lib.tip_resample_reset(state, n, depth, None, 0, st) == 0
    assert lib.tip_resample_push(state, n, depth, pk.data_ptr(), slots.data_ptr(), times.data_ptr(), 6, st) == 0
    assert lib.tip_resample_reset(state, n, depth, slots[1:4].data_ptr(), 3, st) == 0
    counts = torch.full((8, 3), 5, dtype=torch.int32, device="cuda")
    assert lib.tip_resample_get(state, n, depth, slots.data_ptr(), 6, counts[1:].data_ptr(), st) == 0
    t = torch.full((n,), 1.5, dtype=torch.float64, device="cuda")
    out = torch.full((n + 2, 42), 7.0, device="cuda")
    flags = torch.full((n + 2,), 9, dtype=torch.uint8, device="cuda")
    assert lib.tip_resample_emit(state, n, depth, t.data_ptr(), 0.0, -1.0, 1, out[1:].data_ptr(), flags[1:].data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert (buf[:block] == 0xCD).all() and (buf[-block:] == 0xCD).all()
    assert counts.cpu().tolist() == [[5] * 3, [2, 0, 2], [5] * 3, [5] * 3, [5] * 3, [2, 0, 2], [0, 1, 0], [5] * 3]
    assert flags.cpu().tolist() == [9, ro.F_INTERP, ro.F_EMPTY, ro.F_EMPTY, 9]
    o = out.cpu().numpy()
    assert (o[0] == 7.0).all() and (o[-1] == 7.0).all() and np.isnan(o[2:4]).all() and np.isfinite(o[1]).all()
    want = ro.interp(pk[0].cpu().numpy().reshape(6, 7), pk[4].cpu().numpy().reshape(6, 7), 0.5, f32).reshape(42)
    assert np.abs(o[1] - want).max() < 1e-4                       # (the right two packets, half way: the bounds are the tests' above)


def test_push_and_emit_refusals_launch_nothing():
    rs = sensors.PacketResampler(3, "cuda")
    before = rs.state.clone()
    pk = np.zeros((4, 42), f32)
    for args in ((pk, [0, 1, 2], [0.0] * 4), (pk[:, :41], [0] * 4, [0.0] * 4), (pk, [0] * 4, [0.0] * 3), (pk.reshape(-1), [0] * 4, [0.0] * 4)):
        with pytest.raises(ValueError, match=r"push: packets is \[m, 42\]"):
            rs.push(*args)
    with pytest.raises(ValueError, match="push: slots are integers"):
        rs.push(pk, [0.0] * 4, [0.0] * 4)
    for t in ([0.0, 1.0], np.zeros((3, 1)), torch.zeros(4, dtype=torch.float64, device="cuda")):
        with pytest.raises(ValueError, match=r"emit: t is a number or \[3\]"):
            rs.emit(t)
    with pytest.raises(ValueError, match="emit: out is a contiguous float32"):
        rs.emit(0.0, out=torch.empty((3, 41), device="cuda"))
    with pytest.raises(ValueError, match="slot index outside"):
        rs.reset([3])
    rs.push(pk[:0], [], [])                                      # nothing arrived: no launch, no error
    assert torch.equal(rs.state, before) and not rs.state.any()
    out = torch.full((3, 42), 7.0, device="cuda")
    t = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64, device="cuda")
    assert rs.emit(t, out=out) is out and torch.isnan(out).all() and rs.flags.cpu().tolist() == [ro.F_EMPTY] * 3
    torch.cuda.synchronize()


# ---- (h) in front of the engines -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,use_graph", [(8, False), (8, True), (50, True)])
def test_step_packets_of_the_emitted_rows(paper, frames, use_graph):
    """StreamingEngine at n = 2 (a 100 Hz and a 120 Hz wearer): step_packets(front, rs.emit(t)) — the emitted CUDA tensor handed on as
    it is — equals, bit for bit, step_packets in a twin engine on the same rows uploaded from numpy, launch by launch and with
    use_graph=True (at 50 frames the captured frame replays from frame 44 on)."""
    m, _ = paper
    rng = np.random.RandomState(67)
    n, t0 = 2, 20.0
    seqs = _wearers(rng, (100.0, 120.0), frames / 60.0 + 0.1, t0)
    ticks = sensors.tick_times(t0 + 0.04, frames)
    rows, flags = sensors.resample_sequences([p for p, _ in seqs], [s for _, s in seqs], delay=0.012, max_hold=0.1, t_start=float(ticks[0]),
                                             host=True)
    assert all(len(r) >= frames and (f[:frames] <= ro.F_HELD).all() for r, f in zip(rows, flags))
    _, tables = so.case(n, 71)
    fr = sensors.SensorFrontEnd(n, "cuda")
    fr.load(range(n), tables)
    s0 = np.stack([synth.make_recording(2, seed=310 + i)[1] for i in range(n)])
    Engine = tip_amd.streaming.StreamingEngine
    a, b = Engine(m, s0, use_graph=use_graph), Engine(m, s0, use_graph=use_graph)
    rs = sensors.PacketResampler(n, "cuda", delay=0.012, max_hold=0.1)
    at, produced = [0] * n, 0
    for k, t in enumerate(ticks):
        for s, (pk, st) in enumerate(seqs):
            new = int(np.searchsorted(st, t, side="right"))
            rs.push(pk[at[s]:new], [s] * (new - at[s]), st[at[s]:new])
            at[s] = new
        oa = a.step_packets(fr, rs.emit(float(t)))
        oa = None if oa is None else {key: oa[key].clone() for key in ("s_rest", "c_t", "y_last")}
        ob = b.step_packets(fr, np.stack([rows[s][k] for s in range(n)]))
        assert (oa is None) == (ob is None), k
        if oa is not None:
            for key in oa:
                assert torch.equal(oa[key].view(torch.int32), ob[key].view(torch.int32)), (k, key)
            produced += bool(torch.isfinite(oa["y_last"]).all())
    assert produced == frames - 5 and a.captures == b.captures == (1 if use_graph and frames > 44 else 0) and a.frame == b.frame == frames
    torch.cuda.synchronize()


# ---- (i) recorded sessions -----------------------------------------------------------------------------------------------------------------
def test_recorded_sessions_equal_the_live_front_end():
    """resample_sequences -> transform_sequences equals, row for row and bit for bit, the live emit -> front.transform; the rows are
    finite from the first tick on and in the frame format ReplayPool.run takes."""
    rng = np.random.RandomState(73)
    n, t0, K = 2, 5.0, 24
    seqs = _wearers(rng, (100.0, 50.0), 0.6, t0)
    ticks = sensors.tick_times(t0 + 0.05, K)
    _, tables = so.case(n, 79)
    packets, flags = sensors.resample_sequences([p for p, _ in seqs], [s for _, s in seqs], delay=0.025, max_hold=0.1, t_start=float(ticks[0]))
    frames = sensors.transform_sequences([p[:K] for p in packets], tables, host=True)
    fr = sensors.SensorFrontEnd(n, "cuda")
    fr.load(range(n), tables)
    rs = sensors.PacketResampler(n, "cuda", delay=0.025, max_hold=0.1)
    at = [0] * n
    for k, t in enumerate(ticks):
        for s, (pk, st) in enumerate(seqs):
            new = int(np.searchsorted(st, t, side="right"))
            rs.push(pk[at[s]:new], [s] * (new - at[s]), st[at[s]:new])
            at[s] = new
        live = fr.transform(rs.emit(float(t))).cpu().numpy()
        for s in range(n):
            assert np.array_equal(_bits(live[s]), _bits(frames[s][k])), (k, s)
            assert int(rs.flags[s]) == int(flags[s][k])
    assert all(f.shape == (K, 72) and f.dtype == f32 and np.isfinite(f).all() for f in frames)
    assert all((fl[:K].cpu().numpy() == ro.F_INTERP).sum() >= K // 2 for fl in flags)
