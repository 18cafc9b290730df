"""Clock sync and predicted ticks without a GPU: the C-ABI surface of tip_clock_* / tip_predict_* and its refusals before any launch,
every refusal of the Python layer, and the properties of the oracle (tests/sync_oracle.py) that make the GPU tests' comparisons with it
mean something — the clock rule on a drifting hub behind a jittery network, prediction on constant angular rates against the analytic
orientation, and max_predict = 0 against the existing slerp oracle.

No fixture from the reference is needed: the reference keeps no stamps (live_demo_new.py:82-115)."""
import ctypes
import os
import re

import numpy as np
import pytest

import resample_oracle as ro
import sync_oracle as sy
from tip_amd import lib as tlib
from tip_amd import sensors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"tip_clock_state_bytes": 2, "tip_clock_reset": 5, "tip_clock_get": 7, "tip_clock_map": 10, "tip_clock_push": 13,
         "tip_clock_rows": 9, "tip_predict_emit": 10, "tip_predict_rows": 15}      # name: number of arguments
f32 = np.float32
NAN, INF = float("nan"), float("inf")


def _each(fn, ok, nulls, bad):
    INV = -1
    assert all(not isinstance(v, float) or np.isfinite(v) for v in ok)
    for i in nulls:
        a = list(ok)
        a[i] = None
        assert fn(*a) == INV, ("null", i)
    for i, v in bad:
        a = list(ok)
        a[i] = v
        assert fn(*a) == INV, (i, v)


def test_c_abi_surface_and_refusals_before_any_launch():
    """Every new name is declared in the header's section, exported and bound with the declared number of arguments; the ABI is still
    5; the constants agree between the header, lib.py, sensors.py and the oracle; every refusal returns before a launch (this machine
    has no GPU to launch on), and m = 0, n = 0, count = 0, n_in = 0, n_out = 0 return 0."""
    hdr = open(os.path.join(ROOT, "include", "tip_hip.h")).read()
    section = hdr[hdr.index("/* ---- clock sync and predicted ticks"):hdr.index("/* ---- kinematics:")]
    assert set(re.findall(r"TIP_API int (tip_\w+)\(", section)) == set(NAMES) == {n for n in tlib.EXPORTS if n.startswith(("tip_clock_", "tip_predict_"))}
    assert int(re.search(r"#define TIP_ABI_VERSION (\d+)", hdr).group(1)) == 5 and tlib.TIP_ABI_VERSION == 5
    consts = {k: float(v) for k, v in re.findall(r"#define (TIP_CLOCK_LEAK|TIP_CLOCK_SLEW|TIP_PREDICT_SPAN|TIP_RESAMPLE_PREDICTED)\s+(\S+)", hdr)}
    assert consts == {"TIP_CLOCK_LEAK": tlib.TIP_CLOCK_LEAK, "TIP_CLOCK_SLEW": tlib.TIP_CLOCK_SLEW, "TIP_PREDICT_SPAN": tlib.TIP_PREDICT_SPAN,
                      "TIP_RESAMPLE_PREDICTED": tlib.TIP_RESAMPLE_PREDICTED}
    assert (sy.LEAK, sy.SLEW, sy.PREDICT_SPAN, sy.F_PREDICT) == (2e-4, 0.5, 2.0, 5) == tuple(consts[k] for k in
                                                                                          ("TIP_CLOCK_LEAK", "TIP_CLOCK_SLEW", "TIP_PREDICT_SPAN", "TIP_RESAMPLE_PREDICTED"))
    assert sensors.MODES == {"hold": 0, "slerp": 1, "predict": 2} and sensors.PREDICTED == 5
    assert (sensors.INTERPOLATED, sensors.HELD, sensors.STALE, sensors.EMPTY, sensors.EARLY) == (0, 1, 2, 3, 4)
    raw = ctypes.CDLL(tlib.LIB_PATH)
    lib = tlib.load()
    for name, nargs in NAMES.items():
        m = re.search(r"TIP_API int " + name + r"\((.*?)\);", hdr, re.S)
        assert len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")) == nargs, name
        assert hasattr(raw, name) and len(getattr(lib, name).argtypes) == nargs and getattr(lib, name).restype is lib.tip_forward.restype, name
    srcs = re.search(r"^SRCS = (.*)$", open(os.path.join(tlib.CSRC, "Makefile")).read(), re.M).group(1).split()
    assert "tip_clock.hip" in srcs and "-ffp-contract=off" in open(os.path.join(tlib.CSRC, "Makefile")).read()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)        # a non-null, 8-byte aligned pointer: every call below returns before it would launch
    INV = -1
    # the resampler's state keeps its size, the clock's is 32 bytes per slot beside it
    n = ctypes.c_size_t()
    assert lib.tip_resample_state_bytes(3, 8, ctypes.byref(n)) == 0 and n.value == 3 * (16 + 176 * 8)
    assert lib.tip_clock_state_bytes(3, ctypes.byref(n)) == 0 and n.value == 96
    assert lib.tip_clock_state_bytes(0, ctypes.byref(n)) == 0 and n.value == 0
    assert lib.tip_clock_state_bytes(-1, ctypes.byref(n)) == INV and lib.tip_clock_state_bytes(3, None) == INV
    # tip_clock_reset(state, n, slots | null, count, stream)
    assert lib.tip_clock_reset(None, 4, None, 0, None) == INV and lib.tip_clock_reset(p + 4, 4, None, 0, None) == INV
    assert lib.tip_clock_reset(p, -1, None, 0, None) == INV and lib.tip_clock_reset(p, 4, p, -1, None) == INV
    assert lib.tip_clock_reset(p, 0, None, 0, None) == 0 and lib.tip_clock_reset(p, 4, p, 0, None) == 0
    # tip_clock_get(state, n, slots, count, theta_out, counts_out, stream)
    _each(lib.tip_clock_get, [p, 4, p, 1, p, p, None], (0, 2, 4, 5), ((0, p + 4), (1, -1), (3, -1)))
    assert lib.tip_clock_get(p, 4, None, 0, None, None, None) == 0 and lib.tip_clock_get(p, 0, p, 1, p, p, None) == 0
    rule = lambda i, j: ((i, NAN), (i, -1e-6), (i, INF), (i, -INF), (j, NAN), (j, 1.0), (j, 1.5), (j, -0.1), (j, INF))   # noqa: E731
    # tip_clock_map(state, n, slots, stamps, arrivals, m, leak, slew, times_out, stream)
    _each(lib.tip_clock_map, [p, 4, p, p, p, 2, 2e-4, 0.5, p, None], (0, 2, 3, 4, 8), ((0, p + 4), (1, -1), (5, -1)) + rule(6, 7))
    assert lib.tip_clock_map(p, 4, None, None, None, 0, 2e-4, 0.5, None, None) == 0 and lib.tip_clock_map(p, 0, p, p, p, 2, 0.0, 0.0, p, None) == 0
    # tip_clock_push(resample_state, clock_state, n, depth, packets, slots, stamps, arrivals, m, leak, slew, times_out | null, stream)
    _each(lib.tip_clock_push, [p, p, 4, 8, p, p, p, p, 2, 2e-4, 0.5, None, None], (0, 1, 4, 5, 6, 7),
          ((0, p + 4), (1, p + 4), (2, -1), (3, 1), (3, 65), (3, 0), (8, -1)) + rule(9, 10))
    assert lib.tip_clock_push(p, p, 4, 8, None, None, None, None, 0, 2e-4, 0.5, None, None) == 0
    assert lib.tip_clock_push(p, p, 0, 8, p, p, p, p, 2, 2e-4, 0.5, p, None) == 0
    # tip_clock_rows(stamps, arrivals, offsets, n_in, n_seq, leak, slew, times_out, stream)
    _each(lib.tip_clock_rows, [p, p, p, 4, 2, 2e-4, 0.5, p, None], (0, 1, 2, 7), ((3, -1), (4, -1)) + rule(5, 6))
    assert lib.tip_clock_rows(None, None, p, 0, 2, 2e-4, 0.5, None, None) == 0 and lib.tip_clock_rows(p, p, p, 4, 0, 2e-4, 0.5, p, None) == 0
    # tip_predict_emit(state, n, depth, t, delay, max_hold, max_predict, packets_out, flags, stream)
    _each(lib.tip_predict_emit, [p, 4, 8, p, 0.0, -1.0, 0.025, p, p, None], (0, 3, 7, 8),
          ((0, p + 4), (1, -1), (2, 0), (2, 65), (4, -0.01), (4, NAN), (4, INF), (5, NAN), (6, NAN), (6, -0.001), (6, INF)))
    assert lib.tip_predict_emit(p, 0, 8, p, 0.0, 0.5, 0.0, p, p, None) == 0
    # tip_predict_rows(packets, stamps, in_offsets, n_in, t_out, out_offsets, n_out, n_seq, delay, max_hold, max_predict, depth, out, flags, stream)
    ok = [p, p, p, 4, p, p, 3, 1, 0.0, -1.0, 0.025, 8, p, p, None]
    _each(lib.tip_predict_rows, ok, (0, 1, 2, 4, 5, 12, 13),
          ((3, -1), (6, -1), (7, -1), (8, -1.0), (8, INF), (9, NAN), (10, NAN), (10, -1.0), (10, INF), (11, 1), (11, 65)))
    ok[6] = 0
    assert lib.tip_predict_rows(*ok) == 0
    # the two old entries still refuse what they refused: prediction is not a mode of theirs
    assert lib.tip_resample_emit(p, 4, 8, p, 0.01, -1.0, 2, p, p, None) == INV


def test_python_refusals_before_any_launch():
    """Every argument check of ClockSync, PacketResampler(mode="predict"), push(arrivals=, sync=) and sync_sequences comes before a
    device is chosen: on a machine without a GPU each is a ValueError in the caller's name."""
    C, P = sensors.ClockSync, sensors.PacketResampler
    for kw, what in (({"leak": -1e-6}, "leak is"), ({"leak": NAN}, "leak is"), ({"leak": INF}, "leak is"), ({"leak": "x"}, "leak is"),
                     ({"slew": 1.0}, "slew is"), ({"slew": -0.1}, "slew is"), ({"slew": NAN}, "slew is")):
        with pytest.raises(ValueError, match="ClockSync: " + what):
            C(2, "cpu", **kw)
    for n in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="n is the number of slots"):
            C(n, "cpu")
    with pytest.raises(RuntimeError, match="runs on an MI355X"):
        C(2, "cpu", leak=0.0, slew=0.0)
    for kw, what in (({"mode": "predict", "max_predict": -0.001}, "max_predict is"), ({"mode": "predict", "max_predict": NAN}, "max_predict is"),
                     ({"mode": "predict", "max_predict": INF}, "max_predict is"), ({"mode": "predict", "max_predict": "x"}, "max_predict is"),
                     ({"mode": "slerp", "max_predict": 0.01}, "max_predict is"), ({"mode": "hold", "max_predict": 0.0}, "max_predict is"),
                     ({"mode": "extrapolate"}, "mode is"), ({"mode": 2}, "mode is"), ({"mode": "predict", "delay": -0.01}, "delay is")):
        with pytest.raises(ValueError, match="PacketResampler: " + what):
            P(2, "cpu", **kw)
    for kw in ({"mode": "predict"}, {"mode": "predict", "max_predict": 0.0, "delay": 0.0, "max_hold": 0.1}):
        with pytest.raises(RuntimeError, match="runs on an MI355X"):        # good arguments get as far as asking for the device
            P(2, "cpu", **kw)
    pk, t = np.zeros((5, 42), f32), np.arange(5) * 0.01
    R = sensors.resample_sequences
    for kw, what in (({"mode": "predict", "max_predict": -1.0}, "max_predict is"), ({"mode": "slerp", "max_predict": 0.02}, "max_predict is"),
                     ({"mode": "predict", "max_predict": NAN}, "max_predict is")):
        with pytest.raises(ValueError, match="resample_sequences: " + what):
            R([pk], [t], **kw)
    S = sensors.sync_sequences
    for kw, what in (({"leak": -1.0}, "leak is"), ({"leak": NAN}, "leak is"), ({"slew": 1.0}, "slew is"), ({"slew": NAN}, "slew is")):
        with pytest.raises(ValueError, match="sync_sequences: " + what):
            S([t], [t + 5.0], **kw)
    with pytest.raises(ValueError, match="no sequences"):
        S([], [])
    with pytest.raises(ValueError, match="2 stamp arrays for 1 arrival arrays"):
        S([t, t], [t])
    with pytest.raises(ValueError, match=r"stamps_list\[1\] and arrivals_list\[1\] are \[L\]"):
        S([t, t], [t, t[:4]])
    with pytest.raises(ValueError, match=r"arrivals_list\[0\] are float64 seconds"):
        S([t], [t.astype(f32)])
    with pytest.raises(ValueError, match=r"stamps_list\[0\] are float64 seconds"):
        S([t.astype(f32)], [t])


# ---- the clock rule ----------------------------------------------------------------------------------------------------------------------
ULP = float(np.spacing(1.7e9))        # 2.4e-7 s: what an arrival time, an offset or a mapped time of this size is rounded to


def test_clock_rule_on_a_drifting_hub_behind_a_jittery_network():
    """4000 packets at 100 Hz, a true offset of 1.7e9 s, a drift of +40 ppm, delays of 2 ms + Exp(3 ms).  After the first 200 packets
    mapped - (s + theta_true(s)) stays within [min delay, min delay + 1 ms]; mapped times are strictly increasing; their spacing has less
    than a tenth of the arrival spacing's standard deviation.  Times of 1.7e9 s are multiples of 2.4e-7 s, so the delays are the
    realised ones — arrival - (s + theta_true(s)) as fp64 holds them — and the two ends of the interval get 2 ulp of that size: one
    for the rounding of the mapped time, one for that of the time it is compared with."""
    rng = np.random.RandomState(7)
    s, a, theta, _ = sy.hub(rng, 4000)
    truth = s + theta
    realised = a - truth
    mapped, block = sy.clock_sequence(s, a)
    assert np.isfinite(mapped).all() and block[2:] == [4000, 0]
    err = (mapped - truth)[200:]
    print(f"mapped - truth after 200 packets: {err.min():.6e} .. {err.max():.6e} s; realised delays {realised.min():.6e} .. {realised.max():.6e}; ulp {ULP:.2e}")
    assert err.min() >= realised.min() - 2 * ULP and err.max() <= realised.min() + 1e-3 + 2 * ULP
    assert (np.diff(mapped) > 0).all()
    sd_m, sd_a = float(np.std(np.diff(mapped))), float(np.std(np.diff(a)))
    print(f"spacing: std of mapped {sd_m:.3e} s, of arrivals {sd_a:.3e} s, ratio {sd_m / sd_a:.4f}")
    assert sd_m < 0.1 * sd_a


def test_clock_rule_under_a_delay_spike():
    """The same hub; 300 packets in a row (3 s) arrive 50 ms late.  Against the run without the spike no mapped time moves by more than
    leak x elapsed, elapsed counted from the last packet before the spike, which is chosen where the estimate sits on its measurement
    (the smallest delay of the run: the unspiked estimate cannot come down afterwards, so the whole difference is the spiked one's
    rise).  2 ulp of 1.7e9 s for the two mapped times."""
    rng = np.random.RandomState(7)
    s, a, theta, d = sy.hub(rng, 4000)
    j0 = 300 + int(np.argmin((a - (s + theta))[300:3000])) + 1
    late = a.copy()
    late[j0:j0 + 300] += 0.050
    base, _ = sy.clock_sequence(s, a)
    spiked, _ = sy.clock_sequence(s, late)
    assert np.array_equal(base[:j0], spiked[:j0])
    moved = np.abs(spiked - base)[j0:]
    elapsed = (s - s[j0 - 1])[j0:]
    print(f"spike at packet {j0}: mapped times moved by at most {moved.max():.3e} s ({moved[:300].max():.3e} inside); leak x elapsed there "
          f"{sy.LEAK * elapsed[int(np.argmax(moved))]:.3e}; an unfiltered arrival would have moved 5.0e-02")
    assert moved[:300].max() > 10 * ULP                                # (the spike does reach the estimate ...)
    assert (moved <= sy.LEAK * elapsed + 2 * ULP).all()                # (... and no further than the leak lets it)
    assert (np.diff(spiked) > 0).all()


def test_clock_rule_rejections_and_chunking():
    """Duplicates, out-of-order stamps and non-finite values are rejected and counted without touching the estimate; a first packet
    sets it; the blocks of a pool are independent; feeding in chunks is feeding at once."""
    c = sy.Clocks(2)
    slots = [0, 1, 0, 0, 0, 5, 0, 1, -1, 0]
    st = [1.0, 7.0, 1.01, 1.01, 1.005, 2.0, NAN, 7.01, 3.0, 1.02]
    ar = [101.0, 57.0, 101.012, 101.02, 101.03, 0.0, 101.04, NAN, 0.0, 101.021]
    got = c.map(slots, st, ar)
    assert np.array_equal(np.isnan(got), [False, False, False, True, True, True, True, True, True, False])
    assert got[0] == 101.0 and got[1] == 57.0 and got[2] == 1.01 + (100.0 + 2e-4 * (1.01 - 1.0))       # the rise is the leak's
    assert [list(v) for v in c.counts()] == [[3, 1], [3, 1]] and c.s_prev()[0] == 1.02
    twin = sy.Clocks(2)
    parts = [twin.map(slots[i:j], st[i:j], ar[i:j]) for i, j in ((0, 3), (3, 4), (4, 10))]
    assert np.array_equal(np.concatenate(parts).view(np.int64), got.view(np.int64)) and np.array_equal(twin.image(), c.image())
    assert c.image().shape == (2, 32) and not sy.Clocks(2).image().any()
    seq, block = sy.clock_sequence([1.0, 1.01, 1.02], [101.0, 101.012, 101.021])
    assert np.array_equal(seq, got[[0, 2, 9]]) and block == c.blocks[0][:2] + [3, 0]
    # the fall is the slew's: a packet that arrives much earlier than the envelope pulls it down by half the stamp interval
    down = sy.Clocks(1)
    assert down.map([0, 0], [0.0, 0.01], [10.0, 9.0]).tolist() == [10.0, 0.01 + (10.0 - 0.5 * 0.01)]


# ---- prediction --------------------------------------------------------------------------------------------------------------------------
RATES = (0.1, 0.3, 1.0, 2.0, 4.0, 8.0)


def test_prediction_on_constant_angular_rates():
    """Six sensors turning at 0.1 .. 8 rad/s, stamps at 100 Hz +- 20 % jitter, ticks at 60 Hz with delay 0.  The fp64 oracle's
    predicted orientation equals the analytic orientation AT THE TICK within 1e-12 (rotation matrices, entrywise); the held packet
    differs from it by the rate times the packet's age."""
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(11)
    L = 240
    st = ro.stamps_at(rng, L, 100.0, t0=3.0)
    _, pk, analytic = sy.spin_packets(rng, st, RATES)
    ticks = sensors.tick_times(st[2] + 0.001, 130)
    worst, worst_hold, worst_acc, n_pred = np.zeros(6), 0.0, 0.0, 0
    for t in ticks:
        cnt = int(np.searchsorted(st, t, side="right"))
        f, i, u = sy.decide(st[max(0, cnt - 8):cnt], t, None, 0.05)
        if f != sy.F_PREDICT:
            assert f == sy.F_HELD and t - st[cnt - 1] > 2.0 * (st[cnt - 1] - st[cnt - 2]) or t == st[cnt - 1]
            continue
        n_pred += 1
        assert u > 1.0 and i == min(cnt, 8) - 2
        a, b = pk[cnt - 2].reshape(6, 7), pk[cnt - 1].reshape(6, 7)
        got = sy.predict(a, b, u, np.float64, stored=np.float64)
        want = analytic(t)
        worst = np.maximum(worst, np.abs(Rotation.from_quat(got[:, :4]).as_matrix() - want.as_matrix()).max(axis=(1, 2)))
        assert np.abs(np.linalg.norm(got[:, :4], axis=1) - 1.0).max() <= 1e-15
        assert (np.einsum("ni,ni->n", got[:, :4], a[:, :4]) > 0).all()                                    # the earlier packet's sign
        age = t - st[cnt - 1]
        held = (Rotation.from_quat(b[:, :4]).inv() * want).magnitude()
        worst_hold = max(worst_hold, float(np.abs(held - np.asarray(RATES) * age).max()))
        # the acceleration is the newer packet's, turned from its frame into the predicted one
        g = Rotation.from_quat(b[:, :4]).apply(b[:, 4:])
        worst_acc = max(worst_acc, float((np.abs(got[:, 4:] - want.inv().apply(g)).max(axis=1) / np.maximum(1.0, np.linalg.norm(g, axis=1))).max()))
    print(f"{n_pred} predicted ticks of {len(ticks)}; |R_predicted - R_analytic| per rate {dict(zip(RATES, worst))}; "
          f"| angle(hold, analytic) - rate x age | {worst_hold:.3e}; | a - R_analytic^T g | / max(1, |g|) {worst_acc:.3e}")
    assert n_pred >= 100
    assert worst_hold <= 1e-12
    assert worst.max() <= 1e-12


def test_predicted_sensor_nan_rules_and_float32():
    """A zero or non-finite quaternion in either packet: seven NaN; a NaN in the newer packet's acceleration: three; a NaN in the older
    packet's acceleration does not reach the row.  The float32 evaluation is within fp32 noise of the fp64 one."""
    rng = np.random.RandomState(13)
    st = ro.stamps_at(rng, 40, 100.0)
    pk, _, _ = sy.spin_packets(rng, st, RATES)
    a, b = pk[:-1].reshape(-1, 7).copy(), pk[1:].reshape(-1, 7).copy()
    u = rng.uniform(1.0, 3.0, size=len(a))
    lo, hi = sy.predict(a, b, u, f32), sy.predict(a, b, u, np.float64)
    assert lo.dtype == f32 and np.isfinite(lo).all()
    dR = np.abs(ro.rotations(lo.reshape(-1, 42)) - ro.rotations(hi.reshape(-1, 42))).max()
    print(f"fp32 - fp64 over u in 1 .. 3: rotation entries {dR:.3e}, accelerations {np.abs(lo[:, 4:] - hi[:, 4:]).max():.3e}")
    assert dR < 5e-6 and np.abs(lo[:, 4:] - hi[:, 4:]).max() < 5e-5
    a[0, :4] = 0.0
    b[1, 2] = np.nan
    a[2, 0] = np.inf
    a[3, 5] = np.nan
    b[4, 6] = np.nan
    for dtype in (f32, np.float64):
        got = sy.predict(a[:8], b[:8], u[:8], dtype)
        assert np.isnan(got[:3]).all() and np.isfinite(got[5:]).all() and np.isfinite(got[3]).all()
        assert np.isfinite(got[4, :4]).all() and np.isnan(got[4, 4:]).all()
        assert np.array_equal(got[3], sy.predict(pk[:-1].reshape(-1, 7)[3], b[3], u[3], dtype))           # the older acceleration is not read


def test_predict_decision_table():
    s = [1.0, 2.0, 2.5, 3.0]
    D = sy.decide
    assert D([], 3.0, None, 0.1)[0] == sy.F_EMPTY and D([1.0], 1.2, None, 1.0) == (sy.F_HELD, 0, 0.0)
    assert D(s, 0.5, None, 1.0)[0] == sy.F_EARLY and D(s, NAN, None, 1.0)[0] == sy.F_EARLY
    assert D(s, 2.25, None, 1.0) == (sy.F_INTERP, 1, 0.5) and D(s, 3.0, None, 1.0) == (sy.F_HELD, 3, 0.0)       # tau == s_last: held
    assert D(s, 3.25, None, 1.0) == (sy.F_PREDICT, 2, 1.5) and D(s, 4.0, None, 1.0) == (sy.F_PREDICT, 2, 3.0)   # h == 2 b is predicted
    assert D(s, 4.01, None, 1.0) == (sy.F_HELD, 3, 0.0) and D(s, 4.01, 1.0, 1.0)[0] == sy.F_STALE               # past twice the bracket
    assert D(s, 3.25, None, 0.2) == (sy.F_HELD, 3, 0.0) and D(s, 3.25, None, 0.25)[0] == sy.F_PREDICT           # max_predict
    assert D(s, 3.25, 0.4, 1.0) == (sy.F_HELD, 3, 0.0) and D(s, 3.25, 0.5, 1.0)[0] == sy.F_PREDICT              # a bracket longer than max_hold
    assert D(s, 3.25, 0.2, 1.0)[0] == sy.F_STALE and D(s, 3.25, None, 0.0) == (sy.F_HELD, 3, 0.0)


def test_max_predict_zero_is_the_slerp_oracle_bit_for_bit():
    rng = np.random.RandomState(17)
    L = 80
    pk, st = ro.motion_packets(rng, L), ro.stamps_at(rng, L, 100.0, t0=10.0)
    ticks = sensors.tick_times(9.99, 60)
    for delay, hold, any_predicted in ((0.0, None, True), (0.012, None, False), (0.004, 0.011, True), (0.0, 0.004, False)):
        got, flags = sy.rows(pk, st, ticks, delay, hold, 0.0, depth=4)
        want, want_flags = ro.rows(pk, st, ticks, delay, hold, ro.SLERP, depth=4)
        assert np.array_equal(flags, want_flags) and np.array_equal(got.view(np.int32), want.view(np.int32)), (delay, hold)
        some, some_flags = sy.rows(pk, st, ticks, delay, hold, 0.025, depth=4)
        pred = some_flags == sy.F_PREDICT
        assert np.array_equal(some_flags[~pred], want_flags[~pred]) and np.array_equal(some[~pred].view(np.int32), want[~pred].view(np.int32))
        assert (want_flags[pred] != ro.F_INTERP).all() and (pred.sum() > 10) == any_predicted, (delay, hold, int(pred.sum()))   # (a delay of a period, a max_hold below every bracket: none)


def test_oracle_rows_is_the_live_ring_at_every_tick():
    """The oracle's offline form against its live form in predict mode, depth 4, a wrap; the ring image has the device's layout."""
    rng = np.random.RandomState(19)
    L = 60
    pk, st = ro.motion_packets(rng, L), ro.stamps_at(rng, L, 100.0, t0=10.0)
    ticks = sensors.tick_times(10.005, 30)
    off, off_f = sy.rows(pk, st, ticks, 0.0, 0.05, 0.02, depth=4)
    r, at = sy.Rings(1, 4), 0
    for k, t in enumerate(ticks):
        new = int(np.searchsorted(st, t, side="right"))
        r.push(pk[at:new], [0] * (new - at), st[at:new])
        at = new
        row, f = r.emit(t, 0.0, 0.05, 0.02)
        assert f[0] == off_f[k] and np.array_equal(row[0].view(np.int32), off[k].view(np.int32)), k
    assert (off_f == sy.F_PREDICT).sum() >= 20
    img = r.image()
    assert img.shape == (1, 16 + 176 * 4) and img[0, :16].view(np.int32).tolist() == [at % 4, 4, at, 0]
    assert sorted(img[0, 16:48].view(np.float64).tolist()) == r.stamps[0]
