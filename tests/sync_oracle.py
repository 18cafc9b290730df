"""Oracle of clock sync and predicted ticks (csrc/tip_clock.hip; tip_amd.sensors.ClockSync, PacketResampler(mode="predict"),
sync_sequences): the rules of include/tip_hip.h ("clock sync and predicted ticks") in numpy, value by value.

    clock_step      the clock rule on one (stamp, arrival): Python floats, i.e. fp64, the header's statements in the header's order — no
                    statement is fused on the device (-ffp-contract=off), so the device gives the same bits
    Clocks          n blocks (theta, s_prev, count, rejected): map in array order
    clock_sequence  a recorded sequence from a reset block
    decide          the predict decision in front of resample_oracle.decide (mode SLERP): Python floats again
    predict         one sensor past the newer of two packets, vectorised, in fp64 or in any dtype; the float32 evaluation follows the
                    kernel's statement order and is what the GPU tests take their fp32 noise from
    Rings, rows     resample_oracle's with the predict rule

The reference keeps no stamps (live_demo_new.py:82-115): nothing of it is restated here.
"""
import numpy as np

import resample_oracle as ro
from resample_oracle import F_INTERP, F_HELD, F_STALE, F_EMPTY, F_EARLY, PACKET, SLERP  # noqa: F401

F_PREDICT = 5
PREDICT_SPAN = 2.0
TINY_ARC = 1e-5                       # below this arc between the two quaternions the weights are 1 - u and u
LEAK, SLEW = 2e-4, 0.5
NAN = float("nan")


# ---- the clock -------------------------------------------------------------------------------------------------------------------------
def clock_step(block, s, a, leak=LEAK, slew=SLEW):
    """block: [theta, s_prev, count, rejected], changed in place -> mapped (NaN: rejected)."""
    s, a = float(s), float(a)
    theta, s_prev, count, rejected = block
    if not np.isfinite(s) or not np.isfinite(a) or (count > 0 and s <= s_prev):
        block[3] = rejected + 1
        return NAN
    o = a - s
    if count == 0:
        theta = o
    else:
        d = s - s_prev
        up = theta + leak * d
        dn = theta - slew * d
        th = o if o < up else up
        theta = th if th > dn else dn
    block[0], block[1], block[2] = theta, s, count + 1
    return s + theta


class Clocks:
    """tip_clock_map / tip_clock_get / tip_clock_reset on n slots."""

    def __init__(self, n, leak=LEAK, slew=SLEW):
        self.n, self.leak, self.slew = int(n), float(leak), float(slew)
        self.blocks = [[0.0, 0.0, 0, 0] for _ in range(self.n)]

    def reset(self, slots=None):
        for s in range(self.n) if slots is None else slots:
            if 0 <= s < self.n:
                self.blocks[s] = [0.0, 0.0, 0, 0]

    def map(self, slots, stamps, arrivals):
        """-> mapped [m] float64; an arrival for a slot outside [0, n) is not mapped: NaN here (the device writes nothing there)."""
        out = np.full(len(slots), np.nan, dtype=np.float64)
        for j, (sl, s, a) in enumerate(zip(np.asarray(slots).reshape(-1), np.asarray(stamps, dtype=np.float64), np.asarray(arrivals, dtype=np.float64))):
            if 0 <= int(sl) < self.n:
                out[j] = clock_step(self.blocks[int(sl)], s, a, self.leak, self.slew)
        return out

    def theta(self):
        return np.array([b[0] for b in self.blocks], dtype=np.float64)

    def s_prev(self):
        return np.array([b[1] for b in self.blocks], dtype=np.float64)

    def counts(self):
        """count, rejected [n]."""
        return np.array([b[2] for b in self.blocks]), np.array([b[3] for b in self.blocks])

    def image(self):
        """The blocks as the device lays them out: [n, 32] bytes."""
        out = np.zeros((self.n, 32), dtype=np.uint8)
        for i, b in enumerate(self.blocks):
            out[i, :16] = np.array(b[:2], dtype=np.float64).view(np.uint8)
            out[i, 16:24] = np.array(b[2:], dtype=np.int32).view(np.uint8)
        return out


def clock_sequence(stamps, arrivals, leak=LEAK, slew=SLEW):
    """tip_clock_rows on one sequence -> (mapped [L] float64, the block it leaves)."""
    block = [0.0, 0.0, 0, 0]
    out = np.array([clock_step(block, s, a, leak, slew) for s, a in zip(stamps, arrivals)], dtype=np.float64).reshape(len(stamps))
    return out, block


# ---- the predict decision ----------------------------------------------------------------------------------------------------------------
def decide(stamps, tau, max_hold, max_predict):
    """-> (flag, i, u): for F_PREDICT and F_INTERP i and i + 1 are the bracket, for F_HELD packet i is copied."""
    hold = -1.0 if max_hold is None else float(max_hold)
    tau = float(tau)
    if len(stamps) >= 2:
        s_last = float(stamps[-1])
        if tau > s_last:
            s_prev = float(stamps[-2])
            h, b = tau - s_last, s_last - s_prev
            if h <= float(max_predict) and h <= PREDICT_SPAN * b and (hold < 0.0 or b <= hold):
                return F_PREDICT, len(stamps) - 2, (tau - s_prev) / b
    return ro.decide(stamps, tau, max_hold, SLERP)


def predict(a, b, u, dtype=np.float64, stored=np.float32):
    """a, b [..., 7] (the earlier and the newer packet's sensor), u [...] fp64, above 1 -> [..., 7] in `dtype`: the quaternion statements
    of resample_oracle.interp with this u, the arc above d = 1 - 1e-6 taken from the chord |qb - qa| (linear weights are a rate error
    once u is past 1); the newer packet's acceleration held in the global frame.  `stored`: what the packets are
    rounded to first — float32, as a ring holds them; float64 to hold the formula itself against an analytic motion."""
    a = np.asarray(a, dtype=stored).astype(dtype)
    b = np.asarray(b, dtype=stored).astype(dtype)
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), a.shape[:-1])
    with np.errstate(all="ignore"):
        _, ok_a = ro.q2r(a[..., :4], dtype)
        Rb, ok_b = ro.q2r(b[..., :4], dtype)
        qa = a[..., :4] / ro._norm(a)[..., None]
        qb = b[..., :4] / ro._norm(b)[..., None]
        dot = qa[..., 0] * qb[..., 0] + qa[..., 1] * qb[..., 1] + qa[..., 2] * qb[..., 2] + qa[..., 3] * qb[..., 3]
        flip = dot < 0
        qb = np.where(flip[..., None], -qb, qb)
        dot = np.where(flip, -dot, dot)
        d = np.minimum(dot.astype(np.float64), 1.0)
        e = qb.astype(np.float64) - qa.astype(np.float64)
        chord = np.sqrt(e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1] + e[..., 2] * e[..., 2] + e[..., 3] * e[..., 3])
        th = np.where(d > 1.0 - 1e-6, 2.0 * np.arcsin(np.minimum(0.5 * chord, 1.0)), np.arccos(d))
        lin = th < TINY_ARC
        st = np.sin(np.where(lin, 1.0, th))
        w0 = np.where(lin, 1.0 - u, np.sin((1.0 - u) * th) / st)
        w1 = np.where(lin, u, np.sin(u * th) / st)
        f0, f1 = w0.astype(dtype)[..., None], w1.astype(dtype)[..., None]
        q = f0 * qa + f1 * qb
        Rq, ok_q = ro.q2r(q, dtype)
        out = np.empty(a.shape, dtype=dtype)
        out[..., :4] = q / ro._norm(q)[..., None]
        g = [Rb[..., r, 0] * b[..., 4] + Rb[..., r, 1] * b[..., 5] + Rb[..., r, 2] * b[..., 6] for r in range(3)]
        for c in range(3):
            out[..., 4 + c] = Rq[..., 0, c] * g[0] + Rq[..., 1, c] * g[1] + Rq[..., 2, c] * g[2]
    out[~(ok_a & ok_b & ok_q)] = np.nan
    return out


def emit_row(stamps, packets, tau, max_hold, max_predict, dtype=np.float32):
    """The predict rule on one ring: stamps [c], packets [c, 42] fp32 -> (row [42] in `dtype`, flag)."""
    f, i, u = decide(stamps, tau, max_hold, max_predict)
    if f == F_HELD:
        return np.asarray(packets[i], dtype=np.float32).astype(dtype), f
    if f in (F_INTERP, F_PREDICT):
        pa, pb = (np.asarray(packets[j], dtype=np.float32).reshape(6, 7) for j in (i, i + 1))
        return (ro.interp if f == F_INTERP else predict)(pa, pb, u, dtype).reshape(PACKET), f
    return np.full(PACKET, np.nan, dtype=dtype), f


class Rings(ro.Rings):
    """resample_oracle.Rings whose emit is tip_predict_emit."""

    def emit(self, t, delay=0.0, max_hold=None, max_predict=0.025, dtype=np.float32):
        t = np.broadcast_to(np.asarray(t, dtype=np.float64), (self.n,))
        out, flags = np.empty((self.n, PACKET), dtype=dtype), np.empty(self.n, dtype=np.uint8)
        for s in range(self.n):
            out[s], flags[s] = emit_row(self.stamps[s], self.packets[s], t[s] - float(delay), max_hold, max_predict, dtype)
        return out, flags

    def image(self):
        """The rings as the device holds them after pushes from a reset: [n, 16 + 176 depth] bytes — head, have, total, dropped; the
        stamps; the packets; an entry that was never written is zero."""
        d = self.depth
        out = np.zeros((self.n, 16 + 176 * d), dtype=np.uint8)
        for s in range(self.n):
            total, have = int(self.total[s]), len(self.stamps[s])
            head = (total - have) % d if have == d else 0
            out[s, :16] = np.array([head, have, total, int(self.dropped[s])], dtype=np.int32).view(np.uint8)
            st, pk = np.zeros(d, dtype=np.float64), np.zeros((d, PACKET), dtype=np.float32)
            for j in range(have):
                st[(head + j) % d], pk[(head + j) % d] = self.stamps[s][j], self.packets[s][j]
            out[s, 16:16 + 8 * d] = st.view(np.uint8)
            out[s, 16 + 8 * d:] = pk.reshape(-1).view(np.uint8)
        return out


def rows(packets, stamps, t_out, delay=0.0, max_hold=None, max_predict=0.025, depth=8, dtype=np.float32):
    """tip_predict_rows on one sequence: packets [L, 42] fp32, stamps [L] strictly increasing, t_out [K] -> ([K, 42] `dtype`, flags)."""
    packets = np.asarray(packets, dtype=np.float32).reshape(-1, PACKET)
    stamps = np.asarray(stamps, dtype=np.float64)
    t_out = np.asarray(t_out, dtype=np.float64)
    out, flags = np.empty((len(t_out), PACKET), dtype=dtype), np.empty(len(t_out), dtype=np.uint8)
    for r, t in enumerate(t_out):
        cnt = int(np.searchsorted(stamps, t, side="right"))
        lo = max(0, cnt - depth)
        out[r], flags[r] = emit_row(stamps[lo:cnt], packets[lo:cnt], float(t) - float(delay), max_hold, max_predict, dtype)
    return out, flags


# ---- inputs shared by the CPU and GPU tests --------------------------------------------------------------------------------------------
def hub(rng, L, rate_hz=100.0, offset=1.7e9, drift=40e-6, base_delay=0.002, mean_jitter=0.003, s0=12.5):
    """L packets of one hub: stamps [L] on its own clock (exactly periodic from s0), the true offset theta_true(s) = offset + drift *
    (s - s0), and arrivals = s + theta_true(s) + base_delay + Exp(mean_jitter) -> (stamps, arrivals, theta_true, delays)."""
    s = s0 + np.arange(L, dtype=np.float64) * (1.0 / rate_hz)
    theta = offset + drift * (s - s0)
    d = base_delay + rng.exponential(mean_jitter, size=L)
    return s, s + theta + d, theta, d


def spin_packets(rng, stamps, rates, acc_sigma=3.0):
    """Packets [L, 42] fp32 of six sensors that each turn at a constant angular rate: sensor k at rates[k] rad/s about a random axis
    from a random start, quaternion lengths 0.5 .. 2 and either sign per packet -> (packets, the same [L, 42] before their rounding to
    fp32, analytic(t) -> Rotation of the six)."""
    from scipy.spatial.transform import Rotation
    L = len(stamps)
    axis = rng.normal(size=(6, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    start = Rotation.random(6, random_state=rng)
    t0 = float(stamps[0])

    def analytic(t):
        return start * Rotation.from_rotvec(axis * (np.asarray(rates, dtype=np.float64) * (float(t) - t0))[:, None])

    out = np.empty((L, 6, 7), dtype=np.float64)
    for j, t in enumerate(stamps):
        out[j, :, :4] = analytic(t).as_quat() * rng.uniform(0.5, 2.0, size=(6, 1)) * rng.choice([-1.0, 1.0], size=(6, 1))
        out[j, :, 4:] = rng.normal(0.0, acc_sigma, size=(6, 3))
    return out.reshape(L, PACKET).astype(np.float32), out.reshape(L, PACKET), analytic
