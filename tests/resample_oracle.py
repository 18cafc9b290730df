"""Oracle of the timestamped-packet resampler (csrc/tip_resample.hip; tip_amd.sensors.PacketResampler, resample_sequences): the push,
emit and rows rules of include/tip_hip.h ("timestamped packets") in numpy, value by value.

    decide        the emit rule's table: which packet(s) of a ring, the flag, and u — Python floats, i.e. fp64 comparisons of the stated
                  expressions, so that the device takes the same branch on the same inputs
    interp        one sensor between two packets, vectorised over any leading shape, in fp64 or in any dtype.  The float32 evaluation
                  follows the header's operation order (every sum left to right, nothing contracted, the two slerp weights in fp64 and
                  rounded once); it is what the GPU tests take their fp32 noise from
    Rings         n rings of `depth` entries with the counters have / total / dropped: push in array order, emit per slot
    rows          a recorded sequence at its query times: per output row the packets not after the tick, of these the last `depth`

The reference has no resampling: its one rule, the zero-order hold of live_demo_new.py:82-115 / :161-162 (the newest packet not after
the tick), is mode HOLD with delay 0, restated by newest_not_after.
"""
import numpy as np

HOLD, SLERP = 0, 1
F_INTERP, F_HELD, F_STALE, F_EMPTY, F_EARLY = range(5)
PACKET = 42


def _max_hold(max_hold):
    return -1.0 if max_hold is None else float(max_hold)


def decide(stamps, tau, max_hold, mode):
    """stamps: strictly increasing floats.  -> (flag, i, u): for F_HELD packet i is copied, for F_INTERP i and i + 1 are the bracket."""
    max_hold = _max_hold(max_hold)
    tau = float(tau)
    if len(stamps) < 1:
        return F_EMPTY, 0, 0.0
    if not tau >= float(stamps[0]):
        return F_EARLY, 0, 0.0
    s_last = float(stamps[-1])
    if tau >= s_last:
        return (F_HELD if (max_hold < 0.0 or tau - s_last <= max_hold) else F_STALE), len(stamps) - 1, 0.0
    i = int(np.searchsorted(np.asarray(stamps, dtype=np.float64), tau, side="right")) - 1
    s0, s1 = float(stamps[i]), float(stamps[i + 1])
    if mode == HOLD or (max_hold >= 0.0 and s1 - s0 > max_hold):
        return (F_HELD if (max_hold < 0.0 or tau - s0 <= max_hold) else F_STALE), i, 0.0
    return F_INTERP, i, (tau - s0) / (s1 - s0)


def _norm(q):
    return np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3])


def q2r(q, dtype):
    """csrc/tip_sensor.h q2r on q [..., 4] (x, y, z, w) in `dtype`: -> (m [..., 3, 3], ok [...])."""
    q = np.asarray(q, dtype=dtype)
    n2 = q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2] + q[..., 3] * q[..., 3]
    ok = (n2 > 0) & np.isfinite(n2)
    n = np.sqrt(n2)
    x, y, z, w = (q[..., j] / n for j in range(4))
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    two = dtype(2)
    m = np.empty(q.shape[:-1] + (3, 3), dtype=dtype)
    m[..., 0, 0], m[..., 0, 1], m[..., 0, 2] = x2 - y2 - z2 + w2, two * (xy - zw), two * (xz + yw)
    m[..., 1, 0], m[..., 1, 1], m[..., 1, 2] = two * (xy + zw), -x2 + y2 - z2 + w2, two * (yz - xw)
    m[..., 2, 0], m[..., 2, 1], m[..., 2, 2] = two * (xz - yw), two * (yz + xw), -x2 - y2 + z2 + w2
    return m, ok


def interp(a, b, u, dtype=np.float64):
    """a, b [..., 7] (q0 q1 q2 q3 ax ay az; the earlier and the later packet's sensor), u [...] fp64 -> [..., 7] in `dtype`."""
    a = np.asarray(a, dtype=np.float32).astype(dtype)
    b = np.asarray(b, dtype=np.float32).astype(dtype)
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), a.shape[:-1])
    with np.errstate(all="ignore"):
        Ra, ok_a = q2r(a[..., :4], dtype)
        Rb, ok_b = q2r(b[..., :4], dtype)
        qa = a[..., :4] / _norm(a)[..., None]
        qb = b[..., :4] / _norm(b)[..., None]
        dot = qa[..., 0] * qb[..., 0] + qa[..., 1] * qb[..., 1] + qa[..., 2] * qb[..., 2] + qa[..., 3] * qb[..., 3]
        flip = dot < 0
        qb = np.where(flip[..., None], -qb, qb)
        dot = np.where(flip, -dot, dot)
        d = np.minimum(dot.astype(np.float64), 1.0)
        lin = d > 1.0 - 1e-6
        th = np.arccos(np.where(lin, 0.5, d))
        st = np.sin(th)
        w0 = np.where(lin, 1.0 - u, np.sin((1.0 - u) * th) / st)
        w1 = np.where(lin, u, np.sin(u * th) / st)
        f0, f1 = w0.astype(dtype)[..., None], w1.astype(dtype)[..., None]
        q = f0 * qa + f1 * qb
        Rq, ok_q = q2r(q, dtype)
        out = np.empty(a.shape, dtype=dtype)
        out[..., :4] = q / _norm(q)[..., None]
        uf = u.astype(dtype)
        vf = dtype(1) - uf
        g = []
        for r in range(3):
            ga = Ra[..., r, 0] * a[..., 4] + Ra[..., r, 1] * a[..., 5] + Ra[..., r, 2] * a[..., 6]
            gb = Rb[..., r, 0] * b[..., 4] + Rb[..., r, 1] * b[..., 5] + Rb[..., r, 2] * b[..., 6]
            g.append(vf * ga + uf * gb)
        for c in range(3):
            out[..., 4 + c] = Rq[..., 0, c] * g[0] + Rq[..., 1, c] * g[1] + Rq[..., 2, c] * g[2]
    out[~(ok_a & ok_b & ok_q)] = np.nan
    return out


def emit_row(stamps, packets, tau, max_hold, mode, dtype=np.float32):
    """The emit rule on one ring: stamps [c], packets [c, 42] fp32 -> (row [42] in `dtype`, flag)."""
    f, i, u = decide(stamps, tau, max_hold, mode)
    if f == F_HELD:
        return np.asarray(packets[i], dtype=np.float32).astype(dtype), f
    if f == F_INTERP:
        pa, pb = (np.asarray(packets[j], dtype=np.float32).reshape(6, 7) for j in (i, i + 1))
        return interp(pa, pb, u, dtype).reshape(PACKET), f
    return np.full(PACKET, np.nan, dtype=dtype), f


class Rings:
    """tip_resample_push / tip_resample_emit / tip_resample_get / tip_resample_reset on n slots."""

    def __init__(self, n, depth):
        self.n, self.depth = int(n), int(depth)
        self.reset()

    def reset(self, slots=None):
        if slots is None:
            self.stamps = [[] for _ in range(self.n)]
            self.packets = [[] for _ in range(self.n)]
            self.total = np.zeros(self.n, dtype=np.int64)
            self.dropped = np.zeros(self.n, dtype=np.int64)
            return
        for s in slots:
            self.stamps[s], self.packets[s], self.total[s], self.dropped[s] = [], [], 0, 0

    def push(self, packets, slots, times):
        packets = np.asarray(packets, dtype=np.float32).reshape(-1, PACKET)
        for p, s, t in zip(packets, np.asarray(slots).reshape(-1), np.asarray(times, dtype=np.float64).reshape(-1)):
            s = int(s)
            if s < 0 or s >= self.n:
                continue
            if not np.isfinite(t) or (self.stamps[s] and t <= self.stamps[s][-1]):
                self.dropped[s] += 1
                continue
            self.stamps[s].append(float(t))
            self.packets[s].append(p.copy())
            if len(self.stamps[s]) > self.depth:
                del self.stamps[s][0], self.packets[s][0]
            self.total[s] += 1

    def emit(self, t, delay=0.0, max_hold=None, mode=SLERP, dtype=np.float32):
        t = np.broadcast_to(np.asarray(t, dtype=np.float64), (self.n,))
        out, flags = np.empty((self.n, PACKET), dtype=dtype), np.empty(self.n, dtype=np.uint8)
        for s in range(self.n):
            out[s], flags[s] = emit_row(self.stamps[s], self.packets[s], t[s] - float(delay), max_hold, mode, dtype)
        return out, flags

    def counts(self):
        """have, dropped, total [n]."""
        return np.array([len(s) for s in self.stamps]), self.dropped.copy(), self.total.copy()


def rows(packets, stamps, t_out, delay=0.0, max_hold=None, mode=SLERP, depth=8, dtype=np.float32):
    """tip_resample_rows on one sequence: packets [L, 42] fp32, stamps [L] strictly increasing, t_out [K] -> ([K, 42] `dtype`, flags)."""
    packets = np.asarray(packets, dtype=np.float32).reshape(-1, PACKET)
    stamps = np.asarray(stamps, dtype=np.float64)
    t_out = np.asarray(t_out, dtype=np.float64)
    out, flags = np.empty((len(t_out), PACKET), dtype=dtype), np.empty(len(t_out), dtype=np.uint8)
    for r, t in enumerate(t_out):
        cnt = int(np.searchsorted(stamps, t, side="right"))
        lo = max(0, cnt - depth)
        out[r], flags[r] = emit_row(stamps[lo:cnt], packets[lo:cnt], float(t) - float(delay), max_hold, mode, dtype)
    return out, flags


def newest_not_after(packets, stamps, tau):
    """The demo's rule by numpy indexing: the newest packet not after each tau [K] -> (indices [K], -1 where there is none)."""
    return np.searchsorted(np.asarray(stamps, dtype=np.float64), np.asarray(tau, dtype=np.float64), side="right") - 1


def rotations(rows_):
    """[..., 42] -> the six rotation matrices of a row's quaternions [..., 6, 3, 3] (fp64; compare R, not q: the sign is free)."""
    r = np.asarray(rows_, dtype=np.float64)
    q = r.reshape(r.shape[:-1] + (6, 7))[..., :4]
    with np.errstate(all="ignore"):
        m, ok = q2r(q, np.float64)
    m[~ok] = np.nan
    return m


def accelerations(rows_):
    r = np.asarray(rows_, dtype=np.float64)
    return r.reshape(r.shape[:-1] + (6, 7))[..., 4:]


# ---- inputs shared by the CPU and GPU tests --------------------------------------------------------------------------------------------
def stamps_at(rng, L, rate_hz, t0=0.0, jitter=0.2):
    """L strictly increasing stamps at rate_hz from t0, each moved by up to +-jitter of a period (jitter < 0.5 keeps the order)."""
    k = np.arange(L, dtype=np.float64)
    return t0 + (k + rng.uniform(-jitter, jitter, size=L)) * (1.0 / rate_hz)


def motion_packets(rng, L, step=0.15, acc_sigma=3.0):
    """L packets [L, 42] fp32 of a moving wearer: per sensor a random start orientation and a random walk of rotation vectors of about
    `step` rad per packet (far below the 3.0 rad at which the shortest arc becomes ambiguous), quaternion lengths 0.5 .. 2 and either
    sign per packet, accelerations N(0, acc_sigma^2)."""
    from scipy.spatial.transform import Rotation
    out = np.empty((L, 6, 7), dtype=np.float64)
    cur = Rotation.random(6, random_state=rng)
    for t in range(L):
        cur = cur * Rotation.from_rotvec(rng.normal(0.0, step / np.sqrt(3.0), size=(6, 3)))
        out[t, :, :4] = cur.as_quat() * rng.uniform(0.5, 2.0, size=(6, 1)) * rng.choice([-1.0, 1.0], size=(6, 1))
        out[t, :, 4:] = rng.normal(0.0, acc_sigma, size=(6, 3))
    return out.reshape(L, PACKET).astype(np.float32)
