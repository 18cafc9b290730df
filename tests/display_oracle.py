"""Oracle of the display-time poses (csrc/tip_display.hip; tip_amd.display.PoseResampler, resample_poses): the push, emit and rows rules
of include/tip_hip.h ("display-time poses") in numpy, value by value.

    decide        the emit decision: resample_oracle.decide behind the prediction branch -> (flag, ia, ib, u), Python floats (fp64)
    aa2q / q2aa   the two conversions; between: one rotation between (flag 0) or past (flag 5) two rows; root: the root's statement
    emit_row      one ring at one time -> (row [57], quat [18, 4], flag)
    Rings         n rings of `depth` entries with the counters: push / emit / counts / reset / image (the device's bytes)
    rows          a recorded track at its output times: per row the entries not after it, of these the last `depth`

dtype=np.float32 follows the kernel's rounding points (fp32 sums left to right; the sines, cosines and arctangents of the conversions
and the two slerp weights in fp64, rounded once); np.float64 is the reference form of the same statements.  `stored` is what a row is
rounded to before anything else: float32, as a ring holds it; float64 to hold the formula itself against an analytic motion.
"""
import numpy as np

import resample_oracle as ro

HOLD, SLERP, PREDICT = 0, 1, 2
F_INTERP, F_HELD, F_STALE, F_EMPTY, F_EARLY, F_PREDICT = 0, 1, 2, 3, 4, 5
ROTS, ROW = 18, 57
AA_SERIES, Q_SERIES, ANTIPODAL, TINY_ARC = 1e-3, 1e-3, 1e-6, 1e-5
DT = 1.0 / 60.0


def block_bytes(depth):
    return (16 + depth * (8 + 4 * ROW) + 7) // 8 * 8


# ---- the decision ------------------------------------------------------------------------------------------------------------------------
def decide(stamps, tau, max_hold=None, max_predict=0.0, baseline=1, mode=PREDICT):
    """-> (flag, ia, ib, u): for F_HELD row ia is copied; for F_INTERP and F_PREDICT ia is the earlier row and ib the later one."""
    hold = -1.0 if max_hold is None else float(max_hold)
    tau = float(tau)
    cnt = len(stamps)
    if mode == PREDICT and cnt >= 2:
        s_last = float(stamps[-1])
        if tau > s_last:
            b = min(int(baseline), cnt - 1)
            s_a = float(stamps[cnt - 1 - b])
            h, span = tau - s_last, s_last - s_a
            if h <= float(max_predict) and (hold < 0.0 or span <= float(b) * hold):
                return F_PREDICT, cnt - 1 - b, cnt - 1, (tau - s_a) / span
    f, i, u = ro.decide(stamps, tau, max_hold, ro.HOLD if mode == HOLD else ro.SLERP)
    return f, i, (i + 1 if f == F_INTERP else i), u


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------------
def _sum3(v):
    return v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]


def _dot4(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2] + a[..., 3] * b[..., 3]


def aa2q(a, dtype=np.float64):
    """Axis-angles [..., 3] (already in `dtype`) -> quaternions x y z w [..., 4]."""
    a = np.asarray(a, dtype=dtype)
    with np.errstate(all="ignore"):
        t2 = _sum3(a)
        t = np.sqrt(t2)
        t64 = t.astype(np.float64)
        s = np.where(t < dtype(AA_SERIES), dtype(0.5) - t2 / dtype(48), (np.sin(0.5 * t64) / t64).astype(dtype))
        w = np.cos(0.5 * t64).astype(dtype)
    return np.concatenate((s[..., None] * a, w[..., None]), axis=-1)


def q2aa(q, dtype=np.float64):
    """Unit quaternions [..., 4] -> axis-angles [..., 3], the angle in [0, pi]."""
    q = np.asarray(q, dtype=dtype)
    with np.errstate(all="ignore"):
        q = np.where((q[..., 3] < 0)[..., None], -q, q)
        v2 = _sum3(q)
        v = np.sqrt(v2)
        v64, w64 = v.astype(np.float64), q[..., 3].astype(np.float64)
        k = np.where(v < dtype(Q_SERIES), dtype(2) + v2 / dtype(3), (2.0 * np.arctan2(v64, w64) / v64).astype(dtype))
    return k[..., None] * q[..., :3]


def slerp(qa, qb, u, dtype=np.float64, past=False):
    """The quaternion statements of the packet interpolation (past False) or of the predicted sensor (past True) on qa, qb [..., 4] in
    `dtype`, u [...] fp64 -> unit q [..., 4], NaN where a quaternion has no rotation."""
    qa, qb = np.asarray(qa, dtype=dtype), np.asarray(qb, dtype=dtype)
    u = np.broadcast_to(np.asarray(u, dtype=np.float64), qa.shape[:-1])
    with np.errstate(all="ignore"):
        na2, nb2 = _dot4(qa, qa), _dot4(qb, qb)
        ok = (na2 > 0) & np.isfinite(na2) & (nb2 > 0) & np.isfinite(nb2)
        qa = qa / np.sqrt(na2)[..., None]
        qb = qb / np.sqrt(nb2)[..., None]
        dot = _dot4(qa, qb)
        flip = dot < 0
        qb = np.where(flip[..., None], -qb, qb)
        dot = np.where(flip, -dot, dot)
        d = np.minimum(dot.astype(np.float64), 1.0)
        if past:
            e = qb.astype(np.float64) - qa.astype(np.float64)
            chord = np.sqrt(_dot4(e, e))
            th = np.where(d > 1.0 - 1e-6, 2.0 * np.arcsin(np.minimum(0.5 * chord, 1.0)), np.arccos(d))
            lin = th < TINY_ARC
        else:
            lin = d > 1.0 - 1e-6
            th = np.arccos(np.where(lin, 0.5, d))
        st = np.sin(np.where(lin, 1.0, th))
        w0 = np.where(lin, 1.0 - u, np.sin((1.0 - u) * th) / st)
        w1 = np.where(lin, u, np.sin(u * th) / st)
        q = w0.astype(dtype)[..., None] * qa + w1.astype(dtype)[..., None] * qb
        nq2 = _dot4(q, q)
        ok &= (nq2 > 0) & np.isfinite(nq2)
        out = q / np.sqrt(nq2)[..., None]
    out[~ok] = np.nan
    return out


def between(a, b, u, dtype=np.float64, past=False, stored=np.float32):
    """One rotation between (or past) two rows: a, b axis-angles [..., 3], u [...] fp64 -> (axis-angle [..., 3], quaternion [..., 4])."""
    a = np.asarray(a, dtype=stored).astype(dtype)
    b = np.asarray(b, dtype=stored).astype(dtype)
    qa, qb = aa2q(a, dtype), aa2q(b, dtype)
    with np.errstate(all="ignore"):
        apart = ~(np.abs(_dot4(qa, qb)) > dtype(np.float32(ANTIPODAL)))       # (the header's constant is an fp32 literal)
    q = slerp(qa, qb, u, dtype, past)
    q[apart] = np.nan
    return q2aa(q, dtype), q


def root(pa, pb, u, dtype=np.float64, stored=np.float32):
    pa = np.asarray(pa, dtype=stored).astype(dtype)
    pb = np.asarray(pb, dtype=stored).astype(dtype)
    uf = np.asarray(u, dtype=np.float64).astype(dtype)[..., None]
    vf = dtype(1) - uf
    with np.errstate(all="ignore"):
        out = vf * pa + uf * pb
    bad = ~(np.isfinite(pa).all(axis=-1) & np.isfinite(pb).all(axis=-1))
    out[bad] = np.nan
    return out


def emit_row(stamps, rows_, tau, max_hold=None, max_predict=0.0, baseline=1, mode=PREDICT, dtype=np.float32):
    """One ring at one time: stamps [c], rows_ [c, 57] fp32 -> (row [57] and quat [18, 4] in `dtype`, flag)."""
    f, ia, ib, u = decide(stamps, tau, max_hold, max_predict, baseline, mode)
    if f == F_HELD:
        r = np.asarray(rows_[ia], dtype=np.float32)
        return r.astype(dtype), aa2q(r[3:].reshape(ROTS, 3).astype(dtype), dtype), f
    if f in (F_INTERP, F_PREDICT):
        ra, rb = (np.asarray(rows_[j], dtype=np.float32) for j in (ia, ib))
        aa, q = between(ra[3:].reshape(ROTS, 3), rb[3:].reshape(ROTS, 3), u, dtype, past=f == F_PREDICT)
        return np.concatenate((root(ra[:3], rb[:3], u, dtype), aa.reshape(-1))), q, f
    return np.full(ROW, np.nan, dtype=dtype), np.full((ROTS, 4), np.nan, dtype=dtype), f


class Rings:
    """tip_pose_push / tip_pose_emit / tip_pose_get / tip_pose_reset on n slots."""

    def __init__(self, n, depth):
        self.n, self.depth = int(n), int(depth)
        self.reset()

    def reset(self, slots=None):
        if slots is None:
            self.stamps = [[] for _ in range(self.n)]
            self.rows = [[] for _ in range(self.n)]
            self.total = np.zeros(self.n, dtype=np.int64)
            self.dropped = np.zeros(self.n, dtype=np.int64)
            return
        for s in slots:
            self.stamps[s], self.rows[s], self.total[s], self.dropped[s] = [], [], 0, 0

    def push(self, root_, s_rest, t, valid=None, slots=None):
        """root_ [n, 3], s_rest [n, >= 54], t a number or [n], valid [n] or None, slots a list (entries outside [0, n) are skipped)."""
        root_ = np.asarray(root_, dtype=np.float32).reshape(self.n, 3)
        s_rest = np.asarray(s_rest, dtype=np.float32).reshape(self.n, -1)
        t = np.broadcast_to(np.asarray(t, dtype=np.float64), (self.n,))
        for s in (range(self.n) if slots is None else slots):
            s = int(s)
            if s < 0 or s >= self.n or (valid is not None and not valid[s]):
                continue
            if not np.isfinite(t[s]) or (self.stamps[s] and t[s] <= self.stamps[s][-1]):
                self.dropped[s] += 1
                continue
            self.stamps[s].append(float(t[s]))
            self.rows[s].append(np.concatenate((root_[s], s_rest[s, :54])))
            if len(self.stamps[s]) > self.depth:
                del self.stamps[s][0], self.rows[s][0]
            self.total[s] += 1

    def emit(self, t, delay=0.0, max_hold=None, max_predict=0.0, baseline=1, mode=PREDICT, dtype=np.float32):
        """-> (q [n, 57], quat [n, 18, 4], flags [n])."""
        t = np.broadcast_to(np.asarray(t, dtype=np.float64), (self.n,))
        q, quat = np.empty((self.n, ROW), dtype=dtype), np.empty((self.n, ROTS, 4), dtype=dtype)
        flags = np.empty(self.n, dtype=np.uint8)
        for s in range(self.n):
            q[s], quat[s], flags[s] = emit_row(self.stamps[s], self.rows[s], t[s] - float(delay), max_hold, max_predict, baseline, mode, dtype)
        return q, quat, flags

    def counts(self):
        """have, dropped, total [n]."""
        return np.array([len(s) for s in self.stamps]), self.dropped.copy(), self.total.copy()

    def image(self):
        """The rings as the device holds them after pushes from a reset: [n, block_bytes(depth)] bytes — head, have, total, dropped;
        the stamps; the rows; the padding; an entry that was never written is zero."""
        d = self.depth
        out = np.zeros((self.n, block_bytes(d)), dtype=np.uint8)
        for s in range(self.n):
            total, have = int(self.total[s]), len(self.stamps[s])
            head = (total - have) % d if have == d else 0
            out[s, :16] = np.array([head, have, total, int(self.dropped[s])], dtype=np.int32).view(np.uint8)
            st, rw = np.zeros(d, dtype=np.float64), np.zeros((d, ROW), dtype=np.float32)
            for j in range(have):
                st[(head + j) % d], rw[(head + j) % d] = self.stamps[s][j], self.rows[s][j]
            out[s, 16:16 + 8 * d] = st.view(np.uint8)
            out[s, 16 + 8 * d:16 + 8 * d + 4 * ROW * d] = rw.reshape(-1).view(np.uint8)
        return out


def rows(stamps, root_, rows_, t_out, delay=0.0, max_hold=None, max_predict=0.0, baseline=1, mode=PREDICT, depth=8, dtype=np.float32):
    """tip_pose_rows on one track: stamps [L] strictly increasing, root_ [L, 3], rows_ [L, >= 54], t_out [K] ->
    (q [K, 57], quat [K, 18, 4], flags [K])."""
    stamps = np.asarray(stamps, dtype=np.float64)
    full = np.concatenate((np.asarray(root_, dtype=np.float32).reshape(-1, 3), np.asarray(rows_, dtype=np.float32)[:, :54]), axis=1)
    t_out = np.asarray(t_out, dtype=np.float64)
    q, quat = np.empty((len(t_out), ROW), dtype=dtype), np.empty((len(t_out), ROTS, 4), dtype=dtype)
    flags = np.empty(len(t_out), dtype=np.uint8)
    for r, t in enumerate(t_out):
        cnt = int(np.searchsorted(stamps, t, side="right"))
        lo = max(0, cnt - depth)
        q[r], quat[r], flags[r] = emit_row(stamps[lo:cnt], full[lo:cnt], float(t) - float(delay), max_hold, max_predict, baseline, mode, dtype)
    return q, quat, flags


def rotations(q):
    """Rows [..., 57] -> their 18 rotation matrices [..., 18, 3, 3] (fp64, scipy; NaN where the axis-angle is)."""
    from scipy.spatial.transform import Rotation
    a = np.asarray(q, dtype=np.float64)[..., 3:].reshape(-1, 3)
    bad = ~np.isfinite(a).all(axis=1)
    m = Rotation.from_rotvec(np.where(bad[:, None], 0.0, a)).as_matrix()
    m[bad] = np.nan
    return m.reshape(np.shape(q)[:-1] + (ROTS, 3, 3))


def quat_rotations(quat):
    """Quaternions [..., 18, 4] -> rotation matrices [..., 18, 3, 3] (fp64; NaN where the quaternion is)."""
    with np.errstate(all="ignore"):
        m, ok = ro.q2r(np.asarray(quat, dtype=np.float64), np.float64)
    m[~ok] = np.nan
    return m


# ---- inputs shared by the CPU and GPU tests ----------------------------------------------------------------------------------------------
def smooth_track(rng, L, rate_hz=60.0, amp=0.6, speed=1.0, width=111):
    """L rows of a moving body at rate_hz: per joint axis a sum of three sinusoids (amplitude `amp` rad in all, 0.3 .. 2 Hz times
    `speed`) and a root that walks a curve -> (root [L, 3] fp32, s_rest [L, width] fp32 — the first 54 columns the axis-angles, the rest
    noise — and t [L] fp64 from 0)."""
    t = np.arange(L, dtype=np.float64) / rate_hz
    f = rng.uniform(0.3, 2.0, size=(3, 54)) * speed
    ph = rng.uniform(0.0, 2 * np.pi, size=(3, 54))
    am = rng.uniform(0.2, 1.0, size=(3, 54)) * (amp / 3.0)
    aa = (am[None] * np.sin(2 * np.pi * f[None] * t[:, None, None] + ph[None])).sum(axis=1)
    rt = np.stack((1.2 * t + 0.3 * np.sin(1.3 * t), 0.4 * np.sin(0.7 * t + 1.0), 0.95 + 0.03 * np.sin(2 * np.pi * 1.8 * t)), axis=1)
    s_rest = rng.normal(size=(L, width))
    s_rest[:, :54] = aa
    return rt.astype(np.float32), s_rest.astype(np.float32), t


def spin_track(rng, stamps, rates):
    """An analytic track: joint k turns at rates[k] rad/s about a fixed random axis from a random start, the root moves at a constant
    velocity -> (root [L, 3] fp64, axis-angles [L, 18, 3] fp64 (not rounded), analytic(t) -> (Rotation of the 18, root [3]))."""
    from scipy.spatial.transform import Rotation
    axis = rng.normal(size=(ROTS, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    start = Rotation.random(ROTS, random_state=rng)
    p0, vel = rng.normal(size=3), rng.normal(size=3)
    t0 = float(stamps[0])
    rates = np.broadcast_to(np.asarray(rates, dtype=np.float64), (ROTS,))

    def analytic(t):
        return start * Rotation.from_rotvec(axis * (rates * (float(t) - t0))[:, None]), p0 + vel * (float(t) - t0)

    aa = np.stack([analytic(t)[0].as_rotvec() for t in stamps])
    rt = np.stack([analytic(t)[1] for t in stamps])
    return rt, aa, analytic
