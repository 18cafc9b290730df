"""Display-time poses: every wearer's pose at the VIEWER's time (csrc/tip_display.hip; include/tip_hip.h, "display-time poses").

The input side of a pool is free of the 60 Hz grid (sensors.PacketResampler, ClockSync, mode "predict"); its output is not.  A frame's
pose comes once per tick, and it belongs to IMU_N_SMOOTH = 5 frames — 83 ms — before the packet that produced it (the centred 11-tap
acceleration average, real_time_runner.py:279-296, :391-393).  A viewer on its own clock — a headset at 72, 90 or 120 Hz, a renderer that
wants the pose at its next vsync, an export of a replayed session at 30 or 100 fps — gets poses on someone else's grid that are a tenth
of a second old.  PoseResampler keeps each slot's last poses with their fp64 stamps on the device and gives every slot its pose at any
time: held, interpolated between the two entries around it, or continued past the newest one (joints at a constant angular rate, the
root at a constant velocity).  It is a consumer beside the frame, as the trackers and the recorder are:

    ps = PoseResampler(engine.n, engine.device)                       # mode "predict", up to 9 frames past the newest pose
    out = engine.step(frame)                                          # ... at tick t
    root, _ = tracker.step(out)
    if out is not None:                                               # (the lock-step StreamingEngine returns None while it primes)
        ps.push(root, out["s_rest"], pose_time(t), valid=out["valid"])    # one launch, no synchronisation
    q = ps.emit(t_display)                                            # one launch, whenever the viewer wants a pose: [n, 57]
    pq = kinematics.fk(skel, q, scale=tracker.scale)                  # (ps.flags says how each row came about, ps.quat its quaternions)

resample_poses is the same rule for recorded or replayed tracks, all of them in one launch.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import lib as _lib
from . import sensors as _sn
from .replay import DT, IMU_N_SMOOTH
from .streaming import slot_list

MODES = {"hold": _lib.TIP_POSE_HOLD, "slerp": _lib.TIP_POSE_SLERP, "predict": _lib.TIP_POSE_PREDICT}
INTERPOLATED, HELD, STALE, EMPTY, EARLY, PREDICTED = 0, 1, 2, 3, 4, 5      # flags; STALE, EMPTY and EARLY rows are NaN
ROW, ROTS = 57, 18
# The lag a viewer may want to predict across, in frames: IMU_N_SMOOTH (exact: pose_time) + the 6-tap 0.6**k output filter's mean delay
# (sum k 0.6^k / sum 0.6^k = 2.8752 / 2.38336 = 1.206) + the average with the previous pose (0.5) = 6.7; two frames of slack on top.
# A cap, not a measurement: tools/display_bench.py records the prediction error at every horizon up to it.
FILTER_DELAY_FRAMES = 2.8752 / 2.38336
AVERAGE_DELAY_FRAMES = 0.5
MAX_PREDICT = 9 * DT
LIST_CACHE = 64                           # distinct host slot lists of push() kept on the device


def pose_time(tick):
    """The stamp of the pose that the frame fed at `tick` (seconds, a number or an array) produces: tick - IMU_N_SMOOTH * DT, exact by
    construction — the engines' state prediction is for t - IMU_n_smooth (real_time_runner.py:391-393).  Two further delays are the
    output filters', which the library does not apply and does not compensate: a caller that runs the reference's 6-tap 0.6**k filter
    (real_time_runner.py:110-111, :307-320) shows poses a further FILTER_DELAY_FRAMES = 1.206 frames old on average, and one that
    averages with the previous pose (:446-449) AVERAGE_DELAY_FRAMES = 0.5 more; such a caller asks for emit(t + lead) with the lead it
    owes."""
    if isinstance(tick, torch.Tensor):
        return tick.to(torch.float64) - IMU_N_SMOOTH * DT
    return np.asarray(tick, dtype=np.float64) - IMU_N_SMOOTH * DT if np.ndim(tick) else float(tick) - IMU_N_SMOOTH * DT


def _rule(mode, delay, max_hold, max_predict, baseline, depth, who):
    """(mode, delay, max_hold, max_predict, baseline, depth) as the C ABI takes them; anything else is a ValueError in `who`'s name."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"tip_amd.display.{who}: mode is \"predict\", \"slerp\" or \"hold\"; got {mode!r}")

    def number(v):
        try:
            return float(v)
        except (TypeError, ValueError):
            return float("nan")
    d = number(delay)
    if not (d >= 0.0 and np.isfinite(d)):
        raise ValueError(f"tip_amd.display.{who}: delay is the age of the emitted pose in seconds, a finite number >= 0 (a pose past the "
                         f"newest entry is mode \"predict\"'s with max_predict, never a negative delay); got {delay!r}")
    if max_hold is None:
        hold = -1.0
    else:
        hold = number(max_hold)
        if not hold >= 0.0:
            raise ValueError(f"tip_amd.display.{who}: max_hold is None (no limit) or the oldest pose that may be held, in seconds >= 0; "
                             f"got {max_hold!r}")
    far = number(max_predict)
    if not (far >= 0.0 and np.isfinite(far)):
        raise ValueError(f"tip_amd.display.{who}: max_predict is how far past the newest pose a row may be predicted, a finite number of "
                         f"seconds >= 0; got {max_predict!r}")
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 2 <= depth <= 64:
        raise ValueError(f"tip_amd.display.{who}: depth is the number of poses a slot keeps, an int in 2 .. 64; got {depth!r}")
    if isinstance(baseline, bool) or not isinstance(baseline, (int, np.integer)) or not 1 <= baseline <= depth - 1:
        raise ValueError(f"tip_amd.display.{who}: baseline is how many entries back from the newest the rate is taken over, an int in "
                         f"1 .. depth - 1 = {int(depth) - 1}; got {baseline!r}")
    return MODES[mode], d, hold, far, int(baseline), int(depth)


def block_bytes(depth: int) -> int:
    """The bytes of one slot's block (tip_pose_state_bytes(1, depth)): header, stamps, rows, padded to 8."""
    return (16 + int(depth) * (8 + 4 * ROW) + 7) // 8 * 8


class PoseResampler:
    """n rings of the last `depth` poses with their fp64 stamps on `device`, and the launch that gives every slot its pose at a time.
    mode "hold": the newest pose not after t - delay; "slerp": interpolated between the two poses around t - delay (joints on the
    shorter arc, the root linearly), the newest one held past it; "predict": "slerp", and past the newest pose the joints continued at
    the angular rate, the root at the velocity, of the newest entry and the one `baseline` entries before it, by at most max_predict
    seconds (the default is a cap of 9 frames, see MAX_PREDICT).  max_hold (seconds; None: no limit): a pose older than that is not
    held and nothing is interpolated or predicted across a longer gap per bracket — the row is NaN.  No call synchronises; everything
    runs on the current stream; push and emit take only static arguments, so both can sit in a captured graph."""

    def __init__(self, n: int, device, *, mode: str = "predict", delay: float = 0.0, max_hold=None, max_predict=MAX_PREDICT,
                 baseline: int = 1, depth: int = 8):
        who = "PoseResampler"
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"tip_amd.display.{who}: n is the number of slots, at least 1; got {n!r}")
        self.n = int(n)
        self.mode_name = mode
        self.mode, self.delay, self.max_hold, self.max_predict, self.baseline, self.depth = _rule(mode, delay, max_hold, max_predict,
                                                                                                  baseline, depth, who)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("tip_amd.display.PoseResampler runs on an MI355X: give it the engine's device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.load()
        nbytes = ctypes.c_size_t()
        _lib.check(self.lib.tip_pose_state_bytes(self.n, self.depth, ctypes.byref(nbytes)))
        assert nbytes.value == self.n * block_bytes(self.depth)
        with torch.cuda.device(self.device):
            self.state = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            self.t_push = torch.zeros(self.n, dtype=torch.float64, device=self.device)
            self.t = torch.zeros(self.n, dtype=torch.float64, device=self.device)
            self.flags = torch.full((self.n,), EMPTY, dtype=torch.uint8, device=self.device)
            self.quat = torch.full((self.n, ROTS, 4), float("nan"), dtype=torch.float32, device=self.device)
            self._lists = {}
            _lib.check(self.lib.tip_pose_reset(self.state.data_ptr(), self.n, self.depth, None, 0, self._stream()))

    def _stream(self):
        return _lib.current_stream(self.device)

    def _slots(self, slots, who):
        return list(range(self.n)) if slots is None else slot_list(slots, self.n, f"display.PoseResampler.{who}")

    def _times(self, t, own, who):
        """t as the device float64 [n] a launch reads: a CUDA float64 [n] where it lies, anything else through the buffer `own`."""
        if isinstance(t, bool):
            raise ValueError(f"{who}: t is a number or [{self.n}] times in seconds; got {t!r}")
        h = _sn._times_f64(t, f"{who}: t")
        if h.dim() > 1 or (h.dim() == 1 and tuple(h.shape) != (self.n,)):
            raise ValueError(f"{who}: t is a number or [{self.n}] times in seconds; got {tuple(h.shape)}")
        if h.is_cuda and h.dim() == 1 and isinstance(t, torch.Tensor) and t.dtype == torch.float64:
            if h.device != self.device or not h.is_contiguous():
                raise ValueError(f"{who}: a CUDA float64 [{self.n}] tensor is read where it lies: it must be contiguous and on {self.device}")
            return h
        if h.dim() == 0 and not h.is_cuda:
            own.fill_(float(h))
        else:                                                     # (a 0-d value is broadcast)
            own.copy_(h if h.is_cuda else h.contiguous().pin_memory(), non_blocking=True)
        return own

    def push(self, root, s_rest, t, valid=None, slots=None):
        """Append this frame's poses: root [n, 3] (the tracker's) and s_rest [n, >= 54] (the engine's out["s_rest"]; its first 54 columns
        are read), CUDA float32 and contiguous, used where they lie.  t: the poses' stamp, a number (one time for the pool) or [n],
        read as float64 with PacketResampler.emit's rules — a CUDA float64 [n] is used in place, a narrower float type is refused;
        pose_time(tick) is the stamp of the frame fed at `tick`.  valid (the engine's out["valid"], a CUDA bool or uint8 [n]; None:
        every slot): a slot whose entry is False appends nothing.  slots: the slots to append (None: all); one outside [0, n) is
        skipped; a CUDA int32 tensor is used where it lies, which is the form for lists that change every frame (a host list is uploaded
        once and kept, the LIST_CACHE most recent distinct ones; a host [n] of times likewise goes up through pinned memory at every call,
        a CUDA float64 [n] does not).  A stamp that is not finite or not above the slot's newest is refused and
        counted.  One launch, no synchronisation."""
        who = "tip_amd.display.PoseResampler.push"
        for x, name, tail, least in ((root, "root", 3, 3), (s_rest, "s_rest", None, 54)):
            if (not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != self.n or x.shape[1] < least
                    or (tail is not None and x.shape[1] != tail)):
                raise ValueError(f"{who}: {name} is a float32 [{self.n}, {'>= 54' if tail is None else tail}] tensor; got "
                                 f"{(x.dtype, tuple(x.shape)) if isinstance(x, torch.Tensor) else type(x).__name__}")
            if x.device != self.device or not x.is_contiguous():
                raise ValueError(f"{who}: {name} is read where it lies: it must be contiguous and on {self.device}")
        if valid is not None:
            if not (isinstance(valid, torch.Tensor) and valid.dtype in (torch.bool, torch.uint8) and tuple(valid.shape) == (self.n,)):
                raise ValueError(f"{who}: valid is a bool or uint8 tensor [{self.n}] (the engine's out[\"valid\"])")
            if valid.device != self.device or not valid.is_contiguous():
                raise ValueError(f"{who}: valid is read where it lies: it must be contiguous and on {self.device}")
        sl, count = None, 0
        if slots is not None:
            if isinstance(slots, torch.Tensor) and slots.is_cuda:
                if slots.dtype != torch.int32 or slots.dim() != 1 or slots.device != self.device or not slots.is_contiguous():
                    raise ValueError(f"{who}: a CUDA slots tensor is a contiguous int32 [count] on {self.device}")
                sl, count = slots, int(slots.shape[0])
            else:
                try:
                    idx = tuple(int(i) for i in (slots.tolist() if isinstance(slots, (torch.Tensor, np.ndarray)) else slots))
                except (TypeError, ValueError):
                    raise ValueError(f"{who}: slots is a list of slot indices") from None
                if len(set(idx)) != len(idx):
                    raise ValueError(f"{who}: duplicate slot index")
                if not idx:
                    return
                if idx not in self._lists:
                    if len(self._lists) >= LIST_CACHE:            # (the oldest list goes; its memory is reused in stream order)
                        self._lists.pop(next(iter(self._lists)))
                    with torch.cuda.device(self.device):
                        self._lists[idx] = torch.tensor(idx, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
                sl, count = self._lists[idx], len(idx)
        tq = self._times(t, self.t_push, who)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.tip_pose_push(self.state.data_ptr(), self.n, self.depth, None if sl is None else sl.data_ptr(), count,
                                              root.data_ptr(), s_rest.data_ptr(), int(s_rest.shape[1]),
                                              None if valid is None else valid.data_ptr(), tq.data_ptr(), self._stream()))

    def emit(self, t, out=None):
        """Every slot's pose at time t -> q, a CUDA float32 [n, 57] (`out`, or a new tensor): root xyz, the root's axis-angle, the 17
        joints' — what kinematics.fk takes.  `flags` [n] uint8 says how each row came about (INTERPOLATED, HELD, PREDICTED; STALE, EMPTY
        and EARLY rows are NaN) and `quat` [n, 18, 4] holds the row's rotations as unit quaternions x y z w; both are tensors of the
        object, reused every call.  t: a number or anything 0-d, or [n], read as PacketResampler.emit reads it: a CUDA float64 [n] is
        read WHERE IT LIES (what a captured frame needs).  emit(t + lead) for a viewer that owes its own filters a lead (pose_time)."""
        who = "tip_amd.display.PoseResampler.emit"
        if out is None:
            out = torch.empty((self.n, ROW), dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
              or tuple(out.shape) != (self.n, ROW) or not out.is_contiguous()):
            raise ValueError(f"{who}: out is a contiguous float32 [{self.n}, {ROW}] tensor on {self.device}")
        tq = self._times(t, self.t, who)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.tip_pose_emit(self.state.data_ptr(), self.n, self.depth, tq.data_ptr(), self.delay, self.max_hold,
                                              self.max_predict, self.baseline, self.mode, out.data_ptr(), self.quat.data_ptr(),
                                              self.flags.data_ptr(), self._stream()))
        return out

    def reset(self, slots=None):
        """Empty the rings and zero the counters of the listed slots (None: all): a slot that takes a new wearer."""
        idx = self._slots(slots, "reset")
        if not idx:
            return
        with torch.cuda.device(self.device):
            sl = _sn._to(torch.tensor(idx, dtype=torch.int32), self.device)
            _lib.check(self.lib.tip_pose_reset(self.state.data_ptr(), self.n, self.depth, sl.data_ptr(), len(idx), self._stream()))

    def counts(self, slots=None):
        """(have, dropped, total) of the listed slots (None: all), three CUDA int32 tensors [len(slots)]: poses in the ring (0 .. depth),
        poses refused for their stamp, poses taken since the last reset."""
        idx = self._slots(slots, "counts")
        out = torch.zeros((len(idx), 3), dtype=torch.int32, device=self.device)
        if idx:
            with torch.cuda.device(self.device):
                sl = _sn._to(torch.tensor(idx, dtype=torch.int32), self.device)
                _lib.check(self.lib.tip_pose_get(self.state.data_ptr(), self.n, self.depth, sl.data_ptr(), len(idx), out.data_ptr(),
                                                 self._stream()))
        return out[:, 0], out[:, 1], out[:, 2]

    def export_slots(self, slots):
        """The listed slots' pose rings for import_slots of another PoseResampler of the same `depth` (tip_amd.handover); mode, delay and
        limits belong to the object, not the wearer.  One launch, no synchronisation."""
        from . import handover
        return handover.export_simple(self, slots, "poses")

    def import_slots(self, slots, exported):
        """Put exported rings into the listed slots, whatever those held; another `depth` is a ValueError before anything is launched."""
        from . import handover
        handover.import_simple(self, slots, exported, "poses")


def resample_poses(root_list, rows_list, stamps_list, t_out_list=None, *, rate_hz=None, mode="predict", delay=0.0, max_hold=None,
                   max_predict=MAX_PREDICT, baseline=1, depth=8, device=None, host=False, quat=False):
    """Recorded or replayed pose tracks at any output times, all in one launch: root_list[i] is [L_i, 3], rows_list[i] [L_i, >= 54]
    (axis-angles in the first 54 columns: a ReplayResult's s_rest, or qdq[:, 3:] of what kinematics.track_replay returns) and
    stamps_list[i] its stamps [L_i] (float64 seconds; finite and strictly increasing, else a ValueError naming the sequence and the
    row).  Output times: t_out_list[i] [K_i] (float64, any order), or rate_hz= for sensors.sequence_ticks(stamps, rate_hz, delay) — a
    replayed session at 30, 90 or 120 fps.  Every output row is what a PoseResampler(mode, delay, max_hold, max_predict, baseline,
    depth) that was pushed everything stamped up to the row's time emits there, bit for bit.  Returns (q, flags): lists of CUDA float32
    [K_i, 57] and uint8 [K_i] (host=True: numpy arrays); quat=True adds the list of quaternions [K_i, 18, 4]."""
    who = "resample_poses"
    mode_c, delay, hold, far, baseline, depth = _rule(mode, delay, max_hold, max_predict, baseline, depth, who)
    if (t_out_list is None) == (rate_hz is None):
        raise ValueError(f"tip_amd.display.{who}: give the output times as t_out_list or as rate_hz=, one of the two")
    if rate_hz is not None:
        rate = float(rate_hz)
        if not (rate > 0.0 and np.isfinite(rate)):
            raise ValueError(f"tip_amd.display.{who}: rate_hz is the output rate, a finite number > 0; got {rate_hz!r}")
    if not len(rows_list):
        raise ValueError(f"tip_amd.display.{who}: no sequences")
    if len(root_list) != len(rows_list):
        raise ValueError(f"tip_amd.display.{who}: {len(root_list)} root arrays for {len(rows_list)} row arrays")
    lens = []
    for i, (r, p) in enumerate(zip(rows_list, root_list)):
        shape, pshape = (tuple(x.shape) if hasattr(x, "shape") else np.shape(x) for x in (r, p))
        if len(shape) != 2 or shape[1] < 54:
            raise ValueError(f"tip_amd.display.{who}: rows_list[{i}] is [L, >= 54]; got {shape}")
        if pshape != (shape[0], 3):
            raise ValueError(f"tip_amd.display.{who}: root_list[{i}] is [{shape[0]}, 3], one root per row; got {pshape}")
        lens.append(int(shape[0]))
    if len(stamps_list) != len(lens):
        raise ValueError(f"tip_amd.display.{who}: {len(lens)} row arrays for {len(stamps_list)} stamp arrays")
    stamps = []
    for i, (t, L) in enumerate(zip(stamps_list, lens)):                # (sensors.resample_sequences' checks)
        t = _sn._times_f64(t, f"tip_amd.display.{who}: stamps_list[{i}]").detach().cpu().numpy()
        if t.shape != (L,):
            raise ValueError(f"tip_amd.display.{who}: stamps_list[{i}] is [{L}], one stamp per row; got {t.shape}")
        bad = np.flatnonzero(~np.isfinite(t))
        if bad.size:
            raise ValueError(f"tip_amd.display.{who}: stamps_list[{i}] row {int(bad[0])} is not finite")
        bad = np.flatnonzero(~(np.diff(t) > 0.0))
        if bad.size:
            raise ValueError(f"tip_amd.display.{who}: stamps_list[{i}] row {int(bad[0]) + 1} is not after row {int(bad[0])} "
                             "(stamps are strictly increasing)")
        stamps.append(np.ascontiguousarray(t, dtype=np.float64))
    if rate_hz is not None:
        ticks = [_sn.sequence_ticks(s, rate, delay) for s in stamps]
    else:
        if len(t_out_list) != len(lens):
            raise ValueError(f"tip_amd.display.{who}: {len(t_out_list)} output-time arrays for {len(lens)} sequences")
        ticks = []
        for i, t in enumerate(t_out_list):
            h = _sn._times_f64(t, f"tip_amd.display.{who}: t_out_list[{i}]")
            if h.dim() != 1:
                raise ValueError(f"tip_amd.display.{who}: t_out_list[{i}] is [K] output times; got {tuple(h.shape)}")
            ticks.append(h.detach().cpu().numpy())
    out_lens = [int(t.shape[0]) for t in ticks]
    dev = _sn._device_of(list(rows_list) + list(root_list), device)
    lib = _lib.load()
    with torch.cuda.device(dev):
        rows, in_off, _ = _sn._stack([torch.as_tensor(r)[:, :54] for r in rows_list], torch.float32, 54, dev, who, "rows_list")
        root, _, _ = _sn._stack(root_list, torch.float32, 3, dev, who, "root_list")
        st = _sn._to(torch.from_numpy(np.concatenate(stamps)), dev)
        t_out = _sn._to(torch.from_numpy(np.ascontiguousarray(np.concatenate(ticks), dtype=np.float64)), dev)
        out_off = _sn._to(torch.tensor(np.concatenate(([0], np.cumsum(out_lens))), dtype=torch.int64), dev)
        K = int(sum(out_lens))
        q = torch.empty((K, ROW), dtype=torch.float32, device=dev)
        qt = torch.empty((K, ROTS, 4), dtype=torch.float32, device=dev) if quat else None
        flags = torch.empty(K, dtype=torch.uint8, device=dev)
        _lib.check(lib.tip_pose_rows(st.data_ptr(), root.data_ptr(), rows.data_ptr(), 54, in_off.data_ptr(), int(rows.shape[0]),
                                     t_out.data_ptr(), out_off.data_ptr(), K, len(lens), delay, hold, far, baseline, mode_c, depth,
                                     q.data_ptr(), None if qt is None else qt.data_ptr(), flags.data_ptr(), _lib.current_stream(dev)))
    recs, fl = _sn._recordings(q, flags, out_lens, host, True)
    if not quat:
        return recs, fl
    qs = _sn._split(qt, out_lens)
    return recs, fl, ([x.cpu().numpy() for x in qs] if host else qs)
