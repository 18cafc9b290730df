"""Sensor front end: raw IMU packets and the per-slot calibration on the device, in front of the streaming engines.

The reference's live demo does this arithmetic on the host between its socket reader and RTRunner.step
(live_demo_new.py): a packet of 6 sensors x (quaternion, sensor-frame acceleration) becomes 6 rotation matrices and 6
accelerations (:97-112); two holds of a few seconds calibrate a wearer — the heading reset (:150-158, :221-226: R_Gn_Gp, acc_offset)
and the T-pose (:243-248, :52-62: R_B0_S0); and every frame is then put into the room frame and onto the bones (:161-175), which is
the 72-column frame `step(raw)` takes.  Here the tables live in HBM, one block per slot, and one launch per frame writes the engine's
`raw` (csrc/tip_sensor.hip; include/tip_hip.h, "sensor front end").

    front = SensorFrontEnd(n, "cuda")
    front.begin_heading([i]); front.accumulate(packets) ...; front.finish([i])       # hold 1: sensors aligned with the body frame
    front.begin_tpose([i]);   front.accumulate(packets) ...; front.finish([i])       # hold 2: worn, standing in T-pose
    out = engine.step_packets(front, packets)                                        # packets [n,42] -> raw on the device -> the frame
    saved = front.tables([i]); other.load([i], saved)                                # a calibration kept and put back without the holds
    front = SensorFrontEnd(n, "cuda", fill=True)                                     # a sensor that delivers nothing: the mean of its last rows

packets is [n, 42] float32, per sensor q0 q1 q2 q3 ax ay az, the quaternion read as (x, y, z, w): what the demo hands to fairmotion's
Q2R, i.e. scipy's Rotation.from_quat(q).as_matrix() (fairmotion itself is unpinned, as for A2R / R2A).  accumulate() takes the whole
pool's packets and only the slots that are in a hold use theirs, so one wearer calibrates between the frames of the others.  Phases
change through these calls only, so the host's copy of them (PhaseMirror) is exact and nothing here reads the device or synchronises.

Missing readings (csrc/tip_fill.hip; include/tip_hip.h, "missing IMU readings"): the reference fills them when it prepares the real
recordings (preprocess_DIP_TC_new.py:112-136, :160-180).  real_imu_frames is that preparation on the device (rule R, fp64, what
tip_amd.data.combine_motions takes as "imu"); SensorFrontEnd(fill=True) is its live form (rule V: a ring of the last five rows after
filling, per sensor and part), one launch behind the transform; fill_sequences and transform_sequences do the same to recorded frames
and recorded packet sessions, frame for frame what the live front end gives, as recordings for tip_amd.replay.ReplayPool.

Timestamped packets (csrc/tip_resample.hip; include/tip_hip.h, "timestamped packets"): everything above takes one packet per slot per
60 Hz frame, all wearers in step.  The demo gets there with a zero-order hold for its one wearer (live_demo_new.py:82-115, :161-162).
PacketResampler is that for a pool, on the device: packets arrive with fp64 stamps at whatever rate each wearer's sensors send,
emit(t) gives every slot its packet at the tick — held, or interpolated between the two packets around t - delay — and the result
is the [n, 42] every method above and every engine's step_packets take; resample_sequences is the same for recorded sessions.

    rs = PacketResampler(n, "cuda", mode="slerp", delay=1 / 100, max_hold=0.1)      # 100 Hz sensors: one period of delay
    rs.push(packets, slots, times)                                                  # whatever arrived since the last tick
    out = engine.step_packets(front, rs.emit(t))                                    # t: the tick, a number or [n]; rs.flags says how

Clock sync and predicted ticks (csrc/tip_clock.hip; include/tip_hip.h, "clock sync and predicted ticks"): a hub stamps its packets
with a clock of its own, and the server knows only when they arrive.  ClockSync keeps per slot the offset between the two as a lower
envelope of arrival - stamp; push(..., arrivals=, sync=) maps and inserts in one launch; mode "predict" continues the orientation past
the newest packet at the rate of the newest two, so that delay 0 gives a packet AT the tick; sync_sequences and
resample_sequences(mode="predict") are the same for recorded sessions.

    clk = ClockSync(n, "cuda")
    rs = PacketResampler(n, "cuda", mode="predict", delay=0.0, max_hold=0.1)        # max_predict: 25 ms unless given
    rs.push(packets, slots, sensor_stamps, arrivals=arrival_times, sync=clk)        # stamps on each hub's clock, arrivals on the server's
    out = engine.step_packets(front, rs.emit(t))
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import lib as _lib
from .streaming import slot_list

UNCALIBRATED, HEADING, HEADING_DONE, TPOSE, LIVE = range(5)      # the phase word of a calibration block (include/tip_hip.h)
PACKET, TABLE = 42, 126
# the demo's aligned T-pose (front x, left y, up z; live_demo_new.py:52-62), what finish() uses when no r_gp_b0 is given: the exact
# form of A2R([0, 0, pi / 2]) @ [[1,0,0],[0,0,-1],[0,1,0]], whose fp64 product carries 2e-16 residues of cos(pi / 2)
ALIGNED_T_POSE = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
# preprocess_DIP_TC_new.py: the six sensors the model reads (root, left wrist, right wrist, left knee, right knee, head; :166) among
# DIP-IMU's 17, and the same six among TotalCapture's own (its scatter into 17 slots, :89-90, followed by that selection)
SEL_DIP17 = (2, 7, 8, 11, 12, 0)
SEL_TC6 = (5, 2, 3, 0, 1, 4)
# ROT_MAT_OURS of the two corpora: Q2R((.5, .5, .5, .5)) in its exact form, and A2R((pi / 2, 0, 0)) as scipy gives it (tests pin both)
ROT_DIP = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
_C90 = 2.220446049250313e-16                                     # scipy's cos(pi / 2) in from_rotvec([pi / 2, 0, 0]).as_matrix()
ROT_TC = np.array([[1.0, 0.0, 0.0], [0.0, _C90, -1.0], [0.0, 1.0, _C90]])
PARTS = 12                                                       # of a row: the rotation of sensor k (k < 6), the acceleration of sensor k - 6


def _max_gap_arg(max_gap, who):
    """max_gap as the C ABI takes it: None -> -1 (no limit), else an int >= 0."""
    if max_gap is None:
        return -1
    if isinstance(max_gap, bool) or not isinstance(max_gap, (int, np.integer)) or max_gap < 0:
        raise ValueError(f"tip_amd.{who}: max_gap is None (no limit) or a number of consecutive fills >= 0; got {max_gap!r}")
    return int(max_gap)


class PhaseMirror:
    """The phases of n calibration blocks as the device holds them (host only, no GPU): the transitions of tip_sensor_begin / finish /
    set, with a refusal where the device would leave the block untouched.  A call checks every listed slot before it changes any."""

    def __init__(self, n: int):
        self.n = int(n)
        self.phase = [UNCALIBRATED] * self.n

    def begin_heading(self, idx):
        for i in idx:
            if self.phase[i] in (HEADING, TPOSE):
                raise RuntimeError(f"tip_amd.SensorFrontEnd.begin_heading: slot {i} is in a hold (finish() it first)")
        for i in idx:
            self.phase[i] = HEADING

    def begin_tpose(self, idx):
        for i in idx:
            if self.phase[i] != HEADING_DONE:
                raise RuntimeError(f"tip_amd.SensorFrontEnd.begin_tpose: slot {i} has no finished heading (begin_heading, accumulate, "
                                   "finish come first; a live slot starts over at its heading)")
        for i in idx:
            self.phase[i] = TPOSE

    def finish(self, idx):
        for i in idx:
            if self.phase[i] not in (HEADING, TPOSE):
                raise RuntimeError(f"tip_amd.SensorFrontEnd.finish: slot {i} is not accumulating (begin_heading or begin_tpose first)")
        for i in idx:
            self.phase[i] = HEADING_DONE if self.phase[i] == HEADING else LIVE

    def load(self, idx):
        for i in idx:
            self.phase[i] = LIVE

    def live(self, idx=None):
        return np.array([self.phase[i] == LIVE for i in (range(self.n) if idx is None else idx)], dtype=bool)


class SensorFrontEnd:
    """n calibration blocks and a packet buffer [n, 42] on `device`.  max_acc: the clip of the room-frame acceleration (the demo's
    MAX_ACC).  r_gp_b0: the bone orientations of the T-pose, [6, 3, 3] or [6, 9] (kept as fp64); None is the demo's aligned T-pose,
    [[0,0,1],[1,0,0],[0,1,0]] for all six sensors.  Every call is launches and non-blocking copies on the current stream.

    fill=True: a sensor part (9 rotation or 3 acceleration columns) that comes out of the transform with a NaN becomes the mean of the
    slot's last five rows of that part after filling (rule V of include/tip_hip.h), one tip_fill_live launch behind the transform;
    `filled` [n, 12] uint8 says what happened to the last frame (0 good, 1 filled, 2 left NaN: nothing to fill from, or max_gap
    consecutive fills already made; max_gap=None is no limit, as the reference has none).  The rings of a slot are emptied whenever it
    is calibrated anew (finish, load, begin_heading) — a new wearer never inherits another's readings — and by fill_reset."""

    def __init__(self, n: int, device, max_acc: float = 10.0, r_gp_b0=None, *, fill: bool = False, max_gap=None):
        self.n = int(n)
        if self.n < 1:
            raise ValueError(f"tip_amd.SensorFrontEnd: n is the number of slots, at least 1; got {n!r}")
        self.max_acc = float(max_acc)
        if not self.max_acc >= 0.0:
            raise ValueError(f"tip_amd.SensorFrontEnd: max_acc is the acceleration clip, a number >= 0; got {max_acc!r}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("tip_amd.SensorFrontEnd runs on an MI355X: give it the engine's device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.load()
        self.mirror = PhaseMirror(self.n)
        nbytes = ctypes.c_size_t()
        _lib.check(self.lib.tip_sensor_state_bytes(self.n, ctypes.byref(nbytes)))
        self.cal = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        self.packets = torch.zeros((self.n, PACKET), dtype=torch.float32, device=self.device)
        self.r_gp_b0 = None
        if r_gp_b0 is not None:
            r = torch.as_tensor(r_gp_b0, dtype=torch.float64)
            if r.numel() != 54:
                raise ValueError(f"tip_amd.SensorFrontEnd: r_gp_b0 is [6, 3, 3] or [6, 9]; got {tuple(r.shape)}")
            self.r_gp_b0 = self._to_dev(r.reshape(6, 9).contiguous())
        self.fill = bool(fill)
        self.max_gap = _max_gap_arg(max_gap, "SensorFrontEnd")
        if self.max_gap >= 0 and not self.fill:
            raise ValueError("tip_amd.SensorFrontEnd: max_gap limits the fill; give it with fill=True")
        self.fill_state = self.filled = None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.tip_sensor_reset(self.cal.data_ptr(), self.n, self._stream()))
            if self.fill:
                _lib.check(self.lib.tip_fill_state_bytes(self.n, ctypes.byref(nbytes)))
                self.fill_state = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
                self.filled = torch.zeros((self.n, PARTS), dtype=torch.uint8, device=self.device)
                _lib.check(self.lib.tip_fill_reset(self.fill_state.data_ptr(), self.n, None, 0, self._stream()))

    def _stream(self):
        return _lib.current_stream(self.device)

    def _to_dev(self, t):
        """The engines' rule: host -> device without a synchronising copy from pageable memory."""
        return t.to(self.device, non_blocking=True) if t.is_cuda else t.pin_memory().to(self.device, non_blocking=True)

    def _slots(self, slots, who):
        return list(range(self.n)) if slots is None else slot_list(slots, self.n, f"SensorFrontEnd.{who}")

    def _fill(self, packets, who):
        """packets -> the packet buffer (one non-blocking copy); a wrong shape is a ValueError in `who`'s name."""
        p = torch.as_tensor(packets, dtype=torch.float32)
        if tuple(p.shape) != (self.n, PACKET):
            raise ValueError(f"tip_amd.{who}: packets is [{self.n}, {PACKET}] (per sensor q0 q1 q2 q3 ax ay az, the "
                             f"quaternion as x, y, z, w); got {tuple(p.shape)}")
        self.packets.copy_(p if p.is_cuda else p.contiguous().pin_memory(), non_blocking=True)

    def _transform_into(self, raw):
        """One tip_sensor_transform launch: the packet buffer -> raw [n, 72] (a CUDA float32 tensor of this device, contiguous); with
        fill=True one tip_fill_live launch behind it, in place on raw."""
        with torch.cuda.device(self.device):
            _lib.check(self.lib.tip_sensor_transform(self.cal.data_ptr(), self.packets.data_ptr(), self.n, self.max_acc, raw.data_ptr(),
                                                      self._stream()))
            if self.fill:
                _lib.check(self.lib.tip_fill_live(self.fill_state.data_ptr(), self.cal.data_ptr(), raw.data_ptr(), self.n, self.max_gap,
                                                   self.filled.data_ptr(), self._stream()))

    # ---- missing readings (fill=True) ------------------------------------------------------------------------------------------------
    def _fill_reset(self, idx):
        """The rings of the listed slots start empty (nothing without fill=True)."""
        if not self.fill or not idx:
            return
        with torch.cuda.device(self.device):
            sl = self._to_dev(torch.tensor(idx, dtype=torch.int32))
            _lib.check(self.lib.tip_fill_reset(self.fill_state.data_ptr(), self.n, sl.data_ptr(), len(idx), self._stream()))

    def _needs_fill(self, who):
        if not self.fill:
            raise RuntimeError(f"tip_amd.SensorFrontEnd.{who}: this front end was built without fill=True")

    def fill_reset(self, slots=None):
        """Empty the rings and zero the counters of the listed slots (None: all)."""
        self._needs_fill("fill_reset")
        self._fill_reset(self._slots(slots, "fill_reset"))

    def fill_counts(self, slots=None):
        """(have, run, total) of the listed slots (None: all), three CUDA int32 tensors [len(slots), 12]: rows in the ring (0 .. 5),
        consecutive fills up to the last frame, fills since the rings were emptied."""
        self._needs_fill("fill_counts")
        idx = self._slots(slots, "fill_counts")
        out = torch.zeros((len(idx), 3, PARTS), dtype=torch.int32, device=self.device)
        if idx:
            with torch.cuda.device(self.device):
                sl = self._to_dev(torch.tensor(idx, dtype=torch.int32))
                _lib.check(self.lib.tip_fill_get(self.fill_state.data_ptr(), self.n, sl.data_ptr(), len(idx), out.data_ptr(), self._stream()))
        return out[:, 0], out[:, 1], out[:, 2]

    # ---- the two holds ---------------------------------------------------------------------------------------------------------------
    def _begin(self, idx, which):
        if not idx:
            return
        with torch.cuda.device(self.device):
            sl = self._to_dev(torch.tensor(idx, dtype=torch.int32))
            _lib.check(self.lib.tip_sensor_begin(self.cal.data_ptr(), self.n, sl.data_ptr(), len(idx), which, self._stream()))

    def begin_heading(self, slots=None):
        """Start the heading hold of the listed slots (None: all): sensors lying aligned with the body reference frame
        (live_demo_new.py:217-226).  From uncalibrated, from a finished heading, or from live (a re-calibration)."""
        idx = self._slots(slots, "begin_heading")
        self.mirror.begin_heading(idx)
        self._begin(idx, _lib.TIP_SENSOR_HEADING)
        self._fill_reset(idx)

    def begin_tpose(self, slots=None):
        """Start the T-pose hold of the listed slots (live_demo_new.py:236-248); each needs a finished heading."""
        idx = self._slots(slots, "begin_tpose")
        self.mirror.begin_tpose(idx)
        self._begin(idx, _lib.TIP_SENSOR_TPOSE)

    def accumulate(self, packets):
        """One reading of a hold (the demo's get_mean_readings_3_sec takes 181): every slot in a hold adds its packet to its sums; the
        packets of the other slots are ignored and their blocks are not written."""
        self._fill(packets, "SensorFrontEnd.accumulate")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.tip_sensor_accumulate(self.cal.data_ptr(), self.packets.data_ptr(), self.n, self._stream()))

    def finish(self, slots=None):
        """End the hold of the listed slots (None: every slot that is in one): a heading hold leaves R_Gn_Gp (the mean matrices as they
        are) and acc_offset, a T-pose hold R_B0_S0 and a live slot.  A hold without a reading leaves NaN tables (and NaN rows)."""
        if slots is None:
            idx = [i for i in range(self.n) if self.mirror.phase[i] in (HEADING, TPOSE)]
        else:
            idx = self._slots(slots, "finish")
        self.mirror.finish(idx)
        if not idx:
            return
        with torch.cuda.device(self.device):
            sl = self._to_dev(torch.tensor(idx, dtype=torch.int32))
            r = self.r_gp_b0.data_ptr() if self.r_gp_b0 is not None else None
            _lib.check(self.lib.tip_sensor_finish(self.cal.data_ptr(), self.n, sl.data_ptr(), len(idx), r, self._stream()))
        self._fill_reset(idx)

    # ---- saved calibrations ----------------------------------------------------------------------------------------------------------
    def load(self, slots, tables):
        """Put saved tables [len(slots), 126] (R_Gn_Gp 54 | acc_offset 18 | R_B0_S0 54) into the listed slots; they are live at once."""
        idx = self._slots(slots, "load")
        t = torch.as_tensor(tables, dtype=torch.float32)
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if tuple(t.shape) != (len(idx), TABLE):
            raise ValueError(f"tip_amd.SensorFrontEnd.load: tables is [len(slots), {TABLE}]; got {tuple(t.shape)} for {len(idx)} slots")
        self.mirror.load(idx)
        if not idx:
            return
        with torch.cuda.device(self.device):
            sl = self._to_dev(torch.tensor(idx, dtype=torch.int32))
            t = self._to_dev(t.contiguous()).contiguous()
            _lib.check(self.lib.tip_sensor_set(self.cal.data_ptr(), self.n, sl.data_ptr(), len(idx), t.data_ptr(), self._stream()))
        self._fill_reset(idx)

    def tables(self, slots=None):
        """The tables of the listed slots (None: all) as a CUDA tensor [len(slots), 126], whatever their phase."""
        idx = self._slots(slots, "tables")
        out = torch.empty((len(idx), TABLE), dtype=torch.float32, device=self.device)
        if idx:
            with torch.cuda.device(self.device):
                sl = self._to_dev(torch.tensor(idx, dtype=torch.int32))
                _lib.check(self.lib.tip_sensor_get(self.cal.data_ptr(), self.n, sl.data_ptr(), len(idx), out.data_ptr(), self._stream()))
        return out

    def live(self, slots=None):
        """bool [len(slots)] (numpy; None: all n): the slot's calibration is finished or loaded — transform gives it finite rows."""
        return self.mirror.live(None if slots is None else self._slots(slots, "live"))

    # ---- wearer hand-over (tip_amd.handover) -----------------------------------------------------------------------------------------
    def export_slots(self, slots):
        """The listed slots' calibrations as they stand — a hold in progress included: its fp64 sums, count and phase are in the block —
        with their PhaseMirror entries and, with fill=True, their fill rings: a dict of device tensors plus `meta` (tip_amd.handover).
        One launch per buffer on the current stream, no synchronisation."""
        from . import handover
        return handover.export_front(self, slots)

    def import_slots(self, slots, exported):
        """Put exported calibrations into the listed slots, whatever those held; both front ends must agree on `fill` (ValueError
        otherwise, before anything is launched).  A hold in progress goes on where it was: accumulate() and finish() on this object."""
        from . import handover
        handover.import_front(self, slots, exported)

    # ---- the per-frame launch --------------------------------------------------------------------------------------------------------
    def transform(self, packets, out=None):
        """packets [n, 42] -> the calibrated frame [n, 72] the engines' step() takes (54 rotation columns, 18 acceleration columns), into
        `out` (a contiguous CUDA float32 [n, 72] of this device) or a new tensor.  A slot that is not live gets a NaN row; a sensor
        whose quaternion is zero or not finite gets NaN in its own 12 columns."""
        if out is None:
            out = torch.empty((self.n, 72), dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
              or tuple(out.shape) != (self.n, 72) or not out.is_contiguous()):
            raise ValueError(f"tip_amd.SensorFrontEnd.transform: out is a contiguous float32 [{self.n}, 72] tensor on {self.device}")
        self._fill(packets, "SensorFrontEnd.transform")
        self._transform_into(out)
        return out


# ---- recorded data: the real-IMU files, recorded frames with gaps, recorded packet sessions ------------------------------------------
def _device_of(arrays, device):
    if device is not None:
        dev = torch.device(device)
    else:
        dev = next((a.device for a in arrays if isinstance(a, torch.Tensor) and a.is_cuda), torch.device("cuda"))
    if dev.type != "cuda":
        raise RuntimeError("tip_amd.sensors: the fill kernels run on an MI355X; give a CUDA device")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _to(t, dev):
    return t.to(dev, non_blocking=True) if t.is_cuda else t.contiguous().pin_memory().to(dev, non_blocking=True)


def _stack(arrays, dtype, width, dev, who, what):
    """A list of [L_i, ...] arrays whose rows have `width` values -> (one contiguous [N, width] tensor on dev, int64 offsets [R + 1] on
    dev, the lengths)."""
    parts, lens = [], []
    for i, a in enumerate(arrays):
        t = torch.as_tensor(a)
        if t.dim() < 2 or t.numel() != t.shape[0] * width:
            raise ValueError(f"tip_amd.sensors.{who}: {what}[{i}] is [L, {width}] (or that many values per row); got {tuple(t.shape)}")
        parts.append(_to(t.to(dtype).reshape(t.shape[0], width), dev))
        lens.append(int(t.shape[0]))
    if not parts:
        raise ValueError(f"tip_amd.sensors.{who}: no sequences")
    cat = torch.cat(parts, dim=0).contiguous() if len(parts) > 1 else parts[0].contiguous()
    offs = _to(torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int64), dev)
    return cat, offs, lens


def _split(t, lens):
    out, at = [], 0
    for n in lens:
        out.append(t[at:at + n])
        at += n
    return out


def real_imu_frames(ori_list, acc_list, rot, sel=SEL_DIP17, strict=True, device=None):
    """The reference's preparation of real recordings (preprocess_DIP_TC_new.py: get_real_imu_readings_ours_format_knee over
    fill_in_nan_values) for R recordings in one launch: ori_list[i] [L_i, S, 3, 3] and acc_list[i] [L_i, S, 3] (numpy or tensors, read as
    fp64; S = 17 for DIP-IMU, 6 for TotalCapture as it is stored), `sel` the six sensors taken (SEL_DIP17, SEL_TC6), `rot` the corpus'
    rotation (ROT_DIP, ROT_TC).  Returns a list of CUDA fp64 [L_i, 72] (views of one tensor): what tip_amd.data.combine_motions takes
    as files[i]["imu"], in place.  A recording in which a part is still NaN afterwards (a sensor without one reading in rows 0 .. 9) is
    a ValueError naming it, where the reference asserts; strict=False returns it with its NaNs and does not synchronise."""
    who = "real_imu_frames"
    if len(ori_list) != len(acc_list):
        raise ValueError(f"tip_amd.sensors.{who}: {len(ori_list)} orientation arrays for {len(acc_list)} acceleration arrays")
    sel = [int(v) for v in sel]
    rot = np.ascontiguousarray(rot, dtype=np.float64)
    if len(sel) != 6 or rot.shape != (3, 3):
        raise ValueError(f"tip_amd.sensors.{who}: sel is six sensor indices and rot a 3x3 matrix")
    if not len(ori_list):
        raise ValueError(f"tip_amd.sensors.{who}: no sequences")
    shape = tuple(torch.as_tensor(ori_list[0]).shape)
    S = int(shape[1]) if len(shape) >= 3 else 0
    if S < 1 or min(sel) < 0 or max(sel) >= S:
        raise ValueError(f"tip_amd.sensors.{who}: ori_list[i] is [L, S, 3, 3] and sel picks six of the S sensors; got {shape} and {sel}")
    dev = _device_of(list(ori_list) + list(acc_list), device)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ori, offs, lens = _stack(ori_list, torch.float64, S * 9, dev, who, "ori_list")
        acc, _, lens_a = _stack(acc_list, torch.float64, S * 3, dev, who, "acc_list")
        if lens != lens_a:
            raise ValueError(f"tip_amd.sensors.{who}: orientation and acceleration lengths differ: {lens} and {lens_a}")
        N, R = int(ori.shape[0]), len(lens)
        out = torch.empty((N, 72), dtype=torch.float64, device=dev)
        unfilled = torch.zeros(R, dtype=torch.int32, device=dev)
        _lib.check(lib.tip_fill_real(ori.data_ptr(), acc.data_ptr(), N, S, offs.data_ptr(), R, (ctypes.c_int * 6)(*sel),
                                       (ctypes.c_double * 9)(*rot.reshape(-1)), out.data_ptr(), unfilled.data_ptr(),
                                       _lib.current_stream(dev)))
        if strict:
            left = unfilled.cpu().numpy()
            if left.any():
                bad = [f"{i} ({int(left[i])} parts)" for i in np.flatnonzero(left)]
                raise ValueError(f"tip_amd.sensors.{who}: sequences {', '.join(bad)} keep NaN readings after the fill (a sensor without "
                                 "one reading in the rows it is filled from); strict=False returns them as they are")
    return _split(out, lens)


def fill_sequences(frames_list, rule="live", max_gap=None, device=None, host=False, return_flags=False):
    """Recorded frames with gaps -> recordings: frames_list[i] is [L_i, 72] float32 (54 rotation columns, 18 acceleration columns, NaN
    where a sensor delivered nothing); every sequence is filled as SensorFrontEnd(fill=True, max_gap=max_gap) fills a stream that
    starts with empty rings, bit for bit, all of them in one launch.  Returns a list of CUDA float32 [L_i, 72]; host=True: numpy
    arrays, as ReplayPool.run takes them; return_flags=True: (recordings, flags), flags[i] uint8 [L_i, 12] as SensorFrontEnd.filled.
    rule="live" is the only rule for frames: the reference's own rule looks ahead and is real_imu_frames' (fp64, whole files)."""
    who = "fill_sequences"
    if rule != "live":
        raise ValueError(f"tip_amd.sensors.{who}: rule is \"live\" (the reference's look-ahead rule is real_imu_frames'); got {rule!r}")
    gap = _max_gap_arg(max_gap, who)
    dev = _device_of(list(frames_list), device)
    lib = _lib.load()
    with torch.cuda.device(dev):
        frames, offs, lens = _stack(frames_list, torch.float32, 72, dev, who, "frames_list")
        out = torch.empty_like(frames)
        flags = torch.zeros((frames.shape[0], PARTS), dtype=torch.uint8, device=dev)
        _lib.check(lib.tip_fill_rows(frames.data_ptr(), out.data_ptr(), int(frames.shape[0]), offs.data_ptr(), len(lens), gap,
                                       flags.data_ptr(), _lib.current_stream(dev)))
    return _recordings(out, flags, lens, host, return_flags)


def _recordings(out, flags, lens, host, return_flags):
    recs = _split(out, lens)
    if host:
        recs = [r.cpu().numpy() for r in recs]
    if not return_flags:
        return recs
    fl = _split(flags, lens)
    return recs, ([f.cpu().numpy() for f in fl] if host else fl)


def transform_sequences(packets_list, tables, fill=False, max_acc=10.0, max_gap=None, device=None, host=False, return_flags=False):
    """Recorded packet sessions -> recordings: packets_list[i] is [L_i, 42] float32 (SensorFrontEnd's packet layout), tables [R, 126]
    the wearers' calibrations (SensorFrontEnd.tables).  Every row goes through tip_sensor_transform's arithmetic (one row-parallel
    launch, bit for bit what SensorFrontEnd.transform gives frame by frame) and, with fill=True, through fill_sequences' launch in
    place.  Returns as fill_sequences does."""
    who = "transform_sequences"
    gap = _max_gap_arg(max_gap, who)
    if gap >= 0 and not fill:
        raise ValueError(f"tip_amd.sensors.{who}: max_gap limits the fill; give it with fill=True")
    max_acc = float(max_acc)
    if not max_acc >= 0.0:
        raise ValueError(f"tip_amd.sensors.{who}: max_acc is the acceleration clip, a number >= 0; got {max_acc!r}")
    dev = _device_of(list(packets_list) + [tables], device)
    lib = _lib.load()
    with torch.cuda.device(dev):
        packets, offs, lens = _stack(packets_list, torch.float32, PACKET, dev, who, "packets_list")
        t = torch.as_tensor(tables, dtype=torch.float32)
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if tuple(t.shape) != (len(lens), TABLE):
            raise ValueError(f"tip_amd.sensors.{who}: tables is [{len(lens)}, {TABLE}], one per session; got {tuple(t.shape)}")
        t = _to(t, dev).contiguous()
        N = int(packets.shape[0])
        out = torch.empty((N, 72), dtype=torch.float32, device=dev)
        flags = torch.zeros((N, PARTS), dtype=torch.uint8, device=dev)
        stream = _lib.current_stream(dev)
        _lib.check(lib.tip_fill_packets(t.data_ptr(), packets.data_ptr(), N, offs.data_ptr(), len(lens), max_acc, out.data_ptr(), stream))
        if fill:
            _lib.check(lib.tip_fill_rows(out.data_ptr(), out.data_ptr(), N, offs.data_ptr(), len(lens), gap, flags.data_ptr(), stream))
    return _recordings(out, flags, lens, host, return_flags)


# ---- timestamped packets: every wearer resampled to the tick grid ----------------------------------------------------------------------
MODES = {"hold": _lib.TIP_RESAMPLE_HOLD, "slerp": _lib.TIP_RESAMPLE_SLERP, "predict": 2}
# what emit says about a slot's row: interpolated; a packet held (copied bit for bit); NaN because the packet to hold is older than
# max_hold; NaN because the ring is empty; NaN because t - delay is before the ring's oldest packet; continued past the newest packet
# at the rate of the newest two (mode "predict" only)
INTERPOLATED, HELD, STALE, EMPTY, EARLY = range(5)
PREDICTED = _lib.TIP_RESAMPLE_PREDICTED
MAX_PREDICT = 0.025                                              # mode "predict" without a max_predict: a tick and a half


def _resample_rule(mode, delay, max_hold, depth, who):
    """(mode, delay, max_hold, depth) as the C ABI takes them; anything else is a ValueError in `who`'s name."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"tip_amd.sensors.{who}: mode is \"slerp\", \"hold\" or \"predict\"; got {mode!r}")
    try:
        delay = float(delay)
    except (TypeError, ValueError):
        delay = float("nan")
    if not (delay >= 0.0 and np.isfinite(delay)):
        raise ValueError(f"tip_amd.sensors.{who}: delay is the age of the emitted packet in seconds, a finite number >= 0 (a row past "
                         f"the newest packet is mode \"predict\"'s with max_predict, never a negative delay); got {delay!r}")
    if max_hold is None:
        hold = -1.0
    else:
        try:
            hold = float(max_hold)
        except (TypeError, ValueError):
            hold = float("nan")
        if not hold >= 0.0:
            raise ValueError(f"tip_amd.sensors.{who}: max_hold is None (no limit) or the oldest packet that may be held, in seconds "
                             f">= 0; got {max_hold!r}")
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or not 2 <= depth <= 64:
        raise ValueError(f"tip_amd.sensors.{who}: depth is the number of packets a slot keeps, an int in 2 .. 64; got {depth!r}")
    return MODES[mode], delay, hold, int(depth)


def _predict_rule(mode, max_predict, who):
    """max_predict as the C ABI takes it: MAX_PREDICT when mode "predict" names none; a ValueError with any other mode."""
    if mode != "predict":
        if max_predict is not None:
            raise ValueError(f"tip_amd.sensors.{who}: max_predict is mode \"predict\"'s; mode {mode!r} predicts nothing")
        return 0.0
    if max_predict is None:
        return MAX_PREDICT
    try:
        far = float(max_predict)
    except (TypeError, ValueError):
        far = float("nan")
    if not (far >= 0.0 and np.isfinite(far)):
        raise ValueError(f"tip_amd.sensors.{who}: max_predict is how far past the newest packet a row may be predicted, a finite "
                         f"number of seconds >= 0; got {max_predict!r}")
    return far


def _clock_rule(leak, slew, who):
    """(leak, slew) of the clock rule as floats; anything else is a ValueError in `who`'s name."""
    def number(v):
        try:
            return float(v)
        except (TypeError, ValueError):
            return float("nan")
    lk, sl = number(leak), number(slew)
    if not (lk >= 0.0 and np.isfinite(lk)):
        raise ValueError(f"tip_amd.sensors.{who}: leak is the fastest drift the offset may follow upwards, a finite number of seconds "
                         f"per second >= 0; got {leak!r}")
    if not 0.0 <= sl < 1.0:
        raise ValueError(f"tip_amd.sensors.{who}: slew is the share of a stamp interval the offset may fall by, in [0, 1); got {slew!r}")
    return lk, sl


def tick_times(t0, count, rate_hz=60.0):
    """The tick grid: float64 [count], t0 + k * (1.0 / rate_hz) — a product, not a running sum, so tick k is the same number wherever
    it is computed."""
    if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or count < 0:
        raise ValueError(f"tip_amd.sensors.tick_times: count is a number of ticks >= 0; got {count!r}")
    rate, t0 = float(rate_hz), float(t0)
    if not (rate > 0.0 and np.isfinite(rate)) or not np.isfinite(t0):
        raise ValueError(f"tip_amd.sensors.tick_times: t0 is finite and rate_hz a finite number > 0; got {t0!r}, {rate_hz!r}")
    return t0 + np.arange(int(count), dtype=np.float64) * (1.0 / rate)


def _times_f64(t, what):
    """Stamps or query times as a float64 tensor.  Anything that is no tensor goes through numpy as float64 (torch reads a list of
    Python floats as float32: 1.7e9 + 0.123 would become 1.7e9); a tensor must be float64 or of an integer type."""
    if not isinstance(t, torch.Tensor):
        if isinstance(t, (np.ndarray, np.generic)) and t.dtype.kind == "f" and t.dtype.itemsize < 8:
            raise ValueError(f"{what} are float64 seconds; a {t.dtype} array has already lost them (1.7e9 s in float32 resolves 128 s)")
        try:
            return torch.from_numpy(np.asarray(t, dtype=np.float64, order="C"))
        except (TypeError, ValueError):
            raise ValueError(f"{what} are seconds, numbers read as float64; got {type(t).__name__}") from None
    if t.dtype == torch.float64:
        return t
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise ValueError(f"{what} are float64 seconds; a {t.dtype} tensor has already lost them (1.7e9 s in float32 resolves 128 s)")
    return t.to(torch.float64)


def _tick_rule(rate_hz, delay, who):
    """(rate_hz, delay) of a tick grid as floats; anything else is a ValueError in `who`'s name."""
    try:
        rate, delay = float(rate_hz), float(delay)
    except (TypeError, ValueError):
        rate, delay = float("nan"), float("nan")
    if not (rate > 0.0 and np.isfinite(rate)):
        raise ValueError(f"tip_amd.sensors.{who}: rate_hz is the tick rate, a finite number > 0; got {rate_hz!r}")
    if not (delay >= 0.0 and np.isfinite(delay)):
        raise ValueError(f"tip_amd.sensors.{who}: delay is a finite number of seconds >= 0; got {delay!r}")
    return rate, delay


def _pinned_image(parts, device):
    """Host tensors [(tensor, dtype)], each flat -> their device copies, sent up as ONE pinned image in ONE non-blocking copy.  The
    parts are laid out in the order given: put the widest type first and every part stays aligned to its type."""
    sizes = [int(t.numel()) * torch.empty((), dtype=d).element_size() for t, d in parts]
    image = torch.empty(sum(sizes), dtype=torch.uint8).pin_memory()
    at = 0
    for (t, d), nb in zip(parts, sizes):
        image[at: at + nb].view(d).copy_(t.reshape(-1))
        at += nb
    dev, out, at = image.to(device, non_blocking=True), [], 0
    for (t, d), nb in zip(parts, sizes):
        out.append(dev[at: at + nb].view(d))
        at += nb
    return out


class ClockSync:
    """n clock blocks on `device` (csrc/tip_clock.hip; include/tip_hip.h, "clock sync and predicted ticks"): per slot the offset
    between a hub's own clock, which stamps the packets, and the server's, which only sees them arrive.  The estimate is a lower
    envelope of arrival - stamp: it rises by at most `leak` seconds per second of stamps (a crystal's drift) and falls by at most `slew`
    of a stamp interval, so that mapped times are strictly increasing.  map() gives the stamps on the server's clock, which is what
    PacketResampler.push takes as times; push(..., arrivals=, sync=) does both in one launch.  No call synchronises."""

    def __init__(self, n: int, device, *, leak: float = _lib.TIP_CLOCK_LEAK, slew: float = _lib.TIP_CLOCK_SLEW):
        who = "ClockSync"
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"tip_amd.sensors.{who}: n is the number of slots, at least 1; got {n!r}")
        self.n = int(n)
        self.leak, self.slew = _clock_rule(leak, slew, who)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("tip_amd.sensors.ClockSync runs on an MI355X: give it the engine's device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.load()
        nbytes = ctypes.c_size_t()
        _lib.check(self.lib.tip_clock_state_bytes(self.n, ctypes.byref(nbytes)))
        self.state = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.tip_clock_reset(self.state.data_ptr(), self.n, None, 0, self._stream()))

    def _stream(self):
        return _lib.current_stream(self.device)

    def _slots(self, slots, who):
        return list(range(self.n)) if slots is None else slot_list(slots, self.n, f"sensors.ClockSync.{who}")

    def map(self, slots, stamps, arrivals):
        """m arrivals: slots [m], stamps [m] (the sensor's clock) and arrivals [m] (the server's), float64 seconds read as
        PacketResampler.push reads its times -> the stamps on the server's clock, a CUDA float64 [m].  The arrivals of one slot are
        taken in array order; one whose stamp or arrival time is not finite, or whose stamp is not above the slot's last, is counted
        as rejected and maps to NaN, as does an arrival for a slot outside [0, n).  Host inputs go up in ONE non-blocking copy."""
        who = "tip_amd.sensors.ClockSync.map"
        sl, st, ar = torch.as_tensor(slots), _times_f64(stamps, f"{who}: stamps"), _times_f64(arrivals, f"{who}: arrivals")
        m = int(sl.numel())
        if sl.dim() != 1 or tuple(st.shape) != (m,) or tuple(ar.shape) != (m,):
            raise ValueError(f"{who}: slots, stamps and arrivals are [m]; got {tuple(sl.shape)}, {tuple(st.shape)}, {tuple(ar.shape)}")
        if m and (sl.dtype.is_floating_point or sl.dtype == torch.bool):
            raise ValueError(f"{who}: slots are integers; got {sl.dtype}")
        out = torch.full((m,), float("nan"), dtype=torch.float64, device=self.device)
        if m == 0:
            return out
        with torch.cuda.device(self.device):
            if not (sl.is_cuda or st.is_cuda or ar.is_cuda):
                s, a, l = _pinned_image([(st, torch.float64), (ar, torch.float64), (sl.to(torch.int32), torch.int32)], self.device)
            else:
                l, s, a = (_to(t.to(d), self.device).contiguous() for t, d in zip((sl, st, ar), (torch.int32, torch.float64, torch.float64)))
            _lib.check(self.lib.tip_clock_map(self.state.data_ptr(), self.n, l.data_ptr(), s.data_ptr(), a.data_ptr(), m, self.leak,
                                               self.slew, out.data_ptr(), self._stream()))
        return out

    def reset(self, slots=None):
        """Forget the offsets of the listed slots (None: all): a slot whose hub restarted, or that takes a new wearer."""
        idx = self._slots(slots, "reset")
        if not idx:
            return
        with torch.cuda.device(self.device):
            sl = _to(torch.tensor(idx, dtype=torch.int32), self.device)
            _lib.check(self.lib.tip_clock_reset(self.state.data_ptr(), self.n, sl.data_ptr(), len(idx), self._stream()))

    def _get(self, slots, who):
        idx = self._slots(slots, who)
        theta = torch.zeros(len(idx), dtype=torch.float64, device=self.device)
        counts = torch.zeros((len(idx), 2), dtype=torch.int32, device=self.device)
        if idx:
            with torch.cuda.device(self.device):
                sl = _to(torch.tensor(idx, dtype=torch.int32), self.device)
                _lib.check(self.lib.tip_clock_get(self.state.data_ptr(), self.n, sl.data_ptr(), len(idx), theta.data_ptr(),
                                                   counts.data_ptr(), self._stream()))
        return theta, counts

    def export_slots(self, slots):
        """The listed slots' envelopes (32 bytes each) for import_slots of another ClockSync (tip_amd.handover); leak and slew belong to
        the object, not the wearer.  One launch, no synchronisation."""
        from . import handover
        return handover.export_simple(self, slots, "clock")

    def import_slots(self, slots, exported):
        """Put exported envelopes into the listed slots, whatever those held (a block of another size: ValueError, nothing launched)."""
        from . import handover
        handover.import_simple(self, slots, exported, "clock")

    def offsets(self, slots=None):
        """The offset estimates (server's clock minus sensor's, seconds) of the listed slots (None: all): a CUDA float64 tensor."""
        return self._get(slots, "offsets")[0]

    def counts(self, slots=None):
        """(count, rejected) of the listed slots (None: all), two CUDA int32 tensors: arrivals taken, arrivals refused."""
        c = self._get(slots, "counts")[1]
        return c[:, 0], c[:, 1]


class PacketResampler:
    """n rings of the last `depth` packets with their fp64 stamps on `device`, and the per-tick launch that gives every slot its
    packet at the tick (csrc/tip_resample.hip).  mode "hold": the newest packet not after t - delay, the demo's rule at delay 0;
    "slerp": interpolated between the two packets around t - delay (quaternions on the shorter arc, accelerations linearly in the
    global frame), which needs a delay of about one sensor period to have a later packet; "predict" (csrc/tip_clock.hip): "slerp"
    wherever t - delay has a later packet, and past the newest packet — delay 0 — the orientation continued at the angular rate of the
    newest two packets, by at most max_predict seconds and twice their spacing, the newest acceleration held in the global frame.
    max_hold (seconds; None: no limit): a packet older than that is not held and nothing is interpolated or predicted across a
    longer gap — the slot gets a NaN row, which fill=True of the front end fills or the engines' NaN contract takes.  No call synchronises; everything runs on the current stream."""

    def __init__(self, n: int, device, *, mode: str = "slerp", delay: float = 0.0, max_hold=None, depth: int = 8, max_predict=None):
        who = "PacketResampler"
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"tip_amd.sensors.{who}: n is the number of slots, at least 1; got {n!r}")
        self.n = int(n)
        self.mode_name = mode
        self.mode, self.delay, self.max_hold, self.depth = _resample_rule(mode, delay, max_hold, depth, who)
        self.max_predict = _predict_rule(mode, max_predict, who)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("tip_amd.sensors.PacketResampler runs on an MI355X: give it the engine's device")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.lib = _lib.load()
        nbytes = ctypes.c_size_t()
        _lib.check(self.lib.tip_resample_state_bytes(self.n, self.depth, ctypes.byref(nbytes)))
        self.state = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        self.t = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        self.flags = torch.full((self.n,), EMPTY, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.tip_resample_reset(self.state.data_ptr(), self.n, self.depth, None, 0, self._stream()))

    def _stream(self):
        return _lib.current_stream(self.device)

    def _slots(self, slots, who):
        return list(range(self.n)) if slots is None else slot_list(slots, self.n, f"sensors.PacketResampler.{who}")

    def push(self, packets, slots, times, *, arrivals=None, sync=None):
        """m arrivals: packets [m, 42] float32, slots [m] (an arrival for a slot outside [0, n) is skipped), times [m] float64 seconds.
        The arrivals of one slot are taken in array order; one whose stamp is not finite or not above the slot's newest is dropped and
        counted.  Host inputs go up in ONE non-blocking copy from pinned memory; CUDA tensors are used where they lie.  times that are
        no tensor (lists, numpy arrays) are read as float64 whatever they hold; a tensor of a narrower float type is refused: at an
        epoch-sized stamp float32 has already lost the packet's time.
        arrivals [m] and sync (a ClockSync of this pool's n, on this device), both or neither: times are then the SENSOR's stamps,
        arrivals the server's arrival times, and one launch maps every stamp through sync and inserts the packet at the mapped time —
        what sync.map followed by push leaves, bit for bit; an arrival that sync rejects is dropped and counted here too."""
        who = "tip_amd.sensors.PacketResampler.push"
        if (arrivals is None) != (sync is None):
            raise ValueError(f"{who}: arrivals and sync come together (sensor stamps, arrival times and the ClockSync that maps them) "
                             "or not at all")
        args = [torch.as_tensor(packets), torch.as_tensor(slots), _times_f64(times, f"{who}: times")]
        m = int(args[1].numel())
        if args[0].dim() != 2 or tuple(args[0].shape) != (m, PACKET) or args[1].dim() != 1 or tuple(args[2].shape) != (m,):
            raise ValueError(f"{who}: packets is [m, {PACKET}], slots [m] and times [m]; got {tuple(args[0].shape)}, "
                             f"{tuple(args[1].shape)}, {tuple(args[2].shape)}")
        if sync is not None:
            if not isinstance(sync, ClockSync) or sync.n != self.n or sync.device != self.device:
                raise ValueError(f"{who}: sync is a ClockSync of {self.n} slots on {self.device}")
            args.append(_times_f64(arrivals, f"{who}: arrivals"))
            if tuple(args[3].shape) != (m,):
                raise ValueError(f"{who}: arrivals is [m], one arrival time per packet; got {tuple(args[3].shape)} for m = {m}")
        if m == 0:
            return
        if args[1].dtype.is_floating_point or args[1].dtype == torch.bool:
            raise ValueError(f"{who}: slots are integers; got {args[1].dtype}")
        if sync is not None:
            with torch.cuda.device(self.device):
                if not any(a.is_cuda for a in args):
                    # times | arrivals | packets | slots in one pinned image: (8 + 8 + 168 + 4) m bytes, every part aligned to its type
                    t, a, p, s = _pinned_image([(args[2], torch.float64), (args[3], torch.float64), (args[0].to(torch.float32), torch.float32),
                                                (args[1].to(torch.int32), torch.int32)], self.device)
                else:
                    p, s, t, a = (_to(x.to(d), self.device).contiguous()
                                  for x, d in zip(args, (torch.float32, torch.int32, torch.float64, torch.float64)))
                _lib.check(self.lib.tip_clock_push(self.state.data_ptr(), sync.state.data_ptr(), self.n, self.depth, p.data_ptr(),
                                                    s.data_ptr(), t.data_ptr(), a.data_ptr(), m, sync.leak, sync.slew, None, self._stream()))
            return
        dtypes = (torch.float32, torch.int32, torch.float64)
        with torch.cuda.device(self.device):
            if not any(a.is_cuda for a in args):
                # times | packets | slots in one pinned image: 8 m + 168 m + 4 m bytes, every part aligned to its type
                image = torch.empty(180 * m, dtype=torch.uint8).pin_memory()
                image[: 8 * m].view(torch.float64).copy_(args[2].reshape(m))
                image[8 * m: 176 * m].view(torch.float32).copy_(args[0].reshape(-1))
                image[176 * m:].view(torch.int32).copy_(args[1].reshape(m))
                dev = image.to(self.device, non_blocking=True)
                t, p, s = dev[: 8 * m].view(torch.float64), dev[8 * m: 176 * m].view(torch.float32), dev[176 * m:].view(torch.int32)
            else:
                p, s, t = (_to(a.to(d), self.device).contiguous() for a, d in zip(args, dtypes))
            _lib.check(self.lib.tip_resample_push(self.state.data_ptr(), self.n, self.depth, p.data_ptr(), s.data_ptr(), t.data_ptr(),
                                                         m, self._stream()))

    def emit(self, t, out=None):
        """Every slot's packet at tick t -> a CUDA float32 [n, 42] (`out`, or a new tensor); `flags` [n] uint8 says how each row came
        about (INTERPOLATED, HELD, STALE, EMPTY, EARLY, of which the last three are NaN rows, and in mode "predict" PREDICTED).  t: a number or anything 0-d (one tick for the
        pool), or [n]; lists and numpy arrays are read as float64, a tensor of a narrower float type is refused.  A CUDA float64 [n]
        tensor is read WHERE IT LIES, which is what a captured frame needs: it must be contiguous and on this device, else it is
        refused rather than copied behind the caller's back.  Everything else goes through the resampler's own buffer `t`."""
        who = "tip_amd.sensors.PacketResampler.emit"
        if out is None:
            out = torch.empty((self.n, PACKET), dtype=torch.float32, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.device != self.device or out.dtype != torch.float32
              or tuple(out.shape) != (self.n, PACKET) or not out.is_contiguous()):
            raise ValueError(f"{who}: out is a contiguous float32 [{self.n}, {PACKET}] tensor on {self.device}")
        if isinstance(t, bool):
            raise ValueError(f"{who}: t is a number or [{self.n}] times in seconds; got {t!r}")
        h = _times_f64(t, f"{who}: t")
        if h.dim() > 1 or (h.dim() == 1 and tuple(h.shape) != (self.n,)):
            raise ValueError(f"{who}: t is a number or [{self.n}] times in seconds; got {tuple(h.shape)}")
        if h.is_cuda and h.dim() == 1 and isinstance(t, torch.Tensor) and t.dtype == torch.float64:
            if h.device != self.device or not h.is_contiguous():
                raise ValueError(f"{who}: a CUDA float64 [{self.n}] tensor is read where it lies: it must be contiguous and on {self.device}")
            tq = h
        else:
            tq = self.t
            if h.dim() == 0 and not h.is_cuda:
                tq.fill_(float(h))
            else:                                                 # (a 0-d value is broadcast)
                tq.copy_(h if h.is_cuda else h.contiguous().pin_memory(), non_blocking=True)
        with torch.cuda.device(self.device):
            if self.mode == MODES["predict"]:
                _lib.check(self.lib.tip_predict_emit(self.state.data_ptr(), self.n, self.depth, tq.data_ptr(), self.delay, self.max_hold,
                                                      self.max_predict, out.data_ptr(), self.flags.data_ptr(), self._stream()))
            else:
                _lib.check(self.lib.tip_resample_emit(self.state.data_ptr(), self.n, self.depth, tq.data_ptr(), self.delay, self.max_hold,
                                                             self.mode, out.data_ptr(), self.flags.data_ptr(), self._stream()))
        return out

    def export_slots(self, slots):
        """The listed slots' packet rings for import_slots of another PacketResampler of the same `depth` (tip_amd.handover); mode, delay
        and limits belong to the object, not the wearer.  One launch, no synchronisation."""
        from . import handover
        return handover.export_simple(self, slots, "resampler")

    def import_slots(self, slots, exported):
        """Put exported rings into the listed slots, whatever those held; another `depth` is a ValueError before anything is launched."""
        from . import handover
        handover.import_simple(self, slots, exported, "resampler")

    def reset(self, slots=None):
        """Empty the rings and zero the counters of the listed slots (None: all): a slot that takes a new wearer."""
        idx = self._slots(slots, "reset")
        if not idx:
            return
        with torch.cuda.device(self.device):
            sl = _to(torch.tensor(idx, dtype=torch.int32), self.device)
            _lib.check(self.lib.tip_resample_reset(self.state.data_ptr(), self.n, self.depth, sl.data_ptr(), len(idx), self._stream()))

    def counts(self, slots=None):
        """(have, dropped, total) of the listed slots (None: all), three CUDA int32 tensors [len(slots)]: packets in the ring
        (0 .. depth), packets refused for their stamp, packets taken since the last reset."""
        idx = self._slots(slots, "counts")
        out = torch.zeros((len(idx), 3), dtype=torch.int32, device=self.device)
        if idx:
            with torch.cuda.device(self.device):
                sl = _to(torch.tensor(idx, dtype=torch.int32), self.device)
                _lib.check(self.lib.tip_resample_get(self.state.data_ptr(), self.n, self.depth, sl.data_ptr(), len(idx), out.data_ptr(),
                                                            self._stream()))
        return out[:, 0], out[:, 1], out[:, 2]


def _sequence_times(times_list, lens, who):
    """times_list as host float64 arrays, one per sequence, each finite and strictly increasing; a bad one is a ValueError naming the
    sequence and the row."""
    if len(times_list) != len(lens):
        raise ValueError(f"tip_amd.sensors.{who}: {len(lens)} packet arrays for {len(times_list)} time arrays")
    out = []
    for i, (t, L) in enumerate(zip(times_list, lens)):
        if isinstance(t, torch.Tensor):
            t = t.detach().cpu().numpy()
        t = np.ascontiguousarray(t, dtype=np.float64)
        if t.shape != (L,):
            raise ValueError(f"tip_amd.sensors.{who}: times_list[{i}] is [{L}], one stamp per packet row; got {t.shape}")
        bad = np.flatnonzero(~np.isfinite(t))
        if bad.size:
            raise ValueError(f"tip_amd.sensors.{who}: times_list[{i}] row {int(bad[0])} is not finite")
        bad = np.flatnonzero(~(np.diff(t) > 0.0))
        if bad.size:
            raise ValueError(f"tip_amd.sensors.{who}: times_list[{i}] row {int(bad[0]) + 1} is not after row {int(bad[0])} "
                             "(stamps are strictly increasing)")
        out.append(t)
    return out


def sequence_ticks(times, rate_hz=60.0, delay=0.0, t_start=None):
    """The ticks resample_sequences takes a sequence at (host, float64): tick_times from t_start (None: the first stamp + delay, the
    first tick with something to give) while tick - delay <= the last stamp, so that every row has a packet at or after it.
    rate_hz, delay and t_start are checked as resample_sequences checks them; times [L] is the sequence's (ascending) stamps."""
    who = "sequence_ticks"
    rate_hz, delay = _tick_rule(rate_hz, delay, who)
    times = np.asarray(times.detach().cpu().numpy() if isinstance(times, torch.Tensor) else times, dtype=np.float64)
    if times.ndim != 1:
        raise ValueError(f"tip_amd.sensors.{who}: times is [L], a sequence's stamps; got {times.shape}")
    if times.size == 0:
        return np.empty(0, dtype=np.float64)
    if not (np.isfinite(times[0]) and np.isfinite(times[-1])) or (t_start is not None and not np.isfinite(float(t_start))):
        raise ValueError(f"tip_amd.sensors.{who}: the stamps and t_start are finite; got {times[0]!r} .. {times[-1]!r}, {t_start!r}")
    t0 = float(times[0]) + delay if t_start is None else float(t_start)
    most = int(np.floor(max((float(times[-1]) + delay - t0) * rate_hz, -1.0))) + 2
    ticks = tick_times(t0, max(most, 0), rate_hz)
    return ticks[ticks - delay <= times[-1]]


def sync_sequences(stamps_list, arrivals_list, leak=_lib.TIP_CLOCK_LEAK, slew=_lib.TIP_CLOCK_SLEW, device=None):
    """Recorded sessions whose packets carry the SENSOR's stamps beside the server's arrival times -> the stamps on the server's clock:
    stamps_list[i] and arrivals_list[i] are [L_i] float64 seconds, and the result is a list of host float64 arrays [L_i], what
    resample_sequences takes as times_list (a rejected row — a stamp or an arrival time that is not finite, a stamp not above the one
    before it — is NaN there, which resample_sequences refuses by its row).  Every sequence starts from a reset clock and gets, bit for
    bit, what a ClockSync(leak=, slew=) gives when it is fed the sequence in any chunking; all sequences in one launch."""
    who = "sync_sequences"
    leak, slew = _clock_rule(leak, slew, who)
    if not len(stamps_list):
        raise ValueError(f"tip_amd.sensors.{who}: no sequences")
    if len(stamps_list) != len(arrivals_list):
        raise ValueError(f"tip_amd.sensors.{who}: {len(stamps_list)} stamp arrays for {len(arrivals_list)} arrival arrays")
    st, ar, lens = [], [], []
    for i, (s, a) in enumerate(zip(stamps_list, arrivals_list)):
        s, a = _times_f64(s, f"tip_amd.sensors.{who}: stamps_list[{i}]"), _times_f64(a, f"tip_amd.sensors.{who}: arrivals_list[{i}]")
        if s.dim() != 1 or tuple(a.shape) != tuple(s.shape):
            raise ValueError(f"tip_amd.sensors.{who}: stamps_list[{i}] and arrivals_list[{i}] are [L], one arrival time per stamp; got "
                             f"{tuple(s.shape)} and {tuple(a.shape)}")
        st.append(s.detach().cpu())
        ar.append(a.detach().cpu())
        lens.append(int(s.shape[0]))
    dev = _device_of([], device)
    N = int(sum(lens))
    if N == 0:
        return [np.empty(0, dtype=np.float64) for _ in lens]
    with torch.cuda.device(dev):
        s, a, off = _pinned_image([(torch.cat(st), torch.float64), (torch.cat(ar), torch.float64),
                                   (torch.tensor(np.concatenate(([0], np.cumsum(lens))), dtype=torch.int64), torch.int64)], dev)
        out = torch.empty(N, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().tip_clock_rows(s.data_ptr(), a.data_ptr(), off.data_ptr(), N, len(lens), leak, slew, out.data_ptr(),
                                               _lib.current_stream(dev)))
        host = out.cpu().numpy()
    return [h.copy() for h in _split(host, lens)]


def resample_sequences(packets_list, times_list, rate_hz=60.0, *, mode="slerp", delay=0.0, max_hold=None, depth=8, t_start=None,
                       device=None, host=False, max_predict=None):
    """Recorded packet sessions whose stamps are not on the grid -> sessions that are: packets_list[i] is [L_i, 42] float32 and
    times_list[i] its stamps [L_i] (host float64; finite and strictly increasing, else a ValueError naming the sequence and the row).
    Sequence i is taken at sequence_ticks(times_list[i], rate_hz, delay, t_start) — t_start None, a number, or one number per sequence —
    and every output row is what a PacketResampler(mode, delay, max_hold, depth) that was pushed everything stamped up to the row's
    tick emits there, bit for bit, all sequences in one launch (mode "predict" with its max_predict included).  Returns (packets,
    flags): lists of CUDA float32 [K_i, 42] and uint8 [K_i] (host=True: numpy arrays).  The packets are what transform_sequences takes."""
    who = "resample_sequences"
    mode_c, delay, hold, depth = _resample_rule(mode, delay, max_hold, depth, who)
    far = _predict_rule(mode, max_predict, who)
    rate = float(rate_hz)
    if not (rate > 0.0 and np.isfinite(rate)):
        raise ValueError(f"tip_amd.sensors.{who}: rate_hz is the tick rate, a finite number > 0; got {rate_hz!r}")
    if not len(packets_list):
        raise ValueError(f"tip_amd.sensors.{who}: no sequences")
    lens = []
    for i, p in enumerate(packets_list):
        shape = tuple(p.shape) if hasattr(p, "shape") else np.shape(p)
        if len(shape) != 2 or shape[1] != PACKET:
            raise ValueError(f"tip_amd.sensors.{who}: packets_list[{i}] is [L, {PACKET}]; got {shape}")
        lens.append(int(shape[0]))
    times = _sequence_times(times_list, lens, who)
    if t_start is None or np.ndim(t_start) == 0:
        starts = [t_start] * len(lens)
    else:
        starts = [float(v) for v in np.asarray(t_start, dtype=np.float64).reshape(-1)]
        if len(starts) != len(lens):
            raise ValueError(f"tip_amd.sensors.{who}: t_start is None, a number or one number per sequence; got {len(starts)} for {len(lens)}")
    ticks = [sequence_ticks(t, rate, delay, s) for t, s in zip(times, starts)]
    out_lens = [int(t.shape[0]) for t in ticks]
    dev = _device_of(list(packets_list), device)
    lib = _lib.load()
    with torch.cuda.device(dev):
        packets, in_off, _ = _stack(packets_list, torch.float32, PACKET, dev, who, "packets_list")
        stamps = _to(torch.from_numpy(np.concatenate(times)), dev)
        t_out = _to(torch.from_numpy(np.concatenate(ticks)), dev)
        out_off = _to(torch.tensor(np.concatenate(([0], np.cumsum(out_lens))), dtype=torch.int64), dev)
        K = int(sum(out_lens))
        out = torch.empty((K, PACKET), dtype=torch.float32, device=dev)
        flags = torch.empty(K, dtype=torch.uint8, device=dev)
        if mode_c == MODES["predict"]:
            _lib.check(lib.tip_predict_rows(packets.data_ptr(), stamps.data_ptr(), in_off.data_ptr(), int(packets.shape[0]), t_out.data_ptr(),
                                             out_off.data_ptr(), K, len(lens), delay, hold, far, depth, out.data_ptr(), flags.data_ptr(),
                                             _lib.current_stream(dev)))
        else:
            _lib.check(lib.tip_resample_rows(packets.data_ptr(), stamps.data_ptr(), in_off.data_ptr(), int(packets.shape[0]), t_out.data_ptr(),
                                               out_off.data_ptr(), K, len(lens), delay, hold, mode_c, depth, out.data_ptr(), flags.data_ptr(),
                                               _lib.current_stream(dev)))
    return _recordings(out, flags, out_lens, host, True)
