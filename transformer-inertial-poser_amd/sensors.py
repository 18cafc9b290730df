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

packets is [n, 42] float32, per sensor q0 q1 q2 q3 ax ay az, the quaternion read as (x, y, z, w): what the demo hands to fairmotion's
Q2R, i.e. scipy's Rotation.from_quat(q).as_matrix() (fairmotion itself is unpinned, as for A2R / R2A).  accumulate() takes the whole
pool's packets and only the slots that are in a hold use theirs, so one wearer calibrates between the frames of the others.  Phases
change through these calls only, so the host's copy of them (PhaseMirror) is exact and nothing here reads the device or synchronises.
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
    [[0,0,1],[1,0,0],[0,1,0]] for all six sensors.  Every call is launches and non-blocking copies on the current stream."""

    def __init__(self, n: int, device, max_acc: float = 10.0, r_gp_b0=None):
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
        self._check(self.lib.tip_sensor_state_bytes(self.n, ctypes.byref(nbytes)))
        self.cal = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        self.packets = torch.zeros((self.n, PACKET), dtype=torch.float32, device=self.device)
        self.r_gp_b0 = None
        if r_gp_b0 is not None:
            r = torch.as_tensor(r_gp_b0, dtype=torch.float64)
            if r.numel() != 54:
                raise ValueError(f"tip_amd.SensorFrontEnd: r_gp_b0 is [6, 3, 3] or [6, 9]; got {tuple(r.shape)}")
            self.r_gp_b0 = self._to_dev(r.reshape(6, 9).contiguous())
        with torch.cuda.device(self.device):
            self._check(self.lib.tip_sensor_reset(self.cal.data_ptr(), self.n, self._stream()))

    def _check(self, status: int):
        if status < 0:
            raise _lib.TipStatusError(status, self.lib.tip_strerror(status).decode())

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

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
        """One tip_sensor_transform launch: the packet buffer -> raw [n, 72] (a CUDA float32 tensor of this device, contiguous)."""
        with torch.cuda.device(self.device):
            self._check(self.lib.tip_sensor_transform(self.cal.data_ptr(), self.packets.data_ptr(), self.n, self.max_acc, raw.data_ptr(),
                                                      self._stream()))

    # ---- the two holds ---------------------------------------------------------------------------------------------------------------
    def _begin(self, idx, which):
        if not idx:
            return
        with torch.cuda.device(self.device):
            sl = self._to_dev(torch.tensor(idx, dtype=torch.int32))
            self._check(self.lib.tip_sensor_begin(self.cal.data_ptr(), self.n, sl.data_ptr(), len(idx), which, self._stream()))

    def begin_heading(self, slots=None):
        """Start the heading hold of the listed slots (None: all): sensors lying aligned with the body reference frame
        (live_demo_new.py:217-226).  From uncalibrated, from a finished heading, or from live (a re-calibration)."""
        idx = self._slots(slots, "begin_heading")
        self.mirror.begin_heading(idx)
        self._begin(idx, _lib.TIP_SENSOR_HEADING)

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
            self._check(self.lib.tip_sensor_accumulate(self.cal.data_ptr(), self.packets.data_ptr(), self.n, self._stream()))

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
            self._check(self.lib.tip_sensor_finish(self.cal.data_ptr(), self.n, sl.data_ptr(), len(idx), r, self._stream()))

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
            self._check(self.lib.tip_sensor_set(self.cal.data_ptr(), self.n, sl.data_ptr(), len(idx), t.data_ptr(), self._stream()))

    def tables(self, slots=None):
        """The tables of the listed slots (None: all) as a CUDA tensor [len(slots), 126], whatever their phase."""
        idx = self._slots(slots, "tables")
        out = torch.empty((len(idx), TABLE), dtype=torch.float32, device=self.device)
        if idx:
            with torch.cuda.device(self.device):
                sl = self._to_dev(torch.tensor(idx, dtype=torch.int32))
                self._check(self.lib.tip_sensor_get(self.cal.data_ptr(), self.n, sl.data_ptr(), len(idx), out.data_ptr(), self._stream()))
        return out

    def live(self, slots=None):
        """bool [len(slots)] (numpy; None: all n): the slot's calibration is finished or loaded — transform gives it finite rows."""
        return self.mirror.live(None if slots is None else self._slots(slots, "live"))

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
