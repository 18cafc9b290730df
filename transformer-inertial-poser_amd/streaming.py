"""On-device streaming engine: the model-facing half of the reference's RTRunnerMin.step
(/root/reference/real_time_runner_minimal.py:114-167,196) for many lock-stepped IMU streams.

    eng = StreamingEngine(model, s_init)          # s_init [B,114] (q, dq) like RTRunnerMin's
    for frame in imu_frames:                       # frame [B,72]: 6 global rotations (row-major) + 6 accelerations
        out = eng.step(frame)                      # None while the 11-tap smoother primes (first 5 frames, :125-128)
        # out["s_rest"] [B,111] = s_t[3:114] (54 axis-angles, root velocity, zeros), out["c_t"] [B,20], out["y_last"]

Everything between the raw IMU frame and the fed-back history row stays in HBM: ring buffers, smoothing, root-frame
rotation, acc-sum feature, window gather, the forward pass (TIP_FWD_LAST_ROW_ONLY), output filter, SBP decode,
6D <-> axis-angle and the pose averaging (csrc/tip_stream.hip).  FK and the SBP root-translation correction
(:169-194) never feed back into the model input, so they are not part of the frame: tip_amd.kinematics.RootTracker consumes
out["s_rest"] / out["c_t"] in one more launch beside it.  RTRunner's terrain map and IK remain the host's job.

reuse=True (include/tip_hip.h: tip_forward_reuse): a frame's model inputs never change once recorded
(real_time_runner_minimal.py:74,85,137), so its in_linear row and its layer-0 Q / K / V rows are computed ONCE, when the frame enters,
and read from a per-stream ring (40 slots x 4 KiB) in the 39 later windows it appears in: 6.8 % of a window's FLOPs, 4-5 % of a
frame at >= 1024 streams.  Exact only with the stochastic parts off — model.eval(), past_state_dropout = 0, in_dropout = 0 (the
shipped loaders run with past_state_dropout 0.8, where a frame's row differs from window to window: the engine refuses) — and then
BIT-IDENTICAL to the engine that recomputes every window on the two-window encoder (set_plan("fused2"); AUTO's own plan at 1024
streams).  reuse="auto" switches it on where that encoder is the better plan anyway (two or more windows per CU) and the model
allows it.  reset() clears the ring; a ring that does not hold the window's 40 frames yields NaN rows, never stale numbers.

use_graph=True: once the window is full (T = 40 from frame 44 on) the three calls of a frame — ingest, forward_last, consume:
about 23 kernel launches for a handful of streams, each ~8 us of host time, which is what bounds a single stream's frame rate —
are captured ONCE into a HIP graph (torch.cuda.CUDAGraph; frame / call indices come from a counter in the state buffer,
TIP_STREAM_FRAME_AUTO) and every further frame is one copy of the raw frame into a static buffer + one graph launch.  Outputs are
bit-identical to the launch-by-launch loop (tests/test_streaming_gpu.py).  The graph freezes the model's packed weights and plan:
call reset() (or build a new engine) after changing parameters.  What the graph points at is OWNED by the engine for the graph's
lifetime (its own workspace, output row, and a reference to the packed weight image), never the module's evictable per-stream
buffers.  A captured forward is outside the library's cross-stream serialisation (include/tip_hip.h): replay it on the stream
the device's other forwards use, or when none is in flight.  Every replayed frame polls the handle's hand-off word (a pinned
host word, no synchronisation): a lost hand-off of an earlier replay — its y_last was NaN and went into the history ring —
re-primes the engine (reset()), demotes the handle to the non-cooperating plans when TIP_OPT_AUTO_DEMOTE allows, and raises
TipHandoffError.  The launch-by-launch engine does the same: when the model's forward reports that it demoted itself because
of an earlier frame's loss, step() resets the engine and raises instead of consuming on top of a NaN history row.

StaggeredStreamingEngine (below): the same loop for streams that start, warm up and stop ON THEIR OWN — n fixed slots, each with its
own frame counter, attached / detached between frames (attach(slots, s_init_rows), detach(slots)) without re-priming the others.
Windows sit in 40-row slots (rows past a slot's T_i are zero) and the forward is forward_rows (row T_i - 1 of each window;
include/tip_hip.h: tip_forward_rows): every slot costs a T = 40 window whatever its state, so a fresh staggered engine pays the
steady-state price from its first frame on.  No frame index anywhere: use_graph=True captures at the first step.
StaggeredStreamingEngine(..., compact=True) makes that cost follow the load instead: the attached slots are packed into window
positions 0 .. k-1 (include/tip_hip.h: tip_stream_ingest_mapped) and the forward runs on the top of the step of AUTO's cost staircase
that holds them (POOL_LADDER below).

Window length (window=W, both engines; default 40, the paper's — what "40" stands for everywhere above): the reference's runners take
it as max_input_l (real_time_runner_minimal.py:24; real_time_runner.py:29), and train_model.py --seq_len trains at any length.  W in
1 .. 128: rings, buffers and the forward's T follow it (T = min(max(f - 4, 0), W); graph capture from frame W + 4 on); the acc-sum
feature keeps its 40-frame span (the newest min(T, 40) rows).  40 runs the kernels with compile-time trip counts through the same
entry points as ever; any other length the tip_stream_*_w family (include/tip_hip.h), which takes W as a value.  reuse needs 40.

Model shapes (stream_shape below): the engines serve the four models the reference's runners accept — with or without the acc-sum
feature (x_imu 90 / 72 columns) times five or two stationary body points (size_s 131 / 119, c_t 20 / 8 columns) — and take the
shape from the model.  override_history(q, slots): RTRunner with multi_sbp_terrain_and_correction feeds back a pose its host-side
IK corrected, not the pose it returns (real_time_runner.py:483-495); the host hands that pose back between two frames.
override_history_device(q_dev, slots_dev) is the same launch with the list on the device, entries < 0 skipped: tip_amd.terrain runs that
IK on the device and hands its pose back without the host reading anything.

step_packets(front, packets), both engines: the frame from RAW sensor packets [n, 42] instead of the calibrated frame — `front` is a
tip_amd.sensors.SensorFrontEnd (the live demo's calibration and per-frame transform, live_demo_new.py:161-175, on the device), whose
one launch fills the engine's `raw`; everything behind "raw is filled" is step()'s (_step_filled), bit for bit.

export_slots(slots) / import_slots(slots, exported), StaggeredStreamingEngine: a live slot's whole state — its block, its rows, the
s_init it was attached with, its age — into a slot of another staggered engine of any n (plain or compact), where it continues bit for
bit instead of starting at its frame 0 (tip_amd.handover: the whole chain around the engine, files, other devices).
"""
from __future__ import annotations

import bisect
import ctypes
import gc
from typing import Optional

import numpy as np
import torch

from . import lib as _lib

# Compact pools: the batch a frame's forward runs on is the top of the step of AUTO's cost staircase over B that holds the k attached
# slots (one MI355X, 256 CUs, T = 40; tools/auto_sweep.py, profiles/pool/auto_sweep.txt, us per forward):
#   B <= 8: 151-153 | 9-16: 185-186 | 17-24: 248-250 | 25-32: 283-296 | 33-64: 312-316 | 65-128: 459-467 | 129-256: 620-624
# (the one-launch few-stream form steps once per window an XCD takes on, the launch chain grows to 32, the window-split encoder
# serves 64 and 128, one window per CU 256; 1, 2 and 4 cost what 8 does and keep a tiny pool's ingest small).  Beyond 256: whole
# rounds of POOL_ROUND windows plus a remainder served like a small batch, so the tops recur above every round — e.g. 264: 785,
# 272: 815, 280: 878, 320: 915, 384: 1066, 512: 1202, 520: 1367, 576: 1523, 640: 1676, 768: 1852, 832: 2096, 896: 2249, 1024: 2384 —
# except a 25-32 window remainder (288: 925 against 320: 915; 800: 2151 against 832: 2096), which the launch chain serves beside the
# whole rounds no cheaper than 64 windows.
POOL_LADDER = (1, 2, 4, 8, 16, 24, 32, 64, 128, 256)
POOL_REMAINDER = (8, 16, 24, 64, 128, 256)
POOL_ROUND = 256


def pool_ladder(n: int) -> list:
    """The batch sizes a compact pool of n slots runs its forward on: ascending, the last one n itself."""
    n = int(n)
    if n <= 0:
        return []
    out = [b for b in POOL_LADDER if b < n]
    for r in range(POOL_ROUND, n, POOL_ROUND):
        out += [r + b for b in POOL_REMAINDER if r + b < n]
    return out + [n]


def pool_bucket(k: int, ladder) -> int:
    """Smallest entry of `ladder` (ascending) that holds k windows; 0 for k = 0."""
    if k <= 0:
        return 0
    return ladder[bisect.bisect_left(ladder, k)]


SHAPES = ((72, 119), (72, 131), (90, 119), (90, 131))     # (x_imu columns, size_s) the streaming kernels serve
WINDOW_MAX = 128          # window lengths 1 .. 128 (include/tip_hip.h: the tip_stream_*_w family; the training step's T limit)
LIVE_WINDOW_MAX = 40      # live_dropout=True: what tip_forward_live serves (csrc/tip_fused.hip: fused_supported, T <= fz::TMAX = 40)


def check_window(window, who: str) -> int:
    """`window` as an int in [1, WINDOW_MAX]; anything else is a ValueError in `who`'s name (no device needed)."""
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or not 1 <= int(window) <= WINDOW_MAX:
        raise ValueError(f"tip_amd.{who}: window is the window length in frames, an int in [1, {WINDOW_MAX}] (the reference runners' "
                         f"max_input_l); got {window!r}")
    return int(window)


def stream_shape(model):
    """(n_sbps, with_acc_sum) of a model the streaming engines can serve: input_size_imu 72 (six IMUs), size_s = 111 + 4 * n_sbps
    with 2 or 5 stationary body points, with or without the 18 acc-sum columns.  Anything else raises ValueError."""
    n_imu, size_s, acc = int(model.input_size_imu), int(model.size_s), bool(model.with_acc_sum)
    if n_imu != 72 or size_s not in (119, 131):
        raise ValueError(f"tip_amd streaming engines serve x_imu / x_s widths {' | '.join(f'{a} / {b}' for a, b in SHAPES)} "
                         "(input_size_imu 72, with or without acc-sum; size_s 119 or 131: two or five stationary body points); "
                         f"this model has input_size_imu {n_imu}, with_acc_sum {acc}, size_s {size_s}")
    return (size_s - 111) // 4, acc


class SlotPositions:
    """Window positions of a compact pool (host only): the k attached slots hold positions 0 .. k-1, each exactly once.  A slot that
    attaches takes position k; one that detaches leaves its hole to the slot at the last position; re-attaching an attached slot
    keeps its position; reset() lays the attached slots out in slot order."""

    def __init__(self, n: int, attached=()):
        self.n = int(n)
        self.reset(attached)

    def reset(self, attached):
        self.slot_at = sorted({int(s) for s in attached})
        self.pos = [-1] * self.n
        for p, s in enumerate(self.slot_at):
            self.pos[s] = p

    def __len__(self):
        return len(self.slot_at)

    def attach(self, s: int) -> bool:
        """True if the map changed."""
        if self.pos[s] >= 0:
            return False
        self.pos[s] = len(self.slot_at)
        self.slot_at.append(s)
        return True

    def detach(self, s: int) -> bool:
        p = self.pos[s]
        if p < 0:
            return False
        last = self.slot_at.pop()
        if last != s:
            self.slot_at[p] = last
            self.pos[last] = p
        self.pos[s] = -1
        return True



def slot_list(slots, n: int, who: str) -> list:
    """`slots` as a list of ints, each in [0, n) and at most once; anything else is a ValueError in `who`'s name."""
    try:
        idx = [int(i) for i in slots]
    except TypeError:
        raise ValueError(f"tip_amd.{who}: slots must be a list of slot indices") from None
    if any(i < 0 or i >= n for i in idx):
        raise ValueError(f"tip_amd.{who}: slot index outside [0, {n})")
    if len(set(idx)) != len(idx):
        raise ValueError(f"tip_amd.{who}: duplicate slot index")
    return idx


def stage_image(n: int, positions, attach, detach, s_rows):
    """What a compact pool hands the device between two frames, as ONE int32 array: the position map (words 0 .. n-1: position ->
    slot, -1: empty), the slots to attach, the detached slots as int64 (8-byte aligned) and the attached slots' s_init rows (s_rows
    [len(attach), 114] float32, bit-cast).  Returns (image, (o_attach, o_detach, o_rows)), offsets in words."""
    o_det = (n + len(attach) + 1) // 2 * 2
    o_rows = o_det + 2 * len(detach)
    h = np.empty(o_rows + 114 * len(attach), dtype=np.int32)
    h[:n] = -1
    h[: len(positions)] = positions
    h[n: n + len(attach)] = attach
    h[o_det: o_rows] = np.asarray(detach, dtype=np.int64).view(np.int32)
    h[o_rows:] = np.ascontiguousarray(s_rows, dtype=np.float32).reshape(-1).view(np.int32)
    return h, (n, o_det, o_rows)


class _StreamBase:
    """What both engines share: shape, state block, frame buffers, the graph cache and the hand-off contract.  A subclass allocates
    its own in _allocate() (once, before the first reset()), says what a lost hand-off does to it (_reprime, _REPRIMED) and supplies
    the forward that warms a capture up (_warm_forward) and the frame that is captured (_captured_frame)."""

    def __init__(self, model, s_init: torch.Tensor, use_graph: bool, live_dropout: bool = False, window: int = 40):
        self.model = model
        # window: the reference runners' max_input_l — rings, buffers and the forward's T.  40 runs the 40-row entry points (today's
        # kernels, bit for bit); any other length the tip_stream_*_w family (_call)
        self.window = check_window(window, type(self).__name__)
        if live_dropout and self.window > LIVE_WINDOW_MAX:
            raise ValueError(f"tip_amd.{type(self).__name__}(live_dropout=True): the live forward (tip_forward_live) serves windows of at "
                             f"most {LIVE_WINDOW_MAX} frames; got window={self.window}")
        # live_dropout: every frame's forward is model.forward_live (the model as the reference deploys it: past-state keep mask drawn
        # in the first kernel, encoder dropout live in .train() mode, no stash) under the engine's own device seeds
        self.live_dropout = bool(live_dropout)
        self.n_sbps, self.with_acc_sum = stream_shape(model)
        self.nx, self.ns, self.nc = 72 + (18 if self.with_acc_sum else 0), int(model.size_s), 4 * self.n_sbps
        self.use_graph = bool(use_graph)
        self.lib = _lib.load()
        s_init = torch.as_tensor(s_init, dtype=torch.float32)
        if s_init.dim() == 1:
            s_init = s_init.unsqueeze(0)
        assert s_init.shape[1] == 114, "s_init is (q, dq) with 57 dofs each (constants.py:24)"
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError("tip_amd.StreamingEngine runs on an MI355X: move the model to the GPU first")
        if model.training and not self.live_dropout:
            import warnings
            warnings.warn("tip_amd.StreamingEngine: the model is in .train() mode — like the reference's runner without "
                          ".eval() (offline_testing_simple.py:98) every frame then draws the encoder's dropout, here through "
                          "the HIP TRAINING kernels (all rows, activation stash); call model.eval() for the inference plans")
        self.n = int(s_init.shape[0])
        nbytes = ctypes.c_size_t()
        self._check(self.lib.tip_stream_state_bytes_w(self.n, self.window, ctypes.byref(nbytes)))
        self.state = torch.empty(max(nbytes.value, 4), dtype=torch.uint8, device=self.device)
        self.s_init = s_init.to(self.device).contiguous()
        self.x_imu = torch.empty((self.n, self.window, self.nx), dtype=torch.float32, device=self.device)
        self.x_s = torch.empty((self.n, self.window, self.ns), dtype=torch.float32, device=self.device)
        self.s_rest = torch.empty((self.n, 111), dtype=torch.float32, device=self.device)
        self.c_t = torch.empty((self.n, self.nc), dtype=torch.float32, device=self.device)
        self.raw = torch.empty((self.n, 72), dtype=torch.float32, device=self.device)    # static input of the captured graph
        # live_dropout: {encoder seed, state seed} on the device, filled from model._draw_seeds() (torch.manual_seed governs it) at every
        # reset and advanced by tip_seeds_next in front of every frame's forward — a frame is reproduced from the values read before it
        self.seeds = torch.zeros(2, dtype=torch.int64, device=self.device) if self.live_dropout else None
        # captured frames by key (None: the one frame of a lock-step or plain staggered engine; a compact pool: one per bucket), each
        # (graph, workspace, packed weight image, y_last): the graph and what its kernels point at
        self._graphs, self.captures = {}, 0
        self._graph_ws = self._graph_y = None      # the engine's own, sized for n, shared by every entry and kept across reset()
        self._allocate()
        self.reset()

    def _check(self, status: int):
        return _lib.check(status)

    def _stream(self):
        return _lib.current_stream(self.device)

    def _call(self, name: str, *args):
        """tip_stream_<name>(*args, stream) on the current stream at window 40 — the 40-row entry points, as ever — and
        tip_stream_<name>_w(*args, window, stream) at any other length."""
        if self.window == 40:
            self._check(getattr(self.lib, "tip_stream_" + name)(*args, self._stream()))
        else:
            self._check(getattr(self.lib, "tip_stream_" + name.replace("_shaped", "") + "_w")(*args, self.window, self._stream()))

    def _to_dev(self, t):
        """Host -> device without a synchronising copy from pageable memory (an attach between two frames must not drain the queue)."""
        return t.to(self.device, non_blocking=True) if t.is_cuda else t.pin_memory().to(self.device, non_blocking=True)

    def _reset_state(self, s_init):
        """tip_stream_reset_shaped: every block rebuilt from its s_init row, the buffer's shape recorded for the kernels."""
        with torch.cuda.device(self.device):
            self._call("reset_shaped", self.state.data_ptr(), s_init.data_ptr(), self.n, self.n_sbps, 1 if self.with_acc_sum else 0)
            if self.live_dropout:
                self.seeds.copy_(torch.tensor(self.model._draw_seeds(), dtype=torch.int64))

    def _live_forward(self, x_imu, x_s, rows, ws, out, advance=True):
        """live_dropout: tip_seeds_next, then forward_live under the device seeds — the same two calls launch by launch and inside a
        capture, so a replay draws what the launch-by-launch frame would have drawn.  advance=False: a capture's warm-up (its result is
        dropped and must not cost a draw)."""
        if advance:
            _lib.seeds_next(self.seeds.data_ptr(), self._stream())
        return self.model.forward_live(x_imu, x_s, rows=rows, seeds_dev=self.seeds, workspace=ws, out=out)

    def _forget(self):
        """Frame counter back to 0, every captured frame dropped."""
        self.frame = 0
        self._graphs = {}
        self._y_last = None

    # the single captured frame and what it points at; None before the capture and after reset() or a lost hand-off
    _graph = property(lambda self: self._graphs[None][0] if None in self._graphs else None)
    _graph_refs = property(lambda self: self._graphs[None][1:] if None in self._graphs else None)

    # ---- host override of the fed-back pose ----------------------------------------------------------------------------------------
    def override_history(self, q, slots=None):
        """Replace the pose the last step() fed back — columns 0 .. 107 of the newest history row — by the host's corrected one.
        q: [len(slots), 54] (root + 17 joints, axis-angle: s_t[3:57] of the reference) or [len(slots), 114] (a full qdq, of which
        [3:57] is taken); host or CUDA tensor.  slots: slot indices, None = all.  Call it after step() returned the frame it corrects
        and before the next step() (RTRunner's multi_sbp_terrain_and_correction: real_time_runner.py:483-495 feeds back
        st_hist_copy, the IK-corrected copy of the pose it returns).  Root velocity, c_t, the pose average and the output filter are
        not touched.  One small launch on the current stream; with use_graph=True it runs between two replays, nothing is
        re-captured."""
        who = f"{type(self).__name__}.override_history"
        idx = list(range(self.n)) if slots is None else slot_list(slots, self.n, who)
        q = torch.as_tensor(q, dtype=torch.float32)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        if q.dim() != 2 or q.shape[0] != len(idx) or q.shape[1] not in (54, 114):
            raise ValueError(f"tip_amd.{who}: q is [len(slots), 54] (axis-angle root + 17 joints) or "
                             f"[len(slots), 114] (qdq); got {tuple(q.shape)} for {len(idx)} slots")
        if q.shape[1] == 114:
            q = q[:, 3:57]
        self._override_ready(idx)
        if not idx:
            return
        with torch.cuda.device(self.device):
            q = self._to_dev(q.contiguous()).contiguous()
            sl = self._to_dev(torch.tensor(idx, dtype=torch.int32))
            self._call("history_override", self.state.data_ptr(), self.n, sl.data_ptr(), q.data_ptr(), len(idx))

    def override_history_device(self, q_dev, slots_dev):
        """override_history with the list on the device: q_dev [n, 54] float32 and slots_dev [n] int32, both CUDA tensors of this
        engine's device.  Entry j rewrites slot slots_dev[j] from q_dev[j]; an entry below 0, and a slot that has not consumed a frame
        yet, is skipped by the kernel, so the host never reads the list — what tip_amd.terrain.TerrainTracker.feed_back hands over
        (its `fire`).  The same launch as override_history's, on the current stream, between two frames; nothing is re-captured."""
        who = f"{type(self).__name__}.override_history_device"
        for t, dt, tail, what in ((q_dev, torch.float32, (54,), "q_dev [n, 54] float32"), (slots_dev, torch.int32, (), "slots_dev [n] int32")):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self.device and t.dtype == dt and t.is_contiguous()
                    and tuple(t.shape[1:]) == tail and t.dim() == 1 + len(tail)):
                raise ValueError(f"tip_amd.{who}: {what} is a contiguous CUDA tensor on {self.device}")
        if q_dev.shape[0] != slots_dev.shape[0]:
            raise ValueError(f"tip_amd.{who}: q_dev has {q_dev.shape[0]} rows for {slots_dev.shape[0]} list entries")
        if slots_dev.shape[0] == 0:
            return
        with torch.cuda.device(self.device):
            self._call("history_override", self.state.data_ptr(), self.n, slots_dev.data_ptr(), q_dev.data_ptr(), int(slots_dev.shape[0]))

    # ---- raw IMU packets (tip_amd.sensors) ------------------------------------------------------------------------------------------
    def _packets_to_raw(self, front, packets, slots, launch=True):
        """The front half of step_packets: `front` (a sensors.SensorFrontEnd of this engine's n and device) takes the packets [n, 42]
        into its buffer and ONE tip_sensor_transform launch writes the calibrated frame straight into self.raw — no intermediate
        tensor, no device-to-device copy.  Every slot of `slots` must be live (the front end's host mirror): a refusal raises before
        anything is copied or launched.  launch=False: checks only (a compact pool with nothing attached)."""
        who = f"{type(self).__name__}.step_packets"
        if getattr(front, "n", None) != self.n or getattr(front, "device", None) != self.device:
            raise ValueError(f"tip_amd.{who}: the front end serves {getattr(front, 'n', None)} slots on {getattr(front, 'device', None)}, "
                             f"the engine {self.n} on {self.device}")
        for i in slots:
            if not front.mirror.phase[i] == 4:
                raise RuntimeError(f"tip_amd.{who}: slot {i} is not calibrated (phase {front.mirror.phase[i]}: finish its heading and "
                                   "T-pose holds, or load() its tables, before it streams)")
        if launch:
            front._fill(packets, who)
            front._transform_into(self.raw)

    # ---- the hand-off contract ------------------------------------------------------------------------------------------------------
    def _demotions(self):
        """Read by a frame body before and after its forward: a change says that the model answered a lost hand-off in between."""
        return self.model.demotions + self.model.flow_demotions

    def _lost_handoff(self, err=None):
        """An EARLIER frame lost an inter-workgroup hand-off: its NaN row is in the history ring (the prologue would scrub it to 0
        for the next 40 windows: finite, degraded poses) and in the reuse ring.  Re-prime and raise TipHandoffError instead of
        consuming on top of it.  err None: tip_forward's entry check found it, the model demoted itself and served this call.  err:
        the poll before a replay or the reuse forward raised it — demote the handle to the plans without hand-offs when allowed (a
        launch chain instead of the one-launch form first), and pass err on."""
        if err is not None:
            h = self.model._ensure_handle()
            if self.model._answer_handoff(h) is None:
                h.check_clear()
        self._reprime()
        raise err or _lib.TipHandoffError(_lib.TIP_ERR_HANDOFF, "an earlier frame of this engine lost an inter-workgroup hand-off; "
                                          f"the model now runs the non-cooperating plans and {self._REPRIMED}")

    def _poll_handoff(self):
        """Graph mode: tip_forward's entry check never runs during a replay, so the engine reads the hand-off word itself."""
        try:
            self.model.check_handoffs(synchronize=False)
        except _lib.TipHandoffError as e:
            self._lost_handoff(e)

    # ---- captured frames ------------------------------------------------------------------------------------------------------------
    def _capture(self, key):
        """Capture the frame `key` (_captured_frame) into a HIP graph, after its forward ran once outside the capture (_warm_forward)."""
        if self._graph_ws is None:
            # what the captured kernels will point at: allocated OUTSIDE the capture, held by the engine, one for every key and sized for
            # n (the one-launch form keeps its counters at offset 0 for any batch: include/tip_hip.h, tip_workspace_bytes; replays are serial)
            self._graph_ws = torch.empty(self.model.workspace_bytes(self.n, self.window), dtype=torch.uint8, device=self.device)
            self._graph_y = torch.empty((self.n, self.model.size_s), dtype=torch.float32, device=self.device)
        # packs / attaches outside the capture.  The device RNG is put back afterwards: with past_state_dropout or in_dropout live
        # this warm-up would otherwise draw once more than the launch-by-launch loop does
        rng = torch.cuda.get_rng_state(self.device)
        self._warm_forward(key)
        torch.cuda.set_rng_state(rng, self.device)
        torch.cuda.current_stream(self.device).synchronize()
        self._poll_handoff()
        g = torch.cuda.CUDAGraph()
        # no cycle collection inside the capture: a dead cycle may hold another engine's captured graphs, pinned buffers or a library
        # handle (a dropped pool is one: its feeder closures point back at its engine), and their finalizers make HIP calls that a
        # capturing thread must not make.  torch.cuda.graph no longer collects on entry, so the collector could fire on any allocation
        # of the frame's host code.  What is dead now is collected as usual once the capture has ended.
        collecting = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._y_last = self._captured_frame(key)
        finally:
            if collecting:
                gc.enable()
        self._graphs[key] = (g, self._graph_ws, self.model._packed_dev, self._graph_y)
        self.captures += 1
        return g

    def _replay(self, key):
        """One replay of the frame `key`, captured first if it is not; a frame that is already there polls the hand-off word."""
        e = self._graphs.get(key)
        if e is None:
            return self._capture(key).replay()
        self._poll_handoff()
        e[0].replay()


class StreamingEngine(_StreamBase):
    _REPRIMED = "the engine was reset (re-prime it)"

    def __init__(self, model, s_init: torch.Tensor, use_graph: bool = False, reuse: bool = False, live_dropout: bool = False,
                 window: int = 40):
        """window: the window length W in frames, 1 .. 128 — RTRunnerMin's max_input_l (real_time_runner_minimal.py:24,54,131,139):
        the call for frame f has T = min(max(f - 4, 0), W) rows, the rings are W deep, forward_last runs at T = W once the window is
        full and use_graph=True captures from frame W + 4 on; the acc-sum feature still spans the newest min(T, 40) rows.  40 is
        the paper's, on kernels with compile-time trip counts; any other length takes W as a value.  reuse=True needs window=40 (the
        reuse ring is 40 slots: ValueError otherwise; "auto" is then off), live_dropout=True a window the live forward serves
        (at most 40: ValueError otherwise, at construction).
        live_dropout=True: serve the model as the reference deploys it — .train() or .eval() (then only the past-state keep mask is
        live), every frame ingest -> tip_seeds_next -> model.forward_live(seeds_dev=engine.seeds) -> consume, launch by launch and
        captured alike: use_graph=True replays from the usual frame on with a .train() model too and reproduces launch mode bit for
        bit.  reuse=True is refused and "auto" is off (rows differ from window to window)."""
        if live_dropout and reuse is True:
            raise RuntimeError("tip_amd.StreamingEngine(live_dropout=True): reuse=True is not supported — with dropout live a frame's rows "
                               "differ from window to window")
        window = check_window(window, "StreamingEngine")
        if reuse is True and window != 40:
            raise ValueError(f"tip_amd.StreamingEngine(reuse=True): the reuse ring holds 40-frame windows; got window={window}")
        # True / False / "auto" (resolved in _allocate, once the stream count is known)
        self.reuse = False if (live_dropout or window != 40) else reuse
        super().__init__(model, s_init, use_graph, live_dropout, window)

    def _allocate(self):
        model = self.model
        self._ring = self._ctr_ptr = None
        if self.reuse == "auto":
            # the reuse form runs on the two-window encoder (1.049 ms per round of 2 x #CUs windows, ~5.8 % less with the ring); below
            # two windows per CU the one-window kernel (0.527 ms per round of #CUs) is the better plan even without it
            cus = torch.cuda.get_device_properties(self.device).multi_processor_count
            r2, rh = ((self.n + 1) // 2 + cus - 1) // cus, (self.n + cus - 1) // cus
            exact = not (model.training or model.past_state_dropout > 0.0 or model.in_dropout > 0.0)
            self.reuse = exact and self.n > cus and r2 * 1049 * 0.945 < rh * 527
        self.reuse = bool(self.reuse)
        if self.reuse:
            # a frame's in_linear row and layer-0 Q / K / V rows are kept across the 40 windows it appears in
            # (model.forward_last_reuse; exact only with the stochastic parts off — it raises otherwise)
            if model.training or model.past_state_dropout > 0.0 or model.in_dropout > 0.0:
                raise RuntimeError("tip_amd.StreamingEngine(reuse=True) needs model.eval() and a model built with past_state_dropout = 0, "
                                   "in_dropout = 0: with dropout live a frame's rows differ from window to window")
            self._ring = model.reuse_cache(self.n)
            off = ctypes.c_size_t()
            self._check(self.lib.tip_stream_frame_counter_offset(ctypes.byref(off)))
            self._ctr_ptr = self.state.data_ptr() + off.value      # the frame index the ingest kernel keeps (stream 0's block)

    def reset(self):
        self._forget()
        if self._ring is not None:
            self.model.reuse_reset(self._ring)
        self._reset_state(self.s_init)

    _reprime = reset        # (a lost hand-off: the NaN row is in the reuse ring too)

    def _override_ready(self, idx):
        """The slots of `idx` have consumed a frame (lock-step: all of them, from frame 5 on)."""
        if self.frame < 6:
            raise RuntimeError("tip_amd.StreamingEngine.override_history: no frame has been consumed yet (step() returns None while "
                               "the smoother primes: frames 0 .. 4)")

    def _frame(self, raw, f, f_consume, T, ws, out):
        """ingest -> forward_last -> consume on windows of T rows; None while the smoother primes (T = 0).  Launch by launch: frame
        indices f and f - 5, the module's own buffers (ws = out = None).  Captured: TIP_STREAM_FRAME_AUTO twice, T = window, the
        engine's."""
        # (full windows: the reuse forward reads only the newest row of x_imu / x_s — the 35-KB window gather per stream is skipped;
        # reuse implies window 40)
        self._call("ingest_newest" if (self.reuse and T == 40) else "ingest", self.state.data_ptr(), raw.data_ptr(), self.n, f,
                   self.x_imu.data_ptr(), self.x_s.data_ptr())
        if T == 0:
            return None
        x_imu, x_s = self.x_imu, self.x_s
        if T < self.window:      # windows are written densely as [n, T, *] at the head of the preallocated buffers
            x_imu = x_imu.view(-1)[: self.n * T * self.nx].view(self.n, T, self.nx)
            x_s = x_s.view(-1)[: self.n * T * self.ns].view(self.n, T, self.ns)
        mark = self._demotions()
        if self.reuse:
            f_fwd, ctr = (f, None) if ws is None else (0, self._ctr_ptr)
            try:
                y_last = self.model.forward_last_reuse(x_imu, x_s, self._ring, f_fwd, frame_ctr_ptr=ctr, workspace=ws, out=out)
            except _lib.TipHandoffError as e:
                self._lost_handoff(e)
        elif self.live_dropout:
            y_last = self._live_forward(x_imu, x_s, None, ws, out)
        else:
            y_last = self.model.forward_last(x_imu, x_s, workspace=ws, out=out)
        if self._demotions() != mark:
            self._lost_handoff()
        self._call("consume", self.state.data_ptr(), y_last.data_ptr(), self.n, f_consume, self.s_rest.data_ptr(), self.c_t.data_ptr())
        return y_last

    def _warm_forward(self, key):
        if self.live_dropout:
            self._live_forward(self.x_imu, self.x_s, None, self._graph_ws, self._graph_y, advance=False)
            return
        self.model.forward_last(self.x_imu, self.x_s, workspace=self._graph_ws, out=self._graph_y)   # (never touches the ring)

    def _captured_frame(self, key):
        return self._frame(self.raw, _lib.TIP_STREAM_FRAME_AUTO, _lib.TIP_STREAM_FRAME_AUTO, self.window, self._graph_ws, self._graph_y)

    def _replays(self):
        """This frame is a replay of the captured one (steady state, T = window): its input is self.raw."""
        return self.use_graph and self.frame >= self.window + 4 and (self.live_dropout or not self.model.training)

    @torch.no_grad()
    def step(self, raw_imu: torch.Tensor) -> Optional[dict]:
        if self._replays():
            # steady state (T = window): one copy + one graph launch per frame
            self.raw.copy_(torch.as_tensor(raw_imu, dtype=torch.float32).reshape(self.n, 72), non_blocking=True)
            return self._step_filled(self.raw)
        raw = torch.as_tensor(raw_imu, dtype=torch.float32).reshape(self.n, 72).to(self.device, non_blocking=True).contiguous()
        return self._step_filled(raw)

    @torch.no_grad()
    def step_packets(self, front, packets) -> Optional[dict]:
        """step() from raw IMU packets [n, 42] (tip_amd.sensors.SensorFrontEnd: layout, calibration): one tip_sensor_transform launch
        fills the engine's `raw` on the device, then the frame runs as step() runs it.  Lock-step has no detached slots: every slot
        of `front` must be live.  With use_graph=True the launch sits between two replays; nothing is re-captured."""
        self._packets_to_raw(front, packets, range(self.n))
        return self._step_filled(self.raw)

    def export_slots(self, slots):
        """Not served: one frame counter serves all streams of a lock-step engine, so a single stream has no state of its own to take
        along.  Wearers that come and go live in a StaggeredStreamingEngine."""
        raise RuntimeError("tip_amd.StreamingEngine.export_slots: a lock-step engine keeps one frame counter for all its streams; "
                           "wearer hand-over is StaggeredStreamingEngine.export_slots / import_slots")

    def import_slots(self, slots, exported):
        raise RuntimeError("tip_amd.StreamingEngine.import_slots: a lock-step engine keeps one frame counter for all its streams; "
                           "wearer hand-over is StaggeredStreamingEngine.export_slots / import_slots")

    def _step_filled(self, raw) -> Optional[dict]:
        """The frame behind "raw is filled" (raw: [n, 72] on the device; self.raw when the frame replays)."""
        f = self.frame
        if self._replays():
            with torch.cuda.device(self.device):
                self._replay(None)
            self.frame = f + 1
            return {"s_rest": self.s_rest, "c_t": self.c_t, "y_last": self._y_last, "T": self.window}
        T = int(self.lib.tip_stream_window_len_w(f, self.window))
        self.frame = f + 1          # (the frame is ingested whatever its forward does; a lost hand-off resets the counter)
        with torch.cuda.device(self.device):
            y_last = self._frame(raw, f, f - 5, T, None, None)
        return None if T == 0 else {"s_rest": self.s_rest, "c_t": self.c_t, "y_last": y_last, "T": T}


class StaggeredStreamingEngine(_StreamBase):
    """Streams that start, warm up and stop on their own (include/tip_hip.h, "staggered streams"): n fixed slots, each with its
    own frame counter, attached or detached.

        eng = StaggeredStreamingEngine(model, s_init)      # s_init [n,114]: every slot attached, at its frame 0
        out = eng.step(raw)                                # raw [n,72]; always a dict (below)
        eng.detach([3])                                    # slot 3 stops (its state is kept, its rows are skipped)
        eng.attach([3], s_init_rows)                       # slot 3 restarts at its frame 0 from s_init_rows [1,114]

    step() returns s_rest [n,111], c_t [n,20], y_last [n,131] (c_t [n,8], y_last [n,119] for a two-SBP model), T (int32 [n]: the
    slot's window length this frame, 0 while priming or detached) and valid (bool [n]: the slot produced a row this frame).
    Rows of slots that are not valid are NaN in y_last and unchanged in s_rest / c_t.  A frame is ingest_staggered ->
    forward_rows -> consume_staggered with no frame index, so with use_graph=True it is captured once, at the first step, and
    replayed from then on; attach / detach run between replays.  Every slot occupies a T = 40 window in the forward whatever its
    state (a fixed slot -> window map keeps the graph static): a fresh engine pays the steady-state price from its first frame
    on, where StreamingEngine runs shorter windows while it warms up.  .eval() only (fp32); reuse= is refused (the reuse ring
    assumes lock-step frames).  A lost hand-off (StreamingEngine's contract) re-attaches every attached slot with the s_init it
    was last attached with and raises TipHandoffError.

    compact=True: a pool whose cost follows its load.  The k attached slots hold window positions 0 .. k-1 (SlotPositions: a fresh
    engine and reset() lay them out in slot order, a detach moves the last position into the hole, re-attaching keeps the position)
    and the frame runs ingest_mapped -> forward_rows on B = bucket(k) windows (pool_ladder(n); bucket(n) = n) -> consume_mapped; the
    positions k .. B-1 are empty (zero windows), and k = 0 launches nothing.  The map is one device buffer, refreshed between frames
    by a non-blocking copy from pinned memory.  step() returns the same dict, indexed by slot, plus active (k) and batch (B); a slot
    that detaches gets its y_last row set to NaN and its T to 0 on the host side.  use_graph=True keeps one captured frame per
    bucket, captured on first use or by prewarm(); all of them share one workspace sized for n, `captures` counts them, and reset()
    or a lost hand-off (which keeps the positions) drops them all.  Bits: with every slot attached and no detach, positions are the
    slots and B = n — bit-identical to compact=False.  Under AUTO the plan follows B (and AUTO splits a batch into whole rounds plus
    a remainder), so a slot's bits may change when k crosses a bucket edge or the slot moves — within the parity bound of the fp64
    reference; on a pinned plan whose per-window results do not depend on the batch (set_plan("fused")) they do not change, and
    compact=True is bit-identical per slot to compact=False under any attach / detach schedule."""

    _REPRIMED = "every attached slot was re-attached"

    def __init__(self, model, s_init: torch.Tensor, use_graph: bool = False, reuse: bool = False, compact: bool = False,
                 live_dropout: bool = False, window: int = 40):
        """window (StreamingEngine's): windows sit in `window`-row slots and every slot costs a T = window forward, plain and compact.
        The compact pool's ladder (POOL_LADDER) was calibrated at T = 40 and is kept for every window: it is unmeasured elsewhere, and
        it decides cost only, never results.
        live_dropout=True (StreamingEngine's): a .train() model is accepted, and every frame's forward is tip_seeds_next ->
        model.forward_live(rows=..., seeds_dev=engine.seeds) in place of forward_rows, plain and compact, launch by launch and captured."""
        window = check_window(window, "StaggeredStreamingEngine")
        if reuse is True and window != 40:
            raise ValueError(f"tip_amd.StaggeredStreamingEngine(reuse=True): the reuse ring holds 40-frame windows; got window={window}")
        if reuse:
            raise RuntimeError("tip_amd.StaggeredStreamingEngine: reuse= is not supported (the reuse ring assumes lock-step frames)")
        if model.training and not live_dropout:
            raise RuntimeError("tip_amd.StaggeredStreamingEngine needs model.eval() (the inference kernels: forward_rows)")
        self.reuse, self._ring = False, None          # (lock-step only)
        self.compact = bool(compact)
        super().__init__(model, s_init, use_graph, live_dropout, window)
        self.s_rest.zero_()          # (rows of slots that have not produced a row yet: defined, and unchanged until they do)
        self.c_t.zero_()

    def _allocate(self):
        self._attached = [True] * self.n
        self.s_cur = self.s_init.clone()
        self.rows = torch.empty(self.n, dtype=torch.int32, device=self.device)
        if self.compact:
            self.ladder = pool_ladder(self.n)
            self._positions = SlotPositions(self.n)
            self.s_host = self.s_init.cpu()       # the s_init rows slots were last attached with, on the host
            # one device buffer for everything attach / detach hand the device between two frames, filled by ONE copy from
            # pinned memory (_flush, stage_image): the position map (words 0 .. n-1, where every captured frame reads it), then the
            # slots to attach, the slots detached (int64) and the attached slots' s_init rows
            self._stage = torch.empty(self.n * 118 + 2, dtype=torch.int32, device=self.device)
            self.slot_at = self._stage[: self.n]                                         # position -> slot, -1: empty
            self._pending_attach, self._pending_detach = {}, {}
            self.y_slot = torch.full((self.n, self.model.size_s), float("nan"), dtype=torch.float32, device=self.device)
            self.rows_slot = torch.full((self.n,), -1, dtype=torch.int32, device=self.device)
            self._fed, self.fed_frames = None, 0          # device-fed frames (_step_fed): the feeder's two launches, frames launched
            self._s_arriving = []     # import_slots: (event, slots, pinned rows) of s_init rows still on their way to s_host (_s_host_settle)

    def _attach_dev(self, idx):
        if not idx:
            return
        with torch.cuda.device(self.device):
            slots = self._to_dev(torch.tensor(idx, dtype=torch.int32))
            rows = self.s_cur.index_select(0, slots.long()).contiguous()
            self._call("attach", self.state.data_ptr(), self.n, slots.data_ptr(), rows.data_ptr(), len(idx))

    def reset(self):
        """Re-prime: every attached slot restarts at its frame 0 from the s_init it was last attached with; detached slots stay
        detached.  Drops the captured graph(s); a compact pool lays its attached slots out in slot order again."""
        if self.compact:
            self._positions.reset([i for i in range(self.n) if self._attached[i]])
        self._restart()

    def _restart(self):
        """Every attached slot back to its frame 0 (positions kept), graphs dropped."""
        self._forget()
        self._attach_frame = [0] * self.n       # engine frame at which the slot was last attached (override_history: its age)
        self._reset_state(self.s_cur)
        if self.compact:
            self._pending_attach = dict.fromkeys([i for i in range(self.n) if self._attached[i]])   # (re-attached by the next step)
            self._map_dirty = True
        else:
            self._attach_dev([i for i in range(self.n) if self._attached[i]])

    _reprime = _restart

    def attach(self, slots, s_init_rows):
        """(Re)start the listed slots at their frame 0 from s_init_rows [len(slots),114]."""
        idx = slot_list(slots, self.n, "StaggeredStreamingEngine.attach")
        rows = torch.as_tensor(s_init_rows, dtype=torch.float32).reshape(-1, 114) if len(idx) else None
        if rows is not None and rows.shape[0] != len(idx):
            raise ValueError("tip_amd.StaggeredStreamingEngine.attach: one s_init row [114] per slot")
        if not idx:
            return
        for i in idx:
            self._attach_frame[i] = self.frame
        if self.compact:            # host only: the device work goes with the next step's single upload (_flush)
            self._s_host_settle()
            self.s_host[idx] = rows
            for i in idx:
                self._attached[i] = True
                self._map_dirty |= self._positions.attach(i)
                self._pending_attach[i] = None
            return
        with torch.cuda.device(self.device):
            self.s_cur.index_copy_(0, self._to_dev(torch.tensor(idx, dtype=torch.long)), self._to_dev(rows))
        for i in idx:
            self._attached[i] = True
        self._attach_dev(idx)

    def detach(self, slots):
        """Stop the listed slots: from the next frame on they are skipped (NaN y_last row, s_rest / c_t rows unchanged)."""
        idx = slot_list(slots, self.n, "StaggeredStreamingEngine.detach")
        if not idx:
            return
        for i in idx:
            self._attached[i] = False
        if self.compact:            # host only (_flush); an unlisted slot is never ingested, so its attached flag does not matter
            for i in idx:
                self._map_dirty |= self._positions.detach(i)
                self._pending_detach[i] = None
            return
        with torch.cuda.device(self.device):
            sl = self._to_dev(torch.tensor(idx, dtype=torch.int32))
            self._call("detach", self.state.data_ptr(), self.n, sl.data_ptr(), len(idx))

    # ---- wearer hand-over (tip_amd.handover) ---------------------------------------------------------------------------------------------
    def _s_host_settle(self):
        """compact=True: the s_init rows an import_slots took from a DEVICE export reach s_host by a non-blocking copy into pinned
        memory; whoever reads or writes s_host next (an attach, a re-prime's flush) waits for that copy's event here — long past, as a
        rule — and stores the rows.  Nothing to do otherwise."""
        for ev, idx, rows in self._s_arriving:
            ev.synchronize()
            self.s_host[idx] = rows
        self._s_arriving = []

    def export_slots(self, slots):
        """The listed ATTACHED slots' wearers as they stand, for import_slots of another StaggeredStreamingEngine (tip_amd.handover; plain
        or compact, any n, the same window and model shape): a dict of device tensors — `block` [count, block bytes] (rings, pose
        average, frame counter, attached flag), the slots' rows of s_rest, c_t, y_last and T - 1, the s_init rows they were last attached
        with — and `meta`, plain numbers: window, widths, block size and each slot's age in frames (what override_history asks for).
        Exporting does not detach: that is the caller's next call.  A compact pool flushes its pending attach / detach first; then one
        launch and a few gathers on the current stream, after the last frame, no synchronisation.
        live_dropout=True: the blocks move exactly, but the dropout seeds are the ENGINE's, not the wearer's: after an import the wearer
        draws the destination's masks, so its rows differ from an uninterrupted run's (both are draws of the same model)."""
        from . import handover
        return handover.export_engine(self, slots)

    def import_slots(self, slots, exported):
        """Put exported wearers into the listed DETACHED slots (RuntimeError for an attached one; ValueError for another window, model
        shape or block size — all before anything is launched).  The slots become attached at the age they had: from the next step()
        on each continues bit for bit where it was on a plan whose per-window result does not depend on the batch (set_plan("fused"),
        compact=True's rule).  A compact pool gives each a window position as attach does (SlotPositions.attach) and uploads the map with
        the next frame's flush.  Runs on the current stream behind the previous frame, between two replays with use_graph=True: no
        pointer changes, nothing is re-captured.  No synchronisation."""
        from . import handover
        handover.import_engine(self, slots, exported)

    def _override_ready(self, idx):
        for i in idx:
            if not self._attached[i]:
                raise RuntimeError(f"tip_amd.StaggeredStreamingEngine.override_history: slot {i} is detached")
            if self.frame - self._attach_frame[i] < 6:
                raise RuntimeError(f"tip_amd.StaggeredStreamingEngine.override_history: slot {i} has not consumed a frame yet (its "
                                   "first five frames prime the smoother)")

    @property
    def attached(self):
        return list(self._attached)

    @property
    def positions(self):
        """compact=True: the slot at each window position 0 .. k-1."""
        return list(self._positions.slot_at)

    def _rows_forward(self, x_imu, x_s, rows, ws, out, advance=True):
        if self.live_dropout:
            return self._live_forward(x_imu, x_s, rows, ws, out, advance)
        return self.model.forward_rows(x_imu, x_s, rows, workspace=ws, out=out)

    def bucket(self, k: int) -> int:
        """compact=True: the batch the forward runs on with k attached slots."""
        return pool_bucket(k, self.ladder)

    def _frame_staggered(self, ws, out):
        """ingest_staggered -> forward_rows -> consume_staggered: no frame index anywhere (capturable from the first frame on).
        Launch by launch on the module's own workspace and output (ws = out = None), captured on the engine's."""
        self._call("ingest_staggered", self.state.data_ptr(), self.raw.data_ptr(), self.n, self.x_imu.data_ptr(), self.x_s.data_ptr(),
                   self.rows.data_ptr())
        mark = self._demotions()
        y_last = self._rows_forward(self.x_imu, self.x_s, self.rows, ws, out)
        if self._demotions() != mark:
            self._lost_handoff()
        self._call("consume_staggered", self.state.data_ptr(), y_last.data_ptr(), self.rows.data_ptr(), self.n, self.s_rest.data_ptr(),
                   self.c_t.data_ptr())
        return y_last

    # ---- compact pools ----------------------------------------------------------------------------------------------------------
    def _frame_mapped(self, B, ws, out):
        """ingest_mapped -> forward_rows on B windows -> consume_mapped (what a bucket's graph holds); ws / out as _frame_staggered's."""
        self._call("ingest_mapped", self.state.data_ptr(), self.raw.data_ptr(), self.n, self.slot_at.data_ptr(), B, self.x_imu.data_ptr(),
                   self.x_s.data_ptr(), self.rows.data_ptr())
        mark = self._demotions()
        y = self._rows_forward(self.x_imu[:B], self.x_s[:B], self.rows[:B], ws, out)
        if self._demotions() != mark:
            self._lost_handoff()
        self._call("consume_mapped", self.state.data_ptr(), y.data_ptr(), self.rows.data_ptr(), self.slot_at.data_ptr(), B, self.n,
                   self.s_rest.data_ptr(), self.c_t.data_ptr(), self.y_slot.data_ptr(), self.rows_slot.data_ptr())
        return y

    def _flush(self):
        """The attach / detach calls since the last frame, on the device: one non-blocking copy from pinned memory (stage_image:
        position map, slot lists, s_init rows), the attach kernel, and NaN / -1 into the y_last / T rows of the detached slots (no
        kernel writes the rows of a slot that is not listed).  Stream order puts it after the previous frame and before this one."""
        if not (self._map_dirty or self._pending_attach or self._pending_detach):
            return
        att, det = list(self._pending_attach), list(self._pending_detach)
        if att:
            self._s_host_settle()
        h, (o_att, o_det, o_rows) = stage_image(self.n, self._positions.slot_at, att, det, self.s_host[att].numpy())
        self._stage[: h.size].copy_(torch.from_numpy(h).pin_memory(), non_blocking=True)
        base = self._stage.data_ptr()
        if att:
            self._call("attach", self.state.data_ptr(), self.n, base + 4 * o_att, base + 4 * o_rows, len(att))
        if det:
            sl = self._stage[o_det: o_rows].view(torch.int64)
            self.y_slot.index_fill_(0, sl, float("nan"))
            self.rows_slot.index_fill_(0, sl, -1)
        self._map_dirty = False
        self._pending_attach, self._pending_detach = {}, {}

    def _warm_forward(self, B):
        if isinstance(B, tuple):                # (a device-fed frame, ("fed", B): the same forward)
            B = B[1]
        B = self.n if B is None else B          # (the plain engine: all n windows)
        self._rows_forward(self.x_imu[:B], self.x_s[:B], self.rows[:B], self._graph_ws, self._graph_y[:B], advance=False)

    def _captured_frame(self, B):
        ws, y = self._graph_ws, self._graph_y
        if isinstance(B, tuple):
            return self._frame_fed(B[1], ws, y[:B[1]])
        return self._frame_staggered(ws, y) if B is None else self._frame_mapped(B, ws, y[:B])

    # ---- device-fed frames (tip_amd.replay) -----------------------------------------------------------------------------------------
    def _frame_fed(self, B, ws, out):
        """feed -> _frame_mapped -> collect: `raw` is filled on the device by the feeder's first launch and the slots' rows are taken
        away by its second (self._fed: two callables that launch on the current stream with no argument that changes from frame to
        frame).  What a device-fed bucket's graph holds, under the key ("fed", B)."""
        feed, collect = self._fed
        feed()
        y = self._frame_mapped(B, ws, out)
        collect()
        return y

    @torch.no_grad()
    def _step_fed(self):
        """_step_compact for a frame whose `raw` the device fills itself (set_feeder): the same flush, the same capture and replay — one
        captured frame per bucket, feed and collect inside it — and the same hand-off poll, but no host frame, no copy into `raw` and no
        per-frame result (the feeder's collect launch owns the outputs; nothing is launched for T / valid).  Returns (k, B);
        fed_frames counts the frames that launched."""
        if self.model.training and not self.live_dropout:
            raise RuntimeError("tip_amd.StaggeredStreamingEngine needs model.eval() (the inference kernels: forward_rows)")
        k = len(self._positions)
        B = self.bucket(k)
        with torch.cuda.device(self.device):
            self._flush()
            if k:
                if self.use_graph:
                    self._replay(("fed", B))
                else:
                    self._frame_fed(B, None, None)
                self.fed_frames += 1
        self.frame += 1
        return k, B

    def set_feeder(self, feed, collect):
        """Install the two launches _step_fed puts around the engine's frame; captured device-fed frames are dropped (they hold the
        previous feeder's pointers).  compact=True only."""
        if not self.compact:
            raise RuntimeError("tip_amd.StaggeredStreamingEngine.set_feeder: compact=True only")
        self._fed = (feed, collect)
        self._graphs = {key: e for key, e in self._graphs.items() if not isinstance(key, tuple)}

    @torch.no_grad()
    def prewarm(self, buckets=None):
        """compact=True, use_graph=True: capture the frame of every bucket (default: the whole ladder) now, so that no capture
        happens on the hot path.  Without use_graph there is nothing to capture."""
        if not self.compact:
            raise RuntimeError("tip_amd.StaggeredStreamingEngine.prewarm: compact=True only (the plain engine has one graph)")
        bs = self.ladder if buckets is None else [int(b) for b in buckets]
        if any(b not in self.ladder for b in bs):
            raise ValueError(f"tip_amd.StaggeredStreamingEngine.prewarm: buckets must come from the ladder {self.ladder}")
        if not self.use_graph:
            return
        with torch.cuda.device(self.device):
            for B in bs:
                if B not in self._graphs:
                    self._capture(B)

    def _step_compact(self):
        k = len(self._positions)
        B = self.bucket(k)
        with torch.cuda.device(self.device):
            self._flush()
            if k:
                if self.use_graph:
                    self._replay(B)
                else:
                    self._frame_mapped(B, None, None)
            T = self.rows_slot + 1
        self.frame += 1
        return {"s_rest": self.s_rest, "c_t": self.c_t, "y_last": self.y_slot, "T": T, "valid": T > 0, "active": k, "batch": B}

    def _needs_eval(self):
        if self.model.training and not self.live_dropout:
            raise RuntimeError("tip_amd.StaggeredStreamingEngine needs model.eval() (the inference kernels: forward_rows)")

    @torch.no_grad()
    def step(self, raw_imu: torch.Tensor) -> dict:
        self._needs_eval()
        if not self.compact or len(self._positions):          # (a compact pool with nothing attached launches nothing)
            self.raw.copy_(torch.as_tensor(raw_imu, dtype=torch.float32).reshape(self.n, 72), non_blocking=True)
        return self._step_filled()

    @torch.no_grad()
    def step_packets(self, front, packets) -> dict:
        """step() from raw IMU packets [n, 42] (tip_amd.sensors.SensorFrontEnd): one tip_sensor_transform launch fills the engine's
        `raw` on the device, then the frame runs as step() runs it, plain and compact, launch by launch and replayed.  Every ATTACHED
        slot must be live in `front` (its host mirror; RuntimeError otherwise, nothing launched); a detached slot may be anywhere in
        its calibration — its holds run between the frames of the others (front.accumulate) — and its NaN row is never ingested."""
        self._needs_eval()
        self._packets_to_raw(front, packets, [i for i in range(self.n) if self._attached[i]],
                             launch=not self.compact or len(self._positions) > 0)
        return self._step_filled()

    def _step_filled(self) -> dict:
        """The frame behind "self.raw is filled"."""
        if self.compact:
            return self._step_compact()
        with torch.cuda.device(self.device):
            if self.use_graph:
                self._replay(None)
                y_last = self._y_last
            else:
                y_last = self._frame_staggered(None, None)
            T = self.rows + 1
        self.frame += 1
        return {"s_rest": self.s_rest, "c_t": self.c_t, "y_last": y_last, "T": T, "valid": T > 0}
