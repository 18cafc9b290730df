"""The full runner on the device: RTRunner's terrain map, height correction and leg IK (csrc/tip_terrain.hip; include/tip_hip.h,
"terrain").

tip_amd.kinematics tracks what RTRunnerMin.step does behind the model.  RTRunner.step (real_time_runner.py:451-496) — the runner
live_demo_new.py and offline_testing_simple.py start — does more: per stream a height-REGION map that the feet (and, with
multi_sbp_terrain_and_correction, the root) write when a contact ends or has lasted 50 frames (:140-277), a vertical root correction
from that map (:467-472), and a two-joint leg IK that pulls the ankles back to where their contacts hold them (:334-382;
data_utils.py:556-630).  The pose the IK corrects is not the one the runner returns: it is the one it feeds back into the model's
history (:483-495).  All of it is built as a CONSUMER beside the engines, as RootTracker is — no engine kernel, graph or number moves:

    root, viz_locs, q_hist, fire, states = track_terrain(skel, s_init, s_rest, c_t, valid, offsets)      # R ragged sequences, one kernel
    traj = kinematics.track_replay(skel, out, s_init, terrain=dict(map_bound=5.0, grid_size=0.1))       # the script's setting (:169-176)

    tt = TerrainTracker(skel, engine.n, engine.device, map_bound=5.0, grid_size=0.1, multi_sbp=True)
    tt.reset(None, s_init)
    out = engine.step(frame); root, viz_locs = tt.step(out); tt.feed_back(engine)      # three enqueues, no synchronisation

feed_back is engine.override_history_device(tt.q_hist, tt.fire): tt.fire holds the slot index where the IK rewrote the pose on this
frame and -1 elsewhere, and tip_stream_history_override skips entries below 0, so the host never reads the list.

grid_num and diffuse_region are the reference's own expressions (:115, :128), evaluated here and passed as integers.  The decisions the
reference leaves open (a patch off the map, more regions than max_regions, ties, two-SBP models, non-finite rows) are listed in the
header.  Precision as the tracker's: FK fp32, everything behind it fp64, outputs fp32.  PyBullet and fairmotion parity are unpinned, as
everywhere (tests/golden/make_terrain_golden.py).  IK feedback for recorded files runs inside the replay pool's frame:
tip_amd.replay.ReplayPool(terrain=dict(skel=..., multi_sbp=True, ...)).  play_back_gt (real_time_runner.py:396-401) takes s_t and c_t from
the ground truth instead of the model and runs the same tail: it is track_terrain on ground-truth rows.  Out of scope: the arm IK the
reference never calls."""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np

from .kinematics import Skeleton, _check, _dev_f32, _device, _lib, _offsets, _stream, _track_inputs

HEAD_BYTES = 1280                   # include/tip_hip.h, "terrain": the block's fixed part


def grid_num(map_bound: float, grid_size: float) -> int:
    return int(map_bound / grid_size) * 2                    # real_time_runner.py:115


def diffuse_region(grid_size: float) -> int:
    return round(0.5 / grid_size)                            # real_time_runner.py:128


def _leg_chains_ok(skel: Skeleton) -> bool:
    """Both ankles hang below three spherical links (ankle, knee, hip) — what the device's IK asks of the table."""
    for ank in (int(skel.sbp[0]), int(skel.sbp[1])):
        b = ank
        for _ in range(3):
            if b < 1 or skel.state_col[b - 1] < 3:
                return False
            b = int(skel.parent[b - 1])
    return True


class TerrainState:
    """One slot's block as numpy views of a downloaded copy: region_map [G, G], height_map [G, G] (region_height[region_map]),
    region_height / region_weight [n_regions], ticks [3] (lankle, rankle, root), ik_deltas [2, 3], off_map, regions_full, root [3]
    (fp64), and `bytes`, the block itself."""

    def __init__(self, block: np.ndarray, G: int, max_regions: int):
        self.bytes = block
        self.root = block[:24].view("<f8")
        self.c_locs_prev = block[1024:1144].view("<f8").reshape(5, 3)
        self.ik_deltas = block[1144:1192].view("<f8").reshape(2, 3)
        words = block[1192:1224].view("<i4")
        self.ticks = words[:3]
        self.n_regions, self.off_map, self.regions_full = int(words[3]), int(words[4]), int(words[5])
        h0 = HEAD_BYTES
        self.region_height = block[h0:h0 + 8 * max_regions].view("<f8")[:self.n_regions]
        self.region_weight = block[h0 + 8 * max_regions:h0 + 16 * max_regions].view("<f8")[:self.n_regions]
        cells = block[h0 + 16 * max_regions:h0 + 16 * max_regions + 4 * G * G].view("<u4").reshape(G, G)
        self.region_map = (cells >> 16).astype(np.int32)
        self.d2_map = (cells & 0xFFFF).astype(np.int32)

    @property
    def height_map(self):
        return self.region_height[np.minimum(self.region_map, self.n_regions - 1)]


class _State:
    """n blocks on a device (tip_terrain_state_bytes) and the launches on them."""

    def __init__(self, skel, n, device, map_bound, grid_size, multi_sbp, max_regions, who):
        import torch
        self.skel, self.n, self.device = skel, int(n), _device(device)
        self.grid_size = float(grid_size)
        if not (self.grid_size > 0 and float(map_bound) > 0):
            raise ValueError(f"tip_amd.terrain.{who}: map_bound and grid_size are lengths in metres, above 0; got {map_bound!r}, {grid_size!r}")
        self.G, self.D, self.M = grid_num(map_bound, grid_size), diffuse_region(grid_size), int(max_regions)
        if not (1 <= self.D <= 16 and 2 * self.D <= self.G <= 4096):
            raise ValueError(f"tip_amd.terrain.{who}: map_bound {map_bound!r} / grid_size {grid_size!r} give a map of {self.G} cells a side "
                             f"and patches of {2 * self.D}; served: patches of 2 .. 32 cells inside a map of at most 4096")
        if not 1 <= self.M <= 65535:
            raise ValueError(f"tip_amd.terrain.{who}: max_regions is 1 .. 65535; got {max_regions!r}")
        self.flags = 1 if multi_sbp else 0
        if multi_sbp and not _leg_chains_ok(skel):
            raise ValueError(f"tip_amd.terrain.{who}: multi_sbp needs both ankles below three spherical links (hip, knee, ankle)")
        self.tlib, self.lib = _lib()
        nbytes = ctypes.c_size_t()
        _check(self.lib.tip_terrain_state_bytes(self.n, self.G, self.M, ctypes.byref(nbytes)))
        self.stride = nbytes.value // max(self.n, 1)
        with torch.cuda.device(self.device):
            self.buf = torch.zeros(max(nbytes.value, 8), dtype=torch.uint8, device=self.device)
            self.sk = skel.on(self.device)

    def reset(self, slots_dev, count, s_init_dev):
        import torch
        with torch.cuda.device(self.device):
            _check(self.lib.tip_terrain_reset(self.sk.data_ptr(), self.buf.data_ptr(), self.n, self.G, self.M,
                                              None if slots_dev is None else slots_dev.data_ptr(), count, s_init_dev.data_ptr(),
                                              _stream(self.device)))

    def track(self, slots_dev, begin_ptr, end_ptr, count, s_rest, c_t, valid, root, viz, q_hist, fire):
        import torch
        with torch.cuda.device(self.device):
            _check(self.lib.tip_terrain_track(self.sk.data_ptr(), self.buf.data_ptr(), self.n, self.G, self.M, self.D, self.grid_size,
                                              None if slots_dev is None else slots_dev.data_ptr(), begin_ptr, end_ptr, count,
                                              int(s_rest.shape[0]), s_rest.data_ptr(), c_t.data_ptr(), int(c_t.shape[1]),
                                              None if valid is None else valid.data_ptr(), self.flags, root.data_ptr(), viz.data_ptr(),
                                              q_hist.data_ptr(), fire.data_ptr(), _stream(self.device)))

    def view(self, slot: int) -> TerrainState:
        slot = int(slot)
        if not 0 <= slot < self.n:
            raise ValueError(f"tip_amd.terrain: slot index outside [0, {self.n})")
        block = self.buf[slot * self.stride:(slot + 1) * self.stride].cpu().numpy()
        return TerrainState(block, self.G, self.M)


class TerrainStates(Sequence):
    """track_terrain's states, one TerrainState per sequence, downloaded when first asked for; `bytes` [R, block] is the buffer."""

    def __init__(self, st: _State):
        self._st, self._host = st, None

    @property
    def bytes(self) -> np.ndarray:
        if self._host is None:
            self._host = self._st.buf[:self._st.n * self._st.stride].cpu().numpy().reshape(self._st.n, self._st.stride)
        return self._host

    def __len__(self):
        return self._st.n

    def __getitem__(self, i):
        return TerrainState(self.bytes[range(self._st.n)[i]], self._st.G, self._st.M)


def _check_width(c, multi_sbp, who):
    if multi_sbp and c.shape[1] != 20:
        raise ValueError(f"tip_amd.terrain.{who}: multi_sbp corrects by the root's SBP, which a two-SBP model (c_t of 8 columns) does not "
                         "have (the reference indexes a fifth SBP there)")


def track_terrain(skel: Skeleton, s_init, s_rest, c_t, valid, offsets, map_bound: float = 5.0, grid_size: float = 0.1,
                  multi_sbp: bool = False, max_regions: int = 64, chunk=None, device=None):
    """R sequences back to back: s_init [R, 114], s_rest [N, 111], c_t [N, 8 | 20], valid [N] bool, offsets [R + 1] ->
    root [N, 3], viz_locs [N, 5, 3], q_hist [N, 54] (float32), fire [N] (int32: the sequence's index where the IK rewrote the pose, else
    -1) on the device, and the TerrainStates: the rows of RTRunner.step's qdq[:3] and viz_locs and the pose it feeds back, one kernel
    for the lot.  chunk=k runs it k rows of every sequence per launch instead, through the state: the same bits."""
    import torch
    device = _device(device)
    with torch.cuda.device(device):
        s, c, v = _track_inputs(s_rest, c_t, valid, device, "track_terrain")
        _check_width(c, multi_sbp, "track_terrain")
        o = _offsets(offsets, int(s.shape[0]), "track_terrain")
        R = o.shape[0] - 1
        s0 = _dev_f32(s_init if np.ndim(s_init) == 2 else np.asarray(s_init)[None], device, (114,), "track_terrain", "s_init")
        if s0.shape[0] != R:
            raise ValueError(f"tip_amd.terrain.track_terrain: s_init is [R, 114] with one row per sequence ({R}); got {tuple(s0.shape)}")
        n = int(s.shape[0])
        root = torch.empty((n, 3), dtype=torch.float32, device=device)
        viz = torch.empty((n, 5, 3), dtype=torch.float32, device=device)
        q_hist = torch.empty((n, 54), dtype=torch.float32, device=device)
        fire = torch.full((n,), -1, dtype=torch.int32, device=device)
        st = _State(skel, R, device, map_bound, grid_size, multi_sbp, max_regions, "track_terrain")
        if R == 0 or n == 0:
            return root, viz, q_hist, fire, TerrainStates(st)
        st.reset(None, R, s0)
        if chunk is None:
            od = torch.from_numpy(o).pin_memory().to(device, non_blocking=True)
            st.track(None, od.data_ptr(), od.data_ptr() + 8, R, s, c, v, root, viz, q_hist, fire)
        else:
            k = int(chunk)
            if k < 1:
                raise ValueError(f"tip_amd.terrain.track_terrain: chunk is a number of rows, at least 1; got {chunk!r}")
            for first in range(0, int(np.diff(o).max()), k):
                be = np.stack([np.minimum(o[:-1] + first, o[1:]), np.minimum(o[:-1] + first + k, o[1:])])
                bd = torch.from_numpy(be).pin_memory().to(device, non_blocking=True)
                st.track(None, bd[0].data_ptr(), bd[1].data_ptr(), R, s, c, v, root, viz, q_hist, fire)
    return root, viz, q_hist, fire, TerrainStates(st)


class TerrainTracker:
    """The live form: n blocks beside an engine of n slots.
        tt = TerrainTracker(skel, engine.n, engine.device, map_bound=5.0, grid_size=0.1, multi_sbp=True)
        tt.reset(None, s_init)                 # with the engine's s_init; reset(slots, rows) whenever the engine attaches those slots
        out = engine.step(frame)
        root, viz_locs = tt.step(out)          # [n, 3], [n, 5, 3] by slot; tt.q_hist [n, 54] and tt.fire [n] int32 (tensors reused every frame)
        tt.feed_back(engine)                   # engine.override_history_device(tt.q_hist, tt.fire): the IK's pose into the history
    step() is ONE launch on the current stream (call it on the engine's stream, after step; it is not part of the engine's captured
    graph).  out=None — a lock-step engine that is still priming — launches nothing.  Rows whose out["valid"] is False keep their
    state and read (the state's root, 100s, fire -1).  With a `slots` subset the slots left out keep their state too, and their fire
    entries are set to -1 first (one fill more), so that feed_back never repeats an old correction."""

    def __init__(self, skel: Skeleton, n: int, device, map_bound: float = 5.0, grid_size: float = 0.1, multi_sbp: bool = False,
                 max_regions: int = 64):
        import torch
        self.n = int(n)
        if self.n < 1:
            raise ValueError(f"tip_amd.terrain.TerrainTracker: n is the number of slots, at least 1; got {n!r}")
        self._s = _State(skel, self.n, device, map_bound, grid_size, multi_sbp, max_regions, "TerrainTracker")
        self.device, self.multi_sbp = self._s.device, bool(multi_sbp)
        with torch.cuda.device(self.device):
            self.root = torch.zeros((self.n, 3), dtype=torch.float32, device=self.device)
            self.viz_locs = torch.full((self.n, 5, 3), 100.0, dtype=torch.float32, device=self.device)
            self.q_hist = torch.zeros((self.n, 54), dtype=torch.float32, device=self.device)
            self.fire = torch.full((self.n,), -1, dtype=torch.int32, device=self.device)
            self._rows = torch.arange(self.n + 1, dtype=torch.int64, device=self.device)
        self._lists = {}

    def _slot_tensors(self, slots, who):
        import torch
        from .streaming import slot_list
        idx = tuple(slot_list(slots, self.n, f"terrain.TerrainTracker.{who}"))
        if idx not in self._lists:
            with torch.cuda.device(self.device):
                a = np.array(idx, dtype=np.int64)
                host = torch.from_numpy(np.stack([a, a + 1])).pin_memory()
                self._lists[idx] = (torch.from_numpy(a.astype(np.int32)).pin_memory().to(self.device, non_blocking=True),
                                    host.to(self.device, non_blocking=True))
        return idx, self._lists[idx]

    def reset(self, slots, s_init_rows):
        """The listed slots (None: all) start over from s_init_rows [len(slots), 114], as RTRunner.__init__ starts: root = s_init[:3],
        pq_prev = FK(s_init), an empty map."""
        import torch
        with torch.cuda.device(self.device):
            if slots is None:
                count, sl = self.n, None
            else:
                idx, (sl, _) = self._slot_tensors(slots, "reset")
                count = len(idx)
            s0 = _dev_f32(s_init_rows if np.ndim(s_init_rows) == 2 else np.asarray(s_init_rows)[None], self.device, (114,),
                          "TerrainTracker.reset", "s_init_rows")
            if s0.shape[0] != count:
                raise ValueError(f"tip_amd.terrain.TerrainTracker.reset: s_init_rows is [{count}, 114]; got {tuple(s0.shape)}")
            if count:
                self._s.reset(sl, count, s0)
                rows = slice(None) if sl is None else sl.long()
                self.root[rows] = s0[:, :3]
                self.viz_locs[rows] = 100.0
                self.fire[rows] = -1

    def step(self, out, slots=None):
        import torch
        if out is None:
            return self.root, self.viz_locs
        s, c, v = out["s_rest"], out["c_t"], out.get("valid")
        if tuple(s.shape) != (self.n, 111) or s.device != self.device or c.shape[0] != self.n or not s.is_contiguous() or not c.is_contiguous():
            raise ValueError(f"tip_amd.terrain.TerrainTracker.step: out is an engine's frame of {self.n} slots on {self.device}")
        if v is not None and not (isinstance(v, torch.Tensor) and v.dtype in (torch.bool, torch.uint8) and v.shape == (self.n,)):
            raise ValueError("tip_amd.terrain.TerrainTracker.step: out['valid'] is a bool tensor [n]")
        _check_width(c, self.multi_sbp, "TerrainTracker.step")
        if slots is None:
            self._s.track(None, self._rows.data_ptr(), self._rows.data_ptr() + 8, self.n, s, c, v, self.root, self.viz_locs, self.q_hist,
                          self.fire)
        else:
            idx, (sl, be) = self._slot_tensors(slots, "step")
            with torch.cuda.device(self.device):
                self.fire.fill_(-1)
            if idx:
                self._s.track(sl, be[0].data_ptr(), be[1].data_ptr(), len(idx), s, c, v, self.root, self.viz_locs, self.q_hist, self.fire)
        return self.root, self.viz_locs

    def feed_back(self, engine):
        """The pose the IK corrected on this frame into `engine`'s history, for the slots it fired on; nothing is read by the host."""
        engine.override_history_device(self.q_hist, self.fire)

    def state(self, slot: int) -> TerrainState:
        """A downloaded copy of one slot's block (this synchronises: for rendering and tests, not for the loop)."""
        return self._s.view(slot)

    def state_bytes(self) -> np.ndarray:
        """The whole buffer [n, block] as downloaded bytes."""
        return self._s.buf[:self.n * self._s.stride].cpu().numpy().reshape(self.n, self._s.stride)
