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

from typing import Sequence

import numpy as np

from .kinematics import Skeleton, _Blocks, _Tracker, _device, _ragged_scales, _track_ragged

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


class _State(_Blocks):
    """n blocks on a device (tip_terrain_state_bytes) and the launches on them."""
    _reset_fn, _track_fn = "tip_terrain_reset", "tip_terrain_track"

    def __init__(self, skel, n, device, map_bound, grid_size, multi_sbp, max_regions, who):
        super().__init__(skel, n, device)
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
        self.stride = self._alloc("tip_terrain_state_bytes", self.G, self.M) // max(self.n, 1)
        self._reset_args, self._track_args, self._track_tail = (self.G, self.M), (self.G, self.M, self.D, self.grid_size), (self.flags,)

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
                  multi_sbp: bool = False, max_regions: int = 64, chunk=None, device=None, scales=None):
    """R sequences back to back: s_init [R, 114], s_rest [N, 111], c_t [N, 8 | 20], valid [N] bool, offsets [R + 1] ->
    root [N, 3], viz_locs [N, 5, 3], q_hist [N, 54] (float32), fire [N] (int32: the sequence's index where the IK rewrote the pose, else
    -1) on the device, and the TerrainStates: the rows of RTRunner.step's qdq[:3] and viz_locs and the pose it feeds back, one kernel
    for the lot.  chunk=k runs it k rows of every sequence per launch instead, through the state: the same bits.
    scales [R]: the sequences' body scales (tip_amd.kinematics: every joint and COM offset times the scale, nothing else — not the map's
    bound or grid, not the 0.2 m pelvis test, not the IK's thresholds); None is the unscaled kernels."""
    import torch
    scales = _ragged_scales("terrain", "track_terrain", scales, offsets)
    device = _device(device)

    def make(n, R):
        return (_State(skel, R, device, map_bound, grid_size, multi_sbp, max_regions, "track_terrain"),
                (torch.empty((n, 3), dtype=torch.float32, device=device), torch.empty((n, 5, 3), dtype=torch.float32, device=device),
                 torch.empty((n, 54), dtype=torch.float32, device=device), torch.full((n,), -1, dtype=torch.int32, device=device)))

    with torch.cuda.device(device):
        st, outs = _track_ragged("terrain", "track_terrain", s_init, s_rest, c_t, valid, offsets, device, chunk, make,
                                 lambda c: _check_width(c, multi_sbp, "track_terrain"), scales=scales)
    return (*outs, TerrainStates(st))


class TerrainTracker(_Tracker):
    """The live form: n blocks beside an engine of n slots.
        tt = TerrainTracker(skel, engine.n, engine.device, map_bound=5.0, grid_size=0.1, multi_sbp=True)
        tt.reset(None, s_init)                 # with the engine's s_init; reset(slots, rows) whenever the engine attaches those slots
        out = engine.step(frame)
        root, viz_locs = tt.step(out)          # [n, 3], [n, 5, 3] by slot; tt.q_hist [n, 54] and tt.fire [n] int32 (tensors reused every frame)
        tt.feed_back(engine)                   # engine.override_history_device(tt.q_hist, tt.fire): the IK's pose into the history
    step() is ONE launch on the current stream (call it on the engine's stream, after step; it is not part of the engine's captured
    graph).  out=None — a lock-step engine that is still priming — launches nothing.  Rows whose out["valid"] is False keep their
    state and read (the state's root, 100s, fire -1).  With a `slots` subset the slots left out keep their state too, and their fire
    entries are set to -1 first (one fill more), so that feed_back never repeats an old correction.
    A pool of wearers of different heights: tt.reset(slots, rows, scales=[kinematics.scale_of_height(h), ...]) — every wearer's residue,
    map and IK pose on legs of the wearer's own length, still one launch per frame."""
    _mod, _name, _slot_who = "terrain", "TerrainTracker", "terrain.TerrainTracker"

    def __init__(self, skel: Skeleton, n: int, device, map_bound: float = 5.0, grid_size: float = 0.1, multi_sbp: bool = False,
                 max_regions: int = 64):
        import torch
        super().__init__(n, lambda n: _State(skel, n, device, map_bound, grid_size, multi_sbp, max_regions, "TerrainTracker"))
        self.multi_sbp = bool(multi_sbp)
        with torch.cuda.device(self.device):
            self.q_hist = torch.zeros((self.n, 54), dtype=torch.float32, device=self.device)
            self.fire = torch.full((self.n,), -1, dtype=torch.int32, device=self.device)
        self._outs += (self.q_hist, self.fire)

    def reset(self, slots, s_init_rows, scales=None):
        """The listed slots (None: all) start over from s_init_rows [len(slots), 114], as RTRunner.__init__ starts: root = s_init[:3],
        pq_prev = FK(s_init), an empty map.  scales [len(slots)]: the body scales of the wearers these slots take, as
        RootTracker.reset's (tt.scale [n] on the device; step and feed_back are as they were)."""
        super().reset(slots, s_init_rows, scales)

    def _reset_rows(self, rows):
        self.fire[rows] = -1

    def _check_width(self, c):
        _check_width(c, self.multi_sbp, "TerrainTracker.step")

    def _before_subset_step(self):
        import torch
        with torch.cuda.device(self.device):
            self.fire.fill_(-1)

    def feed_back(self, engine):
        """The pose the IK corrected on this frame into `engine`'s history, for the slots it fired on; nothing is read by the host."""
        engine.override_history_device(self.q_hist, self.fire)

    def state(self, slot: int) -> TerrainState:
        """A downloaded copy of one slot's block (this synchronises: for rendering and tests, not for the loop)."""
        return self._s.view(slot)

    def state_bytes(self) -> np.ndarray:
        """The whole buffer [n, block] as downloaded bytes."""
        return self._s.buf[:self.n * self._s.stride].cpu().numpy().reshape(self.n, self._s.stride)
