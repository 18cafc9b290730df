"""Kinematics on the device: forward kinematics of the character, the root track with its stationary-body-point (SBP) correction, and
the evaluation script's seven metrics (csrc/tip_kin.hip; include/tip_hip.h, "kinematics").

The streaming engines and ReplayPool stop at s_rest and c_t — qdq[3:114] of the reference runner.  What RTRunnerMin.step does behind
that (real_time_runner_minimal.py:159-194: integrate the root, PyBullet FK, correct the root by the active SBPs, place the SBP
markers) and what offline_testing_simple.py --compare_gt does with whole trajectories (:422-453: FK of every frame, seven numbers per
file) never feeds back into the model, so it is built as a CONSUMER of the engines' outputs, beside them:

    skel = Skeleton.from_urdf("data/amass.urdf", amass_char_info)        # the user's checkout of the reference; or from_table(npz)
    pq_g = fk(skel, q)                                                   # [N, >= 57] -> [N, L + 1, 7] COM poses (out_jf=True: + link frames)
    out = ReplayPool(model).run(recordings, s_init)
    traj = track_replay(skel, out, s_init)                               # [(qdq [L_i, 114], viz_locs [L_i, 5, 3])]: the script's s_traj_pred rows
    m = evaluate(skel, pred_qdq, gt_qdq, offsets)                        # [R, 7]: angle, j_pos, root_2s, root_5s, root_10s, jerk, root_jerk

    rt = RootTracker(skel, n, device); rt.reset(None, s_init)            # live: one launch per frame, beside the engine
    o = engine.step(frame); root, viz_locs = rt.step(o)                  # on the engine's stream, after step; never inside its graph

A pose is xyz + (x, y, z, w).  FK is fp32; the tracker's scan and root accumulator are fp64 on the fp32 poses, its outputs fp32; the
metrics are fp64 sums.  One detail of the runner the tracker has to undo: :159 integrates the root velocity as predicted, while
s_rest[54:57] is that velocity after the pose averaging of :165-166 — so v = 2 s_rest[54:57] - (the previous valid row's).

Wearers differ in size.  The reference builds its character with scale = h / 1.6 (scale_of_height), and the runners run on the character
they are given; `scale` / `scales` everywhere here is that: every link's joint and COM offset times the wearer's scale before it is
rotated, and nothing else (not the root, not c_t's vectors, no threshold).  fk takes one scale per row, the trackers one per sequence or
slot, set when a slot is reset and at no other time (the carry's pq_prev was computed with it).  scales=None is the unscaled code path,
launch for launch and bit for bit; with scales the *_scaled entries of the library run (kernel instantiations of their own).

RTRunner's terrain map, height correction and leg IK (real_time_runner.py:140-262, 334-382) are tip_amd.terrain, the same kind of
consumer over the same FK; track_replay(..., terrain=dict(map_bound=..., grid_size=...)) routes a replay through it."""
from __future__ import annotations

import ctypes
import xml.etree.ElementTree as ET
from typing import List, Sequence

import numpy as np

DT = 1.0 / 60                       # constants.py:7
MAX_LINKS = 32
SBP_BODIES = ("lankle", "rankle", "lwrist", "rwrist", "root")      # get_cur_step_root_correction_from_all_constr (data_utils.py:502-508)
IMU_BODIES = ("root", "lwrist", "rwrist", "lknee", "rknee", "upperneck")      # data-gen-and-viz-bullet-new.py:157-165 (the knee setting)
METRICS = ("angle", "j_pos", "root_2s", "root_5s", "root_10s", "jerk", "root_jerk")      # offline_testing_simple.py:439-445
_SKEL_DTYPE = np.dtype([("parent", "<i4"), ("state_col", "<i4"), ("joint_xyz", "<f4", 3), ("joint_q", "<f4", 4), ("com_xyz", "<f4", 3)])


def _floats(el, attr, who):
    text = "0 0 0" if el is None else el.get(attr, "0 0 0")
    v = [float(x) for x in text.split()]
    if len(v) != 3:
        raise ValueError(f"tip_amd.kinematics.Skeleton.from_urdf: {who} {attr}={text!r} is not three numbers")
    return np.array(v, dtype=np.float64)


def _rpy_quat(rpy):
    """URDF roll-pitch-yaw (fixed axes x, y, z: R = Rz Ry Rx) as (x, y, z, w)."""
    cr, sr, cp, sp, cy, sy = (f(a / 2) for a in rpy for f in (np.cos, np.sin))
    return np.array([sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy])


class Skeleton:
    """The root and L links in URDF (= PyBullet) order; bodies are numbered 0 (the root) and i + 1 (link i).
    parent [L] (body index, always below the link's own), joint_xyz [L, 3] and joint_q [L, 4] (the joint origin in the parent's link
    frame), com_xyz [L, 3] (the inertial origin), state_col [L] (the column of the 57-wide q where the link's axis-angle starts, -1
    for a fixed joint), sbp [5] (body indices of lankle, rankle, lwrist, rwrist, root), names [L + 1]; imu [6] (body indices of root,
    lwrist, rwrist, lknee, rknee, upperneck) or None: only tip_amd.syndata asks for it."""

    def __init__(self, parent, joint_xyz, joint_q, com_xyz, state_col, sbp, names=None, imu=None):
        who = "tip_amd.kinematics.Skeleton"
        self.parent = np.asarray(parent, dtype=np.int32).reshape(-1)
        L = self.n_links = int(self.parent.shape[0])
        if L > MAX_LINKS:
            raise ValueError(f"{who}: {L} links; the device table holds {MAX_LINKS}")
        self.joint_xyz = np.asarray(joint_xyz, dtype=np.float64).reshape(L, 3)
        self.joint_q = np.asarray(joint_q, dtype=np.float64).reshape(L, 4)
        self.com_xyz = np.asarray(com_xyz, dtype=np.float64).reshape(L, 3)
        self.state_col = np.asarray(state_col, dtype=np.int32).reshape(L)
        self.sbp = np.asarray(sbp, dtype=np.int32).reshape(-1)
        self.names = [str(n) for n in (names if names is not None else ["root"] + [f"link{i}" for i in range(L)])]
        if self.sbp.shape[0] != 5 or (self.sbp < 0).any() or (self.sbp > L).any():
            raise ValueError(f"{who}: sbp is five body indices in 0 .. {L} (lankle, rankle, lwrist, rwrist, root); got {self.sbp.tolist()}")
        if any(p < 0 or p > i for i, p in enumerate(self.parent)):
            raise ValueError(f"{who}: a link's parent comes before it (body index 0 .. i for link i); got {self.parent.tolist()}")
        if any(c != -1 and not 3 <= c <= 54 for c in self.state_col):
            raise ValueError(f"{who}: state_col is -1 (fixed) or a column 3 .. 54 of the 57-wide q; got {self.state_col.tolist()}")
        if len(self.names) != L + 1:
            raise ValueError(f"{who}: names is the root's and the {L} links'")
        self.imu = None if imu is None else np.asarray(imu, dtype=np.int32).reshape(-1)
        if self.imu is not None and (self.imu.shape[0] != 6 or (self.imu < 0).any() or (self.imu > L).any()):
            raise ValueError(f"{who}: imu is six body indices in 0 .. {L} (root, lwrist, rwrist, lknee, rknee, upperneck); got "
                             f"{self.imu.tolist()}")
        self._dev = {}

    @classmethod
    def from_table(cls, table):
        """From a dict or an open .npz with the arrays parent, joint_xyz, joint_q, com_xyz, state_col, sbp and (optionally) names and
        imu — plain or under a "table/" prefix, as tests/golden/tip_kin_golden.npz keeps them (that one has no imu: it serves
        everything here, and tip_amd.syndata says what is missing)."""
        keys = set(table.keys()) if hasattr(table, "keys") else set(table.files)
        pre = "table/" if "table/parent" in keys else ""
        need = ("parent", "joint_xyz", "joint_q", "com_xyz", "state_col", "sbp")
        missing = [k for k in need if pre + k not in keys]
        if missing:
            raise ValueError(f"tip_amd.kinematics.Skeleton.from_table: missing {missing}")
        return cls(*[table[pre + k] for k in need], names=table[pre + "names"] if pre + "names" in keys else None,
                   imu=table[pre + "imu"] if pre + "imu" in keys else None)

    @classmethod
    def from_urdf(cls, path, char_info):
        """Parse a URDF of spherical and fixed joints.  char_info is the reference's character module (amass_char_info.py of the user's
        checkout): joint_idx names the links in PyBullet order, nimble_state_map gives the state columns by our_pose_2_bullet_format's
        rule (data_utils.py:246-259: (nimble_state_map[idx] - 1) * 3 + 6), and lankle, rankle, lwrist, rwrist, root are the SBP bodies;
        lknee, rknee and upperneck, where char_info names them, complete the IMU bodies.
        Refused: an inertial rpy that is not zero (the COM frame would be turned against the link's), a root inertial origin that is
        not zero, any other joint type, more than 32 links."""
        who = "tip_amd.kinematics.Skeleton.from_urdf"
        robot = ET.parse(path).getroot()
        links = {ln.get("name"): ln for ln in robot.findall("link")}
        joints = robot.findall("joint")
        if len(joints) > MAX_LINKS:
            raise ValueError(f"{who}: {len(joints)} links; the device table holds {MAX_LINKS}")
        children = {j.find("child").get("link") for j in joints}
        roots = [n for n in links if n not in children]
        if len(roots) != 1:
            raise ValueError(f"{who}: one link without a parent joint is the root; found {roots}")
        ro = links[roots[0]].find("inertial/origin")
        if np.any(_floats(ro, "xyz", "root inertial") != 0) or np.any(_floats(ro, "rpy", "root inertial") != 0):
            raise ValueError(f"{who}: the root's inertial origin is not zero (the base pose would not be the root link's)")
        body = {roots[0]: 0}
        parent, jxyz, jq, com, col, names = [], [], [], [], [], [roots[0]]
        for i, j in enumerate(joints):
            name, kind = j.get("name"), j.get("type")
            if kind not in ("spherical", "fixed"):
                raise ValueError(f"{who}: joint {name!r} is {kind!r}; only spherical and fixed joints are served")
            pa, child = j.find("parent").get("link"), j.find("child").get("link")
            if pa not in body:
                raise ValueError(f"{who}: joint {name!r} comes before its parent link {pa!r}")
            if char_info.joint_idx.get(name) != i:
                raise ValueError(f"{who}: joint {name!r} is link {i} of the URDF but {char_info.joint_idx.get(name)!r} in char_info.joint_idx")
            io = links[child].find("inertial/origin")
            if np.any(_floats(io, "rpy", f"link {child!r} inertial") != 0):
                raise ValueError(f"{who}: link {child!r} has a non-zero inertial rpy (its COM frame is turned against the link frame)")
            parent.append(body[pa])
            body[child] = i + 1
            names.append(child)
            o = j.find("origin")
            jxyz.append(_floats(o, "xyz", f"joint {name!r}"))
            jq.append(_rpy_quat(_floats(o, "rpy", f"joint {name!r}")))
            com.append(_floats(io, "xyz", f"link {child!r} inertial"))
            col.append(-1 if kind == "fixed" else (char_info.nimble_state_map[i] - 1) * 3 + 6)
        sbp = [getattr(char_info, n) + 1 for n in SBP_BODIES]
        imu = [getattr(char_info, n) + 1 for n in IMU_BODIES] if all(hasattr(char_info, n) for n in IMU_BODIES) else None
        return cls(parent, jxyz, jq, com, col, sbp, names, imu)

    def table(self) -> dict:
        return {"parent": self.parent, "joint_xyz": self.joint_xyz, "joint_q": self.joint_q, "com_xyz": self.com_xyz,
                "state_col": self.state_col, "sbp": self.sbp, "names": np.array(self.names)}

    def pack(self) -> np.ndarray:
        """The device table (include/tip_hip.h, "kinematics") as bytes: 8 words of header, 32 links of 12 words."""
        head = np.zeros(8, dtype="<i4")
        head[0], head[1:6] = self.n_links, self.sbp
        rec = np.zeros(MAX_LINKS, dtype=_SKEL_DTYPE)
        rec["state_col"] = -1
        L = self.n_links
        rec["parent"][:L], rec["state_col"][:L] = self.parent, self.state_col
        rec["joint_xyz"][:L], rec["joint_q"][:L], rec["com_xyz"][:L] = self.joint_xyz, self.joint_q, self.com_xyz
        rec["joint_q"][L:, 3] = 1.0
        return np.frombuffer(head.tobytes() + rec.tobytes(), dtype=np.uint8).copy()

    def on(self, device):
        """The packed table on `device` (uploaded once per device and kept)."""
        import torch
        device = _device(device)
        if device not in self._dev:
            self._dev[device] = torch.from_numpy(self.pack()).pin_memory().to(device, non_blocking=True)
        return self._dev[device]


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def _device(device=None):
    import torch
    d = torch.device("cuda" if device is None else device)
    if d.type != "cuda":
        raise RuntimeError("tip_amd.kinematics runs on an MI355X: give it a cuda device")
    return torch.device("cuda", torch.cuda.current_device()) if d.index is None else d


def _lib():
    from . import lib as tlib
    return tlib, tlib.load()


def _check(status):
    return _lib()[0].check(status)


def _dev_f32(x, device, shape_tail, who, what):
    """x as a contiguous float32 CUDA tensor [rows, *shape_tail or wider]."""
    import torch
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    t = t.to(torch.float32)
    if t.dim() != 1 + len(shape_tail) or any(a != b for a, b in zip(t.shape[1:], shape_tail)):
        raise ValueError(f"tip_amd.kinematics.{who}: {what} is [rows, {', '.join(str(s) for s in shape_tail)}]; got {tuple(t.shape)}")
    if not t.is_cuda:
        t = t.pin_memory().to(device, non_blocking=True)
    return t.to(device).contiguous()


def _offsets(offsets, n_rows, who):
    o = np.asarray(offsets, dtype=np.int64).reshape(-1)
    if o.shape[0] < 1 or o[0] != 0 or (np.diff(o) < 0).any() or o[-1] != n_rows:
        raise ValueError(f"tip_amd.kinematics.{who}: offsets is [R + 1], from 0 up to the number of rows ({n_rows}), never falling; "
                         f"got {o.tolist()[:8]}{'...' if o.shape[0] > 8 else ''}")
    return o


def _stream(device):
    return _lib()[0].current_stream(device)


# ---- the wearer's body scale -----------------------------------------------------------------------------------------------------------
def scale_of_height(h: float) -> float:
    """The reference's rule for a wearer h metres tall: scale = h / 1.6 (data-gen-and-viz-bullet-new.py:256-257, handed to SimAgent as
    PyBullet's globalScaling, bullet_agent.py:47,67)."""
    return float(h) / 1.6


def check_scales(scales, count: int, who: str, scalar_ok: bool = False):
    """`scales` as a float32 numpy array [count], or None for None.  ValueError for anything that is not `count` finite numbers above 0
    (with scalar_ok, one number stands for all).  Host work only: every caller refuses here before it allocates or launches anything.
    (A CUDA tensor is read back for the check.)"""
    if scales is None:
        return None
    if hasattr(scales, "detach"):
        scales = scales.detach().cpu().numpy()
    try:
        a = np.asarray(scales, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"tip_amd.{who}: scales is [{count}] numbers; got {type(scales).__name__}") from None
    if scalar_ok and a.ndim == 0:
        a = np.full(count, float(a))
    if a.shape != (count,):
        raise ValueError(f"tip_amd.{who}: scales is [{count}], one body scale per {'row' if scalar_ok else 'sequence'}; got {a.shape}")
    if not (np.isfinite(a).all() and (a > 0).all()):
        bad = int(np.nonzero(~(np.isfinite(a) & (a > 0)))[0][0])
        raise ValueError(f"tip_amd.{who}: a body scale is a finite number above 0 (height / 1.6); got {a[bad]!r} at {bad}")
    a = a.astype(np.float32)
    if not (np.isfinite(a).all() and (a > 0).all()):
        raise ValueError(f"tip_amd.{who}: a body scale must be finite and above 0 as float32 too")
    return a


def _scales_dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).pin_memory().to(device, non_blocking=True)


# ---- FK ------------------------------------------------------------------------------------------------------------------------------
def fk(skel: Skeleton, q, out_jf: bool = False, device=None, scale=None):
    """q [N, >= 57] (root xyz, root axis-angle, the joints' axis-angles; numpy or a CUDA tensor) -> pq_g [N, L + 1, 7], the COM poses
    (PyBullet's getLinkState fields 0-1), root first; with out_jf=True also pq_jf, the link frames (fields 4-5).  CUDA float32.
    scale: the wearer's body scale, one number or [N] (one per row: rows of many wearers in one launch); None is the unscaled kernel.
    A float32 CUDA tensor [N] is used where it lies, unread by the host: there the kernel's rule holds (a row whose scale is not finite
    or not above 0 comes back NaN)."""
    import torch
    shape = tuple(q.shape) if hasattr(q, "shape") else np.shape(q)
    if len(shape) != 2 or shape[1] < 57:
        raise ValueError(f"tip_amd.kinematics.fk: q is [N, >= 57]; got {shape}")
    on_dev = isinstance(scale, torch.Tensor) and scale.is_cuda
    if on_dev and (scale.dtype != torch.float32 or tuple(scale.shape) != (int(shape[0]),)):
        raise ValueError(f"tip_amd.kinematics.fk: a device scale is float32 [{int(shape[0])}]; got {scale.dtype} {tuple(scale.shape)}")
    sc = scale.contiguous() if on_dev else check_scales(scale, int(shape[0]), "kinematics.fk", scalar_ok=True)
    device = q.device if isinstance(q, torch.Tensor) and q.is_cuda and device is None else _device(device)
    t = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32))
    if t.dim() != 2 or t.shape[1] < 57:
        raise ValueError(f"tip_amd.kinematics.fk: q is [N, >= 57]; got {tuple(t.shape)}")
    t = t.to(torch.float32)
    t = (t if t.is_cuda else t.pin_memory().to(device, non_blocking=True)).contiguous()
    _, lib = _lib()
    n, per = int(t.shape[0]), skel.n_links + 1
    with torch.cuda.device(device):
        sk = skel.on(device)
        pq_g = torch.empty((n, per, 7), dtype=torch.float32, device=device)
        pq_jf = torch.empty((n, per, 7), dtype=torch.float32, device=device) if out_jf else None
        if sc is None:
            _check(lib.tip_kin_fk(sk.data_ptr(), t.data_ptr(), int(t.shape[1]), n, pq_g.data_ptr(), _ptr(pq_jf), _stream(device)))
        else:
            scd = sc.to(device) if on_dev else _scales_dev(sc, device)
            _check(lib.tip_kin_fk_scaled(sk.data_ptr(), t.data_ptr(), int(t.shape[1]), n, pq_g.data_ptr(), _ptr(pq_jf), scd.data_ptr(),
                                         _stream(device)))
    return (pq_g, pq_jf) if out_jf else pq_g


# ---- the root track ------------------------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


class _Blocks:
    """n state blocks on a device with the skeleton beside them, and the reset and track launches on them.  A subclass sizes the
    buffer (_alloc) and names the two entry points (looked up in the loaded library at every launch, so that a wrapper somebody puts
    around one there sees the call), what they take behind (skel, blocks, n) and what track takes behind `valid`.
    `scale`: None, or the [n] float32 device tensor of the blocks' body scales; with one, the entries are the two names + "_scaled" and
    take it in front of the stream (`entries` says which pair the next launch calls)."""
    _reset_fn = _track_fn = None
    _reset_args = _track_args = _track_tail = ()
    scale = None

    def __init__(self, skel, n, device):
        self.skel, self.n, self.device = skel, int(n), _device(device)

    @property
    def entries(self):
        tail = "" if self.scale is None else "_scaled"
        return self._reset_fn + tail, self._track_fn + tail

    def _scale_arg(self):
        return () if self.scale is None else (self.scale.data_ptr(),)

    def _alloc(self, bytes_fn, *shape):
        import torch
        self.tlib, self.lib = _lib()
        nbytes = ctypes.c_size_t()
        _check(getattr(self.lib, bytes_fn)(self.n, *shape, ctypes.byref(nbytes)))
        with torch.cuda.device(self.device):
            self.buf = torch.zeros(max(nbytes.value, 8), dtype=torch.uint8, device=self.device)
            self.sk = self.skel.on(self.device)
        return nbytes.value

    def reset(self, slots_dev, count, s_init_dev):
        import torch
        with torch.cuda.device(self.device):
            _check(getattr(self.lib, self.entries[0])(self.sk.data_ptr(), self.buf.data_ptr(), self.n, *self._reset_args, _ptr(slots_dev), count,
                                  s_init_dev.data_ptr(), *self._scale_arg(), _stream(self.device)))

    def track(self, slots_dev, begin_ptr, end_ptr, count, s_rest, c_t, valid, *outs):
        import torch
        with torch.cuda.device(self.device):
            _check(getattr(self.lib, self.entries[1])(self.sk.data_ptr(), self.buf.data_ptr(), self.n, *self._track_args, _ptr(slots_dev), begin_ptr, end_ptr,
                                  count, int(s_rest.shape[0]), s_rest.data_ptr(), c_t.data_ptr(), int(c_t.shape[1]), _ptr(valid),
                                  *self._track_tail, *(o.data_ptr() for o in outs), *self._scale_arg(), _stream(self.device)))


class _Carry(_Blocks):
    """n carry blocks on a device (tip_kin_carry_bytes) and the launches on them."""
    _reset_fn, _track_fn = "tip_kin_track_reset", "tip_kin_track"

    def __init__(self, skel, n, device):
        super().__init__(skel, n, device)
        self._alloc("tip_kin_carry_bytes")


def _track_inputs(s_rest, c_t, valid, device, who):
    import torch
    s = _dev_f32(s_rest, device, (111,), who, "s_rest")
    c = _dev_f32(c_t, device, (int(np.shape(c_t)[-1]),), who, "c_t")
    if c.shape[1] not in (8, 20) or c.shape[0] != s.shape[0]:
        raise ValueError(f"tip_amd.kinematics.{who}: c_t is [rows, 8 | 20] with s_rest's rows ({s.shape[0]}); got {tuple(c.shape)}")
    if valid is not None:
        v = valid if isinstance(valid, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(valid).astype(np.uint8))
        if v.dim() != 1 or v.shape[0] != s.shape[0]:
            raise ValueError(f"tip_amd.kinematics.{who}: valid is [rows] ({s.shape[0]}); got {tuple(v.shape)}")
        v = v.to(torch.uint8) if v.dtype not in (torch.uint8, torch.bool) else v
        valid = (v if v.is_cuda else v.pin_memory().to(device, non_blocking=True)).to(device).contiguous()
    return s, c, valid


def _ragged_scales(mod, who, scales, offsets):
    """track's / track_terrain's scales [R] checked on the host (R from offsets), before anything else is looked at."""
    if scales is None:
        return None
    return check_scales(scales, max(int(np.asarray(offsets).reshape(-1).shape[0]) - 1, 0), f"{mod}.{who}")


def _track_ragged(mod, who, s_init, s_rest, c_t, valid, offsets, device, chunk, make, check_width=None, scales=None):
    """track and track_terrain behind their outputs: the inputs onto the device and checked (s_rest [N, 111], c_t [N, 8 | 20], valid [N],
    offsets [R + 1], s_init as [R, 114]), then make(N, R) — the caller's state object of R blocks and the tuple of its output tensors —
    then the reset and the track of every sequence, in one launch or, with chunk=k, k rows of every sequence per launch.  Returns what
    make returned.  scales: None, or the sequences' body scales [R] as check_scales returned them — the state object then calls the
    scaled entries with them."""
    import torch
    s, c, v = _track_inputs(s_rest, c_t, valid, device, who)
    if check_width is not None:
        check_width(c)
    o = _offsets(offsets, int(s.shape[0]), who)
    R = o.shape[0] - 1
    s0 = _dev_f32(s_init if np.ndim(s_init) == 2 else np.asarray(s_init)[None], device, (114,), who, "s_init")
    if s0.shape[0] != R:
        raise ValueError(f"tip_amd.{mod}.{who}: s_init is [R, 114] with one row per sequence ({R}); got {tuple(s0.shape)}")
    if scales is not None and scales.shape[0] != R:
        raise ValueError(f"tip_amd.{mod}.{who}: scales is [R], one body scale per sequence ({R}); got {scales.shape}")
    st, outs = make(int(s.shape[0]), R)
    if R == 0 or s.shape[0] == 0:
        return st, outs
    if scales is not None:
        st.scale = _scales_dev(scales, device)
    st.reset(None, R, s0)
    if chunk is None:
        od = torch.from_numpy(o).pin_memory().to(device, non_blocking=True)
        st.track(None, od.data_ptr(), od.data_ptr() + 8, R, s, c, v, *outs)
    else:
        k = int(chunk)
        if k < 1:
            raise ValueError(f"tip_amd.{mod}.{who}: chunk is a number of rows, at least 1; got {chunk!r}")
        for first in range(0, int(np.diff(o).max()), k):
            be = np.stack([np.minimum(o[:-1] + first, o[1:]), np.minimum(o[:-1] + first + k, o[1:])])
            bd = torch.from_numpy(be).pin_memory().to(device, non_blocking=True)
            st.track(None, bd[0].data_ptr(), bd[1].data_ptr(), R, s, c, v, *outs)
    return st, outs


def track(skel: Skeleton, s_init, s_rest, c_t, valid, offsets, device=None, chunk=None, scales=None):
    """R sequences back to back: s_init [R, 114], s_rest [N, 111], c_t [N, 8 | 20], valid [N] bool, offsets [R + 1] ->
    root [N, 3], viz_locs [N, 5, 3] (CUDA float32): the rows of RTRunnerMin.step's qdq[:3] and viz_locs, one kernel for the lot.
    chunk=k runs it k rows of every sequence per launch instead, through the carry: the same bits, for whoever gets rows in pieces.
    scales [R]: the sequences' body scales (None: the unscaled kernels)."""
    import torch
    scales = _ragged_scales("kinematics", "track", scales, offsets)
    device = _device(device)

    def make(n, R):
        return _Carry(skel, R, device), (torch.empty((n, 3), dtype=torch.float32, device=device),
                                         torch.empty((n, 5, 3), dtype=torch.float32, device=device))

    with torch.cuda.device(device):
        return _track_ragged("kinematics", "track", s_init, s_rest, c_t, valid, offsets, device, chunk, make, scales=scales)[1]


def track_replay(skel: Skeleton, results: Sequence, s_init, device=None, terrain=None, scales=None) -> List[tuple]:
    """ReplayPool.run's list -> per recording (qdq [L_i, 114], viz_locs [L_i, 5, 3]) as numpy float32: the script's s_traj_pred and
    viz_locs_seq before its trim (offline_testing_simple.py:123-139) — row 0 and the priming rows are s_init whole with markers at 100,
    row t + 1 is the step on frame t.  replay.trim_like_reference serves both arrays.
    terrain=None is RTRunnerMin's flat ground; terrain=dict(map_bound=..., grid_size=...[, max_regions=...]) is the full runner as the
    script starts it (:169-176, multi_sbp_terrain_and_correction off), through tip_amd.terrain.track_terrain.
    scales [R]: the recordings' body scales — what a file made by motion.syn_files at scale != 1 has to be tracked with."""
    who = "track_replay"
    results = list(results)
    if not results:
        raise ValueError("tip_amd.kinematics.track_replay: no recordings")
    scales = check_scales(scales, len(results), "kinematics.track_replay")
    s0 = np.ascontiguousarray(s_init, dtype=np.float32)
    s0 = s0[None] if s0.ndim == 1 else s0
    if s0.shape != (len(results), 114):
        raise ValueError(f"tip_amd.kinematics.track_replay: s_init is [R, 114], one start state per recording; got {s0.shape} for "
                         f"{len(results)} recordings")
    lens = [int(np.shape(r.s_rest)[0]) for r in results]
    for i, r in enumerate(results):
        if np.shape(r.s_rest) != (lens[i], 111) or np.shape(r.c_t)[0] != lens[i] or np.shape(r.valid) != (lens[i],) or lens[i] < 1:
            raise ValueError(f"tip_amd.kinematics.track_replay: recording {i} is not a ReplayResult of one length (s_rest "
                             f"{np.shape(r.s_rest)}, c_t {np.shape(r.c_t)}, valid {np.shape(r.valid)})")
    widths = {int(np.shape(r.c_t)[1]) for r in results}
    if len(widths) != 1:
        raise ValueError(f"tip_amd.kinematics.track_replay: the recordings' c_t widths differ ({sorted(widths)})")
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    s_rest = np.concatenate([np.asarray(r.s_rest, dtype=np.float32) for r in results])
    c_all = np.concatenate([np.asarray(r.c_t, dtype=np.float32) for r in results])
    v_all = np.concatenate([np.asarray(r.valid, dtype=bool) for r in results])
    kw = {} if scales is None else {"scales": scales}          # (scales=None: the call as it always was)
    if terrain is None:
        root, viz = track(skel, s0, s_rest, c_all, v_all, offs, device, **kw)
    else:
        from .terrain import track_terrain
        extra = set(terrain) - {"map_bound", "grid_size", "max_regions"}
        if extra or not {"map_bound", "grid_size"} <= set(terrain):
            raise ValueError(f"tip_amd.kinematics.track_replay: terrain is dict(map_bound=..., grid_size=...[, max_regions=...]); got "
                             f"{sorted(terrain)}")
        root, viz = track_terrain(skel, s0, s_rest, c_all, v_all, offs, multi_sbp=False, device=device, **kw, **terrain)[:2]
    root, viz = root.cpu().numpy(), viz.cpu().numpy()
    out = []
    for i, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        qdq = np.concatenate([root[a:b], s_rest[a:b]], axis=1)
        out.append((qdq, viz[a:b]))
    return out


class _Tracker:
    """What RootTracker and tip_amd.terrain.TerrainTracker share: n state blocks (self._s) beside an engine of n slots, the per-slot output
    tensors self._outs (root and viz_locs first), the slot lists on the device, reset and step.  _mod, _name and _slot_who make the
    messages."""
    _mod = _name = _slot_who = None

    def __init__(self, n, make_state):
        import torch
        self.n = int(n)
        if self.n < 1:
            raise ValueError(f"tip_amd.{self._mod}.{self._name}: n is the number of slots, at least 1; got {n!r}")
        self._s = make_state(self.n)
        self.device = self._s.device
        with torch.cuda.device(self.device):
            self.root = torch.zeros((self.n, 3), dtype=torch.float32, device=self.device)
            self.viz_locs = torch.full((self.n, 5, 3), 100.0, dtype=torch.float32, device=self.device)
            self._rows = torch.arange(self.n + 1, dtype=torch.int64, device=self.device)
            self.scale = torch.ones(self.n, dtype=torch.float32, device=self.device)      # the slots' body scales; 1 until a reset gives one
        self._outs = (self.root, self.viz_locs)
        self._lists = {}
        self._scale_host = np.ones(self.n, dtype=np.float32)      # the scales as the resets gave them (host): what a hand-over checks

    def _slot_tensors(self, slots, who):
        import torch
        from .streaming import slot_list
        idx = tuple(slot_list(slots, self.n, f"{self._slot_who}.{who}"))
        if idx not in self._lists:
            with torch.cuda.device(self.device):
                a = np.array(idx, dtype=np.int64)
                host = torch.from_numpy(np.stack([a, a + 1])).pin_memory()
                self._lists[idx] = (torch.from_numpy(a.astype(np.int32)).pin_memory().to(self.device, non_blocking=True),
                                    host.to(self.device, non_blocking=True))
        return idx, self._lists[idx]

    def _reset_rows(self, rows):
        """The per-slot output rows of freshly reset slots, beyond root and viz_locs."""

    def _check_width(self, c):
        """step's check of c_t's width, where the tracker has one."""

    def _before_subset_step(self):
        """What a step on a subset of the slots does to the output rows first."""

    @property
    def entries(self):
        """The two library entries the next reset and step call: the unscaled pair until a reset has been given scales."""
        return self._s.entries

    def _unscaled(self):
        """Back to the unscaled entries with every slot at scale 1 (ReplayPool.run(scales=None) after a run with scales)."""
        if self._s.scale is not None:
            self._s.scale = None
            self.scale.fill_(1.0)
            self._scale_host[:] = 1.0

    def reset(self, slots, s_init_rows, scales=None):
        import torch
        from .streaming import slot_list
        who = f"{self._mod}.{self._name}.reset"
        count = self.n if slots is None else len(slot_list(slots, self.n, f"{self._slot_who}.reset"))
        scales = check_scales(scales, count, who)          # (host only: refused before anything is uploaded or launched)
        with torch.cuda.device(self.device):
            if slots is None:
                count, sl = self.n, None
            else:
                idx, (sl, _) = self._slot_tensors(slots, "reset")
                count = len(idx)
            s0 = _dev_f32(s_init_rows if np.ndim(s_init_rows) == 2 else np.asarray(s_init_rows)[None], self.device, (114,),
                          f"{self._name}.reset", "s_init_rows")
            if s0.shape[0] != count:
                raise ValueError(f"tip_amd.{self._mod}.{self._name}.reset: s_init_rows is [{count}, 114]; got {tuple(s0.shape)}")
            if count:
                rows = slice(None) if sl is None else sl.long()
                # a slot's scale is set here and nowhere else: the carry's pq_prev is computed with it.  A reset without scales puts
                # the slot back to 1; a tracker that was never given a scale does not touch the array and keeps the unscaled entries.
                if scales is not None:
                    self._s.scale = self.scale
                    self.scale[rows] = _scales_dev(scales, self.device)
                elif self._s.scale is not None:
                    self.scale[rows] = 1.0
                self._scale_host[slice(None) if sl is None else list(idx)] = 1.0 if scales is None else scales
                self._s.reset(sl, count, s0)
                self.root[rows] = s0[:, :3]
                self.viz_locs[rows] = 100.0
                self._reset_rows(rows)

    def step(self, out, slots=None):
        import torch
        if out is None:
            return self.root, self.viz_locs
        s, c, v = out["s_rest"], out["c_t"], out.get("valid")
        if tuple(s.shape) != (self.n, 111) or s.device != self.device or c.shape[0] != self.n or not s.is_contiguous() or not c.is_contiguous():
            raise ValueError(f"tip_amd.{self._mod}.{self._name}.step: out is an engine's frame of {self.n} slots on {self.device}")
        if v is not None and not (isinstance(v, torch.Tensor) and v.dtype in (torch.bool, torch.uint8) and v.shape == (self.n,)):
            raise ValueError(f"tip_amd.{self._mod}.{self._name}.step: out['valid'] is a bool tensor [n]")
        self._check_width(c)
        if slots is None:
            self._s.track(None, self._rows.data_ptr(), self._rows.data_ptr() + 8, self.n, s, c, v, *self._outs)
        else:
            idx, (sl, be) = self._slot_tensors(slots, "step")
            self._before_subset_step()
            if idx:
                self._s.track(sl, be[0].data_ptr(), be[1].data_ptr(), len(idx), s, c, v, *self._outs)
        return self.root, self.viz_locs

    # ---- wearer hand-over (tip_amd.handover) ---------------------------------------------------------------------------------------------
    def export_slots(self, slots):
        """The listed slots' wearers as they stand (tip_amd.handover): their state block, body scale and output rows as device tensors,
        plus plain metadata (block size, the skeleton table, the scales as the host gave them).  Nothing is reset or detached; one
        launch and a few gathers on the current stream, no synchronisation."""
        from . import handover
        return handover.export_tracker(self, slots)

    def import_slots(self, slots, exported):
        """Put exported wearers into the listed slots: from the next step on each continues bit for bit where it was.  The skeleton table
        and block layout (a terrain tracker: grid_num, max_regions, multi_sbp) must be the exporter's, and a tracker that has never been
        given scales refuses a wearer whose scale is not 1 (ValueError, before anything is launched); one that has takes any.  The
        entries of `fire` that travel are rewritten to the new slot indices."""
        from . import handover
        handover.import_tracker(self, slots, exported)


class RootTracker(_Tracker):
    """The live form: n carry blocks beside an engine of n slots.
        rt = RootTracker(skel, engine.n, engine.device)
        rt.reset(None, s_init)                 # with the engine's s_init; reset(slots, rows) whenever the engine attaches those slots
        out = engine.step(frame)
        root, viz_locs = rt.step(out)          # [n, 3], [n, 5, 3]: this frame's qdq[:3] and viz_locs by slot (tensors reused every frame)
    step() is ONE launch on the current stream (call it on the engine's stream, after step; it is not part of the engine's captured
    graph).  out=None — a lock-step engine that is still priming — launches nothing and returns the rows as they stand.  Rows whose
    out["valid"] is False, and slots left out of `slots`, keep their carry; the former read (carry root, 100s).
    A pool of wearers of different heights: rt.reset(slots, rows, scales=[scale_of_height(h), ...]) — still one launch per frame."""
    _mod, _name, _slot_who = "kinematics", "RootTracker", "RootTracker"

    def __init__(self, skel: Skeleton, n: int, device):
        super().__init__(n, lambda n: _Carry(skel, n, device))

    def reset(self, slots, s_init_rows, scales=None):
        """The listed slots (None: all) start over from s_init_rows [len(slots), 114]: root = s_init[:3], pq_prev = FK(s_init).
        scales [len(slots)]: the body scales of the wearers these slots take (rt.scale [n] holds them on the device, 1 where none was
        given); from the first reset with scales on, reset and step call the scaled entries."""
        super().reset(slots, s_init_rows, scales)


# ---- the seven metrics ---------------------------------------------------------------------------------------------------------------
def root_indices(n: int) -> List[int]:
    """loss_root_dist_pos's row for t = 2, 5 and 10 s among n rows (data_utils.py:383-386), by its own expression: 119 / 299 / 599."""
    return [int(np.minimum(int(t / DT) - 1, n - 1)) for t in (2.0, 5.0, 10.0)]


def evaluate(skel: Skeleton, pred_qdq, gt_qdq, offsets, start: int = 30, end: int = 6, device=None, scales=None) -> np.ndarray:
    """R files back to back: pred_qdq, gt_qdq [N, 114] (numpy or CUDA tensors), offsets [R + 1] -> [R, 7] float64, the columns METRICS in
    the script's order (offline_testing_simple.py:439-445), over rows start .. L - end - 1 of each file with FK of both trajectories.
    The script's means and maxima over files (:447-461) are numpy on the result.  A file with fewer than 4 rows in range is a
    ValueError (the reference would print the NaN of an empty mean; it never sees such a file, :371).
    scales [R]: the files' body scales; both trajectories of a file go through FK at its scale (None: the unscaled kernel)."""
    import torch
    scales = _ragged_scales("kinematics", "evaluate", scales, offsets)
    device = _device(device)
    start, end = int(start), int(end)
    if start < 0 or end < 0:
        raise ValueError(f"tip_amd.kinematics.evaluate: start and end are row counts, >= 0; got {start}, {end}")
    with torch.cuda.device(device):
        p = _dev_f32(pred_qdq, device, (114,), "evaluate", "pred_qdq")
        g = _dev_f32(gt_qdq, device, (114,), "evaluate", "gt_qdq")
        if p.shape != g.shape:
            raise ValueError(f"tip_amd.kinematics.evaluate: pred_qdq {tuple(p.shape)} and gt_qdq {tuple(g.shape)} differ")
        o = _offsets(offsets, int(p.shape[0]), "evaluate")
        R = o.shape[0] - 1
        lens = np.diff(o)
        short = [int(i) for i in np.nonzero(lens < start + end + 4)[0]]
        if short:
            raise ValueError(f"tip_amd.kinematics.evaluate: file {short[0]} has {int(lens[short[0]])} rows; rows {start} .. L - {end} - 1 "
                             f"must leave at least 4 (L >= {start + end + 4})")
        if R == 0:
            return np.zeros((0, 7), dtype=np.float64)
        _, lib = _lib()
        i2, i5, i10 = (int(t / DT) - 1 for t in (2.0, 5.0, 10.0))      # the script's expression; the kernel clamps to each file's own rows
        sk = skel.on(device)
        if scales is not None and scales.shape[0] != R:
            raise ValueError(f"tip_amd.kinematics.evaluate: scales is [R], one body scale per file ({R}); got {scales.shape}")
        rows = None
        if scales is not None:          # one entry per row, expanded on the device ([R] goes up, output_size spares the synchronisation)
            lens_d = torch.from_numpy(lens.astype(np.int64)).pin_memory().to(device, non_blocking=True)
            rows = torch.repeat_interleave(_scales_dev(scales, device), lens_d, output_size=int(p.shape[0]))
        pq_p, pq_g = fk(skel, p, device=device, scale=rows), fk(skel, g, device=device, scale=rows)
        od = torch.from_numpy(o).pin_memory().to(device, non_blocking=True)
        out = torch.empty((R, 7), dtype=torch.float64, device=device)
        _check(lib.tip_kin_metrics(sk.data_ptr(), p.data_ptr(), g.data_ptr(), pq_p.data_ptr(), pq_g.data_ptr(), od.data_ptr(), R, start, end,
                                   i2, i5, i10, out.data_ptr(), _stream(device)))
        return out.cpu().numpy()
