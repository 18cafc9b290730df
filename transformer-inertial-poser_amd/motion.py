"""SMPL pose files to `nimble_qdq`, on the device (csrc/tip_motion.hip; include/tip_hip.h, "motion"): the ground-truth half of the
reference's preprocessing — dip_loader.load, the root augmentation of preprocess_DIP_TC_new.py:98-107 and
data_utils.get_raw_motion_info_nimble_q_dummy_dq (:103-161), which resamples a motion to 60 Hz through fairmotion's get_pose_by_time
and, per output frame, turns 18 rotations into axis-angles and differences the root.  Here it is one launch over any number of ragged
sequences, fp64, and what comes out stays in HBM for the stages behind it:

    f = load_pose_file("ACCAD/.../B1_poses.npz")                             # host only: {"poses", "trans", "fps", "ori", "acc"}
    qdq = qdq_from_smpl([f["poses"]], f["fps"], [f["trans"]])                # [K_i, 114] CUDA fp64 each
    files = syn_files(skel, paths, [body_scale(rng) for _ in paths])         # -> tip_amd.syndata.synthesize: imu, constrs, nimble_qdq
    files = real_files(gt_paths, imu_paths, sensors.ROT_DIP, sensors.SEL_DIP17)   # -> sensors.real_imu_frames: imu, nimble_qdq
    combined = tip_amd.data.combine_motions(files, rates)                    # in place, no host round trip

A row is root xyz, root axis-angle, the 17 spherical joints' axis-angles in nimble state order (the two fixed wrists are dropped), the
root's linear and angular velocity from the pose one DT later, and zeros for the joints' velocities, which the reference fills with
zeros too.  Only SMPL joints 0 .. 21 are read: the body shape and the joint offsets do not enter nimble_qdq, so no SMPL-H body model is
needed.  fairmotion's interpolation is restated from its published source and PyBullet only answers which joints are fixed; parity with
either library stays unpinned (tests/golden/make_motion_golden.py says how the fixture was made).

An offline producer beside the engines, like tip_amd.syndata and tip_amd.kinematics: it touches no engine, graph or other kernel."""
from __future__ import annotations

import pickle
from typing import List, Optional, Sequence

import numpy as np

from .kinematics import Skeleton, _check, _device, _lib, _stream

DT = 1.0 / 60                       # constants.py:7
T0 = 0.015 / 2.0                    # data_utils.py:112
DEFAULT_FPS = 60.0                  # dip_loader.py:156
MIN_COLS = 66                       # SMPL joints 0 .. 21
# constants.py:33-58: the SMPL joints by the character's joint names (bvh_map is the identity on them, amass_char_info.py:167-188)
SMPL_JOINTS = ("root", "lhip", "rhip", "lowerback", "lknee", "rknee", "upperback", "lankle", "rankle", "chest", "ltoe", "rtoe", "lowerneck",
               "lclavicle", "rclavicle", "upperneck", "lshoulder", "rshoulder", "lelbow", "relbow", "lwrist", "rwrist", "lhand", "rhand")
# the shipped character's spherical joints in nimble state order (amass_char_info.py:89-109): output columns 6, 9, ..., 54
STATE_ORDER = ("lhip", "lknee", "lankle", "lowerback", "upperback", "chest", "lclavicle", "lshoulder", "lelbow", "lowerneck", "upperneck",
               "rclavicle", "rshoulder", "relbow", "rhip", "rknee", "rankle")
_tables = {}                        # device -> time table; (device, joints) -> joint table


def time_table(count: int) -> np.ndarray:
    """t_0 .. t_{count-1}: np.cumsum over [0.0075, DT, DT, ...] — the reference's running sum `cur_time += cst.DT` to the bit."""
    if count <= 0:
        return np.zeros(0)
    step = np.full(int(count), DT)
    step[0] = T0
    return np.cumsum(step)


def output_rows(n: int, fps: float) -> int:
    """K: how many 60 Hz rows a source motion of n frames at fps gives — the count of k with t_k < (n - 1) / fps."""
    n, fps = int(n), float(fps)
    if not fps > 0 or not np.isfinite(fps):
        raise ValueError(f"tip_amd.motion.output_rows: fps is a positive number; got {fps}")
    if n < 1:
        return 0
    length = (n - 1) * (1.0 / fps)
    return int(np.count_nonzero(time_table(int(length / DT) + 4) < length))


def joint_table(skel: Optional[Skeleton] = None) -> np.ndarray:
    """int32 [18]: the SMPL joint of the root, then of the joints whose axis-angles fill output columns 6, 9, ..., 54.  From a
    Skeleton's names and state_col, or the shipped character's order."""
    who = "tip_amd.motion"
    if skel is None:
        return np.array([SMPL_JOINTS.index(n) for n in ("root",) + STATE_ORDER], dtype=np.int32)
    if not isinstance(skel, Skeleton):
        raise TypeError(f"{who}: skel is a tip_amd.kinematics.Skeleton; got {type(skel).__name__}")
    out = np.full(18, -1, dtype=np.int32)
    names = [skel.names[0]] + [skel.names[i + 1] for i in range(skel.n_links)]
    cols = [3] + [int(c) for c in skel.state_col]
    for name, col in zip(names, cols):
        if col == -1:
            continue                                                     # a fixed joint: dropped, as the reference drops the wrists
        if name not in SMPL_JOINTS or SMPL_JOINTS.index(name) >= MIN_COLS // 3:
            raise ValueError(f"{who}: the skeleton's joint {name!r} is none of the SMPL joints 0 .. 21 ({', '.join(SMPL_JOINTS[:22])})")
        slot = (col - 3) // 3
        if (col - 3) % 3 or not 0 <= slot < 18 or out[slot] != -1:
            raise ValueError(f"{who}: the skeleton's state columns are 6, 9, ..., 54, each once; joint {name!r} has {col}")
        out[slot] = SMPL_JOINTS.index(name)
    if (out < 0).any():
        raise ValueError(f"{who}: the skeleton fills output columns {[3 + 3 * int(s) for s in np.flatnonzero(out >= 0)]}; nimble_qdq has "
                         "the root and 17 spherical joints (columns 3 .. 56)")
    return out


def _as_f64(x):
    import torch
    if isinstance(x, torch.Tensor):
        return x.to(torch.float64)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float64))


def _check_inputs(poses_list, fps, trans_list):
    """Everything that can be refused before the library or a device is touched -> (poses, trans or None, fps [R], lengths)."""
    who = "tip_amd.motion.qdq_from_smpl"
    poses_list = list(poses_list)
    R = len(poses_list)
    if R == 0:
        raise ValueError(f"{who}: no sequences")
    if trans_list is not None:
        trans_list = list(trans_list)
        if len(trans_list) != R:
            raise ValueError(f"{who}: trans_list has one entry (or None) per sequence ({R}); got {len(trans_list)}")
    f = np.asarray(fps, dtype=np.float64).reshape(-1)
    if f.shape[0] == 1 and np.ndim(fps) == 0:
        f = np.full(R, float(f[0]))
    if f.shape[0] != R:
        raise ValueError(f"{who}: fps is one number or one per sequence ({R}); got {f.shape[0]}")
    if not (np.isfinite(f).all() and (f > 0).all()):
        raise ValueError(f"{who}: fps is positive and finite; got {f.tolist()}")
    lens = []
    for i, p in enumerate(poses_list):
        shape = tuple(p.shape) if hasattr(p, "shape") else ()
        if len(shape) != 2 or shape[1] < MIN_COLS:
            raise ValueError(f"{who}: sequence {i} is [n, >= {MIN_COLS}] (one axis-angle per SMPL joint, joints 0 .. 21 read); got {shape}")
        lens.append(int(shape[0]))
        t = None if trans_list is None else trans_list[i]
        if t is not None:
            ts = tuple(t.shape) if hasattr(t, "shape") else ()
            if len(ts) != 2 or ts[1] != 3:
                raise ValueError(f"{who}: trans of sequence {i} is [n, 3]; got {ts}")
            if ts[0] != shape[0]:
                raise ValueError(f"{who}: sequence {i} has {shape[0]} pose frames and {ts[0]} trans frames")
    return poses_list, trans_list, f, lens


def _times_on(device, count):
    """The time table on `device`, at least `count` long: built on the host, uploaded, kept and grown by doubling."""
    import torch
    have = _tables.get(device)
    if have is None or have.shape[0] < count:
        size = max(1024, int(count), 0 if have is None else 2 * int(have.shape[0]))
        have = _tables[device] = torch.from_numpy(time_table(size)).to(device)
    return have


def _joints_on(device, table):
    import torch
    key = (device, tuple(int(v) for v in table))
    if key not in _tables:
        _tables[key] = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(device)
    return _tables[key]


def qdq_from_smpl(poses_list: Sequence, fps, trans_list: Optional[Sequence] = None, skel: Optional[Skeleton] = None, device=None) -> List:
    """poses_list[i] [n_i, >= 66] (numpy or tensors, read as fp64: DIP-IMU `gt` and TotalCapture `poses` have 72 columns, AMASS SMPL-H
    `poses` 156; columns 0:66 are read), fps one number or one per sequence, trans_list[i] [n_i, 3] or None (then the DIP-IMU root rule:
    rot_up_R on the root rotation, the root at (0, 0, 0.95)) -> a list of CUDA fp64 [K_i, 114], views of one tensor, K_i =
    output_rows(n_i, fps_i).  skel: a tip_amd.kinematics.Skeleton whose names and state_col give the joint order (default: the shipped
    character's).
    ValueError before any device work: no sequences, a sequence that is not [n, >= 66], trans that is not [n, 3] or of another length,
    fps that is not positive or not one per sequence, a skeleton joint that is no SMPL joint."""
    poses_list, trans_list, f, lens = _check_inputs(poses_list, fps, trans_list)
    joints = joint_table(skel)
    import torch
    device = _device(device)
    R = len(lens)
    rows = [output_rows(n, fr) for n, fr in zip(lens, f)]
    in_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    with torch.cuda.device(device):
        ldp = min(int(p.shape[1]) for p in poses_list)                  # one stride for the stacked rows: the narrowest (>= 66)
        parts = [_as_f64(p)[:, :ldp].to(device) for p in poses_list]
        poses = (torch.cat(parts) if R > 1 else parts[0]).contiguous()
        trans = flags = None
        if trans_list is not None and any(t is not None for t in trans_list):
            tp = [torch.zeros((n, 3), dtype=torch.float64, device=device) if t is None else _as_f64(t).to(device)
                  for t, n in zip(trans_list, lens)]
            trans = (torch.cat(tp) if R > 1 else tp[0]).contiguous()
            flags = torch.from_numpy(np.array([0 if t is None else 1 for t in trans_list], dtype=np.int32)).to(device)
        n_in, n_out = int(in_off[-1]), int(out_off[-1])
        times = _times_on(device, max(rows))
        qdq = torch.empty((n_out, 114), dtype=torch.float64, device=device)
        in_dev, out_dev, fps_dev = (torch.from_numpy(a).to(device) for a in (in_off, out_off, f))
        _, lib = _lib()
        _check(lib.tip_motion_qdq(poses.data_ptr() if n_in else None, ldp, None if trans is None or not n_in else trans.data_ptr(),
                                  None if flags is None or not n_in else flags.data_ptr(), in_dev.data_ptr(), out_dev.data_ptr(),
                                  fps_dev.data_ptr(), R, n_in, n_out, times.data_ptr(), int(times.shape[0]),
                                  _joints_on(device, joints).data_ptr(), qdq.data_ptr() if n_out else None, _stream(device)))
        # (the stacked inputs and the offsets go out of scope here: the allocator reuses them in stream order, behind the launch)
    return [qdq[a:b] for a, b in zip(out_off[:-1], out_off[1:])]


def load_pose_file(path: str) -> dict:
    """One pose file as the reference reads it (dip_loader.py:143-162, preprocess_DIP_TC_new.py:56-94), host only and without any
    arithmetic: {"poses": `gt`[:, :72] or else `poses` (None in a file of readings only); "trans": `trans` or None; "fps": `mocap_framerate`, else `frame_rate`, else 60.0;
    "ori", "acc": `imu_ori` / `imu_acc`, or `ori` / `acc`, or None}.  .npz, or .pkl with encoding="latin1"."""
    if path.endswith("npz"):
        data = np.load(path, allow_pickle=False)
        keys = set(data.files)
    elif path.endswith("pkl"):
        with open(path, "rb") as f:
            data = pickle.load(f, encoding="latin1")
        keys = set(data.keys())
    else:
        raise ValueError(f"tip_amd.motion.load_pose_file: {path!r} is neither .npz nor .pkl")
    if "gt" in keys:
        poses = np.array(data["gt"])[:, :72]
    elif "poses" in keys:
        poses = np.array(data["poses"])
    else:
        poses = None                                                     # a TotalCapture readings file
    fps = float(data["mocap_framerate"]) if "mocap_framerate" in keys else (float(data["frame_rate"]) if "frame_rate" in keys else DEFAULT_FPS)
    ori = acc = None
    if "imu_ori" in keys:
        ori, acc = np.array(data["imu_ori"]), np.array(data["imu_acc"])
    elif "ori" in keys:
        ori, acc = np.array(data["ori"]), np.array(data["acc"])
    if poses is None and ori is None:
        raise ValueError(f"tip_amd.motion.load_pose_file: {path!r} has neither poses (`gt` / `poses`) nor readings (keys: {sorted(keys)})")
    return {"poses": poses, "trans": np.array(data["trans"]) if "trans" in keys else None, "fps": fps, "ori": ori, "acc": acc}


def real_files(gt_paths: Sequence[str], imu_paths: Sequence[str], rot, sel, skel: Optional[Skeleton] = None, device=None) -> List[dict]:
    """The reference's load_and_store (preprocess_DIP_TC_new.py:183-211) for a corpus: gt_paths[i] holds the poses, imu_paths[i] (the
    same file for DIP-IMU) the readings; rot and sel as tip_amd.sensors.real_imu_frames takes them (ROT_DIP / SEL_DIP17, ROT_TC /
    SEL_TC6).  -> [{"imu": [L_i, 72], "nimble_qdq": [K_i, 114]}], CUDA fp64, what tip_amd.data.combine_motions takes in place (a file
    that goes on to training also needs "constrs")."""
    from . import sensors
    if len(gt_paths) != len(imu_paths):
        raise ValueError(f"tip_amd.motion.real_files: {len(gt_paths)} pose files for {len(imu_paths)} IMU files")
    gt = [load_pose_file(p) for p in gt_paths]
    imu = [g if pi == pg else load_pose_file(pi) for g, pg, pi in zip(gt, gt_paths, imu_paths)]
    for p, g in zip(gt_paths, gt):
        if g["poses"] is None:
            raise ValueError(f"tip_amd.motion.real_files: {p!r} has no poses (`gt` or `poses`)")
    for p, f in zip(imu_paths, imu):
        if f["ori"] is None:
            raise ValueError(f"tip_amd.motion.real_files: {p!r} has no IMU readings (`imu_ori` / `imu_acc` or `ori` / `acc`)")
    device = _device(device)
    qdq = qdq_from_smpl([g["poses"] for g in gt], [g["fps"] for g in gt], [g["trans"] for g in gt], skel, device)
    frames = sensors.real_imu_frames([f["ori"] for f in imu], [f["acc"] for f in imu], rot, sel, device=device)
    return [{"imu": h, "nimble_qdq": q} for h, q in zip(frames, qdq)]


def syn_files(skel: Skeleton, paths: Sequence[str], scales, device=None) -> List[dict]:
    """The reference's gen_data_job_single_core (data-gen-and-viz-bullet-new.py:228-283) without its pickle: pose files ->
    qdq_from_smpl -> tip_amd.syndata.synthesize, scales[i] the body scale of file i (syndata.body_scale draws the reference's).
    -> [{"imu", "constrs", "nimble_qdq"}], CUDA fp64."""
    from . import syndata
    files = [load_pose_file(p) for p in paths]
    device = _device(device)
    qdq = qdq_from_smpl([f["poses"] for f in files], [f["fps"] for f in files], [f["trans"] for f in files], skel, device)
    return syndata.synthesize(skel, qdq, scales, device)
