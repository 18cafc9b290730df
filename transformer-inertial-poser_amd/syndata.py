"""Synthetic IMU readings and stationary-body-point (SBP) labels from pose sequences, on the device (csrc/tip_syn.hip;
include/tip_hip.h, "synthetic data"): the reference's offline generator, data-gen-and-viz-bullet-new.py, which turns a pose sequence
into the `imu` and `constrs` arrays its pickles hold — PyBullet FK of a randomly scaled character, six orientations and six centred
second differences, and per frame and body a brute-force search over 125 / 1782 / 6200 candidate points chained through the previous
solution (data_utils.get_rot_center_sample_based).  Here it is a handful of launches over any number of ragged sequences, fp64 end to end,
and what comes out stays in HBM for the combiner:

    skel = Skeleton.from_urdf("data/amass.urdf", amass_char_info)            # or from_table(npz) with an `imu` array
    rng = np.random.default_rng(0)
    files = synthesize(skel, qdq_list, [body_scale(rng) for _ in qdq_list])   # qdq_list[i]: [L_i, >= 57] nimble_qdq, numpy or CUDA
    combined = tip_amd.data.combine_motions(files, rates)                     # files[i]["imu"], ["constrs"]: CUDA fp64, used in place
    ds = TrainSubDataset.from_arrays(seq_length, combined.info, combined.IMU, combined.S, IMU_sum=combined.SUM)

The body height is the reference's only augmentation here (h = 1.7 U(0.9, 1.1), skeleton and root translation scaled by h / 1.6, frozen
into each pickle once per corpus); with the generator on the device it can be redrawn per sequence whenever the user likes.
`nimble_qdq` is passed through as the caller gave it, unscaled, as the reference stores it.

An offline producer beside the engines, like tip_amd.kinematics: it touches no engine, graph or other kernel.  The ankle-IMU variant
(USE_KNEE_RATHER_ANKLE_IMU = False) is not here; the loading of AMASS files into nimble_qdq is tip_amd.motion (syn_files chains the two)."""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from .kinematics import MAX_LINKS, Skeleton, _check, _device, _lib, _stream

NOMINAL_H = 1.7                     # constants.py:11
MIN_ROWS = 9                        # 2 * acc_fd_N + 1: the reference's acceleration padding indexes out of range below it (:215-216)
AXIS = 40                           # the grid table's room per axis
_SKEL_DTYPE = np.dtype([("parent", "<i4"), ("state_col", "<i4"), ("joint_xyz", "<f8", 3), ("joint_q", "<f8", 4), ("com_xyz", "<f8", 3)])
_GRID_DTYPE = np.dtype([("n", "<i4", 3), ("pad", "<i4"), ("axis", "<f8", (3, AXIS))])


def body_scale(rng) -> float:
    """One draw of the reference's body height as a scale: h = NOMINAL_H * uniform(0.9, 1.1), scale = h / 1.6 (:249-257).  `rng` is
    anything with .uniform(a, b): numpy's Generator or RandomState, or python's random module."""
    return NOMINAL_H * float(rng.uniform(0.9, 1.1)) / 1.6


def grid_axes():
    """The candidate points of get_rot_center_sample_based per body class, as three axes each, with its own seven np.arange
    expressions (data_utils.py:52-66) — so the lengths and the values are numpy's, to the bit: (feet, wrists, pelvis), the classes of
    SBP slots 0-1, 2-3 and 4.  9 x 6 x 33 = 1782, 5^3 = 125 and 31 x 25 x 8 = 6200 points."""
    wrist = np.arange(-0.02, 0.03, 0.01)
    return ((np.arange(-0.04, 0.05, 0.01), np.arange(-0.04, 0.02, 0.01), np.arange(-0.15, 0.18, 0.01)),
            (wrist, wrist.copy(), wrist.copy()),
            (np.arange(-0.15, 0.16, 0.01), np.arange(-0.1, 0.15, 0.01), np.arange(-0.12, -0.04, 0.01)))


def pack_grids() -> np.ndarray:
    """The grid table (include/tip_hip.h, "synthetic data") as bytes: per class 3 counts, a pad word and 3 x 40 doubles."""
    rec = np.zeros(3, dtype=_GRID_DTYPE)
    for c, axes in enumerate(grid_axes()):
        for k, a in enumerate(axes):
            if a.shape[0] > AXIS:
                raise ValueError(f"tip_amd.syndata: a grid axis of {a.shape[0]} values; the table holds {AXIS}")
            rec["n"][c, k] = a.shape[0]
            rec["axis"][c, k, :a.shape[0]] = a
    return np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()


def check_skeleton(skel: Skeleton):
    """What the syn path needs of a Skeleton beyond tip_amd.kinematics: the six IMU bodies, all bodies distinct and in range, and the
    root and the wrists shared between the two lists (they are tracked once)."""
    who = "tip_amd.syndata"
    if not isinstance(skel, Skeleton):
        raise TypeError(f"{who}: skel is a tip_amd.kinematics.Skeleton; got {type(skel).__name__}")
    if skel.imu is None:
        raise ValueError(f"{who}: the Skeleton has no imu bodies: from_table needs an `imu` array of six body indices (root, lwrist, "
                         "rwrist, lknee, rknee, upperneck) beside the kinematics arrays; from_urdf reads them from char_info")
    L = skel.n_links
    for what, idx, n in (("sbp", skel.sbp, 5), ("imu", skel.imu, 6)):
        if idx.shape[0] != n or (idx < 0).any() or (idx > L).any() or len(set(idx.tolist())) != n:
            raise ValueError(f"{who}: {what} is {n} distinct body indices in 0 .. {L}; got {idx.tolist()}")
    if [int(v) for v in skel.imu[:3]] != [int(skel.sbp[4]), int(skel.sbp[2]), int(skel.sbp[3])]:
        raise ValueError(f"{who}: imu[0:3] (root, lwrist, rwrist) are the bodies sbp[4], sbp[2], sbp[3]; got imu {skel.imu.tolist()}, "
                         f"sbp {skel.sbp.tolist()}")
    if set(skel.imu[3:].tolist()) & set(skel.sbp.tolist()):
        raise ValueError(f"{who}: lknee, rknee and upperneck are not SBP bodies; got imu {skel.imu.tolist()}, sbp {skel.sbp.tolist()}")


def pack_skeleton(skel: Skeleton) -> np.ndarray:
    """The fp64 device table (include/tip_hip.h, "synthetic data") as bytes: 16 words of header, 32 links of 88 bytes."""
    check_skeleton(skel)
    head = np.zeros(16, dtype="<i4")
    head[0], head[1:6], head[6:12] = skel.n_links, skel.sbp, skel.imu
    rec = np.zeros(MAX_LINKS, dtype=_SKEL_DTYPE)
    rec["state_col"] = -1
    L = skel.n_links
    rec["parent"][:L], rec["state_col"][:L] = skel.parent, skel.state_col
    rec["joint_xyz"][:L], rec["joint_q"][:L], rec["com_xyz"][:L] = skel.joint_xyz, skel.joint_q, skel.com_xyz
    rec["joint_q"][L:, 3] = 1.0
    return np.frombuffer(head.tobytes() + rec.tobytes(), dtype=np.uint8).copy()


def _tables_on(skel: Skeleton, device):
    """(skeleton table, grid table) on `device`, uploaded once per Skeleton and device.  uint8 tensors over 8-byte aligned storage."""
    import torch
    key = ("syn", device)
    if key not in skel._dev:
        skel._dev[key] = (torch.from_numpy(pack_skeleton(skel)).to(device), torch.from_numpy(pack_grids()).to(device))
    return skel._dev[key]


def _check_inputs(skel, qdq_list, scales):
    who = "tip_amd.syndata.synthesize"
    check_skeleton(skel)
    qdq_list = list(qdq_list)
    sc = np.asarray(scales, dtype=np.float64).reshape(-1)
    if len(qdq_list) == 0:
        raise ValueError(f"{who}: no sequences")
    if sc.shape[0] != len(qdq_list):
        raise ValueError(f"{who}: scales is one number per sequence ({len(qdq_list)}); got {sc.shape[0]}")
    for i, q in enumerate(qdq_list):
        shape = tuple(q.shape) if hasattr(q, "shape") else ()
        if len(shape) != 2 or shape[1] < 57:
            raise ValueError(f"{who}: sequence {i} is [L, >= 57] (root xyz, root axis-angle, the joints' axis-angles, ...); got {shape}")
        if shape[0] < MIN_ROWS:
            raise ValueError(f"{who}: sequence {i} has {shape[0]} rows; the +-4-frame acceleration and its padding need at least "
                             f"{MIN_ROWS}")
    return qdq_list, sc


def tracked_poses(skel: Skeleton, q, offsets, scales, device=None):
    """q [N, >= 57] CUDA fp64, offsets [R + 1] and scales [R] CUDA (int64, fp64) -> the tracked-pose block [N, 8, 7] CUDA fp64."""
    import torch
    device = _device(device)
    _, lib = _lib()
    with torch.cuda.device(device):
        sk, _ = _tables_on(skel, device)
        P = torch.empty((q.shape[0], 8, 7), dtype=torch.float64, device=device)
        _check(lib.tip_syn_poses(sk.data_ptr(), q.data_ptr(), int(q.shape[1]), offsets.data_ptr(), int(offsets.shape[0]) - 1,
                                 scales.data_ptr(), int(q.shape[0]), P.data_ptr(), _stream(device)))
    return P


def imu_readings(P, offsets, device=None):
    """The tracked-pose block -> imu [N, 72] CUDA fp64."""
    import torch
    device = _device(device)
    _, lib = _lib()
    with torch.cuda.device(device):
        out = torch.empty((P.shape[0], 72), dtype=torch.float64, device=device)
        _check(lib.tip_syn_imu(P.data_ptr(), offsets.data_ptr(), int(offsets.shape[0]) - 1, int(P.shape[0]), out.data_ptr(),
                               _stream(device)))
    return out


def sbp_labels(skel: Skeleton, P, offsets, device=None):
    """The tracked-pose block -> constrs [N, 20] CUDA fp64: one workgroup per (sequence, SBP body), frames in order."""
    import torch
    device = _device(device)
    _, lib = _lib()
    with torch.cuda.device(device):
        _, grids = _tables_on(skel, device)
        out = torch.empty((P.shape[0], 20), dtype=torch.float64, device=device)
        frames = torch.empty((P.shape[0], 5, 15), dtype=torch.float64, device=device)      # the kernels' scratch: R, w, v per (row, body)
        _check(lib.tip_syn_sbp(grids.data_ptr(), P.data_ptr(), offsets.data_ptr(), int(offsets.shape[0]) - 1, int(P.shape[0]),
                               frames.data_ptr(), out.data_ptr(), _stream(device)))
    return out


def upload(qdq_list: Sequence, scales, device):
    """The sequences' first 57 columns back to back as one CUDA fp64 [N, 57], with offsets [R + 1] (int64) and scales [R] on the device."""
    import torch
    parts = []
    for q in qdq_list:
        if isinstance(q, torch.Tensor):
            parts.append(q[:, :57].to(device=device, dtype=torch.float64))
        else:
            parts.append(torch.from_numpy(np.ascontiguousarray(np.asarray(q)[:, :57], dtype=np.float64)).to(device))
    offs = np.concatenate([[0], np.cumsum([int(p.shape[0]) for p in parts])]).astype(np.int64)
    return (torch.cat(parts).contiguous(), torch.from_numpy(offs).to(device),
            torch.from_numpy(np.ascontiguousarray(scales, dtype=np.float64)).to(device), offs)


def synthesize(skel: Skeleton, qdq_list: Sequence, scales, device="cuda") -> List[dict]:
    """qdq_list[i] [L_i, >= 57] (numpy or CUDA tensors: root xyz, root axis-angle, the joints' axis-angles in nimble order; further
    columns are not read), scales [R] -> files[i] = {"imu": [L_i, 72], "constrs": [L_i, 20] (CUDA fp64, views of two tensors that hold
    all sequences back to back), "nimble_qdq": qdq_list[i] itself}: what the reference's generator pickles per motion, with scales[i]
    on every joint and COM offset and on the root xyz of sequence i (body_scale draws the reference's).
    ValueError before any device work: fewer than 9 rows in a sequence, a Skeleton without distinct valid SBP and IMU bodies, scales
    that are not one per sequence."""
    qdq_list, sc = _check_inputs(skel, qdq_list, scales)
    import torch
    device = _device(device)
    with torch.cuda.device(device):
        q, offsets, scale_dev, offs = upload(qdq_list, sc, device)
        P = tracked_poses(skel, q, offsets, scale_dev, device)
        imu = imu_readings(P, offsets, device)
        constrs = sbp_labels(skel, P, offsets, device)
    return [{"imu": imu[a:b], "constrs": constrs[a:b], "nimble_qdq": qdq_list[i]} for i, (a, b) in enumerate(zip(offs[:-1], offs[1:]))]
