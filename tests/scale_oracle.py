"""What a wearer's body scale means, for the tests: a table whose joint and COM offsets are multiplied by the scale — the character a
SimAgent(scale=s) is (bullet_agent.py:47,67: PyBullet's globalScaling) — run through tests/kin_oracle.py and tests/terrain_oracle.py as
they stand.  Nothing else is scaled: not the root of q / s_init, not c_t's vectors, no threshold of either runner.  Thin per-sequence
wrappers; it imports nothing of tip_amd."""
import numpy as np

import kin_oracle as ko
import terrain_oracle as to


def scaled_table(table, s, dtype=np.float64):
    """`table` with joint_xyz and com_xyz times s, the product taken in `dtype` (the float32 restatement rounds the offsets, the scale
    and their product to float32, as float32 code does); everything else the same arrays."""
    t = dict(table.items()) if hasattr(table, "items") else {k: table[k] for k in table.files}
    t["joint_xyz"] = np.asarray(table["joint_xyz"]).astype(dtype) * dtype(s)
    t["com_xyz"] = np.asarray(table["com_xyz"]).astype(dtype) * dtype(s)
    return t


def fk(table, q, scales, dtype=np.float64):
    """(pq_g, pq_jf) [N, L + 1, 7] of q [N, >= 57] with one scale per row."""
    q = np.asarray(q)
    scales = np.broadcast_to(np.asarray(scales, dtype=np.float64), (q.shape[0],))
    L = len(table["parent"])
    g, jf = np.zeros((q.shape[0], L + 1, 7), dtype=dtype), np.zeros((q.shape[0], L + 1, 7), dtype=dtype)
    for s in np.unique(scales):
        rows = np.nonzero(scales == s)[0]
        g[rows], jf[rows] = ko.fk(scaled_table(table, s, dtype), q[rows], dtype)
    return g, jf


def track_ragged(table, s_init, s_rest, c_t, valid, offsets, scales, dtype=np.float64):
    """kin_oracle.track per sequence, each on its own scaled table: root [N, 3], viz_locs [N, 5, 3], row for row."""
    offsets = np.asarray(offsets, dtype=np.int64)
    root, viz = [], []
    for i, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        r, v, _ = ko.track(scaled_table(table, scales[i], dtype), np.asarray(s_init)[i], s_rest[a:b], c_t[a:b], valid[a:b], dtype)
        root.append(r), viz.append(v)
    return np.concatenate(root), np.concatenate(viz)


def track_terrain(table, s_init, s_rest, c_t, valid, scale, map_bound=5.0, grid_size=0.1, multi_sbp=False, max_regions=64,
                  dtype=np.float64):
    """terrain_oracle.track of one sequence on the table scaled by `scale`: (root, viz_locs, q_hist, fire, State, trace)."""
    return to.track(scaled_table(table, scale, dtype), s_init, s_rest, c_t, valid, map_bound, grid_size, multi_sbp, max_regions, dtype)


def track_terrain_ragged(table, s_init, s_rest, c_t, valid, offsets, scales, dtype=np.float64, **kw):
    """track_terrain per sequence: root [N, 3], viz_locs [N, 5, 3], q_hist [N, 54], fire [N] (the sequence's index where the IK rewrote
    the pose, -1 elsewhere: what the device writes) and the list of States."""
    offsets = np.asarray(offsets, dtype=np.int64)
    outs, states = [[], [], [], []], []
    for i, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        r, v, q, f, st, _ = track_terrain(table, np.asarray(s_init)[i], s_rest[a:b], c_t[a:b], valid[a:b], scales[i], dtype=dtype, **kw)
        for o, x in zip(outs, (r, v, q, np.where(f, i, -1).astype(np.int32))):
            o.append(x)
        states.append(st)
    return (*[np.concatenate(o) for o in outs], states)


def evaluate(table, pred_qdq, gt_qdq, offsets, scales, start=30, end=6, dtype=np.float64):
    """kin_oracle.evaluate per file, both trajectories through FK on the file's scaled table: [R, 7]."""
    offsets = np.asarray(offsets, dtype=np.int64)
    return np.stack([np.asarray(ko.evaluate(scaled_table(table, scales[i], dtype), pred_qdq[a:b], gt_qdq[a:b], start, end, dtype), dtype=np.float64)
                     for i, (a, b) in enumerate(zip(offsets[:-1], offsets[1:]))])
