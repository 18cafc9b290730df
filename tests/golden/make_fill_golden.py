#!/usr/bin/env python
"""Golden fixture of the REFERENCE's preparation of real IMU recordings, for tip_amd.sensors.real_imu_frames and the oracle in
tests/sensor_fill_oracle.py: tests/golden/tip_fill_golden.npz.

Runs only where the reference checkout is (argument 1, default /root/reference).  The two functions — fill_in_nan_values and
get_real_imu_readings_ours_format_knee of preprocess_DIP_TC_new.py — are cut out of the file with `ast` when this script runs and are
executed as they are, with `np` and ROT_MAT_OURS in their namespace (the file itself imports fairmotion and pybullet at module level,
which this project does not depend on).  Nothing of the reference's text is stored: the fixture holds the inputs this script draws
and the arrays the reference returns for them.

Three recordings of 17 sensors (L = 12, 37, 120), each through both corpora's rotations (ROT_DIP, ROT_TC) with the DIP selection of
sensors.  The script counts the bad parts per branch of the rule among the six selected sensors, asserts at least 3 of each and stores
the counts; that the reference returned at all says its own finiteness assertions held.

    python tests/golden/make_fill_golden.py [reference checkout]
"""
import ast
import os
import sys

import numpy as np
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import sensor_fill_oracle as fo  # noqa: E402
from tip_amd import sensors  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
OUT = os.path.join(HERE, "tip_fill_golden.npz")
LENGTHS = (12, 37, 120)
SEEDS = (16, 46, 180)
BRANCHES = ("t_lt_10", "t_eq_10", "t_gt_10", "in_long_run", "one_element", "rotation_only", "acceleration_only")


def reference_functions(rot):
    tree = ast.parse(open(os.path.join(REF, "preprocess_DIP_TC_new.py")).read())
    want = ("fill_in_nan_values", "get_real_imu_readings_ours_format_knee")
    nodes = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert sorted(n.name for n in nodes) == sorted(want)
    ns = {"np": np, "ROT_MAT_OURS": rot}
    exec(compile(ast.Module(body=nodes, type_ignores=[]), "preprocess_DIP_TC_new.py", "exec"), ns)
    return ns["get_real_imu_readings_ours_format_knee"]


def draw(L, seed):
    """A recording with every branch of the rule in it; values are float32-representable (the file compresses better)."""
    rng = np.random.RandomState(seed)
    whole = [(7, 14, 23), (0, 20, 35)] if L >= 37 else []        # whole-sensor runs of 9 and 15 rows
    if L >= 120:
        whole += [(11, 60, 67), (2, 90, 101)]
    ori, acc = fo.recording(rng, L, 17, p_bad=0.1, whole=whole)
    ori = ori.astype(np.float32).astype(np.float64)
    acc = acc.astype(np.float32).astype(np.float64)
    if L > 10:                                                   # t == 10: the last row that is filled from rows 0 .. 9
        ori[10, 8] = np.nan
        acc[10, 12] = np.nan
    ori[0, 12] = np.nan                                          # row 0 itself, filled from the rows ahead
    for s in sensors.SEL_DIP17:                                  # every selected sensor reads something in rows 0 .. 9
        ori[3, s] = np.float32(rng.normal(size=(3, 3)))
        acc[4, s] = np.float32(rng.normal(size=3))
    return ori, acc


def count_branches(ori, acc):
    L = ori.shape[0]
    sel = list(sensors.SEL_DIP17)
    Ho, Ha = ori[:, sel].reshape(L, 6, 9), acc[:, sel].reshape(L, 6, 3)
    bo, ba = fo.bad_mask(Ho), fo.bad_mask(Ha)
    c = dict.fromkeys(BRANCHES, 0)
    t = np.arange(L)[:, None]
    for bad, H in ((bo, Ho), (ba, Ha)):
        c["t_lt_10"] += int((bad & (t < 10)).sum())
        c["t_eq_10"] += int((bad & (t == 10)).sum())
        c["t_gt_10"] += int((bad & (t > 10)).sum())
        c["one_element"] += int((bad & (np.isnan(H).sum(axis=2) == 1)).sum())
        for i in range(6):
            a = 0
            while a < L:                                         # runs of 7 or more bad rows: from the sixth row on (t > 10) a fill
                b = a                                            # feeds on fills only
                while b < L and bad[b, i]:
                    b += 1
                if b - a >= 7:
                    c["in_long_run"] += sum(1 for tt in range(a + 5, b) if tt > 10)
                a = max(b, a + 1)
    c["rotation_only"] = int((bo & ~ba).sum())
    c["acceleration_only"] = int((ba & ~bo).sum())
    return c


def main():
    rots = {"dip": sensors.ROT_DIP, "tc": sensors.ROT_TC}
    assert np.array_equal(sensors.ROT_DIP, Rotation.from_quat([0.5, 0.5, 0.5, 0.5]).as_matrix().round())
    assert np.array_equal(sensors.ROT_TC, Rotation.from_rotvec([np.pi / 2, 0, 0]).as_matrix())
    store, totals, filled = {"lengths": np.array(LENGTHS)}, dict.fromkeys(BRANCHES, 0), []
    for i, (L, seed) in enumerate(zip(LENGTHS, SEEDS)):
        ori, acc = draw(L, seed)
        store[f"ori_{i}"], store[f"acc_{i}"] = ori, acc
        for name, rot in rots.items():
            out = reference_functions(rot)(ori.copy(), acc.copy())       # (its two `assert np.isfinite` are inside)
            assert out.shape == (L, 72) and np.isfinite(out).all()
            store[f"out_{name}_{i}"] = out
            mine, unfilled = fo.real_frames(ori, acc, rot, sensors.SEL_DIP17)
            assert unfilled == 0
            assert np.array_equal(mine, out) if name == "dip" else np.abs(mine - out).max() < 1e-13
        c = count_branches(ori, acc)
        filled.append(c["t_lt_10"] + c["t_eq_10"] + c["t_gt_10"])
        for k in BRANCHES:
            totals[k] += c[k]
        print(f"L = {L}: {filled[-1]} filled parts, {c}")
    for k in BRANCHES:
        assert totals[k] >= 3, (k, totals)
    store["branch_names"] = np.array(BRANCHES)
    store["branch_counts"] = np.array([totals[k] for k in BRANCHES])
    store["filled_parts"] = np.array(filled)
    np.savez_compressed(OUT, **store)
    size = os.path.getsize(OUT)
    print(f"{OUT}: {size} bytes; branches {totals}")
    assert size < 500_000


if __name__ == "__main__":
    main()
