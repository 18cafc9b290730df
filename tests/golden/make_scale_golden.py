#!/usr/bin/env python3
"""Golden fixture of the REFERENCE's full runner on SCALED characters, for the per-wearer body scale of tip_amd.kinematics and
tip_amd.terrain: the real RTRunner.step (real_time_runner.py), in both settings of multi_sbp_terrain_and_correction, started on a
character whose joint and COM offsets are multiplied by the scale — what SimAgent(scale=s) is (bullet_agent.py:47,67: PyBullet's
globalScaling), and what the reference's data generator builds with scale = h / 1.6 (data-gen-and-viz-bullet-new.py:256-257).

Runs only in the build container (it reads the reference checkout).  Everything comes from make_terrain_golden.py (kin_rows,
standing_rows, run_reference), make_kin_golden.py and make_runner_golden.py, imported unchanged: KinChar (real FK of data/amass.urdf
through tests/kin_oracle.py: PyBullet parity UNPINNED) is built here on the SCALED table; ScriptedModel, the scipy conversions
(fairmotion parity UNPINNED).  Options as there: five_sbp=True, with_acc_sum=True, map_bound=5.0, grid_size=0.1.

tests/golden/tip_scale_golden.npz (data only): table/* (the UNSCALED table), and per scale tag sA (0.875: tracks 1 and 2) and sB
(1.0625: tracks 0 and 2) make_terrain_golden's keys under sX/trackK/..., plus sX/scale.  s_init[2] of a track is multiplied by the
scale (and by nothing else), so that the standing character's feet stay near the ground.  Scales 1.1, 1.125, 1.15 and 1.2 bring a
decision of these tracks within 2.3e-5 .. 6.6e-5 of its threshold, under the bar below: not for equality tests.

The generator prints, and asserts, what make_terrain_golden.py does: every needed branch at least 3 times across the fixture; every
decision margin >= 1e-4; scale_oracle (terrain_oracle on the scaled table) in fp64 AND in float32 takes the reference's decisions on
every step and ends on its region map.

usage: python tests/golden/make_scale_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
REF = "/root/reference"

import kin_oracle as ko                # noqa: E402
import make_kin_golden as mkg          # noqa: E402
import make_runner_golden as mrg       # noqa: E402
import make_terrain_golden as mtg      # noqa: E402
import scale_oracle as so              # noqa: E402
import terrain_oracle as to            # noqa: E402

TRACKS = {"track0": lambda: mtg.kin_rows(200, 2), "track1": lambda: mtg.kin_rows(260, 7), "track2": lambda: mtg.standing_rows(250, 11)}
SCALES = (("sA", 0.875, ("track1", "track2")), ("sB", 1.0625, ("track0", "track2")))


def main():
    mrg.install_stubs(False)
    sys.modules["fairmotion.ops.quaternion"].Q_diff = mkg.q_diff
    sys.path.insert(0, REF)
    import amass_char_info as info
    from real_time_runner import RTRunner
    torch.Tensor.cuda = lambda self, *a, **k: self      # harness only
    table = ko.read_urdf(os.path.join(REF, "data", "amass.urdf"), info)
    out = {"table/" + k: v for k, v in table.items()}
    counts = {k: 0 for k in to.BRANCHES}
    margins = {k: np.inf for k in to.MARGINS}
    fk_impl = None
    for stag, scale, tags in SCALES:
        char, fk_impl = mkg.make_char(so.scaled_table(table, scale), info, False)      # the character the runner is given
        out[f"{stag}/scale"] = np.float64(scale)
        for tag in tags:
            y, imu, s_init = TRACKS[tag]()
            s_init = s_init.copy()
            s_init[2] *= scale
            shared = None
            for multi in (False, True):
                ref = mtg.run_reference(RTRunner, char, y, imu, s_init, multi)
                s_rest, ct, valid = ref["qdq"][:, 3:], ref["ct"], ref["valid"]
                assert not s_rest[:, 57:].any()
                pre = f"{stag}/{tag}/"
                if shared is None:
                    shared = (s_rest, ct, valid)
                    out.update({pre + "s_init": s_init, pre + "s_rest": s_rest[:, :57], pre + "ct": ct, pre + "valid": valid})
                assert all(np.array_equal(a, b) for a, b in zip(shared, (s_rest, ct, valid)))
                pre += f"m{int(multi)}/"
                rows = np.nonzero(ref["fire"])[0]
                out.update({pre + "root": ref["qdq"][:, :3], pre + "viz_locs": ref["viz_locs"], pre + "fire": ref["fire"],
                            pre + "fire_rows": rows, pre + "q_hist": ref["q_hist"][rows], pre + "ticks": ref["ticks"],
                            pre + "n_regions": ref["n_regions"], pre + "region_map": ref["region_map"].astype(np.int16),
                            pre + "region_height": ref["region_height"], pre + "region_weight": ref["region_weight"],
                            pre + "ik_deltas": ref["ik_deltas"]})
                for f in (np.float64, np.float32):
                    root, viz, qh, fire, st, tr = so.track_terrain(table, s_init, s_rest, ct, valid, scale, mtg.MAP_BOUND, mtg.GRID_SIZE,
                                                                   multi, 64, f)
                    same = (np.array_equal(tr["ticks"][valid], ref["ticks"][valid]) and np.array_equal(tr["n_regions"], ref["n_regions"])
                            and np.array_equal(fire, ref["fire"]) and np.array_equal(st.region_map, ref["region_map"]))
                    err = max(float(np.abs(root - ref["qdq"][:, :3]).max()), float(np.abs(viz - ref["viz_locs"]).max()),
                              float(np.abs(qh - ref["q_hist"]).max()))
                    print(f"scale {scale} {tag} multi={int(multi)} oracle {np.dtype(f).name}: decisions {'equal' if same else 'DIFFER'}, "
                          f"max error {err:.2e}")
                    assert same, (scale, tag, multi, f)
                    if f is np.float64:
                        c, m = tr["counts"], tr["margins"]
                        print(f"    branches {c}\n    margins " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()))
                        assert c["off_map"] == 0 and c["regions_full"] == 0
                        for k in counts:
                            counts[k] += c[k]
                        for k in margins:
                            margins[k] = min(margins[k], m[k])
    print("ACROSS THE FIXTURE: branches", counts)
    print("ACROSS THE FIXTURE: minimum margins", {k: float(f"{v:.3g}") for k, v in margins.items()})
    assert all(counts[k] >= mtg.MIN_BRANCH for k in mtg.NEEDED), counts
    assert all(v >= mtg.MIN_MARGIN for v in margins.values()), margins
    out["branch_counts"] = np.array([counts[k] for k in to.BRANCHES], dtype=np.int64)
    out["min_margins"] = np.array([margins[k] for k in to.MARGINS], dtype=np.float64)
    conv = "scipy stand-in (fairmotion fork absent: parity UNPINNED)"
    out["conversions_impl"] = np.frombuffer(conv.encode(), dtype=np.uint8).copy()
    out["fk_impl"] = np.frombuffer(fk_impl.encode(), dtype=np.uint8).copy()
    path = os.path.join(HERE, "tip_scale_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; FK:", fk_impl)
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
