#!/usr/bin/env python3
"""Golden fixture of the REFERENCE's full runner for tip_amd.terrain: the real RTRunner.step (real_time_runner.py) — root track,
height-region map, establishing-height ticks, vertical correction and leg IK — with a scripted model, in both settings of
multi_sbp_terrain_and_correction.

Runs only in the build container (it reads the reference checkout).  The reference's real_time_runner and data_utils are imported as
they are; what is not installed is stood in exactly as make_kin_golden.py does, and imported from there and from
make_runner_golden.py unchanged: KinChar (real FK of data/amass.urdf through tests/kin_oracle.py: PyBullet parity UNPINNED),
ScriptedModel, prepared_rows, imu_sequence, the scipy conversions (fairmotion parity UNPINNED; Q2A is scipy's as_rotvec).
Options: five_sbp=True, with_acc_sum=True, map_bound=5.0, grid_size=0.1.  The scripted model ignores its input, so the pose the runner
feeds back is captured by wrapping record_state_aa_and_c.

tests/golden/tip_terrain_golden.npz (data only).  Per track {0, 1, 2}:
  trackK/s_init [114], s_rest [n, 57] (qdq[3:60] of every step: columns 60 .. 113 are zero), ct [n, 20], valid [n] — the same in both modes
and per mode m in {0, 1} (multi_sbp_terrain_and_correction):
  trackK/mM/root [n, 3], viz_locs [n, 5, 3], fire [n], fire_rows, q_hist [len(fire_rows), 54] (the fed-back pose where it differs from
  the returned one), ticks [n, 3], n_regions [n] after every step, and the final region_map [100, 100], region_height, region_weight,
  ik_deltas [2, 3].
Tracks 0 and 1 are make_kin_golden.prepared_rows on seeds 2 and 7 over 200 and 260 frames (seed 5 comes within 2.3e-5 of the 0.1
region threshold, under the bar below); track 2 is a standing character made here,
which reaches what those do not: the region-0 rule, tick expiry under unbroken contact, the > 0.5 IK reset, the pelvis over the feet.
The off-map case cannot be recorded: the reference raises there (tests/test_terrain_gpu.py holds it to the oracle instead).

The generator prints, and asserts: every branch taken at least 3 times across the fixture; every decision margin (terrain_oracle's
trace) >= 1e-4; terrain_oracle in fp64 AND in float32 takes the reference's decisions on every step (ticks, region count, fire) and
ends on its region map.

usage: python tests/golden/make_terrain_golden.py
"""
import os
import sys

import numpy as np
import torch
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
REF = "/root/reference"

import kin_oracle as ko                # noqa: E402
import make_kin_golden as mkg          # noqa: E402
import make_runner_golden as mrg       # noqa: E402
import terrain_oracle as to            # noqa: E402

MAP_BOUND, GRID_SIZE, MIN_MARGIN, MIN_BRANCH = 5.0, 0.1, 1e-4, 3
NEEDED = ("merge", "new", "region0", "expiry", "ik_fire", "ik_small", "ik_reset", "pelvis_near")
UP = Rotation.from_rotvec([np.pi / 2, 0, 0])           # the character's zero pose has its legs along -y: y -> z


def standing_rows(n, seed):
    """Model rows, IMU frames and s_init of a character that stands upright and shifts its weight: feet near z = 0, the left foot in
    unbroken contact (its tick runs out every 52 frames), the right one stepping, and three fast swings of the left leg under contact."""
    rng = np.random.RandomState(seed)
    t = np.arange(n)[:, None] / 60.0
    k = np.arange(n)
    aa = 0.04 * rng.uniform(0.3, 1.0, 54) * np.sin(2 * np.pi * rng.uniform(0.3, 1.2, 54) * t + rng.uniform(0, 6, 54))
    for b, amp in ((70, 1.0), (130, -0.9), (190, 1.1)):
        aa[:, 3] += amp * np.exp(-((k - b) / 5.0) ** 2)                      # lhip about x
    vel = 0.05 * np.sin(2 * np.pi * rng.uniform(0.2, 0.6, 3) * t + rng.uniform(0, 6, 3))
    c_t = np.zeros((n, 20))
    on = [np.ones(n), (k % 12) < 8, (k // 7) % 2, (k // 9) % 2, ((k // 40) % 4) != 3]
    for i in range(5):
        c_t[:, 4 * i] = on[i]
        c_t[:, 4 * i + 1:4 * i + 4] = 0.03 * np.sin(2 * np.pi * rng.uniform(0.2, 1.0, 3) * t + rng.uniform(0, 6, 3))
    y = np.zeros((n, 131))
    y[:, :108] = Rotation.from_rotvec(aa.reshape(-1, 3)).as_matrix()[:, :, :2].reshape(n, 108)
    y[:, 108:111] = vel
    y[:, 111:] = c_t
    y[:, 111::4] = np.where(c_t[:, 0::4] > 0, 1.0, -1.0)
    for j in (1, 2, 3):
        y[:, 111 + j::4] *= 5.0
    imu = mrg.smooth_imu_sequence(n, seed)
    yaw = 0.3 * np.sin(2 * np.pi * 0.2 * t[:, 0])
    imu[:, :9] = (Rotation.from_rotvec(np.stack([0 * yaw, 0 * yaw, yaw], axis=1)) * UP).as_matrix().reshape(n, 9)
    s_init = np.zeros(114)
    s_init[:3] = [0.2, -0.1, 0.93]
    s_init[3:6] = UP.as_rotvec()
    return y, imu, s_init


def kin_rows(n, seed):
    rng = np.random.RandomState(500 + seed)
    s_init = np.zeros(114)
    s_init[3:57] = rng.randn(54) * 0.3
    s_init[:3] = [0.2, -0.1, 0.95]
    return mkg.prepared_rows(n, seed), mkg.imu_sequence(n, seed), s_init


def run_reference(RTRunner, char, y, imu, s_init, multi):
    n_frames = y.shape[0]
    model = mkg.ScriptedModel(y)
    runner = RTRunner(char, model, 40, s_init, MAP_BOUND, GRID_SIZE, five_sbp=True, with_acc_sum=True,
                      multi_sbp_terrain_and_correction=multi)
    fed, record = [], runner.record_state_aa_and_c

    def tapped(cur_s, cur_c):
        fed.append(np.array(cur_s[3:57]).copy())
        return record(cur_s, cur_c)

    runner.record_state_aa_and_c = tapped
    s_traj = np.zeros((n_frames, 114))
    s_traj[0] = s_init
    out = {k: [] for k in ("qdq", "ct", "viz_locs", "valid", "q_hist", "ticks", "n_regions")}
    for t in range(n_frames - 1):                                            # the script's loop (offline_testing_simple.py:123-139)
        calls, n_fed = model.k, len(fed)
        res = runner.step(imu[t], s_traj[t, :3], t)
        s_traj[t + 1] = res["qdq"]
        qdq = np.array(res["qdq"]).copy()
        out["qdq"].append(qdq)
        out["ct"].append(np.array(res["ct"]).copy())
        out["viz_locs"].append(np.array(res["viz_locs"]).copy())
        out["valid"].append(model.k > calls)
        out["q_hist"].append(fed[-1] if len(fed) > n_fed else qdq[3:57].copy())
        out["ticks"].append([runner.establishing_height_phase_tick[k] for k in ("lankle", "rankle", "root")])
        out["n_regions"].append(len(runner.region_height_list))
    out = {k: np.array(v) for k, v in out.items()}
    out["fire"] = (out["q_hist"] != out["qdq"][:, 3:57]).any(axis=1)
    out["region_map"] = np.array(runner.height_region_map)
    out["region_height"] = np.array(runner.region_height_list, dtype=np.float64)
    out["region_weight"] = np.array(runner.region_weight_list, dtype=np.float64)
    out["ik_deltas"] = np.stack([runner.ik_target_deltas["lankle"], runner.ik_target_deltas["rankle"]])
    conf = np.array(runner.height_confidence_map)
    out["min_border"] = int(min(np.nonzero(conf > -100)[0].min(), np.nonzero(conf > -100)[1].min(),
                                conf.shape[0] - 1 - np.nonzero(conf > -100)[0].max(), conf.shape[1] - 1 - np.nonzero(conf > -100)[1].max()))
    return out


def main():
    mrg.install_stubs(False)
    sys.modules["fairmotion.ops.quaternion"].Q_diff = mkg.q_diff
    sys.path.insert(0, REF)
    import amass_char_info as info
    from real_time_runner import RTRunner
    torch.Tensor.cuda = lambda self, *a, **k: self      # harness only
    table = ko.read_urdf(os.path.join(REF, "data", "amass.urdf"), info)
    char, fk_impl = mkg.make_char(table, info, False)
    assert to.grid_num(MAP_BOUND, GRID_SIZE) == 100 and to.diffuse_region(GRID_SIZE) == 5
    out = {"table/" + k: v for k, v in table.items()}
    counts = {k: 0 for k in to.BRANCHES}
    margins = {k: np.inf for k in to.MARGINS}
    tracks = (("track0", kin_rows(200, 2)), ("track1", kin_rows(260, 7)), ("track2", standing_rows(250, 11)))
    for tag, (y, imu, s_init) in tracks:
        shared = None
        for multi in (False, True):
            ref = run_reference(RTRunner, char, y, imu, s_init, multi)
            s_rest, ct, valid = ref["qdq"][:, 3:], ref["ct"], ref["valid"]
            assert not s_rest[:, 57:].any()
            if shared is None:
                shared = (s_rest, ct, valid)
                out.update({f"{tag}/s_init": s_init, f"{tag}/s_rest": s_rest[:, :57], f"{tag}/ct": ct, f"{tag}/valid": valid})
            assert all(np.array_equal(a, b) for a, b in zip(shared, (s_rest, ct, valid)))
            pre = f"{tag}/m{int(multi)}/"
            rows = np.nonzero(ref["fire"])[0]
            out.update({pre + "root": ref["qdq"][:, :3], pre + "viz_locs": ref["viz_locs"], pre + "fire": ref["fire"],
                        pre + "fire_rows": rows, pre + "q_hist": ref["q_hist"][rows], pre + "ticks": ref["ticks"],
                        pre + "n_regions": ref["n_regions"], pre + "region_map": ref["region_map"].astype(np.int16),
                        pre + "region_height": ref["region_height"], pre + "region_weight": ref["region_weight"],
                        pre + "ik_deltas": ref["ik_deltas"]})
            for f in (np.float64, np.float32):
                root, viz, qh, fire, st, tr = to.track(table, s_init, s_rest, ct, valid, MAP_BOUND, GRID_SIZE, multi, 64, f)
                same = (np.array_equal(tr["ticks"][valid], ref["ticks"][valid]) and np.array_equal(tr["n_regions"], ref["n_regions"])
                        and np.array_equal(fire, ref["fire"]) and np.array_equal(st.region_map, ref["region_map"]))
                err = max(float(np.abs(root - ref["qdq"][:, :3]).max()), float(np.abs(viz - ref["viz_locs"]).max()),
                          float(np.abs(qh - ref["q_hist"]).max()))
                print(f"{tag} multi={int(multi)} oracle {np.dtype(f).name}: decisions {'equal' if same else 'DIFFER'}, max error {err:.2e}")
                assert same, (tag, multi, f)
                if f is np.float64:
                    c, m = tr["counts"], tr["margins"]
                    updates = c["merge"] + c["new"] + c["region0"]
                    print(f"{tag} multi={int(multi)}: frames {y.shape[0]}, regions {len(st.region_height)}, map updates {updates}, "
                          f"patches >= {ref['min_border']} cells from the border\n    branches {c}\n    margins "
                          + ", ".join(f"{k} {v:.2e}" for k, v in m.items()))
                    assert c["off_map"] == 0 and c["regions_full"] == 0
                    for k in counts:
                        counts[k] += c[k]
                    for k in margins:
                        margins[k] = min(margins[k], m[k])
    print("ACROSS THE FIXTURE: branches", counts)
    print("ACROSS THE FIXTURE: minimum margins", {k: float(f"{v:.3g}") for k, v in margins.items()})
    assert all(counts[k] >= MIN_BRANCH for k in NEEDED), counts
    assert all(v >= MIN_MARGIN for v in margins.values()), margins
    out["branch_counts"] = np.array([counts[k] for k in to.BRANCHES], dtype=np.int64)
    out["min_margins"] = np.array([margins[k] for k in to.MARGINS], dtype=np.float64)
    conv = "scipy stand-in (fairmotion fork absent: parity UNPINNED)"
    out["conversions_impl"] = np.frombuffer(conv.encode(), dtype=np.uint8).copy()
    out["fk_impl"] = np.frombuffer(fk_impl.encode(), dtype=np.uint8).copy()
    path = os.path.join(HERE, "tip_terrain_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; FK:", fk_impl)
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
