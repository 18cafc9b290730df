"""What the full runner's tail costs on the device (tip_amd.terrain; csrc/tip_terrain.hip), and what it replaces.

    python tools/terrain_bench.py [--out FILE]   -> one JSON line per measurement + a table on stderr; FILE (default: the record,
                                                    profiles/terrain/terrain_bench.txt) gets a header and the same lines

  live       TerrainTracker.step + feed_back beside StreamingEngine.step at 1 / 256 / 1024 slots (use_graph=True, multi_sbp on, past the
             warm-up), against the engine frame alone and against RootTracker.step on the same slots: alternating blocks, best block, as
             tools/kin_bench.py
  host_loop  what a user of RTRunner had before: download the frame's s_rest / c_t, tests/terrain_oracle.py's step per stream (numpy,
             fp64), the host override_history — at 1 and 256 streams over 3 frames, one frame at 1024
  post       track_terrain on 50 files x 600 frames (device events, median of 20 after 3 warm-up calls, inputs on the device) against
             the fp64 numpy oracle's host time on 5 of the files, scaled
  kernels    the reset launch (all slots, map 100 and 200 cells a side) and the step launch alone, 200 back to back, at 1 / 256 / 1024
  grid       the structural check: the step at grid_num 100 and 200 (map_bound 5 and 10), 5 repeats each, alternating — the step
             touches a patch, never a map, so the two must differ by no more than the repeats of one differ among themselves
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tip_amd  # noqa: E402
from tip_amd import kinematics as kin, terrain  # noqa: E402
import kin_oracle as ko  # noqa: E402
import terrain_oracle as to  # noqa: E402
from kin_bench import corpus, event_ms, FILES, FRAMES, SIZES  # noqa: E402
from staggered_bench import model, alternate, emit, frames  # noqa: E402


def fabricated(n, seed=7):
    """An engine-shaped frame of n slots whose rows are scripted runner outputs (the synthetic model's own are noise to a tracker)."""
    rows = [ko.scripted_rows(8, seed + i) for i in range(min(n, 32))]
    s_rest = np.stack([rows[i % len(rows)][0] for i in range(n)], axis=1).astype(np.float32)      # [8, n, 111]
    c_t = np.stack([rows[i % len(rows)][1] for i in range(n)], axis=1).astype(np.float32)
    s_init = np.stack([rows[i % len(rows)][2] for i in range(n)]).astype(np.float32)
    return torch.from_numpy(s_rest).cuda(), torch.from_numpy(c_t).cuda(), s_init


def main():
    torch.backends.cudnn.benchmark = False
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "terrain", "terrain_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "tip_kin_golden.npz"))
    skel = kin.Skeleton.from_table(golden)
    table = skel.table()
    recs = []

    def note(rec):
        emit(rec)
        recs.append(rec)

    # ---- post-pass
    s_init, s_rest, c_t, valid, offs = corpus()
    dev = [torch.from_numpy(a).cuda() for a in (s_init, s_rest, c_t)] + [torch.from_numpy(valid).cuda()]
    for multi in (False, True):
        med, lo, hi = event_ms(lambda: terrain.track_terrain(skel, dev[0], dev[1], dev[2], dev[3], offs, multi_sbp=multi))
        note({"what": "post", "multi_sbp": multi, "files": FILES, "frames": FRAMES, "ms_median": round(med, 4), "ms_min": round(lo, 4),
              "ms_max": round(hi, 4)})
    root = terrain.track_terrain(skel, dev[0], dev[1], dev[2], dev[3], offs, multi_sbp=True)[0].cpu().numpy()
    t0 = time.perf_counter()
    worst = 0.0
    for i in range(5):
        a, b = offs[i], offs[i + 1]
        o = to.track(table, s_init[i], s_rest[a:b], c_t[a:b], valid[a:b], 5.0, 0.1, True, 64)
        worst = max(worst, float(np.abs(root[a:b] - o[0]).max()))
    host = (time.perf_counter() - t0) / 5 * FILES
    note({"what": "post_oracle", "host_s_for_50_files": round(host, 2), "device_root_minus_oracle_5_files": worst})

    m = model()
    for n in SIZES:
        fr, s0 = frames(n, n)
        sd, cd, si = fabricated(n)
        engines = [tip_amd.streaming.StreamingEngine(m, s0, use_graph=True) for _ in range(3)]
        rt = kin.RootTracker(skel, n, "cuda")
        rt.reset(None, si)
        tt = terrain.TerrainTracker(skel, n, "cuda", multi_sbp=True)
        tt.reset(None, si)
        for f in range(50):                           # past the warm-up: every window at T = 40
            for e in engines:
                e.step(fr[f % len(fr)])
        torch.cuda.synchronize()

        def fab(i):
            return {"s_rest": sd[i % 8], "c_t": cd[i % 8]}

        def rooted(i):
            engines[1].step(fr[i % len(fr)])
            rt.step(fab(i))

        def full(i):
            engines[2].step(fr[i % len(fr)])
            tt.step(fab(i))
            tt.feed_back(engines[2])

        res = alternate({"engine": lambda i: engines[0].step(fr[i % len(fr)]), "root": rooted, "terrain": full})
        step_alone = event_ms(lambda: [tt.step(fab(k)) for k in range(200)], warm=1, reps=5)[1] / 200 * 1e3
        both_alone = event_ms(lambda: [(tt.step(fab(k)), tt.feed_back(engines[2])) for k in range(200)], warm=1, reps=5)[1] / 200 * 1e3
        reset_us = {}
        for mb in (5.0, 10.0):
            t2 = terrain.TerrainTracker(skel, n, "cuda", map_bound=mb, multi_sbp=True)
            reset_us[int(mb)] = event_ms(lambda: t2.reset(None, si), warm=1, reps=5)[1] * 1e3
            del t2
        note({"what": "live", "n": n, "engine_ms": round(res["engine"], 4), "engine_plus_root_tracker_ms": round(res["root"], 4),
              "engine_plus_terrain_and_feed_back_ms": round(res["terrain"], 4),
              "root_tracker_delta_us": round((res["root"] - res["engine"]) * 1e3, 1),
              "terrain_delta_us": round((res["terrain"] - res["engine"]) * 1e3, 1), "step_us_per_launch": round(step_alone, 2),
              "step_plus_feed_back_us": round(both_alone, 2), "reset_us_grid_100": round(reset_us[5], 1),
              "reset_us_grid_200": round(reset_us[10], 1), "fired": int((tt.fire >= 0).sum()), "root_finite": bool(torch.isfinite(tt.root).all())})
        # the host loop this replaces
        G, D = to.grid_num(5.0, 0.1), to.diffuse_region(0.1)
        states = [to.State(table, si[i], G, 64, np.float64) for i in range(n)]
        tr = to.new_trace()
        n_frames = 3 if n <= 256 else 1
        last = engines[1].step(fr[0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(n_frames):
            s_h, c_h = sd[f].cpu().numpy().astype(np.float64), cd[f].cpu().numpy().astype(np.float64)
            q, sel = [], []
            for i in range(n):
                _, _, qh, fired = to.step(table, states[i], s_h[i], c_h[i], G, D, 0.1, True, np.float64, tr, f)
                if fired:
                    q.append(qh), sel.append(i)
            if sel:
                engines[1].override_history(np.stack(q).astype(np.float32), sel)
            torch.cuda.synchronize()
        note({"what": "host_loop", "n": n, "frames": n_frames, "ms_per_frame": round((time.perf_counter() - t0) / n_frames * 1e3, 2)})
        del engines, rt, tt, last

    # ---- the structural check: the step does not see the size of the map
    n = 256
    sd, cd, si = fabricated(n)
    small = terrain.TerrainTracker(skel, n, "cuda", map_bound=5.0, multi_sbp=True)
    large = terrain.TerrainTracker(skel, n, "cuda", map_bound=10.0, multi_sbp=True)
    small.reset(None, si), large.reset(None, si)
    runs = {100: [], 200: []}
    for _ in range(5):
        for g, t in ((100, small), (200, large)):
            runs[g].append(event_ms(lambda: [t.step({"s_rest": sd[k % 8], "c_t": cd[k % 8]}) for k in range(200)], warm=1, reps=3)[1] / 200 * 1e3)
    spread = max(max(v) - min(v) for v in runs.values())
    diff = abs(statistics.median(runs[100]) - statistics.median(runs[200]))
    note({"what": "grid", "n": n, "step_us_grid_100": [round(v, 2) for v in runs[100]], "step_us_grid_200": [round(v, 2) for v in runs[200]],
          "median_difference_us": round(diff, 2), "repeat_spread_us": round(spread, 2), "within_spread": bool(diff <= spread)})
    m.check_handoffs()
    with open(out_path, "w") as fh:
        fh.write("# tools/terrain_bench.py on one MI355X, one run: TerrainTracker.step + feed_back beside StreamingEngine.step (graph mode,\n"
                 "# alternating blocks, best block; launches alone: 200 back to back), the host loop it replaces (download, terrain_oracle per\n"
                 "# stream in fp64 numpy, host override_history), track_terrain on 50 files x 600 frames (device events, median of 20), and the\n"
                 "# step at maps of 100 and 200 cells a side\n")
        for r in recs:
            fh.write(json.dumps(r) + "\n")
    for r in recs:
        print(r, file=sys.stderr)


if __name__ == "__main__":
    main()
