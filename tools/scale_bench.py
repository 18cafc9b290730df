"""What the per-wearer body scale costs (tip_amd.kinematics / tip_amd.terrain with scales; the SCALED = true kernels of csrc/tip_kin.hip and
csrc/tip_terrain.hip): the scaled and the unscaled launch of the same work, alternated in one process on one tree.

    python tools/scale_bench.py [--out FILE]   -> one JSON line per measurement + a table on stderr; FILE (default: the record,
                                                  profiles/kin/scale_bench.txt) gets a header and the same lines

  post   track and track_terrain (multi_sbp off and on) on 50 files x 600 rows, inputs on the device: REPS rounds of (unscaled, scaled),
         each a median of 5 calls by device events after 2 warm-up calls
  live   RootTracker.step and TerrainTracker.step (multi_sbp on) at 1 / 256 / 1024 slots on fabricated frames, 200 launches back to back:
         REPS rounds of (unscaled tracker, scaled tracker), microseconds per launch

Per measurement: the medians of both columns over the rounds, each column's scatter (max - min over its rounds) and the difference of the
medians.  The scaled trackers carry scales spread over 0.85 .. 1.2 (the value does not change the work).  No bound is asserted."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tip_amd  # noqa: E402,F401
from tip_amd import kinematics as kin, terrain  # noqa: E402
from kin_bench import corpus, event_ms, FILES, FRAMES, SIZES  # noqa: E402
from terrain_bench import fabricated  # noqa: E402

REPS = 7


def scales_for(n):
    return np.linspace(0.85, 1.2, n).astype(np.float32)


def rounds(plain, scaled, unit):
    """REPS rounds of (plain(), scaled()), each returning one figure: the record's two columns."""
    cols = {"unscaled": [], "scaled": []}
    for _ in range(REPS):
        cols["unscaled"].append(plain())
        cols["scaled"].append(scaled())
    med = {k: statistics.median(v) for k, v in cols.items()}
    scatter = {k: max(v) - min(v) for k, v in cols.items()}
    diff = med["scaled"] - med["unscaled"]
    return {f"unscaled_{unit}": round(med["unscaled"], 4), f"scaled_{unit}": round(med["scaled"], 4),
            f"unscaled_scatter_{unit}": round(scatter["unscaled"], 4), f"scaled_scatter_{unit}": round(scatter["scaled"], 4),
            f"scaled_minus_unscaled_{unit}": round(diff, 4), "within_scatter": bool(abs(diff) <= max(scatter.values())),
            "rounds": {k: [round(x, 4) for x in v] for k, v in cols.items()}}


def main():
    torch.backends.cudnn.benchmark = False
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "kin", "scale_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    skel = kin.Skeleton.from_table(np.load(os.path.join(ROOT, "tests", "golden", "tip_kin_golden.npz")))
    recs = []

    def note(rec):
        print(json.dumps(rec), flush=True)
        recs.append(rec)

    # ---- the post-pass
    s_init, s_rest, c_t, valid, offs = corpus()
    dev = [torch.from_numpy(a).cuda() for a in (s_init, s_rest, c_t)] + [torch.from_numpy(valid).cuda()]
    sc = scales_for(FILES)

    def post(fn, **kw):
        return lambda: event_ms(lambda: fn(skel, dev[0], dev[1], dev[2], dev[3], offs, **kw), warm=2, reps=5)[0]

    note({"what": "track", "files": FILES, "rows": FRAMES, **rounds(post(kin.track), post(kin.track, scales=sc), "ms")})
    for multi in (False, True):
        note({"what": "track_terrain", "multi_sbp": multi, "files": FILES, "rows": FRAMES,
              **rounds(post(terrain.track_terrain, multi_sbp=multi), post(terrain.track_terrain, multi_sbp=multi, scales=sc), "ms")})

    # ---- the live step, launches alone
    for n in SIZES:
        sd, cd, si = fabricated(n)
        for what, make in (("RootTracker.step", lambda: kin.RootTracker(skel, n, "cuda")),
                           ("TerrainTracker.step", lambda: terrain.TerrainTracker(skel, n, "cuda", multi_sbp=True))):
            plain, scaled = make(), make()
            plain.reset(None, si)
            scaled.reset(None, si, scales=scales_for(n))
            assert plain.entries[1] + "_scaled" == scaled.entries[1]

            def step(t):
                return lambda: event_ms(lambda: [t.step({"s_rest": sd[k % 8], "c_t": cd[k % 8]}) for k in range(200)], warm=1, reps=3)[1] / 200 * 1e3

            note({"what": what, "n": n, "entries": [plain.entries[1], scaled.entries[1]], **rounds(step(plain), step(scaled), "us"),
                  "root_finite": bool(torch.isfinite(plain.root).all() and torch.isfinite(scaled.root).all())})
            del plain, scaled
    with open(out_path, "w") as fh:
        fh.write("# tools/scale_bench.py on one MI355X, one run, one process: the unscaled and the scaled (per-wearer body scale) launch of the\n"
                 f"# same work, alternated over {REPS} rounds.  track / track_terrain: 50 files x 600 rows, ms per call (median of 5 by device\n"
                 "# events per round).  RootTracker.step / TerrainTracker.step: us per launch, 200 launches back to back (best of 3 per round).\n"
                 "# scatter: max - min of a column over its rounds.\n")
        for r in recs:
            fh.write(json.dumps(r) + "\n")
    for r in recs:
        print({k: v for k, v in r.items() if k != "rounds"}, file=sys.stderr)


if __name__ == "__main__":
    main()
