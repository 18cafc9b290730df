"""What the kinematics post-pass and the live root tracker cost (tip_amd.kinematics; csrc/tip_kin.hip), on the evaluation script's
size: 50 files of 600 frames.

    python tools/kin_bench.py [--out FILE]   -> one JSON line per measurement + a table on stderr; FILE (default: the record,
                                                profiles/kin/kin_bench.txt) gets a header and the same lines

  track      kinematics.track on the 50 x 600 rows, inputs already on the device: device events around the call (the reset launch, the
             offsets upload and the one tracker kernel), median of 20 after 3 warm-up calls
  evaluate   kinematics.evaluate on the same rows against a perturbed copy (two FK launches, the metrics kernel, the read-back)
  fk         kinematics.fk on the 30 000 poses alone
  live       RootTracker.step beside StreamingEngine.step at 1 / 256 / 1024 slots, use_graph=True, past the warm-up: the engine frame
             alone against the engine frame + the tracker's launch, alternating in blocks (best block, as tools/sensor_bench.py), and
             the launch alone back to back
  oracle     tests/kin_oracle.py's fp64 numpy restatement of track and evaluate on the same rows, host wall time, once: the only
             baseline there is (the reference does this through PyBullet, which is not installed here)
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
from tip_amd import kinematics as kin  # noqa: E402
import kin_oracle as ko  # noqa: E402
from staggered_bench import model, alternate, emit, frames  # noqa: E402

FILES, FRAMES = 50, 600
SIZES = (1, 256, 1024)


def corpus():
    rows = [ko.scripted_rows(FRAMES, 1000 + i) for i in range(FILES)]
    s_rest = np.concatenate([r[0] for r in rows]).astype(np.float32)
    c_t = np.concatenate([r[1] for r in rows]).astype(np.float32)
    s_init = np.stack([r[2] for r in rows]).astype(np.float32)
    valid = np.concatenate([np.arange(FRAMES) >= 6 for _ in range(FILES)])
    offs = np.arange(FILES + 1, dtype=np.int64) * FRAMES
    return s_init, s_rest, c_t, valid, offs


def event_ms(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    out = []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    torch.backends.cudnn.benchmark = False
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "kin", "kin_bench.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "tip_kin_golden.npz"))
    skel = kin.Skeleton.from_table(golden)
    table = skel.table()
    s_init, s_rest, c_t, valid, offs = corpus()
    dev = [torch.from_numpy(a).cuda() for a in (s_init, s_rest, c_t)] + [torch.from_numpy(valid).cuda()]
    recs = []

    def note(rec):
        emit(rec)
        recs.append(rec)

    med, lo, hi = event_ms(lambda: kin.track(skel, dev[0], dev[1], dev[2], dev[3], offs))
    note({"what": "track", "files": FILES, "frames": FRAMES, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)})
    root = kin.track(skel, dev[0], dev[1], dev[2], dev[3], offs)[0]
    qdq = torch.cat([root, dev[1]], dim=1).contiguous()
    gt = qdq.clone()
    gt[:, :57] += 0.03 * torch.sin(torch.arange(qdq.shape[0], device="cuda")[:, None] / 37.0 + torch.arange(57, device="cuda")[None])
    med, lo, hi = event_ms(lambda: kin.evaluate(skel, qdq, gt, offs))
    note({"what": "evaluate", "files": FILES, "frames": FRAMES, "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)})
    med, lo, hi = event_ms(lambda: kin.fk(skel, qdq))
    note({"what": "fk", "poses": int(qdq.shape[0]), "ms_median": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4)})

    t0 = time.perf_counter()
    o_root = ko.track_ragged(table, s_init.astype(np.float64), s_rest.astype(np.float64), c_t.astype(np.float64), valid, offs)[0]
    t1 = time.perf_counter()
    qh, gh = qdq.cpu().numpy().astype(np.float64), gt.cpu().numpy().astype(np.float64)
    o_m = np.stack([ko.evaluate(table, qh[a:b], gh[a:b]) for a, b in zip(offs[:-1], offs[1:])])
    t2 = time.perf_counter()
    d_m = kin.evaluate(skel, qdq, gt, offs)
    note({"what": "oracle", "track_host_s": round(t1 - t0, 3), "evaluate_host_s": round(t2 - t1, 3),
          "device_root_minus_oracle": float(np.abs(root.cpu().numpy() - o_root).max()),
          "device_metrics_minus_oracle": float(np.abs(d_m - o_m).max())})

    m = model()
    for n in SIZES:
        fr, s0 = frames(n, n)
        a = tip_amd.streaming.StreamingEngine(m, s0, use_graph=True)
        b = tip_amd.streaming.StreamingEngine(m, s0, use_graph=True)
        rt = kin.RootTracker(skel, n, "cuda")
        rt.reset(None, s0)
        for f in range(50):                           # past the warm-up: every window at T = 40 in both
            a.step(fr[f % len(fr)])
            rt.step(b.step(fr[f % len(fr)]))
        torch.cuda.synchronize()

        def tracked(i):
            rt.step(b.step(fr[i % len(fr)]))

        res = alternate({"engine": lambda i: a.step(fr[i % len(fr)]), "tracked": tracked})
        last = b.step(fr[0])
        med, lo, hi = event_ms(lambda: [rt.step(last) for _ in range(200)], warm=1, reps=5)
        note({"what": "live", "n": n, "engine_ms": round(res["engine"], 4), "engine_plus_tracker_ms": round(res["tracked"], 4),
              "delta_us": round((res["tracked"] - res["engine"]) * 1e3, 1), "tracker_us_per_launch": round(lo / 200 * 1e3, 2),
              "root_finite": bool(torch.isfinite(rt.root).all())})
        del a, b, rt
    m.check_handoffs()
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("# tools/kin_bench.py on one MI355X: kinematics.track / evaluate / fk on 50 files x 600 frames (device events, median of 20\n"
                     "# after 3 warm-up calls, inputs on the device), RootTracker.step beside StreamingEngine.step (graph mode, alternating blocks,\n"
                     "# best block; the launch alone: 200 back to back), and the fp64 numpy oracle's host time on the same rows\n")
            for r in recs:
                fh.write(json.dumps(r) + "\n")
    for r in recs:
        print(r, file=sys.stderr)


if __name__ == "__main__":
    main()
