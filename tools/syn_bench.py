"""What tip_amd.syndata costs (csrc/tip_syn.hip) on a corpus-sized batch: 64 sequences of 3000 frames from the fixture's motion
generator (tests/syn_oracle.motion), each at its own body scale.

    python tools/syn_bench.py [--out FILE]   -> one JSON line per measurement; FILE (default: the record, profiles/syn/syn_bench.txt)
                                                gets a header and the same lines

  poses / imu / sbp   each stage alone on inputs already on the device: device events on the stream around the one call, median of
                      10 after 3 warm-up calls (the SBP search is four launches: the frame quantities, then pelvis, feet, wrists)
  total               synthesize() itself from numpy inputs: the upload, the three stages, no read-back; events, median of 10 after 3
  sbp_per_frame       the SBP stage's ms / frames: the frame launch and the three classes' chain launches one after the other, every
                      chain of a class side by side (R x 1, R x 2 and R x 2 workgroups).  NOT one chain's cost: the launches cannot
                      be told apart by events around the one call — tools/syn_kernels.py times each kernel (profiles/syn/syn_kernels.txt)
  --once              no measurement: synthesize() three times on the same corpus and exit (what tools/syn_kernels.py traces)
  oracle              tests/syn_oracle.py, the fp64 numpy restatement, on a SUBSET it can finish — the first 300 frames of sequence 0 —
                      host wall time, per stage, scaled per frame; and the device's rows of that subset against it (flags that differ
                      are counted, not asserted: this motion is not built under the fixture's guards)
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tip_amd  # noqa: E402,F401
from tip_amd import kinematics as kin  # noqa: E402
from tip_amd import syndata as syn  # noqa: E402
import syn_oracle as so  # noqa: E402

FILES, FRAMES, SUBSET = 64, 3000, 300


def event_ms(fn, warm=3, reps=10):
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
    return {"ms_median": round(statistics.median(out), 4), "ms_min": round(min(out), 4), "ms_max": round(max(out), 4)}


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "syn", "syn_bench.txt")
    files = int(sys.argv[sys.argv.index("--files") + 1]) if "--files" in sys.argv else FILES
    frames = int(sys.argv[sys.argv.index("--frames") + 1]) if "--frames" in sys.argv else FRAMES
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "tip_syn_golden.npz"))
    skel = kin.Skeleton.from_table(golden)
    table = {k[len("table/"):]: golden[k] for k in golden.files if k.startswith("table/")}
    rng = np.random.RandomState(0)
    qs = [so.motion(frames, 100 + i) for i in range(files)]
    scales = [syn.body_scale(rng) for _ in range(files)]
    dev = torch.device("cuda", torch.cuda.current_device())
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    if "--once" in sys.argv:
        for _ in range(3):
            syn.synthesize(skel, qs, scales, dev)
        torch.cuda.synchronize()
        print("ok")
        return
    q, offsets, scale_dev, offs = syn.upload(qs, scales, dev)
    P = syn.tracked_poses(skel, q, offsets, scale_dev, dev)
    emit({"what": "poses", "files": files, "frames": frames, **event_ms(lambda: syn.tracked_poses(skel, q, offsets, scale_dev, dev))})
    emit({"what": "imu", "files": files, "frames": frames, **event_ms(lambda: syn.imu_readings(P, offsets, dev))})
    sbp = event_ms(lambda: syn.sbp_labels(skel, P, offsets, dev))
    emit({"what": "sbp", "files": files, "frames": frames, **sbp})
    emit({"what": "sbp_per_frame", "us_frame_launch_and_three_classes_in_turn": round(sbp["ms_median"] * 1e3 / frames, 3)})
    emit({"what": "total", "files": files, "frames": frames, **event_ms(lambda: syn.synthesize(skel, qs, scales, dev))})
    out = syn.synthesize(skel, qs, scales, dev)
    on = torch.cat([f["constrs"] for f in out])[:, 0::4].mean(0).cpu().numpy()
    emit({"what": "labels", "on_fraction_per_body": [round(float(v), 3) for v in on], "finite": bool(all(torch.isfinite(f["imu"]).all() for f in out))})
    # the oracle on a subset it can finish
    n = min(SUBSET, frames)
    sub = qs[0][:n]
    t0 = time.perf_counter()
    Po = so.tracked_poses(table, sub, scales[0])
    t1 = time.perf_counter()
    Io = so.imu_readings(Po)
    t2 = time.perf_counter()
    Co, _ = so.sbp_labels(Po)
    t3 = time.perf_counter()
    (d,) = syn.synthesize(skel, [sub], [scales[0]], dev)
    di, dc = d["imu"].cpu().numpy(), d["constrs"].cpu().numpy()
    same = (dc[:, 0::4] == Co[:, 0::4])
    rows = same.all(1)
    emit({"what": "oracle", "subset": f"sequence 0, frames 0 .. {n - 1}", "poses_host_ms_per_frame": round((t1 - t0) * 1e3 / n, 4),
          "imu_host_ms_per_frame": round((t2 - t1) * 1e3 / n, 4), "sbp_host_ms_per_frame": round((t3 - t2) * 1e3 / n, 4),
          "scaled_to_corpus_s": round((t3 - t0) / n * files * frames, 1), "device_imu_minus_oracle": float(np.abs(di - Io).max()),
          "flags_that_differ": int((~same).sum()), "device_offsets_minus_oracle_where_flags_agree": float(np.abs(dc[rows] - Co[rows]).max())})
    with open(out_path, "w") as f:
        f.write(f"# tools/syn_bench.py on one MI355X: tip_amd.syndata on {files} sequences x {frames} frames (device events on the stream, median of 10\n"
                "# after 3 warm-up calls; stages on inputs already on the device, total = synthesize() from numpy), and the fp64 numpy\n"
                f"# oracle's host time on the first {n} frames of sequence 0, scaled per frame\n")
        f.write("\n".join(lines) + "\nok\n")
    print("ok")


if __name__ == "__main__":
    main()
