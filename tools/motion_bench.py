"""What tip_amd.motion costs (csrc/tip_motion.hip) on a corpus-sized batch: 64 source sequences of 6000 frames at 120 fps (AMASS
layout: 156 columns and a root path) from the fixture's motion generator (tests/motion_oracle.source_motion) -> 64 x 3000 rows of
nimble_qdq.

    python tools/motion_bench.py [--out FILE]   -> one JSON line per measurement; FILE (default: the record,
                                                   profiles/motion/motion_bench.txt) gets a header and the same lines

  launch    tip_motion_qdq alone on inputs already on the device: device events on the stream around the one call, median of 20
            after 5 warm-up calls; with it the bytes the launch has to move (the two source rows per (row, slot) counted once per row,
            the 114 output columns) over that time, and the rows per second
  total     qdq_from_smpl() itself from numpy inputs: the uploads, the launch, no read-back; events, median of 10 after 3
  oracle    tests/motion_oracle.py, the fp64 numpy / scipy restatement, on a SUBSET it can finish — the first 600 source frames of
            sequence 0 — host wall time per output row, scaled to the corpus; and the device's rows of that subset minus the oracle's
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
from tip_amd import motion  # noqa: E402
import motion_oracle as mo  # noqa: E402

FILES, FRAMES, FPS, SUBSET = 64, 6000, 120.0, 600


def event_ms(fn, warm, reps):
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
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "motion", "motion_bench.txt")
    files = int(sys.argv[sys.argv.index("--files") + 1]) if "--files" in sys.argv else FILES
    frames = int(sys.argv[sys.argv.index("--frames") + 1]) if "--frames" in sys.argv else FRAMES
    if not torch.cuda.is_available():
        raise SystemExit("tools/motion_bench.py measures on an MI355X: no GPU here")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    src = [mo.source_motion(frames, 200 + i, 156, amp=0.4) for i in range(files)]
    poses, trans = [s[0] for s in src], [s[1] for s in src]
    rows = motion.output_rows(frames, FPS)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    # the launch alone: the stacked arrays, offsets and tables on the device once
    _, lib = kin._lib()
    P = torch.from_numpy(np.concatenate(poses)).to(dev)
    T = torch.from_numpy(np.concatenate(trans)).to(dev)
    in_off = torch.arange(files + 1, dtype=torch.int64, device=dev) * frames
    out_off = torch.arange(files + 1, dtype=torch.int64, device=dev) * rows
    fps = torch.full((files,), FPS, dtype=torch.float64, device=dev)
    times = torch.from_numpy(motion.time_table(rows)).to(dev)
    joints = torch.from_numpy(motion.joint_table(None)).to(dev)
    out = torch.empty((files * rows, 114), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        kin._check(lib.tip_motion_qdq(P.data_ptr(), 156, T.data_ptr(), None, in_off.data_ptr(), out_off.data_ptr(), fps.data_ptr(), files,
                                      files * frames, files * rows, times.data_ptr(), rows, joints.data_ptr(), out.data_ptr(), stream))

    t = event_ms(launch, 5, 20)
    n_rows = files * rows
    moved = n_rows * (2 * (66 + 3) + 114) * 8                             # two source rows (66 pose columns + trans) in, 114 columns out
    emit({"what": "launch", "files": files, "source_frames": frames, "fps": FPS, "rows": n_rows, **t,
          "rows_per_s": round(n_rows / (t["ms_median"] * 1e-3)), "gb_per_s_on_bytes_needed": round(moved / (t["ms_median"] * 1e-3) / 1e9, 1)})
    emit({"what": "total", "files": files, "source_frames": frames,
          **event_ms(lambda: motion.qdq_from_smpl(poses, FPS, trans, device=dev), 3, 10)})
    got = motion.qdq_from_smpl(poses, FPS, trans, device=dev)
    same = all(torch.equal(g, out[i * rows:(i + 1) * rows]) for i, g in enumerate(got))
    emit({"what": "check", "qdq_from_smpl_equals_the_launch": bool(same), "finite": bool(torch.isfinite(out).all())})
    # the oracle on a subset it can finish
    n = min(SUBSET, frames)
    t0 = time.perf_counter()
    ref = mo.qdq_from_smpl(poses[0][:n], FPS, trans[0][:n])
    t1 = time.perf_counter()
    (d,) = motion.qdq_from_smpl([poses[0][:n]], FPS, [trans[0][:n]], device=dev)
    emit({"what": "oracle", "subset": f"sequence 0, source frames 0 .. {n - 1} ({ref.shape[0]} rows)",
          "host_ms_per_row": round((t1 - t0) * 1e3 / ref.shape[0], 4), "scaled_to_corpus_s": round((t1 - t0) / ref.shape[0] * n_rows, 1),
          "device_minus_oracle": float(np.abs(d.cpu().numpy() - ref).max())})
    with open(out_path, "w") as f:
        f.write(f"# tools/motion_bench.py on one MI355X: tip_amd.motion on {files} sequences x {frames} source frames at {FPS:g} fps -> {n_rows} rows\n"
                "# (device events on the stream; launch = tip_motion_qdq on inputs already on the device, median of 20 after 5 warm-up calls;\n"
                "# total = qdq_from_smpl() from numpy, median of 10 after 3), and the fp64 numpy oracle's host time on the first\n"
                f"# {n} source frames of sequence 0, scaled per row\n")
        f.write("\n".join(lines) + "\nok\n")
    print("ok")


if __name__ == "__main__":
    main()
