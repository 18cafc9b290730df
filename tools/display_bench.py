"""What display-time poses cost and how good their prediction is (csrc/tip_display.hip; tip_amd.display.PoseResampler, resample_poses),
beside the packet side's emit and RootTracker.step in the same run.

    python tools/display_bench.py [--out FILE] [--files N] [--rows N]   -> one JSON line per measurement; FILE (default: the record,
                                                                          profiles/display/display_bench.txt) gets a header and the same lines

  kernel   at 1, 256 and 1024 slots: tip_pose_push (every push accepted: each launch reads its own row of rising stamps), tip_pose_emit
           with every row predicted 6.7 frames past the newest pose, every row interpolated, and every row held; beside them, in the same
           run, tip_predict_emit of the packet side (every row predicted) and RootTracker.step (one tip_kin_track launch
           over all slots).  Device events around 1000 back-to-back launches, us per launch, all five runs of each
  frame    StreamingEngine.step + RootTracker.step at 1, 256 and 1024 streams with push(pose_time(tick)) + emit(tick + 4 ms) behind them,
           against the same loop without, the two arms alternating in blocks of 30 frames: median, fastest and slowest of 9 blocks per
           arm, ms per frame
  offline  64 tracks x 10 000 rows at 60 Hz to 90 Hz (mode "predict", delay 0): resample_poses as a whole call from numpy (median of 10
           after 3), and the numpy oracle (tests/display_oracle.py, fp64) on the first 600 rows of track 0, host time per row scaled to the
           corpus; the device's rows of that subset against the oracle's
  quality  how far a held and a predicted pose are from the track's own later row, at horizons of 1 .. 9 frames: hold, and predict at
           baseline 1 .. 4, on a smooth synthetic track (tests/display_oracle.smooth_track, 2400 rows) and on the pose rows of the two
           traces of tests/golden/tip_runner_golden.npz (rows 5 .. 69 of qdq: a synthetic-weight model on random IMU frames — jittery,
           the adverse case).  The rule's own arithmetic in fp64 (the oracle, vectorised): this table is about the rule, not the kernel.
           Rotation error: the angle between predicted and true joint rotation, mean and 95th percentile over rows and joints, degrees;
           root error: mean distance, millimetres.  No pass / fail: it exists so that the defaults of baseline and max_predict can be
           revisited with evidence
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tip_amd  # noqa: E402
from tip_amd import display, sensors  # noqa: E402
from tip_amd import kinematics as kin  # noqa: E402
from staggered_bench import frames, model  # noqa: E402
from resample_bench import alternate, arg, event_ms, walk_packets, BLOCKS, PER_BLOCK, TICK  # noqa: E402
from sync_bench import runs_us, LAUNCHES, SIZES  # noqa: E402
import display_oracle as do  # noqa: E402

FILES, ROWS, SUBSET = 64, 10000, 600
LEAD = 6.7 * TICK                         # the derived lag: 5 + 1.2 + 0.5 frames
GOLDEN = os.path.join(ROOT, "tests", "golden")


def skeleton():
    return kin.Skeleton.from_table(np.load(os.path.join(GOLDEN, "tip_kin_golden.npz")))


def kernel_part(n, skel, emit):
    lib = display._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(n)
    ps = display.PoseResampler(n, "cuda", max_hold=0.1)
    root = torch.from_numpy(rng.normal(size=(n, 3)).astype(np.float32)).cuda()
    s_rest = torch.from_numpy((0.3 * rng.normal(size=(n, 111))).astype(np.float32)).cuda()
    d_t = torch.from_numpy(1.0 + np.arange(LAUNCHES + 60, dtype=np.float64)[:, None] * TICK + np.zeros((1, n))).cuda()   # row i: launch i's stamps
    S, D = ps.state.data_ptr(), ps.depth
    q = torch.empty((n, 57), dtype=torch.float32, device="cuda")

    def do_push(i):
        lib.tip_pose_push(S, n, D, None, 0, root.data_ptr(), s_rest.data_ptr(), 111, None, d_t.data_ptr() + 8 * n * i, st)

    rec = {"what": "kernel", "n": n, "launches": LAUNCHES}
    rec["pose_push_us"] = runs_us(do_push, ps.reset)
    rec["poses_taken_in_last_run"] = int(ps.counts()[2].sum())
    # the rings now hold eight poses a frame apart that differ (a still pose would take the small-angle branches): push a moving tail
    ps.reset()
    for k in range(8):
        ps.push(root + 0.01 * k, s_rest + 0.02 * k * torch.sign(s_rest), 1.0 + k * TICK)
    newest = 1.0 + 7 * TICK
    for name, t_q, mode, flag in (("predicted", newest + LEAD, 2, display.PREDICTED), ("interpolated", newest - 0.4 * TICK, 2, display.INTERPOLATED),
                                  ("held", newest + 2 * TICK, 0, display.HELD)):
        t = torch.full((n,), t_q, dtype=torch.float64, device="cuda")
        rec[f"pose_emit_{name}_us"] = runs_us(lambda i: lib.tip_pose_emit(S, n, D, t.data_ptr(), 0.0, 0.1, 9 * TICK, 1, mode, q.data_ptr(),
                                                                           ps.quat.data_ptr(), ps.flags.data_ptr(), st), lambda: None)
        rec[f"rows_{name}"] = int((ps.flags == flag).sum())
    # the packet side's emit, every row predicted, in the same run
    rs = sensors.PacketResampler(n, "cuda", mode="predict", max_hold=0.1)
    walk = walk_packets(rng, 4, sensors_=6 * n).reshape(4, n, 42)
    for k in range(4):
        rs.push(walk[k], np.arange(n), np.full(n, 1.0 + k * TICK))
    t = torch.full((n,), 1.0 + 3.3 * TICK, dtype=torch.float64, device="cuda")
    out = torch.empty((n, 42), dtype=torch.float32, device="cuda")
    rec["packet_emit_predict_us"] = runs_us(lambda i: lib.tip_predict_emit(rs.state.data_ptr(), n, rs.depth, t.data_ptr(), 0.0, 0.1, 0.025,
                                                                            out.data_ptr(), rs.flags.data_ptr(), st), lambda: None)
    rec["packet_rows_predicted"] = int((rs.flags == sensors.PREDICTED).sum())
    # the tracker's per-frame launch
    rt = kin.RootTracker(skel, n, "cuda")
    rt.reset(None, (0.2 * rng.normal(size=(n, 114))).astype(np.float32))
    c_t = torch.from_numpy(rng.uniform(0.0, 1.0, size=(n, 20)).astype(np.float32)).cuda()
    frame = {"s_rest": s_rest, "c_t": c_t}
    rec["root_tracker_step_us"] = runs_us(lambda i: rt.step(frame), lambda: None)
    med = {k: float(np.median(v)) for k, v in rec.items() if k.endswith("_us")}
    rec["pose_emit_predicted_over_packet_emit_median"] = round(med["pose_emit_predicted_us"] / med["packet_emit_predict_us"], 3)
    rec["pose_push_plus_emit_over_tracker_step_median"] = round((med["pose_push_us"] + med["pose_emit_predicted_us"]) / med["root_tracker_step_us"], 3)
    emit(rec)


def frame_part(m, n, skel, emit):
    fr, s_init = frames(n, n)
    a = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=False)
    b = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=False)
    ta, tb = kin.RootTracker(skel, n, "cuda"), kin.RootTracker(skel, n, "cuda")
    ta.reset(None, s_init)
    tb.reset(None, s_init)
    ps = display.PoseResampler(n, "cuda", max_hold=0.1)
    q = torch.empty((n, 57), dtype=torch.float32, device="cuda")
    tick = [0]

    def beside(i):
        tick[0] += 1
        tk = 10.0 + tick[0] * TICK
        out = a.step(fr[i % 8])
        root, _ = ta.step(out)
        if out is not None:
            ps.push(root, out["s_rest"], display.pose_time(tk), valid=out.get("valid"))
        ps.emit(tk + 0.004, out=q)

    def without(i):
        tb.step(b.step(fr[i % 8]))

    for f in range(50):                                           # past the warm-up: every window at T = 40 in both
        beside(f)
        without(f)
    torch.cuda.synchronize()
    res = alternate({"with_push_emit": beside, "without": without})
    med = {k: float(np.median(v)) for k, v in res.items()}
    rec = {"what": "frame", "n": n, "blocks": BLOCKS, "frames_per_block": PER_BLOCK}
    for k, v in res.items():
        rec[f"{k}_ms_median"] = round(med[k], 4)
        rec[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    rec["ratio_of_medians"] = round(med["with_push_emit"] / med["without"], 4)
    rec["delta_us"] = round((med["with_push_emit"] - med["without"]) * 1e3, 1)
    rec["last_frame_predicted"] = int((ps.flags == display.PREDICTED).sum())
    emit(rec)


def offline_part(files, rows, emit):
    rng = np.random.RandomState(0)
    tracks = [do.smooth_track(rng, rows, width=54) for _ in range(files)]
    rt, sr = [t[0] for t in tracks], [t[1] for t in tracks]
    st = [1.7e9 + 10.0 * i + t[2] for i, t in enumerate(tracks)]
    dev = torch.device("cuda", torch.cuda.current_device())
    kw = dict(rate_hz=90.0, mode="predict", max_hold=0.1, device=dev)
    out_rows = int(sum(len(sensors.sequence_ticks(s, 90.0, 0.0)) for s in st))
    emit({"what": "offline_resample_poses_total", "files": files, "rows_per_file": rows, "rows_out": out_rows,
          **event_ms(lambda: display.resample_poses(rt, sr, st, **kw), 3, 10)})
    n = min(SUBSET, rows)
    ticks = sensors.sequence_ticks(st[0][:n], 90.0, 0.0)
    t0 = time.perf_counter()
    hi = do.rows(st[0][:n], rt[0][:n], sr[0][:n], ticks, 0.0, 0.1, display.MAX_PREDICT, 1, do.PREDICT, 8, np.float64)
    t1 = time.perf_counter()
    lo = do.rows(st[0][:n], rt[0][:n], sr[0][:n], ticks, 0.0, 0.1, display.MAX_PREDICT, 1, do.PREDICT, 8, np.float32)
    (d,), (df,) = display.resample_poses([rt[0][:n]], [sr[0][:n]], [st[0][:n]], host=True, **kw)
    p = hi[2] == do.F_PREDICT
    emit({"what": "offline_oracle", "subset": f"track 0, rows 0 .. {n - 1} ({len(ticks)} output rows)", "flags_equal": bool(np.array_equal(df, hi[2])),
          "rows_predicted": int(p.sum()), "oracle_ms_per_row": round((t1 - t0) * 1e3 / max(len(ticks), 1), 4),
          "oracle_scaled_to_corpus_s": round((t1 - t0) / max(len(ticks), 1) * out_rows, 1),
          "device_minus_fp64_rotation": float(np.abs(do.rotations(d[p]) - do.rotations(hi[0][p])).max()),
          "fp32_noise_rotation": float(np.abs(do.rotations(lo[0][p]) - do.rotations(hi[0][p])).max()),
          "device_minus_fp64_root": float(np.abs(d[p][:, :3] - hi[0][p][:, :3]).max()),
          "fp32_noise_root": float(np.abs(lo[0][p][:, :3] - hi[0][p][:, :3]).max())})


def quality_part(emit):
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(3)
    rt, sr, _ = do.smooth_track(rng, 2400)
    tracks = {"smooth_synthetic": [(rt.astype(np.float64), sr[:, :54].astype(np.float64))]}
    z = np.load(os.path.join(GOLDEN, "tip_runner_golden.npz"))
    tracks["runner_golden_traces"] = [(z[f"stream{j}/qdq"][5:, :3], z[f"stream{j}/qdq"][5:, 3:57]) for j in (0, 1)]

    def errors(p_root, p_aa, t_root, t_aa):
        ang = (Rotation.from_rotvec(p_aa.reshape(-1, 3)).inv() * Rotation.from_rotvec(t_aa.reshape(-1, 3))).magnitude()
        return np.degrees(ang), 1e3 * np.linalg.norm(p_root - t_root, axis=1)

    for name, parts in tracks.items():
        for k in range(1, 10):
            rec = {"what": "quality", "track": name, "rows": int(sum(len(p[0]) for p in parts)), "horizon_frames": k}
            for arm in ("hold", 1, 2, 3, 4):
                angs, dists = [], []
                for root, aa in parts:
                    i = np.arange(4, len(root) - k)                # (rows with four entries behind them and the target ahead)
                    if arm == "hold":
                        a, d = errors(root[i], aa[i], root[i + k], aa[i + k])
                    else:
                        u = (arm + k) / arm
                        p_aa, _ = do.between(aa[i - arm].reshape(-1, 18, 3), aa[i].reshape(-1, 18, 3), u, np.float64, past=True, stored=np.float64)
                        a, d = errors(do.root(root[i - arm], root[i], u, np.float64, stored=np.float64), p_aa, root[i + k], aa[i + k])
                    angs.append(a)
                    dists.append(d)
                a, d = np.concatenate(angs), np.concatenate(dists)
                tag = "hold" if arm == "hold" else f"predict_b{arm}"
                rec[f"{tag}_rot_deg_mean_p95"] = [round(float(np.nanmean(a)), 3), round(float(np.nanpercentile(a, 95)), 3)]
                rec[f"{tag}_root_mm_mean"] = round(float(np.nanmean(d)), 2)
            emit(rec)


def main():
    torch.backends.cudnn.benchmark = False
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "display", "display_bench.txt")
    if not torch.cuda.is_available():
        raise SystemExit("tools/display_bench.py measures on an MI355X: no GPU here")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    skel = skeleton()
    for n in SIZES:
        kernel_part(n, skel, emit)
    offline_part(arg("--files", FILES), arg("--rows", ROWS), emit)
    quality_part(emit)
    torch.cuda.empty_cache()
    m = model()
    for n in SIZES:
        frame_part(m, n, skel, emit)
    m.check_handoffs()
    with open(out_path, "w") as f:
        f.write("# tools/display_bench.py on one MI355X, one run.\n"
                "# kernel:  tip_pose_push (every push accepted), tip_pose_emit (all predicted 6.7 frames out / all interpolated / all held), and in the\n"
                "#          same run the packet side's tip_predict_emit (all predicted) and the tracker's per-frame launch: 1000 back-to-back\n"
                "#          launches, us per launch, all five runs of each\n"
                "# offline: 64 tracks x 10 000 rows at 60 Hz to 90 Hz: resample_poses from numpy (median of 10 after 3), the numpy oracle on the first\n"
                "#          rows of track 0 scaled to the corpus, the device's rows of that subset against the oracle's\n"
                "# quality: error of a held pose and of a predicted one (baseline 1 .. 4) against the track's own row k frames later, k = 1 .. 9: joint\n"
                "#          rotation angle (mean, 95th percentile; degrees) and root distance (mean; mm); the rule's arithmetic in fp64\n"
                "# frame:   StreamingEngine.step + RootTracker.step with push + emit behind them against the same loop without, the arms alternating in\n"
                "#          blocks of 30 frames: median, fastest and slowest of 9 blocks, ms per frame\n")
        f.write("\n".join(lines) + "\nok\n")
    print("ok")


if __name__ == "__main__":
    main()
