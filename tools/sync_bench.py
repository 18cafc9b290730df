"""What clock sync and predicted ticks cost (csrc/tip_clock.hip; tip_amd.sensors.ClockSync, PacketResampler(mode="predict"),
sync_sequences), beside the resampler entries they stand next to, in one run.

    python tools/sync_bench.py [--out FILE] [--files N] [--packets N]   -> one JSON line per measurement; FILE (default: the record,
                                                                          profiles/sensor/sync_bench.txt) gets a header and the same lines

  kernel   at 1, 256 and 1024 slots, two arrivals per slot per launch (what 120 Hz sensors deliver per tick), every arrival ACCEPTED (each
           launch reads its own row of rising stamps): tip_clock_map, tip_resample_push, the two back to back, and tip_clock_push (the
           fused launch); tip_resample_emit (slerp, every row interpolated) and tip_predict_emit (every row predicted).  Device events
           around 1000 back-to-back launches, us per launch, all five runs of each
  frame    StreamingEngine.step_packets at 1, 256 and 1024 streams behind push(arrivals=, sync=) + emit in mode "predict" with delay 0,
           against the same engine behind push + emit in mode "slerp" with half a tick of delay (the resampler as it was), host arrays in
           both, the two arms alternating in blocks of 30 frames: median, fastest and slowest of 9 blocks per arm, ms per frame
  offline  64 sessions x 10 000 packets at 100 Hz with epoch-sized offsets: the tip_clock_rows launch alone on inputs already on the
           device (events, median of 20 after 5), sync_sequences and resample_sequences(mode="predict") as whole calls from numpy
           (median of 10 after 3), and the numpy oracle (tests/sync_oracle.py, fp64) on the first 600 packets of session 0, host time per
           row scaled to the corpus; the device's rows of that subset against the oracle's
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
from tip_amd import sensors  # noqa: E402
from staggered_bench import model  # noqa: E402
from resample_bench import alternate, arg, event_ms, live_inputs, walk_packets, BLOCKS, PER_BLOCK, TICK  # noqa: E402
import resample_oracle as ro  # noqa: E402
import sync_oracle as sy  # noqa: E402

SIZES = (1, 256, 1024)
LAUNCHES, WARM, RUNS = 1000, 50, 5
FILES, PACKETS, SUBSET = 64, 10000, 600
OFFSET = 1.7e9


def runs_us(launch, before_run):
    """`launch(i)` LAUNCHES times back to back, RUNS times, `before_run()` (untimed) in front of each -> us per launch, every run."""
    before_run()
    for i in range(WARM):
        launch(i)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    got = []
    for _ in range(RUNS):
        before_run()
        torch.cuda.synchronize()
        a.record()
        for i in range(LAUNCHES):
            launch(i)
        b.record()
        torch.cuda.synchronize()
        got.append(round(a.elapsed_time(b) / LAUNCHES * 1e3, 2))
    return got


def kernel_part(n, emit):
    lib = sensors._lib.load()
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.RandomState(n)
    rs = sensors.PacketResampler(n, "cuda", mode="slerp", delay=TICK / 2, max_hold=0.1)
    clk = sensors.ClockSync(n, "cuda")
    m = 2 * n
    # row i: the stamps of launch i, two per slot, rising from row to row; arrivals = stamps + offset + delay
    rows = (np.arange(LAUNCHES, dtype=np.float64)[:, None] * TICK + np.concatenate((np.full(n, 0.25 * TICK), np.full(n, 0.75 * TICK)))[None, :])
    d_st = torch.from_numpy(1.0 + rows).cuda()
    d_ar = torch.from_numpy(1.0 + rows + OFFSET + 0.002 + rng.exponential(0.003, size=rows.shape)).cuda()
    d_tm = torch.empty(m, dtype=torch.float64, device="cuda")
    d_pk = torch.from_numpy(walk_packets(rng, 2, sensors_=6 * n).reshape(m, 42)).cuda()
    d_sl = torch.from_numpy(np.concatenate((np.arange(n), np.arange(n))).astype(np.int32)).cuda()
    S, C, D = rs.state.data_ptr(), clk.state.data_ptr(), rs.depth
    row = lambda t, i: t.data_ptr() + 8 * m * i                   # noqa: E731

    def fresh():
        rs.reset()
        clk.reset()

    def do_map(i):
        lib.tip_clock_map(C, n, d_sl.data_ptr(), row(d_st, i), row(d_ar, i), m, clk.leak, clk.slew, d_tm.data_ptr(), st)

    def do_push(i):                                               # (the stamps as times: rising, so every packet goes in)
        lib.tip_resample_push(S, n, D, d_pk.data_ptr(), d_sl.data_ptr(), row(d_st, i), m, st)

    def do_both(i):
        lib.tip_clock_map(C, n, d_sl.data_ptr(), row(d_st, i), row(d_ar, i), m, clk.leak, clk.slew, d_tm.data_ptr(), st)
        lib.tip_resample_push(S, n, D, d_pk.data_ptr(), d_sl.data_ptr(), d_tm.data_ptr(), m, st)

    def do_fused(i):
        lib.tip_clock_push(S, C, n, D, d_pk.data_ptr(), d_sl.data_ptr(), row(d_st, i), row(d_ar, i), m, clk.leak, clk.slew, None, st)

    rec = {"what": "kernel", "n": n, "arrivals_per_launch": m, "launches": LAUNCHES}
    for name, fn in (("map", do_map), ("push", do_push), ("map_then_push", do_both), ("push_synced", do_fused)):
        rec[f"{name}_us"] = runs_us(fn, fresh)
    taken = int(rs.counts()[2].sum())
    rec["packets_taken_in_last_run"], rec["rejected"] = taken, int(clk.counts()[1].sum())
    # the rings now hold rising stamps up to row LAUNCHES - 1: a query inside them interpolates, one a quarter tick past them predicts
    out = torch.empty((n, 42), dtype=torch.float32, device="cuda")
    flags = torch.empty(n, dtype=torch.uint8, device="cuda")
    newest = 1.0 + (LAUNCHES - 1) * TICK + 0.75 * TICK + OFFSET + 0.002
    t_in = torch.full((n,), newest - 0.3 * TICK, dtype=torch.float64, device="cuda")
    t_past = torch.full((n,), newest + 0.3 * TICK, dtype=torch.float64, device="cuda")
    rec["emit_slerp_us"] = runs_us(lambda i: lib.tip_resample_emit(S, n, D, t_in.data_ptr(), 0.0, 0.1, 1, out.data_ptr(), flags.data_ptr(), st),
                                   lambda: None)
    rec["rows_interpolated"] = int((flags == sensors.INTERPOLATED).sum())
    rec["emit_predict_us"] = runs_us(lambda i: lib.tip_predict_emit(S, n, D, t_past.data_ptr(), 0.0, 0.1, 0.025, out.data_ptr(), flags.data_ptr(), st),
                                     lambda: None)
    rec["rows_predicted"] = int((flags == sensors.PREDICTED).sum())
    rec["fused_over_two_launches_best"] = round(min(rec["push_synced_us"]) / min(rec["map_then_push_us"]), 3)
    rec["predict_over_slerp_median"] = round(float(np.median(rec["emit_predict_us"]) / np.median(rec["emit_slerp_us"])), 3)
    emit(rec)


def frame_part(m, n, emit):
    front, rs_old, payloads, slots, offs, s_init = live_inputs(n, n)
    rs_new = sensors.PacketResampler(n, "cuda", mode="predict", delay=0.0, max_hold=0.1)
    clk = sensors.ClockSync(n, "cuda")
    a = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=False)
    b = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=False)
    tick = [0, 0]

    def synced(i):
        tick[0] += 1
        tk = 10.0 + tick[0] * TICK
        rs_new.push(payloads[i % 8], slots, tk + offs - OFFSET, arrivals=tk + offs + 0.002, sync=clk)      # stamps on the hub's clock
        a.step_packets(front, rs_new.emit(tk + 0.004))

    def before(i):
        tick[1] += 1
        tk = 10.0 + tick[1] * TICK
        rs_old.push(payloads[i % 8], slots, tk + offs)
        b.step_packets(front, rs_old.emit(tk))

    for f in range(50):                                           # past the warm-up: every window at T = 40 in both
        synced(f)
        before(f)
    torch.cuda.synchronize()
    res = alternate({"synced_predict": synced, "push_slerp": before})
    med = {k: float(np.median(v)) for k, v in res.items()}
    rec = {"what": "frame", "n": n, "blocks": BLOCKS, "frames_per_block": PER_BLOCK}
    for k, v in res.items():
        rec[f"{k}_ms_median"] = round(med[k], 4)
        rec[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    rec["ratio_of_medians"] = round(med["synced_predict"] / med["push_slerp"], 4)
    rec["delta_us"] = round((med["synced_predict"] - med["push_slerp"]) * 1e3, 1)
    rec["last_frame_predicted"] = int((rs_new.flags == sensors.PREDICTED).sum())
    rec["last_frame_interpolated_before"] = int((rs_old.flags == sensors.INTERPOLATED).sum())
    rec["rejected"] = int(clk.counts()[1].sum())
    emit(rec)


def offline_part(files, packets, emit):
    rng = np.random.RandomState(0)
    pk = [walk_packets(rng, packets) for _ in range(files)]
    hubs = [sy.hub(rng, packets, offset=OFFSET + 10.0 * i, drift=rng.uniform(-50e-6, 50e-6)) for i in range(files)]
    st, ar = [h[0] for h in hubs], [h[1] for h in hubs]
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = sensors._lib.load()
    S, A = torch.from_numpy(np.concatenate(st)).to(dev), torch.from_numpy(np.concatenate(ar)).to(dev)
    off = torch.tensor(np.concatenate(([0], np.cumsum([len(s) for s in st]))), dtype=torch.int64, device=dev)
    out = torch.empty_like(S)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        assert lib.tip_clock_rows(S.data_ptr(), A.data_ptr(), off.data_ptr(), int(S.shape[0]), files, sy.LEAK, sy.SLEW, out.data_ptr(), stream) == 0
    t = event_ms(launch, 5, 20)
    emit({"what": "offline_clock_launch", "files": files, "packets_per_file": packets, **t,
          "us_per_step_of_the_longest_sequence": round(t["ms_median"] * 1e3 / packets, 4)})
    emit({"what": "offline_sync_sequences_total", **event_ms(lambda: sensors.sync_sequences(st, ar, device=dev), 3, 10)})
    times = sensors.sync_sequences(st, ar, device=dev)
    same = np.array_equal(np.concatenate(times).view(np.int64), out.cpu().numpy().view(np.int64))
    emit({"what": "offline_predict_total", "rows": int(sum(len(sensors.sequence_ticks(t_, 60.0, 0.0)) for t_ in times)),
          **event_ms(lambda: sensors.resample_sequences(pk, times, 60.0, mode="predict", max_hold=0.1, device=dev), 3, 10)})
    n = min(SUBSET, packets)
    t0 = time.perf_counter()
    want, _ = sy.clock_sequence(st[0][:n], ar[0][:n])
    t1 = time.perf_counter()
    ticks = sensors.sequence_ticks(want, 60.0, 0.0)
    hi, hi_flags = sy.rows(pk[0][:n], want, ticks, 0.0, 0.1, 0.025, 8, np.float64)
    t2 = time.perf_counter()
    lo, _ = sy.rows(pk[0][:n], want, ticks, 0.0, 0.1, 0.025, 8, np.float32)
    (d,), (df,) = sensors.resample_sequences([pk[0][:n]], [times[0][:n]], 60.0, mode="predict", max_hold=0.1, device=dev, host=True)
    p = hi_flags == sy.F_PREDICT
    rows = int(sum(len(sensors.sequence_ticks(t_, 60.0, 0.0)) for t_ in times))
    emit({"what": "offline_oracle", "subset": f"session 0, packets 0 .. {n - 1} ({len(ticks)} rows)",
          "sync_sequences_equals_the_launch": bool(same), "mapped_times_equal_the_oracle": bool(np.array_equal(times[0][:n].view(np.int64), want.view(np.int64))),
          "flags_equal": bool(np.array_equal(df, hi_flags)), "rows_predicted": int(p.sum()),
          "oracle_clock_us_per_packet": round((t1 - t0) * 1e6 / n, 2), "oracle_clock_scaled_to_corpus_s": round((t1 - t0) / n * files * packets, 2),
          "oracle_rows_ms_per_row": round((t2 - t1) * 1e3 / max(len(ticks), 1), 4), "oracle_rows_scaled_to_corpus_s": round((t2 - t1) / max(len(ticks), 1) * rows, 1),
          "device_minus_fp64_rotation": float(np.abs(ro.rotations(d[p]) - ro.rotations(hi[p])).max()),
          "fp32_noise_rotation": float(np.abs(ro.rotations(lo[p]) - ro.rotations(hi[p])).max()),
          "device_minus_fp64_acceleration": float(np.abs(ro.accelerations(d[p]) - ro.accelerations(hi[p])).max()),
          "fp32_noise_acceleration": float(np.abs(ro.accelerations(lo[p]) - ro.accelerations(hi[p])).max())})


def main():
    torch.backends.cudnn.benchmark = False
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sensor", "sync_bench.txt")
    if not torch.cuda.is_available():
        raise SystemExit("tools/sync_bench.py measures on an MI355X: no GPU here")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    for n in SIZES:
        kernel_part(n, emit)
    offline_part(arg("--files", FILES), arg("--packets", PACKETS), emit)
    torch.cuda.empty_cache()
    m = model()
    for n in SIZES:
        frame_part(m, n, emit)
    m.check_handoffs()
    with open(out_path, "w") as f:
        f.write("# tools/sync_bench.py on one MI355X, one run.\n"
                "# kernel:  two accepted arrivals per slot per launch; tip_clock_map, tip_resample_push, the two back to back, tip_clock_push (fused);\n"
                "#          tip_resample_emit (slerp, all interpolated) and tip_predict_emit (all predicted): 1000 back-to-back launches, us per launch,\n"
                "#          all five runs of each\n"
                "# offline: 64 sessions x 10 000 packets: the tip_clock_rows launch alone (median of 20 after 5), sync_sequences and\n"
                "#          resample_sequences(mode=predict) from numpy (median of 10 after 3), the numpy oracle on the first packets of session 0 scaled\n"
                "# frame:   step_packets behind push(arrivals=, sync=) + emit(predict, delay 0) against push + emit(slerp, half a tick of delay), the arms\n"
                "#          alternating in blocks of 30 frames: median, fastest and slowest of 9 blocks, ms per frame\n")
        f.write("\n".join(lines) + "\nok\n")
    print("ok")


if __name__ == "__main__":
    main()
