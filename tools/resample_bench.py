"""What resampling timestamped packets costs (csrc/tip_resample.hip; tip_amd.sensors.PacketResampler, resample_sequences), in one run.

    python tools/resample_bench.py [--out FILE] [--files N] [--packets N]   -> one JSON line per measurement; FILE (default: the
                                                                              record, profiles/sensor/resample_bench.txt) gets a
                                                                              header and the same lines

  kernel   tip_resample_emit alone (slerp, every row interpolated), tip_resample_push of two arrivals per slot alone, and
           tip_sensor_transform alone, at 1, 256 and 1024 slots: device events around 2000 back-to-back launches, us per launch, best
           and median of 5
  frame    StreamingEngine.step_packets at 1, 256 and 1024 streams, a frame with the resampler — push() of the two packets per slot that
           120 Hz sensors deliver per tick (host arrays: one pinned upload), emit(t), step_packets of the emitted tensor — against a frame
           without it — step_packets of host packets [n, 42] — launch by launch and use_graph=True, the two arms alternating in blocks of
           30 frames: median, fastest and slowest of 9 blocks per arm, ms per frame
  offline  resample_sequences on 64 sequences x 10 000 packets at 100 Hz -> the 60 Hz grid (slerp, delay 0.012 s): the
           tip_resample_rows launch alone on inputs already on the device (events, median of 20 after 5), the whole call from numpy
           (uploads, launch, no read-back; events, median of 10 after 3), the numpy oracle (tests/resample_oracle.py, fp32 and fp64) on
           the first 600 packets of sequence 0, host time per output row scaled to the corpus, and the device's rows of that subset
           against the oracle's: flags, rotation matrices and accelerations against fp64, beside the oracle's own fp32 noise
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
from tip_amd import sensors  # noqa: E402
from staggered_bench import model, block  # noqa: E402
import resample_oracle as ro  # noqa: E402

SIZES = (1, 256, 1024)
BLOCKS, PER_BLOCK = 9, 30
FILES, PACKETS, RATE, DELAY, SUBSET = 64, 10000, 100.0, 0.012, 600
TICK = 1.0 / 60.0


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def walk_packets(rng, L, sensors_=6, step=0.05):
    """L packets [L, 42] fp32: per sensor a quaternion random walk (about `step` rad per packet) and accelerations N(0, 3^2)."""
    q = rng.normal(size=(1, sensors_, 4)) + np.cumsum(rng.normal(0.0, step / 2.0, size=(L, sensors_, 4)), axis=0)
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    return np.concatenate((q, rng.normal(0.0, 3.0, size=(L, sensors_, 3))), axis=-1).reshape(L, sensors_ * 7).astype(np.float32)


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


def per_launch_us(fn, launches=2000):
    for _ in range(50):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    got = []
    for _ in range(5):
        torch.cuda.synchronize()
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        got.append(a.elapsed_time(b) / launches * 1e3)
    return round(min(got), 2), round(float(np.median(got)), 2)


def alternate(arms):
    for fn in arms.values():
        block(fn, 8)
    got = {t: [] for t in arms}
    for _ in range(BLOCKS):
        for t, fn in arms.items():
            got[t].append(block(fn, PER_BLOCK))
    return got


def live_inputs(n, seed):
    """A loaded front end, a resampler (slerp, delay half a tick), and per slot the two packets a 120 Hz sensor delivers per tick:
    8 payloads [2 n, 42], the slots [2 n] and the stamps' offsets from the tick [2 n] (host arrays)."""
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(seed)
    rot = lambda k: Rotation.random(n * 6, random_state=seed + k).as_matrix().reshape(n, 54)       # noqa: E731
    tables = np.concatenate([rot(0), rng.randn(n, 18) * 0.1, rot(1)], axis=1).astype(np.float32)
    front = sensors.SensorFrontEnd(n, "cuda")
    front.load(range(n), tables)
    rs = sensors.PacketResampler(n, "cuda", mode="slerp", delay=TICK / 2, max_hold=0.1)
    walk = walk_packets(rng, 16, sensors_=6 * n).reshape(16, n, 42)
    payloads = [np.ascontiguousarray(np.concatenate((walk[2 * j], walk[2 * j + 1]))) for j in range(8)]
    slots = np.concatenate((np.arange(n), np.arange(n))).astype(np.int32)
    offs = np.concatenate((np.full(n, -TICK / 2 - 0.001), np.full(n, -0.001)))
    return front, rs, payloads, slots, offs, (rng.randn(n, 114) * 0.2).astype(np.float32)


def live_part(m, n, emit):
    front, rs, payloads, slots, offs, s_init = live_inputs(n, n)
    lib, st = rs.lib, rs._stream()
    for k in range(4):                                            # rings with eight packets: every emit below interpolates
        rs.push(payloads[k], slots, 1.0 + k * TICK + offs)
    t = torch.full((n,), 1.0 + 3 * TICK, dtype=torch.float64, device="cuda")
    out = torch.empty((n, 42), dtype=torch.float32, device="cuda")
    raw = torch.empty((n, 72), dtype=torch.float32, device="cuda")
    e = per_launch_us(lambda: lib.tip_resample_emit(rs.state.data_ptr(), n, rs.depth, t.data_ptr(), rs.delay, rs.max_hold, rs.mode,
                                                    out.data_ptr(), rs.flags.data_ptr(), st))
    interpolated = int((rs.flags == sensors.INTERPOLATED).sum())
    d_pk, d_sl = torch.tensor(payloads[0]).cuda(), torch.tensor(slots).cuda()
    d_tm = torch.tensor(offs).cuda()                              # (stamps below the rings' newest: every arrival is refused, none copied)
    p_drop = per_launch_us(lambda: lib.tip_resample_push(rs.state.data_ptr(), n, rs.depth, d_pk.data_ptr(), d_sl.data_ptr(), d_tm.data_ptr(),
                                                         2 * n, st))
    front._fill(out, "resample_bench")
    x = per_launch_us(lambda: front._transform_into(raw))
    emit({"what": "kernel", "n": n, "emit_us_per_launch": e[0], "emit_us_median": e[1], "rows_interpolated": interpolated,
          "push_2n_refused_us_per_launch": p_drop[0], "transform_us_per_launch": x[0], "transform_us_median": x[1]})
    for graph in (False, True):
        a = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=graph)
        b = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=graph)
        rs.reset()
        tick = [0]

        def with_rs(i):
            tick[0] += 1
            tk = 10.0 + tick[0] * TICK
            rs.push(payloads[i % 8], slots, tk + offs)
            a.step_packets(front, rs.emit(tk))

        def plain(i):
            b.step_packets(front, payloads[i % 8][:n])

        for f in range(50):                                       # past the warm-up: every window at T = 40 in both
            with_rs(f)
            plain(f)
        torch.cuda.synchronize()
        res = alternate({"resampled": with_rs, "plain": plain})
        med = {k: float(np.median(v)) for k, v in res.items()}
        rec = {"what": "frame", "n": n, "graph": graph, "blocks": BLOCKS, "frames_per_block": PER_BLOCK}
        for k, v in res.items():
            rec[f"{k}_ms_median"] = round(med[k], 4)
            rec[f"{k}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        rec["ratio_of_medians"] = round(med["resampled"] / med["plain"], 4)
        rec["delta_us"] = round((med["resampled"] - med["plain"]) * 1e3, 1)
        have, dropped, total = (int(c.sum()) for c in rs.counts())
        rec["packets_taken"], rec["packets_dropped"] = total, dropped
        rec["last_frame_interpolated"] = int((rs.flags == sensors.INTERPOLATED).sum())
        emit(rec)
        del a, b


def offline_part(files, packets, emit):
    rng = np.random.RandomState(0)
    pk = [walk_packets(rng, packets) for _ in range(files)]
    st = [ro.stamps_at(rng, packets, RATE, t0=1.7e9 + 10.0 * i) for i in range(files)]
    dev = torch.device("cuda", torch.cuda.current_device())
    ticks = [sensors.sequence_ticks(s, 60.0, DELAY) for s in st]
    rows = int(sum(len(t) for t in ticks))
    lib = sensors._lib.load()
    P = torch.from_numpy(np.concatenate(pk)).to(dev)
    S = torch.from_numpy(np.concatenate(st)).to(dev)
    T = torch.from_numpy(np.concatenate(ticks)).to(dev)
    in_off = torch.tensor(np.concatenate(([0], np.cumsum([len(s) for s in st]))), dtype=torch.int64, device=dev)
    out_off = torch.tensor(np.concatenate(([0], np.cumsum([len(t) for t in ticks]))), dtype=torch.int64, device=dev)
    out = torch.empty((rows, 42), dtype=torch.float32, device=dev)
    flags = torch.empty(rows, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        assert lib.tip_resample_rows(P.data_ptr(), S.data_ptr(), in_off.data_ptr(), int(P.shape[0]), T.data_ptr(), out_off.data_ptr(), rows, files,
                                     DELAY, -1.0, sensors.MODES["slerp"], 8, out.data_ptr(), flags.data_ptr(), stream) == 0
    t = event_ms(launch, 5, 20)
    moved = rows * (2 * 42 * 4 + 42 * 4 + 8 + 1)                  # two packets in, one row out, the tick, the flag
    emit({"what": "offline_launch", "files": files, "packets_per_file": packets, "rate_hz": RATE, "rows": rows, **t,
          "rows_per_s": round(rows / (t["ms_median"] * 1e-3)), "gb_per_s_on_bytes_needed": round(moved / (t["ms_median"] * 1e-3) / 1e9, 1)})
    emit({"what": "offline_total", "files": files, "packets_per_file": packets,
          **event_ms(lambda: sensors.resample_sequences(pk, st, 60.0, mode="slerp", delay=DELAY, device=dev), 3, 10)})
    got, got_flags = sensors.resample_sequences(pk, st, 60.0, mode="slerp", delay=DELAY, device=dev)
    same = torch.equal(torch.cat(got).view(torch.int32), out.view(torch.int32)) and torch.equal(torch.cat(got_flags), flags)
    n = min(SUBSET, packets)
    sub_ticks = sensors.sequence_ticks(st[0][:n], 60.0, DELAY)
    t0 = time.perf_counter()
    hi, hi_flags = ro.rows(pk[0][:n], st[0][:n], sub_ticks, DELAY, None, ro.SLERP, 8, np.float64)
    t1 = time.perf_counter()
    lo, _ = ro.rows(pk[0][:n], st[0][:n], sub_ticks, DELAY, None, ro.SLERP, 8, np.float32)
    (d,), (df,) = sensors.resample_sequences([pk[0][:n]], [st[0][:n]], 60.0, mode="slerp", delay=DELAY, device=dev, host=True)
    emit({"what": "offline_oracle", "subset": f"sequence 0, packets 0 .. {n - 1} ({len(sub_ticks)} rows)",
          "resample_sequences_equals_the_launch": bool(same), "flags_equal": bool(np.array_equal(df, hi_flags)),
          "rows_interpolated": int((hi_flags == ro.F_INTERP).sum()),
          "host_ms_per_row": round((t1 - t0) * 1e3 / max(len(sub_ticks), 1), 4),
          "scaled_to_corpus_s": round((t1 - t0) / max(len(sub_ticks), 1) * rows, 1),
          "oracle_over_launch": round((t1 - t0) / max(len(sub_ticks), 1) * rows / (t["ms_median"] * 1e-3)),
          "device_minus_fp64_rotation": float(np.abs(ro.rotations(d) - ro.rotations(hi)).max()),
          "fp32_noise_rotation": float(np.abs(ro.rotations(lo) - ro.rotations(hi)).max()),
          "device_minus_fp64_acceleration": float(np.abs(ro.accelerations(d) - ro.accelerations(hi)).max()),
          "fp32_noise_acceleration": float(np.abs(ro.accelerations(lo) - ro.accelerations(hi)).max())})


def main():
    torch.backends.cudnn.benchmark = False
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sensor", "resample_bench.txt")
    if not torch.cuda.is_available():
        raise SystemExit("tools/resample_bench.py measures on an MI355X: no GPU here")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    offline_part(arg("--files", FILES), arg("--packets", PACKETS), emit)
    torch.cuda.empty_cache()
    m = model()
    for n in SIZES:
        live_part(m, n, emit)
    m.check_handoffs()
    with open(out_path, "w") as f:
        f.write("# tools/resample_bench.py on one MI355X, one run.\n"
                "# offline: resample_sequences, 100 Hz packets with epoch-sized stamps -> the 60 Hz grid, slerp, delay 0.012 s: the tip_resample_rows\n"
                "#          launch alone (device events, median of 20 after 5), the whole call from numpy (median of 10 after 3), the numpy oracle on the\n"
                "#          first packets of sequence 0 scaled per output row, and the device's rows of that subset against the fp64 oracle beside the\n"
                "#          oracle's own fp32 noise\n"
                "# kernel:  tip_resample_emit (every row interpolated), tip_resample_push of 2 n refused arrivals and tip_sensor_transform, each alone,\n"
                "#          2000 back-to-back launches, us per launch (best; median of 5)\n"
                "# frame:   StreamingEngine.step_packets behind push (2 packets per slot, host arrays) + emit against step_packets of host packets, the\n"
                "#          arms alternating in blocks of 30 frames: median, fastest and slowest of 9 blocks, ms per frame\n")
        f.write("\n".join(lines) + "\nok\n")
    print("ok")


if __name__ == "__main__":
    main()
