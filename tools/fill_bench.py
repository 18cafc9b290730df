"""What filling missing IMU readings costs (csrc/tip_fill.hip; tip_amd.sensors), in one run.

    python tools/fill_bench.py [--out FILE] [--files N] [--rows N]   -> one JSON line per measurement (appended to FILE too)

  files    real_imu_frames on 60 recordings x 10 000 rows x 17 sensors with 2 % of the parts bad: the tip_fill_real launch alone
           (device events, best and median of 7), the whole call (concatenation, launch, the strict read-back; wall clock), and the
           numpy oracle of tests/sensor_fill_oracle.py on the first 3 recordings of the same arrays, scaled per row
  kernel   tip_fill_live alone and tip_sensor_transform + tip_fill_live at 1, 256 and 1024 slots: device events around 2000
           back-to-back launches, us per launch
  frame    StreamingEngine.step_packets at 1, 256 and 1024 streams with a fill=True and a fill=False front end on the same packets
           (2 % of the sensors silent), launch by launch and use_graph=True, the two arms alternating in blocks of 30 frames:
           median, fastest and slowest of 9 blocks per arm, ms per frame
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
from staggered_bench import model, block, emit  # noqa: E402
import sensor_fill_oracle as fo  # noqa: E402

SIZES = (1, 256, 1024)
BLOCKS, PER_BLOCK, BAD = 9, 30, 0.02


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def recordings(files, rows, seed=0):
    """files x (ori [rows, 17, 3, 3], acc [rows, 17, 3]) fp64 on the device, BAD of the parts NaN; rows 0 .. 9 are left whole."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    oris, accs = [], []
    for _ in range(files):
        ori = torch.randn((rows, 17, 3, 3), dtype=torch.float64, device="cuda", generator=g)
        acc = torch.randn((rows, 17, 3), dtype=torch.float64, device="cuda", generator=g) * 4
        for t, w in ((ori, (rows, 17, 1, 1)), (acc, (rows, 17, 1))):
            bad = torch.rand(w, device="cuda", generator=g) < BAD
            bad[:10] = False
            t.masked_fill_(bad, float("nan"))
        oris.append(ori), accs.append(acc)
    return oris, accs


def files_part(files, rows):
    oris, accs = recordings(files, rows)
    lib = sensors._lib.load()
    ori, offs, lens = sensors._stack(oris, torch.float64, 17 * 9, torch.device("cuda", 0), "fill_bench", "ori")
    acc, _, _ = sensors._stack(accs, torch.float64, 17 * 3, torch.device("cuda", 0), "fill_bench", "acc")
    N = int(ori.shape[0])
    out = torch.empty((N, 72), dtype=torch.float64, device="cuda")
    unfilled = torch.zeros(files, dtype=torch.int32, device="cuda")
    import ctypes
    sel, rot = (ctypes.c_int * 6)(*sensors.SEL_DIP17), (ctypes.c_double * 9)(*sensors.ROT_DIP.reshape(-1))
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        assert lib.tip_fill_real(ori.data_ptr(), acc.data_ptr(), N, 17, offs.data_ptr(), files, sel, rot, out.data_ptr(), unfilled.data_ptr(),
                                 stream) == 0
    launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(7):
        torch.cuda.synchronize()
        a.record()
        launch()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    del ori, acc
    call = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = sensors.real_imu_frames(oris, accs, sensors.ROT_DIP)
        torch.cuda.synchronize()
        call.append((time.perf_counter() - t0) * 1e3)
    sub = min(3, files)
    t0 = time.perf_counter()
    ref = [fo.real_frames(oris[i].cpu().numpy(), accs[i].cpu().numpy(), sensors.ROT_DIP, sensors.SEL_DIP17)[0] for i in range(sub)]
    oracle_ms = (time.perf_counter() - t0) * 1e3 * files / sub
    same = all(np.array_equal(got[i].cpu().numpy(), ref[i], equal_nan=True) for i in range(sub))
    gb = N * (17 * 12 + 72) * 8 / 1e9
    return {"what": "files", "files": files, "rows": rows, "sensors": 17, "bad_parts": BAD, "fill_real_ms_best": round(min(ms), 3),
            "fill_real_ms_median": round(float(np.median(ms)), 3), "bytes_touched_GB": round(gb, 3),
            "whole_tensor_GBps": round(gb / (min(ms) * 1e-3), 1), "real_imu_frames_call_ms_best": round(min(call), 2),
            "numpy_oracle_ms_scaled_from": sub, "numpy_oracle_ms": round(oracle_ms, 1), "oracle_over_launch": round(oracle_ms / min(ms), 1),
            "bit_identical_to_oracle": bool(same), "unfilled": int(unfilled.sum())}


def inputs(n, seed):
    """Two loaded front ends (fill on, fill off), 8 packets [n, 42] on the device with BAD of the sensors silent, start states."""
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(seed)
    rot = lambda k: Rotation.random(n * 6, random_state=seed + k).as_matrix().reshape(n, 54)       # noqa: E731
    tables = np.concatenate([rot(0), rng.randn(n, 18) * 0.1, rot(1)], axis=1).astype(np.float32)
    fronts = {}
    for tag, kw in (("fill", {"fill": True}), ("plain", {})):
        fronts[tag] = sensors.SensorFrontEnd(n, "cuda", **kw)
        fronts[tag].load(range(n), tables)
    base = Rotation.random(n * 6, random_state=seed + 2)
    packets = []
    for j in range(8):
        q = (base * Rotation.from_rotvec(rng.randn(n * 6, 3) * 0.05)).as_quat() * rng.uniform(0.3, 3.0, size=(n * 6, 1))
        if j:                                                    # (packet 0 whole: the rings have something to fill from)
            q[rng.rand(n * 6) < BAD] = np.nan
        p = np.concatenate([q, rng.randn(n * 6, 3) * 0.5], axis=1).reshape(n, 42).astype(np.float32)
        packets.append(torch.tensor(p).cuda())
    return fronts, packets, (rng.randn(n, 114) * 0.2).astype(np.float32)


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
    return min(got), float(np.median(got))


def alternate(arms):
    for fn in arms.values():
        block(fn, 8)
    got = {t: [] for t in arms}
    for _ in range(BLOCKS):
        for t, fn in arms.items():
            got[t].append(block(fn, PER_BLOCK))
    return got


def main():
    torch.backends.cudnn.benchmark = False
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    recs = [files_part(arg("--files", 60), arg("--rows", 10000))]
    emit(recs[-1])
    torch.cuda.empty_cache()
    m = model()
    for n in SIZES:
        fronts, packets, s_init = inputs(n, n)
        on, off = fronts["fill"], fronts["plain"]
        raw = torch.empty((n, 72), dtype=torch.float32, device="cuda")
        on._fill(packets[1], "fill_bench")
        off._fill(packets[1], "fill_bench")
        off._transform_into(raw)
        lib, st = on.lib, on._stream()
        live = per_launch_us(lambda: lib.tip_fill_live(on.fill_state.data_ptr(), on.cal.data_ptr(), raw.data_ptr(), n, -1, on.filled.data_ptr(), st))
        plain = per_launch_us(lambda: off._transform_into(raw))
        pair = per_launch_us(lambda: on._transform_into(raw))
        rec = {"what": "kernel", "n": n, "fill_live_us_per_launch": round(live[0], 2), "fill_live_us_median": round(live[1], 2),
               "transform_us_per_launch": round(plain[0], 2), "transform_plus_fill_us": round(pair[0], 2)}
        emit(rec)
        recs.append(rec)
        for graph in (False, True):
            a = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=graph)
            b = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=graph)
            for f in range(50):                       # past the warm-up: every window at T = 40 in both
                a.step_packets(on, packets[f % 8])
                b.step_packets(off, packets[f % 8])
            torch.cuda.synchronize()
            res = alternate({"fill": lambda i: a.step_packets(on, packets[i % 8]), "plain": lambda i: b.step_packets(off, packets[i % 8])})
            med = {t: float(np.median(v)) for t, v in res.items()}
            rec = {"what": "frame", "n": n, "graph": graph, "blocks": BLOCKS, "frames_per_block": PER_BLOCK}
            for t, v in res.items():
                rec[f"{t}_ms_median"] = round(med[t], 4)
                rec[f"{t}_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
            rec["ratio_of_medians"] = round(med["fill"] / med["plain"], 4)
            rec["delta_us"] = round((med["fill"] - med["plain"]) * 1e3, 1)
            rec["filled_parts_total"] = int(on.fill_counts()[2].sum())
            emit(rec)
            recs.append(rec)
            del a, b
    m.check_handoffs()
    if out_path:
        with open(out_path, "a") as fh:
            for r in recs:
                fh.write(json.dumps(r) + "\n")
    for r in recs:
        print(r, file=sys.stderr)


if __name__ == "__main__":
    main()
