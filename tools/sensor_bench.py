"""The sensor front end's cost per closed-loop frame: step_packets(front, packets) against step(raw) fed the same frames already
transformed, both arms in ONE run, alternating in blocks, a warm-up for every shape; ms per frame (best of the blocks).  Inputs of
both arms are device tensors (a [n,42] copy + the transform launch against a [n,72] copy).  Also the transform launch alone.

    python tools/sensor_bench.py [--out FILE]   -> one JSON line per measurement (appended to FILE too) + a table on stderr

  frame    StreamingEngine at 1, 256 and 1024 streams, launch by launch and use_graph=True, past the warm-up (T = 40)
  kernel   tip_sensor_transform alone at the same sizes: device events around 2000 back-to-back launches, us per launch
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tip_amd  # noqa: E402
from tip_amd import sensors  # noqa: E402
from staggered_bench import model, alternate, emit  # noqa: E402

SIZES = (1, 256, 1024)


def inputs(n, seed):
    """A loaded front end, 8 packets [n,42] on the device, their transformed frames [n,72], and start states."""
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(seed)
    rot = lambda k: Rotation.random(n * 6, random_state=seed + k).as_matrix().reshape(n, 54)       # noqa: E731
    tables = np.concatenate([rot(0), rng.randn(n, 18) * 0.1, rot(1)], axis=1).astype(np.float32)
    front = sensors.SensorFrontEnd(n, "cuda")
    front.load(range(n), tables)
    base = Rotation.random(n * 6, random_state=seed + 2)
    packets = []
    for _ in range(8):
        q = (base * Rotation.from_rotvec(rng.randn(n * 6, 3) * 0.05)).as_quat() * rng.uniform(0.3, 3.0, size=(n * 6, 1))
        p = np.concatenate([q, rng.randn(n * 6, 3) * 0.5], axis=1).reshape(n, 42).astype(np.float32)
        packets.append(torch.tensor(p).cuda())
    frames = [front.transform(p).clone() for p in packets]
    return front, packets, frames, (rng.randn(n, 114) * 0.2).astype(np.float32)


def kernel_us(front, packets, launches=2000):
    raw = torch.empty((front.n, 72), dtype=torch.float32, device=front.device)
    front._fill(packets[0], "sensor_bench")
    for _ in range(50):
        front._transform_into(raw)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = 1e9
    for _ in range(5):
        torch.cuda.synchronize()
        a.record()
        for _ in range(launches):
            front._transform_into(raw)
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / launches * 1e3)
    return best


def main():
    torch.backends.cudnn.benchmark = False
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    m = model()
    recs = []
    for n in SIZES:
        front, packets, frames, s_init = inputs(n, n)
        k_us = kernel_us(front, packets)
        rec = {"what": "kernel", "n": n, "transform_us_per_launch": round(k_us, 2)}
        emit(rec)
        recs.append(rec)
        for graph in (False, True):
            a = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=graph)
            b = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=graph)
            for f in range(50):                       # past the warm-up: every window at T = 40 in both
                oa = a.step(frames[f % 8])
                ob = b.step_packets(front, packets[f % 8])
            torch.cuda.synchronize()
            same = bool(torch.equal(oa["y_last"].view(torch.int32), ob["y_last"].view(torch.int32)))
            res = alternate({"raw": lambda i: a.step(frames[i % 8]), "packets": lambda i: b.step_packets(front, packets[i % 8])})
            rec = {"what": "frame", "n": n, "graph": graph, "step_raw_ms": round(res["raw"], 4), "step_packets_ms": round(res["packets"], 4),
                   "ratio": round(res["packets"] / res["raw"], 4), "delta_us": round((res["packets"] - res["raw"]) * 1e3, 1),
                   "transform_us_per_launch": round(k_us, 2), "bit_identical_after_50_frames": same}
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
