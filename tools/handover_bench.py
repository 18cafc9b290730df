"""What a wearer hand-over costs (csrc/tip_handover.hip; tip_amd.handover), in one run on one MI355X.

    python tools/handover_bench.py [--out FILE]      -> one JSON line per measurement; FILE (default: the record,
                                                        profiles/handover/handover_bench.txt) gets a header and the same lines

  chain   export_wearers + import_wearers of 1, 64 and 1024 wearers with the whole chain — ClockSync, PacketResampler(depth 8),
          SensorFrontEnd(fill=True), a compact StaggeredStreamingEngine, TerrainTracker(multi_sbp, the script's 100 x 100 map) — from one
          set of objects into another of the same n, as back-to-back launches: device events around the pair and host time to the end
          of the pair (synchronised), median / min / max of 15 after 3.  The yardstick, in the same run: two plain device-to-device
          copy_ of the same number of CONTIGUOUS bytes (out and in again: what the pair moves).  The ratio is recorded, not fixed.
  frame   a compact pool of 64 slots with 40 attached (use_graph=True, every bucket captured first): the frame with an import of 1 and
          of 8 wearers in front of it, against the same frame with an attach of the same slots in front of it — what the pool already
          offered.  Both arms detach the slots again behind the frame; the arms alternate in blocks of 30 frames: median, fastest and
          slowest of 9 blocks per arm, ms per frame (host time, synchronised at the end of a block).
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
import tip_amd  # noqa: E402
from tip_amd import handover, sensors, terrain  # noqa: E402
from tip_amd import kinematics as kin  # noqa: E402
from staggered_bench import frames, model  # noqa: E402
from resample_bench import alternate, BLOCKS, PER_BLOCK  # noqa: E402

SIZES = (1, 64, 1024)
WARM, REPS = 3, 15


def chain(m, skel, n, s_init):
    eng = tip_amd.streaming.StaggeredStreamingEngine(m, s_init, compact=True)
    tt = terrain.TerrainTracker(skel, n, "cuda", multi_sbp=True)
    tt.reset(None, s_init)
    return dict(engine=eng, front=sensors.SensorFrontEnd(n, "cuda", fill=True), resampler=sensors.PacketResampler(n, "cuda", mode="predict"),
                clock=sensors.ClockSync(n, "cuda"), tracker=tt)


def timed(fn, before):
    """fn() REPS times after WARM, before() untimed in front of each: (device-event ms, host ms to the synchronised end)."""
    ev, host = [], []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(WARM + REPS):
        before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            host.append((time.perf_counter() - t0) * 1e3)
            ev.append(a.elapsed_time(b))
    q = lambda v: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]      # noqa: E731
    return q(ev), q(host)


def chain_part(m, skel, n, emit):
    fr, s_init = frames(n, n)
    A, B = chain(m, skel, n, s_init), chain(m, skel, n, s_init)
    for f in range(8):
        A["engine"].step(fr[f % 8])
    slots = list(range(n))
    w = handover.export_wearers(slots, **A)
    per_wearer = sum(int(p["meta"].get(k, 0)) for p in w.parts.values() for k in ("block_bytes", "fill_block_bytes"))
    total = per_wearer * n

    def pair():
        handover.import_wearers(handover.export_wearers(slots, **A), slots, **B)

    ev, host = timed(pair, lambda: B["engine"].detach(slots))
    src, tmp, dst = (torch.empty(total, dtype=torch.uint8, device="cuda") for _ in range(3))
    src.random_(0, 256)

    def copies():
        tmp.copy_(src)
        dst.copy_(tmp)

    cev, chost = timed(copies, lambda: None)
    emit({"what": "chain", "wearers": n, "bytes_per_wearer": per_wearer, "bytes_moved_each_way": total,
          "export_import_event_ms_median_min_max": ev, "export_import_host_ms_median_min_max": host,
          "two_copies_event_ms_median_min_max": cev, "two_copies_host_ms_median_min_max": chost,
          "event_ratio_of_medians": round(ev[0] / cev[0], 2), "host_ratio_of_medians": round(host[0] / chost[0], 2),
          "GBps_over_the_pair_at_event_median": round(2 * total / (ev[0] * 1e-3) / 1e9, 2)})


def frame_part(m, k, emit):
    n, live = 64, 40
    fr, s_init = frames(n, 7)
    warm = tip_amd.streaming.StaggeredStreamingEngine(m, s_init[:8], compact=True)          # the warm-up pool the wearers come from
    for f in range(50):
        warm.step(fr[f % 8][:8])
    w = warm.export_slots(list(range(k)))
    arms = {}
    slots = list(range(n - k, n))
    for tag in ("import", "attach"):
        pool = tip_amd.streaming.StaggeredStreamingEngine(m, s_init, compact=True, use_graph=True)
        pool.detach(list(range(live, n)))
        pool.prewarm()
        for f in range(50):
            pool.step(fr[f % 8])

        def step(i, pool=pool, tag=tag):
            if tag == "import":
                pool.import_slots(slots, w)
            else:
                pool.attach(slots, s_init[slots])
            pool.step(fr[i % 8])
            pool.detach(slots)
        arms[tag] = step
    res = alternate(arms)
    med = {t: float(np.median(v)) for t, v in res.items()}
    rec = {"what": "frame", "pool": n, "attached": live, "wearers_in_front": k, "blocks": BLOCKS, "frames_per_block": PER_BLOCK}
    for t, v in res.items():
        rec[f"{t}_then_frame_ms_median"] = round(med[t], 4)
        rec[f"{t}_then_frame_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    rec["import_over_attach_medians"] = round(med["import"] / med["attach"], 4)
    rec["delta_us"] = round((med["import"] - med["attach"]) * 1e3, 1)
    emit(rec)


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "handover", "handover_bench.txt")
    if not torch.cuda.is_available():
        raise SystemExit("tools/handover_bench.py measures on an MI355X: no GPU here")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    m = model()
    skel = kin.Skeleton.from_table(np.load(os.path.join(ROOT, "tests", "golden", "tip_terrain_golden.npz")))
    for n in SIZES:
        chain_part(m, skel, n, emit)
        torch.cuda.empty_cache()
    for k in (1, 8):
        frame_part(m, k, emit)
    m.check_handoffs()
    with open(out_path, "w") as f:
        f.write("# tools/handover_bench.py on one MI355X, one run.\n"
                "# chain: export_wearers + import_wearers of the whole chain (clock, resampler, front end with fill, compact engine, terrain\n"
                "#        tracker) between two sets of objects, back-to-back launches; device events around the pair and host time to its\n"
                "#        synchronised end, [median, min, max] of 15 after 3; beside it two plain copy_ of the same contiguous bytes\n"
                "# frame: compact pool of 64 with 40 attached, use_graph=True: import of k wearers + frame + detach against attach of the same\n"
                "#        slots + frame + detach, alternating blocks of 30 frames: median, fastest and slowest of 9 blocks, ms per frame\n")
        f.write("\n".join(lines) + "\nok\n")
    print("ok")


if __name__ == "__main__":
    main()
