"""What recording live sessions costs (csrc/tip_record.hip; tip_amd.record.SessionRecorder), in one run on one MI355X.

    python tools/record_bench.py [--out FILE]      -> one JSON line per measurement; FILE (default: the record,
                                                      profiles/record/record_bench.txt) gets a header and the same lines

  At 1, 256 and 1024 slots, every slot attached, open and valid, rows of raw | s_rest | c_t (203 floats, the 4-byte copy path):
  append  the per-frame launch back to back: device events around 100 launches, us per launch, median / min / max of 15 after 3 (the
          pool is drained, untimed, in front of every repetition so that no row is dropped), and the bytes it moves per second.
  frame   a compact pool (use_graph=True, steady state) — the frame alone; with rec.step() behind it; with rec.step() and a drain()
          every 16 frames of the arm's own running count (default staging_pages: max(16, n / 4) pages copied per drain); and the host-synchronising alternative, engine.raw.cpu() behind every frame (IMU rows only, a quarter of
          what the recorder takes) — the arms alternate in blocks of 30 frames: median, fastest and slowest of 9 blocks per arm, ms per
          frame (host time, synchronised at the end of a block).
  drain   n full pages of 64 rows on the queue: drain(wait=True) — the launch, the copy of the staging buffer to pinned memory and
          the filing — host ms, median / min / max of 7 after 2, and us per page.
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
from tip_amd import record  # noqa: E402
from staggered_bench import frames, model  # noqa: E402
from resample_bench import alternate, BLOCKS, PER_BLOCK  # noqa: E402

SIZES = (1, 256, 1024)
LAUNCHES, WARM, REPS = 100, 3, 15
q = lambda v: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]      # noqa: E731


def pool(m, n, fr, s_init):
    eng = tip_amd.streaming.StaggeredStreamingEngine(m, s_init, compact=True, use_graph=True)
    for f in range(50):                                  # (past the warm-up: every slot at T = 40)
        eng.step(fr[f % 8])
    return eng


def drained(rec):
    """Every session closed, brought to the host and forgotten; every slot open again on an empty pool (untimed)."""
    rec.close(range(rec.n))
    rec.drain(wait=True)
    while rec.queued:
        rec.drain(wait=True)
    for s in rec.sessions():
        rec.pop(s.name)
    rec.open(range(rec.n))


def append_part(m, n, emit):
    fr, s_init = frames(n, n)
    eng = pool(m, n, fr, s_init)
    rec = record.SessionRecorder.for_engine(eng)
    rec.open(range(n))
    us = []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(WARM + REPS):
        drained(rec)
        torch.cuda.synchronize()
        a.record()
        for _ in range(LAUNCHES):
            rec.step()
        b.record()
        torch.cuda.synchronize()
        if i >= WARM:
            us.append(a.elapsed_time(b) / LAUNCHES * 1e3)
    c = rec.counters(wait=True)
    moved = 2 * n * rec.width * 4
    emit({"what": "append", "slots": n, "row_floats": rec.width, "launches_per_repetition": LAUNCHES, "rows_dropped": c["rows_dropped"],
          "us_per_launch_median_min_max": q(us), "bytes_read_and_written_per_launch": moved,
          "GBps_at_median": round(moved / (statistics.median(us) * 1e-6) / 1e9, 2), "state_MB": round(rec.state_bytes / 1e6, 1)})


def frame_part(m, n, emit):
    fr, s_init = frames(n, n)
    frames_in_all = 8 + BLOCKS * PER_BLOCK + 8
    arms, recs = {}, {}
    for tag in ("frame", "frame+step", "frame+step+drain16", "frame+raw.cpu()"):
        eng = pool(m, n, fr, s_init)
        rec = None
        if tag == "frame+step":                          # (no drain in this arm: a pool that holds every row of the run)
            rec = record.SessionRecorder.for_engine(eng, pages=n * (frames_in_all // 64 + 2))
        elif tag == "frame+step+drain16":
            rec = record.SessionRecorder.for_engine(eng)
        if rec is not None:
            rec.open(range(n))
            rec.drain(wait=True)                         # (the first pinned buffer is allocated here, not inside a timed block)
            recs[tag] = rec

        def step(i, eng=eng, rec=rec, tag=tag, count=[0]):
            # (i restarts in every block: the drain's rhythm follows the arm's own running frame count)
            eng.step(fr[i % 8])
            count[0] += 1
            if rec is not None:
                rec.step()
                if tag.endswith("drain16") and count[0] % 16 == 0:
                    rec.drain()
            elif tag.endswith("cpu()"):
                eng.raw.cpu()
        arms[tag] = step
    res = alternate(arms)
    med = {t: float(np.median(v)) for t, v in res.items()}
    out = {"what": "frame", "slots": n, "blocks": BLOCKS, "frames_per_block": PER_BLOCK}
    for t, v in res.items():
        out[f"{t}_ms_median_min_max"] = [round(med[t], 4), round(min(v), 4), round(max(v), 4)]
    for t in list(res)[1:]:
        out[f"{t}_minus_frame_us"] = round((med[t] - med["frame"]) * 1e3, 1)
    out["rows_dropped"] = {t: r.counters(wait=True)["rows_dropped"] for t, r in recs.items()}
    d = recs["frame+step+drain16"]
    out["drains"], out["staging_pages"], out["staging_MB"] = d.drains, d.staging_pages, round(d.staging_bytes / 1e6, 2)
    emit(out)


def drain_part(m, n, emit):
    fr, s_init = frames(n, n)
    eng = pool(m, n, fr, s_init)
    rec = record.SessionRecorder.for_engine(eng, staging_pages=n)
    rec.open(range(n))
    ms = []
    for i in range(2 + 7):
        for _ in range(rec.page_rows):                   # every slot fills exactly one page
            rec.step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rec.drain(wait=True)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert rec.queued == 0
        drained(rec)
    ms = ms[2:]
    page = rec.page_rows * rec.width * 4
    emit({"what": "drain", "slots": n, "pages_per_drain": n, "page_bytes": page, "staging_MB": round(rec.staging_bytes / 1e6, 2),
          "drain_wait_host_ms_median_min_max": q(ms), "us_per_page_at_median": round(statistics.median(ms) * 1e3 / n, 2),
          "GBps_to_the_host_at_median": round(n * page / (statistics.median(ms) * 1e-3) / 1e9, 2)})


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "record", "record_bench.txt")
    if not torch.cuda.is_available():
        raise SystemExit("tools/record_bench.py measures on an MI355X: no GPU here")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    m = model()
    for part in (append_part, frame_part, drain_part):
        for n in SIZES:
            part(m, n, emit)
            torch.cuda.empty_cache()
    m.check_handoffs()
    with open(out_path, "w") as f:
        f.write("# tools/record_bench.py on one MI355X, one run.  Rows of raw | s_rest | c_t = 203 floats; every slot attached, open and valid.\n"
                "# append: tip_record_append back to back, device events around 100 launches, us per launch [median, min, max] of 15 after 3\n"
                "# frame:  compact pool, use_graph=True, steady state: the frame alone / + rec.step() / + rec.step() and a drain() every 16\n"
                "#         frames of the arm's running count (default staging_pages) / + engine.raw.cpu() (the synchronising alternative, IMU rows only); alternating blocks of 30 frames,\n"
                "#         ms per frame [median, fastest, slowest] of 9 blocks, host time synchronised at the end of a block\n"
                "# drain:  n full pages of 64 rows: drain(wait=True) — launch, copy of the staging buffer to pinned memory, filing — host ms\n"
                "#         [median, min, max] of 7 after 2\n")
        f.write("\n".join(lines) + "\nok\n")
    print("ok")


if __name__ == "__main__":
    main()
