"""Offline replay of recorded IMU files: tip_amd.replay.ReplayPool (the device feeds itself) against the same replay driven frame by
frame from the host through StaggeredStreamingEngine.step.

    python tools/replay_bench.py [--slots 8,64,256] [--frames 600] [--per-slot 4] [--runs 4]
        -> one JSON line per (slots, path, run) and one summary line per slots

Paper model, synthetic weights, R = per-slot x slots synthetic recordings of --frames frames each (tip_amd.synth.make_recording), graph
mode on in both paths.  A run is "recordings on the host in, trajectories on the host out", timed by the wall clock around it:
  pool  ReplayPool.run: corpus upload, every engine frame (feed -> mapped frame -> collect, one graph launch), one synchronisation,
        download.  The captures of a run (one per bucket it meets) are inside the time: the pool re-captures for every run's buffers.
  host  what a user could write before ReplayPool existed: the same schedule (plan_replay), attach / detach on its frames, one
        eng.step(frame) per engine frame on a compact graph-mode engine with the frame taken from a pinned [F, n, 72] array, the
        frame's s_rest / c_t / T rows stacked into device arrays, one synchronisation, download.  The pinned frame array is assembled
        BEFORE the clock starts (a per-frame gather on the host would only slow this path), and the stacked outputs are left in
        frame-major order (the per-recording scatter is not charged either).
The two paths alternate, --runs runs each, after one unrecorded run each.  Reported: engine frames per second and recordings per
second per run, the median of each path, the host path's own run-to-run spread ((max - min) / median) and the ratio of the medians.
profiles/replay/replay_bench.txt holds the recorded runs."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def host_replay(eng, plan, recs, s0, frames_pinned):
    """The replay without tip_amd.replay's device side: one step() per engine frame, outputs stacked on the device."""
    n, F = eng.n, plan.n_frames
    eng.detach([i for i in range(n) if eng.attached[i]])
    eng.reset()
    s_all = torch.empty((F, n, 111), dtype=torch.float32, device=eng.device)
    c_all = torch.empty((F, n, eng.nc), dtype=torch.float32, device=eng.device)
    t_all = torch.empty((F, n), dtype=torch.int32, device=eng.device)
    for f, (att, det) in enumerate(plan.frames):
        if det:
            eng.detach(det)
        if att:
            eng.attach([s for s, _ in att], s0[[i for _, i in att]])
        out = eng.step(frames_pinned[f])
        s_all[f].copy_(out["s_rest"])
        c_all[f].copy_(out["c_t"])
        t_all[f].copy_(out["T"])
    eng.detach(plan.final_detach)
    torch.cuda.current_stream(eng.device).synchronize()
    return s_all.cpu(), c_all.cpu(), t_all.cpu()


def assemble_frames(plan, recs, n):
    """[F, n, 72] pinned: what each slot is fed on each engine frame (zeros where a slot is idle)."""
    fr = np.zeros((plan.n_frames, n, 72), dtype=np.float32)
    for i, r in enumerate(recs):
        if plan.start[i] >= 0:
            fr[plan.start[i]: plan.start[i] + r.shape[0] - 1, plan.slot[i]] = r[:-1]
    return torch.from_numpy(fr).pin_memory()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="8,64,256")
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--per-slot", type=int, default=4)
    ap.add_argument("--runs", type=int, default=4)
    a = ap.parse_args()
    import tip_amd
    from tip_amd import replay, synth
    from staggered_bench import model

    m = model()
    for n in (int(x) for x in a.slots.split(",")):
        R = a.per_slot * n
        recs, s0 = zip(*(synth.make_recording(a.frames, seed=1000 + i) for i in range(R)))
        recs, s0 = list(recs), np.stack(s0)
        plan = replay.plan_replay([a.frames] * R, n)
        pool = replay.ReplayPool(m, slots=n, use_graph=True)
        eng = tip_amd.streaming.StaggeredStreamingEngine(m, np.zeros((n, 114), dtype=np.float32), use_graph=True, compact=True)
        frames_pinned = assemble_frames(plan, recs, n)

        def run_pool():
            pool.run(recs, s0)
            assert pool.frames == plan.n_frames and pool.restarts == 0

        paths = {"pool": run_pool, "host": lambda: host_replay(eng, plan, recs, s0, frames_pinned)}
        fps = {k: [] for k in paths}
        for r in range(-1, a.runs):                   # (run -1: not recorded)
            for k, fn in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                dt = time.perf_counter() - t0
                if r >= 0:
                    fps[k].append(plan.n_frames / dt)
                    print(json.dumps({"slots": n, "recordings": R, "frames_each": a.frames, "engine_frames": plan.n_frames, "path": k,
                                      "run": r, "seconds": round(dt, 4), "engine_frames_per_s": round(plan.n_frames / dt, 1),
                                      "recordings_per_s": round(R / dt, 2)}), flush=True)
        med = {k: float(np.median(v)) for k, v in fps.items()}
        print(json.dumps({"slots": n, "summary": True, "pool_frames_per_s_median": round(med["pool"], 1),
                          "host_frames_per_s_median": round(med["host"], 1),
                          "pool_recordings_per_s_median": round(med["pool"] * R / plan.n_frames, 2),
                          "host_recordings_per_s_median": round(med["host"] * R / plan.n_frames, 2),
                          "host_spread": round((max(fps["host"]) - min(fps["host"])) / med["host"], 4),
                          "pool_spread": round((max(fps["pool"]) - min(fps["pool"])) / med["pool"], 4),
                          "pool_over_host": round(med["pool"] / med["host"], 4)}), flush=True)
        del pool, eng, frames_pinned
    m.check_handoffs()


if __name__ == "__main__":
    main()
