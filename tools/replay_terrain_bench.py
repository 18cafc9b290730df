"""Offline replay through the FULL runner (terrain map, height correction, leg IK with its feedback into the model's history):
tip_amd.replay.ReplayPool(terrain=...) against the two things a user could do before it.

    python tools/replay_terrain_bench.py [--slots 8,64,256] [--frames 600] [--per-slot 4] [--runs 4]
        -> one JSON line per (slots, path, run) and one summary line per slots

Paper model, synthetic weights with the contact logits of lankle, rankle and root shifted by +0.5 (so that contacts hold and the IK has
something to do), R = per-slot x slots synthetic recordings of --frames frames each (tip_amd.synth.make_recording), graph mode on in
every path, the reference's map (map_bound 5.0, grid_size 0.1).  A run is "recordings on the host in, trajectories on the host out",
timed by the wall clock around it, as in tools/replay_bench.py:
  tracked  ReplayPool(terrain=dict(..., multi_sbp=True)).run: per engine frame ONE graph launch holding feed -> the mapped frame ->
           mask -> terrain step -> history override -> tracked collect; tracker resets on the plan's attach frames; one
           synchronisation; download.  The run's captures are inside the time.
  post     the plain ReplayPool.run, then kinematics.track_replay(terrain=...): what the full runner WITHOUT feedback
           (multi_sbp_terrain_and_correction off) costs today — one more kernel over the downloaded rows.  It does not compute what
           `tracked` computes (no IK feedback); it is the price of the exact post-pass.
  host     the only way to get the IK feedback before this pool: the schedule of plan_replay driven from the host on a compact
           graph-mode engine — per engine frame eng.step(frame from a pinned [F, n, 72] array), TerrainTracker.step, feed_back, the
           frame's rows stacked into device arrays; tracker resets on attach; one synchronisation; download.  The pinned frame array is
           assembled before the clock starts and the stacked outputs stay in frame-major order (neither is charged).
The paths alternate, --runs runs each, after one unrecorded run each.  Reported: engine frames per second per run, the median of each
path, the host path's own run-to-run spread ((max - min) / median) and the two ratios tracked / host and tracked / post.  Launches per
engine frame (host API calls that start device work): tracked 1 graph launch; host 13: the frame copy, 1 graph launch, 2 small kernels
(T, valid), the track, the override and 7 row copies.  profiles/replay/replay_terrain_bench.txt holds the recorded run."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

MAP = dict(map_bound=5.0, grid_size=0.1)
BIAS_INDEX, BIAS_SHIFT = (111, 115, 127), 0.5


def shifted_model():
    import tip_amd
    from tip_amd import synth
    cfg = synth.PAPER
    m = tip_amd.TF_RNN_Past_State(cfg["input_size_imu"], cfg["size_s"], rnn_hid_size=cfg["rnn_hid_size"], tf_hid_size=cfg["tf_hid_size"],
                                  tf_in_dim=cfg["tf_in_dim"], n_heads=cfg["n_heads"], tf_layers=cfg["tf_layers"], dropout=0.0,
                                  in_dropout=0.0, past_state_dropout=0.0, with_rnn=True, with_acc_sum=True)
    w = synth.make_weights(cfg, seed=0)
    w["linear.bias"] = w["linear.bias"].copy()
    w["linear.bias"][list(BIAS_INDEX)] += np.float32(BIAS_SHIFT)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    m = m.cuda().eval()
    m.freeze_packed(True)
    return m


def host_replay(eng, tt, plan, s0, frames_pinned):
    """The tracked replay without the pool's device side: step, tracker step and feed_back per engine frame, outputs stacked."""
    n, F, dev = eng.n, plan.n_frames, eng.device
    eng.detach([i for i in range(n) if eng.attached[i]])
    eng.reset()
    s_all = torch.empty((F, n, 111), dtype=torch.float32, device=dev)
    c_all = torch.empty((F, n, eng.nc), dtype=torch.float32, device=dev)
    t_all = torch.empty((F, n), dtype=torch.int32, device=dev)
    root_all = torch.empty((F, n, 3), dtype=torch.float32, device=dev)
    viz_all = torch.empty((F, n, 5, 3), dtype=torch.float32, device=dev)
    q_all = torch.empty((F, n, 54), dtype=torch.float32, device=dev)
    fire_all = torch.empty((F, n), dtype=torch.int32, device=dev)
    for f, (att, det) in enumerate(plan.frames):
        if det:
            eng.detach(det)
        if att:
            sl, rows = [s for s, _ in att], s0[[i for _, i in att]]
            eng.attach(sl, rows)
            tt.reset(sl, rows)
        out = eng.step(frames_pinned[f])
        tt.step(out)
        tt.feed_back(eng)
        s_all[f].copy_(out["s_rest"])
        c_all[f].copy_(out["c_t"])
        t_all[f].copy_(out["T"])
        root_all[f].copy_(tt.root)
        viz_all[f].copy_(tt.viz_locs)
        q_all[f].copy_(tt.q_hist)
        fire_all[f].copy_(tt.fire)
    eng.detach(plan.final_detach)
    torch.cuda.current_stream(dev).synchronize()
    return [t.cpu() for t in (s_all, c_all, t_all, root_all, viz_all, q_all, fire_all)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="8,64,256")
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--per-slot", type=int, default=4)
    ap.add_argument("--runs", type=int, default=4)
    a = ap.parse_args()
    import tip_amd
    from tip_amd import kinematics as kin, replay, synth, terrain
    from replay_bench import assemble_frames

    m = shifted_model()
    skel = kin.Skeleton.from_table(np.load(os.path.join(ROOT, "tests", "golden", "tip_kin_golden.npz")))
    for n in (int(x) for x in a.slots.split(",")):
        R = a.per_slot * n
        recs, s0 = zip(*(synth.make_recording(a.frames, seed=1000 + i) for i in range(R)))
        recs, s0 = list(recs), np.stack(s0)
        plan = replay.plan_replay([a.frames] * R, n)
        tracked = replay.ReplayPool(m, slots=n, use_graph=True, terrain=dict(skel=skel, multi_sbp=True, **MAP))
        plain = replay.ReplayPool(m, slots=n, use_graph=True)
        eng = tip_amd.streaming.StaggeredStreamingEngine(m, np.zeros((n, 114), dtype=np.float32), use_graph=True, compact=True)
        tt = terrain.TerrainTracker(skel, n, eng.device, multi_sbp=True, **MAP)
        frames_pinned = assemble_frames(plan, recs, n)
        fired = {}

        def run_tracked():
            out = tracked.run(recs, s0)
            assert tracked.frames == plan.n_frames and tracked.restarts == 0
            fired["tracked"] = int(sum(r.fire.sum() for r in out))

        def run_post():
            out = plain.run(recs, s0)
            kin.track_replay(skel, out, s0, terrain=MAP)

        def run_host():
            out = host_replay(eng, tt, plan, s0, frames_pinned)
            fired["host"] = int((out[6] >= 0).sum())

        paths = {"tracked": run_tracked, "post": run_post, "host": run_host}
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
        print(json.dumps({"slots": n, "summary": True, **{f"{k}_frames_per_s_median": round(v, 1) for k, v in med.items()},
                          **{f"{k}_spread": round((max(fps[k]) - min(fps[k])) / med[k], 4) for k in fps},
                          "tracked_over_host": round(med["tracked"] / med["host"], 4),
                          "tracked_over_post": round(med["tracked"] / med["post"], 4),
                          "rows_the_ik_fired_on": fired, "launches_per_frame": {"tracked": 1, "host": 13}}), flush=True)
        del tracked, plain, eng, tt, frames_pinned
    m.check_handoffs()


if __name__ == "__main__":
    main()
