"""Staggered streams (per-slot attach / detach, include/tip_hip.h) against the lock-step engine, both arms in ONE run, alternating
in blocks, a warm-up for every shape; ms per closed-loop frame (best of the blocks) and the outputs' agreement.

    python tools/staggered_bench.py [steady] [rows] [churn]    -> one JSON line per measurement + a table on stderr (default: all)

  steady   n = 1 / 256 / 1024, launch and graph mode: StreamingEngine vs StaggeredStreamingEngine, every slot at T = 40
  rows     forward_rows (rows = 39) vs forward_last at B = 1 / 24 / 256 / 1024, T = 40 (bit-identical outputs checked)
  churn    1024 slots, 10 re-attached every frame (attach launch included) vs the same engine without churn
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tip_amd  # noqa: E402
from tip_amd import synth  # noqa: E402

BLOCKS, PER_BLOCK = 6, 30


def model():
    cfg = synth.PAPER
    m = tip_amd.TF_RNN_Past_State(cfg["input_size_imu"], cfg["size_s"], rnn_hid_size=cfg["rnn_hid_size"], tf_hid_size=cfg["tf_hid_size"],
                                  tf_in_dim=cfg["tf_in_dim"], n_heads=cfg["n_heads"], tf_layers=cfg["tf_layers"], dropout=0.0,
                                  in_dropout=0.0, past_state_dropout=0.0, with_rnn=True, with_acc_sum=True)
    m.load_state_dict({k: torch.tensor(v) for k, v in synth.make_weights(cfg, seed=0).items()})
    m = m.cuda().eval()
    m.freeze_packed(True)
    return m


def frames(n, seed):
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(seed)
    base = Rotation.random(n * 6, random_state=seed).as_matrix().reshape(n, 54).astype(np.float32)
    return [torch.tensor(np.concatenate([base, rng.randn(n, 18).astype(np.float32) * 0.5], axis=1)).cuda() for _ in range(8)], \
        (rng.randn(n, 114) * 0.2).astype(np.float32)


def block(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        fn(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e3


def alternate(arms, k=PER_BLOCK):
    """arms: {tag: fn(i)}; warm-up block each, then BLOCKS rounds alternating; best block per arm (ms per call)."""
    for fn in arms.values():
        block(fn, 8)
    best = {t: 1e9 for t in arms}
    for _ in range(BLOCKS):
        for t, fn in arms.items():
            best[t] = min(best[t], block(fn, k))
    return best


def emit(rec):
    print(json.dumps(rec), flush=True)


def main():
    torch.backends.cudnn.benchmark = False
    parts = [a for a in sys.argv[1:] if a in ("steady", "rows", "churn")] or ["steady", "rows", "churn"]
    m = model()
    rows_out = []
    for n in ((1, 256, 1024) if "steady" in parts else ()):
        fr, s_init = frames(n, n)
        for graph in (False, True):
            lock = tip_amd.streaming.StreamingEngine(m, s_init, use_graph=graph)
            stag = tip_amd.streaming.StaggeredStreamingEngine(m, s_init, use_graph=graph)
            for f in range(50):                       # past the warm-up: every window at T = 40 in both
                a = lock.step(fr[f % 8])
                b = stag.step(fr[f % 8])
            torch.cuda.synchronize()
            diff = float((a["y_last"] - b["y_last"]).abs().max())
            ok = bool(b["valid"].all()) and int(b["T"].min()) == 40
            res = alternate({"lockstep": lambda i: lock.step(fr[i % 8]), "staggered": lambda i: stag.step(fr[i % 8])})
            rec = {"what": "steady", "n": n, "graph": graph, "lockstep_ms": round(res["lockstep"], 4),
                   "staggered_ms": round(res["staggered"], 4), "ratio": round(res["staggered"] / res["lockstep"], 4),
                   "delta_us": round((res["staggered"] - res["lockstep"]) * 1e3, 1), "all_T40": ok,
                   "max_abs_y_diff_after_50_frames": diff}
            emit(rec)
            rows_out.append(rec)
            del lock, stag
    for B in ((1, 24, 256, 1024) if "rows" in parts else ()):
        x_imu, x_s = synth.make_inputs(synth.PAPER, B, 40, seed=B)
        xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
        r39 = torch.full((B,), 39, dtype=torch.int32, device="cuda")
        with torch.no_grad():
            same = bool(torch.equal(m.forward_rows(xi, xs, r39), m.forward_last(xi, xs)))
            res = alternate({"forward_last": lambda i: m.forward_last(xi, xs), "forward_rows": lambda i: m.forward_rows(xi, xs, r39)})
        rec = {"what": "rows", "B": B, "forward_last_ms": round(res["forward_last"], 4), "forward_rows_ms": round(res["forward_rows"], 4),
               "ratio": round(res["forward_rows"] / res["forward_last"], 4),
               "delta_us": round((res["forward_rows"] - res["forward_last"]) * 1e3, 1), "bit_identical": same}
        emit(rec)
        rows_out.append(rec)
    n = 1024
    fr, s_init = frames(n, 7)
    for graph in ((False, True) if "churn" in parts else ()):
        steady = tip_amd.streaming.StaggeredStreamingEngine(m, s_init, use_graph=graph)
        churn = tip_amd.streaming.StaggeredStreamingEngine(m, s_init, use_graph=graph)
        for f in range(50):
            steady.step(fr[f % 8])
            churn.step(fr[f % 8])
        rng = np.random.RandomState(0)

        def churn_step(i):
            sl = [int(s) for s in rng.choice(n, 10, replace=False)]
            churn.attach(sl, s_init[sl])
            churn.step(fr[i % 8])
        res = alternate({"steady": lambda i: steady.step(fr[i % 8]), "churn": churn_step})
        torch.cuda.synchronize()
        rec = {"what": "churn", "n": n, "graph": graph, "steady_ms": round(res["steady"], 4), "churn_ms": round(res["churn"], 4),
               "ratio": round(res["churn"] / res["steady"], 4)}
        emit(rec)
        rows_out.append(rec)
        del steady, churn
    m.check_handoffs()
    for r in rows_out:
        print(r, file=sys.stderr)


if __name__ == "__main__":
    main()
