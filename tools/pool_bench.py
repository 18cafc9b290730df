"""Compact staggered pools (StaggeredStreamingEngine(compact=True)) against plain staggered engines sized for the load, both arms in
ONE run, alternating in blocks, a warm-up for every shape; ms per closed-loop frame (best of the blocks).

    python tools/pool_bench.py [sizes] [churn] [--launch]   -> one JSON line per measurement + a table on stderr (default: both, graph mode)

  sizes   a 1024-slot compact pool with k in {1, 8, 24, 64, 200, 256, 300, 700, 1024} attached vs a plain engine with n = k
          (k = 1024: vs the plain 1024-slot engine)
  churn   1024-slot compact pool at k = 512, prewarmed: 10 slots detached and 10 attached per frame vs the same pool without churn;
          the capture counter must not move
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
from staggered_bench import model, frames, alternate, emit  # noqa: E402

N = 1024
KS = (1, 8, 24, 64, 200, 256, 300, 700, 1024)


def main():
    torch.backends.cudnn.benchmark = False
    parts = [a for a in sys.argv[1:] if a in ("sizes", "churn")] or ["sizes", "churn"]
    graph = "--launch" not in sys.argv
    m = model()
    fr, s_init = frames(N, 3)
    out = []
    Engine = tip_amd.streaming.StaggeredStreamingEngine
    for k in (KS if "sizes" in parts else ()):
        pool = Engine(m, s_init, use_graph=graph, compact=True)
        pool.detach(range(k, N))
        plain = Engine(m, s_init[:k], use_graph=graph)
        frk = [f[:k].contiguous() for f in fr]
        for f in range(50):                       # past the warm-up: every attached window at T = 40 in both
            a = pool.step(fr[f % 8])
            b = plain.step(frk[f % 8])
        torch.cuda.synchronize()
        same = bool(torch.equal(a["valid"][:k], b["valid"])) and bool(a["valid"][:k].all())
        diff = float((a["y_last"][:k] - b["y_last"]).abs().max())
        res = alternate({"plain": lambda i: plain.step(frk[i % 8]), "compact": lambda i: pool.step(fr[i % 8])})
        rec = {"what": "sizes", "n": N, "k": k, "batch": a["batch"], "graph": graph, "plain_ms": round(res["plain"], 4),
               "compact_ms": round(res["compact"], 4), "ratio": round(res["compact"] / res["plain"], 4),
               "delta_us": round((res["compact"] - res["plain"]) * 1e3, 1), "all_valid": same, "max_abs_y_diff_after_50_frames": diff}
        emit(rec)
        out.append(rec)
        del pool, plain
    if "churn" in parts:
        k = 512
        steady = Engine(m, s_init, use_graph=graph, compact=True)
        churn = Engine(m, s_init, use_graph=graph, compact=True)
        for e in (steady, churn):
            e.detach(range(k, N))
            e.prewarm()
        for f in range(50):
            steady.step(fr[f % 8])
            churn.step(fr[f % 8])
        rng = np.random.RandomState(0)
        c0 = churn.captures

        def churn_step(i):
            det = [int(s) for s in rng.choice(churn.positions, 10, replace=False)]
            churn.detach(det)
            attached = churn.attached
            free = [s for s in range(N) if not attached[s]]
            att = [int(s) for s in rng.choice(free, 10, replace=False)]
            churn.attach(att, s_init[att])
            churn.step(fr[i % 8])
        res = alternate({"steady": lambda i: steady.step(fr[i % 8]), "churn": churn_step})
        torch.cuda.synchronize()
        rec = {"what": "churn", "n": N, "k": k, "graph": graph, "steady_ms": round(res["steady"], 4), "churn_ms": round(res["churn"], 4),
               "ratio": round(res["churn"] / res["steady"], 4), "captures_during_churn": churn.captures - c0,
               "active": len(churn.positions)}
        emit(rec)
        out.append(rec)
        del steady, churn
    m.check_handoffs()
    for r in out:
        print(r, file=sys.stderr)


if __name__ == "__main__":
    main()
