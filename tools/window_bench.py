"""Closed-loop frame time of StreamingEngine at window lengths other than the paper's 40, and the ingest / consume kernels alone.

    python tools/window_bench.py [--windows 20,40,80] [--streams 1,256] [--root DIR] [--label NAME]
        -> one JSON line per (streams, graph) with ms per frame at every window, one per (streams, window) with the two kernels' us

Paper model, synthetic weights.  Closed loop: tools/staggered_bench.py's protocol (every engine past its warm-up, so every window is
full; a warm-up block per arm, then best of 6 blocks of 30 frames, the windows alternating block by block), launch by launch and as
a HIP graph.  Kernels: 200 back-to-back tip_stream_ingest(_w) (full windows) resp. tip_stream_consume(_w) calls between two events on
a buffer that went through W + 10 real frames, best of 5 — the time a kernel takes in a busy queue, launch gaps included.
--root DIR measures another checkout of this project (an A/B against an older commit in the same session: a checkout without the
window keyword is measured at 40 only); --label tags the lines.  profiles/window/window_bench.txt holds the recorded runs."""
import argparse
import json
import os
import sys

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", default="20,40,80")
    ap.add_argument("--streams", default="1,256")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    import tip_amd
    from tip_amd import lib as tlib
    from staggered_bench import frames, alternate, model

    has_w = "tip_stream_ingest_w" in tlib.EXPORTS
    windows = [w for w in (int(x) for x in a.windows.split(",")) if has_w or w == 40]
    m = model()
    L = tlib.load()
    for n in (int(x) for x in a.streams.split(",")):
        fr, s_init = frames(n, n)
        for graph in (False, True):
            engs = {w: tip_amd.streaming.StreamingEngine(m, s_init, use_graph=graph, **({"window": w} if has_w else {})) for w in windows}
            for w, e in engs.items():
                for f in range(w + 10):                   # past the warm-up (and, with graph, past the capture at frame w + 4)
                    e.step(fr[f % 8])
            torch.cuda.synchronize()
            res = alternate({w: (lambda i, e=e: e.step(fr[i % 8])) for w, e in engs.items()})
            print(json.dumps({"what": "closed_loop", "label": a.label, "n": n, "graph": graph,
                              **{f"W{w}_ms": round(v, 4) for w, v in res.items()}}), flush=True)
            if not graph:
                for w, e in engs.items():
                    print(json.dumps({"what": "kernels", "label": a.label, "n": n, "W": w, **kernel_us(L, e, fr[0], w, has_w)}), flush=True)
            del engs
    m.check_handoffs()


def kernel_us(L, eng, raw, W, has_w, calls=200, repeats=5):
    """us per ingest (TIP_STREAM_FRAME_AUTO: full windows) and per consume (the same row again and again) on the engine's own buffers;
    the engine is not used afterwards."""
    st = torch.cuda.current_stream().cuda_stream
    y = torch.zeros(eng.n, eng.ns, device="cuda")
    y[:, 0:108:6] = 1.0                                   # a finite pose (first column of every joint's 6D block)
    y[:, 3:108:6] = 1.0
    tail = (W, st) if has_w else (st,)
    ingest = L.tip_stream_ingest_w if has_w else L.tip_stream_ingest
    consume = L.tip_stream_consume_w if has_w else L.tip_stream_consume

    def run(fn):
        best = 1e9
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                assert fn() == 0
            e1.record()
            torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e3 / calls)
        return round(best, 2)

    S = eng.state.data_ptr()
    return {"ingest_us": run(lambda: ingest(S, raw.data_ptr(), eng.n, -1, eng.x_imu.data_ptr(), eng.x_s.data_ptr(), *tail)),
            "consume_us": run(lambda: consume(S, y.data_ptr(), eng.n, -1, eng.s_rest.data_ptr(), eng.c_t.data_ptr(), *tail))}


if __name__ == "__main__":
    main()
