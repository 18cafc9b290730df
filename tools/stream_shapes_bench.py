"""Closed-loop frame time of the streaming engines at the model shapes they serve, all shapes in ONE run, alternating in blocks
(tools/staggered_bench.py's protocol: a warm-up block per arm, then best of 6 blocks of 30 frames): ms per frame at 1, 256 and 1024
streams, lock-step and staggered, launch by launch and HIP graph.

    python tools/stream_shapes_bench.py [n ...]        -> one JSON line per (streams, engine, graph) + a table on stderr

Shapes: x_imu / x_s columns 90 / 131 (the paper's model), 72 / 131 (no acc-sum), 90 / 119 (two SBPs), 72 / 119 (both)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tip_amd  # noqa: E402
from tip_amd import synth  # noqa: E402
from staggered_bench import frames, alternate  # noqa: E402

SHAPES = {"90x131": dict(synth.PAPER), "72x131": dict(synth.PAPER, with_acc_sum=False), "90x119": dict(synth.PAPER, size_s=119),
          "72x119": dict(synth.PAPER, size_s=119, with_acc_sum=False)}


def model_for_cfg(cfg):
    m = tip_amd.TF_RNN_Past_State(cfg["input_size_imu"], cfg["size_s"], rnn_hid_size=cfg["rnn_hid_size"], tf_hid_size=cfg["tf_hid_size"],
                                  tf_in_dim=cfg["tf_in_dim"], n_heads=cfg["n_heads"], tf_layers=cfg["tf_layers"], dropout=0.0,
                                  in_dropout=0.0, past_state_dropout=0.0, with_rnn=True, with_acc_sum=cfg["with_acc_sum"])
    m.load_state_dict({k: torch.tensor(v) for k, v in synth.make_weights(cfg, seed=0).items()})
    m = m.cuda().eval()
    m.freeze_packed(True)
    return m


def main():
    ns = [int(a) for a in sys.argv[1:]] or [1, 256, 1024]
    models = {tag: model_for_cfg(cfg) for tag, cfg in SHAPES.items()}
    out = []
    for n in ns:
        fr, s_init = frames(n, n)
        for kind, Engine in (("lockstep", tip_amd.streaming.StreamingEngine), ("staggered", tip_amd.streaming.StaggeredStreamingEngine)):
            for graph in (False, True):
                engs = {tag: Engine(m, s_init, use_graph=graph) for tag, m in models.items()}
                for f in range(50):                       # past the warm-up: every window at T = 40
                    for e in engs.values():
                        e.step(fr[f % 8])
                torch.cuda.synchronize()
                res = alternate({tag: (lambda i, e=e: e.step(fr[i % 8])) for tag, e in engs.items()})
                rec = {"what": "shapes", "n": n, "engine": kind, "graph": graph, **{tag + "_ms": round(v, 4) for tag, v in res.items()}}
                print(json.dumps(rec), flush=True)
                out.append(rec)
                del engs
    for m in models.values():
        m.check_handoffs()
    for r in out:
        print(r, file=sys.stderr)


if __name__ == "__main__":
    main()
