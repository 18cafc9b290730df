#!/usr/bin/env python3
"""Output bits of the streaming engines as one line, for comparing two trees' host code (or two library builds, TIP_LIB=<path>.so) on
one machine: sha256 prefixes over every frame's s_rest, c_t, y_last (and T / valid where the engine returns them).

    python tools/stream_digest.py [--tree DIR] [--frames 100] [--streams 1,256,1024] [--window 40]   -> DIGEST {...}   (sorted keys;
                                                                                                        compare with cmp)
  --tree DIR   the directory whose tip_amd.py is imported (default: this file's own tree)
  --window W   the window length of every engine (default 40, the 40-row kernels; any other length runs the _w kernels and leaves
               the reuse engine out, whose ring holds 40-frame windows)

Per model shape — the paper's (90, 131) and (72, 119) — and per source — the committed runner trace (tests/golden/tip_runner_golden.npz:
2 streams, 70 frames) and a random closed loop of --frames frames at each stream count: lock-step launch / graph / reuse, staggered
and compact pools launch / graph.  Beyond one stream the staggered engines see an attach or a detach every 9th frame (a few slots
leave, and come back nine frames later with a new s_init); every loop calls override_history once, half way.  Nothing is injected
and no option is set."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def model_for(tip_amd, synth, cfg):
    m = tip_amd.TF_RNN_Past_State(cfg["input_size_imu"], cfg["size_s"], rnn_hid_size=cfg["rnn_hid_size"], tf_hid_size=cfg["tf_hid_size"],
                                  tf_in_dim=cfg["tf_in_dim"], n_heads=cfg["n_heads"], tf_layers=cfg["tf_layers"], dropout=0.0,
                                  in_dropout=0.0, past_state_dropout=0.0, with_rnn=True, with_acc_sum=cfg["with_acc_sum"])
    m.load_state_dict({k: torch.tensor(v) for k, v in synth.make_weights(cfg, seed=0).items()})
    return m.cuda().eval()


def random_loop(n, frames):
    """raw [frames, n, 72]: six fixed random rotations per stream (row-major) + 18 random accelerations per frame; s_init [n, 114]."""
    rng = np.random.RandomState(1000 + n)
    q, _ = np.linalg.qr(rng.randn(n * 6, 3, 3))
    q = q * np.sign(np.linalg.det(q))[:, None, None]
    rot = np.broadcast_to(q.reshape(1, n, 54), (frames, n, 54))
    raw = np.concatenate([rot, rng.randn(frames, n, 18) * 0.5], axis=2).astype(np.float32)
    return raw, (rng.randn(n, 114) * 0.2).astype(np.float32)


def runner_trace(tree):
    z = np.load(os.path.join(tree, "tests", "golden", "tip_runner_golden.npz"))
    raw = np.stack([z["stream0/raw_imu"], z["stream1/raw_imu"]], axis=1).astype(np.float32)[:70]
    return raw, np.stack([z["stream0/s_init"], z["stream1/s_init"]]).astype(np.float32)


def run(eng, raw, s_init, staggered):
    """The loop's digests: {name: 16 hex digits}."""
    frames, n = raw.shape[0], raw.shape[1]
    rng = np.random.RandomState(7 * n + frames)
    hashes = {}
    out_of_loop = []
    for f in range(frames):
        if staggered and n > 1 and f and f % 9 == 0:
            if out_of_loop:
                eng.attach(out_of_loop, (rng.randn(len(out_of_loop), 114) * 0.2).astype(np.float32))
                out_of_loop = []
            else:
                out_of_loop = sorted(int(s) for s in rng.choice(np.arange(1, n), min(n - 1, max(1, n // 10)), replace=False))
                eng.detach(out_of_loop)
        out = eng.step(torch.tensor(raw[f]).cuda())
        for name in ("s_rest", "c_t", "y_last", "T", "valid"):
            h = hashes.setdefault(name, hashlib.sha256())
            v = None if out is None else out.get(name)
            h.update(v.cpu().numpy().tobytes() if isinstance(v, torch.Tensor) else repr(v).encode())
        if f == frames // 2:                  # slot 0 is never detached: it has consumed a frame in every engine by now
            eng.override_history((rng.randn(1 if staggered else n, 54) * 0.3).astype(np.float32), [0] if staggered else None)
    torch.cuda.synchronize()
    return {k: h.hexdigest()[:16] for k, h in hashes.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--streams", default="1,256,1024")
    ap.add_argument("--window", type=int, default=40)
    a = ap.parse_args()
    W = a.window
    tree = os.path.abspath(a.tree)
    sys.path.insert(0, tree)
    import tip_amd
    from tip_amd import synth, streaming as S
    paper = dict(synth.PAPER)
    loops = {"trace": runner_trace(tree)}
    for n in (int(s) for s in a.streams.split(",")):
        loops[f"n{n}"] = random_loop(n, a.frames)
    kw = {} if W == 40 else {"window": W}          # (a --tree from before the window keyword still runs at 40)
    engines = {"lock_launch": lambda m, s: S.StreamingEngine(m, s, **kw),
               "lock_graph": lambda m, s: S.StreamingEngine(m, s, use_graph=True, **kw),
               "lock_reuse": lambda m, s: S.StreamingEngine(m, s, reuse=True),
               "stag_launch": lambda m, s: S.StaggeredStreamingEngine(m, s, **kw),
               "stag_graph": lambda m, s: S.StaggeredStreamingEngine(m, s, use_graph=True, **kw),
               "pool_launch": lambda m, s: S.StaggeredStreamingEngine(m, s, compact=True, **kw),
               "pool_graph": lambda m, s: S.StaggeredStreamingEngine(m, s, use_graph=True, compact=True, **kw)}
    if W != 40:
        del engines["lock_reuse"]                  # the reuse ring holds 40-frame windows
    digest = {}
    for shape, cfg in (("90x131", paper), ("72x119", dict(paper, size_s=119, with_acc_sum=False))):
        m = model_for(tip_amd, synth, cfg)
        for src, (raw, s_init) in loops.items():
            for kind, make in engines.items():
                digest[f"{shape}/{src}/{kind}"] = run(make(m, s_init), raw, s_init, kind[:4] != "lock")
        m.check_handoffs()
    print("DIGEST " + json.dumps(digest, sort_keys=True), flush=True)


if __name__ == "__main__":
    main()
