"""The deployed model (past_state_dropout = 0.8, never .eval()) behind the streaming engines: live_dropout=True against what the engines
do without the keyword, every arm of a comparison in ONE process, alternating in blocks after a warm-up; medians over >= 200 frames.

    python tools/live_bench.py [frame] [eval] [stage] [--out FILE]    -> one JSON line per measurement; the table to FILE (and stderr)
    python tools/live_bench.py kernels                                -> only runs the three encoder instantiations at B = 256, 60 calls
                                                                         each (for tools/kstats.sh: rocprofv3 kernel medians)

  frame   .train() model, 1 / 256 / 1024 streams, every window at T = 40.  Arm A: StreamingEngine without the keyword (training forward:
          all rows, activation stash, no graph), run as TWO engines A and A' — their distance is the spread of a repeated arm.  Arm B:
          live_dropout=True, launch by launch and with use_graph=True.
  eval    .eval() model, 1024 streams: keyword off (torch.rand_like mask + inference forward) against on (mask drawn in the kernel)
  stage   fused_encoder stage (TIP_OPT_PROFILE, device events) at B = 256: inference and live instantiations
"""
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tip_amd  # noqa: E402
from tip_amd import synth  # noqa: E402
from tip_amd.streaming import StreamingEngine  # noqa: E402

BLOCKS, PER_BLOCK = 8, 30          # 240 timed frames per arm
P_STATE = 0.8


def model(train, p_state=P_STATE):
    cfg = synth.PAPER
    m = tip_amd.TF_RNN_Past_State(cfg["input_size_imu"], cfg["size_s"], rnn_hid_size=cfg["rnn_hid_size"], tf_hid_size=cfg["tf_hid_size"],
                                  tf_in_dim=cfg["tf_in_dim"], n_heads=cfg["n_heads"], tf_layers=cfg["tf_layers"], dropout=0.0,
                                  in_dropout=0.0, past_state_dropout=p_state, with_rnn=True, with_acc_sum=True)
    m.load_state_dict({k: torch.tensor(v) for k, v in synth.make_weights(cfg, seed=0).items()})
    m = m.cuda()
    return m.train() if train else m.eval()


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


def alternate(arms):
    """arms: {tag: fn(i)}; a warm-up block each, then BLOCKS rounds alternating -> {tag: (median, min, max)} of the block means (ms / frame)."""
    for fn in arms.values():
        block(fn, 10)
    t = {tag: [] for tag in arms}
    for _ in range(BLOCKS):
        for tag, fn in arms.items():
            t[tag].append(block(fn, PER_BLOCK))
    return {tag: (statistics.median(v), min(v), max(v)) for tag, v in t.items()}


def engines(m, s_init, specs, fr):
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for tag, kw in specs.items():
            torch.manual_seed(1)
            e = out[tag] = StreamingEngine(m, s_init, **kw)
            for f in range(50):                    # past the warm-up and the capture frame: every window at T = 40
                o = e.step(fr[f % 8])
            torch.cuda.synchronize()
            assert o["T"] == 40 and bool(torch.isfinite(o["y_last"]).all()), tag
    return out


def run(specs, m, n, what, lines, emit):
    fr, s_init = frames(n, n)
    eng = engines(m, s_init, specs, fr)
    res = alternate({tag: (lambda i, e=e: e.step(fr[i % 8])) for tag, e in eng.items()})
    rec = {"what": what, "n": n, "frames_per_arm": BLOCKS * PER_BLOCK}
    for tag, (med, lo, hi) in res.items():
        rec[tag + "_ms"] = round(med, 4)
        rec[tag + "_min_max_ms"] = [round(lo, 4), round(hi, 4)]
        lines.append(f"{what:6s} n={n:5d}  {tag:22s} median {med:8.4f} ms/frame   blocks {lo:8.4f} .. {hi:8.4f}")
    emit(rec)
    m.check_handoffs()
    return res


def stage_us(m, fn, name, plan, calls=60):
    m.set_plan(plan, profile=1)
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    m.set_plan(plan, profile=1)                   # (re-arming the profile resets its accumulators)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    st = {k: (ms_, n_) for k, ms_, n_ in m.profile_read()}
    m.set_plan(plan, profile=0)
    ms_, n_ = st[name]
    return ms_ / n_ * 1e3, {k: round(v[0] / v[1] * 1e3, 1) for k, v in st.items()}


def three_forwards(B=256):
    """(inference, live, training) forwards at B windows of T = 40 on the one-window hybrid encoder."""
    x_imu, x_s = synth.make_inputs(synth.PAPER, B, 40, seed=B)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    mi = model(False, 0.0)
    mi.set_plan("fusedh")
    ml, mt = model(True), model(True)
    mt.keep_train_stash = True

    def inference():
        with torch.no_grad():
            return mi.forward_last(xi, xs)
    return mi, ml, mt, inference, (lambda: ml.forward_live(xi, xs)), (lambda: mt(xi, xs))


def main():
    args = sys.argv[1:]
    out_path = args[args.index("--out") + 1] if "--out" in args else None
    parts = [a for a in args if a in ("frame", "eval", "stage", "kernels")] or ["frame", "eval", "stage"]
    assert torch.cuda.is_available(), "live_bench measures on an MI355X; there is no CPU fallback"
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)

    if "kernels" in parts:
        _, _, _, inf, live, train = three_forwards()
        for fn in (inf, live, train):
            for _ in range(60):
                fn()
            torch.cuda.synchronize()
        return
    if "frame" in parts:
        m = model(True)
        for n in (1, 256, 1024):
            res = run({"A_train_forward": {}, "A_repeat": {}, "B_live_launch": {"live_dropout": True},
                       "B_live_graph": {"live_dropout": True, "use_graph": True}}, m, n, "frame", lines, emit)
            a, a2 = res["A_train_forward"][0], res["A_repeat"][0]
            spread = max(abs(a - a2), res["A_train_forward"][2] - res["A_train_forward"][1], res["A_repeat"][2] - res["A_repeat"][1])
            for tag in ("B_live_launch", "B_live_graph"):
                b = res[tag][0]
                lines.append(f"frame  n={n:5d}  {tag} is {min(a, a2) - b:+.4f} ms/frame against arm A ({min(a, a2) / b:.2f}x); "
                             f"spread of arm A (A vs A', block min..max) {spread:.4f} ms -> "
                             f"{'FASTER beyond the spread' if min(a, a2) - b > spread else 'NOT faster beyond the spread'}")
    if "eval" in parts:
        m = model(False)
        run({"off_rand_like_launch": {}, "on_in_kernel_launch": {"live_dropout": True}, "off_rand_like_graph": {"use_graph": True},
             "on_in_kernel_graph": {"live_dropout": True, "use_graph": True}}, m, 1024, "eval", lines, emit)
    if "stage" in parts:
        mi, ml, _, inf, live, _ = three_forwards()
        for tag, mm, fn, plan in (("inference", mi, inf, "fusedh"), ("live", ml, live, "auto")):
            us, allst = stage_us(mm, fn, "fused_encoder", plan)
            emit({"what": "stage", "B": 256, "instantiation": tag, "fused_encoder_us": round(us, 1), "stages_us": allst})
            lines.append(f"stage  B=  256  fused_encoder ({tag:9s}) {us:8.1f} us per call (TIP_OPT_PROFILE, device events); all stages {allst}")
        lines.append("stage  B=  256  training instantiation: tip_train_forward has no profile stages — kernel medians come from "
                     "`tools/kstats.sh live -- python tools/live_bench.py kernels` (rocprofv3, a run of its own)")
    text = "\n".join(lines) + "\n"
    sys.stderr.write(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
