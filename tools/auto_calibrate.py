#!/usr/bin/env python3
"""AUTO's decisions against the box it runs on (the plan selection in csrc/tip_schedule.hip is a cost model in absolute
microseconds, calibrated on one MI355X at one clock).

  python tools/auto_calibrate.py            the 64-batch sweep: AUTO's step time next to every explicit plan that serves the batch;
                                            flags AUTO > 1.10 x the best explicit plan and B1 < B2 with t(B1) > 1.10 x t(B2)
  python tools/auto_calibrate.py --stages   the stage costs the model is built from, re-measured through TIP_OPT_PROFILE = 1
                                            (encoder round of the one- / two-window kernels, window-split encoder on four / two CUs,
                                            recurrence + projection per round, the few-stream plan for 1 .. 44 windows) next to the
                                            constants in csrc/tip_schedule.hip

`sweep()` is what tests/test_auto_model_gpu.py runs."""
import contextlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch

SIZES = sorted(set([1, 2, 8, 9, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257, 258, 287, 288, 289, 300, 319, 320, 321,
                    383, 384, 385, 400, 511, 512, 513, 545, 600, 767, 768, 769, 801, 1000, 1023, 1024, 1025, 1056, 1057, 1064, 1088, 1089,
                    1152, 1153, 1279, 1280, 1281, 1500, 2047, 2048, 2049, 2081, 2112, 2113, 2200]))
TOL = 1.10


def candidates(B, ncu):
    """Explicit single-sequence plans that serve B windows of 40 frames (what AUTO chooses among; its rounds + remainder split has no name)."""
    c = ["fusedh"]
    if B >= 2:
        c.append("fused2")
    if B <= 64:
        c.append("latency")
    if 4 * B <= ncu and B <= 64:
        c.append("fused1s4")
    if 2 * B <= ncu and B <= 128:
        c.append("fused1s2")
    return c


def step_us(m, xi, xs, n):
    with torch.no_grad():
        for _ in range(5):
            m(xi, xs)
        torch.cuda.synchronize()
        best = 1e30
        for _ in range(3):                      # best of three loops: a loop can catch a clock dip or a neighbour's burst
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                m(xi, xs)
            e1.record(); e1.synchronize()
            best = min(best, e0.elapsed_time(e1) / n * 1e3)
    return best


def sweep(m, sizes=SIZES, with_candidates=True, log=None):
    """-> (rows, violations).  rows: (B, auto_us, {plan: us}); violations: human-readable strings."""
    from tip_amd import synth
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    x_imu, x_s = synth.make_inputs(synth.PAPER, 256, 40, seed=4242)
    rows, bad = [], []
    for B in sizes:
        reps = (B + 255) // 256
        xi = torch.tensor(np.tile(x_imu, (reps, 1, 1))[:B]).cuda()
        xs = torch.tensor(np.tile(x_s, (reps, 1, 1))[:B]).cuda()
        n = 60 if B <= 300 else (25 if B <= 1200 else 12)
        m.set_plan("auto")
        ta = step_us(m, xi, xs, n)
        alt = {}
        if with_candidates:
            for p in candidates(B, ncu):
                m.set_plan(p)
                alt[p] = step_us(m, xi, xs, n)
            m.set_plan("auto")
            best = min(alt, key=alt.get)
            if ta > TOL * alt[best]:
                bad.append(f"B={B}: AUTO {ta:.0f} us, plan '{best}' {alt[best]:.0f} us ({ta / alt[best]:.2f}x)")
        rows.append((B, ta, alt))
        if log:
            log(f"B={B:5d}: AUTO {ta:8.1f} us   " + "  ".join(f"{p} {t:8.1f}" for p, t in alt.items()))
    for (b1, t1, _), (b2, t2, _) in zip(rows, rows[1:]):
        if t1 > TOL * t2:
            bad.append(f"B={b1} takes {t1:.0f} us but B={b2} only {t2:.0f} us: a decision boundary sits in the wrong place")
    return rows, bad


def stages(m):
    """The model's ingredients, measured: per-stage event times of one forward (TIP_OPT_PROFILE = 1), median of 15."""
    from tip_amd import synth
    x_imu, x_s = synth.make_inputs(synth.PAPER, 256, 40, seed=4242)

    def run(plan, B):
        reps = (B + 255) // 256
        xi = torch.tensor(np.tile(x_imu, (reps, 1, 1))[:B]).cuda()
        xs = torch.tensor(np.tile(x_s, (reps, 1, 1))[:B]).cuda()
        acc = {}
        with torch.no_grad():
            m.set_plan(plan)
            for _ in range(5):
                m(xi, xs)
            for _ in range(15):
                m.set_plan(plan, profile=1)
                m(xi, xs)
                torch.cuda.synchronize()
                for name, ms, k in m.profile_read():
                    acc.setdefault(name, []).append(ms * 1e3)
        m.set_plan("auto")
        return {k: float(np.median(v)) for k, v in acc.items()}

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    out = []
    a = run("fusedh", ncu); out.append(("one-window encoder, one round of #CUs windows", 527, a.get("fused_encoder")))
    out.append(("recurrence + projection behind one round", 96, (a.get("rnn_recurrence", 0) + a.get("out_linear", 0))))
    a = run("fused2", 2 * ncu); out.append(("two-window encoder, one round of 2 x #CUs windows", 1049, a.get("fused_encoder")))
    a = run("fused1s4", ncu // 4); out.append(("window-split encoder on four CUs (whole forward, AUTO's 305)", 305, sum(a.values())))
    out.append(("  ... its encoder alone (232 in the merge rule)", 232, a.get("fused_encoder")))
    a = run("fused1s2", ncu // 2); out.append(("window-split encoder on two CUs (whole forward, AUTO's 452)", 452, sum(a.values())))
    out.append(("  ... its encoder alone (375 in the merge rule)", 375, a.get("fused_encoder")))
    for r in (1, 8, 16, 24, 32, 44):
        model = 147 + r // 4 if r <= 8 else (181 if r <= 16 else (241 if r <= 24 else (200 + (r - 8) * 3.6 if r <= 32 else 286 + 10 * (r - 32))))
        out.append((f"few-stream plan, {r} windows (whole forward)", round(model), sum(run("latency", r).values())))
    return out


if __name__ == "__main__":
    os.environ.setdefault("TIP_LIB", "measure")
    import tip_amd
    from tip_amd import synth
    with contextlib.redirect_stdout(sys.stderr):
        m = tip_amd.TF_RNN_Past_State(72, 131, rnn_hid_size=512, tf_hid_size=1024, tf_in_dim=256, n_heads=16, tf_layers=4,
                                      dropout=0.0, in_dropout=0.0, past_state_dropout=0.0, with_acc_sum=True)
    m.load_state_dict({k: torch.tensor(v) for k, v in synth.make_weights(synth.PAPER, seed=0).items()})
    m = m.cuda().eval()
    if "--stages" in sys.argv:
        print(f"{'ingredient of the AUTO cost model (csrc/tip_schedule.hip)':68s} {'model us':>9s} {'here us':>9s}  ratio")
        for name, const, meas in stages(m):
            print(f"{name:68s} {const:9.0f} {meas:9.1f}  {meas / const:5.2f}")
    else:
        rows, bad = sweep(m, log=print)
        print(f"{len(rows)} batch sizes, {len(bad)} decision(s) off by more than {int((TOL - 1) * 100)} %")
        for b in bad:
            print("  ", b)
    m.check_handoffs()
