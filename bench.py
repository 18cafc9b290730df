#!/usr/bin/env python3
"""bench.py — IMU frames/s of the TIP forward pass on N MI355X GPUs (BASELINE.json metric).

One "step" = one forward of TF_RNN_Past_State over a batch of B synthetic IMU windows per GPU, inputs resident in HBM.
In streaming, one window forward consumes one new IMU frame per stream, so frames/s == windows/s.
Streams shard on the batch axis (weak scaling, no data-path collective; one RCCL weight broadcast before the timed
region).  --config selects which BASELINE.json configuration is the headline of the run:

    paper256     configs[1]: batch 256 / GPU, seq_len 40, paper model, full [B,T,131] output           (default)
    streams1024  configs[2]/[3]: 1024 concurrent streams / GPU, seq_len 40, last-row output (what RTRunnerMin.step consumes)
    scaled512    configs[4]: 12 layers, d=1024, ffn=4096, seq_len 80, batch 512 / GPU (4096 over 8 GPUs), full output

    python bench.py --gpus 1 --steps 50 --warmup 10 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W [--config streams1024]

A plain run sets up, warms up, times the K steps and prints the headline line; --dump-outputs DIR also writes the last timed
step's output to DIR/y.npy (float32).  Everything else is measured only with --full: the cross-rank self-checks (packed image
and probe-window outputs identical on every rank), north_star's table on this run's N GPUs (`extra.scaling_table`), the CPU
baseline and, at N = 1, every other BASELINE configuration on the same clock (`extra.configs`: B=1 latency with and without
the PCIe hops, 1024 closed-loop streams, B=1024 last-row, B=8192, the scaled model) and the headline step held for >= 3 s
(`extra.sustained`) so that the clock actually held is known.
"""
import argparse
import contextlib
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The host driver of this pool only supports dmabuf IPC: without this RCCL's intra-node transport fails with
# `hipIpcGetMemHandle: invalid argument` as soon as a second rank exists.  Set before HIP / RCCL initialise.
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import tip_amd  # noqa: E402
from tip_amd import synth  # noqa: E402
from tip_amd import dist as tdist  # noqa: E402
from tip_amd import lib as tlib  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 / 16x16x4_f32, dense, 2.4 GHz
PEAK_CLOCK_GHZ = 2.4
PEAK_HBM_GBS = 8000.0

CONFIGS = {
    "paper256": dict(cfg=synth.PAPER, B=256, T=40, last=False,
                     metric="IMU frames/sec (whole node), seq_len=40 batch=256/GPU",
                     workload="TIP paper config (4 layers, 16 heads, d=256, ffn=1024, rnn=512), {B} windows/GPU x {T} frames, "
                              "full [B,T,131] output, inputs resident in HBM"),
    "streams1024": dict(cfg=synth.PAPER, B=1024, T=40, last=True,
                        metric="IMU frames/sec (whole node), 1024 concurrent streams/GPU, seq_len=40, last-row output",
                        workload="TIP paper config, {B} concurrent streams/GPU x {T}-frame sliding window, row T-1 only "
                                 "([B,131]: what RTRunnerMin.step consumes), inputs resident in HBM"),
    "scaled512": dict(cfg=synth.SCALED, B=512, T=80, last=False,
                      metric="IMU frames/sec (whole node), scaled model, seq_len=80 batch=512/GPU",
                      workload="scaled config (12 layers, 16 heads, d=1024, ffn=4096, rnn=512), {B} windows/GPU x {T} frames, "
                               "full [B,T,131] output, random-init weights, inputs resident in HBM"),
}


def build_model(cfg, seed, load):
    with contextlib.redirect_stdout(sys.stderr):   # the reference's constructor prints; stdout carries ONE JSON line
        m = tip_amd.TF_RNN_Past_State(
            cfg["input_size_imu"], cfg["size_s"], rnn_hid_size=cfg["rnn_hid_size"], tf_hid_size=cfg["tf_hid_size"],
            tf_in_dim=cfg["tf_in_dim"], n_heads=cfg["n_heads"], tf_layers=cfg["tf_layers"], dropout=0.0, in_dropout=0.0,
            past_state_dropout=0.0, with_rnn=cfg.get("with_rnn", True), with_acc_sum=cfg.get("with_acc_sum", False))
    if load:
        w = synth.make_weights(cfg, seed=seed)
        m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    return m


def stage_flops(cfg, name, B, T):
    """Algorithmic FLOPs of ONE launch of a stage ('Kernels')."""
    In = cfg["input_size_imu"] + cfg["size_s"] + (18 if cfg.get("with_acc_sum") else 0)
    D, F, L = cfg["tf_in_dim"], cfg["tf_hid_size"], cfg["tf_layers"]
    M = B * T
    if name == "fused_encoder":   # prologue + in_linear + L encoder layers + RNN input projection (fused at its tail)
        R = cfg["rnn_hid_size"]
        return B * (2.0 * T * In * D + L * (2.0 * T * D * 3 * D + 4.0 * T * T * D + 2.0 * T * D * D + 4.0 * T * D * F)
                    + 2.0 * T * D * R)
    if name in ("ffn1_gemm", "ffn2_gemm"):
        return 2.0 * M * D * F
    return None


def timed_loop(fn, iters):
    """ms per call over `iters` back-to-back calls (device time, events on the current stream)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def p50_latency_ms(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def output_digest(y):
    """Order-sensitive 2 x int64 digest of a float32 tensor's BITS (wrap-around arithmetic: identical bits <=> identical digest
    for all practical purposes; NaN payloads included)."""
    b = y.contiguous().view(torch.int32).reshape(-1).to(torch.int64)
    w = (torch.arange(b.numel(), device=b.device, dtype=torch.int64) % 65521) + 1
    return torch.stack([b.sum(), (b * w).sum()])


def probe_outputs(model, cfg, dev, T, batch_xi, batch_xs, last):
    """Self-check of the multi-GPU run (nobody can rehearse it): 4 seed-derived probe windows, IDENTICAL on every rank, are run
    (i) alone (whatever plan AUTO picks for 4 streams) and (ii) as the first 4 windows of this rank's own batch on the bench's
    plan.  Streams are independent and every rank holds rank 0's weights, so both outputs must be bit-identical on all ranks
    (north_star: no per-step cross-GPU dependency).  Returns a [4] int64 digest."""
    px, ps = synth.make_inputs(cfg, 4, T, seed=424242)
    px, ps = torch.tensor(px).to(dev), torch.tensor(ps).to(dev)
    y_alone = model(px, ps)
    xi2, xs2 = batch_xi.clone(), batch_xs.clone()
    n = min(4, xi2.shape[0])
    xi2[:n], xs2[:n] = px[:n], ps[:n]
    y_in = (model.forward_last(xi2, xs2) if last else model(xi2, xs2))[:n]
    torch.cuda.synchronize()
    return torch.cat([output_digest(y_alone), output_digest(y_in)])


DUMP_BYTES = 64_000_000   # --dump-outputs: at most this much in all, over every rank


def dump_outputs(out_dir, y, rank, world):
    """--dump-outputs: the last timed step's output as float32 .npy — DIR/y.npy (one rank) or DIR/y_rank<r>.npy.  Above the
    byte budget, a fixed sample of whole windows (seeded, sorted, the same for the same shape) stands in for the batch."""
    y = y.detach().float().cpu().numpy()
    budget = DUMP_BYTES // world
    if y.nbytes > budget:
        keep = max(1, budget // (y[0].nbytes or 1))
        y = y[np.sort(np.random.default_rng(0).choice(y.shape[0], keep, replace=False))]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "y.npy" if world == 1 else f"y_rank{rank}.npy"), np.ascontiguousarray(y))


def frac_of_peak(cfg, T, windows_per_s, n_gpus=1):
    return windows_per_s * synth.flops_per_window(cfg, T) / 1e12 / (PEAK_FP32_MFMA_TFLOPS * n_gpus)


def cpu_model_name():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.lower().startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    import platform
    return platform.processor() or platform.machine()


def cpu_baseline(cfg, B, T, budget_s=10.0):
    """The reference's CPU path on this box's host cores, bounded sample of the bench workload: the model built from STOCK
    torch.nn modules (oracle/torch_stock.py: nn.Linear / nn.TransformerEncoder / nn.RNN — the dispatch the reference takes;
    bit-identical to the reference's outputs on the golden vectors, tests/test_host_cpu.py).  Second figures: the module's
    torch-op restatement and the scalar C oracle."""
    from oracle import torch_stock
    w = synth.make_weights(cfg, seed=0)
    with contextlib.redirect_stdout(sys.stderr):
        stock = torch_stock.build(cfg, w)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=1234)
    xi, xs = torch.tensor(x_imu), torch.tensor(x_s)
    max_threads = torch.get_num_threads()

    sweep = {}

    def best_threads(fn):
        best, cores = None, 1
        for nt in sorted({1, 8, 16, 32, 64, max_threads}):
            if nt > max_threads:
                continue
            torch.set_num_threads(nt)
            fn()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            sweep[str(nt)] = round(B / dt, 1)
            if best is None or dt < best:
                best, cores = dt, nt
        torch.set_num_threads(cores)
        return cores

    def run_for(fn, budget, cap):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            el = time.perf_counter() - t0
            if el > budget or n >= cap:
                return n, el

    with torch.no_grad():
        f_stock = lambda: stock(xi, xs)   # noqa: E731
        cores = best_threads(f_stock)
        n, el = run_for(f_stock, budget_s, 40)
        out = {"value": B * n / el, "unit": "IMU frames/s", "cores": cores, "kind": "port",
               "cpu_model": cpu_model_name(), "logical_cpus": os.cpu_count(), "torch_default_threads": max_threads,
               "thread_sweep_frames_per_s": dict(sweep),   # one forward each: `cores` is the fastest entry, not the box's core count
               "sample": f"{n} forwards of B={B},T={T} (paper config) through stock torch.nn modules (nn.Linear, "
                         f"nn.TransformerEncoder, nn.RNN: the reference's CPU dispatch), best of 1/8/16/32/64/{max_threads} "
                         f"threads = {cores}, {el:.1f} s"}
        # the reference's own streaming setting: one stream, one thread (offline_testing_simple.py:34, real_time_runner_minimal.py:149)
        torch.set_num_threads(1)
        x1i, x1s = xi[:1].contiguous(), xs[:1].contiguous()
        stock(x1i, x1s)
        n1, el1 = run_for(lambda: stock(x1i, x1s), 2.0, 30)
        b1_ms = el1 / n1 * 1e3
        out["b1_one_thread"] = {"ms_per_window": b1_ms, "realtime_factor_60fps": (1000.0 / b1_ms) / 60.0,
                                "sample": f"{n1} forwards of B=1,T={T}, torch.set_num_threads(1) as the reference's runner"}
        # second figure: the module's own torch-op restatement (SDPA + explicit recurrence loop)
        m = build_model(cfg, 0, True).eval()
        torch.set_num_threads(cores)
        m._forward_torch_ops(xi, xs)
        n2, el2 = run_for(lambda: m._forward_torch_ops(xi, xs), 3.0, 12)
        out["torch_ops_composite"] = {"value": B * n2 / el2, "unit": "IMU frames/s", "cores": cores,
                                      "sample": f"{n2} forwards, same inputs, {el2:.1f} s"}
        torch.set_num_threads(max_threads)
    try:   # the C oracle (scalar port, OpenMP over windows), same workload, bounded
        from oracle import oracle
        nt = oracle.max_threads()
        nb = min(B, max(4 * nt, 32))
        t0 = time.perf_counter()
        oracle.forward(cfg, w, x_imu[:nb], x_s[:nb], dtype=np.float32, nthreads=nt)
        el = time.perf_counter() - t0
        out["oracle_c"] = {"value": nb / el, "unit": "IMU frames/s", "cores": nt,
                           "sample": f"{nb} windows T={T}, scalar C restatement, {el:.1f} s"}
    except Exception as e:  # the oracle is optional for the baseline leg
        out["oracle_c"] = {"error": str(e)}
    return out


def clock_probe(buf):
    st = tlib.load().tip_debug_clock_probe(ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == 0


def smi_sclk_mhz():
    """Current shader clock as rocm-smi reports it (sampled while the GPU is busy); None when unavailable."""
    try:
        out = subprocess.run(["rocm-smi", "-d", str(torch.cuda.current_device()), "--showclocks", "--json"],
                             stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=20).stdout
        card = next(iter(json.loads(out).values()))
        for k, v in card.items():
            if "sclk" in k.lower() and "mhz" in str(v).lower():
                return float(str(v).lower().replace("(", "").replace(")", "").replace("mhz", "").strip())
    except Exception:
        return None
    return None


def sustained_pass(step, ms_est, seconds):
    """Hold the headline step for `seconds`: sustained ms/step, the shader clock held (s_memtime ticks over wall_clock64's
    100 MHz, both read on the device right before and after), rocm-smi's clock sampled mid-run."""
    n = max(50, int(seconds * 1e3 / ms_est))
    probes = torch.zeros(8, dtype=torch.int64, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    clock_probe(probes[0:4])
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    clock_probe(probes[4:8])
    smi = smi_sclk_mhz()                  # the queue is still draining while this runs
    e1.synchronize()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    p = probes.cpu().numpy().astype(np.float64)
    ticks, wall_s = p[4] - p[0], (p[5] - p[1]) / 100e6
    ghz = ticks / wall_s / 1e9 if wall_s > 0 else None
    return {"steps": n, "seconds": ms * 1e-3, "sustained_ms_per_step": ms / n,
            "sclk_ghz_s_memtime": ghz, "probe_xcc": [int(p[2]), int(p[6])], "sclk_mhz_rocm_smi": smi}


def train_step_times(cfg, dev, B=256, T=40, steps=20, warmup=5):
    import warnings
    m = build_model(cfg, 0, load=True).to(dev).train()
    m.ENCODER_DROPOUT = 0.1
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
    x_imu, x_s = synth.make_inputs(cfg, 64, T, seed=5)
    xi = torch.tensor(np.tile(x_imu, (B // 64, 1, 1))).to(dev)
    xs = torch.tensor(np.nan_to_num(np.tile(x_s, (B // 64, 1, 1)))).to(dev)
    tgt = torch.randn(B, T, cfg["size_s"], device=dev)

    def fwd():
        return m(xi, xs)

    def fb():
        for p in m.parameters():
            p.grad = None
        fwd().backward(tgt)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = ((fwd() - tgt) ** 2).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        opt.step()

    res = {"batch": B, "T": T, "encoder_dropout": 0.1, "optimizer": "AdamW + clip_grad_norm_ (torch)"}
    n0 = m.hip_forward_count()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, fn in (("forward_ms", fwd), ("fwd_bwd_ms", fb), ("step_ms", step)):
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            # best of two loops: a one-off allocator event (the caching allocator re-growing the 0.5-GB activation stash after the
            # previous section's empty_cache) otherwise lands in one loop's mean — seen once as forward 3.8 ms instead of 0.80
            res[name] = min(timed_loop(fn, steps), timed_loop(fn, steps))
    res["timing"] = "best of two loops of %d calls" % steps
    assert m.hip_forward_count() > n0, "the HIP training kernels did not run"
    fl = synth.flops_per_window(cfg, T)
    res["fwd_bwd_tflops"] = 3 * B * fl / res["fwd_bwd_ms"] / 1e9
    res["fwd_bwd_frac_of_fp32_mfma_peak"] = res["fwd_bwd_tflops"] / PEAK_FP32_MFMA_TFLOPS
    res["windows_per_s_step"] = B / res["step_ms"] * 1e3
    m.check_handoffs()
    del m, opt
    torch.cuda.empty_cache()
    return res


def zero_edit_runner_latency(cfg, dev, x1i, x1s, frames=240):
    """p50 of `model(x_imu.cuda(), x_s.cuda()).cpu()` exactly as the unedited runner drives the module: .train() mode (model.eval()
    is commented out in offline_testing_simple.py:98), past_state_dropout 0.8, autograd recording (no torch.no_grad in
    real_time_runner_minimal.py:149), host float tensors in, row T-1 read on the host.  T = 40 (steady state) and T growing 1 -> 40
    (the first 40 frames of a run)."""
    import warnings
    with contextlib.redirect_stdout(sys.stderr):
        m = tip_amd.TF_RNN_Past_State(
            cfg["input_size_imu"], cfg["size_s"], rnn_hid_size=cfg["rnn_hid_size"], tf_hid_size=cfg["tf_hid_size"],
            tf_in_dim=cfg["tf_in_dim"], n_heads=cfg["n_heads"], tf_layers=cfg["tf_layers"], dropout=0.0, in_dropout=0.0,
            past_state_dropout=0.8, with_acc_sum=cfg.get("with_acc_sum", False))
    w = synth.make_weights(cfg, seed=0)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    m = m.to(dev)                                   # .cuda(), and NO .eval(): the module stays in training mode
    assert m.training
    h_i, h_s = x1i.cpu(), torch.nan_to_num(x1s.cpu())
    T = h_i.shape[1]
    n0 = m.hip_forward_count()

    def frame(t):
        x_imu, x_s = h_i[:, :t], h_s[:, :t]
        t0 = time.perf_counter()
        y = m(x_imu.cuda(), x_s.cuda()).cpu()
        row = y.squeeze(0)[-1, :].detach().numpy()
        dt = (time.perf_counter() - t0) * 1e3
        assert np.isfinite(row).all()
        return dt

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(30):
            frame(T)
        steady = [frame(T) for _ in range(frames)]
        grow = [frame(t) for _ in range(3) for t in range(1, T + 1)]
        # device time of the call alone (events), inputs resident: what the kernels cost without the host protocol
        d_i, d_s = h_i.to(dev), h_s.to(dev)
        dev_ms = p50_latency_ms(lambda: m(d_i, d_s), 100)
    assert m.hip_forward_count() > n0, "the HIP kernels did not run"
    m.check_handoffs()
    p50 = float(np.median(steady))
    res = {"p50_ms_host_call_T40": p50, "p95_ms_host_call_T40": float(np.percentile(steady, 95)),
           "p50_ms_growing_T_1_to_40": float(np.median(grow)), "max_ms_growing_T_1_to_40": float(np.max(grow)),
           "p50_ms_device_only_T40": dev_ms, "realtime_factor_60fps": (1000.0 / p50) / 60.0,
           "meets_60x_realtime_278us": bool(p50 <= 0.278),
           "mode": ".train() (never .eval()), past_state_dropout 0.8, autograd recording, host tensors in / row T-1 out on the host"}
    del m
    return res


def extra_configs(model, cfg, xi, xs, dev, seconds_budget=40.0):
    """Every other BASELINE.json configuration on this run's clock (N = 1).  A few seconds each."""
    out = {}
    T = xi.shape[1]
    fpw = synth.flops_per_window(cfg, T)
    model.set_plan("auto")
    # -- configs[0]/north_star B=1: device-resident p50, and the per-frame protocol of real_time_runner_minimal.py:146-150
    #    (host window -> H2D -> forward -> D2H of the consumed row)
    x1i, x1s = xi[:1].contiguous(), xs[:1].contiguous()
    for _ in range(10):
        model.forward_last(x1i, x1s)
    lat_full = p50_latency_ms(lambda: model(x1i, x1s), 200)
    lat_last = p50_latency_ms(lambda: model.forward_last(x1i, x1s), 200)
    h_i, h_s = x1i.cpu().pin_memory(), x1s.cpu().pin_memory()
    ts = []
    for _ in range(220):
        t0 = time.perf_counter()
        y = model.forward_last(h_i.to(dev, non_blocking=True), h_s.to(dev, non_blocking=True)).cpu()   # .cpu() synchronises
        ts.append((time.perf_counter() - t0) * 1e3)
    lat_pcie = float(np.median(ts[20:]))
    out["b1_latency"] = {"p50_forward_ms": lat_full, "p50_forward_last_row_ms": lat_last,
                         "realtime_factor_60fps": (1000.0 / lat_full) / 60.0,
                         "p50_ms_with_h2d_window_and_d2h_last_row": lat_pcie,
                         "realtime_factor_60fps_with_pcie": (1000.0 / lat_pcie) / 60.0,
                         "hbm_gbs_weights_plus_io": (14709260 + 56320) / (lat_full * 1e-3) / 1e9,
                         "note": "latency-bound: far below either roofline (weights 14.7 MB + 56 KB I/O per forward)"}
    del y
    # -- the UNEDITED reference runner's call (VERDICT r04 missing #3): offline_testing_simple.py:87-98 builds the module with
    #    past_state_dropout=0.8 and never calls .eval(); real_time_runner_minimal.py:146-150 calls it outside no_grad with host
    #    tensors and takes row T-1 on the host.  So every frame is a TRAINING-mode forward with autograd recording.
    try:
        out["b1_zero_edit_runner"] = zero_edit_runner_latency(cfg, dev, x1i, x1s)
    except Exception as e:
        out["b1_zero_edit_runner"] = {"error": f"{type(e).__name__}: {e}"}
    # -- configs[3] share / B=1024 last-row, and B=8192 on one GPU (north_star sweep point), full output
    for tag, Bx, last in (("b1024_last_row", 1024, True), ("b8192_full", 8192, False)):
        reps = Bx // xi.shape[0]
        bi, bs = xi.repeat(reps, 1, 1), xs.repeat(reps, 1, 1)
        fn = (lambda: model.forward_last(bi, bs)) if last else (lambda: model(bi, bs))
        for _ in range(3):
            fn()
        ms = timed_loop(fn, 12 if Bx <= 1024 else 5)
        out[tag] = {"batch": Bx, "T": T, "ms_per_step": ms, "frames_per_s": Bx / (ms * 1e-3),
                    "whole_forward_frac_of_fp32_mfma_peak": frac_of_peak(cfg, T, Bx / (ms * 1e-3)),
                    "headroom_vs_60fps": (1000.0 / ms) / 60.0}
        del bi, bs
    # -- batches that are not whole rounds of 256 windows: below a round AUTO spreads ONE window over four
    #    (33-64 windows) or two (65-128) CUs; above, it runs whole rounds + a remainder as two launch sequences when that is cheaper
    #    than one more full round
    try:
        rem = {}
        for Bx in (48, 64, 128, 272, 300, 1000):
            reps = (Bx + xi.shape[0] - 1) // xi.shape[0]
            bi, bs = xi.repeat(reps, 1, 1)[:Bx].contiguous(), xs.repeat(reps, 1, 1)[:Bx].contiguous()
            for _ in range(3):
                model(bi, bs)
            ms = timed_loop(lambda: model(bi, bs), 20)
            rem[f"b{Bx}"] = {"ms_per_step": ms, "frames_per_s": Bx / (ms * 1e-3),
                             "whole_forward_frac_of_fp32_mfma_peak": frac_of_peak(cfg, T, Bx / (ms * 1e-3))}
            del bi, bs
        out["non_round_batches"] = rem
    except Exception as e:
        out["non_round_batches"] = {"error": f"{type(e).__name__}: {e}"}
    # -- configs[2]: 1024 closed-loop streams through the on-device streaming engine (ingest -> forward(last row) -> consume)
    try:
        from scipy.spatial.transform import Rotation
        n = 1024
        rng = np.random.RandomState(n)
        base = Rotation.random(n * 6, random_state=n).as_matrix().reshape(n, 54).astype(np.float32)
        s_init = (rng.randn(n, 114) * 0.2).astype(np.float32)
        model.freeze_packed(True)
        eng = tip_amd.streaming.StreamingEngine(model, s_init)
        frames = [torch.tensor(np.concatenate([base, rng.randn(n, 18).astype(np.float32)], axis=1)).to(dev) for _ in range(8)]
        for f in range(60):                      # prime the smoother and fill the 40-frame windows
            eng.step(frames[f % 8])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(60):
            eng.step(frames[f % 8])
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / 60 * 1e3
        out["streams1024_closed_loop"] = {"streams": n, "ms_per_frame": ms, "stream_frames_per_s": n / (ms * 1e-3),
                                          "headroom_vs_60fps_budget_16.7ms": (1000.0 / 60.0) / ms,
                                          "whole_forward_frac_of_fp32_mfma_peak": frac_of_peak(cfg, T, n / (ms * 1e-3))}
        # ... and with SURVEY.md 7-7's exact reuse (tip_forward_reuse: a frame's in_linear row and layer-0 Q | K | V rows computed once,
        # kept in a per-stream ring for the 40 windows the frame appears in; bit-identical outputs — tests/test_reuse_gpu.py).  Valid
        # because this model is built with past_state_dropout = 0 and runs in .eval(); both loops measured back to back on this box
        try:
            eng = tip_amd.streaming.StreamingEngine(model, s_init, reuse=True)
            for f in range(90):                  # prime, fill the windows, one trip round the 40-slot ring
                eng.step(frames[f % 8])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for f in range(60):
                eng.step(frames[f % 8])
            torch.cuda.synchronize()
            ms_r = (time.perf_counter() - t0) / 60 * 1e3
            out["streams1024_closed_loop_reuse"] = {"streams": n, "ms_per_frame": ms_r, "stream_frames_per_s": n / (ms_r * 1e-3),
                                                    "headroom_vs_60fps_budget_16.7ms": (1000.0 / 60.0) / ms_r,
                                                    "vs_recompute": ms_r / ms, "ring_mb": eng._ring.numel() / 1e6,
                                                    "note": "exact reuse of per-frame rows across sliding windows (past_state_dropout = 0, .eval())"}
            del eng
        except Exception as e:
            out["streams1024_closed_loop_reuse"] = {"error": f"{type(e).__name__}: {e}"}
        del frames
    except Exception as e:   # the extras must never take the headline line down
        out["streams1024_closed_loop"] = {"error": f"{type(e).__name__}: {e}"}
    # -- the configuration a live demo runs: ONE closed-loop stream, per-frame latency after the window is full (p50 / p95 over
    #    300 frames; device time by events around the step, host time = wall time of the call without waiting for the GPU)
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import stream_latency
        model.set_plan("auto")
        out["stream1_closed_loop"] = stream_latency.measure(model, 1, frames=300)
        out["stream1_closed_loop"]["note"] = ("warm (260 frames before the first timed one): round 2's 1.37 ms figure was the first "
                                              "60 frames of a cold process (clock ramp + first-use kernel loads), not the loop")
        out["stream1_closed_loop_hip_graph"] = stream_latency.measure(model, 1, frames=300, use_graph=True)
        out["stream1_closed_loop_hip_graph"]["note"] = ("StreamingEngine(use_graph=True): ingest + forward_last + consume captured once, "
                                                        "one graph launch per frame; bit-identical outputs (tests/test_streaming_gpu.py)")
    except Exception as e:
        out["stream1_closed_loop"] = {"error": f"{type(e).__name__}: {e}"}
    # -- self-check: EVERY window of the headline batch against the same forward in fp64 ON THE DEVICE (tip_forward_f64: the module
    #    as train_model.py --double builds it; itself held to 1e-11 of the reference's fp64 outputs by tests/test_f64_gpu.py)
    try:
        x256i, x256s = xi[:256].contiguous(), xs[:256].contiguous()
        m64 = build_model(cfg, 0, load=True).double().to(dev).eval()
        xi64, xs64 = x256i.double(), x256s.double()
        y64 = m64(xi64, xs64)
        ms64 = timed_loop(lambda: m64(xi64, xs64), 3)
        model.set_plan("auto")
        err = float((model(x256i, x256s).double() - y64).abs().max().item())
        out["f64_b256"] = {"batch": int(x256i.shape[0]), "T": T, "dtype": "f64", "ms_per_step": ms64,
                           "headline_plan_max_abs_err_vs_on_device_fp64_all_windows": err, "max_abs_y": float(y64.abs().max().item()),
                           "note": "debugging path (layer-by-layer fp64 kernels), not tuned"}
        del m64, y64
    except Exception as e:
        out["f64_b256"] = {"error": f"{type(e).__name__}: {e}"}
    # -- row a14 / f-2: the training-mode model call and its backward (train_model.py:171-196) at the reference's batch size,
    #    HIP kernels in both directions, encoder dropout p = 0.1 live; forward, forward+backward (3x the forward FLOPs) and the
    #    whole step with clip + AdamW
    try:
        with torch.enable_grad():            # (the extras run inside the caller's no_grad block)
            out["train_b256"] = train_step_times(cfg, dev)
    except Exception as e:
        out["train_b256"] = {"error": f"{type(e).__name__}: {e}"}
    # -- configs[4] share: scaled model, B=512, T=80 (random-init weights on the device)
    try:
        sc = synth.SCALED
        torch.manual_seed(0)
        with torch.device(dev):                       # 152 M parameters: drawn on the GPU
            ms_model = build_model(sc, 0, load=False).eval()
        Bs, Ts = 512, 80
        s_imu, s_s = synth.make_inputs(sc, 64, Ts, seed=99)
        si = torch.tensor(s_imu).to(dev).repeat(Bs // 64, 1, 1)
        ss = torch.tensor(s_s).to(dev).repeat(Bs // 64, 1, 1)
        ms_model(si, ss)
        ms_model(si, ss)
        ms = timed_loop(lambda: ms_model(si, ss), 3)
        out["scaled_b512_t80"] = {"batch": Bs, "T": Ts, "ms_per_step": ms, "frames_per_s": Bs / (ms * 1e-3),
                                  "whole_forward_frac_of_fp32_mfma_peak": frac_of_peak(sc, Ts, Bs / (ms * 1e-3)),
                                  "tflops": Bs / (ms * 1e-3) * synth.flops_per_window(sc, Ts) / 1e12}
        # (configs[4] at its own batch, B = 4096 in total, is `extra.scaling_table.scaled_b4096_total` — at N = 1 all of it on this GPU, chunked by
        #  tip_max_batch)
        del ms_model, si, ss
        torch.cuda.empty_cache()
    except Exception as e:
        out["scaled_b512_t80"] = {"error": f"{type(e).__name__}: {e}"}
    del fpw
    return out


def scaled_row(rank, world, dev, args, timed_row, shard):
    """BASELINE configs[4] on this run's N GPUs: the scaled model (12 layers, d = 1024, ffn = 4096, 16 heads, rnn 512, T = 80), 4096
    windows in total = 4096 / N per GPU, full output.  Rank 0 draws the 152 M parameters (the module's own random init) on its GPU,
    packs them there and broadcasts the 609-MB image once (RCCL over xGMI; timed as `weight_broadcast_ms`, off the timed steps);
    the other ranks never initialise parameters of their own."""
    sc = synth.SCALED
    Ts = 80
    lo, hi = shard
    bt = hi - lo
    torch.manual_seed(0)
    with torch.device(dev if rank == 0 else "meta"):
        m = build_model(sc, 0, load=False)            # rank 0: torch.empty + uniform_ on the GPU; the others: shapes only
    if rank != 0:
        m = m.to_empty(device=dev)                    # (their parameters are never read: broadcast_packed attaches rank 0's image)
    m = m.eval()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    packed = tdist.broadcast_packed(m, src=0, device=dev)
    torch.cuda.synchronize()
    bms = (time.perf_counter() - t0) * 1e3
    # a caller-selected plan without cooperating kernels (the shared-GPU rehearsal) maps to the general plan here: the fused plans
    # are the paper configuration's
    m.set_plan("auto" if args.plan == "auto" else "general", rnn_cluster=args.rnn_cluster)
    s_imu, s_s = synth.make_inputs(sc, 64, Ts, seed=99 + rank)
    reps = (max(bt, 1) + 63) // 64
    si = torch.tensor(s_imu).to(dev).repeat(reps, 1, 1)[:bt].contiguous()
    ss = torch.tensor(s_s).to(dev).repeat(reps, 1, 1)[:bt].contiguous()
    row = timed_row(m, sc, lambda: m(si, ss), 4096, Ts, 3, 2, False)
    row["weight_broadcast_ms"] = bms
    row["packed_image_mb"] = packed.numel() / 1e6
    row["tflops"] = row["frames_per_s"] * synth.flops_per_window(sc, Ts) / 1e12
    row["chunk"] = int(m.chunk_batch(Ts))
    del m, si, ss, packed
    torch.cuda.empty_cache()
    return row


def pin_to_gpu_numa_node(dev_index):
    """Pin this rank's host threads to the CPUs of its GPU's NUMA node (VERDICT r05 #1b: at B = 1 a forward is ~20 launches and
    ~0.12 ms of host time per call, and with eight ranks on one node the scheduler otherwise parks some of them across the socket
    link from their GPU).  PCI address from the HIP device properties -> /sys/bus/pci/devices/<bdf>/{numa_node,local_cpulist};
    the set is intersected with what this process may use (cgroup / taskset) and applied to every thread the process already has
    (runtime threads inherit from then on).  TIP_BENCH_NO_PIN=1 disables.  Returns what was done, for the JSON line."""
    info = {"pinned": False}
    try:
        if os.environ.get("TIP_BENCH_NO_PIN", "0") == "1":
            info["reason"] = "TIP_BENCH_NO_PIN=1"
            return info
        pr = torch.cuda.get_device_properties(dev_index)
        bdf = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
        base = os.path.join("/sys/bus/pci/devices", bdf)
        info["pci"] = bdf
        node = int(open(os.path.join(base, "numa_node")).read().strip())
        info["numa_node"] = node
        cpus = set()
        src = os.path.join("/sys/devices/system/node", f"node{node}", "cpulist") if node >= 0 else os.path.join(base, "local_cpulist")
        for part in open(src).read().strip().split(","):
            if not part:
                continue
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
        allowed = os.sched_getaffinity(0)
        use = cpus & allowed
        info["node_cpus"], info["allowed_cpus"] = len(cpus), len(allowed)
        if not use or use == allowed:
            info["reason"] = "node CPUs == allowed CPUs" if use else "no overlap with the allowed CPUs"
            return info
        for tid in os.listdir("/proc/self/task"):
            try:
                os.sched_setaffinity(int(tid), use)
            except OSError:
                pass
        info["pinned"], info["cpus"] = True, len(use)
    except Exception as e:     # no sysfs entry (container), no permission: run unpinned and say so
        info["reason"] = f"{type(e).__name__}: {e}"
    return info


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: re-run this command line under torch.distributed.run with N ranks on this
    node (one per GPU, rendezvous on 127.0.0.1, a free port) and return its exit code.  A box with fewer than N GPUs is an error —
    never a silent N = 1 measurement — unless TIP_BENCH_SHARE_GPU=1 (the world-size-2 rehearsal on one GPU, tests/test_dist_gpu.py)."""
    import socket
    import subprocess
    share = os.environ.get("TIP_BENCH_SHARE_GPU", "0") == "1"
    have = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if have < n and not (share and have >= 1):
        print(f"bench.py: --gpus {n} requested but this node shows {have} GPU(s); refusing to measure fewer ranks than asked for",
              file=sys.stderr)
        return 2
    port = os.environ.get("MASTER_PORT")
    if not port:
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = str(sk.getsockname()[1])
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", port, os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="paper256", choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=0, help="windows (IMU streams) per GPU; 0 = the configuration's own")
    ap.add_argument("--seq-len", type=int, default=0)
    ap.add_argument("--plan", default="auto", choices=["auto", "general", "fused", "latency", "fused2", "fusedh", "fused1s"])
    ap.add_argument("--rnn-cluster", type=int, default=0)
    ap.add_argument("--full", action="store_true",
                    help="also run the cross-rank self-checks, the CPU baseline and the extras (extra.configs / extra.sustained / "
                         "extra.scaling_table); a plain run times the headline step only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's output to DIR/y.npy (float32; a seeded sample of windows above 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip extra.configs / extra.sustained / extra.scaling_table")
    ap.add_argument("--no-scaled", action="store_true", help="scaling table without the scaled-model row (BASELINE configs[4])")
    ap.add_argument("--sustain-s", type=float, default=3.0)
    ap.add_argument("--prewarm-s", type=float, default=0.5, help="untimed seconds of the same step before the warm-up (clock ramp)")
    ap.add_argument("--profile-all", action="store_true", help="print a per-stage time table (separate pass)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    extras = args.full and not args.no_extra
    cpu_leg = args.full and not args.no_cpu_baseline

    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))   # `python bench.py --gpus N` starts its own N ranks (one per GPU)

    t_main0 = time.perf_counter()
    rank, local_rank, world = tdist.env_rank()
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    # TIP_BENCH_SHARE_GPU=1 + TIP_BENCH_BACKEND=gloo: every rank on cuda:0 over gloo — how tests/test_dist_gpu.py rehearses the
    # world_size-2 control AND data flow of this very file on a 1-GPU box (with a plan without cooperating kernels)
    share_gpu = os.environ.get("TIP_BENCH_SHARE_GPU", "0") == "1"
    backend = os.environ.get("TIP_BENCH_BACKEND", "nccl")
    dev_index = 0 if share_gpu else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    pin = pin_to_gpu_numa_node(dev_index)      # before the process group / the first kernel: threads created later inherit the mask
    use_pg = "RANK" in os.environ          # launched by torch.distributed.run (also exercised with one rank)
    if use_pg:
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    def gather_all(t):
        """all_gather of a small device tensor -> list of tensors on `dev` (gloo has no CUDA all_gather: host round trip)."""
        if not (use_pg and world > 1):
            return [t]
        if backend == "nccl":
            out = [torch.zeros_like(t) for _ in range(world)]
            dist.all_gather(out, t)
            return out
        tc = t.cpu()
        out = [torch.zeros_like(tc) for _ in range(world)]
        dist.all_gather(out, tc)
        return [o.to(dev) for o in out]

    if world != args.gpus:                 # never print an N = 1 line for an N-GPU request (or the other way round)
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: start it as `python bench.py --gpus N` (it spawns its "
                         f"own ranks) or under torch.distributed.run with --nproc-per-node equal to --gpus")

    spec = CONFIGS[args.config]
    cfg = spec["cfg"]
    B, T = args.batch or spec["B"], args.seq_len or spec["T"]
    last = spec["last"]
    synth_weights = args.config != "scaled512"     # 152 M parameters: the module's own random init, drawn on rank 0's GPU
    torch.manual_seed(0)
    model = build_model(cfg, 0, load=(rank == 0 and synth_weights))
    model = model.to(dev).eval()
    t_b0 = time.perf_counter()
    packed = tdist.broadcast_packed(model, src=0, device=dev)      # one-time RCCL broadcast (no-op collective at N=1)
    torch.cuda.synchronize()
    bcast_ms = (time.perf_counter() - t_b0) * 1e3
    image_equal = None
    if args.full:
        # every rank must hold rank 0's image, bit for bit
        csum = packed.view(torch.int32).to(torch.int64).sum().reshape(1)
        sums = gather_all(csum)
        image_equal = all(int(s.item()) == int(sums[0].item()) for s in sums)
        assert image_equal, "a rank's packed weight image differs from rank 0's after the broadcast"
    model.set_plan(args.plan, rnn_cluster=args.rnn_cluster, profile=0)

    x_imu, x_s = synth.make_inputs(cfg, min(B, 256), T, seed=1234 + rank)
    xi, xs = torch.tensor(x_imu).to(dev), torch.tensor(x_s).to(dev)
    if B > xi.shape[0]:
        reps = (B + xi.shape[0] - 1) // xi.shape[0]
        xi, xs = xi.repeat(reps, 1, 1)[:B].contiguous(), xs.repeat(reps, 1, 1)[:B].contiguous()
    step = (lambda: model.forward_last(xi, xs)) if last else (lambda: model(xi, xs))

    def sync_all():
        torch.cuda.synchronize()
        if use_pg:
            dist.barrier()
            torch.cuda.synchronize()

    with torch.no_grad():
        # Bring the GPU from its idle power state to its operating clocks before the W warm-up steps (part of the set-up, like
        # the weight broadcast: a 10-step warm-up is 7 ms, the clock ramp is longer, and the first timed steps would otherwise be
        # measured on a GPU that is still clocking up: 0.704 vs 0.685 ms per step in profiles/r02).  Disclosed as `prewarm_s`.
        t_pw = time.perf_counter()
        while time.perf_counter() - t_pw < args.prewarm_s:
            for _ in range(20):
                step()
            torch.cuda.synchronize()
        for _ in range(args.warmup):
            y = step()
        # event pair around the dominant kernel of every FOURTH step (TIP_OPT_PROFILE = 3): a pair on every launch costs ~7 us of
        # queue barriers per step (0.624 vs 0.631 ms, profiles/r05), which is measurement overhead, not forward time
        model.set_plan(args.plan, rnn_cluster=args.rnn_cluster, profile=3)
        sync_all()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            y = step()
        sync_all()
        elapsed = time.perf_counter() - t0
        prof = model.profile_read()
        model.set_plan(args.plan, rnn_cluster=args.rnn_cluster, profile=0)
    assert torch.isfinite(y).all()
    model.check_handoffs()                 # a lost inter-workgroup hand-off is an error, not a number
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, y, rank, world)
    outputs_equal, digs = None, None
    if args.full:
        # every rank's outputs for the same probe windows must be rank 0's, bit for bit
        with torch.no_grad():
            dig = probe_outputs(model, cfg, dev, T, xi, xs, last)
        digs = gather_all(dig)
        outputs_equal = all(torch.equal(d_, digs[0]) for d_ in digs)
        assert outputs_equal, f"rank outputs differ for identical probe windows: {[d_.tolist() for d_ in digs]}"
    my_ms = elapsed / args.steps * 1e3
    rank_ms = [my_ms]
    if use_pg:
        all_t = gather_all(torch.tensor([elapsed], device=dev, dtype=torch.float64))
        rank_ms = [float(v.item()) / args.steps * 1e3 for v in all_t]
        elapsed = max(float(v.item()) for v in all_t)

    global_b = B * world
    value = global_b * args.steps / elapsed
    nodes = gather_all(torch.tensor([pin.get("numa_node", -2), 1 if pin.get("pinned") else 0, pin.get("cpus", 0)], device=dev, dtype=torch.int64))
    pins = {"rank0": pin, "numa_node_per_rank": [int(v[0].item()) for v in nodes], "pinned_per_rank": [bool(v[1].item()) for v in nodes],
            "cpus_per_rank": [int(v[2].item()) for v in nodes]}

    roofline = None
    if prof:
        name, ms, launches = max(prof, key=lambda r: r[1])
        fl = stage_flops(cfg, name, B, T)
        if fl and launches:
            avg_ms = ms / launches
            ach = fl / (avg_ms * 1e-3) / 1e12
            traffic = None
            tpath = os.path.join(ROOT, "profiles", "traffic.json")
            if os.path.exists(tpath):
                try:
                    traffic = json.load(open(tpath)).get(name, {}).get(f"B{B}_T{T}")
                except Exception:
                    traffic = None
            roofline = {"bound": "mfma", "kernel": name, "achieved": ach, "peak": PEAK_FP32_MFMA_TFLOPS,
                        "unit": "TFLOP/s", "frac": ach / PEAK_FP32_MFMA_TFLOPS, "traffic": traffic,
                        # achieved / frac / avg_launch_ms are measured in THIS run (event pairs around every launch of the kernel);
                        # traffic is NOT: PMC counters need rocprofv3 passes of their own, so the number is the stored result of
                        # tools/collect_profiles.sh's last collection (same kernel, same batch)
                        "traffic_source": "profiles/traffic.json (stored: rocprofv3 PMC passes of tools/collect_profiles.sh, not measured by this run)"
                        if traffic is not None else None,
                        "avg_launch_ms": avg_ms, "launches_timed": launches, "flops_per_launch": fl,
                        "sampling": "HIP event pair around every 4th launch of the kernel inside the timed region"}

    extra = {}
    if args.config == "paper256" and extras:
        # north_star's table on this run's N GPUs, every row with the headline's barrier + max-over-ranks timing:
        #   batch1_per_gpu      one stream per GPU (the latency case; frames/s = N / step time)
        #   batch256_total      256 windows in total, 256 / N per GPU, full output: the headline workload STRONG-scaled (the headline
        #                       itself is weak: 256 per GPU)
        #   streams8192_total   BASELINE configs[3]: 8192 concurrent streams in total, 8192 / N per GPU, last-row output
        #   streams8192_closed_loop_total   the same streams through the on-device streaming engine (whole frame: ingest, forward, consume)
        #   scaled_b4096_total  BASELINE configs[4]: 12 layers, d = 1024, ffn = 4096, T = 80, 4096 windows in total, 4096 / N per GPU,
        #                       full output, with its own one-time broadcast of the 609-MB image (below)
        table = {}

        def timed_row(mdl, c, fn, total, Tt, nst, nwarm, lastrow):
            for _ in range(nwarm):
                fn()
            sync_all()
            t1 = time.perf_counter()
            for _ in range(nst):
                fn()
            sync_all()
            el = torch.tensor([time.perf_counter() - t1], device=dev, dtype=torch.float64)
            els = gather_all(el)
            el_max = max(float(v.item()) for v in els)
            mdl.check_handoffs()
            tot = sum(shard_sizes(total))
            return {"streams_per_gpu": shard_sizes(total)[0], "streams_total": tot, "T": Tt, "steps": nst, "ms_per_step": el_max / nst * 1e3,
                    "frames_per_s": tot * nst / el_max, "output": "last row" if lastrow else "full",
                    "whole_forward_frac_of_fp32_mfma_peak": frac_of_peak(c, Tt, tot * nst / el_max, world)}

        def shard_sizes(total):     # contiguous split of `total` streams over the ranks (tdist.shard_range): the first total % N get one more
            return [hi - lo for lo, hi in (tdist.shard_range(total, r, world) for r in range(world))]

        with torch.no_grad():
            for name, total, lastrow, nst in (("batch1_per_gpu", world, True, 200), ("batch256_total", 256, False, 50),
                                              ("streams8192_total", 8192, True, 10)):
                lo, hi = tdist.shard_range(total, rank, world)
                bt = hi - lo
                reps = (max(bt, 1) + xi.shape[0] - 1) // xi.shape[0]
                ti, ts_ = xi.repeat(reps, 1, 1)[:bt].contiguous(), xs.repeat(reps, 1, 1)[:bt].contiguous()
                fn = (lambda: model.forward_last(ti, ts_)) if lastrow else (lambda: model(ti, ts_))
                table[name] = timed_row(model, cfg, fn, total, T, nst, 3, lastrow)
                del ti, ts_
            # BASELINE configs[3] as the runner would drive it: the 8192 streams CLOSED-LOOP through the on-device front / back end
            # (ingest -> forward(last row) -> consume per frame, nothing crosses PCIe), 8192 / N streams per GPU; measured twice, with
            # every window recomputed and with SURVEY 7-7's exact reuse of per-frame rows where the engine's "auto" rule engages it
            # (>= two windows per CU; this model has no stochastic part) — the row's ms_per_step is the latter's
            try:
                from scipy.spatial.transform import Rotation
                lo, hi = tdist.shard_range(8192, rank, world)
                bt = hi - lo
                rs = np.random.RandomState(8192 + rank)
                base = Rotation.random(bt * 6, random_state=8192 + rank).as_matrix().reshape(bt, 54).astype(np.float32)
                s_init = (rs.randn(bt, 114) * 0.2).astype(np.float32)
                frames = [torch.tensor(np.concatenate([base, rs.randn(bt, 18).astype(np.float32)], axis=1)).to(dev) for _ in range(4)]
                rows = {}
                for tag, kw in (("recompute", {}), ("reuse", {"reuse": "auto"})):
                    eng = tip_amd.streaming.StreamingEngine(model, s_init, **kw)
                    ctr = [0]

                    def one_frame():
                        eng.step(frames[ctr[0] & 3])
                        ctr[0] += 1
                    for _ in range(86):          # smoother primed, windows full (frame 44), one trip round the reuse ring (frame 84)
                        one_frame()
                    rows[tag] = timed_row(model, cfg, one_frame, 8192, T, 10, 2, True)
                    rows[tag]["reuse_engaged"] = bool(eng.reuse)
                    del eng
                row = rows["reuse"]
                row["recompute_ms_per_step"] = rows["recompute"]["ms_per_step"]
                if row["reuse_engaged"]:
                    # the fraction of peak counts the work EXECUTED: with the ring, in_linear and layer 0's QKV projection run for one row
                    # of 40 per window; what the recomputing forward's FLOP count would make of the same time is kept beside it
                    saved = (T - 1) / T * (2.0 * T * (cfg["input_size_imu"] + (18 if cfg.get("with_acc_sum") else 0) + cfg["size_s"]) * cfg["tf_in_dim"]
                                           + 2.0 * T * cfg["tf_in_dim"] * 3 * cfg["tf_in_dim"])
                    row["frac_if_counted_with_the_recomputing_forwards_flops"] = row["whole_forward_frac_of_fp32_mfma_peak"]
                    row["whole_forward_frac_of_fp32_mfma_peak"] *= 1.0 - saved / synth.flops_per_window(cfg, T)
                row["output"] = "closed loop: pose s_t[3:114] and SBP row per stream and frame, on the GPU"
                table["streams8192_closed_loop_total"] = row
                del frames
            except Exception as e:
                table["streams8192_closed_loop_total"] = {"error": f"{type(e).__name__}: {e}"}
            if not args.no_scaled:
                try:
                    table["scaled_b4096_total"] = scaled_row(rank, world, dev, args, timed_row, tdist.shard_range(4096, rank, world))
                except Exception as e:     # the extras never take the headline line down (every rank fails or passes alike: same code, same sizes)
                    table["scaled_b4096_total"] = {"error": f"{type(e).__name__}: {e}"}
        model.check_handoffs()
        extra["scaling_table"] = table
    with torch.no_grad():
        if rank == 0 and world == 1 and extras:
            extra["sustained"] = sustained_pass(step, my_ms, args.sustain_s)
            sus = extra["sustained"]
            if sus.get("sclk_ghz_s_memtime"):
                wps = B / (sus["sustained_ms_per_step"] * 1e-3)
                sus["whole_forward_frac_of_peak_at_2.4GHz"] = frac_of_peak(cfg, T, wps)
                sus["whole_forward_frac_of_peak_at_held_clock"] = frac_of_peak(cfg, T, wps) * PEAK_CLOCK_GHZ / sus["sclk_ghz_s_memtime"]
            extra["p50_forward_ms_batch"] = p50_latency_ms(step, 40)
            if args.config == "paper256":
                extra["configs"] = extra_configs(model, cfg, xi, xs, dev)
                model.set_plan(args.plan, rnn_cluster=args.rnn_cluster, profile=0)
        if args.profile_all and rank == 0:
            model.set_plan(args.plan, rnn_cluster=args.rnn_cluster, profile=1)
            for _ in range(5):
                step()
            torch.cuda.synchronize()
            table = {}
            for n, ms, k in model.profile_read():
                table[n] = {"ms_per_forward": ms / 5, "launches_per_forward": k / 5}
            extra["stage_ms"] = table
            model.set_plan(args.plan, rnn_cluster=args.rnn_cluster, profile=0)
    model.check_handoffs()

    cpu = None
    if rank == 0 and world == 1 and cpu_leg:                      # N = 1 only (the N > 1 lines carry the GPU table; the host cores are the same box's)
        if pin.get("pinned"):                                       # the CPU leg may use every core the process was given
            os.sched_setaffinity(0, range(os.cpu_count()))
        cpu = cpu_baseline(synth.PAPER, 256, 40, budget_s=10.0)

    if rank == 0:
        fpw = synth.flops_per_window(cfg, T)
        line = {
            "metric": spec["metric"],
            "value": value, "unit": "IMU frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": spec["workload"].format(B=B, T=T), "name": args.config,
                       "global_batch": global_b, "seq_len": T, "plan": args.plan,
                       "parallelism": f"batch-sharded x{world}, one-time RCCL weight broadcast, no per-step collective"},
            "roofline": roofline,
            "cpu_baseline": cpu,
            "whole_forward_tflops": value * fpw / 1e12,
            "whole_forward_frac_of_fp32_mfma_peak": value * fpw / 1e12 / (PEAK_FP32_MFMA_TFLOPS * world),
            "world_size": world, "backend": ("nccl (RCCL)" if backend == "nccl" else backend) if use_pg else "single process",
            "per_rank_ms_per_step": {"min": min(rank_ms), "max": max(rank_ms), "all": rank_ms},
            "packed_image_identical_on_all_ranks": image_equal,
            "ranks_output_identical": outputs_equal, "probe_output_digest": [int(v) for v in digs[0].tolist()] if digs else None,
            "weight_broadcast_ms": bcast_ms, "prewarm_s": args.prewarm_s,
            "host_pinning": pins, "wall_s": time.perf_counter() - t_main0,
            "extra": extra,
        }
        # one-line summaries of the other benchmarked shapes LAST, so that they survive a reader that keeps only the tail of stdout
        cfgs = extra.get("configs", {}) if isinstance(extra.get("configs"), dict) else {}
        pick = lambda d, *ks: next((d[k] for k in ks if isinstance(d, dict) and k in d), None)   # noqa: E731
        line["tail_summary"] = {
            "b256_ms": line["ms_per_step"], "b256_frac": line["whole_forward_frac_of_fp32_mfma_peak"],
            "kernel_frac": roofline["frac"] if roofline else None,
            "b1_p50_last_row_ms": pick(cfgs.get("b1_latency"), "p50_forward_last_row_ms"),
            "b1_zero_edit_runner_p50_ms": pick(cfgs.get("b1_zero_edit_runner"), "p50_ms_host_call_T40"),
            "b1024_last_row_ms": pick(cfgs.get("b1024_last_row"), "ms_per_step"),
            "b1024_frac": pick(cfgs.get("b1024_last_row"), "whole_forward_frac_of_fp32_mfma_peak"),
            "streams1024_closed_loop_ms": pick(cfgs.get("streams1024_closed_loop"), "ms_per_frame"),
            "streams1024_closed_loop_reuse_ms": pick(cfgs.get("streams1024_closed_loop_reuse"), "ms_per_frame"),
            "b8192_full_ms": pick(cfgs.get("b8192_full"), "ms_per_step"),
            "b8192_frac": pick(cfgs.get("b8192_full"), "whole_forward_frac_of_fp32_mfma_peak"),
            "train_b256_fwd_bwd_ms": pick(cfgs.get("train_b256"), "fwd_bwd_ms"),
            "train_b256_frac": pick(cfgs.get("train_b256"), "fwd_bwd_frac_of_fp32_mfma_peak"),
            "scaled_b512_frac": pick(cfgs.get("scaled_b512_t80"), "whole_forward_frac_of_fp32_mfma_peak"),
            # north_star's table on this run's N GPUs (totals over all ranks; ms per step, frames/s, fraction of N x fp32-MFMA peak)
            "table_" + str(world) + "gpu": {k: [round(v["ms_per_step"], 4), round(v["frames_per_s"], 1), round(v["whole_forward_frac_of_fp32_mfma_peak"], 4)]
                                            if isinstance(v, dict) and "ms_per_step" in v else v
                                            for k, v in (extra.get("scaling_table") or {}).items()},
            "cpu_frames_per_s": cpu["value"] if cpu else None, "cpu_model": cpu.get("cpu_model") if cpu else None,
        }
        print(json.dumps(line))
    if use_pg:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
