"""GPU parity tests: the HIP path (through the C-ABI) vs golden vectors captured from the reference and vs the
CPU oracle on the same seeded inputs.  Tolerance (north_star): 1e-4 max-abs, fp32, dropout disabled."""
import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from tip_amd import lib as tlib
from oracle import oracle
from conftest import cfg_for_tag, seed_for_tag
from test_host_cpu import make_model, load_synth

pytestmark = pytest.mark.gpu

TOL = 1e-4          # north_star: outputs within 1e-4 max-abs of the reference fp32 forward
TOL_TIGHT = 2e-5    # what fp32 MFMA actually achieves against the fp64 reference on these inputs


def _dev():
    assert torch.cuda.is_available(), "gpu-marked test needs an MI355X"
    return torch.device("cuda:0")


def _gpu_model(cfg, seed, **kw):
    m = make_model(cfg, **kw)
    w = load_synth(m, cfg, seed)
    return m.cuda().eval(), w


def _run(m, x_imu, x_s, last=False):
    n0 = m.hip_forward_count()
    with torch.no_grad():
        xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
        xi0, xs0 = xi.clone(), xs.clone()
        y = (m.forward_last if last else m)(xi, xs)
        torch.cuda.synchronize()
    assert m.hip_forward_count() == n0 + 1, "the HIP path did not run"
    assert torch.equal(xi, xi0) and torch.equal(torch.nan_to_num(xs, nan=7.0), torch.nan_to_num(xs0, nan=7.0)), \
        "inputs were modified (reference clones them, simple_transformer_with_state.py:63-64)"
    return y.cpu().numpy()


PLANS = ["general", "fused"]
ALL_PLANS = ["general", "fused", "latency", "fusedh"]


@pytest.mark.parametrize("plan", ALL_PLANS)
def test_golden_vectors(golden, plan):
    _dev()
    models = {}
    for tag, case in golden.items():
        if "mask" in tag:
            continue
        cfg = cfg_for_tag(tag)
        key = (tag.split("_B")[0])
        if plan != "general" and not tag.startswith("paper"):
            continue   # fused / latency plans specialise the paper configuration; other configs take the general plan
        if key not in models:
            models[key] = _gpu_model(cfg, seed_for_tag(tag))[0]
            models[key].set_plan(plan)
        y = _run(models[key], case["x_imu"], case["x_s"])
        e32 = np.abs(y - case["y32"]).max()
        e64 = np.abs(y - case["y64"]).max()
        assert np.isfinite(y).all(), tag
        assert e32 < TOL and e64 < TOL, (tag, plan, e32, e64)
        assert e64 < TOL_TIGHT, (tag, plan, e64)


@pytest.mark.parametrize("cluster", [1, 2, 4, 8, 16])
def test_rnn_cluster_variants(cluster):
    """Splitting an RNN window-tile over 1..16 cooperating workgroups (streamed or register-resident W_hh) must not
    change a single bit: every variant uses the same canonical k-summation order, so a stream's output cannot
    depend on how many streams share the launch (which is what picks the cluster size)."""
    cfg = synth.PAPER
    m, w = _gpu_model(cfg, 0)
    x_imu, x_s = synth.make_inputs(cfg, 37, 40, seed=11)
    m.set_plan("general", rnn_cluster=1)
    y1 = _run(m, x_imu, x_s)
    m.set_plan("general", rnn_cluster=cluster)
    yc = _run(m, x_imu, x_s)
    assert np.array_equal(y1, yc), np.abs(y1 - yc).max()
    for _ in range(5):
        assert np.array_equal(yc, _run(m, x_imu, x_s)), "hand-off race: run-to-run difference"
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
    assert np.abs(yc - yo).max() < TOL_TIGHT


@pytest.mark.parametrize("B,T", [(1, 1), (1, 40), (5, 12), (37, 40), (256, 40), (300, 40), (1030, 40), (2100, 8)])
def test_rnn_four_window_tiles(B, T):
    """AUTO's recurrence for rnn_hidden 512 (rnn_rows4_kernel: 4-window tiles on 4-workgroup clusters, 4x4x1 MFMAs) against the
    16-window kernels, which are pinned to the oracle above: same numbers up to summation order, for ragged tile counts (rows
    and whole tiles past the batch end are range-checked buffer accesses), 1 / 2 / 4 tiles per cluster and several rounds of
    them; a stream's result must not depend on its batch neighbours (bit-exact), nor on the run."""
    cfg = synth.PAPER
    m, w = _gpu_model(cfg, 0)
    x_imu, x_s = synth.make_inputs(cfg, min(B, 300), T, seed=21)
    reps = (B + x_imu.shape[0] - 1) // x_imu.shape[0]
    x_imu, x_s = np.tile(x_imu, (reps, 1, 1))[:B], np.tile(x_s, (reps, 1, 1))[:B]
    plan = "fusedh"
    m.set_plan(plan, rnn_cluster=16)
    y16 = _run(m, x_imu, x_s)
    m.set_plan(plan, rnn_cluster=tlib.TIP_RNN_CLUSTER_ROWS4)
    y4 = _run(m, x_imu, x_s)
    assert np.isfinite(y4).all()
    assert np.abs(y4 - y16).max() < 5e-6, np.abs(y4 - y16).max()
    m.set_plan(plan, rnn_cluster=0)                                   # AUTO picks the same kernel
    assert np.array_equal(y4, _run(m, x_imu, x_s))
    for _ in range(3):
        assert np.array_equal(y4, _run(m, x_imu, x_s)), "hand-off race: run-to-run difference"
    if B > 8:                                                         # batch neighbours: the last 5 streams alone
        assert np.array_equal(y4[-5:], _run(m, x_imu[-5:], x_s[-5:]))
    if B <= 64:
        yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
        assert np.abs(y4 - yo).max() < TOL_TIGHT


def test_random_shapes_and_nan_patterns_auto_plan():
    """Randomised sweep of the AUTO plan (whatever kernels it picks per shape) against the fp64 oracle: 24 seeded draws of
    (B <= 72, T <= 40) with NaNs scattered through x_s (the reference scrubs them, :65) — a few per window, whole rows, whole
    windows — and, through forward_last, the row the runner consumes."""
    cfg = synth.PAPER
    m, w = _gpu_model(cfg, 3)
    m.set_plan("auto")
    rng = np.random.RandomState(2026)
    for draw in range(24):
        B = int(rng.choice([1, 2, 3, 5, 8, 13, 21, 34, 55, 65, 72]))
        T = int(rng.randint(1, 41))
        x_imu, x_s = synth.make_inputs(cfg, B, T, seed=1000 + draw)
        mode = draw % 4
        if mode == 1:
            x_s[rng.rand(*x_s.shape) < 0.05] = np.nan
        elif mode == 2:
            x_s[rng.randint(B), rng.randint(T), :] = np.nan
        elif mode == 3:
            x_s[rng.randint(B)] = np.nan
        y = _run(m, x_imu, x_s)
        yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
        assert np.isfinite(y).all(), (draw, B, T)
        assert np.abs(y - yo).max() < TOL_TIGHT, (draw, B, T, mode, np.abs(y - yo).max())
        yl = _run(m, x_imu, x_s, last=True)
        assert np.abs(yl.reshape(B, -1) - yo[:, -1]).max() < TOL_TIGHT, (draw, B, T, "last row")


@pytest.mark.parametrize("plan", ALL_PLANS)
@pytest.mark.parametrize("B,T", [(1, 1), (1, 40), (3, 2), (17, 39), (64, 40), (130, 7), (300, 33)])
def test_vs_oracle_shapes(B, T, plan):
    cfg = synth.PAPER
    if plan == "latency" and B > 64:
        pytest.skip("latency plan serves <= 64 concurrent streams")
    m, w = _gpu_model(cfg, 1)
    m.set_plan(plan)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=100 + B)
    y = _run(m, x_imu, x_s)
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float32)
    assert y.shape == (B, T, cfg["size_s"])
    assert np.abs(y - yo).max() < TOL_TIGHT, np.abs(y - yo).max()


@pytest.mark.parametrize("B", [1, 2, 5, 64, 257])
def test_two_window_plan_bit_identical_to_one_window(B):
    """"fused2" carries two windows per workgroup (80 rows = 5 MFMA row blocks, no padding).  Same packed image, same
    per-element summation order, so it must reproduce the one-window plan bit for bit, for odd and even B."""
    cfg = synth.PAPER
    m, w = _gpu_model(cfg, 2)
    x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=300 + B, nan_frac=0.01)
    m.set_plan("fused")
    y1 = _run(m, x_imu, x_s)
    m.set_plan("fused2")
    y2 = _run(m, x_imu, x_s)
    assert np.array_equal(y1, y2), np.abs(y1 - y2).max()
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float32)
    assert np.abs(y2 - yo).max() < TOL_TIGHT
    if B <= 5:   # T != 40 is outside the two-window plan: explicit request is an error, not a silent fallback
        with pytest.raises(RuntimeError):
            with torch.no_grad():
                m(torch.tensor(x_imu[:, :17]).cuda(), torch.tensor(x_s[:, :17]).cuda())


def test_two_window_plan_golden_and_auto_selection(golden):
    cfg = synth.PAPER
    models = {}
    for tag, case in golden.items():
        if not tag.startswith("paper") or "mask" in tag or case["x_imu"].shape[1] != 40:
            continue
        key = tag.split("_B")[0]
        if key not in models:
            models[key] = _gpu_model(cfg, seed_for_tag(tag))[0]
            models[key].set_plan("fused2")
        y = _run(models[key], case["x_imu"], case["x_s"])
        assert np.abs(y - case["y64"]).max() < TOL_TIGHT, tag
    # AUTO weighs rounds of the two-window kernel (2 x #CUs windows each, 1.065 ms) against rounds of the hybrid one-window
    # kernel (#CUs windows, 0.553 ms): the result is bit-identical to the explicit plan it picked.  A remainder
    # behind whole rounds goes to the latency plan (<= 32 windows) or the window-split encoder as a second launch sequence (round 4): bit-identical to the two parts run alone.
    m, _ = _gpu_model(cfg, 0)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for B, picked, rem in ((ncu + 200, "fused2", 0), (2 * ncu + 200, "fusedh", 0), (3 * ncu + 205, "fused2", 0), (ncu - 1, "fusedh", 0),
                           (65, "fused1s", 0), (ncu // 2, "fused1s", 0), (ncu // 2 + 1, "fusedh", 0), (49, "fused1s", 0), (33, "fused1s", 0), (32, "latency", 0),
                           (ncu + 3, "fusedh", 3), (2 * ncu + 3, "fused2", 3), (3 * ncu + 5, "fusedh", 5), (ncu + 100, "fusedh", 100),
                           (ncu + 40, "fusedh", 40), (4 * ncu + 40, "fused2", 40)):
        x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=77)
        m.set_plan("auto")
        ya = _run(m, x_imu, x_s)
        m.set_plan(picked)
        bm = B - rem
        parts = [_run(m, x_imu[:bm], x_s[:bm])]
        if rem:
            m.set_plan("latency" if rem <= 32 else "fused1s")
            parts.append(_run(m, x_imu[bm:], x_s[bm:]))
        assert np.array_equal(ya, np.concatenate(parts)), (B, picked, rem)


@pytest.mark.parametrize("B,T", [(1, 40), (5, 40), (3, 33), (2, 36), (256, 40), (300, 40)])
def test_hybrid_row_tiling_plan(B, T):
    """"fusedh": rows 0-31 on 16x16x4 MFMAs exactly as "fused" (bit-identical: causality keeps later rows out of them), rows
    32-39 on 4x4x1 MFMAs fed by the same weight fragments (summation order differs: tolerance).  Batch independence and
    run-to-run determinism hold within the plan; no inter-workgroup hand-off in the encoder at all."""
    cfg = synth.PAPER
    m, w = _gpu_model(cfg, 1)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=700 + B + T, nan_frac=0.01)
    m.set_plan("fusedh")
    y = _run(m, x_imu, x_s)
    assert np.array_equal(y, _run(m, x_imu, x_s))
    m.set_plan("fused")
    yf = _run(m, x_imu, x_s)
    # the encoder rows 0..31 are the same instructions; the recurrence then carries them unchanged up to step 31
    assert np.array_equal(y[:, :32], yf[:, :32])
    assert np.abs(y - yf).max() < 5e-6
    if B <= 5:
        yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
        assert np.abs(y - yo).max() < TOL_TIGHT
    else:
        yo = oracle.forward(cfg, w, x_imu[:8], x_s[:8], dtype=np.float64)
        assert np.abs(y[:8] - yo).max() < TOL_TIGHT
        sel = np.array([0, 1, 17, B // 2, B - 1])
        m.set_plan("fusedh")
        assert np.array_equal(_run(m, x_imu[sel], x_s[sel]), y[sel])
        assert np.array_equal(_run(m, x_imu, x_s, last=True), y[:, -1])


def test_last_row_only_equals_full():
    cfg = synth.PAPER
    m, _ = _gpu_model(cfg, 0)
    x_imu, x_s = synth.make_inputs(cfg, 33, 40, seed=5)
    y = _run(m, x_imu, x_s)
    yl = _run(m, x_imu, x_s, last=True)
    assert yl.shape == (33, cfg["size_s"])
    assert np.array_equal(y[:, -1], yl)


def test_streaming_growth_T_1_to_40():
    """RTRunnerMin warm-up: T grows 1,2,...,40 (real_time_runner_minimal.py:131); every call consumes row T-1."""
    cfg = synth.PAPER
    m, w = _gpu_model(cfg, 0)
    x_imu, x_s = synth.make_inputs(cfg, 1, 40, seed=9)
    yfull = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
    for T in list(range(1, 41)):
        yl = _run(m, x_imu[:, :T], x_s[:, :T], last=True)
        # causal: the prefix run reproduces row T-1 of the full run
        assert np.abs(yl[0] - yfull[0, T - 1]).max() < TOL_TIGHT, T


def test_keep_mask_semantics(golden):
    """TIP_FWD_KEEP_MASK: x_s * mask / (1-p) == nn.Dropout with the same Bernoulli draw (golden from the reference)."""
    case = golden["paper_mask_s0_B2_T40"]
    cfg = synth.PAPER
    m, _ = _gpu_model(cfg, 0)
    h = m._ensure_handle()
    m.refresh_packed(torch.device("cuda:0"))
    xi, xs = torch.tensor(case["x_imu"]).cuda(), torch.tensor(case["x_s"]).cuda()
    mask = torch.tensor(case["mask"]).cuda()
    p = float(case["p"][0])
    y = torch.empty(2, 40, 131, device="cuda")
    ws = torch.empty(h.workspace_bytes(2, 40), dtype=torch.uint8, device="cuda")
    for plan in (tlib.TIP_PLAN_AUTO, tlib.TIP_PLAN_FUSED, tlib.TIP_PLAN_FUSED2):
        h.set_option(tlib.TIP_OPT_PLAN, plan)
        y.zero_()
        h.forward(xi.data_ptr(), xs.data_ptr(), y.data_ptr(), 2, 40, tlib.TIP_FWD_KEEP_MASK, mask.data_ptr(),
                  1.0 / (1.0 - p), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.abs(y.cpu().numpy() - case["y64"]).max() < TOL_TIGHT, plan
    h.set_option(tlib.TIP_OPT_PLAN, tlib.TIP_PLAN_AUTO)


def test_past_state_dropout_is_live_in_eval():
    """The reference's fresh nn.Dropout (:77) is stochastic even under .eval(): two calls differ; p=0 calls agree."""
    cfg = synth.TINY
    m, _ = _gpu_model(cfg, 0, p_state=0.8)
    x_imu, x_s = synth.make_inputs(cfg, 4, 20, seed=2)
    a, b = _run(m, x_imu, x_s), _run(m, x_imu, x_s)
    assert np.abs(a - b).max() > 1e-3
    m0, _ = _gpu_model(cfg, 0, p_state=0.0)
    a, b = _run(m0, x_imu, x_s), _run(m0, x_imu, x_s)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("plan", PLANS)
def test_properties_at_full_size(plan):
    """BASELINE sizes (B=1024 streams per GPU, T=40): batch independence (a stream's output does not depend on
    which other streams share the launch), NaN scrub (:65), root-velocity columns ignored (:75)."""
    cfg = synth.PAPER
    m, _ = _gpu_model(cfg, 0)
    m.set_plan(plan)
    B = 1024
    x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=77)
    y = _run(m, x_imu, x_s)
    assert np.isfinite(y).all()
    sel = np.array([0, 1, 15, 16, 17, 255, 256, 511, 1000, 1023])
    ysub = _run(m, x_imu[sel], x_s[sel])
    assert np.array_equal(y[sel], ysub)
    xs2 = np.nan_to_num(x_s, nan=0.0)
    xs2[:, :, 108:111] = 3.25
    y2 = _run(m, x_imu, xs2)
    assert np.array_equal(y, y2)
    # sharding == concatenation (what bench.py --gpus N relies on): two half-batches reproduce the full batch
    ya, yb = _run(m, x_imu[:512], x_s[:512]), _run(m, x_imu[512:], x_s[512:])
    assert np.array_equal(np.concatenate([ya, yb]), y)


def test_scaled_config_reduced_depth():
    """BASELINE configs[4] widths (d=1024, ffn=4096, dh=64, T=80) at 2 layers so the oracle finishes in seconds."""
    cfg = dict(synth.SCALED, tf_layers=2)
    m, w = _gpu_model(cfg, 0)
    x_imu, x_s = synth.make_inputs(cfg, 3, 80, seed=4)
    y = _run(m, x_imu, x_s)
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
    assert np.abs(y - yo).max() < TOL_TIGHT, np.abs(y - yo).max()


def _pgemm_launches():
    import ctypes
    n = ctypes.c_ulonglong()
    assert tlib.load().tip_debug_pgemm_launches(ctypes.byref(n)) == 0
    return n.value


def test_scaled_width_takes_the_panel_gemm():
    """BASELINE configs[4] widths on the kernel the scaled-config bench numbers come from: d=1024 / ffn=4096 / T=80 with
    M = B*T = 400 >= 320 rows, so every big linear (QKV, out-proj, FFN) runs `pgemm_kernel` (asserted through the launch
    counter), at 2 layers so the f64 oracle finishes in seconds."""
    cfg = dict(synth.SCALED, tf_layers=2)
    m, w = _gpu_model(cfg, 0)
    x_imu, x_s = synth.make_inputs(cfg, 5, 80, seed=14)
    n0 = _pgemm_launches()
    y = _run(m, x_imu, x_s)
    assert _pgemm_launches() - n0 == 4 * cfg["tf_layers"], "the panel GEMM did not serve the four linears of every layer"
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
    assert np.abs(y - yo).max() < TOL_TIGHT, np.abs(y - yo).max()
    # the LDS-tiled kernel on the same shapes (M < 320 rows) agrees to summation-order noise
    y3 = _run(m, x_imu[:3], x_s[:3])
    assert np.abs(y3 - y[:3]).max() < 5e-6


def test_scaled_config_full_depth_per_gpu_share():
    """BASELINE configs[4], the per-GPU share as bench.py --config scaled512 times it: 12 layers, d=1024, ffn=4096, dh=64,
    T=80, B=512 (40 960 rows; panel GEMM everywhere).  Two windows of the batch against the oracle (a window's result does
    not depend on its batch neighbours, which the next asserts establish bit-exactly at this size), then the
    size-independent properties: shard == concatenation, NaN scrub (:65), root-velocity columns ignored (:75)."""
    cfg = synth.SCALED
    m, w = _gpu_model(cfg, 0)
    B, T = 512, 80
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=44)
    n0 = _pgemm_launches()
    y = _run(m, x_imu, x_s)
    assert _pgemm_launches() - n0 == 4 * cfg["tf_layers"]
    assert y.shape == (B, T, cfg["size_s"]) and np.isfinite(y).all()
    sel = np.array([0, 511])
    yo = oracle.forward(cfg, w, x_imu[sel], x_s[sel], dtype=np.float32)
    assert np.abs(y[sel] - yo).max() < TOL_TIGHT, np.abs(y[sel] - yo).max()
    ya, yb = _run(m, x_imu[:256], x_s[:256]), _run(m, x_imu[256:], x_s[256:])
    assert np.array_equal(np.concatenate([ya, yb]), y)
    xs2 = np.nan_to_num(x_s, nan=0.0)
    xs2[:, :, 108:111] = -7.5
    assert np.array_equal(_run(m, x_imu, xs2), y)
    yl = _run(m, x_imu, x_s, last=True)
    assert np.array_equal(yl, y[:, -1])


def test_auto_plan_at_the_bench_batch_vs_oracle():
    """B = 256, T = 40, plan AUTO — the exact launch bench.py times (pair-split encoder + 16-workgroup RNN clusters) —
    compared directly with the oracle, all 256 windows."""
    cfg = synth.PAPER
    m, w = _gpu_model(cfg, 0)
    m.set_plan("auto")
    x_imu, x_s = synth.make_inputs(cfg, 256, 40, seed=1234)      # bench.py's inputs
    t0 = tlib.spin_timeouts()
    y = _run(m, x_imu, x_s)
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float32)
    assert np.abs(y - yo).max() < TOL_TIGHT, np.abs(y - yo).max()
    assert tlib.spin_timeouts() == t0


def test_load_state_dict_refreshes_packed_image():
    cfg = synth.TINY
    m, w0 = _gpu_model(cfg, 0)
    x_imu, x_s = synth.make_inputs(cfg, 2, 10, seed=1)
    y0 = _run(m, x_imu, x_s)
    w1 = synth.make_weights(cfg, seed=5)
    m.load_state_dict({k: torch.tensor(v) for k, v in w1.items()})
    y1 = _run(m, x_imu, x_s)
    yo = oracle.forward(cfg, w1, x_imu, x_s, dtype=np.float64)
    assert np.abs(y1 - yo).max() < TOL_TIGHT and np.abs(y1 - y0).max() > 1e-3


def test_eval_mode_with_autograd_uses_hip_forward_and_torch_backward():
    """The reference's runners call the model with autograd enabled (real_time_runner_minimal.py:149-150 ends in
    .detach()).  In .eval() mode the forward values must still come from the HIP kernels, and .backward() must work."""
    cfg = synth.TINY
    m, _ = _gpu_model(cfg, 0)
    x_imu, x_s = synth.make_inputs(cfg, 3, 12, seed=6)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    with torch.no_grad():
        y_ng = m(xi, xs)
    n0 = m.hip_forward_count()
    y = m(xi, xs)                      # grad enabled, parameters require grad
    assert m.hip_forward_count() == n0 + 1 and y.requires_grad
    assert torch.equal(y.detach(), y_ng)
    y.square().sum().backward()
    g_hip = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad()
    y2 = m._forward_torch_ops(xi, xs)  # pure torch-op reference for the gradients
    y2.square().sum().backward()
    for k, p in m.named_parameters():
        assert torch.allclose(g_hip[k], p.grad, rtol=1e-3, atol=1e-4), k
    # .train() mode + autograd -> torch-op composite (encoder dropout p=0.1 live, like the reference)
    m.train()
    n1 = m.hip_forward_count()
    with pytest.warns(UserWarning):
        yt = m(xi, xs)
    assert m.hip_forward_count() == n1 and yt.requires_grad
    assert (yt.detach() - y_ng).abs().max() > 1e-3   # dropout makes it differ


def test_latency_plan_is_deterministic_and_batch_independent():
    """The latency plan (auto for B <= 64): run-to-run identical (granule hand-off has no race) and a stream's result
    does not depend on its neighbours within the plan."""
    cfg = synth.PAPER
    m, w = _gpu_model(cfg, 0)
    m.set_plan("latency")
    x_imu, x_s = synth.make_inputs(cfg, 24, 40, seed=21)
    y = _run(m, x_imu, x_s)
    for _ in range(5):
        assert np.array_equal(y, _run(m, x_imu, x_s))
    y1 = _run(m, x_imu[7:8], x_s[7:8])
    assert np.array_equal(y[7:8], y1)
    yl = _run(m, x_imu, x_s, last=True)
    assert np.array_equal(yl, y[:, -1])
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
    assert np.abs(y - yo).max() < TOL_TIGHT


def test_cluster_handoffs_under_uneven_load():
    """Race screen for the inter-workgroup hand-offs (RNN clusters, GEMV granules): results must stay bit-identical
    while a second stream keeps a varying subset of CUs busy, so cluster members are dispatched late / unevenly and
    consumers run with warm L1s (cdna_hip_programming.md, Guideline 16: "test every hand-off under UNEVEN load")."""
    cfg = synth.PAPER
    m, _ = _gpu_model(cfg, 0)
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    # ("latency", 40): the few-stream plan's launch CHAIN (24 < B <= 64) with its GEMV recurrence clusters.  The ONE-launch form
    # (B <= 24) has a stronger requirement than co-residency — every workgroup of a window on the window's XCD — which another
    # stream's kernels can break: its contract under such load is "exact or flagged", test_one_launch_form_under_foreign_stream_load
    cases = [("fused", 200), ("fused", 40), ("latency", 40), ("fused2", 600)]
    cases += [("auto", 256)]   # the bench launch: hybrid one-window encoder + 16-workgroup RNN clusters
    if ncu >= 256:
        cases += [("fused1s2", 100), ("fused1s4", 60)]
    for plan, B in cases:
        m.set_plan(plan)
        x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=31)
        xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
        with torch.no_grad():
            ref = m(xi, xs).clone()
            torch.cuda.synchronize()
            for it in range(25):
                with torch.cuda.stream(side):
                    for _ in range(1 + it % 4):
                        b = a[: 512 * (1 + it % 7)] @ a      # different CU footprints and durations
                y = m(xi, xs)
                torch.cuda.synchronize()
                assert torch.equal(y, ref), (plan, B, it)


@pytest.mark.handoff_fault     # (hand-off waits MAY give up here: that is the contract under test, the autouse counter check does not apply)
@pytest.mark.parametrize("B", [1, 9, 24])
def test_one_launch_form_under_foreign_stream_load(B):
    """The one-launch few-stream form (lat_flow_kernel, B <= 24) places every workgroup of a window on the window's XCD by the
    dispatcher's round-robin rule (id mod 8) and hands activations over through that XCD's L2.  Kernels of ANOTHER stream running
    beside it can break the rule (measured with this load: no loss in 400 forwards at B = 1 and 3, 1 at B = 9, 53 at B = 24); a
    workgroup that finds a producer on another XCD gives up at once.  The contract: every forward is either bit-identical to the
    undisturbed one or NaN-poisoned AND reported (TipHandoffError at the next call) — never finite-but-different; and with
    TIP_OPT_AUTO_DEMOTE (the default) the handle then moves to the plans without hand-offs and keeps running."""
    cfg = synth.PAPER
    m, _ = _gpu_model(cfg, 0)
    h = m._ensure_handle()
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=31)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    h.set_option(tlib.TIP_OPT_AUTO_DEMOTE, 0)
    lost = reported = 0
    with torch.no_grad():
        ref = m(xi, xs).clone()
        torch.cuda.synchronize()
        pending = False                     # a lost launch whose report has not been seen yet
        for it in range(40):
            with torch.cuda.stream(side):
                for _ in range(1 + it % 4):
                    _ = a[: 512 * (1 + it % 7)] @ a
            try:
                y = m(xi, xs)
            except tlib.TipHandoffError:
                assert pending, "a hand-off error without a lost launch in front of it"
                h.check_clear()
                pending, reported = False, reported + 1
                continue
            torch.cuda.synchronize()
            assert not pending, "the call after a lost launch did not report it"
            if torch.equal(y, ref):
                continue
            assert bool(torch.isnan(y).any()), (B, it, "finite but different")
            lost, pending = lost + 1, True
        torch.cuda.synchronize()
        side.synchronize()
        if pending:
            with pytest.raises(tlib.TipHandoffError):
                m(xi, xs)
            h.check_clear()
            reported += 1
        assert reported == lost
        # undisturbed again: exact
        assert torch.equal(m(xi, xs), ref)
    h.set_option(tlib.TIP_OPT_AUTO_DEMOTE, 1)
    print(f"one-launch form, B = {B}: {lost} of 40 forwards lost under foreign-stream load, all reported")


def test_two_forwards_in_flight_on_two_streams():
    """Two forwards of the AUTO plan (cooperating RNN clusters) issued back to back on two HIP streams, with no host
    synchronisation in between, 40 times over: the library serialises them on the device (CoopSerial, tip_internal.h) — without
    that each could hold half of the CUs and starve the other's cluster partners (a ~1 s spin, NaN poison, TipHandoffError).
    Results are bit-identical to the single-stream run, and two module instances (two handles) are serialised as well."""
    cfg = synth.PAPER
    m, _ = _gpu_model(cfg, 0)
    m2, _ = _gpu_model(cfg, 0)
    m.set_plan("auto")
    m2.set_plan("auto")
    xa = [torch.tensor(v).cuda() for v in synth.make_inputs(cfg, 256, 40, seed=61)]
    xb = [torch.tensor(v).cuda() for v in synth.make_inputs(cfg, 200, 40, seed=62)]
    with torch.no_grad():
        ya0, yb0 = m(*xa).clone(), m(*xb).clone()
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        for it in range(40):
            mb = m2 if it % 2 else m
            with torch.cuda.stream(s1):
                ya = m(*xa)
            with torch.cuda.stream(s2):
                yb = mb(*xb)
            if it % 8 == 7:
                torch.cuda.synchronize()
                assert torch.equal(ya, ya0) and torch.equal(yb, yb0), it
        torch.cuda.synchronize()
        assert torch.equal(ya, ya0) and torch.equal(yb, yb0)
    m.check_handoffs()
    m2.check_handoffs()


@pytest.mark.parametrize("D,H,F,L,R,with_rnn,acc,B,T", [
    (64, 8, 48, 1, 64, True, True, 3, 5),       # d_head 8, narrow FFN, one layer
    (128, 4, 320, 2, 192, True, True, 5, 13),    # d_head 32 (attention scale applied in-kernel, not folded)
    (256, 4, 512, 1, 128, True, False, 2, 17),   # d_head 64, no acc-sum columns
    (192, 12, 208, 3, 0, False, True, 4, 9),     # no RNN: linear maps d_model -> size_s directly
    (512, 16, 1024, 1, 512, True, True, 18, 60),  # d_head 32, T=60, register-resident RNN path (R=512)
])
def test_general_plan_configuration_sweep(D, H, F, L, R, with_rnn, acc, B, T):
    """The general plan claims any configuration with d_model,ffn % 16 == 0, d_head in {8,16,32,64}, rnn % 64 == 0."""
    cfg = dict(input_size_imu=72, size_s=131, rnn_hid_size=R if with_rnn else 64, tf_hid_size=F, tf_in_dim=D, n_heads=H,
               tf_layers=L, with_rnn=with_rnn, with_acc_sum=acc)
    m, w = _gpu_model(cfg, 2)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=40 + D)
    y = _run(m, x_imu, x_s)
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
    assert y.shape == yo.shape and np.abs(y - yo).max() < TOL_TIGHT, np.abs(y - yo).max()
    yl = _run(m, x_imu, x_s, last=True)
    assert np.array_equal(yl, y[:, -1])


@pytest.mark.parametrize("cfgname", ["paper", "tiny", "scaled2", "no_rnn", "no_acc_sum", "size_s_119", "train_default"])
def test_device_packer_builds_the_same_image_as_the_host_packer(cfgname):
    """tip_pack_weights_device (pack_ops_kernel) vs tip_pack_weights (a host loop): both read ONE description of the packed
    layout and its folds — the PackOp list of csrc/tip_pack.hip — and share the function that gives an element's value
    (pack_row + pack_value); the kernel decodes the storage order from the element index, the host walks rows.  They must
    agree bit for bit.  What the description itself says is pinned on the CPU: test_packed_image_matches_the_pinned_digests
    (tests/test_host_cpu.py) holds the host's bytes, for these seven configurations and seed, to the digests of the
    hand-written host packer that preceded it.  So: device == host == that packer."""
    cfg = {"paper": synth.PAPER, "tiny": synth.TINY, "scaled2": dict(synth.SCALED, tf_layers=2),
           "no_rnn": dict(synth.PAPER, with_rnn=False), "no_acc_sum": dict(synth.PAPER, with_acc_sum=False),
           "size_s_119": dict(synth.PAPER, size_s=119), "train_default": synth.TRAIN_DEFAULT}[cfgname]
    m, _ = _gpu_model(cfg, 3)
    host = m.pack_host()
    dev = m.pack_device().cpu()
    assert host.numel() == dev.numel()
    a, b = host.view(torch.float32), dev.view(torch.float32)
    assert torch.equal(a, b), int((a != b).sum())
    # and the module uses it: a parameter change reaches the kernels without a host pack
    x_imu, x_s = synth.make_inputs(cfg, 2, 9, seed=1)
    y0 = _run(m, x_imu, x_s)
    with torch.no_grad():
        m.linear.bias.add_(1.0)
    y1 = _run(m, x_imu, x_s)
    assert np.allclose(y1 - y0, 1.0, atol=1e-5)


def test_empty_inputs_raise_like_the_reference():
    """The reference raises RuntimeError on an empty batch or an empty window (its head-interleave reshape fails,
    simple_transformer_with_state.py:88); so does the drop-in."""
    cfg = synth.PAPER
    m, _ = _gpu_model(cfg, 0)
    with torch.no_grad():
        for B, T in ((0, 40), (2, 0)):
            with pytest.raises(RuntimeError):
                m(torch.zeros(B, T, 90).cuda(), torch.zeros(B, T, 131).cuda())
        y = m(torch.zeros(2, 41, 90).cuda(), torch.zeros(2, 41, 131).cuda())     # past the paper's 40 frames: general plan
        assert y.shape == (2, 41, 131) and torch.isfinite(y).all()


@pytest.mark.parametrize("cfgname,B,T", [("paper", 2, 129), ("paper", 3, 200), ("scaled2", 2, 150), ("tiny", 2, 333)])
def test_any_window_length(cfgname, B, T):
    """The reference builds its causal mask for ANY window length (simple_transformer_with_state.py:56-58,85): no t_max.  Past
    T = 128 (the matrix-core attention's reach) the general plan runs the key-tiled attention; d_head 16 / 64 / 32 here."""
    cfg = {"paper": synth.PAPER, "scaled2": dict(synth.SCALED, tf_layers=2), "tiny": synth.TINY}[cfgname]
    m, w = _gpu_model(cfg, 0)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=50 + T)
    y = _run(m, x_imu, x_s)
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
    assert y.shape == yo.shape and np.abs(y - yo).max() < TOL_TIGHT, np.abs(y - yo).max()
    assert np.array_equal(_run(m, x_imu, x_s, last=True), y[:, -1])
    # causality at this length: a shorter prefix reproduces its rows
    Tp = T - 37
    yp = _run(m, x_imu[:, :Tp], x_s[:, :Tp])
    assert np.abs(yp - y[:, :Tp]).max() < 5e-6


def test_very_long_window_properties():
    """T = 4096 (oracle too slow): finite, deterministic, and the first 300 rows equal a 300-frame run (causality)."""
    cfg = synth.PAPER
    m, _ = _gpu_model(cfg, 0)
    x_imu, x_s = synth.make_inputs(cfg, 1, 4096, seed=3)
    y = _run(m, x_imu, x_s)
    assert y.shape == (1, 4096, 131) and np.isfinite(y).all()
    assert np.array_equal(y, _run(m, x_imu, x_s))
    y300 = _run(m, x_imu[:, :300], x_s[:, :300])
    assert np.abs(y300 - y[:, :300]).max() < 5e-6


def test_library_refuses_the_retired_plans():
    """Round 6: the pair-split plan (5) and the split-fp16 plans (7, 8) are gone from every build; the library says so at set_option
    time (host: RuntimeError); 9 (the persistent latency kernel, round 5) stays reserved; option 6 (the split-fp16 image sections) is
    no option any more."""
    m, _ = _gpu_model(synth.PAPER, 0)
    h = m._ensure_handle()
    for plan in (5, 7, 8):
        assert tlib.load().tip_set_option(h._h, tlib.TIP_OPT_PLAN, plan) == tlib.TIP_ERR_UNSUPPORTED_CONFIG
    assert tlib.load().tip_set_option(h._h, tlib.TIP_OPT_PLAN, 9) < 0          # reserved value
    assert tlib.load().tip_set_option(h._h, 6, 1) < 0
    for name in ("fused2s", "fused16", "general16"):
        with pytest.raises(RuntimeError):
            m.set_plan(name)
    m.set_plan("auto")


@pytest.mark.parametrize("B", [65, 256])
def test_fuse_head_option_is_reserved_and_without_effect(B):
    """TIP_OPT_FUSE_HEAD is reserved since round 5 (accepted, ignored): same launches, same bits either way; row T-1 of the full
    output equals the last-row-only output."""
    cfg = synth.PAPER
    m, w = _gpu_model(cfg, 0)
    h = m._ensure_handle()
    x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=123 + B, nan_frac=0.01)
    m.set_plan("auto", profile=1)
    y0 = _run(m, x_imu, x_s)
    assert "out_linear" in [n for n, _, _ in m.profile_read()]
    h.set_option(tlib.TIP_OPT_FUSE_HEAD, 1)
    m.set_plan("auto", profile=1)
    y1 = _run(m, x_imu, x_s)
    assert "out_linear" in [n for n, _, _ in m.profile_read()]
    assert np.isfinite(y1).all() and np.array_equal(y0, y1)
    assert np.array_equal(y1[:, -1], _run(m, x_imu, x_s, last=True))
    h.set_option(tlib.TIP_OPT_FUSE_HEAD, 0)
