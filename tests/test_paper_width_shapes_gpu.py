"""GPU tests of the tuned inference plans OFF the paper model: every member of the family the fused kernels accept (csrc/tip_fused.hip:
fused_supported; the table of tests/test_paper_width_schedule_cpu.py) — other depths (the layer loops' ends, the one-launch form of the
few-stream plan at 10 and 34 stages, its launch chain beyond), other RNN widths and no RNN (the encoders' plain-row output, rnn_ih_gemm,
the streaming recurrence at 1 .. 7 column blocks per wave, head_gemm at K = R / 256), other state widths (the head kernels' column
tails on either side of the register-resident kernel's 129 .. 131, no SBP columns, 223 of the 224 input columns) and the input width at
which the family ends — against the fp64 oracle, under the project's bound for a forward (tests/test_hip_parity.py: TOL_TIGHT).  The
oracle's own fp32 form sits 0.6e-6 .. 1.8e-6 from its fp64 form on these configurations at every depth: the bound leaves 10x over that."""
import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from tip_amd import lib as tlib
from oracle import oracle
from test_host_cpu import make_model, load_synth
from test_paper_width_schedule_cpu import CONFIGS, GROUPS, expected, expected_short, one
from test_reuse_gpu import _lockstep, _raw_frames
from test_schedule_cpu import strip
from test_stream_shapes_gpu import PLANS_119

pytestmark = pytest.mark.gpu
TOL_TIGHT = 2e-5   # tests/test_hip_parity.py:17: a forward against the fp64 oracle

PLAN_ID = {"general": tlib.TIP_PLAN_GENERAL, "fused": tlib.TIP_PLAN_FUSED, "fusedh": tlib.TIP_PLAN_FUSEDH, "fused2": tlib.TIP_PLAN_FUSED2,
           "fused1s": tlib.TIP_PLAN_FUSED1S, "fused1s2": tlib.TIP_PLAN_FUSED1S, "fused1s4": tlib.TIP_PLAN_FUSED1S,
           "latency": tlib.TIP_PLAN_LATENCY, "latency_chain": tlib.TIP_PLAN_LATENCY}
DEPTH = ["L1", "L2", "L7", "L8", "L12"]
WIDTH = ["S111", "S127", "S143n", "S147n", "S151n", "noRNN_L1_S111", "S135", "S143"]

# ---- fixtures: one model and one oracle batch per configuration (and window length), shared by every plan -------------------------
_models, _oracle_cache = {}, {}


def _group(name):
    return next(g for g, names in GROUPS.items() if name in names)


def _oracle_case(name, T):
    """Windows are independent: a plan tested on B windows uses the first B of the configuration's batch.  Nobody writes to it."""
    if (name, T) not in _oracle_cache:
        cfg = CONFIGS[name]
        B = (66 if T == 40 else 9) if _group(name) == "paper" and name != "L12" else (37 if T == 40 else 9)
        x_imu, x_s = synth.make_inputs(cfg, B, T, seed=len(name) + 7 * T)
        w = synth.make_weights(cfg, seed=0)
        yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
        for a in (x_imu, x_s, yo):
            a.setflags(write=False)
        _oracle_cache[(name, T)] = (cfg, w, x_imu, x_s, yo)
    return _oracle_cache[(name, T)]


def _model(name):
    if name not in _models:
        cfg = CONFIGS[name]
        m = make_model(cfg)
        load_synth(m, cfg, 0)
        _models[name] = m.cuda().eval()
    m = _models[name]
    _pin(m, "auto")
    return m


def _pin(m, plan):
    m.set_plan({"latency_chain": "latency"}.get(plan, plan))
    m._ensure_handle().set_option(tlib.TIP_OPT_NO_FLOW, 1 if plan == "latency_chain" else 0)


def _three(m, xi, xs, rows):
    with torch.no_grad():
        out = m(xi, xs).cpu().numpy(), m.forward_last(xi, xs).cpu().numpy(), m.forward_rows(xi, xs, rows).cpu().numpy()
    return out


def _check(name, plan, B, T, want):
    """One (configuration, plan, batch, window length): the schedule names `want`; full output, last row and chosen rows meet the
    oracle; the three forms agree bit for bit; a second run repeats the bits; no hand-off was lost."""
    cfg, w, x_imu, x_s, yo = _oracle_case(name, T)
    S = cfg["size_s"]
    assert B <= x_imu.shape[0]
    m = _model(name)
    h = m._ensure_handle()
    _pin(m, plan)
    try:
        assert strip(h.schedule(B, T)) == want, (name, plan, B, T)
        xi, xs = torch.tensor(x_imu[:B]).cuda(), torch.tensor(x_s[:B]).cuda()
        rows_np = np.random.RandomState(B + T).randint(0, T, size=B)
        rows = torch.tensor(rows_np, dtype=torch.int32, device="cuda")
        t0, n0 = tlib.spin_timeouts(), m.hip_forward_count()
        full, last, got = _three(m, xi, xs, rows)
        full2, last2, got2 = _three(m, xi, xs, rows)
        assert m.hip_forward_count() == n0 + 6, "the HIP path did not run"
        m.check_handoffs()
        assert tlib.spin_timeouts() == t0
        e_full = np.abs(full - yo[:B]).max()
        e_last = np.abs(last - yo[:B, -1]).max()
        e_rows = np.abs(got - yo[np.arange(B), rows_np]).max()
        print(f"paper-width {name} plan={plan} B={B} T={T}: full {e_full:.2e} last {e_last:.2e} rows {e_rows:.2e}")
        assert full.shape == (B, T, S) and last.shape == (B, S) and got.shape == (B, S)
        assert np.isfinite(full).all() and np.isfinite(last).all() and np.isfinite(got).all()
        assert e_full < TOL_TIGHT and e_last < TOL_TIGHT and e_rows < TOL_TIGHT, (name, plan, B, T, e_full, e_last, e_rows)
        # include/tip_hip.h, tip_forward_rows: bit-identical to tip_forward(...)[b, rows[b]] on the same plan, and with rows = T - 1
        # everywhere to the last-row form — so the last-row form is the full output's last row, on every plan
        assert np.array_equal(got, full[np.arange(B), rows_np]), (name, plan, B, T, "forward_rows != forward[b, rows[b]]")
        assert np.array_equal(last, full[:, -1]), (name, plan, B, T, "forward_last != forward[:, -1]")
        assert np.array_equal(full, full2) and np.array_equal(last, last2) and np.array_equal(got, got2), (name, plan, B, T, "run to run")
        return max(e_full, e_last, e_rows)
    finally:
        _pin(m, "auto")


def _refused(name, plan, B=3, T=40):
    cfg, w, x_imu, x_s, yo = _oracle_case(name, T)
    m = _model(name)
    _pin(m, plan)
    try:
        xi, xs = torch.tensor(x_imu[:B]).cuda(), torch.tensor(x_s[:B]).cuda()
        for call in (lambda: m(xi, xs), lambda: m.forward_last(xi, xs)):
            with pytest.raises(RuntimeError), torch.no_grad():
                call()
        torch.cuda.synchronize()
    finally:
        _pin(m, "auto")
    m.check_handoffs()


# ---- 1. rnn_hid_size 512: every plan of the paper model, at other depths and state widths --------------------------------------------
def _paper_cases():
    for name in GROUPS["paper"]:
        for plan, B40, B12 in PLANS_119:
            if name == "L12" and plan not in ("fusedh", "latency", "latency_chain"):
                continue          # twelve layers: image offsets past twice the paper's, on the two plans that walk them differently
            yield pytest.param(name, plan, B40, B12, id=f"{name}-{plan}")


@pytest.mark.parametrize("name,plan,B40,B12", list(_paper_cases()))
def test_every_paper_plan_at_other_depths_and_state_widths(name, plan, B40, B12):
    """general 5 | fused 7 | fusedh 7 | fused2 5 | fused1s2 66 | fused1s4 9 | latency 3 (one launch while 6 + 4 tf_layers <= 34, the
    chain beyond) | latency with TIP_OPT_NO_FLOW 3 | auto 66 windows of 40 rows, and the short-window plans at T = 12."""
    for T, B in ((40, B40), (12, B12)):
        if B == 0:
            continue
        want = (expected(B) if T == 40 else expected_short(B)) if plan == "auto" else one(B, PLAN_ID[plan])
        _check(name, plan, B, T, want)


@pytest.mark.parametrize("name", [n for n in GROUPS["paper"] if n != "L12"])
def test_full_window_plans_refuse_short_windows_off_the_paper_model(name):
    for plan in ("fused2", "fused1s2", "fused1s4"):
        _refused(name, plan, B=3, T=12)


# ---- 2. no RNN input term in the encoder: other RNN widths, no RNN -------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["general", "fused", "fusedh", "auto"])
@pytest.mark.parametrize("name", GROUPS["hybrid"])
def test_other_rnn_widths_and_no_rnn(name, plan):
    """The encoder leaves plain rows (not the RNN input term); rnn_ih_gemm, the streaming recurrence at rnn_hid_size / 64 column
    blocks per wave and head_gemm at K = rnn_hid_size (256 without an RNN) follow.  37 windows: three 16-window tiles, the last ragged.
    AUTO is the hybrid encoder at every batch."""
    for B, T in ((7, 40), (37, 40), (5, 12)):
        _check(name, plan, B, T, one(B, tlib.TIP_PLAN_FUSEDH if plan == "auto" else PLAN_ID[plan]))


@pytest.mark.parametrize("name", GROUPS["hybrid"])
def test_plans_that_need_the_rnn_input_term_refuse(name):
    for plan in ("fused2", "fused1s", "latency"):
        _refused(name, plan)


# ---- 3. more than 224 input columns: the family ends ---------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["general", "auto"])
@pytest.mark.parametrize("name", GROUPS["general"])
def test_wider_inputs_fall_back_to_the_general_plan(name, plan):
    for B, T in ((7, 40), (37, 40), (5, 12)):
        _check(name, plan, B, T, one(B, tlib.TIP_PLAN_GENERAL))


@pytest.mark.parametrize("name", GROUPS["general"])
def test_wider_inputs_are_refused_by_every_fused_plan(name):
    for plan in ("fused", "fusedh", "fused2", "fused1s", "latency"):
        _refused(name, plan)


# ---- 4. would a wrong kernel show?  (CPU only: the oracle against itself) -------------------------------------------------------------
@pytest.mark.parametrize("name", DEPTH)
def test_oracle_depth_sensitivity(name):
    """The oracle without the last layer's tensors is far from the oracle: a kernel that skips (or repeats) a layer cannot pass."""
    cfg, w, x_imu, x_s, yo = _oracle_case(name, 40)
    L = cfg["tf_layers"]
    short = type(w)((k, v) for k, v in w.items() if not k.startswith(f"tf_encode.layers.{L - 1}."))
    assert len(short) == len(w) - 12
    y = oracle.forward(dict(cfg, tf_layers=L - 1), short, x_imu[:3], x_s[:3], dtype=np.float64)
    d = np.abs(y - yo[:3]).max()
    print(f"paper-width {name}: |oracle without layer {L - 1} - oracle| = {d:.3f}")
    assert d > 100 * TOL_TIGHT


@pytest.mark.parametrize("name", WIDTH)
def test_oracle_last_column_is_not_zero(name):
    """A dropped tail column of the output projection would show: the last column's oracle values are not all within the bound of
    zero (they reach 100 x the bound)."""
    for T in (40, 12):
        yo = _oracle_case(name, T)[4]
        assert yo.shape[2] == CONFIGS[name]["size_s"]
        assert not (np.abs(yo[..., -1]) < TOL_TIGHT).all() and np.abs(yo[..., -1]).max() > 100 * TOL_TIGHT, (name, T)


# ---- 5. what the sweep found -----------------------------------------------------------------------------------------------------------
def test_training_forward_projects_every_state_column_at_143():
    """The register-resident output projection (csrc/tip_head.hip) keeps three columns of its ninth column block: it serves 129 .. 131
    state columns.  It used to accept up to 144 and left columns 131 .. N - 1 unwritten — on every inference plan at T = 40 (the S143n
    cases above: 1.05 from the oracle) and in the training forward, which calls the same launcher.  Both fall back to their GEMM now."""
    cfg, w, x_imu, x_s, yo = _oracle_case("S143n", 40)
    m = make_model(cfg)
    load_synth(m, cfg, 0)
    m = m.cuda().train()
    m.ENCODER_DROPOUT = 0.0
    n0 = m.hip_forward_count()
    y = m(torch.tensor(x_imu[:3]).cuda(), torch.tensor(x_s[:3]).cuda())
    assert m.hip_forward_count() == n0 + 1 and type(y.grad_fn).__name__.startswith("_HipTrainFunction"), type(y.grad_fn).__name__
    e = np.abs(y.detach().cpu().numpy() - yo[:3]).max()
    print(f"paper-width S143n training forward B=3 T=40: {e:.2e}")
    assert e < TOL_TIGHT, e


# ---- 6. the streaming ring at the layer loop's ends -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L1", "L7"])
def test_reuse_engine_equals_recomputation_at_other_depths(name):
    """StreamingEngine(reuse=True) == reuse=False bit for bit over 45 frames of 5 streams: the ring holds layer-0 rows, and at
    tf_layers = 1 layer 0 is also the LAST layer (its output feeds the RNN input term, not a next layer)."""
    m = _model(name)
    raw, s_init = _raw_frames(5, 45, 17)
    ref = tip_amd.streaming.StreamingEngine(m, s_init)
    eng = tip_amd.streaming.StreamingEngine(m, s_init, reuse=True)
    assert _lockstep(m, ref, eng, raw) == 1            # frame 44: the first full window
    m.check_handoffs()
