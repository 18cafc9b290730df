"""GPU: the deployed forward (tip_forward_live / model.forward_live: encoder dropout and past-state keep mask live, no stash, any
batch) against the fp64 training oracle with the masks rebuilt from the documented hash, against tip_train_forward, and its device
seeds (seeds_dev, tip_seeds_next).  Bounds are the project's own for the same comparisons (tests/test_train_gpu.py: 2e-5)."""
import ctypes

import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from tip_amd import lib as tlib
from oracle import train_oracle
from test_host_cpu import make_model, load_synth

pytestmark = pytest.mark.gpu

TOL = 2e-5                 # tests/test_train_gpu.py:144 — the same comparison; one flipped keep decision moves outputs by >= 1e-2
P_STATE, P_DROP = 0.8, 0.1
STATE_SITE = 0xFFFFFFF0
SEEDS = (123456789, 987654321)      # (encoder seed, state seed)


def _f32(p):
    """The probability as the C-ABI receives it (a float): the thresholds are floor(float(p) * 2^32)."""
    return float(np.float32(p))


def _model(cfg, p_state=P_STATE, train=True, seed=3):
    assert torch.cuda.is_available()
    m = make_model(cfg, p_state=p_state)
    w = load_synth(m, cfg, seed)
    m = m.cuda()
    m = m.train() if train else m.eval()
    m.ENCODER_DROPOUT = P_DROP
    return m, w


def _state_mask(state_seed, p_state, B, T, S, window_ids=None):
    """keep (0 / 1) of x_s [B,T,S]: element ((win * T + row) * S + col) at site 0xFFFFFFF0 (include/tip_hip.h, tip_draw_keep_mask)."""
    if p_state <= 0.0:
        return None
    per = T * S
    wid = np.arange(B, dtype=np.int64) if window_ids is None else np.asarray(window_ids, dtype=np.int64)
    idx = (wid[:, None] * per + np.arange(per, dtype=np.int64)[None, :]).reshape(-1)
    sc = train_oracle.drop_scale(state_seed, STATE_SITE, idx.size, _f32(p_state), idx)
    return (sc > 0).astype(np.float64).reshape(B, T, S)


def _oracle(cfg, w, x_imu, x_s, seeds, p_drop, p_state, window_ids=None):
    B, T, S = x_s.shape
    mask = _state_mask(seeds[1], p_state, B, T, S, window_ids)
    params = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in w.items()}
    scale = 1.0 / (1.0 - _f32(p_state)) if p_state > 0 else 1.0
    return train_oracle.forward(cfg, params, x_imu, x_s, keep_mask=mask, keep_scale=scale, p_drop=_f32(p_drop) if p_drop > 0 else 0.0,
                                seed=seeds[0], window_ids=window_ids).numpy()


def _stages(m):
    return {n for n, _, _ in m.profile_read()}


@pytest.mark.parametrize("T", [40, 7])
@pytest.mark.parametrize("B", [5, 70, 300])
def test_parity_with_masks_live(B, T):
    """Paper configuration, p_state = 0.8, p_drop = 0.1, fixed seeds: full output, last row and chosen rows (one index out of range: a
    NaN row) against the fp64 oracle under the same masks.  B = 5 runs the few-stream latency plan, B = 70 and B = 300 the hybrid
    encoder's live mode (B = 300: windows of the first and of the second round of workgroups, through window_ids)."""
    cfg = synth.PAPER
    m, w = _model(cfg)
    m.set_plan("auto", profile=1)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=1000 + B + T)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    rows_np = np.random.RandomState(B * 41 + T).randint(0, T, size=B)
    rows_np[B // 2] = T + 3                                        # "no value"
    rows = torch.tensor(rows_np, dtype=torch.int32, device="cuda")
    n0 = m.hip_forward_count()
    full = m.forward_live(xi, xs, last_row_only=False, seeds=SEEDS)
    last = m.forward_live(xi, xs, seeds=SEEDS)
    got = m.forward_live(xi, xs, rows=rows, seeds=SEEDS)
    torch.cuda.synchronize()
    assert m.hip_forward_count() == n0 + 3
    st = _stages(m)
    assert ("latency_chain" in st) == (B == 5) and ("fused_encoder" in st) == (B != 5), st
    assert full.shape == (B, T, cfg["size_s"]) and last.shape == got.shape == (B, cfg["size_s"])
    wid = np.arange(B) if B <= 70 else np.array([0, 1, 255, 256, 257, B // 2, B - 1])
    yo = _oracle(cfg, w, x_imu[wid], x_s[wid], SEEDS, P_DROP, P_STATE, window_ids=wid)
    full, last, got = full.cpu().numpy(), last.cpu().numpy(), got.cpu().numpy()
    assert np.isfinite(full).all() and np.isfinite(last).all()
    e_full = float(np.abs(full[wid] - yo).max())
    e_last = float(np.abs(last[wid] - yo[:, -1]).max())
    ok = rows_np[wid] < T
    e_rows = float(np.abs(got[wid][ok] - yo[np.arange(len(wid))[ok], rows_np[wid][ok]]).max())
    print(f"forward_live B={B} T={T}: |hip - oracle_f64| full {e_full:.3e} last {e_last:.3e} rows {e_rows:.3e}")
    assert e_full <= TOL and e_last <= TOL and e_rows <= TOL, (e_full, e_last, e_rows)
    assert np.isnan(got[B // 2]).all() and np.isfinite(np.delete(got, B // 2, axis=0)).all()
    m.check_handoffs()


def test_same_decisions_as_the_training_forward():
    """forward_live against tip_train_forward (the module's .train() call with the stash kept) under the same seeds at B = 256: the
    keep decisions are a function of (seed, site, element index), not of the kernel that draws them."""
    cfg = synth.PAPER
    B, T = 256, 40
    m, _ = _model(cfg)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=2560)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    y_live = m.forward_live(xi, xs, last_row_only=False, seeds=SEEDS)
    # tip_train_forward with an explicit tip_draw_keep_mask mask: the autograd function, stash kept (no lazy few-window path at B = 256)
    m.keep_train_stash = True
    mask = m._hash_keep_mask(xs, SEEDS[1])
    y_tr = tip_amd.simple_transformer_with_state._HipTrainFunction.apply(m, xi, xs, mask, float(np.float32(P_DROP)), SEEDS[0], *m._plist())
    torch.cuda.synchronize()
    e = float((y_live - y_tr.detach()).abs().max())
    print(f"forward_live vs tip_train_forward at B={B}: {e:.3e}")
    assert torch.isfinite(y_live).all() and e < TOL, e
    m.check_handoffs()


@pytest.mark.parametrize("T", [40, 7])
@pytest.mark.parametrize("B", [1, 24, 25])
def test_dropout_entry_point_is_the_live_one_on_the_few_stream_plan(B, T):
    """tip_forward_dropout and tip_forward_live(rows = seeds_dev = NULL) are one body: the same bits on the same handle, seeds and full
    output — in the one-launch form (B = 1, 24) and on the launch chain (B = 25)."""
    cfg = synth.PAPER
    m, _ = _model(cfg)
    m.refresh_packed()
    h = m._ensure_handle()
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=77 + B)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    ws = torch.empty(m.workspace_bytes(B, T), dtype=torch.uint8, device="cuda")
    y_drop, y_live = (torch.full((B, T, cfg["size_s"]), float("nan"), device="cuda") for _ in range(2))
    stream = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / (1.0 - _f32(P_STATE))
    n0 = m.hip_forward_count()
    h.forward_dropout(xi.data_ptr(), xs.data_ptr(), y_drop.data_ptr(), B, T, 0, None, scale, P_STATE, SEEDS[1], P_DROP, SEEDS[0],
                      ws.data_ptr(), ws.numel(), stream)
    h.forward_live(xi.data_ptr(), xs.data_ptr(), y_live.data_ptr(), B, T, None, 0, None, scale, P_STATE, SEEDS[1], P_DROP, SEEDS[0], None,
                   ws.data_ptr(), ws.numel(), stream)
    torch.cuda.synchronize()
    assert m.hip_forward_count() == n0 + 2
    assert torch.isfinite(y_drop).all() and torch.equal(y_drop, y_live)
    m.check_handoffs()


@pytest.mark.parametrize("B", [5, 70])
def test_seeds_through_device_memory(B):
    """seeds_dev == the same values by argument, bit for bit, on both plans; tip_seeds_next leaves the documented successors (computed
    here on the host) and the forward under them equals the by-argument call with those values."""
    cfg = synth.PAPER
    T = 40
    m, _ = _model(cfg)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=77 + B)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    sd = torch.tensor(SEEDS, dtype=torch.int64, device="cuda")
    a = m.forward_live(xi, xs, seeds=SEEDS)
    b = m.forward_live(xi, xs, seeds_dev=sd)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    tlib.seeds_next(sd.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()

    def succ(s):                                   # include/tip_hip.h, tip_seeds_next
        M = (1 << 64) - 1
        z = (s + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    nxt = tuple(succ(s) for s in SEEDS)
    assert tuple(int(v) & ((1 << 64) - 1) for v in sd.cpu().tolist()) == nxt
    c = m.forward_live(xi, xs, seeds_dev=sd)
    d = m.forward_live(xi, xs, seeds=nxt)
    torch.cuda.synchronize()
    assert torch.equal(c, d)
    assert float((c - a).abs().max()) > 1e-3
    m.check_handoffs()


@pytest.mark.parametrize("B", [5, 70])
def test_dropout_is_live(B):
    cfg = synth.PAPER
    m, _ = _model(cfg)
    x_imu, x_s = synth.make_inputs(cfg, B, 40, seed=5)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    a = m.forward_live(xi, xs, seeds=(11, 22))
    b = m.forward_live(xi, xs, seeds=(11, 22))
    c = m.forward_live(xi, xs, seeds=(12, 22))         # encoder dropout only
    d = m.forward_live(xi, xs, seeds=(11, 23))         # keep mask only
    torch.manual_seed(1)
    e = m.forward_live(xi, xs)
    torch.manual_seed(1)
    f = m.forward_live(xi, xs)
    g = m.forward_live(xi, xs)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(e, f)
    for other in (c, d):
        assert float((a - other).abs().max()) > 1e-3
    assert float((f - g).abs().max()) > 1e-3
    # .eval(): the keep mask alone is live, and it is the oracle's function with p_drop = 0
    m.eval()
    h = m.forward_live(xi, xs, seeds=(11, 22))
    torch.cuda.synchronize()
    assert float((a - h).abs().max()) > 1e-3


def test_eval_mode_matches_oracle_with_keep_mask_only():
    cfg = synth.PAPER
    B, T = 70, 40
    m, w = _model(cfg, train=False)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=6)
    y = m.forward_live(torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda(), last_row_only=False, seeds=SEEDS).cpu().numpy()
    wid = np.arange(0, B, 9)
    yo = _oracle(cfg, w, x_imu[wid], x_s[wid], SEEDS, 0.0, P_STATE, window_ids=wid)
    e = float(np.abs(y[wid] - yo).max())
    assert e <= TOL, e


def test_demoted_handle_is_served():
    """A demoted handle (no cooperating kernel: the few-stream plan's recurrence is one) runs the hybrid live mode at any batch."""
    cfg = synth.PAPER
    T = 40
    m, w = _model(cfg)
    m.set_plan("auto", profile=1)
    h = m._ensure_handle()
    h.set_option(tlib.TIP_OPT_DEMOTED, 1)
    try:
        for B in (1, 5, 70):
            x_imu, x_s = synth.make_inputs(cfg, B, T, seed=90 + B)
            y = m.forward_live(torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda(), last_row_only=False, seeds=SEEDS).cpu().numpy()
            wid = np.arange(B) if B <= 5 else np.array([0, 33, 69])
            yo = _oracle(cfg, w, x_imu[wid], x_s[wid], SEEDS, P_DROP, P_STATE, window_ids=wid)
            e = float(np.abs(y[wid] - yo).max())
            print(f"demoted forward_live B={B}: {e:.3e}")
            assert e <= TOL, (B, e)
        assert "latency_chain" not in _stages(m)
    finally:
        h.set_option(tlib.TIP_OPT_DEMOTED, 0)
    m.check_handoffs()


SHAPES = {"72x119": dict(synth.PAPER, size_s=119, with_acc_sum=False), "90x119": dict(synth.PAPER, size_s=119),
          "72x131": dict(synth.PAPER, with_acc_sum=False)}


@pytest.mark.parametrize("tag", list(SHAPES))
@pytest.mark.parametrize("B", [3, 70])
def test_runner_shapes(tag, B):
    """The two-SBP / no-acc-sum runner shapes on both plans."""
    cfg = SHAPES[tag]
    T = 40
    m, w = _model(cfg, seed=0)
    x_imu, x_s = synth.make_inputs(cfg, B, T, seed=300 + B)
    y = m.forward_live(torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda(), last_row_only=False, seeds=SEEDS).cpu().numpy()
    wid = np.arange(B) if B <= 5 else np.array([0, 40, 69])
    yo = _oracle(cfg, w, x_imu[wid], x_s[wid], SEEDS, P_DROP, P_STATE, window_ids=wid)
    e = float(np.abs(y[wid] - yo).max())
    print(f"forward_live {tag} B={B}: {e:.3e}")
    assert y.shape == (B, T, cfg["size_s"]) and np.isfinite(y).all() and e <= TOL, e
    m.check_handoffs()


def test_health_and_refusals():
    cfg = synth.PAPER
    m, _ = _model(cfg)
    x_imu, x_s = synth.make_inputs(cfg, 70, 40, seed=8)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    n0, t0 = m.hip_forward_count(), tlib.spin_timeouts()     # (the counter is per process: other tests inject faults on purpose)
    for k in range(4):
        y = m.forward_live(xi[: (5 if k % 2 else 70)], xs[: (5 if k % 2 else 70)])
        assert m.hip_forward_count() == n0 + k + 1
    torch.cuda.synchronize()
    assert torch.isfinite(y).all() and not y.requires_grad
    m.check_handoffs()
    assert tlib.spin_timeouts() == t0
    with pytest.raises(RuntimeError):
        m.forward_live(xi, xs, seeds=SEEDS, seeds_dev=torch.zeros(2, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError):
        m.forward_live(xi.double(), xs.double())
    m.in_dropout = 0.1
    try:
        with pytest.raises(RuntimeError):
            m.forward_live(xi, xs)
    finally:
        m.in_dropout = 0.0
    # a configuration the hybrid training forward does not serve, beyond the few-stream plan's reach
    tiny = synth.TINY
    mt = make_model(tiny, p_state=0.5)
    load_synth(mt, tiny, 0)
    mt = mt.cuda().train()
    xt_i, xt_s = synth.make_inputs(tiny, 3, 8, seed=1)
    with pytest.raises(tlib.TipStatusError) as ei:
        mt.forward_live(torch.tensor(xt_i).cuda(), torch.tensor(xt_s).cuda())
    assert ei.value.status == tlib.TIP_ERR_UNSUPPORTED_CONFIG


@pytest.mark.parametrize("B", [3, 70])
def test_c_host_live_call_matches_python_host(B):
    """examples/c_host.c `live`: one tip_forward_live call from plain C equals model.forward_live under the same seeds bit for bit."""
    import os
    import shutil
    import subprocess
    import tempfile
    from conftest import ROOT
    from test_c_host_gpu import _weights, _unit, CSRC
    gcc = shutil.which("gcc")
    assert gcc, "the image ships gcc"
    T = 40
    with tempfile.TemporaryDirectory() as td:
        exe, out = os.path.join(td, "c_host"), os.path.join(td, "y.bin")
        cmd = [gcc, "-O2", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
               os.path.join(ROOT, "examples", "c_host.c"), "-o", exe, "-L", CSRC, "-ltip_hip", "-L", "/opt/rocm/lib", "-lamdhip64",
               "-Wl,-rpath," + CSRC, "-Wl,-rpath,/opt/rocm/lib"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run([exe, out, str(B), str(T), "live"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
        yc = np.fromfile(out, dtype=np.float32).reshape(B, 131)
    m = make_model(synth.PAPER, p_state=P_STATE)
    m.load_state_dict(_weights(m))
    m = m.cuda().train()
    m.ENCODER_DROPOUT = P_DROP
    x_imu = _unit(1000, B * T * 90).reshape(B, T, 90)
    x_s = (np.float32(0.5) * _unit(1001, B * T * 131)).reshape(B, T, 131)
    yp = m.forward_live(torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda(), seeds=(1234, 2024)).cpu().numpy()
    assert np.isfinite(yc).all()
    assert np.array_equal(yc, yp), np.abs(yc - yp).max()
