"""GPU: the streaming engines with live_dropout=True — the model as the reference deploys it (past_state_dropout = 0.8, .train()) behind
StreamingEngine and StaggeredStreamingEngine: graph mode against launch mode bit for bit, frames against the fp64 oracle under the
engine's device seeds, pools under an attach / detach schedule, .eval() with the keep mask alone live."""
import warnings

import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from tip_amd import lib as tlib
from tip_amd.streaming import StreamingEngine, StaggeredStreamingEngine
from test_host_cpu import make_model, load_synth
from test_live_forward_gpu import _oracle, TOL, P_STATE, P_DROP

pytestmark = pytest.mark.gpu


def _model(train=True, p_state=P_STATE):
    cfg = synth.PAPER
    m = make_model(cfg, p_state=p_state)
    w = load_synth(m, cfg, 0)
    m = m.cuda()
    m = m.train() if train else m.eval()
    m.ENCODER_DROPOUT = P_DROP
    return m, w


def _raw_frames(B, F, seed=3):
    """The raw-IMU generator of tests/test_streaming_gpu.py (test_graph_mode_equals_launch_by_launch)."""
    from scipy.spatial.transform import Rotation
    rng = np.random.RandomState(seed)
    raw = np.zeros((F, B, 72), dtype=np.float32)
    for f in range(F):
        raw[f, :, :54] = Rotation.random(B * 6, random_state=100 + f).as_matrix().reshape(B, 54)
        raw[f, :, 54:] = rng.randn(B, 18)
    return raw, rng.randn(B, 114).astype(np.float32) * 0.2


def _run_lockstep(m, raw, s_init, use_graph, manual_seed):
    torch.manual_seed(manual_seed)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*train\\(\\) mode.*")   # live_dropout=True: no ".train() mode" warning
        eng = StreamingEngine(m, s_init, use_graph=use_graph, live_dropout=True)
    outs = []
    for f in range(raw.shape[0]):
        o = eng.step(raw[f])
        outs.append(None if o is None else {k: o[k].clone() for k in ("s_rest", "c_t", "y_last")})
    torch.cuda.synchronize()
    return eng, outs


@pytest.mark.parametrize("n", [3, 300])
def test_graph_mode_equals_launch_mode_with_a_train_model(n):
    """StreamingEngine(model.train(), live_dropout=True), past_state_dropout = 0.8: 60 frames; use_graph=False and use_graph=True under
    the same torch.manual_seed give bit-identical s_rest, c_t, y_last on every frame (the last 16 are replays); another seed differs."""
    m, _ = _model()
    raw, s_init = _raw_frames(n, 60)
    n0, t0 = m.hip_forward_count(), tlib.spin_timeouts()     # (the counter is per process: other tests inject faults on purpose)
    ea, a = _run_lockstep(m, raw, s_init, False, 7)
    assert m.hip_forward_count() == n0 + 55
    eb, b = _run_lockstep(m, raw, s_init, True, 7)
    assert eb._graph is not None and eb.captures == 1
    _, c = _run_lockstep(m, raw, s_init, False, 8)
    differs = False
    for f in range(60):
        assert (a[f] is None) == (b[f] is None) == (f < 5)
        if a[f] is None:
            continue
        for k in ("s_rest", "c_t", "y_last"):
            assert torch.equal(a[f][k], b[f][k]), (f, k)
            assert torch.isfinite(a[f][k]).all(), (f, k)
        differs |= float((a[f]["y_last"] - c[f]["y_last"]).abs().max()) > 1e-3
    assert differs
    assert torch.equal(ea.seeds, eb.seeds)
    m.check_handoffs()
    assert tlib.spin_timeouts() == t0


@pytest.mark.parametrize("use_graph", [False, True], ids=["launch", "graph"])
def test_frames_against_the_oracle(use_graph):
    """Three frames after the window is full: the seeds read before the frame, advanced on the host by the tip_seeds_next rule, and the
    windows the frame ran on give y_last through the fp64 oracle."""
    m, w = _model()
    n = 3
    raw, s_init = _raw_frames(n, 60, seed=5)
    torch.manual_seed(11)
    eng = StreamingEngine(m, s_init, use_graph=use_graph, live_dropout=True)
    checked = 0
    for f in range(60):
        before = [int(v) & tlib._M64 for v in eng.seeds.cpu().tolist()]
        out = eng.step(raw[f])
        if f not in (45, 52, 59):
            continue
        torch.cuda.synchronize()
        assert out["T"] == 40
        seeds = tuple(tlib.seed_successor(s) for s in before)
        assert [int(v) & tlib._M64 for v in eng.seeds.cpu().tolist()] == list(seeds)
        yo = _oracle(synth.PAPER, w, eng.x_imu.cpu().numpy(), eng.x_s.cpu().numpy(), seeds, P_DROP, P_STATE)[:, -1]
        e = float(np.abs(out["y_last"].cpu().numpy() - yo).max())
        print(f"live frame {f} (graph={use_graph}): |y_last - oracle_f64| = {e:.3e}")
        assert e <= TOL, (f, e)
        checked += 1
    assert checked == 3
    m.check_handoffs()


def _schedule(n, F, seed):
    """The random attach / detach schedule of tests/test_staggered_streams_gpu.py (test_graph_mode_equals_launch_by_launch)."""
    rng = np.random.RandomState(seed)
    ev = []
    for f in range(F):
        det = [int(i) for i in range(n) if rng.rand() < 0.03]
        att = [int(i) for i in range(n) if rng.rand() < 0.03 and i not in det]
        ev.append((det, att))
    return ev


def _run_pool(m, raw, s_init, ev, compact, use_graph, manual_seed=21):
    torch.manual_seed(manual_seed)
    eng = StaggeredStreamingEngine(m, s_init, use_graph=use_graph, compact=compact, live_dropout=True)
    outs = []
    for f in range(raw.shape[0]):
        det, att = ev[f]
        eng.detach(det)
        eng.attach(att, s_init[att])
        o = eng.step(raw[f])
        outs.append({k: o[k].clone() for k in ("s_rest", "c_t", "y_last", "T", "valid")})
    torch.cuda.synchronize()
    return eng, outs


@pytest.mark.parametrize("compact", [False, True], ids=["plain", "compact"])
@pytest.mark.parametrize("n", [3, 40])
def test_pools_accept_a_train_model_and_graph_equals_launch(n, compact):
    m, _ = _model()
    s0 = np.zeros((n, 114), dtype=np.float32)
    with pytest.raises(RuntimeError):
        StaggeredStreamingEngine(m, s0, compact=compact)                     # without the keyword: still refused
    with pytest.raises(RuntimeError):
        StaggeredStreamingEngine(m, s0, compact=compact, live_dropout=True, reuse=True)
    F = 70
    raw, s_init = _raw_frames(n, F, seed=30 + n)
    ev = _schedule(n, F, n)
    ea, a = _run_pool(m, raw, s_init, ev, compact, False)
    eb, b = _run_pool(m, raw, s_init, ev, compact, True)
    assert eb.captures >= 1
    seen_valid = seen_invalid = False
    for f in range(F):
        v = a[f]["valid"]
        for k in ("s_rest", "c_t", "y_last", "T", "valid"):
            assert torch.equal(a[f][k].nan_to_num(7.0), b[f][k].nan_to_num(7.0)), (f, k)
        # rows of slots that are not valid: NaN in y_last, unchanged in s_rest / c_t
        assert torch.isfinite(a[f]["y_last"][v]).all() and torch.isnan(a[f]["y_last"][~v]).all()
        assert torch.isfinite(a[f]["s_rest"]).all()
        if f:
            for k in ("s_rest", "c_t"):
                assert torch.equal(a[f][k][~v], a[f - 1][k][~v]), (f, k)
        seen_valid |= bool(v.any())
        seen_invalid |= bool((~v).any())
    assert seen_valid and seen_invalid
    assert torch.equal(ea.seeds, eb.seeds)
    _, c = _run_pool(m, raw, s_init, ev, compact, False, manual_seed=22)
    assert float((a[-1]["y_last"].nan_to_num(0.0) - c[-1]["y_last"].nan_to_num(0.0)).abs().max()) > 1e-3
    m.check_handoffs()


def test_eval_model_keep_mask_is_live_without_torch_rand(monkeypatch):
    """.eval() with past_state_dropout = 0.8 and live_dropout=True: identical input windows give different outputs from frame to frame
    (the mask is drawn in the kernel, fresh per frame), and torch.rand_like is never called during step()."""
    m, w = _model(train=False)
    n = 2
    raw, s_init = _raw_frames(n, 50, seed=9)
    eng = StreamingEngine(m, s_init, live_dropout=True)
    for f in range(46):
        eng.step(raw[f])
    calls = []
    real = torch.rand_like
    monkeypatch.setattr(torch, "rand_like", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    # the same windows twice: forward_live under the engine's seeds, advanced in between as a frame does
    xi, xs = eng.x_imu.clone(), eng.x_s.clone()
    st = torch.cuda.current_stream().cuda_stream
    ys = []
    for _ in range(2):
        tlib.seeds_next(eng.seeds.data_ptr(), st)
        ys.append(m.forward_live(xi, xs, seeds_dev=eng.seeds).clone())
    out = eng.step(raw[46])
    torch.cuda.synchronize()
    assert not calls
    assert float((ys[0] - ys[1]).abs().max()) > 1e-3
    assert torch.isfinite(out["y_last"]).all()
    # and the frame is the oracle's under the keep mask alone (p_drop = 0 in .eval())
    before = [int(v) & tlib._M64 for v in eng.seeds.cpu().tolist()]
    out = eng.step(raw[47])
    torch.cuda.synchronize()
    seeds = tuple(tlib.seed_successor(s) for s in before)
    yo = _oracle(synth.PAPER, w, eng.x_imu.cpu().numpy(), eng.x_s.cpu().numpy(), seeds, 0.0, P_STATE)[:, -1]
    e = float(np.abs(out["y_last"].cpu().numpy() - yo).max())
    assert e <= TOL, e
    m.check_handoffs()


def test_lockstep_refusals_and_defaults():
    m, _ = _model()
    s0 = np.zeros((2, 114), dtype=np.float32)
    with pytest.raises(RuntimeError):
        StreamingEngine(m, s0, live_dropout=True, reuse=True)
    eng = StreamingEngine(m, s0, live_dropout=True, reuse="auto")
    assert eng.reuse is False and eng.seeds.dtype == torch.int64 and tuple(eng.seeds.shape) == (2,)
    with pytest.warns(UserWarning, match="train"):                           # the default is unchanged: the warning stays
        eng = StreamingEngine(m, s0)
    assert eng.seeds is None and eng.live_dropout is False
