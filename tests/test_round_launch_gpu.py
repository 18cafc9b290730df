"""GPU: one round on the hybrid encoder as ONE launch (csrc/tip_round.hip: forward_round_kernel — the encoder workgroups stay on as
recurrence members and as the output projection) against the three launches it replaces (TIP_OPT_NO_ROUND_LAUNCH = 1).

Both forms run the same statements (the encoder's, the four-row recurrence's and the register-resident projection's bodies are shared,
not copied), so every comparison here is on BITS.  What can go wrong is the hand-off inside the launch: a tile with absent windows
(B = 1, 3, 5), a ragged last tile (B = 31, 33), a second round of 32 workgroup ids (B = 33, 36), windows with and without the 4x4x1 tail
rows (T = 33, 40 / T = 1, 2), a stale L2 line of the previous call read as fresh IH or HALL, a stale flag under a graph replay, and a
member that never arrives."""
import warnings

import numpy as np
import pytest
import torch

from tip_amd import synth
from tip_amd import lib as tlib
from oracle import oracle
from test_host_cpu import make_model, load_synth

pytestmark = pytest.mark.gpu

TOL_TIGHT = 2e-5    # tests/test_hip_parity.py: what the fused plans hold against the fp64 oracle
BATCHES = (1, 3, 4, 5, 31, 32, 33, 36)
_MODELS = {}


def _model(size_s=131):
    """One module per state width for the whole file, pinned to the hybrid encoder."""
    if size_s not in _MODELS:
        cfg = dict(synth.PAPER, size_s=size_s)
        m = make_model(cfg)
        w = load_synth(m, cfg, 0)
        _MODELS[size_s] = (m.cuda().eval(), w, cfg)
    m, w, cfg = _MODELS[size_s]
    m.set_plan("fusedh")
    return m, w, cfg


def _form(m, one_launch):
    m._ensure_handle().set_option(tlib.TIP_OPT_NO_ROUND_LAUNCH, 0 if one_launch else 1)


def _inputs(cfg, B, T, seed):
    # (the generator writes whole 4-column SBP groups: the widths 129 and 130 take the first columns of the 131-wide state)
    x_imu, x_s = synth.make_inputs(dict(cfg, size_s=131), B, T, seed=seed, nan_frac=0.01)
    return torch.tensor(x_imu).cuda(), torch.tensor(np.ascontiguousarray(x_s[:, :, :cfg["size_s"]])).cuda()


def _both(m, xi, xs, last=False):
    """(one launch, three launches) of the same call"""
    out = []
    with torch.no_grad():
        for one_launch in (True, False):
            _form(m, one_launch)
            y = m.forward_last(xi, xs) if last else m(xi, xs)
            out.append(y.cpu().numpy())
    return out


def test_the_schedule_takes_the_form_for_these_shapes_and_a_staged_profile_does_not():
    """What the comparisons below compare: the schedule picks the form for every shape of this file exactly when the option allows it.
    (That the launch then IS the new kernel's shows in the missing-member test: window 8's tile is lost only there.)  A forward
    under the every-stage profile runs the three launches — a stage is a launch — and gives the same bits; under the dominant-stage
    profile the one launch is that stage."""
    m, _, cfg = _model()
    h = m._ensure_handle()
    for one_launch in (True, False):
        _form(m, one_launch)
        assert all(h.round_launch(B, T) == one_launch for B in BATCHES for T in (1, 2, 33, 40))
    xi, xs = _inputs(cfg, 36, 40, 1)
    _form(m, True)
    with torch.no_grad():
        y = m(xi, xs).cpu().numpy()
        m.set_plan("fusedh", profile=1)
        yp = m(xi, xs).cpu().numpy()
        torch.cuda.synchronize()
        assert {"fused_encoder", "rnn_recurrence", "out_linear"} <= {n for n, _, _ in m.profile_read()}
        m.set_plan("fusedh", profile=2)
        yd = m(xi, xs).cpu().numpy()
        torch.cuda.synchronize()
        assert [n for n, _, _ in m.profile_read()] == ["fused_encoder"]
        m.set_plan("fusedh")
    assert np.array_equal(y, yp) and np.array_equal(y, yd)
    m.check_handoffs()


@pytest.mark.parametrize("T", [1, 2, 33, 40])
@pytest.mark.parametrize("size_s", [131, 130, 129])
def test_same_bits_as_three_launches(size_s, T):
    m, _, cfg = _model(size_s)
    for B in BATCHES:
        xi, xs = _inputs(cfg, B, T, 100 * T + B)
        y1, y3 = _both(m, xi, xs)
        assert y1.shape == (B, T, size_s) and np.isfinite(y3).all()
        assert np.array_equal(y1, y3), (size_s, B, T, float(np.abs(y1 - y3).max()))
        if T == 40:
            l1, l3 = _both(m, xi, xs, last=True)
            assert np.array_equal(l1, l3) and np.array_equal(l1.reshape(B, size_s), y1[:, -1]), (size_s, B)
    m.check_handoffs()


def test_paper_model_holds_the_oracle_tolerance():
    m, w, cfg = _model()
    x_imu, x_s = synth.make_inputs(cfg, 36, 40, seed=77)
    _form(m, True)
    with torch.no_grad():
        y = m(torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()).cpu().numpy()
    yo = oracle.forward(cfg, w, x_imu, x_s, dtype=np.float64)
    err = float(np.abs(y - yo).max())
    print(f"one-launch round, B = 36, T = 40: max|hip - oracle_f64| = {err:.3e}")
    assert err < TOL_TIGHT, err
    m.check_handoffs()


def test_no_stale_line_of_the_previous_call_is_read():
    """The same tensors five times, then the windows permuted: IH and HALL of call n sit where call n - 1 left its own, in the L2 of
    whichever XCD read them last.  Every call must be the three launches' result for ITS inputs."""
    m, _, cfg = _model()
    B, T = 36, 40
    xi, xs = _inputs(cfg, B, T, 5)
    perm = torch.tensor(np.random.RandomState(0).permutation(B)).cuda()
    xi_p, xs_p = xi[perm].contiguous(), xs[perm].contiguous()
    with torch.no_grad():
        _form(m, False)
        ref, ref_p = m(xi, xs).cpu().numpy(), m(xi_p, xs_p).cpu().numpy()
        assert not np.array_equal(ref, ref_p)
        _form(m, True)
        for i in range(5):
            assert np.array_equal(m(xi, xs).cpu().numpy(), ref), i
        assert np.array_equal(m(xi_p, xs_p).cpu().numpy(), ref_p)
        assert np.array_equal(m(xi, xs).cpu().numpy(), ref)
        assert np.array_equal(m.forward_last(xi_p, xs_p).cpu().numpy().reshape(B, -1), ref_p[:, -1])
    m.check_handoffs()


def test_graph_replay_gives_the_same_result_every_time():
    """A replay carries the captured launch tag: the window flags of the previous replay must be gone (their owners clear them)."""
    m, _, cfg = _model()
    B, T = 36, 40
    xi, xs = _inputs(cfg, B, T, 6)
    with torch.no_grad():
        _form(m, False)
        ref = m(xi, xs).cpu().numpy()
        _form(m, True)
        m(xi, xs)                                   # warm: attributes, workspace
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            y = m(xi, xs)
        for i in range(3):
            y.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert np.array_equal(y.cpu().numpy(), ref), i
    m.check_handoffs()


@pytest.mark.handoff_fault
def test_a_member_that_never_arrives_poisons_its_rows_and_demotes_the_handle():
    """The existing injection (TIP_OPT_FAULT_INJECT bit 1: member 1 of cluster 0 exits at entry; as a workgroup of this launch it is
    workgroup 8, so window 8 is never encoded either).  The call returns; the rows of tile 0 (its cluster) and of tile 2 (its
    window's) are NaN, never finite-but-wrong; the next call reports the loss and the handle goes on without hand-offs."""
    cfg = synth.PAPER
    m = make_model(cfg)
    load_synth(m, cfg, 0)
    m = m.cuda().eval()
    m.set_plan("fusedh")
    h = m._ensure_handle()
    B, T = 36, 40
    xi, xs = _inputs(cfg, B, T, 9)
    with torch.no_grad():
        m.set_plan("fusedh", rnn_cluster=1)
        ref_safe = m(xi, xs).cpu().numpy()
        m.set_plan("fusedh")
        _form(m, True)
        ref = m(xi, xs).cpu().numpy()
        assert np.abs(ref - ref_safe).max() < 5e-6
        h.set_option(tlib.TIP_OPT_FAULT_INJECT, 2)
        y_bad = m(xi, xs).cpu().numpy()
        torch.cuda.synchronize()
        assert np.isnan(y_bad[0:4]).all() and np.isnan(y_bad[8:12]).all()
        ok = np.ones(B, bool)
        ok[0:4] = ok[8:12] = False
        assert np.array_equal(y_bad[ok], ref[ok])
        assert not m.is_demoted()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            y1 = m(xi, xs)                          # entry check trips -> demote -> this call runs
            torch.cuda.synchronize()
        assert any("lost an inter-workgroup hand-off" in str(r.message) for r in rec)
        assert m.is_demoted() and m.demotions == 1 and not h.round_launch(B, T)
        assert np.array_equal(y1.cpu().numpy(), ref_safe)
        assert np.array_equal(m(xi, xs).cpu().numpy(), ref_safe)      # the fault is still injected: nothing cooperating runs
        m.check_handoffs()
        h.set_option(tlib.TIP_OPT_FAULT_INJECT, 0)
        m.undemote()
        assert np.array_equal(m(xi, xs).cpu().numpy(), ref)
        m.check_handoffs()
