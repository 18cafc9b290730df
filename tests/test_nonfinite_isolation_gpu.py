"""GPU: a non-finite window never reaches another window's output (the contract and its harness:
tests/test_nonfinite_oracle.py).  One stream's broken sensor puts a NaN or +-Inf into a batch that also carries healthy streams; the
reference (simple_transformer_with_state.py:60-102) keeps windows independent, so every other window's output is unchanged bit for bit,
the poisoned window is NaN from the poisoned row on, and nothing is ever finite-and-different.

Who shares what with a poisoned window b, per plan (#CUs = multi_processor_count, never a literal):
  latency     every window is a role of ONE launch (B <= 64): all windows share the launch's hand-off words and L2 staging.
  fused1s2/4  one window on 2 / 4 workgroups; neighbours b-1, b+1 sit beside it in the exchange buffer `xchg` and on the same XCD.
  fused,      grid = min(B, #CUs) persistent workgroups, window b then b + #CUs on workgroup b % #CUs: with B = #CUs + 44, windows
  fusedh      0 .. 43 are followed by #CUs .. #CUs + 43 on the same LDS planes (pad rows 40-47, or 33-47 at T = 33).
  fused2      workgroup g carries the window PAIR (2g, 2g + 1), then pair g + #CUs: b and b ^ 1 share an 80(96)-row plane; with
              B = 2 #CUs + 3 pair 1 = (2, 3) is followed on workgroup 1 by pair #CUs + 1 = (2 #CUs + 2,) — the odd last window.
  general     GEMM row tiles run over the flattened [B*T] rows (T = 39, 129: every tile border falls inside a window), the recurrence
              carries 4 (auto) or 16 (rnn_cluster 1..16) windows per tile: b shares its tile with b ^ 1, b ^ 2, ...
  auto        B = #CUs + 1: one whole round + one window on the few-stream plan; #CUs + 44: whole round + 44 windows on the
              window-split encoder, ONE recurrence and projection for both parts (shared tail).
"""
import warnings

import numpy as np
import pytest
import torch

from tip_amd import synth
from tip_amd import lib as tlib
from oracle import oracle
from test_host_cpu import make_model, load_synth
from test_nonfinite_oracle import Poison, poisoned, check_outputs, NAN, INF

pytestmark = pytest.mark.gpu
CFG = synth.PAPER
TOL_TIGHT = 2e-5      # tests/test_hip_parity.py: fp32 MFMA against the fp64 oracle on these inputs

ROT, ACC, ACCSUM = 5, 54 + 6, 72 + 8         # x_imu: 54 rotation | 18 acceleration | 18 acc-sum columns
SPOTS = [("x_imu", c, v) for c in (ROT, ACC, ACCSUM) for v in (NAN, INF, -INF)] + \
        [("x_s", c, v) for c in (7, 109) for v in (INF, -INF)]      # a NaN in x_s is scrubbed (:65); 109: a root-velocity column (:75)


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _rows_of(T):
    return sorted({r for r in (0, 15, 16, 31, 32, T - 1) if r < T})


def _model(seed=0, **kw):
    m = make_model(CFG, **kw)
    w = load_synth(m, CFG, seed)
    return m.cuda().eval(), w


class _Runner:
    """The three output forms of one handle on one (B, T): full, last row, chosen rows."""

    def __init__(self, m, T, fwd=None):
        self.m, self.T = m, T
        self.fwd = fwd

    def __call__(self, x_imu, x_s, form="full", rows=None):
        m = self.m
        xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
        n0 = m.hip_forward_count()
        with torch.no_grad():
            if self.fwd is not None:
                y = self.fwd(xi, xs, form, rows)
            elif form == "full":
                y = m(xi, xs)
            elif form == "last":
                y = m.forward_last(xi, xs)
            else:
                y = m.forward_rows(xi, xs, torch.tensor(rows, dtype=torch.int32).cuda())
        torch.cuda.synchronize()
        assert m.hip_forward_count() > n0, "the HIP path did not run"
        return y.cpu().numpy()


def _healthy(m, t0):
    """Item 4: no hand-off gave up, nothing is flagged, the handle was not demoted."""
    assert tlib.spin_timeouts() == t0, "a hand-off wait gave up on a data NaN"
    m.check_handoffs()
    assert not m.is_demoted() and m.demotions == 0 and m.flow_demotions == 0


def _rows_around(B, T, p):
    """One row per window, on both sides of r in the poisoned windows and spread over [0, T) elsewhere."""
    rows = (np.arange(B) * 7 + 3) % T
    for k, b in enumerate(p.windows):
        rows[b] = (max(p.row - 1, 0), p.row, min(p.row + 1, T - 1), T - 1)[k % 4] if len(p.windows) > 1 else max(p.row - 1, 0)
    return rows.astype(np.int32)


def _first_nan_row(r, item3):
    """Where a poisoned window turns NaN.  "block": the fp32 attention multiplies the masked
    probabilities of r's 16-key block (exact 0) with V in an MFMA, 0 x NaN = NaN: rows 16 * (r // 16) .. r - 1 go too.  "causal": r."""
    return {"block": 16 * (r // 16), "causal": r}[item3]


def _sweep(run, m, x_imu, x_s, specs, tag, w=None, forms=("full", "last", "rows"), item3="block"):
    """Items 1-5 for every poison of `specs` on one handle and batch; item3: the plan's documented answer to item 3."""
    B, T = x_imu.shape[:2]
    ncu = _ncu()
    t0 = tlib.spin_timeouts()
    clean = {"full": run(x_imu, x_s), "last": run(x_imu, x_s, "last")}
    assert np.array_equal(clean["last"], clean["full"][:, -1])
    if w is not None:
        # Where the older tests hold this plan to the oracle, so do the windows here: all of them up to 40, beyond that the first,
        # middle and last, every window that is poisoned in some case and the one that follows it on the same workgroup (the other
        # windows are held to the clean call bit for bit below; the fp64 oracle costs ~10 ms per window on the host)
        named = {b for p in specs for b in p.windows}
        sel = np.arange(B) if B <= 40 else np.unique([b for b in {0, B // 2, B - 1} | named | {b + ncu for b in named} if b < B])
        yo = oracle.forward(CFG, w, x_imu[sel], x_s[sel], dtype=np.float64)
        assert np.abs(clean["full"][sel] - yo).max() < TOL_TIGHT
    every_form = len(specs) <= 24           # (the 78 row x spot pairs of the small batches: last-row and chosen-row forms on every third)
    for k, p in enumerate(specs):
        xi, xs = poisoned(x_imu, x_s, p)
        for form in (forms if every_form or k % 3 == 0 else ("full",)):
            if form == "full":
                y = run(xi, xs)
                check_outputs(y, clean["full"], p, tag=(tag, form))
                for b in p.windows:
                    first = int(np.isnan(y[b]).all(axis=1).argmax())
                    assert first == _first_nan_row(p.row, item3), (tag, p, b, "first all-NaN row", first, "documented:", item3)
            elif form == "last":
                check_outputs(run(xi, xs, "last"), clean["last"], p, rows=T - 1, tag=(tag, form))
            else:
                for shift in (0, 1):            # the poisoned windows' chosen rows: r - 1, then r (and r + 1 .. with several windows)
                    rows = _rows_around(B, T, p)
                    for b in p.windows:
                        rows[b] = min(rows[b] + shift, T - 1)
                    y_clean_rows = clean["full"][np.arange(B), rows]
                    check_outputs(run(xi, xs, "rows", rows), y_clean_rows, p, rows=rows, tag=(tag, form, shift))
        _healthy(m, t0)
    # item 5: the clean call again, on the same handle and workspace
    assert np.array_equal(run(x_imu, x_s), clean["full"]), (tag, "the clean call after the poisoned ones differs from the first")
    assert np.array_equal(run(x_imu, x_s, "last"), clean["last"]), (tag, "last row, afterwards")
    _healthy(m, t0)


def _specs(T, windows_list, full_cross):
    """full_cross (few windows: cheap): every row with every spot, the window sets walked along.  Otherwise EVERY window set at EVERY
    row — spec k takes row k % R of set (k // R) % W — with the 13 spots walked along (13 is coprime to R = 6 and the list has at
    least 13 entries: every spot is used, no row or window set is tied to a spot's parity)."""
    rows = _rows_of(T)
    out = []
    if full_cross:
        for i, r in enumerate(rows):
            for j, (t, c, v) in enumerate(SPOTS):
                out.append(Poison(t, tuple(windows_list[(i + j) % len(windows_list)]), r, c, v))
    else:
        R, W = len(rows), len(windows_list)
        for k in range(max(len(SPOTS), R * W)):
            t, c, v = SPOTS[k % len(SPOTS)]
            out.append(Poison(t, tuple(windows_list[(k // R) % W]), rows[k % R], c, v))
    return out


def _plan_batches(plan, ncu):
    """(B, T, windows_list) per plan: the table of the issue.  windows_list: the sets P to walk through."""
    if plan == "latency":
        return [(1, 40, [(0,)]), (5, 40, [(1,), (4,), (0, 3)]), (5, 33, [(2,), (4,), (1, 2)]), (32, 40, [(9,), (31,), (0, 8, 16)]),
                (32, 33, [(17,), (31,)])]
    if plan == "fused1s2":
        # window b on workgroups 2b, 2b + 1: its exchange slots lie between those of b - 1 and b + 1
        return [(40, 40, [(7,), (39,), (0, 20)]), (min(100, ncu // 2), 40, [(50,), (min(100, ncu // 2) - 1,)])]
    if plan == "fused1s4":
        nb = min(100, 64, ncu // 4)              # four workgroups per window fit up to min(64, #CUs / 4) windows
        return [(min(40, nb), 40, [(7,), (min(40, nb) - 1,), (0, 20)]), (nb, 40, [(nb // 2,), (nb - 1,)])]
    if plan in ("fused", "fusedh"):
        # B = #CUs + 44: workgroup 3 runs window 3, then window #CUs + 3 (3 + #CUs < B) on the same LDS planes; workgroup 43 runs
        # window 43, then the last window #CUs + 43
        B = ncu + 44
        big = [(3,), (B - 1,), (43,), (3, ncu + 2, B - 1)]
        return [(5, 40, [(1,), (4,), (0, 3)]), (5, 33, [(2,), (4,)]), (B, 40, big), (B, 33, big)]
    if plan == "fused2":
        # B = 2 #CUs + 3: #CUs + 2 pairs, the last one odd.  Pair 1 = windows (2, 3) on workgroup 1, which then runs pair #CUs + 1 =
        # the last window 2 #CUs + 2 alone; window 2's pair partner is 3.  B = 5: pairs (0,1) (2,3) (4,)
        B = 2 * ncu + 3
        return [(5, 40, [(2,), (3,), (4,), (0, 4)]), (B, 40, [(2,), (3,), (B - 1,), (0, 1, 2 * ncu)])]
    if plan == "general":
        # T = 39 / 129: no GEMM row tile (16 .. 128 rows of the flattened batch) starts on a window border; windows 0-3 share a
        # four-window recurrence tile, 0-15 a sixteen-window one
        return [(17, 39, [(1,), (16,), (2, 15)]), (2, 129, [(0,), (1,)])]
    if plan == "auto":
        # #CUs + 1: windows 0 .. #CUs - 1 a whole round, the last on the few-stream plan; #CUs + 44: remainder on the window-split
        # encoder, one recurrence tile sequence for both parts (tile of windows #CUs - 4 .. #CUs + 3 spans the parts' border)
        return [(ncu + 1, 40, [(3,), (ncu,), (ncu - 1,)]), (ncu + 44, 40, [(3,), (ncu + 43,), (ncu - 1, ncu), (ncu + 1,)])]
    raise KeyError(plan)


@pytest.mark.parametrize("plan", ["latency", "fused1s2", "fused1s4", "fusedh", "fused", "fused2", "general", "auto"])
def test_inference_plans_isolate_a_nonfinite_window(plan):
    ncu = _ncu()
    m, w = _model(0)
    m.set_plan(plan)
    for B, T, windows_list in _plan_batches(plan, ncu):
        x_imu, x_s = synth.make_inputs(CFG, B, T, seed=9000 + B + T)
        run = _Runner(m, T)
        specs = _specs(T, windows_list, full_cross=B <= 8)
        if T > 40:                               # rows past 40 too: the last row of a long window
            specs += [Poison("x_imu", (1,), 100, ROT, NAN), Poison("x_s", (0,), 128, 7, INF)]
        # (the general plan's attention for windows beyond 40 rows masks per key, not per 16-key MFMA block)
        _sweep(run, m, x_imu, x_s, specs, (plan, B, T), w=w, item3="causal" if T > 40 else "block")


@pytest.mark.parametrize("cluster", [1, 2, 4, 8, 16])
def test_recurrence_clusters_isolate_a_nonfinite_window(cluster):
    """B = 37 = two full 16-window tiles + 5: window 5 shares its tile with 0-15, window 36 closes the ragged tile; the tile's
    workgroups pass h between them through HALL words they poll for a sentinel — a data NaN must not read as one."""
    m, w = _model(0)
    m.set_plan("general", rnn_cluster=cluster)
    B, T = 37, 40
    x_imu, x_s = synth.make_inputs(CFG, B, T, seed=9037)
    _sweep(_Runner(m, T), m, x_imu, x_s, _specs(T, [(5,), (36,), (15, 16)], full_cross=False), ("general", cluster, B), w=w)


# ----------------------------------------------------------------------------------------------------------------------
# the deployed and the training forwards
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Bk", ["5", "70", "cus+44"])
def test_forward_live_isolates_a_nonfinite_window(Bk):
    """tip_forward_live: keep mask drawn in the first kernel (p_state = 0.8), encoder dropout live (.train(): p_drop = 0.1), fixed
    seeds — B = 5 the few-stream plan, 70 the window-split encoder, #CUs + 44 the hybrid encoder's live mode over two rounds
    (window 3, then #CUs + 3 on workgroup 3)."""
    ncu = _ncu()
    B = {"5": 5, "70": 70, "cus+44": ncu + 44}[Bk]
    T = 40
    m, _ = _model(0, p_state=0.8)
    m.train()
    seeds = (1234567, 7654321)

    def fwd(xi, xs, form, rows):
        if form == "rows":
            return m.forward_live(xi, xs, rows=torch.tensor(rows, dtype=torch.int32).cuda(), seeds=seeds)
        return m.forward_live(xi, xs, last_row_only=form == "last", seeds=seeds)

    x_imu, x_s = synth.make_inputs(CFG, B, T, seed=9100 + B)
    windows_list = [(1,), (B - 1,), (0, 3)] if B <= 70 else [(3,), (B - 1,), (3, ncu + 2)]
    _sweep(_Runner(m, T, fwd), m, x_imu, x_s, _specs(T, windows_list, full_cross=False), ("live", B))


def test_fp64_forward_isolates_a_nonfinite_window():
    B, T = 5, 40
    m, w = _model(0)
    m = m.double()
    x_imu, x_s = synth.make_inputs(CFG, B, T, seed=9205)

    def run(xi, xs, form="full", rows=None):
        with torch.no_grad():
            xi, xs = torch.tensor(xi, dtype=torch.float64).cuda(), torch.tensor(xs, dtype=torch.float64).cuda()
            y = m(xi, xs) if form == "full" else m.forward_last(xi, xs)
        torch.cuda.synchronize()
        return y.cpu().numpy()

    # (forward_rows computes in fp32 only and raises for an fp64 module: two output forms here.  The fp64 attention masks per key.)
    _sweep(run, m, x_imu, x_s, _specs(T, [(1,), (4,), (0, 3)], full_cross=False), ("f64", B), w=w, forms=("full", "last"), item3="causal")


@pytest.mark.parametrize("Bk", ["40", "cus+44"])
def test_training_step_isolates_a_nonfinite_window(Bk):
    """The .train() call (_HipTrainFunction: tip_train_forward / tip_train_backward / tip_train_input_grads) on the padded training
    forward.  y as everywhere; after backward the input gradients of every clean window equal the clean run's bit for bit and those
    of the poisoned window are never finite-and-different.  (Weight gradients sum over windows: NaN in the reference as well.)"""
    ncu = _ncu()
    B = {"40": 40, "cus+44": ncu + 44}[Bk]
    T = 40
    m, _ = _model(0)
    m.train()
    x_imu, x_s = synth.make_inputs(CFG, B, T, seed=9300 + B)
    gy = torch.tensor(synth.normal(5, "gy", B * T * CFG["size_s"]).reshape(B, T, -1).astype(np.float32)).cuda()

    def step(xi_np, xs_np):
        xi = torch.tensor(xi_np).cuda().requires_grad_(True)
        xs = torch.tensor(xs_np).cuda().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(77)                    # the same dropout decisions in every call
        n0 = m.hip_forward_count()
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message="tip_amd")   # the torch-op composite announces itself: it must not serve this
            y = m(xi, xs)
            y.backward(gy)
        torch.cuda.synchronize()
        assert m.hip_forward_count() > n0
        return y.detach().cpu().numpy(), xi.grad.cpu().numpy(), xs.grad.cpu().numpy()

    t0 = tlib.spin_timeouts()
    clean = step(x_imu, x_s)
    assert all(np.isfinite(a).all() for a in clean)
    windows_list = [(7,), (B - 1,), (0, 20)] if B == 40 else [(3,), (B - 1,), (3, ncu + 2)]
    for p in _specs(T, windows_list, full_cross=False):      # every window set at every row of the list, forward and backward
        y, gi, gs = step(*poisoned(x_imu, x_s, p))
        check_outputs(y, clean[0], p, tag=("train", B))
        others = np.setdiff1d(np.arange(B), np.array(p.windows))
        for name, g, gc in (("d x_imu", gi, clean[1]), ("d x_s", gs, clean[2])):
            assert np.array_equal(g[others].view(np.uint32), gc[others].view(np.uint32)), (p, name, "a clean window's input gradient changed")
            for b in p.windows:
                same = g[b].view(np.uint32) == gc[b].view(np.uint32)
                assert (same | ~np.isfinite(g[b])).all(), (p, name, "finite and different in the poisoned window")
        _healthy(m, t0)
    again = step(x_imu, x_s)
    assert all(np.array_equal(a, b) for a, b in zip(again, clean))


# ----------------------------------------------------------------------------------------------------------------------
# buffers outlive a call
# ----------------------------------------------------------------------------------------------------------------------
FLOW_STAGE_BYTES, FLOW_WINDOW_BYTES = 64 * 8, 34 * 64 * 8      # csrc/tip_latency.hip: a window's flags are [34 stages][64] u64 at the workspace's front


@pytest.mark.parametrize("shift", [(4, 5), (8, 5), (8, 0), (1, 0)])
def test_workspace_moved_over_its_own_stale_flags(shift):
    """A workspace that moves through memory which held the same handle's workspace before, at a shifted address — the module's own
    per-stream buffer does while a stream warms up (it grows with T; the engines' frame 21 of 5 streams was NaN that way).  The
    one-launch few-stream form keeps completion flags and launch counters at the workspace's front; a fresh area counts from 0 like
    the old one did.  shift = (windows, stages): the new area starts that far into the old one, so window w meets window w + 4's
    stamps of the same epoch (another XCD: it gave up at once), window w + 8's (its own XCD: "done" before the producers ran), or
    the old area whole.  Clean data throughout: the result must be the first call's, bit for bit."""
    B, T = 9, 17
    m, w = _model(0)
    m.set_plan("latency")
    x_imu, x_s = synth.make_inputs(CFG, B, T, seed=9400)
    xi, xs = torch.tensor(x_imu).cuda(), torch.tensor(x_s).cuda()
    need = m.workspace_bytes(B, T)
    off = shift[0] * FLOW_WINDOW_BYTES + shift[1] * FLOW_STAGE_BYTES
    assert off % 256 == 0
    pool = torch.zeros(need + off, dtype=torch.uint8, device="cuda")
    t0 = tlib.spin_timeouts()
    with torch.no_grad():
        y0 = m.forward_last(xi, xs, workspace=pool[:need]).cpu().numpy()
        y1 = m.forward_last(xi, xs, workspace=pool[off:off + need]).cpu().numpy()
        y2 = m.forward_last(xi, xs, workspace=pool[:need]).cpu().numpy()
    yo = oracle.forward(CFG, w, x_imu, x_s, dtype=np.float64)[:, -1]
    assert np.abs(y0 - yo).max() < TOL_TIGHT
    assert np.array_equal(y1, y0) and np.array_equal(y2, y0)
    _healthy(m, t0)
