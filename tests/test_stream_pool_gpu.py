"""GPU tests of compact staggered pools: the position-mapped streaming entry points (tip_stream_ingest_mapped /
tip_stream_consume_mapped, csrc/tip_stream.hip) against the staggered ones, and StaggeredStreamingEngine(compact=True) against
compact=False, the fp64 oracle and the trace of the real reference runner (tests/golden/tip_runner_golden.npz)."""
import ctypes

import numpy as np
import pytest
import torch

import tip_amd
from tip_amd import synth
from tip_amd import lib as tlib
from oracle import oracle
from test_staggered_streams_gpu import paper, trace, _raw_frames, _schedule, _cbuf, TOL_LOOP, TOL_PARITY  # noqa: F401

pytestmark = pytest.mark.gpu
KEYS = ("s_rest", "c_t", "y_last", "T", "valid")
Engine = tip_amd.streaming.StaggeredStreamingEngine


def _state_rows(state, n):
    nb = ctypes.c_size_t()
    assert tlib.load().tip_stream_state_bytes(1, ctypes.byref(nb)) == 0
    return state.view(torch.uint8)[: n * nb.value].view(n, nb.value).cpu()


def test_mapped_entry_points_match_staggered():
    """A random map per frame (a permutation of the listed slots with empty positions between them): every window, rows[p],
    y_slot / rows_slot and the post-consume state of every slot are the staggered calls' bits; empty positions give zero windows and
    -1; a slot attached in the mapped buffer but never listed is not touched."""
    n, B, F = 37, 36, 60
    lib = tlib.load()
    st = torch.cuda.current_stream().cuda_stream
    raw = torch.tensor(_raw_frames(F, n, 21)).cuda()
    s_init = torch.tensor(np.random.RandomState(22).randn(n, 114).astype(np.float32) * 0.2).cuda()
    bufs = []
    for _ in range(2):
        _, state = _cbuf(n)
        assert lib.tip_stream_reset(state.data_ptr(), s_init.data_ptr(), n, st) == 0
        bufs.append(dict(state=state, x_imu=torch.full((n, 40, 90), float("nan"), device="cuda"),
                         x_s=torch.full((n, 40, 131), float("nan"), device="cuda"), rows=torch.empty(n, dtype=torch.int32, device="cuda"),
                         s_rest=torch.zeros(n, 111, device="cuda"), c_t=torch.zeros(n, 20, device="cuda")))
    A, M = bufs
    detached = {3, 11}                  # never attached: listed at some positions (zero window, -1), state untouched
    hidden = 36                         # attached in M but never listed
    start = {s: (s * 7) % 50 for s in range(n) if s not in detached and s != hidden}
    listed_slots = sorted(set(range(n)) - {hidden})
    y_slot = torch.full((n, 131), 7.0, device="cuda")
    rows_slot = torch.full((n,), 99, dtype=torch.int32, device="cuda")
    sl = torch.tensor([hidden], dtype=torch.int32, device="cuda")
    assert lib.tip_stream_attach(M["state"].data_ptr(), n, sl.data_ptr(), s_init[hidden:].data_ptr(), 1, st) == 0
    torch.cuda.synchronize()
    hidden_bytes = _state_rows(M["state"], n)[hidden].clone()
    rng = np.random.RandomState(23)
    for f in range(F):
        for s, f0 in start.items():
            if f == f0:
                sl = torch.tensor([s], dtype=torch.int32, device="cuda")
                for buf in (A, M):
                    assert lib.tip_stream_attach(buf["state"].data_ptr(), n, sl.data_ptr(), s_init[s:].data_ptr(), 1, st) == 0
        # position map: the listed slots that fit (every attached one first), shuffled, with -1 holes
        att = [s for s in listed_slots if s in start and f >= start[s]]
        rest = [s for s in listed_slots if s not in att]
        n_extra = min(len(rest), max(0, B - len(att) - 2))
        extra = list(rng.choice(rest, n_extra, replace=False)) if n_extra else []
        ent = att + [int(s) for s in extra]
        ent += [-1] * (B - len(ent))
        ent = [int(e) for e in rng.permutation(ent)]
        slot_at = torch.tensor(ent, dtype=torch.int32, device="cuda")
        assert lib.tip_stream_ingest_staggered(A["state"].data_ptr(), raw[f].data_ptr(), n, A["x_imu"].data_ptr(), A["x_s"].data_ptr(),
                                               A["rows"].data_ptr(), st) == 0
        assert lib.tip_stream_ingest_mapped(M["state"].data_ptr(), raw[f].data_ptr(), n, slot_at.data_ptr(), B, M["x_imu"].data_ptr(),
                                            M["x_s"].data_ptr(), M["rows"].data_ptr(), st) == 0
        torch.cuda.synchronize()
        ra, rm = A["rows"].cpu(), M["rows"].cpu()
        for p, s in enumerate(ent):
            if s < 0:
                assert rm[p] == -1 and not M["x_imu"][p].any() and not M["x_s"][p].any()
                continue
            assert rm[p] == ra[s], (f, p, s)
            assert torch.equal(M["x_imu"][p], A["x_imu"][s]) and torch.equal(M["x_s"][p], A["x_s"][s]), (f, p, s)
        # teacher-forced rows: random finite rows where rows >= 0, NaN elsewhere (as forward_rows writes them)
        y_pos = torch.tensor(rng.randn(B, 131).astype(np.float32) * 0.3).cuda()
        y_pos[rm.cuda()[:B] < 0] = float("nan")
        y_a = torch.full((n, 131), float("nan"), device="cuda")
        for p, s in enumerate(ent):
            if s >= 0:
                y_a[s] = y_pos[p]
        untouched = (M["s_rest"][hidden].clone(), M["c_t"][hidden].clone())
        assert lib.tip_stream_consume_staggered(A["state"].data_ptr(), y_a.data_ptr(), A["rows"].data_ptr(), n, A["s_rest"].data_ptr(),
                                                A["c_t"].data_ptr(), st) == 0
        assert lib.tip_stream_consume_mapped(M["state"].data_ptr(), y_pos.data_ptr(), M["rows"].data_ptr(), slot_at.data_ptr(), B, n,
                                             M["s_rest"].data_ptr(), M["c_t"].data_ptr(), y_slot.data_ptr(), rows_slot.data_ptr(), st) == 0
        torch.cuda.synchronize()
        sa, sm = _state_rows(A["state"], n), _state_rows(M["state"], n)
        for s in listed_slots:
            assert torch.equal(sa[s], sm[s]), (f, s)
            assert torch.equal(A["s_rest"][s], M["s_rest"][s]) and torch.equal(A["c_t"][s], M["c_t"][s]), (f, s)
        for p, s in enumerate(ent):
            if s >= 0:
                assert torch.equal(y_slot[s].nan_to_num(5.0), y_pos[p].nan_to_num(5.0)) and rows_slot[s] == rm[p], (f, p, s)
        assert torch.equal(sm[hidden], hidden_bytes)
        assert torch.equal(M["s_rest"][hidden], untouched[0]) and torch.equal(M["c_t"][hidden], untouched[1])
        assert bool((y_slot[hidden] == 7.0).all()) and int(rows_slot[hidden]) == 99
    assert int((A["rows"] >= 39).sum()) > 0                   # full windows were reached


def test_mapped_entry_points_refuse_invalid_arguments():
    n = 4
    lib, state = _cbuf(n)
    st = torch.cuda.current_stream().cuda_stream
    raw = torch.zeros(n, 72, device="cuda")
    x_imu, x_s = torch.zeros(n, 40, 90, device="cuda"), torch.zeros(n, 40, 131, device="cuda")
    rows = torch.zeros(n, dtype=torch.int32, device="cuda")
    sa = torch.full((n + 1,), -1, dtype=torch.int32, device="cuda")
    y, sr, ct = torch.zeros(n + 1, 131, device="cuda"), torch.zeros(n, 111, device="cuda"), torch.zeros(n, 20, device="cuda")
    S, R, SA, XI, XS, RW, Y = (t.data_ptr() for t in (state, raw, sa, x_imu, x_s, rows, y))
    bad = -1                                                                              # TIP_ERR_INVALID_ARG
    assert lib.tip_stream_ingest_mapped(S, R, n, SA, n + 1, XI, XS, RW, st) == bad         # B > n
    assert lib.tip_stream_ingest_mapped(S, R, -1, SA, 0, XI, XS, RW, st) == bad
    assert lib.tip_stream_ingest_mapped(S, R, n, SA, -1, XI, XS, RW, st) == bad
    for j in (0, 1, 3, 5, 6, 7):
        args = [S, R, n, SA, n, XI, XS, RW, st]
        args[j] = None
        assert lib.tip_stream_ingest_mapped(*args) == bad, j
    C = [S, Y, RW, SA, n, n, sr.data_ptr(), ct.data_ptr(), None, None, st]
    assert lib.tip_stream_consume_mapped(*C[:4], n + 1, n, *C[6:]) == bad
    assert lib.tip_stream_consume_mapped(*C[:4], -1, n, *C[6:]) == bad
    assert lib.tip_stream_consume_mapped(*C[:4], 0, -1, *C[6:]) == bad
    for j in (0, 1, 2, 3, 6, 7):
        args = list(C)
        args[j] = None
        assert lib.tip_stream_consume_mapped(*args) == bad, j
    assert lib.tip_stream_ingest_mapped(S, R, n, SA, 0, XI, XS, RW, st) == 0           # B = 0: nothing to do
    assert lib.tip_stream_consume_mapped(*C[:4], 0, n, *C[6:]) == 0


def _run(m, raw, s_init, ev, compact, use_graph=False, poison=False, prewarm=False, on_frame=None):
    eng = Engine(m, s_init, use_graph=use_graph, compact=compact)
    if poison:
        eng.x_imu.fill_(float("nan"))
        eng.x_s.fill_(float("nan"))
    if prewarm:
        eng.prewarm()
    outs = []
    for f in range(raw.shape[0]):
        if ev is not None:
            det, att = ev[f]
            eng.detach(det)
            eng.attach(att, s_init[att])
        o = eng.step(raw[f])
        outs.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in o.items()})
        if on_frame is not None:
            on_frame(f, eng, o)
    torch.cuda.synchronize()
    return outs, eng


def _same(a, b, keys=KEYS, slots=None):
    for f in range(len(a)):
        for k in keys:
            x, y = a[f][k], b[f][k]
            if slots is not None:
                x, y = x[slots], y[slots]
            assert torch.equal(x.nan_to_num(7.0), y.nan_to_num(7.0)), (f, k)


@pytest.mark.parametrize("n", [1, 40, 300])
def test_no_churn_is_bit_identical_to_plain_engine(paper, n):
    """Contract 1: every slot attached, no detach — positions are the slots, B = n, and under AUTO every output of every frame is
    compact=False's."""
    m, _ = paper
    F = 120
    raw = _raw_frames(F, n, 30 + n)
    s_init = np.random.RandomState(31).randn(n, 114).astype(np.float32) * 0.2
    a, _ = _run(m, raw, s_init, None, compact=False)
    b, eng = _run(m, raw, s_init, None, compact=True)
    _same(a, b)
    assert eng.positions == list(range(n)) and all(o["active"] == n and o["batch"] == n for o in b)
    assert bool(b[-1]["valid"].all())


def test_fused_plan_premise_window_bits_do_not_depend_on_batch_or_position(paper):
    """The premise of contract 2: on the pinned plan, one window's forward_rows output is the same bits at positions 0 / 5 / 299
    of batches of 1, 7, 300 and 1024."""
    m, _ = paper
    xi1, xs1 = synth.make_inputs(synth.PAPER, 1, 40, seed=40)
    win_i, win_s = torch.tensor(xi1).cuda(), torch.tensor(xs1).cuda()
    row = 39
    m.set_plan("fused")
    try:
        got = []
        for B, positions in ((1, [0]), (7, [0, 5]), (300, [0, 5, 299]), (1024, [0, 5, 299])):
            xi, xs = synth.make_inputs(synth.PAPER, B, 40, seed=41 + B)
            xi, xs = torch.tensor(xi).cuda(), torch.tensor(xs).cuda()
            for p in positions:
                xi2, xs2 = xi.clone(), xs.clone()
                xi2[p], xs2[p] = win_i[0], win_s[0]
                rows = torch.randint(0, 40, (B,), dtype=torch.int32, device="cuda")
                rows[p] = row
                with torch.no_grad():
                    y = m.forward_rows(xi2, xs2, rows)
                got.append((B, p, y[p].cpu()))
    finally:
        m.set_plan("auto")
    for B, p, y in got:
        assert torch.isfinite(y).all()
        assert torch.equal(y, got[0][2]), (B, p)


def test_pinned_plan_is_bit_identical_per_slot_under_churn(paper):
    """Contract 2: set_plan("fused"), n = 300, attach / detach churn for 50 frames — every key of every slot is compact=False's."""
    m, _ = paper
    n, F = 300, 50
    raw = _raw_frames(F, n, 32)
    s_init = np.random.RandomState(33).randn(n, 114).astype(np.float32) * 0.2
    ev = _schedule(n, F, 34, -1)
    m.set_plan("fused")
    try:
        a, _ = _run(m, raw, s_init, ev, compact=False)
        b, _ = _run(m, raw, s_init, ev, compact=True)
    finally:
        m.set_plan("auto")
    _same(a, b)
    assert len({o["batch"] for o in b}) >= 2 and bool(b[-1]["valid"].any())


def _walk(n, F, seed, targets, swaps=2, keep=()):
    """attach / detach events that walk the attached count through `targets` (one per frame) plus `swaps` slots swapped per frame."""
    rng = np.random.RandomState(seed)
    att = set(range(n))
    ev = []
    for f in range(F):
        goal = targets[f]
        det, new = [], []
        free_att = sorted(att - set(keep))
        if len(att) > goal:
            det = [int(s) for s in rng.choice(free_att, min(len(free_att), len(att) - goal), replace=False)]
        sw = [int(s) for s in rng.choice(sorted(set(free_att) - set(det)), min(swaps, len(set(free_att) - set(det))), replace=False)]
        det += sw
        att -= set(det)
        pool = sorted(set(range(n)) - att - set(keep))
        want = max(0, goal - len(att))
        new = [int(s) for s in rng.choice(pool, min(len(pool), want), replace=False)] if want else []
        att |= set(new)
        ev.append((det, new))
    return ev


def test_auto_under_churn_stays_within_parity_of_fp64_oracle(paper):
    """Contract 3: AUTO, a 64-slot pool whose attached count crosses bucket edges — every checked valid row is the fp64 oracle's row
    of the window the ingest built for that slot (read from the engine's buffers at the slot's position)."""
    m, w = paper
    n, F = 64, 48
    raw = _raw_frames(F, n, 35)
    s_init = np.random.RandomState(36).randn(n, 114).astype(np.float32) * 0.2
    targets = [64] * 6 + [40] * 6 + [20] * 6 + [9] * 6 + [30] * 6 + [60] * 6 + [3] * 6 + [64] * 6
    ev = _walk(n, F, 37, targets)
    rng = np.random.RandomState(38)
    seen_b, checked, worst = set(), 0, 0.0

    def check(f, eng, o):
        nonlocal checked, worst
        if f < 5 or f % 2:
            return
        seen_b.add(o["batch"])
        pos = eng.positions
        rows = eng.rows[: o["batch"]].cpu().numpy()
        ps = [p for p in range(len(pos)) if rows[p] >= 0]
        if not ps:
            return
        ps = sorted(rng.choice(ps, min(12, len(ps)), replace=False))
        xi = eng.x_imu[ps].double().cpu().numpy()
        xs = eng.x_s[ps].double().cpu().numpy()
        yo = oracle.forward(synth.PAPER, w, xi, xs, dtype=np.float64)
        y = o["y_last"].cpu().numpy()
        for j, p in enumerate(ps):
            s = pos[p]
            err = float(np.abs(y[s] - yo[j, rows[p]]).max())
            worst = max(worst, err)
            assert err < TOL_PARITY, (f, s, p, int(rows[p]), err)
            checked += 1

    _run(m, raw, s_init, ev, compact=True, on_frame=check)
    assert checked > 100 and len(seen_b) >= 4, (checked, seen_b)
    print("compact pool: worst |y - oracle_f64| =", worst, "buckets", sorted(seen_b))


def test_closed_loop_golden_streams_in_churning_pool_track_reference_runner(trace, paper):
    """Contract 3, closed loop: the two golden streams sit in a 64-slot pool whose other slots churn (the attached count crosses
    bucket edges, the two streams change positions); every valid frame tracks the reference runner within TOL_LOOP."""
    m, _ = paper
    n, F = 64, 70
    gold = {10: 0, 50: 1}
    s_init = np.random.RandomState(40).randn(n, 114).astype(np.float32) * 0.2
    for s, g in gold.items():
        s_init[s] = trace[g]["s_init"]
    noise = _raw_frames(F, n, 41)
    eng = Engine(m, s_init, compact=True)
    eng.detach(list(gold))
    eng.attach(list(gold), s_init[list(gold)])                  # the two streams at the last positions: the churn moves them
    targets = [62 + 2] * 4 + [48] * 8 + [30] * 8 + [12] * 8 + [40] * 8 + [4] * 8 + [64] * 8 + [20] * 18
    ev = _walk(n, F, 42, targets, keep=tuple(gold))
    moved, batches, worst = set(), set(), 0.0
    last_pos = {s: None for s in gold}
    for f in range(F):
        det, att = ev[f]
        eng.detach(det)
        eng.attach(att, s_init[att])
        raw = noise[f].copy()
        for s, g in gold.items():
            raw[s] = trace[g]["raw_imu"][f]
        for s in gold:
            p = eng.positions.index(s)
            if last_pos[s] is not None and p != last_pos[s]:
                moved.add(s)
            last_pos[s] = p
        out = eng.step(raw)
        torch.cuda.synchronize()
        T, valid = out["T"].cpu().numpy(), out["valid"].cpu().numpy()
        for s, g in gold.items():
            if f < 5:
                assert not valid[s] and T[s] == 0 and torch.isnan(out["y_last"][s]).all()
                continue
            k = f - 5
            batches.add(out["batch"])
            assert valid[s] and T[s] == trace[g]["call_T"][k], (f, s)
            e = float(np.abs(out["s_rest"][s].cpu().numpy() - trace[g]["qdq"][f][3:]).max())
            worst = max(worst, e)
            assert e < TOL_LOOP, (f, s, e)
            assert np.abs(out["y_last"][s].cpu().numpy() - trace[g]["y_last_rows"][k]).max() < TOL_LOOP
    assert moved == set(gold) and len(batches) >= 3, (moved, batches)
    print("compact pool closed loop: worst |pose - reference| =", worst, "buckets", sorted(batches))


@pytest.mark.parametrize("n", [3, 40, 300])
def test_graph_mode_equals_launches_and_never_captures_after_prewarm(paper, n):
    """Contract 4: one captured frame per bucket, all captured by prewarm(); under churn that crosses bucket edges the graph engine
    is bit-identical to the launch-by-launch one and `captures` does not grow."""
    m, _ = paper
    F = 120
    raw = _raw_frames(F, n, 50 + n)
    s_init = np.random.RandomState(51).randn(n, 114).astype(np.float32) * 0.2
    lo = max(1, n // 5)
    targets = [n] * 10 + [max(1, n // 2)] * 20 + [lo] * 20 + [0] * 3 + [n] * 20 + [max(1, (2 * n) // 3)] * 47
    ev = _walk(n, F, 52 + n, targets, swaps=min(2, n - 1))
    a, _ = _run(m, raw, s_init, ev, compact=True)
    eng = Engine(m, s_init, use_graph=True, compact=True)
    eng.prewarm()
    c0 = eng.captures
    assert c0 == len(eng.ladder) == len(tip_amd.streaming.pool_ladder(n))
    b = []
    for f in range(F):
        det, att = ev[f]
        eng.detach(det)
        eng.attach(att, s_init[att])
        o = eng.step(raw[f])
        b.append({k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in o.items()})
    torch.cuda.synchronize()
    assert eng.captures == c0
    _same(a, b)
    assert [o["batch"] for o in a] == [o["batch"] for o in b] and len({o["batch"] for o in b}) >= min(3, n)
    m.check_handoffs()


def test_empty_pool_detach_all_and_reattach(paper):
    """k = 0 launches nothing and returns every slot as not valid; detaching everything and re-attaching restarts the slots; the
    same in graph mode."""
    m, _ = paper
    n = 6
    raw = _raw_frames(30, n, 60)
    s_init = np.random.RandomState(61).randn(n, 114).astype(np.float32) * 0.2
    for graph in (False, True):
        eng = Engine(m, s_init, use_graph=graph, compact=True)
        for f in range(8):
            out = eng.step(raw[f])
        torch.cuda.synchronize()
        assert bool(out["valid"].all())
        before = out["s_rest"].clone(), out["c_t"].clone()
        eng.detach(range(n))
        c0 = m.hip_forward_count()
        for f in range(8, 11):
            out = eng.step(raw[f])
            torch.cuda.synchronize()
            assert out["active"] == 0 and out["batch"] == 0
            assert not out["valid"].any() and not out["T"].any() and torch.isnan(out["y_last"]).all()
            assert torch.equal(out["s_rest"], before[0]) and torch.equal(out["c_t"], before[1])
        assert m.hip_forward_count() == c0
        eng.attach([4, 1], s_init[[4, 1]])
        assert eng.positions == [4, 1]
        for f in range(11, 18):
            out = eng.step(raw[f])
        torch.cuda.synchronize()
        assert out["active"] == 2 and out["batch"] == 2
        assert out["valid"].cpu().tolist() == [False, True, False, False, True, False]
        assert out["T"].cpu().tolist() == [0, 2, 0, 0, 2, 0]


def test_poisoned_buffers_are_harmless(paper):
    """NaN-filled window buffers before the first frame, churn: bit-identical to clean buffers, finite where valid."""
    m, _ = paper
    n, F = 40, 50
    raw = _raw_frames(F, n, 62)
    s_init = np.random.RandomState(63).randn(n, 114).astype(np.float32) * 0.2
    ev = _walk(n, F, 64, [40] * 10 + [12] * 20 + [33] * 20)
    a, _ = _run(m, raw, s_init, ev, compact=True)
    b, _ = _run(m, raw, s_init, ev, compact=True, poison=True)
    _same(a, b)
    for o in b:
        v = o["valid"]
        assert torch.isfinite(o["y_last"][v]).all() and torch.isnan(o["y_last"][~v]).all()
        assert torch.isfinite(o["s_rest"]).all()


def test_refusals_and_handoff_contract(paper, monkeypatch):
    """reuse=True and .train() are refused; a lost hand-off (simulated on the host, launch mode and graph mode) re-attaches every
    attached slot, keeps the positions, drops every graph and raises TipHandoffError."""
    m, _ = paper
    n = 5
    s_init = np.random.RandomState(65).randn(n, 114).astype(np.float32) * 0.2
    m.train()
    with pytest.raises(RuntimeError):
        Engine(m, s_init, compact=True)
    m.eval()
    with pytest.raises(RuntimeError):
        Engine(m, s_init, reuse=True, compact=True)
    raw = _raw_frames(20, n, 66)

    eng = Engine(m, s_init, compact=True)
    eng.detach([1])
    eng.detach([3])
    eng.attach([1], s_init[[1]])
    pos = eng.positions
    assert pos == [0, 4, 2, 1]
    for f in range(8):
        out = eng.step(raw[f])
    assert out["valid"].cpu().tolist() == [True, True, True, False, True]
    real = m.forward_rows

    def lossy(*a, **k):
        y = real(*a, **k)
        m.demotions += 1
        return y

    monkeypatch.setattr(m, "forward_rows", lossy)
    d0 = m.demotions
    with pytest.raises(tlib.TipHandoffError):
        eng.step(raw[8])
    monkeypatch.setattr(m, "forward_rows", real)
    m.demotions = d0
    assert eng.positions == pos and eng.attached == [True, True, True, False, True]
    for f in range(6):
        out = eng.step(raw[9 + f])
        torch.cuda.synchronize()
        assert out["T"].cpu().tolist() == ([0] * 5 if f < 5 else [1, 1, 1, 0, 1])

    eng = Engine(m, s_init, use_graph=True, compact=True)
    eng.detach([2])
    eng.prewarm()
    for f in range(7):
        eng.step(raw[f])
    pos, c0 = eng.positions, eng.captures
    assert eng._graphs

    def lost(synchronize=True, clear=False):
        raise tlib.TipHandoffError(tlib.TIP_ERR_HANDOFF, "simulated")

    monkeypatch.setattr(m, "check_handoffs", lost)
    monkeypatch.setattr(m, "_answer_handoff", lambda h: "demoted")
    with pytest.raises(tlib.TipHandoffError):
        eng.step(raw[7])
    monkeypatch.undo()
    assert not eng._graphs and eng.positions == pos
    for f in range(6):
        out = eng.step(raw[8 + f])
        torch.cuda.synchronize()
        assert out["T"].cpu().tolist() == ([0] * 5 if f < 5 else [1, 1, 0, 1, 1])
    assert eng.captures == c0 + 1
    with pytest.raises(ValueError):
        eng.prewarm([7])
