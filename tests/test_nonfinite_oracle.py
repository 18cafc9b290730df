"""CPU: what a non-finite input does in the two CPU restatements of the reference forward (simple_transformer_with_state.py:60-102),
and the harness that holds the HIP path to it (tests/test_nonfinite_isolation_gpu.py imports Poison / poisoned / check_isolation).

The contract.  One call has B windows; a set P of them is poisoned at row r: a quiet NaN, +Inf or -Inf in
x_imu (any column), or +-Inf in x_s (a NaN there is scrubbed at :65, which older tests pin).
  1. every window outside P equals the clean call bit for bit;
  2. in a window of P every column of every row >= r is NaN;
  3. in a window of P each row < r is either bit-equal to the clean call (the C oracle: strictly causal) or all-NaN (the stock
     modules: their additive -inf mask turns NaN + (-inf) into NaN for every query) — never finite and different.
A +-Inf in the root-velocity history columns 108-110 is no exception: :75 multiplies them by 0.0, and 0 * Inf is NaN.
"""
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import pytest
import torch

from tip_amd import synth
from oracle import oracle, torch_stock

NAN, INF = float("nan"), float("inf")


@dataclass(frozen=True)
class Poison:
    tensor: str                 # "x_imu" or "x_s"
    windows: Tuple[int, ...]    # the set P
    row: int                    # r
    col: int
    value: float                # float("nan"), +Inf or -Inf


def poisoned(x_imu, x_s, p: Poison):
    """Copies of the clean inputs with p applied."""
    assert p.tensor in ("x_imu", "x_s") and not np.isfinite(p.value)
    assert p.tensor == "x_imu" or not np.isnan(p.value), "a NaN in x_s is scrubbed: not a poison"
    xi, xs = np.array(x_imu, copy=True), np.array(x_s, copy=True)
    (xi if p.tensor == "x_imu" else xs)[list(p.windows), p.row, p.col] = p.value
    return xi, xs


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_outputs(y_bad, y_clean, p: Poison, rows=None, tag=""):
    """Items 1-3 on one output form: the full output [B,T,S] (rows=None), or one row per window [B,S] where rows[b] says which
    (an int = the same row for every window: T-1 for the last-row form).  Returns item 3's answers for this call, row by row: a subset
    of {"bit-equal", "nan"} (a kernel that skips key blocks above the diagonal may give both), empty when no row < r was looked at."""
    y_bad, y_clean = np.asarray(y_bad), np.asarray(y_clean)
    assert y_bad.shape == y_clean.shape and y_bad.dtype == y_clean.dtype, (tag, y_bad.shape, y_clean.shape)
    B = y_bad.shape[0]
    if y_bad.ndim == 3:
        assert rows is None
        row_of = np.broadcast_to(np.arange(y_bad.shape[1]), y_bad.shape[:2])
    else:
        row_of = np.broadcast_to(np.asarray(rows), (B,))[:, None]
        y_bad, y_clean = y_bad[:, None], y_clean[:, None]
    assert np.isfinite(y_clean).all(), (tag, "the clean call is not finite")
    others = np.setdiff1d(np.arange(B), np.array(p.windows))
    same = (_bits(y_bad) == _bits(y_clean)).all(axis=2)                    # [B, rows]
    nan_row = np.isnan(y_bad).all(axis=2)
    leaked = others[~same[others].all(axis=1)]                             # item 1: ALL other windows, bit for bit
    assert leaked.size == 0, (tag, p, "windows outside P differ from the clean call", leaked[:8].tolist(),
                              "of them NaN somewhere:", [int(b) for b in leaked[:8] if np.isnan(y_bad[b]).any()])
    answers = set()
    for b in p.windows:
        late = row_of[b] >= p.row
        assert nan_row[b][late].all(), (tag, p, "item 2: a row >= r of a poisoned window is not NaN in every column", b,
                                        row_of[b][late][~nan_row[b][late]][:8].tolist())
        early = ~late
        ok = same[b] | nan_row[b]
        assert ok[early].all(), (tag, p, "item 3: a row < r of a poisoned window is finite and different", b,
                                 row_of[b][early][~ok[early]][:8].tolist())
        answers |= {"nan" if n else "bit-equal" for n in nan_row[b][early]}
    return answers


def check_isolation(run, x_imu, x_s, p: Poison, y_clean=None, tag=""):
    """run(x_imu, x_s) -> y [B,T,S].  Items 1-3 of the contract for poison p; returns (y_bad, item 3's answers)."""
    if y_clean is None:
        y_clean = run(x_imu, x_s)
    y_bad = run(*poisoned(x_imu, x_s, p))
    return y_bad, check_outputs(y_bad, y_clean, p, tag=tag)


# ----------------------------------------------------------------------------------------------------------------------
CFG = synth.PAPER
B, T = 4, 40
ROWS = (0, 17, 39)
SPOTS = [("x_imu", 5, NAN), ("x_imu", 5, INF), ("x_imu", 5, -INF), ("x_s", 7, INF), ("x_s", 7, -INF)]


@pytest.fixture(scope="module")
def world():
    w = synth.make_weights(CFG, seed=0)
    x_imu, x_s = synth.make_inputs(CFG, B, T, seed=42)
    stock = torch_stock.build(CFG, w).double()

    def run_c(xi, xs):
        return oracle.forward(CFG, w, xi, xs, dtype=np.float64)

    def run_stock(xi, xs):
        with torch.no_grad():
            return stock(torch.tensor(xi, dtype=torch.float64), torch.tensor(xs, dtype=torch.float64)).numpy()

    return {"x": (x_imu, x_s), "c": run_c, "stock": run_stock, "clean_c": run_c(x_imu, x_s), "clean_stock": run_stock(x_imu, x_s)}


@pytest.mark.parametrize("r", ROWS)
def test_c_oracle_is_strictly_causal_inside_the_poisoned_window(world, r):
    for tensor, col, v in SPOTS:
        p = Poison(tensor, (1,), r, col, v)
        _, ans = check_isolation(world["c"], *world["x"], p, y_clean=world["clean_c"], tag="c")
        assert ans == ({"bit-equal"} if r else set()), (p, ans)


@pytest.mark.parametrize("r", ROWS)
def test_stock_modules_answer_nan_for_the_whole_poisoned_window(world, r):
    for tensor, col, v in SPOTS:
        p = Poison(tensor, (1,), r, col, v)
        _, ans = check_isolation(world["stock"], *world["x"], p, y_clean=world["clean_stock"], tag="stock")
        assert ans == ({"nan"} if r else set()), (p, ans)


def test_several_poisoned_windows(world):
    p = Poison("x_imu", (0, 3), 17, 60, NAN)
    assert check_isolation(world["c"], *world["x"], p, y_clean=world["clean_c"])[1] == {"bit-equal"}
    assert check_isolation(world["stock"], *world["x"], p, y_clean=world["clean_stock"])[1] == {"nan"}


def test_last_row_and_chosen_row_forms(world):
    """check_outputs on [B,S] outputs: the last row, and one chosen row per window on both sides of r."""
    p = Poison("x_imu", (1,), 17, 5, NAN)
    y_bad, _ = check_isolation(world["c"], *world["x"], p, y_clean=world["clean_c"])
    yc = world["clean_c"]
    assert check_outputs(y_bad[:, -1], yc[:, -1], p, rows=T - 1) == set()
    rows = np.array([3, 16, 17, 30])
    pick = (np.arange(B), rows)
    assert check_outputs(y_bad[pick], yc[pick], p, rows=rows) == {"bit-equal"}
    rows[1] = 17
    pick = (np.arange(B), rows)
    assert check_outputs(y_bad[pick], yc[pick], p, rows=rows) == set()
    with pytest.raises(AssertionError, match="item 2"):                    # the clean rows passed off as the poisoned call's
        check_outputs(yc[pick], yc[pick], p, rows=rows)


@pytest.mark.parametrize("v", [INF, -INF])
def test_inf_in_a_root_velocity_column_is_nan_in_the_reference(world, v):
    """:75 is `*= 0.0`: 0 * Inf = NaN, and the C oracle multiplies too.  torch_stock.py overwrites those columns with zeros and stays
    finite there (its docstring says so); the HIP path follows the reference."""
    for r in ROWS:
        p = Poison("x_s", (1,), r, 109, v)
        _, ans = check_isolation(world["c"], *world["x"], p, y_clean=world["clean_c"])
        assert ans == ({"bit-equal"} if r else set())
        xi, xs = poisoned(*world["x"], p)
        assert np.array_equal(world["stock"](xi, xs), world["clean_stock"])


# -- the harness can fail ----------------------------------------------------------------------------------------------
def test_harness_catches_a_cross_window_zero_times_nan_leak(world):
    """Window b's last row picks up 0 * (window b-1's last row): nothing for finite data, NaN behind a poisoned window."""
    def run(xi, xs):
        y = world["c"](xi, xs)
        y[1:, -1] += 0.0 * y[:-1, -1]
        return y
    assert np.array_equal(run(*world["x"]), world["clean_c"])              # invisible to every finite-input test
    for r in ROWS:
        with pytest.raises(AssertionError, match="windows outside P differ"):
            check_isolation(run, *world["x"], Poison("x_imu", (1,), r, 5, NAN))
    check_isolation(run, *world["x"], Poison("x_imu", (B - 1,), 17, 5, NAN))   # (nobody sits behind the last window)


def test_harness_catches_a_hidden_nan(world):
    """Non-finite outputs replaced by zeros: finite-but-wrong where the contract wants NaN."""
    def run(xi, xs):
        y = world["c"](xi, xs)
        y[~np.isfinite(y)] = 0.0
        return y
    for tensor, col, v in SPOTS:
        with pytest.raises(AssertionError, match="item 2"):
            check_isolation(run, *world["x"], Poison(tensor, (1,), 17, col, v))


def test_harness_catches_finite_and_different_early_rows(world):
    def run(xi, xs):
        y = world["c"](xi, xs)
        bad = np.isnan(y).any(axis=(1, 2))
        y[bad, 0] += 1e-9
        return y
    with pytest.raises(AssertionError, match="item 3"):
        check_isolation(run, *world["x"], Poison("x_imu", (1,), 17, 5, NAN))
