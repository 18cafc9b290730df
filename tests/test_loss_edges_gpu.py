"""GPU: the fused training losses (csrc/tip_loss.hip) against oracle/loss_oracle.py (float64) where the kernels' 16-row tiles,
their dynamic LDS and their C ABI have edges: fp64 rows wide enough for more than 64 KB of LDS, window lengths that sit
awkwardly on the tile, row layouts narrow enough for several row groups per tile, and strided buffers with term subsets.
Bounds as in test_loss_gpu.py: 2e-6 of the largest oracle entry for fp32 runs, 1e-12 for fp64 runs."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from make_loss_golden import N_SBPS, make_case, make_constr_case             # noqa: E402
import tip_amd                                                                # noqa: E402
from oracle import loss_oracle                                                # noqa: E402
from test_loss_oracle import NARROW_LAYOUTS, NARROW_SHAPES, make_narrow_case  # noqa: E402

pytestmark = pytest.mark.gpu
REL = {np.float32: 2e-6, np.float64: 1e-12}
DTYPES = [np.float32, np.float64]


def check_train_loss(tag, pred, gt, n_sbps, dtype):
    """train_loss (total, parts, gradient) at one precision against the fp64 oracle; NaN totals as the reference's."""
    rel = REL[dtype]
    o_total, o_parts, o_grad = loss_oracle.train_loss(pred, gt, n_sbps, f32_sigmoid=dtype is np.float32)
    yp = torch.tensor(pred.astype(dtype)).cuda().requires_grad_(True)
    total, parts = tip_amd.learning_utils.train_loss(yp, torch.tensor(gt.astype(dtype)).cuda(), n_sbps, return_parts=True)
    assert total.dtype == yp.dtype
    total.backward()                                                          # a NaN total still back-propagates
    got = np.array([float(total.detach()), *parts.cpu().numpy().astype(np.float64)])
    want = np.array([o_total, *o_parts])
    grad = yp.grad.cpu().numpy().astype(np.float64)
    fin = np.isfinite(want)
    e_grad = np.abs(grad - o_grad).max() / np.abs(o_grad).max()
    print(f"{tag}: oracle {want} got {got} grad rel err {e_grad:.3g}")
    assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, got, want)
    assert np.isfinite(grad).all(), tag                                       # also under a NaN total
    if fin[0]:
        assert abs(got[0] - want[0]) <= rel * abs(want[0]), (tag, got, want)
    if fin[1:].any():
        assert np.abs(got[1:] - want[1:])[fin[1:]].max() <= rel * np.abs(want[1:][fin[1:]]).max(), (tag, got, want)
    assert np.abs(grad - o_grad).max() <= rel * np.abs(o_grad).max(), (tag, e_grad)
    # rows a NaN ground truth masks: exactly zero
    W = pred.shape[-1]
    nq = W - 4 * n_sbps
    mv = np.isnan(gt[:, :, nq - 3:nq - 1]).any(axis=2)
    mc = np.isnan(gt[:, :, nq:]).any(axis=2)
    assert np.all(grad[mv][:, nq - 3:nq] == 0.0) and np.all(grad[mc][:, nq:] == 0.0), tag
    return want


# ---- fp64 rows on both sides of 64 KB of dynamic LDS ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_c", [53, 54, 58, 59, 64])
def test_fp64_constraint_rows_past_64kb_of_lds(n_c):
    """loss_constr_multi in fp64 with W = 4 n_c = 212, 216, 232, 236, 256: the gradient kernel asks for 38 W doubles of LDS
    (64 448, 65 664, 70 528, 71 744, 77 824 bytes), the reduction kernel for 35 W (59 360, 60 480, 64 960, 66 080, 71 680)."""
    assert torch.cuda.is_available()
    gt, pred = (a.astype(np.float64) for a in make_constr_case(n_c, 45, 300 + n_c))
    o_loss, o_grad = loss_oracle.loss_constr_multi(gt, pred, f32_sigmoid=False)

    def run():
        rb = torch.tensor(pred).cuda().requires_grad_(True)
        loss = tip_amd.learning_utils.loss_constr_multi(torch.tensor(gt).cuda(), rb)
        assert loss.dtype == torch.float64
        loss.backward()
        return float(loss.detach()), rb.grad.cpu().numpy()

    loss, g = run()
    print(f"n_c {n_c}: oracle {o_loss!r} got {loss!r} grad err {np.abs(g - o_grad).max() / np.abs(o_grad).max():.3g}")
    assert abs(loss - o_loss) <= 1e-12 * abs(o_loss), (loss, o_loss)
    assert np.isfinite(g).all() and np.all(g[7] == 0.0)                       # the NaN-masked row
    assert np.abs(g - o_grad).max() <= 1e-12 * np.abs(o_grad).max()
    loss2, g2 = run()
    assert loss2 == loss and np.array_equal(g, g2)                            # deterministic


# ---- window lengths against the 16-row tile ------------------------------------------------------------------------------------

# (B, T): one third difference per window | window == tile | the +3 halo and the row0 - 3 lead across a window and a tile
# boundary at once | M < 16 | M % 16 in {1, 15} | T <= 3: no jerk sample, NaN total
WINDOW_SHAPES = [(1, 4), (3, 4), (1, 16), (2, 16), (3, 17), (5, 19), (1, 15), (1, 1), (7, 7)]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("B,T", WINDOW_SHAPES)
def test_window_lengths_against_the_row_tile(B, T, dtype):
    pred, gt = make_case("mix", B, T, 50 + B * T)
    want = check_train_loss(f"B{B} T{T} {dtype.__name__}", pred, gt, N_SBPS, dtype)
    assert np.isnan(want[3]) == (T <= 3) and (T > 3 or np.isnan(want[0]))     # no jerk sample: NaN like the reference


# ---- narrow layouts: several row groups of a tile side by side -----------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("B,T", NARROW_SHAPES)
@pytest.mark.parametrize("n_pose,n_sbps", NARROW_LAYOUTS)
def test_narrow_layouts(n_pose, n_sbps, B, T, dtype):
    """W = 23 (11 row groups of 2 rows) and W = 67 (3 row groups of 6 rows): the third difference starts in the middle of a tile,
    so the jerk gradient's three previous differences are pre-filled from rows of the same tile."""
    pred, gt = make_narrow_case(n_pose, n_sbps, B, T, 40 + B + n_pose)
    want = check_train_loss(f"W{pred.shape[-1]} B{B} T{T} {dtype.__name__}", pred, gt, n_sbps, dtype)
    assert np.isfinite(want).all()


# ---- the C ABI: strided rows, term subsets, every column written ---------------------------------------------------------------

Q, C, J = tip_amd.lib.TIP_LOSS_Q, tip_amd.lib.TIP_LOSS_C, tip_amd.lib.TIP_LOSS_J


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "fp64"])
@pytest.mark.parametrize("terms", [Q, C, J, Q | J], ids=["Q", "C", "J", "QJ"])
def test_c_abi_strides_and_term_subsets(terms, dtype):
    """ld_pred = 140, ld_gt = 135, ld_dpred = 150 on the full 131-column layout; dpred pre-filled with NaN."""
    lib = tip_amd.lib.load()
    f64 = dtype is np.float64
    fwd, bwd = (lib.tip_loss_forward_f64, lib.tip_loss_backward_f64) if f64 else (lib.tip_loss_forward, lib.tip_loss_backward)
    rel, tdt = REL[dtype], torch.float64 if f64 else torch.float32
    B, T = 3, 12
    M = B * T
    pred, gt = make_case("mix", B, T, 0)
    # the oracle, term by term
    p2, g2 = pred.reshape(M, 131), gt.reshape(M, 131)
    lq, gq = loss_oracle.loss_q_only_2axis(g2[:, :111], p2[:, :111])
    lc, gc = loss_oracle.loss_constr_multi(g2[:, 111:], p2[:, 111:], f32_sigmoid=not f64)
    lj, gj = loss_oracle.loss_jerk(pred[:, :, :108])
    o_grad = np.zeros((M, 131))
    if terms & Q:
        o_grad[:, :111] += gq
    if terms & C:
        o_grad[:, 111:] += gc
    if terms & J:
        o_grad[:, :108] += gj.reshape(M, 108)
    o_parts = np.array([lq if terms & Q else 0.0, lc if terms & C else 0.0, lj if terms & J else 0.0])
    o_total = (o_parts[1] + o_parts[0]) + o_parts[2]
    assert np.isfinite(o_total) and np.abs(o_grad).max() > 0
    # padded device rows: nothing in the padding may be read (NaN) or written
    P = torch.full((M, 140), float("nan"), dtype=tdt)
    G = torch.full((M, 135), float("nan"), dtype=tdt)
    P[:, :131], G[:, :131] = torch.tensor(p2.astype(dtype)), torch.tensor(g2.astype(dtype))
    P, G = P.cuda(), G.cuda()
    stats = torch.full((tip_amd.lib.TIP_LOSS_STATS,), float("nan"), dtype=tdt, device="cuda")
    nb = ctypes.c_size_t()
    assert lib.tip_loss_ws_bytes(B, T, ctypes.byref(nb)) == 0
    ws = torch.zeros(nb.value // 8, dtype=torch.float64, device="cuda")
    rc = fwd(P.data_ptr(), 140, G.data_ptr(), 135, B, T, 108, 3, N_SBPS, terms, stats.data_ptr(), ws.data_ptr(), nb.value, None)
    torch.cuda.synchronize()
    assert rc == 0                                                            # TIP_OK
    st = stats.cpu().numpy().astype(np.float64)
    print(f"terms {terms} {dtype.__name__}: stats {st[:4]} oracle {o_total} {o_parts}")
    assert np.isfinite(st[:4]).all()
    assert abs(st[0] - o_total) <= rel * abs(o_total)
    assert np.abs(st[1:4] - o_parts).max() <= rel * np.abs(o_parts).max()
    for i, bit in enumerate((Q, C, J)):
        if not terms & bit:
            assert st[1 + i] == 0.0                                           # a term not selected reports exactly 0
    groups = ((slice(0, 108), Q | J), (slice(108, 111), Q), (slice(111, 131), C))
    gout = torch.tensor([1.7], dtype=tdt, device="cuda")
    for go_ptr, go in ((None, 1.0), (gout.data_ptr(), float(gout.cpu()[0]))):   # NULL = 1; a device scalar
        D = torch.full((M, 150), float("nan"), dtype=tdt, device="cuda")
        rc = bwd(P.data_ptr(), 140, G.data_ptr(), 135, B, T, 108, 3, N_SBPS, terms, stats.data_ptr(), go_ptr, D.data_ptr(), 150, None)
        torch.cuda.synchronize()
        assert rc == 0
        d = D.cpu().numpy().astype(np.float64)
        assert np.isnan(d[:, 131:]).all()                                     # the padding of dpred is not touched
        assert np.isfinite(d[:, :131]).all()                                  # every column of the layout is written
        err = np.abs(d[:, :131] - go * o_grad).max()
        print(f"  gout {go}: grad err {err / (go * np.abs(o_grad).max()):.3g}")
        assert err <= rel * go * np.abs(o_grad).max()
        for cols, users in groups:
            if not terms & users:
                assert np.all(d[:, cols] == 0.0), cols                        # exactly 0, not left as it was
