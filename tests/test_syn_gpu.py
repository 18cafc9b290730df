"""tip_amd.syndata on the device (csrc/tip_syn.hip) against the reference-generated golden (tests/golden/tip_syn_golden.npz) and
tests/syn_oracle.py.  The skeleton comes from the golden's table only.

THE BOUND, derived and not measured: the path is fp64 end to end (unit roundoff 1.1e-16) on magnitudes <= 10, through about a
hundred operations and the x 225 of the second difference: ~2e-11.  BOUND = 1e-9 leaves 50 x.  Flags are compared exactly: the
fixture was built with every on-frame's argmin gap >= 1e-8 and every frame's |min - V_THRES| >= 1e-5 (tests/test_syn_cpu.py holds
it to that), both far above the bound, so no decision can flip and no frame is left out of any comparison.  Inputs that are not the
fixture's (the 9-row sequence, the NaN rows) have the same two conditions asserted on the oracle's trace before anything is compared."""
import numpy as np
import pytest
import torch

import syn_oracle as so
from tip_amd import data
from tip_amd import kinematics as kin
from tip_amd import syndata as syn

pytestmark = pytest.mark.gpu
BOUND = 1e-9
GAP_GUARD, MARGIN_GUARD = 1e-8, 1e-5
GOLDEN = np.load(__file__.replace("test_syn_gpu.py", "golden/tip_syn_golden.npz"))
TABLE = {k[len("table/"):]: GOLDEN[k] for k in GOLDEN.files if k.startswith("table/")}
TAGS = ("A", "B", "C")
Q = {t: GOLDEN[f"{t}/q"] for t in TAGS}
SCALE = {t: float(GOLDEN[f"{t}/scale"]) for t in TAGS}


@pytest.fixture(scope="module")
def skel():
    return kin.Skeleton.from_table(GOLDEN)


def _run(skel, qs, scales):
    """synthesize -> [(imu, constrs)] as numpy."""
    files = syn.synthesize(skel, qs, scales)
    for f, q in zip(files, qs):
        assert f["nimble_qdq"] is q                                        # passed through, not copied or scaled
        assert f["imu"].is_cuda and f["imu"].dtype == torch.float64 and tuple(f["imu"].shape) == (q.shape[0], 72)
        assert f["constrs"].is_cuda and f["constrs"].dtype == torch.float64 and tuple(f["constrs"].shape) == (q.shape[0], 20)
    return [(f["imu"].cpu().numpy(), f["constrs"].cpu().numpy()) for f in files]


@pytest.fixture(scope="module")
def clean(skel):
    """A, B and C in ONE ragged call; every test below compares against these arrays and leaves them alone."""
    return dict(zip(TAGS, _run(skel, [Q[t] for t in TAGS], [SCALE[t] for t in TAGS])))


def _same(a, b):
    """Bit for bit, NaN included."""
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _guards(tr, flags, what):
    """The two conditions under which a comparison against the oracle is exact in its decisions (rows with a finite search only)."""
    gap, mar = tr["gap"][2:-2], tr["margin"][2:-2]
    on = flags[2:-2] == 1
    g = float(gap[on].min()) if on.any() else np.inf
    m = float(mar[np.isfinite(mar)].min())
    print(f"{what}: oracle's smallest on-frame argmin gap {g:.2e}, smallest threshold margin {m:.2e}")
    assert g >= GAP_GUARD and m >= MARGIN_GUARD, what


def _compare(got, ref, what):
    """imu and offsets within BOUND, NaN exactly where the reference has it, flags equal."""
    (imu, c), (r_imu, r_c) = got, ref
    assert np.array_equal(np.isnan(imu), np.isnan(r_imu)) and np.array_equal(np.isnan(c), np.isnan(r_c)), what
    e_imu = float(np.nanmax(np.abs(imu - r_imu)))
    e_off = float(np.nanmax(np.abs(c - r_c)))
    print(f"{what}: |imu - ref| {e_imu:.2e} (orientations {float(np.nanmax(np.abs(imu[:, :54] - r_imu[:, :54]))):.2e}), "
          f"|offsets - ref| {e_off:.2e}, on-frames {c[:, 0::4].sum(0).astype(int).tolist()}")
    assert np.array_equal(c[:, 0::4], r_c[:, 0::4]), what
    assert e_imu <= BOUND and e_off <= BOUND, what


# ---- parity with the reference's arrays ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_parity_with_the_golden(clean, tag):
    _compare(clean[tag], (GOLDEN[f"{tag}/imu"], GOLDEN[f"{tag}/constrs"]), tag)
    c = clean[tag][1]
    assert not c[:2].any() and not c[-2:].any()
    if tag == "C":
        assert c[2:-2, 0::4].all()                                        # one fixed pose: every searched row is on


# ---- independence --------------------------------------------------------------------------------------------------------------------
def test_each_sequence_alone_equals_its_rows_in_the_batch(skel, clean):
    for t in TAGS:
        (imu, c), = _run(skel, [Q[t]], [SCALE[t]])
        assert _same(imu, clean[t][0]) and _same(c, clean[t][1]), t


def test_a_permuted_batch_gives_the_permuted_rows(skel, clean):
    order = ("C", "A", "B")
    for t, (imu, c) in zip(order, _run(skel, [Q[t] for t in order], [SCALE[t] for t in order])):
        assert _same(imu, clean[t][0]) and _same(c, clean[t][1]), t
    # and from device tensors with more columns than are read
    wide = [torch.from_numpy(np.concatenate([Q[t], np.full((Q[t].shape[0], 57), 7.0)], axis=1)).cuda() for t in TAGS]
    for t, (imu, c) in zip(TAGS, _run(skel, wide, [SCALE[t] for t in TAGS])):
        assert _same(imu, clean[t][0]) and _same(c, clean[t][1]), t


# ---- edges ---------------------------------------------------------------------------------------------------------------------------
def test_the_smallest_legal_length_and_its_neighbour(skel, clean):
    """L = 9: one differenced row (row 4, copied to all nine) and label rows 2 .. 6.  Rows 28 .. 36 of A: four of the five bodies have
    on-frames there.  The sequence after it in the batch keeps its bits: the padding is clamped into a sequence's own rows."""
    nine = np.ascontiguousarray(Q["A"][28:37])
    r_imu, r_c, tr = so.synthesize(TABLE, nine, 1.1)
    _guards(tr, r_c[:, 0::4], "L = 9")
    assert r_c[2:7, 0::4].sum() >= 5
    (imu, c), (a_imu, a_c), (imu2, c2) = _run(skel, [nine, Q["A"], nine], [1.1, SCALE["A"], 1.1])
    _compare((imu, c), (r_imu, r_c), "L = 9")
    assert (imu[:, 54:] == imu[4, 54:]).all() and not c[:2].any() and not c[7:].any()
    assert _same(a_imu, clean["A"][0]) and _same(a_c, clean["A"][1])
    assert _same(imu2, imu) and _same(c2, c)                              # and a 9-row sequence at the end of the batch


def test_eight_rows_are_refused(skel):
    with pytest.raises(ValueError, match="has 8 rows"):
        syn.synthesize(skel, [Q["A"], np.ascontiguousarray(Q["A"][:8])], [1.0, 1.0])


# ---- non-finite input ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [40, 64])
def test_a_nan_row_stays_in_its_own_sequence_and_resets_the_chain(skel, clean, row):
    """One NaN in B's q: row 40 (a fast stretch, the labels around it are off anyway) and row 64 (all five chains are on around it).
    B equals the oracle on that input — NaN exactly where the oracle has it (the row's own orientations, the accelerations of rows
    row - 4, row, row + 4), flag 0 on rows row - 1 and row + 1, the chains starting over after — and A and C keep their bits."""
    q = Q["B"].copy()
    q[row, 4] = np.nan
    r_imu, r_c, tr = so.synthesize(TABLE, q, SCALE["B"])
    _guards(tr, r_c[:, 0::4], f"NaN in row {row}")
    assert not r_c[row - 1, 0::4].any() and not r_c[row + 1, 0::4].any() and not np.isnan(r_c).any()
    assert sorted(set(np.nonzero(np.isnan(r_imu))[0].tolist())) == [row - 4, row, row + 4]
    assert r_c[row + 2:, 0::4].any()                                      # the chains do start over
    (a_imu, a_c), (imu, c), (c_imu, c_c) = _run(skel, [Q["A"], q, Q["C"]], [SCALE[t] for t in TAGS])
    _compare((imu, c), (r_imu, r_c), f"B with NaN in row {row}")
    assert _same(a_imu, clean["A"][0]) and _same(a_c, clean["A"][1]) and _same(c_imu, clean["C"][0]) and _same(c_c, clean["C"][1])
    if row == 64:
        assert clean["B"][1][63, 0::4].all() and clean["B"][1][65, 0::4].all()      # they were on in the clean run


# ---- the pipeline: synthesize -> combine_motions without leaving the card -----------------------------------------------------------
def test_combine_motions_takes_the_device_tensors_in_place(skel):
    qs = [np.concatenate([Q[t], np.zeros((Q[t].shape[0], 57))], axis=1) for t in TAGS]          # nimble_qdq is 114 wide
    qs[1] = torch.from_numpy(qs[1]).cuda()                                 # one of them already on the device
    files = syn.synthesize(skel, qs, [SCALE[t] for t in TAGS])
    host = [{k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in f.items()} for f in files]
    biases = np.random.RandomState(3).uniform(-0.1, 0.1, (3, 18))
    dev = data.combine_motions(files, [1, 2, 1], biases=biases)
    ref = data.combine_motions(host, [1, 2, 1], biases=biases)
    assert np.array_equal(dev.info, ref.info) and dev.info.shape[0] == 2   # C (24 rows) is "too short" for the combiner, as a pickle of it is
    for name in ("IMU", "SUM", "S"):
        a, b = getattr(dev, name), getattr(ref, name)
        assert a.shape == b.shape and a.shape[0] == int(dev.info[-1, 1]) and torch.equal(a, b), name
        assert bool(torch.isfinite(a).all()), name
    with pytest.raises(ValueError, match="CUDA fp64"):
        data.combine_motions([dict(files[0], imu=files[0]["imu"].float())], [1], biases=biases)
    with pytest.raises(ValueError, match="CUDA fp64"):
        data.combine_motions([dict(files[0], constrs=files[0]["constrs"].cpu())], [1], biases=biases)
