"""The forward's schedule without a GPU: which plan(s) AUTO picks, when a batch is split into whole rounds + a remainder and when the two
share one recurrence and one output projection (csrc/tip_schedule.hip through tip_debug_schedule).  A handle made without a device reports
256 CUs — the MI355X's count — so the whole decision table of the paper configuration is pinned here, against the rules as the
measurements state them (written out again below, not read back from the library)."""
from math import ceil

import pytest

from tip_amd import lib as tlib
from tip_amd import synth

LAT, SPLIT, HYBRID, TWOWIN, GENERAL = (tlib.TIP_PLAN_LATENCY, tlib.TIP_PLAN_FUSED1S, tlib.TIP_PLAN_FUSEDH, tlib.TIP_PLAN_FUSED2,
                                        tlib.TIP_PLAN_GENERAL)
CUS = 256
ROWS4 = tlib.TIP_RNN_CLUSTER_ROWS4
B_ALL = range(1, 2101)


def handle(cfg):
    return tlib.Handle(tlib.TipConfig(cfg["input_size_imu"], cfg["size_s"], cfg["rnn_hid_size"], cfg["tf_hid_size"], cfg["tf_in_dim"],
                                      cfg["n_heads"], cfg["tf_layers"], 1 if cfg.get("with_rnn", True) else 0,
                                      1 if cfg.get("with_acc_sum", False) else 0, 40))


@pytest.fixture(scope="module")
def paper():
    return handle(synth.PAPER)


# ---- the rules, paper configuration, T = 40, a whole 256-CU device (microseconds) ----
def few_windows(n, lat_bound=32):
    """Latency plan up to 32 windows (48 when the window-split encoder is held to two CUs per window), window-split encoder up to
    #CUs / 2 = 128, beyond that neither."""
    return LAT if 1 <= n <= lat_bound else SPLIT if 1 <= n <= CUS // 2 else None


def rounds(n):
    """(encoder, its time): two windows per workgroup at 1049 us per round of 512 windows, or one at 527 per round of 256."""
    two, one = 1049 * ceil(ceil(n / 2) / CUS), 527 * ceil(n / CUS)
    return (TWOWIN, two) if two < one else (HYBRID, one)


def one_sequence_us(n):
    return rounds(n)[1] + 96 * ceil(n / CUS)            # + recurrence and projection per round


def latency_us(n):
    return 147 + n // 4 if n <= 8 else 181 if n <= 16 else 241 if n <= 24 else 200 + int(3.6 * (n - 8))


def expected(B):
    single = dict(nparts=1, shared_tail=False, parts=[(0, B, few_windows(B) or rounds(B)[0])])
    r = B % CUS
    whole = B - r
    if B <= CUS or few_windows(r) is None:
        return single
    two = dict(nparts=2, shared_tail=False, parts=[(0, whole, rounds(whole)[0]), (whole, r, few_windows(r))])
    if few_windows(r) == SPLIT:
        quad = r <= CUS // 4                             # one window on four CUs
        tiles = lambda n: ceil(ceil(n / 4) / 64)        # noqa: E731  four-window tiles per recurrence cluster
        if (tiles(B) <= 2 or (tiles(B) <= 4 and tiles(whole) >= 3)) and \
                one_sequence_us(whole) + (232 if quad else 375) + 35 < one_sequence_us(B):
            return dict(two, shared_tail=True)
        rem = 305 if quad else 452
    else:
        rem = latency_us(r)
    return two if one_sequence_us(whole) + rem < one_sequence_us(B) else single


def strip(s):
    return {k: s[k] for k in ("nparts", "shared_tail", "parts")}


def test_auto_table_of_the_paper_configuration(paper):
    for B in B_ALL:
        s = paper.schedule(B, 40)
        assert strip(s) == expected(B), B
        assert s["rnn_cluster"] == ROWS4, B
        # the parts tile [0, B)
        assert s["parts"][0][0] == 0 and sum(c for _, c, _ in s["parts"]) == B
        assert all(a[0] + a[1] == b[0] for a, b in zip(s["parts"], s["parts"][1:])), B
        assert s["shared_tail"] is False or s["nparts"] == 2


@pytest.mark.parametrize("B, plan", [(1, LAT), (24, LAT), (32, LAT), (33, SPLIT), (64, SPLIT), (65, SPLIT), (128, SPLIT), (129, HYBRID),
                                     (256, HYBRID), (512, TWOWIN), (1024, TWOWIN)])
def test_single_sequence_cases(paper, B, plan):
    assert strip(paper.schedule(B, 40)) == dict(nparts=1, shared_tail=False, parts=[(0, B, plan)])


@pytest.mark.parametrize("B, rem_plan, shared", [(257, LAT, False), (264, LAT, False), (272, LAT, False), (280, LAT, False), (288, LAT, False),
                                                 (320, SPLIT, True),     # 64 windows on four CUs each
                                                 (384, SPLIT, True),     # 128 windows on two CUs each
                                                 (556, SPLIT, False)])   # measured: 1 533 us shared against 1 509 as two sequences
def test_whole_rounds_plus_remainder_cases(paper, B, rem_plan, shared):
    whole = B - B % 256
    s = paper.schedule(B, 40)
    assert strip(s) == dict(nparts=2, shared_tail=shared, parts=[(0, whole, HYBRID if whole == 256 else TWOWIN), (whole, B - whole, rem_plan)])
    assert s["rnn_cluster"] == ROWS4


def test_other_window_lengths_never_split_and_never_take_a_T40_plan(paper):
    for T, plans in ((39, {8: LAT, 100: HYBRID, 300: HYBRID}), (41, {8: GENERAL, 100: GENERAL, 300: GENERAL})):
        for B, plan in plans.items():
            assert strip(paper.schedule(B, T)) == dict(nparts=1, shared_tail=False, parts=[(0, B, plan)]), (B, T)


def test_demoted_handle_takes_no_cooperating_kernel():
    h = handle(synth.PAPER)
    h.set_option(tlib.TIP_OPT_DEMOTED, 1)
    for B in B_ALL:
        s = h.schedule(B, 40)
        assert strip(s) == dict(nparts=1, shared_tail=False, parts=[(0, B, rounds(B)[0])]), B
        assert s["rnn_cluster"] == 1, B


def test_two_cus_per_window_moves_the_latency_bound_to_48():
    h = handle(synth.PAPER)
    h.set_option(tlib.TIP_OPT_F1S_PARTS, 2)
    for B in range(1, 257):
        assert h.schedule(B, 40)["parts"] == [(0, B, few_windows(B, lat_bound=48) or HYBRID)], B
    assert h.schedule(48, 40)["parts"][0][2] == LAT and h.schedule(49, 40)["parts"][0][2] == SPLIT


def test_masked_stream_never_splits(paper):
    """128 of the device's 256 CUs: the split's cost model is gated to the whole device.  Four CUs per window fit up to 32 windows, two up
    to 64; between 33 and 48 the latency plan still serves (no four-CU form to beat it).  A round is 128 windows (256 for the two-window
    encoder): 256 windows are two rounds of one against one of the other, 257 are three against two."""
    for B in B_ALL:
        assert paper.schedule(B, 40, cus=128)["nparts"] == 1, B
    for B, plan in ((32, LAT), (33, LAT), (48, LAT), (49, SPLIT), (64, SPLIT), (65, HYBRID), (128, HYBRID), (256, TWOWIN), (257, HYBRID)):
        assert paper.schedule(B, 40, cus=128)["parts"] == [(0, B, plan)], B


def test_pinned_plan_that_does_not_serve_the_shape():
    h = handle(synth.PAPER)
    for plan, B, T in ((TWOWIN, 8, 39), (SPLIT, 200, 40), (LAT, 65, 40)):
        h.set_option(tlib.TIP_OPT_PLAN, plan)
        with pytest.raises(tlib.TipStatusError) as ei:
            h.schedule(B, T)
        assert ei.value.status == tlib.TIP_ERR_UNSUPPORTED_CONFIG, (plan, B, T)
    # ... and one that does is taken as it is, for any batch, in one sequence
    for plan in (TWOWIN, HYBRID, tlib.TIP_PLAN_FUSED, GENERAL):
        h.set_option(tlib.TIP_OPT_PLAN, plan)
        for B in (8, 300, 556):
            assert strip(h.schedule(B, 40)) == dict(nparts=1, shared_tail=False, parts=[(0, B, plan)]), (plan, B)


def test_workspace_too_small_for_a_part_keeps_one_sequence(paper):
    """A caller's buffer sized by an older library: the two-sequence split carves every part from the start of the same workspace, and
    falls through to the single sequence when a part's own carve-up would not fit (tip_workspace_bytes = the carve-up + 256)."""
    need = paper.workspace_bytes(256, 40) - 256
    assert strip(paper.schedule(257, 40, workspace_bytes=need)) == expected(257) and expected(257)["nparts"] == 2
    assert strip(paper.schedule(257, 40, workspace_bytes=need - 1)) == dict(nparts=1, shared_tail=False, parts=[(0, 257, TWOWIN)])


def test_reuse_on_full_windows_is_one_sequence_on_the_two_window_encoder(paper):
    for B in (1, 100, 300, 1024):
        assert strip(paper.schedule(B, 40, reuse_full=True)) == dict(nparts=1, shared_tail=False, parts=[(0, B, TWOWIN)]), B


@pytest.mark.parametrize("cfg", [synth.TINY, synth.SCALED])
def test_other_configurations_take_the_general_plan(cfg):
    h = handle(cfg)
    for T in (40, 80):
        for B in (1, 8, 100, 300, 1000):
            assert strip(h.schedule(B, T)) == dict(nparts=1, shared_tail=False, parts=[(0, B, GENERAL)]), (B, T)


def test_bad_arguments(paper):
    for B, T in ((0, 40), (-1, 40), (8, 0)):
        with pytest.raises(tlib.TipStatusError) as ei:
            paper.schedule(B, T)
        assert ei.value.status == -1
