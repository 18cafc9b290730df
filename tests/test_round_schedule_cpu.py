"""The one-launch round in the schedule, without a GPU (csrc/tip_schedule.hip through tip_debug_schedule's tenth word; a handle made
without a device reports 256 CUs).  The rule, written out here and not read back from the library: a batch runs as ONE launch exactly
when TIP_OPT_NO_ROUND_LAUNCH is 0, the handle is not demoted, the whole batch is ONE launch sequence on the one-window hybrid encoder
(chosen by AUTO or pinned) with the four-window recurrence (rnn_hid_size 512, TIP_OPT_RNN_CLUSTER 0 or its ROWS4 value), the state
width is 129..131, T <= 40 and the batch is at most one window per CU — the grid, whole rounds of 32 workgroups, has to fit the device.
Everything tests/test_paper_width_schedule_cpu.py and tests/test_schedule_cpu.py pin (plans, parts, cluster) does not depend on the
option."""
import pytest

from tip_amd import lib as tlib
from tip_amd import synth
from test_schedule_cpu import HYBRID, TWOWIN, GENERAL, LAT, SPLIT, expected, handle, strip

CUS = 256
SHAPES = [(B, T) for B in (1, 3, 4, 5, 31, 32, 33, 36, 64, 65, 128, 129, 255, 256, 257, 300, 512) for T in (1, 2, 33, 40)]


def rule(cfg, B, T, plan, no_round, demoted, cluster=0):
    if no_round or demoted or plan != HYBRID or cluster not in (0, tlib.TIP_RNN_CLUSTER_ROWS4):
        return False
    if not (cfg.get("with_rnn", True) and cfg["rnn_hid_size"] == 512 and 129 <= cfg["size_s"] <= 131):
        return False
    tiles = (B + 3) // 4
    grid = (tiles + 7) // 8 * 32                    # clusters of 4 workgroups, in rounds of 8 clusters
    return T <= 40 and grid <= CUS


def test_default_is_the_one_launch_form_and_the_option_takes_it_away():
    """AUTO takes the form by default (CHANGELOG.md: its slowest run beat the three launches' fastest); TIP_OPT_NO_ROUND_LAUNCH = 1 is the
    three launches everywhere."""
    h = handle(synth.PAPER)
    assert h.get_option(tlib.TIP_OPT_NO_ROUND_LAUNCH) == 0
    assert h.round_launch(256, 40) and h.round_launch(200, 33) and not h.round_launch(100, 40) and not h.round_launch(257, 40)
    h.set_option(tlib.TIP_OPT_NO_ROUND_LAUNCH, 1)
    for plan in (tlib.TIP_PLAN_AUTO, HYBRID):
        h.set_option(tlib.TIP_OPT_PLAN, plan)
        assert not any(h.round_launch(B, T) for B, T in SHAPES)
    with pytest.raises(tlib.TipStatusError):
        h.set_option(tlib.TIP_OPT_NO_ROUND_LAUNCH, 2)


@pytest.mark.parametrize("size_s", [131, 130, 129])
def test_which_batches_take_the_form(size_s):
    cfg = dict(synth.PAPER, size_s=size_s)
    h = handle(cfg)
    for no_round in (0, 1):
        h.set_option(tlib.TIP_OPT_NO_ROUND_LAUNCH, no_round)
        for demoted in (0, 1):
            h.set_option(tlib.TIP_OPT_DEMOTED, demoted)
            for pinned in (tlib.TIP_PLAN_AUTO, HYBRID, TWOWIN, GENERAL, tlib.TIP_PLAN_FUSED):
                h.set_option(tlib.TIP_OPT_PLAN, pinned)
                for B, T in SHAPES:
                    try:
                        s = h.schedule(B, T)
                    except tlib.TipStatusError:            # a pinned plan that does not serve the shape
                        continue
                    plan = s["parts"][0][2] if s["nparts"] == 1 else None
                    want = rule(cfg, B, T, plan, no_round, demoted)
                    assert h.round_launch(B, T) == want, (size_s, no_round, demoted, pinned, B, T, s)
    # AUTO on the paper model: one round of up to 256 windows on the hybrid encoder is B = 129 .. 256 at T = 40 (below, the
    # few-window plans; above, more than one round) and 65 .. 256 at other window lengths
    h.set_option(tlib.TIP_OPT_NO_ROUND_LAUNCH, 0)
    h.set_option(tlib.TIP_OPT_DEMOTED, 0)
    h.set_option(tlib.TIP_OPT_PLAN, tlib.TIP_PLAN_AUTO)
    assert [B for B in range(1, 600) if h.round_launch(B, 40)] == list(range(129, 257))
    assert [B for B in range(1, 600) if h.round_launch(B, 33)] == list(range(65, 257))
    h.set_option(tlib.TIP_OPT_PLAN, HYBRID)
    assert [B for B in range(1, 600) if h.round_launch(B, 40)] == list(range(1, 257))


def test_an_explicit_16_window_recurrence_keeps_the_three_launches():
    h = handle(synth.PAPER)
    h.set_option(tlib.TIP_OPT_NO_ROUND_LAUNCH, 0)
    h.set_option(tlib.TIP_OPT_PLAN, HYBRID)
    for cluster in (1, 2, 4, 8, 16):
        h.set_option(tlib.TIP_OPT_RNN_CLUSTER, cluster)
        assert not h.round_launch(36, 40) and not h.round_launch(256, 40)
    h.set_option(tlib.TIP_OPT_RNN_CLUSTER, tlib.TIP_RNN_CLUSTER_ROWS4)
    assert h.round_launch(36, 40) and h.round_launch(256, 40)


@pytest.mark.parametrize("name,cfg", [("R256", dict(synth.PAPER, rnn_hid_size=256)), ("noRNN", dict(synth.PAPER, with_rnn=False)),
                                      ("S127", dict(synth.PAPER, size_s=127)), ("S143n", dict(synth.PAPER, size_s=143, with_acc_sum=False)),
                                      ("S135", dict(synth.PAPER, size_s=135))])
def test_other_widths_never_take_the_form(name, cfg):
    h = handle(cfg)
    h.set_option(tlib.TIP_OPT_NO_ROUND_LAUNCH, 0)
    for pinned in (tlib.TIP_PLAN_AUTO, HYBRID):
        h.set_option(tlib.TIP_OPT_PLAN, pinned)
        for B, T in SHAPES:
            try:
                assert not h.round_launch(B, T), (name, pinned, B, T)
            except tlib.TipStatusError:
                pass


def test_a_masked_stream_keeps_the_three_launches():
    """Fewer CUs than the device has (a stream with a CU mask): the grid is sized for the whole device."""
    h = handle(synth.PAPER)
    h.set_option(tlib.TIP_OPT_NO_ROUND_LAUNCH, 0)
    h.set_option(tlib.TIP_OPT_PLAN, HYBRID)
    assert h.round_launch(36, 40) and h.round_launch(36, 40, cus=256)
    assert not h.round_launch(36, 40, cus=128) and not h.round_launch(36, 40, cus=255)


def test_the_option_changes_nothing_the_schedule_tables_pin():
    """Plans, parts, shared tail and recurrence cluster at every batch of the paper table, with the form allowed and not."""
    h = handle(synth.PAPER)
    tables = []
    for no_round in (1, 0):
        h.set_option(tlib.TIP_OPT_NO_ROUND_LAUNCH, no_round)
        tables.append([h.schedule(B, T) for B in list(range(1, 700)) + [1000, 2100] for T in (40, 12)])
    assert tables[0] == tables[1]
    for B in (1, 8, 33, 66, 256, 257, 300):
        assert strip(h.schedule(B, 40)) == expected(B)
    assert [expected(B)["parts"] for B in (1, 8, 33, 66, 256)] == [[(0, 1, LAT)], [(0, 8, LAT)], [(0, 33, SPLIT)], [(0, 66, SPLIT)], [(0, 256, HYBRID)]]
