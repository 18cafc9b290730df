"""AUTO's plan for the paper-WIDTH family, without a GPU: the models the hand-tuned inference kernels accept (csrc/tip_fused.hip:
fused_supported — tf_in_dim 256, 16 heads, tf_hid_size 1024, at most 224 input columns, T <= 40, any depth) with the axes they leave
free moved off the paper's values: tf_layers, rnn_hid_size, with_rnn, size_s, with_acc_sum.  The rules, written out here and not read
back from the library:
  * the RNN input term rides in the encoder only at rnn_hid_size 512 (fused_has_rnn_ih): without it (another width, or no RNN) the
    two-window encoder, the window-split encoder and the few-stream plan do not serve the model, and AUTO takes ONE sequence on the
    one-window hybrid encoder at every batch;
  * with it, the schedule is the paper model's: depth and state width are NOT inputs of the cost model (its constants were measured on
    the paper model; a deeper or narrower member of the family takes the same plan at the same batch);
  * more than 224 input columns: the general plan, and every pinned fused-family plan is refused.
tests/test_paper_width_shapes_gpu.py runs the same table against the fp64 oracle."""
import pytest

from tip_amd import lib as tlib
from tip_amd import synth
from test_schedule_cpu import GENERAL, HYBRID, LAT, SPLIT, TWOWIN, expected, handle, strip

FUSED = tlib.TIP_PLAN_FUSED
KIN = 224                       # csrc/tip_fused.hip, fz::KIN: the fused encoders' in_linear K


def _cfg(**kw):
    return dict(synth.PAPER, **kw)


# id -> configuration: the one table of both files
CONFIGS = {
    "L1": _cfg(tf_layers=1), "L2": _cfg(tf_layers=2), "L7": _cfg(tf_layers=7), "L8": _cfg(tf_layers=8), "L12": _cfg(tf_layers=12),
    "R64": _cfg(rnn_hid_size=64), "R256": _cfg(rnn_hid_size=256), "R320": _cfg(rnn_hid_size=320), "R384": _cfg(rnn_hid_size=384),
    "R448": _cfg(rnn_hid_size=448),
    "noRNN": _cfg(with_rnn=False), "noRNN_L1_S111": _cfg(with_rnn=False, tf_layers=1, size_s=111),
    "S111": _cfg(size_s=111), "S127": _cfg(size_s=127), "S143": _cfg(size_s=143),
    "S143n": _cfg(size_s=143, with_acc_sum=False), "S147n": _cfg(size_s=147, with_acc_sum=False),
    "S151n": _cfg(size_s=151, with_acc_sum=False),
    "S135": _cfg(size_s=135),
}


def in_columns(cfg):
    return cfg["input_size_imu"] + (18 if cfg["with_acc_sum"] else 0) + cfg["size_s"]


def group(cfg):
    """'general': too wide for the fused encoders; 'paper': the paper model's schedule; 'hybrid': the one-window hybrid encoder only."""
    if in_columns(cfg) > KIN:
        return "general"
    return "paper" if cfg["with_rnn"] and cfg["rnn_hid_size"] == 512 else "hybrid"


GROUPS = {"general": ["S135", "S143"],
          "paper": ["L1", "L2", "L7", "L8", "L12", "S111", "S127", "S143n", "S147n", "S151n"],
          "hybrid": ["R64", "R256", "R320", "R384", "R448", "noRNN", "noRNN_L1_S111"]}
SHAPES = [(B, 40) for B in (1, 8, 33, 66, 256, 257, 300)] + [(3, 12), (100, 12)]


def test_the_table_is_what_the_issue_says():
    assert {k: in_columns(CONFIGS[k]) for k in ("S111", "S127", "S143", "S143n", "S147n", "S151n", "S135")} == \
        dict(S111=201, S127=217, S143=233, S143n=215, S147n=219, S151n=223, S135=225)
    assert sorted(sum(GROUPS.values(), [])) == sorted(CONFIGS)
    for g, names in GROUPS.items():
        for name in names:
            assert group(CONFIGS[name]) == g, name


def one(B, plan):
    return dict(nparts=1, shared_tail=False, parts=[(0, B, plan)])


def expected_short(B):
    """T < 40, RNN input term in the encoder: the few-stream plan up to its 64 windows (no window-split encoder to beat it), the hybrid
    encoder beyond; never a split (test_schedule_cpu.py: test_other_window_lengths_never_split_and_never_take_a_T40_plan)."""
    return one(B, LAT if B <= 64 else HYBRID)


def refused(h, plan, B, T, parts=0):
    h.set_option(tlib.TIP_OPT_F1S_PARTS, parts)
    h.set_option(tlib.TIP_OPT_PLAN, plan)
    try:
        with pytest.raises(tlib.TipStatusError) as ei:
            h.schedule(B, T)
        return ei.value.status == tlib.TIP_ERR_UNSUPPORTED_CONFIG
    finally:
        h.set_option(tlib.TIP_OPT_PLAN, tlib.TIP_PLAN_AUTO)
        h.set_option(tlib.TIP_OPT_F1S_PARTS, 0)


@pytest.mark.parametrize("name", GROUPS["hybrid"])
def test_without_the_rnn_input_term_auto_takes_the_hybrid_encoder(name):
    cfg = CONFIGS[name]
    h = handle(cfg)
    for B, T in SHAPES:
        s = h.schedule(B, T)
        assert strip(s) == one(B, HYBRID), (name, B, T)
        # the 16-window recurrence kernels (the four-window tiles are rnn_hid_size 512's): 16 workgroups per tile while they fit the CUs
        if cfg["with_rnn"]:
            assert s["rnn_cluster"] == max(c for c in (1, 2, 4, 8, 16) if c == 1 or -(-B // 16) * c <= 256), (name, B, T)
        for plan, parts in ((TWOWIN, 0), (SPLIT, 0), (SPLIT, 2), (SPLIT, 4), (LAT, 0)):
            assert refused(h, plan, B, T, parts), (name, plan, parts, B, T)
    for plan in (FUSED, HYBRID, GENERAL):              # ... and the plans that serve the model are taken as pinned
        h.set_option(tlib.TIP_OPT_PLAN, plan)
        for B, T in SHAPES:
            assert strip(h.schedule(B, T)) == one(B, plan), (name, plan, B, T)


@pytest.mark.parametrize("name", GROUPS["paper"])
def test_depth_and_state_width_are_not_inputs_of_the_cost_model(name):
    """rnn_hid_size 512 at any tf_layers and any size_s with at most 224 input columns: the paper model's table, entry for entry
    (expected(B) of tests/test_schedule_cpu.py at T = 40).  The cost model's microseconds were measured at four layers; a model of
    another depth scales every encoder alike, and the schedule does not look at tf_layers or size_s at all."""
    cfg = CONFIGS[name]
    h, paper = handle(cfg), handle(synth.PAPER)
    for B, T in SHAPES:
        want = expected(B) if T == 40 else expected_short(B)
        s = h.schedule(B, T)
        assert strip(s) == want, (name, B, T)
        assert s == paper.schedule(B, T), (name, B, T)
        assert s["rnn_cluster"] == tlib.TIP_RNN_CLUSTER_ROWS4
    # what the table says at these batches, spelt out once (so that a change of expected() itself shows here)
    assert [expected(B)["parts"] for B in (1, 8, 33, 66, 256)] == [[(0, 1, LAT)], [(0, 8, LAT)], [(0, 33, SPLIT)], [(0, 66, SPLIT)], [(0, 256, HYBRID)]]
    assert expected(257) == dict(nparts=2, shared_tail=False, parts=[(0, 256, HYBRID), (256, 1, LAT)])
    assert expected(300) == dict(nparts=2, shared_tail=True, parts=[(0, 256, HYBRID), (256, 44, SPLIT)])
    # pinned plans: each serves the shapes it serves on the paper model, and is refused where it is there
    assert refused(h, TWOWIN, 3, 12) and refused(h, SPLIT, 3, 12) and refused(h, SPLIT, 256, 40) and refused(h, SPLIT, 66, 40, parts=4)
    assert refused(h, LAT, 66, 40) and refused(h, LAT, 100, 12)
    for plan, B, T in ((TWOWIN, 5, 40), (SPLIT, 66, 40), (LAT, 3, 40), (LAT, 3, 12), (FUSED, 7, 12), (HYBRID, 7, 40), (GENERAL, 5, 40)):
        h.set_option(tlib.TIP_OPT_PLAN, plan)
        assert strip(h.schedule(B, T)) == one(B, plan), (name, plan, B, T)


@pytest.mark.parametrize("name", GROUPS["general"])
def test_more_than_224_input_columns_take_the_general_plan(name):
    cfg = CONFIGS[name]
    assert in_columns(cfg) > KIN
    h = handle(cfg)
    for B, T in SHAPES:
        assert strip(h.schedule(B, T)) == one(B, GENERAL), (name, B, T)
        for plan, parts in ((FUSED, 0), (HYBRID, 0), (TWOWIN, 0), (SPLIT, 0), (SPLIT, 2), (SPLIT, 4), (LAT, 0)):
            assert refused(h, plan, B, T, parts), (name, plan, parts, B, T)
    h.set_option(tlib.TIP_OPT_PLAN, GENERAL)
    assert strip(h.schedule(7, 40)) == one(7, GENERAL)


def test_the_input_width_edge_is_between_224_and_225_columns():
    """In = 223 (S151n) and 224 are inside, 225 (S135) is outside: size_s 152 without acc-sum is exactly KIN."""
    assert in_columns(CONFIGS["S151n"]) == KIN - 1 and in_columns(CONFIGS["S135"]) == KIN + 1
    at = handle(_cfg(size_s=152, with_acc_sum=False))
    assert strip(at.schedule(8, 40)) == expected(8) and strip(at.schedule(300, 40)) == expected(300)
    assert strip(handle(CONFIGS["S135"]).schedule(8, 40)) == one(8, GENERAL)
