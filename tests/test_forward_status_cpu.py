"""What the five forward entry points answer to arguments they refuse, without a GPU: tip_forward, tip_forward_rows, tip_forward_reuse,
tip_forward_dropout and tip_forward_live on one handle of the paper configuration, before and after a packed image is attached.  The
image is a fake 256-aligned host address that tip_attach_packed only stores.  Every row holds at least one invalid argument or B = 0,
so every call returns before the first HIP call — none may pass all checks: on a machine with a GPU it would launch on that address.

The table is the library's as it stood when the entry points still restated their checks one by one, with one row edited since:
tip_forward_dropout lacked the 32-bit bound and answered a 20000-window batch on a handle without an image with NOT_READY; it now
answers UNSUPPORTED_CONFIG like the others (the shared preamble, csrc/tip_abi.hip: forward_prepare)."""
import pytest

from tip_amd import lib as tlib
from tip_amd import synth

OK, INVALID, UNSUPPORTED, NOT_READY, WORKSPACE = 0, -1, -2, -3, -4
PTR = 0x7F00_0000_0000            # 256-aligned, never dereferenced
HUGE = 1 << 40
N = None                          # a null pointer

# what a row changes in an otherwise valid call (B = 1, T = 40, no flags, a large aligned workspace)
COMMON = [
    ("null_x_imu", dict(x_imu=N), INVALID, INVALID),
    ("B_minus_1", dict(B=-1), INVALID, INVALID),
    ("T_0", dict(T=0), INVALID, INVALID),
    ("mask_flag_no_mask", dict(flags=tlib.TIP_FWD_KEEP_MASK), INVALID, INVALID),
    ("B_20000_T_40", dict(B=20000), UNSUPPORTED, UNSUPPORTED),
    ("B_0", dict(B=0), NOT_READY, OK),
    ("workspace_null", dict(ws=N), NOT_READY, WORKSPACE),
    ("workspace_misaligned", dict(ws=PTR + 4), NOT_READY, WORKSPACE),
    ("workspace_16_bytes", dict(ws_bytes=16), NOT_READY, WORKSPACE),
]
DROPOUT = [
    ("p_drop_1", dict(p_drop=1.0), INVALID, INVALID),
    ("p_drop_negative", dict(p_drop=-0.1), INVALID, INVALID),
    ("p_state_1_5", dict(p_state=1.5), INVALID, INVALID),
]
ROWS = {
    "tip_forward": COMMON,
    "tip_forward_rows": COMMON + [("null_rows", dict(rows=N), INVALID, INVALID)],
    "tip_forward_reuse": COMMON + [("T_41", dict(T=41), UNSUPPORTED, UNSUPPORTED), ("frame_idx_38", dict(frame_idx=38), INVALID, INVALID)],
    "tip_forward_dropout": COMMON + DROPOUT,
    "tip_forward_live": COMMON + DROPOUT,
}


def call(lib, h, entry, x_imu=PTR, x_s=PTR, y=PTR, B=1, T=40, flags=0, ws=PTR, ws_bytes=HUGE, rows=PTR, frame_idx=39, p_drop=0.1,
         p_state=0.0):
    tail = (ws, ws_bytes, None)
    if entry == "tip_forward":
        return lib.tip_forward(h, x_imu, x_s, y, B, T, flags, None, 1.0, *tail)
    if entry == "tip_forward_rows":
        return lib.tip_forward_rows(h, x_imu, x_s, y, B, T, rows, flags, None, 1.0, *tail)
    if entry == "tip_forward_reuse":
        return lib.tip_forward_reuse(h, x_imu, x_s, y, B, T, flags, PTR, HUGE, frame_idx, None, *tail)
    if entry == "tip_forward_dropout":
        return lib.tip_forward_dropout(h, x_imu, x_s, y, B, T, flags, None, 1.0, p_state, 7, p_drop, 11, *tail)
    return lib.tip_forward_live(h, x_imu, x_s, y, B, T, None, flags, None, 1.0, p_state, 7, p_drop, 11, None, *tail)


@pytest.fixture(scope="module")
def table():
    """{(entry, row, attached): status}: every row on the handle without an image, then the image attached, then every row again."""
    cfg = synth.PAPER
    handle = tlib.Handle(tlib.TipConfig(cfg["input_size_imu"], cfg["size_s"], cfg["rnn_hid_size"], cfg["tf_hid_size"], cfg["tf_in_dim"],
                                        cfg["n_heads"], cfg["tf_layers"], 1, 1 if cfg.get("with_acc_sum", False) else 0, 40))
    got = {}
    for attached in (False, True):
        if attached:
            handle.attach_packed(PTR, handle.packed_bytes())
        for entry, rows in ROWS.items():
            for name, change, _, _ in rows:
                got[entry, name, attached] = call(handle.lib, handle._h, entry, **change)
    assert handle.forward_count() == 0
    return got


@pytest.mark.parametrize("attached", [False, True], ids=["not_ready", "attached"])
@pytest.mark.parametrize("entry", list(ROWS))
def test_forward_status(table, entry, attached):
    got = [(name, table[entry, name, attached]) for name, _, _, _ in ROWS[entry]]
    print(entry, "attached" if attached else "not ready", got)
    assert got == [(name, at if attached else nr) for name, _, nr, at in ROWS[entry]]
