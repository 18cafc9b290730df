#!/usr/bin/env python3
"""Pinned bytes of the packed weight image (csrc/tip_pack.hip): byte length and SHA-256 of pack_host() per configuration.

The digests were made by the HOST PACKER OF THE COMMIT NAMED IN THE JSON FILE — the hand-written loops that preceded the
one-description packer — never by the code they are now compared with (tests/test_host_cpu.py).  To regenerate after a
deliberate layout change, build libtip_hip.so from a commit whose image is known good and select it by path:

usage: TIP_LIB=/path/to/libtip_hip.so python tests/golden/make_packed_digest.py <commit that built the library>

CPU only.  Data only: names, sizes, digests.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, "tip_packed_digest.json")
SEED = 3


def configs():
    from tip_amd import synth
    P = synth.PAPER
    return {
        "paper": P,                                          # fused section with the RNN input rider
        "no_acc_sum": dict(P, with_acc_sum=False),           # In < 224: padded in-linear columns
        "size_s_119": dict(P, size_s=119),                   # two stationary body points
        "no_rnn": dict(P, with_rnn=False),                   # fused section without the rider; out-linear from d_model
        "tiny": synth.TINY,                                  # d_head 32: q-scale not folded
        "train_default": synth.TRAIN_DEFAULT,                # 8 heads: no fused section
        "scaled2": dict(synth.SCALED, tf_layers=2),          # d_head 64, folded; panel-GEMM fragment sections
    }


def image_digest(cfg):
    """(byte length, SHA-256) of pack_host() of the CPU model carrying synth.make_weights(cfg, seed=SEED)."""
    import torch
    import tip_amd
    from tip_amd import synth
    m = tip_amd.TF_RNN_Past_State(
        cfg["input_size_imu"], cfg["size_s"], rnn_hid_size=cfg["rnn_hid_size"], tf_hid_size=cfg["tf_hid_size"],
        tf_in_dim=cfg["tf_in_dim"], n_heads=cfg["n_heads"], tf_layers=cfg["tf_layers"], dropout=0.0, in_dropout=0.0,
        past_state_dropout=0.0, with_rnn=cfg.get("with_rnn", True), with_acc_sum=cfg.get("with_acc_sum", False))
    m.load_state_dict({k: torch.tensor(v) for k, v in synth.make_weights(cfg, seed=SEED).items()})
    img = m.pack_host().numpy()
    return int(img.nbytes), hashlib.sha256(img.tobytes()).hexdigest()


def main():
    from tip_amd import lib as tlib
    out = {"made_by": "tip_pack_weights (host) of commit " + (sys.argv[1] if len(sys.argv) > 1 else "UNKNOWN"),
           "weights": "synth.make_weights(cfg, seed=%d)" % SEED, "images": {}}
    for name, cfg in configs().items():
        nbytes, sha = image_digest(cfg)
        out["images"][name] = {"bytes": nbytes, "sha256": sha}
        print(name, nbytes, sha)
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", PATH, "with", tlib.LIB_PATH)


if __name__ == "__main__":
    main()
