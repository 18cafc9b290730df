#!/usr/bin/env python3
"""Measurement only: where every workgroup of the one-launch round (csrc/tip_round.hip) is at the end of its three phases, from
s_memrealtime stamps (100 MHz, device-wide), and on which XCD it ran.
usage: TIP_FUSEDH_TRACE=1 python tools/round_trace.py [B]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np, torch
os.environ.setdefault("TIP_LIB", "measure")   # the launchers' TIP_* switches exist in the measurement build only (csrc: make measure)
from tip_amd import synth, lib as tlib
from sweep import model_for
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
m = model_for(synth.PAPER)
m.set_plan("fusedh")
m._ensure_handle().set_option(tlib.TIP_OPT_NO_ROUND_LAUNCH, 0)
x_imu, x_s = synth.make_inputs(synth.PAPER, min(B, 64), 40)
reps = (B + 63) // 64
xi = torch.tensor(np.tile(x_imu, (reps, 1, 1))[:B]).cuda(); xs = torch.tensor(np.tile(x_s, (reps, 1, 1))[:B]).cuda()
assert m._ensure_handle().round_launch(B, 40), "this batch does not take the one-launch round"
with torch.no_grad():
    for _ in range(5):
        m(xi, xs)
    torch.cuda.synchronize()
buf = (ctypes.c_ulonglong * (2048 + 5 * 1024))()
assert tlib.load().tip_debug_read_fh_wg(buf, 2048 + 5 * 1024) == 0
t = np.array(buf[2048:], dtype=np.float64)
n = ((B + 3) // 4 + 7) // 8 * 32
st = t[:4 * n].reshape(n, 4) / 100.0           # us: entry, encoder published, recurrence done, exit
xcc = t[4096:4096 + n].astype(int)
t0 = st[:, 0].min()
st -= t0
real = np.arange(n) < B
names = ("entry", "encoder published", "recurrence done", "exit")
print(f"B = {B}: {n} workgroups, first entry -> last exit {st[:, 3].max():.1f} us")
for k, name in enumerate(names):
    v = st[real, k]
    print(f"  {name:18s} min {v.min():7.1f}  median {np.median(v):7.1f}  max {v.max():7.1f} us")
print("  per XCD (median / max, us):  encoder published | recurrence done | exit")
for x in sorted(set(xcc.tolist())):
    sel = real & (xcc == x)
    if sel.any():
        print(f"    XCD {x}: {np.median(st[sel, 1]):7.1f} / {st[sel, 1].max():7.1f} | {np.median(st[sel, 2]):7.1f} / {st[sel, 2].max():7.1f} | "
              f"{np.median(st[sel, 3]):7.1f} / {st[sel, 3].max():7.1f}   ({int(sel.sum())} workgroups)")
order = np.argsort(-st[:, 3])[:6]
print("  last workgroups out (id, XCD, encoder published, recurrence done, exit):",
      [(int(i), int(xcc[i]), round(float(st[i, 1]), 1), round(float(st[i, 2]), 1), round(float(st[i, 3]), 1)) for i in order])
