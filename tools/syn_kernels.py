"""Kernel times of tip_amd.syndata (csrc/tip_syn.hip), each launch on its own: the three chain launches of the SBP search cannot be
told apart by events around the one call, so this traces them.

    python tools/syn_kernels.py [--out FILE]    -> one JSON line per kernel; FILE (default: the record, profiles/syn/syn_kernels.txt)

It starts `rocprofv3 --kernel-trace --stats -- python tools/syn_bench.py --once` as a child process (64 sequences x 3000 frames,
synthesize() three times; tracing slows the host, not the kernels), reads the trace's kernel table and prints per kernel the number
of launches and the average / min / max duration.  For the chain kernels it adds the cost of ONE frame of ONE chain: every chain of a
launch runs side by side on its own workgroup (64 or 128 workgroups on 256 CUs), so that is the kernel's duration over the 2996
searched frames of a sequence.  `<64, 2>` is the one-wave wrist chain, which has no barrier; `<256, 7>` (feet) and `<256, 25>` (pelvis)
are four waves with one barrier per frame and 7 / 25 candidate points per lane."""
import glob
import json
import os
import re
import sqlite3
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 3000


def main():
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "syn", "syn_kernels.txt")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "syn", "--", sys.executable, os.path.join(ROOT, "tools", "syn_bench.py"),
               "--once", "--frames", str(FRAMES)]
        res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        if res.returncode != 0:
            print(res.stdout[-3000:])
            raise SystemExit(f"rocprofv3 ended with {res.returncode}")
        dbs = glob.glob(os.path.join(tmp, "**", "*.db"), recursive=True)
        if not dbs:
            raise SystemExit("no trace database under " + tmp)
        con = sqlite3.connect(dbs[0])
        rows = con.execute("select name, count(*), avg(end - start), min(end - start), max(end - start), max(workgroup_x), max(grid_x) "
                           "from kernels where name like '%syn_%' group by name order by name").fetchall()
    for name, n, avg, lo, hi, wg, grid in rows:
        short = re.sub(r"\(.*", "", name).replace("void ", "").replace("tip::", "")
        d = {"kernel": short, "launches": n, "workgroups": grid // wg, "threads": wg, "us_avg": round(avg / 1e3, 1), "us_min": round(lo / 1e3, 1),
             "us_max": round(hi / 1e3, 1)}
        if "syn_sbp_kernel" in short:
            d["us_per_frame_of_one_chain"] = round(avg / 1e3 / (FRAMES - 4), 3)
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    if len(lines) < 6:
        raise SystemExit("the trace does not hold the six syn kernels")
    with open(out_path, "w") as f:
        f.write(f"# tools/syn_kernels.py on one MI355X: rocprofv3 --kernel-trace of synthesize() on 64 sequences x {FRAMES} frames, three calls;\n"
                "# per kernel the launches' durations; per chain kernel the duration over the 2996 searched frames = one frame of one chain\n")
        f.write("\n".join(lines) + "\nok\n")
    print("ok")


if __name__ == "__main__":
    main()
