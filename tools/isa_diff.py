#!/usr/bin/env python3
"""Which kernels differ between two builds' device assembly?  Compares TEXT per kernel symbol; it looks for no instruction.

Make the assembly with the Makefile's CXXFLAGS plus `--cuda-device-only -S` (one .s per csrc/*.hip), once per tree, then
  python tools/isa_diff.py OLD NEW            (two .s files, or two directories holding same-named .s files)
Per kernel (a symbol with an .amdhsa_kernel block) the function body and the descriptor block are hashed after stripping comments,
trailing blanks and the function index inside local labels (.LBB<n>_<m>, .Lfunc_end<n>: they move when a neighbour leaves).
Prints per file the symbol counts and the removed / added / changed symbols; exit status 1 when any kernel changed or was added.
The kin, terrain and stream kernels were compared this way by hand; this is that comparison, kept."""
import hashlib
import os
import re
import sys

LABEL = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin)\d+")


def kernels(path):
    """{symbol: digest of its normalised body + descriptor}"""
    lines = [LABEL.sub(r".\1", ln.split(";")[0].rstrip()) for ln in open(path, errors="replace")]
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        body = lines[lines.index(name + ":"):]
        body = body[:next(i for i, ln in enumerate(body) if ln.startswith(".Lfunc_end")) + 1]
        desc = lines[lines.index("\t.amdhsa_kernel " + name):]
        desc = desc[:desc.index("\t.end_amdhsa_kernel") + 1]
        out[name] = hashlib.sha256("\n".join(ln for ln in body + desc if ln.strip()).encode()).hexdigest()
    return out


def main(old, new):
    if os.path.isdir(old):
        files = sorted(set(f for d in (old, new) for f in os.listdir(d) if f.endswith(".s")))
        pairs = [(f, os.path.join(old, f), os.path.join(new, f)) for f in files]
    else:
        pairs = [(os.path.basename(new), old, new)]
    bad = 0
    for label, a, b in pairs:
        ka = kernels(a) if os.path.exists(a) else {}
        kb = kernels(b) if os.path.exists(b) else {}
        removed, added = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
        changed = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
        print(f"{label}: {len(ka)} -> {len(kb)} kernels, {len(removed)} removed, {len(added)} added, {len(changed)} changed")
        for tag, syms in (("removed", removed), ("added", added), ("changed", changed)):
            for k in syms:
                print(f"  {tag:8s}{k}")
        bad += len(added) + len(changed)
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
