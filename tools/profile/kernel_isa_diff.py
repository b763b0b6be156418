#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?  Compares two sets of `hipcc -S` listings kernel by kernel
(paired by mangled name, whichever file of a set holds it): the instruction text and the amdhsa register / spill / LDS figures.
    hipcc <COMMON + DEVICE flags of jpezy_amd/_build.py> -S --cuda-device-only -fuse-cuid=none x.hip -o before/x.s    (each kernel file)
    python tools/profile/kernel_isa_diff.py before/ after/        (directories of *.s, or single listings)
Without -fuse-cuid=none two builds of one source already differ in a symbol.  Comments, the numbering of block labels, whitespace
and the mangled names of the __constant__ tables (c_cos, c_zzinv, ...: their linkage may differ) do not count as differences.
Prints one line per kernel; exit status 1 on any difference or any kernel found on one side only."""
import re
import sys
from pathlib import Path

FIGURES = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"]


def normal(line):
    line = line.split(";")[0]
    line = re.sub(r"\.LBB\d+_", ".LBB_", line)
    line = re.sub(r"_ZN\w*?\d+(c_[a-z0-9_]+)E\b", r"\1", line)
    return " ".join(line.split())


def kernels(path):
    """{mangled name: (instruction lines, figures)} of every listing under path"""
    out = {}
    for f in sorted(path.glob("*.s")) if path.is_dir() else [path]:
        txt = f.read_text()
        meta = {re.search(r"\.name:\s+(\S+)", b).group(1): b for b in txt.split("  - .agpr_count:")[1:]}
        for name, blk in meta.items():
            body = txt.split("\n" + name + ":", 1)[1].split(".amdhsa_kernel " + name, 1)[0]
            code = [n for n in map(normal, body.splitlines()) if n]
            figs = [int(re.search(r"\." + k + r":\s+(\d+)", "  - .agpr_count:" + blk).group(1)) for k in FIGURES]
            if name in out:
                sys.exit(f"{name}: in two listings of {path}")
            out[name] = (code, figs)
    return out


a, b = kernels(Path(sys.argv[1])), kernels(Path(sys.argv[2]))
bad = 0
for name in sorted(a.keys() | b.keys()):
    if name not in a or name not in b:
        verdict = "MISSING in " + (sys.argv[1] if name not in a else sys.argv[2])
    else:
        (ca, fa), (cb, fb) = a[name], b[name]
        what = [f"{k} {x} -> {y}" for k, x, y in zip(FIGURES, fa, fb) if x != y]
        if ca != cb:
            first = next((i for i, (x, y) in enumerate(zip(ca, cb)) if x != y), min(len(ca), len(cb)))
            what.insert(0, f"instructions {len(ca)} -> {len(cb)} lines, first difference at line {first}")
        verdict = "DIFFERS: " + "; ".join(what) if what else f"identical  {len(ca):6d} lines  vgpr {fa[0]:3d} sgpr {fa[2]:3d} spill {fa[3]} scratch {fa[5]} lds {fa[6]}"
    bad += not verdict.startswith("identical")
    print(f"{name}  {verdict}")
print(f"{len(a)} kernels before, {len(b)} after, {bad} not identical")
sys.exit(1 if bad else 0)
