#!/usr/bin/env python3
"""Host side of the optimised writer, on the CPU alone: write_jpeg(optimize=True) against write_jpeg(optimize=False) on one small
coefficient field -- the difference is the symbol histogram, jpezy_host::optimal_table (four tables) and the code tables built from them.

optimal_table's cost is its search loops (Figure K.1), and where they fall relative to a 64-byte line has moved this figure by 20 % with
unchanged instructions when code in front of the function grew (Measurements); the function is therefore aligned to 64
bytes.  This probe makes that claim re-checkable: run it on two checkouts (--root) alternately.  No GPU is used.  Nothing here is an
acceptance bound.

    python tools/measure/measure_optimal_table.py [--root DIR] [--size 64x32] [--rounds 7] [--calls 1000]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[2]))
    ap.add_argument("--size", default="64x32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=1000)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    import jpezy_amd as J
    J.load_library()
    W, H = (int(v) for v in args.size.split("x"))
    rng = np.random.default_rng(1)
    n = J.coeff_count(W, H)
    co = (rng.integers(-30, 31, n) * (rng.random(n) < 0.2)).astype(np.int16)
    print(f"measure_optimal_table: {W}x{H}, {args.rounds} rounds of {args.calls} calls, library {J.library_path()}")
    for optimize in (True, False):
        for _ in range(200):
            J.write_jpeg(co, W, H, optimize=optimize)
        t = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                J.write_jpeg(co, W, H, optimize=optimize)
            t.append((time.perf_counter() - t0) * 1e6 / args.calls)
        print(f"  optimize={optimize!s:5s}  us per call: min {min(t):7.1f}  median {sorted(t)[len(t) // 2]:7.1f}  max {max(t):7.1f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
