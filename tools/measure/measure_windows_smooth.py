#!/usr/bin/env python3
"""What smooth chroma upsampling costs in the window batches: jpezy_decode_windows_dev and jpezy_decode_windows_resized_dev with
jpezy_ctx_set_windows_upsampling at JPEZY_UPSAMPLE_NEAREST (the unchanged kernels of the same build) and at JPEZY_UPSAMPLE_SMOOTH, on the
same files, in one process, the arms alternated round by round after a warm-up of each.  A host clock around work that ends in a device
synchronise; median, minimum and maximum per arm, and whether B - A exceeds the larger spread of the two.

  Workloads   mixed      N own-layout files (measure_windows.py's: widths 320..800, heights 240..600, one window of 224..448 px, scale 1)
              one size   N files of 1920 x 1080 (--distinct different pictures, repeated), a 224 x 224 window each
              resized    measure_windows_resized.py's mixed workload: random-resized-crop sources through resize_pick_window to 224 x 224
  Arms        A  nearest
              B  smooth
              C  one 4096 x 4096 own-layout file and a 224 x 224 window on resident coefficients: dequant_idct_upsampling_packed_dev of the
                 whole picture followed by a device slice (C1), against dequant_idct_region_dev(..., upsampling=UPSAMPLE_SMOOTH) (C2)
  Also        the JPEZY_BATCH_DEBUG laps of one call of A and of B per workload on stderr (the kernel's own time from device events).
  --trace     no timing: three calls of every arm and nothing else, for a run under a kernel tracer of its own.

--check compares B's bytes with a loop of decode_jpeg_region_packed(..., upsampling=UPSAMPLE_SMOOTH) first.  Prints one line per arm and a
JSON line with every figure (times in milliseconds)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpezy_amd as J  # noqa: E402
from jpezy_amd import api  # noqa: E402
from measure_windows import Workload, encode  # noqa: E402
from measure_windows_resized import OUT, Workload as ResizedWorkload  # noqa: E402


def batch_arms(lib, ctx, wl, dev):
    n, Hs, Ws = wl.n, wl.Hs, wl.Ws
    row, slot = Ws * 3, Hs * Ws * 3
    d = {m: torch.zeros((n, Hs, Ws, 3), dtype=torch.uint8, device=dev) for m in (J.UPSAMPLE_NEAREST, J.UPSAMPLE_SMOOTH)}

    def arm(mode):
        def fn():
            assert lib.jpezy_ctx_set_windows_upsampling(ctx._h, mode) == 0
            rc = lib.jpezy_decode_windows_dev(ctx._h, n, wl.data, wl.lens, 0, wl.cwins, J.PIX_RGB24, row, slot, d[mode].data_ptr(), n * slot, wl.infos, wl.placed,
                                              wl.status)
            assert rc == 0, lib.jpezy_hip_last_error()
        return fn

    return {"A nearest": arm(J.UPSAMPLE_NEAREST), "B smooth": arm(J.UPSAMPLE_SMOOTH)}, d


def resized_arms(lib, ctx, wl, dev):
    n = wl.n
    d = {m: torch.zeros((n, OUT, OUT, 3), dtype=torch.uint8, device=dev) for m in (J.UPSAMPLE_NEAREST, J.UPSAMPLE_SMOOTH)}

    def arm(mode):
        def fn():
            assert lib.jpezy_ctx_set_windows_upsampling(ctx._h, mode) == 0
            rc = lib.jpezy_decode_windows_resized_dev(ctx._h, n, wl.data, wl.lens, 0, wl.cwins, wl.mirror, OUT, OUT, J.PIX_RGB24, 0, 0, d[mode].data_ptr(),
                                                      n * OUT * OUT * 3, wl.infos, wl.placed, wl.status)
            assert rc == 0, lib.jpezy_hip_last_error()
        return fn

    return {"A nearest": arm(J.UPSAMPLE_NEAREST), "B smooth": arm(J.UPSAMPLE_SMOOTH)}, d


def single_file_arms(ctx, edge, dev):
    f = encode(ctx, edge, edge, 77)
    info, d_co = ctx.read_jpeg_gpu(f)
    whole = torch.zeros((edge, edge, 3), dtype=torch.uint8, device=dev)
    crop = {k: torch.zeros((224, 224, 3), dtype=torch.uint8, device=dev) for k in (1, 2)}
    x, y = edge // 2 - 101, edge // 2 - 75

    def c1():
        ctx.dequant_idct_upsampling_dev(d_co, info, d_img=whole, upsampling=J.UPSAMPLE_SMOOTH)       # (with d_img: the packed entry)
        crop[1].copy_(whole[y:y + 224, x:x + 224])
        torch.cuda.synchronize()

    def c2():
        ctx.dequant_idct_region_dev(d_co, info, (x, y, 224, 224), 1, d_img=crop[2], upsampling=J.UPSAMPLE_SMOOTH)
        torch.cuda.synchronize()

    return {"C1 whole smooth picture + device slice": c1, "C2 region, smooth": c2}, crop


def timed_rounds(arms, rounds, warmup):
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t) * 1e3)
    return times


def report(name, n, t):
    res = {"arms": {}}
    for k, v in t.items():
        res["arms"][k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "rounds": len(v)}
        print(f"{name} ({n} files), {k}: median {np.median(v):.3f} ms, min {np.min(v):.3f} ms, max {np.max(v):.3f} ms")
    (ka, ra), (kb, rb) = list(res["arms"].items())
    diff = rb["median_ms"] - ra["median_ms"]
    spread = max(ra["max_ms"] - ra["min_ms"], rb["max_ms"] - rb["min_ms"])
    res["second_minus_first_ms"] = diff
    res["larger_spread_ms"] = spread
    res["difference_exceeds_spread"] = bool(abs(diff) > spread)
    print(f"{name}: '{kb}' - '{ka}' = {diff:+.3f} ms of {ra['median_ms']:.3f} ms ({100 * diff / ra['median_ms']:+.1f} %); the larger spread of the two: "
          f"{spread:.3f} ms: the difference {'EXCEEDS' if abs(diff) > spread else 'does NOT exceed'} it")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16, help="different 1920 x 1080 pictures of the one-size workload")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--rounds-one-size", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--whole", type=int, default=4096, help="edge of arm C's file; 0: skip")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--trace", action="store_true", help="three calls of every arm, no timing")
    a = ap.parse_args()
    ctx = J.Context(0)
    lib = api.load_library()
    dev = torch.device("cuda", 0)
    n = a.files
    rng = np.random.default_rng(17)
    sizes = [(int(rng.integers(320, 801)), int(rng.integers(240, 601))) for _ in range(n)]
    files = [encode(ctx, W, H, 1000 + k) for k, (W, H) in enumerate(sizes)]
    wins1 = []
    for W, H in sizes:
        w, h = int(rng.integers(224, min(448, W) + 1)), int(rng.integers(224, min(448, H) + 1))
        wins1.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h, 1))
    big = [encode(ctx, 1920, 1080, 5000 + k) for k in range(a.distinct)]
    one_files = [big[k % a.distinct] for k in range(n)]
    one_wins = [(int(rng.integers(0, 1920 - 224 + 1)), int(rng.integers(0, 1080 - 224 + 1)), 224, 224, 1) for _ in range(n)]
    jobs = [("mixed sizes, scale 1", Workload("mixed", files, sizes, wins1, 448, 448), batch_arms, a.rounds),
            ("one size (1920 x 1080), 224^2 windows", Workload("one size", one_files, [(1920, 1080)] * n, one_wins, 224, 224), batch_arms, a.rounds_one_size),
            ("resized, mixed sizes", ResizedWorkload("resized", files, sizes, np.random.default_rng(18)), resized_arms, a.rounds)]
    result = {"files": n, "workloads": {}}
    for name, wl, make, rounds in jobs:
        arms, d = make(lib, ctx, wl, dev)
        if a.trace:
            for fn in arms.values():
                for _ in range(3):
                    fn()
            continue
        if a.check and make is batch_arms:
            arms["B smooth"]()
            got = d[J.UPSAMPLE_SMOOTH].cpu().numpy()
            for k in range(0, wl.n, max(1, wl.n // 16)):
                x, y, w, h, s = wl.wins[k]
                _, img = ctx.decode_jpeg_region_packed(wl.files[k], (x, y, w, h), scale=s, upsampling=J.UPSAMPLE_SMOOTH)
                assert np.array_equal(got[k, :h, :w], img), (name, k)
            print(f"{name}: B's bytes equal decode_jpeg_region_packed(..., upsampling=UPSAMPLE_SMOOTH) on the files sampled")
        res = report(name, wl.n, timed_rounds(arms, rounds, a.warmup))
        res["bytes_that_differ"] = float((d[J.UPSAMPLE_NEAREST] != d[J.UPSAMPLE_SMOOTH]).float().mean())
        for k, fn in arms.items():
            sys.stderr.write(f"laps of one call of {k}, {name}:\n")
            sys.stderr.flush()
            os.environ["JPEZY_BATCH_DEBUG"] = "1"
            fn()
            del os.environ["JPEZY_BATCH_DEBUG"]
        res["grouped_files"] = int(lib.jpezy_ctx_last_batch_fast_count(ctx._h))
        print(f"{name}: {res['grouped_files']} of {wl.n} files took the grouped path; {100 * res['bytes_that_differ']:.1f} % of the output bytes differ between A and B")
        result["workloads"][name] = res
    assert lib.jpezy_ctx_set_windows_upsampling(ctx._h, J.UPSAMPLE_NEAREST) == 0
    if a.whole:
        arms, crop = single_file_arms(ctx, a.whole, dev)
        if a.trace:
            for fn in arms.values():
                for _ in range(3):
                    fn()
        else:
            name = f"one {a.whole}^2 file, a 224^2 window, resident coefficients"
            res = report(name, 1, timed_rounds(arms, a.rounds, a.warmup))
            res["same_bytes"] = bool(torch.equal(crop[1], crop[2]))
            print(f"{name}: C1's and C2's bytes are equal: {res['same_bytes']}")
            result["workloads"][name] = res
    if not a.trace:
        print(json.dumps(result))


if __name__ == "__main__":
    main()
