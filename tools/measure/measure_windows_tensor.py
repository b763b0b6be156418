#!/usr/bin/env python3
"""Random-resized-crop style input as the normalised float16 [N, 3, 224, 224] tensor a model takes: jpezy_decode_windows_tensor_dev against
the framework pass it replaces, on measure_windows_resized.py's workloads, windows and mirror flags (same seeds), in one process, the arms
alternated round by round after a warm-up of each.  A host clock around work that ends in a device synchronise; median, minimum and spread
(max - min) per arm.

  Arms   A  jpezy_decode_windows_tensor_dev into a float16 NCHW tensor with the ImageNet constants (jpezy_tensor_normalization)
         B  jpezy_decode_windows_resized_dev into [N, 224, 224, 3] bytes, then on the device permute -> float -> sub(mean) -> div(std) -> half
            (after a division by 255): the pass A replaces
         C  jpezy_decode_windows_resized_dev alone: A - C is what the conversion and the differently shaped store add
  Also   the largest difference between A's and B's elements (B evaluates (x / 255 - mean) / std in three float32 steps, A in two with
         constants rounded once: the figure is information, not a check)

Bare ctypes, buffers preallocated and touched.  Prints one line per arm and a JSON line with every figure (times in milliseconds)."""
import argparse
import ctypes as C
import json
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
from measure_windows import encode  # noqa: E402
from measure_windows_resized import OUT, Workload, timed_rounds  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def make_arms(lib, ctx, wl, dev):
    n = wl.n
    d_a = torch.zeros((n, 3, OUT, OUT), dtype=torch.float16, device=dev)
    d_b = torch.zeros((n, 3, OUT, OUT), dtype=torch.float16, device=dev)
    d_u8 = torch.zeros((n, OUT, OUT, 3), dtype=torch.uint8, device=dev)
    scale, bias = J.tensor_normalization(MEAN, STD)
    mean = torch.tensor(MEAN, dtype=torch.float32, device=dev)[None, :, None, None]
    std = torch.tensor(STD, dtype=torch.float32, device=dev)[None, :, None, None]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def arm_a():
        rc = lib.jpezy_decode_windows_tensor_dev(ctx._h, n, wl.data, wl.lens, 0, wl.cwins, wl.mirror, OUT, OUT, J.PIX_RGB24, J.DT_F16, 3, vp(scale), vp(bias),
                                                 *d_a.stride(), d_a.data_ptr(), d_a.numel(), wl.infos, wl.placed, wl.status)
        assert rc == 0, lib.jpezy_hip_last_error()

    def arm_c():
        rc = lib.jpezy_decode_windows_resized_dev(ctx._h, n, wl.data, wl.lens, 0, wl.cwins, wl.mirror, OUT, OUT, J.PIX_RGB24, 0, 0, d_u8.data_ptr(),
                                                  d_u8.numel(), wl.infos, wl.placed, wl.status)
        assert rc == 0, lib.jpezy_hip_last_error()

    def arm_b():
        arm_c()
        d_b.copy_(d_u8.permute(0, 3, 1, 2).float().div_(255.0).sub_(mean).div_(std).half())
        torch.cuda.synchronize()

    return {"A decode_windows_tensor_dev (float16 NCHW, normalised)": arm_a, "B decode_windows_resized_dev + permute/float/sub/div/half": arm_b,
            "C decode_windows_resized_dev alone": arm_c}, d_a, d_b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16, help="different 1920 x 1080 pictures of the one-size workload")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--rounds-one-size", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ctx = J.Context(0)
    lib = api.load_library()
    dev = torch.device("cuda", 0)
    n = a.files
    rng = np.random.default_rng(17)
    sizes = [(int(rng.integers(320, 801)), int(rng.integers(240, 601))) for _ in range(n)]
    files = [encode(ctx, W, H, 1000 + k) for k, (W, H) in enumerate(sizes)]
    big = [encode(ctx, 1920, 1080, 5000 + k) for k in range(a.distinct)]
    crop_rng = np.random.default_rng(18)
    workloads = [(Workload("mixed sizes", files, sizes, crop_rng), a.rounds),
                 (Workload("one size (1920 x 1080)", [big[k % a.distinct] for k in range(n)], [(1920, 1080)] * n, crop_rng), a.rounds_one_size)]
    result = {"files": n, "out": OUT, "workloads": {}}
    for wl, rounds in workloads:
        arms, d_a, d_b = make_arms(lib, ctx, wl, dev)
        t = timed_rounds(arms, rounds, a.warmup)
        res = {"mirrored": int(sum(wl.mirror)), "arms": {}}
        for k, v in t.items():
            res["arms"][k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "rounds": len(v)}
            print(f"{wl.name} ({wl.n} files), {k}: median {np.median(v):.2f} ms, min {np.min(v):.2f} ms, spread {np.max(v) - np.min(v):.2f} ms")
        ra, rb, rc = (res["arms"][k] for k in arms)
        for name, other in (("B", rb), ("C", rc)):
            diff = ra["median_ms"] - other["median_ms"]
            spread = max(ra["max_ms"] - ra["min_ms"], other["max_ms"] - other["min_ms"])
            res[f"a_minus_{name.lower()}_ms"] = diff
            res[f"a_minus_{name.lower()}_beyond_both_spreads"] = bool(abs(diff) > spread)
            print(f"{wl.name}: A - {name} = {diff:.2f} ms (the larger spread of the two: {spread:.2f} ms): "
                  f"{'resolved' if abs(diff) > spread else 'inside the spread'}")
        diff = (d_a.float() - d_b.float()).abs()
        res["max_abs_difference_a_b"], res["elements_that_differ_a_b"] = float(diff.max()), int((diff != 0).sum())
        print(f"{wl.name}: largest difference between A's and B's elements: {res['max_abs_difference_a_b']:g} "
              f"({res['elements_that_differ_a_b']} of {d_a.numel()} elements differ)")
        res["grouped_files"] = int(lib.jpezy_ctx_last_batch_fast_count(ctx._h))
        result["workloads"][wl.name] = res
    print(json.dumps(result))


if __name__ == "__main__":
    main()
