#!/usr/bin/env python3
"""Random-resized-crop style input, every crop brought to 224 x 224 on the device: jpezy_decode_windows_resized_dev against what a caller
did before it, on measure_windows.py's files, in one process, the arms alternated round by round after a warm-up of each.  A host clock
around work that ends in a device synchronise; median, minimum and spread (max - min) per arm.

  Workloads   mixed      N own-layout files, widths 320..800 and heights 240..600 from measure_windows.py's seed
              one size   N files of 1920 x 1080 (--distinct different pictures, repeated)
  Sources     per file a rectangle of 8 % .. 100 % of the picture's area with an aspect ratio of 3/4 .. 4/3 (log-uniform), placed at random,
              from a fixed seed; resize_pick_window turns it into the window and the largest scale that still leaves 224 x 224 pixels
  Arms        A  jpezy_decode_windows_resized_dev into a [N, 224, 224, 3] device tensor
              B  jpezy_decode_windows_dev of the same windows into slots of the largest window, then per file
                 torch.nn.functional.interpolate(..., mode="bilinear", antialias=True) on the device, rounded back to bytes into [N, 224, 224, 3]
              C  jpezy_decode_windows_dev alone on the same windows: A - C is what the second stage adds
  Also        the JPEZY_BATCH_DEBUG laps of one call of A per workload on stderr, and the largest difference between A's and B's bytes (the two
              use different arithmetic: the figure is information, not a check)
  --filter    the resampling filter of arm A (bilinear, box, bicubic, lanczos; B keeps torch's bilinear, so A against B is then information
              only).  With a filter other than bilinear a fourth arm D runs A with the direct loop forced (jpezy_ctx_set_resample_direct),
              alternated with the others, and --stage-rounds rounds measure the RESAMPLING STAGE of A and D alone by the device events the
              library records around it (the "tables up + resample" lap of JPEZY_BATCH_DEBUG, read back from stderr), alternated too
  --direct    arm A itself runs the direct loop (and there is no arm D)

Bare ctypes, buffers preallocated and touched.  Prints one line per arm and a JSON line with every figure (times in milliseconds)."""
import argparse
import ctypes as C
import json
import math
import os
import re
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpezy_amd as J  # noqa: E402
from jpezy_amd import api  # noqa: E402
from measure_windows import encode  # noqa: E402

OUT = 224


def source_rect(rng, W, H):
    """torchvision's RandomResizedCrop recipe: area fraction 0.08..1, log-uniform aspect 3/4..4/3, ten tries, else the centre"""
    for _ in range(10):
        area = W * H * rng.uniform(0.08, 1.0)
        ar = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
        w, h = int(round(math.sqrt(area * ar))), int(round(math.sqrt(area / ar)))
        if 0 < w <= W and 0 < h <= H:
            return int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h
    e = min(W, H)
    return (W - e) // 2, (H - e) // 2, e, e


class Workload:
    def __init__(self, name, files, sizes, rng):
        self.name, self.files, self.sizes, self.n = name, files, sizes, len(files)
        self.wins = [api.resize_pick_window(W, H, source_rect(rng, W, H), OUT, OUT) for W, H in sizes]
        self.arrs = [np.frombuffer(f, dtype=np.uint8) for f in files]
        self.data = (C.c_void_p * self.n)(*[a.ctypes.data for a in self.arrs])
        self.lens = (C.c_size_t * self.n)(*[a.size for a in self.arrs])
        self.cwins = (api.Window * self.n)(*[api.Window(api.Rect(*r), s) for r, s in self.wins])
        self.mirror = (C.c_uint8 * self.n)(*[int(rng.integers(0, 2)) for _ in range(self.n)])
        self.infos, self.placed, self.status = (api.FrameInfo * self.n)(), (api.Rect * self.n)(), (C.c_int * self.n)()
        self.Ws, self.Hs = max(r[2] for r, _ in self.wins), max(r[3] for r, _ in self.wins)


FILTERS = {"bilinear": J.FILTER_BILINEAR, "box": J.FILTER_BOX, "bicubic": J.FILTER_BICUBIC, "lanczos": J.FILTER_LANCZOS}


def stage_ms(fn):
    """one call of fn with JPEZY_BATCH_DEBUG set and stderr in a file: the sum of the call's resampling-stage laps (device events)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as f:
        os.dup2(f.fileno(), 2)
        os.environ["JPEZY_BATCH_DEBUG"] = "1"
        try:
            fn()
        finally:
            del os.environ["JPEZY_BATCH_DEBUG"]
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        text = f.read().decode(errors="replace")
    laps = [float(m) for m in re.findall(r"tables up \+ resample.*?: ([0-9.]+) ms \(device events\)", text)]
    assert laps, text[-400:]
    return sum(laps)


def make_arms(lib, ctx, wl, dev):
    n, Hs, Ws = wl.n, wl.Hs, wl.Ws
    d_a = torch.zeros((n, OUT, OUT, 3), dtype=torch.uint8, device=dev)
    d_b = torch.zeros((n, OUT, OUT, 3), dtype=torch.uint8, device=dev)
    d_slots = torch.zeros((n, Hs, Ws, 3), dtype=torch.uint8, device=dev)
    row, slot = Ws * 3, Hs * Ws * 3
    flip = [bool(m) for m in wl.mirror]

    def arm_a():
        rc = lib.jpezy_decode_windows_resized_dev(ctx._h, n, wl.data, wl.lens, 0, wl.cwins, wl.mirror, OUT, OUT, J.PIX_RGB24, 0, 0, d_a.data_ptr(),
                                                  n * OUT * OUT * 3, wl.infos, wl.placed, wl.status)
        assert rc == 0, lib.jpezy_hip_last_error()

    def arm_c():
        rc = lib.jpezy_decode_windows_dev(ctx._h, n, wl.data, wl.lens, 0, wl.cwins, J.PIX_RGB24, row, slot, d_slots.data_ptr(), n * slot, wl.infos, wl.placed,
                                          wl.status)
        assert rc == 0, lib.jpezy_hip_last_error()

    def arm_b():
        arm_c()
        for k in range(n):
            (_, _, w, h), _ = wl.wins[k]
            img = d_slots[k, :h, :w].permute(2, 0, 1)[None].float()
            res = F.interpolate(img, size=(OUT, OUT), mode="bilinear", antialias=True)[0]
            if flip[k]:
                res = res.flip(2)
            d_b[k] = res.round_().clamp_(0, 255).to(torch.uint8).permute(1, 2, 0)
        torch.cuda.synchronize()

    return {"A decode_windows_resized_dev": arm_a, "B decode_windows_dev + interpolate per file": arm_b, "C decode_windows_dev alone": arm_c}, d_a, d_b


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16, help="different 1920 x 1080 pictures of the one-size workload")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--rounds-one-size", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--filter", choices=sorted(FILTERS), default="bilinear")
    ap.add_argument("--direct", action="store_true", help="arm A runs the direct loop, never the two-pass tile")
    ap.add_argument("--stage-rounds", type=int, default=15, help="rounds of the stage-only A / D measurement (a filter other than bilinear)")
    a = ap.parse_args()
    ctx = J.Context(0)
    ctx.set_windows_filter(FILTERS[a.filter])
    ctx.set_resample_direct(a.direct)
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
    result = {"files": n, "out": OUT, "filter": a.filter, "direct": bool(a.direct), "workloads": {}}
    for wl, rounds in workloads:
        arms, d_a, d_b = make_arms(lib, ctx, wl, dev)
        name_a = "A decode_windows_resized_dev"
        if a.filter != "bilinear" and not a.direct:
            def arm_d(arm_a=arms[name_a]):
                ctx.set_resample_direct(1)
                try:
                    arm_a()
                finally:
                    ctx.set_resample_direct(0)
            arms["D A with the direct loop forced"] = arm_d
        t = timed_rounds(arms, rounds, a.warmup)
        scales = {s: sum(1 for _, q in wl.wins if q == s) for s in (1, 2, 4, 8)}
        res = {"windows_per_scale": scales, "largest_window": [wl.Ws, wl.Hs], "arms": {}}
        for k, v in t.items():
            res["arms"][k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "rounds": len(v)}
            print(f"{wl.name} ({wl.n} files), {k}: median {np.median(v):.2f} ms, min {np.min(v):.2f} ms, spread {np.max(v) - np.min(v):.2f} ms")
        ra, rb, rc = (res["arms"][k] for k in list(arms)[:3])
        margin = rb["median_ms"] - ra["median_ms"]
        spread = max(ra["max_ms"] - ra["min_ms"], rb["max_ms"] - rb["min_ms"])
        res["a_below_b_by_more_than_both_spreads"] = bool(margin > spread)
        res["second_stage_ms"] = ra["median_ms"] - rc["median_ms"]
        print(f"{wl.name}: A's median is {margin:.2f} ms below B's (the larger spread of the two: {spread:.2f} ms): {'holds' if margin > spread else 'DOES NOT HOLD'}")
        print(f"{wl.name}: A - C = {res['second_stage_ms']:.2f} ms (the second stage); windows per scale {scales}, largest window {wl.Ws} x {wl.Hs}")
        res["max_abs_difference_a_b"] = int((d_a.int() - d_b.int()).abs().max())
        print(f"{wl.name}: largest difference between A's and B's bytes: {res['max_abs_difference_a_b']}")
        sys.stderr.write(f"laps of one call of A, {wl.name}:\n")
        sys.stderr.flush()
        os.environ["JPEZY_BATCH_DEBUG"] = "1"
        arms["A decode_windows_resized_dev"]()
        del os.environ["JPEZY_BATCH_DEBUG"]
        res["grouped_files"] = int(lib.jpezy_ctx_last_batch_fast_count(ctx._h))
        res["tiled_files"] = int(lib.jpezy_ctx_last_resample_tiled_count(ctx._h))
        print(f"{wl.name}: {res['grouped_files']} of {wl.n} files took A's grouped path, {res['tiled_files']} the two-pass tile")
        if "D A with the direct loop forced" in arms:
            stage = {"tile": [], "direct": []}
            for _ in range(a.stage_rounds):
                stage["tile"].append(stage_ms(arms[name_a]))
                stage["direct"].append(stage_ms(arms["D A with the direct loop forced"]))
            res["stage_ms"] = {k: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "rounds": len(v)}
                               for k, v in stage.items()}
            st, sd = res["stage_ms"]["tile"], res["stage_ms"]["direct"]
            margin = sd["median_ms"] - st["median_ms"]
            spread = max(st["max_ms"] - st["min_ms"], sd["max_ms"] - sd["min_ms"])
            res["tile_below_direct_by_more_than_both_spreads"] = bool(margin > spread)
            print(f"{wl.name}, resampling stage by device events ({a.filter}): tile median {st['median_ms']:.3f} ms ({st['min_ms']:.3f}..{st['max_ms']:.3f}), "
                  f"direct median {sd['median_ms']:.3f} ms ({sd['min_ms']:.3f}..{sd['max_ms']:.3f}); the tile is {margin:.3f} ms below "
                  f"(the larger spread: {spread:.3f} ms): {'holds' if margin > spread else 'DOES NOT HOLD'}")
        result["workloads"][wl.name] = res
    print(json.dumps(result))


if __name__ == "__main__":
    main()
