#!/usr/bin/env python3
"""JPEZY_DOWNSAMPLE_AVERAGE beside JPEZY_DOWNSAMPLE_POINT: the transform kernel on one 4096 x 4096 frame resident in device memory.

Two pictures: random pixels (the benchmark's workload) and the photo-like picture of tools/measure/measure_sampling.py (smooth gradients
+ mild noise).  The legs take turns inside every round (interleaved); median (min - max) over the rounds, HIP events around K launches:

  point      fdct_quant_dev / fdct_quant_packed_dev (RGB24) of this checkout with the default mode
  average    the same calls with set_chroma_downsampling(DOWNSAMPLE_AVERAGE); the ratio average / point is printed beside it
  parent     with --parent DIR: the point legs of another checkout of the project (the parent commit, built), loaded into the same
             process under another module name and alternated with this checkout's -- "did the default path move", to be read against
             the parent's own min - max spread

Nothing here is an acceptance bound.

    python tools/measure/measure_chroma_average.py [--parent DIR] [--rounds 9] [--iters 10] [--size 4096] [--out FILE]
"""
import argparse
import importlib.util
import os
import statistics
import sys
from pathlib import Path

import numpy as np
import torch


def pictures(W, H):
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    yield "random", [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3)]
    base = 128 + 90 * np.sin(xx / 97.0) * np.cos(yy / 61.0)
    yield "smooth+noise", [np.clip(base * s + rng.normal(0, 3, (H, W)), 0, 255).astype(np.uint8) for s in (1.0, 0.9, 0.8)]


def load_package(root, name):
    """jpezy_amd of the checkout at root, as module `name` (its relative imports and its library follow the package's own directory)"""
    pkg = Path(root).resolve() / "jpezy_amd"
    spec = importlib.util.spec_from_file_location(name, pkg / "__init__.py", submodule_search_locations=[str(pkg)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    mod.load_library()
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    J = load_package(Path(__file__).resolve().parents[2], "jpezy_amd")
    P = load_package(args.parent, "jpezy_amd_parent") if args.parent else None
    W = H = args.size
    dev = torch.device("cuda:0")
    ctx = J.Context(0)
    pctx = P.Context(0) if P else None
    lines = [f"measure_chroma_average: {W}x{H}, {args.rounds} interleaved rounds of {args.iters} calls per leg, {torch.cuda.get_device_name(0)}",
             f"this: {os.path.relpath(J.library_path())}" + (f"; parent: {os.path.relpath(P.library_path())}" if P else ""),
             f"{'picture':13s} {'input':>7s} {'leg':>13s} {'median us':>10s} {'min':>9s} {'max':>9s} {'/ point':>8s}"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, planes in pictures(W, H):
        d = [torch.from_numpy(p).to(dev) for p in planes]
        rgb = torch.from_numpy(np.ascontiguousarray(np.stack(planes, axis=-1))).to(dev)
        co = torch.empty(J.coeff_count(W, H), dtype=torch.int16, device=dev)
        legs = {}
        for inp, call in (("planar", lambda c: c.fdct_quant_dev(d[0], d[1], d[2], W, H, co)),
                          ("RGB24", lambda c: c.fdct_quant_packed_dev(rgb, co, format=J.PIX_RGB24))):
            if pctx:
                legs[inp, "parent point"] = (pctx, None, call)
            legs[inp, "point"] = (ctx, J.DOWNSAMPLE_POINT, call)
            legs[inp, "average"] = (ctx, J.DOWNSAMPLE_AVERAGE, call)
        times = {k: [] for k in legs}
        for rnd in range(args.rounds + 1):                  # round 0 warms up and is dropped
            for key, (c, mode, call) in legs.items():
                if mode is not None:
                    c.set_chroma_downsampling(mode)
                call(c)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.iters):
                    call(c)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[key].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        ctx.set_chroma_downsampling(J.DOWNSAMPLE_POINT)
        for (inp, leg), v in times.items():
            med = statistics.median(v)
            ratio = f"{med / statistics.median(times[inp, 'point']):8.3f}" if leg != "point" else f"{'':8s}"
            lines.append(f"{name:13s} {inp:>7s} {leg:>13s} {med:10.1f} {min(v):9.1f} {max(v):9.1f} {ratio}")
    ctx.close()
    if pctx:
        pctx.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
