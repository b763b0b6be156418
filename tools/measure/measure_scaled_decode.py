#!/usr/bin/env python3
"""Reduced-size decode against the full-size kernels on the same input: one 4096 x 4096 file of jpezy's own layout (smooth picture +
noise), its coefficients resident in HBM.

  device stage   jpezy_dequant_idct_scaled_dev at N = 4, 2, 1 against jpezy_dequant_idct_dev (fused kernel) and
                 jpezy_dequant_idct_generic_dev (the generic pair) at full size: device events around one call, the arms alternated
                 round by round in one process after a warm-up of every arm; median and minimum over the rounds
  end to end     .jpg bytes on the host -> planes on the host: jpezy_decode_jpeg_scaled (scale 2, 4, 8) against jpezy_decode_jpeg,
                 bare ctypes, output planes preallocated and touched, host clock, same alternation

--check compares the three reduced pictures with the numpy restatement of the definition (tests/scaled_model.py) first.
Prints one line per arm and a JSON line with every figure (times in microseconds)."""
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
import jpezy_amd as J  # noqa: E402
from jpezy_amd import api  # noqa: E402


def picture(W, H, seed=5):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.clip((np.sin(xx / 37.0) * 60 + np.cos(yy / 23.0) * 50 + 128)[..., None] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
    return [np.ascontiguousarray(img[..., k]).reshape(-1) for k in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    W = H = a.size
    ctx = J.Context(0)
    dev = torch.device("cuda", 0)
    data = ctx.encode_jpeg(*picture(W, H), W, H)
    info, d_co = ctx.read_jpeg_gpu(data)
    assert ctx.last_huffdec_passes() > 0
    result = {"size": [W, H], "jpg_bytes": len(data), "rounds": a.rounds}

    if a.check:
        sys.path.insert(0, str(ROOT / "tests"))
        import scaled_model as M
        _, co = J.read_jpeg(data)
        for scale in (2, 4, 8):
            got = ctx.decode_jpeg_scaled(data, scale)[1:]
            ok = all(np.array_equal(x, e) for x, e in zip(got, M.decode_planes(co, info, scale)))
            print(f"scale {scale}: equal to the model: {ok}")
            assert ok

    # ---- device stage ----
    full = [torch.empty(W * H, dtype=torch.uint8, device=dev) for _ in range(3)]
    arms = {}
    for scale in (2, 4, 8):
        ws, hs = J.scaled_size(W, H, scale)
        out = [torch.empty(ws * hs, dtype=torch.uint8, device=dev) for _ in range(3)]
        arms[f"scaled_dev N={8 // scale}"] = lambda scale=scale, out=out: ctx.dequant_idct_scaled_dev(d_co, info, scale, *out)
    arms["dequant_idct_dev (fused, full size)"] = lambda: ctx.dequant_idct_dev(d_co, W, H, *full, qt=info.qt, comp_tq=tuple(info.Tq))
    arms["dequant_idct_generic_dev (full size)"] = lambda: ctx.dequant_idct_generic_dev(d_co, info, *full)
    for fn in arms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    for k, t in times.items():
        result[k] = {"median_us": float(np.median(t)), "min_us": float(np.min(t))}
        print(f"{W}x{H} device stage, {k}: median {np.median(t):.1f} us, min {np.min(t):.1f} us")

    # ---- end to end, .jpg bytes on the host -> planes on the host ----
    lib = api.load_library()
    arr = np.frombuffer(data, dtype=np.uint8)
    planes = [np.zeros(W * H, dtype=np.uint8) for _ in range(3)]
    fi = api.FrameInfo()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731

    def e2e(scale):
        if scale == 1:
            rc = lib.jpezy_decode_jpeg(ctx._h, vp(arr), arr.size, 0, C.byref(fi), vp(planes[0]), vp(planes[1]), vp(planes[2]), W * H)
        else:
            rc = lib.jpezy_decode_jpeg_scaled(ctx._h, vp(arr), arr.size, 0, scale, C.byref(fi), vp(planes[0]), vp(planes[1]), vp(planes[2]), W * H)
        assert rc == 0, lib.jpezy_hip_last_error()
    for scale in (1, 2, 4, 8):
        for _ in range(a.warmup):
            e2e(scale)
    host = {s: [] for s in (1, 2, 4, 8)}
    for _ in range(a.rounds):
        for s in host:
            t = time.perf_counter()
            e2e(s)
            host[s].append((time.perf_counter() - t) * 1e6)
    for s, t in host.items():
        name = "jpezy_decode_jpeg" if s == 1 else f"jpezy_decode_jpeg_scaled 1/{s}"
        result[name] = {"median_us": float(np.median(t)), "min_us": float(np.min(t))}
        print(f"{W}x{H} end to end ({len(data) / 1e6:.2f} MB .jpg), {name}: median {np.median(t) / 1e3:.3f} ms, min {np.min(t) / 1e3:.3f} ms")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
