#!/usr/bin/env python3
"""Smooth chroma upsampling against the replicating decode on the same input: one 4096 x 4096 file of jpezy's own 4:2:0 layout (smooth
picture + noise), its coefficients resident in HBM.

  (a) dequant_idct_generic_dev                generic stage 1 + the replicating stage 2 (generic_rgb_kernel)
  (b) dequant_idct_upsampling_dev, smooth     the same stage 1 + smooth_rgb_kernel
  (c) dequant_idct_dev                        the fused kernel, for scale

Device events around one call, the arms alternated round by round in one process after a warm-up of each; median (min - max) over the
rounds.  (b) - (a) is the price of the new second stage against the one it stands beside.  Also printed: the share of output bytes that
differ between the two modes on this picture.  --check compares the smooth picture with the numpy restatement of the definition
(tests/smooth_model.py) first.  --kernels N: only N calls of (a) and (b) each, nothing timed -- the workload of a
`rocprofv3 --kernel-trace --stats` run of its own, which gives the two second-stage kernels' own times.
Prints one line per arm and a JSON line with every figure (times in microseconds)."""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import jpezy_amd as J  # noqa: E402


def picture(W, H, seed=5):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.clip((np.sin(xx / 37.0) * 60 + np.cos(yy / 23.0) * 50 + 128)[..., None] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
    return [np.ascontiguousarray(img[..., k]).reshape(-1) for k in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--kernels", type=int, default=0)
    a = ap.parse_args()
    assert a.rounds >= 7
    W = H = a.size
    ctx = J.Context(0)
    dev = torch.device("cuda", 0)
    data = ctx.encode_jpeg(*picture(W, H), W, H)
    info, d_co = ctx.read_jpeg_gpu(data)
    out = {k: [torch.empty(W * H, dtype=torch.uint8, device=dev) for _ in range(3)] for k in "abc"}
    arms = {
        "(a) generic stage 1 + replicating stage 2": lambda: ctx.dequant_idct_generic_dev(d_co, info, *out["a"]),
        "(b) generic stage 1 + smooth stage 2": lambda: ctx.dequant_idct_upsampling_dev(d_co, info, *out["b"], upsampling=J.UPSAMPLE_SMOOTH),
        "(c) fused kernel": lambda: ctx.dequant_idct_dev(d_co, W, H, *out["c"], qt=info.qt, comp_tq=tuple(info.Tq)),
    }
    if a.kernels:
        for _ in range(a.kernels):
            for k in list(arms)[:2]:
                arms[k]()
        torch.cuda.synchronize()
        print(f"{a.kernels} calls of (a) and (b) each")
        return
    result = {"size": [W, H], "jpg_bytes": len(data), "rounds": a.rounds}

    if a.check:
        sys.path.insert(0, str(ROOT / "tests"))
        import smooth_model as M
        _, co = J.read_jpeg(data)
        got = ctx.decode_jpeg(data, upsampling=J.UPSAMPLE_SMOOTH)[1:]
        ok = all(np.array_equal(x, e) for x, e in zip(got, M.decode_planes(co, info)))
        print(f"smooth: equal to the model: {ok}")
        assert ok

    for fn in arms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    assert all(torch.equal(x, e) for x, e in zip(out["a"], out["c"])), "the generic pair and the fused kernel differ"
    differ = sum(int((x != e).sum()) for x, e in zip(out["a"], out["b"]))
    result["bytes_differ_share"] = differ / (3.0 * W * H)
    print(f"{W}x{H}: {differ} of {3 * W * H} output bytes differ between the two modes ({100.0 * differ / (3 * W * H):.1f} %)")
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
        result[k] = {"median_us": float(np.median(t)), "min_us": float(np.min(t)), "max_us": float(np.max(t))}
        print(f"{W}x{H} device stage, {k}: median {np.median(t):.1f} us ({np.min(t):.1f} - {np.max(t):.1f})")
    ka, kb = list(arms)[:2]
    result["b_minus_a_median_us"] = float(np.median(times[kb]) - np.median(times[ka]))
    print(f"(b) - (a): {result['b_minus_a_median_us']:.1f} us")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
