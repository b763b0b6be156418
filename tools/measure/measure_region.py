#!/usr/bin/env python3
"""Region decode against the full decode on the same input and in the same run: one 4096 x 4096 file of jpezy's own layout (4:2:0) and
one 4:4:4 file of the same picture (smooth picture + noise), centred square windows.

  (a) end to end   .jpg bytes on the host -> planes on the host: jpezy_decode_jpeg_region for each window against jpezy_decode_jpeg, bare
                   ctypes, output planes preallocated and touched, host clock, the arms alternated round by round after a warm-up of every
                   arm; median and minimum over the rounds
  (b) device stage jpezy_dequant_idct_region_dev for each window at scale 1 and scale 2 (the window then has the same number of output
                   pixels, i.e. covers twice the edge of the file) against the full-size stage of the same file -- jpezy_dequant_idct_dev,
                   the fused kernel, for the own layout, jpezy_dequant_idct_generic_dev for 4:4:4 -- and against the whole picture at 1/2
                   (jpezy_dequant_idct_scaled_dev): the coefficients resident in HBM, device events around one call, same alternation
  (c) bytes        what each arm downloads (three planes)

The crossover is the smallest measured window whose region stage is no faster than the full-size stage.  --check compares one window per
file and scale with the slice of the full decode first.  Prints one line per arm and a JSON line with every figure (times in
microseconds)."""
import argparse
import ctypes as C
import io
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
    return np.clip((np.sin(xx / 37.0) * 60 + np.cos(yy / 23.0) * 50 + 128)[..., None] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)


def centred(ws, hs, edge):
    return ((ws - edge) // 2, (hs - edge) // 2, edge, edge)


def timed_rounds(arms, rounds, warmup, device_events):
    """every arm warmed up, then the arms alternated round by round -> {name: [us]}"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            if device_events:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
            else:
                t = time.perf_counter()
                fn()
                times[k].append((time.perf_counter() - t) * 1e6)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, nargs="+", default=[224, 512, 1024, 2048, 3072])
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    assert a.rounds >= 20, "medians of at least 20 repetitions"
    W = H = a.size
    ctx = J.Context(0)
    dev = torch.device("cuda", 0)
    img = picture(W, H)
    files = {"own layout (4:2:0)": ctx.encode_jpeg(*[np.ascontiguousarray(img[..., k]).reshape(-1) for k in range(3)], W, H)}
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=90, subsampling=0)
    files["4:4:4"] = buf.getvalue()
    lib = api.load_library()
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    result = {"size": [W, H], "rounds": a.rounds, "files": {}}

    for tag, data in files.items():
        info, d_co = ctx.read_jpeg_gpu(data)
        own = tag.startswith("own")
        windows = sorted(e for e in a.windows if e <= W)
        res = {"jpg_bytes": len(data), "layout": [[info.H[k], info.V[k]] for k in range(info.ncomp)], "huffman_decoder": "GPU" if ctx.last_huffdec_passes() > 0 else "host"}

        if a.check:
            full = [p.reshape(H, W) for p in ctx.decode_jpeg(data)[1:]]
            half = [p.reshape(H // 2, W // 2) for p in ctx.decode_jpeg_scaled(data, 2)[1:]]
            x, y, w, h = centred(W, H, windows[0])
            got = ctx.decode_jpeg_region(data, (x, y, w, h))[1:]
            ok = all(np.array_equal(g.reshape(h, w), f[y:y + h, x:x + w]) for g, f in zip(got, full))
            x, y, w, h = centred(W // 2, H // 2, windows[0])
            got = ctx.decode_jpeg_region(data, (x, y, w, h), scale=2)[1:]
            ok = ok and all(np.array_equal(g.reshape(h, w), f[y:y + h, x:x + w]) for g, f in zip(got, half))
            print(f"{tag}: the {windows[0]}^2 windows equal the slices of the full decodes: {ok}")
            assert ok

        # ---- (b) device stage ----
        planes = [torch.empty(W * H, dtype=torch.uint8, device=dev) for _ in range(3)]
        arms = {}
        if own:
            arms["full: dequant_idct_dev (fused)"] = lambda: ctx.dequant_idct_dev(d_co, W, H, *planes, qt=info.qt, comp_tq=tuple(info.Tq))
        arms["full: dequant_idct_generic_dev"] = lambda: ctx.dequant_idct_generic_dev(d_co, info, *planes)
        arms["full at 1/2: dequant_idct_scaled_dev"] = lambda: ctx.dequant_idct_scaled_dev(d_co, info, 2, *planes)
        for scale in (1, 2):
            ws, hs = J.scaled_size(W, H, scale)
            for e in windows:
                if e > ws:
                    continue
                arms[f"region {e}^2 at 1/{scale}"] = lambda r=centred(ws, hs, e), s=scale: ctx.dequant_idct_region_dev(d_co, info, r, s, *planes)
        t = timed_rounds(arms, a.rounds, a.warmup, device_events=True)
        res["device_stage"] = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v))} for k, v in t.items()}
        for k, v in t.items():
            print(f"{W}x{H} {tag}, device stage, {k}: median {np.median(v):.1f} us, min {np.min(v):.1f} us")
        full_key = "full: dequant_idct_dev (fused)" if own else "full: dequant_idct_generic_dev"
        full_us = float(np.median(t[full_key]))
        slower = [e for e in sorted(windows) if f"region {e}^2 at 1/1" in t and float(np.median(t[f"region {e}^2 at 1/1"])) >= full_us]
        res["crossover_edge_scale1"] = slower[0] if slower else None
        print(f"{W}x{H} {tag}: the region stage at full size stops beating '{full_key}' ({full_us:.1f} us) at: "
              f"{str(slower[0]) + '^2' if slower else 'no measured window'}")

        # ---- (a) end to end, (c) bytes downloaded ----
        arr = np.frombuffer(data, dtype=np.uint8)
        host = [np.zeros(W * H, dtype=np.uint8) for _ in range(3)]
        fi = api.FrameInfo()

        def whole():
            rc = lib.jpezy_decode_jpeg(ctx._h, vp(arr), arr.size, 0, C.byref(fi), vp(host[0]), vp(host[1]), vp(host[2]), W * H)
            assert rc == 0, lib.jpezy_hip_last_error()

        def window(rect):
            rc = lib.jpezy_decode_jpeg_region(ctx._h, vp(arr), arr.size, 0, 1, C.byref(rect), C.byref(fi), vp(host[0]), vp(host[1]), vp(host[2]), W * H)
            assert rc == 0, lib.jpezy_hip_last_error()

        arms = {"jpezy_decode_jpeg (full)": whole}
        nbytes = {"jpezy_decode_jpeg (full)": 3 * W * H}
        for e in windows:
            arms[f"jpezy_decode_jpeg_region {e}^2"] = lambda r=api.Rect(*centred(W, H, e)): window(r)
            nbytes[f"jpezy_decode_jpeg_region {e}^2"] = 3 * e * e
        t = timed_rounds(arms, a.rounds, a.warmup, device_events=False)
        res["end_to_end"] = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "bytes_downloaded": nbytes[k]} for k, v in t.items()}
        for k, v in t.items():
            print(f"{W}x{H} {tag} ({len(data) / 1e6:.2f} MB .jpg), end to end, {k}: median {np.median(v) / 1e3:.3f} ms, min {np.min(v) / 1e3:.3f} ms, "
                  f"{nbytes[k]} bytes downloaded")
        result["files"][tag] = res
    print(json.dumps(result))


if __name__ == "__main__":
    main()
