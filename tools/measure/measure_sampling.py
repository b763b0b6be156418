#!/usr/bin/env python3
"""4:4:4 and 4:2:2 beside 4:2:0: the transform kernel, the entropy stage and both together, on one 4096 x 4096 frame resident in device memory.

Two pictures: random pixels (the benchmark's workload) and the photo-like picture of tools/measure/measure_quality.py (smooth gradients +
mild noise).  Per sampling, the legs take turns inside every round (interleaved); median / min / max over the rounds:

  transform    fdct_quant_dev, HIP events around K launches
  entropy      write_jpeg_gpu_dev (coefficients in HBM -> the whole .jpg in HBM), Annex-K tables, no restart interval
  entropy rst  the same with a restart interval of one MCU row
  both         fdct_quant_dev + write_jpeg_gpu_dev back to back on one stream
  opt (host)   write_jpeg_gpu with per-image Huffman tables (host-delivered form: histogram kernel, tables on the host, coder, copy),
               host clock around a call that ends synchronised
  roofline     the transform's algorithmic traffic -- 3 bytes in and 3 (4:2:0), 4 (4:2:2) or 6 (4:4:4) bytes out per pixel -- over its
               time, as a fraction of 8.0 TB/s (specification) and of 6.29 TB/s (the float4-copy figure of this GPU)

Samplings: 420, 444, 422, and 422avg -- 4:2:2 with the context in DOWNSAMPLE_AVERAGE (the transform differs; the entropy legs see other
coefficients of the same layout).  422i422, 422nv16, 422yuy2, 422uyvy: the 4:2:2 transform from YCbCr 4:2:2 samples -- planes, one
interleaved chroma plane, packed macropixels (fdct_quant_ycc422_dev / fdct_quant_yuv422_dev; 2 bytes in and 4 out per pixel) --, the
transform leg only.

--root DIR imports jpezy_amd from another checkout of the project (the parent commit beside this one, for the A/B of the 4:2:0 path):
a checkout without a sampling runs the legs of those it has.  Nothing here is an acceptance bound.

    python tools/measure/measure_sampling.py [--root DIR] [--rounds 9] [--iters 10] [--size 4096] [--samplings 420,444,422,422avg] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch


YCC422 = ("422i422", "422nv16", "422yuy2", "422uyvy")


def pictures(W, H):
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    yield "random", [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3)]
    base = 128 + 90 * np.sin(xx / 97.0) * np.cos(yy / 61.0)
    yield "smooth+noise", [np.clip(base * s + rng.normal(0, 3, (H, W)), 0, 255).astype(np.uint8) for s in (1.0, 0.9, 0.8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(Path(__file__).resolve().parents[2]))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--samplings", default="420,444")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    import jpezy_amd as J
    W = H = args.size
    # name -> (the library's constant, bytes of algorithmic traffic per pixel, MCU width, averaged chroma)
    known = {"420": (0, 6, 16, False), "444": (getattr(J, "SAMPLING_444", None), 9, 8, False),
             "422": (getattr(J, "SAMPLING_422", None), 7, 16, False), "422avg": (getattr(J, "SAMPLING_422", None), 7, 16, True)}
    known.update({s: (getattr(J, "SAMPLING_422", None), 6, 16, False) for s in YCC422})     # 2 bytes in, 4 out per pixel
    samplings = [s for s in args.samplings.split(",") if s not in YCC422 and known[s][0] is not None]
    dev = torch.device("cuda:0")
    ctx = J.Context(0)
    lines = [f"measure_sampling: {W}x{H}, {args.rounds} interleaved rounds of {args.iters} calls per leg, {torch.cuda.get_device_name(0)}, "
             f"library {J.library_path()}",
             f"{'picture':13s} {'sampling':>8s} {'leg':>12s} {'median us':>10s} {'min':>9s} {'max':>9s} {'B/px':>5s} {'of 8.0 TB/s':>11s} {'of 6.29':>8s} {'file bytes':>11s}"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for name, planes in pictures(W, H):
        d = [torch.from_numpy(p).to(dev) for p in planes]
        legs = {}
        state = {}
        for s in samplings:
            const, _, mcu_w, avg = known[s]
            kw = {} if s == "420" else {"sampling": const}
            ncoef = J.coeff_count(W, H, **kw)
            bound = J.jpeg_bound(W, H, const) if s != "420" else J.load_library().jpezy_jpeg_bound(W, H)
            co = torch.empty(ncoef, dtype=torch.int16, device=dev)
            out = torch.empty((1, bound), dtype=torch.uint8, device=dev)
            sizes = torch.zeros(1, dtype=torch.int64, device=dev)
            row = (W + mcu_w - 1) // mcu_w
            state[s] = (kw, co, out, sizes, row)

            def fd(kw=kw, co=co, avg=avg):
                if avg:
                    ctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
                ctx.fdct_quant_dev(d[0], d[1], d[2], W, H, co, **kw)
                if avg:
                    ctx.set_chroma_downsampling(J.DOWNSAMPLE_POINT)
            en = lambda kw=kw, co=co, out=out, sizes=sizes: ctx.write_jpeg_gpu_dev(co, W, H, out, sizes, **kw)
            legs[s, "transform"] = (fd, 0, False)
            legs[s, "entropy"] = (en, 0, False)
            legs[s, "entropy rst"] = (en, row, False)
            legs[s, "both"] = (lambda fd=fd, en=en: (fd(), en()), 0, False)
            legs[s, "opt (host)"] = (lambda kw=kw, co=co: ctx.write_jpeg_gpu(co, W, H, **kw), 0, True)
            fd()
            torch.cuda.synchronize()
        # YCbCr 4:2:2 samples in (include/jpezy_hip_ycc422.h): the transform alone -- its coefficients have 4:2:2's layout, so the entropy
        # legs above are theirs too.  The picture's first plane as Y, every second column of the other two as Cb, Cr: any byte is a sample.
        for s in [x for x in args.samplings.split(",") if x in YCC422 and hasattr(ctx, "fdct_quant_ycc422_dev")]:
            co = torch.empty(J.coeff_count(W, H, sampling=J.SAMPLING_422), dtype=torch.int16, device=dev)
            cb, cr = d[1][:, 0::2].contiguous(), d[2][:, 0::2].contiguous()
            if s == "422i422":
                fd = lambda co=co, cb=cb, cr=cr: ctx.fdct_quant_ycc422_dev(d[0], cb, cr, co)
            elif s == "422nv16":
                uv = torch.stack([cb, cr], -1).contiguous()
                fd = lambda co=co, uv=uv: ctx.fdct_quant_ycc422_dev(d[0], uv[..., 0], uv[..., 1], co)
            else:
                fmt = J.YUV_UYVY if s == "422uyvy" else J.YUV_YUY2
                mp = torch.stack([cb, d[0][:, 0::2], cr, d[0][:, 1::2]] if s == "422uyvy" else [d[0][:, 0::2], cb, d[0][:, 1::2], cr], -1).reshape(H, 2 * W).contiguous()
                fd = lambda co=co, mp=mp, fmt=fmt: ctx.fdct_quant_yuv422_dev(mp, co, format=fmt)
            legs[s, "transform"] = (fd, 0, False)
            fd()
            torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for rnd in range(args.rounds + 1):                  # round 0 warms up (scratch, header upload) and is dropped
            for key, (call, ri, host) in legs.items():
                ctx.set_restart_interval(ri)
                ctx.set_huffman_optimize(1 if host else 0)
                if host:
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    for _ in range(2):
                        call()
                    dt = (time.perf_counter() - t) * 1e6 / 2
                else:
                    call()                                  # a changed setting uploads a header: outside the bracket
                    torch.cuda.synchronize()
                    e0.record()
                    for _ in range(args.iters):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    dt = e0.elapsed_time(e1) * 1e3 / args.iters
                if rnd:
                    times[key].append(dt)
        ctx.set_restart_interval(0)
        ctx.set_huffman_optimize(0)
        for (s, leg), v in times.items():
            med = statistics.median(v)
            bpp = known[s][1]
            roof = f"{bpp:5d} {W * H * bpp / (med * 1e-6) / 8.0e12:11.3f} {W * H * bpp / (med * 1e-6) / 6.29e12:8.3f}" if leg == "transform" else f"{'':5s} {'':11s} {'':8s}"
            size = ""
            if leg == "entropy":
                kw, co, out, sizes, _ = state[s]
                ctx.write_jpeg_gpu_dev(co, W, H, out, sizes, **kw)
                torch.cuda.synchronize()
                size = str(int(sizes[0]))
            lines.append(f"{name:13s} {s:>8s} {leg:>12s} {med:10.1f} {min(v):9.1f} {max(v):9.1f} {roof} {size:>11s}")
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
