#!/usr/bin/env python3
"""What planar YCbCr 4:2:0 samples in and out cost against the RGB entry points, on the same picture.

Two inputs, everything resident in device memory: a ring of 6 frames of 4096 x 4096 and one batch of 32 frames of 1920 x 1080 (random
pixels, as bench.py uses; the YCC planes are the RGB frames' own samples: Y of every pixel, Cb / Cr of the top-left pixel of every 2x2,
computed on the device in the reference's FP64 order).  Legs, alternated in one process in interleaved rounds after a warm-up round of
each and timed with device events (K launches per round and leg; median over the rounds, min and max printed):

  encode   fdct_quant_dev on the RGB planes | fdct_quant_ycc_dev on I420 planes | on an NV12 pair (Y + interleaved CbCr)
  decode   dequant_idct_dev into RGB planes | dequant_idct_ycc_dev into I420 planes | into an NV12 pair
  file     decode_jpeg (host RGB planes) | decode_jpeg_ycc (host I420 planes) of one 4096 x 4096 file, host clock around the calls

Before anything is timed the YCC encoders are compared with the RGB one (all coefficients at 4096 x 4096, where the definition says they
are equal; the luma blocks at 1920 x 1080, whose height is even and no multiple of 16) and the YCC decoders with a gray RGB decode.
The RGB kernels are the parent commit's instruction for instruction (tools/profile/kernel_isa_diff.py), so the RGB legs are the parent's.

    python tools/measure/measure_ycc.py [--rounds 7] [--iters 20] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import jpezy_amd as J  # noqa: E402


def ycc_of(rgb):
    """(n, 3, H, W) uint8 -> y (n, H, W), cb, cr (n, CH, CW): the reference's conversion (ref encoder/jpezy_encoder.hpp:244-256) + 128"""
    r, g, b = (rgb[:, k].double() for k in range(3))
    y = torch.trunc((0.2990 * r) + (0.5870 * g) + (0.1140 * b) - 128) + 128
    r2, g2, b2 = r[:, ::2, ::2], g[:, ::2, ::2], b[:, ::2, ::2]
    cb = torch.trunc(-(0.1687 * r2) - (0.3313 * g2) + (0.5000 * b2)) + 128
    cr = torch.trunc((0.5000 * r2) - (0.4187 * g2) - (0.0813 * b2)) + 128
    return tuple(t.to(torch.uint8).contiguous() for t in (y, cb, cr))


def time_legs(legs, rounds, iters):
    times = {name: [] for name in legs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(rounds + 1):                       # round 0 warms every leg up and is dropped
        for name, fn in legs.items():
            e0.record()
            for i in range(iters):
                fn(i)
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return times


def report(title, times, base_of):
    lines = [title, f"{'leg':44s} {'median us':>10s} {'min':>9s} {'max':>9s}  against its RGB sibling"]
    med = {n: statistics.median(t) for n, t in times.items()}
    for name, ts in times.items():
        base = base_of.get(name)
        rel = f"{(med[name] / med[base] - 1) * 100:+.1f} %" if base else ""
        lines.append(f"{name:44s} {med[name]:10.2f} {min(ts):9.2f} {max(ts):9.2f}  {rel}")
    return lines


def measure_shape(ctx, dev, W, H, n, ring, rounds, iters):
    """ring sets of n frames of W x H"""
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    rgb = [torch.randint(0, 256, (n, 3, H, W), dtype=torch.uint8, device=dev, generator=g) for _ in range(ring)]
    ycc = [ycc_of(t) for t in rgb]
    nv = [torch.stack((cb, cr), dim=-1).contiguous() for _, cb, cr in ycc]              # (n, CH, CW, 2)
    ncoef = J.coeff_count(W, H)
    co = [torch.empty(n * ncoef, dtype=torch.int16, device=dev) for _ in range(ring)]
    chk = torch.empty(n * ncoef, dtype=torch.int16, device=dev)

    def enc_rgb(k, out):
        t = rgb[k]
        ctx.fdct_quant_dev(t[:, 0], t[:, 1], t[:, 2], W, H, out, n_frames=n, plane_stride=3 * W * H)

    def sq(t):
        return t[0] if n == 1 else t

    def enc_i420(k, out):
        y, cb, cr = ycc[k]
        ctx.fdct_quant_ycc_dev(sq(y), sq(cb), sq(cr), out)

    def enc_nv12(k, out):
        ctx.fdct_quant_ycc_dev(sq(ycc[k][0]), sq(nv[k][..., 0]), sq(nv[k][..., 1]), out)

    for k in range(ring):
        enc_rgb(k, co[k])
    torch.cuda.synchronize()
    mc, mr = J.mcu_grid(W, H)
    for fn in (enc_i420, enc_nv12):
        fn(0, chk)
        torch.cuda.synchronize()
        a, b = chk.view(n, mr, mc, 6, 64), co[0].view(n, mr, mc, 6, 64)
        if W % 16 == 0 and H % 16 == 0:
            assert torch.equal(a, b), "YCC encode differs from the RGB encode"
        else:
            assert torch.equal(a[..., :4, :], b[..., :4, :]), "YCC encode: luma differs from the RGB encode"
    out_rgb = [torch.empty((n, 3, H, W), dtype=torch.uint8, device=dev) for _ in range(ring)]
    out_ycc = [tuple(torch.empty_like(t) for t in ycc[0]) for _ in range(ring)]
    out_nv = [torch.empty_like(nv[0]) for _ in range(ring)]

    def dec_rgb(k, gray=False):
        o = out_rgb[k]
        ctx.dequant_idct_dev(co[k], W, H, o[:, 0], o[:, 1], o[:, 2], gray=gray, n_frames=n, plane_stride=3 * W * H)

    def dec_i420(k):
        y, cb, cr = out_ycc[k]
        ctx.dequant_idct_ycc_dev(co[k], sq(y), sq(cb), sq(cr))

    def dec_nv12(k):
        ctx.dequant_idct_ycc_dev(co[k], sq(out_ycc[k][0]), sq(out_nv[k][..., 0]), sq(out_nv[k][..., 1]))

    dec_rgb(0, gray=True)
    dec_i420(0)
    dec_nv12(1 % ring)
    torch.cuda.synchronize()
    assert torch.equal(out_ycc[0][0], out_rgb[0][:, 0]), "YCC decode: Y differs from the gray RGB decode"
    if ring > 1:
        dec_i420(1)
        torch.cuda.synchronize()
        assert torch.equal(out_nv[1][..., 0], out_ycc[1][1]) and torch.equal(out_nv[1][..., 1], out_ycc[1][2]), "NV12 decode differs from I420"

    legs = {
        "encode RGB planes (fdct_quant_dev)": lambda i: enc_rgb(i % ring, co[i % ring]),
        "encode I420 (fdct_quant_ycc_dev)": lambda i: enc_i420(i % ring, chk),
        "encode NV12 (fdct_quant_ycc_dev)": lambda i: enc_nv12(i % ring, chk),
        "decode RGB planes (dequant_idct_dev)": lambda i: dec_rgb(i % ring),
        "decode I420 (dequant_idct_ycc_dev)": lambda i: dec_i420(i % ring),
        "decode NV12 (dequant_idct_ycc_dev)": lambda i: dec_nv12(i % ring),
    }
    base = {"encode I420 (fdct_quant_ycc_dev)": "encode RGB planes (fdct_quant_dev)", "encode NV12 (fdct_quant_ycc_dev)": "encode RGB planes (fdct_quant_dev)",
            "decode I420 (dequant_idct_ycc_dev)": "decode RGB planes (dequant_idct_dev)", "decode NV12 (dequant_idct_ycc_dev)": "decode RGB planes (dequant_idct_dev)"}
    times = time_legs(legs, rounds, iters)
    lines = report(f"{n} x {W}x{H} per launch, ring of {ring}, {rounds} interleaved rounds of {iters} launches per leg (us per launch)", times, base)
    return lines, (co[0][:ncoef].cpu().numpy() if n == 1 else None)


def measure_file(ctx, W, H, coeffs, rounds):
    jpg = J.write_jpeg(coeffs, W, H)
    legs = {"file -> host RGB planes (decode_jpeg)": lambda: ctx.decode_jpeg(jpg), "file -> host I420 planes (decode_jpeg_ycc)": lambda: ctx.decode_jpeg_ycc(jpg)}
    times = {name: [] for name in legs}
    for rnd in range(rounds + 1):
        for name, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e6)
    return report(f"one {W}x{H} file of {len(jpg)} bytes, host clock around the call, {rounds} alternated rounds (us per file)", times,
                  {"file -> host I420 planes (decode_jpeg_ycc)": "file -> host RGB planes (decode_jpeg)"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("measure_ycc: no HIP device (nothing here can be measured without one)")
    dev = torch.device("cuda:0")
    ctx = J.Context(0)
    lines = [f"measure_ycc on {torch.cuda.get_device_name(0)}"]
    l1, co = measure_shape(ctx, dev, 4096, 4096, 1, 6, args.rounds, args.iters)
    lines += l1 + [""]
    l2, _ = measure_shape(ctx, dev, 1920, 1080, 32, 2, args.rounds, max(2, args.iters // 4))
    lines += l2 + [""]
    lines += measure_file(ctx, 4096, 4096, co, args.rounds)
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
