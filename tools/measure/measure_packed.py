#!/usr/bin/env python3
"""What the packed (interleaved) pixel boundary costs, and what it saves a caller whose pixels are interleaved.

One 4096 x 4096 random-pixel frame set (a ring of 6 frames, as bench.py uses), everything resident in device memory.  Legs, run in
interleaved rounds on one device and timed with HIP events (K launches per round and leg; median over the rounds, min and max printed):

  encode  (a) planar fdct_quant_dev
          (b) fdct_quant_packed_dev, RGB24 and RGBA32
          (c) what such a caller does without (b): img.permute(2, 0, 1).contiguous() on the device, then (a)
  decode  (a) planar dequant_idct_dev   (b) dequant_idct_packed_dev, RGB24 and RGBA32   (c) (a), then torch.stack(planes, dim=-1)

Acceptance: (b) is faster than (c) and (b)'s slowest round is below (c)'s fastest -- (c) moves about twice the bytes, so anything else
means the new load or store stage is broken.  (b) - (a) is reported as the cost of the boundary.

    python tools/measure/measure_packed.py [--rounds 7] [--iters 20] [--size 4096] [--out FILE]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import jpezy_amd as J  # noqa: E402

RING = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 5
    W = H = args.size
    dev = torch.device("cuda:0")
    ctx = J.Context(0)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    rgb = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(RING)]
    rgba = [torch.cat([t, torch.zeros((H, W, 1), dtype=torch.uint8, device=dev)], dim=-1).contiguous() for t in rgb]
    planar = [t.permute(2, 0, 1).contiguous() for t in rgb]
    ncoef = J.coeff_count(W, H)
    co = [torch.empty(ncoef, dtype=torch.int16, device=dev) for _ in range(RING)]
    for k in range(RING):
        ctx.fdct_quant_dev(planar[k][0], planar[k][1], planar[k][2], W, H, co[k])
    torch.cuda.synchronize()
    # the packed encoders agree with the planar one before anything is timed
    chk = torch.empty(ncoef, dtype=torch.int16, device=dev)
    for fmt, ring in ((J.PIX_RGB24, rgb), (J.PIX_RGBA32, rgba)):
        ctx.fdct_quant_packed_dev(ring[0], chk, format=fmt)
        torch.cuda.synchronize()
        assert torch.equal(chk, co[0]), "packed encode differs from planar"
    out_planes = [torch.empty((3, H, W), dtype=torch.uint8, device=dev) for _ in range(RING)]
    out_rgb = [torch.empty((H, W, 3), dtype=torch.uint8, device=dev) for _ in range(RING)]
    out_rgba = [torch.empty((H, W, 4), dtype=torch.uint8, device=dev) for _ in range(RING)]
    ctx.dequant_idct_dev(co[0], W, H, out_planes[0][0], out_planes[0][1], out_planes[0][2])
    ctx.dequant_idct_packed_dev(co[0], out_rgb[0], format=J.PIX_RGB24)
    ctx.dequant_idct_packed_dev(co[0], out_rgba[0], format=J.PIX_RGBA32)
    torch.cuda.synchronize()
    assert torch.equal(out_rgb[0], out_planes[0].permute(1, 2, 0)), "packed decode differs from planar"
    assert torch.equal(out_rgba[0][:, :, :3], out_rgb[0]) and bool((out_rgba[0][:, :, 3] == 255).all())

    def enc_planar(k):
        p = planar[k]
        ctx.fdct_quant_dev(p[0], p[1], p[2], W, H, co[k])

    def enc_today(k):
        p = rgb[k].permute(2, 0, 1).contiguous()
        ctx.fdct_quant_dev(p[0], p[1], p[2], W, H, co[k])

    def dec_planar(k):
        o = out_planes[k]
        ctx.dequant_idct_dev(co[k], W, H, o[0], o[1], o[2])

    def dec_today(k):
        o = out_planes[k]
        ctx.dequant_idct_dev(co[k], W, H, o[0], o[1], o[2])
        torch.stack((o[0], o[1], o[2]), dim=-1)

    legs = {
        "encode (a) planar": enc_planar,
        "encode (b) packed RGB24": lambda k: ctx.fdct_quant_packed_dev(rgb[k], co[k], format=J.PIX_RGB24),
        "encode (b) packed RGBA32": lambda k: ctx.fdct_quant_packed_dev(rgba[k], co[k], format=J.PIX_RGBA32),
        "encode (c) permute+contiguous, planar": enc_today,
        "decode (a) planar": dec_planar,
        "decode (b) packed RGB24": lambda k: ctx.dequant_idct_packed_dev(co[k], out_rgb[k], format=J.PIX_RGB24),
        "decode (b) packed RGBA32": lambda k: ctx.dequant_idct_packed_dev(co[k], out_rgba[k], format=J.PIX_RGBA32),
        "decode (c) planar, torch.stack": dec_today,
    }
    times = {name: [] for name in legs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(args.rounds + 1):                  # round 0 warms up (allocator, code objects) and is dropped
        for name, fn in legs.items():
            e0.record()
            for i in range(args.iters):
                fn(i % RING)
            e1.record()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)
    lines = [f"measure_packed: {W}x{H}, ring of {RING} frames, {args.rounds} interleaved rounds of {args.iters} launches per leg, "
             f"{torch.cuda.get_device_name(0)}", f"{'leg':42s} {'median us':>10s} {'min':>8s} {'max':>8s}"]
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        lines.append(f"{name:42s} {med[name]:10.2f} {min(ts):8.2f} {max(ts):8.2f}")
    ok = True
    for d, today in (("encode", "encode (c) permute+contiguous, planar"), ("decode", "decode (c) planar, torch.stack")):
        a = med[f"{d} (a) planar"]
        for fmt in ("RGB24", "RGBA32"):
            b = f"{d} (b) packed {fmt}"
            good = med[b] < med[today] and max(times[b]) < min(times[today])
            ok = ok and good
            lines.append(f"{d} {fmt}: packed boundary (b) - (a) = {med[b] - a:+.2f} us ({(med[b] / a - 1) * 100:+.1f} %); "
                         f"(b) {med[b]:.2f} us against (c) {med[today]:.2f} us, slowest (b) {max(times[b]):.2f} "
                         f"{'<' if max(times[b]) < min(times[today]) else '>='} fastest (c) {min(times[today]):.2f}: {'ok' if good else 'FAILED'}")
    lines.append("acceptance (b) < (c) in both directions: " + ("met" if ok else "NOT met"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
