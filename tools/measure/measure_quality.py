#!/usr/bin/env python3
"""What the quality setting (jpezy_ctx_set_quality) costs the encode kernel, and what it does to the file.

Two 4096 x 4096 pictures, resident in device memory: random pixels (the benchmark's workload) and the photo-like picture of
tools/measure/bench_content.py (smooth gradients + mild noise).  For quality 10, 50, 90 and 100:

  time       fdct_quant_dev of the frame, HIP events, K launches per round; the qualities take turns inside every round (interleaved),
             median / min / max over the rounds.  (A change of quality waits for the device: outside the timed brackets.)
  fallback   coefficients resolved through the exact paths (jpezy_ctx_last_fallback_count) per quad of the frame
  evaluator  an upper bound on how often the queue-overflow evaluator ran.  The counter cannot tell its runs from queued resolves (a run
             adds the quad's 1536 coefficients, a quad without one at most the queue's capacity of 382), so the frame is encoded once
             more in bands of one MCU row (64 quads) and every band contributes floor(count / 1536): 0 means it provably never ran.
  size       the file (encode_jpeg, Annex-K Huffman tables) beside Pillow's at the same quality and 4:2:0 -- for orientation only:
             libjpeg averages the chroma of a 2 x 2, this encoder takes its top-left pixel, and the transforms round differently.

Nothing here is an acceptance bound: high quality is expected to be slower (fewer zero coefficients, wider guard bands).

    python tools/measure/measure_quality.py [--rounds 7] [--iters 10] [--size 4096] [--out FILE]
"""
import argparse
import io
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import jpezy_amd as J  # noqa: E402

QUALITIES = (10, 50, 90, 100)


def pictures(W, H):
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    yield "random", [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3)]
    base = 128 + 90 * np.sin(xx / 97.0) * np.cos(yy / 61.0)
    yield "smooth+noise", [np.clip(base * s + rng.normal(0, 3, (H, W)), 0, 255).astype(np.uint8) for s in (1.0, 0.9, 0.8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    W = H = args.size
    assert W % 64 == 0
    quads = (W // 64) * (H // 16)
    dev = torch.device("cuda:0")
    ctx = J.Context(0)
    lines = [f"measure_quality: {W}x{H}, {args.rounds} interleaved rounds of {args.iters} launches per quality, {torch.cuda.get_device_name(0)}",
             f"{'picture':14s} {'quality':>7s} {'median us':>10s} {'min':>8s} {'max':>8s} {'vs q50':>7s} {'fallback/quad':>14s} {'evaluator<=':>11s} "
             f"{'file bytes':>11s} {'Pillow':>11s}"]
    try:
        from PIL import Image
    except ImportError:
        Image = None
    for name, planes in pictures(W, H):
        d = [torch.from_numpy(p).to(dev) for p in planes]
        co = torch.empty(J.coeff_count(W, H), dtype=torch.int16, device=dev)
        band = torch.empty(J.coeff_count(W, 16), dtype=torch.int16, device=dev)
        times = {q: [] for q in QUALITIES}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for rnd in range(args.rounds + 1):              # round 0 warms up and is dropped
            for q in QUALITIES:
                ctx.set_quality(q)
                e0.record()
                for _ in range(args.iters):
                    ctx.fdct_quant_dev(d[0], d[1], d[2], W, H, co)
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    times[q].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        base = statistics.median(times[50])
        for q in QUALITIES:
            ctx.set_quality(q)
            ctx.fallback_count()
            ctx.fdct_quant_dev(d[0], d[1], d[2], W, H, co)
            fb = ctx.fallback_count()
            evaluator = 0
            for y in range(0, H, 16):
                ctx.fdct_quant_dev(d[0][y:y + 16], d[1][y:y + 16], d[2][y:y + 16], W, 16, band)
                evaluator += ctx.fallback_count() // 1536
            size = len(ctx.encode_jpeg(planes[0], planes[1], planes[2], W, H))
            pil = -1
            if Image is not None:
                buf = io.BytesIO()
                Image.fromarray(np.stack(planes, axis=-1)).save(buf, "JPEG", quality=q, subsampling="4:2:0")
                pil = len(buf.getvalue())
            med = statistics.median(times[q])
            lines.append(f"{name:14s} {q:7d} {med:10.2f} {min(times[q]):8.2f} {max(times[q]):8.2f} {med / base:7.3f} {fb / quads:14.3f} {evaluator:11d} "
                         f"{size:11d} {pil:11d}")
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
