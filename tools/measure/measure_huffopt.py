#!/usr/bin/env python3
"""Per-image optimised Huffman tables: what the option costs and gains on one 4096x4096 frame, noise and smooth.

    measure_huffopt.py            wall time of jpezy_write_jpeg_gpu and file size with the setting off and on, interleaved rounds
    measure_huffopt.py --trace    a few calls with the setting on and off and nothing else: run it under
                                  `rocprofv3 --kernel-trace --stats` to read symbol_histogram_kernel beside code_tiles_kernel
                                  (tools/measure/measure_huffopt.sh does both and A/Bs code_tiles_kernel against ab/libjpezy_*.so)
"""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import jpezy_amd as J  # noqa: E402
from jpezy_amd import api  # noqa: E402

W = H = 4096
# A/B against an older build (JPEZY_LIB=ab/libjpezy_<name>.so) that does not have the option yet: bind what it exports, and
# --trace then runs the default path only
api.ABI = [e for e in api.ABI if hasattr(C.CDLL(str(J.library_path())), e[0])] if J.library_path().exists() else api.ABI
HAVE_OPT = any(e[0] == "jpezy_ctx_set_huffman_optimize" for e in api.ABI)


def frames(ctx, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    noise = [torch.randint(0, 256, (W * H,), dtype=torch.uint8, device=dev, generator=g) for _ in range(3)]
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    base = ((xx * 3 + yy * 2) // 8 % 256).float()
    smooth = [(base.roll(k * 77, 1) + torch.randn((H, W), device=dev, generator=g) * 4).clamp(0, 255).to(torch.uint8).reshape(-1) for k in range(3)]
    out = {}
    for name, p in (("noise", noise), ("smooth", smooth)):
        co = torch.empty(J.coeff_count(W, H, False), dtype=torch.int16, device=dev)
        ctx.fdct_quant_dev(p[0], p[1], p[2], W, H, co)
        out[name] = co
    torch.cuda.synchronize()
    return out


def main():
    trace = "--trace" in sys.argv
    ctx = J.Context(0)
    dev = torch.device("cuda:0")
    lib = J.load_library()
    cos = frames(ctx, dev)
    cap = lib.jpezy_jpeg_bound(W, H)
    buf = np.zeros(cap, dtype=np.uint8)

    def call(co, on):
        if HAVE_OPT:
            ctx.set_huffman_optimize(on)
        n = lib.jpezy_write_jpeg_gpu(ctx._h, co.data_ptr(), W, H, 0, b"Encoded by jpezy", buf.ctypes.data_as(C.c_void_p), cap)
        assert n > 0
        return n

    if trace:
        for name in ("noise", "smooth"):
            for on in ((0, 1) if HAVE_OPT else (0,)):
                for _ in range(10):
                    call(cos[name], on)
        torch.cuda.synchronize()
        return
    for name, co in cos.items():
        size = {on: call(co, on) for on in (0, 1)}          # warm: scratch allocated for both
        host = co.cpu().numpy()
        assert bytes(buf[:size[1]]) == J.write_jpeg(host, W, H, optimize=True)
        t = {0: [], 1: []}
        for _ in range(15):
            for on in (0, 1):
                t0 = time.perf_counter()
                call(co, on)
                t[on].append(time.perf_counter() - t0)
        off, on_ = np.median(t[0]) * 1e6, np.median(t[1]) * 1e6
        print(f"{W}x{H} {name}: jpezy_write_jpeg_gpu off {off:.0f} us (min {min(t[0]) * 1e6:.0f}), on {on_:.0f} us (min {min(t[1]) * 1e6:.0f}): "
              f"+{on_ - off:.0f} us; file {size[0]} -> {size[1]} bytes ({100.0 * (size[0] - size[1]) / size[0]:.2f} % smaller)", flush=True)
        # the host's share of the option: four tables from the counts
        h, _ = np.zeros((4, 256), np.uint64), None
        hist = torch.zeros((1, 4, 256), dtype=torch.int64, device=dev)
        ctx.huffman_histogram_dev(co, W, H, hist)
        torch.cuda.synchronize()
        h = hist.cpu().numpy()[0].astype(np.uint64)
        t0 = time.perf_counter()
        for k in range(4):
            J.optimal_table(h[k])
        print(f"    four optimal tables on the host (through the Python wrapper): {(time.perf_counter() - t0) * 1e6:.0f} us; "
              f"symbols per table {[int(np.count_nonzero(h[k])) for k in range(4)]}", flush=True)


if __name__ == "__main__":
    main()
