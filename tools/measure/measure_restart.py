#!/usr/bin/env python3
"""Restart intervals from the GPU entropy coder: what they cost to write and what they gain to read, 4096x4096 colour.

    measure_restart.py [--parent ab/libjpezy_parent.so] [--calls 200]
    measure_restart.py --trace        a few calls per setting and nothing else, for `rocprofv3 --kernel-trace --stats`

1. jpezy_write_jpeg_gpu_dev on noise and on photo-like content (smooth + mild noise, tools/measure/bench_content.py), device events
   around every call, warmed, the legs alternated call by call in one process:
       parent A, parent B   the parent commit's library (a build of the commit this one follows, e.g. from a `git worktree` with
                            jpezy_amd/_build.py, copied to ab/libjpezy_parent.so), two contexts of it: their difference is the
                            spread a leg has against itself in this run
       Ri = 0               this build, no intervals; CONDITION: not slower than the parent by more than that spread
       Ri = 256, 16, 1      this build, one MCU row per interval, and what short intervals cost (recorded, not gated)
2. jpezy_read_jpeg_gpu of this encoder's own file at Ri = 0 and Ri = 256 (wall time, synchronised).

Seeded; no network, no reference; fails without a device."""
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import jpezy_amd as J  # noqa: E402

W = H = 4096
COMMENT = b"Encoded by jpezy"


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def contents(ctx, dev):
    """device coefficients of the two frames"""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = 128 + 90 * np.sin(xx / 97.0) * np.cos(yy / 61.0)
    photo = [np.clip(base * s + rng.normal(0, 3, (H, W)), 0, 255).astype(np.uint8) for s in (1.0, 0.9, 0.8)]
    noise = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3)]
    out = {}
    for name, planes in (("noise", noise), ("photo-like", photo)):
        d = [torch.from_numpy(p.reshape(-1)).to(dev) for p in planes]
        co = torch.empty(J.coeff_count(W, H, False), dtype=torch.int16, device=dev)
        ctx.fdct_quant_dev(d[0], d[1], d[2], W, H, co)
        out[name] = co
    torch.cuda.synchronize()
    return out


class Leg:
    """one context of one library and one restart setting"""

    def __init__(self, name, lib, ri, stride, dev):
        self.name, self.lib, self.ri = name, lib, ri
        self.h = lib.jpezy_ctx_create(0)
        assert self.h, name
        if ri:
            assert lib.jpezy_ctx_set_restart_interval(C.c_void_p(self.h), ri) == 0
        self.out = torch.zeros(stride, dtype=torch.uint8, device=dev)
        self.size = torch.zeros(1, dtype=torch.int64, device=dev)
        self.us = []

    def call(self, co):
        rc = self.lib.jpezy_write_jpeg_gpu_dev(C.c_void_p(self.h), C.c_void_p(co.data_ptr()), W, H, 0, 1, COMMENT,
                                               C.c_void_p(self.out.data_ptr()), C.c_size_t(self.out.numel()),
                                               C.c_void_p(self.size.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, (self.name, rc)

    def file(self):
        return self.out[:int(self.size[0])].cpu().numpy().tobytes()

    def close(self):
        self.lib.jpezy_ctx_destroy(C.c_void_p(self.h))


def bind_parent(path):
    lib = C.CDLL(str(path))
    lib.jpezy_ctx_create.restype = C.c_void_p
    lib.jpezy_ctx_create.argtypes = [C.c_int]
    lib.jpezy_ctx_destroy.argtypes = [C.c_void_p]
    lib.jpezy_write_jpeg_gpu_dev.restype = C.c_int
    return lib


def main():
    assert torch.cuda.is_available(), "measure_restart.py needs a HIP device"
    trace = "--trace" in sys.argv
    calls = int(arg("--calls", 200))
    parent_path = Path(arg("--parent", ROOT / "ab" / "libjpezy_parent.so"))
    dev = torch.device("cuda:0")
    ctx = J.Context(0)
    lib = J.load_library()
    lib.jpezy_ctx_create.restype = C.c_void_p
    cos = contents(ctx, dev)
    stride = lib.jpezy_jpeg_bound(W, H)
    legs = []
    if parent_path.exists() and not trace:
        parent = bind_parent(parent_path)
        legs += [Leg("parent A", parent, 0, stride, dev), Leg("parent B", parent, 0, stride, dev)]
    else:
        print(f"(no parent library at {parent_path}: the Ri = 0 condition is not evaluated)")
    legs += [Leg(f"Ri = {ri}", lib, ri, stride, dev) for ri in (0, 256, 16, 1)]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    files = {}
    for name, co in cos.items():
        for leg in legs:                         # warm: scratch, header upload
            for _ in range(3):
                leg.call(co)
            leg.us = []
        torch.cuda.synchronize()
        host = co.cpu().numpy()
        for leg in legs:                         # every leg writes the host writer's bytes
            want = J.write_jpeg(host, W, H, restart_interval=leg.ri)
            assert leg.file() == want, (name, leg.name)
            files[(name, leg.ri)] = want
        if trace:
            for leg in legs:
                for _ in range(10):
                    leg.call(co)
            torch.cuda.synchronize()
            continue
        for _ in range(calls):
            for leg in legs:
                e0.record()
                leg.call(co)
                e1.record()
                e1.synchronize()
                leg.us.append(e0.elapsed_time(e1) * 1e3)
        print(f"jpezy_write_jpeg_gpu_dev, {W}x{H} colour, {name}, {calls} calls per leg, legs alternated, device events (us):")
        med = {}
        for leg in legs:
            a = np.array(leg.us)
            med[leg.name] = float(np.median(a))
            print(f"    {leg.name:9s} median {np.median(a):8.1f}   min {a.min():8.1f}   p90 {np.percentile(a, 90):8.1f}   "
                  f"file {len(files[(name, leg.ri)])} bytes")
        if "parent A" in med:
            spread = abs(med["parent A"] - med["parent B"])
            slower = med["Ri = 0"] - min(med["parent A"], med["parent B"])
            verdict = "holds" if slower <= spread else "DOES NOT HOLD"
            print(f"    spread between the two parent legs {spread:.1f} us; Ri = 0 against the faster parent leg {slower:+.1f} us: the condition {verdict}")
        print(f"    Ri = 256 against Ri = 0: {med['Ri = 256'] - med['Ri = 0']:+.1f} us; Ri = 16: {med['Ri = 16'] - med['Ri = 0']:+.1f} us; "
              f"Ri = 1: {med['Ri = 1'] - med['Ri = 0']:+.1f} us", flush=True)
    for leg in legs:
        leg.close()
    if trace:
        return
    # 2. the project's own decoder on the project's own files
    ctx.set_huffdec_min_bytes(0)
    for name in cos:
        line = []
        for ri in (0, 256):
            arr = np.frombuffer(files[(name, ri)], dtype=np.uint8)
            d = torch.empty(J.coeff_count(W, H, False), dtype=torch.int16, device=dev)
            for _ in range(3):
                ctx.read_jpeg_gpu_into(arr, d)
            torch.cuda.synchronize()
            assert torch.equal(d, cos[name])
            t = []
            for _ in range(30):
                t0 = time.perf_counter()
                ctx.read_jpeg_gpu_into(arr, d)
                torch.cuda.synchronize()
                t.append((time.perf_counter() - t0) * 1e3)
            line.append(f"Ri = {ri}: median {np.median(t):.3f} ms, min {min(t):.3f} ms, passes {ctx.last_huffdec_passes()}")
        print(f"jpezy_read_jpeg_gpu, {W}x{H} colour, {name} ({len(files[(name, 0)])} bytes): " + "; ".join(line), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
