#!/usr/bin/env python3
"""Lossless transforms (include/jpezy_hip.h, LOSSLESS TRANSFORMS), measured in one process:

  (a) kernel       jpezy_coeff_transform_dev on one 4096 x 4096 4:2:0 coefficient field resident in HBM (50.3 MB read, 50.3 MB written),
                   every operation, against a device-to-device hipMemcpyAsync of the same buffer: device events around one call, every arm
                   warmed up, the arms alternated round by round; median and minimum, and the rate (bytes read + bytes written over time)
  (b) end to end   .jpg bytes on the host -> transformed .jpg bytes on the host, same file: jpezy_transform_jpeg against the pixel route
                   (jpezy_decode_jpeg, the numpy operation on the three planes, jpezy_encode_jpeg), host clock, same alternation

--check compares every operation's kernel output with the numpy model of tests/transform_model.py first.  Prints one line per arm and a
JSON line with every figure (times in microseconds)."""
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

NAMES = ["none", "hflip", "vflip", "transpose", "transverse", "rot90", "rot180", "rot270"]


def picture(W, H, seed=5):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.clip((np.sin(xx / 37.0) * 60 + np.cos(yy / 23.0) * 50 + 128)[..., None] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)


def numpy_op(plane, op):
    return [plane, plane[:, ::-1], plane[::-1], plane.T, plane[::-1, ::-1].T, np.rot90(plane, -1), plane[::-1, ::-1], np.rot90(plane, 1)][op]


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
    ap.add_argument("--e2e-rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    assert a.rounds >= 20 and a.e2e_rounds >= 20, "medians of at least 20 repetitions"
    W = H = a.size
    assert W % 16 == 0
    ctx = J.Context(0)
    dev = torch.device("cuda", 0)
    lib = api.load_library()
    img = picture(W, H)
    planes = [np.ascontiguousarray(img[..., k]).reshape(-1) for k in range(3)]
    data = ctx.encode_jpeg(*planes, W, H)
    info, d_in = ctx.read_jpeg_gpu(data)
    d_in = d_in.reshape(-1)
    n = d_in.numel()
    d_out = torch.empty(n, dtype=torch.int16, device=dev)
    result = {"size": [W, H], "rounds": a.rounds, "field_bytes": 2 * n, "jpg_bytes": len(data)}

    if a.check:
        sys.path.insert(0, str(ROOT / "tests"))
        import transform_model as M
        co = d_in.cpu().numpy().reshape(-1, 6, 64)
        for op in range(8):
            ctx.coeff_transform_dev(d_in, W, H, d_out, op)
            torch.cuda.synchronize()
            ok = np.array_equal(d_out.cpu().numpy().reshape(-1, 6, 64), M.transform_field(co, W, H, M.S420, op)[0])
            print(f"{NAMES[op]}: the kernel's field equals the model's: {ok}")
            assert ok

    # ---- (a) the kernel against the device's own copy ----
    stream = torch.cuda.current_stream(dev).cuda_stream
    # the HIP runtime this process already holds (torch's; a second copy of the library would not see the device)
    loaded = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln]
    assert loaded, "no HIP runtime is loaded"
    hip = C.CDLL(loaded[0])
    hip.hipMemcpyAsync.restype = C.c_int
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    def copy():
        assert hip.hipMemcpyAsync(d_out.data_ptr(), d_in.data_ptr(), 2 * n, 3, stream) == 0        # 3: hipMemcpyDeviceToDevice

    arms = {"hipMemcpyAsync (device to device)": copy}
    for op in range(8):
        arms[f"kernel {NAMES[op]}"] = lambda op=op: ctx.coeff_transform_dev(d_in, W, H, d_out, op)
    t = timed_rounds(arms, a.rounds, a.warmup, device_events=True)
    result["kernel"] = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "TB_per_s": 4 * n / float(np.median(v)) / 1e6} for k, v in t.items()}
    for k, v in t.items():
        print(f"{W}x{H} 4:2:0 field ({2 * n / 1e6:.1f} MB in, {2 * n / 1e6:.1f} MB out), {k}: median {np.median(v):.1f} us, min {np.min(v):.1f} us, "
              f"{4 * n / np.median(v) / 1e6:.2f} TB/s read + written")

    # ---- (b) end to end against the pixel route ----
    arr = np.frombuffer(data, dtype=np.uint8)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    cap = J.jpeg_bound(W, H)
    out = np.zeros(cap, dtype=np.uint8)
    host = [np.zeros(W * H, dtype=np.uint8) for _ in range(3)]
    fi = api.FrameInfo()
    sizes = {}

    def coefficient_route(op):
        rc = lib.jpezy_transform_jpeg(ctx._h, vp(arr), arr.size, op, 0, None, C.byref(fi), vp(out), cap)
        assert rc > 0, lib.jpezy_hip_last_error()
        sizes[f"transform_jpeg {NAMES[op]}"] = rc

    def pixel_route(op):
        rc = lib.jpezy_decode_jpeg(ctx._h, vp(arr), arr.size, 0, C.byref(fi), vp(host[0]), vp(host[1]), vp(host[2]), W * H)
        assert rc == 0, lib.jpezy_hip_last_error()
        turned = [np.ascontiguousarray(numpy_op(p.reshape(H, W), op)) for p in host]
        ho, wo = turned[0].shape
        rc = lib.jpezy_encode_jpeg(ctx._h, vp(turned[0]), vp(turned[1]), vp(turned[2]), wo, ho, 0, b"Encoded by jpezy", vp(out), cap)
        assert rc > 0, lib.jpezy_hip_last_error()
        sizes[f"decode + numpy + encode {NAMES[op]}"] = rc

    arms = {}
    for op in (0, 1, 5, 6):
        arms[f"transform_jpeg {NAMES[op]}"] = lambda op=op: coefficient_route(op)
        arms[f"decode + numpy + encode {NAMES[op]}"] = lambda op=op: pixel_route(op)
    t = timed_rounds(arms, a.e2e_rounds, a.warmup, device_events=False)
    result["end_to_end"] = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "bytes_out": int(sizes[k])} for k, v in t.items()}
    result["huffman_decoder"] = "GPU" if ctx.last_huffdec_passes() > 0 else "host"
    for k, v in t.items():
        print(f"{W}x{H} ({len(data) / 1e6:.2f} MB .jpg), end to end, {k}: median {np.median(v) / 1e3:.3f} ms, min {np.min(v) / 1e3:.3f} ms, {sizes[k]} bytes out")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
