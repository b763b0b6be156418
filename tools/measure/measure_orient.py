#!/usr/bin/env python3
"""Oriented output (include/jpezy_hip_orientation.h): what the property costs, and that it costs nothing where it is off.

  Workloads   windows    measure_windows.py's mixed workload: N own-layout files, 320..800 x 240..600, one 224..448 px window each, scale 1
              resized    measure_windows_resized.py's: the same files, a random-resized-crop rectangle each, to 224 x 224, bilinear
              file       one 1920 x 1080 own-layout file, whole picture to host planes
  Arms        off        the setting at its default (mode 0), untagged files
              parent     the same call through ANOTHER build of the library (--parent-lib: the parent commit's), its own context
              tag 1/3/6  the setting on (mode 1), every file tagged 1 (un-oriented instances), 3 (mirrored), 6 (transposed); a file's window
                         is the SAME source rectangle in every arm, named in the oriented picture's coordinates, so every arm decodes the
                         same MCUs
              file       jpezy_decode_jpeg (the fused kernel) against jpezy_decode_jpeg_oriented with orientation 1, 3 and 6

One process, every arm warmed up, then the arms alternated round by round; a host clock around calls that end in a device synchronise;
median, minimum, maximum per arm, and the ratios to `off`.  --check compares bytes first: parent == off, and every tagged arm against the
permutation of off's windows.  Prints one line per arm and one JSON line (milliseconds)."""
import argparse
import ctypes as C
import json
import struct
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
import jpezy_amd as J  # noqa: E402
from jpezy_amd import api  # noqa: E402
from measure_windows import encode  # noqa: E402
from measure_windows_resized import OUT, source_rect  # noqa: E402

INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}


def tagged(jpg, o):
    """an APP1 with the one-entry IFD0 behind SOI"""
    tiff = b"II" + struct.pack("<HI", 42, 8) + struct.pack("<H", 1) + struct.pack("<HHIHH", 0x0112, 3, 1, o, 0) + struct.pack("<I", 0)
    body = b"Exif\0\0" + tiff
    return jpg[:2] + b"\xff\xe1" + struct.pack(">H", len(body) + 2) + body + jpg[2:]


def orient_np(P, o):
    return {1: lambda: P, 3: lambda: P[::-1, ::-1], 6: lambda: np.rot90(P, -1)}[o]()


class Batch:
    """n files and one window (rect, scale) each, as ctypes arrays"""

    def __init__(self, files, wins):
        self.n = len(files)
        self.arrs = [np.frombuffer(f, dtype=np.uint8) for f in files]
        self.data = (C.c_void_p * self.n)(*[a.ctypes.data for a in self.arrs])
        self.lens = (C.c_size_t * self.n)(*[a.size for a in self.arrs])
        self.wins = wins
        self.cwins = (api.Window * self.n)(*[api.Window(api.Rect(*r), s) for r, s in wins])
        self.infos, self.placed, self.status = (api.FrameInfo * self.n)(), (api.Rect * self.n)(), (C.c_int * self.n)()


def oriented_batch(files, sizes, wins, o):
    """every file tagged o, every window the same source rectangle seen in the oriented picture"""
    out = []
    for (W, H), (r, s) in zip(sizes, wins):
        Ws, Hs = J.scaled_size(W, H, s)
        out.append((J.orient_rect(INVERSE[o], *J.orient_size(o, Ws, Hs), r), s))
    return Batch([tagged(f, o) for f in files], out)


def bind(path):
    lib = C.CDLL(str(path))
    for name, res, args in api.ABI:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


def rounds_of(arms, rounds, warmup):
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t = time.perf_counter()
            fn()
            times[k].append((time.perf_counter() - t) * 1e3)
    return times


def report(name, times, base):
    res = {}
    b = float(np.median(times[base]))
    for k, v in times.items():
        res[k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "rounds": len(v),
                  "ratio_to_" + base: float(np.median(v)) / b}
        print(f"{name}, {k}: median {np.median(v):.3f} ms, min {np.min(v):.3f}, max {np.max(v):.3f}, x{np.median(v) / b:.3f} of '{base}'")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libjpezy_hip.so of the parent commit: an arm of its own")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    ctx = J.Context(0)
    lib = api.load_library()
    dev = torch.device("cuda", 0)
    n = a.files
    rng = np.random.default_rng(17)
    sizes = [(int(rng.integers(320, 801)), int(rng.integers(240, 601))) for _ in range(n)]
    files = [encode(ctx, W, H, 1000 + k) for k, (W, H) in enumerate(sizes)]
    crop = []
    for W, H in sizes:
        w, h = int(rng.integers(224, min(448, W) + 1)), int(rng.integers(224, min(448, H) + 1))
        crop.append(((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h), 1))
    rrc = [api.resize_pick_window(W, H, source_rect(rng, W, H), OUT, OUT) for W, H in sizes]
    mirror = (C.c_uint8 * n)(*[int(rng.integers(0, 2)) for _ in range(n)])
    parent = bind(a.parent_lib) if a.parent_lib else None
    parent_ctx = parent.jpezy_ctx_create(0) if parent else None
    assert parent is None or parent_ctx, "the parent library's context"
    result = {"files": n, "rounds": a.rounds}

    for name, wins, resized in (("windows", crop, False), ("resized", rrc, True)):
        batches = {"off": Batch(files, wins)}
        if parent:
            batches["parent"] = batches["off"]
        for o in (1, 3, 6):
            batches[f"tag {o}"] = oriented_batch(files, sizes, wins, o)
        S = max(max(r[2], r[3]) for r, _ in wins)                     # a slot holds a window in either orientation
        shape = (n, OUT, OUT, 3) if resized else (n, S, S, 3)
        outs = {k: torch.zeros(shape, dtype=torch.uint8, device=dev) for k in batches}

        def arm(k):
            b, d = batches[k], outs[k]
            L, h = (parent, parent_ctx) if k == "parent" else (lib, ctx._h)
            mode = 0 if k in ("off", "parent") else 1

            def fn():
                if L is lib:
                    assert lib.jpezy_ctx_set_windows_orientation(h, mode) == 0
                if resized:
                    rc = L.jpezy_decode_windows_resized_dev(h, n, b.data, b.lens, 0, b.cwins, mirror, OUT, OUT, J.PIX_RGB24, 0, 0, d.data_ptr(), d.numel(),
                                                            b.infos, b.placed, b.status)
                else:
                    rc = L.jpezy_decode_windows_dev(h, n, b.data, b.lens, 0, b.cwins, J.PIX_RGB24, S * 3, S * S * 3, d.data_ptr(), d.numel(), b.infos, b.placed,
                                                    b.status)
                assert rc == 0, L.jpezy_hip_last_error()
            return fn
        arms = {k: arm(k) for k in batches}
        if a.check:
            for fn in arms.values():
                fn()
            torch.cuda.synchronize()
            assert parent is None or torch.equal(outs["parent"], outs["off"]), "the parent's bytes"
            assert torch.equal(outs["tag 1"], outs["off"])
            if not resized:
                off = outs["off"].cpu().numpy()
                for o in (3, 6):
                    got = outs[f"tag {o}"].cpu().numpy()
                    for k, (r, _) in enumerate(wins):
                        O = orient_np(off[k, :r[3], :r[2]], o)
                        assert np.array_equal(got[k, :O.shape[0], :O.shape[1]], O), (o, k)
            print(f"{name}: bytes checked")
        result[name] = report(name, rounds_of(arms, a.rounds, a.warmup), "off")
    lib.jpezy_ctx_set_windows_orientation(ctx._h, 0)

    # one whole picture to the host: the fused kernel against the region stage, un-oriented and oriented
    W, H = 1920, 1080
    big = np.frombuffer(encode(ctx, W, H, 5000), dtype=np.uint8)
    planes = [np.zeros(W * H, dtype=np.uint8) for _ in range(3)]
    p = lambda x: x.ctypes.data_as(C.c_void_p)                         # noqa: E731
    fi, used = api.FrameInfo(), C.c_int(0)

    def whole(o):
        def fn():
            if o is None:
                rc = lib.jpezy_decode_jpeg(ctx._h, p(big), big.size, 0, C.byref(fi), p(planes[0]), p(planes[1]), p(planes[2]), W * H)
            else:
                rc = lib.jpezy_decode_jpeg_oriented(ctx._h, p(big), big.size, 0, 0, 1, None, o, C.byref(used), C.byref(fi), p(planes[0]), p(planes[1]),
                                                    p(planes[2]), W * H)
            assert rc == 0, lib.jpezy_hip_last_error()
        return fn
    arms = {"decode_jpeg": whole(None), "oriented 1": whole(1), "oriented 3": whole(3), "oriented 6": whole(6)}
    result["file 1920x1080"] = report("file 1920x1080", rounds_of(arms, a.rounds, a.warmup), "decode_jpeg")
    if parent:
        parent.jpezy_ctx_destroy(parent_ctx)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
