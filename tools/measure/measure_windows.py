#!/usr/bin/env python3
"""One crop window of each of many files into a device tensor: jpezy_decode_windows_dev against what the library offered before it, on
the same files, in one process, the arms alternated round by round after a warm-up of each.  A host clock around work that ends in a
device synchronise; median, minimum and spread (max - min) per arm.

  Workloads   mixed      N own-layout files (smooth picture + noise, as measure_region.py makes them), widths 320..800 and heights 240..600
                         from a fixed seed, one window of 224..448 px per file at scale 1
              mixed/2    the same files and window sizes at scale 2 where the window fits the half-size picture (scale 1 elsewhere)
              one size   N files of 1920 x 1080 (--distinct different pictures, repeated), a 224 x 224 window each
  Arms        A  jpezy_decode_windows_dev into a device tensor
              B  a loop of jpezy_decode_jpeg_region_packed into one stacked host array, then one upload
              C  jpezy_decode_jpeg_batch (whole pictures to the host), a numpy crop into the stacked array, then one upload (scale 1 only)
  Also        the JPEZY_BATCH_DEBUG laps of one call of A per workload (headers, Huffman chain, transform; the kernel's own time from
              device events) on stderr, and one whole-picture row: a 4096 x 4096 file through A against the fused kernel's device stage

--check compares the bytes of A with B's (and C's) at the measured sizes first.  Bare ctypes, buffers preallocated and touched.  Prints one
line per arm and a JSON line with every figure (times in milliseconds)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
import jpezy_amd as J  # noqa: E402
from jpezy_amd import api  # noqa: E402

vp = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731


def picture(W, H, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.clip((np.sin(xx / 37.0) * 60 + np.cos(yy / 23.0) * 50 + 128)[..., None] + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)


def encode(ctx, W, H, seed):
    img = picture(W, H, seed)
    return ctx.encode_jpeg(*[np.ascontiguousarray(img[..., k]).reshape(-1) for k in range(3)], W, H)


class Workload:
    """files (bytes), sizes, windows [(x, y, w, h, scale)], the slot Hs x Ws"""

    def __init__(self, name, files, sizes, wins, Hs, Ws):
        self.name, self.files, self.sizes, self.wins, self.Hs, self.Ws = name, files, sizes, wins, Hs, Ws
        self.n = len(files)
        self.arrs = [np.frombuffer(f, dtype=np.uint8) for f in files]
        self.data = (C.c_void_p * self.n)(*[a.ctypes.data for a in self.arrs])
        self.lens = (C.c_size_t * self.n)(*[a.size for a in self.arrs])
        self.cwins = (api.Window * self.n)(*[api.Window(api.Rect(x, y, w, h), s) for x, y, w, h, s in wins])
        self.rects = [api.Rect(x, y, w, h) for x, y, w, h, s in wins]
        self.infos, self.placed, self.status = (api.FrameInfo * self.n)(), (api.Rect * self.n)(), (C.c_int * self.n)()


def make_arms(lib, ctx, wl, dev):
    n, Hs, Ws = wl.n, wl.Hs, wl.Ws
    row, slot = Ws * 3, Hs * Ws * 3
    d_a = torch.zeros((n, Hs, Ws, 3), dtype=torch.uint8, device=dev)
    d_b = torch.zeros((n, Hs, Ws, 3), dtype=torch.uint8, device=dev)
    host = torch.zeros((n, Hs, Ws, 3), dtype=torch.uint8)
    h_np = host.numpy()
    fi = api.FrameInfo()

    def arm_a():
        rc = lib.jpezy_decode_windows_dev(ctx._h, n, wl.data, wl.lens, 0, wl.cwins, J.PIX_RGB24, row, slot, d_a.data_ptr(), n * slot, wl.infos, wl.placed, wl.status)
        assert rc == 0, lib.jpezy_hip_last_error()

    def arm_b():
        for k in range(n):
            rc = lib.jpezy_decode_jpeg_region_packed(ctx._h, vp(wl.arrs[k]), wl.arrs[k].size, 0, wl.wins[k][4], C.byref(wl.rects[k]), C.byref(fi), J.PIX_RGB24,
                                                     row, C.c_void_p(h_np[k].ctypes.data), slot)
            assert rc == 0, lib.jpezy_hip_last_error()
        d_b.copy_(host)
        torch.cuda.synchronize()

    arms = {"A decode_windows_dev": arm_a, "B region_packed loop + upload": arm_b}
    d_c = None
    if all(w[4] == 1 for w in wl.wins):
        d_c = torch.zeros((n, Hs, Ws, 3), dtype=torch.uint8, device=dev)
        host_c = torch.zeros((n, Hs, Ws, 3), dtype=torch.uint8)
        hc = host_c.numpy()
        planes = [[np.zeros(W * H, dtype=np.uint8) for _ in range(3)] for W, H in wl.sizes]
        ptrs = [(C.c_void_p * n)(*[p[q].ctypes.data for p in planes]) for q in range(3)]
        caps = (C.c_size_t * n)(*[W * H for W, H in wl.sizes])
        infos, status = (api.FrameInfo * n)(), (C.c_int * n)()

        def arm_c():
            rc = lib.jpezy_decode_jpeg_batch(ctx._h, n, wl.data, wl.lens, 0, infos, ptrs[0], ptrs[1], ptrs[2], caps, status)
            assert rc == 0, lib.jpezy_hip_last_error()
            for k in range(n):
                x, y, w, h, _ = wl.wins[k]
                W, H = wl.sizes[k]
                for q in range(3):
                    hc[k, :h, :w, q] = planes[k][q].reshape(H, W)[y:y + h, x:x + w]
            d_c.copy_(host_c)
            torch.cuda.synchronize()

        arms["C decode_jpeg_batch + crop + upload"] = arm_c
    return arms, d_a, d_b, d_c


def timed_rounds(arms, rounds, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=16, help="different 1920 x 1080 pictures of the one-size workload")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--rounds-one-size", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--whole", type=int, default=4096, help="edge of the whole-picture row; 0: skip")
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    ctx = J.Context(0)
    lib = api.load_library()
    dev = torch.device("cuda", 0)
    n = a.files
    rng = np.random.default_rng(17)
    sizes = [(int(rng.integers(320, 801)), int(rng.integers(240, 601))) for _ in range(n)]
    files = [encode(ctx, W, H, 1000 + k) for k, (W, H) in enumerate(sizes)]
    wins1, wins2 = [], []
    for W, H in sizes:
        w, h = int(rng.integers(224, min(448, W) + 1)), int(rng.integers(224, min(448, H) + 1))
        x, y = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        wins1.append((x, y, w, h, 1))
        ws, hs = J.scaled_size(W, H, 2)
        wins2.append((int(rng.integers(0, ws - w + 1)), int(rng.integers(0, hs - h + 1)), w, h, 2) if w <= ws and h <= hs else (x, y, w, h, 1))
    big = [encode(ctx, 1920, 1080, 5000 + k) for k in range(a.distinct)]
    one_files = [big[k % a.distinct] for k in range(n)]
    one_wins = [(int(rng.integers(0, 1920 - 224 + 1)), int(rng.integers(0, 1080 - 224 + 1)), 224, 224, 1) for _ in range(n)]
    workloads = [(Workload("mixed sizes, scale 1", files, sizes, wins1, 448, 448), a.rounds),
                 (Workload("mixed sizes, scale 2 where the window allows", files, sizes, wins2, 448, 448), a.rounds),
                 (Workload("one size (1920 x 1080), 224^2 windows", one_files, [(1920, 1080)] * n, one_wins, 224, 224), a.rounds_one_size)]
    result = {"files": n, "workloads": {}}
    for wl, rounds in workloads:
        arms, d_a, d_b, d_c = make_arms(lib, ctx, wl, dev)
        if a.check:
            for fn in arms.values():
                fn()
            ok = bool(torch.equal(d_a, d_b)) and (d_c is None or bool(torch.equal(d_a, d_c)))
            print(f"{wl.name}: A's bytes equal B's{'' if d_c is None else ' and C s'}: {ok}")
            assert ok
        t = timed_rounds(arms, rounds, a.warmup)
        res = {"scale2_files": sum(1 for w in wl.wins if w[4] == 2), "arms": {}}
        for k, v in t.items():
            res["arms"][k] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "rounds": len(v)}
            print(f"{wl.name} ({wl.n} files), {k}: median {np.median(v):.2f} ms, min {np.min(v):.2f} ms, spread {np.max(v) - np.min(v):.2f} ms")
        am = res["arms"]["A decode_windows_dev"]["median_ms"]
        holds = True
        for k, r in res["arms"].items():
            if k.startswith("A "):
                continue
            margin = r["median_ms"] - am
            spread = r["max_ms"] - r["min_ms"]
            holds = holds and margin > spread
            print(f"{wl.name}: A is {margin:.2f} ms below '{k}' (that arm's spread: {spread:.2f} ms): {'holds' if margin > spread else 'DOES NOT HOLD'}")
        res["a_below_others_by_more_than_their_spread"] = holds
        result["workloads"][wl.name] = res
        # the laps of one call of A (stderr)
        sys.stderr.write(f"laps of one call of A, {wl.name}:\n")
        sys.stderr.flush()
        os.environ["JPEZY_BATCH_DEBUG"] = "1"
        arms["A decode_windows_dev"]()
        del os.environ["JPEZY_BATCH_DEBUG"]
        res["grouped_files"] = int(lib.jpezy_ctx_last_batch_fast_count(ctx._h))       # of that call of A
        print(f"{wl.name}: {res['grouped_files']} of {wl.n} files took A's grouped path, {res['scale2_files']} windows at scale 2")
    if a.whole:
        # whole pictures run at the region kernel's rate: one row, against the fused kernel's device stage on the same coefficients
        E = a.whole
        f = encode(ctx, E, E, 77)
        wl = Workload(f"whole picture {E}^2", [f], [(E, E)], [(0, 0, 0, 0, 1)], E, E)
        arms, d_a, _, _ = make_arms(lib, ctx, wl, dev)
        arm = arms["A decode_windows_dev"]
        for _ in range(2):
            arm()
        sys.stderr.write(f"laps of one call of A, {wl.name}:\n")
        sys.stderr.flush()
        os.environ["JPEZY_BATCH_DEBUG"] = "1"
        arm()
        del os.environ["JPEZY_BATCH_DEBUG"]
        info, d_co = ctx.read_jpeg_gpu(f)
        img = torch.empty((E, E, 3), dtype=torch.uint8, device=dev)
        us = []
        for r in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ctx.dequant_idct_packed_dev(d_co, img, qt=info.qt, comp_tq=tuple(info.Tq))
            e1.record()
            e1.synchronize()
            if r >= 2:
                us.append(e0.elapsed_time(e1))
        if a.check:
            assert torch.equal(d_a[0], img), "whole picture: A differs from the fused kernel's exact mode"
        result["whole_picture"] = {"edge": E, "fused_packed_device_stage_median_ms": float(np.median(us))}
        print(f"{wl.name}: fused kernel (dequant_idct_packed_dev) device stage: median {np.median(us):.3f} ms; the windows kernel's time is in the laps on stderr")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
