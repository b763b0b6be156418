#!/usr/bin/env python3
"""Development probe: wave lifetimes PER WORKGROUP of the f32 encode kernel, from the per-quad trace of one 4096^2 random frame
(build with tools/ab/ab_build.py trace:-DJPEZY_TRACE, run with JPEZY_LIB=ab/libjpezy_trace.so JPEZY_ALLOW_EXPERIMENT=1).

LDS is released per workgroup: a workgroup holds its slices from its first wave's start to its last wave's end.  The probe prints the
mean wave lifetime, the mean of the workgroups' hold times, their ratio (how much longer the resource is held than it is used), and
the resident waves per SIMD over the steady state -- all waves, and the waves still alive (the rest are finished waves whose workgroup
is not).

    python tools/profile/wave_groups.py [--waves N]     N = waves per workgroup of the launch (default 4; 2 with a forced 2-wave form)
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))
import jpezy_amd as J  # noqa: E402
from jpezy_amd import api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--waves", type=int, default=4)
    a = ap.parse_args()
    W = H = 4096
    ctx = J.Context(0)
    lib = api.load_library()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(1)
    ring = 6
    planes = [torch.randint(0, 256, (ring, W * H), dtype=torch.uint8, device=dev, generator=g) for _ in range(3)]
    out = torch.empty((ring, J.coeff_count(W, H, False)), dtype=torch.int16, device=dev)
    for it in range(12):
        k = it % ring
        ctx.fdct_quant_dev(planes[0][k], planes[1][k], planes[2][k], W, H, out[k])
    torch.cuda.synchronize()
    n = 16384                                           # 64 quads per row (a multiple of --waves), 256 MCU rows
    buf = np.zeros(n * 4, dtype=np.uint64)
    lib.jpezy_debug_read_trace.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.jpezy_debug_read_trace(ctx._h, buf.ctypes.data, n * 4)
    t = buf.reshape(n, 4)
    t0 = t[:, 0].astype(np.int64); t0 -= t0.min()
    life = t[:, 2].astype(np.int64)
    end = t0 + life
    us = 0.01                                           # one tick of s_memrealtime = 10 ns
    wg = a.waves
    g0 = t0.reshape(-1, wg).min(axis=1); g1 = end.reshape(-1, wg).max(axis=1)
    hold = g1 - g0
    gmean = life.reshape(-1, wg).mean(axis=1); gmax = life.reshape(-1, wg).max(axis=1)
    print(f"waves {n}, {wg} per workgroup, kernel span {end.max() * us:.2f} us")
    print("wave lifetime us: mean %.2f  p10 %.2f  p50 %.2f  p90 %.2f  max %.2f" % (
        life.mean() * us, *(np.percentile(life, q) * us for q in (10, 50, 90)), life.max() * us))
    print("per workgroup: mean of (mean lifetime) %.2f us, mean of (max lifetime) %.2f us, mean hold time (first start to last end) %.2f us" % (
        gmean.mean() * us, gmax.mean() * us, hold.mean() * us))
    print("ratio mean(max lifetime per workgroup) / mean lifetime = %.3f;  mean(hold) / mean lifetime = %.3f" % (
        gmax.mean() / life.mean(), hold.mean() / life.mean()))
    print("start skew inside a workgroup (last start - first start): mean %.2f us, p90 %.2f us" % (
        (t0.reshape(-1, wg).max(axis=1) - g0).mean() * us, np.percentile(t0.reshape(-1, wg).max(axis=1) - g0, 90) * us))
    # occupancy over time: slots held (workgroup granular) and waves alive, per SIMD (256 CUs x 4 SIMDs)
    span = int(end.max()) + 1
    held = np.zeros(span + 1); alive = np.zeros(span + 1)
    np.add.at(held, g0, wg); np.add.at(held, g1, -wg)
    np.add.at(alive, t0, 1); np.add.at(alive, end, -1)
    held = np.cumsum(held)[:span] / 1024.0; alive = np.cumsum(alive)[:span] / 1024.0
    lo, hi = int(0.25 * span), int(0.75 * span)         # the steady state: the middle half of the launch
    print("steady state (middle half of the launch): wave slots held %.2f per SIMD, waves alive %.2f per SIMD, alive / held = %.3f" % (
        held[lo:hi].mean(), alive[lo:hi].mean(), alive[lo:hi].mean() / held[lo:hi].mean()))
    print("whole launch: wave slots held %.2f per SIMD, waves alive %.2f per SIMD" % (held.mean(), alive.mean()))


if __name__ == "__main__":
    main()
