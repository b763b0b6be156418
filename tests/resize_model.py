"""numpy restatement of the resampling of include/jpezy_hip.h, BATCH OF WINDOWS, RESIZED: the triangle filter, widened by the
reduction ratio where an axis shrinks, in integer fixed point of 22 fraction bits; horizontal pass, then vertical, each rounded and clipped
to a byte; an optional mirror of the columns.  Written from the header's definition, independently of the C++: no table comes from the
library.  Python floats are binary64 and every operation below is a separate one, in the definition's order."""
import functools
import math

import numpy as np

PRECISION_BITS = 22


@functools.lru_cache(maxsize=None)
def taps(in_size, out_size):
    """(ksize, first[out], count[out], weight[out, ksize]) of one axis; the arrays are read-only (shared between callers)"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ss = 1.0 / fs
    ksize = 2 * int(math.ceil(support)) + 1
    first = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    weight = np.zeros((out_size, ksize), np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        lo = max(0, int(center - support + 0.5))
        hi = min(in_size, int(center + support + 0.5))
        w = []
        for j in range(hi - lo):
            a = abs((j + lo - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        total = 0.0
        for v in w:
            total += v
        first[i], count[i] = lo, hi - lo
        for j, v in enumerate(w):
            k = v / total if total != 0.0 else v
            weight[i, j] = int(0.5 + k * (1 << PRECISION_BITS))
    for a in (first, count, weight):
        a.setflags(write=False)
    return ksize, first, count, weight


def _pass(img, out_size, axis):
    """one pass along `axis` of a uint8 array [h, w, channels]: every channel alike"""
    img = np.moveaxis(img, axis, 0)
    _, first, count, weight = taps(img.shape[0], out_size)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    for i in range(out_size):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for j in range(int(count[i])):
            acc += int(weight[i, j]) * img[int(first[i]) + j].astype(np.int64)
        assert acc.max(initial=0) < 2 ** 31 and acc.min(initial=0) >= 0          # the device accumulates in 32-bit int
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return np.moveaxis(out, 0, axis)


def resize(img, out_w, out_h, mirror=False):
    """uint8 [h, w, bytes] -> uint8 [out_h, out_w, bytes]; bytes 3: every channel resampled; bytes 4: byte 3 is 0xFF and is not resampled"""
    img = np.asarray(img, np.uint8)
    assert img.ndim == 3 and img.shape[2] in (3, 4)
    res = _pass(_pass(img[:, :, :3], out_w, 1), out_h, 0)
    if img.shape[2] == 4:
        res = np.concatenate([res, np.full((out_h, out_w, 1), 0xFF, np.uint8)], axis=2)
    if mirror:
        res = res[:, ::-1]
    return np.ascontiguousarray(res)


def pick_window(W, H, src, out_w, out_h):
    """((x, y, w, h), scale) for the rectangle src of the full-size picture: the largest scale that leaves at least out_w x out_h pixels"""
    x, y, w, h = src
    assert w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= W and y + h <= H
    s = next((t for t in (8, 4, 2) if w // t >= out_w and h // t >= out_h), 1)
    return (x // s, y // s, max(1, w // s), max(1, h // s)), s
