"""numpy restatement of the resampling of include/jpezy_hip.h, BATCH OF WINDOWS, RESIZED with its FILTERS: tests/resize_model.py
with the three things that depend on the filter -- the support, f(x) and the rounding of a negative weight -- as functions of `filter`.
Written from the header's definition, independently of the C++: no table comes from the library.  Python floats are binary64, every
operation below is a separate one in the definition's order, and math.sin is the C library's."""
import functools
import math

import numpy as np

PRECISION_BITS = 22
BILINEAR, BOX, BICUBIC, LANCZOS = 0, 1, 2, 3
FILTERS = (BILINEAR, BOX, BICUBIC, LANCZOS)
SUPPORT = {BILINEAR: 1.0, BOX: 0.5, BICUBIC: 2.0, LANCZOS: 3.0}


def _sinc(x):
    if x == 0.0:
        return 1.0
    px = x * math.pi
    return math.sin(px) / px


def f(filter, x):
    if filter == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if filter == LANCZOS:
        return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0
    x = abs(x)
    if filter == BICUBIC:
        a = -0.5
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
        if x < 2.0:
            return (((x - 5.0) * x + 8.0) * x - 4.0) * a
        return 0.0
    assert filter == BILINEAR
    return 1.0 - x if x < 1.0 else 0.0


@functools.lru_cache(maxsize=None)
def taps(filter, in_size, out_size, weights=True):
    """(ksize, first[out], count[out], weight[out, ksize]) of one axis; the arrays are read-only (shared between callers).  weights=False:
    weight is None (first and count alone are cheap at any size)"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = SUPPORT[filter] * fs
    ss = 1.0 / fs
    ksize = 2 * int(math.ceil(support)) + 1
    first = np.zeros(out_size, np.int32)
    count = np.zeros(out_size, np.int32)
    weight = np.zeros((out_size, ksize), np.int32) if weights else None
    for i in range(out_size):
        center = (i + 0.5) * scale
        lo = max(0, int(center - support + 0.5))
        hi = min(in_size, int(center + support + 0.5))
        first[i], count[i] = lo, hi - lo
        if not weights:
            continue
        w = [f(filter, (j + lo - center + 0.5) * ss) for j in range(hi - lo)]
        total = 0.0
        for v in w:
            total += v
        for j, v in enumerate(w):
            k = v / total if total != 0.0 else v
            weight[i, j] = int(k * (1 << PRECISION_BITS) - 0.5) if k < 0.0 else int(k * (1 << PRECISION_BITS) + 0.5)
    for a in (first, count, weight):
        if a is not None:
            a.setflags(write=False)
    return ksize, first, count, weight


def fits_32_bits(weight):
    """the overflow condition of the definition, per table: 255 * sum(K+) + 2^21 < 2^31 and 255 * sum(K-) <= 2^31 - 2^21 for every output index"""
    w = weight.astype(np.int64)
    pos, neg = np.where(w > 0, w, 0).sum(axis=1), -np.where(w < 0, w, 0).sum(axis=1)
    return bool((255 * pos + (1 << 21) < 2 ** 31).all() and (255 * neg <= 2 ** 31 - (1 << 21)).all())


def tile_span(first, count, tile):
    """the largest number of source samples that `tile` consecutive output indices (from a multiple of tile) span"""
    n = len(first)
    return max(int(first[min(i0 + tile, n) - 1]) + int(count[min(i0 + tile, n) - 1]) - int(first[i0]) for i0 in range(0, n, tile))


def _pass(img, out_size, axis, filter):
    """one pass along `axis` of a uint8 array [h, w, channels]: every channel alike"""
    img = np.moveaxis(img, axis, 0)
    _, first, count, weight = taps(filter, img.shape[0], out_size)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    for i in range(out_size):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for j in range(int(count[i])):
            acc += int(weight[i, j]) * img[int(first[i]) + j].astype(np.int64)
            assert acc.max(initial=0) < 2 ** 31 and acc.min(initial=0) >= -2 ** 31      # the device accumulates in 32-bit int, tap by tap
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)                 # (>> of a negative numpy integer is arithmetic)
    return np.moveaxis(out, 0, axis)


def resize(img, out_w, out_h, filter, mirror=False):
    """uint8 [h, w, bytes] -> uint8 [out_h, out_w, bytes]; bytes 3: every channel resampled; bytes 4: byte 3 is 0xFF and is not resampled"""
    img = np.asarray(img, np.uint8)
    assert img.ndim == 3 and img.shape[2] in (3, 4)
    res = _pass(_pass(img[:, :, :3], out_w, 1, filter), out_h, 0, filter)
    if img.shape[2] == 4:
        res = np.concatenate([res, np.full((out_h, out_w, 1), 0xFF, np.uint8)], axis=2)
    if mirror:
        res = res[:, ::-1]
    return np.ascontiguousarray(res)
