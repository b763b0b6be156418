"""Test helper: the definition of JPEZY_DOWNSAMPLE_AVERAGE (include/jpezy_hip.h, CHROMA DOWNSAMPLING) restated with numpy
over quant_model's block transform and quantiser.

The 4:2:0 RGB encode of quant_model with ONE step changed: Cb and Cr are computed for every pixel of the picture extended to whole
16 x 16 MCUs (the reference's FP64 order, truncating: signed integers, no + 128), and chroma sample (x', y') is
    (c[2y'][2x'] + c[2y'][2x'+1] + c[2y'+1][2x'] + c[2y'+1][2x'+1] + bias(x')) >> 2,   bias = 1 for even x', 2 for odd x',
with an arithmetic shift (it floors) -- libjpeg's h2v2_downsample carried over to signed samples.  The averaging is written here once
(average_2x2) and nowhere borrows library code.  mode = POINT is quant_model's own definition (the top-left pixel of every 2x2).
"""
import numpy as np

import quant_model as QM

POINT, AVERAGE = 0, 1


def average_2x2(c):
    """int plane (2h, 2w) -> (h, w): the floor-averaged 2x2 with the alternating bias 1, 2 along x'"""
    c = np.asarray(c, np.int64)
    s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1], dtype=np.int64) & 1)
    return ((s + bias[None, :]) >> 2).astype(np.int32)            # numpy's >> on signed integers is arithmetic


def padded_samples(r, g, b, W, H):
    """planar uint8 r, g, b -> (ys, cbs, crs) of EVERY pixel of the picture extended to whole 16 x 16 MCUs by clamping, int32"""
    mc, mr = (W + 15) // 16, (H + 15) // 16
    rows, cols = np.minimum(np.arange(mr * 16), H - 1), np.minimum(np.arange(mc * 16), W - 1)
    r, g, b = (np.asarray(p, dtype=np.uint8).reshape(H, W)[np.ix_(rows, cols)].astype(np.float64) for p in (r, g, b))
    ys = np.trunc((0.2990 * r) + (0.5870 * g) + (0.1140 * b) - 128).astype(np.int32)
    cbs = np.trunc(-(0.1687 * r) - (0.3313 * g) + (0.5000 * b)).astype(np.int32)
    crs = np.trunc((0.5000 * r) - (0.4187 * g) - (0.0813 * b)).astype(np.int32)
    return ys, cbs, crs


def dct_from_rgb(r, g, b, W, H, mode=AVERAGE):
    """the unquantised DCT of every block, int32 [mr, mc, 6, 64] natural order"""
    ys, cbs, crs = padded_samples(r, g, b, W, H)
    if mode == POINT:
        cb2, cr2 = cbs[::2, ::2], crs[::2, ::2]
    else:
        cb2, cr2 = average_2x2(cbs), average_2x2(crs)
    return QM._blocks_from_planes(ys, cb2, cr2, False)


def encode_coeffs(r, g, b, W, H, luma, chroma, mode=AVERAGE):
    """int16 [mr, mc, 6, 64] zig-zag: what fdct_quant gives for a colour picture under the mode and the tables"""
    return QM.quantise(dct_from_rgb(r, g, b, W, H, mode), luma, chroma)


def stripes(W, H, a=(200, 60, 60), b=(60, 120, 200)):
    """one-pixel vertical colour stripes: colour a on even columns, b on odd ones -> planar r, g, b (flat uint8)"""
    img = np.empty((H, W, 3), np.uint8)
    img[:, 0::2] = a
    img[:, 1::2] = b
    return tuple(np.ascontiguousarray(img[..., k]).reshape(-1) for k in range(3))


def doubled(W, H, seed=5):
    """a random picture of (ceil(W/2), ceil(H/2)) pixels with every pixel doubled in both directions, cropped to W x H"""
    rng = np.random.default_rng(seed)
    small = rng.integers(0, 256, ((H + 1) // 2, (W + 1) // 2, 3), dtype=np.uint8)
    img = np.repeat(np.repeat(small, 2, axis=0), 2, axis=1)[:H, :W]
    return tuple(np.ascontiguousarray(img[..., k]).reshape(-1) for k in range(3))


def guard_band_colours(limit=4096, band=1e-6):
    """RGB triples whose FP64 Cb or Cr value lies within `band` of an integer (the kernels' FP32 estimate flags them and the FP64
    formula decides): searched on a lattice of the colour cube (every third R and G, every B) -> uint8 [n, 3]"""
    v = np.arange(0, 256, dtype=np.float64)
    r, g, b = np.meshgrid(v[::3], v[::3], v, indexing="ij")
    cb = -(0.1687 * r) - (0.3313 * g) + (0.5000 * b)
    cr = (0.5000 * r) - (0.4187 * g) - (0.0813 * b)
    near = (np.abs(cb - np.rint(cb)) < band) | (np.abs(cr - np.rint(cr)) < band)
    out = np.stack([r[near], g[near], b[near]], axis=-1).astype(np.uint8)
    return out[:limit]
