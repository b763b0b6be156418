"""Test helper: the definition of a reduced-size decode (include/jpezy_hip.h) restated in numpy.

The result is what the reference's decode loop (oracle jo_idct_block + jo_decode_planes_rows; ref decoder/jpezy_decoder.hpp:504-578,
645-676) would give if its block were n x n instead of 8 x 8, n = 8 / scale.  Blocks and samples are vectorised, but every sum is
accumulated term by term in the reference's (v outer, u inner) order and every term is the left-to-right product
cu * cv * dct * COS[u*8/n][x] * COS[v*8/n][y]: elementwise float64 numpy operations are IEEE, so this reproduces the C.  At n = 8 it is
the oracle's decode_planes (tests/test_scaled_model.py), which anchors it.

info: a FrameInfo of jpezy_amd or of the oracle (same field names); coeffs: zig-zag int16 [mcu][block][64] as read_jpeg leaves them.
"""
import functools

import numpy as np

from jpeg_synth import ZZ

INT_MIN = -2 ** 31


@functools.lru_cache(maxsize=None)
def constants():
    """(COS[64] as [u][x], INV_SQRT2): the oracle's, i.e. include/jpezy_constants.h's"""
    from oracle import oracle as O
    c = O.constants()
    return np.asarray(c["cos"], dtype=np.float64).reshape(8, 8), float(c["inv_sqrt2"])


def scaled_size(W, H, scale):
    n = 8 // scale
    return -(-W * n // 8), -(-H * n // 8)


def ref_int(x):
    """int(x) as the reference's x86-64 build executes it: truncation toward zero, INT_MIN outside [-2^31, 2^31) and for NaN"""
    x = np.asarray(x, dtype=np.float64)
    ok = (x >= -2.0 ** 31) & (x < 2.0 ** 31)
    return np.where(ok, np.trunc(np.where(ok, x, 0.0)), INT_MIN).astype(np.int64)


def idct_blocks(dct, n, level):
    """dct: [nb, 64] dequantised coefficients, natural order -> [nb, n (y), n (x)] samples"""
    cos, s2 = constants()
    d = np.asarray(dct, dtype=np.float64).reshape(-1, 8, 8)                   # [nb, v, u]
    step = 8 // n
    s = np.zeros((d.shape[0], n, n))                                          # [nb, y, x]
    for v in range(n):
        cv = s2 if v == 0 else 1.0
        for u in range(n):
            cu = s2 if u == 0 else 1.0
            t = (cu * cv) * d[:, v, u]
            t = t[:, None, None] * cos[u * step, :n][None, None, :]
            t = t * cos[v * step, :n][None, :, None]
            s = s + t
    return ref_int(s / 4 + level)


def revise(v):
    v = np.asarray(v, dtype=np.float64)
    return np.where(v < 0, 0, np.where(v > 255, 255, np.trunc(np.clip(v, 0, 255)))).astype(np.uint8)


def decode_planes(coeffs, info, scale, gray=False):
    """-> (r, g, b) uint8 planes of Ws * Hs bytes, flat"""
    n = 8 // scale
    assert n in (8, 4, 2, 1)
    W, H, ncomp = info.width, info.height, info.ncomp
    hmax, vmax, bpm = info.hmax, info.vmax, info.blocks_per_mcu
    nmcu = info.mcu_cols * info.mcu_rows
    co = np.asarray(coeffs).reshape(nmcu, bpm, 64).astype(np.int64)
    level = 128 if info.precision == 8 else 2048
    # decode_mcu with n for 8: the component planes of every MCU, unwritten positions keep 0 / 0x80
    comp = [np.full((nmcu, vmax * n, hmax * n), 0x80 if i else 0, dtype=np.int64) for i in range(3)]
    blk = 0
    for sc in range(ncomp):
        q = np.array([info.qt[info.Tq[sc] & 3][i] for i in range(64)], dtype=np.int64)
        num_h, num_v = info.H[sc], info.V[sc]
        dupx, dupy = hmax // num_h, vmax // num_v
        for ky in range(num_v):
            for kx in range(num_h):
                dct = np.zeros((nmcu, 64), np.int64)
                dct[:, ZZ] = co[:, blk]                                       # decode_huffman stores dct[ZZ[k]]
                smp = idct_blocks(dct * q, n, level)
                rect = np.repeat(np.repeat(smp, dupy, axis=1), dupx, axis=2)  # block[(y_u / dupc_y) * n + x_u / dupc_x]
                comp[sc][:, ky * n: ky * n + n * dupy, kx * n: kx * n + n * dupx] = rect      # later blocks overwrite earlier ones
                blk += 1
    Ws, Hs = scaled_size(W, H, scale)
    full = [c.reshape(info.mcu_rows, info.mcu_cols, vmax * n, hmax * n).transpose(0, 2, 1, 3)
             .reshape(info.mcu_rows * vmax * n, info.mcu_cols * hmax * n)[:Hs, :Ws].astype(np.float64) for c in comp]
    yv, uv, vv = full
    if gray:
        r = g = b = revise(yv)
    else:                                                                     # make_rgb, ref :567-578
        r = revise(yv + (vv - 0x80) * 1.4020)
        g = revise(yv - (uv - 0x80) * 0.3441 - (vv - 0x80) * 0.7139)
        b = revise(yv + (uv - 0x80) * 1.7718)
    return r.reshape(-1), g.reshape(-1), b.reshape(-1)
