"""Test helper: the definition of the encoder's quality / quantisation-table setting (include/jpezy_hip.h) restated with
numpy and the oracle's own block transform.

The reference's MCU loop (encoder/jpezy_encoder.hpp:58-67, :90-172) with quantization(cs) dividing by the caller's table: the picture is
extended to whole MCUs by clamping the pixel coordinates (:101, :104), make_YCC (:244-256) gives Y of every pixel and Cb / Cr of the
top-left pixel of every 2x2 in the reference's FP64 order, every 8x8 block goes through the oracle's jo_fdct_block, and blk[i] /= qt[cs][i]
is C's truncating int division; the block is read in zig-zag order.  At the Annex-K tables this is oracle.encode_coeffs
(tests/test_quant_host.py asserts it), which keeps the model honest without touching the oracle.
"""
import ctypes as C
import functools

import numpy as np

from jpeg_synth import ZZ


def quality_tables(q):
    """libjpeg's mapping over the oracle's Annex-K tables: s = q < 50 ? 5000 / q : 200 - 2 q; clamp((base * s + 50) / 100, 1, 255)"""
    from oracle import oracle as O
    c = O.constants()
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((np.asarray(c[k], np.int64) * s + 50) // 100, 1, 255).astype(np.uint8) for k in ("qt_luma", "qt_chroma"))


def custom_tables(kind):
    """the three custom sets of the GPU tests: random 1..255, all ones except DC = 255, all 255 except DC = 1"""
    if kind == "random":
        rng = np.random.default_rng(20261019)
        return tuple(rng.integers(1, 256, 64).astype(np.uint8) for _ in range(2))
    base, dc = {"ones_dc255": (1, 255), "255_dc1": (255, 1)}[kind]
    t = np.full(64, base, np.uint8)
    t[0] = dc
    return t, t.copy()


def tables(name):
    """'q<N>' or the name of a custom set -> (luma, chroma)"""
    return quality_tables(int(name[1:])) if name[0] == "q" and name[1:].isdigit() else custom_tables(name)


def fdct_blocks(samples):
    """int [n, 64] (y*8 + x) -> int32 [n, 64]: jo_fdct_block, natural order, not yet quantised"""
    from oracle import oracle as O
    L = O.lib()
    pic = np.ascontiguousarray(samples, dtype=np.int32)
    out = np.zeros_like(pic)
    ip = C.POINTER(C.c_int)
    a, b = pic.ctypes.data, out.ctypes.data
    for k in range(pic.shape[0]):
        L.jo_fdct_block(C.cast(a + 256 * k, ip), C.cast(b + 256 * k, ip))
    return out


def _blocks_from_planes(ys, cbs, crs, gray):
    """padded sample planes (mr*16, mc*16) and (mr*8, mc*8) -> unquantised DCT int32 [mr, mc, 4 | 6, 64] natural order"""
    mr, mc = ys.shape[0] // 16, ys.shape[1] // 16
    # [mr, by, y, mc, bx, x] -> [mr, mc, by, bx, y, x]: block i = by * 2 + bx
    yb = ys.reshape(mr, 2, 8, mc, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mr * mc * 4, 64)
    out = np.zeros((mr * mc, 4 if gray else 6, 64), np.int32)
    out[:, :4] = fdct_blocks(yb).reshape(mr * mc, 4, 64)
    if not gray:
        for k, c in ((4, cbs), (5, crs)):
            out[:, k] = fdct_blocks(c.reshape(mr, 8, mc, 8).transpose(0, 2, 1, 3).reshape(mr * mc, 64))
    return out.reshape(mr, mc, -1, 64)


def dct_from_rgb(r, g, b, W, H, gray=False):
    """planar uint8 r, g, b -> the unquantised DCT of every block, int32 [mr, mc, 4 | 6, 64] natural order"""
    mc, mr = (W + 15) // 16, (H + 15) // 16
    rows, cols = np.minimum(np.arange(mr * 16), H - 1), np.minimum(np.arange(mc * 16), W - 1)
    r, g, b = (np.asarray(p, dtype=np.uint8).reshape(H, W)[np.ix_(rows, cols)].astype(np.float64) for p in (r, g, b))
    ys = np.trunc((0.2990 * r) + (0.5870 * g) + (0.1140 * b) - 128).astype(np.int32)
    r2, g2, b2 = r[::2, ::2], g[::2, ::2], b[::2, ::2]
    cbs = np.trunc(-(0.1687 * r2) - (0.3313 * g2) + (0.5000 * b2)).astype(np.int32)
    crs = np.trunc((0.5000 * r2) - (0.4187 * g2) - (0.0813 * b2)).astype(np.int32)
    return _blocks_from_planes(ys, cbs, crs, gray)


def dct_from_ycc(y, cb=None, cr=None, gray=False):
    """2-D uint8 planes y (H, W), cb / cr (CH, CW) as tests/ycc_model.py takes them -> unquantised DCT, int32 [mr, mc, 4 | 6, 64]"""
    y = np.asarray(y)
    H, W = y.shape
    mc, mr = (W + 15) // 16, (H + 15) // 16
    CW, CH = (W + 1) // 2, (H + 1) // 2
    rows, cols = np.minimum(np.arange(mr * 16), H - 1), np.minimum(np.arange(mc * 16), W - 1)
    ys = y[np.ix_(rows, cols)].astype(np.int32) - 128
    cbs = crs = None
    if not gray:
        crow, ccol = np.minimum(np.arange(mr * 8), CH - 1), np.minimum(np.arange(mc * 8), CW - 1)
        cbs, crs = (np.asarray(c)[np.ix_(crow, ccol)].astype(np.int32) - 128 for c in (cb, cr))
    return _blocks_from_planes(ys, cbs, crs, gray)


def quantise(dct, luma, chroma):
    """unquantised DCT [..., B, 64] natural order -> int16 zig-zag coefficients: C's truncating division by the tables (blocks 0..3 luma)"""
    d = np.asarray(dct, np.int64)
    q = np.empty((d.shape[-2], 64), np.int64)
    q[:4] = np.asarray(luma, np.int64).reshape(64)
    q[4:] = np.asarray(chroma, np.int64).reshape(64)
    out = np.sign(d) * (np.abs(d) // q)
    return out[..., ZZ].astype(np.int16)


def encode_coeffs(r, g, b, W, H, luma, chroma, gray=False):
    return quantise(dct_from_rgb(r, g, b, W, H, gray), luma, chroma)


@functools.lru_cache(maxsize=None)
def synth_dct(W, H, gray=False, frame=0):
    """dct_from_rgb(oracle.synth_rgb(W, H, frame)), computed once and shared; read-only"""
    from oracle import oracle as O
    d = dct_from_rgb(*O.synth_rgb(W, H, frame=frame), W, H, gray)
    d.setflags(write=False)
    return d
