"""Test helper: the definition of the planar YCbCr 4:2:0 entry points (include/jpezy_hip.h) restated with numpy and the
oracle's own block functions.

Encode: what the reference's MCU loop (encoder/jpezy_encoder.hpp:58-67) gives if make_YCC hands over `byte - 128` of the caller's planes
instead of converted pixels -- luma block i of MCU (ux, uy), sample (x, y) = Y[min(uy*16 + 8*(i>>1) + y, H-1)][min(ux*16 + 8*(i&1) + x, W-1)]
- 128, chroma block sample (x, y) = C[min(uy*8 + y, CH-1)][min(ux*8 + x, CW-1)] - 128 -- followed by the oracle's jo_fdct_block,
jo_quantize_block and the zig-zag read order, unchanged.

Decode: component c at its native sampling, ceil(W*H_c/hmax) x ceil(H*V_c/vmax): inverse_quantization and inverse_dct as
tests/scaled_model.py restates them at n = 8, block (kx, ky) of MCU (ux, uy) at ((ux*H_c + kx)*8, (uy*V_c + ky)*8), no replication, no
make_rgb; every byte revise_value of the integer sample.
"""
import ctypes as C
import functools

import numpy as np

from jpeg_synth import ZZ
from scaled_model import idct_blocks, revise


def chroma_size(W, H):
    return (W + 1) // 2, (H + 1) // 2


def component_size(info, c):
    return -(-info.width * info.H[c] // info.hmax), -(-info.height * info.V[c] // info.vmax)


# ---- encode ----
def _emit(samples, cs):
    """samples: int [n, 64] (y*8 + x) -> int16 [n, 64] zig-zag: jo_fdct_block, jo_quantize_block, read in zig-zag order"""
    from oracle import oracle as O
    L = O.lib()
    pic = np.ascontiguousarray(samples, dtype=np.int32)
    out = np.zeros_like(pic)
    ip = C.POINTER(C.c_int)
    a, b = pic.ctypes.data, out.ctypes.data
    for k in range(pic.shape[0]):
        po = C.cast(b + 256 * k, ip)
        L.jo_fdct_block(C.cast(a + 256 * k, ip), po)
        L.jo_quantize_block(po, cs)
    return out[:, ZZ].astype(np.int16)


def encode_coeffs(y, cb=None, cr=None, gray=False):
    """2-D uint8 planes y (H, W), cb / cr (CH, CW) -> int16 [mcu_rows, mcu_cols, 4 | 6, 64] zig-zag coefficients"""
    y = np.asarray(y)
    H, W = y.shape
    mc, mr = (W + 15) // 16, (H + 15) // 16
    rows, cols = np.minimum(np.arange(mr * 16), H - 1), np.minimum(np.arange(mc * 16), W - 1)
    ys = y[np.ix_(rows, cols)].astype(np.int32) - 128
    # [mr, by, y, mc, bx, x] -> [mr, mc, by, bx, y, x]: block i = by * 2 + bx
    yb = ys.reshape(mr, 2, 8, mc, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mr * mc, 4, 64)
    out = np.zeros((mr * mc, 4 if gray else 6, 64), np.int16)
    out[:, :4] = _emit(yb.reshape(-1, 64), 0).reshape(mr * mc, 4, 64)
    if not gray:
        CW, CH = chroma_size(W, H)
        crow, ccol = np.minimum(np.arange(mr * 8), CH - 1), np.minimum(np.arange(mc * 8), CW - 1)
        for k, c in ((4, cb), (5, cr)):
            c = np.asarray(c)
            assert c.shape == (CH, CW)
            s = c[np.ix_(crow, ccol)].astype(np.int32) - 128
            out[:, k] = _emit(s.reshape(mr, 8, mc, 8).transpose(0, 2, 1, 3).reshape(mr * mc, 64), 1)
    return out.reshape(mr, mc, -1, 64)


def planes_from_rgb(r, g, b, W, H):
    """the anchor's planes: Y = jo_rgb_y + 128, Cb / Cr = jo_rgb_cb / cr + 128 of the top-left pixel of every 2x2 (they fit a byte);
    elementwise float64 numpy in the reference's order (ref encoder/jpezy_encoder.hpp:244-256)"""
    r, g, b = (np.asarray(p, dtype=np.uint8).reshape(H, W).astype(np.float64) for p in (r, g, b))
    yv = np.trunc((0.2990 * r) + (0.5870 * g) + (0.1140 * b) - 128) + 128
    r2, g2, b2 = r[::2, ::2], g[::2, ::2], b[::2, ::2]
    cbv = np.trunc(-(0.1687 * r2) - (0.3313 * g2) + (0.5000 * b2)) + 128
    crv = np.trunc((0.5000 * r2) - (0.4187 * g2) - (0.0813 * b2)) + 128
    for p in (yv, cbv, crv):
        assert p.min() >= 0 and p.max() <= 255
    return yv.astype(np.uint8), cbv.astype(np.uint8), crv.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def synth_planes(W, H, kind="random", frame=0):
    """test planes, computed once: 'random' bytes, 'rgb' = planes_from_rgb(synth_rgb), 'flat0', 'flat255'; -> (y, cb, cr), read-only"""
    from oracle import oracle as O
    CW, CH = chroma_size(W, H)
    if kind == "rgb":
        out = planes_from_rgb(*O.synth_rgb(W, H, frame=frame), W, H)
    elif kind == "random":
        rng = np.random.default_rng(1000 * W + H + 7919 * frame)
        out = tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (CH, CW), (CH, CW)))
    else:
        v = {"flat0": 0, "flat255": 255}[kind]
        out = tuple(np.full(s, v, np.uint8) for s in ((H, W), (CH, CW), (CH, CW)))
    for p in out:
        p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def synth_coeffs(W, H, kind="random", gray=False, frame=0):
    """encode_coeffs(synth_planes(...)), computed once and shared; read-only"""
    y, cb, cr = synth_planes(W, H, kind, frame)
    co = encode_coeffs(y, cb, cr, gray)
    co.setflags(write=False)
    return co


# ---- decode ----
def decode_samples(coeffs, info):
    """-> one int64 array (h_c, w_c) per component: the integer samples before revise_value"""
    hmax, vmax, bpm = info.hmax, info.vmax, info.blocks_per_mcu
    nmcu = info.mcu_cols * info.mcu_rows
    co = np.asarray(coeffs).reshape(nmcu, bpm, 64).astype(np.int64)
    level = 128 if info.precision == 8 else 2048
    out, blk = [], 0
    for sc in range(info.ncomp):
        q = np.array([info.qt[info.Tq[sc] & 3][i] for i in range(64)], dtype=np.int64)
        nh, nv = info.H[sc], info.V[sc]
        plane = np.zeros((info.mcu_rows, nv, 8, info.mcu_cols, nh, 8), np.int64)
        for ky in range(nv):
            for kx in range(nh):
                dct = np.zeros((nmcu, 64), np.int64)
                dct[:, ZZ] = co[:, blk]
                # inverse_quantization in 32-bit int arithmetic (ref decoder/jpezy_decoder.hpp:645-650)
                d32 = (dct * q).astype(np.int32).astype(np.int64)
                smp = idct_blocks(d32, 8, level)
                plane[:, ky, :, :, kx, :] = smp.reshape(info.mcu_rows, info.mcu_cols, 8, 8).transpose(0, 2, 1, 3)
                blk += 1
        w, h = component_size(info, sc)
        out.append(plane.reshape(info.mcu_rows * nv * 8, info.mcu_cols * nh * 8)[:h, :w])
    return out


def decode_planes(coeffs, info):
    """-> one uint8 array (h_c, w_c) per component: revise_value of every sample"""
    return [revise(s) for s in decode_samples(coeffs, info)]


def rgb_from_samples(samples, info, gray=False):
    """the chroma anchor: the unclamped samples replicated as decode_mcu replicates them (sampling factors that divide hmax / vmax) and
    put through make_rgb (ref decoder/jpezy_decoder.hpp:567-578) -> flat r, g, b like oracle.decode_planes"""
    W, H = info.width, info.height
    full = []
    for c in range(3):
        if c >= info.ncomp:
            full.append(np.full((H, W), 0x80 if c else 0, np.float64))
            continue
        assert info.hmax % info.H[c] == 0 and info.vmax % info.V[c] == 0
        s = np.repeat(np.repeat(samples[c], info.vmax // info.V[c], axis=0), info.hmax // info.H[c], axis=1)
        full.append(s[:H, :W].astype(np.float64))
    yv, uv, vv = full
    if gray:
        r = g = b = revise(yv)
    else:
        r = revise(yv + (vv - 0x80) * 1.4020)
        g = revise(yv - (uv - 0x80) * 0.3441 - (vv - 0x80) * 0.7139)
        b = revise(yv + (uv - 0x80) * 1.7718)
    return r.reshape(-1), g.reshape(-1), b.reshape(-1)
