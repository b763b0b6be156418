"""Test helper: the definition of the YCbCr 4:2:2 entry points (include/jpezy_hip_ycc422.h) restated with numpy, the
oracle's own block transform and the models it stands on (tests/quant_model.py, sampling422_model.py, ycc_model.py).

Sizes: CW = ceil(W/2), CH = H; a packed row holds ceil(W/2) macropixels of 4 bytes.  Formats (a macropixel covers pixels 2x', 2x'+1):
YUY2 = Y0 Cb Y1 Cr, UYVY = Cb Y0 Cr Y1, YVYU = Y0 Cr Y1 Cb.

Encode: 16 x 8 MCUs of four blocks Y-left, Y-right, Cb, Cr.  Luma sample (x, y) of the clamp-extended picture is
Y[min(y, H-1)][min(x, W-1)] - 128, chroma sample (x', y) is C[min(y, H-1)][min(x', CW-1)] - 128; every block through
quant_model.fdct_blocks (the oracle's jo_fdct_block) and sampling422_model.quantise (C's truncating division, zig-zag order).  With an
odd W the second Y byte of a packed row's last macropixel is not read.

Decode to packed 4:2:2 from any layout: the Y byte of pixel (x, y) is revise_value of the luma sample; the Cb / Cr byte of macropixel x'
in row y is revise_value of the component sample that the nearest-neighbour decode feeds make_rgb for pixel (2x', y) -- the samples
replicated as ycc_model.rgb_from_samples replicates them, read at the even column; 0x80 for a one-component file.  With an odd W the
last macropixel's second Y byte is a copy of its first.
"""
import numpy as np

import quant_model as QM
import sampling422_model as S422
import ycc_model as YM
from scaled_model import revise

YUY2, UYVY, YVYU = 0, 1, 2
FORMATS = (YUY2, UYVY, YVYU)
# byte of Y0, Cb, Cr inside a macropixel; Y1 is two behind Y0
OFFSETS = {YUY2: (0, 1, 3), UYVY: (1, 0, 2), YVYU: (0, 3, 1)}

# the sizes that reach each path of a 128 x 8 octet in a 4-wave workgroup
SIZES = [(1, 1), (2, 1), (7, 5), (15, 17), (16, 8), (17, 9), (100, 100), (128, 8), (144, 8), (512, 8), (528, 16), (1024, 16), (2048, 7)]
ANCHOR_SIZES = [s for s in SIZES if s[0] % 2 == 1 or s[0] % 16 == 0]


def row_bytes(W):
    return 4 * ((W + 1) // 2)


def chroma_size(W, H):
    return (W + 1) // 2, H


def pack(y, cb, cr, fmt, fill=0x5A):
    """planes y (H, W), cb / cr (H, CW) -> uint8 (H, row_bytes).  Odd W: the last macropixel's second Y byte, which no definition reads,
    is `fill`"""
    y, cb, cr = (np.asarray(p, np.uint8) for p in (y, cb, cr))
    H, W = y.shape
    CW = (W + 1) // 2
    assert cb.shape == cr.shape == (H, CW)
    oy, ob, orr = OFFSETS[fmt]
    out = np.full((H, CW, 4), fill, np.uint8)
    out[:, :, oy] = y[:, 0::2]
    out[:, :W // 2, oy + 2] = y[:, 1::2]
    out[:, :, ob] = cb
    out[:, :, orr] = cr
    return out.reshape(H, 4 * CW)


def unpack(img, W, fmt):
    """uint8 (H, >= row_bytes) -> y (H, W), cb, cr (H, CW)"""
    img = np.asarray(img, np.uint8)
    H, CW = img.shape[0], (W + 1) // 2
    m = img[:, :4 * CW].reshape(H, CW, 4)
    oy, ob, orr = OFFSETS[fmt]
    y = np.empty((H, 2 * CW), np.uint8)
    y[:, 0::2] = m[:, :, oy]
    y[:, 1::2] = m[:, :, oy + 2]
    return y[:, :W].copy(), m[:, :, ob].copy(), m[:, :, orr].copy()


def planes_from_rgb(r, g, b, W, H):
    """the anchor's planes: Y = trunc(ref luma) + 128 of every pixel, Cb / Cr = trunc(ref chroma) + 128 of pixel (2x', y) (they fit a
    byte); elementwise float64 numpy in the reference's order (ref encoder/jpezy_encoder.hpp:244-256)"""
    r, g, b = (np.asarray(p, dtype=np.uint8).reshape(H, W).astype(np.float64) for p in (r, g, b))
    yv = np.trunc((0.2990 * r) + (0.5870 * g) + (0.1140 * b) - 128) + 128
    r2, g2, b2 = r[:, ::2], g[:, ::2], b[:, ::2]
    cbv = np.trunc(-(0.1687 * r2) - (0.3313 * g2) + (0.5000 * b2)) + 128
    crv = np.trunc((0.5000 * r2) - (0.4187 * g2) - (0.0813 * b2)) + 128
    for p in (yv, cbv, crv):
        assert p.min() >= 0 and p.max() <= 255
    return yv.astype(np.uint8), cbv.astype(np.uint8), crv.astype(np.uint8)


def samples(y, cb, cr):
    """planes -> (ys, cbs, crs): int32 samples of the clamp-extended picture, ys (mr*8, mc*16), cbs / crs (mr*8, mc*8)"""
    y, cb, cr = (np.asarray(p) for p in (y, cb, cr))
    H, W = y.shape
    CW = (W + 1) // 2
    assert cb.shape == cr.shape == (H, CW)
    mc, mr, _ = S422.geometry(W, H)
    rows = np.minimum(np.arange(mr * 8), H - 1)
    cols, ccols = np.minimum(np.arange(mc * 16), W - 1), np.minimum(np.arange(mc * 8), CW - 1)
    return (y[np.ix_(rows, cols)].astype(np.int32) - 128, cb[np.ix_(rows, ccols)].astype(np.int32) - 128,
            cr[np.ix_(rows, ccols)].astype(np.int32) - 128)


def dct(y, cb, cr):
    """planes -> the unquantised DCT of every block, int32 [mr, mc, 4, 64] natural order"""
    ys, cbs, crs = samples(y, cb, cr)
    mr, mc = ys.shape[0] // 8, ys.shape[1] // 16
    out = np.zeros((mr, mc, 4, 64), np.int32)
    out[:, :, 0:2] = QM.fdct_blocks(S422._blocks(ys, mr, 2 * mc).reshape(-1, 64)).reshape(mr, mc, 2, 64)
    out[:, :, 2] = QM.fdct_blocks(S422._blocks(cbs, mr, mc).reshape(-1, 64)).reshape(mr, mc, 64)
    out[:, :, 3] = QM.fdct_blocks(S422._blocks(crs, mr, mc).reshape(-1, 64)).reshape(mr, mc, 64)
    return out


def encode_coeffs(y, cb, cr, luma, chroma):
    """planes -> int16 [mr, mc, 4, 64] zig-zag coefficients"""
    return S422.quantise(dct(y, cb, cr), luma, chroma)


def encode_coeffs_packed(img, W, fmt, luma, chroma):
    """the packed definition, byte by byte: sample (x, y) is byte 4 (x >> 1) + oy + 2 (x & 1) of row min(y, H-1) at x = min(x, W-1),
    chroma sample (x', y) byte 4 min(x', CW-1) + ob / or"""
    img = np.asarray(img, np.uint8)
    H, CW = img.shape[0], (W + 1) // 2
    oy, ob, orr = OFFSETS[fmt]
    x = np.arange(W)
    xc = np.arange(CW)
    y = img[:, 4 * (x >> 1) + oy + 2 * (x & 1)]
    return encode_coeffs(y, img[:, 4 * xc + ob], img[:, 4 * xc + orr], luma, chroma)


def random_planes(W, H, seed=0):
    rng = np.random.default_rng(4220000 + 1000 * W + H + 7919 * seed)
    CW = (W + 1) // 2
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (H, CW), (H, CW)))


# ---- decode ----
def decode_yuv422(coeffs, info, fmt):
    """coefficients of a parsed file of any layout -> uint8 (H, row_bytes) packed macropixels"""
    W, H = info.width, info.height
    smp = YM.decode_samples(coeffs, info)
    full = []
    for c in range(3):
        if c >= info.ncomp:
            full.append(np.full((H, W), 0x80 if c else 0, np.int64))
            continue
        assert info.hmax % info.H[c] == 0 and info.vmax % info.V[c] == 0
        s = np.repeat(np.repeat(smp[c], info.vmax // info.V[c], axis=0), info.hmax // info.H[c], axis=1)
        full.append(s[:H, :W])
    y = revise(full[0])
    img = pack(y, revise(full[1][:, 0::2]), revise(full[2][:, 0::2]), fmt)
    if W & 1:
        img[:, 4 * (W // 2) + OFFSETS[fmt][0] + 2] = y[:, W - 1]
    return img
