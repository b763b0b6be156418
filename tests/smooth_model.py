"""Test helper: the definition of a decode with smooth (triangle-filter) chroma upsampling (include/jpezy_hip.h, CHROMA UPSAMPLING;
DESIGN.md 4.13) restated in numpy.

Samples are scaled_model.idct_blocks(..., 8, 128), i.e. the reference's inverse_dct (ref decoder/jpezy_decoder.hpp:645-670).  A component
whose replication factor is (2,1), (1,2) or (2,2) is assembled into its native plane, clamped to bytes and brought to picture size with
the integer triangle filter (libjpeg's h2v1 / h1v2 / h2v2 fancy upsamplers, coordinates clamped to the plane's true extent); every other
component is placed as decode_mcu places it (ref :504-528: replication, later blocks overwrite earlier ones), unclamped.  Then make_rgb /
revise_value (ref :531-578, 672-676).  With no smoothed component that is scaled_model.decode_planes(..., scale=1), which
tests/test_smooth_model.py checks.

info: a FrameInfo of jpezy_amd or of the oracle (same field names); coeffs: zig-zag int16 [mcu][block][64] as read_jpeg leaves them.
"""
import numpy as np

from jpeg_synth import ZZ
from scaled_model import idct_blocks, revise

SMOOTHED = ((2, 1), (1, 2), (2, 2))


def factors(info, c):
    """(fx, fy) when component c is smoothed, else None"""
    if c >= info.ncomp:
        return None
    hc, vc = info.H[c], info.V[c]
    if info.hmax % hc or info.vmax % vc:
        return None
    f = (info.hmax // hc, info.vmax // vc)
    return f if f in SMOOTHED else None


def component_size(info, c):
    """(wc, hc) of component c's native plane: jpezy_ycc_component_size"""
    return -(-info.width * info.H[c] // info.hmax), -(-info.height * info.V[c] // info.vmax)


def upsample(P, fx, fy, W, H):
    """the filter: P a native plane [hc, wc] of bytes -> U [H, W]; coordinates outside P clamp to it"""
    P = np.asarray(P, dtype=np.int64)
    hc, wc = P.shape
    X, Y = np.arange(W), np.arange(H)

    def at(yy, xx):
        return P[np.clip(yy, 0, hc - 1)[:, None], np.clip(xx, 0, wc - 1)[None, :]]

    if (fx, fy) == (2, 1):
        i = X >> 1
        n = np.where(X & 1, i + 1, i - 1)
        return (3 * at(Y, i) + at(Y, n) + np.where(X & 1, 2, 1)[None, :]) >> 2
    if (fx, fy) == (1, 2):
        j = Y >> 1
        n = np.where(Y & 1, j + 1, j - 1)
        return (3 * at(j, X) + at(n, X) + np.where(Y & 1, 2, 1)[:, None]) >> 2
    assert (fx, fy) == (2, 2)
    j = Y >> 1
    jd = np.where(Y & 1, j + 1, j - 1)
    i = X >> 1
    n = np.where(X & 1, i + 1, i - 1)
    S_i = 3 * at(j, i) + at(jd, i)
    S_n = 3 * at(j, n) + at(jd, n)
    return (3 * S_i + S_n + np.where(X & 1, 7, 8)[None, :]) >> 4


def _components(coeffs, info):
    """per component: (placed, native) -- decode_mcu's placement cut to [H, W] (unclamped samples; ref :504-528) and the component's own
    block grid cut to its native plane [hc, wc] (unclamped samples)"""
    W, H, ncomp = info.width, info.height, info.ncomp
    hmax, vmax, bpm = info.hmax, info.vmax, info.blocks_per_mcu
    rows, cols = info.mcu_rows, info.mcu_cols
    nmcu = rows * cols
    co = np.asarray(coeffs).reshape(nmcu, bpm, 64).astype(np.int64)
    assert info.precision == 8
    out = []
    blk = 0
    for sc in range(ncomp):
        q = np.array([info.qt[info.Tq[sc] & 3][i] for i in range(64)], dtype=np.int64)
        num_h, num_v = info.H[sc], info.V[sc]
        dupx, dupy = hmax // num_h, vmax // num_v
        mcu = np.full((nmcu, vmax * 8, hmax * 8), 0x80 if sc else 0, dtype=np.int64)      # decode_mcu's comp[] of every MCU
        grid = np.zeros((rows, num_v, 8, cols, num_h, 8), dtype=np.int64)                 # [uy, ky, y, ux, kx, x]
        for ky in range(num_v):
            for kx in range(num_h):
                dct = np.zeros((nmcu, 64), np.int64)
                dct[:, ZZ] = co[:, blk]                                                   # decode_huffman stores dct[ZZ[k]]
                smp = idct_blocks(dct * q, 8, 128)
                rect = np.repeat(np.repeat(smp, dupy, axis=1), dupx, axis=2)
                mcu[:, ky * 8: ky * 8 + 8 * dupy, kx * 8: kx * 8 + 8 * dupx] = rect       # later blocks overwrite earlier ones
                grid[:, ky, :, :, kx, :] = smp.reshape(rows, cols, 8, 8).transpose(0, 2, 1, 3)
                blk += 1
        placed = mcu.reshape(rows, cols, vmax * 8, hmax * 8).transpose(0, 2, 1, 3).reshape(rows * vmax * 8, cols * hmax * 8)[:H, :W]
        wc, hc = component_size(info, sc)
        out.append((placed, grid.reshape(rows * num_v * 8, cols * num_h * 8)[:hc, :wc]))
    return out


def native_plane(coeffs, info, c):
    """P of component c: uint8 [hc, wc], the bytes jpezy_decode_jpeg_ycc returns for it"""
    return np.clip(_components(coeffs, info)[c][1], 0, 255).astype(np.uint8)


def component_planes(coeffs, info):
    """-> three int64 [H, W]: U for a smoothed component, decode_mcu's placement (unclamped samples) for every other one; a missing
    component is 0 / 0x80 (ref :104-105)"""
    out = [np.full((info.height, info.width), 0x80 if i else 0, dtype=np.int64) for i in range(3)]
    for sc, (placed, native) in enumerate(_components(coeffs, info)):
        f = factors(info, sc)
        out[sc] = placed if f is None else upsample(np.clip(native, 0, 255), f[0], f[1], info.width, info.height)
    return out


def centred_ramp_picture(W=64, H=48):
    """(y, cb, cr, cb_full): a 4:2:0 picture whose chroma is a ramp sited at the centre of its 2 x 2 -- cb_full = 64 + x + y at full
    resolution, cb its 2 x 2 box mean (an integer), cr the mirrored ramp, y flat; every colour lies inside the RGB cube, so make_rgb
    clamps nothing"""
    yy, xx = np.mgrid[:H, :W]
    cb_full = 64 + xx + yy
    cr_full = 180 - xx - yy
    box = lambda p: p.reshape(H // 2, 2, W // 2, 2).sum(axis=(1, 3))
    assert not (box(cb_full) % 4).any() and not (box(cr_full) % 4).any()
    y = np.full((H, W), 128, np.uint8)
    return y, (box(cb_full) // 4).astype(np.uint8), (box(cr_full) // 4).astype(np.uint8), cb_full


def cb_of_rgb(r, g, b):
    """the forward formula (JFIF): Cb of full-range RGB, float64"""
    r, g, b = (np.asarray(p, dtype=np.float64) for p in (r, g, b))
    return -0.168736 * r - 0.331264 * g + 0.5 * b + 128.0


def decode_planes(coeffs, info, gray=False):
    """-> (r, g, b) uint8 planes of W * H bytes, flat"""
    yv, uv, vv = (p.astype(np.float64) for p in component_planes(coeffs, info))
    if gray:
        r = g = b = revise(yv)
    else:                                                                                 # make_rgb, ref :567-578
        r = revise(yv + (vv - 0x80) * 1.4020)
        g = revise(yv - (uv - 0x80) * 0.3441 - (vv - 0x80) * 0.7139)
        b = revise(yv + (uv - 0x80) * 1.7718)
    return r.reshape(-1), g.reshape(-1), b.reshape(-1)
