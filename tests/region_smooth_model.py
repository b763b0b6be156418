"""Test helper: the definition of a window decode with smooth (triangle-filter) chroma upsampling at scale 1, 2, 4 or 8 (include/jpezy_hip.h,
SMOOTH UPSAMPLING OF WINDOWS) restated in numpy.

A composition of three things the suite already anchors: samples are scaled_model.idct_blocks(..., N, 128) with N = 8 / scale (at N = 8 the
reference's inverse_dct); a smoothed component (smooth_model.factors) is assembled from its own block grid into its native plane at that
scale, P_s of ceil(Ws / fx) x ceil(Hs / fy) samples -- smooth_model._components with N for 8 and Ws x Hs for W x H --, clamped to bytes and
brought to Ws x Hs with smooth_model.upsample; every other component is placed as scaled_model.decode_planes places it.  Then make_rgb /
revise_value, and the window is a slice.  No outside decoder defines the result for scale != 1 (libjpeg gives chroma a larger inverse DCT
there instead of filtering); tests/test_region_smooth_model.py anchors the pieces: scale 1 is smooth_model, nothing smoothed is
scaled_model, and with replication in the filter's place the planes are scaled_model's placement.

info: a FrameInfo of jpezy_amd or of the oracle (same field names); coeffs: zig-zag int16 [mcu][block][64] as read_jpeg leaves them.
"""
import numpy as np

from jpeg_synth import ZZ
from scaled_model import idct_blocks, revise, scaled_size
from smooth_model import factors, upsample


def plane_size(info, c, scale):
    """(wc_s, hc_s) of component c's native plane at 1/scale"""
    Ws, Hs = scaled_size(info.width, info.height, scale)
    return -(-Ws * info.H[c] // info.hmax), -(-Hs * info.V[c] // info.vmax)


def replicate(P, fx, fy, W, H):
    """what stands in upsample's place in the anchor test: every sample fx x fy times, cut to W x H"""
    return np.repeat(np.repeat(np.asarray(P, dtype=np.int64), fy, axis=0), fx, axis=1)[:H, :W]


def components(coeffs, info, scale):
    """per component: (placed, native) -- decode_mcu's placement with n x n blocks cut to [Hs, Ws] (scaled_model.decode_planes' comp[]) and
    the component's own block grid cut to its native plane [hc_s, wc_s]; unclamped samples both"""
    n = 8 // scale
    assert n in (8, 4, 2, 1) and info.precision == 8
    Ws, Hs = scaled_size(info.width, info.height, scale)
    hmax, vmax, bpm = info.hmax, info.vmax, info.blocks_per_mcu
    rows, cols = info.mcu_rows, info.mcu_cols
    nmcu = rows * cols
    co = np.asarray(coeffs).reshape(nmcu, bpm, 64).astype(np.int64)
    out = []
    blk = 0
    for sc in range(info.ncomp):
        q = np.array([info.qt[info.Tq[sc] & 3][i] for i in range(64)], dtype=np.int64)
        num_h, num_v = info.H[sc], info.V[sc]
        dupx, dupy = hmax // num_h, vmax // num_v
        mcu = np.full((nmcu, vmax * n, hmax * n), 0x80 if sc else 0, dtype=np.int64)
        grid = np.zeros((rows, num_v, n, cols, num_h, n), dtype=np.int64)                 # [uy, ky, y, ux, kx, x]
        for ky in range(num_v):
            for kx in range(num_h):
                dct = np.zeros((nmcu, 64), np.int64)
                dct[:, ZZ] = co[:, blk]                                                   # decode_huffman stores dct[ZZ[k]]
                smp = idct_blocks(dct * q, n, 128)
                rect = np.repeat(np.repeat(smp, dupy, axis=1), dupx, axis=2)
                mcu[:, ky * n: ky * n + n * dupy, kx * n: kx * n + n * dupx] = rect       # later blocks overwrite earlier ones
                grid[:, ky, :, :, kx, :] = smp.reshape(rows, cols, n, n).transpose(0, 2, 1, 3)
                blk += 1
        placed = mcu.reshape(rows, cols, vmax * n, hmax * n).transpose(0, 2, 1, 3).reshape(rows * vmax * n, cols * hmax * n)[:Hs, :Ws]
        wc, hc = plane_size(info, sc, scale)
        out.append((placed, grid.reshape(rows * num_v * n, cols * num_h * n)[:hc, :wc]))
    return out


def component_planes(coeffs, info, scale, filt=upsample, clamp=True):
    """-> three int64 [Hs, Ws]: filt over P_s for a smoothed component (clamp: P_s clamped to bytes first, the definition), the reduced
    decode's placement (unclamped samples) for every other one; a missing component is 0 / 0x80 (ref :104-105)"""
    Ws, Hs = scaled_size(info.width, info.height, scale)
    out = [np.full((Hs, Ws), 0x80 if i else 0, dtype=np.int64) for i in range(3)]
    for sc, (placed, native) in enumerate(components(coeffs, info, scale)):
        f = factors(info, sc)
        out[sc] = placed if f is None else filt(np.clip(native, 0, 255) if clamp else native, f[0], f[1], Ws, Hs)
    return out


def rgb_of(planes, gray=False):
    """make_rgb / revise_value (ref :567-578) over three component planes -> three uint8 arrays of the same shape"""
    yv, uv, vv = (np.asarray(p).astype(np.float64) for p in planes)
    if gray:
        r = g = b = revise(yv)
        return r, g, b
    return (revise(yv + (vv - 0x80) * 1.4020), revise(yv - (uv - 0x80) * 0.3441 - (vv - 0x80) * 0.7139), revise(yv + (uv - 0x80) * 1.7718))


def decode_picture(coeffs, info, scale, gray=False):
    """-> (r, g, b) uint8 [Hs, Ws]: the whole picture at 1/scale"""
    return rgb_of(component_planes(coeffs, info, scale), gray)


def decode_window(coeffs, info, scale, region, gray=False):
    """-> (r, g, b) uint8 planes of w * h bytes, flat: rows y .. y+h, columns x .. x+w of decode_picture"""
    x, y, w, h = region
    return tuple(np.ascontiguousarray(p[y:y + h, x:x + w]).reshape(-1) for p in decode_picture(coeffs, info, scale, gray))
