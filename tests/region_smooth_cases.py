"""Test helper: the files and references the GPU tests of the smooth window decode share (tests/test_gpu_region_smooth.py,
tests/test_gpu_windows_smooth.py).  Files come from jpeg_synth.synth_jpeg -- random coefficients, so a ring sample taken from the wrong
place changes bytes --, are made once and never modified; a reference is one whole picture of tests/region_smooth_model.py per (file, scale,
gray), computed once, read-only, and sliced."""
import functools

import numpy as np

import region_smooth_model as RS
import scaled_model
from jpeg_synth import synth_jpeg

FILL = 0xA5
LAYOUTS = {
    "own": [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
    "h2v1": [(2, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
    "h1v2": [(1, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
    "mixed": [(2, 2, 0, 0), (2, 1, 1, 1), (1, 2, 1, 1)],
    "two_chroma_blocks": [(4, 2, 0, 0), (2, 1, 1, 1), (2, 1, 1, 1)],      # factor 2 with two chroma blocks per MCU
    "411": [(4, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
    "444": [(1, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
    "one": [(1, 1, 0, 0)],
}
NOTHING_SMOOTHED = ("411", "444", "one")
SCALES = (1, 2, 4, 8)
QT = np.arange(1, 129).reshape(2, 64) % 23 + 1                       # one set of quantisers for the frames of a batch


@functools.lru_cache(maxsize=None)
def jpeg(layout, W, H, seed=None, precision=8, restart=0, fixed_qt=False):
    return synth_jpeg(W, H, LAYOUTS[layout], seed=7 * W + H if seed is None else seed, precision=precision, restart=restart,
                      qt=QT if fixed_qt else None)[0]


@functools.lru_cache(maxsize=None)
def parsed(data):
    """(FrameInfo, coefficients) by the host decoder"""
    import jpezy_amd
    info, co = jpezy_amd.read_jpeg(data)
    co.setflags(write=False)
    return info, co


@functools.lru_cache(maxsize=None)
def picture(data, scale, gray):
    """the model's whole picture at 1/scale: three read-only uint8 [Hs, Ws]"""
    info, co = parsed(data)
    out = RS.decode_picture(co, info, scale, gray)
    for a in out:
        a.setflags(write=False)
    return out


def want(data, region, scale, gray):
    x, y, w, h = region
    e = tuple(a[y:y + h, x:x + w] for a in picture(data, scale, gray))
    assert e[0].shape == (h, w), ("region outside the picture", region, scale)
    return e


def interleave(J, fmt, planes):
    nb = 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4
    order = (0, 1, 2) if fmt in (J.PIX_RGB24, J.PIX_RGBA32) else (2, 1, 0)
    img = np.full(planes[0].shape + (nb,), 0xFF, np.uint8)
    for k in range(3):
        img[..., k] = planes[order[k]]
    return img


def windows(info, scale):
    """{name: (x, y, w, h)} in the picture at 1/scale: where a kernel that reads a ring around its MCU can go wrong"""
    n = 8 // scale
    ws, hs = scaled_model.scaled_size(info.width, info.height, scale)
    mw, mh = info.hmax * n, info.vmax * n
    out = {"whole": (0, 0, ws, hs), "corner_00": (0, 0, 1, 1), "corner_10": (ws - 1, 0, 1, 1), "corner_01": (0, hs - 1, 1, 1),
           "corner_11": (ws - 1, hs - 1, 1, 1), "last_column": (ws - 1, 0, 1, hs), "last_row": (0, hs - 1, ws, 1)}
    if mw < ws and mh < hs:                                          # the first interior MCU corner: each of the four needs a diagonal neighbour
        for dx in (-1, 0):
            for dy in (-1, 0):
                out[f"mcu_corner_{dx + 1}{dy + 1}"] = (mw + dx, mh + dy, 1, 1)
    if ws > 2 and hs > 2:
        out["odd_start_odd_size"] = (1, 1, ws - 2, hs - 2)
    return out
