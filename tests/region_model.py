"""Test helper: the definition of a region decode (include/jpezy_hip.h, REGION DECODE).

The result is the existing (scaled) decode, sliced: tests/scaled_model.py's planes reshaped to (Hs, Ws) and cut to the window.  There is
no arithmetic here.
"""
import numpy as np

import scaled_model as M


def decode_region(coeffs, info, region, scale=1, gray=False):
    """region = (x, y, w, h) in the picture at 1/scale -> (r, g, b) uint8 arrays of shape (h, w)"""
    x, y, w, h = region
    ws, hs = M.scaled_size(info.width, info.height, scale)
    assert w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= ws and y + h <= hs, (region, ws, hs)
    return tuple(np.ascontiguousarray(p.reshape(hs, ws)[y:y + h, x:x + w]) for p in M.decode_planes(coeffs, info, scale, gray))
