"""Test helper: a picture that overflows the f32 encode kernels' queue of guard-band hits at force_exact 0 (jpezy_f32_quad.h, QUEUE_CAP).
Every block of it is an integer multiple of one integer block P whose exact transform F is an integer block too: 23 AC coefficients sit
exactly on an integer -- each on a truncation boundary at Q = 1 (quality 100), flagged by level 1 and queued -- which is more than a third
of a work unit's coefficients against a queue of 382 entries.  Shared by tests/test_gpu_sampling422.py and tests/test_gpu_sampling.py."""
from functools import lru_cache

import numpy as np

# an integer F that commutes with the signed permutation by which the Galois map cos t -> cos 3t acts on the rows of the DCT matrix D
# (a signed 4-cycle on rows 1, 3, 7, 5, a signed swap of rows 2, 6, a sign flip of rows 0, 4): P = D^T F D is then rational -- here an
# integer block with entries in -9 .. 8 -- and F = D P D^T, 23 AC entries and no DC, is its exact transform
EXACT_F = [[0, 0, 0, 0, -16, 0, 0, 0], [0, -2, 0, 6, 0, -6, 0, 4], [0, 0, 8, 0, 0, 0, -8, 0], [0, 6, 0, -2, 0, -4, 0, -6],
           [-8, 0, 0, 0, -16, 0, 0, 0], [0, -6, 0, 4, 0, -2, 0, -6], [0, 0, 8, 0, 0, 0, 8, 0], [0, -4, 0, -6, 0, -6, 0, -2]]
QUEUE_CAP = 382                                                            # jpezy_f32_quad.h


def rgb_for(y, cb, cr):
    """uint8 planes whose truncated samples (the reference's FP64 order) are exactly the integer arrays y, cb, cr: a search of the 7^3
    triples around the real inverse"""
    r0, g0, b0 = np.round(y + 128 + 1.402 * cr), np.round(y + 128 - 0.344 * cb - 0.714 * cr), np.round(y + 128 + 1.772 * cb)
    d = np.arange(-3, 4)
    dr, dg, db = (a.reshape(-1) for a in np.meshgrid(d, d, d, indexing="ij"))
    r, g, b = ((c[..., None] + e).clip(0, 255) for c, e in ((r0, dr), (g0, dg), (b0, db)))
    ok = (np.trunc((0.2990 * r) + (0.5870 * g) + (0.1140 * b) - 128) == y[..., None]) & \
         (np.trunc(-(0.1687 * r) - (0.3313 * g) + (0.5000 * b)) == cb[..., None]) & (np.trunc((0.5000 * r) - (0.4187 * g) - (0.0813 * b)) == cr[..., None])
    assert ok.any(-1).all(), "a sample triple no RGB triple reaches"
    k = ok.argmax(-1)[..., None]
    return tuple(np.take_along_axis(c, k, -1)[..., 0].astype(np.uint8).reshape(-1) for c in (r, g, b))


@lru_cache(maxsize=None)
def exact_picture(W, H, pair):
    """(r, g, b, samples): every luma block is k P (k = 1 .. 5 by block), every Cb block k P^T and every Cr block -k P (k = 1 .. 3).
    pair = 2: chroma planes of W / 2 columns, both pixels of a horizontal pair carry the pair's chroma sample, so the point rule and the
    averaged rule of 4:2:2 see the same samples; pair = 1: a chroma sample per pixel (4:4:4)"""
    u, x = np.arange(8)[:, None], np.arange(8)[None, :]
    D = np.cos((2 * x + 1) * u * np.pi / 16) * 0.5
    D[0] /= np.sqrt(2)
    F = np.array(EXACT_F, np.float64)
    P = D.T @ F @ D
    assert np.abs(P - np.round(P)).max() < 1e-9 and np.abs(D @ np.round(P) @ D.T - F).max() < 1e-9
    P = np.round(P).astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    Y = (1 + (xx // 8 + yy // 8) % 5) * P[yy % 8, xx % 8]
    cy, cx = np.mgrid[0:H, 0:W // pair]
    kc = 1 + (cx // 8 + 2 * (cy // 8)) % 3
    Cb, Cr = kc * P.T[cy % 8, cx % 8], -kc * P[cy % 8, cx % 8]
    r, g, b = rgb_for(Y, np.repeat(Cb, pair, 1), np.repeat(Cr, pair, 1))
    return r, g, b, (Y, Cb, Cr)
