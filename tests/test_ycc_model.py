"""Planar YCbCr 4:2:0 in and out, as far as it can be checked without a GPU: the restatement of the definition (tests/ycc_model.py)
against the oracle -- the encode anchor (planes derived from RGB give the RGB path's coefficients wherever the definition says they
must, and differ where it says they must), the flat-plane DCs at the ends of the sample range, and both decode anchors (Y = the r plane
of a gray decode; the unclamped chroma samples, replicated and put through make_rgb, reproduce the oracle's RGB planes).
tests/test_gpu_ycc.py holds the parity tests."""
import numpy as np
import pytest

import ycc_model as M
from jpeg_synth import synth_jpeg

EQUAL_SIZES = [(16, 16), (64, 16), (48, 32), (1, 1), (7, 5), (15, 17), (65, 47), (33, 16), (16, 31)]   # each of W, H a multiple of 16 or odd
DIFFER_SIZES = [(100, 100), (20, 16), (16, 22)]      # an even edge that is no multiple of 16: colour must differ, gray must agree
L420 = [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]
L444 = [(1, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]
L422 = [(2, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]


@pytest.mark.parametrize("W,H", EQUAL_SIZES + DIFFER_SIZES)
def test_encode_anchor(oracle, W, H):
    r, g, b = oracle.synth_rgb(W, H, frame=W * 131 + H)
    y, cb, cr = M.planes_from_rgb(r, g, b, W, H)
    assert np.array_equal(M.encode_coeffs(y, gray=True), oracle.encode_coeffs(r, g, b, W, H, gray=True))
    got, want = M.encode_coeffs(y, cb, cr), oracle.encode_coeffs(r, g, b, W, H)
    assert np.array_equal(got[:, :, :4], want[:, :, :4])
    if (W, H) in EQUAL_SIZES:
        assert np.array_equal(got, want)
    else:
        # behind the even edge the RGB path replicates pixel W-1 (H-1), the chroma plane's last sample belongs to pixel W-2 (H-2)
        assert not np.array_equal(got[:, :, 4:], want[:, :, 4:])


def test_planes_from_rgb_is_the_oracles_conversion(oracle):
    L = oracle.lib()
    r, g, b = oracle.synth_rgb(16, 6, frame=5)
    y, cb, cr = M.planes_from_rgb(r, g, b, 16, 6)
    rr, gg, bb = (p.reshape(6, 16) for p in (r, g, b))
    for yy in range(6):
        for xx in range(16):
            assert int(y[yy, xx]) == L.jo_rgb_y(int(rr[yy, xx]), int(gg[yy, xx]), int(bb[yy, xx])) + 128
    for yy in range(3):
        for xx in range(8):
            px = (int(rr[2 * yy, 2 * xx]), int(gg[2 * yy, 2 * xx]), int(bb[2 * yy, 2 * xx]))
            assert (int(cb[yy, xx]), int(cr[yy, xx])) == (L.jo_rgb_cb(*px) + 128, L.jo_rgb_cr(*px) + 128)


@pytest.mark.parametrize("value,dc_luma,dc_chroma", [(0, -63, -60), (255, 63, 59)])
def test_flat_plane_dcs(value, dc_luma, dc_chroma):
    """samples of -128 / +127: block sums -8192 (the first entry of the exact DC table, a multiple of 8 Q) and +8128"""
    y, c = np.full((16, 16), value, np.uint8), np.full((8, 8), value, np.uint8)
    co = M.encode_coeffs(y, c, c)[0, 0]
    assert co[:4, 0].tolist() == [dc_luma] * 4 and co[4:, 0].tolist() == [dc_chroma] * 2
    assert not co[:, 1:].any()


@pytest.mark.parametrize("name,comps", [("own", L420), ("444", L444), ("422", L422)])
def test_decode_anchors(oracle, name, comps):
    data, _, _ = synth_jpeg(37, 21, comps, seed=11)
    info, co = oracle.read_jpeg(data)
    smp = M.decode_samples(co, info)
    planes = M.decode_planes(co, info)
    assert [p.shape[::-1] for p in planes] == [M.component_size(info, c) for c in range(3)]
    # luma: the existing gray decode stores clamp(Y)
    assert np.array_equal(planes[0].reshape(-1), oracle.decode_planes(co, info, gray=True)[0])
    # chroma: replicated as decode_mcu replicates them and put through make_rgb
    for a, e in zip(M.rgb_from_samples(smp, info), oracle.decode_planes(co, info)):
        assert np.array_equal(a, e)


def test_component_sizes():
    from types import SimpleNamespace as NS
    info = NS(width=37, height=21, H=[2, 1, 1], V=[2, 1, 1], hmax=2, vmax=2)
    assert [M.component_size(info, c) for c in range(3)] == [(37, 21), (19, 11), (19, 11)]
    assert M.chroma_size(37, 21) == (19, 11) and M.chroma_size(16, 16) == (8, 8) and M.chroma_size(1, 1) == (1, 1)
