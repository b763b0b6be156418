"""The numpy restatement of the window decode with smooth chroma upsampling (tests/region_smooth_model.py), anchored by composition: no
outside decoder defines the result at a reduced scale, so each piece is tied to a model the suite already trusts.
  (i)   at scale 1 it is the slice of smooth_model.decode_planes (itself checked against libjpeg-turbo's fancy upsamplers);
  (ii)  with nothing smoothed it is the slice of scaled_model.decode_planes at every scale;
  (iii) with replication in the filter's place, before the byte clamp, the planes are the reduced decode's component placement at every
        scale -- P_s and its extent are the reduced decode's -- and that placement gives scaled_model.decode_planes' bytes; for a component
        whose rectangles decode_mcu lets overlap (two chroma blocks per MCU along a replicated axis) the same through its overwrite rule;
  (iv)  wc_s, hc_s are ceil(Ws * H_c / hmax), ceil(Hs * V_c / vmax) = ceil(Ws / fx), ceil(Hs / fy) for every smoothed component.
tests/test_gpu_region_smooth.py compares the kernels with this model byte for byte."""
import functools

import numpy as np
import pytest

import region_smooth_model as RS
import scaled_model
import smooth_model
from jpeg_synth import synth_jpeg

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
SMOOTHED = ("own", "h2v1", "h1v2", "mixed", "two_chroma_blocks")
SIZES = [(1, 1), (3, 3), (33, 17), (17, 33), (40, 24)]
SCALES = (1, 2, 4, 8)


@functools.lru_cache(maxsize=None)
def jpeg(layout, W, H):
    return synth_jpeg(W, H, LAYOUTS[layout], seed=3 * W + H)[0]


def windows(Ws, Hs):
    out = [(0, 0, Ws, Hs), (Ws - 1, Hs - 1, 1, 1), (0, 0, 1, 1)]
    if Ws > 2 and Hs > 2:
        out.append((1, 1, Ws - 2, Hs - 2))
    return out


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_scale_1_is_the_slice_of_the_smooth_decode(oracle, layout, gray):
    for W, H in SIZES:
        info, co = oracle.read_jpeg(jpeg(layout, W, H))
        full = [p.reshape(H, W) for p in smooth_model.decode_planes(co, info, gray)]
        for x, y, w, h in windows(W, H):
            got = RS.decode_window(co, info, 1, (x, y, w, h), gray)
            for a, e in zip(got, full):
                assert np.array_equal(a.reshape(h, w), e[y:y + h, x:x + w]), (layout, W, H, (x, y, w, h))


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("layout", ["411", "444", "one"])
def test_nothing_smoothed_is_the_slice_of_the_reduced_decode(oracle, layout, scale):
    for W, H in SIZES:
        info, co = oracle.read_jpeg(jpeg(layout, W, H))
        assert all(smooth_model.factors(info, c) is None for c in range(3))
        Ws, Hs = scaled_model.scaled_size(W, H, scale)
        for gray in (False, True):
            full = [p.reshape(Hs, Ws) for p in scaled_model.decode_planes(co, info, scale, gray)]
            for x, y, w, h in windows(Ws, Hs):
                got = RS.decode_window(co, info, scale, (x, y, w, h), gray)
                for a, e in zip(got, full):
                    assert np.array_equal(a.reshape(h, w), e[y:y + h, x:x + w]), (layout, W, H, scale, (x, y, w, h))


UNKNOWN = -10 ** 9


def overlapping_blocks(info, c):
    """decode_mcu writes block (kx, ky) at (kx * n, ky * n) as n * dupx x n * dupy samples (ref :504-528): a component with more than one
    block along an axis it is replicated on has its rectangles overlap, and the later block wins.  The nearest decode of such a component
    is NOT the replication of its native plane -- the smooth mode, which assembles the plane from the component's own block grid, differs
    from it in more than the filter -- so anchor (iii) is stated for it through the reference's own overwrite rule."""
    dupx, dupy = info.hmax // info.H[c], info.vmax // info.V[c]
    return (info.H[c] > 1 and dupx > 1) or (info.V[c] > 1 and dupy > 1)


def overwritten_placement(native, info, c, n, Ws, Hs):
    """decode_mcu's placement rule applied to the blocks of the native plane `native` (cut to its extent: what lies outside is UNKNOWN)"""
    num_h, num_v = info.H[c], info.V[c]
    dupx, dupy = info.hmax // num_h, info.vmax // num_v
    rows, cols = info.mcu_rows, info.mcu_cols
    full = np.full((rows * num_v * n, cols * num_h * n), UNKNOWN, dtype=np.int64)
    full[:native.shape[0], :native.shape[1]] = native
    blocks = full.reshape(rows, num_v, n, cols, num_h, n)
    canvas = np.full((rows, cols, info.vmax * n, info.hmax * n), 0x80 if c else 0, dtype=np.int64)
    for ky in range(num_v):
        for kx in range(num_h):
            smp = blocks[:, ky, :, :, kx, :].transpose(0, 2, 1, 3)                       # [uy, ux, y, x]
            canvas[:, :, ky * n: ky * n + n * dupy, kx * n: kx * n + n * dupx] = np.repeat(np.repeat(smp, dupy, axis=2), dupx, axis=3)
    return canvas.transpose(0, 2, 1, 3).reshape(rows * info.vmax * n, cols * info.hmax * n)[:Hs, :Ws]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_replication_in_the_filters_place_is_the_reduced_decodes_placement(oracle, layout, scale):
    for W, H in SIZES:
        info, co = oracle.read_jpeg(jpeg(layout, W, H))
        Ws, Hs = scaled_model.scaled_size(W, H, scale)
        rep = RS.component_planes(co, info, scale, filt=RS.replicate, clamp=False)
        comps = RS.components(co, info, scale)
        placed = [p for p, _ in comps]
        for c in range(info.ncomp):
            assert rep[c].shape == (Hs, Ws)
            if not overlapping_blocks(info, c):
                assert np.array_equal(rep[c], placed[c]), (layout, W, H, scale, c)
                continue
            # decode_mcu's rectangles overlap: what it shows of P_s' blocks is still P_s' blocks, wherever the sample lies inside P_s
            want = overwritten_placement(comps[c][1], info, c, 8 // scale, Ws, Hs)
            known = want != UNKNOWN
            assert known.any() and np.array_equal(placed[c][known], want[known]), (layout, W, H, scale, c)
        # ... and that placement is scaled_model's: it gives the reduced decode's bytes
        placed += [np.full((Hs, Ws), 0x80, np.int64)] * (3 - info.ncomp)
        for gray in (False, True):
            for a, e in zip(RS.rgb_of(placed, gray), scaled_model.decode_planes(co, info, scale, gray)):
                assert np.array_equal(a.reshape(-1), e), (layout, W, H, scale, gray)


@pytest.mark.parametrize("layout", SMOOTHED)
def test_plane_extent(oracle, layout):
    seen = 0
    for W, H in SIZES:
        info, co = oracle.read_jpeg(jpeg(layout, W, H))
        for scale in SCALES:
            Ws, Hs = scaled_model.scaled_size(W, H, scale)
            comps = RS.components(co, info, scale)
            for c in range(info.ncomp):
                f = smooth_model.factors(info, c)
                if f is None:
                    continue
                wc, hc = RS.plane_size(info, c, scale)
                assert (wc, hc) == (-(-Ws * info.H[c] // info.hmax), -(-Hs * info.V[c] // info.vmax)) == (-(-Ws // f[0]), -(-Hs // f[1]))
                assert comps[c][1].shape == (hc, wc)
                seen += 1
    assert seen >= 4 * len(SIZES)


def test_the_filter_changes_bytes_where_something_is_smoothed(oracle):
    """the reduced smooth decode is not the reduced nearest decode: a model that fell back to replication would pass (ii) and (iii)"""
    for layout in SMOOTHED:
        info, co = oracle.read_jpeg(jpeg(layout, 40, 24))
        for scale in (1, 2, 4):
            Ws, Hs = scaled_model.scaled_size(40, 24, scale)
            got = RS.decode_window(co, info, scale, (0, 0, Ws, Hs))
            want = scaled_model.decode_planes(co, info, scale)
            assert any(not np.array_equal(a, e) for a, e in zip(got, want)), (layout, scale)
