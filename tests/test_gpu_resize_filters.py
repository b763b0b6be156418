"""The resampling filters of the resized batch of windows on the GPU (include/jpezy_hip.h, BATCH OF WINDOWS, RESIZED, FILTERS):
box, bicubic and Lanczos through Context.decode_windows_resized_dev and Context.decode_windows_tensor_dev, in the two-pass tile and in the
direct loop.  The expectation is tests/resize_filter_model.py (the numpy restatement) applied to the bytes Context.decode_jpeg_region_packed
returns for the file's window, scale, gray and format.  The output buffer is pre-filled with a marker and compared as a whole, so padding
and the bytes behind the last slot are checked too.  Which files take the tile is predicted from the restatement's own y tables and
kResampleTileRows and compared with Context.last_resample_tiled_count.  There is no tolerance: every comparison is np.array_equal."""
import re
from pathlib import Path

import numpy as np
import pytest

import resize_filter_model as FM
import resize_model as RM
import tensor_model as TM
import test_gpu_region as TR
import test_gpu_windows as TW
import test_gpu_windows_resized as TZ

pytestmark = pytest.mark.gpu

FILL = TR.FILL
TAIL = 16
J, torch, ctx, own_files = TZ.J, TZ.torch, TZ.ctx, TZ.own_files        # the fixtures of the resized tests: the same six encoder-made files
TILE_H = 16
TILE_ROWS = int(re.search(r"constexpr int kResampleTileRows = (\d+);",
                          (Path(__file__).resolve().parent.parent / "jpezy_amd" / "csrc" / "jpezy_device.h").read_text()).group(1))
NEW_FILTERS = [FM.BOX, FM.BICUBIC, FM.LANCZOS]
FILTER_IDS = {FM.BILINEAR: "bilinear", FM.BOX: "box", FM.BICUBIC: "bicubic", FM.LANCZOS: "lanczos"}

_source = {}


def source(J, ctx, data, reg, scale, fmt, gray=False, smooth=False):
    """the bytes of the file's window as decode_jpeg_region_packed returns them (computed once per window, shared, read-only)"""
    key = (data, reg, scale, fmt, gray, smooth)
    if key not in _source:
        _, img = ctx.decode_jpeg_region_packed(data, reg, scale, fmt, gray, upsampling=J.UPSAMPLE_SMOOTH if smooth else J.UPSAMPLE_NEAREST)
        img.setflags(write=False)
        _source[key] = img
    return _source[key]


def fits_tile(filt, in_h, out_h):
    _, first, count, _ = FM.taps(filt, in_h, out_h, False)
    return FM.tile_span(first, count, TILE_H) <= TILE_ROWS


def run(J, torch, ctx, files, wins, out, fmt, filt, mirror=None, row_extra=0, slot_extra=0, direct=False, smooth=False, keyword=True):
    """one call into a marker-filled buffer; the WHOLE buffer is compared with the expectation.  Returns (the buffer as numpy, the files that
    the restatement's tables say fit the tile)."""
    n = len(files)
    ow, oh = out
    nb = 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4
    row = ow * nb + row_extra
    slot = oh * row + slot_extra
    buf = torch.full((n * slot + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    d_out = buf.as_strided((n, oh, ow, nb), (slot, row, nb, 1))
    kw = dict(filter=filt) if keyword else {}
    if smooth:
        kw["upsampling"] = J.UPSAMPLE_SMOOTH
    ctx.set_resample_direct(direct)
    try:
        res = ctx.decode_windows_resized_dev(files, d_out, wins, mirror, format=fmt, **kw)
    finally:
        ctx.set_resample_direct(0)
    got = buf.cpu().numpy()
    exp = np.full(n * slot + TAIL, FILL, np.uint8)
    fit = 0
    for k in range(n):
        _, placed, status = res[k]
        reg, scale = TW.resolve(files[k], None if wins is None else wins[k])
        assert status == 0 and placed == reg, (k, status, placed, reg)
        img = FM.resize(source(J, ctx, files[k], reg, scale, fmt, smooth=smooth), ow, oh, filt, bool(mirror[k]) if mirror is not None else False)
        for j in range(oh):
            exp[k * slot + j * row:k * slot + j * row + ow * nb] = img[j].reshape(-1)
        fit += fits_tile(filt, reg[3], oh)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, ("first differing byte", int(bad[0]), "slot", int(bad[0]) // slot, "of", n, "count", bad.size, "got", int(got[bad[0]]),
                           "want", int(exp[bad[0]]), out, FILTER_IDS[filt], "direct" if direct else "tile")
    want_tiled = 0 if direct or filt == FM.BILINEAR else fit
    assert ctx.last_resample_tiled_count() == want_tiled, (ctx.last_resample_tiled_count(), want_tiled, out)
    return got, fit


# ---- 1. bytes equal the restatement; the tile and the direct loop give the same bytes ------------------------------------------------------
# 24 x 20; exactly one tile; one past the tile on both axes (a last group of one pixel, single-byte stores); both axes of 17 x 33 grow;
# 3 x 2 and 1 x 1: 208 x 120 spans far more rows than the tile holds and takes the direct loop
OUTS = [(24, 20), (64, 16), (65, 17), (80, 70), (3, 2), (1, 1)]


@pytest.mark.parametrize("fmt_name, row_extra, slot_extra", [("PIX_RGB24", 1, 5), ("PIX_BGRA32", 8, 0)])
@pytest.mark.parametrize("filt", NEW_FILTERS, ids=[FILTER_IDS[f] for f in NEW_FILTERS])
def test_bytes_equal_the_restatement_in_both_forms(J, ctx, torch, own_files, filt, fmt_name, row_extra, slot_extra):
    """16 x 16 ... 208 x 120 whole, at full size and reduced, and a 17 x 33 window, to one size in one call, every second file mirrored"""
    fmt = getattr(J, fmt_name)
    files = list(own_files) + [own_files[4], own_files[5], own_files[3]]
    wins = [None] * 6 + [((0, 0, 17, 33), 1), ((0, 0, 0, 0), 2), ((3, 1, 52, 40), 1)]
    mirror = [k % 2 for k in range(len(files))]
    tiled_somewhere = direct_somewhere = False
    for out in OUTS:
        tile, fit = run(J, torch, ctx, files, wins, out, fmt, filt, mirror, row_extra, slot_extra)
        direct, _ = run(J, torch, ctx, files, wins, out, fmt, filt, mirror, row_extra, slot_extra, direct=True)
        assert np.array_equal(tile, direct), out
        assert ctx.last_batch_fast_count() == len(files)
        tiled_somewhere |= fit > 0
        direct_somewhere |= fit < len(files)
        if out in ((3, 2), (1, 1)):
            assert not fits_tile(filt, 120, out[1])
        if out == (80, 70):
            assert fit == len(files)                                # every axis of every file grows or shrinks by less than 2
    assert tiled_somewhere and direct_somewhere


# ---- 2. the capacity seam -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", NEW_FILTERS, ids=[FILTER_IDS[f] for f in NEW_FILTERS])
def test_the_capacity_seam(J, ctx, torch, own_files, filt):
    """two source heights for out_h = 32 whose largest tile span is exactly kResampleTileRows and one more, found from the tables: the
    first runs the tile, the second the direct loop, both give the restatement's bytes"""
    out = (40, 32)
    spans = {}
    for h in range(out[1], 121):
        _, first, count, _ = FM.taps(filt, h, out[1], False)
        spans.setdefault(FM.tile_span(first, count, TILE_H), h)
    assert TILE_ROWS in spans and TILE_ROWS + 1 in spans, sorted(spans)
    h_in, h_out = spans[TILE_ROWS], spans[TILE_ROWS + 1]
    f = own_files[5]
    _, fit = run(J, torch, ctx, [f], [((4, 0, 52, h_in), 1)], out, J.PIX_RGB24, filt)
    assert fit == 1
    _, fit = run(J, torch, ctx, [f], [((4, 0, 52, h_out), 1)], out, J.PIX_RGB24, filt)
    assert fit == 0
    _, fit = run(J, torch, ctx, [f, f, f], [((4, 0, 52, h_out), 1), ((4, 0, 52, h_in), 1), ((4, 0, 52, h_out), 1)], out, J.PIX_BGRA32, filt,
                 mirror=[1, 1, 0])
    assert fit == 1                                                 # both forms in one launch


# ---- 3. what resize_pick_window leaves is always tiled ------------------------------------------------------------------------------------
def test_lanczos_at_a_ratio_just_below_two_is_always_tiled(J, ctx, torch, own_files):
    f = own_files[5]
    for out_h in (16, 23, 33, 48, 60):
        h = 2 * out_h - 1
        assert fits_tile(FM.LANCZOS, h, out_h)
        _, fit = run(J, torch, ctx, [f, f], [((0, 0, 2 * 20 - 1, h), 1), ((7, 120 - h, 70, h), 1)], (20, out_h), J.PIX_RGB24, FM.LANCZOS, mirror=[0, 1])
        assert fit == 2


# ---- 4. a file on a child context is resampled with the parent's filter --------------------------------------------------------------------
def test_a_restart_interval_file_takes_the_parents_filter(J, ctx, torch, own_files):
    rst = TR.jpeg("own", 101, 70, restart=2)
    assert TR.parsed(rst)[0].restart_interval == 2
    files = [own_files[3], rst, own_files[1], rst]
    wins = [None, None, None, ((30, 9, 50, 29), 1)]
    got, fit = run(J, torch, ctx, files, wins, (60, 40), J.PIX_RGB24, FM.BICUBIC, mirror=[0, 1, 0, 0], row_extra=1)
    assert ctx.last_batch_fast_count() == 2                          # the restart-interval files went file by file ...
    assert fit == 4                                                  # ... and their tiles are counted in the parent's figure
    slot = 40 * (60 * 3 + 1)
    bilinear = RM.resize(source(J, ctx, rst, (0, 0, 101, 70), 1, J.PIX_RGB24), 60, 40, True)
    assert not np.array_equal(got[slot:slot + 60 * 3], bilinear[0].reshape(-1))          # (the child's own setting would give these)
    run(J, torch, ctx, files, wins, (9, 5), J.PIX_BGRA32, FM.LANCZOS, mirror=[0, 1, 0, 0])  # beyond the capacity: the direct loop there too


# ---- 5. the tensor path ---------------------------------------------------------------------------------------------------------------------
def test_bicubic_into_a_tensor(J, ctx, torch, own_files):
    """float32 NCHW with the normalisation of tensor_normalization, float16 channels_last, uint8 planar; every second file mirrored"""
    files = list(own_files) + [own_files[5]]
    wins = [None] * 6 + [((0, 0, 0, 0), 2)]
    n = len(files)
    mirror = [k % 2 for k in range(n)]
    scale, bias = J.tensor_normalization(TM.IMAGENET_MEAN, TM.IMAGENET_STD)
    for ow, oh in ((65, 17), (24, 20)):
        imgs = []
        for k in range(n):
            reg, sc = TW.resolve(files[k], wins[k])
            imgs.append(FM.resize(source(J, ctx, files[k], reg, sc, J.PIX_RGB24), ow, oh, FM.BICUBIC, bool(mirror[k])))
        fit = sum(fits_tile(FM.BICUBIC, TW.resolve(files[k], wins[k])[0][3], oh) for k in range(n))
        for dt, name, channels_last, norm in ((TM.DT_F32, "float32", False, True), (TM.DT_F16, "float16", True, False), (TM.DT_U8, "uint8", False, False)):
            st = (oh * ow * 3, 1, ow * 3, 3) if channels_last else (3 * oh * ow, oh * ow, ow, 1)
            eb = TM.ELEM_BYTES[dt]
            elems = n * 3 * oh * ow
            buf = torch.full((elems * eb + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
            d_out = buf[:elems * eb].view(getattr(torch, name)).as_strided((n, 3, oh, ow), st)
            assert not channels_last or d_out.is_contiguous(memory_format=torch.channels_last)
            s, b = (scale, bias) if norm else (None, None)
            for direct in (False, True):
                buf.fill_(FILL)
                ctx.set_resample_direct(direct)
                try:
                    res = ctx.decode_windows_tensor_dev(files, d_out, wins, mirror, s, b, filter=J.FILTER_BICUBIC)
                finally:
                    ctx.set_resample_direct(0)
                assert all(status == 0 for _, _, status in res)
                assert ctx.last_resample_tiled_count() == (0 if direct else fit) and fit > 0
                exp = np.full(elems * eb + TAIL, FILL, np.uint8)
                for k in range(n):
                    TM.place(exp[:elems * eb].view(TM.STORE[dt]), 0, st, k, imgs[k], dt, 3, s, b)
                assert np.array_equal(buf.cpu().numpy(), exp), (ow, oh, name, direct)


# ---- 6. the setting -------------------------------------------------------------------------------------------------------------------------
def test_the_setting_and_the_keyword(J, ctx, torch, own_files):
    fresh = J.Context(0)
    try:
        assert fresh.windows_filter() == J.FILTER_BILINEAR == 0     # the default
        fresh.set_windows_filter(J.FILTER_LANCZOS)
        for bad in (-1, 4, 77):
            with pytest.raises(J.JpezyError, match="JPEZY_FILTER_"):
                fresh.set_windows_filter(bad)
            assert fresh.windows_filter() == J.FILTER_LANCZOS       # a refusal leaves the setting as it was
    finally:
        fresh.close()
    files, out = list(own_files), (24, 20)
    assert ctx.windows_filter() == J.FILTER_BILINEAR
    # no keyword at all, and the keyword at FILTER_BILINEAR: the bytes of the existing restatement, in the existing kernels
    got_none, _ = run(J, torch, ctx, files, None, out, J.PIX_RGB24, FM.BILINEAR, row_extra=1, keyword=False)
    got_kw, _ = run(J, torch, ctx, files, None, out, J.PIX_RGB24, FM.BILINEAR, row_extra=1)
    assert np.array_equal(got_none, got_kw)
    row = out[0] * 3 + 1
    for k, f in enumerate(files):
        want = RM.resize(source(J, ctx, f, TW.resolve(f, None)[0], 1, J.PIX_RGB24), out[0], out[1])
        for j in range(out[1]):
            at = k * out[1] * row + j * row
            assert np.array_equal(got_none[at:at + out[0] * 3], want[j].reshape(-1)), (k, j)
    # the keyword holds for the call alone and is put back, also when the call raises
    ctx.set_windows_filter(J.FILTER_BOX)
    try:
        run(J, torch, ctx, files[:2], None, out, J.PIX_RGB24, FM.BICUBIC)
        assert ctx.windows_filter() == J.FILTER_BOX
        run(J, torch, ctx, files[:2], None, out, J.PIX_RGB24, FM.BOX, keyword=False)           # the context's setting is what runs
        d_out = torch.empty((1, out[1], out[0], 3), dtype=torch.uint8, device="cuda:0")
        with pytest.raises(J.JpezyError, match="file 0"):
            ctx.decode_windows_resized_dev([files[0][:100]], d_out, filter=J.FILTER_LANCZOS)
        assert ctx.windows_filter() == J.FILTER_BOX
        with pytest.raises(J.JpezyError, match="JPEZY_FILTER_"):
            ctx.decode_windows_resized_dev(files[:1], d_out, filter=9)
        assert ctx.windows_filter() == J.FILTER_BOX
    finally:
        ctx.set_windows_filter(J.FILTER_BILINEAR)
    # smooth chroma upsampling of the source window composes with the filter
    run(J, torch, ctx, files, None, (40, 30), J.PIX_RGB24, FM.BICUBIC, mirror=[1, 0, 1, 0, 1, 0], smooth=True)
