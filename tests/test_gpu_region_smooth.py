"""Region decode with smooth chroma upsampling on the GPU (include/jpezy_hip.h, SMOOTH UPSAMPLING OF WINDOWS): every byte equal to the
slice of the numpy restatement (tests/region_smooth_model.py, anchored by tests/test_region_smooth_model.py), at scale 1 also to the slice
of decode_jpeg_upsampling_packed, and with nothing smoothed also to the nearest region decode.  Varied: what a kernel that reads a ring
around its MCU can get wrong -- the layout, N, gray, windows at the picture's corners (the clamp), around an interior MCU corner (the
diagonal neighbour), at a plane that ends mid-block, store forms, strides, batches, the Huffman head that ran.  Files are read once per
case (read_jpeg_gpu) and many windows go through the device entry into buffers pre-filled with a marker byte and four bytes longer than
needed.  There is no tolerance: every comparison is np.array_equal."""
import io

import numpy as np
import pytest

import region_smooth_cases as K
import scaled_model as M

pytestmark = pytest.mark.gpu

FILL = K.FILL
SIZES = [(1, 1), (2, 2), (3, 3), (16, 16), (33, 17), (17, 33), (40, 24), (260, 5)]


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def run_planar(J, torch, ctx, d_co, info, region, scale, gray, upsampling, n_frames=1, stride=None):
    """-> three uint8 arrays [n_frames, stride] after the four bytes behind the last frame were checked"""
    w, h = region[2], region[3]
    stride = w * h if stride is None else stride
    out = [torch.full((n_frames * stride + 4,), FILL, dtype=torch.uint8, device=d_co.device) for _ in range(3)]
    ctx.dequant_idct_region_dev(d_co, info, region, scale, out[0], out[1], out[2], gray=gray, n_frames=n_frames, plane_stride=stride,
                                upsampling=upsampling)
    torch.cuda.synchronize()
    out = [o.cpu().numpy() for o in out]
    assert all((o[-4:] == FILL).all() for o in out), ("bytes behind the output written", region, scale, gray)
    return [o[:-4].reshape(n_frames, stride) for o in out]


# ---- parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", sorted(K.LAYOUTS))
def test_every_window_is_the_models(J, torch, ctx, layout):
    checked = 0
    for W, H in SIZES:
        data = K.jpeg(layout, W, H)
        info, d_co = ctx.read_jpeg_gpu(data)
        # scale 1: the whole-picture smooth decode, through the file entry
        full = {g: ctx.decode_jpeg_upsampling_packed(data, J.UPSAMPLE_SMOOTH, gray=g)[1] for g in (False, True)}
        for scale in K.SCALES:
            for name, region in K.windows(info, scale).items():
                x, y, w, h = region
                for gray in (False, True):
                    got = run_planar(J, torch, ctx, d_co, info, region, scale, gray, J.UPSAMPLE_SMOOTH)
                    tag = (layout, W, H, scale, name, region, gray)
                    for a, e in zip(got, K.want(data, region, scale, gray)):
                        assert np.array_equal(a[0].reshape(h, w), e), tag
                    if scale == 1:
                        for k in range(3):
                            assert np.array_equal(got[k][0].reshape(h, w), full[gray][y:y + h, x:x + w, k]), tag
                    if layout in K.NOTHING_SMOOTHED:
                        near = run_planar(J, torch, ctx, d_co, info, region, scale, gray, J.UPSAMPLE_NEAREST)
                        for a, e in zip(got, near):
                            assert np.array_equal(a, e), tag
                    checked += 1
    assert checked >= len(SIZES) * len(K.SCALES) * 2 * 7


def test_smooth_differs_from_nearest_where_something_is_smoothed(J, torch, ctx):
    """a build that quietly ran region_kernel would pass every comparison of a layout with nothing smoothed"""
    for layout in ("own", "h2v1", "h1v2", "mixed", "two_chroma_blocks"):
        data = K.jpeg(layout, 40, 24)
        info, d_co = ctx.read_jpeg_gpu(data)
        for scale in (1, 2, 4):
            region = (0, 0) + M.scaled_size(40, 24, scale)
            a = run_planar(J, torch, ctx, d_co, info, region, scale, False, J.UPSAMPLE_SMOOTH)
            b = run_planar(J, torch, ctx, d_co, info, region, scale, False, J.UPSAMPLE_NEAREST)
            assert any(not np.array_equal(p, q) for p, q in zip(a, b)), (layout, scale)


@pytest.mark.parametrize("layout", ["own", "mixed", "two_chroma_blocks", "444"])
def test_packed_formats_with_a_padded_row_stride(J, torch, ctx, layout):
    data = K.jpeg(layout, 40, 24)
    info, d_co = ctx.read_jpeg_gpu(data)
    for fmt in (J.PIX_RGB24, J.PIX_BGR24, J.PIX_RGBA32, J.PIX_BGRA32):
        nb = 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4
        for scale in K.SCALES:
            for name, region in K.windows(info, scale).items():
                x, y, w, h = region
                row = w * nb + 5                                          # rows start at every alignment: both store forms
                buf = torch.full((h * row + 4,), FILL, dtype=torch.uint8, device="cuda:0")
                d_img = buf.as_strided((h, w, nb), (row, nb, 1))
                ctx.dequant_idct_region_dev(d_co, info, region, scale, d_img=d_img, format=fmt, upsampling=J.UPSAMPLE_SMOOTH)
                torch.cuda.synchronize()
                exp = np.full(h * row + 4, FILL, np.uint8)
                img = K.interleave(J, fmt, K.want(data, region, scale, False))
                for j in range(h):
                    exp[j * row:j * row + w * nb] = img[j].reshape(-1)
                assert np.array_equal(buf.cpu().numpy(), exp), (layout, fmt, scale, name, region)


def test_three_frames_with_a_plane_stride(J, torch, ctx):
    for layout, (W, H) in (("own", (33, 17)), ("two_chroma_blocks", (40, 24))):
        files = [K.jpeg(layout, W, H, seed=50 + k, fixed_qt=True) for k in range(3)]
        parts = [ctx.read_jpeg_gpu(f) for f in files]
        info = parts[0][0]
        d_co = torch.cat([p[1].reshape(-1) for p in parts])
        for scale in K.SCALES:
            for name in ("whole", "mcu_corner_11", "odd_start_odd_size", "last_column"):
                region = K.windows(info, scale).get(name)
                if region is None:
                    continue
                w, h = region[2], region[3]
                stride = w * h + 3
                got = run_planar(J, torch, ctx, d_co, info, region, scale, False, J.UPSAMPLE_SMOOTH, n_frames=3, stride=stride)
                for f in range(3):
                    for a, e in zip(got, K.want(files[f], region, scale, False)):
                        assert np.array_equal(a[f, :w * h].reshape(h, w), e), (layout, scale, name, f)
                        assert (a[f, w * h:] == FILL).all(), (layout, scale, name, f)


# ---- the file entries --------------------------------------------------------------------------------------------------------
def pillow_file(subsampling, W=70, H=52):
    from PIL import Image
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(4)
    rgb = np.stack([np.clip(128 + 100 * np.sin((xx * (c + 1) + yy * (4 - c)) / 5.0) + rng.integers(-30, 31, (H, W)), 0, 255) for c in range(3)], axis=-1)
    buf = io.BytesIO()
    Image.fromarray(rgb.astype(np.uint8)).save(buf, "JPEG", quality=85, subsampling=subsampling)
    return buf.getvalue()


def check_file_entries(J, ctx, data, tag, scales=K.SCALES):
    info = K.parsed(data)[0]
    full = ctx.decode_jpeg_upsampling_packed(data, J.UPSAMPLE_SMOOTH)[1]
    for scale in scales:
        for name, region in K.windows(info, scale).items():
            x, y, w, h = region
            fi, r, g, b = ctx.decode_jpeg_region(data, region, scale=scale, upsampling=J.UPSAMPLE_SMOOTH)
            assert (fi.width, fi.height) == (info.width, info.height)
            e = K.want(data, region, scale, False)
            for a, q in zip((r, g, b), e):
                assert np.array_equal(a.reshape(h, w), q), (tag, scale, name, region)
            for fmt in (J.PIX_RGB24, J.PIX_BGRA32):
                _, img = ctx.decode_jpeg_region_packed(data, region, scale=scale, format=fmt, upsampling=J.UPSAMPLE_SMOOTH)
                assert np.array_equal(img, K.interleave(J, fmt, e)), (tag, scale, name, region, fmt)
            if scale == 1:
                assert np.array_equal(np.stack([r, g, b], axis=-1).reshape(h, w, 3), full[y:y + h, x:x + w]), (tag, name)


def test_file_entries_on_a_synthesised_file(J, ctx):
    check_file_entries(J, ctx, K.jpeg("mixed", 40, 24), "mixed")


@pytest.mark.parametrize("subsampling", [2, 1], ids=["420", "422"])
def test_file_entries_on_a_pillow_file(J, ctx, subsampling):
    check_file_entries(J, ctx, pillow_file(subsampling), subsampling)


def test_file_entries_on_a_restart_interval_file(J, ctx):
    data = K.jpeg("own", 40, 24, restart=2)
    assert K.parsed(data)[0].restart_interval == 2                       # the host Huffman head
    check_file_entries(J, ctx, data, "restart")


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_destination_and_the_context_alone(J, torch, ctx):
    data = K.jpeg("own", 40, 24)
    info, d_co = ctx.read_jpeg_gpu(data)
    out = [torch.full((40 * 24 + 4,), FILL, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    with pytest.raises(J.JpezyError, match="upsampling must be"):
        ctx.dequant_idct_region_dev(d_co, info, (0, 0, 8, 8), 1, *out, upsampling=2)
    for region, scale in (((33, 0, 8, 8), 1), ((0, 0, 21, 12), 2), ((0, 0, 5, 4), 8)):       # outside the picture: as today
        with pytest.raises(J.JpezyError, match="status -1: .*lies outside the picture"):
            ctx.dequant_idct_region_dev(d_co, info, region, scale, *out, upsampling=J.UPSAMPLE_SMOOTH)
        with pytest.raises(J.JpezyError, match="status -1: .*lies outside the picture"):
            ctx.decode_jpeg_region(data, region, scale=scale, upsampling=J.UPSAMPLE_SMOOTH)
    with pytest.raises(J.JpezyError, match="upsampling must be"):
        ctx.decode_jpeg_region_packed(data, (0, 0, 8, 8), upsampling=-1)
    # a 12-bit file: refused by the file entries once the header is read, and by the device entries by its precision
    data12 = K.jpeg("own", 40, 24, precision=12)
    for call in (lambda: ctx.decode_jpeg_region(data12, (0, 0, 8, 8), upsampling=J.UPSAMPLE_SMOOTH),
                 lambda: ctx.decode_jpeg_region_packed(data12, (0, 0, 8, 8), scale=2, upsampling=J.UPSAMPLE_SMOOTH)):
        with pytest.raises(J.JpezyError, match="status -4: .*8-bit"):
            call()
    info12, d_co12 = ctx.read_jpeg_gpu(data12)
    assert info12.precision == 12
    with pytest.raises(J.JpezyError, match="status -4: .*8-bit"):
        ctx.dequant_idct_region_dev(d_co12, info12, (0, 0, 8, 8), 1, *out, upsampling=J.UPSAMPLE_SMOOTH)
    ctx.decode_jpeg_region(data12, (0, 0, 8, 8))                          # nearest decodes it, as today
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == FILL).all() for o in out)
    # the context is usable afterwards
    got = run_planar(J, torch, ctx, d_co, info, (3, 5, 30, 17), 1, False, J.UPSAMPLE_SMOOTH)
    for a, e in zip(got, K.want(data, (3, 5, 30, 17), 1, False)):
        assert np.array_equal(a[0].reshape(17, 30), e)
