"""Smooth (triangle-filter) chroma upsampling on the GPU: every byte equal to the numpy restatement of the definition
(tests/smooth_model.py, anchored to the existing decode and to libjpeg-turbo by tests/test_smooth_model.py).  Varied: what selects
another path or another edge of the second stage -- the layout (which components are smoothed, by which rule, beside which placement),
planes of one and two samples, partial MCUs, MCU seams, a second workgroup, gray, the packed store stage, batches and strides, the exact
path of the first stage, the table cache, the Huffman head that ran."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import smooth_model as M
from jpeg_synth import synth_jpeg

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FILL = 0xA5
E_BADARG, E_UNSUPPORTED = -1, -4
LAYOUTS = {
    "own": [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
    "h2v1": [(2, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
    "h1v2": [(1, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
    "mixed": [(2, 2, 0, 0), (2, 1, 1, 1), (1, 2, 1, 1)],
    "411": [(4, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
    "444": [(1, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
    "one": [(1, 1, 0, 0)],
}
NOTHING_SMOOTHED = ("411", "444", "one")
# planes of one and two samples; one MCU, every edge at once; partial MCUs on both axes; neighbours across MCU seams; two workgroups
# across and a last thread with fewer than four pixels
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


# ---- files and references: made once, never modified ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jpeg(layout, W, H, precision=8):
    return synth_jpeg(W, H, LAYOUTS[layout], seed=3 * W + H, precision=precision)[0]


def parsed(data):
    """(FrameInfo, coefficients) by the host decoder: what every Huffman head here must deliver"""
    import jpezy_amd
    return jpezy_amd.read_jpeg(data)


@functools.lru_cache(maxsize=None)
def want(data, gray=False):
    info, co = parsed(data)
    out = M.decode_planes(co, info, gray)
    for a in out:
        a.setflags(write=False)
    return out


def dev_planes(torch, ctx, data, gray, upsampling=1):
    """read_jpeg_gpu -> dequant_idct_upsampling_dev into planes pre-filled with FILL and four bytes longer than needed"""
    info, d_co = ctx.read_jpeg_gpu(data)
    n = info.width * info.height
    out = [torch.full((n + 4,), FILL, dtype=torch.uint8, device=d_co.device) for _ in range(3)]
    ctx.dequant_idct_upsampling_dev(d_co, info, out[0], out[1], out[2], gray=gray, upsampling=upsampling)
    torch.cuda.synchronize()
    out = [o.cpu().numpy() for o in out]
    assert all((o[n:] == FILL).all() for o in out)
    return [o[:n] for o in out]


def _interleave(J, fmt, planes, H, W):
    nb = 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4
    order = (0, 1, 2) if fmt in (J.PIX_RGB24, J.PIX_RGBA32) else (2, 1, 0)
    img = np.full((H, W, nb), 0xFF, np.uint8)
    for k in range(3):
        img[..., k] = planes[order[k]].reshape(H, W)
    return img


# ---- 1. layouts x sizes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_layouts_and_sizes(J, ctx, torch, layout, size):
    W, H = size
    data = jpeg(layout, W, H)
    for gray in (False, True):
        e = want(data, gray)
        info, r, g, b = ctx.decode_jpeg(data, gray=gray, upsampling=J.UPSAMPLE_SMOOTH)
        assert (info.width, info.height) == (W, H)
        for a, x in zip((r, g, b), e):
            assert np.array_equal(a, x), ("decode_jpeg", layout, size, gray)
        for a, x in zip(dev_planes(torch, ctx, data, gray), e):
            assert np.array_equal(a, x), ("dequant_idct_upsampling_dev", layout, size, gray)
        if layout in NOTHING_SMOOTHED:                              # no smoothed component: byte for byte the existing decode
            for a, x in zip(ctx.decode_jpeg(data, gray=gray)[1:], e):
                assert np.array_equal(a, x), ("existing decode", layout, size, gray)
    if layout not in NOTHING_SMOOTHED and W >= 16:                   # ... and with one, not the existing decode
        assert any(not np.array_equal(a, x) for a, x in zip(ctx.decode_jpeg(data)[1:], want(data)))


def test_native_plane_is_the_ycc_decode(J, ctx):
    """P of the definition: exactly the bytes decode_jpeg_ycc returns for the component"""
    for layout in ("h2v1", "h1v2", "own"):
        data = jpeg(layout, 33, 17)
        info, co = parsed(data)
        _, y, cb, cr = ctx.decode_jpeg_ycc(data)
        for c, got in enumerate((y, cb, cr)):
            assert np.array_equal(got, M.native_plane(co, info, c)), (layout, c)


# ---- 2. packed pixels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 3])
@pytest.mark.parametrize("layout", ["own", "mixed"])
def test_packed_with_row_padding(J, ctx, torch, layout, fmt):
    assert (J.PIX_RGB24, J.PIX_BGRA32) == (0, 3)
    W, H = 33, 17
    data = jpeg(layout, W, H)
    dev = torch.device("cuda", 0)
    info, d_co = ctx.read_jpeg_gpu(data)
    for gray in (False, True):
        e = _interleave(J, fmt, want(data, gray), H, W)
        nb = e.shape[2]
        rs = W * nb + 7
        buf = torch.full((H * rs + 16,), FILL, dtype=torch.uint8, device=dev)
        ctx.dequant_idct_upsampling_dev(d_co, info, gray=gray, d_img=buf.as_strided((H, W, nb), (rs, nb, 1)), format=fmt)
        torch.cuda.synchronize()
        a = buf.cpu().numpy()
        rows = a[: H * rs].reshape(H, rs)
        assert np.array_equal(rows[:, : W * nb].reshape(H, W, nb), e), (layout, fmt, gray)
        assert (rows[:, W * nb:] == FILL).all() and (a[H * rs:] == FILL).all()
        if nb == 4:
            assert (rows[:, : W * nb].reshape(H, W, nb)[..., 3] == 0xFF).all()
        _, img = ctx.decode_jpeg_packed(data, format=fmt, gray=gray, upsampling=J.UPSAMPLE_SMOOTH)
        assert np.array_equal(img, e), ("host", layout, fmt, gray)
    # the aligned store forms: 16 x 16 tight (every thread four pixels on a 4-byte boundary)
    data = jpeg(layout, 16, 16)
    _, img = ctx.decode_jpeg_packed(data, format=fmt, upsampling=J.UPSAMPLE_SMOOTH)
    assert np.array_equal(img, _interleave(J, fmt, want(data), 16, 16))


# ---- 3. the device entry ---------------------------------------------------------------------------------------------------------
def _two_frames(data):
    """the file's coefficients and a sign-flipped copy: (FrameInfo, int16 [2, n])"""
    info, co = parsed(data)
    co = co.reshape(-1).astype(np.int32)
    return info, np.stack([co, -co]).astype(np.int16)


def _batch(torch, ctx, info, frames, gray=False):
    W, H = info.width, info.height
    dev = torch.device("cuda", 0)
    stride = W * H + 52                                           # larger than the plane, a multiple of 4
    assert stride % 4 == 0
    d_co = torch.from_numpy(frames).to(dev)
    out = [torch.full((2 * stride,), FILL, dtype=torch.uint8, device=dev) for _ in range(3)]
    ctx.dequant_idct_upsampling_dev(d_co, info, out[0], out[1], out[2], gray=gray, n_frames=2, plane_stride=stride)
    torch.cuda.synchronize()
    out = [o.cpu().numpy().reshape(2, stride) for o in out]
    for f in range(2):
        for a, e in zip(out, M.decode_planes(frames[f], info, gray)):
            assert np.array_equal(a[f, : W * H], e), (f, gray)
    assert all((a[:, W * H:] == FILL).all() for a in out)


def test_device_batch_with_padded_stride(J, ctx, torch):
    info, frames = _two_frames(jpeg("own", 40, 24))
    for gray in (False, True):
        _batch(torch, ctx, info, frames, gray)


def test_device_batch_force_exact(J, torch):
    """every block through the first stage's reference-order path: the same samples, so the same bytes"""
    info, frames = _two_frames(jpeg("mixed", 40, 24))
    c = J.Context(0)
    try:
        c.set_force_exact(1)
        _batch(torch, c, info, frames)
        assert c.fallback_count() > 0
    finally:
        c.close()


def test_two_layouts_on_one_context(J, torch):
    """different layouts and quantiser tables one after the other, and the first again: the context's table cache"""
    c = J.Context(0)
    try:
        for layout in ("h2v1", "h1v2", "h2v1", "own"):
            data = jpeg(layout, 33, 17)
            for a, e in zip(dev_planes(torch, c, data, False), want(data)):
                assert np.array_equal(a, e), layout
    finally:
        c.close()


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def own_file(J, ctx, oracle):
    W, H = 208, 120
    r, g, b = oracle.synth_rgb(W, H, frame=7)
    return ctx.encode_jpeg(r, g, b, W, H)


@pytest.mark.parametrize("head", ["gpu", "host"])
def test_end_to_end_both_huffman_heads(J, own_file, head):
    c = J.Context(0)
    try:
        if head == "gpu":
            c.set_huffdec_min_bytes(0)
        for gray in (False, True):
            info, r, g, b = c.decode_jpeg(own_file, gray=gray, upsampling=J.UPSAMPLE_SMOOTH)
            assert (info.width, info.height) == (208, 120)
            assert (c.last_huffdec_passes() > 0) == (head == "gpu")
            for a, e in zip((r, g, b), want(own_file, gray)):
                assert np.array_equal(a, e), (head, gray)
    finally:
        c.close()


def test_decoder_class_and_cli(J, ctx, oracle, own_file, tmp_path):
    W, H = 208, 120
    path = tmp_path / "a.jpg"
    path.write_bytes(own_file)
    dec = J.Decoder(str(path), ctx=ctx)
    for gray in (False, True):
        got = dec.decode(gray=gray, upsampling=J.UPSAMPLE_SMOOTH)
        assert (dec.pr.width, dec.pr.height) == (W, H)
        assert all(np.array_equal(a, e) for a, e in zip(got, want(own_file, gray)))
    from jpezy_amd import _build
    _build.build_all()
    exe = ROOT / "jpezy_amd" / "bin" / "jpezy_decode"
    for opts, gray in ((["--upsampling=smooth"], False), (["--gray", "--upsampling=smooth"], True), (["--upsampling=smooth", "--scale=1"], False)):
        ppm = tmp_path / "y.ppm"
        p = subprocess.run([str(exe), str(path), str(ppm), *opts], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert ppm.read_bytes() == oracle.format_ppm_p3(W, H, *want(own_file, gray)), opts
        assert f"Decoded image: Netpbm image data, size = {W} x {H}, pixmap, ASCII text" in p.stdout
        ppm.unlink()
    p = subprocess.run([str(exe), str(path), str(tmp_path / "n.ppm"), "--upsampling=nearest"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert (tmp_path / "n.ppm").read_bytes() == oracle.format_ppm_p3(W, H, *ctx.decode_jpeg(own_file)[1:])


# ---- 5. UPSAMPLE_NEAREST is the existing decode -----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["own", "h2v1", "411"])
def test_nearest_is_the_existing_decode(J, ctx, torch, layout):
    W, H = 33, 17
    data = jpeg(layout, W, H)
    dev = torch.device("cuda", 0)
    for gray in (False, True):
        info, r, g, b = ctx.decode_jpeg(data, gray=gray)
        rgb = (r, g, b)
        _, r1, g1, b1 = ctx.decode_jpeg_upsampling(data, J.UPSAMPLE_NEAREST, gray=gray)                  # jpezy_decode_jpeg_upsampling
        assert all(np.array_equal(a, e) for a, e in zip((r1, g1, b1), rgb))
        _, img = ctx.decode_jpeg_upsampling_packed(data, J.UPSAMPLE_NEAREST, format=J.PIX_BGR24, gray=gray)   # ..._upsampling_packed
        assert np.array_equal(img, _interleave(J, J.PIX_BGR24, rgb, H, W))
        for a, e in zip(dev_planes(torch, ctx, data, gray, upsampling=J.UPSAMPLE_NEAREST), rgb):       # jpezy_dequant_idct_upsampling_dev
            assert np.array_equal(a, e)
        info, d_co = ctx.read_jpeg_gpu(data)
        d_img = torch.full((H, W, 4), FILL, dtype=torch.uint8, device=dev)                              # ..._upsampling_packed_dev
        ctx.dequant_idct_upsampling_dev(d_co, info, gray=gray, d_img=d_img, format=J.PIX_RGBA32, upsampling=J.UPSAMPLE_NEAREST)
        torch.cuda.synchronize()
        assert np.array_equal(d_img.cpu().numpy(), _interleave(J, J.PIX_RGBA32, rgb, H, W))
    info, frames = _two_frames(data)                                                                    # n_frames > 1: the batch entry
    stride = W * H + 3
    stride += -stride % 4
    d_co = torch.from_numpy(frames).to(dev)
    got = [torch.full((2 * stride,), FILL, dtype=torch.uint8, device=dev) for _ in range(3)]
    ref = [torch.full((2 * stride,), FILL, dtype=torch.uint8, device=dev) for _ in range(3)]
    ctx.dequant_idct_upsampling_dev(d_co, info, got[0], got[1], got[2], n_frames=2, plane_stride=stride, upsampling=J.UPSAMPLE_NEAREST)
    ctx.dequant_idct_scaled_dev(d_co, info, 1, ref[0], ref[1], ref[2], n_frames=2, plane_stride=stride)
    torch.cuda.synchronize()
    assert all(torch.equal(a, e) for a, e in zip(got, ref))


# ---- 6. refusals leave the context usable -----------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(J, torch, tmp_path):
    c = J.Context(0)
    try:
        data = jpeg("own", 33, 17)

        def still_decodes():
            for a, e in zip(c.decode_jpeg(data, upsampling=J.UPSAMPLE_SMOOTH)[1:], want(data)):
                assert np.array_equal(a, e)
            for a, e in zip(dev_planes(torch, c, data, False), want(data)):
                assert np.array_equal(a, e)

        still_decodes()
        for bad in (2, -1, 100):                                                      # a bad upsampling value
            with pytest.raises(J.JpezyError, match=f"status {E_BADARG}.*upsampling"):
                c.decode_jpeg(data, upsampling=bad)
            with pytest.raises(J.JpezyError, match=f"status {E_BADARG}.*upsampling"):
                c.decode_jpeg_packed(data, upsampling=bad)
            info, d_co = c.read_jpeg_gpu(data)
            out = [torch.full((33 * 17,), FILL, dtype=torch.uint8, device=d_co.device) for _ in range(3)]
            with pytest.raises(J.JpezyError, match=f"status {E_BADARG}.*upsampling"):
                c.dequant_idct_upsampling_dev(d_co, info, out[0], out[1], out[2], upsampling=bad)
            torch.cuda.synchronize()
            assert all((o == FILL).all() for o in out)
            still_decodes()
        deep = jpeg("own", 33, 17, precision=12)                                      # a 12-bit file
        assert parsed(deep)[0].precision == 12
        planes = c.decode_jpeg(deep)[1:]                                              # ... which the existing decode takes
        with pytest.raises(J.JpezyError, match=f"status {E_UNSUPPORTED}.*8-bit"):
            c.decode_jpeg(deep, upsampling=J.UPSAMPLE_SMOOTH)
        with pytest.raises(J.JpezyError, match=f"status {E_UNSUPPORTED}.*8-bit"):
            c.decode_jpeg_packed(deep, upsampling=J.UPSAMPLE_SMOOTH)
        info, d_co = c.read_jpeg_gpu(deep)
        out = [torch.full((33 * 17,), FILL, dtype=torch.uint8, device=d_co.device) for _ in range(3)]
        with pytest.raises(J.JpezyError, match=f"status {E_UNSUPPORTED}.*8-bit"):
            c.dequant_idct_upsampling_dev(d_co, info, out[0], out[1], out[2])
        for a, e in zip(c.decode_jpeg_upsampling(deep, J.UPSAMPLE_NEAREST)[1:], planes):
            assert np.array_equal(a, e)
        still_decodes()
        path = tmp_path / "a.jpg"                                                     # scale = 2 together with smooth
        path.write_bytes(data)
        dec = J.Decoder(str(path), ctx=c)
        with pytest.raises(J.JpezyError, match=f"status {E_UNSUPPORTED}"):
            dec.decode(scale=2, upsampling=J.UPSAMPLE_SMOOTH)
        with pytest.raises(J.JpezyError, match=f"status {E_UNSUPPORTED}"):
            dec.decode(region=(0, 0, 4, 4), upsampling=J.UPSAMPLE_SMOOTH)
        assert all(np.array_equal(a, e) for a, e in zip(dec.decode(upsampling=J.UPSAMPLE_SMOOTH), want(data)))
        still_decodes()
    finally:
        c.close()


# ---- 7. quality, end to end ------------------------------------------------------------------------------------------------------
def test_centred_chroma_comes_back_closer(J):
    """a picture whose chroma is a ramp sited at the centre of its 2 x 2 (tests/test_smooth_model.py checks the premise on the CPU),
    through encode_jpeg_ycc at quality 100: away from the outer two pixels the smooth decode's Cb is no further from the ramp at its
    maximum and strictly closer on average than the replicated decode's"""
    y, cb, cr, cb_full = M.centred_ramp_picture()
    c = J.Context(0)
    try:
        c.set_quality(100)
        data = c.encode_jpeg_ycc(y, cb, cr)
        err = {}
        for name, up in (("smooth", J.UPSAMPLE_SMOOTH), ("nearest", J.UPSAMPLE_NEAREST)):
            info, img = c.decode_jpeg_packed(data, format=J.PIX_RGB24, upsampling=up)
            assert img.shape == (48, 64, 3)
            err[name] = np.abs(M.cb_of_rgb(img[..., 0], img[..., 1], img[..., 2]) - cb_full)[2:-2, 2:-2]
        info, co = parsed(data)
        assert np.array_equal(img.reshape(-1, 3), np.stack(c.decode_jpeg(data)[1:], axis=-1))
        smooth = c.decode_jpeg_packed(data, upsampling=J.UPSAMPLE_SMOOTH)[1]
        assert np.array_equal(smooth.reshape(-1, 3), np.stack(M.decode_planes(co, info), axis=-1))
    finally:
        c.close()
    print({k: (float(v.max()), float(v.mean())) for k, v in err.items()})
    assert err["smooth"].max() <= err["nearest"].max()
    assert err["smooth"].mean() < err["nearest"].mean()
