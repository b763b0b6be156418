"""Packed (interleaved) RGB / BGR / RGBA / BGRA pixels: encode from and decode to one buffer, bit-identical to the planar entry points
and to the oracle.  Only the first (pixel load) and last (pixel store) step of the kernels differ from the planar path, so every test
demands equality; what is varied is what selects another load / store form: the format, W % 16, row and frame strides, the base
address, the workgroup shape (quads per row), gray, the encode variant, the exact-path hooks.

Buffers are built here from oracle.synth_rgb planes; padding, the bytes in front of an offset base and the canaries behind the last row
are 0xA5 and must still be after a decode."""
import ctypes as C
import functools

import numpy as np
import pytest

from jpeg_synth import synth_jpeg

pytestmark = pytest.mark.gpu

FILL = 0xA5
E_BADARG, E_NOSPACE = -1, -6
UNALIGNED = [(1, 1), (7, 5), (15, 17), (65, 47), (100, 100)]
TWO_WAVE = [(16, 16), (64, 16), (1920, 24)]                  # aligned, quads per row not a multiple of 4
FOUR_WAVE = [(1024, 16), (976, 33), (208, 40), (2048, 7)]    # aligned; 976: last quad with one live MCU; 2048x7: a band shorter than an MCU row
L444 = [(1, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]
L422 = [(2, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]
L400 = [(1, 1, 0, 0)]


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


def formats(J):
    return [J.PIX_RGB24, J.PIX_BGR24, J.PIX_RGBA32, J.PIX_BGRA32]


def layout(fmt):
    """(bytes per pixel, byte of r, g, b inside a pixel)"""
    return (3 if fmt < 2 else 4), ((0, 1, 2) if fmt in (0, 2) else (2, 1, 0))


# ---- references: computed once per (size, frame, gray), never modified -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planes(W, H, frame=0):
    from oracle import oracle as O
    p = O.synth_rgb(W, H, frame=frame)
    for a in p:
        a.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def ref_coeffs(W, H, frame=0, gray=False):
    from oracle import oracle as O
    co = O.encode_coeffs(*planes(W, H, frame), W, H, gray=gray).reshape(-1)
    co.setflags(write=False)
    return co


@functools.lru_cache(maxsize=None)
def ref_decoded(W, H, gray=False):
    from oracle import oracle as O
    out = O.decode_planes(ref_coeffs(W, H), O.make_info(W, H), gray)
    for a in out:
        a.setflags(write=False)
    return tuple(out)


def interleave(rgb, W, H, fmt, alpha=0xFF):
    nb, off = layout(fmt)
    img = np.full((H, W, nb), alpha, np.uint8)
    for p, o in zip(rgb, off):
        img[:, :, o] = np.asarray(p).reshape(H, W)
    return img


def strides_for(kind, W, nb):
    tight = W * nb
    return {"tight": tight, "pad16": (tight + 15) // 16 * 16 + 16, "pad5": tight + 5}[kind]


def packed_buffer(frames, W, H, fmt, row_stride, base=0, frame_stride=None, alpha=None, tail=64):
    """host buffer (0xA5 everywhere but the pixels) holding the frames (lists of planes); returns (buffer, frame_stride)"""
    nb, _ = layout(fmt)
    need = (H - 1) * row_stride + W * nb
    fs = frame_stride if frame_stride is not None else H * row_stride
    buf = np.full(base + (len(frames) - 1) * fs + need + tail, FILL, np.uint8)
    for f, rgb in enumerate(frames):
        img = interleave(rgb, W, H, fmt)
        if nb == 4:
            img[:, :, 3] = alpha if alpha is not None else 0
        v = np.lib.stride_tricks.as_strided(buf[base + f * fs:], (H, W, nb), (row_stride, nb, 1))
        v[...] = img
    return buf, fs


def device_view(torch, flat, n, W, H, nb, row_stride, frame_stride, base=0):
    if n == 1:
        return torch.as_strided(flat, (H, W, nb), (row_stride, nb, 1), base)
    return torch.as_strided(flat, (n, H, W, nb), (frame_stride, row_stride, nb, 1), base)


def encode_packed(J, ctx, torch, frames, W, H, fmt, row_stride, gray, base=0, frame_stride=None, alpha=None):
    nb, _ = layout(fmt)
    buf, fs = packed_buffer(frames, W, H, fmt, row_stride, base, frame_stride, alpha)
    flat = torch.from_numpy(buf).to("cuda:0")
    co = torch.empty(len(frames) * J.coeff_count(W, H, gray), dtype=torch.int16, device="cuda:0")
    ctx.fdct_quant_packed_dev(device_view(torch, flat, len(frames), W, H, nb, row_stride, fs, base), co, format=fmt, gray=gray)
    torch.cuda.synchronize()
    assert np.array_equal(flat.cpu().numpy(), buf), "the encoder wrote into its input"
    return co.cpu().numpy()


# ---- 1. encode parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", UNALIGNED + TWO_WAVE + FOUR_WAVE)
def test_encode_equals_oracle_and_planar(J, ctx, torch, size):
    W, H = size
    rgb = planes(W, H)
    for gray in (False, True):
        want = ref_coeffs(W, H, 0, gray)
        assert np.array_equal(ctx.fdct_quant(*rgb, W, H, gray=gray).reshape(-1), want), ("planar", size, gray)
        for variant in (0, 1):
            ctx.set_variant(variant)
            try:
                for fmt in formats(J):
                    got = encode_packed(J, ctx, torch, [rgb], W, H, fmt, W * layout(fmt)[0], gray)
                    assert np.array_equal(got, want), (size, gray, variant, fmt)
            finally:
                ctx.set_variant(1)


@pytest.mark.parametrize("size", [(64, 16), (65, 47), (1024, 16)])
@pytest.mark.parametrize("kind", ["tight", "pad16", "pad5", "base4", "frames3"])
def test_encode_strides_and_base(J, ctx, torch, size, kind):
    """pad16 keeps the 16-byte load form with padded rows; pad5 and a base 4 bytes into the allocation take the byte loop although
    W % 16 == 0; three frames lie frame_stride = H * row_stride + 48 apart"""
    W, H = size
    for fmt in formats(J):
        nb, _ = layout(fmt)
        rs = strides_for(kind if kind in ("tight", "pad16", "pad5") else "tight", W, nb)
        nfr = 3 if kind == "frames3" else 1
        frames = [planes(W, H, f) for f in range(nfr)]
        for gray in (False, True):
            want = np.concatenate([ref_coeffs(W, H, f, gray) for f in range(nfr)])
            for variant in (0, 1):
                ctx.set_variant(variant)
                try:
                    got = encode_packed(J, ctx, torch, frames, W, H, fmt, rs, gray, base=4 if kind == "base4" else 0,
                                        frame_stride=H * rs + 48 if kind == "frames3" else None)
                finally:
                    ctx.set_variant(1)
                assert np.array_equal(got, want), (size, kind, fmt, gray, variant)


@pytest.mark.parametrize("force", [0, 1, 2, 3])
def test_encode_force_exact(J, ctx, torch, force):
    W, H = 80, 48
    rgb = planes(W, H)
    try:
        ctx.set_force_exact(force)
        for fmt in (J.PIX_RGB24, J.PIX_BGRA32):
            for gray in (False, True):
                for variant in (0, 1):
                    ctx.set_variant(variant)
                    for rs in (strides_for("tight", W, layout(fmt)[0]), strides_for("pad5", W, layout(fmt)[0])):
                        got = encode_packed(J, ctx, torch, [rgb], W, H, fmt, rs, gray)
                        assert np.array_equal(got, ref_coeffs(W, H, 0, gray)), (force, fmt, gray, variant, rs)
    finally:
        ctx.set_force_exact(0)
        ctx.set_variant(1)
        ctx.fallback_count()


@pytest.mark.parametrize("size", [(64, 16), (65, 47)])
def test_encode_ignores_the_fourth_byte(J, ctx, torch, size):
    W, H = size
    rgb = planes(W, H)
    alpha = np.random.default_rng(W).integers(0, 256, (H, W), dtype=np.uint8)
    for fmt in (J.PIX_RGBA32, J.PIX_BGRA32):
        for variant in (0, 1):
            ctx.set_variant(variant)
            try:
                got = encode_packed(J, ctx, torch, [rgb], W, H, fmt, W * 4, False, alpha=alpha)
            finally:
                ctx.set_variant(1)
            assert np.array_equal(got, ref_coeffs(W, H)), (size, fmt, variant)


# ---- 2. decode parity ---------------------------------------------------------------------------------------------------------------
def decode_packed(J, ctx, torch, W, H, fmt, kind, gray):
    """dequant_idct_packed_dev into a buffer that ends exactly behind the last row's pixels + 64 canary bytes; returns (pixels (H, W, C),
    the buffer, row stride); the caller checks them"""
    nb, _ = layout(fmt)
    rs = strides_for(kind, W, nb)
    need = (H - 1) * rs + W * nb
    flat = torch.full((need + 64,), FILL, dtype=torch.uint8, device="cuda:0")
    co = torch.from_numpy(np.array(ref_coeffs(W, H))).to("cuda:0")
    ctx.dequant_idct_packed_dev(co, device_view(torch, flat, 1, W, H, nb, rs, 0), format=fmt, gray=gray)
    torch.cuda.synchronize()
    buf = flat.cpu().numpy()
    img = np.lib.stride_tricks.as_strided(buf, (H, W, nb), (rs, nb, 1)).copy()
    untouched = np.ones(buf.size, bool)
    for y in range(H):
        untouched[y * rs: y * rs + W * nb] = False
    assert (buf[untouched] == FILL).all(), ("padding or canary overwritten", W, H, fmt, kind, gray)
    return img


@pytest.mark.parametrize("size", UNALIGNED + [(128, 16), (256, 32), (192, 16), (1920, 24)])
def test_decode_equals_oracle(J, ctx, torch, size):
    """(128,16), (256,32): even quads per row, where the planar kernel swaps whole lines between its two waves; (192,16): odd"""
    W, H = size
    for gray in (False, True):
        want = ref_decoded(W, H, gray)
        for fmt in formats(J):
            for kind in ("tight", "pad16", "pad5"):
                got = decode_packed(J, ctx, torch, W, H, fmt, kind, gray)
                assert np.array_equal(got, interleave(want, W, H, fmt, alpha=0xFF)), (size, gray, fmt, kind)


@pytest.mark.parametrize("size", [(65, 47), (256, 32)])
def test_decode_tolerance_and_force_exact(J, ctx, torch, size):
    W, H = size
    for fmt in (J.PIX_RGB24, J.PIX_BGRA32):
        for gray in (False, True):
            exact = decode_packed(J, ctx, torch, W, H, fmt, "tight", gray)
            ctx.set_decode_tolerance(1)
            try:
                tol = decode_packed(J, ctx, torch, W, H, fmt, "tight", gray)
            finally:
                ctx.set_decode_tolerance(0)
            assert int(np.abs(tol.astype(np.int16) - exact.astype(np.int16)).max()) <= 1, (size, fmt, gray)
            ctx.set_force_exact(1)
            try:
                forced = decode_packed(J, ctx, torch, W, H, fmt, "pad16", gray)
            finally:
                ctx.set_force_exact(0)
                ctx.fallback_count()
            assert np.array_equal(forced, exact), (size, fmt, gray)


# ---- 3. end to end --------------------------------------------------------------------------------------------------------------------
def test_encode_jpeg_packed_equals_encode_jpeg(J, ctx):
    W, H = 100, 60
    rgb = planes(W, H)
    for gray in (False, True):
        want = ctx.encode_jpeg(*rgb, W, H, gray=gray)
        for fmt in formats(J):
            assert ctx.encode_jpeg_packed(interleave(rgb, W, H, fmt, alpha=7), format=fmt, gray=gray) == want, (fmt, gray)


def test_encode_jpeg_packed_cropped_view(J, ctx):
    """an interior 100 x 60 window of a 160 x 90 image, encoded in place: row_stride > W * bytes"""
    big = interleave(planes(160, 90), 160, 90, J.PIX_RGB24)
    view = big[11:71, 23:123]
    assert view.shape == (60, 100, 3) and view.strides == (480, 3, 1) and not view.flags.c_contiguous
    crop = [np.ascontiguousarray(view[:, :, k]).reshape(-1) for k in range(3)]
    assert ctx.encode_jpeg_packed(view, format=J.PIX_RGB24) == ctx.encode_jpeg(*crop, 100, 60)


def test_encode_jpeg_packed_in_several_bands(J, ctx):
    W, H = 256, 96
    rgb = planes(W, H)
    want = ctx.encode_jpeg(*rgb, W, H)
    ctx.set_host_chunk_bytes(16384)
    try:
        for fmt in (J.PIX_RGB24, J.PIX_BGRA32):
            assert ctx.encode_jpeg_packed(interleave(rgb, W, H, fmt), format=fmt) == want, fmt
    finally:
        ctx.set_host_chunk_bytes(4 << 20)


def _files(ctx):
    out = []
    for W, H in ((37, 29), (64, 32)):
        out.append(("own", ctx.encode_jpeg(*planes(W, H), W, H)))
        for name, comps in (("444", L444), ("422", L422), ("400", L400)):
            out.append((name, synth_jpeg(W, H, comps, seed=W)[0]))
    return out


def test_decode_jpeg_packed_equals_decode_jpeg(J, ctx, oracle):
    for min_bytes in (0, 32 << 10):                    # the GPU Huffman decoder / the host decoder for these small scans
        ctx.set_huffdec_min_bytes(min_bytes)
        for name, data in _files(ctx):
            for gray in (False, True):
                info, r, g, b = ctx.decode_jpeg(data, gray=gray)
                W, H = info.width, info.height
                if name == "own":
                    _, orr, og, ob = oracle.decode_jpeg(data, gray)
                    assert all(np.array_equal(a, e) for a, e in zip((r, g, b), (orr, og, ob)))
                for fmt in formats(J):
                    info2, img = ctx.decode_jpeg_packed(data, format=fmt, gray=gray)
                    assert (info2.width, info2.height, info2.ncomp) == (W, H, info.ncomp)
                    assert np.array_equal(img, interleave((r, g, b), W, H, fmt, alpha=0xFF)), (name, W, H, gray, fmt, min_bytes)
    ctx.set_huffdec_min_bytes(32 << 10)


def test_decode_jpeg_packed_row_stride_and_capacity(J, ctx):
    lib = J.load_library()
    for name, data in _files(ctx)[:2]:                 # own layout (fused kernel) and 4:4:4 (generic pair) at 37 x 29
        info, r, g, b = ctx.decode_jpeg(data)
        W, H = info.width, info.height
        arr = np.frombuffer(data, np.uint8)
        for fmt in (J.PIX_BGR24, J.PIX_RGBA32):
            nb, _ = layout(fmt)
            rs = W * nb + 5
            need = (H - 1) * rs + W * nb
            buf = np.full(need + 64, FILL, np.uint8)
            fi = J.FrameInfo()
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            assert lib.jpezy_decode_jpeg_packed(ctx._h, p(arr), arr.size, 0, C.byref(fi), fmt, rs, p(buf), need - 1) == E_NOSPACE
            assert (buf == FILL).all()
            assert lib.jpezy_decode_jpeg_packed(ctx._h, p(arr), arr.size, 0, C.byref(fi), fmt, rs, p(buf), need) == 0
            img = np.lib.stride_tricks.as_strided(buf, (H, W, nb), (rs, nb, 1))
            assert np.array_equal(img, interleave((r, g, b), W, H, fmt, alpha=0xFF)), (name, fmt)
            untouched = np.ones(buf.size, bool)
            for y in range(H):
                untouched[y * rs: y * rs + W * nb] = False
            assert (buf[untouched] == FILL).all(), (name, fmt)


# ---- 4. argument checks -------------------------------------------------------------------------------------------------------------
def test_argument_checks(J, ctx, torch):
    lib = J.load_library()
    W, H = 16, 16
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    co = torch.zeros(J.coeff_count(W, H), dtype=torch.int16, device="cuda:0")
    qt, tq = J.api.annex_k_tables().qt, (C.c_uint8 * 3)(0, 1, 1)
    enc = lambda fmt, rs, h=H: lib.jpezy_fdct_quant_packed_dev(ctx._h, d.data_ptr(), fmt, rs, 0, W, h, 0, 1, co.data_ptr(), None)
    dec = lambda fmt, rs, h=H: lib.jpezy_dequant_idct_packed_dev(ctx._h, co.data_ptr(), C.byref(qt), C.byref(tq), fmt, rs, 0, W, h, 0, 1,
                                                                d.data_ptr(), None)
    for call in (enc, dec):
        assert call(J.PIX_RGB24, W * 3 - 1) == E_BADARG          # rows would overlap
        assert call(J.PIX_RGBA32, W * 4 - 1) == E_BADARG
        assert call(4, 0) == E_BADARG and call(-1, 0) == E_BADARG  # no such format
        # row_stride * H = 2^32: refused before anything is touched (the buffer behind d is 4 KiB)
        assert call(J.PIX_RGB24, 1 << 20, 4096) == E_BADARG
        assert b"32 bits" in lib.jpezy_hip_last_error()
        assert call(J.PIX_RGB24, W * 3) == 0
    torch.cuda.synchronize()
    host = np.zeros(4096, np.uint8)
    out = np.zeros(lib.jpezy_jpeg_bound(W, H), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.jpezy_encode_jpeg_packed(ctx._h, p(host), J.PIX_RGB24, W * 3 - 1, W, H, 0, b"", p(out), out.size) == E_BADARG
    assert lib.jpezy_encode_jpeg_packed(ctx._h, p(host), 7, 0, W, H, 0, b"", p(out), out.size) == E_BADARG
    assert lib.jpezy_encode_jpeg_packed(ctx._h, p(host), J.PIX_RGB24, 1 << 20, W, 4096, 0, b"", p(out), out.size) == E_BADARG
    chw = torch.zeros((3, H, W), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(J.JpezyError):
        ctx.fdct_quant_packed_dev(chw.permute(1, 2, 0), co)     # (H, W, C) in shape, planes in memory
    with pytest.raises(J.JpezyError):
        ctx.fdct_quant_packed_dev(chw, co)


# ---- 5. isolation --------------------------------------------------------------------------------------------------------------------
def test_planar_calls_after_packed_ones(J, ctx, torch, oracle):
    W, H = 208, 40
    rgb = planes(W, H)
    encode_packed(J, ctx, torch, [rgb], W, H, J.PIX_BGRA32, strides_for("pad16", W, 4), False)
    decode_packed(J, ctx, torch, W, H, J.PIX_BGR24, "pad5", False)
    assert np.array_equal(ctx.fdct_quant(*rgb, W, H).reshape(-1), ref_coeffs(W, H))
    got = ctx.dequant_idct(np.array(ref_coeffs(W, H)), W, H)
    for a, e in zip(got, ref_decoded(W, H)):
        assert np.array_equal(a, e)
    d = [torch.from_numpy(np.array(p)).to("cuda:0") for p in rgb]
    co = torch.empty(J.coeff_count(W, H), dtype=torch.int16, device="cuda:0")
    ctx.fdct_quant_dev(d[0], d[1], d[2], W, H, co)
    out = [torch.empty(W * H, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    ctx.dequant_idct_dev(co, W, H, out[0], out[1], out[2])
    torch.cuda.synchronize()
    assert np.array_equal(co.cpu().numpy(), ref_coeffs(W, H))
    for a, e in zip(out, ref_decoded(W, H)):
        assert np.array_equal(a.cpu().numpy(), e)
