"""Reduced-size decode (scale 2, 4, 8) on the GPU: every byte equal to the numpy restatement of the definition (tests/scaled_model.py,
anchored to the oracle at full size by tests/test_scaled_model.py).  Varied: what selects another path or another edge -- N, gray, the
layout (block placement, replication, unwritten ends), ragged Ws / Hs, rows wider than a workgroup, output MCUs narrower than a thread's
four pixels, the level shift, sums outside int32, batches, strides, the packed store stage, the Huffman head that ran."""
import ctypes as C
import functools

import numpy as np
import pytest

import scaled_model as M
from jpeg_synth import ZZ, synth_jpeg, wide_tables
from test_host_codec import ODD_LAYOUTS

pytestmark = pytest.mark.gpu

FILL = 0xA5
E_BADARG, E_NOSPACE = -1, -6
SCALES = (2, 4, 8)
L420 = [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]                # jpezy's own layout
LAYOUTS = {"own": L420, "444": [(1, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)], "422": [(2, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)],
           "one_comp": [(1, 1, 0, 0)], **ODD_LAYOUTS}


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    c.set_huffdec_min_bytes(0)                                   # the GPU Huffman decoder for whatever it takes, small scans too
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---- files and references: made once, never modified ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jpeg(layout, W, H, precision=8, amp=30, restart=0):
    return synth_jpeg(W, H, LAYOUTS[layout], seed=W + H, precision=precision, amp=amp, restart=restart)[0]


def parsed(data):
    """(FrameInfo, coefficients) by the host decoder: what every Huffman head here must deliver"""
    import jpezy_amd
    return jpezy_amd.read_jpeg(data)


@functools.lru_cache(maxsize=None)
def want(data, scale, gray):
    info, co = parsed(data)
    out = M.decode_planes(co, info, scale, gray)
    for a in out:
        a.setflags(write=False)
    return out


def dev_planes(torch, ctx, data, scale, gray):
    """read_jpeg_gpu -> dequant_idct_scaled_dev into planes pre-filled with FILL and one byte longer than needed"""
    info, d_co = ctx.read_jpeg_gpu(data)
    ws, hs = M.scaled_size(info.width, info.height, scale)
    out = [torch.full((ws * hs + 1,), FILL, dtype=torch.uint8, device=d_co.device) for _ in range(3)]
    ctx.dequant_idct_scaled_dev(d_co, info, scale, out[0], out[1], out[2], gray=gray)
    torch.cuda.synchronize()
    out = [o.cpu().numpy() for o in out]
    assert all(o[-1] == FILL for o in out)
    return [o[:-1] for o in out]


def check_both(torch, ctx, data, tag):
    info = None
    for scale in SCALES:
        for gray in (False, True):
            e = want(data, scale, gray)
            info, r, g, b = ctx.decode_jpeg_scaled(data, scale, gray=gray)
            for a, x in zip((r, g, b), e):
                assert np.array_equal(a, x), ("decode_jpeg_scaled", tag, scale, gray)
            for a, x in zip(dev_planes(torch, ctx, data, scale, gray), e):
                assert np.array_equal(a, x), ("dequant_idct_scaled_dev", tag, scale, gray)
    return info


# ---- parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(37, 21), (101, 70)])           # ragged Ws / Hs at every N, partial MCUs on both edges
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_parity_across_layouts(J, ctx, torch, layout, size):
    W, H = size
    info = check_both(torch, ctx, jpeg(layout, W, H), (layout, size))
    assert (info.width, info.height) == (W, H)


# 976x33, 2048x7: rows wider than one workgroup, the last MCU row mostly dropped; 4096x16 at N = 1: 512 pixels from 256 MCUs
@pytest.mark.parametrize("size", [(1, 1), (16, 16), (17, 9), (976, 33), (2048, 7), (4096, 16)])
def test_own_layout_size_edges(J, ctx, torch, size):
    check_both(torch, ctx, jpeg("own", *size), size)


def test_scale_1_is_the_existing_decode(J, ctx, torch):
    for layout in ("own", "422"):
        data = jpeg(layout, 101, 70)
        for gray in (False, True):
            info, r, g, b = ctx.decode_jpeg(data, gray=gray)
            info1, r1, g1, b1 = ctx.decode_jpeg_scaled(data, 1, gray=gray)
            assert (info1.width, info1.height) == (info.width, info.height) == (101, 70)
            assert all(np.array_equal(a, e) for a, e in zip((r1, g1, b1), (r, g, b)))
            _, img = ctx.decode_jpeg_scaled_packed(data, 1, J.PIX_RGB24, gray=gray)
            assert np.array_equal(img, np.stack([r, g, b], axis=-1).reshape(70, 101, 3))
            for a, e in zip(dev_planes(torch, ctx, data, 1, gray), (r, g, b)):
                assert np.array_equal(a, e)


@pytest.mark.parametrize("layout", ["own", "one_comp"])
def test_precision_12(J, ctx, torch, layout):
    """SOF0 precision != 8: the level shift is 2048 (ref :654)"""
    data = jpeg(layout, 37, 21, precision=12, amp=200)
    assert parsed(data)[0].precision == 12
    check_both(torch, ctx, data, layout)


def test_range_16bit_dqt_extremes(J, ctx, torch):
    """Q = 65535 everywhere, +-32767 on the N x N corner: at N = 4 the sums leave int32 (|sum| / 4 up to 4e9) and the sample is
    INT_MIN, 0 after revise_value, where a saturating conversion would give 255"""
    pats = []
    for n in (4, 2, 1):
        for sign in (1, -1):
            nat = np.zeros((8, 8), np.int64)
            nat[:n, :n] = sign * 32767
            pats.append(nat.reshape(-1))
            sx = np.sign(np.cos((2 * 1 + 1) * np.arange(8) * np.pi / 8) + 1e-30)      # the signs that add up at sample x = y = 1 (N = 4)
            alt = np.zeros((8, 8), np.int64)
            alt[:n, :n] = sign * 32767 * np.outer(sx, sx)[:n, :n]
            pats.append(alt.reshape(-1))
    smp4 = M.idct_blocks(np.array(pats) * 65535, 4, 128)
    assert (smp4 == M.INT_MIN).any() and (smp4 > 255).any() and (smp4 < 0).any()
    nm = len(pats)
    co = np.zeros((nm, 6, 64), np.int64)
    for m in range(nm):
        for b in range(6):
            co[m, b] = pats[(m + b) % nm][ZZ]
    data, _, _ = synth_jpeg(16 * nm, 16, L420, qt=np.full((2, 64), 65535), qt_precision=(1, 1), coeffs=co, tables=wide_tables())
    info, hco = parsed(data)
    assert np.array_equal(hco.reshape(-1), co.reshape(-1)) and info.qt[0][0] == 65535
    check_both(torch, ctx, data, "range")


# ---- device entry points: batches, strides, packed pixels -----------------------------------------------------------------------
def _three_frames(data):
    """the file's coefficients, a sign-flipped and a halved copy: (FrameInfo, int16 [3, n])"""
    info, co = parsed(data)
    co = co.reshape(-1).astype(np.int32)
    return info, np.stack([co, -co, co // 2]).astype(np.int16)


@pytest.mark.parametrize("layout", ["own", "h3_partial"])
def test_device_batch_with_padded_stride(J, ctx, torch, layout):
    info, frames = _three_frames(jpeg(layout, 101, 70))
    dev = torch.device("cuda", 0)
    d_co = torch.from_numpy(frames).to(dev)
    for scale in SCALES:
        ws, hs = M.scaled_size(101, 70, scale)
        stride = ws * hs + 52
        for gray in (False, True):
            out = [torch.full((3 * stride,), FILL, dtype=torch.uint8, device=dev) for _ in range(3)]
            ctx.dequant_idct_scaled_dev(d_co, info, scale, out[0], out[1], out[2], gray=gray, n_frames=3, plane_stride=stride)
            torch.cuda.synchronize()
            out = [o.cpu().numpy().reshape(3, stride) for o in out]
            for f in range(3):
                for a, e in zip(out, M.decode_planes(frames[f], info, scale, gray)):
                    assert np.array_equal(a[f, : ws * hs], e), (layout, scale, gray, f)
            assert all((a[:, ws * hs:] == FILL).all() for a in out), (layout, scale, gray)


def test_device_batch_above_the_grid_limit(J, ctx, torch):
    """65537 frames of 8 x 8, one component: the frame index is a grid dimension, the launcher splits at 65535"""
    info, frames = _three_frames(synth_jpeg(8, 8, LAYOUTS["one_comp"], seed=5)[0])
    nf, scale = 65537, 4
    dev = torch.device("cuda", 0)
    d_co = torch.from_numpy(frames).to(dev)[torch.arange(nf, device=dev) % 3].contiguous()
    out = [torch.full((nf * 4 + 1,), FILL, dtype=torch.uint8, device=dev) for _ in range(3)]
    ctx.dequant_idct_scaled_dev(d_co, info, scale, out[0], out[1], out[2], n_frames=nf, plane_stride=4)
    torch.cuda.synchronize()
    ref = [np.stack([M.decode_planes(frames[f], info, scale)[k] for f in range(3)]) for k in range(3)]
    for k in range(3):
        a = out[k].cpu().numpy()
        assert a[-1] == FILL
        assert np.array_equal(a[:-1].reshape(nf, 4), ref[k][np.arange(nf) % 3])


def _interleave(J, fmt, planes, hs, ws):
    nb = 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4
    order = (0, 1, 2) if fmt in (J.PIX_RGB24, J.PIX_RGBA32) else (2, 1, 0)
    img = np.full((hs, ws, nb), 0xFF, np.uint8)
    for k in range(3):
        img[..., k] = planes[order[k]].reshape(hs, ws)
    return img


@pytest.mark.parametrize("fmt", [0, 1, 2, 3])
def test_packed_formats_and_row_padding(J, ctx, torch, fmt):
    assert [J.PIX_RGB24, J.PIX_BGR24, J.PIX_RGBA32, J.PIX_BGRA32] == [0, 1, 2, 3]
    lib = J.load_library()
    dev = torch.device("cuda", 0)
    for layout, (W, H) in (("own", (101, 70)), ("411", (37, 21))):
        data = jpeg(layout, W, H)
        arr = np.frombuffer(data, dtype=np.uint8)
        info, d_co = ctx.read_jpeg_gpu(data)
        for scale in SCALES:
            ws, hs = M.scaled_size(W, H, scale)
            for gray in (False, True):
                e = _interleave(J, fmt, want(data, scale, gray), hs, ws)
                nb = e.shape[2]
                rs = ws * nb + 7
                # device: a view with padded rows into a buffer with a canary behind the last row
                buf = torch.full((hs * rs + 16,), FILL, dtype=torch.uint8, device=dev)
                ctx.dequant_idct_scaled_dev(d_co, info, scale, gray=gray, d_img=buf.as_strided((hs, ws, nb), (rs, nb, 1)), format=fmt)
                torch.cuda.synchronize()
                a = buf.cpu().numpy()
                rows = a[: hs * rs].reshape(hs, rs)
                assert np.array_equal(rows[:, : ws * nb].reshape(hs, ws, nb), e), ("dev", layout, scale, gray)
                assert (rows[:, ws * nb:] == FILL).all() and (a[hs * rs:] == FILL).all()
                # host: tight through the binding, padded rows through the C entry
                _, img = ctx.decode_jpeg_scaled_packed(data, scale, fmt, gray=gray)
                assert np.array_equal(img, e), ("host", layout, scale, gray)
                hb = np.full(hs * rs + 16, FILL, np.uint8)
                fi = J.FrameInfo()
                need = (hs - 1) * rs + ws * nb
                p = lambda x: x.ctypes.data_as(C.c_void_p)
                assert lib.jpezy_decode_jpeg_scaled_packed(ctx._h, p(arr), arr.size, int(gray), scale, C.byref(fi), fmt, rs, p(hb), need - 1) == E_NOSPACE
                assert lib.jpezy_decode_jpeg_scaled_packed(ctx._h, p(arr), arr.size, int(gray), scale, C.byref(fi), fmt, rs, p(hb), need) == 0
                rows = hb[: hs * rs].reshape(hs, rs)
                assert np.array_equal(rows[:, : ws * nb].reshape(hs, ws, nb), e)
                assert (rows[:-1, ws * nb:] == FILL).all() and (hb[need:] == FILL).all()


def test_packed_batch(J, ctx, torch):
    """two frames as a (N, Hs, Ws, C) tensor with padded rows and a padded frame stride"""
    info, frames = _three_frames(jpeg("own", 101, 70))
    dev = torch.device("cuda", 0)
    d_co = torch.from_numpy(frames[:2].copy()).to(dev)
    scale, fmt = 4, J.PIX_BGRA32
    ws, hs = M.scaled_size(101, 70, scale)
    rs, fs = ws * 4 + 4, hs * (ws * 4 + 4) + 24
    buf = torch.full((2 * fs,), FILL, dtype=torch.uint8, device=dev)
    ctx.dequant_idct_scaled_dev(d_co, info, scale, d_img=buf.as_strided((2, hs, ws, 4), (fs, rs, 4, 1)), format=fmt)
    torch.cuda.synchronize()
    a = buf.cpu().numpy().reshape(2, fs)
    for f in range(2):
        rows = a[f, : hs * rs].reshape(hs, rs)
        assert np.array_equal(rows[:, : ws * 4].reshape(hs, ws, 4), _interleave(J, fmt, M.decode_planes(frames[f], info, scale), hs, ws))
        assert (rows[:, ws * 4:] == FILL).all() and (a[f, hs * rs:] == FILL).all()


# ---- the Huffman head ------------------------------------------------------------------------------------------------------------
def test_host_fallback_and_restart_intervals(J, ctx, torch):
    """a regular restart-interval file is decoded on the device, one with a stray marker inside an interval by the host decoder
    (which reads on): both reduced pictures are the model's on the coefficients the host decoder reads"""
    regular = jpeg("own", 101, 70, restart=2)
    pos = [i for i in range(len(regular) - 1) if regular[i] == 0xFF and 0xD0 <= regular[i + 1] <= 0xD7]
    assert len(pos) >= 4 and parsed(regular)[0].restart_interval == 2
    irregular = regular[: pos[2] - 5] + b"\xff\xc4" + regular[pos[2] - 5:]
    assert not np.array_equal(parsed(irregular)[1], parsed(regular)[1])
    for data, on_gpu in ((regular, True), (irregular, False)):
        check_both(torch, ctx, data, on_gpu)
        ctx.decode_jpeg_scaled(data, 4)
        assert (ctx.last_huffdec_passes() > 0) == on_gpu


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors_and_header_only(J, ctx):
    lib = J.load_library()
    data = jpeg("own", 101, 70)
    arr = np.frombuffer(data, dtype=np.uint8)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    for scale in SCALES:
        ws, hs = M.scaled_size(101, 70, scale)
        fi = J.FrameInfo()
        assert lib.jpezy_decode_jpeg_scaled(ctx._h, p(arr), arr.size, 0, scale, C.byref(fi), None, None, None, 0) == 0
        assert (fi.width, fi.height) == (101, 70)
        planes = [np.full(ws * hs, FILL, np.uint8) for _ in range(3)]
        assert lib.jpezy_decode_jpeg_scaled(ctx._h, p(arr), arr.size, 0, scale, C.byref(fi), *map(p, planes), ws * hs - 1) == E_NOSPACE
        assert all((a == FILL).all() for a in planes)
        assert lib.jpezy_decode_jpeg_scaled(ctx._h, p(arr), arr.size, 0, scale, C.byref(fi), *map(p, planes), ws * hs) == 0
        assert (fi.width, fi.height) == (101, 70)
        assert all(np.array_equal(a, e) for a, e in zip(planes, want(data, scale, False)))
    fi = J.FrameInfo()
    planes = [np.zeros(101 * 70, np.uint8) for _ in range(3)]
    for bad in (3, 0, 16, -2):
        assert lib.jpezy_decode_jpeg_scaled(ctx._h, p(arr), arr.size, 0, bad, C.byref(fi), *map(p, planes), 101 * 70) == E_BADARG
        assert lib.jpezy_decode_jpeg_scaled(ctx._h, p(arr), arr.size, 0, bad, C.byref(fi), None, None, None, 0) == E_BADARG
        assert lib.jpezy_decode_jpeg_scaled_packed(ctx._h, p(arr), arr.size, 0, bad, C.byref(fi), 0, 0, p(planes[0]), 101 * 70) == E_BADARG
        with pytest.raises(J.JpezyError):
            ctx.decode_jpeg_scaled(data, bad)
    assert lib.jpezy_decode_jpeg_scaled_packed(ctx._h, p(arr), arr.size, 0, 2, C.byref(fi), 7, 0, p(planes[0]), 101 * 70) == E_BADARG    # no such format


def test_decoder_class_mirror(J, ctx, tmp_path):
    data = jpeg("own", 101, 70)
    path = tmp_path / "a.jpg"
    path.write_bytes(data)
    dec = J.Decoder(str(path), ctx=ctx)
    full = dec.decode()
    assert all(np.array_equal(a, e) for a, e in zip(full, ctx.decode_jpeg(data)[1:]))
    for gray in (False, True):
        got = dec.decode(gray=gray, scale=4)
        assert (dec.pr.width, dec.pr.height) == (101, 70)
        assert all(np.array_equal(a, e) for a, e in zip(got, want(data, 4, gray)))
