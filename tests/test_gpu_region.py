"""Region decode on the GPU: every byte equal to the slice of the numpy restatement of the (scaled) decode (tests/region_model.py over
tests/scaled_model.py, anchored to the oracle at full size by tests/test_scaled_model.py).  Varied: what a windowed kernel can get wrong --
the layout (block placement, replication, unwritten ends), N, gray, where the window starts and ends against the MCU grid and against the
ragged edges, the store form (word / vector against bytes, by address and by how many of a group's four pixels an MCU owns), strides and
padding, batches, the MCUs that are read, the level shift, sums outside int32, the Huffman head that ran.  Files are read once per test
(read_jpeg_gpu) and many windows go through the device entry into buffers pre-filled with a marker byte and one byte longer than needed.
There is no tolerance: every comparison is np.array_equal."""
import ctypes as C
import functools

import numpy as np
import pytest

import region_model as R
import scaled_model as M
from jpeg_synth import ZZ, synth_jpeg, wide_tables
from test_host_codec import ODD_LAYOUTS

pytestmark = pytest.mark.gpu

FILL = 0xA5
E_BADARG, E_NOSPACE = -1, -6
SCALES = (1, 2, 4, 8)
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


@functools.lru_cache(maxsize=None)
def parsed(data):
    """(FrameInfo, coefficients) by the host decoder: what every Huffman head here must deliver"""
    import jpezy_amd
    info, co = jpezy_amd.read_jpeg(data)
    co.setflags(write=False)
    return info, co


@functools.lru_cache(maxsize=None)
def want_full(data, scale, gray):
    """the model's whole picture at 1/scale as three read-only (Hs, Ws) arrays; windows are slices of it"""
    info, co = parsed(data)
    ws, hs = M.scaled_size(info.width, info.height, scale)
    out = tuple(p.reshape(hs, ws) for p in M.decode_planes(co, info, scale, gray))
    for a in out:
        a.setflags(write=False)
    return out


def want(data, region, scale, gray):
    x, y, w, h = region
    e = tuple(a[y:y + h, x:x + w] for a in want_full(data, scale, gray))
    assert e[0].shape == (h, w), ("region outside the picture", region, scale)
    if w * h >= 16:      # a shifted window must not be able to pass by accident: no constant planes
        assert all(np.ptp(a) > 0 for a in e), ("degenerate reference", region, scale, gray)
    return e


def windows(info, scale):
    """{name: (x, y, w, h)} in the picture at 1/scale: the places where a windowed kernel can go wrong"""
    n = 8 // scale
    ws, hs = M.scaled_size(info.width, info.height, scale)
    mw, mh = info.hmax * n, info.vmax * n
    cand = {
        "whole": (0, 0, ws, hs),                                  # the hand-off
        "first": (0, 0, 1, 1),
        "last": (ws - 1, hs - 1, 1, 1),
        "inside_one_mcu": (mw + 1, mh + 1, max(mw - 2, 1), max(mh - 2, 1)) if mw >= 3 and mh >= 3 else (mw, mh, 1, 1),
        "four_mcu_corner": (mw - 1, mh - 1, 2, 2),
        "row": (0, hs // 2, ws, 1),
        "column": (ws // 2, 0, 1, hs),
        "ragged_edges": (ws // 3, hs // 3, ws - ws // 3, hs - hs // 3),
        "from_inside_an_mcu": (mw // 2 + 1, mh // 2 + 1, ws - mw // 2 - 1, hs - mh // 2 - 1),
    }
    return {k: (x, y, w, h) for k, (x, y, w, h) in cand.items() if w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= ws and y + h <= hs}


def run_planar(torch, ctx, d_co, info, region, scale, gray, n_frames=1, stride=None):
    """-> three uint8 arrays [n_frames, stride] after the canary behind the last frame was checked"""
    w, h = region[2], region[3]
    stride = w * h if stride is None else stride
    out = [torch.full((n_frames * stride + 1,), FILL, dtype=torch.uint8, device=d_co.device) for _ in range(3)]
    ctx.dequant_idct_region_dev(d_co, info, region, scale, out[0], out[1], out[2], gray=gray, n_frames=n_frames, plane_stride=stride)
    torch.cuda.synchronize()
    out = [o.cpu().numpy() for o in out]
    assert all(o[-1] == FILL for o in out), ("byte behind the output written", region, scale, gray)
    return [o[:-1].reshape(n_frames, stride) for o in out]


def check_windows(torch, ctx, data, tag, scales=SCALES, grays=(False, True), only=None):
    info, d_co = ctx.read_jpeg_gpu(data)
    for scale in scales:
        for name, region in windows(info, scale).items():
            if only is not None and name not in only:
                continue
            for gray in grays:
                got = run_planar(torch, ctx, d_co, info, region, scale, gray)
                for a, e in zip(got, want(data, region, scale, gray)):
                    assert np.array_equal(a[0].reshape(e.shape), e), (tag, name, region, scale, gray)
    return info


def _interleave(J, fmt, planes):
    nb = 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4
    order = (0, 1, 2) if fmt in (J.PIX_RGB24, J.PIX_RGBA32) else (2, 1, 0)
    img = np.full(planes[0].shape + (nb,), 0xFF, np.uint8)
    for k in range(3):
        img[..., k] = planes[order[k]]
    return img


# ---- parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(37, 21), (101, 70)])           # ragged Ws / Hs at every N, partial MCUs on both edges
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_windows_across_layouts(J, ctx, torch, layout, size):
    W, H = size
    info = check_windows(torch, ctx, jpeg(layout, W, H), (layout, size))
    assert (info.width, info.height) == (W, H)


@pytest.mark.parametrize("size", [(2048, 7), (976, 33)])
def test_wide_rows(J, ctx, torch, size):
    """a window from x = 5 that is wider than one workgroup's row span: 1500 pixels, or as many as the picture at that scale has"""
    data = jpeg("own", *size)
    info, d_co = ctx.read_jpeg_gpu(data)
    for scale in (1, 8):
        ws, hs = M.scaled_size(*size, scale)
        for region in ((5, 0, min(1500, ws - 5), hs), (5, hs - 1, min(1500, ws - 5), 1)):
            for gray in (False, True):
                got = run_planar(torch, ctx, d_co, info, region, scale, gray)
                for a, e in zip(got, want(data, region, scale, gray)):
                    assert np.array_equal(a[0].reshape(e.shape), e), (size, region, scale, gray)


# ---- the store forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [None, 0, 1, 2, 3])               # planes, then the four packed formats
def test_store_paths(J, ctx, torch, fmt):
    """x in {1, 2, 3, 5, 13, 14} and w in 1..9: groups of four output pixels that start in one MCU and end in the next, rows whose first byte
    is at every alignment, the three-byte vector form; packed rows have padding, which keeps the marker byte"""
    data = jpeg("own", 101, 70)
    info, d_co = ctx.read_jpeg_gpu(data)
    dev = d_co.device
    for scale in (1, 4):
        ws, hs = M.scaled_size(101, 70, scale)
        y, h = hs // 2 - 1, 3
        for x in (1, 2, 3, 5, 13, 14):                            # 13, 14: across the MCU boundary at full size too
            for w in range(1, 10):
                region = (x, y, w, h)
                e = want(data, region, scale, False)
                if fmt is None:
                    got = run_planar(torch, ctx, d_co, info, region, scale, False)
                    for a, ee in zip(got, e):
                        assert np.array_equal(a[0].reshape(h, w), ee), (region, scale)
                    continue
                img = _interleave(J, fmt, e)
                nb = img.shape[2]
                for rs in (w * nb + 5, (w * nb + 3) // 4 * 4 + 4):                     # rows at every alignment; rows that all start on a word
                    buf = torch.full((h * rs + 16,), FILL, dtype=torch.uint8, device=dev)
                    ctx.dequant_idct_region_dev(d_co, info, region, scale, d_img=buf.as_strided((h, w, nb), (rs, nb, 1)), format=fmt)
                    torch.cuda.synchronize()
                    a = buf.cpu().numpy()
                    rows = a[: h * rs].reshape(h, rs)
                    assert np.array_equal(rows[:, : w * nb].reshape(h, w, nb), img), (region, scale, fmt, rs)
                    assert (rows[:, w * nb:] == FILL).all() and (a[h * rs:] == FILL).all(), (region, scale, fmt, rs)


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def _three_frames(data):
    """the file's coefficients, a sign-flipped and a halved copy: (FrameInfo, int16 [3, n])"""
    info, co = parsed(data)
    co = co.reshape(-1).astype(np.int32)
    return info, np.stack([co, -co, co // 2]).astype(np.int16)


@pytest.mark.parametrize("layout", ["own", "h3_partial"])
def test_device_batch_with_padded_strides(J, ctx, torch, layout):
    info, frames = _three_frames(jpeg(layout, 101, 70))
    dev = torch.device("cuda", 0)
    d_co = torch.from_numpy(frames).to(dev)
    for scale in SCALES:
        ws, hs = M.scaled_size(101, 70, scale)
        for region in ((ws // 4, hs // 4, ws // 2, hs // 2), (0, 0, ws, hs)):       # a window; the whole picture with a stride that is no multiple of 4
            x, y, w, h = region
            refs = [R.decode_region(frames[f], info, region, scale, False) for f in range(3)]
            stride = w * h + 53
            got = run_planar(torch, ctx, d_co, info, region, scale, False, n_frames=3, stride=stride)
            for f in range(3):
                for a, e in zip(got, refs[f]):
                    assert np.array_equal(a[f, : w * h].reshape(h, w), e), (layout, scale, region, f)
            assert all((a[:, w * h:] == FILL).all() for a in got), (layout, scale, region)
            fmt = J.PIX_BGRA32
            rs, fs = w * 4 + 4, h * (w * 4 + 4) + 25
            buf = torch.full((3 * fs,), FILL, dtype=torch.uint8, device=dev)
            ctx.dequant_idct_region_dev(d_co, info, region, scale, d_img=buf.as_strided((3, h, w, 4), (fs, rs, 4, 1)), format=fmt)
            torch.cuda.synchronize()
            a = buf.cpu().numpy().reshape(3, fs)
            for f in range(3):
                rows = a[f, : h * rs].reshape(h, rs)
                assert np.array_equal(rows[:, : w * 4].reshape(h, w, 4), _interleave(J, fmt, refs[f])), (layout, scale, region, f)
                assert (rows[:, w * 4:] == FILL).all() and (a[f, h * rs:] == FILL).all(), (layout, scale, region, f)


def test_device_batch_above_the_grid_limit(J, ctx, torch):
    """65537 frames of 8 x 8, one component: the frame index is a grid dimension, the launcher splits at 65535"""
    info, frames = _three_frames(synth_jpeg(8, 8, LAYOUTS["one_comp"], seed=5)[0])
    nf, scale, region = 65537, 2, (1, 1, 3, 2)
    dev = torch.device("cuda", 0)
    d_co = torch.from_numpy(frames).to(dev)[torch.arange(nf, device=dev) % 3].contiguous()
    got = run_planar(torch, ctx, d_co, info, region, scale, False, n_frames=nf, stride=7)
    ref = [np.stack([R.decode_region(frames[f], info, region, scale)[k].reshape(-1) for f in range(3)]) for k in range(3)]
    for k in range(3):
        assert np.array_equal(got[k][:, :6], ref[k][np.arange(nf) % 3])
        assert (got[k][:, 6] == FILL).all()


# ---- what is read ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["own", "h4v4"])
def test_only_the_windows_mcus_are_read(J, ctx, torch, layout):
    """the coefficients of every MCU that does not intersect the window overwritten with 0x7FFF: the output does not change"""
    data = jpeg(layout, 101, 70)
    info, co = parsed(data)
    bpm = info.blocks_per_mcu
    dev = torch.device("cuda", 0)
    for scale in (1, 4):
        n = 8 // scale
        mw, mh = info.hmax * n, info.vmax * n
        ws, hs = M.scaled_size(101, 70, scale)
        for region in ((mw + 1, mh - 1, mw, 2), (ws - mw - 1, 0, mw + 1, hs), (mw // 2, mh // 2, 1, 1)):
            x, y, w, h = region
            poisoned = np.array(co).reshape(info.mcu_rows, info.mcu_cols, bpm * 64).copy()
            keep = np.zeros((info.mcu_rows, info.mcu_cols), bool)
            keep[y // mh: (y + h - 1) // mh + 1, x // mw: (x + w - 1) // mw + 1] = True
            assert keep.any() and not keep.all()
            poisoned[~keep] = 0x7FFF
            d_co = torch.from_numpy(poisoned.reshape(-1)).to(dev)
            for gray in (False, True):
                got = run_planar(torch, ctx, d_co, info, region, scale, gray)
                for a, e in zip(got, want(data, region, scale, gray)):
                    assert np.array_equal(a[0].reshape(h, w), e), (layout, scale, region, gray)


# ---- value range -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jpeg12(layout):
    """SOF0 precision 12 with DCs that bring the samples back from the level of 2048 into 0..255 (Q = 16: -960 * 16 / 8 = -1920), so that
    the picture is not one saturated plane and a misplaced window shows"""
    co = synth_jpeg(37, 21, LAYOUTS[layout], seed=58, amp=60)[1].astype(np.int64).reshape(-1, 64)
    co[:, 0] -= 960
    return synth_jpeg(37, 21, LAYOUTS[layout], precision=12, qt=np.full((2, 64), 16), coeffs=co)[0]


@pytest.mark.parametrize("layout", ["own", "one_comp"])
def test_precision_12(J, ctx, torch, layout):
    """SOF0 precision != 8: the level shift is 2048 (ref :654)"""
    data = jpeg12(layout)
    assert parsed(data)[0].precision == 12
    check_windows(torch, ctx, data, ("precision 12", layout), grays=(False,))


def test_range_16bit_dqt_extremes(J, ctx, torch):
    """Q = 65535 everywhere, +-32767 on the N x N corner: sums leave int32 and the sample is INT_MIN, 0 after revise_value, where a
    saturating conversion would give 255 (the file tests/test_gpu_scaled.py builds)"""
    pats = []
    for n in (8, 4, 2, 1):
        for sign in (1, -1):
            nat = np.zeros((8, 8), np.int64)
            nat[:n, :n] = sign * 32767
            pats.append(nat.reshape(-1))
            sx = np.sign(np.cos((2 * 1 + 1) * np.arange(8) * np.pi / 8) + 1e-30)      # the signs that add up at sample x = y = 1 (N = 4)
            alt = np.zeros((8, 8), np.int64)
            alt[:n, :n] = sign * 32767 * np.outer(sx, sx)[:n, :n]
            pats.append(alt.reshape(-1))
    for n in (8, 4):
        smp = M.idct_blocks(np.array(pats) * 65535, n, 128)
        assert (smp == M.INT_MIN).any() and (smp > 255).any() and (smp < 0).any()
    nm = len(pats)
    co = np.zeros((nm, 6, 64), np.int64)
    for m in range(nm):
        for b in range(6):
            co[m, b] = pats[(m + b) % nm][ZZ]
    data, _, _ = synth_jpeg(16 * nm, 16, L420, qt=np.full((2, 64), 65535), qt_precision=(1, 1), coeffs=co, tables=wide_tables())
    info, hco = parsed(data)
    assert np.array_equal(np.asarray(hco).reshape(-1), co.reshape(-1)) and info.qt[0][0] == 65535
    _, d_co = ctx.read_jpeg_gpu(data)
    for scale in SCALES:
        ws, hs = M.scaled_size(16 * nm, 16, scale)
        for region in ((0, 0, ws, hs), (1, 0, ws - 1, hs), (ws // 3, hs // 2, ws // 2, hs - hs // 2)):
            x, y, w, h = region
            for gray in (False, True):
                got = run_planar(torch, ctx, d_co, info, region, scale, gray)
                for a, e in zip(got, (p[y:y + h, x:x + w] for p in want_full(data, scale, gray))):
                    assert np.array_equal(a[0].reshape(h, w), e), (region, scale, gray)


# ---- the host-bytes entries and the Huffman head ------------------------------------------------------------------------------------
def test_heads(J, ctx, torch):
    """a file with restart intervals, a small file handed to the host Huffman decoder (the default threshold) and the same one on the
    GPU decoder: the window is the model's slice on the coefficients the host decoder reads, info carries the file's size"""
    small = jpeg("own", 101, 70)
    assert len(small) < (32 << 10)
    cases = [(jpeg("own", 101, 70, restart=2), 0, True), (small, 32 << 10, False), (small, 0, True)]
    assert parsed(cases[0][0])[0].restart_interval == 2
    try:
        for data, min_bytes, on_gpu in cases:
            ctx.set_huffdec_min_bytes(min_bytes)
            for scale in SCALES:
                ws, hs = M.scaled_size(101, 70, scale)
                for region in ((ws // 3, hs // 4, ws // 2, hs // 2), (0, 0, ws, hs)):
                    x, y, w, h = region
                    for gray in (False, True):
                        e = want(data, region, scale, gray)
                        info, r, g, b = ctx.decode_jpeg_region(data, region, scale=scale, gray=gray)
                        assert (info.width, info.height) == (101, 70)
                        assert (ctx.last_huffdec_passes() > 0) == on_gpu
                        for a, ee in zip((r, g, b), e):
                            assert np.array_equal(a.reshape(h, w), ee), ("planes", min_bytes, region, scale, gray)
                        for fmt in (J.PIX_RGB24, J.PIX_BGRA32):
                            info, img = ctx.decode_jpeg_region_packed(data, region, scale=scale, format=fmt, gray=gray)
                            assert (info.width, info.height) == (101, 70)
                            assert np.array_equal(img, _interleave(J, fmt, e)), ("packed", min_bytes, region, scale, gray, fmt)
    finally:
        ctx.set_huffdec_min_bytes(0)


def test_capacity_header_only_and_errors(J, ctx):
    lib = J.load_library()
    data = jpeg("own", 101, 70)
    arr = np.frombuffer(data, dtype=np.uint8)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    for scale in SCALES:
        ws, hs = M.scaled_size(101, 70, scale)
        for region in ((ws // 3, hs // 4, ws // 2, hs // 2), (0, 0, ws, hs)):
            x, y, w, h = region
            rect = J.Rect(x, y, w, h)
            e = want(data, region, scale, False)
            fi = J.FrameInfo()
            assert lib.jpezy_decode_jpeg_region(ctx._h, p(arr), arr.size, 0, scale, C.byref(rect), C.byref(fi), None, None, None, 0) == 0
            assert (fi.width, fi.height) == (101, 70)
            planes = [np.full(w * h, FILL, np.uint8) for _ in range(3)]
            assert lib.jpezy_decode_jpeg_region(ctx._h, p(arr), arr.size, 0, scale, C.byref(rect), C.byref(fi), *map(p, planes), w * h - 1) == E_NOSPACE
            assert all((a == FILL).all() for a in planes)
            assert lib.jpezy_decode_jpeg_region(ctx._h, p(arr), arr.size, 0, scale, C.byref(rect), C.byref(fi), *map(p, planes), w * h) == 0
            assert all(np.array_equal(a.reshape(h, w), ee) for a, ee in zip(planes, e))
            # packed: padded rows through the C entry, the padding and what lies behind the last row untouched
            fmt, nb = J.PIX_BGR24, 3
            rs = w * nb + 7
            need = (h - 1) * rs + w * nb
            hb = np.full(h * rs + 16, FILL, np.uint8)
            assert lib.jpezy_decode_jpeg_region_packed(ctx._h, p(arr), arr.size, 0, scale, C.byref(rect), C.byref(fi), fmt, rs, None, 0) == 0
            assert lib.jpezy_decode_jpeg_region_packed(ctx._h, p(arr), arr.size, 0, scale, C.byref(rect), C.byref(fi), fmt, rs, p(hb), need - 1) == E_NOSPACE
            assert (hb == FILL).all()
            assert lib.jpezy_decode_jpeg_region_packed(ctx._h, p(arr), arr.size, 0, scale, C.byref(rect), C.byref(fi), fmt, rs, p(hb), need) == 0
            rows = hb[: h * rs].reshape(h, rs)
            assert np.array_equal(rows[:, : w * nb].reshape(h, w, nb), _interleave(J, fmt, e))
            assert (rows[:-1, w * nb:] == FILL).all() and (hb[need:] == FILL).all()
        # a region outside the picture: refused once the header is known, with the output untouched; header only asks for its syntax alone
        out = J.Rect(ws - 1, 0, 2, 1)
        fi = J.FrameInfo()
        planes = [np.full(16, FILL, np.uint8) for _ in range(3)]
        assert lib.jpezy_decode_jpeg_region(ctx._h, p(arr), arr.size, 0, scale, C.byref(out), C.byref(fi), *map(p, planes), 16) == E_BADARG
        msg = lib.jpezy_hip_last_error().decode()
        assert f"2x1+{ws - 1}+0" in msg and f"{ws} x {hs}" in msg
        assert all((a == FILL).all() for a in planes)
        assert lib.jpezy_decode_jpeg_region(ctx._h, p(arr), arr.size, 0, scale, C.byref(out), C.byref(fi), None, None, None, 0) == 0
        with pytest.raises(J.JpezyError, match="outside"):
            ctx.decode_jpeg_region(data, (ws - 1, 0, 2, 1), scale=scale)
        with pytest.raises(J.JpezyError, match="outside"):
            ctx.decode_jpeg_region_packed(data, (0, hs, 1, 1), scale=scale)


def test_settings_have_nothing_to_act_on(J, ctx, torch):
    """force_exact and decode_tolerance change nothing and the fallback counter is not advanced"""
    data = jpeg("own", 101, 70)
    info, d_co = ctx.read_jpeg_gpu(data)
    region = (9, 7, 50, 40)
    try:
        for force, tol in ((1, 0), (0, 1)):
            ctx.set_force_exact(force)
            ctx.set_decode_tolerance(tol)
            ctx.fallback_count()                                  # reading the counter resets it
            got = run_planar(torch, ctx, d_co, info, region, 1, False)
            assert ctx.fallback_count() == 0
            for a, e in zip(got, want(data, region, 1, False)):
                assert np.array_equal(a[0].reshape(e.shape), e)
    finally:
        ctx.set_force_exact(0)
        ctx.set_decode_tolerance(0)


def test_decoder_class_mirror(J, ctx, tmp_path):
    data = jpeg("own", 101, 70)
    path = tmp_path / "a.jpg"
    path.write_bytes(data)
    dec = J.Decoder(str(path), ctx=ctx)
    for scale, region in ((1, (33, 9, 40, 20)), (4, (5, 3, 20, 11))):
        for gray in (False, True):
            got = dec.decode(gray=gray, scale=scale, region=region)
            assert (dec.pr.width, dec.pr.height) == (101, 70)
            ref = ctx.decode_jpeg_region(data, region, scale=scale, gray=gray)[1:]
            assert all(np.array_equal(a, e) for a, e in zip(got, ref))
            assert all(np.array_equal(a.reshape(region[3], region[2]), e) for a, e in zip(got, want(data, region, scale, gray)))
    assert dec.decode(region=(100, 0, 2, 1)) is None
