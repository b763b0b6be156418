"""YCbCr 4:2:2 samples in and out on the GPU (include/jpezy_hip_ycc422.h): every comparison is for equality with
tests/ycc422_model.py.  Encode: planar I422 / NV16 / NV61 and packed YUY2 / UYVY / YVYU through the device entries at the sizes that reach
each path of a 128 x 8 octet in a 4-wave workgroup, the anchor against the RGB 4:2:2 entry, strides and bases, the force levels with their
counters, the shipped overflow path, the settings, the refusals, the launch split.  Decode: files of every layout into the three packed
formats, strides, bases and canaries on the device entry, the file entry's statuses."""
import ctypes as C
import io
from functools import lru_cache

import numpy as np
import pytest

from exact_picture import EXACT_F, QUEUE_CAP, exact_picture
import quant_model as QM
import sampling422_model as S2
import ycc422_model as M
import ycc_model as YM

pytestmark = pytest.mark.gpu

UNSUPPORTED, NOSPACE = -4, -6
UNIT_COEFFS = 2048                      # an octet: 8 MCUs x 4 blocks x 64
PLANAR = ["I422", "NV16", "NV61"]
PACKED = [("YUY2", M.YUY2), ("UYVY", M.UYVY), ("YVYU", M.YVYU)]
FORMS = PLANAR + [n for n, _ in PACKED]
CANARY = 0xEE


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


@pytest.fixture
def qctx(J, ctx):
    """the module's context, handed back at its defaults"""
    yield ctx
    ctx.set_quant_tables(None, None)
    ctx.set_variant(1)
    ctx.set_force_exact(0)
    ctx.set_huffman_optimize(0)
    ctx.set_restart_interval(0)
    ctx.set_chroma_downsampling(J.DOWNSAMPLE_POINT)


@lru_cache(maxsize=None)
def _planes(W, H, kind="random", seed=0):
    if kind == "random":
        out = M.random_planes(W, H, seed)
    else:
        v = {"flat0": 0, "flat255": 255}[kind]
        out = tuple(np.full(s, v, np.uint8) for s in ((H, W), (H, (W + 1) // 2), (H, (W + 1) // 2)))
    for p in out:
        p.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def _want(W, H, kind="random", seed=0, tables="q50"):
    co = M.encode_coeffs(*_planes(W, H, kind, seed), *QM.tables(tables))
    co.setflags(write=False)
    return co


def _shape(W, H):
    mc, mr, _ = S2.geometry(W, H)
    return (mr, mc, 4, 64)


def _out(torch, W, H, n=None):
    return torch.full(_shape(W, H) if n is None else (n,) + _shape(W, H), 0x5A5A, dtype=torch.int16, device="cuda")


def _view(torch, frames, row_stride, base, frame_stride=None):
    """a device view (n, H, B) -- (H, B) for one frame -- of the host arrays `frames` (each (H, B) uint8) inside a canary-filled buffer:
    first byte at `base`, rows row_stride, frames frame_stride apart.  -> (view, whole buffer)"""
    n, (H, B) = len(frames), frames[0].shape
    fs = frame_stride if frame_stride is not None else H * row_stride
    size = base + (n - 1) * fs + (H - 1) * row_stride + B
    buf = torch.full((size + 64,), CANARY, dtype=torch.uint8, device="cuda")
    v = buf[base:].as_strided((n, H, B), (fs, row_stride, 1))
    v.copy_(torch.from_numpy(np.stack(frames)).cuda())
    return (v if n > 1 else v[0]), buf


def _layout(kind, B):
    """(row_stride, base, n_frames) of a kind for rows of B bytes"""
    return {"tight": (B, 0, 1), "pad16": (B + 16, 0, 1), "pad5": (B + 5, 0, 1), "base1": (B, 1, 1), "base8": (B, 8, 1), "frames2": (B + 16, 0, 2)}[kind]


def _encode(J, ctx, form, frames, W, H, kind="tight"):
    """one device call of `form` on the frames [(y, cb, cr), ...] laid out as `kind` says -> int16 coefficients (n,) + shape"""
    import torch
    n = len(frames)
    co = _out(torch, W, H, n if n > 1 else None)
    if form in PLANAR:
        ys, base, _ = _layout(kind, W)
        yv, _ = _view(torch, [f[0] for f in frames], ys, base)
        CW = (W + 1) // 2
        if form == "I422":
            cs, cbase, _ = _layout(kind, CW)
            cb, _ = _view(torch, [f[1] for f in frames], cs, cbase)
            cr, _ = _view(torch, [f[2] for f in frames], cs, cbase)
        else:
            first, second = (1, 2) if form == "NV16" else (2, 1)
            uv = [np.stack([f[first], f[second]], -1).reshape(H, 2 * CW) for f in frames]
            cs, cbase, _ = _layout(kind, 2 * CW)
            v, _ = _view(torch, uv, cs, cbase)
            lo, hi = v[..., 0::2], v[..., 1::2]
            cb, cr = (lo, hi) if form == "NV16" else (hi, lo)
        ctx.fdct_quant_ycc422_dev(yv, cb, cr, co)
    else:
        fmt = dict(PACKED)[form]
        rs, base, _ = _layout(kind, M.row_bytes(W))
        img, _ = _view(torch, [M.pack(*f, fmt) for f in frames], rs, base)
        ctx.fdct_quant_yuv422_dev(img, co, W=W, format=fmt)
    torch.cuda.synchronize()
    return co.cpu().numpy()


def _same(got, want, tag):
    bad = np.argwhere(got != want)
    assert bad.size == 0, (tag, len(bad), bad[:4].tolist())


# ---- 1. encode equals the model ----
@pytest.mark.parametrize("W,H", M.SIZES)
def test_encode_equals_the_model(J, ctx, W, H):
    for form in FORMS:
        _same(_encode(J, ctx, form, [_planes(W, H)], W, H), _want(W, H), (form, W, H))


# ---- 2. the anchor ----
@pytest.mark.parametrize("W,H", M.ANCHOR_SIZES)
def test_anchor_planes_from_rgb_give_the_rgb_entrys_coefficients(J, ctx, oracle, W, H):
    import torch
    r, g, b = oracle.synth_rgb(W, H)
    co = _out(torch, W, H)
    ctx.fdct_quant_dev(*[torch.from_numpy(np.asarray(p).copy()).cuda() for p in (r, g, b)], W, H, co, sampling=J.SAMPLING_422)
    torch.cuda.synchronize()
    want = co.cpu().numpy()
    planes = M.planes_from_rgb(r, g, b, W, H)
    _same(_encode(J, ctx, "I422", [planes], W, H), want, "planar")
    _same(_encode(J, ctx, "YUY2", [planes], W, H), want, "packed")


# ---- 3. strides and bases ----
@pytest.mark.parametrize("kind", ["pad16", "pad5", "base1", "base8", "frames2"])
@pytest.mark.parametrize("W,H", [(128, 8), (130, 47), (1024, 16)])
def test_encode_strides_and_base(J, ctx, W, H, kind):
    """pad16 and frames2 keep the aligned forms where W % 16 == 0, pad5, base1 and base8 take the byte loop: the same coefficients"""
    n = _layout(kind, 1)[2]
    frames = [_planes(W, H, seed=f) for f in range(n)]
    want = np.stack([_want(W, H, seed=f) for f in range(n)]) if n > 1 else _want(W, H)
    for form in FORMS:
        _same(_encode(J, ctx, form, frames, W, H, kind), want, (form, kind))


# ---- 4. the force levels and their counters ----
@pytest.mark.parametrize("kind", ["random", "flat0", "flat255"])
@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_force_levels(J, qctx, level, kind):
    """whole octets only (128 x 8: one, 1024 x 16: sixteen): the queue walk of levels 1 and 2 counts the coefficients of live MCUs, the
    per-lane evaluator of level 3 whole octets -- the same 2048 a unit here"""
    qctx.set_force_exact(level)
    for W, H, units in [(128, 8, 1), (1024, 16, 16)]:
        for form in ("I422", "NV16", "UYVY"):
            qctx.fallback_count()
            _same(_encode(J, qctx, form, [_planes(W, H, kind)], W, H), _want(W, H, kind), (form, level, kind))
            n = qctx.fallback_count()
            if level:
                assert n == UNIT_COEFFS * units, (form, level, kind, n)
            elif kind != "random":
                assert n == 0, (form, kind, n)


# ---- 5. the shipped overflow path, without the hook ----
def test_queue_overflow_without_the_force_hook(J, qctx):
    """exact_picture's samples + 128 as planes (128 x 16: two whole units) at quality 100: 23 AC coefficients of every block sit exactly
    on an integer, 736 of a unit's 2048 against a queue of 382 -- the per-lane evaluator of the aligned planar, aligned packed and
    byte-loop instances runs without the hook, and the counter shows it"""
    W, H = 128, 16
    _, _, _, (Y, Cb, Cr) = exact_picture(W, H, 2)
    planes = tuple((p + 128).astype(np.uint8) for p in (Y, Cb, Cr))
    assert all(((p + 128) >= 0).all() and ((p + 128) <= 255).all() for p in (Y, Cb, Cr))
    d = M.dct(*planes)
    hits = np.count_nonzero(np.array(EXACT_F)) * 32
    assert hits == 736 and hits > QUEUE_CAP and (np.count_nonzero(d.reshape(-1, 64)[:, 1:], axis=1) == 23).all()
    tabs = QM.tables("q100")
    want = S2.quantise(d, *tabs)
    qctx.set_quant_tables(*tabs)
    for form, kind in [("I422", "tight"), ("NV16", "tight"), ("YUY2", "tight"), ("UYVY", "pad16"), ("I422", "base1"), ("YVYU", "pad5")]:
        qctx.fallback_count()
        _same(_encode(J, qctx, form, [planes], W, H, kind), want, (form, kind))
        assert qctx.fallback_count() == 2 * UNIT_COEFFS, (form, kind)


# ---- 6. the settings compose ----
@pytest.mark.parametrize("W,H", [(65, 47), (208, 40)])
def test_settings_compose(J, qctx, W, H):
    y, cb, cr = _planes(W, H)
    img = M.pack(y, cb, cr, M.UYVY)
    mc = S2.geometry(W, H)[0]
    for name, opt, ri in [("q10", 0, 0), ("q100", 0, 1), ("random", 1, mc), ("q50", 1, 1), ("q50", 0, mc)]:
        tabs = QM.tables(name)
        qctx.set_quant_tables(*tabs)
        qctx.set_huffman_optimize(opt)
        qctx.set_restart_interval(ri)
        co = M.encode_coeffs(y, cb, cr, *tabs)
        ref = S2.write_jpeg(co, W, H, quant_tables=tabs, ri=ri, optimize=bool(opt))
        assert qctx.encode_jpeg_yuv422(img, W=W, format=J.YUV_UYVY) == ref, (name, opt, ri, "packed")
        assert qctx.encode_jpeg_ycc422(y, cb, cr) == ref, (name, opt, ri, "planar")
        uv = np.stack([cb, cr], -1)
        assert qctx.encode_jpeg_ycc422(y, uv[..., 0], uv[..., 1]) == ref, (name, opt, ri, "NV16")
        info, back = J.read_jpeg(ref)
        assert (info.H[0], info.V[0], info.H[1], info.V[1], info.H[2], info.V[2]) == (2, 1, 1, 1, 1, 1)
        assert np.array_equal(back, co)


# ---- 7. refusals with a live context ----
def test_variant_0_is_refused_and_the_context_stays_usable(J, qctx):
    import torch
    W, H = 16, 8
    y, cb, cr = _planes(W, H)
    img = M.pack(y, cb, cr, M.YUY2)
    lib = J.load_library()
    qctx.set_variant(0)
    dev = [torch.from_numpy(p.copy()).cuda() for p in (y, cb, cr, img)]
    co = _out(torch, W, H)
    out = np.zeros(J.jpeg_bound(W, H, J.SAMPLING_422), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    calls = [lambda: lib.jpezy_fdct_quant_ycc422_dev(qctx._h, dev[0].data_ptr(), 0, dev[1].data_ptr(), dev[2].data_ptr(), 0, 1, 0, 0, W, H, 1, co.data_ptr(), None),
             lambda: lib.jpezy_fdct_quant_yuv422_dev(qctx._h, dev[3].data_ptr(), 0, 0, 0, W, H, 1, co.data_ptr(), None),
             lambda: lib.jpezy_encode_jpeg_ycc422(qctx._h, p(y), 0, p(cb), p(cr), 0, 1, W, H, b"", p(out), out.size),
             lambda: lib.jpezy_encode_jpeg_yuv422(qctx._h, p(img), 0, 0, W, H, b"", p(out), out.size)]
    for k, call in enumerate(calls):
        assert call() == UNSUPPORTED, k
        assert b"variant 0" in lib.jpezy_hip_last_error()
    torch.cuda.synchronize()
    assert (co.cpu().numpy() == 0x5A5A).all()
    qctx.set_variant(1)
    _same(_encode(J, qctx, "YUY2", [(y, cb, cr)], W, H), _want(W, H), "after the refusal")


def test_averaged_downsampling_is_not_consulted(J, qctx):
    W, H = 65, 47
    y, cb, cr = _planes(W, H)
    before = qctx.encode_jpeg_ycc422(y, cb, cr), qctx.encode_jpeg_yuv422(M.pack(y, cb, cr, M.YVYU), W=W, format=J.YUV_YVYU)
    qctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
    after = qctx.encode_jpeg_ycc422(y, cb, cr), qctx.encode_jpeg_yuv422(M.pack(y, cb, cr, M.YVYU), W=W, format=J.YUV_YVYU)
    assert before == after and before[0] == before[1]
    _same(_encode(J, qctx, "I422", [(y, cb, cr)], W, H), _want(W, H), "averaged set")


# ---- 8. decode ----
def _pil_file(mode, subsampling, W, H):
    from PIL import Image
    from oracle import oracle as O
    r, g, b = O.synth_rgb(W, H, frame=9)
    img = np.stack([p.reshape(H, W) for p in (r, g, b)], -1) // 2 + 40
    buf = io.BytesIO()
    if mode == "L":
        Image.fromarray(img[..., 0].astype(np.uint8), "L").save(buf, "JPEG", quality=85)
    else:
        Image.fromarray(img.astype(np.uint8), "RGB").save(buf, "JPEG", quality=85, subsampling=subsampling)
    return buf.getvalue()


@lru_cache(maxsize=None)
def _file(J, ctx, source, W, H):
    from oracle import oracle as O
    r, g, b = O.synth_rgb(W, H, frame=5)
    if source == "own420":
        return ctx.encode_jpeg(r, g, b, W, H)
    if source == "own422":
        return ctx.encode_jpeg(r, g, b, W, H, sampling=J.SAMPLING_422)
    if source == "own444":
        return ctx.encode_jpeg(r, g, b, W, H, sampling=J.SAMPLING_444)
    if source == "own_gray":
        return ctx.encode_jpeg(r, g, b, W, H, gray=True)
    return _pil_file(*{"pil444": ("RGB", 0), "pil422": ("RGB", 1), "pil_L": ("L", None)}[source], W, H)


@pytest.mark.parametrize("source", ["own420", "own422", "own444", "own_gray", "pil444", "pil422", "pil_L"])
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (17, 9), (130, 47), (1024, 16)])
def test_decode_equals_the_model(J, ctx, oracle, source, W, H):
    data = _file(J, ctx, source, W, H)
    info_o, co = oracle.read_jpeg(data)
    _, y, cb, cr = ctx.decode_jpeg_ycc(data)
    for name, fmt in PACKED:
        want = M.decode_yuv422(co, info_o, fmt)
        info, img = ctx.decode_jpeg_yuv422(data, format=fmt)
        assert (info.width, info.height, info.ncomp) == (W, H, info_o.ncomp) and img.shape == (H, M.row_bytes(W))
        assert np.array_equal(img, want), (source, name)
        gy, gcb, gcr = M.unpack(img, W, fmt)
        assert np.array_equal(gy, y[:H, :W]), (source, name)
        if source in ("own422", "pil422"):
            assert np.array_equal(gcb, cb) and np.array_equal(gcr, cr), (source, name)
        if info_o.ncomp == 1:
            assert (gcb == 0x80).all() and (gcr == 0x80).all()
        if W & 1:                           # the duplicated Y of the last macropixel
            oy = M.OFFSETS[fmt][0]
            assert np.array_equal(img[:, 4 * (W // 2) + oy + 2], img[:, 4 * (W // 2) + oy])


# ---- 9. decode strides, bases and canaries on the device entry ----
@pytest.mark.parametrize("kind", ["tight", "pad16", "pad5", "base1", "base8", "frames2"])
@pytest.mark.parametrize("W,H", [(130, 47), (1024, 16)])
def test_decode_strides_bases_and_canaries(J, ctx, oracle, W, H, kind):
    import torch
    B = M.row_bytes(W)
    rs, base, n = _layout(kind, B)
    fs = H * rs + (48 if n > 1 else 0)
    files = [_file(J, ctx, "own422", W, H)] * n                 # frames of ONE layout and set of tables: the same file
    parsed = [oracle.read_jpeg(d) for d in files]
    info = J.read_jpeg(files[0])[0]
    d_co = torch.from_numpy(np.stack([np.asarray(co, np.int16).reshape(-1) for _, co in parsed])).cuda()
    for name, fmt in PACKED:
        size = base + (n - 1) * fs + (H - 1) * rs + B
        buf = torch.full((size + 64,), CANARY, dtype=torch.uint8, device="cuda")
        view = buf[base:].as_strided((n, H, B), (fs, rs, 1))
        ctx.dequant_idct_generic_yuv422_dev(d_co, info, view if n > 1 else view[0], format=fmt)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        want = np.full(got.shape, CANARY, np.uint8)
        for f in range(n):
            img = M.decode_yuv422(parsed[f][1], parsed[f][0], fmt)
            for yy in range(H):
                o = base + f * fs + yy * rs
                want[o:o + B] = img[yy]
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, kind, len(bad), bad[:4].tolist())


# ---- 10. the file entry's statuses ----
def test_decode_file_statuses(J, ctx):
    lib = J.load_library()
    W, H = 17, 9
    data = np.frombuffer(_file(J, ctx, "own420", W, H), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    info = J.FrameInfo()
    assert lib.jpezy_decode_jpeg_yuv422(ctx._h, p(data), data.size, C.byref(info), 0, 0, None, 0) == 0        # header only
    assert (info.width, info.height) == (W, H)
    B, rs = M.row_bytes(W), M.row_bytes(W) + 7
    need = (H - 1) * rs + B
    pix = np.full(need + 16, CANARY, np.uint8)
    assert lib.jpezy_decode_jpeg_yuv422(ctx._h, p(data), data.size, C.byref(info), 1, rs, p(pix), need - 1) == NOSPACE
    assert (pix == CANARY).all()
    assert lib.jpezy_decode_jpeg_yuv422(ctx._h, p(data), data.size, C.byref(info), 1, rs, p(pix), need) == 0
    want = ctx.decode_jpeg_yuv422(data.tobytes(), format=J.YUV_UYVY)[1]
    rows = np.lib.stride_tricks.as_strided(pix, (H, rs), (rs, 1))
    assert np.array_equal(rows[:, :B], want)
    assert (rows[:-1, B:] == CANARY).all() and (pix[need:] == CANARY).all()                                 # only row_bytes of a row are written
    assert lib.jpezy_decode_jpeg_yuv422(ctx._h, p(data), data.size, C.byref(info), 0, B - 1, p(pix), pix.size) == -1
    assert b"row_stride" in lib.jpezy_hip_last_error()
    garbage = np.frombuffer(b"\xff\xd8 not a jpeg at all " * 4, np.uint8)
    rc = lib.jpezy_decode_jpeg_yuv422(ctx._h, p(garbage), garbage.size, C.byref(info), 0, 0, p(pix), pix.size)
    assert rc < 0 and rc == lib.jpezy_decode_jpeg_ycc(ctx._h, p(garbage), garbage.size, C.byref(info), None, 0, 0, None, None, 0, 1, 0)
    with pytest.raises(J.JpezyError):
        ctx.decode_jpeg_yuv422(garbage.tobytes())


# ---- 11. the launch split ----
def test_encode_across_the_65535_frame_split(J, ctx):
    """65537 frames of 16 x 8 in YUY2: two launches; the frames around the seam and a random sample against the model"""
    import torch
    W, H, n = 16, 8, 65537
    rng = np.random.default_rng(422)
    imgs = rng.integers(0, 256, (n, H, M.row_bytes(W)), dtype=np.uint8)
    co = _out(torch, W, H, n)
    ctx.fdct_quant_yuv422_dev(torch.from_numpy(imgs).cuda(), co, format=J.YUV_YUY2)
    torch.cuda.synchronize()
    got = co.cpu().numpy()
    assert not (got.reshape(n, -1) == 0x5A5A).all(axis=1).any()         # every frame was written
    pick = sorted({0, 1, 65533, 65534, 65535, 65536} | set(rng.integers(0, n, 24).tolist()))
    tabs = QM.tables("q50")
    for f in pick:
        _same(got[f], M.encode_coeffs_packed(imgs[f], W, M.YUY2, *tabs), f)
