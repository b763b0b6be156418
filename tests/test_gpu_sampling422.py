"""4:2:2 chroma sampling on the GPU (include/jpezy_hip.h, CHROMA SAMPLING): the transform kernel against
tests/sampling422_model.py for equality -- planes aligned and deliberately misaligned, the four packed formats with aligned and unaligned
row strides, every force_exact level, the DC by formula and by table, quality and caller tables, a batch, both chroma rules --, the rare
paths on a picture built for them, the GPU entropy coder and histogram on 4-block MCUs against the host writer, the end-to-end entries
against the model's file, those files through our own decoders, the refusals, SAMPLING_420 / SAMPLING_444 against their own models, and
the three *_dev entries on a caller's stream and under capture.

Shapes (the work unit: 8 horizontally adjacent 16 x 8 MCUs = 128 x 8 pixels per wave): W in 16 (one MCU, seven dead slots), 17 and 31
(a partial MCU at odd widths: clamp, byte loop), 128 (exactly one unit: the 16-byte load path), 144 (one unit and a partial one), 1;
H in 8, 9 (a second MCU row of clamped rows), 1."""
from functools import lru_cache

import numpy as np
import pytest

from exact_picture import EXACT_F, QUEUE_CAP, exact_picture
import quant_model as QM
import sampling422_model as S2
import sampling_model as SM
import stream_probe as SP

pytestmark = pytest.mark.gpu

WIDTHS, HEIGHTS = [16, 17, 31, 128, 144, 1], [8, 9, 1]
TABLES = ["q10", "q50", "q100", "random"]
UNSUPPORTED = -4
MODES = [S2.POINT, S2.AVERAGE]


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
    ctx.set_dc_table_lookup(0)
    ctx.set_huffman_optimize(0)
    ctx.set_restart_interval(0)
    ctx.set_chroma_downsampling(J.DOWNSAMPLE_POINT)
    ctx.set_huffdec_min_bytes(32 << 10)


@lru_cache(maxsize=None)
def _rgb(W, H, frame=0):
    from oracle import oracle as O
    return O.synth_rgb(W, H, frame=frame)


def _want(W, H, name, frame=0, mode=S2.POINT):
    return S2.quantise(S2.synth_dct(W, H, frame, mode), *QM.tables(name))


def _shape(W, H):
    mc, mr, _ = S2.geometry(W, H)
    return (mr, mc, 4, 64)


def _out(torch, W, H, n=None):
    shape = _shape(W, H) if n is None else (n,) + _shape(W, H)
    return torch.full(shape, 0x5A5A, dtype=torch.int16, device="cuda")


def _dev_entries(J, ctx, r, g, b, W, H, full=True):
    """every way in: planes tight (aligned bases: the 16-byte load path where W % 16 == 0), planes at base + 1 with an odd plane stride
    (the byte loop), and the four packed formats (full=False: RGB24 and BGRA32), each with a tight row stride, with rows padded by 16
    bytes (3-byte pixels: 48) and with an unaligned row stride (row + 15 bytes; 4-byte pixels: base + 1, row + 5 bytes)"""
    import torch
    S = J.SAMPLING_422
    out = []
    planes = [torch.from_numpy(np.asarray(p).copy()).cuda() for p in (r, g, b)]
    co = _out(torch, W, H)
    ctx.fdct_quant_dev(*planes, W, H, co, sampling=S)
    out.append(("planar", co))
    odd = W * H + 3 if (W * H) % 2 == 0 else W * H + 2                     # an odd plane stride, frames (one here) that far apart
    shifted = []
    for p in (r, g, b):
        buf = torch.full((odd + 1,), 0xEE, dtype=torch.uint8, device="cuda")
        buf[1:1 + W * H] = torch.from_numpy(np.asarray(p).copy()).cuda()
        shifted.append(buf[1:])
    co = _out(torch, W, H)
    ctx.fdct_quant_dev(*shifted, W, H, co, plane_stride=odd, sampling=S)
    out.append(("planar base + 1, odd stride", co))
    rgb = np.stack([np.asarray(p).reshape(H, W) for p in (r, g, b)], axis=-1)
    formats = [("RGB24", J.PIX_RGB24, rgb), ("BGR24", J.PIX_BGR24, rgb[..., ::-1]),
               ("RGBA32", J.PIX_RGBA32, np.concatenate([rgb, np.full((H, W, 1), 9, np.uint8)], axis=-1)),
               ("BGRA32", J.PIX_BGRA32, np.concatenate([rgb[..., ::-1], np.full((H, W, 1), 9, np.uint8)], axis=-1))]
    for name, fmt, img in formats if full else formats[:1] + formats[3:]:
        nb = img.shape[-1]
        co = _out(torch, W, H)
        ctx.fdct_quant_packed_dev(torch.from_numpy(np.ascontiguousarray(img)).cuda(), co, format=fmt, sampling=S)
        out.append((name + " tight", co))
        for pad_px, tag in ((16 // nb if nb == 4 else 16, "aligned pad"), (5 if nb == 3 else 0, "unaligned pad")):
            if pad_px == 0:                                                # 4-byte pixels: an unaligned row stride through a byte view
                flat = torch.full((H * (W * 4 + 5) + 8,), 7, dtype=torch.uint8, device="cuda")
                view = flat[1:1 + H * (W * 4 + 5)].as_strided((H, W, 4), (W * 4 + 5, 4, 1))
                view.copy_(torch.from_numpy(np.ascontiguousarray(img)).cuda())
            else:
                wide = np.full((H, W + pad_px, nb), 7, np.uint8)
                wide[:, :W] = img
                view = torch.from_numpy(wide).cuda()[:, :W]
            co = _out(torch, W, H)
            ctx.fdct_quant_packed_dev(view, co, format=fmt, sampling=S)
            out.append((f"{name} {tag}", co))
    torch.cuda.synchronize()
    return [(n, c.cpu().numpy()) for n, c in out]


def _check_every_entry(J, ctx, r, g, b, W, H, want, tag, full=True):
    for entry, co in _dev_entries(J, ctx, r, g, b, W, H, full):
        bad = np.argwhere(co != want)
        assert bad.size == 0, (entry, tag, len(bad), bad[:4].tolist())


# ---- coefficients ----
@pytest.mark.parametrize("mode", MODES, ids=["point", "average"])
@pytest.mark.parametrize("name", TABLES)
def test_coefficients_equal_the_model_on_the_full_cross(J, qctx, name, mode):
    """144 x 9 (one unit and a partial one, two MCU rows, clamped rows): every table set x force_exact {0, 1, 2, 3} x every entry; and
    once more with the DC read from the exact table"""
    W, H = 144, 9
    qctx.set_quant_tables(*QM.tables(name))
    qctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE if mode == S2.AVERAGE else J.DOWNSAMPLE_POINT)
    want = _want(W, H, name, mode=mode)
    for fe in (0, 1, 2, 3):
        qctx.set_force_exact(fe)
        qctx.fallback_count()
        _check_every_entry(J, qctx, *_rgb(W, H), W, H, want, (name, fe, mode), full=fe == 0)
        n = qctx.fallback_count()
        if fe:
            assert n >= want.size, (name, fe, n)          # the test hooks send every coefficient down the exact paths
    qctx.set_force_exact(0)
    qctx.set_dc_table_lookup(1)
    _check_every_entry(J, qctx, *_rgb(W, H), W, H, want, (name, "dc table", mode), full=False)


@pytest.mark.parametrize("mode", MODES, ids=["point", "average"])
@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("W", WIDTHS)
def test_coefficients_equal_the_model_on_every_shape(J, qctx, W, H, mode):
    qctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE if mode == S2.AVERAGE else J.DOWNSAMPLE_POINT)
    for name in ("q50", "q100"):
        qctx.set_quant_tables(*QM.tables(name))
        want = _want(W, H, name, mode=mode)
        for fe in (0, 3) if name == "q100" else (0,):
            qctx.set_force_exact(fe)
            _check_every_entry(J, qctx, *_rgb(W, H), W, H, want, (name, fe, mode), full=fe == 0)


def test_average_differs_from_point_and_agrees_on_doubled_pixels(J, qctx):
    """the setting acts (a context that says average does not point-sample), and on a picture whose horizontal pixel pairs are equal the
    two rules give the same coefficients"""
    import torch
    W, H = 128, 8
    r, g, b = _rgb(W, H)
    assert not np.array_equal(_want(W, H, "q50"), _want(W, H, "q50", mode=S2.AVERAGE))
    dbl = [np.repeat(np.asarray(p).reshape(H, W)[:, 0::2], 2, axis=1).reshape(-1) for p in (r, g, b)]
    planes = [torch.from_numpy(p.copy()).cuda() for p in dbl]
    got = []
    for mode in (J.DOWNSAMPLE_POINT, J.DOWNSAMPLE_AVERAGE):
        qctx.set_chroma_downsampling(mode)
        co = _out(torch, W, H)
        qctx.fdct_quant_dev(*planes, W, H, co, sampling=J.SAMPLING_422)
        torch.cuda.synchronize()
        got.append(co.cpu().numpy())
    assert np.array_equal(got[0], got[1])
    assert np.array_equal(got[0], S2.encode_coeffs(*dbl, W, H, *QM.tables("q50")))


# ---- the rare paths, for certain ----
@lru_cache(maxsize=None)
def _guard_band_triples():
    """RGB triples whose exact Y, Cb or Cr is an integer: there the FP32 estimate lands inside its guard band and the reference's own FP64
    rounding decides (jpezy_f32_quad.h; tests/test_f32_error_bound.py checks the bands over all 2^24 triples).  A few hundred of each."""
    g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    out = {"y": [], "cb": [], "cr": []}
    for r in range(0, 256, 5):
        for key, n, mod in (("y", 299 * r + 587 * g + 114 * b, 1000), ("cb", -1687 * r - 3313 * g + 5000 * b, 10000),
                            ("cr", 5000 * r - 4187 * g - 813 * b, 10000)):
            gi, bi = np.nonzero(n % mod == 0)
            out[key] += [(r, int(x), int(y)) for x, y in zip(gi[:12], bi[:12])]
    return out


@pytest.mark.parametrize("mode", MODES, ids=["point", "average"])
def test_rare_paths_without_the_force_hook(J, qctx, mode):
    """Two pictures of 144 x 9 at force_exact 0.  (a) Pixels from the guard-band triples only: the colour votes fire in every wave, and
    at quality 100 (every quantiser 1: the widest level-1 bands, no zero coefficients) some coefficients are queued.  (b) Gray blocks
    128 + a (u4(x) + u4(y)) / 2 + a u4(x) u4(y) / 2 with u4 the sign pattern + - - + + - - + of the fourth basis function and a a
    multiple of 8: the luma coefficients (0, 4), (4, 0), (4, 4) -- the rational ones, every cosine +-cos(pi/4) -- are then multiples of
    a, exactly ON a truncation boundary at every quantiser that divides them, which only level 3, the reference's own order of
    operations, can decide.  Equality with the model is then a statement about levels 2 and 3; the counter shows that they ran.  (The queue
    overflow has a picture and a test of its own below.)"""
    W, H = 144, 9
    T = _guard_band_triples()
    assert min(len(v) for v in T.values()) >= 100
    rng = np.random.default_rng(422)
    pix = np.array([T[k][i] for k, i in zip(rng.choice(["y", "cb", "cr"], W * H), rng.integers(0, 100, W * H))], np.uint8)
    band = tuple(np.ascontiguousarray(pix[:, k]) for k in range(3))
    u4 = np.array([1, -1, -1, 1, 1, -1, -1, 1])
    yy, xx = np.mgrid[0:H, 0:W]
    amp = 8 * (1 + (xx // 8 + yy // 8) % 7)                                # per block: multiples of 8, so that n / 8 steps are integers
    v = (128 + amp * (u4[xx % 8] + u4[yy % 8]) // 2 + amp * u4[xx % 8] * u4[yy % 8] // 2).astype(np.uint8).reshape(-1)
    flat = (v, v.copy(), v.copy())
    qctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE if mode == S2.AVERAGE else J.DOWNSAMPLE_POINT)
    for what, (r, g, b) in (("guard band", band), ("rational", flat)):
        dct = S2.dct_from_rgb(r, g, b, W, H, mode)
        for name in ("q100", "q50"):
            qctx.set_quant_tables(*QM.tables(name))
            want = S2.quantise(dct, *QM.tables(name))
            qctx.fallback_count()
            _check_every_entry(J, qctx, r, g, b, W, H, want, (what, name), full=False)
            if name == "q100":
                assert qctx.fallback_count() > 0, what


# ---- the queue overflow, for certain ----
UNIT_COEFFS = 2048                                                         # 32 blocks of a 4:2:2 work unit


@pytest.mark.parametrize("mode", MODES, ids=["point", "average"])
def test_queue_overflow_without_the_force_hook(J, qctx, mode):
    """256 x 16 (four whole work units) at force_exact 0 and quality 100: every block of the picture has 23 AC coefficients exactly on an
    integer -- each one on a truncation boundary at Q = 1, flagged by level 1 and queued --, 736 of a unit's 2048 coefficients against a
    queue of 382: the queue overflows and the per-lane evaluator of the shipped instances (16-byte loads, byte loop, packed) runs without
    the hook.  Equality with the model, which truncates several of these coefficients one below their exact value as the reference's
    FP64 order does; the counter shows that every coefficient of every unit went through the evaluator."""
    import torch
    W, H = 256, 16
    r, g, b, (Y, Cb, Cr) = exact_picture(W, H, 2)          # both pixels of a horizontal pair carry the pair's chroma sample
    ys, cbs, crs = S2.samples_from_rgb(r, g, b, W, H, mode)
    assert np.array_equal(ys, Y) and np.array_equal(cbs, Cb) and np.array_equal(crs, Cr)      # the samples ARE the pattern, either rule
    dct = S2.dct_from_rgb(r, g, b, W, H, mode)
    hits = np.count_nonzero(np.array(EXACT_F)) * 32
    assert hits > QUEUE_CAP and (np.count_nonzero(dct.reshape(-1, 64)[:, 1:], axis=1) == 23).all()
    assert (dct[0, 0, 0].reshape(8, 8) != np.array(EXACT_F)).any()         # the reference's order is off the exact value somewhere
    qctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE if mode == S2.AVERAGE else J.DOWNSAMPLE_POINT)
    qctx.set_quant_tables(*QM.tables("q100"))
    want = S2.quantise(dct, *QM.tables("q100"))
    planes = [torch.from_numpy(p.copy()).cuda() for p in (r, g, b)]
    co = _out(torch, W, H)
    qctx.fallback_count()
    qctx.fdct_quant_dev(*planes, W, H, co, sampling=J.SAMPLING_422)
    torch.cuda.synchronize()
    assert qctx.fallback_count() == 4 * UNIT_COEFFS                        # four units, each one whole through the evaluator
    assert np.array_equal(co.cpu().numpy(), want)
    entries = _dev_entries(J, qctx, r, g, b, W, H)
    assert qctx.fallback_count() == len(entries) * 4 * UNIT_COEFFS
    for entry, got in entries:
        bad = np.argwhere(got != want)
        assert bad.size == 0, (entry, len(bad), bad[:4].tolist())


# ---- batch ----
@pytest.mark.parametrize("stride_pad", [48, 41], ids=["aligned", "odd"])
def test_batch_of_three_frames(J, qctx, stride_pad):
    import torch
    W, H, F = 144, 9, 3
    stride = W * H + stride_pad
    planes = []
    for k in range(3):
        buf = np.full(F * stride, 0xEE, np.uint8)
        for f in range(F):
            buf[f * stride:f * stride + W * H] = _rgb(W, H, f)[k]
        planes.append(torch.from_numpy(buf).cuda())
    co = _out(torch, W, H, F)
    qctx.fdct_quant_dev(*planes, W, H, co, n_frames=F, plane_stride=stride, sampling=J.SAMPLING_422)
    img = np.stack([np.stack([p.reshape(H, W) for p in _rgb(W, H, f)], axis=-1) for f in range(F)])
    cop = _out(torch, W, H, F)
    qctx.fdct_quant_packed_dev(torch.from_numpy(img).cuda(), cop, format=J.PIX_RGB24, sampling=J.SAMPLING_422)
    torch.cuda.synchronize()
    for f in range(F):
        assert np.array_equal(co[f].cpu().numpy(), _want(W, H, "q50", f)), f
        assert np.array_equal(cop[f].cpu().numpy(), _want(W, H, "q50", f)), ("packed", f)


# ---- the entropy coder and the histogram on 4-block MCUs ----
@lru_cache(maxsize=None)
def _field(W, H, kind):
    """coefficient fields [nmcu, 4, 64], read-only: the picture's own; dense small values; sparse with values up to +-1023 and DC steps of
    category 11"""
    mc, mr, _ = S2.geometry(W, H)
    n = mc * mr
    rng = np.random.default_rng(20261021 + W)
    if kind == "picture":
        a = np.array(_want(W, H, "q50")).reshape(n, 4, 64)
    elif kind == "dense":
        a = rng.integers(-12, 13, (n, 4, 64)).astype(np.int16)
    else:
        a = np.where(rng.random((n, 4, 64)) < 0.25, rng.integers(-1023, 1024, (n, 4, 64)), 0).astype(np.int16)
        a[:, :, 0] = np.where(np.arange(n) % 2 == 0, 1000, -1000)[:, None]
        a[:, 1, 0] *= -1
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("kind", ["picture", "dense", "large"])
@pytest.mark.parametrize("W,H", [(16, 8), (1040, 8)], ids=["one-mcu", "65-mcus"])
def test_gpu_writer_and_histogram_equal_the_host(J, qctx, W, H, kind):
    """16 x 8: one MCU; 1040 x 8: 65 MCUs = 260 blocks, the 256-block tile seam between MCU 63 and 64.  Restart interval {0, 1, 5, 64
    (interval = tile)} x optimise, the synchronous form, the device-resident form (optimise off) and the histogram kernel"""
    import torch
    co = _field(W, H, kind)
    d_co = torch.from_numpy(co.copy()).cuda()
    stride = J.jpeg_bound(W, H, J.SAMPLING_422)
    d_out = torch.zeros((1, stride), dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_hist = torch.zeros((1, 4, 256), dtype=torch.int64, device="cuda")
    for ri in (0, 1, 5, 64):
        qctx.set_restart_interval(ri)
        qctx.huffman_histogram_dev(d_co, W, H, d_hist, sampling=J.SAMPLING_422)
        torch.cuda.synchronize()
        want_hist = J.huffman_histogram(co, W, H, sampling=J.SAMPLING_422, restart_interval=ri)
        assert np.array_equal(d_hist[0].cpu().numpy().astype(np.uint64), want_hist), (kind, ri)
        for opt in (0, 1):
            qctx.set_huffman_optimize(opt)
            ref = J.write_jpeg(co, W, H, sampling=J.SAMPLING_422, optimize=bool(opt), restart_interval=ri)
            got = qctx.write_jpeg_gpu(d_co, W, H, sampling=J.SAMPLING_422)[0]
            assert got == ref, (kind, ri, opt, len(got), len(ref))
        qctx.set_huffman_optimize(0)
        d_out.zero_(); d_sizes.zero_()
        qctx.write_jpeg_gpu_dev(d_co, W, H, d_out, d_sizes, sampling=J.SAMPLING_422)
        torch.cuda.synchronize()
        n = int(d_sizes[0])
        ref0 = J.write_jpeg(co, W, H, sampling=J.SAMPLING_422, restart_interval=ri)
        assert n == len(ref0) and d_out[0, :n].cpu().numpy().tobytes() == ref0, (kind, ri, "dev")
        if kind == "dense":                                                # the host writer is the model's (also: tests/test_sampling422_host.py)
            assert ref0 == S2.write_jpeg(co.reshape(_shape(W, H)), W, H, ri=ri)


def test_gpu_writer_batch_and_a_frame_outside_the_code_tables(J, qctx):
    """three frames in one call; frame 1 holds a value of size 11: JPEZY_E_FORMAT (-5) for that frame only, in both forms; the device
    form refuses per-image tables"""
    import torch
    W, H = 1040, 8
    frames = np.stack([_field(W, H, "dense"), _field(W, H, "large"), _field(W, H, "dense")[::-1]]).copy()
    stride = J.jpeg_bound(W, H, J.SAMPLING_422)
    for ri in (0, 5):
        qctx.set_restart_interval(ri)
        for bad in (False, True):
            fr = frames.copy()
            if bad:
                fr[1, 63, 2, 7] = 1024
            refs = [J.write_jpeg(fr[f], W, H, sampling=J.SAMPLING_422, restart_interval=ri) if not (bad and f == 1) else -5 for f in range(3)]
            d_co = torch.from_numpy(fr).cuda()
            got = qctx.write_jpeg_gpu(d_co, W, H, n_frames=3, sampling=J.SAMPLING_422, raise_on_error=False)
            assert got == refs, (ri, bad)
            if bad:
                with pytest.raises(J.JpezyError, match="status -5"):
                    qctx.write_jpeg_gpu(d_co, W, H, n_frames=3, sampling=J.SAMPLING_422)
            d_out = torch.zeros((3, stride), dtype=torch.uint8, device="cuda")
            d_sizes = torch.zeros(3, dtype=torch.int64, device="cuda")
            qctx.write_jpeg_gpu_dev(d_co, W, H, d_out, d_sizes, n_frames=3, sampling=J.SAMPLING_422)
            torch.cuda.synchronize()
            sizes = d_sizes.cpu().tolist()
            for f in range(3):
                if isinstance(refs[f], int):
                    assert sizes[f] == refs[f], (ri, f)
                else:
                    assert sizes[f] == len(refs[f]) and d_out[f, :sizes[f]].cpu().numpy().tobytes() == refs[f], (ri, bad, f)
    qctx.set_huffman_optimize(1)
    with pytest.raises(J.JpezyError, match=f"status {UNSUPPORTED}"):
        qctx.write_jpeg_gpu_dev(d_co, W, H, d_out, d_sizes, n_frames=3, sampling=J.SAMPLING_422)
    with pytest.raises(J.JpezyError, match="status -1"):
        qctx.write_jpeg_gpu(d_co, W, H, gray=True, sampling=J.SAMPLING_422)


def test_gpu_writer_on_a_frame_of_more_than_2048_tiles(J, qctx):
    """5888 x 2880: 368 x 360 = 132480 MCUs = 529920 blocks = 2070 tiles -- past the size up to which the assembling kernel scans the
    tile totals itself.  A synthetic field, uploaded: flat (20 bits per MCU: the most tiles a piece of the stream can touch, the case
    the assembler's window bound is derived for) and a sparse one, without and with restart intervals"""
    import torch
    W, H = 5888, 2880
    n = 368 * 360
    assert J.sampling_geometry(J.SAMPLING_422, W, H) == (368, 360, 4) and (n * 4 + 255) // 256 > 2048
    rng = np.random.default_rng(5888)
    sparse = np.zeros((n, 4, 64), np.int16)
    idx = rng.integers(0, n, 20000)
    sparse[idx, rng.integers(0, 4, 20000), rng.integers(0, 64, 20000)] = rng.integers(-300, 301, 20000)
    for field in (np.zeros((n, 4, 64), np.int16), sparse):
        d_co = torch.from_numpy(field).cuda()
        for ri in (0, 368):
            qctx.set_restart_interval(ri)
            got = qctx.write_jpeg_gpu(d_co, W, H, sampling=J.SAMPLING_422)[0]
            assert got == J.write_jpeg(field, W, H, sampling=J.SAMPLING_422, restart_interval=ri), ri


# ---- end to end ----
@pytest.mark.parametrize("mode", MODES, ids=["point", "average"])
@pytest.mark.parametrize("W,H", [(144, 9), (31, 1)])
def test_encode_jpeg_equals_the_models_file(J, qctx, W, H, mode):
    r, g, b = _rgb(W, H)
    rgb = np.ascontiguousarray(np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1))
    qctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE if mode == S2.AVERAGE else J.DOWNSAMPLE_POINT)
    for name, opt, ri in (("q50", 0, 0), ("q10", 1, 5), ("q100", 0, 1), ("random", 1, 0)):
        tabs = QM.tables(name)
        qctx.set_quant_tables(*tabs)
        qctx.set_huffman_optimize(opt)
        qctx.set_restart_interval(ri)
        ref = S2.write_jpeg(_want(W, H, name, mode=mode), W, H, quant_tables=tabs, ri=ri, optimize=bool(opt))
        assert qctx.encode_jpeg(r, g, b, W, H, sampling=J.SAMPLING_422) == ref, (name, opt, ri)
        assert qctx.encode_jpeg_packed(rgb, sampling=J.SAMPLING_422) == ref, ("packed", name, opt, ri)
        assert qctx.encode_jpeg_packed(np.ascontiguousarray(rgb[..., ::-1]), format=J.PIX_BGR24, sampling=J.SAMPLING_422) == ref, ("BGR", name)


@pytest.mark.parametrize("ri", [0, 5])
def test_files_through_our_decoders(J, qctx, oracle, ri):
    """our own decoder on our own 4:2:2 file (the GPU Huffman decoder forced): 2 x 1 sampling reported, the oracle's pixels; the same
    file with smooth upsampling; and as one entry of a window batch beside a 4:2:0 file"""
    import torch
    W, H = 144, 33
    r, g, b = _rgb(W, H)
    qctx.set_quality(90)
    qctx.set_restart_interval(ri)
    jpg = qctx.encode_jpeg(r, g, b, W, H, sampling=J.SAMPLING_422)
    assert jpg == S2.write_jpeg(_want(W, H, "q90"), W, H, quant_tables=QM.tables("q90"), ri=ri)
    jpg420 = qctx.encode_jpeg(r, g, b, W, H)
    qctx.set_huffdec_min_bytes(0)
    info, dr, dg, db = qctx.decode_jpeg(jpg)
    assert qctx.last_huffdec_passes() > 0
    assert list(info.H)[:3] == [2, 1, 1] and list(info.V)[:3] == [1, 1, 1] and info.blocks_per_mcu == 4
    _, orr, og, ob = oracle.decode_jpeg(jpg)
    assert np.array_equal(dr, orr) and np.array_equal(dg, og) and np.array_equal(db, ob)
    _, sr, sg, sb = qctx.decode_jpeg(jpg, upsampling=J.UPSAMPLE_SMOOTH)
    import smooth_model as UM
    hinfo, co = J.read_jpeg(jpg)
    assert UM.factors(hinfo, 1) == (2, 1)                                             # the h2v1 form of the triangle filter
    for got, want in zip((sr, sg, sb), UM.decode_planes(co, hinfo)):
        assert np.array_equal(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1))
    assert not (np.array_equal(sr, dr) and np.array_equal(sg, dg) and np.array_equal(sb, db))   # the filter acted
    d_win = torch.full((2, H, W, 3), 0xA5, dtype=torch.uint8, device="cuda")
    res = qctx.decode_windows_dev([jpg, jpg420], d_win, [(8, 3, 100, 20), None])
    h_win = d_win.cpu().numpy()
    assert [st for _, _, st in res] == [0, 0]
    whole = np.stack([p.reshape(H, W) for p in (dr, dg, db)], axis=-1)
    x, y, w, h = res[0][1]
    assert (w, h) == (100, 20) and np.array_equal(h_win[0, :h, :w], whole[y:y + h, x:x + w])
    assert (h_win[0, h:] == 0xA5).all() and (h_win[0, :, w:] == 0xA5).all()
    _, r0, g0, b0 = oracle.decode_jpeg(jpg420)
    assert np.array_equal(h_win[1], np.stack([p.reshape(H, W) for p in (r0, g0, b0)], axis=-1))


# ---- the C++ interface ----
def test_cpp_encoder_encode_with_sampling_422(J, qctx, oracle, tmp_path):
    """encoder::encode(file, JPEZY_SAMPLING_422) through the header-only C++ interface (tests/encode422_main.cpp: the pipe syntax the CLI
    uses, with the value the CLI does not spell): the model's file, point-sampled and with the shared context set to average"""
    import subprocess
    from pathlib import Path
    from jpezy_amd import _build
    root = Path(_build.ROOT)
    exe = tmp_path / "encode422_main"
    build = subprocess.run([str(_build.HIPCC), "-std=c++17", "-O1", "-x", "c++", str(root / "tests" / "encode422_main.cpp"), "-I", str(root / "include"),
                            "-I", str(_build.CSRC / "host"), "-o", str(exe), "-L", str(_build.PKG), "-ljpezy_hip", f"-Wl,-rpath,{_build.PKG}",
                            "-lpthread"], capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stderr
    W, H = 144, 9
    r, g, b = _rgb(W, H)
    src = tmp_path / "in.ppm"
    src.write_bytes(oracle.format_ppm_p3(W, H, r, g, b))
    for mode, extra in ((S2.POINT, []), (S2.AVERAGE, ["average"])):
        out = tmp_path / f"out{mode}.jpg"
        p = subprocess.run([str(exe), str(src), str(out), *extra], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        assert out.read_bytes() == S2.write_jpeg(_want(W, H, "q50", mode=mode), W, H), mode


# ---- refusals ----
def test_refusals_leave_the_context_usable(J, qctx):
    import torch
    W, H = 144, 9
    r, g, b = _rgb(W, H)
    planes = [torch.from_numpy(p.copy()).cuda() for p in (r, g, b)]
    co = _out(torch, W, H)
    rgb = torch.from_numpy(np.ascontiguousarray(np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1))).cuda()
    qctx.set_variant(0)
    for call in (lambda: qctx.fdct_quant_dev(*planes, W, H, co, sampling=J.SAMPLING_422),
                 lambda: qctx.fdct_quant_packed_dev(rgb, co, sampling=J.SAMPLING_422),
                 lambda: qctx.encode_jpeg(r, g, b, W, H, sampling=J.SAMPLING_422)):
        with pytest.raises(J.JpezyError, match=f"status {UNSUPPORTED}.*JPEZY_SAMPLING_422"):
            call()
    assert np.array_equal(qctx.fdct_quant(r, g, b, W, H), QM.quantise(QM.synth_dct(W, H), *QM.tables("q50")))   # variant 0 still encodes 4:2:0
    qctx.set_variant(1)
    for bad in (lambda: qctx.fdct_quant_dev(*planes, W, H, co, gray=True, sampling=J.SAMPLING_422),
                lambda: qctx.fdct_quant_dev(*planes, W, H, co, sampling=2),
                lambda: qctx.fdct_quant_packed_dev(rgb, co, sampling=2),
                lambda: qctx.encode_jpeg(r, g, b, W, H, gray=True, sampling=J.SAMPLING_422),
                lambda: qctx.encode_jpeg(r, g, b, W, H, sampling=2),
                lambda: qctx.write_jpeg_gpu(co, W, H, sampling=2),
                lambda: qctx.huffman_histogram_dev(co, W, H, torch.zeros((1, 4, 256), dtype=torch.int64, device="cuda"), sampling=2)):
        with pytest.raises(J.JpezyError, match="status -1"):
            bad()
    qctx.fdct_quant_dev(*planes, W, H, co, sampling=J.SAMPLING_422)
    torch.cuda.synchronize()
    assert np.array_equal(co.cpu().numpy(), _want(W, H, "q50"))
    assert qctx.encode_jpeg(r, g, b, W, H) == J.write_jpeg(QM.quantise(QM.synth_dct(W, H), *QM.tables("q50")), W, H)   # and 4:2:0 as before


# ---- 4:2:0 and 4:4:4 unchanged ----
def test_the_other_two_samplings_return_their_models_bytes(J, qctx, oracle):
    """every *_sampling* entry with SAMPLING_420 and SAMPLING_444 against the models that define them (the oracle, tests/sampling_model.py,
    the host writer): the re-instantiated coder and histogram kernels and the generalised entry points changed nothing for them"""
    import torch
    W, H = 176, 64
    r, g, b = _rgb(W, H)
    planes = [torch.from_numpy(p.copy()).cuda() for p in (r, g, b)]
    rgbh = np.ascontiguousarray(np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1))
    rgb = torch.from_numpy(rgbh).cuda()
    models = {J.SAMPLING_420: np.asarray(oracle.encode_coeffs(r, g, b, W, H), np.int16),
              J.SAMPLING_444: SM.quantise(SM.synth_dct(W, H), *QM.tables("q50"))}
    for S, want in models.items():
        for call in (lambda co: qctx.fdct_quant_dev(*planes, W, H, co, sampling=S), lambda co: qctx.fdct_quant_packed_dev(rgb, co, sampling=S)):
            co = torch.full(want.shape, 0x5A5A, dtype=torch.int16, device="cuda")
            call(co)
            torch.cuda.synchronize()
            assert np.array_equal(co.cpu().numpy(), want), S
        stride = J.jpeg_bound(W, H, S)
        d_out = torch.zeros((1, stride), dtype=torch.uint8, device="cuda")
        d_sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
        d_hist = torch.zeros((1, 4, 256), dtype=torch.int64, device="cuda")
        for ri, opt in ((0, 0), (5, 0), (22, 1), (0, 1)):
            qctx.set_restart_interval(ri)
            qctx.set_huffman_optimize(opt)
            ref = oracle.write_jpeg(want, W, H) if S == J.SAMPLING_420 and not ri and not opt else \
                SM.write_jpeg(want, W, H, ri=ri, optimize=bool(opt)) if S == J.SAMPLING_444 else \
                J.write_jpeg(want, W, H, restart_interval=ri, optimize=bool(opt))
            assert J.write_jpeg(want, W, H, sampling=S, restart_interval=ri, optimize=bool(opt)) == ref, (S, ri, opt)
            assert qctx.write_jpeg_gpu(co, W, H, sampling=S)[0] == ref, (S, ri, opt)
            assert qctx.encode_jpeg(r, g, b, W, H, sampling=S) == ref and qctx.encode_jpeg_packed(rgbh, sampling=S) == ref, (S, ri, opt)
            qctx.huffman_histogram_dev(co, W, H, d_hist, sampling=S)
            torch.cuda.synchronize()
            assert np.array_equal(d_hist[0].cpu().numpy().astype(np.uint64), J.huffman_histogram(want, W, H, sampling=S, restart_interval=ri))
            if not opt:
                d_sizes.zero_()
                qctx.write_jpeg_gpu_dev(co, W, H, d_out, d_sizes, sampling=S)
                torch.cuda.synchronize()
                n = int(d_sizes[0])
                assert n == len(ref) and d_out[0, :n].cpu().numpy().tobytes() == ref, (S, ri, "dev")


# ---- streams and capture ----
TAIL = 64


def _frames(W, H, which):
    return [_rgb(W, H, f) for f in ((0, 1) if which == "A" else (2, 3))]


def _coeff_expect(frames, tail_elems=8):
    body = np.concatenate([np.asarray(f, np.int16).reshape(-1) for f in frames])
    return body.size + tail_elems, [(np.concatenate([body.view(np.uint8), SP.marker(2 * tail_elems)]), None)]


def _probe_transform(torch, J, ctx):
    W, H = 144, 9
    stride = W * H + 4
    planes, expect = {}, {}
    for k in "AB":
        fr = _frames(W, H, k)
        planes[k] = []
        for c in range(3):
            p = np.zeros(2 * stride, np.uint8)
            for f in range(2):
                p[f * stride:f * stride + W * H] = fr[f][c]
            planes[k].append(p)
        elems, expect[k] = _coeff_expect([S2.encode_coeffs(*f, W, H, *QM.tables("q50")) for f in fr])
    d = [torch.empty(2 * stride, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    d_co = torch.empty(elems, dtype=torch.int16, device="cuda:0")
    return SP.Probe(torch, "fdct_quant_dev SAMPLING_422", [(d[c], planes["A"][c], planes["B"][c]) for c in range(3)], [d_co],
                    lambda s: ctx.fdct_quant_dev(*d, W, H, d_co, n_frames=2, plane_stride=stride, stream=s, sampling=J.SAMPLING_422), expect)


def _probe_fields(W, H):
    return {k: [S2.encode_coeffs(*f, W, H, *QM.tables("q50")) for f in _frames(W, H, k)] for k in "AB"}


def _probe_write(torch, J, ctx):
    W, H = 144, 9
    stride = J.jpeg_bound(W, H, J.SAMPLING_422)
    co, expect = {}, {}
    for k, fr in _probe_fields(W, H).items():
        co[k] = np.stack([f.reshape(-1) for f in fr])
        want, mask = SP.marker(2 * stride + TAIL), np.zeros(2 * stride + TAIL, bool)
        mask[2 * stride:] = True
        lens = []
        for f in range(2):
            jpg = np.frombuffer(S2.write_jpeg(fr[f], W, H), np.uint8)
            assert jpg.size < stride
            want[f * stride:f * stride + jpg.size] = jpg
            mask[f * stride:f * stride + jpg.size] = True
            lens.append(jpg.size)
        sizes = np.concatenate([np.array(lens, np.int64).view(np.uint8), SP.marker(16)])
        expect[k] = [(want, mask), (sizes, None)]
    d_co = torch.empty(co["A"].shape, dtype=torch.int16, device="cuda:0")
    d_out = torch.empty(2 * stride + TAIL, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.empty(4, dtype=torch.int64, device="cuda:0")
    return SP.Probe(torch, "write_jpeg_gpu_dev SAMPLING_422", [(d_co, co["A"], co["B"])], [d_out, d_sizes],
                    lambda s: ctx.write_jpeg_gpu_dev(d_co, W, H, d_out[:2 * stride], d_sizes[:2], n_frames=2, stream=s, sampling=J.SAMPLING_422),
                    expect)


def _probe_histogram(torch, J, ctx):
    W, H = 144, 9
    co, expect = {}, {}
    for k, fr in _probe_fields(W, H).items():
        co[k] = np.stack([f.reshape(-1) for f in fr])
        counts = []
        for f in fr:
            h, ok = S2.symbol_counts(f)
            assert ok
            counts.append(h.astype(np.int64).reshape(-1))
        expect[k] = [(np.concatenate([np.concatenate(counts).view(np.uint8), SP.marker(32)]), None)]
    d_co = torch.empty(co["A"].shape, dtype=torch.int16, device="cuda:0")
    d_hist = torch.empty(2 * 1024 + 4, dtype=torch.int64, device="cuda:0")
    return SP.Probe(torch, "huffman_histogram_dev SAMPLING_422", [(d_co, co["A"], co["B"])], [d_hist],
                    lambda s: ctx.huffman_histogram_dev(d_co, W, H, d_hist[:2048].view(2, 4, 256), n_frames=2, stream=s, sampling=J.SAMPLING_422),
                    expect)


PROBES = {"transform": _probe_transform, "write": _probe_write, "histogram": _probe_histogram}


@pytest.fixture(scope="module")
def delay():
    import torch
    return SP.Delay(torch, "cuda:0")


@pytest.mark.parametrize("case", sorted(PROBES))
def test_dev_entries_follow_the_callers_stream(J, qctx, delay, case):
    import torch
    SP.stream_order(torch, delay, PROBES[case](torch, J, qctx))
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", sorted(PROBES))
def test_dev_entries_replay_from_a_captured_graph(J, qctx, case):
    """one call captured on a side stream (one stream, no branches), replayed on A, B, A: every replay equals the models' bytes, which
    the eager warm call is compared with first"""
    import torch
    SP.capture_replay(torch, PROBES[case](torch, J, qctx))
    torch.cuda.synchronize()
