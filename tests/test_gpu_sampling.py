"""4:4:4 chroma sampling on the GPU (include/jpezy_hip.h, CHROMA SAMPLING): the transform kernel against
tests/sampling_model.py for equality -- planar, RGB24 and BGRA32 with a padded row stride, every force_exact level, every table set, the
DC from the exact table --, the rare paths on a picture whose pixels sit on the colour guard bands, the queue overflow on a picture built for it, a batch with a padded frame stride,
the end-to-end entries against the host writer, the files through our own GPU Huffman decoder, the refusals, SAMPLING_420 against the
entries it stands for, and the GPU entropy coder on 3-block MCUs (tile seams inside an MCU, restart intervals, per-image tables, batch,
the device-resident form, the histogram kernel) against the host writer.

Shapes (the work unit is the OCTET: 8 horizontally adjacent 8 x 8 MCUs per wave, four waves per workgroup): 8 x 8 (one MCU, seven dead
MCU slots), 64 x 8 (one full octet), 72 x 24 (a partial last octet, three MCU rows), 33 x 17 (odd edges, clamp, the byte-loop path),
128 x 16 and 256 x 8 (the 8-byte load path; 256 x 8 is one workgroup of four live waves)."""
from functools import lru_cache

import numpy as np
import pytest

from exact_picture import EXACT_F, QUEUE_CAP, exact_picture
import quant_model as QM
import sampling_model as SM

pytestmark = pytest.mark.gpu

TABLES = ["q1", "q50", "q90", "q100", "random", "ones_dc255", "255_dc1"]
OTHER_SHAPES = [(8, 8), (64, 8), (33, 17), (128, 16), (256, 8)]
FEW = ["q50", "q100", "random"]
UNSUPPORTED = -4


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
def qctx(ctx):
    """the module's context, handed back at its defaults"""
    yield ctx
    ctx.set_quant_tables(None, None)
    ctx.set_variant(1)
    ctx.set_force_exact(0)
    ctx.set_dc_table_lookup(0)
    ctx.set_huffman_optimize(0)
    ctx.set_restart_interval(0)
    ctx.set_huffdec_min_bytes(32 << 10)


@lru_cache(maxsize=None)
def _rgb(W, H, frame=0):
    from oracle import oracle as O
    return O.synth_rgb(W, H, frame=frame)


def _want(W, H, name, frame=0):
    return SM.quantise(SM.synth_dct(W, H, frame), *QM.tables(name))


def _shape(W, H):
    mc, mr, _ = SM.geometry(W, H)
    return (mr, mc, 3, 64)


def _dev_entries(J, ctx, r, g, b, W, H):
    """fdct_quant_dev (planar), fdct_quant_packed_dev RGB24 (tight) and BGRA32 (row stride padded by 16 bytes) with sampling=444"""
    import torch
    S = J.SAMPLING_444
    out = []
    planes = [torch.from_numpy(np.asarray(p).copy()).cuda() for p in (r, g, b)]
    co = torch.full(_shape(W, H), 0x5A5A, dtype=torch.int16, device="cuda")
    ctx.fdct_quant_dev(*planes, W, H, co, sampling=S)
    out.append(("planar", co))
    rgb = np.stack([np.asarray(p).reshape(H, W) for p in (r, g, b)], axis=-1)
    co = torch.full(_shape(W, H), 0x5A5A, dtype=torch.int16, device="cuda")
    ctx.fdct_quant_packed_dev(torch.from_numpy(np.ascontiguousarray(rgb)).cuda(), co, format=J.PIX_RGB24, sampling=S)
    out.append(("RGB24", co))
    bgra = np.full((H, W + 4, 4), 7, np.uint8)                   # 16 bytes of padding behind every row
    bgra[:, :W, :3] = rgb[..., ::-1]
    d = torch.from_numpy(bgra).cuda()
    co = torch.full(_shape(W, H), 0x5A5A, dtype=torch.int16, device="cuda")
    ctx.fdct_quant_packed_dev(d[:, :W], co, format=J.PIX_BGRA32, sampling=S)
    out.append(("BGRA32 padded", co))
    torch.cuda.synchronize()
    return [(n, c.cpu().numpy()) for n, c in out]


def _check_every_entry(J, ctx, r, g, b, W, H, want, tag):
    for entry, co in _dev_entries(J, ctx, r, g, b, W, H):
        bad = np.argwhere(co != want)
        assert bad.size == 0, (entry, tag, len(bad), bad[:4].tolist())


# ---- coefficients ----
@pytest.mark.parametrize("name", TABLES)
def test_coefficients_equal_the_model_on_the_full_cross(J, qctx, name):
    """72 x 24: every table set x force_exact {0, 1, 2, 3}, every entry; and once more with the DC read from the exact table"""
    W, H = 72, 24
    qctx.set_quant_tables(*QM.tables(name))
    want = _want(W, H, name)
    for fe in (0, 1, 2, 3):
        qctx.set_force_exact(fe)
        qctx.fallback_count()
        _check_every_entry(J, qctx, *_rgb(W, H), W, H, want, (name, fe))
        n = qctx.fallback_count()
        if fe:
            assert n >= want.size, (name, fe, n)          # the test hooks send every coefficient down the exact paths
    qctx.set_force_exact(0)
    qctx.set_dc_table_lookup(1)
    _check_every_entry(J, qctx, *_rgb(W, H), W, H, want, (name, "dc table"))


@pytest.mark.parametrize("W,H", OTHER_SHAPES)
@pytest.mark.parametrize("name", FEW)
def test_coefficients_equal_the_model_on_the_other_shapes(J, qctx, name, W, H):
    qctx.set_quant_tables(*QM.tables(name))
    want = _want(W, H, name)
    for fe in (0, 3) if name == "q100" else (0,):
        qctx.set_force_exact(fe)
        _check_every_entry(J, qctx, *_rgb(W, H), W, H, want, (name, fe))


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


def test_rare_paths_on_guard_band_pixels(J, qctx):
    """72 x 24 built from such triples only: the colour votes fire in every wave; at quality 100 (every quantiser 1: the widest level-1
    bands, no zero coefficients) levels 2 and 3 run as well.  Equality with the model at force_exact 0 is then a statement about those
    paths; the counter shows they ran."""
    W, H = 72, 24
    T = _guard_band_triples()
    assert min(len(v) for v in T.values()) >= 100
    rng = np.random.default_rng(444)
    pix = np.array([T[k][i] for k, i in zip(rng.choice(["y", "cb", "cr"], W * H), rng.integers(0, 100, W * H))], np.uint8)
    r, g, b = (np.ascontiguousarray(pix[:, k]) for k in range(3))
    rf, gf, bf = (p.astype(np.int64) for p in (r, g, b))
    on_band = ((299 * rf + 587 * gf + 114 * bf) % 1000 == 0) | ((-1687 * rf - 3313 * gf + 5000 * bf) % 10000 == 0) | \
              ((5000 * rf - 4187 * gf - 813 * bf) % 10000 == 0)
    assert on_band.all()
    dct = SM.dct_from_rgb(r, g, b, W, H)
    for name in ("q100", "q50"):
        qctx.set_quant_tables(*QM.tables(name))
        want = SM.quantise(dct, *QM.tables(name))
        qctx.fallback_count()
        _check_every_entry(J, qctx, r, g, b, W, H, want, ("guard band", name))
        if name == "q100":
            assert qctx.fallback_count() > 0


# ---- the queue overflow, for certain ----
def test_queue_overflow_without_the_force_hook(J, qctx):
    """128 x 16 (four whole octets) at force_exact 0 and quality 100, tests/exact_picture.py with a chroma sample per pixel: every block
    has 23 AC coefficients exactly on an integer -- each one on a truncation boundary at Q = 1, flagged by level 1 and queued --, 552 of an
    octet's 1536 coefficients against a queue of 382: the queue overflows and the per-lane evaluator of the shipped instances (8-byte
    loads, packed, and the byte loop through planes that start one byte into their allocations) runs without the hook.  Equality with
    the model; the counter shows that every coefficient of every octet went through the evaluator."""
    import torch
    W, H, OCTET_COEFFS = 128, 16, 1536                                     # 24 blocks of a 4:4:4 octet
    r, g, b, (Y, Cb, Cr) = exact_picture(W, H, 1)
    ys, cbs, crs = SM.samples_from_rgb(r, g, b, W, H)
    assert np.array_equal(ys, Y) and np.array_equal(cbs, Cb) and np.array_equal(crs, Cr)      # the samples ARE the pattern
    dct = SM.dct_from_rgb(r, g, b, W, H)
    hits = np.count_nonzero(np.array(EXACT_F)) * 24
    assert hits > QUEUE_CAP and (np.count_nonzero(dct.reshape(-1, 64)[:, 1:], axis=1) == 23).all()
    qctx.set_quant_tables(*QM.tables("q100"))
    want = SM.quantise(dct, *QM.tables("q100"))
    qctx.fallback_count()
    entries = _dev_entries(J, qctx, r, g, b, W, H)
    shifted = []
    for p in (r, g, b):
        buf = torch.full((W * H + 1,), 0xEE, dtype=torch.uint8, device="cuda")
        buf[1:] = torch.from_numpy(p.copy()).cuda()
        shifted.append(buf[1:])
    co = torch.full(_shape(W, H), 0x5A5A, dtype=torch.int16, device="cuda")
    qctx.fdct_quant_dev(*shifted, W, H, co, sampling=J.SAMPLING_444)
    torch.cuda.synchronize()
    entries.append(("planar base + 1", co.cpu().numpy()))
    assert qctx.fallback_count() == len(entries) * 4 * OCTET_COEFFS        # four octets a call, each one whole through the evaluator
    for entry, got in entries:
        bad = np.argwhere(got != want)
        assert bad.size == 0, (entry, len(bad), bad[:4].tolist())


# ---- batch ----
def test_batch_with_padded_frame_stride(J, qctx):
    import torch
    W, H, F = 72, 24, 3
    stride = W * H + 40                                   # a multiple of 8: the 8-byte load path, frames apart by more than a plane
    planes = []
    for k in range(3):
        buf = np.full(F * stride, 0xEE, np.uint8)
        for f in range(F):
            buf[f * stride:f * stride + W * H] = _rgb(W, H, f)[k]
        planes.append(torch.from_numpy(buf).cuda())
    co = torch.zeros((F,) + _shape(W, H), dtype=torch.int16, device="cuda")
    qctx.fdct_quant_dev(*planes, W, H, co, n_frames=F, plane_stride=stride, sampling=J.SAMPLING_444)
    torch.cuda.synchronize()
    got = co.cpu().numpy()
    for f in range(F):
        assert np.array_equal(got[f], _want(W, H, "q50", f)), f


# ---- end to end ----
@pytest.mark.parametrize("W,H", [(72, 24), (176, 64)])
def test_encode_jpeg_equals_host_writer_of_model_coefficients(J, qctx, W, H):
    r, g, b = _rgb(W, H)
    rgb = np.ascontiguousarray(np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1))
    for name, opt, ri in (("q50", 0, 0), ("q90", 1, 5), ("q100", 0, 22), ("random", 1, 0)):
        tabs = QM.tables(name)
        qctx.set_quant_tables(*tabs)
        qctx.set_huffman_optimize(opt)
        qctx.set_restart_interval(ri)
        ref = J.write_jpeg(_want(W, H, name), W, H, sampling=J.SAMPLING_444, optimize=bool(opt), restart_interval=ri, quant_tables=tabs)
        assert qctx.encode_jpeg(r, g, b, W, H, sampling=J.SAMPLING_444) == ref, (name, opt, ri)
        assert qctx.encode_jpeg_packed(rgb, sampling=J.SAMPLING_444) == ref, ("packed", name, opt, ri)
        if name == "q50" or W == 72:
            assert ref == SM.write_jpeg(_want(W, H, name), W, H, quant_tables=tabs, ri=ri, optimize=bool(opt))


@pytest.mark.parametrize("ri", [0, 5])
def test_files_through_the_gpu_huffman_decoder(J, qctx, oracle, ri):
    """our own decoder on our own 4:4:4 files, the GPU Huffman decoder forced: 1 x 1 sampling reported, the pixels of read_jpeg +
    dequant_idct_generic, which are the oracle's"""
    W, H = 176, 64
    r, g, b = _rgb(W, H)
    qctx.set_quality(90)
    qctx.set_restart_interval(ri)
    jpg = qctx.encode_jpeg(r, g, b, W, H, sampling=J.SAMPLING_444)
    qctx.set_huffdec_min_bytes(0)
    info, dr, dg, db = qctx.decode_jpeg(jpg)
    assert qctx.last_huffdec_passes() > 0
    assert list(info.H) == [1, 1, 1] and list(info.V) == [1, 1, 1] and info.blocks_per_mcu == 3
    hinfo, co = J.read_jpeg(jpg)
    assert np.array_equal(co, _want(W, H, "q90"))
    for got, want in zip((dr, dg, db), qctx.dequant_idct_generic(co, hinfo)):
        assert np.array_equal(got, want)
    _, orr, og, ob = oracle.decode_jpeg(jpg)
    assert np.array_equal(dr, orr) and np.array_equal(dg, og) and np.array_equal(db, ob)


# the model's figures for the picture below at quality 100 (sampling_model / quant_model coefficients, the model's file, the oracle's
# decoder; worked out once, asserted again here): largest channel error of the 4:4:4 file and of the 4:2:0 file
CHECKER_MAX_ERR_444, CHECKER_MAX_ERR_420 = 4, 164


def test_chroma_checkerboard_at_quality_100(J, qctx, oracle):
    """72 x 24, pixels alternating (200, 60, 60) / (60, 60, 200): 4:2:0 keeps the chroma of one pixel in four, so half the pixels come
    back with the other colour's chroma; 4:4:4 at quality 100 loses only the truncations"""
    W, H = 72, 24
    yy, xx = np.mgrid[0:H, 0:W]
    a = ((xx + yy) & 1).astype(bool)
    r = np.where(a, 200, 60).astype(np.uint8).reshape(-1)
    g = np.full(W * H, 60, np.uint8)
    b = np.where(a, 60, 200).astype(np.uint8).reshape(-1)
    src = np.stack([r, g, b]).astype(np.int64)
    ones = np.ones(64, np.uint8)
    err = lambda planes: int(np.abs(np.stack(planes).astype(np.int64) - src).max())
    m444 = SM.write_jpeg(SM.encode_coeffs(r, g, b, W, H, ones, ones), W, H, quant_tables=(ones, ones))
    m420 = J.write_jpeg(QM.encode_coeffs(r, g, b, W, H, ones, ones), W, H, quant_tables=(ones, ones))
    assert err(oracle.decode_jpeg(m444)[1:]) == CHECKER_MAX_ERR_444 and err(oracle.decode_jpeg(m420)[1:]) == CHECKER_MAX_ERR_420
    qctx.set_quality(100)
    f444 = qctx.encode_jpeg(r, g, b, W, H, sampling=J.SAMPLING_444)
    f420 = qctx.encode_jpeg(r, g, b, W, H)
    assert f444 == m444 and f420 == m420
    e444, e420 = err(qctx.decode_jpeg(f444)[1:]), err(qctx.decode_jpeg(f420)[1:])
    assert e444 == CHECKER_MAX_ERR_444 and e420 == CHECKER_MAX_ERR_420
    assert e444 <= e420 and e420 >= 10 * e444                 # no worse, and the 4:2:0 file visibly so


# ---- refusals ----
def test_refusals_leave_the_context_usable(J, qctx):
    import torch
    W, H = 72, 24
    r, g, b = _rgb(W, H)
    planes = [torch.from_numpy(p.copy()).cuda() for p in (r, g, b)]
    co = torch.zeros(_shape(W, H), dtype=torch.int16, device="cuda")
    qctx.set_variant(0)
    for call in (lambda: qctx.fdct_quant_dev(*planes, W, H, co, sampling=J.SAMPLING_444),
                 lambda: qctx.encode_jpeg(r, g, b, W, H, sampling=J.SAMPLING_444)):
        with pytest.raises(J.JpezyError, match=f"status {UNSUPPORTED}"):
            call()
    assert np.array_equal(qctx.fdct_quant(r, g, b, W, H), QM.quantise(QM.synth_dct(W, H), *QM.tables("q50")))   # variant 0 still encodes 4:2:0
    qctx.set_variant(1)
    for bad in (lambda: qctx.fdct_quant_dev(*planes, W, H, co, gray=True, sampling=J.SAMPLING_444),
                lambda: qctx.fdct_quant_dev(*planes, W, H, co, sampling=2),
                lambda: qctx.encode_jpeg(r, g, b, W, H, gray=True, sampling=J.SAMPLING_444),
                lambda: qctx.encode_jpeg(r, g, b, W, H, sampling=-1)):
        with pytest.raises(J.JpezyError, match="status -1"):
            bad()
    qctx.fdct_quant_dev(*planes, W, H, co, sampling=J.SAMPLING_444)
    torch.cuda.synchronize()
    assert np.array_equal(co.cpu().numpy(), _want(W, H, "q50"))


# ---- 4:2:0 unchanged ----
def test_sampling_420_entries_are_their_old_twins(J, qctx):
    import ctypes as C
    import torch
    lib = J.load_library()
    W, H = 80, 48
    r, g, b = _rgb(W, H)
    planes = [torch.from_numpy(p.copy()).cuda() for p in (r, g, b)]
    old = torch.zeros((3, 5, 6, 64), dtype=torch.int16, device="cuda")
    new = torch.zeros_like(old)
    s = torch.cuda.current_stream().cuda_stream
    qctx.fdct_quant_dev(*planes, W, H, old)
    assert lib.jpezy_fdct_quant_sampling_dev(qctx._h, *(p.data_ptr() for p in planes), W * H, W, H, 0, 0, 1, new.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(old, new) and np.array_equal(old.cpu().numpy(), QM.quantise(QM.synth_dct(W, H), *QM.tables("q50")))
    rgb = torch.from_numpy(np.ascontiguousarray(np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1))).cuda()
    new.zero_()
    assert lib.jpezy_fdct_quant_sampling_packed_dev(qctx._h, rgb.data_ptr(), 0, W * 3, 0, W, H, 0, 0, 1, new.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(old, new)
    ref = qctx.encode_jpeg(r, g, b, W, H)
    cap = J.jpeg_bound(W, H)
    buf = np.zeros(cap, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = lib.jpezy_encode_jpeg_sampling(qctx._h, p(r), p(g), p(b), W, H, 0, 0, b"Encoded by jpezy", p(buf), cap)
    assert n == len(ref) and buf[:n].tobytes() == ref
    rgbh = rgb.cpu().numpy()
    n = lib.jpezy_encode_jpeg_sampling_packed(qctx._h, p(rgbh), 0, W * 3, W, H, 0, 0, b"Encoded by jpezy", p(buf), cap)
    assert n == len(ref) and buf[:n].tobytes() == ref
    n = lib.jpezy_write_jpeg_gpu_sampling(qctx._h, old.data_ptr(), W, H, 0, 0, b"Encoded by jpezy", p(buf), cap)
    assert n == len(ref) and buf[:n].tobytes() == ref
    d_hist = torch.zeros((2, 4, 256), dtype=torch.int64, device="cuda")
    qctx.huffman_histogram_dev(old, W, H, d_hist[0:1])
    assert lib.jpezy_huffman_histogram_sampling_dev(qctx._h, old.data_ptr(), W, H, 0, 0, 1, d_hist[1].data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(d_hist[0], d_hist[1]) and int(d_hist[0].sum()) > 0
    # gray through the 4:2:0 value is the old gray entry too
    n = lib.jpezy_encode_jpeg_sampling(qctx._h, p(r), p(g), p(b), W, H, 0, 1, b"Encoded by JPEZY", p(buf), cap)
    assert buf[:n].tobytes() == qctx.encode_jpeg(r, g, b, W, H, gray=True)


# ---- the entropy coder on 3-block MCUs ----
SEAM_W, SEAM_H = 176, 64          # 22 x 8 = 176 MCUs = 528 blocks = three tiles of 256: the seams fall inside MCU 85 and MCU 170
SEAM_RESTARTS = [0, 1, 5, 22, 85, 86, 176, 177]


@lru_cache(maxsize=None)
def _seam_fields():
    """coefficient fields [176, 3, 64], read-only: dense small values; sparse with values up to +-1023 and DC steps of category 11; zeros"""
    rng = np.random.default_rng(20261019)
    n = 176
    dense = rng.integers(-12, 13, (n, 3, 64)).astype(np.int16)
    large = np.where(rng.random((n, 3, 64)) < 0.25, rng.integers(-1023, 1024, (n, 3, 64)), 0).astype(np.int16)
    large[:, :, 0] = np.where(np.arange(n) % 2 == 0, 1000, -1000)[:, None]
    large[84:87] = rng.integers(-1023, 1024, (3, 3, 64))           # the MCUs around the first seam: full blocks (1400 bits and more)
    large[84:87, :, 0] = rng.integers(-20, 21, (3, 3))
    zeros = np.zeros((n, 3, 64), np.int16)
    out = {"dense": dense, "large": large, "zeros": zeros}
    for a in out.values():
        a.setflags(write=False)
    return out


def test_seam_geometry_is_what_the_cases_assume(J):
    assert J.sampling_geometry(J.SAMPLING_444, SEAM_W, SEAM_H) == (22, 8, 3)
    assert 85 * 3 < 256 < 86 * 3 and 170 * 3 < 512 < 171 * 3 and 176 * 3 > 512


@pytest.mark.parametrize("field", ["dense", "large", "zeros"])
@pytest.mark.parametrize("name", ["annex_k", "q100"])
def test_gpu_writer_equals_host_writer_across_tile_seams(J, qctx, field, name):
    """restart interval x optimise, the synchronous form, the device-resident form (optimise off) and the histogram kernel"""
    import torch
    W, H = SEAM_W, SEAM_H
    co = _seam_fields()[field]
    tabs = None if name == "annex_k" else QM.tables(name)
    qctx.set_quant_tables(*(tabs or (None, None)))
    d_co = torch.from_numpy(co.copy()).cuda()
    stride = J.jpeg_bound(W, H, J.SAMPLING_444)
    d_out = torch.zeros((1, stride), dtype=torch.uint8, device="cuda")
    d_sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
    d_hist = torch.zeros((1, 4, 256), dtype=torch.int64, device="cuda")
    for ri in SEAM_RESTARTS:
        qctx.set_restart_interval(ri)
        qctx.huffman_histogram_dev(d_co, W, H, d_hist, sampling=J.SAMPLING_444)
        torch.cuda.synchronize()
        want_hist = J.huffman_histogram(co, W, H, sampling=J.SAMPLING_444, restart_interval=ri)
        assert np.array_equal(d_hist[0].cpu().numpy().astype(np.uint64), want_hist), (field, ri)
        for opt in (0, 1):
            qctx.set_huffman_optimize(opt)
            ref = J.write_jpeg(co, W, H, sampling=J.SAMPLING_444, optimize=bool(opt), restart_interval=ri, quant_tables=tabs)
            got = qctx.write_jpeg_gpu(d_co, W, H, sampling=J.SAMPLING_444)[0]
            assert got == ref, (field, name, ri, opt, len(got), len(ref))
        qctx.set_huffman_optimize(0)
        d_out.zero_(); d_sizes.zero_()
        qctx.write_jpeg_gpu_dev(d_co, W, H, d_out, d_sizes, sampling=J.SAMPLING_444)
        torch.cuda.synchronize()
        n = int(d_sizes[0])
        ref0 = J.write_jpeg(co, W, H, sampling=J.SAMPLING_444, restart_interval=ri, quant_tables=tabs)
        assert n == len(ref0) and d_out[0, :n].cpu().numpy().tobytes() == ref0, (field, name, ri, "dev")
    if field == "dense" and name == "annex_k":          # the model itself, once per seam case
        for ri in (0, 85, 86):
            assert J.write_jpeg(co, W, H, sampling=J.SAMPLING_444, restart_interval=ri) == SM.write_jpeg(co.reshape(8, 22, 3, 64), W, H, ri=ri)


def test_gpu_writer_batch_and_a_frame_outside_the_code_tables(J, qctx):
    """three frames in one call; frame 1 holds a value of size 11: JPEZY_E_FORMAT (-5) for that frame only, in both forms; the device
    form refuses per-image tables"""
    import torch
    W, H = SEAM_W, SEAM_H
    F = _seam_fields()
    frames = np.stack([F["dense"], F["large"], F["dense"][::-1]]).copy()
    stride = J.jpeg_bound(W, H, J.SAMPLING_444)
    for ri in (0, 86):
        qctx.set_restart_interval(ri)
        for bad in (False, True):
            fr = frames.copy()
            if bad:
                fr[1, 85, 1, 7] = 1024
            refs = [J.write_jpeg(fr[f], W, H, sampling=J.SAMPLING_444, restart_interval=ri) if not (bad and f == 1) else -5 for f in range(3)]
            d_co = torch.from_numpy(fr).cuda()
            got = qctx.write_jpeg_gpu(d_co, W, H, n_frames=3, sampling=J.SAMPLING_444, raise_on_error=False)
            assert got == refs, (ri, bad)
            if bad:
                with pytest.raises(J.JpezyError, match="status -5"):
                    qctx.write_jpeg_gpu(d_co, W, H, n_frames=3, sampling=J.SAMPLING_444)
            d_out = torch.zeros((3, stride), dtype=torch.uint8, device="cuda")
            d_sizes = torch.zeros(3, dtype=torch.int64, device="cuda")
            qctx.write_jpeg_gpu_dev(d_co, W, H, d_out, d_sizes, n_frames=3, sampling=J.SAMPLING_444)
            torch.cuda.synchronize()
            sizes = d_sizes.cpu().tolist()
            for f in range(3):
                if isinstance(refs[f], int):
                    assert sizes[f] == refs[f], (ri, f)
                else:
                    assert sizes[f] == len(refs[f]) and d_out[f, :sizes[f]].cpu().numpy().tobytes() == refs[f], (ri, bad, f)
    qctx.set_huffman_optimize(1)
    with pytest.raises(J.JpezyError, match=f"status {UNSUPPORTED}"):
        qctx.write_jpeg_gpu_dev(d_co, W, H, d_out, d_sizes, n_frames=3, sampling=J.SAMPLING_444)
    with pytest.raises(J.JpezyError, match="status -1"):
        qctx.write_jpeg_gpu(d_co, W, H, gray=True, sampling=J.SAMPLING_444)


def test_gpu_writer_on_a_frame_of_more_than_2048_tiles(J, qctx):
    """3360 x 3360: 176400 MCUs = 529200 blocks = 2068 tiles -- past the size up to which the assembling kernel scans the tile totals
    itself (4:4:4 reaches it at a quarter of the pixels 4:2:0 needs).  A flat field (14 bits per MCU: the most tiles a piece of the
    stream can touch) and a sparse one, without and with restart intervals"""
    import torch
    W = H = 3360
    n = 420 * 420
    rng = np.random.default_rng(3360)
    sparse = np.zeros((n, 3, 64), np.int16)
    idx = rng.integers(0, n, 20000)
    sparse[idx, rng.integers(0, 3, 20000), rng.integers(0, 64, 20000)] = rng.integers(-300, 301, 20000)
    for field in (np.zeros((n, 3, 64), np.int16), sparse):
        d_co = torch.from_numpy(field).cuda()
        for ri in (0, 420):
            qctx.set_restart_interval(ri)
            got = qctx.write_jpeg_gpu(d_co, W, H, sampling=J.SAMPLING_444)[0]
            assert got == J.write_jpeg(field, W, H, sampling=J.SAMPLING_444, restart_interval=ri), ri


# ---- CLI ----
def test_cli_sampling_flag(J, oracle, tmp_path):
    """jpezy_encode in.ppm out.jpg --sampling=444 beside --optimize, --restart=N and --quality=N, the token anywhere behind the output
    name; --sampling=420 is the file without the flag; --gpus 1 takes it too (encoder::encode's sampling argument underneath)"""
    import subprocess
    from pathlib import Path
    from jpezy_amd import _build
    _build.build_all()
    enc = Path(_build.BIN) / "jpezy_encode"
    W, H = 72, 24
    r, g, b = _rgb(W, H)
    src = tmp_path / "in.ppm"
    src.write_bytes(oracle.format_ppm_p3(W, H, r, g, b))
    run = lambda *a: subprocess.run([str(x) for x in a], capture_output=True, text=True, timeout=120)
    out = tmp_path / "a.jpg"
    for flags, q, opt, ri in ((["--sampling=444"], 50, False, 0), (["--quality=90", "--sampling=444"], 90, False, 0),
                              (["--optimize", "--sampling=444", "--restart=5", "--quality=100"], 100, True, 5)):
        p = run(enc, src, out, *flags)
        assert p.returncode == 0, (flags, p.stderr)
        want = J.write_jpeg(_want(W, H, f"q{q}"), W, H, sampling=J.SAMPLING_444, optimize=opt, restart_interval=ri, quant_tables=QM.tables(f"q{q}"))
        assert out.read_bytes() == want, flags
        assert f"Output size: {len(want)} byte" in p.stdout
    p = run(enc, src, out, "--sampling=420")
    assert p.returncode == 0 and out.read_bytes() == oracle.encode_jpeg(r, g, b, W, H)
    p = run(enc, "--gpus", 1, "--sampling=444", src, out)
    assert p.returncode == 0, p.stderr
    assert out.read_bytes() == J.write_jpeg(_want(W, H, "q50"), W, H, sampling=J.SAMPLING_444)
