"""Quality 1..100 and caller-supplied quantisation tables on the GPU (jpezy_ctx_set_quality / jpezy_ctx_set_quant_tables; DESIGN.md
4.10): every encode entry point against tests/quant_model.py -- the reference's MCU loop with quantization(cs) dividing by the caller's
table -- for equality, at every table set, both encode variants and every force_exact level; the DC at its boundaries through the
level-1 quantiser and through the exact table; the value-range extremes at Q = 1; the files against the host writer with tables; the
default setting byte for byte; the rules of the setter; our own decoder on our own files.

Shapes: the smallest at which the quad kernel can go wrong -- 16 x 16 (one MCU, three dead lanes' worth), 64 x 16 (one full quad),
80 x 48 (a partial last quad, three rows), 33 x 17 (odd edges, clamp)."""
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import quant_model as QM
import ycc_model as YM

pytestmark = pytest.mark.gpu

TABLES = ["q1", "q25", "q50", "q75", "q90", "q100", "random", "ones_dc255", "255_dc1"]
OTHER_SHAPES = [(16, 16), (64, 16), (33, 17)]
FEW = ["q1", "q90", "q100", "random"]


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


@lru_cache(maxsize=None)
def _rgb(W, H):
    from oracle import oracle as O
    return O.synth_rgb(W, H)


def _want(W, H, gray, name):
    return QM.quantise(QM.synth_dct(W, H, gray), *QM.tables(name))


@lru_cache(maxsize=None)
def _ycc_dct(W, H, gray):
    y, cb, cr = YM.synth_planes(W, H, "random")
    d = QM.dct_from_ycc(y, cb, cr, gray)
    d.setflags(write=False)
    return d


def _dev_entries(ctx, W, H, gray):
    """fdct_quant_dev, fdct_quant_packed_dev (RGB24 and BGRA32) and fdct_quant_ycc_dev on the shared pictures:
    -> [(entry name, 'rgb' | 'ycc', coefficients)]"""
    import torch
    r, g, b = _rgb(W, H)
    mc, mr = (W + 15) // 16, (H + 15) // 16
    shape = (mr, mc, 4 if gray else 6, 64)
    out = []
    planes = [torch.from_numpy(p.copy()).cuda() for p in (r, g, b)]
    co = torch.zeros(shape, dtype=torch.int16, device="cuda")
    ctx.fdct_quant_dev(*planes, W, H, co, gray=gray)
    out.append(("fdct_quant_dev", "rgb", co))
    rgb = np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1)
    co = torch.zeros(shape, dtype=torch.int16, device="cuda")
    ctx.fdct_quant_packed_dev(torch.from_numpy(np.ascontiguousarray(rgb)).cuda(), co, format=0, gray=gray)
    out.append(("fdct_quant_packed_dev RGB24", "rgb", co))
    bgra = np.concatenate([rgb[..., ::-1], np.full((H, W, 1), 7, np.uint8)], axis=-1)
    co = torch.zeros(shape, dtype=torch.int16, device="cuda")
    ctx.fdct_quant_packed_dev(torch.from_numpy(np.ascontiguousarray(bgra)).cuda(), co, format=3, gray=gray)
    out.append(("fdct_quant_packed_dev BGRA32", "rgb", co))
    y, cb, cr = (torch.from_numpy(p.copy()).cuda() for p in YM.synth_planes(W, H, "random"))
    co = torch.zeros(shape, dtype=torch.int16, device="cuda")
    ctx.fdct_quant_ycc_dev(y, cb, cr, co, gray=gray)
    out.append(("fdct_quant_ycc_dev", "ycc", co))
    torch.cuda.synchronize()
    return [(n, k, c.cpu().numpy()) for n, k, c in out]


def _check_every_entry(ctx, W, H, gray, name, tag):
    luma, chroma = QM.tables(name)
    want = {"rgb": _want(W, H, gray, name), "ycc": QM.quantise(_ycc_dct(W, H, gray), luma, chroma)}
    r, g, b = _rgb(W, H)
    got = ctx.fdct_quant(r, g, b, W, H, gray=gray)
    assert np.array_equal(got, want["rgb"]), ("fdct_quant", name, tag)
    for entry, kind, co in _dev_entries(ctx, W, H, gray):
        assert np.array_equal(co, want[kind]), (entry, name, tag)


# ---- coefficients ----
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("name", TABLES)
def test_coefficients_equal_the_model_on_the_full_cross(qctx, name, gray):
    """80 x 48: every table set x {colour, gray} x variant {0, 1} x force_exact {0, 1, 2, 3} (levels 2 and 3 exist in variant 1 only),
    every entry point; and once more with the DC read from the exact table"""
    W, H = 80, 48
    qctx.set_quant_tables(*QM.tables(name))
    got = qctx.quant_tables()
    assert all(np.array_equal(a, b) for a, b in zip(got, QM.tables(name)))
    for variant, levels in ((0, (0, 1)), (1, (0, 1, 2, 3))):
        qctx.set_variant(variant)
        for fe in levels:
            qctx.set_force_exact(fe)
            _check_every_entry(qctx, W, H, gray, name, (variant, fe))
    qctx.set_force_exact(0)
    qctx.set_dc_table_lookup(1)
    _check_every_entry(qctx, W, H, gray, name, "dc table")


@pytest.mark.parametrize("W,H", OTHER_SHAPES)
@pytest.mark.parametrize("name", FEW)
def test_coefficients_equal_the_model_on_the_other_shapes(qctx, name, W, H):
    qctx.set_quant_tables(*QM.tables(name))
    for variant in (0, 1):
        qctx.set_variant(variant)
        for gray in (False, True):
            _check_every_entry(qctx, W, H, gray, name, variant)


# ---- the DC at its boundaries ----
@lru_cache(maxsize=None)
def _grey_tiles():
    """256 x 256: 16 x 16 flat tiles, one per grey level 0..255; its unquantised DCT; the luma block sum of every level"""
    lv = np.arange(256, dtype=np.uint8).reshape(16, 16)
    p = np.repeat(np.repeat(lv, 16, axis=0), 16, axis=1).reshape(-1)
    d = QM.dct_from_rgb(p, p, p, 256, 256)
    d.setflags(write=False)
    f = np.arange(256, dtype=np.float64)
    sums = 64 * np.trunc((0.2990 * f) + (0.5870 * f) + (0.1140 * f) - 128).astype(np.int64)
    return p, d, sums


@pytest.mark.parametrize("name", ["q100", "q50", "ones_dc255"])
def test_dc_boundaries_through_the_quantiser_and_through_the_table(qctx, name):
    """flat blocks: the block sum is 64 (Y - 128).  At quality 100 every sum is a multiple of 8 Q, at quality 50 (Q = 16, 17) and at
    DC = 255 only some are; the results are equal with the DC through the level-1 quantiser (where the create-time checks allow it) and
    with the table-lookup hook on"""
    p, dct, sums = _grey_tiles()
    luma, chroma = QM.tables(name)
    want = QM.quantise(dct, luma, chroma)
    multiple = (np.abs(sums) % (8 * int(luma[0])) == 0)
    assert multiple.any() and (name == "q100" or not multiple.all())
    qctx.set_quant_tables(luma, chroma)
    for variant in (0, 1):
        qctx.set_variant(variant)
        for hook in (0, 1):
            qctx.set_dc_table_lookup(hook)
            assert np.array_equal(qctx.fdct_quant(p, p, p, 256, 256), want), (name, variant, hook)


# ---- the extremes of the value range at Q = 1 ----
def test_extreme_coefficients_at_quality_100(J, qctx, oracle):
    """0 / 255 in coefficient (4, 4)'s sign pattern, and its negative: +-1020 there, the largest AC value 8-bit input can give (size 10);
    the DC differences between such blocks stay inside category 11; the encode succeeds and the file decodes"""
    sgn = np.array([1, -1, -1, 1, 1, -1, -1, 1])
    pat = np.outer(sgn, sgn)
    ones = np.ones(64, np.uint8)
    zz44 = QM.ZZ.index(4 * 8 + 4)
    for sign in (1, -1):
        p = np.where(np.tile(pat * sign, (2, 2)) > 0, 255, 0).astype(np.uint8).reshape(-1)
        want = QM.encode_coeffs(p, p, p, 16, 16, ones, ones)
        assert (want[0, 0, :4, zz44] == sign * 1020).all()
        qctx.set_quality(100)
        for variant in (0, 1):
            qctx.set_variant(variant)
            assert np.array_equal(qctx.fdct_quant(p, p, p, 16, 16), want), (sign, variant)
        jpg = qctx.encode_jpeg(p, p, p, 16, 16)
        assert jpg == J.write_jpeg(want, 16, 16, quant_tables=(ones, ones))
        info, r, g, b = qctx.decode_jpeg(jpg)
        _, orr, og, ob = oracle.decode_jpeg(jpg)
        assert np.array_equal(r, orr) and np.array_equal(g, og) and np.array_equal(b, ob)
    # black beside white: DC -1023 and +1015 in neighbouring blocks, a difference of category 11
    p = np.zeros((16, 16), np.uint8)
    p[:, 8:] = 255
    p = p.reshape(-1)
    want = QM.encode_coeffs(p, p, p, 16, 16, ones, ones)
    assert int(want[0, 0, 1, 0]) - int(want[0, 0, 0, 0]) > 1023
    assert qctx.encode_jpeg(p, p, p, 16, 16) == J.write_jpeg(want, 16, 16, quant_tables=(ones, ones))


# ---- files ----
def _dev_file(ctx, co, W, H, gray):
    import torch
    import jpezy_amd
    stride = jpezy_amd.load_library().jpezy_jpeg_bound(W, H)
    out = torch.zeros((1, stride), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
    ctx.write_jpeg_gpu_dev(torch.from_numpy(co.copy()).cuda(), W, H, out, sizes, gray=gray)
    torch.cuda.synchronize()
    n = int(sizes[0])
    assert n > 0
    return out[0, :n].cpu().numpy().tobytes()


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("name", ["q90", "random"])
def test_files_equal_the_host_writer_with_tables(J, qctx, name, gray):
    import torch
    W, H = 80, 48
    luma, chroma = QM.tables(name)
    qctx.set_quant_tables(luma, chroma)
    r, g, b = _rgb(W, H)
    rgb = np.ascontiguousarray(np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1))
    want = _want(W, H, gray, name)
    y, cb, cr = YM.synth_planes(W, H, "random")
    want_ycc = QM.quantise(_ycc_dct(W, H, gray), luma, chroma)
    for opt, ri in ((0, 0), (1, 0), (0, 3), (1, 3)):
        qctx.set_huffman_optimize(opt)
        qctx.set_restart_interval(ri)
        ref = J.write_jpeg(want, W, H, gray=gray, optimize=bool(opt), restart_interval=ri, quant_tables=(luma, chroma))
        assert qctx.encode_jpeg(r, g, b, W, H, gray=gray) == ref, ("encode_jpeg", opt, ri)
        assert qctx.encode_jpeg_packed(rgb, gray=gray) == ref, ("encode_jpeg_packed", opt, ri)
        assert qctx.encode_jpeg_ycc(y, cb, cr, gray=gray) == J.write_jpeg(want_ycc, W, H, gray=gray, optimize=bool(opt), restart_interval=ri,
                                                                         quant_tables=(luma, chroma)), ("encode_jpeg_ycc", opt, ri)
        assert qctx.write_jpeg_gpu(torch.from_numpy(want.copy()).cuda(), W, H, gray=gray)[0] == ref, ("write_jpeg_gpu", opt, ri)
        if not opt:                                            # the device-resident form refuses per-image tables
            assert _dev_file(qctx, want, W, H, gray) == ref, ("write_jpeg_gpu_dev", ri)


def test_default_setting_is_untouched(J, qctx, oracle):
    """a context that never calls the setters, sets quality 50 or passes the Annex-K tables writes every byte it wrote before"""
    W, H = 80, 48
    r, g, b = _rgb(W, H)
    c = oracle.constants()
    fresh = J.Context(0)
    try:
        before = fresh.encode_jpeg(r, g, b, W, H)
        co_before = fresh.fdct_quant(r, g, b, W, H)
        assert before == oracle.encode_jpeg(r, g, b, W, H)
        steps = [("set_quality(50)", lambda: fresh.set_quality(50)),
                 ("set_quant_tables(Annex K)", lambda: fresh.set_quant_tables(c["qt_luma"], c["qt_chroma"])),
                 ("set_quality(10), set_quality(50)", lambda: (fresh.set_quality(10), fresh.set_quality(50))),
                 ("set_quant_tables(None, None)", lambda: fresh.set_quant_tables(None, None))]
        for what, step in steps:
            step()
            assert fresh.encode_jpeg(r, g, b, W, H) == before, what
            assert np.array_equal(fresh.fdct_quant(r, g, b, W, H), co_before), what
            assert all(np.array_equal(a, b_) for a, b_ in zip(fresh.quant_tables(), (c["qt_luma"], c["qt_chroma"]))), what
        fresh.set_quality(10)
        assert fresh.encode_jpeg(r, g, b, W, H) != before
    finally:
        fresh.close()


# ---- the rules of the setter ----
def test_setter_argument_rules_leave_the_context_as_it_was(J, qctx):
    ones = np.ones(64, np.uint8)
    zero = ones.copy()
    zero[63] = 0
    qctx.set_quality(75)
    was = qctx.quant_tables()
    for bad in ((zero, ones), (ones, zero), (None, ones), (ones, None)):
        with pytest.raises(J.JpezyError, match="status -1"):
            qctx.set_quant_tables(*bad)
    for q in (0, 101):
        with pytest.raises(J.JpezyError, match="status -1"):
            qctx.set_quality(q)
    assert all(np.array_equal(a, b) for a, b in zip(qctx.quant_tables(), was))
    assert all(np.array_equal(a, b) for a, b in zip(was, J.quality_tables(75)))


def test_change_of_tables_between_two_streams(qctx):
    """the setter waits for the device before it rewrites the tables: a call in flight on one stream keeps the tables it was issued
    with, the call issued afterwards on another stream gets the new ones"""
    import torch
    W, H = 512, 512
    r, g, b = _rgb(W, H)
    planes = [torch.from_numpy(p.copy()).cuda() for p in (r, g, b)]
    mc, mr = W // 16, H // 16
    a = torch.zeros((mr, mc, 6, 64), dtype=torch.int16, device="cuda")
    bb = torch.zeros_like(a)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    qctx.set_quality(90)
    qctx.fdct_quant_dev(*planes, W, H, a, stream=s1.cuda_stream)
    qctx.set_quality(10)
    qctx.fdct_quant_dev(*planes, W, H, bb, stream=s2.cuda_stream)
    torch.cuda.synchronize()
    dct = QM.synth_dct(W, H)
    assert np.array_equal(a.cpu().numpy(), QM.quantise(dct, *QM.tables("q90")))
    assert np.array_equal(bb.cpu().numpy(), QM.quantise(dct, *QM.tables("q10")))


def test_setter_is_refused_during_capture_and_the_device_writer_is_capturable(J, qctx):
    """on the context's own stream: a setter call inside a capture is refused and leaves the context as it was; write_jpeg_gpu_dev is
    captured after the tables (and the header) are in place and replayed on changed coefficients.  One stream, no parallel branches."""
    import torch
    W, H = 80, 48
    luma, chroma = QM.tables("q90")
    qctx.set_quant_tables(luma, chroma)
    frames = [QM.quantise(QM.synth_dct(W, H, False, frame=f), luma, chroma) for f in (0, 1)]
    co = torch.from_numpy(frames[0].copy()).cuda()
    stride = J.load_library().jpezy_jpeg_bound(W, H)
    out = torch.zeros((1, stride), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = torch.cuda.ExternalStream(qctx.stream())
    qctx.write_jpeg_gpu_dev(co, W, H, out, sizes, stream=s.cuda_stream)      # header and scratch: outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    refused = []
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            for call in (lambda: qctx.set_quality(10), lambda: qctx.set_quant_tables(None, None)):
                try:
                    call()
                    refused.append(None)
                except J.JpezyError as e:
                    refused.append(str(e))
            qctx.write_jpeg_gpu_dev(co, W, H, out, sizes, stream=s.cuda_stream)
    assert all(m is not None and "status -1" in m and "captured" in m for m in refused), refused
    assert all(np.array_equal(a, b) for a, b in zip(qctx.quant_tables(), (luma, chroma)))
    for f in (1, 0):
        co.copy_(torch.from_numpy(frames[f].copy()).cuda())
        out.zero_(); sizes.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want = J.write_jpeg(frames[f], W, H, quant_tables=(luma, chroma))
        assert int(sizes[0]) == len(want) and out[0, :len(want)].cpu().numpy().tobytes() == want, f
    # the context still encodes with the tables it had
    r, g_, b = _rgb(W, H)
    assert np.array_equal(qctx.fdct_quant(r, g_, b, W, H), frames[0])


# ---- our own decoder on our own files ----
@pytest.mark.parametrize("q", [90, 10])
def test_round_trip_through_the_fused_decoder(qctx, oracle, q):
    W, H = 80, 48
    r, g, b = _rgb(W, H)
    qctx.set_quality(q)
    jpg = qctx.encode_jpeg(r, g, b, W, H)
    info, dr, dg, db = qctx.decode_jpeg(jpg)
    oinfo, orr, og, ob = oracle.decode_jpeg(jpg)
    luma, chroma = QM.tables(f"q{q}")
    assert np.array_equal(np.array(info.qt[0][:]), luma) and np.array_equal(np.array(info.qt[1][:]), chroma)
    assert np.array_equal(dr, orr) and np.array_equal(dg, og) and np.array_equal(db, ob)


def test_fallback_counter_at_quality_100(qctx):
    """a sanity check, not a rate: with every quantiser 1 the guard bands are at their widest and no coefficient is zero"""
    W, H = 80, 48
    r, g, b = _rgb(W, H)
    qctx.set_quality(100)
    qctx.fallback_count()
    got = qctx.fdct_quant(r, g, b, W, H)
    n = qctx.fallback_count()
    assert 0 < n <= got.size, n
    assert np.array_equal(got, _want(W, H, False, "q100"))


# ---- CLI ----
def test_cli_quality_flag(J, qctx, oracle, tmp_path):
    """jpezy_encode in.ppm out.jpg --quality=N beside --gray, --optimize and --restart=N, the token anywhere behind the output name;
    and with --i420"""
    from jpezy_amd import _build
    _build.build_all()
    enc = Path(_build.BIN) / "jpezy_encode"
    W, H = 80, 48
    r, g, b = _rgb(W, H)
    src = tmp_path / "in.ppm"
    src.write_bytes(oracle.format_ppm_p3(W, H, r, g, b))
    run = lambda *a: subprocess.run([str(x) for x in a], capture_output=True, text=True, timeout=120)
    for flags, q, gray, opt, ri in ((["--quality=90"], 90, False, False, 0), (["--gray", "--quality=25"], 25, True, False, 0),
                                    (["--quality=100", "--optimize", "--gray"], 100, True, True, 0),
                                    (["--optimize", "--restart=3", "--quality=1"], 1, False, True, 3),
                                    (["--quality=50"], 50, False, False, 0)):
        out = tmp_path / "a.jpg"
        p = run(enc, src, out, *flags)
        assert p.returncode == 0, (flags, p.stderr)
        want = J.write_jpeg(_want(W, H, gray, f"q{q}"), W, H, gray, optimize=opt, restart_interval=ri, quant_tables=QM.tables(f"q{q}"))
        assert out.read_bytes() == want, flags
    assert out.read_bytes() == oracle.encode_jpeg(r, g, b, W, H)           # --quality=50 is the file without the flag
    y, cb, cr = YM.synth_planes(W, H, "random")
    yuv = tmp_path / "in.yuv"
    yuv.write_bytes(y.tobytes() + cb.tobytes() + cr.tobytes())
    p = run(enc, f"--i420={W}x{H}", yuv, tmp_path / "b.jpg", "--quality=75", "--restart=2")
    assert p.returncode == 0, p.stderr
    luma, chroma = QM.tables("q75")
    assert (tmp_path / "b.jpg").read_bytes() == J.write_jpeg(QM.quantise(_ycc_dct(W, H, False), luma, chroma), W, H, restart_interval=2,
                                                            quant_tables=(luma, chroma))
