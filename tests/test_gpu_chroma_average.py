"""JPEZY_DOWNSAMPLE_AVERAGE on the GPU (include/jpezy_hip.h, CHROMA DOWNSAMPLING): the transform kernel's averaged
chroma stage against tests/chroma_average_model.py for equality -- planar, RGB24 and BGRA32 with a padded row stride, every
force_exact level, three table sets --, a picture whose colours sit on the colour guard bands, a call of three frames, the mode
leaving no trace once it is switched off or where it is not consulted, the end-to-end entries against the host writer, the refusals,
the aliasing claim on the device, and the CLI flag.

Shapes (the work unit is the quad: four 16 x 16 MCUs per wave, lane = 4 * pixel row + MCU): 1 x 1 and 2 x 2 (all clamp), 17 x 33 (odd
edges: the last 2x2 is clamped duplicates in both directions; the byte loop), 72 x 24 (five MCUs: a partial quad), 128 x 32 (the
16-byte load form, two quads = one two-wave workgroup, two MCU rows), 126 x 30 (its unaligned neighbour), 256 x 16 (four quads: the
four-wave workgroup of the planar cooperative load)."""
import io
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import chroma_average_model as CA
import quant_model as QM
import sampling_model as SM
import ycc_model as YM

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(1, 1), (2, 2), (17, 33), (72, 24), (128, 32), (126, 30), (256, 16)]
TABLES = ["q50", "q100", "255_dc1"]
PICTURES = ["random", "synth", "zeros", "full", "guard"]
BADARG, UNSUPPORTED = -1, -4


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
def actx(J, ctx):
    """the module's context in the averaged mode, handed back at its defaults"""
    ctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
    yield ctx
    ctx.set_chroma_downsampling(J.DOWNSAMPLE_POINT)
    ctx.set_quant_tables(None, None)
    ctx.set_variant(1)
    ctx.set_force_exact(0)
    ctx.set_huffman_optimize(0)
    ctx.set_restart_interval(0)


@lru_cache(maxsize=None)
def _guard_colours():
    cols = CA.guard_band_colours()
    cols.setflags(write=False)
    return cols


@lru_cache(maxsize=None)
def _picture(kind, W, H, frame=0):
    """planar r, g, b (flat uint8, read-only), computed once"""
    if kind == "random":
        rng = np.random.default_rng(977 * W + H + 31 * frame)
        out = tuple(rng.integers(0, 256, W * H, dtype=np.uint8) for _ in range(3))
    elif kind == "synth":
        from oracle import oracle as O
        out = tuple(np.asarray(p).copy() for p in O.synth_rgb(W, H, frame=frame))
    elif kind == "stripes":
        out = CA.stripes(W, H)
    elif kind == "guard":
        # colours whose FP64 Cb or Cr sits on an integer, shuffled over the picture: every lane's vote fires, the 2x2s mix them
        cols = _guard_colours()
        pick = np.random.default_rng(W + 1000 * H).integers(0, len(cols), W * H)
        out = tuple(np.ascontiguousarray(cols[pick, k]) for k in range(3))
    else:
        out = tuple(np.full(W * H, {"zeros": 0, "full": 255}[kind], np.uint8) for _ in range(3))
    for p in out:
        p.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def _dct(kind, W, H, frame=0, mode=CA.AVERAGE):
    d = CA.dct_from_rgb(*_picture(kind, W, H, frame), W, H, mode)
    d.setflags(write=False)
    return d


def _want(kind, W, H, name, frame=0, mode=CA.AVERAGE):
    return QM.quantise(_dct(kind, W, H, frame, mode), *QM.tables(name))


def _shape(W, H, n=None, gray=False):
    s = ((H + 15) // 16, (W + 15) // 16, 4 if gray else 6, 64)
    return s if n is None else (n,) + s


def _dev_entries(J, ctx, r, g, b, W, H):
    """fdct_quant_dev (planar), fdct_quant_packed_dev RGB24 (tight) and BGRA32 (row stride padded by 16 bytes)"""
    import torch
    out = []
    planes = [torch.from_numpy(np.asarray(p).copy()).cuda() for p in (r, g, b)]
    co = torch.full(_shape(W, H), 0x5A5A, dtype=torch.int16, device="cuda")
    ctx.fdct_quant_dev(*planes, W, H, co)
    out.append(("planar", co))
    rgb = np.stack([np.asarray(p).reshape(H, W) for p in (r, g, b)], axis=-1)
    co = torch.full(_shape(W, H), 0x5A5A, dtype=torch.int16, device="cuda")
    ctx.fdct_quant_packed_dev(torch.from_numpy(np.ascontiguousarray(rgb)).cuda(), co, format=J.PIX_RGB24)
    out.append(("RGB24", co))
    bgra = np.full((H, W + 4, 4), 7, np.uint8)                   # 16 bytes of padding behind every row
    bgra[:, :W, :3] = rgb[..., ::-1]
    d = torch.from_numpy(bgra).cuda()
    co = torch.full(_shape(W, H), 0x5A5A, dtype=torch.int16, device="cuda")
    ctx.fdct_quant_packed_dev(d[:, :W], co, format=J.PIX_BGRA32)
    out.append(("BGRA32 padded", co))
    torch.cuda.synchronize()
    return [(n, c.cpu().numpy()) for n, c in out]


def _check_every_entry(J, ctx, kind, W, H, want, tag):
    for entry, co in _dev_entries(J, ctx, *_picture(kind, W, H), W, H):
        bad = np.argwhere(co != want)
        assert bad.size == 0, (entry, tag, len(bad), bad[:4].tolist())


# ---- coefficients ----
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("kind", PICTURES)
def test_coefficients_equal_the_model(J, actx, kind, W, H):
    if kind == "guard":
        assert len(_guard_colours()) >= 64          # the search cannot pass empty
    for name in TABLES:
        actx.set_quant_tables(*QM.tables(name))
        _check_every_entry(J, actx, kind, W, H, _want(kind, W, H, name), (kind, name))


def test_the_averaged_stage_differs_from_point_sampling(J, actx):
    """the test above cannot pass on the point-sampling kernel: on random pixels the two models differ in the chroma blocks only"""
    W, H = 72, 24
    a, p = _want("random", W, H, "q50"), _want("random", W, H, "q50", mode=CA.POINT)
    assert np.array_equal(a[:, :, :4], p[:, :, :4]) and not np.array_equal(a[:, :, 4:], p[:, :, 4:])


@pytest.mark.parametrize("fe", [1, 2, 3])
def test_force_exact_levels_give_the_same_coefficients(J, actx, fe):
    W, H = 72, 24
    for name in TABLES:
        actx.set_quant_tables(*QM.tables(name))
        actx.set_force_exact(fe)
        actx.fallback_count()
        want = _want("random", W, H, name)
        _check_every_entry(J, actx, "random", W, H, want, (name, fe))
        assert actx.fallback_count() >= want.size, (name, fe)    # the hooks send every coefficient down the exact paths


def test_three_frames_in_one_call(J, actx):
    import torch
    W, H, n = 72, 24, 3
    frames = [_picture("random", W, H, f) for f in range(n)]
    want = np.stack([_want("random", W, H, "q50", f) for f in range(n)])
    planes = [torch.from_numpy(np.concatenate([fr[k] for fr in frames])).cuda() for k in range(3)]
    co = torch.full(_shape(W, H, n), 0x5A5A, dtype=torch.int16, device="cuda")
    actx.fdct_quant_dev(*planes, W, H, co, n_frames=n)
    rgb = np.stack([np.stack([fr[k].reshape(H, W) for k in range(3)], axis=-1) for fr in frames])
    cp = torch.full(_shape(W, H, n), 0x5A5A, dtype=torch.int16, device="cuda")
    actx.fdct_quant_packed_dev(torch.from_numpy(np.ascontiguousarray(rgb)).cuda(), cp, format=J.PIX_RGB24)
    torch.cuda.synchronize()
    assert np.array_equal(co.cpu().numpy(), want) and np.array_equal(cp.cpu().numpy(), want)
    # the host-buffer transform (bands of MCU rows through the same launch)
    got = actx.fdct_quant(*[np.concatenate([fr[k] for fr in frames]) for k in range(3)], W, H, n_frames=n)
    assert np.array_equal(np.asarray(got).reshape(want.shape), want)


# ---- nothing leaks ----
def test_back_to_point_is_a_fresh_context(J, ctx):
    W, H = 72, 24
    r, g, b = _picture("random", W, H)
    ctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
    assert ctx.chroma_downsampling() == J.DOWNSAMPLE_AVERAGE
    averaged = ctx.encode_jpeg(r, g, b, W, H)
    ctx.set_chroma_downsampling(J.DOWNSAMPLE_POINT)
    assert ctx.chroma_downsampling() == J.DOWNSAMPLE_POINT
    fresh = J.Context(0)
    try:
        assert fresh.chroma_downsampling() == J.DOWNSAMPLE_POINT
        want = _want("random", W, H, "q50", mode=CA.POINT)
        for c in (ctx, fresh):
            assert np.array_equal(np.asarray(c.fdct_quant(r, g, b, W, H)).reshape(want.shape), want)
            _check_every_entry(J, c, "random", W, H, want, "point")
        jpg = ctx.encode_jpeg(r, g, b, W, H)
        assert jpg == fresh.encode_jpeg(r, g, b, W, H) == J.write_jpeg(want, W, H) and jpg != averaged
    finally:
        fresh.close()


def test_gray_444_and_ycc_do_not_consult_the_mode(J, actx):
    import torch
    W, H = 72, 24
    r, g, b = _picture("random", W, H)
    luma, chroma = QM.tables("q50")
    gray = QM.encode_coeffs(r, g, b, W, H, luma, chroma, gray=True)
    assert np.array_equal(np.asarray(actx.fdct_quant(r, g, b, W, H, gray=True)).reshape(gray.shape), gray)
    assert actx.encode_jpeg(r, g, b, W, H, gray=True) == J.write_jpeg(gray, W, H, gray=True)
    want444 = SM.encode_coeffs(r, g, b, W, H, luma, chroma)
    planes = [torch.from_numpy(np.asarray(p).copy()).cuda() for p in (r, g, b)]
    co = torch.full(want444.shape, 0x5A5A, dtype=torch.int16, device="cuda")
    actx.fdct_quant_dev(*planes, W, H, co, sampling=J.SAMPLING_444)
    torch.cuda.synchronize()
    assert np.array_equal(co.cpu().numpy(), want444)
    assert actx.encode_jpeg(r, g, b, W, H, sampling=J.SAMPLING_444) == SM.write_jpeg(want444, W, H)
    y, cb, cr = YM.synth_planes(W, H, "random")
    assert actx.encode_jpeg_ycc(y, cb, cr) == J.write_jpeg(YM.encode_coeffs(y, cb, cr), W, H)
    # SAMPLING_420 as an argument is the entry it stands for: the mode acts
    co = torch.full(_shape(W, H), 0x5A5A, dtype=torch.int16, device="cuda")
    actx.fdct_quant_dev(*planes, W, H, co, sampling=J.SAMPLING_420)
    torch.cuda.synchronize()
    assert np.array_equal(co.cpu().numpy(), _want("random", W, H, "q50"))


# ---- end to end ----
@pytest.mark.parametrize("run", ["plain", "optimize", "restart5_q90"])
@pytest.mark.parametrize("W,H", [(72, 24), (17, 33)])
def test_files_equal_the_host_writer(J, actx, W, H, run):
    Image = pytest.importorskip("PIL.Image")
    r, g, b = _picture("synth", W, H)
    name, opts = "q50", {}
    if run == "optimize":
        actx.set_huffman_optimize(1)
        opts = {"optimize": True}
    elif run == "restart5_q90":
        actx.set_restart_interval(5)
        actx.set_quality(90)
        name, opts = "q90", {"restart_interval": 5, "quant_tables": QM.tables("q90")}
    want = _want("synth", W, H, name)
    ref = J.write_jpeg(want, W, H, **opts)
    assert ref != J.write_jpeg(_want("synth", W, H, name, mode=CA.POINT), W, H, **opts)
    assert actx.encode_jpeg(r, g, b, W, H) == ref
    img = np.stack([p.reshape(H, W) for p in (b, g, r)], axis=-1)
    assert actx.encode_jpeg_packed(img, format=J.PIX_BGR24) == ref
    im = Image.open(io.BytesIO(ref))
    im.load()
    assert im.size == (W, H) and im.mode == "RGB"
    info, dr, dg, db = actx.decode_jpeg(ref)
    assert (info.width, info.height) == (W, H) and len(dr) == len(dg) == len(db) == W * H


# ---- refusals ----
def test_refusals_leave_the_context_usable(J, actx):
    import torch
    for mode in (2, -1):
        with pytest.raises(J.JpezyError, match=f"status {BADARG}"):
            actx.set_chroma_downsampling(mode)
    assert actx.chroma_downsampling() == J.DOWNSAMPLE_AVERAGE
    W, H = 72, 24
    r, g, b = _picture("random", W, H)
    planes = [torch.from_numpy(np.asarray(p).copy()).cuda() for p in (r, g, b)]
    rgb = torch.from_numpy(np.ascontiguousarray(np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1))).cuda()
    co = torch.full(_shape(W, H), 0x5A5A, dtype=torch.int16, device="cuda")
    actx.set_variant(0)
    for call in (lambda: actx.fdct_quant_dev(*planes, W, H, co), lambda: actx.fdct_quant_packed_dev(rgb, co, format=J.PIX_RGB24),
                 lambda: actx.fdct_quant(r, g, b, W, H), lambda: actx.encode_jpeg(r, g, b, W, H),
                 lambda: actx.encode_jpeg_packed(rgb.cpu().numpy(), format=J.PIX_RGB24)):
        with pytest.raises(J.JpezyError, match=f"status {UNSUPPORTED}"):
            call()
    torch.cuda.synchronize()
    assert (co.cpu().numpy() == 0x5A5A).all()                    # nothing was launched
    # the same context, still on variant 0: gray does not consult the mode
    luma, chroma = QM.tables("q50")
    gray = QM.encode_coeffs(r, g, b, W, H, luma, chroma, gray=True)
    assert np.array_equal(np.asarray(actx.fdct_quant(r, g, b, W, H, gray=True)).reshape(gray.shape), gray)
    actx.set_variant(1)
    _check_every_entry(J, actx, "random", W, H, _want("random", W, H, "q50"), "after the refusal")


# ---- the point of it ----
def test_stripes_alias_less_on_the_device(J, actx):
    W, H = 64, 48
    src = _picture("stripes", W, H)
    flat = np.stack(src).astype(np.float64)
    actx.set_quality(90)
    mse = {}
    for mode in (J.DOWNSAMPLE_POINT, J.DOWNSAMPLE_AVERAGE):
        actx.set_chroma_downsampling(mode)
        _, r, g, b = actx.decode_jpeg(actx.encode_jpeg(*src, W, H))
        mse[mode] = float(np.mean((np.stack([np.asarray(p).reshape(-1) for p in (r, g, b)]).astype(np.float64) - flat) ** 2))
    print("stripes at quality 90, MSE: point %.1f, average %.1f" % (mse[J.DOWNSAMPLE_POINT], mse[J.DOWNSAMPLE_AVERAGE]))
    assert mse[J.DOWNSAMPLE_AVERAGE] < mse[J.DOWNSAMPLE_POINT]


# ---- CLI ----
def test_cli_writes_the_bytes_of_the_context(J, actx, tmp_path):
    exe = ROOT / "jpezy_amd" / "bin" / "jpezy_encode"
    assert exe.exists()
    W, H = 72, 24
    r, g, b = _picture("synth", W, H)
    ppm = tmp_path / "in.ppm"
    ppm.write_text("P3\n%d %d\n255\n" % (W, H) + " ".join(map(str, np.stack([r, g, b], axis=-1).reshape(-1).tolist())) + "\n")
    actx.set_quality(90)
    averaged = actx.encode_jpeg(r, g, b, W, H)
    actx.set_chroma_downsampling(J.DOWNSAMPLE_POINT)
    pointed = actx.encode_jpeg(r, g, b, W, H)
    assert averaged != pointed
    for flags, want in ((["--chroma=average", "--quality=90"], averaged), (["--quality=90", "--chroma=point"], pointed), (["--quality=90"], pointed),
                        (["--quality=90", "--sampling=420", "--chroma=average"], averaged)):
        out = tmp_path / "out.jpg"
        p = subprocess.run([str(exe), str(ppm), str(out), *flags], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        assert out.read_bytes() == want, flags
        out.unlink()
    out = tmp_path / "batch.jpg"
    p = subprocess.run([str(exe), "--gpus", "1", "--chroma=average", str(ppm), str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    actx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
    actx.set_quant_tables(None, None)
    assert out.read_bytes() == actx.encode_jpeg(r, g, b, W, H)
