"""Smooth chroma upsampling, as far as it can be checked without a GPU: the numpy restatement of its definition (tests/smooth_model.py)
against the existing decode where nothing is smoothed, against libjpeg-turbo's fancy upsamplers (through Pillow) where something is,
the ramp property of the filter, the per-component rule of a mixed layout, and the argument checks of the new entry points that come
before any device is touched.  tests/test_gpu_smooth.py holds the parity tests."""
import ctypes as C
import io

import numpy as np
import pytest

import scaled_model
import smooth_model as M
from jpeg_synth import synth_jpeg

E_BADARG, E_UNSUPPORTED = -1, -4
L444 = [(1, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]
L411 = [(4, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]
ONE = [(1, 1, 0, 0)]
ONE_2X2 = [(2, 2, 0, 0)]
MIXED = [(2, 2, 0, 0), (2, 1, 1, 1), (1, 2, 1, 1)]


def chroma_over(h, v):
    return [(h, v, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("layout", [L444, L411, ONE, ONE_2X2], ids=["444", "411", "one", "one_2x2"])
def test_nothing_smoothed_is_the_existing_decode(oracle, layout, gray):
    for W, H in ((37, 21), (16, 16), (3, 3)):
        data, _, _ = synth_jpeg(W, H, layout, seed=5)
        info, co = oracle.read_jpeg(data)
        assert all(M.factors(info, c) is None for c in range(3))
        got = M.decode_planes(co, info, gray)
        want = scaled_model.decode_planes(co, info, 1, gray)
        for a, e in zip(got, want):
            assert np.array_equal(a, e)


SIZES = [(64, 48), (33, 17), (47, 65), (16, 16), (17, 16), (16, 17), (48, 9), (7, 40), (6, 6), (5, 3)]


@pytest.mark.parametrize("hv", [(2, 2), (2, 1), (1, 2), (1, 1)])
def test_filter_is_libjpeg_turbos_fancy_upsampling(oracle, hv):
    """DC-only blocks under quantisers of 8: both inverse transforms give DC + 128 exactly, so only the upsamplers are compared.
    draft("YCbCr") makes libjpeg return the upsampled components without colour conversion."""
    Image = pytest.importorskip("PIL.Image")
    planes = 0
    for W, H in SIZES:
        for seed in range(3):
            data, _, _ = synth_jpeg(W, H, chroma_over(*hv), seed=seed, density=0.0, qt=np.full((2, 64), 8))
            im = Image.open(io.BytesIO(data))
            im.draft("YCbCr", im.size)
            im.load()
            assert im.mode == "YCbCr"
            want = np.asarray(im)
            info, co = oracle.read_jpeg(data)
            got = M.component_planes(co, info)
            for c in range(3):
                assert (M.factors(info, c) is not None) == (c > 0 and hv != (1, 1))
                assert np.array_equal(np.clip(got[c], 0, 255), want[:, :, c]), (hv, W, H, seed, c)
                planes += 1
    assert planes == 90


@pytest.mark.parametrize("fx,fy,rep_err", [(2, 2, 3), (2, 1, 1), (1, 2, 2)])
def test_ramp_comes_back(fx, fy, rep_err):
    """the ramp 2x + 4y + 10, box-averaged fx x fy (the mean is an integer): the filter gives it back exactly away from the outermost
    sample ring, replication is off by 3, 1, 2"""
    W, H = 32, 24
    y, x = np.mgrid[:H, :W]
    ramp = 2 * x + 4 * y + 10
    box = ramp.reshape(H // fy, fy, W // fx, fx).sum(axis=(1, 3))
    assert not (box % (fx * fy)).any()
    P = box // (fx * fy)
    U = M.upsample(P, fx, fy, W, H)
    inner = (slice(fy, H - fy), slice(fx, W - fx))
    assert np.array_equal(U[inner], ramp[inner])
    rep = np.repeat(np.repeat(P, fy, axis=0), fx, axis=1)
    assert int(np.abs(rep - ramp)[inner].max()) == rep_err
    assert int(np.abs(U - ramp).max()) <= rep_err                    # the clamped ring is no worse than replication


def _filter_by_the_letter(P, fx, fy, W, H):
    """the definition's formulas, one pixel at a time"""
    hc, wc = P.shape

    def p(i, j):
        return int(P[min(max(j, 0), hc - 1), min(max(i, 0), wc - 1)])

    U = np.zeros((H, W), np.int64)
    for Y in range(H):
        for X in range(W):
            i, j = X >> 1, Y >> 1
            if (fx, fy) == (2, 1):
                U[Y, X] = (3 * p(i, Y) + p(i + 1, Y) + 2) >> 2 if X & 1 else (3 * p(i, Y) + p(i - 1, Y) + 1) >> 2
            elif (fx, fy) == (1, 2):
                U[Y, X] = (3 * p(X, j) + p(X, j + 1) + 2) >> 2 if Y & 1 else (3 * p(X, j) + p(X, j - 1) + 1) >> 2
            else:
                d = 1 if Y & 1 else -1
                s = lambda k: 3 * p(k, j) + p(k, j + d)
                U[Y, X] = (3 * s(i) + s(i + 1) + 7) >> 4 if X & 1 else (3 * s(i) + s(i - 1) + 8) >> 4
    return U


def test_mixed_layout_each_component_its_own_rule(oracle):
    W, H = 29, 19
    data, _, _ = synth_jpeg(W, H, MIXED, seed=11)
    info, co = oracle.read_jpeg(data)
    assert [M.factors(info, c) for c in range(3)] == [None, (1, 2), (2, 1)]
    assert [M.component_size(info, c) for c in range(3)] == [(29, 19), (29, 10), (15, 19)]
    got = M.component_planes(co, info)
    luma_only = scaled_model.decode_planes(co, info, 1, True)[0].reshape(H, W)
    assert np.array_equal(np.clip(got[0], 0, 255), luma_only)                         # component 0: the existing placement
    for c in (1, 2):
        P = M.native_plane(co, info, c)
        assert P.shape == M.component_size(info, c)[::-1]
        assert np.array_equal(got[c], _filter_by_the_letter(P, *M.factors(info, c), W, H))
    # the two rules are not interchangeable on this file
    assert not np.array_equal(got[1], scaled_model_component(co, info, 1)) and not np.array_equal(got[2], scaled_model_component(co, info, 2))


def scaled_model_component(co, info, c):
    """component c as the existing decode places it (replication): the model's placement"""
    return M._components(co, info)[c][0]


def test_quality_picture_premise():
    """the picture tests/test_gpu_smooth.py decodes both ways: with its chroma planes taken as they are (no transform error), the smooth
    decode's Cb error away from the outer two pixels is no larger at its maximum and strictly smaller on average than replication's"""
    y, cb, cr, cb_full = M.centred_ramp_picture()
    H, W = y.shape
    err = {}
    for name, up in (("smooth", lambda p: M.upsample(p, 2, 2, W, H)), ("nearest", lambda p: np.repeat(np.repeat(p.astype(np.int64), 2, 0), 2, 1))):
        yv, uv, vv = y.astype(np.float64), up(cb).astype(np.float64), up(cr).astype(np.float64)
        r = scaled_model.revise(yv + (vv - 0x80) * 1.4020)
        g = scaled_model.revise(yv - (uv - 0x80) * 0.3441 - (vv - 0x80) * 0.7139)
        b = scaled_model.revise(yv + (uv - 0x80) * 1.7718)
        assert 0 < min(r.min(), g.min(), b.min()) and max(r.max(), g.max(), b.max()) < 255          # nothing clamped
        err[name] = np.abs(M.cb_of_rgb(r, g, b) - cb_full)[2:-2, 2:-2]
    print({k: (float(v.max()), float(v.mean())) for k, v in err.items()})
    assert err["smooth"].max() <= err["nearest"].max() and err["smooth"].mean() < err["nearest"].mean()
    assert err["nearest"].mean() - err["smooth"].mean() > 0.1                                       # a margin the transform's rounding does not eat


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def test_constants(J):
    assert (J.UPSAMPLE_NEAREST, J.UPSAMPLE_SMOOTH) == (0, 1)


def test_argument_checks_before_any_device(J):
    lib = J.load_library()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    qt = ((C.c_uint16 * 64) * 4)()
    one = (C.c_uint8 * 3)(1, 1, 1)
    tq = (C.c_uint8 * 3)(0, 1, 1)
    info = J.FrameInfo()

    def calls(ctx, up, precision=8):
        return {
            "dequant_idct_upsampling_dev": lambda: lib.jpezy_dequant_idct_upsampling_dev(ctx, p, C.byref(qt), 3, C.byref(one), C.byref(one), C.byref(tq),
                                                                                         precision, 16, 16, 0, up, 1, 256, p, p, p, None),
            "dequant_idct_upsampling_packed_dev": lambda: lib.jpezy_dequant_idct_upsampling_packed_dev(None, p, C.byref(qt), 3, C.byref(one), C.byref(one),
                                                                                                       C.byref(tq), precision, 16, 16, 0, up, 0, 0, 0, 1,
                                                                                                       p, None),
            "decode_jpeg_upsampling": lambda: lib.jpezy_decode_jpeg_upsampling(ctx, p, 64, 0, up, C.byref(info), p, p, p, 1024),
            "decode_jpeg_upsampling_packed": lambda: lib.jpezy_decode_jpeg_upsampling_packed(ctx, p, 64, 0, up, C.byref(info), 0, 0, p, buf.size),
        }

    for up in (J.UPSAMPLE_NEAREST, J.UPSAMPLE_SMOOTH):                                # a null context is refused with a message
        for name, call in calls(None, up).items():
            assert call() == E_BADARG, (name, up)
            msg = lib.jpezy_hip_last_error()
            assert b"context" in msg or b"argument" in msg, (name, up, msg)
    for up in (2, -1, 7):                                                             # any other value, before the context is looked at
        for name, call in calls(None, up).items():
            assert call() == E_BADARG, (name, up)
            assert b"upsampling" in lib.jpezy_hip_last_error(), (name, up)
    for name, call in calls(None, J.UPSAMPLE_SMOOTH, precision=12).items():           # the device entries know the precision up front
        if name.startswith("dequant"):
            assert call() == E_UNSUPPORTED, name
            assert b"8-bit" in lib.jpezy_hip_last_error()


def test_decoder_refuses_smooth_with_scale_or_region(J, tmp_path):
    d = J.Decoder(tmp_path / "missing.jpg")
    for kw in (dict(scale=2), dict(region=(0, 0, 1, 1)), dict(scale=4, region=(0, 0, 1, 1))):
        with pytest.raises(J.JpezyError, match=f"status {E_UNSUPPORTED}"):
            d.decode(upsampling=J.UPSAMPLE_SMOOTH, **kw)
    assert d.decode(upsampling=J.UPSAMPLE_SMOOTH) is None                             # a missing file: as without the keyword
