"""JPEZY_DOWNSAMPLE_AVERAGE, host side (include/jpezy_hip.h, CHROMA DOWNSAMPLING): the model of the definition
(tests/chroma_average_model.py) against the point-sampling model it extends, the floor and the bias on hand-made 2x2s, pixel-doubled
pictures, the aliasing claim on one-pixel colour stripes through the oracle's writer and decoder, and the surface of the ABI.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import chroma_average_model as CA
import quant_model as QM

ROOT = Path(__file__).resolve().parent.parent
BADARG = -1


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.mark.parametrize("W,H", [(64, 48), (17, 33), (1, 1)])
@pytest.mark.parametrize("name", ["q50", "q100"])
def test_point_mode_is_quant_model(oracle, W, H, name):
    r, g, b = oracle.synth_rgb(W, H, frame=2)
    luma, chroma = QM.tables(name)
    point = CA.encode_coeffs(r, g, b, W, H, luma, chroma, mode=CA.POINT)
    assert np.array_equal(point, QM.encode_coeffs(r, g, b, W, H, luma, chroma))
    if name == "q50":
        assert np.array_equal(point, oracle.encode_coeffs(r, g, b, W, H))
    # the luma blocks do not depend on the mode
    assert np.array_equal(CA.encode_coeffs(r, g, b, W, H, luma, chroma)[:, :, :4], point[:, :, :4])


def test_floor_and_bias_on_hand_made_2x2s():
    def at_both_parities(quad):
        """the 2x2 placed at x' = 0 and at x' = 1"""
        c = np.tile(np.asarray(quad, np.int64).reshape(2, 2), (1, 2))
        return CA.average_2x2(c)[0].tolist()
    assert at_both_parities([-1, -1, -1, -1]) == [-1, -1]        # truncation toward zero would give 0
    assert at_both_parities([0, 0, 0, 1]) == [0, 0]
    assert at_both_parities([0, 0, 1, 1]) == [0, 1]
    assert at_both_parities([1, 0, 1, 0]) == [0, 1]              # the position inside the 2x2 does not matter
    assert at_both_parities([-127, -127, -127, -128]) == [-127, -127]
    assert at_both_parities([-1, -1, -2, -2]) == [-2, -1]
    # libjpeg's rule on unsigned samples, shifted by 128: adding 128 to the four inputs adds 128 to the result
    rng = np.random.default_rng(11)
    c = rng.integers(-128, 128, (16, 16))
    assert np.array_equal(CA.average_2x2(c + 128), CA.average_2x2(c) + 128)
    u = c + 128
    s = u[0::2, 0::2] + u[0::2, 1::2] + u[1::2, 0::2] + u[1::2, 1::2]
    assert np.array_equal(CA.average_2x2(u), (s + np.array([1, 2] * 4)) // 4)


@pytest.mark.parametrize("W,H", [(64, 48), (61, 47)])
def test_pixel_doubled_pictures_give_the_same_coefficients_in_both_modes(W, H):
    r, g, b = CA.doubled(W, H)
    for name in ("q50", "q100"):
        luma, chroma = QM.tables(name)
        assert np.array_equal(CA.encode_coeffs(r, g, b, W, H, luma, chroma, mode=CA.AVERAGE),
                              CA.encode_coeffs(r, g, b, W, H, luma, chroma, mode=CA.POINT)), name


def _mse(oracle, co, W, H, src):
    _, r, g, b = oracle.decode_jpeg(oracle.write_jpeg(co, W, H))
    got = np.stack([np.asarray(p).reshape(-1) for p in (r, g, b)]).astype(np.float64)
    return float(np.mean((got - np.stack(src).astype(np.float64)) ** 2))


def test_stripes_alias_less_when_averaged(oracle):
    """one-pixel colour stripes, Annex-K tables: point sampling reproduces one colour everywhere (wrong by d on half the pixels), the
    average is wrong by d / 2 on all of them -- half the squared error"""
    W, H = 64, 48
    src = CA.stripes(W, H)
    c = oracle.constants()
    mse = {m: _mse(oracle, CA.encode_coeffs(*src, W, H, c["qt_luma"], c["qt_chroma"], mode=m), W, H, src) for m in (CA.POINT, CA.AVERAGE)}
    print("stripes MSE: point %.1f, average %.1f" % (mse[CA.POINT], mse[CA.AVERAGE]))
    assert mse[CA.AVERAGE] < mse[CA.POINT]


def test_guard_band_search_finds_colours():
    cols = CA.guard_band_colours()
    assert len(cols) >= 64 and cols.dtype == np.uint8 and cols.shape[1] == 3


def test_header_library_and_package_agree(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    assert re.search(r"enum\s+jpezy_downsampling\s*\{\s*JPEZY_DOWNSAMPLE_POINT\s*=\s*0\s*,\s*JPEZY_DOWNSAMPLE_AVERAGE\s*=\s*1\s*\}", text)
    assert re.search(r"int\s+jpezy_ctx_set_chroma_downsampling\(jpezy_ctx\*\s*ctx,\s*int\s+mode\);", text)
    assert re.search(r"int\s+jpezy_ctx_chroma_downsampling\(jpezy_ctx\*\s*ctx\);", text)
    lib = C.CDLL(str(J.library_path()))
    for name in ("jpezy_ctx_set_chroma_downsampling", "jpezy_ctx_chroma_downsampling"):
        assert hasattr(lib, name), name
    assert (J.DOWNSAMPLE_POINT, J.DOWNSAMPLE_AVERAGE) == (0, 1)
    assert callable(J.Context.set_chroma_downsampling) and callable(J.Context.chroma_downsampling)
    # a null context is refused without a device
    lib.jpezy_ctx_set_chroma_downsampling.argtypes = [C.c_void_p, C.c_int]
    lib.jpezy_ctx_chroma_downsampling.argtypes = [C.c_void_p]
    assert lib.jpezy_ctx_set_chroma_downsampling(None, 1) == BADARG
    assert lib.jpezy_ctx_chroma_downsampling(None) == BADARG
