"""Reduced-size decode, as far as it can be checked without a GPU: the numpy restatement of its definition (tests/scaled_model.py)
against the oracle at full size, its normalisation and orientation against box means of the full-size picture, the size helper, and
the argument checks of the new entry points that come before any device is touched.  tests/test_gpu_scaled.py holds the parity tests."""
import ctypes as C

import numpy as np
import pytest

import scaled_model as M
from jpeg_synth import synth_jpeg
from test_host_codec import ODD_LAYOUTS

E_BADARG = -1
L420 = [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]
ANCHOR_LAYOUTS = {"own": L420, **{k: ODD_LAYOUTS[k] for k in ("h3_partial", "h4v2_partial", "one_comp_2x2")}}


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("layout", sorted(ANCHOR_LAYOUTS))
def test_model_at_full_size_is_the_oracle(oracle, layout, gray):
    data, _, _ = synth_jpeg(37, 21, ANCHOR_LAYOUTS[layout], seed=3)
    info, co = oracle.read_jpeg(data)
    want = oracle.decode_planes(co, info, gray)
    got = M.decode_planes(co, info, 1, gray)
    for a, e in zip(got, want):
        assert np.array_equal(a, e)


@pytest.mark.parametrize("scale", [2, 4, 8])
def test_luma_normalisation_and_orientation(oracle, scale):
    """a smooth asymmetric picture: the reduced luma stays within one of the s x s box mean of the full-size luma (measured 0.5 /
    0.5625 / 0.5 for n = 4 / 2 / 1; at n = 1 both are truncations of the same mean, so < 1 is a theorem).  A transposed or
    mis-normalised transform misses by tens."""
    W, H = 64, 48
    y, x = np.mgrid[:H, :W]
    r, g, b = 60 + 2 * x, 60 + 3 * y, 60 + x + y
    data = oracle.encode_jpeg(r.astype(np.uint8), g.astype(np.uint8), b.astype(np.uint8), W, H)
    info, co = oracle.read_jpeg(data)
    full = oracle.decode_planes(co, info, True)[0].reshape(H, W).astype(np.float64)
    box = full.reshape(H // scale, scale, W // scale, scale).mean(axis=(1, 3))
    got = M.decode_planes(co, info, scale, True)[0].reshape(H // scale, W // scale).astype(np.float64)
    d = float(np.abs(got - box).max())
    print(f"scale {scale}: max |model - box mean| = {d}")
    assert d <= 1.0


def test_model_ref_int():
    x = [0.0, -0.9, 2.0 ** 31 - 0.5, 2.0 ** 31, -2.0 ** 31, -2.0 ** 31 - 1, 1.5e10, float("nan"), float("inf")]
    assert M.ref_int(x).tolist() == [0, 0, 2 ** 31 - 1, M.INT_MIN, M.INT_MIN, M.INT_MIN, M.INT_MIN, M.INT_MIN, M.INT_MIN]


def test_scaled_size(J):
    lib = J.load_library()
    for W, H in [(1, 1), (8, 8), (9, 17), (65535, 65535)]:
        for scale in (1, 2, 4, 8):
            n = 8 // scale
            ws, hs = C.c_int(-1), C.c_int(-1)
            assert lib.jpezy_scaled_size(W, H, scale, C.byref(ws), C.byref(hs)) == 0
            assert (ws.value, hs.value) == (-(-W * n // 8), -(-H * n // 8)) == M.scaled_size(W, H, scale) == J.scaled_size(W, H, scale)
    ws, hs = C.c_int(-1), C.c_int(-1)
    for bad in (0, 3, 16, -1):
        assert lib.jpezy_scaled_size(64, 64, bad, C.byref(ws), C.byref(hs)) == E_BADARG
        assert b"scale_denom" in lib.jpezy_hip_last_error()
    for W, H in [(0, 5), (5, 0), (-1, 5)]:
        assert lib.jpezy_scaled_size(W, H, 2, C.byref(ws), C.byref(hs)) == E_BADARG
    assert (ws.value, hs.value) == (-1, -1)
    assert lib.jpezy_scaled_size(9, 17, 4, None, None) == 0
    with pytest.raises(J.JpezyError):
        J.scaled_size(64, 64, 3)


def test_null_context_is_refused_with_a_message(J):
    lib = J.load_library()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    qt = ((C.c_uint16 * 64) * 4)()
    one = (C.c_uint8 * 3)(1, 1, 1)
    tq = (C.c_uint8 * 3)(0, 1, 1)
    info = J.FrameInfo()
    for scale in (1, 2, 4, 8):
        calls = {
            "dequant_idct_scaled_dev": lambda: lib.jpezy_dequant_idct_scaled_dev(None, p, C.byref(qt), 3, C.byref(one), C.byref(one), C.byref(tq), 8, 16, 16,
                                                                                 0, scale, 1, 256, p, p, p, None),
            "dequant_idct_scaled_packed_dev": lambda: lib.jpezy_dequant_idct_scaled_packed_dev(None, p, C.byref(qt), 3, C.byref(one), C.byref(one),
                                                                                               C.byref(tq), 8, 16, 16, 0, scale, 0, 0, 0, 1, p, None),
            "decode_jpeg_scaled": lambda: lib.jpezy_decode_jpeg_scaled(None, p, 64, 0, scale, C.byref(info), p, p, p, 1024),
            "decode_jpeg_scaled_packed": lambda: lib.jpezy_decode_jpeg_scaled_packed(None, p, 64, 0, scale, C.byref(info), 0, 0, p, buf.size),
        }
        for name, call in calls.items():
            rc = call()
            assert rc == E_BADARG, (name, scale)
            msg = lib.jpezy_hip_last_error()
            assert b"context" in msg or b"argument" in msg, (name, scale, msg)
