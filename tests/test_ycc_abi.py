"""The planar YCbCr 4:2:0 part of the C-ABI, as far as it can be checked without a GPU: the two size helpers, c_step outside {1, 2}, and
the argument checks (strides, null pointers, null context) that come before any device is touched.  tests/test_gpu_ycc.py holds the parity tests."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import ycc_model as M

ROOT = Path(__file__).resolve().parent.parent
E_BADARG = -1


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def test_chroma_size(J):
    lib = J.load_library()
    for W, H in [(1, 1), (2, 2), (7, 5), (16, 16), (33, 16), (65535, 65535)]:
        cw, ch = C.c_int(-1), C.c_int(-1)
        assert lib.jpezy_ycc_chroma_size(W, H, C.byref(cw), C.byref(ch)) == 0
        assert (cw.value, ch.value) == ((W + 1) // 2, (H + 1) // 2) == M.chroma_size(W, H) == J.ycc_chroma_size(W, H)
    cw, ch = C.c_int(-1), C.c_int(-1)
    for W, H in [(0, 5), (5, 0), (-1, 5), (65536, 5)]:
        assert lib.jpezy_ycc_chroma_size(W, H, C.byref(cw), C.byref(ch)) == E_BADARG
    assert (cw.value, ch.value) == (-1, -1)
    assert lib.jpezy_ycc_chroma_size(9, 17, None, None) == 0
    with pytest.raises(J.JpezyError):
        J.ycc_chroma_size(0, 1)


def _info(J, W, H, comps):
    info = J.FrameInfo()
    info.width, info.height, info.ncomp, info.precision = W, H, len(comps), 8
    for i, (h, v) in enumerate(comps):
        info.H[i], info.V[i] = h, v
    info.hmax, info.vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    return info


@pytest.mark.parametrize("comps", [[(2, 2), (1, 1), (1, 1)], [(1, 1), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(4, 2), (2, 1), (2, 2)], [(1, 1)]])
def test_component_size(J, comps):
    lib = J.load_library()
    for W, H in [(1, 1), (37, 21), (64, 48), (101, 70)]:
        info = _info(J, W, H, comps)
        for c in range(len(comps)):
            w, h = C.c_int(-1), C.c_int(-1)
            assert lib.jpezy_ycc_component_size(C.byref(info), c, C.byref(w), C.byref(h)) == 0
            assert (w.value, h.value) == M.component_size(info, c) == J.ycc_component_size(info, c)
        for bad in (-1, len(comps), 3):
            assert lib.jpezy_ycc_component_size(C.byref(info), bad, None, None) == E_BADARG
    assert lib.jpezy_ycc_component_size(None, 0, None, None) == E_BADARG
    assert lib.jpezy_ycc_component_size(C.byref(J.FrameInfo()), 0, None, None) == E_BADARG      # not a parsed header


def _calls(J, c_step=1, ctx=None):
    lib = J.load_library()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    qt = ((C.c_uint16 * 64) * 4)()
    tq = (C.c_uint8 * 3)(0, 1, 1)
    info = J.FrameInfo()
    keep = (buf, qt, tq, info)
    return keep, {
        "fdct_quant_ycc_dev": lambda: lib.jpezy_fdct_quant_ycc_dev(ctx, p, 0, p, p, 0, c_step, 0, 0, 16, 16, 0, 1, p, None),
        "dequant_idct_ycc_dev": lambda: lib.jpezy_dequant_idct_ycc_dev(ctx, p, C.byref(qt), C.byref(tq), p, 0, p, p, 0, c_step, 0, 0, 16, 16, 1, None),
        "encode_jpeg_ycc": lambda: lib.jpezy_encode_jpeg_ycc(ctx, p, 0, p, p, 0, c_step, 16, 16, 0, b"", p, buf.size),
        "decode_jpeg_ycc": lambda: lib.jpezy_decode_jpeg_ycc(ctx, p, 64, C.byref(info), p, 0, 1024, p, p, 0, c_step, 1024),
    }


def test_null_context_is_refused_with_a_message(J):
    lib = J.load_library()
    keep, calls = _calls(J)
    for name, call in calls.items():
        rc = call()
        assert rc == E_BADARG, name
        msg = lib.jpezy_hip_last_error()
        assert b"context" in msg or b"argument" in msg, (name, msg)


def test_null_pointers_are_refused_with_a_message_before_the_context(J):
    """with a null context too: the pointer checks come first, so no device is touched"""
    lib = J.load_library()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    qt = ((C.c_uint16 * 64) * 4)()
    tq = (C.c_uint8 * 3)(0, 1, 1)
    info = J.FrameInfo()
    N = None
    calls = {
        "fdct y": lambda: lib.jpezy_fdct_quant_ycc_dev(N, N, 0, p, p, 0, 1, 0, 0, 16, 16, 0, 1, p, N),
        "fdct cb": lambda: lib.jpezy_fdct_quant_ycc_dev(N, p, 0, N, p, 0, 1, 0, 0, 16, 16, 0, 1, p, N),
        "fdct cr": lambda: lib.jpezy_fdct_quant_ycc_dev(N, p, 0, p, N, 0, 1, 0, 0, 16, 16, 0, 1, p, N),
        "fdct coeffs": lambda: lib.jpezy_fdct_quant_ycc_dev(N, p, 0, p, p, 0, 1, 0, 0, 16, 16, 0, 1, N, N),
        "fdct gray y": lambda: lib.jpezy_fdct_quant_ycc_dev(N, N, 0, N, N, 0, 1, 0, 0, 16, 16, 1, 1, p, N),
        "idct coeffs": lambda: lib.jpezy_dequant_idct_ycc_dev(N, N, C.byref(qt), C.byref(tq), p, 0, p, p, 0, 1, 0, 0, 16, 16, 1, N),
        "idct qt": lambda: lib.jpezy_dequant_idct_ycc_dev(N, p, N, C.byref(tq), p, 0, p, p, 0, 1, 0, 0, 16, 16, 1, N),
        "idct tq": lambda: lib.jpezy_dequant_idct_ycc_dev(N, p, C.byref(qt), N, p, 0, p, p, 0, 1, 0, 0, 16, 16, 1, N),
        "idct y": lambda: lib.jpezy_dequant_idct_ycc_dev(N, p, C.byref(qt), C.byref(tq), N, 0, p, p, 0, 1, 0, 0, 16, 16, 1, N),
        "encode y": lambda: lib.jpezy_encode_jpeg_ycc(N, N, 0, p, p, 0, 1, 16, 16, 0, b"", p, buf.size),
        "encode cb": lambda: lib.jpezy_encode_jpeg_ycc(N, p, 0, N, p, 0, 1, 16, 16, 0, b"", p, buf.size),
        "encode out": lambda: lib.jpezy_encode_jpeg_ycc(N, p, 0, p, p, 0, 1, 16, 16, 0, b"", N, buf.size),
        "decode data": lambda: lib.jpezy_decode_jpeg_ycc(N, N, 64, C.byref(info), p, 0, 1024, p, p, 0, 1, 1024),
        "decode info": lambda: lib.jpezy_decode_jpeg_ycc(N, p, 64, N, p, 0, 1024, p, p, 0, 1, 1024),
        "decode chroma without y": lambda: lib.jpezy_decode_jpeg_ycc(N, p, 64, C.byref(info), N, 0, 0, p, p, 0, 1, 1024),
    }
    for name, call in calls.items():
        assert call() == E_BADARG, name
        msg = lib.jpezy_hip_last_error()
        assert b"null" in msg and b"context" not in msg, (name, msg)
    # gray encode: the chroma pointers may be null -- the call gets as far as the context
    assert lib.jpezy_fdct_quant_ycc_dev(N, p, 0, N, N, 0, 1, 0, 0, 16, 16, 1, 1, p, N) == E_BADARG
    assert b"context" in lib.jpezy_hip_last_error()


@pytest.mark.parametrize("c_step", [0, 3, -1, 4])
def test_c_step_outside_1_2_is_refused(J, c_step):
    lib = J.load_library()
    keep, calls = _calls(J, c_step)
    for name, call in calls.items():
        assert call() == E_BADARG, name
        assert b"c_step" in lib.jpezy_hip_last_error(), (name, lib.jpezy_hip_last_error())


def test_strides_are_checked_before_the_context(J):
    lib = J.load_library()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    for args, word in [((15, p, p, 0, 1, 0, 0), b"y_stride"), ((0, p, p, 7, 1, 0, 0), b"c_stride"), ((0, p, p, 14, 2, 0, 0), b"c_stride"),
                       ((1 << 31, p, p, 0, 1, 0, 0), b"32 bits"), ((0, p, p, 0, 1, 255, 0), b"y_frame_stride"), ((0, p, p, 0, 1, 0, 63), b"c_frame_stride")]:
        assert lib.jpezy_fdct_quant_ycc_dev(None, p, *args, 16, 16, 0, 1, p, None) == E_BADARG
        assert word in lib.jpezy_hip_last_error(), (args, lib.jpezy_hip_last_error())
    for W, H in [(0, 16), (16, 0), (65536, 16)]:
        assert lib.jpezy_fdct_quant_ycc_dev(None, p, 0, p, p, 0, 1, 0, 0, W, H, 0, 1, p, None) == E_BADARG


def test_header_declares_the_entry_points():
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("jpezy_ycc_chroma_size", "jpezy_ycc_component_size", "jpezy_fdct_quant_ycc_dev", "jpezy_dequant_idct_ycc_dev",
                 "jpezy_encode_jpeg_ycc", "jpezy_decode_jpeg_ycc"):
        assert re.search(r"\b" + name + r"\s*\(", code), name
    assert "PLANAR YCbCr 4:2:0" in text and "NOT provided in YCC form" in text
