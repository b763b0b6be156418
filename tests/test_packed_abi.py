"""The packed-pixel (interleaved RGB / BGR / RGBA / BGRA) part of the C-ABI, as far as it can be checked without a GPU: the format
helper, the agreement of the header's enum with the Python constants, and the argument checks that come before any device is touched.
tests/test_gpu_packed.py holds the parity tests."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
E_BADARG = -1


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def test_pixel_bytes(J):
    lib = J.load_library()
    assert [lib.jpezy_pixel_bytes(f) for f in range(4)] == [3, 3, 4, 4]
    assert lib.jpezy_pixel_bytes(-1) == E_BADARG and lib.jpezy_pixel_bytes(4) == E_BADARG


def test_header_enum_equals_python_constants(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    body = re.search(r"enum\s+jpezy_pixel_format\s*\{([^}]*)\}", text).group(1)
    enum = {k: int(v) for k, v in re.findall(r"JPEZY_(PIX_\w+)\s*=\s*(\d+)", body)}
    assert enum == {"PIX_RGB24": J.PIX_RGB24, "PIX_BGR24": J.PIX_BGR24, "PIX_RGBA32": J.PIX_RGBA32, "PIX_BGRA32": J.PIX_BGRA32}
    assert sorted(enum.values()) == [0, 1, 2, 3]
    from jpezy_amd import api
    assert (api.PIX_RGB24, api.PIX_BGR24, api.PIX_RGBA32, api.PIX_BGRA32) == (0, 1, 2, 3)


def test_null_context_is_refused_with_a_message(J):
    lib = J.load_library()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    qt = ((C.c_uint16 * 64) * 4)()
    tq = (C.c_uint8 * 3)(0, 1, 1)
    info = J.FrameInfo()
    calls = {
        "fdct_quant_packed_dev": lambda: lib.jpezy_fdct_quant_packed_dev(None, p, 0, 0, 0, 16, 16, 0, 1, p, None),
        "dequant_idct_packed_dev": lambda: lib.jpezy_dequant_idct_packed_dev(None, p, C.byref(qt), C.byref(tq), 0, 0, 0, 16, 16, 0, 1, p, None),
        "encode_jpeg_packed": lambda: lib.jpezy_encode_jpeg_packed(None, p, 0, 0, 16, 16, 0, b"", p, buf.size),
        "decode_jpeg_packed": lambda: lib.jpezy_decode_jpeg_packed(None, p, 64, 0, C.byref(info), 0, 0, p, buf.size),
    }
    for name, call in calls.items():
        rc = call()
        assert rc < 0, name
        msg = lib.jpezy_hip_last_error()
        assert b"context" in msg or b"argument" in msg, (name, msg)
