"""Region decode (include/jpezy_hip.h, REGION DECODE), as far as it can be checked without a GPU: jpezy_region_check against the scaled
size, the argument checks of the five entry points -- all of which come before the context is looked at, so they are made here with a
null context -- and what the header says.  tests/test_gpu_region.py holds the parity tests."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import scaled_model as M

ROOT = Path(__file__).resolve().parent.parent
E_BADARG = -1
SCALES = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _err(lib):
    return lib.jpezy_hip_last_error().decode()


@pytest.mark.parametrize("size", [(1, 1), (9, 17), (101, 70), (65535, 65535)])
def test_region_check_against_the_scaled_size(J, size):
    lib = J.load_library()
    W, H = size
    for scale in SCALES:
        ws, hs = M.scaled_size(W, H, scale)
        assert (ws, hs) == J.scaled_size(W, H, scale)
        inside = [(0, 0, ws, hs), (0, 0, 1, 1), (ws - 1, hs - 1, 1, 1), (0, hs - 1, ws, 1), (ws - 1, 0, 1, hs), (ws // 2, hs // 3, ws - ws // 2, hs - hs // 3)]
        outside = [(0, 0, ws + 1, hs), (0, 0, ws, hs + 1), (1, 0, ws, hs), (0, 1, ws, hs), (ws, 0, 1, 1), (0, hs, 1, 1), (-1, 0, 1, 1), (0, -1, 1, 1),
                   (0, 0, 0, 1), (0, 0, 1, 0), (0, 0, -2, 1), (2 ** 31 - 1, 0, 2 ** 31 - 1, 1), (0, 2 ** 31 - 1, 1, 2 ** 31 - 1)]
        for x, y, w, h in inside:
            assert lib.jpezy_region_check(W, H, scale, C.byref(J.Rect(x, y, w, h))) == 0, (size, scale, (x, y, w, h))
            J.region_check(W, H, scale, (x, y, w, h))
        for x, y, w, h in outside:
            assert lib.jpezy_region_check(W, H, scale, C.byref(J.Rect(x, y, w, h))) == E_BADARG, (size, scale, (x, y, w, h))
            msg = _err(lib)
            assert f"{w}x{h}+{x}+{y}" in msg, msg                       # the region is named ...
            if w >= 1 and h >= 1 and x >= 0 and y >= 0:
                assert f"{ws} x {hs}" in msg, msg                       # ... and so is the picture it had to lie in
            with pytest.raises(J.JpezyError, match="region"):
                J.region_check(W, H, scale, (x, y, w, h))


def test_region_check_other_arguments(J):
    lib = J.load_library()
    rect = J.Rect(0, 0, 1, 1)
    for bad in (0, 3, 16, -1):
        assert lib.jpezy_region_check(64, 64, bad, C.byref(rect)) == E_BADARG and "scale_denom" in _err(lib)
    for W, H in [(0, 5), (5, 0), (-1, 5)]:
        assert lib.jpezy_region_check(W, H, 2, C.byref(rect)) == E_BADARG and "width and height" in _err(lib)
    assert lib.jpezy_region_check(64, 64, 2, None) == E_BADARG and "null region" in _err(lib)


def test_every_entry_refuses_bad_arguments_before_the_context(J):
    """W x H = 40 x 24; every call has a NULL context and exactly one bad argument, which the message must name; with none bad the call
    gets as far as the context and says so"""
    lib = J.load_library()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    qt = ((C.c_uint16 * 64) * 4)()
    one = (C.c_uint8 * 3)(1, 1, 1)
    tq = (C.c_uint8 * 3)(0, 1, 1)
    info = J.FrameInfo()
    W, H = 40, 24
    good = J.Rect(3, 2, 5, 4)

    def planar_dev(scale=2, rect=good, stride=20, co=p, q=C.byref(qt), out=(p, p, p), nf=1, wh=(W, H)):
        return lib.jpezy_dequant_idct_region_dev(None, co, q, 3, C.byref(one), C.byref(one), C.byref(tq), 8, wh[0], wh[1], 0, scale,
                                                 C.byref(rect) if rect is not None else None, nf, stride, *out, None)

    def packed_dev(scale=2, rect=good, fmt=0, row=0, frame=0, co=p, pix=p, nf=1):
        return lib.jpezy_dequant_idct_region_packed_dev(None, co, C.byref(qt), 3, C.byref(one), C.byref(one), C.byref(tq), 8, W, H, 0, scale,
                                                        C.byref(rect) if rect is not None else None, fmt, row, frame, nf, pix, None)

    def planar_host(scale=2, rect=good, inf=info):
        return lib.jpezy_decode_jpeg_region(None, p, 64, 0, scale, C.byref(rect) if rect is not None else None,
                                            C.byref(inf) if inf is not None else None, p, p, p, 1024)

    def packed_host(scale=2, rect=good, fmt=0, row=0, inf=info):
        return lib.jpezy_decode_jpeg_region_packed(None, p, 64, 0, scale, C.byref(rect) if rect is not None else None,
                                                   C.byref(inf) if inf is not None else None, fmt, row, p, buf.size)

    ws, hs = M.scaled_size(W, H, 2)                                      # 20 x 12
    outside = J.Rect(ws - 4, 2, 5, 4)
    syntax = J.Rect(3, 2, 0, 4)
    cases = [
        # (call, what the message names)
        (lambda: planar_dev(), "context"), (lambda: packed_dev(), "context"), (lambda: planar_host(), "context"), (lambda: packed_host(), "context"),
        (lambda: planar_dev(scale=3), "scale_denom"), (lambda: packed_dev(scale=0), "scale_denom"),
        (lambda: planar_host(scale=16), "scale_denom"), (lambda: packed_host(scale=-2), "scale_denom"),
        (lambda: planar_dev(rect=outside), f"5x4+{ws - 4}+2"), (lambda: packed_dev(rect=outside), f"{ws} x {hs}"),
        (lambda: planar_dev(rect=syntax), "0x4+3+2"), (lambda: packed_dev(rect=syntax), "0x4+3+2"),
        (lambda: planar_host(rect=syntax), "0x4+3+2"), (lambda: packed_host(rect=syntax), "0x4+3+2"),
        (lambda: planar_dev(rect=None), "null pointer"), (lambda: packed_dev(rect=None), "null pointer"),
        (lambda: planar_host(rect=None), "null pointer"), (lambda: packed_host(rect=None), "null pointer"),
        (lambda: planar_host(inf=None), "null pointer"), (lambda: packed_host(inf=None), "null pointer"),
        (lambda: planar_dev(co=None), "null pointer"), (lambda: planar_dev(q=None), "null pointer"), (lambda: planar_dev(out=(p, None, p)), "null pointer"),
        (lambda: packed_dev(co=None), "null pointer"), (lambda: packed_dev(pix=None), "null pointer"),
        (lambda: planar_dev(stride=19), "plane_stride"), (lambda: planar_dev(nf=0), "n_frames"), (lambda: planar_dev(wh=(0, H)), "width/height"),
        (lambda: packed_dev(fmt=7), "pixel format"), (lambda: packed_host(fmt=-1), "pixel format"),
        (lambda: packed_dev(row=14), "row_stride"), (lambda: packed_host(row=14), "row_stride"),
        (lambda: packed_dev(fmt=2, row=20, frame=3 * 20 + 19), "frame_stride"),
        (lambda: planar_dev(co=C.c_void_p(buf.ctypes.data + 2)), "16-byte aligned"),
    ]
    for i, (call, names) in enumerate(cases):
        assert call() == E_BADARG, i
        assert names in _err(lib), (i, names, _err(lib))
    for name in ("dequant_idct_region_dev", "dequant_idct_region_packed_dev", "decode_jpeg_region", "decode_jpeg_region_packed"):
        call = {"dequant_idct_region_dev": planar_dev, "dequant_idct_region_packed_dev": packed_dev, "decode_jpeg_region": planar_host,
                "decode_jpeg_region_packed": packed_host}[name]
        assert call(scale=5) == E_BADARG and _err(lib).startswith(name + ":"), _err(lib)


def test_header_declares_the_region_section(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    assert "REGION DECODE" in text and "typedef struct jpezy_rect { int x, y, w, h; } jpezy_rect;" in text
    section = text[text.index("REGION DECODE"):text.index("PLANAR YCbCr 4:2:0 SAMPLES")]
    assert "NOT provided" in section and "no silent clipping" in section and "WHOLE scan is still Huffman-decoded" in section
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = ("jpezy_region_check", "jpezy_dequant_idct_region_dev", "jpezy_dequant_idct_region_packed_dev", "jpezy_decode_jpeg_region",
             "jpezy_decode_jpeg_region_packed")
    lib = J.load_library()
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in {n for n, _, _ in J.api.ABI}
    assert "region decode" in text[text.index("NOT provided in YCC form"):]
