"""Smooth upsampling of windows (include/jpezy_hip.h, SMOOTH UPSAMPLING OF WINDOWS), as far as it can be checked without a GPU: what the
header says and the library exports, and every refusal the new entries make before they look at the context -- made here with bare ctypes
and a null context, including which of two bad arguments is named.  tests/test_gpu_region_smooth.py and tests/test_gpu_windows_smooth.py
hold the parity tests."""
import ctypes as C
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
E_BADARG, E_UNSUPPORTED = -1, -4
NEAREST, SMOOTH = 0, 1


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _err(lib):
    return lib.jpezy_hip_last_error().decode()


NEW = ("jpezy_dequant_idct_region_upsampling_dev", "jpezy_dequant_idct_region_upsampling_packed_dev", "jpezy_decode_jpeg_region_upsampling",
       "jpezy_decode_jpeg_region_upsampling_packed", "jpezy_ctx_set_windows_upsampling", "jpezy_ctx_windows_upsampling")


def test_header_declares_the_section_and_the_library_exports_it(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    section = text[text.index(" * SMOOTH UPSAMPLING OF WINDOWS"):]
    for phrase in ("ceil(Ws / fx) x ceil(Hs / fy)", "NO OUTSIDE REFERENCE EXISTS", "DCT_scaled_size", "NOT provided", "8-bit", "jpezy_region_check"):
        assert phrase in section, phrase
    upsampling = text[text.index(" * CHROMA UPSAMPLING"):text.index(" * SMOOTH UPSAMPLING OF WINDOWS")]
    assert "smooth with reduced-size or region decode" not in upsampling          # the gap this section closes
    # the four region entries are declared in a header of their own that jpezy_hip.h includes; the two context functions in jpezy_hip.h
    assert '#include "jpezy_hip_region_upsampling.h"' in section
    part = (ROOT / "include" / "jpezy_hip_region_upsampling.h").read_text()
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    lib = J.load_library()
    bound = {n for n, _, _ in J.api.ABI + J.api.ABI_REGION_UPSAMPLING}
    for name in NEW:
        code = strip(text if name.startswith("jpezy_ctx_") else part)
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in bound and getattr(lib, name).argtypes is not None


# ---- the device entries: (entry with upsampling, entry without, the arguments behind `region`) ---------------------------------------
QT = (C.c_uint16 * 256)(*([16] * 256))
HS, VS, TQ = (C.c_uint8 * 3)(2, 1, 1), (C.c_uint8 * 3)(2, 1, 1), (C.c_uint8 * 3)(0, 1, 1)
COEF = C.c_void_p(0x1000)          # never dereferenced: a null context is refused before any device work
PIX = C.c_void_p(0x2000)


def planar(lib, up, precision=8, W=64, H=48, scale=1, region=(0, 0, 8, 8), n_frames=1, stride=64, coef=COEF, dst=PIX, ctx=None):
    r = (C.c_int * 4)(*region) if region is not None else None
    head = (ctx, coef, QT, 3, HS, VS, TQ, precision, W, H, 0)
    tail = (scale, r, n_frames, C.c_size_t(stride), dst, dst, dst, None)
    if up is None:
        return lib.jpezy_dequant_idct_region_dev(*head, *tail)
    return lib.jpezy_dequant_idct_region_upsampling_dev(*head, up, *tail)


def packed(lib, up, precision=8, W=64, H=48, scale=1, region=(0, 0, 8, 8), fmt=0, row=0, frame=0, n_frames=1, coef=COEF, dst=PIX, ctx=None):
    r = (C.c_int * 4)(*region) if region is not None else None
    head = (ctx, coef, QT, 3, HS, VS, TQ, precision, W, H, 0)
    tail = (scale, r, fmt, C.c_size_t(row), C.c_size_t(frame), n_frames, dst, None)
    if up is None:
        return lib.jpezy_dequant_idct_region_packed_dev(*head, *tail)
    return lib.jpezy_dequant_idct_region_upsampling_packed_dev(*head, up, *tail)


@pytest.mark.parametrize("entry", [planar, packed], ids=["planes", "packed"])
def test_bad_upsampling_is_named_before_anything_else(J, entry):
    lib = J.load_library()
    for up in (2, -1, 255):
        # every other argument bad too: upsampling is the one that is named, and the (null) context is never reached
        assert entry(lib, up, W=0, scale=3, region=None, coef=None, dst=None) == E_BADARG
        assert "upsampling must be" in _err(lib)


@pytest.mark.parametrize("entry", [planar, packed], ids=["planes", "packed"])
def test_twelve_bit_is_unsupported(J, entry):
    lib = J.load_library()
    assert entry(lib, SMOOTH, precision=12) == E_UNSUPPORTED
    assert "8-bit" in _err(lib)
    assert entry(lib, SMOOTH, precision=12, W=0, region=None) == E_UNSUPPORTED     # before the region entry's own checks
    # nearest: the region entry's verdict (it decodes 12-bit files: here it gets as far as the null context)
    assert entry(lib, NEAREST, precision=12) == E_BADARG and _err(lib) == "null context"


BAD = [dict(coef=None), dict(dst=None), dict(region=None), dict(W=0), dict(H=70000), dict(n_frames=0), dict(scale=3), dict(region=(0, 0, 0, 8)),
       dict(region=(-1, 0, 8, 8)), dict(region=(60, 0, 8, 8)), dict(scale=8, region=(0, 0, 9, 6)), dict(coef=C.c_void_p(0x1002)), dict(),
       dict(coef=None, scale=3), dict(scale=3, region=(60, 0, 8, 8)), dict(W=0, n_frames=0)]


@pytest.mark.parametrize("entry,extra", [(planar, [dict(stride=63), dict(stride=63, coef=C.c_void_p(0x1002))]),
                                         (packed, [dict(fmt=9), dict(row=23), dict(fmt=2, row=30), dict(frame=8), dict(fmt=9, coef=C.c_void_p(0x1002))])],
                         ids=["planes", "packed"])
def test_both_modes_reproduce_the_region_entrys_verdicts(J, entry, extra):
    """the argument checks are the region entry's, in its order: the same status and -- but for the entry's name -- the same message, for
    nearest (handed over) and for smooth (its own copy of the checks)"""
    lib = J.load_library()
    strip = lambda m: re.sub(r"^dequant_idct_region(_upsampling)?(_packed)?_dev: ", "", m)
    for kw in BAD + extra:
        want = entry(lib, None, **kw), _err(lib)
        assert want[0] == E_BADARG, kw
        got_n = entry(lib, NEAREST, **kw), _err(lib)
        assert got_n == want, kw
        got_s = entry(lib, SMOOTH, **kw), _err(lib)
        assert (got_s[0], strip(got_s[1])) == (want[0], strip(want[1])), kw


def test_file_entries(J):
    lib = J.load_library()
    data = np.zeros(16, np.uint8)
    info = J.FrameInfo()
    rect = (C.c_int * 4)(0, 0, 4, 4)
    dst = np.zeros(64, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def planes(up, scale=1, r=rect, i=info):
        a = (None, p(data), data.size, 0)
        b = (scale, r, C.byref(i) if i is not None else None, p(dst), p(dst), p(dst), 16)
        return lib.jpezy_decode_jpeg_region(*a, *b) if up is None else lib.jpezy_decode_jpeg_region_upsampling(*a, up, *b)

    def pk(up, scale=1, r=rect, i=info, fmt=0, row=0):
        a = (None, p(data), data.size, 0)
        b = (scale, r, C.byref(i) if i is not None else None, fmt, C.c_size_t(row), p(dst), 64)
        return lib.jpezy_decode_jpeg_region_packed(*a, *b) if up is None else lib.jpezy_decode_jpeg_region_upsampling_packed(*a, up, *b)

    strip = lambda m: re.sub(r"^decode_jpeg_region(_upsampling)?(_packed)?: ", "", m)
    for entry, more in ((planes, []), (pk, [dict(fmt=7), dict(row=5)])):
        assert entry(5, scale=3, r=None, i=None) == E_BADARG and "upsampling must be" in _err(lib)
        for kw in [dict(), dict(scale=3), dict(r=None), dict(i=None), dict(r=(C.c_int * 4)(0, 0, 0, 4)), dict(r=(C.c_int * 4)(-1, 0, 4, 4))] + more:
            want = entry(None, **kw), _err(lib)
            assert want[0] == E_BADARG
            assert (entry(NEAREST, **kw), _err(lib)) == want, kw
            got = entry(SMOOTH, **kw), _err(lib)
            assert (got[0], strip(got[1])) == (want[0], strip(want[1])), kw


def test_windows_setting_with_a_null_context(J):
    lib = J.load_library()
    assert lib.jpezy_ctx_set_windows_upsampling(None, 2) == E_BADARG and "upsampling must be" in _err(lib)
    assert lib.jpezy_ctx_set_windows_upsampling(None, SMOOTH) == E_BADARG and _err(lib) == "null context"
    assert lib.jpezy_ctx_set_windows_upsampling(None, NEAREST) == E_BADARG and _err(lib) == "null context"
    assert lib.jpezy_ctx_windows_upsampling(None) == E_BADARG and _err(lib) == "null context"


def test_python_keywords_exist(J):
    sig = lambda f: inspect.signature(f).parameters
    for f in (J.Context.decode_jpeg_region, J.Context.decode_jpeg_region_packed, J.Context.dequant_idct_region_dev):
        assert sig(f)["upsampling"].default == J.UPSAMPLE_NEAREST, f.__name__
    for f in (J.Context.decode_windows_dev, J.Context.decode_windows_resized_dev):
        assert sig(f)["upsampling"].default is None, f.__name__
    assert callable(J.Context.set_windows_upsampling) and callable(J.Context.windows_upsampling)
    assert (J.UPSAMPLE_NEAREST, J.UPSAMPLE_SMOOTH) == (NEAREST, SMOOTH)
