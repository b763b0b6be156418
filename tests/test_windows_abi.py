"""Batch of windows (include/jpezy_hip.h, BATCH OF WINDOWS), as far as it can be checked without a GPU: what the header says and the
library exports, jpezy_window_fit against a Python restatement of the definition, and every refusal jpezy_decode_windows_dev makes before
it looks at the context -- made here with a null context, including which of two bad arguments is named.  tests/test_gpu_windows.py holds
the parity tests."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import scaled_model as M

ROOT = Path(__file__).resolve().parent.parent
E_BADARG, E_NOSPACE = -1, -6
SCALES = (1, 2, 4, 8)
BYTES = {0: 3, 1: 3, 2: 4, 3: 4}                                   # JPEZY_PIX_*


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _err(lib):
    return lib.jpezy_hip_last_error().decode()


def fit_model(W, H, win, fmt, row, slot):
    """the header's definition: (status, placed or None)"""
    (x, y, w, h), scale = win
    if fmt not in BYTES or W <= 0 or H <= 0 or scale not in SCALES:
        return E_BADARG, None
    ws, hs = M.scaled_size(W, H, scale)
    if w == 0 and h == 0:
        x, y, w, h = 0, 0, ws, hs
    if w < 1 or h < 1 or x < 0 or y < 0 or x + w > ws or y + h > hs:
        return E_BADARG, None
    nb = BYTES[fmt]
    if w * nb > row or (h - 1) * row + w * nb > slot:
        return E_NOSPACE, (x, y, w, h)
    return 0, (x, y, w, h)


def c_fit(J, W, H, win, fmt, row, slot):
    placed = J.Rect(-7, -7, -7, -7)
    w = J.Window(J.Rect(*win[0]), win[1])
    rc = J.load_library().jpezy_window_fit(W, H, C.byref(w), fmt, row, slot, C.byref(placed))
    return rc, (placed.x, placed.y, placed.w, placed.h)


def test_header_declares_the_section_and_the_library_exports_it(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    assert "BATCH OF WINDOWS" in text and "typedef struct jpezy_window { jpezy_rect region; int scale_denom; } jpezy_window;" in text
    section = text[text.index(" * BATCH OF WINDOWS"):text.index("PLANAR YCbCr 4:2:0 SAMPLES")]
    for phrase in ("jpezy_decode_jpeg_region_packed", "Bytes touched", "NOT provided", "slot_stride", "stream capture", "fallback counter"):
        assert phrase in section, phrase
    region = text[text.index(" * REGION DECODE"):text.index(" * BATCH OF WINDOWS")]
    assert "BATCH OF WINDOWS" in region[region.index("NOT provided"):]           # the region section points here
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = J.load_library()
    for name in ("jpezy_window_fit", "jpezy_decode_windows_dev", "jpezy_ctx_set_windows_slice_files"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in {n for n, _, _ in J.api.ABI}
    assert C.sizeof(J.Window) == 20


@pytest.mark.parametrize("size", [(1, 1), (17, 9), (101, 70), (65535, 65535)])
def test_window_fit_resolves_the_whole_picture_at_each_scale(J, size):
    W, H = size
    for scale in SCALES:
        ws, hs = M.scaled_size(W, H, scale)
        for fmt in (0, 3):
            nb = BYTES[fmt]
            for xy in ((0, 0), (5, 3)):                                      # x, y are not looked at in the whole-picture form
                rc, placed = c_fit(J, W, H, ((xy[0], xy[1], 0, 0), scale), fmt, ws * nb, hs * ws * nb)
                assert (rc, placed) == (0, (0, 0, ws, hs)), (size, scale, fmt)
                assert fit_model(W, H, ((xy[0], xy[1], 0, 0), scale), fmt, ws * nb, hs * ws * nb) == (0, (0, 0, ws, hs))
        # a null window: the whole picture at full size
        placed = J.Rect()
        assert J.load_library().jpezy_window_fit(W, H, None, 0, W * 3, H * W * 3, C.byref(placed)) == 0
        assert (placed.x, placed.y, placed.w, placed.h) == (0, 0, W, H)
    assert J.window_fit(W, H, None, J.PIX_RGBA32, W * 4, W * H * 4) == (0, 0, W, H)
    assert J.window_fit(W, H, ((0, 0, 1, 1), 8), J.PIX_RGB24, 3, 3) == (0, 0, 1, 1)


def test_window_fit_against_the_restatement(J):
    W, H = 101, 70
    n = 0
    for scale in SCALES + (0, 3, 16):
        ws, hs = M.scaled_size(W, H, scale) if scale in SCALES else (W, H)
        regions = [(0, 0, ws, hs), (0, 0, 1, 1), (ws - 1, hs - 1, 1, 1), (3, 2, 5, 4), (1, 0, ws, hs), (0, 1, ws, hs), (ws, 0, 1, 1), (0, hs, 1, 1),
                   (-1, 0, 1, 1), (0, -1, 2, 2), (0, 0, 0, 1), (0, 0, 1, 0), (0, 0, -2, 1), (0, 0, ws + 1, 1), (2 ** 31 - 1, 0, 2 ** 31 - 1, 1)]
        for reg in regions:
            for fmt in (0, 2, 4, -1):
                nb = BYTES.get(fmt, 3)
                w, h = max(reg[2], 1), max(reg[3], 1)
                for row, slot in ((w * nb, h * w * nb), (w * nb + 7, (h - 1) * (w * nb + 7) + w * nb), (1 << 20, 1 << 30)):
                    want = fit_model(W, H, (reg, scale), fmt, row, slot)
                    rc, placed = c_fit(J, W, H, (reg, scale), fmt, row, slot)
                    assert rc == want[0], (reg, scale, fmt, row, slot, _err(J.load_library()))
                    assert placed == (want[1] if want[1] is not None else (-7, -7, -7, -7)), (reg, scale, fmt)
                    n += 1
    assert n > 500
    lib = J.load_library()
    one = J.Window(J.Rect(0, 0, 1, 1), 1)
    for bad in [(0, 5), (5, 0), (-1, 5)]:
        assert lib.jpezy_window_fit(bad[0], bad[1], C.byref(one), 0, 64, 64, None) == E_BADARG and "width and height" in _err(lib)
    assert lib.jpezy_window_fit(8, 8, C.byref(J.Window(J.Rect(0, 0, 1, 1), 3)), 0, 64, 64, None) == E_BADARG and "scale_denom" in _err(lib)
    assert lib.jpezy_window_fit(8, 8, C.byref(one), 9, 64, 64, None) == E_BADARG and "pixel format" in _err(lib)
    assert lib.jpezy_window_fit(8, 8, C.byref(J.Window(J.Rect(6, 0, 3, 1), 1)), 0, 64, 64, None) == E_BADARG
    assert "3x1+6+0" in _err(lib) and "8 x 8" in _err(lib)                        # the region and the picture it had to lie in
    assert lib.jpezy_window_fit(8, 8, C.byref(one), 0, 64, 64, None) == 0          # placed may be null
    with pytest.raises(J.JpezyError, match="outside the picture"):
        J.window_fit(8, 8, (6, 0, 3, 1), J.PIX_RGB24, 64, 64)
    with pytest.raises(J.JpezyError, match="does not fit"):
        J.window_fit(8, 8, (0, 0, 3, 2), J.PIX_RGB24, 8, 64)


@pytest.mark.parametrize("fmt", [0, 3])
def test_both_fit_inequalities_at_equality_and_one_byte_short(J, fmt):
    nb = BYTES[fmt]
    W, H = 40, 24
    for win in (((3, 2, 5, 4), 2), ((0, 0, 0, 0), 4), ((39, 23, 1, 1), 1), ((0, 0, 40, 1), 1)):
        _, (x, y, w, h) = c_fit(J, W, H, win, fmt, 1 << 20, 1 << 30)
        tight = w * nb
        for row in (tight, tight + 5):
            need = (h - 1) * row + tight
            assert c_fit(J, W, H, win, fmt, row, need) == (0, (x, y, w, h))                     # both at equality (row == tight) / the slot at equality
            assert c_fit(J, W, H, win, fmt, row, need - 1) == (E_NOSPACE, (x, y, w, h))         # the slot one byte short
            assert "does not fit" in _err(J.load_library())
        assert c_fit(J, W, H, win, fmt, tight - 1, 1 << 30) == (E_NOSPACE, (x, y, w, h))        # the row one byte short
        assert fit_model(W, H, win, fmt, tight - 1, 1 << 30)[0] == E_NOSPACE and fit_model(W, H, win, fmt, tight, (h - 1) * tight + tight)[0] == 0


def test_the_entry_refuses_bad_arguments_before_the_context(J):
    """every call has a NULL context; with nothing bad the call gets as far as the context and says so"""
    lib = J.load_library()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    n = 2
    data = (C.c_void_p * n)(buf.ctypes.data, buf.ctypes.data)
    lens = (C.c_size_t * n)(64, 64)
    infos, placed, status = (J.FrameInfo * n)(), (J.Rect * n)(), (C.c_int * n)()
    wins = (J.Window * n)(J.Window(J.Rect(0, 0, 4, 4), 1), J.Window(J.Rect(0, 0, 0, 0), 2))

    def call(n=n, data=data, lens=lens, wins=wins, fmt=0, row=16, slot=64, pix=p, cap=4096, infos=infos, placed=placed, status=status):
        return lib.jpezy_decode_windows_dev(None, n, data, lens, 0, wins, fmt, row, slot, pix, cap, infos, placed, status)

    assert call() == E_BADARG and "null context" in _err(lib)
    assert call(wins=None, placed=None) == E_BADARG and "null context" in _err(lib)          # both arrays may be null
    assert call(cap=n * 64) == E_BADARG and "null context" in _err(lib)                      # n * slot_stride == pix_cap
    assert call(n=0, data=None, lens=None, infos=None, status=None, pix=None, fmt=9, row=0) == 0      # n == 0: nothing is looked at
    cases = [
        (dict(n=-1), E_BADARG, "n must not be negative"),
        (dict(data=None), E_BADARG, "null pointer"), (dict(lens=None), E_BADARG, "null pointer"), (dict(infos=None), E_BADARG, "null pointer"),
        (dict(status=None), E_BADARG, "null pointer"), (dict(pix=None), E_BADARG, "null pointer"),
        (dict(fmt=4), E_BADARG, "pixel format"), (dict(fmt=-1), E_BADARG, "pixel format"),
        (dict(row=0), E_BADARG, "row_stride and slot_stride"), (dict(slot=0), E_BADARG, "row_stride and slot_stride"),
        (dict(row=1 << 32), E_BADARG, "32 bits"),
        (dict(cap=n * 64 - 1), E_NOSPACE, "pix_cap"), (dict(slot=(1 << 63) + 5, cap=4096), E_NOSPACE, "pix_cap"),
        # which of two bad arguments is named: the order is n, arrays, format, strides, capacity
        (dict(n=-1, data=None), E_BADARG, "n must not be negative"),
        (dict(data=None, fmt=9), E_BADARG, "null pointer"),
        (dict(fmt=9, row=0), E_BADARG, "pixel format"),
        (dict(row=0, cap=1), E_BADARG, "row_stride and slot_stride"),
        (dict(row=1 << 32, cap=1), E_BADARG, "32 bits"),
        (dict(status=None, cap=1), E_BADARG, "null pointer"),
    ]
    for i, (kw, code, names) in enumerate(cases):
        assert call(**kw) == code, (i, kw)
        msg = _err(lib)
        assert names in msg and msg.startswith("decode_windows_dev:"), (i, kw, msg)
    assert (np.frombuffer(buf, np.uint8) == 0).all()
    assert lib.jpezy_ctx_set_windows_slice_files(None, 2) == E_BADARG and "null context" in _err(lib)
