"""Batch of windows, resized (include/jpezy_hip.h, BATCH OF WINDOWS, RESIZED), as far as it can be checked without a GPU: what the header says
and the library exports; jpezy_resize_taps -- the arithmetic's only floating-point part -- against tests/resize_model.py; that restatement
against Pillow's BILINEAR resize as an independent anchor; jpezy_resize_pick_window against a few-line restatement; and every refusal
jpezy_decode_windows_resized_dev makes before it looks at the context, made here with a null context, including which of two bad arguments
is named.  tests/test_gpu_windows_resized.py holds the parity tests.  Every comparison is exact."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import resize_model as RM
import scaled_model as M

ROOT = Path(__file__).resolve().parent.parent
E_BADARG, E_NOSPACE = -1, -6
NAMES = ("jpezy_resize_taps", "jpezy_resize_pick_window", "jpezy_decode_windows_resized_dev")


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _err(lib):
    return lib.jpezy_hip_last_error().decode()


def test_header_declares_the_section_and_the_library_exports_it(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    section = text[text.index(" * BATCH OF WINDOWS, RESIZED"):text.index("PLANAR YCbCr 4:2:0 SAMPLES")]
    for phrase in ("Weights", "Passes", "2^22", "Mirror", "Identity", "Bytes touched", "NOT provided", "cannot overflow", "255 * (2^22 + 65536) + 2^21 < 2^31",
                   "jpezy_decode_jpeg_region_packed", "less than s full-size", "stream capture"):
        assert phrase in section, phrase
    not_provided = section[section.index("NOT provided"):section.index("*/")]
    for phrase in ("float or planar", "nearest, bicubic", "per-file output size", "vertical", "host-memory", "smooth chroma upsampling"):
        assert phrase in not_provided, phrase
    windows = text[text.index(" * BATCH OF WINDOWS"):text.index(" * BATCH OF WINDOWS, RESIZED")]
    tail = windows[windows.index("NOT provided"):]
    assert "RESIZED" in tail and "arbitrary sizes" not in tail                   # the batch section points here
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = J.load_library()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in {n for n, _, _ in J.api.ABI}
    for name in ("resize_taps", "resize_pick_window"):
        assert callable(getattr(J, name))
    assert callable(J.Context.decode_windows_resized_dev)


def c_taps(J, n_in, n_out, cap=None, tables=True):
    lib = J.load_library()
    ksize = C.c_int(-7)
    rc = lib.jpezy_resize_taps(n_in, n_out, C.byref(ksize), None, None, None, 0)
    if rc != 0 or not tables:
        return rc, ksize.value, None, None, None
    first, count = np.full(n_out, -7, np.int32), np.full(n_out, -7, np.int32)
    weight = np.full((n_out, ksize.value), -7, np.int32)
    cap = weight.size if cap is None else cap
    rc = lib.jpezy_resize_taps(n_in, n_out, C.byref(ksize), first.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
                               weight.ctypes.data_as(C.c_void_p), cap)
    return rc, ksize.value, first, count, weight


TAP_SIZES = [(1, 1), (1, 8), (8, 1), (9, 3), (16, 16), (17, 24), (70, 24), (120, 7), (777, 224), (65535, 1), (1, 65535)]


@pytest.mark.parametrize("n_in, n_out", TAP_SIZES)
def test_resize_taps_equal_the_restatement(J, n_in, n_out):
    ksize, first, count, weight = RM.taps(n_in, n_out)
    rc, got_k, got_first, got_count, got_weight = c_taps(J, n_in, n_out)
    assert rc == 0 and got_k == ksize
    assert np.array_equal(got_first, first) and np.array_equal(got_count, count) and np.array_equal(got_weight, weight)
    assert (count >= 1).all() and (count <= ksize).all() and (first >= 0).all() and (first + count <= n_in).all()
    behind = np.arange(ksize)[None, :] >= got_count[:, None]
    assert (got_weight[behind] == 0).all()                                       # zero behind count
    assert (got_weight >= 0).all()
    off = np.abs(got_weight.sum(axis=1, dtype=np.int64) - (1 << 22))
    assert (off <= got_count // 2 + 1).all(), int(off.max())
    # what the accumulator bound in the header rests on
    assert (255 * got_weight.sum(axis=1, dtype=np.int64) + (1 << 21) < 2 ** 31).all()
    a, b, c = J.resize_taps(n_in, n_out)
    assert np.array_equal(a, first) and np.array_equal(b, count) and np.array_equal(c, weight)


def test_identity_taps_are_one_full_weight():
    for n in (1, 2, 16, 777):
        ksize, first, count, weight = RM.taps(n, n)
        assert ksize == 3
        for i in range(n):
            row = [int(weight[i, j]) for j in range(int(count[i]))]
            assert sorted(row)[-1] == 1 << 22 and sum(row) == 1 << 22 and int(first[i]) + row.index(1 << 22) == i
    img = np.random.default_rng(1).integers(0, 256, (9, 13, 3), dtype=np.uint8)
    assert np.array_equal(RM.resize(img, 13, 9), img)
    assert np.array_equal(RM.resize(img, 13, 9, mirror=True), img[:, ::-1])


def test_resize_taps_refusals_and_the_capacity_at_equality_and_one_short(J):
    lib = J.load_library()
    k = C.c_int()
    for n_in, n_out in ((0, 4), (4, 0), (-1, 4), (65536, 4), (4, 65536)):
        assert lib.jpezy_resize_taps(n_in, n_out, C.byref(k), None, None, None, 0) == E_BADARG and "1..65535" in _err(lib)
    assert lib.jpezy_resize_taps(8, 4, None, None, None, None, 0) == E_BADARG and "null pointer" in _err(lib)
    for n_in, n_out in ((70, 24), (9, 3), (1, 8)):
        ksize = RM.taps(n_in, n_out)[0]
        rc, got_k, first, count, weight = c_taps(J, n_in, n_out, cap=n_out * ksize)
        assert rc == 0 and got_k == ksize and (weight != -7).all()
        rc, got_k, first, count, weight = c_taps(J, n_in, n_out, cap=n_out * ksize - 1)
        assert rc == E_NOSPACE and "weight_cap" in _err(lib) and got_k == ksize
        assert (weight == -7).all() and (first == -7).all() and (count == -7).all()          # nothing is written
    first = np.zeros(4, np.int32)
    assert lib.jpezy_resize_taps(8, 4, C.byref(k), first.ctypes.data_as(C.c_void_p), None, None, 0) == E_BADARG and "together" in _err(lib)
    with pytest.raises(J.JpezyError, match="1..65535"):
        J.resize_taps(0, 4)


PILLOW_SHAPES = [((33, 70), (24, 24)), ((17, 9), (24, 24)), ((16, 16), (16, 16)), ((208, 120), (32, 48)), ((1, 1), (8, 8)), ((300, 7), (5, 64)),
                 ((64, 48), (63, 47)), ((40, 24), (80, 48)), ((555, 777), (224, 224)), ((9, 1), (3, 3))]


@pytest.mark.parametrize("src, dst", PILLOW_SHAPES)
def test_the_restatement_equals_pillow_bilinear(src, dst):
    """an independent anchor (the restatement remains the pin): Pillow's BILINEAR resize of a 3-channel image, byte for byte"""
    Image = pytest.importorskip("PIL.Image")
    (w, h), (ow, oh) = src, dst
    rng = np.random.default_rng(w * 1000 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([np.clip(128 + 100 * np.sin((xx * (c + 1) + yy * (3 - c)) / 5.0) + rng.integers(-60, 61, (h, w)), 0, 255) for c in range(3)],
                   axis=2).astype(np.uint8)
    want = np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), Image.BILINEAR))
    assert np.array_equal(RM.resize(img, ow, oh), want)


def c_pick(J, W, H, src, out_w, out_h):
    win = J.Window(J.Rect(-7, -7, -7, -7), -7)
    rc = J.load_library().jpezy_resize_pick_window(W, H, C.byref(J.Rect(*src)), out_w, out_h, C.byref(win))
    return rc, ((win.region.x, win.region.y, win.region.w, win.region.h), win.scale_denom)


def test_pick_window_against_the_restatement(J):
    lib = J.load_library()
    cases = []
    out_w, out_h = 10, 6
    W, H = 400, 300
    for ratio in (1, 2, 4, 8):                                       # w / out_w at equality and one pixel short, h roomy; then the same for h
        for short in (0, 1):
            cases.append((W, H, (3, 5, out_w * ratio - short, 200), out_w, out_h))
            cases.append((W, H, (3, 5, 300, out_h * ratio - short), out_w, out_h))
            cases.append((W, H, (7, 9, out_w * ratio - short, out_h * ratio - short), out_w, out_h))
    cases += [(W, H, (0, 0, 1, 1), 8, 8), (W, H, (399, 299, 1, 1), 1, 1), (1, 1, (0, 0, 1, 1), 224, 224), (W, H, (0, 0, 400, 300), 1, 1)]
    for W2, H2 in ((17, 9), (33, 70)):                               # touching the right / bottom edge of odd-sized pictures, at every scale
        for out in ((1, 1), (2, 1), (4, 2), (8, 4), (16, 8), (3, 3)):
            for src in ((0, 0, W2, H2), (1, 0, W2 - 1, H2), (0, 1, W2, H2 - 1), (W2 - 9, H2 - 9, 9, 9), (W2 - 1, H2 - 1, 1, 1), (5, 3, W2 - 5, H2 - 3)):
                cases.append((W2, H2, src, out[0], out[1]))
    scales = set()
    for W2, H2, src, ow, oh in cases:
        want = RM.pick_window(W2, H2, src, ow, oh)
        rc, got = c_pick(J, W2, H2, src, ow, oh)
        assert rc == 0 and got == want, (W2, H2, src, ow, oh, got, want)
        assert J.resize_pick_window(W2, H2, src, ow, oh) == want
        (x, y, w, h), s = got
        assert lib.jpezy_region_check(W2, H2, s, C.byref(J.Rect(x, y, w, h))) == 0, (W2, H2, src, got, _err(lib))
        ws, hs = M.scaled_size(W2, H2, s)
        assert x + w <= ws and y + h <= hs
        # the crop's edges move by less than s full-size pixels
        assert 0 <= src[0] - x * s < s and 0 <= src[1] - y * s < s and (s == 1 or 0 <= src[2] - w * s < s)
        scales.add(s)
    assert scales == {1, 2, 4, 8} and len(cases) > 80
    one = (0, 0, 1, 1)
    for W2, H2, src, ow, oh, names in ((8, 8, (6, 0, 3, 1), 1, 1, "outside the picture"), (8, 8, (0, 0, 0, 1), 1, 1, "w, h >= 1"), (0, 8, one, 1, 1, "width and height"),
                                       (8, 8, one, 0, 1, "out_w and out_h"), (8, 8, one, 1, 65536, "out_w and out_h"), (8, 8, (-1, 0, 2, 2), 1, 1, "x, y >= 0")):
        rc, got = c_pick(J, W2, H2, src, ow, oh)
        assert rc == E_BADARG and names in _err(lib) and got == ((-7, -7, -7, -7), -7), (src, _err(lib))
    assert lib.jpezy_resize_pick_window(8, 8, None, 1, 1, C.byref(J.Window())) == E_BADARG and "null pointer" in _err(lib)
    assert lib.jpezy_resize_pick_window(8, 8, C.byref(J.Rect(*one)), 1, 1, None) == E_BADARG and "null pointer" in _err(lib)


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
    mirror = (C.c_uint8 * n)(1, 0)

    # out 5 x 4 pixels of 3 bytes: tight rows are 15 bytes, a tight slot is 60
    def call(n=n, data=data, lens=lens, wins=wins, mirror=mirror, ow=5, oh=4, fmt=0, row=16, slot=64, pix=p, cap=4096, infos=infos, placed=placed,
             status=status):
        return lib.jpezy_decode_windows_resized_dev(None, n, data, lens, 0, wins, mirror, ow, oh, fmt, row, slot, pix, cap, infos, placed, status)

    assert call() == E_BADARG and "null context" in _err(lib)
    assert call(wins=None, placed=None, mirror=None) == E_BADARG and "null context" in _err(lib)       # the three arrays may be null
    assert call(row=0, slot=0, cap=120) == E_BADARG and "null context" in _err(lib)                    # both strides 0 = tight: 2 * 60 bytes
    assert call(row=15, slot=60) == E_BADARG and "null context" in _err(lib)                           # both at equality
    assert call(row=16, slot=3 * 16 + 15) == E_BADARG and "null context" in _err(lib)                  # the slot at equality
    assert call(cap=n * 64) == E_BADARG and "null context" in _err(lib)                                # n * slot_stride == pix_cap
    assert call(ow=65535, oh=1, row=0, slot=0, cap=1 << 20) == E_BADARG and "null context" in _err(lib)
    assert call(n=0, data=None, lens=None, infos=None, status=None, pix=None, fmt=9, ow=0, row=1) == 0  # n == 0: nothing is looked at
    cases = [
        (dict(n=-1), E_BADARG, "n must not be negative"),
        (dict(data=None), E_BADARG, "null pointer"), (dict(lens=None), E_BADARG, "null pointer"), (dict(infos=None), E_BADARG, "null pointer"),
        (dict(status=None), E_BADARG, "null pointer"), (dict(pix=None), E_BADARG, "null pointer"),
        (dict(fmt=4), E_BADARG, "pixel format"), (dict(fmt=-1), E_BADARG, "pixel format"),
        (dict(ow=0), E_BADARG, "out_w and out_h"), (dict(oh=0), E_BADARG, "out_w and out_h"), (dict(ow=65536), E_BADARG, "out_w and out_h"),
        (dict(oh=-3), E_BADARG, "out_w and out_h"),
        (dict(row=1 << 32), E_BADARG, "32 bits"), (dict(row=14), E_BADARG, "row_stride smaller"),
        (dict(slot=3 * 16 + 14), E_NOSPACE, "does not fit"), (dict(row=0, slot=59), E_NOSPACE, "does not fit"),
        (dict(cap=n * 64 - 1), E_NOSPACE, "pix_cap"), (dict(row=0, slot=0, cap=119), E_NOSPACE, "pix_cap"), (dict(slot=(1 << 63) + 5), E_NOSPACE, "pix_cap"),
        # which of two bad arguments is named: the order is n, arrays, format, output size, row stride, slot stride, capacity
        (dict(n=-1, data=None), E_BADARG, "n must not be negative"),
        (dict(data=None, fmt=9), E_BADARG, "null pointer"),
        (dict(fmt=9, ow=0), E_BADARG, "pixel format"),
        (dict(ow=0, row=1), E_BADARG, "out_w and out_h"),
        (dict(row=14, slot=1), E_BADARG, "row_stride smaller"),
        (dict(row=1 << 32, slot=1), E_BADARG, "32 bits"),
        (dict(slot=1, cap=1), E_NOSPACE, "does not fit"),
        (dict(status=None, cap=1), E_BADARG, "null pointer"),
    ]
    for i, (kw, code, names) in enumerate(cases):
        assert call(**kw) == code, (i, kw, _err(lib))
        msg = _err(lib)
        assert names in msg and msg.startswith("decode_windows_resized_dev:"), (i, kw, msg)
    assert (np.frombuffer(buf, np.uint8) == 0).all()
