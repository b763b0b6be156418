"""YCbCr 4:2:2 samples in and out (include/jpezy_hip_ycc422.h), as far as it can be checked without a GPU: the size
helpers, the argument checks that come before any device is touched (null context; null pointers, formats, c_step, strides and the
32-bit limit before the context), the ties of tests/ycc422_model.py to the definitions that exist, and the declared / exported / bound
set of entries.  tests/test_gpu_ycc422.py holds the parity tests."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import quant_model as QM
import sampling422_model as S2
import ycc422_model as M

ROOT = Path(__file__).resolve().parent.parent
E_BADARG = -1
ENTRIES = ("jpezy_yuv422_row_bytes", "jpezy_ycc422_chroma_size", "jpezy_fdct_quant_ycc422_dev", "jpezy_encode_jpeg_ycc422",
           "jpezy_fdct_quant_yuv422_dev", "jpezy_encode_jpeg_yuv422", "jpezy_dequant_idct_generic_yuv422_dev", "jpezy_decode_jpeg_yuv422")


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


# ---- 1. the size helpers ----
def test_size_helpers(J):
    lib = J.load_library()
    for W, H in M.SIZES + [(65535, 65535), (3, 2)]:
        assert lib.jpezy_yuv422_row_bytes(W) == 4 * ((W + 1) // 2) == M.row_bytes(W) == J.yuv422_row_bytes(W)
        cw, ch = C.c_int(-1), C.c_int(-1)
        assert lib.jpezy_ycc422_chroma_size(W, H, C.byref(cw), C.byref(ch)) == 0
        assert (cw.value, ch.value) == ((W + 1) // 2, H) == M.chroma_size(W, H) == J.ycc422_chroma_size(W, H)
    cw, ch = C.c_int(-1), C.c_int(-1)
    for bad in (0, -1, 65536):
        assert lib.jpezy_yuv422_row_bytes(bad) == E_BADARG
        assert lib.jpezy_ycc422_chroma_size(bad, 5, C.byref(cw), C.byref(ch)) == E_BADARG
        assert lib.jpezy_ycc422_chroma_size(5, bad, C.byref(cw), C.byref(ch)) == E_BADARG
        with pytest.raises(J.JpezyError):
            J.yuv422_row_bytes(bad)
        with pytest.raises(J.JpezyError):
            J.ycc422_chroma_size(bad, 1)
    assert (cw.value, ch.value) == (-1, -1)
    assert lib.jpezy_ycc422_chroma_size(9, 17, None, None) == 0
    cw = C.c_int(-1)
    assert lib.jpezy_ycc422_chroma_size(9, 17, C.byref(cw), None) == 0 and cw.value == 5
    assert lib.jpezy_ycc422_chroma_size(9, 17, None, C.byref(cw)) == 0 and cw.value == 17


# ---- 2, 3. the checks in front of the device ----
class Args:
    """valid arguments of every entry for a 16 x 16 picture; the buffers are never dereferenced (a null context is refused first)"""

    def __init__(self, J):
        self.lib = J.load_library()
        self.buf = np.zeros(4096, np.uint8)
        self.p = self.buf.ctypes.data_as(C.c_void_p)
        self.qt = ((C.c_uint16 * 64) * 4)()
        self.hs, self.vs, self.tq = (C.c_uint8 * 3)(2, 1, 1), (C.c_uint8 * 3)(1, 1, 1), (C.c_uint8 * 3)(0, 1, 1)
        self.info = J.FrameInfo()

    def ycc_dev(self, ctx=None, y=1, ys=0, cb=1, cr=1, cs=0, step=1, yfs=0, cfs=0, W=16, H=16, n=1, co=1):
        q = lambda f: self.p if f else None
        return self.lib.jpezy_fdct_quant_ycc422_dev(ctx, q(y), ys, q(cb), q(cr), cs, step, yfs, cfs, W, H, n, q(co), None)

    def ycc_file(self, ctx=None, y=1, ys=0, cb=1, cr=1, cs=0, step=1, W=16, H=16, out=1):
        q = lambda f: self.p if f else None
        return self.lib.jpezy_encode_jpeg_ycc422(ctx, q(y), ys, q(cb), q(cr), cs, step, W, H, b"", q(out), self.buf.size)

    def yuv_dev(self, ctx=None, pix=1, fmt=0, rs=0, fs=0, W=16, H=16, n=1, co=1):
        q = lambda f: self.p if f else None
        return self.lib.jpezy_fdct_quant_yuv422_dev(ctx, q(pix), fmt, rs, fs, W, H, n, q(co), None)

    def yuv_file(self, ctx=None, pix=1, fmt=0, rs=0, W=16, H=16, out=1):
        q = lambda f: self.p if f else None
        return self.lib.jpezy_encode_jpeg_yuv422(ctx, q(pix), fmt, rs, W, H, b"", q(out), self.buf.size)

    def idct_dev(self, ctx=None, co=1, qt=1, hs=1, vs=1, tq=1, fmt=0, rs=0, fs=0, W=16, H=16, n=1, pix=1):
        q = lambda f: self.p if f else None
        r = lambda f, a: C.byref(a) if f else None
        return self.lib.jpezy_dequant_idct_generic_yuv422_dev(ctx, q(co), r(qt, self.qt), 3, r(hs, self.hs), r(vs, self.vs), r(tq, self.tq), 8, W, H, fmt,
                                                              rs, fs, n, q(pix), None)

    def decode_file(self, ctx=None, data=1, info=1, fmt=0, rs=0, pix=1):
        q = lambda f: self.p if f else None
        return self.lib.jpezy_decode_jpeg_yuv422(ctx, q(data), 64, C.byref(self.info) if info else None, fmt, rs, q(pix), self.buf.size)

    def err(self):
        return self.lib.jpezy_hip_last_error()


def test_null_context_is_refused_with_a_message(J):
    a = Args(J)
    for call in (a.ycc_dev, a.ycc_file, a.yuv_dev, a.yuv_file, a.idct_dev, a.decode_file):
        assert call() == E_BADARG, call.__name__
        assert b"context" in a.err(), (call.__name__, a.err())


def test_null_pointers_are_refused_before_the_context(J):
    a = Args(J)
    calls = [(a.ycc_dev, k) for k in ("y", "cb", "cr", "co")] + [(a.ycc_file, k) for k in ("y", "cb", "cr", "out")]
    calls += [(a.yuv_dev, k) for k in ("pix", "co")] + [(a.yuv_file, k) for k in ("pix", "out")]
    calls += [(a.idct_dev, k) for k in ("co", "qt", "hs", "vs", "tq", "pix")] + [(a.decode_file, k) for k in ("data", "info")]
    for call, k in calls:
        assert call(**{k: 0}) == E_BADARG, (call.__name__, k)
        assert b"null" in a.err() and b"context" not in a.err(), (call.__name__, k, a.err())


@pytest.mark.parametrize("fmt", [-1, 3, 4, 255])
def test_a_format_outside_0_2_is_refused_before_the_context(J, fmt):
    a = Args(J)
    for call in (a.yuv_dev, a.yuv_file, a.idct_dev, a.decode_file):
        assert call(fmt=fmt) == E_BADARG, call.__name__
        assert b"format" in a.err() and b"context" not in a.err(), (call.__name__, a.err())


@pytest.mark.parametrize("step", [0, 3, -1, 4])
def test_c_step_outside_1_2_is_refused_before_the_context(J, step):
    a = Args(J)
    for call in (a.ycc_dev, a.ycc_file):
        assert call(step=step) == E_BADARG, call.__name__
        assert b"c_step" in a.err() and b"context" not in a.err(), (call.__name__, a.err())


def test_strides_are_checked_before_the_context(J):
    """the list of test_ycc_abi.py's test of this name at CH = H, extended by the packed entries"""
    a = Args(J)
    # 16 x 16: W = 16, CW = 8, CH = 16; tight frame strides 256 (Y) and 128 / 256 (chroma, c_step 1 / 2)
    for kw, word in [(dict(ys=15), b"y_stride"), (dict(cs=7), b"c_stride"), (dict(cs=14, step=2), b"c_stride"), (dict(ys=1 << 31), b"32 bits"),
                     (dict(cs=1 << 31), b"32 bits"), (dict(yfs=255), b"y_frame_stride"), (dict(cfs=127), b"c_frame_stride"),
                     (dict(cfs=254, step=2), b"c_frame_stride")]:
        assert a.ycc_dev(**kw) == E_BADARG, kw
        assert word in a.err() and b"context" not in a.err(), (kw, a.err())
    for kw, word in [(dict(ys=15), b"y_stride"), (dict(cs=7), b"c_stride"), (dict(cs=14, step=2), b"c_stride"), (dict(ys=1 << 31), b"32 bits")]:
        assert a.ycc_file(**kw) == E_BADARG, kw
        assert word in a.err() and b"context" not in a.err(), (kw, a.err())
    # packed: row_bytes = 32, a frame = 15 * row_stride + 32
    for call in (a.yuv_dev, a.idct_dev):
        for kw, word in [(dict(rs=31), b"row_stride"), (dict(rs=1 << 31), b"32 bits"), (dict(fs=511), b"frame_stride"),
                         (dict(rs=40, fs=631), b"frame_stride"), (dict(W=17, rs=35), b"row_stride")]:
            assert call(**kw) == E_BADARG, (call.__name__, kw)
            assert word in a.err() and b"context" not in a.err(), (call.__name__, kw, a.err())
    for kw, word in [(dict(rs=31), b"row_stride"), (dict(rs=1 << 31), b"32 bits"), (dict(W=17, rs=35), b"row_stride")]:
        assert a.yuv_file(**kw) == E_BADARG, kw
        assert word in a.err() and b"context" not in a.err(), (kw, a.err())
    # (the file decode learns W and H from the file: its stride is checked once the header is read)
    for W, H in [(0, 16), (16, 0), (65536, 16), (16, 65536), (-1, 16)]:
        for call in (a.ycc_dev, a.ycc_file, a.yuv_dev, a.yuv_file, a.idct_dev):
            assert call(W=W, H=H) == E_BADARG, (call.__name__, W, H)
            assert b"context" not in a.err(), (call.__name__, a.err())
    # a stride that is just large enough gets as far as the context
    for rc in (a.ycc_dev(ys=16, cs=8, yfs=256, cfs=128), a.ycc_dev(cs=15, step=2, cfs=255), a.yuv_dev(rs=32, fs=512), a.yuv_dev(rs=40, fs=632),
               a.idct_dev(rs=32, fs=512), a.yuv_dev(W=17, rs=36)):
        assert rc == E_BADARG and b"context" in a.err(), a.err()


# ---- 4. the model's ties to the definitions that exist ----
@pytest.fixture(scope="module")
def annex_k(oracle):
    return QM.tables("q50")


@pytest.mark.parametrize("W,H", M.ANCHOR_SIZES)
def test_anchor_planes_from_rgb_give_the_rgb_paths_coefficients(oracle, annex_k, W, H):
    want = S2.quantise(S2.synth_dct(W, H), *annex_k)
    got = M.encode_coeffs(*M.planes_from_rgb(*oracle.synth_rgb(W, H), W, H), *annex_k)
    assert np.array_equal(got, want)                # (synth_dct is dct_from_rgb(synth_rgb, POINT), computed once)


def test_anchor_at_an_even_width_that_is_no_multiple_of_16_holds_for_luma(oracle, annex_k):
    """the RGB path replicates pixel W-1, whose chroma no 4:2:2 plane holds: the luma blocks agree, the last chroma column need not"""
    W, H = 100, 100
    want = S2.quantise(S2.synth_dct(W, H), *annex_k)
    got = M.encode_coeffs(*M.planes_from_rgb(*oracle.synth_rgb(W, H), W, H), *annex_k)
    assert np.array_equal(got[:, :, :2], want[:, :, :2])
    assert np.array_equal(got[:, :-1], want[:, :-1])              # every MCU that the clamp does not reach


@pytest.mark.parametrize("value,dc_luma,dc_chroma", [(0, -63, -60), (255, 63, 59)])
def test_flat_plane_dcs(oracle, annex_k, value, dc_luma, dc_chroma):
    """samples of -128 / +127: the DCs DESIGN.md 4.8 states for the 4:2:0 planes"""
    co = M.encode_coeffs(np.full((8, 16), value, np.uint8), np.full((8, 8), value, np.uint8), np.full((8, 8), value, np.uint8), *annex_k)[0, 0]
    assert co[:2, 0].tolist() == [dc_luma] * 2 and co[2:, 0].tolist() == [dc_chroma] * 2
    assert not co[:, 1:].any()


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("W,H", [(1, 1), (2, 1), (7, 5), (15, 17), (16, 8), (17, 9)])
def test_unpack_of_pack_is_the_identity(fmt, W, H):
    y, cb, cr = M.random_planes(W, H)
    img = M.pack(y, cb, cr, fmt)
    assert img.shape == (H, M.row_bytes(W))
    y2, cb2, cr2 = M.unpack(img, W, fmt)
    assert np.array_equal(y, y2) and np.array_equal(cb, cb2) and np.array_equal(cr, cr2)
    # the byte order of the three formats, spelled out on the first macropixel
    first = {M.YUY2: (y[0, 0], cb[0, 0], cr[0, 0]), M.UYVY: (cb[0, 0], y[0, 0], cr[0, 0]), M.YVYU: (y[0, 0], cr[0, 0], cb[0, 0])}[fmt]
    assert (img[0, 0], img[0, 1], img[0, 3 if fmt != M.UYVY else 2]) == first
    if W > 1:
        assert img[0, 3 if fmt == M.UYVY else 2] == y[0, 1]


@pytest.mark.parametrize("fmt", M.FORMATS)
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (16, 8), (17, 9), (100, 100)])
def test_the_packed_model_is_the_planar_model_on_the_unpacked_planes(oracle, annex_k, fmt, W, H):
    y, cb, cr = M.random_planes(W, H, seed=fmt)
    want = M.encode_coeffs(y, cb, cr, *annex_k)
    for fill in (0, 0xFF):                  # odd W: the byte that is not read
        img = M.pack(y, cb, cr, fmt, fill=fill)
        assert np.array_equal(M.encode_coeffs_packed(img, W, fmt, *annex_k), want)
        assert np.array_equal(M.encode_coeffs(*M.unpack(img, W, fmt), *annex_k), want)


# ---- 5. declared, exported, bound ----
def test_header_declares_every_entry_and_the_library_exports_it(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    assert '#include "jpezy_hip_ycc422.h"' in text
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    part = strip((ROOT / "include" / "jpezy_hip_ycc422.h").read_text())
    declared = set(re.findall(r"\b(jpezy_[a-z0-9_]+)\s*\(", part))
    assert declared == set(ENTRIES) == {n for n, _, _ in J.api.ABI_YCC422}
    assert not declared & set(re.findall(r"\b(jpezy_[a-z0-9_]+)\s*\(", strip(text)))      # jpezy_hip.h's own set is closed
    assert not declared & {n for n, _, _ in J.api.ABI}
    lib = J.load_library()
    raw = C.CDLL(str(J.library_path()))
    for name in ENTRIES:
        assert hasattr(raw, name), f"libjpezy_hip.so does not export {name}"
        assert getattr(lib, name).argtypes is not None
    for k, name in enumerate(("JPEZY_YUV_YUY2", "JPEZY_YUV_UYVY", "JPEZY_YUV_YVYU")):
        assert re.search(name + r"\s*=\s*%d\b" % k, part)
    assert (J.YUV_YUY2, J.YUV_UYVY, J.YUV_YVYU) == (M.YUY2, M.UYVY, M.YVYU) == (0, 1, 2)
