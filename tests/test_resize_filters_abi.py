"""The resampling filters of the resized batch of windows (include/jpezy_hip.h, BATCH OF WINDOWS, RESIZED, FILTERS), as far
as they can be checked without a GPU: jpezy_resize_taps_filter against tests/resize_filter_model.py for all four filters, that restatement
against Pillow's BOX / BICUBIC / LANCZOS resize as an independent anchor, the bilinear tables against the existing function and the
existing restatement, the refusals, and the symbols.  Every comparison is exact."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import resize_filter_model as FM
import resize_model as RM

ROOT = Path(__file__).resolve().parent.parent
E_BADARG, E_UNSUPPORTED = -1, -4
NAMES = ("jpezy_resize_taps_filter", "jpezy_ctx_set_windows_filter", "jpezy_ctx_windows_filter", "jpezy_ctx_set_resample_direct",
         "jpezy_ctx_last_resample_tiled_count")
FILTER_NAMES = {FM.BILINEAR: "FILTER_BILINEAR", FM.BOX: "FILTER_BOX", FM.BICUBIC: "FILTER_BICUBIC", FM.LANCZOS: "FILTER_LANCZOS"}


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _err(lib):
    return lib.jpezy_hip_last_error().decode()


def c_taps(J, filt, n_in, n_out):
    lib = J.load_library()
    ksize = C.c_int(-7)
    rc = lib.jpezy_resize_taps_filter(filt, n_in, n_out, C.byref(ksize), None, None, None, 0)
    if rc != 0:
        return rc, ksize.value, None, None, None
    first, count = np.full(n_out, -7, np.int32), np.full(n_out, -7, np.int32)
    weight = np.full((n_out, ksize.value), -7, np.int32)
    rc = lib.jpezy_resize_taps_filter(filt, n_in, n_out, C.byref(ksize), first.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
                                      weight.ctypes.data_as(C.c_void_p), weight.size)
    return rc, ksize.value, first, count, weight


def test_the_symbols_the_constants_and_the_header(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = J.load_library()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in {n for n, _, _ in J.api.ABI}
    enum = re.search(r"enum\s+jpezy_filter\s*\{([^}]*)\}", code).group(1)
    for value, name in FILTER_NAMES.items():
        assert re.search(r"\bJPEZY_" + name + r"\s*=\s*%d\b" % value, enum), name
        assert getattr(J, name) == value
    section = text[text.index(" * BATCH OF WINDOWS, RESIZED"):text.index(" * BATCH OF WINDOWS, TENSOR OUTPUT")]
    for phrase in ("FILTERS", "fsup", "a = -0.5", "sinc(x / 3)", "platform's binary64 sin", "arithmetic", "JPEZY_E_UNSUPPORTED",
                   "2^31 - 2^21", "Hamming", "filter of the context the call was made on"):
        assert phrase in section, phrase
    for name in ("set_windows_filter", "windows_filter", "set_resample_direct", "last_resample_tiled_count"):
        assert callable(getattr(J.Context, name))


# growing, equal and shrinking; the extremes of the size range; ratios just below 2, where the capacity of the two-pass tile is decided
SWEEP = [(1, 1), (1, 8), (1, 64), (8, 1), (9, 3), (16, 16), (17, 24), (17, 80), (33, 70), (40, 24), (63, 32), (64, 64), (70, 24), (120, 7),
         (120, 2), (208, 3), (208, 64), (447, 224), (777, 224), (4096, 1), (65535, 100), (65535, 1), (100, 65535), (65535, 65535)]


@pytest.mark.parametrize("filt", FM.FILTERS)
@pytest.mark.parametrize("n_in, n_out", SWEEP)
def test_taps_equal_the_restatement(J, filt, n_in, n_out):
    ksize, first, count, weight = FM.taps(filt, n_in, n_out)
    rc, got_k, got_first, got_count, got_weight = c_taps(J, filt, n_in, n_out)
    assert rc == 0, _err(J.load_library())                                        # (the overflow condition does not fire)
    assert got_k == ksize
    assert np.array_equal(got_first, first) and np.array_equal(got_count, count) and np.array_equal(got_weight, weight)
    assert (count >= 1).all() and (count <= ksize).all() and (first >= 0).all() and (first + count <= n_in).all()
    assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()    # what the tile's span of source rows rests on
    assert (got_weight[np.arange(ksize)[None, :] >= got_count[:, None]] == 0).all()          # zero behind count
    assert FM.fits_32_bits(weight)
    if filt in (FM.BILINEAR, FM.BOX):
        assert (weight >= 0).all()
    a, b, c = J.resize_taps(n_in, n_out, filter=filt)
    assert np.array_equal(a, first) and np.array_equal(b, count) and np.array_equal(c, weight)
    if n_in == n_out:                                                             # identity: one full weight on the sample itself
        rows = np.arange(n_out)
        assert (first <= rows).all() and (weight[rows, rows - first] == 1 << 22).all() and (np.abs(weight).sum(axis=1) == 1 << 22).all()
    FM.taps.cache_clear()


@pytest.mark.parametrize("n_in, n_out", [s for s in SWEEP if max(s) < 65535] + [(65535, 100)])
def test_bilinear_is_the_existing_function_and_the_existing_restatement(J, n_in, n_out):
    ksize, first, count, weight = RM.taps(n_in, n_out)
    k2, f2, c2, w2 = FM.taps(FM.BILINEAR, n_in, n_out)
    assert k2 == ksize and np.array_equal(f2, first) and np.array_equal(c2, count) and np.array_equal(w2, weight)
    lib = J.load_library()
    old_k = C.c_int()
    old_first, old_count, old_weight = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32), np.zeros((n_out, ksize), np.int32)
    assert lib.jpezy_resize_taps(n_in, n_out, C.byref(old_k), old_first.ctypes.data_as(C.c_void_p), old_count.ctypes.data_as(C.c_void_p),
                                 old_weight.ctypes.data_as(C.c_void_p), old_weight.size) == 0
    rc, new_k, new_first, new_count, new_weight = c_taps(J, FM.BILINEAR, n_in, n_out)
    assert rc == 0 and new_k == old_k.value == ksize
    assert np.array_equal(new_first, old_first) and np.array_equal(new_count, old_count) and np.array_equal(new_weight, old_weight)
    assert np.array_equal(old_weight, weight)
    a, b, c = J.resize_taps(n_in, n_out)                                          # the keyword's default
    assert np.array_equal(a, first) and np.array_equal(b, count) and np.array_equal(c, weight)
    RM.taps.cache_clear()
    FM.taps.cache_clear()


def test_the_restatement_resizes_as_the_existing_one_at_bilinear():
    img = np.random.default_rng(5).integers(0, 256, (21, 34, 4), dtype=np.uint8)
    for out in ((34, 21), (9, 30), (50, 4), (1, 1)):
        for mirror in (False, True):
            assert np.array_equal(FM.resize(img, out[0], out[1], FM.BILINEAR, mirror), RM.resize(img, out[0], out[1], mirror))
    for filt in FM.FILTERS:                                                       # identity, every filter
        assert np.array_equal(FM.resize(img, 34, 21, filt), np.concatenate([img[:, :, :3], np.full((21, 34, 1), 255, np.uint8)], axis=2))
        assert np.array_equal(FM.resize(img[:, :, :3], 34, 21, filt, mirror=True), img[:, ::-1, :3])


def test_the_tile_capacity_holds_every_lanczos_ratio_below_two():
    """kResampleTileRows (jpezy_device.h) against the tables: no tile of 16 output rows spans more source rows at a ratio below 2, which is
    what jpezy_resize_pick_window leaves"""
    rows = int(re.search(r"constexpr int kResampleTileRows = (\d+);", (ROOT / "jpezy_amd" / "csrc" / "jpezy_device.h").read_text()).group(1))
    worst = 0
    for n_out in list(range(1, 80)) + [112, 224, 299, 384]:
        for n_in in (range(n_out, 2 * n_out) if n_out < 80 else (2 * n_out - 1, 2 * n_out - 2, n_out * 19 // 10)):
            _, first, count, _ = FM.taps(FM.LANCZOS, n_in, n_out, False)
            worst = max(worst, FM.tile_span(first, count, 16))
    FM.taps.cache_clear()
    assert worst <= rows and worst == 42, worst


PILLOW_SHAPES = [((33, 70), (24, 24)), ((17, 9), (24, 24)), ((16, 16), (16, 16)), ((208, 120), (32, 48)), ((1, 1), (8, 8)), ((300, 7), (5, 64)),
                 ((64, 48), (63, 47)), ((40, 24), (80, 48)), ((555, 777), (224, 224)), ((9, 1), (3, 3))]


@pytest.mark.parametrize("filt", [FM.BOX, FM.BICUBIC, FM.LANCZOS])
@pytest.mark.parametrize("src, dst", PILLOW_SHAPES)
def test_the_restatement_equals_pillow(src, dst, filt):
    """an independent anchor (the restatement remains the pin): Pillow's resize of a 3-channel image, byte for byte, on the ten shapes of the
    bilinear anchor (tests/test_resized_abi.py), with random and with 0 / 255 pixels (the latter drive the negative lobes into the clip)"""
    Image = pytest.importorskip("PIL.Image")
    resample = {FM.BOX: Image.BOX, FM.BICUBIC: Image.BICUBIC, FM.LANCZOS: Image.LANCZOS}[filt]
    (w, h), (ow, oh) = src, dst
    rng = np.random.default_rng(w * 1000 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.stack([np.clip(128 + 100 * np.sin((xx * (c + 1) + yy * (3 - c)) / 5.0) + rng.integers(-60, 61, (h, w)), 0, 255) for c in range(3)],
                      axis=2).astype(np.uint8)
    extreme = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    for img in (smooth, extreme):
        want = np.asarray(Image.fromarray(img, "RGB").resize((ow, oh), resample))
        assert np.array_equal(FM.resize(img, ow, oh, filt), want)


def test_refusals(J):
    lib = J.load_library()
    k = C.c_int(-7)
    for filt in (-1, 4, 99):
        assert lib.jpezy_resize_taps_filter(filt, 8, 4, C.byref(k), None, None, None, 0) == E_BADARG and "JPEZY_FILTER_" in _err(lib)
        assert lib.jpezy_resize_taps_filter(filt, 0, 4, C.byref(k), None, None, None, 0) == E_BADARG and "JPEZY_FILTER_" in _err(lib)      # named first
        assert k.value == -7
        assert lib.jpezy_ctx_set_windows_filter(None, filt) == E_BADARG and "JPEZY_FILTER_" in _err(lib)
        with pytest.raises(J.JpezyError, match="JPEZY_FILTER_"):
            J.resize_taps(8, 4, filter=filt)
    for n_in, n_out in ((0, 4), (4, 0), (65536, 4), (4, 65536)):                  # jpezy_resize_taps's contract otherwise
        assert lib.jpezy_resize_taps_filter(FM.LANCZOS, n_in, n_out, C.byref(k), None, None, None, 0) == E_BADARG and "1..65535" in _err(lib)
    assert lib.jpezy_resize_taps_filter(FM.BICUBIC, 8, 4, None, None, None, None, 0) == E_BADARG and "null pointer" in _err(lib)
    ksize = FM.taps(FM.BICUBIC, 70, 24)[0]
    first, count, weight = np.full(24, -7, np.int32), np.full(24, -7, np.int32), np.full((24, ksize), -7, np.int32)
    ptr = [a.ctypes.data_as(C.c_void_p) for a in (first, count, weight)]
    assert lib.jpezy_resize_taps_filter(FM.BICUBIC, 70, 24, C.byref(k), *ptr, weight.size - 1) == -6 and "weight_cap" in _err(lib)
    assert (weight == -7).all() and (first == -7).all() and k.value == ksize
    assert lib.jpezy_resize_taps_filter(FM.BICUBIC, 70, 24, C.byref(k), *ptr, weight.size) == 0 and (weight != -7).all()
    for valid in FM.FILTERS:                                                      # a valid filter gets as far as the context
        assert lib.jpezy_ctx_set_windows_filter(None, valid) == E_BADARG and "null context" in _err(lib)
    for fn in (lib.jpezy_ctx_windows_filter, lib.jpezy_ctx_last_resample_tiled_count):
        assert fn(None) == E_BADARG and "null context" in _err(lib)
    assert lib.jpezy_ctx_set_resample_direct(None, 1) == E_BADARG and "null context" in _err(lib)
