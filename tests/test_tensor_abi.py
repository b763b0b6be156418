"""Tensor output of the resized batch of windows (include/jpezy_hip.h, BATCH OF WINDOWS, TENSOR OUTPUT), as far as it can be checked without a
GPU: what the header says and the library exports; the restatement tests/tensor_model.py against independent implementations (numpy's
binary16, torch's bfloat16 on the CPU); jpezy_tensor_normalization against the binary64 formula; and every refusal
jpezy_decode_windows_tensor_dev makes before it looks at the context, made here with a null context, including which of two bad arguments
is named.  tests/test_gpu_windows_tensor.py holds the parity tests.  Every comparison is exact."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import tensor_model as TM

ROOT = Path(__file__).resolve().parent.parent
E_BADARG, E_NOSPACE = -1, -6
NAMES = ("jpezy_tensor_normalization", "jpezy_decode_windows_tensor_dev")


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _err(lib):
    return lib.jpezy_hip_last_error().decode()


def test_header_declares_the_section_and_the_library_exports_it(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    section = text[text.index(" * BATCH OF WINDOWS, TENSOR OUTPUT"):text.index("PLANAR YCbCr 4:2:0 SAMPLES")]
    for phrase in ("Source bytes", "Element type", "NOT fused", "0x7FFF", "Placement", "IN ELEMENTS", "Fit", "Bytes touched", "neighbouring element",
                   "[2^-100, 2^100]", "stream capture", "this order: n < 0", "three-step", "NOT provided"):
        assert phrase in section, phrase
    # the two lists that named the gap point here now
    resized = text[text.index(" * BATCH OF WINDOWS, RESIZED"):text.index(" * BATCH OF WINDOWS, TENSOR OUTPUT")]
    assert "TENSOR OUTPUT" in resized[resized.index("NOT provided"):resized.index("*/")]
    design = (ROOT / "DESIGN.md").read_text()
    s415 = design[design.index("### 4.15"):design.index("### 4.16")]
    assert "4.17" in s415[s415.index("**Not provided**"):] and "### 4.17" in design
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = J.load_library()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in {n for n, _, _ in J.api.ABI}
    assert (J.DT_U8, J.DT_F32, J.DT_F16, J.DT_BF16) == (TM.DT_U8, TM.DT_F32, TM.DT_F16, TM.DT_BF16) == (0, 1, 2, 3)
    assert re.search(r"JPEZY_DT_U8 = 0, JPEZY_DT_F32 = 1, JPEZY_DT_F16 = 2, JPEZY_DT_BF16 = 3", code)
    assert callable(J.tensor_normalization) and callable(J.Context.decode_windows_tensor_dev)


# ---- the restatement against independent implementations -----------------------------------------------------------------------------------
IMAGENET = [(float(s), float(b)) for s, b in zip(*TM.normalization(TM.IMAGENET_MEAN, TM.IMAGENET_STD))]
PAIRS = [(1.0, 0.0), (1.0 / 255.0, 0.0), (2.0 ** -20, 0.0), (300.0, 0.0), (-300.0, 7.0), (2.0 ** -20, -2.0 ** -15), (0.0, 0.0), (0.0, -0.5),
         (2.0 ** -100, 0.0), (2.0 ** 100, -2.0 ** 100), (257.0, 0.5), (8.0 + 2.0 ** -7, 2.0 ** -9)] + IMAGENET
BYTES = np.arange(256, dtype=np.uint8)


@pytest.mark.parametrize("scale, bias", PAIRS)
def test_f16_equals_numpy(scale, bias):
    v = TM.affine(BYTES, scale, bias)
    with np.errstate(over="ignore"):
        want = v.astype(np.float16).view(np.uint16)
    got = TM.elements(BYTES, TM.DT_F16, scale, bias)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    if (scale, bias) == (2.0 ** -20, 0.0):                              # bytes 0..63 land in binary16 subnormals, and keep their values
        assert ((got[1:64] & 0x7C00) == 0).all() and (got[1:64] != 0).all() and (got[64] & 0x7C00) != 0
    if (scale, bias) == (300.0, 0.0):                                   # 300 * 218 = 65400 rounds to 65408 < 65520 <= 300 * 219: inf
        assert (got[219:] == 0x7C00).all() and (got[:219] < 0x7C00).all()


def test_f16_rounding_ties_and_edges():
    """the integer conversion itself, over bit patterns the bytes above do not reach: every tie of the subnormal range's coarsest and finest
    shifts, the largest finite value and the first that overflows, both signs"""
    rng = np.random.default_rng(7)
    u = np.concatenate([rng.integers(0x33000000, 0x47800000, 200000, dtype=np.int64), rng.integers(0, 0x7F800000, 50000, dtype=np.int64),
                        np.arange(0x387FC000 - 64, 0x387FC000 + 64), np.arange(0x477FE000 - 8, 0x477FF000 + 8), np.arange(0x33000000 - 4, 0x33000000 + 4),
                        (np.arange(0, 2048, dtype=np.int64) << 12) + 0x38000000, np.array([0, 0x7F800000])])
    u = np.concatenate([u, u | 0x80000000]).astype(np.uint32)
    v = u.view(np.float32)
    with np.errstate(over="ignore"):
        want = v.astype(np.float16).view(np.uint16)
    assert np.array_equal(TM.f16_bits(v), want)


@pytest.mark.parametrize("scale, bias", PAIRS)
def test_bf16_equals_torch_cpu(scale, bias):
    import torch
    v = TM.affine(BYTES, scale, bias)
    want = torch.from_numpy(v.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = TM.elements(BYTES, TM.DT_BF16, scale, bias)
    assert got.dtype == np.uint16 and np.array_equal(got, want)


def test_f32_and_u8_elements():
    for scale, bias in PAIRS:
        v = TM.affine(BYTES, scale, bias)
        assert np.isfinite(v).all()
        assert np.array_equal(TM.elements(BYTES, TM.DT_F32, scale, bias), v.view(np.uint32))
        # the product and the sum are rounded separately: equal to the binary64 evaluation rounded twice
        prod = (BYTES.astype(np.float64) * np.float64(np.float32(scale))).astype(np.float32)
        assert np.array_equal(v, (prod.astype(np.float64) + np.float64(np.float32(bias))).astype(np.float32))
    assert np.array_equal(TM.elements(BYTES, TM.DT_U8), BYTES)
    # with the ImageNet constants one fused operation differs from the two separate ones for some bytes: the restatement pins "not fused"
    differ = 0
    for scale, bias in IMAGENET:
        fused = (BYTES.astype(np.float64) * np.float64(np.float32(scale)) + np.float64(np.float32(bias))).astype(np.float32)
        differ += int((fused != TM.affine(BYTES, scale, bias)).sum())
    assert differ > 0


# ---- jpezy_tensor_normalization ------------------------------------------------------------------------------------------------------------
def c_norm(J, mean, std, C_=None):
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    n = mean.size if C_ is None else C_
    scale, bias = np.full(3, -7, np.float32), np.full(3, -7, np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = J.load_library().jpezy_tensor_normalization(n, vp(mean), vp(std), vp(scale), vp(bias))
    return rc, scale, bias


def test_normalization_equals_the_binary64_formula(J):
    rng = np.random.default_rng(3)
    cases = [(TM.IMAGENET_MEAN, TM.IMAGENET_STD), ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)), ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), ((0.449,), (0.226,)),
             ((-3.0, 1e-30, 7e20), (-0.25, 1e-12, 3e25))]
    cases += [(tuple(rng.uniform(-2, 2, 3)), tuple(rng.uniform(0.01, 3, 3))) for _ in range(50)]
    for mean, std in cases:
        rc, scale, bias = c_norm(J, mean, std)
        n = len(mean)
        assert rc == 0
        for c in range(n):
            assert scale[c] == np.float32(1.0 / (255.0 * std[c])) and bias[c] == np.float32(-mean[c] / std[c]), (mean, std, c)
        assert (scale[n:] == -7).all() and (bias[n:] == -7).all()
        want_s, want_b = TM.normalization(mean, std)
        got_s, got_b = J.tensor_normalization(mean, std)
        assert np.array_equal(got_s, want_s) and np.array_equal(got_b, want_b) and got_s.dtype == np.float32
        assert np.array_equal(scale[:n], want_s) and np.array_equal(bias[:n], want_b)


def test_normalization_refusals(J):
    lib = J.load_library()
    ok = (0.5, 0.5, 0.5)
    for mean, std in ((ok, (0.5, 0.0, 0.5)), (ok, (0.5, 0.5, np.inf)), (ok, (np.nan, 0.5, 0.5)), (ok, (0.5, -np.inf, 0.5)), ((0.5, np.inf, 0.5), ok),
                      ((np.nan, 0.5, 0.5), ok), (ok, (-0.0, 0.5, 0.5))):
        rc, scale, bias = c_norm(J, mean, std)
        assert rc == E_BADARG and "std must be finite and not zero" in _err(lib), (mean, std)
        assert (scale == -7).all() and (bias == -7).all()                # nothing is written
        with pytest.raises(J.JpezyError, match="tensor_normalization"):
            J.tensor_normalization(mean, std)
    for n in (0, 2, 4, -1):
        assert c_norm(J, ok, ok, C_=n)[0] == E_BADARG and "C must be 3 or 1" in _err(lib)
    a = np.zeros(3)
    vp = a.ctypes.data_as(C.c_void_p)
    for k in range(4):
        args = [vp] * 4
        args[k] = None
        assert lib.jpezy_tensor_normalization(3, *args) == E_BADARG and "null pointer" in _err(lib)


# ---- the placement rule ----------------------------------------------------------------------------------------------------------------------
def test_layout_rule_on_torch_layouts():
    """the restated rule admits what torch produces and nothing that overlaps: checked by brute force on small shapes"""
    import itertools
    import torch
    t = torch.empty(2, 3, 5, 4)
    for view in (t, t.contiguous(memory_format=torch.channels_last), torch.empty(2, 5, 4, 3).permute(0, 3, 1, 2), torch.empty(2, 3, 5, 9)[:, :, :, :4],
                 torch.empty(4, 3, 5, 4)[::2], torch.empty(2, 3, 5, 8)[:, :, :, ::2], torch.empty(3, 5, 4, 2).permute(3, 0, 1, 2)):
        assert TM.layout_status((2, 3, 5, 4), view.stride(), 10 ** 6) == 0, view.stride()
    assert TM.layout_status((2, 3, 5, 4), t.stride(), 120) == 0 and TM.layout_status((2, 3, 5, 4), t.stride(), 119) == E_NOSPACE
    assert TM.layout_status((2, 3, 5, 4), torch.empty(1, 3, 5, 4).expand(2, 3, 5, 4).stride(), 10 ** 6) == E_BADARG      # stride 0 over n == 2
    ext = (2, 3, 2, 3)
    for strides in itertools.product(range(0, 8), repeat=4):
        offs = [sum(i * s for i, s in zip(idx, strides)) for idx in itertools.product(*[range(e) for e in ext])]
        distinct = len(set(offs)) == len(offs)
        admitted = TM.layout_status(ext, strides, 10 ** 6) == 0
        assert not admitted or distinct, strides                         # the rule never admits an overlap
        if admitted:
            assert max(offs) + 1 <= 10 ** 6 and TM.layout_status(ext, strides, max(offs) + 1) == 0 and TM.layout_status(ext, strides, max(offs)) == E_NOSPACE


# ---- the entry's refusals, with a null context ---------------------------------------------------------------------------------------------
def test_the_entry_refuses_bad_arguments_before_the_context(J):
    """every call has a NULL context; with nothing bad the call gets as far as the context and says so"""
    lib = J.load_library()
    buf = np.zeros(4096, np.uint8)
    base = buf.ctypes.data
    assert base % 4 == 0
    n = 2
    data = (C.c_void_p * n)(base, base)
    lens = (C.c_size_t * n)(64, 64)
    infos, placed, status = (J.FrameInfo * n)(), (J.Rect * n)(), (C.c_int * n)()
    wins = (J.Window * n)(J.Window(J.Rect(0, 0, 4, 4), 1), J.Window(J.Rect(0, 0, 0, 0), 2))
    mirror = (C.c_uint8 * n)(1, 0)
    fl = lambda *v: (C.c_float * len(v))(*v)
    one, zero = fl(1, 1, 1), fl(0, 0, 0)

    # [2, 3, 4, 5] in float32, NCHW tight: strides (60, 20, 5, 1), 120 elements
    def call(n=n, data=data, lens=lens, gray=0, wins=wins, mirror=mirror, ow=5, oh=4, fmt=0, dt=1, ch=3, scale=one, bias=zero, st=(60, 20, 5, 1), out=base,
             cap=120, infos=infos, placed=placed, status=status):
        return lib.jpezy_decode_windows_tensor_dev(None, n, data, lens, gray, wins, mirror, ow, oh, fmt, dt, ch, scale, bias, *st, C.c_void_p(out), cap, infos,
                                                   placed, status)

    def reaches_the_context(**kw):
        assert call(**kw) == E_BADARG and "null context" in _err(lib), (kw, _err(lib))

    reaches_the_context()
    reaches_the_context(wins=None, placed=None, mirror=None, scale=None, bias=None)                        # the optional arrays may be null
    reaches_the_context(fmt=1)
    reaches_the_context(st=(60, 1, 15, 3))                                                                     # NHWC tight
    reaches_the_context(st=(3, 1, 30, 6))                                                                      # [H, W, n, C]: the rule has no fixed order
    reaches_the_context(st=(64, 21, 5, 1), cap=64 + 42 + 15 + 4 + 1)                                           # padded, cap at equality
    reaches_the_context(st=(60, 20, 5, 1), ow=1, oh=1, ch=1, gray=1, n=1, cap=1)                               # extents of 1: their strides are not looked at
    reaches_the_context(st=(0, 0, 0, 0), ow=1, oh=1, ch=1, gray=1, n=1, cap=1)
    reaches_the_context(ch=1, gray=1, st=(20, 0, 5, 1), cap=40)
    reaches_the_context(ow=65535, oh=65535, st=(3 * 65535 * 65535, 65535 * 65535, 65535, 1), cap=2 * 3 * 65535 * 65535)
    for dt, align in ((0, 1), (2, 2), (3, 2), (1, 4)):
        kw = dict(scale=None, bias=None) if dt == 0 else {}
        reaches_the_context(dt=dt, out=base + align, **kw)                                                     # aligned to the element, not to a vector
    reaches_the_context(scale=fl(2.0 ** -100, -2.0 ** 100, 0.0), bias=fl(-0.0, 2.0 ** 100, -2.0 ** -100))  # the band's edges, both signs, zero
    assert call(n=0, data=None, lens=None, infos=None, status=None, out=0, fmt=9, ow=0, dt=9, st=(-1, 0, 0, 0)) == 0      # n == 0: nothing is looked at
    cases = [
        (dict(n=-1), E_BADARG, "n must not be negative"),
        (dict(data=None), E_BADARG, "null pointer"), (dict(lens=None), E_BADARG, "null pointer"), (dict(infos=None), E_BADARG, "null pointer"),
        (dict(status=None), E_BADARG, "null pointer"), (dict(out=0), E_BADARG, "null pointer"),
        (dict(fmt=4), E_BADARG, "unknown pixel format"), (dict(fmt=-1), E_BADARG, "unknown pixel format"),
        (dict(fmt=2), E_BADARG, "alpha is never a tensor channel"), (dict(fmt=3), E_BADARG, "alpha is never a tensor channel"),
        (dict(ow=0), E_BADARG, "out_w and out_h"), (dict(oh=65536), E_BADARG, "out_w and out_h"),
        (dict(ch=2), E_BADARG, "channels must be 3 or 1"), (dict(ch=4), E_BADARG, "channels must be 3 or 1"), (dict(ch=0), E_BADARG, "channels must be 3 or 1"),
        (dict(ch=1, st=(20, 0, 5, 1)), E_BADARG, "needs gray"),
        (dict(dt=4), E_BADARG, "unknown element type"), (dict(dt=-1), E_BADARG, "unknown element type"),
        (dict(bias=None), E_BADARG, "together"), (dict(scale=None), E_BADARG, "together"),
        (dict(dt=0), E_BADARG, "JPEZY_DT_U8 takes no scale"),
        (dict(scale=fl(1, 2.0 ** -101, 1)), E_BADARG, "magnitude"), (dict(scale=fl(1, 1, 2.0 ** 101)), E_BADARG, "magnitude"),
        (dict(bias=fl(float("inf"), 0, 0)), E_BADARG, "magnitude"), (dict(bias=fl(0, float("nan"), 0)), E_BADARG, "magnitude"),
        (dict(scale=fl(-2.0 ** 101, 1, 1)), E_BADARG, "magnitude"), (dict(bias=fl(0, 0, 1e-45)), E_BADARG, "magnitude"),
        (dict(st=(60, 20, 5, -1)), E_BADARG, "must not be negative"), (dict(st=(-60, 20, 5, 1)), E_BADARG, "must not be negative"),
        (dict(st=(60, 20, 4, 1)), E_BADARG, "a place of its own"),                                            # sh = out_w - 1 with sw = 1
        (dict(st=(60, 20, 5, 0)), E_BADARG, "a place of its own"), (dict(st=(59, 20, 5, 1)), E_BADARG, "a place of its own"),
        (dict(st=(60, 19, 5, 1)), E_BADARG, "a place of its own"), (dict(st=(0, 20, 5, 1)), E_BADARG, "a place of its own"),
        (dict(st=(60, 1, 15, 2)), E_BADARG, "a place of its own"), (dict(st=(1, 1, 1, 1)), E_BADARG, "a place of its own"),
        (dict(cap=119), E_NOSPACE, "cap_elems"), (dict(cap=0), E_NOSPACE, "cap_elems"), (dict(st=(64, 21, 5, 1), cap=64 + 42 + 15 + 4), E_NOSPACE, "cap_elems"),
        (dict(st=(12, 4, 1, 1 << 62), cap=(1 << 64) - 1), E_NOSPACE, "cap_elems"),                                 # 4 * 2^62: the sum does not fit in 64 bits
        (dict(out=base + 2), E_BADARG, "aligned"), (dict(out=base + 1, dt=2), E_BADARG, "aligned"), (dict(out=base + 3, dt=3), E_BADARG, "aligned"),
        # which of two bad arguments is named: n, arrays, format, output size, channels, gray, dtype, scale / bias pair, U8 with a scale, the
        # values, negative strides, overlapping strides, capacity, alignment
        (dict(n=-1, data=None), E_BADARG, "n must not be negative"),
        (dict(data=None, fmt=9), E_BADARG, "null pointer"),
        (dict(fmt=9, ow=0), E_BADARG, "unknown pixel format"),
        (dict(fmt=2, ow=0), E_BADARG, "alpha"),
        (dict(ow=0, ch=2), E_BADARG, "out_w and out_h"),
        (dict(ch=2, dt=9), E_BADARG, "channels must be 3 or 1"),
        (dict(ch=1, dt=9), E_BADARG, "needs gray"),
        (dict(dt=9, bias=None), E_BADARG, "unknown element type"),
        (dict(dt=0, bias=None), E_BADARG, "together"),
        (dict(dt=0, scale=fl(0, 0, 1e38)), E_BADARG, "JPEZY_DT_U8 takes no scale"),
        (dict(scale=fl(1e38, 1, 1), st=(60, 20, 5, -1)), E_BADARG, "magnitude"),
        (dict(st=(60, 20, 4, -1)), E_BADARG, "must not be negative"),
        (dict(st=(60, 20, 4, 1), cap=1), E_BADARG, "a place of its own"),
        (dict(cap=119, out=base + 1), E_NOSPACE, "cap_elems"),
    ]
    for i, (kw, code, names) in enumerate(cases):
        assert call(**kw) == code, (i, kw, _err(lib))
        msg = _err(lib)
        assert names in msg and msg.startswith("decode_windows_tensor_dev:"), (i, kw, msg)
        st = kw.get("st", (60, 20, 5, 1))
        if names in ("must not be negative", "a place of its own", "cap_elems"):                               # the restated rule gives the same verdict
            assert TM.layout_status((2, kw.get("ch", 3), 4, 5), st, kw.get("cap", 120)) == code, (i, kw)
    assert (buf == 0).all()
