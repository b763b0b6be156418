"""Batch of windows, resized, straight into a tensor, on the GPU (include/jpezy_hip.h, BATCH OF WINDOWS, TENSOR OUTPUT;
Context.decode_windows_tensor_dev).  The expectation is tests/tensor_model.py (the restatement of the element conversion and the placement)
applied to tests/resize_model.py's resampling of the region restatement, i.e. to the bytes tests/test_gpu_windows_resized.py expects of
decode_windows_resized_dev.  The output tensor is a strided view of a marker-filled byte buffer with a tail of 16 bytes, and the WHOLE
buffer is compared as bytes: row padding, slot padding, the elements between strided ones, the slot of a file that failed, the other half
of a word next to a 2-byte element and the tail are all checked.  There is no tolerance: every comparison is np.array_equal."""
import numpy as np
import pytest

import region_smooth_cases as K
import resize_model as RM
import tensor_model as TM
import test_gpu_region as TR
import test_gpu_windows as TW
import test_gpu_windows_resized as TZ

pytestmark = pytest.mark.gpu

FILL = TR.FILL
TAIL = 16
J, torch, ctx, own_files = TZ.J, TZ.torch, TZ.ctx, TZ.own_files        # the fixtures of the resized tests: the same six encoder-made files

SIZES = [(1, 1), (3, 2), (4, 1), (5, 7), (64, 16), (65, 17), (130, 19)]   # a partial group of four; one tile; one past it in each axis; three tiles wide
DTYPES = [TM.DT_U8, TM.DT_F32, TM.DT_F16, TM.DT_BF16]
DT_NAMES = {TM.DT_U8: "uint8", TM.DT_F32: "float32", TM.DT_F16: "float16", TM.DT_BF16: "bfloat16"}
SCALE, BIAS = TM.normalization(TM.IMAGENET_MEAN, TM.IMAGENET_STD)


def strides_of(layout, n, C, H, W):
    """(sn, sc, sh, sw) in elements"""
    if layout == "nchw":
        return C * H * W, H * W, W, 1
    if layout == "nchw_rows":                                      # sh = W + 1: the alignment of a row's first element changes every row
        return C * H * (W + 1) + 3, H * (W + 1), W + 1, 1
    if layout == "nhwc":
        return H * W * C, 1, W * C, C
    if layout == "nhwc_rows":
        return H * (W * C + 1) + 2, 1, W * C + 1, C
    if layout == "sw2":                                            # neither form: single elements, every second one
        return C * H * 2 * W, H * 2 * W, 2 * W, 2
    raise ValueError(layout)


def run(J, torch, ctx, files, out, dt, layout, C=3, wins=None, mirror="alternate", fmt=None, gray=False, scale=None, bias=None, base=0, expect=None,
        smooth=False, **kw):
    """one call into a marker-filled buffer; the WHOLE buffer is compared as bytes with the expectation: the elements of file k where
    expect[k] == 0 (default: every file), the marker everywhere else.  Returns (the call's result list, the buffer as numpy bytes)."""
    n = len(files)
    ow, oh = out
    fmt = J.PIX_RGB24 if fmt is None else fmt
    if mirror == "alternate":
        mirror = [k % 2 for k in range(n)]                         # every second file
    st = strides_of(layout, n, C, oh, ow) if isinstance(layout, str) else layout
    eb = TM.ELEM_BYTES[dt]
    elems = base + sum((e - 1) * s for e, s in zip((n, C, oh, ow), st)) + 1
    buf = torch.full((elems * eb + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    d_out = buf[:elems * eb].view(getattr(torch, DT_NAMES[dt])).as_strided((n, C, oh, ow), st, base)
    res = ctx.decode_windows_tensor_dev(files, d_out, wins, mirror, scale, bias, format=fmt, gray=gray, raise_on_error=False, **kw)
    got = buf.cpu().numpy()
    exp = np.full(elems * eb + TAIL, FILL, np.uint8)
    exp_elems = exp[:elems * eb].view(TM.STORE[dt])
    for k in range(n):
        info, placed, status = res[k]
        assert status == (0 if expect is None else expect[k]), (k, status)
        if status != 0:
            continue
        reg, sc = TW.resolve(files[k], None if wins is None else wins[k])
        assert placed == reg, (k, placed, reg)
        flip = bool(mirror[k]) if mirror is not None else False
        if smooth:
            img = RM.resize(K.interleave(J, fmt, K.want(files[k], reg, sc, bool(gray))), ow, oh, flip)
        else:
            img = TZ.want_resized(files[k], reg, sc, bool(gray), fmt, ow, oh, flip)
        TM.place(exp_elems, base, st, k, img, dt, C, scale, bias)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, ("first differing byte", int(bad[0]), "element", int(bad[0]) // eb, "count", bad.size, "got", int(got[bad[0]]), "want",
                           int(exp[bad[0]]), out, layout, st)
    return res, got


def norm(dt):
    return {} if dt == TM.DT_U8 else dict(scale=SCALE, bias=BIAS)


# ---- 1. sizes x layouts x element types ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES, ids=[DT_NAMES[d] for d in DTYPES])
@pytest.mark.parametrize("layout", ["nchw", "nchw_rows", "nhwc", "nhwc_rows", "sw2"])
def test_sizes_layouts_and_element_types(J, torch, ctx, own_files, layout, dt):
    """every output size in every layout and element type, every second file mirrored, ImageNet normalisation for the float types.  With
    rows W + 1 elements apart the vector store and the single-element store both run in one image"""
    for out in SIZES:
        res, _ = run(J, torch, ctx, own_files, out, dt, layout, **norm(dt))
        assert ctx.last_batch_fast_count() == len(own_files)


# ---- 2. a base that is aligned to the element and not to the vector ---------------------------------------------------------------------
@pytest.mark.parametrize("dt", [TM.DT_F16, TM.DT_BF16, TM.DT_U8], ids=["float16", "bfloat16", "uint8"])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_base_offset_of_one_element(J, torch, ctx, own_files, layout, dt):
    for out in ((64, 16), (65, 17), (5, 7)):
        run(J, torch, ctx, own_files[:3], out, dt, layout, base=1, **norm(dt))


# ---- 3. mirror, channel order, gray -------------------------------------------------------------------------------------------------------
def test_mirror_is_the_column_reverse(J, torch, ctx, own_files):
    files = [f for f in own_files[:4] for _ in (0, 1)]
    out, n = (13, 6), 8
    _, got = run(J, torch, ctx, files, out, TM.DT_F32, "nchw", scale=SCALE, bias=BIAS)       # (mirror: every second file)
    t = got[:n * 3 * 6 * 13 * 4].view(np.uint32).reshape(n, 3, 6, 13)
    for k in range(0, n, 2):
        assert np.array_equal(t[k + 1], t[k][:, :, ::-1]), k


def test_bgr_is_rgb_with_the_channels_reversed(J, torch, ctx, own_files):
    out, n = (9, 5), len(own_files)
    for dt, layout in ((TM.DT_U8, "nchw"), (TM.DT_F16, "nhwc")):
        _, rgb = run(J, torch, ctx, own_files, out, dt, layout)
        _, bgr = run(J, torch, ctx, own_files, out, dt, layout, fmt=J.PIX_BGR24)
        shape = (n, 3, 5, 9) if layout == "nchw" else (n, 5, 9, 3)
        a, b = (g[:-TAIL].view(TM.STORE[dt]).reshape(shape) for g in (rgb, bgr))
        assert np.array_equal(b, a[:, ::-1] if layout == "nchw" else a[..., ::-1])


@pytest.mark.parametrize("C", [1, 3])
def test_gray(J, torch, ctx, own_files, C):
    """gray with one channel (byte 0) and with three (equal bytes), a one-component file beside three-component ones; with C == 1 "nhwc" has
    sc == sw == 1 and is the planar form"""
    files = own_files + [TR.jpeg("one_comp", 37, 21)]
    for dt, layout in ((TM.DT_U8, "nchw_rows"), (TM.DT_BF16, "nhwc"), (TM.DT_F16, "sw2"), (TM.DT_F32, "nchw")):
        s, b = (None, None) if dt == TM.DT_U8 else (SCALE[:C], BIAS[:C])
        _, got = run(J, torch, ctx, files, (10, 12), dt, layout, C=C, gray=True, scale=s, bias=b)
    if C == 3:                                                       # (the last call: float32, tight NCHW) one scale for all: equal channels
        _, got = run(J, torch, ctx, files, (10, 12), TM.DT_F32, "nchw", gray=True, scale=SCALE[[0, 0, 0]], bias=BIAS[[0, 0, 0]])
        t = got[:-TAIL].view(np.uint32).reshape(len(files), 3, 12, 10)
        assert np.array_equal(t[:, 0], t[:, 1]) and np.array_equal(t[:, 0], t[:, 2])
    with pytest.raises(J.JpezyError, match="needs gray"):
        ctx.decode_windows_tensor_dev(own_files[:1], torch.empty((1, 1, 4, 4), dtype=torch.uint8, device="cuda:0"))


# ---- 4. normalisation: the ranges of binary16 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale, bias", [(2.0 ** -20, 0.0), (300.0, 0.0), (-300.0, 7.0)], ids=["subnormals", "inf", "minus_inf"])
def test_f16_subnormals_and_overflow(J, torch, ctx, own_files, scale, bias):
    s, b = np.full(3, scale, np.float32), np.full(3, bias, np.float32)
    _, got = run(J, torch, ctx, own_files, (24, 24), TM.DT_F16, "nchw", scale=s, bias=b)
    bits = got[:-TAIL].view(np.uint16)
    if scale == 2.0 ** -20:                                          # bytes 1..63 are subnormal in binary16 and must not be flushed
        assert (((bits & 0x7C00) == 0) & ((bits & 0x3FF) != 0)).any() and ((bits & 0x7C00) != 0).any()
    else:
        assert (bits == (0x7C00 if scale > 0 else 0xFC00)).any() and ((bits & 0x7C00) != 0x7C00).any()


def test_imagenet_normalisation_in_f16(J, torch, ctx, own_files):
    """through tensor_normalization, into torch.empty(...), its channels_last form and a permuted NHWC tensor: the calls of the issue"""
    scale, bias = J.tensor_normalization(TM.IMAGENET_MEAN, TM.IMAGENET_STD)
    assert np.array_equal(scale, SCALE) and np.array_equal(bias, BIAS)
    n, H, W = len(own_files), 17, 20
    a = torch.empty(n, 3, H, W, dtype=torch.float16, device="cuda:0")
    b = torch.empty(n, 3, H, W, dtype=torch.float16, device="cuda:0").contiguous(memory_format=torch.channels_last)
    c = torch.empty(n, H, W, 3, dtype=torch.float16, device="cuda:0").permute(0, 3, 1, 2)
    want = np.zeros((n, 3, H, W), np.uint16)
    for k, f in enumerate(own_files):
        reg, sc = TW.resolve(f, None)
        img = TZ.want_resized(f, reg, sc, False, J.PIX_RGB24, W, H, False)
        for ch in range(3):
            want[k, ch] = TM.elements(img[:, :, ch], TM.DT_F16, scale[ch], bias[ch])
    for t in (a, b, c):
        res = ctx.decode_windows_tensor_dev(own_files, t, scale=scale, bias=bias)
        assert [st for _, _, st in res] == [0] * n
        assert np.array_equal(t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16), want)


# ---- 5. no model: the bytes of decode_windows_resized_dev -------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", [(65, 17), (5, 7)])
def test_u8_nhwc_equals_the_resized_call(J, torch, ctx, own_files, out):
    ow, oh = out
    n = len(own_files)
    mirror = [k % 2 for k in range(n)]
    row, slot = ow * 3 + 2, oh * (ow * 3 + 2) + 7
    packed = torch.full((n * slot + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    tensor = packed.clone()
    ctx.decode_windows_resized_dev(own_files, packed.as_strided((n, oh, ow, 3), (slot, row, 3, 1)), None, mirror)
    ctx.decode_windows_tensor_dev(own_files, tensor.as_strided((n, 3, oh, ow), (slot, 1, row, 3)), None, mirror)
    assert np.array_equal(tensor.cpu().numpy(), packed.cpu().numpy())


# ---- 6. failures ----------------------------------------------------------------------------------------------------------------------------
def test_a_failing_file_leaves_its_slot_alone(J, torch, ctx, own_files):
    cut = own_files[5][:len(own_files[5]) * 2 // 3]                # ends in mid-scan
    cut_rc, _ = TW.region_packed(J, ctx, cut, (0, 0, 30, 20), 1, J.PIX_RGB24)
    assert cut_rc < 0
    files = [own_files[3], own_files[4], cut, own_files[3], own_files[2]]
    wins = [((5, 3, 40, 20), 1), None, ((0, 0, 30, 20), 1), ((60, 0, 10, 10), 1), ((1, 1, 13, 7), 2)]
    expect = [0, 0, cut_rc, -1, 0]
    for dt, layout in ((TM.DT_F16, "nchw_rows"), (TM.DT_U8, "nhwc_rows"), (TM.DT_F32, "sw2")):
        res, _ = run(J, torch, ctx, files, (8, 6), dt, layout, wins=wins, expect=expect, **norm(dt))
        assert res[3][0].width == 64 and res[3][1] == (0, 0, 0, 0)
    d_out = torch.empty((5, 3, 6, 8), dtype=torch.float16, device="cuda:0")
    with pytest.raises(J.JpezyError, match=r"decode_windows_tensor_dev: file 2: "):
        ctx.decode_windows_tensor_dev(files, d_out, wins)
    with pytest.raises(J.JpezyError, match="d_out"):
        ctx.decode_windows_tensor_dev(own_files[:1], torch.zeros((1, 3, 4, 4), dtype=torch.float16))
    with pytest.raises(J.JpezyError, match="d_out"):
        ctx.decode_windows_tensor_dev(own_files[:1], torch.zeros((1, 3, 4, 4), dtype=torch.float64, device="cuda:0"))
    with pytest.raises(J.JpezyError, match="a place of its own"):
        ctx.decode_windows_tensor_dev(own_files[:2], torch.zeros((1, 3, 4, 4), dtype=torch.float16, device="cuda:0").expand(2, 3, 4, 4))
    with pytest.raises(J.JpezyError, match="alpha"):
        ctx.decode_windows_tensor_dev(own_files[:1], d_out[:1], format=J.PIX_RGBA32)
    with pytest.raises(J.JpezyError, match="takes no scale"):
        ctx.decode_windows_tensor_dev(own_files[:1], torch.zeros((1, 3, 4, 4), dtype=torch.uint8, device="cuda:0"), scale=SCALE, bias=BIAS)
    with pytest.raises(J.JpezyError, match="mirror"):
        ctx.decode_windows_tensor_dev(own_files[:1], d_out[:1], mirror=[0, 1])
    assert ctx.decode_windows_tensor_dev([], torch.zeros((0, 3, 4, 4), device="cuda:0")) == []


# ---- 7. paths -------------------------------------------------------------------------------------------------------------------------------
def test_slices_and_the_per_file_path_give_the_same_bytes(J, torch, ctx, own_files):
    rst = TR.jpeg("own", 101, 70, restart=2)                       # a restart interval: the child-context path
    assert TR.parsed(rst)[0].restart_interval == 2
    files = [own_files[3], rst, own_files[5], TR.jpeg("444", 37, 21), own_files[1], rst]
    wins = [((5, 3, 40, 20), 1), ((30, 9, 50, 29), 1), None, None, ((0, 0, 0, 0), 1), ((0, 0, 0, 0), 2)]
    for dt, layout in ((TM.DT_F16, "nchw_rows"), (TM.DT_BF16, "nhwc")):
        _, together = run(J, torch, ctx, files, (12, 10), dt, layout, wins=wins, **norm(dt))
        fast = ctx.last_batch_fast_count()
        assert 3 <= fast <= len(files) - 2                           # the restart-interval files went file by file
        try:
            for per_slice in (1, 2):
                ctx.set_windows_slice_files(per_slice)
                _, sliced = run(J, torch, ctx, files, (12, 10), dt, layout, wins=wins, **norm(dt))
                assert np.array_equal(sliced, together) and ctx.last_batch_fast_count() == fast
        finally:
            ctx.set_windows_slice_files(0)


# ---- 8. smooth upsampling of the source window ------------------------------------------------------------------------------------------------
def test_smooth_upsampling(J, torch, ctx, own_files):
    files = [own_files[5], own_files[3], K.jpeg("own", 40, 24, restart=2)]
    wins = [((7, 9, 150, 100), 1), ((0, 0, 0, 0), 2), ((3, 2, 30, 20), 1)]
    _, smooth = run(J, torch, ctx, files, (24, 24), TM.DT_F16, "nchw", wins=wins, smooth=True, upsampling=J.UPSAMPLE_SMOOTH, scale=SCALE, bias=BIAS)
    assert ctx.windows_upsampling() == J.UPSAMPLE_NEAREST
    _, nearest = run(J, torch, ctx, files, (24, 24), TM.DT_F16, "nchw", wins=wins, scale=SCALE, bias=BIAS)
    assert not np.array_equal(smooth, nearest)
