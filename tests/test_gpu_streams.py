"""What include/jpezy_hip.h promises of the *_dev entry points about streams, executed: asynchronous on the caller's stream and in its
order (P1), capturable and replayable (P2), and the written rules (P3) -- a table or scratch change is refused inside a capture and leaves
the capture alive, a change of tables between two streams waits for the device, the synchronous window-batch entries refuse a capture and
are complete on return.  The procedures are tests/stream_probe.py's; the expected bytes are the numpy models' and the oracle's
(tests/scaled_model.py, region_model.py, smooth_model.py, region_smooth_model.py, ycc_model.py, quant_model.py, sampling_model.py,
chroma_average_model.py, huffopt_model.py, resize_model.py, tensor_model.py), never another call of the entry under test.

Every case has two inputs A and B of one size, layout and set of tables: for the decoders B is A with every coefficient's sign flipped,
for the encoders two oracle.synth_rgb frames each.  Shapes are the smallest with the whole launch structure: 101 x 70 in jpezy's own
layout and 37 x 21 in 4:2:2 and h3_partial (partial MCUs on both edges, more than one workgroup) for the any-layout entries, 64 x 48 for
the fused ones, 40 x 24 for 4:4:4, 128 x 32 for averaged chroma; two frames wherever an entry takes a frame count, with planes
w * h + 4 bytes apart (rounded up to the multiple of 4 the any-layout batch entry asks for, where it is that entry).  The window is
(13, 9, 50, 29) of 101 x 70, (5, 3, 18, 9) of 37 x 21, and the pixels they cover at 1/4.

COVERAGE lists, for every method of jpezy_amd.api.Context that takes a stream, the tests that hold it to P1 and P2;
test_every_stream_taking_method_has_a_row needs no GPU and fails when a method with a stream parameter has no row."""
import ctypes as C
import fnmatch
import functools
import inspect

import numpy as np
import pytest

import chroma_average_model as CM
import huffopt_model as HM
import quant_model as QM
import region_smooth_model as RS
import sampling_model as SM
import scaled_model as M
import smooth_model as SMOOTH
import stream_probe as SP
import tensor_model as TM
import test_gpu_region as TR
import test_gpu_windows as TW
import test_gpu_windows_resized as TZ
import test_gpu_windows_tensor as TT
import ycc_model as YM

pytestmark = pytest.mark.gpu

FILL = SP.FILL
TAIL = 16                                                          # bytes behind what an entry writes: they keep the marker
SHAPES = [("own", 101, 70), ("422", 37, 21), ("h3_partial", 37, 21)]
WINDOW = {(101, 70): (13, 9, 50, 29), (37, 21): (5, 3, 18, 9)}


# ---- the table of the issue: which test holds which stream-taking method to P1 (stream order, asynchrony) and P2 (capture, replay) ----
COVERAGE = {
    "dequant_idct_generic_dev": ("test_stream_order[*-generic*]", "test_capture_replay[*-generic*]"),
    "dequant_idct_scaled_dev": ("test_stream_order[*-scaled*]", "test_capture_replay[*-scaled*]"),
    "dequant_idct_upsampling_dev": ("test_stream_order[*-upsampling*]", "test_capture_replay[*-upsampling*]"),
    "dequant_idct_region_dev": ("test_stream_order[*-region*]", "test_capture_replay[*-region*]"),
    "dequant_idct_dev": ("test_stream_order[fused-planes]", "test_capture_replay[fused-planes]"),
    "dequant_idct_packed_dev": ("test_stream_order[fused-packed]", "test_capture_replay[fused-packed]"),
    "dequant_idct_ycc_dev": ("test_stream_order[fused-ycc]", "test_capture_replay[fused-ycc]"),
    "fdct_quant_packed_dev": ("test_stream_order[encode-packed]", "test_capture_replay[encode-packed]"),
    "fdct_quant_ycc_dev": ("test_stream_order[encode-ycc]", "test_capture_replay[encode-ycc]"),
    "huffman_histogram_dev": ("test_stream_order[histogram]", "test_capture_replay[histogram]"),
    "fdct_quant_dev": ("test_stream_order[encode-444], test_stream_order[encode-average]",
                       "test_capture_replay[encode-444], test_capture_replay[encode-average]; 4:2:0: "
                       "test_gpu_entropy.py::test_device_resident_async_variant"),
    "write_jpeg_gpu_dev": ("test_stream_order[write-444]",
                           "test_capture_replay[write-444]; 4:2:0: test_gpu_entropy.py::test_device_resident_async_variant, "
                           "test_gpu_restart.py, test_gpu_quant.py::test_setter_is_refused_during_capture_and_the_device_writer_is_capturable"),
    "coeff_transform_dev": ("test_stream_order[transform]", "test_gpu_transform.py (the capture of two frames); test_capture_replay[transform]"),
}


def test_every_stream_taking_method_has_a_row():
    """no GPU: the methods are read from the class"""
    from jpezy_amd import api
    takes = {n for n, f in inspect.getmembers(api.Context, inspect.isfunction) if "stream" in inspect.signature(f).parameters}
    assert takes, "no method of Context takes a stream: the derivation is broken"
    assert takes == set(COVERAGE), ("stream-taking methods without a row", sorted(takes - set(COVERAGE)), "rows without a method",
                                    sorted(set(COVERAGE) - takes))
    ids = {f"{fn}[{c}]" for fn in ("test_stream_order", "test_capture_replay") for c in CASES}
    for method, cells in COVERAGE.items():
        for cell in cells:
            named = [w.strip(" ,;") for w in cell.split() if w.startswith("test_stream_order[") or w.startswith("test_capture_replay[")]
            assert named, (method, cell)
            for pat in named:
                assert fnmatch.filter(ids, pat.replace("[", "[[]", 1)), (method, "names no case of this module", pat)


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def delay(torch):
    return SP.Delay(torch, "cuda:0")


# ---- inputs and expectations of the decoders: made once, never modified ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coeffs(layout, W, H):
    """(FrameInfo, A, B): int16 [2, n] each -- the file's coefficients and their halves, and both with the sign flipped"""
    info, three = TR._three_frames(TR.jpeg(layout, W, H))
    a = np.ascontiguousarray(three[[0, 2]])
    b = (-a.astype(np.int32)).astype(np.int16)
    assert np.array_equal(b[0], three[1])
    for x in (a, b):
        x.setflags(write=False)
    return info, a, b


@functools.lru_cache(maxsize=None)
def pictures(layout, W, H, kind, scale):
    """{"A" | "B": [frame] of three (Hs, Ws) planes}: the whole picture of every frame under the model of `kind`"""
    info, a, b = coeffs(layout, W, H)
    ws, hs = M.scaled_size(W, H, scale)
    model = {"nearest": lambda co: M.decode_planes(co, info, scale, False),
             "smooth": lambda co: SMOOTH.decode_planes(co, info, False),
             "region_smooth": lambda co: RS.decode_picture(co, info, scale, False)}[kind]
    assert kind != "smooth" or scale == 1
    return {k: [[np.asarray(p).reshape(hs, ws) for p in model(x[f])] for f in range(2)] for k, x in (("A", a), ("B", b))}


def window_at(W, H, scale):
    """the window of the picture at full size, and the pixels of the picture at 1/scale it covers"""
    x, y, w, h = WINDOW[(W, H)]
    x0, y0, x1, y1 = x // scale, y // scale, -(-(x + w) // scale), -(-(y + h) // scale)
    return x0, y0, x1 - x0, y1 - y0


def cut(pics, region):
    x, y, w, h = region
    return {k: [[p[y:y + h, x:x + w] for p in frame] for frame in v] for k, v in pics.items()}


def align4(n):
    return (n + 3) & ~3


def planar_probe(torch, name, src, pics, n, stride, call):
    """src = (A, B) coefficients [2, ncoef]; pics = {"A" | "B": [frame][plane]}; call(d_co, planes, stream)"""
    a, b = src[0][:n], src[1][:n]
    d_co = torch.empty(a.shape, dtype=torch.int16, device="cuda:0")
    outs = [torch.empty(n * stride + TAIL, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    expect = {k: SP.planes_buffers(v[:n], stride, TAIL) for k, v in pics.items()}
    return SP.Probe(torch, name, [(d_co, a, b)], outs, lambda s: call(d_co, outs, s), expect)


def packed_probe(torch, J, name, src, pics, fmt, call):
    """two frames of packed pixels with padded rows and a padded frame; call(d_co, d_img, stream)"""
    nb = 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4
    h, w = pics["A"][0][0].shape
    rs = w * nb + 5
    fs = align4(h * rs) + 4
    d_co = torch.empty(src[0].shape, dtype=torch.int16, device="cuda:0")
    buf = torch.empty(2 * fs + TAIL, dtype=torch.uint8, device="cuda:0")
    d_img = buf.as_strided((2, h, w, nb), (fs, rs, nb, 1))
    expect = {k: SP.packed_buffer([TR._interleave(J, fmt, frame) for frame in v], rs, fs, TAIL) for k, v in pics.items()}
    return SP.Probe(torch, name, [(d_co, src[0], src[1])], [buf], lambda s: call(d_co, d_img, s), expect)


def _shape_cases(out, layout, W, H, fmt_name):
    """the cases of one file: a function of its own, so that every builder closes over this file's values"""
    n1 = W * H
    batch = align4(n1 + 4)                                         # the any-layout batch entry asks for a multiple of 4

    def add(name, build):
        def make(torch, J, ctx):
            info, a, b = coeffs(layout, W, H)
            return build(torch, J, ctx, info, (a, b), getattr(J, fmt_name))
        out[f"{layout}{W}x{H}-{name}"] = make

    def pics(kind, scale=1, region=None):
        p = pictures(layout, W, H, kind, scale)
        return p if region is None else cut(p, region)

    add("generic", lambda torch, J, ctx, info, src, fmt: planar_probe(
        torch, "dequant_idct_generic_dev", src, pics("nearest"), 1, n1,
        lambda d_co, o, s: ctx.dequant_idct_generic_dev(d_co, info, *[t[:n1] for t in o], stream=s)))
    add("generic-batch", lambda torch, J, ctx, info, src, fmt: planar_probe(
        torch, "dequant_idct_generic_dev n_frames=2", src, pics("nearest"), 2, batch,
        lambda d_co, o, s: ctx.dequant_idct_generic_dev(d_co, info, *o, stream=s, n_frames=2, plane_stride=batch)))
    add("upsampling", lambda torch, J, ctx, info, src, fmt: planar_probe(
        torch, "dequant_idct_upsampling_dev", src, pics("smooth"), 2, batch,
        lambda d_co, o, s: ctx.dequant_idct_upsampling_dev(d_co, info, *o, stream=s, n_frames=2, plane_stride=batch)))
    add("upsampling-packed", lambda torch, J, ctx, info, src, fmt: packed_probe(
        torch, J, "dequant_idct_upsampling_dev packed", src, pics("smooth"), fmt,
        lambda d_co, d_img, s: ctx.dequant_idct_upsampling_dev(d_co, info, stream=s, d_img=d_img, format=fmt)))

    def scaled(scale):
        ws, hs = M.scaled_size(W, H, scale)
        stride = align4(ws * hs + 4) if scale == 1 else ws * hs + 4          # scale 1 is the any-layout batch entry
        add(f"scaled{scale}", lambda torch, J, ctx, info, src, fmt: planar_probe(
            torch, f"dequant_idct_scaled_dev 1/{scale}", src, pics("nearest", scale), 2, stride,
            lambda d_co, o, s: ctx.dequant_idct_scaled_dev(d_co, info, scale, *o, stream=s, n_frames=2, plane_stride=stride)))
        add(f"scaled{scale}-packed", lambda torch, J, ctx, info, src, fmt: packed_probe(
            torch, J, f"dequant_idct_scaled_dev 1/{scale} packed", src, pics("nearest", scale), fmt,
            lambda d_co, d_img, s: ctx.dequant_idct_scaled_dev(d_co, info, scale, stream=s, d_img=d_img, format=fmt)))

    def region(scale, mode, kind, up):
        rg = window_at(W, H, scale)
        stride = rg[2] * rg[3] + 4
        add(f"region{scale}-{mode}", lambda torch, J, ctx, info, src, fmt: planar_probe(
            torch, f"dequant_idct_region_dev 1/{scale} {up}", src, pics(kind, scale, rg), 2, stride,
            lambda d_co, o, s: ctx.dequant_idct_region_dev(d_co, info, rg, scale, *o, stream=s, n_frames=2, plane_stride=stride,
                                                           upsampling=getattr(J, up))))
        add(f"region{scale}-{mode}-packed", lambda torch, J, ctx, info, src, fmt: packed_probe(
            torch, J, f"dequant_idct_region_dev 1/{scale} {up} packed", src, pics(kind, scale, rg), fmt,
            lambda d_co, d_img, s: ctx.dequant_idct_region_dev(d_co, info, rg, scale, stream=s, d_img=d_img, format=fmt,
                                                               upsampling=getattr(J, up))))

    for scale in (1, 4):
        scaled(scale)
        region(scale, "replicated", "nearest", "UPSAMPLE_NEAREST")
        region(scale, "smooth", "region_smooth", "UPSAMPLE_SMOOTH")


def any_layout_cases():
    """{id: builder(torch, J, ctx) -> Probe} of the generic, scaled, upsampling and region entries, planes and packed"""
    out = {}
    fmts = {"own": "PIX_BGRA32", "422": "PIX_RGB24", "h3_partial": "PIX_RGBA32"}
    for layout, W, H in SHAPES:
        _shape_cases(out, layout, W, H, fmts[layout])
    return out


# ---- the fused decoders of jpezy's own layout, 64 x 48 -----------------------------------------------------------------------------------
FW, FH = 64, 48


def fused_planes(torch, J, ctx):
    info, a, b = coeffs("own", FW, FH)
    stride = FW * FH + 4
    tq = tuple(info.Tq[i] for i in range(3))
    return planar_probe(torch, "dequant_idct_dev", (a, b), pictures("own", FW, FH, "nearest", 1), 2, stride,
                        lambda d_co, o, s: ctx.dequant_idct_dev(d_co, FW, FH, *o, qt=info.qt, comp_tq=tq, n_frames=2, plane_stride=stride, stream=s))


def fused_packed(torch, J, ctx):
    info, a, b = coeffs("own", FW, FH)
    tq = tuple(info.Tq[i] for i in range(3))
    return packed_probe(torch, J, "dequant_idct_packed_dev", (a, b), pictures("own", FW, FH, "nearest", 1), J.PIX_BGR24,
                        lambda d_co, d_img, s: ctx.dequant_idct_packed_dev(d_co, d_img, format=J.PIX_BGR24, qt=info.qt, comp_tq=tq, stream=s))


def fused_ycc(torch, J, ctx):
    """two frames of Y, Cb, Cr at their native sampling, frames 4 bytes further apart than a plane"""
    info, a, b = coeffs("own", FW, FH)
    tq = tuple(info.Tq[i] for i in range(3))
    cw, ch = YM.chroma_size(FW, FH)
    sizes = [(FH, FW), (ch, cw), (ch, cw)]
    d_co = torch.empty(a.shape, dtype=torch.int16, device="cuda:0")
    bufs = [torch.empty(2 * (h * w + 4) + TAIL, dtype=torch.uint8, device="cuda:0") for h, w in sizes]
    views = [t.as_strided((2, h, w), (h * w + 4, w, 1)) for t, (h, w) in zip(bufs, sizes)]
    expect = {}
    for k, x in (("A", a), ("B", b)):
        want = [SP.marker(t.numel()) for t in bufs]
        for f in range(2):
            for c, p in enumerate(YM.decode_planes(x[f], info)):
                h, w = sizes[c]
                assert p.shape == (h, w)
                want[c][f * (h * w + 4):f * (h * w + 4) + h * w] = p.reshape(-1)
        expect[k] = [(w_, None) for w_ in want]
    return SP.Probe(torch, "dequant_idct_ycc_dev", [(d_co, a, b)], bufs,
                    lambda s: ctx.dequant_idct_ycc_dev(d_co, *views, qt=info.qt, comp_tq=tq, stream=s), expect)


# ---- the encoders: two oracle.synth_rgb frames for A, two more for B ---------------------------------------------------------------------
def rgb_frames(W, H, which):
    from oracle import oracle as O
    return [O.synth_rgb(W, H, frame=f) for f in ((0, 1) if which == "A" else (2, 3))]


def coeff_expect(frames, tail_elems=8):
    """int16 coefficients of the frames, one behind the other, and the marker behind them"""
    body = np.concatenate([np.asarray(f, np.int16).reshape(-1) for f in frames])
    return body.size + tail_elems, [(np.concatenate([body.view(np.uint8), SP.marker(2 * tail_elems)]), None)]


def encode_packed(torch, J, ctx):
    from oracle import oracle as O
    imgs, expect = {}, {}
    for k in "AB":
        fr = rgb_frames(FW, FH, k)
        imgs[k] = np.stack([np.stack([p.reshape(FH, FW) for p in f], axis=-1) for f in fr])
        elems, expect[k] = coeff_expect([O.encode_coeffs(*f, FW, FH) for f in fr])
    d_img = torch.empty(imgs["A"].shape, dtype=torch.uint8, device="cuda:0")
    d_co = torch.empty(elems, dtype=torch.int16, device="cuda:0")
    return SP.Probe(torch, "fdct_quant_packed_dev", [(d_img, imgs["A"], imgs["B"])], [d_co],
                    lambda s: ctx.fdct_quant_packed_dev(d_img, d_co, format=J.PIX_RGB24, stream=s), expect)


def encode_ycc(torch, J, ctx):
    planes, expect = {}, {}
    for k, frames in (("A", (0, 1)), ("B", (2, 3))):
        fr = [YM.synth_planes(FW, FH, "random", f) for f in frames]
        planes[k] = [np.stack([f[c] for f in fr]) for c in range(3)]
        elems, expect[k] = coeff_expect([YM.encode_coeffs(*f) for f in fr])
    d = [torch.empty(p.shape, dtype=torch.uint8, device="cuda:0") for p in planes["A"]]
    d_co = torch.empty(elems, dtype=torch.int16, device="cuda:0")
    return SP.Probe(torch, "fdct_quant_ycc_dev", [(d[c], planes["A"][c], planes["B"][c]) for c in range(3)], [d_co],
                    lambda s: ctx.fdct_quant_ycc_dev(d[0], d[1], d[2], d_co, stream=s), expect)


def _planar_encoder(torch, name, W, H, model, call):
    """fdct_quant_dev on two frames whose planes lie W * H + 4 bytes apart; model(r, g, b) -> the frame's coefficients"""
    stride = W * H + 4
    planes, expect = {}, {}
    for k in "AB":
        fr = rgb_frames(W, H, k)
        planes[k] = []
        for c in range(3):
            p = np.zeros(2 * stride, np.uint8)
            for f in range(2):
                p[f * stride:f * stride + W * H] = fr[f][c]
            planes[k].append(p)
        elems, expect[k] = coeff_expect([model(*f) for f in fr])
    d = [torch.empty(2 * stride, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    d_co = torch.empty(elems, dtype=torch.int16, device="cuda:0")
    return SP.Probe(torch, name, [(d[c], planes["A"][c], planes["B"][c]) for c in range(3)], [d_co], lambda s: call(d, d_co, stride, s), expect)


def encode_444(torch, J, ctx):
    W, H = 40, 24
    luma, chroma = QM.tables("q50")
    return _planar_encoder(torch, "fdct_quant_dev SAMPLING_444", W, H, lambda r, g, b: SM.encode_coeffs(r, g, b, W, H, luma, chroma),
                           lambda d, d_co, stride, s: ctx.fdct_quant_dev(*d, W, H, d_co, n_frames=2, plane_stride=stride, stream=s,
                                                                         sampling=J.SAMPLING_444))


def encode_average(torch, J, ctx):
    """(the context is in DOWNSAMPLE_AVERAGE while this probe is used: the averaged fixture)"""
    W, H = 128, 32
    luma, chroma = QM.tables("q50")
    return _planar_encoder(torch, "fdct_quant_dev DOWNSAMPLE_AVERAGE", W, H, lambda r, g, b: CM.encode_coeffs(r, g, b, W, H, luma, chroma),
                           lambda d, d_co, stride, s: ctx.fdct_quant_dev(*d, W, H, d_co, n_frames=2, plane_stride=stride, stream=s))


def write_444(torch, J, ctx):
    """two 4:4:4 files into slots of jpeg_bound bytes: the files, their sizes and the bytes behind the last slot are compared (what lies
    between a file's end and its slot's is not defined)"""
    W, H = 40, 24
    luma, chroma = QM.tables("q50")
    stride = J.jpeg_bound(W, H, J.SAMPLING_444)
    co, expect = {}, {}
    for k in "AB":
        fr = [SM.encode_coeffs(*f, W, H, luma, chroma) for f in rgb_frames(W, H, k)]
        co[k] = np.stack([f.reshape(-1) for f in fr])
        want, mask = SP.marker(2 * stride + TAIL), np.zeros(2 * stride + TAIL, bool)
        mask[2 * stride:] = True
        lens = []
        for f in range(2):
            jpg = np.frombuffer(SM.write_jpeg(fr[f], W, H), np.uint8)
            assert jpg.size < stride
            want[f * stride:f * stride + jpg.size] = jpg
            mask[f * stride:f * stride + jpg.size] = True
            lens.append(jpg.size)
        sizes = np.concatenate([np.array(lens, np.int64).view(np.uint8), SP.marker(16)])
        expect[k] = [(want, mask), (sizes, None)]
    d_co = torch.empty(co["A"].shape, dtype=torch.int16, device="cuda:0")
    d_out = torch.empty(2 * stride + TAIL, dtype=torch.uint8, device="cuda:0")
    d_sizes = torch.empty(4, dtype=torch.int64, device="cuda:0")
    return SP.Probe(torch, "write_jpeg_gpu_dev SAMPLING_444", [(d_co, co["A"], co["B"])], [d_out, d_sizes],
                    lambda s: ctx.write_jpeg_gpu_dev(d_co, W, H, d_out[:2 * stride], d_sizes[:2], n_frames=2, stream=s, sampling=J.SAMPLING_444),
                    expect)


def histogram(torch, J, ctx):
    from oracle import oracle as O
    co, expect = {}, {}
    for k in "AB":
        fr = [O.encode_coeffs(*f, FW, FH) for f in rgb_frames(FW, FH, k)]
        co[k] = np.stack([np.asarray(f, np.int16).reshape(-1) for f in fr])
        counts = []
        for f in fr:
            h, ok = HM.symbol_counts_np(f)
            assert ok
            counts.append(h.astype(np.int64).reshape(-1))
        expect[k] = [(np.concatenate([np.concatenate(counts).view(np.uint8), SP.marker(32)]), None)]
    d_co = torch.empty(co["A"].shape, dtype=torch.int16, device="cuda:0")
    d_hist = torch.empty(2 * 1024 + 4, dtype=torch.int64, device="cuda:0")
    return SP.Probe(torch, "huffman_histogram_dev", [(d_co, co["A"], co["B"])], [d_hist],
                    lambda s: ctx.huffman_histogram_dev(d_co, FW, FH, d_hist[:2048].view(2, 4, 256), n_frames=2, stream=s), expect)


def transform(torch, J, ctx):
    """coeff_transform_dev, which test_gpu_transform.py captures: here on a side stream behind a delay too"""
    import transform_model as XM
    from oracle import oracle as O
    W, H = FW, FH
    co, expect = {}, {}
    for k in "AB":
        fr = [np.asarray(O.encode_coeffs(*f, W, H), np.int16) for f in rgb_frames(W, H, k)]
        co[k] = np.stack([f.reshape(-1) for f in fr])
        elems, expect[k] = coeff_expect([XM.transform_field(f, W, H, XM.S420, J.XFORM_ROT90)[0] for f in fr])
    d_in = torch.empty(co["A"].shape, dtype=torch.int16, device="cuda:0")
    d_out = torch.empty(elems, dtype=torch.int16, device="cuda:0")
    return SP.Probe(torch, "coeff_transform_dev", [(d_in, co["A"], co["B"])], [d_out],
                    lambda s: ctx.coeff_transform_dev(d_in, W, H, d_out, J.XFORM_ROT90, n_frames=2, stream=s), expect)


CASES = {**any_layout_cases(), "fused-planes": fused_planes, "fused-packed": fused_packed, "fused-ycc": fused_ycc, "encode-packed": encode_packed,
         "encode-ycc": encode_ycc, "encode-444": encode_444, "encode-average": encode_average, "write-444": write_444, "histogram": histogram,
         "transform": transform}


@pytest.fixture
def probe(request, torch, J, ctx):
    """the case's Probe; the context is put into the chroma mode the case is about and handed back at its default"""
    case = request.param
    if case == "encode-average":
        ctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
    yield CASES[case](torch, J, ctx)
    torch.cuda.synchronize()
    ctx.set_chroma_downsampling(J.DOWNSAMPLE_POINT)


# ---- P1, P2 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe", sorted(CASES), indirect=True)
def test_stream_order(torch, delay, probe):
    """P1: behind a delay and the copy of input B on its own stream the call returns while the delay runs and writes B's bytes"""
    SP.stream_order(torch, delay, probe)


@pytest.mark.parametrize("probe", ["own101x70-generic"], indirect=True)
def test_probe_fails_on_a_wrong_stream(torch, delay, probe):
    """the control of P1, once: the call on an idle second stream reads input A while the copy of B waits behind the delay -- the output
    is A's, which test_stream_order would report.  A stale read by construction; nothing is read or written outside a buffer."""
    SP.wrong_stream(torch, delay, probe)


@pytest.mark.parametrize("probe", sorted(CASES), indirect=True)
def test_capture_replay(torch, probe):
    """P2: one call captured on a side stream (one stream, no branches), replayed on A, B, A"""
    SP.capture_replay(torch, probe)


# ---- P3: the written rules ------------------------------------------------------------------------------------------------------------------
def other_tables(info, J):
    """a copy of the FrameInfo with every quantiser 3 * q / 2 + 1: another set of tables for the same coefficients"""
    other = J.FrameInfo()
    C.memmove(C.byref(other), C.byref(info), C.sizeof(J.FrameInfo))
    for t in range(4):
        for i in range(64):
            other.qt[t][i] = min(255, info.qt[t][i] * 3 // 2 + 1)
    return other


def check(torch, outs, expect, what):
    for k, (o, (want, mask)) in enumerate(zip(outs, expect)):
        got = o.view(torch.uint8).reshape(-1).cpu().numpy()
        bad = np.nonzero(got != want if mask is None else (got != want) & mask)[0]
        assert bad.size == 0, (what, "output", k, "bytes that differ", bad.size, "first", int(bad[0]), "got", int(got[bad[0]]), "want", int(want[bad[0]]))


def refill(torch, outs):
    for o in outs:
        o.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()


def untouched(torch, outs):
    return all(bool((o.view(torch.uint8) == FILL).all()) for o in outs)


TABLE_RULE = ["dequant_idct_dev", "dequant_idct_generic_dev", "dequant_idct_region_dev"]


@pytest.mark.parametrize("entry", TABLE_RULE)
def test_new_tables_are_refused_inside_a_capture(J, torch, entry):
    """after a warm call with tables T1, a call with T2 inside a capture is JPEZY_E_BADARG and says why; the capture goes on, a T1 call is
    captured behind the refusal and the graph replays to T1's bytes; afterwards the context decodes with T1 and with T2"""
    W, H = (FW, FH) if entry == "dequant_idct_dev" else (101, 70)
    info, a, _ = coeffs("own", W, H)
    infos = {"T1": info, "T2": other_tables(info, J)}
    region = window_at(W, H, 1) if entry == "dequant_idct_region_dev" else (0, 0, W, H)
    n = region[2] * region[3]
    stride = align4(n + 4)
    model = lambda fi: [[p.reshape(H, W)[region[1]:region[1] + region[3], region[0]:region[0] + region[2]] for p in M.decode_planes(a[f], fi, 1, False)]
                        for f in range(2)]
    expect = {k: SP.planes_buffers(model(fi), stride, TAIL) for k, fi in infos.items()}
    assert any((x[0] != y[0]).any() for x, y in zip(expect["T1"], expect["T2"]))
    c = J.Context(0)
    try:
        d_co = torch.from_numpy(np.array(a)).to("cuda:0")
        outs = [torch.empty(2 * stride + TAIL, dtype=torch.uint8, device="cuda:0") for _ in range(3)]

        def call(which, stream):
            fi = infos[which]
            if entry == "dequant_idct_dev":
                c.dequant_idct_dev(d_co, W, H, *outs, qt=fi.qt, comp_tq=tuple(fi.Tq[i] for i in range(3)), n_frames=2, plane_stride=stride, stream=stream)
            elif entry == "dequant_idct_generic_dev":
                c.dequant_idct_generic_dev(d_co, fi, *outs, stream=stream, n_frames=2, plane_stride=stride)
            else:
                c.dequant_idct_region_dev(d_co, fi, region, 1, *outs, stream=stream, n_frames=2, plane_stride=stride)
        s = torch.cuda.Stream()
        refill(torch, outs)
        call("T1", s.cuda_stream)                                  # tables and scratch: outside the capture
        torch.cuda.synchronize()
        check(torch, outs, expect["T1"], "warm call with T1")
        refill(torch, outs)
        g = torch.cuda.CUDAGraph()
        refused = None
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                try:
                    call("T2", s.cuda_stream)
                except J.JpezyError as e:
                    refused = str(e)
                call("T1", s.cuda_stream)
        assert refused is not None and "status -1" in refused and "captured" in refused, refused
        torch.cuda.synchronize()
        assert untouched(torch, outs), "something ran during the capture"
        g.replay()
        torch.cuda.synchronize()
        check(torch, outs, expect["T1"], "replay of the T1 call captured behind the refusal")
        for which in ("T1", "T2", "T1"):                           # no re-upload mishap: the cache still says T1, then follows the caller
            refill(torch, outs)
            call(which, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            check(torch, outs, expect[which], f"default-stream call with {which} after the capture")
    finally:
        torch.cuda.synchronize()
        c.close()


def test_change_of_tables_between_two_streams_decode_side(J, torch, delay):
    """the decode twin of test_gpu_quant.py::test_change_of_tables_between_two_streams: dequant_idct_generic_dev with T1 on one stream
    -- behind a delay, so that its launches are certainly pending -- and at once with T2 on another, no synchronisation between the two.
    The second call rewrites the context's tables only after the whole device has drained (include/jpezy_hip.h, Streams), which also ends
    the first call's use of the context's sample scratch: one context serves both, as the header's 'one call in flight' allows."""
    W, H = 101, 70
    info, a, _ = coeffs("own", W, H)
    infos = {"T1": info, "T2": other_tables(info, J)}
    expect = {k: SP.planes_buffers([M.decode_planes(a[0], fi, 1, False)], W * H, TAIL) for k, fi in infos.items()}
    assert any((x[0] != y[0]).any() for x, y in zip(expect["T1"], expect["T2"]))
    c = J.Context(0)
    try:
        d_co = torch.from_numpy(np.array(a[0])).to("cuda:0")
        outs = {k: [torch.empty(W * H + TAIL, dtype=torch.uint8, device="cuda:0") for _ in range(3)] for k in infos}
        c.dequant_idct_generic_dev(d_co, infos["T1"], *[o[:W * H] for o in outs["T1"]])      # scratch and code: before the two calls
        refill(torch, outs["T1"] + outs["T2"])
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(s1):
            delay.queue(20.0)
        c.dequant_idct_generic_dev(d_co, infos["T1"], *[o[:W * H] for o in outs["T1"]], stream=s1.cuda_stream)
        c.dequant_idct_generic_dev(d_co, infos["T2"], *[o[:W * H] for o in outs["T2"]], stream=s2.cuda_stream)
        torch.cuda.synchronize()
        check(torch, outs["T1"], expect["T1"], "the call issued with T1")
        check(torch, outs["T2"], expect["T2"], "the call issued with T2")
    finally:
        torch.cuda.synchronize()
        c.close()


# ---- a cold context inside a capture ----------------------------------------------------------------------------------------------------------
def _capture_refusal(J, torch, call):
    """call() inside a capture on a side stream, beside one torch operation -> (the refusal's text or None, whether the graph replays)"""
    tick = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    refused = None
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            try:
                call(s.cuda_stream)
            except J.JpezyError as e:
                refused = str(e)
            tick.add_(1)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    return refused, int(tick[0]) == 1


def test_cold_generic_decoder_is_refused_inside_a_capture(J, torch):
    """the any-layout decoder's samples live in the context and grow by a free and an allocation, which a capture forbids: the first call
    of a context, and the first that needs more scratch, is JPEZY_E_BADARG inside a capture before anything is touched -- the capture
    stays valid, the outputs keep the marker, and the same call outside a capture then decodes"""
    W, H = 101, 70
    info, a, _ = coeffs("own", W, H)
    pics = pictures("own", W, H, "nearest", 1)["A"]
    stride = align4(W * H + 4)
    c = J.Context(0)
    try:
        d_co = torch.from_numpy(np.array(a)).to("cuda:0")
        outs = [torch.empty(2 * stride + TAIL, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        one = lambda s: c.dequant_idct_generic_dev(d_co, info, *[o[:W * H] for o in outs], stream=s)
        two = lambda s: c.dequant_idct_generic_dev(d_co, info, *outs, stream=s, n_frames=2, plane_stride=stride)
        for what, call, frames in (("first call of the context", one, pics[:1]), ("first call with two frames", two, pics)):
            refill(torch, outs)
            refused, alive = _capture_refusal(J, torch, call)
            assert refused is not None and "status -1" in refused and "captured" in refused, (what, refused)
            assert alive, (what, "the capture did not survive the refusal")
            assert untouched(torch, outs), what
            call(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            check(torch, outs, SP.planes_buffers(frames, stride, TAIL + (2 - len(frames)) * stride), what + ", outside a capture")
        refill(torch, outs)
        refused, alive = _capture_refusal(J, torch, two)             # warm now: captured, and the replay inside the helper decoded
        assert refused is None and alive
        check(torch, outs, SP.planes_buffers(pics, stride, TAIL), "the warm call, captured and replayed")
    finally:
        torch.cuda.synchronize()
        c.close()


def test_cold_entropy_coder_is_refused_inside_a_capture(J, torch, oracle):
    """the same for write_jpeg_gpu_dev, whose code tables, header and scratch are the context's"""
    W, H = FW, FH
    frames = [oracle.synth_rgb(W, H, frame=f) for f in (0, 1)]
    co = [np.asarray(oracle.encode_coeffs(*f, W, H), np.int16).reshape(-1) for f in frames]
    want = [np.frombuffer(oracle.write_jpeg(x, W, H), np.uint8) for x in co]
    stride = J.jpeg_bound(W, H)
    c = J.Context(0)
    try:
        d_co = torch.from_numpy(np.stack(co)).to("cuda:0")
        d_out = torch.empty(2 * stride + TAIL, dtype=torch.uint8, device="cuda:0")
        d_sizes = torch.empty(4, dtype=torch.int64, device="cuda:0")
        outs = [d_out, d_sizes]
        one = lambda s: c.write_jpeg_gpu_dev(d_co, W, H, d_out[:stride], d_sizes[:1], n_frames=1, stream=s)
        two = lambda s: c.write_jpeg_gpu_dev(d_co, W, H, d_out[:2 * stride], d_sizes[:2], n_frames=2, stream=s)

        def files_ok(n, what):
            got, sizes = d_out.cpu().numpy(), d_sizes.cpu().numpy()
            for f in range(n):
                assert int(sizes[f]) == want[f].size and np.array_equal(got[f * stride:f * stride + want[f].size], want[f]), (what, f)
            assert (got[n * stride:] == FILL).all() and (sizes[n:].view(np.uint8) == FILL).all(), what
        for what, call, n in (("first call of the context", one, 1), ("first call with two frames", two, 2)):
            refill(torch, outs)
            refused, alive = _capture_refusal(J, torch, call)
            assert refused is not None and "status -1" in refused and "captured" in refused, (what, refused)
            assert alive, (what, "the capture did not survive the refusal")
            assert untouched(torch, outs), what
            call(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            files_ok(n, what + ", outside a capture")
        refill(torch, outs)
        refused, alive = _capture_refusal(J, torch, two)
        assert refused is None and alive
        files_ok(2, "the warm call, captured and replayed")
    finally:
        torch.cuda.synchronize()
        c.close()


# ---- the synchronous window-batch entries -------------------------------------------------------------------------------------------------------
WIN_FILES = [("own", 101, 70), ("422", 37, 21), ("own", 37, 21)]
WINS = [((13, 9, 50, 29), 1), ((0, 0, 0, 0), 1), ((0, 0, 0, 0), 2)]
WIN_SLOT = (50, 29)                                                # (Ws, Hs) of decode_windows_dev's slots
WIN_OUT = (16, 12)                                                 # (out_w, out_h) of the resized forms


def _window_call(J, torch, ctx, entry):
    """-> (buffer, call(), expectation of the whole buffer) of one window-batch entry on the three files"""
    files = [TR.jpeg(*f) for f in WIN_FILES]
    fmt = J.PIX_RGB24
    regs = [TW.resolve(f, w) for f, w in zip(files, WINS)]
    if entry == "decode_windows_dev":
        ws, hs = WIN_SLOT
        row, slot = ws * 3 + 5, hs * (ws * 3 + 5) + 7
        buf = torch.empty(3 * slot + TAIL, dtype=torch.uint8, device="cuda:0")
        d_out = buf.as_strided((3, hs, ws, 3), (slot, row, 3, 1))
        exp = SP.marker(3 * slot + TAIL)
        for k, (reg, scale) in enumerate(regs):
            img = TW.want_img(files[k], reg, scale, False, fmt)
            for j in range(reg[3]):
                exp[k * slot + j * row:k * slot + j * row + reg[2] * 3] = img[j].reshape(-1)
        return buf, lambda: ctx.decode_windows_dev(files, d_out, WINS, format=fmt), exp
    ow, oh = WIN_OUT
    mirror = [0, 1, 0]
    imgs = [TZ.want_resized(files[k], reg, scale, False, fmt, ow, oh, bool(mirror[k])) for k, (reg, scale) in enumerate(regs)]
    if entry == "decode_windows_resized_dev":
        row, slot = ow * 3 + 5, oh * (ow * 3 + 5) + 7
        buf = torch.empty(3 * slot + TAIL, dtype=torch.uint8, device="cuda:0")
        d_out = buf.as_strided((3, oh, ow, 3), (slot, row, 3, 1))
        exp = SP.marker(3 * slot + TAIL)
        for k, img in enumerate(imgs):
            for j in range(oh):
                exp[k * slot + j * row:k * slot + j * row + ow * 3] = img[j].reshape(-1)
        return buf, lambda: ctx.decode_windows_resized_dev(files, d_out, WINS, mirror, format=fmt), exp
    st = TT.strides_of("nchw_rows", 3, 3, oh, ow)
    elems = sum((e - 1) * s for e, s in zip((3, 3, oh, ow), st)) + 1
    buf = torch.empty(elems * 4 + TAIL, dtype=torch.uint8, device="cuda:0")
    d_out = buf[:elems * 4].view(torch.float32).as_strided((3, 3, oh, ow), st)
    exp = SP.marker(elems * 4 + TAIL)
    for k, img in enumerate(imgs):
        TM.place(exp[:elems * 4].view(np.uint32), 0, st, k, img, TM.DT_F32, 3, TT.SCALE, TT.BIAS)
    return buf, lambda: ctx.decode_windows_tensor_dev(files, d_out, WINS, mirror, TT.SCALE, TT.BIAS, format=fmt), exp


@pytest.mark.parametrize("entry", ["decode_windows_dev", "decode_windows_resized_dev", "decode_windows_tensor_dev"])
def test_window_batch_entries_are_synchronous_and_refuse_a_capture(J, torch, delay, entry):
    """inside a capture of the context's stream the call raises, names the capture and leaves every byte of d_out alone; after the capture
    the same call on the same context gives the models' bytes; and with a delay pending on an unrelated stream the pixels are complete
    when the call returns -- read back by a copy on a third stream, with no device-wide synchronisation"""
    c = J.Context(0)
    try:
        buf, call, exp = _window_call(J, torch, c, entry)
        refill(torch, [buf])
        s = torch.cuda.ExternalStream(c.stream())
        g = torch.cuda.CUDAGraph()
        tick = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        refused = None
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                try:
                    call()
                except J.JpezyError as e:
                    refused = str(e)
                tick.add_(1)
        assert refused is not None and "status -1" in refused and "capture" in refused and entry in refused, refused
        torch.cuda.synchronize()
        assert untouched(torch, [buf]), "d_out was written by the refused call"
        res = call()
        assert [st for _, _, st in res] == [0, 0, 0]
        torch.cuda.synchronize()
        check(torch, [buf], [(exp, None)], "the same call after the capture")
        # complete on return
        refill(torch, [buf])
        host = torch.empty(buf.numel(), dtype=torch.uint8).pin_memory()
        busy, reader = torch.cuda.Stream(), torch.cuda.Stream()
        with torch.cuda.stream(busy):
            delay.queue(50.0)
        res = call()
        with torch.cuda.stream(reader):
            host.copy_(buf, non_blocking=True)
        reader.synchronize()
        got = host.numpy().copy()
        busy.synchronize()
        assert [st for _, _, st in res] == [0, 0, 0]
        bad = np.nonzero(got != exp)[0]
        assert bad.size == 0, ("pixels incomplete when the call returned", bad.size, "first", int(bad[0]))
    finally:
        torch.cuda.synchronize()
        c.close()
