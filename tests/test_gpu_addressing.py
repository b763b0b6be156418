"""Addresses of the batch entries where 32 bits end: every *_dev method of jpezy_amd.api.Context that takes a frame count, or frames from
a tensor's leading dimension, computes base + f * stride + y * row_stride + x.  The kernels keep 32-bit row offsets on purpose (W, H <=
65535; row_stride * H < 2^32 for the packed and YCbCr entries) and carry frame offsets in size_t.  A narrowed frame offset does not
crash: it reads or writes a valid address 2 or 4 GiB away.  Four procedures put the entries where that shows:

  P1  across the 65535-frame launch split: 65537 frames of 9 x 7 (an edge clamp, one MCU), built from three distinct frames with the frame
      index stamped in, planes and frames a padded stride apart; frames 0, 65534, 65535, 65536 and a seeded random dozen against the model
  P2  three frames FAR = 2^31 + 16 bytes apart (2^31 + 20 too where the entry picks its load or store form by alignment): frame 1 starts
      past 2 GiB, frame 2 past 4 GiB; 37 x 21 (partial MCUs on both edges); decoders: every byte of the gaps keeps the marker
  P3  row offsets up to the admitted 2^32 - 1: 16 x 65535 with a row stride of 65536 (YCbCr: 65536 and the largest admitted multiple of 16
      for the chroma planes), one megapixel addressed across 4 GiB; the first stride past the limit is JPEZY_E_BADARG.  (The limit is
      row_stride * H <= 2^32 - 1, and 65537 * 65535 is exactly that: 65537 is admitted -- the fused packed entries run it too -- and
      65538 is the first stride refused.)
  P4  (a) one frame of 65535 x 32784 = 2,148,499,440 pixels, whose 4:2:0 coefficients pass 2^32 bytes inside the frame: a tile of 48 rows
      repeated 683 times, every tile of the output against the model's result for the one tile; (b) a dense batch of 684 frames of
      2048 x 1024, five distinct ones repeated, whose coefficients pass 2^32 bytes at frame 683: every frame against its source's

The expected bytes are the numpy models' and the oracle's (quant_model, sampling_model, chroma_average_model, ycc_model, scaled_model,
region_model, smooth_model, region_smooth_model, transform_model, oracle.encode_coeffs, J.write_jpeg, J.huffman_histogram), never another
call of the entry under test.  Buffers are filled with a marker and compared on the device (tests/addressing_probe.py); only the place of
a first mismatch comes back, and a failure states it modulo 2^31 and 2^32.

COVERAGE names, for every such method and every variant it dispatches on, the test that holds it to each procedure;
tests/test_addressing_table.py needs no GPU and fails when a method has no row or a cell names a test that does not exist."""
import ctypes as C
import fnmatch
import functools
import inspect
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import addressing_probe as AP
import chroma_average_model as CM
import quant_model as QM
import region_model as R
import region_smooth_model as RS
import sampling_model as SM
import scaled_model as M
import smooth_model as SMOOTH
import test_gpu_region as TR
import transform_model as XM
import ycc_model as YM
from jpeg_synth import synth_jpeg

pytestmark = pytest.mark.gpu

N_SPLIT = AP.SPLIT + 2                                             # 65537: one full launch and two frames
FAR = AP.FAR
SMALL = (9, 7)                                                     # P1: one MCU with an edge clamp in both directions
RAGGED = (37, 21)                                                  # P2: partial MCUs on both edges
TALL = (16, 65535)                                                 # P3
SCALES = (1, 2, 4, 8)
NEED = 64 << 30


def align4(n):
    return (n + 3) & ~3


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def torch():
    """the module needs 64 GB of device memory: an MI355X must have them, anything smaller skips"""
    import torch
    props = torch.cuda.get_device_properties(0)
    if props.total_memory < NEED:
        assert "gfx950" not in getattr(props, "gcnArchName", ""), "an MI355X must hold the buffers of this module (up to 40 GB a test)"
        pytest.skip("needs 64 GB of device memory (not an MI355X)")
    return torch


@pytest.fixture
def ctx(J, torch):
    """a context of its own per test, closed behind it, and the allocator's cache given back"""
    c = J.Context(0)
    yield c
    torch.cuda.synchronize()
    c.close()
    torch.cuda.empty_cache()


# ---- inputs: made once, never modified ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layout_info(layout, W, H):
    """the FrameInfo of a layout of tests/test_gpu_region.py at W x H: the header of a small synthesised file, resized"""
    import jpezy_amd as J
    small, _ = J.read_jpeg(synth_jpeg(16, 16, TR.LAYOUTS[layout], seed=7)[0])
    info = J.FrameInfo()
    C.memmove(C.byref(info), C.byref(small), C.sizeof(J.FrameInfo))
    info.width, info.height = W, H
    info.mcu_cols, info.mcu_rows = -(-W // (8 * info.hmax)), -(-H // (8 * info.vmax))
    return info


def random_field(nmcu, bpm, seed, density=0.15):
    """sparse coefficients as jpeg_synth draws them: 15 % of the ACs in +-30, DCs in +-60; flat int16, read-only"""
    rng = np.random.default_rng(1000 + seed)
    co = np.zeros((nmcu, bpm, 64), np.int16)
    mask = rng.random(co.shape) < density
    co[mask] = rng.integers(-30, 31, int(mask.sum()), dtype=np.int16)
    co[..., 0] = rng.integers(-60, 61, (nmcu, bpm), dtype=np.int16)
    co = co.reshape(-1)
    co.setflags(write=False)
    return co


@functools.lru_cache(maxsize=None)
def fields_of(layout, W, H, K=3):
    info = layout_info(layout, W, H)
    return tuple(random_field(info.mcu_cols * info.mcu_rows, info.blocks_per_mcu, 10 * W + H + j) for j in range(K))


@functools.lru_cache(maxsize=None)
def rgb(W, H, j):
    from oracle import oracle as O
    out = tuple(np.asarray(p).reshape(H, W) for p in O.synth_rgb(W, H, frame=j))
    for p in out:
        p.setflags(write=False)
    return out


def pixel_bytes(fmt_name):
    return 3 if fmt_name.endswith("24") else 4


def red_at(fmt_name):
    return 0 if fmt_name.startswith("PIX_RGB") else 2


# ---- the encoders: (entry, variant) -> a form ------------------------------------------------------------------------------------------------
def coefficient_model(mode, W, H):
    """r, g, b (flat) -> the frame's coefficients under the mode: the oracle's for 4:2:0 and gray, the numpy models' for the others"""
    from oracle import oracle as O
    luma, chroma = QM.tables("q50")                                # Annex K
    return {"420": lambda r, g, b: O.encode_coeffs(r, g, b, W, H),
            "gray": lambda r, g, b: O.encode_coeffs(r, g, b, W, H, True),
            "444": lambda r, g, b: SM.encode_coeffs(r, g, b, W, H, luma, chroma),
            "average": lambda r, g, b: CM.encode_coeffs(r, g, b, W, H, luma, chroma)}[mode]


def _encoder(J, name, mode, W, H, surfaces, sources, stamp, model, call):
    sampling = J.SAMPLING_444 if mode == "444" else J.SAMPLING_420
    return SimpleNamespace(name=name, mode=mode, surfaces=surfaces, sources=sources, stamp=stamp, model=model, call=call,
                           cpf=J.coeff_count(W, H, mode == "gray", sampling), sampling=sampling, gray=mode == "gray")


def enc_planar(J, mode, W, H, frame_stride, K=3):
    """fdct_quant_dev: three planes, frames frame_stride apart"""
    cm = coefficient_model(mode, W, H)
    form = _encoder(J, f"fdct_quant_dev {mode} {W}x{H} plane_stride={frame_stride}", mode, W, H, [AP.Surface(H, W, W, frame_stride)] * 3,
                    [list(rgb(W, H, j)) for j in range(K)], [(0, 0), (0, 1), (0, 2)], lambda a: cm(*[p.reshape(-1) for p in a]), None)
    form.call = lambda ctx, bufs, n, d_co: ctx.fdct_quant_dev(*bufs, W, H, d_co, gray=form.gray, n_frames=n, plane_stride=form.surfaces[0].frame_stride,
                                                              sampling=form.sampling)
    return form


def enc_packed(J, mode, fmt_name, W, H, row_stride, frame_stride, K=3):
    """fdct_quant_packed_dev: the strides are the tensor's"""
    cm = coefficient_model(mode, W, H)
    fmt, nb, ri = getattr(J, fmt_name), pixel_bytes(fmt_name), red_at(fmt_name)
    s = AP.Surface(H, W * nb, row_stride, frame_stride)

    def model(a):
        img = a[0].reshape(H, W, nb)
        return cm(*[np.ascontiguousarray(img[..., c]).reshape(-1) for c in (ri, 1, 2 - ri)])
    form = _encoder(J, f"fdct_quant_packed_dev {mode} {fmt_name} {W}x{H} row_stride={s.row_stride} frame_stride={s.frame_stride}", mode, W, H, [s],
                    [[TR._interleave(J, fmt, rgb(W, H, j)).reshape(H, W * nb)] for j in range(K)], [(0, k * nb + ri) for k in range(3)], model, None)
    form.call = lambda ctx, bufs, n, d_co: ctx.fdct_quant_packed_dev(bufs[0].as_strided((n, H, W, nb), (s.frame_stride, s.row_stride, nb, 1)),
                                                                     d_co, format=fmt, gray=form.gray, sampling=form.sampling)
    return form


def enc_ycc(J, mode, W, H, y_stride, y_frame, c_stride, c_frame, K=3):
    """fdct_quant_ycc_dev: a luma and a chroma row and frame stride"""
    cw, ch = YM.chroma_size(W, H)
    sy, sc = AP.Surface(H, W, y_stride, y_frame), AP.Surface(ch, cw, c_stride, c_frame)
    form = _encoder(J, f"fdct_quant_ycc_dev {mode} {W}x{H} y strides {sy.row_stride}, {sy.frame_stride}, c strides {sc.row_stride}, {sc.frame_stride}",
                    mode, W, H, [sy, sc, sc], [list(YM.synth_planes(W, H, "random", j)) for j in range(K)], [(0, 0), (0, 1), (0, 2)],
                    lambda a: YM.encode_coeffs(a[0], a[1], a[2], mode == "gray"), None)

    def call(ctx, bufs, n, d_co):
        v = [b.as_strided((n, s.rows, s.row_bytes), (s.frame_stride, s.row_stride, 1)) for b, s in zip(bufs, form.surfaces)]
        ctx.fdct_quant_ycc_dev(v[0], v[1], v[2], d_co, gray=form.gray)
    form.call = call
    return form


COEFF_MARK = -23131                                                # 0xA5A5


def run_encoder(torch, ctx, form, n, frames):
    """n frames through the entry; the coefficients of `frames` against the model of the stamped source"""
    bufs = AP.place_frames(torch, form.surfaces, form.sources, n, form.stamp)
    d_co = torch.full((n * form.cpf + 8,), COEFF_MARK, dtype=torch.int16, device=AP.DEVICE)
    form.call(ctx, bufs, n, d_co[:n * form.cpf])
    torch.cuda.synchronize()
    assert bool((d_co[n * form.cpf:] == COEFF_MARK).all()), f"{form.name}: coefficients behind frame {n - 1} were written"
    K = len(form.sources)
    for f in frames:
        want = np.asarray(form.model(AP.stamped(form.sources[f % K], f, form.stamp)), np.int16).reshape(-1)
        assert want.size == form.cpf
        bad = (d_co[f * form.cpf:(f + 1) * form.cpf] != torch.from_numpy(want).to(AP.DEVICE)).nonzero()
        if bad.numel():
            k = int(bad[0, 0])
            raise AssertionError(f"{form.name}: frame {f}: coefficient {k} is {int(d_co[f * form.cpf + k])}, the model's {int(want[k])}; first "
                                 f"difference at {AP.where(2 * (f * form.cpf + k))} of d_coeffs; the frame's pixels start at "
                                 f"{AP.where(f * form.surfaces[0].frame_stride)}")
    del bufs, d_co


# ---- the decoders --------------------------------------------------------------------------------------------------------------------------
def whole_region(W, H, scale):
    ws, hs = M.scaled_size(W, H, scale)
    return (0, 0, ws, hs)


def inner_region(W, H, scale):
    """a window that starts and ends inside MCUs and covers block 0, where the frame's stamp is"""
    ws, hs = M.scaled_size(W, H, scale)
    x, y = (1, 1) if ws > 2 and hs > 2 else (0, 0)
    return (x, y, max(1, ws - x - (1 if ws > 3 else 0)), max(1, hs - y - (1 if hs > 3 else 0)))


def decoder(J, entry, layout, W, H, fmt_name=None, scale=1, smooth=False, region=None, fields=None, K=3):
    """a decoding entry in one variant -> a form: fields, the shape of every output per frame, model(field) -> those outputs,
    call(ctx, d_co, n, bufs, surfaces)"""
    info = layout_info(layout, W, H)
    ws, hs = M.scaled_size(W, H, scale)
    w, h = (region[2], region[3]) if region is not None else (ws, hs)
    tq = tuple(info.Tq[i] for i in range(3))
    up = J.UPSAMPLE_SMOOTH if smooth else J.UPSAMPLE_NEAREST
    if entry == "dequant_idct_ycc_dev":
        sizes = [YM.component_size(info, c) for c in range(3)]
        shapes = [(ch, cw) for cw, ch in sizes]
        planes = lambda co: YM.decode_planes(co, info)
    else:
        shapes = [(h, w)] * 3
        if entry == "dequant_idct_region_dev":
            planes = (lambda co: RS.decode_window(co, info, scale, region)) if smooth else (lambda co: R.decode_region(co, info, region, scale))
        elif entry == "dequant_idct_upsampling_dev":
            planes = lambda co: SMOOTH.decode_planes(co, info)
        else:
            planes = lambda co: M.decode_planes(co, info, scale)
    model = lambda co: [np.asarray(p).reshape(s) for p, s in zip(planes(co), shapes)]
    if fmt_name is not None:
        fmt, nb = getattr(J, fmt_name), pixel_bytes(fmt_name)
        shapes = [(h, w * nb)]
        model = lambda co: [TR._interleave(J, fmt, [np.asarray(p).reshape(h, w) for p in planes(co)]).reshape(h, w * nb)]

    def call(ctx, d_co, n, bufs, surfaces):
        s = surfaces[0]
        if fmt_name is not None:
            d_img = bufs[0].as_strided((n, h, w, nb), (s.frame_stride, s.row_stride, nb, 1))
            if entry == "dequant_idct_packed_dev":
                return ctx.dequant_idct_packed_dev(d_co, d_img, format=fmt, qt=info.qt, comp_tq=tq)
            if entry == "dequant_idct_scaled_dev":
                return ctx.dequant_idct_scaled_dev(d_co, info, scale, d_img=d_img, format=fmt)
            if entry == "dequant_idct_upsampling_dev":
                return ctx.dequant_idct_upsampling_dev(d_co, info, d_img=d_img, format=fmt)
            assert entry == "dequant_idct_region_dev", entry
            return ctx.dequant_idct_region_dev(d_co, info, region, scale, d_img=d_img, format=fmt, upsampling=up)
        if entry == "dequant_idct_ycc_dev":
            v = [b.as_strided((n, x.rows, x.row_bytes), (x.frame_stride, x.row_stride, 1)) for b, x in zip(bufs, surfaces)]
            return ctx.dequant_idct_ycc_dev(d_co, v[0], v[1], v[2], qt=info.qt, comp_tq=tq)
        assert all(x.row_stride == x.row_bytes for x in surfaces), "planes have no row stride"
        kw = dict(n_frames=n, plane_stride=s.frame_stride)
        if entry == "dequant_idct_dev":
            return ctx.dequant_idct_dev(d_co, W, H, *bufs, qt=info.qt, comp_tq=tq, **kw)
        if entry == "dequant_idct_generic_dev":
            return ctx.dequant_idct_generic_dev(d_co, info, *bufs, **kw)
        if entry == "dequant_idct_scaled_dev":
            return ctx.dequant_idct_scaled_dev(d_co, info, scale, *bufs, **kw)
        if entry == "dequant_idct_upsampling_dev":
            return ctx.dequant_idct_upsampling_dev(d_co, info, *bufs, **kw)
        assert entry == "dequant_idct_region_dev", entry
        return ctx.dequant_idct_region_dev(d_co, info, region, scale, *bufs, upsampling=up, **kw)
    name = f"{entry} {layout} {W}x{H}" + (f" {fmt_name}" if fmt_name else " planes") + f" 1/{scale}" + (" smooth" if smooth else "") + \
        (f" region {region}" if region is not None else "")
    return SimpleNamespace(name=name, fields=fields_of(layout, W, H, K) if fields is None else fields, shapes=shapes, model=model, call=call)


def run_decoder(torch, ctx, form, n, strides, frames, gaps):
    """n frames through the entry into marker-filled buffers; strides: (row_stride or None, frame_stride) per output.  The frames in
    `frames` against the model of the stamped field, their row padding and the bytes behind the frames in `gaps` against the marker"""
    surfaces = [AP.Surface(r, rb, rs, fs) for (r, rb), (rs, fs) in zip(form.shapes, strides)]
    d_co = AP.place_fields(torch, form.fields, n)
    bufs = [AP.alloc(torch, s, n) for s in surfaces]
    who = form.name + " strides " + ", ".join(f"{s.row_stride}/{s.frame_stride}" for s in surfaces)
    form.call(ctx, d_co, n, bufs, surfaces)
    torch.cuda.synchronize()
    K = len(form.fields)
    for f in frames:
        AP.check_frame(torch, who, surfaces, bufs, f, form.model(AP.stamp_field(form.fields[f % K], f)))
    AP.check_gaps(who, surfaces, bufs, n, gaps)
    del bufs, d_co


def refused(J, torch, call, surfaces, n=1):
    """the call on buffers laid out with strides past the limit: JPEZY_E_BADARG, before anything is looked at"""
    bufs = [torch.empty(s.size(n), dtype=torch.uint8, device=AP.DEVICE) for s in surfaces]
    with pytest.raises(J.JpezyError, match="status -1"):
        call(bufs, surfaces)
    del bufs


# ==== P1: across the 65535-frame launch split ====================================================================================================
def p1_encoders(J):
    W, H = SMALL
    out = {}
    for mode in ("444", "average"):
        out[f"fdct_quant-{mode}"] = lambda mode=mode: enc_planar(J, mode, W, H, W * H + 4)
    for mode in ("420", "average", "444"):
        out[f"fdct_quant_packed-rgb24-tight-{mode}"] = lambda mode=mode: enc_packed(J, mode, "PIX_RGB24", W, H, None, None)
        out[f"fdct_quant_packed-bgra32-padded-{mode}"] = lambda mode=mode: enc_packed(J, mode, "PIX_BGRA32", W, H, W * 4 + 4, H * (W * 4 + 4) + 8)
    cw, ch = YM.chroma_size(W, H)
    for mode in ("420", "gray"):                                   # (tests/test_gpu_ycc.py crosses the split with tight 1 x 1 frames)
        out[f"fdct_quant_ycc-{mode}"] = lambda mode=mode: enc_ycc(J, mode, W, H, W + 3, H * (W + 3) + 5, cw + 2, ch * (cw + 2) + 7)
    return out


P1_ENCODERS = sorted(p1_encoders(None))


@pytest.mark.parametrize("case", P1_ENCODERS)
def test_encoders_across_the_launch_split(J, torch, ctx, case):
    form = p1_encoders(J)[case]()
    if form.mode == "average":
        ctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
    run_encoder(torch, ctx, form, N_SPLIT, AP.sample(N_SPLIT))


def p1_decoders(J):
    """{case: (form builder, strides)}: planes a padded multiple of 4 apart, packed rows padded and frames a padded multiple of 4 apart"""
    W, H = SMALL
    plane = [(None, align4(W * H) + 4)] * 3

    def packed(w, h, nb):
        return [(w * nb + 5, align4(h * (w * nb + 5)) + 8)]
    out = {"dequant_idct_packed": (lambda: decoder(J, "dequant_idct_packed_dev", "own", W, H, "PIX_BGR24"), packed(W, H, 3))}
    for layout in ("own", "422"):
        out[f"upsampling-planes-{layout}"] = (lambda layout=layout: decoder(J, "dequant_idct_upsampling_dev", layout, W, H, smooth=True), plane)
        out[f"upsampling-packed-{layout}"] = (lambda layout=layout: decoder(J, "dequant_idct_upsampling_dev", layout, W, H, "PIX_RGBA32", smooth=True),
                                              packed(W, H, 4))
    cw, ch = YM.chroma_size(W, H)
    out["dequant_idct_ycc"] = (lambda: decoder(J, "dequant_idct_ycc_dev", "own", W, H),
                               [(W + 3, H * (W + 3) + 5)] + [(cw + 2, ch * (cw + 2) + 7)] * 2)
    for scale in SCALES:
        ws, hs = M.scaled_size(W, H, scale)
        out[f"scaled{scale}-planes"] = (lambda scale=scale: decoder(J, "dequant_idct_scaled_dev", "422", W, H, scale=scale),
                                        [(None, align4(ws * hs) + 4)] * 3)
        out[f"scaled{scale}-packed"] = (lambda scale=scale: decoder(J, "dequant_idct_scaled_dev", "422", W, H, "PIX_RGB24", scale=scale),
                                        packed(ws, hs, 3))
        rg = inner_region(W, H, scale)
        for smooth in (False, True):
            kind = "smooth" if smooth else "nearest"
            out[f"region{scale}-planes-{kind}"] = (
                lambda scale=scale, smooth=smooth, rg=rg: decoder(J, "dequant_idct_region_dev", "own", W, H, scale=scale, smooth=smooth, region=rg),
                [(None, align4(rg[2] * rg[3]) + 4)] * 3)
            out[f"region{scale}-packed-{kind}"] = (
                lambda scale=scale, smooth=smooth, rg=rg: decoder(J, "dequant_idct_region_dev", "own", W, H, "PIX_BGRA32", scale=scale,
                                                                  smooth=smooth, region=rg), packed(rg[2], rg[3], 4))
    return out


P1_DECODERS = sorted(p1_decoders(None))


@pytest.mark.parametrize("case", P1_DECODERS)
def test_decoders_across_the_launch_split(J, torch, ctx, case):
    build, strides = p1_decoders(J)[case]
    frames = AP.sample(N_SPLIT)
    run_decoder(torch, ctx, build(), N_SPLIT, strides, frames, frames)


XFORM_SIZE = {"420": (32, 16), "444": (16, 8)}                     # 2 x 1 MCUs: a swap of the axes changes the grid


def own_fields(J, sampling_name, W, H, K=3):
    """K coefficient fields of the encoder's own layouts (6-block MCUs of 16 x 16, 3-block MCUs of 8 x 8)"""
    mc, mr, bpm = J.sampling_geometry(getattr(J, "SAMPLING_" + sampling_name), W, H)
    return [random_field(mc * mr, bpm, 77 * W + H + j) for j in range(K)]


def compare_rows(torch, who, got, f, want, bytes_per_row):
    """row f of a device tensor [n, k] against the model's; the first difference as a byte offset of the whole output"""
    want = torch.from_numpy(np.ascontiguousarray(want).reshape(-1)).to(got.device)
    assert want.dtype == got.dtype and want.numel() == got.shape[1], (who, want.dtype, got.dtype, want.numel(), got.shape)
    bad = (got[f] != want).nonzero()
    if bad.numel():
        k = int(bad[0, 0])
        raise AssertionError(f"{who}: frame {f}: element {k} is {int(got[f, k])}, the model's {int(want[k])}; first difference at "
                             f"{AP.where(f * bytes_per_row + k * got.element_size())}")


@pytest.mark.parametrize("sampling", ["420", "444"])
@pytest.mark.parametrize("op", ["ROT90", "HFLIP"])
def test_transform_across_the_launch_split(J, torch, ctx, op, sampling):
    W, H = XFORM_SIZE[sampling]
    smp, xop, n = getattr(J, "SAMPLING_" + sampling), getattr(J, "XFORM_" + op), N_SPLIT
    fields = own_fields(J, sampling, W, H)
    wo, ho, _, _ = J.transform_geometry(xop, W, H, smp)
    assert (wo, ho) == ((H, W) if op == "ROT90" else (W, H))
    cpf = J.coeff_count(wo, ho, sampling=smp)
    d_in = AP.place_fields(torch, fields, n)
    d_out = torch.full((n * cpf + 8,), COEFF_MARK, dtype=torch.int16, device=AP.DEVICE)
    ctx.coeff_transform_dev(d_in, W, H, d_out[:n * cpf], xop, sampling=smp, n_frames=n)
    torch.cuda.synchronize()
    assert bool((d_out[n * cpf:] == COEFF_MARK).all()), "coefficients behind the last frame were written"
    bpm = 6 if sampling == "420" else 3
    for f in AP.sample(n):
        src = AP.stamp_field(fields[f % 3], f).reshape(-1, bpm, 64)
        want, w2, h2 = XM.transform_field(src, W, H, XM.S420 if sampling == "420" else XM.S444, xop)
        assert (w2, h2) == (wo, ho)
        compare_rows(torch, f"coeff_transform_dev {op} {sampling} {W}x{H}", d_out[:n * cpf].view(n, cpf), f, want.astype(np.int16), 2 * cpf)


@pytest.mark.parametrize("sampling,interval", [("420", 1), ("444", 4)])
def test_histogram_across_the_launch_split(J, torch, ctx, sampling, interval):
    """24 x 16: two MCUs of 4:2:0 with the predictors reset at each, six of 4:4:4 in intervals of four and two"""
    W, H, n = 24, 16, N_SPLIT
    smp = getattr(J, "SAMPLING_" + sampling)
    fields = own_fields(J, sampling, W, H)
    ctx.set_restart_interval(interval)
    d_co = AP.place_fields(torch, fields, n)
    d_hist = torch.full((n * 1024 + 4,), -1, dtype=torch.int64, device=AP.DEVICE)
    ctx.huffman_histogram_dev(d_co, W, H, d_hist[:n * 1024].view(n, 4, 256), n_frames=n, sampling=smp)
    torch.cuda.synchronize()
    assert bool((d_hist[n * 1024:] == -1).all()), "counts behind the last frame were written"
    plain = J.huffman_histogram(AP.stamp_field(fields[0], 0), W, H, smp, 0)
    assert not np.array_equal(plain, J.huffman_histogram(AP.stamp_field(fields[0], 0), W, H, smp, interval)), "the interval changes nothing"
    for f in AP.sample(n):
        want = J.huffman_histogram(AP.stamp_field(fields[f % 3], f), W, H, smp, interval).astype(np.int64)
        compare_rows(torch, f"huffman_histogram_dev {sampling} {W}x{H} restart interval {interval}", d_hist[:n * 1024].view(n, 1024), f, want, 8192)


def check_files(torch, J, who, d_out, d_sizes, stride, frames, want_file):
    """frame f's file at d_out + f * stride and its length against want_file(f)"""
    sizes = d_sizes.cpu().numpy()
    for f in frames:
        want = np.frombuffer(want_file(f), np.uint8)
        assert int(sizes[f]) == want.size, f"{who}: frame {f}: size {int(sizes[f])}, the host writer's {want.size}; slot at {AP.where(f * stride)}"
        got = d_out[f * stride:f * stride + want.size]
        bad = (got != torch.from_numpy(want.copy()).to(got.device)).nonzero()
        if bad.numel():
            k = int(bad[0, 0])
            raise AssertionError(f"{who}: frame {f}: byte {k} of the file is {int(got[k])}, the host writer's {int(want[k])}; first difference at "
                                 f"{AP.where(f * stride + k)}")


def test_writer_444_across_the_launch_split(J, torch, ctx):
    W, H = SMALL
    n, smp = N_SPLIT, J.SAMPLING_444
    fields = own_fields(J, "444", W, H)
    stride = J.jpeg_bound(W, H, smp)
    d_co = AP.place_fields(torch, fields, n)
    d_out = torch.empty(n * stride + AP.TAIL, dtype=torch.uint8, device=AP.DEVICE)
    AP.fill(d_out)
    d_sizes = torch.full((n + 2,), -77, dtype=torch.int64, device=AP.DEVICE)
    ctx.write_jpeg_gpu_dev(d_co, W, H, d_out[:n * stride], d_sizes[:n], n_frames=n, sampling=smp)
    torch.cuda.synchronize()
    assert bool((d_sizes[n:] == -77).all()) and AP.first_other(d_out, n * stride, d_out.numel()) is None, "written behind the last frame"
    check_files(torch, J, f"write_jpeg_gpu_dev 444 {W}x{H}", d_out, d_sizes, stride, AP.sample(n),
                lambda f: J.write_jpeg(AP.stamp_field(fields[f % 3], f), W, H, sampling=smp))


# ==== P2: frames more than 4 GiB apart ============================================================================================================
def p2_encoders(J):
    W, H = RAGGED
    out = {}
    for mode in ("420", "gray", "average"):
        out[f"fdct_quant-{mode}-{FAR}"] = lambda mode=mode: enc_planar(J, mode, W, H, FAR)
    for stride in (FAR, FAR + 4):                                  # 4:4:4, packed and YCbCr pick their load form by alignment
        out[f"fdct_quant-444-{stride}"] = lambda s=stride: enc_planar(J, "444", W, H, s)
        for mode in ("420", "444", "average"):
            out[f"fdct_quant_packed-{mode}-{stride}"] = lambda s=stride, mode=mode: enc_packed(J, mode, "PIX_BGRA32", W, H, W * 4 + 12, s)
        for mode in ("420", "gray"):
            out[f"fdct_quant_ycc-{mode}-{stride}"] = lambda s=stride, mode=mode: enc_ycc(J, mode, W, H, W + 3, s, (W + 1) // 2 + 5, s + 8)
    return out


P2_ENCODERS = sorted(p2_encoders(None))


@pytest.mark.parametrize("case", P2_ENCODERS)
def test_encoders_with_frames_4_gib_apart(J, torch, ctx, case):
    form = p2_encoders(J)[case]()
    if form.mode == "average":
        ctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
    run_encoder(torch, ctx, form, 3, [0, 1, 2])


def p2_decoders(J):
    """{case: (form builder, strides)}"""
    W, H = RAGGED
    out = {}

    def add(case, build, packed_bytes=0, size=(W, H)):
        for stride in ((FAR, FAR + 4) if packed_bytes else (FAR,)):            # the packed store form goes by alignment
            strides = [(size[0] * packed_bytes + 5, stride)] if packed_bytes else [(None, stride)] * 3
            out[f"{case}-{stride}"] = (build, strides)
    add("dequant_idct-planes", lambda: decoder(J, "dequant_idct_dev", "own", W, H))
    add("dequant_idct_packed", lambda: decoder(J, "dequant_idct_packed_dev", "own", W, H, "PIX_BGR24"), 3)
    for stride in (FAR, FAR + 4):
        out[f"dequant_idct_ycc-{stride}"] = (lambda: decoder(J, "dequant_idct_ycc_dev", "own", W, H),
                                             [(W + 3, stride), ((W + 1) // 2 + 5, stride + 8), ((W + 1) // 2 + 5, stride + 8)])
    for layout in ("own", "422"):
        add(f"generic-planes-{layout}", lambda layout=layout: decoder(J, "dequant_idct_generic_dev", layout, W, H))
        add(f"upsampling-planes-{layout}", lambda layout=layout: decoder(J, "dequant_idct_upsampling_dev", layout, W, H, smooth=True))
        add(f"upsampling-packed-{layout}", lambda layout=layout: decoder(J, "dequant_idct_upsampling_dev", layout, W, H, "PIX_RGB24", smooth=True), 3)
    for scale in SCALES:
        size = M.scaled_size(W, H, scale)
        add(f"scaled{scale}-planes", lambda scale=scale: decoder(J, "dequant_idct_scaled_dev", "422", W, H, scale=scale))
        add(f"scaled{scale}-packed", lambda scale=scale: decoder(J, "dequant_idct_scaled_dev", "422", W, H, "PIX_RGBA32", scale=scale), 4, size)
        rg = inner_region(W, H, scale)
        for smooth in (False, True):
            kind = "smooth" if smooth else "nearest"
            add(f"region{scale}-planes-{kind}",
                lambda scale=scale, smooth=smooth, rg=rg: decoder(J, "dequant_idct_region_dev", "own", W, H, scale=scale, smooth=smooth, region=rg))
            add(f"region{scale}-packed-{kind}",
                lambda scale=scale, smooth=smooth, rg=rg: decoder(J, "dequant_idct_region_dev", "own", W, H, "PIX_BGRA32", scale=scale, smooth=smooth,
                                                                  region=rg), 4, rg[2:])
    return out


P2_DECODERS = sorted(p2_decoders(None))


@pytest.mark.parametrize("case", P2_DECODERS)
def test_decoders_with_frames_4_gib_apart(J, torch, ctx, case):
    build, strides = p2_decoders(J)[case]
    run_decoder(torch, ctx, build(), 3, strides, [0, 1, 2], [0, 1, 2])


@pytest.mark.parametrize("sampling", ["420", "444"])
def test_writer_with_slots_4_gib_apart(J, torch, ctx, sampling):
    """d_out of shape [3, FAR]: the files and their sizes; the bytes behind the third slot keep the marker"""
    W, H = RAGGED
    smp, n = getattr(J, "SAMPLING_" + sampling), 3
    fields = own_fields(J, sampling, W, H)
    d_co = AP.place_fields(torch, fields, n)
    d_out = torch.empty(n * FAR + AP.TAIL, dtype=torch.uint8, device=AP.DEVICE)
    AP.fill(d_out)
    d_sizes = torch.full((n + 2,), -77, dtype=torch.int64, device=AP.DEVICE)
    ctx.write_jpeg_gpu_dev(d_co, W, H, d_out[:n * FAR].view(n, FAR), d_sizes[:n], n_frames=n, sampling=smp)
    torch.cuda.synchronize()
    assert bool((d_sizes[n:] == -77).all()) and AP.first_other(d_out, n * FAR, d_out.numel()) is None, "written behind the last slot"
    check_files(torch, J, f"write_jpeg_gpu_dev {sampling} {W}x{H} out_stride={FAR}", d_out, d_sizes, FAR, range(n),
                lambda f: J.write_jpeg(AP.stamp_field(fields[f % 3], f), W, H, sampling=smp))


# ==== P3: row offsets up to the admitted 2^32 - 1 ==================================================================================================
ROW = 65536                                                        # x H = 65535: 4,294,901,760
LIMIT = 0xFFFFFFFF


def first_refused(rows):
    """the first row stride whose product with the row count does not fit in 32 bits"""
    return LIMIT // rows + 1


def test_row_limits_are_what_the_cases_assume():
    """(no GPU work) 65536 * 65535 is admitted, and so is 65537 * 65535 = 2^32 - 1: the first refused stride of 65535 rows is 65538"""
    W, H = TALL
    assert ROW * H == 4294901760 <= LIMIT and 65537 * H == LIMIT and first_refused(H) == 65538
    assert chroma_row(H) == 131056 and chroma_row(H) * ((H + 1) // 2) <= LIMIT and first_refused((H + 1) // 2) == 131072


def chroma_row(H):
    """the largest admitted multiple of 16 as the row stride of (H + 1) // 2 rows"""
    return LIMIT // ((H + 1) // 2) // 16 * 16


@pytest.mark.parametrize("mode", ["420", "444", "average", "420-at-the-limit"])
def test_packed_encoder_with_rows_across_4_gib(J, torch, ctx, mode):
    """(at the limit: a row stride of 65537, whose product with H is 2^32 - 1; rows at every alignment)"""
    W, H = TALL
    mode, row = (mode, ROW) if mode != "420-at-the-limit" else ("420", first_refused(H) - 1)
    form = enc_packed(J, mode, "PIX_RGBA32", W, H, row, None, K=1)
    if mode == "average":
        ctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
    run_encoder(torch, ctx, form, 1, [0])
    d_co = torch.empty(form.cpf, dtype=torch.int16, device=AP.DEVICE)
    bad = enc_packed(J, mode, "PIX_RGBA32", W, H, first_refused(H), None, K=1)
    refused(J, torch, lambda bufs, s: bad.call(ctx, bufs, 1, d_co), bad.surfaces)


@pytest.mark.parametrize("mode", ["420", "gray"])
def test_ycc_encoder_with_rows_across_4_gib(J, torch, ctx, mode):
    W, H = TALL
    ch = (H + 1) // 2
    form = enc_ycc(J, mode, W, H, ROW, None, chroma_row(H), None, K=1)
    run_encoder(torch, ctx, form, 1, [0])
    d_co = torch.empty(form.cpf, dtype=torch.int16, device=AP.DEVICE)
    for ys, cs in ((first_refused(H), chroma_row(H)),) + (((ROW, first_refused(ch)),) if mode == "420" else ()):
        bad = enc_ycc(J, mode, W, H, ys, None, cs, None, K=1)
        refused(J, torch, lambda bufs, s: bad.call(ctx, bufs, 1, d_co), bad.surfaces)


def p3_decoders(J):
    """{case: (form builder, strides, strides past the limit)}: RGBA32 rows of 64 (32 at 1/2) bytes, ROW apart"""
    W, H = TALL
    one = lambda rows, row=None: ([(row or LIMIT // rows // 16 * 16, None)], [(first_refused(rows), None)])
    out = {
        "dequant_idct_packed": (lambda: decoder(J, "dequant_idct_packed_dev", "own", W, H, "PIX_RGBA32"), *one(H, ROW)),
        "dequant_idct_packed-at-the-limit": (lambda: decoder(J, "dequant_idct_packed_dev", "own", W, H, "PIX_RGBA32"), *one(H, first_refused(H) - 1)),
        "upsampling-packed": (lambda: decoder(J, "dequant_idct_upsampling_dev", "own", W, H, "PIX_RGBA32", smooth=True), *one(H, ROW)),
        "dequant_idct_ycc": (lambda: decoder(J, "dequant_idct_ycc_dev", "own", W, H), [(ROW, None)] + [(chroma_row(H), None)] * 2,
                             [(first_refused(H), None)] + [(chroma_row(H), None)] * 2),
    }
    for scale in SCALES:
        hs = M.scaled_size(W, H, scale)[1]
        row = ROW if scale == 1 else None
        whole = whole_region(W, H, scale)
        out[f"scaled{scale}-packed"] = (lambda scale=scale: decoder(J, "dequant_idct_scaled_dev", "own", W, H, "PIX_RGBA32", scale=scale), *one(hs, row))
        for smooth in (False, True):
            out[f"region{scale}-packed-{'smooth' if smooth else 'nearest'}"] = (
                lambda scale=scale, smooth=smooth, whole=whole: decoder(J, "dequant_idct_region_dev", "own", W, H, "PIX_RGBA32", scale=scale,
                                                                        smooth=smooth, region=whole), *one(hs, row))
    return out

P3_DECODERS = sorted(p3_decoders(None))


@pytest.mark.parametrize("case", P3_DECODERS)
def test_decoders_with_rows_across_4_gib(J, torch, ctx, case):
    """the frame against the model, the row padding and the bytes behind the last row against the marker, all on the device; then the
    first stride past the limit: JPEZY_E_BADARG"""
    build, strides, past = p3_decoders(J)[case]
    form = build()
    run_decoder(torch, ctx, form, 1, strides, [0], [0])
    torch.cuda.empty_cache()
    d_co = AP.place_fields(torch, form.fields, 1)
    surfaces = [AP.Surface(r, rb, rs, fs) for (r, rb), (rs, fs) in zip(form.shapes, past)]
    refused(J, torch, lambda bufs, s: form.call(ctx, d_co, 1, bufs, s), surfaces)


# ==== P4: one frame of more than 2^31 pixels, and dense offsets past 2^32 bytes ====================================================================
def expect_equal(who, unit, got, want, rows=None):
    """AP.first_mismatch as an assertion: names the unit (tile, frame, MCU row) of the first difference and its byte offset"""
    bad = AP.first_mismatch(got, want, rows)
    if bad is not None:
        idx, off, g, w = bad
        raise AssertionError(f"{who}: {unit} {idx[0]}, element {idx[1:]}: got {g}, the model's {w}; first difference at {AP.where(off)}")


def marked(torch, elems, dtype):
    """elems elements and AP.TAIL bytes of tail, every byte the marker"""
    size = torch.empty(0, dtype=dtype).element_size()
    buf = torch.empty(elems + AP.TAIL // size, dtype=dtype, device=AP.DEVICE)
    AP.fill(buf.view(torch.uint8))
    return buf


def tail_kept(torch, who, buf, elems):
    bad = AP.first_other(buf.view(torch.uint8), elems * buf.element_size(), buf.numel() * buf.element_size())
    assert bad is None, f"{who}: the byte at {AP.where(bad)}, behind the output, was written"


# ---- (a) one huge frame: a tile of 48 rows repeated 683 times down the frame ---------------------------------------------------------------------
BIG = (65535, 32784)                                               # 2,148,499,440 pixels; 6.4 GB of 4:2:0 coefficients
TILE_ROWS, TILES = 48, 683


def phase_shows(nbytes):
    """a tile of this many bytes does not divide 2^31 or 2^32: an offset wrapped there lands at another phase of the tiling"""
    return (1 << 31) % nbytes != 0 and (1 << 32) % nbytes != 0


def test_the_huge_frame_is_what_the_cases_assume():
    """(no GPU work)"""
    W, H = BIG
    assert TILE_ROWS * TILES == H and W * H == 2148499440 > 1 << 31 and W * TILE_ROWS == 3145680 and phase_shows(W * TILE_ROWS)
    assert (H // 16) * 4096 * 384 * 2 > 1 << 32


@pytest.mark.parametrize("mode", ["420", "gray", "444", "average"])
def test_encoder_on_one_frame_of_2_gigapixels(J, torch, ctx, mode):
    """every group of three MCU rows (six of 4:4:4) is the model's coefficients of the one tile"""
    W, H = BIG
    tile = rgb(W, TILE_ROWS, 0)
    want = np.asarray(coefficient_model(mode, W, TILE_ROWS)(*[p.reshape(-1) for p in tile]), np.int16).reshape(1, -1)
    sampling = J.SAMPLING_444 if mode == "444" else J.SAMPLING_420
    cpf = J.coeff_count(W, H, mode == "gray", sampling)
    assert cpf == TILES * want.size and phase_shows(2 * want.size)
    if mode == "average":
        ctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
    planes = [torch.from_numpy(np.array(p).reshape(-1)).to(AP.DEVICE).repeat(TILES) for p in tile]
    d_co = marked(torch, cpf, torch.int16)
    ctx.fdct_quant_dev(*planes, W, H, d_co[:cpf], gray=mode == "gray", sampling=sampling)
    torch.cuda.synchronize()
    who = f"fdct_quant_dev {mode} {W}x{H}"
    expect_equal(who, "tile", d_co[:cpf].view(TILES, -1), torch.from_numpy(want).to(AP.DEVICE))
    tail_kept(torch, who, d_co, cpf)


BIG_DECODERS = {"dequant_idct": ("dequant_idct_dev", "own", 1, False), "generic-422": ("dequant_idct_generic_dev", "422", 1, False),
                "scaled2": ("dequant_idct_scaled_dev", "own", 2, False), "upsampling": ("dequant_idct_upsampling_dev", "own", 1, True)}


@pytest.mark.parametrize("case", sorted(BIG_DECODERS))
def test_decoder_on_one_frame_of_2_gigapixels(J, torch, ctx, case):
    """the coefficients of one tile repeated: every tile of the output is the model's tile.  The smooth filter sees the neighbouring tile
    across a seam: interior tiles are the middle tile of the model run on three stacked tiles, the first and the last tile that model's"""
    entry, layout, scale, smooth = BIG_DECODERS[case]
    W, H = BIG
    stack = 3 if smooth else 1
    tinfo = layout_info(layout, W, TILE_ROWS)
    field = random_field(tinfo.mcu_cols * tinfo.mcu_rows, tinfo.blocks_per_mcu, 4242)
    big = decoder(J, entry, layout, W, H, scale=scale, smooth=smooth, fields=())
    model = decoder(J, entry, layout, W, stack * TILE_ROWS, scale=scale, smooth=smooth, fields=())
    ws, hs = M.scaled_size(W, H, scale)
    rows = hs // TILES
    assert rows * TILES == hs and phase_shows(rows * ws)
    want = [np.asarray(p).reshape(stack, rows * ws) for p in model.model(np.tile(field, stack))]
    d_co = torch.from_numpy(np.array(field)).to(AP.DEVICE).repeat(TILES)
    surfaces = [AP.Surface(hs, ws)] * 3
    bufs = [AP.alloc(torch, s, 1) for s in surfaces]
    big.call(ctx, d_co, 1, bufs, surfaces)
    torch.cuda.synchronize()
    which = torch.ones(TILES, dtype=torch.long, device=AP.DEVICE)
    which[0], which[-1] = 0, 2
    for k in range(3):
        got = bufs[k][:hs * ws].view(TILES, rows * ws)
        w = torch.from_numpy(want[k]).to(AP.DEVICE)
        expect_equal(f"{big.name}, output {k}", "tile", got, w, which if smooth else None)
    AP.check_gaps(big.name, surfaces, bufs, 1, [0])


@pytest.mark.parametrize("op", ["ROT90", "ROT180"])
def test_transform_on_one_frame_of_2_gigapixels(J, torch, ctx, op):
    """ROT90 mirrors the height, which is whole MCUs; ROT180 mirrors the width too, whose last MCU is partial: with trim, the only form the
    entry takes at this size.  The field is a tile of three MCU rows repeated; 2049 = 3 * 683, so source row 2048 - c is tile row 2 - c % 3:
    ROT90's output is, in every MCU row, the tile's three output columns repeated, ROT180's the tile's output repeated down the frame"""
    W, H = BIG
    xop, trim = getattr(J, "XFORM_" + op), op == "ROT180"
    cols = -(-W // 16)
    tile = random_field(cols * 3, 6, 909).reshape(-1, 6, 64)
    want, tw, th = XM.transform_field(tile, W, TILE_ROWS, XM.S420, xop, trim)
    wo, ho, _, _ = J.transform_geometry(xop, W, H, J.SAMPLING_420, trim)
    assert (wo, ho) == ((H, W) if op == "ROT90" else (W // 16 * 16, H)) and (tw, th) == ((TILE_ROWS, W) if op == "ROT90" else (wo, TILE_ROWS))
    cpf = J.coeff_count(wo, ho)
    assert cpf == TILES * want.size and phase_shows(2 * want.size)
    d_in = torch.from_numpy(np.array(tile).reshape(-1)).to(AP.DEVICE).repeat(TILES)
    d_out = marked(torch, cpf, torch.int16)
    ctx.coeff_transform_dev(d_in, W, H, d_out[:cpf], xop, trim=trim, n_frames=1)
    torch.cuda.synchronize()
    who = f"coeff_transform_dev {op} {W}x{H}"
    w = torch.from_numpy(np.ascontiguousarray(want, np.int16)).to(AP.DEVICE)
    if op == "ROT90":                                              # [4096 MCU rows][2049 = 683 * 3 MCU columns][384]
        expect_equal(who, "MCU row", d_out[:cpf].view(cols, TILES, 3 * 384), w.view(cols, 1, 3 * 384))
    else:
        expect_equal(who, "tile", d_out[:cpf].view(TILES, -1), w.view(1, -1))
    tail_kept(torch, who, d_out, cpf)


# ---- (b) a dense batch: 684 frames of 2048 x 1024, five distinct ones repeated --------------------------------------------------------------------
DENSE = (2048, 1024)
N_DENSE, K_DENSE = 684, 5


def test_the_dense_batch_is_what_the_cases_assume():
    """(no GPU work) frame 683 of the 4:2:0 coefficients starts past 2^32 bytes, and a frame does not divide 2^32"""
    W, H = DENSE
    frame = (W // 16) * (H // 16) * 384 * 2
    assert frame == 6291456 and (N_DENSE - 1) * frame == 4297064448 > 1 << 32 and phase_shows(frame) and N_DENSE % K_DENSE


@functools.lru_cache(maxsize=None)
def dense_coefficients(mode, j):
    """the model's coefficients of source frame j under the mode (planar and packed entries read the same pixels)"""
    W, H = DENSE
    out = np.asarray(coefficient_model(mode, W, H)(*[p.reshape(-1) for p in rgb(W, H, j)]), np.int16).reshape(-1)
    out.setflags(write=False)
    return out


def dense_encoders(J):
    W, H = DENSE
    out = {}
    for mode in ("420", "gray", "444", "average"):
        out[f"fdct_quant-{mode}"] = lambda mode=mode: enc_planar(J, mode, W, H, None, K=K_DENSE)
    for mode in ("420", "444", "average"):
        out[f"fdct_quant_packed-{mode}"] = lambda mode=mode: enc_packed(J, mode, "PIX_RGB24", W, H, None, None, K=K_DENSE)
    for mode in ("420", "gray"):
        out[f"fdct_quant_ycc-{mode}"] = lambda mode=mode: enc_ycc(J, mode, W, H, None, None, None, None, K=K_DENSE)
    return out


@pytest.mark.parametrize("case", sorted(dense_encoders(None)))
def test_dense_batch_encoders(J, torch, ctx, case):
    """every frame's coefficients against the model's for its source, on the device"""
    form = dense_encoders(J)[case]()
    n = N_DENSE
    if form.mode == "average":
        ctx.set_chroma_downsampling(J.DOWNSAMPLE_AVERAGE)
    if case.startswith("fdct_quant_ycc"):
        wants = [np.asarray(form.model(src), np.int16).reshape(-1) for src in form.sources]
    else:
        wants = [dense_coefficients(form.mode, j) for j in range(K_DENSE)]
    bufs = AP.place_frames(torch, form.surfaces, form.sources, n, [])
    d_co = marked(torch, n * form.cpf, torch.int16)
    form.call(ctx, bufs, n, d_co[:n * form.cpf])
    torch.cuda.synchronize()
    del bufs
    expect_equal(form.name, "frame", d_co[:n * form.cpf].view(n, form.cpf), torch.from_numpy(np.stack(wants)).to(AP.DEVICE),
                 torch.arange(n, device=AP.DEVICE) % K_DENSE)
    tail_kept(torch, form.name, d_co, n * form.cpf)


def dense_decoders(J):
    W, H = DENSE
    rg = inner_region(W, H, 1)
    return {"dequant_idct": lambda: decoder(J, "dequant_idct_dev", "own", W, H, K=K_DENSE),
            "generic-422": lambda: decoder(J, "dequant_idct_generic_dev", "422", W, H, K=K_DENSE),
            "scaled2-422": lambda: decoder(J, "dequant_idct_scaled_dev", "422", W, H, scale=2, K=K_DENSE),
            "upsampling-own": lambda: decoder(J, "dequant_idct_upsampling_dev", "own", W, H, smooth=True, K=K_DENSE),
            "region-smooth-own": lambda: decoder(J, "dequant_idct_region_dev", "own", W, H, smooth=True, region=rg, K=K_DENSE)}


@pytest.mark.parametrize("case", sorted(dense_decoders(None)))
def test_dense_batch_decoders(J, torch, ctx, case):
    """684 frames whose coefficients pass 2^32 bytes (the any-layout entries' sample scratch in the context too): every frame against the
    model's picture of its source, on the device"""
    form = dense_decoders(J)[case]()
    n = N_DENSE
    surfaces = [AP.Surface(r, rb) for r, rb in form.shapes]
    wants = [form.model(f) for f in form.fields]
    d_co = AP.place_fields(torch, form.fields, n, stamp=False)
    bufs = [AP.alloc(torch, s, n) for s in surfaces]
    form.call(ctx, d_co, n, bufs, surfaces)
    torch.cuda.synchronize()
    del d_co
    which = torch.arange(n, device=AP.DEVICE) % K_DENSE
    for k, (s, buf) in enumerate(zip(surfaces, bufs)):
        stack = torch.from_numpy(np.stack([np.ascontiguousarray(w[k], np.uint8).reshape(s.rows, s.row_bytes) for w in wants])).to(AP.DEVICE)
        expect_equal(f"{form.name}, output {k}", "frame", buf.as_strided((n, s.rows, s.row_bytes), (s.frame_stride, s.row_stride, 1)), stack, which)
    AP.check_gaps(form.name, surfaces, bufs, n, [n - 1])


@pytest.mark.parametrize("sampling", ["420", "444"])
def test_dense_batch_histogram(J, torch, ctx, sampling):
    W, H = DENSE
    n, smp = N_DENSE, getattr(J, "SAMPLING_" + sampling)
    fields = own_fields(J, sampling, W, H, K_DENSE)
    wants = np.stack([J.huffman_histogram(f, W, H, smp).astype(np.int64).reshape(-1) for f in fields])
    d_co = AP.place_fields(torch, fields, n, stamp=False)
    d_hist = marked(torch, n * 1024, torch.int64)
    ctx.huffman_histogram_dev(d_co, W, H, d_hist[:n * 1024].view(n, 4, 256), n_frames=n, sampling=smp)
    torch.cuda.synchronize()
    who = f"huffman_histogram_dev {sampling} {W}x{H}"
    expect_equal(who, "frame", d_hist[:n * 1024].view(n, 1024), torch.from_numpy(wants).to(AP.DEVICE), torch.arange(n, device=AP.DEVICE) % K_DENSE)
    tail_kept(torch, who, d_hist, n * 1024)


@pytest.mark.parametrize("sampling", ["420", "444"])
def test_dense_batch_writer(J, torch, ctx, sampling):
    """sparse fields, slots of jpeg_bound bytes: the slots pass 2^32 bytes as well, and the batch is coded in several passes.  Every
    frame's file and size against J.write_jpeg of its source"""
    W, H = DENSE
    n, smp = N_DENSE, getattr(J, "SAMPLING_" + sampling)
    mc, mr, bpm = J.sampling_geometry(smp, W, H)
    fields = [random_field(mc * mr, bpm, 31 + j, density=0.02) for j in range(K_DENSE)]
    files = [np.frombuffer(J.write_jpeg(f, W, H, sampling=smp), np.uint8) for f in fields]
    stride = J.jpeg_bound(W, H, smp)
    d_co = AP.place_fields(torch, fields, n, stamp=False)
    d_out = marked(torch, n * stride, torch.uint8)
    d_sizes = torch.full((n + 2,), -77, dtype=torch.int64, device=AP.DEVICE)
    ctx.write_jpeg_gpu_dev(d_co, W, H, d_out[:n * stride], d_sizes[:n], n_frames=n, sampling=smp)
    torch.cuda.synchronize()
    who = f"write_jpeg_gpu_dev {sampling} {W}x{H}"
    which = torch.arange(n, device=AP.DEVICE) % K_DENSE
    lens = torch.tensor([f.size for f in files], dtype=torch.int64, device=AP.DEVICE)
    expect_equal(who + " sizes", "frame", d_sizes[:n].view(n, 1), lens.view(-1, 1), which)
    assert bool((d_sizes[n:] == -77).all()), "sizes behind the last frame were written"
    for j, f in enumerate(files):
        frames = len(range(j, n, K_DENSE))
        got = d_out.as_strided((frames, f.size), (K_DENSE * stride, 1), j * stride)
        bad = AP.first_mismatch(got, torch.from_numpy(f.copy()).to(AP.DEVICE).view(1, -1))
        if bad is not None:
            idx, off, g, w = bad
            raise AssertionError(f"{who}: frame {j + K_DENSE * idx[0]}: byte {idx[1]} of the file is {g}, the host writer's {w}; first difference "
                                 f"at {AP.where(off)}")
    tail_kept(torch, who, d_out, n * stride)


# ==== the table: method -> variant -> (P1, P2, P3, P4) ==============================================================================================
# A cell names tests of this module (name[case], shell patterns allowed) or of another (file.py::name), separated by ", ", or is
# "n/a: <reason>".
NO_ROWS = "n/a: planes and coefficient fields have no row stride"
NO_STRIDE = "n/a: no stride argument: the frames' fields lie one behind the other"
P4_ELSEWHERE = ("n/a: the huge frame and the dense batch run the planar and any-layout entries; this entry shares their kernels and differs in "
                "its output stage, whose frame and row offsets P2 and P3 take past 2^32")
ONE_SCALE = "n/a: P4 runs one reduced scale, 1/2; the scales differ in the block size alone, which P1 to P3 vary"
SPLITS = "test_gpu_launch_splits.py::"


def _scaled_rows():
    out = {}
    for scale in SCALES:
        p1 = f"test_decoders_across_the_launch_split[scaled{scale}-planes]"
        if scale == 4:
            p1 += ", test_gpu_scaled.py::test_device_batch_above_the_grid_limit"
        p4 = {1: "test_dense_batch_decoders[generic-422], test_decoder_on_one_frame_of_2_gigapixels[generic-422]",
              2: "test_dense_batch_decoders[scaled2-422], test_decoder_on_one_frame_of_2_gigapixels[scaled2]"}.get(scale, ONE_SCALE)
        out[f"planes 1/{scale}"] = (p1, f"test_decoders_with_frames_4_gib_apart[scaled{scale}-planes-*]", NO_ROWS, p4)
        out[f"packed 1/{scale}"] = (f"test_decoders_across_the_launch_split[scaled{scale}-packed]",
                                    f"test_decoders_with_frames_4_gib_apart[scaled{scale}-packed-*]",
                                    f"test_decoders_with_rows_across_4_gib[scaled{scale}-packed]", P4_ELSEWHERE)
    return out


def _region_rows():
    out = {}
    for scale in SCALES:
        for kind in ("nearest", "smooth"):
            p1 = f"test_decoders_across_the_launch_split[region{scale}-planes-{kind}]"
            if (scale, kind) == (2, "nearest"):
                p1 += ", test_gpu_region.py::test_device_batch_above_the_grid_limit"
            p4 = "test_dense_batch_decoders[region-smooth-own]" if (scale, kind) == (1, "smooth") else \
                "n/a: the dense batch runs the window entry once, smooth at full size; it has no scratch that grows with the batch"
            out[f"planes {kind} 1/{scale}"] = (p1, f"test_decoders_with_frames_4_gib_apart[region{scale}-planes-{kind}-*]", NO_ROWS, p4)
            out[f"packed {kind} 1/{scale}"] = (f"test_decoders_across_the_launch_split[region{scale}-packed-{kind}]",
                                               f"test_decoders_with_frames_4_gib_apart[region{scale}-packed-{kind}-*]",
                                               f"test_decoders_with_rows_across_4_gib[region{scale}-packed-{kind}]", P4_ELSEWHERE)
    return out


def _encoder_row(entry, modes, p1, p3):
    return {mode: (p1(mode), f"test_encoders_with_frames_4_gib_apart[{entry}-{mode}-*]", p3(mode),
                   f"test_dense_batch_encoders[{entry}-{mode}]" +
                   (f", test_encoder_on_one_frame_of_2_gigapixels[{mode}]" if entry == "fdct_quant" else "")) for mode in modes}


COVERAGE = {
    "fdct_quant_dev": _encoder_row(
        "fdct_quant", ("420", "gray", "444", "average"),
        lambda m: f"test_encoders_across_the_launch_split[fdct_quant-{m}]" if m in ("444", "average") else
        SPLITS + "test_fdct_quant_dev_across_launch_splits, " + SPLITS + "test_fdct_quant_dev_ragged_frames_across_the_split",
        lambda m: NO_ROWS),
    "fdct_quant_packed_dev": _encoder_row(
        "fdct_quant_packed", ("420", "444", "average"), lambda m: f"test_encoders_across_the_launch_split[fdct_quant_packed-*-{m}]",
        lambda m: f"test_packed_encoder_with_rows_across_4_gib[{m}*]"),
    "fdct_quant_ycc_dev": _encoder_row(
        "fdct_quant_ycc", ("420", "gray"), lambda m: f"test_encoders_across_the_launch_split[fdct_quant_ycc-{m}]" +
        (", test_gpu_ycc.py::test_encode_across_the_launch_split" if m == "420" else ""),
        lambda m: f"test_ycc_encoder_with_rows_across_4_gib[{m}]"),
    "dequant_idct_dev": {"planes": (
        SPLITS + "test_dequant_idct_dev_across_launch_split", "test_decoders_with_frames_4_gib_apart[dequant_idct-planes-*]", NO_ROWS,
        "test_dense_batch_decoders[dequant_idct], test_decoder_on_one_frame_of_2_gigapixels[dequant_idct]")},
    "dequant_idct_packed_dev": {"packed": (
        "test_decoders_across_the_launch_split[dequant_idct_packed]", "test_decoders_with_frames_4_gib_apart[dequant_idct_packed-*]",
        "test_decoders_with_rows_across_4_gib[dequant_idct_packed*]", P4_ELSEWHERE)},
    "dequant_idct_ycc_dev": {"ycc": (
        "test_decoders_across_the_launch_split[dequant_idct_ycc]", "test_decoders_with_frames_4_gib_apart[dequant_idct_ycc-*]",
        "test_decoders_with_rows_across_4_gib[dequant_idct_ycc]", P4_ELSEWHERE)},
    "dequant_idct_generic_dev": {"planes": (
        SPLITS + "test_generic_batch_decode_across_launch_split", "test_decoders_with_frames_4_gib_apart[generic-planes-*]", NO_ROWS,
        "test_dense_batch_decoders[generic-422], test_decoder_on_one_frame_of_2_gigapixels[generic-422]")},
    "dequant_idct_scaled_dev": _scaled_rows(),
    "dequant_idct_upsampling_dev": {
        "planes smooth": ("test_decoders_across_the_launch_split[upsampling-planes-*]", "test_decoders_with_frames_4_gib_apart[upsampling-planes-*]",
                          NO_ROWS, "test_dense_batch_decoders[upsampling-own], test_decoder_on_one_frame_of_2_gigapixels[upsampling]"),
        "packed smooth": ("test_decoders_across_the_launch_split[upsampling-packed-*]", "test_decoders_with_frames_4_gib_apart[upsampling-packed-*]",
                          "test_decoders_with_rows_across_4_gib[upsampling-packed]", P4_ELSEWHERE),
        "nearest": ("n/a: UPSAMPLE_NEAREST hands the call to dequant_idct_generic_dev's launcher (test_gpu_smooth.py::test_nearest_is_the_"
                    "existing_decode), whose row this is",) * 4},
    "dequant_idct_region_dev": _region_rows(),
    "coeff_transform_dev": {
        "420": ("test_transform_across_the_launch_split[*-420]", NO_STRIDE, NO_ROWS, "test_transform_on_one_frame_of_2_gigapixels[*]"),
        "444": ("test_transform_across_the_launch_split[*-444]", NO_STRIDE, NO_ROWS,
                "n/a: the huge frame is set for 4:2:0; both samplings share the kernel and differ in the MCU's block table, which P1 varies")},
    "huffman_histogram_dev": {s: (f"test_histogram_across_the_launch_split[{s}-*]", NO_STRIDE, NO_ROWS, f"test_dense_batch_histogram[{s}]")
                              for s in ("420", "444")},
    "write_jpeg_gpu_dev": {
        "420": (SPLITS + "test_gpu_writer_across_the_65535_frame_split", "test_writer_with_slots_4_gib_apart[420]", NO_ROWS,
                "test_dense_batch_writer[420]"),
        "444": ("test_writer_444_across_the_launch_split", "test_writer_with_slots_4_gib_apart[444]", NO_ROWS, "test_dense_batch_writer[444]")},
}


def batch_methods():
    """the methods of jpezy_amd.api.Context the table is about: *_dev, with an n_frames parameter or frames from the leading dimension
    of a pixel tensor (d_img: packed pixels, d_y: the luma plane)"""
    from jpezy_amd import api
    return {n for n, f in inspect.getmembers(api.Context, inspect.isfunction)
            if n.endswith("_dev") and {"n_frames", "d_img", "d_y"} & set(inspect.signature(f).parameters)}


def module_ids():
    """the ids pytest gives the tests of this module, from their parametrize marks (the mark nearest the function comes first)"""
    import itertools
    out = set()
    for name, fn in list(globals().items()):
        if not (name.startswith("test_") and inspect.isfunction(fn)):
            continue
        axes = [["-".join(str(x) for x in (v if isinstance(v, (tuple, list)) else (v,))) for v in m.args[1]]
                for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]
        out |= {f"{name}[{'-'.join(c)}]" for c in itertools.product(*axes)} if axes else {name}
    return out


def check_table():
    """every derived method has a row, every row a method; every cell is n/a with a reason or names tests that exist"""
    methods = batch_methods()
    assert len(methods) >= 13, ("the derivation is broken", sorted(methods))
    assert methods == set(COVERAGE), ("methods without a row", sorted(methods - set(COVERAGE)), "rows without a method", sorted(set(COVERAGE) - methods))
    ids = module_ids()
    here = Path(__file__).resolve().parent
    for method, variants in COVERAGE.items():
        assert variants, method
        for variant, cells in variants.items():
            assert len(cells) == 4, (method, variant, "one cell per procedure")
            for p, cell in enumerate(cells, 1):
                if cell.startswith("n/a: "):
                    assert len(cell) > 20, (method, variant, p, "n/a needs its reason")
                    continue
                for token in cell.split(", "):
                    if "::" in token:
                        file, name = token.split("::")
                        assert re.search(rf"^def {re.escape(name)}\(", (here / file).read_text(), re.M), (method, variant, p, "no such test", token)
                    else:
                        assert fnmatch.filter(ids, token.replace("[", "[[]", 1)), (method, variant, p, "names no test of this module", token)
