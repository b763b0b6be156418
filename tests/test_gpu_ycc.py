"""Planar YCbCr 4:2:0 samples in and out (I420 / NV12 / NV21): every comparison is for equality with the restatement of the definition
in tests/ycc_model.py.  What is varied is what selects another load / store form or another path: W % 16, strides and base addresses,
planar or interleaved chroma, the workgroup shape (quads per row), gray, the encode variant, the exact-path hooks, the ends of the
sample range.  Padding, the bytes in front of an offset base and behind the last row are 0xA5 and must still be after a decode."""
import functools
import io
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ycc_model as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FILL = 0xA5
E_NOSPACE = -6
INT_MIN = -2 ** 31
SMALL = [(1, 1), (7, 5), (15, 17), (65, 47), (100, 100), (16, 16), (64, 16)]
LARGE = [(208, 40), (976, 33), (1024, 16), (2048, 7), (1920, 24)]    # 976: last quad with one live MCU; 1920: quads per row not a multiple of 4
ANCHOR = [(16, 16), (64, 16), (1, 1), (7, 5), (15, 17), (65, 47), (976, 33), (1024, 16), (2048, 7)]   # W, H each a multiple of 16 or odd
NO_ANCHOR = [(100, 100), (208, 40), (1920, 24)]     # an even edge that is no multiple of 16: gray and the luma blocks agree, chroma need not
FORMATS = ["i420", "nv12", "nv21"]


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def padded(tight, pad):
    return {"tight": tight, "pad16": (tight + 15) // 16 * 16 + 16, "pad5": tight + 5}[pad]


class Planes:
    """Host buffers (0xA5 everywhere but the samples) and device views of n frames in one of the three formats."""

    def __init__(self, torch, n, W, H, fmt, pad="tight", base=0, frame_gap=0, frames=None):
        self.W, self.H, self.n, self.fmt = W, H, n, fmt
        CW, CH = M.chroma_size(W, H)
        step = 1 if fmt == "i420" else 2
        self.ys, self.cs = padded(W, pad), padded(CW * step, pad)
        self.yfs, self.cfs = H * self.ys + frame_gap, CH * self.cs + frame_gap
        self.hy = np.full(base + n * self.yfs + 64, FILL, np.uint8)
        nc = 2 if fmt == "i420" else 1
        self.hc = [np.full(base + n * self.cfs + 64, FILL, np.uint8) for _ in range(nc)]
        ast = np.lib.stride_tricks.as_strided
        self.vy = ast(self.hy[base:], (n, H, W), (self.yfs, self.ys, 1))
        if fmt == "i420":
            self.vcb, self.vcr = (ast(h[base:], (n, CH, CW), (self.cfs, self.cs, 1)) for h in self.hc)
        else:
            uv = ast(self.hc[0][base:], (n, CH, CW, 2), (self.cfs, self.cs, 2, 1))
            self.vcb, self.vcr = (uv[..., 0], uv[..., 1]) if fmt == "nv12" else (uv[..., 1], uv[..., 0])
        if frames is not None:
            for f, (y, cb, cr) in enumerate(frames):
                self.vy[f], self.vcb[f], self.vcr[f] = y, cb, cr
        self.dy = torch.from_numpy(self.hy).to("cuda:0")
        self.dc = [torch.from_numpy(h).to("cuda:0") for h in self.hc]

        def view(flat, shape, strides, off):
            if n == 1:
                shape, strides = shape[1:], strides[1:]
            return torch.as_strided(flat, shape, strides, off)
        self.ty = view(self.dy, (n, H, W), (self.yfs, self.ys, 1), base)
        if fmt == "i420":
            self.tcb, self.tcr = (view(d, (n, CH, CW), (self.cfs, self.cs, 1), base) for d in self.dc)
        else:
            first, second = (view(self.dc[0], (n, CH, CW), (self.cfs, self.cs, 2), base + k) for k in (0, 1))
            self.tcb, self.tcr = (first, second) if fmt == "nv12" else (second, first)

    def device_bytes(self):
        return [self.dy.cpu().numpy()] + [d.cpu().numpy() for d in self.dc]

    def host_bytes(self):
        return [self.hy] + self.hc


def encode(J, ctx, torch, frames, W, H, fmt, gray=False, **kw):
    P = Planes(torch, len(frames), W, H, fmt, frames=frames, **kw)
    co = torch.empty(len(frames) * J.coeff_count(W, H, gray), dtype=torch.int16, device="cuda:0")
    ctx.fdct_quant_ycc_dev(P.ty, P.tcb, P.tcr, co, gray=gray)
    torch.cuda.synchronize()
    for a, e in zip(P.device_bytes(), P.host_bytes()):
        assert np.array_equal(a, e), "the encoder wrote into its input"
    return co.cpu().numpy()


def want_coeffs(W, H, kind, gray, n=1):
    return np.concatenate([M.synth_coeffs(W, H, kind, gray, f).reshape(-1) for f in range(n)])


# ---- 1. encode ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SMALL + LARGE)
def test_encode_equals_model(J, ctx, torch, size):
    W, H = size
    for gray in (False, True):
        want = want_coeffs(W, H, "random", gray)
        for variant in (0, 1):
            ctx.set_variant(variant)
            try:
                for fmt in FORMATS:
                    got = encode(J, ctx, torch, [M.synth_planes(W, H, "random")], W, H, fmt, gray)
                    assert np.array_equal(got, want), (size, gray, variant, fmt)
            finally:
                ctx.set_variant(1)


@pytest.mark.parametrize("size", ANCHOR + NO_ANCHOR)
def test_encode_of_planes_from_rgb_is_the_rgb_encode(J, ctx, torch, oracle, size):
    """the anchor: each of W and H a multiple of 16 or odd -> the coefficients of fdct_quant on the RGB pixels; at every size the gray
    coefficients and the luma blocks"""
    W, H = size
    rgb = oracle.synth_rgb(W, H)
    for gray in (False, True):
        want = want_coeffs(W, H, "rgb", gray)
        assert np.array_equal(encode(J, ctx, torch, [M.synth_planes(W, H, "rgb")], W, H, "i420", gray), want), (size, gray)
        of_rgb = ctx.fdct_quant(*rgb, W, H, gray=gray).reshape(-1)
        if gray or size in ANCHOR:
            assert np.array_equal(of_rgb, want), (size, gray)
        else:
            assert np.array_equal(of_rgb.reshape(-1, 6, 64)[:, :4], want.reshape(-1, 6, 64)[:, :4]), size


@pytest.mark.parametrize("size", [(64, 16), (65, 47), (1024, 16)])
@pytest.mark.parametrize("kind", ["pad16", "pad5", "base1", "base8", "frames2"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_encode_strides_and_base(J, ctx, torch, size, kind, fmt):
    """pad16 keeps the 16 / 8-byte load form with padded rows; pad5, an odd base and a base 8 bytes into the allocation (Y no
    longer 16-byte aligned) take the byte loop although W % 16 == 0; frames2: two frames a padded frame stride apart"""
    W, H = size
    kw = {"pad16": dict(pad="pad16"), "pad5": dict(pad="pad5"), "base1": dict(base=1), "base8": dict(base=8),
          "frames2": dict(pad="pad16", frame_gap=48)}[kind]
    n = 2 if kind == "frames2" else 1
    frames = [M.synth_planes(W, H, "random", f) for f in range(n)]
    for gray in (False, True):
        for variant in (0, 1):
            ctx.set_variant(variant)
            try:
                got = encode(J, ctx, torch, frames, W, H, fmt, gray, **kw)
            finally:
                ctx.set_variant(1)
            assert np.array_equal(got, want_coeffs(W, H, "random", gray, n)), (size, kind, fmt, gray, variant)


@pytest.mark.parametrize("force", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", ["random", "flat0", "flat255"])
def test_encode_force_levels(J, ctx, torch, force, kind):
    """levels 1-3 on the small sizes, and the ends of the sample range (chroma -128: block sum -8192, a flagged DC) at every level"""
    sizes = SMALL if kind == "random" else [(16, 16), (65, 47)]
    ctx.set_force_exact(force)
    try:
        for W, H in sizes:
            for gray in (False, True):
                for variant in ((0, 1) if force in (0, 1) else (1,)):
                    ctx.set_variant(variant)
                    for fmt in ("i420", "nv12"):
                        got = encode(J, ctx, torch, [M.synth_planes(W, H, kind)], W, H, fmt, gray)
                        assert np.array_equal(got, want_coeffs(W, H, kind, gray)), (W, H, kind, force, gray, variant, fmt)
    finally:
        ctx.set_variant(1)
        ctx.set_force_exact(0)


def test_flat_plane_dcs(J, ctx, torch):
    for kind, dl, dc in (("flat0", -63, -60), ("flat255", 63, 59)):
        co = encode(J, ctx, torch, [M.synth_planes(16, 16, kind)], 16, 16, "i420").reshape(6, 64)
        assert co[:4, 0].tolist() == [dl] * 4 and co[4:, 0].tolist() == [dc] * 2 and not co[:, 1:].any()


def test_encode_across_the_launch_split(J, ctx, torch):
    """more than 65535 frames of 1 x 1: every frame's blocks are flat, so the model is a table of 256 flat MCUs"""
    n = 65535 + 3
    v = np.arange(256, dtype=np.uint8)
    table = M.encode_coeffs(np.repeat(v, 16)[None, :].repeat(16, 0), np.repeat(v, 8)[None, :].repeat(8, 0), np.repeat(v, 8)[None, :].repeat(8, 0))[0]
    rng = np.random.default_rng(5)
    y, cb, cr = (rng.integers(0, 256, n, dtype=np.uint8) for _ in range(3))
    d = [torch.from_numpy(p.reshape(n, 1, 1)).to("cuda:0") for p in (y, cb, cr)]
    co = torch.empty(n * 6 * 64, dtype=torch.int16, device="cuda:0")
    ctx.fdct_quant_ycc_dev(d[0], d[1], d[2], co)
    torch.cuda.synchronize()
    got = co.cpu().numpy().reshape(n, 6, 64)
    assert np.array_equal(got[:, :4], table[y][:, :4]) and np.array_equal(got[:, 4], table[cb][:, 4]) and np.array_equal(got[:, 5], table[cr][:, 5])


# ---- 2. decode ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def own_file(W, H):
    """a file written by this encoder from the model's coefficients -> (bytes, info, coefficients, model planes)"""
    import jpezy_amd as J
    from oracle import oracle as O
    co = M.synth_coeffs(W, H, "rgb")
    jpg = J.write_jpeg(co.reshape(-1), W, H)
    info = O.make_info(W, H)
    planes = M.decode_planes(co, info)
    for p in planes:
        p.setflags(write=False)
    return jpg, info, co, tuple(planes)


@pytest.mark.parametrize("size", SMALL + LARGE)
def test_decode_equals_model_and_gray_decode(J, ctx, size):
    W, H = size
    jpg, _, _, want = own_file(W, H)
    gray_r = ctx.decode_jpeg(jpg, gray=True)[1].reshape(H, W)
    assert np.array_equal(want[0], gray_r)                                          # the luma anchor, on the model itself
    for interleaved in (False, True):
        info, y, cb, cr = ctx.decode_jpeg_ycc(jpg, interleaved=interleaved)
        assert (info.width, info.height) == (W, H)
        assert np.array_equal(y, gray_r), (size, interleaved)
        assert np.array_equal(cb, want[1]) and np.array_equal(cr, want[2]), (size, interleaved)


def decode_dev(J, ctx, torch, co, W, H, fmt, luma_only=False, only=None, n=1, **kw):
    """-> (Planes after the decode, device bytes)"""
    P = Planes(torch, n, W, H, fmt, **kw)
    d_co = torch.from_numpy(np.array(co).reshape(-1)).to("cuda:0")
    tcb = None if luma_only or only == "cr" else P.tcb
    tcr = None if luma_only or only == "cb" else P.tcr
    ctx.dequant_idct_ycc_dev(d_co, P.ty, tcb, tcr)
    torch.cuda.synchronize()
    return P, P.device_bytes()


@pytest.mark.parametrize("size", [(64, 16), (65, 47), (1024, 16), (976, 33)])
@pytest.mark.parametrize("kind", ["tight", "pad16", "pad5", "base1", "base8", "frames2"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_strides_bases_and_canaries(J, ctx, torch, size, kind, fmt):
    W, H = size
    kw = {"tight": {}, "pad16": dict(pad="pad16"), "pad5": dict(pad="pad5"), "base1": dict(base=1), "base8": dict(base=8),
          "frames2": dict(pad="pad16", frame_gap=48)}[kind]
    n = 2 if kind == "frames2" else 1
    _, _, co, want = own_file(W, H)
    P, got = decode_dev(J, ctx, torch, np.concatenate([co.reshape(-1)] * n), W, H, fmt, n=n, **kw)
    for f in range(n):
        P.vy[f], P.vcb[f], P.vcr[f] = want                                           # the expected image: samples over the 0xA5 fill
    for a, e in zip(got, P.host_bytes()):
        assert np.array_equal(a, e), (size, kind, fmt)


@pytest.mark.parametrize("size", [(64, 16), (65, 47)])
def test_decode_luma_only_and_single_chroma_pointer(J, ctx, torch, size):
    W, H = size
    _, _, co, want = own_file(W, H)
    for fmt in FORMATS:
        P, got = decode_dev(J, ctx, torch, co, W, H, fmt, luma_only=True)
        P.vy[0] = want[0]
        for a, e in zip(got, P.host_bytes()):
            assert np.array_equal(a, e), ("luma only", size, fmt)
        for only in ("cb", "cr"):                  # the other channel's bytes of an interleaved plane stay 0xA5
            P, got = decode_dev(J, ctx, torch, co, W, H, fmt, only=only)
            P.vy[0] = want[0]
            (P.vcb if only == "cb" else P.vcr)[0] = want[1 if only == "cb" else 2]
            for a, e in zip(got, P.host_bytes()):
                assert np.array_equal(a, e), (only, size, fmt)


@pytest.mark.parametrize("size", [(65, 47), (1024, 16)])
def test_decode_force_exact_and_tolerance(J, ctx, torch, size):
    W, H = size
    jpg, _, co, want = own_file(W, H)
    ctx.set_force_exact(1)
    try:
        for fmt in ("i420", "nv12"):
            P, got = decode_dev(J, ctx, torch, co, W, H, fmt)
            P.vy[0], P.vcb[0], P.vcr[0] = want
            for a, e in zip(got, P.host_bytes()):
                assert np.array_equal(a, e), ("force", size, fmt)
    finally:
        ctx.set_force_exact(0)
    ctx.set_decode_tolerance(1)
    try:
        _, y, cb, cr = ctx.decode_jpeg_ycc(jpg)
    finally:
        ctx.set_decode_tolerance(0)
    dy = int(np.abs(y.astype(int) - want[0].astype(int)).max())
    print(f"tolerance mode {size}: max |dY| = {dy}")
    assert dy <= 1 and np.array_equal(cb, want[1]) and np.array_equal(cr, want[2])


def _pil_file(mode, subsampling, W=93, H=61):
    from PIL import Image
    from oracle import oracle as O
    r, g, b = O.synth_rgb(W, H, frame=9)
    img = np.stack([p.reshape(H, W) for p in (r, g, b)], -1) // 2 + 40
    buf = io.BytesIO()
    if mode == "L":
        Image.fromarray(img[..., 0].astype(np.uint8), "L").save(buf, "JPEG", quality=85)
    else:
        Image.fromarray(img.astype(np.uint8), "RGB").save(buf, "JPEG", quality=85, subsampling=subsampling)
    return buf.getvalue()


@pytest.mark.parametrize("layout", ["444", "422", "one_component"])
def test_decode_other_layouts_of_pil_files(J, ctx, oracle, layout):
    data = _pil_file("L" if layout == "one_component" else "RGB", {"444": 0, "422": 1}.get(layout))
    info_o, co = oracle.read_jpeg(data)
    want = M.decode_planes(co, info_o)
    for interleaved in ((False,) if layout == "one_component" else (False, True)):
        info, y, cb, cr = ctx.decode_jpeg_ycc(data, interleaved=interleaved)
        assert (info.ncomp, info.hmax, info.vmax) == (info_o.ncomp, info_o.hmax, info_o.vmax)
        assert np.array_equal(y, want[0]), layout
        if layout == "one_component":
            assert cb is None and cr is None
        else:
            assert np.array_equal(cb, want[1]) and np.array_equal(cr, want[2]), (layout, interleaved)
    assert np.array_equal(y.reshape(-1), ctx.decode_jpeg(data, gray=True)[1])


@pytest.mark.parametrize("layout", ["420", "444"])
def test_decode_16bit_quantiser_file_whose_samples_leave_int32(J, ctx, oracle, layout):
    from test_gpu_decode_range import L420, L444, _overflow_file
    data, _, _ = _overflow_file({"420": L420, "444": L444}[layout])
    info_o, co = oracle.read_jpeg(data)
    smp = M.decode_samples(co, info_o)
    allv = np.concatenate([s.reshape(-1) for s in smp])
    assert allv.max() > 255 and ((allv < 0) & (allv != INT_MIN)).any() and (allv == INT_MIN).any()          # both sides, and outside int32
    want = M.decode_planes(co, info_o)
    _, y, cb, cr = ctx.decode_jpeg_ycc(data)
    assert np.array_equal(y, want[0]) and np.array_equal(cb, want[1]) and np.array_equal(cr, want[2])
    assert np.array_equal(y.reshape(-1), ctx.decode_jpeg(data, gray=True)[1])



def test_decode_buffer_too_small_and_header_only(J, ctx):
    import ctypes as C
    lib = J.load_library()
    jpg = own_file(65, 47)[0]
    arr = np.frombuffer(jpg, np.uint8)
    info = J.FrameInfo()
    assert lib.jpezy_decode_jpeg_ycc(ctx._h, arr.ctypes.data, arr.size, C.byref(info), None, 0, 0, None, None, 0, 1, 0) == 0
    assert (info.width, info.height) == (65, 47)
    y, c = np.full(65 * 47, FILL, np.uint8), np.full(33 * 24, FILL, np.uint8)
    assert lib.jpezy_decode_jpeg_ycc(ctx._h, arr.ctypes.data, arr.size, C.byref(info), y.ctypes.data, 0, y.size - 1, c.ctypes.data, c.ctypes.data, 0, 1, c.size) == E_NOSPACE
    assert lib.jpezy_decode_jpeg_ycc(ctx._h, arr.ctypes.data, arr.size, C.byref(info), y.ctypes.data, 0, y.size, c.ctypes.data, c.ctypes.data, 0, 1, c.size - 1) == E_NOSPACE
    assert (y == FILL).all() and (c == FILL).all()


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(65, 47), (208, 40), (1920, 24)])
@pytest.mark.parametrize("mode", ["plain", "optimize", "restart"])
def test_encode_jpeg_ycc_bytes(J, ctx, size, mode):
    W, H = size
    mc = (W + 15) // 16
    y, cb, cr = M.synth_planes(W, H, "rgb")
    uv = np.stack([cb, cr], -1)
    ctx.set_huffman_optimize(mode == "optimize")
    ctx.set_restart_interval(mc if mode == "restart" else 0)
    try:
        for gray in (False, True):
            co = M.synth_coeffs(W, H, "rgb", gray).reshape(-1)
            want = J.write_jpeg(co, W, H, gray=gray, optimize=mode == "optimize", restart_interval=mc if mode == "restart" else 0)
            assert ctx.encode_jpeg_ycc(y, cb, cr, gray=gray) == want, (size, mode, gray, "i420")
            assert ctx.encode_jpeg_ycc(y, uv[..., 0], uv[..., 1], gray=gray) == want, (size, mode, gray, "nv12")
    finally:
        ctx.set_huffman_optimize(False)
        ctx.set_restart_interval(0)


@pytest.mark.parametrize("fmt", FORMATS + ["padded"])
def test_encode_jpeg_ycc_in_several_bands(J, fmt):
    """host_chunk_bytes forced small: bands of one MCU row each (on a context of its own, so that the shared one keeps its chunk size)"""
    W, H = 208, 100
    y, cb, cr = M.synth_planes(W, H, "random")
    want = J.write_jpeg(M.synth_coeffs(W, H, "random").reshape(-1), W, H)
    c = J.Context(0)
    try:
        c.set_host_chunk_bytes(4096)
        if fmt == "i420":
            args = (y, cb, cr)
        elif fmt == "padded":
            big = [np.full((p.shape[0], p.shape[1] + 13), FILL, np.uint8) for p in (y, cb, cr)]
            for b, p in zip(big, (y, cb, cr)):
                b[:, :p.shape[1]] = p
            args = tuple(b[:, :p.shape[1]] for b, p in zip(big, (y, cb, cr)))
        else:
            uv = np.stack([cb, cr] if fmt == "nv12" else [cr, cb], -1)
            args = (y, uv[..., 0], uv[..., 1]) if fmt == "nv12" else (y, uv[..., 1], uv[..., 0])
        assert c.encode_jpeg_ycc(*args) == want, fmt
        assert c.encode_jpeg_ycc(y, gray=True) == J.write_jpeg(M.synth_coeffs(W, H, "random", True).reshape(-1), W, H, gray=True)
    finally:
        c.close()


@pytest.mark.parametrize("size", [(33, 17), (100, 100), (1024, 16)])
def test_round_trip(J, ctx, oracle, size):
    W, H = size
    y, cb, cr = M.synth_planes(W, H, "rgb")
    jpg = ctx.encode_jpeg_ycc(y, cb, cr)
    info_o, co = oracle.read_jpeg(jpg)
    assert np.array_equal(co.reshape(-1), M.synth_coeffs(W, H, "rgb").reshape(-1))
    want = M.decode_planes(co, info_o)
    _, y2, cb2, cr2 = ctx.decode_jpeg_ycc(jpg, interleaved=True)
    assert np.array_equal(y2, want[0]) and np.array_equal(cb2, want[1]) and np.array_equal(cr2, want[2])


def test_cli_pair(J, tmp_path):
    from jpezy_amd import _build
    _build.build_all()
    enc, dec = ROOT / "jpezy_amd" / "bin" / "jpezy_encode", ROOT / "jpezy_amd" / "bin" / "jpezy_decode"
    W, H = 33, 17
    y, cb, cr = M.synth_planes(W, H, "rgb")
    src, jpg, back = tmp_path / "in.yuv", tmp_path / "out.jpg", tmp_path / "back.yuv"
    src.write_bytes(y.tobytes() + cb.tobytes() + cr.tobytes())
    run = lambda *a: subprocess.run([str(x) for x in a], capture_output=True, text=True, timeout=300)
    p = run(enc, f"--i420={W}x{H}", src, jpg)
    assert p.returncode == 0, p.stderr
    co = M.synth_coeffs(W, H, "rgb")
    assert jpg.read_bytes() == J.write_jpeg(co.reshape(-1), W, H)
    p = run(dec, "--i420", jpg, back)
    assert p.returncode == 0, p.stderr
    from oracle import oracle as O
    want = M.decode_planes(co, O.make_info(W, H))
    assert back.read_bytes() == b"".join(w.tobytes() for w in want)
    # --gray, --optimize, --restart keep their meaning
    p = run(enc, f"--i420={W}x{H}", src, jpg, "--gray", "--optimize", "--restart=3")
    assert p.returncode == 0, p.stderr
    assert jpg.read_bytes() == J.write_jpeg(M.synth_coeffs(W, H, "rgb", True).reshape(-1), W, H, gray=True, optimize=True, restart_interval=3)
    # a file of another layout is refused with a message
    other = tmp_path / "444.jpg"
    other.write_bytes(_pil_file("RGB", 0))
    p = run(dec, "--i420", other, back)
    assert p.returncode == 1 and "4:2:0" in p.stderr
    # a plane file of the wrong size
    src.write_bytes(b"\0" * 10)
    p = run(enc, f"--i420={W}x{H}", src, jpg)
    assert p.returncode == 1 and "bytes" in p.stderr
