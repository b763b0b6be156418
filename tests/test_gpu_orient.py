"""Oriented output on the GPU (include/jpezy_hip_orientation.h): every byte equal to tests/orient_model.py's permutation of the bytes the
EXISTING decode returns.  The picture P of a (file, scale, upsampling) is decoded once through the entry without an orientation; every
oriented window must be orient(P, o) sliced.  Varied: what a store stage that reads its samples through a mirrored or transposed map can
get wrong -- the layout (which rows and columns replicate, which are smoothed), N, windows at the corners, across an interior MCU corner
from an odd origin, one pixel wide or high, the store forms, odd strides and pointers, batches of frames, streams, the window batches and
their two paths.  All windows of a (file, scale, upsampling) go into ONE marker-filled device buffer that is compared whole, so a byte
written outside an output shows.  There is no tolerance: every comparison is exact."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import orient_model as OM
import region_smooth_cases as K
import resize_filter_model as FM
import resize_model as RM
import scaled_model as M
import tensor_model as TM

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
FILL = K.FILL
GUARD = 8
# one file per layout class the body distinguishes: (layout, W, H)
FILES = [("own", 33, 17), ("own", 16, 16), ("444", 9, 23), ("h2v1", 40, 24), ("h1v2", 24, 40), ("one", 17, 33), ("411", 35, 10), ("own", 1, 1)]
SMOOTHED = ("own", "h2v1", "h1v2")


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


def windows(info, scale, o):
    """{name: (x, y, w, h)} in the ORIENTED picture at 1/scale"""
    n = 8 // scale
    Ws, Hs = M.scaled_size(info.width, info.height, scale)
    Wo, Ho = OM.size(o, Ws, Hs)
    mw, mh = info.hmax * n, info.vmax * n
    out = {"whole": (0, 0, Wo, Ho), "corner_00": (0, 0, 1, 1), "corner_10": (Wo - 1, 0, 1, 1), "corner_01": (0, Ho - 1, 1, 1),
           "corner_11": (Wo - 1, Ho - 1, 1, 1), "column": (Wo // 2, 0, 1, Ho), "row": (0, Ho // 2, Wo, 1)}
    if mw < Ws and mh < Hs:
        # two pixels on either side of the first interior MCU corner of the SOURCE, seen in the oriented picture, then from an odd origin
        sx0, sy0 = max(mw - 2, 0), max(mh - 2, 0)
        x, y, w, h = OM.window_of(o, Ws, Hs, (sx0, sy0, min(mw + 2, Ws) - sx0, min(mh + 2, Hs) - sy0))
        if x % 2 == 0:
            x, w = (x + 1, w - 1) if w >= 4 else (x - 1, w + 1) if x > 0 else (x, w)
        if y % 2 == 0:
            y, h = (y + 1, h - 1) if h >= 4 else (y - 1, h + 1) if y > 0 else (y, h)
        sx, sy, sw, sh = OM.rect(o, Ws, Hs, (x, y, w, h))
        if sx // mw != (sx + sw - 1) // mw and sy // mh != (sy + sh - 1) // mh:
            out["four_mcu_corner_odd_origin"] = (x, y, w, h)
    if Wo > 2:
        out["left_edge_1_mod_4"] = (1, 0, Wo - 2, Ho)
    if Wo > 6:
        out["left_edge_5"] = (5, 0, Wo - 6, Ho)
    return out


def existing_picture(torch, ctx, d_co, info, scale, upsampling, gray=False):
    """P: the whole picture through the entry WITHOUT an orientation, [Hs, Ws, 3] (r, g, b)"""
    Ws, Hs = M.scaled_size(info.width, info.height, scale)
    out = [torch.empty(Ws * Hs, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    ctx.dequant_idct_region_dev(d_co, info, (0, 0, Ws, Hs), scale, *out, gray=gray, upsampling=upsampling)
    torch.cuda.synchronize()
    P = np.stack([o.cpu().numpy().reshape(Hs, Ws) for o in out], axis=-1)
    P.setflags(write=False)
    return P


class Arena:
    """one marker-filled device buffer; outputs are carved out of it with guard bytes between them, the expectation is built beside it"""

    def __init__(self, torch, nbytes):
        self.buf = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda:0")
        self.exp = np.full(nbytes, FILL, np.uint8)
        self.at = GUARD
        self.tags = []

    def take(self, nbytes, tag, misalign=0):
        at = (self.at + 3) // 4 * 4 + misalign
        self.at = at + nbytes + GUARD
        assert self.at <= self.exp.size
        self.tags.append((at, tag))
        return at

    def check(self, torch):
        torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        bad = np.nonzero(got != self.exp)[0]
        if bad.size:
            first = int(bad[0])
            tag = [t for a, t in self.tags if a <= first + GUARD][-1:]      # (a byte in a guard belongs to the output behind or in front)
            raise AssertionError(("first differing byte", first, "got", int(got[first]), "want", int(self.exp[first]), "count", int(bad.size), "in", tag))


def run_windows(J, torch, ctx, data, d_co, info, scale, upsampling, orientations=OM.ORIENTATIONS, frames=1, files=None, stream=None):
    """every window of every orientation through both device entries into one arena; returns the number of launches"""
    P = [existing_picture(torch, ctx, d_co[f * (d_co.numel() // frames):], info, scale, upsampling) for f in range(frames)] if frames > 1 else \
        [existing_picture(torch, ctx, d_co, info, scale, upsampling)]
    Ws, Hs = M.scaled_size(info.width, info.height, scale)
    arena = Arena(torch, (len(list(orientations)) * 12 * (7 * Ws * Hs + 64 * (Ws + Hs) + 256) + 4096) * frames)
    launches = 0
    kw = {} if stream is None else dict(stream=stream.cuda_stream)
    for o in orientations:
        O = [OM.orient(p, o) for p in P]
        for k, (name, win) in enumerate(windows(info, scale, o).items()):
            x, y, w, h = win
            want = [q[y:y + h, x:x + w] for q in O]
            assert want[0].shape[:2] == (h, w), (o, name, win)
            tag = (info.width, info.height, scale, upsampling, o, name, win)
            # planes: frames a plane and three bytes apart
            stride = w * h + (3 if frames > 1 else 0)
            at = [arena.take(frames * stride, tag + ("plane", c)) for c in range(3)]
            ctx.dequant_idct_region_dev(d_co, info, win, scale, *[arena.buf[a:] for a in at], n_frames=frames, plane_stride=stride, upsampling=upsampling,
                                        orientation=o, **kw)
            for c in range(3):
                for f in range(frames):
                    arena.exp[at[c] + f * stride:at[c] + f * stride + w * h] = want[f][:, :, c].reshape(-1)
            # packed: RGB24 and BGRA32 in turn, an odd row stride, a pointer one byte off a multiple of four
            fmt = (J.PIX_RGB24, J.PIX_BGRA32)[(k + o) % 2]
            nb = 3 if fmt == J.PIX_RGB24 else 4
            row = (w * nb) | 1 if (w * nb) % 2 == 0 else w * nb + 2
            frame = h * row + 5
            a = arena.take(frames * frame, tag + ("packed", fmt), misalign=1)
            d_img = arena.buf.as_strided((frames, h, w, nb), (frame, row, nb, 1), a) if frames > 1 else arena.buf.as_strided((h, w, nb), (row, nb, 1), a)
            ctx.dequant_idct_region_dev(d_co, info, win, scale, d_img=d_img, format=fmt, upsampling=upsampling, orientation=o, **kw)
            for f in range(frames):
                img = K.interleave(J, fmt, [want[f][:, :, c] for c in range(3)])
                for j in range(h):
                    arena.exp[a + f * frame + j * row:a + f * frame + j * row + w * nb] = img[j].reshape(-1)
            launches += 2
    if stream is not None:
        stream.synchronize()
    arena.check(torch)
    return launches


# ---- 1. every file, orientation, scale, upsampling, window, through the two device entries ----------------------------------------------
@pytest.mark.parametrize("layout,W,H", FILES, ids=[f"{l}-{w}x{h}" for l, w, h in FILES])
def test_every_oriented_window_is_the_existing_decode_permuted(J, torch, ctx, layout, W, H):
    data = K.jpeg(layout, W, H)
    info, d_co = ctx.read_jpeg_gpu(data)
    launches = 0
    for scale in K.SCALES:
        for up in (J.UPSAMPLE_NEAREST, J.UPSAMPLE_SMOOTH) if layout in SMOOTHED else (J.UPSAMPLE_NEAREST,):
            launches += run_windows(J, torch, ctx, data, d_co, info, scale, up)
    assert launches >= 4 * 8 * 7 * 2


def test_the_permutation_is_seen(J, torch, ctx):
    """a build whose oriented instances ignored their bits would pass nothing above -- unless P were symmetric: it is not"""
    for layout, W, H in FILES[:7]:
        info, d_co = ctx.read_jpeg_gpu(K.jpeg(layout, W, H))
        P = existing_picture(torch, ctx, d_co, info, 1, J.UPSAMPLE_NEAREST)
        for o in range(2, 9):
            O = OM.orient(P, o)
            assert O.shape != P.shape or not np.array_equal(O, P), (layout, o)
        for j in range(1, P.shape[0]):
            assert not np.array_equal(P[j], P[j - 1]), (layout, "rows", j)
        for i in range(1, P.shape[1]):
            assert not np.array_equal(P[:, i], P[:, i - 1]), (layout, "columns", i)


def test_gray(J, torch, ctx):
    data = K.jpeg("own", 33, 17)
    info, d_co = ctx.read_jpeg_gpu(data)
    for scale, up in ((1, J.UPSAMPLE_SMOOTH), (2, J.UPSAMPLE_NEAREST)):
        P = existing_picture(torch, ctx, d_co, info, scale, up, gray=True)
        for o in (3, 6):
            Wo, Ho = OM.size(o, P.shape[1], P.shape[0])
            out = [torch.full((Wo * Ho + 4,), FILL, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
            ctx.dequant_idct_region_dev(d_co, info, (0, 0, Wo, Ho), scale, *out, gray=True, upsampling=up, orientation=o)
            torch.cuda.synchronize()
            for c in range(3):
                got = out[c].cpu().numpy()
                assert np.array_equal(got[:-4].reshape(Ho, Wo), OM.orient(P, o)[:, :, c]) and (got[-4:] == FILL).all(), (scale, o, c)


# ---- 2. the device entries: frames, streams, capture ---------------------------------------------------------------------------------
def test_two_frames_in_one_call(J, torch, ctx):
    files = [K.jpeg("own", 33, 17, seed=70 + k, fixed_qt=True) for k in range(2)]
    parts = [ctx.read_jpeg_gpu(f) for f in files]
    d_co = torch.cat([p[1].reshape(-1) for p in parts])
    for scale, up in ((1, J.UPSAMPLE_NEAREST), (2, J.UPSAMPLE_SMOOTH)):
        run_windows(J, torch, ctx, None, d_co, parts[0][0], scale, up, orientations=(2, 5, 6, 7), frames=2)


def test_on_a_callers_stream(J, torch, ctx):
    data = K.jpeg("h2v1", 40, 24)
    info, d_co = ctx.read_jpeg_gpu(data)
    torch.cuda.synchronize()
    # the context's own stream, wrapped: a stream that is not the default one, and none taken from torch's pool -- the suite's stream
    # tests (tests/test_gpu_streams.py) run later in the same process and depend on which pool streams are still unused
    s = torch.cuda.ExternalStream(ctx.stream())
    with torch.cuda.stream(s):
        run_windows(J, torch, ctx, data, d_co, info, 1, J.UPSAMPLE_SMOOTH, orientations=(4, 8), stream=s)


def test_captured_and_replayed(J, torch, ctx):
    data = K.jpeg("own", 33, 17)
    info, d_co = ctx.read_jpeg_gpu(data)
    P = existing_picture(torch, ctx, d_co, info, 1, J.UPSAMPLE_SMOOTH)
    o, win = 6, (1, 3, 11, 20)                                        # of the 17 x 33 oriented picture
    x, y, w, h = win
    out = [torch.full((w * h + 4,), FILL, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    call = lambda st: ctx.dequant_idct_region_dev(d_co, info, win, 1, *out, upsampling=J.UPSAMPLE_SMOOTH, orientation=o, stream=st)
    call(torch.cuda.current_stream().cuda_stream)                    # the tables go up outside the capture
    torch.cuda.synchronize()
    s, g = torch.cuda.ExternalStream(ctx.stream()), torch.cuda.CUDAGraph()      # (no stream from torch's pool: see above)
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call(s.cuda_stream)
    for _ in range(2):
        for t in out:
            t.fill_(FILL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        for c in range(3):
            got = out[c].cpu().numpy()
            assert np.array_equal(got[:-4].reshape(h, w), OM.orient(P, o)[y:y + h, x:x + w, c]) and (got[-4:] == FILL).all()


# ---- 3. the file entries and the tag --------------------------------------------------------------------------------------------------
def test_file_entries_and_the_tag_source(J, torch, ctx):
    plain = K.jpeg("own", 33, 17)
    info, d_co = ctx.read_jpeg_gpu(plain)
    for scale, up in ((1, J.UPSAMPLE_NEAREST), (2, J.UPSAMPLE_SMOOTH), (8, J.UPSAMPLE_NEAREST)):
        P = existing_picture(torch, ctx, d_co, info, scale, up)
        for o in OM.ORIENTATIONS:
            data = OM.tagged(plain, OM.app1(value=o, order="MM" if o % 2 else "II", place="last"))
            O = OM.orient(P, o)
            Ho, Wo = O.shape[:2]
            # the file's own tag, the whole picture
            fi, r, g, b, size, used = ctx.decode_jpeg_oriented(data, J.ORIENT_FROM_FILE, scale=scale, upsampling=up)
            assert (fi.width, fi.height, size, used) == (33, 17, (Wo, Ho), o)
            assert np.array_equal(np.stack([r, g, b], axis=-1).reshape(Ho, Wo, 3), O), (scale, up, o)
            # ... equals the explicit call on the untagged file, and an explicit orientation overrides the tag
            _, img, used = ctx.decode_jpeg_oriented_packed(plain, o, scale=scale, upsampling=up, format=J.PIX_BGRA32)
            assert used == o and np.array_equal(img, K.interleave(J, J.PIX_BGRA32, [O[:, :, c] for c in range(3)]))
            other = 1 + o % 8
            _, img, used = ctx.decode_jpeg_oriented_packed(data, other, scale=scale, upsampling=up)
            assert used == other and np.array_equal(img, OM.orient(P, other))
            for name, win in windows(info, scale, o).items():
                if name not in ("corner_11", "four_mcu_corner_odd_origin", "left_edge_1_mod_4"):
                    continue
                x, y, w, h = win
                _, r, g, b, size, used = ctx.decode_jpeg_oriented(data, region=win, scale=scale, upsampling=up)
                assert size == (w, h) and used == o
                assert np.array_equal(np.stack([r, g, b], axis=-1).reshape(h, w, 3), O[y:y + h, x:x + w]), (scale, up, o, name)
    # a tag of 9 is no tag; Decoder.decode(orient=True) reads the file's
    nine = OM.tagged(plain, OM.app1(value=9))
    assert ctx.decode_jpeg_oriented(nine)[5] == 1
    with pytest.raises(J.JpezyError, match="lies outside the picture of 17 x 33"):
        ctx.decode_jpeg_oriented(plain, 6, region=(0, 0, 33, 17))


def test_decoder_class(J, torch, ctx, tmp_path):
    plain = K.jpeg("own", 33, 17)
    info, d_co = ctx.read_jpeg_gpu(plain)
    P = existing_picture(torch, ctx, d_co, info, 1, J.UPSAMPLE_NEAREST)
    path = tmp_path / "six.jpg"
    path.write_bytes(OM.tagged(plain, OM.app1(value=6)))
    d = J.Decoder(str(path), ctx=ctx)
    r, g, b = d.decode(orient=True)
    assert d.orientation == 6 and d.size == (17, 33) and (d.pr.width, d.pr.height) == (33, 17)
    assert np.array_equal(np.stack([r, g, b], axis=-1).reshape(33, 17, 3), OM.orient(P, 6))
    r, g, b = d.decode()                                              # the default is today's behaviour
    assert np.array_equal(np.stack([r, g, b], axis=-1).reshape(17, 33, 3), P)


# ---- 4. the window batches ------------------------------------------------------------------------------------------------------------
BATCH = [("own", 33, 17, 1), ("444", 9, 23, 6), ("own", 16, 16, 1), ("own", 40, 24, 3), ("444", 23, 31, 8), ("own", 24, 40, 5)]


def batch_files(extra=()):
    files = [OM.tagged(K.jpeg(l, w, h), OM.app1(value=o, order="II" if k % 2 else "MM")) if o != 1 or k else K.jpeg(l, w, h)
             for k, (l, w, h, o) in enumerate(BATCH)]
    return files + list(extra), [o for _, _, _, o in BATCH] + [1] * len(extra)


def oriented_sources(J, ctx, files, orients, wins, fmt=None):
    """per file: the window's pixels [h, w, 3 or 4] of orient(P, o), P the existing packed decode at the window's scale"""
    fmt = J.PIX_RGB24 if fmt is None else fmt
    out = []
    for f, o, (reg, scale) in zip(files, orients, wins):
        info = K.parsed(f)[0]
        Ws, Hs = M.scaled_size(info.width, info.height, scale)
        P = ctx.decode_jpeg_region_packed(f, (0, 0, Ws, Hs), scale=scale, format=fmt)[1]
        O = OM.orient(P, o)
        x, y, w, h = reg if reg[2] else (0, 0) + OM.size(o, Ws, Hs)
        assert O[y:y + h, x:x + w].shape[:2] == (h, w)
        out.append(np.ascontiguousarray(O[y:y + h, x:x + w]))
    return out


def own_windows(files, orients):
    """a window of its own size per file, in the oriented picture, scales 1 and 2 in turn; one whole-picture form"""
    wins = []
    for k, (f, o) in enumerate(zip(files, orients)):
        info = K.parsed(f)[0]
        scale = 1 + k % 2
        Wo, Ho = OM.size(o, *M.scaled_size(info.width, info.height, scale))
        wins.append(((0, 0, 0, 0), scale) if k == 3 else ((1, k % 3, Wo - 2 - k % 2, Ho - 1 - k % 3), scale))
    return wins


def run_batch(J, torch, ctx, files, orients, wins, setting=1):
    n = len(files)
    src = oriented_sources(J, ctx, files, orients if setting else [1] * n, wins)
    Hm, Wm = max(s.shape[0] for s in src), max(s.shape[1] for s in src)
    row, slot = Wm * 3 + 1, Hm * (Wm * 3 + 1) + 3
    buf = torch.full((n * slot + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    ctx.set_windows_orientation(setting)
    try:
        res = ctx.decode_windows_dev(files, buf.as_strided((n, Hm, Wm, 3), (slot, row, 3, 1)), wins)
    finally:
        ctx.set_windows_orientation(0)
    exp = np.full(n * slot + GUARD, FILL, np.uint8)
    for k, s in enumerate(src):
        assert res[k][2] == 0 and res[k][1][2:] == (s.shape[1], s.shape[0]), (k, res[k][1:])
        for j in range(s.shape[0]):
            exp[k * slot + j * row:k * slot + j * row + s.shape[1] * 3] = s[j].reshape(-1)
    got = buf.cpu().numpy()
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, ("first differing byte", int(bad[0]), "file", int(bad[0]) // slot, "count", bad.size)
    return res


def test_windows_batch_mixed_orientations(J, torch, ctx):
    files, orients = batch_files()
    wins = own_windows(files, orients)
    assert ctx.windows_orientation() == 0
    run_batch(J, torch, ctx, files, orients, wins)
    assert ctx.last_batch_fast_count() == len(files)                 # the grouped path: two layouts, un-oriented and oriented launches
    assert ctx.windows_orientation() == 0
    # the setting off: the tags are ignored, the same call gives the un-oriented windows
    plain_wins = own_windows(files, [1] * len(files))
    run_batch(J, torch, ctx, files, orients, plain_wins, setting=0)


def test_windows_batch_per_file_path_and_a_tag_of_nine(J, torch, ctx):
    flat = K.synth_jpeg(24, 40, K.LAYOUTS["own"], seed=3, density=0.0)[0]
    rst = K.jpeg("own", 40, 24, restart=2)
    nine = OM.tagged(K.jpeg("own", 33, 17), OM.app1(value=9))
    extra = [OM.tagged(flat, OM.app1(value=8)), OM.tagged(rst, OM.app1(value=7)), nine]
    files, orients = batch_files(extra)
    orients[-3:] = [8, 7, 1]
    wins = own_windows(files, orients)
    ctx.set_windows_slice_files(1)
    try:
        run_batch(J, torch, ctx, files, orients, wins)
        assert ctx.last_batch_fast_count() < len(files)              # the restart-interval file at least went file by file
    finally:
        ctx.set_windows_slice_files(0)


@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
def test_windows_resized_batch(J, torch, ctx, filt):
    files, orients = batch_files()
    wins = own_windows(files, orients)
    n, ow, oh = len(files), 13, 10
    mirror = [k % 2 for k in range(n)]
    fcode = {"bilinear": (J.FILTER_BILINEAR, FM.BILINEAR), "bicubic": (J.FILTER_BICUBIC, FM.BICUBIC)}[filt]
    buf = torch.full((n * oh * ow * 3 + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    ctx.set_windows_orientation(1)
    try:
        res = ctx.decode_windows_resized_dev(files, buf[:n * oh * ow * 3].view(n, oh, ow, 3), wins, mirror, filter=fcode[0])
    finally:
        ctx.set_windows_orientation(0)
    got = buf.cpu().numpy()
    assert (got[-GUARD:] == FILL).all()
    for k, s in enumerate(oriented_sources(J, ctx, files, orients, wins)):
        assert res[k][2] == 0
        want = FM.resize(s, ow, oh, fcode[1], bool(mirror[k]))         # the mirror acts after the orientation
        if filt == "bilinear":
            assert np.array_equal(want, RM.resize(s, ow, oh, bool(mirror[k])))
        assert np.array_equal(got[k * oh * ow * 3:(k + 1) * oh * ow * 3].reshape(oh, ow, 3), want), (filt, k)


def test_windows_tensor_batch_float16_channels_last(J, torch, ctx):
    files, orients = batch_files()
    wins = own_windows(files, orients)
    n, ow, oh = len(files), 12, 9
    mirror = [k % 2 for k in range(n)]
    scale, bias = TM.normalization(TM.IMAGENET_MEAN, TM.IMAGENET_STD)
    d_out = torch.zeros((n, 3, oh, ow), dtype=torch.float16, device="cuda:0").contiguous(memory_format=torch.channels_last)
    ctx.set_windows_orientation(1)
    try:
        res = ctx.decode_windows_tensor_dev(files, d_out, wins, mirror, scale, bias)
    finally:
        ctx.set_windows_orientation(0)
    got = d_out.cpu().numpy().view(np.uint16)                           # logical [n, C, H, W]
    for k, s in enumerate(oriented_sources(J, ctx, files, orients, wins)):
        assert res[k][2] == 0
        img = RM.resize(s, ow, oh, bool(mirror[k]))
        for c in range(3):
            assert np.array_equal(got[k, c], TM.elements(img[:, :, c], TM.DT_F16, scale[c], bias[c])), (k, c)


# ---- 5. the command-line tools ----------------------------------------------------------------------------------------------------------
def test_cli_decode_orient(J, torch, ctx, tmp_path):
    exe = Path(J.library_path()).parent / "bin" / "jpezy_decode"
    plain = K.jpeg("own", 33, 17)
    info, d_co = ctx.read_jpeg_gpu(plain)
    src = tmp_path / "in.jpg"
    src.write_bytes(OM.tagged(plain, OM.app1(value=6)))
    for args, scale, win in (([], 1, None), (["--scale=2"], 2, None), (["--region=8x9+3+5"], 1, (3, 5, 8, 9))):
        P = existing_picture(torch, ctx, d_co, info, scale, J.UPSAMPLE_NEAREST)
        O = OM.orient(P, 6)
        if win:
            O = O[win[1]:win[1] + win[3], win[0]:win[0] + win[2]]
        out = tmp_path / "out.ppm"
        r = subprocess.run([str(exe), str(src), str(out), "--orient", *args], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        tok = [t for line in out.read_text().splitlines() if not line.startswith("#") for t in line.split()]
        assert tok[:4] == ["P3", str(O.shape[1]), str(O.shape[0]), "255"], tok[:4]
        assert np.array_equal(np.array(tok[4:], dtype=np.int64).reshape(O.shape), O), args
        assert f"size = {O.shape[1]} x {O.shape[0]}" in r.stdout and "Loaded JPEG: 33x17" in r.stdout


def test_cli_tran_auto_orient(J, torch, ctx, tmp_path):
    exe = Path(J.library_path()).parent / "bin" / "jpezy_tran"
    enc = J.Context(0)
    try:
        rng = np.random.default_rng(9)
        W, H = 48, 32                                                 # whole MCUs: nothing to trim
        planes = [rng.integers(0, 256, W * H, dtype=np.uint8) for _ in range(3)]
        plain = enc.encode_jpeg(*planes, W, H)
    finally:
        enc.close()
    P = ctx.decode_jpeg_packed(plain)[1]
    for o in OM.ORIENTATIONS:
        src, out = tmp_path / f"in{o}.jpg", tmp_path / f"out{o}.jpg"
        src.write_bytes(OM.tagged(plain, OM.app1(value=o)))
        r = subprocess.run([str(exe), str(src), str(out), "--auto-orient"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        data = out.read_bytes()
        assert J.jpeg_orientation(data) == 1                           # upright and untagged
        assert np.array_equal(ctx.decode_jpeg_packed(data)[1], OM.orient(P, o)), o
