"""Lossless transforms on the GPU (include/jpezy_hip.h, LOSSLESS TRANSFORMS): the kernel of jpezy_kernels_transform.hip against the numpy
model (tests/transform_model.py), exactly; the group laws by chaining device calls; jpezy_transform_jpeg byte for byte against the host
writer fed by the model; pixels against the numpy image operation; the refusals; stream capture."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeg_synth
import transform_model as M

pytestmark = pytest.mark.gpu

E_BADARG, E_UNSUPPORTED, E_NOSPACE = -1, -4, -6
SENTINEL = 0x5A5A
GUARD = 4096                                                              # int16 elements behind the destination


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


def _bpm(sampling):
    return 3 if sampling == M.S444 else 6


def _fields(W, H, sampling, n_frames, kind):
    """[n_frames][mcu][block][64]: 'tag' marks every element with its source position, 'random' spans all of int16"""
    m = M.mcu_px(sampling)
    n = (-(-W // m)) * (-(-H // m)) * _bpm(sampling) * 64
    if kind == "tag":
        flat = ((np.arange(n_frames * n, dtype=np.int64) % 65536) - 32768).astype(np.int16)
    else:
        rng = np.random.default_rng(W * 131 + H * 7 + sampling)
        flat = rng.integers(-32768, 32768, n_frames * n, dtype=np.int64).astype(np.int16)
        flat[5::977] = -32768
    return flat.reshape(n_frames, -1, _bpm(sampling), 64)


def _run_kernel(J, ctx, co, W, H, sampling, op, trim):
    """the device call on co [n_frames][...] with a sentinel-filled destination and a guard behind it -> the output frames"""
    import torch
    n_frames = co.shape[0]
    Wo, Ho, _, _ = J.transform_geometry(op, W, H, sampling, trim)
    n_out = J.coeff_count(Wo, Ho, sampling=sampling)
    d_in = torch.from_numpy(co.reshape(-1).copy()).cuda()
    d_out = torch.full((n_frames * n_out + GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
    ctx.coeff_transform_dev(d_in, W, H, d_out, op, trim=trim, sampling=sampling, n_frames=n_frames)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[n_frames * n_out:] == SENTINEL).all(), "the guard behind the destination was written"
    assert np.array_equal(d_in.cpu().numpy(), co.reshape(-1)), "the source was written"
    return got[:n_frames * n_out].reshape(n_frames, -1, _bpm(sampling), 64), Wo, Ho


def _check_kernel(J, ctx, W, H, sampling, op, trim, n_frames, kind):
    co = _fields(W, H, sampling, n_frames, kind)
    got, Wo, Ho = _run_kernel(J, ctx, co, W, H, sampling, op, trim)
    for f in range(n_frames):
        want, wo, ho = M.transform_field(co[f], W, H, sampling, op, trim)
        assert (wo, ho) == (Wo, Ho)
        assert np.array_equal(got[f], want), (W, H, sampling, M.NAMES[op], trim, n_frames, kind, f)


GRIDS = [(1, 1), (1, 5), (5, 1), (3, 2), (7, 5), (33, 17)]               # MCU columns x rows; the last: 3366 / 1683 blocks, 106 / 53 workgroups, the final one ragged


@pytest.mark.parametrize("sampling", [M.S420, M.S444])
@pytest.mark.parametrize("op", range(8))
def test_kernel_against_the_model(J, ctx, op, sampling):
    m = M.mcu_px(sampling)
    for cols, rows in GRIDS:
        for n_frames in (1, 3):
            for kind in ("tag", "random"):
                _check_kernel(J, ctx, cols * m, rows * m, sampling, op, False, n_frames, kind)


@pytest.mark.parametrize("sampling,size,trimmed", [(M.S420, (40, 24), (32, 16)), (M.S444, (13, 9), (8, 8))])
def test_kernel_trims_a_partial_mcu(J, ctx, sampling, size, trimmed):
    """a partial MCU on each axis: with trim every operation runs and the mirrored axes shrink; TRANSPOSE and NONE run without"""
    W, H = size
    for op in range(8):
        swap, mx, my = M.OPS[op]
        for kind in ("tag", "random"):
            _check_kernel(J, ctx, W, H, sampling, op, True, 2, kind)
        wt, ht = (trimmed[0] if mx else W), (trimmed[1] if my else H)
        assert J.transform_geometry(op, W, H, sampling, True)[:2] == ((ht, wt) if swap else (wt, ht))
    for op in (M.TRANSPOSE, M.NONE):
        for kind in ("tag", "random"):
            _check_kernel(J, ctx, W, H, sampling, op, False, 2, kind)


@pytest.mark.parametrize("sampling,size", [(M.S420, (48, 32)), (M.S444, (24, 40))])
def test_group_laws_on_the_device(J, ctx, sampling, size):
    import torch
    W, H = size
    co = _fields(W, H, sampling, 1, "random")
    n = co.size

    def chain(ops):
        cur, w, h = torch.from_numpy(co.reshape(-1).copy()).cuda(), W, H
        for op in ops:
            nxt = torch.full((n,), SENTINEL, dtype=torch.int16, device="cuda")
            ctx.coeff_transform_dev(cur, w, h, nxt, op, sampling=sampling)
            w, h = J.transform_geometry(op, w, h, sampling)[:2]
            cur = nxt
        torch.cuda.synchronize()
        return cur.cpu().numpy(), w, h

    def same(a, b):
        return a[1:] == b[1:] and np.array_equal(a[0], b[0])

    none = chain([M.NONE])
    assert np.array_equal(none[0], co.reshape(-1)) and none[1:] == (W, H)
    assert same(chain([M.HFLIP, M.HFLIP]), none)
    assert same(chain([M.ROT90] * 4), none)
    assert same(chain([M.ROT90]), chain([M.TRANSPOSE, M.HFLIP]))
    assert same(chain([M.TRANSVERSE]), chain([M.TRANSPOSE, M.ROT180]))
    assert not same(chain([M.ROT90]), chain([M.ROT270]))


def test_coeff_transform_dev_under_stream_capture(J, ctx):
    import torch
    W, H, sampling, op = 80, 48, M.S420, M.ROT90
    fields = [_fields(W, H, sampling, 2, kind) for kind in ("tag", "random")]
    d_in = torch.from_numpy(fields[0].reshape(-1).copy()).cuda()
    d_out = torch.full((fields[0].size + GUARD,), SENTINEL, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ctx.coeff_transform_dev(d_in, W, H, d_out, op, sampling=sampling, n_frames=2, stream=s.cuda_stream)
    for turn in range(2):                                                 # replayed twice, on different coefficients
        d_in.copy_(torch.from_numpy(fields[turn].reshape(-1).copy()).cuda())
        d_out.fill_(SENTINEL)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert (got[fields[0].size:] == SENTINEL).all()
        for f in range(2):
            want, _, _ = M.transform_field(fields[turn][f], W, H, sampling, op)
            assert np.array_equal(got[f * want.size:(f + 1) * want.size], want.reshape(-1)), (turn, f)


# ---- files ----
def _pil_file(W, H, subsampling, seed=5):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(xx * 5 + yy * 3) % 256, (xx * yy) % 256, rng.integers(0, 256, (H, W))], axis=-1).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=90, optimize=True, subsampling=subsampling)
    return buf.getvalue()


L420 = [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]


def _source(J, ctx, oracle, name):
    if name == "own420":
        return ctx.encode_jpeg(*oracle.synth_rgb(48, 32, frame=3), 48, 32)
    if name == "own444":
        return ctx.encode_jpeg(*oracle.synth_rgb(40, 24, frame=4), 40, 24, sampling=J.SAMPLING_444)
    if name == "synth_rst":
        return jpeg_synth.synth_jpeg(48, 32, L420, seed=21, qmax=200, restart=4)[0]
    if name == "synth_tq000":
        return jpeg_synth.synth_jpeg(48, 32, [(2, 2, 0, 0), (1, 1, 0, 1), (1, 1, 0, 1)], seed=22, qmax=200)[0]
    if name == "pil420":
        return _pil_file(48, 32, 2)
    if name == "pil444":
        return _pil_file(48, 32, 0)
    raise KeyError(name)


def _expected(J, data, op, optimize, restart, comment=None):
    """the host writer fed by the model: (bytes, model coefficients, Wout, Hout, sampling, (luma', chroma'))"""
    info, co = J.read_jpeg(data)
    sampling = M.S444 if info.H[0] == 1 else M.S420
    out, Wo, Ho = M.transform_field(co.reshape(-1, _bpm(sampling), 64), info.width, info.height, sampling, op)
    tabs = tuple(M.quant_table(op, np.array(info.qt[info.Tq[k]][:])).astype(np.uint8) for k in (0, 1))
    text = info.comment if comment is None else comment
    want = J.write_jpeg(out, Wo, Ho, comment=bytes(text), optimize=optimize, restart_interval=restart, quant_tables=tabs, sampling=sampling)
    return want, out, Wo, Ho, sampling, tabs


@pytest.mark.parametrize("name", ["own420", "own444", "synth_rst", "synth_tq000", "pil420", "pil444"])
def test_files_byte_for_byte(J, ctx, oracle, name):
    from PIL import Image
    data = _source(J, ctx, oracle, name)
    src_info, _ = J.read_jpeg(data)
    if name == "synth_tq000":
        assert list(src_info.Tq) == [0, 0, 0]
    if name.startswith("synth"):                                          # random tables: asymmetric, so a table that was not transposed shows
        t = np.array(src_info.qt[0][:]).reshape(8, 8)
        assert not np.array_equal(t, t.T)
    try:
        for optimize, restart in ((False, 0), (True, 0), (False, 5), (True, 5)):
            ctx.set_huffman_optimize(optimize)
            ctx.set_restart_interval(restart)
            for op in range(8):
                want, co, Wo, Ho, sampling, tabs = _expected(J, data, op, optimize, restart)
                got, info = ctx.transform_jpeg(data, op)
                assert got == want, (name, M.NAMES[op], optimize, restart, len(got), len(want))
                assert (info.width, info.height, info.restart_interval) == (Wo, Ho, restart)
                if optimize or restart:
                    continue
                back, bco = J.read_jpeg(got)                              # what a reader sees: the model's coefficients, size and tables
                assert (back.width, back.height) == (Wo, Ho) and np.array_equal(bco.reshape(co.shape), co)
                assert list(back.Tq) == [0, 1, 1] and list(back.H) == list(src_info.H) and list(back.V) == list(src_info.V)
                for k in (0, 1):
                    assert np.array_equal(np.array(back.qt[k][:]), tabs[k]) and np.array_equal(np.array(info.qt[k][:]), tabs[k])
                assert bytes(back.comment) == bytes(src_info.comment) == bytes(info.comment)
                assert Image.open(io.BytesIO(got)).size == (Wo, Ho)
    finally:
        ctx.set_huffman_optimize(False)
        ctx.set_restart_interval(0)


def test_files_through_the_gpu_huffman_decoder(J, ctx, oracle):
    """set_huffdec_min_bytes(0): the GPU Huffman decoder, not the host's, feeds the kernel"""
    data = ctx.encode_jpeg(*oracle.synth_rgb(208, 128, frame=3), 208, 128)
    ctx.set_huffdec_min_bytes(0)
    try:
        for op in range(8):
            got, _ = ctx.transform_jpeg(data, op)
            assert ctx.last_huffdec_passes() > 0
            assert got == _expected(J, data, op, False, 0)[0], M.NAMES[op]
    finally:
        ctx.set_huffdec_min_bytes(32 << 10)


def test_comment_argument(J, ctx, oracle):
    data = _source(J, ctx, oracle, "own420")
    assert bytes(J.read_jpeg(data)[0].comment) == b"Encoded by jpezy"
    for comment in (b"", b"turned"):
        got, info = ctx.transform_jpeg(data, M.ROT90, comment=comment)
        assert got == _expected(J, data, M.ROT90, False, 0, comment=comment)[0]
        assert bytes(info.comment) == comment == bytes(J.read_jpeg(got)[0].comment)


@pytest.mark.parametrize("name", ["own420", "own444", "synth_rst", "synth_tq000"])
def test_none_with_optimise_is_lossless_recompression(J, ctx, oracle, name):
    data = _source(J, ctx, oracle, name)
    info, co = J.read_jpeg(data)
    sampling = M.S444 if info.H[0] == 1 else M.S420
    tabs = tuple(np.array(info.qt[info.Tq[k]][:]).astype(np.uint8) for k in (0, 1))
    plain = J.write_jpeg(co, info.width, info.height, comment=bytes(info.comment), quant_tables=tabs, sampling=sampling)
    ctx.set_huffman_optimize(True)
    try:
        got, _ = ctx.transform_jpeg(data, M.NONE)
    finally:
        ctx.set_huffman_optimize(False)
    assert len(got) <= len(plain), (len(got), len(plain))
    assert np.array_equal(J.read_jpeg(got)[1], co)


@pytest.mark.parametrize("size", [(48, 32), (64, 64), (16, 80)])
@pytest.mark.parametrize("seed", [0, 1])
def test_pixels_are_the_image_operation(J, ctx, oracle, seed, size):
    """exact on these inputs (the CPU oracle alone gives zero differing samples on them); not guaranteed in general: the reference's
    IDCT sums in a different order after a flip"""
    W, H = size
    data = ctx.encode_jpeg(*oracle.synth_rgb(W, H, frame=seed), W, H)
    _, r, g, b = ctx.decode_jpeg(data)
    img = np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1)
    for op in range(1, 8):
        got, info = ctx.transform_jpeg(data, op)
        dinfo, r2, g2, b2 = ctx.decode_jpeg(got)
        want = M.pixel_op(img, op)
        assert (dinfo.width, dinfo.height) == (want.shape[1], want.shape[0]) == (info.width, info.height)
        back = np.stack([p.reshape(dinfo.height, dinfo.width) for p in (r2, g2, b2)], axis=-1)
        assert np.array_equal(back, want), (M.NAMES[op], int((back != want).sum()))


def test_refusals_leave_the_context_usable(J, ctx, oracle):
    rng = np.random.default_rng(9)
    good = _source(J, ctx, oracle, "own420")
    three = rng.integers(1, 200, (3, 64))
    partial = ctx.encode_jpeg(*oracle.synth_rgb(40, 24, frame=1), 40, 24)
    cases = [
        ("one component", jpeg_synth.synth_jpeg(32, 32, [(1, 1, 0, 0)], seed=1)[0], M.ROT90, "component"),
        ("4:2:2", _pil_file(48, 32, 1), M.ROT90, "2x1"),
        ("16-bit DQT", jpeg_synth.synth_jpeg(48, 32, L420, seed=2, qt_precision=[1, 1])[0], M.ROT90, "16-bit DQT"),
        ("precision 12", jpeg_synth.synth_jpeg(48, 32, L420, seed=3, precision=12)[0], M.ROT90, "precision 12"),
        ("Cb / Cr tables", jpeg_synth.synth_jpeg(48, 32, [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 2, 1)], seed=4, qt=three)[0], M.ROT90, "Cb and Cr"),
        ("partial MCU", partial, M.HFLIP, "width"),
        ("partial MCU", partial, M.VFLIP, "height"),
    ]
    for what, data, op, named in cases:
        with pytest.raises(J.JpezyError) as e:
            ctx.transform_jpeg(data, op)
        assert f"status {E_UNSUPPORTED}:" in str(e.value) and named in str(e.value), (what, str(e.value))
        got, _ = ctx.transform_jpeg(good, M.ROT180)                       # the same context then transforms a good file
        assert got == _expected(J, good, M.ROT180, False, 0)[0], what
    # the partial file goes through with trim, and TRANSPOSE needs none
    for op, trim in ((M.HFLIP, True), (M.ROT180, True), (M.TRANSPOSE, False)):
        info, co = J.read_jpeg(partial)
        out, Wo, Ho = M.transform_field(co.reshape(-1, 6, 64), 40, 24, M.S420, op, trim)
        tabs = tuple(M.quant_table(op, np.array(info.qt[k][:])).astype(np.uint8) for k in (0, 1))
        got, oinfo = ctx.transform_jpeg(partial, op, trim=trim)
        assert got == J.write_jpeg(out, Wo, Ho, comment=bytes(info.comment), quant_tables=tabs) and (oinfo.width, oinfo.height) == (Wo, Ho)


def test_a_cap_one_byte_short_is_nospace(J, ctx, oracle):
    lib = J.load_library()
    data = _source(J, ctx, oracle, "own420")
    want = _expected(J, data, M.ROT90, False, 0)[0]
    arr = np.frombuffer(data, dtype=np.uint8)
    info = J.FrameInfo()
    buf = np.full(len(want) + 64, 0xA5, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.jpezy_transform_jpeg(ctx._h, p(arr), arr.size, M.ROT90, 0, None, C.byref(info), p(buf), len(want) - 1) == E_NOSPACE
    assert (buf[len(want) - 1:] == 0xA5).all(), "written past cap"
    assert lib.jpezy_transform_jpeg(ctx._h, p(arr), arr.size, M.ROT90, 0, None, C.byref(info), p(buf), len(want)) == len(want)
    assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xA5).all()
    assert lib.jpezy_transform_jpeg(ctx._h, p(arr), arr.size, M.ROT90, 0, None, C.byref(info), None, 0) == 0      # header and geometry only
    assert (info.width, info.height) == (32, 48)
