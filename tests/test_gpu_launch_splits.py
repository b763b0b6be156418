"""Batches that the entry points must cut into several launches or passes (include/jpezy_hip.h, frame counts): the frame index is
a grid dimension, so every batch entry point splits at 65535 frames, and the GPU Huffman writer also splits at 1 GiB of
worst-case stream.  Every frame has its own content, so a misplaced offset at a split changes bytes; every assertion names the
frame.  The seams: f0 = 65535 (and 2 * 65535) for the grid limit, f0 = `per` for the worst-case rule."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPLIT = 65535                    # frames per launch (grid.y / grid.z)
N1 = SPLIT + 2                   # 65537: one full launch + 2 frames
N2 = 2 * SPLIT + 3               # three launches
FORMAT, NOSPACE = -5, -6


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


def _sample(n, seams, k=24, seed=0):
    rng = np.random.default_rng(seed + n)
    s = {0, n - 1}
    for f0 in seams:
        s |= {f0 - 1, f0, f0 + 1}
    s |= set(int(x) for x in rng.integers(0, n, k))
    return sorted(f for f in s if 0 <= f < n)


def _planes(n, W, H, seed):
    """n frames of random planes with the frame index stamped into the first pixels (distinct even where noise repeats)"""
    rng = np.random.default_rng(seed)
    pl = rng.integers(0, 256, (3, n, W * H), dtype=np.uint8)
    idx = np.arange(n)
    for q in range(3):
        pl[q, :, 0] = idx & 0xFF
        pl[q, :, 1 % (W * H)] = (idx >> 8) & 0xFF
    return pl


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_tall_frame_equals_frames_in_order(oracle):
    """the oracle of n 16x16 frames in one call: a 16 x 16n frame has no edge clamp, so its MCUs are the frames' in order"""
    pl = _planes(5, 16, 16, 1)
    for gray in (False, True):
        tall = oracle.encode_coeffs(pl[0].reshape(-1), pl[1].reshape(-1), pl[2].reshape(-1), 16, 16 * 5, gray).reshape(5, -1)
        for f in range(5):
            one = oracle.encode_coeffs(pl[0, f], pl[1, f], pl[2, f], 16, 16, gray).reshape(-1)
            assert np.array_equal(tall[f], one), (gray, f)
        co = tall.reshape(5, -1)
        info = oracle.make_info(16, 16 * 5)
        dec = oracle.decode_planes(co.reshape(-1) if not gray else _to6(co, 5).reshape(-1), info, gray)
        for f in range(5):
            one = oracle.decode_planes(co[f] if not gray else _to6(co[f:f + 1], 1).reshape(-1), oracle.make_info(16, 16), gray)
            for q in range(3):
                assert np.array_equal(dec[q][f * 256:(f + 1) * 256], one[q]), (gray, f, q)


def _to6(co4, n):
    """gray coefficients (4 blocks per MCU) in the decoder's 6-block layout (zero chroma)"""
    co = np.zeros((n, 6, 64), np.int16)
    co[:, :4] = co4.reshape(n, 4, 64)
    return co


@pytest.mark.parametrize("n", [N1, N2])
def test_fdct_quant_dev_across_launch_splits(J, ctx, oracle, n):
    import torch
    W = H = 16
    pl = _planes(n, W, H, 7 + n)
    d = [_dev(pl[q].reshape(-1)) for q in range(3)]
    for gray in (False, True):
        want = oracle.encode_coeffs(pl[0].reshape(-1), pl[1].reshape(-1), pl[2].reshape(-1), W, H * n, gray).reshape(n, -1)
        for variant in (0, 1):
            ctx.set_variant(variant)
            out = torch.full((n * want.shape[1],), -32768, dtype=torch.int16, device="cuda")
            ctx.fdct_quant_dev(d[0], d[1], d[2], W, H, out, gray=gray, n_frames=n)
            torch.cuda.synchronize()
            got = out.cpu().numpy().reshape(n, -1)
            bad = np.flatnonzero((got != want).any(axis=1))
            assert bad.size == 0, f"gray={gray} variant={variant}: frames {bad[:8].tolist()} differ (first of {bad.size})"
    ctx.set_variant(1)


def test_fdct_quant_dev_ragged_frames_across_the_split(J, ctx, oracle):
    """9x7 frames (edge clamp in both directions), 65536 of them: sampled frames around the seam and at random"""
    import torch
    W, H, n = 9, 7, SPLIT + 1
    pl = _planes(n, W, H, 9)
    d = [_dev(pl[q].reshape(-1)) for q in range(3)]
    for gray in (False, True):
        cpf = J.coeff_count(W, H, gray)
        for variant in (0, 1):
            ctx.set_variant(variant)
            out = torch.full((n * cpf,), -32768, dtype=torch.int16, device="cuda")
            ctx.fdct_quant_dev(d[0], d[1], d[2], W, H, out, gray=gray, n_frames=n)
            torch.cuda.synchronize()
            got = out.cpu().numpy().reshape(n, -1)
            for f in _sample(n, [SPLIT]):
                want = oracle.encode_coeffs(pl[0, f], pl[1, f], pl[2, f], W, H, gray).reshape(-1)
                assert np.array_equal(got[f], want), f"gray={gray} variant={variant} frame {f}"
    ctx.set_variant(1)


def test_host_fdct_quant_one_chunk_over_the_split(J, oracle):
    """the host entry with a chunk size that puts all 65537 frames into one chunk of the pipeline: the device entry it calls
    must split that chunk"""
    W = H = 16
    n = N1
    pl = _planes(n, W, H, 11)
    c = J.Context(0)
    try:
        c.set_host_chunk_bytes(64 << 20)                        # 87381 frames of 16x16 per chunk
        got = c.fdct_quant(pl[0].reshape(-1), pl[1].reshape(-1), pl[2].reshape(-1), W, H, n_frames=n).reshape(n, -1)
    finally:
        c.close()
    want = oracle.encode_coeffs(pl[0].reshape(-1), pl[1].reshape(-1), pl[2].reshape(-1), W, H * n).reshape(n, -1)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"frames {bad[:8].tolist()} differ (first of {bad.size})"


def _oracle_coeffs(oracle, n, seed):
    pl = _planes(n, 16, 16, seed)
    return oracle.encode_coeffs(pl[0].reshape(-1), pl[1].reshape(-1), pl[2].reshape(-1), 16, 16 * n).reshape(n, -1)


def test_dequant_idct_dev_across_launch_split(J, ctx, oracle):
    import torch
    n, W, H = N1, 16, 16
    co = _oracle_coeffs(oracle, n, 13)
    d_co = _dev(co.reshape(-1))
    rng = np.random.default_rng(3)
    qtab = type(J.api.annex_k_tables().qt)()
    qrand = rng.integers(1, 40, (4, 64))
    for t in range(4):
        for i in range(64):
            qtab[t][i] = int(qrand[t, i])
    cases = [("annex-k", None, (0, 1, 1), 0), ("tables 2/3", qtab, (2, 3, 3), 0), ("tolerance", None, (0, 1, 1), 1)]
    for name, qt, tq, tol in cases:
        info = oracle.make_info(W, H * n)
        if qt is not None:
            for t in range(4):
                for i in range(64):
                    info.qt[t][i] = qt[t][i]
            for c in range(3):
                info.Tq[c] = tq[c]
        ctx.set_decode_tolerance(tol)
        for gray in (False, True):
            want = oracle.decode_planes(co.reshape(-1), info, gray)
            out = [torch.zeros(n * W * H, dtype=torch.uint8, device="cuda") for _ in range(3)]
            ctx.dequant_idct_dev(d_co, W, H, out[0], out[1], out[2], qt=qt, comp_tq=tq, gray=gray, n_frames=n)
            torch.cuda.synchronize()
            for q in range(3):
                got = out[q].cpu().numpy().astype(np.int16).reshape(n, -1)
                diff = np.abs(got - want[q].astype(np.int16).reshape(n, -1)).max(axis=1)
                bad = np.flatnonzero(diff > (1 if tol else 0))
                assert bad.size == 0, f"{name} gray={gray} plane {q}: frames {bad[:8].tolist()} differ (first of {bad.size})"
    ctx.set_decode_tolerance(0)


def test_generic_batch_decode_across_launch_split(J, ctx, oracle):
    """jpezy_dequant_idct_generic_batch_dev above 65535 frames: a 4:4:4 layout of 8x8 frames, planes a padded stride apart"""
    import torch
    from jpeg_synth import synth_jpeg
    n = N1
    data, co1, _ = synth_jpeg(8, 8, [(1, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)], seed=5)
    info, _ = J.read_jpeg(data)
    oinfo, _ = oracle.read_jpeg(data)
    assert (info.ncomp, info.blocks_per_mcu, info.mcu_cols, info.mcu_rows) == (3, 3, 1, 1)
    rng = np.random.default_rng(17)
    co = np.zeros((n, 3, 64), np.int16)
    mask = rng.random(co.shape) < 0.2
    co[mask] = rng.integers(-30, 31, int(mask.sum()))
    co[:, :, 0] = rng.integers(-60, 61, (n, 3))
    co[:, 0, 1] = (np.arange(n) % 61) - 30                   # frame stamp
    stride = 64 + 12                                         # > W * H, a multiple of 4
    d_co = _dev(co.reshape(-1))
    tall = oracle.FrameInfo()
    C.memmove(C.byref(tall), C.byref(oinfo), C.sizeof(oinfo))
    tall.height, tall.mcu_rows = 8 * n, n
    for gray in (False, True):
        want = oracle.decode_planes(co.reshape(-1), tall, gray)
        pl = [torch.full((n * stride,), 0x5A, dtype=torch.uint8, device="cuda") for _ in range(3)]
        ctx.dequant_idct_generic_dev(d_co, info, pl[0], pl[1], pl[2], gray=gray, n_frames=n, plane_stride=stride)
        torch.cuda.synchronize()
        for q in range(3):
            got = pl[q].cpu().numpy().reshape(n, stride)
            bad = np.flatnonzero((got[:, :64] != want[q].reshape(n, 64)).any(axis=1))
            assert bad.size == 0, f"gray={gray} plane {q}: frames {bad[:8].tolist()} differ (first of {bad.size})"
            assert (got[:, 64:] == 0x5A).all(), f"gray={gray} plane {q}: bytes between the planes were written"


# ---- the entries of the other pixel kinds: their own frame advances across the seam ----
_SHARED = {}


def _shared_coeffs(oracle):
    """the coefficients of N1 16x16 frames for the fused decode cases: computed once, read-only"""
    if "co" not in _SHARED:
        co = _oracle_coeffs(oracle, N1, 29)
        d_co = _dev(co.reshape(-1))
        co.setflags(write=False)
        _SHARED["co"] = (co, d_co)
    return _SHARED["co"]


def _packed(pl, n, W, H, format):
    """_planes as an (n, H, W, C) picture of the format: the frame stride is the tensor's"""
    nb, blue_first = (3, False) if format == 0 else (4, True)
    img = np.full((n, H * W, nb), 0xFF, np.uint8)
    for q in range(3):
        img[:, :, 2 - q if blue_first else q] = pl[q]
    return img.reshape(n, H, W, nb)


def _rows(t, n, frames):
    """frames `frames` of a device tensor of n frames, on the host"""
    import torch
    return t.view(n, -1)[torch.as_tensor(frames, device=t.device)].cpu().numpy()


def _encode_case(J, ctx, oracle, case):
    """-> (variants, W, H, launch(out), want(f)) of one encode entry over n = N1 frames of one MCU"""
    import sampling422_model as S422
    import sampling_model as S444
    import ycc_model as YM
    n = N1
    kind, _, sub = case.partition("-")
    if kind == "packed":
        W = H = 16
        fmt = {"rgb24": J.api.PIX_RGB24, "bgra32": J.api.PIX_BGRA32}[sub]
        pl = _planes(n, W, H, 31)
        d_img = _dev(_packed(pl, n, W, H, fmt))
        return ((0, 1), (False, True), J.coeff_count, W, H,
                lambda out, gray: ctx.fdct_quant_packed_dev(d_img, out, format=fmt, gray=gray),
                lambda f, gray: oracle.encode_coeffs(pl[0, f], pl[1, f], pl[2, f], W, H, gray))
    if kind == "ycc":
        W = H = 16
        pl = _planes(n, W, H, 37)
        y, cb, cr = pl[0].reshape(n, 16, 16), pl[1][:, :64].reshape(n, 8, 8), pl[2][:, :64].reshape(n, 8, 8)
        d_y = _dev(y)
        if sub == "planes":
            d_cb, d_cr = _dev(cb), _dev(cr)
        else:                                                    # one interleaved chroma plane: Cb and Cr neighbours, c_step 2
            d_uv = _dev(np.stack([cb, cr], axis=-1))
            d_cb, d_cr = d_uv[..., 0], d_uv[..., 1]
        return ((0, 1), (False, True), J.coeff_count, W, H,
                lambda out, gray: ctx.fdct_quant_ycc_dev(d_y, d_cb, d_cr, out, gray=gray),
                lambda f, gray: YM.encode_coeffs(y[f], cb[f], cr[f], gray))
    sampling, model, (W, H) = {"444": (J.api.SAMPLING_444, S444, (8, 8)), "422": (J.api.SAMPLING_422, S422, (16, 8))}[kind]
    luma, chroma = ctx.quant_tables()
    pl = _planes(n, W, H, 41 + W)
    count = lambda W, H, gray: J.coeff_count(W, H, sampling=sampling)
    want = lambda f, gray: model.encode_coeffs(pl[0, f], pl[1, f], pl[2, f], W, H, luma, chroma)
    if sub == "planes":
        d = [_dev(pl[q].reshape(-1)) for q in range(3)]
        return ((1,), (False,), count, W, H, lambda out, gray: ctx.fdct_quant_dev(d[0], d[1], d[2], W, H, out, n_frames=n, sampling=sampling), want)
    d_img = _dev(_packed(pl, n, W, H, J.api.PIX_RGB24))
    return ((1,), (False,), count, W, H, lambda out, gray: ctx.fdct_quant_packed_dev(d_img, out, sampling=sampling), want)


def _decode_case(J, ctx, oracle, case, frames):
    """runs one fused decode entry over N1 16x16 frames and compares the sampled frames"""
    import torch
    import ycc_model as YM
    n, W, H = N1, 16, 16
    co, d_co = _shared_coeffs(oracle)
    info = oracle.make_info(W, H)
    kind, _, sub = case.partition("-")
    if kind == "decode_packed":
        fmt = {"rgb24": J.api.PIX_RGB24, "bgra32": J.api.PIX_BGRA32}[sub]
        nb = J.api.pixel_bytes(fmt)
        for gray in (False, True):
            d_img = torch.zeros((n, H, W, nb), dtype=torch.uint8, device="cuda")
            ctx.dequant_idct_packed_dev(d_co, d_img, format=fmt, gray=gray)
            torch.cuda.synchronize()
            got = _rows(d_img, n, frames).reshape(len(frames), H * W, nb)
            for i, f in enumerate(frames):
                want = _packed(np.stack(oracle.decode_planes(co[f], info, gray))[:, None, :], 1, W, H, fmt).reshape(H * W, nb)
                assert np.array_equal(got[i], want), f"{case} gray={gray} frame {f}"
        return
    for luma_only in (False, True):
        d_y = torch.zeros((n, H, W), dtype=torch.uint8, device="cuda")
        d_uv = torch.zeros((n, 2, H // 2, W // 2) if sub == "planes" else (n, H // 2, W // 2, 2), dtype=torch.uint8, device="cuda")
        d_cb, d_cr = (d_uv[:, 0], d_uv[:, 1]) if sub == "planes" else (d_uv[..., 0], d_uv[..., 1])
        ctx.dequant_idct_ycc_dev(d_co, d_y, None if luma_only else d_cb, None if luma_only else d_cr)
        torch.cuda.synchronize()
        got = [_rows(t.contiguous(), n, frames) for t in (d_y, d_cb, d_cr)]
        for i, f in enumerate(frames):
            want = YM.decode_planes(co[f], info)
            for q in range(1 if luma_only else 3):
                assert np.array_equal(got[q][i], want[q].reshape(-1)), f"{case} luma_only={luma_only} component {q} frame {f}"
            if luma_only:
                assert not got[1][i].any() and not got[2][i].any(), f"{case}: chroma of frame {f} written by a luma-only call"


@pytest.mark.parametrize("case", ["packed-rgb24", "packed-bgra32", "ycc-planes", "ycc-interleaved", "444-planes", "444-packed", "422-planes",
                                  "422-packed", "decode_packed-rgb24", "decode_packed-bgra32", "decode_ycc-planes", "decode_ycc-interleaved"])
def test_other_pixel_kinds_across_the_launch_split(J, ctx, oracle, case):
    """65537 frames of one MCU through the entries whose frame advances are not the planar 4:2:0 ones': the packed buffer's frame stride,
    the two strides of the YCbCr planes, the coefficients per frame of 4:4:4 and 4:2:2, and the fused decoder's packed and native-sample
    outputs.  Expected values: the oracle and the CPU models, for the frames around the seam and a random sample"""
    import torch
    n = N1
    frames = _sample(n, [SPLIT])
    if case.startswith("decode"):
        _decode_case(J, ctx, oracle, case, frames)
        return
    variants, grays, count, W, H, launch, want = _encode_case(J, ctx, oracle, case)
    try:
        for gray in grays:
            cpf = count(W, H, gray)
            expect = {f: np.asarray(want(f, gray)).reshape(-1) for f in frames}
            for variant in variants:
                ctx.set_variant(variant)
                out = torch.full((n * cpf,), -32768, dtype=torch.int16, device="cuda")
                launch(out, gray)
                torch.cuda.synchronize()
                got = _rows(out, n, frames)
                for i, f in enumerate(frames):
                    assert np.array_equal(got[i], expect[f]), f"{case} gray={gray} variant={variant} frame {f}"
    finally:
        ctx.set_variant(1)


# ---- the GPU Huffman writer ----
def _host_batch(J, co, W, H, n, gray=False, cap=None, comment=b"Encoded by jpezy"):
    """jpezy_write_jpeg_batch with a caller-chosen cap (the Python wrapper reserves jpezy_jpeg_bound per frame)"""
    lib = J.load_library()
    cap = cap or lib.jpezy_jpeg_bound(W, H)
    co = np.ascontiguousarray(co, dtype=np.int16)
    buf = np.empty(cap * n, np.uint8)
    sizes = (C.c_long * n)()
    rc = lib.jpezy_write_jpeg_batch(co.ctypes.data_as(C.c_void_p), W, H, int(gray), n, comment, buf.ctypes.data_as(C.c_void_p),
                                    cap, sizes, 0)
    return rc, buf, np.ctypeslib.as_array(sizes).copy(), cap


def _gpu_batch(J, ctx, d_co, W, H, n, cap, gray=False, comment=b"Encoded by jpezy"):
    lib = J.load_library()
    buf = np.empty(cap * n, np.uint8)
    sizes = (C.c_long * n)()
    rc = lib.jpezy_write_jpeg_gpu_batch(ctx._h, d_co.data_ptr(), W, H, int(gray), n, comment, buf.ctypes.data_as(C.c_void_p),
                                        cap, sizes)
    return rc, buf, np.ctypeslib.as_array(sizes).copy()


def _gpu_dev(ctx, d_co, W, H, n, stride, gray=False, comment=b"Encoded by jpezy"):
    import torch
    d_out = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
    d_sz = torch.zeros(n, dtype=torch.int64, device="cuda")
    ctx.write_jpeg_gpu_dev(d_co, W, H, d_out, d_sz, gray=gray, comment=comment, n_frames=n)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().reshape(-1), d_sz.cpu().numpy()


def _files_equal(buf_a, cap_a, sz_a, buf_b, cap_b, sz_b, frames, what):
    for f in frames:
        assert sz_a[f] == sz_b[f], f"{what}: frame {f} size {sz_a[f]} != {sz_b[f]}"
        if sz_a[f] > 0:
            a = buf_a[f * cap_a: f * cap_a + sz_a[f]]
            b = buf_b[f * cap_b: f * cap_b + sz_b[f]]
            assert np.array_equal(a, b), f"{what}: frame {f} bytes differ"


def _all_files_equal(buf_a, cap_a, sz_a, buf_b, cap_b, sz_b, n, what):
    bad = np.flatnonzero(np.asarray(sz_a) != np.asarray(sz_b))
    assert bad.size == 0, f"{what}: sizes of frames {bad[:8].tolist()} differ"
    smax = int(max(sz_a.max(), 0))
    a = buf_a.reshape(n, cap_a)[:, :smax].copy()
    b = buf_b.reshape(n, cap_b)[:, :smax].copy()
    cols = np.arange(smax)[None, :]
    a[cols >= np.asarray(sz_a)[:, None]] = 0
    b[cols >= np.asarray(sz_b)[:, None]] = 0
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, f"{what}: frames {bad[:8].tolist()} differ (first of {bad.size})"


def test_gpu_writer_across_the_65535_frame_split(J, ctx, oracle):
    W = H = 16
    n = N1
    co = _oracle_coeffs(oracle, n, 21)
    d_co = _dev(co.reshape(-1))
    rc, hbuf, hsz, hcap = _host_batch(J, co, W, H, n)
    assert rc == 0 and (hsz > 0).all()
    rc, gbuf, gsz = _gpu_batch(J, ctx, d_co, W, H, n, hcap)
    assert rc == 0, J.load_library().jpezy_hip_last_error()
    _all_files_equal(gbuf, hcap, gsz, hbuf, hcap, hsz, n, "write_jpeg_gpu_batch")
    stride = (int(hsz.max()) + 64) // 64 * 64
    dbuf, dsz = _gpu_dev(ctx, d_co, W, H, n, stride)
    _all_files_equal(dbuf, stride, dsz, hbuf, hcap, hsz, n, "write_jpeg_gpu_dev")
    for f in _sample(n, [SPLIT], k=8):
        assert hbuf[f * hcap: f * hcap + hsz[f]].tobytes() == oracle.write_jpeg(co[f], W, H), f"oracle: frame {f}"

    # per-frame verdicts across the seam: an out-of-table AC coefficient in frames 65534 and 65535 only
    bad_frames = [SPLIT - 1, SPLIT]
    co_bad = co.copy()
    for f in bad_frames:
        co_bad[f, 5 * 64 + 7] = 1024
    d_bad = _dev(co_bad.reshape(-1))
    rc, gbuf2, gsz2 = _gpu_batch(J, ctx, d_bad, W, H, n, hcap)
    assert rc == FORMAT
    assert np.flatnonzero(gsz2 < 0).tolist() == bad_frames and (gsz2[bad_frames] == FORMAT).all()
    keep = np.ones(n, bool)
    keep[bad_frames] = False
    _files_equal(gbuf2, hcap, gsz2, hbuf, hcap, hsz, np.flatnonzero(keep)[::97].tolist() + [SPLIT - 2, SPLIT + 1], "verdict pass")
    dbuf2, dsz2 = _gpu_dev(ctx, d_bad, W, H, n, stride)
    assert np.flatnonzero(dsz2 < 0).tolist() == bad_frames and (dsz2[bad_frames] == FORMAT).all()
    _all_files_equal(dbuf2.reshape(n, stride)[keep].reshape(-1), stride, dsz2[keep], hbuf.reshape(n, hcap)[keep].reshape(-1), hcap,
                     hsz[keep], int(keep.sum()), "write_jpeg_gpu_dev, verdict pass")
    # the next call on the same context is clean: no verdict leaks from the status array into it
    rc, gbuf3, gsz3 = _gpu_batch(J, ctx, d_co, W, H, n, hcap)
    assert rc == 0
    _files_equal(gbuf3, hcap, gsz3, hbuf, hcap, hsz, _sample(n, [SPLIT]), "after verdicts")
    dbuf3, dsz3 = _gpu_dev(ctx, d_co, W, H, n, stride)
    _all_files_equal(dbuf3, stride, dsz3, hbuf, hcap, hsz, n, "write_jpeg_gpu_dev after verdicts")


def _frames_per_pass(J, W, H):
    """the pass rule of both forms of the writer (jpezy_entropy.hip): worst-case streams of 208 bytes per block in whole 16 KB pieces,
    at most 1 GiB of them per pass"""
    mc, mr = J.mcu_grid(W, H)
    nblk = mc * mr * 6
    piece = 16384
    u_stride = (nblk * 208 + 8 + piece - 1) // piece * piece
    return min(65535, (1 << 30) // u_stride)


def test_gpu_writer_across_the_worst_case_pass_split(J, ctx, oracle):
    """1080p: passes of `per` frames; per + 2 frames of mixed dense and sparse content, two of them refused at the seam"""
    import torch
    W, H = 1920, 1080
    per = _frames_per_pass(J, W, H)
    assert per == 105
    n = per + 2
    assert per < n
    mc, mr = J.mcu_grid(W, H)
    cpf = J.coeff_count(W, H)
    rng = np.random.default_rng(1080)
    base = np.zeros((3, mc * mr, 6, 64), np.int16)
    base[0, :, :, 0] = rng.integers(-200, 201, (mc * mr, 6))          # sparse: DC only
    mask = rng.random((mc * mr, 6, 64)) < 0.5
    base[1][mask] = rng.integers(-60, 61, int(mask.sum()))             # dense
    base[2, ::3] = base[1, ::3]                                        # mixed
    base[2, 1::3, :, :3] = rng.integers(-900, 901, ((mc * mr + 1) // 3, 6, 3))
    co = np.empty((n, cpf), np.int16)
    for f in range(n):
        co[f] = base[f % 3].reshape(-1)
        co[f, 0] = f - 50                                               # frame stamp: the first DC
        co[f, 64 * 6 * (f % (mc * mr))] = (f % 7) - 3
    d_co = _dev(co.reshape(-1))
    hcap = (max(len(J.write_jpeg(co[f], W, H)) for f in range(3)) + (64 << 10)) // 4096 * 4096
    rc, hbuf, hsz, _ = _host_batch(J, co, W, H, n, cap=hcap)
    assert rc == 0, hsz[hsz < 0]
    rc, gbuf, gsz = _gpu_batch(J, ctx, d_co, W, H, n, hcap)
    assert rc == 0, J.load_library().jpezy_hip_last_error()
    _all_files_equal(gbuf, hcap, gsz, hbuf, hcap, hsz, n, "write_jpeg_gpu_batch 1080p")
    stride = (int(hsz.max()) + 64) // 64 * 64
    dbuf, dsz = _gpu_dev(ctx, d_co, W, H, n, stride)
    _all_files_equal(dbuf, stride, dsz, hbuf, hcap, hsz, n, "write_jpeg_gpu_dev 1080p")
    for f in (per - 1, per, n - 1):
        assert hbuf[f * hcap: f * hcap + hsz[f]].tobytes() == oracle.write_jpeg(co[f], W, H), f"oracle: frame {f}"
    del dbuf, gbuf
    # per-frame verdicts on both sides of the pass seam
    bad_frames = [per - 1, per]
    for f in bad_frames:
        co[f, 64 * 6 * 100 + 64 * 4 + 9] = -1500
    d_bad = _dev(co.reshape(-1))
    del d_co
    rc, gbuf2, gsz2 = _gpu_batch(J, ctx, d_bad, W, H, n, hcap)
    assert rc == FORMAT
    assert np.flatnonzero(gsz2 < 0).tolist() == bad_frames
    ok = [f for f in range(n) if f not in bad_frames]
    _files_equal(gbuf2, hcap, gsz2, hbuf, hcap, hsz, ok, "1080p verdict pass")
    dbuf2, dsz2 = _gpu_dev(ctx, d_bad, W, H, n, stride)
    assert np.flatnonzero(dsz2 < 0).tolist() == bad_frames and (dsz2[bad_frames] == FORMAT).all()
    _files_equal(dbuf2, stride, dsz2, hbuf, hcap, hsz, ok, "1080p write_jpeg_gpu_dev verdict pass")
    del d_bad
    torch.cuda.empty_cache()
