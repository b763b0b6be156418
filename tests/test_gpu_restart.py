"""Restart intervals from the GPU entropy coder (jpezy_ctx_set_restart_interval): every entry point against the host writer
jpezy_write_jpeg_rst byte for byte, the seams of the launch shape, per-image tables on top, the device-resident form in a captured
graph and one byte short of room, and the files read back by the context's own restart-interval decoder.

The launch shape (jpezy_entropy.hip): a tile (the blocks of one coding workgroup) never straddles an interval -- an interval of Ri
MCUs takes ceil(6 Ri / 256) tiles, all full but its last; restart_bases_kernel rounds the bit offset up to a byte behind every
interval's last tile; assemble_restart_kernel gathers a 64-byte chunk of the unstuffed stream U from however many tiles touch it
and notes the markers behind its bytes; the stuffing kernel inserts them.  The seam tests are named after those mechanisms."""
import subprocess
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import entropy_model as M
import restart_model as R

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = ["rand64", "rand17x33", "gradient52x40", "rand16", "greyramp256x16", "flatgrey256"]
# 16 x 16: one MCU; 688 x 16: 43 MCUs, the first 256-block boundary falls inside an MCU; 2048 x 16: 128 MCUs = three full tiles
SHAPES = [(16, 16), (688, 16), (2048, 16), (272, 48), (328, 232)]


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
def octx(J):
    c = J.Context(0)
    c.set_huffman_optimize(1)
    yield c
    c.close()


def _dev(co):
    import torch
    return torch.from_numpy(np.array(co, dtype=np.int16)).cuda()          # (a copy: the cached fields are read-only)


def _grid(W, H):
    return (W + 15) // 16, (H + 15) // 16


def _intervals(W, H):
    cols, rows = _grid(W, H)
    nmcu = cols * rows
    return sorted({ri for ri in (1, 2, 5, 42, 43, 64, 128, cols, nmcu - 1, nmcu, 65535) if ri >= 1})


@lru_cache(maxsize=None)
def _frames(W, H, gray):
    """three frames [3, nmcu, 4|6, 64] of different content (so that every frame has its own pads): small values with zero runs and
    0xFF-rich blocks, a near-flat frame, larger values"""
    cols, rows = _grid(W, H)
    n = cols * rows
    rng = np.random.default_rng(W * 7 + H)
    a = rng.integers(-6, 7, (n, 6, 64)).astype(np.int16)
    a[..., 8:] *= (rng.random((n, 6, 56)) < 0.3)
    a[..., 0] = rng.integers(-900, 900, (n, 6))
    flat = a.reshape(-1, 64)
    flat[::7, 63] = 1000                                   # blocks without EOB
    flat[3::11, 1:] = 0
    flat[3::11, 40] = -300                                 # two ZRL codes
    flat[5::13, 1:] = 1023                                 # dense blocks: re-coded by the DirectWriter, full of 0xFF bytes
    b = np.zeros((n, 6, 64), np.int16)
    b[..., 0] = 37
    b[::3, 2, 1] = -1
    c = rng.integers(-200, 201, (n, 6, 64)).astype(np.int16)
    co = np.stack([a, b, c])
    co = np.ascontiguousarray(co[:, :, :4]) if gray else co
    co.setflags(write=False)
    return co


def _gpu_dev_files(ctx, co, W, H, gray, n):
    """write_jpeg_gpu_dev: the files and their sizes"""
    import torch
    stride = ctx_bound(W, H)
    out = torch.zeros((n, stride), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
    ctx.write_jpeg_gpu_dev(_dev(co), W, H, out, sizes, gray=gray, n_frames=n)
    torch.cuda.synchronize()
    sz = sizes.cpu().numpy()
    assert (sz > 0).all(), sz
    host = out.cpu().numpy()
    return [host[f, :sz[f]].tobytes() for f in range(n)]


def ctx_bound(W, H):
    import jpezy_amd
    return jpezy_amd.load_library().jpezy_jpeg_bound(W, H)


def _check_all_writers(J, ctx, co, W, H, gray, ri, optimize=False):
    """one frame through write_jpeg_gpu and (Annex K) write_jpeg_gpu_dev against the host writer"""
    ctx.set_restart_interval(ri)
    try:
        want = J.write_jpeg(co, W, H, gray, optimize=optimize, restart_interval=ri)
        got = ctx.write_jpeg_gpu(_dev(co), W, H, gray=gray)[0]
        assert got == want, ("write_jpeg_gpu", W, H, gray, ri, _first_difference(got, want))
        if not optimize:
            got = _gpu_dev_files(ctx, co, W, H, gray, 1)[0]
            assert got == want, ("write_jpeg_gpu_dev", W, H, gray, ri, _first_difference(got, want))
        return want
    finally:
        ctx.set_restart_interval(0)


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = next((i for i in range(n) if a[i] != b[i]), n)
    return dict(len_got=len(a), len_want=len(b), at=d, got=a[max(0, d - 4):d + 8].hex(), want=b[max(0, d - 4):d + 8].hex())


# ---- byte identity over the grid ----
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("W,H", SHAPES)
def test_coefficient_entry_points_equal_host_writer(J, ctx, W, H, gray):
    co = _frames(W, H, gray)
    try:
        for ri in _intervals(W, H):
            ctx.set_restart_interval(ri)
            assert ctx.restart_interval() == ri
            want = [J.write_jpeg(co[f], W, H, gray, restart_interval=ri) for f in range(3)]
            one = ctx.write_jpeg_gpu(_dev(co[0]), W, H, gray=gray)
            assert one[0] == want[0], ("write_jpeg_gpu", ri, _first_difference(one[0], want[0]))
            batch = ctx.write_jpeg_gpu(_dev(co), W, H, gray=gray, n_frames=3)
            for f in range(3):
                assert batch[f] == want[f], ("write_jpeg_gpu_batch", ri, f, _first_difference(batch[f], want[f]))
            dev = _gpu_dev_files(ctx, co, W, H, gray, 3)
            for f in range(3):
                assert dev[f] == want[f], ("write_jpeg_gpu_dev", ri, f, _first_difference(dev[f], want[f]))
        assert len({len(w) for w in want}) == 3
    finally:
        ctx.set_restart_interval(0)


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("W,H", SHAPES)
def test_pixel_entry_points_equal_host_writer(J, ctx, oracle, W, H, gray):
    r, g, b = oracle.synth_rgb(W, H, frame=5)
    co = ctx.fdct_quant(r, g, b, W, H, gray=gray)
    packed = np.ascontiguousarray(np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1))
    try:
        for ri in _intervals(W, H):
            ctx.set_restart_interval(ri)
            want = J.write_jpeg(co, W, H, gray, restart_interval=ri)
            assert ctx.encode_jpeg(r, g, b, W, H, gray=gray) == want, ("encode_jpeg", ri)
            assert ctx.encode_jpeg_packed(packed, gray=gray) == want, ("encode_jpeg_packed", ri)
    finally:
        ctx.set_restart_interval(0)


# ---- the seams of the launch shape ----
def _noise(nmcu, seed, gray=False):
    rng = np.random.default_rng(seed)
    co = rng.integers(-40, 41, (nmcu, 4 if gray else 6, 64)).astype(np.int16)
    co[..., 0] = rng.integers(-500, 500, co.shape[:2])
    return co


@pytest.mark.parametrize("gray", [False, True])
def test_interval_ends_exactly_at_a_tile_end(J, ctx, gray):
    """Ri = 128: 768 blocks, three full tiles and no short one -- the byte rounding of restart_bases_kernel behind a FULL tile.
    256 and 384 MCUs: two and three such intervals."""
    for W, H in ((4096, 16), (2048, 48)):
        nmcu = _grid(W, H)[0] * _grid(W, H)[1]
        _check_all_writers(J, ctx, _noise(nmcu, nmcu, gray), W, H, gray, 128)


@pytest.mark.parametrize("gray", [False, True])
def test_interval_ends_two_blocks_into_a_tile(J, ctx, gray):
    """Ri = 43: 258 blocks, a full tile and a tile of TWO blocks (6 Ri is even: the shortest last tile there is).  On flat content
    that tile is one byte of stream, so a 64-byte chunk of U takes bits from more than two tiles (assemble_chunk_restart's loop);
    on noise the short tile lies inside one chunk."""
    for H in (32, 48):
        nmcu = 43 * (H // 16)
        flat = np.zeros((nmcu, 4 if gray else 6, 64), np.int16)
        flat[:, :, 0] = 9
        for co in (flat, _noise(nmcu, 43 + H, gray)):
            _check_all_writers(J, ctx, co, 688, H, gray, 43)
    # and one MCU more or less per interval: last tiles of 8 blocks and of 252
    nmcu = 3 * 44
    _check_all_writers(J, ctx, _noise(nmcu, 44, gray), 16 * nmcu, 16, gray, 44)
    _check_all_writers(J, ctx, _noise(nmcu, 42, gray), 16 * nmcu, 16, gray, 42)


def test_interval_whose_last_block_is_recoded_by_the_direct_writer(J, ctx):
    """a block that overflows its LDS row (entropy_model.fits_row is False) as the last block of an interval, colour (the Cr block)
    and gray (luma block 3; the two zero chroma blocks follow it): the DirectWriter's partial last word is the tile's last"""
    z = M.block_of_bits(1121, t=1)
    assert z is not None and not M.fits_row(z, 0, 1) and not M.fits_row(M.dense_block(), 0, 0)
    co = _noise(6, 61).copy()
    co[1, 5] = z
    co[3, 5] = M.dense_block(3)
    co[3, 4] = M.dense_block(-3)
    for ri in (1, 2):
        _check_all_writers(J, ctx, co, 96, 16, False, ri)
    g = _noise(6, 62, gray=True).copy()
    g[1, 3] = M.dense_block(1)
    g[3, 3] = M.block_of_bits(1121, t=0, pred=0, dc=0)
    for ri in (1, 2):
        _check_all_writers(J, ctx, g, 96, 16, True, ri)


def test_every_pad_length_and_no_pad(J, ctx):
    """intervals of every bit length mod 8 (entropy_model.tuner_block): pads of 0..7 bits, among them the interval that ends on a
    byte and gets none"""
    mcus = [R.mcu_of_bits(bits) for bits in range(40, 48)]
    co = np.stack(mcus + [R.flat_mcu()])
    assert sorted(b % 8 for b in R.interval_bits(co, 1)[:-1]) == list(range(8))
    want = _check_all_writers(J, ctx, co, 16 * co.shape[0], 16, False, 1)
    assert R.split(want)[1] == R.scan(co, 1)
    # two MCUs per interval, every interval on a byte: no pad bit anywhere but in the frame's last byte
    co = np.stack([R.mcu_of_bits(b) for b in (40, 48, 56, 64, 43)])
    assert all(b % 8 == 0 for b in R.interval_bits(co, 2)[:-1]) and R.interval_bits(co, 2)[-1] % 8 == 3
    _check_all_writers(J, ctx, co, 16 * co.shape[0], 16, False, 2)


def test_ff_as_the_last_data_byte_before_a_marker(J, ctx):
    """an interval that ends, on a byte, in ten one bits: FF 00 FF Dn -- the stuffing kernel stuffs the data byte and not the marker"""
    co = None
    for bits in range(6, 80):
        z = M.tuner_block(bits, 0)
        if z is None:
            continue
        mcu = R.flat_mcu()
        mcu[0] = z
        mcu[5] = M.dense_block()
        cand = np.stack([mcu, R.flat_mcu(), mcu, mcu])
        if R.interval_bits(cand, 1)[0] % 8 == 0:
            co = cand
            break
    assert co is not None and R.unstuffed_intervals(co, 1)[0][-1] == 0xFF
    want = _check_all_writers(J, ctx, co, 64, 16, False, 1)
    assert R.split(want)[1].count(b"\xff\x00\xff\xd0") == 1 and b"\xff\x00\xff\xd2" in R.split(want)[1]


@lru_cache(maxsize=None)
def _flat_bits():
    assert R.interval_bits(np.stack([R.flat_mcu()] * 3), 1) == [32, 32, 32]
    return 32


@pytest.mark.parametrize("lead", [32, 40, 56])
def test_markers_at_chunk_and_piece_borders(J, ctx, lead):
    """flat content is 32 bits per MCU, so with Ri = 16 every interval is 64 bytes -- one chunk of U.  lead = 32: every interval ends
    on the LAST byte of a chunk, the 256th on the last byte of a 16 KB piece (the marker is the last thing the piece's workgroup
    writes, the next piece's offset counts it).  lead = 40 (the first MCU one byte longer): every interval ends on the FIRST byte of
    a chunk, the 256th on the first byte of the second piece.  lead = 56: three bytes in, chunk and marker interleave.
    4224 MCUs: 16.5 KB of stream, two pieces."""
    W, H = 1024, 1056
    cols, rows = _grid(W, H)
    nmcu = cols * rows
    assert nmcu * _flat_bits() // 8 > 16384
    co = np.zeros((nmcu, 6, 64), np.int16)
    co[0] = R.mcu_of_bits(lead)
    assert R.interval_bits(co[:32], 16) == [15 * 32 + lead, 512]
    want = _check_all_writers(J, ctx, co, W, H, False, 16)
    seg = R.split(want)[1]
    assert R.markers(seg) == R.expected_markers(nmcu, 16) and len(R.markers(seg)) == 263


def test_flat_content_one_mcu_per_interval(J, ctx, octx):
    """the shortest intervals there are: 4 bytes with the Annex-K tables (16 markers per chunk of U), 2 bytes with the frame's own
    one-bit codes (32 markers per chunk: the 192 bytes per chunk the stuffing kernel stages are all used)"""
    W, H = 272, 48
    nmcu = 17 * 3
    co = np.zeros((nmcu, 6, 64), np.int16)
    want = _check_all_writers(J, ctx, co, W, H, False, 1)
    assert len(R.split(want)[1]) == 4 * nmcu + 2 * (nmcu - 1)
    want = _check_all_writers(J, octx, co, W, H, False, 1, optimize=True)
    assert len(R.split(want)[1]) == 2 * nmcu + 2 * (nmcu - 1)
    g = np.zeros((nmcu, 4, 64), np.int16)
    _check_all_writers(J, ctx, g, W, H, True, 1)
    _check_all_writers(J, octx, g, W, H, True, 1, optimize=True)


@pytest.mark.parametrize("gray", [False, True])
def test_more_tiles_than_one_batch_of_the_offsets_kernel(J, ctx, gray):
    """restart_bases_kernel walks tiles and intervals in batches of 2048 with a running carry -- the number ASM_SELF_TILES also is,
    above which a frame without intervals takes its offsets from a kernel of their own.  The smallest frame with more tiles and
    Ri = one MCU row: 16 x 32784, 2049 rows of one MCU, 2049 tiles, 2049 intervals.  Flat but for a few MCUs; the host writer only."""
    W, H = 16, 2049 * 16
    nmcu = 2049
    co = np.zeros((nmcu, 4 if gray else 6, 64), np.int16)
    co[:, :, 0] = 5
    co[[0, 2047, 2048], 0, 1:9] = (-700, 3, 90, -5, 200, -200, 1, 1)
    _check_all_writers(J, ctx, co, W, H, gray, 1)
    # three MCUs per row: 683 rows and one more
    W, H = 48, 684 * 16
    co = np.zeros((3 * 684, 4 if gray else 6, 64), np.int16)
    co[::5, 1, 0] = 11
    _check_all_writers(J, ctx, co, W, H, gray, 3)


# ---- per-image tables on top ----
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("W,H", [(688, 16), (272, 48), (328, 232)])
def test_optimised_tables_with_restart_intervals(J, octx, W, H, gray):
    import torch
    co = _frames(W, H, gray)[:, :, :, :]
    co = np.ascontiguousarray(co[::2])                       # (the frame of larger values and the first one)
    cols, rows = _grid(W, H)
    try:
        for ri in (1, 5, 43, cols, cols * rows - 1):
            octx.set_restart_interval(ri)
            got = octx.write_jpeg_gpu(_dev(co), W, H, gray=gray, n_frames=2)
            for f in range(2):
                want = J.write_jpeg(co[f], W, H, gray, optimize=True, restart_interval=ri)
                assert got[f] == want, (ri, f, _first_difference(got[f], want))
            if (W, H) != (328, 232) or ri == cols:
                hist = torch.full((2, 4, 256), -1, dtype=torch.int64, device="cuda")
                octx.huffman_histogram_dev(_dev(co), W, H, hist, gray=gray, n_frames=2)
                torch.cuda.synchronize()
                for f in range(2):
                    want_h, ok = R.symbol_counts(co[f], ri, gray)
                    assert ok and np.array_equal(hist[f].cpu().numpy(), want_h), (ri, f)
                    if ri == 1:       # (every MCU's DC differences are taken against 0: not the counts of the frame without restarts)
                        assert not np.array_equal(want_h, R.symbol_counts(co[f], 0, gray)[0])
    finally:
        octx.set_restart_interval(0)


def test_device_resident_form_still_refuses_optimised_tables(J, octx):
    import torch
    co = _frames(272, 48, False)[0]
    out = torch.zeros((1, ctx_bound(272, 48)), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
    octx.set_restart_interval(5)
    try:
        with pytest.raises(J.JpezyError, match="status -4"):
            octx.write_jpeg_gpu_dev(_dev(co), 272, 48, out, sizes)
    finally:
        octx.set_restart_interval(0)
    assert not out.any()


# ---- the device-resident form ----
def test_device_resident_form_in_a_captured_graph(J, ctx):
    import torch
    W, H, n = 272, 48, 3
    frames = _frames(W, H, False)
    co = _dev(frames)
    out = torch.zeros((n, ctx_bound(W, H)), dtype=torch.uint8, device="cuda")
    sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
    ctx.set_restart_interval(17)
    try:
        ctx.write_jpeg_gpu_dev(co, W, H, out, sizes, n_frames=n)          # header and scratch: outside the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                ctx.write_jpeg_gpu_dev(co, W, H, out, sizes, n_frames=n, stream=s.cuda_stream)
        for turn in range(2):                                             # replayed twice on changed coefficients
            changed = np.roll(frames, turn + 1, axis=0).copy()
            changed[:, turn, 0, 0] += 3
            co.copy_(torch.from_numpy(changed).cuda())
            out.zero_(); sizes.zero_()
            g.replay()
            torch.cuda.synchronize()
            for f in range(n):
                want = J.write_jpeg(changed[f], W, H, restart_interval=17)
                assert int(sizes[f]) == len(want) and out[f, :len(want)].cpu().numpy().tobytes() == want, (turn, f)
    finally:
        ctx.set_restart_interval(0)


def test_nospace_one_byte_short(J, ctx):
    """out_stride one byte short of the file: JPEZY_E_NOSPACE and nothing written -- the fit decision counts pads and markers"""
    import torch
    W, H = 272, 48
    co = _frames(W, H, False)[0]
    ctx.set_restart_interval(2)
    try:
        want = J.write_jpeg(co, W, H, restart_interval=2)
        assert len(want) > len(J.write_jpeg(co, W, H)) + 2 * 24
        for short, verdict in ((1, -6), (0, len(want))):
            stride = len(want) - short
            buf = torch.full((stride + 4096,), 0xA5, dtype=torch.uint8, device="cuda")        # the file's room and a guard behind it
            sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
            ctx.write_jpeg_gpu_dev(_dev(co), W, H, buf[:stride].view(1, stride), sizes)
            torch.cuda.synchronize()
            assert int(sizes[0]) == verdict
            host = buf.cpu().numpy()
            assert (host[stride:] == 0xA5).all()
            if short:
                assert (host == 0xA5).all()
            else:
                assert host[:stride].tobytes() == want
    finally:
        ctx.set_restart_interval(0)


def test_comment_room_and_range(J, ctx):
    co = _frames(272, 48, False)[0]
    c390, c391 = (bytes(0x61 + i % 26 for i in range(n)) for n in (390, 391))
    with pytest.raises(J.JpezyError, match="status -1"):
        ctx.set_restart_interval(-1)
    with pytest.raises(J.JpezyError, match="status -1"):
        ctx.set_restart_interval(65536)
    assert ctx.restart_interval() == 0
    ctx.set_restart_interval(65535)
    try:
        assert ctx.restart_interval() == 65535
        ctx.set_restart_interval(4)
        assert ctx.write_jpeg_gpu(_dev(co), 272, 48, comment=c390)[0] == J.write_jpeg(co, 272, 48, comment=c390, restart_interval=4)
        with pytest.raises(J.JpezyError, match="status -1"):
            ctx.write_jpeg_gpu(_dev(co), 272, 48, comment=c391)
    finally:
        ctx.set_restart_interval(0)
    assert ctx.write_jpeg_gpu(_dev(co), 272, 48, comment=c391)[0] == J.write_jpeg(co, 272, 48, comment=c391)


def test_out_of_range_coefficient(J, ctx):
    co = _frames(272, 48, False)[0].copy()
    co[20, 2, 7] = 1024
    ctx.set_restart_interval(3)
    try:
        with pytest.raises(J.JpezyError):
            ctx.write_jpeg_gpu(_dev(co), 272, 48)
        good = _frames(272, 48, False)[0]
        assert ctx.write_jpeg_gpu(_dev(good), 272, 48)[0] == J.write_jpeg(good, 272, 48, restart_interval=3)
        _flags_do_not_leak_between_the_two_forms(J, ctx)
    finally:
        ctx.set_restart_interval(0)


def _flags_do_not_leak_between_the_two_forms(J, ctx):
    """Both forms keep their per-frame error flags in one scratch layout of the context.  272 x 48 (51 MCUs, two tiles), Ri = 3, three
    frames, the middle one with a coefficient of 1024: the host-delivered form, then the device-resident form, refuse frame 1 alone;
    the three good frames through the device-resident and then the host-delivered form: nothing is left of the refusals."""
    import ctypes as C
    import torch
    W, H, n = 272, 48, 3
    lib = J.load_library()
    cap = ctx_bound(W, H)
    good = np.array(_frames(W, H, False))
    bad = good.copy()
    bad[1, 20, 2, 7] = 1024
    want = [J.write_jpeg(good[f], W, H, restart_interval=3) for f in range(n)]

    def batch(co):
        buf = np.zeros(cap * n, np.uint8)
        sizes = (C.c_long * n)()
        rc = lib.jpezy_write_jpeg_gpu_batch(ctx._h, _dev(co).data_ptr(), W, H, 0, n, b"Encoded by jpezy", buf.ctypes.data_as(C.c_void_p), cap, sizes)
        return rc, [sizes[f] if sizes[f] < 0 else buf[f * cap: f * cap + sizes[f]].tobytes() for f in range(n)]

    def dev(co):
        out = torch.zeros((n, cap), dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(n, dtype=torch.int64, device="cuda")
        ctx.write_jpeg_gpu_dev(_dev(co), W, H, out, sizes, n_frames=n)
        torch.cuda.synchronize()
        sz, host = sizes.cpu().numpy(), out.cpu().numpy()
        return [int(sz[f]) if sz[f] < 0 else host[f, :sz[f]].tobytes() for f in range(n)]

    FORMAT = -5
    rc, got = batch(bad)
    assert rc == FORMAT and got == [want[0], FORMAT, want[2]], (rc, [g if isinstance(g, int) else len(g) for g in got])
    got = dev(bad)
    assert got == [want[0], FORMAT, want[2]], [g if isinstance(g, int) else len(g) for g in got]
    assert dev(good) == want
    rc, got = batch(good)
    assert rc == 0 and got == want


# ---- round trips ----
def test_own_decoder_takes_the_files_on_its_restart_path(J, ctx, oracle):
    """read_jpeg_gpu: the regular-restart device path (one pass), with intervals short enough for a lane each and long enough for
    subsequences inside every interval; decode_jpeg: the planes of the file without restarts"""
    W, H = 328, 232
    co = _frames(W, H, False)[2]
    cols, rows = _grid(W, H)
    ctx.set_huffdec_min_bytes(0)
    plain = J.write_jpeg(co, W, H)
    want_planes = ctx.decode_jpeg(plain)
    try:
        for ri, per_lane in ((1, True), (3, True), (105, False)):
            ctx.set_restart_interval(ri)
            jpg = ctx.write_jpeg_gpu(_dev(co), W, H)[0]
            n_int = -(-cols * rows // ri)
            assert (len(R.split(jpg)[1]) // n_int <= 4096) == per_lane, (ri, len(jpg))
            info, d = ctx.read_jpeg_gpu(jpg)
            assert info.restart_interval == ri and ctx.last_huffdec_passes() == 1
            assert np.array_equal(d.cpu().numpy().reshape(co.shape), co)
            got = ctx.decode_jpeg(jpg)
            for k in range(1, 4):
                assert np.array_equal(got[k], want_planes[k]), (ri, k)
            info, back = oracle.read_jpeg(jpg)
            assert info.restart_interval == ri and np.array_equal(back.reshape(co.shape), co)
    finally:
        ctx.set_restart_interval(0)
        ctx.set_huffdec_min_bytes(32 << 10)


def test_setting_is_per_context_and_zero_restores_every_byte(J, ctx):
    other = J.Context(0)
    try:
        for name in FIXTURES:
            z = np.load(GOLDEN / f"{name}.npz")
            W, H = int(z["W"]), int(z["H"])
            other.set_restart_interval(3)
            assert other.write_jpeg_gpu(_dev(z["coeffs"]), W, H)[0] == J.write_jpeg(z["coeffs"], W, H, restart_interval=3)
            # a second context is unaffected ...
            assert ctx.restart_interval() == 0
            assert ctx.write_jpeg_gpu(_dev(z["coeffs"]), W, H)[0] == z["jpg"].tobytes(), name
            # ... and back at 0 the first writes the golden bytes again, through both forms
            other.set_restart_interval(0)
            assert other.write_jpeg_gpu(_dev(z["coeffs"]), W, H)[0] == z["jpg"].tobytes(), name
            assert other.write_jpeg_gpu(_dev(z["coeffs_gray"]), W, H, gray=True)[0] == z["jpg_gray"].tobytes(), name
            assert _gpu_dev_files(other, z["coeffs"], W, H, False, 1)[0] == z["jpg"].tobytes(), name
    finally:
        other.close()


def test_cli_restart_flag(J, ctx, oracle, tmp_path):
    """jpezy_encode in.ppm out.jpg [--gray] [--optimize] [--restart=N], the token anywhere behind the output name; jpezy_decode gives
    the ppm of the run without the flag; a malformed N is a usage error"""
    from jpezy_amd import _build
    _build.build_all()
    enc, dec = Path(_build.BIN) / "jpezy_encode", Path(_build.BIN) / "jpezy_decode"
    W, H = 100, 37
    r, g, b = oracle.synth_rgb(W, H, frame=1)
    src = tmp_path / "in.ppm"
    src.write_bytes(oracle.format_ppm_p3(W, H, r, g, b))

    def run(exe, *args):
        return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=120)
    plain, plain_ppm = tmp_path / "plain.jpg", tmp_path / "plain.ppm"
    assert run(enc, src, plain).returncode == 0
    assert run(dec, plain, plain_ppm).returncode == 0
    for flags, gray, opt in ((["--restart=5"], False, False), (["--gray", "--restart=5"], True, False),
                             (["--restart=2", "--optimize", "--gray"], True, True), (["--optimize", "--restart=7"], False, True),
                             (["--restart=0"], False, False)):
        out = tmp_path / "a.jpg"
        p = run(enc, src, out, *flags)
        assert p.returncode == 0, (flags, p.stderr)
        ri = int(next(f for f in flags if f.startswith("--restart=")).split("=")[1])
        co = ctx.fdct_quant(r, g, b, W, H, gray=gray)
        assert out.read_bytes() == J.write_jpeg(co, W, H, gray, optimize=opt, restart_interval=ri), flags
        if not gray:
            back = tmp_path / "a.ppm"
            assert run(dec, out, back).returncode == 0
            assert back.read_bytes() == plain_ppm.read_bytes(), flags
    usage = run(enc, src)
    assert usage.returncode != 0
    for bad in ("--restart=", "--restart=x", "--restart=-1", "--restart=65536", "--restart=5x", "--restart=123456"):
        p = run(enc, src, tmp_path / "b.jpg", bad)
        assert p.returncode == usage.returncode and p.stderr == usage.stderr, bad
