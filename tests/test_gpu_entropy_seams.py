"""The GPU entropy coder's internal seams, each hit on purpose by a field built with the bit-length model (tests/entropy_model.py,
checked against the host writer by tests/test_entropy_model.py), and the comment limit through every GPU writer.  Every field
goes through write_jpeg_gpu (one frame and a batch) and write_jpeg_gpu_dev and must give the bytes of the host writer and of the
oracle; every construction asserts that it landed on its seam.  The seams (jpezy_entropy.hip):
- the in-place LDS row: a block stream of up to 140 bytes (35 words) is coded in the row, a longer one is re-coded (DirectWriter);
- blocks shorter than a 32-bit word, whose bits the owner of a partial word pulls from the following lanes, at tile ends;
- 256-block tiles; self-scanning assembly up to ASM_SELF_TILES = 2048 tiles per frame, the tile-bases kernel beyond;
- 0xFF counting per 64-byte chunk and per 16 KB piece of the unstuffed stream, and the last byte before the pad bits and EOI;
- DC prediction across tiles and frames (every frame of a batch starts from a predictor of 0)."""
import re
from pathlib import Path

import numpy as np
import pytest

import entropy_model as M

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CHUNK, PIECE = 64, 16384
BADARG = -1


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


def _dev(co):
    import torch
    return torch.from_numpy(np.ascontiguousarray(co, dtype=np.int16).reshape(-1)).cuda()


def check_field(J, ctx, oracle, co, W, H, gray=False, batch=2, what=""):
    """host writer == oracle == write_jpeg_gpu == write_jpeg_gpu (batch) == write_jpeg_gpu_dev (batch)"""
    import torch
    co = np.ascontiguousarray(co, dtype=np.int16).reshape(-1)
    want = J.write_jpeg(co, W, H, gray=gray)
    assert want == oracle.write_jpeg(co, W, H, gray=gray), f"{what}: host writer != oracle"
    d = _dev(co)
    assert ctx.write_jpeg_gpu(d, W, H, gray=gray) == [want], f"{what}: write_jpeg_gpu, one frame"
    db = _dev(np.tile(co, batch))
    assert ctx.write_jpeg_gpu(db, W, H, gray=gray, n_frames=batch) == [want] * batch, f"{what}: write_jpeg_gpu, batch"
    stride = (len(want) + 127) // 64 * 64
    d_out = torch.zeros((batch, stride), dtype=torch.uint8, device="cuda")
    d_sz = torch.zeros(batch, dtype=torch.int64, device="cuda")
    ctx.write_jpeg_gpu_dev(db, W, H, d_out, d_sz, gray=gray, n_frames=batch)
    torch.cuda.synchronize()
    out, sz = d_out.cpu().numpy(), d_sz.cpu().numpy()
    for f in range(batch):
        assert sz[f] == len(want) and out[f, :sz[f]].tobytes() == want, f"{what}: write_jpeg_gpu_dev frame {f}"
    return want


def _table(i):
    return 0 if i % 6 < 4 else 1


def _zero_bits(i, gray=False):
    return 6 if _table(i) == 0 else 4          # DC difference 0 + EOB


def exact_block(bits, t):
    z = M.tuner_block(bits, t)
    return z if z is not None else M.block_of_bits(bits, 0, t)


def frame_of_bits(total, gray=False, filler=900):
    """[nmcu, bpm, 64] of exactly `total` coded bits, DC 0 everywhere: filler blocks of `filler` bits, then zero blocks, and the
    last stored block (Cr; the last luma block in gray) tuned to the exact length"""
    bpm = 4 if gray else 6
    nmcu = max(1, -(-total // (4 * filler + (8 if gray else 2 * filler))))
    n = nmcu * 6
    last = n - 1 if not gray else n - 3
    zero = [_zero_bits(i) for i in range(n)]
    co = np.zeros((nmcu, bpm, 64), np.int16)
    fixed = 0
    for i in range(n):
        if i == last:
            continue
        rest_min = sum(zero[j] for j in range(i + 1, n) if j != last)
        if i < last and not (gray and i % 6 >= 4) and total - fixed - filler - rest_min >= 400:
            co[i // 6, i % 6] = M.block_of_bits(filler, 0, _table(i))
            fixed += filler
        else:
            fixed += zero[i]
    z = exact_block(total - fixed, _table(last))
    assert z is not None, (total, fixed)
    co[last // 6, last % 6] = z
    assert int(M.block_lengths(co, gray).sum()) == total
    return co


def _tile_count(W, H):
    mc, mr = (W + 15) // 16, (H + 15) // 16
    return -(-mc * mr * 6 // 256)


# ---- the in-place row against the DirectWriter ----
@pytest.mark.parametrize("gray", [False, True])
def test_blocks_at_the_row_limit(J, ctx, oracle, gray):
    """blocks of 139, 140 (in the row) and 141 bytes (re-coded), and the 208-byte worst case, side by side in one tile"""
    lengths = [8 * 139 - 7, 8 * 139, 8 * 140 - 1, 8 * 140, 8 * 140 + 1, 8 * 141]
    luma = []
    for bits in lengths:
        z = M.block_of_bits(bits, 0, 0)
        assert M.block_bits(z, 0, 0) == bits and M.fits_row(z, 0, 0) == (bits <= 8 * M.ROW_BYTES), bits
        luma.append(z)
    worst = M.dense_block(dc=-1023)
    nmcu = 4
    co = np.zeros((nmcu, 4 if gray else 6, 64), np.int16)
    slots = [(m, i) for m in range(nmcu) for i in range(4)]
    for (m, i), z in zip(slots, luma):
        co[m, i] = z
    co[1, 3, 0] = 1023                                       # the DC before the worst block: a category-11 difference
    co[2, 0] = worst
    if not gray:
        for m in range(nmcu):
            for i, bits in ((4, 8 * 140), (5, 8 * 140 + 1)):
                z = M.block_of_bits(bits - m, 0, 1)
                co[m, i] = z
    lens = M.block_lengths(co, gray)
    rows = lens.reshape(nmcu, 6)
    assert rows[2, 0] == 9 + 11 + 63 * 26 and (rows[2, 0] + 7) // 8 == 208
    assert {8 * 139, 8 * 140, 8 * 140 + 1} <= set(int(x) for x in lens)
    check_field(J, ctx, oracle, co, 32, 32, gray, what=f"row limit gray={gray}")


# ---- blocks shorter than a word at tile ends ----
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("end", [255, 256, 257])
def test_short_blocks_end_at_tile_boundary(J, ctx, oracle, end, gray):
    """long blocks, then a run of blocks shorter than 32 bits that ends at coded block `end` (255: the last lane of tile 0,
    256: the first lane of tile 1), then long blocks again: the partial words before and inside the run are completed from
    the rows of the following lanes up to the tile's end"""
    nmcu = 3 * 256 // 6
    co = np.zeros((nmcu, 4 if gray else 6, 64), np.int16)
    start = 180
    for i in range(nmcu * 6):
        if gray and i % 6 >= 4:
            continue
        if start <= i <= end:
            continue                                      # zero block: 6 or 4 bits
        co[i // 6, i % 6] = M.block_of_bits(200 + 7 * (i % 5), 0, _table(i))
    lens = M.block_lengths(co, gray)
    assert (lens[start:end + 1] < 32).all() and lens[end + 1] >= (4 if gray and (end + 1) % 6 >= 4 else 32)
    assert lens[end + 1:end + 4].max() >= 32 and lens[start - 4:start].max() >= 32
    check_field(J, ctx, oracle, co, 16 * nmcu, 16, gray, what=f"short run to {end}")


# ---- frame-level tile counts: self-scanning assembly against the tile-bases path ----
@pytest.mark.parametrize("W,H,tiles", [(22192, 1008, 2048), (21184, 1056, 2049)])
def test_frames_of_2048_and_2049_tiles(J, ctx, oracle, W, H, tiles):
    assert _tile_count(W, H) == tiles
    mc, mr = (W + 15) // 16, (H + 15) // 16
    rng = np.random.default_rng(tiles)
    co = np.zeros((mc * mr, 6, 64), np.int16)
    co[:, :, 0] = rng.integers(-300, 301, (mc * mr, 6))
    k = rng.integers(1, 64, (mc * mr, 6, 3))
    np.put_along_axis(co, k, rng.integers(-40, 41, k.shape).astype(np.int16), axis=2)
    co[-1, -1, 1:] = 1023                                     # a dense last block: the last tile's end is full of 0xFF bytes
    check_field(J, ctx, oracle, co, W, H, batch=2, what=f"{tiles} tiles")


# ---- stream lengths around 4-byte words, 64-byte chunks and 16 KB pieces ----
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("L", [63, 64, 65, PIECE - 1, PIECE, PIECE + 1, 4 * PIECE - 1, 4 * PIECE + 1])
def test_stream_lengths_on_chunk_and_piece_boundaries(J, ctx, oracle, L, gray):
    for total in (8 * L, 8 * L - 3):
        co = frame_of_bits(total, gray)
        nmcu = co.shape[0]
        stream = M.unstuffed_stream(co, gray)
        assert len(stream) == L and len(stream) % 4 in (0, 1, 3)
        if total == 8 * L and not gray:
            assert stream[-1] == 0xFF                          # the last data byte is 0xFF (no pad bits behind it)
        jpg = check_field(J, ctx, oracle, co, 16 * nmcu, 16, gray, what=f"L={L} bits={total}")
        assert M.scan_of(jpg) == stream


# ---- 0xFF bytes on the chunk and piece edges ----
@pytest.mark.parametrize("P", [CHUNK - 1, CHUNK, 3 * CHUNK - 1, PIECE - 1, PIECE, 2 * PIECE - 1, 2 * PIECE])
def test_ff_byte_on_chunk_and_piece_edges(J, ctx, oracle, P):
    """a 0xFF byte as the last / first byte of a 64-byte chunk and of a 16 KB piece: a prefix of exactly the right length in
    front of a dense luma block whose code has runs of 21 one bits"""
    dense = M.block_bitstring(M.dense_block(), 0, 0)
    offs = [o for o in range(len(dense) - 8) if dense[o:o + 8] == "11111111"]
    done = False
    for o in offs:
        prefix = 8 * P - o
        if prefix < 200:
            continue
        # the dense block goes at luma slot 0 of MCU m; the blocks before it carry exactly `prefix` bits
        pre = frame_of_bits(prefix)
        m = pre.shape[0]
        co = np.zeros((m + 2, 6, 64), np.int16)
        co[:m] = pre
        co[m, 0] = M.dense_block()
        stream = M.unstuffed_stream(co)
        assert stream[P] == 0xFF and int(M.block_lengths(co)[:6 * m].sum()) == prefix
        check_field(J, ctx, oracle, co, 16 * (m + 2), 16, what=f"0xFF at {P}")
        done = True
        break
    assert done


# ---- DC prediction across tiles and frames ----
@pytest.mark.parametrize("gray", [False, True])
def test_dc_chains_of_category_11_across_tiles_and_frames(J, ctx, oracle, gray):
    import torch
    nmcu = 2 * 256 // 6 + 5                                     # three tiles
    bpm = 4 if gray else 6
    co = np.zeros((nmcu, bpm, 64), np.int16)
    sign = np.where(np.arange(nmcu * 4) % 2 == 0, 1023, -1023)
    co[:, :4, 0] = sign.reshape(nmcu, 4)
    if not gray:
        co[:, 4, 0] = np.where(np.arange(nmcu) % 2 == 0, -1023, 1023)
        co[:, 5, 0] = np.where(np.arange(nmcu) % 2 == 0, 1023, -1023)
    co[::7, :, 5] = 3
    # every difference after the first of a chain is +-2046 (category 11), including those at the tile borders (blocks 256, 512)
    diffs = [category for category in (M.category(d) for d in np.diff(sign))]
    assert set(diffs) == {11}
    W = 16 * nmcu
    check_field(J, ctx, oracle, co, W, 16, gray, batch=3, what=f"DC chains gray={gray}")
    # a batch whose frames end on the opposite sign of the next frame's first DC: each frame's first DC is coded against 0
    frames = [co, -co, co]
    want = [J.write_jpeg(f, W, 16, gray=gray) for f in frames]
    got = ctx.write_jpeg_gpu(_dev(np.stack(frames)), W, 16, gray=gray, n_frames=3)
    assert got == want
    stride = (max(len(w) for w in want) + 127) // 64 * 64
    d_out = torch.zeros((3, stride), dtype=torch.uint8, device="cuda")
    d_sz = torch.zeros(3, dtype=torch.int64, device="cuda")
    ctx.write_jpeg_gpu_dev(_dev(np.stack(frames)), W, 16, d_out, d_sz, gray=gray, n_frames=3)
    torch.cuda.synchronize()
    for f in range(3):
        assert d_out[f, :int(d_sz[f])].cpu().numpy().tobytes() == want[f], f


# ---- one comment limit for every writer ----
def _max_comment():
    return int(re.search(r"#define\s+JPEZY_MAX_COMMENT\s+(\d+)", (ROOT / "include" / "jpezy_hip.h").read_text()).group(1))


def test_comment_limit_through_every_writer(J, ctx, oracle):
    import ctypes as C
    import torch
    lib = J.load_library()
    limit = _max_comment()
    W, H = 32, 16
    rng = np.random.default_rng(8)
    co = rng.integers(-40, 41, (2, 6, 64)).astype(np.int16)
    r, g, b = oracle.synth_rgb(W, H, frame=3)
    co_rgb = oracle.encode_coeffs(r, g, b, W, H).reshape(-1)
    d = _dev(co)
    for n in (0, 1, limit, limit + 1):
        c = bytes((0x61 + i % 26) for i in range(n))
        if n <= limit:
            want = J.write_jpeg(co, W, H, comment=c)
            assert want == oracle.write_jpeg(co, W, H, comment=c), n
            assert J.write_jpeg_batch(np.stack([co, co]), W, H, 2, comment=c) == [want, want], n
            assert ctx.write_jpeg_gpu(d, W, H, comment=c) == [want], n
            assert ctx.write_jpeg_gpu(_dev(np.stack([co, co])), W, H, comment=c, n_frames=2) == [want, want], n
            d_out = torch.zeros((1, 4096), dtype=torch.uint8, device="cuda")
            d_sz = torch.zeros(1, dtype=torch.int64, device="cuda")
            ctx.write_jpeg_gpu_dev(d, W, H, d_out, d_sz, comment=c)
            torch.cuda.synchronize()
            assert d_out[0, :int(d_sz[0])].cpu().numpy().tobytes() == want, n
            want_rgb = J.write_jpeg(co_rgb, W, H, comment=c)
            assert ctx.encode_jpeg(r, g, b, W, H, comment=c) == want_rgb, n
            _, jpgs = J.encode_batch_multi([0, 0], np.tile(r, 3), np.tile(g, 3), np.tile(b, 3), W, H, 3, chunk_frames=1, comment=c)
            assert jpgs == [want_rgb] * 3, n
            with J.MultiEncoder([0], W, H, chunk_frames=2) as Mh:
                _, jpgs = Mh.encode(np.tile(r, 2), np.tile(g, 2), np.tile(b, 2), 2, comment=c)
            assert jpgs == [want_rgb] * 2, n
            continue
        # one byte over the limit: every writer refuses it with JPEZY_E_BADARG, and says why
        buf = np.zeros(1 << 16, np.uint8)
        sizes = (C.c_long * 2)()
        p = buf.ctypes.data_as(C.c_void_p)
        cp = co.ctypes.data_as(C.c_void_p)
        rcs = {
            "write_jpeg": lib.jpezy_write_jpeg(cp, W, H, 0, c, p, 1 << 16),
            "write_jpeg_batch": lib.jpezy_write_jpeg_batch(cp, W, H, 0, 1, c, p, 1 << 16, sizes, 1),
            "write_jpeg_gpu": lib.jpezy_write_jpeg_gpu(ctx._h, d.data_ptr(), W, H, 0, c, p, 1 << 16),
            "write_jpeg_gpu_batch": lib.jpezy_write_jpeg_gpu_batch(ctx._h, d.data_ptr(), W, H, 0, 1, c, p, 1 << 16, sizes),
        }
        d_out = torch.zeros((1, 4096), dtype=torch.uint8, device="cuda")
        d_sz = torch.zeros(1, dtype=torch.int64, device="cuda")
        rcs["write_jpeg_gpu_dev"] = lib.jpezy_write_jpeg_gpu_dev(ctx._h, d.data_ptr(), W, H, 0, 1, c, d_out.data_ptr(), 4096,
                                                                 d_sz.data_ptr(), None)
        rp = [np.ascontiguousarray(x).ctypes.data_as(C.c_void_p) for x in (r, g, b)]
        rcs["encode_jpeg"] = lib.jpezy_encode_jpeg(ctx._h, rp[0], rp[1], rp[2], W, H, 0, c, p, 1 << 16)
        for name, rc in rcs.items():
            assert rc == BADARG, (name, rc)
        with pytest.raises(J.JpezyError, match="status -1.*JPEZY_MAX_COMMENT"):
            J.encode_batch_multi([0], r, g, b, W, H, 1, comment=c)
        with J.MultiEncoder([0], W, H) as Mh:
            with pytest.raises(J.JpezyError, match="status -1.*JPEZY_MAX_COMMENT"):
                Mh.encode(r, g, b, 1, comment=c)
    torch.cuda.synchronize()
    # the context is still good after the refusals
    assert ctx.write_jpeg_gpu(d, W, H) == [J.write_jpeg(co, W, H)]
