"""The GPU entropy coder's seams (jpezy_entropy.hip) in every MCU layout, table set and restart form: what
tests/test_gpu_entropy_seams.py and tests/test_gpu_restart.py build for 4:2:0 with the Annex-K tables, built here for 4:4:4 (3 coded
blocks per MCU, the tile border inside MCU 85) and 4:2:2 (4 blocks), under per-image Huffman tables (a flat block is 2 bits, a DC code
may be 12 bits and any AC code 16) and with restart intervals, down to intervals of ONE byte.  Every field is built bit-exactly by
tests/scan_model.py (proved equal to the host writer by tests/test_scan_model.py) and every construction asserts from the model that
it landed on its seam.  The expectation is always the host writer's file, byte for byte; for fields the Python model can walk it is
the model's file too.  Against it: write_jpeg_gpu (one frame and a batch whose every frame opens against predictors of 0),
write_jpeg_gpu_dev into marker-filled buffers (Annex K only: it refuses per-image tables) and huffman_histogram_dev.

The seams: the 140-byte LDS row and its licence (RowWriter) against the DirectWriter; blocks shorter than a word whose bits the owner
of a partial word pulls from up to fifteen following rows, at tile ends; 256-block tiles that never straddle a restart interval;
64-byte chunks and 16 KB pieces of the unstuffed stream U in the three assembling kernels; the stuffing kernel that places RSTn.

Coverage (K: Annex K, P: per-image tables; ri: with restart intervals; layouts 444 / 422 unless more are named):
  row limit 139 / 140 / 141 bytes, worst block, every table position    K            test_blocks_at_the_row_limit
  stream ends in word 34 / 1121 .. 1152 bits re-coded / 16-bit AC code  P, + 420, gray  test_blocks_at_the_row_limit_with_per_image_tables
  licence-only refusal, last lane and lane 0                            K, P, + 420, gray  test_block_refused_by_the_licence_alone
  sub-word run to block 255 / 256 / 257                                 K            test_short_blocks_end_at_tile_boundary
  2- and 4-bit blocks, 12 to a word, to block 255 / 256 / 257           P, + 420, gray  test_two_bit_blocks_end_at_tile_boundary
  run to the end of an interval whose last tile has 2 .. 14 blocks      K, P, ri, + 420, gray  test_short_run_ends_an_interval_whose_last_tile_is_short
  stream of 63 / 64 / 65 / 16383 / 16384 / 16385 bytes, 8L and 8L - 3    K            test_stream_lengths_on_chunk_and_piece_boundaries
  interval ends on byte 63 / 64 of a chunk, 16383 / 16384 of a piece    K, ri        test_interval_ends_on_chunk_and_piece_borders
  0xFF last / first byte of a chunk and a piece                         K            test_ff_byte_on_chunk_and_piece_edges
  FF 00 FF Dn on a chunk edge                                           K, ri        test_ff_as_the_last_data_byte_of_an_interval_on_a_chunk_edge
  category-11 DC chains over tiles, batch frames, interval starts       K, P, ri, + 420, gray (ri)  test_dc_chains_of_category_11
  one-byte intervals: flat, shifted output offsets, interleaved with FF P, ri = 1    test_restart_intervals_of_one_byte
  more than 2048 tiles                                                  P, ri = 0 and one MCU row  test_more_than_2048_tiles_with_per_image_tables
  whole tiles of worst blocks                                           K (all re-coded), P (in the rows), ri  test_whole_tiles_of_worst_blocks
Left empty on purpose: exact stream lengths and 0xFF edges under per-image tables (the tables move with every tuned block; the chunk and
piece arithmetic they exercise does not see the tables); 4:2:0 with Annex K where tests/test_gpu_entropy_seams.py and
tests/test_gpu_restart.py have the case; a two-byte interval ending in 0xFF (impossible: see test_restart_intervals_of_one_byte); a
whole tile re-coded under the frame's own tables (no optimal code keeps every block over sixteen bits a coefficient)."""
import hashlib
from functools import lru_cache

import numpy as np
import pytest

import scan_model as S

pytestmark = pytest.mark.gpu

NEW = ["444", "422"]                         # the layouts test_gpu_entropy_seams.py / test_gpu_restart.py never built a seam for
ALL = ["444", "422", "420", "420gray"]       # per-image tables and restart-specific items: 4:2:0 too
MODEL_BLOCKS = 6000                          # fields up to this many coded blocks are also compared with the model's file
MARK = 0xA5
CHUNK, PIECE = S.CHUNK, S.PIECE


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def ctxs(J):
    """{optimize: context}: Annex K, and per-image optimised tables"""
    plain, opt = J.Context(0), J.Context(0)
    opt.set_huffman_optimize(1)
    yield {False: plain, True: opt}
    plain.close()
    opt.close()


def _dev(frames):
    import torch
    return torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f, np.int16).reshape(-1) for f in frames]))).cuda()


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = next((i for i in range(n) if a[i] != b[i]), n)
    return dict(len_got=len(a), len_want=len(b), at=d, got=a[max(0, d - 4):d + 8].hex(), want=b[max(0, d - 4):d + 8].hex())


def _row(nmcu, layout):
    """(W, H) of a frame of nmcu MCUs in one MCU row"""
    return S.frame_size(nmcu, 1, layout)


def _expected(J, co, layout, W, H, ri, optimize, frames, tables, what):
    """(the host writer's file, the symbol counts) of every frame; the file is also the model's for fields it can walk"""
    L = S.LAYOUTS[layout]
    nmcu = S.mcus(co, L).shape[0]
    walkable = nmcu * L.coded <= MODEL_BLOCKS or ri == 1
    want, counts = [], []
    for k, f in enumerate(frames):
        if k and f is frames[0]:
            want.append(want[0]), counts.append(counts[0])
            continue
        w = J.write_jpeg(f, W, H, gray=L.gray, optimize=optimize, restart_interval=ri, sampling=L.sampling)
        if walkable:
            T = tables if (k == 0 and tables is not None) else (S.frame_tables(f, L, ri) if optimize else None)
            assert w == S.write_jpeg(f, W, H, L, T, ri), f"{what}: host writer != model, frame {k}"
            counts.append(S.symbol_counts(f, L, ri)[0])
        else:
            counts.append(None if L.gray else J.huffman_histogram(f, W, H, sampling=L.sampling, restart_interval=ri).astype(np.int64))
        assert len(w) <= J.jpeg_bound(W, H, L.sampling), what
        want.append(w)
    return want, counts


def _gpu_equals(ctx, frames, layout, W, H, ri, optimize, want, counts, what):
    """write_jpeg_gpu (one frame, batch), write_jpeg_gpu_dev into marker-filled buffers (Annex K), huffman_histogram_dev"""
    import torch
    L = S.LAYOUTS[layout]
    n = len(frames)
    ctx.set_restart_interval(ri)
    try:
        got = ctx.write_jpeg_gpu(_dev(frames[:1]), W, H, gray=L.gray, sampling=L.sampling)
        assert got[0] == want[0], (what, "write_jpeg_gpu, one frame", _first_difference(got[0], want[0]))
        d = _dev(frames)
        got = ctx.write_jpeg_gpu(d, W, H, gray=L.gray, n_frames=n, sampling=L.sampling)
        for k in range(n):
            assert got[k] == want[k], (what, "write_jpeg_gpu, batch", k, _first_difference(got[k], want[k]))
        if not optimize:
            stride = (max(len(w) for w in want) + 127) // 64 * 64
            d_out = torch.full((n, stride), MARK, dtype=torch.uint8, device="cuda")
            d_sz = torch.full((n,), -77, dtype=torch.int64, device="cuda")
            ctx.write_jpeg_gpu_dev(d, W, H, d_out, d_sz, gray=L.gray, n_frames=n, sampling=L.sampling)
            torch.cuda.synchronize()
            out, sz = d_out.cpu().numpy(), d_sz.cpu().numpy()
            for k in range(n):
                assert sz[k] == len(want[k]), (what, "write_jpeg_gpu_dev size", k, int(sz[k]), len(want[k]))
                assert out[k, :sz[k]].tobytes() == want[k], (what, "write_jpeg_gpu_dev", k, _first_difference(out[k, :sz[k]].tobytes(), want[k]))
                assert (out[k, sz[k]:] == MARK).all(), (what, "write_jpeg_gpu_dev wrote behind the file", k)
        hist = torch.full((n, 4, 256), -1, dtype=torch.int64, device="cuda")
        ctx.huffman_histogram_dev(d, W, H, hist, gray=L.gray, n_frames=n, sampling=L.sampling)
        torch.cuda.synchronize()
        hist = hist.cpu().numpy()
        for k in range(n):
            if counts[k] is not None:
                assert (hist[k] == counts[k]).all(), (what, "huffman_histogram_dev", k)
    finally:
        ctx.set_restart_interval(0)


def check_field(J, ctxs, co, layout, W, H, ri=0, optimize=False, frames=None, tables=None, what=""):
    """host writer (== the model for fields it can walk) == write_jpeg_gpu, one frame == write_jpeg_gpu, batch ==
    write_jpeg_gpu_dev (Annex K), and huffman_histogram_dev == the model's counts.  frames: the batch (default: the field twice)."""
    frames = [co, co] if frames is None else frames
    want, counts = _expected(J, co, layout, W, H, ri, optimize, frames, tables, what)
    _gpu_equals(ctxs[bool(optimize)], frames, layout, W, H, ri, optimize, want, counts, what)
    return want[0]


def _filler(i, layout, tables=None):
    """a long block (200 .. 228 bits, DC 0) for coded position i"""
    return S.block_of_bits(200 + 7 * (i % 5), 0, S.table_of(layout, i), None, tables)


def _put(co, layout, g, z):
    """z into coded block g of the frame (which must be a stored one)"""
    L = S.LAYOUTS[layout]
    assert S.is_stored(L, g), g
    co[g // L.coded, g % L.coded] = z


def _predecessor(layout, g):
    """the coded block whose DC predicts block g's (the previous block of the component), without restart intervals"""
    L = S.LAYOUTS[layout]
    m, i = divmod(g, L.coded)
    if i >= L.luma:
        return (m - 1) * L.coded + i
    return g - 1 if i >= 1 else (m - 1) * L.coded + L.luma - 1


# ---- 1. the in-place row against the DirectWriter ----
ROW_LENGTHS = [8 * 139 - 7, 8 * 139, 8 * 140 - 1, 8 * 140, 8 * 140 + 1, 8 * 141]


@lru_cache(maxsize=None)
def _row_limit_field(layout):
    """per table position of the MCU (each luma slot, Cb, Cr) eight consecutive MCUs: the six lengths, a DC of 1023 in the block
    that predicts the next one, and the worst block with a DC of -1023"""
    L = S.LAYOUTS[layout]
    per = len(ROW_LENGTHS) + 2
    nmcu = L.stored * per
    co = np.zeros((nmcu, L.stored, 64), np.int16)
    exact, worst = {}, []
    for i in range(L.stored):
        t = 0 if i < L.luma else 1
        for k, bits in enumerate(ROW_LENGTHS):
            g = (i * per + k) * L.coded + i
            _put(co, layout, g, S.block_of_bits(bits, 0, t))
            exact[g] = bits
        g = (i * per + per - 1) * L.coded + i
        _put(co, layout, g, S.worst_block(None, t, dc=-1023))
        _put(co, layout, _predecessor(layout, g), S.flat_block(1023))
        worst.append(g)
    co.setflags(write=False)
    return co, exact, worst


@pytest.mark.parametrize("layout", NEW)
def test_blocks_at_the_row_limit(J, ctxs, layout):
    """blocks of 139, 140 bytes (in the row), 141 bytes (re-coded) and the worst block after a category-11 DC step, side by side in
    one tile, at every table position of the layout: the lane's table is i < LUMA, its predictor zg[-(bpm - (LUMA - 1)) * 64]"""
    L = S.LAYOUTS[layout]
    co, exact, worst = _row_limit_field(layout)
    nmcu = co.shape[0]
    lens, verdicts = S.block_lengths(co, layout), S.block_verdicts(co, layout)
    assert S.tiles(nmcu, layout) == [(0, nmcu * L.coded)] and nmcu * L.coded <= 256
    for g, bits in exact.items():
        assert lens[g] == bits and verdicts[g] == ("row" if bits <= 8 * S.ROW_BYTES else "words"), (g, bits, int(lens[g]), verdicts[g])
    assert {g % L.coded for g in exact} == set(range(L.stored)) == {g % L.coded for g in worst}
    for g in worst:
        luma = S.table_of(layout, g) == 0
        assert lens[g] == ((9 + 11 + 63 * 26) if luma else (11 + 11 + 63 * 22)) and verdicts[g] != "row", (g, int(lens[g]))
    assert (int(lens[worst[0]]) + 7) // 8 == 208                      # kMaxBlockBytes
    check_field(J, ctxs, co, layout, *_row(nmcu, layout), what=f"row limit {layout}")


def _symbol_blocks(symbols):
    """blocks (DC 0) that emit the AC symbols [(run, size)] in order, as many per block as fit its 63 positions"""
    blocks, z, pos = [], np.zeros(64, np.int16), 0
    for run, size in symbols:
        if pos + run + 1 > 63:
            blocks.append(z)
            z, pos = np.zeros(64, np.int16), 0
        pos += run + 1
        z[pos] = (1 << size) - 1 if (pos + size) % 2 else -((1 << size) - 1)
    blocks.append(z)
    return blocks


RARE = (1, 2)                                  # the AC symbol (run, size) that occurs once in the frame


@lru_cache(maxsize=None)
def _ladder():
    """luma blocks whose AC symbols have the counts 1, 2, 3, 5, ... 144 (the rarest first): under the rarer symbols of the frame a
    Huffman tree as deep as it gets, so that the rarest symbols take the 16 bits Figure K.3 limits a code to"""
    symbols = []
    for k, n in enumerate((1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144)):
        symbols += [(k % 4 + 1, k // 4 + 2)] * n
    assert symbols[0] == RARE
    return _symbol_blocks(symbols)


def _mix(n1, n8, n9, n10):
    """a block of 63 coefficients in ascending order of cost (the long codes at the end, behind the reads)"""
    assert n1 + n8 + n9 + n10 == 63
    return S.ac_block([1] * n1 + [8] * n8 + [9] * n9 + [10] * n10)


@lru_cache(maxsize=None)
def _row_limit_image_field(layout):
    """per-image tables: luma blocks a (its stream ends in word 34, coded in the row), b (1121 .. 1152 bits, re-coded), a third that
    takes the rest of a fixed pool of 44 coefficients each of sizes 8, 9 and 10 -- so the frame's tables do not depend on how the
    pool is split --, the ladder with the frame's rarest symbol first, and a cascade of the sizes 7 .. 1, each twice as frequent as the one before, which
    puts the pool's codes at 9 or 10 bits.  The chroma blocks are flat.  Searched: the cascade's base count (n_ones), then the split."""
    L = S.LAYOUTS[layout]
    pool = 44

    def frame(n_ones, a, b):
        rest = [pool - a[k] - b[k] for k in range(3)]
        luma = [_mix(63 - sum(a), *a), _mix(63 - sum(b), *b), _mix(63 - sum(rest), *rest)] + _ladder()
        # the cascade above the pool: sizes 7, 6, ... 1, each twice as frequent as the one before, 63 coefficients a block
        sizes = [s for k, s in enumerate(range(7, 0, -1)) for _ in range(n_ones << k)]
        luma += [S.ac_block(sizes[o:o + 63], sign=1 - 2 * (o % 2)) for o in range(0, len(sizes), 63)]
        co = np.zeros((-(-len(luma) // L.luma), L.stored, 64), np.int16)
        for k, z in enumerate(luma):
            co[k // L.luma, k % L.luma] = z
        return co

    def lands(n_ones):
        tables = S.freeze(S.frame_tables(frame(n_ones, (22, 22, 19), (22, 22, 19)), layout))
        ac = S.codes(tables)[2]
        if ac[(RARE[0] << 4) | RARE[1]][1] != 16:
            return None
        splits = [(i, j, k) for i in range(14, 30) for j in range(14, 30) for k in range(10, 30) if 56 <= i + j + k <= 63]
        bits = lambda z: S.block_bits(z, 0, 0, tables)
        for a in splits:
            za = _mix(63 - sum(a), *a)
            if not (1089 <= bits(za) <= 1120 and S.fits_row(za, 0, 0, tables)):
                continue
            for b in splits:
                if any(a[k] + b[k] > pool for k in range(3)) or 3 * pool - sum(a) - sum(b) > 63:
                    continue
                zb = _mix(63 - sum(b), *b)
                if 1121 <= bits(zb) <= 1152 and not S.fits_row(zb, 0, 0, tables):
                    co = frame(n_ones, a, b)
                    assert S.freeze(S.frame_tables(co, layout)) == tables          # the split does not move the tables
                    return co, tables
        return None

    _, (co, tables) = S.search((100, 150, 200, 300), lands)
    gc = (3 // L.luma) * L.coded + 3 % L.luma                       # the first block of the ladder
    co.setflags(write=False)
    return co, tables, (0, (1 if L.luma > 1 else L.coded), gc)


@pytest.mark.parametrize("layout", ALL)
def test_blocks_at_the_row_limit_with_per_image_tables(J, ctxs, layout):
    """under the frame's own tables: a block whose stream ends in word 34 of its row and stays there, one of 1121 .. 1152 bits that is
    re-coded, and a block coded with a 16-bit AC code (Annex K has none over 16 either, but there the long codes are the rare runs)"""
    L = S.LAYOUTS[layout]
    co, tables, (ga, gb, gc) = _row_limit_image_field(layout)
    nmcu = co.shape[0]
    assert max(ga, gb, gc) < 256 and S.tile_of_block(nmcu, layout, 0, gc)[0] == 0
    assert max(n for _, n in S.codes(tables)[2].values()) == 16
    check_field(J, ctxs, co, layout, *_row(nmcu, layout), optimize=True, tables=tables, what=f"row limit, per-image tables {layout}")


def _licence_slots(layout):
    """(the last lane of tile 0, lane 0 of the first later tile whose first block is stored)"""
    first = next(g for g in (256, 512) if S.is_stored(layout, g))
    assert S.is_stored(layout, 255)
    return 255, first


CHAIN = [(1, 1), (1, 2), (2, 1)] + [(0, s) for s in range(9, 0, -1)]       # AC symbols (run, size) from rare to frequent


def _chain_blocks(c0):
    """blocks (DC 0) whose AC symbols have counts that grow like the Fibonacci numbers from c0 + 3 on, each at least the sum of all
    but the one before it: above a symbol that occurs c0 times (and the EOBs and the reserved code point beside it) the Huffman tree is
    one chain, and that symbol's code has 13 bits though it is not rarer than one in four hundred"""
    counts = [c0 + 3]
    for _ in CHAIN:
        counts.append(max(sum(counts[:-1]) + 2 if len(counts) > 1 else 0, counts[-1] + 1))
    blocks = _symbol_blocks([sym for sym, n in zip(CHAIN, counts[1:]) for _ in range(n)])
    for z in blocks:                   # no EOB (its count would stand in the chain's way): +-1, the most frequent symbol, up to position 63
        z[1 + int(np.flatnonzero(z)[-1]):] = 1
    return blocks


@lru_cache(maxsize=None)
def _licence_field(layout, per_image):
    """(field, its tables or None, the two slots).  Annex K: long blocks everywhere and in the slots the fewest leading -1023 the
    licence refuses.  Per-image tables: k leading -1023 in the slots, and in each table that has such a block a chain of symbols
    (_chain_blocks) that keeps the code of (0, 10) long; searched: k."""
    L = S.LAYOUTS[layout]
    slots = _licence_slots(layout)

    def lands(k):
        per_table = [sum(S.table_of(L, g) == t for g in slots) for t in (0, 1)]
        chains = [_chain_blocks(k * n) if per_image and n else [] for n in per_table]
        need = max([3 * 256 // L.coded + 1, -(-len(chains[0]) // L.luma) + 2, -(-len(chains[1]) // 2) + 2])
        co = np.zeros((need, L.stored, 64), np.int16)
        it = [iter(chains[0]), iter(chains[1])]
        for g in range(need * L.coded):
            if not S.is_stored(L, g):
                continue
            t = S.table_of(L, g)
            if g in slots:
                _put(co, layout, g, S.ac_block([10] * k, 0, -1) if per_image else S.licence_block(None, t))
            elif per_image:
                _put(co, layout, g, next(it[t], S.ac_block([1] * 63) if per_table[t] else S.flat_block()))
            else:
                _put(co, layout, g, _filler(g, layout))
        tables = S.freeze(S.frame_tables(co, layout)) if per_image else None
        verdicts, lens = S.block_verdicts(co, layout, tables), S.block_lengths(co, layout, tables)
        return (co, tables) if all(verdicts[g] == "licence" and lens[g] <= 8 * 80 for g in slots) else None

    _, (co, tables) = S.search((18, 20, 22, 24, 26, 28), lands)
    co.setflags(write=False)
    return co, tables, slots


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("layout", ALL)
def test_block_refused_by_the_licence_alone(J, ctxs, layout, per_image):
    """a block of at most 80 bytes -- leading +-1023, then zeros -- whose words come due before the coefficients under them are read:
    re-coded by the DirectWriter although it is far under the row's 140 bytes.  One as the last lane of a tile, one as lane 0."""
    co, tables, slots = _licence_field(layout, per_image)
    nmcu = co.shape[0]
    lens, verdicts = S.block_lengths(co, layout, tables), S.block_verdicts(co, layout, tables)
    for g, lane in zip(slots, (255, 0)):
        assert verdicts[g] == "licence" and lens[g] <= 8 * 80, (g, verdicts[g], int(lens[g]))
        assert S.tile_of_block(nmcu, layout, 0, g)[1] == lane
        z = S.mcus(co, layout)[g // S.LAYOUTS[layout].coded, g % S.LAYOUTS[layout].coded]
        assert np.count_nonzero(z[1:]) >= 10 and (np.abs(z[1:1 + np.count_nonzero(z[1:])]) == 1023).all()
    if not per_image:
        assert sum(v != "row" for v in verdicts) == 2           # (the chain's rarest symbols have long codes of their own)
    check_field(J, ctxs, co, layout, *_row(nmcu, layout), optimize=per_image, tables=tables, what=f"licence {layout} per_image={per_image}")


# ---- 2. blocks shorter than a word at tile ends ----
@pytest.mark.parametrize("layout", NEW)
@pytest.mark.parametrize("end", [255, 256, 257])
def test_short_blocks_end_at_tile_boundary(J, ctxs, layout, end):
    """long blocks, then a run of blocks shorter than 32 bits that ends at coded block `end` (255: the last lane of tile 0, 256: the
    first lane of tile 1 -- with 3-block MCUs a block inside MCU 85), then long blocks again"""
    L = S.LAYOUTS[layout]
    nmcu = 3 * 256 // L.coded
    start = 180
    co = np.zeros((nmcu, L.stored, 64), np.int16)
    for g in range(nmcu * L.coded):
        if not start <= g <= end:
            _put(co, layout, g, _filler(g, layout))
    lens = S.block_lengths(co, layout)
    assert (lens[start:end + 1] < 32).all() and lens[end + 1:end + 4].min() >= 32 and lens[start - 4:start].min() >= 32
    assert S.tile_of_block(nmcu, layout, 0, end) == (end // 256, end % 256)
    check_field(J, ctxs, co, layout, *_row(nmcu, layout), what=f"short run to {end} {layout}")


def _flat_run_field(layout, nmcu, start, end, tables_of=None):
    """all flat but four long blocks in front of the run [start, end] and four behind it (the nearest stored ones)"""
    L = S.LAYOUTS[layout]
    co = np.zeros((nmcu, L.stored, 64), np.int16)
    before = [g for g in range(start - 1, -1, -1) if S.is_stored(L, g)][:4]
    behind = [g for g in range(end + 1, nmcu * L.coded) if S.is_stored(L, g)][:4]
    for g in before + behind:
        _put(co, layout, g, S.ac_block([3, 2, 1, 4, 1, 2, 3, 1, 2, 1, 1, 5] + [1] * (g % 7)))
    return co, before, behind


def _words_of_whole_blocks(offsets, lens, first, count):
    """the most blocks of the tile [first, first + count) whose whole streams lie in one 32-bit word of the tile's stream"""
    base, by_word = int(offsets[first]), {}
    for g in range(first, first + count):
        o, n = int(offsets[g]) - base, int(lens[g])
        if n and o // 32 == (o + n - 1) // 32:
            by_word[o // 32] = by_word.get(o // 32, 0) + 1
    return max(by_word.values(), default=0)


def _deepest_pull(offsets, bitstrings, first, count):
    """the largest distance, in lanes, between the owner of a word of the tile's stream (the lane whose block holds the word's first
    bit) and a following lane that puts a ONE bit into that word: what the owner's tail completion has to reach"""
    base, deepest = int(offsets[first]), 0
    owner = {}
    for g in range(first, first + count):
        o, n = int(offsets[g]) - base, len(bitstrings[g])
        for w in range(-(-o // 32), (o + n - 1) // 32 + 1 if n else 0):
            owner.setdefault(w, g)                                   # the first block that reaches bit 32 w holds it
        if n and o % 32 and (o // 32) in owner and "1" in bitstrings[g][:32 - o % 32]:
            deepest = max(deepest, g - owner[o // 32])
    return deepest


@pytest.mark.parametrize("layout", ALL)
@pytest.mark.parametrize("end", [255, 256, 257])
def test_two_bit_blocks_end_at_tile_boundary(J, ctxs, layout, end):
    """per-image tables on a mostly flat field: both DC tables and both AC tables put their most frequent symbol in ONE bit, a flat
    block is 2 bits and sixteen whole blocks fit one word -- the owner of a partial word pulls from fifteen following rows (Annex K
    never goes past eight).  A one-bit code is a zero bit, so a flat block is `00` and would hide a row that was not pulled: every
    fourth block of the run steps its DC by +-1 and is the four bits `10 v 0` -- a word still holds twelve or thirteen whole blocks."""
    L = S.LAYOUTS[layout]
    nmcu = 3 * 256 // L.coded + 1
    start = 150
    co, before, behind = _flat_run_field(layout, nmcu, start, end)
    dc = [0, 0, 0]
    for g in range(nmcu * L.coded):                                  # the DC steps of the run; every later block keeps its component's DC
        if S.is_stored(L, g):
            comp = S.component(L, g % L.coded)
            dc[comp] ^= 1 if start <= g <= end and g % 4 == 3 else 0
            co[g // L.coded, g % L.coded, 0] = dc[comp]
    tables = S.freeze(S.frame_tables(co, layout))
    g = S.geometry(co, layout, tables)
    lens, bits = g.lengths, S.block_bitstrings(co, layout, tables)
    lo, hi = before[0] + 1, behind[0] - 1                  # the run as it is: the short blocks between the long ones
    # (gray: the two zero chroma blocks behind a luma block 3 are coded flat as well, so there the run ends with them)
    assert lo <= start and end <= hi <= end + 2 and (hi == end or L.gray)
    assert set(int(n) for n in lens[lo:hi + 1]) == {2, 4} and all(lens[b] >= 32 for b in before + behind)
    assert S.tile_of_block(nmcu, layout, 0, end) == (end // 256, end % 256)        # 255: the run's last block is the tile's last lane
    assert _words_of_whole_blocks(g.offsets, lens, 0, 256) >= 10
    assert _deepest_pull(g.offsets, bits, 0, 256) >= 9                             # a one bit from beyond the eighth following lane
    check_field(J, ctxs, co, layout, *_row(nmcu, layout), optimize=True, tables=tables, what=f"2-bit run to {end} {layout}")


@pytest.mark.parametrize("per_image", [False, True])
@pytest.mark.parametrize("layout,ri", [("444", 86), ("444", 90), ("422", 65), ("422", 67), ("420", 43), ("420", 45), ("420gray", 45)])
def test_short_run_ends_an_interval_whose_last_tile_is_short(J, ctxs, layout, ri, per_image):
    """the same run ending at the LAST block of a restart interval whose last tile holds fewer than 16 blocks (2 .. 14): every
    block of that tile is shorter than a word, and so is the whole tile"""
    L = S.LAYOUTS[layout]
    bpi = ri * L.coded
    assert 0 < bpi - 256 < 16
    nmcu = 2 * ri + 3
    co = np.zeros((nmcu, L.stored, 64), np.int16)
    long_block = lambda g: S.ac_block([3, 2, 1, 4, 1, 2, 3, 1, 2, 1, 1, 5] + [1] * (g % 7)) if per_image else _filler(g, layout)
    run = 41                                                   # the interval's last 41 blocks are flat
    for iv in (0, 1):
        end = (iv + 1) * bpi
        # Annex K: long blocks up to the run; per-image tables: a mostly flat field (a flat block is 2 bits) with long blocks only in the
        # six positions in front of the run
        for g in range(iv * bpi if not per_image else end - run - 6, end - run):
            if S.is_stored(L, g):
                _put(co, layout, g, long_block(g))
    for g in range(2 * bpi, nmcu * L.coded):
        if S.is_stored(L, g):
            _put(co, layout, g, S.ac_block([2, 1, 1, 3]))
    tables = S.freeze(S.frame_tables(co, layout, ri)) if per_image else None
    g = S.geometry(co, layout, tables, ri)
    assert g.tiles[:4] == [(0, 256), (256, bpi - 256), (bpi, 256), (bpi + 256, bpi - 256)]
    for end in (bpi, 2 * bpi):
        assert (g.lengths[end - run:end] < 32).all() and g.lengths[end - run - 6:end - run].max() >= 32
        if per_image:
            assert (g.lengths[end - run:end] == 2).all()
    assert g.tile_bits[1] == g.lengths[256:bpi].sum() < (32 if per_image else 128) and g.tile_bits[3] == g.tile_bits[1]
    check_field(J, ctxs, co, layout, *_row(nmcu, layout), ri=ri, optimize=per_image, tables=tables, what=f"short run to interval end {layout} ri={ri}")


# ---- 3. stream lengths around 64-byte chunks and 16 KB pieces ----
@pytest.mark.parametrize("layout", NEW)
@pytest.mark.parametrize("nbytes", [63, 64, 65, PIECE - 1, PIECE, PIECE + 1])
def test_stream_lengths_on_chunk_and_piece_boundaries(J, ctxs, layout, nbytes):
    for total in (8 * nbytes, 8 * nbytes - 3):
        co = S.frame_of_bits(total, layout)
        assert co is not None, (layout, total)
        nmcu = co.shape[0]
        stream = S.unstuffed_stream(co, layout)
        assert len(stream) == nbytes and S.geometry(co, layout).stream_bits == total
        jpg = check_field(J, ctxs, co, layout, *_row(nmcu, layout), what=f"L={nbytes} bits={total} {layout}")
        assert S.M.scan_of(jpg) == stream


@pytest.mark.parametrize("layout", NEW)
@pytest.mark.parametrize("nbytes", [64, 65, PIECE, PIECE + 1])
def test_interval_ends_on_chunk_and_piece_borders(J, ctxs, layout, nbytes):
    """a first restart interval of exactly `nbytes`: its last byte is the last byte of a chunk / piece (the marker behind the border
    byte) or the first byte of the next (in front of it), with and without pad bits.  Flat intervals follow; where the first is one
    MCU they are two (4:4:4) or three bytes each, 32 or 21 markers to a chunk: the RSTn numbers wrap past 7 inside one chunk."""
    L = S.LAYOUTS[layout]
    for total in (8 * nbytes, 8 * nbytes - 3):
        first = S.frame_of_bits(total, layout)
        ri = first.shape[0]
        more = 70 if ri == 1 else 3
        co = np.concatenate([first, np.zeros((ri * more, L.stored, 64), np.int16)])
        nmcu = co.shape[0]
        parts = S.unstuffed_intervals(co, layout, None, ri)
        assert len(parts) == more + 1 and len(parts[0]) == nbytes
        marks, extra = S.chunk_stats(co, layout, None, ri)
        assert marks[(nbytes - 1) // CHUNK] >= 1 and marks.sum() == more
        if ri == 1:
            flat = {"444": 2, "422": 3}[layout]                 # 14 and 20 bits with the Annex-K tables
            assert {len(p) for p in parts[1:]} == {flat} and marks.max() >= 64 // flat > 8 and extra.max() >= 2 * marks.max()
        want = check_field(J, ctxs, co, layout, *_row(nmcu, layout), ri=ri, what=f"interval of {nbytes} bytes, bits={total} {layout}")
        assert S.RM.markers(S.RM.split(want)[1]) == S.RM.expected_markers(nmcu, ri)


# ---- 4. 0xFF bytes on the chunk and piece edges ----
@pytest.mark.parametrize("layout", NEW)
@pytest.mark.parametrize("P", [CHUNK - 1, CHUNK, PIECE - 1, PIECE])
def test_ff_byte_on_chunk_and_piece_edges(J, ctxs, layout, P):
    """an 0xFF as the last / first byte of a 64-byte chunk and of a 16 KB piece: a prefix of exactly the right length in front of a
    dense luma block, whose code has runs of 21 one bits"""
    L = S.LAYOUTS[layout]
    dense = S.block_bitstring(S.dense_block(), 0, 0)
    for o in (o for o in range(len(dense) - 8) if dense[o:o + 8] == "11111111"):
        prefix = 8 * P - o
        pre = S.frame_of_bits(prefix, layout) if prefix >= 200 else None
        if pre is None:
            continue
        m = pre.shape[0]
        co = np.zeros((m + 2, L.stored, 64), np.int16)
        co[:m] = pre
        co[m, 0] = S.dense_block()
        stream = S.unstuffed_stream(co, layout)
        assert stream[P] == 0xFF and int(S.block_lengths(co, layout)[:L.coded * m].sum()) == prefix
        check_field(J, ctxs, co, layout, *_row(m + 2, layout), what=f"0xFF at {P} {layout}")
        return
    raise AssertionError("no offset of the dense block puts an 0xFF there")


@pytest.mark.parametrize("layout", NEW)
@pytest.mark.parametrize("nbytes", [2 * CHUNK, 2 * CHUNK + 1])
def test_ff_as_the_last_data_byte_of_an_interval_on_a_chunk_edge(J, ctxs, layout, nbytes):
    """an interval that ends, on a byte, in ten one bits (its last block's last coefficient is 1023 at position 63): FF 00 FF Dn, the
    0xFF being the last byte of a chunk (nbytes = 128) or the first byte of the next (129)"""
    L = S.LAYOUTS[layout]
    tail = np.zeros((1, L.stored, 64), np.int16)
    tail[0, L.stored - 1, 63] = 1023
    first = S.frame_of_bits(8 * nbytes - int(S.block_lengths(tail, layout).sum()), layout)
    assert first is not None
    head = np.concatenate([first, tail])
    ri = head.shape[0]
    other = np.zeros((ri, L.stored, 64), np.int16)
    co = np.concatenate([head, other, head, other])
    parts = S.unstuffed_intervals(co, layout, None, ri)
    assert len(parts) == 4 and len(parts[0]) == nbytes and parts[0][-1] == 0xFF and parts[2][-1] == 0xFF
    assert (nbytes - 1) % CHUNK in (CHUNK - 1, 0)
    want = check_field(J, ctxs, co, layout, *_row(co.shape[0], layout), ri=ri, what=f"FF 00 FF Dn at {nbytes} {layout}")
    seg = S.RM.split(want)[1]
    assert seg.count(b"\xff\x00\xff\xd0") == 1 and seg.count(b"\xff\x00\xff\xd2") == 1


# ---- 5. DC prediction across tiles, frames and interval starts ----
def _dc_chain_field(layout, nmcu):
    """category-11 chains in every component, each with its own values: Y +-1023 from block to block, Cb -1021 / +1023 and
    Cr +1022 / -1022 from MCU to MCU -- a predictor taken from another component's block, or another block of the component, gives
    another difference"""
    L = S.LAYOUTS[layout]
    co = np.zeros((nmcu, L.stored, 64), np.int16)
    co[:, :L.luma, 0] = np.where(np.arange(nmcu * L.luma) % 2 == 0, 1023, -1023).reshape(nmcu, L.luma)
    if L.stored > L.luma:
        co[:, L.luma, 0] = np.where(np.arange(nmcu) % 2 == 0, -1021, 1023)
        co[:, L.luma + 1, 0] = np.where(np.arange(nmcu) % 2 == 0, 1022, -1022)
    co[::7, :, 5] = 3
    return co


@pytest.mark.parametrize("layout,ri", [("444", 0), ("444", 85), ("444", 86), ("422", 0), ("422", 63), ("422", 65), ("420", 43), ("420gray", 43)])
def test_dc_chains_of_category_11(J, ctxs, layout, ri):
    """the chains cross both tile borders of a three-tile frame, the frames of a batch (every frame opens against 0) and interval
    starts; 4:4:4 with ri = 85 / 86: an interval of 255 / 258 blocks, so the intervals start one block before / two blocks behind a
    256-block border of the frame and the predictor address crosses it"""
    L = S.LAYOUTS[layout]
    nmcu = 2 * 256 // L.coded + 6
    assert len(S.tiles(nmcu, layout)) == 3
    co = _dc_chain_field(layout, nmcu)
    cats = {}
    for k, (z, pred, t) in enumerate(S.coded_blocks(co, layout, ri)):
        if z is not None:
            cats.setdefault(S.component(L, k % L.coded), []).append(S.M.category(int(z[0]) - pred))
    starts = len(S.intervals(nmcu, ri))
    for comp, c in cats.items():                                   # category 10 only against the 0 an interval opens with
        assert set(c) <= {10, 11} and c.count(10) <= starts and c.count(11) >= len(c) - starts, (comp, set(c))
    if ri:
        assert any(f % 256 for f, _ in S.tiles(nmcu, layout, ri)[1:])      # intervals that start off the frame's 256-block borders
    W, H = _row(nmcu, layout)
    check_field(J, ctxs, co, layout, W, H, ri=ri, frames=[co, -co, co], what=f"DC chains {layout} ri={ri}")
    check_field(J, ctxs, co, layout, W, H, ri=ri, optimize=True, frames=[co, -co], what=f"DC chains, per-image tables {layout} ri={ri}")


# ---- 6. restart intervals of one byte ----
ONE_BYTE_FRAME = (128, 257)         # MCU columns, rows: two whole 16 KB pieces of one-byte intervals and part of a third


@lru_cache(maxsize=None)
def _shifted_head(layout):
    """the first two MCUs of the `shifted` variant: not flat, so that the pieces behind them start at other output offsets -- searched
    so that, in the expected file, the first output byte of at least one piece lies on a multiple of 4 and that of another does not"""
    L = S.LAYOUTS[layout]
    cols, rows = ONE_BYTE_FRAME

    def family():
        for a in ((5, -3, 1), (5, 0, 0), (300, -3, 1), (1023, 1023, 5), (7, 7, 7)):
            for b in (-2, 0, 90):
                head = np.zeros((2, L.stored, 64), np.int16)
                head[0, 0, 1:4] = a
                head[1, L.stored - 1, 2] = b
                yield head

    def lands(head):
        co = np.zeros((cols * rows, L.stored, 64), np.int16)
        co[:2] = head
        tables = S.frame_tables(co, layout, 1)
        _, extra = S.chunk_stats_of(S.unstuffed_intervals(co, layout, tables, 1))
        hdr = len(S.header(*S.frame_size(cols, rows, layout), layout, tables, 1))
        at = [(hdr + o) % 4 for o in S.piece_output_offsets(extra)]
        return 0 in at and any(at)

    return S.search(family(), lands)[0]


@pytest.mark.parametrize("layout", NEW)
@pytest.mark.parametrize("variant", ["flat", "shifted", "interleaved"])
def test_restart_intervals_of_one_byte(J, ctxs, layout, variant):
    """Flat content under its own tables is 6 bits an MCU in 4:4:4 and 8 bits in 4:2:2: with one MCU per interval every interval is
    ONE byte of the unstuffed stream, a 64-byte chunk carries 64 markers (`marks` all ones, 128 bytes added) and a whole 16 KB piece
    fills the stuffing kernel's staging buffer to exactly 256 x 192 bytes.
    shifted: the first intervals are not flat, so that later pieces start at an output offset that is no multiple of 4.
    interleaved: every third interval ends in 0xFF.  Two bytes cannot: in front of the eight one bits (value bits: every code holds a
    zero bit) stand the codes of every block of the MCU, nine of them at the least (DC and EOB of the blocks in front, DC, three
    ZRL and the coefficient's code in the last) -- so these are the three-byte intervals `xx xx FF`, coded `xx xx FF 00 FF Dn`."""
    L = S.LAYOUTS[layout]
    cols, rows = ONE_BYTE_FRAME
    nmcu = cols * rows
    W, H = S.frame_size(cols, rows, layout)
    co = np.zeros((nmcu, L.stored, 64), np.int16)
    if variant == "shifted":
        co[:2] = _shifted_head(layout)
    if variant == "interleaved":
        found = _interleaved_ff_mcu(layout)
        co[::3] = found
    tables = S.freeze(S.frame_tables(co, layout, 1))
    parts = S.unstuffed_intervals(co, layout, tables, 1)
    marks, extra = S.chunk_stats_of(parts)
    per = PIECE // CHUNK
    if variant == "flat":
        assert {len(p) for p in parts} == {1} and len(parts) == nmcu == 2 * PIECE + 128
        assert b"".join(parts[:70]) == bytes(70) and 0xFF not in b"".join(parts)
        assert (marks[:2 * per] == 64).all() and (extra[:2 * per] == 128).all() and marks[2 * per:].sum() == 127
    elif variant == "shifted":
        assert len(parts[0]) > 1 and {len(p) for p in parts[2:]} == {1}
        assert (marks[per:2 * per] == 64).all() and (extra[per:2 * per] == 128).all()
    else:
        assert sorted({len(p) for p in parts}) == [1, 3] and all(p[-1] == 0xFF for p in parts[::3]) and len(b"".join(parts)) > 2 * PIECE
        assert all(0xFF not in p for p in parts[1::3]) and int(extra.max()) >= 64 + 21
    want = check_field(J, ctxs, co, layout, W, H, ri=1, optimize=True, frames=[co], tables=tables, what=f"one-byte intervals {variant} {layout}")
    hdr, seg = S.RM.split(want)
    offs = [len(hdr) + o for o in S.piece_output_offsets(extra)]
    assert len(offs) >= 3 and len(seg) == len(b"".join(parts)) + int(extra.sum())
    if variant == "flat":
        assert seg[:9] == bytes.fromhex("00ffd000ffd100ffd2") and [o - offs[0] for o in offs[:3]] == [0, 3 * PIECE, 6 * PIECE]
    if variant == "shifted":
        # of the pieces' first output bytes in the file at least one lies on a multiple of 4 and one does not
        assert 0 in [o % 4 for o in offs] and any(o % 4 for o in offs), offs


@lru_cache(maxsize=None)
def _interleaved_ff_mcu(layout):
    """an MCU that, as every third of a flat frame coded with the frame's own tables and one MCU per interval, takes exactly three
    bytes of which the last is 0xFF, while the flat MCUs still take one byte: searched over the last coefficient's size and the DC /
    first coefficient of the first block (which move the length by single bits)"""
    L = S.LAYOUTS[layout]

    def family():
        for size in (8, 9, 10):
            for dc in (0, 1, -2, 5, -9):
                for a1 in (0, 1, -2, 4):
                    mcu = np.zeros((L.stored, 64), np.int16)
                    mcu[L.stored - 1, 63] = (1 << size) - 1
                    mcu[0, 0], mcu[0, 1] = dc, a1
                    yield mcu

    def lands(mcu):
        co = np.zeros((66, L.stored, 64), np.int16)
        co[::3] = mcu
        tables = S.frame_tables(co, layout, 1)
        parts = S.unstuffed_intervals(co[:3], layout, tables, 1)
        bits = S.interval_bits(co[:3], layout, tables, 1)
        return bits[0] == 24 and parts[0][-1] == 0xFF and len(parts[1]) == 1 and len(parts[2]) == 1

    mcu, _ = S.search(family(), lands)
    return mcu


# ---- 7. more than 2048 tiles with per-image tables ----
@pytest.mark.parametrize("layout,cols,rows", [("444", 420, 420), ("422", 245, 535)])
@pytest.mark.parametrize("restart", [False, True])
def test_more_than_2048_tiles_with_per_image_tables(J, ctxs, layout, cols, rows, restart):
    """4:4:4 at 3360 x 3360 (2068 tiles) and the smallest 4:2:2 frame past 2048 tiles (3920 x 4280: 131075 MCUs, 2049 tiles): the
    tile-bases path with the wide window of one-bit codes (assemble_kernel<false, ASM_WIN_ANY>), which these layouts reach at a quarter
    and a half of 4:2:0's pixels; a flat frame and a sparse one in one batch, each with its own tables; ri = one MCU row as well.
    The host writer's files, compared by length and SHA-256."""
    import torch
    L = S.LAYOUTS[layout]
    W, H = S.frame_size(cols, rows, layout)
    nmcu = cols * rows
    ri = cols if restart else 0
    # (131073 and 131074 MCUs, the fewest past 2048 tiles of 4:2:2, have no factorisation within 65535 pixels a side)
    assert -(-nmcu * L.coded // 256) == {"444": 2068, "422": 2049}[layout]
    if restart:
        assert len(S.tiles(nmcu, layout, ri)) > 2048
    rng = np.random.default_rng(cols)
    flat = np.zeros((nmcu, L.stored, 64), np.int16)
    flat[:, :, 0] = 21
    sparse = np.zeros((nmcu, L.stored, 64), np.int16)
    sparse[:, :, 0] = rng.integers(-60, 61, (nmcu, L.stored))
    k = rng.integers(1, 64, (nmcu, L.stored, 2))
    np.put_along_axis(sparse, k, (rng.integers(-9, 10, k.shape) * (rng.random(k.shape) < 0.2)).astype(np.int16), axis=2)
    sparse[-1, -1, 1:] = 1023
    ctx = ctxs[True]
    ctx.set_restart_interval(ri)
    try:
        d = _dev([flat, sparse])
        got = ctx.write_jpeg_gpu(d, W, H, n_frames=2, sampling=L.sampling)
        hist = torch.full((2, 4, 256), -1, dtype=torch.int64, device="cuda")
        ctx.huffman_histogram_dev(d, W, H, hist, n_frames=2, sampling=L.sampling)
        torch.cuda.synchronize()
        hist = hist.cpu().numpy()
    finally:
        ctx.set_restart_interval(0)
    for f, co in enumerate((flat, sparse)):
        want = J.write_jpeg(co, W, H, optimize=True, restart_interval=ri, sampling=L.sampling)
        assert len(got[f]) == len(want) and hashlib.sha256(got[f]).digest() == hashlib.sha256(want).digest(), (layout, restart, f, _first_difference(got[f], want))
        assert (hist[f] == J.huffman_histogram(co, W, H, sampling=L.sampling, restart_interval=ri).astype(np.int64)).all(), (layout, restart, f)
    assert len(got[0]) < len(got[1])


# ---- 8. whole tiles of worst blocks ----
@pytest.mark.parametrize("layout", NEW)
@pytest.mark.parametrize("restart", [False, True])
def test_whole_tiles_of_worst_blocks(J, ctxs, layout, restart):
    """two full tiles and a ragged third in which EVERY block is re-coded by the DirectWriter -- dense +-1023 blocks with alternating
    +-1023 DCs: what TILE_STREAM_WORDS and stream_stride are sized for -- and the file within jpeg_bound.  Under the frame's own
    tables the same field is the longest there is as well, 63 x 11 bits a block: one AC symbol, coded in one bit (no optimal code
    keeps a whole tile over sixteen bits a coefficient, which is what the row refuses), so there it fills the rows instead."""
    L = S.LAYOUTS[layout]
    nmcu = 600 // L.coded
    ri = 300 // L.coded if restart else 0                      # intervals of 300 blocks: a full tile and one of 44, twice
    co = _dc_chain_field(layout, nmcu)                          # every component's DC alternates: differences of category 11
    for g in range(nmcu * L.coded):
        co[g // L.coded, g % L.coded, 1:] = 1023 if g % 3 else -1023
    verdicts, lens = S.block_verdicts(co, layout, None, ri), S.block_lengths(co, layout, None, ri)
    tl = S.tiles(nmcu, layout, ri)
    assert all(v != "row" for v in verdicts), [k for k, v in enumerate(verdicts) if v == "row"][:8]
    assert lens.min() >= 63 * 22 and lens.max() == 9 + 11 + 63 * 26                     # chroma at its longest, luma at its
    assert [c for _, c in tl] == ([256, 44, 256, 44] if restart else [256, 256, 88])
    W, H = _row(nmcu, layout)
    want = check_field(J, ctxs, co, layout, W, H, ri=ri, what=f"worst tiles {layout} ri={ri}")
    assert len(want) <= J.jpeg_bound(W, H, L.sampling)
    tables = S.freeze(S.frame_tables(co, layout, ri))
    assert all(v == "row" for v in S.block_verdicts(co, layout, tables, ri))
    check_field(J, ctxs, co, layout, W, H, ri=ri, optimize=True, tables=tables, what=f"worst tiles, per-image tables {layout} ri={ri}")
