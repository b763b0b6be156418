"""tests/scan_model.py against the host writer, the host histogram and the four older models, before it is used to build the fields
of tests/test_gpu_entropy_layout_seams.py; and every builder against what it promises (exact bits, the row verdict and its reason).
No GPU: the host library only."""
import numpy as np
import pytest

import entropy_model as M
import huffopt_model as HM
import restart_model as RM
import sampling422_model as S2
import sampling_model as SM
import scan_model as S
from test_entropy_model import _random_field

LAYOUTS = ["420", "420gray", "444", "422"]
NMCU = 8
INTERVALS = [0, 1, 5, 3]            # 5: intervals of 5 and 3 MCUs; 3: a last interval of 2


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _field(layout, seed):
    L = S.LAYOUTS[layout]
    return _random_field(np.random.default_rng(1000 * seed + L.coded + L.stored), NMCU, L.stored)


def _size(layout):
    return S.frame_size(NMCU, 1, layout)


# ---- the model is the host writer ----
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_file_equals_host_writer(J, layout, optimize):
    L = S.LAYOUTS[layout]
    W, H = _size(layout)
    for seed in range(2):
        co = _field(layout, seed)
        for ri in INTERVALS:
            want = J.write_jpeg(co, W, H, gray=L.gray, comment=b"seam", optimize=optimize, restart_interval=ri, sampling=L.sampling)
            got = S.write_jpeg(co, W, H, layout, ri=ri, comment=b"seam", optimize=optimize)
            assert got == want, (layout, optimize, seed, ri)
            # the stuffed scan is U with 0xFF00 and the markers put in: the chunk statistics add up to the difference
            tabs = S.frame_tables(co, layout, ri) if optimize else None
            U = S.unstuffed_stream(co, layout, tabs, ri)
            marks, extra = S.chunk_stats(co, layout, tabs, ri)
            assert len(RM.split(want)[1]) == len(U) + int(extra.sum())
            assert int(marks.sum()) == len(S.intervals(NMCU, ri)) - 1
            g = S.geometry(co, layout, tabs, ri)
            assert (g.stream_bits + 7) // 8 == len(U)


@pytest.mark.parametrize("layout", ["420", "444", "422"])
def test_counts_equal_host_histogram(J, layout):
    L = S.LAYOUTS[layout]
    W, H = _size(layout)
    co = _field(layout, 2)
    for ri in INTERVALS:
        hist, ok = S.symbol_counts(co, layout, ri)
        assert ok
        assert (J.huffman_histogram(co, W, H, sampling=L.sampling, restart_interval=ri).astype(np.int64) == hist).all(), (layout, ri)


# ---- and it is each older model where their domains overlap ----
@pytest.mark.parametrize("gray", [False, True])
def test_equals_entropy_and_restart_models(gray):
    layout = "420gray" if gray else "420"
    co = _field(layout, 3)
    assert (S.block_lengths(co, layout) == M.block_lengths(co, gray)).all()
    assert "".join(S.block_bitstrings(co, layout)) == M.frame_bitstring(co, gray)
    assert S.unstuffed_stream(co, layout, pad_bit=0) == M.unstuffed_stream(co, gray)
    for (z, p, t), (z2, p2, t2) in zip(S.coded_blocks(co, layout), M.coded_blocks(co, gray)):
        assert (p, t) == (p2, t2) and S.fits_row(z, p, t) == M.fits_row(z2, p2, t2)
    assert (S.symbol_counts(co, layout)[0] == HM.symbol_counts(co, gray)[0]).all()
    for ri in INTERVALS[1:]:
        tabs = RM.frame_tables(co, ri, gray)
        assert S.frame_tables(co, layout, ri) == tabs
        for T in (None, tabs):
            assert S.scan(co, layout, T, ri) == RM.scan(co, ri, gray, T)
            assert S.interval_bits(co, layout, T, ri) == RM.interval_bits(co, ri, gray, T)
            assert S.unstuffed_intervals(co, layout, T, ri) == RM.unstuffed_intervals(co, ri, gray, T)


@pytest.mark.parametrize("layout,model", [("444", SM), ("422", S2)])
def test_equals_sampling_models(layout, model):
    W, H = _size(layout)
    co = _field(layout, 4)
    for ri in INTERVALS:
        assert (S.symbol_counts(co, layout, ri)[0] == model.symbol_counts(co, ri)[0]).all()
        for optimize in (False, True):
            assert S.write_jpeg(co, W, H, layout, ri=ri, comment=b"c", optimize=optimize) == model.write_jpeg(co, W, H, b"c", None, ri, optimize)


# ---- the geometry ----
def test_tiles_never_straddle_an_interval():
    # 4:4:4, 86 MCUs an interval: 258 blocks, a full tile and one of two blocks; the frame's last interval is shorter
    assert S.tiles(200, "444", 86) == [(0, 256), (256, 2), (258, 256), (514, 2), (516, 84)]
    assert S.tiles(200, "444", 0) == [(0, 256), (256, 256), (512, 88)] == S.tiles(200, "444", 200)      # one interval: the plain tiles
    assert S.restart_tpi(85, "444") == 1 and S.restart_tpi(86, "444") == 2 and S.restart_tpi(64, "422") == 1
    assert S.tile_of_block(200, "444", 86, 257) == (1, 1) and S.tile_of_block(200, "444", 86, 258) == (2, 0)
    for layout in LAYOUTS:
        for ri in (0, 1, 7, 43, 64, 100):
            tl = S.tiles(100, layout, ri)
            assert sum(c for _, c in tl) == 100 * S.LAYOUTS[layout].coded and all(0 < c <= 256 for _, c in tl)
            assert [f for f, _ in tl] == sorted(f for f, _ in tl)


def test_geometry_offsets_hold_the_pads():
    co = _field("422", 5)
    for ri in (0, 3):
        g = S.geometry(co, "422", None, ri)
        bits = "".join(format(b, "08b") for b in S.unstuffed_stream(co, "422", None, ri))
        blocks = S.block_bitstrings(co, "422", None, ri)
        for o, s in zip(g.offsets, blocks):
            assert bits[o:o + len(s)] == s
        assert g.tile_offsets == [int(g.offsets[f]) for f, _ in g.tiles]


# ---- the builders land on what they promise ----
def _image_tables(layout):
    """per-image tables of a field rich enough to have every category"""
    L = S.LAYOUTS[layout]
    rng = np.random.default_rng(77)
    co = rng.integers(-1023, 1024, (24, L.stored, 64)).astype(np.int16)
    co[..., 1:] >>= rng.integers(0, 11, (24, L.stored, 63)).astype(np.int16)
    co[:8, :, 0] = 0                                                       # DC differences of 0 ...
    co[8:16, :, 0] = np.where(np.arange(8) % 2 == 0, 1023, -1023)[:, None]  # ... and of category 11, in every component
    return S.frame_tables(co, layout)


@pytest.mark.parametrize("per_image", [False, True])
def test_blocks_of_exact_bits_and_their_verdict(per_image):
    tables = _image_tables("444") if per_image else None
    for t in (0, 1):
        for pred, dc in ((0, 0), (1023, -1023)):
            # (these per-image tables code a run-0 coefficient in at most 15 bits: no such block is longer than 63 x 15 bits)
            for bits in (333, 511, 700, 901) if per_image else (8 * 139 - 7, 8 * 139, 8 * 140 - 1, 8 * 140, 8 * 140 + 1, 8 * 141, 900, 333):
                z = S.block_of_bits(bits, pred, t, dc, tables)
                assert z is not None, (per_image, t, bits)
                assert S.block_bits(z, pred, t, tables) == bits
                assert S.row_verdict(z, pred, t, tables) == ("row" if bits <= 8 * S.ROW_BYTES else "words"), (per_image, t, bits)
        for bits in (8, 13, 21, 30):
            z = S.tuner_block(bits, t, tables)
            assert z is None or S.block_bits(z, 0, t, tables) == bits
        assert any(S.tuner_block(bits, t, tables) is not None for bits in range(8, 32))


def test_worst_block_is_the_bound_of_the_scratch():
    for t in (0, 1):
        z = S.worst_block(None, t)
        assert (np.abs(z[1:]) == 1023).all()
        assert S.block_bits(z, 1023, t) == ((9 + 11 + 63 * 26) if t == 0 else (11 + 11 + 63 * 22)) <= M.WORST_BLOCK_BITS
        assert S.row_verdict(z, 1023, t) == "licence"            # its words come due long before the coefficients under them are read


def test_licence_only_refusal():
    """ten or more leading +-1023 and nothing else: a word is due before the coefficients under it are read, at under 80 bytes"""
    # per-image tables in which (0, 10) has a long code: counts that grow like the Fibonacci numbers above it make the Huffman tree one
    # chain (where a large value is frequent, as in _image_tables, it costs 15 bits, and no word comes due ahead of two coefficients)
    ac, dc = np.zeros(256, np.int64), np.zeros(256, np.int64)
    ac[0x00], ac[0x0A] = 2, 20
    counts = [25]
    for sym in [0x11, 0x12, 0x21] + list(range(9, 0, -1)):
        counts.append(max(sum(counts[:-1]) + 2 if len(counts) > 1 else 0, counts[-1] + 1))
        ac[sym] = counts[-1]
    dc[0], dc[1] = 100, 10
    sparse = [HM.optimal_table(dc)[:2]] * 2 + [HM.optimal_table(ac)[:2]] * 2
    assert S.codes(sparse)[2][0x0A][1] == 13
    assert S.licence_block(_image_tables("422"), 0) is None
    for tables in (None, sparse):
        for t in (0, 1):
            z = S.licence_block(tables, t)
            assert z is not None and np.count_nonzero(z[1:]) >= 10 and (z[1 + np.count_nonzero(z[1:]):] == 0).all()
            assert S.block_bits(z, 0, t, tables) <= 8 * 80 and S.row_verdict(z, 0, t, tables) == "licence"
            z[np.count_nonzero(z[1:])] = 0                            # one coefficient fewer: coded in the row
            assert S.row_verdict(z, 0, t, tables) == "row"


@pytest.mark.parametrize("layout", LAYOUTS)
def test_frames_of_exact_bits(layout):
    for ri in (0, 2):
        for total in (8 * 63, 8 * 64 - 3, 8 * 65, 4000 - 3):
            co = S.frame_of_bits(total, layout, None, ri)
            assert co is not None, (layout, ri, total)
            g = S.geometry(co, layout, None, ri)
            assert g.stream_bits == total and len(S.unstuffed_stream(co, layout, None, ri)) == (total + 7) // 8
            assert (co[..., 0] == 0).all()


def test_search_failure_is_a_failure():
    assert S.search(iter(range(5)), lambda k: k == 3 and "found") == (3, "found")
    with pytest.raises(AssertionError, match="lands on the seam"):
        S.search(iter(range(5)), lambda k: None)
