"""Per-image optimised Huffman tables on the host: jpezy_huffman_optimal_table against a plain-Python restatement of Annex K.2
(tests/huffopt_model.py), jpezy_write_jpeg_opt against the oracle's reader, PIL and the restatement's bit writer, and the
code-length bounds the coder's scratch sizes and jpezy_jpeg_bound rest on."""
import ctypes as C
import heapq
import io
import re
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import huffopt_model as HM

ROOT = Path(__file__).resolve().parent.parent
FIXTURES = ["rand64", "rand17x33", "gradient52x40", "rand16", "greyramp256x16", "flatgrey256"]


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _fib_freq(n, first=1):
    """counts 1, 2, 3, 5, 8, ... on the symbols first, first + 1, ..."""
    freq = np.zeros(256, np.uint64)
    freq[first:first + n] = HM.fibonacci_counts(n)
    return freq


def _cases():
    rng = np.random.default_rng(20261)
    cases = {}
    for i in range(12):
        freq = np.zeros(256, np.uint64)
        n = int(rng.integers(2, 257))
        idx = rng.choice(256, n, replace=False)
        freq[idx] = rng.integers(1, [4, 100, 100000, 1 << 40][i % 4], n)     # small ranges: many ties
        cases[f"random{i}"] = freq
    geo = np.zeros(256, np.uint64)
    geo[:40] = [3 ** k for k in range(40)]                                   # depth 40 before limiting
    cases["geometric40"] = geo
    import entropy_model as M
    ac = np.zeros(256, np.uint64)
    for (run, s) in M.tables()[0]["ac"]:
        ac[(run << 4) | s] = 1 + (run * 7 + s * 13) % 50
    ac[0x00], ac[0xF0] = 1000, 3
    assert np.count_nonzero(ac) == 162
    cases["all162"] = ac
    single = np.zeros(256, np.uint64)
    single[0x00] = 12345
    cases["single"] = single
    cases["fib19"] = _fib_freq(19)
    cases["fib36"] = _fib_freq(36, first=17)
    return cases


CASES = _cases()


def _kraft(bits):
    return sum(Fraction(int(b), 1 << (l + 1)) for l, b in enumerate(bits))


def _heap_cost(freq):
    """sum f * len of a plain Huffman code over the symbols of freq plus the reserved symbol of count 1"""
    h = [int(f) for f in freq if f] + [1]
    heapq.heapify(h)
    cost = 0
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        cost += a + b
        heapq.heappush(h, a + b)
    return cost


@pytest.mark.parametrize("name", sorted(CASES))
def test_optimal_table_equals_restatement(J, name):
    freq = CASES[name]
    bits, vals = J.optimal_table(freq)
    want_bits, want_vals, depth = HM.optimal_table(freq)
    assert list(bits) == want_bits and list(vals) == want_vals
    if name == "fib19":
        assert depth == 19
    if name in ("fib19", "geometric40"):
        assert depth > 16                      # the limiting branch (Figure K.3) is taken
    if name == "fib36":
        assert depth > 32 and int(freq.sum()) > 5 * 10 ** 7
    # properties: every used symbol once, lengths within 16, room left for the all-ones code
    used = [s for s in range(256) if freq[s]]
    assert sorted(vals) == used and int(np.sum(bits)) == len(used)
    lens = HM.lengths(bits)
    assert max(lens) <= 16
    assert _kraft(bits) <= 1 - Fraction(1, 1 << max(lens))
    if name == "single":
        assert list(bits) == [1] + [0] * 15 and list(vals) == [0x00]
    if depth <= 16:                             # nothing was limited: the code is optimal over the augmented alphabet
        code = HM.codes(bits, vals)             # (the reserved symbol, count 1, keeps the slot it left at the longest length)
        assert sum(int(freq[s]) * code[s][1] for s in used) + depth == _heap_cost(freq)


def test_all_zero_counts_give_an_empty_table(J):
    bits, vals = J.optimal_table(np.zeros(256, np.uint64))
    assert not bits.any() and vals.size == 0


def _golden(golden_dir, name):
    return np.load(golden_dir / f"{name}.npz")


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("name", FIXTURES)
def test_write_jpeg_optimize_on_fixtures(J, oracle, golden_dir, name, gray):
    from PIL import Image
    z = _golden(golden_dir, name)
    W, H = int(z["W"]), int(z["H"])
    co = z["coeffs_gray"] if gray else z["coeffs"]
    fixed = J.write_jpeg(co, W, H, gray)
    assert fixed == (z["jpg_gray"] if gray else z["jpg"]).tobytes()
    opt = J.write_jpeg(co, W, H, gray, optimize=True)
    # the oracle's reader: the fixture's coefficients, the frame fields of the Annex-K file
    info, got = oracle.read_jpeg(opt)
    info0, got0 = oracle.read_jpeg(fixed)
    assert np.array_equal(got, got0)
    assert np.array_equal(got[:, :, :co.shape[-2]].reshape(co.shape), co)
    for field, _ in type(info)._fields_:
        a, b = getattr(info, field), getattr(info0, field)
        assert (bytes(a) == bytes(b)) if hasattr(a, "_length_") else (a == b), field
    # PIL: the same pixels
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(opt))), np.asarray(Image.open(io.BytesIO(fixed))))
    # the restatement's tables and bit writer: the same bytes
    assert opt == HM.write_jpeg(co, gray, fixed)
    assert len(opt) < len(fixed)
    print(f"{name} gray={gray}: {len(fixed)} -> {len(opt)} bytes")


def _stress_coeffs(rng, nmcu, bpm=6):
    """the recipe of tests/test_gpu_entropy.py"""
    co = np.zeros((nmcu, bpm, 64), np.int16)
    for m in range(nmcu):
        for b in range(bpm):
            blk = co[m, b]
            kind = rng.integers(0, 8)
            if kind == 0:
                pass                                        # all zero: DC diff + EOB
            elif kind == 1:
                blk[0] = rng.integers(-1023, 1024)
                blk[63] = rng.integers(1, 1024)             # 62 zeros then a value: three ZRLs, no EOB
            elif kind == 2:
                blk[:] = rng.integers(-1023, 1024, 64)      # dense, maximal categories
            elif kind == 3:
                blk[0] = -1023
                blk[1:] = 1023                              # long runs of 1-bits: 0xFF bytes to stuff
            elif kind == 4:
                blk[rng.integers(1, 64, 5)] = rng.integers(-7, 8, 5)
            elif kind == 5:
                blk[17] = 1; blk[34] = -1; blk[51] = 2      # runs of exactly 16: ZRL + run 0
            elif kind == 6:
                blk[0] = rng.integers(-1023, 1024)
                blk[16] = -512                              # run 15 (no ZRL), size 10
            else:
                blk[:] = rng.integers(-3, 4, 64)
    return co


@pytest.mark.parametrize("size", [(48, 32), (100, 60)])
def test_stress_coefficients_read_back(J, oracle, size):
    W, H = size
    rng = np.random.default_rng(W * 131 + H)
    mc, mr = J.mcu_grid(W, H)
    co = _stress_coeffs(rng, mc * mr).reshape(mr, mc, 6, 64)
    opt = J.write_jpeg(co, W, H, False, optimize=True)
    assert np.array_equal(oracle.read_jpeg(opt)[1], co)
    assert np.array_equal(J.read_jpeg(opt)[1], co)
    assert opt == HM.write_jpeg(co, False, J.write_jpeg(co, W, H, False))
    g = np.ascontiguousarray(co[:, :, :4])
    optg = J.write_jpeg(g, W, H, True, optimize=True)
    back = oracle.read_jpeg(optg)[1]
    assert np.array_equal(back[:, :, :4], g) and not back[:, :, 4:].any()


def test_numpy_count_equals_block_loop():
    """the two counting helpers of tests/huffopt_model.py agree (the GPU tests use the numpy one for their largest frame)"""
    rng = np.random.default_rng(5)
    co = rng.integers(-6, 7, (7, 7, 6, 64)).astype(np.int16)
    co[..., 8:] *= (rng.random((7, 7, 6, 56)) < 0.3)
    co[..., 0] = rng.integers(-900, 900, (7, 7, 6))
    flat = co.reshape(-1, 64)
    flat[::7, 63] = 1000
    flat[3::11, 1:] = 0
    flat[3::11, 40] = -300                                        # run 39: two ZRLs
    flat[5, 9] = 1023
    for gray in (False, True):
        c = np.ascontiguousarray(co[:, :, :4]) if gray else co
        a, b = HM.symbol_counts(c, gray), HM.symbol_counts_np(c, gray)
        assert np.array_equal(a[0], b[0]) and a[1] and b[1]
        assert a[0][2, 0xF0] > 0 and a[0][2, 0x00] > 0
    co[0, 0, 0, 3] = 1024
    a, b = HM.symbol_counts(co), HM.symbol_counts_np(co)
    assert np.array_equal(a[0], b[0]) and not a[1] and not b[1]


def test_refusals(J):
    lib = J.load_library()
    co = np.zeros((1, 1, 6, 64), np.int16)
    buf = np.empty(lib.jpezy_jpeg_bound(16, 16), np.uint8)

    def call(c, comment=b"x"):
        return lib.jpezy_write_jpeg_opt(c.ctypes.data_as(C.c_void_p), 16, 16, 0, comment, buf.ctypes.data_as(C.c_void_p), buf.size)
    assert call(co) > 0
    for pos, val in ((5, 1024), (5, -1024), (0, 2048), (0, -2048)):
        bad = co.copy()
        bad[0, 0, 2, pos] = val
        assert call(bad) == -5, (pos, val)                       # JPEZY_E_FORMAT
        with pytest.raises(J.JpezyError):
            J.write_jpeg(bad, 16, 16, optimize=True)
    limit = int(re.search(r"#define JPEZY_MAX_COMMENT (\d+)", (ROOT / "include" / "jpezy_hip.h").read_text()).group(1))
    assert call(co, b"c" * limit) > 0
    assert call(co, b"c" * (limit + 1)) == -1                     # JPEZY_E_BADARG
    assert lib.jpezy_huffman_optimal_table(None, None, None) == -1


# ---- the bounds the coder's scratch sizes and jpezy_jpeg_bound rest on, with arbitrary tables ----
def test_longest_codes_any_table_can_have(J):
    """a DC table has at most 12 symbols (categories 0..11): with the reserved symbol 13 leaves, so no code is longer than 12 bits --
    reached by the counts 1, 2, 3, 5, ...; an AC code is at most 16 bits whatever the counts"""
    dc = np.zeros(256, np.uint64)
    dc[:12] = HM.fibonacci_counts(12)
    bits, vals = J.optimal_table(dc)
    assert max(HM.lengths(bits)) == 12
    assert max(HM.lengths(J.optimal_table(CASES["fib36"])[0])) == 16
    block = 12 + 11 + 63 * (16 + 10)
    assert block == 1661 and -(-block // 8) <= 208                # the 208 bytes per block of the GPU coder's scratch
    mcu = 6 * block
    assert mcu == 9966 and 2 * -(-mcu // 8) + 2 + 2 <= 2688       # every byte stuffed + pad byte (stuffed) + EOI
    assert 12 + 11 <= 31 and 16 + 10 <= 31 and 16 + 6 <= 31       # every append of the GPU coder


def test_worst_case_frame_fits_the_bound_and_the_header(J, oracle):
    """the densest frame there is (every AC coefficient of size 10, every DC difference of category 11), coded with its own
    tables, stays within jpezy_jpeg_bound; no optimised header is longer than the Annex-K one"""
    lib = J.load_library()
    W, H = 48, 32
    rng = np.random.default_rng(7)
    co = rng.choice(np.array([-1023, 1023, -512, 513], np.int16), (2, 3, 6, 64))
    co[..., 0] = np.where(np.arange(36).reshape(2, 3, 6) % 2, 1023, -1023)
    opt = J.write_jpeg(co, W, H, optimize=True)
    assert len(opt) <= lib.jpezy_jpeg_bound(W, H)
    assert np.array_equal(oracle.read_jpeg(opt)[1], co)
    limit = int(re.search(r"#define JPEZY_MAX_COMMENT (\d+)", (ROOT / "include" / "jpezy_hip.h").read_text()).group(1))
    for c in (co, _stress_coeffs(np.random.default_rng(3), 6).reshape(2, 3, 6, 64)):
        a = J.write_jpeg(c, W, H, comment=b"c" * limit)
        b = J.write_jpeg(c, W, H, comment=b"c" * limit, optimize=True)
        assert b.index(b"\xff\xda") <= a.index(b"\xff\xda") and a.index(b"\xff\xda") + 14 <= 1024
