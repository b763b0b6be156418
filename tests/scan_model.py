"""One bit-level model of the scan for every MCU layout, table set and restart form the GPU entropy coder has
(jpezy_amd/csrc/jpezy_entropy.hip), used to BUILD coefficient fields that sit on the coder's seams
(tests/test_gpu_entropy_layout_seams.py).  Pure Python and numpy: no library and no GPU behind it.  It is not the reference:
tests/test_scan_model.py proves it equal to the host writer and to the four older models (entropy_model, restart_model,
sampling_model, sampling422_model) where their domains overlap, and every field it builds is still checked against the host writer.

Parameters everywhere:
- layout: "420", "420gray", "444", "422" (LAYOUTS): coded and stored blocks per MCU, the luma count, the component and table of
  every coded position; gray codes two zero chroma blocks that are not stored;
- tables: None for Annex K (tests/golden/ref_tables.json), or four (bits, vals) in DHT order YDc, CDc, YAc, CAc;
- ri: MCUs per restart interval, 0 for none.

What it knows beyond the bits: the coder's in-place LDS row (RowWriter: whether a block is coded in its row, and why not), its
tiles of 256 coded blocks that never straddle an interval (restart_tpi / restart_tiles of jpezy_entropy.h), the 64-byte chunks and
16 KB pieces of the unstuffed stream, and per chunk the markers and the bytes the stuffing pass adds.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import entropy_model as M
import huffopt_model as HM
import restart_model as RM

PAD_BIT = RM.PAD_BIT
ROW_BYTES = 140                 # the in-place row of a lane holds 35 words of stream
TILE, CHUNK, PIECE = 256, 64, 16384
CHUNK_BITS, PIECE_BITS = 8 * CHUNK, 8 * PIECE

# sampling: the library's enum (jpezy_amd.SAMPLING_420 / _444 / _422); mcu_w, mcu_h in pixels
Layout = namedtuple("Layout", "name coded stored luma mcu_w mcu_h sampling gray")
LAYOUTS = {
    "420": Layout("420", 6, 6, 4, 16, 16, 0, False),
    "420gray": Layout("420gray", 6, 4, 4, 16, 16, 0, True),
    "444": Layout("444", 3, 3, 1, 8, 8, 1, False),
    "422": Layout("422", 4, 4, 2, 16, 8, 3, False),
}


def layout_of(layout):
    return layout if isinstance(layout, Layout) else LAYOUTS[layout]


def component(layout, i):
    """component (0 Y, 1 Cb, 2 Cr) of coded position i of an MCU"""
    L = layout_of(layout)
    return 0 if i < L.luma else i - L.luma + 1


def table_of(layout, i):
    """Huffman table (0 luma, 1 chroma) of coded block i of a frame"""
    L = layout_of(layout)
    return 0 if i % L.coded < L.luma else 1


def is_stored(layout, i):
    L = layout_of(layout)
    return i % L.coded < L.stored


def mcus(coeffs, layout):
    return np.asarray(coeffs).reshape(-1, layout_of(layout).stored, 64)


def frame_size(nmcu_cols, nmcu_rows, layout):
    """(W, H) of a frame of that many MCUs"""
    L = layout_of(layout)
    return nmcu_cols * L.mcu_w, nmcu_rows * L.mcu_h


# ---- code tables ----
def freeze(tables):
    """a hashable copy of four (bits, vals); None stays None"""
    return None if tables is None else tuple((tuple(int(b) for b in bits), tuple(int(v) for v in vals)) for bits, vals in tables)


@lru_cache(maxsize=None)
def _codes(frozen):
    if frozen is not None:
        return [HM.codes(b, v) for b, v in frozen]
    T = M.tables()
    out = [dict(T[t]["dc"]) for t in (0, 1)]
    for t in (0, 1):
        ac = {(run << 4) | s: c for (run, s), c in T[t]["ac"].items()}
        ac[0x00], ac[0xF0] = T[t]["eob"], T[t]["zrl"]
        out.append(ac)
    return out


def codes(tables=None):
    """[YDc, CDc, YAc, CAc] of {symbol: (code, length)}; DC symbols are categories, AC symbols (run << 4) | size, 0x00 EOB, 0xF0 ZRL"""
    return _codes(freeze(tables))


# ---- one block ----
def block_puts(z, pred, t, tables=None):
    """the appends of one block as (n_read, bits) in coding order: n_read is the zig-zag position the coder has read up to
    (RowWriter::read_up_to) when it appends; z None is an all-zero block"""
    C = codes(tables)
    dc, ac = C[t], C[2 + t]
    d = (0 if z is None else int(z[0])) - int(pred)
    c = M.category(d)
    assert c <= 11, "DC difference outside the tables"
    puts = [(0, M._bits(*dc[c]) + M._value_bits(d, c))]
    prev = 0
    if z is not None:
        for n in range(1, 64):
            v = int(z[n])
            if v == 0:
                continue
            run = n - prev - 1
            prev = n
            while run > 15:
                puts.append((n, M._bits(*ac[0xF0])))
                run -= 16
            s = M.category(v)
            assert s <= 10, "AC value outside the tables"
            puts.append((n, M._bits(*ac[(run << 4) | s]) + M._value_bits(v, s)))
    if prev != 63:
        puts.append((63, M._bits(*ac[0x00])))
    return puts


def block_bitstring(z, pred, t, tables=None):
    return "".join(b for _, b in block_puts(z, pred, t, tables))


def block_bits(z, pred, t, tables=None):
    return len(block_bitstring(z, pred, t, tables))


def row_verdict(z, pred, t, tables=None):
    """"row": the GPU coder codes the block in its LDS row; otherwise why it re-codes it (DirectWriter) -- "words": a word past
    word 34 of the row is due (a stream over 35 words); "licence": word j is due while a coefficient at or above 2j - 6 is unread.
    The reason is that of the FIRST word refused, as RowWriter::word sees it."""
    wj2, nacc = -6, 0
    for npos, b in block_puts(z, pred, t, tables):
        tot = nacc + len(b)
        nacc = tot & 31
        if tot >= 32:
            if wj2 > npos:
                return "words" if wj2 > 63 else "licence"
            wj2 += 2
    if nacc > 0 and wj2 > 63:
        return "words"
    return "row"


def fits_row(z, pred, t, tables=None):
    return row_verdict(z, pred, t, tables) == "row"


# ---- a frame ----
def intervals(nmcu, ri):
    """[(first MCU, MCUs)] of every restart interval (ri = 0: the whole frame)"""
    step = ri if ri else max(nmcu, 1)
    return [(m, min(step, nmcu - m)) for m in range(0, nmcu, step)]


def coded_blocks(coeffs, layout="420", ri=0):
    """(z or None, pred, table) of every coded block of one frame, in stream order, the predictors reset at interval starts"""
    L = layout_of(layout)
    co = mcus(coeffs, L)
    pred = [0, 0, 0]
    for m in range(co.shape[0]):
        if ri and m % ri == 0:
            pred = [0, 0, 0]
        for i in range(L.coded):
            comp = component(L, i)
            z = co[m, i] if i < L.stored else None
            yield z, pred[comp], 0 if comp == 0 else 1
            pred[comp] = 0 if z is None else int(z[0])


def _distinct_mcus(coeffs, layout):
    """(distinct MCUs [k, stored, 64], the index of every MCU among them): with one MCU per interval every MCU is coded from
    predictors of zero, so a large frame of few distinct MCUs is coded once per distinct MCU"""
    L = layout_of(layout)
    co = mcus(coeffs, L)
    rows = np.ascontiguousarray(co.reshape(co.shape[0], -1))
    seen, first, inv = {}, [], np.empty(co.shape[0], np.int64)
    for m in range(co.shape[0]):
        k = seen.setdefault(rows[m].tobytes(), len(seen))
        if k == len(first):
            first.append(m)
        inv[m] = k
    return co[first], inv


def block_bitstrings(coeffs, layout="420", tables=None, ri=0):
    if ri == 1 and mcus(coeffs, layout).shape[0] > 64:
        uniq, inv = _distinct_mcus(coeffs, layout)
        per = [[block_bitstring(z, p, t, tables) for z, p, t in coded_blocks(u, layout)] for u in uniq]
        return [s for k in inv for s in per[k]]
    return [block_bitstring(z, p, t, tables) for z, p, t in coded_blocks(coeffs, layout, ri)]


def block_lengths(coeffs, layout="420", tables=None, ri=0):
    return np.array([len(s) for s in block_bitstrings(coeffs, layout, tables, ri)], dtype=np.int64)


def block_verdicts(coeffs, layout="420", tables=None, ri=0):
    return [row_verdict(z, p, t, tables) for z, p, t in coded_blocks(coeffs, layout, ri)]


def symbol_counts(coeffs, layout="420", ri=0):
    """hist[4][256] (DHT order) of the symbols the scan emits, and whether every value was in range"""
    hist = np.zeros((4, 256), np.int64)
    ok = True
    if ri == 1 and mcus(coeffs, layout).shape[0] > 64:
        uniq, inv = _distinct_mcus(coeffs, layout)
        for u, n in zip(uniq, np.bincount(inv, minlength=len(uniq))):
            h, good = symbol_counts(u, layout)
            hist += h * int(n)
            ok &= good
        return hist, ok
    for z, pred, t in coded_blocks(coeffs, layout, ri):
        c, syms, good = HM.block_symbols(z, pred)
        ok &= good
        hist[t, c] += 1
        for s in syms:
            hist[2 + t, s] += 1
    return hist, ok


def frame_tables(coeffs, layout="420", ri=0):
    """the frame's four optimal tables [(bits, vals)] in DHT order"""
    hist, ok = symbol_counts(coeffs, layout, ri)
    assert ok
    return [HM.optimal_table(hist[k])[:2] for k in range(4)]


def interval_bitstrings(coeffs, layout="420", tables=None, ri=0):
    L = layout_of(layout)
    if ri == 1 and mcus(coeffs, L).shape[0] > 64:
        uniq, inv = _distinct_mcus(coeffs, L)
        per = ["".join(block_bitstring(z, p, t, tables) for z, p, t in coded_blocks(u, L)) for u in uniq]
        return [per[k] for k in inv]
    blocks = block_bitstrings(coeffs, L, tables, ri)
    return ["".join(blocks[m * L.coded:(m + n) * L.coded]) for m, n in intervals(len(blocks) // L.coded, ri)]


def interval_bits(coeffs, layout="420", tables=None, ri=0):
    return [len(s) for s in interval_bitstrings(coeffs, layout, tables, ri)]


def unstuffed_intervals(coeffs, layout="420", tables=None, ri=0, pad_bit=PAD_BIT):
    """every interval's bytes before stuffing, padded with pad_bit up to a byte"""
    return [RM.padded(s, pad_bit) for s in interval_bitstrings(coeffs, layout, tables, ri)]


def unstuffed_stream(coeffs, layout="420", tables=None, ri=0, pad_bit=PAD_BIT):
    """the GPU coder's stream U: the padded intervals back to back, no stuffing and no markers"""
    return b"".join(unstuffed_intervals(coeffs, layout, tables, ri, pad_bit))


def scan(coeffs, layout="420", tables=None, ri=0, pad_bit=PAD_BIT):
    """the entropy-coded segment as the file holds it, between the SOS header and EOI: stuffed, RSTn behind every interval but the last"""
    parts = unstuffed_intervals(coeffs, layout, tables, ri, pad_bit)
    out = bytearray()
    for k, p in enumerate(parts):
        out += p.replace(b"\xff", b"\xff\x00")
        if k + 1 < len(parts):
            out += bytes([0xFF, 0xD0 + k % 8])
    return bytes(out)


# ---- the file ----
def header(W, H, layout="420", tables=None, ri=0, comment=None):
    """SOI .. SOS.  4:2:0: the oracle writer's header with the DHT segments replaced (huffopt_model.header_with_tables) and a DRI
    segment in front of SOS; 4:4:4 / 4:2:2: the per-layout headers of sampling_model / sampling422_model"""
    L = layout_of(layout)
    tables = None if tables is None else [(list(b), list(v)) for b, v in tables]
    if L.name == "444":
        import sampling_model as SM
        return SM.header(W, H, comment, None, tables, ri)
    if L.name == "422":
        import sampling422_model as S2
        return S2.header(W, H, comment, None, tables, ri)
    from oracle import oracle as O
    mc, mr = O.mcu_grid(W, H)
    base = O.write_jpeg(np.zeros((mr * mc, L.stored, 64), np.int16), W, H, L.gray, comment)
    hdr = RM.split(base)[0] if tables is None else HM.header_with_tables(base, tables)
    if ri:
        sos = hdr.index(b"\xff\xda")
        hdr = hdr[:sos] + b"\xff\xdd\x00\x04" + int(ri).to_bytes(2, "big") + hdr[sos:]
    return hdr


def write_jpeg(coeffs, W, H, layout="420", tables=None, ri=0, comment=None, optimize=False):
    """the whole file; optimize: with the frame's own tables (frame_tables) instead of `tables`"""
    if optimize:
        tables = frame_tables(coeffs, layout, ri)
    return header(W, H, layout, tables, ri, comment) + scan(coeffs, layout, tables, ri) + b"\xff\xd9"


# ---- the coder's geometry ----
def device_ri(nmcu, ri):
    """the interval the DEVICE acts on (Job::restart): 0 too for an interval that holds the whole frame"""
    return ri if 0 < ri < nmcu else 0


def restart_tpi(ri, layout):
    """tiles per restart interval (restart_tpi of jpezy_entropy.h)"""
    return (ri * layout_of(layout).coded + TILE - 1) // TILE


def tiles(nmcu, layout="420", ri=0):
    """[(first coded block, blocks)] of every coding workgroup's tile: 256 blocks of the frame or, with restart intervals, of an
    interval -- every interval starts a tile of its own (restart_tile_first / restart_tiles of jpezy_entropy.h)"""
    L = layout_of(layout)
    out = []
    for m, n in intervals(nmcu, device_ri(nmcu, ri)):
        first, count = m * L.coded, n * L.coded
        out += [(first + o, min(TILE, count - o)) for o in range(0, count, TILE)]
    return out


def tile_of_block(nmcu, layout, ri, g):
    """(tile index, lane) of coded block g"""
    for k, (first, count) in enumerate(tiles(nmcu, layout, ri)):
        if first <= g < first + count:
            return k, g - first
    raise IndexError(g)


Geometry = namedtuple("Geometry", "lengths offsets tiles tile_bits tile_offsets stream_bits")


def geometry(coeffs, layout="420", tables=None, ri=0):
    """lengths / offsets: bits of every coded block and its first bit in U (pads of the intervals in front of it included);
    tiles, tile_bits, tile_offsets likewise per tile; stream_bits: the last block's last bit + 1 (before the frame's own pad)"""
    L = layout_of(layout)
    lengths = block_lengths(coeffs, L, tables, ri)
    nmcu = len(lengths) // L.coded
    offsets = np.zeros(len(lengths), np.int64)
    pos = 0
    ivs = intervals(nmcu, device_ri(nmcu, ri))
    for k, (m, n) in enumerate(ivs):
        for g in range(m * L.coded, (m + n) * L.coded):
            offsets[g] = pos
            pos += int(lengths[g])
        if k + 1 < len(ivs):
            pos += -pos % 8
    tl = tiles(nmcu, L, ri)
    tile_bits = [int(lengths[f:f + c].sum()) for f, c in tl]
    return Geometry(lengths, offsets, tl, tile_bits, [int(offsets[f]) for f, _ in tl], pos)


def chunk_of(bit):
    return int(bit) // CHUNK_BITS


def piece_of(bit):
    return int(bit) // PIECE_BITS


def chunk_stats(coeffs, layout="420", tables=None, ri=0):
    """per 64-byte chunk of U: (markers, extra) -- the RSTn markers behind bytes of the chunk (a marker belongs to the chunk that
    holds the last byte of its interval) and the bytes the stuffing pass adds (one per 0xFF byte, two per marker)"""
    return chunk_stats_of(unstuffed_intervals(coeffs, layout, tables, ri))


def chunk_stats_of(parts):
    """chunk_stats of the intervals' unstuffed bytes"""
    U = np.frombuffer(b"".join(parts), np.uint8)
    n = -(-len(U) // CHUNK)
    ends = np.cumsum([len(p) for p in parts[:-1]], dtype=np.int64)
    marks = np.bincount((ends - 1) // CHUNK, minlength=n) if len(ends) else np.zeros(n, np.int64)
    ff = np.bincount(np.flatnonzero(U == 0xFF) // CHUNK, minlength=n)
    return marks, ff + 2 * marks


def piece_output_offsets(extra):
    """from chunk_stats' extra: the offset in the stuffed scan of the first byte every 16 KB piece of U puts out"""
    per = PIECE // CHUNK
    return [p * PIECE + int(extra[:p * per].sum()) for p in range(-(-len(extra) // per))]


# ---- builders ----
def ac_block(sizes, dc=0, sign=1):
    return M.ac_block(sizes, dc, sign)


def dense_block(dc=0, sign=1):
    """every AC coefficient +-1023: the longest code and ten equal value bits"""
    z = np.full(64, sign * 1023, np.int16)
    z[0] = dc
    return z


def flat_block(dc=0):
    z = np.zeros(64, np.int16)
    z[0] = dc
    return z


def block_of_bits(target, pred=0, t=0, dc=None, tables=None):
    """a block of exactly `target` coded bits that keeps its bits behind its reads: all 63 AC positions non-zero (no run, no EOB),
    categories in ascending order of their cost (the long codes at the end), so that the GPU coder codes it in its row whenever
    target <= 8 * ROW_BYTES; only symbols the tables have; None if no such block exists"""
    dc = pred if dc is None else dc
    sizes = _sizes_of_bits(int(target), int(pred), int(t), int(dc), freeze(tables))
    return None if sizes is None else ac_block(sizes, dc)


@lru_cache(maxsize=None)
def _sizes_of_bits(target, pred, t, dc, frozen):
    C = _codes(frozen)
    cost = {s: C[2 + t][s][1] + s for s in range(1, 11) if s in C[2 + t]}
    c = M.category(dc - pred)
    if c not in C[t] or not cost:
        return None
    rest = target - (C[t][c][1] + c)
    reach = {0: ()}
    for _ in range(63):
        nxt = {}
        for b, sizes in reach.items():
            for s, cs in cost.items():
                nb = b + cs
                if nb <= rest and nb not in nxt:
                    nxt[nb] = sizes + (s,)
        reach = nxt
    if rest not in reach:
        return None
    return tuple(sorted(reach[rest], key=lambda s: (cost[s], s)))


@lru_cache(maxsize=None)
def _short_lengths(t, frozen):
    C = _codes(frozen)
    out = {}
    for a in range(0, 11):
        for b in range(0, 11):
            for c in range(0, 6):
                sizes = (a, b, c)
                z = ac_block(sizes)
                try:
                    n = block_bits(z, 0, t, frozen)
                except KeyError:            # a symbol the tables do not have
                    continue
                out.setdefault(n, sizes)
    return out


def tuner_block(bits, t=0, tables=None):
    """a block of exactly `bits` coded bits with DC 0 after a DC of 0: at most three coefficients at positions 1..3 (None if there
    is none of that length)"""
    s = _short_lengths(int(t), freeze(tables)).get(int(bits))
    return None if s is None else ac_block(s)


def exact_block(bits, t=0, tables=None):
    z = tuner_block(bits, t, tables)
    return z if z is not None else block_of_bits(bits, 0, t, None, tables)


def _worst_size(tables, t):
    C = codes(tables)
    cost = {s: C[2 + t][s][1] + s for s in range(1, 11) if s in C[2 + t]}
    return max(cost, key=lambda k: (cost[k], k))


def worst_block(tables=None, t=0, dc=-1023):
    """the longest block the tables can code at table t: at every AC position the category whose code + value bits is longest, all
    value bits one.  Annex K, luma: 16 + 10 bits, 63 x 26 = 1638 bits and the DC's 9 + 11 after a category-11 step -- 1658 of the
    1660 bits the coder's scratch gives a block (chroma's longest run-0 code is 12 bits: 1408)"""
    return ac_block([_worst_size(tables, t)] * 63, dc)


def licence_block(tables=None, t=0, dc=0, pred=0, sign=-1, max_bytes=80):
    """a block the RowWriter refuses by its licence alone: the fewest leading coefficients of the longest category, then zeros, for
    which a word is due before the coefficients under it are read -- far under the row's 140 bytes.  None if there is none within
    max_bytes."""
    s = _worst_size(tables, t)
    for k in range(1, 64):
        z = ac_block([s] * k, dc, sign)
        if block_bits(z, pred, t, tables) > 8 * max_bytes:
            return None
        if row_verdict(z, pred, t, tables) == "licence":
            return z
    return None


def frame_of_bits(total, layout="420", tables=None, ri=0, filler=900, lead=None):
    """[nmcu, stored, 64] whose stream U holds exactly `total` bits up to the end of its last coded block (the pad bits behind the
    intervals in front of it included), DC 0 everywhere: filler blocks of `filler` bits, then flat blocks, and the last stored
    block tuned to the exact length.  ri: the last block lies in the last interval, so no pad depends on it.
    lead: blocks put in front (a list, in coded order of the stored positions).  None if the tuner has no block of the length."""
    L = layout_of(layout)
    frozen = freeze(tables)
    per_mcu = sum(filler if i < L.stored else block_bits(None, 0, 1, frozen) for i in range(L.coded))
    nmcu = max(1, -(-total // per_mcu))
    while True:
        co = _fill(total, L, frozen, ri, filler, nmcu, lead)
        if co is not None or nmcu > -(-total // per_mcu) + 3:
            return co
        nmcu += 1


def _fill(total, L, frozen, ri, filler, nmcu, lead):
    co = np.zeros((nmcu, L.stored, 64), np.int16)
    stored = [(m, i) for m in range(nmcu) for i in range(L.stored)]
    last = stored[-1]
    k0 = 0
    for z in lead or []:
        co[stored[k0]] = z
        k0 += 1
    fill = [block_of_bits(filler, 0, t, None, frozen) for t in (0, 1)]
    if fill[0] is None or fill[1] is None:
        return None
    flat_last = block_bits(flat_block(), 0, 0 if last[1] < L.luma else 1, frozen)
    # fill greedily, measuring the stream as the model states it (pads included)
    bits = lambda: geometry(co, L, frozen, ri).stream_bits
    base = bits()
    flat = [block_bits(flat_block(), 0, t, frozen) for t in (0, 1)]
    for m, i in stored[k0:-1]:
        t = 0 if i < L.luma else 1
        if total - base - (filler - flat[t]) < 400 + 7 * len(intervals(nmcu, ri)):
            break
        co[m, i] = fill[t]
        base += filler - flat[t]
    base = bits()
    z = exact_block(total - (base - flat_last), 0 if last[1] < L.luma else 1, frozen)
    if z is None:
        return None
    co[last] = z
    return co if bits() == total else None


def settle(build, layout="420", ri=0, rounds=8):
    """Per-image tables depend on the field they code.  build(tables) makes the field with its exact-length blocks built for
    `tables` (None: Annex K, the first guess); this repeats it with the tables the field then has until they no longer change.
    Returns (field, its frame tables, frozen) -- every exact length the builder promised holds under them -- or None."""
    tables = None
    for _ in range(rounds):
        co = build(tables)
        if co is None:
            return None
        have = freeze(frame_tables(co, layout, ri))
        if have == tables:
            return co, have
        tables = have
    return None


def search(candidates, lands):
    """the first candidate that lands on its seam: `candidates` yields fields (or anything), `lands(candidate)` returns a truthy
    finding or None / False.  Per-image tables depend on the field they code, so builders for them try a small seeded family and
    recompute frame_tables for each.  Nothing found is an AssertionError (a test failure, never a skip)."""
    tried = 0
    for cand in candidates:
        tried += 1
        found = lands(cand)
        if found:
            return cand, found
    raise AssertionError(f"no field of the family lands on the seam ({tried} tried)")
