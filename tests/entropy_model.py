"""A bit-level model of jpezy's Huffman tail, used to BUILD coefficient fields that sit on the GPU entropy coder's seams
(tests/test_gpu_entropy_seams.py).  It is not the reference: every field it builds is still checked against the host writer
and the oracle.  tests/test_entropy_model.py proves it equal to the host writer on random fields first.

What it knows:
- the Annex-K code of every symbol (tests/golden/ref_tables.json, the reference's own tables), hence a block's coded length;
- the coded order of a frame (6 blocks per MCU, gray frames code two zero chroma blocks) and the three DC predictors;
- the GPU coder's in-place LDS row (jpezy_entropy.hip, RowWriter): whether a block is coded in its row or re-coded by the
  DirectWriter (a stream over 35 words = 140 bytes, or a word due before the coefficients under it have been read);
- the entropy-coded segment of a file, with its 0x00 stuffing removed.
"""
import json
from functools import lru_cache
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"
ROW_BYTES = 140             # the in-place row of a lane holds 35 words of stream
WORST_BLOCK_BITS = 1660     # 11 + 11 (chroma DC, category 11) + 63 x (16-bit code + 10 value bits)


@lru_cache(maxsize=None)
def tables():
    """per table t (0 luma, 1 chroma): dc[cat] = (code, len), ac[(run, size)] = (code, len), eob, zrl"""
    h = json.loads((GOLDEN / "ref_tables.json").read_text())["huffman"]
    out = []
    for p in ("Y", "C"):
        dc = {k: (h[p + "DcCodeT"][k], h[p + "DcSizeT"][k]) for k in range(12)}
        code, size = h[p + "AcCodeT"], h[p + "AcSizeT"]
        eob, zrl = h[p + "EOBidx"], h[p + "ZRLidx"]
        ac = {}
        for run in range(16):
            for s in range(1, 11):
                # the reference's 162-entry order: EOB, (run 0..14, size 1..10), ZRL, (run 15, size 1..10)
                i = run * 10 + s if run < 15 else zrl + s
                ac[(run, s)] = (code[i], size[i])
        out.append({"dc": dc, "ac": ac, "eob": (code[eob], size[eob]), "zrl": (code[zrl], size[zrl])})
    return out


def category(v):
    return int(abs(int(v))).bit_length()


def _bits(value, n):
    return format(value & ((1 << n) - 1), f"0{n}b") if n else ""


def _value_bits(v, s):
    v = int(v)
    return _bits(v if v >= 0 else v - 1, s)


def block_puts(z, pred, t):
    """the appends of one block as (n_read, bits) in coding order: n_read is the zig-zag position the coder has read up to
    (RowWriter::read_up_to) when it appends; z None is an all-zero block"""
    T = tables()[t]
    dcv = 0 if z is None else int(z[0])
    d = dcv - int(pred)
    c = category(d)
    code, ln = T["dc"][c]
    puts = [(0, _bits(code, ln) + _value_bits(d, c))]
    prev = 0
    if z is not None:
        for n in range(1, 64):
            v = int(z[n])
            if v == 0:
                continue
            run = n - prev - 1
            prev = n
            while run > 15:
                puts.append((n, _bits(*T["zrl"])))
                run -= 16
            s = category(v)
            code, ln = T["ac"][(run, s)]
            puts.append((n, _bits(code, ln) + _value_bits(v, s)))
    if prev != 63:
        puts.append((63, _bits(*T["eob"])))
    return puts


def block_bitstring(z, pred, t):
    return "".join(b for _, b in block_puts(z, pred, t))


def block_bits(z, pred, t):
    return len(block_bitstring(z, pred, t))


def fits_row(z, pred, t):
    """True when the GPU coder codes the block in its LDS row, False when it is re-coded by the DirectWriter: word j of the
    private stream may be stored once every coefficient below 2j - 6 has been read, and the row ends after word 34"""
    wj2, nacc = -6, 0
    for npos, b in block_puts(z, pred, t):
        t_ = nacc + len(b)
        nacc = t_ & 31
        if t_ >= 32:
            if wj2 > npos:
                return False
            wj2 += 2
    if nacc > 0 and wj2 > 63:
        return False
    return True


def coded_blocks(coeffs, gray=False):
    """(z or None, pred, table) of every coded block of one frame, in stream order; coeffs [nmcu, 4|6, 64]"""
    co = np.asarray(coeffs).reshape(-1, 4 if gray else 6, 64)
    pred = [0, 0, 0]
    for m in range(co.shape[0]):
        for i in range(6):
            comp = 0 if i < 4 else i - 3
            z = None if (gray and i >= 4) else co[m, i]
            yield z, pred[comp], 0 if comp == 0 else 1
            pred[comp] = 0 if z is None else int(z[0])


def block_lengths(coeffs, gray=False):
    return np.array([block_bits(z, p, t) for z, p, t in coded_blocks(coeffs, gray)], dtype=np.int64)


def frame_bitstring(coeffs, gray=False):
    return "".join(block_bitstring(z, p, t) for z, p, t in coded_blocks(coeffs, gray))


def unstuffed_stream(coeffs, gray=False, pad_bit=0):
    """the frame's entropy-coded bytes before 0xFF00 stuffing (pad bits as include/jpezy_constants.h JPEZY_PAD_BIT)"""
    s = frame_bitstring(coeffs, gray)
    s += str(pad_bit) * (-len(s) % 8)
    return bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))


def scan_of(jpg):
    """the entropy-coded segment of a jpezy file (after SOS, before EOI) with its stuffed 0x00 bytes removed"""
    jpg = bytes(jpg)
    sos = jpg.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")
    assert jpg[-2:] == b"\xff\xd9"
    return jpg[start:-2].replace(b"\xff\x00", b"\xff")


def ff_positions(stream):
    return np.flatnonzero(np.frombuffer(bytes(stream), dtype=np.uint8) == 0xFF)


# ---- builders ----
def ac_block(sizes, dc=0, sign=1):
    """a block whose AC coefficient at zig-zag position n has category sizes[n - 1] (0: zero); values are the largest of their
    category (all value bits one), negated with sign = -1"""
    z = np.zeros(64, np.int16)
    z[0] = dc
    for n, s in enumerate(sizes, start=1):
        if s:
            z[n] = sign * ((1 << s) - 1)
    return z


def block_of_bits(target, pred=0, t=0, dc=None):
    """a block of exactly `target` coded bits that keeps its bits behind its reads: all 63 AC positions non-zero (no run, no
    EOB), categories in ascending order of their code length (the long codes at the end), so that the GPU coder codes it in its
    row whenever target <= 8 * ROW_BYTES; None if no such block exists"""
    dc = pred if dc is None else dc
    sizes = _sizes_of_bits(int(target), int(pred), int(t), int(dc))
    return None if sizes is None else ac_block(sizes, dc)


@lru_cache(maxsize=None)
def _sizes_of_bits(target, pred, t, dc):
    T = tables()[t]
    cost = {s: T["ac"][(0, s)][1] + s for s in range(1, 11)}
    rest = target - len(block_puts(np.array([dc] + [0] * 63), pred, t)[0][1])
    # reach[k] = {bits: sizes} reachable with k coefficients (a small knapsack over the ten categories)
    reach = {0: ()}
    for _ in range(63):
        nxt = {}
        for b, sizes in reach.items():
            for s in range(1, 11):
                nb = b + cost[s]
                if nb <= rest and nb not in nxt:
                    nxt[nb] = sizes + (s,)
        reach = nxt
    if rest not in reach:
        return None
    return tuple(sorted(reach[rest], key=lambda s: (cost[s], s)))


@lru_cache(maxsize=None)
def _short_lengths(t):
    """{coded bits: AC sizes} of blocks with at most three small coefficients at positions 1..3 (DC difference 0)"""
    out = {}
    for a in range(0, 11):
        for b in range(0, 11):
            for c in range(0, 6):
                sizes = (a, b, c)
                n = block_bits(ac_block(sizes), 0, t)
                out.setdefault(n, sizes)
    return out


def tuner_block(bits, t=0):
    """a block of exactly `bits` coded bits with DC 0 after a DC of 0 (None if there is none of that length)"""
    s = _short_lengths(t).get(bits)
    return None if s is None else ac_block(s)


def dense_block(dc=0):
    """the densest luma content: every AC coefficient +1023 (16-bit code, ten one bits): runs of 21 one bits, 0xFF bytes"""
    z = np.full(64, 1023, np.int16)
    z[0] = dc
    return z
