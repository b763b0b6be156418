"""A plain-Python restatement of per-image optimised Huffman tables (tests/test_huffopt_host.py, tests/test_gpu_huffopt.py):
the symbols a frame's coder emits, ITU-T T.81 Annex K.2 (Figures K.1 - K.4), and a bit writer that takes arbitrary tables.

It is not the reference: every file it builds is still read back through the oracle.  What it adds is a second statement of the
rules the product implements twice (host writer, GPU coder), so that tables and bytes can be compared bit for bit.
"""
import numpy as np

import entropy_model as M

TABLE_IDS = (0x00, 0x01, 0x10, 0x11)        # DHT order: YDc, CDc, YAc, CAc


# ---- the symbols of a frame ----
def block_symbols(z, pred):
    """(dc category, [ac symbols in order], in_range) of one block; z None is an all-zero block.  Out-of-range values are the
    clamped symbol the coder emits (category 11, size 10)."""
    ok = True
    d = (0 if z is None else int(z[0])) - int(pred)
    c = M.category(d)
    if c > 11:
        ok, c = False, 11
    syms = []
    prev = 0
    if z is not None:
        for n in range(1, 64):
            v = int(z[n])
            if v == 0:
                continue
            run = n - prev - 1
            prev = n
            syms += [0xF0] * (run >> 4)
            s = M.category(v)
            if s > 10:
                ok, s = False, 10
            syms.append(((run & 15) << 4) | s)
    if prev != 63:
        syms.append(0x00)
    return c, syms, ok


def symbol_counts(coeffs, gray=False):
    """hist[4][256] (DHT order) of one frame and whether every value was in range; the per-block Python loop"""
    hist = np.zeros((4, 256), np.int64)
    ok = True
    for z, pred, t in M.coded_blocks(coeffs, gray):
        c, syms, good = block_symbols(z, pred)
        ok &= good
        hist[t, c] += 1
        for s in syms:
            hist[2 + t, s] += 1
    return hist, ok


def symbol_counts_np(coeffs, gray=False):
    """the same counts in numpy, for frames too large for the per-block loop"""
    bpm = 4 if gray else 6
    co = np.asarray(coeffs, dtype=np.int64).reshape(-1, bpm, 64)
    nmcu = co.shape[0]
    hist = np.zeros((4, 256), np.int64)
    ok = True
    # DC: every component's blocks in scan order, the predictor is the previous one
    comps = [(co[:, :4, 0].reshape(-1), 0)]
    if not gray:
        comps += [(co[:, 4, 0], 1), (co[:, 5, 0], 1)]
    for dc, t in comps:
        d = np.diff(dc, prepend=0)
        cat = np.where(d == 0, 0, np.floor(np.log2(np.maximum(np.abs(d), 1))).astype(np.int64) + 1)
        ok &= bool((cat <= 11).all())
        hist[t] += np.bincount(np.minimum(cat, 11), minlength=256)
    if gray:
        hist[1, 0] += 2 * nmcu
        hist[3, 0] += 2 * nmcu
    # AC: for every non-zero coefficient the distance to the previous non-zero position (0: the DC)
    for t, blocks in ((0, co[:, :4].reshape(-1, 64)), (1, co[:, 4:].reshape(-1, 64))):
        if blocks.size == 0:
            continue
        nz = blocks != 0
        nz[:, 0] = False
        pos = np.arange(64)[None, :]
        last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)
        prev = np.concatenate([np.zeros((blocks.shape[0], 1), np.int64), last[:, :-1]], axis=1)
        run = (pos - prev - 1)[nz]
        a = np.abs(blocks[nz])
        size = np.floor(np.log2(a)).astype(np.int64) + 1
        ok &= bool((size <= 10).all())
        size = np.minimum(size, 10)
        hist[2 + t] += np.bincount(((run & 15) << 4) | size, minlength=256)
        hist[2 + t, 0xF0] += int((run >> 4).sum())
        hist[2 + t, 0x00] += int((last[:, 63] != 63).sum())
    return hist, ok


# ---- Annex K.2 ----
def optimal_table(freq):
    """(bits[16], vals, depth): Figures K.1 - K.4 with the reserved symbol 256, ties toward the larger symbol value, code sizes of
    any depth; depth is the longest code BEFORE Figure K.3 limits it to 16 (reserved symbol included)"""
    f = [int(x) for x in freq] + [1]
    if not any(f[:256]):
        return [0] * 16, [], 0
    codesize = [0] * 257
    others = [-1] * 257
    while True:
        c1 = c2 = -1
        v = None
        for i in range(257):
            if f[i] and (v is None or f[i] <= v):
                v, c1 = f[i], i
        v = None
        for i in range(257):
            if f[i] and i != c1 and (v is None or f[i] <= v):
                v, c2 = f[i], i
        if c2 < 0:
            break
        f[c1] += f[c2]
        f[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    depth = max(codesize)
    bits = [0] * 258
    for s in codesize:
        if s:
            bits[s] += 1
    for i in range(257, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [j for size in range(1, 258) for j in range(256) if codesize[j] == size]
    return bits[1:17], vals, depth


def codes(bits, vals):
    """{symbol: (code, length)}: the canonical codes of a DHT specification (Annex C)"""
    out = {}
    code = p = 0
    for length in range(1, 17):
        for _ in range(int(bits[length - 1])):
            out[int(vals[p])] = (code, length)
            code += 1
            p += 1
        code <<= 1
    return out


def lengths(bits):
    return [length for length in range(1, 17) for _ in range(int(bits[length - 1]))]


def frame_tables(coeffs, gray=False):
    """the frame's four optimal tables [(bits, vals)] in DHT order"""
    hist, ok = symbol_counts(coeffs, gray)
    assert ok
    return [optimal_table(hist[k])[:2] for k in range(4)]


# ---- the file ----
def header_with_tables(annex_k_file, tables):
    """the header (SOI .. SOS) of a file written with Annex-K tables, its four DHT segments replaced by `tables`"""
    data = bytes(annex_k_file)
    assert data[:2] == b"\xff\xd8"
    out, pos, k = bytearray(data[:2]), 2, 0
    while True:
        assert data[pos] == 0xFF
        marker, n = data[pos + 1], int.from_bytes(data[pos + 2:pos + 4], "big")
        if marker == 0xC4:
            bits, vals = tables[k]
            out += b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([TABLE_IDS[k]]) + bytes(int(b) for b in bits) + bytes(int(v) for v in vals)
            k += 1
        else:
            out += data[pos:pos + 2 + n]
        pos += 2 + n
        if marker == 0xDA:
            assert k == 4
            return bytes(out)


def entropy_segment(coeffs, gray, tables):
    """the stuffed entropy-coded segment of a frame coded with `tables` (zero pad bits)"""
    T = [codes(b, v) for b, v in tables]
    parts = []
    for z, pred, t in M.coded_blocks(coeffs, gray):
        c, syms, ok = block_symbols(z, pred)
        assert ok
        d = (0 if z is None else int(z[0])) - int(pred)
        parts.append(M._bits(*T[t][c]) + M._value_bits(d, c))
        nzv = [] if z is None else [int(v) for v in z[1:] if v != 0]
        it = iter(nzv)
        for s in syms:
            parts.append(M._bits(*T[2 + t][s]))
            if s not in (0x00, 0xF0):
                parts.append(M._value_bits(next(it), s & 15))
    s = "".join(parts)
    s += "0" * (-len(s) % 8)
    raw = bytes(int(s[i:i + 8], 2) for i in range(0, len(s), 8))
    return raw.replace(b"\xff", b"\xff\x00")


def write_jpeg(coeffs, gray, annex_k_file, tables=None):
    """the whole file with the frame's optimal tables (or `tables`): header of the Annex-K file with new DHT segments, scan, EOI"""
    tables = frame_tables(coeffs, gray) if tables is None else tables
    return header_with_tables(annex_k_file, tables) + entropy_segment(coeffs, gray, tables) + b"\xff\xd9"


def fibonacci_counts(n):
    """1, 2, 3, 5, 8, ...: the counts that make a Huffman tree as deep as it gets (n symbols plus the reserved one: depth n)"""
    out = [1, 2]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]
