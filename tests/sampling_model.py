"""Test helper: the definition of the encoder's 4:4:4 chroma sampling (include/jpezy_hip.h) restated with numpy, the
oracle's own block transform and the bit-level models of the scan (tests/entropy_model.py, huffopt_model.py, restart_model.py).

Coefficients: the picture is extended to whole 8 x 8 MCUs by clamping the pixel coordinates (ref encoder/jpezy_encoder.hpp:101,104); Y, Cb
and Cr of EVERY pixel in the reference's FP64 order (:244-256), truncating -- nothing of make_YCC:116-143 --; every block through
quant_model.fdct_blocks (the oracle's jo_fdct_block) and C's truncating division by the tables (Y: luma, Cb / Cr: chroma); zig-zag order;
int16 [mcu_rows, mcu_cols, 3, 64].

File: the oracle writer's header for the same size and comment with (a) SOF0 stating H, V = 1,1 for all three components, (b) the DQT /
DHT segments given, (c) a DRI segment in front of SOS; then the scan of 3-block MCUs -- Y with the luma tables, Cb / Cr with the chroma
ones, one DC predictor per component, reset at every restart interval's start --, intervals padded, stuffed and separated by RSTn.

It is not the reference (which writes 4:2:0 only): tests/test_sampling_host.py ties it to the 4:2:0 definition wherever the two share a
sample and reads every file back.
"""
import functools

import numpy as np

import entropy_model as M
import huffopt_model as HM
import quant_model as QM
import restart_model as RM
from jpeg_synth import ZZ

SAMPLING_420, SAMPLING_444 = 0, 1


def geometry(W, H):
    """(mcu_cols, mcu_rows, blocks_per_mcu)"""
    return (W + 7) // 8, (H + 7) // 8, 3


def samples_from_rgb(r, g, b, W, H):
    """planar uint8 -> (ys, cbs, crs): int32 sample planes (mr*8, mc*8) of the clamp-extended picture, every pixel converted"""
    mc, mr, _ = geometry(W, H)
    rows, cols = np.minimum(np.arange(mr * 8), H - 1), np.minimum(np.arange(mc * 8), W - 1)
    r, g, b = (np.asarray(p, dtype=np.uint8).reshape(H, W)[np.ix_(rows, cols)].astype(np.float64) for p in (r, g, b))
    ys = np.trunc((0.2990 * r) + (0.5870 * g) + (0.1140 * b) - 128).astype(np.int32)
    cbs = np.trunc(-(0.1687 * r) - (0.3313 * g) + (0.5000 * b)).astype(np.int32)
    crs = np.trunc((0.5000 * r) - (0.4187 * g) - (0.0813 * b)).astype(np.int32)
    return ys, cbs, crs


def dct_from_rgb(r, g, b, W, H):
    """planar uint8 r, g, b -> the unquantised DCT of every block, int32 [mr, mc, 3, 64] natural order"""
    mc, mr, _ = geometry(W, H)
    out = np.zeros((mr * mc, 3, 64), np.int32)
    for k, p in enumerate(samples_from_rgb(r, g, b, W, H)):
        out[:, k] = QM.fdct_blocks(p.reshape(mr, 8, mc, 8).transpose(0, 2, 1, 3).reshape(mr * mc, 64))
    return out.reshape(mr, mc, 3, 64)


def quantise(dct, luma, chroma):
    """unquantised DCT [..., 3, 64] natural order -> int16 zig-zag coefficients: C's truncating division (block 0 luma, 1 and 2 chroma)"""
    d = np.asarray(dct, np.int64)
    q = np.empty((3, 64), np.int64)
    q[0] = np.asarray(luma, np.int64).reshape(64)
    q[1:] = np.asarray(chroma, np.int64).reshape(64)
    out = np.sign(d) * (np.abs(d) // q)
    return out[..., ZZ].astype(np.int16)


def encode_coeffs(r, g, b, W, H, luma, chroma):
    return quantise(dct_from_rgb(r, g, b, W, H), luma, chroma)


@functools.lru_cache(maxsize=None)
def synth_dct(W, H, frame=0):
    """dct_from_rgb(oracle.synth_rgb(W, H, frame)), computed once and shared; read-only"""
    from oracle import oracle as O
    d = dct_from_rgb(*O.synth_rgb(W, H, frame=frame), W, H)
    d.setflags(write=False)
    return d


# ---- the scan ----
def coded_blocks(coeffs):
    """(z, pred, table) of every coded block, in stream order, from predictors of zero; coeffs [nmcu, 3, 64]"""
    co = np.asarray(coeffs).reshape(-1, 3, 64)
    pred = [0, 0, 0]
    for m in range(co.shape[0]):
        for i in range(3):
            yield co[m, i], pred[i], 0 if i == 0 else 1
            pred[i] = int(co[m, i, 0])


def _bitstring(co, tables):
    """the bits of a run of MCUs coded from predictors of zero; tables: [(bits, vals)] x 4 in DHT order, None for Annex K"""
    if tables is None:
        return "".join(M.block_bitstring(z, p, t) for z, p, t in coded_blocks(co))
    T = [HM.codes(b, v) for b, v in tables]
    parts = []
    for z, pred, t in coded_blocks(co):
        c, syms, ok = HM.block_symbols(z, pred)
        assert ok
        parts.append(M._bits(*T[t][c]) + M._value_bits(int(z[0]) - int(pred), c))
        it = iter([int(v) for v in z[1:] if v != 0])
        for s in syms:
            parts.append(M._bits(*T[2 + t][s]))
            if s not in (0x00, 0xF0):
                parts.append(M._value_bits(next(it), s & 15))
    return "".join(parts)


def intervals(coeffs, ri):
    co = np.asarray(coeffs).reshape(-1, 3, 64)
    step = ri if ri else co.shape[0]
    return [co[m:m + step] for m in range(0, co.shape[0], step)]


def scan(coeffs, ri, tables=None):
    """the entropy-coded segment as the file holds it, between the SOS header and EOI"""
    parts = [RM.padded(_bitstring(co, tables)) for co in intervals(coeffs, ri)]
    out = bytearray()
    for k, p in enumerate(parts):
        out += p.replace(b"\xff", b"\xff\x00")
        if k + 1 < len(parts):
            out += bytes([0xFF, 0xD0 + k % 8])
    return bytes(out)


def symbol_counts(coeffs, ri=0):
    """hist[4][256] (DHT order YDc, CDc, YAc, CAc) of the symbols the scan emits, and whether every value was in range"""
    hist = np.zeros((4, 256), np.int64)
    ok = True
    for co in intervals(coeffs, ri):
        for z, pred, t in coded_blocks(co):
            c, syms, good = HM.block_symbols(z, pred)
            ok &= good
            hist[t, c] += 1
            for s in syms:
                hist[2 + t, s] += 1
    return hist, ok


def frame_tables(coeffs, ri=0):
    hist, ok = symbol_counts(coeffs, ri)
    assert ok
    return [HM.optimal_table(hist[k])[:2] for k in range(4)]


# ---- the file ----
def header(W, H, comment=None, quant_tables=None, tables=None, ri=0):
    """SOI .. SOS: the oracle's 4:2:0 header for (W, H, comment) with the 4:4:4 sampling factors, the given DQT / DHT segments and DRI"""
    from oracle import oracle as O
    mc, mr = O.mcu_grid(W, H)
    base, _ = RM.split(O.write_jpeg(np.zeros((mr, mc, 6, 64), np.int16), W, H, False, comment))
    out, pos, k = bytearray(base[:2]), 2, 0
    while pos < len(base):
        assert base[pos] == 0xFF
        marker, n = base[pos + 1], int.from_bytes(base[pos + 2:pos + 4], "big")
        seg = bytearray(base[pos:pos + 2 + n])
        if marker == 0xDB and quant_tables is not None:
            assert n == 67 and seg[4] in (0, 1)
            seg[5:] = bytes(int(v) for v in np.asarray(quant_tables[seg[4]]).reshape(64)[ZZ])
        elif marker == 0xC4 and tables is not None:
            bits, vals = tables[k]
            seg = bytearray(b"\xff\xc4" + (19 + len(vals)).to_bytes(2, "big") + bytes([HM.TABLE_IDS[k]]) + bytes(int(b) for b in bits) +
                            bytes(int(v) for v in vals))
            k += 1
        elif marker == 0xC0:
            assert seg[9] == 3 and seg[11] == 0x22 and seg[14] == 0x11 and seg[17] == 0x11
            seg[11] = 0x11
        elif marker == 0xDA and ri:
            out += b"\xff\xdd\x00\x04" + int(ri).to_bytes(2, "big")
        out += seg
        pos += 2 + n
    return bytes(out)


def write_jpeg(coeffs, W, H, comment=None, quant_tables=None, ri=0, optimize=False):
    """the whole 4:4:4 file for coefficients [mr, mc, 3, 64]"""
    tables = frame_tables(coeffs, ri) if optimize else None
    return header(W, H, comment, quant_tables, tables, ri) + scan(coeffs, ri, tables) + b"\xff\xd9"
