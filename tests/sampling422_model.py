"""Test helper: the definition of the encoder's 4:2:2 chroma sampling (include/jpezy_hip.h) restated with numpy, the
oracle's own block transform and the bit-level models of the scan (tests/entropy_model.py, huffopt_model.py, restart_model.py).

Coefficients: the picture is extended to whole 16 x 8 MCUs by clamping the pixel coordinates; Y of every pixel; Cb and Cr of every pixel
in the reference's FP64 order, truncating, then decimated horizontally only -- point sampling takes pixel 2 x' (make_YCC's rule in one
direction), the averaged rule is (c[2 x'] + c[2 x' + 1] + bias(x')) >> 1 with bias 0 / 1 for even / odd x' and an arithmetic shift
(libjpeg's h2v1_downsample on signed samples) --; every block through quant_model.fdct_blocks (the oracle's jo_fdct_block) and C's
truncating division by the tables (Y: luma, Cb / Cr: chroma); zig-zag order; int16 [mcu_rows, mcu_cols, 4, 64], blocks Y-left, Y-right,
Cb, Cr.

File: the oracle writer's header for the same size and comment with (a) SOF0 stating H, V = 2,1 / 1,1 / 1,1, (b) the DQT / DHT segments
given, (c) a DRI segment in front of SOS; then the scan of 4-block MCUs -- the two Y blocks with the luma tables and one running
predictor, Cb / Cr with the chroma ones and a predictor each, all reset at every restart interval's start --, intervals padded, stuffed
and separated by RSTn.

It is not the reference (which writes 4:2:0 only): tests/test_sampling422_host.py ties it to the 4:4:4 and 4:2:0 definitions wherever they
share a sample and reads every file back.
"""
import functools

import numpy as np

import entropy_model as M
import huffopt_model as HM
import quant_model as QM
import restart_model as RM
import sampling_model as SM
from jpeg_synth import ZZ

SAMPLING_422 = 3
POINT, AVERAGE = 0, 1


def geometry(W, H):
    """(mcu_cols, mcu_rows, blocks_per_mcu)"""
    return (W + 15) // 16, (H + 7) // 8, 4


def h2v1_average(c):
    """[rows, 2 n] signed per-pixel samples -> [rows, n]: (a + b + bias) >> 1, bias 0 for even, 1 for odd output columns, floor shift"""
    c = np.asarray(c, np.int32)
    bias = (np.arange(c.shape[1] // 2) & 1).astype(np.int32)
    return (c[:, 0::2] + c[:, 1::2] + bias) >> 1


def samples_from_rgb(r, g, b, W, H, mode=POINT):
    """planar uint8 -> (ys, cbs, crs): int32 planes of the clamp-extended picture, ys (mr*8, mc*16), cbs / crs (mr*8, mc*8)"""
    mc, mr, _ = geometry(W, H)
    rows, cols = np.minimum(np.arange(mr * 8), H - 1), np.minimum(np.arange(mc * 16), W - 1)
    r, g, b = (np.asarray(p, dtype=np.uint8).reshape(H, W)[np.ix_(rows, cols)].astype(np.float64) for p in (r, g, b))
    ys = np.trunc((0.2990 * r) + (0.5870 * g) + (0.1140 * b) - 128).astype(np.int32)
    cbs = np.trunc(-(0.1687 * r) - (0.3313 * g) + (0.5000 * b)).astype(np.int32)
    crs = np.trunc((0.5000 * r) - (0.4187 * g) - (0.0813 * b)).astype(np.int32)
    if mode == AVERAGE:
        return ys, h2v1_average(cbs), h2v1_average(crs)
    assert mode == POINT
    return ys, cbs[:, 0::2], crs[:, 0::2]


def _blocks(plane, mr, n):
    """(mr*8, n*8) plane -> [mr, n, 64]"""
    return plane.reshape(mr, 8, n, 8).transpose(0, 2, 1, 3).reshape(mr, n, 64)


def dct_from_rgb(r, g, b, W, H, mode=POINT):
    """planar uint8 r, g, b -> the unquantised DCT of every block, int32 [mr, mc, 4, 64] natural order"""
    mc, mr, _ = geometry(W, H)
    ys, cbs, crs = samples_from_rgb(r, g, b, W, H, mode)
    out = np.zeros((mr, mc, 4, 64), np.int32)
    out[:, :, 0:2] = QM.fdct_blocks(_blocks(ys, mr, 2 * mc).reshape(-1, 64)).reshape(mr, mc, 2, 64)
    out[:, :, 2] = QM.fdct_blocks(_blocks(cbs, mr, mc).reshape(-1, 64)).reshape(mr, mc, 64)
    out[:, :, 3] = QM.fdct_blocks(_blocks(crs, mr, mc).reshape(-1, 64)).reshape(mr, mc, 64)
    return out


def quantise(dct, luma, chroma):
    """unquantised DCT [..., 4, 64] natural order -> int16 zig-zag coefficients: C's truncating division (blocks 0, 1 luma, 2, 3 chroma)"""
    d = np.asarray(dct, np.int64)
    q = np.empty((4, 64), np.int64)
    q[:2] = np.asarray(luma, np.int64).reshape(64)
    q[2:] = np.asarray(chroma, np.int64).reshape(64)
    out = np.sign(d) * (np.abs(d) // q)
    return out[..., ZZ].astype(np.int16)


def encode_coeffs(r, g, b, W, H, luma, chroma, mode=POINT):
    return quantise(dct_from_rgb(r, g, b, W, H, mode), luma, chroma)


@functools.lru_cache(maxsize=None)
def synth_dct(W, H, frame=0, mode=POINT):
    """dct_from_rgb(oracle.synth_rgb(W, H, frame)), computed once and shared; read-only"""
    from oracle import oracle as O
    d = dct_from_rgb(*O.synth_rgb(W, H, frame=frame), W, H, mode)
    d.setflags(write=False)
    return d


# ---- the scan ----
def coded_blocks(coeffs):
    """(z, pred, table) of every coded block, in stream order, from predictors of zero; coeffs [nmcu, 4, 64]"""
    co = np.asarray(coeffs).reshape(-1, 4, 64)
    pred = [0, 0, 0]                       # Y (running through both luma blocks), Cb, Cr
    for m in range(co.shape[0]):
        for i in range(4):
            comp = max(0, i - 1)
            yield co[m, i], pred[comp], 0 if i < 2 else 1
            pred[comp] = int(co[m, i, 0])


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
    co = np.asarray(coeffs).reshape(-1, 4, 64)
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
    """SOI .. SOS: the 4:4:4 model's header (the oracle's with the DQT / DHT / DRI segments given) with SOF0's luma factors 2, 1"""
    base = bytearray(SM.header(W, H, comment, quant_tables, tables, ri))
    pos = 2
    while pos < len(base):
        assert base[pos] == 0xFF
        marker, n = base[pos + 1], int.from_bytes(base[pos + 2:pos + 4], "big")
        if marker == 0xC0:
            assert base[pos + 9] == 3 and base[pos + 11] == 0x11 and base[pos + 14] == 0x11 and base[pos + 17] == 0x11
            base[pos + 11] = 0x21
            return bytes(base)
        pos += 2 + n
    raise AssertionError("no SOF0")


def write_jpeg(coeffs, W, H, comment=None, quant_tables=None, ri=0, optimize=False):
    """the whole 4:2:2 file for coefficients [mr, mc, 4, 64]"""
    tables = frame_tables(coeffs, ri) if optimize else None
    return header(W, H, comment, quant_tables, tables, ri) + scan(coeffs, ri, tables) + b"\xff\xd9"
