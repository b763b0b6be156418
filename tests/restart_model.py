"""A bit-level model of a scan with restart intervals (ITU-T T.81 B.2.4.4 / E.1.4), built on tests/entropy_model.py and, for per-image
tables, tests/huffopt_model.py: per interval the block bit strings with the three predictors back at zero, the JPEZY_PAD_BIT fill up
to a byte, 0xFF00 stuffing, and the RSTn marker FF D0+(k mod 8) behind every interval but the last.

It is not the reference: tests/test_restart_host.py proves it equal to the host writer on random fields before it is used to
place interval ends on the GPU coder's seams (tests/test_gpu_restart.py), and every file is still read back by other readers.
"""
import re
from pathlib import Path

import numpy as np

import entropy_model as M
import huffopt_model as HM

ROOT = Path(__file__).resolve().parent.parent


def _define(path, name):
    m = re.search(rf"#define\s+{name}\s+(\d+)", (ROOT / path).read_text())
    assert m, f"{path} must define {name}"
    return int(m.group(1))


PAD_BIT = _define("include/jpezy_constants.h", "JPEZY_PAD_BIT")
MAX_COMMENT = _define("include/jpezy_hip.h", "JPEZY_MAX_COMMENT")
MAX_COMMENT_RESTART = _define("include/jpezy_hip.h", "JPEZY_MAX_COMMENT_RESTART")


def mcus(coeffs, gray=False):
    return np.asarray(coeffs).reshape(-1, 4 if gray else 6, 64)


def n_intervals(nmcu, ri):
    return -(-nmcu // ri) if ri else 1


def intervals(coeffs, ri, gray=False):
    """the MCUs of every restart interval, in order (ri = 0: the whole frame)"""
    co = mcus(coeffs, gray)
    step = ri if ri else co.shape[0]
    return [co[m:m + step] for m in range(0, co.shape[0], step)]


def _bitstring(co, gray, tables):
    """the bits of a run of MCUs coded from predictors of zero; tables: [(bits, vals)] x 4 in DHT order, None for Annex K"""
    if tables is None:
        return M.frame_bitstring(co, gray)
    T = [HM.codes(b, v) for b, v in tables]
    parts = []
    for z, pred, t in M.coded_blocks(co, gray):
        c, syms, ok = HM.block_symbols(z, pred)
        assert ok
        d = (0 if z is None else int(z[0])) - int(pred)
        parts.append(M._bits(*T[t][c]) + M._value_bits(d, c))
        it = iter([] if z is None else [int(v) for v in z[1:] if v != 0])
        for s in syms:
            parts.append(M._bits(*T[2 + t][s]))
            if s not in (0x00, 0xF0):
                parts.append(M._value_bits(next(it), s & 15))
    return "".join(parts)


def interval_bitstrings(coeffs, ri, gray=False, tables=None):
    return [_bitstring(co, gray, tables) for co in intervals(coeffs, ri, gray)]


def interval_bits(coeffs, ri, gray=False, tables=None):
    """coded bits of every interval, before padding"""
    return [len(s) for s in interval_bitstrings(coeffs, ri, gray, tables)]


def padded(bits, pad_bit=PAD_BIT):
    bits += str(pad_bit) * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def unstuffed_intervals(coeffs, ri, gray=False, tables=None, pad_bit=PAD_BIT):
    """every interval's bytes before stuffing (what the GPU coder's unstuffed stream U is the concatenation of)"""
    return [padded(s, pad_bit) for s in interval_bitstrings(coeffs, ri, gray, tables)]


def scan(coeffs, ri, gray=False, tables=None, pad_bit=PAD_BIT):
    """the entropy-coded segment as the file holds it, between the SOS header and EOI"""
    parts = unstuffed_intervals(coeffs, ri, gray, tables, pad_bit)
    out = bytearray()
    for k, p in enumerate(parts):
        out += p.replace(b"\xff", b"\xff\x00")
        if k + 1 < len(parts):
            out += bytes([0xFF, 0xD0 + k % 8])
    return bytes(out)


def symbol_counts(coeffs, ri, gray=False):
    """tests/huffopt_model.py's counts with the predictors reset at every interval's start"""
    hist = np.zeros((4, 256), np.int64)
    ok = True
    for co in intervals(coeffs, ri, gray):
        h, good = HM.symbol_counts(co, gray)
        hist += h
        ok &= good
    return hist, ok


def frame_tables(coeffs, ri, gray=False):
    hist, ok = symbol_counts(coeffs, ri, gray)
    assert ok
    return [HM.optimal_table(hist[k])[:2] for k in range(4)]


# ---- reading a file back ----
def split(jpg):
    """(header up to and including the SOS segment, entropy-coded segment still stuffed and with its markers) of a file"""
    jpg = bytes(jpg)
    sos = jpg.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")
    assert jpg[-2:] == b"\xff\xd9"
    return jpg[:start], jpg[start:-2]


def dri_of(jpg):
    """(offset of the DRI segment, its interval), or (None, 0); the segment must stand directly in front of SOS"""
    hdr, _ = split(jpg)
    sos = hdr.index(b"\xff\xda")
    if hdr[sos - 6:sos - 2] != b"\xff\xdd\x00\x04":
        assert b"\xff\xdd" not in hdr[2:sos]
        return None, 0
    return sos - 6, int.from_bytes(hdr[sos - 2:sos], "big")


def markers(segment):
    """the markers inside an entropy-coded segment, in order: every 0xFF that no 0x00 follows"""
    seg = bytes(segment)
    return [seg[i + 1] for i in range(len(seg) - 1) if seg[i] == 0xFF and seg[i + 1] != 0x00]


def expected_markers(nmcu, ri):
    return [0xD0 + k % 8 for k in range(n_intervals(nmcu, ri) - 1)]


# ---- builders ----
def flat_mcu(gray=False):
    """an MCU of zero blocks: 32 bits with the Annex-K tables -- the shortest interval there is"""
    return np.zeros((4 if gray else 6, 64), np.int16)


def mcu_of_bits(bits, gray=False):
    """an MCU of exactly `bits` coded bits after predictors of zero (Annex K): five flat blocks (26 bits) and M.tuner_block in luma
    block 0; None where no such block exists"""
    z = M.tuner_block(bits - 26, 0)
    if z is None:
        return None
    mcu = flat_mcu(gray)
    mcu[0] = z
    return mcu
