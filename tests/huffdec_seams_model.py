"""Constructions for the GPU Huffman decoder's seams (tests/test_gpu_huffdec_seams.py; proved on the CPU by
tests/test_huffdec_seams_model.py).  A bit-level model of a baseline scan -- every symbol of a frame with its bit offset in the
unstuffed stream, its kind, its block and the decoder's zig-zag index in front of it -- and builders that put a chosen symbol,
stuffing byte or block end on a chosen boundary of the decoder (jpezy_huffdec.hip): 64-byte unstuffing chunks and the 256-chunk
workgroups of the copy kernel, 1,024-bit subsequences, their quarter marks, the coefficient pass's 64-subsequence workgroups and
the synchronisation's 256-lane workgroups.  Every builder asserts from the symbol table that it landed where it says.

It is not the reference: the ground truth of a case is the coefficient field it was built from, and the file is written by the
host writer (jpezy's own 4:2:0 and gray layouts, checked with entropy_model) or by jpeg_synth.synth_jpeg (other layouts and tables).

The filler between the seams is random: sparse blocks that end in an EOB, and one block of an exact coded length (all 63 AC
positions non-zero, categories drawn at random from a knapsack table) in front of every aimed symbol.  Nothing repeats: a periodic
stream is by design the host decoder's (ScanState::periodic, scan_hopeless).  Where the MCU's table sequence has a period the
filler blocks are short (Builder.__init__ says why): a decoder started on a guess must find the MCU phase inside its warm-up.

Longest blocks: 16 + 15 bits is the longest symbol the decoder takes (a DC category 16 is the host decoder's), so no block exceeds
31 + 63 * 31 = 1,984 bits: a block longer than two subsequences (2,048 bits) cannot exist.  Annex K reaches 1,660 bits
(entropy_model.WORST_BLOCK_BITS), long_tables() 1,984."""
import bisect
import copy
import re
from functools import lru_cache
from pathlib import Path

import numpy as np

import entropy_model as M
from jpeg_synth import annex_k_tables, canonical, synth_jpeg, table_of, wide_tables

ROOT = Path(__file__).resolve().parent.parent
HUFFDEC_HIP = ROOT / "jpezy_amd" / "csrc" / "jpezy_huffdec.hip"
CAPI_HUFFDEC_HIP = ROOT / "jpezy_amd" / "csrc" / "jpezy_capi_huffdec.hip"


# ---- the decoder's geometry, read from its source ----
def read_geometry():
    src = HUFFDEC_HIP.read_text()

    def num(pattern):
        m = re.search(pattern, src)
        assert m, f"jpezy_huffdec.hip no longer has {pattern!r}"
        return int(m.group(1))
    sub = num(r"#define\s+JPEZY_SUBSEQ_BITS\s+(\d+)")
    return {
        "JPEZY_SUBSEQ_BITS": sub,
        "WGS": num(r"constexpr int WGS = (\d+);"),
        "EMIT_PARTS": num(r"constexpr int EMIT_PARTS = (\d+),"),
        "CHUNK": num(r"constexpr int CHUNK = (\d+);"),
        "OVERFLOW_DEFAULT": num(r"constexpr int OVERFLOW_DEFAULT = (\d+) \* 1024 / SUBSEQ_BITS;") * 1024 // sub,
        "OVERFLOW": num(r"constexpr int OVERFLOW = (\d+) \* 1024 / SUBSEQ_BITS;") * 1024 // sub,
        "DC_PER_WG": num(r"constexpr int DC_PER_WG = (\d+);"),
        "COPY_WG_CHUNKS": num(r"__shared__ uint32_t buf\[(\d+) \* CHUNK / 4 \+ 4\];"),          # chunks of a workgroup of unstuff_copy_kernel
        "PER_LANE_LIMIT": int(re.search(r"per_lane = n_int >= 1 && n_all / n_int <= (\d+);", CAPI_HUFFDEC_HIP.read_text()).group(1)),
    }


# what the constructions below were written for: tests/test_huffdec_seams_model.py fails when the source says anything else
EXPECTED_GEOMETRY = {"JPEZY_SUBSEQ_BITS": 1024, "WGS": 256, "EMIT_PARTS": 4, "CHUNK": 64, "OVERFLOW_DEFAULT": 3, "OVERFLOW": 12,
                     "DC_PER_WG": 2048, "COPY_WG_CHUNKS": 256, "PER_LANE_LIMIT": 4096}
GEOMETRY = read_geometry()
SUBSEQ_BITS = GEOMETRY["JPEZY_SUBSEQ_BITS"]
WGS = GEOMETRY["WGS"]
EMIT_PARTS = GEOMETRY["EMIT_PARTS"]
CHUNK = GEOMETRY["CHUNK"]
OVERFLOW_DEFAULT = GEOMETRY["OVERFLOW_DEFAULT"]
OVERFLOW = GEOMETRY["OVERFLOW"]
DC_PER_WG = GEOMETRY["DC_PER_WG"]
PART_BITS = SUBSEQ_BITS // EMIT_PARTS
EMIT_SUBS = WGS // EMIT_PARTS                      # subsequences of a coefficient-pass workgroup
COPY_WG_BYTES = GEOMETRY["COPY_WG_CHUNKS"] * CHUNK                      # stuffed bytes of a workgroup of the unstuffing copy kernel
PAD_BIT = int(re.search(r"#define\s+JPEZY_PAD_BIT\s+(\d)", (ROOT / "include" / "jpezy_constants.h").read_text()).group(1))


# ---- layouts ----
@lru_cache(maxsize=None)
def _annex_k():
    return annex_k_tables()


def long_tables():
    """wide_tables() with the run-0 codes of sizes 11..15 at 16 bits as well: every coefficient of a block can then be a 31-bit
    symbol (blocks of up to 31 + 63 * 31 = 1,984 bits).  All codes of more than 10 bits start with six ones, as in wide_tables()."""
    dc = [(c, c + 1) for c in range(6)] + [(c, 12) for c in range(6, 12)] + [(12, 14), (13, 14), (14, 16), (15, 16), (16, 16)]
    base = [0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
    ac = [(0x00, 1)] + [(sym, 8 if i < 100 else 9 if i < 135 else 10) for i, sym in enumerate(base)]
    ac += [((r << 4) | s, 16) for r in range(0, 16) for s in range(11, 16)]
    d, a = table_of(dc), table_of(ac)
    return {(0, 0): d, (0, 1): d, (1, 0): a, (1, 1): a}


def dense_tables():
    """wide_tables() with the code space above the 10-bit codes filled to its last code but one: 31 codes of 11 bits, one each of
    12..15 bits, and run 0 / size 15 at 16 bits -- 1111111111111110, the code with the most one bits a table may have.  A block of
    +32767 everywhere is then 30 one bits and a zero for ever: three 0xFF in every 31 bits, the most stuffing a stream can hold."""
    w = wide_tables()
    base = [0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]
    ac = [(0x00, 1)] + [(sym, 8 if i < 100 else 9 if i < 135 else 10) for i, sym in enumerate(base)]
    ac += [((r << 4) | s, 11) for r in range(1, 16) for s in range(11, 16)][:31]
    ac += [(11, 12), (12, 13), (13, 14), (14, 15), (15, 16)]
    a = table_of(ac)
    assert canonical(*a)[15] == (0xFFFE, 16)
    return {(0, 0): w[(0, 0)], (0, 1): w[(0, 1)], (1, 0): a, (1, 1): a}


class Layout:
    """comps: [(H, V, Tq, Td)] as synth_jpeg takes them.  writer: 'own' / 'own_gray' (the host writer, Annex K, pad bit
    JPEZY_PAD_BIT; gray codes two zero chroma blocks per MCU) or 'synth' (jpeg_synth, pad bits one)."""

    def __init__(self, name, comps, tables=None, writer="synth"):
        self.name, self.comps, self.tables, self.writer = name, comps, tables, writer
        tabs = _annex_k() if tables is None else tables
        self.enc = {k: canonical(*v) for k, v in tabs.items()}
        self.seq = [td for (h, v, _, td) in comps for _ in range(h * v)]          # table selector of every block of an MCU
        self.comp = [ci for ci, (h, v, _, _) in enumerate(comps) for _ in range(h * v)]
        self.bpm = len(self.seq)
        self.period = next(p for p in range(1, self.bpm + 1)
                           if self.bpm % p == 0 and all(self.seq[i] == self.seq[i - p] for i in range(p, self.bpm)))
        self.mcu_w = 8 * max(c[0] for c in comps)
        self.mcu_h = 8 * max(c[1] for c in comps)
        self.forced_zero = {4, 5} if writer == "own_gray" else set()
        self.pad_bit = 1 if writer == "synth" else PAD_BIT

    def __repr__(self):
        return self.name

    def fits(self, nmcu):
        try:
            return bool(self.grid(nmcu))
        except AssertionError:
            return False

    def grid(self, nmcu):
        """(mcu_cols, mcu_rows) of a frame of exactly nmcu MCUs inside 65,535 x 65,535"""
        most = 65535 // max(self.mcu_w, self.mcu_h)
        for cols in range(min(nmcu, most), 0, -1):
            if nmcu % cols == 0 and nmcu // cols <= most:
                return cols, nmcu // cols
        raise AssertionError(f"{nmcu} MCUs fit no frame")


YUV420 = [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]
LAYOUTS = {
    "own420": Layout("own420", YUV420, writer="own"),                                        # table period 6
    "own_gray": Layout("own_gray", YUV420, writer="own_gray"),                               # period 6, chroma blocks all zero
    "s444": Layout("s444", [(1, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]),                      # period 3
    "shared": Layout("shared", [(1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 0)]),                  # three components, one table pair: period 1
    "one": Layout("one", [(1, 1, 0, 0)]),                                                    # one component
    # (wide_tables() has ONE table pair under both selectors: with Td (0, 1, 1) no decoder could tell the MCU phase from the stream, two
    # of three guesses would stay wrong for ever and the file would be the host decoder's by scan_hopeless -- so one selector, period 1)
    "wide444": Layout("wide444", [(1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 1, 0)], tables=wide_tables()),
    "long_one": Layout("long_one", [(1, 1, 0, 0)], tables=long_tables()),
    "dense_one": Layout("dense_one", [(1, 1, 0, 0)], tables=dense_tables()),
}
ANNEX_LAYOUTS = ["own420", "own_gray", "s444", "shared", "one"]
assert [LAYOUTS[n].period for n in ANNEX_LAYOUTS] == [6, 6, 3, 1, 1]


# ---- one block ----
def _bits(value, n):
    return format(value & ((1 << n) - 1), f"0{n}b") if n else ""


def _cat(v):
    return int(abs(int(v))).bit_length()


def _vbits(v, s):
    return _bits(v if v >= 0 else v - 1, s)


_CODE_STRINGS = {}


def _strings(table):
    """{symbol: its code as a bit string} of a table of (code, length) pairs (kept per table object: the layouts own them)"""
    got = _CODE_STRINGS.get(id(table))
    if got is None or got[0] is not table:
        got = _CODE_STRINGS[id(table)] = (table, {sym: _bits(code, ln) for sym, (code, ln) in table.items()})
    return got[1]


def encode_block(z, pred, dc_t, ac_t, end_with_zrl=False):
    """-> ([(nbits, kind, k, n)], bit string): every symbol of the block with the decoder's zig-zag index k in front of it (0: a DC
    symbol) and the position n it codes (-1: ZRL, EOB).  end_with_zrl: the zero run that ends the block is coded with ZRL symbols in
    place of the EOB (what no encoder writes: the decoders' edge k + 16 == 64 and the refusal one position further)."""
    dcs, acs = _strings(dc_t), _strings(ac_t)
    zl = z.tolist() if hasattr(z, "tolist") else list(z)
    d = zl[0] - int(pred)
    c = abs(d).bit_length()
    code = dcs[c]
    syms, parts = [(len(code) + c, "DC", 0, 0)], [code + _vbits(d, c)]
    k = 1
    for n in range(1, 64):
        v = zl[n]
        if not v:
            continue
        run = n - k
        while run > 15:
            code = acs[0xF0]
            syms.append((len(code), "ZRL", k, -1))
            parts.append(code)
            k += 16
            run -= 16
        s = abs(v).bit_length()
        code = acs[(run << 4) | s]
        syms.append((len(code) + s, "AC", k, n))
        parts.append(code + format((v if v >= 0 else v - 1) & ((1 << s) - 1), "b").zfill(s))
        k = n + 1
    if k <= 63:
        code = acs[0xF0 if end_with_zrl else 0x00]
        syms.append((len(code), "ZRL" if end_with_zrl else "EOB", k, -1))
        parts.append(code)
    return syms, "".join(parts)


class Symbols:
    """the symbols of a frame: starts[i] (bit offset in the unstuffed stream), recs[i] = (nbits, kind, block, k, n)"""

    def __init__(self, starts, recs, total_bits, nblocks, period):
        self.starts, self.recs, self.total_bits, self.nblocks, self.period = starts, recs, total_bits, nblocks, period

    def state_at(self, pos):
        """the true decoder state at bit `pos`: (p, b, k, blocks completed before it) -- p: offset from pos of the first code word at
        or behind it, b: its block inside the table period, k: the zig-zag index in front of it"""
        i = bisect.bisect_left(self.starts, pos)
        if i == len(self.starts):
            return self.total_bits - pos, self.nblocks % self.period, 0, self.nblocks
        _, _, block, k, _ = self.recs[i]
        return self.starts[i] - pos, block % self.period, k, block

    def at(self, start):
        i = bisect.bisect_left(self.starts, start)
        assert i < len(self.starts) and self.starts[i] == start, f"no symbol starts at bit {start}"
        return self.recs[i]

    def covering(self, pos):
        """index of the symbol that holds bit pos"""
        return bisect.bisect_right(self.starts, pos) - 1


def stuffed(stream):
    return bytes(stream).replace(b"\xff", b"\xff\x00")


def removed_before(stream, offset):
    """stuffing bytes that lie in front of offset `offset` of the STUFFED stream"""
    ff = M.ff_positions(stream)
    return int(np.count_nonzero(ff + np.arange(len(ff)) + 1 < offset))


def stuffed_offset(stream, u):
    """offset in the stuffed stream of unstuffed byte u"""
    return u + int(np.count_nonzero(M.ff_positions(stream) < u))


def entropy_segment(jpg):
    """the entropy-coded bytes of a one-scan file as they stand (stuffed, restart markers included): SOS header to the EOI"""
    jpg = bytes(jpg)
    sos = jpg.index(b"\xff\xda")
    start = sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")
    end = jpg.rindex(b"\xff\xd9")
    return jpg[start:end]


# ---- blocks of an exact coded length ----
@lru_cache(maxsize=None)
def _reach(costs):
    """R[k][b]: b bits can be made of k run-0 coefficients with the (size, cost) pairs of `costs`"""
    top = 63 * max(c for _, c in costs)
    R = np.zeros((64, top + 1), bool)
    R[0, 0] = True
    for k in range(63):
        for _, c in costs:
            R[k + 1, c:] |= R[k, :top + 1 - c]
    return R


def _costs(ac_t):
    return tuple((s, ac_t[s][1] + s) for s in range(1, 16) if s in ac_t)


def exact_ac(ac_t, rest, rng):
    """63 non-zero AC coefficients (no run, no EOB) of exactly `rest` coded bits, categories and values at random; None if impossible"""
    costs = _costs(ac_t)
    R = _reach(costs)
    if rest < 0 or rest >= R.shape[1] or not R[63, rest]:
        return None
    z = np.zeros(64, np.int16)
    b = rest
    for k in range(63, 0, -1):
        ok = [(s, c) for s, c in costs if c <= b and R[k - 1, b - c]]
        s, c = ok[int(rng.integers(len(ok)))]
        mag = int(rng.integers(1 << (s - 1), 1 << s))
        z[k] = mag if rng.random() < 0.5 else -mag
        b -= c
    assert b == 0
    return z


# ---- the stream under construction ----
class Builder:
    def __init__(self, layout, seed=0, density=0.25, amp=60):
        self.L = layout
        self.rng = np.random.default_rng(seed)
        # A decoder started on a guess finds the MCU phase only by walking several MCUs (each change of table throws it out of step, and
        # it falls back into step in a phase that is right by chance).  Where the table sequence has a long period the filler is
        # therefore one coefficient of +-1 per block -- some 200 bits per MCU --, so that even the warm-up of a speculation distance of
        # one subsequence (JPEZY_HUFFDEC_OVERFLOW=1) holds several MCUs: speculation_misses() then finds a fifth of the lanes starting
        # wrong, against more than half with blocks of 100 bits and more, which scan_hopeless hands to the host decoder
        # (test_light_filler_finds_the_mcu_phase_within_one_subsequence).
        self.light = layout.period > 3
        self.density, self.amp, self.bulk_density, self.bulk_amp = density, amp, 0.5, 1000
        if layout.period == 3:
            self.amp, self.bulk_density, self.bulk_amp = 4, density, 4
        self._pool, self._pool_at = None, 0
        self.blocks, self.parts, self.starts, self.recs = [], [], [], []
        self.bits = 0
        self.pred = [0] * len(layout.comps)
        self.landed = []

    def clone(self):
        b = copy.copy(self)
        b.rng = copy.deepcopy(self.rng)
        for name in ("blocks", "parts", "starts", "recs", "pred", "landed"):
            setattr(b, name, list(getattr(self, name)))
        return b

    @property
    def slot(self):
        return len(self.blocks) % self.L.bpm

    def tables_of(self, slot):
        td = self.L.seq[slot]
        return self.L.enc[(0, td)], self.L.enc[(1, td)]

    def add(self, z, end_with_zrl=False):
        slot = self.slot
        z = np.asarray(z, np.int16)
        assert slot not in self.L.forced_zero or not z.any()
        comp = self.L.comp[slot]
        syms, s = encode_block(z, self.pred[comp], *self.tables_of(slot), end_with_zrl=end_with_zrl)
        bi, pos = len(self.blocks), self.bits
        for nb, kind, k, n in syms:
            self.starts.append(pos)
            self.recs.append((nb, kind, bi, k, n))
            pos += nb
        assert pos - self.bits == len(s)
        self.pred[comp] = int(z[0])
        self.blocks.append(z)
        self.parts.append(s)
        self.bits = pos

    def symbols(self):
        return Symbols(self.starts, self.recs, self.bits, len(self.blocks), self.L.period)

    def stream(self):
        s = "".join(self.parts)
        s += str(self.L.pad_bit) * (-len(s) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""

    # -- filler --
    def _dc(self, comp, spread=30):
        p = self.pred[comp]
        return p + int(self.rng.integers(-spread, spread + 1)) - (40 if p > 400 else -40 if p < -400 else 0)

    def _draw(self):
        if self._pool is None or self._pool_at == len(self._pool):
            self._pool, self._pool_at = self.rng.integers(0, 1 << 30, 4096).tolist(), 0
        self._pool_at += 1
        return self._pool[self._pool_at - 1]

    def noise(self, ncoef=None, bulk=False):
        """one random block: ncoef (default: about density * 63) coefficients of up to +-amp at random positions, then an EOB;
        bulk: half of the positions, up to +-1000 (the long stretches in front of a workgroup seam: fewer symbols per KB)"""
        slot = self.slot
        z = np.zeros(64, np.int16)
        if slot in self.L.forced_zero:
            return self.add(z)
        if self.light and ncoef is None:                     # one coefficient of +-1, a DC step of at most 3
            r = self._draw()
            z[1 + r % 63] = 1 if r & 64 else -1
            p = self.pred[self.L.comp[slot]]
            z[0] = p + (r >> 8) % 7 - 3 - (2 if p > 400 else -2 if p < -400 else 0)
            return self.add(z)
        n = int(self.rng.binomial(63, self.bulk_density if bulk else self.density)) if ncoef is None else ncoef
        if n:
            at = self.rng.choice(63, n, replace=False) + 1
            mag = self.rng.integers(1, (self.bulk_amp if bulk else self.amp) + 1, n)
            z[at] = np.where(self.rng.random(n) < 0.5, mag, -mag)
        z[0] = self._dc(self.L.comp[slot])
        self.add(z)

    def noise_blocks(self, n):
        for _ in range(n):
            self.noise()

    def noise_to(self, bit):
        """random blocks while the stream is shorter than `bit` bits"""
        while self.bits < bit:
            self.noise()

    def tune_then(self, target, make_tail, hi=None):
        """random blocks, one block of an exact length, then the blocks make_tail gives, so that a point of that tail lies at
        bit `target`.  make_tail(slot, preds) -> None (this slot will not do) or (blocks, pre): the blocks to add behind the exact
        block when the next block is `slot` and the predictors are `preds`, and the bits from the exact block's end to the point."""
        guard = 0
        hi = hi or (600 if self.light else 1400)             # (light filler: the exact block is kept short as well)
        while True:
            guard += 1
            assert guard < 100000 and target - self.bits > 0, f"cannot reach bit {target} from {self.bits}"
            slot = self.slot
            if slot not in self.L.forced_zero and target - self.bits <= hi + 1200:
                comp = self.L.comp[slot]
                dc_t, ac_t = self.tables_of(slot)
                dcv = self._dc(comp)
                d = dcv - self.pred[comp]
                preds = list(self.pred)
                preds[comp] = dcv
                tail = make_tail((slot + 1) % self.L.bpm, preds)
                if tail is not None:
                    blocks, pre = tail
                    rest = target - pre - self.bits - (dc_t[_cat(d)][1] + _cat(d))
                    z = exact_ac(ac_t, rest, self.rng) if rest <= hi else None
                    if z is not None:
                        z[0] = dcv
                        self.add(z)
                        for t in blocks:
                            self.add(*t) if isinstance(t, tuple) else self.add(t)
                        return
            if target - self.bits > hi + 1200:
                self.noise(bulk=target - self.bits > 16 * SUBSEQ_BITS)
            else:
                self.noise(1 if slot not in self.L.forced_zero else 0)

    def tail_bits(self, slot, preds, blocks):
        """bits of `blocks` coded from block slot `slot` with predictors `preds` (updated), and the symbols of the last one"""
        total, syms = 0, []
        for t in blocks:
            z, zrl = (t if isinstance(t, tuple) else (t, False))
            comp = self.L.comp[slot]
            syms, s = encode_block(z, preds[comp], *self.tables_of(slot), end_with_zrl=zrl)
            preds[comp] = int(z[0])
            total += len(s)
            slot = (slot + 1) % self.L.bpm
        return total, syms

    def finish_at(self, total_bits):
        """end the stream, at the end of an MCU, after exactly total_bits bits"""
        def tail(slot, preds):
            blocks = []
            while slot != 0:
                if slot not in self.L.forced_zero:
                    return None
                blocks.append(np.zeros(64, np.int16))
                slot = (slot + 1) % self.L.bpm
            return blocks, self.tail_bits((self.slot + 1) % self.L.bpm, preds, blocks)[0]
        self.tune_then(total_bits, tail)
        assert self.bits == total_bits and self.slot == 0
        return self

    def finish(self, more_mcus=2):
        """random blocks to the end of the MCU and more_mcus further"""
        while self.slot:
            self.noise()
        self.noise_blocks(more_mcus * self.L.bpm)
        while not self.L.fits(len(self.blocks) // self.L.bpm):        # (a prime number of MCUs beyond one row's width)
            self.noise_blocks(self.L.bpm)
        return self

    # -- an aimed symbol --
    def place(self, kind, boundary, amount):
        """a symbol of `kind` (TARGET_KINDS) that ends `amount` bits behind bit `boundary` (0: exactly on it)"""
        got = {}

        def tail(slot, preds):
            pre_blocks = []
            last_only = kind.startswith("mcu_last")
            while (slot in self.L.forced_zero and not (last_only and slot == self.L.bpm - 1)) or (last_only and slot != self.L.bpm - 1):
                if slot not in self.L.forced_zero:
                    return None
                pre_blocks.append(np.zeros(64, np.int16))
                slot = (slot + 1) % self.L.bpm
            first = (self.slot + 1) % self.L.bpm
            p2 = list(preds)
            pre, _ = self.tail_bits(first, p2, pre_blocks)
            t = target_block(self.L, kind, slot, p2[self.L.comp[slot]], self.rng)
            if t is None:
                return None
            z, want = t
            _, syms = self.tail_bits(slot, list(p2), [z])
            off = 0
            for nb, sk, k, n in syms:
                if (sk, n) == want:
                    break
                off += nb
            else:
                raise AssertionError((kind, want))
            if amount >= nb:
                return None
            got.update(nbits=nb, symbol=sk)
            return pre_blocks + [z], pre + off + (nb - amount)
        self.tune_then(boundary, tail)
        land = check_landing(self.symbols(), kind, boundary, amount, got["nbits"], got["symbol"], self.L.bpm)
        self.landed.append(land)
        return land


TARGET_KINDS = ("ac", "dc", "eob", "zrl", "k63", "mcu_last_eob", "mcu_last_k63")


@lru_cache(maxsize=None)
def _long_ac(layout_name, td):
    """(run, size) of the longest AC symbol of a table (the smallest run among them)"""
    ac_t = LAYOUTS[layout_name].enc[(1, td)]
    return max(((sym >> 4, sym & 15) for sym in ac_t if sym & 15), key=lambda rs: (ac_t[(rs[0] << 4) | rs[1]][1] + rs[1], -rs[0]))


@lru_cache(maxsize=None)
def _long_dc(layout_name, td):
    dc_t = LAYOUTS[layout_name].enc[(0, td)]
    return max((c for c in dc_t if c <= 15), key=lambda c: (dc_t[c][1] + c, c))


def _mag(rng, s):
    m = int(rng.integers(1 << (s - 1), 1 << s))
    return m if rng.random() < 0.5 else -m


def target_block(L, kind, slot, pred, rng):
    """(block, (symbol kind, coded position)) whose named symbol is the aimed one; None if the slot cannot hold one"""
    z = np.zeros(64, np.int16)
    if slot in L.forced_zero:                        # gray's zero chroma block: its EOB is the last symbol of the MCU
        return (z, ("EOB", -1)) if kind == "mcu_last_eob" else None
    td = L.seq[slot]
    run, size = _long_ac(L.name, td)
    z[0] = pred + int(rng.integers(-20, 21))
    small = lambda: _mag(rng, int(rng.integers(1, 5)))
    if kind == "ac":
        z[1], z[2] = small(), small()
        z[3 + run] = _mag(rng, size)
        z[6 + run] = small()
        return z, ("AC", 3 + run)
    if kind == "dc":
        c = _long_dc(L.name, td)
        m = int(rng.integers(1 << (c - 1), 1 << c))
        z[0] = pred - m if pred >= 0 else pred + m
        z[1], z[5] = small(), small()
        return z, ("DC", 0)
    if kind in ("eob", "mcu_last_eob"):
        z[1], z[2], z[3] = small(), small(), small()
        return z, ("EOB", -1)
    if kind == "zrl":
        z[1] = small()
        z[20] = small()
        return z, ("ZRL", -1)
    if kind in ("k63", "mcu_last_k63"):
        z[1] = small()
        z[62 - run] = small()
        z[63] = _mag(rng, size)
        return z, ("AC", 63)
    raise AssertionError(kind)


def check_landing(sym, kind, boundary, amount, nbits, symbol, bpm=0):
    """the aimed symbol starts nbits - amount bits in front of the boundary: the assertion every placement passes"""
    start = boundary + amount - nbits
    nb, sk, block, k, n = sym.at(start)
    assert (nb, sk) == (nbits, symbol) and 0 <= amount < nb, (kind, boundary, amount, nb, sk)
    if kind == "dc":
        assert k == 0
    if kind in ("k63", "mcu_last_k63"):
        assert n == 63
    if kind.startswith("mcu_last"):
        assert bpm and block % bpm == bpm - 1
    p, b, k2, done = sym.state_at(boundary)
    if amount == 0:
        assert p == 0
    else:
        assert p == amount and sym.covering(boundary) == sym.covering(start) and start < boundary
    return dict(kind=kind, boundary=boundary, amount=amount, nbits=nb, symbol=sk, block=block, k=k, state=(p, b, k2), blocks_before=done)


def symbol_starts(coeffs, layout, zrl_blocks=()):
    """the symbol table of a whole frame (coeffs [nblocks, 64] in scan order), built afresh: what the builders' claims are checked with"""
    b = Builder(layout)
    for i, z in enumerate(np.asarray(coeffs).reshape(-1, 64)):
        b.add(z, end_with_zrl=i in zrl_blocks)
    return b.symbols()


# ---- a model of the speculation walk (jpezy_huffdec.hip, spec_kernel): how many lanes arrive in a wrong state ----
def speculation_misses(stream, layout, sym, overflow=None, lanes=None):
    """Lane i starts `overflow` subsequences in front of its own from the guess (0, 0, 0) and walks up to its own subsequence as a
    synchronisation walk does (bits that are no code: one bit on, block abandoned; a run past position 63 ends the block).  Returns
    a bool per lane: the state it arrives in is not the true one.  This is how the filler of the builders was chosen and what
    FlatCase's claim rests on (tests/test_huffdec_seams_model.py runs it); it knows nothing of the kernels' launches."""
    overflow = OVERFLOW_DEFAULT if overflow is None else overflow
    dec = {k: {(ln, code): s for s, (code, ln) in t.items()} for k, t in layout.enc.items()}
    bits = "".join(format(x, "08b") for x in stream)
    n_sub = -(-len(bits) // SUBSEQ_BITS)
    bits += "0" * (40 * SUBSEQ_BITS)

    def step(pos, b, k):
        tab = dec[(0 if k == 0 else 1, layout.seq[b])]
        for ln in range(1, 17):
            s = tab.get((ln, int(bits[pos:pos + ln], 2)))
            if s is None:
                continue
            if k == 0 and s > 16:
                break
            run, size = (0, s) if k == 0 else (63, 0) if s == 0 else (s >> 4, s & 15)
            if k + run + 1 > 63:
                return pos + ln + size, (b + 1) % layout.period, 0
            return pos + ln + size, b, k + run + 1
        return pos + 1, (b + 1) % layout.period, 0
    wrong = []
    for i in (range(n_sub) if lanes is None else lanes):
        pos, b, k = max(0, i - overflow) * SUBSEQ_BITS, 0, 0
        while pos < i * SUBSEQ_BITS:
            pos, b, k = step(pos, b, k)
        wrong.append((pos - i * SUBSEQ_BITS, b, k) != sym.state_at(i * SUBSEQ_BITS)[:3])
    return np.array(wrong)


# ---- cases ----
class Case:
    """a constructed file: name, layout, coeffs [nmcu, bpm, 64] (the ground truth), W, H, the model's unstuffed stream, where it
    landed (a list of dicts), and which path must decode it: host_rule None (the GPU decoder) or the decoder's own rule that sends
    it to the host decoder"""

    def __init__(self, name, builder, host_rule=None):
        L = builder.L
        assert builder.slot == 0, "a frame ends at the end of an MCU"
        self.name, self.layout, self.host_rule = name, L, host_rule
        self.coeffs = np.stack(builder.blocks).reshape(-1, L.bpm, 64)
        self.nmcu = self.coeffs.shape[0]
        cols, rows = L.grid(self.nmcu)
        self.W, self.H = cols * L.mcu_w, rows * L.mcu_h
        self.stream = builder.stream()
        self.total_bits = builder.bits
        self.landed = list(builder.landed)
        self.n_sub = -(-len(self.stream) * 8 // SUBSEQ_BITS)

    def __repr__(self):
        return self.name

    def write(self, J):
        """the file: jpezy's host writer for its own layouts, synth_jpeg for the others"""
        L = self.layout
        if L.writer == "own":
            return J.write_jpeg(self.coeffs, self.W, self.H, False)
        if L.writer == "own_gray":
            assert not self.coeffs[:, 4:].any()
            return J.write_jpeg(np.ascontiguousarray(self.coeffs[:, :4]), self.W, self.H, True)
        return synth_jpeg(self.W, self.H, L.comps, coeffs=self.coeffs, tables=L.tables)[0]

    def symbols(self):
        return symbol_starts(self.coeffs, self.layout)


def kind_amounts(layout):
    """[(kind, amount)]: every kind of aimed symbol with every amount by which it can straddle a boundary in this layout"""
    L = LAYOUTS[layout]
    rng = np.random.default_rng(0)
    b = Builder(L)
    out = []
    for kind in TARGET_KINDS:
        longest = 0
        for slot in range(L.bpm):
            if kind.startswith("mcu_last") and slot != L.bpm - 1:
                continue
            t = target_block(L, kind, slot, 0, rng)
            if t is None:
                continue
            z, want = t
            _, syms = b.tail_bits(slot, [0] * len(L.comps), [z])
            longest = max([longest] + [nb for nb, sk, k, n in syms if (sk, n) == want])
        out += [(kind, a) for a in range(longest)]
    return out


BOUNDARY_KINDS = ("interior", "quarter", "emit_wg", "sync_wg")


def boundaries(bkind):
    """the bit positions of one kind of boundary, far enough apart for a placement each, in ascending order (endless)"""
    j = 0
    while True:
        j += 1
        if bkind == "interior":
            if (3 * j) % EMIT_SUBS:
                yield 3 * j * SUBSEQ_BITS
        elif bkind == "quarter":
            yield 3 * j * SUBSEQ_BITS + (1 + j % (EMIT_PARTS - 1)) * PART_BITS
        elif bkind == "emit_wg":
            if (j * EMIT_SUBS) % WGS:
                yield j * EMIT_SUBS * SUBSEQ_BITS
        elif bkind == "sync_wg":
            yield j * WGS * SUBSEQ_BITS


def straddle_case(layout, bkind, placements, seed=1):
    """one file with every (kind, amount) of `placements` on a boundary of kind bkind of its own"""
    L = LAYOUTS[layout]
    b = Builder(L, seed=seed)
    for (kind, amount), boundary in zip(placements, boundaries(bkind)):
        b.place(kind, boundary, amount)
    b.finish()
    return Case(f"{bkind}-{layout}-{len(placements)}", b)


# ---- A. stuffing bytes on chunk and workgroup seams (offsets in the STUFFED scan) ----
def _pattern_block(pred, rng):
    """a luma block (Annex K) whose code holds a 0xFF byte, 0xFF 0x00 as data and 0xFF 0xFF, each at some bit offset: +1023 is
    1111111110000011 1111111111, -1 is 00 0"""
    z = np.zeros(64, np.int16)
    z[0] = pred + int(rng.integers(-5, 6))
    z[1] = 1023
    z[2:7] = -1
    z[7] = z[8] = z[9] = 1023
    z[10] = int(rng.integers(1, 30))
    return z


PATTERNS = {"ff": "1" * 8, "ff00": "1" * 8 + "0" * 8, "ffff": "1" * 16}


def place_bytes(b, pattern, Q):
    """the bytes of `pattern` (data bytes: FF / FF 00 / FF FF) with the first 0xFF at offset Q of the stuffed scan"""
    want = PATTERNS[pattern]
    # the stuffing in front of the pattern depends on the random blocks in front of it: settle all but the last few hundred bytes,
    # then try (with fresh random blocks each time) until the offset is met
    b.noise_to(8 * (Q - Q // 8 - 500))
    u = Q - removed_before(b.stream(), Q) - min(30, Q // 16)
    for attempt in range(400):
        t = b.clone()
        t.rng = np.random.default_rng([Q, attempt])

        def tail(slot, preds):
            if slot in t.L.forced_zero or t.L.seq[slot] != 0:
                return None
            z = _pattern_block(preds[t.L.comp[slot]], t.rng)
            s = encode_block(z, preds[t.L.comp[slot]], *t.tables_of(slot))[1]
            for o in range(len(s) - len(want)):
                if s[o:o + len(want)] == want:
                    return [z], o
            return None
        t.tune_then(8 * u, tail)
        t.noise()
        stream = t.stream()
        q = stuffed_offset(stream, u)
        if q == Q:
            n = len(want) // 8
            assert stream[u:u + n] == bytes(int(want[8 * i:8 * i + 8], 2) for i in range(n)), (pattern, Q)
            st = stuffed(stream)
            assert st[Q] == 0xFF and st[Q + 1] == 0x00
            t.landed.append(dict(kind=pattern, stuffed_offset=Q, unstuffed_offset=u, stuffed=st[Q:Q + 4].hex()))
            b.__dict__.update(t.__dict__)
            return
        u += Q - q
    raise AssertionError(f"no {pattern} at stuffed offset {Q}")


def stuffing_seam_case(layout, seam, seed=3):
    """FF | 00, FF 00 | 00 (the second zero is data) and FF 00 FF 00 in its three positions across seams `seam` bytes apart"""
    b = Builder(LAYOUTS[layout], seed=seed)
    step = max(1, 6 * CHUNK // seam)
    plan = [("ff", -1), ("ff00", -2), ("ffff", -3), ("ffff", -2), ("ffff", -1)]
    for i, (pattern, d) in enumerate(plan):
        place_bytes(b, pattern, (1 + i) * step * seam + d)
    b.finish()
    st = stuffed(b.stream())
    for (pattern, d), land in zip(plan, b.landed):
        Q = land["stuffed_offset"]
        assert (Q - d) % seam == 0
        want = {"ff": "ff00", "ff00": "ff0000", "ffff": "ff00ff00"}[pattern]
        assert st[Q:Q + len(want) // 2].hex() == want
    return Case(f"stuffing-{layout}-seam{seam}", b)


def chunk_counts(stream):
    """stuffing bytes per 64-byte chunk of the stuffed scan"""
    st = np.frombuffer(stuffed(stream), np.uint8)
    ff = M.ff_positions(stream)
    at = ff + np.arange(len(ff)) + 1
    return np.bincount(at // CHUNK, minlength=-(-len(st) // CHUNK))


def dense_case(seed=4):
    """The most stuffing a chunk can hold.  A chunk that is all FF 00 pairs cannot be coded: every code word has a zero bit and a
    symbol has at most 31 bits, so no more than 30 one bits follow one another (three 0xFF bytes); with Annex K it is 19 (two).
    Six luma blocks of +1023 everywhere -- 21-bit runs of ones every 26 bits -- are the densest Annex-K stream; the stuffing it
    sheds also leaves the launch (sized before unstuffing) with subsequences that hold no data."""
    b = Builder(LAYOUTS["one"], seed=seed)
    b.noise_blocks(30)
    for i in range(6):
        z = np.full(64, 1023, np.int16)
        z[0] = b.pred[0] + (i * 37) % 11 - 5
        z[1 + i] = -1023 + i                                  # (no two of the six alike)
        b.add(z)
    b.noise_blocks(30)
    c = Case("stuffing-dense", b)
    counts = chunk_counts(c.stream)
    n_sub_max = -(-len(stuffed(c.stream)) * 8 // SUBSEQ_BITS)
    assert counts.max() >= 20 and n_sub_max - c.n_sub >= 2, (counts.max(), n_sub_max, c.n_sub)
    c.landed = [dict(kind="dense", most_stuffing_in_a_chunk=int(counts.max()), n_sub_max=n_sub_max, n_sub=c.n_sub)]
    return c


def densest_case(seed=4):
    """the same with dense_tables(): 30 one bits and a zero, over and over -- 27 to 28 of a chunk's 64 bytes are stuffing, the most
    any baseline stream can reach (an all-FF 00 chunk would be 32)"""
    b = Builder(LAYOUTS["dense_one"], seed=seed)
    b.noise_blocks(30)
    for i in range(6):
        z = np.full(64, 32767, np.int16)
        z[0] = b.pred[0] + (i * 37) % 11 - 5
        b.add(z)
    b.noise_blocks(30)
    c = Case("stuffing-densest", b)
    counts = chunk_counts(c.stream)
    assert counts.max() >= 27, counts.max()
    c.landed = [dict(kind="dense", most_stuffing_in_a_chunk=int(counts.max()))]
    return c


def shift_cases(seed=5):
    """four files whose stuffing bytes in front of the first workgroup seam of the copy kernel number 0, 1, 2, 3 (mod 4)"""
    base = Builder(LAYOUTS["own420"], seed=seed)
    base.noise_to(8 * (COPY_WG_BYTES - 3000))
    found = {}
    for j in range(64):
        t = base.clone()
        for _ in range(j):
            while t.L.seq[t.slot] != 0:
                t.noise()
            t.add(_pattern_block(t.pred[0], t.rng))
        t.noise_to(8 * (COPY_WG_BYTES + 600))
        t.finish()
        stream = t.stream()
        assert len(stuffed(stream)) > COPY_WG_BYTES + 64
        r = removed_before(stream, COPY_WG_BYTES)
        if r % 4 not in found:
            t.landed.append(dict(kind="shift", removed_before_seam=r, shift=r % 4))
            found[r % 4] = Case(f"stuffing-shift{r % 4}", t)
        if len(found) == 4:
            break
    assert sorted(found) == [0, 1, 2, 3]
    return [found[r] for r in range(4)]


def stuffed_length_case(layout, length, seed=6):
    """a scan of exactly `length` stuffed bytes: the EOI's 0xFF is byte `length` of the scan (the last byte of a chunk when
    length % 64 == 63, of a copy workgroup when length == 16,383)"""
    base = Builder(LAYOUTS[layout], seed=seed)
    base.noise_to(8 * (length - length // 8 - 500))
    u = length - removed_before(base.stream(), length) - (30 if length > 600 else 0)
    for attempt in range(400):
        t = base.clone()
        t.rng = np.random.default_rng([length, attempt])
        t.finish_at(8 * u - 3)
        got = len(stuffed(t.stream()))
        if got == length:
            t.landed.append(dict(kind="stuffed_length", length=length, unstuffed=u))
            return Case(f"length{length}-{layout}", t)
        u += length - got
    raise AssertionError(length)


def last_byte_ff_case(layout, seed=7):
    """the scan's last data byte is 0xFF (FF 00 FF D9): coefficient 63 of the last block, value bits all one, ends on a byte end"""
    b = Builder(LAYOUTS[layout], seed=seed)
    b.noise_blocks(3 * b.L.bpm)
    b.place("mcu_last_k63", 8 * (b.bits // 8 + 400), 0)
    blocks = [x.copy() for x in b.blocks]
    blocks[-1][63] = (1 << _cat(blocks[-1][63])) - 1         # the largest value of its category: same length, value bits all one
    r = Builder(b.L)
    for x in blocks:
        r.add(x)
    assert r.bits == b.bits and r.bits % 8 == 0 and r.slot == 0
    stream = r.stream()
    assert stream[-1] == 0xFF and stuffed(stream)[-2:] == b"\xff\x00"
    r.landed.append(dict(kind="last_byte_ff", bits=r.bits))
    return Case(f"lastff-{layout}", r)


def nsub_case(layout, n, over, seed=8):
    """an unstuffed stream of exactly 128 n bytes (n subsequences), or one byte more (over: n + 1 subsequences)"""
    b = Builder(LAYOUTS[layout], seed=seed + n)
    bytes_ = SUBSEQ_BITS // 8 * n + (1 if over else 0)
    b.finish_at(8 * bytes_ - (5 if n % 2 else 0))            # (with and without pad bits)
    c = Case(f"nsub{n + (1 if over else 0)}-{'over' if over else 'full'}-{layout}", b)
    assert len(c.stream) == bytes_ and c.n_sub == n + (1 if over else 0)
    c.landed = [dict(kind="n_sub", n_sub=c.n_sub, unstuffed_bytes=bytes_)]
    return c


NSUB_BASES = (1, 2, 3, 4, 63, 64, 255, 256, 259)             # n and n + 1: 1 2 3 4 5 63 64 65 255 256 257 259 260


# ---- B. further cases ----
def exact_block(b, nbits, dc_cat=None):
    """a block of exactly nbits coded bits for the builder's next slot (every AC position non-zero)"""
    slot = b.slot
    comp = b.L.comp[slot]
    dc_t, ac_t = b.tables_of(slot)
    if dc_cat is None:
        dcv = b._dc(comp)
    else:
        m = int(b.rng.integers(1 << (dc_cat - 1), 1 << dc_cat))
        dcv = b.pred[comp] - m if b.pred[comp] >= 0 else b.pred[comp] + m
    c = _cat(dcv - b.pred[comp])
    z = exact_ac(ac_t, nbits - dc_t[c][1] - c, b.rng)
    assert z is not None, nbits
    z[0] = dcv
    return z


def block_at(b, bit, nbits, dc_cat=None, then=()):
    """a block of nbits bits that starts at bit `bit` (and blocks of `then` bits right behind it)"""
    def tail(slot, preds):
        if slot in b.L.forced_zero or b.L.seq[slot] != 0:
            return None
        t = b.clone()
        t.pred = list(preds)
        t.blocks = t.blocks + [None]
        blocks = []
        for n in (nbits,) + tuple(then):
            if t.slot in t.L.forced_zero or t.L.seq[t.slot] != 0:
                return None
            z = exact_block(t, n, dc_cat)
            blocks.append(z)
            t.pred[t.L.comp[t.slot]] = int(z[0])
            t.blocks = t.blocks + [None]
        return blocks, 0
    b.tune_then(bit, tail)


def lanes_inside_one_block(sym, n_sub):
    """subsequences that complete no block and whose marks all lie inside one block"""
    out = []
    for i in range(n_sub):
        a, e = sym.state_at(i * SUBSEQ_BITS), sym.state_at((i + 1) * SUBSEQ_BITS)
        inside = a[3] == e[3] and (a[2] != 0 or a[0] > 0) and (e[2] != 0 or e[0] > 0)
        if inside and (i + 1) * SUBSEQ_BITS <= sym.total_bits:
            out.append(i)
    return out


def long_blocks_case(layout, sizes, seed=9):
    """blocks longer than a subsequence: one, two in a row, and one that starts in the last quarter of lane 255 of the first
    synchronisation workgroup"""
    b = Builder(LAYOUTS[layout], seed=seed)
    one, two, late = sizes
    dc_cat = 15 if b.L.tables is not None else None
    block_at(b, 6 * SUBSEQ_BITS - 150, one, dc_cat)             # (1,174 bits and more: lane 6 lies inside it)
    block_at(b, 11 * SUBSEQ_BITS + 700, two[0], dc_cat, then=(two[1],))
    start = (WGS - 1) * SUBSEQ_BITS + 3 * PART_BITS + 40
    block_at(b, start, late, dc_cat)
    b.finish()
    c = Case(f"long-blocks-{layout}", b)
    sym = c.symbols()
    lanes = lanes_inside_one_block(sym, c.n_sub)
    assert WGS in lanes and len(lanes) >= 3, lanes
    nb, kind, block, k, n = sym.at(start)
    assert kind == "DC" and sym.state_at(start + late)[0] == 0
    c.landed = [dict(kind="long_blocks", sizes=sizes, lanes_without_a_block_end=lanes)]
    return c


def short_blocks_case(layout, seed=10):
    """a stretch of minimum-length blocks (DC difference 0, EOB) between noisy stretches: more than 170 blocks in a subsequence"""
    b = Builder(LAYOUTS[layout], seed=seed)
    b.noise_to(4 * SUBSEQ_BITS + 300)
    b.finish(0)
    for _ in range(300 // b.L.bpm * b.L.bpm):
        z = np.zeros(64, np.int16)
        z[0] = 0 if b.slot in b.L.forced_zero else b.pred[b.L.comp[b.slot]]
        b.add(z)
    b.noise_to(b.bits + 4 * SUBSEQ_BITS)
    b.finish()
    c = Case(f"short-blocks-{layout}", b)
    sym = c.symbols()
    per = [sym.state_at((i + 1) * SUBSEQ_BITS)[3] - sym.state_at(i * SUBSEQ_BITS)[3] for i in range(c.n_sub - 1)]
    assert max(per) >= 170, per
    c.landed = [dict(kind="short_blocks", most_blocks_in_a_subsequence=max(per))]
    return c


def scan_end_case(layout, total_bits, seed=11):
    """the last block ends after exactly total_bits bits"""
    b = Builder(LAYOUTS[layout], seed=seed + total_bits % 97)
    b.finish_at(total_bits)
    c = Case(f"end{total_bits}-{layout}", b)
    c.landed = [dict(kind="scan_end", bits=total_bits, pad_bits=-total_bits % 8, lane=(total_bits - 1) // SUBSEQ_BITS)]
    return c


SCAN_ENDS = ([6 * SUBSEQ_BITS, 6 * SUBSEQ_BITS + PART_BITS, 6 * SUBSEQ_BITS + 2 * PART_BITS, 6 * SUBSEQ_BITS + 3 * PART_BITS]
             + [8 * 900 - r for r in range(1, 8)]
             + [WGS * SUBSEQ_BITS - 100, WGS * SUBSEQ_BITS, WGS * SUBSEQ_BITS + 100])


def zrl_case(reach, seed=12):
    """a block whose closing zero run is coded as a ZRL in place of the EOB (no encoder writes it): reach 64 -- the run ends exactly
    at position 63 (k + 16 == 64), a valid block for both decoders; reach 65 -- one position further, refused by both"""
    b = Builder(LAYOUTS["s444"], seed=seed)
    b.noise_blocks(40 * 3)
    z = np.zeros(64, np.int16)
    z[0] = b.pred[0] + 3
    z[5] = -7
    z[reach - 17] = 9                                       # the decoder's index behind it: reach - 16
    b.add(z, end_with_zrl=True)
    zi = len(b.blocks) - 1
    nb, kind, block, k, n = b.recs[-1]
    assert kind == "ZRL" and k + 16 == reach
    b.finish(30)
    c = Case(f"zrl-reach{reach}", b)
    c.zrl_blocks = (zi,)
    c.landed = [dict(kind="zrl_end", k=k, reach=reach)]
    return c


def raw_file(case):
    """the case's model stream behind the header synth_jpeg writes for its layout (for streams no encoder writes)"""
    L = case.layout
    blank = synth_jpeg(case.W, case.H, L.comps, coeffs=np.zeros_like(case.coeffs), tables=L.tables)[0]
    return blank[:len(blank) - 2 - len(entropy_segment(blank))] + stuffed(case.stream) + b"\xff\xd9"


# ---- D. DC pass ----
DC_PASS_MCUS = (511, 512, 513, 1024, 1025, 2047, 2048, 2049, 4096, 4097)


def dc_pass_file(nmcu, seed=13):
    """(file, coefficients [nmcu, 6, 64]) of a 4:2:0 frame with random non-zero DC differences, every value inside int16.  The luma
    component (4 blocks per MCU) has 4 nmcu DC terms, each chroma component (1 per MCU) nmcu: nmcu in DC_PASS_MCUS puts the chroma
    counts on 2,047 / 2,048 / 2,049 / 4,096 / 4,097 and the luma counts -- multiples of 4 -- on 2,044 / 2,048 / 2,052 / 4,096 / 4,100
    (and 8,188 ... 16,388): both sides of one and two DC_PER_WG workgroups."""
    rng = np.random.default_rng(seed + nmcu)
    L = LAYOUTS["own420"]
    dd = rng.integers(1, 41, (nmcu, 6)) * rng.choice([-1, 1], (nmcu, 6))
    run = [0, 0, 0]
    for m in range(nmcu):
        for i in range(6):
            c = L.comp[i]
            if abs(run[c] + dd[m, i]) > 30000:
                dd[m, i] = -dd[m, i]
            run[c] += int(dd[m, i])
    assert (dd != 0).all()
    cols, rows = L.grid(nmcu)
    data, co, _ = synth_jpeg(cols * 16, rows * 16, YUV420, seed=seed + nmcu, density=0.06, dc_diffs=dd)
    co = co.reshape(nmcu, 6, 64)
    assert co.dtype == np.int16 and np.abs(co[..., 0].astype(np.int64)).max() <= 32767
    return data, co


# ---- E. restart intervals ----
class RestartCase:
    """a file of restart intervals: one Builder per interval (predictors at zero), R MCUs each (the last may have fewer)"""

    def __init__(self, name, layout, builders, landed=()):
        L = LAYOUTS[layout]
        self.name, self.layout, self.host_rule = name, L, None
        counts = [len(b.blocks) // L.bpm for b in builders]
        self.R = counts[0]
        assert all(b.slot == 0 for b in builders) and all(c == self.R for c in counts[:-1]) and 0 < counts[-1] <= self.R, counts
        self.coeffs = np.stack([z for b in builders for z in b.blocks]).reshape(-1, L.bpm, 64)
        self.nmcu = self.coeffs.shape[0]
        cols, rows = L.grid(self.nmcu)
        self.W, self.H = cols * L.mcu_w, rows * L.mcu_h
        self.streams = [b.stream() for b in builders]
        self.landed = list(landed) + [l for b in builders for l in b.landed]

    def __repr__(self):
        return self.name

    def segment(self):
        out = b""
        for i, s in enumerate(self.streams):
            out += (bytes([0xFF, 0xD0 + (i - 1) % 8]) if i else b"") + stuffed(s)
        return out

    def write(self, J=None):
        return synth_jpeg(self.W, self.H, self.layout.comps, coeffs=self.coeffs, tables=self.layout.tables, restart=self.R)[0]

    def bytes_per_interval(self):
        """what the decoder divides to choose the lane-per-stream kernel: the bytes from the first scan byte to the end of the file,
        by the number of intervals"""
        return (len(self.segment()) + 2) // len(self.streams)


PER_LANE_LIMIT = GEOMETRY["PER_LANE_LIMIT"]              # bytes per interval up to which a lane walks a whole interval
TINY_LENGTHS = (1, 3, 4, 5, 63, 64, 65)


def _one_block_interval(nbits, seed, last_ff=False):
    for s in range(seed, seed + 200):
        b = Builder(LAYOUTS["one"], seed=s)
        if nbits <= 8:
            z = np.zeros(64, np.int16)
        elif nbits <= 120:
            z = M.tuner_block(nbits, 0)
            if z is None:
                nbits -= 1
                continue
        else:
            z = exact_block(b, nbits)
            if last_ff:
                if _cat(z[63]) < 8:
                    continue
                z[63] = (1 << _cat(z[63])) - 1
        b.add(z)
        if last_ff or 0xFF not in b.stream():
            return b
    raise AssertionError(nbits)


def tiny_intervals_case(seed=14):
    """intervals of one block whose stuffed length is 1, 3, 4, 5, 63, 64, 65 bytes (three of each, other contents), and one whose
    last data byte is 0xFF in front of its RSTn: the lane-per-stream kernel's zero words behind a stream's end"""
    builders, landed = [], []
    for rep in range(3):
        for n in TINY_LENGTHS:
            b = _one_block_interval(8 * n - (rep if n > 1 else 2), seed + 1000 * rep + n)
            assert len(stuffed(b.stream())) == n, (n, len(b.stream()))
            builders.append(b)
            landed.append(dict(kind="interval_bytes", interval=len(builders) - 1, stuffed_bytes=n))
        b = _one_block_interval(8 * (40 + rep), seed + 77 + rep, last_ff=True)
        assert b.stream()[-1] == 0xFF and b.bits % 8 == 0
        builders.append(b)
        landed.append(dict(kind="interval_last_byte_ff", interval=len(builders) - 1))
    b = Builder(LAYOUTS["one"], seed=seed)
    b.noise()
    builders.append(b)                                       # (the last interval ends at the EOI, not at an RSTn)
    c = RestartCase("restart-tiny", "one", builders, landed)
    seg = c.segment()
    assert b"\xff\x00\xff\xd0" in seg or b"\xff\x00\xff\xd1" in seg or any(bytes([0xFF, 0, 0xFF, 0xD0 + q]) in seg for q in range(8))
    assert c.bytes_per_interval() <= PER_LANE_LIMIT
    return c


def per_lane_limit_cases(seed=15):
    """two files of four intervals of random blocks, the bytes per interval just under and just over the lane-per-stream limit"""
    n_int = 4

    def case(R, name):
        builders = []
        for i in range(n_int):
            b = Builder(LAYOUTS["one"], seed=seed + i)
            b.noise_blocks(R)
            builders.append(b)
        return RestartCase(name, "one", builders)
    R = 100
    while case(R, "probe").bytes_per_interval() <= PER_LANE_LIMIT - 400:
        R += 8
    while case(R, "probe").bytes_per_interval() <= PER_LANE_LIMIT:
        R += 1
    out = [case(R - 1, "restart-limit-under"), case(R, "restart-limit-over")]
    for c in out:
        c.landed = [dict(kind="per_lane_limit", bytes_per_interval=c.bytes_per_interval(), per_lane=c.bytes_per_interval() <= PER_LANE_LIMIT)]
    assert len(out) == 2 and out[0].bytes_per_interval() <= PER_LANE_LIMIT < out[1].bytes_per_interval()
    return out


def fill_exact(b, total_bits, nblocks):
    """exactly nblocks random blocks of exactly total_bits bits (layouts of one block per MCU): the density of each block is steered
    by what is left, the last block has the exact length"""
    assert b.L.bpm == 1
    for left in range(nblocks, 1, -1):
        want = (total_bits - 900 - b.bits) / (left - 1)
        b.noise(int(min(60, max(1, round((want - 12) / 15)))))
    z = exact_block(b, total_bits - b.bits)
    b.add(z)
    assert b.bits == total_bits and len(b.blocks) == nblocks
    return b


def workgroup_intervals_case(seed=16):
    """an interval of exactly 256 subsequences, one of 257 and a short last one: the batch form, whose workgroups never straddle
    two streams"""
    R = 820
    sizes = [WGS * SUBSEQ_BITS - 3, WGS * SUBSEQ_BITS + 5]
    builders = [fill_exact(Builder(LAYOUTS["one"], seed=seed + i), t, R) for i, t in enumerate(sizes)]
    last = Builder(LAYOUTS["one"], seed=seed + 9)
    last.noise_blocks(200)
    builders.append(last)
    c = RestartCase("restart-256-257", "one", builders)
    subs = [-(-len(s) * 8 // SUBSEQ_BITS) for s in c.streams]
    assert subs[:2] == [WGS, WGS + 1] and c.bytes_per_interval() > PER_LANE_LIMIT
    c.landed = [dict(kind="interval_subsequences", subsequences=subs)]
    return c


SEAM_PATTERNS = (("ff", -1), ("ff00", -2), ("ffff", -3), ("ffff", -2), ("ffff", -1))       # FF | 00, FF 00 | 00, FF 00 FF 00 in three positions


def interval_seam_case(per_lane, which, seed=17):
    """one of the section-A chunk-seam stuffing patterns (SEAM_PATTERNS[which]) across the seam behind a stream's first chunk and
    across the seam in front of its last chunk, in the first and in the last interval; per_lane: short intervals (lane-per-stream
    kernel), else long ones (batch form)"""
    pattern, d = SEAM_PATTERNS[which]
    builders = []
    for i, nbytes in enumerate(((3000, 1200) if per_lane else (14000, 4000))):
        b = Builder(LAYOUTS["one"], seed=seed + 10 * which + i)
        place_bytes(b, pattern, CHUNK + d)
        b.noise_to(8 * nbytes)
        m0 = len(stuffed(b.stream())) // CHUNK + 10
        for m in range(m0, m0 + 24):                         # (what follows the pattern must end inside the next chunk)
            t = b.clone()
            place_bytes(t, pattern, m * CHUNK + d)
            n = len(stuffed(t.stream()))
            if m * CHUNK + 2 < n <= (m + 1) * CHUNK:
                break
        assert m * CHUNK + 2 < n <= (m + 1) * CHUNK, (m, n)
        b = t
        b.landed[-1]["last_chunk"] = m
        st = stuffed(b.stream())
        want = {"ff": "ff00", "ff00": "ff0000", "ffff": "ff00ff00"}[pattern]
        for Q in (CHUNK + d, m * CHUNK + d):
            assert st[Q:Q + len(want) // 2].hex() == want, (pattern, Q)
        builders.append(b)
    # the first interval sets R: it has the most blocks
    assert len(builders[0].blocks) >= len(builders[1].blocks)
    c = RestartCase(f"restart-seams-{'lane' if per_lane else 'batch'}-{pattern}{-d}", "one", builders)
    assert (c.bytes_per_interval() <= PER_LANE_LIMIT) == per_lane, c.bytes_per_interval()
    return c


# ---- the exception table: what the decoder itself hands to the host decoder ----
RULE_LOW_LONG_CODE = "a code of more than 10 bits below the hi table's region (build_dev_table returns false)"
RULE_DC_CATEGORY_16 = "a DC category 16 (decode_step<EMIT> returns false: no int16 holds the difference)"
RULE_PERIODIC = "a periodic stream (ScanState::periodic / scan_hopeless: it never falls into step)"
# The fourth rule, more than 48 blocks per MCU, has no case: one or three components of at most 4 x 4 blocks are 48 at the most,
# and the header parser takes no other component count.


def low_code_tables():
    """Annex K's DC tables and an AC table whose EOB has 2 bits and every other symbol 11 bits: the 11-bit codes start at
    01000000000, far below the six leading ones the device's second table covers"""
    ak = _annex_k()
    ac = table_of([(0x00, 2)] + [(sym, 11) for sym in [0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]])
    return {(0, 0): ak[(0, 0)], (0, 1): ak[(0, 1)], (1, 0): ac, (1, 1): ac}


LAYOUTS["lowcode"] = Layout("lowcode", [(1, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)], tables=low_code_tables())


def low_code_case(seed=18, mcus=60):
    b = Builder(LAYOUTS["lowcode"], seed=seed)
    b.noise_blocks(3 * mcus)
    b.landed.append(dict(kind="low_long_code", first_11_bit_code=_strings(b.L.enc[(1, 0)])[0xF0]))
    return Case(f"exception-lowcode-{seed}", b, host_rule=RULE_LOW_LONG_CODE)


def dc16_case(seed=19):
    """wide_tables(): a DC difference of 40,000 between two values inside int16"""
    b = Builder(LAYOUTS["wide444"], seed=seed)
    b.noise_blocks(3 * 40)
    for v in (-20000, 20000):
        z = np.zeros(64, np.int16)
        z[0], z[3] = v, 5
        b.add(z)
        b.noise_blocks(2)
    sym = b.symbols()
    assert any(kind == "DC" and nb == 32 for nb, kind, _, _, _ in sym.recs)
    b.noise_blocks(3 * 40)
    b.landed.append(dict(kind="dc_category_16", difference=40000))
    return Case("exception-dc16", b, host_rule=RULE_DC_CATEGORY_16)


class FlatCase:
    """A flat colour frame of jpezy's own layout: every DC difference but the first zero, no AC -- 32 bits per MCU for ever.  The first
    MCU (luma DC 5: 36 bits) shifts the period by 4 bits against the subsequences: a decoder started on the guess stays in a wrong
    parse that leaves every subsequence as it entered it (speculation_misses(): nearly every lane), the lanes agree with one another,
    and the true state would creep down the 254 subsequences one lane per step.  (With a shift of a multiple of 8 bits the guess
    IS the true parse and the frame decodes on the GPU at once.)"""
    name, layout, host_rule, landed, stream = "exception-periodic", LAYOUTS["own420"], RULE_PERIODIC, [dict(kind="flat", first_mcu_bits=36)], None

    def __init__(self, W=2032, H=1024):
        self.W, self.H = W, H
        self.nmcu = (W // 16) * (H // 16)
        self.coeffs = np.zeros((self.nmcu, 6, 64), np.int16)
        self.coeffs[:, :4, 0] = 5
        bits = M.block_lengths(self.coeffs[:2])
        assert int(bits[:6].sum()) == 36 and int(bits[6:].sum()) == 32

    def __repr__(self):
        return self.name

    def write(self, J):
        return J.write_jpeg(self.coeffs, self.W, self.H, False)


# ---- the registry: every constructed file by name ----
STRADDLE_LAYOUTS = ANNEX_LAYOUTS + ["wide444", "long_one"]


def straddle_for(bkind, layout):
    """interior boundaries and quarter marks: every (kind, amount) of the layout in one file.  The workgroup seams are 8 KB and 32 KB
    of stream apart: there the pairs are dealt out among the five Annex-K layouts (each pair at each seam in one of them), and the
    31-bit symbol's amounts between the two wide-table layouts."""
    wg = bkind in ("emit_wg", "sync_wg")
    if layout in ANNEX_LAYOUTS:
        placements = _dealt(bkind)[layout] if wg else kind_amounts(layout)
    else:
        placements = [("ac", a) for a in range(31)][STRADDLE_LAYOUTS.index(layout) - 5::2] if wg else kind_amounts(layout)
    return straddle_case(layout, bkind, placements, seed=1 + BOUNDARY_KINDS.index(bkind))


@lru_cache(maxsize=None)
def seam_pairs():
    """what lands on each kind of workgroup seam (8 KB and 32 KB of stream apart): the 26-bit AC symbol at every amount 0..25, every
    amount of the short kinds (EOB, ZRL, the EOB that ends an MCU), and every fourth amount of the DC symbol, of coefficient 63
    and of the coefficient 63 that ends an MCU"""
    have = set().union(*(kind_amounts(lay) for lay in ANNEX_LAYOUTS))
    pairs = []
    for kind in TARGET_KINDS:
        amounts = sorted(a for k, a in have if k == kind)
        amounts = [a for a in amounts if kind in ("ac", "eob", "zrl", "mcu_last_eob") or a % 4 == 0]
        pairs += [(kind, a) for a in amounts[len(amounts) // 2:] + amounts[:len(amounts) // 2]]      # (a middle amount first)
    return pairs


@lru_cache(maxsize=None)
def _dealt(bkind):
    """{layout: [(kind, amount)]}: every pair of seam_pairs() in one layout that has it.  Coefficient-pass seams: in turn.
    Synchronisation seams: of every kind the first pair goes to own420, the second to s444, the third to own_gray (the layouts with a
    table period, where b wraps at the end of an MCU), the others in turn to the two layouts of period 1 -- the short filler blocks
    of the first three make 32 KB of stream thousands of blocks."""
    have = {lay: kind_amounts(lay) for lay in ANNEX_LAYOUTS}
    out = {lay: [] for lay in ANNEX_LAYOUTS}
    periodic, flat = ["own420", "s444", "own_gray"], ["shared", "one"]
    taken = {}
    for j, pair in enumerate(seam_pairs()):
        if bkind == "sync_wg":
            got = taken.setdefault(pair[0], [])
            order = [lay for lay in periodic if lay not in got] + [flat[(j + t) % 2] for t in range(2)] + periodic
        else:
            order = [ANNEX_LAYOUTS[(j + t) % 5] for t in range(5)]
        lay = next(lay for lay in order if pair in have[lay])
        out[lay].append(pair)
        if bkind == "sync_wg":
            got.append(lay)
    return out


def _registry():
    R = {}
    for bk in BOUNDARY_KINDS:
        for lay in STRADDLE_LAYOUTS:
            R[f"{bk}-{lay}"] = ("B", straddle_for, (bk, lay))
    for lay in ("own420", "one"):
        R[f"stuffing-seam{CHUNK}-{lay}"] = ("A", stuffing_seam_case, (lay, CHUNK))
    R[f"stuffing-seam{COPY_WG_BYTES}-own420"] = ("A", stuffing_seam_case, ("own420", COPY_WG_BYTES))
    R["stuffing-dense"] = ("A", dense_case, ())
    R["stuffing-densest"] = ("A", densest_case, ())
    for r in range(4):
        R[f"stuffing-shift{r}"] = ("A", lambda r=r: shift_cases()[r], ())
    for n in (CHUNK - 1, CHUNK, CHUNK + 1, COPY_WG_BYTES - 1, COPY_WG_BYTES, COPY_WG_BYTES + 1):
        R[f"length{n}-own420"] = ("A", stuffed_length_case, ("own420", n))
    for n in (CHUNK - 1, COPY_WG_BYTES - 1):
        R[f"length{n}-one"] = ("A", stuffed_length_case, ("one", n))
    for lay in ("own420", "one"):
        R[f"lastff-{lay}"] = ("A", last_byte_ff_case, (lay,))
    for i, n in enumerate(NSUB_BASES):
        for over in (False, True):
            R[f"nsub{n + over}-{'over' if over else 'full'}"] = ("A", nsub_case, (("own420", "one", "s444")[i % 3], n, over))
    R["long-blocks-one"] = ("B", long_blocks_case, ("one", (1300, (1025, 1600), 1600)))
    R["long-blocks-own420"] = ("B", long_blocks_case, ("own420", (1600, (1200, 1450), 1500)))
    R["long-blocks-long_one"] = ("B", long_blocks_case, ("long_one", (1984, (1900, 1984), 1984)))
    for lay in ("own420", "own_gray"):
        R[f"short-blocks-{lay}"] = ("B", short_blocks_case, (lay,))
    for t in SCAN_ENDS:
        R[f"end{t}-own420"] = ("B", scan_end_case, ("own420", t))
    for t in SCAN_ENDS[4:11]:
        R[f"end{t}-one"] = ("B", scan_end_case, ("one", t))
    R["zrl-reach64"] = ("B", zrl_case, (64,))
    R["exception-lowcode"] = ("X", low_code_case, ())
    R["exception-dc16"] = ("X", dc16_case, ())
    R["exception-periodic"] = ("X", FlatCase, ())
    R["restart-tiny"] = ("E", tiny_intervals_case, ())
    R["restart-limit-under"] = ("E", lambda: per_lane_limit_cases()[0], ())
    R["restart-limit-over"] = ("E", lambda: per_lane_limit_cases()[1], ())
    R["restart-256-257"] = ("E", workgroup_intervals_case, ())
    for w, (pattern, d) in enumerate(SEAM_PATTERNS):
        R[f"restart-seams-lane-{pattern}{-d}"] = ("E", interval_seam_case, (True, w))
        R[f"restart-seams-batch-{pattern}{-d}"] = ("E", interval_seam_case, (False, w))
    return R


shift_cases = lru_cache(maxsize=None)(shift_cases)
per_lane_limit_cases = lru_cache(maxsize=None)(per_lane_limit_cases)
REGISTRY = _registry()
EXCEPTIONS = {"exception-lowcode": RULE_LOW_LONG_CODE, "exception-dc16": RULE_DC_CATEGORY_16, "exception-periodic": RULE_PERIODIC}


def names(section):
    return [n for n, (sec, _, _) in REGISTRY.items() if sec == section]


@lru_cache(maxsize=None)
def case(name):
    _, f, args = REGISTRY[name]
    c = f(*args)
    assert (c.host_rule is not None) == (name in EXCEPTIONS)
    return c


_FILES = {}


def file_of(J, name):
    """the bytes of a registered case (written once per process)"""
    if name not in _FILES:
        c = case(name)
        _FILES[name] = raw_file(c) if getattr(c, "zrl_blocks", None) else c.write(J)
    return _FILES[name]
