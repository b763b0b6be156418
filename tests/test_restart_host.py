"""Restart intervals in the host writer (jpezy_write_jpeg_rst): the model of tests/restart_model.py first proved equal to it, then the
file format over a grid of intervals and shapes -- DRI in front of SOS, RSTn in order, predictors reset, every reader agrees --
and the cases that sit on the rule's edges: pads of 0..7 bits, 0xFF in front of a marker, the size bound, the comment's room."""
import ctypes as C
import io
from functools import lru_cache

import numpy as np
import pytest

import entropy_model as M
import huffopt_model as HM
import restart_model as R
from jpeg_synth import synth_jpeg
from test_jpeg_bound import worst_field

BADARG, FORMAT = -1, -5
SHAPES = [(16, 16), (48, 32), (17, 33), (272, 48)]       # 272 x 48: 17 MCUs per row -- with Ri = 1 the marker index wraps past D7 twice


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _grid(W, H):
    return (W + 15) // 16, (H + 15) // 16


def _intervals(W, H):
    cols, rows = _grid(W, H)
    nmcu = cols * rows
    return sorted({ri for ri in (1, 2, 3, 7, 8, 9, cols, nmcu - 1, nmcu, nmcu + 1, 65535) if ri >= 1})


@lru_cache(maxsize=None)
def _field(W, H, gray):
    """small values with zero runs, wandering DCs, a block without EOB and one with ZRL codes here and there"""
    cols, rows = _grid(W, H)
    rng = np.random.default_rng(W * 1000 + H + gray)
    co = rng.integers(-5, 6, (rows * cols, 6, 64)).astype(np.int16)
    co[..., 6:] *= (rng.random((rows * cols, 6, 58)) < 0.25)
    co[..., 0] = rng.integers(-700, 700, (rows * cols, 6))
    flat = co.reshape(-1, 64)
    flat[::5, 63] = 900
    flat[2::7, 1:] = 0
    flat[2::7, 45] = -77
    co = np.ascontiguousarray(co[:, :4]) if gray else co
    co.setflags(write=False)
    return co


@lru_cache(maxsize=None)
def _plain(J, W, H, gray, optimize):
    return J.write_jpeg(_field(W, H, gray), W, H, gray, optimize=optimize)


def _pixels(jpg):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(jpg)).convert("RGB"))


def _rst(J, co, W, H, gray, ri, optimize, comment=b"", cap=None):
    """jpezy_write_jpeg_rst through ctypes: (status or size, bytes)"""
    lib = J.load_library()
    co = np.ascontiguousarray(co, dtype=np.int16)
    cap = lib.jpezy_jpeg_bound(W, H) if cap is None else cap
    buf = np.zeros(cap, np.uint8)
    n = lib.jpezy_write_jpeg_rst(co.ctypes.data_as(C.c_void_p), W, H, int(gray), comment, ri, int(optimize), buf.ctypes.data_as(C.c_void_p), cap)
    return n, (buf[:n].tobytes() if n > 0 else b"")


# ---- the model against the host writer, before it is used for anything ----
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("seed", range(4))
def test_model_equals_host_writer(J, seed, gray):
    from test_entropy_model import _random_field
    rng = np.random.default_rng(300 + seed)
    co = _random_field(rng, 6, 4 if gray else 6)
    for ri in (1, 2, 4, 5):
        jpg = J.write_jpeg(co, 48, 32, gray=gray, comment=b"", restart_interval=ri)
        hdr, seg = R.split(jpg)
        assert seg == R.scan(co, ri, gray), (seed, gray, ri)
        assert R.dri_of(jpg) == (len(hdr) - 14 - 6, ri)
        tabs = R.frame_tables(co, ri, gray)
        opt = J.write_jpeg(co, 48, 32, gray=gray, comment=b"", optimize=True, restart_interval=ri)
        assert R.split(opt)[1] == R.scan(co, ri, gray, tables=tabs), (seed, gray, ri)
        assert R.split(opt)[0] == HM.header_with_tables(hdr, tabs)


# ---- the grid ----
@pytest.mark.parametrize("optimize", [0, 1])
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("W,H", SHAPES)
def test_grid(J, oracle, W, H, gray, optimize):
    co = _field(W, H, gray)
    cols, rows = _grid(W, H)
    nmcu = cols * rows
    plain = _plain(J, W, H, gray, bool(optimize))
    want_px = _pixels(plain)
    for ri in _intervals(W, H):
        jpg = J.write_jpeg(co, W, H, gray, optimize=bool(optimize), restart_interval=ri)
        tag = (W, H, gray, optimize, ri)
        hdr, seg = R.split(jpg)
        # the scan equals the model byte for byte (with the frame's own tables: built from the counts with predictors reset)
        tabs = R.frame_tables(co, ri, gray) if optimize else None
        assert seg == R.scan(co, ri, gray, tables=tabs), tag
        # DRI directly in front of SOS; the markers: exactly ceil(nmcu / Ri) - 1 of them, D0..D7, D0...
        assert R.dri_of(jpg) == (len(hdr) - 14 - 6, ri), tag
        got = R.markers(seg)
        assert got == R.expected_markers(nmcu, ri) and len(got) == -(-nmcu // ri) - 1, tag
        # both readers return the coefficients and the interval
        for reader in (J.read_jpeg, oracle.read_jpeg):
            info, back = reader(jpg)
            assert info.restart_interval == ri, tag
            back = back.reshape(nmcu, -1, 64)
            assert np.array_equal(back[:, :co.shape[1]], co) and not back[:, co.shape[1]:].any(), tag
        # an independent decoder sees the picture of the file without restarts
        assert np.array_equal(_pixels(jpg), want_px), tag
        if ri >= nmcu:        # the DRI segment and no marker: apart from those six bytes it is the file without restarts
            at = len(hdr) - 14 - 6
            assert jpg[:at] + jpg[at + 6:] == plain, tag
            assert got == []


def test_interval_zero_is_the_plain_writer(J):
    for W, H in SHAPES:
        for gray in (False, True):
            co = _field(W, H, gray)
            for optimize in (0, 1):
                n, jpg = _rst(J, co, W, H, gray, 0, optimize, comment=b"Encoded by jpezy")
                assert jpg == J.write_jpeg(co, W, H, gray, comment=b"Encoded by jpezy", optimize=bool(optimize))
                assert R.dri_of(jpg) == (None, 0)


# ---- the edges of the rule ----
def test_every_pad_length(J):
    """interval bit lengths congruent to 0..7 (mod 8), each built with tuner_block: the pad is 0..7 bits of JPEZY_PAD_BIT"""
    seen = set()
    mcus = []
    for bits in range(40, 120):
        if bits % 8 in seen:
            continue
        mcu = R.mcu_of_bits(bits)
        if mcu is not None:
            seen.add(bits % 8)
            mcus.append((bits, mcu))
    assert seen == set(range(8))
    co = np.stack([m for _, m in mcus] + [R.flat_mcu()])
    W, H = 16 * co.shape[0], 16
    assert R.interval_bits(co, 1)[:-1] == [b for b, _ in mcus]
    jpg = J.write_jpeg(co, W, H, comment=b"", restart_interval=1)
    seg = R.split(jpg)[1]
    assert seg == R.scan(co, 1)
    # every interval stands alone: its bytes are the model's padded bytes, and the pad bits are JPEZY_PAD_BIT
    parts = R.unstuffed_intervals(co, 1)
    for (bits, _), p in zip(mcus, parts):
        assert len(p) == (bits + 7) // 8
        pad = -bits % 8
        assert p[-1] & ((1 << pad) - 1) == ((1 << pad) - 1 if R.PAD_BIT else 0)


def test_synth_writer_agrees_where_the_pad_conventions_coincide(J):
    """tests/jpeg_synth.py pads with ones; intervals built to end on a byte have no pad bits, so both writers give one segment"""
    aligned = [R.mcu_of_bits(b) for b in (40, 48, 56, 64, 72)]
    aligned = [m for m in aligned if m is not None]
    assert len(aligned) >= 3
    for ri in (1, 2):
        n = len(aligned) // ri * ri
        co = np.stack(aligned[:n] + [R.flat_mcu()] * ri)          # (the last interval: 32 bits per flat MCU)
        assert all(b % 8 == 0 for b in R.interval_bits(co, ri))
        W, H = 16 * co.shape[0], 16
        jpg = J.write_jpeg(co, W, H, comment=b"", restart_interval=ri)
        other, _, _ = synth_jpeg(W, H, [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)], coeffs=co, restart=ri)
        assert R.split(jpg)[1] == R.split(other)[1]


def test_ff_as_the_last_byte_before_a_marker(J):
    """data whose last full byte before a marker is 0xFF: FF 00 FF Dn -- the data byte is stuffed, the marker is not"""
    co = None
    # the last block of the interval: all AC +1023 ends in ten one bits; walk the front of the MCU until the interval ends on a byte
    for bits in range(6, 80):
        z = M.tuner_block(bits, 0)
        if z is None:
            continue
        mcu = R.flat_mcu()
        mcu[0] = z
        mcu[5] = M.dense_block()
        cand = np.stack([mcu, R.flat_mcu()])
        if R.interval_bits(cand, 1)[0] % 8 == 0:
            co = cand
            break
    assert co is not None and R.unstuffed_intervals(co, 1)[0][-1] == 0xFF
    jpg = J.write_jpeg(co, 32, 16, comment=b"", restart_interval=1)
    seg = R.split(jpg)[1]
    assert seg == R.scan(co, 1)
    assert b"\xff\x00\xff\xd0" in seg
    info, back = J.read_jpeg(jpg)
    assert np.array_equal(back.reshape(co.shape), co)


def test_dense_field(J, oracle):
    co = np.stack([np.stack([M.dense_block(dc) for dc in (5, -5, 7, 0, 3, -3)])] * 6)
    for ri in (1, 2, 4):
        jpg = J.write_jpeg(co, 48, 32, comment=b"", restart_interval=ri)
        assert R.split(jpg)[1] == R.scan(co, ri)
        assert R.markers(R.split(jpg)[1]) == R.expected_markers(6, ri)
        info, back = oracle.read_jpeg(jpg)
        assert np.array_equal(back.reshape(co.shape), co) and info.restart_interval == ri


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("W,H", [(16, 16), (17, 17), (64, 48)])
def test_bound_holds_at_one_mcu_per_interval(J, W, H, gray):
    """the worst-case MCU content of tests/test_jpeg_bound.py at Ri = 1 with the longest comment a restart file may carry: an interval
    adds at most a pad byte (two if stuffed) and a marker, 4 bytes per MCU, inside the spare bytes jpezy_jpeg_bound leaves per MCU"""
    lib = J.load_library()
    co = worst_field(W, H, gray)
    comment = bytes(0x41 + i % 26 for i in range(R.MAX_COMMENT_RESTART))
    plain = J.write_jpeg(co, W, H, gray=gray, comment=comment)
    for optimize in (False, True):
        jpg = J.write_jpeg(co, W, H, gray=gray, comment=comment, optimize=optimize, restart_interval=1)
        assert len(jpg) <= lib.jpezy_jpeg_bound(W, H), (W, H, gray, optimize, len(jpg))
    jpg = J.write_jpeg(co, W, H, gray=gray, comment=comment, restart_interval=1)
    nmcu = co.shape[0]
    # (with predictors reset the DC differences are no longer all of category 11, so the intervals themselves may be shorter)
    assert len(jpg) <= len(plain) + 6 + 4 * (nmcu - 1)
    # the analytic form: header + every MCU's worst bits, all stuffed, + 4 bytes per interval + pad and EOI
    worst = 1024 + nmcu * (2 * ((6 * 1661 + 7) // 8) + 4) + 4
    assert worst <= lib.jpezy_jpeg_bound(W, H)
    assert R.MAX_COMMENT_RESTART == R.MAX_COMMENT - 6 == 390


def test_comment_room(J):
    co = _field(48, 32, False)
    c390, c391, c396 = (bytes(0x61 + i % 26 for i in range(n)) for n in (390, 391, 396))
    lib = J.load_library()
    n, jpg = _rst(J, co, 48, 32, False, 3, 0, comment=c390)
    assert n > 0 and len(R.split(jpg)[0]) == 1024                  # the header fills its 1024 bytes exactly
    for optimize in (0, 1):
        n, _ = _rst(J, co, 48, 32, False, 3, optimize, comment=c391)
        assert n == BADARG
        assert b"JPEZY_MAX_COMMENT_RESTART" in lib.jpezy_hip_last_error()
        n, jpg = _rst(J, co, 48, 32, False, 0, optimize, comment=c396)
        assert n > 0 and jpg == J.write_jpeg(co, 48, 32, comment=c396, optimize=bool(optimize))
    n, _ = _rst(J, co, 48, 32, False, 0, 0, comment=c396 + b"x")
    assert n == BADARG


@pytest.mark.parametrize("ri", [-1, 65536, -65536, 1 << 20])
def test_interval_out_of_range(J, ri):
    n, _ = _rst(J, _field(48, 32, False), 48, 32, False, ri, 0)
    assert n == BADARG
    with pytest.raises(J.JpezyError, match="status -1"):
        J.write_jpeg(_field(48, 32, False), 48, 32, restart_interval=ri)


def test_value_outside_the_tables_is_still_format_error(J):
    co = _field(48, 32, False).copy()
    co[4, 2, 9] = 1024
    for optimize in (0, 1):
        n, _ = _rst(J, co, 48, 32, False, 2, optimize)
        assert n == FORMAT
    # a DC difference that is in range only because the predictor was reset is not an error; inside an interval it still is
    co = np.zeros((6, 6, 64), np.int16)
    co[:, :4, 0] = np.array([1500, 1500, -1500, -1500, 1500, 1500])[:, None]
    n, jpg = _rst(J, co, 48, 32, False, 2, 0)
    assert n > 0 and R.split(jpg)[1] == R.scan(co, 2)
    for ri in (0, 4, 6):
        n, _ = _rst(J, co, 48, 32, False, ri, 0)
        assert n == FORMAT, ri


def test_too_small_a_buffer(J):
    co = _field(48, 32, False)
    n, jpg = _rst(J, co, 48, 32, False, 1, 0)
    assert n == len(jpg) > 0
    for cap in (n - 1, n - 3, 700):
        m, _ = _rst(J, co, 48, 32, False, 1, 0, cap=cap)
        assert m == -6
    m, again = _rst(J, co, 48, 32, False, 1, 0, cap=n)
    assert m == n and again == jpg
