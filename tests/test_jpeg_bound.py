"""The size contract of the writers (include/jpezy_hip.h): jpezy_jpeg_bound(W, H) holds the largest file any writer can produce
with a comment of up to JPEZY_MAX_COMMENT bytes, and every writer refuses a longer comment with JPEZY_E_BADARG.  Host side: the
analytic worst case, a measured maximal-stuffing field, and the refusal of the host writers (the GPU writers:
tests/test_gpu_entropy_seams.py)."""
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SIZES = [(1, 1), (16, 16), (17, 17), (65535, 1)]
HEADER_NO_COMMENT = 623          # SOI, APP0, 2 x DQT, 4 x DHT, SOF0, SOS
BADARG = -1


def _max_comment():
    m = re.search(r"#define\s+JPEZY_MAX_COMMENT\s+(\d+)", (ROOT / "include" / "jpezy_hip.h").read_text())
    assert m, "include/jpezy_hip.h must name the comment limit (JPEZY_MAX_COMMENT)"
    return int(m.group(1))


MAX_COMMENT = _max_comment()


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _comment(n):
    return bytes((0x41 + i % 26) for i in range(n))


def worst_field(W, H, gray):
    """the longest coding the writer accepts, with as many 0xFF bytes as it allows: every DC difference of category 11 (the
    components' DC values alternate +1023 / -1023), every AC coefficient +1023 (a 16-bit code whose first nine bits are one,
    then ten one value bits: runs of 21 one bits)"""
    from tests import entropy_model as M
    mc, mr = (W + 15) // 16, (H + 15) // 16
    bpm = 4 if gray else 6
    co = np.full((mc * mr, bpm, 64), 1023, np.int16)
    # DC per component in coded order: luma blocks 0..3 of every MCU form one chain, Cb and Cr one each
    luma = np.where(np.arange(mc * mr * 4) % 2 == 0, 1023, -1023).astype(np.int16)
    co[:, :4, 0] = luma.reshape(-1, 4)
    if not gray:
        ch = np.where(np.arange(mc * mr) % 2 == 0, 1023, -1023).astype(np.int16)
        co[:, 4, 0] = ch
        co[:, 5, 0] = ch
    assert M.category(2046) == 11
    return co


def test_header_length_and_max_comment_fit_the_bound_constant(J):
    z = np.zeros(6 * 64, np.int16)
    for n in (0, 1, 16, MAX_COMMENT):
        jpg = J.write_jpeg(z, 16, 16, comment=_comment(n))
        sos = jpg.index(b"\xff\xda")
        hdr = sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big")
        assert hdr == HEADER_NO_COMMENT + (n + 5 if n else 0), n
    # the longest header is exactly the 1024 bytes jpezy_jpeg_bound reserves for it (and the device writer's header buffer)
    assert HEADER_NO_COMMENT + MAX_COMMENT + 5 <= 1024


@pytest.mark.parametrize("W,H", SIZES)
def test_bound_analytic(J, W, H):
    """header with the longest comment + 1660 bits per block, every byte stuffed, + EOI <= jpezy_jpeg_bound"""
    from tests import entropy_model as M
    lib = J.load_library()
    nmcu = ((W + 15) // 16) * ((H + 15) // 16)
    stream = (nmcu * 6 * M.WORST_BLOCK_BITS + 7) // 8
    worst = HEADER_NO_COMMENT + MAX_COMMENT + 5 + 2 * stream + 2
    assert worst <= lib.jpezy_jpeg_bound(W, H), (W, H, worst, lib.jpezy_jpeg_bound(W, H))


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("W,H", SIZES)
def test_bound_holds_for_worst_field_with_max_comment(J, oracle, W, H, gray):
    from tests import entropy_model as M
    lib = J.load_library()
    co = worst_field(W, H, gray)
    jpg = J.write_jpeg(co, W, H, gray=gray, comment=_comment(MAX_COMMENT))
    assert len(jpg) <= lib.jpezy_jpeg_bound(W, H), (W, H, gray, len(jpg))
    assert jpg == oracle.write_jpeg(co, W, H, gray=gray, comment=_comment(MAX_COMMENT))
    # the field really is the heavy one: every luma block codes 9 + 11 + 63 x 26 bits after the first, and a 0xFF byte is
    # stuffed at least once per 26 bits of dense AC code
    nmcu = co.shape[0]
    lens = M.block_lengths(co, gray)
    assert lens[6:].max() == 1658 if nmcu > 1 else lens.max() >= 1656
    scan = M.scan_of(jpg)
    assert len(M.ff_positions(scan)) >= nmcu * 4 * 63 * 26 // 8 // 4, (W, H, gray)


def test_com_length_field(J):
    z = np.zeros(6 * 64, np.int16)
    jpg = J.write_jpeg(z, 16, 16, comment=_comment(MAX_COMMENT))
    k = jpg.index(b"\xff\xfe")
    assert int.from_bytes(jpg[k + 2:k + 4], "big") == MAX_COMMENT + 3
    assert jpg[k + 4:k + 4 + MAX_COMMENT + 1] == _comment(MAX_COMMENT) + b"\x00"


@pytest.mark.parametrize("n", [MAX_COMMENT + 1, 1024, 65532, 65533, 65535, 70000])
def test_host_writers_refuse_longer_comment(J, n):
    import ctypes as C
    lib = J.load_library()
    z = np.zeros(6 * 64, np.int16)
    cap = 1 << 17
    buf = np.zeros(cap, np.uint8)
    rc = lib.jpezy_write_jpeg(z.ctypes.data_as(C.c_void_p), 16, 16, 0, _comment(n), buf.ctypes.data_as(C.c_void_p), cap)
    assert rc == BADARG, (n, rc)
    assert b"JPEZY_MAX_COMMENT" in lib.jpezy_hip_last_error()
    sizes = (C.c_long * 2)()
    z2 = np.zeros(2 * 6 * 64, np.int16)
    rc = lib.jpezy_write_jpeg_batch(z2.ctypes.data_as(C.c_void_p), 16, 16, 0, 2, _comment(n), buf.ctypes.data_as(C.c_void_p),
                                    cap // 2, sizes, 2)
    assert rc == BADARG, (n, rc)
    with pytest.raises(J.JpezyError, match="status -1"):
        J.write_jpeg(z, 16, 16, comment=_comment(n))


def test_host_writers_accept_up_to_the_limit(J, oracle):
    rng = np.random.default_rng(5)
    co = rng.integers(-60, 61, (2, 6, 64)).astype(np.int16)
    for n in (0, 1, MAX_COMMENT - 1, MAX_COMMENT):
        c = _comment(n)
        one = J.write_jpeg(co, 32, 16, comment=c)
        assert one == oracle.write_jpeg(co, 32, 16, comment=c), n
        batch = J.write_jpeg_batch(np.stack([co, co]), 32, 16, 2, comment=c, threads=2)
        assert batch == [one, one], n
