"""Oriented output (include/jpezy_hip_orientation.h), as far as it can be checked without a GPU: the EXIF parser over well-formed and
malformed segments, the geometry helpers against tests/orient_model.py, what the header says and the library exports, and every refusal
the new entries make before they look at the context -- made with bare ctypes and a null context, in the order the header documents.
tests/test_gpu_orient.py holds the parity tests."""
import ctypes as C
import inspect
import io
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import orient_model as OM
from jpeg_synth import synth_jpeg

ROOT = Path(__file__).resolve().parent.parent
E_BADARG, E_UNSUPPORTED = -1, -4
NEAREST, SMOOTH = 0, 1
OWN = [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]
JPG = synth_jpeg(33, 17, OWN, seed=5)[0]


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _err(lib):
    return lib.jpezy_hip_last_error().decode()


def raw_orientation(lib, data, n=None):
    """the C entry on exactly n bytes that end where their allocation ends"""
    data = bytes(data)
    n = len(data) if n is None else n
    buf = (C.c_uint8 * max(n, 1)).from_buffer_copy(data[:n] + (b"" if n else b"\0"))
    return lib.jpezy_jpeg_orientation(buf, n)


# ---- the parser -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["II", "MM"])
@pytest.mark.parametrize("place", ["alone", "first", "last"])
def test_the_tag_is_returned(J, order, place):
    for o in OM.ORIENTATIONS:
        assert J.jpeg_orientation(OM.tagged(JPG, OM.app1(value=o, order=order, place=place))) == o
        assert J.jpeg_orientation(OM.tagged(JPG, OM.app1(value=o, order=order, place=place, typ=4))) == o        # LONG, count 1


def test_pillows_exif_is_read(J):
    Image = pytest.importorskip("PIL.Image")
    for o in OM.ORIENTATIONS:
        exif = Image.Exif()
        exif[0x0112] = o
        exif[0x010F] = "a maker"                                     # a second entry, with its value outside the directory
        buf = io.BytesIO()
        Image.fromarray(np.zeros((9, 12, 3), np.uint8)).save(buf, "JPEG", exif=exif)
        assert b"Exif\0\0MM" in buf.getvalue()                         # Pillow writes big-endian
        assert J.jpeg_orientation(buf.getvalue()) == o


def test_the_first_exif_segment_decides_and_others_are_passed_over(J):
    xmp = OM.app1(payload=b"<x:xmpmeta/>", ident=b"http://ns.adobe.com/xap/1.0/\0")
    app0 = b"\xff\xe0\x00\x04\x00\x00"
    assert J.jpeg_orientation(OM.tagged(JPG, app0 + xmp + OM.app1(value=6) + OM.app1(value=3))) == 6
    assert J.jpeg_orientation(OM.tagged(JPG, OM.app1(value=9) + OM.app1(value=3))) == 1       # the first one decides, wrong as it is
    assert J.jpeg_orientation(OM.tagged(JPG, b"\xff\xff\xff" + OM.app1(value=8)[1:])) == 8    # fill bytes in front of the marker
    assert J.jpeg_orientation(JPG + OM.app1(value=6)) == 1                                    # behind SOS: not looked at


BAD = {
    "value 0": OM.app1(value=0),
    "value 9": OM.app1(value=9),
    "value 0xFFFF": OM.app1(value=0xFFFF),
    "value 0x10006 as LONG": OM.app1(value=0x10006, typ=4),
    "XMP, not Exif": OM.app1(payload=b"<x:xmpmeta/>", ident=b"http://ns.adobe.com/xap/1.0/\0"),
    "wrong TIFF magic": OM.app1(magic=43),
    "wrong byte order mark": OM.app1(payload=b"IM" + OM.tiff()[2:]),
    "IFD offset past the segment": OM.app1(ifd=4000),
    "IFD offset inside the header": OM.app1(ifd=4),
    "IFD offset at the last byte": OM.app1(ifd=len(OM.tiff()) - 1),
    "entry count past the segment": OM.app1(n_entries=3),
    "entry count 0xFFFF": OM.app1(n_entries=0xFFFF),
    "type ASCII": OM.app1(typ=2),
    "count 2": OM.app1(count=2),
    "count 0": OM.app1(count=0),
    "segment length 2": b"\xff\xe1\x00\x02",
    "segment length 1": b"\xff\xe1\x00\x01",
    "segment length past the file": OM.app1(length=0xFFF0),
    "identifier cut": OM.app1(payload=b"", ident=b"Exif\0"),
    "no TIFF header": OM.app1(payload=b""),
    "another tag": OM.app1(tag=0x0113),
}


@pytest.mark.parametrize("name", sorted(BAD))
def test_anything_wrong_gives_1(J, name):
    assert raw_orientation(J.load_library(), OM.tagged(JPG, BAD[name])) == 1


def test_no_app1_null_and_empty(J):
    lib = J.load_library()
    assert J.jpeg_orientation(JPG) == 1
    assert lib.jpezy_jpeg_orientation(None, 0) == 1
    assert lib.jpezy_jpeg_orientation(None, 100) == 1
    assert raw_orientation(lib, JPG, 0) == 1
    assert J.jpeg_orientation(b"") == 1
    assert J.jpeg_orientation(b"\xff\xd8") == 1
    assert J.jpeg_orientation(b"\x00\xd8" + OM.app1(value=6)) == 1      # no SOI


@pytest.mark.parametrize("order", ["II", "MM"])
def test_a_file_cut_at_every_byte_of_the_app1(J, order):
    lib = J.load_library()
    seg = OM.app1(value=6, order=order, place="last")
    full = OM.tagged(JPG, seg)
    for n in range(2, 2 + len(seg)):                                  # the cut lies inside the segment: it is not complete
        assert raw_orientation(lib, full, n) == 1, n
    assert raw_orientation(lib, full, 2 + len(seg)) == 6               # complete, the rest of the file missing


def test_parser_under_asan_ubsan_on_every_mutation_and_truncation(tmp_path):
    """tests/fuzz/exif_fuzz.cpp: jpezy_exif.h as a stand-alone CPU program under AddressSanitizer + UBSan over the cases above, and over
    every truncation and every single-byte mutation of two valid segments (II and MM)"""
    import shutil
    import struct
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    cases = [(OM.tagged(JPG, OM.app1(value=o, order=order, place=place, typ=typ)), o) for order in ("II", "MM") for place in ("alone", "first", "last")
             for typ in (3, 4) for o in OM.ORIENTATIONS]
    cases += [(OM.tagged(JPG, seg), 1) for seg in BAD.values()] + [(JPG, 1), (b"", 1), (b"\xff\xd8", 1)]
    (tmp_path / "cases.bin").write_bytes(b"".join(struct.pack("<II", len(d), want) + d for d, want in cases))
    valid = []
    for order in ("II", "MM"):
        valid.append(tmp_path / f"valid_{order}.bin")
        valid[-1].write_bytes(b"\xff\xd8" + OM.app1(value=6, order=order, place="last") + b"\xff\xda\x00\x02")
    exe = tmp_path / "exif_fuzz"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        str(ROOT / "tests" / "fuzz" / "exif_fuzz.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    if "cannot find -lasan" in r.stderr or "libasan" in r.stderr and "No such file" in r.stderr:
        pytest.skip("no libasan for the host compiler in this image")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), *map(str, valid)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{len(cases)} recorded cases, 0 wrong" in r.stdout and r.stdout.rstrip().endswith(", 0 wrong")
    assert r.stdout.count("every truncation and every single-byte mutation") == 2


# ---- geometry --------------------------------------------------------------------------------------------------------------------------
def windows(Wo, Ho):
    out = [(0, 0, Wo, Ho), (0, 0, 1, 1), (Wo - 1, Ho - 1, 1, 1), (Wo // 2, 0, 1, Ho), (0, Ho // 2, Wo, 1)]
    if Wo > 2 and Ho > 2:
        out.append((1, 1, Wo - 2, Ho - 2))
    return out


@pytest.mark.parametrize("W,H", [(1, 1), (1, 9), (7, 5), (33, 17)])
def test_size_and_rect_are_the_models(J, W, H):
    for o in OM.ORIENTATIONS:
        assert J.orient_size(o, W, H) == OM.size(o, W, H)
        for win in windows(*OM.size(o, W, H)):
            assert J.orient_rect(o, W, H, win) == OM.rect(o, W, H, win), (o, win)


def test_size_and_rect_refusals(J):
    lib = J.load_library()
    a, b = C.c_int(7), C.c_int(7)
    rect, src = (C.c_int * 4)(0, 0, 2, 2), (C.c_int * 4)(9, 9, 9, 9)
    assert lib.jpezy_orient_size(6, 7, 5, None, C.byref(b)) == E_BADARG and _err(lib) == "orient_size: null pointer"
    for o in (0, 9, -1):
        assert lib.jpezy_orient_size(o, 7, 5, C.byref(a), C.byref(b)) == E_BADARG and _err(lib) == "orient_size: orientation must be 1..8"
    assert lib.jpezy_orient_size(6, 0, 5, C.byref(a), C.byref(b)) == E_BADARG and "must be positive" in _err(lib)
    assert (a.value, b.value) == (7, 7)
    assert lib.jpezy_orient_rect(0, 7, 5, None, src) == E_BADARG and _err(lib) == "orient_rect: null pointer"
    assert lib.jpezy_orient_rect(6, 7, 5, rect, None) == E_BADARG and _err(lib) == "orient_rect: null pointer"
    assert lib.jpezy_orient_rect(0, 0, 5, rect, src) == E_BADARG and _err(lib) == "orient_rect: orientation must be 1..8"
    assert lib.jpezy_orient_rect(6, 7, 0, (C.c_int * 4)(0, 0, 0, 0), src) == E_BADARG and "must be positive" in _err(lib)
    assert lib.jpezy_orient_rect(6, 7, 5, (C.c_int * 4)(0, 0, 0, 2), src) == E_BADARG and "needs w, h >= 1" in _err(lib)
    assert lib.jpezy_orient_rect(6, 7, 5, (C.c_int * 4)(-1, 0, 2, 2), src) == E_BADARG and "needs w, h >= 1" in _err(lib)
    # the oriented picture of a 7 x 5 one is 5 x 7 for 6 and 7 x 5 for 3
    assert lib.jpezy_orient_rect(6, 7, 5, (C.c_int * 4)(0, 0, 6, 1), src) == E_BADARG and "lies outside the oriented picture of 5 x 7" in _err(lib)
    assert lib.jpezy_orient_rect(3, 7, 5, (C.c_int * 4)(0, 0, 1, 6), src) == E_BADARG and "lies outside the oriented picture of 7 x 5" in _err(lib)
    assert list(src) == [9, 9, 9, 9]
    assert lib.jpezy_orient_rect(6, 7, 5, (C.c_int * 4)(0, 0, 5, 7), src) == 0 and list(src) == [0, 0, 7, 5]


# ---- header, exports, binding ----------------------------------------------------------------------------------------------------------
NEW = ("jpezy_jpeg_orientation", "jpezy_orient_size", "jpezy_orient_rect", "jpezy_dequant_idct_region_oriented_dev",
       "jpezy_dequant_idct_region_oriented_packed_dev", "jpezy_decode_jpeg_oriented", "jpezy_decode_jpeg_oriented_packed",
       "jpezy_ctx_set_windows_orientation", "jpezy_ctx_windows_orientation")


def test_header_declares_the_section_and_the_library_exports_it(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    section = text[text.index(" * ORIENTED OUTPUT"):]
    assert '#include "jpezy_hip_orientation.h"' in section
    part = (ROOT / "include" / "jpezy_hip_orientation.h").read_text()
    for phrase in ("PERMUTATION OF PIXELS", "NOT provided", "JPEZY_ORIENT_FROM_FILE 0", "(Ws-1-Y, Hs-1-X)", "IFD0 only"):
        assert phrase in part, phrase
    strip = lambda t: re.sub(r"/\*.*?\*/", "", t, flags=re.S)
    lib = J.load_library()
    listed = {n for n, _, _ in J.api.ABI_ORIENTATION}
    assert listed == set(NEW)
    main = {n for n, _, _ in J.api.ABI}
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", strip(part)), name
        assert not re.search(r"\b" + name + r"\s*\(", strip(text)), name        # jpezy_hip.h's own text declares a closed set
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
        assert name not in main
    assert J.ORIENT_FROM_FILE == 0


def test_python_surface(J):
    sig = lambda f: inspect.signature(f).parameters
    assert sig(J.Context.dequant_idct_region_dev)["orientation"].default is None
    assert sig(J.Context.decode_jpeg_oriented)["orientation"].default == J.ORIENT_FROM_FILE
    assert sig(J.Context.decode_jpeg_oriented_packed)["orientation"].default == J.ORIENT_FROM_FILE
    assert sig(J.Decoder.decode)["orient"].default is False
    assert callable(J.Context.set_windows_orientation) and callable(J.Context.windows_orientation)


# ---- refusals with a null context, in the documented order ----------------------------------------------------------------------------
QT = (C.c_uint16 * 256)(*([16] * 256))
HS, VS, TQ = (C.c_uint8 * 3)(2, 1, 1), (C.c_uint8 * 3)(2, 1, 1), (C.c_uint8 * 3)(0, 1, 1)
COEF = C.c_void_p(0x1000)          # never dereferenced: a null context is refused before any device work
PIX = C.c_void_p(0x2000)


def planar(lib, o, up=NEAREST, precision=8, W=64, H=48, scale=1, region=(0, 0, 8, 8), n_frames=1, stride=64 * 48, coef=COEF, dst=PIX):
    r = (C.c_int * 4)(*region) if region is not None else None
    return lib.jpezy_dequant_idct_region_oriented_dev(None, coef, QT, 3, HS, VS, TQ, precision, W, H, 0, up, scale, r, o, n_frames, stride, dst, dst, dst,
                                                      None)


def packed(lib, o, up=NEAREST, precision=8, W=64, H=48, scale=1, region=(0, 0, 8, 8), fmt=0, row=0, frame=0, n_frames=1, coef=COEF, dst=PIX):
    r = (C.c_int * 4)(*region) if region is not None else None
    return lib.jpezy_dequant_idct_region_oriented_packed_dev(None, coef, QT, 3, HS, VS, TQ, precision, W, H, 0, up, scale, r, o, fmt, row, frame,
                                                             n_frames, dst, None)


@pytest.mark.parametrize("entry,name", [(planar, "dequant_idct_region_oriented_dev"), (packed, "dequant_idct_region_oriented_packed_dev")])
def test_device_entries_with_a_null_context(J, entry, name):
    lib = J.load_library()
    for o in (0, 9, -3):                                              # the orientation first, whatever else is wrong
        assert entry(lib, o, up=7, region=None, coef=None) == E_BADARG and _err(lib) == name + ": orientation must be 1..8"
    for o in (3, 6):
        assert entry(lib, o, up=7, region=None) == E_BADARG and "upsampling must be" in _err(lib)
        assert entry(lib, o, up=SMOOTH, precision=12, region=None) == E_UNSUPPORTED and "8-bit" in _err(lib)
        assert entry(lib, o, dst=None, region=None) == E_BADARG and _err(lib) == name + ": null pointer"
        assert entry(lib, o, region=None) == E_BADARG and _err(lib) == name + ": null pointer"
        assert entry(lib, o, W=0) == E_BADARG and "1..65535" in _err(lib)
        assert entry(lib, o, n_frames=0) == E_BADARG and "n_frames" in _err(lib)
        assert entry(lib, o, scale=3) == E_BADARG and "scale_denom must be" in _err(lib)
        assert entry(lib, o, region=(0, 0, 0, 8)) == E_BADARG and "needs w, h >= 1" in _err(lib)
        assert entry(lib, o, coef=C.c_void_p(0x1002)) == E_BADARG and "16-byte aligned" in _err(lib)
        assert entry(lib, o) == E_BADARG and _err(lib) == "null context"
    # the window is held against the ORIENTED picture: 64 x 48 shown in orientation 6 is 48 x 64
    assert entry(lib, 6, region=(0, 0, 48, 64)) == E_BADARG and _err(lib) == "null context"
    assert entry(lib, 6, region=(0, 0, 64, 48)) == E_BADARG and "lies outside the picture of 48 x 64 at scale_denom 1" in _err(lib)
    assert entry(lib, 3, region=(0, 0, 64, 48)) == E_BADARG and _err(lib) == "null context"
    assert entry(lib, 8, scale=2, region=(0, 0, 24, 32)) == E_BADARG and _err(lib) == "null context"
    assert entry(lib, 8, scale=2, region=(0, 0, 25, 32)) == E_BADARG and "48 x 64" not in _err(lib) and "24 x 32 at scale_denom 2" in _err(lib)
    # orientation 1 is the existing entry's call: its name in the message
    assert entry(lib, 1, region=None) == E_BADARG and "oriented" not in _err(lib)


def test_file_entries_with_a_null_context(J):
    lib = J.load_library()
    data = np.frombuffer(OM.tagged(JPG, OM.app1(value=6)), np.uint8)
    info, used = J.FrameInfo(), C.c_int(-7)
    dst = np.zeros(4096, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rect = (C.c_int * 4)(0, 0, 4, 4)

    def planes(o, up=NEAREST, scale=1, r=rect, i=info):
        return lib.jpezy_decode_jpeg_oriented(None, p(data), data.size, 0, up, scale, r, o, C.byref(used), C.byref(i) if i is not None else None, p(dst),
                                              p(dst), p(dst), 1024)

    def pk(o, up=NEAREST, scale=1, r=rect, i=info, fmt=0, row=0):
        return lib.jpezy_decode_jpeg_oriented_packed(None, p(data), data.size, 0, up, scale, r, o, C.byref(used), C.byref(i) if i is not None else None,
                                                     fmt, C.c_size_t(row), p(dst), 4096)

    for entry, name in ((planes, "decode_jpeg_oriented"), (pk, "decode_jpeg_oriented_packed")):
        used.value = -7
        assert entry(9, up=5, scale=3, i=None) == E_BADARG and "upsampling must be" in _err(lib)
        for o in (9, -1):
            assert entry(o, scale=3, i=None) == E_BADARG and _err(lib) == name + ": orientation must be JPEZY_ORIENT_FROM_FILE or 1..8"
        assert entry(6, scale=3, i=None) == E_BADARG and _err(lib) == name + ": null pointer"
        assert entry(6, scale=3) == E_BADARG and "scale_denom must be" in _err(lib)
        assert entry(6, r=(C.c_int * 4)(0, 0, 0, 4)) == E_BADARG and "needs w, h >= 1" in _err(lib)
        assert used.value == -7                                      # not written while an argument is unsound
        for o, want in ((6, 6), (0, 6), (3, 3)):                     # 0: the file's own tag
            for r in (rect, None):
                assert entry(o, r=r) == E_BADARG and _err(lib) == "null context", (o, r)
                assert used.value == want
        assert entry(1) == E_BADARG and "null context" in _err(lib) and used.value == 1
    assert pk(6, fmt=9) == E_BADARG and "unknown pixel format" in _err(lib)
    assert pk(6, fmt=9, r=None) == E_BADARG and "unknown pixel format" in _err(lib)
    assert pk(6, row=5) == E_BADARG and "row_stride smaller" in _err(lib)


def test_windows_setting_with_a_null_context(J):
    lib = J.load_library()
    for mode in (2, -1):
        assert lib.jpezy_ctx_set_windows_orientation(None, mode) == E_BADARG and "mode must be 0" in _err(lib)
    assert lib.jpezy_ctx_set_windows_orientation(None, 1) == E_BADARG and _err(lib) == "null context"
    assert lib.jpezy_ctx_set_windows_orientation(None, 0) == E_BADARG and _err(lib) == "null context"
    assert lib.jpezy_ctx_windows_orientation(None) == E_BADARG and _err(lib) == "null context"


# ---- the command-line tools: the rules that need no GPU ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bins():
    from jpezy_amd import _build
    _build.build_all()
    return ROOT / "jpezy_amd" / "bin"


def _run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_decode_orient_is_parsed(bins, tmp_path):
    dec, src, out = bins / "jpezy_decode", tmp_path / "x.jpg", tmp_path / "y.ppm"
    p = _run(dec, src)
    assert p.returncode == 1 and "[OPT: --orient]" in p.stderr
    for form in ("--orient=6", "--orientation", "--orient=", "--oriented"):
        for opts in ([form], ["--gray", form], [form, "--scale=2"], ["--scale=2", "--region=4x4+0+0", form]):
            p = _run(dec, src, out, *opts)
            assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_decode <input.(jpg | jpeg)>"), opts
            assert "by roki" not in p.stdout and not out.exists()
    # well formed, alone and beside the other options: past the rules (the file does not exist)
    for opts in (["--orient"], ["--orient", "--gray"], ["--scale=2", "--orient"], ["--region=4x4+0+0", "--orient", "--scale=4"], ["--orient", "--upsampling=smooth"]):
        p = _run(dec, src, out, *opts)
        assert p.returncode == 1 and "Usage" not in p.stderr and not out.exists(), opts
    # the refusals of --upsampling=smooth stay word for word
    for opts in (["--orient", "--upsampling=smooth", "--scale=2"], ["--upsampling=smooth", "--region=4x4+0+0", "--orient"]):
        p = _run(dec, src, out, *opts)
        assert p.returncode == 1 and "--upsampling=smooth writes whole pictures at full size" in p.stderr and "Usage" not in p.stderr, opts


def test_cli_tran_auto_orient_is_parsed(bins, tmp_path):
    tran, src, dst = bins / "jpezy_tran", tmp_path / "x.jpg", tmp_path / "y.jpg"
    p = _run(tran)
    assert p.returncode == 1 and "| --auto-orient)" in p.stderr
    for opts in (["--auto-orient=6"], ["--auto-orient", "--rotate=90"], ["--none", "--auto-orient"], ["--auto-orient", "--auto-orient"], ["--auto"],
                 ["--autoorient"]):
        p = _run(tran, src, dst, *opts)
        assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_tran <input.(jpg | jpeg)> <output.(jpg | jpeg)>"), opts
        assert "by roki" not in p.stdout and not dst.exists()
    for opts in (["--auto-orient"], ["--auto-orient", "--trim"], ["--optimize", "--auto-orient", "--restart=4"]):
        p = _run(tran, src, dst, *opts)
        assert p.returncode == 1 and "Usage" not in p.stderr and "input_file" in p.stderr and not dst.exists(), opts
