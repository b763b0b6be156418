"""Lossless transforms (include/jpezy_hip.h, LOSSLESS TRANSFORMS), the argument checks of the four entries: all of them come before the
context is looked at, so they are made here with a null context and exactly one bad argument at a time, which the message must name; with
none bad the call gets as far as the context and says so.  tests/test_gpu_transform.py holds the parity tests."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
E_BADARG = -1


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _err(lib):
    return lib.jpezy_hip_last_error().decode()


def test_every_entry_refuses_bad_arguments_before_the_context(J):
    lib = J.load_library()
    raw = np.zeros(1 << 16, np.uint8)
    base = (raw.ctypes.data + 15) & ~15                                   # 16-byte aligned; never dereferenced: the context is null
    W, H = 48, 32                                                         # 3 x 2 MCUs at 4:2:0: 2304 elements, 4608 bytes per frame
    frame = 2 * J.coeff_count(W, H)
    a, b = C.c_void_p(base), C.c_void_p(base + 3 * frame)
    info = J.FrameInfo()
    tab = (C.c_uint8 * 64)(*([1] * 64))
    ints = [C.c_int() for _ in range(4)]

    def geom(op=5, flags=0, wh=(W, H), sampling=0):
        return lib.jpezy_transform_geometry(op, flags, wh[0], wh[1], sampling, *(C.byref(x) for x in ints))

    def tables(op=5, src=tab, dst=tab):
        return lib.jpezy_quant_tables_transform(op, src, dst)

    def dev(op=5, flags=0, wh=(W, H), sampling=0, nf=1, d_in=a, d_out=b):
        return lib.jpezy_coeff_transform_dev(None, d_in, wh[0], wh[1], sampling, op, flags, nf, d_out, None)

    def file(op=5, flags=0, data=a, n=64, comment=None, inf=info, out=b, cap=1024):
        return lib.jpezy_transform_jpeg(None, data, n, op, flags, comment, C.byref(inf) if inf is not None else None, out, cap)

    assert geom() == 0 and tables() == 0                                  # the pure host functions need no context
    cases = [
        (lambda: dev(), "context"), (lambda: file(), "context"), (lambda: file(out=None, cap=0), "context"),
        (lambda: dev(flags=1), "context"), (lambda: file(flags=1, comment=b"x" * 396), "context"),
        (lambda: geom(op=8), "op"), (lambda: geom(op=-1), "op"), (lambda: tables(op=8), "op"), (lambda: tables(op=-1), "op"),
        (lambda: dev(op=8), "op"), (lambda: dev(op=-1), "op"), (lambda: file(op=8), "op"), (lambda: file(op=-1), "op"),
        (lambda: geom(flags=2), "flags"), (lambda: geom(flags=-1), "flags"), (lambda: dev(flags=4), "flags"), (lambda: file(flags=3), "flags"),
        (lambda: geom(sampling=2), "sampling"), (lambda: dev(sampling=2), "sampling"), (lambda: dev(sampling=-1), "sampling"),
        (lambda: geom(wh=(0, H)), "width/height"), (lambda: geom(wh=(W, -3)), "width/height"), (lambda: geom(wh=(65536, H)), "width/height"),
        (lambda: dev(wh=(0, H)), "width/height"), (lambda: dev(wh=(W, 0)), "width/height"),
        (lambda: dev(nf=0), "n_frames"), (lambda: dev(nf=-2), "n_frames"),
        (lambda: dev(d_in=None), "null"), (lambda: dev(d_out=None), "null"), (lambda: tables(src=None), "null"), (lambda: tables(dst=None), "null"),
        (lambda: file(data=None), "null"), (lambda: file(inf=None), "null"), (lambda: file(n=0), "empty"),
        (lambda: dev(d_in=C.c_void_p(base + 2)), "16-byte aligned"), (lambda: dev(d_out=C.c_void_p(base + 3 * frame + 8)), "16-byte aligned"),
        (lambda: dev(d_out=a), "overlap"), (lambda: dev(d_out=C.c_void_p(base + frame - 16)), "overlap"),
        (lambda: dev(nf=4), "overlap"),                                   # four frames of input reach into d_out, three frames on
        (lambda: dev(d_in=b, d_out=C.c_void_p(base + 3 * frame - 16)), "overlap"),
        (lambda: file(comment=b"x" * 397), "JPEZY_MAX_COMMENT"),
    ]
    for i, (call, names) in enumerate(cases):
        assert call() == E_BADARG, (i, names)
        assert names in _err(lib), (i, names, _err(lib))
    assert dev(nf=3) == E_BADARG and "context" in _err(lib)               # three frames end where d_out begins: no overlap
    assert dev(d_out=C.c_void_p(base + frame)) == E_BADARG and "context" in _err(lib)
    # the edge rule is an argument check of the device entry too: UNSUPPORTED without trim, as far as the context with it
    assert dev(op=1, wh=(40, 24)) == -4 and "width" in _err(lib) and "16" in _err(lib)
    assert dev(op=1, wh=(40, 24), flags=1) == E_BADARG and "context" in _err(lib)
    for name, call in (("transform_geometry", geom), ("quant_tables_transform", tables), ("coeff_transform_dev", dev), ("transform_jpeg", file)):
        assert call(op=9) == E_BADARG and _err(lib).startswith(name + ":"), _err(lib)


def test_header_declares_the_transform_section(J):
    text = (ROOT / "include" / "jpezy_hip.h").read_text()
    assert "LOSSLESS TRANSFORMS" in text
    section = text[text.index("LOSSLESS TRANSFORMS"):]
    for phrase in ("NOT carried", "APPn segments (EXIF, ICC)", "density", "NOT provided", "-32768 stays -32768", "Q'[v][u] = Q[u][v]"):
        assert phrase in section, phrase
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = J.load_library()
    for kind, name in (("int", "jpezy_transform_geometry"), ("int", "jpezy_coeff_transform_dev"), ("int", "jpezy_quant_tables_transform"),
                       ("long", "jpezy_transform_jpeg")):
        assert re.search(r"\b" + kind + r"\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in {n for n, _, _ in J.api.ABI}
    values = dict(re.findall(r"JPEZY_XFORM_(\w+) = (\d)", code))
    assert values == {"NONE": "0", "HFLIP": "1", "VFLIP": "2", "TRANSPOSE": "3", "TRANSVERSE": "4", "ROT90": "5", "ROT180": "6", "ROT270": "7"}
    assert [J.XFORM_NONE, J.XFORM_HFLIP, J.XFORM_VFLIP, J.XFORM_TRANSPOSE, J.XFORM_TRANSVERSE, J.XFORM_ROT90, J.XFORM_ROT180,
            J.XFORM_ROT270] == list(range(8)) and J.XFORM_TRIM == 1
    assert re.search(r"#define\s+JPEZY_XFORM_TRIM\s+1\b", code)
