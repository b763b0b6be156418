"""Quality 1..100 and caller-supplied quantisation tables (include/jpezy_hip.h), as far as they can be checked without
a GPU: the model against the oracle, the quality mapping against libjpeg's (Pillow), the argument rules, the host writer with tables,
the size bound, and host restatements of the three device-side facts the setting rests on -- both create-time DC checks and the
level-1 guard band for every table that matters, and the 32-bit range of encode variant 0's fixed point."""
import ctypes as C
import io
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import quant_model as QM
from jpeg_synth import ZZ

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(16, 16), (64, 16), (80, 48), (33, 17)]
f32 = np.float32


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _dqt_tables(jpg):
    """{table id: 64 entries in natural order} of a file's 8-bit DQT segments"""
    out, i = {}, 2
    while i < len(jpg):
        assert jpg[i] == 0xFF
        mk, n = jpg[i + 1], struct.unpack(">H", jpg[i + 2:i + 4])[0]
        if mk == 0xDA:
            break
        if mk == 0xDB:
            j, end = i + 4, i + 2 + n
            while j < end:
                assert jpg[j] >> 4 == 0                       # Pq = 0
                t = np.zeros(64, np.int64)
                t[ZZ] = list(jpg[j + 1:j + 65])
                out[jpg[j] & 15] = t
                j += 65
        i += 2 + n
    return out


# ---- the model ----
@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("W,H", SHAPES)
def test_model_equals_the_oracle_at_the_annex_k_tables(oracle, W, H, gray):
    c = oracle.constants()
    r, g, b = oracle.synth_rgb(W, H)
    assert np.array_equal(QM.quantise(QM.synth_dct(W, H, gray), c["qt_luma"], c["qt_chroma"]), oracle.encode_coeffs(r, g, b, W, H, gray))


def test_ycc_model_with_the_custom_divide_equals_ycc_model_at_annex_k(oracle):
    import ycc_model as YM
    c = oracle.constants()
    for W, H in SHAPES:
        y, cb, cr = YM.synth_planes(W, H, "random")
        assert np.array_equal(QM.quantise(QM.dct_from_ycc(y, cb, cr), c["qt_luma"], c["qt_chroma"]), YM.synth_coeffs(W, H, "random"))


# ---- quality mapping ----
def test_quality_tables_equal_libjpegs_for_every_quality(J, oracle):
    from PIL import Image
    c = oracle.constants()
    im = Image.fromarray(np.zeros((8, 8, 3), np.uint8))
    for q in range(1, 101):
        luma, chroma = J.quality_tables(q)
        buf = io.BytesIO()
        im.save(buf, "JPEG", quality=q)
        t = _dqt_tables(buf.getvalue())
        assert np.array_equal(luma, t[0]) and np.array_equal(chroma, t[1]), q
        ml, mc = QM.quality_tables(q)
        assert np.array_equal(luma, ml) and np.array_equal(chroma, mc), q
    luma, chroma = J.quality_tables(50)
    assert np.array_equal(luma, c["qt_luma"]) and np.array_equal(chroma, c["qt_chroma"])
    assert all((t == 255).all() for t in J.quality_tables(1)) and all((t == 1).all() for t in J.quality_tables(100))


def test_argument_errors(J):
    lib = J.load_library()
    for q in (0, 101, -5):
        with pytest.raises(J.JpezyError, match="status -1"):
            J.quality_tables(q)
    ones = np.ones(64, np.uint8)
    zero = ones.copy()
    zero[17] = 0
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    z = np.zeros(6 * 64, np.int16)
    buf = np.zeros(4096, np.uint8)
    # the writer and the probe take the setter's rules: a zero entry, one null pointer of two
    for luma, chroma in ((zero, ones), (ones, zero)):
        assert lib.jpezy_write_jpeg_qt(p(z), 16, 16, 0, b"", p(luma), p(chroma), 0, 0, p(buf), buf.size) == -1
        assert lib.jpezy_quant_tables_probe(p(luma), p(chroma), None, None, None) == -1
    for luma, chroma in ((None, p(ones)), (p(ones), None)):
        assert lib.jpezy_write_jpeg_qt(p(z), 16, 16, 0, b"", luma, chroma, 0, 0, p(buf), buf.size) == -1
        assert lib.jpezy_quant_tables_probe(luma, chroma, None, None, None) == -1
    # the context's setters answer a null context before anything else (their table rules on a GPU: tests/test_gpu_quant.py)
    assert lib.jpezy_ctx_set_quant_tables(None, p(ones), p(ones)) == -1 and lib.jpezy_ctx_set_quality(None, 50) == -1
    assert lib.jpezy_ctx_quant_tables(None, p(buf), p(buf)) == -1
    assert lib.jpezy_quality_tables(50, None, p(buf)) == -1
    with pytest.raises(J.JpezyError):
        J.write_jpeg(z, 16, 16, quant_tables=(np.full(64, 256), ones))


# ---- the host writer ----
def _fields(W, H):
    rng = np.random.default_rng(W * 131 + H)
    n = ((W + 15) // 16) * ((H + 15) // 16)
    co = rng.integers(-40, 41, (n, 6, 64)).astype(np.int16)
    co[..., 20:] *= (rng.random((n, 6, 44)) < 0.2)
    co[..., 0] = rng.integers(-1000, 1001, (n, 6))
    co[::3, 0, 5] = 1020
    return co


@pytest.mark.parametrize("name", ["q1", "q90", "q100", "random", "ones_dc255"])
def test_host_writer_files_parse_back_with_every_reader(J, oracle, name):
    from PIL import Image
    luma, chroma = QM.tables(name)
    W, H = 80, 48
    co = _fields(W, H)
    for opt, ri in ((False, 0), (True, 0), (False, 4), (True, 4)):
        jpg = J.write_jpeg(co, W, H, optimize=opt, restart_interval=ri, quant_tables=(luma, chroma))
        info, back = J.read_jpeg(jpg)
        assert np.array_equal(back.reshape(co.shape), co)
        assert np.array_equal(np.array(info.qt[0][:]), luma) and np.array_equal(np.array(info.qt[1][:]), chroma)
        assert [info.Tq[i] for i in range(3)] == [0, 1, 1] and info.restart_interval == ri
        oinfo, oback = oracle.read_jpeg(jpg)
        assert np.array_equal(oback.reshape(co.shape), co)
        assert np.array_equal(np.array(oinfo.qt[0][:]), luma) and np.array_equal(np.array(oinfo.qt[1][:]), chroma)
        t = _dqt_tables(jpg)
        assert np.array_equal(t[0], luma) and np.array_equal(t[1], chroma)
        im = Image.open(io.BytesIO(jpg))
        im.load()                                              # libjpeg decodes the whole scan
        assert im.size == (W, H)
        pq = {k: np.asarray(v) for k, v in im.quantization.items()}
        # (Pillow hands the tables over in natural or in zig-zag order depending on its version)
        for k, want in ((0, luma), (1, chroma)):
            nat = np.zeros(64, np.int64)
            nat[ZZ] = pq[k]
            assert np.array_equal(pq[k], want) or np.array_equal(nat, want)


def test_host_writer_with_null_tables_gives_the_bytes_of_write_jpeg_rst(J, oracle):
    lib = J.load_library()
    c = oracle.constants()
    W, H = 80, 48
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for gray in (False, True):
        co = np.ascontiguousarray(_fields(W, H)[:, :4 if gray else 6])
        cap = lib.jpezy_jpeg_bound(W, H)
        for opt, ri in ((0, 0), (1, 0), (0, 4), (1, 4)):
            buf = np.zeros(cap, np.uint8)
            n = lib.jpezy_write_jpeg_qt(p(co), W, H, int(gray), b"note", None, None, ri, opt, p(buf), cap)
            want = J.write_jpeg(co, W, H, gray=gray, comment=b"note", optimize=bool(opt), restart_interval=ri)
            assert n == len(want) and buf[:n].tobytes() == want, (gray, opt, ri)
            # ... and so do the Annex-K tables handed over explicitly
            assert J.write_jpeg(co, W, H, gray=gray, comment=b"note", optimize=bool(opt), restart_interval=ri,
                                quant_tables=(c["qt_luma"], c["qt_chroma"])) == want


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("W,H", [(1, 1), (16, 16), (17, 17), (65535, 1)])
def test_size_bound_holds_with_all_ones_tables_in_the_header(J, W, H, gray):
    from tests.test_jpeg_bound import HEADER_NO_COMMENT, MAX_COMMENT, _comment, worst_field
    ones = np.ones(64, np.uint8)
    co = worst_field(W, H, gray)
    jpg = J.write_jpeg(co, W, H, gray=gray, comment=_comment(MAX_COMMENT), quant_tables=(ones, ones))
    plain = J.write_jpeg(co, W, H, gray=gray, comment=_comment(MAX_COMMENT))
    assert len(jpg) == len(plain) <= J.load_library().jpezy_jpeg_bound(W, H)           # the DQT segments have a fixed length
    sos = jpg.index(b"\xff\xda")
    assert sos + 2 + int.from_bytes(jpg[sos + 2:sos + 4], "big") == HEADER_NO_COMMENT + MAX_COMMENT + 5 <= 1024


# ---- the level-1 guard band and the two DC checks, restated in numpy with the kernel's FP32 operations ----
def fma(a, b, c):
    # float32 fused multiply-add: the product of two float32 is exact in float64; one rounding
    return (np.asarray(a, f32).astype(np.float64) * np.float64(b) + np.asarray(c, f32).astype(np.float64)).astype(f32)


def delta1_restated(c, qt):
    """DeviceTables::f32col[t][j].delta1 for every block column j as build_encode_tables forms it: 1.25 x the worst level-1 bound over
    the column's coefficients, the DC left out"""
    cos = c["cos"].reshape(8, 8)
    s = c["inv_sqrt2"]
    cu = np.where(np.arange(8) == 0, s, 1.0)
    absum = np.zeros(8)
    for x in range(8):                                         # the builder's order of summation
        absum = absum + np.abs(cos[:, x])
    out = np.zeros(8, f32)
    for j in range(8):
        worst = 0.0
        for i in range(8):
            if i == 0 and j == 0:
                continue
            ks = cu[j] * cu[i] / (4.0 * float(qt[i * 8 + j]))
            amp = 128.0 * absum[i] * absum[j] * ks
            worst = max(worst, 13.0 * 2.0 ** -24 * amp + 2.0 ** -23 * amp)
        out[j] = f32(1.25 * worst)
    return out


def dc_checks_restated(c, Q, delta1):
    """-> (want, formula_ok, generic_ok, generic, flagged): DeviceTables::dcq for DC quantiser Q, whether f32::dc_formula reproduces it,
    whether the level-1 quantiser with dc_formula on its flagged sums may be used (both create-time checks), what that path gives and
    which sums its guard test flags"""
    s = c["inv_sqrt2"]
    S = np.arange(-8192, 8193)
    dct = np.trunc(((S * s) * s) / 4).astype(np.int64)
    want = np.sign(dct) * (np.abs(dct) // Q)
    a = np.abs(S).astype(f32)
    d = np.trunc(fma(a, f32(0.125), np.full(a.shape, -0.125, f32)))
    rq, bias = f32(1.0) / f32(Q), f32(0.5) / f32(Q)
    formula = np.copysign(np.trunc(fma(d, rq, np.full(a.shape, bias, f32))), S).astype(np.int64)
    ks = f32(s * s / (4.0 * Q))
    tp = fma(S.astype(f32), ks, np.full(S.shape, delta1, f32))
    flagged = (tp - np.floor(tp)).astype(f32) < f32(delta1) + f32(delta1)
    generic = np.where(flagged, formula, np.trunc(tp).astype(np.int64))
    formula_ok = bool(np.array_equal(formula, want))
    return want, formula_ok, formula_ok and bool(np.array_equal(np.where(flagged, want, generic), want)), generic, flagged


def _dc_cases():
    """(name, luma, chroma): (a) the quality tables, (b) all ones with only the DC entry varied over 1..255, and the custom sets"""
    for q in range(1, 101):
        yield (f"q{q}",) + QM.quality_tables(q)
    for q0 in range(1, 256):
        t = np.ones(64, np.uint8)
        t[0] = q0
        yield f"ones_dc{q0}", t, t.copy()
    for name in ("random", "255_dc1"):
        yield (name,) + QM.custom_tables(name)


def test_both_dc_checks_and_the_level1_band_for_every_dc_quantiser(J, oracle):
    """For every table set: delta1 as the builder computes it equals the restatement and stays below 0.25; the path the builder chooses
    for the DC -- the level-1 quantiser with dc_formula on the flagged sums (DCG), or the exact table when a check fails -- reproduces
    int(((S s) s) / 4) / Q for every block sum S.  Every DC quantiser 1..255 is covered (b), the quality tables bring their own column-0
    guard bands (a)."""
    c = oracle.constants()
    seen, fallback = set(), set()
    for name, luma, chroma in _dc_cases():
        d1, dcg, _ = J.quant_tables_probe(luma, chroma)
        for t, qt in enumerate((luma, chroma)):
            want1 = delta1_restated(c, qt)
            assert np.array_equal(d1[t], want1), (name, t)
            assert float(d1[t].max()) < 0.25
            Q = int(qt[0])
            seen.add(Q)
            want, formula_ok, generic_ok, generic, flagged = dc_checks_restated(c, Q, d1[t][0])
            assert dcg[t] == int(generic_ok), (name, t, Q)
            assert np.abs(want).max() == 1023 // Q and np.abs(want).max() < 2 ** 15          # what the 16-bit table must hold
            if generic_ok:
                assert np.array_equal(generic, want), (name, t)
                # flagged sums take dc_formula: every multiple of 8 Q is among them (more with a wide band beside a large DC quantiser)
                assert flagged[np.arange(-8192, 8193) % (8 * Q) == 0].all()
            else:
                # the launcher takes the !DCG instance and the exact table, `want` itself.  It is always dc_formula that fails, never
                # the quantiser on an unflagged sum
                assert not formula_ok and np.array_equal(np.where(flagged, want, generic), want), (name, t)
                fallback.add(Q)
    assert seen == set(range(1, 256))
    # Which DC quantisers fall back: s * s = 0.4999999999999999 puts int(((S s) s) / 4) at (|S| - 1) >> 3, which is what
    # dc_formula computes -- except at the four |S| where the FP64 product rounds up to S / 2 exactly and the value is |S| / 8.  There the
    # formula is one short, and that shows exactly when Q divides |S| / 8.
    s2 = c["inv_sqrt2"]
    S = np.arange(1, 8193)
    exact = S[np.trunc(((S * s2) * s2) / 4) * 8 == S] // 8
    assert exact.tolist() == [369, 379, 738, 758]
    assert fallback == {Q for Q in range(1, 256) if any(v % Q == 0 for v in exact)} == {1, 2, 3, 6, 9, 18, 41, 82, 123, 246}
    # the guard of the builder: the largest band any table of entries >= 1 can have is that of Q = 1, far below 0.25
    ones = np.ones(64, np.uint8)
    assert 1.0e-3 < float(J.quant_tables_probe(ones, ones)[0].max()) < 1.2e-3


def test_uneven_table_flags_more_sums_than_the_multiples_of_8q(J, oracle):
    """Q[0] = 255 beside entries of 1: column 0's delta1 (8e-4, from the 1s) exceeds 1 / (8 Q[0]) = 4.9e-4, so the guard test flags
    sums that are no multiple of 8 Q[0]; they take dc_formula, and the result is still the table's"""
    c = oracle.constants()
    luma, chroma = QM.custom_tables("ones_dc255")
    d1, dcg, _ = J.quant_tables_probe(luma, chroma)
    assert float(d1[0][0]) > 1.0 / (8 * 255)
    want, _, generic_ok, generic, flagged = dc_checks_restated(c, 255, d1[0][0])
    assert flagged.sum() > (np.arange(-8192, 8193) % (8 * 255) == 0).sum()
    assert generic_ok and dcg == [1, 1] and np.array_equal(generic, want)


# ---- encode variant 0: the fixed point of its quotients ----
@pytest.mark.parametrize("name", ["ones", "all255", "q1", "q50", "q100", "255_dc1", "ones_dc255"])
def test_variant0_fixed_point_stays_inside_int32(J, oracle, name):
    """n = (int)(F * qscale) with qscale = cu cv / (4 Q) * 2^bits at the extreme amplitudes: |F[i][j]| <= 128 * sum|cos_i| * sum|cos_j|
    for the two butterfly passes' output, and the block sum +-8192 at (0, 0); bits is the widest width that keeps |n| < 2^31 under the
    bound |v| <= 1024 the host uses, never more than 24"""
    c = oracle.constants()
    if name in ("ones", "all255"):
        luma = chroma = np.full(64, 1 if name == "ones" else 255, np.uint8)
    else:
        luma, chroma = QM.tables(name)
    bits = J.quant_tables_probe(luma, chroma)[2]
    qmin = int(min(luma.min(), chroma.min()))
    assert bits == max(b for b in range(25) if 1024 * 2 ** b < qmin * 2 ** 31)
    assert bits == {1: 20, 255: 24}.get(qmin, bits) and (name != "q50" or bits == 24)
    cos = np.abs(c["cos"].reshape(8, 8)).sum(axis=1)
    s = c["inv_sqrt2"]
    cu = np.where(np.arange(8) == 0, s, 1.0)
    amp = 128.0 * np.outer(cos, cos)                           # [i][j]
    amp[0, 0] = 8192.0
    for qt in (luma, chroma):
        qscale = np.outer(cu, cu) / (4.0 * qt.reshape(8, 8).astype(np.float64)) * float(1 << bits)
        n = amp * qscale
        assert n.max() < 2.0 ** 31 - 1, (name, n.max())
        # one unit of the fixed point, as a distance on v / Q, against the 3e-11 the kernel's comment derives for the FP64 error:
        # three orders of magnitude at the widest width, more at every narrower one
        assert 2.0 ** -bits > 1e3 * 3e-11


# ---- CLI ----
def test_cli_quality_argument_rules(tmp_path, oracle):
    """--quality=N is one token, parsed the way --restart=N is: a malformed or out-of-range N is the usage error, in single-file mode
    and with --i420 (the files themselves: tests/test_gpu_quant.py)"""
    from jpezy_amd import _build
    _build.build_all()
    enc = Path(_build.BIN) / "jpezy_encode"
    run = lambda *a: subprocess.run([str(x) for x in a], capture_output=True, text=True, timeout=120)
    src = tmp_path / "in.ppm"
    r, g, b = oracle.synth_rgb(16, 16)
    src.write_bytes(oracle.format_ppm_p3(16, 16, r, g, b))
    usage = run(enc, src)
    assert usage.returncode != 0 and usage.stderr.startswith("Usage: jpezy_encode")
    for bad in ("--quality=", "--quality=x", "--quality=0", "--quality=101", "--quality=-1", "--quality=5x", "--quality=123456", "--quality=9 0"):
        p = run(enc, src, tmp_path / "b.jpg", bad)
        assert p.returncode == usage.returncode and p.stderr == usage.stderr and "by roki" not in p.stdout, bad
        p = run(enc, src, tmp_path / "b.jpg", "--gray", "--restart=3", bad)
        assert p.returncode == usage.returncode and p.stderr == usage.stderr, bad
    yuv = tmp_path / "in.yuv"
    yuv.write_bytes(bytes(16 * 16 + 2 * 8 * 8))
    i420_usage = run(enc, "--i420=16x16", yuv)
    assert i420_usage.returncode != 0 and "--quality=N" in i420_usage.stderr
    for bad in ("--quality=", "--quality=0", "--quality=101", "--quality=7.5"):
        p = run(enc, "--i420=16x16", yuv, tmp_path / "c.jpg", "--optimize", bad)
        assert p.returncode == i420_usage.returncode and p.stderr == i420_usage.stderr, bad
    assert not (tmp_path / "b.jpg").exists() and not (tmp_path / "c.jpg").exists()
