"""4:4:4 chroma sampling, host side (include/jpezy_hip.h, CHROMA SAMPLING): the host writer's bytes against tests/sampling_model.py, the
reader's view of those files, the size bound, the symbol histogram, the rules of the ABI and of the CLI.  No GPU."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import quant_model as QM
import sampling_model as SM

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "jpezy_amd" / "bin"
BADARG, UNSUPPORTED = -1, -4
SIZES = [(176, 64), (33, 17)]
TABLES = ["annex_k", "q90", "random"]
RESTARTS = [0, 1, 5, 22]
MAX_COMMENT = 396


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _tables(name):
    return None if name == "annex_k" else QM.tables(name)


@pytest.fixture(scope="module")
def fields(oracle):
    """model coefficients of the synthetic picture per (W, H, tables): computed once, read-only"""
    out = {}
    for (W, H), name in itertools.product(SIZES, TABLES):
        c = oracle.constants()
        luma, chroma = _tables(name) or (c["qt_luma"], c["qt_chroma"])
        co = SM.quantise(SM.synth_dct(W, H), luma, chroma)
        co.setflags(write=False)
        out[W, H, name] = co
    return out


def test_model_agrees_with_420_where_the_definitions_share_a_sample(oracle):
    """16 x 16: Y of every pixel and Cb / Cr of the even pixel positions are the samples the 4:2:0 definition (quant_model) takes"""
    W = H = 16
    r, g, b = oracle.synth_rgb(W, H, frame=3)
    ys, cbs, crs = SM.samples_from_rgb(r, g, b, W, H)
    rows = cols = np.arange(16)
    rf, gf, bf = (np.asarray(p).reshape(H, W).astype(np.float64) for p in (r, g, b))
    y420 = np.trunc((0.2990 * rf) + (0.5870 * gf) + (0.1140 * bf) - 128).astype(np.int32)
    assert np.array_equal(ys, y420)
    # the 4:2:0 blocks themselves: quant_model's unquantised DCT of the decimated planes equals the DCT of our planes decimated
    d420 = QM.dct_from_rgb(r, g, b, W, H)
    assert np.array_equal(d420[0, 0, 4], QM.fdct_blocks(cbs[::2, ::2].reshape(1, 64))[0])
    assert np.array_equal(d420[0, 0, 5], QM.fdct_blocks(crs[::2, ::2].reshape(1, 64))[0])
    yb = ys.reshape(2, 8, 2, 8).transpose(0, 2, 1, 3).reshape(4, 64)
    assert np.array_equal(d420[0, 0, :4], QM.fdct_blocks(yb))
    # and the four luma blocks of the 4:2:0 MCU are the luma blocks of the four 4:4:4 MCUs
    d444 = SM.dct_from_rgb(r, g, b, W, H)
    assert np.array_equal(d444[:, :, 0].reshape(4, 64), d420[0, 0, :4])
    assert rows.size == cols.size


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("ri", RESTARTS)
@pytest.mark.parametrize("name", TABLES)
@pytest.mark.parametrize("W,H", SIZES)
def test_host_writer_bytes_and_read_back(J, fields, W, H, name, ri, optimize):
    co = fields[W, H, name]
    qt = _tables(name)
    jpg = J.write_jpeg(co, W, H, sampling=J.SAMPLING_444, quant_tables=qt, restart_interval=ri, optimize=optimize)
    assert jpg == SM.write_jpeg(co, W, H, quant_tables=qt, ri=ri, optimize=optimize)
    assert len(jpg) <= J.jpeg_bound(W, H, J.SAMPLING_444)
    info, back = J.read_jpeg(jpg)
    assert (info.width, info.height, info.ncomp) == (W, H, 3)
    assert list(info.H) == [1, 1, 1] and list(info.V) == [1, 1, 1] and info.blocks_per_mcu == 3
    assert (info.mcu_cols, info.mcu_rows) == SM.geometry(W, H)[:2]
    assert np.array_equal(np.asarray(back).reshape(co.shape), co)
    if qt is not None:
        assert np.array_equal(np.asarray(info.qt[0][:64]), qt[0]) and np.array_equal(np.asarray(info.qt[1][:64]), qt[1])


def worst_field(W, H):
    """tests/test_jpeg_bound.py's field for 3-block MCUs: every DC difference of category 11, every AC +1023"""
    mc, mr, _ = SM.geometry(W, H)
    co = np.full((mc * mr, 3, 64), 1023, np.int16)
    co[:, :, 0] = np.where(np.arange(mc * mr) % 2 == 0, 1023, -1023).astype(np.int16)[:, None]
    return co


@pytest.mark.parametrize("ri", [0, 1])
@pytest.mark.parametrize("W,H", [(1, 1), (8, 8), (9, 9), (65535, 1), (33, 17)])
def test_bound_holds_for_worst_fields(J, W, H, ri):
    import entropy_model as M
    comment = bytes((0x41 + i % 26) for i in range(MAX_COMMENT - (6 if ri else 0)))
    bound = J.jpeg_bound(W, H, J.SAMPLING_444)
    nmcu = SM.geometry(W, H)[0] * SM.geometry(W, H)[1]
    assert bound == 1024 + 1344 * nmcu
    # analytic: the longest header, 1661 bits per block, every byte stuffed, per interval pad + stuffed pad + marker, EOI
    assert 623 + MAX_COMMENT + 5 + 2 * ((nmcu * 3 * 1661 + 7) // 8) + 4 * nmcu + 2 <= bound
    for sign in (1, -1):          # -1023: value bits 0000000000 behind the code; +1023: all ones, the 0xFF-heavy field
        co = worst_field(W, H)
        co[:, :, 1:] *= sign
        jpg = J.write_jpeg(co, W, H, sampling=J.SAMPLING_444, comment=comment, restart_interval=ri)
        assert len(jpg) <= bound, (W, H, ri, sign, len(jpg), bound)
        if nmcu <= 15:
            assert jpg == SM.write_jpeg(co, W, H, comment=comment, ri=ri)
    if nmcu > 1 and nmcu <= 15:
        lens = [M.block_bits(z, p, t) for z, p, t in SM.coded_blocks(worst_field(W, H))]
        assert max(lens[3:]) == 1658                      # a luma block with the Annex-K codes: 9 + 11 + 63 x 26
    # the 4:2:0 bound cannot serve: per 16 x 16 pixels it allows 2688 bytes, twelve worst-case blocks stuffed take 4983
    assert 2 * ((12 * 1661 + 7) // 8) > 6 * 64 * 7


@pytest.mark.parametrize("ri", [0, 5])
def test_symbol_histogram_matches_model(J, fields, ri):
    co = fields[33, 17, "q90"]
    want, ok = SM.symbol_counts(co, ri)
    assert ok
    got = J.huffman_histogram(co, 33, 17, sampling=J.SAMPLING_444, restart_interval=ri)
    assert np.array_equal(got.astype(np.int64), want)
    bad = np.array(co).copy()
    bad[0, 0, 1, 5] = 2000
    with pytest.raises(J.JpezyError, match="status -5"):
        J.huffman_histogram(bad, 33, 17, sampling=J.SAMPLING_444)


def test_geometry_helpers(J):
    for W, H in itertools.product([1, 7, 8, 9, 65535], repeat=2):
        assert J.sampling_geometry(J.SAMPLING_444, W, H) == ((W + 7) // 8, (H + 7) // 8, 3)
        assert J.sampling_geometry(J.SAMPLING_420, W, H) == ((W + 15) // 16, (H + 15) // 16, 6)
        assert J.coeff_count(W, H, sampling=J.SAMPLING_444) == 192 * ((W + 7) // 8) * ((H + 7) // 8)
        assert J.coeff_count(W, H, sampling=J.SAMPLING_420) == J.coeff_count(W, H)
        assert J.jpeg_bound(W, H, J.SAMPLING_420) == J.load_library().jpezy_jpeg_bound(W, H)
    lib = J.load_library()
    for bad in (-1, 2, 444):
        assert lib.jpezy_sampling_geometry(bad, 8, 8, None, None, None) == BADARG
        assert lib.jpezy_coeff_count_sampling(8, 8, bad) == 0 and lib.jpezy_jpeg_bound_sampling(8, 8, bad) == 0
        with pytest.raises(J.JpezyError, match="status -1"):
            J.sampling_geometry(bad, 8, 8)
    for W, H in ((0, 8), (8, 0), (65536, 8)):
        assert lib.jpezy_sampling_geometry(1, W, H, None, None, None) == BADARG
        assert lib.jpezy_coeff_count_sampling(W, H, 1) == 0


def test_abi_refusals_and_420_twins(J, oracle):
    lib = J.load_library()
    W, H = 33, 17
    rng = np.random.default_rng(7)
    co444 = rng.integers(-40, 41, J.coeff_count(W, H, sampling=J.SAMPLING_444)).astype(np.int16)
    cap = J.jpeg_bound(W, H, J.SAMPLING_444)
    buf = np.zeros(cap, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    # gray + 444, bad sampling
    assert lib.jpezy_write_jpeg_sampling(p(co444), W, H, 1, 1, b"x", None, None, 0, 0, p(buf), cap) == BADARG
    assert b"gray" in lib.jpezy_hip_last_error()
    for bad in (-1, 2):
        assert lib.jpezy_write_jpeg_sampling(p(co444), W, H, bad, 0, b"x", None, None, 0, 0, p(buf), cap) == BADARG
        assert b"sampling" in lib.jpezy_hip_last_error()
    with pytest.raises(J.JpezyError, match="status -1"):
        J.write_jpeg(co444, W, H, gray=True, sampling=J.SAMPLING_444)
    # one table of two, a zero entry
    t = np.full(64, 3, np.uint8)
    assert lib.jpezy_write_jpeg_sampling(p(co444), W, H, 1, 0, b"x", p(t), None, 0, 0, p(buf), cap) == BADARG
    z = t.copy(); z[9] = 0
    assert lib.jpezy_write_jpeg_sampling(p(co444), W, H, 1, 0, b"x", p(t), p(z), 0, 0, p(buf), cap) == BADARG
    # too small a buffer: JPEZY_E_NOSPACE, never a partial file reported as one
    assert lib.jpezy_write_jpeg_sampling(p(co444), W, H, 1, 0, b"x", None, None, 0, 0, p(buf), 700) == -6
    # SAMPLING_420 is the old entry, byte for byte, gray included
    for gray in (False, True):
        co = rng.integers(-40, 41, J.coeff_count(W, H, gray)).astype(np.int16)
        for ri, opt, qt in ((0, False, None), (3, True, QM.tables("q90")), (1, False, QM.tables("random"))):
            old = J.write_jpeg(co, W, H, gray=gray, restart_interval=ri, optimize=opt, quant_tables=qt)
            n = lib.jpezy_write_jpeg_sampling(p(co), W, H, 0, int(gray), b"Encoded by JPEZY" if gray else b"Encoded by jpezy",
                                              p(qt[0]) if qt else None, p(qt[1]) if qt else None, ri, int(opt), p(buf), cap)
            assert n > 0 and buf[:n].tobytes() == old
            if not gray and ri == 0 and not opt and qt is None:
                assert old == oracle.write_jpeg(co, W, H)
    import huffopt_model as HM
    co = rng.integers(-40, 41, J.coeff_count(W, H)).astype(np.int16)
    assert np.array_equal(J.huffman_histogram(co, W, H, sampling=J.SAMPLING_420).astype(np.int64), HM.symbol_counts(co)[0])


def test_pil_opens_a_444_file(J, fields):
    Image = pytest.importorskip("PIL.Image")
    import io
    jpg = J.write_jpeg(fields[33, 17, "q90"], 33, 17, sampling=J.SAMPLING_444, quant_tables=QM.tables("q90"), restart_interval=5, optimize=True)
    im = Image.open(io.BytesIO(jpg))
    im.load()
    assert im.size == (33, 17) and im.mode == "RGB"


# ---- CLI rules ----
@pytest.fixture(scope="module")
def enc():
    from jpezy_amd import _build
    _build.build_all()
    exe = BIN / "jpezy_encode"
    assert exe.exists()
    return exe


def _run(*args):
    return subprocess.run([str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_cli_sampling_rules(enc, tmp_path):
    ppm = tmp_path / "x.ppm"
    ppm.write_text("P3\n2 2\n255\n" + "1 2 3 " * 4 + "\n")
    out = tmp_path / "y.jpg"
    for form in ("--sampling=", "--sampling=422", "--sampling=4444", "--sampling=444x"):
        p = _run(enc, ppm, out, form)
        assert p.returncode == 1 and p.stderr.startswith("Usage: jpezy_encode") and not out.exists(), form
    rule = "--sampling=444 writes colour files from RGB input on one GPU"
    for opts in (["--gray", "--sampling=444"], ["--sampling=444", "--gray"], ["--optimize", "--gray", "--sampling=444"]):
        p = _run(enc, ppm, out, *opts)
        assert p.returncode == 1 and rule in p.stderr and "Usage" not in p.stderr and not out.exists(), opts
    yuv = tmp_path / "x.yuv"
    yuv.write_bytes(bytes(6))
    p = _run(enc, "--i420=2x2", yuv, out, "--sampling=444")
    assert p.returncode == 1 and rule in p.stderr and not out.exists()
    p = _run(enc, "--gpus", 2, "--sampling=444", ppm, out)
    assert p.returncode == 1 and rule in p.stderr and not out.exists()
    p = _run(enc, "--gpus", 1, "--gray", "--sampling=444", ppm, out)
    assert p.returncode == 1 and rule in p.stderr and not out.exists()
