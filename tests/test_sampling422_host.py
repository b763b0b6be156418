"""4:2:2 chroma sampling, host side (include/jpezy_hip.h, CHROMA SAMPLING): tests/sampling422_model.py tied to the 4:4:4
and 4:2:0 definitions where they share a sample, the host writer's bytes against it, the reader's and the oracle decoder's view of those
files, the size bound, the symbol histogram and the rules of the ABI.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

import quant_model as QM
import sampling422_model as S2
import sampling_model as SM

BADARG, FORMAT, NOSPACE = -1, -5, -6
WIDTHS, HEIGHTS = [1, 15, 16, 17, 33], [1, 7, 8, 9, 17]
TABLES = ["q10", "q50", "q100"]
MAX_COMMENT = 396


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _restarts(W, H):
    mc, mr, _ = S2.geometry(W, H)
    return [0, 1, 5, mc * mr + 3]


@pytest.fixture(scope="module")
def fields(oracle):
    """model coefficients of the synthetic picture per (W, H, tables): the transform once per size, read-only"""
    out = {}
    for W, H, name in itertools.product(WIDTHS, HEIGHTS, TABLES):
        co = S2.quantise(S2.synth_dct(W, H), *QM.tables(name))
        co.setflags(write=False)
        out[W, H, name] = co
    return out


# ---- the definition against the two that exist ----
@pytest.fixture(scope="module")
def picture(oracle):
    W, H = 37, 19
    return (W, H) + tuple(oracle.synth_rgb(W, H, frame=3))


def test_luma_is_the_444_luma_block_for_block(picture):
    W, H, r, g, b = picture
    d422, d444 = S2.dct_from_rgb(r, g, b, W, H), SM.dct_from_rgb(r, g, b, W, H)
    mc, mr, _ = S2.geometry(W, H)
    y444 = np.zeros((mr, 2 * mc, 64), np.int32)          # the 4:4:4 grid may be one 8-pixel column short of whole 16 x 8 MCUs
    y444[:, :d444.shape[1]] = d444[:, :, 0]
    if d444.shape[1] < 2 * mc:                           # that column holds clamped duplicates of column W - 1: compute it from the samples
        ys = S2.samples_from_rgb(r, g, b, W, H)[0]
        y444[:, -1] = QM.fdct_blocks(S2._blocks(ys, mr, 2 * mc)[:, -1])
    assert np.array_equal(d422[:, :, :2].reshape(mr, 2 * mc, 64), y444)


def test_point_chroma_is_the_444_chroma_at_even_x(picture):
    W, H, r, g, b = picture
    _, cb2, cr2 = S2.samples_from_rgb(r, g, b, W, H)
    _, cb4, cr4 = SM.samples_from_rgb(r, g, b, W, H)
    n = cb4[:, 0::2].shape[1]
    assert np.array_equal(cb2[:, :n], cb4[:, 0::2]) and np.array_equal(cr2[:, :n], cr4[:, 0::2])


def test_point_chroma_on_even_rows_is_the_420_point_sample(oracle):
    W, H = 32, 16
    r, g, b = oracle.synth_rgb(W, H, frame=3)
    _, cb2, cr2 = S2.samples_from_rgb(r, g, b, W, H)
    d420 = QM.dct_from_rgb(r, g, b, W, H)
    for k, c in ((4, cb2), (5, cr2)):
        assert np.array_equal(d420[0, :, k], QM.fdct_blocks(S2._blocks(c[0::2], 1, 2)[0]))


def test_average_of_a_flat_picture_is_the_flat_value():
    for v in (-128, -1, 0, 1, 127):
        assert np.array_equal(S2.h2v1_average(np.full((3, 16), v, np.int32)), np.full((3, 8), v, np.int32))


def test_average_is_libjpegs_rule_moved_by_128():
    rng = np.random.default_rng(422)
    c = rng.integers(-128, 128, (64, 32)).astype(np.int32)
    u = c + 128                                           # libjpeg's h2v1_downsample: unsigned samples, bias 0, 1, 0, 1, ..., >> 1
    bias = np.arange(16) & 1
    assert np.array_equal(S2.h2v1_average(c), ((u[:, 0::2] + u[:, 1::2] + bias) >> 1) - 128)


# ---- the host writer ----
@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("W,H", list(itertools.product(WIDTHS, HEIGHTS)))
def test_host_writer_bytes_and_read_back(J, oracle, fields, W, H, optimize):
    for name in TABLES:
        co, qt = fields[W, H, name], QM.tables(name)
        for ri in _restarts(W, H):
            jpg = J.write_jpeg(co, W, H, sampling=J.SAMPLING_422, quant_tables=qt, restart_interval=ri, optimize=optimize)
            assert jpg == S2.write_jpeg(co, W, H, quant_tables=qt, ri=ri, optimize=optimize), (name, ri)
            assert len(jpg) <= J.jpeg_bound(W, H, J.SAMPLING_422)
        info, back = J.read_jpeg(jpg)
        assert (info.width, info.height, info.ncomp) == (W, H, 3)
        assert list(info.H)[:3] == [2, 1, 1] and list(info.V)[:3] == [1, 1, 1] and info.blocks_per_mcu == 4
        assert (info.mcu_cols, info.mcu_rows) == S2.geometry(W, H)[:2]
        assert np.array_equal(np.asarray(back).reshape(co.shape), co)
        assert np.array_equal(np.asarray(info.qt[0][:64]), qt[0]) and np.array_equal(np.asarray(info.qt[1][:64]), qt[1])
        oinfo, oco = oracle.read_jpeg(jpg)                # the independent any-layout decoder reads the same coefficients and decodes them
        assert np.array_equal(oco.reshape(co.shape), co)
        _, pr, pg, pb = oracle.decode_jpeg(jpg)
        assert pr.size == pg.size == pb.size == W * H


def test_pil_opens_a_422_file(J, fields):
    Image = pytest.importorskip("PIL.Image")
    import io
    jpg = J.write_jpeg(fields[33, 17, "q50"], 33, 17, sampling=J.SAMPLING_422, quant_tables=QM.tables("q50"), restart_interval=5, optimize=True)
    im = Image.open(io.BytesIO(jpg))
    im.load()
    assert im.size == (33, 17) and im.mode == "RGB"


def worst_field(W, H):
    """tests/test_jpeg_bound.py's field for 4-block MCUs: every DC difference of category 11, every AC +1023"""
    mc, mr, _ = S2.geometry(W, H)
    co = np.full((mc * mr, 4, 64), 1023, np.int16)
    co[:, :, 0] = np.where(np.arange(mc * mr) % 2 == 0, 1023, -1023).astype(np.int16)[:, None]
    co[:, 1, 0] *= -1                                     # the second luma block predicts from the first: alternate inside the MCU too
    return co


@pytest.mark.parametrize("ri", [0, 1])
@pytest.mark.parametrize("W,H", [(1, 1), (16, 8), (17, 9), (65535, 1), (33, 17)])
def test_bound_holds_for_worst_fields(J, W, H, ri):
    comment = bytes((0x41 + i % 26) for i in range(MAX_COMMENT - (6 if ri else 0)))
    bound = J.jpeg_bound(W, H, J.SAMPLING_422)
    nmcu = S2.geometry(W, H)[0] * S2.geometry(W, H)[1]
    assert bound == 1024 + 1792 * nmcu
    # analytic: the longest header, 1661 bits per block, every byte stuffed, per interval pad + stuffed pad + marker, EOI
    assert 623 + MAX_COMMENT + 5 + 2 * ((nmcu * 4 * 1661 + 7) // 8) + 4 * nmcu + 2 <= bound
    for sign in (1, -1):
        co = worst_field(W, H)
        co[:, :, 1:] *= sign
        jpg = J.write_jpeg(co, W, H, sampling=J.SAMPLING_422, comment=comment, restart_interval=ri)
        assert len(jpg) <= bound, (W, H, ri, sign, len(jpg), bound)
        if nmcu <= 15:
            assert jpg == S2.write_jpeg(co, W, H, comment=comment, ri=ri)


@pytest.mark.parametrize("ri", [0, 5])
def test_symbol_histogram_matches_model(J, fields, ri):
    co = fields[33, 17, "q50"]
    want, ok = S2.symbol_counts(co, ri)
    assert ok
    got = J.huffman_histogram(co, 33, 17, sampling=J.SAMPLING_422, restart_interval=ri)
    assert np.array_equal(got.astype(np.int64), want)
    bad = np.array(co).copy()
    bad[0, 0, 1, 5] = 2000
    with pytest.raises(J.JpezyError, match="status -5"):
        J.huffman_histogram(bad, 33, 17, sampling=J.SAMPLING_422)


def test_geometry_helpers(J):
    assert J.SAMPLING_422 == 3
    for W, H in itertools.product([1, 7, 8, 9, 15, 16, 17, 65535], repeat=2):
        mc, mr = (W + 15) // 16, (H + 7) // 8
        assert J.sampling_geometry(J.SAMPLING_422, W, H) == (mc, mr, 4) == S2.geometry(W, H)
        assert J.coeff_count(W, H, sampling=J.SAMPLING_422) == 256 * mc * mr
        assert J.jpeg_bound(W, H, J.SAMPLING_422) == 1024 + 1792 * mc * mr
    lib = J.load_library()
    for bad in (-1, 2, 444):
        assert lib.jpezy_sampling_geometry(bad, 8, 8, None, None, None) == BADARG
        assert b"JPEZY_SAMPLING_422 = 3" in lib.jpezy_hip_last_error()
        assert lib.jpezy_coeff_count_sampling(8, 8, bad) == 0 and lib.jpezy_jpeg_bound_sampling(8, 8, bad) == 0
        with pytest.raises(J.JpezyError, match="status -1"):
            J.sampling_geometry(bad, 8, 8)
    for W, H in ((0, 8), (8, 0), (65536, 8)):
        assert lib.jpezy_sampling_geometry(3, W, H, None, None, None) == BADARG
        assert lib.jpezy_coeff_count_sampling(W, H, 3) == 0 and lib.jpezy_jpeg_bound_sampling(W, H, 3) == 0


def test_abi_refusals(J):
    lib = J.load_library()
    W, H = 33, 17
    rng = np.random.default_rng(7)
    co = rng.integers(-40, 41, J.coeff_count(W, H, sampling=J.SAMPLING_422)).astype(np.int16)
    cap = J.jpeg_bound(W, H, J.SAMPLING_422)
    buf = np.zeros(cap, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    err = lambda: lib.jpezy_hip_last_error().decode()
    assert lib.jpezy_write_jpeg_sampling(p(co), W, H, 3, 1, b"x", None, None, 0, 0, p(buf), cap) == BADARG
    assert "gray is not available with JPEZY_SAMPLING_422" in err()
    with pytest.raises(J.JpezyError, match="status -1"):
        J.write_jpeg(co, W, H, gray=True, sampling=J.SAMPLING_422)
    with pytest.raises(J.JpezyError, match="gray"):
        J.coeff_count(W, H, gray=True, sampling=J.SAMPLING_422)
    t = np.full(64, 3, np.uint8)
    assert lib.jpezy_write_jpeg_sampling(p(co), W, H, 3, 0, b"x", p(t), None, 0, 0, p(buf), cap) == BADARG
    assert "one of the two tables is null" in err()
    z = t.copy(); z[9] = 0
    assert lib.jpezy_write_jpeg_sampling(p(co), W, H, 3, 0, b"x", p(t), p(z), 0, 0, p(buf), cap) == BADARG
    assert "table entry is zero" in err()
    # too small a buffer: JPEZY_E_NOSPACE, never a partial file reported as one
    assert lib.jpezy_write_jpeg_sampling(p(co), W, H, 3, 0, b"x", None, None, 0, 0, p(buf), 700) == NOSPACE
    assert "output buffer too small" in err()
    bad = co.copy(); bad[64 * 2 + 5] = 2000
    assert lib.jpezy_write_jpeg_sampling(p(bad), W, H, 3, 0, b"x", None, None, 0, 0, p(buf), cap) == FORMAT
    assert "outside" in err()
    with pytest.raises(J.JpezyError, match="does not match"):
        J.write_jpeg(co[:-64], W, H, sampling=J.SAMPLING_422)
    # the lossless transforms keep their own two-value check
    ints = [C.c_int() for _ in range(4)]
    assert lib.jpezy_transform_geometry(5, 0, 32, 16, 3, *(C.byref(x) for x in ints)) == BADARG
    assert "sampling" in err()
