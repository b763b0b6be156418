"""Lossless transforms, the part that needs no GPU: the model (tests/transform_model.py) against the float64 DCT of the transformed
pixels, the group laws on the model, and the two pure host functions jpezy_transform_geometry / jpezy_quant_tables_transform against the
model.  tests/test_gpu_transform.py checks the kernel and the files against the same model."""
import ctypes as C

import numpy as np
import pytest

import transform_model as M

SIZES = [(1, 1), (8, 8), (16, 16), (17, 33), (40, 24), (65535, 65535)]


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.mark.parametrize("op", range(8))
def test_block_rule_is_the_dct_of_the_pixel_operation(op):
    rng = np.random.default_rng(100 + op)
    D = M.dct_matrix()
    assert np.abs(D @ D.T - np.eye(8)).max() < 1e-14
    worst = 0.0
    for _ in range(20):
        X = rng.uniform(-128, 128, (8, 8))
        want = D @ M.pixel_op(X, op) @ D.T
        got = M.block_rule(D @ X @ D.T, op)
        worst = max(worst, np.abs(got - want).max())
    assert worst < 1e-9, worst


def test_pixel_op_matches_numpy():
    img = np.arange(5 * 7 * 3).reshape(5, 7, 3)
    want = [img, img[:, ::-1], img[::-1], img.transpose(1, 0, 2), img[::-1, ::-1].transpose(1, 0, 2), np.rot90(img, -1), img[::-1, ::-1],
            np.rot90(img, 1)]
    for op in range(8):
        assert np.array_equal(M.pixel_op(img, op), want[op]), op


def _random_field(rng, W, H, sampling):
    m = M.mcu_px(sampling)
    n = (-(-W // m)) * (-(-H // m))
    return rng.integers(-32768, 32768, (n, 3 if sampling == M.S444 else 6, 64), dtype=np.int64).astype(np.int16)


def _chain(co, W, H, sampling, ops):
    for op in ops:
        co, W, H = M.transform_field(co, W, H, sampling, op)
    return co, W, H


@pytest.mark.parametrize("sampling,size", [(M.S420, (48, 32)), (M.S420, (16, 80)), (M.S444, (40, 24)), (M.S444, (8, 8))])
def test_group_laws_on_the_model(sampling, size):
    rng = np.random.default_rng(7)
    W, H = size
    co = _random_field(rng, W, H, sampling)
    co[0, 0, 5] = -32768
    same = lambda a, b: a[1:] == b[1:] and np.array_equal(a[0], b[0])
    none = _chain(co, W, H, sampling, [M.NONE])
    assert np.array_equal(none[0], co) and none[1:] == (W, H)
    assert same(_chain(co, W, H, sampling, [M.HFLIP, M.HFLIP]), none)
    assert same(_chain(co, W, H, sampling, [M.ROT90] * 4), none)
    assert same(_chain(co, W, H, sampling, [M.ROT90]), _chain(co, W, H, sampling, [M.TRANSPOSE, M.HFLIP]))
    assert same(_chain(co, W, H, sampling, [M.TRANSVERSE]), _chain(co, W, H, sampling, [M.TRANSPOSE, M.ROT180]))
    assert same(_chain(co, W, H, sampling, [M.ROT90, M.ROT270]), none)
    assert not same(_chain(co, W, H, sampling, [M.ROT90]), _chain(co, W, H, sampling, [M.ROT270]))


def test_model_trims_and_keeps_the_source_pitch():
    """40 x 24 at 4:2:0 is 3 x 2 MCUs; HFLIP with trim uses the first two columns (32 pixels) of both rows (the height is not mirrored and
    keeps its partial MCU), read at the source's pitch of three"""
    rng = np.random.default_rng(3)
    co = _random_field(rng, 40, 24, M.S420)
    out, Wo, Ho = M.transform_field(co, 40, 24, M.S420, M.HFLIP, trim=True)
    assert (Wo, Ho) == (32, 24) and out.shape == (4, 6, 64)
    src = co.reshape(2, 3, 6, 64)
    # MCU (0, 0) of the output is MCU (1, 0) of the source with its luma columns exchanged; chroma block in place
    assert np.array_equal(np.abs(out.reshape(2, 2, 6, 64)[0, 0, 0].astype(int)), np.abs(src[0, 1, 1].astype(int)))
    assert np.array_equal(np.abs(out.reshape(2, 2, 6, 64)[1, 1, 4].astype(int)), np.abs(src[1, 0, 4].astype(int)))
    assert out.reshape(2, 2, 6, 64)[0, 0, 1, 0] == src[0, 1, 0, 0]                              # the DC keeps its sign


@pytest.mark.parametrize("size", SIZES)
def test_geometry_agrees_with_the_model(J, size):
    lib = J.load_library()
    W, H = size
    for sampling in (M.S420, M.S444):
        m = M.mcu_px(sampling)
        for op in range(8):
            for trim in (False, True):
                v = [C.c_int(-7) for _ in range(4)]
                rc = lib.jpezy_transform_geometry(op, 1 if trim else 0, W, H, sampling, *(C.byref(x) for x in v))
                msg = lib.jpezy_hip_last_error().decode()
                try:
                    want = M.geometry(op, W, H, sampling, trim)
                except M.Refused as e:
                    assert rc == e.status, (size, sampling, op, trim, rc)
                    assert e.axis in msg and str(m) in msg, msg                      # the axis and the multiple are named
                    assert all(x.value == -7 for x in v)
                    with pytest.raises(J.JpezyError, match=e.axis):
                        J.transform_geometry(op, W, H, sampling, trim)
                    continue
                assert rc == 0, (size, sampling, op, trim, msg)
                assert tuple(x.value for x in v) == want == J.transform_geometry(op, W, H, sampling, trim)
                assert lib.jpezy_transform_geometry(op, 1 if trim else 0, W, H, sampling, None, None, None, None) == 0   # any pointer may be NULL


def test_geometry_refusals_by_hand(J):
    """the cases the table above implies, spelled out: 40 x 24 at 4:2:0 has a partial MCU on both axes, at 4:4:4 on none"""
    lib = J.load_library()
    g = lambda op, flags, W, H, s: lib.jpezy_transform_geometry(op, flags, W, H, s, None, None, None, None)
    for op in (M.HFLIP, M.VFLIP, M.TRANSVERSE, M.ROT90, M.ROT180, M.ROT270):
        assert g(op, 0, 40, 24, M.S420) == M.E_UNSUPPORTED, op
        assert g(op, 1, 40, 24, M.S420) == 0 and g(op, 0, 40, 24, M.S444) == 0, op
    assert g(M.TRANSPOSE, 0, 40, 24, M.S420) == 0 and g(M.NONE, 0, 17, 33, M.S420) == 0        # TRANSPOSE never needs trimming
    assert J.transform_geometry(M.TRANSPOSE, 40, 24) == (24, 40, 3, 2)
    assert J.transform_geometry(M.ROT90, 40, 24, trim=True) == (16, 40, 3, 1)                  # H is mirrored: 24 -> 16; W keeps its partial MCU
    assert J.transform_geometry(M.ROT270, 40, 24, trim=True) == (24, 32, 2, 2)
    assert J.transform_geometry(M.ROT180, 17, 33, M.S444, trim=True) == (16, 32, 2, 4)
    # nothing left: BADARG, only with trim; without it the same size is UNSUPPORTED
    assert g(M.HFLIP, 1, 15, 64, M.S420) == M.E_BADARG and "width" in lib.jpezy_hip_last_error().decode()
    assert g(M.VFLIP, 1, 64, 7, M.S444) == M.E_BADARG and "height" in lib.jpezy_hip_last_error().decode()
    assert g(M.HFLIP, 0, 15, 64, M.S420) == M.E_UNSUPPORTED
    assert g(M.VFLIP, 1, 15, 64, M.S420) == 0                                                   # the width is not mirrored


def test_quant_tables_agree_with_the_model(J):
    lib = J.load_library()
    rng = np.random.default_rng(11)
    luma, chroma = J.quality_tables(50)
    assert not np.array_equal(luma.reshape(8, 8), luma.reshape(8, 8).T)                         # Annex K is not symmetric: it matters
    for table in (luma, chroma, rng.integers(1, 256, 64).astype(np.uint8)):
        for op in range(8):
            want = M.quant_table(op, table)
            assert np.array_equal(J.quant_tables_transform(op, table), want), op
            assert np.array_equal(want, table) == (not M.OPS[op][0] or np.array_equal(table.reshape(8, 8), table.reshape(8, 8).T))
            buf = table.copy()                                                                  # in place
            assert lib.jpezy_quant_tables_transform(op, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)) == 0
            assert np.array_equal(buf, want)
