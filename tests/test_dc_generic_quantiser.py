"""The one-quad encode kernel sends the DC through the level-1 quantiser like any coefficient (f32::quant_block_column, DCG):
on the j == 0 lane the column pass leaves the block's integer sample sum in F[0].x (exact in FP32), the quantiser forms
t' = fma(sum, ks, delta1) and q = (int)t', and flags the coefficient when fract(t') < 2 delta1; a flagged DC is settled in
place by f32::dc_formula.  This test evaluates exactly those FP32 operations in numpy (as tests/test_f32_error_bound.py does)
for every sum in [-8192, 8192] and both DC quantisers and compares with DeviceTables::dcq, int(((S * s) * s) / 4) / Q in
binary64 with C's truncating division.  (jpezy_ctx_create repeats the check against the device table and keeps the table
lookup if it ever fails.)"""
import numpy as np

f32 = np.float32


def fma(a, b, c):
    # float32 fused multiply-add: the product of two float32 is exact in float64; one rounding
    return (np.asarray(a, f32).astype(np.float64) * np.float64(b) + np.asarray(c, f32).astype(np.float64)).astype(f32)


def dc_formula(S, Q):
    """f32::dc_formula: sign(S) * (((|S| - 1) >> 3) / Q) in the kernel's FP32 operations"""
    a = np.abs(S).astype(f32)
    d = np.trunc(fma(a, f32(0.125), np.full(a.shape, -0.125, f32)))
    rq, bias = f32(1.0) / f32(Q), f32(0.5) / f32(Q)
    u = fma(d, rq, np.full(a.shape, bias, f32))
    return np.copysign(np.trunc(u), S).astype(np.int64)


def column0_delta1(c, qt):
    """DeviceTables::f32col[t][0].delta1 as jpezy_ctx_create builds it: 1.25 x the worst level-1 bound over the column's
    coefficients, the DC left out (it has no transform error)"""
    cos = c["cos"].reshape(8, 8)
    s = c["inv_sqrt2"]
    cu = np.where(np.arange(8) == 0, s, 1.0)
    absum = np.abs(cos).sum(axis=1)
    amp = 128.0 * np.outer(absum, absum) * np.outer(cu, cu) / (4.0 * qt.reshape(8, 8))
    bound = 13 * 2.0 ** -24 * amp + 2.0 ** -23 * amp
    bound[0, 0] = 0
    return f32(1.25 * bound[:, 0].max())


def test_dc_through_the_generic_quantiser_reproduces_the_exact_table(oracle):
    c = oracle.constants()
    s = c["inv_sqrt2"]
    S = np.arange(-8192, 8193)
    for qt in (c["qt_luma"], c["qt_chroma"]):
        Q = int(qt[0])
        dct = np.trunc(((S * s) * s) / 4).astype(np.int64)
        want = np.sign(dct) * (np.abs(dct) // Q)                       # DeviceTables::dcq
        ks = f32(s * s / (4.0 * Q))                                    # F32Column::ks of coefficient (0, 0)
        delta1 = column0_delta1(c, qt)
        th = delta1 + delta1
        tp = fma(S.astype(f32), ks, np.full(S.shape, delta1, f32))     # t' = fma(sum, ks, delta1)
        fr = (tp - np.floor(tp)).astype(f32)                           # v_fract_f32
        flagged = fr < th
        got = np.where(flagged, dc_formula(S, Q), np.trunc(tp).astype(np.int64))
        assert np.array_equal(got, want), Q
        # the guard test flags the sums 8 Q m and nothing else: t = sum / (8 Q) is a multiple of 1 / (8 Q) >= 1e-3, the FP32
        # error of t' is below 1e-5 and delta1 about 1e-4
        assert np.array_equal(flagged, S % (8 * Q) == 0), Q
        assert 8 * float(delta1) < 1.0 / (8 * Q)
        err = np.abs(tp.astype(np.float64) - float(delta1) - S / (8.0 * Q)).max()
        assert err < 1e-5 < float(delta1) / 4, (err, delta1)
        # on a flagged sum other than zero (int)t' is off by one on one side of zero -- which side depends on the constants;
        # the kernel must not rely on it, the closed form gives sign(sum) * (|m| - 1)
        m = S[flagged] // (8 * Q)
        assert np.array_equal(want[flagged], np.sign(m) * (np.abs(m) - 1))
        assert np.any(np.trunc(tp[flagged]).astype(np.int64) != want[flagged])
