"""Encode variant 1 sends the DC through the level-1 quantiser; a DC whose block sum is a multiple of 8 Q sits exactly on a
truncation boundary, is flagged by the guard test and settled by the closed form inside the candidate branch, without a queue
entry and without being counted as an exact fallback.  Random pixels put 0.6 % of the blocks there; these frames put every
block there: flat MCUs of every level (luma sums 64 Y, chroma sums 64 C: multiples of 128 / 136 for every even Y and every C
that is a multiple of 17, both signs, zero included) and noise whose luma block sums are forced onto multiples of 128."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module", params=[0, 1], ids=["enc-f64", "enc-f32"])
def ctx(J, request):
    c = J.Context(0)
    c.set_variant(request.param)
    c.variant = request.param
    yield c
    c.close()


def ref_luma(v):
    """the reference's luma sample of a gray pixel (r = g = b = v), its FP64 expression term for term"""
    v = np.asarray(v, np.float64)
    return np.trunc((0.2990 * v) + (0.5870 * v) + (0.1140 * v) - 128.0).astype(np.int64)


def flat_mcus():
    """256 x 256 pixels: MCU (my, mx) is flat at level 16 my + mx"""
    lvl = (16 * np.arange(16)[:, None] + np.arange(16)[None, :]).astype(np.uint8)
    return np.kron(lvl, np.ones((16, 16), np.uint8))


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("channels", ["equal", "distinct"])
def test_flat_mcus_of_every_level(J, ctx, oracle, gray, channels):
    W = H = 256
    a = flat_mcus()
    if channels == "equal":
        r = g = b = a.reshape(-1)
    else:
        r, g, b = a.reshape(-1), (255 - a).reshape(-1), ((a.astype(np.int64) * 7) % 256).astype(np.uint8).reshape(-1)
    want = oracle.encode_coeffs(r, g, b, W, H, gray)
    ctx.fallback_count()
    got = ctx.fdct_quant(r, g, b, W, H, gray=gray)
    assert np.array_equal(got, want)
    # a flat block's AC coefficients are exact zeros in every precision: nothing is near a non-zero integer, nothing is resolved,
    # and a boundary DC is not a fallback
    if ctx.variant == 1:
        assert ctx.fallback_count() == 0


@pytest.mark.parametrize("gray", [False, True])
def test_noise_with_every_luma_sum_on_a_boundary(J, ctx, oracle, gray):
    W, H = 512, 256
    rng = np.random.default_rng(20)
    img = rng.integers(0, 256, (H, W)).astype(np.int64)
    yt = ref_luma(np.arange(256))
    for by in range(H // 8):
        for bx in range(W // 8):
            blk = img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].reshape(-1).copy()
            rest = int(yt[blk].sum() % 128)            # lower single pixels by one luma step until the sum is a multiple of 8 Q
            k = 0
            while rest:
                v = blk[k % 64]
                if v > 0 and yt[v] - yt[v - 1] == 1:
                    blk[k % 64] = v - 1
                    rest -= 1
                k += 1
            img[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = blk.reshape(8, 8)
    sums = yt[img].reshape(H // 8, 8, W // 8, 8).sum(axis=(1, 3))
    assert np.all(sums % 128 == 0) and np.any(sums > 0) and np.any(sums < 0)
    p = img.astype(np.uint8).reshape(-1)
    want = oracle.encode_coeffs(p, p, p, W, H, gray)
    got = ctx.fdct_quant(p, p, p, W, H, gray=gray)
    assert np.array_equal(got, want)
