"""The bit-length model that builds the seam fields of tests/test_gpu_entropy_seams.py must agree with the host writer before it
is trusted to place anything: same unstuffed stream (hence the same block lengths and 0xFF positions) on random fields."""
import numpy as np
import pytest

import entropy_model as M


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _random_field(rng, nmcu, bpm):
    co = np.zeros((nmcu, bpm, 64), np.int16)
    for m in range(nmcu):
        for b in range(bpm):
            kind = rng.integers(0, 5)
            if kind == 0:
                co[m, b, 0] = rng.integers(-1023, 1024)
            elif kind == 1:
                co[m, b] = rng.integers(-1023, 1024, 64)
            elif kind == 2:
                pos = rng.integers(1, 64, 4)
                co[m, b, pos] = rng.integers(-300, 301, 4)
            elif kind == 3:
                co[m, b, 0] = rng.integers(-50, 51)
                co[m, b, 63] = rng.integers(1, 1024)            # ZRL chain, no EOB
            else:
                co[m, b] = rng.integers(-2, 3, 64)
    return co


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("seed", range(4))
def test_model_equals_host_writer(J, seed, gray):
    rng = np.random.default_rng(100 + seed)
    W, H = 48, 32
    co = _random_field(rng, 6, 4 if gray else 6)
    jpg = J.write_jpeg(co, W, H, gray=gray, comment=b"")
    scan = M.scan_of(jpg)
    assert M.unstuffed_stream(co, gray) == scan
    bits = int(M.block_lengths(co, gray).sum())
    assert (bits + 7) // 8 == len(scan)
    assert np.array_equal(M.ff_positions(scan), M.ff_positions(M.unstuffed_stream(co, gray)))


def test_builders_hit_their_lengths(J):
    for t in (0, 1):
        for target in (1112, 1113, 1119, 1120):
            z = M.block_of_bits(target, t=t)
            assert z is not None and M.block_bits(z, 0, t) == target
            assert M.fits_row(z, 0, t), (t, target)           # coded in the LDS row
        z = M.block_of_bits(1121, t=t)
        assert M.block_bits(z, 0, t) == 1121 and not M.fits_row(z, 0, t)
    for n, s in M._short_lengths(0).items():
        assert M.block_bits(M.ac_block(s), 0, 0) == n
    # the densest block overtakes its reads at once: always re-coded
    assert not M.fits_row(M.dense_block(), 0, 0)
    # a row that ends exactly at the 35th word fits, one bit more does not
    co = np.stack([M.block_of_bits(1120), M.block_of_bits(1121)] + [np.zeros(64, np.int16)] * 4)[None]
    jpg = J.write_jpeg(co, 16, 16, comment=b"")
    assert M.unstuffed_stream(co) == M.scan_of(jpg)
