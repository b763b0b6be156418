"""Per-image optimised Huffman tables on the GPU: the symbol histogram kernel against the Python count (tests/huffopt_model.py),
the optimising context against the host's optimising writer byte for byte, end to end through the oracle's reader and the
context's own decoder, and the setting switched off again."""
import hashlib
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

import huffopt_model as HM

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
FIXTURES = ["rand64", "rand17x33", "gradient52x40", "rand16", "greyramp256x16", "flatgrey256"]


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def octx(J):
    c = J.Context(0)
    c.set_huffman_optimize(1)
    yield c
    c.close()


def _dev(co):
    import torch
    return torch.from_numpy(np.ascontiguousarray(co, dtype=np.int16)).cuda()


def _grid(W, H):
    return (W + 15) // 16, (H + 15) // 16


def _random_field(W, H, seed):
    """small values with zero runs, a few large ones, DCs that wander"""
    mc, mr = _grid(W, H)
    rng = np.random.default_rng(seed)
    co = rng.integers(-6, 7, (mr, mc, 6, 64)).astype(np.int16)
    co[..., 8:] *= (rng.random((mr, mc, 6, 56)) < 0.3)
    co[..., 0] = rng.integers(-900, 900, (mr, mc, 6))
    flat = co.reshape(-1, 64)
    flat[::7, 63] = 1000                                   # blocks without EOB
    flat[3::11, 1:] = 0
    flat[3::11, 40] = -300                                 # run 39: two ZRLs
    return co


def _wide_field(gray):
    """the field of test_gpu_entropy.test_narrow_and_wide_tiles_in_one_launch: 48 tiles, ZRL chains, size-10 values"""
    bpm = 4 if gray else 6
    rng = np.random.default_rng(606 + gray)
    co = rng.integers(-3, 4, (32, 64, bpm, 64)).astype(np.int16)
    co[..., 20:] *= (rng.random((32, 64, bpm, 44)) < 0.2)
    flat = co.reshape(-1, 64)
    nb = flat.shape[0]
    per_tile = 256 * bpm // 6 if gray else 256
    for t, (where, pos, val) in enumerate([(0, 0, 128), (per_tile - 1, 63, -129), (5, 17, 1023), (100, 1, -1023), (7, 0, -128), (9, 5, 127)]):
        flat[(3 * t + 1) * per_tile + where, pos] = val
    dense = rng.integers(-127, 128, (40, 64)).astype(np.int16)
    dense[dense == 0] = 99
    flat[20 * per_tile + 30: 20 * per_tile + 70] = dense
    flat[nb - 1, 63] = -128
    return co


def _batch_frames():
    """three frames of 208 x 120 with different content: flat, noise, gradient"""
    mc, mr = _grid(208, 120)
    rng = np.random.default_rng(208120)
    flat = np.zeros((mr, mc, 6, 64), np.int16)
    flat[..., 0] = 37
    noise = rng.integers(-200, 201, (mr, mc, 6, 64)).astype(np.int16)
    grad = np.zeros((mr, mc, 6, 64), np.int16)
    grad[..., 0] = (np.arange(mr * mc * 6).reshape(mr, mc, 6) % 90) * 5 - 200
    grad[..., 1] = 3
    grad[..., 2] = -1
    return np.stack([flat, noise, grad])


@lru_cache(maxsize=None)
def _case(name, gray):
    """(coefficients [frames, ...], W, H, frames) of a named case, built once per session"""
    if name in FIXTURES:
        z = np.load(GOLDEN / f"{name}.npz")
        return (z["coeffs_gray"] if gray else z["coeffs"])[None], int(z["W"]), int(z["H"]), 1
    if name == "wide1024x512":
        return _wide_field(gray)[None], 1024, 512, 1
    if name == "batch3":
        co, W, H = _batch_frames(), 208, 120
    else:
        W, H = {"r112": (112, 112), "r17": (17, 17)}[name]
        co = _random_field(W, H, W)[None]
    return (np.ascontiguousarray(co[:, :, :, :4]) if gray else co), W, H, co.shape[0]


@lru_cache(maxsize=None)
def _counts(name, gray):
    co, W, H, n = _case(name, gray)
    count = HM.symbol_counts_np if name == "wide1024x512" else HM.symbol_counts
    out = [count(co[f], gray) for f in range(n)]
    assert all(ok for _, ok in out)
    return np.stack([h for h, _ in out])


SHAPES = FIXTURES + ["r112", "r17", "wide1024x512", "batch3"]


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("name", SHAPES)
def test_histogram_kernel_equals_python_count(J, ctx, name, gray):
    import torch
    co, W, H, n = _case(name, gray)
    if name == "r112":
        assert _grid(W, H)[0] * _grid(W, H)[1] * 6 == 294          # a tile border inside an MCU
    hist = torch.full((n, 4, 256), -1, dtype=torch.int64, device="cuda")
    ctx.huffman_histogram_dev(_dev(co), W, H, hist, gray=gray, n_frames=n)
    torch.cuda.synchronize()
    got, want = hist.cpu().numpy(), _counts(name, gray)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    if name == "batch3":
        assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[1], want[2])


def test_histogram_counts_out_of_range_values_as_the_clamped_symbol(J, ctx):
    import torch
    co = _random_field(48, 32, 9)
    co[0, 1, 2, 5] = 1024
    co[1, 2, 4, 9] = -20000
    co[1, 0, 0, 0] = 32000
    co[1, 0, 1, 0] = -32000
    want, ok = HM.symbol_counts(co)
    assert not ok
    hist = torch.zeros((1, 4, 256), dtype=torch.int64, device="cuda")
    ctx.huffman_histogram_dev(_dev(co), 48, 32, hist)
    torch.cuda.synchronize()
    assert np.array_equal(hist.cpu().numpy()[0], want)


@pytest.mark.parametrize("gray", [False, True])
@pytest.mark.parametrize("name", SHAPES)
def test_optimizing_context_equals_host_writer(J, octx, name, gray):
    co, W, H, n = _case(name, gray)
    got = octx.write_jpeg_gpu(_dev(co), W, H, gray=gray, n_frames=n)
    want = [J.write_jpeg(co[f], W, H, gray, optimize=True) for f in range(n)]
    for f in range(n):
        assert got[f] == want[f], (name, gray, f)
        assert len(got[f]) < len(J.write_jpeg(co[f], W, H, gray))
    if name == "batch3":
        hdr = [g[:g.index(b"\xff\xda")] for g in got]
        assert len({bytes(h) for h in hdr}) == 3


def _fib19_field():
    """160 x 128, zero chroma: the luma AC symbol counts are 1, 2, 3, 5, ... over 19 symbols (17,709 symbols): EOB, run 0 with
    sizes 1..10, run 1 with sizes 1..8"""
    fib = HM.fibonacci_counts(19)
    rng = np.random.default_rng(19)
    eob = fib[11]                                                   # 233 blocks end in zeros
    run1 = dict(zip(range(1, 9), fib[:8]))
    run0 = dict(zip(range(1, 11), fib[8:11] + fib[12:]))
    one = [s for s, n in run0.items() for _ in range(n)]
    two = [s for s, n in run1.items() for _ in range(n)]
    rng.shuffle(one)
    rng.shuffle(two)
    mc, mr = _grid(160, 128)
    co = np.zeros((mr, mc, 6, 64), np.int16)
    luma = co[:, :, :4].reshape(-1, 64).copy()
    nfull = luma.shape[0] - eob                                     # blocks filled up to position 63: no EOB

    def value(s):
        return int(rng.integers(1 << (s - 1), 1 << s)) * int(rng.choice([-1, 1]))
    for k in range(luma.shape[0]):
        pos = 1
        if k < nfull:
            for _ in range(len(two) // (nfull - k)):                # the run-1 symbols, spread over the full blocks
                luma[k, pos + 1] = value(two.pop())
                pos += 2
        while pos <= (63 if k < nfull else 62) and one:             # a block that ends before position 63 codes an EOB
            luma[k, pos] = value(one.pop())
            pos += 1
        assert k >= nfull or pos == 64
    assert not one and not two
    luma[:, 0] = rng.integers(-100, 100, luma.shape[0])
    co[:, :, :4] = luma.reshape(mr, mc, 4, 64)
    return co


def test_length_limited_codes_through_the_device_coder(J, octx):
    co = _fib19_field()
    hist, ok = HM.symbol_counts(co)
    assert ok and sorted(int(c) for c in hist[2] if c) == HM.fibonacci_counts(19)
    bits, vals, depth = HM.optimal_table(hist[2])
    assert depth > 16 and max(HM.lengths(bits)) == 16                # Figure K.3 was needed: 16-bit codes are in use
    want = J.write_jpeg(co, 160, 128, optimize=True)
    assert octx.write_jpeg_gpu(_dev(co), 160, 128)[0] == want
    assert want == HM.write_jpeg(co, False, J.write_jpeg(co, 160, 128))


def test_byte_stuffing_heavy_stream(J, octx):
    co = np.zeros((4, 4, 6, 64), np.int16)
    co[..., 0] = -1023
    co[..., 1:] = 1023
    jpg = octx.write_jpeg_gpu(_dev(co), 64, 64)[0]
    assert jpg == J.write_jpeg(co, 64, 64, optimize=True)
    assert b"\xff\x00" in jpg[jpg.index(b"\xff\xda") + 14:-2]


def test_flat_frame_of_more_than_2048_tiles(J, octx):
    """With one-bit codes a flat block is 2 bits and a tile 512: a 16 KB piece of the stream touches up to 258 tiles, more than the
    window assemble_kernel<false> loads for Annex-K tables.  4736 x 4736 is the smallest frame on that path."""
    W = H = 4736
    mc, mr = J.mcu_grid(W, H)
    assert -(-mc * mr * 6 // 256) > 2048
    rng = np.random.default_rng(W)
    for variant in range(2):
        co = np.zeros((mr, mc, 6, 64), np.int16)
        if variant == 1:
            co[0, 0, :, 0] = (-700, 3, 90, -5, 200, -200)
            co[0, 0, :, 1:] = rng.integers(-30, 31, (6, 63))
        for gray in (False, True):
            c = np.ascontiguousarray(co[:, :, :4]) if gray else co
            want = J.write_jpeg(c, W, H, gray, optimize=True)
            got = octx.write_jpeg_gpu(_dev(c), W, H, gray=gray)[0]
            assert len(got) == len(want) and hashlib.sha256(got).digest() == hashlib.sha256(want).digest(), (variant, gray)


@pytest.mark.parametrize("size", [(52, 40), (208, 120)])
def test_end_to_end(J, ctx, octx, oracle, size):
    W, H = size
    r, g, b = oracle.synth_rgb(W, H, frame=3)
    octx.set_huffdec_min_bytes(0)
    for gray in (False, True):
        co = ctx.fdct_quant(r, g, b, W, H, gray=gray)
        jpg = octx.encode_jpeg(r, g, b, W, H, gray=gray)
        assert jpg == J.write_jpeg(co, W, H, gray, optimize=True)
        packed = np.ascontiguousarray(np.stack([p.reshape(H, W) for p in (r, g, b)], axis=-1))
        assert octx.encode_jpeg_packed(packed, gray=gray) == jpg
        info, back = oracle.read_jpeg(jpg)
        assert np.array_equal(back[:, :, :co.shape[-2]], co) and not back[:, :, co.shape[-2]:].any()
        for dgray in (False, True):
            want = oracle.decode_jpeg(jpg, gray=dgray)
            got = octx.decode_jpeg(jpg, gray=dgray)
            for k in range(1, 4):
                assert np.array_equal(got[k], want[k]), (gray, dgray, k)


def test_own_decoder_reads_single_symbol_tables(J, octx, oracle):
    """the optimised flatgrey256 file: three of its tables hold one symbol, coded in one bit"""
    co, W, H, _ = _case("flatgrey256", False)
    jpg = octx.write_jpeg_gpu(_dev(co), W, H)[0]
    tabs = HM.frame_tables(co[0])
    assert sum(len(v) == 1 for _, v in tabs) == 3
    octx.set_huffdec_min_bytes(0)
    want = oracle.decode_jpeg(jpg)
    got = octx.decode_jpeg(jpg)
    for k in range(1, 4):
        assert np.array_equal(got[k], want[k])
    info, d = octx.read_jpeg_gpu(jpg)
    assert np.array_equal(d.cpu().numpy(), co[0])


def test_setting_off_restores_every_byte(J):
    import torch
    c = J.Context(0)
    try:
        for name in FIXTURES:
            z = np.load(GOLDEN / f"{name}.npz")
            W, H = int(z["W"]), int(z["H"])
            c.set_huffman_optimize(1)
            assert c.write_jpeg_gpu(_dev(z["coeffs"]), W, H)[0] == J.write_jpeg(z["coeffs"], W, H, optimize=True)
            c.set_huffman_optimize(0)
            assert c.write_jpeg_gpu(_dev(z["coeffs"]), W, H)[0] == z["jpg"].tobytes(), name
            assert c.write_jpeg_gpu(_dev(z["coeffs_gray"]), W, H, gray=True)[0] == z["jpg_gray"].tobytes(), name
        # the asynchronous form is refused while the setting is on, and nothing of the refusal stays behind
        z = np.load(GOLDEN / "rand64.npz")
        W, H = int(z["W"]), int(z["H"])
        out = torch.zeros((1, 8192), dtype=torch.uint8, device="cuda")
        sizes = torch.zeros(1, dtype=torch.int64, device="cuda")
        c.set_huffman_optimize(1)
        with pytest.raises(J.JpezyError, match="status -4"):
            c.write_jpeg_gpu_dev(_dev(z["coeffs"]), W, H, out, sizes)
        c.set_huffman_optimize(0)
        c.write_jpeg_gpu_dev(_dev(z["coeffs"]), W, H, out, sizes)
        torch.cuda.synchronize()
        want = z["jpg"].tobytes()
        assert int(sizes[0]) == len(want) and out[0, :len(want)].cpu().numpy().tobytes() == want
        with pytest.raises(J.JpezyError):
            c.set_huffman_optimize(2)
    finally:
        c.close()


def test_out_of_range_coefficient_raises_and_the_context_goes_on(J, octx):
    co = _random_field(48, 32, 11)
    bad = co.copy()
    bad[1, 1, 0, 5] = 1024
    with pytest.raises(J.JpezyError):
        octx.write_jpeg_gpu(_dev(bad), 48, 32)
    bad = co.copy()
    bad[0, 0, 5, 0] = 2048
    with pytest.raises(J.JpezyError):
        octx.write_jpeg_gpu(_dev(bad), 48, 32)
    assert octx.write_jpeg_gpu(_dev(co), 48, 32)[0] == J.write_jpeg(co, 48, 32, optimize=True)
    # in a batch only the bad frame is refused
    lib = J.load_library()
    import ctypes as C
    both = np.stack([bad, co])
    cap = lib.jpezy_jpeg_bound(48, 32)
    buf = np.empty(2 * cap, np.uint8)
    sizes = (C.c_long * 2)()
    d = _dev(both)
    rc = lib.jpezy_write_jpeg_gpu_batch(octx._h, d.data_ptr(), 48, 32, 0, 2, b"Encoded by jpezy", buf.ctypes.data_as(C.c_void_p), cap, sizes)
    assert rc == -5 and sizes[0] == -5
    assert buf[cap:cap + sizes[1]].tobytes() == J.write_jpeg(co, 48, 32, optimize=True)


def test_cli_optimize_flag(J, ctx, oracle, tmp_path):
    """jpezy_encode in.ppm out.jpg [--gray] [--optimize], the flags in either order: the bytes of the optimising writer"""
    import subprocess
    from jpezy_amd import _build
    _build.build_all()
    enc = Path(_build.BIN) / "jpezy_encode"
    W, H = 100, 37
    r, g, b = oracle.synth_rgb(W, H, frame=1)
    src = tmp_path / "in.ppm"
    src.write_bytes(oracle.format_ppm_p3(W, H, r, g, b))
    for flags, gray in ((["--optimize"], False), (["--gray", "--optimize"], True), (["--optimize", "--gray"], True), ([], False)):
        out = tmp_path / "o.jpg"
        p = subprocess.run([str(enc), str(src), str(out), *flags], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr
        co = ctx.fdct_quant(r, g, b, W, H, gray=gray)
        assert out.read_bytes() == J.write_jpeg(co, W, H, gray, optimize="--optimize" in flags), flags
