"""The GPU decoder at its value-range edges, bit-exact against the oracle unless a test says +-1 (tests/test_decode_range.py holds the
CPU side: the oracle's conversion rule against a numpy restatement of the reference, 16-bit DQT parsing, DC refusal).

(a) the exact-mode range gate of the fused kernel (MODE 0: some quantiser above 256) and the generic kernel's gate, at and one above the
    limit; (b) 16-bit and mixed DQT files in every layout; (c) reference-order sums past +-2^31 (the reference's sample is INT_MIN there:
    0 after revise_value, where a saturating conversion would give 255); (d) wide Huffman symbols; (e) DC values outside int16."""
import ctypes as C

import numpy as np
import pytest

from jpeg_synth import ZZ, synth_jpeg, wide_tables
from test_decode_range import L420, L444, GRAY, overflow_blocks, dc_walk, _dc_file

pytestmark = pytest.mark.gpu

QMAX = [257, 300, 1000, 4096, 32768, 65535]
L422 = [(2, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture()
def ctx(J):
    c = J.Context(0)
    c.set_huffdec_min_bytes(0)
    yield c
    c.close()


def _qt_arr(qt):
    a = ((C.c_uint16 * 64) * 4)()
    for t in range(len(qt)):
        for i in range(64):
            a[t][i] = int(qt[t][i])
    return a


def _info(oracle, W, H, qt):
    info = oracle.make_info(W, H)
    for t in range(2):
        for i in range(64):
            info.qt[t][i] = int(qt[t][i])
    return info


def _basis_patterns(limit):
    pats = []
    for u in range(8):
        for v in range(8):
            sx = np.sign(np.cos((2 * np.arange(8) + 1) * u * np.pi / 16) + 1e-30)
            sy = np.sign(np.cos((2 * np.arange(8) + 1) * v * np.pi / 16) + 1e-30)
            pats.append((np.outer(sy, sx) * limit).reshape(-1).astype(np.int64))
    return pats


def _gate_coeffs(W, H, mag, seed):
    """4:2:0 coefficients (zig-zag) with ONE block per quad of four MCUs at magnitude `mag` (random signs or a basis sign pattern),
    every other block zero; returns (coeffs, number of special blocks)"""
    rng = np.random.default_rng(seed)
    mc, mr = (W + 15) // 16, (H + 15) // 16
    co = np.zeros((mr, mc, 6, 64), np.int64)
    pats = _basis_patterns(mag)
    n = 0
    for y in range(mr):
        for q in range(0, mc, 4):
            nat = rng.choice([-mag, mag], 64) if (n % 3 == 0) else pats[n % 64]
            co[y, q, n % 6] = nat[ZZ]
            n += 1
    return co.astype(np.int16).reshape(-1), n


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("qmax", QMAX)
@pytest.mark.parametrize("size", [(128, 32), (72, 40)])            # 4-wave-aligned rows / a ragged last quad
def test_range_gate_at_its_boundary(J, ctx, oracle, qmax, size):
    W, H = size
    rng = np.random.default_rng(qmax)
    qt = rng.integers(1, qmax + 1, (2, 64))
    qt[qmax % 2, 0] = qmax
    qa, info = _qt_arr(qt), _info(oracle, W, H, qt)
    limit = (1 << 23) // qmax
    counts = {}
    for mag, above in ((limit, False), (limit + 1, True)):
        if mag > 32767:
            continue
        co, nspecial = _gate_coeffs(W, H, mag, seed=mag)
        for gray in (False, True):
            want = oracle.decode_planes(co, info, gray)
            fb = {}
            for force in (1, 0):
                ctx.set_force_exact(force)
                got = ctx.dequant_idct(co, W, H, qt=qa, gray=gray)
                for a, e in zip(got, want):
                    assert np.array_equal(a, e), (qmax, mag, gray, force)
                fb[force] = ctx.fallback_count()
            # every wave holds one special block: above the limit every wave is forced (at least one live MCU's 256 luma samples
            # through the reference order per wave), at the limit none is (fewer samples than above)
            counts[above, gray] = fb[0]
            if above:
                assert fb[0] >= 256 * nspecial and fb[0] > counts[False, gray], (qmax, mag, gray, fb, counts)
            for force in (0, 1):
                ctx.set_force_exact(force)
                got = ctx.dequant_idct_generic(co, info, gray=gray)
                for a, e in zip(got, want):
                    assert np.array_equal(a, e), ("generic", qmax, mag, gray, force)
            ctx.set_force_exact(0)
            # tolerance mode: within one; exact where coef_limit = 2^15 / qmax = 0 (every non-zero block is forced)
            ctx.set_decode_tolerance(1)
            got = ctx.dequant_idct(co, W, H, qt=qa, gray=gray)
            ctx.set_decode_tolerance(0)
            d = max(int(np.abs(a.astype(np.int16) - e.astype(np.int16)).max()) for a, e in zip(got, want))
            assert d <= (0 if qmax > 32768 else 1), (qmax, mag, gray, d)


# ------------------------------------------------------------------------------------------------------------------ (b)
def _dqt_files(layout, seed, pq=(1, 1), W=93, H=61, precision=8):
    from test_host_codec import ODD_LAYOUTS
    comps = {"420": L420, "444": L444, "422": L422, "gray": GRAY, "p12": GRAY, **ODD_LAYOUTS}[layout]
    rng = np.random.default_rng(seed)
    qt = rng.integers(1, 65536, (2, 64))
    for t in range(2):
        if not pq[t]:
            qt[t] = rng.integers(1, 256, 64)
    qt[0, 0] = 65535 if pq[0] else 255
    return synth_jpeg(W, H, comps, seed=seed, qt=qt, qt_precision=pq, amp=200, precision=12 if layout == "p12" else precision)


LAYOUTS = ["420", "444", "422", "gray", "p12", "411", "h4v2_partial", "h3_partial", "v4", "h4v4", "one_comp_2x2"]


@pytest.mark.parametrize("pq", [(1, 1), (0, 1)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_16bit_dqt_files(J, ctx, oracle, layout, pq):
    data, co, _ = _dqt_files(layout, seed=len(layout) + pq[0], pq=pq)
    info, d_co = ctx.read_jpeg_gpu(data)
    assert ctx.last_huffdec_passes() > 0 or layout == "h4v4", layout      # (29 blocks per MCU: the host head, test_gpu_huffdec)
    _, hco = J.read_jpeg(data)
    assert np.array_equal(d_co.cpu().numpy().reshape(-1), hco.reshape(-1)) and np.array_equal(hco.reshape(-1), co)
    for gray in (False, True):
        _, r, g, b = ctx.decode_jpeg(data, gray=gray)
        want = oracle.decode_jpeg(data, gray)
        for a, e in zip((r, g, b), want[-3:]):
            assert np.array_equal(a, np.asarray(e).reshape(-1)), (layout, gray)


@pytest.mark.parametrize("layout", ["420", "444", "gray"])
def test_16bit_dqt_batch_mixed_with_8bit(J, ctx, layout):
    """one geometry, 8-bit-table and 16-bit-table files: the batch splits them by quantiser tables; every file as decoded alone"""
    files = [_dqt_files(layout, seed=s, pq=pq, W=160, H=96)[0] for s, pq in ((1, (0, 0)), (2, (1, 1)), (3, (0, 0)), (4, (0, 1)), (5, (1, 1)))]
    files.insert(2, files[1])
    out = ctx.decode_jpeg_batch(files)
    for f, o in zip(files, out):
        _, r, g, b = ctx.decode_jpeg(f)
        assert all(np.array_equal(a, e) for a, e in zip(o[1:], (r, g, b)))


# ------------------------------------------------------------------------------------------------------------------ (c)
def _overflow_file(comps):
    blocks = overflow_blocks()
    bpm = sum(h * v for h, v, _, _ in comps)
    hmax = max(c[0] for c in comps)
    vmax = max(c[1] for c in comps)
    n = len(blocks) * bpm
    W, H = 8 * hmax * n, 8 * vmax
    co = np.zeros((n, bpm, 64), np.int64)
    for m in range(n):                                     # each block position of the MCU carries every overflow block in turn
        co[m, m // len(blocks)] = blocks[m % len(blocks)][ZZ]
    qt = np.full((2, 64), 65535)
    return synth_jpeg(W, H, comps, qt=qt, qt_precision=(1, 1), coeffs=co, tables=wide_tables())


@pytest.mark.parametrize("layout", ["420", "444", "gray"])
def test_int32_overflow_files(J, ctx, oracle, layout):
    comps = {"420": L420, "444": L444, "gray": GRAY}[layout]
    data, co, _ = _overflow_file(comps)
    for gray in (False, True):
        _, r, g, b = ctx.decode_jpeg(data, gray=gray)
        want = oracle.decode_jpeg(data, gray)
        for a, e in zip((r, g, b), want[-3:]):
            assert np.array_equal(a, np.asarray(e).reshape(-1)), (layout, gray)
        out = ctx.decode_jpeg_batch([data, data, data], gray=gray)
        for o in out:
            for a, e in zip(o[1:], want[-3:]):
                assert np.array_equal(a, np.asarray(e).reshape(-1)), ("batch", layout, gray)


@pytest.mark.parametrize("gray", [False, True])
def test_int32_overflow_direct(J, ctx, oracle, gray):
    """the fused kernel on host and device buffers (dequant_idct / dequant_idct_dev) and the generic one, Q = 65535 everywhere"""
    import torch
    blocks = overflow_blocks()
    W, H = 16 * 4 * len(blocks), 16                          # one quad per overflow block
    mc = W // 16
    co = np.zeros((1, mc, 6, 64), np.int64)
    for m in range(mc):
        co[0, m, m % 6] = blocks[(m // 6) % len(blocks)][ZZ]
        co[0, m, (m + 3) % 6] = blocks[(m // 3) % len(blocks)][ZZ]
    co = co.astype(np.int16).reshape(-1)
    qt = np.full((2, 64), 65535)
    qa, info = _qt_arr(qt), _info(oracle, W, H, qt)
    want = oracle.decode_planes(co, info, gray)
    got = ctx.dequant_idct(co, W, H, qt=qa, gray=gray)
    assert all(np.array_equal(a, e) for a, e in zip(got, want))
    got = ctx.dequant_idct_generic(co, info, gray=gray)
    assert all(np.array_equal(a, e) for a, e in zip(got, want))
    dev = torch.device("cuda", 0)
    d_co = torch.from_numpy(co).to(dev)
    out = [torch.zeros(W * H, dtype=torch.uint8, device=dev) for _ in range(3)]
    ctx.dequant_idct_dev(d_co, W, H, out[0], out[1], out[2], qt=qa, gray=gray)
    torch.cuda.synchronize()
    assert all(np.array_equal(a.cpu().numpy(), e) for a, e in zip(out, want))


# ------------------------------------------------------------------------------------------------------------------ (d)
def _wide_file(comps, seed, W=200, H=120, dc_cat16=False):
    """random coefficients of every size up to 15 bits (AC) and DC values over all of int16 (DC categories up to 15, 16 if asked)"""
    rng = np.random.default_rng(seed)
    bpm = sum(h * v for h, v, _, _ in comps)
    hmax = max(c[0] for c in comps)
    vmax = max(c[1] for c in comps)
    nmcu = -(-((W + 7) // 8) // hmax) * -(-((H + 7) // 8) // vmax)
    co = np.zeros((nmcu, bpm, 64), np.int64)
    mask = rng.random(co.shape) < 0.04                       # (long blocks would leave the device decoder's lanes out of step)
    size = rng.integers(1, 16, co.shape)
    mag = (1 << (size - 1)) + (rng.integers(0, 1 << 15, co.shape) % (1 << (size - 1)))
    co[mask] = (mag * rng.choice([-1, 1], co.shape))[mask]
    dcv = rng.integers(-32768, 32768, (nmcu, bpm))
    if not dc_cat16:                                       # consecutive DC values of one component at most 32767 apart
        dcv = np.clip(dcv, -16000, 16000)
    co[..., 0] = dcv
    return synth_jpeg(W, H, comps, coeffs=co, tables=wide_tables(), qt=np.full((2, 64), 3))


@pytest.mark.parametrize("layout", ["420", "444", "gray"])
def test_wide_huffman_symbols(J, ctx, oracle, layout):
    comps = {"420": L420, "444": L444, "gray": GRAY}[layout]
    on_gpu = 0
    for seed in range(3):
        data, co, _ = _wide_file(comps, seed)
        info, d_co = ctx.read_jpeg_gpu(data)
        on_gpu += ctx.last_huffdec_passes() > 0                       # the device decoder took the wide tables (a stream it cannot
                                                                     # bring into step goes to the host decoder: the same result)
        _, hco = J.read_jpeg(data)
        _, oco = oracle.read_jpeg(data)
        got = d_co.cpu().numpy().reshape(-1)
        assert np.array_equal(got, hco.reshape(-1)) and np.array_equal(got, oco.reshape(-1)) and np.array_equal(got, co)
        _, r, g, b = ctx.decode_jpeg(data)
        want = oracle.decode_jpeg(data)
        assert all(np.array_equal(a, np.asarray(e).reshape(-1)) for a, e in zip((r, g, b), want[-3:]))
    assert on_gpu >= 2, layout


def test_32bit_symbol(J, ctx, oracle):
    """DC category 16 with a 16-bit code: 32 bits for one symbol.  The device decoder hands such a file to the host decoder (its DC
    differences are int16); the result is the host's and the oracle's"""
    data, co, _ = _wide_file(GRAY, 7, dc_cat16=True)
    assert co.dtype == np.int16 and np.abs(np.diff(co.reshape(-1, 64)[:, 0].astype(np.int64))).max() >= 32768
    _, d_co = ctx.read_jpeg_gpu(data)
    _, hco = J.read_jpeg(data)
    _, oco = oracle.read_jpeg(data)
    got = d_co.cpu().numpy().reshape(-1)
    assert np.array_equal(got, hco.reshape(-1)) and np.array_equal(got, oco.reshape(-1)) and np.array_equal(got, co)
    out = ctx.decode_jpeg_batch([data, data])
    want = oracle.decode_jpeg(data)
    assert all(np.array_equal(a, np.asarray(e).reshape(-1)) for o in out for a, e in zip(o[1:], want[-3:]))


# ------------------------------------------------------------------------------------------------------------------ (e)
def _status(J, fn):
    try:
        fn()
    except J.JpezyError as e:
        return str(e)
    return None


def _excursion(target, lead):
    """lead zero differences, then 0, 5, a walk of three steps to `target` and back to zero in two: every difference within +-32767,
    so no DC category 16 -- what stops such a file on the GPU is the DC range check alone"""
    d = [0] * lead + [0, 5] + dc_walk(target - 5) + [-(target // 2), -(target - target // 2)]
    assert max(abs(x) for x in d) <= 32767
    return d


_SELF_SUM_OFF = """
import sys
import numpy as np
import jpezy_amd as J
good, bad = (open(p, "rb").read() for p in sys.argv[1:3])
ctx = J.Context(0)
ctx.set_huffdec_min_bytes(0)
_, co = ctx.read_jpeg_gpu(good)
assert ctx.last_huffdec_passes() > 0
assert np.array_equal(co.cpu().numpy().reshape(-1), J.read_jpeg(good)[1].reshape(-1))
try:
    ctx.read_jpeg_gpu(bad)
except J.JpezyError as e:
    assert "status -4" in str(e) and "leaves int16" in str(e), str(e)
else:
    raise SystemExit("a DC value outside int16 was decoded")
ctx.close()
print("refused")
"""


# (layout, component, lead, restart interval): 6 / 16 DC values; 5000 DC values with the excursion inside the third workgroup of the
# single-file DC pass (2048 values each) or crossing into it at its first value (lead 4092: the value at 4096 is the first outside);
# restart intervals of 8 MCUs (the lane-per-stream kernel, the excursion inside the second interval)
DC_CASES = [("gray", 0, 0, 0), ("420", 2, 0, 0), ("420", 1, 8, 8), ("gray", 0, 8, 8), ("gray", 0, 4994, 0), ("gray", 0, 4092, 0)]


@pytest.mark.parametrize("target", [32768, -32769])
@pytest.mark.parametrize("layout,comp,lead,restart", DC_CASES)
def test_dc_outside_int16_refused_on_the_gpu_paths(J, ctx, oracle, tmp_path, target, layout, comp, lead, restart):
    """A DC value one past int16, reached and left in steps the device decoder takes (no category 16): read_jpeg_gpu, decode_jpeg and the
    batch return the host decoder's status (JPEZY_E_UNSUPPORTED); the same file with the excursion ending at the edge decodes on the GPU.
    Single file: dc_local / dc_add (both forms); batch: dc_prefix_batch_kernel, or the lane-per-stream kernel for small files and
    restart intervals."""
    import os
    import subprocess
    import sys
    comps = GRAY if layout == "gray" else L420
    edge = 32767 if target > 0 else -32768
    bad, _, _ = _dc_file(_excursion(target, lead), comps, comp, restart=restart)
    good, gco, _ = _dc_file(_excursion(edge, lead), comps, comp, restart=restart)
    host = _status(J, lambda: J.read_jpeg(bad))
    assert host and "status -4" in host
    # the twin at the edge: decoded by the device decoder, equal to the host decoder
    _, d_co = ctx.read_jpeg_gpu(good)
    assert ctx.last_huffdec_passes() > 0
    assert np.array_equal(d_co.cpu().numpy().reshape(-1), gco)
    for call in (lambda: ctx.read_jpeg_gpu(bad), lambda: ctx.decode_jpeg(bad)):
        got = _status(J, call)
        assert got and "status -4" in got and "leaves int16" in got, got
    want = oracle.decode_jpeg(good)
    if not restart:                                          # (files with restart intervals are not batch candidates)
        out = ctx.decode_jpeg_batch([good, good, good])
        assert ctx.last_batch_fast_count() == 3
    out = ctx.decode_jpeg_batch([good, bad, good, bad, good], raise_on_error=False)
    for i, o in enumerate(out):
        if i % 2:
            assert o is None
        else:
            assert all(np.array_equal(a, np.asarray(e).reshape(-1)) for a, e in zip(o[1:], want[-3:]))
    if lead > 2048:                                          # the three-launch form of the DC pass (a knob read once: a fresh process)
        (tmp_path / "good.jpg").write_bytes(good)
        (tmp_path / "bad.jpg").write_bytes(bad)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env = dict(os.environ, JPEZY_DC_SELF_SUM_MAX="0", PYTHONPATH=root)
        r = subprocess.run([sys.executable, "-c", _SELF_SUM_OFF, str(tmp_path / "good.jpg"), str(tmp_path / "bad.jpg")], cwd=root, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "refused" in r.stdout, r.stdout + r.stderr
