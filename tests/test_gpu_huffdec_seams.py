"""The GPU Huffman decoder (jpezy_huffdec.hip, jpezy_huffdec_core.h, jpezy_capi_huffdec.hip) at its own seams, each hit on purpose
by a file from tests/huffdec_seams_model.py (proved on the CPU by tests/test_huffdec_seams_model.py): stuffing bytes on the 64-byte
chunks and 16 KB workgroups of the unstuffing kernels, symbols of every kind across subsequence ends, quarter marks and the
workgroup seams of the coefficient and synchronisation passes, blocks longer than a subsequence, stretches of minimum-length
blocks, every way a scan can end, the DC pass around its 2,048-term workgroups, restart intervals through the batch form and the
lane-per-stream kernel, and the speculation distance at 1 and at the window's limit.

Every case compares three things bit for bit -- the coefficients the file was built from, the host decoder, the GPU decoder -- and
asserts which path ran: the GPU decoder (last_huffdec_passes() > 0) for every case but the ones of the exception table
(huffdec_seams_model.EXCEPTIONS), each of which names the decoder's own rule that hands it to the host decoder and asserts == 0."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import huffdec_seams_model as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    c.set_huffdec_min_bytes(0)          # every scan through the GPU decoder, however small
    yield c
    c.close()


def three_way(J, ctx, case, data, on_gpu):
    """constructed coefficients == host decoder == GPU decoder, and the path that ran"""
    truth = case.coeffs
    info, host = J.read_jpeg(data)
    assert np.array_equal(host.reshape(truth.shape), truth), f"{case}: host decoder != constructed coefficients"
    ginfo, got = ctx.read_jpeg_gpu(data)
    passes = ctx.last_huffdec_passes()
    got = got.cpu().numpy()
    print(f"{case}: {len(data)} bytes, last_huffdec_passes {passes}, landed {len(case.landed)}")
    assert (ginfo.width, ginfo.height, ginfo.ncomp, ginfo.blocks_per_mcu) == (info.width, info.height, info.ncomp, info.blocks_per_mcu)
    assert got.size == truth.size
    got = got.reshape(truth.shape)
    assert np.array_equal(got, truth), (str(case), np.argwhere(got != truth)[:5].tolist())
    if on_gpu:
        assert passes > 0, f"{case}: handed to the host decoder (no rule of the exception table says so)"
    else:
        assert passes == 0, f"{case}: decoded on the GPU, but {case.host_rule} sends it to the host decoder"


def run(J, ctx, name):
    assert name not in S.EXCEPTIONS
    three_way(J, ctx, S.case(name), S.file_of(J, name), on_gpu=True)


STRADDLES = [n for n, (_, f, _) in S.REGISTRY.items() if f is S.straddle_for]


# ---- A. unstuffing ----
@pytest.mark.parametrize("name", S.names("A"))
def test_unstuffing(J, ctx, name):
    run(J, ctx, name)


@pytest.mark.parametrize("name", [f"length{S.CHUNK - 1}-own420", f"length{S.COPY_WG_BYTES - 1}-one", "lastff-own420"])
def test_bytes_behind_the_eoi(J, ctx, name):
    rng = np.random.default_rng(5)
    data = S.file_of(J, name)
    for tail in (b"\x00", b"\xff", b"\xff\x00\xff\xd9", rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()):
        three_way(J, ctx, S.case(name), data + tail, on_gpu=True)


# ---- B. symbols on lane, mark and workgroup boundaries: one test per kind of boundary ----
@pytest.mark.parametrize("layout", S.STRADDLE_LAYOUTS)
def test_symbols_across_interior_subsequence_ends(J, ctx, layout):
    run(J, ctx, f"interior-{layout}")


@pytest.mark.parametrize("layout", S.STRADDLE_LAYOUTS)
def test_symbols_across_quarter_marks(J, ctx, layout):
    run(J, ctx, f"quarter-{layout}")


@pytest.mark.parametrize("layout", S.STRADDLE_LAYOUTS)
def test_symbols_across_coefficient_pass_workgroup_seams(J, ctx, layout):
    run(J, ctx, f"emit_wg-{layout}")


@pytest.mark.parametrize("layout", S.STRADDLE_LAYOUTS)
def test_symbols_across_synchronisation_workgroup_seams(J, ctx, layout):
    run(J, ctx, f"sync_wg-{layout}")


@pytest.mark.parametrize("name", [n for n in S.names("B") if n not in STRADDLES])
def test_long_blocks_short_blocks_scan_ends(J, ctx, name):
    run(J, ctx, name)


def test_zrl_one_position_past_the_block_is_refused_by_both(J, ctx):
    """k + 16 == 65: the same refusal from the host decoder and from read_jpeg_gpu (zrl-reach64, the valid edge, is a case above)"""
    data = S.raw_file(S.zrl_case(65))
    with pytest.raises(J.JpezyError) as host:
        J.read_jpeg(data)
    with pytest.raises(J.JpezyError) as gpu:
        ctx.read_jpeg_gpu(data)
    status = [re.search(r"status (-?\d+)", str(e.value)).group(1) for e in (host, gpu)]
    assert status[0] == status[1], (str(host.value), str(gpu.value))
    run(J, ctx, "zrl-reach64")          # and the context is still good


@pytest.mark.parametrize("name", sorted(S.EXCEPTIONS))
def test_exception_table(J, ctx, name):
    c = S.case(name)
    assert c.host_rule == S.EXCEPTIONS[name]
    three_way(J, ctx, c, S.file_of(J, name), on_gpu=False)


# ---- C. speculation distance ----
def test_speculation_distance_one_and_window_limit(J, tmp_path):
    """JPEZY_HUFFDEC_OVERFLOW is read once per process: a fresh child for 1 and for OVERFLOW (the window's limit) decodes every
    section-B file -- the straddles, the long and the short blocks, the scan ends, the ZRL edge; same coefficients, all on the GPU"""
    names = S.names("B")
    for name in names:
        (tmp_path / f"{name}.jpg").write_bytes(S.file_of(J, name))
        np.save(tmp_path / f"{name}.npy", S.case(name).coeffs)
    script = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {str(ROOT)!r})\n"
        "from pathlib import Path\n"
        "import jpezy_amd as J\n"
        "ctx = J.Context(0); ctx.set_huffdec_min_bytes(0)\n"
        f"files = sorted(Path({str(tmp_path)!r}).glob('*.jpg'))\n"
        "for f in files:\n"
        "    want = np.load(f.with_suffix('.npy'))\n"
        "    info, got = ctx.read_jpeg_gpu(f.read_bytes())\n"
        "    assert ctx.last_huffdec_passes() > 0, f'{f.name}: host decoder used'\n"
        "    assert np.array_equal(got.cpu().numpy().reshape(want.shape), want), f.name\n"
        "print('OK', len(files))\n")
    for overflow in (1, S.OVERFLOW):
        env = dict(os.environ, JPEZY_HUFFDEC_OVERFLOW=str(overflow))
        p = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=240)
        assert p.returncode == 0 and f"OK {len(names)}" in p.stdout, (overflow, p.stdout[-2000:] + p.stderr[-2000:])


# ---- D. DC pass ----
@pytest.mark.parametrize("nmcu", S.DC_PASS_MCUS)
def test_dc_pass_around_its_workgroups(J, ctx, nmcu):
    data, co = S.dc_pass_file(nmcu)

    class Named:
        coeffs, landed, host_rule = co, [dict(kind="dc_pass", luma_terms=4 * nmcu, chroma_terms=nmcu)], None

        def __repr__(self):
            return f"dc-pass-{nmcu}"
    assert {4 * nmcu // S.DC_PER_WG, nmcu // S.DC_PER_WG} <= {0, 1, 2, 3, 4, 8}
    three_way(J, ctx, Named(), data, on_gpu=True)


# ---- E. batch form and lane-per-stream kernel ----
@pytest.mark.parametrize("name", S.names("E"))
def test_restart_intervals(J, ctx, name):
    run(J, ctx, name)


def test_constructed_files_in_one_batch(J, ctx, oracle):
    """every constructed file of sections A and B (restart files take no batch form) twice -- the batch form takes groups of two and
    more files of one size, so each file is its own pair -- beside the exception table's files and ordinary ones, in one
    decode_jpeg_batch call: the pixels of the per-file decode, and exactly the files the tests above assert on the GPU path take the
    batch form"""
    names = S.names("A") + S.names("B")
    files = [S.file_of(J, n) for n in names for _ in (0, 1)]
    gpu = len(files)
    files += [S.file_of(J, n) for n in sorted(S.EXCEPTIONS) for _ in (0, 1)]          # the host decoder's: not counted
    for k in range(3):
        r, g, b = oracle.synth_rgb(208, 120, frame=300 + k)
        files.append(ctx.encode_jpeg(r, g, b, 208, 120))
        ctx.read_jpeg_gpu(files[-1])
        assert ctx.last_huffdec_passes() > 0
        gpu += 1
    order = np.random.default_rng(1).permutation(len(files))
    files = [files[i] for i in order]
    got = ctx.decode_jpeg_batch(files)
    fast = ctx.last_batch_fast_count()
    print(f"{len(files)} files in one batch, {fast} took the batch form, {gpu} decode on the GPU one by one")
    one = {}
    for i, f in enumerate(files):
        if f not in one:
            one[f] = ctx.decode_jpeg(f)
        for q in (1, 2, 3):
            assert np.array_equal(got[i][q], one[f][q]), (i, q)
    assert fast == gpu, (fast, gpu)
