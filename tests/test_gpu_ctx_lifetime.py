"""Lifetime of what a context, its host pipeline, its batch children and a multi-lane handle own (jpezy_owners.h: device and
pinned buffers, streams, events, threads): create / use / destroy cycles that touch every owner and must neither leak device
memory nor change a byte of output; growth and reuse of the pinned staging buffers across small, large, small calls; a context
that stays usable after a call failed in the middle of a batch."""
import ctypes as C
import gc

import numpy as np
import pytest

from jpeg_synth import synth_jpeg

pytestmark = pytest.mark.gpu

W0, H0 = 64, 48                 # 4 x 3 MCUs: at host_chunk_bytes = 4096 a frame is three bands (9216 bytes > 2 chunks, one MCU row each)
OWN_LAYOUT = [(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]

# Free device memory after cycle 2 minus after cycle 10 of test_every_owner_through_ten_create_use_destroy_cycles, and the step
# free memory moves in, both read on one MI355X with the parent of the change that introduced the owning types -- the code that
# freed every buffer by hand is the reference for "leaks nothing".  The parent: 308379910144 bytes free after cycle 2 and after
# cycle 10.  The step (hipMemGetInfo around one hipMalloc): allocations up to 1 MiB do not move the figure (the runtime serves
# them from memory it already holds), 2 MiB + 1 byte lowers it by 4 MiB -- steps of 2 MiB.
PARENT_DROP_BYTES = 0
GRANULE_BYTES = 2 << 20


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


def _frame(oracle, W, H, k):
    """planes, oracle coefficients, oracle file, oracle planes of that file"""
    r, g, b = oracle.synth_rgb(W, H, frame=1000 * W + k)
    co = oracle.encode_coeffs(r, g, b, W, H)
    jpg = oracle.write_jpeg(co, W, H)
    return dict(rgb=(r, g, b), co=co, jpg=jpg, planes=oracle.decode_planes(co, oracle.make_info(W, H)))


@pytest.fixture(scope="module")
def ref(oracle):
    """computed once, read-only: frames of the cycle test (64 x 48: four of jpezy's own files, one file with a restart interval)
    and two frames each at 16 x 16 and 256 x 256"""
    out = {(W0, H0): [_frame(oracle, W0, H0, k) for k in range(4)]}
    rst, _, _ = synth_jpeg(W0, H0, OWN_LAYOUT, seed=5, restart=2)
    out["rst"] = dict(jpg=rst, planes=list(oracle.decode_jpeg(rst)[1:]))
    for n in (16, 256):
        out[(n, n)] = [_frame(oracle, n, n, k) for k in range(2)]
    return out


def _planes_equal(got, want):
    return all(np.array_equal(a, e) for a, e in zip(got, want))


def _decode_paths(J, ctx, fr, W, H):
    """GPU entropy writer (host-buffer form), GPU Huffman decoder, host fallback: (jpg, coefficients, coefficients)"""
    import torch
    d_co = torch.from_numpy(fr["co"].reshape(-1)).to("cuda:0")
    jpg = ctx.write_jpeg_gpu(d_co, W, H)[0]
    ctx.set_huffdec_min_bytes(0)
    _, gco = ctx.read_jpeg_gpu(fr["jpg"])
    assert ctx.last_huffdec_passes() > 0, "the GPU Huffman decoder did not take the file"
    ctx.set_huffdec_min_bytes(1 << 40)
    _, hco = ctx.read_jpeg_gpu(fr["jpg"])
    assert ctx.last_huffdec_passes() == 0, "the host fallback was not taken"
    ctx.set_huffdec_min_bytes(0)
    return jpg, gco.cpu().numpy(), hco.cpu().numpy()


def _cycle(J, ref):
    """one call of every family on a fresh context and a fresh two-lane handle, everything destroyed again; the outputs"""
    frames = ref[(W0, H0)]
    fr = frames[0]
    out = {}
    ctx = J.Context(0)
    try:
        ctx.set_host_chunk_bytes(4096)
        out["fdct"] = ctx.fdct_quant(*fr["rgb"], W0, H0)
        out["idct"] = ctx.dequant_idct(fr["co"], W0, H0)
        out["e2e"] = ctx.encode_jpeg(*fr["rgb"], W0, H0)
        out["jpg"], out["gco"], out["hco"] = _decode_paths(J, ctx, fr, W0, H0)
        got = ctx.decode_jpeg_batch([f["jpg"] for f in frames] + [ref["rst"]["jpg"]])
        assert ctx.last_batch_fast_count() == 4, "the four equal files did not take the batch form"
        out["batch"] = [list(g[1:]) for g in got]
    finally:
        ctx.close()
    planes = [np.concatenate([f["rgb"][k] for f in frames[:3]]) for k in range(3)]
    with J.MultiEncoder([0, 0], W0, H0, chunk_frames=1) as M:
        out["multi_host"] = M.encode(*planes, 3, want_coeffs=True)
        out["multi_root"] = M.encode(*planes, 3, want_coeffs=True, on_root_device=True)
    return out


def _flat(out):
    """every output of a cycle as one list of byte strings"""
    items = [out["fdct"], *out["idct"], out["e2e"], out["jpg"], out["gco"], out["hco"]]
    for planes in out["batch"]:
        items += planes
    for co, jpgs in (out["multi_host"], out["multi_root"]):
        items += [co, *jpgs]
    return [x if isinstance(x, bytes) else np.ascontiguousarray(x).tobytes() for x in items]


def _free_bytes():
    import torch
    gc.collect()
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def test_every_owner_through_ten_create_use_destroy_cycles(J, oracle, ref):
    """Ten cycles of: context + host-buffer FDCT / IDCT / encode in bands (HostPipe ring, its streams, events and threads), GPU
    entropy writer (e_pinned), GPU Huffman decoder and host fallback (h_fb_pin), a batch with four fast files and one restart-interval
    file (b_pin, b_stage, the download stream, the drainers, a child context), a two-lane handle to host memory and to the root
    device (Lane, Slot); everything destroyed.  Cycle 1 equals the oracle, cycle 10 equals cycle 1 byte for byte, and free device
    memory after cycle 10 is not lower than after cycle 2 by more than the hand-freeing parent's own drop plus one allocation
    granule (a buffer leaked once per cycle shows as eight times its size).
    Parent, one MI355X: drop 0 bytes, granule 2 MiB (PARENT_DROP_BYTES, GRANULE_BYTES above).  What the runtime serves from memory
    it already holds does not move the figure, so the bound catches leaked streams, rings and megabyte buffers at once and kilobyte
    buffers only once they have filled a granule."""
    frames = ref[(W0, H0)]
    first = _cycle(J, ref)
    fr = frames[0]
    assert np.array_equal(first["fdct"], fr["co"]) and _planes_equal(first["idct"], fr["planes"])
    assert first["e2e"] == fr["jpg"] and first["jpg"] == fr["jpg"]
    assert np.array_equal(first["gco"], fr["co"]) and np.array_equal(first["hco"], fr["co"])
    for got, want in zip(first["batch"], [f["planes"] for f in frames] + [ref["rst"]["planes"]]):
        assert _planes_equal(got, want)
    for co, jpgs in (first["multi_host"], first["multi_root"]):
        assert np.array_equal(co.reshape(3, -1), np.stack([f["co"].reshape(-1) for f in frames[:3]]))
        assert jpgs == [f["jpg"] for f in frames[:3]]
    want = _flat(first)
    free = {}
    for cycle in range(2, 11):
        last = _flat(_cycle(J, ref))
        if cycle in (2, 10):
            free[cycle] = _free_bytes()
    drop = free[2] - free[10]
    print(f"free device memory after cycle 2: {free[2]}, after cycle 10: {free[10]}, drop {drop} bytes")
    assert last == want, "cycle 10 differs from cycle 1"
    assert drop <= PARENT_DROP_BYTES + GRANULE_BYTES, (drop, PARENT_DROP_BYTES, GRANULE_BYTES)


def test_small_large_small_on_one_context(J, oracle, ref):
    """16 x 16, 256 x 256, 16 x 16 through the paths with a pinned buffer of their own: entropy writer (exact size), batch
    scans (n + n/4 + 4096), host fallback (exact, soft), batch planes (n + n/4, soft) -- each grows once and the over-sized
    buffer is used again by the small call after it.  Every output against the oracle."""
    ctx = J.Context(0)
    try:
        for n in (16, 256, 16):
            a, b = ref[(n, n)]
            for fr in (a, b):
                jpg, gco, hco = _decode_paths(J, ctx, fr, n, n)
                assert jpg == fr["jpg"], n
                assert np.array_equal(gco, fr["co"]) and np.array_equal(hco, fr["co"]), n
            got = ctx.decode_jpeg_batch([a["jpg"], b["jpg"]])
            assert ctx.last_batch_fast_count() == 2, n
            for g, fr in zip(got, (a, b)):
                assert _planes_equal(g[1:], fr["planes"]), n
    finally:
        ctx.close()


def _batch_with_caps(J, ctx, files, caps):
    """jpezy_decode_jpeg_batch with the caller's plane capacities as given: (rc, status, planes)"""
    lib = J.load_library()
    n = len(files)
    arrs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    planes = [[np.zeros(W0 * H0, dtype=np.uint8) for _ in range(3)] for _ in range(n)]
    vpa = C.c_void_p * n
    rr, gg, bb = (vpa(*[p[k].ctypes.data for p in planes]) for k in range(3))
    infos, status = (J.FrameInfo * n)(), (C.c_int * n)()
    rc = lib.jpezy_decode_jpeg_batch(ctx._h, n, vpa(*[a.ctypes.data for a in arrs]), (C.c_size_t * n)(*[a.size for a in arrs]), 0, infos,
                                     rr, gg, bb, (C.c_size_t * n)(*caps), status)
    return rc, list(status), planes


def test_a_failing_file_mid_batch_leaves_the_context_usable(J, oracle, ref):
    """one plane buffer too small among four good files: the batch returns that file's error (an argument error; the other files are
    decoded), and the next call on the same context with good arguments equals the oracle"""
    frames = ref[(W0, H0)]
    files = [f["jpg"] for f in frames] + [frames[0]["jpg"]]
    ok_cap = W0 * H0
    ctx = J.Context(0)
    try:
        ctx.set_huffdec_min_bytes(0)
        rc, status, planes = _batch_with_caps(J, ctx, files, [ok_cap, ok_cap, ok_cap - 1, ok_cap, ok_cap])
        assert rc < 0 and status[2] == rc and "file 2" in J.load_library().jpezy_hip_last_error().decode()
        for i in (0, 1, 3, 4):
            assert status[i] == 0 and _planes_equal(planes[i], frames[i % 4]["planes"]), i
        rc, status, planes = _batch_with_caps(J, ctx, files, [ok_cap] * 5)
        assert rc == 0 and status == [0] * 5
        for i in range(5):
            assert _planes_equal(planes[i], frames[i % 4]["planes"]), i
        assert ctx.encode_jpeg(*frames[1]["rgb"], W0, H0) == frames[1]["jpg"]
    finally:
        ctx.close()
