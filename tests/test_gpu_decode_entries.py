"""Identities between the decode entries of the C-ABI that hold because one entry hands its call to another, or because two entries run
the same stage into different memory: they held before the host layer got its one driver and must survive it.  Three 40 x 24 files
(jpezy's own 4:2:0, 4:2:2, one component); the calls go through bare ctypes (tests/decode_entry_table.py), so strides the Python
wrappers never pass are covered."""
import numpy as np
import pytest

import decode_entry_table as T

pytestmark = pytest.mark.gpu
W, H = T.W, T.H
FILL = 0xA5
FILES = ("420", "422", "one")


@pytest.fixture(scope="module")
def env():
    import jpezy_amd as J
    ctx = J.Context(0)
    yield T.Env(J, ctx._h)
    ctx.close()


def host_planes(env, entry, file, n, **over):
    for h in env.host:
        h[:] = FILL
    rc, _ = env.call(entry, file, over)
    assert rc == 0, (entry, file, over, env.lib.jpezy_hip_last_error().decode())
    assert all((h[n:n + 64] == FILL).all() for h in env.host), "written behind the plane"
    return [h[:n].copy() for h in env.host]


def host_packed(env, entry, file, w, h, fmt, **over):
    """-> (planes r, g, b de-interleaved, alpha or None); rows 5 bytes wider than tight, the bytes between them must keep the fill"""
    nb = 4 if fmt >= 2 else 3
    row = w * nb + 5
    buf = env.host[0]
    buf[:] = FILL
    rc, _ = env.call(entry, file, dict(over, format=fmt, row_stride=row, pix_cap=(h - 1) * row + w * nb))
    assert rc == 0, (entry, file, over, env.lib.jpezy_hip_last_error().decode())
    img = buf[:h * row].reshape(h, row)
    assert (img[:-1, w * nb:] == FILL).all() and (buf[(h - 1) * row + w * nb:] == FILL).all(), "bytes outside the rows were written"
    px = img[:, :w * nb].reshape(h, w, nb)
    order = (2, 1, 0) if fmt in (1, 3) else (0, 1, 2)
    return [px[:, :, k].reshape(-1).copy() for k in order], (px[:, :, 3].copy() if nb == 4 else None)


def dev_planes(env, entry, file, n, n_frames=1, stride=None, **over):
    """-> [frame][plane] of what a planar device entry wrote"""
    import torch
    outs = env.files[file]["dev_tensors"]
    for o in outs:
        o.fill_(FILL)
    torch.cuda.synchronize()
    stride = stride if stride is not None else n
    if entry != "dequant_idct_generic_dev":
        over = dict(over, n_frames=n_frames, plane_stride=stride)
    rc, _ = env.call(entry, file, over)
    assert rc == 0, (entry, file, over, env.lib.jpezy_hip_last_error().decode())
    got = [o.cpu().numpy() for o in outs]
    for g in got:
        for f in range(n_frames - 1):
            assert (g[f * stride + n:(f + 1) * stride] == FILL).all(), "bytes between the frames were written"
        assert (g[(n_frames - 1) * stride + n:] == FILL).all(), "written behind the last frame"
    return [[g[f * stride:f * stride + n].copy() for g in got] for f in range(n_frames)]


def dev_packed(env, entry, file, w, h, **over):
    """-> planes r, g, b de-interleaved from tight RGB24"""
    import torch
    out = env.files[file]["dev_tensors"][0]
    out.fill_(FILL)
    torch.cuda.synchronize()
    rc, _ = env.call(entry, file, over)
    assert rc == 0, (entry, file, over, env.lib.jpezy_hip_last_error().decode())
    got = out.cpu().numpy()
    assert (got[w * h * 3:] == FILL).all()
    px = got[:w * h * 3].reshape(h, w, 3)
    return [px[:, :, k].reshape(-1).copy() for k in range(3)]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def full(env):
    """jpezy_decode_jpeg's planes of every file: the reference of most identities, computed once"""
    return {f: host_planes(env, "decode_jpeg", f, W * H) for f in FILES}


@pytest.mark.parametrize("file", FILES)
def test_forwarding_host_entries(env, full, file):
    assert same(host_planes(env, "decode_jpeg_scaled", file, W * H, scale=1), full[file])
    assert same(host_planes(env, "decode_jpeg_upsampling", file, W * H, upsampling=T.NEAREST), full[file])
    for s in (1, 2, 4, 8):
        ws, hs = T.scaled_size(s)
        scaled = host_planes(env, "decode_jpeg_scaled", file, ws * hs, scale=s)
        assert same(host_planes(env, "decode_jpeg_region", file, ws * hs, scale=s, region=(0, 0, ws, hs)), scaled), s
    assert same(host_planes(env, "decode_jpeg_scaled", file, W * H, scale=1), full[file])


PAIRS = [("decode_jpeg_packed", "decode_jpeg", {}), ("decode_jpeg_scaled_packed", "decode_jpeg_scaled", dict(scale=2)),
         ("decode_jpeg_scaled_packed", "decode_jpeg_scaled", dict(scale=1)),
         ("decode_jpeg_region_packed", "decode_jpeg_region", dict(scale=2, region=T.REGION)),
         ("decode_jpeg_region_packed", "decode_jpeg_region", dict(scale=1, region=(7, 5, 30, 17))),
         ("decode_jpeg_region_packed", "decode_jpeg_region", dict(scale=4, region=(0, 0, 10, 6))),
         ("decode_jpeg_upsampling_packed", "decode_jpeg_upsampling", dict(upsampling=T.SMOOTH)),
         ("decode_jpeg_upsampling_packed", "decode_jpeg_upsampling", dict(upsampling=T.NEAREST))]


@pytest.mark.parametrize("file", FILES)
def test_packed_host_entries_equal_their_planar_twins(env, file):
    for packed, planar, over in PAIRS:
        w, h = T.out_size(packed, over.get("scale", 2), over.get("region", T.REGION))
        want = host_planes(env, planar, file, w * h, **over)
        for fmt in (0, 3):                          # RGB24, BGRA32
            got, alpha = host_packed(env, packed, file, w, h, fmt, **over)
            assert same(got, want), (packed, over, fmt)
            assert alpha is None or (alpha == 0xFF).all(), (packed, over, fmt)


@pytest.mark.parametrize("file", FILES)
def test_device_entries_equal_their_host_twins(env, full, file):
    assert same(dev_planes(env, "dequant_idct_generic_dev", file, W * H)[0], full[file])
    for frame in dev_planes(env, "dequant_idct_generic_batch_dev", file, W * H, n_frames=2, stride=W * H + 4):
        assert same(frame, full[file])
    for s in (1, 2, 4, 8):
        ws, hs = T.scaled_size(s)
        want = host_planes(env, "decode_jpeg_scaled", file, ws * hs, scale=s)
        # scale_denom 1 is the generic batch entry, which asks for a stride that is a multiple of 4
        for frame in dev_planes(env, "dequant_idct_scaled_dev", file, ws * hs, n_frames=2, stride=ws * hs + (4 if s == 1 else 3), scale=s):
            assert same(frame, want), s
        assert same(dev_packed(env, "dequant_idct_scaled_packed_dev", file, ws, hs, scale=s), want), s
        for region in ((ws - 5, hs - 3, 5, 3), (0, 0, ws, hs)):
            w, h = region[2:]
            want = host_planes(env, "decode_jpeg_region", file, w * h, scale=s, region=region)
            for frame in dev_planes(env, "dequant_idct_region_dev", file, w * h, n_frames=2, stride=w * h + 3, scale=s, region=region):
                assert same(frame, want), (s, region)
            assert same(dev_packed(env, "dequant_idct_region_packed_dev", file, w, h, scale=s, region=region), want), (s, region)
    for mode in (T.SMOOTH, T.NEAREST):
        want = host_planes(env, "decode_jpeg_upsampling", file, W * H, upsampling=mode)
        assert same(dev_planes(env, "dequant_idct_upsampling_dev", file, W * H, upsampling=mode)[0], want), mode
        for frame in dev_planes(env, "dequant_idct_upsampling_dev", file, W * H, n_frames=2, stride=W * H + 4, upsampling=mode):
            assert same(frame, want), mode
        assert same(dev_packed(env, "dequant_idct_upsampling_packed_dev", file, W, H, upsampling=mode), want), mode


@pytest.mark.parametrize("file", FILES)
def test_gray_gives_three_equal_planes(env, file):
    for entry, over in [("decode_jpeg", {}), ("decode_jpeg_scaled", dict(scale=2)), ("decode_jpeg_region", dict(scale=2, region=T.REGION)),
                        ("decode_jpeg_upsampling", dict(upsampling=T.SMOOTH))]:
        w, h = T.out_size(entry)
        r, g, b = host_planes(env, entry, file, w * h, gray=1, **over)
        assert np.array_equal(r, g) and np.array_equal(g, b), entry
    for entry, over in [("dequant_idct_generic_dev", {}), ("dequant_idct_generic_batch_dev", {}), ("dequant_idct_scaled_dev", dict(scale=2)),
                        ("dequant_idct_region_dev", dict(scale=2, region=T.REGION)), ("dequant_idct_upsampling_dev", dict(upsampling=T.SMOOTH))]:
        w, h = T.out_size(entry)
        r, g, b = dev_planes(env, entry, file, w * h, gray=1, **over)[0]
        assert np.array_equal(r, g) and np.array_equal(g, b), entry
