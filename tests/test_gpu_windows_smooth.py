"""Batches of windows with smooth chroma upsampling on the GPU (include/jpezy_hip.h, SMOOTH UPSAMPLING OF WINDOWS;
Context.set_windows_upsampling, Context.decode_windows_dev, Context.decode_windows_resized_dev): every slot equal to the numpy restatement
(tests/region_smooth_model.py) and to decode_jpeg_region_packed(..., upsampling=UPSAMPLE_SMOOTH); the resized form equal to
tests/resize_model.py over those bytes.  The output tensor is pre-filled with 0xA5 and compared as a whole, so every byte outside the
windows -- row padding, the rest of a slot, the slot of a file that was refused, the bytes behind the last slot -- is checked too.  There is
no tolerance: every comparison is np.array_equal."""
import numpy as np
import pytest

import region_smooth_cases as K
import resize_model as RM
import scaled_model as M

pytestmark = pytest.mark.gpu

FILL = K.FILL
E_UNSUPPORTED = -4
TAIL = 16
OWN_SIZES = [(16, 16), (17, 9), (40, 24), (64, 48), (33, 70), (208, 120)]


@pytest.fixture(scope="module")
def J():
    import jpezy_amd
    jpezy_amd.load_library()
    return jpezy_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture()
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def own_files(J):
    """encoder-made files of jpezy's own layout, six sizes, three sets of quantiser tables: files whose streams settle in the batch form
    of the GPU Huffman decoder, so the grouped path takes them.  Noisy in every channel: chroma differs from sample to sample."""
    enc = J.Context(0)
    out = []
    try:
        for k, (W, H) in enumerate(OWN_SIZES):
            rng = np.random.default_rng(300 + k)
            yy, xx = np.mgrid[0:H, 0:W]
            planes = [np.clip(128 + 80 * np.sin((xx * (c + 2) + yy * (3 - c)) / 3.0 + c) + rng.integers(-60, 61, (H, W)), 0, 255).astype(np.uint8).reshape(-1)
                      for c in range(3)]
            enc.set_quality((40, 60, 92)[k % 3])
            out.append(enc.encode_jpeg(*planes, W, H))
    finally:
        enc.close()
    assert [(K.parsed(f)[0].width, K.parsed(f)[0].height) for f in out] == OWN_SIZES
    return out


def resolve(data, win):
    info = K.parsed(data)[0]
    scale = 1 if win is None or len(win) == 4 else win[1]
    reg = (0, 0, 0, 0) if win is None else tuple(win if len(win) == 4 else win[0])
    if reg[2] == 0 and reg[3] == 0:
        reg = (0, 0) + M.scaled_size(info.width, info.height, scale)
    return reg, scale


def nbytes(J, fmt):
    return 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4


def run(J, torch, ctx, files, wins, fmt, Hs, Ws, row_extra=0, expect=None, compare=True, **kw):
    """one decode_windows_dev call into a marker-filled buffer -> (result list, the whole buffer as numpy); compare: the WHOLE buffer against
    the smooth model's windows where expect[k] == 0 (default: every file) and the marker everywhere else"""
    n = len(files)
    nb = nbytes(J, fmt)
    row = Ws * nb + row_extra
    slot = Hs * row
    buf = torch.full((n * slot + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    d_out = buf.as_strided((n, Hs, Ws, nb), (slot, row, nb, 1))
    res = ctx.decode_windows_dev(files, d_out, wins, format=fmt, raise_on_error=False, **kw)
    got = buf.cpu().numpy()
    if not compare:
        return res, got
    exp = np.full(n * slot + TAIL, FILL, np.uint8)
    for k in range(n):
        info, placed, status = res[k]
        assert status == (0 if expect is None else expect[k]), (k, status)
        if status != 0:
            continue
        reg, scale = resolve(files[k], None if wins is None else wins[k])
        assert placed == reg, (k, placed, reg)
        img = K.interleave(J, fmt, K.want(files[k], reg, scale, False))
        for j in range(reg[3]):
            exp[k * slot + j * row:k * slot + j * row + reg[2] * nb] = img[j].reshape(-1)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, ("first differing byte", int(bad[0]), "slot", int(bad[0]) // slot, "of", n, "count", bad.size)
    return res, got


def mixed_call(own_files):
    """files and windows of one call: sizes, layouts and scales mixed, a restart-interval file and a 12-bit file among them"""
    files, wins = [], []
    for k, f in enumerate(own_files):
        info = K.parsed(f)[0]
        scale = K.SCALES[k % 4]
        ws, hs = M.scaled_size(info.width, info.height, scale)
        files += [f, f]
        wins += [((0, 0, 0, 0), scale), ((ws // 3, hs // 4, ws - ws // 3, hs - hs // 4), scale)]
    for j, layout in enumerate(("h2v1", "h1v2", "mixed", "two_chroma_blocks", "444", "411", "one")):
        for W, H in ((33, 17), (40, 24)):
            f = K.jpeg(layout, W, H)
            for scale in (K.SCALES[j % 4], K.SCALES[(j + 1) % 4]):
                ws, hs = M.scaled_size(W, H, scale)
                files.append(f)
                wins.append(((0, 0, 0, 0), scale) if scale == 8 else ((1, 1, ws - 1, hs - 1), scale))
    rst = K.jpeg("own", 40, 24, restart=2)
    assert K.parsed(rst)[0].restart_interval == 2
    twelve = K.jpeg("own", 40, 24, precision=12)
    special = {len(files): "restart", len(files) + 1: "restart", len(files) + 2: "twelve"}
    files += [rst, rst, twelve]
    wins += [((3, 2, 30, 20), 1), ((0, 0, 0, 0), 2), ((0, 0, 8, 8), 1)]
    return files, wins, special


def test_one_call_mixes_sizes_layouts_and_scales(J, torch, ctx, own_files):
    files, wins, special = mixed_call(own_files)
    twelve = [k for k, v in special.items() if v == "twelve"]
    restart = [k for k, v in special.items() if v == "restart"]
    # what the grouped path takes does not depend on the upsampling: the same call without the 12-bit file, nearest
    keep = [k for k in range(len(files)) if k not in twelve]
    run(J, torch, ctx, [files[k] for k in keep], [wins[k] for k in keep], J.PIX_RGB24, 120, 208, compare=False)
    grouped = ctx.last_batch_fast_count()
    assert 2 * len(own_files) <= grouped <= len(files) - len(twelve) - len(restart)
    ctx.set_windows_upsampling(J.UPSAMPLE_SMOOTH)
    expect = [E_UNSUPPORTED if k in twelve else 0 for k in range(len(files))]
    for fmt, row_extra in ((J.PIX_RGB24, 1), (J.PIX_BGRA32, 0)):
        res, _ = run(J, torch, ctx, files, wins, fmt, 120, 208, row_extra=row_extra, expect=expect)       # the 12-bit slot keeps the fill
        assert ctx.last_batch_fast_count() == grouped
        d_out = torch.zeros((len(files), 120, 208, nbytes(J, fmt)), dtype=torch.uint8, device="cuda:0")
        with pytest.raises(J.JpezyError, match=rf"status -4: decode_windows_dev: file {twelve[0]}: .*8-bit"):
            ctx.decode_windows_dev(files, d_out, wins, format=fmt)
    # every slot is the per-file entry's
    for k in range(len(files)):
        if k in twelve:
            continue
        reg, scale = resolve(files[k], wins[k])
        _, img = ctx.decode_jpeg_region_packed(files[k], reg, scale=scale, format=J.PIX_RGB24, upsampling=J.UPSAMPLE_SMOOTH)
        assert np.array_equal(img, K.interleave(J, J.PIX_RGB24, K.want(files[k], reg, scale, False))), k


@pytest.mark.parametrize("scale", [1, 2])
def test_picture_corners_of_the_first_and_last_file_of_a_group(J, torch, ctx, own_files, scale):
    """the neighbouring files' coefficients lie directly beside theirs: a ring sample taken across the picture's edge would be another
    file's (or lie outside the buffer)"""
    ctx.set_windows_upsampling(J.UPSAMPLE_SMOOTH)
    first, mid, last = own_files[2], own_files[4], own_files[3]
    for size in (1, 2):
        for cx in (0, 1):
            for cy in (0, 1):
                wins = []
                for f in (first, last):
                    info = K.parsed(f)[0]
                    ws, hs = M.scaled_size(info.width, info.height, scale)
                    wins.append(((cx * (ws - size), cy * (hs - size), size, size), scale))
                run(J, torch, ctx, [first, mid, last], [wins[0], ((0, 0, 0, 0), scale), wins[1]], J.PIX_RGB24, 70, 64)
                assert ctx.last_batch_fast_count() == 3


def test_slices_give_the_same_bytes(J, torch, ctx, own_files):
    ctx.set_windows_upsampling(J.UPSAMPLE_SMOOTH)
    files = [own_files[k] for k in (5, 0, 3, 1, 4)]
    wins = [((7, 9, 150, 100), 1), None, ((0, 0, 0, 0), 2), ((0, 0, 0, 0), 4), ((2, 3, 13, 30), 2)]
    _, whole = run(J, torch, ctx, files, wins, J.PIX_BGRA32, 100, 150)
    ctx.set_windows_slice_files(2)
    _, sliced = run(J, torch, ctx, files, wins, J.PIX_BGRA32, 100, 150)
    assert ctx.last_batch_fast_count() == 5 and np.array_equal(whole, sliced)


def test_the_default_is_nearest_and_the_setting_goes_both_ways(J, torch, ctx, own_files):
    files, wins = [own_files[3], own_files[2]], [((5, 3, 40, 20), 1), ((0, 0, 0, 0), 2)]
    assert ctx.windows_upsampling() == J.UPSAMPLE_NEAREST
    _, near = run(J, torch, ctx, files, wins, J.PIX_RGB24, 48, 64, compare=False)
    for k in range(2):                                                # today's bytes: the per-file entry without the keyword
        reg, scale = resolve(files[k], wins[k])
        _, img = ctx.decode_jpeg_region_packed(files[k], reg, scale=scale)
        slot = near[k * 48 * 64 * 3:(k + 1) * 48 * 64 * 3].reshape(48, 64, 3)
        assert np.array_equal(slot[:reg[3], :reg[2]], img)
    ctx.set_windows_upsampling(J.UPSAMPLE_SMOOTH)
    assert ctx.windows_upsampling() == J.UPSAMPLE_SMOOTH
    _, smooth = run(J, torch, ctx, files, wins, J.PIX_RGB24, 48, 64)
    assert not np.array_equal(smooth, near)
    with pytest.raises(J.JpezyError, match="upsampling must be"):
        ctx.set_windows_upsampling(2)
    assert ctx.windows_upsampling() == J.UPSAMPLE_SMOOTH                # a bad value leaves the setting alone
    ctx.set_windows_upsampling(J.UPSAMPLE_NEAREST)
    _, again = run(J, torch, ctx, files, wins, J.PIX_RGB24, 48, 64, compare=False)
    assert np.array_equal(again, near)


def test_the_keyword_holds_for_one_call(J, torch, ctx, own_files):
    files, wins = [own_files[3], own_files[2]], [((5, 3, 40, 20), 1), ((0, 0, 0, 0), 2)]
    _, near = run(J, torch, ctx, files, wins, J.PIX_RGB24, 48, 64, compare=False)
    run(J, torch, ctx, files, wins, J.PIX_RGB24, 48, 64, upsampling=J.UPSAMPLE_SMOOTH)
    assert ctx.windows_upsampling() == J.UPSAMPLE_NEAREST
    ctx.set_windows_upsampling(J.UPSAMPLE_SMOOTH)
    _, got = run(J, torch, ctx, files, wins, J.PIX_RGB24, 48, 64, compare=False, upsampling=J.UPSAMPLE_NEAREST)
    assert np.array_equal(got, near) and ctx.windows_upsampling() == J.UPSAMPLE_SMOOTH
    with pytest.raises(J.JpezyError, match="upsampling must be"):
        run(J, torch, ctx, files, wins, J.PIX_RGB24, 48, 64, compare=False, upsampling=3)
    assert ctx.windows_upsampling() == J.UPSAMPLE_SMOOTH
    # a call that fails puts the setting back too
    d_out = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda:0")
    ctx.set_windows_upsampling(J.UPSAMPLE_NEAREST)
    with pytest.raises(J.JpezyError):
        ctx.decode_windows_dev([b"not a jpeg"], d_out, upsampling=J.UPSAMPLE_SMOOTH)
    assert ctx.windows_upsampling() == J.UPSAMPLE_NEAREST


# ---- resized ---------------------------------------------------------------------------------------------------------------------
def run_resized(J, torch, ctx, files, wins, out, fmt, mirror=None, **kw):
    """the whole marker-filled buffer against resize_model over the smooth model's windows"""
    n = len(files)
    ow, oh = out
    nb = nbytes(J, fmt)
    row = ow * nb + 3
    slot = oh * row + 5
    buf = torch.full((n * slot + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    d_out = buf.as_strided((n, oh, ow, nb), (slot, row, nb, 1))
    res = ctx.decode_windows_resized_dev(files, d_out, wins, mirror, format=fmt, **kw)
    got = buf.cpu().numpy()
    exp = np.full(n * slot + TAIL, FILL, np.uint8)
    for k in range(n):
        reg, scale = resolve(files[k], None if wins is None else wins[k])
        assert res[k][1] == reg and res[k][2] == 0
        src = K.interleave(J, fmt, K.want(files[k], reg, scale, False))
        img = RM.resize(src, ow, oh, bool(mirror[k]) if mirror is not None else False)
        for j in range(oh):
            exp[k * slot + j * row:k * slot + j * row + ow * nb] = img[j].reshape(-1)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, ("first differing byte", int(bad[0]), "slot", int(bad[0]) // slot, "of", n, "count", bad.size)
    return got


@pytest.mark.parametrize("out, fmt_name", [((24, 24), "PIX_RGB24"), ((7, 5), "PIX_BGRA32")])
def test_resized_is_the_resampling_of_the_smooth_window(J, torch, ctx, own_files, out, fmt_name):
    rst = K.jpeg("own", 40, 24, restart=2)                              # the per-file path
    files = [own_files[5], own_files[3], own_files[1], K.jpeg("mixed", 40, 24), rst, own_files[5]]
    wins = [((7, 9, 150, 100), 1), ((0, 0, 0, 0), 2), None, ((1, 1, 19, 11), 2), ((3, 2, 30, 20), 1), ((2, 1, 50, 29), 4)]
    mirror = [0, 1, 0, 1, 1, 0]
    fmt = getattr(J, fmt_name)
    ctx.set_windows_upsampling(J.UPSAMPLE_SMOOTH)
    smooth = run_resized(J, torch, ctx, files, wins, out, fmt, mirror)
    ctx.set_windows_upsampling(J.UPSAMPLE_NEAREST)
    assert np.array_equal(run_resized(J, torch, ctx, files, wins, out, fmt, mirror, upsampling=J.UPSAMPLE_SMOOTH), smooth)
    assert ctx.windows_upsampling() == J.UPSAMPLE_NEAREST


def test_resized_large_ratio(J, torch, ctx, own_files):
    f = own_files[5]
    assert RM.taps(208, 3)[0] >= 139
    ctx.set_windows_upsampling(J.UPSAMPLE_SMOOTH)
    run_resized(J, torch, ctx, [f, f], [((0, 0, 208, 120), 1), ((5, 0, 1, 120), 1)], (3, 2), J.PIX_RGB24)


@pytest.mark.parametrize("layout", ["444", "one"])
def test_nothing_smoothed_both_smooth_entries_give_the_replicate_entries_bytes(J, torch, ctx, layout):
    """the smooth and the replicate entries are two instances of one kernel body: on a layout that smooths nothing, at a ragged 37 x 21
    and N = 8 and 1, the smooth region entry (planes and one packed format) and the smooth window-batch entry return byte for byte
    what the replicate entries return -- whole buffers, padding included"""
    assert layout in K.NOTHING_SMOOTHED
    W, H = 37, 21
    data = K.jpeg(layout, W, H)
    info, d_co = ctx.read_jpeg_gpu(data)
    fmt, nb = J.PIX_BGR24, 3
    for scale in (1, 8):
        ws, hs = M.scaled_size(W, H, scale)
        for region in ((0, 0, ws, hs), (1, 1, ws - 1, hs - 1)):            # the second: an origin that is no multiple of 4
            x, y, w, h = region
            got = {}
            for ups in (J.UPSAMPLE_NEAREST, J.UPSAMPLE_SMOOTH):
                planes = [torch.full((w * h + 4,), FILL, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
                ctx.dequant_idct_region_dev(d_co, info, region, scale, *planes, upsampling=ups)
                row = w * nb + 5
                buf = torch.full((h * row + 4,), FILL, dtype=torch.uint8, device="cuda:0")
                ctx.dequant_idct_region_dev(d_co, info, region, scale, d_img=buf.as_strided((h, w, nb), (row, nb, 1)), format=fmt, upsampling=ups)
                torch.cuda.synchronize()
                # (run: both files' status 0 and the whole buffer against the model, which replicates where nothing is smoothed)
                batch = run(J, torch, ctx, [data, data], [(region, scale), ((0, 0, 0, 0), scale)], fmt, hs, ws, row_extra=5, upsampling=ups)[1]
                got[ups] =[p.cpu().numpy() for p in planes] + [buf.cpu().numpy(), batch]
            # the replicate entries against the model, so that equality is not equality of two untouched buffers
            for a, e in zip(got[J.UPSAMPLE_NEAREST][:3], K.want(data, region, scale, False)):
                assert np.array_equal(a[:w * h].reshape(h, w), e), (layout, scale, region)
            for a, b in zip(got[J.UPSAMPLE_NEAREST], got[J.UPSAMPLE_SMOOTH]):
                assert np.array_equal(a, b), (layout, scale, region)
