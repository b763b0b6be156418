"""Batch of windows on the GPU (include/jpezy_hip.h, BATCH OF WINDOWS; Context.decode_windows_dev): one window of each of many files of
mixed sizes, layouts, quantiser and Huffman tables, scales and formats, left in a device tensor.  The independent reference is the numpy
restatement tests/test_gpu_region.py uses (tests/region_model.py over tests/scaled_model.py), imported from there; a subset is also
compared with decode_jpeg_region_packed.  The output tensor is pre-filled with 0xA5 and compared as a whole, so every byte outside the
windows -- row padding, the rest of a slot, the slot of a file that failed, the bytes behind the last slot -- is checked too.  There is
no tolerance: every comparison is np.array_equal."""
import ctypes as C
import functools

import numpy as np
import pytest

import scaled_model as M
import test_gpu_region as TR

pytestmark = pytest.mark.gpu

FILL = TR.FILL
E_BADARG, E_NOSPACE = -1, -6
SCALES = (1, 2, 4, 8)
TAIL = 16                                                          # bytes behind the last slot that must keep the marker
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


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def own_files(J):
    """encoder-made files of jpezy's own layout: six sizes, qualities 30 / 50 / 90 in turn (three sets of quantiser tables), the third and
    the last with optimised Huffman tables (three sets of device Huffman tables)"""
    enc = J.Context(0)
    out = []
    try:
        for k, (W, H) in enumerate(OWN_SIZES):
            rng = np.random.default_rng(100 + k)
            yy, xx = np.mgrid[0:H, 0:W]
            planes = [np.clip(128 + 90 * np.sin((xx * (c + 2) + yy * (3 - c)) / 9.0 + c) + rng.integers(-25, 26, (H, W)), 0, 255).astype(np.uint8).reshape(-1)
                      for c in range(3)]
            enc.set_quality((30, 50, 90)[k % 3])
            enc.set_huffman_optimize(1 if k in (2, 5) else 0)
            out.append(enc.encode_jpeg(*planes, W, H))
    finally:
        enc.close()
    infos = [TR.parsed(f)[0] for f in out]
    assert [(i.width, i.height) for i in infos] == OWN_SIZES
    assert len({bytes(np.asarray(i.qt).tobytes()) for i in infos}) == 3
    return out


def scale_of(win):
    return 1 if win is None or len(win) == 4 else win[1]


def resolve(data, win):
    """(x, y, w, h), scale of a window as the header defines it"""
    info = TR.parsed(data)[0]
    scale = scale_of(win)
    reg = (0, 0, 0, 0) if win is None else tuple(win if len(win) == 4 else win[0])
    if reg[2] == 0 and reg[3] == 0:
        reg = (0, 0) + M.scaled_size(info.width, info.height, scale)
    return reg, scale


@functools.lru_cache(maxsize=None)
def want_img(data, reg, scale, gray, fmt):
    import jpezy_amd
    img = TR._interleave(jpezy_amd, fmt, TR.want(data, reg, scale, gray))
    img.setflags(write=False)
    return img


def run(J, torch, ctx, files, wins, fmt, Hs, Ws, gray=False, row_extra=0, slot=None, expect=None, raises=None):
    """one call into a marker-filled buffer; the WHOLE buffer is compared with the expectation built from the model: file k's window where
    expect[k] == 0 (default: every file), the marker everywhere else.  Returns the call's result list."""
    n = len(files)
    nb = 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4
    row = Ws * nb + row_extra
    slot = Hs * row if slot is None else slot
    buf = torch.full((n * slot + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    d_out = buf.as_strided((n, Hs, Ws, nb), (slot, row, nb, 1))
    if raises is not None:
        with pytest.raises(J.JpezyError, match=raises):
            ctx.decode_windows_dev(files, d_out, wins, format=fmt, gray=gray)
    res = ctx.decode_windows_dev(files, d_out, wins, format=fmt, gray=gray, raise_on_error=False)
    if raises is not None:
        buf2 = torch.full_like(buf, FILL)
        buf, d_out = buf2, buf2.as_strided((n, Hs, Ws, nb), (slot, row, nb, 1))
        res = ctx.decode_windows_dev(files, d_out, wins, format=fmt, gray=gray, raise_on_error=False)
    got = buf.cpu().numpy()
    exp = np.full(n * slot + TAIL, FILL, np.uint8)
    for k in range(n):
        info, placed, status = res[k]
        want_status = 0 if expect is None else expect[k]
        if want_status is not None:
            assert status == want_status, (k, status, want_status)
        if status != 0:
            continue
        reg, scale = resolve(files[k], None if wins is None else wins[k])
        assert placed == reg, (k, placed, reg)
        fi = TR.parsed(files[k])[0]
        assert (info.width, info.height, info.ncomp) == (fi.width, fi.height, fi.ncomp)
        img = want_img(files[k], reg, scale, bool(gray), fmt)
        x, y, w, h = reg
        for j in range(h):
            exp[k * slot + j * row:k * slot + j * row + w * nb] = img[j].reshape(-1)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, ("first differing byte", int(bad[0]), "slot", int(bad[0]) // slot, "of", n, "count", bad.size)
    return res


def region_packed(J, ctx, data, reg, scale, fmt, gray=False):
    """(status, pixels) of the per-file entry through the C function"""
    arr = np.frombuffer(data, np.uint8)
    nb = 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4
    pix = np.zeros((reg[3], reg[2], nb), np.uint8)
    fi = J.FrameInfo()
    rc = J.load_library().jpezy_decode_jpeg_region_packed(ctx._h, arr.ctypes.data_as(C.c_void_p), arr.size, int(gray), scale, C.byref(J.Rect(*reg)),
                                                           C.byref(fi), fmt, 0, pix.ctypes.data_as(C.c_void_p), pix.size)
    return rc, pix


def seam_windows(data, scales):
    """[(region, scale)] for a file: test_gpu_region.windows() -- first and last MCU, the ragged right and bottom edge, a 1 x 1 window at
    the last pixel, windows that start inside an MCU -- plus an odd x with an odd w and the whole-picture form"""
    info = TR.parsed(data)[0]
    out = []
    for scale in scales:
        ws, hs = M.scaled_size(info.width, info.height, scale)
        for name, reg in TR.windows(info, scale).items():
            out.append((reg, scale))
        if ws >= 3:
            out.append(((1, 0, ws - 1 if (ws - 1) % 2 else ws - 2, min(3, hs)), scale))                 # odd x, odd w
        out.append(((0, 0, 0, 0), scale))
    return out


# ---- 1. mixed sizes, own layout, one call -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name, row_extra", [("PIX_RGB24", 1), ("PIX_BGRA32", 0)])
def test_mixed_sizes_in_one_call(J, ctx, torch, own_files, fmt_name, row_extra):
    """six sizes, three sets of quantiser tables, three sets of Huffman tables, the four scales mixed across the files, every seam window of
    every file: one call (a file is listed once per window).  RGB24 rows are Ws * 3 + 1 apart: every alignment, the byte store form"""
    files, wins = [], []
    for k, f in enumerate(own_files):
        for reg, scale in seam_windows(f, (SCALES[k % 4], SCALES[(k + 1) % 4])):
            files.append(f)
            wins.append((reg, scale))
    assert {w[1] for w in wins} == set(SCALES) and len(files) > 100
    res = run(J, torch, ctx, files, wins, getattr(J, fmt_name), 120, 208, row_extra=row_extra)
    assert all(st == 0 for _, _, st in res)
    assert ctx.last_batch_fast_count() == len(files)               # encoder-made files settle: all of them went through the one chain


# ---- 2. other layouts beside own-layout files -----------------------------------------------------------------------------------------
OTHER = sorted(set(TR.LAYOUTS) - {"own"})


@pytest.mark.parametrize("gray", [False, True])
def test_other_layouts_in_the_same_call(J, ctx, torch, own_files, gray):
    """4:4:4, 4:2:2, one component and the odd layouts, two sizes each, one 12-bit file, between own-layout files"""
    files, wins = [], []
    for k, layout in enumerate(OTHER):
        for size in ((37, 21), (101, 70)):
            f = TR.jpeg(layout, *size)
            info = TR.parsed(f)[0]
            scale = SCALES[(k + size[0]) % 4]
            named = TR.windows(info, scale)
            for name in ("ragged_edges", "from_inside_an_mcu", "four_mcu_corner"):
                if name in named:
                    files.append(f)
                    wins.append((named[name], scale))
            files.append(f)
            wins.append(None if k % 2 else ((0, 0, 0, 0), SCALES[(k + 1) % 4]))
        files.append(own_files[k % len(own_files)])
        wins.append(((1, 1, 7, 5), 1))
    f12 = TR.jpeg12("own")
    assert TR.parsed(f12)[0].precision == 12
    files += [f12, f12]
    wins += [((3, 2, 20, 11), 1), ((0, 0, 0, 0), 2)]
    run(J, torch, ctx, files, wins, J.PIX_BGR24 if gray else J.PIX_RGBA32, 70, 101, gray=gray, row_extra=3 if gray else 0)


# ---- 3. the grouped path really ran --------------------------------------------------------------------------------------------------
def test_the_grouped_path_ran(J, ctx, torch, own_files):
    """eligibility is read from the existing entry: decode_jpeg_batch([f, f]) took the batch form for both"""
    cand = list(own_files) + [TR.jpeg(layout, 101, 70) for layout in ("own", "444", "one_comp")]
    eligible = []
    for f in cand:
        ctx.decode_jpeg_batch([f, f])
        eligible.append(ctx.last_batch_fast_count() == 2)
    sizes = {OWN_SIZES[k] for k in range(len(own_files)) if eligible[k]}
    assert len(sizes) >= 4, ("encoder-made files of four different sizes must settle in the existing batch entry", eligible)
    wins = [((1, 1, 9, 5), 1) if TR.parsed(f)[0].width > 16 and TR.parsed(f)[0].height > 9 else None for f in cand]
    res = run(J, torch, ctx, cand, wins, J.PIX_RGB24, 120, 208)
    assert all(st == 0 for _, _, st in res)
    assert ctx.last_batch_fast_count() >= sum(eligible), (ctx.last_batch_fast_count(), eligible)


# ---- 4. files the grouped path declines, beside good ones -----------------------------------------------------------------------------
def test_declined_and_broken_files_beside_good_ones(J, ctx, torch, own_files):
    fmt = J.PIX_RGB24
    good = own_files[3]                                            # 64 x 48
    rst = TR.jpeg("own", 101, 70, restart=2)
    assert TR.parsed(rst)[0].restart_interval == 2
    whole = own_files[2]                                           # 40 x 24
    cut = own_files[5][:len(own_files[5]) * 2 // 3]                # ends in mid-scan
    garbage = bytes(np.random.default_rng(5).integers(0, 256, 300, dtype=np.uint8))
    Hs, Ws = 30, 50
    files = [good, rst, cut, garbage, good, good, whole]
    wins = [((5, 3, 40, 20), 1), ((30, 9, 50, 29), 1), ((0, 0, 30, 20), 1), None, ((60, 0, 10, 10), 1), ((0, 0, 50, 30), 1), ((1, 1, 13, 7), 2)]
    cut_rc, _ = region_packed(J, ctx, cut, (0, 0, 30, 20), 1, fmt)
    bad_rc, _ = region_packed(J, ctx, garbage, (0, 0, 1, 1), 1, fmt)
    assert cut_rc < 0 and bad_rc < 0
    # the slot is one byte shorter than 50 x 30 pixels need: file 5 alone does not fit
    slot = Hs * Ws * 3 - 1
    expect = [0, 0, cut_rc, bad_rc, E_BADARG, E_NOSPACE, 0]
    res = run(J, torch, ctx, files, wins, fmt, Hs, Ws, slot=slot, expect=expect, raises=r"decode_windows_dev: file 2: ")
    assert [st for _, _, st in res] == expect
    assert res[4][0].width == 64 and res[5][1] == (0, 0, 50, 30)   # the header and the window are reported for files refused for their window
    # the restart-interval file: the per-file entry's bytes
    rc, pix = region_packed(J, ctx, rst, (30, 9, 50, 29), 1, fmt)
    assert rc == 0 and np.array_equal(pix, want_img(rst, (30, 9, 50, 29), 1, False, fmt))
    rc, pix = region_packed(J, ctx, good, (5, 3, 40, 20), 1, fmt)
    assert rc == 0 and np.array_equal(pix, want_img(good, (5, 3, 40, 20), 1, False, fmt))
    # with the slot one byte longer file 5 fits
    expect[5] = 0
    run(J, torch, ctx, files, wins, fmt, Hs, Ws, slot=slot + 1, expect=expect, raises="file 2")


# ---- 5. slices ----------------------------------------------------------------------------------------------------------------------
def test_slices_give_the_same_bytes(J, ctx, torch, own_files):
    files = own_files[:5]
    wins = [((0, 0, 0, 0), 2), ((2, 1, 9, 7), 1), ((3, 3, 30, 20), 1), ((0, 0, 0, 0), 8), ((1, 20, 31, 50), 1)]
    try:
        for per_slice in (2, 0, 1):                                # three slices, one, five
            ctx.set_windows_slice_files(per_slice)
            run(J, torch, ctx, files, wins, J.PIX_BGRA32, 70, 33)
            assert ctx.last_batch_fast_count() == 5
        with pytest.raises(J.JpezyError, match="windows_slice_files"):
            ctx.set_windows_slice_files(513)
    finally:
        ctx.set_windows_slice_files(0)


# ---- 6. the workgroup-to-file search over many descriptors ------------------------------------------------------------------------------
def test_three_hundred_files(J, ctx, torch, own_files):
    """300 descriptors in one launch (16 x 16 and 24 x 8 alternating, one or two MCUs each): the search runs nine steps deep"""
    enc = J.Context(0)
    try:
        rng = np.random.default_rng(9)
        small = enc.encode_jpeg(*[rng.integers(0, 256, 24 * 8, dtype=np.uint8) for _ in range(3)], 24, 8)
    finally:
        enc.close()
    pair = (own_files[0], small)
    regs = (((0, 0, 16, 16), (3, 5, 9, 2), (15, 15, 1, 1), (0, 0, 0, 0)), ((0, 0, 24, 8), (13, 1, 7, 5), (23, 7, 1, 1), (15, 0, 2, 8)))
    files = [pair[k % 2] for k in range(300)]
    wins = [(regs[k % 2][(k // 2) % 4], 1) for k in range(300)]
    res = run(J, torch, ctx, files, wins, J.PIX_RGB24, 16, 24, row_extra=2)
    assert all(st == 0 for _, _, st in res) and ctx.last_batch_fast_count() == 300


# ---- 7. tolerance -------------------------------------------------------------------------------------------------------------------
def test_tolerance_and_force_exact_change_nothing(J, ctx, torch, own_files):
    rst = TR.jpeg("own", 101, 70, restart=2)                       # one file for the child contexts too
    files = [own_files[5], own_files[3], rst, own_files[5]]
    wins = [((7, 9, 150, 100), 1), None, ((0, 0, 0, 0), 1), ((0, 0, 0, 0), 2)]
    try:
        for force, tol in ((0, 1), (1, 0)):
            ctx.set_force_exact(force)
            ctx.set_decode_tolerance(tol)
            ctx.fallback_count()                                   # reading the counter resets it
            run(J, torch, ctx, files, wins, J.PIX_RGB24, 120, 208)
            assert ctx.fallback_count() == 0
    finally:
        ctx.set_force_exact(0)
        ctx.set_decode_tolerance(0)


# ---- 8. shared context buffers ---------------------------------------------------------------------------------------------------------
def test_call_sizes_and_the_batch_entry_afterwards(J, ctx, torch, own_files):
    before = ctx.decode_jpeg_batch(own_files)
    run(J, torch, ctx, [own_files[4]], [((1, 1, 30, 60), 1)], J.PIX_RGB24, 60, 30)                  # n = 1
    assert run(J, torch, ctx, [], [], J.PIX_RGB24, 4, 4) == []                                      # n = 0
    run(J, torch, ctx, own_files, None, J.PIX_BGR24, 120, 208)                                      # whole pictures, windows = None
    run(J, torch, ctx, own_files[:2], [((0, 0, 0, 0), 4), ((0, 0, 0, 0), 8)], J.PIX_RGBA32, 4, 5)
    # whole pictures are what the existing packed entries give
    img = ctx.decode_jpeg_packed(own_files[5], format=J.PIX_BGR24)[1]
    assert np.array_equal(img, want_img(own_files[5], (0, 0, 208, 120), 1, False, J.PIX_BGR24))
    img = ctx.decode_jpeg_scaled_packed(own_files[0], 4, format=J.PIX_RGBA32)[1]
    assert np.array_equal(img, want_img(own_files[0], (0, 0, 4, 4), 4, False, J.PIX_RGBA32))
    after = ctx.decode_jpeg_batch(own_files)
    for a, b in zip(before, after):
        assert all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    # a tensor that is not what the binding asks for
    with pytest.raises(J.JpezyError, match="d_out"):
        ctx.decode_windows_dev(own_files[:1], torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
