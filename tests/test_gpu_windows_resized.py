"""Batch of windows, resized, on the GPU (include/jpezy_hip.h, BATCH OF WINDOWS, RESIZED; Context.decode_windows_resized_dev): one window of
each of several files of mixed sizes, layouts, tables and scales, every window resampled to one output size.  The expectation is
tests/resize_model.py (the numpy restatement of the resampling) over the region restatement tests/test_gpu_region.py uses, interleaved per
format as tests/test_gpu_windows.py does.  The output buffer is pre-filled with 0xA5 and compared as a whole, so row padding, slot
padding, the slot of a file that failed and the bytes behind the last slot are checked too.  There is no tolerance: every comparison is
np.array_equal."""
import functools

import numpy as np
import pytest

import resize_model as RM
import scaled_model as M
import test_gpu_region as TR
import test_gpu_windows as TW

pytestmark = pytest.mark.gpu

FILL = TR.FILL
E_BADARG, E_NOSPACE = -1, -6
TAIL = 16                                                          # bytes behind the last slot that must keep the marker
OWN_SIZES = TW.OWN_SIZES


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
    """the six encoder-made files of tests/test_gpu_windows.py, built the same way: 16 x 16 ... 208 x 120, qualities 30 / 50 / 90 in turn, the
    third and the last with optimised Huffman tables"""
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
    assert [(TR.parsed(f)[0].width, TR.parsed(f)[0].height) for f in out] == OWN_SIZES
    return out


@functools.lru_cache(maxsize=None)
def want_resized(data, reg, scale, gray, fmt, out_w, out_h, mirror):
    img = RM.resize(TW.want_img(data, reg, scale, gray, fmt), out_w, out_h, mirror)
    img.setflags(write=False)
    return img


def run(J, torch, ctx, files, wins, out, fmt, mirror=None, gray=False, row_extra=0, slot_extra=0, slot=None, expect=None, raises=None):
    """one call into a marker-filled buffer; the WHOLE buffer is compared with the expectation: file k's out_w x out_h pixels where
    expect[k] == 0 (default: every file), the marker everywhere else.  Returns (the call's result list, the buffer as numpy, row, slot)."""
    n = len(files)
    ow, oh = out
    nb = 3 if fmt in (J.PIX_RGB24, J.PIX_BGR24) else 4
    row = ow * nb + row_extra
    slot = (oh * row + slot_extra) if slot is None else slot
    buf = torch.full((n * slot + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    d_out = buf.as_strided((n, oh, ow, nb), (slot, row, nb, 1))
    if raises is not None:
        with pytest.raises(J.JpezyError, match=raises):
            ctx.decode_windows_resized_dev(files, d_out, wins, mirror, format=fmt, gray=gray)
        buf.fill_(FILL)
    res = ctx.decode_windows_resized_dev(files, d_out, wins, mirror, format=fmt, gray=gray, raise_on_error=False)
    got = buf.cpu().numpy()
    exp = np.full(n * slot + TAIL, FILL, np.uint8)
    for k in range(n):
        info, placed, status = res[k]
        want_status = 0 if expect is None else expect[k]
        if want_status is not None:
            assert status == want_status, (k, status, want_status)
        if status != 0:
            continue
        reg, scale = TW.resolve(files[k], None if wins is None else wins[k])
        assert placed == reg, (k, placed, reg)                                       # the SOURCE window as decoded
        fi = TR.parsed(files[k])[0]
        assert (info.width, info.height, info.ncomp) == (fi.width, fi.height, fi.ncomp)
        img = want_resized(files[k], reg, scale, bool(gray), fmt, ow, oh, bool(mirror[k]) if mirror is not None else False)
        for j in range(oh):
            exp[k * slot + j * row:k * slot + j * row + ow * nb] = img[j].reshape(-1)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, ("first differing byte", int(bad[0]), "slot", int(bad[0]) // slot, "of", n, "count", bad.size, "got", int(got[bad[0]]),
                           "want", int(exp[bad[0]]))
    return res, got, row, slot


def slot_pixels(got, k, out, nb, row, slot):
    ow, oh = out
    return np.stack([got[k * slot + j * row:k * slot + j * row + ow * nb].reshape(ow, nb) for j in range(oh)])


# ---- 1. mixed up- and down-sampling in one call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", [(24, 24), (7, 5), (1, 1), (32, 48), (130, 19)])
@pytest.mark.parametrize("fmt_name, row_extra, slot_extra", [("PIX_RGB24", 1, 5), ("PIX_BGRA32", 8, 0)])
def test_whole_pictures_of_mixed_sizes_to_one_size(J, ctx, torch, own_files, out, fmt_name, row_extra, slot_extra):
    """16 x 16 ... 208 x 120 to one size: 17 x 9 grows to 24 x 24 while 208 x 120 shrinks 8.7 x 5 times; 7 x 5 and the odd RGB24 rows force the
    byte stores; padded rows and slots keep the marker.  130 x 19 is three workgroups wide and two high per file (a workgroup is a tile of
    64 x 16 output pixels), the last group of a row two pixels"""
    res, _, _, _ = run(J, torch, ctx, own_files, None, out, getattr(J, fmt_name), row_extra=row_extra, slot_extra=slot_extra)
    assert all(st == 0 for _, _, st in res)
    assert ctx.last_batch_fast_count() == len(own_files)


# ---- 2. windows at every scale, degenerate sources, every picture edge ----------------------------------------------------------------------
def test_windows_at_every_scale(J, ctx, torch, own_files):
    files, wins = [], []
    for k, f in enumerate(own_files):
        info = TR.parsed(f)[0]
        for scale in (1, 2, 4, 8):
            ws, hs = M.scaled_size(info.width, info.height, scale)
            regs = [(0, 0, ws, hs), (ws - 1, hs - 1, 1, 1), (0, 0, 1, 1), (ws - 1, 0, 1, hs), (0, hs - 1, ws, 1),           # whole, 1 x 1, 1 x h, w x 1
                    (ws // 3, 0, ws - ws // 3, max(1, hs // 2)), (0, hs // 3, max(1, ws // 2), hs - hs // 3)]                  # right + top, left + bottom
            for reg in regs[(k + scale) % 2::2] + regs[1:2]:
                files.append(f)
                wins.append((reg, scale))
    assert {w[1] for w in wins} == {1, 2, 4, 8} and any(w[0][2:] == (1, 1) for w in wins) and any(w[0][2] == 1 and w[0][3] > 1 for w in wins)
    out = (9, 6)
    res, got, row, slot = run(J, torch, ctx, files, wins, out, J.PIX_RGB24, row_extra=2)
    assert all(st == 0 for _, _, st in res) and ctx.last_batch_fast_count() == len(files)
    ones = [k for k, w in enumerate(wins) if w[0][2:] == (1, 1)]
    for k in ones:                                                   # every output pixel of a 1 x 1 source equals it
        px = slot_pixels(got, k, out, 3, row, slot)
        src = TW.want_img(files[k], wins[k][0], wins[k][1], False, J.PIX_RGB24)
        assert (px == src[0, 0]).all(), k


# ---- 3. a ratio far beyond any tile ---------------------------------------------------------------------------------------------------------
def test_large_ratio(J, ctx, torch, own_files):
    """208 x 120 to 3 x 2: about 140 horizontal and 120 vertical taps per output pixel; and a column and a row of it to one pixel"""
    f = own_files[5]
    assert RM.taps(208, 3)[0] >= 139
    run(J, torch, ctx, [f, f, f], [((0, 0, 208, 120), 1), ((0, 7, 208, 1), 1), ((5, 0, 1, 120), 1)], (3, 2), J.PIX_RGB24)
    run(J, torch, ctx, [f], None, (1, 1), J.PIX_BGRA32)


# ---- 4. identity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt_name", ["PIX_RGB24", "PIX_RGBA32"])
def test_identity_equals_decode_windows_dev(J, ctx, torch, own_files, fmt_name):
    fmt = getattr(J, fmt_name)
    nb = 3 if fmt == J.PIX_RGB24 else 4
    w, h = 13, 7
    files = [own_files[1], own_files[2], own_files[3], own_files[4], own_files[5], own_files[5]]
    wins = [((2, 1, w, h), 1), ((20, 17, w, h), 1), ((3, 2, w, h), 2), ((0, 10, w, h), 2), ((13, 8, w, h), 4), ((0, 0, w, h), 8)]
    _, got, row, slot = run(J, torch, ctx, files, wins, (w, h), fmt, row_extra=3)
    buf = torch.full((len(files) * slot + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    ctx.decode_windows_dev(files, buf.as_strided((len(files), h, w, nb), (slot, row, nb, 1)), wins, format=fmt)
    assert np.array_equal(buf.cpu().numpy(), got)


# ---- 5. mirror --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", [(24, 24), (7, 5)])
def test_mirror_is_the_column_reverse(J, ctx, torch, own_files, out):
    """every file once without and once with the flag, mixed in one call"""
    files = [f for f in own_files for _ in (0, 1)]
    mirror = [k % 2 for k in range(len(files))]
    for fmt, nb in ((J.PIX_RGB24, 3), (J.PIX_BGRA32, 4)):
        _, got, row, slot = run(J, torch, ctx, files, None, out, fmt, mirror=mirror, row_extra=1 if nb == 3 else 0)
        for k in range(0, len(files), 2):
            assert np.array_equal(slot_pixels(got, k + 1, out, nb, row, slot), slot_pixels(got, k, out, nb, row, slot)[:, ::-1]), k


# ---- 6. gray, other layouts ---------------------------------------------------------------------------------------------------------------
OTHER = sorted(set(TR.LAYOUTS) - {"own"})


@pytest.mark.parametrize("gray", [False, True])
def test_gray_and_other_layouts(J, ctx, torch, own_files, gray):
    rst = TR.jpeg("own", 101, 70, restart=2)                       # the per-file path in these formats too
    files = [TR.jpeg(layout, 37, 21) for layout in OTHER] + [own_files[2], own_files[4], rst, rst]
    wins = [None if k % 2 else ((1, 0, 11 + k % 5, 9), 2 if k % 4 == 0 else 1) for k in range(len(files))]      # (37 x 21 is 19 x 11 at 1/2)
    mirror = [(k // 2) % 2 for k in range(len(files))]
    run(J, torch, ctx, files, wins, (10, 12), J.PIX_BGR24 if gray else J.PIX_RGBA32, mirror=mirror, gray=gray, row_extra=2 if gray else 0)


# ---- 7. paths -----------------------------------------------------------------------------------------------------------------------------
def test_paths_give_the_same_bytes(J, ctx, torch, own_files):
    """a restart-interval file (child context) and a file of another layout (a group of its own) beside grouped ones: the bytes of each file
    alone; the grouped count is the existing entry's; slices of one and two files give the bytes of automatic"""
    rst = TR.jpeg("own", 101, 70, restart=2)
    assert TR.parsed(rst)[0].restart_interval == 2
    files = [own_files[3], rst, own_files[5], TR.jpeg("444", 37, 21), own_files[1], rst]
    wins = [((5, 3, 40, 20), 1), ((30, 9, 50, 29), 1), None, None, ((0, 0, 0, 0), 1), ((0, 0, 0, 0), 2)]
    mirror = [0, 1, 1, 0, 0, 0]
    out, fmt = (12, 10), J.PIX_RGB24
    _, together, row, slot = run(J, torch, ctx, files, wins, out, fmt, mirror=mirror, row_extra=1)
    fast = ctx.last_batch_fast_count()
    big = torch.empty((len(files), 120, 208, 3), dtype=torch.uint8, device="cuda:0")
    ctx.decode_windows_dev(files, big, wins, format=fmt)
    assert fast == ctx.last_batch_fast_count() and 3 <= fast <= len(files) - 2          # the restart-interval files went file by file
    for k in range(len(files)):
        _, alone, _, _ = run(J, torch, ctx, [files[k]], [wins[k]], out, fmt, mirror=[mirror[k]], row_extra=1)
        assert np.array_equal(alone[:slot], together[k * slot:(k + 1) * slot]), k
    try:
        for per_slice in (1, 2):
            ctx.set_windows_slice_files(per_slice)
            _, sliced, _, _ = run(J, torch, ctx, files, wins, out, fmt, mirror=mirror, row_extra=1)
            assert np.array_equal(sliced, together) and ctx.last_batch_fast_count() == fast
    finally:
        ctx.set_windows_slice_files(0)


# ---- 8. failures --------------------------------------------------------------------------------------------------------------------------
def test_failing_files_leave_their_slots_alone(J, ctx, torch, own_files):
    fmt = J.PIX_RGB24
    cut = own_files[5][:len(own_files[5]) * 2 // 3]                # ends in mid-scan
    cut_rc, _ = TW.region_packed(J, ctx, cut, (0, 0, 30, 20), 1, fmt)
    assert cut_rc < 0
    files = [own_files[3], cut, own_files[3], own_files[2]]
    wins = [((5, 3, 40, 20), 1), ((0, 0, 30, 20), 1), ((60, 0, 10, 10), 1), ((1, 1, 13, 7), 2)]
    expect = [0, cut_rc, E_BADARG, 0]
    res, _, _, _ = run(J, torch, ctx, files, wins, (8, 6), fmt, expect=expect, raises=r"decode_windows_resized_dev: file 1: ", row_extra=1, slot_extra=3)
    assert [st for _, _, st in res] == expect
    assert res[2][0].width == 64 and res[2][1] == (0, 0, 0, 0)     # the header is reported; a window outside the picture is not placed
    # slots one byte too small: the call is refused and nothing is written
    ow, oh = 8, 6
    slot = oh * ow * 3 - 1
    buf = torch.full((2 * slot + TAIL,), FILL, dtype=torch.uint8, device="cuda:0")
    d_out = buf.as_strided((2, oh, ow, 3), (slot, ow * 3, 3, 1))
    with pytest.raises(J.JpezyError, match="does not fit a slot"):
        ctx.decode_windows_resized_dev(own_files[:2], d_out)
    ctx.decode_windows_resized_dev(own_files[:2], d_out, raise_on_error=False)
    assert (buf.cpu().numpy() == FILL).all()
    d_out = torch.full((2 * (slot + 1),), FILL, dtype=torch.uint8, device="cuda:0").as_strided((2, oh, ow, 3), (slot + 1, ow * 3, 3, 1))
    assert [st for _, _, st in ctx.decode_windows_resized_dev(own_files[:2], d_out)] == [0, 0]       # one byte longer: it fits
    with pytest.raises(J.JpezyError, match="d_out"):
        ctx.decode_windows_resized_dev(own_files[:1], torch.zeros((1, 4, 4, 3), dtype=torch.uint8))
    with pytest.raises(J.JpezyError, match="mirror"):
        ctx.decode_windows_resized_dev(own_files[:1], d_out[:1], mirror=[0, 1])
    assert ctx.decode_windows_resized_dev([], torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device="cuda:0")) == []


# ---- 9. the windows of resize_pick_window, as they come ---------------------------------------------------------------------------------------
def test_pick_window_feeds_the_call(J, ctx, torch, own_files):
    files, wins = [], []
    for k, f in enumerate(own_files):
        info = TR.parsed(f)[0]
        W, H = info.width, info.height
        for src in ((0, 0, W, H), (W // 5, H // 7, W - W // 5, H - H // 7), (1, 1, max(1, W // 2), max(1, H // 2))):
            win = J.resize_pick_window(W, H, src, 16, 16)
            assert win == RM.pick_window(W, H, src, 16, 16)
            files.append(f)
            wins.append(win)
    assert {w[1] for w in wins} >= {1, 2, 4}                        # 208 x 120 leaves 16 x 16 at 1/4, 64 x 48 at 1/2
    res, _, _, _ = run(J, torch, ctx, files, wins, (16, 16), J.PIX_RGB24)
    assert all(st == 0 for _, _, st in res)
