"""tests/orient_model.py, the restatement of oriented output (include/jpezy_hip_orientation.h), held against itself and against an outside
implementation: the eight maps against the table's source-pixel column and against Pillow's ImageOps.exif_transpose on a non-square file,
and rect() against slicing orient() of an index image.  No GPU, no library: the library's own helpers are compared with this model in
tests/test_orient_abi.py."""
import io

import numpy as np
import pytest

import orient_model as OM

SIZES = [(1, 1), (1, 9), (7, 5), (33, 17)]


def index_image(W, H):
    """[H, W, 2]: every pixel holds its own (x, y)"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([xx, yy], axis=-1)


def windows(Wo, Ho):
    """the windows the GPU test takes, in a picture of Wo x Ho: whole, corners, odd origin, a column, a row, a left edge at x % 4 == 1"""
    out = [(0, 0, Wo, Ho), (0, 0, 1, 1), (Wo - 1, 0, 1, 1), (0, Ho - 1, 1, 1), (Wo - 1, Ho - 1, 1, 1), (Wo // 2, 0, 1, Ho), (0, Ho // 2, Wo, 1)]
    if Wo > 2 and Ho > 2:
        out.append((1, 1, Wo - 2, Ho - 2))
    if Wo > 5:
        out.append((5, 0, Wo - 5, Ho))
    if Wo > 1:
        out.append((1, 0, Wo - 1, Ho))
    return out


@pytest.mark.parametrize("W,H", SIZES)
def test_orient_is_the_tables_source_pixel(W, H):
    P = index_image(W, H)
    for o in OM.ORIENTATIONS:
        O = OM.orient(P, o)
        Wo, Ho = OM.size(o, W, H)
        assert O.shape == (Ho, Wo, 2), o
        for Y in range(Ho):
            for X in range(Wo):
                assert tuple(O[Y, X]) == OM.source_pixel(o, W, H, X, Y), (o, X, Y)
        assert np.array_equal(OM.orient(O, OM.INVERSE[o]), P), o


@pytest.mark.parametrize("W,H", SIZES)
def test_rect_is_what_slicing_the_oriented_index_image_shows(W, H):
    P = index_image(W, H)
    for o in OM.ORIENTATIONS:
        O = OM.orient(P, o)
        Wo, Ho = OM.size(o, W, H)
        for win in windows(Wo, Ho):
            x, y, w, h = win
            seen = O[y:y + h, x:x + w].reshape(-1, 2)
            sx, sy, sw, sh = OM.rect(o, W, H, win)
            assert (sw, sh) == ((w, h) if o < 5 else (h, w)), (o, win)
            assert (seen[:, 0].min(), seen[:, 1].min(), seen[:, 0].max(), seen[:, 1].max()) == (sx, sy, sx + sw - 1, sy + sh - 1), (o, win)
            assert {tuple(p) for p in seen} == {(a, b) for a in range(sx, sx + sw) for b in range(sy, sy + sh)}, (o, win)
            assert OM.window_of(o, W, H, (sx, sy, sw, sh)) == win, (o, win)


def test_the_eight_maps_are_pillows_exif_transpose():
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    rng = np.random.default_rng(3)
    P = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)               # 7 x 5
    for o in OM.ORIENTATIONS:
        exif = Image.Exif()
        exif[0x0112] = o
        buf = io.BytesIO()
        Image.fromarray(P).save(buf, "PNG", exif=exif)
        im = Image.open(io.BytesIO(buf.getvalue()))
        assert im.getexif().get(0x0112) == o
        got = np.asarray(ImageOps.exif_transpose(im))
        assert np.array_equal(got, OM.orient(P, o)), o


def test_the_fixture_builder_writes_what_pillow_reads():
    """the hand-built APP1 of the parser's tests is read by an independent reader, in both byte orders and every place"""
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(buf, "JPEG")
    for order in ("II", "MM"):
        for place in ("alone", "first", "last"):
            for o in OM.ORIENTATIONS:
                jpg = OM.tagged(buf.getvalue(), OM.app1(value=o, order=order, place=place))
                assert Image.open(io.BytesIO(jpg)).getexif().get(0x0112) == o, (order, place, o)
