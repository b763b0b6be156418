"""Test helper: the numpy restatement of oriented output (include/jpezy_hip_orientation.h) and the fixtures its tests share.

The rule is a permutation of the pixels of the picture P the existing decode returns: O = orient(P, o) for the eight values of the EXIF
Orientation tag.  orient() is written with numpy's own flips, rot90 and transpose, exactly as the definition's table names them;
source_pixel() is the table's third column; rect() maps a window of O to the rectangle of P it shows.  tests/test_orient_model.py holds the
three against each other, against an index image, and against Pillow's ImageOps.exif_transpose.

Fixtures: app1() builds an APP1 segment by hand (both byte orders, the tag first, last or alone in IFD0, and every way of being wrong the
parser's tests need), tagged() puts a segment behind SOI of any .jpg."""
import struct

import numpy as np

ORIENTATIONS = range(1, 9)
INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}       # orient(orient(P, o), INVERSE[o]) is P


def orient(P, o):
    """P: [H, W] or [H, W, C]"""
    if o == 1:
        return P
    if o == 2:
        return P[:, ::-1]
    if o == 3:
        return P[::-1, ::-1]
    if o == 4:
        return P[::-1]
    axes = (1, 0) + tuple(range(2, P.ndim))
    if o == 5:
        return P.transpose(axes)
    if o == 6:
        return np.rot90(P, -1)
    if o == 7:
        return P[::-1, ::-1].transpose(axes)
    if o == 8:
        return np.rot90(P, 1)
    raise ValueError(o)


def size(o, W, H):
    return (W, H) if o < 5 else (H, W)


def source_pixel(o, W, H, X, Y):
    """(x, y) in P (W x H) of pixel (X, Y) of orient(P, o): the table's third column"""
    return {1: (X, Y), 2: (W - 1 - X, Y), 3: (W - 1 - X, H - 1 - Y), 4: (X, H - 1 - Y), 5: (Y, X), 6: (Y, H - 1 - X), 7: (W - 1 - Y, H - 1 - X),
            8: (W - 1 - Y, X)}[o]


def rect(o, W, H, region):
    """the rectangle of P (W x H) that the window (x, y, w, h) of orient(P, o) shows: the bounding box of its corners' source pixels"""
    x, y, w, h = region
    a = source_pixel(o, W, H, x, y)
    b = source_pixel(o, W, H, x + w - 1, y + h - 1)
    x0, x1 = sorted((a[0], b[0]))
    y0, y1 = sorted((a[1], b[1]))
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


def window_of(o, W, H, source):
    """the inverse of rect(): the window of orient(P, o) that shows the rectangle `source` of P"""
    Wo, Ho = size(o, W, H)
    return rect(INVERSE[o], Wo, Ho, source)


# ---- fixtures: an APP1 segment built by hand --------------------------------------------------------------------------------------------
def tiff(value=6, order="II", place="alone", tag=0x0112, typ=3, count=1, magic=42, ifd=8, n_entries=None):
    """a TIFF structure with one IFD.  place: the orientation entry 'alone', 'first' or 'last' among two others; typ 3 = SHORT, 4 = LONG,
    2 = ASCII; n_entries: the count the IFD claims (default: what it holds); ifd: the offset the header claims"""
    e = "<" if order == "II" else ">"
    def entry(t, ty, n, v):
        field = struct.pack(e + "H", v & 0xFFFF) + b"\0\0" if ty == 3 else struct.pack(e + "I", v & 0xFFFFFFFF)
        return struct.pack(e + "HHI", t, ty, n) + field
    mine = entry(tag, typ, count, value)
    others = [entry(0x011A, 4, 1, 72), entry(0x0128, 3, 1, 2)]       # XResolution (as a LONG, for the fixture's sake), ResolutionUnit
    entries = {"alone": [mine], "first": [mine] + others, "last": others + [mine]}[place]
    head = (b"II" if order == "II" else b"MM") + struct.pack(e + "HI", magic, ifd)
    return head + struct.pack(e + "H", len(entries) if n_entries is None else n_entries) + b"".join(entries) + struct.pack(e + "I", 0)


def app1(payload=None, ident=b"Exif\0\0", length=None, **kw):
    """the APP1 segment: marker, length (default: the true one), identifier, payload (default: tiff(**kw))"""
    body = ident + (tiff(**kw) if payload is None else payload)
    return b"\xff\xe1" + struct.pack(">H", len(body) + 2 if length is None else length) + body


def tagged(jpg, segment):
    """segment (or several, concatenated) behind SOI of the .jpg"""
    jpg = bytes(jpg)
    assert jpg[:2] == b"\xff\xd8"
    return jpg[:2] + segment + jpg[2:]
