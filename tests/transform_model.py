"""Test helper: a numpy restatement of the lossless transforms (include/jpezy_hip.h, LOSSLESS TRANSFORMS) on
[mcu][block][64] zig-zag int16 fields and on quantiser tables.  It shares no code with the product: blocks are taken to natural order,
moved as whole component planes of blocks with numpy indexing, and put back.

    op  name        output pixel (x', y') is source pixel   out size   swap mirror_x mirror_y
    0   NONE        (x', y')                                 W x H      0    0        0
    1   HFLIP       (W-1-x', y')                             W x H      0    1        0
    2   VFLIP       (x', H-1-y')                             W x H      0    0        1
    3   TRANSPOSE   (y', x')                                 H x W      1    0        0
    4   TRANSVERSE  (W-1-y', H-1-x')                         H x W      1    1        1
    5   ROT90       (y', H-1-x')                             H x W      1    0        1
    6   ROT180      (W-1-x', H-1-y')                         W x H      0    1        1
    7   ROT270      (W-1-y', x')                             H x W      1    1        0
"""
import numpy as np

NONE, HFLIP, VFLIP, TRANSPOSE, TRANSVERSE, ROT90, ROT180, ROT270 = range(8)
NAMES = ["none", "hflip", "vflip", "transpose", "transverse", "rot90", "rot180", "rot270"]
# (swap, mirror_x, mirror_y): which SOURCE axis is mirrored, whether the axes change places
OPS = [(0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0), (1, 1, 1), (1, 0, 1), (0, 1, 1), (1, 1, 0)]
S420, S444 = 0, 1
E_BADARG, E_UNSUPPORTED = -1, -4

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
               28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
               47, 55, 62, 63])                                   # zig-zag position -> natural index v * 8 + u


class Refused(Exception):
    def __init__(self, status, axis=None):
        super().__init__(f"status {status} ({axis})")
        self.status = status
        self.axis = axis


def mcu_px(sampling):
    return 8 if sampling == S444 else 16


def pixel_source(op, W, H):
    """(sx, sy) index arrays of shape (Hout, Wout): the source pixel of every output pixel"""
    swap, _, _ = OPS[op]
    Wo, Ho = (H, W) if swap else (W, H)
    yo, xo = np.meshgrid(np.arange(Ho), np.arange(Wo), indexing="ij")
    table = [(xo, yo), (W - 1 - xo, yo), (xo, H - 1 - yo), (yo, xo), (W - 1 - yo, H - 1 - xo), (yo, H - 1 - xo), (W - 1 - xo, H - 1 - yo),
             (W - 1 - yo, xo)]
    return table[op]


def pixel_op(img, op):
    """the operation on an array whose first two axes are (y, x)"""
    sx, sy = pixel_source(op, img.shape[1], img.shape[0])
    return img[sy, sx]


def geometry(op, W, H, sampling=S420, trim=False):
    """(Wout, Hout, C, R): output size and used source MCUs; Refused(E_UNSUPPORTED) for a mirrored axis with a partial MCU and no trim,
    Refused(E_BADARG) when trimming leaves nothing"""
    swap, mx, my = OPS[op]
    m = mcu_px(sampling)
    size = [W, H]
    for k, (mirrored, axis) in enumerate(((mx, "width"), (my, "height"))):
        if mirrored and size[k] % m:
            if not trim:
                raise Refused(E_UNSUPPORTED, axis)
            size[k] = size[k] // m * m
            if not size[k]:
                raise Refused(E_BADARG, axis)
    C, R = -(-size[0] // m), -(-size[1] // m)
    return (size[1], size[0], C, R) if swap else (size[0], size[1], C, R)


def block_rule(nat, op):
    """out[v][u] = s * in[vs][us] on arrays [..., 8, 8] in natural order (any dtype; int16 negation wraps: -32768 stays)"""
    swap, mx, my = OPS[op]
    v, u = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    vs, us = (u, v) if swap else (v, u)
    src = nat[..., vs, us]
    odd = ((mx * us + my * vs) & 1).astype(bool)
    return np.where(odd, np.negative(src), src).astype(nat.dtype)


def _planes(co, cols, rows, sampling):
    """[rows*cols, B, 64] zig-zag -> list of component planes [Gr, Gc, 8, 8] in natural order"""
    co = np.asarray(co, dtype=np.int16)
    B = 3 if sampling == S444 else 6
    f = co.reshape(rows, cols, B, 64)
    nat = np.zeros_like(f)
    nat[..., ZZ] = f
    nat = nat.reshape(rows, cols, B, 8, 8)
    if sampling == S444:
        return [nat[:, :, k] for k in range(3)]
    # luma block (bx, by) is block 2 * (by & 1) + (bx & 1) of MCU (bx >> 1, by >> 1)
    luma = nat[:, :, :4].reshape(rows, cols, 2, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(2 * rows, 2 * cols, 8, 8)
    return [luma, nat[:, :, 4], nat[:, :, 5]]


def _field(planes, sampling):
    """the inverse of _planes: [rows*cols, B, 64] zig-zag int16"""
    if sampling == S444:
        nat = np.stack(planes, axis=2)
    else:
        luma = planes[0]
        rows, cols = luma.shape[0] // 2, luma.shape[1] // 2
        quad = luma.reshape(rows, 2, cols, 2, 8, 8).transpose(0, 2, 1, 3, 4, 5).reshape(rows, cols, 4, 8, 8)
        nat = np.concatenate([quad, planes[1][:, :, None], planes[2][:, :, None]], axis=2)
    rows, cols, B = nat.shape[:3]
    return nat.reshape(rows, cols, B, 64)[..., ZZ].reshape(rows * cols, B, 64).astype(np.int16)


def transform_field(co, W, H, sampling, op, trim=False):
    """one frame's coefficients [mcu][block][64] (zig-zag int16) of a W x H picture -> (coefficients of the output, Wout, Hout)"""
    swap, mx, my = OPS[op]
    m = mcu_px(sampling)
    cols, rows = -(-W // m), -(-H // m)                            # the source buffer's own grid (its row pitch)
    Wout, Hout, C, R = geometry(op, W, H, sampling, trim)
    out = []
    for k, plane in enumerate(_planes(co, cols, rows, sampling)):
        f = 2 if (sampling == S420 and k == 0) else 1
        used = plane[:f * R, :f * C]                               # the used source MCUs
        Gr, Gc = used.shape[:2]
        byo, bxo = np.meshgrid(np.arange(Gc if swap else Gr), np.arange(Gr if swap else Gc), indexing="ij")
        sx, sy = (byo, bxo) if swap else (bxo, byo)
        if mx:
            sx = Gc - 1 - sx
        if my:
            sy = Gr - 1 - sy
        out.append(block_rule(used[sy, sx], op))
    return _field(out, sampling), Wout, Hout


def quant_table(op, table):
    """natural-order table of 64 -> the output file's: the transpose with swap"""
    t = np.asarray(table).reshape(8, 8)
    return (t.T if OPS[op][0] else t).reshape(64).copy()


def dct_matrix():
    """orthonormal 8-point DCT-II: F = D @ X @ D.T, F[v][u]"""
    k, n = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    D = np.cos((2 * n + 1) * k * np.pi / 16) * np.sqrt(2 / 8)
    D[0] /= np.sqrt(2)
    return D
