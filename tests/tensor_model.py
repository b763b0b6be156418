"""Restatement of include/jpezy_hip.h, BATCH OF WINDOWS, TENSOR OUTPUT, in numpy: what an element is for each element type, where it lies, and
which strides are admitted.  The conversions to binary16 and bfloat16 are written out in integer arithmetic on the bit patterns, so that
numpy's astype(float16) and torch's .to(bfloat16) remain independent implementations to compare against (tests/test_tensor_abi.py).  The
source bytes are tests/resize_model.py's; nothing here resamples."""
import numpy as np

DT_U8, DT_F32, DT_F16, DT_BF16 = 0, 1, 2, 3
ELEM_BYTES = {DT_U8: 1, DT_F32: 4, DT_F16: 2, DT_BF16: 2}
STORE = {DT_U8: np.uint8, DT_F32: np.uint32, DT_F16: np.uint16, DT_BF16: np.uint16}      # an element's bit pattern
E_BADARG, E_NOSPACE = -1, -6
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def normalization(mean, std):
    """scale[c] = (float)(1.0 / (255.0 * std[c])), bias[c] = (float)(-mean[c] / std[c]), binary64 with every operation separate"""
    scale = np.array([np.float32(1.0 / (255.0 * float(s))) for s in std], np.float32)
    bias = np.array([np.float32(-float(m) / float(s)) for m, s in zip(mean, std)], np.float32)
    return scale, bias


def value_in_band(v):
    v = float(np.float32(v))
    return v == 0.0 or (np.isfinite(v) and 2.0 ** -100 <= abs(v) <= 2.0 ** 100)


def affine(b, scale, bias):
    """v = (float)b * scale + bias in binary32: numpy rounds the product and the sum separately"""
    prod = np.asarray(b).astype(np.float32) * np.float32(scale)
    return (prod + np.float32(bias)).astype(np.float32)


def f16_bits(v):
    """binary32 -> binary16 bit patterns: round to nearest even, subnormals kept, overflow to inf (no NaN comes in)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    a = u & 0x7FFFFFFF
    # normal results: rebias the exponent (127 -> 15) and round the 13 bits that go; a carry runs into the exponent, as it should
    r = a - (112 << 23)
    normal = (r + 0xFFF + ((r >> 13) & 1)) >> 13
    normal = np.minimum(normal, 0x7C00)                             # 65520 and above: inf
    # subnormal results, |v| < 2^-14: the 24-bit significand m * 2^(e - 150) in units of 2^-24 is m >> (126 - e)
    e = a >> 23
    m = (a & 0x7FFFFF) | np.where(e > 0, 0x800000, 0)
    s = np.clip(126 - e, 1, 26)                                     # (e <= 112 here, so s >= 14; from 25 on the result is 0)
    q = m >> s
    rem = m & ((np.int64(1) << s) - 1)
    half = np.int64(1) << (s - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    sub = np.where(126 - e >= 25, 0, q)
    return (sign | np.where(a >= 0x38800000, normal, sub)).astype(np.uint16)


def bf16_bits(v):
    """the upper 16 bits of u + 0x7FFF + ((u >> 16) & 1)"""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def elements(b, dt, scale=1.0, bias=0.0):
    """the bit patterns (STORE[dt]) of the bytes b of ONE channel"""
    b = np.asarray(b, np.uint8)
    if dt == DT_U8:
        return b.copy()
    v = affine(b, scale, bias)
    if dt == DT_F32:
        return v.view(np.uint32).copy()
    return f16_bits(v) if dt == DT_F16 else bf16_bits(v)


def layout_status(extents, strides, cap_elems):
    """0, E_BADARG (a negative stride; strides that give two index tuples one element) or E_NOSPACE; extents and strides (n, C, H, W)"""
    if any(s < 0 for s in strides):
        return E_BADARG
    need = 1
    for s, e in sorted((s, e) for s, e in zip(strides, extents) if e > 1):
        if s < need:
            return E_BADARG
        need = s * e
    return 0 if sum((e - 1) * s for s, e in zip(strides, extents)) + 1 <= cap_elems else E_NOSPACE


def place(buf, base_elem, strides, k, img, dt, channels, scale=None, bias=None):
    """file k's elements into buf (a numpy array of STORE[dt], the tensor's storage counted in elements): img is the file's [H, W, 3] source
    bytes, element (k, c, y, x) goes to base_elem + k*sn + c*sc + y*sh + x*sw"""
    sn, sc, sh, sw = strides
    H, W = img.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    for c in range(channels):
        e = elements(img[:, :, c], dt, 1.0 if scale is None else scale[c], 0.0 if bias is None else bias[c])
        buf[base_elem + k * sn + c * sc + yy * sh + xx * sw] = e
