"""Test helper of tests/test_gpu_addressing.py: buffers whose frames, rows or planes lie gigabytes apart, filled and checked on the device.

A Surface is one buffer an entry reads or writes: per frame `rows` rows of `row_bytes` bytes, `row_stride` bytes apart, frames
`frame_stride` bytes apart -- a plane (row_stride = W), a packed image, one component of a YCbCr picture.  Outputs are filled with MARK and
compared ON THE DEVICE: a frame with the model's bytes through a strided view, the row padding and the gaps between and behind the frames
with MARK in chunks of CHUNK bytes, so that no temporary doubles the footprint and only the position of a first mismatch comes back to the
host.  Inputs are written through the same views, every frame with its index stamped into three of its first bytes.

A failure names the entry, the variant, the frame and the first differing byte offset, and states that offset modulo 2^31 and 2^32: a
wrapped address shows there as a small number, wrong arithmetic does not."""
import numpy as np

MARK = 0xA5
CHUNK = 1 << 28
SPLIT = 65535                                                      # frames per launch: the frame index is a grid dimension
FAR = (1 << 31) + 16                                               # a frame stride: frame 1 starts past 2 GiB, frame 2 past 4 GiB
TAIL = 64                                                          # marker bytes behind the last frame


def where(offset):
    return f"byte offset {offset} (mod 2^31 = {offset % (1 << 31)}, mod 2^32 = {offset % (1 << 32)})"


class Surface:
    def __init__(self, rows, row_bytes, row_stride=None, frame_stride=None):
        self.rows, self.row_bytes = int(rows), int(row_bytes)
        self.row_stride = int(row_stride) if row_stride else self.row_bytes
        assert self.row_stride >= self.row_bytes
        self.frame_bytes = (self.rows - 1) * self.row_stride + self.row_bytes
        self.frame_stride = int(frame_stride) if frame_stride else self.rows * self.row_stride
        assert self.frame_stride >= self.frame_bytes

    def size(self, n):
        """bytes of a buffer of n frames and the tail"""
        return (n - 1) * self.frame_stride + max(self.frame_bytes, self.frame_stride if n > 8 else 0) + TAIL

    def frame(self, buf, f):
        """the (rows, row_bytes) view of frame f"""
        return buf.as_strided((self.rows, self.row_bytes), (self.row_stride, 1), f * self.frame_stride)


def sample(n, seed=0, k=12):
    """frames 0 and n - 1, both sides of every launch split, and a seeded random dozen"""
    rng = np.random.default_rng(20261020 + seed + n)
    s = {0, n - 1} | {int(x) for x in rng.integers(0, n, k)}
    for f0 in range(SPLIT, n, SPLIT):
        s |= {f0 - 1, f0, f0 + 1}
    return sorted(f for f in s if 0 <= f < n)


# ---- the device side ----------------------------------------------------------------------------------------------------------------------
DEVICE = "cuda:0"


def fill(buf, value=MARK):
    flat = buf.view(-1)
    for lo in range(0, flat.numel(), CHUNK):
        flat[lo:lo + CHUNK].fill_(value)


def alloc(torch, surface, n):
    buf = torch.empty(surface.size(n), dtype=torch.uint8, device=DEVICE)
    fill(buf)
    return buf


def _first_true(bad):
    """flat index of the first True of a bool tensor, or None (argmax of equal maxima is the first of them)"""
    import torch
    flat = bad.reshape(-1)
    return int(flat.to(torch.uint8).argmax()) if bool(flat.any()) else None


def first_other(buf, lo, hi, value=MARK):
    """offset of the first byte of buf[lo:hi] that is not `value`, or None; one CHUNK at a time"""
    for a in range(lo, hi, CHUNK):
        k = _first_true(buf[a:min(a + CHUNK, hi)] != value)
        if k is not None:
            return a + k
    return None


def first_mismatch(got, want, rows=None):
    """got: any view of a device buffer; want: a tensor of got's shape, or one that broadcasts against it (same number of dimensions),
    or, with rows (a LongTensor over got's first dimension), a stack whose entry rows[i] is expected at got[i].  Compared along the
    first dimension in chunks of about CHUNK bytes -> None, or (index, byte offset in the buffer, got, want)"""
    per = max(1, got[0].numel() * got.element_size())
    step = max(1, CHUNK // per)
    for a in range(0, got.shape[0], step):
        b = min(a + step, got.shape[0])
        w = want[rows[a:b]] if rows is not None else (want[a:b] if want.shape[0] == got.shape[0] else want)
        part = got[a:b]
        k = _first_true(part != w)
        if k is not None:
            idx = [int(i) for i in np.unravel_index(k, tuple(part.shape))]
            value = int(w.expand_as(part)[tuple(idx)])
            idx[0] += a
            elems = got.storage_offset() + sum(i * s for i, s in zip(idx, got.stride()))
            return idx, elems * got.element_size(), int(got[tuple(idx)]), value
    return None


def first_difference(surface, buf, f, want):
    """frame f of the buffer against `want` (a device tensor (rows, row_bytes)), then its row padding against MARK -> None, or
    (byte offset in buf, got, want)"""
    s = surface
    bad = first_mismatch(s.frame(buf, f), want)
    if bad is not None:
        return bad[1:]
    pad = s.row_stride - s.row_bytes
    if pad and s.rows > 1:
        view = buf.as_strided((s.rows - 1, pad), (s.row_stride, 1), f * s.frame_stride + s.row_bytes)
        bad = first_mismatch(view, view.new_full((1, 1), MARK))
        if bad is not None:
            return bad[1:]
    return None


def check_frame(torch, who, surfaces, bufs, f, want):
    """want: one (rows, row_bytes) uint8 array per surface, the model's"""
    for k, (s, buf, w) in enumerate(zip(surfaces, bufs, want)):
        w = np.ascontiguousarray(w, np.uint8).reshape(s.rows, s.row_bytes)
        bad = first_difference(s, buf, f, torch.from_numpy(w).to(buf.device))
        assert bad is None, f"{who}: frame {f}, output {k}: first difference at {where(bad[0])}, got {bad[1]}, want {bad[2]}"


def check_gaps(who, surfaces, bufs, n, frames):
    """the bytes between each frame of `frames` and the next, and behind the last frame, are MARK"""
    for k, (s, buf) in enumerate(zip(surfaces, bufs)):
        for f in sorted(set(frames) | {n - 1}):
            lo = f * s.frame_stride + s.frame_bytes
            hi = (f + 1) * s.frame_stride if f < n - 1 else buf.numel()
            bad = first_other(buf, lo, hi)
            assert bad is None, f"{who}: output {k}: the byte behind frame {f} at {where(bad)} was written ({int(buf[bad])})"


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def stamped(arrays, f, stamp):
    """a copy of the frame's arrays with the frame index in the three stamp bytes; stamp: [(surface, byte of row 0)] * 3"""
    out = [np.array(a, np.uint8) for a in arrays]
    for k, (s, off) in enumerate(stamp):
        out[s][0, off] = (f >> (8 * k)) & 0xFF
    return out


def place_frames(torch, surfaces, sources, n, stamp):
    """n frames into fresh buffers: frame f is sources[f % len(sources)] (one (rows, row_bytes) array per surface) with f stamped.  Few
    frames are written one by one through their views; many (small) ones are gathered and stamped on the device."""
    K = len(sources)
    bufs = [alloc(torch, s, n) for s in surfaces]
    if n <= 8:
        for f in range(n):
            for s, buf, a in zip(surfaces, bufs, stamped(sources[f % K], f, stamp)):
                s.frame(buf, f).copy_(torch.from_numpy(a.reshape(s.rows, s.row_bytes)).to(buf.device))
        return bufs
    idx = torch.arange(n, device=DEVICE)
    for k, (s, buf) in enumerate(zip(surfaces, bufs)):
        base = np.full((K, s.frame_stride), MARK, np.uint8)
        for j in range(K):
            for r in range(s.rows):
                base[j, r * s.row_stride:r * s.row_stride + s.row_bytes] = np.asarray(sources[j][k]).reshape(s.rows, s.row_bytes)[r]
        frames = buf[:n * s.frame_stride].view(n, s.frame_stride)
        frames.copy_(torch.from_numpy(base).to(buf.device)[idx % K])
        for j, (sk, off) in enumerate(stamp):
            if sk == k:
                frames[:, off] = ((idx >> (8 * j)) & 0xFF).to(torch.uint8)
    return bufs


def stamp_field(field, f):
    """a copy of a coefficient field (flat int16) with the frame index in the first three coefficients of block 0"""
    out = np.array(field, np.int16).reshape(-1)
    out[0], out[1], out[2] = f % 61 - 30, f // 61 % 61 - 30, f // 3721 % 61 - 30
    return out


def place_fields(torch, fields, n, stamp=True):
    """[n, ncoef] int16 on the device: frame f is stamp_field(fields[f % K], f), or fields[f % K] as it is"""
    K = len(fields)
    idx = torch.arange(n, device=DEVICE)
    d = torch.from_numpy(np.stack([np.asarray(x, np.int16).reshape(-1) for x in fields])).to(DEVICE)[idx % K].contiguous()
    if not stamp:
        return d
    d[:, 0] = (idx % 61 - 30).to(torch.int16)
    d[:, 1] = (idx // 61 % 61 - 30).to(torch.int16)
    d[:, 2] = (idx // 3721 % 61 - 30).to(torch.int16)
    return d
