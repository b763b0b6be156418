"""The fixed table of calls behind tests/golden/fused_entry_errors.json: the encoder's entries of the C-ABI and the three fused decode
entries of the project's own layout, fifteen in all, driven through bare ctypes -- with a null context (the checks that come before
the context; runs without a GPU) and with a real one.  tools/gen/record_fused_entry_errors.py records (entry, case, status, last_error
text, and for a call that succeeds the SHA-256 of every buffer it may write) from a build of the commit BEFORE a change of the host
layer; tests/test_fused_entry_errors.py replays the table against the build under test.  The twin of tests/decode_entry_table.py.

A row is (entry, case, overrides): the call is the entry's good argument list (Env.call) with `overrides` applied.  Overrides named
variant / avg / chunk are settings of the context, made before the call and put back after it; they need a real context."""
import ctypes as C
import hashlib

import numpy as np

W, H = 40, 24
BANDED = (90, 110)               # 9900 pixels: more than twice the 4096-byte chunk at one byte per pixel, ragged in both directions
S420, S444, S422 = 0, 1, 3
MAX_COMMENT = 396                # JPEZY_MAX_COMMENT

PLANAR_IN = ["fdct_quant", "fdct_quant_dev", "fdct_quant_sampling_dev", "encode_jpeg", "encode_jpeg_sampling"]
PACKED_IN = ["fdct_quant_packed_dev", "fdct_quant_sampling_packed_dev", "encode_jpeg_packed", "encode_jpeg_sampling_packed"]
YCC_IN = ["fdct_quant_ycc_dev", "encode_jpeg_ycc"]
DECODE = ["dequant_idct", "dequant_idct_dev", "dequant_idct_packed_dev", "dequant_idct_ycc_dev"]
ENTRIES = PLANAR_IN + PACKED_IN + YCC_IN + DECODE
HOST = ["fdct_quant", "dequant_idct", "encode_jpeg", "encode_jpeg_packed", "encode_jpeg_ycc", "encode_jpeg_sampling", "encode_jpeg_sampling_packed"]
FILE = [e for e in ENTRIES if e.startswith("encode_jpeg")]
DEV = [e for e in ENTRIES if e not in HOST]
SETTINGS = ("variant", "avg", "chunk")

# the pointer arguments of every entry, by the names Env.call gives them
POINTERS = {
    "fdct_quant": ("r", "g", "b", "co"), "dequant_idct": ("co", "qt", "comp_tq", "r", "g", "b"),
    "fdct_quant_dev": ("r", "g", "b", "co"), "fdct_quant_sampling_dev": ("r", "g", "b", "co"),
    "fdct_quant_packed_dev": ("pix", "co"), "fdct_quant_sampling_packed_dev": ("pix", "co"),
    "fdct_quant_ycc_dev": ("y", "cb", "cr", "co"),
    "encode_jpeg": ("r", "g", "b", "out"), "encode_jpeg_sampling": ("r", "g", "b", "out"),
    "encode_jpeg_packed": ("pix", "out"), "encode_jpeg_sampling_packed": ("pix", "out"),
    "encode_jpeg_ycc": ("y", "cb", "cr", "out"),
    "dequant_idct_dev": ("co", "qt", "comp_tq", "r", "g", "b"), "dequant_idct_packed_dev": ("co", "qt", "comp_tq", "pix"),
    "dequant_idct_ycc_dev": ("co", "qt", "comp_tq", "y"),
}


def _has(entry, arg):
    """whether the entry has this argument"""
    if arg == "n_frames":
        return entry not in FILE
    if arg == "gray":
        return entry != "dequant_idct_ycc_dev"
    if arg == "plane_stride":
        return entry in ("fdct_quant_dev", "fdct_quant_sampling_dev", "dequant_idct_dev")
    if arg in ("format", "row_stride"):
        return "packed" in entry
    if arg == "frame_stride":
        return "packed" in entry and entry in DEV
    if arg in ("y_stride", "c_stride", "c_step"):
        return "ycc" in entry
    if arg in ("y_frame_stride", "c_frame_stride"):
        return "ycc" in entry and entry in DEV
    if arg == "sampling":
        return "sampling" in entry
    if arg == "comment":
        return entry in FILE
    raise KeyError(arg)


def _bad_rows():
    """one bad argument at a time, then two for every pair of neighbouring checks; no setting of the context"""
    rows = []
    add = lambda entry, case, **over: rows.append((entry, case, over))
    for e in ENTRIES:
        add(e, "none_bad")
        for p in POINTERS[e]:
            add(e, "null_" + p, **{p: None})
        add(e, "w_0", W=0)
        add(e, "h_65536", H=65536)
        if e in DEV:
            add(e, "misaligned_coeffs", co="misaligned")
        if _has(e, "n_frames"):
            add(e, "n_frames_0", n_frames=0)
        if _has(e, "plane_stride"):
            add(e, "plane_stride_small", plane_stride=W * H - 1)
        if _has(e, "format"):
            add(e, "bad_format", format=7)
            add(e, "negative_format", format=-1)
            add(e, "row_stride_small", row_stride=W * 3 - 1)
            add(e, "row_stride_past_32_bits", row_stride=(1 << 32) // H + 1)
        if _has(e, "frame_stride"):
            add(e, "frame_stride_small", format=2, row_stride=W * 4 + 4, frame_stride=(H - 1) * (W * 4 + 4) + W * 4 - 1, n_frames=2)
        if _has(e, "c_step"):
            add(e, "c_step_0", c_step=0)
            add(e, "c_step_3", c_step=3)
            add(e, "y_stride_small", y_stride=W - 1)
            add(e, "c_stride_small", c_stride=W // 2 - 1)
            add(e, "c_stride_small_interleaved", c_step=2, cr="cb+1", c_stride=W - 2)
            add(e, "y_stride_past_32_bits", y_stride=(1 << 32) // H + 1)
            add(e, "c_stride_past_32_bits", c_stride=(1 << 32) // (H // 2) + 1)
        if _has(e, "y_frame_stride"):
            add(e, "y_frame_stride_small", y_frame_stride=W * H - 1, n_frames=2)
            add(e, "c_frame_stride_small", c_frame_stride=(W // 2) * (H // 2) - 1, n_frames=2)
        if _has(e, "sampling"):
            for s in (2, 4, -1):
                add(e, f"sampling_{s}", sampling=s)
            add(e, "gray_444", sampling=S444, gray=1)
            add(e, "gray_422", sampling=S422, gray=1)
            # forwarded at 4:2:0: the plain entry's checks, order and texts
            add(e, "forwarded_null_first", sampling=S420, **{POINTERS[e][0]: None})
            add(e, "forwarded_null_last", sampling=S420, **{POINTERS[e][-1]: None})
            if e in DEV:
                add(e, "forwarded_misaligned", sampling=S420, co="misaligned")
            if _has(e, "plane_stride"):
                add(e, "forwarded_plane_stride_small", sampling=S420, plane_stride=W * H - 1)
            if _has(e, "format"):
                add(e, "forwarded_bad_format", sampling=S420, format=7)
            if _has(e, "comment"):
                add(e, "forwarded_long_comment", sampling=S420, comment=b"c" * (MAX_COMMENT + 1))
        if _has(e, "comment"):
            add(e, "long_comment", comment=b"c" * (MAX_COMMENT + 1))
            add(e, "longest_comment", comment=b"c" * MAX_COMMENT)
    # two bad arguments: which check wins
    for e in ("fdct_quant_dev", "fdct_quant_sampling_dev"):
        add(e, "n_frames_0_and_w_0", n_frames=0, W=0)
        add(e, "w_0_and_null_r", W=0, r=None)
        add(e, "null_r_and_misaligned", r=None, co="misaligned")
        add(e, "misaligned_and_plane_stride_small", co="misaligned", plane_stride=W * H - 1)
    add("fdct_quant_sampling_dev", "n_frames_0_and_sampling_2", n_frames=0, sampling=2)
    add("fdct_quant_sampling_dev", "sampling_4_and_gray", sampling=4, gray=1)
    add("fdct_quant_sampling_dev", "gray_444_and_null_r", sampling=S444, gray=1, r=None)
    for e in ("fdct_quant_packed_dev", "fdct_quant_sampling_packed_dev", "dequant_idct_packed_dev"):
        add(e, "n_frames_0_and_bad_format", n_frames=0, format=7)
        add(e, "bad_format_and_row_stride_small", format=7, row_stride=1)
        add(e, "row_stride_small_and_past_32_bits", W=65535, H=65535, row_stride=70000)
        add(e, "frame_stride_small_and_null_pix", frame_stride=1, pix=None)
        add(e, "null_pix_and_misaligned", pix=None, co="misaligned")
    add("fdct_quant_sampling_packed_dev", "h_65536_and_sampling_-1", H=65536, sampling=-1)
    add("fdct_quant_sampling_packed_dev", "sampling_2_and_gray", sampling=2, gray=1)
    add("fdct_quant_sampling_packed_dev", "gray_422_and_bad_format", sampling=S422, gray=1, format=7)
    for e in ("fdct_quant_ycc_dev", "dequant_idct_ycc_dev", "encode_jpeg_ycc"):
        add(e, "w_0_and_c_step_3", W=0, c_step=3)
        add(e, "c_step_3_and_y_stride_small", c_step=3, y_stride=1)
        add(e, "y_stride_small_and_c_stride_small", y_stride=1, c_stride=1)
        add(e, "c_stride_small_and_past_32_bits", c_stride=1, y_stride=(1 << 32) // H + 1)
        add(e, "c_stride_small_and_null_y", c_stride=1, y=None)
    for e in ("fdct_quant_ycc_dev", "dequant_idct_ycc_dev"):
        add(e, "past_32_bits_and_y_frame_stride_small", c_stride=(1 << 32) // (H // 2) + 1, y_frame_stride=1)
        add(e, "y_frame_stride_small_and_c_frame_stride_small", y_frame_stride=1, c_frame_stride=1)
        add(e, "c_frame_stride_small_and_null_y", c_frame_stride=1, y=None)
        add(e, "null_co_and_n_frames_0", co=None, n_frames=0)
        add(e, "n_frames_0_and_misaligned", n_frames=0, co="misaligned")
    add("fdct_quant_ycc_dev", "gray_null_cb_and_n_frames_0", gray=1, cb=None, cr=None, n_frames=0)
    add("dequant_idct_ycc_dev", "null_qt_and_n_frames_0", qt=None, n_frames=0)
    add("fdct_quant", "w_0_and_null_r", W=0, r=None)
    add("fdct_quant", "n_frames_0_and_null_co", n_frames=0, co=None)
    add("dequant_idct", "w_0_and_null_qt", W=0, qt=None)
    add("dequant_idct", "n_frames_0_and_null_b", n_frames=0, b=None)
    for e in ("dequant_idct_dev",):
        add(e, "n_frames_0_and_null_qt", n_frames=0, qt=None)
        add(e, "null_b_and_misaligned", b=None, co="misaligned")
        add(e, "misaligned_and_plane_stride_small", co="misaligned", plane_stride=W * H - 1)
    add("dequant_idct_packed_dev", "null_comp_tq_and_misaligned", comp_tq=None, co="misaligned")
    long = b"c" * (MAX_COMMENT + 1)
    for e in ("encode_jpeg", "encode_jpeg_sampling"):
        add(e, "h_65536_and_null_out", H=65536, out=None)
        add(e, "null_r_and_long_comment", r=None, comment=long)
    add("encode_jpeg_sampling", "w_0_and_sampling_-1", W=0, sampling=-1)
    add("encode_jpeg_sampling", "sampling_2_and_gray", sampling=2, gray=1)
    add("encode_jpeg_sampling", "gray_422_and_null_r", sampling=S422, gray=1, r=None)
    for e in ("encode_jpeg_packed", "encode_jpeg_sampling_packed"):
        add(e, "w_0_and_bad_format", W=0, format=7)
        add(e, "row_stride_small_and_null_pix", row_stride=1, pix=None)
        add(e, "null_out_and_long_comment", out=None, comment=long)
    add("encode_jpeg_sampling_packed", "w_0_and_sampling_4", W=0, sampling=4)
    add("encode_jpeg_sampling_packed", "gray_444_and_bad_format", sampling=S444, gray=1, format=7)
    add("encode_jpeg_ycc", "null_cb_and_long_comment", cb=None, comment=long)
    add("encode_jpeg_ycc", "gray_null_chroma_and_long_comment", gray=1, cb=None, cr=None, comment=long)
    return rows


def _setting_rows():
    """what needs a real context: the variant refusals against their neighbours, and every call that succeeds"""
    rows = []
    add = lambda entry, case, **over: rows.append((entry, case, over))
    long = b"c" * (MAX_COMMENT + 1)
    for e in PLANAR_IN + PACKED_IN + YCC_IN:
        samplings = (S420, S444, S422) if _has(e, "sampling") else (S420,)
        for s in samplings:
            tag = {S420: "", S444: "_444", S422: "_422"}[s] if _has(e, "sampling") else ""
            tag = "_420" if _has(e, "sampling") and s == S420 else tag
            over = dict(sampling=s) if _has(e, "sampling") else {}
            # every combination, refused ones included: variant 0 with 4:4:4, with 4:2:2, and with averaging where it acts
            for gray in ((0, 1) if s == S420 else (0,)):
                for avg in (0, 1):
                    for variant in (0, 1):
                        add(e, f"combo{tag}_{'gray' if gray else 'colour'}_{'avg' if avg else 'point'}_v{variant}", gray=gray, avg=avg,
                            variant=variant, **over)
            # the variant refusal against the checks on both sides of it
            bad_v = dict(variant=0, avg=1, **over)
            last = POINTERS[e][-1]
            if e in YCC_IN:
                continue
            add(e, f"variant_0{tag}_and_null_{last}", **bad_v, **{last: None})
            add(e, f"variant_0{tag}_and_null_{POINTERS[e][0]}", **bad_v, **{POINTERS[e][0]: None})
            if e in DEV:
                add(e, f"variant_0{tag}_and_misaligned", **bad_v, co="misaligned")
            if _has(e, "plane_stride"):
                add(e, f"variant_0{tag}_and_plane_stride_small", **bad_v, plane_stride=W * H - 1)
            if _has(e, "format"):
                add(e, f"variant_0{tag}_and_bad_format", **bad_v, format=7)
                add(e, f"variant_0{tag}_and_row_stride_small", **bad_v, row_stride=1)
            if _has(e, "comment"):
                add(e, f"variant_0{tag}_and_long_comment", **bad_v, comment=long)
            if _has(e, "sampling") and s != S420:
                add(e, f"variant_0{tag}_and_gray", **bad_v, gray=1)
    for e in ENTRIES:
        if _has(e, "n_frames"):
            add(e, "ok_two_frames", n_frames=2)
        if _has(e, "plane_stride"):
            add(e, "ok_two_frames_odd_stride", n_frames=2, plane_stride=W * H + 3)
            if _has(e, "sampling"):
                add(e, "ok_444_two_frames_odd_stride", n_frames=2, plane_stride=W * H + 3, sampling=S444)
                add(e, "ok_422_two_frames_odd_stride", n_frames=2, plane_stride=W * H + 3, sampling=S422, avg=1)
        if _has(e, "format"):
            for fmt, name in enumerate(("rgb", "bgr", "rgba", "bgra")):
                nb = 3 if fmt < 2 else 4
                over = dict(frame_stride=H * (W * nb + 5) + 7, n_frames=2) if _has(e, "frame_stride") else {}
                for s in ((S420, S444, S422) if _has(e, "sampling") else (S420,)):
                    so = dict(sampling=s) if _has(e, "sampling") else {}
                    add(e, f"ok_{name}_wide_rows_s{s}", format=fmt, row_stride=W * nb + 5, **over, **so)
                    add(e, f"ok_{name}_tight_avg_s{s}", format=fmt, avg=1, **so)
                    add(e, f"ok_{name}_tight_v0_s{s}", format=fmt, variant=0, **so)
                if e not in DECODE:
                    add(e, f"ok_{name}_gray", format=fmt, gray=1, **({"sampling": S420} if _has(e, "sampling") else {}))
        if _has(e, "c_step"):
            two = dict(n_frames=2, y_frame_stride=H * (W + 3) + 5, c_frame_stride=(H // 2) * (W + 4) + 3) if _has(e, "y_frame_stride") else {}
            add(e, "ok_wide_rows", y_stride=W + 3, c_stride=W // 2 + 1, **two)
            add(e, "ok_interleaved", c_step=2, cr="cb+1", **two)
            add(e, "ok_interleaved_cr_first", c_step=2, cb="cr+1")
            add(e, "ok_interleaved_wide_rows", c_step=2, cr="cb+1", c_stride=W + 4, y_stride=W + 3, **two)
            add(e, "ok_step_2_apart", c_step=2)
            if e in YCC_IN:
                add(e, "ok_gray_null_chroma", gray=1, cb=None, cr=None)
                add(e, "ok_gray_null_chroma_two_frames", gray=1, cb=None, cr=None, **two)
                add(e, "ok_interleaved_v0", c_step=2, cr="cb+1", variant=0)
            else:
                add(e, "ok_luma_only", cb=None, cr=None, **two)
        if e in DECODE and _has(e, "gray"):
            add(e, "ok_gray", gray=1)
            add(e, "ok_gray_two_frames", gray=1, n_frames=2)
        if _has(e, "comment"):
            add(e, "ok_no_comment", comment=None)
            add(e, "cap_short", cap="short")
            if not _has(e, "sampling"):
                add(e, "cap_short_gray", cap="short", gray=1)
            else:
                add(e, "cap_short_444", cap="short", sampling=S444)
                add(e, "cap_short_422", cap="short", sampling=S422)
            add(e, "cap_0", cap=0)
        if e in HOST:
            # several ragged bands of every kind (the 4:4:4 and 4:2:2 entries: the whole frame in one piece)
            big = dict(W=BANDED[0], H=BANDED[1], chunk=4096)
            banded = dict(big, sampling=S420) if _has(e, "sampling") else big
            for gray in ((0, 1) if _has(e, "gray") else (0,)):
                name = "ok_banded_gray" if gray else "ok_banded"
                add(e, name, gray=gray, **banded)
                if e not in DECODE:
                    add(e, name + "_avg", gray=gray, avg=1, **banded)
                    add(e, name + "_v0", gray=gray, variant=0, **banded)
                if _has(e, "c_step"):
                    add(e, name + "_interleaved", gray=gray, c_step=2, cr="cb+1", **banded)
                    add(e, name + "_wide_rows", gray=gray, y_stride=BANDED[0] + 7, c_stride=BANDED[0] // 2 + 3, **banded)
                if _has(e, "format"):
                    add(e, name + "_bgra_wide_rows", gray=gray, format=3, row_stride=BANDED[0] * 4 + 9, **banded)
                if _has(e, "n_frames"):
                    add(e, name + "_two_frames", gray=gray, n_frames=2, **banded)
            if _has(e, "sampling"):
                for s in (S444, S422):
                    add(e, f"ok_banded_s{s}", sampling=s, **big)
                    add(e, f"ok_banded_s{s}_avg", sampling=s, avg=1, **big)
                    if _has(e, "format"):
                        add(e, f"ok_banded_s{s}_bgra_wide_rows", sampling=s, format=3, row_stride=BANDED[0] * 4 + 9, **big)
            add(e, "whole_frames_per_chunk", chunk=4096, **({"n_frames": 2} if _has(e, "n_frames") else {}))
    # the FP64 kernel has no 4:4:4 / 4:2:2 form: what the loops above named ok_... is a refusal there
    refused = lambda e, over: _has(e, "sampling") and over.get("variant") == 0 and over.get("sampling", S444) != S420
    return [(e, "refused" + case[2:] if case.startswith("ok") and refused(e, over) else case, over) for e, case, over in rows]


def table(half):
    """half: "null_context" or "real_context" -> [(entry, case, overrides)]"""
    return _bad_rows() if half == "null_context" else _bad_rows() + _setting_rows()


class Env:
    """Buffers and the calls themselves.  ctx None: the null-context half (host memory everywhere; every call is refused before
    anything is read or written).  With a context the device entries get device memory from torch.  Inputs are seeded noise, large
    enough for every layout of the table; outputs are refilled with 0x5A before every call, and a succeeding call's SHA-256 is taken
    over all of them."""
    IN_BYTES = 1 << 17
    OUT_BYTES = 1 << 19

    def __init__(self, J, ctx=None):
        self.J, self.lib, self.ctx = J, J.load_library(), ctx
        rng = np.random.default_rng(2024)
        self.src = [rng.integers(0, 256, self.IN_BYTES, dtype=np.uint8) for _ in range(3)]
        co = np.zeros(self.IN_BYTES // 2, np.int16)
        mask = rng.random(co.size) < 0.2
        co[mask] = rng.integers(-30, 31, int(mask.sum()))
        co[::64] = rng.integers(-60, 61, co.size // 64)
        self.co = co
        self.out = [np.full(self.OUT_BYTES, 0x5A, np.uint8) for _ in range(3)]
        self.qt = J.api.annex_k_tables().qt
        self.dev = None
        if ctx is not None:
            import torch
            dev = torch.device("cuda", self.lib.jpezy_ctx_device(ctx))
            self.dev = dict(src=[torch.from_numpy(s).to(dev) for s in self.src], co=torch.from_numpy(co).to(dev),
                            out=[torch.full((self.OUT_BYTES,), 0x5A, dtype=torch.uint8, device=dev) for _ in range(3)])
            torch.cuda.synchronize()

    def _settings(self, variant=1, avg=0, chunk=4 << 20):
        assert self.lib.jpezy_ctx_set_variant(self.ctx, variant) == 0
        assert self.lib.jpezy_ctx_set_chroma_downsampling(self.ctx, avg) == 0
        self.lib.jpezy_ctx_set_host_chunk_bytes(self.ctx, chunk)

    def _args(self, entry, a):
        c, s = self.ctx, None
        planar = [a["r"], a["g"], a["b"]]
        packed = [a["pix"], a["format"], a["row_stride"]]
        ycc = [a["y"], a["y_stride"], a["cb"], a["cr"], a["c_stride"], a["c_step"]]
        dec = [a["co"], a["qt"], a["comp_tq"]]
        tail_file = [a["comment"], a["out"], a["cap"]]
        whg = [a["W"], a["H"], a["gray"]]
        return {
            "fdct_quant": lambda: [c, *planar, *whg, a["n_frames"], a["co"]],
            "dequant_idct": lambda: [c, *dec, *whg, a["n_frames"], *planar],
            "fdct_quant_dev": lambda: [c, *planar, a["plane_stride"], *whg, a["n_frames"], a["co"], s],
            "fdct_quant_sampling_dev": lambda: [c, *planar, a["plane_stride"], a["W"], a["H"], a["sampling"], a["gray"], a["n_frames"], a["co"], s],
            "fdct_quant_packed_dev": lambda: [c, *packed, a["frame_stride"], *whg, a["n_frames"], a["co"], s],
            "fdct_quant_sampling_packed_dev": lambda: [c, *packed, a["frame_stride"], a["W"], a["H"], a["sampling"], a["gray"], a["n_frames"], a["co"], s],
            "fdct_quant_ycc_dev": lambda: [c, *ycc, a["y_frame_stride"], a["c_frame_stride"], *whg, a["n_frames"], a["co"], s],
            "encode_jpeg": lambda: [c, *planar, *whg, *tail_file],
            "encode_jpeg_sampling": lambda: [c, *planar, a["W"], a["H"], a["sampling"], a["gray"], *tail_file],
            "encode_jpeg_packed": lambda: [c, *packed, *whg, *tail_file],
            "encode_jpeg_sampling_packed": lambda: [c, *packed, a["W"], a["H"], a["sampling"], a["gray"], *tail_file],
            "encode_jpeg_ycc": lambda: [c, *ycc, *whg, *tail_file],
            "dequant_idct_dev": lambda: [c, *dec, a["plane_stride"], *whg, a["n_frames"], *planar, s],
            "dequant_idct_packed_dev": lambda: [c, *dec, a["format"], a["row_stride"], a["frame_stride"], *whg, a["n_frames"], a["pix"], s],
            "dequant_idct_ycc_dev": lambda: [c, *dec, *ycc, a["y_frame_stride"], a["c_frame_stride"], a["W"], a["H"], a["n_frames"], s],
        }[entry]()

    def call(self, entry, over):
        """-> (status, sha256 of the output buffers or None): the entry's good arguments with `over` applied"""
        over = dict(over)
        settings = {k: over.pop(k) for k in SETTINGS if k in over}
        on_dev = self.ctx is not None and entry in DEV
        if on_dev:
            src, co, out = ([t.data_ptr() for t in self.dev["src"]], self.dev["co"].data_ptr(), [t.data_ptr() for t in self.dev["out"]])
            for t in self.dev["out"]:
                t.fill_(0x5A)
        else:
            src, co, out = ([s.ctypes.data for s in self.src], self.co.ctypes.data, [o.ctypes.data for o in self.out])
            for o in self.out:
                o.fill(0x5A)
        decode = entry in DECODE
        pixels = out if decode else src                 # the decoders write pixels and read coefficients; the encoders the other way round
        keep = [(C.c_uint8 * 3)(0, 1, 1)]
        w, h = over.get("W", W), over.get("H", H)
        a = dict(r=pixels[0], g=pixels[1], b=pixels[2], pix=pixels[0], y=pixels[0], cb=pixels[1], cr=pixels[2],
                 co=co if decode else out[0], out=out[0], qt=C.pointer(self.qt), comp_tq=C.pointer(keep[0]),
                 W=W, H=H, gray=0, n_frames=1, sampling=S444, plane_stride=w * h if 0 < w * h < self.IN_BYTES else W * H,
                 format=0, row_stride=0, frame_stride=0, y_stride=0, c_stride=0, c_step=1, y_frame_stride=0, c_frame_stride=0,
                 comment=b"fused entry table", cap=None)
        a.update(over)
        if a["co"] == "misaligned":
            a["co"] = (co if decode else out[0]) + 2
        if a["cr"] == "cb+1":
            a["cr"] = a["cb"] + 1
        if a["cb"] == "cr+1":
            a["cb"], a["cr"] = pixels[1] + 1, pixels[1]
        if entry in FILE and (a["cap"] is None or a["cap"] == "short"):
            s = a["sampling"] if _has(entry, "sampling") and a["sampling"] in (S420, S444, S422) else S420
            bound = self.lib.jpezy_jpeg_bound_sampling(a["W"], a["H"], s) if (a["W"], a["H"]) in ((W, H), BANDED) else self.OUT_BYTES
            assert 0 < bound <= self.OUT_BYTES
            if a["cap"] == "short":                     # one byte less than the file the same call writes
                n, _ = self.call(entry, dict(over, cap=bound, **settings))
                assert n > 0, (entry, over, n)
                for o in self.out:
                    o.fill(0x5A)
                bound = n - 1
            a["cap"] = bound
        fn = getattr(self.lib, "jpezy_" + entry)
        if settings:
            self._settings(**settings)
        try:
            rc = int(fn(*self._args(entry, a)))
            if on_dev:
                assert self.lib.jpezy_ctx_sync(self.ctx) == 0        # the device entries are asynchronous
        finally:
            if settings:
                self._settings()
        if rc < 0:
            return rc, None
        sha = hashlib.sha256()
        for k in range(3):
            sha.update(self.dev["out"][k].cpu().numpy().tobytes() if on_dev else self.out[k].tobytes())
        return rc, sha.hexdigest()

    def record(self, half):
        """-> [{"entry", "case", "status", "error"[, "sha256"]}] in the table's order"""
        rows = []
        for entry, case, over in table(half):
            rc, sha = self.call(entry, over)
            row = dict(entry=entry, case=case, status=rc, error=self.lib.jpezy_hip_last_error().decode() if rc < 0 else "")
            if sha is not None:
                row["sha256"] = sha
            rows.append(row)
        return rows
