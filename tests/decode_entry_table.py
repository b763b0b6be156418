"""The fixed table of calls behind tests/golden/decode_entry_errors.json: every decode entry of the C-ABI driven through bare ctypes, with
a null context (the checks that come before the context; runs without a GPU) and with a real one (three 40 x 24 files of
tests/jpeg_synth.py).  tools/gen/record_decode_entry_errors.py records (entry, case, status, last_error text) from a build of the commit
BEFORE a change of the host layer; tests/test_decode_entry_errors.py replays the table against the build under test.

A row is (entry, file, case, overrides): the call is the entry's good argument list (Env.call) with `overrides` applied."""
import ctypes as C

import numpy as np

import jpeg_synth

W, H = 40, 24
SMOOTH, NEAREST = 1, 0
FILES = {
    "420": dict(comps=[(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]),
    "422": dict(comps=[(2, 1, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)]),
    "one": dict(comps=[(1, 1, 0, 0)]),
    "420p12": dict(comps=[(2, 2, 0, 0), (1, 1, 1, 1), (1, 1, 1, 1)], precision=12),     # header cases only
}

HOST_PLANAR = {"decode_jpeg": (), "decode_jpeg_scaled": ("scale",), "decode_jpeg_region": ("scale", "region"),
               "decode_jpeg_upsampling": ("upsampling",)}
HOST_PACKED = {"decode_jpeg_packed": (), "decode_jpeg_scaled_packed": ("scale",), "decode_jpeg_region_packed": ("scale", "region"),
               "decode_jpeg_upsampling_packed": ("upsampling",)}
DEV_PLANAR = {"dequant_idct_generic_dev": None, "dequant_idct_generic_batch_dev": (), "dequant_idct_scaled_dev": ("scale",),
              "dequant_idct_region_dev": ("scale", "region"), "dequant_idct_upsampling_dev": ("upsampling",)}
DEV_PACKED = {"dequant_idct_scaled_packed_dev": ("scale",), "dequant_idct_region_packed_dev": ("scale", "region"),
              "dequant_idct_upsampling_packed_dev": ("upsampling",)}
HOST_ENTRIES = [*HOST_PLANAR, *HOST_PACKED, "decode_jpeg_ycc"]
DEV_ENTRIES = [*DEV_PLANAR, *DEV_PACKED]
ENTRIES = HOST_ENTRIES + DEV_ENTRIES
# decode entries of api.ABI this table leaves alone: the batch (a list of files with a status each) and the three fused entries for the
# project's own layout, which tests/fused_entry_table.py drives beside the encoder's entries
NOT_IN_TABLE = {"jpezy_decode_jpeg_batch", "jpezy_dequant_idct_dev", "jpezy_dequant_idct_packed_dev", "jpezy_dequant_idct_ycc_dev"}

REGION = (3, 2, 5, 4)           # inside the 20 x 12 picture of scale_denom 2 (the default scale of every row)


def scaled_size(scale):
    n = 8 // scale
    return (W * n + 7) // 8, (H * n + 7) // 8


def out_size(entry, scale=2, region=REGION):
    """(w, h) of what the entry writes with the table's default arguments"""
    if "region" in entry:
        return region[2], region[3]
    if "scaled" in entry:
        return scaled_size(scale)
    return W, H


def _null_rows():
    rows = []
    add = lambda entry, case, **over: rows.append((entry, "420", case, over))
    for e in ENTRIES:
        add(e, "none_bad")
    for e in HOST_ENTRIES:
        add(e, "null_info", info=None)
        add(e, "null_data", data=None)
    for e in HOST_PLANAR:
        add(e, "null_r", r=None)
        add(e, "null_b", b=None)
    for e in HOST_PACKED:
        add(e, "null_pix", pix=None)
        add(e, "bad_format", format=7)
        add(e, "negative_format", format=-1)
        add(e, "row_stride_small", row_stride=out_size(e)[0] * 3 - 1)
    for e in ENTRIES:
        if "scaled" in e or "region" in e:
            for s in (0, 3, 16, -2):
                add(e, f"bad_scale_{s}", scale=s)
        if "upsampling" in e:
            add(e, "bad_upsampling", upsampling=2)
            add(e, "negative_upsampling", upsampling=-1)
            add(e, "nearest", upsampling=NEAREST)
        if "region" in e:
            add(e, "null_region", region=None)
            add(e, "region_outside", region=(17, 2, 5, 4))
            add(e, "region_outside_below", region=(3, 9, 5, 4))
            add(e, "region_zero_width", region=(3, 2, 0, 4))
            add(e, "region_negative_x", region=(-1, 2, 5, 4))
            add(e, "region_whole", region=(0, 0, 20, 12))
    add("decode_jpeg_scaled", "scale_1", scale=1)
    add("decode_jpeg_scaled_packed", "scale_1", scale=1)
    add("decode_jpeg_scaled_packed", "scale_1_bad_format", scale=1, format=7)
    add("decode_jpeg_ycc", "c_step_3", c_step=3)
    add("decode_jpeg_ycc", "c_step_0", c_step=0)
    add("decode_jpeg_ycc", "chroma_without_y", y=None)
    add("decode_jpeg_ycc", "all_null", y=None, cb=None, cr=None)
    for e in DEV_ENTRIES:
        add(e, "null_coeffs", co=None)
        add(e, "null_qt", qt=None)
        add(e, "null_comp_h", comp_h=None)
        add(e, "null_comp_tq", comp_tq=None)
        add(e, "misaligned_coeffs", co="misaligned")
        add(e, "n_frames_0", n_frames=0)
        add(e, "w_0", W=0)
        add(e, "h_65536", H=65536)
        if "upsampling" in e:
            add(e, "precision_12_smooth", precision=12)
    for e in DEV_PLANAR:
        add(e, "null_g", g=None)
        if DEV_PLANAR[e] is not None:
            w, h = out_size(e)
            add(e, "plane_stride_small", plane_stride=(w * h - 1) & ~3 if "region" not in e and "scaled" not in e else w * h - 1, n_frames=2)
    for e in DEV_PACKED:
        w, h = out_size(e)
        add(e, "null_pix", pix=None)
        add(e, "bad_format", format=7)
        add(e, "row_stride_small", row_stride=w * 3 - 1)
        add(e, "frame_stride_small", format=2, row_stride=w * 4 + 4, frame_stride=(h - 1) * (w * 4 + 4) + w * 4 - 1, n_frames=2)
    # two bad arguments: which check wins
    add("decode_jpeg_scaled", "bad_scale_and_null_info", scale=3, info=None)
    add("decode_jpeg_scaled_packed", "bad_scale_and_bad_format", scale=3, format=7)
    add("decode_jpeg_region", "bad_scale_and_null_region", scale=3, region=None)
    add("decode_jpeg_region", "bad_scale_and_region_zero_width", scale=3, region=(3, 2, 0, 4))
    add("decode_jpeg_region_packed", "region_zero_width_and_bad_format", region=(3, 2, 0, 4), format=7)
    add("decode_jpeg_region_packed", "bad_format_and_row_stride_small", format=7, row_stride=1)
    add("decode_jpeg_upsampling", "bad_upsampling_and_null_info", upsampling=2, info=None)
    add("decode_jpeg_upsampling_packed", "bad_upsampling_and_bad_format", upsampling=2, format=7)
    add("decode_jpeg_ycc", "c_step_3_and_null_data", c_step=3, data=None)
    add("decode_jpeg_ycc", "null_info_and_chroma_without_y", info=None, y=None)
    add("dequant_idct_region_dev", "null_r_and_bad_scale", r=None, scale=3)
    add("dequant_idct_region_dev", "bad_scale_and_region_outside", scale=3, region=(17, 2, 5, 4))
    add("dequant_idct_region_dev", "plane_stride_small_and_misaligned", plane_stride=19, co="misaligned")
    add("dequant_idct_region_dev", "n_frames_0_and_w_0", n_frames=0, W=0)
    add("dequant_idct_region_packed_dev", "bad_format_and_misaligned", format=7, co="misaligned")
    add("dequant_idct_region_packed_dev", "null_pix_and_null_coeffs", pix=None, co=None)
    add("dequant_idct_upsampling_dev", "bad_upsampling_and_precision_12", upsampling=2, precision=12)
    add("dequant_idct_upsampling_packed_dev", "precision_12_and_bad_format", precision=12, format=7)
    return rows


def _real_rows():
    rows = []
    for f in ("420", "422", "one"):
        add = lambda entry, case, **over: rows.append((entry, f, case, over))
        for e in HOST_PLANAR:
            w, h = out_size(e)
            add(e, "ok")
            add(e, "ok_gray", gray=1)
            add(e, "plane_cap_short", plane_cap=w * h - 1)
            add(e, "header_only", r=None, g=None, b=None)
        for e in HOST_PACKED:
            w, h = out_size(e)
            add(e, "ok")
            add(e, "ok_bgra_wide_rows", format=3, row_stride=w * 4 + 5)
            add(e, "pix_cap_short", pix_cap=h * w * 3 - 1)
            add(e, "pix_cap_short_wide_rows", row_stride=w * 3 + 5, pix_cap=(h - 1) * (w * 3 + 5) + w * 3 - 1)
            add(e, "row_stride_small", row_stride=w * 3 - 1)
            add(e, "header_only", pix=None)
        for e in HOST_ENTRIES:
            add(e, "len_header", len="header")
            add(e, "len_8", len=8)
            add(e, "len_0", len=0)
            if "region" in e:
                for s in (1, 2, 4, 8):
                    ws, hs = scaled_size(s)
                    add(e, f"ok_scale_{s}", scale=s, region=(ws - 5, hs - 3, 5, 3))
                    add(e, f"region_outside_right_scale_{s}", scale=s, region=(ws - 4, 0, 5, 3))
                    add(e, f"region_outside_below_scale_{s}", scale=s, region=(0, hs - 2, 5, 3))
                    add(e, f"whole_scale_{s}", scale=s, region=(0, 0, ws, hs), plane_cap=ws * hs, pix_cap=ws * hs * 3)
                    add(e, f"whole_cap_short_scale_{s}", scale=s, region=(0, 0, ws, hs), plane_cap=ws * hs - 1, pix_cap=ws * hs * 3 - 1)
            if "scaled" in e:
                for s in (1, 4, 8):
                    ws, hs = scaled_size(s)
                    add(e, f"ok_scale_{s}", scale=s, plane_cap=ws * hs, pix_cap=ws * hs * 3)
                    add(e, f"cap_short_scale_{s}", scale=s, plane_cap=ws * hs - 1, pix_cap=ws * hs * 3 - 1)
                add(e, "bad_scale", scale=3)
            if "upsampling" in e:
                add(e, "nearest", upsampling=NEAREST)
                add(e, "nearest_cap_short", upsampling=NEAREST, plane_cap=W * H - 1, pix_cap=W * H * 3 - 1)
                add(e, "bad_upsampling", upsampling=2)
        cw, ch = {"420": (20, 12), "422": (20, 24), "one": (0, 0)}[f]
        add("decode_jpeg_ycc", "ok")
        add("decode_jpeg_ycc", "ok_interleaved", c_step=2, cr="cb+1")
        add("decode_jpeg_ycc", "ok_luma_only", cb=None, cr=None)
        add("decode_jpeg_ycc", "header_only", y=None, cb=None, cr=None)
        add("decode_jpeg_ycc", "y_cap_short", y_cap=W * H - 1)
        add("decode_jpeg_ycc", "c_cap_short", c_cap=max(cw * ch - 1, 0))
        add("decode_jpeg_ycc", "y_stride_small", y_stride=W - 1)
        add("decode_jpeg_ycc", "c_stride_small", c_stride=cw - 1 if cw else 1)
        # the device entries on this file's coefficients: one frame, two frames, and what each refuses once it has a context
        for e in DEV_ENTRIES:
            w, h = out_size(e)
            add(e, "ok")
            add(e, "ok_gray", gray=1)
            if e != "dequant_idct_generic_dev":
                add(e, "ok_two_frames", n_frames=2)
            if e in DEV_PLANAR and "generic" not in e:
                add(e, "two_frames_odd_stride", n_frames=2, plane_stride=w * h + 3)
            if "scaled" in e or "region" in e:
                for s in (1, 4, 8):
                    ws, hs = scaled_size(s)
                    add(e, f"ok_scale_{s}", scale=s, region=(ws - 5, hs - 3, 5, 3))
                    add(e, f"whole_two_frames_scale_{s}", scale=s, region=(0, 0, ws, hs), n_frames=2, plane_stride=ws * hs + 3,
                        frame_stride=ws * hs * 3 + 3)
            if "upsampling" in e:
                add(e, "nearest", upsampling=NEAREST)
                add(e, "nearest_two_frames_odd_stride", upsampling=NEAREST, n_frames=2, plane_stride=W * H + 3, frame_stride=W * H * 3 + 3)
            if f != "420":
                continue
            add(e, "null_coeffs", co=None)
            add(e, "null_qt", qt=None)
            add(e, "null_comp_v", comp_v=None)
            add(e, "misaligned_coeffs", co="misaligned")
            add(e, "n_frames_0", n_frames=0)
            add(e, "w_0", W=0)
            add(e, "ncomp_2", ncomp=2)
            add(e, "sampling_factor_5", comp_h=(5, 1, 1))
            if "scaled" in e or "region" in e:
                add(e, "bad_scale", scale=3)
                add(e, "bad_scale_and_null_coeffs", scale=3, co=None)
                add(e, "bad_scale_and_w_0", scale=3, W=0)
            if "upsampling" in e:
                add(e, "bad_upsampling", upsampling=2)
                add(e, "precision_12_smooth", precision=12)
                add(e, "bad_upsampling_and_w_0", upsampling=2, W=0)
            if "region" in e:
                add(e, "region_outside", region=(17, 2, 5, 4))
                add(e, "null_region", region=None)
            if e in DEV_PLANAR:
                add(e, "null_b", b=None)
                add(e, "null_b_and_misaligned", b=None, co="misaligned")
                if DEV_PLANAR[e] is not None:
                    add(e, "plane_stride_small", plane_stride=(w * h - 1) & ~3 if "region" not in e and "scaled" not in e else w * h - 1,
                        n_frames=2)
                    add(e, "plane_stride_small_and_misaligned", plane_stride=16, n_frames=2, co="misaligned")
            else:
                add(e, "null_pix", pix=None)
                add(e, "bad_format", format=7)
                add(e, "bad_format_and_null_coeffs", format=7, co=None)
                add(e, "row_stride_small", row_stride=w * 3 - 1)
                add(e, "frame_stride_small", format=2, row_stride=w * 4 + 4, frame_stride=(h - 1) * (w * 4 + 4) + w * 4 - 1, n_frames=2)
                add(e, "two_frames_odd_frame_stride", n_frames=2, frame_stride=h * w * 3 + 3)
    for e in HOST_ENTRIES:
        if "upsampling" in e:
            rows.append((e, "420p12", "smooth_12_bit", {}))
            rows.append((e, "420p12", "smooth_12_bit_header_only", dict(r=None, g=None, b=None, pix=None)))
            rows.append((e, "420p12", "nearest_12_bit_header_only", dict(upsampling=NEAREST, r=None, g=None, b=None, pix=None)))
    return rows


def table(half):
    """half: "null_context" or "real_context" -> [(entry, file, case, overrides)]"""
    return _null_rows() if half == "null_context" else _real_rows()


def header_length(data):
    sos = data.index(b"\xff\xda")
    return sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")


class Env:
    """Buffers and the calls themselves.  ctx None: the null-context half (host memory everywhere; nothing is ever written).  With a context
    the device entries get device memory from torch, large enough for whatever an unexpected success would write."""
    OUT_BYTES = 1 << 16

    def __init__(self, J, ctx=None):
        self.J, self.lib, self.ctx = J, J.load_library(), ctx
        self.files = {}
        self.host = [np.zeros(self.OUT_BYTES, np.uint8) for _ in range(3)]
        self.keep = []
        for key, spec in FILES.items():
            data, _, _ = jpeg_synth.synth_jpeg(W, H, seed=11, **spec)
            buf = np.frombuffer(data, np.uint8).copy()
            f = dict(data=data, buf=buf, hdr=header_length(data), info=J.FrameInfo())
            if ctx is None:
                f["co"] = self.host[0].ctypes.data
                f["dev_out"] = [h.ctypes.data for h in self.host]
                f["layout"] = (3, (1, 1, 1), (1, 1, 1), (0, 1, 1), 8)
            elif key != "420p12":
                import torch
                dev = torch.device("cuda", J.load_library().jpezy_ctx_device(ctx))
                info = f["info"]
                assert self.lib.jpezy_read_jpeg_gpu(ctx, buf.ctypes.data, buf.size, C.byref(info), None, 0) >= 0
                n = info.mcu_cols * info.mcu_rows * info.blocks_per_mcu * 64
                d_co = torch.zeros(2 * n + 64, dtype=torch.int16, device=dev)
                assert self.lib.jpezy_read_jpeg_gpu(ctx, buf.ctypes.data, buf.size, C.byref(info), d_co.data_ptr(), n) >= 0
                d_co[n:2 * n] = d_co[:n]
                outs = [torch.zeros(self.OUT_BYTES, dtype=torch.uint8, device=dev) for _ in range(3)]
                torch.cuda.synchronize()
                self.keep += [d_co, *outs]
                f["co"] = d_co.data_ptr()
                f["dev_out"] = [o.data_ptr() for o in outs]
                f["dev_tensors"] = outs
                f["layout"] = (info.ncomp, tuple(max(1, v) for v in info.H), tuple(max(1, v) for v in info.V), tuple(info.Tq), info.precision)
                f["qt"] = info.qt
            self.files[key] = f

    def call(self, entry, file, over):
        """-> (status, info): the entry's good arguments with `over` applied"""
        f = self.files[file]
        ncomp, hs, vs, tq, precision = f.get("layout", (3, (1, 1, 1), (1, 1, 1), (0, 1, 1), 8))
        a = dict(data=f["buf"].ctypes.data, len=f["buf"].size, gray=0, scale=2, region=REGION, upsampling=SMOOTH, info=True,
                 r=self.host[0].ctypes.data, g=self.host[1].ctypes.data, b=self.host[2].ctypes.data, plane_cap=self.OUT_BYTES,
                 format=0, row_stride=0, pix=self.host[0].ctypes.data, pix_cap=self.OUT_BYTES,
                 y=self.host[0].ctypes.data, y_stride=0, y_cap=self.OUT_BYTES, cb=self.host[1].ctypes.data, cr=self.host[2].ctypes.data,
                 c_stride=0, c_step=1, c_cap=self.OUT_BYTES,
                 co=f.get("co"), qt=True, ncomp=ncomp, comp_h=hs, comp_v=vs, comp_tq=tq, precision=precision, W=W, H=H, n_frames=1,
                 plane_stride=W * H, frame_stride=0)
        host = entry in HOST_ENTRIES
        if not host:
            a.update(r=f["dev_out"][0], g=f["dev_out"][1], b=f["dev_out"][2], pix=f["dev_out"][0])
        a.update(over)
        if a["len"] == "header":
            a["len"] = f["hdr"]
        if a["co"] == "misaligned":
            a["co"] = f["co"] + 2
        if a["cr"] == "cb+1":
            a["cr"] = a["cb"] + 1
        info = self.J.FrameInfo()
        keep = []

        def arr3(v):
            if v is None:
                return None
            keep.append((C.c_uint8 * 3)(*v))
            return C.addressof(keep[-1])

        rect = None
        if a["region"] is not None:
            keep.append(self.J.Rect(*a["region"]))
            rect = C.addressof(keep[-1])
        extra = dict(scale=a["scale"], region=rect, upsampling=a["upsampling"])
        p_info = C.byref(info) if a["info"] else None
        if a["qt"] is True:
            keep.append(f.get("qt", ((C.c_uint16 * 64) * 4)()))
            a["qt"] = C.addressof(keep[-1])
        fn = getattr(self.lib, "jpezy_" + entry)
        if entry == "decode_jpeg_ycc":
            args = [self.ctx, a["data"], a["len"], p_info, a["y"], a["y_stride"], a["y_cap"], a["cb"], a["cr"], a["c_stride"], a["c_step"], a["c_cap"]]
        elif host:
            names = HOST_PLANAR.get(entry, HOST_PACKED.get(entry))
            tail = [a["r"], a["g"], a["b"], a["plane_cap"]] if entry in HOST_PLANAR else [a["format"], a["row_stride"], a["pix"], a["pix_cap"]]
            args = [self.ctx, a["data"], a["len"], a["gray"]] + [extra[n] for n in names] + [p_info] + tail
        else:
            names = DEV_PLANAR.get(entry, DEV_PACKED.get(entry))
            head = [self.ctx, a["co"], a["qt"], a["ncomp"], arr3(a["comp_h"]), arr3(a["comp_v"]), arr3(a["comp_tq"]), a["precision"], a["W"], a["H"],
                    a["gray"]]
            if names is None:           # jpezy_dequant_idct_generic_dev: one frame, no stride
                tail = [a["r"], a["g"], a["b"], None]
            elif entry in DEV_PLANAR:
                tail = [a["n_frames"], a["plane_stride"], a["r"], a["g"], a["b"], None]
            else:
                tail = [a["format"], a["row_stride"], a["frame_stride"], a["n_frames"], a["pix"], None]
            args = head + [extra[n] for n in names or ()] + tail
        rc = int(fn(*args))
        if self.ctx is not None and not host:
            assert self.lib.jpezy_ctx_sync(self.ctx) == 0        # the device entries are asynchronous
        return rc, info

    def record(self, half):
        """-> [{"entry", "file", "case", "status", "error"[, "info"]}] in the table's order"""
        out = []
        for entry, file, case, over in table(half):
            rc, info = self.call(entry, file, over)
            row = dict(entry=entry, file=file, case=case, status=rc, error=self.lib.jpezy_hip_last_error().decode() if rc < 0 else "")
            if "header_only" in case and rc == 0:
                row["info"] = [info.width, info.height, info.ncomp, info.precision, info.blocks_per_mcu]
            out.append(row)
        return out
