"""ctypes binding of include/jpezy_hip.h plus a Python mirror of the reference's encoder/decoder surface.

Naming follows the reference: `Encoder(property, r, g, b).encode(output_file, gray=...)` mirrors
`jpezy::encoder<T>::encode<MODE_TAG>(const char*)` (ref encoder/jpezy_encoder.hpp:22-77) and
`Decoder(filename).decode(gray=...)` mirrors `jpezy::decoder<>::decode<MODE_TAG>()`
(ref decoder/jpezy_decoder.hpp:39-134).  All compute goes through the C-ABI; nothing here touches oracle/.
"""
import contextlib
import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
# JPEZY_LIB: development aid (tools/ab/ab_run.sh): load another build of the same library for A/B timing
_LIBPATH = Path(os.environ["JPEZY_LIB"]) if os.environ.get("JPEZY_LIB") else _PKG / "libjpezy_hip.so"
_LIB = None


class JpezyError(RuntimeError):
    pass


class FrameInfo(C.Structure):
    _fields_ = [
        ("width", C.c_int), ("height", C.c_int), ("ncomp", C.c_int), ("precision", C.c_int),
        ("H", C.c_int * 3), ("V", C.c_int * 3), ("Tq", C.c_int * 3),
        ("hmax", C.c_int), ("vmax", C.c_int), ("mcu_cols", C.c_int), ("mcu_rows", C.c_int),
        ("blocks_per_mcu", C.c_int), ("restart_interval", C.c_int),
        ("major_rev", C.c_int), ("minor_rev", C.c_int), ("units", C.c_int),
        ("hdensity", C.c_int), ("vdensity", C.c_int), ("format", C.c_int),
        ("comment", C.c_char * 256),
        ("qt", (C.c_uint16 * 64) * 4),
    ]


class Rect(C.Structure):
    """jpezy_rect: a window of the picture at the requested scale"""
    _fields_ = [("x", C.c_int), ("y", C.c_int), ("w", C.c_int), ("h", C.c_int)]


class Window(C.Structure):
    """jpezy_window: a region of the picture at 1/scale_denom; w == h == 0: the whole picture at that scale"""
    _fields_ = [("region", Rect), ("scale_denom", C.c_int)]


class MultiOut(C.Structure):
    _fields_ = [("coeffs", C.c_void_p), ("jpg", C.c_void_p), ("jpg_stride", C.c_size_t), ("jpg_sizes", C.POINTER(C.c_longlong)),
                ("on_root_device", C.c_int)]


class MultiLaneStats(C.Structure):
    _fields_ = [("device", C.c_int), ("staged", C.c_int), ("frames", C.c_long), ("wall_ms", C.c_double), ("kernel_ms", C.c_double),
                ("bytes_up", C.c_ulonglong), ("bytes_down", C.c_ulonglong)]


# every symbol include/jpezy_hip.h declares: (name, restype, argtypes)
_u8p, _i16p, _vp = C.POINTER(C.c_uint8), C.POINTER(C.c_int16), C.c_void_p
_QT = C.POINTER((C.c_uint16 * 64) * 4)
_TQ = C.POINTER(C.c_uint8 * 3)
ABI = [
    ("jpezy_hip_last_error", C.c_char_p, []),
    ("jpezy_hip_device_count", C.c_int, []),
    ("jpezy_hip_is_experimental_build", C.c_int, []),
    ("jpezy_ctx_create", _vp, [C.c_int]),
    ("jpezy_ctx_destroy", None, [_vp]),
    ("jpezy_ctx_sync", C.c_int, [_vp]),
    ("jpezy_ctx_device", C.c_int, [_vp]),
    ("jpezy_ctx_stream", _vp, [_vp]),
    ("jpezy_mcu_cols", C.c_int, [C.c_int]),
    ("jpezy_mcu_rows", C.c_int, [C.c_int]),
    ("jpezy_coeff_count", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("jpezy_fdct_quant", C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    ("jpezy_fdct_quant_dev", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    ("jpezy_dequant_idct", C.c_int, [_vp, _vp, _QT, _TQ, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("jpezy_dequant_idct_dev", C.c_int, [_vp, _vp, _QT, _TQ, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    ("jpezy_dequant_idct_generic", C.c_int, [_vp, _vp, _QT, C.c_int, _TQ, _TQ, _TQ, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp]),
    ("jpezy_dequant_idct_generic_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    ("jpezy_dequant_idct_generic_batch_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                                       _vp, _vp, _vp, _vp]),
    ("jpezy_ctx_set_force_exact", None, [_vp, C.c_int]),
    ("jpezy_ctx_set_variant", C.c_int, [_vp, C.c_int]),
    ("jpezy_ctx_set_decode_tolerance", C.c_int, [_vp, C.c_int]),
    ("jpezy_ctx_set_host_chunk_bytes", None, [_vp, C.c_size_t]),
    ("jpezy_ctx_last_fallback_count", C.c_long, [_vp]),
    ("jpezy_write_jpeg", C.c_long, [_vp, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t]),
    ("jpezy_jpeg_bound", C.c_size_t, [C.c_int, C.c_int]),
    ("jpezy_write_jpeg_batch", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t, C.POINTER(C.c_long), C.c_int]),
    ("jpezy_write_jpeg_gpu", C.c_long, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t]),
    ("jpezy_write_jpeg_gpu_batch", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t, C.POINTER(C.c_long)]),
    ("jpezy_write_jpeg_gpu_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t, _vp, _vp]),
    ("jpezy_ctx_set_huffman_optimize", C.c_int, [_vp, C.c_int]),
    ("jpezy_huffman_histogram_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    ("jpezy_huffman_optimal_table", C.c_int, [_vp, _vp, _vp]),
    ("jpezy_write_jpeg_opt", C.c_long, [_vp, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t]),
    ("jpezy_write_jpeg_rst", C.c_long, [_vp, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.c_int, _vp, C.c_size_t]),
    ("jpezy_ctx_set_restart_interval", C.c_int, [_vp, C.c_int]),
    ("jpezy_ctx_restart_interval", C.c_int, [_vp]),
    ("jpezy_quality_tables", C.c_int, [C.c_int, _vp, _vp]),
    ("jpezy_ctx_set_quant_tables", C.c_int, [_vp, _vp, _vp]),
    ("jpezy_ctx_set_quality", C.c_int, [_vp, C.c_int]),
    ("jpezy_ctx_quant_tables", C.c_int, [_vp, _vp, _vp]),
    ("jpezy_ctx_set_chroma_downsampling", C.c_int, [_vp, C.c_int]),
    ("jpezy_ctx_chroma_downsampling", C.c_int, [_vp]),
    ("jpezy_write_jpeg_qt", C.c_long, [_vp, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, _vp, C.c_int, C.c_int, _vp, C.c_size_t]),
    ("jpezy_quant_tables_probe", C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(C.c_int)]),
    ("jpezy_ctx_set_dc_table_lookup", None, [_vp, C.c_int]),
    ("jpezy_ctx_set_encode_groups", C.c_int, [_vp, C.c_int]),
    ("jpezy_ctx_encode_groups", C.c_int, [_vp]),
    ("jpezy_encode_jpeg", C.c_long, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t]),
    ("jpezy_shard_range", None, [C.c_long, C.c_int, C.c_int, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    ("jpezy_encode_batch_multi", C.c_int, [C.POINTER(C.c_int), C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p,
                                           C.POINTER(MultiOut)]),
    ("jpezy_multi_create", _vp, [C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    ("jpezy_multi_destroy", None, [_vp]),
    ("jpezy_multi_encode", C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_char_p, C.POINTER(MultiOut)]),
    ("jpezy_multi_last_stats", C.c_int, [_vp, C.POINTER(MultiLaneStats), C.c_int]),
    ("jpezy_multi_chunk_frames", C.c_int, [_vp]),
    ("jpezy_multi_feeder_threads", C.c_int, [_vp]),
    ("jpezy_multi_set_feeder_threads", C.c_int, [_vp, C.c_int]),
    ("jpezy_read_jpeg", C.c_int, [_vp, C.c_size_t, C.POINTER(FrameInfo), _vp, C.c_size_t]),
    ("jpezy_read_jpeg_gpu", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(FrameInfo), _vp, C.c_size_t]),
    ("jpezy_decode_jpeg", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.POINTER(FrameInfo), _vp, _vp, _vp, C.c_size_t]),
    ("jpezy_decode_jpeg_batch", C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("jpezy_ctx_last_huffdec_passes", C.c_int, [_vp]),
    ("jpezy_ctx_last_batch_fast_count", C.c_int, [_vp]),
    ("jpezy_ctx_set_huffdec_min_bytes", None, [_vp, C.c_size_t]),
    ("jpezy_pixel_bytes", C.c_int, [C.c_int]),
    ("jpezy_fdct_quant_packed_dev", C.c_int, [_vp, _vp, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    ("jpezy_dequant_idct_packed_dev", C.c_int, [_vp, _vp, _QT, _TQ, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    ("jpezy_encode_jpeg_packed", C.c_long, [_vp, _vp, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t]),
    ("jpezy_decode_jpeg_packed", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.POINTER(FrameInfo), C.c_int, C.c_size_t, _vp, C.c_size_t]),
    ("jpezy_scaled_size", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("jpezy_dequant_idct_scaled_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                                _vp, _vp, _vp, _vp]),
    ("jpezy_dequant_idct_scaled_packed_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                       C.c_size_t, C.c_size_t, C.c_int, _vp, _vp]),
    ("jpezy_decode_jpeg_scaled", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(FrameInfo), _vp, _vp, _vp, C.c_size_t]),
    ("jpezy_decode_jpeg_scaled_packed", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(FrameInfo), C.c_int, C.c_size_t, _vp, C.c_size_t]),
    ("jpezy_region_check", C.c_int, [C.c_int, C.c_int, C.c_int, _vp]),
    ("jpezy_dequant_idct_region_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int,
                                                C.c_size_t, _vp, _vp, _vp, _vp]),
    ("jpezy_dequant_idct_region_packed_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp,
                                                       C.c_int, C.c_size_t, C.c_size_t, C.c_int, _vp, _vp]),
    ("jpezy_decode_jpeg_region", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp, C.POINTER(FrameInfo), _vp, _vp, _vp, C.c_size_t]),
    ("jpezy_decode_jpeg_region_packed", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, _vp, C.POINTER(FrameInfo), C.c_int, C.c_size_t, _vp,
                                                  C.c_size_t]),
    ("jpezy_window_fit", C.c_int, [C.c_int, C.c_int, _vp, C.c_int, C.c_size_t, C.c_size_t, _vp]),
    ("jpezy_decode_windows_dev", C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, C.c_int, C.c_size_t, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp]),
    ("jpezy_ctx_set_windows_slice_files", C.c_int, [_vp, C.c_int]),
    ("jpezy_resize_taps", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), _vp, _vp, _vp, C.c_size_t]),
    ("jpezy_resize_taps_filter", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), _vp, _vp, _vp, C.c_size_t]),
    ("jpezy_ctx_set_windows_filter", C.c_int, [_vp, C.c_int]),
    ("jpezy_ctx_windows_filter", C.c_int, [_vp]),
    ("jpezy_ctx_set_resample_direct", C.c_int, [_vp, C.c_int]),
    ("jpezy_ctx_last_resample_tiled_count", C.c_int, [_vp]),
    ("jpezy_resize_pick_window", C.c_int, [C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp]),
    ("jpezy_decode_windows_resized_dev", C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_size_t, _vp,
                                                   C.c_size_t, _vp, _vp, _vp]),
    ("jpezy_tensor_normalization", C.c_int, [C.c_int, _vp, _vp, _vp, _vp]),
    ("jpezy_decode_windows_tensor_dev", C.c_int, [_vp, C.c_int, _vp, _vp, C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp,
                                                  C.c_int64, C.c_int64, C.c_int64, C.c_int64, _vp, C.c_size_t, _vp, _vp, _vp]),
    ("jpezy_ycc_chroma_size", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("jpezy_ycc_component_size", C.c_int, [C.POINTER(FrameInfo), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("jpezy_fdct_quant_ycc_dev", C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                           C.c_int, _vp, _vp]),
    ("jpezy_dequant_idct_ycc_dev", C.c_int, [_vp, _vp, _QT, _TQ, _vp, C.c_size_t, _vp, _vp, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_int,
                                             C.c_int, C.c_int, _vp]),
    ("jpezy_encode_jpeg_ycc", C.c_long, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t]),
    ("jpezy_decode_jpeg_ycc", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(FrameInfo), _vp, C.c_size_t, C.c_size_t, _vp, _vp, C.c_size_t, C.c_int,
                                        C.c_size_t]),
    ("jpezy_sampling_geometry", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("jpezy_coeff_count_sampling", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("jpezy_jpeg_bound_sampling", C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    ("jpezy_fdct_quant_sampling_dev", C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    ("jpezy_fdct_quant_sampling_packed_dev", C.c_int, [_vp, _vp, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp,
                                                       _vp]),
    ("jpezy_write_jpeg_sampling", C.c_long, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, _vp, C.c_int, C.c_int, _vp, C.c_size_t]),
    ("jpezy_write_jpeg_gpu_sampling", C.c_long, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t]),
    ("jpezy_write_jpeg_gpu_sampling_batch", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t, _vp]),
    ("jpezy_write_jpeg_gpu_sampling_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t, _vp, _vp]),
    ("jpezy_huffman_histogram_sampling_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    ("jpezy_huffman_histogram_sampling", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    ("jpezy_encode_jpeg_sampling", C.c_long, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t]),
    ("jpezy_encode_jpeg_sampling_packed", C.c_long, [_vp, _vp, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp,
                                                     C.c_size_t]),
    ("jpezy_transform_geometry", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int),
                                           C.POINTER(C.c_int)]),
    ("jpezy_coeff_transform_dev", C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    ("jpezy_quant_tables_transform", C.c_int, [C.c_int, _vp, _vp]),
    ("jpezy_transform_jpeg", C.c_long, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_char_p, C.POINTER(FrameInfo), _vp, C.c_size_t]),
    ("jpezy_dequant_idct_upsampling_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                    C.c_size_t, _vp, _vp, _vp, _vp]),
    ("jpezy_dequant_idct_upsampling_packed_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                           C.c_size_t, C.c_size_t, C.c_int, _vp, _vp]),
    ("jpezy_decode_jpeg_upsampling", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(FrameInfo), _vp, _vp, _vp, C.c_size_t]),
    ("jpezy_decode_jpeg_upsampling_packed", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.POINTER(FrameInfo), C.c_int, C.c_size_t, _vp,
                                                      C.c_size_t]),
    ("jpezy_ctx_set_windows_upsampling", C.c_int, [_vp, C.c_int]),
    ("jpezy_ctx_windows_upsampling", C.c_int, [_vp]),
]

# include/jpezy_hip_region_upsampling.h (part of jpezy_hip.h): the region entries with the chroma upsampling as an argument.  ABI above is
# jpezy_hip.h's own declarations, whose decode entries are a closed, recorded set (tests/decode_entry_table.py)
ABI_REGION_UPSAMPLING = [
    ("jpezy_dequant_idct_region_upsampling_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                           _vp, C.c_int, C.c_size_t, _vp, _vp, _vp, _vp]),
    ("jpezy_dequant_idct_region_upsampling_packed_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                                  C.c_int, _vp, C.c_int, C.c_size_t, C.c_size_t, C.c_int, _vp, _vp]),
    ("jpezy_decode_jpeg_region_upsampling", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(FrameInfo), _vp, _vp, _vp,
                                                      C.c_size_t]),
    ("jpezy_decode_jpeg_region_upsampling_packed", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(FrameInfo), C.c_int,
                                                             C.c_size_t, _vp, C.c_size_t]),
]

# include/jpezy_hip_orientation.h (part of jpezy_hip.h): the EXIF orientation tag, the geometry of the eight orientations, the region and
# file entries with an orientation argument, the orientation setting of the window batches.  Kept out of ABI for the same reason
ABI_ORIENTATION = [
    ("jpezy_jpeg_orientation", C.c_int, [_vp, C.c_size_t]),
    ("jpezy_orient_size", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("jpezy_orient_rect", C.c_int, [C.c_int, C.c_int, C.c_int, _vp, _vp]),
    ("jpezy_dequant_idct_region_oriented_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                         _vp, C.c_int, C.c_int, C.c_size_t, _vp, _vp, _vp, _vp]),
    ("jpezy_dequant_idct_region_oriented_packed_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                                C.c_int, _vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, _vp, _vp]),
    ("jpezy_decode_jpeg_oriented", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.POINTER(C.c_int), C.POINTER(FrameInfo),
                                             _vp, _vp, _vp, C.c_size_t]),
    ("jpezy_decode_jpeg_oriented_packed", C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.POINTER(C.c_int),
                                                    C.POINTER(FrameInfo), C.c_int, C.c_size_t, _vp, C.c_size_t]),
    ("jpezy_ctx_set_windows_orientation", C.c_int, [_vp, C.c_int]),
    ("jpezy_ctx_windows_orientation", C.c_int, [_vp]),
]
ORIENT_FROM_FILE = 0        # JPEZY_ORIENT_FROM_FILE: the orientation argument of decode_jpeg_oriented[_packed] -- the file's own tag

# include/jpezy_hip_ycc422.h (part of jpezy_hip.h): YCbCr 4:2:2 samples in and out -- planar I422 / NV16 and packed YUY2 / UYVY / YVYU.
# Kept out of ABI for the same reason
ABI_YCC422 = [
    ("jpezy_yuv422_row_bytes", C.c_int, [C.c_int]),
    ("jpezy_ycc422_chroma_size", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("jpezy_fdct_quant_ycc422_dev", C.c_int, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int,
                                              _vp, _vp]),
    ("jpezy_encode_jpeg_ycc422", C.c_long, [_vp, _vp, C.c_size_t, _vp, _vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t]),
    ("jpezy_fdct_quant_yuv422_dev", C.c_int, [_vp, _vp, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    ("jpezy_encode_jpeg_yuv422", C.c_long, [_vp, _vp, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_char_p, _vp, C.c_size_t]),
    ("jpezy_dequant_idct_generic_yuv422_dev", C.c_int, [_vp, _vp, _vp, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                                        C.c_size_t, C.c_int, _vp, _vp]),
    ("jpezy_decode_jpeg_yuv422", C.c_int, [_vp, _vp, C.c_size_t, C.POINTER(FrameInfo), C.c_int, C.c_size_t, _vp, C.c_size_t]),
]
YUV_YUY2, YUV_UYVY, YUV_YVYU = 0, 1, 2          # JPEZY_YUV_*: Y0 Cb Y1 Cr / Cb Y0 Cr Y1 / Y0 Cr Y1 Cb

# chroma sampling of the encoder's *_sampling entry points: 4:2:0 (the reference's 2x2 / 1x1 / 1x1, everything as without the keyword)
# or 4:4:4 (8 x 8 MCUs of Y, Cb, Cr, no decimation; include/jpezy_hip.h has the definition)
SAMPLING_420, SAMPLING_444 = 0, 1
SAMPLING_422 = 3                               # 2x1 / 1x1 / 1x1: 16 x 8 MCUs of Y, Y, Cb, Cr (2 is kept free for 4:4:0 and refused)
ENCODE_GROUPS_AUTO, ENCODE_GROUPS_4_COOP, ENCODE_GROUPS_2_COOP, ENCODE_GROUPS_2_DIRECT = 0, 1, 2, 3   # Context.set_encode_groups
DOWNSAMPLE_POINT, DOWNSAMPLE_AVERAGE = 0, 1     # Context.set_chroma_downsampling: how 4:2:0 and 4:2:2 chroma is made from RGB pixels

# enum jpezy_pixel_format: packed (interleaved) pixels, 3 or 4 bytes each
PIX_RGB24, PIX_BGR24, PIX_RGBA32, PIX_BGRA32 = 0, 1, 2, 3

# enum jpezy_xform: lossless transforms in the coefficient domain (libjpeg's JXFORM order), and the flag that lets a mirrored axis drop its
# partial MCU column / row
XFORM_NONE, XFORM_HFLIP, XFORM_VFLIP, XFORM_TRANSPOSE, XFORM_TRANSVERSE, XFORM_ROT90, XFORM_ROT180, XFORM_ROT270 = range(8)
XFORM_TRIM = 1

# enum jpezy_upsampling: how the decoder brings subsampled chroma to picture size -- replication (the reference's, the default) or the
# triangle filter over the component's native plane (include/jpezy_hip.h, CHROMA UPSAMPLING)
UPSAMPLE_NEAREST, UPSAMPLE_SMOOTH = 0, 1
FILTER_BILINEAR, FILTER_BOX, FILTER_BICUBIC, FILTER_LANCZOS = 0, 1, 2, 3      # enum jpezy_filter

# enum jpezy_dtype: the element type of decode_windows_tensor_dev's output
DT_U8, DT_F32, DT_F16, DT_BF16 = 0, 1, 2, 3
E_UNSUPPORTED = -4          # JPEZY_E_UNSUPPORTED


def pixel_bytes(fmt):
    return _check(load_library().jpezy_pixel_bytes(int(fmt)))


def library_path():
    return _LIBPATH


def load_library():
    """Load libjpezy_hip.so (built by `python -m jpezy_amd._build` / __graft_entry__.build()).  Fails loudly."""
    global _LIB
    if _LIB is None:
        if not _LIBPATH.exists():
            raise JpezyError(f"{_LIBPATH} is missing: build it with `python -m jpezy_amd._build` "
                             "(there is no CPU fallback for the jpezy hot path)")
        # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7.  Import torch first so
        # that our DT_NEEDED(libamdhip64.so.7) binds to the copy torch already loaded; a second runtime in
        # the same process cannot see the GPU.  Without torch the system ROCm runtime is used.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        lib = C.CDLL(str(_LIBPATH))
        for name, res, args in ABI + ABI_REGION_UPSAMPLING + ABI_ORIENTATION + ABI_YCC422:
            fn = getattr(lib, name)          # AttributeError if the library does not export the symbol
            fn.restype = res
            fn.argtypes = args
        if lib.jpezy_hip_is_experimental_build() and os.environ.get("JPEZY_ALLOW_EXPERIMENT") != "1":
            raise JpezyError(f"{_LIBPATH} was built with a wrong-result timing probe (JPEZY_EXPERIMENT); "
                             "set JPEZY_ALLOW_EXPERIMENT=1 to load it for timing only")
        _LIB = lib
    return _LIB


def _check(rc):
    if rc < 0:
        raise JpezyError(f"jpezy status {rc}: {load_library().jpezy_hip_last_error().decode()}")
    return rc


def mcu_grid(W, H):
    lib = load_library()
    return lib.jpezy_mcu_cols(W), lib.jpezy_mcu_rows(H)


def coeff_count(W, H, gray=False, sampling=SAMPLING_420):
    if sampling != SAMPLING_420:
        if gray:
            raise JpezyError("coeff_count: gray is not available with SAMPLING_444 / SAMPLING_422")
        sampling_geometry(sampling, W, H)
        return load_library().jpezy_coeff_count_sampling(W, H, int(sampling))
    return load_library().jpezy_coeff_count(W, H, int(gray))


def sampling_geometry(sampling, W, H):
    """(mcu_cols, mcu_rows, blocks_per_mcu) of a W x H frame: 16 x 16 MCUs of 6 blocks (SAMPLING_420), 8 x 8 MCUs of 3 (SAMPLING_444)
    or 16 x 8 MCUs of 4 (SAMPLING_422)"""
    mc, mr, bpm = C.c_int(), C.c_int(), C.c_int()
    _check(load_library().jpezy_sampling_geometry(int(sampling), W, H, C.byref(mc), C.byref(mr), C.byref(bpm)))
    return mc.value, mr.value, bpm.value


def jpeg_bound(W, H, sampling=SAMPLING_420):
    """bytes that hold the .jpg of any W x H coefficient field of the sampling"""
    if sampling != SAMPLING_420:
        sampling_geometry(sampling, W, H)
        return load_library().jpezy_jpeg_bound_sampling(W, H, int(sampling))
    return load_library().jpezy_jpeg_bound(W, H)


def huffman_histogram(coeffs, W, H, sampling=SAMPLING_420, restart_interval=0):
    """uint64 [4, 256]: the symbols write_jpeg(..., sampling=) emits for the frame, table k in DHT order YDc, CDc, YAc, CAc (host)"""
    coeffs = np.ascontiguousarray(coeffs, dtype=np.int16)
    if coeffs.size != coeff_count(W, H, sampling=sampling):
        raise JpezyError("coefficient buffer size does not match W, H, sampling")
    hist = np.zeros((4, 256), dtype=np.uint64)
    _check(load_library().jpezy_huffman_histogram_sampling(_np_ptr(coeffs), W, H, int(sampling), int(restart_interval), _np_ptr(hist)))
    return hist


def scaled_size(W, H, scale):
    """(Ws, Hs) of a W x H file decoded at 1/scale (scale 1, 2, 4 or 8): ceil(W * n / 8), ceil(H * n / 8) with n = 8 / scale"""
    ws, hs = C.c_int(), C.c_int()
    _check(load_library().jpezy_scaled_size(int(W), int(H), int(scale), C.byref(ws), C.byref(hs)))
    return ws.value, hs.value


def _rect(region):
    x, y, w, h = (int(v) for v in region)
    return Rect(x, y, w, h)


def region_check(W, H, scale, region):
    """raises JpezyError unless region = (x, y, w, h) lies inside a W x H file decoded at 1/scale, i.e. inside scaled_size(W, H, scale)"""
    _check(load_library().jpezy_region_check(int(W), int(H), int(scale), C.byref(_rect(region))))


def jpeg_orientation(data):
    """the EXIF Orientation tag (1..8) of .jpg bytes; 1 when the file has none or anything about it is wrong (jpezy_jpeg_orientation)"""
    arr = np.frombuffer(bytes(data), dtype=np.uint8)
    return load_library().jpezy_jpeg_orientation(_np_ptr(arr) if arr.size else None, arr.size)


def orient_size(orientation, W, H):
    """(Wo, Ho) of a W x H picture shown in the orientation (1..8): swapped for 5..8 (jpezy_orient_size)"""
    wo, ho = C.c_int(), C.c_int()
    _check(load_library().jpezy_orient_size(int(orientation), int(W), int(H), C.byref(wo), C.byref(ho)))
    return wo.value, ho.value


def orient_rect(orientation, W, H, region):
    """the rectangle (x, y, w, h) of a W x H picture that the window region = (x, y, w, h) of its oriented form shows (jpezy_orient_rect)"""
    src = Rect()
    _check(load_library().jpezy_orient_rect(int(orientation), int(W), int(H), C.byref(_rect(region)), C.byref(src)))
    return src.x, src.y, src.w, src.h


def _window(win):
    """None, (x, y, w, h) or ((x, y, w, h), scale) -> Window; None: the whole picture at full size"""
    if win is None:
        return Window(Rect(0, 0, 0, 0), 1)
    if len(win) == 2 and not isinstance(win[0], (int, np.integer)):
        return Window(_rect(win[0]), int(win[1]))
    return Window(_rect(win), 1)


def window_fit(W, H, window, format=PIX_RGB24, row_stride=0, slot_stride=0):
    """the window (None, (x, y, w, h) or ((x, y, w, h), scale)) of a W x H file as decode_windows_dev decodes it, as (x, y, w, h); raises
    JpezyError when it lies outside the picture or does not fit a slot of slot_stride bytes with rows row_stride apart (jpezy_window_fit)"""
    placed = Rect()
    _check(load_library().jpezy_window_fit(int(W), int(H), C.byref(_window(window)), int(format), int(row_stride), int(slot_stride), C.byref(placed)))
    return placed.x, placed.y, placed.w, placed.h


def resize_taps(in_size, out_size, filter=FILTER_BILINEAR):
    """(first, count, weights) of one axis of decode_windows_resized_dev's resampling with the filter given (FILTER_*): int32 arrays
    [out_size], [out_size] and [out_size, ksize] (integer weights of 22 fraction bits, zero behind count); the definition is in
    include/jpezy_hip.h (jpezy_resize_taps_filter)"""
    lib = load_library()
    ksize = C.c_int()
    _check(lib.jpezy_resize_taps_filter(int(filter), int(in_size), int(out_size), C.byref(ksize), None, None, None, 0))
    first, count = np.zeros(int(out_size), np.int32), np.zeros(int(out_size), np.int32)
    weights = np.zeros((int(out_size), ksize.value), np.int32)
    _check(lib.jpezy_resize_taps_filter(int(filter), int(in_size), int(out_size), C.byref(ksize), _np_ptr(first), _np_ptr(count), _np_ptr(weights),
                                        weights.size))
    return first, count, weights


def resize_pick_window(W, H, src, out_w, out_h):
    """((x, y, w, h), scale): the window of decode_windows_resized_dev for the rectangle src = (x, y, w, h) of the full-size W x H picture and
    an output of out_w x out_h -- the largest scale of 8, 4, 2, 1 that leaves at least out_w x out_h pixels (jpezy_resize_pick_window)"""
    win = Window()
    _check(load_library().jpezy_resize_pick_window(int(W), int(H), C.byref(_rect(src)), int(out_w), int(out_h), C.byref(win)))
    return (win.region.x, win.region.y, win.region.w, win.region.h), win.scale_denom


def tensor_normalization(mean, std):
    """(scale, bias), float32 arrays of len(mean): scale[c] = 1 / (255 * std[c]) and bias[c] = -mean[c] / std[c], evaluated in binary64 and
    rounded once -- the constants with which decode_windows_tensor_dev's byte * scale + bias is (byte / 255 - mean) / std
    (jpezy_tensor_normalization).  mean and std: sequences of 3 or 1 numbers"""
    mean, std = np.atleast_1d(np.asarray(mean, dtype=np.float64)), np.atleast_1d(np.asarray(std, dtype=np.float64))
    if mean.ndim != 1 or mean.shape != std.shape:
        raise JpezyError("tensor_normalization: mean and std must be sequences of one length")
    scale, bias = np.zeros(mean.size, np.float32), np.zeros(mean.size, np.float32)
    _check(load_library().jpezy_tensor_normalization(int(mean.size), _np_ptr(mean), _np_ptr(std), _np_ptr(scale), _np_ptr(bias)))
    return scale, bias


def transform_geometry(op, W, H, sampling=SAMPLING_420, trim=False):
    """(Wout, Hout, src_cols, src_rows) of the lossless transform op (XFORM_*) of a W x H picture: the output's size and the source MCUs
    that are used; a mirrored axis with a partial MCU raises unless trim"""
    v = [C.c_int() for _ in range(4)]
    _check(load_library().jpezy_transform_geometry(int(op), XFORM_TRIM if trim else 0, int(W), int(H), int(sampling), *(C.byref(x) for x in v)))
    return tuple(x.value for x in v)


def quant_tables_transform(op, table):
    """the quantiser table (64 entries, natural order) of the transformed file: the transpose for the operations that swap the axes"""
    t = _table(table, "quant_tables_transform")
    out = np.zeros(64, np.uint8)
    _check(load_library().jpezy_quant_tables_transform(int(op), _np_ptr(t), _np_ptr(out)))
    return out


def ycc_chroma_size(W, H):
    """(CW, CH) = (ceil(W/2), ceil(H/2)): the chroma planes of a W x H picture in planar YCbCr 4:2:0 (I420 / NV12)"""
    cw, ch = C.c_int(), C.c_int()
    _check(load_library().jpezy_ycc_chroma_size(int(W), int(H), C.byref(cw), C.byref(ch)))
    return cw.value, ch.value


def ycc_component_size(info, comp):
    """(w, h) of component comp of a parsed file at its native sampling: ceil(W * H_c / hmax), ceil(H * V_c / vmax)"""
    w, h = C.c_int(), C.c_int()
    _check(load_library().jpezy_ycc_component_size(C.byref(info), int(comp), C.byref(w), C.byref(h)))
    return w.value, h.value


def yuv422_row_bytes(W):
    """4 * ceil(W/2): the bytes of a row of packed YCbCr 4:2:2 macropixels (YUY2 / UYVY / YVYU)"""
    return _check(load_library().jpezy_yuv422_row_bytes(int(W)))


def ycc422_chroma_size(W, H):
    """(CW, CH) = (ceil(W/2), H): the chroma planes of a W x H picture in planar YCbCr 4:2:2 (I422 / NV16)"""
    cw, ch = C.c_int(), C.c_int()
    _check(load_library().jpezy_ycc422_chroma_size(int(W), int(H), C.byref(cw), C.byref(ch)))
    return cw.value, ch.value


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _table(t, who):
    """one quantisation table: 64 entries, natural order, as a contiguous uint8 array (values outside 0..255 are refused here)"""
    a = np.asarray(t)
    if a.size != 64 or a.min() < 0 or a.max() > 255:
        raise JpezyError(f"{who}: a quantisation table is 64 entries in 0..255")
    return np.ascontiguousarray(a.reshape(64), dtype=np.uint8)


def quality_tables(quality):
    """(luma, chroma): the 64-entry tables (natural order, uint8) of libjpeg's quality 1..100 over the Annex-K tables; 50 is Annex K"""
    luma, chroma = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    _check(load_library().jpezy_quality_tables(int(quality), _np_ptr(luma), _np_ptr(chroma)))
    return luma, chroma


def quant_tables_probe(luma=None, chroma=None):
    """diagnostic, no GPU: (delta1 float32 [2, 8], dc_generic [2], qfrac_bits) -- what Context.set_quant_tables would build"""
    pl = None if luma is None else _table(luma, "quant_tables_probe")
    pc = None if chroma is None else _table(chroma, "quant_tables_probe")
    d1, dcg, bits = np.zeros((2, 8), np.float32), (C.c_int * 2)(), C.c_int()
    _check(load_library().jpezy_quant_tables_probe(None if pl is None else _np_ptr(pl), None if pc is None else _np_ptr(pc), _np_ptr(d1), dcg,
                                                   C.byref(bits)))
    return d1, [dcg[0], dcg[1]], bits.value


ANNEX_K_INFO = None


def annex_k_tables():
    """(qt[4][64] ctypes array, comp_tq) of a file written by jpezy_encode, parsed from a header-only file."""
    global ANNEX_K_INFO
    if ANNEX_K_INFO is None:
        z = np.zeros(6 * 64, dtype=np.int16)
        info, _ = read_jpeg(write_jpeg(z, 16, 16))
        ANNEX_K_INFO = info
    return ANNEX_K_INFO


class Context:
    """One per GPU: wraps jpezy_ctx (stream + device tables + staging)."""

    def __init__(self, device=0):
        lib = load_library()
        self._h = lib.jpezy_ctx_create(device)
        if not self._h:
            raise JpezyError("jpezy_ctx_create failed: " + lib.jpezy_hip_last_error().decode())
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            load_library().jpezy_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _check(load_library().jpezy_ctx_sync(self._h))

    def set_force_exact(self, on):
        load_library().jpezy_ctx_set_force_exact(self._h, int(on))

    def set_variant(self, variant):
        _check(load_library().jpezy_ctx_set_variant(self._h, int(variant)))

    def set_decode_tolerance(self, on):
        """0: bit-exact decode (default); 1: luma in FP32, every output byte within one of the reference's."""
        _check(load_library().jpezy_ctx_set_decode_tolerance(self._h, int(on)))

    def set_huffman_optimize(self, on):
        """0: Annex-K tables (default); 1: write_jpeg_gpu, encode_jpeg and encode_jpeg_packed give every frame its own optimal
        Huffman tables (the bytes of write_jpeg(..., optimize=True)); write_jpeg_gpu_dev is refused while it is on."""
        _check(load_library().jpezy_ctx_set_huffman_optimize(self._h, int(on)))

    def set_restart_interval(self, n):
        """MCUs per restart interval (0..65535; default 0: none) that write_jpeg_gpu[_dev], encode_jpeg and encode_jpeg_packed write:
        a DRI segment and RSTn markers, the bytes of write_jpeg(..., restart_interval=n); huffman_histogram_dev counts accordingly."""
        _check(load_library().jpezy_ctx_set_restart_interval(self._h, int(n)))

    def restart_interval(self):
        return _check(load_library().jpezy_ctx_restart_interval(self._h))

    def set_quant_tables(self, luma, chroma):
        """the quantisation tables (64 entries each, natural order, 1..255) of every encode entry point of this context and of the DQT
        segments write_jpeg_gpu[_dev] write; (None, None): back to Annex K.  Waits for the device when the setting changes; refused
        while the context's stream is being captured."""
        pl = None if luma is None else _table(luma, "set_quant_tables")
        pc = None if chroma is None else _table(chroma, "set_quant_tables")
        _check(load_library().jpezy_ctx_set_quant_tables(self._h, None if pl is None else _np_ptr(pl), None if pc is None else _np_ptr(pc)))

    def set_quality(self, quality):
        """set_quant_tables(*quality_tables(quality)): libjpeg's quality 1..100; 50 is the default"""
        _check(load_library().jpezy_ctx_set_quality(self._h, int(quality)))

    def quant_tables(self):
        """(luma, chroma) the context encodes with"""
        luma, chroma = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
        _check(load_library().jpezy_ctx_quant_tables(self._h, _np_ptr(luma), _np_ptr(chroma)))
        return luma, chroma

    def set_chroma_downsampling(self, mode):
        """DOWNSAMPLE_POINT (default): Cb and Cr of the top-left pixel of every 2x2, the reference's rule; DOWNSAMPLE_AVERAGE: the
        floor-averaged 2x2 with libjpeg's alternating bias (include/jpezy_hip.h, CHROMA DOWNSAMPLING).  Acts on every colour 4:2:0
        RGB transform of the context (fdct_quant[_dev], fdct_quant_packed_dev, encode_jpeg[_packed]) and, with its own horizontal
        (h2v1) rule, on every SAMPLING_422 one; gray, SAMPLING_444 and the planar-YCbCr entries do not consult it.  Refused with encode variant 0 when such a transform is launched."""
        _check(load_library().jpezy_ctx_set_chroma_downsampling(self._h, int(mode)))

    def chroma_downsampling(self):
        return _check(load_library().jpezy_ctx_chroma_downsampling(self._h))

    def set_dc_table_lookup(self, on):
        """test hook: the encode kernels read the quantised DC from the exact table even where the level-1 quantiser may take it"""
        load_library().jpezy_ctx_set_dc_table_lookup(self._h, int(on))

    def set_encode_groups(self, groups):
        """ENCODE_GROUPS_AUTO (default): the workgroup form of the planar RGB / gray 4:2:0 encode launch is chosen from the frame's
        geometry; ENCODE_GROUPS_4_COOP, _2_COOP, _2_DIRECT force one form (tests, A/B measurements: the same bits in every form).
        A launch whose frame the forced form is not legal for raises JpezyError (JPEZY_E_BADARG); include/jpezy_hip.h has the rules."""
        _check(load_library().jpezy_ctx_set_encode_groups(self._h, int(groups)))

    def encode_groups(self):
        return _check(load_library().jpezy_ctx_encode_groups(self._h))

    def stream(self):
        """the context's own hipStream_t as an integer"""
        return load_library().jpezy_ctx_stream(self._h)

    def set_host_chunk_bytes(self, n):
        """bytes of input per chunk of the streaming host-buffer entry points (default 4 MiB)"""
        load_library().jpezy_ctx_set_host_chunk_bytes(self._h, int(n))

    def fallback_count(self):
        return load_library().jpezy_ctx_last_fallback_count(self._h)

    # ---- host-buffer entry points (numpy) ----
    def fdct_quant(self, r, g, b, W, H, gray=False, n_frames=1):
        planes = [np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in (r, g, b)]
        for p in planes:
            if p.size != W * H * n_frames:
                raise JpezyError("plane size does not match W*H*n_frames")
        mc, mr = mcu_grid(W, H)
        out = np.empty((n_frames, mr, mc, 4 if gray else 6, 64), dtype=np.int16)
        _check(load_library().jpezy_fdct_quant(self._h, _np_ptr(planes[0]), _np_ptr(planes[1]), _np_ptr(planes[2]),
                                               W, H, int(gray), n_frames, _np_ptr(out)))
        return out[0] if n_frames == 1 else out

    def dequant_idct(self, coeffs, W, H, qt=None, comp_tq=(0, 1, 1), gray=False, n_frames=1):
        coeffs = np.ascontiguousarray(coeffs, dtype=np.int16)
        if coeffs.size != coeff_count(W, H, False) * n_frames:
            raise JpezyError("coefficient buffer size does not match the 6-block layout")
        qtab = qt if qt is not None else annex_k_tables().qt
        tq = (C.c_uint8 * 3)(*comp_tq)
        planes = [np.empty(W * H * n_frames, dtype=np.uint8) for _ in range(3)]
        _check(load_library().jpezy_dequant_idct(self._h, _np_ptr(coeffs), C.byref(qtab), C.byref(tq), W, H, int(gray),
                                                 n_frames, _np_ptr(planes[0]), _np_ptr(planes[1]), _np_ptr(planes[2])))
        return planes

    # ---- what the any-layout decode wrappers share ----
    def _stage_head(self, coeffs, info, gray):
        """the leading arguments of the any-layout transform entries: context, coefficients (a pointer), the FrameInfo's tables and
        layout (the sampling factors of absent components as 1), precision, size, gray"""
        hs = (C.c_uint8 * 3)(*[max(1, info.H[i]) for i in range(3)])
        vs = (C.c_uint8 * 3)(*[max(1, info.V[i]) for i in range(3)])
        tq = (C.c_uint8 * 3)(*[info.Tq[i] for i in range(3)])
        return (self._h, coeffs, C.byref(info.qt), info.ncomp, C.byref(hs), C.byref(vs), C.byref(tq), info.precision or 8,
                info.width, info.height, int(gray))

    def _decode_planes(self, fn, data, args, size):
        """a jpezy_decode_jpeg* entry that writes three planes: the header call (null planes), the allocation -- size(info) bytes a
        plane --, the decode call.  args: the entry's arguments between len and info."""
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        info = FrameInfo()
        _check(fn(self._h, _np_ptr(arr), arr.size, *args, C.byref(info), None, None, None, 0))
        n = size(info)
        r, g, b = (np.empty(n, dtype=np.uint8) for _ in range(3))
        _check(fn(self._h, _np_ptr(arr), arr.size, *args, C.byref(info), _np_ptr(r), _np_ptr(g), _np_ptr(b), n))
        return info, r, g, b

    def _decode_packed(self, fn, data, args, format, size):
        """the same for an entry that writes packed pixels: size(info) is (width, height) of the image"""
        nb = pixel_bytes(format)
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        info = FrameInfo()
        _check(fn(self._h, _np_ptr(arr), arr.size, *args, C.byref(info), int(format), 0, None, 0))
        w, h = size(info)
        img = np.empty((h, w, nb), dtype=np.uint8)
        _check(fn(self._h, _np_ptr(arr), arr.size, *args, C.byref(info), int(format), 0, _np_ptr(img), img.size))
        return info, img

    def dequant_idct_generic(self, coeffs, info, gray=False):
        """any baseline layout (1/3 components, sampling 1..4): info is the FrameInfo of read_jpeg"""
        coeffs = np.ascontiguousarray(coeffs, dtype=np.int16)
        W, H = info.width, info.height
        planes = [np.empty(W * H, dtype=np.uint8) for _ in range(3)]
        _check(load_library().jpezy_dequant_idct_generic(*self._stage_head(_np_ptr(coeffs), info, gray)[:7], W, H, int(gray),
                                                         _np_ptr(planes[0]), _np_ptr(planes[1]), _np_ptr(planes[2])))
        return planes

    def dequant_idct_generic_dev(self, d_coeffs, info, d_r, d_g, d_b, gray=False, stream=None, n_frames=1, plane_stride=None):
        """any-layout decode on device memory (torch tensors): coefficients as read_jpeg_gpu leaves them -> planes; n_frames > 1:
        that many frames of the layout in one pair of launches (jpezy_dequant_idct_generic_batch_dev)"""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(d_coeffs.device).cuda_stream
        head = self._stage_head(d_coeffs.data_ptr(), info, gray)
        if n_frames == 1 and plane_stride is None:
            _check(load_library().jpezy_dequant_idct_generic_dev(*head, d_r.data_ptr(), d_g.data_ptr(), d_b.data_ptr(), stream))
        else:       # n_frames frames of this layout: coefficients frame after frame, planes plane_stride apart
            stride = plane_stride if plane_stride is not None else info.width * info.height
            _check(load_library().jpezy_dequant_idct_generic_batch_dev(*head, n_frames, stride, d_r.data_ptr(), d_g.data_ptr(), d_b.data_ptr(),
                                                                       stream))

    # ---- device-pointer entry points (torch tensors on this context's device) ----
    def fdct_quant_dev(self, d_r, d_g, d_b, W, H, d_coeffs, gray=False, n_frames=1, plane_stride=None, stream=None, sampling=SAMPLING_420):
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(d_r.device).cuda_stream
        stride = plane_stride if plane_stride is not None else W * H
        if sampling != SAMPLING_420:      # d_coeffs: coeff_count(W, H, sampling=sampling) elements per frame
            _check(load_library().jpezy_fdct_quant_sampling_dev(self._h, d_r.data_ptr(), d_g.data_ptr(), d_b.data_ptr(), stride, W, H,
                                                                int(sampling), int(gray), n_frames, d_coeffs.data_ptr(), stream))
            return
        _check(load_library().jpezy_fdct_quant_dev(self._h, d_r.data_ptr(), d_g.data_ptr(), d_b.data_ptr(), stride, W, H,
                                                   int(gray), n_frames, d_coeffs.data_ptr(), stream))

    # ---- entropy coding on the GPU: same bytes as write_jpeg ----
    def write_jpeg_gpu(self, d_coeffs, W, H, gray=False, comment=None, n_frames=1, sampling=SAMPLING_420, raise_on_error=True):
        """Device coefficients (torch int16 tensor, the output of fdct_quant_dev; its producing stream must be
        synchronised) -> list of .jpg bytes, Huffman coding + bit packing + byte stuffing on the GPU.
        sampling=SAMPLING_444 / SAMPLING_422: coefficients of 3- / 4-block MCUs; raise_on_error=False (that form only): a frame that failed is its negative
        status in the list instead of an exception for the whole call."""
        lib = load_library()
        if comment is None:
            comment = b"Encoded by JPEZY" if gray else b"Encoded by jpezy"
        if sampling != SAMPLING_420:
            cap = jpeg_bound(W, H, sampling)
            buf = np.empty(cap * n_frames, dtype=np.uint8)
            sizes = (C.c_long * n_frames)()
            rc = lib.jpezy_write_jpeg_gpu_sampling_batch(self._h, d_coeffs.data_ptr(), W, H, int(sampling), int(gray), n_frames, comment,
                                                         _np_ptr(buf), cap, sizes)
            if raise_on_error or (rc < 0 and all(n >= 0 for n in sizes)):
                _check(rc)
            return [buf[f * cap: f * cap + sizes[f]].tobytes() if sizes[f] >= 0 else int(sizes[f]) for f in range(n_frames)]
        cap = lib.jpezy_jpeg_bound(W, H)
        buf = np.empty(cap * n_frames, dtype=np.uint8)
        sizes = (C.c_long * n_frames)()
        rc = lib.jpezy_write_jpeg_gpu_batch(self._h, d_coeffs.data_ptr(), W, H, int(gray), n_frames, comment, _np_ptr(buf), cap, sizes)
        _check(rc)
        return [buf[f * cap: f * cap + sizes[f]].tobytes() for f in range(n_frames)]

    def write_jpeg_gpu_dev(self, d_coeffs, W, H, d_out, d_sizes, gray=False, comment=None, n_frames=1, stream=None, sampling=SAMPLING_420):
        """Asynchronous, device-resident: d_out is a torch uint8 tensor [n_frames, out_stride], d_sizes int64 [n_frames];
        every frame's complete .jpg is left in d_out[f, :d_sizes[f]]."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(d_coeffs.device).cuda_stream
        if comment is None:
            comment = b"Encoded by JPEZY" if gray else b"Encoded by jpezy"
        stride = d_out.numel() // n_frames
        if sampling != SAMPLING_420:
            _check(load_library().jpezy_write_jpeg_gpu_sampling_dev(self._h, d_coeffs.data_ptr(), W, H, int(sampling), int(gray), n_frames, comment,
                                                                    d_out.data_ptr(), stride, d_sizes.data_ptr(), stream))
            return
        _check(load_library().jpezy_write_jpeg_gpu_dev(self._h, d_coeffs.data_ptr(), W, H, int(gray), n_frames, comment,
                                                       d_out.data_ptr(), stride, d_sizes.data_ptr(), stream))

    def huffman_histogram_dev(self, d_coeffs, W, H, d_hist, gray=False, n_frames=1, stream=None, sampling=SAMPLING_420):
        """Asynchronous: d_hist (torch int64 tensor [n_frames, 4, 256] on the device) receives the frames' symbol counts, table k in
        DHT order YDc, CDc, YAc, CAc."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(d_coeffs.device).cuda_stream
        if d_hist.numel() != n_frames * 4 * 256 or d_hist.element_size() != 8 or not d_hist.is_contiguous():
            raise JpezyError("huffman_histogram_dev: d_hist must be a contiguous 64-bit tensor of n_frames * 4 * 256 elements")
        if sampling != SAMPLING_420:
            _check(load_library().jpezy_huffman_histogram_sampling_dev(self._h, d_coeffs.data_ptr(), W, H, int(sampling), int(gray), n_frames,
                                                                       d_hist.data_ptr(), stream))
            return
        _check(load_library().jpezy_huffman_histogram_dev(self._h, d_coeffs.data_ptr(), W, H, int(gray), n_frames, d_hist.data_ptr(), stream))

    def read_jpeg_gpu(self, data):
        """.jpg bytes -> (FrameInfo, torch int16 tensor [mcu_rows, mcu_cols, blocks_per_mcu, 64] on the device): header
        parsed on the host, Huffman decoding on the GPU (restart intervals as independent streams; the host decoder for anything irregular)."""
        import torch
        lib = load_library()
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        info = FrameInfo()
        _check(lib.jpezy_read_jpeg_gpu(self._h, _np_ptr(arr), arr.size, C.byref(info), None, 0))
        co = torch.empty((info.mcu_rows, info.mcu_cols, info.blocks_per_mcu, 64), dtype=torch.int16, device=f"cuda:{self.device}")
        _check(lib.jpezy_read_jpeg_gpu(self._h, _np_ptr(arr), arr.size, C.byref(info), co.data_ptr(), co.numel()))
        return info, co

    def read_jpeg_gpu_into(self, arr, d_coeffs):
        """read_jpeg_gpu without the header-only call or an allocation: arr a contiguous numpy uint8 array holding the file,
        d_coeffs a torch int16 tensor on this context's device with room for the frame's coefficients; returns FrameInfo."""
        info = FrameInfo()
        _check(load_library().jpezy_read_jpeg_gpu(self._h, _np_ptr(arr), arr.size, C.byref(info), d_coeffs.data_ptr(), d_coeffs.numel()))
        return info

    def decode_jpeg(self, data, gray=False, upsampling=UPSAMPLE_NEAREST):
        """.jpg bytes -> (FrameInfo, r, g, b) planes of width*height bytes (decoder::decode end to end).  upsampling=UPSAMPLE_SMOOTH:
        2:1 chroma through the triangle filter (decode_jpeg_upsampling)."""
        if upsampling != UPSAMPLE_NEAREST:
            return self.decode_jpeg_upsampling(data, upsampling, gray=gray)
        return self._decode_planes(load_library().jpezy_decode_jpeg, data, (int(gray),), lambda info: info.width * info.height)

    def decode_jpeg_batch(self, files, gray=False, raise_on_error=True):
        """list of .jpg byte strings -> list of (FrameInfo, r, g, b) (None for a file that failed when raise_on_error is
        False); the files are decoded concurrently on this context's device (jpezy_decode_jpeg_batch)."""
        lib = load_library()
        n = len(files)
        arrs = [np.frombuffer(bytes(f), dtype=np.uint8) for f in files]
        infos = (FrameInfo * n)()
        sizes = []
        for i, a in enumerate(arrs):          # header pass on the host: plane sizes
            rc = lib.jpezy_decode_jpeg(self._h, _np_ptr(a), a.size, int(gray), C.byref(infos[i]), None, None, None, 0)
            sizes.append(infos[i].width * infos[i].height if rc == 0 else 0)
        planes = [[np.empty(max(sz, 1), dtype=np.uint8) for _ in range(3)] for sz in sizes]
        vpa = C.c_void_p * n
        data = vpa(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * n)(*[a.size for a in arrs])
        rr, gg, bb = (vpa(*[p[k].ctypes.data for p in planes]) for k in range(3))
        caps = (C.c_size_t * n)(*sizes)
        status = (C.c_int * n)()
        rc = lib.jpezy_decode_jpeg_batch(self._h, n, data, lens, int(gray), infos, rr, gg, bb, caps, status)
        if rc != 0 and raise_on_error:
            _check(rc)
        out = []
        for i in range(n):
            if status[i] != 0:
                out.append(None)
                continue
            fi = FrameInfo()
            C.memmove(C.byref(fi), C.byref(infos[i]), C.sizeof(FrameInfo))
            out.append((fi, planes[i][0][: sizes[i]], planes[i][1][: sizes[i]], planes[i][2][: sizes[i]]))
        return out

    def decode_windows_dev(self, files, d_out, windows=None, format=PIX_RGB24, gray=False, raise_on_error=True, upsampling=None):
        """one crop window of each of the .jpg byte strings in `files` (sizes mixed) as packed pixels into d_out, a torch uint8 tensor
        [n, Hs, Ws, bytes] on this context's device with stride(3) == 1 and stride(2) == bytes; rows are stride(1) apart, slots stride(0).
        windows: None (whole pictures at full size) or a list of None, (x, y, w, h) or ((x, y, w, h), scale), in the picture at 1/scale.
        File k's window lands at d_out[k, :h, :w]; nothing else of d_out is written.  Returns a list of (FrameInfo, (x, y, w, h), status);
        synchronous (jpezy_decode_windows_dev).  upsampling: None (the context's setting, set_windows_upsampling) or a value that holds for
        this call alone."""
        if upsampling is not None:
            with self._windows_upsampling(upsampling):
                return self.decode_windows_dev(files, d_out, windows, format, gray, raise_on_error)
        lib = load_library()
        n = len(files)
        nb = pixel_bytes(format)
        if d_out.dim() != 4 or str(d_out.dtype) != "torch.uint8" or not d_out.is_cuda or d_out.device.index != self.device:
            raise JpezyError("decode_windows_dev: d_out must be a uint8 tensor [n, Hs, Ws, bytes] on the context's device")
        if d_out.shape[0] != n or d_out.shape[3] != nb or (n and (d_out.stride(3) != 1 or d_out.stride(2) != nb)):
            raise JpezyError(f"decode_windows_dev: d_out must hold {n} slots of pixels of {nb} contiguous bytes")
        if windows is not None and len(windows) != n:
            raise JpezyError("decode_windows_dev: one window per file")
        arrs = [np.frombuffer(bytes(f), dtype=np.uint8) for f in files]
        data = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
        wins = (Window * max(n, 1))(*[_window(w) for w in windows]) if windows is not None else None
        infos, placed, status = (FrameInfo * max(n, 1))(), (Rect * max(n, 1))(), (C.c_int * max(n, 1))()
        row, slot = (d_out.stride(1), d_out.stride(0)) if n else (1, 1)
        # pix_cap: what the tensor's storage holds behind its first byte (n whole slots must lie inside it)
        cap = d_out.untyped_storage().nbytes() - d_out.storage_offset() if n else 0
        rc = lib.jpezy_decode_windows_dev(self._h, n, data, lens, int(gray), wins, int(format), row, slot, d_out.data_ptr() if n else None, cap,
                                          infos, placed, status)
        if rc != 0 and raise_on_error:
            _check(rc)
        out = []
        for i in range(n):
            fi = FrameInfo()
            C.memmove(C.byref(fi), C.byref(infos[i]), C.sizeof(FrameInfo))
            out.append((fi, (placed[i].x, placed[i].y, placed[i].w, placed[i].h), status[i]))
        return out

    def decode_windows_resized_dev(self, files, d_out, windows=None, mirror=None, format=PIX_RGB24, gray=False, raise_on_error=True,
                                   upsampling=None, filter=None):
        """one crop window of each of the .jpg byte strings in `files`, every window of its own size, each resampled (triangle filter,
        antialiased where it shrinks; include/jpezy_hip.h, BATCH OF WINDOWS, RESIZED) to the out_h x out_w of d_out, a torch uint8 tensor
        [n, out_h, out_w, bytes] under decode_windows_dev's stride rules.  windows: as there (resize_pick_window gives the window and scale
        for a rectangle of the full-size picture); mirror: None or one flag per file, the file's output columns reversed.  Every file writes
        exactly d_out[k]; nothing else of d_out's storage is written.  Returns a list of (FrameInfo, (x, y, w, h), status), the rectangle
        being the source window as decoded; synchronous (jpezy_decode_windows_resized_dev).  upsampling: as decode_windows_dev's (the
        source window's chroma; the resampling behind it is the same).  filter: None (the context's setting, set_windows_filter) or one
        of FILTER_* that holds for this call alone."""
        if filter is not None:
            with self._windows_filter(filter):
                return self.decode_windows_resized_dev(files, d_out, windows, mirror, format, gray, raise_on_error, upsampling)
        if upsampling is not None:
            with self._windows_upsampling(upsampling):
                return self.decode_windows_resized_dev(files, d_out, windows, mirror, format, gray, raise_on_error)
        lib = load_library()
        n = len(files)
        nb = pixel_bytes(format)
        if d_out.dim() != 4 or str(d_out.dtype) != "torch.uint8" or not d_out.is_cuda or d_out.device.index != self.device:
            raise JpezyError("decode_windows_resized_dev: d_out must be a uint8 tensor [n, out_h, out_w, bytes] on the context's device")
        if d_out.shape[0] != n or d_out.shape[3] != nb or (n and (d_out.stride(3) != 1 or d_out.stride(2) != nb)):
            raise JpezyError(f"decode_windows_resized_dev: d_out must hold {n} slots of pixels of {nb} contiguous bytes")
        if windows is not None and len(windows) != n:
            raise JpezyError("decode_windows_resized_dev: one window per file")
        if mirror is not None and len(mirror) != n:
            raise JpezyError("decode_windows_resized_dev: one mirror flag per file")
        arrs = [np.frombuffer(bytes(f), dtype=np.uint8) for f in files]
        data = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
        wins = (Window * max(n, 1))(*[_window(w) for w in windows]) if windows is not None else None
        flags = (C.c_uint8 * max(n, 1))(*[1 if m else 0 for m in mirror]) if mirror is not None else None
        infos, placed, status = (FrameInfo * max(n, 1))(), (Rect * max(n, 1))(), (C.c_int * max(n, 1))()
        row, slot = (d_out.stride(1), d_out.stride(0)) if n else (0, 0)
        cap = d_out.untyped_storage().nbytes() - d_out.storage_offset() if n else 0
        rc = lib.jpezy_decode_windows_resized_dev(self._h, n, data, lens, int(gray), wins, flags, int(d_out.shape[2]), int(d_out.shape[1]), int(format),
                                                  row, slot, d_out.data_ptr() if n else None, cap, infos, placed, status)
        if rc != 0 and raise_on_error:
            _check(rc)
        out = []
        for i in range(n):
            fi = FrameInfo()
            C.memmove(C.byref(fi), C.byref(infos[i]), C.sizeof(FrameInfo))
            out.append((fi, (placed[i].x, placed[i].y, placed[i].w, placed[i].h), status[i]))
        return out

    def decode_windows_tensor_dev(self, files, d_out, windows=None, mirror=None, scale=None, bias=None, format=PIX_RGB24, gray=False,
                                  raise_on_error=True, upsampling=None, filter=None):
        """decode_windows_resized_dev straight into the tensor a model takes (include/jpezy_hip.h, BATCH OF WINDOWS, TENSOR OUTPUT): d_out is a
        torch tensor of LOGICAL shape [n, C, out_h, out_w] on this context's device, C = 3 or 1 (1 needs gray), dtype uint8, float32, float16
        or bfloat16, with ANY strides -- torch.empty(n, 3, H, W), the same in channels_last and nhwc.permute(0, 3, 1, 2) all work; the dtype
        and the strides are read from the tensor.  Element (k, c, y, x) is byte c of the resized pixel (format: PIX_RGB24 or PIX_BGR24), for
        the float types byte * scale[c] + bias[c] in float32 (two roundings, never fused) converted to the dtype; scale and bias: None (1
        and 0; required for uint8) or C numbers each, tensor_normalization(mean, std) gives them for (byte / 255 - mean) / std.  Only d_out's
        own elements are written.  windows, mirror, upsampling, filter and the returned list: as decode_windows_resized_dev's; synchronous
        (jpezy_decode_windows_tensor_dev)."""
        if filter is not None:
            with self._windows_filter(filter):
                return self.decode_windows_tensor_dev(files, d_out, windows, mirror, scale, bias, format, gray, raise_on_error, upsampling)
        if upsampling is not None:
            with self._windows_upsampling(upsampling):
                return self.decode_windows_tensor_dev(files, d_out, windows, mirror, scale, bias, format, gray, raise_on_error)
        import torch
        lib = load_library()
        n = len(files)
        dtypes = {torch.uint8: DT_U8, torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16}
        if d_out.dim() != 4 or d_out.dtype not in dtypes or not d_out.is_cuda or d_out.device.index != self.device:
            raise JpezyError("decode_windows_tensor_dev: d_out must be a uint8, float32, float16 or bfloat16 tensor [n, C, out_h, out_w] on the "
                             "context's device")
        if d_out.shape[0] != n:
            raise JpezyError(f"decode_windows_tensor_dev: d_out must hold {n} files")
        if windows is not None and len(windows) != n:
            raise JpezyError("decode_windows_tensor_dev: one window per file")
        if mirror is not None and len(mirror) != n:
            raise JpezyError("decode_windows_tensor_dev: one mirror flag per file")
        if (scale is None) != (bias is None):
            raise JpezyError("decode_windows_tensor_dev: scale and bias are given together or not at all")
        channels = int(d_out.shape[1])
        if scale is not None:
            scale, bias = (np.ascontiguousarray(np.atleast_1d(np.asarray(v, dtype=np.float32))) for v in (scale, bias))
            if scale.shape != (channels,) or bias.shape != (channels,):
                raise JpezyError(f"decode_windows_tensor_dev: scale and bias must hold {channels} values each")
        arrs = [np.frombuffer(bytes(f), dtype=np.uint8) for f in files]
        data = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
        wins = (Window * max(n, 1))(*[_window(w) for w in windows]) if windows is not None else None
        flags = (C.c_uint8 * max(n, 1))(*[1 if m else 0 for m in mirror]) if mirror is not None else None
        infos, placed, status = (FrameInfo * max(n, 1))(), (Rect * max(n, 1))(), (C.c_int * max(n, 1))()
        # cap_elems: what the tensor's storage holds behind its first element
        cap = d_out.untyped_storage().nbytes() // d_out.element_size() - d_out.storage_offset() if n else 0
        rc = lib.jpezy_decode_windows_tensor_dev(self._h, n, data, lens, int(gray), wins, flags, int(d_out.shape[3]), int(d_out.shape[2]), int(format),
                                                 dtypes[d_out.dtype], channels, _np_ptr(scale) if scale is not None else None,
                                                 _np_ptr(bias) if bias is not None else None, *[int(v) for v in d_out.stride()],
                                                 d_out.data_ptr() if n else None, cap, infos, placed, status)
        if rc != 0 and raise_on_error:
            _check(rc)
        out = []
        for i in range(n):
            fi = FrameInfo()
            C.memmove(C.byref(fi), C.byref(infos[i]), C.sizeof(FrameInfo))
            out.append((fi, (placed[i].x, placed[i].y, placed[i].w, placed[i].h), status[i]))
        return out

    def set_windows_slice_files(self, n):
        """files per slice of decode_windows_dev's grouped path; 0: automatic (a test and measurement knob)"""
        _check(load_library().jpezy_ctx_set_windows_slice_files(self._h, int(n)))

    def set_windows_upsampling(self, upsampling):
        """chroma upsampling of decode_windows_dev and decode_windows_resized_dev: UPSAMPLE_NEAREST (the default) or UPSAMPLE_SMOOTH
        (jpezy_ctx_set_windows_upsampling); any other value raises and leaves the setting unchanged"""
        _check(load_library().jpezy_ctx_set_windows_upsampling(self._h, int(upsampling)))

    def windows_upsampling(self):
        """the setting of set_windows_upsampling"""
        return _check(load_library().jpezy_ctx_windows_upsampling(self._h))

    @contextlib.contextmanager
    def _windows_upsampling(self, upsampling):
        """the setting for one call: set, and put back afterwards whatever the call did"""
        before = self.windows_upsampling()
        self.set_windows_upsampling(upsampling)
        try:
            yield
        finally:
            self.set_windows_upsampling(before)

    def set_windows_filter(self, filter):
        """resampling filter of decode_windows_resized_dev and decode_windows_tensor_dev: FILTER_BILINEAR (the default), FILTER_BOX,
        FILTER_BICUBIC or FILTER_LANCZOS (jpezy_ctx_set_windows_filter); any other value raises and leaves the setting unchanged"""
        _check(load_library().jpezy_ctx_set_windows_filter(self._h, int(filter)))

    def windows_filter(self):
        """the setting of set_windows_filter"""
        return _check(load_library().jpezy_ctx_windows_filter(self._h))

    @contextlib.contextmanager
    def _windows_filter(self, filter):
        """the setting for one call: set, and put back afterwards whatever the call did"""
        before = self.windows_filter()
        self.set_windows_filter(filter)
        try:
            yield
        finally:
            self.set_windows_filter(before)

    def set_resample_direct(self, on):
        """on: box, bicubic and Lanczos resample every file with the direct loop, never the two-pass tile (a test and measurement knob; the
        bytes do not depend on it)"""
        _check(load_library().jpezy_ctx_set_resample_direct(self._h, 1 if on else 0))

    def last_resample_tiled_count(self):
        """files of the last decode_windows_resized_dev / decode_windows_tensor_dev call that took the two-pass tile"""
        return load_library().jpezy_ctx_last_resample_tiled_count(self._h)

    def set_huffdec_min_bytes(self, n):
        load_library().jpezy_ctx_set_huffdec_min_bytes(self._h, n)

    def last_batch_fast_count(self):
        """files of the last decode_jpeg_batch call that took the batch form of the Huffman decoder kernels"""
        return load_library().jpezy_ctx_last_batch_fast_count(self._h)

    def last_huffdec_passes(self):
        """synchronisation passes of the last read_jpeg_gpu call; 0 = the host decoder was used"""
        return load_library().jpezy_ctx_last_huffdec_passes(self._h)

    def encode_jpeg(self, r, g, b, W, H, gray=False, comment=None, sampling=SAMPLING_420):
        """Host planes -> .jpg bytes, both stages on the GPU (encoder::encode end to end).  sampling=SAMPLING_444: a 4:4:4 file; SAMPLING_422: a 4:2:2 file
        (the context's chroma-downsampling setting acts on it)."""
        lib = load_library()
        r, g, b = (np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in (r, g, b))
        if not (r.size == g.size == b.size == W * H):
            raise JpezyError("plane size does not match W*H")
        if comment is None:
            comment = b"Encoded by JPEZY" if gray else b"Encoded by jpezy"
        if sampling != SAMPLING_420:
            cap = jpeg_bound(W, H, sampling)
            buf = np.empty(cap, dtype=np.uint8)
            n = _check(lib.jpezy_encode_jpeg_sampling(self._h, _np_ptr(r), _np_ptr(g), _np_ptr(b), W, H, int(sampling), int(gray), comment,
                                                      _np_ptr(buf), cap))
            return buf[:n].tobytes()
        cap = lib.jpezy_jpeg_bound(W, H)
        buf = np.empty(cap, dtype=np.uint8)
        n = lib.jpezy_encode_jpeg(self._h, _np_ptr(r), _np_ptr(g), _np_ptr(b), W, H, int(gray), comment, _np_ptr(buf), cap)
        _check(n)
        return buf[:n].tobytes()

    def dequant_idct_dev(self, d_coeffs, W, H, d_r, d_g, d_b, qt=None, comp_tq=(0, 1, 1), gray=False, n_frames=1,
                         plane_stride=None, stream=None):
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(d_coeffs.device).cuda_stream
        qtab = qt if qt is not None else annex_k_tables().qt
        tq = (C.c_uint8 * 3)(*comp_tq)
        stride = plane_stride if plane_stride is not None else W * H
        _check(load_library().jpezy_dequant_idct_dev(self._h, d_coeffs.data_ptr(), C.byref(qtab), C.byref(tq), stride, W, H,
                                                     int(gray), n_frames, d_r.data_ptr(), d_g.data_ptr(), d_b.data_ptr(),
                                                     stream))

    # ---- packed (interleaved) pixels ----
    def encode_jpeg_packed(self, img, format=PIX_RGB24, gray=False, comment=None, sampling=SAMPLING_420):
        """numpy uint8 (H, W, C) interleaved pixels -> .jpg bytes (the bytes encode_jpeg gives for the same pixels).  Taken as it is,
        without a copy, whenever strides[2] == 1 and strides[1] == C: strides[0] becomes row_stride, so a cropped view encodes in place."""
        lib = load_library()
        nb = pixel_bytes(format)
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != nb:
            raise JpezyError(f"encode_jpeg_packed: a uint8 array of shape (H, W, {nb}) is expected")
        if not (img.strides[2] == 1 and img.strides[1] == nb and img.strides[0] >= img.shape[1] * nb):
            img = np.ascontiguousarray(img)
        H, W = img.shape[:2]
        if comment is None:
            comment = b"Encoded by JPEZY" if gray else b"Encoded by jpezy"
        if sampling != SAMPLING_420:
            cap = jpeg_bound(W, H, sampling)
            buf = np.empty(cap, dtype=np.uint8)
            n = _check(lib.jpezy_encode_jpeg_sampling_packed(self._h, _np_ptr(img), int(format), img.strides[0], W, H, int(sampling), int(gray),
                                                             comment, _np_ptr(buf), cap))
            return buf[:n].tobytes()
        cap = lib.jpezy_jpeg_bound(W, H)
        buf = np.empty(cap, dtype=np.uint8)
        n = lib.jpezy_encode_jpeg_packed(self._h, _np_ptr(img), int(format), img.strides[0], W, H, int(gray), comment, _np_ptr(buf), cap)
        _check(n)
        return buf[:n].tobytes()

    def decode_jpeg_packed(self, data, format=PIX_RGB24, gray=False, upsampling=UPSAMPLE_NEAREST):
        """.jpg bytes -> (FrameInfo, uint8 array (H, W, C)) of interleaved pixels; the fourth byte of a 32-bit format is 0xFF.
        upsampling=UPSAMPLE_SMOOTH: decode_jpeg_upsampling_packed."""
        if upsampling != UPSAMPLE_NEAREST:
            return self.decode_jpeg_upsampling_packed(data, upsampling, format=format, gray=gray)
        return self._decode_packed(load_library().jpezy_decode_jpeg_packed, data, (int(gray),), format, lambda info: (info.width, info.height))

    @staticmethod
    def _packed_layout(d_img, nb, who):
        """(n_frames, H, W, row_stride, frame_stride) of a torch uint8 tensor (H, W, C) or (N, H, W, C) whose pixels are interleaved"""
        import torch
        if d_img.dtype != torch.uint8 or d_img.dim() not in (3, 4) or d_img.shape[-1] != nb:
            raise JpezyError(f"{who}: a uint8 tensor of shape (H, W, {nb}) or (N, H, W, {nb}) is expected")
        if d_img.stride(-1) != 1 or d_img.stride(-2) != nb:
            raise JpezyError(f"{who}: the pixels are not interleaved (stride(-1) must be 1 and stride(-2) {nb})")
        H, W = int(d_img.shape[-3]), int(d_img.shape[-2])
        n = int(d_img.shape[0]) if d_img.dim() == 4 else 1
        row = int(d_img.stride(-3))
        frame = int(d_img.stride(0)) if d_img.dim() == 4 and n > 1 else 0
        return n, H, W, row, frame

    def fdct_quant_packed_dev(self, d_img, d_coeffs, format=PIX_RGB24, gray=False, stream=None, sampling=SAMPLING_420):
        """device packed pixels (torch uint8 (H, W, C) or (N, H, W, C); row and frame strides are the tensor's) -> d_coeffs"""
        import torch
        n, H, W, row, frame = self._packed_layout(d_img, pixel_bytes(format), "fdct_quant_packed_dev")
        if stream is None:
            stream = torch.cuda.current_stream(d_img.device).cuda_stream
        if sampling != SAMPLING_420:
            _check(load_library().jpezy_fdct_quant_sampling_packed_dev(self._h, d_img.data_ptr(), int(format), row, frame, W, H, int(sampling),
                                                                       int(gray), n, d_coeffs.data_ptr(), stream))
            return
        _check(load_library().jpezy_fdct_quant_packed_dev(self._h, d_img.data_ptr(), int(format), row, frame, W, H, int(gray), n,
                                                          d_coeffs.data_ptr(), stream))

    def dequant_idct_packed_dev(self, d_coeffs, d_img, format=PIX_RGB24, qt=None, comp_tq=(0, 1, 1), gray=False, stream=None):
        """device coefficients (6-block layout) -> device packed pixels written into d_img (layout as for fdct_quant_packed_dev)"""
        import torch
        n, H, W, row, frame = self._packed_layout(d_img, pixel_bytes(format), "dequant_idct_packed_dev")
        if stream is None:
            stream = torch.cuda.current_stream(d_coeffs.device).cuda_stream
        qtab = qt if qt is not None else annex_k_tables().qt
        tq = (C.c_uint8 * 3)(*comp_tq)
        _check(load_library().jpezy_dequant_idct_packed_dev(self._h, d_coeffs.data_ptr(), C.byref(qtab), C.byref(tq), int(format), row, frame,
                                                            W, H, int(gray), n, d_img.data_ptr(), stream))

    # ---- planar YCbCr 4:2:0 samples (I420 / YV12 / NV12 / NV21): the file's own sample domain, no colour conversion ----
    def encode_jpeg_ycc(self, y, cb=None, cr=None, gray=False, comment=None):
        """2-D numpy uint8 planes -> .jpg bytes: y (H, W), cb and cr (ceil(H/2), ceil(W/2)).  Strides and c_step are read from the arrays,
        so uv[..., 0], uv[..., 1] of an NV12 plane (H/2, W/2, 2) encode in place.  gray: luma only, cb and cr are not read."""
        lib = load_library()
        y = np.asarray(y)
        if y.dtype != np.uint8 or y.ndim != 2:
            raise JpezyError("encode_jpeg_ycc: y must be a 2-D uint8 array")
        H, W = y.shape
        if y.strides[1] != 1 or y.strides[0] < W:
            y = np.ascontiguousarray(y)
        c_stride, c_step, pcb, pcr = 0, 1, None, None
        if not gray:
            cw, ch = ycc_chroma_size(W, H)
            cb, cr = np.asarray(cb), np.asarray(cr)
            for c in (cb, cr):
                if c.dtype != np.uint8 or c.shape != (ch, cw):
                    raise JpezyError(f"encode_jpeg_ycc: cb and cr must be uint8 arrays of shape ({ch}, {cw})")
            ok = cb.strides == cr.strides and cb.strides[1] in (1, 2) and cb.strides[0] >= (cw - 1) * cb.strides[1] + 1
            if not ok:
                cb, cr = np.ascontiguousarray(cb), np.ascontiguousarray(cr)
            c_stride, c_step = (cb.strides[0] if ch > 1 else 0), (cb.strides[1] if cw > 1 else 1)
            pcb, pcr = _np_ptr(cb), _np_ptr(cr)
        if comment is None:
            comment = b"Encoded by JPEZY" if gray else b"Encoded by jpezy"
        cap = lib.jpezy_jpeg_bound(W, H)
        buf = np.empty(cap, dtype=np.uint8)
        n = lib.jpezy_encode_jpeg_ycc(self._h, _np_ptr(y), y.strides[0] if H > 1 else 0, pcb, pcr, c_stride, c_step, W, H, int(gray), comment,
                                      _np_ptr(buf), cap)
        _check(n)
        return buf[:n].tobytes()

    def decode_jpeg_ycc(self, data, interleaved=False):
        """.jpg bytes -> (FrameInfo, y, cb, cr): the components at their native sampling as 2-D uint8 arrays (no upsampling, no colour
        conversion; cb = cr = None for a one-component file).  interleaved: cb and cr are the two views uv[..., 0], uv[..., 1] of one
        (h, w, 2) array (NV12)."""
        lib = load_library()
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        info = FrameInfo()
        _check(lib.jpezy_decode_jpeg_ycc(self._h, _np_ptr(arr), arr.size, C.byref(info), None, 0, 0, None, None, 0, 1, 0))
        w0, h0 = ycc_component_size(info, 0)
        y = np.empty((h0, w0), dtype=np.uint8)
        cb = cr = pcb = pcr = None
        c_stride, c_step, c_cap = 0, 1, 0
        if info.ncomp == 3:
            (w1, h1), (w2, h2) = ycc_component_size(info, 1), ycc_component_size(info, 2)
            if interleaved and (w1, h1) == (w2, h2):
                uv = np.empty((h1, w1, 2), dtype=np.uint8)
                cb, cr = uv[..., 0], uv[..., 1]
                c_stride, c_step, c_cap = 2 * w1, 2, uv.size - 1
            else:
                wm = max(w1, w2)
                cb, cr = np.empty((h1, wm), dtype=np.uint8)[:, :w1], np.empty((h2, wm), dtype=np.uint8)[:, :w2]
                c_stride, c_cap = wm, min((h1 - 1) * wm + w1, (h2 - 1) * wm + w2)
                if interleaved:
                    raise JpezyError("decode_jpeg_ycc: the chroma components of this file differ in size and cannot share one interleaved plane")
            pcb, pcr = cb.ctypes.data, cr.ctypes.data
        _check(lib.jpezy_decode_jpeg_ycc(self._h, _np_ptr(arr), arr.size, C.byref(info), _np_ptr(y), w0, y.size, pcb, pcr, c_stride, c_step, c_cap))
        return info, y, cb, cr

    @staticmethod
    def _ycc_layout(d_y, d_cb, d_cr, who):
        """(n_frames, H, W, y_stride, y_frame_stride, c_stride, c_step, c_frame_stride) of torch uint8 tensors (H, W) / (CH, CW) or with a
        leading frame dimension; d_cb / d_cr None: luma only"""
        import torch
        if d_y.dtype != torch.uint8 or d_y.dim() not in (2, 3) or (d_y.shape[-1] > 1 and d_y.stride(-1) != 1):
            raise JpezyError(f"{who}: d_y must be a uint8 tensor (H, W) or (N, H, W) whose rows are contiguous")
        H, W = int(d_y.shape[-2]), int(d_y.shape[-1])
        n = int(d_y.shape[0]) if d_y.dim() == 3 else 1
        ys = int(d_y.stride(-2)) if H > 1 else 0
        yfs = int(d_y.stride(0)) if d_y.dim() == 3 and n > 1 else 0
        cs, step, cfs = 0, 1, 0
        chroma = [c for c in (d_cb, d_cr) if c is not None]
        if chroma:
            cw, ch = ycc_chroma_size(W, H)
            c0 = chroma[0]
            for c in chroma:
                if c.dtype != torch.uint8 or c.dim() != d_y.dim() or tuple(c.shape[-2:]) != (ch, cw) or (c.dim() == 3 and int(c.shape[0]) != n):
                    raise JpezyError(f"{who}: chroma tensors must be uint8 of shape ({ch}, {cw}) with d_y's frame dimension")
                if c.stride() != c0.stride():
                    raise JpezyError(f"{who}: d_cb and d_cr must have the same strides")
            step = int(c0.stride(-1)) if cw > 1 else 1
            cs = int(c0.stride(-2)) if ch > 1 else 0
            cfs = int(c0.stride(0)) if c0.dim() == 3 and n > 1 else 0
        return n, H, W, ys, yfs, cs, step, cfs

    def fdct_quant_ycc_dev(self, d_y, d_cb, d_cr, d_coeffs, gray=False, stream=None):
        """device Y, Cb, Cr samples (torch uint8 (H, W) and (CH, CW), or with a leading frame dimension; strides are the tensors', so the two
        views of an interleaved NV12 plane work) -> d_coeffs.  gray: luma only, d_cb and d_cr may be None."""
        import torch
        n, H, W, ys, yfs, cs, step, cfs = self._ycc_layout(d_y, None if gray else d_cb, None if gray else d_cr, "fdct_quant_ycc_dev")
        if stream is None:
            stream = torch.cuda.current_stream(d_y.device).cuda_stream
        pcb, pcr = (None, None) if gray else (d_cb.data_ptr(), d_cr.data_ptr())
        _check(load_library().jpezy_fdct_quant_ycc_dev(self._h, d_y.data_ptr(), ys, pcb, pcr, cs, step, yfs, cfs, W, H, int(gray), n,
                                                       d_coeffs.data_ptr(), stream))

    def dequant_idct_ycc_dev(self, d_coeffs, d_y, d_cb=None, d_cr=None, qt=None, comp_tq=(0, 1, 1), stream=None):
        """device coefficients (6-block layout) -> the components at their native sampling, written into d_y (H, W) and d_cb, d_cr (CH, CW)
        (layout as for fdct_quant_ycc_dev); d_cb = d_cr = None: luma only"""
        import torch
        n, H, W, ys, yfs, cs, step, cfs = self._ycc_layout(d_y, d_cb, d_cr, "dequant_idct_ycc_dev")
        if stream is None:
            stream = torch.cuda.current_stream(d_coeffs.device).cuda_stream
        qtab = qt if qt is not None else annex_k_tables().qt
        tq = (C.c_uint8 * 3)(*comp_tq)
        _check(load_library().jpezy_dequant_idct_ycc_dev(self._h, d_coeffs.data_ptr(), C.byref(qtab), C.byref(tq), d_y.data_ptr(), ys,
                                                         d_cb.data_ptr() if d_cb is not None else None, d_cr.data_ptr() if d_cr is not None else None,
                                                         cs, step, yfs, cfs, W, H, n, stream))

    # ---- YCbCr 4:2:2 samples (planar I422 / YV16 / NV16 / NV61, packed YUY2 / UYVY / YVYU; include/jpezy_hip_ycc422.h) ----
    def encode_jpeg_ycc422(self, y, cb, cr, comment=None):
        """2-D numpy uint8 planes -> the bytes of a 4:2:2 .jpg: y (H, W), cb and cr (H, ceil(W/2)).  Strides and c_step are read from the
        arrays, so uv[..., 0], uv[..., 1] of an NV16 plane (H, W/2, 2) encode in place."""
        lib = load_library()
        y = np.asarray(y)
        if y.dtype != np.uint8 or y.ndim != 2:
            raise JpezyError("encode_jpeg_ycc422: y must be a 2-D uint8 array")
        H, W = y.shape
        if y.strides[1] != 1 or y.strides[0] < W:
            y = np.ascontiguousarray(y)
        cw, ch = ycc422_chroma_size(W, H)
        cb, cr = np.asarray(cb), np.asarray(cr)
        for c in (cb, cr):
            if c.dtype != np.uint8 or c.shape != (ch, cw):
                raise JpezyError(f"encode_jpeg_ycc422: cb and cr must be uint8 arrays of shape ({ch}, {cw})")
        if not (cb.strides == cr.strides and cb.strides[1] in (1, 2) and cb.strides[0] >= (cw - 1) * cb.strides[1] + 1):
            cb, cr = np.ascontiguousarray(cb), np.ascontiguousarray(cr)
        c_stride, c_step = (cb.strides[0] if ch > 1 else 0), (cb.strides[1] if cw > 1 else 1)
        if comment is None:
            comment = b"Encoded by jpezy"
        cap = jpeg_bound(W, H, SAMPLING_422)
        buf = np.empty(cap, dtype=np.uint8)
        n = _check(lib.jpezy_encode_jpeg_ycc422(self._h, _np_ptr(y), y.strides[0] if H > 1 else 0, _np_ptr(cb), _np_ptr(cr), c_stride, c_step, W, H,
                                                comment, _np_ptr(buf), cap))
        return buf[:n].tobytes()

    def fdct_quant_ycc422_dev(self, d_luma, d_cb, d_cr, d_coeffs):
        """device Y (d_luma), Cb, Cr samples (torch uint8 (H, W) and (H, CW), or with a leading frame dimension; strides are the tensors', so the two
        views of an interleaved NV16 plane work) -> d_coeffs in the 4:2:2 layout, on torch's current stream of the tensors' device"""
        import torch
        who = "fdct_quant_ycc422_dev"
        if d_luma.dtype != torch.uint8 or d_luma.dim() not in (2, 3) or (d_luma.shape[-1] > 1 and d_luma.stride(-1) != 1):
            raise JpezyError(f"{who}: d_luma must be a uint8 tensor (H, W) or (N, H, W) whose rows are contiguous")
        H, W = int(d_luma.shape[-2]), int(d_luma.shape[-1])
        n = int(d_luma.shape[0]) if d_luma.dim() == 3 else 1
        cw, ch = ycc422_chroma_size(W, H)
        for c in (d_cb, d_cr):
            if c.dtype != torch.uint8 or c.dim() != d_luma.dim() or tuple(c.shape[-2:]) != (ch, cw) or (c.dim() == 3 and int(c.shape[0]) != n):
                raise JpezyError(f"{who}: chroma tensors must be uint8 of shape ({ch}, {cw}) with d_luma's frame dimension")
        if d_cb.stride() != d_cr.stride():
            raise JpezyError(f"{who}: d_cb and d_cr must have the same strides")
        ys = int(d_luma.stride(-2)) if H > 1 else 0
        yfs = int(d_luma.stride(0)) if d_luma.dim() == 3 and n > 1 else 0
        step = int(d_cb.stride(-1)) if cw > 1 else 1
        cs = int(d_cb.stride(-2)) if ch > 1 else 0
        cfs = int(d_cb.stride(0)) if d_cb.dim() == 3 and n > 1 else 0
        stream = torch.cuda.current_stream(d_luma.device).cuda_stream
        _check(load_library().jpezy_fdct_quant_ycc422_dev(self._h, d_luma.data_ptr(), ys, d_cb.data_ptr(), d_cr.data_ptr(), cs, step, yfs, cfs, W, H, n,
                                                          d_coeffs.data_ptr(), stream))

    def encode_jpeg_yuv422(self, img, W=None, format=YUV_YUY2, comment=None):
        """numpy uint8 (H, >= row_bytes) packed macropixels with contiguous rows -> the bytes of a 4:2:2 .jpg.  W defaults to
        img.shape[1] // 2; strides[0] becomes row_stride, so a view with padded rows encodes in place."""
        lib = load_library()
        img = np.asarray(img)
        if img.dtype != np.uint8 or img.ndim != 2:
            raise JpezyError("encode_jpeg_yuv422: a 2-D uint8 array (H, row bytes) is expected")
        H = img.shape[0]
        W = img.shape[1] // 2 if W is None else int(W)
        if img.shape[1] < yuv422_row_bytes(W):
            raise JpezyError(f"encode_jpeg_yuv422: rows of {img.shape[1]} bytes hold fewer than W = {W} pixels")
        if img.strides[1] != 1 or img.strides[0] < img.shape[1]:
            img = np.ascontiguousarray(img)
        if comment is None:
            comment = b"Encoded by jpezy"
        cap = jpeg_bound(W, H, SAMPLING_422)
        buf = np.empty(cap, dtype=np.uint8)
        n = _check(lib.jpezy_encode_jpeg_yuv422(self._h, _np_ptr(img), int(format), img.strides[0] if H > 1 else 0, W, H, comment, _np_ptr(buf), cap))
        return buf[:n].tobytes()

    @staticmethod
    def _yuv422_layout(d_pix, W, who):
        """(n_frames, H, W, row_stride, frame_stride) of a torch uint8 tensor (H, B) or (N, H, B) of packed macropixels"""
        import torch
        if d_pix.dtype != torch.uint8 or d_pix.dim() not in (2, 3) or (d_pix.shape[-1] > 1 and d_pix.stride(-1) != 1):
            raise JpezyError(f"{who}: a uint8 tensor (H, B) or (N, H, B) whose rows are contiguous is expected")
        H, B = int(d_pix.shape[-2]), int(d_pix.shape[-1])
        W = B // 2 if W is None else int(W)
        if B < yuv422_row_bytes(W):
            raise JpezyError(f"{who}: rows of {B} bytes hold fewer than W = {W} pixels")
        n = int(d_pix.shape[0]) if d_pix.dim() == 3 else 1
        row = int(d_pix.stride(-2)) if H > 1 else 0
        frame = int(d_pix.stride(0)) if d_pix.dim() == 3 and n > 1 else 0
        return n, H, W, row, frame

    def fdct_quant_yuv422_dev(self, d_pix, d_coeffs, W=None, format=YUV_YUY2):
        """device packed macropixels (torch uint8 (H, B) or (N, H, B); row and frame strides are the tensor's; W defaults to B // 2)
        -> d_coeffs in the 4:2:2 layout, on torch's current stream of the tensor's device"""
        import torch
        n, H, W, row, frame = self._yuv422_layout(d_pix, W, "fdct_quant_yuv422_dev")
        stream = torch.cuda.current_stream(d_pix.device).cuda_stream
        _check(load_library().jpezy_fdct_quant_yuv422_dev(self._h, d_pix.data_ptr(), int(format), row, frame, W, H, n, d_coeffs.data_ptr(), stream))

    def decode_jpeg_yuv422(self, data, format=YUV_YUY2):
        """.jpg bytes of any layout -> (FrameInfo, uint8 array (H, row_bytes)) of packed macropixels"""
        lib = load_library()
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        info = FrameInfo()
        _check(lib.jpezy_decode_jpeg_yuv422(self._h, _np_ptr(arr), arr.size, C.byref(info), int(format), 0, None, 0))
        img = np.empty((info.height, yuv422_row_bytes(info.width)), dtype=np.uint8)
        _check(lib.jpezy_decode_jpeg_yuv422(self._h, _np_ptr(arr), arr.size, C.byref(info), int(format), 0, _np_ptr(img), img.size))
        return info, img

    def dequant_idct_generic_yuv422_dev(self, d_coeffs, info, d_pix, format=YUV_YUY2):
        """any-layout decode on device memory: coefficients as read_jpeg_gpu leaves them (frame after frame) -> packed macropixels written
        into d_pix (torch uint8 (H, B) or (N, H, B), B >= row_bytes; strides are the tensor's), on torch's current stream of the device"""
        import torch
        n, H, W, row, frame = self._yuv422_layout(d_pix, info.width, "dequant_idct_generic_yuv422_dev")
        if H != info.height:
            raise JpezyError(f"dequant_idct_generic_yuv422_dev: the tensor has {H} rows, the picture {info.height}")
        stream = torch.cuda.current_stream(d_coeffs.device).cuda_stream
        head = self._stage_head(d_coeffs.data_ptr(), info, False)[:10]
        _check(load_library().jpezy_dequant_idct_generic_yuv422_dev(*head, int(format), row, frame, n, d_pix.data_ptr(), stream))

    # ---- reduced-size decode (scale 1, 2, 4, 8: an N x N inverse transform per block, N = 8 / scale; include/jpezy_hip.h) ----
    def decode_jpeg_scaled(self, data, scale, gray=False):
        """.jpg bytes -> (FrameInfo, r, g, b) planes of Ws*Hs bytes, (Ws, Hs) = scaled_size(width, height, scale); the FrameInfo keeps
        the file's own width and height.  scale 1 is decode_jpeg."""
        def size(info):
            ws, hs = scaled_size(info.width, info.height, scale)
            return ws * hs
        return self._decode_planes(load_library().jpezy_decode_jpeg_scaled, data, (int(gray), int(scale)), size)

    def decode_jpeg_scaled_packed(self, data, scale, format=PIX_RGB24, gray=False):
        """.jpg bytes -> (FrameInfo, uint8 array (Hs, Ws, C)) of interleaved pixels at 1/scale; the fourth byte of a 32-bit format is 0xFF."""
        return self._decode_packed(load_library().jpezy_decode_jpeg_scaled_packed, data, (int(gray), int(scale)), format,
                                   lambda info: scaled_size(info.width, info.height, scale))

    def dequant_idct_scaled_dev(self, d_coeffs, info, scale, d_r=None, d_g=None, d_b=None, gray=False, stream=None, n_frames=1,
                                plane_stride=None, d_img=None, format=PIX_RGB24):
        """any-layout decode at 1/scale on device memory (torch tensors): coefficients as read_jpeg_gpu leaves them -> planes of Ws*Hs
        bytes (n_frames frames plane_stride apart, default Ws*Hs), or, with d_img, packed pixels written into a uint8 tensor (Hs, Ws, C) or
        (N, Hs, Ws, C) whose strides give the row and frame strides, as dequant_idct_packed_dev takes it"""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(d_coeffs.device).cuda_stream
        Ws, Hs = scaled_size(info.width, info.height, scale)
        head = (*self._stage_head(d_coeffs.data_ptr(), info, gray), int(scale))
        if d_img is not None:
            n, H, W, row, frame = self._packed_layout(d_img, pixel_bytes(format), "dequant_idct_scaled_dev")
            if (W, H) != (Ws, Hs):
                raise JpezyError(f"dequant_idct_scaled_dev: d_img is {W} x {H}, the scaled size is {Ws} x {Hs}")
            _check(load_library().jpezy_dequant_idct_scaled_packed_dev(*head, int(format), row, frame, n, d_img.data_ptr(), stream))
            return
        stride = plane_stride if plane_stride is not None else Ws * Hs
        _check(load_library().jpezy_dequant_idct_scaled_dev(*head, n_frames, stride, d_r.data_ptr(), d_g.data_ptr(), d_b.data_ptr(), stream))

    # ---- chroma upsampling (UPSAMPLE_NEAREST: the existing decode; UPSAMPLE_SMOOTH: the triangle filter; include/jpezy_hip.h) ----
    def decode_jpeg_upsampling(self, data, upsampling, gray=False):
        """.jpg bytes -> (FrameInfo, r, g, b) planes of width*height bytes with the upsampling chosen.  UPSAMPLE_NEAREST is decode_jpeg."""
        return self._decode_planes(load_library().jpezy_decode_jpeg_upsampling, data, (int(gray), int(upsampling)),
                                   lambda info: info.width * info.height)

    def decode_jpeg_upsampling_packed(self, data, upsampling, format=PIX_RGB24, gray=False):
        """.jpg bytes -> (FrameInfo, uint8 array (H, W, C)) of interleaved pixels with the upsampling chosen."""
        return self._decode_packed(load_library().jpezy_decode_jpeg_upsampling_packed, data, (int(gray), int(upsampling)), format,
                                   lambda info: (info.width, info.height))

    def dequant_idct_upsampling_dev(self, d_coeffs, info, d_r=None, d_g=None, d_b=None, gray=False, stream=None, n_frames=1,
                                    plane_stride=None, d_img=None, format=PIX_RGB24, upsampling=UPSAMPLE_SMOOTH):
        """any-layout decode with the upsampling chosen on device memory (torch tensors): coefficients as read_jpeg_gpu leaves them ->
        planes of W*H bytes (n_frames frames plane_stride apart, default W*H), or, with d_img, packed pixels written into a uint8 tensor
        (H, W, C) or (N, H, W, C) whose strides give the row and frame strides, as dequant_idct_packed_dev takes it"""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(d_coeffs.device).cuda_stream
        head = (*self._stage_head(d_coeffs.data_ptr(), info, gray), int(upsampling))
        if d_img is not None:
            n, H, W, row, frame = self._packed_layout(d_img, pixel_bytes(format), "dequant_idct_upsampling_dev")
            if (W, H) != (info.width, info.height):
                raise JpezyError(f"dequant_idct_upsampling_dev: d_img is {W} x {H}, the file is {info.width} x {info.height}")
            _check(load_library().jpezy_dequant_idct_upsampling_packed_dev(*head, int(format), row, frame, n, d_img.data_ptr(), stream))
            return
        stride = plane_stride if plane_stride is not None else info.width * info.height
        _check(load_library().jpezy_dequant_idct_upsampling_dev(*head, n_frames, stride, d_r.data_ptr(), d_g.data_ptr(), d_b.data_ptr(), stream))

    # ---- region decode (a window (x, y, w, h) of the picture at 1/scale: the scaled decode, sliced; include/jpezy_hip.h) ----
    def decode_jpeg_region(self, data, region, scale=1, gray=False, upsampling=UPSAMPLE_NEAREST):
        """.jpg bytes -> (FrameInfo, r, g, b) planes of w*h bytes: the window region = (x, y, w, h) of the picture at 1/scale.  The
        FrameInfo keeps the file's own width and height.  upsampling=UPSAMPLE_SMOOTH: 2:1 chroma through the triangle filter over its
        plane at that scale (jpezy_decode_jpeg_region_upsampling)."""
        lib = load_library()
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        info, rect = FrameInfo(), _rect(region)
        n = max(rect.w, 0) * max(rect.h, 0)
        r, g, b = (np.empty(max(n, 1), dtype=np.uint8) for _ in range(3))
        _check(lib.jpezy_decode_jpeg_region_upsampling(self._h, _np_ptr(arr), arr.size, int(gray), int(upsampling), int(scale), C.byref(rect),
                                                       C.byref(info), _np_ptr(r), _np_ptr(g), _np_ptr(b), n))
        return info, r, g, b

    def decode_jpeg_region_packed(self, data, region, scale=1, format=PIX_RGB24, gray=False, upsampling=UPSAMPLE_NEAREST):
        """.jpg bytes -> (FrameInfo, uint8 array (h, w, C)) of interleaved pixels of the window; the fourth byte of a 32-bit format is 0xFF.
        upsampling: as decode_jpeg_region's."""
        lib = load_library()
        nb = pixel_bytes(format)
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        info, rect = FrameInfo(), _rect(region)
        img = np.empty((max(rect.h, 1), max(rect.w, 1), nb), dtype=np.uint8)
        _check(lib.jpezy_decode_jpeg_region_upsampling_packed(self._h, _np_ptr(arr), arr.size, int(gray), int(upsampling), int(scale), C.byref(rect),
                                                              C.byref(info), int(format), 0, _np_ptr(img), img.size))
        return info, img

    # ---- oriented output (include/jpezy_hip_orientation.h): the picture mirrored / rotated / transposed as an EXIF orientation says ----
    def decode_jpeg_oriented(self, data, orientation=ORIENT_FROM_FILE, region=None, scale=1, gray=False, upsampling=UPSAMPLE_NEAREST):
        """.jpg bytes -> (FrameInfo, r, g, b, (w, h), orientation_used): the window region = (x, y, w, h) of the ORIENTED picture at 1/scale
        (None: all of it) as planes of w*h bytes.  orientation: 1..8, or ORIENT_FROM_FILE for the file's own EXIF tag.  The FrameInfo
        keeps the file's own width and height (jpezy_decode_jpeg_oriented)."""
        lib = load_library()
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        info, used = FrameInfo(), C.c_int(0)
        rect = None if region is None else _rect(region)
        head = (self._h, _np_ptr(arr), arr.size, int(gray), int(upsampling), int(scale), None if rect is None else C.byref(rect), int(orientation),
                C.byref(used), C.byref(info))
        if rect is None:
            _check(lib.jpezy_decode_jpeg_oriented(*head, None, None, None, 0))
            w, h = orient_size(used.value, *scaled_size(info.width, info.height, scale))
        else:
            w, h = max(rect.w, 0), max(rect.h, 0)
        r, g, b = (np.empty(max(w * h, 1), dtype=np.uint8) for _ in range(3))
        _check(lib.jpezy_decode_jpeg_oriented(*head, _np_ptr(r), _np_ptr(g), _np_ptr(b), w * h))
        return info, r[:w * h], g[:w * h], b[:w * h], (w, h), used.value

    def decode_jpeg_oriented_packed(self, data, orientation=ORIENT_FROM_FILE, region=None, scale=1, format=PIX_RGB24, gray=False,
                                    upsampling=UPSAMPLE_NEAREST):
        """.jpg bytes -> (FrameInfo, uint8 array (h, w, C), orientation_used): the same window as interleaved pixels"""
        lib = load_library()
        nb = pixel_bytes(format)
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        info, used = FrameInfo(), C.c_int(0)
        rect = None if region is None else _rect(region)
        head = (self._h, _np_ptr(arr), arr.size, int(gray), int(upsampling), int(scale), None if rect is None else C.byref(rect), int(orientation),
                C.byref(used), C.byref(info), int(format), 0)
        if rect is None:
            _check(lib.jpezy_decode_jpeg_oriented_packed(*head, None, 0))
            w, h = orient_size(used.value, *scaled_size(info.width, info.height, scale))
        else:
            w, h = max(rect.w, 1), max(rect.h, 1)
        img = np.empty((h, w, nb), dtype=np.uint8)
        _check(lib.jpezy_decode_jpeg_oriented_packed(*head, _np_ptr(img), img.size))
        return info, img, used.value

    def set_windows_orientation(self, mode):
        """0 (default): the window batches ignore the EXIF orientation; 1: every file's own tag is honoured -- windows are then in the
        coordinates of the oriented picture (jpezy_ctx_set_windows_orientation)"""
        _check(load_library().jpezy_ctx_set_windows_orientation(self._h, int(mode)))

    def windows_orientation(self):
        return _check(load_library().jpezy_ctx_windows_orientation(self._h))

    def dequant_idct_region_dev(self, d_coeffs, info, region, scale=1, d_r=None, d_g=None, d_b=None, gray=False, stream=None, n_frames=1,
                                plane_stride=None, d_img=None, format=PIX_RGB24, upsampling=UPSAMPLE_NEAREST, orientation=None):
        """the window region = (x, y, w, h) of the picture at 1/scale on device memory (torch tensors): the WHOLE frames' coefficients as
        read_jpeg_gpu leaves them -> planes of w*h bytes (n_frames frames plane_stride apart, default w*h), or, with d_img, packed pixels
        written into a uint8 tensor (h, w, C) or (N, h, w, C) whose strides give the row and frame strides.  upsampling: as
        decode_jpeg_region's (jpezy_dequant_idct_region_upsampling[_packed]_dev).  orientation 1..8: region is a window of the ORIENTED
        picture (jpezy_dequant_idct_region_oriented[_packed]_dev); None: the entries without the argument."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(d_coeffs.device).cuda_stream
        rect = _rect(region)
        head = (*self._stage_head(d_coeffs.data_ptr(), info, gray), int(upsampling), int(scale), C.byref(rect))
        if d_img is not None:
            n, H, W, row, frame = self._packed_layout(d_img, pixel_bytes(format), "dequant_idct_region_dev")
            if (W, H) != (rect.w, rect.h):
                raise JpezyError(f"dequant_idct_region_dev: d_img is {W} x {H}, the region is {rect.w} x {rect.h}")
            if orientation is not None:
                _check(load_library().jpezy_dequant_idct_region_oriented_packed_dev(*head, int(orientation), int(format), row, frame, n, d_img.data_ptr(),
                                                                                    stream))
                return
            _check(load_library().jpezy_dequant_idct_region_upsampling_packed_dev(*head, int(format), row, frame, n, d_img.data_ptr(), stream))
            return
        stride = plane_stride if plane_stride is not None else rect.w * rect.h
        if orientation is not None:
            _check(load_library().jpezy_dequant_idct_region_oriented_dev(*head, int(orientation), n_frames, stride, d_r.data_ptr(), d_g.data_ptr(),
                                                                         d_b.data_ptr(), stream))
            return
        _check(load_library().jpezy_dequant_idct_region_upsampling_dev(*head, n_frames, stride, d_r.data_ptr(), d_g.data_ptr(), d_b.data_ptr(), stream))

    # ---- lossless transforms in the coefficient domain (include/jpezy_hip.h, LOSSLESS TRANSFORMS) ----
    def transform_jpeg(self, data, op, trim=False, comment=None):
        """.jpg bytes -> (.jpg bytes of the flipped / rotated / transposed picture, FrameInfo of the output): GPU Huffman decoder,
        transform kernel, GPU entropy coder; no pixel is computed.  op: XFORM_*; trim: drop the partial MCU column / row of a mirrored
        axis; comment None: the source's COM text is carried over, b"": none.  The context's set_huffman_optimize and
        set_restart_interval settings act; its quantiser setting does not."""
        lib = load_library()
        arr = np.frombuffer(bytes(data), dtype=np.uint8)
        info = FrameInfo()
        flags = XFORM_TRIM if trim else 0
        _check(lib.jpezy_transform_jpeg(self._h, _np_ptr(arr), arr.size, int(op), flags, comment, C.byref(info), None, 0))
        cap = jpeg_bound(info.width, info.height, SAMPLING_444 if info.H[0] == 1 else SAMPLING_420)
        buf = np.empty(cap, dtype=np.uint8)
        n = _check(lib.jpezy_transform_jpeg(self._h, _np_ptr(arr), arr.size, int(op), flags, comment, C.byref(info), _np_ptr(buf), cap))
        return buf[:n].tobytes(), info

    def coeff_transform_dev(self, d_in, W, H, d_out, op, trim=False, sampling=SAMPLING_420, n_frames=1, stream=None):
        """Asynchronous: n_frames coefficient fields of a W x H picture (torch int16 tensors on the device) from d_in to a different
        tensor d_out, which holds coeff_count(Wout, Hout, sampling=) elements per frame (transform_geometry)"""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(d_in.device).cuda_stream
        wo, ho, _, _ = transform_geometry(op, W, H, sampling, trim)
        if d_in.numel() < n_frames * coeff_count(W, H, sampling=sampling) or d_out.numel() < n_frames * coeff_count(wo, ho, sampling=sampling):
            raise JpezyError("coeff_transform_dev: d_in / d_out are smaller than n_frames fields of the source / output size")
        _check(load_library().jpezy_coeff_transform_dev(self._h, d_in.data_ptr(), int(W), int(H), int(sampling), int(op), XFORM_TRIM if trim else 0,
                                                        int(n_frames), d_out.data_ptr(), stream))


# ---- host serial tail / head ----
def optimal_table(freq):
    """256 symbol counts -> (bits[16], vals[nval]) of the optimal Huffman table (Annex K.2; jpezy_huffman_optimal_table)"""
    f = np.ascontiguousarray(freq, dtype=np.uint64)
    if f.size != 256:
        raise JpezyError("optimal_table: 256 counts are expected")
    bits, vals = np.zeros(16, dtype=np.uint8), np.zeros(256, dtype=np.uint8)
    n = _check(load_library().jpezy_huffman_optimal_table(_np_ptr(f), _np_ptr(bits), _np_ptr(vals)))
    return bits, vals[:n].copy()


def write_jpeg(coeffs, W, H, gray=False, comment=None, optimize=False, restart_interval=0, quant_tables=None, sampling=SAMPLING_420):
    """zig-zag int16 coefficients -> the .jpg bytes jpezy_encode writes (header + Huffman + EOI); optimize: with the frame's own
    optimal Huffman tables instead of Annex K (same coefficients, smaller file); restart_interval: MCUs per restart interval
    (DRI segment, RSTn markers, predictors reset), 0 for none; quant_tables = (luma, chroma): the tables the DQT segments state
    (64 entries each, natural order, 1..255) instead of Annex K -- the coefficients are written as they are.
    sampling=SAMPLING_444: coefficients of 8 x 8 MCUs of Y, Cb, Cr (coeff_count(W, H, sampling=SAMPLING_444)), a 4:4:4 file;
    SAMPLING_422: 16 x 8 MCUs of Y, Y, Cb, Cr, a 4:2:2 file."""
    lib = load_library()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.int16)
    if sampling != SAMPLING_420:
        if not gray and coeffs.size != coeff_count(W, H, sampling=sampling):
            raise JpezyError("coefficient buffer size does not match W, H, sampling")
        if comment is None:
            comment = b"Encoded by jpezy"
        luma, chroma = (_table(t, "write_jpeg") for t in quant_tables) if quant_tables is not None else (None, None)
        cap = jpeg_bound(W, H, sampling)
        buf = np.empty(cap, dtype=np.uint8)
        n = _check(lib.jpezy_write_jpeg_sampling(_np_ptr(coeffs), W, H, int(sampling), int(gray), comment,
                                                 _np_ptr(luma) if luma is not None else None, _np_ptr(chroma) if chroma is not None else None,
                                                 int(restart_interval), int(bool(optimize)), _np_ptr(buf), cap))
        return buf[:n].tobytes()
    if coeffs.size != lib.jpezy_coeff_count(W, H, int(gray)):
        raise JpezyError("coefficient buffer size does not match W, H, gray")
    if comment is None:
        comment = b"Encoded by JPEZY" if gray else b"Encoded by jpezy"   # ref encode_io.hpp:149,181
    cap = lib.jpezy_jpeg_bound(W, H)
    buf = np.empty(cap, dtype=np.uint8)
    if quant_tables is not None:
        luma, chroma = (_table(t, "write_jpeg") for t in quant_tables)
        n = _check(lib.jpezy_write_jpeg_qt(_np_ptr(coeffs), W, H, int(gray), comment, _np_ptr(luma), _np_ptr(chroma), int(restart_interval),
                                           int(bool(optimize)), _np_ptr(buf), cap))
        return buf[:n].tobytes()
    if restart_interval != 0:
        n = _check(lib.jpezy_write_jpeg_rst(_np_ptr(coeffs), W, H, int(gray), comment, int(restart_interval), int(bool(optimize)),
                                            _np_ptr(buf), cap))
        return buf[:n].tobytes()
    fn = lib.jpezy_write_jpeg_opt if optimize else lib.jpezy_write_jpeg
    n = _check(fn(_np_ptr(coeffs), W, H, int(gray), comment, _np_ptr(buf), cap))
    return buf[:n].tobytes()


def write_jpeg_batch(coeffs, W, H, n_frames, gray=False, comment=None, threads=0):
    """n_frames independent frames through the host Huffman/JFIF tail on `threads` host threads; returns a list of bytes."""
    lib = load_library()
    coeffs = np.ascontiguousarray(coeffs, dtype=np.int16)
    if coeffs.size != lib.jpezy_coeff_count(W, H, int(gray)) * n_frames:
        raise JpezyError("coefficient buffer size does not match W, H, gray, n_frames")
    if comment is None:
        comment = b"Encoded by JPEZY" if gray else b"Encoded by jpezy"
    cap = lib.jpezy_jpeg_bound(W, H)
    buf = np.empty(cap * n_frames, dtype=np.uint8)
    sizes = (C.c_long * n_frames)()
    _check(lib.jpezy_write_jpeg_batch(_np_ptr(coeffs), W, H, int(gray), n_frames, comment, _np_ptr(buf), cap, sizes, threads))
    return [buf[f * cap: f * cap + sizes[f]].tobytes() for f in range(n_frames)]


def shard_range(n_units, n_shards, k):
    """[lo, hi) of shard k: the C entry jpezy_shard_range (the rule jpezy_encode_batch_multi partitions by)."""
    lo, n = C.c_long(), C.c_long()
    load_library().jpezy_shard_range(n_units, n_shards, k, C.byref(lo), C.byref(n))
    return lo.value, lo.value + n.value


def _multi_call(call, root_device, r, g, b, W, H, n_frames, gray, comment, want_coeffs, want_jpg, on_root_device, jpg_stride, raw=False):
    """Shared body of encode_batch_multi and MultiEncoder.encode: buffers, the jpezy_multi_out record, the call, the results."""
    lib = load_library()
    planes = [p if raw else np.ascontiguousarray(p, dtype=np.uint8).reshape(-1) for p in (r, g, b)]
    ptrs = []
    for p in planes:
        if hasattr(p, "data_ptr"):              # a (pinned) torch tensor in host memory
            if p.numel() != W * H * n_frames:
                raise JpezyError("plane size does not match W*H*n_frames")
            ptrs.append(C.c_void_p(p.data_ptr()))
        else:
            if p.size != W * H * n_frames:
                raise JpezyError("plane size does not match W*H*n_frames")
            ptrs.append(_np_ptr(p))
    if comment is None:
        comment = b"Encoded by JPEZY" if gray else b"Encoded by jpezy"
    cpf = lib.jpezy_coeff_count(W, H, int(gray))
    stride = int(jpg_stride) if jpg_stride else lib.jpezy_jpeg_bound(W, H)
    sizes = (C.c_longlong * n_frames)()
    out = MultiOut()
    out.on_root_device = int(bool(on_root_device))
    out.jpg_stride = stride
    out.jpg_sizes = sizes
    keep = []
    if on_root_device:
        import torch
        dev = torch.device("cuda", int(root_device))
        if want_coeffs:
            t = torch.empty(n_frames * cpf, dtype=torch.int16, device=dev); keep.append(t); out.coeffs = t.data_ptr()
        if want_jpg:
            t = torch.zeros(n_frames * stride, dtype=torch.uint8, device=dev); keep.append(t); out.jpg = t.data_ptr()
    else:
        if want_coeffs:
            t = np.empty(n_frames * cpf, dtype=np.int16); keep.append(t); out.coeffs = t.ctypes.data
        if want_jpg:
            t = np.empty(n_frames * stride, dtype=np.uint8); keep.append(t); out.jpg = t.ctypes.data
    rc = call(ptrs, comment, out)
    if rc != 0 and not (rc == -5 and want_jpg):
        _check(rc)
    if raw:                                     # (the benchmark: no per-file Python objects inside its bracket)
        return keep, sizes
    host = [k.cpu().numpy() if on_root_device else k for k in keep]
    co = host.pop(0).reshape(n_frames, -1) if want_coeffs else None
    jpg = None
    if want_jpg:
        buf = host.pop(0)
        jpg = [buf[f * stride: f * stride + sizes[f]].tobytes() if sizes[f] > 0 else int(sizes[f]) for f in range(n_frames)]
    return co, jpg


def encode_batch_multi(devices, r, g, b, W, H, n_frames, gray=False, chunk_frames=0, comment=None, want_coeffs=False, want_jpg=True,
                       on_root_device=False, jpg_stride=None):
    """jpezy_encode_batch_multi (one-shot: handle created and destroyed inside): n_frames frames (host planes, n_frames * W * H bytes
    each) over the GPUs `devices` (devices[0] = root).  Returns (coeffs or None, list of .jpg bytes or None).  on_root_device: the
    results are gathered into the root GPU's memory (torch tensors on that device) and copied to the host here only to be returned."""
    lib = load_library()
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])

    def call(ptrs, comment, out):
        return lib.jpezy_encode_batch_multi(devs, len(devices), ptrs[0], ptrs[1], ptrs[2], W, H, int(gray), n_frames, int(chunk_frames), comment,
                                            C.byref(out))
    return _multi_call(call, devices[0], r, g, b, W, H, n_frames, gray, comment, want_coeffs, want_jpg, on_root_device, jpg_stride)


class MultiEncoder:
    """jpezy_multi_create / jpezy_multi_encode / jpezy_multi_destroy: a reusable handle over the GPUs `devices` for frames of one
    size -- contexts, streams and the pinned staging rings live as long as it does; encode() may be called with any number of frames."""

    def __init__(self, devices, W, H, gray=False, chunk_frames=0):
        lib = load_library()
        self.devices = [int(d) for d in devices]
        self.W, self.H, self.gray = int(W), int(H), bool(gray)
        devs = (C.c_int * len(self.devices))(*self.devices)
        self._h = lib.jpezy_multi_create(devs, len(self.devices), self.W, self.H, int(self.gray), int(chunk_frames))
        if not self._h:
            raise JpezyError(lib.jpezy_hip_last_error().decode(errors="replace"))
        self.chunk_frames = lib.jpezy_multi_chunk_frames(self._h)
        self.feeder_threads = lib.jpezy_multi_feeder_threads(self._h)

    def set_feeder_threads(self, n):
        _check(load_library().jpezy_multi_set_feeder_threads(self._h, int(n)))
        self.feeder_threads = int(n)

    def encode(self, r, g, b, n_frames, comment=None, want_coeffs=False, want_jpg=True, on_root_device=False, jpg_stride=None, raw=False):
        lib = load_library()
        if not self._h:
            raise JpezyError("MultiEncoder is closed")

        def call(ptrs, comment, out):
            return lib.jpezy_multi_encode(self._h, ptrs[0], ptrs[1], ptrs[2], n_frames, comment, C.byref(out))
        return _multi_call(call, self.devices[0], r, g, b, self.W, self.H, n_frames, self.gray, comment, want_coeffs, want_jpg, on_root_device,
                           jpg_stride, raw=raw)

    def stats(self):
        """per lane of the last encode(): dicts of jpezy_multi_lane_stats"""
        lib = load_library()
        arr = (MultiLaneStats * len(self.devices))()
        n = lib.jpezy_multi_last_stats(self._h, arr, len(self.devices))
        return [{k: getattr(arr[i], k) for k, _ in MultiLaneStats._fields_} for i in range(min(n, len(self.devices)))]

    def close(self):
        if self._h:
            load_library().jpezy_multi_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_jpeg(data):
    """.jpg bytes -> (FrameInfo, int16 coeffs [mcu_rows, mcu_cols, blocks_per_mcu, 64] in zig-zag order)."""
    lib = load_library()
    arr = np.frombuffer(bytes(data), dtype=np.uint8)
    info = FrameInfo()
    _check(lib.jpezy_read_jpeg(_np_ptr(arr), arr.size, C.byref(info), None, 0))
    co = np.zeros((info.mcu_rows, info.mcu_cols, info.blocks_per_mcu, 64), dtype=np.int16)
    _check(lib.jpezy_read_jpeg(_np_ptr(arr), arr.size, C.byref(info), _np_ptr(co), co.size))
    return info, co


_DEFAULT_CTX = {}


def default_context(device=0):
    if device not in _DEFAULT_CTX:
        _DEFAULT_CTX[device] = Context(device)
    return _DEFAULT_CTX[device]


class Encoder:
    """Mirror of jpezy::encoder<T> (ref encoder/jpezy_encoder.hpp:22-77): holds copies of the planes;
    encode() runs the compute stage and the Huffman stage on the GPU (Context.encode_jpeg; the JFIF header and EOI
    come from the host), writes the file and returns the number of bytes written."""

    block_size = 8

    def __init__(self, width, height, r, g, b, ctx=None):
        self.width, self.height = int(width), int(height)
        self.r, self.g, self.b = (np.array(p, dtype=np.uint8, copy=True).reshape(-1) for p in (r, g, b))
        self.ctx = ctx

    def coefficients(self, gray=False):
        ctx = self.ctx or default_context()
        return ctx.fdct_quant(self.r, self.g, self.b, self.width, self.height, gray=gray)

    def encode_bytes(self, gray=False):
        ctx = self.ctx or default_context()
        return ctx.encode_jpeg(self.r, self.g, self.b, self.width, self.height, gray=gray)

    def encode(self, output_file, gray=False):
        data = self.encode_bytes(gray)
        with open(output_file, "wb") as f:
            f.write(data)
        return len(data)


class Decoder:
    """Mirror of jpezy::decoder<> (ref decoder/jpezy_decoder.hpp:39-134): decode() returns (r, g, b) planes
    of W*H bytes each, or None where the reference returns an empty optional."""

    rgb_size, block_size, blocks_size, mcu_size = 3, 8, 64, 4

    def __init__(self, filename, ctx=None):
        self.filename = filename
        self.ctx = ctx
        self.pr = None
        self.orientation, self.size = 1, None     # decode(orient=True): the orientation applied and the planes' (width, height)

    def decode(self, gray=False, scale=1, region=None, upsampling=UPSAMPLE_NEAREST, orient=False):
        """scale 2, 4 or 8: planes of scaled_size(width, height, scale) (Context.decode_jpeg_scaled); region = (x, y, w, h): planes of
        w*h bytes, that window of the picture at 1/scale (Context.decode_jpeg_region); self.pr keeps the file's size.
        upsampling=UPSAMPLE_SMOOTH: 2:1 chroma through the triangle filter (Context.decode_jpeg_upsampling), full size and whole
        pictures only: together with scale != 1 or a region it raises JpezyError with status JPEZY_E_UNSUPPORTED.
        orient=True: the file's EXIF orientation is applied (Context.decode_jpeg_oriented) -- the planes are those of the oriented picture,
        region is a window of it, self.orientation says what was applied and self.size the planes' (width, height)."""
        if upsampling != UPSAMPLE_NEAREST and (scale != 1 or region is not None):
            raise JpezyError(f"jpezy status {E_UNSUPPORTED}: Decoder.decode: smooth upsampling is not provided with reduced-size or region decode")
        try:
            with open(self.filename, "rb") as f:
                data = f.read()
            ctx = self.ctx or default_context()
            # Huffman head, IDCT and colour conversion on the GPU
            if orient:
                info, r, g, b, self.size, self.orientation = ctx.decode_jpeg_oriented(data, ORIENT_FROM_FILE, region=region, scale=scale, gray=gray,
                                                                                      upsampling=upsampling)
            elif region is not None:
                info, r, g, b = ctx.decode_jpeg_region(data, region, scale=scale, gray=gray)
            else:
                info, r, g, b = ctx.decode_jpeg(data, gray=gray, upsampling=upsampling) if scale == 1 else ctx.decode_jpeg_scaled(data, scale, gray=gray)
        except (OSError, JpezyError):
            return None
        self.pr = info
        return r, g, b
