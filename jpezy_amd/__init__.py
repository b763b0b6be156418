"""jpezy_amd -- MI355X-native (gfx950) baseline-JPEG hot path of falgon/jpezy.

The product is the C-ABI shared library `libjpezy_hip.so` (include/jpezy_hip.h): hand-written HIP kernels
for RGB->YCbCr + 4:2:0 + FDCT + quantise + zig-zag and dequantise + IDCT + upsample + YCbCr->RGB, plus the
host-side Huffman/JFIF tail.  This package is the Python binding used by tests/ and bench.py (torch is
only plumbing: device memory and streams) and a mirror of the reference's `encoder` / `decoder` surface.

There is no CPU fallback: importing works anywhere, but every compute call needs the built library and
a HIP device and raises JpezyError otherwise.
"""
from .api import (  # noqa: F401
    Context,
    DOWNSAMPLE_AVERAGE,
    DOWNSAMPLE_POINT,
    DT_BF16,
    DT_F16,
    DT_F32,
    DT_U8,
    Decoder,
    Encoder,
    FILTER_BICUBIC,
    FILTER_BILINEAR,
    FILTER_BOX,
    FILTER_LANCZOS,
    FrameInfo,
    JpezyError,
    MultiEncoder,
    PIX_BGR24,
    PIX_BGRA32,
    PIX_RGB24,
    PIX_RGBA32,
    Rect,
    Window,
    SAMPLING_420,
    SAMPLING_444,
    UPSAMPLE_NEAREST,
    UPSAMPLE_SMOOTH,
    XFORM_HFLIP,
    XFORM_NONE,
    XFORM_ROT180,
    XFORM_ROT270,
    XFORM_ROT90,
    XFORM_TRANSPOSE,
    XFORM_TRANSVERSE,
    XFORM_TRIM,
    XFORM_VFLIP,
    coeff_count,
    encode_batch_multi,
    huffman_histogram,
    jpeg_bound,
    library_path,
    load_library,
    mcu_grid,
    optimal_table,
    quality_tables,
    quant_tables_probe,
    quant_tables_transform,
    read_jpeg,
    region_check,
    resize_pick_window,
    resize_taps,
    window_fit,
    sampling_geometry,
    scaled_size,
    shard_range,
    tensor_normalization,
    transform_geometry,
    write_jpeg,
    write_jpeg_batch,
    ycc_chroma_size,
    ycc_component_size,
)

__all__ = [
    "Context", "DOWNSAMPLE_AVERAGE", "DOWNSAMPLE_POINT", "DT_BF16", "DT_F16", "DT_F32", "DT_U8", "Decoder", "Encoder", "FILTER_BICUBIC", "FILTER_BILINEAR", "FILTER_BOX", "FILTER_LANCZOS", "FrameInfo", "JpezyError", "MultiEncoder", "PIX_BGR24", "PIX_BGRA32", "PIX_RGB24", "PIX_RGBA32", "Rect", "SAMPLING_420", "SAMPLING_444", "UPSAMPLE_NEAREST", "UPSAMPLE_SMOOTH", "Window", "XFORM_HFLIP", "XFORM_NONE", "XFORM_ROT180", "XFORM_ROT270", "XFORM_ROT90", "XFORM_TRANSPOSE", "XFORM_TRANSVERSE", "XFORM_TRIM", "XFORM_VFLIP", "coeff_count", "encode_batch_multi", "huffman_histogram", "jpeg_bound", "library_path",
    "load_library", "mcu_grid", "optimal_table", "quality_tables", "quant_tables_probe", "quant_tables_transform", "read_jpeg", "region_check", "resize_pick_window", "resize_taps", "sampling_geometry", "scaled_size", "shard_range", "tensor_normalization", "transform_geometry", "window_fit", "write_jpeg", "write_jpeg_batch", "ycc_chroma_size", "ycc_component_size",
]
