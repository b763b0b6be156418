// jpezy_capi_internal.h -- what the translation units of the C-ABI share (internal): error macros, the context (owners: jpezy_owners.h).
// jpezy_capi.hip (context, the two transform stages), jpezy_capi_entropy.hip (Huffman coding: the host writer's entry points, the GPU
// coder's two forms, encoder::encode end to end), jpezy_capi_huffdec.hip (GPU Huffman decoding of one file, decoder::decode end to end),
// jpezy_capi_decode_batch.hip (the batch form), jpezy_capi_packed.hip (the entry points for packed, i.e. interleaved, pixels),
// jpezy_capi_scaled.hip (reduced-size decode), jpezy_capi_ycc.hip (planar YCbCr 4:2:0 samples in and out), jpezy_capi_ycc422.hip (YCbCr
// 4:2:2 samples in and out: planes and packed macropixels), jpezy_capi_sampling.hip (chroma
// sampling as an argument of the encoder's entries), jpezy_capi_transform.hip (lossless transforms in the coefficient domain),
// jpezy_capi_smooth.hip (smooth chroma upsampling in the decoder), jpezy_capi_windows.hip (a batch of crop windows into device memory),
// jpezy_capi_resized.hip (the same batch resized to one output size: tap tables and the second stage), jpezy_capi_multi.hip (the multi-GPU handle).
// What the decode entries share beyond this -- the description of a transform stage, the geometry of a layout, the file-decode driver,
// the head of the device entries, the fused kernel's core -- is in jpezy_capi_decode.h; what the encode entries share -- where the pixels
// are, the transform core, the file-encode driver -- is in jpezy_capi_encode.h.  Both include this file.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <new>
#include <string>
#include <thread>
#include <functional>
#include <vector>

#include "../../include/jpezy_constants.h"
#include "../../include/jpezy_hip.h"
#include "jpezy_device.h"
#include "jpezy_entropy.h"
#include "jpezy_huffdec.h"
#include "jpezy_host_codec.h"
#include "jpezy_owners.h"
#include "jpezy_hostpipe.h"

using namespace jpezy_dev;

namespace jpezy_capi {

// one comment limit for every writer (include/jpezy_hip.h, JPEZY_MAX_COMMENT)
inline int check_comment(const char* comment, const char* who)
{
    if (jpezy_host::comment_ok(comment)) return JPEZY_OK;
    return set_err(JPEZY_E_BADARG, std::string(who) + ": comment longer than JPEZY_MAX_COMMENT (" + std::to_string(JPEZY_MAX_COMMENT) + " bytes)");
}
// (at most 65535 x 65535: W * H fits in 32 bits, no caller needs a guard of its own for that)
inline int check_wh(int W, int H)
{
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535) return set_err(JPEZY_E_BADARG, "width/height must be in 1..65535 (16-bit SOF0 fields)");
    return JPEZY_OK;
}
#define HIP_TRY(expr)                                     \
    do {                                                  \
        hipError_t e__ = (expr);                          \
        if (e__ != hipSuccess) return hip_err(e__, #expr); \
    } while (0)

// No exception crosses the C ABI (include/jpezy_hip.h): every extern "C" body that allocates host memory is a
// function-try-block ending in JPEZY_CATCH.
#define JPEZY_CATCH                                                                                         \
    catch (const std::bad_alloc&) { return set_err(JPEZY_E_NOSPACE, "out of host memory"); }                \
    catch (const std::exception& e) { return set_err(JPEZY_E_HIP, std::string("unexpected exception: ") + e.what()); }

// coefficient buffers are moved with 16-byte accesses (one MCU = 768 or 512 bytes, so only the base matters)
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

inline bool stream_is_capturing(hipStream_t s)
{
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
}

// Scratch that lives in the context grows by a hipFree and a hipMalloc.  HIP refuses both while a stream is being captured and
// invalidates the capture over it, so a *_dev entry whose scratch must grow refuses first, with nothing freed, allocated or enqueued:
// the first call with these arguments belongs outside the capture, as for the tables.
inline int grow_outside_capture(DevBuf& b, size_t n, hipStream_t s, const char* what)
{
    if (n <= b.cap) return JPEZY_OK;
    if (stream_is_capturing(s))
        return set_err(JPEZY_E_BADARG, std::string(what) + ": the context's scratch cannot grow while the stream is being captured; "
                                                            "make the first call with these arguments outside the capture");
    return b.reserve(n);
}

// Context-wide device tables (dequantiser constants, cached JFIF header) may be read by launches still in flight on ANY
// stream the caller drives this context with: before rewriting them, wait for the whole device; and never from inside
// a stream capture (a synchronisation there would invalidate the capture).
// own_stream_only: the context is a child of jpezy_decode_jpeg_batch -- it is only ever driven on its own stream, so waiting for
// that stream is enough (eight children that each stalled the whole device for every file with new tables serialised the batch).
inline int drain_before_table_rewrite(hipStream_t s, const char* what, bool own_stream_only = false)
{
    if (stream_is_capturing(s))
        return set_err(JPEZY_E_BADARG, std::string(what) + ": new tables/header cannot be uploaded while the stream is being captured; "
                                                            "make the first call with these arguments outside the capture");
    if (own_stream_only)
        HIP_TRY(hipStreamSynchronize(s));
    else
        HIP_TRY(hipDeviceSynchronize());
    return JPEZY_OK;
}

inline const int kQt[2][64] = { JPEZY_QT_LUMA_INIT, JPEZY_QT_CHROMA_INIT };
inline const unsigned char kZzInv[64] = JPEZY_ZZ_INV_INIT;   // natural index -> zig-zag position

constexpr int kMaxFramesPerLaunch = 65535;   // the frame index is a grid dimension: larger batches go out as several launches

// Chunks of the streaming host-buffer entry points: MCU-row bands of a frame that is large against the chunk size, otherwise
// several whole frames.  Chunk k covers frames [f0, f0 + nf) and, in band mode (nf == 1), MCU rows [y0, y1) of frame f0.
// Its planes are rows(H) pixel rows of W (whole frames: nf planes of W x H), plane_bytes each, plane_off into the caller's plane;
// its coefficients are coef_bytes (B blocks per MCU), coef_off int16 elements into the caller's.
struct HostChunk {
    int f0, nf, y0, y1;
    int rows(int H) const { return std::min(H - y0 * 16, (y1 - y0) * 16); }
    size_t plane_bytes(int W, int H) const { return nf > 1 ? (size_t)W * H * nf : (size_t)rows(H) * W; }
    size_t plane_off(int W, int H) const { return (size_t)f0 * W * H + (size_t)y0 * 16 * W; }
    size_t coef_bytes(int W, int B) const { return (size_t)nf * (y1 - y0) * jpezy_mcu_cols(W) * B * 128; }
    size_t coef_off(int W, int H, int B) const { return ((size_t)f0 * jpezy_mcu_rows(H) + (size_t)y0) * jpezy_mcu_cols(W) * B * 64; }
};

inline std::vector<HostChunk> plan_host_chunks(int W, int H, int n_frames, size_t bytes_per_px, size_t target)
{
    std::vector<HostChunk> out;
    const int mcu_rows = jpezy_mcu_rows(H);
    const size_t frame_bytes = (size_t)W * H * bytes_per_px;
    if (frame_bytes > 2 * target) {
        const size_t row_bytes = (size_t)16 * W * bytes_per_px;
        const int rows_per = (int)std::max<size_t>(1, target / row_bytes);
        for (int f = 0; f < n_frames; ++f)
            for (int y = 0; y < mcu_rows; y += rows_per) out.push_back({ f, 1, y, std::min(y + rows_per, mcu_rows) });
    } else {
        const int per = (int)std::max<size_t>(1, target / std::max<size_t>(frame_bytes, 1));
        for (int f = 0; f < n_frames; f += per) out.push_back({ f, std::min(per, n_frames - f), 0, mcu_rows });
    }
    return out;
}

// a chunk's planes sit one behind the other in its slot, this many bytes apart (a multiple of 16: the aligned kernel stays usable)
inline size_t plane_pitch(const std::vector<HostChunk>& chunks, int W, int H)
{
    size_t P = 0;
    for (const HostChunk& k : chunks) P = std::max(P, k.plane_bytes(W, H));
    return (P + 15) & ~(size_t)15;
}

// packed (interleaved) pixels: jpezy_capi_packed.hip, jpezy_capi_scaled.hip
struct PackedLayout {
    int bytes;                 // per pixel
    int off[3];                // byte of r, g, b inside a pixel
    size_t row_stride, frame_stride;
};

// format, strides and the 32-bit row-offset limit; before anything is touched
// (row_stride >= W * bytes and row_stride * H fits in 32 bits: so does the tight image, no caller needs a guard of its own for that)
inline int packed_layout(const char* who, int format, size_t row_stride, size_t frame_stride, int W, int H, PackedLayout* L)
{
    const int bytes = jpezy_pixel_bytes(format);
    if (bytes < 0) return set_err(JPEZY_E_BADARG, std::string(who) + ": unknown pixel format");
    const size_t tight = (size_t)W * bytes;
    const size_t rs = row_stride ? row_stride : tight;
    if (rs < tight) return set_err(JPEZY_E_BADARG, std::string(who) + ": row_stride smaller than W * bytes per pixel");
    if (rs > 0xFFFFFFFFull / (size_t)H) return set_err(JPEZY_E_BADARG, std::string(who) + ": row_stride * H must fit in 32 bits");
    const size_t need = (size_t)(H - 1) * rs + tight;
    const size_t fs = frame_stride ? frame_stride : (size_t)H * rs;
    if (fs < need) return set_err(JPEZY_E_BADARG, std::string(who) + ": frame_stride smaller than (H-1) * row_stride + W * bytes per pixel");
    const bool blue_first = format == JPEZY_PIX_BGR24 || format == JPEZY_PIX_BGRA32;
    *L = { bytes, { blue_first ? 2 : 0, 1, blue_first ? 0 : 2 }, rs, fs };
    return JPEZY_OK;
}

// planar YCbCr 4:2:0 samples: jpezy_capi_ycc.hip
struct YccLayout {
    int CW, CH;
    size_t ys, cs, yfs, cfs;      // resolved strides
};

// c_step, strides and the 32-bit row-offset limit (W, H already checked); before the context or a device is touched
// chroma_rows: the chroma planes' height where it is not ceil(H/2) -- H for 4:2:2 samples (jpezy_capi_ycc422.hip)
inline int ycc_layout(const char* who, int W, int H, size_t y_stride, size_t c_stride, int c_step, size_t y_frame_stride, size_t c_frame_stride,
                      YccLayout* L, int chroma_rows = 0)
{
    if (c_step != 1 && c_step != 2) return set_err(JPEZY_E_BADARG, std::string(who) + ": c_step must be 1 (planes) or 2 (one interleaved plane)");
    const int CW = (W + 1) / 2, CH = chroma_rows ? chroma_rows : (H + 1) / 2;
    const size_t ys = y_stride ? y_stride : (size_t)W;
    const size_t c_min = (size_t)(CW - 1) * c_step + 1;
    const size_t cs = c_stride ? c_stride : (size_t)CW * c_step;
    if (ys < (size_t)W) return set_err(JPEZY_E_BADARG, std::string(who) + ": y_stride smaller than W");
    if (cs < c_min) return set_err(JPEZY_E_BADARG, std::string(who) + ": c_stride smaller than (CW-1) * c_step + 1");
    if (ys > 0xFFFFFFFFull / (size_t)H || cs > 0xFFFFFFFFull / (size_t)CH)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": y_stride * H and c_stride * CH must fit in 32 bits");
    const size_t yfs = y_frame_stride ? y_frame_stride : (size_t)H * ys;
    const size_t cfs = c_frame_stride ? c_frame_stride : (size_t)CH * cs;
    if (yfs < (size_t)(H - 1) * ys + (size_t)W) return set_err(JPEZY_E_BADARG, std::string(who) + ": y_frame_stride smaller than (H-1) * y_stride + W");
    if (cfs < (size_t)(CH - 1) * cs + c_min) return set_err(JPEZY_E_BADARG, std::string(who) + ": c_frame_stride smaller than a chroma plane");
    *L = { CW, CH, ys, cs, yfs, cfs };
    return JPEZY_OK;
}

// packed YCbCr 4:2:2 macropixels (YUY2 / UYVY / YVYU): jpezy_capi_ycc422.hip
struct Yuv422Layout {
    int off[3];                // byte of Y0, Cb, Cr inside a macropixel (Y1 two behind Y0)
    size_t row_bytes, row_stride, frame_stride;
};

// format, strides and the 32-bit row-offset limit (W, H already checked); before the context or a device is touched
inline int yuv422_layout(const char* who, int format, size_t row_stride, size_t frame_stride, int W, int H, Yuv422Layout* L)
{
    if (format != JPEZY_YUV_YUY2 && format != JPEZY_YUV_UYVY && format != JPEZY_YUV_YVYU)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": format must be JPEZY_YUV_YUY2, JPEZY_YUV_UYVY or JPEZY_YUV_YVYU");
    const size_t row_bytes = (size_t)4 * ((W + 1) / 2);
    const size_t rs = row_stride ? row_stride : row_bytes;
    if (rs < row_bytes) return set_err(JPEZY_E_BADARG, std::string(who) + ": row_stride smaller than 4 * ceil(W/2)");
    if (rs > 0xFFFFFFFFull / (size_t)H) return set_err(JPEZY_E_BADARG, std::string(who) + ": row_stride * H must fit in 32 bits");
    const size_t fs = frame_stride ? frame_stride : (size_t)H * rs;
    if (fs < (size_t)(H - 1) * rs + row_bytes)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": frame_stride smaller than (H-1) * row_stride + 4 * ceil(W/2)");
    const bool uyvy = format == JPEZY_YUV_UYVY, yvyu = format == JPEZY_YUV_YVYU;
    *L = { { uyvy ? 1 : 0, uyvy ? 0 : yvyu ? 3 : 1, uyvy ? 2 : yvyu ? 1 : 3 }, row_bytes, rs, fs };
    return JPEZY_OK;
}

}  // namespace jpezy_capi
using namespace jpezy_capi;

struct jpezy_ctx {
    int device = 0;
    Stream stream;
    DevBuf d_tab;                  // DeviceTables
    DevBuf d_counter;              // unsigned long long [COUNTER_SHARDS]
    DevBuf d_dqscale;              // double [3][8][8]
    DevBuf d_dqt;                  // int [3][64]
    DevBuf d_dqscale_f;            // float [8][8] luma constants in FP32 (decode tolerance mode)
    int dec_tolerance = 0;         // 0 = bit-exact decode (default), 1 = luma in FP32, output within one of the reference per channel
    uint16_t dq_cache[3][64];
    int coef_limit = 0;            // 2^15 / largest quantiser: the generic kernels and the tolerance mode of the fused kernel
    int coef_limit_exact = 0;      // 2^23 / largest quantiser: the fused kernel's exact mode (fast path + reference sum err by <= 1.2e-6 against a guard band of 3.8e-6)
    bool dq_valid = false;
    int force_exact = 0;           // 0 normal, 1 everything through the reference-order path, 2 (f32 variant) through level 2,
                                   // 3 (f32 variant) through the per-lane evaluator of the queue-overflow case
#ifndef JPEZY_DEFAULT_VARIANT
#define JPEZY_DEFAULT_VARIANT 1
#endif
    int variant = JPEZY_DEFAULT_VARIANT;   // encode kernel: 0 = FP64 butterflies, 1 = FP32 first level (default), 2 = variant 1's arithmetic in persistent workgroups
    int n_cus = 0;                 // compute units of the device (grid of the persistent kernel)
    float dc_rq[2] = { 0, 0 }, dc_bias[2] = { 0, 0 };   // f32::dc_formula's constants; 0: the table-free DC does not reproduce the DC table (build_encode_tables)
    uint8_t qt[2][64];             // the quantisation tables d_tab was built from (natural order): the header's DQT segments, jpezy_ctx_quant_tables
    bool qt_default = true;        // ... are the Annex-K tables
    int chroma_downsampling = 0;   // JPEZY_DOWNSAMPLE_POINT; read when a colour 4:2:0 RGB transform is launched (jpezy_ctx_set_chroma_downsampling)
    bool dc_table_lookup = false;  // test hook (jpezy_ctx_set_dc_table_lookup): the DC from DeviceTables::dcq even where the checks allow the quantiser
    int encode_groups = 0;         // JPEZY_ENCODE_GROUPS_AUTO; a forced workgroup form of variant 1's planar launch (jpezy_ctx_set_encode_groups)
    DevBuf d_trace;                // JPEZY_TRACE builds: 4 words per wave + 9 phase stamps (JPEZY_TRACE=3)
    DevBuf dump_t;                 // JPEZY_DUMP_T builds: level-1 t values of the last jpezy_fdct_quant_dev call
    DevBuf in[3], out, scratch;    // staging for the host-buffer entry points; scratch: samples of the generic decoder
    // GPU entropy coder (jpezy_entropy.hip): code tables + the scratch of a pass (entropy::Scratch; jpezy_capi_entropy.hip's Pass::plan
    // sizes them by entropy::scratch_sizes)
    DevBuf d_codes;                // jpezy_dev::entropy::CodeTables, the Annex-K image (ensure_code_tables)
    DevBuf e_S, e_tt;              // tile streams; tile totals (bits)
    DevBuf e_base, e_ft;           // frame-relative tile bit offsets, first tile per 16 KB piece of output: frames whose assembling kernel does not scan the totals itself
    DevBuf e_U;                    // unstuffed streams
    DevBuf e_cnt, e_fft;           // bytes stuffing adds: in front of a chunk (64 bytes) inside its piece (256 chunks), and per piece
    DevBuf e_small;                // [F] stream bytes (uint64) | [F] bytes stuffing adds (uint64, host-delivered form) | [F] flags (uint32): the
                                   // host-delivered form's error flags, the device-resident form's latched copy of e_status
    DevBuf e_status;               // per-frame error flags of the device-resident entropy path: zero between calls (cleared by their consumer)
    DevBuf e_out, e_coef;          // host-delivered form: stuffed streams; jpezy_encode_jpeg[_packed]: the frame's coefficients
    DevBuf e_tmp;                  // scratch of entropy::launch_scan_u32 (GPU Huffman decoder)
    PinBuf e_pinned;               // pinned host staging of the stuffed streams
    DevBuf x_coef;                 // jpezy_transform_jpeg: the transformed coefficients (the source's lie in `out`)
    int huff_optimize = 0;         // 1: the host-delivered entropy entry points build every frame's own Huffman tables (jpezy_ctx_set_huffman_optimize)
    DevBuf e_hist, e_hstat;        // per-image tables: symbol counts [frames][4][256] uint64; error flags of jpezy_huffman_histogram_dev (never read)
    DevBuf e_codes_opt;            // ... and the frames' CodeTables images [frames]
    int restart_interval = 0;      // MCUs per restart interval the entropy entry points write (jpezy_ctx_set_restart_interval); 0: none
    DevBuf e_rpad, e_mk;           // restart intervals: pad bits in front of every interval (uint64), RSTn markers behind a chunk's bytes (uint64 mask)
    PinBuf e_hist_pin, e_codes_pin;    // pinned host twins of the two
    DevBuf h_scan, h_U, h_cnt, h_off, h_state, h_setup, h_small, h_dc, h_dcbuf;   // GPU Huffman decoder (jpezy_huffdec.hip)
    std::vector<uint8_t> h_setup_host;  // the device tables h_setup holds (jpezy_read_jpeg_gpu uploads them only when they change)
    const void* h_setup_dev = nullptr;  // ... and the allocation they were uploaded to
    PinBuf h_fb_pin;                    // pinned buffer for the host decoder's coefficients (read_jpeg_host_to_device)
    int h_last_passes = 0;         // synchronisation passes of the last jpezy_read_jpeg_gpu (0: the host decoder was used)
    size_t h_min_bytes = 32 << 10;    // scans shorter than this are decoded on the host: the GPU path has ~0.32 ms of fixed cost, the host decoder
                                      // takes ~10.5 us per KiB of scan (tools/measure/huffdec_threshold.py, profiles/r04_huffdec_threshold.txt: they cross at
                                      // ~30 KiB; round 3: 0.6 ms, 64 KiB; round 2: 3 ms, 256 KiB)
    static constexpr int B_DEPTH = 3;   // slices of jpezy_decode_jpeg_batch whose planes may be on their way to the host while the next one is decoded
    DevBuf b_scan, b_U, b_cnt, b_rb, b_state, b_prop, b_meta, b_coef, b_planes[B_DEPTH];   // jpezy_decode_jpeg_batch, batch form of the Huffman decoder
    int b_last_fast = 0;           // files of the last jpezy_decode_jpeg_batch call that took the batch form (diagnostic hook)
    PinBuf b_pin;                  // pinned staging of the concatenated scans
    PinBuf b_stage[B_DEPTH];       // pinned staging of a slice's planes (one download per slice)
    PinBuf w_pin;                  // jpezy_decode_windows_dev: pinned staging of a slice's dequantiser sets and window descriptors
    DevBuf w_tab;                  // ... and their device copy
    int w_slice_files = 0;         // files per slice of its grouped path; 0: automatic (jpezy_ctx_set_windows_slice_files)
    int w_upsampling = 0;          // chroma upsampling of the two windows entries: JPEZY_UPSAMPLE_NEAREST (jpezy_ctx_set_windows_upsampling)
    int w_orientation = 0;         // 1: the windows entries honour every file's EXIF orientation (jpezy_ctx_set_windows_orientation)
    DevBuf w_scr;                  // jpezy_decode_windows_resized_dev: a slice's (a child context: one file's) windows as decoded, packed pixels
    PinBuf r_pin;                  // ... pinned staging of a launch's resample descriptors and tap tables
    DevBuf r_tab;                  // ... and their device copy
    int w_filter = 0;              // resampling filter of the resized and the tensor entry: JPEZY_FILTER_BILINEAR (jpezy_ctx_set_windows_filter)
    int r_direct = 0;              // 1: the direct loop for every file, never the two-pass tile (jpezy_ctx_set_resample_direct)
    int r_last_tiled = 0;          // files of the last resized / tensor call that took the two-pass tile (jpezy_ctx_last_resample_tiled_count)
    DevBuf e_hdr;                  // JFIF header bytes of the device-resident variant (cached per W, H, comment)
    jpezy_host::HostPipe pipe;     // staging ring of the streaming host-buffer entry points (jpezy_hostpipe.h)
    size_t host_chunk_bytes = 4u << 20;   // bytes of input per chunk of that pipeline (jpezy_ctx_set_host_chunk_bytes)
    bool is_batch_child = false;       // a worker of jpezy_decode_jpeg_batch: only ever driven on its own stream
    std::vector<jpezy_ctx*> workers;   // jpezy_decode_jpeg_batch: one child context (stream, buffers, tables) per file in flight
    uint8_t e_hdr_host[1024];
    size_t e_hdr_len = 0;

    // the children first, then nothing of this context in flight; after that the members free themselves
    ~jpezy_ctx()
    {
        for (jpezy_ctx* w : workers) delete w;
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

// The chunks of a streaming host-buffer entry through the context's staging ring (jpezy_hostpipe.h).  plan(i): the host segments of
// chunk i; transform(i, d_in, d_out, stream): its stage on the staged buffers, a C status.  The status of a failed stage, and its
// message, win over the pipeline's error.
template <class Plan, class Transform>
int run_host_bands(jpezy_ctx* c, size_t chunks, size_t max_in, size_t max_out, Plan plan, Transform transform)
{
    int rc_stage = JPEZY_OK;
    std::string err;
    auto stage = [&](int i, uint8_t* d_in, uint8_t* d_out, hipStream_t s) -> hipError_t {
        const int rc = transform(i, d_in, d_out, s);
        if (rc != JPEZY_OK) { rc_stage = rc; return hipErrorLaunchFailure; }
        return hipSuccess;
    };
    const hipError_t e = c->pipe.run(c->device, c->stream, (int)chunks, max_in, max_out, plan, stage, &err);
    if (rc_stage != JPEZY_OK) return rc_stage;
    if (e != hipSuccess) return set_err(JPEZY_E_HIP, err.empty() ? std::string("host pipeline: ") + hipGetErrorString(e) : err);
    return JPEZY_OK;
}

// ---- helpers shared by the translation units (C linkage, hidden: not part of the ABI) ----
// streams of the batch form of the GPU Huffman decoder (jpezy_capi_huffdec.hip)
// A stream is an entropy-coded segment that starts in the known state (bit 0, block 0, DC, predictors 0): the scan of a file
// (jpezy_decode_jpeg_batch: one stream per file, every file with its own tables) or one restart interval of a scan
// (jpezy_read_jpeg_gpu: the intervals of a file share one set of tables).  All streams of a call have the same MCU structure.
struct DevStream {
    const uint8_t* scan;                // host memory: the segment, up to (not including) the marker that ends it
    size_t n;
    unsigned total_blocks;              // blocks the stream holds (whole MCUs)
    unsigned long long coeff_off;       // int16 offset of its first coefficient in the output
    unsigned setup;                     // index into the call's tables
};
struct StreamGeom {
    unsigned bpm, ncomp, cstart[3], ccount[3];      // blocks per MCU; component q owns blocks [cstart, cstart + ccount) of every MCU
};

#define JPEZY_INTERNAL __attribute__((visibility("hidden")))
extern "C" {
JPEZY_INTERNAL int jpezy_internal_check_dims(const jpezy_ctx* c, int W, int H, int n_frames);
// the cached dequantiser tables
JPEZY_INTERNAL int jpezy_internal_upload_dequant(jpezy_ctx* c, const uint16_t qt[4][64], const uint8_t comp_tq[3], hipStream_t s);
// the GPU Huffman decoder over a list of independent streams, the device tables of one scan, the block structure of an MCU (jpezy_capi_huffdec.hip)
JPEZY_INTERNAL int jpezy_internal_huffdec_streams(jpezy_ctx* c, const std::vector<DevStream>& streams, const std::vector<jpezy_dev::huffdec::Setup>& setups,
                                                  const std::vector<char>& setup_usable, const StreamGeom& geom, int16_t* d_coef, size_t coef_elems,
                                                  std::vector<char>& ok, const std::function<void(const char*)>& lap, bool per_lane);
JPEZY_INTERNAL bool jpezy_internal_build_dev_setup(jpezy_dev::huffdec::Setup& S, const jpezy_host::ScanSetup& setup, const jpezy_frame_info& info, unsigned total_blocks);
JPEZY_INTERNAL StreamGeom jpezy_internal_stream_geom(const jpezy_frame_info& info);
// the GPU entropy coder's entries for a sampling (jpezy_capi_entropy.hip): jpezy_write_jpeg_gpu_dev / _batch and jpezy_huffman_histogram_dev
// are these at JPEZY_SAMPLING_420; with JPEZY_SAMPLING_444 / JPEZY_SAMPLING_422 gray is 0 (the callers refuse it) and d_coeffs holds 3- / 4-block MCUs.
// luma, chroma: the tables of the header's two DQT segments for this call (natural order, entries 1..255; both null: the context's, which
// is what every public writer passes) -- jpezy_transform_jpeg states the source file's tables without touching the context's setting
JPEZY_INTERNAL int jpezy_internal_write_jpeg_gpu_dev(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int sampling, int n_frames,
                                                     const char* comment, uint8_t* d_out, size_t out_stride, long long* d_sizes, void* stream,
                                                     const uint8_t* luma = nullptr, const uint8_t* chroma = nullptr);
JPEZY_INTERNAL int jpezy_internal_write_jpeg_gpu_batch(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int sampling, int n_frames,
                                                       const char* comment, uint8_t* out, size_t cap, long* sizes, const uint8_t* luma = nullptr,
                                                       const uint8_t* chroma = nullptr);
JPEZY_INTERNAL int jpezy_internal_huffman_histogram_dev(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int sampling, int n_frames,
                                                        unsigned long long* d_hist, void* stream);
}
