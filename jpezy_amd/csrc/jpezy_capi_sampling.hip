// jpezy_capi_sampling.hip -- the C-ABI of include/jpezy_hip.h, part 9: chroma sampling as an argument of the encoder's entry points.
// JPEZY_SAMPLING_420 is the existing entry of the same name without _sampling -- the same kernels, the same bytes --; JPEZY_SAMPLING_444 is the
// reference's per-sample arithmetic with make_YCC's decimation (encoder/jpezy_encoder.hpp:116-143) left out: 8 x 8 MCUs of Y, Cb, Cr
// (include/jpezy_hip.h has the definition).  The transform is jpezy_kernels_f32_444.hip (the kernel body and the launcher, shared with
// 4:2:2, are jpezy_f32_octet.h's); the Huffman stage is the GPU entropy coder with
// the MCU layout 3 / 1 / 3 (jpezy_entropy.h, Job::coded / luma) or the host writer (jpezy_host_codec.cpp, McuLayout).
// JPEZY_SAMPLING_422 is the same per-sample arithmetic with make_YCC's decimation applied horizontally only: 16 x 8 MCUs of Y, Y, Cb, Cr,
// layout 4 / 2 / 4; the transform is jpezy_kernels_f32_422.hip, which also holds the averaged (h2v1) chroma stage that the context's
// JPEZY_DOWNSAMPLE_AVERAGE setting selects.  The entries here check their own arguments, forward JPEZY_SAMPLING_420 to the plain entry and
// hand everything else to the transform core and the file-encode driver (jpezy_capi_encode.h).
#include "jpezy_capi_encode.h"

namespace {

int check_sampling(int sampling, const char* who)
{
    if (jpezy_host::sampling_known(sampling)) return JPEZY_OK;
    return set_err(JPEZY_E_BADARG, std::string(who) + ": unknown sampling (JPEZY_SAMPLING_420 = 0, JPEZY_SAMPLING_444 = 1, JPEZY_SAMPLING_422 = 3)");
}

// gray together with 4:4:4 or 4:2:2: such a gray file has no use that the gray 4:2:0 file lacks
int check_gray(int sampling, int gray, const char* who)
{
    if (sampling != JPEZY_SAMPLING_420 && gray)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": gray is not available with " + sampling_name(sampling));
    return JPEZY_OK;
}

}  // namespace

extern "C" {

int jpezy_sampling_geometry(int sampling, int W, int H, int* mcu_cols, int* mcu_rows, int* blocks_per_mcu)
{
    if (int rc = check_sampling(sampling, "sampling_geometry")) return rc;
    if (int rc = check_wh(W, H)) return rc;
    const jpezy_host::McuLayout L = jpezy_host::mcu_layout(sampling, false);
    if (mcu_cols) *mcu_cols = (W + L.mcu_w - 1) / L.mcu_w;
    if (mcu_rows) *mcu_rows = (H + L.mcu_h - 1) / L.mcu_h;
    if (blocks_per_mcu) *blocks_per_mcu = L.stored;
    return JPEZY_OK;
}

size_t jpezy_coeff_count_sampling(int W, int H, int sampling)
{
    int mc, mr, bpm;
    if (jpezy_sampling_geometry(sampling, W, H, &mc, &mr, &bpm) != JPEZY_OK) return 0;
    return (size_t)mc * (size_t)mr * (size_t)bpm * 64;
}

size_t jpezy_jpeg_bound_sampling(int W, int H, int sampling)
{
    if (check_sampling(sampling, "jpeg_bound_sampling") != JPEZY_OK || check_wh(W, H) != JPEZY_OK) return 0;
    return jpezy_host::jpeg_bound_sampling(W, H, sampling);
}

// stands in for encoder/jpezy_encoder.hpp:90-172 (make_YCC without :116-143, DCT, quantization) on 8 x 8 MCUs
int jpezy_fdct_quant_sampling_dev(jpezy_ctx* c, const uint8_t* d_r, const uint8_t* d_g, const uint8_t* d_b, size_t plane_stride, int W, int H,
                                  int sampling, int gray, int n_frames, int16_t* d_coeffs, void* stream)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (int rc = check_sampling(sampling, "fdct_quant_sampling_dev")) return rc;
    if (int rc = check_gray(sampling, gray, "fdct_quant_sampling_dev")) return rc;
    if (sampling == JPEZY_SAMPLING_420) return jpezy_fdct_quant_dev(c, d_r, d_g, d_b, plane_stride, W, H, gray, n_frames, d_coeffs, stream);
    if (int rc = check_encode_variant(c, sampling, 0, "fdct_quant_sampling_dev")) return rc;
    if (!d_r || !d_g || !d_b || !d_coeffs) return set_err(JPEZY_E_BADARG, "null device pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    if (plane_stride < (size_t)W * H) return set_err(JPEZY_E_BADARG, "plane_stride smaller than W*H");
    return jpezy_internal_fdct_quant_core(c, EncodeSource::planes(d_r, d_g, d_b, plane_stride), sampling, W, H, 0, n_frames, d_coeffs, (hipStream_t)stream);
}

// the same from packed pixels (jpezy_fdct_quant_packed_dev's formats, strides and limits)
int jpezy_fdct_quant_sampling_packed_dev(jpezy_ctx* c, const uint8_t* d_pix, int format, size_t row_stride, size_t frame_stride, int W, int H,
                                         int sampling, int gray, int n_frames, int16_t* d_coeffs, void* stream)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (int rc = check_sampling(sampling, "fdct_quant_sampling_packed_dev")) return rc;
    if (int rc = check_gray(sampling, gray, "fdct_quant_sampling_packed_dev")) return rc;
    if (sampling == JPEZY_SAMPLING_420)
        return jpezy_fdct_quant_packed_dev(c, d_pix, format, row_stride, frame_stride, W, H, gray, n_frames, d_coeffs, stream);
    if (int rc = check_encode_variant(c, sampling, 0, "fdct_quant_sampling_packed_dev")) return rc;
    PackedLayout L;
    if (int rc = packed_layout("fdct_quant_sampling_packed_dev", format, row_stride, frame_stride, W, H, &L)) return rc;
    if (!d_pix || !d_coeffs) return set_err(JPEZY_E_BADARG, "null device pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    return jpezy_internal_fdct_quant_core(c, EncodeSource::packed(L, d_pix), sampling, W, H, 0, n_frames, d_coeffs, (hipStream_t)stream);
}

// the reference's writer (encoder/jpezy_writer.hpp:20-105, encoder/jpezy_encoder.hpp:174-242) for the sampling's scan: jpezy_write_jpeg_qt
long jpezy_write_jpeg_sampling(const int16_t* coeffs, int W, int H, int sampling, int gray, const char* comment, const uint8_t luma[64],
                               const uint8_t chroma[64], int restart_interval, int optimize, uint8_t* out, size_t cap)
try {
    if (int rc = check_sampling(sampling, "write_jpeg_sampling")) return rc;
    if (int rc = check_gray(sampling, gray, "write_jpeg_sampling")) return rc;
    if (sampling == JPEZY_SAMPLING_420) return jpezy_write_jpeg_qt(coeffs, W, H, gray, comment, luma, chroma, restart_interval, optimize, out, cap);
    if ((luma == nullptr) != (chroma == nullptr))
        return set_err(JPEZY_E_BADARG, "write_jpeg_sampling: one of the two tables is null (both null: Annex K)");
    for (int k = 0; luma && k < 64; ++k)
        if (!luma[k] || !chroma[k]) return set_err(JPEZY_E_BADARG, "write_jpeg_sampling: a quantisation table entry is zero (1..255)");
    std::string err;
    const long n = jpezy_host::write_jpeg_sampling(coeffs, W, H, sampling, comment, restart_interval, optimize != 0, out, cap, &err, luma, chroma);
    if (n < 0) g_err = err;
    return n;
}
JPEZY_CATCH

// jpezy_write_jpeg_gpu[_batch, _dev] for the sampling: the GPU entropy coder (Huffman coding, bit packing, byte stuffing, RSTn) on 3-block
// (4:2:2: 4-block) MCUs; same bytes as jpezy_write_jpeg_sampling with the context's tables, restart interval and optimise setting
int jpezy_write_jpeg_gpu_sampling_batch(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int sampling, int gray, int n_frames,
                                        const char* comment, uint8_t* out, size_t cap, long* sizes)
{
    if (int rc = check_sampling(sampling, "write_jpeg_gpu_sampling")) return rc;
    if (int rc = check_gray(sampling, gray, "write_jpeg_gpu_sampling")) return rc;
    return jpezy_internal_write_jpeg_gpu_batch(c, d_coeffs, W, H, gray, sampling, n_frames, comment, out, cap, sizes);
}

long jpezy_write_jpeg_gpu_sampling(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int sampling, int gray, const char* comment, uint8_t* out,
                                   size_t cap)
{
    long size = 0;
    const int rc = jpezy_write_jpeg_gpu_sampling_batch(c, d_coeffs, W, H, sampling, gray, 1, comment, out, cap, &size);
    if (rc != JPEZY_OK && size >= 0) return rc;
    if (size == JPEZY_E_FORMAT) set_err(JPEZY_E_FORMAT, "write_jpeg_gpu_sampling: coefficient outside the code tables");
    if (size == JPEZY_E_NOSPACE) set_err(JPEZY_E_NOSPACE, "write_jpeg_gpu_sampling: output buffer too small");
    return size;
}

// asynchronous and capturable; JPEZY_E_UNSUPPORTED while Huffman optimisation is on, as jpezy_write_jpeg_gpu_dev
int jpezy_write_jpeg_gpu_sampling_dev(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int sampling, int gray, int n_frames, const char* comment,
                                      uint8_t* d_out, size_t out_stride, long long* d_sizes, void* stream)
{
    if (int rc = check_sampling(sampling, "write_jpeg_gpu_sampling_dev")) return rc;
    if (int rc = check_gray(sampling, gray, "write_jpeg_gpu_sampling_dev")) return rc;
    return jpezy_internal_write_jpeg_gpu_dev(c, d_coeffs, W, H, gray, sampling, n_frames, comment, d_out, out_stride, d_sizes, stream);
}

// jpezy_huffman_histogram_dev for the sampling
int jpezy_huffman_histogram_sampling_dev(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int sampling, int gray, int n_frames,
                                         unsigned long long* d_hist, void* stream)
{
    if (int rc = check_sampling(sampling, "huffman_histogram_sampling_dev")) return rc;
    if (int rc = check_gray(sampling, gray, "huffman_histogram_sampling_dev")) return rc;
    return jpezy_internal_huffman_histogram_dev(c, d_coeffs, W, H, gray, sampling, n_frames, d_hist, stream);
}

// the symbols that writer emits (host; restart_interval as the writer's): hist[k][sym], DHT order YDc, CDc, YAc, CAc.
// JPEZY_E_FORMAT when a value lies outside the code tables (counted as the clamped symbol)
int jpezy_huffman_histogram_sampling(const int16_t* coeffs, int W, int H, int sampling, int restart_interval, unsigned long long hist[4][256])
{
    if (int rc = check_sampling(sampling, "huffman_histogram_sampling")) return rc;
    if (int rc = check_wh(W, H)) return rc;
    if (!coeffs || !hist || restart_interval < 0) return set_err(JPEZY_E_BADARG, "huffman_histogram_sampling: bad argument");
    if (!jpezy_host::symbol_histogram_sampling(coeffs, W, H, sampling, hist, restart_interval))
        return set_err(JPEZY_E_FORMAT, "huffman_histogram_sampling: coefficient outside the code tables");
    return JPEZY_OK;
}

// encoder::encode end to end (encoder/jpezy_encoder.hpp:38-77) for the sampling: host planes in, .jpg bytes out
long jpezy_encode_jpeg_sampling(jpezy_ctx* c, const uint8_t* r, const uint8_t* g, const uint8_t* b, int W, int H, int sampling, int gray,
                                const char* comment, uint8_t* out, size_t cap)
try {
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    if (int rc = check_sampling(sampling, "encode_jpeg_sampling")) return rc;
    if (int rc = check_gray(sampling, gray, "encode_jpeg_sampling")) return rc;
    if (sampling == JPEZY_SAMPLING_420) return jpezy_encode_jpeg(c, r, g, b, W, H, gray, comment, out, cap);
    if (int rc = check_encode_variant(c, sampling, 0, "encode_jpeg_sampling")) return rc;
    if (!r || !g || !b || !out) return set_err(JPEZY_E_BADARG, "encode_jpeg_sampling: null pointer");
    if (int rc = check_comment(comment, "encode_jpeg_sampling")) return rc;
    return jpezy_internal_encode_file(c, planar_encode_request(r, g, b, W, H, sampling, 0, comment, out, cap));
}
JPEZY_CATCH

long jpezy_encode_jpeg_sampling_packed(jpezy_ctx* c, const uint8_t* pix, int format, size_t row_stride, int W, int H, int sampling, int gray,
                                       const char* comment, uint8_t* out, size_t cap)
try {
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    if (int rc = check_sampling(sampling, "encode_jpeg_sampling_packed")) return rc;
    if (int rc = check_gray(sampling, gray, "encode_jpeg_sampling_packed")) return rc;
    if (sampling == JPEZY_SAMPLING_420) return jpezy_encode_jpeg_packed(c, pix, format, row_stride, W, H, gray, comment, out, cap);
    if (int rc = check_encode_variant(c, sampling, 0, "encode_jpeg_sampling_packed")) return rc;
    PackedLayout L;
    if (int rc = packed_layout("encode_jpeg_sampling_packed", format, row_stride, 0, W, H, &L)) return rc;
    if (!pix || !out) return set_err(JPEZY_E_BADARG, "encode_jpeg_sampling_packed: null pointer");
    if (int rc = check_comment(comment, "encode_jpeg_sampling_packed")) return rc;
    return jpezy_internal_encode_file(c, packed_encode_request(pix, L, W, H, sampling, 0, comment, out, cap));
}
JPEZY_CATCH

}  // extern "C"
