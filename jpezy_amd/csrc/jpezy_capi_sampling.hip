// jpezy_capi_sampling.hip -- the C-ABI of include/jpezy_hip.h, part 9: chroma sampling as an argument of the encoder's entry points.
// JPEZY_SAMPLING_420 is the existing entry of the same name without _sampling -- the same kernels, the same bytes --; JPEZY_SAMPLING_444 is the
// reference's per-sample arithmetic with make_YCC's decimation (encoder/jpezy_encoder.hpp:116-143) left out: 8 x 8 MCUs of Y, Cb, Cr
// (include/jpezy_hip.h has the definition).  The transform is jpezy_kernels_f32_444.hip (the kernel body and the launcher, shared with
// 4:2:2, are jpezy_f32_octet.h's); the Huffman stage is the GPU entropy coder with
// the MCU layout 3 / 1 / 3 (jpezy_entropy.h, Job::coded / luma) or the host writer (jpezy_host_codec.cpp, McuLayout).
// JPEZY_SAMPLING_422 is the same per-sample arithmetic with make_YCC's decimation applied horizontally only: 16 x 8 MCUs of Y, Y, Cb, Cr,
// layout 4 / 2 / 4; the transform is jpezy_kernels_f32_422.hip, which also holds the averaged (h2v1) chroma stage that the context's
// JPEZY_DOWNSAMPLE_AVERAGE setting selects.
#include "jpezy_capi_internal.h"

namespace jpezy_dev {
hipError_t launch_fdct_quant_f32_444(const EncParams& p, int force, hipStream_t stream);   // jpezy_kernels_f32_444.hip
hipError_t launch_fdct_quant_f32_422(const EncParams& p, int force, bool average, hipStream_t stream);   // jpezy_kernels_f32_422.hip
}

namespace {

int check_sampling(int sampling, const char* who)
{
    if (jpezy_host::sampling_known(sampling)) return JPEZY_OK;
    return set_err(JPEZY_E_BADARG, std::string(who) + ": unknown sampling (JPEZY_SAMPLING_420 = 0, JPEZY_SAMPLING_444 = 1, JPEZY_SAMPLING_422 = 3)");
}

const char* sampling_name(int sampling) { return sampling == JPEZY_SAMPLING_422 ? "JPEZY_SAMPLING_422" : "JPEZY_SAMPLING_444"; }

// gray together with 4:4:4 or 4:2:2: such a gray file has no use that the gray 4:2:0 file lacks
int check_gray(int sampling, int gray, const char* who)
{
    if (sampling != JPEZY_SAMPLING_420 && gray)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": gray is not available with " + sampling_name(sampling));
    return JPEZY_OK;
}

// what every 4:4:4 / 4:2:2 transform entry refuses before it touches anything: encode variant 0 (the FP64 kernel has neither form)
int check_variant(const jpezy_ctx* c, int sampling, const char* who)
{
    if (c->variant == 0)
        return set_err(JPEZY_E_UNSUPPORTED, std::string(who) + ": encode variant 0 (FP64) has no " + sampling_name(sampling) + " form; use variant 1");
    return JPEZY_OK;
}

// EncParams of a 4:4:4 / 4:2:2 launch: 8 x 8 / 16 x 8 MCUs, work units of 8 MCUs per MCU row in quads_per_row
// (jpezy_f32_octet.h)
int enc_params_sampling(jpezy_ctx* c, int sampling, int W, int H, int n_frames, int16_t* d_coeffs, hipStream_t s, EncParams* p)
{
    if (int rc = jpezy_internal_enc_params(c, W, H, 0, n_frames, d_coeffs, s, p)) return rc;
    int bpm;
    jpezy_sampling_geometry(sampling, W, H, &p->mcu_cols, &p->mcu_rows, &bpm);
    p->coeffs_per_frame = jpezy_coeff_count_sampling(W, H, sampling);
    p->quads_per_row = (p->mcu_cols + 7) / 8;
    fast_div_setup((unsigned)p->quads_per_row, &p->qpr_magic, &p->qpr_shift);
    return JPEZY_OK;
}

int launch_sampling(jpezy_ctx* c, int sampling, const EncParams& p, size_t frame_stride, int n_frames, hipStream_t s)
{
    for (int f0 = 0; f0 < n_frames; f0 += kMaxFramesPerLaunch) {
        EncParams q = p;
        q.n_frames = n_frames - f0 < kMaxFramesPerLaunch ? n_frames - f0 : kMaxFramesPerLaunch;
        const size_t adv = (size_t)f0 * frame_stride;
        if (q.pix) q.pix += adv;
        q.r += adv; q.g += adv; q.b += adv;
        q.coeffs += (size_t)f0 * p.coeffs_per_frame;
        // (the laboratory's persistent variants 2 and 3 hand 4:4:4 to this launch as they do every frame they do not cover)
        // 4:2:2 decimates, so the context's chroma-downsampling setting is read here, at launch, as the 4:2:0 transforms read it
        if (sampling == JPEZY_SAMPLING_422) HIP_TRY(launch_fdct_quant_f32_422(q, c->force_exact, c->chroma_downsampling == JPEZY_DOWNSAMPLE_AVERAGE, s));
        else HIP_TRY(launch_fdct_quant_f32_444(q, c->force_exact, s));
    }
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
    if (int rc = check_variant(c, sampling, "fdct_quant_sampling_dev")) return rc;
    if (!d_r || !d_g || !d_b || !d_coeffs) return set_err(JPEZY_E_BADARG, "null device pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    if (plane_stride < (size_t)W * H) return set_err(JPEZY_E_BADARG, "plane_stride smaller than W*H");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    EncParams p;
    p.r = d_r; p.g = d_g; p.b = d_b;
    p.plane_stride = plane_stride;
    if (int rc = enc_params_sampling(c, sampling, W, H, n_frames, d_coeffs, s, &p)) return rc;
    return launch_sampling(c, sampling, p, plane_stride, n_frames, s);
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
    if (int rc = check_variant(c, sampling, "fdct_quant_sampling_packed_dev")) return rc;
    PackedLayout L;
    if (int rc = packed_layout("fdct_quant_sampling_packed_dev", format, row_stride, frame_stride, W, H, &L)) return rc;
    if (!d_pix || !d_coeffs) return set_err(JPEZY_E_BADARG, "null device pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    EncParams p;
    p.pix = d_pix;
    p.r = d_pix + L.off[0]; p.g = d_pix + L.off[1]; p.b = d_pix + L.off[2];
    p.plane_stride = L.frame_stride;
    p.row_stride = (unsigned)L.row_stride;
    p.pix_bytes = L.bytes;
    p.swap_rb = L.off[0] != 0;
    if (int rc = enc_params_sampling(c, sampling, W, H, n_frames, d_coeffs, s, &p)) return rc;
    return launch_sampling(c, sampling, p, L.frame_stride, n_frames, s);
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

}  // extern "C"

namespace {

// 4:4:4 / 4:2:2 end to end: pixels up, the transform kernel, then the GPU writer on the frame's coefficients (the context's quantisation tables
// in the DQT segments, its restart interval and its optimise setting act there)
template <class UPLOAD_AND_LAUNCH>
long encode_sampling(jpezy_ctx* c, int sampling, int W, int H, const char* comment, uint8_t* out, size_t cap, UPLOAD_AND_LAUNCH up)
{
    const size_t ncoef = jpezy_coeff_count_sampling(W, H, sampling);
    if (int rc = c->e_coef.reserve(ncoef * sizeof(int16_t))) return rc;
    if (int rc = up(c->e_coef.as<int16_t>())) return rc;
    return jpezy_write_jpeg_gpu_sampling(c, c->e_coef.as<int16_t>(), W, H, sampling, 0, comment, out, cap);
}

}  // namespace

extern "C" {

// encoder::encode end to end (encoder/jpezy_encoder.hpp:38-77) for the sampling: host planes in, .jpg bytes out
long jpezy_encode_jpeg_sampling(jpezy_ctx* c, const uint8_t* r, const uint8_t* g, const uint8_t* b, int W, int H, int sampling, int gray,
                                const char* comment, uint8_t* out, size_t cap)
try {
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    if (int rc = check_sampling(sampling, "encode_jpeg_sampling")) return rc;
    if (int rc = check_gray(sampling, gray, "encode_jpeg_sampling")) return rc;
    if (sampling == JPEZY_SAMPLING_420) return jpezy_encode_jpeg(c, r, g, b, W, H, gray, comment, out, cap);
    if (int rc = check_variant(c, sampling, "encode_jpeg_sampling")) return rc;
    if (!r || !g || !b || !out) return set_err(JPEZY_E_BADARG, "encode_jpeg_sampling: null pointer");
    if (int rc = check_comment(comment, "encode_jpeg_sampling")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t P = ((size_t)W * H + 15) & ~(size_t)15;
    return encode_sampling(c, sampling, W, H, comment, out, cap, [&](int16_t* d_coef) -> int {
        if (int rc = c->in[0].reserve(3 * P)) return rc;
        uint8_t* d = (uint8_t*)c->in[0].p;
        const uint8_t* src[3] = { r, g, b };
        for (int q = 0; q < 3; ++q) HIP_TRY(hipMemcpyAsync(d + q * P, src[q], (size_t)W * H, hipMemcpyHostToDevice, c->stream));
        return jpezy_fdct_quant_sampling_dev(c, d, d + P, d + 2 * P, (size_t)W * H, W, H, sampling, 0, 1, d_coef, c->stream);
    });
}
JPEZY_CATCH

long jpezy_encode_jpeg_sampling_packed(jpezy_ctx* c, const uint8_t* pix, int format, size_t row_stride, int W, int H, int sampling, int gray,
                                       const char* comment, uint8_t* out, size_t cap)
try {
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    if (int rc = check_sampling(sampling, "encode_jpeg_sampling_packed")) return rc;
    if (int rc = check_gray(sampling, gray, "encode_jpeg_sampling_packed")) return rc;
    if (sampling == JPEZY_SAMPLING_420) return jpezy_encode_jpeg_packed(c, pix, format, row_stride, W, H, gray, comment, out, cap);
    if (int rc = check_variant(c, sampling, "encode_jpeg_sampling_packed")) return rc;
    PackedLayout L;
    if (int rc = packed_layout("encode_jpeg_sampling_packed", format, row_stride, 0, W, H, &L)) return rc;
    if (!pix || !out) return set_err(JPEZY_E_BADARG, "encode_jpeg_sampling_packed: null pointer");
    if (int rc = check_comment(comment, "encode_jpeg_sampling_packed")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the picture goes up as it lies in the caller's buffer, row padding included, up to the last byte of its last row
    const size_t bytes = (size_t)(H - 1) * L.row_stride + (size_t)W * L.bytes;
    return encode_sampling(c, sampling, W, H, comment, out, cap, [&](int16_t* d_coef) -> int {
        if (int rc = c->in[0].reserve(bytes)) return rc;
        HIP_TRY(hipMemcpyAsync(c->in[0].p, pix, bytes, hipMemcpyHostToDevice, c->stream));
        return jpezy_fdct_quant_sampling_packed_dev(c, (const uint8_t*)c->in[0].p, format, L.row_stride, 0, W, H, sampling, 0, 1, d_coef,
                                                    c->stream);
    });
}
JPEZY_CATCH

}  // extern "C"
