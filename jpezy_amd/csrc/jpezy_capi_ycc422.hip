// jpezy_capi_ycc422.hip -- the C-ABI of include/jpezy_hip_ycc422.h: YCbCr 4:2:2 samples in and out -- planar I422 / YV16 / NV16 / NV61 and
// packed macropixels YUY2 / UYVY / YVYU.  The caller's bytes are a 4:2:2 file's own sample domain: the encode kernel skips the colour
// conversion (load step and sample stage differ, jpezy_kernels_f32_422_ycc.hip), the decode's second stage skips make_rgb
// (generic_yuv422_kernel); coefficients keep the 4:2:2 layout, so the Huffman stages, optimised tables, restart intervals and the file
// header are the RGB 4:2:2 entries'.
#include "jpezy_capi_decode.h"
#include "jpezy_capi_encode.h"

namespace {

// the checks of the two packed encode entries that come before the context
int yuv422_head(const char* who, int format, size_t row_stride, size_t frame_stride, int W, int H, Yuv422Layout* L)
{
    if (int rc = check_wh(W, H)) return rc;
    return yuv422_layout(who, format, row_stride, frame_stride, W, H, L);
}

}  // namespace

extern "C" {

int jpezy_yuv422_row_bytes(int W)
{
    if (int rc = check_wh(W, 1)) return rc;
    return 4 * ((W + 1) / 2);
}

int jpezy_ycc422_chroma_size(int W, int H, int* CW, int* CH)
{
    if (int rc = check_wh(W, H)) return rc;
    if (CW) *CW = (W + 1) / 2;
    if (CH) *CH = H;
    return JPEZY_OK;
}

int jpezy_fdct_quant_ycc422_dev(jpezy_ctx* c, const uint8_t* d_y, size_t y_stride, const uint8_t* d_cb, const uint8_t* d_cr, size_t c_stride,
                                int c_step, size_t y_frame_stride, size_t c_frame_stride, int W, int H, int n_frames, int16_t* d_coeffs,
                                void* stream)
{
    if (int rc = check_wh(W, H)) return rc;
    YccLayout L;
    if (int rc = ycc_layout("fdct_quant_ycc422_dev", W, H, y_stride, c_stride, c_step, y_frame_stride, c_frame_stride, &L, H)) return rc;
    if (!d_y || !d_cb || !d_cr || !d_coeffs) return set_err(JPEZY_E_BADARG, "fdct_quant_ycc422_dev: null device pointer");
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    if (int rc = check_encode_variant(c, JPEZY_SAMPLING_422, 0, "fdct_quant_ycc422_dev")) return rc;
    return jpezy_internal_fdct_quant_core(c, EncodeSource::ycc422(d_y, d_cb, d_cr, L, c_step), JPEZY_SAMPLING_422, W, H, 0, n_frames, d_coeffs,
                                          (hipStream_t)stream);
}

int jpezy_fdct_quant_yuv422_dev(jpezy_ctx* c, const uint8_t* d_pix, int format, size_t row_stride, size_t frame_stride, int W, int H,
                                int n_frames, int16_t* d_coeffs, void* stream)
{
    Yuv422Layout L;
    if (int rc = yuv422_head("fdct_quant_yuv422_dev", format, row_stride, frame_stride, W, H, &L)) return rc;
    if (!d_pix || !d_coeffs) return set_err(JPEZY_E_BADARG, "fdct_quant_yuv422_dev: null device pointer");
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    if (int rc = check_encode_variant(c, JPEZY_SAMPLING_422, 0, "fdct_quant_yuv422_dev")) return rc;
    return jpezy_internal_fdct_quant_core(c, EncodeSource::yuv422(L, format, d_pix), JPEZY_SAMPLING_422, W, H, 0, n_frames, d_coeffs,
                                          (hipStream_t)stream);
}

// host planes -> .jpg bytes on the host: a file encode (jpezy_internal_encode_file) of one band with up to three input segments (the Y
// rows, and the chroma rows as two planes or as one interleaved plane), as jpezy_encode_jpeg_ycc's bands
long jpezy_encode_jpeg_ycc422(jpezy_ctx* c, const uint8_t* y, size_t y_stride, const uint8_t* cb, const uint8_t* cr, size_t c_stride, int c_step,
                              int W, int H, const char* comment, uint8_t* out, size_t cap)
try {
    if (int rc = check_wh(W, H)) return rc;
    YccLayout L;
    if (int rc = ycc_layout("encode_jpeg_ycc422", W, H, y_stride, c_stride, c_step, 0, 0, &L, H)) return rc;
    if (!y || !cb || !cr || !out) return set_err(JPEZY_E_BADARG, "encode_jpeg_ycc422: null pointer");
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    if (int rc = check_comment(comment, "encode_jpeg_ycc422")) return rc;
    if (int rc = check_encode_variant(c, JPEZY_SAMPLING_422, 0, "encode_jpeg_ycc422")) return rc;   // before anything is uploaded
    // one interleaved plane (Cb and Cr neighbours) travels as one segment: its rows hold 2 * CW sample bytes from the lower pointer
    const bool inter = c_step == 2 && (cb + 1 == cr || cr + 1 == cb);
    const uint8_t* c_lo = inter ? std::min(cb, cr) : nullptr;
    const size_t c_row_bytes = inter ? (size_t)2 * L.CW : (size_t)(L.CW - 1) * c_step + 1;
    // the planes go up as they lie in the caller's buffers, row padding included, up to the last sample byte of the last row
    const size_t y_bytes = (size_t)(H - 1) * L.ys + (size_t)W, c_bytes = (size_t)(H - 1) * L.cs + c_row_bytes;
    auto pad16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t o1 = pad16(y_bytes), o2 = o1 + pad16(c_bytes);
    return jpezy_internal_encode_file(c, { W, H, JPEZY_SAMPLING_422, 0, comment, out, cap, 2,
        [&](const HostChunk&, size_t, std::vector<jpezy_host::Segment>& in) {
            in.push_back({ const_cast<uint8_t*>(y), y_bytes, 0 });
            if (inter) {
                in.push_back({ const_cast<uint8_t*>(c_lo), c_bytes, o1 });
            } else {
                in.push_back({ const_cast<uint8_t*>(cb), c_bytes, o1 });
                in.push_back({ const_cast<uint8_t*>(cr), c_bytes, o2 });
            }
        },
        [&](const HostChunk&, size_t, const uint8_t* d_in) {
            return EncodeSource::ycc422(d_in, inter ? d_in + o1 + (cb > cr ? 1 : 0) : d_in + o1, inter ? d_in + o1 + (cr > cb ? 1 : 0) : d_in + o2, L, c_step);
        } });
}
JPEZY_CATCH

// host macropixels -> .jpg bytes on the host: one band, one segment
long jpezy_encode_jpeg_yuv422(jpezy_ctx* c, const uint8_t* pix, int format, size_t row_stride, int W, int H, const char* comment, uint8_t* out,
                              size_t cap)
try {
    Yuv422Layout L;
    if (int rc = yuv422_head("encode_jpeg_yuv422", format, row_stride, 0, W, H, &L)) return rc;
    if (!pix || !out) return set_err(JPEZY_E_BADARG, "encode_jpeg_yuv422: null pointer");
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    if (int rc = check_comment(comment, "encode_jpeg_yuv422")) return rc;
    if (int rc = check_encode_variant(c, JPEZY_SAMPLING_422, 0, "encode_jpeg_yuv422")) return rc;
    const size_t bytes = (size_t)(H - 1) * L.row_stride + L.row_bytes;
    return jpezy_internal_encode_file(c, { W, H, JPEZY_SAMPLING_422, 0, comment, out, cap, 2,
        [&](const HostChunk&, size_t, std::vector<jpezy_host::Segment>& in) { in.push_back({ const_cast<uint8_t*>(pix), bytes, 0 }); },
        [&](const HostChunk&, size_t, const uint8_t* d_in) { return EncodeSource::yuv422(L, format, d_in); } });
}
JPEZY_CATCH

int jpezy_dequant_idct_generic_yuv422_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                          const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int format,
                                          size_t row_stride, size_t frame_stride, int n_frames, uint8_t* d_pix, void* stream)
{
    Yuv422Layout L;
    if (int rc = yuv422_head("dequant_idct_generic_yuv422_dev", format, row_stride, frame_stride, W, H, &L)) return rc;
    if (int rc = dev_null_check("dequant_idct_generic_yuv422_dev", { d_coeffs, qt, comp_h, comp_v, comp_tq, d_pix })) return rc;
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (int rc = dev_aligned_check(d_coeffs)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_generic_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, 0, n_frames },
                                           DecodeSink::yuv422_packed(d_pix, L.off[0], L.off[1], L.off[2], (unsigned)L.row_stride, L.frame_stride),
                                           (hipStream_t)stream, 0);
}

// .jpg bytes -> macropixels on the host: the header, the coefficients (read_coeffs), the any-layout pair with the packed 4:2:2 second
// stage for EVERY layout -- this project's own 4:2:0 files too: two launches, not the fused kernel's one --, then the rows by a 2-D
// copy, so that only row_bytes of each caller row are written
int jpezy_decode_jpeg_yuv422(jpezy_ctx* c, const uint8_t* data, size_t len, jpezy_frame_info* info, int format, size_t row_stride, uint8_t* pix,
                             size_t pix_cap)
try {
    if (format != JPEZY_YUV_YUY2 && format != JPEZY_YUV_UYVY && format != JPEZY_YUV_YVYU)
        return set_err(JPEZY_E_BADARG, "decode_jpeg_yuv422: format must be JPEZY_YUV_YUY2, JPEZY_YUV_UYVY or JPEZY_YUV_YVYU");
    if (!data || !info) return set_err(JPEZY_E_BADARG, "decode_jpeg_yuv422: null pointer");
    if (!c) return set_err(JPEZY_E_BADARG, "decode_jpeg_yuv422: null context");
    int rc = jpezy_read_jpeg_gpu(c, data, len, info, nullptr, 0);           // header only
    if (rc < 0) return rc;
    if (!pix) return JPEZY_OK;
    const int W = info->width, H = info->height;
    if (int rc2 = jpezy_internal_check_dims(c, W, H, 1)) return rc2;
    if (info->ncomp != 1 && info->ncomp != 3) return set_err(JPEZY_E_UNSUPPORTED, "dimension not supported (the reference accepts 1 or 3)");
    Yuv422Layout L;
    if (int rc2 = yuv422_layout("decode_jpeg_yuv422", format, row_stride, 0, W, H, &L)) return rc2;
    if (pix_cap < (size_t)(H - 1) * L.row_stride + L.row_bytes) return set_err(JPEZY_E_NOSPACE, "decode_jpeg_yuv422: pixel buffer too small");
    if (int rc2 = read_coeffs(c, data, len, info, "decode_jpeg_yuv422")) return rc2;
    if (int rc2 = c->in[0].reserve(L.row_bytes * (size_t)H)) return rc2;
    uint8_t* d = (uint8_t*)c->in[0].p;                                       // tight rows on the device
    if (int rc2 = jpezy_internal_generic_dev_core(c, DecodeSource::file((const int16_t*)c->out.p, *info, 0),
                                                  DecodeSink::yuv422_packed(d, L.off[0], L.off[1], L.off[2], (unsigned)L.row_bytes, L.row_bytes * (size_t)H),
                                                  c->stream, 0))
        return rc2;
    HIP_TRY(hipMemcpy2DAsync(pix, L.row_stride, d, L.row_bytes, L.row_bytes, (size_t)H, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return JPEZY_OK;
}
JPEZY_CATCH

}  // extern "C"
