// jpezy_capi_smooth.hip -- the C-ABI of include/jpezy_hip.h, part 11: chroma upsampling as an argument of the decoder's entries.
// JPEZY_UPSAMPLE_NEAREST is handed to the existing entry points as it is; JPEZY_UPSAMPLE_SMOOTH takes the any-layout pair for every
// layout, jpezy's own included, with smooth_rgb_kernel (jpezy_kernels_smooth.hip) as the second stage.  Header parse and Huffman
// decoding are those of jpezy_decode_jpeg.
#include "jpezy_capi_internal.h"

namespace {

// 0: nearest (forward to the existing entry), 1: smooth, negative: the status to return
int upsampling_mode(const char* who, int upsampling, int precision)
{
    if (upsampling == JPEZY_UPSAMPLE_NEAREST) return 0;
    if (upsampling != JPEZY_UPSAMPLE_SMOOTH)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": upsampling must be JPEZY_UPSAMPLE_NEAREST or JPEZY_UPSAMPLE_SMOOTH");
    if (precision != 8)
        return set_err(JPEZY_E_UNSUPPORTED, std::string(who) + ": JPEZY_UPSAMPLE_SMOOTH is defined for 8-bit files only");
    return 1;
}

}  // namespace

extern "C" {

int jpezy_dequant_idct_upsampling_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                      const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray, int upsampling,
                                      int n_frames, size_t plane_stride, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream)
{
    const int mode = upsampling_mode("dequant_idct_upsampling_dev", upsampling, precision);
    if (mode < 0) return mode;
    if (mode == 0)              // one frame: the entry without a stride, as jpezy_dequant_idct_scaled_dev does at scale_denom 1
        return n_frames == 1 ? jpezy_dequant_idct_generic_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, d_r, d_g, d_b, stream)
                             : jpezy_dequant_idct_generic_batch_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, n_frames,
                                                                    plane_stride, d_r, d_g, d_b, stream);
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!d_coeffs || !qt || !comp_h || !comp_v || !comp_tq || !d_r || !d_g || !d_b) return set_err(JPEZY_E_BADARG, "null pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    if (n_frames > 1 && (plane_stride < (size_t)W * H || (plane_stride & 3)))
        return set_err(JPEZY_E_BADARG, "dequant_idct_upsampling_dev: plane_stride must hold a plane and be a multiple of 4");
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_generic_dev_core(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, W, H, gray, precision, d_r, d_g, d_b, (hipStream_t)stream,
                                           nullptr, n_frames, n_frames > 1 ? plane_stride : 0, 0, 0, 0, 0, 1);
}

int jpezy_dequant_idct_upsampling_packed_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                             const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray,
                                             int upsampling, int format, size_t row_stride, size_t frame_stride, int n_frames, uint8_t* d_pix,
                                             void* stream)
{
    const int mode = upsampling_mode("dequant_idct_upsampling_packed_dev", upsampling, precision);
    if (mode < 0) return mode;
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    PackedLayout L;
    if (int rc = packed_layout("dequant_idct_upsampling_packed_dev", format, row_stride, frame_stride, W, H, &L)) return rc;
    if (!d_coeffs || !qt || !comp_h || !comp_v || !comp_tq || !d_pix) return set_err(JPEZY_E_BADARG, "null pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    // nearest: the generic pair's packed store stage, as jpezy_dequant_idct_scaled_packed_dev reaches it at scale_denom 1
    return jpezy_internal_generic_dev_core(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, W, H, gray, precision, d_pix + L.off[0], d_pix + L.off[1],
                                           d_pix + L.off[2], (hipStream_t)stream, nullptr, n_frames, L.frame_stride, L.bytes, (unsigned)L.row_stride, 0,
                                           0, mode);
}

// .jpg bytes -> planes on the host: jpezy_decode_jpeg's head, the two stages, a download of W * H bytes per plane
int jpezy_decode_jpeg_upsampling(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int upsampling, jpezy_frame_info* info, uint8_t* r,
                                 uint8_t* g, uint8_t* b, size_t plane_cap)
try {
    if (upsampling == JPEZY_UPSAMPLE_NEAREST) return jpezy_decode_jpeg(c, data, len, gray, info, r, g, b, plane_cap);
    if (int mode = upsampling_mode("decode_jpeg_upsampling", upsampling, 8); mode < 0) return mode;
    if (!c || !info) return set_err(JPEZY_E_BADARG, "decode_jpeg_upsampling: bad argument");
    int rc = jpezy_read_jpeg_gpu(c, data, len, info, nullptr, 0);           // header only
    if (rc < 0) return rc;
    if (int mode = upsampling_mode("decode_jpeg_upsampling", upsampling, info->precision); mode < 0) return mode;
    if (!r || !g || !b) return JPEZY_OK;
    const int W = info->width, H = info->height;
    if (int rc2 = jpezy_internal_check_dims(c, W, H, 1)) return rc2;
    const size_t plane = (size_t)W * H;
    if (plane_cap < plane) return set_err(JPEZY_E_NOSPACE, "decode_jpeg_upsampling: plane buffers too small");
    if (int rc2 = read_coeffs(c, data, len, info, "decode_jpeg_upsampling")) return rc2;
    for (int k = 0; k < 3; ++k)
        if (int rc2 = c->in[k].reserve(plane)) return rc2;
    const Layout l(*info);
    if (int rc2 = jpezy_internal_generic_dev_core(c, (const int16_t*)c->out.p, info->qt, info->ncomp, l.hs, l.vs, l.tq, W, H, gray, info->precision,
                                                  (uint8_t*)c->in[0].p, (uint8_t*)c->in[1].p, (uint8_t*)c->in[2].p, c->stream, nullptr, 1, 0, 0, 0, 0,
                                                  0, 1))
        return rc2;
    uint8_t* dst[3] = { r, g, b };
    for (int k = 0; k < 3; ++k) HIP_TRY(hipMemcpyAsync(dst[k], c->in[k].p, plane, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return JPEZY_OK;
}
JPEZY_CATCH

// the same into host packed pixels: the device image is tight, the caller's rows are row_stride apart
int jpezy_decode_jpeg_upsampling_packed(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int upsampling, jpezy_frame_info* info,
                                        int format, size_t row_stride, uint8_t* pix, size_t pix_cap)
try {
    if (upsampling == JPEZY_UPSAMPLE_NEAREST) return jpezy_decode_jpeg_packed(c, data, len, gray, info, format, row_stride, pix, pix_cap);
    if (int mode = upsampling_mode("decode_jpeg_upsampling_packed", upsampling, 8); mode < 0) return mode;
    if (!c || !info) return set_err(JPEZY_E_BADARG, "decode_jpeg_upsampling_packed: bad argument");
    if (jpezy_pixel_bytes(format) < 0) return set_err(JPEZY_E_BADARG, "decode_jpeg_upsampling_packed: unknown pixel format");
    int rc = jpezy_read_jpeg_gpu(c, data, len, info, nullptr, 0);           // header only
    if (rc < 0) return rc;
    if (int mode = upsampling_mode("decode_jpeg_upsampling_packed", upsampling, info->precision); mode < 0) return mode;
    if (!pix) return JPEZY_OK;
    const int W = info->width, H = info->height;
    if (int rc2 = jpezy_internal_check_dims(c, W, H, 1)) return rc2;
    PackedLayout L;
    if (int rc2 = packed_layout("decode_jpeg_upsampling_packed", format, row_stride, 0, W, H, &L)) return rc2;
    const size_t tight = (size_t)W * L.bytes;
    if (pix_cap < (size_t)(H - 1) * L.row_stride + tight) return set_err(JPEZY_E_NOSPACE, "decode_jpeg_upsampling_packed: pixel buffer too small");
    if (tight * (size_t)H > 0xFFFFFFFFull) return set_err(JPEZY_E_BADARG, "decode_jpeg_upsampling_packed: image of more than 2^32 bytes");
    if (int rc2 = read_coeffs(c, data, len, info, "decode_jpeg_upsampling_packed")) return rc2;
    if (int rc2 = c->in[0].reserve(tight * (size_t)H)) return rc2;
    uint8_t* d_pix = (uint8_t*)c->in[0].p;
    const Layout l(*info);
    if (int rc2 = jpezy_internal_generic_dev_core(c, (const int16_t*)c->out.p, info->qt, info->ncomp, l.hs, l.vs, l.tq, W, H, gray, info->precision,
                                                  d_pix + L.off[0], d_pix + L.off[1], d_pix + L.off[2], c->stream, nullptr, 1, 0, L.bytes,
                                                  (unsigned)tight, 0, 0, 1))
        return rc2;
    if (L.row_stride == tight)
        HIP_TRY(hipMemcpyAsync(pix, d_pix, tight * (size_t)H, hipMemcpyDeviceToHost, c->stream));
    else      // only bytes [0, W * bytes) of each of the caller's rows are written
        HIP_TRY(hipMemcpy2DAsync(pix, L.row_stride, d_pix, tight, tight, (size_t)H, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return JPEZY_OK;
}
JPEZY_CATCH

}  // extern "C"
