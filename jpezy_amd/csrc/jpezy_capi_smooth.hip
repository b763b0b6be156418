// jpezy_capi_smooth.hip -- the C-ABI of include/jpezy_hip.h, part 11: chroma upsampling as an argument of the decoder's entries.
// JPEZY_UPSAMPLE_NEAREST is handed to the existing entry points as it is; JPEZY_UPSAMPLE_SMOOTH takes the any-layout pair for every
// layout, jpezy's own included, with smooth_rgb_kernel (jpezy_kernels_smooth.hip) as the second stage.  Header parse and Huffman
// decoding are those of jpezy_decode_jpeg.
#include "jpezy_capi_decode.h"

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
    if (int rc = dev_head(c, W, H, n_frames, { d_coeffs, qt, comp_h, comp_v, comp_tq, d_r, d_g, d_b }, d_coeffs)) return rc;
    if (n_frames > 1 && (plane_stride < (size_t)W * H || (plane_stride & 3)))
        return set_err(JPEZY_E_BADARG, "dequant_idct_upsampling_dev: plane_stride must hold a plane and be a multiple of 4");
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_generic_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames },
                                           DecodeSink::planes(d_r, d_g, d_b, n_frames > 1 ? plane_stride : 0), (hipStream_t)stream, mode);
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
    if (int rc = dev_null_check(nullptr, { d_coeffs, qt, comp_h, comp_v, comp_tq, d_pix })) return rc;
    if (int rc = dev_aligned_check(d_coeffs)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // nearest: the generic pair's packed store stage, as jpezy_dequant_idct_scaled_packed_dev reaches it at scale_denom 1
    return jpezy_internal_generic_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames },
                                           DecodeSink::packed(L, d_pix), (hipStream_t)stream, mode);
}

// .jpg bytes -> planes on the host: jpezy_decode_jpeg's head, the two stages, a download of W * H bytes per plane
int jpezy_decode_jpeg_upsampling(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int upsampling, jpezy_frame_info* info, uint8_t* r,
                                 uint8_t* g, uint8_t* b, size_t plane_cap)
try {
    if (upsampling == JPEZY_UPSAMPLE_NEAREST) return jpezy_decode_jpeg(c, data, len, gray, info, r, g, b, plane_cap);
    if (int mode = upsampling_mode("decode_jpeg_upsampling", upsampling, 8); mode < 0) return mode;
    if (!c || !info) return set_err(JPEZY_E_BADARG, "decode_jpeg_upsampling: bad argument");
    return jpezy_internal_decode_file(c, data, len, info, DecodeRequest::planes("decode_jpeg_upsampling", DecodeStage::Smooth, gray, r, g, b, plane_cap));
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
    return jpezy_internal_decode_file(c, data, len, info,
                                      DecodeRequest::packed("decode_jpeg_upsampling_packed", DecodeStage::Smooth, gray, format, row_stride, pix, pix_cap));
}
JPEZY_CATCH

}  // extern "C"
