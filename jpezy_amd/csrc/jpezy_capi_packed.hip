// jpezy_capi_packed.hip -- the C-ABI of include/jpezy_hip.h, part 5: packed (interleaved) RGB / BGR / RGBA / BGRA pixels.  The same
// kernels as the planar entry points with another first (pixel load) and last (pixel store) step; results are the planar ones'.  The
// entries check their arguments and describe the buffer (EncodeSource::packed, DecodeSink::packed, packed_encode_request); the work is
// the cores' and the drivers' (jpezy_capi_encode.h, jpezy_capi_decode.h).
#include "jpezy_capi_decode.h"
#include "jpezy_capi_encode.h"

namespace jpezy_capi {

// What a file encode from packed pixels hands the driver: one input segment per band, which goes up as it lies in the caller's buffer,
// row padding included, up to the last byte of its last row.  For jpezy_encode_jpeg_packed and jpezy_encode_jpeg_sampling_packed.
EncodeRequest packed_encode_request(const uint8_t* pix, const PackedLayout& L, int W, int H, int sampling, int gray, const char* comment,
                                                uint8_t* out, size_t cap)
{
    return { W, H, sampling, gray, comment, out, cap, (size_t)L.bytes,
             [=](const HostChunk& k, size_t, std::vector<jpezy_host::Segment>& in) {
                 in.push_back({ const_cast<uint8_t*>(pix) + (size_t)k.y0 * 16 * L.row_stride, (size_t)(k.rows(H) - 1) * L.row_stride + (size_t)W * L.bytes, 0 });
             },
             [=](const HostChunk& k, size_t, const uint8_t* d_in) {
                 PackedLayout band = L;
                 band.frame_stride = (size_t)k.rows(H) * L.row_stride;          // the tight frame stride of the band's rows
                 return EncodeSource::packed(band, d_in);
             } };
}

}  // namespace jpezy_capi

extern "C" {

int jpezy_pixel_bytes(int format)
{
    switch (format) {
    case JPEZY_PIX_RGB24: case JPEZY_PIX_BGR24: return 3;
    case JPEZY_PIX_RGBA32: case JPEZY_PIX_BGRA32: return 4;
    default: return JPEZY_E_BADARG;
    }
}

int jpezy_fdct_quant_packed_dev(jpezy_ctx* c, const uint8_t* d_pix, int format, size_t row_stride, size_t frame_stride, int W, int H,
                                int gray, int n_frames, int16_t* d_coeffs, void* stream)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    PackedLayout L;
    if (int rc = packed_layout("fdct_quant_packed_dev", format, row_stride, frame_stride, W, H, &L)) return rc;
    if (!d_pix || !d_coeffs) return set_err(JPEZY_E_BADARG, "null device pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    if (int rc = check_encode_variant(c, JPEZY_SAMPLING_420, gray, "fdct_quant_packed_dev")) return rc;
    return jpezy_internal_fdct_quant_core(c, EncodeSource::packed(L, d_pix), JPEZY_SAMPLING_420, W, H, gray, n_frames, d_coeffs, (hipStream_t)stream);
}

int jpezy_dequant_idct_packed_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], const uint8_t comp_tq[3], int format,
                                  size_t row_stride, size_t frame_stride, int W, int H, int gray, int n_frames, uint8_t* d_pix, void* stream)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    PackedLayout L;
    if (int rc = packed_layout("dequant_idct_packed_dev", format, row_stride, frame_stride, W, H, &L)) return rc;
    if (!d_coeffs || !qt || !comp_tq || !d_pix) return set_err(JPEZY_E_BADARG, "null pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    return jpezy_internal_fused_dev_core(c, d_coeffs, qt, comp_tq, DecodeSink::packed(L, d_pix), W, H, gray, n_frames, (hipStream_t)stream);
}

// packed pixels on the host -> .jpg bytes on the host
long jpezy_encode_jpeg_packed(jpezy_ctx* c, const uint8_t* pix, int format, size_t row_stride, int W, int H, int gray, const char* comment,
                              uint8_t* out, size_t cap)
try {
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    PackedLayout L;
    if (int rc = packed_layout("encode_jpeg_packed", format, row_stride, 0, W, H, &L)) return rc;
    if (!pix || !out) return set_err(JPEZY_E_BADARG, "encode_jpeg_packed: null pointer");
    if (int rc = check_comment(comment, "encode_jpeg_packed")) return rc;
    if (int rc = check_encode_variant(c, JPEZY_SAMPLING_420, gray, "encode_jpeg_packed")) return rc;   // before anything is uploaded
    return jpezy_internal_encode_file(c, packed_encode_request(pix, L, W, H, JPEZY_SAMPLING_420, gray, comment, out, cap));
}
JPEZY_CATCH

// .jpg bytes -> packed pixels on the host: jpezy_decode_jpeg with the packed store stage of the fused kernel (jpezy's own layout) or
// of the generic pair (every other layout); the device image is tight, the caller's rows are row_stride apart
int jpezy_decode_jpeg_packed(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, jpezy_frame_info* info, int format, size_t row_stride,
                             uint8_t* pix, size_t pix_cap)
try {
    if (!c || !info) return set_err(JPEZY_E_BADARG, "decode_jpeg_packed: bad argument");
    if (jpezy_pixel_bytes(format) < 0) return set_err(JPEZY_E_BADARG, "decode_jpeg_packed: unknown pixel format");
    return jpezy_internal_decode_file(c, data, len, info, DecodeRequest::packed("decode_jpeg_packed", DecodeStage::Full, gray, format, row_stride, pix, pix_cap));
}
JPEZY_CATCH

}  // extern "C"
