// jpezy_capi_scaled.hip -- the C-ABI of include/jpezy_hip.h, part 6: reduced-size decode (scale_denom 2, 4, 8).  Header parse and
// Huffman decoding are those of jpezy_decode_jpeg; the transform stage is the pair of jpezy_kernels_scaled.hip for every layout.
// scale_denom 1 is handed to the full-size entry points as it is: no full-size work runs through the kernels of this part.
#include "jpezy_capi_decode.h"

extern "C" {

int jpezy_internal_scaled_dev_core(jpezy_ctx* c, const DecodeSource& src, const DecodeSink& out, hipStream_t s, int log2n)
{
    ScaledDecParams p;
    if (int rc = decode_geometry(c, src, out, &p)) return rc;
    p.log2n = log2n;
    (void)jpezy_scaled_size(src.W, src.H, 8 >> log2n, &p.Ws, &p.Hs);
    const int per = scaled_frames_per_launch(p);             // samples scratch: the frames of one launch (launches run in stream order)
    if (per < 1) return set_err(JPEZY_E_UNSUPPORTED, "scaled decoder: frame of more than 2^31 blocks");
    if (int rc = grow_outside_capture(c->scratch, (geometry_blocks(p) << (2 * log2n)) * sizeof(int) * (size_t)std::min(src.n_frames, per), s,
                                      "scaled decoder"))
        return rc;
    if (int rc = upload_dequant(c, src, s)) return rc;
    p.samples = c->scratch.as<int>();
    HIP_TRY(launch_dequant_idct_scaled(p, s));
    return JPEZY_OK;
}

int jpezy_scaled_size(int W, int H, int scale_denom, int* Ws, int* Hs)
{
    if (log2n_of(scale_denom) < 0) return bad_scale("scaled_size");
    if (W <= 0 || H <= 0) return set_err(JPEZY_E_BADARG, "scaled_size: width and height must be positive");
    const long n = 8 / scale_denom;
    if (Ws) *Ws = (int)(((long)W * n + 7) / 8);
    if (Hs) *Hs = (int)(((long)H * n + 7) / 8);
    return JPEZY_OK;
}

int jpezy_dequant_idct_scaled_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                  const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray, int scale_denom,
                                  int n_frames, size_t plane_stride, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream)
{
    if (scale_denom == 1)       // one frame: the entry without a stride, so that a plane stride of W * H needs no alignment here either
        return n_frames == 1 ? jpezy_dequant_idct_generic_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, d_r, d_g, d_b, stream)
                             : jpezy_dequant_idct_generic_batch_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, n_frames,
                                                                    plane_stride, d_r, d_g, d_b, stream);
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    const int log2n = log2n_of(scale_denom);
    if (log2n < 0) return bad_scale("dequant_idct_scaled_dev");
    if (int rc = dev_null_check(nullptr, { d_coeffs, qt, comp_h, comp_v, comp_tq, d_r, d_g, d_b })) return rc;
    if (int rc = dev_aligned_check(d_coeffs)) return rc;
    int Ws, Hs;
    (void)jpezy_scaled_size(W, H, scale_denom, &Ws, &Hs);
    if (plane_stride < (size_t)Ws * Hs) return set_err(JPEZY_E_BADARG, "dequant_idct_scaled_dev: plane_stride must hold a plane of Ws * Hs bytes");
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_scaled_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames },
                                          DecodeSink::planes(d_r, d_g, d_b, plane_stride), (hipStream_t)stream, log2n);
}

int jpezy_dequant_idct_scaled_packed_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                         const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray,
                                         int scale_denom, int format, size_t row_stride, size_t frame_stride, int n_frames, uint8_t* d_pix,
                                         void* stream)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    const int log2n = log2n_of(scale_denom);
    if (log2n < 0) return bad_scale("dequant_idct_scaled_packed_dev");
    int Ws, Hs;
    (void)jpezy_scaled_size(W, H, scale_denom, &Ws, &Hs);
    PackedLayout L;
    if (int rc = packed_layout("dequant_idct_scaled_packed_dev", format, row_stride, frame_stride, Ws, Hs, &L)) return rc;
    if (int rc = dev_null_check(nullptr, { d_coeffs, qt, comp_h, comp_v, comp_tq, d_pix })) return rc;
    if (int rc = dev_aligned_check(d_coeffs)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const DecodeSource src = { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames };
    if (scale_denom == 1)       // the generic pair's packed store stage, under its own rules (batch form: frame_stride a multiple of 4)
        return jpezy_internal_generic_dev_core(c, src, DecodeSink::packed(L, d_pix), (hipStream_t)stream, 0);
    return jpezy_internal_scaled_dev_core(c, src, DecodeSink::packed(L, d_pix), (hipStream_t)stream, log2n);
}

// .jpg bytes -> reduced planes on the host: jpezy_decode_jpeg's head, the scaled stage, a download of Ws * Hs bytes per plane
int jpezy_decode_jpeg_scaled(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int scale_denom, jpezy_frame_info* info, uint8_t* r,
                             uint8_t* g, uint8_t* b, size_t plane_cap)
try {
    if (scale_denom == 1) return jpezy_decode_jpeg(c, data, len, gray, info, r, g, b, plane_cap);
    if (!c || !info) return set_err(JPEZY_E_BADARG, "decode_jpeg_scaled: bad argument");
    if (log2n_of(scale_denom) < 0) return bad_scale("decode_jpeg_scaled");
    DecodeRequest rq = DecodeRequest::planes("decode_jpeg_scaled", DecodeStage::Scaled, gray, r, g, b, plane_cap);
    rq.scale_denom = scale_denom;
    return jpezy_internal_decode_file(c, data, len, info, rq);
}
JPEZY_CATCH

// the same into host packed pixels: the device image is tight, the caller's rows are row_stride apart
int jpezy_decode_jpeg_scaled_packed(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int scale_denom, jpezy_frame_info* info, int format,
                                    size_t row_stride, uint8_t* pix, size_t pix_cap)
try {
    if (scale_denom == 1) return jpezy_decode_jpeg_packed(c, data, len, gray, info, format, row_stride, pix, pix_cap);
    if (!c || !info) return set_err(JPEZY_E_BADARG, "decode_jpeg_scaled_packed: bad argument");
    if (log2n_of(scale_denom) < 0) return bad_scale("decode_jpeg_scaled_packed");
    if (jpezy_pixel_bytes(format) < 0) return set_err(JPEZY_E_BADARG, "decode_jpeg_scaled_packed: unknown pixel format");
    DecodeRequest rq = DecodeRequest::packed("decode_jpeg_scaled_packed", DecodeStage::Scaled, gray, format, row_stride, pix, pix_cap);
    rq.scale_denom = scale_denom;
    return jpezy_internal_decode_file(c, data, len, info, rq);
}
JPEZY_CATCH

}  // extern "C"
