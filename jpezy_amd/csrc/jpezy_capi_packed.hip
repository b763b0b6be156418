// jpezy_capi_packed.hip -- the C-ABI of include/jpezy_hip.h, part 5: packed (interleaved) RGB / BGR / RGBA / BGRA pixels.  The same
// kernels as the planar entry points with another first (pixel load) and last (pixel store) step; results are the planar ones'.
#include "jpezy_capi_decode.h"

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
    const bool avg = jpezy_internal_averaged_chroma(c, gray);
    if (int rc = jpezy_internal_check_variant_avg(c, avg, "fdct_quant_packed_dev")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    EncParams p;
    p.pix = d_pix;
    p.r = d_pix + L.off[0]; p.g = d_pix + L.off[1]; p.b = d_pix + L.off[2];
    p.plane_stride = L.frame_stride;
    p.row_stride = (unsigned)L.row_stride;
    p.pix_bytes = L.bytes;
    p.swap_rb = L.off[0] != 0;
    if (int rc = jpezy_internal_enc_params(c, W, H, gray, n_frames, d_coeffs, s, &p)) return rc;
    for (int f0 = 0; f0 < n_frames; f0 += kMaxFramesPerLaunch) {
        EncParams q = p;
        q.n_frames = n_frames - f0 < kMaxFramesPerLaunch ? n_frames - f0 : kMaxFramesPerLaunch;
        const size_t adv = (size_t)f0 * L.frame_stride;
        q.pix += adv; q.r += adv; q.g += adv; q.b += adv;
        q.coeffs += (size_t)f0 * p.coeffs_per_frame;
        // variant 0: the FP64 kernel's byte loop; every other variant: the f32 kernel's packed launch (the laboratory's persistent
        // variants 2 and 3 hand packed input to it as they do every frame they do not cover)
        // (JPEZY_DOWNSAMPLE_AVERAGE: the same launch with the averaged chroma stage; variant 0 was refused above)
        if (avg)
            HIP_TRY(launch_fdct_quant_f32_packed_avg(q, c->force_exact, s));
        else if (c->variant == 0)
            HIP_TRY(launch_fdct_quant_packed(q, gray != 0, c->force_exact != 0, s));
        else
            HIP_TRY(launch_fdct_quant_f32_packed(q, gray != 0, c->force_exact, s));
    }
    return JPEZY_OK;
}

int jpezy_dequant_idct_packed_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], const uint8_t comp_tq[3], int format,
                                  size_t row_stride, size_t frame_stride, int W, int H, int gray, int n_frames, uint8_t* d_pix, void* stream)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    PackedLayout L;
    if (int rc = packed_layout("dequant_idct_packed_dev", format, row_stride, frame_stride, W, H, &L)) return rc;
    if (!d_coeffs || !qt || !comp_tq || !d_pix) return set_err(JPEZY_E_BADARG, "null pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = jpezy_internal_upload_dequant(c, qt, comp_tq, s)) return rc;
    DecParams p;
    p.pix = d_pix;
    p.r = d_pix + L.off[0]; p.g = d_pix + L.off[1]; p.b = d_pix + L.off[2];
    p.plane_stride = L.frame_stride;
    p.row_stride = (unsigned)L.row_stride;
    p.pix_bytes = L.bytes;
    p.swap_rb = L.off[0] != 0;
    jpezy_internal_dec_params(c, d_coeffs, W, H, n_frames, &p);
    for (int f0 = 0; f0 < n_frames; f0 += kMaxFramesPerLaunch) {
        DecParams q = p;
        q.n_frames = n_frames - f0 < kMaxFramesPerLaunch ? n_frames - f0 : kMaxFramesPerLaunch;
        q.coeffs += (size_t)f0 * p.coeffs_per_frame;
        const size_t adv = (size_t)f0 * L.frame_stride;
        q.pix += adv; q.r += adv; q.g += adv; q.b += adv;
        HIP_TRY(launch_dequant_idct_packed(q, gray != 0, c->force_exact != 0, c->dec_tolerance != 0, s));
    }
    return JPEZY_OK;
}

// packed pixels on the host -> .jpg bytes on the host: jpezy_encode_jpeg with one input segment per band instead of three
long jpezy_encode_jpeg_packed(jpezy_ctx* c, const uint8_t* pix, int format, size_t row_stride, int W, int H, int gray, const char* comment,
                              uint8_t* out, size_t cap)
try {
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    PackedLayout L;
    if (int rc = packed_layout("encode_jpeg_packed", format, row_stride, 0, W, H, &L)) return rc;
    if (!pix || !out) return set_err(JPEZY_E_BADARG, "encode_jpeg_packed: null pointer");
    if (int rc = check_comment(comment, "encode_jpeg_packed")) return rc;
    if (int rc = jpezy_internal_check_variant_avg(c, jpezy_internal_averaged_chroma(c, gray), "encode_jpeg_packed")) return rc;   // before anything is uploaded
    HIP_TRY(hipSetDevice(c->device));
    const int B = gray ? 4 : 6;
    if (int rc = c->e_coef.reserve(jpezy_coeff_count(W, H, gray) * sizeof(int16_t))) return rc;
    const std::vector<HostChunk> chunks = plan_host_chunks(W, H, 1, (size_t)L.bytes, c->host_chunk_bytes);
    const size_t tight = (size_t)W * L.bytes;
    // a band goes up as it lies in the caller's buffer, row padding included, up to the last byte of its last row
    auto band_bytes = [&](const HostChunk& k) { return (size_t)(k.rows(H) - 1) * L.row_stride + tight; };
    size_t max_in = 0;
    for (const HostChunk& k : chunks) max_in = std::max(max_in, band_bytes(k));
    int rc_kernel = JPEZY_OK;
    std::string err;
    auto plan = [&](int i) {
        const HostChunk& k = chunks[(size_t)i];
        jpezy_host::ChunkPlan p;
        p.in.push_back({ const_cast<uint8_t*>(pix) + (size_t)k.y0 * 16 * L.row_stride, band_bytes(k), 0 });
        return p;
    };
    auto kernel = [&](int i, uint8_t* d_in, uint8_t*, hipStream_t s) -> hipError_t {
        const HostChunk& k = chunks[(size_t)i];
        const int rc = jpezy_fdct_quant_packed_dev(c, d_in, format, L.row_stride, 0, W, k.rows(H), gray, 1,
                                                   c->e_coef.as<int16_t>() + k.coef_off(W, H, B), s);
        if (rc != JPEZY_OK) { rc_kernel = rc; return hipErrorLaunchFailure; }
        return hipSuccess;
    };
    const hipError_t e = c->pipe.run(c->device, c->stream, (int)chunks.size(), max_in, 0, plan, kernel, &err);
    if (rc_kernel != JPEZY_OK) return rc_kernel;
    if (e != hipSuccess) return set_err(JPEZY_E_HIP, err.empty() ? std::string("host pipeline: ") + hipGetErrorString(e) : err);
    return jpezy_write_jpeg_gpu(c, (const int16_t*)c->e_coef.p, W, H, gray, comment, out, cap);
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
