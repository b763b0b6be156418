// jpezy_capi_scaled.hip -- the C-ABI of include/jpezy_hip.h, part 6: reduced-size decode (scale_denom 2, 4, 8).  Header parse and
// Huffman decoding are those of jpezy_decode_jpeg; the transform stage is the pair of jpezy_kernels_scaled.hip for every layout.
// scale_denom 1 is handed to the full-size entry points as it is: no full-size work runs through the kernels of this part.
#include "jpezy_capi_internal.h"

namespace {

// 8 / scale_denom as a shift: 2, 1, 0 for the denominators 2, 4, 8; -1 for anything else (1 included: it never gets here)
int log2n_of(int scale_denom) { return scale_denom == 2 ? 2 : scale_denom == 4 ? 1 : scale_denom == 8 ? 0 : -1; }

int bad_scale(const char* who) { return set_err(JPEZY_E_BADARG, std::string(who) + ": scale_denom must be 1, 2, 4 or 8"); }

// geometry + tables + the two launches on device memory; asynchronous on stream s (the tables are uploaded synchronously when they
// changed since the last call).  d_r, d_g, d_b: planes, or with pix_bytes != 0 the channel bytes of pixel (0, 0).
int scaled_dev_core(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3], const uint8_t comp_v[3],
                    const uint8_t comp_tq[3], int precision, int W, int H, int gray, int log2n, int n_frames, size_t plane_stride, int pix_bytes,
                    unsigned row_stride, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, hipStream_t s)
{
    if (ncomp != 1 && ncomp != 3) return set_err(JPEZY_E_UNSUPPORTED, "dimension not supported (the reference accepts 1 or 3)");
    ScaledDecParams p;
    p.log2n = log2n;
    p.ncomp = ncomp; p.gray = gray != 0;
    p.level = precision == 8 ? 128 : 2048;                    // ref :654
    p.hmax = p.vmax = 0;
    p.blocks_per_mcu = 0;
    for (int k = 0; k < 3; ++k) { p.ch[k] = p.cv[k] = 1; p.blk_start[k] = 1 << 20; }
    for (int k = 0; k < ncomp; ++k) {
        p.ch[k] = comp_h[k]; p.cv[k] = comp_v[k];
        if (p.ch[k] < 1 || p.ch[k] > 4 || p.cv[k] < 1 || p.cv[k] > 4)
            return set_err(JPEZY_E_UNSUPPORTED, "sampling factors outside 1..4 (ITU-T T.81 B.2.2)");
        p.hmax = p.ch[k] > p.hmax ? p.ch[k] : p.hmax;
        p.vmax = p.cv[k] > p.vmax ? p.cv[k] : p.vmax;
        p.blk_start[k] = p.blocks_per_mcu;
        p.blocks_per_mcu += p.ch[k] * p.cv[k];
    }
    const int Hblock = (W >> 3) + ((W & 7) > 0), Vblock = (H >> 3) + ((H & 7) > 0);   // get_blocks, ref :166-169
    p.mcu_cols = Hblock / p.hmax + ((Hblock % p.hmax) ? 1 : 0);
    p.mcu_rows = Vblock / p.vmax + ((Vblock % p.vmax) ? 1 : 0);
    (void)jpezy_scaled_size(W, H, 8 >> log2n, &p.Ws, &p.Hs);
    const size_t nblk = (size_t)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu;
    p.n_frames = n_frames;
    p.plane_stride = plane_stride;
    p.pix_bytes = pix_bytes;
    p.row_stride = row_stride;
    const int per = scaled_frames_per_launch(p);             // samples scratch: the frames of one launch (launches run in stream order)
    if (per < 1) return set_err(JPEZY_E_UNSUPPORTED, "scaled decoder: frame of more than 2^31 blocks");
    if (int rc = c->scratch.reserve((nblk << (2 * log2n)) * sizeof(int) * (size_t)std::min(n_frames, per))) return rc;
    const uint8_t tq3[3] = { comp_tq[0], (uint8_t)(ncomp > 1 ? comp_tq[1] : 0), (uint8_t)(ncomp > 2 ? comp_tq[2] : 0) };
    if (int rc = jpezy_internal_upload_dequant(c, qt, tq3, s)) return rc;
    p.coeffs = d_coeffs;
    p.samples = c->scratch.as<int>();
    p.qt = c->d_dqt.as<int>();
    p.r = d_r; p.g = d_g; p.b = d_b;
    HIP_TRY(launch_dequant_idct_scaled(p, s));
    return JPEZY_OK;
}

}  // namespace

extern "C" {

int jpezy_scaled_size(int W, int H, int scale_denom, int* Ws, int* Hs)
{
    if (scale_denom != 1 && log2n_of(scale_denom) < 0) return bad_scale("scaled_size");
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
    if (!d_coeffs || !qt || !comp_h || !comp_v || !comp_tq || !d_r || !d_g || !d_b) return set_err(JPEZY_E_BADARG, "null pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    int Ws, Hs;
    (void)jpezy_scaled_size(W, H, scale_denom, &Ws, &Hs);
    if (plane_stride < (size_t)Ws * Hs) return set_err(JPEZY_E_BADARG, "dequant_idct_scaled_dev: plane_stride must hold a plane of Ws * Hs bytes");
    HIP_TRY(hipSetDevice(c->device));
    return scaled_dev_core(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, log2n, n_frames, plane_stride, 0, 0, d_r, d_g,
                           d_b, (hipStream_t)stream);
}

int jpezy_dequant_idct_scaled_packed_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                         const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray,
                                         int scale_denom, int format, size_t row_stride, size_t frame_stride, int n_frames, uint8_t* d_pix,
                                         void* stream)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (scale_denom != 1 && log2n_of(scale_denom) < 0) return bad_scale("dequant_idct_scaled_packed_dev");
    int Ws, Hs;
    (void)jpezy_scaled_size(W, H, scale_denom, &Ws, &Hs);
    PackedLayout L;
    if (int rc = packed_layout("dequant_idct_scaled_packed_dev", format, row_stride, frame_stride, Ws, Hs, &L)) return rc;
    if (!d_coeffs || !qt || !comp_h || !comp_v || !comp_tq || !d_pix) return set_err(JPEZY_E_BADARG, "null pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    if (scale_denom == 1)       // the generic pair's packed store stage, under its own rules (batch form: frame_stride a multiple of 4)
        return jpezy_internal_generic_dev_core(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, W, H, gray, precision, d_pix + L.off[0],
                                               d_pix + L.off[1], d_pix + L.off[2], (hipStream_t)stream, nullptr, n_frames, L.frame_stride, L.bytes,
                                               (unsigned)L.row_stride);
    return scaled_dev_core(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, log2n_of(scale_denom), n_frames, L.frame_stride,
                           L.bytes, (unsigned)L.row_stride, d_pix + L.off[0], d_pix + L.off[1], d_pix + L.off[2], (hipStream_t)stream);
}

// .jpg bytes -> reduced planes on the host: jpezy_decode_jpeg's head, the scaled stage, a download of Ws * Hs bytes per plane
int jpezy_decode_jpeg_scaled(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int scale_denom, jpezy_frame_info* info, uint8_t* r,
                             uint8_t* g, uint8_t* b, size_t plane_cap)
try {
    if (scale_denom == 1) return jpezy_decode_jpeg(c, data, len, gray, info, r, g, b, plane_cap);
    if (!c || !info) return set_err(JPEZY_E_BADARG, "decode_jpeg_scaled: bad argument");
    const int log2n = log2n_of(scale_denom);
    if (log2n < 0) return bad_scale("decode_jpeg_scaled");
    int rc = jpezy_read_jpeg_gpu(c, data, len, info, nullptr, 0);           // header only
    if (rc < 0) return rc;
    if (!r || !g || !b) return JPEZY_OK;
    const int W = info->width, H = info->height;
    if (int rc2 = jpezy_internal_check_dims(c, W, H, 1)) return rc2;
    int Ws, Hs;
    (void)jpezy_scaled_size(W, H, scale_denom, &Ws, &Hs);
    const size_t plane = (size_t)Ws * Hs;
    if (plane_cap < plane) return set_err(JPEZY_E_NOSPACE, "decode_jpeg_scaled: plane buffers too small");
    if (int rc2 = read_coeffs(c, data, len, info, "decode_jpeg_scaled")) return rc2;
    for (int k = 0; k < 3; ++k)
        if (int rc2 = c->in[k].reserve(plane)) return rc2;
    const Layout l(*info);
    if (int rc2 = scaled_dev_core(c, (const int16_t*)c->out.p, info->qt, info->ncomp, l.hs, l.vs, l.tq, info->precision, W, H, gray, log2n, 1, plane,
                                  0, 0, (uint8_t*)c->in[0].p, (uint8_t*)c->in[1].p, (uint8_t*)c->in[2].p, c->stream))
        return rc2;
    uint8_t* dst[3] = { r, g, b };
    for (int k = 0; k < 3; ++k) HIP_TRY(hipMemcpyAsync(dst[k], c->in[k].p, plane, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return JPEZY_OK;
}
JPEZY_CATCH

// the same into host packed pixels: the device image is tight, the caller's rows are row_stride apart
int jpezy_decode_jpeg_scaled_packed(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int scale_denom, jpezy_frame_info* info, int format,
                                    size_t row_stride, uint8_t* pix, size_t pix_cap)
try {
    if (scale_denom == 1) return jpezy_decode_jpeg_packed(c, data, len, gray, info, format, row_stride, pix, pix_cap);
    if (!c || !info) return set_err(JPEZY_E_BADARG, "decode_jpeg_scaled_packed: bad argument");
    const int log2n = log2n_of(scale_denom);
    if (log2n < 0) return bad_scale("decode_jpeg_scaled_packed");
    if (jpezy_pixel_bytes(format) < 0) return set_err(JPEZY_E_BADARG, "decode_jpeg_scaled_packed: unknown pixel format");
    int rc = jpezy_read_jpeg_gpu(c, data, len, info, nullptr, 0);           // header only
    if (rc < 0) return rc;
    if (!pix) return JPEZY_OK;
    const int W = info->width, H = info->height;
    if (int rc2 = jpezy_internal_check_dims(c, W, H, 1)) return rc2;
    int Ws, Hs;
    (void)jpezy_scaled_size(W, H, scale_denom, &Ws, &Hs);
    PackedLayout L;
    if (int rc2 = packed_layout("decode_jpeg_scaled_packed", format, row_stride, 0, Ws, Hs, &L)) return rc2;
    const size_t tight = (size_t)Ws * L.bytes;
    if (pix_cap < (size_t)(Hs - 1) * L.row_stride + tight) return set_err(JPEZY_E_NOSPACE, "decode_jpeg_scaled_packed: pixel buffer too small");
    if (tight * (size_t)Hs > 0xFFFFFFFFull) return set_err(JPEZY_E_BADARG, "decode_jpeg_scaled_packed: image of more than 2^32 bytes");
    if (int rc2 = read_coeffs(c, data, len, info, "decode_jpeg_scaled_packed")) return rc2;
    if (int rc2 = c->in[0].reserve(tight * (size_t)Hs)) return rc2;
    uint8_t* d_pix = (uint8_t*)c->in[0].p;
    const Layout l(*info);
    if (int rc2 = scaled_dev_core(c, (const int16_t*)c->out.p, info->qt, info->ncomp, l.hs, l.vs, l.tq, info->precision, W, H, gray, log2n, 1, 0,
                                  L.bytes, (unsigned)tight, d_pix + L.off[0], d_pix + L.off[1], d_pix + L.off[2], c->stream))
        return rc2;
    if (L.row_stride == tight)
        HIP_TRY(hipMemcpyAsync(pix, d_pix, tight * (size_t)Hs, hipMemcpyDeviceToHost, c->stream));
    else      // only bytes [0, Ws * bytes) of each of the caller's rows are written
        HIP_TRY(hipMemcpy2DAsync(pix, L.row_stride, d_pix, tight, tight, (size_t)Hs, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return JPEZY_OK;
}
JPEZY_CATCH

}  // extern "C"
