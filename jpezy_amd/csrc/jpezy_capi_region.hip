// jpezy_capi_region.hip -- the C-ABI of include/jpezy_hip.h, part 8: region-of-interest decode (a window of the picture at scale_denom 1,
// 2, 4, 8).  Header parse and Huffman decoding are those of jpezy_decode_jpeg -- the whole scan is decoded, the coefficient buffer stays
// full size --; the transform, colour and store stage is the one kernel of jpezy_kernels_region.hip over the MCUs that intersect the
// window, and only the window is downloaded.  A window that is the whole picture is handed to the reduced-size entry points as it is.
#include "jpezy_capi_internal.h"

namespace {

// 8 / scale_denom as a shift: 3, 2, 1, 0 for the denominators 1, 2, 4, 8; -1 for anything else
int log2n_of(int scale_denom) { return scale_denom == 1 ? 3 : scale_denom == 2 ? 2 : scale_denom == 4 ? 1 : scale_denom == 8 ? 0 : -1; }

int bad_scale(const char* who) { return set_err(JPEZY_E_BADARG, std::string(who) + ": scale_denom must be 1, 2, 4 or 8"); }

std::string region_text(const jpezy_rect& r)
{
    return std::to_string(r.w) + "x" + std::to_string(r.h) + "+" + std::to_string(r.x) + "+" + std::to_string(r.y);
}

// what a region must satisfy whatever the picture is
int region_syntax(const char* who, const jpezy_rect* r)
{
    if (!r) return set_err(JPEZY_E_BADARG, std::string(who) + ": null region");
    if (r->w < 1 || r->h < 1 || r->x < 0 || r->y < 0)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": region " + region_text(*r) + " (w x h + x + y) needs w, h >= 1 and x, y >= 0");
    return JPEZY_OK;
}

// ... and inside a W x H file decoded at 1 / scale_denom (both already checked): no silent clipping
int region_inside(const char* who, int W, int H, int scale_denom, const jpezy_rect* r)
{
    if (int rc = region_syntax(who, r)) return rc;
    int Ws, Hs;
    (void)jpezy_scaled_size(W, H, scale_denom, &Ws, &Hs);
    if ((long)r->x + r->w > Ws || (long)r->y + r->h > Hs)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": region " + region_text(*r) + " (w x h + x + y) lies outside the picture of " +
                                           std::to_string(Ws) + " x " + std::to_string(Hs) + " at scale_denom " + std::to_string(scale_denom));
    return JPEZY_OK;
}

bool whole_picture(int W, int H, int scale_denom, const jpezy_rect& r)
{
    int Ws, Hs;
    (void)jpezy_scaled_size(W, H, scale_denom, &Ws, &Hs);
    return r.x == 0 && r.y == 0 && r.w == Ws && r.h == Hs;
}

// geometry + tables + the launch on device memory; asynchronous on stream s (the tables are uploaded synchronously when they changed since
// the last call).  d_r, d_g, d_b: the window's planes, or with pix_bytes != 0 the channel bytes of its first pixel.  The region is inside.
int region_dev_core(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3], const uint8_t comp_v[3],
                    const uint8_t comp_tq[3], int precision, int W, int H, int gray, int log2n, const jpezy_rect& rg, int n_frames,
                    size_t plane_stride, int pix_bytes, unsigned row_stride, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, hipStream_t s)
{
    if (ncomp != 1 && ncomp != 3) return set_err(JPEZY_E_UNSUPPORTED, "dimension not supported (the reference accepts 1 or 3)");
    RegionDecParams p;
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
    p.x = rg.x; p.y = rg.y; p.w = rg.w; p.h = rg.h;
    const int mw = p.hmax << log2n, mh = p.vmax << log2n;    // an MCU of the picture at this scale
    p.ux0 = rg.x / mw; p.ucols = (rg.x + rg.w - 1) / mw - p.ux0 + 1;
    p.uy0 = rg.y / mh; p.urows = (rg.y + rg.h - 1) / mh - p.uy0 + 1;
    p.n_frames = n_frames;
    p.plane_stride = plane_stride;
    p.pix_bytes = pix_bytes;
    p.row_stride = row_stride;
    const uint8_t tq3[3] = { comp_tq[0], (uint8_t)(ncomp > 1 ? comp_tq[1] : 0), (uint8_t)(ncomp > 2 ? comp_tq[2] : 0) };
    if (int rc = jpezy_internal_upload_dequant(c, qt, tq3, s)) return rc;
    p.coeffs = d_coeffs;
    p.qt = c->d_dqt.as<int>();
    p.r = d_r; p.g = d_g; p.b = d_b;
    HIP_TRY(launch_dequant_idct_region(p, s));
    return JPEZY_OK;
}

// what the two device entry points check alike, before the context is looked at
int dev_head(const char* who, const void* d_coeffs, const void* qt, const void* comp_h, const void* comp_v, const void* comp_tq, int W, int H,
             int scale_denom, const jpezy_rect* region, int n_frames)
{
    if (!d_coeffs || !qt || !comp_h || !comp_v || !comp_tq || !region) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (int rc = check_wh(W, H)) return rc;
    if (n_frames <= 0) return set_err(JPEZY_E_BADARG, "n_frames must be positive");
    if (log2n_of(scale_denom) < 0) return bad_scale(who);
    return region_inside(who, W, H, scale_denom, region);
}

}  // namespace

extern "C" {

int jpezy_region_check(int W, int H, int scale_denom, const jpezy_rect* region)
{
    if (log2n_of(scale_denom) < 0) return bad_scale("region_check");
    if (W <= 0 || H <= 0) return set_err(JPEZY_E_BADARG, "region_check: width and height must be positive");
    return region_inside("region_check", W, H, scale_denom, region);
}

int jpezy_dequant_idct_region_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                  const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray, int scale_denom,
                                  const jpezy_rect* region, int n_frames, size_t plane_stride, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b,
                                  void* stream)
{
    const char* who = "dequant_idct_region_dev";
    if (!d_r || !d_g || !d_b) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (int rc = dev_head(who, d_coeffs, qt, comp_h, comp_v, comp_tq, W, H, scale_denom, region, n_frames)) return rc;
    if (plane_stride < (size_t)region->w * region->h)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": plane_stride must hold a plane of w * h bytes");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    // the whole picture: what a full request costs today (the batch form of the full-size entry asks for a plane_stride that is a multiple
    // of 4; a batch that does not have one stays here)
    if (whole_picture(W, H, scale_denom, *region) && !(scale_denom == 1 && n_frames > 1 && plane_stride % 4))
        return jpezy_dequant_idct_scaled_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, scale_denom, n_frames,
                                             plane_stride, d_r, d_g, d_b, stream);
    HIP_TRY(hipSetDevice(c->device));
    return region_dev_core(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, log2n_of(scale_denom), *region, n_frames,
                           plane_stride, 0, 0, d_r, d_g, d_b, (hipStream_t)stream);
}

int jpezy_dequant_idct_region_packed_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                         const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray,
                                         int scale_denom, const jpezy_rect* region, int format, size_t row_stride, size_t frame_stride,
                                         int n_frames, uint8_t* d_pix, void* stream)
{
    const char* who = "dequant_idct_region_packed_dev";
    if (!d_pix) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (int rc = dev_head(who, d_coeffs, qt, comp_h, comp_v, comp_tq, W, H, scale_denom, region, n_frames)) return rc;
    PackedLayout L;
    if (int rc = packed_layout(who, format, row_stride, frame_stride, region->w, region->h, &L)) return rc;
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (whole_picture(W, H, scale_denom, *region) && !(scale_denom == 1 && n_frames > 1 && L.frame_stride % 4))
        return jpezy_dequant_idct_scaled_packed_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, scale_denom, format,
                                                    row_stride, frame_stride, n_frames, d_pix, stream);
    HIP_TRY(hipSetDevice(c->device));
    return region_dev_core(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, log2n_of(scale_denom), *region, n_frames,
                           L.frame_stride, L.bytes, (unsigned)L.row_stride, d_pix + L.off[0], d_pix + L.off[1], d_pix + L.off[2],
                           (hipStream_t)stream);
}

// .jpg bytes -> the window's planes on the host: jpezy_decode_jpeg_scaled's head, the region stage, a download of w * h bytes per plane
int jpezy_decode_jpeg_region(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int scale_denom, const jpezy_rect* region,
                             jpezy_frame_info* info, uint8_t* r, uint8_t* g, uint8_t* b, size_t plane_cap)
try {
    const char* who = "decode_jpeg_region";
    if (!info || !region) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    const int log2n = log2n_of(scale_denom);
    if (log2n < 0) return bad_scale(who);
    if (int rc = region_syntax(who, region)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    int rc = jpezy_read_jpeg_gpu(c, data, len, info, nullptr, 0);           // header only
    if (rc < 0) return rc;
    if (!r || !g || !b) return JPEZY_OK;
    const int W = info->width, H = info->height;
    if (int rc2 = jpezy_internal_check_dims(c, W, H, 1)) return rc2;
    if (int rc2 = region_inside(who, W, H, scale_denom, region)) return rc2;
    if (whole_picture(W, H, scale_denom, *region)) return jpezy_decode_jpeg_scaled(c, data, len, gray, scale_denom, info, r, g, b, plane_cap);
    const size_t plane = (size_t)region->w * region->h;
    if (plane_cap < plane) return set_err(JPEZY_E_NOSPACE, std::string(who) + ": plane buffers too small");
    if (int rc2 = read_coeffs(c, data, len, info, who)) return rc2;
    for (int k = 0; k < 3; ++k)
        if (int rc2 = c->in[k].reserve(plane)) return rc2;
    const Layout l(*info);
    if (int rc2 = region_dev_core(c, (const int16_t*)c->out.p, info->qt, info->ncomp, l.hs, l.vs, l.tq, info->precision, W, H, gray, log2n, *region, 1,
                                  plane, 0, 0, (uint8_t*)c->in[0].p, (uint8_t*)c->in[1].p, (uint8_t*)c->in[2].p, c->stream))
        return rc2;
    uint8_t* dst[3] = { r, g, b };
    for (int k = 0; k < 3; ++k) HIP_TRY(hipMemcpyAsync(dst[k], c->in[k].p, plane, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return JPEZY_OK;
}
JPEZY_CATCH

// the same into host packed pixels: the device image is tight, the caller's rows are row_stride apart
int jpezy_decode_jpeg_region_packed(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int scale_denom, const jpezy_rect* region,
                                    jpezy_frame_info* info, int format, size_t row_stride, uint8_t* pix, size_t pix_cap)
try {
    const char* who = "decode_jpeg_region_packed";
    if (!info || !region) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    const int log2n = log2n_of(scale_denom);
    if (log2n < 0) return bad_scale(who);
    if (int rc = region_syntax(who, region)) return rc;
    PackedLayout L;
    if (int rc = packed_layout(who, format, row_stride, 0, region->w, region->h, &L)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    int rc = jpezy_read_jpeg_gpu(c, data, len, info, nullptr, 0);           // header only
    if (rc < 0) return rc;
    if (!pix) return JPEZY_OK;
    const int W = info->width, H = info->height;
    if (int rc2 = jpezy_internal_check_dims(c, W, H, 1)) return rc2;
    if (int rc2 = region_inside(who, W, H, scale_denom, region)) return rc2;
    if (whole_picture(W, H, scale_denom, *region))
        return jpezy_decode_jpeg_scaled_packed(c, data, len, gray, scale_denom, info, format, row_stride, pix, pix_cap);
    const size_t tight = (size_t)region->w * L.bytes, rows = (size_t)region->h;
    if (pix_cap < (rows - 1) * L.row_stride + tight) return set_err(JPEZY_E_NOSPACE, std::string(who) + ": pixel buffer too small");
    if (int rc2 = read_coeffs(c, data, len, info, who)) return rc2;
    if (int rc2 = c->in[0].reserve(tight * rows)) return rc2;
    uint8_t* d_pix = (uint8_t*)c->in[0].p;
    const Layout l(*info);
    if (int rc2 = region_dev_core(c, (const int16_t*)c->out.p, info->qt, info->ncomp, l.hs, l.vs, l.tq, info->precision, W, H, gray, log2n, *region, 1,
                                  0, L.bytes, (unsigned)tight, d_pix + L.off[0], d_pix + L.off[1], d_pix + L.off[2], c->stream))
        return rc2;
    if (L.row_stride == tight)
        HIP_TRY(hipMemcpyAsync(pix, d_pix, tight * rows, hipMemcpyDeviceToHost, c->stream));
    else      // only bytes [0, w * bytes) of each of the caller's rows are written
        HIP_TRY(hipMemcpy2DAsync(pix, L.row_stride, d_pix, tight, tight, rows, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return JPEZY_OK;
}
JPEZY_CATCH

}  // extern "C"
