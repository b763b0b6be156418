// jpezy_capi_region.hip -- the C-ABI of include/jpezy_hip.h, part 8: region-of-interest decode (a window of the picture at scale_denom 1,
// 2, 4, 8).  Header parse and Huffman decoding are those of jpezy_decode_jpeg -- the whole scan is decoded, the coefficient buffer stays
// full size --; the transform, colour and store stage is the one kernel of jpezy_kernels_region.hip over the MCUs that intersect the
// window, and only the window is downloaded.  A window that is the whole picture is handed to the reduced-size entry points as it is.
// Also here: oriented output (include/jpezy_hip_orientation.h) -- the pure helpers over jpezy_exif.h, the two device entries and the two
// file entries with an orientation argument, and the stage core's orientation.
#include "jpezy_capi_decode.h"

namespace {

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

// what the two device entry points check alike, before the context is looked at
int region_dev_head(const char* who, const void* d_coeffs, const void* qt, const void* comp_h, const void* comp_v, const void* comp_tq, int W, int H,
                    int scale_denom, const jpezy_rect* region, int n_frames)
{
    if (int rc = dev_null_check(who, { d_coeffs, qt, comp_h, comp_v, comp_tq, region })) return rc;
    if (int rc = check_wh(W, H)) return rc;
    if (n_frames <= 0) return set_err(JPEZY_E_BADARG, "n_frames must be positive");
    if (log2n_of(scale_denom) < 0) return bad_scale(who);
    return region_inside(who, W, H, scale_denom, region);
}

}  // namespace

// ... and inside a W x H file decoded at 1 / scale_denom (both already checked): no silent clipping
int jpezy_capi::region_inside(const char* who, int W, int H, int scale_denom, const jpezy_rect* r)
{
    if (int rc = region_syntax(who, r)) return rc;
    int Ws, Hs;
    (void)jpezy_scaled_size(W, H, scale_denom, &Ws, &Hs);
    if ((long)r->x + r->w > Ws || (long)r->y + r->h > Hs)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": region " + region_text(*r) + " (w x h + x + y) lies outside the picture of " +
                                           std::to_string(Ws) + " x " + std::to_string(Hs) + " at scale_denom " + std::to_string(scale_denom));
    return JPEZY_OK;
}

bool jpezy_capi::whole_picture(int W, int H, int scale_denom, const jpezy_rect& r)
{
    int Ws, Hs;
    (void)jpezy_scaled_size(W, H, scale_denom, &Ws, &Hs);
    return r.x == 0 && r.y == 0 && r.w == Ws && r.h == Hs;
}

extern "C" {

int jpezy_internal_region_dev_core(jpezy_ctx* c, const DecodeSource& src, const DecodeSink& out, hipStream_t s, int log2n, const jpezy_rect& rg,
                                   int upsampling, int orientation)
{
    RegionDecParams p;
    if (int rc = decode_geometry(c, src, out, &p)) return rc;
    p.log2n = log2n;
    int Ws, Hs;
    (void)jpezy_scaled_size(src.W, src.H, 8 >> log2n, &Ws, &Hs);
    // oriented: the kernel is given the source-side rectangle of the window and the orientation's three bits; the MCUs are that
    // rectangle's.  Orientation 1: the parameters are the ones they were
    const jpezy_exif::Rect sr = jpezy_exif::orient_rect(orientation, Ws, Hs, { rg.x, rg.y, rg.w, rg.h });
    p.orient = jpezy_exif::orient_bits(orientation);
    p.x = sr.x; p.y = sr.y; p.w = sr.w; p.h = sr.h;
    const int mw = p.hmax << log2n, mh = p.vmax << log2n;    // an MCU of the picture at this scale
    p.ux0 = sr.x / mw; p.ucols = (sr.x + sr.w - 1) / mw - p.ux0 + 1;
    p.uy0 = sr.y / mh; p.urows = (sr.y + sr.h - 1) / mh - p.uy0 + 1;
    if (int rc = upload_dequant(c, src, s)) return rc;
    if (upsampling) {
        HIP_TRY(launch_dequant_idct_region_smooth(p, Ws, Hs, s));
        return JPEZY_OK;
    }
    HIP_TRY(launch_dequant_idct_region(p, s));
    return JPEZY_OK;
}

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
    if (int rc = dev_null_check(who, { d_r, d_g, d_b })) return rc;
    if (int rc = region_dev_head(who, d_coeffs, qt, comp_h, comp_v, comp_tq, W, H, scale_denom, region, n_frames)) return rc;
    if (plane_stride < (size_t)region->w * region->h)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": plane_stride must hold a plane of w * h bytes");
    if (int rc = dev_aligned_check(d_coeffs)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    // the whole picture: what a full request costs today (the batch form of the full-size entry asks for a plane_stride that is a multiple
    // of 4; a batch that does not have one stays here)
    if (whole_picture(W, H, scale_denom, *region) && !(scale_denom == 1 && n_frames > 1 && plane_stride % 4))
        return jpezy_dequant_idct_scaled_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, scale_denom, n_frames,
                                             plane_stride, d_r, d_g, d_b, stream);
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_region_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames },
                                          DecodeSink::planes(d_r, d_g, d_b, plane_stride), (hipStream_t)stream, log2n_of(scale_denom), *region);
}

int jpezy_dequant_idct_region_packed_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                         const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray,
                                         int scale_denom, const jpezy_rect* region, int format, size_t row_stride, size_t frame_stride,
                                         int n_frames, uint8_t* d_pix, void* stream)
{
    const char* who = "dequant_idct_region_packed_dev";
    if (int rc = dev_null_check(who, { d_pix })) return rc;
    if (int rc = region_dev_head(who, d_coeffs, qt, comp_h, comp_v, comp_tq, W, H, scale_denom, region, n_frames)) return rc;
    PackedLayout L;
    if (int rc = packed_layout(who, format, row_stride, frame_stride, region->w, region->h, &L)) return rc;
    if (int rc = dev_aligned_check(d_coeffs)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (whole_picture(W, H, scale_denom, *region) && !(scale_denom == 1 && n_frames > 1 && L.frame_stride % 4))
        return jpezy_dequant_idct_scaled_packed_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, scale_denom, format,
                                                    row_stride, frame_stride, n_frames, d_pix, stream);
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_region_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames },
                                          DecodeSink::packed(L, d_pix), (hipStream_t)stream, log2n_of(scale_denom), *region);
}

// .jpg bytes -> the window's planes on the host: jpezy_decode_jpeg_scaled's head, the region stage, a download of w * h bytes per plane
int jpezy_decode_jpeg_region(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int scale_denom, const jpezy_rect* region,
                             jpezy_frame_info* info, uint8_t* r, uint8_t* g, uint8_t* b, size_t plane_cap)
try {
    const char* who = "decode_jpeg_region";
    if (!info || !region) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (log2n_of(scale_denom) < 0) return bad_scale(who);
    if (int rc = region_syntax(who, region)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    DecodeRequest rq = DecodeRequest::planes(who, DecodeStage::Region, gray, r, g, b, plane_cap);
    rq.scale_denom = scale_denom;
    rq.region = region;
    return jpezy_internal_decode_file(c, data, len, info, rq);
}
JPEZY_CATCH

// the same into host packed pixels: the device image is tight, the caller's rows are row_stride apart
int jpezy_decode_jpeg_region_packed(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int scale_denom, const jpezy_rect* region,
                                    jpezy_frame_info* info, int format, size_t row_stride, uint8_t* pix, size_t pix_cap)
try {
    const char* who = "decode_jpeg_region_packed";
    if (!info || !region) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (log2n_of(scale_denom) < 0) return bad_scale(who);
    if (int rc = region_syntax(who, region)) return rc;
    PackedLayout L;
    if (int rc = packed_layout(who, format, row_stride, 0, region->w, region->h, &L)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    DecodeRequest rq = DecodeRequest::packed(who, DecodeStage::Region, gray, format, row_stride, pix, pix_cap);
    rq.scale_denom = scale_denom;
    rq.region = region;
    return jpezy_internal_decode_file(c, data, len, info, rq);
}
JPEZY_CATCH

// ---- the same four entries with the chroma upsampling as an argument (include/jpezy_hip.h, SMOOTH UPSAMPLING OF WINDOWS).
// JPEZY_UPSAMPLE_NEAREST is handed to the entry above as it is; JPEZY_UPSAMPLE_SMOOTH makes the same checks in the same order and runs
// region_smooth_kernel (jpezy_kernels_region.hip) -- for the whole picture too: there is no smooth reduced-size entry to hand it to ----

int jpezy_dequant_idct_region_upsampling_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                             const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray,
                                             int upsampling, int scale_denom, const jpezy_rect* region, int n_frames, size_t plane_stride,
                                             uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream)
{
    const char* who = "dequant_idct_region_upsampling_dev";
    const int mode = upsampling_mode(who, upsampling, precision);
    if (mode < 0) return mode;
    if (mode == 0)
        return jpezy_dequant_idct_region_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, scale_denom, region, n_frames,
                                             plane_stride, d_r, d_g, d_b, stream);
    if (int rc = dev_null_check(who, { d_r, d_g, d_b })) return rc;
    if (int rc = region_dev_head(who, d_coeffs, qt, comp_h, comp_v, comp_tq, W, H, scale_denom, region, n_frames)) return rc;
    if (plane_stride < (size_t)region->w * region->h)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": plane_stride must hold a plane of w * h bytes");
    if (int rc = dev_aligned_check(d_coeffs)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_region_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames },
                                          DecodeSink::planes(d_r, d_g, d_b, plane_stride), (hipStream_t)stream, log2n_of(scale_denom), *region, mode);
}

int jpezy_dequant_idct_region_upsampling_packed_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp,
                                                    const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W,
                                                    int H, int gray, int upsampling, int scale_denom, const jpezy_rect* region, int format,
                                                    size_t row_stride, size_t frame_stride, int n_frames, uint8_t* d_pix, void* stream)
{
    const char* who = "dequant_idct_region_upsampling_packed_dev";
    const int mode = upsampling_mode(who, upsampling, precision);
    if (mode < 0) return mode;
    if (mode == 0)
        return jpezy_dequant_idct_region_packed_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, scale_denom, region, format,
                                                    row_stride, frame_stride, n_frames, d_pix, stream);
    if (int rc = dev_null_check(who, { d_pix })) return rc;
    if (int rc = region_dev_head(who, d_coeffs, qt, comp_h, comp_v, comp_tq, W, H, scale_denom, region, n_frames)) return rc;
    PackedLayout L;
    if (int rc = packed_layout(who, format, row_stride, frame_stride, region->w, region->h, &L)) return rc;
    if (int rc = dev_aligned_check(d_coeffs)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_region_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames },
                                          DecodeSink::packed(L, d_pix), (hipStream_t)stream, log2n_of(scale_denom), *region, mode);
}

// .jpg bytes -> the window's planes on the host; a 12-bit file is refused once its header is read (jpezy_internal_decode_file)
int jpezy_decode_jpeg_region_upsampling(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int upsampling, int scale_denom,
                                        const jpezy_rect* region, jpezy_frame_info* info, uint8_t* r, uint8_t* g, uint8_t* b, size_t plane_cap)
try {
    const char* who = "decode_jpeg_region_upsampling";
    if (upsampling == JPEZY_UPSAMPLE_NEAREST) return jpezy_decode_jpeg_region(c, data, len, gray, scale_denom, region, info, r, g, b, plane_cap);
    if (int mode = upsampling_mode(who, upsampling, 8); mode < 0) return mode;
    if (!info || !region) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (log2n_of(scale_denom) < 0) return bad_scale(who);
    if (int rc = region_syntax(who, region)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    DecodeRequest rq = DecodeRequest::planes(who, DecodeStage::RegionSmooth, gray, r, g, b, plane_cap);
    rq.scale_denom = scale_denom;
    rq.region = region;
    return jpezy_internal_decode_file(c, data, len, info, rq);
}
JPEZY_CATCH

int jpezy_decode_jpeg_region_upsampling_packed(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int upsampling, int scale_denom,
                                               const jpezy_rect* region, jpezy_frame_info* info, int format, size_t row_stride, uint8_t* pix,
                                               size_t pix_cap)
try {
    const char* who = "decode_jpeg_region_upsampling_packed";
    if (upsampling == JPEZY_UPSAMPLE_NEAREST)
        return jpezy_decode_jpeg_region_packed(c, data, len, gray, scale_denom, region, info, format, row_stride, pix, pix_cap);
    if (int mode = upsampling_mode(who, upsampling, 8); mode < 0) return mode;
    if (!info || !region) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (log2n_of(scale_denom) < 0) return bad_scale(who);
    if (int rc = region_syntax(who, region)) return rc;
    PackedLayout L;
    if (int rc = packed_layout(who, format, row_stride, 0, region->w, region->h, &L)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    DecodeRequest rq = DecodeRequest::packed(who, DecodeStage::RegionSmooth, gray, format, row_stride, pix, pix_cap);
    rq.scale_denom = scale_denom;
    rq.region = region;
    return jpezy_internal_decode_file(c, data, len, info, rq);
}
JPEZY_CATCH

// ---- oriented output (include/jpezy_hip_orientation.h): the tag's parser and the geometry are jpezy_exif.h's; the entries are the
// upsampling entries above with the window held against the oriented picture and the stage core told the orientation.  Orientation 1 is
// handed to the entry above as it is ----

int jpezy_jpeg_orientation(const uint8_t* data, size_t len) { return jpezy_exif::jpeg_orientation(data, len); }

int jpezy_orient_size(int orientation, int W, int H, int* Wo, int* Ho)
{
    if (!Wo || !Ho) return set_err(JPEZY_E_BADARG, "orient_size: null pointer");
    if (orientation < 1 || orientation > 8) return bad_orientation("orient_size", false);
    if (W <= 0 || H <= 0) return set_err(JPEZY_E_BADARG, "orient_size: width and height must be positive");
    oriented_wh(orientation, W, H, Wo, Ho);
    return JPEZY_OK;
}

int jpezy_orient_rect(int orientation, int W, int H, const jpezy_rect* oriented, jpezy_rect* source)
{
    const char* who = "orient_rect";
    if (!oriented || !source) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (orientation < 1 || orientation > 8) return bad_orientation(who, false);
    if (W <= 0 || H <= 0) return set_err(JPEZY_E_BADARG, std::string(who) + ": width and height must be positive");
    if (int rc = region_syntax(who, oriented)) return rc;
    int Wo, Ho;
    oriented_wh(orientation, W, H, &Wo, &Ho);
    if ((long)oriented->x + oriented->w > Wo || (long)oriented->y + oriented->h > Ho)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": region " + region_text(*oriented) + " (w x h + x + y) lies outside the oriented picture of " +
                                           std::to_string(Wo) + " x " + std::to_string(Ho));
    const jpezy_exif::Rect s = jpezy_exif::orient_rect(orientation, W, H, { oriented->x, oriented->y, oriented->w, oriented->h });
    *source = { s.x, s.y, s.w, s.h };
    return JPEZY_OK;
}

int jpezy_dequant_idct_region_oriented_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                           const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray, int upsampling,
                                           int scale_denom, const jpezy_rect* region, int orientation, int n_frames, size_t plane_stride,
                                           uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream)
{
    const char* who = "dequant_idct_region_oriented_dev";
    if (orientation < 1 || orientation > 8) return bad_orientation(who, false);
    if (orientation == 1)
        return jpezy_dequant_idct_region_upsampling_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, upsampling, scale_denom,
                                                        region, n_frames, plane_stride, d_r, d_g, d_b, stream);
    const int mode = upsampling_mode(who, upsampling, precision);
    if (mode < 0) return mode;
    int Wo, Ho;
    oriented_wh(orientation, W, H, &Wo, &Ho);
    if (int rc = dev_null_check(who, { d_r, d_g, d_b })) return rc;
    if (int rc = region_dev_head(who, d_coeffs, qt, comp_h, comp_v, comp_tq, Wo, Ho, scale_denom, region, n_frames)) return rc;
    if (plane_stride < (size_t)region->w * region->h)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": plane_stride must hold a plane of w * h bytes");
    if (int rc = dev_aligned_check(d_coeffs)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_region_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames },
                                          DecodeSink::planes(d_r, d_g, d_b, plane_stride), (hipStream_t)stream, log2n_of(scale_denom), *region, mode,
                                          orientation);
}

int jpezy_dequant_idct_region_oriented_packed_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp,
                                                  const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W,
                                                  int H, int gray, int upsampling, int scale_denom, const jpezy_rect* region, int orientation,
                                                  int format, size_t row_stride, size_t frame_stride, int n_frames, uint8_t* d_pix, void* stream)
{
    const char* who = "dequant_idct_region_oriented_packed_dev";
    if (orientation < 1 || orientation > 8) return bad_orientation(who, false);
    if (orientation == 1)
        return jpezy_dequant_idct_region_upsampling_packed_dev(c, d_coeffs, qt, ncomp, comp_h, comp_v, comp_tq, precision, W, H, gray, upsampling,
                                                               scale_denom, region, format, row_stride, frame_stride, n_frames, d_pix, stream);
    const int mode = upsampling_mode(who, upsampling, precision);
    if (mode < 0) return mode;
    int Wo, Ho;
    oriented_wh(orientation, W, H, &Wo, &Ho);
    if (int rc = dev_null_check(who, { d_pix })) return rc;
    if (int rc = region_dev_head(who, d_coeffs, qt, comp_h, comp_v, comp_tq, Wo, Ho, scale_denom, region, n_frames)) return rc;
    PackedLayout L;
    if (int rc = packed_layout(who, format, row_stride, frame_stride, region->w, region->h, &L)) return rc;
    if (int rc = dev_aligned_check(d_coeffs)) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_region_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames },
                                          DecodeSink::packed(L, d_pix), (hipStream_t)stream, log2n_of(scale_denom), *region, mode, orientation);
}

namespace {
// what the two file entries check alike, in the order the header documents; *o: the orientation to apply
int oriented_file_head(const char* who, const uint8_t* data, size_t len, int upsampling, int scale_denom, const jpezy_rect* region, int orientation,
                       int* orientation_used, const jpezy_frame_info* info, int* o)
{
    if (int mode = upsampling_mode(who, upsampling, 8); mode < 0) return mode;
    if (orientation != JPEZY_ORIENT_FROM_FILE && (orientation < 1 || orientation > 8)) return bad_orientation(who, true);
    if (!info) return set_err(JPEZY_E_BADARG, std::string(who) + ": null pointer");
    if (log2n_of(scale_denom) < 0) return bad_scale(who);
    if (region)
        if (int rc = region_syntax(who, region)) return rc;
    *o = orientation == JPEZY_ORIENT_FROM_FILE ? jpezy_exif::jpeg_orientation(data, len) : orientation;
    if (orientation_used) *orientation_used = *o;
    return JPEZY_OK;
}
}  // namespace

int jpezy_decode_jpeg_oriented(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int upsampling, int scale_denom, const jpezy_rect* region,
                               int orientation, int* orientation_used, jpezy_frame_info* info, uint8_t* r, uint8_t* g, uint8_t* b,
                               size_t plane_cap)
try {
    const char* who = "decode_jpeg_oriented";
    int o;
    if (int rc = oriented_file_head(who, data, len, upsampling, scale_denom, region, orientation, orientation_used, info, &o)) return rc;
    if (o == 1 && region) return jpezy_decode_jpeg_region_upsampling(c, data, len, gray, upsampling, scale_denom, region, info, r, g, b, plane_cap);
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (o == 1 && upsampling == JPEZY_UPSAMPLE_NEAREST) return jpezy_decode_jpeg_scaled(c, data, len, gray, scale_denom, info, r, g, b, plane_cap);
    DecodeRequest rq = DecodeRequest::planes(who, upsampling == JPEZY_UPSAMPLE_NEAREST ? DecodeStage::Region : DecodeStage::RegionSmooth, gray, r, g, b,
                                             plane_cap);
    rq.scale_denom = scale_denom;
    rq.region = region;
    rq.orientation = o;
    rq.whole_oriented = region == nullptr;
    return jpezy_internal_decode_file(c, data, len, info, rq);
}
JPEZY_CATCH

int jpezy_decode_jpeg_oriented_packed(jpezy_ctx* c, const uint8_t* data, size_t len, int gray, int upsampling, int scale_denom,
                                      const jpezy_rect* region, int orientation, int* orientation_used, jpezy_frame_info* info, int format,
                                      size_t row_stride, uint8_t* pix, size_t pix_cap)
try {
    const char* who = "decode_jpeg_oriented_packed";
    int o;
    if (int rc = oriented_file_head(who, data, len, upsampling, scale_denom, region, orientation, orientation_used, info, &o)) return rc;
    if (o == 1 && region)
        return jpezy_decode_jpeg_region_upsampling_packed(c, data, len, gray, upsampling, scale_denom, region, info, format, row_stride, pix, pix_cap);
    if (region) {
        PackedLayout L;
        if (int rc = packed_layout(who, format, row_stride, 0, region->w, region->h, &L)) return rc;
    } else if (jpezy_pixel_bytes(format) < 0) {
        return set_err(JPEZY_E_BADARG, std::string(who) + ": unknown pixel format");
    }
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (o == 1 && upsampling == JPEZY_UPSAMPLE_NEAREST)
        return jpezy_decode_jpeg_scaled_packed(c, data, len, gray, scale_denom, info, format, row_stride, pix, pix_cap);
    DecodeRequest rq = DecodeRequest::packed(who, upsampling == JPEZY_UPSAMPLE_NEAREST ? DecodeStage::Region : DecodeStage::RegionSmooth, gray, format,
                                             row_stride, pix, pix_cap);
    rq.scale_denom = scale_denom;
    rq.region = region;
    rq.orientation = o;
    rq.whole_oriented = region == nullptr;
    return jpezy_internal_decode_file(c, data, len, info, rq);
}
JPEZY_CATCH

}  // extern "C"
