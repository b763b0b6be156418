// jpezy_capi_encode.h -- what the encode entries of the C-ABI share (internal); the twin of jpezy_capi_decode.h.  A transform launch is
// described by where the pixels are on the device (EncodeSource); one core, jpezy_internal_fdct_quant_core (jpezy_capi.hip), turns the
// source, the sampling and the context's settings into kernel parameters, cuts the batch at the launch limit and picks the launcher.
// A file encode (pixels on the host -> .jpg bytes on the host) is one driver, jpezy_internal_encode_file (jpezy_capi_entropy.hip),
// steered by an EncodeRequest; the public entries check their own arguments, in their own order, and call one of the two.
#pragma once
#include "jpezy_capi_internal.h"

namespace jpezy_capi {

// where the pixels are on the device.  Planes: r, g, b, frames frame_stride apart.  Packed (pix_bytes 3 or 4): pix is the buffer's first
// byte, r, g, b the channel bytes of pixel (0, 0), rows row_stride apart, swap_rb: blue comes first.  Planar YCbCr 4:2:0 (c_step 1 or
// 2): r = Y (rows row_stride, frames frame_stride apart), g, b = Cb, Cr (rows c_row_stride, samples c_step, frames c_frame_stride
// apart; null in a gray transform, which does not read them).
struct EncodeSource {
    const uint8_t *r, *g, *b;
    size_t frame_stride;
    const uint8_t* pix;
    int pix_bytes;
    unsigned row_stride;
    int swap_rb;
    unsigned c_row_stride;
    int c_step;
    size_t c_frame_stride;
    // YCbCr 4:2:2 samples (JPEZY_SAMPLING_422 only): the planar description with CH = H, or (y_step 2) packed macropixels -- r, g, b the
    // Y0, Cb, Cr bytes of macropixel (0, 0), c_step 4, pix the buffer's first byte, both row and both frame strides the buffer's
    int y_step = 1, yuv_format = 0;
    static EncodeSource planes(const uint8_t* r, const uint8_t* g, const uint8_t* b, size_t plane_stride)
    {
        return { r, g, b, plane_stride, nullptr, 0, 0, 0, 0, 0, 0 };
    }
    static EncodeSource packed(const PackedLayout& L, const uint8_t* pix)
    {
        return { pix + L.off[0], pix + L.off[1], pix + L.off[2], L.frame_stride, pix, L.bytes, (unsigned)L.row_stride, L.off[0] != 0, 0, 0, 0 };
    }
    static EncodeSource ycc(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, const YccLayout& L, int c_step, int gray)
    {
        return { y, gray ? nullptr : cb, gray ? nullptr : cr, L.yfs, nullptr, 0, (unsigned)L.ys, 0, (unsigned)L.cs, c_step, L.cfs };
    }
    static EncodeSource ycc422(const uint8_t* y, const uint8_t* cb, const uint8_t* cr, const YccLayout& L, int c_step) { return ycc(y, cb, cr, L, c_step, 0); }
    static EncodeSource yuv422(const Yuv422Layout& L, int format, const uint8_t* pix)
    {
        return { pix + L.off[0], pix + L.off[1], pix + L.off[2], L.frame_stride, pix, 0, (unsigned)L.row_stride, 0, (unsigned)L.row_stride, 4,
                 L.frame_stride, 2, format };
    }
    bool is_ycc() const { return c_step != 0; }
    // the same source `frames` frames on; chroma planes that are not there stay null
    void advance(size_t frames)
    {
        const size_t adv = frames * frame_stride, c_adv = is_ycc() ? frames * c_frame_stride : adv;
        r += adv;
        if (g) g += c_adv;
        if (b) b += c_adv;
        if (pix) pix += adv;
    }
};

inline const char* sampling_name(int sampling) { return sampling == JPEZY_SAMPLING_422 ? "JPEZY_SAMPLING_422" : "JPEZY_SAMPLING_444"; }

// JPEZY_DOWNSAMPLE_AVERAGE acts on a transform: colour, from RGB pixels (planes or packed), and the stage decimates -- 4:2:0 and 4:2:2;
// never planar YCbCr input (its chroma is the caller's), never 4:4:4
inline bool encode_averaged(const jpezy_ctx* c, int sampling, int gray)
{
    return !gray && sampling != JPEZY_SAMPLING_444 && c->chroma_downsampling == JPEZY_DOWNSAMPLE_AVERAGE;
}

// What a transform from RGB pixels refuses before it touches anything: encode variant 0 (the FP64 kernel) has no 4:4:4 or 4:2:2 form
// and no averaged chroma stage.  The entries raise it at their own place in their check order, under their own name.
inline int check_encode_variant(const jpezy_ctx* c, int sampling, int gray, const char* who)
{
    if (c->variant != 0) return JPEZY_OK;
    if (sampling != JPEZY_SAMPLING_420)
        return set_err(JPEZY_E_UNSUPPORTED, std::string(who) + ": encode variant 0 (FP64) has no " + sampling_name(sampling) + " form; use variant 1");
    if (encode_averaged(c, sampling, gray))
        return set_err(JPEZY_E_UNSUPPORTED, std::string(who) + ": encode variant 0 (FP64) has no JPEZY_DOWNSAMPLE_AVERAGE form; use variant 1 "
                                                              "or JPEZY_DOWNSAMPLE_POINT");
    return JPEZY_OK;
}

// ---- a file encode: pixels on the host -> .jpg bytes on the host ----
// What differs between the pixel kinds: how many bytes a pixel costs the chunk planner (3; the packed format's; 1 or 2 for YCbCr),
// which host segments make up a band (appended to ChunkPlan::in; P: the plane pitch of the call's bands, plane_pitch), and the
// EncodeSource of a band whose segments were staged at d_in.
struct EncodeRequest {
    int W, H, sampling, gray;
    const char* comment;
    uint8_t* out;
    size_t cap;
    size_t bytes_per_px;
    std::function<void(const HostChunk& k, size_t P, std::vector<jpezy_host::Segment>& in)> segments;
    std::function<EncodeSource(const HostChunk& k, size_t P, const uint8_t* d_in)> source;
};

// a file encode from packed pixels (jpezy_capi_packed.hip): jpezy_encode_jpeg_packed and jpezy_encode_jpeg_sampling_packed
JPEZY_INTERNAL EncodeRequest packed_encode_request(const uint8_t* pix, const PackedLayout& L, int W, int H, int sampling, int gray, const char* comment,
                                                   uint8_t* out, size_t cap);
// ... and from planes (jpezy_capi_entropy.hip): jpezy_encode_jpeg and jpezy_encode_jpeg_sampling
JPEZY_INTERNAL EncodeRequest planar_encode_request(const uint8_t* r, const uint8_t* g, const uint8_t* b, int W, int H, int sampling, int gray,
                                                   const char* comment, uint8_t* out, size_t cap);

}  // namespace jpezy_capi

extern "C" {
// The one place that fills an EncParams, cuts a batch at kMaxFramesPerLaunch and chooses the launcher (jpezy_capi.hip); asynchronous on
// stream s.  sampling is known, gray is 0 with 4:4:4 / 4:2:2, the variant refusals (check_encode_variant) were raised: the arguments are
// the callers' to check.
JPEZY_INTERNAL int jpezy_internal_fdct_quant_core(jpezy_ctx* c, const EncodeSource& src, int sampling, int W, int H, int gray, int n_frames,
                                                  int16_t* d_coeffs, hipStream_t s);
// e_coef, upload and transform (4:2:0: band by band through run_host_bands; 4:4:4 / 4:2:2: the frame as one band, uploaded directly),
// then the GPU writer (jpezy_capi_entropy.hip).  The arguments are the callers' to check.
JPEZY_INTERNAL long jpezy_internal_encode_file(jpezy_ctx* c, const EncodeRequest& rq);
}
