// jpezy_capi_decode.h -- what the decode entries of the C-ABI share (internal).  A transform stage is described by two values: where the
// coefficients come from (DecodeSource) and where the pixels go on the device (DecodeSink); the three stage cores -- any-layout pair
// (jpezy_capi.hip), reduced-size pair (jpezy_capi_scaled.hip), region kernel (jpezy_capi_region.hip) -- take the two and fill their
// kernel parameters' common part through one geometry function.  A file decode (.jpg bytes on the host -> pixels on the host) is one
// driver, jpezy_internal_decode_file (jpezy_capi_huffdec.hip), steered by a DecodeRequest; the public entries check their own
// arguments and call it.
#pragma once
#include "jpezy_capi_internal.h"
#include "jpezy_exif.h"

namespace jpezy_capi {

// sampling factors and quantiser-table selectors of the (up to) three components
struct Layout {
    uint8_t hs[3], vs[3], tq[3];
    explicit Layout(const jpezy_frame_info& info)
    {
        for (int k = 0; k < 3; ++k) { hs[k] = (uint8_t)info.H[k]; vs[k] = (uint8_t)info.V[k]; tq[k] = (uint8_t)info.Tq[k]; }
    }
    Layout(const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3])
    {
        for (int k = 0; k < 3; ++k) { hs[k] = comp_h[k]; vs[k] = comp_v[k]; tq[k] = comp_tq[k]; }
    }
};

// jpezy's own files: three 8-bit components sampled 2x2, 1x1, 1x1 -- the layout of the fused kernel
inline bool own_layout(const jpezy_frame_info* info)
{
    return info->ncomp == 3 && info->precision == 8 && info->H[0] == 2 && info->V[0] == 2 && info->H[1] == 1 && info->V[1] == 1 &&
           info->H[2] == 1 && info->V[2] == 1;
}

// n_frames frames of one layout, size and set of quantiser tables, their coefficients one behind the other in device memory
struct DecodeSource {
    const int16_t* d_coeffs;
    const uint16_t (*qt)[64];
    int ncomp;
    Layout layout;
    int precision, W, H, gray, n_frames;
    // one frame as jpezy_read_jpeg_gpu left it
    static DecodeSource file(const int16_t* d_coeffs, const jpezy_frame_info& info, int gray)
    {
        return { d_coeffs, info.qt, info.ncomp, Layout(info), info.precision, info.width, info.height, gray, 1 };
    }
};

// where the pixels go on the device.  Planes: r, g, b, frames frame_stride apart.  Packed (pix_bytes 3 or 4): r, g, b are the channel
// bytes of pixel (0, 0), rows row_stride apart.  Native component planes (ycc, the any-layout pair only): r, g, b are sample (0, 0) of
// the components (null: not wanted), rows row_stride / c_row_stride apart, chroma samples c_step apart.  The fused kernel's batches
// (jpezy_internal_fused_dev_core) also read c_frame_stride, the chroma planes' frame stride, and pix, the packed buffer's first byte;
// the three stage cores read neither.  Packed YCbCr 4:2:2 macropixels (yuv422, the any-layout pair only): r, g, b are the Y0, Cb, Cr
// bytes of macropixel (0, 0), rows row_stride, frames frame_stride (any value) apart.
struct DecodeSink {
    uint8_t *r, *g, *b;
    size_t frame_stride;
    int pix_bytes;
    unsigned row_stride;
    int ycc, c_step;
    unsigned c_row_stride;
    size_t c_frame_stride = 0;
    uint8_t* pix = nullptr;
    int yuv422 = 0;             // packed YCbCr 4:2:2 macropixels (the any-layout pair only): r, g, b are the Y0, Cb, Cr bytes of macropixel (0, 0)
    static DecodeSink planes(uint8_t* r, uint8_t* g, uint8_t* b, size_t plane_stride) { return { r, g, b, plane_stride, 0, 0, 0, 1, 0 }; }
    static DecodeSink packed(const PackedLayout& L, uint8_t* pix)
    {
        return { pix + L.off[0], pix + L.off[1], pix + L.off[2], L.frame_stride, L.bytes, (unsigned)L.row_stride, 0, 1, 0, 0, pix };
    }
    static DecodeSink ycc_planes(uint8_t* y, uint8_t* cb, uint8_t* cr, unsigned y_row_stride, int c_step, unsigned c_row_stride,
                                 size_t y_frame_stride = 0, size_t c_frame_stride = 0)
    {
        return { y, cb, cr, y_frame_stride, 0, y_row_stride, 1, c_step, c_row_stride, c_frame_stride };
    }
    // y_off, cb_off, cr_off: where the three bytes lie inside a macropixel (the format); rows row_stride, frames frame_stride apart
    static DecodeSink yuv422_packed(uint8_t* pix, int y_off, int cb_off, int cr_off, unsigned row_stride, size_t frame_stride)
    {
        return { pix + y_off, pix + cb_off, pix + cr_off, frame_stride, 2, row_stride, 0, 1, 0, 0, pix, 1 };
    }
    // the same sink `frames` frames on; component planes that are not wanted stay null
    void advance(size_t frames)
    {
        const size_t adv = frames * frame_stride, c_adv = ycc ? frames * c_frame_stride : adv;
        r += adv;
        if (g) g += c_adv;
        if (b) b += c_adv;
        if (pix) pix += adv;
    }
};

// What GenericDecParams, ScaledDecParams and RegionDecParams share by name: the MCU geometry of the layout (get_blocks, ref :166-169),
// the level shift, and where coefficients, quantisers and pixels are.  The quantisers are the context's (jpezy_internal_upload_dequant
// fills them; the pointer does not move).
template <class Params>
int decode_geometry(jpezy_ctx* c, const DecodeSource& src, const DecodeSink& out, Params* params)
{
    Params& p = *params;
    if (src.ncomp != 1 && src.ncomp != 3) return set_err(JPEZY_E_UNSUPPORTED, "dimension not supported (the reference accepts 1 or 3)");
    p.ncomp = src.ncomp; p.gray = src.gray != 0;
    p.level = src.precision == 8 ? 128 : 2048;                // ref :654
    p.hmax = p.vmax = 0;
    p.blocks_per_mcu = 0;
    for (int k = 0; k < 3; ++k) { p.ch[k] = p.cv[k] = 1; p.blk_start[k] = 1 << 20; }
    for (int k = 0; k < src.ncomp; ++k) {
        p.ch[k] = src.layout.hs[k]; p.cv[k] = src.layout.vs[k];
        if (p.ch[k] < 1 || p.ch[k] > 4 || p.cv[k] < 1 || p.cv[k] > 4)
            return set_err(JPEZY_E_UNSUPPORTED, "sampling factors outside 1..4 (ITU-T T.81 B.2.2)");
        p.hmax = p.ch[k] > p.hmax ? p.ch[k] : p.hmax;
        p.vmax = p.cv[k] > p.vmax ? p.cv[k] : p.vmax;
        p.blk_start[k] = p.blocks_per_mcu;
        p.blocks_per_mcu += p.ch[k] * p.cv[k];
    }
    const int Hblock = (src.W >> 3) + ((src.W & 7) > 0), Vblock = (src.H >> 3) + ((src.H & 7) > 0);
    p.mcu_cols = Hblock / p.hmax + ((Hblock % p.hmax) ? 1 : 0);
    p.mcu_rows = Vblock / p.vmax + ((Vblock % p.vmax) ? 1 : 0);
    p.n_frames = src.n_frames;
    p.plane_stride = out.frame_stride;
    p.pix_bytes = out.pix_bytes;
    p.row_stride = out.row_stride;
    p.coeffs = src.d_coeffs;
    p.qt = c->d_dqt.as<int>();
    p.r = out.r; p.g = out.g; p.b = out.b;
    return JPEZY_OK;
}
template <class Params>
size_t geometry_blocks(const Params& p) { return (size_t)p.mcu_cols * p.mcu_rows * p.blocks_per_mcu; }

// the context's dequantiser tables for the components the layout has
inline int upload_dequant(jpezy_ctx* c, const DecodeSource& src, hipStream_t s)
{
    const uint8_t tq3[3] = { src.layout.tq[0], (uint8_t)(src.ncomp > 1 ? src.layout.tq[1] : 0), (uint8_t)(src.ncomp > 2 ? src.layout.tq[2] : 0) };
    return jpezy_internal_upload_dequant(c, src.qt, tq3, s);
}

// 8 / scale_denom as a shift: 3, 2, 1, 0 for the denominators 1, 2, 4, 8; -1 for anything else
inline int log2n_of(int scale_denom) { return scale_denom == 1 ? 3 : scale_denom == 2 ? 2 : scale_denom == 4 ? 1 : scale_denom == 8 ? 0 : -1; }
inline int bad_scale(const char* who) { return set_err(JPEZY_E_BADARG, std::string(who) + ": scale_denom must be 1, 2, 4 or 8"); }

// the file's size as region_inside is to see it for a window of the oriented picture: swapped for the transposed orientations
// (jpezy_scaled_size treats the two axes alike)
inline void oriented_wh(int orientation, int W, int H, int* Wo, int* Ho)
{
    const bool tr = (jpezy_exif::orient_bits(orientation) & jpezy_exif::kTranspose) != 0;
    *Wo = tr ? H : W; *Ho = tr ? W : H;
}
inline int bad_orientation(const char* who, bool from_file_allowed)
{
    return set_err(JPEZY_E_BADARG, std::string(who) + (from_file_allowed ? ": orientation must be JPEZY_ORIENT_FROM_FILE or 1..8" : ": orientation must be 1..8"));
}

// 0: nearest (the entries hand the call to the existing entry), 1: smooth, negative: the status to return
inline int upsampling_mode(const char* who, int upsampling, int precision)
{
    if (upsampling == JPEZY_UPSAMPLE_NEAREST) return 0;
    if (upsampling != JPEZY_UPSAMPLE_SMOOTH)
        return set_err(JPEZY_E_BADARG, std::string(who) + ": upsampling must be JPEZY_UPSAMPLE_NEAREST or JPEZY_UPSAMPLE_SMOOTH");
    if (precision != 8)
        return set_err(JPEZY_E_UNSUPPORTED, std::string(who) + ": JPEZY_UPSAMPLE_SMOOTH is defined for 8-bit files only");
    return 1;
}

// ---- the head of the jpezy_dequant_idct_*_dev entries, in pieces: the entries make the same checks in different orders, and the order
// is observable (which of two bad arguments is named) ----
// who null: the plain text of the entries that look at the context first
inline int dev_null_check(const char* who, std::initializer_list<const void*> pointers)
{
    for (const void* p : pointers)
        if (!p) return set_err(JPEZY_E_BADARG, who ? std::string(who) + ": null pointer" : std::string("null pointer"));
    return JPEZY_OK;
}
inline int dev_aligned_check(const int16_t* d_coeffs)
{
    return aligned16(d_coeffs) ? JPEZY_OK : set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
}
// context, dimensions and frame count first, then the pointers: every entry but the region pair (which looks at the context last)
inline int dev_head(jpezy_ctx* c, int W, int H, int n_frames, std::initializer_list<const void*> pointers, const int16_t* d_coeffs)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (int rc = dev_null_check(nullptr, pointers)) return rc;
    return dev_aligned_check(d_coeffs);
}

// ---- a file decode: .jpg bytes on the host -> pixels on the host ----
// the file's coefficients into c->out (GPU Huffman decoder, or the host's for what it declines); info holds the parsed header
inline int read_coeffs(jpezy_ctx* c, const uint8_t* data, size_t len, jpezy_frame_info* info, const char* who)
{
    const size_t ncoef = (size_t)info->mcu_cols * info->mcu_rows * info->blocks_per_mcu * 64;
    // sized from untrusted SOF0 fields: a block costs at least 2 bits of scan (1-bit DC code + 1-bit EOB code)
    if (ncoef / 64 > 4 * len) return set_err(JPEZY_E_FORMAT, std::string(who) + ": scan too short for the declared dimensions");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = c->out.reserve(ncoef * sizeof(int16_t))) return rc;
    const int rc = jpezy_read_jpeg_gpu(c, data, len, info, (int16_t*)c->out.p, ncoef);
    return rc < 0 ? rc : JPEZY_OK;
}

// Full: the fused kernel for jpezy's own layout, the any-layout pair for every other; Smooth: the any-layout pair with the smooth second
// stage for every layout; Scaled, Region: the kernels of those parts; RegionSmooth: the region stage with smooth chroma upsampling
// (jpezy_kernels_region.hip), at every scale and for the whole picture too
enum class DecodeStage { Full, Scaled, Region, Smooth, RegionSmooth };

struct DecodeRequest {
    const char* who;            // the entry: prefix of the messages
    DecodeStage stage;
    int gray;
    int scale_denom;            // size rule: the picture at 1 / scale_denom (Scaled, Region: 2, 4, 8 resp. 1, 2, 4, 8, checked by the entry) ...
    const jpezy_rect* region;   // ... or, Region, this window of it (syntax checked by the entry); null otherwise
    // sink: three host planes of cap bytes each, or (format >= 0) packed host pixels at dst[0], rows row_stride apart (0: tight), cap bytes
    int format;
    size_t row_stride;
    uint8_t* dst[3];
    size_t cap;
    // oriented output (Region, RegionSmooth; include/jpezy_hip_orientation.h): the orientation applied, 1..8 -- region is then a window of
    // the ORIENTED picture; whole_oriented: no region was given, the window is all of that picture
    int orientation = 1;
    bool whole_oriented = false;
    static DecodeRequest planes(const char* who, DecodeStage stage, int gray, uint8_t* r, uint8_t* g, uint8_t* b, size_t plane_cap)
    {
        return { who, stage, gray, 1, nullptr, -1, 0, { r, g, b }, plane_cap, 1, false };
    }
    static DecodeRequest packed(const char* who, DecodeStage stage, int gray, int format, size_t row_stride, uint8_t* pix, size_t pix_cap)
    {
        return { who, stage, gray, 1, nullptr, format, row_stride, { pix, pix, pix }, pix_cap, 1, false };
    }
    bool is_packed() const { return format >= 0; }
};

// what a region must satisfy inside a W x H file decoded at 1 / scale_denom; the window is the whole picture (jpezy_capi_region.hip)
JPEZY_INTERNAL int region_inside(const char* who, int W, int H, int scale_denom, const jpezy_rect* r);
JPEZY_INTERNAL bool whole_picture(int W, int H, int scale_denom, const jpezy_rect& r);

// one file of a launch of resample_kernel: its w x h source pixels at src_off (a multiple of 4) behind the launch's source, its output at dst_off
// (bytes; elements for a tensor output)
struct ResampleJob {
    unsigned long long src_off, dst_off;
    int w, h, mirror;
};
// how a launch resamples: the filter (a value of enum jpezy_filter) and direct != 0: no file takes the two-pass tile
struct ResampleHow {
    int filter, direct;
};

}  // namespace jpezy_capi

extern "C" {
// The stage cores: geometry + tables + launches on device memory; asynchronous on stream s (the tables are uploaded synchronously when
// they changed since the last call).  The arguments are the callers' to check.
// any-layout pair; upsampling != 0 (JPEZY_UPSAMPLE_SMOOTH): smooth_rgb_kernel in generic_rgb_kernel's place (jpezy_capi.hip)
JPEZY_INTERNAL int jpezy_internal_generic_dev_core(jpezy_ctx* c, const DecodeSource& src, const DecodeSink& out, hipStream_t s, int upsampling);
// the fused kernel of the project's own layout (three 8-bit components, 2x2 / 1x1 / 1x1) over n_frames frames: the dequantiser upload,
// the one place that fills a DecParams and cuts a batch at kMaxFramesPerLaunch, and the choice among the planar, packed and native-sample
// launches by the sink (jpezy_capi.hip).  gray: luma only for a native-sample sink
JPEZY_INTERNAL int jpezy_internal_fused_dev_core(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], const uint8_t comp_tq[3],
                                                 const DecodeSink& out, int W, int H, int gray, int n_frames, hipStream_t s);
// reduced size, log2n = 2, 1, 0 (jpezy_capi_scaled.hip)
JPEZY_INTERNAL int jpezy_internal_scaled_dev_core(jpezy_ctx* c, const DecodeSource& src, const DecodeSink& out, hipStream_t s, int log2n);
// the window rg (inside the picture) at log2n = 3, 2, 1, 0; the sink is the window's; upsampling != 0 (JPEZY_UPSAMPLE_SMOOTH, 8-bit files):
// region_smooth_kernel in region_kernel's place (jpezy_capi_region.hip).  orientation 2..8: rg is a window of the ORIENTED picture
// (inside it) and the ORIENT instances of the two kernels run; 1: the launches made without the argument
JPEZY_INTERNAL int jpezy_internal_region_dev_core(jpezy_ctx* c, const DecodeSource& src, const DecodeSink& out, hipStream_t s, int log2n,
                                                  const jpezy_rect& rg, int upsampling = 0, int orientation = 1);
// the second stage of the resized batch of windows: tap tables and descriptors of `jobs` through c->r_pin / c->r_tab, then resample_kernel
// (jpezy_capi_resized.hip).  tensor: resample_tensor_kernel in its place -- d_dst is the tensor's first element, ResampleJob::dst_off counts
// elements, dst_stride is not read and bytes is 3.  how: the filter and the form, the CALL's (a child context is handed its parent's);
// *tiled: the jobs that run the two-pass tile.  JPEZY_E_UNSUPPORTED: a table whose weights could overflow a 32-bit accumulator
JPEZY_INTERNAL int jpezy_internal_resample(jpezy_ctx* c, const std::vector<ResampleJob>& jobs, const uint8_t* d_src, unsigned src_stride,
                                           uint8_t* d_dst, size_t dst_stride, int out_w, int out_h, int bytes, hipStream_t s, const ResampleHow& how,
                                           int* tiled, hipEvent_t t0 = nullptr, hipEvent_t t1 = nullptr, const TensorOut* tensor = nullptr);
// header, output size, capacity, coefficients (read_coeffs), staging in c->in, the stage, download, synchronise (jpezy_capi_huffdec.hip).
// No output pointer: header only.  c and info are not null.
JPEZY_INTERNAL int jpezy_internal_decode_file(jpezy_ctx* c, const uint8_t* data, size_t len, jpezy_frame_info* info, const DecodeRequest& rq);
}
