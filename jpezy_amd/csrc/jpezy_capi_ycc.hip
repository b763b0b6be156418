// jpezy_capi_ycc.hip -- the C-ABI of include/jpezy_hip.h, part 7: planar YCbCr 4:2:0 samples (I420 / YV12 / NV12 / NV21) in and out.  The
// caller's planes are the file's own sample domain: the encode kernels skip the colour conversion (first step and sample stage differ),
// the decode kernels skip replication and make_rgb (last step differs); coefficients keep their layout, so the Huffman stages, optimised
// tables, restart intervals and the file header are the RGB entries'.
#include "jpezy_capi_decode.h"
#include "jpezy_capi_encode.h"

extern "C" {

int jpezy_ycc_chroma_size(int W, int H, int* CW, int* CH)
{
    if (int rc = check_wh(W, H)) return rc;
    if (CW) *CW = (W + 1) / 2;
    if (CH) *CH = (H + 1) / 2;
    return JPEZY_OK;
}

int jpezy_ycc_component_size(const jpezy_frame_info* info, int comp, int* w, int* h)
{
    if (!info) return set_err(JPEZY_E_BADARG, "ycc_component_size: null argument");
    if (info->ncomp < 1 || info->ncomp > 3 || comp < 0 || comp >= info->ncomp)
        return set_err(JPEZY_E_BADARG, "ycc_component_size: the file has no such component");
    const int hc = info->H[comp], vc = info->V[comp];
    if (info->width <= 0 || info->height <= 0 || hc < 1 || vc < 1 || info->hmax < hc || info->vmax < vc)
        return set_err(JPEZY_E_BADARG, "ycc_component_size: not a parsed frame header");
    if (w) *w = (int)(((long)info->width * hc + info->hmax - 1) / info->hmax);
    if (h) *h = (int)(((long)info->height * vc + info->vmax - 1) / info->vmax);
    return JPEZY_OK;
}

int jpezy_fdct_quant_ycc_dev(jpezy_ctx* c, const uint8_t* d_y, size_t y_stride, const uint8_t* d_cb, const uint8_t* d_cr, size_t c_stride,
                             int c_step, size_t y_frame_stride, size_t c_frame_stride, int W, int H, int gray, int n_frames,
                             int16_t* d_coeffs, void* stream)
{
    if (int rc = check_wh(W, H)) return rc;
    YccLayout L;
    if (int rc = ycc_layout("fdct_quant_ycc_dev", W, H, y_stride, c_stride, c_step, y_frame_stride, c_frame_stride, &L)) return rc;
    if (!d_y || !d_coeffs || (!gray && (!d_cb || !d_cr))) return set_err(JPEZY_E_BADARG, "fdct_quant_ycc_dev: null device pointer");
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    return jpezy_internal_fdct_quant_core(c, EncodeSource::ycc(d_y, d_cb, d_cr, L, c_step, gray), JPEZY_SAMPLING_420, W, H, gray, n_frames, d_coeffs,
                                          (hipStream_t)stream);
}

int jpezy_dequant_idct_ycc_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], const uint8_t comp_tq[3], uint8_t* d_y,
                               size_t y_stride, uint8_t* d_cb, uint8_t* d_cr, size_t c_stride, int c_step, size_t y_frame_stride,
                               size_t c_frame_stride, int W, int H, int n_frames, void* stream)
{
    if (int rc = check_wh(W, H)) return rc;
    YccLayout L;
    if (int rc = ycc_layout("dequant_idct_ycc_dev", W, H, y_stride, c_stride, c_step, y_frame_stride, c_frame_stride, &L)) return rc;
    if (!d_coeffs || !qt || !comp_tq || !d_y) return set_err(JPEZY_E_BADARG, "dequant_idct_ycc_dev: null pointer");
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    return jpezy_internal_fused_dev_core(c, d_coeffs, qt, comp_tq, DecodeSink::ycc_planes(d_y, d_cb, d_cr, (unsigned)L.ys, c_step, (unsigned)L.cs, L.yfs, L.cfs),
                                         W, H, !d_cb && !d_cr, n_frames, (hipStream_t)stream);
}

// host planes -> .jpg bytes on the host: a file encode (jpezy_internal_encode_file) with up to three input segments per band (the Y rows,
// and the chroma rows as two planes or as one interleaved plane)
long jpezy_encode_jpeg_ycc(jpezy_ctx* c, const uint8_t* y, size_t y_stride, const uint8_t* cb, const uint8_t* cr, size_t c_stride, int c_step,
                           int W, int H, int gray, const char* comment, uint8_t* out, size_t cap)
try {
    if (int rc = check_wh(W, H)) return rc;
    YccLayout L;
    if (int rc = ycc_layout("encode_jpeg_ycc", W, H, y_stride, c_stride, c_step, 0, 0, &L)) return rc;
    if (!y || !out || (!gray && (!cb || !cr))) return set_err(JPEZY_E_BADARG, "encode_jpeg_ycc: null pointer");
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    if (int rc = check_comment(comment, "encode_jpeg_ycc")) return rc;
    // one interleaved plane (Cb and Cr neighbours) travels as one segment: its rows hold 2 * CW sample bytes from the lower pointer
    const bool inter = !gray && c_step == 2 && (cb + 1 == cr || cr + 1 == cb);
    const uint8_t* c_lo = inter ? std::min(cb, cr) : nullptr;
    const size_t c_row_bytes = inter ? (size_t)2 * L.CW : (size_t)(L.CW - 1) * c_step + 1;
    // a band goes up as it lies in the caller's buffers, row padding included, up to the last sample byte of its last row
    auto y_bytes = [=](const HostChunk& k) { return (size_t)(k.rows(H) - 1) * L.ys + (size_t)W; };
    auto c_bytes = [=](const HostChunk& k) { return (size_t)((k.rows(H) + 1) / 2 - 1) * L.cs + c_row_bytes; };
    auto pad16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    return jpezy_internal_encode_file(c, { W, H, JPEZY_SAMPLING_420, gray, comment, out, cap, (size_t)(gray ? 1 : 2),
        [&](const HostChunk& k, size_t, std::vector<jpezy_host::Segment>& in) {
            in.push_back({ const_cast<uint8_t*>(y) + (size_t)k.y0 * 16 * L.ys, y_bytes(k), 0 });
            if (gray) return;
            const size_t coff = (size_t)k.y0 * 8 * L.cs, o1 = pad16(y_bytes(k)), o2 = o1 + pad16(c_bytes(k));
            if (inter) {
                in.push_back({ const_cast<uint8_t*>(c_lo) + coff, c_bytes(k), o1 });
            } else {
                in.push_back({ const_cast<uint8_t*>(cb) + coff, c_bytes(k), o1 });
                in.push_back({ const_cast<uint8_t*>(cr) + coff, c_bytes(k), o2 });
            }
        },
        [&](const HostChunk& k, size_t, const uint8_t* d_in) {
            const size_t o1 = pad16(y_bytes(k)), o2 = o1 + pad16(c_bytes(k));
            YccLayout band = L;
            band.yfs = (size_t)k.rows(H) * L.ys;            // the tight frame strides of the band's rows
            band.cfs = (size_t)((k.rows(H) + 1) / 2) * L.cs;
            return EncodeSource::ycc(d_in, inter ? d_in + o1 + (cb > cr ? 1 : 0) : d_in + o1, inter ? d_in + o1 + (cr > cb ? 1 : 0) : d_in + o2, band,
                                     c_step, gray);
        } });
}
JPEZY_CATCH

// .jpg bytes -> component planes on the host: jpezy_decode_jpeg with the native-sample store stage of the fused kernel (jpezy's own layout)
// or of the generic pair (every other layout).  The device planes are tight; an interleaved chroma plane whose Cb and Cr are neighbours
// is written interleaved on the device and comes down as one plane, any other c_step == 2 request is scattered on the host so that
// only the caller's sample bytes are written.
int jpezy_decode_jpeg_ycc(jpezy_ctx* c, const uint8_t* data, size_t len, jpezy_frame_info* info, uint8_t* y, size_t y_stride, size_t y_cap,
                          uint8_t* cb, uint8_t* cr, size_t c_stride, int c_step, size_t c_cap)
try {
    if (c_step != 1 && c_step != 2) return set_err(JPEZY_E_BADARG, "decode_jpeg_ycc: c_step must be 1 (planes) or 2 (one interleaved plane)");
    if (!data || !info) return set_err(JPEZY_E_BADARG, "decode_jpeg_ycc: null pointer");
    if (!y && (cb || cr)) return set_err(JPEZY_E_BADARG, "decode_jpeg_ycc: null pointer: a chroma plane without the Y plane");
    if (!c) return set_err(JPEZY_E_BADARG, "decode_jpeg_ycc: null context");
    int rc = jpezy_read_jpeg_gpu(c, data, len, info, nullptr, 0);           // header only
    if (rc < 0) return rc;
    if (!y && !cb && !cr) return JPEZY_OK;
    const int W = info->width, H = info->height;
    if (int rc2 = jpezy_internal_check_dims(c, W, H, 1)) return rc2;
    if (info->ncomp != 1 && info->ncomp != 3) return set_err(JPEZY_E_UNSUPPORTED, "dimension not supported (the reference accepts 1 or 3)");
    int cw[3] = { 0, 0, 0 }, ch[3] = { 0, 0, 0 };
    for (int k = 0; k < info->ncomp; ++k)
        if (int rc2 = jpezy_ycc_component_size(info, k, &cw[k], &ch[k])) return rc2;
    uint8_t* host[3] = { y, info->ncomp == 3 ? cb : nullptr, info->ncomp == 3 ? cr : nullptr };     // a one-component file writes Y only
    const size_t ys = y_stride ? y_stride : (size_t)cw[0];
    if (ys < (size_t)cw[0]) return set_err(JPEZY_E_BADARG, "decode_jpeg_ycc: y_stride smaller than the Y plane's width");
    if (y_cap < (size_t)(ch[0] - 1) * ys + (size_t)cw[0]) return set_err(JPEZY_E_NOSPACE, "decode_jpeg_ycc: Y buffer too small");
    const int cwm = std::max(cw[1], cw[2]);
    const size_t cs = c_stride ? c_stride : (size_t)cwm * c_step;
    for (int k = 1; k < 3; ++k) {
        if (!host[k]) continue;
        if (cs < (size_t)(cw[k] - 1) * c_step + 1) return set_err(JPEZY_E_BADARG, "decode_jpeg_ycc: c_stride smaller than (wc-1) * c_step + 1");
        if (c_cap < (size_t)(ch[k] - 1) * cs + (size_t)(cw[k] - 1) * c_step + 1) return set_err(JPEZY_E_NOSPACE, "decode_jpeg_ycc: chroma buffer too small");
    }
    if (int rc2 = read_coeffs(c, data, len, info, "decode_jpeg_ycc")) return rc2;
    // device planes: Y tight in in[0]; chroma tight planes in in[1] / in[2], or one tight interleaved plane in in[1]
    const bool inter = c_step == 2 && host[1] && host[2] && (host[1] + 1 == host[2] || host[2] + 1 == host[1]) && cw[1] == cw[2] && ch[1] == ch[2] &&
                       cs >= (size_t)2 * cw[1];
    if (int rc2 = c->in[0].reserve((size_t)cw[0] * ch[0])) return rc2;
    uint8_t* d[3] = { (uint8_t*)c->in[0].p, nullptr, nullptr };
    if (inter) {
        if (int rc2 = c->in[1].reserve((size_t)2 * cw[1] * ch[1])) return rc2;
        d[1] = (uint8_t*)c->in[1].p + (host[1] > host[2] ? 1 : 0);
        d[2] = (uint8_t*)c->in[1].p + (host[2] > host[1] ? 1 : 0);
    } else {
        for (int k = 1; k < 3; ++k) {
            if (!host[k]) continue;
            if (int rc2 = c->in[k].reserve((size_t)cwm * ch[k])) return rc2;
            d[k] = (uint8_t*)c->in[k].p;
        }
    }
    const int d_step = inter ? 2 : 1;
    const size_t d_cs = inter ? (size_t)2 * cw[1] : (size_t)cwm;       // (the generic pair: one chroma row stride for both components)
    const DecodeSource src = DecodeSource::file((const int16_t*)c->out.p, *info, 0);
    if (own_layout(info)) {
        if (int rc2 = jpezy_dequant_idct_ycc_dev(c, src.d_coeffs, src.qt, src.layout.tq, d[0], (size_t)cw[0], d[1], d[2], d_cs, d_step, 0, 0, W, H, 1, c->stream))
            return rc2;
    } else if (int rc2 = jpezy_internal_generic_dev_core(c, src, DecodeSink::ycc_planes(d[0], d[1], d[2], (unsigned)cw[0], d_step, (unsigned)d_cs), c->stream, 0)) {
        return rc2;
    }
    // only sample bytes of the caller's rows are written
    HIP_TRY(hipMemcpy2DAsync(y, ys, d[0], (size_t)cw[0], (size_t)cw[0], (size_t)ch[0], hipMemcpyDeviceToHost, c->stream));
    std::vector<uint8_t> tmp[3];
    if (inter) {
        HIP_TRY(hipMemcpy2DAsync(std::min(host[1], host[2]), cs, c->in[1].p, d_cs, d_cs, (size_t)ch[1], hipMemcpyDeviceToHost, c->stream));
    } else {
        for (int k = 1; k < 3; ++k) {
            if (!host[k]) continue;
            if (c_step == 1) {
                HIP_TRY(hipMemcpy2DAsync(host[k], cs, d[k], d_cs, (size_t)cw[k], (size_t)ch[k], hipMemcpyDeviceToHost, c->stream));
            } else {
                tmp[k].resize((size_t)d_cs * ch[k]);
                HIP_TRY(hipMemcpyAsync(tmp[k].data(), d[k], tmp[k].size(), hipMemcpyDeviceToHost, c->stream));
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 1; k < 3; ++k)
        if (!tmp[k].empty())
            for (int yy = 0; yy < ch[k]; ++yy)
                for (int xx = 0; xx < cw[k]; ++xx) host[k][(size_t)yy * cs + (size_t)xx * 2] = tmp[k][(size_t)yy * d_cs + xx];
    return JPEZY_OK;
}
JPEZY_CATCH

}  // extern "C"
