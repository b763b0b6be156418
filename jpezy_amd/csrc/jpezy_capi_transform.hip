// jpezy_capi_transform.hip -- the C-ABI of include/jpezy_hip.h, part 10: lossless transforms (flip, rotate, transpose, none) in the
// coefficient domain.  The reference has no such mode; the definition is in the header.  jpezy_transform_jpeg connects the two halves that
// exist -- the head of jpezy_read_jpeg_gpu (header on the host, scan through the GPU Huffman decoder or the host's) and the GPU entropy
// coder behind jpezy_write_jpeg_gpu_sampling -- with the one kernel of jpezy_kernels_transform.hip between them; no pixel is computed.
#include "jpezy_capi_decode.h"

namespace {

struct Op { int swap, mirror_x, mirror_y; };
// libjpeg's JXFORM order: none, hflip, vflip, transpose, transverse, rot90, rot180, rot270
constexpr Op kOps[8] = { { 0, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 }, { 1, 0, 0 }, { 1, 1, 1 }, { 1, 0, 1 }, { 0, 1, 1 }, { 1, 1, 0 } };

int check_op(const char* who, int op, int flags)
{
    if (op < 0 || op > 7) return set_err(JPEZY_E_BADARG, std::string(who) + ": unknown op " + std::to_string(op) + " (JPEZY_XFORM_NONE = 0 .. JPEZY_XFORM_ROT270 = 7)");
    if (flags & ~JPEZY_XFORM_TRIM) return set_err(JPEZY_E_BADARG, std::string(who) + ": unknown flags (JPEZY_XFORM_TRIM = 1 is the only one)");
    return JPEZY_OK;
}

int check_sampling(const char* who, int sampling)
{
    if (sampling == JPEZY_SAMPLING_420 || sampling == JPEZY_SAMPLING_444) return JPEZY_OK;
    return set_err(JPEZY_E_BADARG, std::string(who) + ": unknown sampling (JPEZY_SAMPLING_420 = 0, JPEZY_SAMPLING_444 = 1)");
}

struct Geometry {
    int Wt, Ht;          // the source's trimmed size
    int C, R;            // ... in MCUs
    int Wout, Hout;
};

// op, flags, sampling and size are good: the edge rule.  A mirrored source axis must be whole MCUs or be trimmed to them.
int geometry(const char* who, int op, int flags, int W, int H, int sampling, Geometry* g)
{
    const int m = sampling == JPEZY_SAMPLING_444 ? 8 : 16;
    const Op o = kOps[op];
    int len[2] = { W, H };
    const int mirrored[2] = { o.mirror_x, o.mirror_y };
    const char* axis[2] = { "width", "height" };
    for (int k = 0; k < 2; ++k) {
        if (!mirrored[k] || len[k] % m == 0) continue;
        if (!(flags & JPEZY_XFORM_TRIM))
            return set_err(JPEZY_E_UNSUPPORTED, std::string(who) + ": the " + axis[k] + " (" + std::to_string(len[k]) + ") is mirrored and is not a multiple of " +
                                                    std::to_string(m) + ": the partial MCU would land on the leading edge (JPEZY_XFORM_TRIM drops it)");
        len[k] = len[k] / m * m;
        if (!len[k])
            return set_err(JPEZY_E_BADARG, std::string(who) + ": nothing is left of the " + axis[k] + " after trimming it to a multiple of " + std::to_string(m));
    }
    g->Wt = len[0];
    g->Ht = len[1];
    g->C = (len[0] + m - 1) / m;
    g->R = (len[1] + m - 1) / m;
    g->Wout = o.swap ? len[1] : len[0];
    g->Hout = o.swap ? len[0] : len[1];
    return JPEZY_OK;
}

// the kernel on n_frames fields; everything is checked
int enqueue(const int16_t* d_in, int W, int sampling, int op, const Geometry& g, int n_frames, int16_t* d_out, size_t in_frame, size_t out_frame,
            hipStream_t s)
{
    XformParams p;
    p.in = d_in;
    p.out = d_out;
    p.in_frame = in_frame;
    p.out_frame = out_frame;
    p.blocks_per_mcu = sampling == JPEZY_SAMPLING_444 ? 3 : 6;
    p.src_pitch = sampling == JPEZY_SAMPLING_444 ? (W + 7) / 8 : (W + 15) / 16;
    p.C = g.C;
    p.R = g.R;
    p.swap = kOps[op].swap;
    p.mirror_x = kOps[op].mirror_x;
    p.mirror_y = kOps[op].mirror_y;
    p.n_frames = n_frames;
    HIP_TRY(launch_coeff_transform(p, s));
    return JPEZY_OK;
}

// Pq != 0 in a DQT segment in front of SOS (the marker parser has accepted the file; jpezy_frame_info keeps the values, not the precision)
bool has_16bit_dqt(const uint8_t* d, size_t len)
{
    size_t i = 2;
    while (i + 4 <= len && d[i] == 0xFF) {
        const unsigned mk = d[i + 1];
        if (mk == 0xFF) { ++i; continue; }
        if (mk == 0xDA) break;
        const size_t n = ((size_t)d[i + 2] << 8) | d[i + 3];
        if (mk == 0xDB)
            for (size_t j = i + 4; j < i + 2 + n && j < len;) {
                const unsigned pq = d[j] >> 4;
                if (pq) return true;
                j += 65;
            }
        i += 2 + n;
    }
    return false;
}

// what jpezy_transform_jpeg accepts: the two layouts the writer writes, with tables it can state.  *sampling, luma / chroma (natural order)
int accept_file(const uint8_t* data, size_t len, const jpezy_frame_info& info, int* sampling, uint8_t luma[64], uint8_t chroma[64])
{
    auto no = [](const std::string& why) { return set_err(JPEZY_E_UNSUPPORTED, "transform_jpeg: " + why); };
    if (info.ncomp != 3) return no("a file of " + std::to_string(info.ncomp) + " component(s): three are needed (Y, Cb, Cr)");
    if (info.precision != 8) return no("sample precision " + std::to_string(info.precision) + ": only 8-bit files");
    const bool all1 = info.H[0] == 1 && info.V[0] == 1, chroma1 = info.H[1] == 1 && info.V[1] == 1 && info.H[2] == 1 && info.V[2] == 1;
    if (chroma1 && all1) *sampling = JPEZY_SAMPLING_444;
    else if (chroma1 && info.H[0] == 2 && info.V[0] == 2) *sampling = JPEZY_SAMPLING_420;
    else
        return no("sampling factors " + std::to_string(info.H[0]) + "x" + std::to_string(info.V[0]) + ", " + std::to_string(info.H[1]) + "x" +
                  std::to_string(info.V[1]) + ", " + std::to_string(info.H[2]) + "x" + std::to_string(info.V[2]) +
                  ": only 2x2, 1x1, 1x1 (4:2:0) and 1x1, 1x1, 1x1 (4:4:4), the layouts the writer writes");
    if (has_16bit_dqt(data, len)) return no("a 16-bit DQT segment (Pq = 1): the writer states 8-bit tables");
    for (int k = 0; k < 3; ++k) {
        if (info.Tq[k] < 0 || info.Tq[k] > 3) return no("a quantiser table selector outside 0..3");
        for (int i = 0; i < 64; ++i)
            if (info.qt[info.Tq[k]][i] < 1 || info.qt[info.Tq[k]][i] > 255)
                return no("a quantiser table entry outside 1..255 (table " + std::to_string(info.Tq[k]) + ")");
    }
    if (std::memcmp(info.qt[info.Tq[1]], info.qt[info.Tq[2]], sizeof info.qt[0]))
        return no("Cb and Cr use different quantiser tables: the writer states one chroma table");
    for (int i = 0; i < 64; ++i) {
        luma[i] = (uint8_t)info.qt[info.Tq[0]][i];
        chroma[i] = (uint8_t)info.qt[info.Tq[1]][i];
    }
    return JPEZY_OK;
}

}  // namespace

extern "C" {

int jpezy_transform_geometry(int op, int flags, int W, int H, int sampling, int* Wout, int* Hout, int* src_cols, int* src_rows)
{
    if (int rc = check_op("transform_geometry", op, flags)) return rc;
    if (int rc = check_sampling("transform_geometry", sampling)) return rc;
    if (int rc = check_wh(W, H)) return rc;
    Geometry g;
    if (int rc = geometry("transform_geometry", op, flags, W, H, sampling, &g)) return rc;
    if (Wout) *Wout = g.Wout;
    if (Hout) *Hout = g.Hout;
    if (src_cols) *src_cols = g.C;
    if (src_rows) *src_rows = g.R;
    return JPEZY_OK;
}

int jpezy_quant_tables_transform(int op, const uint8_t in[64], uint8_t out[64])
{
    if (int rc = check_op("quant_tables_transform", op, 0)) return rc;
    if (!in || !out) return set_err(JPEZY_E_BADARG, "quant_tables_transform: null pointer");
    uint8_t t[64];
    for (int v = 0; v < 8; ++v)
        for (int u = 0; u < 8; ++u) t[v * 8 + u] = kOps[op].swap ? in[u * 8 + v] : in[v * 8 + u];
    std::memcpy(out, t, 64);
    return JPEZY_OK;
}

int jpezy_coeff_transform_dev(jpezy_ctx* c, const int16_t* d_in, int W, int H, int sampling, int op, int flags, int n_frames, int16_t* d_out,
                              void* stream)
{
    if (int rc = check_op("coeff_transform_dev", op, flags)) return rc;
    if (int rc = check_sampling("coeff_transform_dev", sampling)) return rc;
    if (int rc = check_wh(W, H)) return rc;
    if (n_frames <= 0) return set_err(JPEZY_E_BADARG, "coeff_transform_dev: n_frames must be positive");
    if (!d_in || !d_out) return set_err(JPEZY_E_BADARG, "coeff_transform_dev: null device pointer");
    if (!aligned16(d_in) || !aligned16(d_out)) return set_err(JPEZY_E_BADARG, "coeff_transform_dev: d_in and d_out must be 16-byte aligned");
    Geometry g;
    if (int rc = geometry("coeff_transform_dev", op, flags, W, H, sampling, &g)) return rc;
    const size_t in_frame = jpezy_coeff_count_sampling(W, H, sampling), out_frame = jpezy_coeff_count_sampling(g.Wout, g.Hout, sampling);
    const uintptr_t a0 = (uintptr_t)d_in, a1 = a0 + (size_t)n_frames * in_frame * sizeof(int16_t);
    const uintptr_t b0 = (uintptr_t)d_out, b1 = b0 + (size_t)n_frames * out_frame * sizeof(int16_t);
    if (a0 < b1 && b0 < a1) return set_err(JPEZY_E_BADARG, "coeff_transform_dev: d_in and d_out overlap (the kernel does not work in place)");
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    return enqueue(d_in, W, sampling, op, g, n_frames, d_out, in_frame, out_frame, (hipStream_t)stream);
}

long jpezy_transform_jpeg(jpezy_ctx* c, const uint8_t* data, size_t len, int op, int flags, const char* comment, jpezy_frame_info* out_info,
                          uint8_t* out, size_t cap)
try {
    if (int rc = check_op("transform_jpeg", op, flags)) return rc;
    if (!data || !len || !out_info) return set_err(JPEZY_E_BADARG, "transform_jpeg: null pointer (data, out_info) or an empty file");
    if (int rc = check_comment(comment, "transform_jpeg")) return rc;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");

    // 1. header on the host; what the file must be; where its edges go
    jpezy_frame_info info;
    if (int rc = jpezy_read_jpeg_gpu(c, data, len, &info, nullptr, 0)) return rc;
    int sampling;
    uint8_t src_qt[2][64], qt[2][64];
    if (int rc = accept_file(data, len, info, &sampling, src_qt[0], src_qt[1])) return rc;
    if (int rc = check_wh(info.width, info.height)) return rc;
    Geometry g;
    if (int rc = geometry("transform_jpeg", op, flags, info.width, info.height, sampling, &g)) return rc;
    for (int t = 0; t < 2; ++t) (void)jpezy_quant_tables_transform(op, src_qt[t], qt[t]);
    const char* text = comment ? comment : info.comment;          // NULL carries the source's COM text over, "" writes none
    if (c->restart_interval && std::strlen(text) > JPEZY_MAX_COMMENT_RESTART)
        return set_err(JPEZY_E_BADARG, "transform_jpeg: with a restart interval the comment may be at most JPEZY_MAX_COMMENT_RESTART bytes");

    // 2. the output's header fields: those of the header the writer will write (its Huffman tables are not part of them)
    {
        uint8_t hdr[1024 + 8] = { 0 };
        const size_t n = jpezy_host::write_header(g.Wout, g.Hout, text, hdr, 1024, nullptr, c->restart_interval, qt[0], qt[1], sampling);
        if (!n) return set_err(JPEZY_E_BADARG, "transform_jpeg: the writer's header does not fit (comment too long)");
        hdr[n] = 0xFF;
        hdr[n + 1] = 0xD9;
        jpezy_host::ScanSetup setup;
        std::string err;
        if (int rc = jpezy_host::parse_header(hdr, n + 2, out_info, &setup, &err)) return set_err(rc, "transform_jpeg: " + err);
    }
    if (!out) return 0;

    // 3. the scan, as jpezy_read_jpeg_gpu reads it, into c->out; 4. the kernel into the second buffer; 5. the GPU entropy coder
    if (int rc = read_coeffs(c, data, len, &info, "transform_jpeg")) return rc;
    const size_t in_frame = jpezy_coeff_count_sampling(info.width, info.height, sampling);
    const size_t out_frame = jpezy_coeff_count_sampling(g.Wout, g.Hout, sampling);
    if (int rc = c->x_coef.reserve(out_frame * sizeof(int16_t))) return rc;
    if (int rc = enqueue(c->out.as<int16_t>(), info.width, sampling, op, g, 1, c->x_coef.as<int16_t>(), in_frame, out_frame, c->stream)) return rc;
    long size = 0;
    const int rc = jpezy_internal_write_jpeg_gpu_batch(c, c->x_coef.as<int16_t>(), g.Wout, g.Hout, 0, sampling, 1, text, out, cap, &size, qt[0], qt[1]);
    if (rc != JPEZY_OK && size >= 0) return rc;
    if (size == JPEZY_E_FORMAT) set_err(JPEZY_E_FORMAT, "transform_jpeg: coefficient outside the code tables");
    if (size == JPEZY_E_NOSPACE) set_err(JPEZY_E_NOSPACE, "transform_jpeg: output buffer too small");
    return size;
}
JPEZY_CATCH

}  // extern "C"
