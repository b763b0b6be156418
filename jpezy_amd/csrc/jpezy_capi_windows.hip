// jpezy_capi_windows.hip -- the C-ABI of include/jpezy_hip.h, part 13: a batch of crop windows (one window of each of n files, sizes and
// quantiser tables mixed, packed pixels left in device memory), and part 14's entry: the same batch with every window resized to one output
// size (jpezy_decode_windows_resized_dev; one driver serves both).  Files of one LAYOUT go through the batch form of the GPU Huffman decoder
// together, whatever their sizes (a stream carries its own block count and coefficient offset), and through ONE launch of windows_kernel
// per scale present (jpezy_kernels_region.hip); what that path declines goes file by file: read_coeffs and the region stage core on a
// child context, straight into the file's slot.  Nothing is downloaded.  Resized: the same launches write a context-owned scratch of packed
// pixels, every file by its own height, and one launch of resample_kernel per slice (jpezy_kernels_resized.hip) writes the slots.  Part 15's
// entry, jpezy_decode_windows_tensor_dev, is the resized call with resample_tensor_kernel (jpezy_kernels_resized_tensor.hip) as that launch.
// With jpezy_ctx_set_windows_orientation(ctx, 1) (include/jpezy_hip_orientation.h) every file's EXIF orientation is honoured: windows are
// those of the oriented picture, the launches are given their source-side rectangles, and the files whose orientation is not 1 go out in
// an oriented launch of their own per scale.
#include "jpezy_capi_decode.h"
#include "jpezy_tensor_layout.h"

namespace {

const char* const kWho = "decode_windows_dev";
const char* const kWhoResized = "decode_windows_resized_dev";
const char* const kWhoTensor = "decode_windows_tensor_dev";

// the resized call's own arguments (null: jpezy_decode_windows_dev)
struct Resize {
    int out_w, out_h;
    const uint8_t* mirror_x;            // [n] or null
    const TensorOut* tensor;            // null: packed pixels.  Otherwise the slots are a tensor's: d_pix is its first element, slot_stride
                                        // its stride over files in ELEMENTS, row_stride is not read (jpezy_decode_windows_tensor_dev)
    // filled in by windows_driver from the context the call was made on, so that a child context resamples as its parent would
    ResampleHow how = {};               // the filter (jpezy_ctx_set_windows_filter) and the direct-loop knob
    std::atomic<int>* tiled = nullptr;  // files that took the two-pass tile, counted over the call's launches
};

inline size_t up4(size_t v) { return (v + 3) & ~(size_t)3; }

// the window as it will be decoded (whole-picture form resolved), inside the picture, fitting its slot (fit: the resized call's windows
// have no slot of their own size to fit); W, H, bytes already checked
int resolve_window(const char* who, int W, int H, const jpezy_window* win, int bytes, size_t row_stride, size_t slot_stride, jpezy_rect* placed,
                   bool fit = true)
{
    const int scale = win ? win->scale_denom : 1;
    if (log2n_of(scale) < 0) return bad_scale(who);
    jpezy_rect r = win ? win->region : jpezy_rect{ 0, 0, 0, 0 };
    if (r.w == 0 && r.h == 0) {                    // the whole picture at that scale (x, y are not looked at)
        r.x = r.y = 0;
        (void)jpezy_scaled_size(W, H, scale, &r.w, &r.h);
    }
    if (int rc = region_inside(who, W, H, scale, &r)) return rc;
    if (placed) *placed = r;
    if (!fit) return JPEZY_OK;
    const size_t tight = (size_t)r.w * (size_t)bytes;
    if (tight > row_stride || (size_t)(r.h - 1) * row_stride + tight > slot_stride)
        return set_err(JPEZY_E_NOSPACE, std::string(who) + ": a window of " + std::to_string(r.w) + " x " + std::to_string(r.h) + " pixels of " +
                                            std::to_string(bytes) + " bytes does not fit a slot of " + std::to_string(slot_stride) +
                                            " bytes with rows " + std::to_string(row_stride) + " apart");
    return JPEZY_OK;
}

struct Cand {
    jpezy_host::ScanSetup setup;
    const uint8_t* scan = nullptr;      // grouped path: the file from its first scan byte
    size_t n = 0;
    size_t nblk = 0;                    // blocks of the whole file
    jpezy_rect rect = { 0, 0, 0, 0 };     // the window as placed: with the orientation setting on, in the ORIENTED picture's coordinates
    jpezy_rect src = { 0, 0, 0, 0 };      // ... and the rectangle of the decoded picture it shows (jpezy_orient_rect); rect itself otherwise
    int orient = 1;                     // the file's orientation as applied: 1 with the setting off
    int log2n = 3;
    int st = JPEZY_OK;                  // < 0: decided before any device work
    bool parsed = false, good = false;  // good: the grouped path takes it
    std::string msg;
};

bool same_layout(const jpezy_frame_info& x, const jpezy_frame_info& y)
{
    if (x.ncomp != y.ncomp || x.precision != y.precision) return false;
    for (int q = 0; q < x.ncomp; ++q)
        if (x.H[q] != y.H[q] || x.V[q] != y.V[q]) return false;
    return true;
}

bool same_tables(const jpezy_host::ScanSetup& a, const jpezy_host::ScanSetup& b0)
{
    if (std::memcmp(a.Td, b0.Td, sizeof a.Td) || std::memcmp(a.present, b0.present, sizeof a.present) || std::memcmp(a.bits, b0.bits, sizeof a.bits)) return false;
    for (int t = 0; t < 8; ++t)
        if (a.present[t] && (a.nvals[t] != b0.nvals[t] || std::memcmp(a.vals[t], b0.vals[t], (size_t)a.nvals[t]))) return false;
    return true;
}

// the dequantisers of the file's (up to) three components, natural order: what jpezy_internal_upload_dequant puts into d_dqt
void dequant_set(const jpezy_frame_info& fi, int out[192])
{
    for (int k = 0; k < 3; ++k) {
        const int t = (k < fi.ncomp ? fi.Tq[k] : 0) & 3;
        for (int i = 0; i < 64; ++i) out[k * 64 + i] = fi.qt[t][i];
    }
}

struct SliceOut {
    size_t row_stride, slot_stride;
    uint8_t* d_pix;
    int bytes, swap_rb, gray;
    const Resize* rz;
    int smooth;                         // the context's windows upsampling: windows_smooth_kernel in windows_kernel's place
};

// One slice of a group (one layout; sizes, windows, scales and tables mixed): the Huffman decoding of all files in one sequence of
// launches, then one windows_kernel launch per scale present over the files that settled.  ok[k] = 1 for those; the others are left to
// the per-file path, whose verdict is the authoritative one.  Resized (out.rz): the launches write c->w_scr, rows the slice's widest window
// (rounded up to 4 bytes) apart, every file's rows behind the file before; one resample_kernel launch then fills the slots.
int decode_slice(jpezy_ctx* c, const std::vector<int>& files, const std::vector<Cand>& all, const jpezy_frame_info* info, const SliceOut& out,
                 std::vector<char>& ok)
{
    namespace HD = jpezy_dev::huffdec;
    hipStream_t s = c->stream;
    const unsigned nf = (unsigned)files.size();
    const jpezy_frame_info& gi = info[files[0]];
    ok.assign(nf, 0);
    const bool dbg = std::getenv("JPEZY_BATCH_DEBUG") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_mark = now();
    auto lap = [&](const char* what) {
        if (!dbg) return;
        (void)hipStreamSynchronize(s);
        const double t = now();
        std::fprintf(stderr, "  windows slice (%u files): %-28s %.3f ms\n", nf, what, (t - t_mark) * 1e3);
        t_mark = t;
    };
    // Device Huffman tables once per DISTINCT set of tables.  Setup::total_blocks is read by the single-stream emit_kernel alone: every
    // kernel this call can reach (speculate / sync / emit / DC of the batch form, the lane-per-stream kernel) takes the stream's own count
    // from BatchFile, so files of different sizes share a Setup and the sharing is keyed on the tables only.
    std::vector<DevStream> streams(nf);
    std::vector<HD::Setup> setups;
    std::vector<char> setup_usable;
    std::vector<unsigned> first_with;
    size_t coef_elems = 0;
    bool small = nf > 1;
    for (unsigned k = 0; k < nf; ++k) {
        const Cand& cd = all[(size_t)files[k]];
        unsigned j = (unsigned)first_with.size();
        for (unsigned q = (unsigned)first_with.size(); q-- > 0;)
            if (same_tables(cd.setup, all[(size_t)files[first_with[q]]].setup)) { j = q; break; }
        if (j == first_with.size()) {
            setups.emplace_back();
            setup_usable.push_back(jpezy_internal_build_dev_setup(setups.back(), cd.setup, info[files[k]], (unsigned)cd.nblk) ? 1 : 0);
            if (first_with.size() < 64) first_with.push_back(k);
            j = (unsigned)setups.size() - 1;
        }
        streams[k] = { cd.scan, cd.n, (unsigned)cd.nblk, (unsigned long long)coef_elems, j };
        coef_elems += (cd.nblk * 64 + 7) & ~(size_t)7;                  // whole files, 16-byte aligned
        small = small && cd.n <= 4096;
    }
    const bool per_lane = small && setups.size() == 1;
    if (int rc = c->b_coef.reserve(coef_elems * sizeof(int16_t))) return rc;
    if (int rc = jpezy_internal_huffdec_streams(c, streams, setups, setup_usable, jpezy_internal_stream_geom(gi), (int16_t*)c->b_coef.p, coef_elems, ok, lap, per_lane)) return rc;

    // resized: where the windows go in the scratch
    std::vector<unsigned long long> scr_off(nf, 0);
    size_t scr_stride = 0;
    if (out.rz) {
        size_t wmax = 0, rows = 0;
        for (unsigned k = 0; k < nf; ++k)
            if (ok[k]) wmax = std::max(wmax, (size_t)all[(size_t)files[k]].rect.w);
        scr_stride = up4(wmax * (size_t)out.bytes);
        for (unsigned k = 0; k < nf; ++k) {
            if (!ok[k]) continue;
            scr_off[k] = (unsigned long long)rows * scr_stride;
            rows += (size_t)all[(size_t)files[k]].rect.h;
        }
        if (rows)
            if (int rc = c->w_scr.reserve(rows * scr_stride)) return rc;
    }

    // descriptor tables: one per launch (a scale; a second one for a scale whose workgroups would not fit 32 bits), the dequantiser sets
    // de-duplicated in front of them -- built in the context's pinned staging, one upload
    // (with the orientation setting on: files whose orientation is 1 keep the un-oriented launch, the others share an oriented one)
    struct Launch { int log2n; bool oriented; unsigned long long total; std::vector<WindowDesc> desc; };
    std::vector<Launch> launches;
    std::vector<int> qsets;                                           // [sets][192]
    for (unsigned k = 0; k < nf; ++k) {
        if (!ok[k]) continue;
        const int i = files[k];
        const Cand& cd = all[(size_t)i];
        int q[192];
        dequant_set(info[i], q);
        size_t qs = qsets.size() / 192;
        for (size_t t = qsets.size() / 192; t-- > 0;)
            if (!std::memcmp(&qsets[t * 192], q, sizeof q)) { qs = t; break; }
        if (qs == qsets.size() / 192) qsets.insert(qsets.end(), q, q + 192);
        const int mw = info[i].hmax << cd.log2n, mh = info[i].vmax << cd.log2n;       // an MCU of the picture at this scale
        WindowDesc d;
        std::memset(&d, 0, sizeof d);
        d.coeff_off = streams[k].coeff_off;
        d.out_off = out.rz ? scr_off[k] : (unsigned long long)i * out.slot_stride;
        const bool oriented = cd.orient != 1;
        d.qset = (int)qs | (oriented ? jpezy_exif::orient_bits(cd.orient) << kWindowOrientShift : 0);      // (qs < 512: a set per file at most)
        d.mcu_cols = info[i].mcu_cols;
        // the kernel's rectangle is the source-side one (the window itself when un-oriented); so are the MCUs
        const jpezy_rect& sr = cd.src;
        d.x = sr.x; d.y = sr.y; d.w = sr.w; d.h = sr.h;
        d.ux0 = sr.x / mw; d.ucols = (sr.x + sr.w - 1) / mw - d.ux0 + 1;
        d.uy0 = sr.y / mh;
        if (out.smooth) {               // the picture at this scale: the extent of the smoothed components' planes (inside the file's MCU grid)
            int Ws, Hs;
            (void)jpezy_scaled_size(info[i].width, info[i].height, 8 >> cd.log2n, &Ws, &Hs);
            if (Ws > info[i].mcu_cols * mw || Hs > info[i].mcu_rows * mh) { ok[k] = 0; continue; }      // (no header gives this: left to the per-file path)
            d.pad[0] = (unsigned)Ws; d.pad[1] = (unsigned)Hs;
        }
        const unsigned long long wgs = (unsigned long long)d.ucols * (unsigned long long)((sr.y + sr.h - 1) / mh - d.uy0 + 1);
        Launch* L = nullptr;
        for (Launch& l : launches)
            if (l.log2n == cd.log2n && l.oriented == oriented && l.total + wgs <= 0xFFFFFFFFull) L = &l;
        if (!L) { launches.push_back({ cd.log2n, oriented, 0, {} }); L = &launches.back(); }
        d.wg0 = (unsigned)L->total;
        L->total += wgs;
        L->desc.push_back(d);
    }
    if (launches.empty()) return JPEZY_OK;
    size_t bytes = qsets.size() * sizeof(int);                        // (a multiple of 64)
    for (const Launch& l : launches) bytes += l.desc.size() * sizeof(WindowDesc);
    if (int rc = c->w_pin.reserve(bytes, bytes + (bytes >> 2))) return rc;
    if (int rc = c->w_tab.reserve(bytes)) return rc;
    std::memcpy(c->w_pin.p, qsets.data(), qsets.size() * sizeof(int));
    size_t at = qsets.size() * sizeof(int);
    std::vector<size_t> desc_at;
    for (const Launch& l : launches) {
        std::memcpy(c->w_pin.p + at, l.desc.data(), l.desc.size() * sizeof(WindowDesc));
        desc_at.push_back(at);
        at += l.desc.size() * sizeof(WindowDesc);
    }
    HIP_TRY(hipMemcpyAsync(c->w_tab.p, c->w_pin.p, bytes, hipMemcpyHostToDevice, s));
    WindowsParams p;
    std::memset(&p, 0, sizeof p);
    {
        // the layout's geometry through the one function the stage cores use (the sizes it derives are not read here)
        RegionDecParams g;
        const DecodeSource src = DecodeSource::file((const int16_t*)c->b_coef.p, gi, out.gray);
        if (int rc = decode_geometry(c, src, DecodeSink::planes(nullptr, nullptr, nullptr, 0), &g)) return rc;
        p.ncomp = g.ncomp; p.gray = g.gray; p.level = g.level; p.hmax = g.hmax; p.vmax = g.vmax; p.blocks_per_mcu = g.blocks_per_mcu;
        for (int k = 0; k < 3; ++k) { p.ch[k] = g.ch[k]; p.cv[k] = g.cv[k]; p.blk_start[k] = g.blk_start[k]; }
    }
    p.coeffs = (const int16_t*)c->b_coef.p;
    p.qsets = (const int*)c->w_tab.p;
    p.pix = out.rz ? (uint8_t*)c->w_scr.p : out.d_pix;
    p.row_stride = out.rz ? scr_stride : out.row_stride;
    p.pix_bytes = out.bytes; p.swap_rb = out.swap_rb;
    Event ev0, ev1;                                                   // JPEZY_BATCH_DEBUG: the kernel's own time, from device events
    if (dbg) {
        HIP_TRY(ev0.create(hipEventDefault));
        HIP_TRY(ev1.create(hipEventDefault));
    }
    for (size_t l = 0; l < launches.size(); ++l) {
        p.log2n = launches[l].log2n;
        p.desc = (const WindowDesc*)((const uint8_t*)c->w_tab.p + desc_at[l]);
        p.n_desc = (unsigned)launches[l].desc.size();
        if (dbg) HIP_TRY(hipEventRecord(ev0, s));
        HIP_TRY(out.smooth ? launch_dequant_idct_windows_smooth(p, launches[l].total, s, launches[l].oriented)
                           : launch_dequant_idct_windows(p, launches[l].total, s, launches[l].oriented));
        if (dbg) {
            float ms = 0;
            HIP_TRY(hipEventRecord(ev1, s));
            HIP_TRY(hipEventSynchronize(ev1));
            HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
            std::fprintf(stderr, "  windows slice (%u files): %s<%d%s>, %u files, %llu workgroups: %.3f ms (device events)\n", nf,
                         out.smooth ? "windows_smooth_kernel" : "windows_kernel", 1 << p.log2n, launches[l].oriented ? ", oriented" : "", p.n_desc,
                         launches[l].total, (double)ms);
        }
    }
    if (out.rz) {
        lap("windows transform");
        std::vector<ResampleJob> jobs;
        for (unsigned k = 0; k < nf; ++k) {
            if (!ok[k]) continue;
            const int i = files[k];
            const jpezy_rect& r = all[(size_t)i].rect;
            jobs.push_back({ scr_off[k], (unsigned long long)i * out.slot_stride, r.w, r.h, out.rz->mirror_x && out.rz->mirror_x[i] ? 1 : 0 });
        }
        int tiled = 0;
        if (int rc = jpezy_internal_resample(c, jobs, (const uint8_t*)c->w_scr.p, (unsigned)scr_stride, out.d_pix, out.row_stride, out.rz->out_w,
                                             out.rz->out_h, out.bytes, s, out.rz->how, &tiled, dbg ? (hipEvent_t)ev0 : nullptr,
                                             dbg ? (hipEvent_t)ev1 : nullptr, out.rz->tensor))
            return rc;
        out.rz->tiled->fetch_add(tiled);
        if (dbg) {
            float ms = 0;
            HIP_TRY(hipEventSynchronize(ev1));
            HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
            std::fprintf(stderr, "  windows slice (%u files): tables up + %s<%d>, filter %d, %d of %zu files tiled, to %d x %d: %.3f ms (device events)\n", nf,
                         out.rz->tensor ? "resample_tensor_kernel" : "resample_kernel", out.rz->tensor ? out.rz->tensor->dtype : out.bytes,
                         out.rz->how.filter, tiled, jobs.size(), out.rz->out_w, out.rz->out_h, (double)ms);
        }
    }
    HIP_TRY(hipStreamSynchronize(s));                                 // (the pinned staging is the next slice's; the call is synchronous anyway)
    lap(out.rz ? "resample" : "windows transform");
    return JPEZY_OK;
}

}  // namespace

extern "C" {

int jpezy_window_fit(int W, int H, const jpezy_window* win, int format, size_t row_stride, size_t slot_stride, jpezy_rect* placed)
{
    const char* who = "window_fit";
    const int bytes = jpezy_pixel_bytes(format);
    if (bytes < 0) return set_err(JPEZY_E_BADARG, std::string(who) + ": unknown pixel format");
    if (W <= 0 || H <= 0) return set_err(JPEZY_E_BADARG, std::string(who) + ": width and height must be positive");
    return resolve_window(who, W, H, win, bytes, row_stride, slot_stride, placed);
}

int jpezy_ctx_set_windows_slice_files(jpezy_ctx* c, int n)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (n < 0 || n > kWindowMaxFiles) return set_err(JPEZY_E_BADARG, "windows_slice_files must be 0 (automatic) or 1..512");
    c->w_slice_files = n;
    return JPEZY_OK;
}

int jpezy_ctx_set_windows_upsampling(jpezy_ctx* c, int upsampling)
{
    if (upsampling != JPEZY_UPSAMPLE_NEAREST && upsampling != JPEZY_UPSAMPLE_SMOOTH)
        return set_err(JPEZY_E_BADARG, "windows_upsampling: upsampling must be JPEZY_UPSAMPLE_NEAREST or JPEZY_UPSAMPLE_SMOOTH");
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    c->w_upsampling = upsampling;
    return JPEZY_OK;
}

int jpezy_ctx_windows_upsampling(jpezy_ctx* c)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    return c->w_upsampling;
}

int jpezy_ctx_set_windows_orientation(jpezy_ctx* c, int mode)
{
    if (mode != 0 && mode != 1) return set_err(JPEZY_E_BADARG, "windows_orientation: mode must be 0 (ignore the tag) or 1 (honour every file's own)");
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    c->w_orientation = mode;
    return JPEZY_OK;
}

int jpezy_ctx_windows_orientation(jpezy_ctx* c)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    return c->w_orientation;
}

int jpezy_ctx_set_windows_filter(jpezy_ctx* c, int filter)
{
    if (filter != JPEZY_FILTER_BILINEAR && filter != JPEZY_FILTER_BOX && filter != JPEZY_FILTER_BICUBIC && filter != JPEZY_FILTER_LANCZOS)
        return set_err(JPEZY_E_BADARG, "windows_filter: filter must be one of JPEZY_FILTER_*");
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    c->w_filter = filter;
    return JPEZY_OK;
}

int jpezy_ctx_windows_filter(jpezy_ctx* c)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    return c->w_filter;
}

int jpezy_ctx_set_resample_direct(jpezy_ctx* c, int on)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    c->r_direct = on ? 1 : 0;
    return JPEZY_OK;
}

int jpezy_ctx_last_resample_tiled_count(jpezy_ctx* c)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    return c->r_last_tiled;
}

}  // extern "C"

namespace {

// The driver of both entries, behind their own argument checks (n >= 1, arrays, format, strides, capacity): headers and windows, the grouped
// path slice by slice, the per-file path, the verdict.  rz null: every window into its slot as it is (jpezy_decode_windows_dev); otherwise
// every window resampled to rz->out_w x rz->out_h (jpezy_decode_windows_resized_dev; with rz->tensor into a tensor,
// jpezy_decode_windows_tensor_dev).
int windows_driver(jpezy_ctx* c, const char* who_c, int n, const uint8_t* const* data, const size_t* len, int gray, const jpezy_window* windows,
                   int format, int bytes, size_t row_stride, size_t slot_stride, uint8_t* d_pix, jpezy_frame_info* info, jpezy_rect* placed,
                   int* status, const Resize* rz_call)
{
    const std::string who = who_c;
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    std::atomic<int> tiled{ 0 };
    Resize rz_ctx;
    if (rz_call) {
        rz_ctx = *rz_call;
        rz_ctx.how = { c->w_filter, c->r_direct };
        rz_ctx.tiled = &tiled;
        c->r_last_tiled = 0;
    }
    const Resize* const rz = rz_call ? &rz_ctx : nullptr;
    HIP_TRY(hipSetDevice(c->device));
    {
        hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(c->stream, &st) == hipSuccess && st != hipStreamCaptureStatusNone)
            return set_err(JPEZY_E_BADARG, who + ": the call is synchronous and cannot run inside a stream capture");
    }
    c->b_last_fast = 0;
    const int smooth = c->w_upsampling == JPEZY_UPSAMPLE_SMOOTH ? 1 : 0;
    const bool honour_tag = c->w_orientation != 0;      // read once, here: a child context decodes what the call's context decided
    const bool blue_first = format == JPEZY_PIX_BGR24 || format == JPEZY_PIX_BGRA32;
    std::vector<Cand> all((size_t)n);
    std::vector<char> done((size_t)n, 0);

    // ---- headers and windows, spread over host threads ----
    auto prep = [&](int i) {
        Cand& cd = all[(size_t)i];
        std::memset(&info[i], 0, sizeof info[i]);
        if (placed) placed[i] = { 0, 0, 0, 0 };
        if (!data[i]) { cd.st = JPEZY_E_BADARG; cd.msg = "null file"; return; }
        std::string err;
        if (int rc = jpezy_host::parse_header(data[i], len[i], &info[i], &cd.setup, &err); rc < 0) { cd.st = rc; cd.msg = err; return; }
        cd.parsed = true;
        const jpezy_frame_info& fi = info[i];
        if (int rc = check_wh(fi.width, fi.height)) { cd.st = rc; cd.msg = g_err; return; }
        if (smooth)                     // this file alone: its slot stays untouched, the others are decoded
            if (int mode = upsampling_mode(who_c, JPEZY_UPSAMPLE_SMOOTH, fi.precision); mode < 0) { cd.st = mode; cd.msg = g_err; return; }
        const jpezy_window* win = windows ? &windows[i] : nullptr;
        // the file's tag, parsed once; the window is then one of the oriented picture, whose size is the file's with the axes swapped for
        // the transposed orientations
        cd.orient = honour_tag ? jpezy_exif::jpeg_orientation(data[i], len[i]) : 1;
        int Wo, Ho;
        oriented_wh(cd.orient, fi.width, fi.height, &Wo, &Ho);
        const int fit = resolve_window(who_c, Wo, Ho, win, bytes, row_stride, slot_stride, &cd.rect, rz == nullptr);
        if (placed && (fit == JPEZY_OK || fit == JPEZY_E_NOSPACE)) placed[i] = cd.rect;       // (a window inside the picture is reported, fitting or not)
        if (fit) { cd.st = fit; cd.msg = g_err; return; }
        cd.log2n = log2n_of(win ? win->scale_denom : 1);
        {
            int Ws, Hs;
            (void)jpezy_scaled_size(fi.width, fi.height, 8 >> cd.log2n, &Ws, &Hs);
            const jpezy_exif::Rect sr = jpezy_exif::orient_rect(cd.orient, Ws, Hs, { cd.rect.x, cd.rect.y, cd.rect.w, cd.rect.h });
            cd.src = { sr.x, sr.y, sr.w, sr.h };
        }
        // what the grouped path takes: jpezy_decode_jpeg_batch's rule -- every baseline layout decode_mcu handles (1 or 3 components,
        // sampling factors 1..4, at most 48 blocks per MCU), tables present, no restart interval, the scan bounds
        bool fits = (fi.ncomp == 1 || fi.ncomp == 3) && fi.restart_interval == 0 && fi.blocks_per_mcu >= 1 && fi.blocks_per_mcu <= 48;
        for (int q = 0; q < fi.ncomp && fits; ++q) fits = fi.H[q] >= 1 && fi.H[q] <= 4 && fi.V[q] >= 1 && fi.V[q] <= 4;
        if (!fits || cd.setup.scan_pos >= len[i]) return;
        for (int q = 0; q < fi.ncomp; ++q)
            if (!(cd.setup.Td[q] >= 0 && cd.setup.Td[q] <= 2 && cd.setup.present[cd.setup.Td[q]] && cd.setup.present[4 + cd.setup.Td[q]])) return;
        size_t ns = len[i] - cd.setup.scan_pos;
        const size_t nblk = (size_t)fi.mcu_cols * fi.mcu_rows * (size_t)fi.blocks_per_mcu;
        if (ns == 0 || nblk > 4 * len[i] || nblk >= 0xFFFFFFFFull) return;
        ns = std::min(ns, nblk * 432 + 4096);          // a long tail behind the scan is not uploaded (see jpezy_read_jpeg_gpu)
        if (ns >= 0xFFFFFFFFull) return;
        cd.scan = data[i] + cd.setup.scan_pos; cd.n = ns; cd.nblk = nblk;
        cd.good = true;
    };
    const auto t_head = std::chrono::steady_clock::now();
    {
        unsigned hwp = std::thread::hardware_concurrency();
        const int nt = (int)std::max(1u, std::min<unsigned>(std::min<unsigned>(hwp ? hwp : 4u, 8u), (unsigned)(n + 15) / 16));
        std::atomic<int> next{ 0 };
        auto work = [&] { for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) prep(i); };
        Joiner pool;
        for (int t = 1; t < nt; ++t) pool.start(work);
        work();
    }
    if (std::getenv("JPEZY_BATCH_DEBUG"))
        std::fprintf(stderr, "  windows (%d files): %-28s %.3f ms\n", n, "headers + windows", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_head).count() * 1e3);

    // ---- the grouped path: by layout only; a group of one as well (no child context is needed for it, and one rule decides the path) ----
    const SliceOut out = { row_stride, slot_stride, d_pix, bytes, blue_first ? 1 : 0, gray, rz, smooth };
    std::vector<char> taken((size_t)n, 0);
    for (int a = 0; a < n; ++a) {
        if (taken[(size_t)a] || !all[(size_t)a].good) continue;
        std::vector<int> grp;
        for (int k = a; k < n; ++k)
            if (!taken[(size_t)k] && all[(size_t)k].good && same_layout(info[a], info[k])) { taken[(size_t)k] = 1; grp.push_back(k); }
        // slices: coefficients (2 bytes each), the scan and the decoder's scratch over it (the scan, its unstuffed copy, 20 bytes of state
        // per subsequence: below 4 bytes per scan byte) stay under ~1.5 GB, at most 512 files (jpezy_ctx_set_windows_slice_files: a fixed count).
        // Resized: the scratch of the slice's windows (rows of its widest window, the sum of their heights) counts against the same bound
        const size_t max_files = c->w_slice_files > 0 ? (size_t)c->w_slice_files : (size_t)kWindowMaxFiles;
        for (size_t s0 = 0; s0 < grp.size();) {
            std::vector<int> slice;
            size_t mem = 0, wmax = 0, rows = 0;
            while (s0 < grp.size() && slice.size() < max_files) {
                const Cand& cd = all[(size_t)grp[s0]];
                const size_t need = cd.nblk * 128 + cd.n * 4 + 4096;
                const size_t wm = rz ? std::max(wmax, (size_t)cd.rect.w) : 0, rw = rz ? rows + (size_t)cd.rect.h : 0;
                if (!slice.empty() && mem + need + up4(wm * (size_t)bytes) * rw > ((size_t)3 << 29)) break;
                mem += need; wmax = wm; rows = rw;
                slice.push_back(grp[s0++]);
            }
            std::vector<char> okv;
            if (decode_slice(c, slice, all, info, out, okv) != JPEZY_OK) continue;          // (the per-file path reports what is wrong)
            for (size_t k = 0; k < slice.size(); ++k)
                if (okv[k]) { done[(size_t)slice[k]] = 1; status[slice[k]] = JPEZY_OK; ++c->b_last_fast; }
        }
    }

    // ---- everything else file by file on the child contexts: restart intervals, streams that did not settle, irregular streams ----
    std::vector<int> rest;
    for (int i = 0; i < n; ++i) {
        if (all[(size_t)i].st < 0) status[i] = all[(size_t)i].st;
        else if (!done[(size_t)i]) rest.push_back(i);
    }
    if (!rest.empty()) {
        unsigned hw = std::thread::hardware_concurrency();
        if (hw == 0) hw = 4;
        const int nw = (int)std::min<unsigned>(std::min<unsigned>((unsigned)rest.size(), hw), 8u);
        while ((int)c->workers.size() < nw) {
            jpezy_ctx* w = jpezy_ctx_create(c->device);
            if (!w) return JPEZY_E_HIP;                                  // message set by jpezy_ctx_create
            w->is_batch_child = true;
            c->workers.push_back(w);
        }
        for (int k = 0; k < nw; ++k) {                                   // the definition has no inexact path: tolerance off, whatever the parent says
            c->workers[(size_t)k]->h_min_bytes = c->h_min_bytes;
            c->workers[(size_t)k]->dec_tolerance = 0;
            c->workers[(size_t)k]->force_exact = 0;
        }
        auto one = [&](jpezy_ctx* w, int i) -> int {
            const Cand& cd = all[(size_t)i];
            if (int rc = read_coeffs(w, data[i], len[i], &info[i], who_c)) return rc;
            // resized: the window into the child's scratch, rows rounded up to 4 bytes, then the one-entry form of the second stage
            const size_t scr_stride = up4((size_t)cd.rect.w * (size_t)bytes);
            if (rz)
                if (int rc = w->w_scr.reserve(scr_stride * (size_t)cd.rect.h)) return rc;
            const PackedLayout L = { bytes, { blue_first ? 2 : 0, 1, blue_first ? 0 : 2 }, rz ? scr_stride : row_stride, 0 };
            // the region stage core, for a whole picture too (the full window): the defined arithmetic, straight into the slot
            if (int rc = jpezy_internal_region_dev_core(w, DecodeSource::file((const int16_t*)w->out.p, info[i], gray),
                                                        DecodeSink::packed(L, rz ? (uint8_t*)w->w_scr.p : d_pix + (size_t)i * slot_stride), w->stream,
                                                        cd.log2n, cd.rect, smooth, cd.orient))
                return rc;
            if (rz) {
                const std::vector<ResampleJob> job = { { 0, (unsigned long long)i * slot_stride, cd.rect.w, cd.rect.h, rz->mirror_x && rz->mirror_x[i] ? 1 : 0 } };
                int n_tiled = 0;                                         // the parent's filter, not the child's own setting
                if (int rc = jpezy_internal_resample(w, job, (const uint8_t*)w->w_scr.p, (unsigned)scr_stride, d_pix, row_stride, rz->out_w, rz->out_h, bytes,
                                                     w->stream, rz->how, &n_tiled, nullptr, nullptr, rz->tensor))
                    return rc;
                tiled.fetch_add(n_tiled);
            }
            HIP_TRY(hipStreamSynchronize(w->stream));
            return JPEZY_OK;
        };
        auto work = [&](int k) {
            for (size_t q = (size_t)k; q < rest.size(); q += (size_t)nw) {
                const int i = rest[q];
                status[i] = one(c->workers[(size_t)k], i);
                if (status[i] < 0) all[(size_t)i].msg = g_err;           // this thread's message
            }
        };
        Joiner pool;
        for (int k = 1; k < nw; ++k) pool.start(work, k);
        work(0);
    }
    if (rz) c->r_last_tiled = tiled.load();
    for (int i = 0; i < n; ++i)
        if (status[i] < 0) return set_err(status[i], who + ": file " + std::to_string(i) + ": " + all[(size_t)i].msg);
    return JPEZY_OK;
}

}  // namespace

extern "C" {

int jpezy_decode_windows_dev(jpezy_ctx* c, int n, const uint8_t* const* data, const size_t* len, int gray, const jpezy_window* windows, int format,
                             size_t row_stride, size_t slot_stride, uint8_t* d_pix, size_t pix_cap, jpezy_frame_info* info, jpezy_rect* placed,
                             int* status)
try {
    const std::string who = kWho;
    // what needs no device, before the context is looked at
    if (n < 0) return set_err(JPEZY_E_BADARG, who + ": n must not be negative");
    if (n == 0) return JPEZY_OK;
    if (!data || !len || !info || !status || !d_pix) return set_err(JPEZY_E_BADARG, who + ": null pointer");
    const int bytes = jpezy_pixel_bytes(format);
    if (bytes < 0) return set_err(JPEZY_E_BADARG, who + ": unknown pixel format");
    if (row_stride == 0 || slot_stride == 0)
        return set_err(JPEZY_E_BADARG, who + ": row_stride and slot_stride must be given (windows differ in size: there is no 0 = tight)");
    if (row_stride > 0xFFFFFFFFull) return set_err(JPEZY_E_BADARG, who + ": row_stride must fit in 32 bits");
    if (slot_stride > pix_cap / (size_t)n) return set_err(JPEZY_E_NOSPACE, who + ": n * slot_stride exceeds pix_cap");
    return windows_driver(c, kWho, n, data, len, gray, windows, format, bytes, row_stride, slot_stride, d_pix, info, placed, status, nullptr);
}
JPEZY_CATCH

int jpezy_decode_windows_resized_dev(jpezy_ctx* c, int n, const uint8_t* const* data, const size_t* len, int gray, const jpezy_window* windows,
                                     const uint8_t* mirror_x, int out_w, int out_h, int format, size_t row_stride, size_t slot_stride,
                                     uint8_t* d_pix, size_t pix_cap, jpezy_frame_info* info, jpezy_rect* placed, int* status)
try {
    const std::string who = kWhoResized;
    // what needs no device, before the context is looked at
    if (n < 0) return set_err(JPEZY_E_BADARG, who + ": n must not be negative");
    if (n == 0) return JPEZY_OK;
    if (!data || !len || !info || !status || !d_pix) return set_err(JPEZY_E_BADARG, who + ": null pointer");
    const int bytes = jpezy_pixel_bytes(format);
    if (bytes < 0) return set_err(JPEZY_E_BADARG, who + ": unknown pixel format");
    if (out_w < 1 || out_h < 1 || out_w > 65535 || out_h > 65535) return set_err(JPEZY_E_BADARG, who + ": out_w and out_h must be in 1..65535");
    const size_t tight = (size_t)out_w * (size_t)bytes;
    if (row_stride == 0) row_stride = tight;
    if (row_stride > 0xFFFFFFFFull) return set_err(JPEZY_E_BADARG, who + ": row_stride must fit in 32 bits");
    if (row_stride < tight) return set_err(JPEZY_E_BADARG, who + ": row_stride smaller than out_w * bytes per pixel");
    if (slot_stride == 0) slot_stride = (size_t)out_h * row_stride;
    if (slot_stride < (size_t)(out_h - 1) * row_stride + tight)
        return set_err(JPEZY_E_NOSPACE, who + ": an output of " + std::to_string(out_w) + " x " + std::to_string(out_h) + " pixels of " + std::to_string(bytes) +
                                            " bytes does not fit a slot of " + std::to_string(slot_stride) + " bytes with rows " +
                                            std::to_string(row_stride) + " apart");
    if (slot_stride > pix_cap / (size_t)n) return set_err(JPEZY_E_NOSPACE, who + ": n * slot_stride exceeds pix_cap");
    const Resize rz = { out_w, out_h, mirror_x, nullptr, {}, nullptr };
    return windows_driver(c, kWhoResized, n, data, len, gray, windows, format, bytes, row_stride, slot_stride, d_pix, info, placed, status, &rz);
}
JPEZY_CATCH

int jpezy_decode_windows_tensor_dev(jpezy_ctx* c, int n, const uint8_t* const* data, const size_t* len, int gray, const jpezy_window* windows,
                                    const uint8_t* mirror_x, int out_w, int out_h, int format, int dtype, int channels, const float* scale,
                                    const float* bias, int64_t sn, int64_t sc, int64_t sh, int64_t sw, void* d_out, size_t cap_elems,
                                    jpezy_frame_info* info, jpezy_rect* placed, int* status)
try {
    const std::string who = kWhoTensor;
    // what needs no device, before the context is looked at, in the order include/jpezy_hip.h documents
    if (n < 0) return set_err(JPEZY_E_BADARG, who + ": n must not be negative");
    if (n == 0) return JPEZY_OK;
    if (!data || !len || !info || !status || !d_out) return set_err(JPEZY_E_BADARG, who + ": null pointer");
    const int bytes = jpezy_pixel_bytes(format);
    if (bytes < 0) return set_err(JPEZY_E_BADARG, who + ": unknown pixel format");
    if (bytes != 3) return set_err(JPEZY_E_BADARG, who + ": the pixel format must be JPEZY_PIX_RGB24 or JPEZY_PIX_BGR24 (alpha is never a tensor channel)");
    if (out_w < 1 || out_h < 1 || out_w > 65535 || out_h > 65535) return set_err(JPEZY_E_BADARG, who + ": out_w and out_h must be in 1..65535");
    if (channels != 3 && channels != 1) return set_err(JPEZY_E_BADARG, who + ": channels must be 3 or 1");
    if (channels == 1 && !gray) return set_err(JPEZY_E_BADARG, who + ": channels == 1 needs gray != 0");
    if (dtype != JPEZY_DT_U8 && dtype != JPEZY_DT_F32 && dtype != JPEZY_DT_F16 && dtype != JPEZY_DT_BF16)
        return set_err(JPEZY_E_BADARG, who + ": unknown element type (dtype must be one of JPEZY_DT_*)");
    if (!scale != !bias) return set_err(JPEZY_E_BADARG, who + ": scale and bias are given together or not at all");
    if (dtype == JPEZY_DT_U8 && scale) return set_err(JPEZY_E_BADARG, who + ": JPEZY_DT_U8 takes no scale and bias");
    static_assert(JPEZY_DT_U8 == kTensorU8 && JPEZY_DT_F32 == kTensorF32 && JPEZY_DT_F16 == kTensorF16 && JPEZY_DT_BF16 == kTensorBF16, "TensorOut::dtype");
    TensorOut t;
    std::memset(&t, 0, sizeof t);
    for (int k = 0; k < 3; ++k) t.scale[k] = 1.0f;
    for (int k = 0; k < channels && scale; ++k) {
        if (!jpezy_host::tensor_value_in_band(scale[k]) || !jpezy_host::tensor_value_in_band(bias[k]))
            return set_err(JPEZY_E_BADARG, who + ": scale and bias values must be 0 or finite with a magnitude in [2^-100, 2^100] (channel " +
                                               std::to_string(k) + ")");
        t.scale[k] = scale[k]; t.bias[k] = bias[k];
    }
    const long long extent[4] = { n, channels, out_h, out_w }, stride[4] = { sn, sc, sh, sw };
    const size_t elem = dtype == JPEZY_DT_U8 ? 1 : dtype == JPEZY_DT_F32 ? 4 : 2;
    switch (jpezy_host::tensor_layout_check(extent, stride, cap_elems)) {
    case jpezy_host::kTensorNegative: return set_err(JPEZY_E_BADARG, who + ": strides must not be negative");
    case jpezy_host::kTensorOverlap:
        return set_err(JPEZY_E_BADARG, who + ": the strides (" + std::to_string(sn) + ", " + std::to_string(sc) + ", " + std::to_string(sh) + ", " +
                                           std::to_string(sw) + ") do not give every element of [" + std::to_string(n) + ", " + std::to_string(channels) + ", " +
                                           std::to_string(out_h) + ", " + std::to_string(out_w) + "] a place of its own");
    case jpezy_host::kTensorNoSpace:
        return set_err(JPEZY_E_NOSPACE, who + ": a tensor [" + std::to_string(n) + ", " + std::to_string(channels) + ", " + std::to_string(out_h) + ", " +
                                            std::to_string(out_w) + "] with these strides does not fit cap_elems = " + std::to_string(cap_elems));
    default: break;
    }
    if ((uintptr_t)d_out % elem) return set_err(JPEZY_E_BADARG, who + ": d_out must be aligned to the element size");
    t.sc = (unsigned long long)sc; t.sh = (unsigned long long)sh; t.sw = (unsigned long long)sw;
    t.dtype = dtype; t.channels = channels;
    const Resize rz = { out_w, out_h, mirror_x, &t, {}, nullptr };
    return windows_driver(c, kWhoTensor, n, data, len, gray, windows, format, bytes, 0, (size_t)sn, (uint8_t*)d_out, info, placed, status, &rz);
}
JPEZY_CATCH

}  // extern "C"
