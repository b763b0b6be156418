// jpezy_capi_entropy.hip -- the C-ABI, part 2: the Huffman tail of encoder::encode (ref encoder/jpezy_encoder.hpp:174-225): the host
// writer's entry points, the GPU entropy coder in its host-delivered and its device-resident form -- one Pass (plan,
// launch chain) for both --, and encoder::encode end to end: the file-encode driver of every pixel kind and sampling
// (jpezy_internal_encode_file, jpezy_capi_encode.h) and its planar entry.
#include "jpezy_capi_encode.h"

extern "C" {
size_t jpezy_jpeg_bound(int W, int H) { return jpezy_host::jpeg_bound(W, H); }

int jpezy_write_jpeg_batch(const int16_t* coeffs, int W, int H, int gray, int n_frames, const char* comment, uint8_t* out,
                           size_t cap, long* sizes, int threads)
try {
    if (!coeffs || !out || !sizes || n_frames <= 0) return set_err(JPEZY_E_BADARG, "write_jpeg_batch: bad argument");
    if (int rc = check_comment(comment, "write_jpeg_batch")) return rc;
    const size_t cpf = jpezy_coeff_count(W, H, gray);
    if (!cpf) return set_err(JPEZY_E_BADARG, "write_jpeg_batch: bad dimensions");
    unsigned nt = threads > 0 ? (unsigned)threads : std::thread::hardware_concurrency();
    if (nt == 0) nt = 1;
    if (nt > (unsigned)n_frames) nt = (unsigned)n_frames;
    std::atomic<int> next{ 0 };
    std::atomic<int> failed{ 0 };
    auto work = [&]() {
        for (int f = next.fetch_add(1); f < n_frames; f = next.fetch_add(1)) {
            sizes[f] = jpezy_host::write_jpeg(coeffs + (size_t)f * cpf, W, H, gray != 0, comment, 0, false, out + (size_t)f * cap, cap, nullptr);
            if (sizes[f] < 0) failed.store(1);
        }
    };
    {
        Joiner pool;
        for (unsigned t = 1; t < nt; ++t) pool.start(work);
        work();
    }
    return failed.load() ? set_err(JPEZY_E_FORMAT, "write_jpeg_batch: at least one frame failed (see sizes[])") : JPEZY_OK;
}
JPEZY_CATCH

// ---- GPU entropy coding: same bytes as jpezy_write_jpeg, coefficients already on the device ----
namespace {

// the device image of four tables (DHT order YDc, CDc, YAc, CAc; nullptr: Annex K): canonical codes per symbol, and the AC codes
// of small values with their value bits appended (CodeTables::fast)
void fill_code_image(jpezy_dev::entropy::CodeTables& h, const jpezy_host::HuffTable* tabs)
{
    uint16_t code[4][256];
    uint8_t len[4][256];
    jpezy_host::enc_code_tables(code, len, tabs);
    std::memset(&h, 0, sizeof h);
    for (int t = 0; t < 2; ++t) {      // DHT order: YDc, CDc, YAc, CAc
        for (int k = 0; k < 12; ++k) h.dc[t][k] = ((uint32_t)code[t][k] << 8) | len[t][k];
        for (int k = 0; k < 256; ++k) h.ac[t][k] = ((uint32_t)code[2 + t][k] << 8) | len[2 + t][k];
        for (int run = 0; run < 16; ++run)
            for (int v = -32; v < 32; ++v) {
                if (v == 0) continue;
                const int a = v < 0 ? -v : v;
                int sz = 0;
                while ((a >> sz) != 0) ++sz;
                const int k = (run << 4) | sz;
                const uint32_t bits = ((uint32_t)code[2 + t][k] << sz) | ((uint32_t)(v + (v >> 31)) & ((1u << sz) - 1u));
                h.fast[t][(run << 6) | (v + 32)] = (bits << 5) | (uint32_t)(len[2 + t][k] + sz);
            }
    }
}

// s: the stream the caller enqueues on -- the first call of a context allocates and copies synchronously, which a capture of s forbids
int ensure_code_tables(jpezy_ctx* c, hipStream_t s)
{
    if (c->d_codes.p) return JPEZY_OK;
    std::vector<jpezy_dev::entropy::CodeTables> hv(1);       // 10 KB: off the stack
    fill_code_image(hv[0], nullptr);
    if (int rc = grow_outside_capture(c->d_codes, sizeof hv[0], s, "entropy coder")) return rc;
    HIP_TRY(hipMemcpy(c->d_codes.p, &hv[0], sizeof hv[0], hipMemcpyHostToDevice));
    return JPEZY_OK;
}

// restart: the context's setting; an interval that holds the whole frame changes the header alone, so the device is told of none
// sampling: JPEZY_SAMPLING_420 (gray or colour) or JPEZY_SAMPLING_444 / _422 (colour; the callers have refused gray) -- the job's MCU layout
void make_job(jpezy_dev::entropy::Job& job, const int16_t* d_coeffs, int W, int H, int gray, int F, const jpezy_dev::entropy::CodeTables* tables,
              int restart, int sampling = JPEZY_SAMPLING_420)
{
    const jpezy_host::McuLayout L = jpezy_host::mcu_layout(sampling, gray != 0);
    const size_t n_mcu = (size_t)((W + L.mcu_w - 1) / L.mcu_w) * (size_t)((H + L.mcu_h - 1) / L.mcu_h);
    job.restart = restart > 0 && (size_t)restart < n_mcu ? (unsigned)restart : 0u;
    job.coeffs = d_coeffs;
    job.coeffs_per_frame = n_mcu * (size_t)L.stored * 64;
    job.tables = tables;
    job.blocks_per_frame = (unsigned)(n_mcu * (size_t)L.coded);
    job.bpm = L.stored;
    job.coded = L.coded;
    job.luma = L.luma;
    job.n_frames = F;
    job.tables_stride = 0;
}

// with a restart interval the six DRI bytes come out of the comment's room (JPEZY_MAX_COMMENT_RESTART)
int check_restart_comment(const jpezy_ctx* c, const char* comment, const char* who)
{
    if (jpezy_host::restart_ok(c->restart_interval, comment)) return JPEZY_OK;
    return set_err(JPEZY_E_BADARG, std::string(who) + ": with a restart interval the comment may be at most JPEZY_MAX_COMMENT_RESTART (" +
                                       std::to_string(JPEZY_MAX_COMMENT_RESTART) + " bytes)");
}

// frames per pass with per-image tables: a frame's table image is 10 KB
constexpr int kMaxOptFramesPerPass = 1024;

// frames of one pass of either form: worst-case streams of 1 GiB, and the frame index is a grid dimension
int frames_per_pass(const jpezy_ctx* c, int W, int H, int gray, int n_frames, int sampling)
{
    jpezy_dev::entropy::Job job;
    make_job(job, nullptr, W, H, gray, 1, nullptr, c->restart_interval, sampling);
    const size_t per = std::min<size_t>(std::min<size_t>((size_t)n_frames, kMaxFramesPerLaunch), jpezy_dev::entropy::max_pass_frames(job));
    return c->huff_optimize ? std::min((int)per, kMaxOptFramesPerPass) : (int)per;
}

// One pass: F frames, all resident in the context's scratch buffers.
struct Pass {
    jpezy_dev::entropy::Job job;
    jpezy_dev::entropy::Scratch sc;
    unsigned long long* added = nullptr;   // [F] bytes stuffing adds to a frame (host-delivered form)
    hipStream_t s = nullptr;

    // Builds the job and reserves the scratch.  The per-frame error flags come in two protocols:
    //   resident = false (host-delivered form): status is cleared here, set by the coder and read by the host after the pass;
    //   resident = true (device-resident form, capturable): status is the context's e_status, zero between calls -- zeroed once when it
    //     grows (first call, never inside a capture); the consumer of the tile totals latches and clears it, the stuffing kernel reads
    //     the latched copy.  Nothing is reserved and nothing synchronised on a call whose arguments the context has seen.
    int plan(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int F, bool resident, hipStream_t stream, int sampling)
    {
        namespace E = jpezy_dev::entropy;
        s = stream;
        make_job(job, d_coeffs, W, H, gray, F, c->d_codes.as<E::CodeTables>(), c->restart_interval, sampling);
        const E::ScratchSizes z = E::scratch_sizes(job, c->huff_optimize != 0);
        // (every buffer that must grow refuses inside a capture of s; nothing has been enqueued by then)
        auto grow = [&](DevBuf& b, size_t n) { return grow_outside_capture(b, n, s, "entropy coder"); };
        if (int rc = grow(c->e_S, z.tile_stream)) return rc;
        if (int rc = grow(c->e_tt, z.tile_total)) return rc;
        if (int rc = grow(c->e_base, z.tile_base)) return rc;
        if (int rc = grow(c->e_ft, z.first_tile)) return rc;
        if (int rc = grow(c->e_rpad, z.restart_pad)) return rc;
        if (int rc = grow(c->e_U, z.U)) return rc;
        if (int rc = grow(c->e_cnt, z.ff_loc)) return rc;
        if (int rc = grow(c->e_fft, z.ff_piece)) return rc;
        if (int rc = grow(c->e_mk, z.markers)) return rc;
        if (int rc = grow(c->e_small, 2 * z.bytes + z.flags)) return rc;      // [F] stream bytes | [F] added bytes | [F] flags
        sc.tile_stream = c->e_S.as<uint32_t>();
        sc.tile_total = c->e_tt.as<uint32_t>();
        sc.tile_base = c->e_base.as<unsigned long long>();
        sc.first_tile = c->e_ft.as<uint32_t>();
        sc.restart_pad = c->e_rpad.as<unsigned long long>();
        sc.U = c->e_U.as<uint32_t>();
        sc.u_stride = E::stream_stride(job);
        sc.ft_stride = (unsigned)(sc.u_stride / E::assemble_piece_bytes());
        sc.ff_loc = c->e_cnt.as<uint32_t>();
        sc.ff_piece = c->e_fft.as<uint32_t>();
        sc.markers = c->e_mk.as<unsigned long long>();
        sc.bytes = c->e_small.as<unsigned long long>();
        added = sc.bytes + F;
        unsigned* flags = reinterpret_cast<unsigned*>(added + F);
        if (!resident) {
            sc.status = flags;
            sc.latched = nullptr;
            HIP_TRY(hipMemsetAsync(sc.status, 0, z.flags, s));
        } else {
            if (c->e_status.cap < z.flags) {
                if (int rc = grow(c->e_status, z.flags)) return rc;
                HIP_TRY(hipMemsetAsync(c->e_status.p, 0, c->e_status.cap, s));
            }
            sc.status = c->e_status.as<unsigned>();
            sc.latched = flags;
        }
        return JPEZY_OK;
    }

    // every block coded once into its tile's stream; tile offsets; streams assembled, and the bytes stuffing adds counted
    int code(bool any_tables) const
    {
        namespace E = jpezy_dev::entropy;
        HIP_TRY(E::launch_code_tiles(job, sc, s));
        // the coder may have raised error flags that only their consumer (tile offsets / assembly) clears: if the call ends between
        // the two, the flags are cleared here so that they do not leak into the context's next call
        hipError_t e = E::launch_tile_bases(job, sc, s);
        if (e == hipSuccess) e = E::launch_assemble(job, sc, any_tables, s);
        if (e == hipSuccess) return JPEZY_OK;
        (void)hipMemsetAsync(sc.status, 0, sizeof(unsigned) * (size_t)job.n_frames, s);
        return hip_err(e, "entropy stage (tile offsets / assembly)");
    }

    // byte stuffing (restart intervals: and the markers): streams out_stride apart, or with plan.hdr whole files and their verdicts
    int stuff(uint8_t* out, size_t out_stride, const jpezy_dev::entropy::FilePlan& plan) const
    {
        HIP_TRY(jpezy_dev::entropy::launch_stuff(job, sc, out, out_stride, plan, s));
        return JPEZY_OK;
    }
};

// symbol counts of the job's frames (job.tables is not read)
int enqueue_histogram(const jpezy_dev::entropy::Job& job, unsigned long long* d_hist, unsigned* d_status, hipStream_t s)
{
    HIP_TRY(jpezy_dev::entropy::launch_zero_histogram(d_hist, job.n_frames, s));      // (not hipMemsetAsync: jpezy_huffstat.hip)
    HIP_TRY(jpezy_dev::entropy::launch_symbol_histogram(job, d_hist, d_status, s));
    return JPEZY_OK;
}

// one pass of the host-delivered form
int entropy_chunk(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int F, const char* comment, uint8_t* out,
                  size_t cap, long* sizes, bool* any_failed, int sampling, const uint8_t* luma, const uint8_t* chroma)
{
    namespace E = jpezy_dev::entropy;
    hipStream_t s = c->stream;
    const bool optimize = c->huff_optimize != 0;
    Pass p;
    if (int rc = p.plan(c, d_coeffs, W, H, gray, F, false, s, sampling)) return rc;

    // 0. per-image tables: the frames' symbol counts come to the host, which builds every frame's four tables (Annex K.2) and
    //    sends their code images back; the coder then takes frame f's image.  One extra synchronisation and two small copies.
    std::vector<jpezy_host::HuffTable> tabs;
    if (optimize) {
        const size_t hist_bytes = (size_t)F * 4 * 256 * sizeof(unsigned long long), img_bytes = (size_t)F * sizeof(E::CodeTables);
        if (int rc = c->e_hist.reserve(hist_bytes)) return rc;
        if (int rc = c->e_hist_pin.reserve(hist_bytes)) return rc;
        if (int rc = c->e_codes_opt.reserve(img_bytes)) return rc;
        if (int rc = c->e_codes_pin.reserve(img_bytes)) return rc;
        if (int rc = enqueue_histogram(p.job, c->e_hist.as<unsigned long long>(), p.sc.status, s)) return rc;
        HIP_TRY(hipMemcpyAsync(c->e_hist_pin.p, c->e_hist.p, hist_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        tabs.resize((size_t)F * 4);
        const unsigned long long* hist = c->e_hist_pin.as<unsigned long long>();
        for (int f = 0; f < F; ++f) {
            for (int k = 0; k < 4; ++k) {
                jpezy_host::HuffTable& t = tabs[(size_t)f * 4 + k];
                t.nval = jpezy_host::optimal_table(hist + ((size_t)f * 4 + k) * 256, t.bits, t.vals);
            }
            fill_code_image(c->e_codes_pin.as<E::CodeTables>()[f], &tabs[(size_t)f * 4]);
        }
        HIP_TRY(hipMemcpyAsync(c->e_codes_opt.p, c->e_codes_pin.p, img_bytes, hipMemcpyHostToDevice, s));
        p.job.tables = c->e_codes_opt.as<E::CodeTables>();
        p.job.tables_stride = 1;
    }
    // 1. codes; 2. unstuffed streams, one per frame; their lengths and the bytes stuffing adds to them
    if (int rc = p.code(optimize)) return rc;
    HIP_TRY(E::launch_ff_frame_totals(p.job, p.sc, p.added, s));
    std::vector<unsigned long long> nbytes(F), fftot(F);
    std::vector<unsigned> status(F);
    HIP_TRY(hipMemcpyAsync(nbytes.data(), p.sc.bytes, sizeof(unsigned long long) * F, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(status.data(), p.sc.status, sizeof(unsigned) * F, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(fftot.data(), p.added, sizeof(unsigned long long) * F, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));

    // 3. byte stuffing into a buffer sized from the actual lengths (fftot: the bytes stuffing adds -- with restart intervals the markers too)
    unsigned long long max_out = 0;
    for (int f = 0; f < F; ++f)
        if (nbytes[f] + fftot[f] > max_out) max_out = nbytes[f] + fftot[f];
    const size_t o_stride = ((size_t)max_out + 2 + 63) / 64 * 64;
    if (int rc = c->e_out.reserve(o_stride * F)) return rc;
    if (int rc = p.stuff(c->e_out.as<uint8_t>(), o_stride, E::FilePlan())) return rc;

    // 4. header + entropy-coded segment + EOI into the caller's buffers.  One device-to-host copy of all streams into a
    //    pinned staging buffer (per-frame copies into pageable memory cost more than the kernels for small frames).
    if (int rc = c->e_pinned.reserve(o_stride * F)) return rc;
    HIP_TRY(hipMemcpyAsync(c->e_pinned.p, c->e_out.p, o_stride * F, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // (four threads when there is much to hand out: a core copies ~25 GB/s -- 256 frames of 1080p noise, 168 MB: 11.9 -> 7 ms per call)
    std::atomic<int> failed{ 0 };
    auto hand_out = [&](int f0, int step) {
        for (int f = f0; f < F; f += step) {
            uint8_t* dst = out + (size_t)f * cap;
            if (status[f]) { sizes[f] = JPEZY_E_FORMAT; failed.store(1); continue; }
            const size_t hdr = jpezy_host::write_header(W, H, comment, dst, cap, optimize ? &tabs[(size_t)f * 4] : nullptr, c->restart_interval, luma, chroma, sampling);
            const size_t body = (size_t)(nbytes[f] + fftot[f]);
            if (!hdr || hdr + body + 2 > cap) { sizes[f] = JPEZY_E_NOSPACE; failed.store(1); continue; }
            std::memcpy(dst + hdr, c->e_pinned.p + (size_t)f * o_stride, body);
            dst[hdr + body] = 0xFF;
            dst[hdr + body + 1] = 0xD9;
            sizes[f] = (long)(hdr + body + 2);
        }
    };
    const int n_copy = o_stride * (size_t)F > ((size_t)8 << 20) && F >= 4 ? 4 : 1;
    {
        Joiner helpers;
        for (int t = 1; t < n_copy; ++t) helpers.start(hand_out, t, n_copy);
        hand_out(0, n_copy);
    }
    if (failed.load()) *any_failed = true;
    return JPEZY_OK;
}

}  // namespace

// The three GPU writers and the histogram for a sampling (jpezy_capi_sampling.hip; JPEZY_SAMPLING_420: the public entries below).
// Device-resident, asynchronous variant: everything is enqueued on `stream`, nothing is copied to the host.
int jpezy_internal_write_jpeg_gpu_dev(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int sampling, int n_frames, const char* comment,
                                      uint8_t* d_out, size_t out_stride, long long* d_sizes, void* stream, const uint8_t* luma, const uint8_t* chroma)
{
    namespace E = jpezy_dev::entropy;
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!d_coeffs || !d_out || !d_sizes) return set_err(JPEZY_E_BADARG, "write_jpeg_gpu_dev: null pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "write_jpeg_gpu_dev: d_coeffs must be 16-byte aligned");
    if (int rc = check_comment(comment, "write_jpeg_gpu_dev")) return rc;
    if (int rc = check_restart_comment(c, comment, "write_jpeg_gpu_dev")) return rc;
    if (c->huff_optimize)      // (before anything is enqueued or cached: the context is left as it was)
        return set_err(JPEZY_E_UNSUPPORTED, "write_jpeg_gpu_dev: per-image Huffman tables are built on the host and this call is asynchronous; "
                                            "use jpezy_write_jpeg_gpu[_batch] or jpezy_ctx_set_huffman_optimize(ctx, 0)");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    if (int rc = ensure_code_tables(c, s)) return rc;
    // header bytes: cached on the device per (W, H, comment, restart interval, quantisation tables: the bytes are compared) -- uploaded outside any capture on first use; 1024 bytes hold the
    // header with the longest comment allowed (JPEZY_MAX_COMMENT; with a DRI segment JPEZY_MAX_COMMENT_RESTART)
    uint8_t hdr[1024];
    const size_t hdr_len = jpezy_host::write_header(W, H, comment, hdr, sizeof hdr, nullptr, c->restart_interval, luma ? luma : c->qt[0],
                                                    chroma ? chroma : c->qt[1], sampling);
    if (!hdr_len) return set_err(JPEZY_E_BADARG, "write_jpeg_gpu_dev: comment too long");
    if (c->e_hdr_len != hdr_len || std::memcmp(c->e_hdr_host, hdr, hdr_len)) {
        if (int rc = drain_before_table_rewrite(s, "write_jpeg_gpu_dev")) return rc;   // an earlier launch (any stream) may still read the old header
        if (int rc = c->e_hdr.reserve(sizeof hdr)) return rc;                          // (behind the capture check: the first call allocates)
        HIP_TRY(hipMemcpy(c->e_hdr.p, hdr, hdr_len, hipMemcpyHostToDevice));
        std::memcpy(c->e_hdr_host, hdr, hdr_len);
        c->e_hdr_len = hdr_len;
    }
    const int per = frames_per_pass(c, W, H, gray, n_frames, sampling);
    const size_t cpf = sampling == JPEZY_SAMPLING_420 ? jpezy_coeff_count(W, H, gray) : jpezy_coeff_count_sampling(W, H, sampling);
    for (int f0 = 0; f0 < n_frames; f0 += per) {
        Pass p;
        if (int rc = p.plan(c, d_coeffs + (size_t)f0 * cpf, W, H, gray, std::min(per, n_frames - f0), true, s, sampling)) return rc;
        if (int rc = p.code(false)) return rc;
        // files written (header, stuffed stream, EOI, size or verdict)
        E::FilePlan files;
        files.hdr = c->e_hdr.as<uint8_t>();
        files.hdr_len = hdr_len;
        files.sizes = d_sizes + f0;
        if (int rc = p.stuff(d_out + (size_t)f0 * out_stride, out_stride, files)) return rc;
    }
    return JPEZY_OK;
}

int jpezy_write_jpeg_gpu_dev(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int n_frames, const char* comment,
                             uint8_t* d_out, size_t out_stride, long long* d_sizes, void* stream)
{
    return jpezy_internal_write_jpeg_gpu_dev(c, d_coeffs, W, H, gray, JPEZY_SAMPLING_420, n_frames, comment, d_out, out_stride, d_sizes, stream);
}

int jpezy_internal_write_jpeg_gpu_batch(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int sampling, int n_frames, const char* comment,
                                        uint8_t* out, size_t cap, long* sizes, const uint8_t* luma, const uint8_t* chroma)
try {
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!d_coeffs || !out || !sizes) return set_err(JPEZY_E_BADARG, "write_jpeg_gpu: null pointer");
    if (int rc = check_comment(comment, "write_jpeg_gpu")) return rc;
    if (int rc = check_restart_comment(c, comment, "write_jpeg_gpu")) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = ensure_code_tables(c, c->stream)) return rc;
    const int per = frames_per_pass(c, W, H, gray, n_frames, sampling);
    bool any_failed = false;
    const size_t cpf = sampling == JPEZY_SAMPLING_420 ? jpezy_coeff_count(W, H, gray) : jpezy_coeff_count_sampling(W, H, sampling);
    for (int f0 = 0; f0 < n_frames; f0 += per) {
        const int F = std::min(per, n_frames - f0);
        if (int rc = entropy_chunk(c, d_coeffs + (size_t)f0 * cpf, W, H, gray, F, comment, out + (size_t)f0 * cap, cap, sizes + f0, &any_failed, sampling,
                                   luma ? luma : c->qt[0], chroma ? chroma : c->qt[1]))
            return rc;
    }
    return any_failed ? set_err(JPEZY_E_FORMAT, "write_jpeg_gpu: at least one frame failed (see sizes[])") : JPEZY_OK;
}
JPEZY_CATCH

int jpezy_write_jpeg_gpu_batch(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int n_frames, const char* comment,
                               uint8_t* out, size_t cap, long* sizes)
{
    return jpezy_internal_write_jpeg_gpu_batch(c, d_coeffs, W, H, gray, JPEZY_SAMPLING_420, n_frames, comment, out, cap, sizes);
}

long jpezy_write_jpeg_gpu(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, const char* comment, uint8_t* out, size_t cap)
{
    long size = 0;
    const int rc = jpezy_write_jpeg_gpu_batch(c, d_coeffs, W, H, gray, 1, comment, out, cap, &size);
    if (rc != JPEZY_OK && size >= 0) return rc;
    if (size == JPEZY_E_FORMAT) set_err(JPEZY_E_FORMAT, "write_jpeg_gpu: coefficient outside the Annex-K code tables");
    if (size == JPEZY_E_NOSPACE) set_err(JPEZY_E_NOSPACE, "write_jpeg_gpu: output buffer too small");
    return size;
}

int jpezy_ctx_set_huffman_optimize(jpezy_ctx* c, int on)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (on != 0 && on != 1) return set_err(JPEZY_E_BADARG, "huffman optimize: 0 (Annex-K tables) or 1 (per-image tables)");
    c->huff_optimize = on;
    return JPEZY_OK;
}

int jpezy_ctx_set_restart_interval(jpezy_ctx* c, int mcus)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (mcus < 0 || mcus > 65535) return set_err(JPEZY_E_BADARG, "restart interval: 0 (none) or 1..65535 MCUs (16-bit DRI field)");
    c->restart_interval = mcus;
    return JPEZY_OK;
}

int jpezy_ctx_restart_interval(const jpezy_ctx* c)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    return c->restart_interval;
}

int jpezy_internal_huffman_histogram_dev(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int sampling, int n_frames,
                                         unsigned long long* d_hist, void* stream)
{
    namespace E = jpezy_dev::entropy;
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!d_coeffs || !d_hist) return set_err(JPEZY_E_BADARG, "huffman_histogram_dev: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t cpf = sampling == JPEZY_SAMPLING_420 ? jpezy_coeff_count(W, H, gray) : jpezy_coeff_count_sampling(W, H, sampling);
    for (int f0 = 0; f0 < n_frames; f0 += kMaxFramesPerLaunch) {
        const int F = std::min(kMaxFramesPerLaunch, n_frames - f0);
        if (int rc = grow_outside_capture(c->e_hstat, sizeof(unsigned) * (size_t)F, s, "huffman_histogram_dev")) return rc;
        E::Job job;
        make_job(job, d_coeffs + (size_t)f0 * cpf, W, H, gray, F, nullptr, c->restart_interval, sampling);
        if (int rc = enqueue_histogram(job, d_hist + (size_t)f0 * 4 * 256, c->e_hstat.as<unsigned>(), s)) return rc;
    }
    return JPEZY_OK;
}

int jpezy_huffman_histogram_dev(jpezy_ctx* c, const int16_t* d_coeffs, int W, int H, int gray, int n_frames, unsigned long long* d_hist,
                                void* stream)
{
    return jpezy_internal_huffman_histogram_dev(c, d_coeffs, W, H, gray, JPEZY_SAMPLING_420, n_frames, d_hist, stream);
}

int jpezy_huffman_optimal_table(const unsigned long long freq[256], uint8_t bits[16], uint8_t vals[256])
{
    if (!freq || !bits || !vals) return set_err(JPEZY_E_BADARG, "huffman_optimal_table: null pointer");
    return jpezy_host::optimal_table(freq, bits, vals);
}

// the three forms of the host writer (jpezy_host::write_jpeg)
static long host_write(const int16_t* coeffs, int W, int H, int gray, const char* comment, int restart, int optimize, uint8_t* out, size_t cap,
                       const uint8_t* luma = nullptr, const uint8_t* chroma = nullptr)
try {
    std::string err;
    const long n = jpezy_host::write_jpeg(coeffs, W, H, gray != 0, comment, restart, optimize != 0, out, cap, &err, luma, chroma);
    if (n < 0) g_err = err;
    return n;
}
JPEZY_CATCH

long jpezy_write_jpeg(const int16_t* coeffs, int W, int H, int gray, const char* comment, uint8_t* out, size_t cap)
{
    return host_write(coeffs, W, H, gray, comment, 0, 0, out, cap);
}

long jpezy_write_jpeg_opt(const int16_t* coeffs, int W, int H, int gray, const char* comment, uint8_t* out, size_t cap)
{
    return host_write(coeffs, W, H, gray, comment, 0, 1, out, cap);
}

long jpezy_write_jpeg_rst(const int16_t* coeffs, int W, int H, int gray, const char* comment, int restart_interval, int optimize,
                          uint8_t* out, size_t cap)
{
    return host_write(coeffs, W, H, gray, comment, restart_interval, optimize, out, cap);
}

long jpezy_write_jpeg_qt(const int16_t* coeffs, int W, int H, int gray, const char* comment, const uint8_t luma[64], const uint8_t chroma[64],
                         int restart_interval, int optimize, uint8_t* out, size_t cap)
{
    if ((luma == nullptr) != (chroma == nullptr)) return set_err(JPEZY_E_BADARG, "write_jpeg_qt: one of the two tables is null (both null: Annex K)");
    for (int k = 0; luma && k < 64; ++k)
        if (!luma[k] || !chroma[k]) return set_err(JPEZY_E_BADARG, "write_jpeg_qt: a quantisation table entry is zero (1..255)");
    return host_write(coeffs, W, H, gray, comment, restart_interval, optimize, out, cap, luma, chroma);
}

// Pixels on the host -> .jpg bytes on the host, both stages on the GPU (what encoder::encode does end to end), for every pixel kind and
// sampling: the request says what a band's host segments are and where its pixels then lie on the device.
long jpezy_internal_encode_file(jpezy_ctx* c, const EncodeRequest& rq)
{
    HIP_TRY(hipSetDevice(c->device));
    const int W = rq.W, H = rq.H;
    const bool s420 = rq.sampling == JPEZY_SAMPLING_420;
    const int B = rq.gray ? 4 : 6;
    if (int rc = c->e_coef.reserve((s420 ? jpezy_coeff_count(W, H, rq.gray) : jpezy_coeff_count_sampling(W, H, rq.sampling)) * sizeof(int16_t))) return rc;
    // 4:2:0: the pixels go up band by band (jpezy_hostpipe.h) while the bands before them are transformed into the frame's coefficient
    // buffer on the device.  4:4:4 / 4:2:2: the whole frame is one band
    const std::vector<HostChunk> chunks = s420 ? plan_host_chunks(W, H, 1, rq.bytes_per_px, c->host_chunk_bytes)
                                               : std::vector<HostChunk>{ { 0, 1, 0, jpezy_mcu_rows(H) } };
    const size_t P = plane_pitch(chunks, W, H);
    auto plan = [&](int i) {
        jpezy_host::ChunkPlan p;
        rq.segments(chunks[(size_t)i], P, p.in);
        return p;
    };
    size_t max_in = 0;                          // whole 16 bytes behind the last segment: the aligned kernels stay usable
    for (size_t i = 0; i < chunks.size(); ++i)
        for (const jpezy_host::Segment& g : plan((int)i).in) max_in = std::max(max_in, (g.slot_off + g.bytes + 15) & ~(size_t)15);
    auto transform = [&](int i, uint8_t* d_in, uint8_t*, hipStream_t s) {
        const HostChunk& k = chunks[(size_t)i];
        return jpezy_internal_fdct_quant_core(c, rq.source(k, P, d_in), rq.sampling, W, k.rows(H), rq.gray, 1,
                                              c->e_coef.as<int16_t>() + (s420 ? k.coef_off(W, H, B) : 0), s);
    };
    if (s420) {
        if (int rc = run_host_bands(c, chunks.size(), max_in, 0, plan, transform)) return rc;
    } else {
        // That band is uploaded directly on the context's stream, not through the pinned ring: streaming 4:4:4 / 4:2:2 frames band by band
        // would change speed and first-call allocation, and is a feature with measurements of its own.
        if (int rc = c->in[0].reserve(max_in)) return rc;
        for (const jpezy_host::Segment& g : plan(0).in)
            HIP_TRY(hipMemcpyAsync((uint8_t*)c->in[0].p + g.slot_off, g.host, g.bytes, hipMemcpyHostToDevice, c->stream));
        if (int rc = transform(0, (uint8_t*)c->in[0].p, nullptr, c->stream)) return rc;
    }
    // the Huffman stage on the whole frame (the context's quantisation tables in the DQT segments, its restart interval and its optimise
    // setting act there), through the public entries: their texts
    if (s420) return jpezy_write_jpeg_gpu(c, c->e_coef.as<int16_t>(), W, H, rq.gray, rq.comment, rq.out, rq.cap);
    return jpezy_write_jpeg_gpu_sampling(c, c->e_coef.as<int16_t>(), W, H, rq.sampling, 0, rq.comment, rq.out, rq.cap);
}

// planar RGB on the host -> .jpg bytes on the host
long jpezy_encode_jpeg(jpezy_ctx* c, const uint8_t* r, const uint8_t* g, const uint8_t* b, int W, int H, int gray, const char* comment,
                       uint8_t* out, size_t cap)
try {
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    if (!r || !g || !b || !out) return set_err(JPEZY_E_BADARG, "encode_jpeg: null pointer");
    if (int rc = check_comment(comment, "encode_jpeg")) return rc;
    if (int rc = check_encode_variant(c, JPEZY_SAMPLING_420, gray, "encode_jpeg")) return rc;   // before anything is uploaded
    return jpezy_internal_encode_file(c, planar_encode_request(r, g, b, W, H, JPEZY_SAMPLING_420, gray, comment, out, cap));
}
JPEZY_CATCH

}  // extern "C"

namespace jpezy_capi {

// What a file encode from planes hands the driver: three input segments per band, a plane pitch apart
EncodeRequest planar_encode_request(const uint8_t* r, const uint8_t* g, const uint8_t* b, int W, int H, int sampling, int gray, const char* comment,
                                    uint8_t* out, size_t cap)
{
    return { W, H, sampling, gray, comment, out, cap, 3,
             [=](const HostChunk& k, size_t P, std::vector<jpezy_host::Segment>& in) {
                 const uint8_t* src[3] = { r, g, b };
                 for (int q = 0; q < 3; ++q) in.push_back({ const_cast<uint8_t*>(src[q]) + k.plane_off(W, H), k.plane_bytes(W, H), (size_t)q * P });
             },
             [=](const HostChunk& k, size_t P, const uint8_t* d_in) { return EncodeSource::planes(d_in, d_in + P, d_in + 2 * P, (size_t)k.rows(H) * W); } };
}

}  // namespace jpezy_capi
