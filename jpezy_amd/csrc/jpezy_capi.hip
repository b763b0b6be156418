// jpezy_capi.hip -- the C-ABI of include/jpezy_hip.h, part 1: the per-GPU context (device id, stream, device constant tables, staging
// buffers, fallback counter) and the two transform stages: the core of every encode transform (jpezy_internal_fdct_quant_core, steered by
// an EncodeSource), the core of the fused decode kernel (jpezy_internal_fused_dev_core, steered by a DecodeSink), the planar entries of
// both and the any-layout decode pair.  No CPU fallback: every compute entry point needs a HIP device.
#include "jpezy_capi_decode.h"
#include "jpezy_capi_encode.h"

extern "C" {

const char* jpezy_hip_last_error(void) { return g_err.c_str(); }

int jpezy_hip_is_experimental_build(void)
{
#ifdef JPEZY_EXPERIMENT
    return 1;
#else
    return 0;
#endif
}

int jpezy_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int jpezy_mcu_cols(int W) { return (W / 16) + ((W % 16) ? 1 : 0); }
int jpezy_mcu_rows(int H) { return (H / 16) + ((H % 16) ? 1 : 0); }
size_t jpezy_coeff_count(int W, int H, int gray)
{
    if (W <= 0 || H <= 0) return 0;
    return (size_t)jpezy_mcu_cols(W) * (size_t)jpezy_mcu_rows(H) * (gray ? 4 : 6) * 64;
}

// Every quantiser-dependent device constant of the encode kernels as a function of the two tables (natural order, entries 1..255):
// F32Column::ks / delta1 / th, DeviceTables::qt / qinv / qscale / qfrac_bits / rq_dc / dcq, and dc_formula's constants dc_rq / dc_bias --
// zero when one of the two checks against dcq fails for these tables, which makes the launcher take the !DCG instance and the table.
// jpezy_ctx_create calls it with the Annex-K tables, jpezy_ctx_set_quant_tables with the caller's.  false (and *why): a level-1 guard
// band that would reach 0.25.
static bool build_encode_tables(const int qt[2][64], DeviceTables& h, float dc_rq[2], float dc_bias[2], std::string* why)
{
    std::memset(&h, 0, sizeof h);
    const double S = JPEZY_INV_SQRT2;
    int pos_of_row[8];                 // inverse of kPairRow: where the f32 kernel keeps coefficient row i of a block column
    for (int pp = 0; pp < 8; ++pp) pos_of_row[kPairRow[pp]] = pp;
    int qmin = 255;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) qmin = std::min(qmin, qt[t][k]);
    h.qfrac_bits = qfrac_bits(qmin);   // encode variant 0: the widest fixed point whose quotients stay inside int32 (jpezy_device.h)
    for (int t = 0; t < 2; ++t) {
        for (int j = 0; j < 8; ++j)
            for (int i = 0; i < 8; ++i) {
                const double cu = j ? 1.0 : S, cv = i ? 1.0 : S;
                h.qscale[t][j][i] = cu * cv / (4.0 * qt[t][i * 8 + j]) * (double)(1 << h.qfrac_bits);
            }
        h.rq_dc[t] = 1.0 / qt[t][0];
        for (int k = 0; k < 64; ++k) {
            h.qt[t][k] = qt[t][k];
            h.qinv[t][k] = 1.0 / qt[t][k];
        }
        for (int j = 0; j < 8; ++j)
            for (int i = 0; i < 8; ++i) {
                const double cu = j ? 1.0 : S, cv = i ? 1.0 : S;
                // the f32 kernel's 8-point transform leaves output 4 without its factor cos(pi/4); it is applied here
                const double k4 = 0x1.6a09e667f3bcdp-1;      // cos(pi/4), correctly rounded
                h.f32col[t][j].ks[pos_of_row[i]] = (float)(cu * cv / (4.0 * qt[t][i * 8 + j]) * (i == 4 ? k4 : 1.0) * (j == 4 ? k4 : 1.0));
            }
    }
    for (int t = 0; t < 2; ++t)
        for (int sum = -8192; sum <= 8192; ++sum) {
            const double cu = S, cv = S;
            const int dct = (int)((double)sum * cu * cv / 4);          // int(sum * cu * cv / 4), no contraction (build flag)
            h.dcq[t][sum + 8192] = (int16_t)(dct / qt[t][0]);      // |.| <= 1024 / Q_t[0]
        }
    // the table-free form of the same value (f32::dc_formula, persistent encode kernels): usable only if it reproduces the table for
    // every sum with these constants -- evaluated here with the kernel's own FP32 operations
    for (int t = 0; t < 2; ++t) {
        const float rq = 1.0f / (float)qt[t][0], bias = 0.5f / (float)qt[t][0];
        bool ok = true;
        for (int sum = -8192; sum <= 8192 && ok; ++sum) {
            const float d = std::trunc(std::fmaf(std::fabs((float)sum), 0.125f, -0.125f));
            const float q = std::trunc(std::fmaf(d, rq, bias));
            ok = (int)std::copysign(q, (float)sum) == (int)h.dcq[t][sum + 8192];
        }
        dc_rq[t] = ok ? rq : 0.f;
        dc_bias[t] = ok ? bias : 0.f;
    }
    {
        // f32 kernel, level 1: |t_fp32 - t| <= gamma_13 * S_i * S_j * 128 * ks + 2^-23 * |t|max, S_u = sum_x |cos_u(x)|
        // (13 roundings at most on any input->output path of the two butterfly passes; ks rounded to FP32 and the
        // fused product-and-bias fma(F, ks, delta1) rounded once: 2 * 2^-24 relative to |t| + delta1 <= 128 * S_i * S_j * ks
        // -- the few 1e-12 that delta1 adds to that rounding disappear in the 25 % margin).  tests/test_f32_error_bound.py re-derives it.
        static const double kCos[64] = JPEZY_COS_INIT;
        double S1[8];
        for (int u = 0; u < 8; ++u) {
            S1[u] = 0;
            for (int x = 0; x < 8; ++x) S1[u] += std::fabs(kCos[u * 8 + x]);
        }
        for (int t = 0; t < 2; ++t)
            for (int j = 0; j < 8; ++j) {
                double worst = 0;
                for (int i = 0; i < 8; ++i) {
                    if (i == 0 && j == 0) continue;            // DC: an exact integer sum, no transform error (checked for every sum below)
                    const double cu = j ? 1.0 : S, cv = i ? 1.0 : S;
                    const double ks = cu * cv / (4.0 * qt[t][i * 8 + j]);
                    const double amp = 128.0 * S1[i] * S1[j] * ks;
                    const double bound = 13.0 * 0x1p-24 * amp + 0x1p-23 * amp;
                    if (bound > worst) worst = bound;
                }
                const float d1 = (float)(1.25 * worst);
                // The kernel tells "near an integer other than zero" from "in the band around zero" by |t'| > 0.5: that needs
                // 2 delta1 well below 0.5.  delta1 peaks at Q = 1, at 1.15e-3 (column 1); no table of entries >= 1 comes near 0.25.
                if (!(d1 < 0.25f)) {
                    if (why) *why = "quantisation tables: level-1 guard band of " + std::to_string(d1) + " reaches 0.25";
                    return false;
                }
                h.f32col[t][j].delta1[0] = h.f32col[t][j].delta1[1] = d1;
                h.f32col[t][j].th = d1 + d1;               // exact: a doubling
            }
        // The one-quad kernel sends the DC through that quantiser too (f32::quant_block_column, DCG): t' = fma(sum, ks, delta1), flagged
        // <=> fract(t') < 2 delta1 -> dc_formula (verified above), else (int)t'.  The same FP32 operations for every sum against the table;
        // a set of constants for which they do not reproduce it keeps the table lookup (dc_rq = 0).
        for (int t = 0; t < 2; ++t) {
            const F32Column& col = h.f32col[t][0];
            bool ok = true;
            for (int sum = -8192; sum <= 8192 && ok; ++sum) {
                const float tp = std::fmaf((float)sum, col.ks[0], col.delta1[0]);
                const bool flagged = tp - std::floor(tp) < col.th;         // v_fract_f32
                ok = flagged || (int)tp == (int)h.dcq[t][sum + 8192];
            }
            if (!ok) dc_rq[t] = dc_bias[t] = 0.f;
        }
    }
    for (int j = 0; j < 8; ++j)
        for (int hh = 0; hh < 2; ++hh) {
            uint32_t w = 0;
            for (int k = 0; k < 4; ++k) w |= (uint32_t)(2 * kZzInv[kPairRow[4 * hh + k] * 8 + j]) << (8 * k);
            for (int t = 0; t < 2; ++t) (hh ? h.f32col[t][j].zz_hi : h.f32col[t][j].zz_lo) = w;
        }
    return true;
}

jpezy_ctx* jpezy_ctx_create(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_err(JPEZY_E_NODEVICE, "no HIP device (the jpezy hot path has no CPU fallback)");
        return nullptr;
    }
    if (device < 0 || device >= n) {
        set_err(JPEZY_E_NODEVICE, "device index out of range");
        return nullptr;
    }
    jpezy_ctx* c = new (std::nothrow) jpezy_ctx;
    if (!c) {
        set_err(JPEZY_E_NOSPACE, "out of host memory");
        return nullptr;
    }
    c->device = device;
    if (hipDeviceGetAttribute(&c->n_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || c->n_cus <= 0) c->n_cus = 256;
#ifdef JPEZY_WITH_LAB
    // laboratory builds only (tools/ab/ab_run.sh): the default encode kernel of every context from the environment.  The shipped
    // library reads no environment variable -- a stray one must not switch every context to another kernel
    if (const char* v = getenv("JPEZY_ENC_VARIANT")) {
        const int k = atoi(v);
        if (k >= 0 && k <= 3) c->variant = k;
    }
#endif
    std::vector<DeviceTables> hbuf(1); // 66 KB: off the stack, and private to this call (contexts may be created concurrently)
    DeviceTables& h = hbuf[0];
    std::string why;
    if (!build_encode_tables(kQt, h, c->dc_rq, c->dc_bias, &why)) {     // (cannot happen: the Annex-K tables pass every check)
        set_err(JPEZY_E_BADARG, why);
        delete c;
        return nullptr;
    }
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) c->qt[t][k] = (uint8_t)kQt[t][k];
    bool ok = hipSetDevice(device) == hipSuccess;
    ok = ok && c->stream.create() == hipSuccess;
    ok = ok && c->d_tab.try_reserve(sizeof(DeviceTables)) == hipSuccess;
    ok = ok && c->d_counter.try_reserve(sizeof(unsigned long long) * COUNTER_SHARDS) == hipSuccess;
    ok = ok && c->d_dqscale.try_reserve(sizeof(double) * 3 * 64) == hipSuccess;
    ok = ok && c->d_dqt.try_reserve(sizeof(int) * 3 * 64) == hipSuccess;
    ok = ok && c->d_dqscale_f.try_reserve(sizeof(float) * 64) == hipSuccess;
    ok = ok && hipMemcpy(c->d_tab.p, &h, sizeof h, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemset(c->d_counter.p, 0, sizeof(unsigned long long) * COUNTER_SHARDS) == hipSuccess;
    if (!ok) {
        set_err(JPEZY_E_HIP, std::string("context creation failed: ") + hipGetErrorString(hipGetLastError()));
        jpezy_ctx_destroy(c);
        return nullptr;
    }
    return c;
}

void jpezy_ctx_destroy(jpezy_ctx* c)
{
    if (c) delete c;
}

int jpezy_ctx_sync(jpezy_ctx* c)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return JPEZY_OK;
}

int jpezy_ctx_device(const jpezy_ctx* c) { return c ? c->device : -1; }
void* jpezy_ctx_stream(const jpezy_ctx* c) { return c ? (void*)(hipStream_t)c->stream : nullptr; }

void jpezy_ctx_set_force_exact(jpezy_ctx* c, int on)
{
    if (c) c->force_exact = on < 0 ? 0 : on > 3 ? 3 : on;
}

void jpezy_ctx_set_dc_table_lookup(jpezy_ctx* c, int on)
{
    if (c) c->dc_table_lookup = on != 0;
}

static_assert(JPEZY_ENCODE_GROUPS_AUTO == ENC_GROUPS_AUTO && JPEZY_ENCODE_GROUPS_4_COOP == ENC_GROUPS_4_COOP &&
              JPEZY_ENCODE_GROUPS_2_COOP == ENC_GROUPS_2_COOP && JPEZY_ENCODE_GROUPS_2_DIRECT == ENC_GROUPS_2_DIRECT,
              "enum jpezy_encode_groups and the launcher's values");

int jpezy_ctx_set_encode_groups(jpezy_ctx* c, int groups)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (groups < JPEZY_ENCODE_GROUPS_AUTO || groups > JPEZY_ENCODE_GROUPS_2_DIRECT) return set_err(JPEZY_E_BADARG, "set_encode_groups: no such workgroup form");
    c->encode_groups = groups;
    return JPEZY_OK;
}

int jpezy_ctx_encode_groups(const jpezy_ctx* c) { return c ? c->encode_groups : set_err(JPEZY_E_BADARG, "null context"); }

int jpezy_quality_tables(int quality, uint8_t luma[64], uint8_t chroma[64])
{
    if (!luma || !chroma) return set_err(JPEZY_E_BADARG, "quality_tables: null pointer");
    if (quality < 1 || quality > 100) return set_err(JPEZY_E_BADARG, "quality must be in 1..100");
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;        // libjpeg's jpeg_quality_scaling
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            const int v = (kQt[t][k] * s + 50) / 100;                        // jpeg_add_quant_table, baseline: clamped to 1..255
            (t ? chroma : luma)[k] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
        }
    return JPEZY_OK;
}

// both null: Annex K; one null or a zero entry: JPEZY_E_BADARG
static int tables_from_args(const char* who, const uint8_t* luma, const uint8_t* chroma, int qt[2][64])
{
    if ((luma == nullptr) != (chroma == nullptr)) return set_err(JPEZY_E_BADARG, std::string(who) + ": one of the two tables is null (both null: Annex K)");
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) {
            qt[t][k] = luma ? (t ? chroma : luma)[k] : kQt[t][k];
            if (qt[t][k] < 1) return set_err(JPEZY_E_BADARG, std::string(who) + ": a quantisation table entry is zero (1..255)");
        }
    return JPEZY_OK;
}

int jpezy_quant_tables_probe(const uint8_t luma[64], const uint8_t chroma[64], float delta1[2][8], int dc_generic[2], int* qfrac)
try {
    int qt[2][64];
    if (int rc = tables_from_args("quant_tables_probe", luma, chroma, qt)) return rc;
    std::vector<DeviceTables> hbuf(1);
    float rq[2], bias[2];
    std::string why;
    if (!build_encode_tables(qt, hbuf[0], rq, bias, &why)) return set_err(JPEZY_E_BADARG, why);
    for (int t = 0; t < 2; ++t) {
        if (delta1)
            for (int j = 0; j < 8; ++j) delta1[t][j] = hbuf[0].f32col[t][j].delta1[0];
        if (dc_generic) dc_generic[t] = rq[t] != 0.f;
    }
    if (qfrac) *qfrac = hbuf[0].qfrac_bits;
    return JPEZY_OK;
}
JPEZY_CATCH

int jpezy_ctx_set_quant_tables(jpezy_ctx* c, const uint8_t luma[64], const uint8_t chroma[64])
try {
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    int qt[2][64];
    if (int rc = tables_from_args("set_quant_tables", luma, chroma, qt)) return rc;
    bool same = true;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) same = same && qt[t][k] == c->qt[t][k];
    if (same) return JPEZY_OK;                                   // the device tables are rewritten only when the setting changes
    std::vector<DeviceTables> hbuf(1);
    float rq[2], bias[2];
    std::string why;
    if (!build_encode_tables(qt, hbuf[0], rq, bias, &why)) return set_err(JPEZY_E_BADARG, why);
    HIP_TRY(hipSetDevice(c->device));
    // a launch on ANY stream may still read the tables: the rule of the dequantiser tables (wait for the device; never inside a capture).
    // Nothing of the context has changed when this refuses.
    if (int rc = drain_before_table_rewrite(c->stream, "set_quant_tables")) return rc;
    HIP_TRY(hipMemcpy(c->d_tab.p, &hbuf[0], sizeof hbuf[0], hipMemcpyHostToDevice));
    for (int t = 0; t < 2; ++t) {
        for (int k = 0; k < 64; ++k) c->qt[t][k] = (uint8_t)qt[t][k];
        c->dc_rq[t] = rq[t];
        c->dc_bias[t] = bias[t];
    }
    c->qt_default = !std::memcmp(qt, kQt, sizeof qt);
    return JPEZY_OK;
}
JPEZY_CATCH

int jpezy_ctx_set_quality(jpezy_ctx* c, int quality)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    uint8_t luma[64], chroma[64];
    if (int rc = jpezy_quality_tables(quality, luma, chroma)) return rc;
    return jpezy_ctx_set_quant_tables(c, luma, chroma);
}

int jpezy_ctx_quant_tables(const jpezy_ctx* c, uint8_t luma[64], uint8_t chroma[64])
{
    if (!c || !luma || !chroma) return set_err(JPEZY_E_BADARG, "quant_tables: null pointer");
    std::memcpy(luma, c->qt[0], 64);
    std::memcpy(chroma, c->qt[1], 64);
    return JPEZY_OK;
}

int jpezy_ctx_set_decode_tolerance(jpezy_ctx* c, int on)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (on != 0 && on != 1) return set_err(JPEZY_E_BADARG, "decode tolerance: 0 (bit-exact) or 1 (within one per channel)");
    c->dec_tolerance = on;
    return JPEZY_OK;
}

int jpezy_ctx_set_variant(jpezy_ctx* c, int variant)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (variant < 0 || variant > 3) return set_err(JPEZY_E_BADARG, "unknown kernel variant");
#ifndef JPEZY_WITH_LAB
    if (variant >= 2)
        return set_err(JPEZY_E_UNSUPPORTED, "encode variants 2 and 3 (persistent kernels) exist only in laboratory builds (-DJPEZY_WITH_LAB, "
                                            "python -m jpezy_amd._build --lab): measured not faster than variant 1, they are not shipped");
#endif
    c->variant = variant;
    return JPEZY_OK;
}

long jpezy_ctx_last_fallback_count(jpezy_ctx* c)
{
    if (!c) return -1;
    static thread_local unsigned long long shards[COUNTER_SHARDS];
    if (hipSetDevice(c->device) != hipSuccess) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpy(shards, c->d_counter.p, sizeof shards, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (hipMemset(c->d_counter.p, 0, sizeof shards) != hipSuccess) return -1;
    unsigned long long v = 0;
    for (unsigned long long s : shards) v += s;
#ifdef JPEZY_WITH_LAB
    // encode variant 2 (laboratory): a workgroup whose bounded spin ran out drains the launch and raises bit 40 of the last shard --
    // the coefficients of that launch are incomplete.  Surfaced as an error, not as a count.
    if (shards[COUNTER_SHARDS - 1] >> 40) {
        set_err(JPEZY_E_HIP, "encode variant 2: a persistent workgroup gave up waiting for its ring (spin cap); the last launch's coefficients are incomplete");
        return -1;
    }
#endif
    return (long)v;
}

int jpezy_internal_check_dims(const jpezy_ctx* c, int W, int H, int n_frames)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (int rc = check_wh(W, H)) return rc;
    if (n_frames <= 0) return set_err(JPEZY_E_BADARG, "n_frames must be positive");
    return JPEZY_OK;
}

int jpezy_ctx_set_chroma_downsampling(jpezy_ctx* c, int mode)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    if (mode != JPEZY_DOWNSAMPLE_POINT && mode != JPEZY_DOWNSAMPLE_AVERAGE)
        return set_err(JPEZY_E_BADARG, "unknown chroma downsampling (JPEZY_DOWNSAMPLE_POINT = 0, JPEZY_DOWNSAMPLE_AVERAGE = 1)");
    c->chroma_downsampling = mode;
    return JPEZY_OK;
}

int jpezy_ctx_chroma_downsampling(jpezy_ctx* c)
{
    if (!c) return set_err(JPEZY_E_BADARG, "null context");
    return c->chroma_downsampling;
}

// Every encode transform: the source says where the pixels are, the sampling which MCUs they form, the context everything else.
int jpezy_internal_fdct_quant_core(jpezy_ctx* c, const EncodeSource& src, int sampling, int W, int H, int gray, int n_frames, int16_t* d_coeffs,
                                   hipStream_t s)
{
    HIP_TRY(hipSetDevice(c->device));
    const bool s420 = sampling == JPEZY_SAMPLING_420;
    EncParams p;
    p.r = src.r; p.g = src.g; p.b = src.b;
    p.plane_stride = src.frame_stride;
    p.pix = src.pix;
    p.row_stride = src.row_stride;
    p.pix_bytes = src.pix_bytes;
    p.swap_rb = src.swap_rb;
    p.c_row_stride = src.c_row_stride;
    p.c_step = src.c_step;
    p.c_frame_stride = src.c_frame_stride;
    p.y_step = src.y_step;
    p.yuv_format = src.yuv_format;
    p.coeffs = d_coeffs;
    p.coeffs_per_frame = s420 ? jpezy_coeff_count(W, H, gray) : jpezy_coeff_count_sampling(W, H, sampling);
    p.tab = c->d_tab.as<DeviceTables>();
    p.dcq_luma = p.tab->dcq[0];          // address arithmetic only: d_tab is a device pointer
    p.dcq_chroma = p.tab->dcq[1];
    p.fallback_count = c->d_counter.as<unsigned long long>();
#ifdef JPEZY_TRACE
    if (int rc = c->d_trace.reserve(sizeof(unsigned long long) * 13 * 65536)) return rc;
    p.trace = c->d_trace.as<unsigned long long>();
#endif
#ifdef JPEZY_DUMP_T
    if (int rc = c->dump_t.reserve(p.coeffs_per_frame * (size_t)n_frames * sizeof(float))) return rc;
    HIP_TRY(hipMemsetAsync(c->dump_t.p, 0, p.coeffs_per_frame * (size_t)n_frames * sizeof(float), s));
    p.dump_t = (float*)c->dump_t.p;
#endif
    p.W = W; p.H = H;
    // MCUs and work units per MCU row: 16 x 16 MCUs in quads of four (jpezy_f32_quad.h), or the sampling's 8 x 8 / 16 x 8 MCUs in
    // octets of eight (jpezy_f32_octet.h)
    if (s420) {
        p.mcu_cols = jpezy_mcu_cols(W);
        p.mcu_rows = jpezy_mcu_rows(H);
        p.quads_per_row = (p.mcu_cols + 3) / 4;
    } else {
        jpezy_sampling_geometry(sampling, W, H, &p.mcu_cols, &p.mcu_rows, nullptr);
        p.quads_per_row = (p.mcu_cols + 7) / 8;
    }
    fast_div_setup((unsigned)p.quads_per_row, &p.qpr_magic, &p.qpr_shift);
    // dc_table_lookup (test hook): the launchers then take the !DCG instance and DeviceTables::dcq, as when a create-time check fails
    for (int t = 0; t < 2; ++t) { p.dc_rq[t] = c->dc_table_lookup ? 0.f : c->dc_rq[t]; p.dc_bias[t] = c->dc_table_lookup ? 0.f : c->dc_bias[t]; }

    // The launcher, by (pixel kind, sampling, averaged chroma, variant).  Variant 0 is the FP64 kernel: planes, packed pixels and YCbCr at
    // 4:2:0 with point chroma (the entries refused everything else, check_encode_variant); every other variant is the f32 kernel.  The
    // averaged stage is read here, at launch (never YCbCr input, never 4:4:4), and 4:4:4 / 4:2:2 serve planes and packed pixels alike.
    const bool g = gray != 0, avg = !src.is_ycc() && encode_averaged(c, sampling, gray), f64 = c->variant == 0;
    const int force = c->force_exact;
    // the forced workgroup form acts on variant 1's planar launch alone (the last line of the lambda)
    const int groups = (s420 && !src.is_ycc() && !src.pix_bytes && !avg && c->variant == 1) ? c->encode_groups : JPEZY_ENCODE_GROUPS_AUTO;
    auto launch =[&](const EncParams& q) -> hipError_t {
        if (sampling == JPEZY_SAMPLING_444) return launch_fdct_quant_f32_444(q, force, s);
        if (sampling == JPEZY_SAMPLING_422 && src.is_ycc()) return launch_fdct_quant_f32_422_ycc(q, force, s);     // YCbCr 4:2:2 samples
        if (sampling == JPEZY_SAMPLING_422) return launch_fdct_quant_f32_422(q, force, avg, s);
        if (src.is_ycc()) return f64 ? launch_fdct_quant_ycc(q, g, force != 0, s) : launch_fdct_quant_f32_ycc(q, g, force, s);
        if (src.pix_bytes) {
            if (avg) return launch_fdct_quant_f32_packed_avg(q, force, s);
            return f64 ? launch_fdct_quant_packed(q, g, force != 0, s) : launch_fdct_quant_f32_packed(q, g, force, s);
        }
        if (avg) return launch_fdct_quant_f32_avg(q, force, s);
#ifdef JPEZY_WITH_LAB
        // the persistent kernels cover planar 4:2:0 with point chroma only, and were measured and archived with the Annex-K tables: every
        // other frame goes to variant 1's launch
        if (c->variant == 3 && c->qt_default) return launch_fdct_quant_f32_ps2(q, g, force, c->n_cus, s);
        if (c->variant == 2 && c->qt_default) return launch_fdct_quant_f32_ps(q, g, force, c->n_cus, s);
#endif
        return f64 ? launch_fdct_quant(q, g, force != 0, s) : launch_fdct_quant_f32(q, g, force, s, groups);
    };
    if (groups != JPEZY_ENCODE_GROUPS_AUTO && !fdct_quant_f32_groups_legal(p, groups))
        return set_err(JPEZY_E_BADARG, "the workgroup form forced by jpezy_ctx_set_encode_groups is not legal for this frame");
    // the kernels put the frame index in a grid dimension: larger batches go out in chunks
    EncodeSource at = src;
    for (int f0 = 0; f0 < n_frames; f0 += kMaxFramesPerLaunch) {
        EncParams q = p;
        q.n_frames = std::min(n_frames - f0, kMaxFramesPerLaunch);
        q.r = at.r; q.g = at.g; q.b = at.b; q.pix = at.pix;
        q.coeffs += (size_t)f0 * p.coeffs_per_frame;
        HIP_TRY(launch(q));
        at.advance((size_t)q.n_frames);
    }
    return JPEZY_OK;
}

int jpezy_fdct_quant_dev(jpezy_ctx* c, const uint8_t* d_r, const uint8_t* d_g, const uint8_t* d_b,
                         size_t plane_stride, int W, int H, int gray, int n_frames, int16_t* d_coeffs, void* stream)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!d_r || !d_g || !d_b || !d_coeffs) return set_err(JPEZY_E_BADARG, "null device pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    if (plane_stride < (size_t)W * H) return set_err(JPEZY_E_BADARG, "plane_stride smaller than W*H");
    if (int rc = check_encode_variant(c, JPEZY_SAMPLING_420, gray, "fdct_quant_dev")) return rc;
    return jpezy_internal_fdct_quant_core(c, EncodeSource::planes(d_r, d_g, d_b, plane_stride), JPEZY_SAMPLING_420, W, H, gray, n_frames, d_coeffs,
                                          (hipStream_t)stream);
}

#ifdef JPEZY_DUMP_T
int jpezy_debug_read_t(jpezy_ctx* c, float* host, size_t n)
{
    HIP_TRY(hipDeviceSynchronize());
    if (n * sizeof(float) > c->dump_t.cap) return set_err(JPEZY_E_BADARG, "debug_read_t: more than the last call dumped");
    HIP_TRY(hipMemcpy(host, c->dump_t.p, n * sizeof(float), hipMemcpyDeviceToHost));
    return JPEZY_OK;
}
#endif

#ifdef JPEZY_TRACE
int jpezy_debug_read_trace(jpezy_ctx* c, unsigned long long* host, size_t n)
{
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, c->d_trace.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return JPEZY_OK;
}
#endif

void jpezy_ctx_set_host_chunk_bytes(jpezy_ctx* c, size_t n)
{
    if (c) c->host_chunk_bytes = n < 4096 ? 4096 : n;
}

int jpezy_fdct_quant(jpezy_ctx* c, const uint8_t* r, const uint8_t* g, const uint8_t* b, int W, int H, int gray,
                     int n_frames, int16_t* coeffs)
try {
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!r || !g || !b || !coeffs) return set_err(JPEZY_E_BADARG, "null host pointer");
    if (int rc = check_encode_variant(c, JPEZY_SAMPLING_420, gray, "fdct_quant")) return rc;   // before anything is uploaded
    HIP_TRY(hipSetDevice(c->device));
    const size_t plane = (size_t)W * H;
    const int B = gray ? 4 : 6;
    const std::vector<HostChunk> chunks = plan_host_chunks(W, H, n_frames, 3, c->host_chunk_bytes);
    const size_t P = plane_pitch(chunks, W, H);
    size_t max_out = 0;
    for (const HostChunk& k : chunks) max_out = std::max(max_out, k.coef_bytes(W, B));
    const uint8_t* src[3] = { r, g, b };
    auto plan = [&](int i) {
        const HostChunk& k = chunks[(size_t)i];
        jpezy_host::ChunkPlan p;
        for (int q = 0; q < 3; ++q) p.in.push_back({ const_cast<uint8_t*>(src[q]) + k.plane_off(W, H), k.plane_bytes(W, H), (size_t)q * P });
        p.out.push_back({ coeffs + k.coef_off(W, H, B), k.coef_bytes(W, B), 0 });
        return p;
    };
    return run_host_bands(c, chunks.size(), 3 * P, max_out, plan, [&](int i, uint8_t* d_in, uint8_t* d_out, hipStream_t s) {
        const HostChunk& k = chunks[(size_t)i];
        const int Hc = k.rows(H);
        return jpezy_fdct_quant_dev(c, d_in, d_in + P, d_in + 2 * P, k.nf > 1 ? plane : (size_t)Hc * W, W, Hc, gray, k.nf, (int16_t*)d_out, s);
    });
}
JPEZY_CATCH

int jpezy_internal_upload_dequant(jpezy_ctx* c, const uint16_t qt[4][64], const uint8_t comp_tq[3], hipStream_t s)
{
    uint16_t sel[3][64];
    for (int k = 0; k < 3; ++k) std::memcpy(sel[k], qt[comp_tq[k] & 3], sizeof sel[k]);
    if (c->dq_valid && !std::memcmp(sel, c->dq_cache, sizeof sel)) return JPEZY_OK;
    // A previous launch -- on this or another stream -- may still be reading the tables.
    if (int rc = drain_before_table_rewrite(s, "dequant_idct", c->is_batch_child && s == c->stream)) return rc;
    static thread_local double h_scale[3][8][8];
    static thread_local int h_qt[3][64];
    const double S = JPEZY_INV_SQRT2;
    for (int k = 0; k < 3; ++k)
        for (int u = 0; u < 8; ++u)
            for (int v = 0; v < 8; ++v) {
                const double cu = u ? 1.0 : S, cv = v ? 1.0 : S;
                // the reference's final / 4 (ref :667) is folded in here: an exact scaling of every intermediate value
                h_scale[k][u][v] = cu * cv * (double)sel[k][v * 8 + u] * 0.25;
                h_qt[k][v * 8 + u] = sel[k][v * 8 + u];
            }
    static thread_local float h_scale_f[8][8];
    for (int u = 0; u < 8; ++u)
        for (int v = 0; v < 8; ++v) h_scale_f[u][v] = (float)h_scale[0][u][v];
    HIP_TRY(hipMemcpy(c->d_dqscale.p, h_scale, sizeof h_scale, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_dqscale_f.p, h_scale_f, sizeof h_scale_f, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_dqt.p, h_qt, sizeof h_qt, hipMemcpyHostToDevice));
    std::memcpy(c->dq_cache, sel, sizeof sel);
    int qmax = 1;
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 64; ++i) qmax = sel[k][i] > qmax ? sel[k][i] : qmax;
    c->coef_limit = 32768 / qmax;
    // Fused kernel, exact mode: with |c * Q| <= 2^23 every dequantised input is below 2^21 and the two FP64 butterfly passes err
    // by at most (8 * 6 * 8 + 6 * 64) * 2^21 * 2^-53 = 1.8e-7.  The value they must truncate like -- the reference's own
    // reference-order sum of 64 such terms -- carries a rounding error of its own, at most 64 partial sums of up to 2^27 each
    // rounded to 2^-53 relative and divided by 4: 64 * 2^27 * 2^-53 / 4 = 2.4e-7 ... 1e-6 by the coarsest count.  Together
    // at most 1.2e-6 against the 2^-18 = 3.8e-6 guard band: a margin of about three (not twenty, as this comment used to say).
    // Every 8-bit quantiser table gives a limit >= 32768: no int16 coefficient can exceed it and the kernel without the range
    // test is launched (tests/test_gpu_tolerance.py::test_all_coefficients_at_the_int16_extremes_with_q255).
    c->coef_limit_exact = (1 << 23) / qmax;
    c->dq_valid = true;
    return JPEZY_OK;
}

// The fused kernel over a batch: tables, parameters, the split at the launch limit, and the launch the sink asks for.
int jpezy_internal_fused_dev_core(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], const uint8_t comp_tq[3], const DecodeSink& out,
                                  int W, int H, int gray, int n_frames, hipStream_t s)
{
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = jpezy_internal_upload_dequant(c, qt, comp_tq, s)) return rc;
    DecParams p;
    p.coeffs_per_frame = jpezy_coeff_count(W, H, 0);
    p.plane_stride = out.frame_stride;
    p.dqscale = c->d_dqscale.as<double>();
    p.dqscale_f = c->d_dqscale_f.as<float>();
    p.dqt = c->d_dqt.as<int>();
    p.coef_limit = c->dec_tolerance ? c->coef_limit : c->coef_limit_exact;
    p.fallback_count = c->d_counter.as<unsigned long long>();
    p.W = W; p.H = H;
    p.mcu_cols = jpezy_mcu_cols(W);
    p.mcu_rows = jpezy_mcu_rows(H);
    p.quads_per_row = (p.mcu_cols + 3) / 4;
    p.row_stride = out.row_stride;
    p.pix_bytes = out.pix_bytes;
    p.swap_rb = out.pix && out.r != out.pix;                 // blue comes first
    if (out.ycc) { p.c_row_stride = out.c_row_stride; p.c_step = out.c_step; p.c_frame_stride = out.c_frame_stride; }
    const auto launch = out.ycc ? launch_dequant_idct_ycc : out.pix_bytes ? launch_dequant_idct_packed : launch_dequant_idct;
    DecodeSink at = out;
    for (int f0 = 0; f0 < n_frames; f0 += kMaxFramesPerLaunch) {
        p.n_frames = std::min(n_frames - f0, kMaxFramesPerLaunch);
        p.coeffs = d_coeffs + (size_t)f0 * p.coeffs_per_frame;
        p.r = at.r; p.g = at.g; p.b = at.b; p.pix = at.pix;
        HIP_TRY(launch(p, gray != 0, c->force_exact != 0, c->dec_tolerance != 0, s));
        at.advance((size_t)p.n_frames);
    }
    return JPEZY_OK;
}

int jpezy_dequant_idct_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], const uint8_t comp_tq[3],
                           size_t plane_stride, int W, int H, int gray, int n_frames, uint8_t* d_r, uint8_t* d_g,
                           uint8_t* d_b, void* stream)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!d_coeffs || !qt || !comp_tq || !d_r || !d_g || !d_b) return set_err(JPEZY_E_BADARG, "null pointer");
    if (!aligned16(d_coeffs)) return set_err(JPEZY_E_BADARG, "d_coeffs must be 16-byte aligned");
    if (plane_stride < (size_t)W * H) return set_err(JPEZY_E_BADARG, "plane_stride smaller than W*H");
    return jpezy_internal_fused_dev_core(c, d_coeffs, qt, comp_tq, DecodeSink::planes(d_r, d_g, d_b, plane_stride), W, H, gray, n_frames,
                                         (hipStream_t)stream);
}

int jpezy_dequant_idct(jpezy_ctx* c, const int16_t* coeffs, const uint16_t qt[4][64], const uint8_t comp_tq[3], int W,
                       int H, int gray, int n_frames, uint8_t* r, uint8_t* g, uint8_t* b)
try {
    if (int rc = jpezy_internal_check_dims(c, W, H, n_frames)) return rc;
    if (!coeffs || !qt || !comp_tq || !r || !g || !b) return set_err(JPEZY_E_BADARG, "null pointer");
    HIP_TRY(hipSetDevice(c->device));
    if (int rc = jpezy_internal_upload_dequant(c, qt, comp_tq, c->stream)) return rc;      // tables first: never rewritten while chunks are in flight
    const size_t plane = (size_t)W * H;
    const std::vector<HostChunk> chunks = plan_host_chunks(W, H, n_frames, 3, c->host_chunk_bytes);
    const size_t P = plane_pitch(chunks, W, H);
    size_t max_in = 0;
    for (const HostChunk& k : chunks) max_in = std::max(max_in, k.coef_bytes(W, 6));
    uint8_t* dst[3] = { r, g, b };
    auto plan = [&](int i) {
        const HostChunk& k = chunks[(size_t)i];
        jpezy_host::ChunkPlan p;
        p.in.push_back({ const_cast<int16_t*>(coeffs) + k.coef_off(W, H, 6), k.coef_bytes(W, 6), 0 });
        for (int q = 0; q < 3; ++q) p.out.push_back({ dst[q] + k.plane_off(W, H), k.plane_bytes(W, H), (size_t)q * P });
        return p;
    };
    return run_host_bands(c, chunks.size(), max_in, 3 * P, plan, [&](int i, uint8_t* d_in, uint8_t* d_out, hipStream_t s) {
        const HostChunk& k = chunks[(size_t)i];
        const int Hc = k.rows(H);
        return jpezy_dequant_idct_dev(c, (const int16_t*)d_in, qt, comp_tq, k.nf > 1 ? plane : (size_t)Hc * W, W, Hc, gray, k.nf, d_out, d_out + P,
                                      d_out + 2 * P, s);
    });
}
JPEZY_CATCH

// geometry + tables + the two launches of the any-layout decoder on device memory; asynchronous on stream s (the tables are
// uploaded synchronously when they changed since the last call)
int jpezy_internal_generic_dev_core(jpezy_ctx* c, const DecodeSource& src, const DecodeSink& out, hipStream_t s, int upsampling)
{
    GenericDecParams p;
    if (int rc = decode_geometry(c, src, out, &p)) return rc;
    p.W = src.W; p.H = src.H;
    // (a packed 4:2:2 sink's frames may be any number of bytes apart: its entry checked the stride against a frame's bytes)
    if (src.n_frames < 1 || (src.n_frames > 1 && !out.yuv422 && (out.frame_stride < (size_t)src.W * src.H || (out.frame_stride & 3))))
        return set_err(JPEZY_E_BADARG, "generic decoder, batch form: plane stride must hold a plane and be a multiple of 4");
    p.ycc = out.ycc;
    p.c_step = out.c_step;
    p.c_row_stride = out.c_row_stride;
    const int per = generic_frames_per_launch(p);            // samples scratch: the frames of one launch (launches run in stream order)
    if (per < 1) return set_err(JPEZY_E_UNSUPPORTED, "generic decoder: frame of more than 2^31 blocks");
    if (int rc = grow_outside_capture(c->scratch, geometry_blocks(p) * 64 * sizeof(int) * (size_t)std::min(src.n_frames, per), s, "generic decoder"))
        return rc;
    // per-component dequantiser constants (fast path) and integer quantisers (reference-order path), cached in the context
    if (int rc = upload_dequant(c, src, s)) return rc;
    p.samples = c->scratch.as<int>();
    p.dqscale = c->d_dqscale.as<double>();
    p.coef_limit = c->coef_limit;
    p.force_exact = c->force_exact != 0;
    p.fallback_count = c->d_counter.as<unsigned long long>();
    HIP_TRY(launch_dequant_idct_generic(p, s, out.yuv422 ? launch_generic_yuv422 : upsampling ? launch_smooth_rgb : nullptr));
    return JPEZY_OK;
}

int jpezy_dequant_idct_generic_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                   const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray,
                                   uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream)
{
    if (int rc = dev_head(c, W, H, 1, { d_coeffs, qt, comp_h, comp_v, comp_tq, d_r, d_g, d_b }, d_coeffs)) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_generic_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, 1 },
                                           DecodeSink::planes(d_r, d_g, d_b, 0), (hipStream_t)stream, 0);
}

int jpezy_dequant_idct_generic_batch_dev(jpezy_ctx* c, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                         const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray,
                                         int n_frames, size_t plane_stride, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream)
{
    if (int rc = dev_head(c, W, H, n_frames, { d_coeffs, qt, comp_h, comp_v, comp_tq, d_r, d_g, d_b }, d_coeffs)) return rc;
    if (plane_stride < (size_t)W * H || (plane_stride & 3)) return set_err(JPEZY_E_BADARG, "plane_stride must hold a plane and be a multiple of 4");
    HIP_TRY(hipSetDevice(c->device));
    return jpezy_internal_generic_dev_core(c, { d_coeffs, qt, ncomp, Layout(comp_h, comp_v, comp_tq), precision, W, H, gray, n_frames },
                                           DecodeSink::planes(d_r, d_g, d_b, plane_stride), (hipStream_t)stream, 0);
}

// host coefficients -> host planes through the any-layout pair (8-bit samples)
int jpezy_dequant_idct_generic(jpezy_ctx* c, const int16_t* coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                               const uint8_t comp_v[3], const uint8_t comp_tq[3], int W, int H, int gray, uint8_t* r, uint8_t* g,
                               uint8_t* b)
{
    if (int rc = jpezy_internal_check_dims(c, W, H, 1)) return rc;
    if (int rc = dev_null_check(nullptr, { coeffs, qt, comp_h, comp_v, comp_tq, r, g, b })) return rc;
    HIP_TRY(hipSetDevice(c->device));
    DecodeSource src = { nullptr, qt, ncomp, Layout(comp_h, comp_v, comp_tq), 8, W, H, gray, 1 };
    GenericDecParams geom;
    if (int rc = decode_geometry(c, src, DecodeSink::planes(nullptr, nullptr, nullptr, 0), &geom)) return rc;
    const size_t plane = (size_t)W * H, coef_bytes = geometry_blocks(geom) * 64 * sizeof(int16_t);
    for (int k = 0; k < 3; ++k)
        if (int rc = c->in[k].reserve(plane)) return rc;
    if (int rc = c->out.reserve(coef_bytes)) return rc;
    HIP_TRY(hipMemcpyAsync(c->out.p, coeffs, coef_bytes, hipMemcpyHostToDevice, c->stream));
    src.d_coeffs = (const int16_t*)c->out.p;
    if (int rc = jpezy_internal_generic_dev_core(c, src, DecodeSink::planes((uint8_t*)c->in[0].p, (uint8_t*)c->in[1].p, (uint8_t*)c->in[2].p, 0),
                                                 c->stream, 0))
        return rc;
    uint8_t* dst[3] = { r, g, b };
    for (int k = 0; k < 3; ++k) HIP_TRY(hipMemcpyAsync(dst[k], c->in[k].p, plane, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return JPEZY_OK;
}

}  // extern "C"
