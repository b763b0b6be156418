// jpezy_host_codec.cpp -- the serial tail (encode) and head (decode) of the codec, on the host.
//
// BASELINE.json north_star keeps Huffman coding with the fixed Annex-K tables on the CPU; the GPU hands
// over / receives zig-zagged int16 coefficients.  This file produces exactly the bytes the reference's
// jpezy_writer + encoder::encode_huffman would (ref encoder/jpezy_writer.hpp:20-105,
// encoder/jpezy_encoder.hpp:174-242) and parses what decoder::analyze_header / decode_huffman accept
// (ref decoder/jpezy_decoder.hpp:171-502, 583-642), but is organised for throughput: symbol-indexed code
// LUTs, a 64-bit bit accumulator, canonical max-code decoding with an 8-bit first-level lookup.
#include "jpezy_host_codec.h"

#include <cstring>
#include <optional>
#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#include "../../include/jpezy_constants.h"

namespace jpezy_host {
namespace {

const uint8_t kZZ[64] = JPEZY_ZZ_INIT;
const uint8_t kQtLuma[64] = JPEZY_QT_LUMA_INIT;
const uint8_t kQtChroma[64] = JPEZY_QT_CHROMA_INIT;

struct HuffSpec {
    uint8_t bits[16];
    const uint8_t* vals;
    int nval;
};
const uint8_t kDcLVals[] = JPEZY_DC_LUMA_VALS_INIT, kDcCVals[] = JPEZY_DC_CHROMA_VALS_INIT;
const uint8_t kAcLVals[] = JPEZY_AC_LUMA_VALS_INIT, kAcCVals[] = JPEZY_AC_CHROMA_VALS_INIT;
const HuffSpec kSpec[4] = {   // order of the DHT segments in the file: YDc, CDc, YAc, CAc (jpezy_writer.hpp:61-64)
    { JPEZY_DC_LUMA_BITS_INIT, kDcLVals, JPEZY_DC_LUMA_NVAL },
    { JPEZY_DC_CHROMA_BITS_INIT, kDcCVals, JPEZY_DC_CHROMA_NVAL },
    { JPEZY_AC_LUMA_BITS_INIT, kAcLVals, JPEZY_AC_LUMA_NVAL },
    { JPEZY_AC_CHROMA_BITS_INIT, kAcCVals, JPEZY_AC_CHROMA_NVAL },
};
const uint8_t kSpecId[4] = { 0x00, 0x01, 0x10, 0x11 };

// ---- encoder LUT: symbol -> (code, length), canonical codes of Annex C ----
struct EncLut {
    uint16_t code[256];
    uint8_t len[256];
};
struct EncTables {
    EncLut t[4];
    EncTables() { for (int k = 0; k < 4; ++k) set(k, kSpec[k].bits, kSpec[k].vals); }
    explicit EncTables(const HuffTable* tabs) { for (int k = 0; k < 4; ++k) set(k, tabs[k].bits, tabs[k].vals); }
    void set(int k, const uint8_t* bits, const uint8_t* vals)
    {
        std::memset(&t[k], 0, sizeof t[k]);
        unsigned code = 0;
        int p = 0;
        for (int l = 1; l <= 16; ++l) {
            for (int c = 0; c < bits[l - 1]; ++c, ++p) {
                t[k].code[vals[p]] = (uint16_t)code++;
                t[k].len[vals[p]] = (uint8_t)l;
            }
            code <<= 1;
        }
    }
};
const EncTables& enc_tables()
{
    static const EncTables e;
    return e;
}

// ---- MSB-first bit packer with 0xFF00 stuffing; raw byte writes realign on a byte (zero pad bits) ----
class BitSink {
public:
    BitSink(uint8_t* p, size_t cap) : p_(p), end_(p + cap), cur_(p) {}
    bool ok() const { return !overflow_; }
    size_t size() const { return (size_t)(cur_ - p_); }

    void raw(unsigned v)
    {
        flush_partial();
        if (cur_ < end_) *cur_++ = (uint8_t)v; else overflow_ = true;
    }
    void raw16(unsigned v) { raw(v >> 8); raw(v & 0xFF); }
    void raw_n(const void* s, size_t n)
    {
        const uint8_t* b = static_cast<const uint8_t*>(s);
        for (size_t i = 0; i < n; ++i) raw(b[i]);
    }
    inline void bits(unsigned v, int n)   // append the low n bits of v
    {
        acc_ = (acc_ << n) | (v & ((1u << n) - 1u));
        nacc_ += n;
        while (nacc_ >= 8) {
            const unsigned byte = (unsigned)(acc_ >> (nacc_ - 8)) & 0xFFu;
            nacc_ -= 8;
            put(byte);
            if (byte == 0xFF) put(0x00);
        }
    }
    void flush_partial()
    {
        if (nacc_ > 0) {   // pad bits: JPEZY_PAD_BIT (frozen bofstream semantics): 0 -- the byte cannot be 0xFF
            unsigned byte = (unsigned)(acc_ << (8 - nacc_)) & 0xFFu;
#if JPEZY_PAD_BIT
            byte |= (1u << (8 - nacc_)) - 1u;
            put(byte);
            if (byte == 0xFF) put(0x00);
#else
            put(byte);
#endif
            nacc_ = 0;
        }
        acc_ = 0;
    }

private:
    inline void put(unsigned b)
    {
        if (cur_ < end_) *cur_++ = (uint8_t)b; else overflow_ = true;
    }
    uint8_t* p_;
    uint8_t* end_;
    uint8_t* cur_;
    uint64_t acc_ = 0;
    int nacc_ = 0;
    bool overflow_ = false;
};

inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

// one block: DC difference category + AC run/size symbols (ref jpezy_encoder.hpp:174-225)
inline bool put_block(BitSink& o, const int16_t* z, int& pred, const EncLut& dc, const EncLut& ac)
{
    const int diff = z[0] - pred;
    pred = z[0];
    const int di = bit_length((unsigned)(diff < 0 ? -diff : diff));
    if (di > 11) return false;                                    // reference: throw runtime_error (:186)
    o.bits(dc.code[di], dc.len[di]);
    if (di) o.bits((unsigned)(diff < 0 ? diff - 1 : diff), di);

    int run = 0;
    for (int n = 1; n < 64; ++n) {
        const int v = z[n];
        if (v == 0) {
            ++run;
            continue;
        }
        while (run > 15) {
            o.bits(ac.code[0xF0], ac.len[0xF0]);                  // ZRL
            run -= 16;
        }
        const int s = bit_length((unsigned)(v < 0 ? -v : v));
        if (s > 10) return false;                                 // outside K.5/K.6 (reference: :207 / aliasing)
        const int sym = (run << 4) | s;
        o.bits(ac.code[sym], ac.len[sym]);
        o.bits((unsigned)(v < 0 ? v - 1 : v), s);
        run = 0;
    }
    if (run) o.bits(ac.code[0x00], ac.len[0x00]);                 // EOB when the block ends in zeros (:219-220)
    return true;
}

void put_header(BitSink& o, int W, int H, const char* comment, const HuffTable* tabs, int restart, const uint8_t* luma, const uint8_t* chroma,
                int sampling = JPEZY_SAMPLING_420)
{
    static const uint8_t soi_app0[] = { 0xFF, 0xD8, 0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0x00,
                                        0x01, 0x02, 0x01, 0x00, 0x60, 0x00, 0x60, 0x00, 0x00 };
    o.raw_n(soi_app0, sizeof soi_app0);
    if (comment && *comment) {
        const size_t n = std::strlen(comment);
        o.raw(0xFF); o.raw(0xFE);
        o.raw16((unsigned)(n + 3));
        o.raw_n(comment, n + 1);
    }
    for (int t = 0; t < 2; ++t) {
        const uint8_t* q = t ? (chroma ? chroma : kQtChroma) : (luma ? luma : kQtLuma);   // Pq = 0: 8-bit entries, zig-zag order
        o.raw(0xFF); o.raw(0xDB); o.raw16(67); o.raw((unsigned)t);
        for (int i = 0; i < 64; ++i) o.raw(q[kZZ[i]]);
    }
    for (int k = 0; k < 4; ++k) {
        o.raw(0xFF); o.raw(0xC4);
        const uint8_t* bits = tabs ? tabs[k].bits : kSpec[k].bits;
        const uint8_t* vals = tabs ? tabs[k].vals : kSpec[k].vals;
        const int nval = tabs ? tabs[k].nval : kSpec[k].nval;
        o.raw16((unsigned)(19 + nval));
        o.raw(kSpecId[k]);
        o.raw_n(bits, 16);
        o.raw_n(vals, (size_t)nval);
    }
    const uint8_t sof[] = { 0xFF, 0xC0, 0x00, 0x11, 0x08, (uint8_t)(H >> 8), (uint8_t)H, (uint8_t)(W >> 8), (uint8_t)W,
                            0x03, 0x00, (uint8_t)(sampling == JPEZY_SAMPLING_444 ? 0x11 : sampling == JPEZY_SAMPLING_422 ? 0x21 : 0x22), 0x00,
                            0x01, 0x11, 0x01, 0x02, 0x11, 0x01 };   // luma H, V: 2, 2; 4:4:4: 1, 1; 4:2:2: 2, 1 -- chroma 1, 1 always
    o.raw_n(sof, sizeof sof);
    if (restart > 0) {                                            // DRI: MCUs per restart interval, directly in front of SOS
        o.raw(0xFF); o.raw(0xDD); o.raw16(4); o.raw16((unsigned)restart);
    }
    static const uint8_t sos[] = { 0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x00, 0x00, 0x01, 0x11, 0x02, 0x11, 0x00, 0x3F, 0x00 };
    o.raw_n(sos, sizeof sos);
}

}  // namespace

bool comment_ok(const char* comment)
{
    return !comment || std::strlen(comment) <= JPEZY_MAX_COMMENT;      // the COM length field (n + 3) can then never wrap
}

bool restart_ok(int restart, const char* comment)
{
    if (restart < 0 || restart > 65535) return false;
    return restart == 0 || !comment || std::strlen(comment) <= JPEZY_MAX_COMMENT_RESTART;   // the six DRI bytes come out of the comment's room
}

size_t write_header(int W, int H, const char* comment, uint8_t* out, size_t cap, const HuffTable* tabs, int restart, const uint8_t* luma,
                    const uint8_t* chroma, int sampling)
{
    if (!comment_ok(comment) || !restart_ok(restart, comment)) return 0;
    if (!sampling_known(sampling)) return 0;
    BitSink o(out, cap);
    put_header(o, W, H, comment, tabs, restart, luma, chroma, sampling);
    return o.ok() ? o.size() : 0;
}

void enc_code_tables(uint16_t code[4][256], uint8_t len[4][256], const HuffTable* tabs)
{
    const EncTables own = tabs ? EncTables(tabs) : EncTables();
    const EncTables& T = tabs ? own : enc_tables();
    for (int k = 0; k < 4; ++k) {
        std::memcpy(code[k], T.t[k].code, sizeof T.t[k].code);
        std::memcpy(len[k], T.t[k].len, sizeof T.t[k].len);
    }
}

size_t jpeg_bound(int W, int H)
{
    const size_t nmcu = (size_t)((W + 15) / 16) * (size_t)((H + 15) / 16);
    // Worst case with ANY tables optimal_table can return (Annex K included): a DC code of at most kMaxDcCodeBits = 12 bits (13
    // leaves with the reserved symbol) + 11 value bits, 63 AC codes of at most 16 bits (Figure K.3) + 10 value bits:
    // kMaxBlockBits = 1661 bits per block (207.6 bytes: the GPU coder's scratch gives a block entropy::kMaxBlockBytes),
    // kMaxMcuBits = 9966 bits = 1246 bytes per MCU, 2492 if every byte were 0xFF and stuffed; pad byte (two if stuffed) and EOI
    // fit in the 196 bytes left of 2688 = 6 * 64 * 7.  A table never has more symbols than its Annex-K counterpart (12 / 162),
    // so no header is longer than the Annex-K one: the 1024 bytes and JPEZY_MAX_COMMENT stand.  (static_asserts: jpezy_host_codec.h)
    // Restart intervals: every interval but the last adds a pad byte at the most (two if it is 0xFF and stuffed) and a 2-byte marker,
    // so at one MCU per interval 4 bytes per MCU; with the frame's own pad and EOI (4 bytes, once) that is still inside the 196 bytes
    // 2492 leaves of 2688.  The six DRI bytes come out of the comment's room (JPEZY_MAX_COMMENT_RESTART).  (tests/test_restart_host.py)
    // Quantisation tables (jpezy_write_jpeg_qt, jpezy_ctx_set_quant_tables): the bound does not depend on them.  The two DQT segments
    // have a fixed length, and the worst-case scan above is the worst case of the CODE (every value of the largest size the tables hold),
    // whatever quantiser produced the values; on 8-bit input no table makes a value leave the code tables (|AC| <= 1020, DC difference
    // <= 2038 at Q = 1).  (tests/test_quant_host.py)
    return 1024 + nmcu * 6 * 64 * 7;
}

size_t jpeg_bound_sampling(int W, int H, int sampling)
{
    if (sampling == JPEZY_SAMPLING_422) {
        // Per 16 x 8 MCU of four blocks: kMaxMcuBits422 = 4 * 1661 = 6644 bits = 831 bytes, 1662 if every byte were 0xFF and stuffed; a
        // restart interval per MCU adds at most 4 bytes, the frame's own pad and EOI 4 once: inside the 130 bytes 1662 leaves of
        // 1792 = 4 * 64 * 7.  The header differs in one sampling byte: 1024 stands.  (static_assert: jpezy_host_codec.h)
        const size_t nmcu = (size_t)((W + 15) / 16) * (size_t)((H + 7) / 8);
        return 1024 + nmcu * 4 * 64 * 7;
    }
    if (sampling != JPEZY_SAMPLING_444) return jpeg_bound(W, H);
    // The same derivation per 8 x 8 MCU of three blocks: kMaxMcuBits444 = 3 * 1661 = 4983 bits = 623 bytes, 1246 if every byte were
    // 0xFF and stuffed; a restart interval per MCU adds at most 4 bytes (pad, stuffed pad, marker), the frame's own pad and EOI 4 once:
    // inside the 98 bytes 1246 leaves of 1344 = 3 * 64 * 7.  The header is the 4:2:0 one with other sampling bytes: 1024 stands.
    const size_t nmcu = (size_t)((W + 7) / 8) * (size_t)((H + 7) / 8);
    return 1024 + nmcu * 3 * 64 * 7;
}

// ---- per-image optimised tables ----
// The symbols of one block, as put_block emits them (out-of-range values: the clamped symbol, and false).
namespace {
inline bool count_block(const int16_t* z, int& pred, unsigned long long* dc, unsigned long long* ac)
{
    bool ok = true;
    const int diff = z[0] - pred;
    pred = z[0];
    int di = bit_length((unsigned)(diff < 0 ? -diff : diff));
    if (di > 11) { ok = false; di = 11; }
    ++dc[di];
    int run = 0;
    for (int n = 1; n < 64; ++n) {
        const int v = z[n];
        if (v == 0) { ++run; continue; }
        ac[0xF0] += (unsigned)(run >> 4);
        int s = bit_length((unsigned)(v < 0 ? -v : v));
        if (s > 10) { ok = false; s = 10; }
        ++ac[((run & 15) << 4) | s];
        run = 0;
    }
    if (run) ++ac[0x00];
    return ok;
}
}  // namespace

// The scan as a layout (jpezy_host_codec.h, McuLayout): luma blocks share one predictor (the first luma block of an MCU predicts from the
// previous MCU's last one, the later ones from the block before), chroma block i predicts from the same index one MCU back; blocks
// that are coded but not stored are zero blocks.
namespace {
inline size_t layout_mcus(int W, int H, const McuLayout& L)
{
    return (size_t)((W + L.mcu_w - 1) / L.mcu_w) * (size_t)((H + L.mcu_h - 1) / L.mcu_h);
}
bool symbol_histogram_layout(const int16_t* coeffs, int W, int H, const McuLayout& L, unsigned long long hist[4][256], int restart)
{
    static const int16_t kZeroBlock[64] = { 0 };
    std::memset(hist, 0, sizeof(unsigned long long) * 4 * 256);
    const size_t nmcu = layout_mcus(W, H, L);
    int pred[3] = { 0, 0, 0 };
    bool ok = true;
    for (size_t mcu = 0; mcu < nmcu; ++mcu) {
        const int16_t* z = coeffs + mcu * (size_t)L.stored * 64;
        if (restart > 0 && mcu % (size_t)restart == 0) pred[0] = pred[1] = pred[2] = 0;     // as the writer resets them
        for (int i = 0; i < L.luma; ++i) ok &= count_block(z + i * 64, pred[0], hist[0], hist[2]);
        for (int i = L.luma; i < L.coded; ++i) ok &= count_block(i < L.stored ? z + i * 64 : kZeroBlock, pred[1 + i - L.luma], hist[1], hist[3]);
    }
    return ok;
}
}  // namespace

bool symbol_histogram(const int16_t* coeffs, int W, int H, bool gray, unsigned long long hist[4][256], int restart)
{
    return symbol_histogram_layout(coeffs, W, H, mcu_layout(JPEZY_SAMPLING_420, gray), hist, restart);
}

bool symbol_histogram_sampling(const int16_t* coeffs, int W, int H, int sampling, unsigned long long hist[4][256], int restart)
{
    return symbol_histogram_layout(coeffs, W, H, mcu_layout(sampling, false), hist, restart);
}

// (aligned(64): the search loops of Figure K.1 are this function's whole cost, and where they fall relative to a 64-byte line moved the
// host side of the optimised writer by 20 % when code in front of the function grew -- 168 against 139 us per call on a 64 x 32 field,
// the same instructions.  Starting the function on a line pins the loops' placement to the function's own code; a change INSIDE the
// function can still move them: tools/measure/measure_optimal_table.py re-checks the figure on the CPU.)
__attribute__((aligned(64))) int optimal_table(const unsigned long long freq_in[256], uint8_t bits_out[16], uint8_t vals[256])
{
    // a code tree over 257 leaves is at most 256 deep (libjpeg stops at 32, which ~25 million symbols can exceed: depth d takes
    // only about Fibonacci(d + 2) of them)
    constexpr int MAXLEN = 256;
    unsigned long long freq[257];
    int codesize[257], others[257], bits[MAXLEN + 1];
    std::memset(bits_out, 0, 16);
    int nval = 0;
    for (int i = 0; i < 256; ++i) { freq[i] = freq_in[i]; nval += freq[i] != 0; }
    if (nval == 0) return 0;
    freq[256] = 1;                                        // the reserved symbol: no code of all ones (K.2)
    for (int i = 0; i < 257; ++i) { codesize[i] = 0; others[i] = -1; }
    for (;;) {                                            // Figure K.1
        int c1 = -1, c2 = -1;
        unsigned long long v = ~0ull;
        for (int i = 0; i <= 256; ++i)                    // least non-zero count; ties: the larger symbol
            if (freq[i] && freq[i] <= v) { v = freq[i]; c1 = i; }
        v = ~0ull;
        for (int i = 0; i <= 256; ++i)                    // the next one
            if (freq[i] && freq[i] <= v && i != c1) { v = freq[i]; c2 = i; }
        if (c2 < 0) break;
        freq[c1] += freq[c2];
        freq[c2] = 0;
        for (++codesize[c1]; others[c1] >= 0;) { c1 = others[c1]; ++codesize[c1]; }
        others[c1] = c2;
        for (++codesize[c2]; others[c2] >= 0;) { c2 = others[c2]; ++codesize[c2]; }
    }
    for (int i = 0; i <= MAXLEN; ++i) bits[i] = 0;        // Figure K.2
    for (int i = 0; i <= 256; ++i)
        if (codesize[i]) ++bits[codesize[i]];
    for (int i = MAXLEN; i > 16; --i)                     // Figure K.3
        while (bits[i] > 0) {
            int j = i - 2;
            while (bits[j] == 0) --j;
            bits[i] -= 2;
            ++bits[i - 1];
            bits[j + 1] += 2;
            --bits[j];
        }
    {
        int i = 16;
        while (bits[i] == 0) --i;
        --bits[i];                                        // the reserved symbol leaves the longest length
    }
    for (int l = 1; l <= 16; ++l) bits_out[l - 1] = (uint8_t)bits[l];
    int p = 0;                                            // Figure K.4: by code size, then ascending value
    for (int l = 1; l <= MAXLEN; ++l)
        for (int j = 0; j < 256; ++j)
            if (codesize[j] == l) vals[p++] = (uint8_t)j;
    return nval;
}

namespace {
long write_jpeg_layout(const int16_t* coeffs, int W, int H, const McuLayout& L, int sampling, const char* comment, int restart, bool optimize, uint8_t* out,
                       size_t cap, std::string* err, const uint8_t* luma, const uint8_t* chroma)
{
    if (!coeffs || !out || W <= 0 || H <= 0 || W > 65535 || H > 65535) {
        if (err) *err = "write_jpeg: bad argument";
        return JPEZY_E_BADARG;
    }
    if (!comment_ok(comment)) {
        if (err) *err = "write_jpeg: comment longer than JPEZY_MAX_COMMENT (" + std::to_string(JPEZY_MAX_COMMENT) + " bytes)";
        return JPEZY_E_BADARG;
    }
    if (restart < 0 || restart > 65535) {
        if (err) *err = "write_jpeg: restart interval must be in 0..65535 MCUs";
        return JPEZY_E_BADARG;
    }
    if (!restart_ok(restart, comment)) {
        if (err) *err = "write_jpeg: with a restart interval the comment may be at most JPEZY_MAX_COMMENT_RESTART (" +
                        std::to_string(JPEZY_MAX_COMMENT_RESTART) + " bytes)";
        return JPEZY_E_BADARG;
    }
    HuffTable tabs[4];
    std::optional<EncTables> own;
    if (optimize) {      // the frame's own tables, from the symbols THIS scan emits: the DC difference at an interval start is taken against 0
        unsigned long long hist[4][256];
        if (!symbol_histogram_layout(coeffs, W, H, L, hist, restart)) {
            if (err) *err = "write_jpeg: coefficient outside the code tables";
            return JPEZY_E_FORMAT;
        }
        for (int k = 0; k < 4; ++k) tabs[k].nval = optimal_table(hist[k], tabs[k].bits, tabs[k].vals);
        own.emplace(tabs);
    }
    const EncTables& T = own ? *own : enc_tables();

    BitSink o(out, cap);
    put_header(o, W, H, comment, optimize ? tabs : nullptr, restart, luma, chroma, sampling);

    static const int16_t kZeroBlock[64] = { 0 };
    const size_t nmcu = layout_mcus(W, H, L);
    int pred[3] = { 0, 0, 0 };                                     // pre_DC: reset only at a restart interval's start
    for (size_t mcu = 0; mcu < nmcu; ++mcu) {
        const int16_t* z = coeffs + mcu * (size_t)L.stored * 64;
        if (restart > 0 && mcu != 0 && mcu % (size_t)restart == 0) {
            // behind every interval but the last: pad to a byte (JPEZY_PAD_BIT, a padded 0xFF stuffed), then RSTn, never stuffed
            o.raw(0xFF); o.raw(0xD0 + (unsigned)((mcu / (size_t)restart - 1) & 7));
            pred[0] = pred[1] = pred[2] = 0;
        }
        bool good = true;
        for (int i = 0; i < L.luma; ++i) good &= put_block(o, z + i * 64, pred[0], T.t[0], T.t[2]);
        for (int i = L.luma; i < L.coded; ++i) good &= put_block(o, i < L.stored ? z + i * 64 : kZeroBlock, pred[1 + i - L.luma], T.t[1], T.t[3]);
        if (!good) {
            if (err) *err = "write_jpeg: coefficient outside the Annex-K code tables";
            return JPEZY_E_FORMAT;
        }
        if (!o.ok()) break;
    }
    o.raw(0xFF); o.raw(0xD9);
    if (!o.ok()) {
        if (err) *err = "write_jpeg: output buffer too small";
        return JPEZY_E_NOSPACE;
    }
    return (long)o.size();
}
}  // namespace

long write_jpeg(const int16_t* coeffs, int W, int H, bool gray, const char* comment, int restart, bool optimize, uint8_t* out, size_t cap,
                std::string* err, const uint8_t* luma, const uint8_t* chroma)
{
    return write_jpeg_layout(coeffs, W, H, mcu_layout(JPEZY_SAMPLING_420, gray), JPEZY_SAMPLING_420, comment, restart, optimize, out, cap, err, luma, chroma);
}

long write_jpeg_sampling(const int16_t* coeffs, int W, int H, int sampling, const char* comment, int restart, bool optimize, uint8_t* out,
                         size_t cap, std::string* err, const uint8_t* luma, const uint8_t* chroma)
{
    if (!sampling_known(sampling)) {
        if (err) *err = "write_jpeg: unknown sampling";
        return JPEZY_E_BADARG;
    }
    return write_jpeg_layout(coeffs, W, H, mcu_layout(sampling, false), sampling, comment, restart, optimize, out, cap, err, luma, chroma);
}

// ======================================================================================================
// reader
// ======================================================================================================
namespace {

struct DecTable {
    int n = 0;
    uint8_t val[256];
    int32_t maxcode[18];   // maxcode[l]: largest code of length l (or -1)
    int32_t valptr[17];
    int32_t mincode[17];
    uint8_t look_len[256]; // 8-bit first-level lookup: code length (0 = longer than 8)
    bool prefix_code = true; // false: the counts over-subscribe the code space; no lookup, the bit-by-bit search decides
    uint8_t look_val[256];
    // a table no DHT segment defined holds no codes: every symbol read from it fails, like the reference's empty
    // huffman_table (decode_huffman_impl finds nothing and throws, :629-641)
    DecTable()
    {
        std::memset(look_len, 0, sizeof look_len);
        std::memset(look_val, 0, sizeof look_val);
        std::memset(val, 0, sizeof val);
        for (int l = 0; l < 18; ++l) maxcode[l] = -1;
        for (int l = 0; l < 17; ++l) valptr[l] = mincode[l] = 0;
    }
};

void build_dec(DecTable& t, const uint8_t bits[16], const uint8_t* vals, int n)
{
    t.n = n;
    std::memcpy(t.val, vals, (size_t)n);
    std::memset(t.look_len, 0, sizeof t.look_len);
    int code = 0, p = 0;
    t.prefix_code = true;
    for (int l = 1; l <= 16; ++l) {
        if (code + (int)bits[l - 1] > (1 << l)) t.prefix_code = false;
        if (bits[l - 1]) {
            t.valptr[l] = p;
            t.mincode[l] = code;
            for (int c = 0; c < bits[l - 1]; ++c, ++p, ++code) {
                if (l <= 8 && code < (1 << l)) {       // an over-subscribed DHT yields codes no l-bit read can equal: not in the LUT
                    const int lo = code << (8 - l);
                    for (int f = 0; f < (1 << (8 - l)); ++f) {
                        t.look_len[lo + f] = (uint8_t)l;
                        t.look_val[lo + f] = vals[p];
                    }
                }
            }
            t.maxcode[l] = code - 1;
        } else {
            t.maxcode[l] = -1;
            t.valptr[l] = p;
            t.mincode[l] = code;
        }
        code <<= 1;
    }
    t.maxcode[17] = 0x7FFFFFFF;
    if (!t.prefix_code) std::memset(t.look_len, 0, sizeof t.look_len);
}

struct Reader {
    const uint8_t* p;
    size_t len, pos = 0;
    uint64_t acc = 0;
    int nacc = 0;
    int pad = 0;       // zero bytes fed past the end of the data

    int byte() { nacc = 0; acc = 0; return pos < len ? p[pos++] : -1; }
    int word() { const int a = byte(), b = byte(); return (a < 0 || b < 0) ? -1 : (a << 8) | b; }
    void skip(long n) { nacc = 0; acc = 0; if (n > 0) pos += (size_t)n; if (pos > len) pos = len; }

    inline void fill()
    {
        while (nacc <= 56) {
            unsigned b = 0;
            if (pos < len) {
                b = p[pos++];
                if (b == 0xFF && pos < len && p[pos] == 0x00) ++pos;   // stuffed zero
            } else {
                ++pad;
            }
            acc = (acc << 8) | b;
            nacc += 8;
        }
    }
    inline int peek8() { if (nacc < 8) fill(); return (int)((acc >> (nacc - 8)) & 0xFF); }
    inline int get(int n)
    {
        if (n == 0) return 0;
        if (nacc < n) fill();
        nacc -= n;
        return (int)((acc >> nacc) & ((1u << n) - 1u));
    }
    // Before a byte-level marker scan (restart handling): give back the whole bytes that were buffered
    // but not used.  A stuffed 0xFF00 pair was consumed as one buffered byte.
    void realign()
    {
        int whole = nacc / 8 - pad;
        size_t q = pos;
        for (; whole > 0 && q > 0; --whole) {
            --q;
            if (q > 0 && p[q] == 0x00 && p[q - 1] == 0xFF) --q;
        }
        pos = q;
        nacc = 0; acc = 0; pad = 0;
    }
};

inline int decode_symbol(Reader& r, const DecTable& t)
{
    const int look = r.peek8();
    int l = t.look_len[look];
    if (l) {
        r.nacc -= l;
        return t.look_val[look];
    }
    int code = t.prefix_code ? r.get(8) : 0;
    for (l = t.prefix_code ? 9 : 1; l <= 16; ++l) {
        code = (code << 1) | r.get(1);
        // the codes of length l are mincode..maxcode; both tests, so that a DHT whose counts do not describe a prefix code
        // (over-subscribed, or with gaps) behaves like the reference's search for an equal (length, code) pair (:629-640)
        if (code >= t.mincode[l] && code <= t.maxcode[l]) return t.val[t.valptr[l] + code - t.mincode[l]];
    }
    return -1;
}

inline int extend(int v, int cat) { return (v & (1 << (cat - 1))) ? v : v - ((1 << cat) - 1); }

int next_marker(Reader& r)   // ref decoder/jpezy_decoder.hpp:486-502
{
    for (;;) {
        int c = r.byte();
        if (c < 0) return -1;
        if (c != 0xFF) continue;
        c = r.byte();
        if (c < 0) return -1;
        if (c == 0) continue;
        if (c > 0x02 && c < 0xC0) return 0xFF;
        return c;
    }
}

}  // namespace

namespace {
int read_jpeg_impl(const uint8_t* data, size_t len, jpezy_frame_info* info, int16_t* coeffs, size_t coeff_cap, std::string* err,
                   ScanSetup* setup);
}

int read_jpeg(const uint8_t* data, size_t len, jpezy_frame_info* info, int16_t* coeffs, size_t coeff_cap,
              std::string* err)
{
    return read_jpeg_impl(data, len, info, coeffs, coeff_cap, err, nullptr);
}

int parse_header(const uint8_t* data, size_t len, jpezy_frame_info* info, ScanSetup* setup, std::string* err)
{
    if (!setup) { if (err) *err = "parse_header: bad argument"; return JPEZY_E_BADARG; }
    std::memset(setup, 0, sizeof *setup);
    return read_jpeg_impl(data, len, info, nullptr, 0, err, setup);
}

namespace {
int read_jpeg_impl(const uint8_t* data, size_t len, jpezy_frame_info* info, int16_t* coeffs, size_t coeff_cap, std::string* err,
                   ScanSetup* setup)
{
    auto fail = [&](int code, const char* msg) { if (err) *err = msg; return code; };
    if (!data || !info) return fail(JPEZY_E_BADARG, "read_jpeg: bad argument");
    std::memset(info, 0, sizeof *info);
    info->hdensity = info->vdensity = 1;

    Reader r{ data, len };
    DecTable* ht = new DecTable[8];   // [tc*4 + th]
    struct Free { DecTable* p; ~Free() { delete[] p; } } guard{ ht };
    int Td[3] = { 0, 0, 0 };
    bool have_ht = false, have_qt = false, have_sos = false, have_sof = false;

    // SOI
    for (;;) {
        const int mk = next_marker(r);
        if (mk < 0) return fail(JPEZY_E_FORMAT, "read_jpeg: no SOI");
        if (mk == 0xD8) break;
    }
    while (!have_sos) {
        const int mk = next_marker(r);
        if (mk < 0) return fail(JPEZY_E_FORMAT, "read_jpeg: truncated header");
        switch (mk) {
        case 0xC0: {   // SOF0 (:279-305)
            r.word();
            info->precision = r.byte();
            info->height = r.word();
            info->width = r.word();
            info->ncomp = r.byte();
            if (info->ncomp != 3 && info->ncomp != 1) return fail(JPEZY_E_FORMAT, "read_jpeg: dimension not supported");
            for (int i = 0; i < info->ncomp; ++i) {
                r.byte();
                const int c = r.byte();
                if (c < 0) return fail(JPEZY_E_FORMAT, "read_jpeg: truncated SOF0");
                info->H[i] = c >> 4;
                info->V[i] = c & 15;
                if (info->H[i] > info->hmax) info->hmax = info->H[i];
                if (info->V[i] > info->vmax) info->vmax = info->V[i];
                info->Tq[i] = r.byte();
            }
            have_sof = true;
            break;
        }
        case 0xC4: {   // DHT (:190-256)
            const long seg = r.word() - 2;
            const size_t end = r.pos + (size_t)(seg > 0 ? seg : 0);
            do {
                const int id = r.byte();
                if (id < 0 || (id >> 4) > 1 || (id & 15) > 3) return fail(JPEZY_E_FORMAT, "read_jpeg: bad DHT id");
                uint8_t bits[16], vals[256];
                int n = 0;
                for (int i = 0; i < 16; ++i) { const int b = r.byte(); if (b < 0) return fail(JPEZY_E_FORMAT, "read_jpeg: truncated DHT"); bits[i] = (uint8_t)b; n += b; }
                if (n > 256) return fail(JPEZY_E_FORMAT, "read_jpeg: invalid size table");
                for (int i = 0; i < n; ++i) { const int b = r.byte(); if (b < 0) return fail(JPEZY_E_FORMAT, "read_jpeg: truncated DHT"); vals[i] = (uint8_t)b; }
                build_dec(ht[(id >> 4) * 4 + (id & 15)], bits, vals, n);
                if (setup) {
                    const int slot = (id >> 4) * 4 + (id & 15);
                    setup->present[slot] = 1;
                    setup->nvals[slot] = n;
                    std::memcpy(setup->bits[slot], bits, 16);
                    std::memcpy(setup->vals[slot], vals, (size_t)n);
                }
            } while (r.pos < end);
            have_ht = true;
            break;
        }
        case 0xDB: {   // DQT (:258-277)
            const long seg = r.word() - 2;
            const size_t end = r.pos + (size_t)(seg > 0 ? seg : 0);
            do {
                const int c = r.byte();
                if (c < 0) return fail(JPEZY_E_FORMAT, "read_jpeg: truncated DQT");
                uint16_t* q = info->qt[c & 3];
                for (int i = 0; i < 64; ++i) {
                    const int v = (c >> 4) ? r.word() : r.byte();
                    if (v < 0) return fail(JPEZY_E_FORMAT, "read_jpeg: truncated DQT");
                    q[kZZ[i]] = (uint16_t)v;
                }
            } while (r.pos < end);
            have_qt = true;
            break;
        }
        case 0xDC: r.word(); info->height = r.word(); break;                 // DNL
        case 0xDD: r.word(); info->restart_interval = r.word(); break;       // DRI
        case 0xD9: return fail(JPEZY_E_FORMAT, "read_jpeg: EOI before SOS");   // analyze_header throws (:187)
        case 0xDA: {   // SOS (:307-334)
            r.word();
            const int ns = r.byte();
            if (ns < 0 || ns > 3) return fail(JPEZY_E_FORMAT, "read_jpeg: bad SOS");
            for (int i = 0; i < ns; ++i) {
                r.byte();
                const int c = r.byte();
                if (c < 0 || (c >> 4) > 2 || (c & 15) > 2) return fail(JPEZY_E_FORMAT, "read_jpeg: bad SOS table id");
                Td[i] = c >> 4;
            }
            r.byte(); r.byte(); r.byte();
            have_sos = true;
            break;
        }
        case 0xFE: {   // COM (:405-410)
            const long seg = r.word() - 2;
            size_t k = 0;
            for (long i = 0; i < seg; ++i) {
                const int c = r.byte();
                if (c < 0) return fail(JPEZY_E_FORMAT, "read_jpeg: truncated COM");
                if (c && k + 1 < sizeof info->comment) info->comment[k++] = (char)c;
            }
            info->comment[k] = 0;
            break;
        }
        case 0xE0: {   // APP0 (:422-448)
            const long seg = r.word() - 2;
            if (seg >= 4) {
                char id[5];
                for (char& ch : id) ch = (char)r.byte();
                if (!std::memcmp(id, "JFIF", 4)) {
                    info->format = 1;
                    info->major_rev = r.byte();
                    info->minor_rev = r.byte();
                    info->units = r.byte();
                    info->hdensity = r.word();
                    info->vdensity = r.word();
                    r.byte(); r.byte();
                    r.skip(seg - 14);
                } else if (!std::memcmp(id, "JFXX", 4)) {
                    info->format = 2;
                    r.byte();
                    r.skip(seg - 1);
                } else {
                    r.skip(seg - 4);
                }
            } else {
                r.skip(seg);
            }
            break;
        }
        // frames the reference does not support: it builds an exception object and never throws it (:412-421)
        case 0xC1: case 0xC2: case 0xC3: case 0xC5: case 0xC6: case 0xC7: case 0xC9: case 0xCA: case 0xCB:
        case 0xCD: case 0xCE: case 0xCF: case 0xDF: case 0xCC: case 0xDE:
            break;
        default:
            if (mk >= 0xE1 && mk <= 0xEF) { r.skip(r.word() - 2); break; }
            return fail(JPEZY_E_FORMAT, "read_jpeg: Marker error");          // :480-481
        }
    }
    if (!(have_ht || have_qt || have_sos)) return fail(JPEZY_E_FORMAT, "read_jpeg: not decodable");
    if (!have_sof || info->hmax <= 0 || info->vmax <= 0) return fail(JPEZY_E_FORMAT, "read_jpeg: no frame header");

    const int Vblock = (info->height >> 3) + ((info->height & 7) > 0);   // get_blocks (:166-169)
    const int Hblock = (info->width >> 3) + ((info->width & 7) > 0);
    info->mcu_cols = Hblock / info->hmax + ((Hblock % info->hmax) ? 1 : 0);
    info->mcu_rows = Vblock / info->vmax + ((Vblock % info->vmax) ? 1 : 0);
    info->blocks_per_mcu = 0;
    for (int i = 0; i < info->ncomp; ++i) {
        if (info->H[i] <= 0 || info->V[i] <= 0) return fail(JPEZY_E_FORMAT, "read_jpeg: zero sampling factor");
        info->blocks_per_mcu += info->H[i] * info->V[i];
    }
    if (setup) {
        setup->scan_pos = r.pos;
        for (int i = 0; i < 3; ++i) setup->Td[i] = Td[i];
    }
    if (!coeffs) return JPEZY_OK;

    const size_t nmcu = (size_t)info->mcu_cols * info->mcu_rows;
    if (coeff_cap < nmcu * (size_t)info->blocks_per_mcu * 64) return fail(JPEZY_E_NOSPACE, "read_jpeg: coefficient buffer too small");

    int pred[3] = { 0, 0, 0 };
    size_t restart_counter = 0;
    int16_t* z = coeffs;
    for (size_t mcu = 0; mcu < nmcu; ++mcu) {
        for (int sc = 0; sc < info->ncomp; ++sc) {
            // the reference selects BOTH tables with scomp[sc].Td (:630)
            const DecTable& dc = ht[0 * 4 + Td[sc]];
            const DecTable& ac = ht[1 * 4 + Td[sc]];
            for (int kb = info->H[sc] * info->V[sc]; kb > 0; --kb, z += 64) {
                int cat = decode_symbol(r, dc);
                if (cat < 0 || cat > 16) return fail(JPEZY_E_FORMAT, "read_jpeg: decode_huffman");
                if (cat) pred[sc] += extend(r.get(cat), cat);
                // the reference's predictor and dct[0] are int (:596-597, 692-693); the coefficients here are int16
                if (pred[sc] < -32768 || pred[sc] > 32767)
                    return fail(JPEZY_E_UNSUPPORTED, ("read_jpeg: DC of component " + std::to_string(sc) + " leaves int16 (" +
                                                      std::to_string(pred[sc]) + ") in block " + std::to_string((z - coeffs) / 64) +
                                                      " (MCU " + std::to_string(mcu) + ")").c_str());
                z[0] = (int16_t)pred[sc];
                int k = 1;
                while (k < 64) {
                    const int rs = decode_symbol(r, ac);
                    if (rs < 0) return fail(JPEZY_E_FORMAT, "read_jpeg: decode_huffman");
                    if (rs == 0) break;
                    const int run = rs >> 4, s = rs & 15;
                    if (run + k > 63) return fail(JPEZY_E_FORMAT, "read_jpeg: decode_huffman");
                    for (int i = 0; i < run; ++i) z[k++] = 0;
                    z[k++] = (int16_t)(s ? extend(r.get(s), s) : 0);
                }
                while (k < 64) z[k++] = 0;
                if (r.pad > 16) return fail(JPEZY_E_FORMAT, "read_jpeg: truncated scan");
            }
        }
        if (info->restart_interval && ++restart_counter >= (size_t)info->restart_interval) {   // :152-163
            restart_counter = 0;
            r.realign();
            const int mk = next_marker(r);
            if (mk >= 0xD0 && mk <= 0xD7) pred[0] = pred[1] = pred[2] = 0;
        }
    }
    return JPEZY_OK;
}
}  // namespace

size_t entropy_segment_length(const uint8_t* scan, size_t n)
{
    size_t i = 0;
#if defined(__SSE2__)
    const __m128i ff = _mm_set1_epi8((char)0xFF), zero = _mm_setzero_si128();
    for (; i + 17 <= n; i += 16) {
        const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i*>(scan + i));
        const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(scan + i + 1));
        const int hit = _mm_movemask_epi8(_mm_andnot_si128(_mm_cmpeq_epi8(b, zero), _mm_cmpeq_epi8(a, ff)));   // 0xFF, next != 0x00
        if (hit) return i + (size_t)__builtin_ctz((unsigned)hit);
    }
#endif
    for (; i < n; ++i)
        if (scan[i] == 0xFF && (i + 1 >= n || scan[i + 1] != 0x00)) return i;
    return n;
}

}  // namespace jpezy_host
