// jpezy_host_codec.h -- host-side serial tail/head of the codec (internal C++ API behind the C-ABI):
// JFIF writer + Annex-K Huffman encoder, marker parser + Huffman decoder.  Product code: independent of
// oracle/ (which restates the same reference functions for checking).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/jpezy_hip.h"

namespace jpezy_host {

// ref encoder/jpezy_writer.hpp:20-105 + encoder/jpezy_encoder.hpp:174-242: header, entropy-coded segment, EOI; the size or a JPEZY_E_* status.
// restart: MCUs per restart interval (0: none, as the reference): DRI in the header; behind every interval but the last the bits are
// padded to a byte (JPEZY_PAD_BIT) and RSTn (n = interval index mod 8) follows; predictors zero at every interval's start.
// optimize: the frame's own optimal tables (below), built from the symbols this scan emits, for Annex K's: same coefficients, same decoded
// pixels, a smaller file.
// luma, chroma: the quantisation tables the two DQT segments state (natural order, 8-bit entries; nullptr: Annex K) -- the header's only;
// the coefficients are written as they are.
long write_jpeg(const int16_t* coeffs, int W, int H, bool gray, const char* comment, int restart, bool optimize, uint8_t* out, size_t cap,
                std::string* err, const uint8_t* luma = nullptr, const uint8_t* chroma = nullptr);
size_t jpeg_bound(int W, int H);

// ---- chroma sampling (JPEZY_SAMPLING_*, include/jpezy_hip.h) ----
// The scan of a frame as a layout: `coded` blocks per MCU of which the first `luma` are luma blocks (luma Huffman tables, one predictor
// running through them) and the rest one block each of Cb, Cr (chroma tables, a predictor per component); `stored` blocks per MCU lie in
// the coefficient buffer, the coded ones beyond them are zero blocks; an MCU covers mcu_w x mcu_h pixels.
// 4:2:0: 6 / 4 / 6 on 16 x 16 pixels, gray 6 / 4 / 4; 4:4:4: 3 / 1 / 3 on 8 x 8; 4:2:2: 4 / 2 / 4 on 16 x 8.
struct McuLayout {
    int coded, luma, stored, mcu_w, mcu_h;
};
inline McuLayout mcu_layout(int sampling, bool gray)
{
    if (sampling == JPEZY_SAMPLING_444) return McuLayout{ 3, 1, 3, 8, 8 };
    if (sampling == JPEZY_SAMPLING_422) return McuLayout{ 4, 2, 4, 16, 8 };
    return McuLayout{ 6, 4, gray ? 4 : 6, 16, 16 };
}
inline bool sampling_known(int sampling) { return sampling == JPEZY_SAMPLING_420 || sampling == JPEZY_SAMPLING_444 || sampling == JPEZY_SAMPLING_422; }
// write_jpeg / jpeg_bound / symbol_histogram for a sampling (colour only); JPEZY_SAMPLING_420: exactly those, gray = false
long write_jpeg_sampling(const int16_t* coeffs, int W, int H, int sampling, const char* comment, int restart, bool optimize, uint8_t* out,
                         size_t cap, std::string* err, const uint8_t* luma = nullptr, const uint8_t* chroma = nullptr);
size_t jpeg_bound_sampling(int W, int H, int sampling);
bool symbol_histogram_sampling(const int16_t* coeffs, int W, int H, int sampling, unsigned long long hist[4][256], int restart = 0);
// false for a comment longer than JPEZY_MAX_COMMENT: every writer refuses it (JPEZY_E_BADARG)
bool comment_ok(const char* comment);
// One Huffman table as a DHT segment states it: bits[l - 1] codes of length l, their symbols in vals[0..nval).
struct HuffTable {
    uint8_t bits[16];
    uint8_t vals[256];
    int nval;
};
// the bytes before the entropy-coded segment (SOI .. SOS, 644 with the default comment); 0 if cap is too small or the
// comment too long.  tabs: the four tables of the DHT segments in file order YDc, CDc, YAc, CAc (nullptr: Annex K)
// restart: MCUs per restart interval (0: none) -- a DRI segment in front of SOS; 0 is returned too for a restart interval outside
// 0..65535 or, with one, a comment longer than JPEZY_MAX_COMMENT_RESTART
// luma, chroma: the tables of the two DQT segments (natural order; nullptr: Annex K); the segments' length does not depend on them
// sampling: JPEZY_SAMPLING_420 (SOF0 states 2x2, 1x1, 1x1), JPEZY_SAMPLING_444 (1x1 three times) or JPEZY_SAMPLING_422 (2x1, 1x1, 1x1);
// 0 is returned for any other value
size_t write_header(int W, int H, const char* comment, uint8_t* out, size_t cap, const HuffTable* tabs = nullptr, int restart = 0,
                    const uint8_t* luma = nullptr, const uint8_t* chroma = nullptr, int sampling = 0);
bool restart_ok(int restart, const char* comment);
// canonical (code, length) per symbol of four tables in DHT order YDc, CDc, YAc, CAc (for the GPU coder); nullptr: Annex K
void enc_code_tables(uint16_t code[4][256], uint8_t len[4][256], const HuffTable* tabs = nullptr);

// ---- per-image optimised tables (ITU-T T.81 Annex K.2) ----
// Code lengths the coder and its scratch sizes rest on, for ANY table optimal_table can return (derivation: jpeg_bound):
constexpr int kMaxDcCodeBits = 12;      // 12 categories + the reserved symbol = 13 leaves: no leaf deeper than 12
constexpr int kMaxAcCodeBits = 16;      // Figure K.3
constexpr int kMaxBlockBits = kMaxDcCodeBits + 11 + 63 * (kMaxAcCodeBits + 10);      // 1661
constexpr int kMaxMcuBits = 6 * kMaxBlockBits;                                        // 9966
static_assert(kMaxBlockBits == 1661, "the GPU coder's scratch gives a coded block entropy::kMaxBlockBytes (jpezy_entropy.h ties the two)");
static_assert(kMaxMcuBits == 9966 && 2 * ((kMaxMcuBits + 7) / 8) + 2 + 2 <= 2688, "jpeg_bound: a stuffed MCU, pad byte and EOI within 2688 bytes");
constexpr int kMaxMcuBits444 = 3 * kMaxBlockBits;                                     // 4983: an 8 x 8 MCU of Y, Cb, Cr
static_assert(kMaxMcuBits444 == 4983 && 2 * ((kMaxMcuBits444 + 7) / 8) + 4 + 4 <= 1344,
              "jpeg_bound_sampling: a stuffed 4:4:4 MCU, a restart interval's pad and marker, the frame's pad and EOI within 1344 bytes");
constexpr int kMaxMcuBits422 = 4 * kMaxBlockBits;                                     // 6644: a 16 x 8 MCU of Y, Y, Cb, Cr
static_assert(kMaxMcuBits422 == 6644 && 2 * ((kMaxMcuBits422 + 7) / 8) + 4 + 4 <= 1792,
              "jpeg_bound_sampling: a stuffed 4:2:2 MCU, a restart interval's pad and marker, the frame's pad and EOI within 1792 bytes");
static_assert(kMaxDcCodeBits + 11 <= 31 && kMaxAcCodeBits + 10 <= 31, "one append of the GPU coder (code + value bits) is at most 31 bits");
// freq[sym] -> (bits, vals) of the optimal prefix code with no code longer than 16 bits and none of all ones; returns the
// number of symbols (those with freq != 0).  Exactly Figures K.1 - K.4, every tie in K.1 resolved toward the larger symbol
// value, working arrays for trees of any depth (256 symbols): a second implementation reproduces it bit for bit.
int optimal_table(const unsigned long long freq[256], uint8_t bits[16], uint8_t vals[256]);
// hist[k][sym]: how often the writer emits symbol sym from table k (DHT order) for this frame.  Returns false when a value lies
// outside the code tables (DC category over 11, |AC| > 1023): counted as the largest size.
// restart: MCUs per restart interval (0: none); the DC predictors are zero at every interval's start
bool symbol_histogram(const int16_t* coeffs, int W, int H, bool gray, unsigned long long hist[4][256], int restart = 0);

// What the entropy decoder needs besides jpezy_frame_info: where the scan data start, the raw DHT specifications
// (slot = tc*4 + th: 0..3 DC, 4..7 AC) and the table selector of each scan component (the reference uses Td for both
// the DC and the AC table, decoder/jpezy_decoder.hpp:630).
struct ScanSetup {
    size_t scan_pos;
    int Td[3];
    uint8_t present[8];
    int nvals[8];
    uint8_t bits[8][16];
    uint8_t vals[8][256];
};
// header only (the marker parser of read_jpeg): fills info and setup
int parse_header(const uint8_t* data, size_t len, jpezy_frame_info* info, ScanSetup* setup, std::string* err);

// ref decoder/jpezy_decoder.hpp:171-502, 583-642
int read_jpeg(const uint8_t* data, size_t len, jpezy_frame_info* info, int16_t* coeffs, size_t coeff_cap,
              std::string* err);

// Length of the entropy-coded segment that starts at scan[0]: it ends before the first marker -- a 0xFF followed by anything but 0x00 --
// or before a 0xFF that is the last byte (decoder::decode_huffman reads on until its bit reader meets one, ref decoder/jpezy_decoder.hpp:
// 583-642); n when there is none.  Compressed data holds a 0xFF every ~256 bytes, so this is a 16-bytes-at-a-time compare, not a memchr
// per 0xFF.
size_t entropy_segment_length(const uint8_t* scan, size_t n);

}  // namespace jpezy_host
