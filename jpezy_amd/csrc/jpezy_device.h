// jpezy_device.h -- shared declarations of the gfx950 kernels and their launchers (internal).
#pragma once
#include "jpezy_experiment.h"
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace jpezy_dev {

// Fixed-point scale of encode variant 0's quantiser guard band: a coefficient is v/Q * 2^bits truncated to int32.  |v| <= 1024 (the DC of
// a block of -128s; every other coefficient stays below 128 * 5.13^2 / 4 = 842), so |v/Q| <= 1024 / Qmin with Qmin the smallest entry of
// the two tables, and bits = qfrac_bits(Qmin) is the largest width, at most QFRAC_BITS_MAX, with 1024 / Qmin * 2^bits < 2^31: 24 with the
// Annex-K tables (Qmin = 10, the width this kernel has always had), 20 at Qmin = 1.  DeviceTables::qfrac_bits carries it.
constexpr int QFRAC_BITS_MAX = 24;
inline int qfrac_bits(int qmin)
{
    int bits = QFRAC_BITS_MAX;
    while (bits > 0 && (1024ll << bits) >= (long long)qmin << 31) --bits;
    return bits;
}

// Per (table, block column j) record of the f32 encode kernel: one 64-byte line per lane, three loads off one address.
// The kernel's packed 8-point transform delivers its outputs as the pairs (0,4) (2,6) (1,3) (5,7): everything indexed by
// the coefficient row is stored in that order, position p <-> row kPairRow[p].
constexpr int kPairRow[8] = { 0, 4, 2, 6, 1, 3, 5, 7 };
struct F32Column {
    float ks[8];              // ks[p] = cu(j) * cv(i) / (4 * Q_t[i*8+j]) * cos(pi/4)^[i == 4] * cos(pi/4)^[j == 4], i = kPairRow[p]
    // level-1 guard band: 1.25 x max over i of the worst-case FP32 error of t[i][j] = F[i][j] * ks
    // (jpezy_capi.hip; tests/test_f32_error_bound.py re-derives it); twice, as the addend pair of a v_pk_fma_f32
    float delta1[2];
    float th;                 // 2 * delta1: the kernel's test is fract(F * ks + delta1) < th
    // byte p of zz_lo (p < 4) / zz_hi (p - 4) = 2 * (zig-zag position of natural coefficient (kPairRow[p], j)): the byte
    // offsets of one block column inside a staged block, packed so the kernel spends two registers on them instead of eight
    uint32_t zz_lo, zz_hi;
    uint32_t pad[3];
};
static_assert(sizeof(F32Column) == 64, "one record per 64-byte line");

// Device-resident tables built by the host at context creation (jpezy_capi.hip).
struct DeviceTables {
    F32Column f32col[2][8];   // first: every field at an immediate offset from the table pointer
    // quantised DC as a function of the block's integer sample sum S in [-8192, 8192] (index S + 8192):
    // dcq[t][.] = int(((S * s) * s) / 4) / Q_t[0] with s = 1/sqrt(2), evaluated on the host in the reference's
    // exact FP64 order (ref encoder/jpezy_encoder.hpp:163,171).  16-bit entries: |dcq| reaches 1024 at Q_t[0] = 1
    int16_t dcq[2][16385];
    // encode variant 0: qscale[t][j][i] = cu(j) * cv(i) / (4 * Q_t[i*8+j]) * 2^qfrac_bits   (t: 0 luma, 1 chroma)
    double qscale[2][8][8];
    double rq_dc[2];          // 1 / Q_t[0]
    int qt[2][64];            // natural order
    double qinv[2][64];       // 1.0 / Q_t[k] (levels 2/3 of the f32 kernel)
    int qfrac_bits;           // encode variant 0: fraction width of its fixed-point quotients (qfrac_bits() above), one for both tables
};

// The exact-path counter is sharded over COUNTER_SHARDS words: thousands of waves adding to ONE word serialise
// at ~12 ns per atomic (88 per us, MI355X_MICROARCH.md 'dequeue') and held every wave slot until they drained.
constexpr int COUNTER_SHARDS = 1024;

// Waves per workgroup.  Waves never talk to each other (no s_barrier); the only effect of the grouping is which
// quads share a CU.  Measured on 4096^2 / 32x1080p encode: 2 waves (two adjacent quads = one 128-byte line of every
// pixel row) is ~4 % faster than 1 or 4.
#ifndef JPEZY_WPB
#define JPEZY_WPB 2
#endif
constexpr int WPB = JPEZY_WPB;

struct EncParams {
    const uint8_t* r;
    const uint8_t* g;
    const uint8_t* b;
    size_t plane_stride;      // bytes between frames of one plane
    int16_t* coeffs;
    size_t coeffs_per_frame;  // int16 elements
    const DeviceTables* tab;
    const int16_t* dcq_luma;         // &tab->dcq[0][0], &tab->dcq[1][0]: separate kernel arguments so that the f32 kernel's
    const int16_t* dcq_chroma;       // DC lookups are scalar-base + 32-bit-offset loads
    unsigned long long* fallback_count;
    int W, H, mcu_cols, mcu_rows, quads_per_row, n_frames;
    unsigned qpr_magic, qpr_shift;   // fast_div by quads_per_row
    int groups_per_row;              // f32 kernel: workgroups per MCU row, and fast_div by it (set by its launcher)
    unsigned gpr_magic, gpr_shift;
    // persistent f32 kernel (variant 2): groups of four quads over all frames of the launch, fast_div by the groups of one frame
    unsigned ps_total_groups, ps_groups_per_frame, gpf_magic, gpf_shift;
    // variant 3: quads over all frames of the launch, fast_div by the quads of one frame
    unsigned ps_total_quads, ps_quads_per_frame, qpf_magic, qpf_shift;
    // quantised DC without the table (f32::dc_formula, and the one-quad kernel's DC through the level-1 quantiser with dc_formula on the
    // flagged sums): fl(1 / Q_t[0]) and 1 / (2 Q_t[0]); 0: one of the two did not reproduce DeviceTables::dcq for these constants (checked
    // for every sum at context creation) and neither may be used
    float dc_rq[2], dc_bias[2];
    // Packed (interleaved) pixels, jpezy_fdct_quant_packed_dev: pix_bytes = 3 or 4 (0: planes).  r, g, b then point at the three channel
    // bytes of pixel (0, 0) of frame 0, pixel (x, y) of a channel lies x * pix_bytes + y * row_stride behind it and plane_stride is the
    // frame stride.  pix = the first byte of the buffer, swap_rb = blue comes first (the 16-byte load form de-interleaves whole words and
    // picks its v_perm selectors by it).  Only the packed kernel instances read these four; the planar ones are compiled as before.
    const uint8_t* pix = nullptr;
    unsigned row_stride = 0;
    int pix_bytes = 0, swap_rb = 0;
    // Planar YCbCr 4:2:0 input, jpezy_fdct_quant_ycc_dev (the YCC kernel instances only): r = the Y plane (rows row_stride apart, frames
    // plane_stride), g / b = the Cb / Cr samples (0, 0) -- rows c_row_stride apart, samples c_step (1: planes, 2: one interleaved plane),
    // frames c_frame_stride.  Appended behind every field the other instances read: their argument offsets are what they were.
    unsigned c_row_stride = 0;
    int c_step = 0;
    size_t c_frame_stride = 0;
    // YCbCr 4:2:2 input, jpezy_fdct_quant_ycc422_dev / jpezy_fdct_quant_yuv422_dev (jpezy_kernels_f32_422_ycc.hip only): the fields above
    // with CH = H.  y_step: bytes between the Y samples of a row -- 1 (planes) or 2 (packed macropixels: r, g, b then are the Y0, Cb, Cr
    // bytes of macropixel (0, 0), c_step is 4, both row strides and both frame strides are the buffer's and pix is its first byte).
    // yuv_format: the packed format (enum JPEZY_YUV_*), which picks the aligned load's v_perm selectors.  Behind every field the other
    // instances read, with defaults: their argument offsets are what they were.
    int y_step = 1, yuv_format = 0;
#ifdef JPEZY_TRACE
    unsigned long long* trace;       // development builds only (tools/profile/wave_trace.py): 4 words per wave
#endif
#ifdef JPEZY_DUMP_T
    float* dump_t;                   // development builds only (tools/measure/check_level1_bound.py): the f32 kernel's level-1
                                     // t = F * ks of every coefficient, coefficient-buffer layout, NATURAL order in a block
#endif
};

struct DecParams {
    const int16_t* coeffs;
    size_t coeffs_per_frame;
    uint8_t* r;
    uint8_t* g;
    uint8_t* b;
    size_t plane_stride;
    const double* dqscale;    // [3 comps][8 (u=lane col)][8 (v)] : cu*cv*Q[v*8+u] / 4   (dequant and the final / 4 folded in)
    const float* dqscale_f;   // [8 (u)][8 (v)]: the luma constants rounded to FP32 (tolerance mode)
    const int* dqt;           // [3 comps][64] natural order quant values (exact path)
    int coef_limit;           // raw coefficients above it send the wave to the exact path: 2^23 / largest quantiser (exact mode;
                              // >= 32768 = no test needed) or 2^15 / largest quantiser (tolerance mode)
    unsigned long long* fallback_count;
    int W, H, mcu_cols, mcu_rows, quads_per_row, n_frames;
    unsigned qpr_magic, qpr_shift;   // fast_div by quads_per_row (set by the launcher)
    // packed (interleaved) output, jpezy_dequant_idct_packed_dev: the same four fields as EncParams' (r, g, b = the channel bytes of pixel
    // (0, 0), plane_stride = the frame stride); the fourth byte of a 32-bit pixel is written as 0xFF
    uint8_t* pix = nullptr;
    unsigned row_stride = 0;
    int pix_bytes = 0, swap_rb = 0;
    // native planar YCbCr 4:2:0 output, jpezy_dequant_idct_ycc_dev: the same fields as EncParams' (r = Y, g = Cb, b = Cr; g == b == null:
    // luma only)
    unsigned c_row_stride = 0;
    int c_step = 0;
    size_t c_frame_stride = 0;
};

// (magic, shift) such that n / d == (((n - mulhi(n, magic)) >> 1) + mulhi(n, magic)) >> shift for all 32-bit n;
// magic == 0 encodes d == 1
inline void fast_div_setup(unsigned d, unsigned* magic, unsigned* shift)
{
    unsigned l = 0;
    while ((1ull << l) < d) ++l;                       // ceil(log2 d)
    *magic = (unsigned)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    *shift = l ? l - 1 : 0;
    if (d == 1) { *magic = 0; *shift = 0; }
}

hipError_t launch_fdct_quant(const EncParams& p, bool gray, bool force_exact, hipStream_t stream);
// variant 1: FP32 first level, FP64 second level, reference-order third level.  force: 0 normal, 1 every
// coefficient through the reference-order chain, 2 every coefficient through the FP64 second level, 3 every quad
// through the per-lane evaluator of the queue-overflow case.
// groups: the workgroup form, the values of enum jpezy_encode_groups (include/jpezy_hip.h; jpezy_capi.hip asserts that they agree).
// AUTO: the launcher's rule by the frame's geometry; a form that is not legal for the frame (fdct_quant_f32_groups_legal) is refused.
enum { ENC_GROUPS_AUTO = 0, ENC_GROUPS_4_COOP = 1, ENC_GROUPS_2_COOP = 2, ENC_GROUPS_2_DIRECT = 3 };
hipError_t launch_fdct_quant_f32(const EncParams& p, bool gray, int force, hipStream_t stream, int groups = ENC_GROUPS_AUTO);
bool fdct_quant_f32_groups_legal(const EncParams& p, int groups);
// the same two kernels for packed (interleaved) pixels (EncParams::pix_bytes != 0): the f32 one with a 16-byte load form that separates
// the channels in registers, the FP64 one through its byte loop
hipError_t launch_fdct_quant_f32_packed(const EncParams& p, bool gray, int force, hipStream_t stream);
hipError_t launch_fdct_quant_packed(const EncParams& p, bool gray, bool force_exact, hipStream_t stream);
bool packed_is_aligned16(const void* pix, int W, size_t row_stride, size_t frame_stride);
// the f32 kernel's colour launches with the averaged chroma stage (JPEZY_DOWNSAMPLE_AVERAGE; jpezy_kernels_f32_avg.hip): planes, packed pixels
hipError_t launch_fdct_quant_f32_avg(const EncParams& p, int force, hipStream_t stream);
hipError_t launch_fdct_quant_f32_packed_avg(const EncParams& p, int force, hipStream_t stream);
// ... and for planar YCbCr 4:2:0 samples (EncParams::c_step != 0): no colour conversion, the planes are the file's own sample domain
hipError_t launch_fdct_quant_f32_ycc(const EncParams& p, bool gray, int force, hipStream_t stream);
hipError_t launch_fdct_quant_ycc(const EncParams& p, bool gray, bool force_exact, hipStream_t stream);
// 4:4:4 (8 x 8 MCUs of Y, Cb, Cr) and 4:2:2 (16 x 8 MCUs of Y, Y, Cb, Cr; average: the averaged h2v1 chroma stage) from planes or packed
// pixels alike: quads_per_row counts work units of 8 MCUs (jpezy_f32_octet.h; jpezy_kernels_f32_444.hip, jpezy_kernels_f32_422.hip)
hipError_t launch_fdct_quant_f32_444(const EncParams& p, int force, hipStream_t stream);
hipError_t launch_fdct_quant_f32_422(const EncParams& p, int force, bool average, hipStream_t stream);
// 4:2:2 from YCbCr 4:2:2 samples, planar (EncParams::y_step 1, c_step 1 or 2) or packed macropixels (y_step 2): the same octets without
// a colour conversion (jpezy_kernels_f32_422_ycc.hip)
hipError_t launch_fdct_quant_f32_422_ycc(const EncParams& p, int force, hipStream_t stream);
// variant 2: the same arithmetic in persistent workgroups with LDS-DMA loader waves (jpezy_kernels_f32_ps.hip); frames whose rows do
// not divide into groups of four quads, or unaligned planes, go to variant 1's launch.  n_cus: compute units of the device.
hipError_t launch_fdct_quant_f32_ps(const EncParams& p, bool gray, int force, int n_cus, hipStream_t stream);
bool fdct_quant_f32_ps_applies(const EncParams& p);
// variant 3: persistent workgroups of 16 compute waves, every wave prefetching its next quad's pixels into registers; any frame
// with W % 16 == 0 and 16-byte aligned planes, anything else goes to variant 1's launch
hipError_t launch_fdct_quant_f32_ps2(const EncParams& p, bool gray, int force, int n_cus, hipStream_t stream);
// tolerant: luma in FP32 without guard band (samples within one of the reference's, jpezy_kernels_decode.hip); chroma stays exact
hipError_t launch_dequant_idct(const DecParams& p, bool gray, bool force_exact, bool tolerant, hipStream_t stream);
// the same kernel with the packed store stage (DecParams::pix_bytes != 0)
hipError_t launch_dequant_idct_packed(const DecParams& p, bool gray, bool force_exact, bool tolerant, hipStream_t stream);
// the same kernel with the native-sample store stage (DecParams::c_step != 0); gray: luma only
hipError_t launch_dequant_idct_ycc(const DecParams& p, bool gray, bool force_exact, bool tolerant, hipStream_t stream);

// any-layout decode (jpezy_kernels_generic.hip)
struct GenericDecParams {
    const int16_t* coeffs;
    int* samples;             // [block][64] natural order, scratch
    const int* qt;            // [3 comps][64] natural order
    uint8_t* r;
    uint8_t* g;
    uint8_t* b;
    int W, H, ncomp, gray;
    int ch[3], cv[3], hmax, vmax, mcu_cols, mcu_rows, blocks_per_mcu;
    int blk_start[3];         // first block of each component inside an MCU
    int level;                // level shift of inverse_dct: 128, or 2048 when SOF0 says precision != 8 (ref :654)
    unsigned mw_magic, mw_shift, mh_magic, mh_shift;        // fast_div by hmax*8, vmax*8 (set by the launcher)
    unsigned dx_magic[3], dx_shift[3], dy_magic[3], dy_shift[3];   // fast_div by hmax/H, vmax/V of each component
    const double* dqscale;    // [3 comps][8 (u)][8 (v)] cu*cv*Q/4 as for the fused kernel (fast path)
    int coef_limit;           // raw coefficients above it send their block to the reference-order path
    int force_exact;          // test hook: every block through the reference-order path
    unsigned long long* fallback_count;   // samples evaluated in reference order (sharded, COUNTER_SHARDS)
    // batch form: n_frames frames of ONE layout, size and set of quantiser tables; frame f's coefficients at coeffs + f * blocks * 64,
    // its samples at samples + f * blocks * 64, its planes at r/g/b + f * plane_stride (a multiple of 4)
    int n_frames = 1;
    size_t plane_stride = 0;
    // packed (interleaved) output: pix_bytes = 3 or 4 (0: planes); r, g, b = the channel bytes of pixel (0, 0), rows row_stride apart,
    // frames plane_stride apart (any value then); byte 3 of a 32-bit pixel = 0xFF
    int pix_bytes = 0;
    unsigned row_stride = 0;
    // native component planes (jpezy_decode_jpeg_ycc on a layout that is not this project's own): ycc != 0 -- r, g, b = sample (0, 0) of
    // component 0, 1, 2 (null: not written); rows row_stride (component 0) / c_row_stride apart, chroma samples c_step apart; no colour
    // conversion, no replication
    int ycc = 0, c_step = 1;
    unsigned c_row_stride = 0;
};
// stage2: a launcher that stands in for generic_rgb_kernel behind the unchanged generic_idct_kernel (same parameters, same grid:
// 256 pixels of four rows per workgroup, the frame in grid.z); null: generic_rgb_kernel / generic_ycc_kernel
typedef hipError_t (*GenericStage2)(const GenericDecParams& q, dim3 grid, hipStream_t stream);
hipError_t launch_dequant_idct_generic(const GenericDecParams& p, hipStream_t stream, GenericStage2 stage2 = nullptr);
// smooth (triangle-filter) chroma upsampling (jpezy_kernels_smooth.hip; include/jpezy_hip.h, CHROMA UPSAMPLING)
hipError_t launch_smooth_rgb(const GenericDecParams& q, dim3 grid, hipStream_t stream);
// packed YCbCr 4:2:2 macropixels in generic_rgb_kernel's place (jpezy_kernels_generic.hip; include/jpezy_hip_ycc422.h): q.r, q.g, q.b are the
// Y0, Cb, Cr bytes of macropixel (0, 0), rows q.row_stride, frames q.plane_stride apart
hipError_t launch_generic_yuv422(const GenericDecParams& q, dim3 grid, hipStream_t stream);
// frames of p's layout one pair of launches takes (the launcher loops over larger batches); 0: a frame too large for one launch
int generic_frames_per_launch(const GenericDecParams& p);

// reduced-size decode of any layout (jpezy_kernels_scaled.hip): an N x N inverse transform per block, N = 1 << log2n = 4, 2, 1
struct ScaledDecParams {
    const int16_t* coeffs;
    int* samples;             // [block][N*N], scratch
    const int* qt;            // [3 comps][64] natural order
    uint8_t* r;
    uint8_t* g;
    uint8_t* b;
    int Ws, Hs;               // the output: ceil(W * N / 8) x ceil(H * N / 8)
    int log2n, ncomp, gray;
    int ch[3], cv[3], hmax, vmax, mcu_cols, mcu_rows, blocks_per_mcu;
    int blk_start[3];         // first block of each component inside an MCU
    int level;                // 128, or 2048 when SOF0 says precision != 8 (ref :654)
    unsigned mw_magic, mw_shift, mh_magic, mh_shift;        // fast_div by hmax*N, vmax*N (set by the launcher)
    unsigned dx_magic[3], dx_shift[3], dy_magic[3], dy_shift[3];   // fast_div by hmax/H, vmax/V of each component
    // n_frames frames of ONE layout, size and set of quantiser tables: frame f's coefficients at coeffs + f * blocks * 64, its samples at
    // samples + f * blocks * N*N, its planes at r/g/b + f * plane_stride (any value that holds a plane)
    int n_frames = 1;
    size_t plane_stride = 0;
    // packed (interleaved) output as in GenericDecParams: pix_bytes = 3 or 4 (0: planes); r, g, b = the channel bytes of pixel (0, 0),
    // rows row_stride apart, frames plane_stride apart; byte 3 of a 32-bit pixel = 0xFF
    int pix_bytes = 0;
    unsigned row_stride = 0;
};
hipError_t launch_dequant_idct_scaled(const ScaledDecParams& p, hipStream_t stream);
// frames of p's layout one pair of launches takes (the launcher loops over larger batches); 0: a frame too large for one launch
int scaled_frames_per_launch(const ScaledDecParams& p);

// region-of-interest decode of any layout (jpezy_kernels_region.hip): a window of the picture at scale 8 / N, N = 1 << log2n = 8, 4, 2, 1,
// from the MCUs that intersect it -- one launch, no intermediate in device memory
struct RegionDecParams {
    const int16_t* coeffs;    // the WHOLE frame's coefficients; only the blocks of MCUs that intersect the window are read
    const int* qt;            // [3 comps][64] natural order
    uint8_t* r;               // byte (0, 0) of the window's output: planes w * h, or with pix_bytes != 0 the channel bytes of its first pixel
    uint8_t* g;
    uint8_t* b;
    int x, y, w, h;           // the window, in the coordinates of the picture at the requested scale
    int ux0, uy0, ucols, urows;   // the MCUs that intersect it: columns [ux0, ux0 + ucols), rows [uy0, uy0 + urows)
    int log2n, ncomp, gray;
    int ch[3], cv[3], hmax, vmax, mcu_cols, mcu_rows, blocks_per_mcu;
    int blk_start[3];         // first block of each component inside an MCU
    int level;                // 128, or 2048 when SOF0 says precision != 8 (ref :654)
    // n_frames frames of ONE layout, size and set of quantiser tables: frame f's coefficients at coeffs + f * blocks * 64, its output at
    // r/g/b + f * plane_stride (any value that holds a window)
    int n_frames = 1;
    // oriented output (include/jpezy_hip_orientation.h): != 0 launches the ORIENT instances -- bit 0 transpose, bit 1 mirror x, bit 2 mirror
    // y.  {x, y, w, h} is then the SOURCE-side rectangle of the oriented window (jpezy_orient_rect), the output is h x w pixels when
    // transposed (planes: rows h apart), and output pixel (u, v) -- transposed: (v, u) -- is source pixel (x + u, y + v), a mirrored axis
    // counted from the rectangle's far edge.  (It sits in the four bytes of padding in front of plane_stride: every other member, and the
    // second kernel argument of the smooth form, lies where it lay.)
    int orient = 0;
    size_t plane_stride = 0;
    // packed (interleaved) output as in ScaledDecParams: pix_bytes = 3 or 4 (0: planes, rows w apart); rows row_stride apart, frames
    // plane_stride apart; byte 3 of a 32-bit pixel = 0xFF
    int pix_bytes = 0;
    unsigned row_stride = 0;
};
static_assert(sizeof(RegionDecParams) == 168, "orient fills padding: the kernel arguments of the un-oriented instances do not move");
hipError_t launch_dequant_idct_region(const RegionDecParams& p, hipStream_t stream);

// a batch of crop windows (jpezy_kernels_region.hip): the windows of many files of ONE layout at ONE scale 8 / N in one launch; size, window,
// destination and quantiser tables are per file.  One descriptor per file, 64 bytes, read with scalar loads.
struct WindowDesc {
    unsigned long long coeff_off;   // int16 offset of the file's first coefficient (the WHOLE file's coefficients lie there)
    unsigned long long out_off;     // byte offset of the window's pixel (0, 0) behind WindowsParams::pix
    int qset;                       // index of the file's dequantiser set; oriented launches: | RegionDecParams::orient's bits << kWindowOrientShift
    int mcu_cols;                   // MCU columns of the file
    int x, y, w, h;                 // the window, in the coordinates of the picture at the launch's scale
    int ux0, uy0, ucols;            // the MCUs that intersect it: columns [ux0, ux0 + ucols), rows from uy0
    unsigned wg0;                   // index of the file's first workgroup; ascending over the table, workgroup wg0 + r * ucols + c = MCU (ux0 + c, uy0 + r)
    unsigned pad[2];                // windows_smooth_kernel: Ws, Hs -- the file's picture at the launch's scale; windows_kernel reads neither
};
static_assert(sizeof(WindowDesc) == 64, "one descriptor per 64-byte line");
// a launch has at most one dequantiser set per file and a slice at most 512 files (jpezy_ctx_set_windows_slice_files): qset needs 10 bits
constexpr int kWindowMaxFiles = 512, kWindowOrientShift = 28, kWindowQsetMask = (1 << kWindowOrientShift) - 1;
static_assert(kWindowMaxFiles <= kWindowQsetMask && (7 << kWindowOrientShift) > 0, "WindowDesc::qset holds a set index and three orientation bits");
struct WindowsParams {
    const int16_t* coeffs;
    const int* qsets;               // [sets][3 comps][64] natural order: the de-duplicated dequantiser sets of the launch's files
    const WindowDesc* desc;
    uint8_t* pix;
    unsigned n_desc, wg_base;       // wg_base: the first workgroup of this launch (set by the launcher)
    size_t row_stride;
    int log2n, ncomp, gray;
    int ch[3], cv[3], hmax, vmax, blocks_per_mcu;
    int blk_start[3];               // first block of each component inside an MCU
    int level;                      // 128, or 2048 when SOF0 says precision != 8 (ref :654)
    int pix_bytes, swap_rb;         // 3 or 4 bytes per pixel; swap_rb: blue is byte 0; byte 3 of a 32-bit pixel = 0xFF
};
// oriented: the ORIENT instances -- every descriptor holds the SOURCE-side rectangle and its file's bits in qset (above)
hipError_t launch_dequant_idct_windows(const WindowsParams& p, unsigned long long total_wg, hipStream_t stream, bool oriented = false);

// region and window-batch decode with smooth chroma upsampling (jpezy_kernels_region.hip; include/jpezy_hip.h, SMOOTH UPSAMPLING OF
// WINDOWS): the same parameters and grids as the two launchers above, and the picture's size Ws x Hs at the launch's scale -- an argument
// here, WindowDesc::pad[0], pad[1] of every file there.  Both must lie inside the file's MCU grid (jpezy_scaled_size of the file's size does)
hipError_t launch_dequant_idct_region_smooth(const RegionDecParams& p, int Ws, int Hs, hipStream_t stream);
hipError_t launch_dequant_idct_windows_smooth(const WindowsParams& p, unsigned long long total_wg, hipStream_t stream, bool oriented = false);

// a batch of windows, resized (jpezy_kernels_resized.hip; include/jpezy_hip.h, BATCH OF WINDOWS, RESIZED): the packed pixels of MANY windows
// of different sizes, each resampled to the launch's out_w x out_h.  One descriptor per file; a workgroup is one tile of kResampleTileW x
// kResampleTileH output pixels of one file and finds its file as windows_kernel's do.
constexpr int kResampleTileW = 64, kResampleTileH = 16;
// source rows the two-pass form of the stage holds in LDS (jpezy_resample_core.h): a tile's rows span less than
// (kResampleTileH - 1) * r + 2 * fsup * r + 1 source rows at a vertical ratio r >= 1, 42 at most for Lanczos (fsup 3) below r = 2
constexpr int kResampleTileRows = 44;
struct ResampleDesc {
    unsigned long long src_off;     // byte offset of the source window's pixel (0, 0) behind ResampleParams::src (a multiple of 4)
    unsigned long long dst_off;     // byte offset of the file's output pixel (0, 0) behind ResampleParams::dst
    unsigned xfc, xw, yfc, yw;      // the file's four tap tables, as indices into ResampleParams::taps: first | count << 16 per output index,
                                    // and the integer weights [out][k]
    int w, h;                       // the source window (what the tables were built for; the kernel needs neither for its addresses)
    int kx, ky;                     // weights per output column / row in the tables (ksize)
    int mirror;                     // output column i is column out_w - 1 - i of the unmirrored result
    unsigned wg0;                   // index of the file's first workgroup, ascending over the table
    unsigned tiled;                 // 1: every tile of the file spans at most kResampleTileRows source rows and runs the two-pass form
                                    // (read by the launches of launch_resample / launch_resample_tensor with tile == true only)
    unsigned pad;
};
static_assert(sizeof(ResampleDesc) == 64, "one descriptor per 64-byte line");
struct ResampleParams {
    const uint8_t* src;             // packed pixels of pix_bytes each, rows src_stride apart (a multiple of 4), every file's by its own height
    const int* taps;                // the launch's tap tables
    const ResampleDesc* desc;
    uint8_t* dst;
    unsigned n_desc, wg_base;       // wg_base: the first workgroup of this launch (set by the launcher)
    unsigned src_stride, dst_stride;
    int out_w, out_h;
    int pix_bytes;                  // 3 or 4; byte 3 of a 32-bit pixel is written as 0xFF and not read
};
// tile: the kernel instance that holds the two-pass form and takes it for the files with ResampleDesc::tiled; false: the direct loop for
// every file, whatever the descriptors say
hipError_t launch_resample(const ResampleParams& p, unsigned long long total_wg, hipStream_t stream, bool tile = false);

// the same stage with a tensor behind it (jpezy_kernels_resized_tensor.hip; include/jpezy_hip.h, BATCH OF WINDOWS, TENSOR OUTPUT): the three
// bytes of an output pixel become `channels` elements of `dtype`, (float)byte * scale[c] + bias[c] for the float types, element (c, y, x) of
// a file at dst + (ResampleDesc::dst_off + c*sc + y*sh + x*sw) * element size.  With it ResampleDesc::dst_off counts ELEMENTS (k * sn),
// ResampleParams::pix_bytes is 3 (the source's) and dst_stride is not read.  dtype: the values of JPEZY_DT_*.
enum { kTensorU8 = 0, kTensorF32 = 1, kTensorF16 = 2, kTensorBF16 = 3 };
struct TensorOut {
    float scale[3], bias[3];        // per channel; not read for kTensorU8
    unsigned long long sc, sh, sw;  // strides in elements
    int dtype, channels;            // channels: 3, or 1 (channel 0 alone)
};
hipError_t launch_resample_tensor(const ResampleParams& p, const TensorOut& t, unsigned long long total_wg, hipStream_t stream, bool tile = false);

// lossless transforms in the coefficient domain (jpezy_kernels_transform.hip; include/jpezy_hip.h, LOSSLESS TRANSFORMS): every output
// block is one source block, permuted (swap) and with some coefficients negated (mirror) -- pure data movement
struct XformParams {
    const int16_t* in;        // source frames, [src_rows][src_pitch][B][64] each
    int16_t* out;             // destination frames, [out_rows][out_cols][B][64] each; never overlaps in
    size_t in_frame, out_frame;   // int16 elements per frame
    int blocks_per_mcu;       // 6 (4:2:0: Y00 Y01 Y10 Y11 Cb Cr) or 3 (4:4:4)
    int src_pitch;            // MCU columns of the source buffer (its row pitch; >= C)
    int C, R;                 // MCU columns / rows of the source that are used (after trimming)
    int swap, mirror_x, mirror_y;
    int n_frames;
};
hipError_t launch_coeff_transform(const XformParams& p, hipStream_t stream);

#if defined(__HIPCC__)
// The reference's sample int(sum / 4 + sl) (ref decoder/jpezy_decoder.hpp:667) as its x86-64 build executes it: cvttsd2si truncates
// toward zero and gives INT_MIN for every value outside [-2^31, 2^31) and for NaN, where v_cvt_i32_f64 saturates (INT_MAX above the
// range: 255 instead of the reference's 0).  Every place where a reference-order sum becomes a sample goes through it; such sums
// leave the range only with 16-bit quantisers (|sum| / 4 up to 64 * 32768 * 65535 / 4 = 3.4e10).  The fast paths' samples stay
// below 2^28 by their coefficient gates and keep the plain conversion.  Same rule: oracle jo_ref_int.
__device__ __forceinline__ int ref_int(double x)
{
    return (x >= -2147483648.0 && x < 2147483648.0) ? (int)x : (int)0x80000000u;
}
#endif

}  // namespace jpezy_dev
