/*
 * jpezy_hip.h -- C-ABI of the MI355X (gfx950) baseline-JPEG hot path of falgon/jpezy.
 *
 * The reference has no FFI seam: its hot path is a set of private member functions of two class
 * templates.  This header is the seam a maintainer binds instead; every entry
 * point cites the reference code it replaces (paths relative to /root/reference/src/).
 *
 * Conventions: plain C, no exceptions cross the boundary.  Functions returning int give 0 on success
 * and a negative jpezy_status otherwise; jpezy_hip_last_error() (thread-local) says why.  The caller
 * owns every buffer it passes; the library owns streams and scratch inside the opaque context.  A
 * context is used by one thread at a time; distinct contexts (one per GPU) may run concurrently.
 * There is NO CPU fallback: without a HIP device every compute entry point fails with JPEZY_E_NODEVICE.
 *
 * Device pointers: every coefficient pointer handed to a *_dev / *_gpu entry point must be 16-byte aligned (the
 * kernels move coefficients as 16-byte accesses; one MCU is 768 or 512 bytes, so only the base matters) -- a
 * misaligned one is refused with JPEZY_E_BADARG.  Pixel planes may have any alignment (an unaligned kernel variant
 * takes them).
 * Streams: the *_dev entry points are asynchronous on the caller's stream and one context may be driven on several
 * streams by its one thread.  The context-wide device tables (dequantiser constants of jpezy_dequant_idct*_dev, the
 * cached JFIF header of jpezy_write_jpeg_gpu_dev) are rewritten only when the caller's tables / comment / size
 * change; the library then waits for the WHOLE device first (launches on other streams may still read them), and it
 * refuses (JPEZY_E_BADARG) to do so while `stream` is being captured into a hipGraph: make the first call with new
 * tables outside the capture.  The same holds for the scratch that lives in the context (the samples of the any-layout and
 * reduced-size decoders, the buffers and code tables of the entropy entry points): it grows by a free and an allocation, so a
 * call that needs more of it than the context holds is refused with JPEZY_E_BADARG inside a capture, before anything is freed,
 * allocated or enqueued -- make the first call of a context, and the first with larger frames or more of them, outside the capture.
 *
 * Coefficient buffer layout (both directions), per frame:
 *     int16_t coeffs[mcu_rows][mcu_cols][B][64]
 * MCUs row-major with mcu_cols = ceil(W/16), mcu_rows = ceil(H/16) (encoder/jpezy_encoder.hpp:55-56);
 * B = 6 blocks in the order Y0(top-left) Y1(top-right) Y2(bottom-left) Y3(bottom-right) Cb Cr
 * (jpezy_encoder.hpp:227-242), or B = 4 (Y0..Y3) when gray != 0 -- in GRAY_MODE the reference zeroes
 * the chroma blocks (jpezy_encoder.hpp:61-64) so they are not materialised; inside a block the 64
 * quantised coefficients are in ZIG-ZAG order: coeffs[n] = q[ZZ[n]] (jpezy.hpp:36-45).
 * Pixel planes are planar 8-bit r, g, b with row stride W, W*H bytes each (jpezy_encoder.hpp:105,266).
 * Packed pixels (the *_packed entry points at the end of this header): one interleaved buffer, 3 or 4 bytes per pixel, rows
 * row_stride bytes apart.
 */
#ifndef JPEZY_HIP_H
#define JPEZY_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jpezy_ctx jpezy_ctx;

enum jpezy_status {
    JPEZY_OK = 0,
    JPEZY_E_BADARG = -1,      /* null pointer, non-positive or > 65535 dimension, ...                */
    JPEZY_E_NODEVICE = -2,    /* no HIP device / device index out of range                           */
    JPEZY_E_HIP = -3,         /* a HIP runtime call failed (message in jpezy_hip_last_error)         */
    JPEZY_E_UNSUPPORTED = -4, /* decode layout other than jpezy's own 2x2,1x1,1x1 3-component files,
                                 or a DC coefficient outside int16 (the reference's int predictor)   */
    JPEZY_E_FORMAT = -5,      /* malformed JPEG / Huffman stream (the reference throws runtime_error) */
    JPEZY_E_NOSPACE = -6      /* output buffer too small                                             */
};

const char* jpezy_hip_last_error(void);
int jpezy_hip_device_count(void);
/* 1 when the library was built with a timing-probe switch that gives wrong results (development builds of tools/ab/ab_build.py,
 * jpezy_amd/csrc/jpezy_experiment.h); 0 for every build that may be shipped or tested. */
int jpezy_hip_is_experimental_build(void);

/* ---- context: one per GPU.  Owns a HIP stream, staging buffers and the device constant tables ---- */
jpezy_ctx* jpezy_ctx_create(int device);
void jpezy_ctx_destroy(jpezy_ctx* ctx);
int jpezy_ctx_sync(jpezy_ctx* ctx);
int jpezy_ctx_device(const jpezy_ctx* ctx);
void* jpezy_ctx_stream(const jpezy_ctx* ctx);   /* the context's own hipStream_t (non-blocking) */

/* ---- geometry helpers (jpezy_encoder.hpp:55-56) ---- */
int jpezy_mcu_cols(int W);
int jpezy_mcu_rows(int H);
size_t jpezy_coeff_count(int W, int H, int gray);   /* int16 elements per frame */

/*
 * ENCODE compute stage.  Replaces, for every MCU of every frame, the reference's
 *   encoder::make_YCC      (encoder/jpezy_encoder.hpp:90-144)   RGB->YCbCr, edge clamp, 2x2 decimation
 *   RGB::Y/Cb/Cr           (:244-256)                            truncating FP64 colour conversion
 *   encoder::DCT           (:146-166)                            8x8 FDCT, int(sum*cu*cv/4)
 *   encoder::quantization  (:168-172)                            Annex-K, C++ int division
 *   the ZZ read order of encode_huffman (:195,212)               zig-zag
 * i.e. everything in the MCU loop (:58-67) except encode_huffman.  Results are bit-identical to the
 * reference arithmetic evaluated in IEEE binary64 without contraction ("exactness").
 *
 * jpezy_fdct_quant: host buffers (what encoder::encode calls).  r,g,b: n_frames consecutive W*H planes.
 */
int jpezy_fdct_quant(jpezy_ctx* ctx, const uint8_t* r, const uint8_t* g, const uint8_t* b, int W, int H,
                     int gray, int n_frames, int16_t* coeffs);
/*
 * The host-buffer entry points (jpezy_fdct_quant, jpezy_dequant_idct, jpezy_encode_jpeg) stream: the call is cut into chunks of
 * about `n` bytes of input (default 4 MiB: MCU-row bands of a large frame, or several small frames) that flow through a ring of
 * pinned staging buffers -- upload of chunk c + 1, kernel of chunk c and download of chunk c - 1 overlap, PCIe runs in both
 * directions at once and the device footprint is the ring, not the batch (host path).  Tuning / test knob.
 */
void jpezy_ctx_set_host_chunk_bytes(jpezy_ctx* ctx, size_t n);
/*
 * jpezy_fdct_quant_dev: same, all pointers are DEVICE pointers; plane_stride = bytes between
 * consecutive frames of one plane (>= W*H); asynchronous on `stream`, a hipStream_t with HIP's own
 * meaning (NULL = the default stream; jpezy_ctx_stream() = the context's private stream).  Used by
 * batch drivers / the benchmark with inputs resident in HBM.
 * Frame counts: any n_frames > 0.  The frame index is a grid dimension, so a batch of more than 65535 frames is enqueued as
 * several launches of at most 65535 frames each (the same holds for jpezy_dequant_idct_dev and
 * jpezy_dequant_idct_generic_batch_dev); the host-buffer entry points cut their chunks without regard to that limit.
 */
int jpezy_fdct_quant_dev(jpezy_ctx* ctx, const uint8_t* d_r, const uint8_t* d_g, const uint8_t* d_b,
                         size_t plane_stride, int W, int H, int gray, int n_frames, int16_t* d_coeffs,
                         void* stream);

/*
 * DECODE compute stage.  Replaces, for every MCU, the reference's
 *   decoder::inverse_quantization (decoder/jpezy_decoder.hpp:645-650)
 *   decoder::inverse_dct          (:652-670)      int(sum/4 + 128), no clamp
 *   decode_mcu's replication      (:519-524)      nearest-neighbour chroma upsample
 *   decoder::make_rgb / to_r,g,b / revise_value (:531-578, 672-676)
 * for files with jpezy's own layout (3 components, sampling 2x2,1x1,1x1, 8-bit).  qt: four 64-entry
 * tables in NATURAL order (as analyze_dqt leaves them, :258-277); comp_tq[c] selects the table of
 * component c (Frame_component::Tq).  gray != 0 is GRAY_MODE: r = g = b = clamp(Y) (:561); coeffs keep
 * the 6-block layout (a decoded file always carries chroma blocks).
 */
int jpezy_dequant_idct(jpezy_ctx* ctx, const int16_t* coeffs, const uint16_t qt[4][64],
                       const uint8_t comp_tq[3], int W, int H, int gray, int n_frames, uint8_t* r,
                       uint8_t* g, uint8_t* b);
int jpezy_dequant_idct_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64],
                           const uint8_t comp_tq[3], size_t plane_stride, int W, int H, int gray,
                           int n_frames, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream);

/*
 * DECODE compute stage for ANY baseline layout the reference's decode_mcu handles (decoder/jpezy_decoder.hpp:504-565):
 * 1 or 3 components, sampling factors 1..4 per direction (block placement as decode_mcu does it, :516-524), any table selectors.  coeffs as jpezy_read_jpeg delivers them
 * ([mcu][component blocks, ky outer, kx inner][64], zig-zag).  Blocks go through a fast FP64 inverse transform with a
 * guard band; a block with a sample inside the band is recomputed in the reference's own order (the 64-term sum, one
 * sample per lane), then the replication upsample and make_rgb run one thread per four pixels -- correct for every
 * layout, about a third of the speed of jpezy_dequant_idct, which handles jpezy_encode's own 2x2,1x1,1x1 files in one pass.
 * With ncomp == 1 the missing chroma planes read 0x80 as in the reference (:104-105).
 */
int jpezy_dequant_idct_generic(jpezy_ctx* ctx, const int16_t* coeffs, const uint16_t qt[4][64], int ncomp,
                               const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3], int W, int H,
                               int gray, uint8_t* r, uint8_t* g, uint8_t* b);
/*
 * The same on device memory, asynchronous on `stream` (a hipStream_t): d_coeffs as jpezy_read_jpeg_gpu leaves them,
 * d_r, d_g, d_b planes of W*H bytes.  precision: the SOF0 sample precision (8, or anything else for the reference's
 * 2048 level shift, decoder/jpezy_decoder.hpp:654).  The intermediate samples live in the context: one call in flight per
 * context.
 */
int jpezy_dequant_idct_generic_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp,
                                   const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision,
                                   int W, int H, int gray, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream);

/*
 * The same for n_frames frames of ONE layout, size and set of quantiser tables in one pair of launches (the loop a caller with many
 * small files of a layout would otherwise run): frame f's coefficients at d_coeffs + f * (blocks of a frame) * 64, its planes at
 * d_r/d_g/d_b + f * plane_stride (>= W*H, a multiple of 4).  jpezy_decode_jpeg_batch uses it for the layouts that are not jpezy's own.
 * Any n_frames > 0: batches of more than 65535 frames go out as several pairs of launches (the frame index is a grid dimension).
 */
int jpezy_dequant_idct_generic_batch_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp,
                                         const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision,
                                         int W, int H, int gray, int n_frames, size_t plane_stride, uint8_t* d_r, uint8_t* d_g,
                                         uint8_t* d_b, void* stream);

/* Test hook: route EVERY coefficient / sample through the kernels' exact-order fallback (the path a
 * guard-band hit takes).  0 = normal, 1 = reference-order path, 2 = (encode variant 1 only) the FP64 second
 * level, which may still defer to the reference-order path, 3 = (encode variant 1 only) the per-lane evaluator a
 * quad falls back to when it has more guard-band hits than its queue holds.  Exists so the rare branches have
 * parity tests. */
void jpezy_ctx_set_force_exact(jpezy_ctx* ctx, int on);
/* Encode kernel variant: 0 = FP64 butterflies (round-1 kernel), 1 = packed-FP32 first level + FP64 second level +
 * reference-order third level, one quad of four MCUs per wave (the default).  Two independently written kernels with proven error
 * bounds that must agree bit for bit (tests/test_gpu_parity.py runs every case through both).
 * 2 and 3 are LABORATORY variants, present only in libraries built with -DJPEZY_WITH_LAB (python -m jpezy_amd._build --lab;
 * tools/ab/ab_build.py): variant 1's arithmetic in persistent workgroups -- 2: loader waves stream the pixels into an LDS ring by
 * LDS-DMA, 3: sixteen computing waves per CU prefetch their next quad into registers (frames whose rows divide into groups of 16
 * MCUs and 16-byte aligned planes; anything else is handed to variant 1's launch).  Both are parity-green and were measured NOT
 * faster than variant 1 (docs/ROUND5.md), so the shipped library does not contain them: it answers JPEZY_E_UNSUPPORTED and keeps
 * the context's kernel.  Returns JPEZY_OK, JPEZY_E_BADARG (no such variant) or JPEZY_E_UNSUPPORTED.  tests/test_gpu_persistent.py. */
int jpezy_ctx_set_variant(jpezy_ctx* ctx, int variant);
/* Workgroup form of encode variant 1's launch for planar RGB / gray 4:2:0 frames with point-sampled chroma (jpezy_fdct_quant[_dev],
 * jpezy_encode_jpeg; no other launch consults it).  AUTO (default): chosen per launch from the frame's geometry.  The other three force
 * one form, for tests and A/B measurements -- the results are the same bits in every form:
 *   4_COOP    four quads per workgroup, pixels fetched cooperatively in 256-byte row pieces; legal where W % 16 == 0, the planes and
 *             their stride are 16-byte aligned and the quads of a row divide by four
 *   2_COOP    two quads per workgroup, fetched cooperatively in 128-byte row pieces; legal under the same alignment, any quad count
 *   2_DIRECT  two quads per workgroup, every lane loads its own 16 pixels; always legal
 * The setter returns JPEZY_E_BADARG for a value that names no form; a launch whose frame the forced form is not legal for returns
 * JPEZY_E_BADARG and launches nothing.  tests/test_gpu_encode_groups.py. */
enum jpezy_encode_groups { JPEZY_ENCODE_GROUPS_AUTO = 0, JPEZY_ENCODE_GROUPS_4_COOP = 1, JPEZY_ENCODE_GROUPS_2_COOP = 2, JPEZY_ENCODE_GROUPS_2_DIRECT = 3 };
int jpezy_ctx_set_encode_groups(jpezy_ctx* ctx, int groups);
int jpezy_ctx_encode_groups(const jpezy_ctx* ctx);
/*
 * Decode tolerance (opt-in; default 0).  BASELINE.json's north_star asks of the decoder "PPM output within +-1 LSB per
 * channel"; the default kernels deliver more (every byte equal to the reference's truncating FP64 arithmetic,
 * decoder/jpezy_decoder.hpp:652-676).  With on = 1, jpezy_dequant_idct[_dev] and jpezy_decode_jpeg[_batch] (jpezy's own
 * 2x2,1x1,1x1 layout) run the LUMA inverse transforms as FP32 butterflies without guard band or exact path: a luma
 * sample equals the reference's or differs from it by one, chroma samples, colour conversion and clamping stay
 * bit-exact, so every output byte is within one of the reference's (a unit on Cb would be 1.77 on B: chroma is never
 * relaxed).  Waves that hold out-of-range coefficients (|c * Q| > 2^15) still take the exact path.  Returns 0 or
 * JPEZY_E_BADARG.
 */
int jpezy_ctx_set_decode_tolerance(jpezy_ctx* ctx, int on);
/* Synchronises the device and returns how many coefficients/samples were resolved through the
 * exact-order fallback on this context since the previous call (the counter is then reset); -1 on error */
long jpezy_ctx_last_fallback_count(jpezy_ctx* ctx);

/*
 * HOST serial tail / head (stay on the CPU per BASELINE.json north_star).
 *
 * jpezy_write_jpeg replaces jpezy_writer::write_header/write_eoi (encoder/jpezy_writer.hpp:20-105) and
 * encoder::encode_huffman (encoder/jpezy_encoder.hpp:174-225) with the Annex-K tables of
 * encoder/huffman_table.hpp.  comment may be NULL/"" (no COM segment).  Returns bytes written (the
 * value encoder::encode returns, :76) or a negative status.
 */
long jpezy_write_jpeg(const int16_t* coeffs, int W, int H, int gray, const char* comment, uint8_t* out,
                      size_t cap);
/*
 * Per-image optimised Huffman tables (what libjpeg calls `optimize`): the same coefficients and the same decoded pixels in a smaller
 * file.  The four DHT segments then hold the frame's own tables, built from its symbol counts exactly as ITU-T T.81 Annex K.2
 * states (Figures K.1 - K.4, a reserved symbol so that no code is all ones, every tie toward the larger symbol value, no code longer
 * than 16 bits).  jpezy_write_jpeg_opt is jpezy_write_jpeg with such tables, on the host; the GPU coder writes the same bytes when
 * jpezy_ctx_set_huffman_optimize is on.  A value outside the code tables is JPEZY_E_FORMAT, as for jpezy_write_jpeg.
 */
long jpezy_write_jpeg_opt(const int16_t* coeffs, int W, int H, int gray, const char* comment, uint8_t* out,
                          size_t cap);
/*
 * The table construction alone (pure host function): freq[sym] = how often symbol sym occurs -> bits[l - 1] = codes of length l,
 * vals = the symbols in order of code length, then ascending value (a DHT segment's two arrays).  Returns the number of symbols
 * (those with a non-zero count) or JPEZY_E_BADARG.  A single used symbol gets the one-bit code 0.
 */
int jpezy_huffman_optimal_table(const unsigned long long freq[256], uint8_t bits[16], uint8_t vals[256]);
/*
 * jpezy_write_jpeg with restart intervals (ITU-T T.81 B.2.4.4, E.1.4): restart_interval = MCUs per interval, 0..65535, anything
 * else is JPEZY_E_BADARG.  0: no DRI segment and no RSTn marker -- the bytes of jpezy_write_jpeg (optimize = 0) or
 * jpezy_write_jpeg_opt (optimize != 0).  Otherwise a DRI segment FF DD 00 04 hi lo stands directly in front of SOS; behind every
 * interval but the last the bits are padded to a byte with JPEZY_PAD_BIT (the fill the frame's last byte gets: with the default 0 a
 * padded byte cannot be 0xFF, in a JPEZY_PAD_BIT 1 build a padded 0xFF is stuffed like any other) and the marker FF D0+(k mod 8)
 * follows interval k, never stuffed; the three DC predictors are zero at the start of every interval.  Nothing follows the last
 * interval but the usual pad and EOI, so restart_interval >= the MCU count writes the DRI segment and no marker.
 * optimize != 0: the frame's own tables (Annex K.2) from the symbols THIS scan emits -- the DC difference at an interval's start
 * is taken against 0, so the counts differ from those of the file without restarts.
 * The comment may be at most JPEZY_MAX_COMMENT_RESTART bytes when restart_interval > 0.  The GPU coder writes the same bytes with
 * jpezy_ctx_set_restart_interval.
 */
long jpezy_write_jpeg_rst(const int16_t* coeffs, int W, int H, int gray, const char* comment, int restart_interval,
                          int optimize, uint8_t* out, size_t cap);
/*
 * The longest comment (bytes before the terminating NUL) any writer accepts: jpezy_write_jpeg[_batch], jpezy_write_jpeg_gpu[_batch,
 * _dev], jpezy_encode_jpeg and jpezy_multi_encode / jpezy_encode_batch_multi all refuse a longer one with JPEZY_E_BADARG.  It is
 * what makes the header fit 1024 bytes: 623 bytes of markers and tables + a COM segment of n + 5 bytes (marker, length, text, NUL).
 */
#define JPEZY_MAX_COMMENT 396
/*
 * With a restart interval (jpezy_ctx_set_restart_interval, jpezy_write_jpeg_rst) the header also holds the six bytes of the DRI
 * segment, which come out of the comment's room: a longer comment is then JPEZY_E_BADARG.  JPEZY_MAX_COMMENT itself does not change.
 */
#define JPEZY_MAX_COMMENT_RESTART 390
/*
 * A cap that always suffices for a comment of up to JPEZY_MAX_COMMENT bytes: 1024 bytes of header + 2688 bytes per MCU.  The worst
 * MCU codes 4 x 1658 + 2 x 1660 bits (every AC coefficient a 16-bit code + 10 value bits, the DC difference 9 or 11 + 11 bits), i.e.
 * 1244 bytes, 2488 if every byte were 0xFF and stuffed; the pad bits (one byte, two if stuffed) and the 2-byte EOI fit in the
 * 200 bytes per MCU left over (tests/test_jpeg_bound.py).
 * With per-image tables (jpezy_write_jpeg_opt, jpezy_ctx_set_huffman_optimize) a DC code is at most 12 bits (12 categories + the
 * reserved symbol: 13 leaves) and an AC code at most 16: a block is at most 12 + 11 + 63 x 26 = 1661 bits, an MCU 9966 bits = 1246
 * bytes, 2492 stuffed -- still within 2688; and no table has more symbols than its Annex-K counterpart (12 / 162), so the header is
 * never longer.  The same bound holds (tests/test_huffopt_host.py).
 * With restart intervals every interval but the last adds at most a pad byte (two if it is 0xFF and stuffed) and the 2-byte RSTn
 * marker: at the shortest interval of one MCU that is at most 4 bytes per MCU, which together with the frame's own pad and EOI
 * (4 bytes, once) still fit in the 196 bytes per MCU that 2492 leaves of 2688; the six DRI bytes come out of the comment's room
 * (JPEZY_MAX_COMMENT_RESTART).  The same bound holds (tests/test_restart_host.py).
 */
size_t jpezy_jpeg_bound(int W, int H);
/*
 * The same serial tail for a batch of independent frames, spread over `threads` host threads (0 = all cores):
 * frame f reads coeffs + f*jpezy_coeff_count(W,H,gray) and writes at most `cap` bytes at out + f*cap; sizes[f]
 * receives the bytes written or a negative status.  Returns 0 if every frame succeeded.  Frames are independent
 * (pre_DC and the bit cursor are per file, encoder/jpezy_encoder.hpp:180-181), so this is plain host parallelism.
 */
int jpezy_write_jpeg_batch(const int16_t* coeffs, int W, int H, int gray, int n_frames, const char* comment,
                           uint8_t* out, size_t cap, long* sizes, int threads);

/*
 * The same tail on the GPU ("entropy coding off the critical path"): coefficients already in device
 * memory (the output of jpezy_fdct_quant_dev), bytes identical to jpezy_write_jpeg.  pre_DC (encoder/jpezy_encoder.hpp:
 * 180-181) becomes a read of the previous block's DC and the bit cursor a prefix sum of the blocks' code lengths (every
 * block is coded once; the sum is formed per 256 blocks and across them afterwards); the 0xFF00 stuffing of the reference's
 * bofstream is a second prefix sum.  out/sizes are host memory: frame f writes at
 * most cap bytes at out + f*cap and sizes[f] receives its length or a negative status.  Synchronous.
 * Frame counts (here and in jpezy_write_jpeg_gpu_dev): any n_frames > 0.  The batch is coded in passes of at most 65535 frames (the
 * frame index is a grid dimension) and at most 1 GiB of worst-case stream (208 bytes per block; at least one frame per pass).
 */
long jpezy_write_jpeg_gpu(jpezy_ctx* ctx, const int16_t* d_coeffs, int W, int H, int gray, const char* comment,
                          uint8_t* out, size_t cap);
int jpezy_write_jpeg_gpu_batch(jpezy_ctx* ctx, const int16_t* d_coeffs, int W, int H, int gray, int n_frames,
                               const char* comment, uint8_t* out, size_t cap, long* sizes);
/*
 * Device-resident, asynchronous form of the same: everything is enqueued on `stream` (HIP semantics, NULL = default
 * stream; the coefficients must have been produced on it or be complete), nothing is copied to the host, no host
 * synchronisation.  Frame f's complete file (header, entropy-coded segment, EOI) is written at d_out + f*out_stride
 * and d_sizes[f] (device memory) receives its length, JPEZY_E_FORMAT or JPEZY_E_NOSPACE (out_stride too small; nothing
 * is written past it).  Scratch is sized for the worst case of 208 bytes per block and LIVES IN THE CONTEXT (the tile
 * streams, their bit totals, the unstuffed stream): calls of the entropy entry points (this one, jpezy_write_jpeg_gpu[_batch],
 * jpezy_encode_jpeg, jpezy_read_jpeg_gpu, jpezy_decode_jpeg) on one context must not overlap in time -- issue them on one
 * stream or order the streams with events; frames that are to be in flight together need a context each.
 */
int jpezy_write_jpeg_gpu_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, int W, int H, int gray, int n_frames,
                             const char* comment, uint8_t* d_out, size_t out_stride, long long* d_sizes, void* stream);
/*
 * Per-image optimised Huffman tables on the GPU path (opt-in; default 0).  With on = 1, jpezy_write_jpeg_gpu, jpezy_write_jpeg_gpu_batch,
 * jpezy_encode_jpeg and jpezy_encode_jpeg_packed write the bytes of jpezy_write_jpeg_opt: a kernel counts every frame's symbols, the
 * host builds the frame's four tables from the counts (one extra synchronisation and two small copies per call) and the coder runs
 * with a table image per frame; every frame of a batch gets its own DHT segments.  With on = 0 every byte is what it was.
 * Restrictions: jpezy_write_jpeg_gpu_dev returns JPEZY_E_UNSUPPORTED while the setting is on (the tables are built on the host and
 * that call is asynchronous); the multi-GPU handle (jpezy_multi_*, jpezy_encode_batch_multi) owns its contexts and always writes
 * Annex-K tables.  Returns 0 or JPEZY_E_BADARG.
 */
int jpezy_ctx_set_huffman_optimize(jpezy_ctx* ctx, int on);
/*
 * Restart intervals on the GPU path (opt-in; default 0 = none).  With mcus > 0, jpezy_write_jpeg_gpu, jpezy_write_jpeg_gpu_batch,
 * jpezy_write_jpeg_gpu_dev, jpezy_encode_jpeg and jpezy_encode_jpeg_packed write the bytes of jpezy_write_jpeg_rst(..., mcus,
 * optimize, ...) with optimize = the context's jpezy_ctx_set_huffman_optimize setting, and jpezy_huffman_histogram_dev counts with
 * the predictors reset at every interval's start.  Every value 1..65535 is coded on the GPU at every frame size.  The coder's
 * workgroups never straddle an interval (an interval takes ceil(6 * mcus / 256) of them), so an interval of an MCU row or longer
 * costs one more launch than no interval (about 10 us on a 4096 x 4096 frame), while short intervals leave most lanes of a workgroup
 * idle (one MCU per interval: 10 to 15 times the time; DESIGN.md 4.6 has the figures).
 * jpezy_write_jpeg_gpu_dev stays asynchronous and capturable.  With 0 every byte is what it was.  A comment longer than
 * JPEZY_MAX_COMMENT_RESTART is refused with JPEZY_E_BADARG while the setting is non-zero.
 * The multi-GPU handle (jpezy_multi_*, jpezy_encode_batch_multi) owns its contexts and always writes files without restart
 * intervals.  jpezy_ctx_set_restart_interval returns 0, or JPEZY_E_BADARG for a value outside 0..65535;
 * jpezy_ctx_restart_interval returns the setting (JPEZY_E_BADARG for a null context).
 */
int jpezy_ctx_set_restart_interval(jpezy_ctx* ctx, int mcus);
int jpezy_ctx_restart_interval(const jpezy_ctx* ctx);
/*
 * Quality and caller-supplied quantisation tables (opt-in; default: the Annex-K tables of jpezy.hpp:131-152, libjpeg's quality 50).
 * The reference has no such setting, so the definition is this project's own: two tables of 64 entries in NATURAL order, luma and
 * chroma, every entry in 1..255 (the file stays baseline, Pq = 0).  The coefficients are those of the reference's MCU loop
 * (encoder/jpezy_encoder.hpp:58-67, :90-172) with quantization(cs) (:168-172) dividing by the caller's table instead of
 * YQuantumTb / CQuantumTb: blk[i] /= qt[cs][i], C's truncating int division, every coefficient bit for bit -- both encode variants,
 * every force_exact level, planar, packed and YCbCr input.  The file is the writer's for those coefficients with the caller's tables
 * in the two DQT segments (jpezy_writer.hpp:46-58: luma as table 0, chroma as table 1, zig-zag order); optimised Huffman tables and
 * restart intervals compose with it unchanged.
 *
 * jpezy_quality_tables (pure host function): libjpeg's mapping for an integer quality 1..100 -- s = q < 50 ? 5000 / q : 200 - 2 q,
 * entry = clamp((base * s + 50) / 100, 1, 255) in integer arithmetic, base = the Annex-K tables.  Quality 50 is Annex K itself, 1 is
 * 255 everywhere, 100 is 1 everywhere.  JPEZY_E_BADARG for a quality outside 1..100 or a null pointer.
 *
 * jpezy_ctx_set_quant_tables: the setting of every encode entry of the context -- jpezy_fdct_quant[_dev], jpezy_fdct_quant_packed_dev,
 * jpezy_fdct_quant_ycc_dev, jpezy_encode_jpeg[_packed, _ycc], and the DQT segments of the header jpezy_write_jpeg_gpu[_batch, _dev]
 * write (those three code the coefficients they are given, whatever tables produced them).  Both pointers null: back to Annex K.
 * JPEZY_E_BADARG for one null pointer of two or a zero entry.  A context that never calls it, or that sets quality 50 or the Annex-K
 * tables, writes every byte it wrote before and launches the same kernels.  The device constants are rewritten only when the
 * setting changes, and then under the rule of the dequantiser tables: the call waits for the whole device (launches on any stream may
 * still read them) and is refused with JPEZY_E_BADARG, the context unchanged, while the context's stream is being captured.
 * jpezy_write_jpeg_gpu_dev stays asynchronous and capturable once the tables are in place (its first call with a new header uploads it).
 * jpezy_ctx_set_quality is jpezy_quality_tables + jpezy_ctx_set_quant_tables; jpezy_ctx_quant_tables reads the setting back.
 *
 * jpezy_write_jpeg_qt: the host writer (jpezy_write_jpeg_rst) with the tables of the DQT segments; null tables give the bytes of
 * jpezy_write_jpeg_rst.  The coefficients are written as they are.
 *
 * Value range: at Q = 1 an AC coefficient reaches 1020 (size 10) and a DC difference 2038 (category 11): inside the code tables, so no
 * table makes 8-bit input JPEZY_E_FORMAT, and jpezy_jpeg_bound does not depend on the tables.  Small quantisers cost time: more
 * coefficients are non-zero and more fall into the kernels' guard bands (DESIGN.md 4.10 has the figures).
 * Out of scope: the multi-GPU handle (jpezy_multi_*, jpezy_encode_batch_multi) owns its contexts and always writes Annex-K tables;
 * jpezy_write_jpeg[_opt, _rst, _batch] keep their signatures and bytes; no per-frame tables inside one batch call; no 16-bit tables;
 * chroma sampling is an argument of the *_sampling entry points (end of this header), not a context setting.
 */
int jpezy_quality_tables(int quality, uint8_t luma[64], uint8_t chroma[64]);
int jpezy_ctx_set_quant_tables(jpezy_ctx* ctx, const uint8_t luma[64], const uint8_t chroma[64]);
int jpezy_ctx_set_quality(jpezy_ctx* ctx, int quality);
int jpezy_ctx_quant_tables(const jpezy_ctx* ctx, uint8_t luma[64], uint8_t chroma[64]);
long jpezy_write_jpeg_qt(const int16_t* coeffs, int W, int H, int gray, const char* comment, const uint8_t luma[64],
                         const uint8_t chroma[64], int restart_interval, int optimize, uint8_t* out, size_t cap);
/*
 * Diagnostic (pure host function): what jpezy_ctx_set_quant_tables would build for these tables (null, null: Annex K), in place of
 * quantization(cs) (encoder/jpezy_encoder.hpp:168-172) -- delta1[t][j] = the level-1 guard band of block column j of table t,
 * dc_generic[t] = 1 when both create-time checks allow the DC of table t through the level-1 quantiser (0: the kernels read the
 * DC from the exact table; one 0 sends both tables there), *qfrac_bits = the fraction width of encode variant 0's fixed point.
 * Any output pointer may be null.  JPEZY_E_BADARG as for the setter, and for tables whose guard band would reach 0.25 (none can).
 * Test hook beside jpezy_ctx_set_force_exact: jpezy_ctx_set_dc_table_lookup(ctx, 1) makes the context's encode kernels read the DC
 * from that table even where the checks pass, so that the lookup has parity tests at every table.
 */
int jpezy_quant_tables_probe(const uint8_t luma[64], const uint8_t chroma[64], float delta1[2][8], int dc_generic[2], int* qfrac_bits);
void jpezy_ctx_set_dc_table_lookup(jpezy_ctx* ctx, int on);
/*
 * The symbol-counting kernel on its own, asynchronous on `stream`: d_hist[f][k][sym] (device memory, [n_frames][4][256], zeroed
 * here) = how often the coder emits symbol sym from table k (DHT order: 0 YDc, 1 CDc, 2 YAc, 3 CAc) for frame f.  A value outside
 * the code tables is counted as the clamped symbol the coder would emit (size 10, category 11).
 */
int jpezy_huffman_histogram_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, int W, int H, int gray, int n_frames,
                                unsigned long long* d_hist, void* stream);
/*
 * encoder::encode end to end (encoder/jpezy_encoder.hpp:38-77) with both stages on the GPU: host planar r,g,b in,
 * host .jpg bytes out; returns the byte count (the value encoder::encode returns) or a negative status.
 */
long jpezy_encode_jpeg(jpezy_ctx* ctx, const uint8_t* r, const uint8_t* g, const uint8_t* b, int W, int H, int gray,
                       const char* comment, uint8_t* out, size_t cap);

/*
 * MULTI-GPU, one host process (north_star: "host C++ ... partition the input batch and gather ... over xGMI").
 *
 * jpezy_shard_range: the partition rule of every batch entry point and of jpezy_amd/sharding.py -- shard k of n_shards owns the
 * contiguous units [*first, *first + *count) of n_units; counts differ by at most one, the earlier shards take the extra.
 *
 * jpezy_multi_create / jpezy_multi_encode / jpezy_multi_destroy: encoder::encode (encoder/jpezy_encoder.hpp:38-77) for n_frames
 * independent frames of one size, i.e. the loop a caller of the reference runs over encoder objects, spread over the n_dev GPUs
 * devices[0..n_dev) of this node; devices[0] is the ROOT (the calling thread drives it, one more host thread per further device).
 * The HANDLE owns, per entry of devices (a "lane"): a context, an upload stream, download streams and a ring of six slots, each a pinned
 * host buffer + a device buffer per direction, sized for chunk_frames frames (<= 0: about 28 MB of planes per chunk: 4 frames of 1080p,
 * one 4096^2 frame).  Nothing is allocated inside jpezy_multi_encode once the handle has served one call of the same shape, so a caller
 * with a stream of batches creates it once.  A call shards its frames over the lanes (jpezy_shard_range, any n_frames > 0, it may change
 * from call to call) and every lane streams its shard through its ring: feeder threads copy the caller's planes into pinned slots and
 * start the uploads, the lane's thread enqueues FDCT + Huffman stage per chunk, drainer threads bring the results back at their real
 * length -- upload of chunk c + 1, kernels of chunk c and download of chunk c - 1 overlap, PCIe runs in both directions.  The caller's
 * PAGEABLE memory never reaches the DMA engines (uploads straight from it run at an eighth of the link's rate); planes the caller has
 * pinned itself (hipHostMalloc / hipHostRegister; detected with hipPointerGetAttributes) are uploaded as they are, without the copy.
 * r, g, b: host memory, n_frames consecutive W*H planes each.  out says what is wanted and where:
 *   coeffs      NULL, or room for n_frames * jpezy_coeff_count(W, H, gray) int16 (the layout of jpezy_fdct_quant)
 *   jpg         NULL, or n_frames * jpg_stride bytes: frame f's complete file at jpg + f * jpg_stride (MCU loop AND Huffman tail on
 *               the frame's GPU, only the finished file travels, at its real length); jpg_sizes[f] (HOST memory, n_frames entries)
 *               receives its length, JPEZY_E_FORMAT or JPEZY_E_NOSPACE (jpg_stride too small for it)
 *   on_root_device  0: coeffs / jpg are HOST memory -- every device delivers its shard over its own PCIe link;
 *                   1: they are memory of devices[0] (coeffs 16-byte aligned) -- the consumer runs on that GPU: the other devices'
 *                      results are gathered into it chunk by chunk with hipMemcpyPeerAsync (xGMI between the GPUs of a node), the
 *                      root's own chunks are written in place.
 * THE GATHER IS hipMemcpyPeerAsync, NOT RCCL (north_star says "gather coefficient buffers with RCCL over xGMI"): one host process owns
 * every device here, so a peer copy is the point-to-point transfer over the same xGMI link, with no communicator to build, no
 * rendezvous and no second library in the link line of a C++ caller.  The one-process-per-GPU harness (jpezy_amd/sharding.py,
 * bench.py --gpus N) is where RCCL moves the same buffers (send/recv to the consumer rank).
 * An index may appear more than once in devices (several lanes on one GPU, each with its own context and streams): that is how the
 * multi-lane path is exercised on a one-GPU box (tests/test_gpu_multi.py).  jpezy_multi_encode returns JPEZY_OK, or the first failing
 * lane's code (message: which device and why); JPEZY_E_FORMAT when every lane ran but a frame was refused (see jpg_sizes).  Synchronous;
 * one call at a time per handle; the calling thread's current HIP device is what it was on return.
 * jpezy_multi_last_stats: per lane of the last call -- frames, wall time, the GPU time of its kernels (sum over its chunks, HIP
 * events), bytes uploaded and brought back, whether the planes were staged (1) or were the caller's pinned memory (0); returns the
 * number of lanes, fills at most cap entries.  jpezy_multi_chunk_frames: the chunk size the handle settled on.
 * jpezy_multi_feeder_threads / jpezy_multi_set_feeder_threads: the staging threads per lane (a core copies ~11 GB/s into pinned
 * memory, a PCIe link takes ~50: the default is what the host's cores allow when every lane runs its own, between 2 and 4 -- three keep a link busy; 1..6; tuning knob).
 *
 * jpezy_encode_batch_multi: the one-shot form (create, one call, destroy; chunk_frames is clamped to the largest shard so that a
 * single large frame does not reserve a ring for sixteen) -- what jpezy_encode --gpus N calls.
 * Replaces, for a batch: the caller's loop over encoder objects; inside each frame encoder/jpezy_encoder.hpp:55-67 and :174-225.
 * The handle's contexts are its own: it always point-samples the chroma (jpezy_ctx_set_chroma_downsampling does not reach them).
 */
typedef struct jpezy_multi_out {
    int16_t* coeffs;
    uint8_t* jpg;
    size_t jpg_stride;
    long long* jpg_sizes;
    int on_root_device;
} jpezy_multi_out;
typedef struct jpezy_multi_lane_stats {
    int device;
    int staged;
    long frames;
    double wall_ms, kernel_ms;
    unsigned long long bytes_up, bytes_down;
} jpezy_multi_lane_stats;
typedef struct jpezy_multi jpezy_multi;
void jpezy_shard_range(long n_units, int n_shards, int k, long* first, long* count);
jpezy_multi* jpezy_multi_create(const int* devices, int n_dev, int W, int H, int gray, int chunk_frames);
void jpezy_multi_destroy(jpezy_multi* m);
int jpezy_multi_encode(jpezy_multi* m, const uint8_t* r, const uint8_t* g, const uint8_t* b, int n_frames, const char* comment,
                       const jpezy_multi_out* out);
int jpezy_multi_last_stats(const jpezy_multi* m, jpezy_multi_lane_stats* stats, int cap);
int jpezy_multi_chunk_frames(const jpezy_multi* m);
int jpezy_multi_feeder_threads(const jpezy_multi* m);
int jpezy_multi_set_feeder_threads(jpezy_multi* m, int n);
int jpezy_encode_batch_multi(const int* devices, int n_dev, const uint8_t* r, const uint8_t* g, const uint8_t* b, int W, int H, int gray,
                             int n_frames, int chunk_frames, const char* comment, const jpezy_multi_out* out);

typedef struct jpezy_frame_info {
    int width, height, ncomp, precision;
    int H[3], V[3], Tq[3];
    int hmax, vmax, mcu_cols, mcu_rows, blocks_per_mcu;
    int restart_interval;
    int major_rev, minor_rev, units, hdensity, vdensity;
    int format;               /* 0 undefined, 1 JFIF, 2 JFXX (jpezy.hpp:155-160) */
    char comment[256];
    uint16_t qt[4][64];       /* natural order */
} jpezy_frame_info;

/*
 * jpezy_read_jpeg replaces decoder::analyze_header and the marker parsers (decoder/jpezy_decoder.hpp:
 * 171-502) and decoder::decode_huffman (:583-642).  coeffs (may be NULL: headers only) receives
 * [mcu][block][64] int16 in zig-zag order with DC prediction undone.
 */
int jpezy_read_jpeg(const uint8_t* data, size_t len, jpezy_frame_info* info, int16_t* coeffs,
                    size_t coeff_cap);
/*
 * The same head with the Huffman decoding on the GPU (decode side): the header is parsed on the
 * host, the entropy-coded segment is decoded by the self-synchronising parallel decoder of jpezy_huffdec.hip, the
 * coefficients ([mcu][block][64] zig-zag int16, coeff_cap elements) are left in DEVICE memory, ready for
 * jpezy_dequant_idct_dev / _generic.  A scan with restart intervals (DRI / RSTn, decoder/jpezy_decoder.hpp:152-163) is decoded as
 * that many independent streams when it is regular -- one RSTn behind every interval but the last, nothing else.  Anything irregular
 * (a missing or extra marker, an invalid code, an early end) is decoded by jpezy_read_jpeg's host decoder instead and uploaded, so
 * results and error codes are always those of jpezy_read_jpeg.  d_coeffs may be NULL (header only).  Synchronous.
 */
int jpezy_read_jpeg_gpu(jpezy_ctx* ctx, const uint8_t* data, size_t len, jpezy_frame_info* info, int16_t* d_coeffs,
                        size_t coeff_cap);
/*
 * decoder::decode end to end (decoder/jpezy_decoder.hpp:76-134): .jpg bytes in, planar r,g,b (plane_cap >= width*height
 * bytes each) out; info receives the header fields.  jpezy's own layout (3 components sampled 2x2/1x1/1x1, 8 bit) runs
 * Huffman decoding, dequantisation, IDCT and colour conversion on the device in one fused kernel; every other baseline
 * layout the reference accepts takes the same device Huffman decoder and the generic kernels.  r,g,b NULL: header only.
 */
int jpezy_decode_jpeg(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, jpezy_frame_info* info, uint8_t* r,
                      uint8_t* g, uint8_t* b, size_t plane_cap);
/*
 * jpezy_decode_jpeg for n files at once (n decoder objects of the reference, decoder/jpezy_decoder.hpp:39-134, one per
 * file).  Files without restart intervals are grouped by size, layout (any the reference's decode_mcu handles: 1 or 3 components,
 * sampling factors 1..4) and quantiser tables and decoded TOGETHER: one sequence of Huffman-decoder launches per slice of 16 scans
 * (every file with its own code tables), one inverse-transform launch per slice (the fused kernel for jpezy's own 2x2/1x1/1x1 layout,
 * the generic kernels for the others), the planes of a slice copied out while the next slice is decoded -- a single file keeps 80
 * waves busy for a chain of launches that is pure latency, a slice fills the chip for the same chain; a batch is bounded by PCIe.
 * Everything else (irregular or non-converging streams, single files)
 * is decoded file by file, up to 8 in flight on child contexts, with the host decoder as the last word, as before.  data[i] / len[i]: file i;
 * r[i], g[i], b[i]: its planes (plane_cap[i] >= width*height bytes each; sizes come from a header-only jpezy_decode_jpeg or
 * jpezy_read_jpeg call); info[i] and status[i] (JPEZY_OK or that file's negative error code) are written per file.
 * Returns JPEZY_OK when every file decoded, else the first failing file's code (message: which file and why); the other
 * files' outputs are complete either way.
 */
int jpezy_decode_jpeg_batch(jpezy_ctx* ctx, int n, const uint8_t* const* data, const size_t* len, int gray,
                            jpezy_frame_info* info, uint8_t* const* r, uint8_t* const* g, uint8_t* const* b,
                            const size_t* plane_cap, int* status);
/* Synchronisation passes the last jpezy_read_jpeg_gpu call needed; 0 = the host decoder was used (test/diagnostic hook). */
int jpezy_ctx_last_huffdec_passes(jpezy_ctx* ctx);
/* Files of the last jpezy_decode_jpeg_batch call that were decoded by the batch form of the kernels (test/diagnostic hook). */
int jpezy_ctx_last_batch_fast_count(jpezy_ctx* ctx);
/* Scans shorter than n bytes are decoded on the host (default 32 KiB: the GPU decoder has ~0.32 ms of fixed cost, which the host decoder spends on ~30 KiB of scan); 0
 * sends every scan to the GPU decoder (tests). */
void jpezy_ctx_set_huffdec_min_bytes(jpezy_ctx* ctx, size_t n);

/*
 * PACKED (INTERLEAVED) PIXELS.  The reference keeps three planes (jpezy_encoder.hpp:24-28; its CLI builds an interleaved image and
 * splits it, encode_io.hpp:151); a caller with a decoded camera frame, an H x W x C array or a framebuffer has interleaved pixels.
 * These entry points take and return them as they are: only the first step (pixel load) and the last step (pixel store) of the kernels
 * differ, the arithmetic, the guard bands, the exact paths and the Huffman stages are the planar ones', and every coefficient and every
 * pixel byte equals what the planar sibling gives for the same pixels.
 *
 *   Addressing    pixel (x, y) of frame f starts at pix + f*frame_stride + y*row_stride + x*bytes, bytes = jpezy_pixel_bytes(format)
 *   row_stride    >= W*bytes; 0 = tight (W*bytes)
 *   frame_stride  >= (H-1)*row_stride + W*bytes; 0 = H*row_stride
 *   Size limit    row_stride * H must fit in 32 bits (JPEZY_E_BADARG otherwise): the kernels keep 32-bit row offsets as the planar ones do
 *   Alignment     none required.  W % 16 == 0 with base, row_stride and frame_stride multiples of 16 takes the 16-byte load / store form
 *                 (channels separated / merged in registers); everything else moves single bytes
 *   Bytes touched only bytes [0, W*bytes) of each row are read or written: never row padding, never anything behind the last row's W*bytes
 *                 (jpezy_encode_jpeg_packed alone may READ the padding between the rows of a band when it uploads it)
 *   32-bit formats  encode ignores the fourth byte, decode writes 0xFF into it
 *   gray          the planar meaning: encode computes luma from the three channels and emits the 4-block layout, decode writes r = g = b = clamp(Y)
 *   Context settings  jpezy_ctx_set_force_exact, _set_variant, _set_decode_tolerance and _set_host_chunk_bytes act as on the planar entries.
 *                 Encode variant 0 (FP64) reads packed pixels through its byte loop; the laboratory's variants 2 and 3 hand packed input to
 *                 variant 1's launch, as they do every frame they do not cover
 *   Batches       more than 65535 frames go out as several launches, as in jpezy_fdct_quant_dev
 *
 * NOT provided in packed form: the host-buffer jpezy_fdct_quant / jpezy_dequant_idct, jpezy_decode_jpeg_batch, the multi-GPU handle, the
 * jpezy::encoder / decoder class surface and the CLIs (they mirror the reference's planar constructors and P3 files), formats with alpha
 * first, 16-bit channels.
 */
enum jpezy_pixel_format { JPEZY_PIX_RGB24 = 0, JPEZY_PIX_BGR24 = 1, JPEZY_PIX_RGBA32 = 2, JPEZY_PIX_BGRA32 = 3 };
int jpezy_pixel_bytes(int format);          /* 3, 3, 4, 4; JPEZY_E_BADARG otherwise (pure host function) */
/* jpezy_fdct_quant_dev for packed pixels in device memory; replaces the same reference lines (encoder/jpezy_encoder.hpp:90-172, 195, 212,
 * 244-256).  Asynchronous on `stream`. */
int jpezy_fdct_quant_packed_dev(jpezy_ctx* ctx, const uint8_t* d_pix, int format, size_t row_stride, size_t frame_stride, int W, int H,
                                int gray, int n_frames, int16_t* d_coeffs, void* stream);
/* jpezy_dequant_idct_dev writing packed pixels (decoder/jpezy_decoder.hpp:519-524, 531-578, 645-676); jpezy's own 2x2,1x1,1x1 layout.
 * Asynchronous on `stream`; the table rules of jpezy_dequant_idct_dev apply. */
int jpezy_dequant_idct_packed_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], const uint8_t comp_tq[3], int format,
                                  size_t row_stride, size_t frame_stride, int W, int H, int gray, int n_frames, uint8_t* d_pix, void* stream);
/* jpezy_encode_jpeg from host packed pixels (encoder/jpezy_encoder.hpp:38-77): streamed in MCU-row bands like it, one input segment per
 * band instead of three; the bytes are those of jpezy_encode_jpeg for the same pixels. */
long jpezy_encode_jpeg_packed(jpezy_ctx* ctx, const uint8_t* pix, int format, size_t row_stride, int W, int H, int gray, const char* comment,
                              uint8_t* out, size_t cap);
/* jpezy_decode_jpeg into host packed pixels (decoder/jpezy_decoder.hpp:76-134), for every layout it accepts: jpezy's own through the fused
 * kernel, everything else through the generic pair, files handed to the host Huffman decoder included.  pix NULL: header only;
 * pix_cap < (H-1)*row_stride + W*bytes: JPEZY_E_NOSPACE. */
int jpezy_decode_jpeg_packed(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, jpezy_frame_info* info, int format, size_t row_stride,
                             uint8_t* pix, size_t pix_cap);

/*
 * REDUCED-SIZE DECODE (1/2, 1/4, 1/8).  scale_denom is 1, 2, 4 or 8 and N = 8 / scale_denom is the edge of a block in output samples;
 * the output is Ws x Hs = ceil(W*N/8) x ceil(H*N/8).  The reference has no such mode: the definition is this project's own
 * and says that the result is what the reference's decode loop would give if its block were N x N instead of 8 x 8:
 *
 *   dequantise    as always (decoder/jpezy_decoder.hpp:645-650): dct[nat] = (int)coef * qt[Tq][nat], 32-bit int
 *   transform     inverse_dct (:652-670) over the N x N low-frequency corner, for y, x < N: sum = 0.0; v = 0..N-1 outer, u = 0..N-1 inner:
 *                 sum += cu * cv * dct[v*8+u] * COS[(u*8/N)*8 + x] * COS[(v*8/N)*8 + y], left to right in binary64 without contraction, COS the
 *                 8-point table (cos((2x+1)u*pi/2N) is its entry (u*8/N, x)); sample = int(sum / 4 + level) with the reference's conversion
 *                 (INT_MIN outside int32), level = 128 or 2048.  The 1/4 holds for every N: an N-point inverse fed 8-point-scaled
 *                 coefficients has that normalisation; for N = 1 the sample is int(DC*Q/8 + level), the block mean
 *   placement     decode_mcu (:504-528) with N for 8: the MCU is hmax*N x vmax*N, block (kx, ky) is written at (kx*N, ky*N) as a rectangle of
 *                 N*dupx x N*dupy, the last writer stays, unwritten positions keep 0 / 0x80, rows >= Hs and columns >= Ws are dropped.  A
 *                 subsampled component is replicated as the reference replicates it, not given a larger transform
 *   colour        make_rgb / revise_value and gray (:531-578, 672-676) unchanged
 *
 * Every layout jpezy_decode_jpeg accepts is accepted, jpezy's own included: all of them take the two kernels of jpezy_kernels_scaled.hip
 * (every sample evaluated directly in the order above: no fast path, no guard band).  jpezy_ctx_set_force_exact and
 * jpezy_ctx_set_decode_tolerance therefore have nothing to act on here, and the fallback counter is not advanced.
 * scale_denom = 1 is handed to the full-size entry point named with each function, under that entry's own rules: byte for byte the existing decode.
 * JPEZY_E_BADARG for any other denominator.
 */
/* Ws, Hs (either may be NULL) for a W x H file; JPEZY_E_BADARG for a denominator outside {1, 2, 4, 8} or a non-positive size.  Pure host
 * function. */
int jpezy_scaled_size(int W, int H, int scale_denom, int* Ws, int* Hs);
/* jpezy_dequant_idct_generic_batch_dev at reduced size (stands in for decoder/jpezy_decoder.hpp:504-578, 645-676 with an N x N block; the
 * reference has no such mode, the definition above is this project's own): d_r, d_g, d_b planes of Ws*Hs bytes, frame f's at
 * + f * plane_stride (>= Ws*Hs, no alignment asked).  The generic entry's table, scratch (one call in flight per context) and capture rules
 * apply; more than 65535 frames go out as several pairs of launches.  scale_denom 1: jpezy_dequant_idct_generic_dev for one frame,
 * jpezy_dequant_idct_generic_batch_dev (plane_stride a multiple of 4) for more. */
int jpezy_dequant_idct_scaled_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                  const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray, int scale_denom,
                                  int n_frames, size_t plane_stride, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream);
/* The same writing packed pixels (same reference lines, same remark: no such mode in the reference, the definition is this project's own).
 * The addressing rules of the packed section apply with Ws, Hs for W, H: pixel (x, y) of frame f at d_pix + f*frame_stride + y*row_stride +
 * x*bytes, row_stride 0 = Ws*bytes, frame_stride 0 = Hs*row_stride, only bytes [0, Ws*bytes) of a row are written, byte 3 of a 32-bit pixel
 * is 0xFF.  scale_denom 1: the generic kernels' packed store stage (n_frames > 1 then asks for a frame_stride that is a multiple of 4). */
int jpezy_dequant_idct_scaled_packed_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp,
                                         const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W,
                                         int H, int gray, int scale_denom, int format, size_t row_stride, size_t frame_stride, int n_frames,
                                         uint8_t* d_pix, void* stream);
/* jpezy_decode_jpeg at reduced size (decoder/jpezy_decoder.hpp:76-134 with the transform stage above; the reference has no such mode, the
 * definition is this project's own): header parse and Huffman decoding exactly as jpezy_decode_jpeg does them (GPU decoder, host decoder
 * for what it declines), then the scaled stage and a download of Ws*Hs bytes per plane.  info keeps the FILE's width and height.  r, g, b
 * NULL: header only; plane_cap < Ws*Hs: JPEZY_E_NOSPACE.  scale_denom 1: jpezy_decode_jpeg. */
int jpezy_decode_jpeg_scaled(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, int scale_denom, jpezy_frame_info* info, uint8_t* r,
                             uint8_t* g, uint8_t* b, size_t plane_cap);
/* The same into host packed pixels (jpezy_decode_jpeg_packed at reduced size; same reference lines and remark): pix NULL: header only;
 * pix_cap < (Hs-1)*row_stride + Ws*bytes: JPEZY_E_NOSPACE.  scale_denom 1: jpezy_decode_jpeg_packed. */
int jpezy_decode_jpeg_scaled_packed(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, int scale_denom, jpezy_frame_info* info,
                                    int format, size_t row_stride, uint8_t* pix, size_t pix_cap);

/*
 * REGION DECODE (a crop window of the picture, full size or reduced).  The reference decodes whole pictures only; a loader that feeds
 * crops, a viewer that tiles a large scan or a detector that re-reads a box wants a part.  The definition is this project's own
 *  and adds no arithmetic:
 *
 *   Coordinates   a region {x, y, w, h} lives in the picture at the requested scale, Ws x Hs = jpezy_scaled_size(W, H, scale_denom),
 *                 scale_denom one of 1, 2, 4, 8
 *   Result        output byte (i, j) of every plane, 0 <= i < w, 0 <= j < h, is byte (x + i, y + j) of what jpezy_decode_jpeg_scaled gives
 *                 for the same file, gray and scale_denom -- at scale_denom 1 that is jpezy_decode_jpeg in its exact mode.  Packed pixels:
 *                 the same against jpezy_decode_jpeg_scaled_packed.  Chroma is replicated, not interpolated, and make_rgb is per pixel, so
 *                 a pixel depends only on the MCU that covers it and the slice of the decode is the decode of the MCUs the window touches
 *   Inside        w, h >= 1, x, y >= 0, x + w <= Ws, y + h <= Hs; anything else is JPEZY_E_BADARG with a message that names the region and
 *                 Ws x Hs.  There is no silent clipping
 *   Arithmetic    every sample is evaluated in the definition's order (the scaled section's sum with N = 8 / scale_denom, N = 8 included:
 *                 dequantise in 32-bit int, v outer, u inner, left to right in binary64, int(sum / 4 + level)): no fast path, no guard band.
 *                 jpezy_ctx_set_force_exact and jpezy_ctx_set_decode_tolerance have nothing to act on and the fallback counter is not
 *                 advanced
 *   Whole picture a region that is the whole picture is handed to the reduced-size entry point of the same shape (and by it, at
 *                 scale_denom 1, to the full-size one) under that entry's own rules: it costs what it costs today.  One exception: a
 *                 device batch at scale_denom 1 whose plane or frame stride is no multiple of 4, which the full-size batch entry refuses,
 *                 stays with the region kernel
 *   What is saved the inverse transform, the colour stage and the stores run over the MCUs that intersect the window only, only their
 *                 coefficient blocks are read, and only w * h bytes per plane (h rows of w * bytes) travel back to the host
 *   What is not   the WHOLE scan is still Huffman-decoded and the coefficient buffer stays full size: jpezy_decode_jpeg_region pays the
 *                 upload and the entropy decoding of the whole file
 *   Bytes touched no byte outside the w x h output is written: never row padding, never anything between the frames of a batch
 *
 * NOT provided: several regions of ONE file per call, regions in jpezy_decode_jpeg_batch (one window of each of many files in one
 * call is the next section, BATCH OF WINDOWS), YCC-plane output of a region, skipping the Huffman decoding of restart intervals outside
 * the window.
 */
typedef struct jpezy_rect { int x, y, w, h; } jpezy_rect;
/* JPEZY_OK when region lies inside a W x H file decoded at 1 / scale_denom, else JPEZY_E_BADARG and the message.  Pure host function. */
int jpezy_region_check(int W, int H, int scale_denom, const jpezy_rect* region);
/* jpezy_dequant_idct_scaled_dev for a window (stands in for decoder/jpezy_decoder.hpp:504-578, 645-676 over the MCUs the window touches; the
 * reference has no such mode, the definition above is this project's own): d_coeffs the WHOLE frames' coefficients as jpezy_read_jpeg_gpu
 * leaves them, d_r, d_g, d_b planes of w*h bytes, frame f's at + f * plane_stride (>= w*h, no alignment asked).  Null pointers, scale,
 * region and strides are refused before the context is looked at.  One launch per 65535 frames, no scratch; the generic entry's table and
 * capture rules apply.  Asynchronous on `stream`. */
int jpezy_dequant_idct_region_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                  const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray, int scale_denom,
                                  const jpezy_rect* region, int n_frames, size_t plane_stride, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b,
                                  void* stream);
/* The same writing packed pixels (same reference lines, same remark).  The addressing rules of the packed section apply with w, h for W, H:
 * pixel (i, j) of the window of frame f at d_pix + f*frame_stride + j*row_stride + i*bytes, row_stride 0 = w*bytes, frame_stride 0 =
 * h*row_stride, only bytes [0, w*bytes) of a row are written, byte 3 of a 32-bit pixel is 0xFF. */
int jpezy_dequant_idct_region_packed_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp,
                                         const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W,
                                         int H, int gray, int scale_denom, const jpezy_rect* region, int format, size_t row_stride,
                                         size_t frame_stride, int n_frames, uint8_t* d_pix, void* stream);
/* jpezy_decode_jpeg_scaled for a window (decoder/jpezy_decoder.hpp:76-134 with the region stage; the reference has no such mode, the
 * definition is this project's own): header parse and Huffman decoding of the whole file exactly as jpezy_decode_jpeg does them (GPU
 * decoder, host decoder for what it declines), then the region stage and a download of w*h bytes per plane.  info keeps the FILE's width
 * and height.  r, g, b NULL: header only, and the region is then checked for w, h >= 1 and x, y >= 0 alone; plane_cap < w*h:
 * JPEZY_E_NOSPACE. */
int jpezy_decode_jpeg_region(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, int scale_denom, const jpezy_rect* region,
                             jpezy_frame_info* info, uint8_t* r, uint8_t* g, uint8_t* b, size_t plane_cap);
/* The same into host packed pixels (jpezy_decode_jpeg_scaled_packed for a window; same reference lines and remark): pix NULL: header only;
 * pix_cap < (h-1)*row_stride + w*bytes: JPEZY_E_NOSPACE. */
int jpezy_decode_jpeg_region_packed(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, int scale_denom, const jpezy_rect* region,
                                    jpezy_frame_info* info, int format, size_t row_stride, uint8_t* pix, size_t pix_cap);

/*
 * BATCH OF WINDOWS (one crop window of each of n files, sizes mixed, packed pixels left in device memory).  What an input pipeline for
 * training or inference asks of a GPU decoder: a few hundred .jpg files of DIFFERENT sizes, one crop of each, possibly at 1/2 or 1/4, side
 * by side in device memory as one [n, h, w, bytes] tensor.  The definition is this project's own and adds no arithmetic.
 * For file k of n:
 *
 *   Window        {region, scale_denom}: scale_denom one of 1, 2, 4, 8, region in the picture at that scale (REGION DECODE's coordinates).
 *                 region.w == 0 && region.h == 0: the whole picture at that scale (x, y are then not looked at).  windows == NULL: whole
 *                 pictures at full size
 *   Result        every byte of the window equals what jpezy_decode_jpeg_region_packed returns for the same file, gray, scale_denom, region
 *                 and format, in that entry's exact arithmetic (the region section's: dequantise in 32-bit int, v outer, u inner, left to
 *                 right in binary64, int(sum / 4 + level), replication, make_rgb per pixel)
 *   Whole picture the result equals what jpezy_decode_jpeg_scaled_packed returns -- jpezy_decode_jpeg_packed in its exact mode at
 *                 scale_denom 1.  It is computed by the windowed kernel over the full window, at that kernel's rate
 *   No inexact path  the result never depends on jpezy_ctx_set_decode_tolerance or jpezy_ctx_set_force_exact, and the fallback counter is
 *                 not advanced
 *   Output        packed pixels (JPEZY_PIX_*) in DEVICE memory: pixel (i, j) of file k's window at
 *                 d_pix + k*slot_stride + j*row_stride + i*bytes.  Both strides are given (windows differ in size: there is no 0 = tight);
 *                 row_stride fits in 32 bits
 *   Fit           a window fits when w*bytes <= row_stride and (h-1)*row_stride + w*bytes <= slot_stride; n*slot_stride <= pix_cap is
 *                 checked once for the call (JPEZY_E_NOSPACE)
 *   Bytes touched no byte outside a file's w*bytes x h rectangle is written: not row padding, not the rest of a slot, not the slot of a
 *                 file that failed.  Byte 3 of a 32-bit pixel is 0xFF
 *   Per file      as in jpezy_decode_jpeg_batch: info[k] (the file's header), placed[k] (the window as decoded, w and h filled in for a
 *                 whole picture; the array may be NULL) and status[k].  The header is read first; a window outside the picture is
 *                 JPEZY_E_BADARG for that file, a window that does not fit its slot JPEZY_E_NOSPACE, a broken file gets the code
 *                 jpezy_decode_jpeg_region_packed gives it; the other files are complete either way.  The call returns JPEZY_OK or the
 *                 first failing file's code with a message that names the file
 *   Paths         files of one layout (components, sampling factors, precision) go through the GPU Huffman decoder together, whatever
 *                 their sizes and tables, and through one transform launch per scale; restart intervals, streams that do not settle and
 *                 irregular streams go file by file on child contexts.  Same bytes either way.  jpezy_ctx_last_batch_fast_count: the files
 *                 the grouped path delivered
 *   Synchronous   on return the pixels are complete in device memory.  Refused inside a stream capture
 *
 * NOT provided: host-memory, planar or YCC output; smooth upsampling of windows; skipping the Huffman decoding of MCUs outside a window (the
 * whole scan of every file is decoded).  Windows of different sizes brought to ONE output size are the section after this one, BATCH OF
 * WINDOWS, RESIZED.
 */
typedef struct jpezy_window { jpezy_rect region; int scale_denom; } jpezy_window;
/* Pure host function: the window of a W x H file as it will be decoded (whole-picture form resolved; win NULL: the whole picture at full
 * size) into *placed (may be NULL), and whether it fits the slot.  JPEZY_E_BADARG: format, W, H, scale_denom, a window outside the picture
 * (placed is then not written); JPEZY_E_NOSPACE: it does not fit row_stride / slot_stride (placed is written). */
int jpezy_window_fit(int W, int H, const jpezy_window* win, int format, size_t row_stride, size_t slot_stride, jpezy_rect* placed);
/* The batch (stands in for n calls of decoder/jpezy_decoder.hpp:76-134 with the region stage; the reference has no such mode, the definition
 * above is this project's own).  data[k], len[k]: the files in host memory; windows: n of them or NULL; d_pix: device memory of pix_cap
 * bytes.  Refused before the context is looked at, in this order: n < 0, (n == 0 is JPEZY_OK,) null arrays, format, zero strides,
 * row_stride beyond 32 bits, n*slot_stride > pix_cap (JPEZY_E_NOSPACE). */
int jpezy_decode_windows_dev(jpezy_ctx* ctx, int n, const uint8_t* const* data, const size_t* len, int gray, const jpezy_window* windows,
                             int format, size_t row_stride, size_t slot_stride, uint8_t* d_pix, size_t pix_cap, jpezy_frame_info* info,
                             jpezy_rect* placed, int* status);
/* Files per slice of the grouped path: 0 = automatic (at most 512, coefficients + scans + decoder scratch under ~1.5 GB), 1..512 = that many.
 * A test and measurement knob, per context; the bytes do not depend on it. */
int jpezy_ctx_set_windows_slice_files(jpezy_ctx* ctx, int n);

/*
 * BATCH OF WINDOWS, RESIZED (one crop window of each of n files, every window of its own size, all brought to ONE out_w x out_h and left in
 * device memory as one [n, out_h, out_w, bytes] tensor; optionally mirrored).  What random-resized-crop, a centre crop of the short side or a
 * thumbnail ask for: the window decode of BATCH OF WINDOWS, unchanged, and a resampling stage behind it.  The definition is this project's
 * own (restated in tests/resize_model.py) and is integer fixed point, so that it is exact without a guard band:
 *
 *   Filter        separable; the triangle filter, widened by the reduction ratio where an axis shrinks (antialiased), plain two-tap
 *                 bilinear where it grows
 *   Weights       one axis, in_size source samples to out_size output samples, in binary64 on the host, every operation separate and in
 *                 this order (no fused multiply-add):
 *                     scale = in_size / out_size      fs = max(scale, 1.0)      support = fs      ss = 1.0 / fs
 *                 output index i:
 *                     center = (i + 0.5) * scale
 *                     first  = max(0, (int)(center - support + 0.5))      last = min(in_size, (int)(center + support + 0.5))
 *                     count  = last - first
 *                 j in [0, count):
 *                     a   = |(j + first - center + 0.5) * ss|             w_j = a < 1 ? 1 - a : 0
 *                     k_j = w_j / sum(w) when sum(w) != 0, else w_j       K_j = (int)(0.5 + k_j * 2^22)
 *                 jpezy_resize_taps returns exactly these tables
 *   Passes        horizontal first: t = clip((2^21 + sum_j K_j * src[first + j]) >> 22, 0, 255) per channel, a byte; the vertical pass is
 *                 the same formula over t.  32-bit int accumulators; they cannot overflow for sizes up to 65535: the weights of one output
 *                 sum to at most 2^22 + count / 2, count <= 131071, and 255 * (2^22 + 65536) + 2^21 < 2^31
 *   Byte 3        of a 32-bit pixel is 0xFF and is not resampled
 *   Identity      in_size == out_size gives the weights (2^22, 0): a pass returns its input, with no special case
 *   Mirror        per file: output column i of a mirrored file is column out_w - 1 - i of the unmirrored result
 *   Result        file k's out_w x out_h pixels equal the above applied to the bytes jpezy_decode_jpeg_region_packed returns for the file's
 *                 window, gray, scale_denom and format.  Nothing about the window decode changes; chroma of the window is replicated as
 *                 there.  For 3-byte pixels the result equals Pillow 12's Image.resize(size, BILINEAR) of the window byte for byte (its RGBA
 *                 mode premultiplies alpha and is not the definition)
 *   Window        as in BATCH OF WINDOWS; windows == NULL: whole pictures at full size.  jpezy_resize_pick_window turns a source rectangle
 *                 in full-size coordinates into the window and the largest scale_denom that still leaves at least out_w x out_h pixels
 *   Output        packed pixels in DEVICE memory: pixel (i, j) of file k at d_pix + k*slot_stride + j*row_stride + i*bytes.  All outputs
 *                 have one size, so both strides may be 0 = tight (row_stride = out_w*bytes, slot_stride = out_h*row_stride)
 *   Fit           checked once for the call: out_w*bytes <= row_stride (JPEZY_E_BADARG), (out_h-1)*row_stride + out_w*bytes <= slot_stride
 *                 and n*slot_stride <= pix_cap (JPEZY_E_NOSPACE); nothing is written then
 *   Bytes touched no byte outside a file's out_w*bytes x out_h rectangle is written: not row padding, not the rest of a slot, not the slot
 *                 of a file that failed
 *   Per file      info[k], placed[k] (the SOURCE window as decoded) and status[k] as in BATCH OF WINDOWS; a window outside the picture is
 *                 JPEZY_E_BADARG for that file, the other files are complete
 *   Paths         those of BATCH OF WINDOWS (grouped by layout; child contexts for restart intervals, streams that do not settle and
 *                 irregular streams), each with the resampling launch behind it: per slice of a group, per file on a child context.  Same
 *                 bytes either way.  jpezy_ctx_last_batch_fast_count and jpezy_ctx_set_windows_slice_files act as there.  The decoded
 *                 windows of a slice lie in a scratch of the context (rows of the slice's widest window, the sum of the windows' heights)
 *                 that counts against the slice bound
 *   Synchronous   on return the pixels are complete in device memory.  Refused inside a stream capture
 *
 *   FILTERS       The above is JPEZY_FILTER_BILINEAR, the default.  jpezy_ctx_set_windows_filter chooses another filter for this entry and
 *                 for jpezy_decode_windows_tensor_dev (restated in tests/resize_filter_model.py).  Everything above holds
 *                 -- separable passes, horizontal first, each rounded and clipped to a byte, 22 fraction bits, 32-bit accumulators,
 *                 byte 3, the mirror, the shapes of first / count / ksize -- and three things become functions of the filter:
 *                     filter                   value   fsup   f(x)
 *                     JPEZY_FILTER_BILINEAR    0       1      1 - |x| for |x| < 1, else 0
 *                     JPEZY_FILTER_BOX         1       0.5    1 for -0.5 < x <= 0.5, else 0
 *                     JPEZY_FILTER_BICUBIC     2       2      with a = -0.5 and x = |x|: ((a + 2) * x - (a + 3)) * x * x + 1 for x < 1;
 *                                                             (((x - 5) * x + 8) * x - 4) * a for x < 2; else 0
 *                     JPEZY_FILTER_LANCZOS     3       3      sinc(x) * sinc(x / 3) for -3 <= x < 3, else 0; sinc(0) = 1,
 *                                                             sinc(x) = sin(pi * x) / (pi * x), pi * x one product with
 *                                                             pi = 3.14159265358979323846
 *                   Support    support = fsup * fs (fs and ss as above), ksize = 2 * (int)ceil(support) + 1; first, last and count from
 *                              center -+ support + 0.5 exactly as above
 *                   Weights    w_j = f((j + first - center + 0.5) * ss), k_j = w_j / sum(w) when sum(w) != 0, else w_j
 *                   Rounding   K_j = (int)(k_j * 2^22 + 0.5) for k_j >= 0 and (int)(k_j * 2^22 - 0.5) for k_j < 0
 *                 Every binary64 operation is separate and in the order written.  JPEZY_FILTER_LANCZOS, alone of the four, rests on the
 *                 platform's binary64 sin (the C library's); the others are plain arithmetic.  Bicubic and Lanczos have negative weights:
 *                 an accumulator can be negative, its shift >> 22 is arithmetic, and the clip to 0..255 follows it.  The accumulators
 *                 cannot overflow when, for every output index, 255 * (sum of the positive K) + 2^21 < 2^31 and 255 * (sum of the
 *                 negative K's magnitudes) <= 2^31 - 2^21.  The tables' builder checks this condition and answers JPEZY_E_UNSUPPORTED
 *                 where it fails (jpezy_resize_taps_filter, and the two entries for the file concerned); it is a condition, not a proof,
 *                 and has not been seen to fail: the largest sums met are 1.125 * 2^22 and 0.125 * 2^22 (bicubic), 1.279 * 2^22 and
 *                 0.279 * 2^22 (Lanczos).  With JPEZY_FILTER_BILINEAR every table, and so every byte, is the one defined above.  For
 *                 3-byte pixels box, bicubic and Lanczos equal Pillow 12's Image.resize(size, BOX / BICUBIC / LANCZOS) byte for byte.
 *                 A file of a child context (Paths) is resampled with the filter of the context the call was made on.
 *
 * NOT provided: other filters (nearest, bicubic); a per-file output size; a vertical mirror; host-memory output; smooth chroma upsampling
 * of the source window.  What stood first on this list, float or planar (CHW) output and normalisation, is the section after this
 * one: BATCH OF WINDOWS, TENSOR OUTPUT.  Of the list as it stands, smooth chroma upsampling exists (jpezy_ctx_set_windows_upsampling) and
 * so do bicubic, Lanczos and box (FILTERS above); the nearest and the Hamming filter are what is still not provided under "other filters".
 */
enum jpezy_filter { JPEZY_FILTER_BILINEAR = 0, JPEZY_FILTER_BOX = 1, JPEZY_FILTER_BICUBIC = 2, JPEZY_FILTER_LANCZOS = 3 };
/* Pure host function: the tables of one axis.  *ksize = 2 * (int)ceil(support) + 1 (>= every count); first[out_size], count[out_size],
 * weight[out_size][ksize], zero behind count.  first, count and weight all NULL: *ksize only.  Sizes outside 1..65535: JPEZY_E_BADARG;
 * weight_cap (in elements) < out_size * ksize: JPEZY_E_NOSPACE. */
int jpezy_resize_taps(int in_size, int out_size, int* ksize, int* first, int* count, int32_t* weight, size_t weight_cap);
/* The same for a filter of enum jpezy_filter (FILTERS above): jpezy_resize_taps's contract, and JPEZY_E_BADARG for an unknown filter
 * (checked first), JPEZY_E_UNSUPPORTED when the weights of some output index fail the accumulator condition.  jpezy_resize_taps is this
 * function at JPEZY_FILTER_BILINEAR. */
int jpezy_resize_taps_filter(int filter, int in_size, int out_size, int* ksize, int* first, int* count, int32_t* weight, size_t weight_cap);
/* The resampling filter of jpezy_decode_windows_resized_dev and jpezy_decode_windows_tensor_dev, per context: a value of enum jpezy_filter,
 * JPEZY_FILTER_BILINEAR by default.  An unknown value is JPEZY_E_BADARG and leaves the setting unchanged.  The getter returns the
 * setting. */
int jpezy_ctx_set_windows_filter(jpezy_ctx* ctx, int filter);
int jpezy_ctx_windows_filter(jpezy_ctx* ctx);
/* Test and measurement knobs, per context; the bytes do not depend on them.  Box, bicubic and Lanczos run a two-pass form of the
 * resampling kernel (the horizontal pass of a tile's source rows once, through LDS) for every file whose tiles span few enough source
 * rows, and the direct loop of the bilinear filter for the others.  on != 0: the direct loop for every file.
 * jpezy_ctx_last_resample_tiled_count: the files of the context's last resized or tensor call that ran the two-pass form. */
int jpezy_ctx_set_resample_direct(jpezy_ctx* ctx, int on);
int jpezy_ctx_last_resample_tiled_count(jpezy_ctx* ctx);
/* Pure host function: src, a rectangle in the FULL-SIZE picture (inside W x H, else JPEZY_E_BADARG), as a window for an output of
 * out_w x out_h: s = the largest of 8, 4, 2, 1 with src.w / s >= out_w and src.h / s >= out_h (integer division), else 1;
 * *win = {{src.x / s, src.y / s, max(1, src.w / s), max(1, src.h / s)}, s}.  That window always lies inside the picture at 1/s
 * (jpezy_scaled_size is ceil(W / s)).  Its edges are src's rounded down to the grid of s: the crop's edges move by less than s full-size
 * pixels.  A caller that wants an exact crop passes its own jpezy_window at scale_denom 1. */
int jpezy_resize_pick_window(int W, int H, const jpezy_rect* src, int out_w, int out_h, jpezy_window* win);
/* The batch (stands in for n calls of decoder/jpezy_decoder.hpp:76-134 with the region stage and a resampling the reference does not have;
 * the definition above is this project's own).  jpezy_decode_windows_dev's arguments and contracts, and: mirror_x n flags or NULL (none);
 * every file writes exactly out_w x out_h pixels.  Refused before the context is looked at, in this order: n < 0, (n == 0 is JPEZY_OK,)
 * null arrays, format, out_w / out_h outside 1..65535, row_stride beyond 32 bits or below out_w*bytes, slot_stride too small
 * (JPEZY_E_NOSPACE), n*slot_stride > pix_cap (JPEZY_E_NOSPACE). */
int jpezy_decode_windows_resized_dev(jpezy_ctx* ctx, int n, const uint8_t* const* data, const size_t* len, int gray,
                                     const jpezy_window* windows, const uint8_t* mirror_x, int out_w, int out_h, int format, size_t row_stride,
                                     size_t slot_stride, uint8_t* d_pix, size_t pix_cap, jpezy_frame_info* info, jpezy_rect* placed,
                                     int* status);

/*
 * BATCH OF WINDOWS, TENSOR OUTPUT (the resized batch written straight into the tensor a model takes: [n, C, out_h, out_w] in uint8, float32,
 * float16 or bfloat16, planar, channels-last or any other strides, with (x/255 - mean)/std applied).  The resampling kernel holds every output
 * pixel's three bytes in registers just before it stores them; the conversion happens there, so no second pass reads and writes the batch.
 * Nothing about the window decode or the resampling changes.  The definition is this project's own (restated in
 * tests/tensor_model.py):
 *
 *   Source bytes  for file k the out_w x out_h pixels that jpezy_decode_windows_resized_dev defines for the same files, windows, mirror flags,
 *                 gray and windows-upsampling setting in a 3-byte format: b[k][y][x][c], c in 0..2, is byte c of the pixel.  JPEZY_PIX_RGB24
 *                 puts R in channel 0, JPEZY_PIX_BGR24 puts B in channel 0.  The 32-bit formats are refused (JPEZY_E_BADARG): alpha is never
 *                 a tensor channel
 *   Shape         logical [n, C, out_h, out_w], C = channels, 3 or 1.  C == 1 needs gray != 0 (else JPEZY_E_BADARG) and is byte 0; with
 *                 gray and C == 3 the three source bytes are equal, as they are in the packed form
 *   Element type  JPEZY_DT_U8    the byte.  scale and bias must both be NULL (else JPEZY_E_BADARG): planar uint8
 *                 JPEZY_DT_F32   v = (float)b * scale[c] + bias[c] in binary32, the multiplication and the addition each rounded to nearest
 *                                even and NOT fused
 *                 JPEZY_DT_F16   v converted to binary16, round to nearest even, subnormals kept, overflow to +-inf
 *                 JPEZY_DT_BF16  the upper 16 bits of u + 0x7FFF + ((u >> 16) & 1), u being v's bit pattern
 *   scale, bias   C floats each, both given or both NULL (NULL: scale 1, bias 0).  Every value is 0 or finite with a magnitude in
 *                 [2^-100, 2^100] (else JPEZY_E_BADARG): then no binary32 step overflows or gives a subnormal, and NaN cannot occur
 *   Placement     four strides IN ELEMENTS (sn, sc, sh, sw), all >= 0: element (k, c, y, x) lies at
 *                 d_out + (k*sn + c*sc + y*sh + x*sw) * element size.  The strides must give every element a place of its own: of the
 *                 dimensions of extent > 1, sorted by stride, the smallest stride is >= 1 and every other one >= the stride before it times
 *                 that dimension's extent (else JPEZY_E_BADARG).  NCHW, NHWC, torch's channels_last, padded rows and padded slots are all
 *                 instances of this one rule; the stride of a dimension of extent 1 is not looked at beyond its sign
 *   Fit           sum over the dimensions of (extent - 1) * stride, + 1 <= cap_elems, else JPEZY_E_NOSPACE and nothing is written.  d_out
 *                 is aligned to the element size (else JPEZY_E_BADARG)
 *   Bytes touched only the elements named above: not row padding, not slot padding, not the slot of a file that failed, not the half of a
 *                 4-byte word that belongs to a neighbouring element
 *   Unchanged     info, placed, status, the per-file failure rule, the grouped / sliced / child-context paths, synchronisation and the
 *                 refusal inside a stream capture are those of jpezy_decode_windows_resized_dev
 *   Filter        the resampling filter is the context's (jpezy_ctx_set_windows_filter; BATCH OF WINDOWS, RESIZED, FILTERS): bilinear by
 *                 default, box, bicubic or Lanczos
 *
 * NOT provided: per-file output sizes; the nearest and the Hamming filter; a vertical mirror; host-memory output; float output from the
 * other decode entries.
 */
enum jpezy_dtype { JPEZY_DT_U8 = 0, JPEZY_DT_F32 = 1, JPEZY_DT_F16 = 2, JPEZY_DT_BF16 = 3 };
/* Pure host function: scale[c] = (float)(1.0 / (255.0 * std[c])), bias[c] = (float)(-mean[c] / std[c]) for c < C (3 or 1), computed in binary64
 * with every operation separate.  They are the two constants of (b/255 - mean)/std = b * (1 / (255 * std)) + (-mean / std), each evaluated in
 * binary64 and rounded once to binary32; an element is then the multiplication and the addition above and nothing else.  It may differ in
 * the last bits from a framework's three-step binary32 evaluation (divide by 255, subtract, divide).  JPEZY_E_BADARG: C, a null pointer, a std that is zero or not finite, a mean that is not finite (nothing
 * is written then). */
int jpezy_tensor_normalization(int C, const double* mean, const double* std, float* scale, float* bias);
/* The batch (stands in for n calls of decoder/jpezy_decoder.hpp:76-134 with the region stage, a resampling and a conversion the reference does
 * not have; the definition above is this project's own).  jpezy_decode_windows_resized_dev's arguments and contracts with the tensor's
 * description in place of the two byte strides; d_out: device memory of cap_elems ELEMENTS.  Refused before the context is looked at, in
 * this order: n < 0, (n == 0 is JPEZY_OK,) null arrays, an unknown format, a 32-bit format, out_w / out_h outside 1..65535, channels other
 * than 3 or 1, channels == 1 without gray, an unknown dtype, scale without bias or bias without scale, JPEZY_DT_U8 with a scale, a scale or
 * bias value outside the band, a negative stride, strides that overlap, cap_elems too small (JPEZY_E_NOSPACE), a misaligned d_out. */
int jpezy_decode_windows_tensor_dev(jpezy_ctx* ctx, int n, const uint8_t* const* data, const size_t* len, int gray,
                                    const jpezy_window* windows, const uint8_t* mirror_x, int out_w, int out_h, int format, int dtype,
                                    int channels, const float* scale, const float* bias, int64_t sn, int64_t sc, int64_t sh, int64_t sw,
                                    void* d_out, size_t cap_elems, jpezy_frame_info* info, jpezy_rect* placed, int* status);

/*
 * PLANAR YCbCr 4:2:0 SAMPLES (I420 / YV12 / NV12 / NV21) IN AND OUT.  The file format is full-range BT.601 YCbCr sampled 2x2, 1x1, 1x1: a
 * caller that already holds such planes (a video decoder, a camera, an ISP) holds the file's own sample domain.  The reference only takes
 * RGB (encoder/jpezy_encoder.hpp:24-28) and only gives RGB (decoder/jpezy_decoder.hpp:531-578), so the definition is this project's own
 * (restated in tests/ycc_model.py):
 *
 *   Sizes         CW = ceil(W/2), CH = ceil(H/2) (jpezy_ycc_chroma_size)
 *   Encode        the result of the reference's MCU loop (encoder/jpezy_encoder.hpp:58-67) if make_YCC (:90-144) handed over, instead of
 *                 converted pixels, for luma block i of MCU (ux, uy), sample (x, y):
 *                     (int)Y[min(uy*16 + 8*(i>>1) + y, H-1)][min(ux*16 + 8*(i&1) + x, W-1)] - 128
 *                 and for the Cb / Cr block, sample (x, y):
 *                     (int)C[min(uy*8 + y, CH-1)][min(ux*8 + x, CW-1)] - 128
 *                 DCT (:146-166), quantization (:168-172) and the zig-zag order are unchanged.  gray != 0: luma only, the 4-block layout;
 *                 the chroma pointers are not read and may be NULL.
 *   Anchor        with Y = Y_ref + 128 and Cb / Cr = the reference's chroma of the top-left pixel of every 2x2 + 128 (they fit a byte), the
 *                 coefficients equal jpezy_fdct_quant's for the RGB pixels whenever each of W and H is a multiple of 16 or odd, and for
 *                 gray at every size.  (Behind an even edge that is no multiple of 16 the RGB path replicates pixel W-1, whose chroma
 *                 sample no 4:2:0 plane holds: the plane's last sample belongs to pixel W-2.)
 *   Range         samples span [-128, 127] in all three components (the RGB path's chroma stops at -127): block sums span [-8192, 8128],
 *                 the range the exact DC table and its create-time check cover; flat planes of 0 give DCs -63 / -60, of 255 +63 / +59
 *   Decode        component c at its native sampling, ceil(W*H_c/hmax) x ceil(H*V_c/vmax) samples (jpezy_ycc_component_size): for this
 *                 project's own layout W x H, CW x CH, CW x CH.  inverse_quantization and inverse_dct (decoder/jpezy_decoder.hpp:645-670)
 *                 unchanged; block (kx, ky) of MCU (ux, uy) of component c is placed at ((ux*H_c + kx)*8, (uy*V_c + ky)*8); no replication
 *                 and no make_rgb; every byte is revise_value (:672-676) of the integer sample, so a sample of INT_MIN gives 0.  The Y plane
 *                 equals the r plane of jpezy_decode_jpeg(..., gray = 1).  jpezy_ctx_set_decode_tolerance(1): Y within one, chroma exact.
 *   Addressing    sample (x, y) of Y of frame f: y_ptr + f*y_frame_stride + y*y_stride + x; of Cb: cb_ptr + f*c_frame_stride + y*c_stride +
 *                 x*c_step, Cr the same from cr_ptr.  c_step 1: planes (I420; YV12 by exchanging the pointers); 2: one interleaved plane
 *                 (NV12: cr = cb + 1; NV21: cb = cr + 1).  Any other c_step: JPEZY_E_BADARG.  Strides of 0 mean tight (W; CW*c_step; H*y_stride;
 *                 CH*c_stride); a c_stride may be as small as (CW-1)*c_step + 1.  y_stride*H and c_stride*CH must fit in 32 bits.
 *   Alignment     none required.  W % 16 == 0 with 16-byte aligned Y base and strides and 8-byte aligned chroma planes (c_step 1) or a
 *                 16-byte aligned interleaved plane whose Cb and Cr are neighbours (c_step 2) takes the 16 / 8-byte form
 *   Bytes touched only sample bytes are read or written: never padding, never the other channel's bytes of an interleaved plane when only
 *                 one chroma pointer is given (decode), never anything behind the last row (jpezy_encode_jpeg_ycc alone may READ the
 *                 padding between the rows of a band when it uploads it)
 *   Context settings  jpezy_ctx_set_force_exact (levels 1-3), _set_variant, _set_decode_tolerance, _set_host_chunk_bytes, _set_huffman_optimize
 *                 and _set_restart_interval act as on the RGB entries.  Encode variant 0 (FP64) reads the planes through its byte loop; the
 *                 laboratory's variants 2 and 3 hand YCC input to variant 1's launch
 *
 * NOT provided in YCC form: jpezy_decode_jpeg_batch, the multi-GPU handle, reduced-size decode, region decode, the host-buffer jpezy_fdct_quant /
 * jpezy_dequant_idct, the jpezy::encoder / decoder class surface, 4:4:4 INPUT, limited-range (16-235) video levels: the caller's
 * planes are taken as the file's full-range samples.  (4:2:2 input and output -- I422 / NV16 planes, YUY2 / UYVY / YVYU macropixels -- has
 * entries of its own: jpezy_hip_ycc422.h, included at the end of this file.)
 */
/* CW, CH (either may be NULL) of a W x H picture; JPEZY_E_BADARG for a size outside 1..65535.  Pure host function (stands in for the
 * decimation of encoder/jpezy_encoder.hpp:134-142). */
int jpezy_ycc_chroma_size(int W, int H, int* CW, int* CH);
/* Width and height (either may be NULL) of component comp of a parsed file at its native sampling (decoder/jpezy_decoder.hpp:166-169,
 * 504-528 without the replication); JPEZY_E_BADARG for a component the file does not have.  Pure host function. */
int jpezy_ycc_component_size(const jpezy_frame_info* info, int comp, int* w, int* h);
/* jpezy_fdct_quant_dev from Y, Cb, Cr samples in device memory: stands in for encoder/jpezy_encoder.hpp:90-172 with make_YCC's conversion
 * (:244-256) taken out.  Asynchronous on `stream`; more than 65535 frames go out as several launches. */
int jpezy_fdct_quant_ycc_dev(jpezy_ctx* ctx, const uint8_t* d_y, size_t y_stride, const uint8_t* d_cb, const uint8_t* d_cr, size_t c_stride,
                             int c_step, size_t y_frame_stride, size_t c_frame_stride, int W, int H, int gray, int n_frames,
                             int16_t* d_coeffs, void* stream);
/* jpezy_dequant_idct_dev writing the components at their native sampling (decoder/jpezy_decoder.hpp:645-676 without decode_mcu's
 * replication :504-528 and make_rgb :531-578); jpezy's own 2x2,1x1,1x1 layout, the fused kernel.  d_cb == d_cr == NULL: luma only.
 * Asynchronous on `stream`; the table and capture rules of jpezy_dequant_idct_dev apply. */
int jpezy_dequant_idct_ycc_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], const uint8_t comp_tq[3], uint8_t* d_y,
                               size_t y_stride, uint8_t* d_cb, uint8_t* d_cr, size_t c_stride, int c_step, size_t y_frame_stride,
                               size_t c_frame_stride, int W, int H, int n_frames, void* stream);
/* jpezy_encode_jpeg from host Y, Cb, Cr planes (encoder/jpezy_encoder.hpp:38-77 without the conversion): streamed in MCU-row bands, up to
 * three input segments per band (16*k luma rows, ceil(rows/2) chroma rows; an interleaved plane travels as one segment); the Huffman
 * stage is jpezy_write_jpeg_gpu, so the optimise and restart settings act. */
long jpezy_encode_jpeg_ycc(jpezy_ctx* ctx, const uint8_t* y, size_t y_stride, const uint8_t* cb, const uint8_t* cr, size_t c_stride, int c_step,
                           int W, int H, int gray, const char* comment, uint8_t* out, size_t cap);
/* jpezy_decode_jpeg into host component planes (decoder/jpezy_decoder.hpp:76-134 without :504-578's replication and conversion), for every
 * layout it accepts: jpezy's own through the fused kernel, everything else through the generic pair, files handed to the host Huffman
 * decoder included.  y, cb, cr all NULL: header only.  A one-component file writes y only.  JPEZY_E_NOSPACE when y_cap <
 * (h0-1)*y_stride + w0 or c_cap < (hc-1)*c_stride + (wc-1)*c_step + 1 (w, h: jpezy_ycc_component_size). */
int jpezy_decode_jpeg_ycc(jpezy_ctx* ctx, const uint8_t* data, size_t len, jpezy_frame_info* info, uint8_t* y, size_t y_stride, size_t y_cap,
                          uint8_t* cb, uint8_t* cr, size_t c_stride, int c_step, size_t c_cap);

/*
 * CHROMA SAMPLING as an argument of the encoder's entry points (opt-in; every entry above keeps its signature, kernels and bytes).
 * The reference writes 2x2 / 1x1 / 1x1 only, so the definition of 4:4:4 is this project's own: the reference's per-sample arithmetic
 * with the decimation step left out.
 *
 *   sampling      JPEZY_SAMPLING_420 = 0: the entry of the same name without _sampling, gray passed on -- the same kernels, the same bytes.
 *                 JPEZY_SAMPLING_444 = 1: below.  JPEZY_SAMPLING_422 = 3: the block behind this one.  Any other value: JPEZY_E_BADARG
 *                 (2 is kept free for 4:4:0, the layout a transposed 4:2:2 file would have).
 *   MCU           8 x 8 pixels; mcu_cols = ceil(W / 8), mcu_rows = ceil(H / 8); three blocks in the order Y, Cb, Cr.  The picture is
 *                 extended to whole MCUs by clamping pixel coordinates (min(x, W-1), min(y, H-1)) as make_YCC does
 *                 (encoder/jpezy_encoder.hpp:101,104).
 *   Samples       Y, Cb and Cr of EVERY pixel from RGB::Y / Cb / Cr in the reference's FP64 order (:244-256), truncating.  Nothing of
 *                 make_YCC:116-143 (the pick of every second sample) applies.
 *   Transform     every block through DCT (:146-166) and quantization(cs) (:168-172) with the context's tables (Annex K, or
 *                 jpezy_ctx_set_quality / _set_quant_tables): Y by the luma table, Cb and Cr by the chroma table; zig-zag order.
 *   Coefficients  int16 [frame][mcu_y][mcu_x][3][64]: 192 * mcu_cols * mcu_rows elements per frame (jpezy_coeff_count_sampling), twice
 *                 the 4:2:0 count per pixel.
 *   File          the reference's writer (encoder/jpezy_writer.hpp:20-105, encoder/jpezy_encoder.hpp:174-242) except: SOF0 states H, V =
 *                 1,1 / 1,1 / 1,1; the scan's MCUs hold three blocks; DC prediction runs per component; Y is coded with the luma
 *                 Huffman tables, Cb and Cr with the chroma ones.  Optimised tables, restart intervals (counted in 8 x 8 MCUs) and DQT
 *                 tables compose as they do for 4:2:0.  jpezy_read_jpeg[_gpu] and jpezy_decode_jpeg* read such files (H = V = 1,1,1,
 *                 blocks_per_mcu = 3).
 *   Bound         jpezy_jpeg_bound_sampling: 1024 + 1344 per 8 x 8 MCU (three blocks of at most 1661 bits = 623 bytes, 1246 stuffed,
 *                 plus restart / pad / EOI); jpezy_jpeg_bound is per 16 x 16 MCU of six blocks and too small for 4:4:4.
 *   Refused       gray != 0 with JPEZY_SAMPLING_444 (JPEZY_E_BADARG: a gray 4:4:4 file has no use that the gray 4:2:0 file lacks);
 *                 encode variant 0, the FP64 kernel, with JPEZY_SAMPLING_444 (JPEZY_E_UNSUPPORTED; the context stays usable).
 *   Context settings  jpezy_ctx_set_force_exact (levels 0-3), _set_dc_table_lookup, _set_quality / _set_quant_tables act on the 4:4:4
 *                 transform as on the 4:2:0 one; jpezy_encode_jpeg_sampling[_packed] honour _set_huffman_optimize and
 *                 _set_restart_interval.
 *   Alignment     none required.  W % 8 == 0 with 8-byte aligned planes and plane stride (packed: 16-byte aligned base and strides)
 *                 takes the 8-byte (24 / 32-byte) load form.
 *
 * jpezy_encode_jpeg_sampling[_packed] run both stages on the GPU: the transform kernel, then jpezy_write_jpeg_gpu_sampling (the 4:2:0
 * entries' streaming upload in MCU-row bands is not built for 4:4:4: the picture goes up in one piece).
 * NOT provided for 4:4:4: the multi-GPU handle; planar YCbCr 4:4:4 INPUT; 4:4:0; gray; encode variant 0.
 *
 * JPEZY_SAMPLING_422 = 3 (2x1 / 1x1 / 1x1: full vertical chroma resolution, half the horizontal).  The definition is this project's own,
 * as for 4:4:4; everything said above holds except:
 *
 *   MCU           16 x 8 pixels; mcu_cols = ceil(W / 16), mcu_rows = ceil(H / 8); four blocks in the order Y-left, Y-right, Cb, Cr;
 *                 the same clamped extension to whole MCUs.
 *   Samples       Y of every pixel.  Point sampling (the default): chroma sample (x', y) is the Cb / Cr of pixel (min(2 x', W-1),
 *                 min(y, H-1)) -- the reference's decimation rule (make_YCC:134-142) in the horizontal direction only.
 *                 JPEZY_DOWNSAMPLE_AVERAGE (jpezy_ctx_set_chroma_downsampling) is honoured: (c[y][2x'] + c[y][2x'+1] + bias(x')) >> 1
 *                 over the per-pixel samples of the clamped extension, bias 0 for even x', 1 for odd x', arithmetic shift: libjpeg's
 *                 h2v1_downsample carried over to signed samples (adding 128 to both inputs adds 128 to the result).
 *   Coefficients  int16 [frame][mcu_y][mcu_x][4][64]: 256 * mcu_cols * mcu_rows elements per frame.
 *   File          SOF0 states H, V = 2,1 / 1,1 / 1,1; the scan's MCUs hold four blocks, the two luma blocks with the luma Huffman
 *                 tables and one running predictor, Cb and Cr with the chroma ones; restart intervals are counted in 16 x 8 MCUs.
 *   Bound         jpezy_jpeg_bound_sampling: 1024 + 1792 per 16 x 8 MCU (four blocks of at most 1661 bits = 831 bytes, 1662 stuffed,
 *                 plus restart / pad / EOI).
 *   Refused       gray != 0 (JPEZY_E_BADARG); encode variant 0 (JPEZY_E_UNSUPPORTED; the context stays usable).
 *   Alignment     none required.  W % 16 == 0 with 16-byte aligned planes and plane stride (packed: 16-byte aligned base and strides)
 *                 takes the 16-byte (48 / 64-byte) load form.
 * NOT provided for 4:2:2: the multi-GPU handle; planar YCbCr 4:2:2 or YUY2 / UYVY INPUT; 4:4:0; gray; encode variant 0; the lossless
 * transforms (jpezy_transform_jpeg refuses a 2x1 file, jpezy_transform_geometry / jpezy_coeff_transform_dev answer JPEZY_E_BADARG for any
 * sampling other than 0 and 1).
 */
#define JPEZY_SAMPLING_420 0
#define JPEZY_SAMPLING_444 1
#define JPEZY_SAMPLING_422 3   /* 2 is kept free for 4:4:0 and refused */
/* mcu_cols, mcu_rows, blocks_per_mcu (any may be NULL) of a W x H frame; pure host functions.  The counts are 0 for a bad argument. */
int jpezy_sampling_geometry(int sampling, int W, int H, int* mcu_cols, int* mcu_rows, int* blocks_per_mcu);
size_t jpezy_coeff_count_sampling(int W, int H, int sampling);   /* int16 elements per frame */
size_t jpezy_jpeg_bound_sampling(int W, int H, int sampling);
/* jpezy_fdct_quant_dev / jpezy_fdct_quant_packed_dev for the sampling: stand in for encoder/jpezy_encoder.hpp:90-172 (4:4:4: without
 * :116-143).  d_coeffs holds jpezy_coeff_count_sampling elements per frame.  Asynchronous on `stream`. */
int jpezy_fdct_quant_sampling_dev(jpezy_ctx* ctx, const uint8_t* d_r, const uint8_t* d_g, const uint8_t* d_b, size_t plane_stride, int W,
                                  int H, int sampling, int gray, int n_frames, int16_t* d_coeffs, void* stream);
int jpezy_fdct_quant_sampling_packed_dev(jpezy_ctx* ctx, const uint8_t* d_pix, int format, size_t row_stride, size_t frame_stride, int W,
                                         int H, int sampling, int gray, int n_frames, int16_t* d_coeffs, void* stream);
/* jpezy_write_jpeg_qt for the sampling (host writer; stands in for encoder/jpezy_writer.hpp:20-105 + encoder/jpezy_encoder.hpp:174-242);
 * out must hold jpezy_jpeg_bound_sampling bytes to be safe for any coefficients */
long jpezy_write_jpeg_sampling(const int16_t* coeffs, int W, int H, int sampling, int gray, const char* comment, const uint8_t luma[64],
                               const uint8_t chroma[64], int restart_interval, int optimize, uint8_t* out, size_t cap);
/* jpezy_write_jpeg_gpu / _batch / _dev for the sampling: the GPU entropy coder on the sampling's MCUs; the bytes of jpezy_write_jpeg_sampling
 * with the context's DQT tables, restart interval (counted in the sampling's MCUs) and optimise setting.  out / d_out hold
 * jpezy_jpeg_bound_sampling bytes per frame to be safe.  _dev: asynchronous and capturable, JPEZY_E_UNSUPPORTED while
 * jpezy_ctx_set_huffman_optimize is on; a frame with a value outside the code tables gets JPEZY_E_FORMAT in its size slot, the others
 * are written. */
long jpezy_write_jpeg_gpu_sampling(jpezy_ctx* ctx, const int16_t* d_coeffs, int W, int H, int sampling, int gray, const char* comment,
                                   uint8_t* out, size_t cap);
int jpezy_write_jpeg_gpu_sampling_batch(jpezy_ctx* ctx, const int16_t* d_coeffs, int W, int H, int sampling, int gray, int n_frames,
                                        const char* comment, uint8_t* out, size_t cap, long* sizes);
int jpezy_write_jpeg_gpu_sampling_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, int W, int H, int sampling, int gray, int n_frames,
                                      const char* comment, uint8_t* d_out, size_t out_stride, long long* d_sizes, void* stream);
/* jpezy_huffman_histogram_dev for the sampling (the context's restart interval acts, as there) */
int jpezy_huffman_histogram_sampling_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, int W, int H, int sampling, int gray, int n_frames,
                                         unsigned long long* d_hist, void* stream);
/* the symbols that writer emits for the frame (host function): hist[k][sym], k in DHT order YDc, CDc, YAc, CAc; JPEZY_E_FORMAT (counts
 * of the clamped symbols) when a value lies outside the code tables */
int jpezy_huffman_histogram_sampling(const int16_t* coeffs, int W, int H, int sampling, int restart_interval, unsigned long long hist[4][256]);
/* jpezy_encode_jpeg / jpezy_encode_jpeg_packed for the sampling (encoder/jpezy_encoder.hpp:38-77) */
long jpezy_encode_jpeg_sampling(jpezy_ctx* ctx, const uint8_t* r, const uint8_t* g, const uint8_t* b, int W, int H, int sampling, int gray,
                                const char* comment, uint8_t* out, size_t cap);
long jpezy_encode_jpeg_sampling_packed(jpezy_ctx* ctx, const uint8_t* pix, int format, size_t row_stride, int W, int H, int sampling,
                                       int gray, const char* comment, uint8_t* out, size_t cap);

/*
 * CHROMA DOWNSAMPLING of the 4:2:0 RGB encode (opt-in context setting; default JPEZY_DOWNSAMPLE_POINT: every byte is what it was).
 * The reference point-samples -- Cb and Cr of the top-left pixel of every 2x2 (make_YCC, encoder/jpezy_encoder.hpp:134-142) -- so the
 * definition of the averaged mode is this project's own.  JPEZY_DOWNSAMPLE_AVERAGE changes that one step and nothing else:
 *
 *   Extension     the picture is extended to whole 16 x 16 MCUs by clamping pixel coordinates, as before (:101,104).
 *   Samples       Cb and Cr of EVERY pixel from RGB::Cb / Cr in the reference's FP64 order, truncating (:249-256): the per-pixel
 *                 samples of JPEZY_SAMPLING_444 -- signed integers, no + 128.
 *   Average       chroma sample (x', y') = (c[2y'][2x'] + c[2y'][2x'+1] + c[2y'+1][2x'] + c[2y'+1][2x'+1] + bias(x')) >> 2 with bias 1
 *                 for even x', 2 for odd x', and an arithmetic shift (it floors): libjpeg's h2v2_downsample (alternating bias 1, 2
 *                 and >> 2 on unsigned samples) carried over to signed samples -- adding 128 to the four inputs adds 128 to the
 *                 result.  A 2x2 never crosses an MCU edge; at an odd picture edge it averages the clamped duplicates.
 *   Unchanged     luma, DCT, quantiser, zig-zag, the coefficient layout [frame][mcu_y][mcu_x][6][64], jpezy_coeff_count,
 *                 jpezy_jpeg_bound, header and scan: the writers and both Huffman stages never learn that the mode exists.  A
 *                 picture whose 2x2s are uniform (every pixel doubled) gives the coefficients of JPEZY_DOWNSAMPLE_POINT.
 *   Acts on       every colour 4:2:0 RGB transform of the context: jpezy_fdct_quant[_dev], jpezy_fdct_quant_packed_dev,
 *                 jpezy_encode_jpeg[_packed], and the *_sampling* entries called with JPEZY_SAMPLING_420, which forward to those.
 *                 The setting is read when a transform is launched; no device table changes, so the setter waits for nothing.
 *   4:2:2         JPEZY_SAMPLING_422 consults the setting too, with its own horizontal-only rule (CHROMA SAMPLING above).
 *   Not consulted gray != 0 (no chroma is computed); JPEZY_SAMPLING_444 (nothing is decimated); the planar-YCbCr entries (*_ycc*:
 *                 the caller's chroma samples are the file's); the lossless transforms.  None of them changes a byte.
 *   Refused       any other mode: JPEZY_E_BADARG.  A colour 4:2:0 RGB transform with encode variant 0 (the FP64 kernel has no averaged
 *                 stage) while the mode is JPEZY_DOWNSAMPLE_AVERAGE: JPEZY_E_UNSUPPORTED, nothing launched, the context stays usable.
 *   Context settings  jpezy_ctx_set_force_exact (levels 0-3), _set_dc_table_lookup, _set_quality / _set_quant_tables,
 *                 _set_huffman_optimize and _set_restart_interval act as on the point-sampled transform.
 *
 * The multi-GPU handle (jpezy_multi_*, jpezy_encode_batch_multi) owns its contexts and always point-samples.
 * jpezy_ctx_chroma_downsampling returns the setting (JPEZY_E_BADARG for a null context).
 */
enum jpezy_downsampling { JPEZY_DOWNSAMPLE_POINT = 0, JPEZY_DOWNSAMPLE_AVERAGE = 1 };
int jpezy_ctx_set_chroma_downsampling(jpezy_ctx* ctx, int mode);
int jpezy_ctx_chroma_downsampling(jpezy_ctx* ctx);

/*
 * LOSSLESS TRANSFORMS: flip, rotate, transpose of a picture in the COEFFICIENT domain (what jpegtran -rotate / -flip / -transpose and
 * tjTransform do).  A caller with a .jpg that is to stand upright, mirrored or transposed needs no pixel: every output coefficient is an
 * input coefficient, possibly negated, so nothing is decoded to samples, nothing is quantised again and no generation of quality is lost.
 * The reference has no such mode; the definition is this project's own (restated in tests/transform_model.py).
 *
 *   Operations    libjpeg's JXFORM order; (x', y') an output pixel, W x H the (trimmed) source size:
 *                     op                        source pixel        out size  swap  mirror_x  mirror_y
 *                     0 JPEZY_XFORM_NONE        (x', y')            W x H     0     0         0
 *                     1 JPEZY_XFORM_HFLIP       (W-1-x', y')        W x H     0     1         0
 *                     2 JPEZY_XFORM_VFLIP       (x', H-1-y')        W x H     0     0         1
 *                     3 JPEZY_XFORM_TRANSPOSE   (y', x')            H x W     1     0         0
 *                     4 JPEZY_XFORM_TRANSVERSE  (W-1-y', H-1-x')    H x W     1     1         1
 *                     5 JPEZY_XFORM_ROT90       (y', H-1-x')        H x W     1     0         1      (clockwise)
 *                     6 JPEZY_XFORM_ROT180      (W-1-x', H-1-y')    W x H     0     1         1
 *                     7 JPEZY_XFORM_ROT270      (W-1-y', x')        H x W     1     1         0      (clockwise)
 *                 mirror_x / mirror_y: the SOURCE axis that is mirrored; swap: the axes change places.
 *   Blocks        per component plane, block grid Gc x Gr over the used source MCUs C x R (4:2:0 luma: 2C x 2R; 4:2:0 chroma and every
 *                 4:4:4 plane: C x R): output block (bx', by') is source block (sx, sy) = swap ? (by', bx') : (bx', by'), then
 *                 sx = Gc-1-sx if mirror_x, then sy = Gr-1-sy if mirror_y.  The output's MCU grid is C x R (R x C with swap) and its MCUs
 *                 hold their blocks in the writer's order: 4:2:0 Y00 Y01 Y10 Y11 Cb Cr, luma block (bx, by) being block 2*(by&1) + (bx&1) of
 *                 MCU (bx>>1, by>>1); 4:4:4 Y Cb Cr.
 *   Coefficients  natural order, v the vertical and u the horizontal frequency: out[v][u] = s * in[vs][us], (vs, us) = swap ? (u, v) : (v, u),
 *                 s = -1 when mirror_x * us + mirror_y * vs is odd.  In the buffers' zig-zag order that is one fixed permutation and a
 *                 64-bit sign mask per operation.  The DC never changes sign.  Negation is int16 two's complement: -32768 stays -32768 (no
 *                 decoded file has such an AC value; the device entry takes any int16).
 *   Tables        the quantiser tables travel with the coefficients: with swap the output's are the transposes, Q'[v][u] = Q[u][v]
 *                 (jpezy_quant_tables_transform; the Annex-K tables are not symmetric).
 *   Edges         m = 16 (4:2:0) or 8 (4:4:4).  A MIRRORED source axis whose length is no multiple of m would put the padding on the
 *                 leading edge: with flags = 0 that is JPEZY_E_UNSUPPORTED (the message names the axis and the multiple); with
 *                 JPEZY_XFORM_TRIM the partial MCU column / row is dropped, the length becomes floor(len / m) * m, and if nothing is left
 *                 the call is JPEZY_E_BADARG.  An axis that is not mirrored keeps its length and its partial MCU (TRANSPOSE never trims).
 *                 C, R are the MCU counts of the trimmed size; the source buffer keeps its own row pitch of mcu_cols(W).
 *   Files         jpezy_transform_jpeg accepts SOF0, 8 bit, three components sampled 2x2, 1x1, 1x1 or 1x1, 1x1, 1x1 (the layouts the
 *                 writer writes), every used quantiser entry in 1..255, Cb and Cr with tables of equal CONTENTS (ids may differ).  Y's
 *                 table goes out as table 0, the chroma table as table 1 (one table for all three: written twice).  The source's restart
 *                 interval and Huffman tables are read and not carried over.  Everything else -- one component, 4:2:2 and other factors,
 *                 a 16-bit DQT, precision other than 8, different Cb / Cr tables -- is JPEZY_E_UNSUPPORTED with the reason named, and the
 *                 context stays usable.  A coefficient outside the writer's code tables is the writer's JPEZY_E_FORMAT.
 *   Output file   the existing writer's file (jpezy_write_jpeg_sampling) for the output size and sampling: the (transposed) source tables
 *                 in DQT; the context's jpezy_ctx_set_huffman_optimize and jpezy_ctx_set_restart_interval settings, the interval counted in
 *                 OUTPUT MCUs; the context's own quantiser setting is NOT used and NOT changed; comment NULL carries the source's COM text
 *                 over (as jpezy_frame_info keeps it: at most 255 bytes), "" writes none.
 *   NOT carried   APPn segments (EXIF, ICC) and the JFIF density fields: the header is the writer's.  The orientation tag is not read.
 *   With JPEZY_XFORM_NONE the same path is lossless recompression: a file re-coded with per-image Huffman tables or restart intervals, not
 *                 one coefficient changed.
 *
 * NOT provided: 4:2:2 and other layouts; one-component files; cropping in the coefficient domain; the multi-GPU handle; a batch form of
 * jpezy_transform_jpeg (jpezy_coeff_transform_dev takes n_frames).
 */
enum jpezy_xform {
    JPEZY_XFORM_NONE = 0, JPEZY_XFORM_HFLIP = 1, JPEZY_XFORM_VFLIP = 2, JPEZY_XFORM_TRANSPOSE = 3, JPEZY_XFORM_TRANSVERSE = 4,
    JPEZY_XFORM_ROT90 = 5, JPEZY_XFORM_ROT180 = 6, JPEZY_XFORM_ROT270 = 7
};
#define JPEZY_XFORM_TRIM 1      /* flags: drop the partial MCU column / row of a mirrored axis */
/* The edge rule alone (pure host function): Wout x Hout = the output's size, src_cols x src_rows = C x R, the source MCUs that are used.
 * Any output pointer may be NULL.  JPEZY_E_BADARG: op outside 0..7, unknown flag bits, unknown sampling, a size outside 1..65535, nothing
 * left after trimming; JPEZY_E_UNSUPPORTED: a mirrored axis with a partial MCU and no JPEZY_XFORM_TRIM. */
int jpezy_transform_geometry(int op, int flags, int W, int H, int sampling, int* Wout, int* Hout, int* src_cols, int* src_rows);
/* The kernel on device memory (jpezy_kernels_transform.hip): n_frames coefficient fields of a W x H picture (jpezy_coeff_count_sampling(W,
 * H, sampling) elements each, consecutive) from d_in to d_out (jpezy_coeff_count_sampling(Wout, Hout, sampling) elements each).  d_out is
 * a DIFFERENT buffer: overlapping ranges are JPEZY_E_BADARG, as are pointers that are not 16-byte aligned.  Asynchronous on `stream` and
 * capturable: it neither allocates nor synchronises, and touches no state of the context.  Any n_frames > 0 (launches of at most 65535
 * frames).  Arguments are checked before the context is looked at. */
int jpezy_coeff_transform_dev(jpezy_ctx* ctx, const int16_t* d_in, int W, int H, int sampling, int op, int flags, int n_frames, int16_t* d_out,
                              void* stream);
/* Q'[v][u] = Q[u][v] for the operations with swap, a copy for the others (pure host function; natural order; in == out is allowed). */
int jpezy_quant_tables_transform(int op, const uint8_t in[64], uint8_t out[64]);
/* A .jpg in, the transformed .jpg out: the header on the host, the scan through the path jpezy_read_jpeg_gpu takes (the host decoder below
 * jpezy_ctx_set_huffdec_min_bytes and for irregular streams, as there), the transform kernel, the GPU entropy coder.  Returns the bytes
 * written or a negative status.  out_info receives the OUTPUT's header fields (size, MCU grid, tables, restart interval, comment).
 * out == NULL: header and geometry only (returns 0).  A cap of jpezy_jpeg_bound_sampling(Wout, Hout, sampling) is always enough; a smaller
 * one that does not hold the file is JPEZY_E_NOSPACE and nothing is written past it.  Synchronous; the second coefficient buffer lives in
 * the context, and the rule of the entropy entry points (one call in flight per context) applies. */
long jpezy_transform_jpeg(jpezy_ctx* ctx, const uint8_t* data, size_t len, int op, int flags, const char* comment, jpezy_frame_info* out_info,
                          uint8_t* out, size_t cap);

/*
 * CHROMA UPSAMPLING.  The decoder brings a subsampled component up to picture size by replication, because the reference's decode_mcu
 * does (decoder/jpezy_decoder.hpp:504-528): on a 4:2:0 file that puts 2 x 2 steps on every coloured edge and gradient.  libjpeg,
 * libjpeg-turbo and nvJPEG interpolate 2:1 chroma with a triangle filter by default ("fancy upsampling").  upsampling selects:
 *
 *   JPEZY_UPSAMPLE_NEAREST = 0   today's behaviour: the call is handed to the existing entry point named with each function, under that
 *                                entry's own rules -- the same kernels, byte for byte the existing decode
 *   JPEZY_UPSAMPLE_SMOOTH  = 1   below.  The reference has no such mode; the definition is this project's own (restated
 *                                in tests/smooth_model.py).  Any other value: JPEZY_E_BADARG.
 *
 *   Smoothed      component c with sampling (H_c, V_c) is smoothed iff hmax % H_c == 0, vmax % V_c == 0 and (fx, fy) = (hmax / H_c,
 *                 vmax / V_c) is (2, 1), (1, 2) or (2, 2).  Every other component -- full resolution, factors 3 and 4, the reference's
 *                 overwrite quirk for factors that do not divide -- is placed exactly as the existing decode places it.  A file with no
 *                 smoothed component (4:4:4, one component, the chroma of 4:1:1) therefore decodes byte for byte as it does today.
 *   Native plane  P of a smoothed component is wc x hc = ceil(W*H_c/hmax) x ceil(H*V_c/vmax) (jpezy_ycc_component_size);
 *                 P[y][x] = min(max(sample, 0), 255) of the integer sample inverse_dct gives (:645-670), block ((x>>3) % H_c, (y>>3) % V_c)
 *                 of MCU ((x>>3) / H_c, (y>>3) / V_c): exactly the bytes jpezy_decode_jpeg_ycc returns for that component.  Reads outside
 *                 the plane clamp their coordinates to [0, wc-1] x [0, hc-1]: the edge is the component's true extent, not the padded block.
 *   Filter        U(X, Y) for X < W, Y < H, with i = X>>1, j = Y>>1, integer arithmetic, >> a shift of a non-negative int:
 *                   (2,1)  X even: (3*P(i,Y) + P(i-1,Y) + 1) >> 2          X odd: (3*P(i,Y) + P(i+1,Y) + 2) >> 2
 *                   (1,2)  Y even: (3*P(X,j) + P(X,j-1) + 1) >> 2          Y odd: (3*P(X,j) + P(X,j+1) + 2) >> 2
 *                   (2,2)  d = -1 for even Y, +1 for odd Y; S(i) = 3*P(i,j) + P(i,j+d);
 *                          X even: (3*S(i) + S(i-1) + 8) >> 4              X odd: (3*S(i) + S(i+1) + 7) >> 4
 *                 These are libjpeg's h2v1 / h1v2 / h2v2 fancy upsamplers; the coordinate clamp reproduces their special-cased first and
 *                 last columns.  libjpeg replicates planes no wider than two samples; here the formula holds at every size.
 *   Colour        make_rgb / revise_value and gray (:531-578, 672-676) as always, in the reference's FP64 order: a smoothed component
 *                 enters as U, every other component as the integer sample it has today, unclamped as today.
 *   Siting        the filter takes chroma to sit at the centre of its 2 x 2 (JFIF, libjpeg's writer).  jpezy_encode_jpeg keeps the top-left
 *                 pixel's chroma as the reference does, so on its files the filter is half a pixel off in phase; the mode is made for
 *                 files from elsewhere and for centred chroma fed through jpezy_encode_jpeg_ycc.
 *   Kernels       every layout, jpezy's own included, takes the any-layout pair: generic_idct_kernel unchanged (fast path, guard band,
 *                 jpezy_ctx_set_force_exact and the fallback counter as in jpezy_dequant_idct_generic_dev), then smooth_rgb_kernel
 *                 (jpezy_kernels_smooth.hip) in generic_rgb_kernel's place.  jpezy_ctx_set_decode_tolerance has nothing to act on.
 *   Refused       precision != 8 with JPEZY_UPSAMPLE_SMOOTH: JPEZY_E_UNSUPPORTED, the context stays usable.
 *
 * NOT provided here: jpezy_decode_jpeg_batch; a fused one-pass kernel for jpezy's own layout (it
 * would need a halo from the neighbouring MCUs); 12-bit files; the host-buffer jpezy_dequant_idct* entries; a box-average decimation in
 * the encoder (the natural follow-up: it would make the encoder's own files centred).  Region decode, reduced sizes and the batches of
 * windows take the mode through SMOOTH UPSAMPLING OF WINDOWS below.
 */
enum jpezy_upsampling { JPEZY_UPSAMPLE_NEAREST = 0, JPEZY_UPSAMPLE_SMOOTH = 1 };
/* jpezy_dequant_idct_generic_batch_dev with the upsampling chosen (stands in for decoder/jpezy_decoder.hpp:504-578, 645-676; the reference
 * replicates, the smooth definition above is this project's own): d_r, d_g, d_b planes of W*H bytes, frame f's at + f * plane_stride
 * (n_frames > 1: >= W*H and a multiple of 4, the generic batch entry's rule).  Asynchronous on `stream` and capturable; the generic entry's
 * table, scratch (one call in flight per context) and capture rules apply; more than 65535 frames go out as several pairs of launches.
 * JPEZY_UPSAMPLE_NEAREST: jpezy_dequant_idct_generic_dev for one frame, jpezy_dequant_idct_generic_batch_dev for more. */
int jpezy_dequant_idct_upsampling_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                      const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray, int upsampling,
                                      int n_frames, size_t plane_stride, uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream);
/* The same writing packed pixels (same reference lines, same remark).  The addressing rules of the packed section apply: pixel (x, y) of
 * frame f at d_pix + f*frame_stride + y*row_stride + x*bytes, row_stride 0 = W*bytes, frame_stride 0 = H*row_stride, only bytes
 * [0, W*bytes) of a row are written, byte 3 of a 32-bit pixel is 0xFF; n_frames > 1 asks for a frame_stride that is a multiple of 4.
 * JPEZY_UPSAMPLE_NEAREST: the generic kernels' packed store stage, as jpezy_dequant_idct_scaled_packed_dev reaches it at scale_denom 1. */
int jpezy_dequant_idct_upsampling_packed_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp,
                                             const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W,
                                             int H, int gray, int upsampling, int format, size_t row_stride, size_t frame_stride, int n_frames,
                                             uint8_t* d_pix, void* stream);
/* jpezy_decode_jpeg with the upsampling chosen (decoder/jpezy_decoder.hpp:76-134 with the second stage above; the reference replicates):
 * header parse and Huffman decoding exactly as jpezy_decode_jpeg does them (GPU decoder, host decoder for what it declines), then the two
 * stages and a download of W*H bytes per plane.  r, g, b NULL: header only (a 12-bit file is refused there already);
 * plane_cap < W*H: JPEZY_E_NOSPACE.  JPEZY_UPSAMPLE_NEAREST: jpezy_decode_jpeg. */
int jpezy_decode_jpeg_upsampling(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, int upsampling, jpezy_frame_info* info, uint8_t* r,
                                 uint8_t* g, uint8_t* b, size_t plane_cap);
/* The same into host packed pixels (jpezy_decode_jpeg_packed with the upsampling chosen; same reference lines and remark): pix NULL: header
 * only; pix_cap < (H-1)*row_stride + W*bytes: JPEZY_E_NOSPACE.  JPEZY_UPSAMPLE_NEAREST: jpezy_decode_jpeg_packed. */
int jpezy_decode_jpeg_upsampling_packed(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, int upsampling, jpezy_frame_info* info,
                                        int format, size_t row_stride, uint8_t* pix, size_t pix_cap);

/*
 * SMOOTH UPSAMPLING OF WINDOWS.  The chroma upsampling above as a property of the window decode: one window of one file
 * (jpezy_*_region_upsampling*), a batch of windows and a batch of windows resized (jpezy_ctx_set_windows_upsampling), at full size and at
 * 1/2, 1/4, 1/8, for any layout.  JPEZY_UPSAMPLE_NEAREST stays the default and is handed to the existing entry, byte for byte.  With
 * JPEZY_UPSAMPLE_SMOOTH, let s = scale_denom in {1, 2, 4, 8}, N = 8 / s and Ws x Hs = jpezy_scaled_size(W, H, s):
 *
 *   Smoothed      the rule of CHROMA UPSAMPLING, unchanged: hmax % H_c == 0, vmax % V_c == 0, (fx, fy) = (hmax / H_c, vmax / V_c) one of
 *                 (2,1), (1,2), (2,2).  Every other component is placed exactly as the (scaled) nearest decode places it: replication,
 *                 later blocks overwrite earlier ones, unclamped samples.
 *   Native plane  P_s of a smoothed component is wc_s x hc_s = ceil(Ws / fx) x ceil(Hs / fy) (libjpeg's downsampled_width of the reduced
 *                 picture; at s = 1 the wc x hc above).  Block (bx, by) of the component's own block grid -- block (bx % H_c, by % V_c) of MCU
 *                 (bx / H_c, by / V_c) -- gives the N x N samples at (bx*N, by*N); a sample is ref_int(sum / 4 + 128) over the N x N
 *                 low-frequency corner in the reduced-size decode's order (v outer, u inner, left to right in binary64; REDUCED-SIZE DECODE),
 *                 clamped to 0..255.  At s = 1 this is P.
 *   Filter        the formulas above applied to P_s for X < Ws, Y < Hs; coordinates outside P_s clamp to [0, wc_s-1] x [0, hc_s-1], the
 *                 plane's true extent, not the padded block.
 *   Colour        make_rgb / revise_value and gray as always.
 *   Window        {x, y, w, h} is rows y .. y+h, columns x .. x+w of that picture; the window checks are jpezy_region_check's.
 *
 * Consequences: at s = 1 the result is byte for byte the slice of what jpezy_decode_jpeg_upsampling[_packed] returns; a file with no smoothed
 * component gives byte for byte the existing region decode at every scale.  12-bit files: JPEZY_E_UNSUPPORTED ("8-bit").
 * For s != 1 NO OUTSIDE REFERENCE EXISTS: at reduced sizes libjpeg does not filter at all, it gives chroma a larger inverse DCT
 * (jdmaster.c, per-component DCT_scaled_size).  One filter at every scale, over the planes the reduced decode already defines, is this
 * project's own rule (restated in tests/region_smooth_model.py).
 * Kernels: region_smooth_kernel / windows_smooth_kernel (jpezy_kernels_region_smooth.hip) in region_kernel's / windows_kernel's place: one
 * launch, one workgroup per MCU that intersects the window, no intermediate in device memory.  A window that is the whole picture runs the
 * same kernel (there is no smooth reduced-size entry to hand it to).
 *
 * NOT provided: the mode in jpezy::Decoder / the jpezy_decode CLI together with --scale / --region (they keep refusing it); planar or
 * host-memory batches of windows; libjpeg-style IDCT-scaled chroma at reduced sizes; 12-bit files.
 */
/* The four region entries with the upsampling chosen -- jpezy_dequant_idct_region_upsampling_dev, jpezy_dequant_idct_region_upsampling_packed_dev,
 * jpezy_decode_jpeg_region_upsampling, jpezy_decode_jpeg_region_upsampling_packed -- are declared in a header of their own, part of this one.
 * The decode entries declared in THIS file are a closed set: what each of them answers to a fixed table of calls is recorded
 * (tests/golden/decode_entry_errors.json) and replayed against every build.  The new entries' answers are pinned to the region entries'
 * own instead, call by call (tests/test_region_smooth_abi.py). */
#include "jpezy_hip_region_upsampling.h"
/* The chroma upsampling of jpezy_decode_windows_dev and jpezy_decode_windows_resized_dev (no counterpart in the reference: a setting of this
 * library's context): JPEZY_UPSAMPLE_NEAREST (the default: exactly the launches made without this setting) or JPEZY_UPSAMPLE_SMOOTH -- the
 * grouped path launches windows_smooth_kernel, the per-file path the region stage in smooth mode; the resampling stage behind either is
 * unchanged.  A 12-bit file then gets JPEZY_E_UNSUPPORTED for that file: its slot is untouched, the others are complete.  Any other value,
 * or a null context: JPEZY_E_BADARG, the setting unchanged.  The getter returns the setting (JPEZY_E_BADARG for a null context). */
int jpezy_ctx_set_windows_upsampling(jpezy_ctx* ctx, int upsampling);
int jpezy_ctx_windows_upsampling(jpezy_ctx* ctx);

/*
 * ORIENTED OUTPUT.  The EXIF Orientation tag, applied in the store stage of the window decode: the picture the existing decode returns --
 * at any scale, nearest or smooth -- mirrored, rotated or transposed by one of the tag's eight values, and windows taken from THAT picture.
 * Orientation 4 is the vertical mirror the sections above list as not provided; the other seven come from the same mechanism.  The tag's
 * parser, the geometry helpers, the region and file entries with an orientation argument and the context setting of the window batches
 * are declared, and the rule is spelled out, in a header of their own, part of this one -- for the reason given above
 * jpezy_hip_region_upsampling.h: the decode entries declared in THIS file are a closed, recorded set.  Nothing declared here changes:
 * without the new entries and with the setting at its default every launch is the one made before.
 */
#include "jpezy_hip_orientation.h"

/*
 * YCbCr 4:2:2 SAMPLES IN AND OUT (planar I422 / NV16, packed YUY2 / UYVY / YVYU): the 4:2:2 counterpart of the planar 4:2:0 section above.
 * The definition and the entries are in a header of their own, part of this one, for the reason given above
 * jpezy_hip_region_upsampling.h.  Nothing declared here changes.
 */
#include "jpezy_hip_ycc422.h"

#ifdef __cplusplus
}
#endif
#endif
