/* jpezy_hip_ycc422.h -- part of jpezy_hip.h (included by it, inside its extern "C"; not to be included on its own): YCbCr 4:2:2 SAMPLES IN
 * AND OUT -- planar I422 / YV16 (ffmpeg's yuvj422p) and NV16 / NV61, and packed macropixels YUY2 / UYVY / YVYU -- without an RGB detour.
 * A capture card, a webcam, an MJPEG or video pipeline holds its frames in one of these forms, which is a 4:2:2 file's own sample domain,
 * as I420 / NV12 is a 4:2:0 file's (jpezy_hip.h, PLANAR YCbCr 4:2:0 SAMPLES).  The reference only takes RGB
 * (encoder/jpezy_encoder.hpp:24-28), only writes 4:2:0 and only gives RGB (decoder/jpezy_decoder.hpp:531-578), so the definition is this
 * project's own (restated in tests/ycc422_model.py):
 *
 *   Sizes         CW = ceil(W/2), CH = H.  A packed row holds ceil(W/2) macropixels of 4 bytes: row_bytes = 4 * ceil(W/2).
 *   Formats       a macropixel covers pixels 2x', 2x'+1:  JPEZY_YUV_YUY2  Y0 Cb Y1 Cr;  JPEZY_YUV_UYVY  Cb Y0 Cr Y1;  JPEZY_YUV_YVYU  Y0 Cr Y1 Cb.
 *                 All samples are full range; the caller's bytes are the file's samples.
 *   Encode        16 x 8 MCUs of four blocks Y-left, Y-right, Cb, Cr; coefficients int16 [frame][mcu_y][mcu_x][4][64] zig-zag, the layout
 *                 and geometry of jpezy_sampling_geometry(JPEZY_SAMPLING_422, W, H).  Luma sample (x, y) of the clamp-extended picture is
 *                 (int)Y[min(y, H-1)][min(x, W-1)] - 128, chroma sample (x', y) is (int)C[min(y, H-1)][min(x', CW-1)] - 128; every block
 *                 goes through the reference's DCT and quantization(cs) with the context's tables.  With an odd W the second Y byte of a
 *                 packed row's last macropixel is not read.
 *   File          the 4:2:2 file of those coefficients (SOF0 2,1 / 1,1 / 1,1), byte for byte what jpezy_write_jpeg_sampling gives for
 *                 them; quality / caller tables, optimised Huffman tables and restart intervals compose as for the RGB 4:2:2 entries; the
 *                 bound is jpezy_jpeg_bound_sampling(W, H, JPEZY_SAMPLING_422).
 *   Anchor        planes made from RGB pixels as Y = trunc(ref luma) + 128 of every pixel, Cb / Cr = trunc(ref chroma) + 128 of pixel
 *                 (2x', y) give the coefficients of jpezy_fdct_quant_sampling_dev(.., JPEZY_SAMPLING_422) (point sampling) whenever W is a
 *                 multiple of 16 or odd; the luma blocks agree at every size.  (An even W that is no multiple of 16: the RGB path
 *                 replicates pixel W-1, whose chroma no 4:2:2 plane holds.)
 *   Settings      jpezy_ctx_set_chroma_downsampling is not consulted: the chroma is the caller's.  Encode variant 0 (FP64) is refused with
 *                 JPEZY_E_UNSUPPORTED and the context stays usable.  There is no gray form.  jpezy_ctx_set_force_exact (levels 1-3),
 *                 _set_huffman_optimize, _set_restart_interval and the quantisation tables act as on the RGB 4:2:2 entries.
 *   Decode        to packed 4:2:2 from ANY layout the any-layout pair accepts.  The Y byte of pixel (x, y) is revise_value of the luma
 *                 sample (the r plane of jpezy_decode_jpeg(.., gray = 1), the y plane of jpezy_decode_jpeg_ycc).  The Cb / Cr byte of
 *                 macropixel x' in row y is revise_value of the component sample the nearest-neighbour decode feeds make_rgb for pixel
 *                 (2x', y): a 2x1 file's native sample (x', y) -- jpezy_decode_jpeg_ycc's chroma planes --, a 2x2 file's sample
 *                 (x', y >> 1), a 1x1 file's sample at the even pixel (the encoder's point-sampling rule in reverse), 0x80 for a
 *                 one-component file.  With an odd W the last macropixel's second Y byte is a copy of its first: every one of a row's
 *                 row_bytes bytes is defined, nothing between row_bytes and row_stride is touched.
 *
 * NOT provided in this form: smooth upsampling, reduced size, regions and windows, the batch and multi-GPU entries, a gray encode,
 * limited-range (16-235) video levels.
 *
 * Check order: sizes, format, c_step, strides and null pointers come before the context (a null context still gets these messages), then
 * the context, the alignment of d_coeffs and the variant.  Batches of more than 65535 frames go out as several launches.
 */
#ifndef JPEZY_HIP_YCC422_H
#define JPEZY_HIP_YCC422_H
#ifndef JPEZY_HIP_H
#error "include jpezy_hip.h"
#endif

enum { JPEZY_YUV_YUY2 = 0, JPEZY_YUV_UYVY = 1, JPEZY_YUV_YVYU = 2 };

/* 4 * ceil(W/2), the bytes of a packed row; JPEZY_E_BADARG for a W outside 1..65535.  Pure host function (no counterpart in the reference,
 * which has no packed form). */
int jpezy_yuv422_row_bytes(int W);
/* CW = ceil(W/2), CH = H (either may be NULL) of a W x H picture; JPEZY_E_BADARG for a size outside 1..65535.  Pure host function (stands
 * in for the chroma extent of encoder/jpezy_encoder.hpp:101-104 at 2x1 sampling). */
int jpezy_ycc422_chroma_size(int W, int H, int* CW, int* CH);

/* Planar samples on the device -> coefficients (stands in for make_YCC + DCT + quantization, encoder/jpezy_encoder.hpp:58-67, 92-121, with
 * the planes in make_YCC's place).  I422 / YV16: c_step 1; NV16 / NV61: c_step 2, d_cb and d_cr one byte apart.  Arguments and addressing
 * rules of jpezy_fdct_quant_ycc_dev with CH = H: strides in bytes, 0 = tight (W; CW * c_step; H * y_stride; H * c_stride);
 * y_stride * H and c_stride * H must fit 32 bits.  Asynchronous on `stream`. */
int jpezy_fdct_quant_ycc422_dev(jpezy_ctx* ctx, const uint8_t* d_y, size_t y_stride, const uint8_t* d_cb, const uint8_t* d_cr, size_t c_stride,
                                int c_step, size_t y_frame_stride, size_t c_frame_stride, int W, int H, int n_frames, int16_t* d_coeffs,
                                void* stream);
/* Host planes -> .jpg bytes (encoder::encode end to end, encoder/jpezy_encoder.hpp:38-77, from samples).  Returns the file's size. */
long jpezy_encode_jpeg_ycc422(jpezy_ctx* ctx, const uint8_t* y, size_t y_stride, const uint8_t* cb, const uint8_t* cr, size_t c_stride, int c_step,
                              int W, int H, const char* comment, uint8_t* out, size_t cap);
/* Packed macropixels on the device -> coefficients (same reference lines).  row_stride 0 = row_bytes, frame_stride 0 = H * row_stride;
 * row_stride * H must fit 32 bits.  Asynchronous on `stream`. */
int jpezy_fdct_quant_yuv422_dev(jpezy_ctx* ctx, const uint8_t* d_pix, int format, size_t row_stride, size_t frame_stride, int W, int H,
                                int n_frames, int16_t* d_coeffs, void* stream);
/* Host macropixels -> .jpg bytes (encoder/jpezy_encoder.hpp:38-77, from samples).  Returns the file's size. */
long jpezy_encode_jpeg_yuv422(jpezy_ctx* ctx, const uint8_t* pix, int format, size_t row_stride, int W, int H, const char* comment, uint8_t* out,
                              size_t cap);
/* Coefficients of any layout on the device -> packed 4:2:2 on the device: n_frames frames of one layout, frame_stride apart (stands in for
 * decoder/jpezy_decoder.hpp:504-528, 645-676 without make_rgb, :531-578).  The arguments of jpezy_dequant_idct_generic_batch_dev with the
 * packed sink in the planes' place.  Asynchronous on `stream`. */
int jpezy_dequant_idct_generic_yuv422_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                          const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int format,
                                          size_t row_stride, size_t frame_stride, int n_frames, uint8_t* d_pix, void* stream);
/* .jpg bytes -> host macropixels (decoder::decode end to end, decoder/jpezy_decoder.hpp:76-134, without make_rgb).  pix NULL: header only.
 * JPEZY_E_NOSPACE when pix_cap is below (H-1) * row_stride + row_bytes.  Every layout, this project's own 4:2:0 files included, goes
 * through the any-layout pair: two launches, not the fused kernel's one.  Only row_bytes of each caller row are written. */
int jpezy_decode_jpeg_yuv422(jpezy_ctx* ctx, const uint8_t* data, size_t len, jpezy_frame_info* info, int format, size_t row_stride,
                             uint8_t* pix, size_t pix_cap);
#endif
