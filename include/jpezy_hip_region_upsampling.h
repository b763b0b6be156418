/* jpezy_hip_region_upsampling.h -- part of jpezy_hip.h (included by it, inside its extern "C"; not to be included on its own): the region
 * entries with the chroma upsampling as an argument.  The definition is jpezy_hip.h's section SMOOTH UPSAMPLING OF WINDOWS. */
#ifndef JPEZY_HIP_REGION_UPSAMPLING_H
#define JPEZY_HIP_REGION_UPSAMPLING_H
#ifndef JPEZY_HIP_H
#error "include jpezy_hip.h"
#endif

/* jpezy_dequant_idct_region_dev with the upsampling chosen (stands in for decoder/jpezy_decoder.hpp:504-578, 645-676; the reference
 * replicates and has no window, the definition above is this project's own): the entry's arguments, checks and order of checks, with the
 * upsampling check in front of them.  JPEZY_UPSAMPLE_NEAREST: jpezy_dequant_idct_region_dev. */
int jpezy_dequant_idct_region_upsampling_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                             const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray,
                                             int upsampling, int scale_denom, const jpezy_rect* region, int n_frames, size_t plane_stride,
                                             uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream);
/* The same writing packed pixels (same reference lines, same remark).  JPEZY_UPSAMPLE_NEAREST: jpezy_dequant_idct_region_packed_dev. */
int jpezy_dequant_idct_region_upsampling_packed_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp,
                                                    const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W,
                                                    int H, int gray, int upsampling, int scale_denom, const jpezy_rect* region, int format,
                                                    size_t row_stride, size_t frame_stride, int n_frames, uint8_t* d_pix, void* stream);
/* jpezy_decode_jpeg_region with the upsampling chosen (decoder/jpezy_decoder.hpp:76-134 with the stage above; the reference replicates and
 * has no window).  A 12-bit file is refused once its header is read.  JPEZY_UPSAMPLE_NEAREST: jpezy_decode_jpeg_region. */
int jpezy_decode_jpeg_region_upsampling(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, int upsampling, int scale_denom,
                                        const jpezy_rect* region, jpezy_frame_info* info, uint8_t* r, uint8_t* g, uint8_t* b, size_t plane_cap);
/* The same into host packed pixels (same reference lines and remark).  JPEZY_UPSAMPLE_NEAREST: jpezy_decode_jpeg_region_packed. */
int jpezy_decode_jpeg_region_upsampling_packed(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, int upsampling, int scale_denom,
                                               const jpezy_rect* region, jpezy_frame_info* info, int format, size_t row_stride, uint8_t* pix,
                                               size_t pix_cap);
#endif
