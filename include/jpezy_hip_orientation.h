/* jpezy_hip_orientation.h -- part of jpezy_hip.h (included by it, inside its extern "C"; not to be included on its own): the EXIF
 * Orientation tag and oriented output of the window decode.  The definition is jpezy_hip.h's section ORIENTED OUTPUT, spelled out here.
 *
 * Let P be the picture the existing decode returns: Ws x Hs = jpezy_scaled_size(W, H, s) pixels at any scale s in {1, 2, 4, 8}, with
 * JPEZY_UPSAMPLE_NEAREST or JPEZY_UPSAMPLE_SMOOTH.  The oriented picture O = orient(P, o), o in 1..8 (the values of the EXIF tag):
 *
 *      o   O                                   source pixel of O[Y][X]
 *      1   P                                   (X, Y)
 *      2   P mirrored left-right               (Ws-1-X, Y)
 *      3   P rotated by 180 degrees            (Ws-1-X, Hs-1-Y)
 *      4   P mirrored top-bottom               (X, Hs-1-Y)
 *      5   P transposed                        (Y, X)
 *      6   P rotated by 90 degrees clockwise   (Y, Hs-1-X)
 *      7   P transposed over the anti-diagonal (Ws-1-Y, Hs-1-X)
 *      8   P rotated by 90 degrees counter-cw  (Ws-1-Y, X)
 *
 * O is Hs x Ws pixels for o >= 5.  A window {x, y, w, h} of an oriented decode is rows y .. y+h, columns x .. x+w of O: every byte is a byte
 * of the existing decode, moved.  The rule is a PERMUTATION OF PIXELS, not a transform of coefficients (the inverse DCT's summation order,
 * replication and the smooth filter's rounding do not commute with a transposition bit for bit), so a partial MCU at the right or bottom
 * edge is no obstacle: unlike jpezy_transform_jpeg nothing is refused or trimmed.  The reference has no such mode; the definition is this
 * project's own (restated in tests/orient_model.py, whose eight maps agree with Pillow's ImageOps.exif_transpose).
 * Kernels: the ORIENT instances of region_kernel / region_smooth_kernel / windows_kernel / windows_smooth_kernel (jpezy_kernels_region.hip):
 * the same launch, the same samples in LDS, a different read pattern of them in the store stage -- no second pass, no intermediate.
 *
 * NOT provided: native component (YCbCr) planes; jpezy_decode_jpeg_batch; an orientation per file given by the caller; carrying EXIF
 * through the encoder or jpezy_transform_jpeg; tags in IFDs other than IFD0. */
#ifndef JPEZY_HIP_ORIENTATION_H
#define JPEZY_HIP_ORIENTATION_H
#ifndef JPEZY_HIP_H
#error "include jpezy_hip.h"
#endif

/* the orientation argument of the file entries: the file's own tag */
#define JPEZY_ORIENT_FROM_FILE 0

/* The EXIF Orientation of a .jpg in host memory (no counterpart in the reference, which skips every APPn segment; pure host function, no
 * context, never fails): the tag's value 1..8, or 1 when anything is missing or wrong.  The first APP1 segment in front of SOS whose
 * payload starts with "Exif\0\0" decides; both byte orders ("II*\0", "MM\0*"); IFD0 only; tag 0x0112 of type SHORT (or LONG) and count 1;
 * a value outside 1..8 gives 1.  Every offset is checked against the segment before it is used; nothing outside data[0, len) is read;
 * data NULL or len 0 gives 1. */
int jpezy_jpeg_orientation(const uint8_t* data, size_t len);
/* The size of orient(P, o) for a P of W x H pixels (own definition; pure): W x H for o in 1..4, H x W for o in 5..8.
 * o outside 1..8, W or H < 1, or a null pointer: JPEZY_E_BADARG. */
int jpezy_orient_size(int orientation, int W, int H, int* Wo, int* Ho);
/* The rectangle of P (W x H pixels) whose pixels the window `oriented` of orient(P, o) shows (own definition; pure): `source` has the
 * window's size, transposed for o >= 5.  Checks in this order: a null pointer, o outside 1..8, W or H < 1, then a window with w, h < 1 or
 * x, y < 0 or one that lies outside the oriented picture: JPEZY_E_BADARG each. */
int jpezy_orient_rect(int orientation, int W, int H, const jpezy_rect* oriented, jpezy_rect* source);

/* jpezy_dequant_idct_region_upsampling_dev with the orientation chosen (stands in for decoder/jpezy_decoder.hpp:504-578, 645-676; the
 * reference has neither window nor orientation): `region` is a window of orient(P, orientation) and the output is its w x h pixels, planes
 * w apart.  The orientation check comes first (outside 1..8: JPEZY_E_BADARG), then the entry's own checks in its order with the region held
 * against the ORIENTED picture.  Orientation 1 with JPEZY_UPSAMPLE_NEAREST: jpezy_dequant_idct_region_dev, byte for byte; orientation 1
 * otherwise: jpezy_dequant_idct_region_upsampling_dev.  Asynchronous on `stream`, capturable as that entry is. */
int jpezy_dequant_idct_region_oriented_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp, const uint8_t comp_h[3],
                                           const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W, int H, int gray, int upsampling,
                                           int scale_denom, const jpezy_rect* region, int orientation, int n_frames, size_t plane_stride,
                                           uint8_t* d_r, uint8_t* d_g, uint8_t* d_b, void* stream);
/* The same writing packed pixels (same reference lines, same remark): jpezy_dequant_idct_region_upsampling_packed_dev's arguments and
 * checks. */
int jpezy_dequant_idct_region_oriented_packed_dev(jpezy_ctx* ctx, const int16_t* d_coeffs, const uint16_t qt[4][64], int ncomp,
                                                  const uint8_t comp_h[3], const uint8_t comp_v[3], const uint8_t comp_tq[3], int precision, int W,
                                                  int H, int gray, int upsampling, int scale_denom, const jpezy_rect* region, int orientation,
                                                  int format, size_t row_stride, size_t frame_stride, int n_frames, uint8_t* d_pix, void* stream);
/* jpezy_decode_jpeg_region_upsampling with the orientation chosen (decoder/jpezy_decoder.hpp:76-134 with the stage above; the reference
 * ignores the tag).  orientation: 1..8, or JPEZY_ORIENT_FROM_FILE for jpezy_jpeg_orientation(data, len); anything else JPEZY_E_BADARG.
 * region: a window of the oriented picture, NULL: all of it (the region stage then, not the fused kernel).  *orientation_used (may be
 * NULL) is what was applied, set as soon as the arguments are found sound.  Checks in this order: upsampling, orientation, info NULL,
 * scale_denom, the region's syntax, ctx NULL; then the file.  r, g, b NULL: header only -- info holds the FILE's width and height, as for
 * the region entries.  plane_cap < w * h: JPEZY_E_NOSPACE.  Orientation 1 with a region: jpezy_decode_jpeg_region_upsampling. */
int jpezy_decode_jpeg_oriented(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, int upsampling, int scale_denom, const jpezy_rect* region,
                               int orientation, int* orientation_used, jpezy_frame_info* info, uint8_t* r, uint8_t* g, uint8_t* b,
                               size_t plane_cap);
/* The same into host packed pixels (same reference lines and remark); the format and stride checks stand behind the region's syntax when a
 * region is given, behind the header otherwise (the output's size is the file's to say). */
int jpezy_decode_jpeg_oriented_packed(jpezy_ctx* ctx, const uint8_t* data, size_t len, int gray, int upsampling, int scale_denom,
                                      const jpezy_rect* region, int orientation, int* orientation_used, jpezy_frame_info* info, int format,
                                      size_t row_stride, uint8_t* pix, size_t pix_cap);

/* The orientation of jpezy_decode_windows_dev, jpezy_decode_windows_resized_dev and jpezy_decode_windows_tensor_dev (no counterpart in the
 * reference: a setting of this library's context).  0, the default: exactly the launches made without this setting.  1: every file's own
 * tag is honoured -- a window is then in the coordinates of the file's ORIENTED picture, the whole-picture form {0,0,0,0} is the whole
 * oriented picture, `placed` reports oriented coordinates, and jpezy_window_fit / jpezy_resize_pick_window are to be given the oriented
 * size (jpezy_orient_size).  mirror_x of the resized and tensor calls acts after the orientation, unchanged.  Files whose orientation is 1
 * still run the un-oriented kernels: a mixed group is two launches per scale.  Any other mode, or a null context: JPEZY_E_BADARG, the
 * setting unchanged.  The getter returns the setting (JPEZY_E_BADARG for a null context). */
int jpezy_ctx_set_windows_orientation(jpezy_ctx* ctx, int mode);
int jpezy_ctx_windows_orientation(jpezy_ctx* ctx);
#endif
