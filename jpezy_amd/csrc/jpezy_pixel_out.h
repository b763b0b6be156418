// jpezy_pixel_out.h -- the pixel-output stage every any-layout decode kernel ends in: the reference's colour conversion and the store forms
// of a thread's four consecutive pixels of a row.  The decoders share it (generic, scaled, smooth, region / windows, resized); the fused quad
// kernel of jpezy_kernels_decode.hip has a tuned colour path and a 16-pixel store of its own and does not come through here.
#pragma once
#include "jpezy_wave.h"

namespace jpezy_dev {

// revise_value (ref decoder/jpezy_decoder.hpp:672-676)
__device__ __forceinline__ uint32_t revise(double v) { return (v < 0.0) ? 0u : (v > 255.0) ? 255u : (uint32_t)v; }
__device__ __forceinline__ int clamp8(int s) { return min(max(s, 0), 255); }

// make_rgb (ref :531-578) in the reference's FP64 order, left to right: the library is built without contraction, and nothing here may be
// reassociated.  y, u, v: the integer samples of the pixel (a missing component: 0 / 0x80, ref :104-105).
__device__ __forceinline__ void make_rgb(bool gray, int y, int u, int v, uint32_t& r, uint32_t& g, uint32_t& b)
{
    const double yp = y, up = u, vp = v;
    if (!gray) {
        r = revise(yp + (vp - 0x80) * 1.4020);
        g = revise(yp - (up - 0x80) * 0.3441 - (vp - 0x80) * 0.7139);
        b = revise(yp + (up - 0x80) * 1.7718);
    } else {
        r = g = b = revise(yp);
    }
}

// Packed (interleaved) pixels of PIX = 3 or 4 bytes: byte j of w0 / w1 / w2 is channel byte 0 / 1 / 2 of pixel j, px the first byte of pixel
// 0.  All four pixels and a 4-byte aligned px: one 12- or 16-byte store (byte 3 of a 32-bit pixel = 0xFF); single bytes otherwise.  Which of
// red and blue is byte 0 is the caller's to decide: it hands the words over in byte order.
template <int PIX>
__device__ __forceinline__ void store_packed4(uint8_t* px, unsigned npx, uint32_t w0, uint32_t w1, uint32_t w2)
{
    static_assert(PIX == 3 || PIX == 4, "packed pixels of 3 or 4 bytes");
    auto byte = [](uint32_t w, unsigned j) { return (w >> (8 * j)) & 0xFFu; };
    if (npx == 4 && ((uintptr_t)px & 3u) == 0) {
        if (PIX == 3) {
            typedef unsigned v3u __attribute__((ext_vector_type(3)));
            typedef v3u v3u_a4 __attribute__((aligned(4)));
            v3u v;
            v.x = byte(w0, 0) | byte(w1, 0) << 8 | byte(w2, 0) << 16 | byte(w0, 1) << 24;
            v.y = byte(w1, 1) | byte(w2, 1) << 8 | byte(w0, 2) << 16 | byte(w1, 2) << 24;
            v.z = byte(w2, 2) | byte(w0, 3) << 8 | byte(w1, 3) << 16 | byte(w2, 3) << 24;
            *reinterpret_cast<v3u_a4*>(px) = v;
        } else {
            typedef unsigned v4u __attribute__((ext_vector_type(4)));
            typedef v4u v4u_a4 __attribute__((aligned(4)));
            v4u v;
            v.x = byte(w0, 0) | byte(w1, 0) << 8 | byte(w2, 0) << 16 | 0xFF000000u;
            v.y = byte(w0, 1) | byte(w1, 1) << 8 | byte(w2, 1) << 16 | 0xFF000000u;
            v.z = byte(w0, 2) | byte(w1, 2) << 8 | byte(w2, 2) << 16 | 0xFF000000u;
            v.w = byte(w0, 3) | byte(w1, 3) << 8 | byte(w2, 3) << 16 | 0xFF000000u;
            *reinterpret_cast<v4u_a4*>(px) = v;
        }
    } else {
        for (unsigned j = 0; j < npx; ++j) {
            px[j * PIX] = (uint8_t)byte(w0, j); px[j * PIX + 1] = (uint8_t)byte(w1, j); px[j * PIX + 2] = (uint8_t)byte(w2, j);
            if (PIX == 4) px[j * PIX + 3] = 0xFF;
        }
    }
}

// Planes: byte j of rw / gw / bw is pixel j's, stored at r / g / b + off.  One word per plane when all four pixels exist and the caller's
// predicate word_ok says that the three addresses are multiples of 4 (each kernel keeps its own form of it); single bytes otherwise.
__device__ __forceinline__ void store_planes4(uint8_t* r, uint8_t* g, uint8_t* b, size_t off, unsigned npx, uint32_t rw, uint32_t gw, uint32_t bw,
                                              bool word_ok)
{
    if (npx == 4 && word_ok) {
        *reinterpret_cast<uint32_t*>(r + off) = rw;
        *reinterpret_cast<uint32_t*>(g + off) = gw;
        *reinterpret_cast<uint32_t*>(b + off) = bw;
    } else {
        for (unsigned j = 0; j < npx; ++j) {
            r[off + j] = (uint8_t)(rw >> (8 * j)); g[off + j] = (uint8_t)(gw >> (8 * j)); b[off + j] = (uint8_t)(bw >> (8 * j));
        }
    }
}

// the address form of word_ok: rows and frames may be any number of bytes apart
__device__ __forceinline__ bool planes_word_aligned(const uint8_t* r, const uint8_t* g, const uint8_t* b, size_t off)
{
    return ((((uintptr_t)(r + off)) | ((uintptr_t)(g + off)) | ((uintptr_t)(b + off))) & 3u) == 0;
}

}  // namespace jpezy_dev
