// jpezy_kernels_resized.hip -- a batch of windows, resized: the second stage behind windows_kernel / region_kernel.  The packed pixels of
// MANY windows of different sizes, each brought to the launch's out_w x out_h by the separable triangle filter of include/jpezy_hip.h,
// BATCH OF WINDOWS, RESIZED, in 32-bit integer fixed point.
//   resample_kernel<PIX> : one workgroup = one tile of kResampleTileW x kResampleTileH output pixels of one file; the grid is 1-D over the
//       sum of the files' tiles.  A workgroup finds its file by windows_kernel's binary search over the files' first-workgroup indices
//       (ResampleDesc::wg0): the index and every descriptor field depend on blockIdx alone, so they are wave-uniform and live in scalar
//       registers.  A thread owns four consecutive OUTPUT pixels of a row.  For each of them it walks the column's vertical taps, and
//       for every such source row evaluates the horizontal pass at that column (the byte t of the definition: (2^21 + sum K * src) >> 22,
//       clipped), then accumulates K * t: the vertical pass over exactly the bytes a separate horizontal pass would have stored.  Both
//       tap loops are runtime loops over the tables' counts, so every ratio runs the same code and nothing is staged in LDS: a source of
//       4096 columns to one pixel is a loop of 8192 taps, not a tile that has to fit.  The price is that a horizontal byte is evaluated
//       once per output row that uses it (about twice when an axis shrinks, DESIGN.md 4.15 has the count).  All of that is
//       resample_four of jpezy_resample_core.h, which the tensor form of this stage (jpezy_kernels_resized_tensor.hip) runs too.
//       Stores: the four pixels as one 12- or 16-byte store when all four exist and the address is a multiple of 4, single bytes
//       otherwise (windows_kernel's stage 2).  Byte 3 of a 32-bit pixel is 0xFF and is never read.
//   resample_kernel<PIX, true> : the instance of the filters wider than the triangle (box, bicubic, Lanczos).  A file
//       whose descriptor says `tiled` runs resample_four_tiled: the horizontal pass once per source row of the tile into
//       kResampleTileRows x 48 words of static LDS, one barrier, the vertical pass out of LDS (jpezy_resample_core.h has the layout and
//       its bank arithmetic).  Every other file of the launch runs resample_four as above: the flag is the descriptor's, so the branch
//       is wave-uniform.  resample_kernel<PIX, false> is the kernel above, without LDS; the triangle filter launches it alone.
// No byte outside a file's out_w * PIX x out_h rectangle is written; the source is read inside the file's w x h window only (the tables
// hold first + count <= size, jpezy_resize_taps).
#include "jpezy_resample_core.h"
#include "jpezy_pixel_out.h"

namespace jpezy_dev {
namespace resized {

template <int PIX, bool TILE>
__global__ __launch_bounds__(kThreads) void resample_kernel(ResampleParams p)
{
    const ResampleDesc d = workgroup_file(p);
    int ox0, oy, npx;
    uint32_t w0, w1, w2;                          // byte j of w0 / w1 / w2: channel byte 0 / 1 / 2 of pixel j
    if constexpr (TILE) {
        __shared__ uint32_t tile[kTileWords];
        if (!(d.tiled ? resample_four_tiled<PIX>(p, d, tile, ox0, oy, npx, w0, w1, w2) : resample_four<PIX>(p, d, ox0, oy, npx, w0, w1, w2))) return;
    } else {
        if (!resample_four<PIX>(p, d, ox0, oy, npx, w0, w1, w2)) return;
    }

    uint8_t* px = p.dst + d.dst_off + (size_t)oy * p.dst_stride + (size_t)ox0 * PIX;
    store_packed4<PIX>(px, (unsigned)npx, w0, w1, w2);
}

}  // namespace resized

// total_wg: the workgroups of the call, desc[k].wg0 counted from 0.  A launch takes at most 2^24 - 1 of them (launch_dequant_idct_windows'
// rule: its global size stays below 2^32), larger calls go out as several launches that start at wg_base.
hipError_t launch_resample(const ResampleParams& p, unsigned long long total_wg, hipStream_t s, bool tile)
{
    if ((p.pix_bytes != 3 && p.pix_bytes != 4) || p.n_desc < 1 || total_wg < 1 || total_wg > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (p.out_w < 1 || p.out_h < 1 || p.out_w > 65535 || p.out_h > 65535 || (p.src_stride & 3u)) return hipErrorInvalidValue;
    constexpr unsigned long long per = (1ull << 24) - 1;
    for (unsigned long long w0 = 0; w0 < total_wg; w0 += per) {
        ResampleParams q = p;
        q.wg_base = (unsigned)w0;
        const unsigned n_wg = (unsigned)(total_wg - w0 < per ? total_wg - w0 : per);
        if (q.pix_bytes == 3 && tile) hipLaunchKernelGGL((resized::resample_kernel<3, true>), dim3(n_wg), dim3(resized::kThreads), 0, s, q);
        else if (q.pix_bytes == 3) hipLaunchKernelGGL((resized::resample_kernel<3, false>), dim3(n_wg), dim3(resized::kThreads), 0, s, q);
        else if (tile) hipLaunchKernelGGL((resized::resample_kernel<4, true>), dim3(n_wg), dim3(resized::kThreads), 0, s, q);
        else hipLaunchKernelGGL((resized::resample_kernel<4, false>), dim3(n_wg), dim3(resized::kThreads), 0, s, q);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace jpezy_dev
