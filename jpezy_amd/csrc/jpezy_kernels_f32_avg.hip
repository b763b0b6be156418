// jpezy_kernels_f32_avg.hip -- encode variant 1 with JPEZY_DOWNSAMPLE_AVERAGE: the one-quad kernels of jpezy_f32_onequad.h instantiated
// with the averaged chroma stage (jpezy_f32_quad.h, step 2b, AVG), colour 4:2:0 RGB input only, planar and packed.  A file of its own
// so that jpezy_kernels_f32.hip compiles what it compiled before: the default (point-sampling) instances carry no trace of the mode.
// The launchers choose the workgroup shapes as launch_fdct_quant_f32 / launch_fdct_quant_f32_packed do; the test hooks' instances
// (force 1..3) exist in the two-wave byte-loop form only, as the 4:4:4 kernel's do.
#include "jpezy_f32_onequad.h"

namespace jpezy_dev {

namespace {

// EW, ALIGNED: workgroup shape and load form; PIX: 0 planes, 3 / 4 packed pixels
template <bool ALIGNED, int FORCE, int EW, int PIX>
void avg_launch(const EncParams& p, dim3 grid, hipStream_t s)
{
    const bool dcg = p.dc_rq[0] != 0.f && p.dc_rq[1] != 0.f;            // as enc_f32_launch2
    if constexpr (PIX == 0) {
        if (dcg) hipLaunchKernelGGL((f32::fdct_quant_f32_kernel<false, ALIGNED, FORCE, EW, true, true>), grid, dim3(64 * EW), 0, s, p);
        else hipLaunchKernelGGL((f32::fdct_quant_f32_kernel<false, ALIGNED, FORCE, EW, false, true>), grid, dim3(64 * EW), 0, s, p);
    } else {
        if (dcg) hipLaunchKernelGGL((f32::fdct_quant_f32_packed_kernel<false, ALIGNED, FORCE, EW, true, PIX, true>), grid, dim3(64 * EW), 0, s, p);
        else hipLaunchKernelGGL((f32::fdct_quant_f32_packed_kernel<false, ALIGNED, FORCE, EW, false, PIX, true>), grid, dim3(64 * EW), 0, s, p);
    }
}

template <int PIX>
hipError_t avg_launch_shape(const EncParams& p0, bool al, int force, hipStream_t stream)
{
    EncParams p = p0;
    const int ew = (al && p.quads_per_row % 4 == 0 && force == 0) ? 4 : 2;
    p.groups_per_row = (p.quads_per_row + ew - 1) / ew;
    const long groups = (long)p.mcu_rows * p.groups_per_row;
    if (groups <= 0 || p.n_frames <= 0) return hipSuccess;
    if (p.n_frames > 65535) return hipErrorInvalidValue;               // grid.y limit; callers chunk larger batches
    fast_div_setup((unsigned)p.groups_per_row, &p.gpr_magic, &p.gpr_shift);
    const dim3 grid((unsigned)groups, (unsigned)p.n_frames);
    if (force == 1) avg_launch<false, 1, 2, PIX>(p, grid, stream);
    else if (force == 2) avg_launch<false, 2, 2, PIX>(p, grid, stream);
    else if (force == 3) avg_launch<false, 3, 2, PIX>(p, grid, stream);
    else if (ew == 4) avg_launch<true, 0, 4, PIX>(p, grid, stream);
    else if (al) avg_launch<true, 0, 2, PIX>(p, grid, stream);
    else avg_launch<false, 0, 2, PIX>(p, grid, stream);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fdct_quant_f32_avg(const EncParams& p, int force, hipStream_t stream)
{
    const bool al = (p.W % 16 == 0) && (p.plane_stride % 16 == 0) && (((uintptr_t)p.r | (uintptr_t)p.g | (uintptr_t)p.b) % 16 == 0);
    return avg_launch_shape<0>(p, al, force, stream);
}

hipError_t launch_fdct_quant_f32_packed_avg(const EncParams& p, int force, hipStream_t stream)
{
    if (p.pix_bytes != 3 && p.pix_bytes != 4) return hipErrorInvalidValue;
    const bool al = packed_is_aligned16(p.pix, p.W, p.row_stride, p.plane_stride);
    return p.pix_bytes == 3 ? avg_launch_shape<3>(p, al, force, stream) : avg_launch_shape<4>(p, al, force, stream);
}

}  // namespace jpezy_dev
