// jpezy_wave.h -- the wave-level plumbing every kernel file shares.  No arithmetic of the codec: the decoders' colour and store stage is
// shared through jpezy_pixel_out.h; the transforms, colour formulas and tables of the two encoders are NOT shared (see jpezy_kernels_f64.hip
// on why).
#pragma once
#include "jpezy_device.h"

namespace jpezy_dev {

__device__ __forceinline__ unsigned fast_div(unsigned n, unsigned magic, unsigned shift)   // see fast_div_setup
{
    const unsigned q = __umulhi(n, magic);
    return magic ? (((n - q) >> 1) + q) >> shift : n;
}

// wave-uniform "some lane": one v_cmp into an SGPR pair + s_cmp (HIP's __any goes through a 0/1 VGPR)
__device__ __forceinline__ bool wave_any(bool x) { return __builtin_amdgcn_ballot_w64(x) != 0ull; }

__device__ __forceinline__ void wave_sync()
{
    // LDS traffic of one wave is executed in order; this only stops the compiler from moving LDS
    // accesses of different lanes across the phase boundary.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A 1-D grid over the workgroups of many files (WindowDesc, ResampleDesc): the file of workgroup wg is the last descriptor whose first
// workgroup is <= wg (wg0 ascending, desc[0].wg0 == first workgroup of the call).  The result depends on blockIdx alone; a kernel passes it
// through readfirstlane and then reads the descriptor with scalar loads.
template <class Desc>
__device__ __forceinline__ unsigned find_file(const Desc* __restrict__ desc, unsigned n, unsigned wg)
{
    unsigned lo = 0, hi = n;                      // invariant: desc[lo].wg0 <= wg, and (hi == n or desc[hi].wg0 > wg)
    while (hi - lo > 1) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (desc[mid].wg0 <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

// Outputs are streamed out and never re-read by the kernel: a non-temporal store leaves less dirty data in the eight
// L2s for the end-of-kernel write-back (measured on the f32 encode kernel: 2 us per 4096^2 frame).
__device__ __forceinline__ void nt_store16(uint4* dst, uint4 v)
{
    typedef unsigned v4u __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(v4u{v.x, v.y, v.z, v.w}, reinterpret_cast<v4u*>(dst));
}

// planes a launcher may hand to the 16-byte load / store instance of its kernel
template <typename P>
static bool is_aligned16(const P& p, const void* a, const void* b, const void* c)
{
    return (p.W % 16 == 0) && (p.plane_stride % 16 == 0) && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) % 16 == 0);
}

}  // namespace jpezy_dev
