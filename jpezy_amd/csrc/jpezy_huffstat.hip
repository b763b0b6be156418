// jpezy_huffstat.hip -- symbol statistics of a frame for per-image optimised Huffman tables ("optimised tables"):
// how often the coder (jpezy_entropy.hip, code_block) will emit every symbol of the four tables.  The counts go to the host, which
// builds the tables (jpezy_host::optimal_table, Annex K.2) the coder then runs with.
//
// One WAVE per block, one lane per zig-zag position -- not the coder's lane per block: the block arrives as one 128-byte row, the
// mask of its non-zero coefficients is a ballot, the run in front of a coefficient is the distance to the next set bit below its
// lane, and every non-zero coefficient is one LDS atomic -- there is no loop over the coefficients.  A workgroup (4 waves) counts
// HB consecutive stored blocks of one frame into its own LDS histogram (2 x (16 + 256) 32-bit bins) and flushes the non-zero bins
// with one 64-bit global atomic each; integer sums do not depend on the order of arrival.
// Gray frames code two zero chroma blocks per MCU (DC category 0 and EOB each, predictor 0): they are not walked, workgroup 0 of the
// frame adds 2 * MCUs to those two bins.
// Restart intervals (Job::restart != 0, the RST instance): the predictors of an interval's first MCU are zero, as the coder has them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpezy_entropy.h"

namespace jpezy_dev {
namespace entropy {

constexpr int HWG = 256;            // threads of a workgroup: 4 waves
constexpr unsigned HB = 1024;       // stored blocks per workgroup: 4096 x 4096 -> 384 workgroups, 544 x 384 flushes at the most
constexpr int HBATCH = 4;           // blocks a wave requests before it counts the first of them

struct LdsHist {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
static_assert((unsigned long long)HB * 64ull < (1ull << 32), "a workgroup's bin cannot overflow 32 bits");

// CODED / LUMA: the MCU as a layout (Job::coded, Job::luma; jpezy_entropy.h) -- 6 / 4 for 4:2:0 (gray: 4 of the 6 stored), 3 / 1 for 4:4:4,
// 4 / 2 for 4:2:2
template <bool RST, unsigned CODED = 6u, unsigned LUMA = 4u>
__global__ __launch_bounds__(HWG) void symbol_histogram_kernel(Job job, unsigned long long* hist, unsigned* status)
{
    __shared__ LdsHist L;
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, frame = blockIdx.y;
    uint32_t* const bins = &L.dc[0][0];
    constexpr unsigned NBINS = sizeof(LdsHist) / 4;
    for (unsigned i = tid; i < NBINS; i += HWG) bins[i] = 0;
    __syncthreads();

    const unsigned bpm = (unsigned)job.bpm;
    const unsigned nstored = job.blocks_per_frame / CODED * bpm;                   // blocks the frame holds in memory
    const int16_t* fc = job.coeffs + (size_t)frame * job.coeffs_per_frame;
    const unsigned w0 = blockIdx.x * HB + wave * (HB / 4);                         // this wave's blocks: [w0, w1)
    const unsigned w1 = w0 + HB / 4 < nstored ? w0 + HB / 4 : nstored;
    bool bad = false;
    for (unsigned b0 = w0; b0 < w1; b0 += HBATCH) {
        int v[HBATCH], pred[HBATCH];
#pragma unroll
        for (int j = 0; j < HBATCH; ++j) {
            const unsigned sb = b0 + j;
            v[j] = 0;
            pred[j] = 0;
            if (sb < w1) {                                                         // (wave-uniform)
                const int16_t* z = fc + (size_t)sb * 64;
                v[j] = z[lane];
                // lane 0: the DC predictor as code_tiles_kernel reads it -- the previous block of the component, 0 for the frame's first
                const unsigned mcu = sb / bpm, i = sb - mcu * bpm;
                if (lane == 0) {
                    if (i >= 1 && i < LUMA) pred[j] = z[-64];
                    else if (mcu != 0 && !(RST && mcu % job.restart == 0u)) pred[j] = i == 0 ? z[-(int)(bpm - (LUMA - 1u)) * 64] : z[-(int)bpm * 64];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < HBATCH; ++j) {
            const unsigned sb = b0 + j;
            if (sb >= w1) break;
            const unsigned i = sb % bpm, t = i < LUMA ? 0u : 1u;
            const unsigned long long nz = __builtin_amdgcn_ballot_w64(v[j] != 0) & ~1ull;      // bit n: AC position n is non-zero
            if (lane == 0) {
                const int diff = v[j] - pred[j];
                const unsigned a = (unsigned)(diff < 0 ? -diff : diff);
                unsigned di = a ? 32u - (unsigned)__builtin_clz(a) : 0u;
                if (di > 11u) { bad = true; di = 11u; }
                atomicAdd(&L.dc[t][di], 1u);
            } else if (v[j] != 0) {
                const unsigned long long below = nz & ((1ull << lane) - 1ull);
                const unsigned prev = below ? 63u - (unsigned)__builtin_clzll(below) : 0u;     // 0: the DC
                const unsigned run = lane - prev - 1u;
                const unsigned a = (unsigned)(v[j] < 0 ? -v[j] : v[j]);
                unsigned sz = 32u - (unsigned)__builtin_clz(a);
                if (sz > 10u) { bad = true; sz = 10u; }
                atomicAdd(&L.ac[t][((run & 15u) << 4) | sz], 1u);
                if (run > 15u) atomicAdd(&L.ac[t][0xF0], run >> 4);                            // ZRL codes in front of it
            } else if (lane == 63u) {
                atomicAdd(&L.ac[t][0x00], 1u);                                                 // the block ends in zeros: EOB
            }
        }
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) atomicOr(status + frame, 1u);
    __syncthreads();

    unsigned long long* const H = hist + (size_t)frame * 4 * 256;
    for (unsigned i = tid; i < NBINS; i += HWG) {
        unsigned long long c = bins[i];
        // bins[0..32): dc[t][cat] -> table t; bins[32..544): ac[t][sym] -> table 2 + t
        const unsigned k = i < 32u ? i >> 4 : 2u + ((i - 32u) >> 8), sym = i < 32u ? i & 15u : (i - 32u) & 255u;
        if (CODED == 6u && bpm == 4u && blockIdx.x == 0 && sym == 0u && (k == 1u || k == 3u)) c += 2ull * (job.blocks_per_frame / 6u);
        if (c) atomicAdd(H + k * 256u + sym, c);
    }
}

// The counters are zeroed by a kernel, not by hipMemsetAsync: a memset node of a captured graph writes its value on the graph's first
// launch only and stale bytes on every later one (seen with a bare hipMemsetAsync in a graph of one node), which made a captured
// jpezy_huffman_histogram_dev right once and wrong on every replay (tests/test_gpu_streams.py, test_capture_replay[histogram]).
__global__ __launch_bounds__(HWG) void zero_histogram_kernel(unsigned long long* hist, size_t n)
{
    const size_t i = (size_t)blockIdx.x * HWG + threadIdx.x;
    if (i < n) hist[i] = 0;
}

hipError_t launch_zero_histogram(unsigned long long* hist, int n_frames, hipStream_t s)
{
    if (n_frames <= 0) return hipSuccess;
    const size_t n = (size_t)n_frames * 4 * 256;                // at most 65535 frames a launch: 2^18 workgroups
    hipLaunchKernelGGL(zero_histogram_kernel, dim3((unsigned)((n + HWG - 1) / HWG)), dim3(HWG), 0, s, hist, n);
    return hipGetLastError();
}

hipError_t launch_symbol_histogram(const Job& job, unsigned long long* hist, unsigned* status, hipStream_t s)
{
    if (!job.blocks_per_frame || job.n_frames <= 0) return hipSuccess;
    if (job.n_frames > 65535 || !layout_ok(job) || job.blocks_per_frame % (unsigned)job.coded) return hipErrorInvalidValue;
    const unsigned nstored = job.blocks_per_frame / (unsigned)job.coded * (unsigned)job.bpm;
    const dim3 grid((nstored + HB - 1) / HB, (unsigned)job.n_frames);
    if (job.coded == 3) {
        if (job.restart) hipLaunchKernelGGL((symbol_histogram_kernel<true, 3u, 1u>), grid, dim3(HWG), 0, s, job, hist, status);
        else hipLaunchKernelGGL((symbol_histogram_kernel<false, 3u, 1u>), grid, dim3(HWG), 0, s, job, hist, status);
    } else if (job.coded == 4) {
        if (job.restart) hipLaunchKernelGGL((symbol_histogram_kernel<true, 4u, 2u>), grid, dim3(HWG), 0, s, job, hist, status);
        else hipLaunchKernelGGL((symbol_histogram_kernel<false, 4u, 2u>), grid, dim3(HWG), 0, s, job, hist, status);
    } else if (job.restart)
        hipLaunchKernelGGL(symbol_histogram_kernel<true>, grid, dim3(HWG), 0, s, job, hist, status);
    else
        hipLaunchKernelGGL(symbol_histogram_kernel<false>, grid, dim3(HWG), 0, s, job, hist, status);
    return hipGetLastError();
}

}  // namespace entropy
}  // namespace jpezy_dev
