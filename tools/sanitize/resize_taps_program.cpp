// A stand-alone program (its own main) over jpezy_amd/csrc/jpezy_resize_taps.h -- the tap tables of the resized batch of windows for the four
// filters of enum jpezy_filter -- for a sanitizer run on the CPU:
//
//     clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -I jpezy_amd/csrc \
//         tools/sanitize/resize_taps_program.cpp -o /tmp/resize_taps && /tmp/resize_taps      # "N checks, 0 wrong" and no sanitizer report
//
// The sizes are the sweep of tests/test_resize_filters_abi.py (growing, equal, shrinking, 65535 -> 65535, 65535 -> 100, 4096 -> 1, 1 -> 64).
// The tables are written into buffers of exactly out_size and out_size * ksize elements, so a write behind either is a report; the checks
// are the tables' invariants: first and first + count inside the source and never decreasing, count in 1..ksize, zeros behind count,
// weights that sum to 2^22 within count / 2 + 1, the accumulator condition, the identity at in == out, and a tile span that covers every
// output index of the tile.
#include "jpezy_resize_taps.h"

#include <cstdio>
#include <cstdlib>

using namespace jpezy_host;

static int checks = 0, wrong = 0;

static void expect(bool ok, const char* what, int filter, int in_size, int out_size)
{
    ++checks;
    if (!ok) { ++wrong; std::printf("WRONG: %s (filter %d, %d -> %d)\n", what, filter, in_size, out_size); }
}

int main()
{
    static const int sizes[][2] = { { 1, 1 }, { 1, 8 }, { 1, 64 }, { 8, 1 }, { 9, 3 }, { 16, 16 }, { 17, 24 }, { 17, 80 }, { 33, 70 }, { 40, 24 },
                                    { 63, 32 }, { 64, 64 }, { 70, 24 }, { 120, 7 }, { 120, 2 }, { 208, 3 }, { 208, 64 }, { 447, 224 }, { 777, 224 },
                                    { 4096, 1 }, { 65535, 100 }, { 65535, 1 }, { 100, 65535 }, { 65535, 65535 } };
    for (int filter = kFilterBilinear; filter <= kFilterLanczos; ++filter)
        for (const auto& sz : sizes) {
            const int in_size = sz[0], out_size = sz[1];
            const int ksize = resize_ksize(filter, in_size, out_size);
            int* const first = (int*)std::malloc(sizeof(int) * (size_t)out_size);
            int* const count = (int*)std::malloc(sizeof(int) * (size_t)out_size);
            int32_t* const weight = (int32_t*)std::malloc(sizeof(int32_t) * (size_t)out_size * (size_t)ksize);
            expect(resize_taps_into(filter, in_size, out_size, ksize, first, count, weight), "the accumulator condition", filter, in_size, out_size);
            bool inside = true, ordered = true, zeros = true, sums = true, identity = true;
            for (int i = 0; i < out_size; ++i) {
                inside = inside && first[i] >= 0 && count[i] >= 1 && count[i] <= ksize && first[i] + count[i] <= in_size;
                if (i) ordered = ordered && first[i] >= first[i - 1] && first[i] + count[i] >= first[i - 1] + count[i - 1];
                long long sum = 0;
                for (int j = 0; j < ksize; ++j) {
                    const int32_t k = weight[(size_t)i * (size_t)ksize + (size_t)j];
                    sum += k;
                    if (j >= count[i]) zeros = zeros && k == 0;
                    if (in_size == out_size) identity = identity && k == (first[i] + j == i && j < count[i] ? 1 << 22 : 0);
                }
                sums = sums && std::llabs(sum - (1ll << 22)) <= count[i] / 2 + 1;
            }
            expect(inside, "first and count inside the source", filter, in_size, out_size);
            expect(ordered, "first and first + count never decrease", filter, in_size, out_size);
            expect(zeros, "zeros behind count", filter, in_size, out_size);
            expect(sums, "the weights of an output sum to 2^22", filter, in_size, out_size);
            expect(identity, "identity weights", filter, in_size, out_size);
            const int span = resize_tile_span(first, count, out_size, 16);
            bool covered = span >= 1 && span <= in_size;
            for (int i = 0; i < out_size; ++i) covered = covered && first[i] + count[i] - first[i - i % 16] <= span;
            expect(covered, "the tile span covers every output index of its tile", filter, in_size, out_size);
            const ResizeTaps t = resize_taps(filter, in_size, out_size);
            bool same = t.ksize == ksize && t.fits;
            for (int i = 0; i < out_size && same; ++i) same = t.first[(size_t)i] == first[i] && t.count[(size_t)i] == count[i];
            for (size_t q = 0; q < (size_t)out_size * (size_t)ksize && same; ++q) same = t.weight[q] == weight[q];
            expect(same, "resize_taps equals resize_taps_into", filter, in_size, out_size);
            std::free(first);
            std::free(count);
            std::free(weight);
        }
    expect(!resize_filter_known(-1) && !resize_filter_known(4) && resize_filter_known(0) && resize_filter_known(3), "known filters", 0, 0, 0);
    std::printf("%d checks, %d wrong\n", checks, wrong);
    return wrong ? 1 : 0;
}
