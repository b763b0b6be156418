// jpezy_tran <input.(jpg | jpeg)> <output.(jpg | jpeg)> (--rotate=(90 | 180 | 270) | --flip=(h | v) | --transpose | --transverse | --none |
//            --auto-orient) [OPT: --trim] [OPT: --optimize] [OPT: --restart=N]
// This project's own tool (the reference has none): a lossless transform of a .jpg in the coefficient domain through jpezy_transform_jpeg
// (include/jpezy_hip.h, LOSSLESS TRANSFORMS) -- what jpegtran -rotate / -flip / -transpose / -transverse do.  Exactly one operation;
// --none re-codes the file as it is (with --optimize: per-image Huffman tables; --restart=N: restart intervals of N MCUs, 0..65535).
// --auto-orient is the operation whose effect on the pixels is the one the input's EXIF orientation asks for (jpezy_jpeg_orientation;
// include/jpezy_hip_orientation.h): the output is upright, and untagged since no APPn segment is carried.  The partial-MCU rule applies to
// it as to the operation it picks.
// --trim drops the partial MCU column / row of a mirrored axis; without it such a file is refused with the library's message.
// Exit codes and messages as the other two CLIs: a usage error prints the usage line and exits 1 before anything is loaded; a file the
// library refuses prints its reason and exits 1, and no output file is written.
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string_view>
#include <vector>

#include "jpezy.hpp"

namespace {

int disp_error()
{
    std::cerr << "Usage: jpezy_tran <input.(jpg | jpeg)> <output.(jpg | jpeg)> (--rotate=(90 | 180 | 270) | --flip=(h | v) | --transpose | --transverse | --none | --auto-orient)"
                 " [OPT: --trim] [OPT: --optimize] [OPT: --restart=N]"
              << std::endl;
    return EXIT_FAILURE;
}

bool has_ext(std::string_view s, std::string_view ext)
{
    return s.find(ext, s.find_first_of('.')) != std::string_view::npos;
}

// --auto-orient as a value of op_of: resolved once the file is read
constexpr int kAutoOrient = 100;

// the operation that turns a picture tagged `orientation` upright: orient(P, o) of include/jpezy_hip_orientation.h's table, held against
// LOSSLESS TRANSFORMS' own table of source pixels (not against the names)
int op_for_orientation(int orientation)
{
    constexpr int ops[8] = { JPEZY_XFORM_NONE, JPEZY_XFORM_HFLIP, JPEZY_XFORM_ROT180, JPEZY_XFORM_VFLIP, JPEZY_XFORM_TRANSPOSE, JPEZY_XFORM_ROT90,
                             JPEZY_XFORM_TRANSVERSE, JPEZY_XFORM_ROT270 };
    return ops[orientation - 1];
}

// the operation an option names (JPEZY_XFORM_*, kAutoOrient), -1 when it names none, -2 when it is one with a bad value
int op_of(std::string_view sv)
{
    if (sv == "--none") return JPEZY_XFORM_NONE;
    if (sv == "--auto-orient") return kAutoOrient;
    if (sv == "--transpose") return JPEZY_XFORM_TRANSPOSE;
    if (sv == "--transverse") return JPEZY_XFORM_TRANSVERSE;
    if (sv.substr(0, 9) == "--rotate=") {
        const std::string_view n = sv.substr(9);
        return n == "90" ? JPEZY_XFORM_ROT90 : n == "180" ? JPEZY_XFORM_ROT180 : n == "270" ? JPEZY_XFORM_ROT270 : -2;
    }
    if (sv.substr(0, 7) == "--flip=") {
        const std::string_view n = sv.substr(7);
        return n == "h" ? JPEZY_XFORM_HFLIP : n == "v" ? JPEZY_XFORM_VFLIP : -2;
    }
    return -1;
}

// --restart=N: N in 0..65535, -1 for anything else
int restart_of(std::string_view n)
{
    long v = 0;
    if (n.empty() || n.size() > 5) return -1;
    for (const char ch : n) {
        if (ch < '0' || ch > '9') return -1;
        v = v * 10 + (ch - '0');
    }
    return v <= 65535 ? static_cast<int>(v) : -1;
}

int run(const char* in, const char* out, int op, int flags, bool optimize, int restart)
{
    jpezy::disp_logo();
    std::ifstream ifs(in, std::ios::binary);
    if (!ifs.is_open()) {
        std::cerr << "input_file" << std::endl;
        return EXIT_FAILURE;
    }
    const std::vector<std::uint8_t> data((std::istreambuf_iterator<char>(ifs)), std::istreambuf_iterator<char>());
    if (op == kAutoOrient) op = op_for_orientation(jpezy_jpeg_orientation(data.data(), data.size()));
    jpezy_ctx* ctx = jpezy::detail::device_context();
    auto fail = [] {
        std::cerr << "transform failed: " << jpezy_hip_last_error() << std::endl;
        return EXIT_FAILURE;
    };
    if (jpezy_ctx_set_huffman_optimize(ctx, optimize ? 1 : 0) != JPEZY_OK || jpezy_ctx_set_restart_interval(ctx, restart) != JPEZY_OK) return fail();
    jpezy_frame_info info;
    if (jpezy_transform_jpeg(ctx, data.data(), data.size(), op, flags, nullptr, &info, nullptr, 0) < 0) return fail();
    const int sampling = info.H[0] == 1 ? JPEZY_SAMPLING_444 : JPEZY_SAMPLING_420;
    std::vector<std::uint8_t> jpg(jpezy_jpeg_bound_sampling(info.width, info.height, sampling));
    const long n = jpezy_transform_jpeg(ctx, data.data(), data.size(), op, flags, nullptr, &info, jpg.data(), jpg.size());
    if (n < 0) return fail();
    std::ofstream ofs(out, std::ios::binary | std::ios::trunc);
    ofs.write(reinterpret_cast<const char*>(jpg.data()), static_cast<std::streamsize>(n));
    if (!ofs) {
        std::cerr << "output_file" << std::endl;
        return EXIT_FAILURE;
    }
    std::cout << "Transformed image: JPEG image data, size = " << info.width << " x " << info.height << ", " << n << " bytes" << std::endl;
    return EXIT_SUCCESS;
}

}  // namespace

int main(const int argc, const char* argv[])
{
    if (argc < 4 || argc > 7) return disp_error();
    const std::string_view in = argv[1], out = argv[2];
    if (!((has_ext(in, "jpeg") || has_ext(in, "jpg")) && (has_ext(out, "jpeg") || has_ext(out, "jpg")))) return disp_error();

    int op = -1, flags = 0, restart = 0;
    bool optimize = false, has_restart = false;
    for (int k = 3; k < argc; ++k) {
        const std::string_view sv = argv[k];
        const int o = op_of(sv);
        if (o == -2 || (o >= 0 && op >= 0)) return disp_error();      // a bad value, or a second operation
        if (o >= 0) { op = o; continue; }
        if (sv == "--trim" && !(flags & JPEZY_XFORM_TRIM)) { flags |= JPEZY_XFORM_TRIM; continue; }
        if (sv == "--optimize" && !optimize) { optimize = true; continue; }
        if (sv.substr(0, 10) == "--restart=" && !has_restart) {
            restart = restart_of(sv.substr(10));
            if (restart < 0) return disp_error();
            has_restart = true;
            continue;
        }
        return disp_error();
    }
    if (op < 0) return disp_error();
    try {
        return run(argv[1], argv[2], op, flags, optimize, restart);
    } catch (const std::runtime_error& e) {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }
}
