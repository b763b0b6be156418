// jpezy_decode <input.(jpg | jpeg)> ( <output.ppm | [OPT: --gray]> | -v ) [--scale=N] [--region=WxH+X+Y] [--orient] [--upsampling=smooth|nearest]
// Same argv rules, transcript and exit codes as the reference's src/decoder/main.cpp.  --scale=N (N = 1, 2, 4, 8; this project's own
// option, looked for in argv[3] .. argv[5] the way --gray is) writes the picture at 1/N; any other N is the usage error.
// --region=WxH+X+Y (this project's own option, X11 geometry order, looked for in the same places) writes the W x H window whose top-left
// pixel is (X, Y) of the picture at 1/N (jpezy_decode_jpeg_region); a malformed geometry is the usage error, a well-formed one that does
// not lie inside the picture prints the library's message and writes no file.
// --upsampling=smooth (this project's own option, looked for in the same places) brings 2:1 chroma to picture size with the triangle
// filter (jpezy_decode_jpeg_upsampling; include/jpezy_hip.h, CHROMA UPSAMPLING); --upsampling=nearest is the default, replication.  Any
// other value is the usage error; smooth together with --scale= other than 1 or with --region= prints one rule line and writes no file.
// --orient (this project's own option, looked for in the same places) applies the file's EXIF orientation (jpezy_decode_jpeg_oriented;
// include/jpezy_hip_orientation.h): the picture is written upright, --scale= and --region= then speak of the oriented picture, and
// --upsampling=smooth composes with it as far as it composes with those.  Any other word that begins with --orient is the usage error.
// jpezy_decode --i420 <input.(jpg | jpeg)> <output.yuv>   (this project's own option) writes the file's own samples, without upsampling
// or colour conversion, as raw planes: Y, then Cb, then Cr (full range: ffmpeg's yuvj420p) through jpezy_decode_jpeg_ycc.  Only a
// 4:2:0 file (sampling 2x2, 1x1, 1x1) is such a picture: any other layout is refused with a message.
// jpezy_decode --yuy2 | --uyvy <input.(jpg | jpeg)> <output.yuv>   (this project's own option) writes a file of any layout as packed
// YCbCr 4:2:2 macropixels, tight rows (full range: ffmpeg's rawvideo yuyv422 / uyvy422) through jpezy_decode_jpeg_yuv422
// (include/jpezy_hip_ycc422.h).  Exactly these four arguments: --gray, --scale=, --region=, --upsampling=, --orient are usage errors.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <cstdint>
#include <iterator>
#include <string_view>
#include <vector>

#include "decode_io.hpp"
#include "jpezy_decoder.hpp"

namespace {

int disp_error()
{
    std::cerr << "Usage: jpezy_decode <input.(jpg | jpeg)> ( <output.ppm | [OPT: --gray]> | -v ) [OPT: --scale=(1 | 2 | 4 | 8)] [OPT: --region=WxH+X+Y]"
                 " [OPT: --orient] [OPT: --upsampling=(smooth | nearest)]"
              << std::endl;
    return EXIT_FAILURE;
}

bool has_ext(std::string_view s, std::string_view ext)
{
    return s.find(ext, s.find_first_of('.')) != std::string_view::npos;
}

template <class CL, class T>
int output(jpezy::decoder<T>& dec, const char* out, int scale, const jpezy_rect* region, int upsampling, bool orient)
{
    auto raw_op = region ? dec.template decode<CL>(scale, *region, orient) : dec.template decode<CL>(scale, upsampling, orient);
    if (!raw_op) {
        std::cerr << "decode failed" << std::endl;
        return EXIT_FAILURE;
    }
    const auto raw = std::move(raw_op.value());
    const auto& [r, g, b] = raw;
    jpezy::decode_io dec_io(dec.out_width, dec.out_height, r, g, b);
    std::ofstream ofs(out, std::ios_base::out | std::ios_base::trunc);
    ofs << dec_io;
    std::cout << "Decoded image: Netpbm image data, size = " << dec.out_width << " x " << dec.out_height << ", pixmap, ASCII text"
              << std::endl;
    return EXIT_SUCCESS;
}

template <class T>
int run(const char* in, const char* out, bool gray, int scale, const jpezy_rect* region, int upsampling, bool orient)
{
    jpezy::disp_logo();
    jpezy::decoder<T> dec(in);
    return gray ? output<jpezy::GRAY_MODE>(dec, out, scale, region, upsampling, orient)
                : output<jpezy::COLOR_MODE>(dec, out, scale, region, upsampling, orient);
}

// the one rule of --upsampling=smooth: whole pictures at full size as P3 files
int upsampling_rule()
{
    std::cerr << "jpezy_decode: --upsampling=smooth writes whole pictures at full size: it does not combine with --scale= other than 1, --region= or --i420"
              << std::endl;
    return EXIT_FAILURE;
}

// --upsampling=V inside an option: JPEZY_UPSAMPLE_SMOOTH / _NEAREST for smooth / nearest, -2 for anything else, -1 when the option is
// not there
int upsampling_of(std::string_view opt)
{
    constexpr std::string_view key = "--upsampling=";
    const auto at = opt.find(key);
    if (at == std::string_view::npos) return -1;
    const std::string_view v = opt.substr(at + key.size());
    return v == "smooth" ? JPEZY_UPSAMPLE_SMOOTH : v == "nearest" ? JPEZY_UPSAMPLE_NEAREST : -2;
}

// --scale=N inside an option: N when it is 1, 2, 4 or 8, 0 for anything else, 1 when the option is not there
int scale_of(std::string_view opt)
{
    constexpr std::string_view key = "--scale=";
    const auto at = opt.find(key);
    if (at == std::string_view::npos) return 1;
    const std::string_view n = opt.substr(at + key.size());
    return n == "1" ? 1 : n == "2" ? 2 : n == "4" ? 4 : n == "8" ? 8 : 0;
}

// --region=WxH+X+Y inside an option: 1 and *r when it is well formed (decimal numbers, W, H >= 1), 0 when it is not, -1 when the option
// is not there
int region_of(std::string_view opt, jpezy_rect* r)
{
    constexpr std::string_view key = "--region=";
    const auto at = opt.find(key);
    if (at == std::string_view::npos) return -1;
    std::string_view g = opt.substr(at + key.size());
    int val[4];                                        // W, H, X, Y
    constexpr char sep[4] = { 'x', '+', '+', '\0' };   // what follows each number
    for (int k = 0; k < 4; ++k) {
        std::size_t n = 0;
        long v = 0;
        while (n < g.size() && g[n] >= '0' && g[n] <= '9' && n < 9) v = v * 10 + (g[n++] - '0');
        if (!n) return 0;
        val[k] = static_cast<int>(v);
        g.remove_prefix(n);
        if (sep[k] ? (g.empty() || g[0] != sep[k]) : !g.empty()) return 0;
        if (sep[k]) g.remove_prefix(1);
    }
    if (val[0] < 1 || val[1] < 1) return 0;
    *r = jpezy_rect{ val[2], val[3], val[0], val[1] };
    return 1;
}

int i420_main(const int argc, const char* argv[])
{
    if (argc != 4) {
        std::cerr << "Usage: jpezy_decode --i420 <input.(jpg | jpeg)> <output.yuv>" << std::endl;
        return EXIT_FAILURE;
    }
    jpezy::disp_logo();
    std::ifstream ifs(argv[2], std::ios::binary);
    const std::vector<std::uint8_t> data((std::istreambuf_iterator<char>(ifs)), std::istreambuf_iterator<char>());
    jpezy_ctx* ctx = jpezy::detail::device_context();
    jpezy_frame_info info;
    if (!ifs.is_open() || jpezy_decode_jpeg_ycc(ctx, data.data(), data.size(), &info, nullptr, 0, 0, nullptr, nullptr, 0, 1, 0) != JPEZY_OK) {
        std::cerr << "decode failed" << std::endl;
        return EXIT_FAILURE;
    }
    const bool is420 = info.ncomp == 3 && info.H[0] == 2 && info.V[0] == 2 && info.H[1] == 1 && info.V[1] == 1 && info.H[2] == 1 && info.V[2] == 1;
    if (!is420) {
        std::cerr << "jpezy_decode --i420: " << argv[2] << " is not a 4:2:0 file (its sampling is not 2x2, 1x1, 1x1)" << std::endl;
        return EXIT_FAILURE;
    }
    int CW = 0, CH = 0;
    jpezy_ycc_chroma_size(info.width, info.height, &CW, &CH);
    const std::size_t ny = static_cast<std::size_t>(info.width) * info.height, nc = static_cast<std::size_t>(CW) * CH;
    std::vector<std::uint8_t> out(ny + 2 * nc);
    if (jpezy_decode_jpeg_ycc(ctx, data.data(), data.size(), &info, out.data(), 0, ny, out.data() + ny, out.data() + ny + nc, 0, 1, nc) != JPEZY_OK) {
        std::cerr << "decode failed: " << jpezy_hip_last_error() << std::endl;
        return EXIT_FAILURE;
    }
    std::ofstream ofs(argv[3], std::ios::binary | std::ios::trunc);
    ofs.write(reinterpret_cast<const char*>(out.data()), static_cast<std::streamsize>(out.size()));
    if (!ofs) { std::cerr << "output_file" << std::endl; return EXIT_FAILURE; }
    std::cout << "Decoded image: raw planar YCbCr 4:2:0 (Y, Cb, Cr), size = " << info.width << " x " << info.height << std::endl;
    return EXIT_SUCCESS;
}

// jpezy_decode --yuy2 | --uyvy in.jpg out.yuv: a file of any layout as packed YCbCr 4:2:2 macropixels, tight rows (ffmpeg's rawvideo
// yuyv422 / uyvy422), through jpezy_decode_jpeg_yuv422; exactly four arguments, every other option is a usage error
int yuv422_main(const int argc, const char* argv[], const int format)
{
    if (argc != 4) {
        std::cerr << "Usage: jpezy_decode --yuy2 | --uyvy <input.(jpg | jpeg)> <output.yuv>" << std::endl;
        return EXIT_FAILURE;
    }
    jpezy::disp_logo();
    std::ifstream ifs(argv[2], std::ios::binary);
    const std::vector<std::uint8_t> data((std::istreambuf_iterator<char>(ifs)), std::istreambuf_iterator<char>());
    jpezy_ctx* ctx = jpezy::detail::device_context();
    jpezy_frame_info info;
    if (!ifs.is_open() || jpezy_decode_jpeg_yuv422(ctx, data.data(), data.size(), &info, format, 0, nullptr, 0) != JPEZY_OK) {
        std::cerr << "decode failed" << std::endl;
        return EXIT_FAILURE;
    }
    std::vector<std::uint8_t> out(static_cast<std::size_t>(jpezy_yuv422_row_bytes(info.width)) * info.height);
    if (jpezy_decode_jpeg_yuv422(ctx, data.data(), data.size(), &info, format, 0, out.data(), out.size()) != JPEZY_OK) {
        std::cerr << "decode failed: " << jpezy_hip_last_error() << std::endl;
        return EXIT_FAILURE;
    }
    std::ofstream ofs(argv[3], std::ios::binary | std::ios::trunc);
    ofs.write(reinterpret_cast<const char*>(out.data()), static_cast<std::streamsize>(out.size()));
    if (!ofs) { std::cerr << "output_file" << std::endl; return EXIT_FAILURE; }
    std::cout << "Decoded image: raw packed YCbCr 4:2:2 (" << (format == JPEZY_YUV_UYVY ? "UYVY" : "YUY2") << "), size = " << info.width << " x "
              << info.height << std::endl;
    return EXIT_SUCCESS;
}

}  // namespace

int main(const int argc, const char* argv[])
{
    if (argc >= 2 && (std::string_view(argv[1]) == "--yuy2" || std::string_view(argv[1]) == "--uyvy")) {
        try {
            return yuv422_main(argc, argv, std::string_view(argv[1]) == "--uyvy" ? JPEZY_YUV_UYVY : JPEZY_YUV_YUY2);
        } catch (const std::runtime_error& e) {
            std::cerr << e.what() << std::endl;
            return EXIT_FAILURE;
        }
    }
    if (argc >= 2 && std::string_view(argv[1]) == "--i420") {
        for (int k = 2; k < argc; ++k) {
            const int up = upsampling_of(argv[k]);
            if (up == -2) return disp_error();
            if (up == JPEZY_UPSAMPLE_SMOOTH) return upsampling_rule();
        }
        try {
            return i420_main(argc, argv);
        } catch (const std::runtime_error& e) {
            std::cerr << e.what() << std::endl;
            return EXIT_FAILURE;
        }
    }
    if (argc > 6 || argc < 3) return disp_error();

    const std::string_view sv0 = argv[1], sv1 = argv[2];
    const std::string_view opt[3] = { argc > 3 ? std::string_view(argv[3]) : std::string_view(), argc > 4 ? std::string_view(argv[4]) : std::string_view(),
                                      argc > 5 ? std::string_view(argv[5]) : std::string_view() };

    if (!((has_ext(sv0, "jpeg") || has_ext(sv0, "jpg")) && has_ext(sv1, "ppm"))) return disp_error();

    bool gray = false, verbose = false, has_region = false, orient = false;
    int scale = 1, upsampling = -1;
    jpezy_rect region{};
    for (const std::string_view sv : opt) {
        gray = gray || sv.find("--gray") != std::string_view::npos;
        verbose = verbose || sv.find("-v") != std::string_view::npos;
        const int sc = scale_of(sv);
        if (!sc) return disp_error();
        if (scale == 1) scale = sc;
        jpezy_rect r;
        const int rg = region_of(sv, &r);
        if (!rg) return disp_error();
        if (rg > 0 && !has_region) { region = r; has_region = true; }
        const int up = upsampling_of(sv);
        if (up == -2) return disp_error();
        if (upsampling < 0) upsampling = up;
        if (sv.substr(0, 8) == "--orient") {
            if (sv != "--orient") return disp_error();
            orient = true;
        }
    }
    if (upsampling < 0) upsampling = JPEZY_UPSAMPLE_NEAREST;
    if (upsampling == JPEZY_UPSAMPLE_SMOOTH && (scale != 1 || has_region)) return upsampling_rule();
    const jpezy_rect* rp = has_region ? &region : nullptr;
    try {
        return verbose ? run<jpezy::Debug>(argv[1], argv[2], gray, scale, rp, upsampling, orient)
                       : run<jpezy::Release>(argv[1], argv[2], gray, scale, rp, upsampling, orient);
    } catch (const std::runtime_error& e) {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }
}
