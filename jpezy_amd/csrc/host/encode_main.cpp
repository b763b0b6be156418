// jpezy_encode <input.ppm> ( <output.(jpeg | jpg) [OPT: --gray] [OPT: --optimize] [OPT: --restart=N] [OPT: --quality=N] [OPT: --chroma=average|point]> | <output.ppm> | --debug )
// Same argv rules, transcript and exit codes as the reference's src/encoder/main.cpp; the codec underneath is
// the MI355X path (jpezy_encoder.hpp).
// Extension (not in the reference):  --optimize (single-file mode only, either side of --gray) writes the file with its own optimal
// Huffman tables (jpezy_ctx_set_huffman_optimize): same pixels, fewer bytes.
// Extension (not in the reference):  --restart=N (single-file mode only, one token, anywhere behind the output name) writes restart
// intervals of N MCUs, 0..65535 (jpezy_ctx_set_restart_interval); a malformed N is a usage error.
// Extension (not in the reference):  --quality=N (single-file mode and --i420, one token, anywhere behind the output name) encodes with
// libjpeg's quality N, 1..100 (jpezy_ctx_set_quality; 50 is the default); a malformed or out-of-range N is a usage error.
// Extension (not in the reference):  --sampling=444|420 (single-file mode, one token, anywhere behind the output name) writes the file with
// 4:4:4 chroma sampling (jpezy_encode_jpeg_sampling: 8 x 8 MCUs, no chroma decimation) or, the default, 4:2:0; composes with --optimize,
// --restart, --quality and --gpus 1.  Together with --gray, --i420 or --gpus N > 1, 444 prints the rule and exits 1.
// Extension (not in the reference):  --chroma=average|point (single-file mode, one token, anywhere behind the output name) makes the 4:2:0
// chroma by averaging every 2x2 (jpezy_ctx_set_chroma_downsampling, JPEZY_DOWNSAMPLE_AVERAGE) or, the default, from its top-left pixel;
// composes with --optimize, --restart, --quality, --sampling=420 and --gpus 1.  Together with --gray, --i420, --sampling=444 or
// --gpus N > 1, average prints the rule and exits 1; point is always the file without the flag.
// Extension (not in the reference):  jpezy_encode --gpus N [--gray] <in1.ppm> <out1.jpg> [<in2.ppm> <out2.jpg> ...]
// encodes a list of files on up to N GPUs of this node through jpezy_encode_batch_multi: runs of consecutive inputs of one size
// form a batch, a batch is sharded over the GPUs frame by frame.
// Extension (not in the reference):  jpezy_encode --i420=WxH <in.yuv> <out.jpg> [--gray] [--optimize] [--restart=N] [--quality=N]
// encodes a raw planar YCbCr 4:2:0 file -- the W x H Y plane, then the ceil(W/2) x ceil(H/2) Cb and Cr planes, full range (ffmpeg's
// yuvj420p) -- through jpezy_encode_jpeg_ycc: the samples go into the file as they are, without a colour conversion.
// Extension (not in the reference):  jpezy_encode --yuy2=WxH | --uyvy=WxH <in.yuv> <out.jpg> [--optimize] [--restart=N] [--quality=N]
// encodes raw packed YCbCr 4:2:2 macropixels, tight rows of 4 * ceil(W/2) bytes, full range (ffmpeg's rawvideo yuyv422 / uyvy422) into a
// 4:2:2 file through jpezy_encode_jpeg_yuv422, on the --i420 code path; every other option there is a usage error.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <string_view>

#include "encode_io.hpp"

#include <cstdint>
#include <vector>

namespace {

int disp_error()
{
    std::cerr << "Usage: jpezy_encode <input.ppm> ( <ouput.(jpeg | jpg) [OPT: --gray]> | <output.ppm> | --debug )" << std::endl;
    return EXIT_FAILURE;
}

enum class Mode { JPEG, GRAY, PPM, DEBUG, UD };

// "jpeg"/"jpg"/"ppm" anywhere after the first '.', as the reference's find(pattern, find_first_of('.')) (:71-84)
bool has_ext(std::string_view s, std::string_view ext)
{
    return s.find(ext, s.find_first_of('.')) != std::string_view::npos;
}

// jpezy_encode --gpus N [--gray] in out [in out ...]
int parse_sampling(std::string_view tok);
int sampling_rule();
int take_sampling(std::vector<const char*>& args, std::size_t from);
int parse_chroma(std::string_view tok);
int chroma_rule();
int take_chroma(std::vector<const char*>& args, std::size_t from);

int batch_main(const int argc_in, const char* argv_in[])
{
    std::vector<const char*> args(argv_in, argv_in + argc_in);
    const int sampling = take_sampling(args, 3);
    const int chroma = take_chroma(args, 3);
    const int argc = static_cast<int>(args.size());
    const char* const* argv = args.data();
    const int want = std::atoi(argv[2]);
    int a = 3;
    bool gray = false;
    if (a < argc && std::string_view(argv[a]) == "--gray") { gray = true; ++a; }
    if (want <= 0 || a >= argc || (argc - a) % 2 != 0 || sampling < 0 || chroma < 0) {
        std::cerr << "Usage: jpezy_encode --gpus N [--gray] <in1.ppm> <out1.jpg> [<in2.ppm> <out2.jpg> ...]" << std::endl;
        return EXIT_FAILURE;
    }
    if (sampling == JPEZY_SAMPLING_444 && (gray || want > 1)) return sampling_rule();
    if (chroma == JPEZY_DOWNSAMPLE_AVERAGE && (gray || want > 1 || sampling == JPEZY_SAMPLING_444)) return chroma_rule();
    const int have = jpezy_hip_device_count();
    if (have <= 0) { std::cerr << "jpezy_encode: no HIP device (the jpezy hot path has no CPU fallback)" << std::endl; return EXIT_FAILURE; }
    std::vector<int> devices;
    for (int d = 0; d < want && d < have; ++d) devices.push_back(d);
    jpezy::disp_logo();
    const int n_files = (argc - a) / 2;
    int f = 0;
    jpezy_ctx* single = nullptr;
    while (f < n_files) {
        std::vector<std::uint8_t> r, g, b;
        std::size_t W = 0, H = 0;
        int n = 0;
        for (; f + n < n_files; ++n) {                      // a run of consecutive inputs of one size
            jpezy::encode_io pnm(argv[a + 2 * (f + n)]);
            if (!pnm) { std::cerr << "The file is not found or the formatting error" << std::endl; return EXIT_FAILURE; }
            if (n == 0) { W = pnm.image_width(); H = pnm.image_height(); }
            else if (pnm.image_width() != W || pnm.image_height() != H) break;
            pnm.append_planes(r, g, b);
        }
        const std::size_t stride = jpezy_jpeg_bound_sampling(static_cast<int>(W), static_cast<int>(H), sampling);
        std::vector<std::uint8_t> jpg(stride * static_cast<std::size_t>(n));
        std::vector<long long> sizes(static_cast<std::size_t>(n));
        const char* comment = gray ? "Encoded by JPEZY" : "Encoded by jpezy";
        if (sampling == JPEZY_SAMPLING_444) {      // one GPU (checked above): frame by frame through the single-file entry
            if (!single) single = jpezy_ctx_create(devices[0]);
            if (!single) { std::cerr << "jpezy_ctx_create: " << jpezy_hip_last_error() << std::endl; return EXIT_FAILURE; }
            const std::size_t px = W * H;
            for (int i = 0; i < n; ++i) {
                const std::size_t o = px * static_cast<std::size_t>(i);
                sizes[static_cast<std::size_t>(i)] = jpezy_encode_jpeg_sampling(single, r.data() + o, g.data() + o, b.data() + o, static_cast<int>(W), static_cast<int>(H),
                                                                                sampling, 0, comment, jpg.data() + stride * static_cast<std::size_t>(i), stride);
                if (sizes[static_cast<std::size_t>(i)] < 0) { std::cerr << "jpezy_encode_jpeg_sampling: " << jpezy_hip_last_error() << std::endl; jpezy_ctx_destroy(single); return EXIT_FAILURE; }
            }
        } else if (n == 1 || chroma == JPEZY_DOWNSAMPLE_AVERAGE) {
            // a run of one frame has nothing to shard: the ordinary single-file path (streams the frame band by band, no ring of
            // whole-frame slots: a 16K x 16K file would otherwise reserve several GB of pinned memory for nothing)
            if (!single) single = jpezy_ctx_create(devices[0]);
            if (!single) { std::cerr << "jpezy_ctx_create: " << jpezy_hip_last_error() << std::endl; return EXIT_FAILURE; }
            // (--chroma=average, one GPU, checked above: the multi-GPU handle always point-samples, so every frame of the run goes this way)
            if (jpezy_ctx_set_chroma_downsampling(single, chroma) != JPEZY_OK) { std::cerr << "jpezy_ctx_set_chroma_downsampling: " << jpezy_hip_last_error() << std::endl; jpezy_ctx_destroy(single); return EXIT_FAILURE; }
            const std::size_t px = W * H;
            for (int i = 0; i < n; ++i) {
                const std::size_t o = px * static_cast<std::size_t>(i);
                sizes[static_cast<std::size_t>(i)] = jpezy_encode_jpeg(single, r.data() + o, g.data() + o, b.data() + o, static_cast<int>(W), static_cast<int>(H), gray ? 1 : 0,
                                                                       comment, jpg.data() + stride * static_cast<std::size_t>(i), stride);
                if (sizes[static_cast<std::size_t>(i)] < 0) { std::cerr << "jpezy_encode_jpeg: " << jpezy_hip_last_error() << std::endl; jpezy_ctx_destroy(single); return EXIT_FAILURE; }
            }
        } else {
            jpezy_multi_out out{ nullptr, jpg.data(), stride, sizes.data(), 0 };
            const int rc = jpezy_encode_batch_multi(devices.data(), static_cast<int>(devices.size()), r.data(), g.data(), b.data(), static_cast<int>(W),
                                                    static_cast<int>(H), gray ? 1 : 0, n, 0, comment, &out);
            if (rc != JPEZY_OK) { std::cerr << "jpezy_encode_batch_multi: " << jpezy_hip_last_error() << std::endl; if (single) jpezy_ctx_destroy(single); return EXIT_FAILURE; }
        }
        for (int i = 0; i < n; ++i) {
            const char* name = argv[a + 2 * (f + i) + 1];
            std::ofstream ofs(name, std::ios::binary);
            ofs.write(reinterpret_cast<const char*>(jpg.data() + stride * static_cast<std::size_t>(i)), static_cast<std::streamsize>(sizes[static_cast<std::size_t>(i)]));
            if (!ofs) { std::cerr << "output_file" << std::endl; return EXIT_FAILURE; }
            std::cout << name << ": Output size: " << sizes[static_cast<std::size_t>(i)] << " byte" << std::endl;
        }
        f += n;
    }
    if (single) jpezy_ctx_destroy(single);
    std::cout << "Encoded " << n_files << " file(s) on " << devices.size() << " GPU(s)" << std::endl;
    return EXIT_SUCCESS;
}

// a decimal number in 0..65535, or -1
int parse_u16(std::string_view tok)
{
    if (tok.empty() || tok.size() > 5) return -1;
    int n = 0;
    for (const char ch : tok) {
        if (ch < '0' || ch > '9') return -1;
        n = n * 10 + (ch - '0');
    }
    return n <= 65535 ? n : -1;
}

// "--restart=N" with N a decimal number in 0..65535: N; anything else that starts like it: -1
int parse_restart(std::string_view tok)
{
    tok.remove_prefix(std::string_view("--restart=").size());
    return parse_u16(tok);
}

// "--quality=N" with N a decimal number in 1..100: N; anything else that starts like it: -1
int parse_quality(std::string_view tok)
{
    tok.remove_prefix(std::string_view("--quality=").size());
    const int n = parse_u16(tok);
    return n >= 1 && n <= 100 ? n : -1;
}

// "--sampling=444" / "--sampling=420": JPEZY_SAMPLING_*; anything else that starts like it: -1
int parse_sampling(std::string_view tok)
{
    tok.remove_prefix(std::string_view("--sampling=").size());
    return tok == "444" ? JPEZY_SAMPLING_444 : tok == "420" ? JPEZY_SAMPLING_420 : -1;
}

int sampling_rule()
{
    std::cerr << "jpezy_encode: --sampling=444 writes colour files from RGB input on one GPU; it cannot be combined with --gray, --i420 or --gpus N > 1"
              << std::endl;
    return EXIT_FAILURE;
}

// takes the one "--sampling=..." token at or behind position `from` out of args: its value, JPEZY_SAMPLING_420 when there is none, -1 malformed
int take_sampling(std::vector<const char*>& args, std::size_t from)
{
    for (std::size_t i = from; i < args.size(); ++i)
        if (std::string_view(args[i]).rfind("--sampling=", 0) == 0) {
            const int s = parse_sampling(args[i]);
            args.erase(args.begin() + static_cast<std::ptrdiff_t>(i));
            return s;
        }
    return JPEZY_SAMPLING_420;
}

// "--chroma=average" / "--chroma=point": JPEZY_DOWNSAMPLE_*; anything else that starts like it: -1
int parse_chroma(std::string_view tok)
{
    tok.remove_prefix(std::string_view("--chroma=").size());
    return tok == "average" ? JPEZY_DOWNSAMPLE_AVERAGE : tok == "point" ? JPEZY_DOWNSAMPLE_POINT : -1;
}

int chroma_rule()
{
    std::cerr << "jpezy_encode: --chroma=average averages the 4:2:0 chroma of colour files from RGB input on one GPU; it cannot be combined with --gray, "
                 "--i420, --sampling=444 or --gpus N > 1"
              << std::endl;
    return EXIT_FAILURE;
}

// takes the one "--chroma=..." token at or behind position `from` out of args: its value, JPEZY_DOWNSAMPLE_POINT when there is none, -1 malformed
int take_chroma(std::vector<const char*>& args, std::size_t from)
{
    for (std::size_t i = from; i < args.size(); ++i)
        if (std::string_view(args[i]).rfind("--chroma=", 0) == 0) {
            const int s = parse_chroma(args[i]);
            args.erase(args.begin() + static_cast<std::ptrdiff_t>(i));
            return s;
        }
    return JPEZY_DOWNSAMPLE_POINT;
}

// jpezy_encode --i420=WxH in.yuv out.jpg [--gray] [--optimize] [--restart=N] [--quality=N]
// yuv >= 0 (JPEZY_YUV_YUY2 / JPEZY_YUV_UYVY): jpezy_encode --yuy2=WxH | --uyvy=WxH in.yuv out.jpg [--optimize] [--restart=N] [--quality=N]
int i420_main(const int argc, const char* argv[], const int yuv = -1)
{
    const auto usage = [yuv] {
        if (yuv >= 0)
            std::cerr << "Usage: jpezy_encode --yuy2=WxH | --uyvy=WxH <input.yuv> <output.(jpeg | jpg)> [OPT: --optimize] [OPT: --restart=N] [OPT: --quality=N]" << std::endl;
        else
            std::cerr << "Usage: jpezy_encode --i420=WxH <input.yuv> <output.(jpeg | jpg)> [OPT: --gray] [OPT: --optimize] [OPT: --restart=N] [OPT: --quality=N]" << std::endl;
        return EXIT_FAILURE;
    };
    std::string_view dims = argv[1];
    dims.remove_prefix(std::string_view("--i420=").size());      // (--yuy2= and --uyvy= are as long)
    const auto x = dims.find('x');
    if (x == std::string_view::npos || argc < 4) return usage();
    const int W = parse_u16(dims.substr(0, x)), H = parse_u16(dims.substr(x + 1));
    if (W <= 0 || H <= 0) return usage();
    bool gray = false, optimize = false;
    int restart = 0, quality = 0;
    for (int i = 4; i < argc; ++i) {
        const std::string_view o = argv[i];
        if (o == "--gray" && yuv < 0) gray = true;
        else if (o == "--optimize") optimize = true;
        else if (o.rfind("--restart=", 0) == 0 && (restart = parse_restart(o)) >= 0) continue;
        else if (o.rfind("--quality=", 0) == 0 && (quality = parse_quality(o)) >= 1) continue;
        else if (yuv >= 0) return usage();                         // no gray form, one sampling, the caller's chroma
        else if (o.rfind("--sampling=", 0) == 0 && parse_sampling(o) == JPEZY_SAMPLING_420) continue;
        else if (o.rfind("--sampling=", 0) == 0 && parse_sampling(o) == JPEZY_SAMPLING_444) return sampling_rule();
        else if (o.rfind("--chroma=", 0) == 0 && parse_chroma(o) == JPEZY_DOWNSAMPLE_POINT) continue;
        else if (o.rfind("--chroma=", 0) == 0 && parse_chroma(o) == JPEZY_DOWNSAMPLE_AVERAGE) return chroma_rule();
        else return usage();
    }
    jpezy::disp_logo();
    int CW = 0, CH = 0;
    jpezy_ycc_chroma_size(W, H, &CW, &CH);
    const std::size_t ny = static_cast<std::size_t>(W) * H, nc = static_cast<std::size_t>(CW) * CH;
    std::ifstream ifs(argv[2], std::ios::binary);
    std::vector<std::uint8_t> buf((std::istreambuf_iterator<char>(ifs)), std::istreambuf_iterator<char>());
    if (yuv >= 0) {
        const std::size_t need = static_cast<std::size_t>(jpezy_yuv422_row_bytes(W)) * H;
        if (!ifs.is_open() || buf.size() != need) {
            std::cerr << "jpezy_encode: " << argv[2] << " must hold " << need << " bytes (rows of " << jpezy_yuv422_row_bytes(W) << " bytes of a " << W
                      << " x " << H << " picture), it holds " << buf.size() << std::endl;
            return EXIT_FAILURE;
        }
    } else if (!ifs.is_open() || buf.size() != ny + 2 * nc) {
        std::cerr << "jpezy_encode: " << argv[2] << " must hold " << ny + 2 * nc << " bytes (Y, Cb, Cr planes of a " << W << " x " << H
                  << " picture), it holds " << buf.size() << std::endl;
        return EXIT_FAILURE;
    }
    try {
        jpezy_ctx* ctx = jpezy::detail::device_context();
        if (optimize && jpezy_ctx_set_huffman_optimize(ctx, 1) != JPEZY_OK) throw std::runtime_error(std::string("jpezy_ctx_set_huffman_optimize: ") + jpezy_hip_last_error());
        if (restart && jpezy_ctx_set_restart_interval(ctx, restart) != JPEZY_OK) throw std::runtime_error(std::string("jpezy_ctx_set_restart_interval: ") + jpezy_hip_last_error());
        if (quality && jpezy_ctx_set_quality(ctx, quality) != JPEZY_OK) throw std::runtime_error(std::string("jpezy_ctx_set_quality: ") + jpezy_hip_last_error());
        std::vector<std::uint8_t> jpg(yuv >= 0 ? jpezy_jpeg_bound_sampling(W, H, JPEZY_SAMPLING_422) : jpezy_jpeg_bound(W, H));
        const long n = yuv >= 0 ? jpezy_encode_jpeg_yuv422(ctx, buf.data(), yuv, 0, W, H, "Encoded by jpezy", jpg.data(), jpg.size())
                                : jpezy_encode_jpeg_ycc(ctx, buf.data(), 0, buf.data() + ny, buf.data() + ny + nc, 0, 1, W, H, gray ? 1 : 0,
                                                        gray ? "Encoded by JPEZY" : "Encoded by jpezy", jpg.data(), jpg.size());
        if (n < 0) throw std::runtime_error(std::string(yuv >= 0 ? "jpezy_encode_jpeg_yuv422: " : "jpezy_encode_jpeg_ycc: ") + jpezy_hip_last_error());
        std::ofstream ofs(argv[3], std::ios::binary);
        ofs.write(reinterpret_cast<const char*>(jpg.data()), static_cast<std::streamsize>(n));
        if (!ofs) throw std::runtime_error("output_file");
        std::cout << argv[3] << ": Output size: " << n << " byte" << std::endl;
    } catch (const std::runtime_error& e) {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }
    return EXIT_SUCCESS;
}

}  // namespace

int main(const int argc_in, const char* argv_in[])
{
    if (argc_in >= 3 && std::string_view(argv_in[1]) == "--gpus") return batch_main(argc_in, argv_in);
    if (argc_in >= 2 && std::string_view(argv_in[1]).rfind("--i420=", 0) == 0) return i420_main(argc_in, argv_in);
    if (argc_in >= 2 && std::string_view(argv_in[1]).rfind("--yuy2=", 0) == 0) return i420_main(argc_in, argv_in, JPEZY_YUV_YUY2);
    if (argc_in >= 2 && std::string_view(argv_in[1]).rfind("--uyvy=", 0) == 0) return i420_main(argc_in, argv_in, JPEZY_YUV_UYVY);
    if (argc_in < 3) return disp_error();
    // the one --restart=N and the one --quality=N token are taken out; what is left is read as before
    std::vector<const char*> args(argv_in, argv_in + argc_in);
    int restart = 0, quality = 0;
    for (std::size_t i = 3; i < args.size(); ++i)
        if (std::string_view(args[i]).rfind("--restart=", 0) == 0) {
            restart = parse_restart(args[i]);
            if (restart < 0) return disp_error();
            args.erase(args.begin() + static_cast<std::ptrdiff_t>(i));
            break;
        }
    for (std::size_t i = 3; i < args.size(); ++i)
        if (std::string_view(args[i]).rfind("--quality=", 0) == 0) {
            quality = parse_quality(args[i]);
            if (quality < 0) return disp_error();
            args.erase(args.begin() + static_cast<std::ptrdiff_t>(i));
            break;
        }
    const int sampling = take_sampling(args, 3);
    if (sampling < 0) return disp_error();
    const int chroma = take_chroma(args, 3);
    if (chroma < 0) return disp_error();
    const int argc = static_cast<int>(args.size());
    const char* const* argv = args.data();

    Mode m1 = Mode::UD, m2 = Mode::UD;
    bool optimize = false;
    const std::string_view sv1 = argv[2];
    const std::string_view sv2 = argc > 3 ? std::string_view(argv[3]) : std::string_view();   // the reference reads argv[3] unguarded

    if (has_ext(sv1, "jpeg") || has_ext(sv1, "jpg")) {
        m1 = Mode::JPEG;
        if (sv2.find("--gray") != std::string_view::npos) m2 = Mode::GRAY;
        const std::string_view sv3 = argc > 4 ? std::string_view(argv[4]) : std::string_view();
        optimize = sv2 == "--optimize" || sv3 == "--optimize";
        if (sv2 == "--optimize" && sv3 == "--gray") m2 = Mode::GRAY;
    } else if (has_ext(sv1, "ppm")) {
        m1 = Mode::PPM;
    } else if (sv1 == "--debug") {
        m1 = Mode::DEBUG;
    } else {
        return disp_error();
    }
    if (sampling == JPEZY_SAMPLING_444 && (m1 != Mode::JPEG || m2 == Mode::GRAY)) return m1 == Mode::JPEG ? sampling_rule() : disp_error();
    if (chroma == JPEZY_DOWNSAMPLE_AVERAGE && (m1 != Mode::JPEG || m2 == Mode::GRAY || sampling == JPEZY_SAMPLING_444))
        return m1 == Mode::JPEG ? chroma_rule() : disp_error();

    jpezy::disp_logo();

    jpezy::raii_messenger section("Reading the input file...");
    jpezy::encode_io pnm(argv[1]);
    if (!pnm) {
        std::cerr << "The file is not found or the formatting error" << std::endl;
        return disp_error();
    }
    const auto t1 = section.stop();
    section.restart("Start encoding and writing ...");

    try {
        if (m1 == Mode::JPEG) {
            if (optimize && jpezy_ctx_set_huffman_optimize(jpezy::detail::device_context(), 1) != JPEZY_OK)
                throw std::runtime_error(std::string("jpezy_ctx_set_huffman_optimize: ") + jpezy_hip_last_error());
            if (restart && jpezy_ctx_set_restart_interval(jpezy::detail::device_context(), restart) != JPEZY_OK)
                throw std::runtime_error(std::string("jpezy_ctx_set_restart_interval: ") + jpezy_hip_last_error());
            if (quality && jpezy_ctx_set_quality(jpezy::detail::device_context(), quality) != JPEZY_OK)
                throw std::runtime_error(std::string("jpezy_ctx_set_quality: ") + jpezy_hip_last_error());
            if (chroma && jpezy_ctx_set_chroma_downsampling(jpezy::detail::device_context(), chroma) != JPEZY_OK)
                throw std::runtime_error(std::string("jpezy_ctx_set_chroma_downsampling: ") + jpezy_hip_last_error());
            std::ofstream ofs(argv[2], std::ios::binary);
            if (m2 == Mode::GRAY) ofs << (pnm | jpezy::to_jpeg(argv[2]) | jpezy::gray_scale);
            else ofs << (pnm | jpezy::to_jpeg(argv[2], sampling));
        } else if (m1 == Mode::PPM) {
            std::ofstream ofs(argv[2]);
            static_cast<std::ostream&>(ofs) << pnm;
        } else {
            std::cout << pnm << std::endl;
        }
    } catch (const std::runtime_error& e) {
        std::cerr << e.what() << std::endl;
        return EXIT_FAILURE;
    }

    const auto t2 = section.stop();
    if (t1 && t2) std::cout << "Total processing time: " << *t1 + *t2 << std::endl;
    return EXIT_SUCCESS;
}
