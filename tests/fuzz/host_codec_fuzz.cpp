// ASan/UBSan harness for the host-side codec (marker parser, Huffman decoder, writer): built and driven by
// tests/fuzz/run_host_fuzz.py on the CPU (sanitizers are not available on the GPU pool).  Every file named on the
// command line (or listed in @file) goes through parse_header and read_jpeg; what decodes is written again with
// write_jpeg when it has jpezy's own layout.  The harness only checks that nothing reads or writes out of bounds and
// that errors come back as error codes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../jpezy_amd/csrc/jpezy_host_codec.h"

static std::vector<unsigned char> slurp(const char* path)
{
    std::ifstream f(path, std::ios::binary);
    return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv)
{
    std::vector<std::string> files;
    for (int i = 1; i < argc; ++i) {
        if (argv[i][0] == '@') {
            std::ifstream l(argv[i] + 1);
            for (std::string s; std::getline(l, s);) if (!s.empty()) files.push_back(s);
        } else files.push_back(argv[i]);
    }
    size_t ok = 0, rejected = 0, rewritten = 0;
    for (const std::string& path : files) {
        const std::vector<unsigned char> d = slurp(path.c_str());
        jpezy_frame_info info;
        std::memset(&info, 0, sizeof info);
        jpezy_host::ScanSetup setup;
        std::string err;
        if (jpezy_host::parse_header(d.data(), d.size(), &info, &setup, &err) < 0) { ++rejected; continue; }
        const size_t ncoef = (size_t)info.mcu_cols * info.mcu_rows * info.blocks_per_mcu * 64;
        if (ncoef == 0 || ncoef > (size_t(1) << 26)) { ++rejected; continue; }       // absurd dimensions: not this harness' business
        std::vector<int16_t> co(ncoef);
        std::memset(&info, 0, sizeof info);
        if (jpezy_host::read_jpeg(d.data(), d.size(), &info, co.data(), co.size(), &err) < 0) { ++rejected; continue; }
        ++ok;
        const bool own = info.ncomp == 3 && info.H[0] == 2 && info.V[0] == 2 && info.H[1] == 1 && info.V[1] == 1 && info.H[2] == 1 && info.V[2] == 1;
        if (own && info.width > 0 && info.height > 0) {
            std::vector<unsigned char> out(jpezy_host::jpeg_bound(info.width, info.height));
            (void)jpezy_host::write_jpeg(co.data(), info.width, info.height, false, nullptr, 0, false, out.data(), out.size(), &err);
            // a deliberately short buffer must be refused, not overrun
            (void)jpezy_host::write_jpeg(co.data(), info.width, info.height, false, nullptr, 0, false, out.data(), out.size() / 16, &err);
            ++rewritten;
        }
    }
    std::printf("%zu files: %zu decoded, %zu rejected, %zu re-encoded\n", files.size(), ok, rejected, rewritten);
    return 0;
}
