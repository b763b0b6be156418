// Test program of tests/test_gpu_sampling422.py: encoder::encode(file, JPEZY_SAMPLING_422) through the C++ interface's own pipe
// syntax -- the call jpezy_encode makes for --sampling=444, with the value the CLI does not spell yet.
//   encode422_main in.ppm out.jpg [average]
#include <fstream>
#include <iostream>
#include <string>

#include "encode_io.hpp"

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    jpezy::encode_io pnm(argv[1]);
    if (!pnm) return 3;
    try {
        if (argc > 3 && std::string(argv[3]) == "average" &&
            jpezy_ctx_set_chroma_downsampling(jpezy::detail::device_context(), JPEZY_DOWNSAMPLE_AVERAGE) != JPEZY_OK)
            return 4;
        std::ofstream ofs(argv[2], std::ios::binary);
        ofs << (pnm | jpezy::to_jpeg(argv[2], JPEZY_SAMPLING_422));
    } catch (const std::runtime_error& e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
    return 0;
}
