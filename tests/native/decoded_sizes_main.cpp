// decoded_sizes_main.cpp -- streamly_lz4::Engine::decodedSizes from a program of its own (tests/test_decoded_size_gpu.py):
//   decoded_sizes_main STREAM.bin CHECKSUMS(0|1) MAXUNCOMP   prints one size or per-block code per line
// The stream is a dense BlockMax4MB one (headerKind 4).  Exit status 1 with the message on stderr when the call throws.
#include "streamly_lz4.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    const streamly_lz4::Array framed((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    streamly_lz4::BlockConfig cfg = streamly_lz4::setBlockMaxSize(streamly_lz4::BlockSize::BlockMax4MB, streamly_lz4::defaultBlockConfig());
    cfg = streamly_lz4::setBlockChecksum(std::atoi(argv[2]) != 0, cfg);
    try {
        streamly_lz4::Engine eng(0);
        for (int32_t s : eng.decodedSizes(cfg, framed, std::atoi(argv[3]))) std::printf("%d\n", (int)s);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
