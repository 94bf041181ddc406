// decompress_partial_main.cpp -- streamly_lz4::Engine::decompressPartial from a program of its own (tests/test_partial_decode_gpu.py):
//   decompress_partial_main STREAM.bin CHECKSUMS(0|1) TARGET OUT.bin   writes the prefixes back to back, prints one length per line
// The stream is a dense one with sizes in its headers (headerKind 8).  Exit status 1 with the message on stderr when the call throws.
#include "streamly_lz4.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    std::ifstream f(argv[1], std::ios::binary);
    const streamly_lz4::Array framed((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    streamly_lz4::BlockConfig cfg = streamly_lz4::setBlockChecksum(std::atoi(argv[2]) != 0, streamly_lz4::defaultBlockConfig());
    try {
        streamly_lz4::Engine eng(0);
        std::ofstream o(argv[4], std::ios::binary);
        for (const streamly_lz4::Array &a : eng.decompressPartial(cfg, framed, std::atoi(argv[3]))) {
            std::printf("%zu\n", a.size());
            o.write((const char *)a.data(), (std::streamsize)a.size());
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
