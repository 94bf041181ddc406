// dict_mirror_main.cpp -- the C++ mirror of the shared-dictionary calls from a program of its own (tests/test_dict_gpu.py):
//   dict_mirror_main DICT.bin RECORDS.bin RECORD_LEN FRAMED.bin DECODED.bin
// CompressStreams::loadDict on slot 0 (the dictionary copied to device memory first), Engine::compressWithDict over the records
// (RECORDS.bin cut every RECORD_LEN bytes), Engine::decompressWithDict over what that gave; writes the framed arrays and the
// decoded arrays back to back and prints one framed length per line.  Exit status 1 with the message on stderr when a call throws.
#include "streamly_lz4.hpp"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

static streamly_lz4::Array slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    return streamly_lz4::Array((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char **argv)
{
    if (argc != 6) return 2;
    const streamly_lz4::Array dict = slurp(argv[1]), all = slurp(argv[2]);
    const size_t len = (size_t)std::atoi(argv[3]);
    std::vector<streamly_lz4::Array> records;
    for (size_t at = 0; at < all.size(); at += len)
        records.emplace_back(all.begin() + (long)at, all.begin() + (long)(at + len < all.size() ? at + len : all.size()));
    const streamly_lz4::BlockConfig cfg = streamly_lz4::defaultBlockConfig();
    try {
        streamly_lz4::Engine eng(0);
        uint8_t *dDev = nullptr;
        if (hipMalloc((void **)&dDev, dict.size() + 1) != hipSuccess ||
            hipMemcpy(dDev, dict.data(), dict.size(), hipMemcpyHostToDevice) != hipSuccess)
            return 3;
        streamly_lz4::CompressStreams cs(eng, 1);
        cs.loadDict(0, dDev, (int)dict.size());
        const std::vector<streamly_lz4::Array> framed = eng.compressWithDict(cfg, 1, records, cs, 0);
        std::ofstream fo(argv[4], std::ios::binary), dout(argv[5], std::ios::binary);
        for (const streamly_lz4::Array &a : framed) {
            std::printf("%zu\n", a.size());
            fo.write((const char *)a.data(), (std::streamsize)a.size());
        }
        for (const streamly_lz4::Array &a : eng.decompressWithDict(cfg, framed, dict))
            dout.write((const char *)a.data(), (std::streamsize)a.size());
        (void)hipDeviceSynchronize();
        (void)hipFree(dDev);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
