// dict_args_main.cpp -- the argument checks of the shared-dictionary calls (mi355lz4_cstreams_load_dict, mi355lz4_compress_dict_device,
// mi355lz4_decompress_dict_device, mi355lz4_compress_dict, mi355lz4_decompress_dict) from a program of its own, built from the host
// sources with -fsanitize=address,undefined against the stubbed launchers of san_stubs.cpp and san_stubs_dict.cpp (`make asan-dict`).  No device is needed
// and none is used: every call here returns before its first HIP call -- a launcher reached would abort.  The engine
// the decode checks run against is a plain mi355lz4_ctx of this program's own (engine.hpp), never created on or handed to a device;
// a mi355lz4_cstreams cannot be had without a device, so the calls that take one are driven up to its null check.
#include "../../streamly-lz4_amd/csrc/engine.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed: %s\n", __FILE__, __LINE__, #cond, mi355lz4_last_error()); \
            failures++;                                                     \
        }                                                                   \
    } while (0)

static bool said(const char *what) { return std::strstr(mi355lz4_last_error(), what) != nullptr; }

int main()
{
    uint8_t byte[64] = {0};
    uint64_t off[2] = {0, 0};
    int32_t len[2] = {0, 0}, res[2] = {7, 7};
    const uint8_t *ptrs[2] = {byte, byte};
    mi355lz4_ctx eng;                       // switches at their defaults, nothing of a device
    mi355lz4_cstreams *noSet = nullptr;

    // ---- the compress side: a null engine, a null set
    CHECK(mi355lz4_cstreams_load_dict(nullptr, noSet, 0, byte, 8) == MI355LZ4_E_ARG && said("cstreams_load_dict"));
    CHECK(mi355lz4_cstreams_load_dict(&eng, noSet, 0, byte, 8) == MI355LZ4_E_ARG && said("cstreams_load_dict"));
    CHECK(mi355lz4_compress_dict_device(nullptr, noSet, 0, byte, off, len, 0, 16, 1, 1, 8, byte, 64, res) == MI355LZ4_E_ARG &&
          said("compress_dict_device"));
    CHECK(mi355lz4_compress_dict_device(&eng, noSet, 0, byte, off, len, 0, 16, 1, 1, 8, byte, 64, res) == MI355LZ4_E_ARG);
    size_t outLen = 99;
    CHECK(mi355lz4_compress_dict(nullptr, noSet, 0, ptrs, len, 1, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG &&
          outLen == 0 && said("compress_dict"));
    outLen = 99;
    CHECK(mi355lz4_compress_dict(&eng, noSet, 0, ptrs, len, 1, 1, 8, byte, sizeof(byte), &outLen, nullptr, nullptr) == MI355LZ4_E_ARG &&
          outLen == 0);
    CHECK(mi355lz4_compress_dict(&eng, noSet, 0, ptrs, len, 1, 1, 8, byte, sizeof(byte), nullptr, nullptr, nullptr) == MI355LZ4_E_ARG);

    // ---- mi355lz4_decompress_dict_device: every check lies in front of the first HIP call
    auto dec = [&](mi355lz4_ctx *c, const uint8_t *framed, const uint64_t *bo, int n, int kind, int fixed, const uint8_t *dict,
                   int dictLen, const uint64_t *oo, int32_t *r) {
        return mi355lz4_decompress_dict_device(c, framed, 64, bo, n, kind, fixed, dict, dictLen, byte, oo, nullptr, r);
    };
    CHECK(dec(nullptr, byte, off, 1, 8, 0, byte, 8, off, res) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, byte, off, -1, 8, 0, byte, 8, off, res) == MI355LZ4_E_ARG && said("decompress_dict_device"));
    CHECK(dec(&eng, byte, off, 1, 5, 0, byte, 8, off, res) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, byte, off, 1, 4, -1, byte, 8, off, res) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, byte, off, 1, 8, 0, byte, -1, off, res) == MI355LZ4_E_ARG && said("dictionary"));
    CHECK(dec(&eng, byte, off, 1, 8, 0, nullptr, 8, off, res) == MI355LZ4_E_ARG && said("dictionary"));
    CHECK(dec(&eng, nullptr, off, 1, 8, 0, byte, 8, off, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(dec(&eng, byte, nullptr, 1, 8, 0, byte, 8, off, res) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, byte, off, 1, 8, 0, byte, 8, nullptr, res) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, byte, off, 1, 8, 0, byte, 8, off, nullptr) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, nullptr, nullptr, 0, 8, 0, nullptr, 0, nullptr, nullptr) == MI355LZ4_OK);      // no blocks: nothing to do
    CHECK(dec(&eng, nullptr, nullptr, 0, 8, 0, nullptr, 8, nullptr, nullptr) == MI355LZ4_E_ARG);   // ... but the dictionary is checked
    eng.plan.active = true;                 // a range begun with mi355lz4_decompress_linked_begin is open
    CHECK(dec(&eng, byte, off, 1, 8, 0, byte, 8, off, res) == MI355LZ4_E_ARG && said("still open"));
    eng.plan.active = false;
    CHECK(res[0] == 7 && res[1] == 7);

    // ---- mi355lz4_decompress_dict: the checks, and the host walk of the chain (an empty and a cut one end the call before the device)
    int got = 99;
    outLen = 99;
    CHECK(mi355lz4_decompress_dict(nullptr, byte, 0, 8, 0, byte, 8, byte, 64, &outLen, res, 2, &got) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_decompress_dict(&eng, byte, 0, 8, 0, byte, 8, byte, 64, nullptr, res, 2, &got) == MI355LZ4_E_ARG && said("decompress_dict"));
    CHECK(mi355lz4_decompress_dict(&eng, byte, 0, 8, 0, byte, 8, byte, 64, &outLen, res, 2, nullptr) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_decompress_dict(&eng, byte, 0, 8, 0, byte, 8, byte, 64, &outLen, res, -1, &got) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_decompress_dict(&eng, byte, 0, 5, 0, byte, 8, byte, 64, &outLen, res, 2, &got) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_decompress_dict(&eng, byte, 0, 4, -1, byte, 8, byte, 64, &outLen, res, 2, &got) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_decompress_dict(&eng, byte, 0, 8, 0, byte, -1, byte, 64, &outLen, res, 2, &got) == MI355LZ4_E_ARG && said("dictionary"));
    CHECK(mi355lz4_decompress_dict(&eng, byte, 0, 8, 0, nullptr, 8, byte, 64, &outLen, res, 2, &got) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_decompress_dict(&eng, byte, 0, 8, 0, byte, 8, byte, 64, &outLen, res, 2, &got) == MI355LZ4_OK && outLen == 0 && got == 0);
    std::vector<uint8_t> cut = {100, 0, 0, 0, 50, 0, 0, 0, 1, 2, 3};    // a header that promises 100 bytes, 3 of them there
    got = 99;
    outLen = 99;
    CHECK(mi355lz4_decompress_dict(&eng, cut.data(), cut.size(), 8, 0, byte, 8, byte, 64, &outLen, res, 2, &got) == MI355LZ4_E_STREAM &&
          outLen == 0 && got == 0);
    eng.plan.active = true;
    CHECK(mi355lz4_decompress_dict(&eng, byte, 0, 8, 0, byte, 8, byte, 64, &outLen, res, 2, &got) == MI355LZ4_E_ARG && said("still open"));
    eng.plan.active = false;

    if (failures) return 1;
    std::printf("dict_args_main ok\n");
    return 0;
}
