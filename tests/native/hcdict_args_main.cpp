// hcdict_args_main.cpp -- the argument checks of the high-compression dictionary calls (mi355lz4_hcdict_create, _load, _size,
// mi355lz4_compress_hcdict_device, mi355lz4_compress_hcdict) from a program of its own, built from the host sources with
// -fsanitize=address,undefined against the stubbed launchers (`make asan-hcdict`).  No device is needed and none is used: every
// call here returns before its first HIP call -- a launcher reached would abort.  The engine and the dictionary object are plain
// structs of this program's own (engine.hpp), never created on or handed to a device.
#include "../../streamly-lz4_amd/csrc/engine.hpp"

#include <cstdio>
#include <cstring>

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
    uint8_t byte[64];
    std::memset(byte, 0xA5, sizeof(byte));
    uint64_t off[2] = {0, 0};
    int32_t len[2] = {0, 0}, res[2] = {7, 7};
    const uint8_t *ptrs[2] = {byte, byte};
    mi355lz4_ctx eng;                       // switches at their defaults, nothing of a device
    mi355lz4_hcdict hd;                     // device 0 like the engine, no image
    mi355lz4_hcdict far;
    far.device = 5;
    mi355lz4_hcdict *got = &hd;

    // ---- the object
    CHECK(mi355lz4_hcdict_create(nullptr, &got) == MI355LZ4_E_ARG && got == nullptr && said("hcdict_create"));
    CHECK(mi355lz4_hcdict_create(&eng, nullptr) == MI355LZ4_E_ARG && said("hcdict_create"));
    mi355lz4_hcdict_destroy(nullptr);
    CHECK(mi355lz4_hcdict_size(nullptr) == MI355LZ4_E_ARG && said("hcdict_size"));
    CHECK(mi355lz4_hcdict_size(&hd) == 0);
    CHECK(mi355lz4_hcdict_load(nullptr, &hd, byte, 8) == MI355LZ4_E_ARG && said("hcdict_load"));
    CHECK(mi355lz4_hcdict_load(&eng, nullptr, byte, 8) == MI355LZ4_E_ARG && said("hcdict_load"));
    CHECK(mi355lz4_hcdict_load(&eng, &far, byte, 8) == MI355LZ4_E_ARG && said("hcdict_load") && said("device 5"));
    CHECK(mi355lz4_hcdict_load(&eng, &hd, byte, -1) == MI355LZ4_E_ARG && said("bad dictionary"));
    CHECK(mi355lz4_hcdict_load(&eng, &hd, nullptr, 8) == MI355LZ4_E_ARG && said("bad dictionary"));
    CHECK(mi355lz4_hcdict_size(&hd) == 0);

    // ---- mi355lz4_compress_hcdict_device: every check lies in front of the first HIP call
    auto enc = [&](mi355lz4_ctx *c, const mi355lz4_hcdict *h, const uint8_t *src, int maxLen, int n, int kind, uint8_t *slots,
                   size_t stride, int32_t *fl) {
        return mi355lz4_compress_hcdict_device(c, h, src, off, len, 0, maxLen, n, kind, slots, stride, fl);
    };
    eng.compLevel = 9;
    CHECK(enc(nullptr, &hd, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_hcdict_device"));
    CHECK(enc(&eng, nullptr, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_hcdict_device"));
    CHECK(enc(&eng, &far, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("device 5"));
    eng.compLevel = 0;
    CHECK(enc(&eng, &hd, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("mi355lz4_compress_dict_device"));
    eng.compLevel = 3;
    CHECK(enc(&eng, &hd, byte, 16, -1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_hcdict_device"));
    CHECK(enc(&eng, &hd, byte, 16, 1, 5, byte, 64, res) == MI355LZ4_E_ARG);
    CHECK(enc(&eng, &hd, byte, -1, 1, 8, byte, 64, res) == MI355LZ4_E_ARG);
    CHECK(enc(&eng, &hd, byte, (4 << 20) + 1, 1, 8, byte, (size_t)8 << 20, res) == MI355LZ4_E_ARG && said("maxBlockLen"));
    CHECK(enc(&eng, &hd, nullptr, 16, 0, 8, nullptr, 0, nullptr) == MI355LZ4_OK);                 // no blocks: nothing to do
    CHECK(enc(&eng, &hd, nullptr, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("null src"));
    CHECK(enc(&eng, &hd, byte, 16, 1, 8, nullptr, 64, res) == MI355LZ4_E_ARG && said("null output"));
    CHECK(enc(&eng, &hd, byte, 16, 1, 8, byte, 64, nullptr) == MI355LZ4_E_ARG && said("null output"));
    CHECK(enc(&eng, &hd, byte, 16, 1, 8, byte, 16 + 16 + 8 - 1, res) == MI355LZ4_E_CAPACITY && said("slotStride"));
    eng.blockChecksum = 1;                  // the trailer counts
    CHECK(enc(&eng, &hd, byte, 16, 1, 8, byte, 16 + 16 + 8 + 3, res) == MI355LZ4_E_CAPACITY);
    eng.blockChecksum = 0;
    CHECK(res[0] == 7 && res[1] == 7);

    // ---- mi355lz4_compress_hcdict: null arguments, the level and the lengths are checked on the host
    size_t outLen = 99;
    CHECK(mi355lz4_compress_hcdict(nullptr, &hd, ptrs, len, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG &&
          outLen == 0 && said("compress_hcdict"));
    outLen = 99;
    CHECK(mi355lz4_compress_hcdict(&eng, nullptr, ptrs, len, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG && outLen == 0);
    CHECK(mi355lz4_compress_hcdict(&eng, nullptr, ptrs, len, 1, 8, byte, sizeof(byte), nullptr, nullptr, nullptr) == MI355LZ4_E_ARG);
    eng.compLevel = 0;
    CHECK(mi355lz4_compress_hcdict(&eng, &hd, ptrs, len, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG &&
          said("mi355lz4_compress_dict"));
    eng.compLevel = 9;
    len[1] = (4 << 20) + 1;
    CHECK(mi355lz4_compress_hcdict(&eng, &hd, ptrs, len, 2, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG &&
          said("block 1") && outLen == 0);
    len[1] = -1;
    CHECK(mi355lz4_compress_hcdict(&eng, &hd, ptrs, len, 2, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG && said("block 1"));
    len[1] = 0;
    CHECK(mi355lz4_compress_hcdict(&eng, &hd, ptrs, len, -1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_compress_hcdict(&eng, &hd, ptrs, len, 1, 5, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_compress_hcdict(&eng, &hd, ptrs, len, 0, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_OK && outLen == 0);
    CHECK(res[0] == 7 && res[1] == 7);
    for (uint8_t b : byte) CHECK(b == 0xA5);

    if (failures) return 1;
    std::printf("hcdict_args_main ok\n");
    return 0;
}
