// fastdict_args_main.cpp -- the argument checks of the level-0 calls against a prepared dictionary (mi355lz4_compress_fastdict_device,
// mi355lz4_compress_fastdict, mi355lz4_debug_hcdict_fast_image) from a program of its own, built from the host sources with
// -fsanitize=address,undefined against the stubbed launchers (`make asan-fastdict`).  No device is needed and none is used: every
// call here returns before its first HIP call -- a launcher reached would abort.  The engine and the dictionary object are plain
// structs of this program's own (engine.hpp), never created on or handed to a device.
#include "../../streamly-lz4_amd/csrc/engine.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" int mi355lz4_debug_hcdict_fast_image(mi355lz4_hcdict *hd, uint8_t *bytes);   // (a diagnostic hook: not in the public header)

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
    mi355lz4_ctx eng;                       // switches at their defaults (level 0), nothing of a device
    mi355lz4_hcdict hd;                     // device 0 like the engine, no images
    mi355lz4_hcdict far;
    far.device = 5;

    // ---- the diagnostic hook
    CHECK(mi355lz4_debug_hcdict_fast_image(nullptr, byte) == MI355LZ4_E_ARG && said("debug_hcdict_fast_image"));
    CHECK(mi355lz4_debug_hcdict_fast_image(&hd, nullptr) == MI355LZ4_E_ARG && said("debug_hcdict_fast_image"));

    // ---- mi355lz4_compress_fastdict_device: every check lies in front of the first HIP call, the knob read included
    auto enc = [&](mi355lz4_ctx *c, const mi355lz4_hcdict *h, const uint8_t *src, int maxLen, int n, int kind, uint8_t *slots,
                   size_t stride, int32_t *fl, int accel = 1) {
        return mi355lz4_compress_fastdict_device(c, h, src, off, len, 0, maxLen, n, accel, kind, slots, stride, fl);
    };
    setenv("MI355LZ4_FASTDICT_WAVES", "-2", 1);
    CHECK(enc(nullptr, &hd, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_fastdict_device"));
    CHECK(enc(&eng, nullptr, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_fastdict_device"));
    CHECK(enc(&eng, &far, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("device 5"));
    for (int level : {1, 9, 12, -1}) {
        eng.compLevel = level;
        CHECK(enc(&eng, &hd, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("mi355lz4_compress_hcdict_device"));
    }
    eng.compLevel = 0;
    CHECK(enc(&eng, &hd, byte, 16, -1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_fastdict_device"));
    CHECK(enc(&eng, &hd, byte, 16, 1, 5, byte, 64, res) == MI355LZ4_E_ARG);
    CHECK(enc(&eng, &hd, byte, -1, 1, 8, byte, 64, res) == MI355LZ4_E_ARG);
    CHECK(enc(&eng, &hd, byte, (4 << 20) + 1, 1, 8, byte, (size_t)8 << 20, res) == MI355LZ4_E_ARG && said("maxBlockLen"));
    CHECK(enc(&eng, &hd, nullptr, 16, 0, 8, nullptr, 0, nullptr) == MI355LZ4_OK);                 // no blocks: nothing to do
    CHECK(enc(&eng, &hd, nullptr, 16, 0, 8, nullptr, 0, nullptr, -5) == MI355LZ4_OK);             // (any accel: it is clamped)
    CHECK(enc(&eng, &hd, nullptr, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("null src"));
    CHECK(enc(&eng, &hd, byte, 16, 1, 8, nullptr, 64, res) == MI355LZ4_E_ARG && said("null output"));
    CHECK(enc(&eng, &hd, byte, 16, 1, 8, byte, 64, nullptr) == MI355LZ4_E_ARG && said("null output"));
    CHECK(enc(&eng, &hd, byte, 16, 1, 8, byte, 16 + 16 + 8 - 1, res) == MI355LZ4_E_CAPACITY && said("slotStride"));
    eng.blockChecksum = 1;                  // the trailer counts
    CHECK(enc(&eng, &hd, byte, 16, 1, 8, byte, 16 + 16 + 8 + 3, res) == MI355LZ4_E_CAPACITY);
    eng.blockChecksum = 0;
    CHECK(res[0] == 7 && res[1] == 7);

    // ---- mi355lz4_compress_fastdict: null arguments, the level and the lengths are checked on the host
    size_t outLen = 99;
    CHECK(mi355lz4_compress_fastdict(nullptr, &hd, ptrs, len, 1, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG &&
          outLen == 0 && said("compress_fastdict"));
    outLen = 99;
    CHECK(mi355lz4_compress_fastdict(&eng, nullptr, ptrs, len, 1, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG && outLen == 0);
    CHECK(mi355lz4_compress_fastdict(&eng, nullptr, ptrs, len, 1, 1, 8, byte, sizeof(byte), nullptr, nullptr, nullptr) == MI355LZ4_E_ARG);
    eng.compLevel = 3;
    CHECK(mi355lz4_compress_fastdict(&eng, &hd, ptrs, len, 1, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG &&
          said("mi355lz4_compress_hcdict"));
    eng.compLevel = 0;
    len[1] = (4 << 20) + 1;
    CHECK(mi355lz4_compress_fastdict(&eng, &hd, ptrs, len, 2, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG &&
          said("block 1") && outLen == 0);
    len[1] = -1;
    CHECK(mi355lz4_compress_fastdict(&eng, &hd, ptrs, len, 2, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG && said("block 1"));
    len[1] = 0;
    CHECK(mi355lz4_compress_fastdict(&eng, &hd, ptrs, len, -1, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_compress_fastdict(&eng, &hd, ptrs, len, 1, 1, 5, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_compress_fastdict(&eng, &hd, ptrs, len, 0, 1, 8, byte, sizeof(byte), &outLen, res, res) == MI355LZ4_OK && outLen == 0);
    CHECK(res[0] == 7 && res[1] == 7);
    for (uint8_t b : byte) CHECK(b == 0xA5);

    if (failures) return 1;
    std::printf("fastdict_args_main ok\n");
    return 0;
}
