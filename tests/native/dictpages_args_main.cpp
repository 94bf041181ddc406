// dictpages_args_main.cpp -- the argument checks of the fast fixed-size page calls against a prepared dictionary
// (mi355lz4_compress_pages_fastdict_device, mi355lz4_compress_pages_fastdict) from a program of its own, built from the host sources
// with -fsanitize=address,undefined against the stubbed launchers (`make asan-dictpages`).  They are the fast page calls' checks plus
// the object's: accel takes any value.  No device is needed and none is used: every call here returns before its first HIP call -- a
// launcher reached would abort.  The engine and the dictionary objects are plain structs of this program's own (engine.hpp), never
// created on or handed to a device.
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
    int32_t len[2] = {0, 0}, ps[2] = {16, 16}, res[8] = {7, 7, 7, 7, 7, 7, 7, 7};
    const uint8_t *ptrs[2] = {byte, byte};
    mi355lz4_ctx eng;                       // switches at their defaults (level 0), nothing of a device
    mi355lz4_hcdict hd;                     // device 0 like the engine, no images
    mi355lz4_hcdict far;
    far.device = 5;

    // ---- mi355lz4_compress_pages_fastdict_device: every check lies in front of the first HIP call, the knob read included
    auto dev = [&](mi355lz4_ctx *c, const mi355lz4_hcdict *h, const uint8_t *src, const uint64_t *so, const int32_t *sl, int n,
                   const int32_t *p, int maxPages, int kind, uint8_t *pages, size_t stride, int32_t *a, int32_t *b, int32_t *np,
                   int32_t *cons, int accel = 1) {
        return mi355lz4_compress_pages_fastdict_device(c, h, src, so, sl, n, p, maxPages, accel, kind, pages, stride, a, b, np, cons);
    };
    CHECK(dev(nullptr, &hd, byte, off, len, 1, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG &&
          said("compress_pages_fastdict_device"));
    CHECK(dev(&eng, nullptr, byte, off, len, 1, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG &&
          said("compress_pages_fastdict_device"));
    CHECK(dev(&eng, nullptr, byte, off, len, 0, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);   // (no inputs either)
    CHECK(dev(&eng, &far, byte, off, len, 1, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("device 5"));
    CHECK(dev(&eng, &hd, byte, off, len, -1, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("compress_pages_fastdict_device"));
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 0, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("compress_pages_fastdict_device"));
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, -3, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);
    for (int kind : {-1, 1, 2, 5, 12})
        CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, kind, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, 8, byte, 8, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);        // stride < header + 1
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, 4, byte, 4, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, 0, byte, 0, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);
    CHECK(dev(&eng, &hd, nullptr, nullptr, nullptr, 0, nullptr, 1, 0, nullptr, 1, nullptr, nullptr, nullptr, nullptr) == MI355LZ4_OK);   // no inputs
    CHECK(dev(&eng, &hd, nullptr, off, len, 1, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(dev(&eng, &hd, byte, nullptr, len, 1, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(dev(&eng, &hd, byte, off, nullptr, 1, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);
    CHECK(dev(&eng, &hd, byte, off, len, 1, nullptr, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, 8, nullptr, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, 8, byte, 24, nullptr, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, 8, byte, 24, res, nullptr, res + 4, res + 6) == MI355LZ4_E_ARG);
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, 8, byte, 24, res, res + 2, nullptr, res + 6) == MI355LZ4_E_ARG);
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, 8, byte, 24, res, res + 2, res + 4, nullptr) == MI355LZ4_E_ARG);
    eng.blockChecksum = 1;                  // a checksummed page format is out of scope
    CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("checksum"));
    CHECK(dev(&eng, &hd, byte, off, len, 0, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("checksum"));
    CHECK(mi355lz4_compress_pages_fastdict(&eng, &hd, ptrs, len, 1, 16, 1, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("checksum"));
    eng.blockChecksum = 0;
    eng.compExact = 1; eng.linkedCompress = 1;                         // these switches play no part
    CHECK(dev(&eng, &hd, byte, off, len, 0, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_OK);
    for (int accel : {-7, 0, 1, 65537, 1 << 30})                       // accel is clamped, never refused
        CHECK(dev(&eng, &hd, byte, off, len, 0, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6, accel) == MI355LZ4_OK);
    eng.compExact = 0; eng.linkedCompress = 0;
    for (int level : {1, 9, 12}) {                                     // the wave encoder is level 0's
        eng.compLevel = level;
        CHECK(dev(&eng, &hd, byte, off, len, 1, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("level"));
        CHECK(dev(&eng, &hd, byte, off, len, 0, ps, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("level"));
        CHECK(mi355lz4_compress_pages_fastdict(&eng, &hd, ptrs, len, 1, 16, 1, 1, 8, byte, 24, res, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG && said("level"));
    }
    eng.compLevel = 0;

    // ---- mi355lz4_compress_pages_fastdict: the object, the lengths, pageSize and the stride are checked on the host
    auto host = [&](mi355lz4_ctx *c, const mi355lz4_hcdict *h, const uint8_t *const *src, const int32_t *sl, int n, int pageSize,
                    int maxPages, int kind, uint8_t *pages, size_t stride, int accel = 1) {
        return mi355lz4_compress_pages_fastdict(c, h, src, sl, n, pageSize, maxPages, accel, kind, pages, stride, res, res + 2, res + 4, res + 6);
    };
    CHECK(host(nullptr, &hd, ptrs, len, 1, 16, 1, 8, byte, 24) == MI355LZ4_E_ARG && said("compress_pages_fastdict"));
    CHECK(host(&eng, nullptr, ptrs, len, 1, 16, 1, 8, byte, 24) == MI355LZ4_E_ARG && said("compress_pages_fastdict"));
    CHECK(host(&eng, nullptr, nullptr, nullptr, 0, 16, 1, 8, nullptr, 24) == MI355LZ4_E_ARG);        // (no inputs either)
    CHECK(host(&eng, &hd, ptrs, len, -1, 16, 1, 8, byte, 24) == MI355LZ4_E_ARG && said("compress_pages_fastdict"));
    CHECK(host(&eng, &hd, ptrs, len, 1, 0, 1, 8, byte, 24) == MI355LZ4_E_ARG);                    // pageSize < 1
    CHECK(host(&eng, &hd, ptrs, len, 1, -5, 1, 8, byte, 24) == MI355LZ4_E_ARG);
    CHECK(host(&eng, &hd, ptrs, len, 1, 16, 0, 8, byte, 24) == MI355LZ4_E_ARG);                   // maxPages < 1
    CHECK(host(&eng, &hd, ptrs, len, 1, 16, 1, 3, byte, 24) == MI355LZ4_E_ARG);
    CHECK(host(&eng, &hd, ptrs, len, 1, 16, 1, 8, byte, 23) == MI355LZ4_E_ARG);                   // stride < header + pageSize
    CHECK(host(&eng, &hd, nullptr, nullptr, 0, 16, 1, 8, nullptr, 24) == MI355LZ4_OK);            // no inputs
    CHECK(host(&eng, &hd, nullptr, len, 1, 16, 1, 8, byte, 24) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(host(&eng, &hd, ptrs, nullptr, 1, 16, 1, 8, byte, 24) == MI355LZ4_E_ARG);
    CHECK(host(&eng, &hd, ptrs, len, 1, 16, 1, 8, nullptr, 24) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_compress_pages_fastdict(&eng, &hd, ptrs, len, 1, 16, 1, 1, 8, byte, 24, nullptr, res + 2, res + 4, res + 6) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_compress_pages_fastdict(&eng, &hd, ptrs, len, 1, 16, 1, 1, 8, byte, 24, res, res + 2, res + 4, nullptr) == MI355LZ4_E_ARG);
    len[1] = -1;
    CHECK(host(&eng, &hd, ptrs, len, 2, 16, 1, 8, byte, 24) == MI355LZ4_E_ARG && said("input 1"));
    len[1] = MI355LZ4_MAX_INPUT_SIZE + 1;
    CHECK(host(&eng, &hd, ptrs, len, 2, 16, 1, 8, byte, 24) == MI355LZ4_E_ARG && said("input 1"));
    len[1] = 5;
    ptrs[1] = nullptr;
    CHECK(host(&eng, &hd, ptrs, len, 2, 16, 1, 8, byte, 24) == MI355LZ4_E_ARG && said("input 1"));
    for (int32_t r : res) CHECK(r == 7);
    for (uint8_t b : byte) CHECK(b == 0xA5);

    if (failures) return 1;
    std::printf("dictpages_args_main ok\n");
    return 0;
}
