// cframes_args_main.cpp -- the argument checks of the frame writer (mi355lz4_cframes_bound / _create / _destroy / _reserve /
// _compress, mi355lz4_compress_frames) from a program of its own, built from the host sources with -fsanitize=address,undefined
// against the stubbed launchers (`make asan-cframes`).  No device is needed and none is used: every call here returns before its
// first HIP call -- a launcher reached would abort.  The engine and the far object are plain structs of this program's own
// (engine.hpp), never handed to a device.  (What needs the device -- the codes, the capacity answer of the host form -- is in
// tests/test_cframes_gpu.py.)
#include "../../streamly-lz4_amd/csrc/engine.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
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

static uint64_t bound_by_hand(uint64_t len, int id, unsigned flags)
{
    const uint64_t bmax = (uint64_t)1 << (8 + 2 * id);
    const uint64_t nb = (len + bmax - 1) / bmax;
    return ((flags & 4u) ? 15u : 7u) + nb * ((flags & 2u) ? 8u : 4u) + len + 4u + ((flags & 8u) ? 4u : 0u);
}

int main()
{
    uint8_t byte[64];
    std::memset(byte, 0xA5, sizeof(byte));
    uint64_t off[2] = {0, 0}, len[2] = {0, 0}, cap[2] = {64, 64};
    int64_t res[2] = {7, 7};
    mi355lz4_ctx eng;                       // switches at their defaults, nothing of a device
    mi355lz4_cframes far;                   // an object of another device's engine
    far.device = 5;

    // ---- the bound: the formula, for every block size and flag set, at the lengths around a block's end
    for (int id = 4; id <= 7; id++)
        for (unsigned flags = 0; flags < 16; flags++) {
            const uint64_t bmax = (uint64_t)1 << (8 + 2 * id);
            for (uint64_t n : {(uint64_t)0, (uint64_t)1, bmax - 1, bmax, bmax + 1, 3 * bmax, 3 * bmax + 5, ((uint64_t)1 << 40) + 3})
                CHECK(mi355lz4_cframes_bound(n, id, flags) == bound_by_hand(n, id, flags));
        }
    CHECK(mi355lz4_cframes_bound(100, 3, 0) == 0 && mi355lz4_cframes_bound(100, 8, 0) == 0 && mi355lz4_cframes_bound(100, 4, 16u) == 0);
    CHECK(mi355lz4_cframes_bound(0, 4, 0) == 11 && mi355lz4_cframes_bound(0, 4, 15u) == 23);

    // ---- _create / _destroy
    mi355lz4_cframes *w = &far;
    CHECK(mi355lz4_cframes_create(nullptr, &w) == MI355LZ4_E_ARG && w == nullptr && said("cframes_create"));
    CHECK(mi355lz4_cframes_create(&eng, nullptr) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_cframes_create(&eng, &w) == MI355LZ4_OK && w != nullptr);        // host memory only: nothing of a device yet
    mi355lz4_cframes_destroy(nullptr);      // nothing to do

    // ---- _reserve
    CHECK(mi355lz4_cframes_reserve(nullptr, w, 1, 64, 64, 4) == MI355LZ4_E_ARG && said("cframes_reserve"));
    CHECK(mi355lz4_cframes_reserve(&eng, nullptr, 1, 64, 64, 4) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_cframes_reserve(&eng, &far, 1, 64, 64, 4) == MI355LZ4_E_ARG && said("device 5"));
    CHECK(mi355lz4_cframes_reserve(&eng, w, -1, 64, 64, 4) == MI355LZ4_E_ARG && said("nInputs"));
    for (int id : {3, 8, 0, -1, INT_MAX})
        CHECK(mi355lz4_cframes_reserve(&eng, w, 1, 64, 64, id) == MI355LZ4_E_ARG && said("blockSizeId"));
    CHECK(mi355lz4_cframes_reserve(&eng, w, 1, 64, (uint64_t)INT_MAX << 16, 4) == MI355LZ4_E_ARG && said("block bound"));
    CHECK(mi355lz4_cframes_reserve(&eng, w, INT_MAX / 2 + 1, 64, 64, 4) == MI355LZ4_E_ARG && said("block bound"));      // (the spacers count)
    CHECK(mi355lz4_cframes_reserve(&eng, w, 0, 0, 0, 4) == MI355LZ4_OK);

    // ---- _compress
    auto compress = [&](mi355lz4_ctx *c, mi355lz4_cframes *o, int n, int id, unsigned flags, uint64_t total = 64) {
        return mi355lz4_cframes_compress(c, o, byte, 64, off, len, n, 64, total, id, flags, 1, byte, off, cap, res);
    };
    CHECK(compress(nullptr, w, 1, 4, 0) == MI355LZ4_E_ARG && said("cframes_compress"));
    CHECK(compress(&eng, nullptr, 1, 4, 0) == MI355LZ4_E_ARG);
    CHECK(compress(&eng, &far, 1, 4, 0) == MI355LZ4_E_ARG && said("device 5"));
    for (int n : {-1, INT_MIN})
        CHECK(compress(&eng, w, n, 4, 0) == MI355LZ4_E_ARG && said("nInputs"));
    for (int id : {3, 8, -4})
        CHECK(compress(&eng, w, 1, id, 0) == MI355LZ4_E_ARG && said("blockSizeId"));
    for (unsigned flags : {16u, 32u, 0x80000000u, 31u})
        CHECK(compress(&eng, w, 1, 4, flags) == MI355LZ4_E_ARG && said("flag"));
    CHECK(compress(&eng, w, 1, 4, 0, (uint64_t)INT_MAX << 16) == MI355LZ4_E_ARG && said("block bound"));
    CHECK(compress(&eng, w, INT_MAX - 1, 4, 0, 65536) == MI355LZ4_E_ARG && said("block bound"));
    CHECK(compress(&eng, w, INT_MAX / 2 + 1, 4, 1u) == MI355LZ4_E_ARG && said("block bound"));
    CHECK(mi355lz4_cframes_compress(&eng, w, byte, 64, nullptr, len, 1, 64, 64, 4, 0, 1, byte, off, cap, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_cframes_compress(&eng, w, byte, 64, off, nullptr, 1, 64, 64, 4, 0, 1, byte, off, cap, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_cframes_compress(&eng, w, nullptr, 64, off, len, 1, 64, 64, 4, 0, 1, byte, off, cap, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_cframes_compress(&eng, w, byte, 64, off, len, 1, 64, 64, 4, 0, 1, nullptr, off, cap, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_cframes_compress(&eng, w, byte, 64, off, len, 1, 64, 64, 4, 0, 1, byte, nullptr, cap, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_cframes_compress(&eng, w, byte, 64, off, len, 1, 64, 64, 4, 0, 1, byte, off, nullptr, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_cframes_compress(&eng, w, byte, 64, off, len, 1, 64, 64, 4, 0, 1, byte, off, cap, nullptr) == MI355LZ4_E_ARG && said("null pointer"));
    // no inputs: MI355LZ4_OK, every array may be null, every flag is known
    CHECK(mi355lz4_cframes_compress(&eng, w, nullptr, 0, nullptr, nullptr, 0, 0, 0, 7, 15u, 1, nullptr, nullptr, nullptr, nullptr) == MI355LZ4_OK);
    CHECK(res[0] == 7 && res[1] == 7);

    // ---- mi355lz4_compress_frames
    const uint8_t *in[2] = {byte, nullptr};
    size_t inLen[2] = {8, 3}, outLen = 99;
    uint8_t out[64];
    CHECK(mi355lz4_compress_frames(nullptr, in, inLen, 1, 4, 0, 1, out, 64, &outLen, res) == MI355LZ4_E_ARG && outLen == 0);
    CHECK(mi355lz4_compress_frames(&eng, in, inLen, -1, 4, 0, 1, out, 64, &outLen, res) == MI355LZ4_E_ARG && said("nInputs"));
    CHECK(mi355lz4_compress_frames(&eng, in, inLen, 1, 9, 0, 1, out, 64, &outLen, res) == MI355LZ4_E_ARG && said("blockSizeId"));
    CHECK(mi355lz4_compress_frames(&eng, in, inLen, 1, 4, 16u, 1, out, 64, &outLen, res) == MI355LZ4_E_ARG && said("flag"));
    CHECK(mi355lz4_compress_frames(&eng, nullptr, inLen, 1, 4, 0, 1, out, 64, &outLen, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_compress_frames(&eng, in, nullptr, 1, 4, 0, 1, out, 64, &outLen, res) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_compress_frames(&eng, in, inLen, 1, 4, 0, 1, out, 64, nullptr, res) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_compress_frames(&eng, in, inLen, 1, 4, 0, 1, out, 64, &outLen, nullptr) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_compress_frames(&eng, in, inLen, 2, 4, 0, 1, out, 64, &outLen, res) == MI355LZ4_E_ARG && said("input 1 is null"));
    outLen = 99;
    CHECK(mi355lz4_compress_frames(&eng, nullptr, nullptr, 0, 4, 15u, 1, nullptr, 0, &outLen, nullptr) == MI355LZ4_OK && outLen == 0);
    CHECK(mi355lz4_compress_frames(&eng, nullptr, nullptr, 0, 7, 0, 1, nullptr, 0, nullptr, nullptr) == MI355LZ4_OK);
    CHECK(res[0] == 7 && res[1] == 7);

    mi355lz4_cframes_destroy(w);            // it never held device memory: no HIP call
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("cframes_args_main: every argument check holds\n");
    return 0;
}
