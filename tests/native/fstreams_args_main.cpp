// fstreams_args_main.cpp -- the argument checks of the fast linked streams (mi355lz4_fstreams_create / _destroy / _count / _reset /
// _set_dict, mi355lz4_compress_streams_fast_device, mi355lz4_compress_streams_fast, and the hook mi355lz4_debug_fstreams_peek) from a
// program of its own, built from the host sources with -fsanitize=address,undefined against the stubbed launchers
// (`make asan-fstreams`).  No device is needed and none is used: every call here returns before its first HIP call -- a launcher
// reached would abort.  The engine and the sets are plain structs of this program's own (engine.hpp), never created on or handed
// to a device.
#include "../../streamly-lz4_amd/csrc/engine.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" int mi355lz4_debug_fstreams_peek(mi355lz4_fstreams *fs, int slot, uint8_t *hostBytes65536, int *count);   // (a hook: not in the public header)

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
    uint64_t off[4] = {0, 0, 0, 0};
    int32_t len[4] = {0, 0, 0, 0}, res[4] = {7, 7, 7, 7};
    const uint8_t *ptrs[4] = {byte, byte, byte, byte};
    mi355lz4_ctx eng;                       // switches at their defaults (level 0), nothing of a device
    mi355lz4_fstreams set;                  // device 0, four slots, no state
    set.nSlots = 4;
    mi355lz4_fstreams farSet;
    farSet.device = 5;
    farSet.nSlots = 4;

    // ---- the set: create, count, destroy, reset, set_dict, the hook
    mi355lz4_fstreams *out = &set;
    CHECK(mi355lz4_fstreams_create(nullptr, 4, &out) == MI355LZ4_E_ARG && out == nullptr && said("fstreams_create"));
    CHECK(mi355lz4_fstreams_create(&eng, 4, nullptr) == MI355LZ4_E_ARG);
    for (int n : {0, -1, INT_MIN}) {
        out = &set;
        CHECK(mi355lz4_fstreams_create(&eng, n, &out) == MI355LZ4_E_ARG && out == nullptr);
    }
    CHECK(mi355lz4_fstreams_count(nullptr) == MI355LZ4_E_ARG && said("fstreams_count"));
    CHECK(mi355lz4_fstreams_count(&set) == 4);
    mi355lz4_fstreams_destroy(nullptr);     // nothing to do
    int32_t one[1] = {0};
    CHECK(mi355lz4_fstreams_reset(nullptr, &set, one, 1) == MI355LZ4_E_ARG && said("fstreams_reset"));
    CHECK(mi355lz4_fstreams_reset(&eng, nullptr, one, 1) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_fstreams_reset(&eng, &farSet, one, 1) == MI355LZ4_E_ARG && said("device 5"));
    CHECK(mi355lz4_fstreams_set_dict(nullptr, &set, 0, byte, 8) == MI355LZ4_E_ARG && said("fstreams_set_dict"));
    CHECK(mi355lz4_fstreams_set_dict(&eng, nullptr, 0, byte, 8) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_fstreams_set_dict(&eng, &farSet, 0, byte, 8) == MI355LZ4_E_ARG && said("device 5"));
    for (int slot : {-1, 4, INT_MAX, INT_MIN})
        CHECK(mi355lz4_fstreams_set_dict(&eng, &set, slot, byte, 8) == MI355LZ4_E_ARG && said("of 4"));
    CHECK(mi355lz4_fstreams_set_dict(&eng, &set, 0, byte, -1) == MI355LZ4_E_ARG && said("bad dictionary"));
    CHECK(mi355lz4_fstreams_set_dict(&eng, &set, 0, nullptr, 8) == MI355LZ4_E_ARG && said("bad dictionary"));
    int count = 7;
    CHECK(mi355lz4_debug_fstreams_peek(nullptr, 0, byte, &count) == MI355LZ4_E_ARG && said("debug_fstreams_peek"));
    for (int slot : {-1, 4, INT_MAX})
        CHECK(mi355lz4_debug_fstreams_peek(&set, slot, byte, &count) == MI355LZ4_E_ARG);
    CHECK(count == 7);

    // ---- mi355lz4_compress_streams_fast_device: every check lies in front of the first HIP call, the knob read included
    int32_t first[3] = {0, 1, 2}, slot[2] = {0, 1};
    auto enc = [&](mi355lz4_ctx *c, mi355lz4_fstreams *s, const uint8_t *src, int maxLen, int n, const int32_t *sf, const int32_t *sl,
                   int ns, int kind, uint8_t *slots, size_t stride, int32_t *fl, int accel = 1) {
        return mi355lz4_compress_streams_fast_device(c, s, src, off, len, 0, maxLen, n, sf, sl, ns, accel, kind, slots, stride, fl);
    };
    setenv("MI355LZ4_FSTREAMS_WAVES", "-2", 1);
    CHECK(enc(nullptr, &set, byte, 16, 2, first, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_streams_fast_device"));
    CHECK(enc(&eng, nullptr, byte, 16, 2, first, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_streams_fast_device"));
    CHECK(enc(&eng, &farSet, byte, 16, 2, first, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("device 5"));
    for (int level : {1, 9, 12, -1}) {
        eng.compLevel = level;
        CHECK(enc(&eng, &set, byte, 16, 2, first, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("fast streams are level 0's encoder"));
    }
    eng.compLevel = 0;
    // the stream table
    CHECK(enc(&eng, &set, byte, 16, -1, first, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("bad stream table"));
    CHECK(enc(&eng, &set, byte, 16, 2, first, slot, -1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("bad stream table"));
    CHECK(enc(&eng, &set, byte, 16, 2, nullptr, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("bad stream table"));
    CHECK(enc(&eng, &set, byte, 16, 2, first, nullptr, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("bad stream table"));
    CHECK(enc(&eng, &set, byte, 16, 3, first, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("do not cover"));
    int32_t from1[3] = {1, 1, 2};
    CHECK(enc(&eng, &set, byte, 16, 2, from1, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("do not cover"));
    int32_t down[3] = {0, 3, 2};
    CHECK(enc(&eng, &set, byte, 16, 2, down, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("not ascending"));
    for (int32_t bad : {-1, 4, INT32_MAX, INT32_MIN}) {
        int32_t sl[2] = {0, bad};
        CHECK(enc(&eng, &set, byte, 16, 2, first, sl, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("names slot"));
    }
    int32_t twice[2] = {3, 3};
    CHECK(enc(&eng, &set, byte, 16, 2, first, twice, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("named twice"));
    // the blocks and the buffers
    CHECK(enc(&eng, &set, byte, 16, 2, first, slot, 2, 5, byte, 64, res) == MI355LZ4_E_ARG);
    CHECK(enc(&eng, &set, byte, -1, 2, first, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG);
    CHECK(enc(&eng, &set, byte, (4 << 20) + 1, 2, first, slot, 2, 8, byte, (size_t)8 << 20, res) == MI355LZ4_E_ARG && said("maxBlockLen"));
    int32_t none[1] = {0};
    CHECK(enc(&eng, &set, nullptr, 16, 0, none, nullptr, 0, 8, nullptr, 0, nullptr) == MI355LZ4_OK);        // no blocks: nothing to do
    CHECK(enc(&eng, &set, nullptr, 16, 0, none, nullptr, 0, 8, nullptr, 0, nullptr, -5) == MI355LZ4_OK);    // (any accel: it is clamped)
    int32_t empty[3] = {0, 0, 0};
    CHECK(enc(&eng, &set, nullptr, 16, 0, empty, slot, 2, 8, nullptr, 0, nullptr) == MI355LZ4_OK);          // two empty streams
    CHECK(enc(&eng, &set, nullptr, 16, 2, first, slot, 2, 8, byte, 64, res) == MI355LZ4_E_ARG && said("null src"));
    CHECK(enc(&eng, &set, byte, 16, 2, first, slot, 2, 8, nullptr, 64, res) == MI355LZ4_E_ARG && said("null output"));
    CHECK(enc(&eng, &set, byte, 16, 2, first, slot, 2, 8, byte, 64, nullptr) == MI355LZ4_E_ARG && said("null output"));
    CHECK(enc(&eng, &set, byte, 16, 2, first, slot, 2, 8, byte, 16 + 16 + 8 - 1, res) == MI355LZ4_E_CAPACITY && said("slotStride"));
    eng.blockChecksum = 1;                  // the trailer counts
    CHECK(enc(&eng, &set, byte, 16, 2, first, slot, 2, 8, byte, 16 + 16 + 8 + 3, res) == MI355LZ4_E_CAPACITY);
    eng.blockChecksum = 0;
    CHECK(res[0] == 7 && res[1] == 7);

    // ---- mi355lz4_compress_streams_fast: the table, the level and the lengths are checked on the host, nothing is enqueued
    size_t outLen = 99;
    auto hostEnc = [&](mi355lz4_ctx *c, mi355lz4_fstreams *s, int n, const int32_t *sf, const int32_t *sl, int ns, int kind, size_t *ol) {
        return mi355lz4_compress_streams_fast(c, s, ptrs, len, n, sf, sl, ns, 1, kind, byte, sizeof(byte), ol, res, res);
    };
    CHECK(hostEnc(nullptr, &set, 2, first, slot, 2, 8, &outLen) == MI355LZ4_E_ARG && outLen == 0 && said("compress_streams_fast"));
    outLen = 99;
    CHECK(hostEnc(&eng, nullptr, 2, first, slot, 2, 8, &outLen) == MI355LZ4_E_ARG && outLen == 0);
    CHECK(hostEnc(&eng, nullptr, 2, first, slot, 2, 8, nullptr) == MI355LZ4_E_ARG);
    CHECK(hostEnc(&eng, &farSet, 2, first, slot, 2, 8, &outLen) == MI355LZ4_E_ARG && said("device 5"));
    eng.compLevel = 3;
    CHECK(hostEnc(&eng, &set, 2, first, slot, 2, 8, &outLen) == MI355LZ4_E_ARG && said("level 0's encoder"));
    eng.compLevel = 0;
    CHECK(hostEnc(&eng, &set, 2, down, slot, 2, 8, &outLen) == MI355LZ4_E_ARG && said("not ascending"));
    CHECK(hostEnc(&eng, &set, 2, first, twice, 2, 8, &outLen) == MI355LZ4_E_ARG && said("named twice"));
    CHECK(hostEnc(&eng, &set, 3, first, slot, 2, 8, &outLen) == MI355LZ4_E_ARG && said("do not cover"));
    len[1] = (4 << 20) + 1;
    outLen = 99;
    CHECK(hostEnc(&eng, &set, 2, first, slot, 2, 8, &outLen) == MI355LZ4_E_ARG && said("block 1 length") && outLen == 0);
    len[1] = -1;
    CHECK(hostEnc(&eng, &set, 2, first, slot, 2, 8, &outLen) == MI355LZ4_E_ARG && said("block 1 length"));
    len[1] = 0;
    CHECK(hostEnc(&eng, &set, 2, first, slot, 2, 5, &outLen) == MI355LZ4_E_ARG);
    CHECK(hostEnc(&eng, &set, 0, none, nullptr, 0, 8, &outLen) == MI355LZ4_OK && outLen == 0);
    CHECK(res[0] == 7 && res[1] == 7);
    for (uint8_t b : byte) CHECK(b == 0xA5);

    if (failures) return 1;
    std::printf("fstreams_args_main ok\n");
    return 0;
}
