// hstreams_args_main.cpp -- the level of a set of fast linked streams (mi355lz4_fstreams_set_level / _get_level) and what it does
// to the argument checks of mi355lz4_compress_streams_fast_device and mi355lz4_compress_streams_fast, from a program of its own,
// built from the host sources with -fsanitize=address,undefined against the stubbed launchers (`make asan-hstreams`).  No device
// is needed and none is used.  The engine and the sets are plain structs of this program's own (engine.hpp), never created on or
// handed to a device.
//
// How far a call at set level 9 comes: both forms make their first HIP call, hipSetDevice, behind their last argument check and in
// front of the stream table's upload and the launch.  So that the program says the same with and without a card, the engine and
// the set name a device ordinal no machine has: the call passes every check, fails there with MI355LZ4_E_HIP, and the stubbed
// launcher (san_stubs_hstreams.cpp counts its calls) is not reached.  Reaching it takes a device: tests/test_hstreams_gpu.py.
#include "../../streamly-lz4_amd/csrc/engine.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

extern int san_hstreams_launches;           // (san_stubs_hstreams.cpp)

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
    const int NO_SUCH_DEVICE = 1 << 20;
    uint8_t byte[64], outBuf[256];
    std::memset(byte, 0xA5, sizeof(byte));
    std::memset(outBuf, 0x5A, sizeof(outBuf));
    uint64_t off[2] = {0, 16};
    int32_t len[2] = {16, 16}, res[2] = {7, 7};
    const uint8_t *ptrs[2] = {byte, byte + 16};
    mi355lz4_ctx eng;                       // switches at their defaults (level 0), nothing of a device
    eng.device = NO_SUCH_DEVICE;
    mi355lz4_fstreams set;                  // four slots, no state
    set.device = NO_SUCH_DEVICE;
    set.nSlots = 4;

    // ---- the attribute: default, range, null set; nothing of a device
    CHECK(mi355lz4_fstreams_get_level(&set) == 0);
    for (int level = 0; level <= 12; level++)
        CHECK(mi355lz4_fstreams_set_level(&set, level) == MI355LZ4_OK && mi355lz4_fstreams_get_level(&set) == level);
    CHECK(mi355lz4_fstreams_set_level(&set, 9) == MI355LZ4_OK);
    for (int bad : {13, -1, INT_MAX, INT_MIN}) {
        CHECK(mi355lz4_fstreams_set_level(&set, bad) == MI355LZ4_E_ARG && said("fstreams_set_level") && said("0..12"));
        CHECK(mi355lz4_fstreams_get_level(&set) == 9);          // unchanged
    }
    CHECK(mi355lz4_fstreams_set_level(nullptr, 3) == MI355LZ4_E_ARG && said("fstreams_set_level"));
    CHECK(mi355lz4_fstreams_get_level(nullptr) == MI355LZ4_E_ARG && said("fstreams_get_level"));
    CHECK(mi355lz4_fstreams_get_level(&set) == 9);
    CHECK(mi355lz4_fstreams_set_level(&set, 0) == MI355LZ4_OK && mi355lz4_fstreams_get_level(&set) == 0);

    int32_t first[3] = {0, 1, 2}, slot[2] = {0, 1};
    auto enc = [&](int accel) {
        return mi355lz4_compress_streams_fast_device(&eng, &set, byte, off, len, 0, 16, 2, first, slot, 2, accel, 8, outBuf, 64, res);
    };
    size_t outLen = 99;
    auto hostEnc = [&]() {
        return mi355lz4_compress_streams_fast(&eng, &set, ptrs, len, 2, first, slot, 2, 1, 8, outBuf, sizeof(outBuf), &outLen, res, res);
    };

    // ---- set level 9, engine level 0: both forms pass every argument check (any accel: the level ignores it) and end at the
    // first HIP call; at set level 0 they do the same
    setenv("MI355LZ4_HSTREAMS_GROUPS", "-3", 1);
    for (int setLevel : {9, 12, 1, 0}) {
        CHECK(mi355lz4_fstreams_set_level(&set, setLevel) == MI355LZ4_OK);
        for (int accel : {1, 0, -5, 70000}) CHECK(enc(accel) == MI355LZ4_E_HIP && said("hipSetDevice"));
        outLen = 99;
        CHECK(hostEnc() == MI355LZ4_E_HIP && said("hipSetDevice") && outLen == 0);
    }
    CHECK(san_hstreams_launches == 0);      // (no device: see the head of the file)

    // ---- engine level 1, 9 or 12: refused with the level-0 message whatever the set's level is
    for (int setLevel : {0, 3, 9, 12})
        for (int level : {1, 9, 12, -1}) {
            CHECK(mi355lz4_fstreams_set_level(&set, setLevel) == MI355LZ4_OK);
            eng.compLevel = level;
            CHECK(enc(1) == MI355LZ4_E_ARG && said("compress_streams_fast_device: compression level") && said("fast streams are level 0's encoder"));
            outLen = 99;
            CHECK(hostEnc() == MI355LZ4_E_ARG && said("compress_streams_fast: compression level") && said("fast streams are level 0's encoder") && outLen == 0);
            CHECK(mi355lz4_fstreams_get_level(&set) == setLevel);
        }
    eng.compLevel = 0;

    // ---- at set level 9 the other argument checks are level 0's
    CHECK(mi355lz4_fstreams_set_level(&set, 9) == MI355LZ4_OK);
    int32_t twice[2] = {3, 3}, down[3] = {0, 3, 2};
    CHECK(mi355lz4_compress_streams_fast_device(&eng, &set, byte, off, len, 0, 16, 2, first, twice, 2, 1, 8, outBuf, 64, res) == MI355LZ4_E_ARG && said("named twice"));
    CHECK(mi355lz4_compress_streams_fast_device(&eng, &set, byte, off, len, 0, 16, 2, down, slot, 2, 1, 8, outBuf, 64, res) == MI355LZ4_E_ARG && said("not ascending"));
    CHECK(mi355lz4_compress_streams_fast_device(&eng, &set, byte, off, len, 0, (4 << 20) + 1, 2, first, slot, 2, 1, 8, outBuf, (size_t)8 << 20, res) == MI355LZ4_E_ARG && said("maxBlockLen"));
    CHECK(mi355lz4_compress_streams_fast_device(&eng, &set, nullptr, off, len, 0, 16, 2, first, slot, 2, 1, 8, outBuf, 64, res) == MI355LZ4_E_ARG && said("null src"));
    CHECK(mi355lz4_compress_streams_fast_device(&eng, &set, byte, off, len, 0, 16, 2, first, slot, 2, 1, 8, outBuf, 16 + 16 + 8 - 1, res) == MI355LZ4_E_CAPACITY);
    int32_t none[1] = {0};
    CHECK(mi355lz4_compress_streams_fast_device(&eng, &set, nullptr, nullptr, nullptr, 0, 16, 0, none, nullptr, 0, 1, 8, nullptr, 0, nullptr) == MI355LZ4_OK);
    len[1] = -1;
    outLen = 99;
    CHECK(hostEnc() == MI355LZ4_E_ARG && said("block 1 length") && outLen == 0);
    len[1] = 16;

    CHECK(res[0] == 7 && res[1] == 7);
    for (uint8_t b : byte) CHECK(b == 0xA5);
    for (uint8_t b : outBuf) CHECK(b == 0x5A);
    CHECK(san_hstreams_launches == 0);

    if (failures) return 1;
    std::printf("hstreams_args_main ok\n");
    return 0;
}
