// dictset_args_main.cpp -- the argument checks of the dictionary-set calls (mi355lz4_dictset_create / _destroy / _count,
// mi355lz4_compress_fastdict_multi_device, mi355lz4_compress_fastdict_multi, mi355lz4_decompress_dict_multi_device,
// mi355lz4_decompress_dict_multi, and the hook mi355lz4_debug_dictset_last) from a program of its own, built from the host sources
// with -fsanitize=address,undefined against the stubbed launchers (`make asan-dictset`).  No device is needed and none is used:
// every call here returns before its first HIP call -- a launcher reached would abort.  The engine, the dictionaries and the set are
// plain structs of this program's own (engine.hpp), never created on or handed to a device.
#include "../../streamly-lz4_amd/csrc/engine.hpp"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" int mi355lz4_debug_dictset_last(mi355lz4_dictset *ds, int out[2]);   // (a diagnostic hook: not in the public header)

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
    int32_t len[2] = {0, 0}, res[2] = {7, 7}, idx[2] = {0, -1};
    const uint8_t *ptrs[2] = {byte, byte};
    mi355lz4_ctx eng;                       // switches at their defaults (level 0), nothing of a device
    mi355lz4_hcdict hd;                     // device 0 like the engine, no images
    mi355lz4_hcdict far;
    far.device = 5;
    mi355lz4_dictset set;                   // device 0, two members, no table
    set.n = 2;
    mi355lz4_dictset farSet;
    farSet.device = 5;
    farSet.n = 1;

    // ---- mi355lz4_dictset_create / _count / _destroy and the hook
    const mi355lz4_hcdict *two[2] = {&hd, &hd}, *withNull[2] = {&hd, nullptr}, *withFar[2] = {&hd, &far};
    mi355lz4_dictset *out = &set;
    CHECK(mi355lz4_dictset_create(nullptr, two, 2, &out) == MI355LZ4_E_ARG && out == nullptr && said("dictset_create"));
    out = &set;
    CHECK(mi355lz4_dictset_create(&eng, nullptr, 2, &out) == MI355LZ4_E_ARG && out == nullptr);
    CHECK(mi355lz4_dictset_create(&eng, two, 2, nullptr) == MI355LZ4_E_ARG);
    for (int n : {0, -1, 65537, INT_MAX, INT_MIN}) {
        out = &set;
        CHECK(mi355lz4_dictset_create(&eng, two, n, &out) == MI355LZ4_E_ARG && out == nullptr && said("1..65536"));
    }
    CHECK(mi355lz4_dictset_create(&eng, withNull, 2, &out) == MI355LZ4_E_ARG && said("member 1 is null"));
    CHECK(mi355lz4_dictset_create(&eng, withFar, 2, &out) == MI355LZ4_E_ARG && said("device 5"));
    CHECK(mi355lz4_dictset_count(nullptr) == MI355LZ4_E_ARG && said("dictset_count"));
    CHECK(mi355lz4_dictset_count(&set) == 2);
    mi355lz4_dictset_destroy(nullptr);      // nothing to do
    int last[2] = {7, 7};
    CHECK(mi355lz4_debug_dictset_last(nullptr, last) == MI355LZ4_E_ARG && said("debug_dictset_last"));
    CHECK(mi355lz4_debug_dictset_last(&set, nullptr) == MI355LZ4_E_ARG);
    CHECK(last[0] == 7 && last[1] == 7);

    // ---- mi355lz4_compress_fastdict_multi_device: every check lies in front of the first HIP call, the knob read included
    auto enc = [&](mi355lz4_ctx *c, const mi355lz4_dictset *s, const int32_t *di, const uint8_t *src, int maxLen, int n, int kind,
                   uint8_t *slots, size_t stride, int32_t *fl, int accel = 1) {
        return mi355lz4_compress_fastdict_multi_device(c, s, di, src, off, len, 0, maxLen, n, accel, kind, slots, stride, fl);
    };
    setenv("MI355LZ4_FASTDICT_WAVES", "-2", 1);
    CHECK(enc(nullptr, &set, idx, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_fastdict_multi_device"));
    CHECK(enc(&eng, nullptr, idx, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_fastdict_multi_device"));
    CHECK(enc(&eng, &farSet, idx, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("device 5"));
    for (int level : {1, 9, 12, -1}) {
        eng.compLevel = level;
        CHECK(enc(&eng, &set, idx, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("level 0's encoder"));
    }
    eng.compLevel = 0;
    CHECK(enc(&eng, &set, idx, byte, 16, -1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("compress_fastdict_multi_device"));
    CHECK(enc(&eng, &set, idx, byte, 16, 1, 5, byte, 64, res) == MI355LZ4_E_ARG);
    CHECK(enc(&eng, &set, idx, byte, -1, 1, 8, byte, 64, res) == MI355LZ4_E_ARG);
    CHECK(enc(&eng, &set, idx, byte, (4 << 20) + 1, 1, 8, byte, (size_t)8 << 20, res) == MI355LZ4_E_ARG && said("maxBlockLen"));
    CHECK(enc(&eng, &set, nullptr, nullptr, 16, 0, 8, nullptr, 0, nullptr) == MI355LZ4_OK);       // no blocks: nothing to do
    CHECK(enc(&eng, &set, nullptr, nullptr, 16, 0, 8, nullptr, 0, nullptr, -5) == MI355LZ4_OK);   // (any accel: it is clamped)
    CHECK(enc(&eng, &set, nullptr, byte, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("null dictIdx"));
    CHECK(enc(&eng, &set, idx, nullptr, 16, 1, 8, byte, 64, res) == MI355LZ4_E_ARG && said("null src"));
    CHECK(enc(&eng, &set, idx, byte, 16, 1, 8, nullptr, 64, res) == MI355LZ4_E_ARG && said("null output"));
    CHECK(enc(&eng, &set, idx, byte, 16, 1, 8, byte, 64, nullptr) == MI355LZ4_E_ARG && said("null output"));
    CHECK(enc(&eng, &set, idx, byte, 16, 1, 8, byte, 16 + 16 + 8 - 1, res) == MI355LZ4_E_CAPACITY && said("slotStride"));
    eng.blockChecksum = 1;                  // the trailer counts
    CHECK(enc(&eng, &set, idx, byte, 16, 1, 8, byte, 16 + 16 + 8 + 3, res) == MI355LZ4_E_CAPACITY);
    eng.blockChecksum = 0;
    CHECK(res[0] == 7 && res[1] == 7);

    // ---- mi355lz4_compress_fastdict_multi: null arguments, the level, the indices and the lengths are checked on the host
    size_t outLen = 99;
    auto hostEnc = [&](mi355lz4_ctx *c, const mi355lz4_dictset *s, const int32_t *di, int n, int kind, size_t *ol) {
        return mi355lz4_compress_fastdict_multi(c, s, di, ptrs, len, n, 1, kind, byte, sizeof(byte), ol, res, res);
    };
    CHECK(hostEnc(nullptr, &set, idx, 1, 8, &outLen) == MI355LZ4_E_ARG && outLen == 0 && said("compress_fastdict_multi"));
    outLen = 99;
    CHECK(hostEnc(&eng, nullptr, idx, 1, 8, &outLen) == MI355LZ4_E_ARG && outLen == 0);
    CHECK(hostEnc(&eng, nullptr, idx, 1, 8, nullptr) == MI355LZ4_E_ARG);
    eng.compLevel = 3;
    CHECK(hostEnc(&eng, &set, idx, 1, 8, &outLen) == MI355LZ4_E_ARG && said("level 0's encoder"));
    eng.compLevel = 0;
    CHECK(hostEnc(&eng, &set, nullptr, 1, 8, &outLen) == MI355LZ4_E_ARG && said("null dictIdx"));
    for (int32_t bad : {2, -2, INT32_MAX, INT32_MIN}) {
        idx[1] = bad;
        outLen = 99;
        CHECK(hostEnc(&eng, &set, idx, 2, 8, &outLen) == MI355LZ4_E_ARG && said("block 1 names dictionary") && outLen == 0);
    }
    idx[1] = -1;
    len[1] = (4 << 20) + 1;
    CHECK(hostEnc(&eng, &set, idx, 2, 8, &outLen) == MI355LZ4_E_ARG && said("block 1 length") && outLen == 0);
    len[1] = -1;
    CHECK(hostEnc(&eng, &set, idx, 2, 8, &outLen) == MI355LZ4_E_ARG && said("block 1 length"));
    len[1] = 0;
    CHECK(hostEnc(&eng, &set, idx, -1, 8, &outLen) == MI355LZ4_E_ARG);
    CHECK(hostEnc(&eng, &set, idx, 1, 5, &outLen) == MI355LZ4_E_ARG);
    CHECK(hostEnc(&eng, &set, idx, 0, 8, &outLen) == MI355LZ4_OK && outLen == 0);
    CHECK(res[0] == 7 && res[1] == 7);

    // ---- mi355lz4_decompress_dict_multi_device
    auto dec = [&](mi355lz4_ctx *c, const mi355lz4_dictset *s, const int32_t *di, const uint8_t *framed, const uint64_t *bo, int n,
                   int kind, int fixed, const uint64_t *oo, int32_t *r) {
        return mi355lz4_decompress_dict_multi_device(c, framed, sizeof(byte), bo, n, kind, fixed, s, di, byte, oo, nullptr, r);
    };
    CHECK(dec(nullptr, &set, idx, byte, off, 1, 8, 0, off, res) == MI355LZ4_E_ARG && said("decompress_dict_multi_device"));
    CHECK(dec(&eng, nullptr, idx, byte, off, 1, 8, 0, off, res) == MI355LZ4_E_ARG && said("decompress_dict_multi_device"));
    CHECK(dec(&eng, &farSet, idx, byte, off, 1, 8, 0, off, res) == MI355LZ4_E_ARG && said("device 5"));
    eng.plan.active = true;
    CHECK(dec(&eng, &set, idx, byte, off, 1, 8, 0, off, res) == MI355LZ4_E_ARG && said("still open"));
    eng.plan.active = false;
    CHECK(dec(&eng, &set, idx, byte, off, -1, 8, 0, off, res) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, &set, idx, byte, off, 1, 5, 0, off, res) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, &set, idx, byte, off, 1, 4, -1, off, res) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, &set, nullptr, nullptr, nullptr, 0, 8, 0, nullptr, nullptr) == MI355LZ4_OK);  // no blocks: nothing to do
    CHECK(dec(&eng, &set, nullptr, byte, off, 1, 8, 0, off, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(dec(&eng, &set, idx, nullptr, off, 1, 8, 0, off, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(dec(&eng, &set, idx, byte, nullptr, 1, 8, 0, off, res) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, &set, idx, byte, off, 1, 8, 0, nullptr, res) == MI355LZ4_E_ARG);
    CHECK(dec(&eng, &set, idx, byte, off, 1, 8, 0, off, nullptr) == MI355LZ4_E_ARG);
    CHECK(res[0] == 7 && res[1] == 7);

    // ---- mi355lz4_decompress_dict_multi: the chain is walked and the indices are checked on the host
    std::vector<uint8_t> framed;            // two blocks of one literal each: {compLen 2, uncompLen 1, token 0x10, 'A'}
    for (int k = 0; k < 2; k++) {
        const uint8_t blk[10] = {2, 0, 0, 0, 1, 0, 0, 0, 0x10, 0x41};
        framed.insert(framed.end(), blk, blk + 10);
    }
    int got = 99;
    auto hostDec = [&](mi355lz4_ctx *c, const mi355lz4_dictset *s, const int32_t *di, int kind, int fixed, int maxBlocks, size_t *ol, int *nb) {
        return mi355lz4_decompress_dict_multi(c, framed.data(), framed.size(), kind, fixed, s, di, byte, sizeof(byte), ol, res, maxBlocks, nb);
    };
    outLen = 99;
    CHECK(hostDec(nullptr, &set, idx, 8, 0, 2, &outLen, &got) == MI355LZ4_E_ARG && outLen == 0 && got == 0 && said("decompress_dict_multi"));
    CHECK(hostDec(&eng, nullptr, idx, 8, 0, 2, &outLen, &got) == MI355LZ4_E_ARG);
    CHECK(hostDec(&eng, &set, idx, 8, 0, 2, nullptr, &got) == MI355LZ4_E_ARG);
    CHECK(hostDec(&eng, &set, idx, 8, 0, 2, &outLen, nullptr) == MI355LZ4_E_ARG);
    CHECK(hostDec(&eng, &set, idx, 5, 0, 2, &outLen, &got) == MI355LZ4_E_ARG);
    CHECK(hostDec(&eng, &set, idx, 8, -1, 2, &outLen, &got) == MI355LZ4_E_ARG);
    CHECK(hostDec(&eng, &set, idx, 8, 0, -1, &outLen, &got) == MI355LZ4_E_ARG);
    eng.plan.active = true;
    CHECK(hostDec(&eng, &set, idx, 8, 0, 2, &outLen, &got) == MI355LZ4_E_ARG && said("still open"));
    eng.plan.active = false;
    CHECK(hostDec(&eng, &set, nullptr, 8, 0, 2, &outLen, &got) == MI355LZ4_E_ARG && said("null dictIdx"));
    for (int32_t bad : {2, -2, INT32_MAX, INT32_MIN}) {
        idx[1] = bad;
        outLen = 99; got = 99;
        CHECK(hostDec(&eng, &set, idx, 8, 0, 2, &outLen, &got) == MI355LZ4_E_ARG && said("block 1 names dictionary") && outLen == 0 && got == 0);
    }
    idx[1] = -1;
    CHECK(res[0] == 7 && res[1] == 7);
    for (uint8_t b : byte) CHECK(b == 0xA5);

    if (failures) return 1;
    std::printf("dictset_args_main ok\n");
    return 0;
}
