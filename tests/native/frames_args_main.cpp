// frames_args_main.cpp -- the argument checks of the frame batches (mi355lz4_frames_create / _destroy / _load / _inputs / _blocks /
// _total / _sizes / _get_sizes / _decode, mi355lz4_decompress_frames) from a program of its own, built from the host sources with
// -fsanitize=address,undefined against the stubbed launchers (`make asan-frames`).  No device is needed and none is used: every
// call here returns before its first HIP call -- a launcher reached would abort.  The engine and the far object are plain structs
// of this program's own (engine.hpp), never handed to a device.  (The capacity answer of mi355lz4_decompress_frames comes
// behind a load, which needs the device: tests/test_frames_gpu.py has it.)
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

int main()
{
    uint8_t byte[64];
    std::memset(byte, 0xA5, sizeof(byte));
    uint64_t off[2] = {0, 0}, len[2] = {0, 0};
    int64_t res[2] = {7, 7};
    mi355lz4_ctx eng;                       // switches at their defaults, nothing of a device
    mi355lz4_frames far;                    // an object of another device's engine
    far.device = 5;

    // ---- _create / _destroy and the queries
    mi355lz4_frames *fr = &far;
    CHECK(mi355lz4_frames_create(nullptr, &fr) == MI355LZ4_E_ARG && fr == nullptr && said("frames_create"));
    CHECK(mi355lz4_frames_create(&eng, nullptr) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_frames_create(&eng, &fr) == MI355LZ4_OK && fr != nullptr);      // host memory only: nothing of a device yet
    mi355lz4_frames_destroy(nullptr);       // nothing to do
    CHECK(mi355lz4_frames_inputs(nullptr) == MI355LZ4_E_ARG && said("frames_inputs"));
    CHECK(mi355lz4_frames_inputs(fr) == MI355LZ4_E_ARG);                            // nothing loaded
    CHECK(mi355lz4_frames_blocks(nullptr) == MI355LZ4_E_ARG && mi355lz4_frames_blocks(fr) == MI355LZ4_E_ARG && said("frames_blocks"));
    CHECK(mi355lz4_frames_total(nullptr) == 0 && mi355lz4_frames_total(fr) == 0);
    CHECK(mi355lz4_frames_sizes(nullptr) == nullptr && mi355lz4_frames_sizes(fr) == nullptr);
    CHECK(mi355lz4_frames_get_sizes(nullptr, res) == MI355LZ4_E_ARG && mi355lz4_frames_get_sizes(fr, res) == MI355LZ4_E_ARG);

    // ---- _decode before any _load
    CHECK(mi355lz4_frames_decode(&eng, fr, byte, off, res) == MI355LZ4_E_ARG && said("nothing is loaded"));

    // ---- _load
    CHECK(mi355lz4_frames_load(nullptr, fr, byte, 64, off, len, 1, 0) == MI355LZ4_E_ARG && said("frames_load"));
    CHECK(mi355lz4_frames_load(&eng, nullptr, byte, 64, off, len, 1, 0) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_frames_load(&eng, &far, byte, 64, off, len, 1, 0) == MI355LZ4_E_ARG && said("device 5"));
    for (int n : {-1, INT_MIN})
        CHECK(mi355lz4_frames_load(&eng, fr, byte, 64, off, len, n, 0) == MI355LZ4_E_ARG && said("nInputs"));
    for (unsigned flags : {4u, 8u, 0x80000000u, 7u})
        CHECK(mi355lz4_frames_load(&eng, fr, byte, 64, off, len, 1, flags) == MI355LZ4_E_ARG && said("flag"));
    CHECK(mi355lz4_frames_load(&eng, fr, byte, 64, nullptr, len, 1, 0) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_frames_load(&eng, fr, byte, 64, off, nullptr, 1, 0) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_frames_load(&eng, fr, nullptr, 64, off, len, 1, 0) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_frames_inputs(fr) == MI355LZ4_E_ARG);                            // a refused load loads nothing
    // no inputs: MI355LZ4_OK, every array may be null, both flags are known
    CHECK(mi355lz4_frames_load(&eng, fr, nullptr, 0, nullptr, nullptr, 0, 3u) == MI355LZ4_OK);
    CHECK(mi355lz4_frames_inputs(fr) == 0 && mi355lz4_frames_blocks(fr) == 0 && mi355lz4_frames_total(fr) == 0);
    CHECK(mi355lz4_frames_get_sizes(fr, nullptr) == MI355LZ4_OK);

    // ---- _decode
    CHECK(mi355lz4_frames_decode(nullptr, fr, byte, off, res) == MI355LZ4_E_ARG && said("frames_decode"));
    CHECK(mi355lz4_frames_decode(&eng, nullptr, byte, off, res) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_frames_decode(&eng, &far, byte, off, res) == MI355LZ4_E_ARG && said("device 5"));
    CHECK(mi355lz4_frames_decode(&eng, fr, nullptr, nullptr, nullptr) == MI355LZ4_OK);      // no inputs: nothing to do
    CHECK(res[0] == 7 && res[1] == 7);

    // ---- mi355lz4_decompress_frames
    const uint8_t *in[2] = {byte, nullptr};
    size_t inLen[2] = {8, 3}, outLen = 99;
    uint8_t out[16];
    CHECK(mi355lz4_decompress_frames(nullptr, in, inLen, 1, 0, out, 16, &outLen, res) == MI355LZ4_E_ARG && outLen == 0);
    CHECK(mi355lz4_decompress_frames(&eng, in, inLen, -1, 0, out, 16, &outLen, res) == MI355LZ4_E_ARG && said("nInputs"));
    CHECK(mi355lz4_decompress_frames(&eng, in, inLen, 1, 4u, out, 16, &outLen, res) == MI355LZ4_E_ARG && said("flag"));
    CHECK(mi355lz4_decompress_frames(&eng, nullptr, inLen, 1, 0, out, 16, &outLen, res) == MI355LZ4_E_ARG && said("null pointer"));
    CHECK(mi355lz4_decompress_frames(&eng, in, nullptr, 1, 0, out, 16, &outLen, res) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_decompress_frames(&eng, in, inLen, 1, 0, out, 16, nullptr, res) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_decompress_frames(&eng, in, inLen, 1, 0, out, 16, &outLen, nullptr) == MI355LZ4_E_ARG);
    CHECK(mi355lz4_decompress_frames(&eng, in, inLen, 2, 0, out, 16, &outLen, res) == MI355LZ4_E_ARG && said("input 1 is null"));
    outLen = 99;
    CHECK(mi355lz4_decompress_frames(&eng, nullptr, nullptr, 0, 3u, nullptr, 0, &outLen, nullptr) == MI355LZ4_OK && outLen == 0);
    CHECK(mi355lz4_decompress_frames(&eng, nullptr, nullptr, 0, 0, nullptr, 0, nullptr, nullptr) == MI355LZ4_OK);
    CHECK(res[0] == 7 && res[1] == 7);

    mi355lz4_frames_destroy(fr);            // it never held device memory: no HIP call
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("frames_args_main: every argument check holds\n");
    return 0;
}
