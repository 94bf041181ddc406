// checksum.hpp -- xxHash32 of many byte ranges at once on gfx950: the block checksums of the LZ4 block format
// (reference src/Streamly/Internal/LZ4/Config.hs:118-158, "Checksum (4 byte, optional)"; the LZ4 frame format's
// B.Checksum: xxh32, seed 0, over a block's compressed bytes, little-endian).
//
// Within a range xxh32 is four serial chains, v_j = rotl(v_j + w * P2, 13) * P1 over word j of every 16-byte stripe, so
// the only parallelism is across ranges.  Four lanes own a range, lane j its accumulator j; a wave holds 16 ranges.
// Each step a lane reads word j of XXH_AHEAD consecutive stripes (dword loads at +0, +16, ...: the range's group of
// lanes touches 16 contiguous bytes per load, 256 per step, instead of 64 scattered lanes), and the next step's words
// are in flight while this step's chain runs.  v_mul_lo_u32 issues at the rate of any other
// VOP3 instruction on gfx950 (profiles/r06_valu_issue_rate.txt: 4.4 cycles per wave-instruction at 4 waves/SIMD, as
// v_add3_u32), so the chain uses the plain multiply.  The four accumulators meet in lane 0 of the group, which hashes
// the tail (< 16 bytes) and finishes.  Global loads may be byte-misaligned (unaligned_load: no extra cost
// when coalesced), so any offset is read directly.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#define XXH_P1 2654435761u
#define XXH_P2 2246822519u
#define XXH_P3 3266489917u
#define XXH_P4 668265263u
#define XXH_P5 374761393u
// stripes whose words a lane has in flight while it hashes the ones before them: a range's chain is bound by the
// latency of its loads otherwise (measured: 64 bytes ahead cost 59 ns per 16 bytes on one range)
#define XXH_AHEAD 16

namespace lz4dev {

__device__ __forceinline__ uint32_t xxh_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

__device__ __forceinline__ uint32_t xxh_round(uint32_t v, uint32_t w) { return xxh_rotl(v + w * XXH_P2, 13) * XXH_P1; }

// one unaligned little-endian word of global memory
__device__ __forceinline__ uint32_t xxh_word(const uint8_t *p)
{
    typedef uint32_t __attribute__((aligned(1))) u32u;
    return *(const LZ4_GLOBAL u32u *)p;
}

// xxh32(seed) of [p, p + len), computed by the four lanes q = 0..3 of a group (every lane calls it with the same
// p / len / seed; len < 0: the group has no range).  The result is valid in the group's lane 0.
__device__ __forceinline__ uint32_t xxh32_group(const uint8_t *p, int64_t len, uint32_t seed, int q)
{
    const int64_t stripes = len >= 16 ? len / 16 : 0;
    uint32_t v = seed + (q == 0 ? XXH_P1 + XXH_P2 : q == 1 ? XXH_P2 : q == 2 ? 0u : 0u - XXH_P1);
    const uint8_t *w = p + 4 * q;
    int64_t s = 0;
    if (stripes >= XXH_AHEAD) {
        uint32_t a[XXH_AHEAD];
#pragma unroll
        for (int k = 0; k < XXH_AHEAD; k++) a[k] = xxh_word(w + 16 * k);
        for (s = XXH_AHEAD; s + XXH_AHEAD <= stripes; s += XXH_AHEAD) {
            uint32_t b[XXH_AHEAD];
#pragma unroll
            for (int k = 0; k < XXH_AHEAD; k++) b[k] = xxh_word(w + 16 * (s + k));
#pragma unroll
            for (int k = 0; k < XXH_AHEAD; k++) { v = xxh_round(v, a[k]); a[k] = b[k]; }
        }
#pragma unroll
        for (int k = 0; k < XXH_AHEAD; k++) v = xxh_round(v, a[k]);
    }
    for (; s + 4 <= stripes; s += 4) {
        const uint32_t b0 = xxh_word(w + 16 * s), b1 = xxh_word(w + 16 * (s + 1)), b2 = xxh_word(w + 16 * (s + 2)),
                       b3 = xxh_word(w + 16 * (s + 3));
        v = xxh_round(v, b0); v = xxh_round(v, b1); v = xxh_round(v, b2); v = xxh_round(v, b3);
    }
    for (; s < stripes; s++) v = xxh_round(v, xxh_word(w + 16 * s));
    // the four accumulators to lane 0 of the group
    const int base = (int)(__lane_id() & ~3u);
    const uint32_t v1 = __shfl(v, base), v2 = __shfl(v, base + 1), v3 = __shfl(v, base + 2), v4 = __shfl(v, base + 3);
    uint32_t h = stripes ? xxh_rotl(v1, 1) + xxh_rotl(v2, 7) + xxh_rotl(v3, 12) + xxh_rotl(v4, 18) : seed + XXH_P5;
    if (q != 0 || len < 0) return h;
    h += (uint32_t)len;
    const uint8_t *t = p + 16 * stripes;
    const uint8_t *e = p + len;
    for (; t + 4 <= e; t += 4) h = xxh_rotl(h + xxh_word(t) * XXH_P3, 17) * XXH_P4;
    for (; t < e; t++) h = xxh_rotl(h + (uint32_t)*(const LZ4_GLOBAL uint8_t *)t * XXH_P5, 11) * XXH_P1;
    h ^= h >> 15; h *= XXH_P2;
    h ^= h >> 13; h *= XXH_P3;
    h ^= h >> 16;
    return h;
}

}  // namespace lz4dev
