// encode_exact.hpp -- the reference-exact compress mode (mi355lz4_set_compress_exact).
//
// exact_encode_block restates LZ4_compress_generic_validated for (limitedOutput, byU32, usingExtDict, dictIssue, hash5),
// cbits/lz4.c:851-1240 -- oracle/lz4_oracle.c `compress_extdict` is the spec, statement by statement.  It reads and writes
// the 4096-entry hash table in the reference's order, so its bytes AND the table it leaves are the reference's.
//
// Form: one wavefront per block chain, the table in LDS (16 KiB).  The parse is serial and every lane runs it with the
// same (wave-uniform) values: no divergence, one coalesced load per probe.  The lanes share the data-parallel steps --
// LZ4_count (256 bytes per step), literal copies, length runs, and the table passes of the chain driver (zero, renorm,
// canonicalise, load, store).
//
// Chain driver (k_exact_chain / k_exact_verify / k_exact_finish in kernels/encode.inc): a call's blocks are cut into pieces of
// P blocks.  Piece p > 0 starts R blocks early from a zeroed table (the run-in), records the canonical table it assumed
// at its first block and the canonical table after its last block; a piece is exact when its predecessor is and the two
// tables agree (api.cpp, exact_encode).  Canonical: an entry no position of the next block can use -- below
// start - 65536 after that block's renorm -- reads 0.  Such an entry fails the distance test (`matchIndex + 65535 <
// current`) at every position of that block and every later one, its table slot is rewritten without looking at it,
// and LZ4_renormDictT maps it to 0: two tables equal after canonicalisation give the same bytes and the same canonical
// table from then on.
#pragma once

#include "kernels.h"
#include "lz4_device.hpp"

namespace lz4dev {

#define EXACT_HASHLOG 12
static_assert(EXACT_TABLE == (1 << EXACT_HASHLOG), "kernels.h");

typedef uint32_t exact_u32u __attribute__((aligned(1)));
typedef uint64_t exact_u64u __attribute__((aligned(1)));

__device__ __forceinline__ uint32_t ex_rd32(const uint8_t *p) { return *(const LZ4_GLOBAL exact_u32u *)as_global(p); }
__device__ __forceinline__ uint64_t ex_rd64(const uint8_t *p) { return *(const LZ4_GLOBAL exact_u64u *)as_global(p); }
__device__ __forceinline__ uint32_t ex_rd8(const uint8_t *p) { return *as_global(p); }

// cbits/lz4.c:706-716, little-endian, hashLog 12
__device__ __forceinline__ uint32_t ex_hash5(const uint8_t *p)
{
    return (uint32_t)(((ex_rd64(p) << 24) * 889523592379ULL) >> (64 - EXACT_HASHLOG));
}

__device__ __forceinline__ uint32_t ex_uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// LZ4_count (cbits/lz4.c:603-626): common-prefix length of a[0..) and b[0..), a bounded by lim.  Wave-wide: each step
// compares 256 bytes, 4 per lane; the first lane that sees a difference (or the end) fixes the length.
__device__ __forceinline__ uint32_t ex_common_len(const uint8_t *a, const uint8_t *b, const uint8_t *lim)
{
    const uint32_t total = (lim > a) ? (uint32_t)(lim - a) : 0u;
    const uint32_t lane = (uint32_t)lane_id();
    for (uint32_t done = 0; done < total; done += 4u * LZ4_WAVE) {
        const uint32_t k = done + 4u * lane;
        uint32_t stop = 4;
        if (k + 4u <= total) {
            const uint32_t x = ex_rd32(a + k) ^ ex_rd32(b + k);
            if (x) stop = (uint32_t)__builtin_ctz(x) >> 3;
        } else {
            for (uint32_t j = 0; j < 4; j++)
                if (k + j >= total || ex_rd8(a + k + j) != ex_rd8(b + k + j)) { stop = j; break; }
        }
        const uint64_t m = __ballot(stop < 4);
        if (m) {
            const int first = __builtin_ctzll(m);
            const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)stop, first);
            const uint32_t r = done + 4u * (uint32_t)first + s;
            return r < total ? r : total;
        }
    }
    return total;
}

// `cnt` bytes of 255 at op (a length field's run, cbits/lz4.c:1040-1043, 1127-1133)
__device__ __forceinline__ void ex_fill255(uint8_t *op, uint32_t cnt, bool write)
{
    if (!write) return;
    LZ4_GLOBAL uint8_t *d = as_global(op);
    for (uint32_t i = (uint32_t)lane_id(); i < cnt; i += LZ4_WAVE) d[i] = 255;
}

__device__ __forceinline__ void ex_put(uint8_t *p, uint32_t v, bool write)
{
    if (write && lane_id() == 0) *as_global(p) = (uint8_t)v;
}

// One block of the stream: src[0..n), dictionary = the dictSize bytes that end at dictEnd (only the last 64 KiB are ever
// read: every match lies within 65535 bytes of its position), the table in LDS.  Returns the compressed size, 0 when it
// does not fit in cap (as the reference; with cap = LZ4_compressBound(n) it always fits).  write = false runs the parse
// for its table alone (a run-in block) and stores nothing.  All lanes of the wave call it with the same arguments.
__device__ int exact_encode_block(uint32_t *tab, const uint8_t *src, int n, const uint8_t *dictEnd, const ExactBlock &m,
                                  uint32_t accel, uint8_t *dst, int cap, bool write)
{
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t startIndex = m.start;
    const uint32_t dictSize = m.dictSize;
    const uint32_t prefixIdxLimit = startIndex - dictSize;
    const bool dictSmall = m.dictSmall != 0;
    const uint8_t *dict = dictEnd - dictSize;      // only dereferenced within the last 65536 bytes
    const long mflimitPlusOne = (long)n - LZ4_MFLIMIT + 1;
    const uint8_t *matchlimit = src + n - LZ4_LASTLITERALS;
    uint8_t *op = dst;
    uint8_t *const olimit = dst + cap;
    long ip = 0, anchor = 0;
    uint32_t forwardH, offset = 0;
    const uint8_t *match = nullptr;
    bool matchInDict = false;
    uint32_t token = 0;                             // the open sequence's token byte, stored when its match length is known
    uint8_t *tokenAt = nullptr;

    auto tab_set = [&](uint32_t h, uint32_t v) {
        if (lane == 0) tab[h] = v;                  // one wave's LDS accesses complete in order: later reads see it
    };
    // a literal run behind a new token, cbits/lz4.c:1022-1046 (seq) and 1204-1231 (the last one); false: output full
    auto literals = [&](uint32_t lit, bool seq) -> bool {
        if (!seq && op + lit + 1 + ((lit + 255 - 15) / 255) > olimit) return false;
        tokenAt = op++;
        if (seq && op + lit + (2 + 1 + LZ4_LASTLITERALS) + (lit / 255) > olimit) return false;
        if (lit >= 15) {
            uint32_t rest = lit - 15;
            token = 15u << 4;
            ex_fill255(op, rest / 255, write);
            op += rest / 255;
            ex_put(op++, rest % 255, write);
        } else {
            token = lit << 4;
        }
        if (write) wave_copy_bytes(op, src + anchor, lit);
        op += lit;
        return true;
    };

    if (n < 13) goto last_literals;                 // :921 (LZ4_minLength)

    tab_set(ex_hash5(src), startIndex);             // :924
    ip = 1;
    forwardH = ex_hash5(src + ip);

    for (;;) {
        // ---- search, :956-1014 ----
        {
            long forwardIp = ip;
            uint32_t step = 1;
            uint32_t searchMatchNb = accel << 6;
            for (;;) {
                const uint32_t h = forwardH;
                const uint32_t current = startIndex + (uint32_t)forwardIp;
                const uint32_t matchIndex = ex_uni(tab[h]);
                ip = forwardIp;
                forwardIp += step;
                step = searchMatchNb++ >> 6;
                if (forwardIp > mflimitPlusOne) goto last_literals;        // :969
                if (matchIndex < startIndex) {                              // :985-989
                    match = dict + (matchIndex - prefixIdxLimit);
                    matchInDict = true;
                } else {                                                    // :990-993
                    match = src + (matchIndex - startIndex);
                    matchInDict = false;
                }
                forwardH = ex_hash5(src + forwardIp);                       // :997
                tab_set(h, current);                                        // :998
                if (dictSmall && matchIndex < prefixIdxLimit) continue;     // :1001
                if (matchIndex + LZ4_MAXDIST < current) continue;           // :1003-1006
                if (ex_rd32(match) == ex_rd32(src + ip)) {                  // :1009-1012
                    offset = current - matchIndex;
                    break;
                }
            }
        }
        // ---- catch up, :1019 ----
        {
            const uint8_t *low = matchInDict ? dict : src;
            while (ip > anchor && match > low && ex_rd8(src + ip - 1) == ex_rd8(match - 1)) { ip--; match--; }
        }
        if (!literals((uint32_t)(ip - anchor), true)) return 0;
    next_match:
        // ---- offset, :1065-1068 ----
        ex_put(op, offset & 255u, write);
        ex_put(op + 1, offset >> 8, write);
        op += 2;
        // ---- match length, :1076-1136 ----
        {
            uint32_t mc;
            if (matchInDict) {                                              // :1078-1090
                const uint8_t *limit = src + ip + (dictEnd - match);
                if (limit > matchlimit) limit = matchlimit;
                mc = ex_common_len(src + ip + LZ4_MINMATCH, match + LZ4_MINMATCH, limit);
                ip += (long)mc + LZ4_MINMATCH;
                if (src + ip == limit) {
                    const uint32_t more = ex_common_len(limit, src, matchlimit);
                    mc += more;
                    ip += more;
                }
            } else {                                                        // :1091-1095
                mc = ex_common_len(src + ip + LZ4_MINMATCH, match + LZ4_MINMATCH, matchlimit);
                ip += (long)mc + LZ4_MINMATCH;
            }
            if (op + (1 + LZ4_LASTLITERALS) + (mc + 240) / 255 > olimit) return 0;   // :1097-1121
            if (mc >= 15) {                                                 // :1123-1135
                token += 15;
                mc -= 15;
                ex_fill255(op, mc / 255, write);
                op += mc / 255;
                ex_put(op++, mc % 255, write);
            } else {
                token += mc;
            }
            ex_put(tokenAt, token, write);
        }
        anchor = ip;
        if (ip >= mflimitPlusOne) break;                                    // :1143
        tab_set(ex_hash5(src + ip - 2), startIndex + (uint32_t)(ip - 2));  // :1146
        // ---- immediate re-test at ip, :1159-1196 ----
        {
            const uint32_t h = ex_hash5(src + ip);
            const uint32_t current = startIndex + (uint32_t)ip;
            const uint32_t matchIndex = ex_uni(tab[h]);
            if (matchIndex < startIndex) { match = dict + (matchIndex - prefixIdxLimit); matchInDict = true; }
            else { match = src + (matchIndex - startIndex); matchInDict = false; }
            tab_set(h, current);
            if ((dictSmall ? (matchIndex >= prefixIdxLimit) : true) && (matchIndex + LZ4_MAXDIST >= current) &&
                ex_rd32(match) == ex_rd32(src + ip)) {
                tokenAt = op++;
                token = 0;
                offset = current - matchIndex;
                goto next_match;
            }
        }
        forwardH = ex_hash5(src + (++ip));                                  // :1200
    }

last_literals:                                                              // :1204-1231
    {
        if (!literals((uint32_t)(n - anchor), false)) return 0;
        ex_put(tokenAt, token, write);
    }
    return (int)(op - dst);
}

} // namespace lz4dev
