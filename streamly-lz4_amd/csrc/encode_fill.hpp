// encode_fill.hpp -- fixed-size output pages (mi355lz4_compress_pages_device): LZ4_compress_destSize on the GPU.
//
// fill_encode_page restates LZ4_compress_generic_validated (cbits/lz4.c:851-1240) for the instances LZ4_compress_destSize
// reaches (cbits/lz4.c:1382-1396): (fillOutput | notLimited, byU16 | byU32, noDict, noDictIssue, acceleration 1), from a
// zeroed table at currentOffset 0.  They differ from the instance encode_exact.hpp restates in what a table entry is --
// a position of this page's source, nothing in front of it -- in byU16's hash (4 bytes, 13 bits, no distance test), and in
// the four fill rules: the literal rewind (:1028-1032), the token rewind (:1057-1062), the shortened match (:1097-1117) and the
// adapted last run (:1206-1213).  tests/native/fill_model.c is the same restatement on the CPU.
//
// Form: encode_exact.hpp's.  One wavefront, the table in LDS (16 KiB: 8192 x u16 or 4096 x u32), a serial parse that every lane
// runs with the same values, and the lanes sharing LZ4_count, the literal copies and the length runs.  Stores are exact-length:
// the reference's wild copies and 4-byte length writes are not restated, so nothing behind the returned size is written.  A token
// is stored when its match length is known, so a rewound sequence has stored nothing that the last run does not overwrite:
// the literal rewind comes before the run's first store, and the token rewind can only follow the immediate re-test (:1159-1196),
// whose sequence has no literals (behind a literal run the test at :1029 has already asked for the same room).
#pragma once

#include "encode_exact.hpp"

namespace lz4dev {

enum FillTable { byU16 = 0, byU32 = 1 };

#define FILL_64K_LIMIT 65547          // LZ4_64Klimit, cbits/lz4.c:684: below it LZ4_compress_destSize takes byU16 (:1390)
static_assert(EXACT_TABLE * 4 == 8192 * 2, "either table is 16 KiB");

// LZ4_hashPosition (cbits/lz4.c:698-722) on a 64-bit little-endian host: byU16 hashes 4 bytes to LZ4_HASHLOG + 1 = 13 bits,
// byU32 5 bytes to 12
template <FillTable TT>
__device__ __forceinline__ uint32_t fill_hash(const uint8_t *p)
{
    if (TT == byU16) return (ex_rd32(p) * 2654435761u) >> (32 - (EXACT_HASHLOG + 1));
    return ex_hash5(p);
}

// One page: as much of src[0..n) as fits into dst[0..cap), n > 0, the table in LDS zeroed by the caller.  fill = true is
// fillOutput, fill = false notLimited (cap is not looked at: the caller has seen cap >= LZ4_compressBound(n), :1387).  Returns
// the page's size, 0 for cap < 1 (:902), and in `used` the bytes of src it holds (*inputConsumed; n when fill is false: :1388
// leaves *srcSizePtr alone).  All lanes of the wave call it with the same arguments.
template <FillTable TT>
__device__ int fill_encode_page(uint32_t *tab32, const uint8_t *src, int n, uint8_t *dst, int cap, bool fill, int &used)
{
    const uint32_t lane = (uint32_t)lane_id();
    uint16_t *tab16 = (uint16_t *)tab32;
    const long mflimitPlusOne = (long)n - LZ4_MFLIMIT + 1;
    const uint8_t *matchlimit = src + n - LZ4_LASTLITERALS;
    uint8_t *op = dst;
    uint8_t *const olimit = dst + cap;
    long ip = 0, anchor = 0;
    uint32_t forwardH;
    long match = 0;                                 // a position of src, as every table entry is (noDict, startIndex 0)
    uint32_t token = 0;                             // the open sequence's token byte, stored when its match length is known
    uint8_t *tokenAt = nullptr;

    auto tab_get = [&](uint32_t h) -> uint32_t { return ex_uni(TT == byU16 ? (uint32_t)tab16[h] : tab32[h]); };
    auto tab_set = [&](uint32_t h, uint32_t v) {
        if (lane == 0) {                            // one wave's LDS accesses complete in order: later reads see it
            if (TT == byU16) tab16[h] = (uint16_t)v; else tab32[h] = v;
        }
    };
    // the length field and the bytes of a literal run behind its token (:1033-1043, :1220-1230)
    auto run = [&](uint32_t lit) {
        tokenAt = op++;
        if (lit >= 15) {
            const uint32_t rest = lit - 15;
            token = 15u << 4;
            ex_fill255(op, rest / 255, true);
            op += rest / 255;
            ex_put(op++, rest % 255, true);
        } else {
            token = lit << 4;
        }
        wave_copy_bytes(op, src + anchor, lit);
        op += lit;
    };

    used = n;
    if (fill && cap < 1) return 0;                  // :902
    if (n < 13) goto last_literals;                 // :921 (LZ4_minLength)

    tab_set(fill_hash<TT>(src), 0u);                // :924
    ip = 1;
    forwardH = fill_hash<TT>(src + ip);

    for (;;) {
        // ---- search, :956-1014 ----
        {
            long forwardIp = ip;
            uint32_t step = 1;
            uint32_t searchMatchNb = 1u << 6;
            for (;;) {
                const uint32_t h = forwardH;
                const uint32_t current = (uint32_t)forwardIp;
                const uint32_t matchIndex = tab_get(h);     // a zero is position 0 of this source: a candidate like any other
                ip = forwardIp;
                forwardIp += step;
                step = searchMatchNb++ >> 6;
                if (forwardIp > mflimitPlusOne) goto last_literals;        // :969
                match = (long)matchIndex;                                   // :995
                forwardH = fill_hash<TT>(src + forwardIp);                  // :997
                tab_set(h, current);                                        // :998
                if (TT != byU16 && matchIndex + LZ4_MAXDIST < current) continue;   // :1003-1006 (byU16: every position is in reach)
                if (ex_rd32(src + match) == ex_rd32(src + ip)) break;       // :1009-1012
            }
        }
        // ---- catch up, :1019 ----
        while (ip > anchor && match > 0 && ex_rd8(src + ip - 1) == ex_rd8(src + match - 1)) { ip--; match--; }
        // ---- literals, :1022-1046 ----
        {
            const uint32_t lit = (uint32_t)(ip - anchor);
            // literal rewind, :1028-1032: token, length field, literals, offset, token and MFLIMIT - MINMATCH last literals
            if (fill && op + 1 + (lit + 240) / 255 + lit + 2 + 1 + LZ4_MFLIMIT - LZ4_MINMATCH > olimit) goto last_literals;
            run(lit);
        }
    next_match:
        // ---- token rewind, :1057-1062 (nothing of the sequence is stored yet: its token waits for the match length) ----
        if (fill && op + 2 + 1 + LZ4_MFLIMIT - LZ4_MINMATCH > olimit) {
            op = tokenAt;
            goto last_literals;
        }
        // ---- offset, :1069-1073 ----
        {
            const uint32_t offset = (uint32_t)(ip - match);
            ex_put(op, offset & 255u, true);
            ex_put(op + 1, offset >> 8, true);
            op += 2;
        }
        // ---- match length, :1091-1136 ----
        {
            uint32_t mc = ex_common_len(src + ip + LZ4_MINMATCH, src + match + LZ4_MINMATCH, matchlimit);
            ip += (long)mc + LZ4_MINMATCH;
            if (fill && op + (1 + LZ4_LASTLITERALS) + (mc + 240) / 255 > olimit) {
                // shortened match, :1099-1104: 14 in the token's terms and every byte of room but the last run's six as 255s
                const uint32_t shorter = 15 - 1 + ((uint32_t)(olimit - op) - 1 - LZ4_LASTLITERALS) * 255;
                ip -= (long)(mc - shorter);
                mc = shorter;                       // (:1105-1117 tidies a table that is not used again)
            }
            if (mc >= 15) {                                                 // :1123-1135
                token += 15;
                mc -= 15;
                ex_fill255(op, mc / 255, true);
                op += mc / 255;
                ex_put(op++, mc % 255, true);
            } else {
                token += mc;
            }
            ex_put(tokenAt, token, true);
        }
        anchor = ip;
        if (ip >= mflimitPlusOne) break;                                    // :1143
        tab_set(fill_hash<TT>(src + ip - 2), (uint32_t)(ip - 2));          // :1146
        // ---- immediate re-test at ip, :1159-1196 ----
        {
            const uint32_t h = fill_hash<TT>(src + ip);
            const uint32_t current = (uint32_t)ip;
            const uint32_t matchIndex = tab_get(h);
            tab_set(h, current);
            if ((TT == byU16 || matchIndex + LZ4_MAXDIST >= current) && ex_rd32(src + matchIndex) == ex_rd32(src + ip)) {
                match = (long)matchIndex;
                tokenAt = op++;
                token = 0;
                goto next_match;
            }
        }
        forwardH = fill_hash<TT>(src + (++ip));                             // :1200
    }

last_literals:                                                              // :1204-1231
    {
        uint32_t lastRun = (uint32_t)(n - anchor);
        if (fill && op + lastRun + 1 + (lastRun + 255 - 15) / 255 > olimit) {
            lastRun = (uint32_t)(olimit - op) - 1;                          // adapted last run, :1212-1213
            lastRun -= (lastRun + 256 - 15) / 256;
        }
        run(lastRun);
        ex_put(tokenAt, token, true);
        used = (int)(anchor + lastRun);                                     // :1229, :1234
    }
    return (int)(op - dst);
}

} // namespace lz4dev
