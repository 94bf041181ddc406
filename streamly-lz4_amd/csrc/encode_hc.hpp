// encode_hc.hpp -- high-compression LZ4 block encoder (mi355lz4_set_compression_level 1..12), one workgroup per block.
//
// The output is plain LZ4 (every decoder reads it); only the search differs from k_encode's fast mode.  Instead of one
// table candidate per position and greedy selection, every position gets the longest match a hash chain of depth
// 2^(level-1) finds (LZ4HC's chain: a ring of 64 Ki 16-bit distances, indexed p & 0xFFFF), and a one-step lazy parse
// chooses among them: at p, take the match unless the one at p+1 is longer.  DESIGN.md section 9.
//
// A workgroup of HC_THREADS threads owns a block at a time (persistent grid, blocks strided over the workgroups) and works
// through the window -- the dictionary's bytes (linked compression), then the block's -- in rounds of HC_THREADS
// positions, one per thread:
//   1. insert: each position's 4-byte hash is linked to the previous position with that hash.  Inside a wave, positions of
//      equal hash are grouped with ballots; the waves then take the head table in wave order, one barrier each, so the
//      chains never depend on the order in which lanes or waves happen to run;
//   2. search (block rounds only, and only positions the parse can still reach): walk the chain up to the level's depth,
//      bytes compared in global memory (L2), best[p] = (length, offset) into LDS;
//   3. parse (wave 0): the lazy rule over the round's best[], one ballot per 64 positions; the chosen sequences are parked
//      one per lane and written 64 at a time by encode_wave.hpp's emit_sequences.
// Parsing lags the search by one position (the rule at p reads best[p+1]): best[0] is the previous round's last position.
//
// Matches found by the search are capped at HC_CAP bytes (a run of zeros would otherwise compare the whole block at every
// position); a taken match of HC_CAP bytes is extended by the wave at parse time.  The ring is only valid for positions
// that no later insert has overwritten: a search in a round that has inserted up to rEnd looks no further back than
// rEnd - 65536 (offsets of up to 64 Ki - HC_THREADS at a round's first position, 65535 at its last).
// End rules as k_encode (cbits/lz4.c:214-221): inputs < 13 bytes are all literals, no match starts within the last 12
// bytes, the last 5 bytes are literals.  No scratch memory: everything lives in LDS (160 KiB: one workgroup per CU).
#pragma once

#include "encode_wave.hpp"

namespace lz4dev {

#define HC_THREADS 1024
#define HC_WAVES (HC_THREADS / LZ4_WAVE)
#define HC_HEAD 6144            /* head table entries (u32): 24 KiB; with the 128 KiB ring and best[], 155 KiB of LDS */
#define HC_CAP 256              /* longest match a search measures */
#define HC_NONE 0xffffffffu

struct HcLds {
    uint16_t chain[65536];          // distance to the previous position of the same hash; 0 = none
    uint32_t head[HC_HEAD];         // last position of each hash, HC_NONE = none
    uint32_t best[HC_THREADS + 1];  // length | offset << 16 of positions r - 1 .. rEnd - 1; 0 = no match
    int32_t cur;                    // the parse's position: positions below it are never searched
};

__device__ __forceinline__ uint32_t hc_load32(const uint8_t *p) { return *(const LZ4_GLOBAL u32_unaligned *)p; }
__device__ __forceinline__ uint32_t hc_hash(uint32_t v)
{
    return (uint32_t)(((uint64_t)(v * 2654435761u) * (uint64_t)HC_HEAD) >> 32);
}

// Length of the common prefix of a and b, at most lim bytes; reads never pass a + lim or b + lim.
__device__ __forceinline__ int hc_common(const uint8_t *a, const uint8_t *b, int lim)
{
    int k = 0;
    while (k + 8 <= lim) {
        const uint64_t x = *(const LZ4_GLOBAL u64_unaligned *)(a + k) ^ *(const LZ4_GLOBAL u64_unaligned *)(b + k);
        if (x) return k + (int)(__builtin_ctzll(x) >> 3);
        k += 8;
    }
    while (k < lim && as_global(a)[k] == as_global(b)[k]) k++;
    return k;
}

// Inserts the window positions [r, rEnd) (those with four bytes left before `end`).  Every thread of the workgroup calls it.
__device__ __forceinline__ void hc_insert(HcLds &L, const uint8_t *src, int r, int rEnd, int end)
{
    const int t = (int)threadIdx.x, lane = lane_id(), wave = t >> 6;
    const int p = r + t;
    const bool valid = p < rEnd && p + 4 <= end;
    const uint32_t h = valid ? hc_hash(hc_load32(src + p)) : HC_NONE;
    int predLane = -1;
    bool last = false;
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint64_t todo = __ballot(valid); todo;) {
        const uint32_t lh = (uint32_t)__builtin_amdgcn_readlane((int)h, (int)__builtin_ctzll(todo));
        const uint64_t m = __ballot(valid && h == lh);
        todo &= ~m;
        if (valid && h == lh) {
            const uint64_t lo = m & below;
            predLane = lo ? 63 - (int)__builtin_clzll(lo) : -1;
            last = (m >> lane) == 1ull;
        }
    }
    if (valid && predLane >= 0) L.chain[p & 0xFFFF] = (uint16_t)(lane - predLane);
    for (int w = 0; w < HC_WAVES; w++) {
        __syncthreads();
        if (wave == w && valid) {
            if (predLane < 0) {
                const uint32_t hd = L.head[h];
                L.chain[p & 0xFFFF] = (hd != HC_NONE && (uint32_t)p - hd <= 65535u) ? (uint16_t)((uint32_t)p - hd) : (uint16_t)0;
            }
            if (last) L.head[h] = (uint32_t)p;
        }
    }
    __syncthreads();
}

// best[] entry of window position p: the longest match (>= 4 bytes) within `depth` chain steps, nearest first on ties.
__device__ __forceinline__ uint32_t hc_search(const HcLds &L, const uint8_t *src, int p, int rEnd, int end, int depth)
{
    const int limit = min(end - LZ4_LASTLITERALS - p, HC_CAP);        // >= 8: p <= end - 13
    const int lowest = max(max(p - LZ4_MAXDIST, rEnd - 65536), 0);
    const uint32_t v0 = hc_load32(src + p);
    uint32_t tailMine = v0;                                             // my bytes [bl - 3, bl + 1)
    int bl = 3, bo = 0;
    uint32_t dist = L.chain[p & 0xFFFF];
    int cand = p - (int)dist;
    for (int d = 0; d < depth && dist != 0u && cand >= lowest; d++) {
        const uint32_t c0 = hc_load32(src + cand);
        const uint32_t ct = hc_load32(src + cand + bl - 3);
        const uint32_t nd = L.chain[cand & 0xFFFF];
        if (c0 == v0 && ct == tailMine) {
            const int len = 4 + hc_common(src + p + 4, src + cand + 4, limit - 4);
            if (len > bl) {
                bl = len;
                bo = p - cand;
                if (bl >= limit) break;
                tailMine = hc_load32(src + p + bl - 3);
            }
        }
        dist = nd;
        cand -= (int)nd;
    }
    return bl >= LZ4_MINMATCH ? (uint32_t)bl | ((uint32_t)bo << 16) : 0u;
}

// One block: n bytes at src, dictLen bytes of dictionary in front of them; writes the LZ4 block to dst, returns its length.
// Every thread of the workgroup calls it with the same arguments; the return value is meaningful in wave 0.
// PREPARED (k_encode_hc_dict, a mi355lz4_hcdict): the caller has loaded chain[] and head[] as they are after the inserts of
// the dictionary's positions [0, dictLen - 3) -- those whose four bytes lie inside the dictionary -- so only the last three
// positions, which hash across the seam into the block, are inserted here; the rounds, the parse and the bytes are the same.
template <bool PREPARED = false>
__device__ int encode_block_hc(HcLds &L, const uint8_t *blockSrc, int n, int dictLen, uint8_t *dst, int depth)
{
    const int t = (int)threadIdx.x, lane = lane_id(), wave = t >> 6;
    if (n < LZ4_MFLIMIT + 1) {                        // all literals (cbits/lz4.c:1263-1273 for n == 0: a single 0 token)
        if (wave == 0) {
            if (lane == 0) dst[0] = (uint8_t)(n << 4);
            if (lane < n) dst[1 + lane] = blockSrc[lane];
        }
        return 1 + n;
    }
    const uint8_t *src = blockSrc - dictLen;          // window position 0 = the dictionary's first byte
    const int end = dictLen + n;
    if (!PREPARED)
        for (int i = t; i < HC_HEAD; i += HC_THREADS) L.head[i] = HC_NONE;
    if (t == 0) { L.cur = dictLen; L.best[0] = 0u; }
    __syncthreads();
    if (PREPARED) {
        if (dictLen > 0) hc_insert(L, src, max(dictLen - 3, 0), dictLen, end);
    } else {
        for (int r = 0; r < dictLen; r += HC_THREADS) hc_insert(L, src, r, min(r + HC_THREADS, dictLen), end);
    }

    // wave 0's parse state (uniform)
    uint8_t *op = dst;
    int cur = dictLen, anchor = dictLen;
    int q0 = 0, q1 = 0, q2 = 0, q3 = 0, qCnt = 0;
    for (int r = dictLen; r < end; r += HC_THREADS) {
        const int rEnd = min(r + HC_THREADS, end);
        hc_insert(L, src, r, rEnd, end);
        const int p = r + t;
        uint32_t b = 0u;
        if (p < rEnd && p >= L.cur && p <= end - (LZ4_MFLIMIT + 1)) b = hc_search(L, src, p, rEnd, end, depth);
        L.best[1 + t] = b;
        __syncthreads();
        if (wave == 0) {
            // decisions for q in [cur, qEnd): best[q - (r - 1)] and the one behind it are in this round's best[]
            const int qEnd = rEnd == end ? end - LZ4_MFLIMIT : rEnd - 1;
            while (cur < qEnd) {
                const int q = cur + lane;
                uint32_t v = 0u, vn = 0u;
                if (q < qEnd) { v = L.best[q - r + 1]; vn = L.best[q - r + 2]; }
                const uint32_t len = v & 0xFFFFu, lenN = vn & 0xFFFFu;
                const uint64_t m = __ballot(len >= LZ4_MINMATCH && lenN <= len);
                if (!m) { cur = min(cur + LZ4_WAVE, qEnd); continue; }
                const int k = (int)__builtin_ctzll(m);
                const int mpos = cur + k;
                const int off = (int)((uint32_t)__builtin_amdgcn_readlane((int)v, k) >> 16);
                int mlen = __builtin_amdgcn_readlane((int)len, k);
                if (mlen == HC_CAP) {                      // the search stopped measuring: the wave extends the match
                    const int lim = end - LZ4_LASTLITERALS - mpos;
                    for (;;) {
                        const int i = mlen + lane;
                        const bool miss = i >= lim || as_global(src)[mpos + i] != as_global(src)[mpos - off + i];
                        const uint64_t mm = __ballot(miss);
                        if (mm) { mlen += (int)__builtin_ctzll(mm); break; }
                        mlen += LZ4_WAVE;
                    }
                }
                q0 = enc_writelane(q0, anchor, qCnt); q1 = enc_writelane(q1, mpos, qCnt);
                q2 = enc_writelane(q2, mlen, qCnt); q3 = enc_writelane(q3, off, qCnt);
                if (++qCnt == LZ4_WAVE) { op = emit_sequences(src, op, q0, q1, q2, q3, qCnt); qCnt = 0; }
                cur = anchor = mpos + mlen;
            }
            if (lane == 0) { L.cur = cur; L.best[0] = L.best[rEnd - r]; }
        }
        __syncthreads();
    }
    if (wave != 0) return 0;
    if (qCnt) op = emit_sequences(src, op, q0, q1, q2, q3, qCnt);
    // the last literals (cbits/lz4.c:1183-1199)
    const uint32_t lit = (uint32_t)(end - anchor);
    const uint32_t ext = lit >= 15u ? 1u + (lit - 15u) / 255u : 0u;
    if (lane == 0) {
        op[0] = (uint8_t)(min(lit, 15u) << 4);
        if (lit >= 15u) {
            uint32_t rest = lit - 15u, o = 1;
            while (rest >= 255u) { op[o++] = 255; rest -= 255u; }
            op[o] = (uint8_t)rest;
        }
    }
    wave_copy_bytes(op + 1 + ext, src + anchor, lit);
    return (int)(op + 1 + ext + lit - dst);
}

} // namespace lz4dev
