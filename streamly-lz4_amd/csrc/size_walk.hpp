// size_walk.hpp -- how many bytes does a block decode to?  One wavefront walks a block's token chain and adds up
// lit + matchlen; it reads the compressed bytes and nothing else (no output ring, no copies, no scratch, no atomics).
//
// The walk is steps 1-4 of decode_par.hpp as a kernel of its own:
//   1. window     1 KiB of the compressed stream in LDS (16 B / lane), next to it one bit per byte: "this byte is not 255".
//                 A length extension is a run of 255s and the byte that ends it, so "where does the run that starts at q
//                 end" is a count of trailing zeros in that bit vector -- no loop over the bytes.
//   2. speculate  every lane parses 8 candidate token positions (512 candidates): where would the next token be if one
//                 started here?  Runs of up to 31 extension bytes are followed through the bit vector.
//   3. chain      pointer jumping over that successor table (three squaring rounds, then groups of 8 lanes): sequence r
//                 of the batch ends up on lane r.
//   4. lengths    lane r reads its sequence's fields (aligned dword reads + a byte funnel: an unaligned LDS access costs
//                 about a cycle per active lane, decode_par.hpp) and a DPP wave scan of lit + matchlen places it.
// A batch takes the sequences that lie entirely inside the window and in front of the block's last sequence.  Anything
// else -- a literal run or an extension run that leaves the window (a 64 KiB incompressible block is one token with 257
// extension bytes, a block of zeros one match with as many), the block's last sequence, a malformed field -- is ONE
// sequence walked by the whole wave from global memory (sw_step): the run of 255s is skipped 1 KiB at a time with a
// ballot over "byte != 255".  That step is also the only place where a block is judged, so the acceptance rule below
// stands in one piece of code.
//
// size = s >= 0 exactly when
//   1. the chain is well formed: every token, extension byte, literal run and offset lies inside the block, and the
//      chain ends exactly at the block's end with a sequence of literals only;
//   2. the block keeps the end-of-block rules every conforming encoder keeps (cbits/lz4.c:214-221): a block of under 13
//      bytes has no match, the last match starts at least 12 bytes before the end (at s - 12 or earlier: the decoder's
//      check, :1991, and what the compressor's mflimitPlusOne allows -- it writes such blocks) and the last 5 bytes are
//      literals;
//   3. s <= maxUncomp;
//   4. no offset is 0; an empty block is the single byte 0x00 (the reference decodes no other into zero bytes of
//      capacity, cbits/lz4.c:1781-1785); and no match that carries extension bytes AND ends within the last 64 output
//      bytes reaches in front of the block.
// Rules 2 and 4 are what makes decoding into exactly s bytes the same as decoding into any larger capacity: capacity
// enters the reference decoder through its oend-relative checks only (cbits/lz4.c:1797-1924).  Rule 2 keeps the
// end-of-block checks silent.  The last clause of rule 4 is about the code a BAD offset gets: the fast loop rejects it
// in front of the match's extension bytes (:1853), the safe loop behind them (:2073), and which loop a sequence sees
// depends on its distance from oend (:1858) -- so such a match, whose source may or may not exist (that is the
// decoder's business: a dictionary), is left to the capacity the caller would have used anyway.  Offsets are not
// judged otherwise.
#pragma once

#include "decode_par.hpp"

namespace lz4dev {

#define SW_WIN 1024          // bytes of compressed stream staged per window (16 per lane)
#define SW_NL 8              // token candidates per lane
#define SW_NODES (SW_NL * LZ4_WAVE)
#define SW_FAR 0x40000000u   // "the sequence does not end inside the window"
#define SW_TAIL 64           // the reference's FASTLOOP_SAFE_DISTANCE (rule 4)

#define SIZE_E_UNKNOWN (-0x7F000005)   // = MI355LZ4_BLK_E_SIZE_UNKNOWN

struct __attribute__((aligned(16))) SizeLds {
    uint8_t win[SW_WIN + 16];            // 16 bytes of zeros behind the window: a dword read may start at its last byte
    uint32_t nz[SW_WIN / 32 + 2];        // bit q: window byte q is not 255; two words of zeros behind it (a run that leaves the window)
    uint16_t jump[SW_NODES + 8];         // successor table, entries are byte offsets into itself (decode_par.hpp)
};

// 16 bytes at the 16-byte aligned address q, zeros where they lie outside [lo, hi)
__device__ __forceinline__ uint4 sw_fetch16(const uint8_t *q, const uint8_t *lo, const uint8_t *hi)
{
    if (q >= lo && q + 16 <= hi) {
        const par_v4 v = *as_global((const par_v4 *)q);
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    uint32_t w[4] = {0, 0, 0, 0};
    for (int k = 0; k < 16; k++)
        if (q + k >= lo && q + k < hi) w[k >> 2] |= (uint32_t)as_global(q)[k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// bit k: byte k of the 16 is not 255
__device__ __forceinline__ uint32_t sw_not255(uint4 v)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) m |= (((w[k >> 2] >> (8 * (k & 3))) & 0xffu) != 0xffu ? 1u : 0u) << k;
    return m;
}

// First position in [pos, iend) of the block at src whose byte is not 255, or iend: the whole wave, 1 KiB per step.
__device__ __forceinline__ int sw_skip_run(const uint8_t *src, int pos, int iend, const uint8_t *lo, const uint8_t *hi, int lane)
{
    while (pos < iend) {
        const uintptr_t a = (uintptr_t)(src + pos);
        const uintptr_t base = a & ~(uintptr_t)15;
        const int rel0 = pos - (int)(a - base);                  // block position of lane 0's first byte
        uint32_t m = sw_not255(sw_fetch16((const uint8_t *)(base + 16u * (uint32_t)lane), lo, hi));
        const int p0 = rel0 + 16 * lane;
        const int loK = pos - p0, hiK = iend - p0;                // my bytes [loK, hiK) are the run's
        if (loK > 0) m &= (loK >= 16) ? 0u : (0xffffu << loK);
        if (hiK < 16) m &= (hiK <= 0) ? 0u : ((1u << hiK) - 1u);
        const uint64_t b = __ballot(m != 0u);
        if (b) {
            const int l = (int)__builtin_ctzll(b);
            return rel0 + 16 * l + (int)__builtin_ctz((uint32_t)__builtin_amdgcn_readlane((int)m, l));
        }
        pos = rel0 + 16 * LZ4_WAVE;
    }
    return iend;
}

// window position of the first byte at or behind q (< SW_WIN) that is not 255, SW_FAR when none of the next 32 is
__device__ __forceinline__ uint32_t sw_run_end(const SizeLds &L, uint32_t q)
{
    const uint32_t d0 = L.nz[q >> 5], d1 = L.nz[(q >> 5) + 1];
    const uint32_t w = (uint32_t)((((uint64_t)d1 << 32) | d0) >> (q & 31u));
    return w ? q + (uint32_t)__builtin_ctz(w) : SW_FAR;
}

// The sequence whose token t lies at window position c (b1: the byte behind it): literal length, position of its offset
// field, position of the next token -- SW_FAR (or beyond) when a field leaves the window.
__device__ __forceinline__ uint32_t sw_parse(const SizeLds &L, uint32_t c, uint32_t t, uint32_t b1, uint32_t &lit, uint32_t &offPos)
{
    uint32_t p = c + 1u;
    lit = t >> 4;
    offPos = SW_FAR;
    if (lit == 15u) {
        if (b1 != 255u) { lit = 15u + b1; p = c + 2u; }
        else {
            const uint32_t r = sw_run_end(L, c + 1u);
            if (r >= SW_FAR) return SW_FAR;
            lit = 15u + 255u * (r - (c + 1u)) + L.win[r];
            p = r + 1u;
        }
    }
    offPos = p + lit;
    if ((t & 15u) != 15u) return offPos + 2u;
    if (offPos + 2u >= SW_WIN) return SW_FAR;
    const uint32_t r = sw_run_end(L, offPos + 2u);
    return (r >= SW_FAR) ? SW_FAR : r + 1u;
}

// What the walk carries from sequence to sequence (wave-uniform).
struct SizeWalk {
    int ip;                  // block position of the next token
    uint64_t op;             // output bytes so far
    uint64_t lastMl;         // length of the last match
    uint64_t riskEnd;        // output position behind the last match that has extension bytes and reaches in front of the block
    bool anyMatch, risk, zeroOff;
};

// One sequence by the whole wave, from global memory.  0: go on; 1: it was the block's last sequence, w.lastMl / w.op are
// final and lastLit is its length; -1: the chain is malformed.
__device__ __forceinline__ int sw_step(SizeWalk &w, const uint8_t *src, int iend, const uint8_t *lo, const uint8_t *hi, int lane,
                                       uint64_t &lastLit)
{
    const LZ4_GLOBAL uint8_t *g = as_global(src);
    const uint32_t t = g[w.ip];
    int pos = w.ip + 1;
    uint64_t lit = t >> 4;
    if (lit == 15u) {
        const int r = sw_skip_run(src, pos, iend, lo, hi, lane);
        if (r >= iend) return -1;
        lit = 15u + 255ull * (uint64_t)(r - pos) + g[r];
        pos = r + 1;
    }
    if (lit > (uint64_t)(iend - pos)) return -1;
    pos += (int)lit;
    if (pos == iend) { lastLit = lit; w.op += lit; return 1; }
    if (pos + 2 > iend) return -1;
    const uint32_t off = (uint32_t)g[pos] | ((uint32_t)g[pos + 1] << 8);
    pos += 2;
    uint64_t ml = t & 15u;
    const bool mlx = ml == 15u;
    if (mlx) {
        const int r = sw_skip_run(src, pos, iend, lo, hi, lane);
        if (r >= iend) return -1;
        ml = 15u + 255ull * (uint64_t)(r - pos) + g[r];
        pos = r + 1;
    }
    ml += LZ4_MINMATCH;
    if (pos >= iend) return -1;                       // a block ends with literals: a token must follow a match
    const uint64_t at = w.op + lit;
    if (off == 0u) w.zeroOff = true;
    if (mlx && off > at) { w.risk = true; w.riskEnd = at + ml; }
    w.op = at + ml;
    w.lastMl = ml;
    w.anyMatch = true;
    w.ip = pos;
    return 0;
}

// Decoded size of the block src[0, srcLen), or SIZE_E_UNKNOWN (the rule at the top of this file).  [lo, hi) bounds every read.
// WINDOW: the block of a standard LZ4 frame (kernels/frames.inc).  Only the last clause of rule 4 is dropped: in a linked frame a
// long match from the window that ends near the block's end is legitimate, and a frame promises no particular code for a bad
// offset -- the decode into exactly s bytes says whether the source exists.  Rule 2 stays.
template <bool WINDOW = false>
__device__ __forceinline__ int decoded_size_block(const uint8_t *src, int srcLen, int maxUncomp, const uint8_t *lo,
                                                  const uint8_t *hi, SizeLds &L)
{
    const int lane = lane_id();
    const int iend = srcLen;
    const uint8_t *jumpB = (const uint8_t *)L.jump;
    SizeWalk w;
    w.ip = 0; w.op = 0; w.lastMl = 0; w.riskEnd = 0; w.anyMatch = false; w.risk = false; w.zeroOff = false;
    uint64_t lastLit = 0;

    for (;;) {
        if (w.op > (uint64_t)maxUncomp) return SIZE_E_UNKNOWN;
        int nseq = 0;
        if (iend - w.ip >= 32) {
            // ---------------- 1. window ----------------
            const uint8_t *gp = src + w.ip;
            const uintptr_t abase = (uintptr_t)gp & ~(uintptr_t)15;
            const int wofs = (int)((uintptr_t)gp - abase);
            const int ipW0 = w.ip - wofs;                                  // block position of window byte 0
            const int iendW = (int)min((int64_t)iend - ipW0, (int64_t)1 << 20);   // block end in window coordinates
            const int inLim = min(iendW - 1, SW_WIN);                      // a batch's sequence ends at or before this: inside the window, a token behind it
            wave_fence();
            {
                const uint4 v = sw_fetch16((const uint8_t *)(abase + 16u * (uint32_t)lane), lo, hi);
                *(uint4 *)&L.win[16 * lane] = v;
                ((uint16_t *)L.nz)[lane] = (uint16_t)sw_not255(v);
            }
            wave_fence();

            // ---------------- 2. speculative parse ----------------
            const uint32_t absorb = 2u * ((uint32_t)min(inLim, SW_NODES - 1) + 1u);
            uint32_t J[SW_NL];
            {
                const uint64_t b0 = *(const uint64_t *)&L.win[SW_NL * lane], b8 = *(const uint64_t *)&L.win[SW_NL * lane + 8];
#pragma unroll
                for (int j = 0; j < SW_NL; j++) {
                    const uint32_t t = (uint32_t)(b0 >> (8 * j)) & 0xffu;
                    const uint32_t b1 = (j < 7) ? ((uint32_t)(b0 >> (8 * (j + 1))) & 0xffu) : ((uint32_t)b8 & 0xffu);
                    uint32_t lit, offPos;
                    const uint32_t nxt = sw_parse(L, (uint32_t)(SW_NL * lane + j), t, b1, lit, offPos);
                    J[j] = min(2u * min(nxt, (uint32_t)SW_NODES), absorb);
                }
                uint32_t *tw = (uint32_t *)&L.jump[SW_NL * lane];
#pragma unroll
                for (int p = 0; p < SW_NL / 2; p++) tw[p] = J[2 * p] | (J[2 * p + 1] << 16);
                if (lane == 0) L.jump[SW_NODES] = (uint16_t)(2 * SW_NODES);     // absorbing state behind the table
            }
            wave_fence();

            // ---------------- 3. chain: sequence r -> lane r ----------------
            uint32_t c2 = (lane == 0) ? 2u * (uint32_t)wofs : absorb;          // 2 x token position
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const int d = 1 << k;
                const int cj = (int)*(const uint16_t *)(jumpB + c2);
#pragma unroll
                for (int j = 0; j < SW_NL; j++) J[j] = (uint32_t)*(const uint16_t *)(jumpB + J[j]);
                const int sh = par_bperm(cj, (lane - d) & 63);
                if (lane >= d && lane < 2 * d) c2 = (uint32_t)sh;
                wave_fence();
                uint32_t *tw = (uint32_t *)&L.jump[SW_NL * lane];
#pragma unroll
                for (int p = 0; p < SW_NL / 2; p++) tw[p] = J[2 * p] | (J[2 * p + 1] << 16);
                wave_fence();
            }
#pragma unroll
            for (int g = 1; g < LZ4_WAVE / 8; g++) {
                int cj = (int)absorb;
                if (lane >= 8 * (g - 1) && lane < 8 * g) cj = (int)*(const uint16_t *)(jumpB + c2);
                const int sh = par_bperm(cj, (lane - 8) & 63);
                if (lane >= 8 * g && lane < 8 * g + 8) c2 = (uint32_t)sh;
            }

            // ---------------- 4. my sequence's lengths, a scan places it ----------------
            const bool has = c2 < absorb;
            const uint32_t cc = has ? (c2 >> 1) : 0u;
            const uint32_t tb = lds_u32_any(L.win, cc);
            const uint32_t t = tb & 0xffu;
            uint32_t lit, offPos;
            const uint32_t nxt = sw_parse(L, cc, t, (tb >> 8) & 0xffu, lit, offPos);
            const bool ok = has && nxt < SW_FAR && (int)nxt <= inLim;
            const uint32_t off16 = lds_u32_any(L.win, min(offPos, (uint32_t)SW_WIN)) & 0xffffu;
            const bool mlx = (t & 15u) == 15u;
            uint32_t ml = (t & 15u) + LZ4_MINMATCH;
            if (mlx) {
                const uint32_t r = min(nxt - 1u, (uint32_t)SW_WIN);
                ml += 255u * (r - min(offPos + 2u, r)) + L.win[r];
            }
            const int len = ok ? (int)(lit + ml) : 0;
            const int incl = par_scan_incl(len);
            const uint64_t okm = __ballot(ok);
            nseq = (~okm) ? (int)__builtin_ctzll(~okm) : LZ4_WAVE;
            if (nseq > 0) {
                const bool act = lane < nseq;
                const uint64_t at = w.op + (uint64_t)(uint32_t)(incl - (int)ml);          // where my match starts
                if (__ballot(act && off16 == 0u)) w.zeroOff = true;
                const uint64_t rm = __ballot(act && mlx && (uint64_t)off16 > at);
                if (rm) {
                    w.risk = true;
                    w.riskEnd = w.op + (uint64_t)(uint32_t)__builtin_amdgcn_readlane(incl, 63 - (int)__builtin_clzll(rm));
                }
                w.lastMl = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)ml, nseq - 1);
                w.anyMatch = true;
                w.op += (uint64_t)(uint32_t)__builtin_amdgcn_readlane(incl, nseq - 1);
                w.ip = ipW0 + __builtin_amdgcn_readlane((int)nxt, nseq - 1);
            }
        }
        if (nseq == 0) {
            const int r = sw_step(w, src, iend, lo, hi, lane, lastLit);
            if (r < 0) return SIZE_E_UNKNOWN;
            if (r > 0) break;
        }
    }
    // the chain is well formed (rule 1); rules 2-4
    const uint64_t s = w.op;
    if (s > (uint64_t)maxUncomp) return SIZE_E_UNKNOWN;
    if (w.anyMatch && (s < LZ4_MFLIMIT + 1 || lastLit < LZ4_LASTLITERALS || lastLit + w.lastMl < LZ4_MFLIMIT)) return SIZE_E_UNKNOWN;
    if (w.zeroOff) return SIZE_E_UNKNOWN;
    if (s == 0 && (srcLen != 1 || as_global(src)[0] != 0)) return SIZE_E_UNKNOWN;
    if (!WINDOW && w.risk && w.riskEnd + SW_TAIL >= s) return SIZE_E_UNKNOWN;
    return (int)s;
}

} // namespace lz4dev
