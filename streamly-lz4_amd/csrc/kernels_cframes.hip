// kernels_cframes.hip -- writing batches of standard LZ4 frames: the frame layer on the device (mi355lz4_cframes).
//
// A translation unit of its own for the reason kernels_hstreams.hip gives: kernels added to kernels.hip have moved other kernels'
// register and spill counts.  Nothing here calls an encoder; the compressed blocks come from the engine's own call (cframes.cpp),
// which runs between launch_cframes_plan and launch_cframes_finish.  What is shared with kernels.hip is source -- wave_copy_bytes
// (lz4_device.hpp), xxh32_group (checksum.hpp) -- and one launcher, launch_scan_u64.
//
// plan:   k_cframes_count   per input: is its range inside src and its length inside the call's bound, how many blocks
//         k_scan_u64        every input's first block
//         k_cframes_plan    per table entry: the engine call's srcOff[] / srcLen[] and the block -> input map
// finish: k_cframes_sizes   per entry: stored or compressed, the length of its piece of the frame
//         k_scan_u64        where every piece lies
//         k_cframes_layout  per input: the frame's length, the capacity verdict, frameLen[i]
//         k_cframes_pack    per entry and 16 KiB of it: size word and payload to their place (k_cframes_bsum: the block checksums)
//         k_cframes_head    per input: header, end mark, content checksum
//
// All addresses are 64-bit.  Every read of src lies inside an input's range, which k_cframes_count held to [0, srcBufLen); every
// write lies inside [dstOff[i], dstOff[i] + frameLen[i]) of an input whose frame fits dstCap[i].
#include "kernels.h"

#include "lz4_device.hpp"
#include "checksum.hpp"

#include <algorithm>
#include <atomic>

using namespace lz4dev;

// first table entry of input i: its first block, and the spacers of the inputs in front of it
__device__ __forceinline__ uint64_t cfrm_first(const CFramesArgs &a, int i)
{
    return a.blockFirst[i] + ((a.flags & CFRM_LINKED) ? (uint64_t)i : 0u);
}
// an input the table has no room for: its blocks end behind the call's block bound (and so do those of every input after it)
__device__ __forceinline__ bool cfrm_over(const CFramesArgs &a, int i, int nb) { return nb > 0 && a.blockFirst[i + 1] > (uint64_t)a.realCap; }

__global__ __launch_bounds__(256) void k_cframes_count(CFramesArgs a)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= a.nInputs) return;
    const uint64_t off = a.inOff[i], len = a.inLen[i];
    bool ok = off <= a.srcBufLen && len <= a.srcBufLen - off && len <= a.maxInputLen;
    const uint64_t nb = len / a.bmax + (len % a.bmax ? 1u : 0u);
    if (nb > (uint64_t)a.realCap) ok = false;
    a.nb[i] = ok ? (int32_t)nb : -1;
}

// Grid-stride over the table.  The input of entry e is the last one whose first entry is <= e (inputs without blocks share their
// first entry with the next one, and lose); what lies behind its blocks is its spacer, or the table's unused end.
__global__ __launch_bounds__(256) void k_cframes_plan(CFramesArgs a)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < (int64_t)a.tabCap; e += (int64_t)gridDim.x * 256) {
        int lo = 0, hi = a.nInputs - 1;
        while (lo < hi) {
            const int mid = lo + (hi - lo + 1) / 2;
            if (cfrm_first(a, mid) <= (uint64_t)e) lo = mid; else hi = mid - 1;
        }
        const int i = lo, nb = a.nb[i];
        const uint64_t k = (uint64_t)e - cfrm_first(a, i);
        const bool real = nb > 0 && k < (uint64_t)nb && !cfrm_over(a, i, nb);
        uint64_t off = 0;
        int32_t n = 0;
        if (real) {
            const uint64_t at = k * (uint64_t)a.bmax, len = a.inLen[i];
            off = a.inOff[i] + at;
            n = (int32_t)min((uint64_t)a.bmax, len - at);
        }
        a.srcOff[e] = off; a.srcLen[e] = n; a.blockInput[e] = real ? i : -1;
    }
}

// what the frame holds of entry e: n stored bytes when the encoder gave c >= n (or nothing), else its c bytes
struct CfrmBlock { int n; int payload; bool stored; };
__device__ __forceinline__ CfrmBlock cfrm_block(const CFramesArgs &a, int64_t e)
{
    CfrmBlock b;
    b.n = a.srcLen[e];
    const int c = a.framedLen[e] - 4;
    b.stored = c <= 0 || c >= b.n;
    b.payload = b.stored ? b.n : c;
    return b;
}

__global__ __launch_bounds__(256) void k_cframes_sizes(CFramesArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)a.tabCap) return;
    int32_t p = 0;
    if (a.blockInput[e] >= 0) p = 4 + cfrm_block(a, e).payload + ((a.flags & CFRM_BLOCK_CHECKSUM) ? 4 : 0);
    a.piece[e] = p;
}

__device__ __forceinline__ uint32_t cfrm_header_bytes(uint32_t flags) { return (flags & CFRM_CONTENT_SIZE) ? 15u : 7u; }

__global__ __launch_bounds__(256) void k_cframes_layout(CFramesArgs a)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= a.nInputs) return;
    const int nb = a.nb[i];
    int64_t v = FRW_E_INPUT;
    if (nb >= 0 && !cfrm_over(a, i, nb)) {
        uint64_t body = 0, p0 = 0;
        if (nb > 0) {
            const uint64_t e0 = cfrm_first(a, i);
            p0 = a.pieceOff[e0];
            body = a.pieceOff[e0 + (uint64_t)nb] - p0;
        }
        const uint64_t hdr = cfrm_header_bytes(a.flags);
        const uint64_t total = hdr + body + 4u + ((a.flags & CFRM_CONTENT_CHECKSUM) ? 4u : 0u);
        v = total > a.dstCap[i] ? (int64_t)FRW_E_CAPACITY : (int64_t)total;
        a.base[i] = a.dstOff[i] + hdr - p0;
    }
    a.verdict[i] = v;
    a.frameLen[i] = v;
}

__device__ __forceinline__ void cfrm_store32(uint8_t *p, uint32_t v)
{
    LZ4_GLOBAL uint8_t *g = as_global(p);
    g[0] = (uint8_t)v; g[1] = (uint8_t)(v >> 8); g[2] = (uint8_t)(v >> 16); g[3] = (uint8_t)(v >> 24);
}

// One wavefront per (entry, piece of CFRM_PIECE payload bytes) on a persistent grid: a block of 4 MiB is 256 waves' work, so the
// copy's parallelism is not the block count.  Piece 0 writes the size word too.  A stored block comes from src, a compressed one
// from behind the 4-byte header of its slot.
__global__ __launch_bounds__(LZ4_WAVE) void k_cframes_pack(CFramesArgs a, int perBlock)
{
    const int64_t items = (int64_t)a.tabCap * perBlock;
    for (int64_t t = (int64_t)blockIdx.x; t < items; t += (int64_t)gridDim.x) {
        const int64_t e = t / perBlock;
        const uint32_t j = (uint32_t)(t - e * perBlock);
        const int i = uni(a.blockInput[e]);
        if (i < 0 || uni64(a.verdict[i]) < 0) continue;
        const CfrmBlock b = cfrm_block(a, e);
        const uint32_t payload = (uint32_t)uni(b.payload), from = j * CFRM_PIECE;
        if (from >= payload) continue;                                  // (payload > 0: a block has bytes)
        const bool stored = uni((int)b.stored) != 0;
        uint8_t *to = a.dst + (uint64_t)uni64((int64_t)(a.base[i] + a.pieceOff[e]));
        const uint8_t *data = stored ? a.src + (uint64_t)uni64((int64_t)a.srcOff[e]) : a.slots + (uint64_t)e * a.slotStride + 4;
        if (j == 0 && lane_id() == 0) cfrm_store32(to, payload | (stored ? 0x80000000u : 0u));
        wave_copy_bytes(to + 4 + from, data + from, min(CFRM_PIECE, payload - from));
    }
}

// block checksums, four lanes per entry: over the payload as stored, read where k_cframes_pack reads it
__global__ __launch_bounds__(256) void k_cframes_bsum(CFramesArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e = t >> 2;
    const int q = (int)(t & 3);
    const uint8_t *p = a.slots;
    int64_t L = -1;
    uint8_t *to = nullptr;
    if (e < (int64_t)a.tabCap) {
        const int i = a.blockInput[e];
        if (i >= 0 && a.verdict[i] >= 0) {
            const CfrmBlock b = cfrm_block(a, e);
            p = b.stored ? a.src + a.srcOff[e] : a.slots + (uint64_t)e * a.slotStride + 4;
            L = b.payload;
            to = a.dst + a.base[i] + a.pieceOff[e] + 4u + (uint64_t)b.payload;
        }
    }
    const uint32_t h = xxh32_group(p, L, 0u, q);
    if (q == 0 && L >= 0) cfrm_store32(to, h);
}

// xxh32 (seed 0) of a frame descriptor -- FLG, BD and, with `sized`, the 8 bytes of the content size -- from registers
__device__ __forceinline__ uint32_t cfrm_descriptor_hash(uint32_t flg, uint32_t bd, uint64_t size, bool sized)
{
    uint32_t h = XXH_P5 + (sized ? 10u : 2u);
    uint32_t b0 = flg, b1 = bd;
    if (sized) {
        h = xxh_rotl(h + (flg | (bd << 8) | ((uint32_t)(size & 0xffffu) << 16)) * XXH_P3, 17) * XXH_P4;
        h = xxh_rotl(h + (uint32_t)(size >> 16) * XXH_P3, 17) * XXH_P4;
        b0 = (uint32_t)(size >> 48) & 0xffu; b1 = (uint32_t)(size >> 56);
    }
    h = xxh_rotl(h + b0 * XXH_P5, 11) * XXH_P1;
    h = xxh_rotl(h + b1 * XXH_P5, 11) * XXH_P1;
    h ^= h >> 15; h *= XXH_P2;
    h ^= h >> 13; h *= XXH_P3;
    h ^= h >> 16;
    return h;
}

// Four lanes per input: the content checksum over the input (xxh32 is four serial chains: one huge input is hashed by four lanes,
// the limit k_frames_finish has on the decode side), then lane 0 writes everything of the frame that is no block.
__global__ __launch_bounds__(256) void k_cframes_head(CFramesArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t >> 2), q = (int)(t & 3);
    const uint8_t *p = a.src;
    int64_t L = -1, v = -1;
    uint64_t len = 0;
    if (i < a.nInputs) {
        v = a.verdict[i];
        if (v >= 0) {
            len = a.inLen[i];
            if (a.flags & CFRM_CONTENT_CHECKSUM) { p = a.src + a.inOff[i]; L = (int64_t)len; }
        }
    }
    const uint32_t h = xxh32_group(p, L, 0u, q);
    if (q != 0 || v < 0) return;
    uint8_t *f = a.dst + a.dstOff[i];
    const bool sized = (a.flags & CFRM_CONTENT_SIZE) != 0;
    const uint32_t flg = 0x40u | ((a.flags & CFRM_LINKED) ? 0u : 0x20u) | ((a.flags & CFRM_BLOCK_CHECKSUM) ? 0x10u : 0u) |
                         (sized ? 0x08u : 0u) | ((a.flags & CFRM_CONTENT_CHECKSUM) ? 0x04u : 0u);
    const uint32_t bd = (uint32_t)a.bsid << 4;
    cfrm_store32(f, 0x184D2204u);
    LZ4_GLOBAL uint8_t *g = as_global(f);
    g[4] = (uint8_t)flg; g[5] = (uint8_t)bd;
    uint32_t at = 6;
    if (sized) { cfrm_store32(f + 6, (uint32_t)len); cfrm_store32(f + 10, (uint32_t)(len >> 32)); at = 14; }
    g[at] = (uint8_t)(cfrm_descriptor_hash(flg, bd, len, sized) >> 8);
    uint8_t *end = f + (uint64_t)v - 4u - (L >= 0 ? 4u : 0u);
    cfrm_store32(end, 0u);
    if (L >= 0) cfrm_store32(end + 4, h);
}

static int cframes_cus()
{
    static std::atomic<int> cus[64];                                    // CUs per device, asked for once
    int dev = 0;
    (void)hipGetDevice(&dev);
    int nc = cus[dev & 63].load(std::memory_order_relaxed);
    if (nc <= 0) {
        if (hipDeviceGetAttribute(&nc, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || nc <= 0) nc = 256;
        cus[dev & 63].store(nc, std::memory_order_relaxed);
    }
    return nc;
}
static inline unsigned per256(int64_t n) { return (unsigned)((n + 255) / 256); }

void launch_cframes_plan(const CFramesArgs &a, hipStream_t s)
{
    if (a.nInputs <= 0) return;
    hipLaunchKernelGGL(k_cframes_count, dim3(per256(a.nInputs)), dim3(256), 0, s, a);
    launch_scan_u64(a.nb, a.nInputs, a.blockFirst, s);
    const unsigned grid = (unsigned)std::min<int64_t>(per256(a.tabCap), (int64_t)cframes_cus() * 8);
    hipLaunchKernelGGL(k_cframes_plan, dim3(grid), dim3(256), 0, s, a);
}

void launch_cframes_finish(const CFramesArgs &a, hipStream_t s)
{
    if (a.nInputs <= 0) return;
    hipLaunchKernelGGL(k_cframes_sizes, dim3(per256(a.tabCap)), dim3(256), 0, s, a);
    launch_scan_u64(a.piece, a.tabCap, a.pieceOff, s);
    hipLaunchKernelGGL(k_cframes_layout, dim3(per256(a.nInputs)), dim3(256), 0, s, a);
    const int perBlock = std::max(1, (int)(((uint32_t)a.maxBlockLen + CFRM_PIECE - 1) / CFRM_PIECE));
    const int64_t items = (int64_t)a.tabCap * perBlock;
    hipLaunchKernelGGL(k_cframes_pack, dim3((unsigned)std::min<int64_t>(items, (int64_t)cframes_cus() * 32)), dim3(LZ4_WAVE), 0, s, a, perBlock);
    if (a.flags & CFRM_BLOCK_CHECKSUM) hipLaunchKernelGGL(k_cframes_bsum, dim3(per256((int64_t)a.tabCap * 4)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_cframes_head, dim3(per256((int64_t)a.nInputs * 4)), dim3(256), 0, s, a);
}

// ---------------------------------------------------------------------------
// the host form's gather: the frames of a group, bound-spaced in dst, packed back to back
// ---------------------------------------------------------------------------
// exclusive scan of the lengths >= 0 (k_scan_u64 for 64-bit lengths: a frame may be longer than 2 GiB); one 1024-thread workgroup
__global__ __launch_bounds__(1024) void k_cframes_scan_len(const int64_t *len, int n, uint64_t *offs)
{
    __shared__ uint64_t part[1024];
    const int t = (int)threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    uint64_t sum = 0;
    for (int i = lo; i < hi; i++) sum += (uint64_t)max(len[i], (int64_t)0);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint64_t v = (t >= d) ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - sum;
    for (int i = lo; i < hi; i++) { offs[i] = run; run += (uint64_t)max(len[i], (int64_t)0); }
    if (t == 1023) offs[n] = part[1023];
}

// workgroup (x, y) of 4 waves: frames x, x + gridDim.x, ..; of each the 16 KiB pieces 4 * y + wave, + 4 * gridDim.y, ..
__global__ __launch_bounds__(256) void k_cframes_gather(const uint8_t *dst, const uint64_t *dstOff, const int64_t *frameLen, int n,
                                                        const uint64_t *scanOff, uint8_t *dense, uint64_t denseCap)
{
    if (scanOff[n] > denseCap) return;
    const uint64_t wave = (uint64_t)blockIdx.y * 4u + (threadIdx.x >> 6), step = (uint64_t)gridDim.y * 4u;
    for (int i = (int)blockIdx.x; i < n; i += (int)gridDim.x) {
        const int64_t len = uni64(frameLen[i]);
        if (len <= 0) continue;
        const uint8_t *from = dst + (uint64_t)uni64((int64_t)dstOff[i]);
        uint8_t *to = dense + (uint64_t)uni64((int64_t)scanOff[i]);
        for (uint64_t at = wave * CFRM_PIECE; at < (uint64_t)len; at += step * CFRM_PIECE)
            wave_copy_bytes(to + at, from + at, (uint32_t)min((uint64_t)CFRM_PIECE, (uint64_t)len - at));
    }
}

void launch_cframes_gather(const uint8_t *dst, const uint64_t *dstOff, const int64_t *frameLen, int nInputs, uint64_t *scanOff,
                           uint8_t *dense, uint64_t denseCap, hipStream_t s)
{
    hipLaunchKernelGGL(k_cframes_scan_len, dim3(1), dim3(1024), 0, s, frameLen, nInputs, scanOff);
    if (nInputs <= 0) return;
    const unsigned gx = (unsigned)std::min(nInputs, 2048);
    const unsigned gy = (unsigned)std::max(1, std::min(64, 2048 / nInputs));
    hipLaunchKernelGGL(k_cframes_gather, dim3(gx, gy), dim3(256), 0, s, dst, dstOff, frameLen, nInputs, (const uint64_t *)scanOff, dense,
                       denseCap);
}
