// host_batch.cpp -- the host-buffer calls of the C ABI (include/mi355lz4.h): blocks in caller memory go to the device, through the
// device-pointer calls of api.cpp, and back.  Host-side plumbing only, like api.cpp.
#include "engine.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace mi355lz4_detail;

// ---------------------------------------------------------------------------
// Pipelined host-buffer calls.  A call is cut into groups of blocks; the H2D copy of
// group i+1, the kernels of group i and the D2H copy of group i-1 run on three streams, and the CPU copies
// between pageable caller memory and the pinned staging slots run meanwhile on the copy pool.  Caller
// memory that is already page-locked (hipHostMalloc / hipHostRegister, e.g. a torch pinned tensor) is
// handed to the DMA engines directly.
// ---------------------------------------------------------------------------
// The pipelined calls keep the caller's stream, two copy streams and two compute streams busy; HIP multiplexes
// streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and streams that share a queue serialize
// (measured: compress 33 -> 41 GB/s with 8).  The variable is the process's: the library does not set it.

static bool pipe_trace()
{
    static const bool v = [] { const char *e = getenv("MI355LZ4_TRACE"); return e && atoi(e); }();
    return v;
}
static double now_ms()
{
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}
#define PTRACE(...) do { if (pipe_trace()) { fprintf(stderr, "[%10.3f] ", now_ms()); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

// Staging copies of a call of one or two groups go in pieces (decompress_host_pipelined): how many, and where piece q begins
static size_t sub_pieces(int groups, size_t bytes)
{
    static const int forced = [] { const char *e = getenv("MI355LZ4_STAGE_PIECES"); return e ? atoi(e) : 0; }();
    if (forced > 0) return (size_t)forced;
    // (measured, 10 MiB out / 3.6 MB in, ms per call: 1 piece 0.613, 2: 0.584, 4: 0.611, 8: 0.809 -- a piece costs ~30 us of calls and waits)
    return (groups > 2 || bytes < ((size_t)1 << 20)) ? 1 : 2;
}
static size_t piece_cut(size_t bytes, size_t q, size_t pieces)
{
    if (q >= pieces) return bytes;
    return (bytes / pieces * q) & ~(size_t)4095;
}

static size_t group_bytes()
{
    static const size_t v = [] {
        const char *e = getenv("MI355LZ4_GROUP_MB");
        const long mb = e ? atol(e) : 64;
        return (size_t)((mb < 1) ? 1 : (mb > 4096 ? 4096 : mb)) << 20;
    }();
    return v;
}

static bool host_range_is_pinned(const void *p, size_t n)
{
    if (!p || !n) return false;
    if (const char *e = getenv("MI355LZ4_NO_DIRECT")) if (atoi(e)) return false;
    hipPointerAttribute_t at;
    for (const uint8_t *q : {(const uint8_t *)p, (const uint8_t *)p + (n - 1)}) {
        if (hipPointerGetAttributes(&at, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (at.type != hipMemoryTypeHost) return false;
    }
    return true;
}

// the streams of a pipelined call and its pinned memory: two staging slots each way (none for a side that is page-locked: direct)
// of the largest group's bytes, and the per-group results
static int pipe_setup(mi355lz4_ctx *c, bool directIn, size_t maxIn, bool directOut, size_t maxOut, size_t metaBytes)
{
    if (!c->sIn) HIP_TRY(hipStreamCreateWithFlags(&c->sIn, hipStreamNonBlocking));
    if (!c->sOut) HIP_TRY(hipStreamCreateWithFlags(&c->sOut, hipStreamNonBlocking));
    for (hipStream_t &k : c->sK) if (!k) HIP_TRY(hipStreamCreateWithFlags(&k, hipStreamNonBlocking));
    int r;
    if (!directIn && (r = pin_reserve(c->pinIn, 2 * (maxIn + 16)))) return r;
    if (!directOut && (r = pin_reserve(c->pinOut, 2 * maxOut))) return r;
    return pin_reserve(c->pinMeta, metaBytes);
}

// groups of consecutive blocks, about group_bytes() of lens[] each: group g is blocks [gFirst[g], gFirst[g + 1])
static std::vector<int> cut_groups(const int32_t *lens, int n)
{
    std::vector<int> gFirst;
    size_t acc = 0;
    for (int i = 0; i < n; i++) {
        if (i == 0 || acc >= group_bytes()) { gFirst.push_back(i); acc = 0; }
        acc += (size_t)lens[i];
    }
    gFirst.push_back(n);
    return gFirst;
}

// run the device-API entry points on another stream of the same engine for the duration of a scope
struct StreamSwap {
    mi355lz4_ctx *c;
    hipStream_t saved;
    StreamSwap(mi355lz4_ctx *ctx, hipStream_t s) : c(ctx), saved(ctx->stream) { c->stream = s; }
    ~StreamSwap() { c->stream = saved; }
};

// events of one pipelined call, destroyed together; per group: its input is on the device, its kernels are done, its output is back
struct EventSet {
    std::vector<hipEvent_t> ev, in, k, out;
    explicit EventSet(int groups) : in((size_t)groups), k((size_t)groups), out((size_t)groups) {}
    ~EventSet() { for (hipEvent_t e : ev) if (e) hipEventDestroy(e); }
    int make(hipEvent_t *made)
    {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ev.push_back(e);
        *made = e;
        return 0;
    }
    int make_group(int g) { int r = make(&in[(size_t)g]); if (!r) r = make(&k[(size_t)g]); return r ? r : make(&out[(size_t)g]); }
};

// never return from a pipelined call with work in flight that still references caller or ctx buffers
struct DrainOnExit {
    mi355lz4_ctx *c;
    ~DrainOnExit()
    {
        if (c->sIn) hipStreamSynchronize(c->sIn);
        hipStreamSynchronize(c->stream);
        for (hipStream_t k : c->sK) if (k) hipStreamSynchronize(k);
        if (c->sOut) hipStreamSynchronize(c->sOut);
    }
};

// Dictionary in force before block 0, to c->scratch: only its last 64 KiB can be referenced, and
// keeping exactly 64 KiB preserves the reference's "dictSize >= 64 KB => no offset
// check" behaviour (cbits/lz4.c:1764).  *dlen = the bytes kept (0: none).
static int upload_dict(mi355lz4_ctx *c, int linked, const uint8_t *dict, int dictLen, uint32_t *dlen)
{
    *dlen = 0;
    if (!linked || !dict || dictLen <= 0) return 0;
    *dlen = (dictLen > 65536) ? 65536u : (uint32_t)dictLen;
    if (int r = dev_reserve(c->scratch, 65536 + 16)) return r;
    HIP_TRY(hipMemcpyAsync(c->scratch.p, dict + (dictLen - (int)*dlen), *dlen, hipMemcpyHostToDevice, c->stream));
    return 0;
}

// n bytes of page-locked memory to c->in + at, on the input copy stream
static int copy_in(mi355lz4_ctx *c, size_t at, const uint8_t *src, size_t n)
{
    HIP_TRY(hipMemcpyAsync((uint8_t *)c->in.p + at, src, n, hipMemcpyHostToDevice, c->sIn));
    return 0;
}
// One group's input, the contiguous host range src[0..n), to c->in + at: directly (slot null: src is page-locked), or through the
// pinned slot -- in pieces for a call of one or two groups, which has no other group's copies to hide its own staging behind: the
// copy engine moves one piece while the host copies the next (sub_pieces)
static int stage_range(mi355lz4_ctx *c, size_t at, const uint8_t *src, size_t n, uint8_t *slot, int groups)
{
    if (!slot) return copy_in(c, at, src, n);
    const size_t pieces = sub_pieces(groups, n);
    for (size_t q = 0; q < pieces; q++) {
        const size_t a = piece_cut(n, q, pieces), b = piece_cut(n, q + 1, pieces);
        pool_copy(slot + a, src + a, b - a);
        if (int r = copy_in(c, at + a, slot + a, b - a)) return r;
    }
    return 0;
}

// ---------------------------------------------------------------------------
// host-buffer batched API
// ---------------------------------------------------------------------------
static inline int32_t host_le32(const uint8_t *p)
{
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

// the streams of a mi355lz4_compress_streams / mi355lz4_decompress_dstreams call: every stream continues through its slot of the
// set, whatever group its blocks fall into (null: mi355lz4_compress_batch / mi355lz4_decompress_batch, no set)
template <class Set> struct HostStreams { Set *set; const int32_t *first, *slot; int n; };
// the loaded slot of a mi355lz4_compress_dict call: every block of every group from a copy of it (null: no dictionary)
// (hc: a mi355lz4_compress_hcdict call instead, every block against that prepared dictionary at the engine's level)
// (fast: a mi355lz4_compress_fastdict call, the same object at level 0 with the call's accel)
// (dset: a mi355lz4_compress_fastdict_multi call, block i against member dictIdx[i] of that set; the indices go up with the lengths)
struct HostDict {
    const mi355lz4_cstreams *set; int slot; const mi355lz4_hcdict *hc = nullptr; bool fast = false;
    const mi355lz4_dictset *dset = nullptr; const int32_t *dictIdx = nullptr;
};
// the set of a mi355lz4_compress_streams_fast call, in the place of HostStreams' exact set (null: the exact form)
typedef HostStreams<mi355lz4_fstreams> HostFastStreams;

static int compress_host(mi355lz4_ctx *c, const uint8_t *const *src, const int32_t *srcLen,
                         int nBlocks, int accel, int headerKind, uint8_t *framedOut, size_t cap,
                         size_t *outLen, int32_t *blockFramedLen, int32_t *status, const HostStreams<mi355lz4_cstreams> *hs,
                         const HostDict *hd = nullptr, const HostFastStreams *hf = nullptr)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (nBlocks < 0 || (headerKind != 4 && headerKind != 8) || !outLen)
        return fail(MI355LZ4_E_ARG, "compress_batch: bad arguments");
    *outLen = 0;
    if (nBlocks == 0) return MI355LZ4_OK;
    if (!src || !srcLen || !framedOut) return fail(MI355LZ4_E_ARG, "compress_batch: null pointer");
    HIP_TRY(hipSetDevice(c->device));

    size_t total = 0;
    int maxLen = 0;
    bool contiguous = true;                    // blocks back to back in caller memory, every start 16-aligned
    std::vector<uint64_t> offs((size_t)nBlocks);
    for (int i = 0; i < nBlocks; i++) {
        // compressChunk's size check, Internal/LZ4.hs:237-241 (BlockHasSize limit = LZ4_MAX_INPUT_SIZE)
        if (srcLen[i] < 0 || (unsigned)srcLen[i] > (unsigned)MI355LZ4_MAX_INPUT_SIZE)
            return fail(MI355LZ4_E_ARG, "compress_batch: block %d length %d exceeds the maximum block size", i, srcLen[i]);
        if (srcLen[i] > 0 && !src[i]) return fail(MI355LZ4_E_ARG, "compress_batch: block %d is null", i);
        offs[(size_t)i] = total;
        if (i > 0 && src[i] != src[0] + total) contiguous = false;
        // 16-aligned block starts; back to back for a linked stream (a block's dictionary lies directly in front of it)
        total += (c->linkedCompress && !hs && !hd && !hf) ? (size_t)srcLen[i] : (((size_t)srcLen[i] + 15) & ~(size_t)15);
        if (srcLen[i] > maxLen) maxLen = srcLen[i];
    }
    const size_t stride = mi355lz4_slot_stride_ex(maxLen, headerKind, c->blockChecksum);
    const int trailer = c->blockChecksum ? 4 : 0;

    const std::vector<int> gFirst = cut_groups(srcLen, nBlocks);
    const int G = (int)gFirst.size() - 1;
    size_t maxIn = 0, maxBlocksG = 0;
    for (int g = 0; g < G; g++) {
        const size_t lo = offs[(size_t)gFirst[g]], hi = (gFirst[g + 1] < nBlocks) ? offs[(size_t)gFirst[g + 1]] : total;
        if (hi - lo > maxIn) maxIn = hi - lo;
        if ((size_t)(gFirst[g + 1] - gFirst[g]) > maxBlocksG) maxBlocksG = (size_t)(gFirst[g + 1] - gFirst[g]);
    }
    const bool directIn = contiguous && host_range_is_pinned(src[0], total);
    const bool directOut = host_range_is_pinned(framedOut, cap);

    int r;
    if ((r = pipe_setup(c, directIn, maxIn, directOut, maxBlocksG * stride, (size_t)nBlocks * 4 + (size_t)G * 8))) return r;
    if ((r = dev_reserve(c->in, total + 16)) || (r = dev_reserve(c->offA, (size_t)nBlocks * 8)) || (r = dev_reserve(c->lenA, (size_t)nBlocks * 4)) ||
        (r = dev_reserve(c->lenB, (size_t)nBlocks * 4)) || (r = dev_reserve(c->slots, (size_t)nBlocks * stride)) ||
        (r = dev_reserve(c->dense, (size_t)nBlocks * stride)) || (r = dev_reserve(c->offB, ((size_t)nBlocks + (size_t)G) * 8)))
        return r;
    if (hd && hd->dset && (r = dev_reserve(c->res, (size_t)nBlocks * 4))) return r;

    DrainOnExit drain{c};
    EventSet evs(G);
    std::vector<hipEvent_t> &evIn = evs.in, &evK = evs.k, &evOut = evs.out;
    HIP_TRY(hipMemcpyAsync(c->offA.p, offs.data(), (size_t)nBlocks * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->lenA.p, srcLen, (size_t)nBlocks * 4, hipMemcpyHostToDevice, c->stream));
    if (hd && hd->dset) HIP_TRY(hipMemcpyAsync(c->res.p, hd->dictIdx, (size_t)nBlocks * 4, hipMemcpyHostToDevice, c->stream));
    // offs / srcLen are pageable: make sure the copies have consumed them before they go away
    HIP_TRY(hipStreamSynchronize(c->stream));

    int32_t *flenPin = (int32_t *)c->pinMeta.p;                              // framed length of every block
    uint64_t *totPin = (uint64_t *)((uint8_t *)c->pinMeta.p + (size_t)nBlocks * 4);   // compressed bytes of every group
    std::vector<size_t> outAt((size_t)G, 0), outN((size_t)G, 0);
    size_t outPos = 0;
    int bad = 0;
    bool overflow = false;

    // Phase 1 -- input.  A block takes the encoder ~2 ms whatever else runs (it is latency-bound), and a
    // group of a few hundred blocks fills a fraction of the chip, so the kernels of consecutive groups go to
    // different compute streams and overlap each other as well as the copies.
    for (int g = 0; g < G; g++) {
        const int b0 = gFirst[g], b1 = gFirst[g + 1];
        const size_t lo = offs[(size_t)b0], hi = (b1 < nBlocks) ? offs[(size_t)b1] : total;
        if ((r = evs.make_group(g))) return r;
        if (directIn) {
            if ((r = copy_in(c, lo, src[0] + lo, hi - lo))) return r;
        } else {
            uint8_t *slot = (uint8_t *)c->pinIn.p + (size_t)(g & 1) * (maxIn + 16);
            if (g >= 2) HIP_TRY(hipEventSynchronize(evIn[(size_t)g - 2]));   // the copy that last read this slot
            // (in pieces for a call of one or two groups: the copy engine moves one while the host copies the next, sub_pieces)
            const int pieces = (int)sub_pieces(G, hi - lo);
            for (int q = 0; q < pieces; q++) {
                const int q0 = b0 + (int)((int64_t)(b1 - b0) * q / pieces), q1 = b0 + (int)((int64_t)(b1 - b0) * (q + 1) / pieces);
                if (q1 <= q0) continue;
                const size_t plo = offs[(size_t)q0], phi = (q1 < nBlocks) ? offs[(size_t)q1] : total;
                std::vector<CopyTask> tasks;
                for (int i = q0; i < q1; i++)
                    if (srcLen[i] > 0) tasks.push_back({slot + (offs[(size_t)i] - lo), src[i], (size_t)srcLen[i]});
                pool_run(tasks);
                if (phi > plo && (r = copy_in(c, plo, slot + (plo - lo), phi - plo))) return r;
            }
        }
        HIP_TRY(hipEventRecord(evIn[(size_t)g], c->sIn));
        StreamSwap on(c, c->sK[(c->compExact || hs || hf) ? 0 : (g & 1)]);   // an exact stream's groups follow each other, and a slot's
        HIP_TRY(hipStreamWaitEvent(c->stream, evIn[(size_t)g], 0));
        PTRACE("compress: group %d H2D enqueued (%zu bytes, direct %d)", g, hi - lo, (int)directIn);
        // (a linked stream: the last block of the group before is this group's first dictionary)
        if (hs) {                                  // (a group seam inside a stream: the slot continues in the next group's launch)
            const EncodeArgs a = make_encode_args((const uint8_t *)c->in.p, (const uint64_t *)c->offA.p + b0, (const int32_t *)c->lenA.p + b0,
                                                  0, maxLen, b1 - b0, accel, headerKind, (uint8_t *)c->slots.p + (size_t)b0 * stride,
                                                  stride, (int32_t *)c->lenB.p + b0);
            r = streams_enqueue(c, hs->set, a, b0, b1, hs->first, hs->slot, hs->n);
        } else if (hf) {                           // (the same seam rule; the staging is not contiguous per stream: the kernel stages)
            const EncodeArgs a = make_encode_args((const uint8_t *)c->in.p, (const uint64_t *)c->offA.p + b0, (const int32_t *)c->lenA.p + b0,
                                                  0, maxLen, b1 - b0, accel, headerKind, (uint8_t *)c->slots.p + (size_t)b0 * stride,
                                                  stride, (int32_t *)c->lenB.p + b0);
            r = fstreams_enqueue(c, hf->set, a, b0, b1, hf->first, hf->slot, hf->n);
        } else if (hd && hd->dset) {               // (every block against the member it names; the set and its members only read)
            r = mi355lz4_compress_fastdict_multi_device(c, hd->dset, (const int32_t *)c->res.p + b0, (const uint8_t *)c->in.p,
                                                        (const uint64_t *)c->offA.p + b0, (const int32_t *)c->lenA.p + b0, 0, maxLen,
                                                        b1 - b0, accel, headerKind, (uint8_t *)c->slots.p + (size_t)b0 * stride, stride,
                                                        (int32_t *)c->lenB.p + b0);
        } else if (hd && hd->hc && hd->fast) {     // (the same, by the wave encoder)
            r = mi355lz4_compress_fastdict_device(c, hd->hc, (const uint8_t *)c->in.p, (const uint64_t *)c->offA.p + b0,
                                                  (const int32_t *)c->lenA.p + b0, 0, maxLen, b1 - b0, accel, headerKind,
                                                  (uint8_t *)c->slots.p + (size_t)b0 * stride, stride, (int32_t *)c->lenB.p + b0);
        } else if (hd && hd->hc) {                 // (independent blocks, the image only read, a staging scratch per compute stream)
            r = mi355lz4_compress_hcdict_device(c, hd->hc, (const uint8_t *)c->in.p, (const uint64_t *)c->offA.p + b0,
                                                (const int32_t *)c->lenA.p + b0, 0, maxLen, b1 - b0, headerKind,
                                                (uint8_t *)c->slots.p + (size_t)b0 * stride, stride, (int32_t *)c->lenB.p + b0);
        } else if (hd) {                           // (independent blocks, the slot only read: the groups may overlap)
            r = mi355lz4_compress_dict_device(c, hd->set, hd->slot, (const uint8_t *)c->in.p, (const uint64_t *)c->offA.p + b0,
                                              (const int32_t *)c->lenA.p + b0, 0, maxLen, b1 - b0, accel, headerKind,
                                              (uint8_t *)c->slots.p + (size_t)b0 * stride, stride, (int32_t *)c->lenB.p + b0);
        } else {
            r = encode_device(c, (const uint8_t *)c->in.p, (const uint64_t *)c->offA.p + b0,
                              (const int32_t *)c->lenA.p + b0, 0, maxLen, b1 - b0, accel, headerKind,
                              (uint8_t *)c->slots.p + (size_t)b0 * stride, stride, (int32_t *)c->lenB.p + b0, b0, srcLen + b0);
        }
        if (r) return r;
        uint64_t *goff = (uint64_t *)c->offB.p + b0 + g;                       // b1 - b0 + 1 offsets of this group
        r = mi355lz4_compact_device(c, (const uint8_t *)c->slots.p + (size_t)b0 * stride, stride,
                                    (const int32_t *)c->lenB.p + b0, b1 - b0, (uint8_t *)c->dense.p + (size_t)b0 * stride,
                                    (size_t)(b1 - b0) * stride, goff);
        if (r) return r;
        HIP_TRY(hipMemcpyAsync(flenPin + b0, (const int32_t *)c->lenB.p + b0, (size_t)(b1 - b0) * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(totPin + g, goff + (b1 - b0), 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(evK[(size_t)g], c->stream));
    }
    // Phase 2 -- output, once the last input copy is through: on this link both directions together run
    // at ~39 GB/s each against 57 GB/s for one alone (scripts/pcie_rate.py) and the output is the small
    // side, so it only overlaps the tail of the kernels.  D2H of group t while the pool copies group t-1 out.
    // The output copies go to the INPUT copy stream, behind the last input copy: HIP multiplexes streams onto four
    // hardware queues by default, and the caller's stream, one copy stream and two compute streams use them up.
    // Data that barely compresses sends back as much as it took in: then the two directions do overlap (own stream).
    hipStream_t so = c->sIn;
    for (int t = 0; t < G + 1; t++) {
        if (t < G) {
            const int g = t, b0 = gFirst[g], b1 = gFirst[g + 1];
            HIP_TRY(hipEventSynchronize(evK[(size_t)g]));
            if (g == 0) {
                const size_t in0 = ((gFirst[1] < nBlocks) ? offs[(size_t)gFirst[1]] : total) - offs[0];
                if ((size_t)totPin[0] * 8 > in0 * 5) so = c->sOut;
            }
            PTRACE("compress: group %d kernels done", g);
            for (int i = b0; i < b1; i++) {
                const int32_t f = flenPin[i];
                if (blockFramedLen) blockFramedLen[i] = f;
                if (status) status[i] = (f > headerKind) ? f - headerKind - trailer : 0;
                if (f <= headerKind) bad++;
            }
            outAt[(size_t)g] = outPos;
            outN[(size_t)g] = (size_t)totPin[g];
            outPos += outN[(size_t)g];
            if (outPos > cap) overflow = true;
            if (!bad && !overflow && outN[(size_t)g]) {
                uint8_t *dst = directOut ? framedOut + outAt[(size_t)g] : (uint8_t *)c->pinOut.p + (size_t)(g & 1) * maxBlocksG * stride;
                HIP_TRY(hipMemcpyAsync(dst, (const uint8_t *)c->dense.p + (size_t)b0 * stride, outN[(size_t)g], hipMemcpyDeviceToHost, so));
            }
            HIP_TRY(hipEventRecord(evOut[(size_t)g], so));
        }
        if (t >= 1) {
            const int g = t - 1;
            HIP_TRY(hipEventSynchronize(evOut[(size_t)g]));
            PTRACE("compress: group %d D2H done (%zu bytes)", g, outN[(size_t)g]);
            if (!directOut && !bad && !overflow && outN[(size_t)g])
                pool_copy(framedOut + outAt[(size_t)g], (const uint8_t *)c->pinOut.p + (size_t)(g & 1) * maxBlocksG * stride, outN[(size_t)g]);
        }
    }
    if (bad) return fail(MI355LZ4_E_BLOCK, "compress_batch: %d block(s) failed", bad);
    if (overflow) return fail(MI355LZ4_E_CAPACITY, "compress_batch: need %llu bytes, have %zu", (unsigned long long)outPos, cap);
    *outLen = outPos;
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_compress_batch(mi355lz4_ctx *c, const uint8_t *const *src, const int32_t *srcLen,
                                       int nBlocks, int accel, int headerKind, uint8_t *framedOut, size_t cap,
                                       size_t *outLen, int32_t *blockFramedLen, int32_t *status)
{
    return compress_host(c, src, srcLen, nBlocks, accel, headerKind, framedOut, cap, outLen, blockFramedLen, status, nullptr);
}

// Host-buffer form of mi355lz4_compress_streams_device: the group pipeline of mi355lz4_compress_batch, its groups one behind
// the other on one compute stream like an exact call's.  The lengths are the caller's host array: checked before anything is queued.
extern "C" int mi355lz4_compress_streams(mi355lz4_ctx *c, mi355lz4_cstreams *cs, const uint8_t *const *src,
                                         const int32_t *srcLen, int nBlocks, const int32_t *streamFirst,
                                         const int32_t *streamSlot, int nStreams, int accel, int headerKind,
                                         uint8_t *framedOut, size_t cap, size_t *outLen, int32_t *blockFramedLen,
                                         int32_t *status)
{
    if (outLen) *outLen = 0;
    const int r = streams_check(c, cs, nBlocks, streamFirst, streamSlot, nStreams, "compress_streams");
    if (r) return r;
    const HostStreams<mi355lz4_cstreams> hs{cs, streamFirst, streamSlot, nStreams};
    return compress_host(c, src, srcLen, nBlocks, accel, headerKind, framedOut, cap, outLen, blockFramedLen, status, &hs);
}

// Host-buffer form of mi355lz4_compress_streams_fast_device: the same pipeline, the groups one behind the other on one compute
// stream (a group's first blocks read the slots the group before saved).  The lengths are the caller's host array: checked before
// anything is queued.
extern "C" int mi355lz4_compress_streams_fast(mi355lz4_ctx *c, mi355lz4_fstreams *fs, const uint8_t *const *src,
                                              const int32_t *srcLen, int nBlocks, const int32_t *streamFirst,
                                              const int32_t *streamSlot, int nStreams, int accel, int headerKind,
                                              uint8_t *framedOut, size_t cap, size_t *outLen, int32_t *blockFramedLen,
                                              int32_t *status)
{
    if (outLen) *outLen = 0;
    int r = fstreams_check(c, fs, nBlocks, streamFirst, streamSlot, nStreams, "compress_streams_fast");
    if (r) return r;
    int maxLen = 0;
    for (int i = 0; srcLen && i < nBlocks; i++) {
        if (srcLen[i] < 0 || srcLen[i] > HCDICT_MAX_BLOCK)
            return fail(MI355LZ4_E_ARG, "compress_streams_fast: block %d length %d outside 0..%d", i, srcLen[i], HCDICT_MAX_BLOCK);
        if (srcLen[i] > maxLen) maxLen = srcLen[i];
    }
    if ((r = dict_batch_shape_check("compress_streams_fast", "a fast stream's block", nBlocks, headerKind, maxLen))) return r;
    const HostFastStreams hf{fs, streamFirst, streamSlot, nStreams};
    return compress_host(c, src, srcLen, nBlocks, accel, headerKind, framedOut, cap, outLen, blockFramedLen, status, nullptr, nullptr, &hf);
}

// Host-buffer form of mi355lz4_compress_dict_device: the group pipeline of mi355lz4_compress_batch, every group's blocks from a
// copy of the loaded slot.  The lengths are the caller's host array: checked before anything is queued.
extern "C" int mi355lz4_compress_dict(mi355lz4_ctx *c, const mi355lz4_cstreams *cs, int dictSlot, const uint8_t *const *src,
                                      const int32_t *srcLen, int nBlocks, int accel, int headerKind, uint8_t *framedOut,
                                      size_t cap, size_t *outLen, int32_t *blockFramedLen, int32_t *status)
{
    if (outLen) *outLen = 0;
    if (!c || !cs) return fail(MI355LZ4_E_ARG, "compress_dict: null argument");
    if (mi355lz4_cstreams_count(cs) <= dictSlot || dictSlot < 0) return fail(MI355LZ4_E_ARG, "compress_dict: slot %d out of range", dictSlot);
    if (engine_compression_level(c) != 0)
        return fail(MI355LZ4_E_ARG, "compress_dict: compression level %d; the dictionary batch is level 0's encoder", engine_compression_level(c));
    const HostDict hd{cs, dictSlot};
    return compress_host(c, src, srcLen, nBlocks, accel, headerKind, framedOut, cap, outLen, blockFramedLen, status, nullptr, &hd);
}

// Host-buffer form of mi355lz4_compress_hcdict_device: the same pipeline, every group's blocks against the prepared dictionary at the
// engine's level (1..12).  The lengths are the caller's host array: checked before anything is queued.
extern "C" int mi355lz4_compress_hcdict(mi355lz4_ctx *c, const mi355lz4_hcdict *hcd, const uint8_t *const *src,
                                        const int32_t *srcLen, int nBlocks, int headerKind, uint8_t *framedOut, size_t cap,
                                        size_t *outLen, int32_t *blockFramedLen, int32_t *status)
{
    if (outLen) *outLen = 0;
    if (!c || !hcd) return fail(MI355LZ4_E_ARG, "compress_hcdict: null argument");
    if (engine_compression_level(c) < 1)
        return fail(MI355LZ4_E_ARG, "compress_hcdict: compression level %d; level 0 against a dictionary is mi355lz4_compress_dict",
                    engine_compression_level(c));
    for (int i = 0; srcLen && i < nBlocks; i++)
        if (srcLen[i] < 0 || srcLen[i] > HCDICT_MAX_BLOCK)
            return fail(MI355LZ4_E_ARG, "compress_hcdict: block %d length %d outside 0..%d", i, srcLen[i], HCDICT_MAX_BLOCK);
    HostDict hd{nullptr, 0};
    hd.hc = hcd;
    return compress_host(c, src, srcLen, nBlocks, 0, headerKind, framedOut, cap, outLen, blockFramedLen, status, nullptr, &hd);
}

// Host-buffer form of mi355lz4_compress_fastdict_device: the same pipeline, every group's blocks against the prepared dictionary by
// the wave encoder (level 0).  The lengths are the caller's host array: checked before anything is queued.
extern "C" int mi355lz4_compress_fastdict(mi355lz4_ctx *c, const mi355lz4_hcdict *hcd, const uint8_t *const *src,
                                          const int32_t *srcLen, int nBlocks, int accel, int headerKind, uint8_t *framedOut,
                                          size_t cap, size_t *outLen, int32_t *blockFramedLen, int32_t *status)
{
    if (outLen) *outLen = 0;
    if (!c || !hcd) return fail(MI355LZ4_E_ARG, "compress_fastdict: null argument");
    if (engine_compression_level(c) != 0)
        return fail(MI355LZ4_E_ARG, "compress_fastdict: compression level %d; levels 1..12 against a dictionary are mi355lz4_compress_hcdict",
                    engine_compression_level(c));
    for (int i = 0; srcLen && i < nBlocks; i++)
        if (srcLen[i] < 0 || srcLen[i] > HCDICT_MAX_BLOCK)
            return fail(MI355LZ4_E_ARG, "compress_fastdict: block %d length %d outside 0..%d", i, srcLen[i], HCDICT_MAX_BLOCK);
    HostDict hd{nullptr, 0};
    hd.hc = hcd;
    hd.fast = true;
    return compress_host(c, src, srcLen, nBlocks, accel, headerKind, framedOut, cap, outLen, blockFramedLen, status, nullptr, &hd);
}

// Host-buffer form of mi355lz4_compress_fastdict_multi_device: the same pipeline, block i against member dictIdx[i] of the set (-1:
// none).  The indices and the lengths are the caller's host arrays: checked before anything is queued.
extern "C" int mi355lz4_compress_fastdict_multi(mi355lz4_ctx *c, const mi355lz4_dictset *ds, const int32_t *dictIdx,
                                                const uint8_t *const *src, const int32_t *srcLen, int nBlocks, int accel,
                                                int headerKind, uint8_t *framedOut, size_t cap, size_t *outLen,
                                                int32_t *blockFramedLen, int32_t *status)
{
    if (outLen) *outLen = 0;
    if (!c || !ds) return fail(MI355LZ4_E_ARG, "compress_fastdict_multi: null argument");
    if (engine_compression_level(c) != 0)
        return fail(MI355LZ4_E_ARG, "compress_fastdict_multi: compression level %d; a dictionary set is level 0's encoder",
                    engine_compression_level(c));
    if (nBlocks > 0 && !dictIdx) return fail(MI355LZ4_E_ARG, "compress_fastdict_multi: null dictIdx");
    const int nDicts = mi355lz4_dictset_count(ds);
    for (int i = 0; i < nBlocks; i++)
        if (dictIdx[i] < -1 || dictIdx[i] >= nDicts)
            return fail(MI355LZ4_E_ARG, "compress_fastdict_multi: block %d names dictionary %d of %d", i, dictIdx[i], nDicts);
    for (int i = 0; srcLen && i < nBlocks; i++)
        if (srcLen[i] < 0 || srcLen[i] > HCDICT_MAX_BLOCK)
            return fail(MI355LZ4_E_ARG, "compress_fastdict_multi: block %d length %d outside 0..%d", i, srcLen[i], HCDICT_MAX_BLOCK);
    HostDict hd{nullptr, 0};
    hd.dset = ds;
    hd.dictIdx = dictIdx;
    return compress_host(c, src, srcLen, nBlocks, accel, headerKind, framedOut, cap, outLen, blockFramedLen, status, nullptr, &hd);
}

extern "C" int mi355lz4_index_host_ex(const uint8_t *framedIn, size_t inLen, int headerKind, int fixedUncomp,
                                      int blockChecksum, uint64_t *blockOff, int32_t *uncompLen, int maxBlocks, int *nBlocks)
{
    const size_t trailer = blockChecksum ? 4u : 0u;
    if (!nBlocks || (headerKind != 4 && headerKind != 8) || maxBlocks < 0 || (inLen && !framedIn))
        return fail(MI355LZ4_E_ARG, "index_host: bad arguments");
    size_t pos = 0;
    int k = 0;
    *nBlocks = 0;
    while (pos < inLen) {
        if (pos + (size_t)headerKind > inLen)
            return fail(MI355LZ4_E_STREAM, "index_host: incomplete block header at offset %zu", pos);
        const int32_t cl = host_le32(framedIn + pos);
        const int32_t ul = (headerKind == 8) ? host_le32(framedIn + pos + 4) : fixedUncomp;
        if (cl <= 0) return fail(MI355LZ4_E_STREAM, "index_host: block %d has compressed length %d", k, cl);
        if (pos + (size_t)headerKind + (size_t)cl + trailer > inLen)
            return fail(MI355LZ4_E_STREAM, "index_host: incomplete block %d (needs %zu bytes)", k, (size_t)cl + trailer);
        if (k >= maxBlocks) return fail(MI355LZ4_E_CAPACITY, "index_host: more than %d blocks", maxBlocks);
        if (blockOff) blockOff[k] = pos;
        if (uncompLen) uncompLen[k] = ul;
        pos += (size_t)headerKind + (size_t)cl + trailer;
        k++;
    }
    *nBlocks = k;
    return MI355LZ4_OK;
}
extern "C" int mi355lz4_index_host(const uint8_t *framedIn, size_t inLen, int headerKind, int fixedUncomp,
                                   uint64_t *blockOff, int32_t *uncompLen, int maxBlocks, int *nBlocks)
{
    return mi355lz4_index_host_ex(framedIn, inLen, headerKind, fixedUncomp, 0, blockOff, uncompLen, maxBlocks, nBlocks);
}

// A chain of blocks in host memory, indexed, and its output layout: block i at ooff[i], ooff[n] = total
struct HostChain {
    std::vector<uint64_t> boff, ooff;
    std::vector<int32_t> ulen;
    int n = 0;
    uint64_t total = 0;
};
// Index the chain (at most maxBlocks blocks) and lay it out back to back, block i taking width(i, ulen[i]) bytes.  `who` names the
// call in the messages; a negative size is `malformed` (MI355LZ4_E_STREAM; the dstreams call says MI355LZ4_E_ARG, also for a
// chain the indexer calls MI355LZ4_E_STREAM).
template <class Width>
static int host_chain(HostChain &h, const char *who, int malformed, const uint8_t *framedIn, size_t inLen, int headerKind,
                      int fixedUncomp, int blockChecksum, int maxBlocks, Width width)
{
    h.boff.resize((size_t)maxBlocks + 1);
    h.ulen.resize((size_t)maxBlocks + 1);
    const int r = mi355lz4_index_host_ex(framedIn, inLen, headerKind, fixedUncomp, blockChecksum, h.boff.data(), h.ulen.data(), maxBlocks, &h.n);
    if (r == MI355LZ4_E_STREAM && malformed != r) return fail(malformed, "%s: %s", who, std::string(mi355lz4_last_error()).c_str());
    if (r) return r;
    h.ooff.resize((size_t)h.n + 1);
    h.total = 0;
    for (int i = 0; i < h.n; i++) {
        if (h.ulen[(size_t)i] < 0) return fail(malformed, "%s: block %d has negative size", who, i);
        h.ooff[(size_t)i] = h.total;
        h.total += (uint64_t)width(i, h.ulen[(size_t)i]);
    }
    h.ooff[(size_t)h.n] = h.total;
    return MI355LZ4_OK;
}
static int32_t at_capacity(int, int32_t ulen) { return ulen; }     // blocks back to back at their header (or fixed) capacity

// The end of a synchronous decode: the results are in c->res, block i's bytes at h.ooff[i] of c->out.  Packs the decoded blocks
// back to back into out (a block may decode to fewer bytes than its place) -- in one copy when every block filled its place,
// else block by block.
static int host_tail(mi355lz4_ctx *c, const char *who, const HostChain &h, uint8_t *out, size_t cap, size_t *outLen,
                     int32_t *blockLen, int *nBlocksOut)
{
    const int n = h.n;
    std::vector<int32_t> res((size_t)n);
    HIP_TRY(hipMemcpyAsync(res.data(), c->res.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int bad = 0, r;
    uint64_t need = 0;
    for (int i = 0; i < n; i++) {
        if (blockLen) blockLen[i] = res[(size_t)i];
        if (res[(size_t)i] < 0) bad++; else need += (uint64_t)res[(size_t)i];
    }
    *nBlocksOut = n;
    // The capacity is judged after the decode, also where the size pass has already said what the call needs: a size
    // vouches for the chain, not for the offsets, so a block of known size can still fail in the decoder, and a call with a
    // failed block returns E_BLOCK with its blockLen[] whether or not the output would have fitted.
    if (bad) return fail(MI355LZ4_E_BLOCK, "%s: %d block(s) failed", who, bad);
    if (need > cap) return fail(MI355LZ4_E_CAPACITY, "%s: need %llu bytes, have %zu", who, (unsigned long long)need, cap);
    if (need && !out) return fail(MI355LZ4_E_ARG, "%s: null output", who);
    if (need == h.total) {
        if ((r = d2h_staged(c, out, c->out.p, (size_t)h.total))) return r;
    } else {
        uint64_t w = 0;
        for (int i = 0; i < n; i++) {
            if (res[(size_t)i] > 0)
                HIP_TRY(hipMemcpyAsync(out + w, (const uint8_t *)c->out.p + h.ooff[(size_t)i], (size_t)res[(size_t)i],
                                       hipMemcpyDeviceToHost, c->stream));
            w += (uint64_t)res[(size_t)i];
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    *outLen = (size_t)need;
    return MI355LZ4_OK;
}

// One stream, output laid out at capacity offsets: groups of blocks flow through H2D -> decode (-> linked
// fixup of the group, which looks back into the groups before it) -> D2H on three streams.
static int decompress_host_pipelined(mi355lz4_ctx *c, const uint8_t *framedIn, size_t inLen, int headerKind,
                                     int fixedUncomp, int linked, const uint8_t *dict, int dictLen, const HostChain &h,
                                     uint8_t *out, size_t *outLen, int32_t *blockLen, int *nBlocksOut,
                                     const HostStreams<mi355lz4_dstreams> *hs = nullptr)
{
    const std::vector<uint64_t> &boff = h.boff, &ooff = h.ooff;
    const int n = h.n;
    const std::vector<int> gFirst = cut_groups(h.ulen.data(), n);
    const int G = (int)gFirst.size() - 1;
    auto in_lo = [&](int b) -> size_t { return (b < n) ? (size_t)boff[(size_t)b] : inLen; };
    size_t maxIn = 0, maxOut = 0;
    for (int g = 0; g < G; g++) {
        maxIn = std::max(maxIn, in_lo(gFirst[g + 1]) - in_lo(gFirst[g]));
        maxOut = std::max(maxOut, (size_t)(ooff[(size_t)gFirst[g + 1]] - ooff[(size_t)gFirst[g]]));
    }
    const bool directIn = host_range_is_pinned(framedIn, inLen);
    const bool directOut = host_range_is_pinned(out, (size_t)h.total);
    int r;
    if ((r = pipe_setup(c, directIn, maxIn, directOut, maxOut + 16, (size_t)n * 4))) return r;
    if ((r = dev_reserve(c->in, inLen + 16)) || (r = dev_reserve(c->out, (size_t)h.total + 16)) || (r = dev_reserve(c->offA, (size_t)n * 8)) ||
        (r = dev_reserve(c->offB, ((size_t)n + 1) * 8)) || (r = dev_reserve(c->res, (size_t)n * 4)))
        return r;

    DrainOnExit drain{c};
    EventSet evs(G);
    std::vector<hipEvent_t> &evIn = evs.in, &evK = evs.k, &evOut = evs.out;
    uint32_t dlen = 0;
    if ((r = upload_dict(c, linked, dict, dictLen, &dlen))) return r;
    // (boff / ooff outlive everything this call enqueues -- it drains its streams before it returns --, and the kernels that read the
    // device copies are ordered behind these on the same stream: no wait here)
    HIP_TRY(hipMemcpyAsync(c->offA.p, boff.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->offB.p, ooff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));

    int32_t *resPin = (int32_t *)c->pinMeta.p;
    std::vector<std::vector<hipEvent_t>> evPiece((size_t)G);      // device-to-host copy in pieces (small calls): an event behind every piece but the last
    // input copy of group g: enqueued one group AHEAD of its kernels, because a linked decode waits on the
    // host for its first pass (decode_device) and the copy engine should be busy meanwhile
    auto stage_in = [&](int g) -> int {
        const int b0 = gFirst[g], b1 = gFirst[g + 1];
        const size_t lo = in_lo(b0), hi = in_lo(b1);
        int rr;
        if ((rr = evs.make_group(g))) return rr;
        if (!directIn && g >= 2) HIP_TRY(hipEventSynchronize(evIn[(size_t)g - 2]));   // the copy that last read this slot
        if ((rr = stage_range(c, lo, framedIn + lo, hi - lo, directIn ? nullptr : (uint8_t *)c->pinIn.p + (size_t)(g & 1) * (maxIn + 16), G)))
            return rr;
        HIP_TRY(hipEventRecord(evIn[(size_t)g], c->sIn));
        return 0;
    };
    if (G > 0 && (r = stage_in(0))) return r;
    for (int t = 0; t < G + 1; t++) {
        if (t < G) {                                                           // ---- stage A, group t
            const int g = t, b0 = gFirst[g], b1 = gFirst[g + 1];
            if (linked && g + 1 < G && (r = stage_in(g + 1))) return r;
            HIP_TRY(hipStreamWaitEvent(c->stream, evIn[(size_t)g], 0));
            // the group's blocks, with the whole framed buffer as bounds and the blocks before it as look-back
            DecodeCall d{(const uint8_t *)c->in.p, inLen, (const uint64_t *)c->offA.p + b0, b1 - b0, headerKind, fixedUncomp, linked,
                         (uint8_t *)c->out.p, (const uint64_t *)c->offB.p + b0, nullptr, (int32_t *)c->res.p + b0};
            d.dict0 = dlen ? (const uint8_t *)c->scratch.p : nullptr; d.dict0Len = dlen; d.lookBack = b0;
            // (many streams: each continues through its slot, so a group seam inside a stream needs no look-back)
            r = hs ? dstreams_enqueue(c, hs->set, d, b0, b1, hs->first, hs->slot, hs->n) : decode_device(c, d);
            if (r) return r;
            HIP_TRY(hipMemcpyAsync(resPin + b0, (const int32_t *)c->res.p + b0, (size_t)(b1 - b0) * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipEventRecord(evK[(size_t)g], c->stream));
            HIP_TRY(hipStreamWaitEvent(c->sOut, evK[(size_t)g], 0));
            const size_t olo = (size_t)ooff[(size_t)b0], ohi = (size_t)ooff[(size_t)b1];
            if (ohi > olo) {
                if (directOut) {
                    HIP_TRY(hipMemcpyAsync(out + olo, (const uint8_t *)c->out.p + olo, ohi - olo, hipMemcpyDeviceToHost, c->sOut));
                } else {
                    // slot g & 1 was emptied by stage C of group g - 2, one iteration ago
                    uint8_t *slot = (uint8_t *)c->pinOut.p + (size_t)(g & 1) * (maxOut + 16);
                    const size_t pieces = sub_pieces(G, ohi - olo);
                    for (size_t q = 0; q < pieces; q++) {
                        const size_t a = piece_cut(ohi - olo, q, pieces), b = piece_cut(ohi - olo, q + 1, pieces);
                        HIP_TRY(hipMemcpyAsync(slot + a, (const uint8_t *)c->out.p + olo + a, b - a, hipMemcpyDeviceToHost, c->sOut));
                        if (q + 1 < pieces) {
                            hipEvent_t e;
                            if ((r = evs.make(&e))) return r;
                            HIP_TRY(hipEventRecord(e, c->sOut));
                            evPiece[(size_t)g].push_back(e);
                        }
                    }
                }
            }
            HIP_TRY(hipEventRecord(evOut[(size_t)g], c->sOut));
        }
        if (t >= 1) {                                                          // ---- stage C, group t-1
            const int g = t - 1, b0 = gFirst[g], b1 = gFirst[g + 1];
            const size_t olo = (size_t)ooff[(size_t)b0], ohi = (size_t)ooff[(size_t)b1];
            const size_t pieces = evPiece[(size_t)g].size() + 1;
            for (size_t q = 0; q < pieces; q++) {
                // (the last piece's event is the group's: the results' copy and every piece lie in front of it)
                HIP_TRY(hipEventSynchronize(q + 1 < pieces ? evPiece[(size_t)g][q] : evOut[(size_t)g]));
                if (!directOut && ohi > olo) {
                    const uint8_t *slot = (const uint8_t *)c->pinOut.p + (size_t)(g & 1) * (maxOut + 16);
                    const size_t a = piece_cut(ohi - olo, q, pieces), b = piece_cut(ohi - olo, q + 1, pieces);
                    if (b > a) pool_copy(out + olo + a, slot + a, b - a);
                }
            }
        }
        if (!linked && t + 1 < G && (r = stage_in(t + 1))) return r;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));

    int bad = 0;
    bool full = true;
    uint64_t need = 0;
    for (int i = 0; i < n; i++) {
        const int32_t ri = resPin[i];
        if (blockLen) blockLen[i] = ri;
        if (ri < 0) bad++; else need += (uint64_t)ri;
        if (ri != h.ulen[(size_t)i]) full = false;
    }
    *nBlocksOut = n;
    if (bad) return fail(MI355LZ4_E_BLOCK, "decompress_batch: %d block(s) failed", bad);
    if (!full) {
        // a block may decode to fewer bytes than its capacity: pack the blocks back to back, in place
        uint64_t w = 0;
        for (int i = 0; i < n; i++) {
            const uint64_t len = (uint64_t)resPin[i];
            if (len && w != ooff[(size_t)i]) memmove(out + w, out + ooff[(size_t)i], (size_t)len);
            w += len;
        }
    }
    *outLen = (size_t)need;
    return MI355LZ4_OK;
}

// mi355lz4_decompress_batch (one stream, linked or not, maybe a dictionary) and mi355lz4_decompress_streams (a stream table)
static int decompress_host(mi355lz4_ctx *c, const uint8_t *framedIn, size_t inLen, int headerKind, int fixedUncomp, int linked,
                           const uint8_t *dict, int dictLen, const int32_t *streamFirst, int nStreams, uint8_t *out, size_t cap,
                           size_t *outLen, int32_t *blockLen, int maxBlocks, int *nBlocksOut)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (!outLen || !nBlocksOut || maxBlocks < 0) return fail(MI355LZ4_E_ARG, "decompress_batch: bad arguments");
    *outLen = 0;
    *nBlocksOut = 0;
    HostChain h;
    int r = host_chain(h, "decompress_batch", MI355LZ4_E_STREAM, framedIn, inLen, headerKind, fixedUncomp, c->blockChecksum, maxBlocks, at_capacity);
    if (r) return r;
    const int n = h.n;
    if (n == 0) return MI355LZ4_OK;
    HIP_TRY(hipSetDevice(c->device));
    // the pipelined path writes every block at its capacity offset: it needs room for that layout and one stream
    if (!streamFirst && cap >= h.total && h.total > 0)
        return decompress_host_pipelined(c, framedIn, inLen, headerKind, fixedUncomp, linked, dict, dictLen, h, out, outLen,
                                         blockLen, nBlocksOut);
    if ((r = dev_reserve(c->in, inLen + 16)) || (r = dev_reserve(c->offA, (size_t)n * 8)) || (r = dev_reserve(c->offB, ((size_t)n + 1) * 8)) ||
        (r = dev_reserve(c->res, (size_t)n * 4)))
        return r;
    uint32_t dlen = 0;
    if ((r = upload_dict(c, linked, dict, dictLen, &dlen))) return r;
    if ((r = h2d_staged(c, c->in.p, framedIn, inLen))) return r;
    HIP_TRY(hipMemcpyAsync(c->offA.p, h.boff.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    // Blocks without a size in their header: the token chains say what every block decodes to (size_walk.hpp).  When every
    // size is known the output is laid out back to back at those sizes -- sum(size) device bytes instead of
    // n * fixedUncomp, one copy back instead of one per block -- and each block is decoded into exactly its size, which
    // by the size pass's acceptance rule gives what decoding into fixedUncomp gives.  One block without a known size
    // (malformed, or larger than fixedUncomp) and the whole call is laid out at fixedUncomp, as before.
    const int32_t *capDev = nullptr;
    if (headerKind == 4) {
        if ((r = dev_reserve(c->lenB, (size_t)n * 4))) return r;
        launch_decoded_size((const uint8_t *)c->in.p, inLen, (const uint64_t *)c->offA.p, n, headerKind, fixedUncomp,
                            c->blockChecksum, (int32_t *)c->lenB.p, nullptr, c->stream);
        if ((r = check_launch("size launch"))) return r;
        std::vector<int32_t> sz((size_t)n);
        HIP_TRY(hipMemcpyAsync(sz.data(), c->lenB.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        bool known = true;
        for (int i = 0; i < n && known; i++) known = sz[(size_t)i] >= 0;
        if (known) {
            h.total = 0;
            for (int i = 0; i < n; i++) { h.ooff[(size_t)i] = h.total; h.total += (uint64_t)sz[(size_t)i]; }
            h.ooff[(size_t)n] = h.total;
            capDev = (const int32_t *)c->lenB.p;
        }
    }
    if ((r = dev_reserve(c->out, (size_t)h.total + 16))) return r;
    HIP_TRY(hipMemcpyAsync(c->offB.p, h.ooff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int32_t *sfDev = nullptr;
    if (streamFirst) {
        if (nStreams == 0 || streamFirst[nStreams] > n)
            return fail(MI355LZ4_E_ARG, "decompress_streams: the stream table names block %d of %d", nStreams ? streamFirst[nStreams] : 0, n);
        if ((r = dev_reserve(c->lenA, ((size_t)nStreams + 1) * 4))) return r;
        HIP_TRY(hipMemcpyAsync(c->lenA.p, streamFirst, ((size_t)nStreams + 1) * 4, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        sfDev = (const int32_t *)c->lenA.p;
    }
    DecodeCall d{(const uint8_t *)c->in.p, inLen, (const uint64_t *)c->offA.p, n, headerKind, fixedUncomp, linked,
                 (uint8_t *)c->out.p, (const uint64_t *)c->offB.p, capDev, (int32_t *)c->res.p};
    d.dict0 = dlen ? (const uint8_t *)c->scratch.p : nullptr; d.dict0Len = dlen; d.streamFirst = sfDev; d.nStreams = nStreams;
    if ((r = decode_device(c, d))) return r;
    return host_tail(c, "decompress_batch", h, out, cap, outLen, blockLen, nBlocksOut);
}

extern "C" int mi355lz4_decompress_batch(mi355lz4_ctx *c, const uint8_t *framedIn, size_t inLen, int headerKind,
                                         int fixedUncomp, int linked, const uint8_t *dict, int dictLen,
                                         uint8_t *out, size_t cap, size_t *outLen, int32_t *blockLen,
                                         int maxBlocks, int *nBlocksOut)
{
    return decompress_host(c, framedIn, inLen, headerKind, fixedUncomp, linked, dict, dictLen, nullptr, 0, out, cap,
                           outLen, blockLen, maxBlocks, nBlocksOut);
}

extern "C" int mi355lz4_decompress_streams(mi355lz4_ctx *c, const uint8_t *framedIn, size_t inLen, int headerKind,
                                           int fixedUncomp, const int32_t *streamFirst, int nStreams,
                                           uint8_t *out, size_t cap, size_t *outLen, int32_t *blockLen,
                                           int maxBlocks, int *nBlocksOut)
{
    if (nStreams < 0 || (nStreams > 0 && !streamFirst))
        return fail(MI355LZ4_E_ARG, "decompress_streams: bad stream table");
    for (int s = 0; s < nStreams; s++)
        if (streamFirst[s] < 0 || streamFirst[s + 1] < streamFirst[s])
            return fail(MI355LZ4_E_ARG, "decompress_streams: stream table is not ascending at %d", s);
    return decompress_host(c, framedIn, inLen, headerKind, fixedUncomp, 1, nullptr, 0, streamFirst, nStreams, out, cap,
                           outLen, blockLen, maxBlocks, nBlocksOut);
}

// Host-buffer form of mi355lz4_decompress_dstreams_device: the group pipeline of mi355lz4_decompress_batch, every group's
// streams continuing their slots.  The chain is walked on the host: a bad length is MI355LZ4_E_ARG before anything is queued.
extern "C" int mi355lz4_decompress_dstreams(mi355lz4_ctx *c, mi355lz4_dstreams *ds, const uint8_t *framedIn, size_t inLen,
                                            int headerKind, int fixedUncomp, const int32_t *streamFirst,
                                            const int32_t *streamSlot, int nStreams, uint8_t *out, size_t cap, size_t *outLen,
                                            int32_t *blockLen, int maxBlocks, int *nBlocksOut)
{
    if (outLen) *outLen = 0;
    if (nBlocksOut) *nBlocksOut = 0;
    if (!c || !ds) return fail(MI355LZ4_E_ARG, "decompress_dstreams: null argument");
    if (!outLen || !nBlocksOut || maxBlocks < 0 || fixedUncomp < 0 || (headerKind != 4 && headerKind != 8))
        return fail(MI355LZ4_E_ARG, "decompress_dstreams: bad arguments");
    HostChain h;
    int r = host_chain(h, "decompress_dstreams", MI355LZ4_E_ARG, framedIn, inLen, headerKind, fixedUncomp, c->blockChecksum, maxBlocks, at_capacity);
    if (r) return r;
    const int n = h.n;
    if ((r = dstreams_check(c, ds, n, streamFirst, streamSlot, nStreams, "decompress_dstreams"))) return r;
    if (n == 0) return MI355LZ4_OK;
    // every block is written at its capacity offset (the header's size, or fixedUncomp) before the results are known
    if (cap < h.total) return fail(MI355LZ4_E_CAPACITY, "decompress_dstreams: need %llu bytes, have %zu", (unsigned long long)h.total, cap);
    if (h.total && !out) return fail(MI355LZ4_E_ARG, "decompress_dstreams: null output");
    HIP_TRY(hipSetDevice(c->device));
    const HostStreams<mi355lz4_dstreams> hs{ds, streamFirst, streamSlot, nStreams};
    return decompress_host_pipelined(c, framedIn, inLen, headerKind, fixedUncomp, 0, nullptr, 0, h, out, outLen, blockLen, nBlocksOut, &hs);
}

// The first target[k] (or targetAll) bytes of every block of a chain in host memory.  One group, synchronous: the whole chain goes up,
// one partial decode lays the prefixes out back to back at min(target, capacity), and only they come back -- in one copy when every
// block gave all it was asked for, else block by block.
extern "C" int mi355lz4_decompress_partial(mi355lz4_ctx *c, const uint8_t *framedIn, size_t inLen, int headerKind,
                                           int fixedUncomp, const int32_t *target, int targetAll, uint8_t *out, size_t cap,
                                           size_t *outLen, int32_t *blockLen, int maxBlocks, int *nBlocksOut)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (!outLen || !nBlocksOut || maxBlocks < 0 || fixedUncomp < 0 || (headerKind != 4 && headerKind != 8))
        return fail(MI355LZ4_E_ARG, "decompress_partial: bad arguments");
    if (c->plan.active) return fail(MI355LZ4_E_ARG, "a linked decode begun with mi355lz4_decompress_linked_begin is still open");
    *outLen = 0;
    *nBlocksOut = 0;
    // device layout: block k's prefix at scan(min(target, capacity)) -- what the call may write of it and no more
    HostChain h;
    int r = host_chain(h, "decompress_partial", MI355LZ4_E_STREAM, framedIn, inLen, headerKind, fixedUncomp, c->blockChecksum, maxBlocks,
                       [&](int i, int32_t ulen) { const int32_t t = target ? target[i] : targetAll; return t > 0 ? std::min(t, ulen) : 0; });
    if (r) return r;
    const int n = h.n;
    if (n == 0) return MI355LZ4_OK;
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int32_t> tgt((size_t)n, targetAll);
    if (target) std::copy(target, target + n, tgt.begin());
    if ((r = dev_reserve(c->in, inLen + 16)) || (r = dev_reserve(c->offA, (size_t)n * 8)) || (r = dev_reserve(c->offB, ((size_t)n + 1) * 8)) ||
        (r = dev_reserve(c->res, (size_t)n * 4)) || (r = dev_reserve(c->lenA, (size_t)n * 4)) || (r = dev_reserve(c->out, (size_t)h.total + 16)))
        return r;
    if ((r = h2d_staged(c, c->in.p, framedIn, inLen))) return r;
    HIP_TRY(hipMemcpyAsync(c->offA.p, h.boff.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->offB.p, h.ooff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->lenA.p, tgt.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // (the vectors are pageable memory)
    r = mi355lz4_decompress_partial_device(c, (const uint8_t *)c->in.p, inLen, (const uint64_t *)c->offA.p, n, headerKind, fixedUncomp,
                                           (uint8_t *)c->out.p, (const uint64_t *)c->offB.p, nullptr, (const int32_t *)c->lenA.p,
                                           (int32_t *)c->res.p);
    if (r) return r;
    return host_tail(c, "decompress_partial", h, out, cap, outLen, blockLen, nBlocksOut);
}

// Independent blocks of a chain in host memory against one dictionary in host memory (mi355lz4_decompress_dict_device).  One group,
// synchronous, as the partial form: the chain and the dictionary's last 64 KiB go up (keeping exactly 64 KiB of a longer one
// preserves "dictSize >= 64 KB => no offset check", upload_dict), one decode lays the blocks out at their capacities, one copy back.
extern "C" int mi355lz4_decompress_dict(mi355lz4_ctx *c, const uint8_t *framedIn, size_t inLen, int headerKind, int fixedUncomp,
                                        const uint8_t *dict, int dictLen, uint8_t *out, size_t cap, size_t *outLen,
                                        int32_t *blockLen, int maxBlocks, int *nBlocksOut)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (!outLen || !nBlocksOut || maxBlocks < 0 || fixedUncomp < 0 || (headerKind != 4 && headerKind != 8))
        return fail(MI355LZ4_E_ARG, "decompress_dict: bad arguments");
    if (dictLen < 0 || (dictLen > 0 && !dict)) return fail(MI355LZ4_E_ARG, "decompress_dict: bad dictionary");
    if (c->plan.active) return fail(MI355LZ4_E_ARG, "a linked decode begun with mi355lz4_decompress_linked_begin is still open");
    *outLen = 0;
    *nBlocksOut = 0;
    HostChain h;
    int r = host_chain(h, "decompress_dict", MI355LZ4_E_STREAM, framedIn, inLen, headerKind, fixedUncomp, c->blockChecksum, maxBlocks, at_capacity);
    if (r) return r;
    const int n = h.n;
    if (n == 0) return MI355LZ4_OK;
    HIP_TRY(hipSetDevice(c->device));
    if ((r = dev_reserve(c->in, inLen + 16)) || (r = dev_reserve(c->offA, (size_t)n * 8)) || (r = dev_reserve(c->offB, ((size_t)n + 1) * 8)) ||
        (r = dev_reserve(c->res, (size_t)n * 4)) || (r = dev_reserve(c->out, (size_t)h.total + 16)))
        return r;
    uint32_t dlen = 0;
    if ((r = upload_dict(c, 1, dict, dictLen, &dlen))) return r;
    if ((r = h2d_staged(c, c->in.p, framedIn, inLen))) return r;
    HIP_TRY(hipMemcpyAsync(c->offA.p, h.boff.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->offB.p, h.ooff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // (the vectors and the dictionary are pageable memory)
    r = mi355lz4_decompress_dict_device(c, (const uint8_t *)c->in.p, inLen, (const uint64_t *)c->offA.p, n, headerKind, fixedUncomp,
                                        dlen ? (const uint8_t *)c->scratch.p : nullptr, (int)dlen, (uint8_t *)c->out.p,
                                        (const uint64_t *)c->offB.p, nullptr, (int32_t *)c->res.p);
    if (r) return r;
    return host_tail(c, "decompress_dict", h, out, cap, outLen, blockLen, nBlocksOut);
}

// Host-buffer form of mi355lz4_decompress_dict_multi_device: mi355lz4_decompress_dict's single group with the first nBlocks entries
// of dictIdx (of maxBlocks) in place of the dictionary.  The chain is walked and the indices are checked on the host first.
extern "C" int mi355lz4_decompress_dict_multi(mi355lz4_ctx *c, const uint8_t *framedIn, size_t inLen, int headerKind, int fixedUncomp,
                                              const mi355lz4_dictset *ds, const int32_t *dictIdx, uint8_t *out, size_t cap,
                                              size_t *outLen, int32_t *blockLen, int maxBlocks, int *nBlocksOut)
{
    if (outLen) *outLen = 0;
    if (nBlocksOut) *nBlocksOut = 0;
    if (!c || !ds) return fail(MI355LZ4_E_ARG, "decompress_dict_multi: null argument");
    if (!outLen || !nBlocksOut || maxBlocks < 0 || fixedUncomp < 0 || (headerKind != 4 && headerKind != 8))
        return fail(MI355LZ4_E_ARG, "decompress_dict_multi: bad arguments");
    if (c->plan.active) return fail(MI355LZ4_E_ARG, "a linked decode begun with mi355lz4_decompress_linked_begin is still open");
    HostChain h;
    int r = host_chain(h, "decompress_dict_multi", MI355LZ4_E_STREAM, framedIn, inLen, headerKind, fixedUncomp, c->blockChecksum, maxBlocks, at_capacity);
    if (r) return r;
    const int n = h.n;
    if (n == 0) return MI355LZ4_OK;
    if (!dictIdx) return fail(MI355LZ4_E_ARG, "decompress_dict_multi: null dictIdx");
    const int nDicts = mi355lz4_dictset_count(ds);
    for (int i = 0; i < n; i++)
        if (dictIdx[i] < -1 || dictIdx[i] >= nDicts)
            return fail(MI355LZ4_E_ARG, "decompress_dict_multi: block %d names dictionary %d of %d", i, dictIdx[i], nDicts);
    HIP_TRY(hipSetDevice(c->device));
    if ((r = dev_reserve(c->in, inLen + 16)) || (r = dev_reserve(c->offA, (size_t)n * 8)) || (r = dev_reserve(c->offB, ((size_t)n + 1) * 8)) ||
        (r = dev_reserve(c->res, (size_t)n * 4)) || (r = dev_reserve(c->lenA, (size_t)n * 4)) || (r = dev_reserve(c->out, (size_t)h.total + 16)))
        return r;
    if ((r = h2d_staged(c, c->in.p, framedIn, inLen))) return r;
    HIP_TRY(hipMemcpyAsync(c->offA.p, h.boff.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->offB.p, h.ooff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->lenA.p, dictIdx, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // (the vectors and the indices are pageable memory)
    r = mi355lz4_decompress_dict_multi_device(c, (const uint8_t *)c->in.p, inLen, (const uint64_t *)c->offA.p, n, headerKind, fixedUncomp,
                                              ds, (const int32_t *)c->lenA.p, (uint8_t *)c->out.p, (const uint64_t *)c->offB.p, nullptr,
                                              (int32_t *)c->res.p);
    if (r) return r;
    return host_tail(c, "decompress_dict_multi", h, out, cap, outLen, blockLen, nBlocksOut);
}

// Host-buffer form of mi355lz4_compress_pages_device: inputs in host memory, one pageSize for all.  One group, synchronous, as the
// partial form: the inputs go up packed back to back, the device call fills engine-owned pages, the four arrays come back, and of
// every page that was written its bytes [0, headerKind + compLen) -- the rest of the caller's `pages` stays as it was.
// (fast: mi355lz4_compress_pages_fast_device with `accel` makes the pages; with hcd, mi355lz4_compress_pages_fastdict_device against
// that prepared dictionary; `who` names the caller in the messages)
static int pages_host(mi355lz4_ctx *c, const char *who, bool fast, int accel, const uint8_t *const *src, const int32_t *srcLen,
                      int nInputs, int pageSize, int maxPages, int headerKind, uint8_t *pages, size_t pageStride, int32_t *pageSrcLen,
                      int32_t *pageCompLen, int32_t *nPages, int32_t *consumed, const mi355lz4_hcdict *hcd = nullptr)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (nInputs < 0 || maxPages < 1 || pageSize < 1 || (headerKind != 0 && headerKind != 4 && headerKind != 8) ||
        pageStride < (size_t)headerKind + (size_t)pageSize)
        return fail(MI355LZ4_E_ARG, "%s: bad arguments", who);
    if (c->blockChecksum) return fail(MI355LZ4_E_ARG, "%s: block checksums are on; pages carry no trailer", who);
    if (fast && c->compLevel != 0) return fail(MI355LZ4_E_ARG, "%s: compression level %d; fast pages are level 0's encoder", who, c->compLevel);
    if (nInputs == 0) return MI355LZ4_OK;
    if (!src || !srcLen || !pages || !pageSrcLen || !pageCompLen || !nPages || !consumed)
        return fail(MI355LZ4_E_ARG, "%s: null pointer", who);
    const size_t n = (size_t)nInputs, np = n * (size_t)maxPages;
    std::vector<uint64_t> off(n);
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        if (srcLen[i] < 0 || srcLen[i] > MI355LZ4_MAX_INPUT_SIZE || (srcLen[i] > 0 && !src[i]))
            return fail(MI355LZ4_E_ARG, "%s: input %zu: bad length or null pointer", who, i);
        off[i] = total;
        total += (uint64_t)srcLen[i];
    }
    HIP_TRY(hipSetDevice(c->device));
    int r;
    // c->res: pageSrcLen[np], pageCompLen[np], nPages[n], consumed[n]; c->lenB: pageSize[n]
    if ((r = dev_reserve(c->in, (size_t)total + 16)) || (r = dev_reserve(c->offA, n * 8)) || (r = dev_reserve(c->lenA, n * 4)) ||
        (r = dev_reserve(c->lenB, n * 4)) || (r = dev_reserve(c->res, (2 * np + 2 * n) * 4)) || (r = dev_reserve(c->out, np * pageStride + 16)))
        return r;
    // the inputs packed into the pinned staging buffer, then one copy
    if ((r = pin_reserve(c->pinIn, (size_t)total + 16))) return r;
    std::vector<CopyTask> tasks;
    for (size_t i = 0; i < n; i++)
        if (srcLen[i] > 0) tasks.push_back(CopyTask{(uint8_t *)c->pinIn.p + off[i], src[i], (size_t)srcLen[i]});
    pool_run(tasks);
    if (total) HIP_TRY(hipMemcpyAsync(c->in.p, c->pinIn.p, (size_t)total, hipMemcpyHostToDevice, c->stream));
    const std::vector<int32_t> ps(n, pageSize);
    HIP_TRY(hipMemcpyAsync(c->offA.p, off.data(), n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->lenA.p, srcLen, n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->lenB.p, ps.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // (the vectors are pageable memory)
    int32_t *dSrcLen = (int32_t *)c->res.p, *dCompLen = dSrcLen + np, *dPages = dCompLen + np, *dCons = dPages + n;
    if (hcd)
        r = mi355lz4_compress_pages_fastdict_device(c, hcd, (const uint8_t *)c->in.p, (const uint64_t *)c->offA.p, (const int32_t *)c->lenA.p,
                                                    nInputs, (const int32_t *)c->lenB.p, maxPages, accel, headerKind, (uint8_t *)c->out.p,
                                                    pageStride, dSrcLen, dCompLen, dPages, dCons);
    else if (fast)
        r = mi355lz4_compress_pages_fast_device(c, (const uint8_t *)c->in.p, (const uint64_t *)c->offA.p, (const int32_t *)c->lenA.p,
                                                nInputs, (const int32_t *)c->lenB.p, maxPages, accel, headerKind, (uint8_t *)c->out.p,
                                                pageStride, dSrcLen, dCompLen, dPages, dCons);
    else
        r = mi355lz4_compress_pages_device(c, (const uint8_t *)c->in.p, (const uint64_t *)c->offA.p, (const int32_t *)c->lenA.p, nInputs,
                                           (const int32_t *)c->lenB.p, maxPages, headerKind, (uint8_t *)c->out.p, pageStride, dSrcLen,
                                           dCompLen, dPages, dCons);
    if (r) return r;
    std::vector<int32_t> back(2 * np + 2 * n);
    HIP_TRY(hipMemcpyAsync(back.data(), c->res.p, back.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int32_t *hSrcLen = back.data(), *hCompLen = hSrcLen + np, *hPages = hCompLen + np, *hCons = hPages + n;
    for (size_t i = 0; i < n; i++) {
        nPages[i] = hPages[i];
        consumed[i] = hCons[i];
        for (size_t k = 0; k < (size_t)hPages[i]; k++) {
            const size_t at = i * (size_t)maxPages + k;
            pageSrcLen[at] = hSrcLen[at];
            pageCompLen[at] = hCompLen[at];
            HIP_TRY(hipMemcpyAsync(pages + at * pageStride, (const uint8_t *)c->out.p + at * pageStride,
                                   (size_t)headerKind + (size_t)hCompLen[at], hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_compress_pages(mi355lz4_ctx *c, const uint8_t *const *src, const int32_t *srcLen, int nInputs, int pageSize,
                                       int maxPages, int headerKind, uint8_t *pages, size_t pageStride, int32_t *pageSrcLen,
                                       int32_t *pageCompLen, int32_t *nPages, int32_t *consumed)
{
    return pages_host(c, "compress_pages", false, 0, src, srcLen, nInputs, pageSize, maxPages, headerKind, pages, pageStride, pageSrcLen,
                      pageCompLen, nPages, consumed);
}

// Host-buffer form of mi355lz4_compress_pages_fast_device: the same single group, the pages by the wave encoder at `accel`.
extern "C" int mi355lz4_compress_pages_fast(mi355lz4_ctx *c, const uint8_t *const *src, const int32_t *srcLen, int nInputs, int pageSize,
                                            int maxPages, int accel, int headerKind, uint8_t *pages, size_t pageStride,
                                            int32_t *pageSrcLen, int32_t *pageCompLen, int32_t *nPages, int32_t *consumed)
{
    return pages_host(c, "compress_pages_fast", true, accel, src, srcLen, nInputs, pageSize, maxPages, headerKind, pages, pageStride,
                      pageSrcLen, pageCompLen, nPages, consumed);
}

// Host-buffer form of mi355lz4_compress_pages_fastdict_device: the same single group, the pages against the prepared dictionary.
extern "C" int mi355lz4_compress_pages_fastdict(mi355lz4_ctx *c, const mi355lz4_hcdict *hcd, const uint8_t *const *src,
                                                const int32_t *srcLen, int nInputs, int pageSize, int maxPages, int accel, int headerKind,
                                                uint8_t *pages, size_t pageStride, int32_t *pageSrcLen, int32_t *pageCompLen,
                                                int32_t *nPages, int32_t *consumed)
{
    if (!c || !hcd) return fail(MI355LZ4_E_ARG, "compress_pages_fastdict: null argument");
    return pages_host(c, "compress_pages_fastdict", true, accel, src, srcLen, nInputs, pageSize, maxPages, headerKind, pages, pageStride,
                      pageSrcLen, pageCompLen, nPages, consumed, hcd);
}

// the size pass over blocks in host memory: H2D, mi355lz4_decoded_size_device, sizes back; synchronous
extern "C" int mi355lz4_decoded_sizes_host(mi355lz4_ctx *c, const uint8_t *framed, size_t len, const uint64_t *blockOff,
                                           int nBlocks, int headerKind, int maxUncomp, int32_t *size)
{
    if (!c || nBlocks < 0 || maxUncomp < 0 || (headerKind != 4 && headerKind != 8) ||
        (nBlocks > 0 && (!framed || !blockOff || !size)))
        return fail(MI355LZ4_E_ARG, "decoded_sizes_host: bad arguments");
    if (nBlocks == 0) return MI355LZ4_OK;
    HIP_TRY(hipSetDevice(c->device));
    int r;
    if ((r = dev_reserve(c->in, len + 16)) || (r = dev_reserve(c->offA, (size_t)nBlocks * 8)) || (r = dev_reserve(c->lenB, (size_t)nBlocks * 4)))
        return r;
    if ((r = h2d_staged(c, c->in.p, framed, len))) return r;
    HIP_TRY(hipMemcpyAsync(c->offA.p, blockOff, (size_t)nBlocks * 8, hipMemcpyHostToDevice, c->stream));
    r = mi355lz4_decoded_size_device(c, (const uint8_t *)c->in.p, len, (const uint64_t *)c->offA.p, nBlocks, headerKind, maxUncomp,
                                     (int32_t *)c->lenB.p, nullptr);
    if (r) return r;
    HIP_TRY(hipMemcpyAsync(size, c->lenB.p, (size_t)nBlocks * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI355LZ4_OK;
}

