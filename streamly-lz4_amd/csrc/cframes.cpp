// cframes.cpp -- writing batches of standard LZ4 frames on the device (mi355lz4_cframes; kernels_cframes.hip).
//
// lz4_frame.cpp writes the frame format on the host, one frame per call from host memory.  This is the write side as a face of
// the C ABI, the counterpart of frames.cpp: a caller-owned object holds the block table and the slots, _compress turns many
// device-resident inputs into one frame each and only enqueues.  The compressed blocks are the engine's own -- one internal
// call over every block of every input, 4-byte headers (a frame's size word is one) -- and everything else is the kernels of
// kernels_cframes.hip.
#include "engine.hpp"

#include <climits>
#include <cstring>
#include <new>
#include <vector>

using namespace mi355lz4_detail;

namespace {

const unsigned kKnownFlags = MI355LZ4_CFRAMES_LINKED | MI355LZ4_CFRAMES_BLOCK_CHECKSUM | MI355LZ4_CFRAMES_CONTENT_SIZE |
                             MI355LZ4_CFRAMES_CONTENT_CHECKSUM;

// consecutive 64-byte aligned arrays out of one allocation
struct Carve {
    uint8_t *p;
    size_t at = 0;
    template <class T> T *take(size_t n)
    {
        T *r = p ? (T *)(p + at) : nullptr;
        at += (n * sizeof(T) + 63) & ~(size_t)63;
        return r;
    }
};
void carve_inputs(CFramesArgs &a, Carve &c, size_t n)
{
    a.nb = c.take<int32_t>(n); a.blockFirst = c.take<uint64_t>(n + 1);
    a.verdict = c.take<int64_t>(n); a.base = c.take<uint64_t>(n);
}
void carve_entries(CFramesArgs &a, Carve &c, size_t t)
{
    a.srcOff = c.take<uint64_t>(t); a.srcLen = c.take<int32_t>(t); a.blockInput = c.take<int32_t>(t);
    a.framedLen = c.take<int32_t>(t); a.piece = c.take<int32_t>(t); a.pieceOff = c.take<uint64_t>(t + 1);
}

// The shape of a call from its host-side bounds: the table holds totalLen / bmax + nInputs blocks, and with linked frames one
// spacer per input; a block is min(bmax, maxInputLen) bytes at the most.
int shape(const char *who, int nInputs, uint64_t maxInputLen, uint64_t totalLen, int blockSizeId, unsigned flags, CFramesArgs &a)
{
    if (nInputs < 0) return fail(MI355LZ4_E_ARG, "%s: nInputs < 0", who);
    if (blockSizeId < 4 || blockSizeId > 7) return fail(MI355LZ4_E_ARG, "%s: blockSizeId %d outside 4..7", who, blockSizeId);
    if (flags & ~kKnownFlags) return fail(MI355LZ4_E_ARG, "%s: unknown flag bits 0x%x", who, flags);
    const uint64_t bmax = (uint64_t)1 << (8 + 2 * blockSizeId);
    const uint64_t real = totalLen / bmax + (uint64_t)nInputs;
    const uint64_t tab = real + ((flags & MI355LZ4_CFRAMES_LINKED) ? (uint64_t)nInputs : 0u);
    if (tab >= (uint64_t)INT_MAX)
        return fail(MI355LZ4_E_ARG, "%s: a block bound of %llu (totalLen / block size + nInputs, and a spacer per linked input): it must fit an int",
                    who, (unsigned long long)tab);
    a.nInputs = nInputs; a.maxInputLen = maxInputLen; a.bmax = (uint32_t)bmax; a.bsid = blockSizeId; a.flags = flags;
    a.realCap = (int)real; a.tabCap = (int)tab;
    a.maxBlockLen = (int)(maxInputLen < bmax ? maxInputLen : bmax);
    a.slotStride = mi355lz4_slot_stride(a.maxBlockLen, 4);
    return MI355LZ4_OK;
}

int owner(const mi355lz4_ctx *c, const mi355lz4_cframes *w, const char *who)
{
    if (!c || !w) return fail(MI355LZ4_E_ARG, "%s: null argument", who);
    if (w->device != c->device)
        return fail(MI355LZ4_E_ARG, "%s: the object lives on device %d, the engine on %d", who, w->device, c->device);
    return MI355LZ4_OK;
}

// the object's scratch for that shape; `grew` says that an allocation was made (the caller then is not enqueue-only)
int reserve(mi355lz4_ctx *c, mi355lz4_cframes *w, CFramesArgs &a)
{
    Carve ni{nullptr}, ne{nullptr};
    carve_inputs(a, ni, (size_t)a.nInputs);
    carve_entries(a, ne, (size_t)a.tabCap);
    const size_t slotBytes = (size_t)a.tabCap * a.slotStride;
    if (ni.at > w->perInput.cap || ne.at > w->perEntry.cap || slotBytes > w->slots.cap) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipStreamSynchronize(c->stream));           // a call that still uses the scratch about to be replaced
    }
    int r;
    if ((r = dev_reserve(w->perInput, ni.at)) || (r = dev_reserve(w->perEntry, ne.at)) || (r = dev_reserve(w->slots, slotBytes))) return r;
    Carve ci{(uint8_t *)w->perInput.p}, ce{(uint8_t *)w->perEntry.p};
    carve_inputs(a, ci, (size_t)a.nInputs);
    carve_entries(a, ce, (size_t)a.tabCap);
    a.slots = (uint8_t *)w->slots.p;
    return MI355LZ4_OK;
}

}  // namespace

extern "C" uint64_t mi355lz4_cframes_bound(uint64_t len, int blockSizeId, unsigned flags)
{
    if (blockSizeId < 4 || blockSizeId > 7 || (flags & ~kKnownFlags)) return 0;
    const uint64_t bmax = (uint64_t)1 << (8 + 2 * blockSizeId);
    const uint64_t nb = len / bmax + (len % bmax ? 1u : 0u);
    return ((flags & MI355LZ4_CFRAMES_CONTENT_SIZE) ? 15u : 7u) + nb * (4u + ((flags & MI355LZ4_CFRAMES_BLOCK_CHECKSUM) ? 4u : 0u)) + len + 4u +
           ((flags & MI355LZ4_CFRAMES_CONTENT_CHECKSUM) ? 4u : 0u);
}

extern "C" int mi355lz4_cframes_create(mi355lz4_ctx *c, mi355lz4_cframes **out)
{
    if (out) *out = nullptr;
    if (!c || !out) return fail(MI355LZ4_E_ARG, "cframes_create: null argument");
    mi355lz4_cframes *w = new (std::nothrow) mi355lz4_cframes();
    if (!w) return fail(MI355LZ4_E_ARG, "out of host memory");
    w->device = c->device;
    *out = w;
    return MI355LZ4_OK;
}

extern "C" void mi355lz4_cframes_destroy(mi355lz4_cframes *w)
{
    if (!w) return;
    if (w->perInput.p || w->perEntry.p || w->slots.p) {
        hipSetDevice(w->device);
        hipDeviceSynchronize();             // calls that still use the scratch
    }
    dev_release(w->perInput); dev_release(w->perEntry); dev_release(w->slots);
    delete w;
}

extern "C" int mi355lz4_cframes_reserve(mi355lz4_ctx *c, mi355lz4_cframes *w, int nInputs, uint64_t maxInputLen, uint64_t totalLen,
                                        int blockSizeId)
{
    if (int r = owner(c, w, "cframes_reserve")) return r;
    CFramesArgs a{};
    // (the linked layout is the larger one: a reserve serves both)
    if (int r = shape("cframes_reserve", nInputs, maxInputLen, totalLen, blockSizeId, MI355LZ4_CFRAMES_LINKED, a)) return r;
    if (nInputs == 0) return MI355LZ4_OK;
    return reserve(c, w, a);
}

// Enqueue only when the scratch is there.  The engine's call runs with its reference-exact mode and its block checksums off (a
// frame is its own stream, and its block checksums are its own) and with the linked switch the flags ask for; all three are put
// back before the call returns.
extern "C" int mi355lz4_cframes_compress(mi355lz4_ctx *c, mi355lz4_cframes *w, const uint8_t *src, uint64_t srcBufLen,
                                         const uint64_t *inOff, const uint64_t *inLen, int nInputs, uint64_t maxInputLen,
                                         uint64_t totalLen, int blockSizeId, unsigned flags, int accel, uint8_t *dst,
                                         const uint64_t *dstOff, const uint64_t *dstCap, int64_t *frameLen)
{
    if (int r = owner(c, w, "cframes_compress")) return r;
    CFramesArgs a{};
    if (int r = shape("cframes_compress", nInputs, maxInputLen, totalLen, blockSizeId, flags, a)) return r;
    if (nInputs == 0) return MI355LZ4_OK;
    if (!inOff || !inLen || !dst || !dstOff || !dstCap || !frameLen || (!src && srcBufLen > 0))
        return fail(MI355LZ4_E_ARG, "cframes_compress: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    if (int r = reserve(c, w, a)) return r;
    a.src = src; a.srcBufLen = srcBufLen; a.inOff = inOff; a.inLen = inLen;
    a.dst = dst; a.dstOff = dstOff; a.dstCap = dstCap; a.frameLen = frameLen;
    launch_cframes_plan(a, c->stream);
    if (int r = check_launch("cframes plan launch")) return r;
    const int savedSum = c->blockChecksum, savedLinked = c->linkedCompress;
    const int savedExact = engine_swap_compress_exact(c, 0);
    c->blockChecksum = 0;
    c->linkedCompress = (flags & MI355LZ4_CFRAMES_LINKED) ? 1 : 0;
    // (src may be null when every input is empty; the engine's check wants a pointer only with bytes to read)
    const int r = encode_device(c, src, a.srcOff, a.srcLen, 0, a.maxBlockLen, a.tabCap, accel, 4, a.slots, a.slotStride, a.framedLen, 0);
    c->linkedCompress = savedLinked;
    c->blockChecksum = savedSum;
    engine_swap_compress_exact(c, savedExact);
    if (r) return r;
    launch_cframes_finish(a, c->stream);
    return check_launch("cframes finish launch");
}

// Host buffers, synchronous.  Inputs go to the device in groups whose inputs and bound-spaced frames stay under a budget
// (MI355LZ4_CFRAMES_BUDGET_MB, default 1024; an input is never split, so one input alone may exceed it); a group is one image {inOff,
// inLen, dstOff, dstCap, the bytes} and one staged copy, _compress into the bound-spaced layout, the gather, and one copy back.
// The frames collect in a host buffer of the call and reach `out` when all of them are known to fit.
extern "C" int mi355lz4_compress_frames(mi355lz4_ctx *c, const uint8_t *const *in, const size_t *inLen, int nInputs, int blockSizeId,
                                        unsigned flags, int accel, uint8_t *out, size_t cap, size_t *outLen, int64_t *frameLen)
{
    if (outLen) *outLen = 0;
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    {
        CFramesArgs probe{};
        if (int r = shape("compress_frames", nInputs, 0, 0, blockSizeId, flags, probe)) return r;
    }
    if (nInputs == 0) return MI355LZ4_OK;
    if (!in || !inLen || !frameLen || !outLen) return fail(MI355LZ4_E_ARG, "compress_frames: null pointer");
    const size_t n = (size_t)nInputs;
    for (size_t i = 0; i < n; i++)
        if (!in[i] && inLen[i] > 0) return fail(MI355LZ4_E_ARG, "compress_frames: input %zu is null", i);
    HIP_TRY(hipSetDevice(c->device));
    const int mb = env_int("MI355LZ4_CFRAMES_BUDGET_MB", 1024);
    const uint64_t budget = (uint64_t)(mb < 1 ? 1 : mb) << 20;
    mi355lz4_cframes *w = nullptr;
    int r = mi355lz4_cframes_create(c, &w);
    if (r) return r;
    std::vector<uint8_t> frames;            // every group's dense frames, in input order
    uint64_t total = 0;
    for (size_t g0 = 0; g0 < n && !r;) {
        size_t g1 = g0;
        uint64_t bytes = 0, bound = 0, longest = 0;
        while (g1 < n) {
            const uint64_t b = mi355lz4_cframes_bound(inLen[g1], blockSizeId, flags);
            if (g1 > g0 && bytes + bound + inLen[g1] + b > budget) break;
            bytes += inLen[g1]; bound += b;
            if (inLen[g1] > longest) longest = inLen[g1];
            g1++;
        }
        const size_t m = g1 - g0;
        // {inOff[m], inLen[m], dstOff[m], dstCap[m], the bytes}
        const size_t head = (4 * m * 8 + 63) & ~(size_t)63;
        std::vector<uint8_t> image(head + (size_t)bytes);
        uint64_t *meta = (uint64_t *)image.data();
        uint64_t at = 0, to = 0;
        for (size_t i = 0; i < m; i++) {
            const uint64_t b = mi355lz4_cframes_bound(inLen[g0 + i], blockSizeId, flags);
            meta[i] = at; meta[m + i] = inLen[g0 + i]; meta[2 * m + i] = to; meta[3 * m + i] = b;
            if (inLen[g0 + i]) memcpy(image.data() + head + at, in[g0 + i], inLen[g0 + i]);
            at += inLen[g0 + i]; to += b;
        }
        // the group's results: frameLen[m], then the gather's scan, m + 1 entries
        std::vector<int64_t> res(2 * m + 1);
        if ((r = dev_reserve(c->in, image.size())) || (r = dev_reserve(c->out, (size_t)bound + 16)) || (r = dev_reserve(c->dense, (size_t)bound + 16)) ||
            (r = dev_reserve(c->res, res.size() * 8)) || (r = h2d_staged(c, c->in.p, image.data(), image.size())))
            break;
        const uint64_t *dMeta = (const uint64_t *)c->in.p;
        int64_t *dLen = (int64_t *)c->res.p;
        uint64_t *dScan = (uint64_t *)c->res.p + m;
        if ((r = mi355lz4_cframes_compress(c, w, (const uint8_t *)c->in.p + head, bytes, dMeta, dMeta + m, (int)m, longest, bytes, blockSizeId,
                                           flags, accel, (uint8_t *)c->out.p, dMeta + 2 * m, dMeta + 3 * m, dLen)))
            break;
        launch_cframes_gather((const uint8_t *)c->out.p, dMeta + 2 * m, dLen, (int)m, dScan, (uint8_t *)c->dense.p, bound, c->stream);
        if ((r = check_launch("cframes gather launch")) || (r = d2h_staged(c, (uint8_t *)res.data(), c->res.p, res.size() * 8))) break;
        const uint64_t dense = (uint64_t)res[2 * m];
        for (size_t i = 0; i < m; i++) frameLen[g0 + i] = res[i];
        total += dense;
        if (total <= cap) {                 // (past the capacity only the total is still wanted)
            const size_t had = frames.size();
            frames.resize(had + (size_t)dense);
            if ((r = d2h_staged(c, frames.data() + had, c->dense.p, (size_t)dense))) break;
        }
        g0 = g1;
    }
    mi355lz4_cframes_destroy(w);
    if (r) return r;
    *outLen = (size_t)total;
    if (total > cap)
        return fail(MI355LZ4_E_CAPACITY, "compress_frames: the frames take %llu bytes, the buffer holds %zu", (unsigned long long)total, cap);
    if (total > 0 && !out) return fail(MI355LZ4_E_ARG, "compress_frames: null output");
    if (total > 0) memcpy(out, frames.data(), (size_t)total);
    return MI355LZ4_OK;
}
