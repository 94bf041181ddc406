// frames.cpp -- batches of standard LZ4 frames on the device (mi355lz4_frames; kernels/frames.inc).
//
// lz4_frame.cpp reads the frame format on the host, one buffer per call.  This is the same format as a face of the C ABI: a
// caller-owned object holds a parsed batch, _load parses many inputs on the device and reports their exact decoded sizes, _decode
// decodes them all and only enqueues.  The tables are sized by what the scan counted -- frames and blocks that are really there --
// never by a declared content size or by blocks x maximum block size (the crafted-frame rule of lz4_frame.cpp).
#include "engine.hpp"

#include <climits>
#include <cstring>
#include <new>
#include <vector>

using namespace mi355lz4_detail;

namespace {

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

void carve_inputs(FramesArgs &a, Carve &c, int n)
{
    const size_t m = (size_t)n;
    a.inOff = c.take<uint64_t>(m); a.inLen = c.take<uint64_t>(m);
    a.errPos = c.take<uint64_t>(m);
    a.frameFirst = c.take<uint64_t>(m + 1); a.blockFirst = c.take<uint64_t>(m + 1);
    a.sizes = c.take<int64_t>(m); a.errKey = c.take<uint64_t>(m);
    a.nFrames = c.take<int32_t>(m); a.nBlocks = c.take<int32_t>(m); a.err = c.take<int32_t>(m);
    a.counts = c.take<uint32_t>(16);
}
void carve_frames(FramesArgs &a, Carve &c, size_t nF)
{
    a.frames = c.take<FrmFrame>(nF); a.linked = c.take<int32_t>(nF);
}
void carve_blocks(FramesArgs &a, Carve &c, size_t nB)
{
    a.blocks = c.take<FrmBlock>(nB);
    a.decOff = c.take<uint64_t>(nB); a.decOut = c.take<uint64_t>(nB);
    a.bsumFail = c.take<int32_t>(nB); a.indep = c.take<int32_t>(nB);
    a.decCap = c.take<int32_t>(nB); a.decRes = c.take<int32_t>(nB);
}

int frames_owner(const mi355lz4_ctx *c, const mi355lz4_frames *fr, const char *who)
{
    if (!c || !fr) return fail(MI355LZ4_E_ARG, "%s: null argument", who);
    if (fr->device != c->device)
        return fail(MI355LZ4_E_ARG, "%s: the object lives on device %d, the engine on %d", who, fr->device, c->device);
    return MI355LZ4_OK;
}

}  // namespace

extern "C" int mi355lz4_frames_create(mi355lz4_ctx *c, mi355lz4_frames **out)
{
    if (out) *out = nullptr;
    if (!c || !out) return fail(MI355LZ4_E_ARG, "frames_create: null argument");
    mi355lz4_frames *fr = new (std::nothrow) mi355lz4_frames();
    if (!fr) return fail(MI355LZ4_E_ARG, "out of host memory");
    fr->device = c->device;
    *out = fr;
    return MI355LZ4_OK;
}

extern "C" void mi355lz4_frames_destroy(mi355lz4_frames *fr)
{
    if (!fr) return;
    if (fr->perInput.p || fr->perFrame.p || fr->perBlock.p || fr->pin.p) {
        hipSetDevice(fr->device);
        hipDeviceSynchronize();             // calls that still use the tables
    }
    dev_release(fr->perInput); dev_release(fr->perFrame); dev_release(fr->perBlock);
    pin_release(fr->pin);
    delete fr;
}

extern "C" int mi355lz4_frames_load(mi355lz4_ctx *c, mi355lz4_frames *fr, const uint8_t *buf, uint64_t bufLen,
                                    const uint64_t *inOff, const uint64_t *inLen, int nInputs, unsigned flags)
{
    if (int r = frames_owner(c, fr, "frames_load")) return r;
    if (nInputs < 0) return fail(MI355LZ4_E_ARG, "frames_load: nInputs < 0");
    if (flags & ~(MI355LZ4_FRAMES_SKIP_CONTENT_CHECKSUM | MI355LZ4_FRAMES_SKIP_BLOCK_CHECKSUM))
        return fail(MI355LZ4_E_ARG, "frames_load: unknown flag bits 0x%x", flags);
    if (nInputs > 0 && (!inOff || !inLen || (!buf && bufLen > 0))) return fail(MI355LZ4_E_ARG, "frames_load: null pointer");
    fr->loaded = false;
    fr->total = 0;
    FramesArgs a{};
    a.buf = buf; a.bufLen = bufLen; a.nInputs = nInputs; a.flags = flags;
    if (nInputs == 0) { fr->a = a; fr->loaded = true; return MI355LZ4_OK; }
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)nInputs;
    int r;
    Carve need{nullptr};
    carve_inputs(a, need, nInputs);
    if ((r = dev_reserve(fr->perInput, need.at)) || (r = pin_reserve(fr->pin, 64 + n * sizeof(int64_t)))) return r;
    Carve ci{(uint8_t *)fr->perInput.p};
    carve_inputs(a, ci, nInputs);
    HIP_TRY(hipMemcpyAsync((void *)a.inOff, inOff, n * 8, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync((void *)a.inLen, inLen, n * 8, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(a.counts, 0, 64, c->stream));
    launch_frames_scan(a, c->stream);
    if ((r = check_launch("frames scan launch"))) return r;
    // the first of the load's two waits: how many frames and blocks there are sizes the tables
    uint64_t *pinU = (uint64_t *)fr->pin.p;
    HIP_TRY(hipMemcpyAsync(&pinU[0], a.frameFirst + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&pinU[1], a.blockFirst + n, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t nF = pinU[0], nB = pinU[1];
    if (nF >= (uint64_t)INT_MAX || nB >= (uint64_t)INT_MAX)
        return fail(MI355LZ4_E_ARG, "frames_load: %llu frames and %llu blocks in one call: the counts must fit an int",
                    (unsigned long long)nF, (unsigned long long)nB);
    a.nFramesAll = (int)nF; a.nBlocksAll = (int)nB;
    Carve needF{nullptr}, needB{nullptr};
    carve_frames(a, needF, (size_t)nF + 1);
    carve_blocks(a, needB, (size_t)nB + 1);
    if ((r = dev_reserve(fr->perFrame, needF.at)) || (r = dev_reserve(fr->perBlock, needB.at))) return r;
    Carve cf{(uint8_t *)fr->perFrame.p}, cb{(uint8_t *)fr->perBlock.p};
    carve_frames(a, cf, (size_t)nF + 1);
    carve_blocks(a, cb, (size_t)nB + 1);
    // (zeroed: a walk that comes out shorter than the first leaves frames of no blocks behind, not garbage)
    HIP_TRY(hipMemsetAsync(a.frames, 0, ((size_t)nF + 1) * sizeof(FrmFrame), c->stream));
    HIP_TRY(hipMemsetAsync(a.blocks, 0, ((size_t)nB + 1) * sizeof(FrmBlock), c->stream));
    launch_frames_load(a, c->stream);
    if ((r = check_launch("frames load launch"))) return r;
    // the second: the sizes, and how long the two lists of the decode are
    HIP_TRY(hipMemcpyAsync(&pinU[2], a.counts, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(fr->sizesHost(), a.sizes, n * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint32_t *cnt = (const uint32_t *)&pinU[2];
    a.nIndep = (int)cnt[0]; a.nLinked = (int)cnt[1];
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++)
        if (fr->sizesHost()[i] > 0) total += (uint64_t)fr->sizesHost()[i];
    fr->total = total;
    fr->a = a;
    fr->loaded = true;
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_frames_inputs(const mi355lz4_frames *fr)
{
    return (fr && fr->loaded) ? fr->a.nInputs : fail(MI355LZ4_E_ARG, "frames_inputs: no loaded object");
}
extern "C" int mi355lz4_frames_blocks(const mi355lz4_frames *fr)
{
    return (fr && fr->loaded) ? fr->a.nBlocksAll : fail(MI355LZ4_E_ARG, "frames_blocks: no loaded object");
}
extern "C" uint64_t mi355lz4_frames_total(const mi355lz4_frames *fr) { return (fr && fr->loaded) ? fr->total : 0; }
extern "C" const int64_t *mi355lz4_frames_sizes(const mi355lz4_frames *fr) { return (fr && fr->loaded) ? fr->a.sizes : nullptr; }
extern "C" int mi355lz4_frames_get_sizes(const mi355lz4_frames *fr, int64_t *sizesHost)
{
    if (!fr || !fr->loaded) return fail(MI355LZ4_E_ARG, "frames_get_sizes: no loaded object");
    if (fr->a.nInputs > 0 && !sizesHost) return fail(MI355LZ4_E_ARG, "frames_get_sizes: null pointer");
    if (fr->a.nInputs > 0) memcpy(sizesHost, fr->sizesHost(), (size_t)fr->a.nInputs * sizeof(int64_t));
    return MI355LZ4_OK;
}

// Enqueue only.  The compressed blocks of independent frames go through the engine's own planner in one internal call -- 4-byte
// headers (a frame's size word is one), capacities = the sizes, the engine's checksum switch off: a frame's block checksums are
// its own -- everything else is the kernels of kernels/frames.inc.
extern "C" int mi355lz4_frames_decode(mi355lz4_ctx *c, const mi355lz4_frames *fr, uint8_t *out, const uint64_t *outOff,
                                      int64_t *result)
{
    if (int r = frames_owner(c, fr, "frames_decode")) return r;
    if (!fr->loaded) return fail(MI355LZ4_E_ARG, "frames_decode: nothing is loaded");
    if (fr->a.nInputs == 0) return MI355LZ4_OK;
    if (!outOff || !result || (!out && fr->total > 0)) return fail(MI355LZ4_E_ARG, "frames_decode: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    FramesArgs a = fr->a;
    a.out = out; a.outOff = outOff; a.result = result;
    int r;
    launch_frames_place(a, c->stream);
    if ((r = check_launch("frames place launch"))) return r;
    if (a.nIndep > 0) {
        const int saved = c->blockChecksum;
        c->blockChecksum = 0;
        r = decode_device(c, {a.buf, a.bufLen, a.decOff, a.nIndep, 4, 0, 0, out, a.decOut, a.decCap, a.decRes});
        c->blockChecksum = saved;
        if (r) return r;
    }
    launch_frames_decode(a, c->stream);
    return check_launch("frames decode launch");
}

// Host buffers, synchronous: the inputs to the device behind their offsets and lengths (one staged copy), _load, then _decode
// into a dense layout (input i at the scan of the sizes), and the outputs and results back.
extern "C" int mi355lz4_decompress_frames(mi355lz4_ctx *c, const uint8_t *const *in, const size_t *inLen, int nInputs,
                                          unsigned flags, uint8_t *out, size_t cap, size_t *outLen, int64_t *result)
{
    if (outLen) *outLen = 0;
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (nInputs < 0) return fail(MI355LZ4_E_ARG, "decompress_frames: nInputs < 0");
    if (flags & ~(MI355LZ4_FRAMES_SKIP_CONTENT_CHECKSUM | MI355LZ4_FRAMES_SKIP_BLOCK_CHECKSUM))
        return fail(MI355LZ4_E_ARG, "decompress_frames: unknown flag bits 0x%x", flags);
    if (nInputs == 0) return MI355LZ4_OK;
    if (!in || !inLen || !result || !outLen) return fail(MI355LZ4_E_ARG, "decompress_frames: null pointer");
    const size_t n = (size_t)nInputs;
    size_t bytes = 0;
    for (size_t i = 0; i < n; i++) {
        if (!in[i] && inLen[i] > 0) return fail(MI355LZ4_E_ARG, "decompress_frames: input %zu is null", i);
        bytes += inLen[i];
    }
    HIP_TRY(hipSetDevice(c->device));
    // {inOff[n], inLen[n], the bytes}, one host image and one staged copy
    const size_t head = (2 * n * 8 + 63) & ~(size_t)63;
    std::vector<uint8_t> image(head + bytes);
    uint64_t *meta = (uint64_t *)image.data();
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        meta[i] = at; meta[n + i] = inLen[i];
        if (inLen[i]) memcpy(image.data() + head + at, in[i], inLen[i]);
        at += inLen[i];
    }
    int r;
    if ((r = dev_reserve(c->in, image.size())) || (r = h2d_staged(c, c->in.p, image.data(), image.size()))) return r;
    const uint8_t *dIn = (const uint8_t *)c->in.p;
    mi355lz4_frames *fr = nullptr;
    if ((r = mi355lz4_frames_create(c, &fr))) return r;
    r = mi355lz4_frames_load(c, fr, dIn + head, bytes, (const uint64_t *)dIn, (const uint64_t *)dIn + n, nInputs, flags);
    if (!r && fr->total > cap) {
        *outLen = (size_t)fr->total;
        r = fail(MI355LZ4_E_CAPACITY, "decompress_frames: the inputs decode to %llu bytes, the buffer holds %zu",
                 (unsigned long long)fr->total, cap);
    }
    if (!r && fr->total > 0 && !out) r = fail(MI355LZ4_E_ARG, "decompress_frames: null output");
    bool anyBad = false;
    if (!r) {
        std::vector<uint64_t> outOff(n);
        uint64_t run = 0;
        for (size_t i = 0; i < n; i++) { outOff[i] = run; if (fr->sizesHost()[i] > 0) run += (uint64_t)fr->sizesHost()[i]; }
        if (!(r = dev_reserve(c->out, (size_t)fr->total + 16)) && !(r = dev_reserve(c->offA, n * 8)) && !(r = dev_reserve(c->res, n * 8)) &&
            !(r = h2d_staged(c, c->offA.p, (const uint8_t *)outOff.data(), n * 8)) &&
            !(r = mi355lz4_frames_decode(c, fr, (uint8_t *)c->out.p, (const uint64_t *)c->offA.p, (int64_t *)c->res.p)) &&
            !(r = d2h_staged(c, (uint8_t *)result, c->res.p, n * 8)) && !(r = d2h_staged(c, out, c->out.p, (size_t)fr->total))) {
            // an input that failed at decode time held its size's worth of the layout: close the gaps, so that input i lies at
            // the scan of the results >= 0 and the caller needs nothing but result[] to find it
            size_t to = 0;
            for (size_t i = 0; i < n; i++) {
                const int64_t s = fr->sizesHost()[i];
                if (result[i] < 0) { anyBad = true; continue; }
                if (to != outOff[i] && s > 0) memmove(out + to, out + outOff[i], (size_t)s);
                to += (size_t)s;
            }
            *outLen = to;
        }
    }
    mi355lz4_frames_destroy(fr);
    if (r) return r;
    return anyBad ? fail(MI355LZ4_E_BLOCK, "decompress_frames: some input failed; see result[]") : MI355LZ4_OK;
}
