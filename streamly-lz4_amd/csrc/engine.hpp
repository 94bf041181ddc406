// engine.hpp -- what the layers of the C ABI share (internal, not installed): api.cpp holds the engine and the device-pointer
// calls, host_batch.cpp the host-buffer calls on top of them, legacy.cpp the LZ4_* face; multi_device.cpp, lz4_frame.cpp and
// host_stream.cpp read an engine's switches.  Everything that is not extern "C" lives in mi355lz4_detail.
#pragma once

#include "../../include/mi355lz4.h"

#include "kernels.h"
#include "linked_plan.hpp"

#include <hip/hip_runtime.h>

#include <vector>

namespace mi355lz4_detail {

// The message mi355lz4_last_error returns: ONE buffer per thread for the whole library (api.cpp), written through fail() only.
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int check_launch(const char *what);
int env_int(const char *name, int dflt);

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return mi355lz4_detail::fail(MI355LZ4_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                         __FILE__, __LINE__);                                  \
    } while (0)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};
int dev_reserve(DevBuf &b, size_t bytes);
int pin_reserve(DevBuf &b, size_t bytes);
void dev_release(DevBuf &b);
void pin_release(DevBuf &b);

// The host copy pool (api.cpp): run all tasks, the calling thread working too; one large range, cut into slices.  Both return
// when every byte is copied.
struct CopyTask { uint8_t *dst; const uint8_t *src; size_t n; };
void pool_run(const std::vector<CopyTask> &tasks);
void pool_copy(uint8_t *dst, const uint8_t *src, size_t n);

}  // namespace mi355lz4_detail

struct mi355lz4_ctx {
    using DevBuf = mi355lz4_detail::DevBuf;
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    int decoder = 0;
    int linkedCompress = 0;                 // compress calls treat their blocks as consecutive blocks of one stream
    int blockChecksum = 0;                  // every block's data is followed by its xxh32 (mi355lz4_set_block_checksum)
    int compLevel = 0;                      // 0: k_encode (fast); 1..9: k_encode_hc (mi355lz4_set_compression_level)
    int compExact = 0;                      // compress calls continue ONE reference-exact stream (mi355lz4_set_compress_exact)
    // ... that stream's state (the device counterpart of LZ4_stream_t): currentOffset and dictSize here, the table and
    // the previous array's last bytes in exState; fresh = the table is still to be zeroed (a new stream)
    struct ExactStream { uint32_t cur = 0, dictSize = 0; int dictBytes = 0; bool fresh = true; int last[4] = {0, 0, 0, 0}; } ex;
    DevBuf exState, exMeta, exTabs, exFlags;
    DevBuf ckBuf;                           // ... the decode side's per-block verdicts (k_xxh32_verify)
    hipEvent_t ckEvent = nullptr;           // ... end of the last decode that read them, and the stream it ran on
    hipStream_t ckStream = nullptr;
    // workspaces of the host-buffer API (grown on demand, reused across calls)
    DevBuf in, slots, dense, out, offA, offB, lenA, lenB, res, scratch;
    DevBuf tokBuf;                          // decoder variant 3: token lists
    DevBuf tolPool, tolMeta;                // deferred-copy decode of a long linked stream (linked_replay.hpp)
    DevBuf linkBuf, ptrBuf, pinStat;        // ... its failure count, control block and source pointers (linked_ptr.hpp)
    DevBuf pinIn, pinOut;   // pinned host staging
    DevBuf pinMeta;         // pinned: per-group sizes coming back from the device
    hipStream_t sIn = nullptr, sOut = nullptr;   // copy streams of the pipelined host-buffer API (created on first use)
    hipStream_t sK[2] = {nullptr, nullptr};   // compute streams: kernels of consecutive groups overlap
    // a linked decode whose data half is still to be issued (mi355lz4_decompress_linked_begin / _end)
    struct LinkedPlan {
        bool active = false, split = false;
        DecodeArgs a;
        int first = 0, last = -1, pool = 0, seg = 0;
    } plan;
    // small-batch compression: per-segment sequence lists, one scratch buffer per stream the engine has been used on
    // (the host pipelines run two groups at a time on two compute streams; work on ONE stream is ordered)
    struct SegScratch { hipStream_t s = nullptr; DevBuf b; unsigned long long tick = 0; } seg[4];
    int nSeg = 0;
    unsigned long long segTick = 0;
    // mi355lz4_compress_hcdict_device: the workgroups' staging windows (dictionary + block), one scratch per stream as above
    SegScratch hcStage[4];
    int nHcStage = 0;
    int linkedAsyncCap = 0;                // > 0: linked device decodes do not wait on the host (mi355lz4_set_linked_async)
    RuninState runin;                      // the run-in decode's adaptive state (linked_plan.hpp)
    int linkedPath = -1;                   // diagnostics: how the last linked call was finished (LinkedPath; mi355lz4_debug_runin_state)
    int runinShareE6 = -1;                 // diagnostics: the dictionary share the last linked call sampled, in millionths (-1: none)
    int segMode = -1;                      // small-batch segments per block: -1 auto, 0 off, k forced (mi355lz4_set_segments)
    hipEvent_t linkEvent = nullptr;        // end of the last linked decode's use of linkBuf / tolPool / tolMeta / ptrBuf
    hipStream_t linkStream = nullptr;      // ... and the stream it ran on
    bool linkBusy = false;
    unsigned long long *stats = nullptr;   // diagnostics: device counters of the lane-parallel decoder (off by default)
    uint32_t *cuDbg = nullptr;             // diagnostics: 16 words per block from the workgroup-per-block decoder (mi355lz4_debug_cu)
};

// A prepared high-compression dictionary (api.cpp, "high-compression levels against a shared dictionary"): the device image
// k_hcdict_build wrote (kernels.h, HCDICT_*), and beside it the wave encoder's table image from k_hcdict_build_fast (FASTDICT_*)
// for level 0.  keep is what the last _load enqueued; the kernels read the images' own counts.
struct mi355lz4_hcdict {
    int device = 0;
    int keep = 0;
    uint8_t *image = nullptr;
    uint8_t *fastImage = nullptr;
};

// A set of prepared dictionaries (api.cpp, "dictionary sets"): n entries of kernels.h's DictSetEntry on the device, filled from
// the members' image pointers at creation -- the members are borrowed, and a _hcdict_load rebuilds their images in place -- and
// behind them the two words {stagings, grid} of the last multi compress call.
struct mi355lz4_dictset {
    int device = 0;
    int n = 0;
    DictSetEntry *table = nullptr;         // n entries, then uint32 last[2]
    uint32_t *last() const { return (uint32_t *)(table + n); }
};

// The per-call stream table of the three sets of slots (api.cpp, stream_table_upload): {first block, end block, slot} per stream
// goes through a ring of pinned buffers; an entry is reused once the launch that read it is done.
struct StreamTableRing {                    // (shared with mi355lz4_dstreams, the decode side's set)
    struct Ring { mi355lz4_detail::DevBuf pin, dev; hipEvent_t ev = nullptr; bool busy = false; } ring[4];
    int next = 0;
    void release()
    {
        for (auto &r : ring) {
            if (r.ev) hipEventDestroy(r.ev);
            r.ev = nullptr; r.busy = false;
            mi355lz4_detail::pin_release(r.pin);
            mi355lz4_detail::dev_release(r.dev);
        }
    }
};

// A set of slots on one device, written once for both sides: the compress side's slot is CSTREAM_SLOT_BYTES, the decode side's
// (mi355lz4_dstreams, below) DSTREAM_SLOT_BYTES.  `who` names the calling entry point in the messages.
struct SlotSet {
    int device = 0;
    int nSlots = 0;
    uint8_t *state = nullptr;               // nSlots * the side's slot size
    StreamTableRing table;
};
struct mi355lz4_cstreams : SlotSet {};
struct mi355lz4_dstreams : SlotSet {};
struct mi355lz4_fstreams : SlotSet {        // (the fast compress side's set: a slot is the decode side's, FSTREAM_SLOT_BYTES)
    int level = 0;                          // 0: the wave encoder; 1..12: the hash-chain encoder (mi355lz4_fstreams_set_level)
};

// A parsed batch of standard LZ4 frames (frames.cpp, kernels/frames.inc): the tables of the last _load on the
// device -- a fixed number of bytes per input, per frame and per block -- the counts the load read back, and the host copy of the
// sizes.  buf is borrowed; inOff and inLen are the object's own copies.
struct mi355lz4_frames {
    using DevBuf = mi355lz4_detail::DevBuf;
    int device = 0;
    bool loaded = false;
    FramesArgs a{};                        // what the kernels are handed (the decode fills in out, outOff, result)
    uint64_t total = 0;
    DevBuf perInput, perFrame, perBlock;   // the tables
    DevBuf pin;                            // pinned: {frames, blocks}, then {indep, linked}, then the sizes
    int64_t *sizesHost() const { return (int64_t *)((uint8_t *)pin.p + 64); }
};

// A frame writer (cframes.cpp, kernels_cframes.hip): the scratch of its calls on the device -- a fixed number of
// bytes per input and per entry of the block table, and the slots the engine's internal call compresses into.  Grown on demand
// (mi355lz4_cframes_reserve ahead of time); nothing of a call is kept in it.
struct mi355lz4_cframes {
    using DevBuf = mi355lz4_detail::DevBuf;
    int device = 0;
    DevBuf perInput, perEntry, slots;
};

namespace mi355lz4_detail {

// pageable host memory <-> device through pinned staging, on the engine's stream (api.cpp)
int h2d_staged(mi355lz4_ctx *c, void *dstDev, const uint8_t *srcHost, size_t bytes);
int d2h_staged(mi355lz4_ctx *c, uint8_t *dstHost, const void *srcDev, size_t bytes);

// an engine's switches as the code above the C ABI sees them; _swap_ sets the switch, keeps the stream and returns the old value
int engine_block_checksum(const mi355lz4_ctx *c);
int engine_compression_level(const mi355lz4_ctx *c);
int engine_compress_exact(const mi355lz4_ctx *c);
int engine_swap_compress_exact(mi355lz4_ctx *c, int on);

// the device layer as the host-buffer and legacy layers call it (api.cpp); accel is clamped to 1..65537
EncodeArgs make_encode_args(const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride, int maxBlockLen,
                            int nBlocks, int accel, int headerKind, uint8_t *slots, size_t slotStride, int32_t *framedLen);
int encode_device(mi355lz4_ctx *c, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride,
                  int maxBlockLen, int nBlocks, int accel, int headerKind, uint8_t *slots, size_t slotStride, int32_t *framedLen,
                  int lookBack, const int32_t *hostLen = nullptr);
int decode_device(mi355lz4_ctx *c, const DecodeCall &d);
int streams_check(const mi355lz4_ctx *c, const mi355lz4_cstreams *cs, int nBlocks, const int32_t *streamFirst,
                  const int32_t *streamSlot, int nStreams, const char *who);
int streams_enqueue(mi355lz4_ctx *c, mi355lz4_cstreams *cs, const EncodeArgs &a, int b0, int b1, const int32_t *streamFirst,
                    const int32_t *streamSlot, int nStreams);
int fstreams_check(const mi355lz4_ctx *c, const mi355lz4_fstreams *fs, int nBlocks, const int32_t *streamFirst,
                   const int32_t *streamSlot, int nStreams, const char *who);
int dict_batch_shape_check(const char *who, const char *what, int nBlocks, int headerKind, int maxBlockLen);
int fstreams_enqueue(mi355lz4_ctx *c, mi355lz4_fstreams *fs, const EncodeArgs &a, int b0, int b1, const int32_t *streamFirst,
                     const int32_t *streamSlot, int nStreams);
int dstreams_check(const mi355lz4_ctx *c, const mi355lz4_dstreams *ds, int nBlocks, const int32_t *streamFirst,
                   const int32_t *streamSlot, int nStreams, const char *who);
int dstreams_enqueue(mi355lz4_ctx *c, mi355lz4_dstreams *ds, const DecodeCall &d, int b0, int b1, const int32_t *streamFirst,
                     const int32_t *streamSlot, int nStreams);

}  // namespace mi355lz4_detail
