// streamly_lz4.hpp -- C++ host-side mirror of the reference's operator interface
// for the LZ4 hot path (GHC is not available in the build image, and the
// reference host code is compiled Haskell, so the mirror above the C ABI is C++).
//
// Same names, argument meaning and error behaviour as
//   Streamly.LZ4                 (reference src/Streamly/LZ4.hs:94-122)
//   Streamly.Internal.LZ4        (reference src/Streamly/Internal/LZ4.hs:338-651)
//   Streamly.Internal.LZ4.Config (reference src/Streamly/Internal/LZ4/Config.hs)
// over a pull stream of byte arrays (the analogue of `SerialT m (Array Word8)`).
// Errors the reference raises with `error`/`Parser.die` are thrown as
// streamly_lz4::Error carrying the same message text.
//
// All codec arithmetic happens on the GPU through include/mi355lz4.h; the
// combinators batch `batchBlocks` arrays per call.  There is no CPU codec here.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

struct mi355lz4_ctx;
struct mi355lz4_cstreams;
struct mi355lz4_hcdict;
struct mi355lz4_dictset;
struct mi355lz4_dstreams;
struct mi355lz4_fstreams;
struct mi355lz4_frames;
struct mi355lz4_cframes;

namespace streamly_lz4 {

using Array = std::vector<uint8_t>;                     // Array Word8

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

// Pull stream: next() fills `out` and returns true (Yield), or returns false (Stop).
class ArrayStream {
public:
    virtual ~ArrayStream() = default;
    virtual bool next(Array &out) = 0;
};
using StreamPtr = std::unique_ptr<ArrayStream>;

StreamPtr fromList(std::vector<Array> arrays);          // Stream.fromList
std::vector<Array> toList(ArrayStream &s);              // Stream.toList

// ---- Config.hs:109-136 ------------------------------------------------------
enum class BlockSize { BlockHasSize, BlockMax64KB, BlockMax256KB, BlockMax1MB, BlockMax4MB };
struct BlockConfig {
    BlockSize blockSize = BlockSize::BlockHasSize;
    bool blockChecksum = false;     // every block carries the xxh32 of its data behind it (Config.hs:118-158)
};
struct FrameConfig { bool hasEndMark = false; };
inline BlockConfig defaultBlockConfig() { return BlockConfig{}; }                       // Config.hs:159-160
inline FrameConfig defaultFrameConfig() { return FrameConfig{}; }                       // Config.hs:100-103
inline BlockConfig setBlockMaxSize(BlockSize bs, BlockConfig c) { c.blockSize = bs; return c; }   // Config.hs:139-140
inline FrameConfig setFrameEndMark(bool v, FrameConfig c) { c.hasEndMark = v; return c; }         // Config.hs:78-79
// Config.hs:151 (`undefined` there): block layout | compLen | uncompLen (optional) | data | xxh32(data), LE32 |.  The
// combinators below write and expect the trailer; decoding checks it on the GPU and throws an Error naming the block
// ("block checksum mismatch") after the blocks in front of it have been delivered.
inline BlockConfig setBlockChecksum(bool v, BlockConfig c) { c.blockChecksum = v; return c; }

int metaSize(const BlockConfig &c);                     // Internal/LZ4.hs:177-181
int maxBlockSize(const BlockConfig &c);                 // Internal/LZ4.hs:275-281
int trailerSize(const BlockConfig &c);                  // 4 with setBlockChecksum True, else 0

// GPU engine handle shared by the combinators.
class Engine {
public:
    explicit Engine(int device = 0, size_t batchBlocks = 4096);
    ~Engine();
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;
    mi355lz4_ctx *ctx() const { return ctx_; }
    size_t batchBlocks() const { return batch_; }
    void setBatchBlocks(size_t n) { batch_ = n ? n : 1; }
    // compressChunks then writes a LINKED stream like the reference's (each block's dictionary is the block before it
    // within a batch; Internal/LZ4.hs:376,389 keeps the previous chunk alive for exactly this); decompressChunks
    // reads either kind.  Default off: independent blocks.
    void setLinkedCompress(bool on);
    bool linkedCompress() const { return linked_; }
    // Compression level of compressChunks and lz4FrameCompress (mi355lz4_set_compression_level): 0 (default) the fast
    // encoder, 1..9 the hash-chain encoder (LZ4HC's levels; `speed` is then ignored), 10..12 as 9.  Throws Error otherwise.
    // The streams and frames it writes are ordinary ones: nothing on the decode side changes.
    void setCompressionLevel(int level);
    int compressionLevel() const;
    // Reference-exact compression (mi355lz4_set_compress_exact): compressChunks writes the bytes the reference's
    // compressChunksD writes -- one linked stream, LZ4_compress_fast_continue's -- for level 0.  compressChunks starts a
    // new stream when it starts and continues it across its batches.  Switching it on starts a new stream.
    void setCompressExact(bool on);
    bool compressExact() const;
    void resetCompressStream();
    // Decoded sizes without decoding (mi355lz4_decoded_size_device): what every block of the dense framed stream `framed`
    // (host memory; cfg gives the header kind and whether blocks carry checksum trailers) decodes to, read off the token
    // chains on the GPU: a size, or a negative per-block code (MI355LZ4_BLK_E_SIZE_UNKNOWN where the chain gives none of
    // at most maxUncomp bytes).  Throws Error on a malformed header chain or a failed call.
    std::vector<int32_t> decodedSizes(const BlockConfig &cfg, const Array &framed, int maxUncomp);
    // Partial decode (mi355lz4_decompress_partial): the first `target` bytes of every block of the dense framed stream
    // `framed` (host memory), one array per block -- what LZ4_decompress_safe_partial gives for it; only the prefixes come
    // back from the device.  fixedUncomp: the blocks' capacity when the framing carries no size.  Throws Error on a
    // malformed header chain, a failed block or a failed call.
    std::vector<Array> decompressPartial(const BlockConfig &cfg, const Array &framed, int target, int fixedUncomp = 0);
    // Many exact streams in one call (mi355lz4_compress_streams): streams[s] are the next arrays of the pipeline that owns
    // slot slots[s] of cs; the result holds, per stream, one framed array per input array -- what compressChunksD yields for
    // them at this point of that pipeline's stream.  Throws Error.
    std::vector<std::vector<Array>> compressStreams(const BlockConfig &cfg, int speed, const std::vector<std::vector<Array>> &streams,
                                                    class CompressStreams &cs, const std::vector<int32_t> &slots);
    // Many fast linked streams in one call (mi355lz4_compress_streams_fast): compressStreams' arguments and result with a
    // FastCompressStreams -- the wave encoder at level 0, every array compressed with the last 64 KiB of the array before it in
    // its pipeline as dictionary; not the reference's bytes (compressStreams has those), a linked stream all the same, which
    // decompressStreams reads however it is cut.  All arrays of all pipelines are compressed at once.  Throws Error.
    std::vector<std::vector<Array>> compressStreamsFast(const BlockConfig &cfg, int speed, const std::vector<std::vector<Array>> &streams,
                                                        class FastCompressStreams &fs, const std::vector<int32_t> &slots);
    // Many linked decode streams continued across calls (mi355lz4_decompress_dstreams): streams[s] are the next resized
    // blocks (header + data each) of the pipeline that owns slot slots[s] of ds; the result holds, per stream, one decoded
    // array per block -- what decompressChunksRawD yields for them at this point of that pipeline's stream; the previous
    // output it threads through lives in the slot, on the device.  Throws Error (a failed block included).
    std::vector<std::vector<Array>> decompressStreams(const BlockConfig &cfg, const std::vector<std::vector<Array>> &streams,
                                                      class DecompressStreams &ds, const std::vector<int32_t> &slots);
    // Shared-dictionary batches (mi355lz4_compress_dict / mi355lz4_decompress_dict).  compressWithDict: every array compressed
    // on its own against slot `slot` of cs, which CompressStreams::loadDict has loaded -- one framed array per input array, the
    // reference's bytes for LZ4_loadDict + LZ4_compress_fast_continue on a copy of the loaded stream; the slot is only read.
    // decompressWithDict: resized blocks (header + data each), every one decoded against `dict` (host memory, may be empty) as
    // LZ4_decompress_safe_usingDict does -- one decoded array per block.  Both throw Error (a failed block included).
    std::vector<Array> compressWithDict(const BlockConfig &cfg, int speed, const std::vector<Array> &arrays,
                                        const class CompressStreams &cs, int slot);
    std::vector<Array> decompressWithDict(const BlockConfig &cfg, const std::vector<Array> &blocks, const Array &dict);
    // The same batch at the engine's compression level 1..12 (mi355lz4_compress_hcdict): every array compressed on its own by
    // the hash-chain encoder with the dictionary of `hd` (HcDict::load) in front of it -- lz4 -9 -D dict; decompressWithDict
    // reads the result with the dictionary's bytes.  The object is only read.  Throws Error (level 0 included).
    std::vector<Array> compressWithDictHC(const BlockConfig &cfg, const std::vector<Array> &arrays, const class HcDict &hd);
    // The same batch at level 0 by the wave encoder (mi355lz4_compress_fastdict): the engine's own fast parse against the
    // dictionary of `hd`, not the reference's bytes (compressWithDict has those); decompressWithDict reads the result.
    std::vector<Array> compressWithDictFast(const BlockConfig &cfg, const std::vector<Array> &arrays, const class HcDict &hd, int accel = 1);
    // The same batch with a dictionary per array (mi355lz4_compress_fastdict_multi): array i against member dictIdx[i] of `ds`
    // (-1: none), the bytes compressWithDictFast writes for it against that member alone.  decompressWithDicts reads the result:
    // block i against the kept bytes of member dictIdx[i] (mi355lz4_decompress_dict_multi).  One index per array; an index that
    // names no member throws Error before anything runs.  The set and its members are only read.
    std::vector<Array> compressWithDictsFast(const BlockConfig &cfg, const std::vector<Array> &arrays, const class DictSet &ds,
                                             const std::vector<int32_t> &dictIdx, int accel = 1);
    std::vector<Array> decompressWithDicts(const BlockConfig &cfg, const std::vector<Array> &blocks, const class DictSet &ds,
                                           const std::vector<int32_t> &dictIdx);
    // Fixed-size output pages (mi355lz4_compress_pages): every array cut into a chain of at most maxPages pages whose blocks are
    // at most pageSize bytes -- page k is what LZ4_compress_destSize makes of the bytes behind pages 0..k-1.  Per input the pages in
    // order, each with cfg's header in front of its block (an ordinary block for decompressChunks when the header carries both
    // sizes), and in `consumed` (when given) the bytes of every input its pages hold: less than its length when maxPages was too
    // few.  Throws Error (block checksums in cfg included: pages carry no trailer).
    std::vector<std::vector<Array>> compressPages(const BlockConfig &cfg, const std::vector<Array> &arrays, int pageSize, int maxPages,
                                                  std::vector<int32_t> *consumed = nullptr);
    // The same chains at the engine's speed (mi355lz4_compress_pages_fast): every page is a prefix of the sequences this engine's
    // level-0 encoder finds in the next 64 KiB at the most, closed by the literal run that fills the page -- valid, independently
    // decodable pages, not LZ4_compress_destSize's bytes; highly compressible input gives pages that are not full.  Level 0 only.
    std::vector<std::vector<Array>> compressPagesFast(const BlockConfig &cfg, const std::vector<Array> &arrays, int pageSize, int maxPages,
                                                      std::vector<int32_t> *consumed = nullptr, int accel = 1);
    // ... with the dictionary of a loaded HcDict in front of every page (mi355lz4_compress_pages_fastdict): a page is a prefix of the
    // block compressWithDictFast writes for the next 64 KiB at the most, and decodes with decompressWithDict and the same dictionary.
    // Small records fill about half as many pages as without the dictionary.  Level 0 only; the object is only read.
    std::vector<std::vector<Array>> compressPagesWithDictFast(const BlockConfig &cfg, const std::vector<Array> &arrays, const class HcDict &hd,
                                                              int pageSize, int maxPages, std::vector<int32_t> *consumed = nullptr,
                                                              int accel = 1);
    // Many inputs of standard LZ4 frames in one call (mi355lz4_decompress_frames): each input is what `lz4 -d` accepts -- any
    // sequence of LZ4 frames and skippable frames, or nothing -- and comes back decoded.  The batched counterpart of
    // lz4FrameDecompress below, parsed, sized and decoded on the device.  When some input fails, throws Error; with `result`
    // given it does not: result[i] is then input i's size or its MI355LZ4_FRM_E_* code, and a failed input's array is empty.
    std::vector<Array> decompressFrames(const std::vector<Array> &inputs, unsigned flags = 0, std::vector<int64_t> *result = nullptr);
    // Many inputs, one standard LZ4 frame each, in one call (mi355lz4_compress_frames): the batched counterpart of
    // lz4FrameCompress below, cut into blocks, compressed and laid out on the device.  blockSizeId 4..7 (64 KiB .. 4 MiB), flags
    // MI355LZ4_CFRAMES_*; the engine's compression level applies.  Throws Error.
    std::vector<Array> compressFrames(const std::vector<Array> &inputs, int blockSizeId = 4, unsigned flags = 0, int accel = 1);
private:
    mi355lz4_ctx *ctx_ = nullptr;
    size_t batch_;
    bool linked_ = false;
};

// A parsed batch of standard LZ4 frames on the engine's device (mi355lz4_frames), for callers whose data is device-resident:
// load() parses many inputs and returns their exact decoded sizes (it waits for the engine's stream), decode() decodes them all
// and only enqueues.  All pointers are DEVICE memory; buf is borrowed until the decodes that use it have run.
class Frames {
public:
    explicit Frames(Engine &eng);                       // throws Error
    ~Frames();
    Frames(const Frames &) = delete;
    Frames &operator=(const Frames &) = delete;
    mi355lz4_frames *handle() const { return fr_; }
    // input i is buf[inOff[i], inOff[i] + inLen[i]); the sizes or MI355LZ4_FRM_E_* codes, one per input; replaces the last load
    std::vector<int64_t> load(const uint8_t *buf, uint64_t bufLen, const uint64_t *inOff, const uint64_t *inLen, int nInputs,
                              unsigned flags = 0);
    int inputs() const;
    int blocks() const;
    uint64_t total() const;                             // sum of the sizes >= 0
    const int64_t *sizesDevice() const;
    // input i with a size goes to out[outOff[i], outOff[i] + size); result[i] = its size or a code
    void decode(uint8_t *out, const uint64_t *outOff, int64_t *result);
private:
    Engine &eng_;
    mi355lz4_frames *fr_ = nullptr;
};

// A frame writer on the engine's device (mi355lz4_cframes), for callers whose data is device-resident: compress() turns many
// inputs into one standard LZ4 frame each and only enqueues once the scratch is there (reserve(), or an earlier call of the
// shape).  All pointers are DEVICE memory; frameLen[i] is frame i's length or an MI355LZ4_FRW_E_* code.
class FrameWriter {
public:
    explicit FrameWriter(Engine &eng);                  // throws Error
    ~FrameWriter();
    FrameWriter(const FrameWriter &) = delete;
    FrameWriter &operator=(const FrameWriter &) = delete;
    mi355lz4_cframes *handle() const { return w_; }
    static uint64_t bound(uint64_t len, int blockSizeId, unsigned flags);     // the exact worst case of one frame
    void reserve(int nInputs, uint64_t maxInputLen, uint64_t totalLen, int blockSizeId);
    // input i is src[inOff[i], inOff[i] + inLen[i]) and becomes one frame at dst + dstOff[i], dstCap[i] bytes at the most
    void compress(const uint8_t *src, uint64_t srcBufLen, const uint64_t *inOff, const uint64_t *inLen, int nInputs, uint64_t maxInputLen,
                  uint64_t totalLen, int blockSizeId, unsigned flags, int accel, uint8_t *dst, const uint64_t *dstOff,
                  const uint64_t *dstCap, int64_t *frameLen);
private:
    Engine &eng_;
    mi355lz4_cframes *w_ = nullptr;
};

// A set of nSlots device-resident reference-exact compress streams (mi355lz4_cstreams: about 80 KiB a slot), one per
// pipeline a host runs at once; Engine::compressStreams compresses the next arrays of many of them in one call.
class CompressStreams {
public:
    CompressStreams(Engine &eng, int nSlots);          // every slot reset; throws Error
    ~CompressStreams();
    CompressStreams(const CompressStreams &) = delete;
    CompressStreams &operator=(const CompressStreams &) = delete;
    mi355lz4_cstreams *handle() const { return cs_; }
    int count() const;
    void reset();                                       // LZ4_resetStream, all slots
    void reset(const std::vector<int32_t> &slots);      // ... the listed ones
    // LZ4_loadDict on a slot (mi355lz4_cstreams_load_dict): table, currentOffset 65536 and the last 64 KiB of
    // dictDevice[0, len) (DEVICE memory; under 8 bytes: no dictionary); enqueued, the slot keeps its own copy
    void loadDict(int slot, const uint8_t *dictDevice, int len);
private:
    Engine &eng_;
    mi355lz4_cstreams *cs_ = nullptr;
};

// A set of nSlots device-resident fast linked compress streams (mi355lz4_fstreams: about 64 KiB a slot, the last array's last
// 64 KiB and their count), one per pipeline a host runs at once; Engine::compressStreamsFast continues many of them in one call.
class FastCompressStreams {
public:
    FastCompressStreams(Engine &eng, int nSlots);      // every slot reset; throws Error
    ~FastCompressStreams();
    FastCompressStreams(const FastCompressStreams &) = delete;
    FastCompressStreams &operator=(const FastCompressStreams &) = delete;
    mi355lz4_fstreams *handle() const { return fs_; }
    int count() const;
    void reset();                                       // no dictionary, all slots
    void reset(const std::vector<int32_t> &slots);      // ... the listed ones
    // mi355lz4_fstreams_set_dict: the slot becomes the last 64 KiB of dictDevice[0, len) (DEVICE memory; len 0 equals a
    // reset); enqueued, the slot keeps its own copy
    void setDict(int slot, const uint8_t *dictDevice, int len);
    // mi355lz4_fstreams_set_level: the set's compression level for the calls made after it -- 0 the wave encoder (default), 1..12
    // the hash-chain encoder; a host-side attribute, nothing is enqueued.  Throws Error outside 0..12 (the level stays).
    void setLevel(int level);
    int level() const;
private:
    Engine &eng_;
    mi355lz4_fstreams *fs_ = nullptr;
};

// A prepared high-compression dictionary on the engine's device (mi355lz4_hcdict: about 216 KiB -- the dictionary's last 64 KiB
// and the image of the hash-chain encoder's tables after its inserts), for Engine::compressWithDictHC.
class HcDict {
public:
    explicit HcDict(Engine &eng);                       // the empty dictionary; throws Error
    ~HcDict();
    HcDict(const HcDict &) = delete;
    HcDict &operator=(const HcDict &) = delete;
    mi355lz4_hcdict *handle() const { return hd_; }
    int size() const;                                   // bytes the last load kept: min(len, 65536)
    // builds the image from dictDevice[0, len) (DEVICE memory); enqueued, the object keeps its own copy; replaces the last load
    void load(const uint8_t *dictDevice, int len);
private:
    Engine &eng_;
    mi355lz4_hcdict *hd_ = nullptr;
};

// A set of prepared dictionaries (mi355lz4_dictset), for Engine::compressWithDictsFast / decompressWithDicts, where every array
// names its member.  The members are borrowed: they must outlive the set (the same one may stand at several indices), and
// HcDict::load on a member is seen by the set without a new one.
class DictSet {
public:
    DictSet(Engine &eng, const std::vector<const HcDict *> &members);   // 1..65536 members on the engine's device; throws Error
    ~DictSet();
    DictSet(const DictSet &) = delete;
    DictSet &operator=(const DictSet &) = delete;
    mi355lz4_dictset *handle() const { return ds_; }
    int count() const;
private:
    mi355lz4_dictset *ds_ = nullptr;
};

// A set of nSlots device-resident linked decode streams (mi355lz4_dstreams: about 64 KiB a slot -- the last block's last
// 64 KiB and their count), one per pipeline a host runs at once; Engine::decompressStreams decodes the next blocks of many
// of them in one call.
class DecompressStreams {
public:
    DecompressStreams(Engine &eng, int nSlots);        // every slot reset; throws Error
    ~DecompressStreams();
    DecompressStreams(const DecompressStreams &) = delete;
    DecompressStreams &operator=(const DecompressStreams &) = delete;
    mi355lz4_dstreams *handle() const { return ds_; }
    int count() const;
    void reset();                                       // no dictionary, all slots
    void reset(const std::vector<int32_t> &slots);      // ... the listed ones
    // LZ4_setStreamDecode: the slot's state becomes the last 64 KiB of dictDevice[0, len) (DEVICE memory); enqueued
    void setDict(int slot, const uint8_t *dictDevice, int len);
private:
    Engine &eng_;
    mi355lz4_dstreams *ds_ = nullptr;
};

// ---- Streamly.LZ4 / Streamly.Internal.LZ4 -------------------------------------
// compressChunks cfg speed          (LZ4.hs:94-100, Internal/LZ4.hs:353-394)
StreamPtr compressChunks(const BlockConfig &cfg, int speed, StreamPtr in, Engine &eng);
// resizeChunksD cfg conf            (Internal/LZ4.hs:432-523)
StreamPtr resizeChunks(const BlockConfig &cfg, const FrameConfig &conf, StreamPtr in);
// decompressChunksRawD cfg          (Internal/LZ4.hs:539-567)
StreamPtr decompressChunksRaw(const BlockConfig &cfg, StreamPtr in, Engine &eng);
// decompressChunks cfg = decompressChunksRawD cfg . resizeChunksD cfg defaultFrameConfig  (LZ4.hs:114-122)
StreamPtr decompressChunks(const BlockConfig &cfg, StreamPtr in, Engine &eng);
// decompressChunks over a BATCH of arrays that lie back to back in one buffer (array i = lens[i] bytes), the result as
// slices of ONE buffer.  Same results and same errors as decompressChunks over fromList of those arrays.  Why it
// exists: an `Array Word8` of the reference is a slice of a shared buffer, so its combinators move no bytes between
// stages; Array here is an owning vector and the array-at-a-time form above pays an allocation and a copy per array
// and per stage (1.1 ms for the reference's own 10 MiB benchmark files -- more than the GPU call).  This form makes
// the copies the reference would make: none on the way in, one (device -> host) on the way out.
struct ArrayBatch {
    uint8_t *buf = nullptr;             // the arrays' bytes, back to back (not zero-filled; recycled by release())
    size_t cap = 0;
    std::vector<size_t> off;            // array i = buf[off[i] .. off[i + 1]); size() = arrays + 1
    size_t count() const { return off.empty() ? 0 : off.size() - 1; }
    void release();                     // hands the buffer back (kept for the next call: no fresh page faults)
    ArrayBatch() = default;
    ArrayBatch(ArrayBatch &&o) noexcept : buf(o.buf), cap(o.cap), off(std::move(o.off)) { o.buf = nullptr; o.cap = 0; }
    ArrayBatch &operator=(ArrayBatch &&o) noexcept { release(); buf = o.buf; cap = o.cap; off = std::move(o.off); o.buf = nullptr; o.cap = 0; return *this; }
    ArrayBatch(const ArrayBatch &) = delete;
    ArrayBatch &operator=(const ArrayBatch &) = delete;
    ~ArrayBatch() { release(); }
};
ArrayBatch decompressChunksBatch(const BlockConfig &cfg, const FrameConfig &conf, const uint8_t *data,
                                 const uint64_t *lens, size_t n, Engine &eng);
// Released result buffers are kept for the next call (at most four, 64 MiB in all); this hands them back to the allocator.
void trimBuffers();
// simpleFrameParserD                (Internal/LZ4.hs:590-651): consumes the 7-byte
// frame header from the head of the stream; returns the parsed configs and the
// stream of what follows.
std::pair<std::pair<BlockConfig, FrameConfig>, StreamPtr> simpleFrameParser(StreamPtr in);
// decompressChunksWithD simpleFrameParserD  (Internal/LZ4.hs:569-577)
StreamPtr decompressChunksWith(StreamPtr in, Engine &eng);

// ---- the standard LZ4 frame format (interop with liblz4's LZ4F_* and the lz4 CLI) ----
// What simpleFrameParserD stops short of (Internal/LZ4.hs:631-638 rejects independent blocks, checksums and
// content size; :605 skips the header checksum): csrc/lz4_frame.cpp.
struct Lz4FrameOptions {
    BlockSize blockMax = BlockSize::BlockMax64KB;       // BD byte; one of BlockMax64KB .. BlockMax4MB
    bool blockChecksum = false;                         // xxh32 behind every block
    bool contentChecksum = true;                        // xxh32 of the content behind the end mark (the CLI's default)
    bool contentSize = false;                           // 8-byte content size in the descriptor
    bool linkedBlocks = false;                          // block-dependent frame (the lz4 tool's default): smaller on text
};
uint32_t xxh32(const uint8_t *p, size_t len, uint32_t seed);
// One frame (all blocks in one batch; independent blocks unless opt.linkedBlocks).
Array lz4FrameCompress(const Array &data, int speed, Engine &eng, const Lz4FrameOptions &opt = Lz4FrameOptions());
// Host half of the reader: parses ONE frame at frame[at...] (advancing at), verifies header and block checksums and
// re-frames the blocks for the engine ([compLen LE32][LZ4 block], stored blocks as literal-only blocks).
// Returns false for a skippable frame.
struct Lz4FrameIndex {
    bool independent = false, hasContentSize = false, hasContentChecksum = false;
    size_t blockMax = 0;
    uint64_t contentSize = 0;
    uint32_t contentChecksum = 0;
    Array framed;
    std::vector<size_t> blockAt;                        // offsets of the block headers in framed, plus its size
};
bool lz4FrameParse(const Array &frame, size_t &at, Lz4FrameIndex &ix);
// Any sequence of frames and skippable frames; linked or independent blocks, stored blocks, all checksums verified.
Array lz4FrameDecompress(const Array &frame, Engine &eng);

} // namespace streamly_lz4
