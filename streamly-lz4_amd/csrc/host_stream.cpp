// host_stream.cpp -- C++ mirror of Streamly.LZ4 / Streamly.Internal.LZ4 stream
// combinators (include/streamly_lz4.hpp) over the batched GPU ABI, plus a small
// C surface (slz4_*) so that tests and other languages can drive them.
//
// Host logic only (state machines, header bookkeeping, batching).  Every codec
// byte is produced by the GPU through mi355lz4_compress_batch /
// mi355lz4_decompress_batch.  Reference line numbers refer to
// src/Streamly/Internal/LZ4.hs unless stated otherwise.
#include "../../include/streamly_lz4.hpp"
#include "../../include/mi355lz4.h"
#include "block_checksum_scope.hpp"

#include <cstring>
#include <deque>
#include <mutex>
#include <string>

namespace streamly_lz4 {

// ---------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------
static int32_t le32(const uint8_t *p)
{
    return (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}

int metaSize(const BlockConfig &c) { return c.blockSize == BlockSize::BlockHasSize ? 8 : 4; }   // :177-181

int maxBlockSize(const BlockConfig &c)                                                           // :275-281
{
    switch (c.blockSize) {
    case BlockSize::BlockHasSize: return MI355LZ4_MAX_INPUT_SIZE;
    case BlockSize::BlockMax64KB: return 64 * 1024;
    case BlockSize::BlockMax256KB: return 256 * 1024;
    case BlockSize::BlockMax1MB: return 1024 * 1024;
    case BlockSize::BlockMax4MB: return 4 * 1024 * 1024;
    }
    return 0;
}

int trailerSize(const BlockConfig &c) { return c.blockChecksum ? 4 : 0; }

static int fixedUncompSize(const BlockConfig &c)                                                 // :189-198
{
    return c.blockSize == BlockSize::BlockHasSize ? 0 : maxBlockSize(c);
}

namespace {
class ListStream : public ArrayStream {
public:
    explicit ListStream(std::vector<Array> a) : arrays_(std::move(a)) {}
    bool next(Array &out) override
    {
        if (pos_ >= arrays_.size()) return false;
        out = std::move(arrays_[pos_++]);
        return true;
    }
private:
    std::vector<Array> arrays_;
    size_t pos_ = 0;
};
} // namespace

StreamPtr fromList(std::vector<Array> arrays) { return StreamPtr(new ListStream(std::move(arrays))); }

std::vector<Array> toList(ArrayStream &s)
{
    std::vector<Array> out;
    Array a;
    while (s.next(a)) out.push_back(std::move(a));
    return out;
}

// ---------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------
Engine::Engine(int device, size_t batchBlocks) : batch_(batchBlocks ? batchBlocks : 1)
{
    if (mi355lz4_create(&ctx_, device) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::Engine: ") + mi355lz4_last_error());
}
void Engine::setLinkedCompress(bool on) { mi355lz4_set_linked_compress(ctx_, on ? 1 : 0); linked_ = on; }
void Engine::setCompressionLevel(int level)
{
    if (mi355lz4_set_compression_level(ctx_, level) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::Engine::setCompressionLevel: ") + mi355lz4_last_error());
}
int Engine::compressionLevel() const { return mi355lz4_get_compression_level(ctx_); }
void Engine::setCompressExact(bool on)
{
    if (mi355lz4_set_compress_exact(ctx_, on ? 1 : 0) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::Engine::setCompressExact: ") + mi355lz4_last_error());
}
bool Engine::compressExact() const { return mi355lz4_get_compress_exact(ctx_) == 1; }
void Engine::resetCompressStream()
{
    if (mi355lz4_compress_exact_reset(ctx_) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::Engine::resetCompressStream: ") + mi355lz4_last_error());
}

Engine::~Engine() { mi355lz4_destroy(ctx_); }

// host bytes -> device, the size pass, sizes back (mi355lz4_decoded_sizes_host)
std::vector<int32_t> Engine::decodedSizes(const BlockConfig &cfg, const Array &framed, int maxUncomp)
{
    const int hk = metaSize(cfg);
    const BlockChecksumScope scope(ctx_, cfg.blockChecksum);
    std::vector<uint64_t> off(framed.size() / (size_t)(hk + 1) + 2);
    int n = 0;
    if (mi355lz4_index_host_ex(framed.data(), framed.size(), hk, maxUncomp, cfg.blockChecksum ? 1 : 0, off.data(), nullptr,
                               (int)off.size() - 1, &n) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::Engine::decodedSizes: ") + mi355lz4_last_error());
    std::vector<int32_t> size((size_t)n);
    if (n && mi355lz4_decoded_sizes_host(ctx_, framed.data(), framed.size(), off.data(), n, hk, maxUncomp, size.data()) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::Engine::decodedSizes: ") + mi355lz4_last_error());
    return size;
}

// host bytes -> device, one partial decode, the prefixes back (mi355lz4_decompress_partial).  The chain is indexed first, so the
// buffer the prefixes come back in is sum(min(target, capacity)) bytes and not a worst case.
std::vector<Array> Engine::decompressPartial(const BlockConfig &cfg, const Array &framed, int target, int fixedUncomp)
{
    const int hk = metaSize(cfg);
    const BlockChecksumScope scope(ctx_, cfg.blockChecksum);
    std::vector<uint64_t> off(framed.size() / (size_t)(hk + 1) + 2);
    std::vector<int32_t> len(off.size());
    int n = 0;
    if (mi355lz4_index_host_ex(framed.data(), framed.size(), hk, fixedUncomp, cfg.blockChecksum ? 1 : 0, off.data(), len.data(),
                               (int)off.size() - 1, &n) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::Engine::decompressPartial: ") + mi355lz4_last_error());
    size_t room = 0;
    for (int k = 0; k < n; k++)
        if (target > 0 && len[(size_t)k] > 0) room += (size_t)(target < len[(size_t)k] ? target : len[(size_t)k]);
    Array packed(room + 16);
    size_t outLen = 0;
    int got = 0;
    if (mi355lz4_decompress_partial(ctx_, framed.data(), framed.size(), hk, fixedUncomp, nullptr, target, packed.data(), room,
                                    &outLen, len.data(), n, &got) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::Engine::decompressPartial: ") + mi355lz4_last_error());
    std::vector<Array> out((size_t)got);
    size_t pos = 0;
    for (int k = 0; k < got; k++) {
        out[(size_t)k].assign(packed.begin() + (ptrdiff_t)pos, packed.begin() + (ptrdiff_t)(pos + (size_t)len[(size_t)k]));
        pos += (size_t)len[(size_t)k];
    }
    return out;
}

CompressStreams::CompressStreams(Engine &eng, int nSlots) : eng_(eng)
{
    if (mi355lz4_cstreams_create(eng.ctx(), nSlots, &cs_) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::CompressStreams: ") + mi355lz4_last_error());
}
CompressStreams::~CompressStreams() { mi355lz4_cstreams_destroy(cs_); }
int CompressStreams::count() const { return mi355lz4_cstreams_count(cs_); }
void CompressStreams::reset()
{
    if (mi355lz4_cstreams_reset(eng_.ctx(), cs_, nullptr, 0) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::CompressStreams::reset: ") + mi355lz4_last_error());
}
void CompressStreams::reset(const std::vector<int32_t> &slots)
{
    if (slots.empty()) return;
    if (mi355lz4_cstreams_reset(eng_.ctx(), cs_, slots.data(), (int)slots.size()) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::CompressStreams::reset: ") + mi355lz4_last_error());
}

std::vector<std::vector<Array>> Engine::compressStreams(const BlockConfig &cfg, int speed, const std::vector<std::vector<Array>> &streams,
                                                        CompressStreams &cs, const std::vector<int32_t> &slots)
{
    if (slots.size() != streams.size()) throw Error("compressStreams: one slot per stream");
    const int meta = metaSize(cfg);
    std::vector<const uint8_t *> ptrs;
    std::vector<int32_t> lens, first{0};
    size_t cap = 16;
    for (const auto &st : streams) {
        for (const Array &a : st) {
            if (a.size() > (size_t)maxBlockSize(cfg))                           // compressChunk, Internal/LZ4.hs:237-241
                throw Error("compressChunk: Source array length " + std::to_string(a.size()) +
                            " exceeds the maximum block size of " + std::to_string(maxBlockSize(cfg)));
            ptrs.push_back(a.data());
            lens.push_back((int32_t)a.size());
            cap += (size_t)mi355lz4_compress_bound((int)a.size()) + (size_t)meta + 4;
        }
        first.push_back((int32_t)lens.size());
    }
    const int n = (int)lens.size();
    std::vector<uint8_t> framed(cap);
    std::vector<int32_t> flen((size_t)n + 1), status((size_t)n + 1);
    ptrs.push_back(nullptr);
    lens.push_back(0);
    size_t outLen = 0;
    if (mi355lz4_compress_streams(ctx_, cs.handle(), ptrs.data(), lens.data(), n, first.data(), slots.data(), (int)streams.size(),
                                  speed < 0 ? 0 : speed, meta, framed.data(), cap, &outLen, flen.data(), status.data()) != MI355LZ4_OK)
        throw Error(std::string("compressStreams: ") + mi355lz4_last_error());
    std::vector<std::vector<Array>> out(streams.size());
    size_t pos = 0;
    int k = 0;
    for (size_t s = 0; s < streams.size(); s++)
        for (size_t i = 0; i < streams[s].size(); i++, k++) {
            out[s].emplace_back(framed.begin() + (long)pos, framed.begin() + (long)(pos + (size_t)flen[(size_t)k]));
            pos += (size_t)flen[(size_t)k];
        }
    return out;
}

FastCompressStreams::FastCompressStreams(Engine &eng, int nSlots) : eng_(eng)
{
    if (mi355lz4_fstreams_create(eng.ctx(), nSlots, &fs_) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::FastCompressStreams: ") + mi355lz4_last_error());
}
FastCompressStreams::~FastCompressStreams() { mi355lz4_fstreams_destroy(fs_); }
int FastCompressStreams::count() const { return mi355lz4_fstreams_count(fs_); }
void FastCompressStreams::reset()
{
    if (mi355lz4_fstreams_reset(eng_.ctx(), fs_, nullptr, 0) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::FastCompressStreams::reset: ") + mi355lz4_last_error());
}
void FastCompressStreams::reset(const std::vector<int32_t> &slots)
{
    if (slots.empty()) return;
    if (mi355lz4_fstreams_reset(eng_.ctx(), fs_, slots.data(), (int)slots.size()) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::FastCompressStreams::reset: ") + mi355lz4_last_error());
}
void FastCompressStreams::setDict(int slot, const uint8_t *dictDevice, int len)
{
    if (mi355lz4_fstreams_set_dict(eng_.ctx(), fs_, slot, dictDevice, len) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::FastCompressStreams::setDict: ") + mi355lz4_last_error());
}
void FastCompressStreams::setLevel(int level)
{
    if (mi355lz4_fstreams_set_level(fs_, level) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::FastCompressStreams::setLevel: ") + mi355lz4_last_error());
}
int FastCompressStreams::level() const { return mi355lz4_fstreams_get_level(fs_); }

std::vector<std::vector<Array>> Engine::compressStreamsFast(const BlockConfig &cfg, int speed, const std::vector<std::vector<Array>> &streams,
                                                        FastCompressStreams &fs, const std::vector<int32_t> &slots)
{
    if (slots.size() != streams.size()) throw Error("compressStreamsFast: one slot per stream");
    const int meta = metaSize(cfg);
    std::vector<const uint8_t *> ptrs;
    std::vector<int32_t> lens, first{0};
    size_t cap = 16;
    for (const auto &st : streams) {
        for (const Array &a : st) {
            if (a.size() > (size_t)maxBlockSize(cfg))                           // compressChunk, Internal/LZ4.hs:237-241
                throw Error("compressChunk: Source array length " + std::to_string(a.size()) +
                            " exceeds the maximum block size of " + std::to_string(maxBlockSize(cfg)));
            ptrs.push_back(a.data());
            lens.push_back((int32_t)a.size());
            cap += (size_t)mi355lz4_compress_bound((int)a.size()) + (size_t)meta + 4;
        }
        first.push_back((int32_t)lens.size());
    }
    const int n = (int)lens.size();
    std::vector<uint8_t> framed(cap);
    std::vector<int32_t> flen((size_t)n + 1), status((size_t)n + 1);
    ptrs.push_back(nullptr);
    lens.push_back(0);
    size_t outLen = 0;
    if (mi355lz4_compress_streams_fast(ctx_, fs.handle(), ptrs.data(), lens.data(), n, first.data(), slots.data(), (int)streams.size(),
                                  speed < 0 ? 0 : speed, meta, framed.data(), cap, &outLen, flen.data(), status.data()) != MI355LZ4_OK)
        throw Error(std::string("compressStreamsFast: ") + mi355lz4_last_error());
    std::vector<std::vector<Array>> out(streams.size());
    size_t pos = 0;
    int k = 0;
    for (size_t s = 0; s < streams.size(); s++)
        for (size_t i = 0; i < streams[s].size(); i++, k++) {
            out[s].emplace_back(framed.begin() + (long)pos, framed.begin() + (long)(pos + (size_t)flen[(size_t)k]));
            pos += (size_t)flen[(size_t)k];
        }
    return out;
}

void CompressStreams::loadDict(int slot, const uint8_t *dictDevice, int len)
{
    if (mi355lz4_cstreams_load_dict(eng_.ctx(), cs_, slot, dictDevice, len) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::CompressStreams::loadDict: ") + mi355lz4_last_error());
}

std::vector<Array> Engine::compressWithDict(const BlockConfig &cfg, int speed, const std::vector<Array> &arrays, const CompressStreams &cs,
                                            int slot)
{
    const int meta = metaSize(cfg);
    std::vector<const uint8_t *> ptrs;
    std::vector<int32_t> lens;
    size_t cap = 16;
    for (const Array &a : arrays) {
        if (a.size() > (size_t)maxBlockSize(cfg))                               // compressChunk, Internal/LZ4.hs:237-241
            throw Error("compressChunk: Source array length " + std::to_string(a.size()) +
                        " exceeds the maximum block size of " + std::to_string(maxBlockSize(cfg)));
        ptrs.push_back(a.data());
        lens.push_back((int32_t)a.size());
        cap += (size_t)mi355lz4_compress_bound((int)a.size()) + (size_t)meta + 4;
    }
    const int n = (int)lens.size();
    std::vector<uint8_t> framed(cap);
    std::vector<int32_t> flen((size_t)n + 1), status((size_t)n + 1);
    ptrs.push_back(nullptr);
    lens.push_back(0);
    size_t outLen = 0;
    if (mi355lz4_compress_dict(ctx_, cs.handle(), slot, ptrs.data(), lens.data(), n, speed < 0 ? 0 : speed, meta, framed.data(), cap,
                               &outLen, flen.data(), status.data()) != MI355LZ4_OK)
        throw Error(std::string("compressWithDict: ") + mi355lz4_last_error());
    std::vector<Array> out;
    size_t pos = 0;
    for (int k = 0; k < n; k++) {
        out.emplace_back(framed.begin() + (long)pos, framed.begin() + (long)(pos + (size_t)flen[(size_t)k]));
        pos += (size_t)flen[(size_t)k];
    }
    return out;
}

HcDict::HcDict(Engine &eng) : eng_(eng)
{
    if (mi355lz4_hcdict_create(eng.ctx(), &hd_) != MI355LZ4_OK) throw Error(std::string("streamly_lz4::HcDict: ") + mi355lz4_last_error());
}
HcDict::~HcDict() { mi355lz4_hcdict_destroy(hd_); }
int HcDict::size() const { return mi355lz4_hcdict_size(hd_); }
void HcDict::load(const uint8_t *dictDevice, int len)
{
    if (mi355lz4_hcdict_load(eng_.ctx(), hd_, dictDevice, len) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::HcDict::load: ") + mi355lz4_last_error());
}

std::vector<Array> Engine::compressWithDictHC(const BlockConfig &cfg, const std::vector<Array> &arrays, const HcDict &hd)
{
    const int meta = metaSize(cfg);
    std::vector<const uint8_t *> ptrs;
    std::vector<int32_t> lens;
    size_t cap = 16;
    for (const Array &a : arrays) {
        if (a.size() > (size_t)maxBlockSize(cfg))                               // compressChunk, Internal/LZ4.hs:237-241
            throw Error("compressChunk: Source array length " + std::to_string(a.size()) +
                        " exceeds the maximum block size of " + std::to_string(maxBlockSize(cfg)));
        ptrs.push_back(a.data());
        lens.push_back((int32_t)a.size());
        cap += (size_t)mi355lz4_compress_bound((int)a.size()) + (size_t)meta + 4;
    }
    const int n = (int)lens.size();
    std::vector<uint8_t> framed(cap);
    std::vector<int32_t> flen((size_t)n + 1), status((size_t)n + 1);
    ptrs.push_back(nullptr);
    lens.push_back(0);
    size_t outLen = 0;
    if (mi355lz4_compress_hcdict(ctx_, hd.handle(), ptrs.data(), lens.data(), n, meta, framed.data(), cap, &outLen, flen.data(),
                                 status.data()) != MI355LZ4_OK)
        throw Error(std::string("compressWithDictHC: ") + mi355lz4_last_error());
    std::vector<Array> out;
    size_t pos = 0;
    for (int k = 0; k < n; k++) {
        out.emplace_back(framed.begin() + (long)pos, framed.begin() + (long)(pos + (size_t)flen[(size_t)k]));
        pos += (size_t)flen[(size_t)k];
    }
    return out;
}

std::vector<Array> Engine::compressWithDictFast(const BlockConfig &cfg, const std::vector<Array> &arrays, const HcDict &hd, int accel)
{
    const int meta = metaSize(cfg);
    std::vector<const uint8_t *> ptrs;
    std::vector<int32_t> lens;
    size_t cap = 16;
    for (const Array &a : arrays) {
        if (a.size() > (size_t)maxBlockSize(cfg))                               // compressChunk, Internal/LZ4.hs:237-241
            throw Error("compressChunk: Source array length " + std::to_string(a.size()) +
                        " exceeds the maximum block size of " + std::to_string(maxBlockSize(cfg)));
        ptrs.push_back(a.data());
        lens.push_back((int32_t)a.size());
        cap += (size_t)mi355lz4_compress_bound((int)a.size()) + (size_t)meta + 4;
    }
    const int n = (int)lens.size();
    std::vector<uint8_t> framed(cap);
    std::vector<int32_t> flen((size_t)n + 1), status((size_t)n + 1);
    ptrs.push_back(nullptr);
    lens.push_back(0);
    size_t outLen = 0;
    if (mi355lz4_compress_fastdict(ctx_, hd.handle(), ptrs.data(), lens.data(), n, accel, meta, framed.data(), cap, &outLen, flen.data(),
                                 status.data()) != MI355LZ4_OK)
        throw Error(std::string("compressWithDictFast: ") + mi355lz4_last_error());
    std::vector<Array> out;
    size_t pos = 0;
    for (int k = 0; k < n; k++) {
        out.emplace_back(framed.begin() + (long)pos, framed.begin() + (long)(pos + (size_t)flen[(size_t)k]));
        pos += (size_t)flen[(size_t)k];
    }
    return out;
}

// host arrays -> device, one chain of pages per array, the written pages back (mi355lz4_compress_pages; accel > 0:
// mi355lz4_compress_pages_fast at that acceleration; with hd, mi355lz4_compress_pages_fastdict against that prepared dictionary)
static std::vector<std::vector<Array>> pages_arrays(mi355lz4_ctx *ctx_, const char *who, int accel, const BlockConfig &cfg,
                                                    const std::vector<Array> &arrays, int pageSize, int maxPages, std::vector<int32_t> *consumed,
                                                    const mi355lz4_hcdict *hd = nullptr)
{
    if (cfg.blockChecksum) throw Error(std::string(who) + ": pages carry no block checksum");
    if (pageSize < 1 || maxPages < 1) throw Error(std::string(who) + ": pageSize and maxPages must be at least 1");
    const int meta = metaSize(cfg);
    const size_t n = arrays.size(), stride = (size_t)meta + (size_t)pageSize;
    std::vector<const uint8_t *> ptrs;
    std::vector<int32_t> lens;
    for (const Array &a : arrays) {
        if (a.size() > (size_t)MI355LZ4_MAX_INPUT_SIZE) throw Error(std::string(who) + ": array of " + std::to_string(a.size()) + " bytes");
        ptrs.push_back(a.data());
        lens.push_back((int32_t)a.size());
    }
    ptrs.push_back(nullptr);
    lens.push_back(0);
    std::vector<uint8_t> pages(n * (size_t)maxPages * stride + 1);
    std::vector<int32_t> srcLen(n * (size_t)maxPages + 1), compLen(n * (size_t)maxPages + 1), count(n + 1), cons(n + 1);
    const int rc = hd ? mi355lz4_compress_pages_fastdict(ctx_, hd, ptrs.data(), lens.data(), (int)n, pageSize, maxPages, accel, meta, pages.data(),
                                                         stride, srcLen.data(), compLen.data(), count.data(), cons.data())
                 : accel > 0 ? mi355lz4_compress_pages_fast(ctx_, ptrs.data(), lens.data(), (int)n, pageSize, maxPages, accel, meta, pages.data(),
                                                            stride, srcLen.data(), compLen.data(), count.data(), cons.data())
                             : mi355lz4_compress_pages(ctx_, ptrs.data(), lens.data(), (int)n, pageSize, maxPages, meta, pages.data(), stride,
                                                       srcLen.data(), compLen.data(), count.data(), cons.data());
    if (rc != MI355LZ4_OK)
        throw Error(std::string(who) + ": " + mi355lz4_last_error());
    std::vector<std::vector<Array>> out(n);
    for (size_t i = 0; i < n; i++)
        for (size_t k = 0; k < (size_t)count[i]; k++) {
            const size_t at = i * (size_t)maxPages + k;
            out[i].emplace_back(pages.begin() + (long)(at * stride), pages.begin() + (long)(at * stride + (size_t)meta + (size_t)compLen[at]));
        }
    if (consumed) consumed->assign(cons.begin(), cons.begin() + (long)n);
    return out;
}

std::vector<std::vector<Array>> Engine::compressPages(const BlockConfig &cfg, const std::vector<Array> &arrays, int pageSize, int maxPages,
                                                      std::vector<int32_t> *consumed)
{
    return pages_arrays(ctx_, "compressPages", 0, cfg, arrays, pageSize, maxPages, consumed);
}

// ... the pages by the engine's own encoder with an output budget (mi355lz4_compress_pages_fast)
std::vector<std::vector<Array>> Engine::compressPagesFast(const BlockConfig &cfg, const std::vector<Array> &arrays, int pageSize, int maxPages,
                                                          std::vector<int32_t> *consumed, int accel)
{
    return pages_arrays(ctx_, "compressPagesFast", accel < 1 ? 1 : accel, cfg, arrays, pageSize, maxPages, consumed);
}

// ... and with a prepared dictionary in front of every page (mi355lz4_compress_pages_fastdict)
std::vector<std::vector<Array>> Engine::compressPagesWithDictFast(const BlockConfig &cfg, const std::vector<Array> &arrays, const HcDict &hd,
                                                                  int pageSize, int maxPages, std::vector<int32_t> *consumed, int accel)
{
    return pages_arrays(ctx_, "compressPagesWithDictFast", accel < 1 ? 1 : accel, cfg, arrays, pageSize, maxPages, consumed, hd.handle());
}

std::vector<Array> Engine::decompressWithDict(const BlockConfig &cfg, const std::vector<Array> &blocks, const Array &dict)
{
    const int meta = metaSize(cfg);
    const BlockChecksumScope scope(ctx_, cfg.blockChecksum);
    Array framed;
    size_t cap = 16;
    for (const Array &a : blocks) {
        if (a.size() < (size_t)meta) throw Error("decompressWithDict: an array shorter than a block header");
        const int64_t u = (meta == 8) ? (int64_t)(int32_t)((uint32_t)a[4] | ((uint32_t)a[5] << 8) | ((uint32_t)a[6] << 16) |
                                                           ((uint32_t)a[7] << 24))
                                      : (int64_t)fixedUncompSize(cfg);
        if (u > 0) cap += (size_t)u;
        framed.insert(framed.end(), a.begin(), a.end());
    }
    const int n = (int)blocks.size();
    Array out(cap);
    std::vector<int32_t> blen((size_t)n + 1);
    size_t outLen = 0;
    int got = 0;
    if (mi355lz4_decompress_dict(ctx_, framed.data(), framed.size(), meta, fixedUncompSize(cfg), dict.empty() ? nullptr : dict.data(),
                                 (int)dict.size(), out.data(), cap, &outLen, blen.data(), n, &got) != MI355LZ4_OK)
        throw Error(std::string("decompressWithDict: ") + mi355lz4_last_error());
    std::vector<Array> res;
    size_t pos = 0;
    for (int k = 0; k < got; k++) {
        res.emplace_back(out.begin() + (long)pos, out.begin() + (long)(pos + (size_t)blen[(size_t)k]));
        pos += (size_t)blen[(size_t)k];
    }
    return res;
}

Frames::Frames(Engine &eng) : eng_(eng)
{
    if (mi355lz4_frames_create(eng.ctx(), &fr_) != MI355LZ4_OK) throw Error(std::string("streamly_lz4::Frames: ") + mi355lz4_last_error());
}
Frames::~Frames() { mi355lz4_frames_destroy(fr_); }
int Frames::inputs() const { return mi355lz4_frames_inputs(fr_); }
int Frames::blocks() const { return mi355lz4_frames_blocks(fr_); }
uint64_t Frames::total() const { return mi355lz4_frames_total(fr_); }
const int64_t *Frames::sizesDevice() const { return mi355lz4_frames_sizes(fr_); }
std::vector<int64_t> Frames::load(const uint8_t *buf, uint64_t bufLen, const uint64_t *inOff, const uint64_t *inLen, int nInputs,
                                  unsigned flags)
{
    if (mi355lz4_frames_load(eng_.ctx(), fr_, buf, bufLen, inOff, inLen, nInputs, flags) != MI355LZ4_OK)
        throw Error(std::string("Frames::load: ") + mi355lz4_last_error());
    std::vector<int64_t> sizes((size_t)nInputs);
    mi355lz4_frames_get_sizes(fr_, sizes.data());
    return sizes;
}
void Frames::decode(uint8_t *out, const uint64_t *outOff, int64_t *result)
{
    if (mi355lz4_frames_decode(eng_.ctx(), fr_, out, outOff, result) != MI355LZ4_OK)
        throw Error(std::string("Frames::decode: ") + mi355lz4_last_error());
}

FrameWriter::FrameWriter(Engine &eng) : eng_(eng)
{
    if (mi355lz4_cframes_create(eng.ctx(), &w_) != MI355LZ4_OK) throw Error(std::string("streamly_lz4::FrameWriter: ") + mi355lz4_last_error());
}
FrameWriter::~FrameWriter() { mi355lz4_cframes_destroy(w_); }
uint64_t FrameWriter::bound(uint64_t len, int blockSizeId, unsigned flags) { return mi355lz4_cframes_bound(len, blockSizeId, flags); }
void FrameWriter::reserve(int nInputs, uint64_t maxInputLen, uint64_t totalLen, int blockSizeId)
{
    if (mi355lz4_cframes_reserve(eng_.ctx(), w_, nInputs, maxInputLen, totalLen, blockSizeId) != MI355LZ4_OK)
        throw Error(std::string("FrameWriter::reserve: ") + mi355lz4_last_error());
}
void FrameWriter::compress(const uint8_t *src, uint64_t srcBufLen, const uint64_t *inOff, const uint64_t *inLen, int nInputs,
                           uint64_t maxInputLen, uint64_t totalLen, int blockSizeId, unsigned flags, int accel, uint8_t *dst,
                           const uint64_t *dstOff, const uint64_t *dstCap, int64_t *frameLen)
{
    if (mi355lz4_cframes_compress(eng_.ctx(), w_, src, srcBufLen, inOff, inLen, nInputs, maxInputLen, totalLen, blockSizeId, flags, accel,
                                  dst, dstOff, dstCap, frameLen) != MI355LZ4_OK)
        throw Error(std::string("FrameWriter::compress: ") + mi355lz4_last_error());
}

std::vector<Array> Engine::compressFrames(const std::vector<Array> &inputs, int blockSizeId, unsigned flags, int accel)
{
    const int n = (int)inputs.size();
    std::vector<const uint8_t *> ptrs;
    std::vector<size_t> lens;
    size_t cap = 0;
    for (const Array &a : inputs) {
        ptrs.push_back(a.data()); lens.push_back(a.size());
        cap += (size_t)mi355lz4_cframes_bound(a.size(), blockSizeId, flags);
    }
    ptrs.push_back(nullptr);
    lens.push_back(0);
    std::vector<int64_t> flen((size_t)n + 1);
    Array out(cap + 1);
    size_t outLen = 0;
    if (mi355lz4_compress_frames(ctx_, ptrs.data(), lens.data(), n, blockSizeId, flags, accel, out.data(), cap, &outLen, flen.data()) != MI355LZ4_OK)
        throw Error(std::string("compressFrames: ") + mi355lz4_last_error());
    std::vector<Array> res;
    size_t pos = 0;
    for (int k = 0; k < n; k++) {
        res.emplace_back(out.begin() + (long)pos, out.begin() + (long)(pos + (size_t)flen[(size_t)k]));
        pos += (size_t)flen[(size_t)k];
    }
    return res;
}

std::vector<Array> Engine::decompressFrames(const std::vector<Array> &inputs, unsigned flags, std::vector<int64_t> *result)
{
    const int n = (int)inputs.size();
    std::vector<const uint8_t *> ptrs;
    std::vector<size_t> lens;
    for (const Array &a : inputs) { ptrs.push_back(a.data()); lens.push_back(a.size()); }
    ptrs.push_back(nullptr);
    lens.push_back(0);
    std::vector<int64_t> res((size_t)n + 1);
    size_t outLen = 0;
    // one call that fails for its capacity sizes the buffer (the C ABI's own way), the second decodes
    int rc = mi355lz4_decompress_frames(ctx_, ptrs.data(), lens.data(), n, flags, nullptr, 0, &outLen, res.data());
    Array out(outLen);
    if (rc == MI355LZ4_E_CAPACITY)
        rc = mi355lz4_decompress_frames(ctx_, ptrs.data(), lens.data(), n, flags, out.data(), out.size(), &outLen, res.data());
    if (rc != MI355LZ4_OK && !(rc == MI355LZ4_E_BLOCK && result)) throw Error(std::string("decompressFrames: ") + mi355lz4_last_error());
    std::vector<Array> parts;
    size_t pos = 0;
    for (int k = 0; k < n; k++) {
        const size_t len = res[(size_t)k] > 0 ? (size_t)res[(size_t)k] : 0;
        parts.emplace_back(out.begin() + (long)pos, out.begin() + (long)(pos + len));
        pos += len;
    }
    if (result) result->assign(res.begin(), res.begin() + n);
    return parts;
}

DictSet::DictSet(Engine &eng, const std::vector<const HcDict *> &members)
{
    std::vector<const mi355lz4_hcdict *> h;
    for (const HcDict *m : members) h.push_back(m ? m->handle() : nullptr);
    if (mi355lz4_dictset_create(eng.ctx(), h.data(), (int)h.size(), &ds_) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::DictSet: ") + mi355lz4_last_error());
}
DictSet::~DictSet() { mi355lz4_dictset_destroy(ds_); }
int DictSet::count() const { return mi355lz4_dictset_count(ds_); }

std::vector<Array> Engine::compressWithDictsFast(const BlockConfig &cfg, const std::vector<Array> &arrays, const DictSet &ds,
                                                 const std::vector<int32_t> &dictIdx, int accel)
{
    if (dictIdx.size() != arrays.size()) throw Error("compressWithDictsFast: one dictionary index per array");
    const int meta = metaSize(cfg);
    std::vector<const uint8_t *> ptrs;
    std::vector<int32_t> lens, idx(dictIdx);
    size_t cap = 16;
    for (const Array &a : arrays) {
        if (a.size() > (size_t)maxBlockSize(cfg))                               // compressChunk, Internal/LZ4.hs:237-241
            throw Error("compressChunk: Source array length " + std::to_string(a.size()) +
                        " exceeds the maximum block size of " + std::to_string(maxBlockSize(cfg)));
        ptrs.push_back(a.data());
        lens.push_back((int32_t)a.size());
        cap += (size_t)mi355lz4_compress_bound((int)a.size()) + (size_t)meta + 4;
    }
    const int n = (int)lens.size();
    std::vector<uint8_t> framed(cap);
    std::vector<int32_t> flen((size_t)n + 1), status((size_t)n + 1);
    ptrs.push_back(nullptr);
    lens.push_back(0);
    idx.push_back(-1);
    size_t outLen = 0;
    if (mi355lz4_compress_fastdict_multi(ctx_, ds.handle(), idx.data(), ptrs.data(), lens.data(), n, accel, meta, framed.data(), cap,
                                         &outLen, flen.data(), status.data()) != MI355LZ4_OK)
        throw Error(std::string("compressWithDictsFast: ") + mi355lz4_last_error());
    std::vector<Array> out;
    size_t pos = 0;
    for (int k = 0; k < n; k++) {
        out.emplace_back(framed.begin() + (long)pos, framed.begin() + (long)(pos + (size_t)flen[(size_t)k]));
        pos += (size_t)flen[(size_t)k];
    }
    return out;
}

std::vector<Array> Engine::decompressWithDicts(const BlockConfig &cfg, const std::vector<Array> &blocks, const DictSet &ds,
                                               const std::vector<int32_t> &dictIdx)
{
    if (dictIdx.size() != blocks.size()) throw Error("decompressWithDicts: one dictionary index per block");
    const int meta = metaSize(cfg);
    const BlockChecksumScope scope(ctx_, cfg.blockChecksum);
    Array framed;
    size_t cap = 16;
    for (const Array &a : blocks) {
        if (a.size() < (size_t)meta) throw Error("decompressWithDicts: an array shorter than a block header");
        const int64_t u = (meta == 8) ? (int64_t)(int32_t)((uint32_t)a[4] | ((uint32_t)a[5] << 8) | ((uint32_t)a[6] << 16) |
                                                           ((uint32_t)a[7] << 24))
                                      : (int64_t)fixedUncompSize(cfg);
        if (u > 0) cap += (size_t)u;
        framed.insert(framed.end(), a.begin(), a.end());
    }
    const int n = (int)blocks.size();
    Array out(cap);
    std::vector<int32_t> blen((size_t)n + 1), idx(dictIdx);
    idx.push_back(-1);
    size_t outLen = 0;
    int got = 0;
    if (mi355lz4_decompress_dict_multi(ctx_, framed.data(), framed.size(), meta, fixedUncompSize(cfg), ds.handle(), idx.data(), out.data(),
                                       cap, &outLen, blen.data(), n, &got) != MI355LZ4_OK)
        throw Error(std::string("decompressWithDicts: ") + mi355lz4_last_error());
    std::vector<Array> res;
    size_t pos = 0;
    for (int k = 0; k < got; k++) {
        res.emplace_back(out.begin() + (long)pos, out.begin() + (long)(pos + (size_t)blen[(size_t)k]));
        pos += (size_t)blen[(size_t)k];
    }
    return res;
}

DecompressStreams::DecompressStreams(Engine &eng, int nSlots) : eng_(eng)
{
    if (mi355lz4_dstreams_create(eng.ctx(), nSlots, &ds_) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::DecompressStreams: ") + mi355lz4_last_error());
}
DecompressStreams::~DecompressStreams() { mi355lz4_dstreams_destroy(ds_); }
int DecompressStreams::count() const { return mi355lz4_dstreams_count(ds_); }
void DecompressStreams::reset()
{
    if (mi355lz4_dstreams_reset(eng_.ctx(), ds_, nullptr, 0) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::DecompressStreams::reset: ") + mi355lz4_last_error());
}
void DecompressStreams::reset(const std::vector<int32_t> &slots)
{
    if (slots.empty()) return;
    if (mi355lz4_dstreams_reset(eng_.ctx(), ds_, slots.data(), (int)slots.size()) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::DecompressStreams::reset: ") + mi355lz4_last_error());
}
void DecompressStreams::setDict(int slot, const uint8_t *dictDevice, int len)
{
    if (mi355lz4_dstreams_set_dict(eng_.ctx(), ds_, slot, dictDevice, len) != MI355LZ4_OK)
        throw Error(std::string("streamly_lz4::DecompressStreams::setDict: ") + mi355lz4_last_error());
}

std::vector<std::vector<Array>> Engine::decompressStreams(const BlockConfig &cfg, const std::vector<std::vector<Array>> &streams,
                                                          DecompressStreams &ds, const std::vector<int32_t> &slots)
{
    if (slots.size() != streams.size()) throw Error("decompressStreams: one slot per stream");
    const int meta = metaSize(cfg);
    const BlockChecksumScope scope(ctx_, cfg.blockChecksum);
    Array framed;
    std::vector<int32_t> first{0};
    size_t cap = 16;
    int n = 0;
    for (const auto &st : streams) {
        for (const Array &a : st) {
            if (a.size() < (size_t)meta) throw Error("decompressStreams: an array shorter than a block header");
            const int64_t u = (meta == 8) ? (int64_t)(int32_t)((uint32_t)a[4] | ((uint32_t)a[5] << 8) | ((uint32_t)a[6] << 16) |
                                                               ((uint32_t)a[7] << 24))
                                          : (int64_t)fixedUncompSize(cfg);
            if (u > 0) cap += (size_t)u;
            framed.insert(framed.end(), a.begin(), a.end());
            n++;
        }
        first.push_back((int32_t)n);
    }
    Array out(cap);
    std::vector<int32_t> blen((size_t)n + 1);
    std::vector<int32_t> slot(slots);
    slot.push_back(0);
    size_t outLen = 0;
    int got = 0;
    if (mi355lz4_decompress_dstreams(ctx_, ds.handle(), framed.data(), framed.size(), meta, fixedUncompSize(cfg), first.data(),
                                     slot.data(), (int)streams.size(), out.data(), cap, &outLen, blen.data(), n, &got) != MI355LZ4_OK)
        throw Error(std::string("decompressStreams: ") + mi355lz4_last_error());
    std::vector<std::vector<Array>> res(streams.size());
    size_t pos = 0;
    int k = 0;
    for (size_t s = 0; s < streams.size(); s++)
        for (size_t i = 0; i < streams[s].size(); i++, k++) {
            res[s].emplace_back(out.begin() + (long)pos, out.begin() + (long)(pos + (size_t)blen[(size_t)k]));
            pos += (size_t)blen[(size_t)k];
        }
    return res;
}

// ---------------------------------------------------------------------------
// compressChunksD (:353-394) + compressChunk (:226-281)
// ---------------------------------------------------------------------------
namespace {
class CompressStream : public ArrayStream {
public:
    CompressStream(BlockConfig cfg, int speed, StreamPtr in, Engine &eng)
        : cfg_(cfg), speed_(speed < 0 ? 0 : speed) /* speed = max speed0 0, :364 */, in_(std::move(in)), eng_(eng)
    {
        if (eng_.compressExact()) eng_.resetCompressStream();   // one stream per compressChunksD (:357), across the batches
    }

    bool next(Array &out) override
    {
        if (ready_.empty() && !done_) fill();
        if (ready_.empty()) return false;
        out = std::move(ready_.front());
        ready_.pop_front();
        return true;
    }

private:
    void fill()
    {
        std::vector<Array> batch;
        Array a;
        size_t bytes = 0;
        while (batch.size() < eng_.batchBlocks() && bytes < (size_t)1 << 30) {
            if (!in_->next(a)) { done_ = true; break; }
            if (a.size() >= ((size_t)2 << 30))                                   // :384-385
                throw Error("compressChunksD: Array element > 2 GB encountered");
            if (a.size() > (size_t)maxBlockSize(cfg_))                          // :237-241
                throw Error("compressChunk: Source array length " + std::to_string(a.size()) +
                            " exceeds the maximum block size of " + std::to_string(maxBlockSize(cfg_)));
            bytes += a.size();
            batch.push_back(std::move(a));
        }
        if (batch.empty()) return;
        const int n = (int)batch.size();
        const int meta = metaSize(cfg_);
        const int tr = trailerSize(cfg_);
        std::vector<const uint8_t *> ptrs((size_t)n);
        std::vector<int32_t> lens((size_t)n), flen((size_t)n), status((size_t)n);
        size_t cap = 0;
        for (int i = 0; i < n; i++) {
            ptrs[(size_t)i] = batch[(size_t)i].data();
            lens[(size_t)i] = (int32_t)batch[(size_t)i].size();
            cap += (size_t)mi355lz4_compress_bound(lens[(size_t)i]) + (size_t)meta + (size_t)tr;   // :244-251
        }
        Array framed(cap);
        size_t outLen = 0;
        BlockChecksumScope ck(eng_.ctx(), cfg_.blockChecksum);
        int r = mi355lz4_compress_batch(eng_.ctx(), ptrs.data(), lens.data(), n, speed_, meta, framed.data(), cap,
                                        &outLen, flen.data(), status.data());
        if (r != MI355LZ4_OK) {
            // status[] is only filled when the call got as far as the per-block results
            for (int i = 0; r == MI355LZ4_E_BLOCK && i < n; i++)
                if (status[(size_t)i] <= 0)                                     // :257-260
                    throw Error("compressChunk: c_compressFastContinue failed. uncompLenC: " +
                                std::to_string(lens[(size_t)i]) + "compLenC: " + std::to_string(status[(size_t)i]));
            throw Error(std::string("compressChunks: ") + mi355lz4_last_error());
        }
        size_t pos = 0;
        for (int i = 0; i < n; i++) {                                           // one Array per block, :261-268
            ready_.emplace_back(framed.begin() + (long)pos, framed.begin() + (long)(pos + (size_t)flen[(size_t)i]));
            pos += (size_t)flen[(size_t)i];
        }
    }

    BlockConfig cfg_;
    int speed_;
    StreamPtr in_;
    Engine &eng_;
    std::deque<Array> ready_;
    bool done_ = false;
};
} // namespace

StreamPtr compressChunks(const BlockConfig &cfg, int speed, StreamPtr in, Engine &eng)
{
    return StreamPtr(new CompressStream(cfg, speed, std::move(in), eng));
}

// ---------------------------------------------------------------------------
// resizeChunksD (:432-523)
// ---------------------------------------------------------------------------
namespace {
class ResizeStream : public ArrayStream {
public:
    ResizeStream(BlockConfig cfg, FrameConfig conf, StreamPtr in) : cfg_(cfg), conf_(conf), in_(std::move(in)) {}

    bool next(Array &out) override
    {
        const size_t meta = (size_t)metaSize(cfg_);
        for (;;) {
            switch (st_) {
            case St::Init: {                                                    // RInit, :488-496
                if (!in_->next(buf_)) {
                    if (conf_.hasEndMark) throw Error("resizeChunksD: No end mark found");   // :495
                    st_ = St::Done;
                    return false;
                }
                st_ = St::Process;
                break;
            }
            case St::Process: {                                                 // process, :459-484
                const size_t len = buf_.size();
                if (len < 4) { st_ = St::Accumulate; break; }                   // :461-462
                if (conf_.hasEndMark && le32(buf_.data()) == 0) { st_ = St::Footer; break; }   // :451-456,464-466
                if (len <= meta) { st_ = St::Accumulate; break; }               // :468-469
                const int32_t compressedSize = le32(buf_.data());               // :471-473 (compSizeOffset = 0)
                // a negative size would make `required` wrap; the reference would then mis-slice.
                if (compressedSize < 0) throw Error("resizeChunksD: negative compressed length in block header");
                const size_t required = (size_t)compressedSize + meta + (size_t)trailerSize(cfg_);   // :474 (+ the trailer)
                if (len == required) {                                          // :475-476
                    out = std::move(buf_);
                    buf_.clear();
                    st_ = St::Init;
                    return true;
                }
                if (len < required) { st_ = St::Accumulate; break; }            // :477-478
                out.assign(buf_.begin(), buf_.begin() + (long)required);        // :479-484
                buf_.erase(buf_.begin(), buf_.begin() + (long)required);
                st_ = St::Process;
                return true;
            }
            case St::Accumulate: {                                              // RAccumulate, :498-505
                Array more;
                if (!in_->next(more)) throw Error("resizeChunksD: Incomplete block");   // :505
                buf_.insert(buf_.end(), more.begin(), more.end());              // Array.splice, :502
                st_ = St::Process;
                break;
            }
            case St::Footer: {                                                  // RFooter, :506-522
                const size_t footer = conf_.hasEndMark ? 4 : 0;                 // :404-408
                if (buf_.size() < footer) {
                    Array more;
                    if (!in_->next(more)) throw Error("resizeChunksD: Incomplete footer");  // :517
                    buf_.insert(buf_.end(), more.begin(), more.end());
                    break;
                }
                // validateFooter always succeeds (:410-411); anything after the mark is ignored (:507)
                st_ = St::Done;
                return false;
            }
            case St::Done:
                return false;
            }
        }
    }

private:
    enum class St { Init, Process, Accumulate, Footer, Done };
    BlockConfig cfg_;
    FrameConfig conf_;
    StreamPtr in_;
    Array buf_;
    St st_ = St::Init;
};
} // namespace

StreamPtr resizeChunks(const BlockConfig &cfg, const FrameConfig &conf, StreamPtr in)
{
    return StreamPtr(new ResizeStream(cfg, conf, std::move(in)));
}

// ---------------------------------------------------------------------------
// decompressChunksRawD (:539-567) + decompressChunk (:291-336)
// ---------------------------------------------------------------------------
namespace {
class DecompressStream : public ArrayStream {
public:
    DecompressStream(BlockConfig cfg, StreamPtr in, Engine &eng) : cfg_(cfg), in_(std::move(in)), eng_(eng) {}

    bool next(Array &out) override
    {
        if (ready_.empty() && !done_) fill();
        if (ready_.empty()) {
            // a block that failed its checksum: the blocks in front of it have been delivered, now the error
            if (!pendingErr_.empty()) { std::string e; e.swap(pendingErr_); throw Error(e); }
            return false;
        }
        out = std::move(ready_.front());
        ready_.pop_front();
        return true;
    }

private:
    void fill()
    {
        const int meta = metaSize(cfg_);
        const int tr = trailerSize(cfg_);
        std::vector<Array> batch;
        Array a;
        size_t bytes = 0, outBytes = 0;
        while (batch.size() < eng_.batchBlocks() && bytes < (size_t)1 << 30 && outBytes < (size_t)2 << 30) {
            if (!in_->next(a)) { done_ = true; break; }
            // decompressChunk's header checks, :299-318
            if (a.size() < (size_t)meta) throw Error("decompressChunk: input array is shorter than the block header");
            if (a.size() < (size_t)(meta + tr)) throw Error("decompressChunk: input array is shorter than the block header and checksum");
            const int32_t compLen = le32(a.data());
            const int64_t arrDataLen = (int64_t)a.size() - meta - tr;
            const int64_t uncompLen = (meta == 8) ? (int64_t)le32(a.data() + 4) : (int64_t)fixedUncompSize(cfg_);
            if (compLen <= 0) throw Error("decompressChunk: compressed data length > 2GB");              // :309-310
            if ((int64_t)compLen < arrDataLen)                                                          // :311-315
                throw Error("decompressChunk: input array data length " + std::to_string(arrDataLen) +
                            " is less than the compressed data length specified in the header " + std::to_string(compLen));
            if ((int64_t)compLen > arrDataLen)   // the case the reference misses (it would read past the array)
                throw Error("decompressChunk: input array data length " + std::to_string(arrDataLen) +
                            " is shorter than the compressed data length specified in the header " + std::to_string(compLen));
            if (compLen > mi355lz4_compress_bound(MI355LZ4_MAX_INPUT_SIZE))                                 // :316-318
                throw Error("decompressChunk: compressed data length is more than the max limit: " +
                            std::to_string(mi355lz4_compress_bound(MI355LZ4_MAX_INPUT_SIZE)));
            if (uncompLen < 0) throw Error("decompressChunk: negative uncompressed length in block header");
            bytes += a.size();
            outBytes += (size_t)uncompLen;
            batch.push_back(std::move(a));
        }
        if (batch.empty()) return;
        int n = (int)batch.size();
        Array framed;
        framed.reserve(bytes);
        for (auto &b : batch) framed.insert(framed.end(), b.begin(), b.end());
        Array out(outBytes ? outBytes : 1);
        std::vector<int32_t> blockLen((size_t)n);
        size_t outLen = 0;
        int got = 0;
        BlockChecksumScope ck(eng_.ctx(), cfg_.blockChecksum);
        // The reference always decodes with stream (linked) semantics; prev_ is the array its
        // DecompressDo state keeps alive (:564).
        int r = mi355lz4_decompress_batch(eng_.ctx(), framed.data(), framed.size(), meta, fixedUncompSize(cfg_), 1,
                                          prev_.empty() ? nullptr : prev_.data(), (int)prev_.size(), out.data(),
                                          out.size(), &outLen, blockLen.data(), n, &got);
        if (r == MI355LZ4_E_BLOCK && cfg_.blockChecksum) {
            // In stream order: the blocks in front of the first failing one are delivered (decoded again, alone: the batch
            // call packs nothing when a block fails), then the error.  Only with block checksums, whose error is new.
            size_t pos = 0;
            int k = 0;
            while (k < got && blockLen[(size_t)k] >= 0) { pos += (size_t)meta + (size_t)le32(framed.data() + pos) + (size_t)tr; k++; }
            if (k < got) {
                const int32_t code = blockLen[(size_t)k];
                pendingErr_ = code == MI355LZ4_BLK_E_CHECKSUM
                    ? "decompressChunk: block checksum mismatch in block " + std::to_string(seen_ + (uint64_t)k) +
                      " (its data does not match its xxh32 trailer)"
                    : "decompressChunk: c_decompressSafeContinue failed in block " + std::to_string(seen_ + (uint64_t)k) +
                      "\ndecompLenC = " + std::to_string(code);
                done_ = true;
                if (k > 0) {
                    r = mi355lz4_decompress_batch(eng_.ctx(), framed.data(), pos, meta, fixedUncompSize(cfg_), 1,
                                                  prev_.empty() ? nullptr : prev_.data(), (int)prev_.size(), out.data(),
                                                  out.size(), &outLen, blockLen.data(), k, &got);
                    if (r != MI355LZ4_OK || got != k) throw Error(std::string("decompressChunks: ") + mi355lz4_last_error());
                }
                n = k;
                r = MI355LZ4_OK;
            }
        }
        if (r == MI355LZ4_E_BLOCK) {
            size_t pos = 0;
            for (int i = 0; i < got; i++) {
                const int32_t compLen = le32(framed.data() + pos);
                if (blockLen[(size_t)i] < 0)                                                             // :325-330
                    throw Error("decompressChunk: c_decompressSafeContinue failed. \narrDataLen = " +
                                std::to_string(compLen) + "\ncompLenC = " + std::to_string(compLen) +
                                "\nuncompLenC = " + std::to_string(meta == 8 ? le32(framed.data() + pos + 4) : fixedUncompSize(cfg_)) +
                                "\ndecompLenC = " + std::to_string(blockLen[(size_t)i]));
                pos += (size_t)meta + (size_t)compLen + (size_t)tr;
            }
        }
        if (r != MI355LZ4_OK) throw Error(std::string("decompressChunks: ") + mi355lz4_last_error());
        size_t pos = 0;
        for (int i = 0; i < n; i++) {                                           // one Array per block, :331-336
            const size_t len = (size_t)blockLen[(size_t)i];
            ready_.emplace_back(out.begin() + (long)pos, out.begin() + (long)(pos + len));
            if (len > 0) prev_ = ready_.back();                                 // cbits/lz4.c:2331,2353: only result > 0 moves the dictionary
            pos += len;
        }
        seen_ += (uint64_t)n;
    }

    BlockConfig cfg_;
    StreamPtr in_;
    Engine &eng_;
    std::deque<Array> ready_;
    Array prev_;
    bool done_ = false;
    uint64_t seen_ = 0;             // blocks of the stream in front of this batch
    std::string pendingErr_;
};
} // namespace

StreamPtr decompressChunksRaw(const BlockConfig &cfg, StreamPtr in, Engine &eng)
{
    return StreamPtr(new DecompressStream(cfg, std::move(in), eng));
}

StreamPtr decompressChunks(const BlockConfig &cfg, StreamPtr in, Engine &eng)                   // LZ4.hs:114-122
{
    return decompressChunksRaw(cfg, resizeChunks(cfg, defaultFrameConfig(), std::move(in)), eng);
}

// Result buffers of the batch form are recycled: a fresh 10 MiB allocation costs its page faults (0.3-0.6 ms, as much
// as the GPU call) every time; a buffer handed back by slz4_arrays_free / ArrayBatch's owner is kept for the next call.
namespace {
struct BufPool {
    std::mutex mu;
    std::vector<std::pair<size_t, uint8_t *>> free_;       // (capacity, buffer)
    uint8_t *get(size_t n, size_t &cap)
    {
        {
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = 0; i < free_.size(); i++)
                if (free_[i].first >= n && free_[i].first <= 2 * n + (1u << 20)) {
                    uint8_t *p = free_[i].second; cap = free_[i].first;
                    held -= cap;
                    free_.erase(free_.begin() + (long)i);
                    return p;
                }
        }
        cap = n;
        return new uint8_t[n];
    }
    // The pool holds at most four buffers and POOL_BYTES in all (round 3 kept up to 4 x 256 MiB for the life of the
    // process); slz4_trim() / trim() hands everything back.
    static constexpr size_t POOL_BYTES = (size_t)64 << 20;
    size_t held = 0;
    void put(uint8_t *p, size_t cap)
    {
        std::lock_guard<std::mutex> g(mu);
        if (free_.size() < 4 && held + cap <= POOL_BYTES) { free_.emplace_back(cap, p); held += cap; return; }
        delete[] p;
    }
    void trim()
    {
        std::lock_guard<std::mutex> g(mu);
        for (auto &f : free_) delete[] f.second;
        free_.clear();
        held = 0;
    }
};
BufPool &buf_pool() { static BufPool *p = new BufPool(); return *p; }
} // namespace
void ArrayBatch::release() { if (buf) { buf_pool().put(buf, cap); buf = nullptr; cap = 0; } }
void trimBuffers() { buf_pool().trim(); }

// decompressChunks over arrays that already lie back to back (streamly_lz4.hpp): when the bytes are a well-formed
// run of whole blocks that all decode, one index walk and one GPU call do what resizeChunksD + decompressChunksRawD do
// array by array.  Anything else -- a trailing partial block, an end mark, a block the decoder rejects -- goes through
// the combinators themselves, which is what yields the reference's error for it.
ArrayBatch decompressChunksBatch(const BlockConfig &cfg, const FrameConfig &conf, const uint8_t *data,
                                 const uint64_t *lens, size_t n, Engine &eng)
{
    size_t total = 0;
    for (size_t i = 0; i < n; i++) total += (size_t)lens[i];
    ArrayBatch res;
    const int meta = metaSize(cfg);
    const size_t tr = (size_t)trailerSize(cfg);
    if (!conf.hasEndMark && total > 0 && total < ((size_t)1 << 31)) {
        // how many whole blocks? (a header walk: compLen <= 0, or a block that runs past the end, ends the fast path)
        size_t nbk = 0, p = 0;
        bool whole = true;
        while (p < total) {
            if (total - p < (size_t)meta) { whole = false; break; }
            const int32_t compLen = le32(data + p);
            if (compLen <= 0 || (size_t)compLen + tr > total - p - (size_t)meta) { whole = false; break; }
            p += (size_t)meta + (size_t)compLen + tr;
            nbk++;
        }
        if (whole && nbk > 0 && nbk < ((size_t)1 << 24)) {
            std::vector<uint64_t> boff(nbk + 1);
            std::vector<int32_t> ulen(nbk + 1), blen(nbk + 1);
            int nb = 0;
            if (mi355lz4_index_host_ex(data, total, meta, fixedUncompSize(cfg), cfg.blockChecksum, boff.data(), ulen.data(),
                                       (int)nbk, &nb) ==
                    MI355LZ4_OK && (size_t)nb == nbk) {
                size_t cap = 0;
                bool sane = true;
                for (int i = 0; i < nb; i++) { if (ulen[(size_t)i] < 0) sane = false; else cap += (size_t)ulen[(size_t)i]; }
                if (sane && cap < ((size_t)1 << 32)) {
                    res.buf = buf_pool().get(cap + 16, res.cap);
                    size_t outLen = 0;
                    int got = 0;
                    BlockChecksumScope ck(eng.ctx(), cfg.blockChecksum);
                    const int r = mi355lz4_decompress_batch(eng.ctx(), data, total, meta, fixedUncompSize(cfg), 1, nullptr, 0,
                                                            res.buf, cap + 16, &outLen, blen.data(), nb, &got);
                    if (r == MI355LZ4_OK && got == nb) {
                        res.off.resize((size_t)nb + 1);
                        size_t pos = 0;
                        for (int i = 0; i < nb; i++) { res.off[(size_t)i] = pos; pos += (size_t)blen[(size_t)i]; }
                        res.off[(size_t)nb] = pos;
                        return res;
                    }
                    // A block the decoder rejected: the arrays are decoded a second time below, by the combinators, because
                    // that is what raises the reference's error at the reference's block (the batch call only says that some
                    // block failed).  The double decode is paid on the error path only.
                    res.release();
                }
            }
        }
    }
    // the general path: the combinators, array by array
    std::vector<Array> v;
    v.reserve(n);
    size_t pos = 0;
    for (size_t i = 0; i < n; i++) { v.emplace_back(data + pos, data + pos + lens[i]); pos += (size_t)lens[i]; }
    StreamPtr s = decompressChunksRaw(cfg, resizeChunks(cfg, conf, fromList(std::move(v))), eng);
    std::vector<Array> outv = toList(*s);
    size_t outTotal = 0;
    for (const Array &a : outv) outTotal += a.size();
    res.buf = buf_pool().get(outTotal + 1, res.cap);
    res.off.resize(outv.size() + 1);
    pos = 0;
    for (size_t i = 0; i < outv.size(); i++) {
        res.off[i] = pos;
        if (!outv[i].empty()) memcpy(res.buf + pos, outv[i].data(), outv[i].size());
        pos += outv[i].size();
    }
    res.off[outv.size()] = pos;
    return res;
}

// ---------------------------------------------------------------------------
// simpleFrameParserD (:590-651) and decompressChunksWithD (:569-577)
// ---------------------------------------------------------------------------
namespace {
// Puts an already-pulled array back in front of a stream.
class PrependStream : public ArrayStream {
public:
    PrependStream(Array first, StreamPtr rest) : first_(std::move(first)), rest_(std::move(rest)), hasFirst_(!first_.empty()) {}
    bool next(Array &out) override
    {
        if (hasFirst_) { out = std::move(first_); hasFirst_ = false; return true; }
        return rest_->next(out);
    }
private:
    Array first_;
    StreamPtr rest_;
    bool hasFirst_;
};
} // namespace

std::pair<std::pair<BlockConfig, FrameConfig>, StreamPtr> simpleFrameParser(StreamPtr in)
{
    // gather the 7 header bytes: magic(4) FLG(1) BD(1) HC(1)
    Array head, a;
    while (head.size() < 7) {
        if (!in->next(a)) throw Error("simpleFrameParserD: unexpected end of input in frame header");
        head.insert(head.end(), a.begin(), a.end());
    }
    const long magic = (long)head[0] | ((long)head[1] << 8) | ((long)head[2] << 16) | ((long)head[3] << 24);
    if (magic != 407708164L)                                                    // :607-618
        throw Error("The parsed magic " + std::to_string(magic) + " does not match 407708164");
    const uint8_t flg = head[4];                                                // :620-642
    const bool isVersion01 = !(flg & 0x80) && (flg & 0x40);
    if (!isVersion01) throw Error("Version is not 01");
    if (flg & 0x20) throw Error("Block independence is not yet supported");
    if (flg & 0x10) throw Error("Block checksum is not yet supported");
    if (flg & 0x08) throw Error("Content size is not yet supported");
    if (flg & 0x04) throw Error("Content checksum is not yet supported");
    if (flg & 0x01) throw Error("Dict is not yet supported");
    BlockConfig cfg;
    switch (head[5] >> 4) {                                                     // :644-651
    case 4: cfg.blockSize = BlockSize::BlockMax64KB; break;
    case 5: cfg.blockSize = BlockSize::BlockMax256KB; break;
    case 6: cfg.blockSize = BlockSize::BlockMax1MB; break;
    case 7: cfg.blockSize = BlockSize::BlockMax4MB; break;
    default: throw Error("parseBD: Unknown block max size");
    }
    // head[6] is the header checksum: read, not verified (:605)
    FrameConfig fc;
    fc.hasEndMark = true;                                                       // :598-600
    Array rest(head.begin() + 7, head.end());
    return {{cfg, fc}, StreamPtr(new PrependStream(std::move(rest), std::move(in)))};
}

StreamPtr decompressChunksWith(StreamPtr in, Engine &eng)                       // :569-577
{
    auto parsed = simpleFrameParser(std::move(in));
    const BlockConfig cfg = parsed.first.first;
    const FrameConfig conf = parsed.first.second;
    return decompressChunksRaw(cfg, resizeChunks(cfg, conf, std::move(parsed.second)), eng);
}

} // namespace streamly_lz4

// ===========================================================================
// C surface over the combinators (tests / other-language bindings)
// ===========================================================================
using namespace streamly_lz4;

struct slz4_arrays { std::vector<Array> v; ArrayBatch b; bool flat = false; };
struct slz4_engine { Engine *e; };

static thread_local std::string g_slz4_err;

// kind: the BlockSize (0..4), plus SLZ4_BLOCK_CHECKSUM for setBlockChecksum True
#define SLZ4_BLOCK_CHECKSUM 0x100
static BlockConfig cfg_from_kind(int kind)
{
    BlockConfig c;
    c.blockChecksum = (kind & SLZ4_BLOCK_CHECKSUM) != 0;
    switch (kind & ~SLZ4_BLOCK_CHECKSUM) {
    case 0: c.blockSize = BlockSize::BlockHasSize; break;
    case 1: c.blockSize = BlockSize::BlockMax64KB; break;
    case 2: c.blockSize = BlockSize::BlockMax256KB; break;
    case 3: c.blockSize = BlockSize::BlockMax1MB; break;
    case 4: c.blockSize = BlockSize::BlockMax4MB; break;
    default: throw Error("unknown BlockSize kind");
    }
    return c;
}

static StreamPtr list_from_c(const uint8_t *data, const uint64_t *lens, size_t n)
{
    std::vector<Array> v;
    v.reserve(n);
    size_t pos = 0;
    for (size_t i = 0; i < n; i++) {
        v.emplace_back(data + pos, data + pos + lens[i]);
        pos += lens[i];
    }
    return fromList(std::move(v));
}

template <typename F>
static int guarded(slz4_arrays **out, F f)
{
    try {
        StreamPtr s = f();
        slz4_arrays *r = new slz4_arrays();
        r->v = toList(*s);
        *out = r;
        return 0;
    } catch (const std::exception &e) {
        g_slz4_err = e.what();
        *out = nullptr;
        return -1;
    }
}

extern "C" {

const char *slz4_last_error(void) { return g_slz4_err.c_str(); }

int slz4_engine_create(slz4_engine **out, int device, size_t batchBlocks)
{
    try {
        slz4_engine *h = new slz4_engine();
        h->e = new Engine(device, batchBlocks);
        *out = h;
        return 0;
    } catch (const std::exception &e) {
        g_slz4_err = e.what();
        *out = nullptr;
        return -1;
    }
}
void slz4_engine_destroy(slz4_engine *h) { if (h) { delete h->e; delete h; } }
void slz4_engine_set_batch(slz4_engine *h, size_t n) { if (h) h->e->setBatchBlocks(n); }
void slz4_engine_set_linked_compress(slz4_engine *h, int on) { if (h) h->e->setLinkedCompress(on != 0); }
mi355lz4_ctx *slz4_engine_ctx(slz4_engine *h) { return h ? h->e->ctx() : nullptr; }

size_t slz4_arrays_count(const slz4_arrays *a) { return a ? (a->flat ? a->b.count() : a->v.size()) : 0; }
size_t slz4_arrays_len(const slz4_arrays *a, size_t i) { return a->flat ? a->b.off[i + 1] - a->b.off[i] : a->v[i].size(); }
const uint8_t *slz4_arrays_data(const slz4_arrays *a, size_t i) { return a->flat ? a->b.buf + a->b.off[i] : a->v[i].data(); }
void slz4_arrays_free(slz4_arrays *a) { delete a; }
// result buffers kept for reuse (<= 64 MiB in all) go back to the allocator
void slz4_trim(void) { streamly_lz4::trimBuffers(); }
// flat results (the batch forms): the shared buffer and the n + 1 offsets; returns 0 when `a` is not flat
int slz4_arrays_flat(const slz4_arrays *a, const uint8_t **base, const size_t **offsets)
{
    if (!a || !a->flat) return 0;
    *base = a->b.buf;
    *offsets = a->b.off.data();
    return 1;
}

int slz4_compress_chunks(slz4_engine *h, int blockSizeKind, int speed, const uint8_t *data, const uint64_t *lens,
                         size_t n, slz4_arrays **out)
{
    return guarded(out, [&] { return compressChunks(cfg_from_kind(blockSizeKind), speed, list_from_c(data, lens, n), *h->e); });
}

int slz4_resize_chunks(int blockSizeKind, int hasEndMark, const uint8_t *data, const uint64_t *lens, size_t n,
                       slz4_arrays **out)
{
    return guarded(out, [&] {
        FrameConfig fc; fc.hasEndMark = hasEndMark != 0;
        return resizeChunks(cfg_from_kind(blockSizeKind), fc, list_from_c(data, lens, n));
    });
}

int slz4_decompress_chunks_raw(slz4_engine *h, int blockSizeKind, const uint8_t *data, const uint64_t *lens, size_t n,
                               slz4_arrays **out)
{
    return guarded(out, [&] { return decompressChunksRaw(cfg_from_kind(blockSizeKind), list_from_c(data, lens, n), *h->e); });
}

int slz4_decompress_chunks(slz4_engine *h, int blockSizeKind, int hasEndMark, const uint8_t *data, const uint64_t *lens,
                           size_t n, slz4_arrays **out)
{
    try {
        BlockConfig cfg = cfg_from_kind(blockSizeKind);
        FrameConfig fc; fc.hasEndMark = hasEndMark != 0;
        slz4_arrays *r = new slz4_arrays();
        try { r->b = decompressChunksBatch(cfg, fc, data, lens, n, *h->e); } catch (...) { delete r; throw; }
        r->flat = true;
        *out = r;
        return 0;
    } catch (const std::exception &e) {
        g_slz4_err = e.what();
        *out = nullptr;
        return -1;
    }
}

// decompressChunks array at a time, as a stream consumer sees it: *out always holds the arrays delivered before the
// stream raised (all of them when it returns 0); on -1 slz4_last_error() is the error.
int slz4_decompress_chunks_stream(slz4_engine *h, int blockSizeKind, int hasEndMark, const uint8_t *data, const uint64_t *lens,
                                  size_t n, slz4_arrays **out)
{
    slz4_arrays *r = new slz4_arrays();
    *out = r;
    try {
        FrameConfig fc; fc.hasEndMark = hasEndMark != 0;
        const BlockConfig cfg = cfg_from_kind(blockSizeKind);
        StreamPtr s = decompressChunksRaw(cfg, resizeChunks(cfg, fc, list_from_c(data, lens, n)), *h->e);
        Array a;
        while (s->next(a)) r->v.push_back(std::move(a));
        return 0;
    } catch (const std::exception &e) {
        g_slz4_err = e.what();
        return -1;
    }
}

int slz4_decompress_chunks_with(slz4_engine *h, const uint8_t *data, const uint64_t *lens, size_t n, slz4_arrays **out)
{
    return guarded(out, [&] { return decompressChunksWith(list_from_c(data, lens, n), *h->e); });
}

// frame-header parser alone: returns BlockSize kind (1..4) or -1
int slz4_simple_frame_parser(const uint8_t *data, const uint64_t *lens, size_t n, int *hasEndMark, slz4_arrays **rest)
{
    int kind = -1;
    int r = guarded(rest, [&] {
        auto parsed = simpleFrameParser(list_from_c(data, lens, n));
        kind = (int)parsed.first.first.blockSize;
        if (hasEndMark) *hasEndMark = parsed.first.second.hasEndMark ? 1 : 0;
        return std::move(parsed.second);
    });
    return r == 0 ? kind : -1;
}

// ---- standard LZ4 frames (csrc/lz4_frame.cpp) ----
uint32_t slz4_xxh32(const uint8_t *data, size_t len, uint32_t seed) { return xxh32(data, len, seed); }

// flags: bit 0 block checksums, bit 1 content checksum, bit 2 content size, bit 3 linked blocks
int slz4_lz4frame_compress(slz4_engine *h, int blockSizeKind, int flags, int speed, const uint8_t *data, size_t len,
                           slz4_arrays **out)
{
    return guarded(out, [&] {
        Lz4FrameOptions o;
        o.blockMax = cfg_from_kind(blockSizeKind).blockSize;
        o.blockChecksum = flags & 1; o.contentChecksum = flags & 2; o.contentSize = flags & 4; o.linkedBlocks = flags & 8;
        std::vector<Array> v;
        v.push_back(lz4FrameCompress(Array(data, data + len), speed, *h->e, o));
        return fromList(std::move(v));
    });
}

int slz4_lz4frame_decompress(slz4_engine *h, const uint8_t *data, size_t len, slz4_arrays **out)
{
    return guarded(out, [&] {
        std::vector<Array> v;
        v.push_back(lz4FrameDecompress(Array(data, data + len), *h->e));
        return fromList(std::move(v));
    });
}

} // extern "C"
