// kernels.h -- launch interface between the host layers (api.cpp, host_batch.cpp, legacy.cpp, host_stream.cpp, multi_device.cpp)
// and the kernels (kernels.hip and its family files, kernels/*.inc).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

// per-block header rejection codes (mirrors MI355LZ4_BLK_E_* in include/mi355lz4.h)
#define BLK_E_COMPLEN   (-0x7F000001)
#define BLK_E_TRUNCATED (-0x7F000002)
#define BLK_E_UNCOMPLEN (-0x7F000003)
#define BLK_E_CHECKSUM  (-0x7F000004)
#define BLK_E_SIZE_UNKNOWN (-0x7F000005)
// LZ4_compressBound(LZ4_MAX_INPUT_SIZE): reference lz4_MAX_OUTPUT_SIZE, Internal/LZ4.hs:145-147
#define MAX_COMP_LEN 2122219150

struct DecodeArgs {
    const uint8_t *framed;
    uint64_t framedLen;
    const uint64_t *blockOff;
    int nBlocks;
    int headerKind;
    int fixedUncomp;
    int linked;
    uint8_t *out;
    const uint64_t *outOff;
    const int32_t *outCap;   // may be null
    int32_t *result;
    const uint8_t *dict0;    // linked only: dictionary in force before block 0 (may be null)
    uint32_t dict0Len;
    const int32_t *streamFirst;   // linked only: stream s = blocks [streamFirst[s], streamFirst[s+1]); null = one stream
    int nStreams;
    int lookBack;                 // linked, one stream: blocks of the SAME stream that precede block 0 in result[] /
                                  // outOff[] (already final); lets a long stream be decoded range by range
    // Below, the fields one decode path alone arms are grouped by that path (a group is reset with `a.tol = {}`); what several
    // paths read stays flat.  The groups sit where their fields always sat: the layout of the kernel argument is part of the build.
    // deferred-copy decode of one long linked stream (linked_replay.hpp; kernels/linked_tolerant.inc, read by the pointer passes
    // too): per-block state of the tolerant pass and the pool its deferred lists live in; all null when the pool is not available
    struct {
        void *pool;               // TolEntry[regions][TOL_LIST_CAP]
        int regions;
        int per;                  // list regions per block of a tolerant launch: block segFirst + i owns regions [i * per, (i + 1) * per)
        uint32_t *counter;        // regions handed out so far
        int32_t *region;          // per block: region index, or -1 (no list: serial path)
        int32_t *count;           // per block: entries appended (may exceed the capacity: overflow)
        int32_t *size;            // per block: result of the tolerant decode
    } tol;
    // one long linked stream, data-parallel second pass (linked_ptr.hpp)
    uint32_t *linkStat;           // filled by the standalone pass: {blocks with a codec error, first, last}
    int segFirst, segEnd;         // blocks the second-pass kernels cover in this launch
    struct {                      // the pointer passes (kernels/linked_ptr.inc)
        uint32_t *buf;            // source pointers of the segment's bytes
        uint64_t cap;             // ... capacity in pointers
        void *ctl;                // PtrCtl
        uint32_t *bad;            // per stream (one entry without streamFirst): left to the serial walk
    } ptr;
    int asyncGate;                // second-pass kernels return at once when linkStat[0] == 0 (asynchronous linked decode)
    int onlyBlk;                  // >= 0: the fetch covers this block alone (mi355lz4_decompress_linked_end_last); -1: all
    // run starts of a linked stream's dependent blocks (k_run_starts -> k_decode_fixup_runs, kernels/linked_walk.inc): list[0] = count,
    // list[1..] = first block of each run, at most cap of them; null: the launch covers one run that starts at segFirst
    struct {
        int32_t *list;
        int cap;
    } runs;
    // long linked streams, run-in decode (kernels/runin.inc, k_runin_*): pieces of `piece` consecutive blocks of [segFirst, segEnd)
    struct {
        uint8_t *ring;            // scratch: two blocks per piece (piece p at ring + p * 2 * stride)
        uint64_t stride;          // >= the largest block capacity
        const uint8_t *zeroPage;  // 64 KiB of 0x00: the stand-in for the dictionary of the block a run-in starts at.  The big linked
                                  // blocks (cu, below) read it too, for their first pass: that path sets and clears it beside its own group
        int piece;                // blocks per piece
        int in;                   // blocks a piece decodes in front of its own (<= 64)
        int spin;                 // k_runin_fix: how many times a piece polls for the piece in front of it before it leaves itself to the next round
        int round;                // k_runin_fix: the round this launch is
        int32_t *res;             // per block of the segment: its result (result[] is written when everything is final)
        int32_t *info;            // per piece {block the run-in's dictionary came from | -1 | -2 exact, its length, its ring slot, -}
        uint32_t *dirty;          // per piece: the round in which it is to be redone, 0xffffffff = none
        uint32_t *ctl;            // [0] pieces marked for the next round, [1] give the call up (1: a block failed, 2: a chain of dirty pieces)
    } run;
    // experiment builds only (MI355LZ4_EXPERIMENTS; decode_par.hpp, LIST; kernels/decode_tok.inc): block blk's token list lives at list +
    // blockOff[blk] / 2 (a sequence is at least three compressed bytes), cnt[blk] entries; both null without the list pass
    struct {
        uint8_t *list;
        int32_t *cnt;
    } tok;
    // diagnostics of the workgroup-per-block decoder (mi355lz4_debug_cu): 16 words per block, null = off
    uint32_t *cuDbg;
    int cuBail;                 // workgroup-per-block decoder: leave blocks that do not suit it (hardly compressible; long literal runs) to the lane-parallel one at once (decoder variant 0; variant 4 keeps them)
    // big linked blocks by the workgroup-per-block decoder (launch_cu_linked, kernels/decode_par_cu.inc): every dependent block decoded with
    // a guess of its dictionary -- zeros (run.zeroPage) in pass 1, from pass 2 on a snapshot of the last 64 KiB its predecessor decoded to in
    // the pass before -- until no snapshot changes any more
    struct {
        uint8_t *snap;          // [nBlocks][65536]
        uint32_t *flags;        // [0] snapshots that changed in the last launch_cu_tails, [1] blocks the form cannot take, [2 + k] block k's snapshot changed
        int32_t *res;           // [nBlocks] results of the passes (published by the caller when the snapshots have settled)
        int pass;
    } cu;
    // block checksums (mi355lz4_set_block_checksum): every block's data is followed by a 4-byte xxh32 trailer, and
    // ckFail[blk] != 0 says k_xxh32_verify found that they do not match; null = no trailers (read_block_header)
    const int32_t *ckFail = nullptr;
    // partial decode (mi355lz4_decompress_partial_device): target[blk] = how many bytes of block blk are wanted; the block is
    // decoded as LZ4_decompress_safe_partial does with min(target, capacity) as its output end.  null = full decode (every other call)
    const int32_t *target = nullptr;
};

struct EncodeArgs {
    const uint8_t *src;
    const uint64_t *srcOff;  // may be null -> blk * blockStride
    const int32_t *srcLen;   // may be null -> uniformLen
    uint64_t blockStride;
    int uniformLen;
    int nBlocks;
    int accel;
    int headerKind;
    uint8_t *slots;
    size_t slotStride;
    int32_t *framedLen;
    unsigned long long *stats;   // diagnostics only (ENC_STATS builds); may be null
    int linked;                  // the blocks are consecutive blocks of ONE stream: block i-1 is block i's dictionary
    int lookBack;                // linked: blocks of the same stream that precede block 0 in srcOff[] / srcLen[]
};

// reference-exact compression (encode_exact.hpp, mi355lz4_set_compress_exact): one block of the stream as the host
// computed it from the lengths -- the state LZ4_compress_fast_continue reaches before it calls the encoder
// (cbits/lz4.c:1565-1627)
struct ExactBlock {
    uint32_t start;      // currentOffset after the renorm (startIndex)
    uint32_t dictSize;   // after the renorm clamp and the reset of dictionaries under 4 bytes
    uint32_t delta;      // LZ4_renormDictT before this block: entries < delta -> 0, the others -= delta (0: none)
    int32_t n;           // the array's length
    int32_t dictSmall;   // cbits/lz4.c:1627
    int32_t pad;
};
#define EXACT_TABLE 4096     // LZ4_HASHLOG 12, byU32

// One array of n bytes through LZ4_compress_fast_continue's statements around the encoder (cbits/lz4.c:1565-1634), from the
// scalars and the length alone: the block's state, and cur (currentOffset) and dictSize advanced behind it.  The host plans the
// single stream with it (api.cpp, exact_encode); k_exact_streams and k_exact_dict run it per wave.  Whoever holds the table
// applies the renorm that a non-zero delta asks for.
__host__ __device__ inline ExactBlock exact_step(uint32_t &cur, uint32_t &dictSize, uint32_t n)
{
    ExactBlock m;
    m.delta = 0;
    if (cur + n > 0x80000000u) {                                        // LZ4_renormDictT, :1545-1562
        m.delta = cur - 65536u;
        cur = 65536u;
        if (dictSize > 65536u) dictSize = 65536u;
    }
    if (dictSize - 1u < 4u - 1u) dictSize = 0;                          // :1581-1587
    m.start = cur; m.dictSize = dictSize; m.n = (int32_t)n; m.pad = 0;
    m.dictSmall = (dictSize < 65536u && dictSize < cur) ? 1 : 0;        // :1627
    cur += n;                                                           // :1633-1634
    dictSize = n;
    return m;
}

struct ExactArgs {
    EncodeArgs e;                // blocks, slots, headers, framedLen, accel (clamped); e.linked is not used
    const ExactBlock *meta;      // nBlocks + 1 entries (the last: the state after the call)
    const uint8_t *dict0;        // the dictionary in force before block 0: dict0Len bytes (the previous array's last ones)
    int dict0Len;
    uint32_t *state;             // the stream's table before the call (k_exact_chain reads), after it (k_exact_finish writes)
    uint8_t *dictSave;           // k_exact_finish: the last array's last min(n, 65536) bytes (may be dict0)
    uint32_t *assumed;           // nPieces tables: what piece p assumed at its first block (canonical)
    uint32_t *finalT;            // nPieces tables: piece p's table after its last block (canonical)
    int32_t *eq;                 // k_exact_verify: eq[p] = finalT[p-1] == assumed[p]
    int piece;                   // P: blocks per piece
    int runin;                   // R: blocks a piece starts early (from a zeroed table)
    int nPieces;
};

// many reference-exact streams in one call (mi355lz4_compress_streams_device; kernels/encode.inc, k_exact_streams).  One slot of a
// mi355lz4_cstreams is the device form of LZ4_stream_t: the table, the previous array's last 64 KiB and the scalars.
#define CSTREAM_SCALAR_OFF ((size_t)EXACT_TABLE * 4)              // uint32 {currentOffset, dictSize, saved bytes, -}: zeroed with the table
#define CSTREAM_DICT_OFF   (CSTREAM_SCALAR_OFF + 64)              // the saved dictionary bytes
#define CSTREAM_SLOT_BYTES (CSTREAM_DICT_OFF + 65536)             // 81984: about 80 KiB a slot

struct ExactStreamsArgs {
    EncodeArgs e;                // blocks, slots, headers, framedLen, accel (clamped); e.uniformLen bounds every length
    const int32_t *work;         // per wave of the launch {first block, end block, slot of the set}
    uint8_t *state;              // the set's slots, CSTREAM_SLOT_BYTES each
};

// a batch against one loaded slot (mi355lz4_compress_dict_device; kernels/encode.inc, k_exact_dict): every block from a copy of
// the slot's state, the slot itself read-only
struct ExactDictArgs {
    EncodeArgs e;                // blocks, slots, headers, framedLen, accel (clamped); e.uniformLen bounds every length
    const uint8_t *state;        // the one slot, CSTREAM_SLOT_BYTES
};

// fixed-size output pages (mi355lz4_compress_pages_device; encode_fill.hpp; kernels/encode.inc, k_exact_pages): input i is cut into
// pages of pageSize[i] compressed bytes, page (i, k) at pages + (i * maxPages + k) * pageStride, each LZ4_compress_destSize's
struct PagesArgs {
    const uint8_t *src;
    const uint64_t *srcOff;
    const int32_t *srcLen;
    int nInputs;
    const int32_t *pageSize;     // per input: the reference's targetDstSize (the block's bytes, without the header)
    int maxPages;
    int headerKind;              // 0, 4 or 8
    uint8_t *pages;
    size_t pageStride;
    int32_t *pageSrcLen;         // [nInputs * maxPages]: what the page consumed
    int32_t *pageCompLen;        // [nInputs * maxPages]: the reference's return value
    int32_t *nPages;             // [nInputs]
    int32_t *consumed;           // [nInputs]
};
#define PAGES_MAX_INPUT 0x7E000000   // LZ4_MAX_INPUT_SIZE (MI355LZ4_MAX_INPUT_SIZE in include/mi355lz4.h)
// the same pages from the wave encoder with an output budget (mi355lz4_compress_pages_fast_device; kernels/encode.inc, k_pages_fast):
// pageCompLen is the page's length, pageSize[i] its budget
struct PagesFastArgs {
    PagesArgs p;
    int accel;                   // clamped to 1..65537
};

// a prepared high-compression dictionary (mi355lz4_hcdict; kernels/encode.inc, k_hcdict_build): the image of encode_hc.hpp's chain[]
// and head[] after the inserts of the kept bytes' positions [0, keep - 3), the count, and the object's own copy of the bytes
#define HCDICT_CHAIN_BYTES ((size_t)65536 * 2)
#define HCDICT_HEAD_ENTRIES 6144                                  // HC_HEAD (encode_hc.hpp; checked where the kernels are compiled)
#define HCDICT_TABLE_BYTES (HCDICT_CHAIN_BYTES + (size_t)HCDICT_HEAD_ENTRIES * 4)    // 155648: chain, then head, as HcLds starts
#define HCDICT_KEEP_OFF    HCDICT_TABLE_BYTES                     // uint32 keep = min(len, 65536) (the rest of the 64 bytes is unused)
#define HCDICT_DICT_OFF    (HCDICT_KEEP_OFF + 64)                 // the kept bytes, the first one first
#define HCDICT_IMAGE_BYTES (HCDICT_DICT_OFF + 65536)              // 221248: about 216 KiB an object
#define HCDICT_MAX_BLOCK   (4 << 20)                              // the largest block of a mi355lz4_compress_hcdict_device call

// a batch against one prepared dictionary (mi355lz4_compress_hcdict_device; kernels/encode.inc, k_encode_hc_dict): workgroup w
// lays the kept bytes and, behind them, one block at a time into its window at stage + w * stageStride -- the dictionary ends
// and the block starts at byte 65536 of the window -- so that encode_block_hc sees what a linked call sees
struct HcDictArgs {
    EncodeArgs e;                // blocks, slots, headers, framedLen; e.uniformLen bounds every length; accel, linked, lookBack unused
    const uint8_t *image;        // HCDICT_IMAGE_BYTES, read-only
    uint8_t *stage;              // encode_hc_dict_grid(nBlocks) windows
    size_t stageStride;          // >= 65536 + e.uniformLen
};

// the wave encoder's side of a mi355lz4_hcdict (kernels/encode.inc, k_hcdict_build_fast): a second allocation beside
// the image above -- encode_wave.hpp's table (positions, then tags) after the seed steps of the kept bytes that hold no seam
// position, then uint32 {keep, first position of the first seam step, -, -}.  The kept bytes themselves are the image's.
#define FASTDICT_TABLE_BYTES 10240                                // ENC_TABLE_ENTRIES 16-bit units (checked where the kernels are compiled)
#define FASTDICT_KEEP_OFF    FASTDICT_TABLE_BYTES
#define FASTDICT_IMAGE_BYTES (FASTDICT_KEEP_OFF + 16)
#define FASTDICT_SCRATCH_MAX ((size_t)1 << 30)                    // the staging windows of one call (the bound of SEG_SCRATCH_MAX)
#define FASTDICT_WAVES_DEFAULT 16                                 // waves per CU of k_encode_fastdict's grid (MI355LZ4_FASTDICT_WAVES)

// a level-0 batch against one prepared dictionary (mi355lz4_compress_fastdict_device; kernels/encode.inc, k_encode_fastdict): wave w
// lays the kept bytes and, behind them, one block at a time into its window at stage + w * stageStride, as HcDictArgs' workgroups do
struct FastDictArgs {
    EncodeArgs e;                // blocks, slots, headers, framedLen, accel (clamped); e.uniformLen bounds every length; linked, lookBack unused
    const uint8_t *image;        // HCDICT_IMAGE_BYTES, read-only: the kept bytes
    const uint8_t *fast;         // FASTDICT_IMAGE_BYTES, read-only
    uint8_t *stage;              // one window per wave of the grid
    size_t stageStride;          // >= 65536 + e.uniformLen + 64
};

// fixed-size output pages against the same object (mi355lz4_compress_pages_fastdict_device; kernels/encode.inc, k_pages_fastdict):
// PagesFastArgs' chains by FastDictArgs' grid -- wave w walks inputs w, w + grid, .. and stages every page's slice of the input
// behind the kept bytes in its window
struct PagesFastDictArgs {
    PagesArgs p;
    int accel;                   // clamped to 1..65537
    const uint8_t *image;        // HCDICT_IMAGE_BYTES, read-only: the kept bytes
    const uint8_t *fast;         // FASTDICT_IMAGE_BYTES, read-only
    uint8_t *stage;              // one window per wave of the grid
    size_t stageStride;          // >= 65536 + 65536 + 64: a page never holds more than 65536 input bytes
};

// a set of prepared dictionaries (mi355lz4_dictset): a table on the device, one entry per member, that holds
// the members' two images by pointer -- the set owns neither -- and, behind the entries, two words {stagings, grid} of the last
// mi355lz4_compress_fastdict_multi_device call (diagnostics: mi355lz4_debug_dictset_last)
struct DictSetEntry {
    const uint8_t *image;        // HCDICT_IMAGE_BYTES: the kept bytes and their count
    const uint8_t *fast;         // FASTDICT_IMAGE_BYTES
};
#define DICTSET_MAX 65536

// a level-0 batch in which block i names its dictionary (mi355lz4_compress_fastdict_multi_device; kernels/encode.inc,
// k_encode_fastdict_multi): FastDictArgs' grid and windows; wave w takes order[w * nBlocks / grid, (w + 1) * nBlocks / grid), the
// blocks grouped by dictIdx (launch_dictset_group), and restages its window when the member changes
struct FastDictMultiArgs {
    EncodeArgs e;                // as FastDictArgs'
    const DictSetEntry *set;     // nDicts entries
    int nDicts;
    const int32_t *dictIdx;      // per block: a member, or -1 (no dictionary); anything else: framedLen 0, the slot untouched
    int32_t *order;              // scratch, nBlocks: the block numbers grouped by dictIdx
    uint32_t *bins;              // scratch, nDicts + 2: counts, then cursors, of the groups {-1, 0 .. nDicts - 1, out of range}
    int32_t *range;              // scratch, grid + 1: wave w takes order[range[w], range[w + 1])
    uint32_t *last;              // the set's {stagings, grid}
    uint8_t *stage;              // one window per wave of the grid
    size_t stageStride;          // >= 65536 + e.uniformLen + 64
};

// independent blocks, each against the kept bytes of the member it names (mi355lz4_decompress_dict_multi_device;
// kernels/linked_walk.inc, k_decode_dict_multi): d.dict0 / d.dict0Len are not used
#define BLK_E_DICT (-0x7F000006)
struct DictMultiArgs {
    DecodeArgs d;
    const DictSetEntry *set;
    int nDicts;
    const int32_t *dictIdx;      // per block: a member, or -1 (no dictionary); anything else: result BLK_E_DICT, nothing written
};

// many linked decode streams continued across calls (mi355lz4_decompress_dstreams_device; kernels/linked_walk.inc, k_decode_dstreams).
// One slot of a mi355lz4_dstreams is the device form of LZ4_streamDecode_t for separately allocated blocks: the last
// min(r, 65536) bytes of the stream's last block that decoded to r > 0 bytes, at the slot's start, and that count.
#define DSTREAM_DICT_BYTES 65536
#define DSTREAM_COUNT_OFF  ((size_t)DSTREAM_DICT_BYTES)           // uint32 count (the rest of the 64 bytes is unused)
#define DSTREAM_SLOT_BYTES (DSTREAM_COUNT_OFF + 64)               // 65600: about 64 KiB a slot

struct DStreamsArgs {
    DecodeArgs d;                // blocks, headers, outputs, result, ckFail; nothing of the linked second pass is used
    const int32_t *work;         // per wave of the launch {first block, end block, slot of the set}
    uint8_t *state;              // the set's slots, DSTREAM_SLOT_BYTES each
};

// many fast linked compress streams continued across calls (mi355lz4_compress_streams_fast_device; kernels/encode.inc,
// k_fstreams_plan / k_encode_fstreams / k_fstreams_save).  One slot of a mi355lz4_fstreams is the dstreams slot:
// the last min(n, 65536) bytes of the stream's last good block at the slot's start, and that count (0: no dictionary) --
// launch_dstreams_set serves _reset and _set_dict of both sets.
#define FSTREAM_DICT_BYTES DSTREAM_DICT_BYTES
#define FSTREAM_COUNT_OFF  DSTREAM_COUNT_OFF
#define FSTREAM_SLOT_BYTES DSTREAM_SLOT_BYTES
#define FSTREAMS_WAVES_DEFAULT FASTDICT_WAVES_DEFAULT             // waves per CU of k_encode_fstreams' grid (MI355LZ4_FSTREAMS_WAVES)

struct FStreamsArgs {
    EncodeArgs e;                // blocks, slots, headers, framedLen, accel (clamped); e.uniformLen bounds every length; linked, lookBack unused
    const int32_t *work;         // per stream with blocks in the call {first block, end block, slot of the set}
    int nWork;
    uint8_t *state;              // the set's slots, FSTREAM_SLOT_BYTES each
    int32_t *good;               // scratch, nWork: the stream's first block with a bad length, or its end block
    int32_t *blockStream;        // scratch, nBlocks: the entry of work[] a block belongs to
    uint8_t *stage;              // one window per wave of the grid
    size_t stageStride;          // >= 65536 + e.uniformLen + 64
};

// small batches: a block's segments are compressed by several waves (kernels/encode.inc, "K2, small batches")
struct EncodeSegArgs {
    EncodeArgs e;
    int segs;                    // segments per block
    int segLen;                  // bytes per segment (the last one takes the rest)
    uint64_t *lists;             // sequence records: block b's segment j at lists + b * listStride + s0 / 4 + j
    size_t listStride;           // records per block: maxBlockLen / 4 + segs + 1
    uint32_t *segCount;          // records per segment
    uint32_t *segBytes;          // bytes a segment's records emit to (k_seg_sizes)
    int32_t *segPrevEnd;         // end of the last sequence in front of the segment
};
void launch_encode_seg(const EncodeSegArgs &a, hipStream_t s);
void launch_decode_seq(const DecodeArgs &a, hipStream_t s);
void launch_decode_par(const DecodeArgs &a, unsigned long long *stats, hipStream_t s);
void launch_decode_cu(const DecodeArgs &a, hipStream_t s);       // one workgroup per block (decode_cu.hpp): calls that do not fill the GPU
// partial decode (a.target set): form 1 = one wavefront per block, sequence at a time; 4 = one workgroup per block for the blocks
// their target does not cut short, the others left to the lane-parallel form; anything else = the lane-parallel form
void launch_decode_partial(const DecodeArgs &a, int form, hipStream_t s);
#ifdef MI355LZ4_EXPERIMENTS
void launch_decode_tok(const DecodeArgs &a, hipStream_t s);      // token lists (a.tok.list / a.tok.cnt), then the list-driven decoder
#endif
#define PAR_STATS_COUNT 32
// What the runtime says about kernel `which` of the lane-parallel family (kernels/kernel_info.inc lists them): out[0] = resident
// workgroups per CU, out[1] = static LDS bytes, out[2] = registers, out[3] = sizeof(ParLds).  0, -1 for an unknown kernel, or a hipError_t.
int decode_kernel_info(int which, int *out);
void launch_linked_tolerant(const DecodeArgs &a, hipStream_t s);   // both cover blocks [a.segFirst, a.segEnd)
void launch_linked_resolve(const DecodeArgs &a, hipStream_t s);
void launch_linked_resolve_a(const DecodeArgs &a, hipStream_t s);   // pointers only (no output byte is read)
void launch_linked_resolve_b(const DecodeArgs &a, hipStream_t s);   // data: fetch, finish, fallbacks
void launch_linked_fetch_block(const DecodeArgs &a, hipStream_t s);  // data: the fetch of block a.onlyBlk alone; PtrCtl::lastOpen tells whether it is complete
size_t ptr_ctl_last_open_offset();
void launch_longest_stream(const DecodeArgs &a, hipStream_t s);   // linkStat[3]
void launch_cu_linked(const DecodeArgs &a, bool decode, hipStream_t s);   // one pass over the dependent blocks (a.cu.pass; decode = false: the first launch has made it), then the snapshots
void launch_cu_publish(const DecodeArgs &a, hipStream_t s);      // a.cu.res -> a.result for the dependent blocks
void launch_dict_share(const DecodeArgs &a, int step, int count, hipStream_t s);   // linkStat[8], [9]: bytes taken directly from the dictionary / bytes walked, over `count` blocks from a.segFirst on
void launch_link_stat(const DecodeArgs &a, hipStream_t s);       // linkStat from result[] (the decode launchers call it themselves)
void launch_runin_decode(const DecodeArgs &a, hipStream_t s);    // long linked stream: every piece with its run-in + the comparison
void launch_runin_fix(const DecodeArgs &a, hipStream_t s);       // ... one round (a.run.round) of pieces to be redone
void launch_runin_publish(const DecodeArgs &a, hipStream_t s);   // ... results into result[]
void launch_linked_runs(const DecodeArgs &a, hipStream_t s);      // one stream, short runs of dependent blocks: one wave per run, exact decoder with dictionary
size_t ptr_ctl_bytes();
size_t tol_region_bytes();
void launch_encode(const EncodeArgs &a, bool bigBlocks, hipStream_t s);   // bigBlocks: some block is above 64 KiB
void launch_encode_hc(const EncodeArgs &a, int level, hipStream_t s);      // compression levels 1..12 (encode_hc.hpp)
// reference-exact compression (encode_exact.hpp): speculate pieces first..first+count-1, or redo them from their
// predecessors' tables; compare piece p's assumed table with piece p-1's final one for p = first..first+count-1;
// save the stream's state
void launch_exact_chain(const ExactArgs &a, int first, int count, int redo, hipStream_t s);
void launch_exact_verify(const ExactArgs &a, int first, int count, hipStream_t s);
void launch_exact_finish(const ExactArgs &a, hipStream_t s);
// many reference-exact streams: one wave per entry of a.work walks its blocks from its slot's state and stores the state back
void launch_exact_streams(const ExactStreamsArgs &a, int nWork, hipStream_t s);
// LZ4_loadDict on one slot (slotState = its CSTREAM_SLOT_BYTES): table, scalars and the last min(len, 65536) bytes of dict
void launch_cstreams_load_dict(uint8_t *slotState, const uint8_t *dict, int len, hipStream_t s);
// one wave per block, each from a copy of the slot's state; nothing is stored back
void launch_exact_dict(const ExactDictArgs &a, hipStream_t s);
// fixed-size output pages: one wave per input walks its chain of pages, each from a zeroed table
void launch_exact_pages(const PagesArgs &a, hipStream_t s);
// the same chains, each page by the wave encoder with an output budget: one wave per input at k_encode's occupancy
void launch_pages_fast(const PagesFastArgs &a, hipStream_t s);
// a prepared high-compression dictionary: one workgroup builds the image (HCDICT_IMAGE_BYTES) from the last min(len, 65536) bytes of dict
void launch_hcdict_build(uint8_t *image, const uint8_t *dict, int len, hipStream_t s);
// compression levels 1..12 against that image: a persistent grid of encode_hc_dict_grid(nBlocks) workgroups, one window of a.stage each
int encode_hc_dict_grid(int nBlocks);
void launch_encode_hc_dict(const HcDictArgs &a, int level, hipStream_t s);
// the wave encoder's table image of the same dictionary (FASTDICT_IMAGE_BYTES): one wavefront
void launch_hcdict_build_fast(uint8_t *fast, const uint8_t *dict, int len, hipStream_t s);
// level 0 against both images: a persistent grid of encode_fastdict_grid(..) single waves, one window of a.stage each.  knob:
// MI355LZ4_FASTDICT_WAVES (> 0 waves per CU, < 0 waves in all, 0 the default); the grid shrinks to FASTDICT_SCRATCH_MAX of windows
int encode_fastdict_grid(int nBlocks, int knob, size_t stageStride);
// a window of that grid (the stageStride of the four argument structs that have one): the dictionary, the block, and what the
// encoder may ask for around a position near the block's end (the 56 bytes behind a candidate, the 8 in front of the next one),
// in whole 256-byte lines
inline size_t fastdict_window_stride(int maxBlockLen) { return 65536 + (((size_t)maxBlockLen + 64 + 255) & ~(size_t)255); }
void launch_encode_fastdict(const FastDictArgs &a, int grid, hipStream_t s);
// fixed-size output pages against both images: the same grid over inputs (encode_fastdict_grid(nInputs, ..)), one chain at a time per wave
void launch_pages_fastdict(const PagesFastDictArgs &a, int grid, hipStream_t s);
// level 0 with a dictionary per block: the grouping pass (a.bins, a.order, a.last from a.dictIdx; four small launches, nothing
// read on the host), then the grid above over the grouped blocks
void launch_dictset_group(const FastDictMultiArgs &a, int grid, hipStream_t s);
void launch_encode_fastdict_multi(const FastDictMultiArgs &a, int grid, hipStream_t s);
// many fast linked streams: the plan (a.good, a.blockStream from the lengths; one wave per entry of a.work), the persistent grid of
// single waves over all blocks of all streams (the slots only read), then the slots' new tails (one workgroup per entry of
// a.work), one behind the other on s.  Nothing is read on the host.
void launch_fstreams(const FStreamsArgs &a, int grid, hipStream_t s);
// ... of a set whose level is 1..12 (mi355lz4_fstreams_set_level): the same plan and the same save around k_encode_hc_fstreams, a
// persistent grid of encode_hc_fstreams_grid(..) workgroups of the hash-chain encoder, one window of a.stage each -- the smallest
// of the blocks, the CUs and the windows FASTDICT_SCRATCH_MAX holds.  knob: MI355LZ4_HSTREAMS_GROUPS, that many workgroups,
// clamped to 1..CUs (0: not set)
int encode_hc_fstreams_grid(int nBlocks, int knob, size_t stageStride);
void launch_fstreams_hc(const FStreamsArgs &a, int grid, int level, hipStream_t s);
void launch_encode_hc_fstreams(const FStreamsArgs &a, int grid, int depth, hipStream_t s);     // (its middle launch: kernels_hstreams.hip)
// independent blocks against one external dictionary (a.dict0, a.dict0Len; a.linked is not used): one wave per block
void launch_decode_dict(const DecodeArgs &a, hipStream_t s);
// ... each against the member of a set that it names: one wave per block
void launch_decode_dict_multi(const DictMultiArgs &a, hipStream_t s);
// many linked decode streams: one wave per entry of a.work walks its blocks from its slot's dictionary and stores the tail back;
// launch_dstreams_set: slots [first, first + count) take the keep <= 65536 bytes at src as their dictionary (0: reset)
void launch_decode_dstreams(const DStreamsArgs &a, int nWork, hipStream_t s);
void launch_dstreams_set(uint8_t *state, int first, int count, const uint8_t *src, uint32_t keep, hipStream_t s);
void launch_compact(const uint8_t *slots, size_t slotStride, const int32_t *framedLen, int nBlocks,
                    uint8_t *dense, size_t denseCap, uint64_t *denseOff, hipStream_t s);
void launch_interleave(const uint8_t *local, const uint64_t *localOff, int nLocal, int rank, int nRanks,
                       uint8_t *global, const uint64_t *globalOff, hipStream_t s);
void launch_index(const uint8_t *framed, uint64_t framedLen, const uint64_t *blockOff, int nBlocks,
                  int headerKind, int fixedUncomp, int32_t *scratchSizes, uint64_t *outOff, hipStream_t s);
// decoded sizes (size_walk.hpp): size[i] = what block i decodes to, read off its token chain, or BLK_E_SIZE_UNKNOWN / a
// header code; outOff (may be null) = exclusive scan of the sizes that are known, nBlocks + 1 entries.  trailer: every
// block's data is followed by a 4-byte checksum (it must lie inside the framed buffer; it is not verified here).
void launch_decoded_size(const uint8_t *framed, uint64_t framedLen, const uint64_t *blockOff, int nBlocks, int headerKind,
                         int maxUncomp, int trailer, int32_t *size, uint64_t *outOff, hipStream_t s);
// block checksums (checksum.hpp): xxh32(seed) of base + off[i], len[i] bytes -> out[i]; the compress side's trailers
// (slot i's data hashed, the trailer written behind it, framedLen[i] += 4; failed blocks left alone); the decode side's
// per-block flags (fail[i] = data does not match its trailer; 0 for blocks whose header or trailer is out of bounds)
void launch_xxh32_ranges(const uint8_t *base, const uint64_t *off, const int32_t *len, int n, uint32_t seed, uint32_t *out,
                         hipStream_t s);
void launch_xxh32_append(uint8_t *slots, size_t slotStride, int headerKind, int32_t *framedLen, int n, hipStream_t s);
void launch_xxh32_verify(const DecodeArgs &a, int32_t *fail, hipStream_t s);
// batches of standard LZ4 frames (mi355lz4_frames; kernels/frames.inc).  Input i is buf[inOff[i], inOff[i] + inLen[i]):
// any sequence of LZ4 frames and skippable frames.  The tables cost a fixed number of bytes per input, per frame and per block.
#define FRM_E_MAGIC            (-0x7F000101)   // = MI355LZ4_FRM_E_* (include/mi355lz4.h)
#define FRM_E_HEADER           (-0x7F000102)
#define FRM_E_HEADER_CHECKSUM  (-0x7F000103)
#define FRM_E_TRUNCATED        (-0x7F000104)
#define FRM_E_BLOCK_SIZE       (-0x7F000105)
#define FRM_E_BLOCK_CHECKSUM   (-0x7F000106)
#define FRM_E_BLOCK            (-0x7F000107)
#define FRM_E_CONTENT_SIZE     (-0x7F000108)
#define FRM_E_CONTENT_CHECKSUM (-0x7F000109)
#define FRM_SKIP_CONTENT_CHECKSUM 1u
#define FRM_SKIP_BLOCK_CHECKSUM   2u
// a frame's flags word: the FLG byte of its descriptor, and
#define FRM_F_BROKEN 0x100u                    // a structural error ended the frame: it has no end mark, size or checksum to check
// what the decode does with a block (FramesArgs::kind)
enum { FRM_K_NONE = 0, FRM_K_COMP = 1, FRM_K_STORED = 2, FRM_K_LINKED = 3 };

struct FrmFrame {
    uint64_t endPos;         // position of the end mark in buf (of the structural error: a broken frame)
    uint64_t declared;       // content size of the descriptor
    uint64_t outRel;         // where the frame's content starts in its input's output (k_frames_layout)
    uint64_t size;           // the frame's content size (k_frames_layout)
    int32_t input, firstBlock, nBlocks;
    uint32_t flags;          // FLG | FRM_F_*
    uint32_t blockMax;
    uint32_t checksum;       // the content checksum word
};
struct FrmBlock {
    uint64_t payOff;         // the block's bytes in buf; its size word lies 4 bytes in front
    uint64_t outRel;         // where it decodes to in its input's output (k_frames_layout)
    uint32_t n;              // stored bytes; bit 31: the block is stored, not compressed
    int32_t frame;
    int32_t size;            // what it decodes to, or SIZE_E_UNKNOWN (k_frames_sizes)
    int32_t kind;            // FRM_K_* (k_frames_layout)
};
struct FramesArgs {
    const uint8_t *buf; uint64_t bufLen;
    const uint64_t *inOff, *inLen;      // the object's copies
    int nInputs; uint32_t flags;
    // per input
    int32_t *nFrames, *nBlocks;         // k_frames_scan's counts
    int32_t *err; uint64_t *errPos;     // ... the first structural error (0: none) and its position in buf
    uint64_t *frameFirst, *blockFirst;  // exclusive scans of the counts, nInputs + 1 entries
    int64_t *sizes;                     // the decoded size, or the load-time code
    uint64_t *errKey;                   // decode: the smallest (position << 4 | code) of the decode-time errors
    // per frame, per block
    FrmFrame *frames; FrmBlock *blocks;
    int nFramesAll, nBlocksAll;
    int32_t *bsumFail;                  // per block: its checksum does not match (k_frames_bsum)
    // lists made by k_frames_layout: counts[0] compressed blocks of independent frames, counts[1] linked frames
    uint32_t *counts; int32_t *indep; int32_t *linked;
    // decode: the engine's call over the indep list
    uint64_t *decOff, *decOut; int32_t *decCap, *decRes;
    int nIndep, nLinked;
    uint8_t *out; const uint64_t *outOff; int64_t *result;
};
void launch_frames_scan(const FramesArgs &a, hipStream_t s);      // counts, first structural error, the scans of the counts
void launch_frames_load(const FramesArgs &a, hipStream_t s);      // fill, block checksums, sizes, layout
void launch_frames_place(const FramesArgs &a, hipStream_t s);     // decode: errKey reset, the engine call's arrays from outOff
void launch_frames_decode(const FramesArgs &a, hipStream_t s);    // decode: stored blocks, linked frames, verdicts, checksums, result
// writing batches of standard LZ4 frames (mi355lz4_cframes; kernels_cframes.hip).  Input i is src[inOff[i], inOff[i] +
// inLen[i]) and becomes one frame at dst + dstOff[i].  The block table of a call has tabCap entries: realCap real blocks at the
// most, and with CFRM_LINKED one zero-length spacer behind every input's blocks -- block k of input i is entry blockFirst[i] + k
// (+ i with spacers).  An entry past the real ones, a spacer and an entry of a refused input have length 0 and blockInput -1.
#define FRW_E_CAPACITY (-0x7F000201)           // = MI355LZ4_FRW_E_* (include/mi355lz4.h)
#define FRW_E_INPUT    (-0x7F000202)
#define CFRM_LINKED            1u              // = MI355LZ4_CFRAMES_*
#define CFRM_BLOCK_CHECKSUM    2u
#define CFRM_CONTENT_SIZE      4u
#define CFRM_CONTENT_CHECKSUM  8u
#define CFRM_PIECE 16384u                      // k_cframes_pack: bytes of a block's payload one wave copies
struct CFramesArgs {
    const uint8_t *src; uint64_t srcBufLen;
    const uint64_t *inOff, *inLen;
    int nInputs;
    uint64_t maxInputLen;
    uint32_t bmax;                             // the frames' block maximum, 1 << (8 + 2 * bsid)
    int bsid;
    uint32_t flags;                            // CFRM_*
    int realCap, tabCap;
    int maxBlockLen;                           // min(bmax, maxInputLen): what the engine's call is told
    uint8_t *dst; const uint64_t *dstOff, *dstCap; int64_t *frameLen;
    // per input
    int32_t *nb;                               // blocks of the input, -1: refused by its range or its length (k_cframes_count)
    uint64_t *blockFirst;                      // exclusive scan of nb, nInputs + 1 entries
    int64_t *verdict;                          // what frameLen[i] gets (k_cframes_layout)
    uint64_t *base;                            // dstOff[i] + header bytes - pieceOff[the input's first entry]
    // per entry of the table: the engine call's arrays, and what the frame layer makes of its results
    uint64_t *srcOff; int32_t *srcLen; int32_t *blockInput; int32_t *framedLen;
    int32_t *piece;                            // 4 + payload + 4 with block checksums; 0 for an entry that is no block
    uint64_t *pieceOff;                        // exclusive scan of piece, tabCap + 1 entries
    uint8_t *slots; size_t slotStride;
};
void launch_scan_u64(const int32_t *sizes, int n, uint64_t *offs, hipStream_t s);   // k_scan_u64 (kernels/compact.inc), n + 1 offsets
void launch_cframes_plan(const CFramesArgs &a, hipStream_t s);    // k_cframes_count, the scan, k_cframes_plan
void launch_cframes_finish(const CFramesArgs &a, hipStream_t s);  // behind the engine's call: sizes, the scan, layout, pack, head
// dense[run, run + frameLen[i]) = dst[dstOff[i], ..) for the inputs with frameLen[i] >= 0, run = the scan of those lengths (host
// form: scanOff is scratch of nInputs + 1 entries; scanOff[nInputs] = the total); nothing is copied when the total is above denseCap
void launch_cframes_gather(const uint8_t *dst, const uint64_t *dstOff, const int64_t *frameLen, int nInputs, uint64_t *scanOff,
                           uint8_t *dense, uint64_t denseCap, hipStream_t s);
void launch_generate(int kind, uint8_t *dst, int blockLen, int nBlocks, uint64_t firstBlock,
                     uint64_t blockStep, uint32_t litMax, uint32_t offMax, hipStream_t s);
