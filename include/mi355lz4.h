/*
 * mi355lz4.h -- C ABI of the MI355X (gfx950) LZ4 block engine.
 *
 * This is the drop-in boundary for the hot path of composewell/streamly-lz4:
 * the two foreign calls made once per block by Streamly.Internal.LZ4,
 *
 *   c_compressFastContinue    src/Streamly/Internal/LZ4.hs:123-131 -> cbits/lz4.c:1565
 *   c_decompressSafeContinue  src/Streamly/Internal/LZ4.hs:133-140 -> cbits/lz4.c:2322
 *
 * plus the framing those calls are wrapped in (compressChunk :226-281,
 * decompressChunk :291-336, header layout :177-207).
 *
 * Two faces:
 *   (1) include/lz4.h  -- the exact 7 legacy symbols the Haskell imports today
 *       (one block per call; source compatible, not how a GPU should be fed);
 *   (2) this header    -- the batched ABI (N blocks per call) the modified
 *       Haskell combinators in INTEGRATION.md bind with `ccall safe`.
 *
 * Plain pointers and sizes only; no C++ or torch types.  All functions return
 * MI355LZ4_OK (0) or a negative MI355LZ4_E_* code unless stated otherwise.
 * Every entry point fails with MI355LZ4_E_NO_DEVICE when no gfx950 device is
 * usable: there is NO CPU fallback.
 *
 * Framed block layout (identical to the reference, little-endian int32s):
 *   headerKind 8 (BlockHasSize, default): [compLen][uncompLen][compLen bytes]
 *   headerKind 4 (BlockMax64KB..4MB)    : [compLen][compLen bytes]
 *
 * Blocks produced by the compressor are INDEPENDENT LZ4 blocks (no reference
 * into a previous block), which the reference's linked decoder accepts
 * unchanged.  The decompressor also accepts the reference's LINKED streams:
 * see mi355lz4_decompress_batch_device (linked != 0).
 */
#ifndef MI355LZ4_H
#define MI355LZ4_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355LZ4_VERSION 100

/* ---- status codes --------------------------------------------------- */
#define MI355LZ4_OK              0
#define MI355LZ4_E_NO_DEVICE    (-1)  /* no usable HIP device / not gfx950 */
#define MI355LZ4_E_HIP          (-2)  /* a HIP runtime call failed (see mi355lz4_last_error) */
#define MI355LZ4_E_ARG          (-3)  /* bad argument */
#define MI355LZ4_E_CAPACITY     (-4)  /* output buffer too small */
#define MI355LZ4_E_BLOCK        (-5)  /* at least one block failed; see per-block status */
#define MI355LZ4_E_STREAM       (-6)  /* malformed framed stream (header chain) */

/* Per-block decode results follow the reference: >= 0 is the decoded size,
 * -1 .. -(compLen+1) is cbits/lz4.c:2163's -(ip-src)-1.  Header-level
 * rejections (what decompressChunk checks at Internal/LZ4.hs:309-318, plus the
 * short-array case it misses) use this separate range: */
#define MI355LZ4_BLK_E_COMPLEN   (-0x7F000001)  /* compLen <= 0 or > LZ4_compressBound(LZ4_MAX_INPUT_SIZE) */
#define MI355LZ4_BLK_E_TRUNCATED (-0x7F000002)  /* header/data runs past the framed buffer */
#define MI355LZ4_BLK_E_UNCOMPLEN (-0x7F000003)  /* negative uncompLen / exceeds output capacity */
#define MI355LZ4_BLK_E_CHECKSUM (-0x7F000004)   /* data does not match its trailer (mi355lz4_set_block_checksum) */
#define MI355LZ4_BLK_E_SIZE_UNKNOWN (-0x7F000005) /* mi355lz4_decoded_size_device: the token chain gives no size the call vouches for */
#define MI355LZ4_BLK_E_DICT (-0x7F000006)       /* mi355lz4_decompress_dict_multi_device: dictIdx[i] names no member of the set */

/* per-input codes of the frame batches (mi355lz4_frames: sizes[] and result[]); an input reports the error with the smallest
 * byte position in it */
#define MI355LZ4_FRM_E_MAGIC            (-0x7F000101)  /* no frame begins here (trailing bytes too) */
#define MI355LZ4_FRM_E_HEADER           (-0x7F000102)  /* version, reserved bits, BD code, DictID */
#define MI355LZ4_FRM_E_HEADER_CHECKSUM  (-0x7F000103)
#define MI355LZ4_FRM_E_TRUNCATED        (-0x7F000104)  /* the input ends inside a frame */
#define MI355LZ4_FRM_E_BLOCK_SIZE       (-0x7F000105)  /* a block word above the frame's block maximum */
#define MI355LZ4_FRM_E_BLOCK_CHECKSUM   (-0x7F000106)
#define MI355LZ4_FRM_E_BLOCK            (-0x7F000107)  /* no size to vouch for, or the decode does not give that size */
#define MI355LZ4_FRM_E_CONTENT_SIZE     (-0x7F000108)
#define MI355LZ4_FRM_E_CONTENT_CHECKSUM (-0x7F000109)

#define MI355LZ4_MAX_INPUT_SIZE 0x7E000000      /* = LZ4_MAX_INPUT_SIZE, cbits/lz4.h:170 */

typedef struct mi355lz4_ctx mi355lz4_ctx;

/* ---- what a call may write -------------------------------------------
 * A caller's arrays lie next to other live data, so every call is confined to the ranges below, whatever its blocks'
 * results (tests/test_write_confinement_gpu.py holds every kernel to it with guard patterns around every range).
 * Decode calls (_decompress_batch_device, _decompress_streams_device, _decompress_linked_begin / _end / _end_last):
 *   no byte of `out` outside the union of [outOff[i], outOff[i] + cap_i), where cap_i is outCap[i], else the header's
 *   uncompLen / fixedUncomp, and 0 when the header is rejected for its uncompLen -- for a block that decodes, one that
 *   fails with a negative code and one whose header is rejected alike; result[] only in [0, nBlocks) (with lookBack,
 *   result[-1] and the seam block's output are the caller's: read, never written); framed, blockOff, outOff, outCap
 *   and streamFirst are never written.
 * Partial decode (_decompress_partial_device): no byte of `out` outside the union of [outOff[i], outOff[i] +
 *   min(target[i], cap_i)), cap_i as above -- stricter than the reference, whose wide copies run up to 31 bytes past a
 *   sequence -- and nothing at all for a block whose header is rejected or whose target is negative; whatever the
 *   block's result, so prefixes can lie back to back at outOff = scan(min(target, cap)).  result[] only in
 *   [0, nBlocks); target, framed, blockOff, outOff and outCap are never written.
 * Compress calls (_compress_batch_device: level 0, 1..9, exact; linked or not; segments automatic, forced or off;
 *   checksums on or off): nothing outside the union of [slots + i*slotStride, slots + i*slotStride +
 *   mi355lz4_slot_stride_ex(maxBlockLen, headerKind, checksum)), even when the caller's slotStride is larger (the
 *   rest of a wider stride is the caller's); framedLen[] only in [0, nBlocks); src, srcOff and srcLen never.
 * _compact_device: dense[0, denseOff[k + 1]) for the last block k that fits (denseOff[k + 1] <= denseCap; nothing
 *   when none fits), denseOff[0..nBlocks];
 *   _index_device: outOff[0..nBlocks]; _decoded_size_device: size[0..nBlocks), outOff[0..nBlocks]; _interleave_device: global + globalOff[j*nRanks + rank] for the local blocks'
 *   lengths; _generate_device: dst[0, nBlocks * blockLen); _xxh32_device: out[i] for len[i] >= 0.  Inputs never.
 * Host-buffer calls (_compress_batch, _decompress_batch, _decompress_partial, _decompress_streams, _multi_*): nothing at or past
 *   framedOut + cap / out + cap or in front of either pointer; blockFramedLen, status and blockLen only in
 *   [0, nBlocks) / [0, maxBlocks); inputs never.
 * Many exact streams (_compress_streams_device): the slot ranges of _compress_batch_device, framedLen[0, nBlocks)
 *   (a stream stopped by a bad length leaves its remaining slots untouched and sets their framedLen to 0) and the slots
 *   of `cs` that streamSlot[] names for a stream with blocks; never a slot of `cs` the call does not name, never src,
 *   srcOff or srcLen.  _compress_streams is a host-buffer call as above.
 * Many decode streams (_decompress_dstreams_device): no byte of `out` outside the union of [outOff[i], outOff[i] + cap_i),
 *   cap_i as for the decode calls, whatever the blocks' results; result[] only in [0, nBlocks); of `ds` only the slots that
 *   streamSlot[] names for a stream with blocks -- never a slot the call does not name, never framed, blockOff, outOff or
 *   outCap.  _dstreams_reset / _dstreams_set_dict write the slots they name and nothing else (never the dictionary handed
 *   in).  _decompress_dstreams is a host-buffer call as above.
 * Many fast linked streams (_compress_streams_fast_device): slots[i*slotStride, i*slotStride + framedLen[i]) inside the slot ranges
 *   of _compress_batch_device, framedLen[0, nBlocks) (a stream stopped by a bad length leaves its remaining slots untouched
 *   and sets their framedLen to 0), the slots of `fs` that streamSlot[] names for a stream with blocks, and engine scratch;
 *   never a slot of `fs` the call does not name, never src, srcOff or srcLen.  _fstreams_reset / _fstreams_set_dict write the
 *   slots they name and nothing else (never the dictionary handed in).  _compress_streams_fast is a host-buffer call as above.
 * Shared-dictionary batches: _cstreams_load_dict writes the slot of `cs` it names and nothing else (never the dictionary
 *   handed in).  _compress_dict_device: the slot ranges of _compress_batch_device and framedLen[0, nBlocks); never any
 *   slot of `cs` -- the loaded slot is only read -- never src, srcOff or srcLen.  _decompress_dict_device: no byte of `out`
 *   outside the union of [outOff[i], outOff[i] + cap_i), cap_i as for the decode calls, for a block that decodes, one that
 *   fails and one whose header is rejected alike; result[] only in [0, nBlocks); never the dictionary, framed, blockOff,
 *   outOff or outCap.  _compress_dict and _decompress_dict are host-buffer calls as above.
 * High-compression dictionary batches: _hcdict_load writes the object it is handed and nothing else (never the dictionary handed
 *   in).  _compress_hcdict_device: the slot ranges of _compress_batch_device and framedLen[0, nBlocks) (a length outside
 *   0..maxBlockLen: framedLen[i] = 0, the slot untouched); never the mi355lz4_hcdict -- it is only read -- never src, srcOff or
 *   srcLen.  _compress_hcdict is a host-buffer call as above.  _compress_fastdict_device and _compress_fastdict: the same
 *   ranges and the same rules, at level 0.
 * Fixed-size pages (_compress_pages_device): of page (i, k) -- the pageStride bytes at pages + (i*maxPages + k)*pageStride --
 *   the bytes [0, headerKind + pageCompLen[i*maxPages + k]) and nothing behind them (stricter than the reference, whose wide
 *   copies write past what it returns); pages that are not written -- behind nPages[i], of a skipped input -- not at all.
 *   pageSrcLen[] and pageCompLen[] only at the entries of pages written; nPages[i]; consumed[i] unless the input is skipped
 *   (nPages[i] = 0 is then all that is written for it).  Never src, srcOff, srcLen or pageSize.  _compress_pages writes the same
 *   ranges of the caller's host arrays and nothing else.  _compress_pages_fast_device and _compress_pages_fast: the same ranges
 *   and the same rules.  _compress_pages_fastdict_device and _compress_pages_fastdict: the same ranges and the same rules again,
 *   and never the mi355lz4_hcdict, which is only read.
 * Dictionary sets: _dictset_create writes the set it returns and nothing else.  _compress_fastdict_multi_device: the slot ranges
 *   of _compress_fastdict_device and framedLen[0, nBlocks) (a length outside 0..maxBlockLen or an index outside -1..n-1:
 *   framedLen[i] = 0, the slot untouched); never a member of the set or its images, never dictIdx, src, srcOff or srcLen.
 *   _decompress_dict_multi_device: the ranges of _decompress_dict_device, and nothing of `out` for a block whose index names no
 *   member (result[i] = MI355LZ4_BLK_E_DICT); never a member, dictIdx, framed, blockOff, outOff or outCap.  Of the set itself the
 *   compress call writes two diagnostic words.  _compress_fastdict_multi and _decompress_dict_multi are host-buffer calls as above.
 * Frame batches: _frames_load writes the object it is handed and nothing else (never buf, inOff or inLen).  _frames_decode: no
 *   byte of `out` outside the union of [outOff[i], outOff[i] + sizes[i]) over the inputs with sizes[i] >= 0 -- whatever `buf` holds
 *   at decode time, for an input that decodes and one that fails at decode time alike -- nothing at all for an input whose size is
 *   a code; result[] only in [0, nInputs); never buf or outOff; of the object only its decode scratch.  _decompress_frames is a
 *   host-buffer call as above (result only in [0, nInputs)).
 * Frame writer: _cframes_compress: dst[dstOff[i], dstOff[i] + frameLen[i]) for the inputs with frameLen[i] >= 0 -- nothing behind
 *   a frame's end inside its capacity -- nothing of dst for an input that gets a code; frameLen[] only in [0, nInputs); the
 *   object's scratch; never src, inOff, inLen, dstOff or dstCap.  _cframes_reserve writes nothing but the object.
 *   _compress_frames is a host-buffer call as above (frameLen only in [0, nInputs); nothing of out with MI355LZ4_E_CAPACITY).
 * Scratch that a call needs is the engine's own. */

/* ---- engine lifecycle ------------------------------------------------ */
int mi355lz4_version(void);
/* Thread-local description of the last failure in this library. */
const char *mi355lz4_last_error(void);
/* Number of usable gfx950 devices (0 when none; never fails). */
int mi355lz4_device_count(void);
/* Create an engine bound to HIP device `device` with its own stream.
 *
 * Threads: an engine is NOT thread-safe -- one engine per thread, or the caller serialises its calls (the
 * reference's contexts are the same: one per stream, one Haskell thread, Internal/LZ4.hs:105-143).  Different
 * engines may be used from different threads at the same time.  mi355lz4_last_error is thread-local.
 *
 * Streams: every *_device call only ENQUEUES work on the engine's stream (its own, or the one given to
 * mi355lz4_set_stream) and returns; the exception is a linked decode (linked != 0, or the streams call), which
 * waits on the host for its first pass before it decides whether a second one is needed.  The scratch memory of a
 * linked decode belongs to the engine: two linked decodes of ONE engine must be issued on the same stream, or the
 * caller orders them.  The host-buffer calls (mi355lz4_compress_batch, mi355lz4_decompress_batch, ..._streams)
 * are synchronous and use, besides the engine's stream, two copy streams and two compute streams created on first
 * use, plus a small pool of host threads for staging pageable memory (MI355LZ4_COPY_THREADS, default 8); for the
 * duration of such a call the engine's stream is one of its own.
 * Which *_device call is in which class (tests/test_stream_order_gpu.py holds every one to it on a non-blocking stream:
 * the enqueue-only ones return before work queued in front of them on the stream has run):
 *   wait on the host, by design: mi355lz4_decompress_batch_device with linked != 0 (unless mi355lz4_set_linked_async),
 *     mi355lz4_decompress_streams_device, mi355lz4_decompress_linked_begin / _end / _end_last, and
 *     mi355lz4_compress_batch_device in reference-exact mode (mi355lz4_set_compress_exact: it reads the lengths back);
 *   only enqueue: every other one -- mi355lz4_compress_batch_device at level 0 (segments or not, linked or not, block
 *     checksums or not) and at levels 1..9, _compact_device, _decompress_batch_device with linked == 0 or with
 *     mi355lz4_set_linked_async, _decompress_partial_device, _index_device, _decoded_size_device, _xxh32_device,
 *     _generate_device, _interleave_device, _compress_streams_device, _compress_dict_device, _decompress_dict_device,
 *     _compress_hcdict_device, _compress_fastdict_device, _compress_fastdict_multi_device, _decompress_dict_multi_device,
 *     the three _compress_pages*_device calls, _decompress_dstreams_device, _compress_streams_fast_device, and the calls
 *     that prepare their state on the stream (_cstreams_reset, _cstreams_load_dict, _hcdict_load, _dstreams_reset,
 *     _dstreams_set_dict, _fstreams_reset, _fstreams_set_dict).
 *   An enqueue-only call may still wait in three cases, none of which reads the caller's data early: the first use of a
 *   scratch and a scratch that has to grow (hipMalloc / hipFree; the calls that stage dictionary windows -- _compress_hcdict_device,
 *   _compress_fastdict_device, _compress_fastdict_multi_device, _compress_pages_fastdict_device, _compress_streams_fast_device --
 *   synchronise the stream before their staging grows), a fifth stream taking over one of
 *   the four per-stream scratches (segments, dictionary staging: the engine waits for the stream that used it), and the
 *   fifth of five _compress_streams_device / _compress_streams_fast_device / _decompress_dstreams_device calls in flight
 *   on one set (the stream table goes through a ring of four).
 *   The frame batches are methods of an object and carry no suffix: mi355lz4_frames_load waits on the host by design (twice:
 *   for the counts that size its tables, and for the sizes), mi355lz4_frames_decode only enqueues
 *   (tests/test_frames_stream_gpu.py holds it to the same protocol).  So do the frame writer's: mi355lz4_cframes_compress only
 *   enqueues once the object's scratch is large enough (mi355lz4_cframes_reserve, or an earlier call of the shape;
 *   tests/test_cframes_stream_gpu.py).
 *
 * Process environment: the library sets no environment variable; the HIP runtime's settings (GPU_MAX_HW_QUEUES
 * among them) are the process's. */
int mi355lz4_create(mi355lz4_ctx **out, int device);
void mi355lz4_destroy(mi355lz4_ctx *ctx);
/* Launch on a caller-owned hipStream_t instead (e.g. torch's current stream). */
int mi355lz4_set_stream(mi355lz4_ctx *ctx, void *hipStream);
void *mi355lz4_get_stream(mi355lz4_ctx *ctx);
int mi355lz4_synchronize(mi355lz4_ctx *ctx);
/* Linked decodes without a host wait.  mi355lz4_decompress_batch_device(linked != 0) normally waits on the host for
 * its first pass, to learn whether any block needs its dictionary and which ones (a stream of independent blocks pays
 * that wait and nothing else).  With maxDecodedBlockSize > 0 (an upper bound of any block's decoded size, e.g. 65536)
 * the call only enqueues: the second pass is issued over all blocks of the call and its kernels return at once when
 * the first pass found nothing to do (about a dozen empty launches per 4096 blocks).  The call can then be captured in
 * a graph and no longer serialises a caller's pipeline; it costs more than the wait on big batches of independent
 * blocks (measured in DESIGN.md), which is why it is opt-in.  0 restores the default.  The streams call
 * (mi355lz4_decompress_streams_device) always waits; mi355lz4_decompress_dstreams_device never does.
 * Before capturing such a call in a graph, make ONE warm-up call with the largest batch the graph will see: the
 * scratch is sized for ALL blocks of the call whether or not any is dependent (lists: one byte per output byte, up
 * to 16384 blocks' worth; source pointers: four bytes per output byte of a 4096-block segment, about 1 GiB) and is
 * allocated (hipMalloc / hipFree, not capturable) the first time a call needs more than the engine holds. */
int mi355lz4_set_linked_async(mi355lz4_ctx *ctx, int maxDecodedBlockSize);
/* Small batches.  With fewer blocks in a call than the chip has wave slots, the compressor cuts every block
 * (8 KiB .. 4 MiB, independent blocks) into segments that several wavefronts compress at once (a block still
 * comes out as one valid LZ4 block; the seams cost about 1 % of size on text).  segs: -1 = automatic (default;
 * MI355LZ4_SEG in the environment overrides it), 0 = never, 2..64 = that many segments whenever possible.
 * Consequences a caller should know: (1) the compressed BYTES of a block depend on how many blocks share the call
 * (the small tail batch of a stream is cut into segments, the big batches before it are not); every form decodes to
 * the same data, and segs = 0 gives bytes that do not depend on the batch.  (2) The segment path keeps a device
 * scratch of about twice the call's input per stream it was used on (at most four streams; a fifth takes over the
 * slot used longest ago) until mi355lz4_destroy; automatic mode leaves the path alone once that scratch would pass
 * 1 GiB, a forced count does not. */
int mi355lz4_set_segments(mi355lz4_ctx *ctx, int segs);
/* Decoder variant: 0 = chosen per call (default), 1 = sequence-at-a-time kernel, 2 = lane-parallel kernel (one wavefront
 * per block: what fills the GPU when a call brings thousands of blocks), 4 = one workgroup per block (sixteen wavefronts
 * share a block's output in LDS, 32 KiB at a time: a block's latency is 1.5-2 x shorter; in a linked call it is the
 * first, standalone pass -- blocks that need their dictionary go through the second pass as ever).  Variant 0 takes
 * variant 4 for calls of up to 256 blocks -- 512 when they hold 16 KiB of compressed bytes or more on average, none when
 * less than 3 KiB -- and variant 2 otherwise (MI355LZ4_CU_BLOCKS = n in the environment: up to n blocks whatever their
 * size; 0 = never); under variant 0 the kernel itself hands a block that saves less than a sixteenth of its size to the
 * lane-parallel decoder (long literal runs end that form's segments), under variant 4 it does not.
 * Tuning/ablation knob; results are identical.  Any other value: MI355LZ4_E_ARG. */
int mi355lz4_set_decoder(mi355lz4_ctx *ctx, int variant);
/* on != 0: the compress calls treat the blocks of a call as consecutive blocks of ONE stream and use block
 * i-1 as block i's dictionary whenever it lies directly in front of it in memory -- what the reference's
 * LZ4_compress_fast_continue does with the previous chunk (cbits/lz4.c:1608-1636, kept alive by
 * Internal/LZ4.hs:376,389).  The output is then a LINKED stream like the reference's (+6 % ratio on text);
 * it must be decoded with linked != 0, in order.  Default off: independent blocks (they shard). */
int mi355lz4_set_linked_compress(mi355lz4_ctx *ctx, int on);

/* = LZ4_compressBound (cbits/lz4.c:674, lz4.h:171): n + n/255 + 16, 0 if n too large */
int mi355lz4_compress_bound(int n);
/* Bytes one worst-case framed slot needs for a block of blockLen bytes, rounded up to 16. */
size_t mi355lz4_slot_stride(int blockLen, int headerKind);

/* ---- device-resident batched API (all data pointers are DEVICE pointers;
 *      asynchronous on the engine's stream) -----------------------------
 * Where a call's regions may lie.  Every block of a call is a region of its own: block i of a decode call is read at
 * framed + blockOff[i] and written at out + outOff[i]; block i of a compress call is read at src + srcOff[i] (or at
 * src + i * blockStride) and written at slots + i * slotStride; a dictionary, a local block of _interleave_device and a
 * range of _xxh32_device are regions too.
 *   - Regions may lie in any order and at any distance from each other: no array of offsets has to ascend, a block may lie
 *     below its predecessor or below the call's first block, and two blocks may be more than 2^32 bytes apart.  A linked
 *     decode's blocks are given in stream order in the ARRAYS; where their bytes lie is free ("separately allocated
 *     blocks").  Only the linked compressor looks at placement: block i - 1 is block i's dictionary when it lies directly
 *     in front of it.
 *   - Output regions (cap_i bytes at outOff[i], a slot, a range of dense / global) must not overlap each other or any
 *     input region of the same call.
 *   - Offsets, strides and a decode call's uint64_t framedLen are full 64-bit quantities, and so is every product the
 *     engine forms from them (i * slotStride, i * blockStride, a slot's place in a cstreams / dstreams set): buffers,
 *     strides and state sets beyond 4 GiB are ordinary arguments.
 * tests/test_placement_gpu.py runs every call below with its regions permuted, straddling and beyond 2^31 and 2^32. */

/* Compress nBlocks blocks.  Block i is src[srcOff[i] .. srcOff[i]+srcLen[i]);
 * srcOff == NULL means srcOff[i] = i * blockStride; srcLen == NULL means every
 * block is maxBlockLen bytes (maxBlockLen must bound every srcLen[i]: it picks
 * the hash-table entry width).  Block i's framed bytes
 * ([header][data]) are written at slots + i*slotStride and their count
 * (headerKind + compLen) to framedLen[i].  accel follows
 * LZ4_compress_fast_continue (clamped to [1,65537], cbits/lz4.c:1577-1578).
 * replaces: compressChunk, Internal/LZ4.hs:226-281. */
int mi355lz4_compress_batch_device(mi355lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff,
                                   const int32_t *srcLen, uint64_t blockStride, int maxBlockLen, int nBlocks,
                                   int accel, int headerKind, uint8_t *slots, size_t slotStride,
                                   int32_t *framedLen);

/* Pack slots into one dense framed stream: denseOff[0..nBlocks] receives the
 * exclusive scan of framedLen (denseOff[nBlocks] = total), dense the bytes.
 * Nothing is written at or past dense + denseCap: a block that does not fit is
 * skipped, and the caller sees it by denseOff[nBlocks] > denseCap (the call is
 * asynchronous, so it cannot report that itself).  nBlocks * slotStride always
 * suffices. */
int mi355lz4_compact_device(mi355lz4_ctx *ctx, const uint8_t *slots, size_t slotStride,
                            const int32_t *framedLen, int nBlocks, uint8_t *dense, size_t denseCap,
                            uint64_t *denseOff);

/* Decompress nBlocks framed blocks.  Block i's header starts at
 * framed + blockOff[i]; its output goes to out + outOff[i] with capacity
 * outCap[i] (outCap == NULL: capacity = header uncompLen, or fixedUncomp for
 * headerKind 4).  result[i] = decoded size or a negative code (see above).
 * linked == 0: every block is decoded on its own (LZ4_decompress_safe).
 * linked != 0: reference stream semantics -- block i may reference the output
 * of the last block before it that decoded to > 0 bytes, exactly as under
 * LZ4_decompress_safe_continue with separately allocated blocks
 * (cbits/lz4.c:2322-2359); blocks must be given in stream order.  Blocks that
 * decode on their own (everything this engine's compressor emits) are final
 * after the parallel kernel; blocks that reach into their predecessor are
 * resolved by a second, data-parallel pass: up to 512 big blocks (512 KiB
 * and more: BlockMax1MB / BlockMax4MB streams) by a workgroup each against a
 * guess of their dictionary, pass after pass until the guesses stand (DESIGN.md
 * 0c: scratch 64 KiB per block), short runs of them by a wave per
 * run, spans of 576 MiB and more by the run-in decode (pieces of the span,
 * each decoded from a few blocks in front of it and checked against what the
 * piece in front wrote, DESIGN.md 0b: scratch two blocks per piece, at most
 * 4096 pieces),
 * everything else through source pointers + pointer jumping (DESIGN.md 1:
 * scratch 1 + 4 bytes per output byte of up to 4096 blocks at a time).  With
 * linked != 0 the call WAITS for the first pass on the engine's stream (it
 * reads back how many blocks need the second pass and sizes it); with
 * linked == 0 it only enqueues work.  Environment knobs of the second pass
 * (read per call; for tests and measurements): MI355LZ4_LINKED_RUNS,
 * MI355LZ4_LINKED_RUNIN (0 = never, 1 = always), MI355LZ4_LINKED_RUNIN_PIECE,
 * MI355LZ4_LINKED_RUNIN_BLOCKS, MI355LZ4_LINKED_RUNIN_SPIN (polls a piece waits for the piece in front of it inside a launch),
 * MI355LZ4_LINKED_PTR, MI355LZ4_LINKED_PTR_BLOCKS, MI355LZ4_LINKED_POOL_BLOCKS,
 * MI355LZ4_LINKED_BIG (0 = never the big-block path; n = blocks from n KiB on).
 * replaces: decompressChunk, Internal/LZ4.hs:291-336. */
int mi355lz4_decompress_batch_device(mi355lz4_ctx *ctx, const uint8_t *framed, uint64_t framedLen,
                                     const uint64_t *blockOff, int nBlocks, int headerKind, int fixedUncomp,
                                     int linked, uint8_t *out, const uint64_t *outOff, const int32_t *outCap,
                                     int32_t *result);

/* Many linked streams in one call.  Stream s is the blocks
 * [streamFirst[s], streamFirst[s+1]) (device array of nStreams + 1 ascending
 * block indices); inside a stream the semantics are those of linked != 0
 * above, and no block ever sees another stream's output.  The dependency chain
 * inside a stream is serial by construction of the format, so a stream is walked
 * by one wavefront (lane-parallel inside each block) and throughput comes from
 * the number of streams in the call.
 * replaces: one decompressChunksRawD state machine per stream,
 * Internal/LZ4.hs:539-567 -> cbits/lz4.c:2322. */
int mi355lz4_decompress_streams_device(mi355lz4_ctx *ctx, const uint8_t *framed, uint64_t framedLen,
                                       const uint64_t *blockOff, int nBlocks, int headerKind, int fixedUncomp,
                                       const int32_t *streamFirst, int nStreams, uint8_t *out,
                                       const uint64_t *outOff, const int32_t *outCap, int32_t *result);

/* Read the headers of nBlocks framed blocks at blockOff[] and produce
 * outOff[0..nBlocks] = exclusive scan of their uncompressed sizes. */
int mi355lz4_index_device(mi355lz4_ctx *ctx, const uint8_t *framed, uint64_t framedLen,
                          const uint64_t *blockOff, int nBlocks, int headerKind, int fixedUncomp,
                          uint64_t *outOff);

/* Decoded sizes without decoding.  Blocks framed without an uncompressed length (headerKind 4) say nowhere what they
 * decode to; this call reads it off their token chains -- the compressed bytes and nothing else, one wavefront per block --
 * so that a caller can lay its output out densely instead of at fixedUncomp per block.  It only enqueues on the engine's
 * stream.  headerKind 8 is accepted too: the data is walked and the header's uncompLen ignored (a cross-check of headers).
 * size[i] = s >= 0 exactly when
 *   1. the chain is well formed: every token, extension byte, literal run and offset field lies inside the block's
 *      compLen bytes, and the chain ends exactly at their end with a sequence of literals only;
 *   2. the block keeps the end-of-block rules every conforming encoder keeps (cbits/lz4.c:214-221): under 13 bytes no match,
 *      the last match starts at least 12 bytes before the end, the last 5 bytes are literals;
 *   3. s <= maxUncomp;
 *   4. no offset is 0, an empty block is the one byte 0x00, and no match that has length-extension bytes and ends within
 *      the last 64 bytes of output reaches in front of the block (the code a bad offset gets there depends on the capacity).
 * Otherwise size[i] = MI355LZ4_BLK_E_SIZE_UNKNOWN; a block whose header is rejected keeps that code
 * (MI355LZ4_BLK_E_COMPLEN, MI355LZ4_BLK_E_TRUNCATED -- also when block checksums are on and the trailer lies past
 * framedLen; the checksum itself is not verified here).  Offsets are not judged beyond rule 4: whether a source lies inside
 * the block or a dictionary is the decoder's business.
 * What a size vouches for: decoding that block into a capacity of exactly size[i] gives the result and the bytes that
 * decoding it into any larger capacity gives (capacity enters the reference decoder only through its end-of-output
 * checks, cbits/lz4.c:1797-1924) -- so outCap = size, outOff = the scan is a drop-in layout for the decode calls.
 * outOff (optional, nBlocks + 1 entries) = exclusive scan of size[i] >= 0 ? size[i] : 0.
 * The call writes size[0..nBlocks) and outOff[0..nBlocks] and nothing else; framed and blockOff are never written.
 * MI355LZ4_E_ARG: null ctx, nBlocks < 0, maxUncomp < 0, a headerKind other than 4 / 8, a null framed / blockOff / size
 * with nBlocks > 0.  nBlocks == 0 is MI355LZ4_OK (outOff[0] = 0 when given). */
int mi355lz4_decoded_size_device(mi355lz4_ctx *ctx, const uint8_t *framed, uint64_t framedLen,
                                 const uint64_t *blockOff, int nBlocks, int headerKind, int maxUncomp,
                                 int32_t *size, uint64_t *outOff /* optional, nBlocks+1 */);

/* Partial decode: the first target[i] bytes of every block, for time proportional to what is asked for.
 * result[i] is what LZ4_decompress_safe_partial(data_i, out + outOff[i], compLen_i, target[i], cap_i) returns
 * (cbits/lz4.c:2179-2185: LZ4_decompress_generic in its partial mode with min(target, cap) as the output end), and
 * out[outOff[i] .. outOff[i] + result[i]) holds the bytes it writes there.  For a well-formed block of n decoded bytes
 * that is min(target[i], cap_i, n) and the prefix of the data.  A malformed block often gives a non-negative result
 * too: the partial mode stops before it reaches the damage and forgives at the output end what the full mode rejects.
 * (A match with offset 0 that the output end clips copies every byte onto itself, cbits/lz4.c:2112-2113: the bytes
 * such a block yields there are what lay in `out` before, here as in the reference.)
 * Block arguments, cap_i and header rejections are those of mi355lz4_decompress_batch_device with linked == 0; the
 * reference's partial mode has no dictionary, so there is no linked form.  target is a device array of nBlocks entries:
 * target[i] < 0 gives MI355LZ4_BLK_E_UNCOMPLEN and nothing is written, target[i] == 0 gives 0 whatever the block holds.
 * The call returns as the full decode does (per-block failures are in result[]); it only enqueues on the engine's
 * stream, waits for nothing and does not read target on the host.  Block checksums, when on, are verified over the
 * whole compressed block as in every decode call (the trailer covers the compressed bytes, not the prefix).
 * What the call may write: see the top of this header.
 * Decoder variants: the lane-parallel decoder leaves a block after the batch that reaches its target; variant 0 always
 * takes it (a partial call's work is the prefixes, which only the device knows); variant 4 gives the workgroup form the
 * blocks whose target does not cut them short and hands the others to the lane-parallel form.
 * MI355LZ4_E_ARG: null ctx, nBlocks < 0, fixedUncomp < 0, a headerKind other than 4 / 8, a null target / framed /
 * blockOff / outOff / result with nBlocks > 0, a range begun with mi355lz4_decompress_linked_begin still open.
 * nBlocks == 0 is MI355LZ4_OK. */
int mi355lz4_decompress_partial_device(mi355lz4_ctx *ctx, const uint8_t *framed, uint64_t framedLen,
                                       const uint64_t *blockOff, int nBlocks, int headerKind, int fixedUncomp,
                                       uint8_t *out, const uint64_t *outOff, const int32_t *outCap /* may be NULL */,
                                       const int32_t *target /* device, nBlocks entries */, int32_t *result);

/* The same for blocks in host memory: framed[0..len) goes to the device, mi355lz4_decoded_size_device runs over it with
 * host blockOff[], and size[0..nBlocks) (host) comes back.  Synchronous; same argument checks, same per-block codes.
 * What streamly_lz4::Engine::decodedSizes calls. */
int mi355lz4_decoded_sizes_host(mi355lz4_ctx *ctx, const uint8_t *framed, size_t len, const uint64_t *blockOff,
                                int nBlocks, int headerKind, int maxUncomp, int32_t *size);

/* ---- host-buffer batched API (what the Haskell shim binds; synchronous) -
 * A call is pipelined over groups of blocks (MI355LZ4_GROUP_MB, default 64 MiB):
 * H2D of group i+1, the kernels of group i and D2H of group i-1 overlap on
 * separate streams.  Caller buffers that are page-locked (hipHostMalloc /
 * hipHostRegister) are handed to the DMA engines directly; pageable ones are
 * staged through pinned slots by a small copy pool (MI355LZ4_COPY_THREADS).
 * A call of one or two groups has no other group to hide its staging behind:
 * its staging copies go in two pieces, the DMA engine moving one while the
 * pool copies the other (MI355LZ4_STAGE_PIECES overrides the count).  10 MiB
 * of 64 KiB blocks, decompress: 0.57 ms from pageable buffers, 0.43 ms from
 * page-locked ones (the kernel: 0.10 ms). */

/* Compress nBlocks host arrays into one dense framed stream in framedOut
 * (capacity cap).  blockFramedLen[i] (optional) = headerKind + compLen of
 * block i, so the caller can slice one Array per block like compressChunk does.
 * status[i] (optional) = compLen > 0, or 0 on failure (reference convention,
 * Internal/LZ4.hs:257-260). */
int mi355lz4_compress_batch(mi355lz4_ctx *ctx, const uint8_t *const *src, const int32_t *srcLen,
                            int nBlocks, int accel, int headerKind, uint8_t *framedOut, size_t cap,
                            size_t *outLen, int32_t *blockFramedLen, int32_t *status);

/* Walk the header chain of a dense framed stream on the host
 * (resizeChunksD's job, Internal/LZ4.hs:459-484): fills blockOff[k] and
 * uncompLen[k] for up to maxBlocks blocks; *nBlocks = blocks found.
 * MI355LZ4_E_STREAM on a malformed chain (trailing partial block). */
int mi355lz4_index_host(const uint8_t *framedIn, size_t inLen, int headerKind, int fixedUncomp,
                        uint64_t *blockOff, int32_t *uncompLen, int maxBlocks, int *nBlocks);

/* Decompress a dense framed stream held in host memory.  Output blocks are
 * written back to back into out; blockLen[k] = decoded size of block k (>= 0)
 * or its negative code.  linked as for the device call; when linked, dict /
 * dictLen (host memory, may be NULL/0) is the output of the block that preceded
 * framedIn[0] in the stream -- the array the Haskell decoder state keeps alive
 * (Internal/LZ4.hs:564) -- so a stream can be fed in several calls. */
int mi355lz4_decompress_batch(mi355lz4_ctx *ctx, const uint8_t *framedIn, size_t inLen, int headerKind,
                              int fixedUncomp, int linked, const uint8_t *dict, int dictLen, uint8_t *out,
                              size_t cap, size_t *outLen, int32_t *blockLen, int maxBlocks, int *nBlocks);

/* Partial decode of a chain in host memory: the first target[k] bytes of block k (target == NULL: targetAll bytes of
 * every block).  The chain is walked as mi355lz4_decompress_batch walks it (with the trailers when block checksums are
 * on); the prefixes come back packed back to back in out[0 .. *outLen), blockLen[k] holds block k's result
 * (mi355lz4_decompress_partial_device's result[k]).  Only the prefixes cross the link on the way back -- that is what
 * this form is for.  Synchronous, and a single group: the whole chain goes to the device, one partial decode, one copy
 * back (block by block when some block gave fewer bytes than asked); the group pipeline of the full decode is not used.
 * MI355LZ4_E_BLOCK when a block failed (blockLen[] says which), MI355LZ4_E_CAPACITY when the prefixes need more than
 * cap bytes (nothing is written then).  The multi-device handle has no partial call. */
int mi355lz4_decompress_partial(mi355lz4_ctx *ctx, const uint8_t *framedIn, size_t inLen, int headerKind,
                                int fixedUncomp, const int32_t *target /* host, one per block, or NULL */, int targetAll,
                                uint8_t *out, size_t cap, size_t *outLen, int32_t *blockLen, int maxBlocks, int *nBlocks);

/* Host-buffer form of mi355lz4_decompress_streams_device: framedIn holds the blocks
 * of nStreams linked streams back to back, stream s = blocks
 * [streamFirst[s], streamFirst[s+1]) (host array, ascending).  Blocks outside
 * every stream are decoded on their own.  Otherwise as mi355lz4_decompress_batch. */
int mi355lz4_decompress_streams(mi355lz4_ctx *ctx, const uint8_t *framedIn, size_t inLen, int headerKind,
                                int fixedUncomp, const int32_t *streamFirst, int nStreams, uint8_t *out,
                                size_t cap, size_t *outLen, int32_t *blockLen, int maxBlocks, int *nBlocks);

/* ---- several GPUs behind one handle, one process --------
 * A host caller is bound by PCIe (one link per GPU), so for the Haskell process -- one process, host buffers -- more GPUs
 * is more links.  A multi handle owns one engine per entry of devices[] (the same device may be named more than once).
 * The two calls below take the arguments of mi355lz4_compress_batch / mi355lz4_decompress_batch (independent blocks:
 * linked = 0, no dictionary) and give the same results, byte for byte: the batch is cut into one contiguous block range
 * per device (equal shares of the uncompressed bytes), every range goes through its engine's host-buffer call on a host
 * thread of its own, and the results lie in order in the caller's one buffer -- a host consumer needs no gather.
 * (Between ranks the north star's block i -> GPU i mod n is used, with a kernel on the root that interleaves the ranks'
 * outputs, gather.py; towards host memory that would make every device-to-host copy one copy per block.)
 * A handle is not thread-safe (one call at a time), like an engine.  mi355lz4_multi_last_error is thread-local.
 * replaces: compressChunk / decompressChunk, Internal/LZ4.hs:226-281, :291-336, one FFI call per batch. */
typedef struct mi355lz4_multi mi355lz4_multi;
int mi355lz4_create_multi(mi355lz4_multi **out, const int *devices, int n);
void mi355lz4_destroy_multi(mi355lz4_multi *m);
int mi355lz4_multi_device_count(const mi355lz4_multi *m);
/* engine i of the handle (e.g. for mi355lz4_set_decoder); owned by the handle */
mi355lz4_ctx *mi355lz4_multi_engine(mi355lz4_multi *m, int i);
const char *mi355lz4_multi_last_error(void);
int mi355lz4_multi_compress_batch(mi355lz4_multi *m, const uint8_t *const *src, const int32_t *srcLen, int nBlocks,
                                  int accel, int headerKind, uint8_t *framedOut, size_t cap, size_t *outLen,
                                  int32_t *blockFramedLen, int32_t *status);
int mi355lz4_multi_decompress_batch(mi355lz4_multi *m, const uint8_t *framedIn, size_t inLen, int headerKind,
                                    int fixedUncomp, uint8_t *out, size_t cap, size_t *outLen, int32_t *blockLen,
                                    int maxBlocks, int *nBlocks);

/* ---- one linked stream over several GPUs ----------
 * A linked stream does not shard by round-robin: block k's dictionary is the
 * output of block k-1 (cbits/lz4.c:2347-2355).  It shards by CONTIGUOUS RANGES:
 * engine r decodes blocks [b_r, b_r+1) and needs one thing from engine r-1, the
 * output of block b_r - 1 (the seam: at most 64 KiB of it are ever read).
 *
 * _begin issues everything that does not READ that output: the standalone pass,
 * the tolerant re-decode of the dependent blocks, source pointers and pointer
 * jumping over the range (where a byte comes from depends on tokens only).
 * _end issues the rest: the bytes are fetched from their roots, the first of
 * which lie in the seam, and the results are set.  Between the two calls the
 * caller places the seam at out + outOff[-1] (its size in result[-1]) in the
 * engine's stream order.  lookBack = 1 says outOff[-1] / result[-1] exist (the
 * arrays handed in point at their second element); lookBack = 0: the range
 * starts the stream.  Otherwise the arguments are those of
 * mi355lz4_decompress_batch_device with linked != 0, and so are the results.
 * Spread over G engines the serial part of a stream is G fetches, not G ranges
 * (streamly_lz4_amd/linked_shard.py drives it over torch.distributed).
 * A range whose dependent blocks do not fit one pointer segment
 * (MI355LZ4_LINKED_PTR_BLOCKS, default 4096 blocks of 64 KiB) is correct but
 * leaves all its work to _end. */
int mi355lz4_decompress_linked_begin(mi355lz4_ctx *ctx, const uint8_t *framed, uint64_t framedLen,
                                     const uint64_t *blockOff, int nBlocks, int headerKind, int fixedUncomp,
                                     uint8_t *out, const uint64_t *outOff, const int32_t *outCap,
                                     int32_t *result, int lookBack);
int mi355lz4_decompress_linked_end(mi355lz4_ctx *ctx);
/* Between _begin and _end: make the LAST block of the range final ahead of the others, so that it can go to the rank
 * that holds the next range while this rank's own fetch is still to run (a stream over G GPUs then waits G times for
 * one block, not for a range).  The seam -- the output of the block in front of the range (lookBack) -- must be in
 * place before this call, exactly as for _end: the fetch reads it.  Returns 1 when the last block's BYTES are final
 * after this call (the call waits for them), 0 when they are not available this way -- call _end first -- or a
 * negative MI355LZ4_E_* code.  Only the bytes are final: result[nBlocks-1] keeps the first pass's code until _end has
 * run, so take the block's size from its header (or from the capacity handed in), not from result[].  _end must still
 * be called.  (Reference semantics as for _begin: cbits/lz4.c:2347-2355.) */
int mi355lz4_decompress_linked_end_last(mi355lz4_ctx *ctx);

/* ---- synthetic inputs (bench / test support; SURVEY.md 8d generators) ---
 * kind: 0 = xorshift64* random, 1 = lzsynth(litMax, offMax), 2 = text-like.
 * Block i of the batch is seeded by (firstBlock + i * blockStep); it is written
 * at dst + i*blockLen.  dst is a device pointer. */
int mi355lz4_generate_device(mi355lz4_ctx *ctx, int kind, uint8_t *dst, int blockLen, int nBlocks,
                             uint64_t firstBlock, uint64_t blockStep, uint32_t litMax, uint32_t offMax);

/* ---- ordered multi-GPU gather support -------------------
 * Scatter rank-local dense blocks into the global stream on the root:
 * local block j of rank g (nRanks ranks, round-robin) is global block
 * j*nRanks+g; its bytes local[localOff[j] .. localOff[j+1]) are copied to
 * global + globalOff[j*nRanks+g].  All pointers are device pointers. */
int mi355lz4_interleave_device(mi355lz4_ctx *ctx, const uint8_t *local, const uint64_t *localOff,
                               int nLocalBlocks, int rank, int nRanks, uint8_t *global,
                               const uint64_t *globalOff);

/* ---- block checksums (Streamly.Internal.LZ4.Config setBlockChecksum, Config.hs:118-158) ----------------
 * With the switch on, every framed block carries a 4-byte trailer behind its data:
 *   [compLen][uncompLen (headerKind 8)][compLen bytes][xxh32 of those bytes, seed 0, little-endian]
 * -- with headerKind 4, byte for byte an LZ4 frame block with B.Checksum set.  compLen does not count the trailer.
 * on != 0:
 *   compress calls (_compress_batch_device, _compress_batch; linked or not) append the trailer: framedLen[i] and
 *   blockFramedLen[i] include it, the data bytes are those of the same call with the switch off, and the device call
 *   needs slotStride >= LZ4_compressBound(maxBlockLen) + headerKind + 4 (mi355lz4_slot_stride_ex) or returns
 *   MI355LZ4_E_CAPACITY;
 *   every decode call (_decompress_batch_device, _decompress_streams_device, _decompress_linked_begin / _end / _end_last,
 *   _decompress_batch, _decompress_streams, _decompress_dstreams_device, _decompress_dstreams) expects the trailer: each block's data is hashed on the device before the block
 *   is decoded; a trailer that lies past the framed buffer gives MI355LZ4_BLK_E_TRUNCATED, a mismatch
 *   MI355LZ4_BLK_E_CHECKSUM (the call returns MI355LZ4_E_BLOCK).  Such a block is a header-rejected block: in a linked
 *   stream the block after it sees what it sees after any rejected block.  The host-buffer calls walk the chain with the
 *   trailers (mi355lz4_index_host_ex).
 * Default off.  mi355lz4_index_device and the legacy face (include/lz4.h) do not look at it. */
int mi355lz4_set_block_checksum(mi355lz4_ctx *ctx, int on);
/* Compression level of the engine's compress calls (_compress_batch_device, _compress_batch, the frame and legacy faces
 * that go through them; linked or not, block checksums or not):
 *   0      the default: the fast encoder, `accel` as in LZ4_compress_fast; its output is unchanged by this call;
 *   1..9   the hash-chain encoder (LZ4HC's levels): every position's longest match within 2^(level-1) chain steps, a
 *          one-step lazy parse; smaller output, slower; `accel` is ignored.  Deterministic, plain LZ4 blocks that
 *          every decoder reads; linked compression uses the same dictionary as level 0;
 *   10..12 accepted, searched as 9 (mi355lz4_get_compression_level then returns 9).
 * At every level mi355lz4_compress_batch_device only enqueues: the hash-chain encoder is one launch on the engine's stream and
 * reads no length on the host.
 * Anything else, or a null ctx: MI355LZ4_E_ARG.  The multi handle's compress call needs its engines to agree. */
int mi355lz4_set_compression_level(mi355lz4_ctx *ctx, int level);
/* The effective level (0..9), or MI355LZ4_E_ARG for a null ctx. */
int mi355lz4_get_compression_level(const mi355lz4_ctx *ctx);
/* Reference-exact compression.  While on, the ctx holds ONE compress stream -- the device counterpart of LZ4_stream_t --
 * and every _compress_batch / _compress_batch_device call appends its blocks to it, in order: block i's bytes are those of
 * LZ4_compress_fast_continue on one stream over separately allocated arrays (the external-dictionary path, as
 * Streamly.Internal.LZ4's compressChunksD drives it), whatever `accel` (clamped to 1..65537), lengths (0 up to
 * LZ4_MAX_INPUT_SIZE) or placement in memory; across calls, through the 2 GiB renormalisation.  The engine keeps its own
 * copy of the table, the offsets and the previous array's last 64 KiB: the caller may free a call's buffers.
 * Header kinds 4 / 8, block checksums, compaction and the pipelined host call work unchanged; the linked switch
 * (mi355lz4_set_linked_compress) is ignored; frames (lz4FrameCompress) and the legacy face do not use the stream.
 * The device call waits on the engine's stream (it reads the lengths, and its verify step decides which speculated
 * pieces are redone).  Refused with MI355LZ4_E_ARG at the compress call: a compression level other than 0, forced
 * segments (mi355lz4_set_segments k > 0); the multi handle refuses engines in this mode.
 * Switching it on starts a new stream; default off, and off nothing changes.  MI355LZ4_EXACT_RUNIN=R (default 12; 0: one
 * serial chain) and MI355LZ4_EXACT_PIECE=P (default max(4, blocks / 2048)) set the speculation, read per call. */
int mi355lz4_set_compress_exact(mi355lz4_ctx *ctx, int on);
/* 1 while the mode is on, 0 off, MI355LZ4_E_ARG for a null ctx. */
int mi355lz4_get_compress_exact(const mi355lz4_ctx *ctx);
/* Start a new exact stream (LZ4_createStream): the next call's first block has no dictionary and a zeroed table. */
int mi355lz4_compress_exact_reset(mi355lz4_ctx *ctx);
/* ---- many reference-exact streams in one call ------------------------------------------------------------------------
 * The compress-side counterpart of mi355lz4_decompress_streams_device: a host that runs many pipelines at once (files,
 * connections, shards) keeps one slot per pipeline and compresses the next arrays of all of them in ONE call.
 *
 * A mi355lz4_cstreams is an opaque set of nSlots device-resident compress streams, owned by the caller and bound to the
 * device of the engine it was created with (any engine on that device may use it; one call at a time).  One slot holds
 * everything LZ4_stream_t holds, all of it on the device: the 4096-entry table, the previous array's last 64 KiB,
 * currentOffset, dictSize and the number of saved dictionary bytes -- 81984 bytes, about 80 KiB a slot (2560 slots:
 * 200 MiB).  Nothing of a slot lives on the host, which is what lets the device call return without waiting.
 * _create leaves every slot reset; _reset is LZ4_resetStream for slots[0..n) (slots == NULL: all of them), enqueued on the
 * engine's stream; _destroy waits for the device. */
typedef struct mi355lz4_cstreams mi355lz4_cstreams;
int mi355lz4_cstreams_create(mi355lz4_ctx *ctx, int nSlots, mi355lz4_cstreams **out);
void mi355lz4_cstreams_destroy(mi355lz4_cstreams *cs);
int mi355lz4_cstreams_count(const mi355lz4_cstreams *cs);
int mi355lz4_cstreams_reset(mi355lz4_ctx *ctx, mi355lz4_cstreams *cs, const int32_t *slots, int n);
/* Compress nBlocks blocks that belong to nStreams streams.  The block arguments and the outputs are those of
 * mi355lz4_compress_batch_device (slotStride as mi355lz4_slot_stride_ex says).  Stream s of the call is the blocks
 * [streamFirst[s], streamFirst[s+1]) and continues the state in slot streamSlot[s]; an empty stream leaves its slot
 * untouched.  streamFirst (nStreams + 1 entries, streamFirst[0] == 0, streamFirst[nStreams] == nBlocks, ascending) and
 * streamSlot are small HOST arrays, checked before anything is enqueued and used up before the call returns.
 * MI355LZ4_E_ARG: a table that is not ascending or does not cover the blocks, a slot out of range, the same slot twice in
 * one call, `cs` created on another device, a compression level other than 0.
 * Bytes: every stream's blocks are what LZ4_compress_fast_continue writes on one LZ4_stream_t over separately allocated
 * arrays (the external-dictionary path, the reference's compressChunksD), for any accel (clamped to 1..65537), lengths
 * 0..maxBlockLen and placement in memory, across calls and through the 2 GiB renormalisation: a stream given in one call
 * and the same stream given one block per call give the same bytes.  A block's dictionary is the array before it IN ITS
 * STREAM -- for a stream's first block in a call, the tail the slot saved -- so a call's source may be overwritten or
 * freed once the call has run.
 * Asynchronous: the call only enqueues on the engine's stream; it does not read srcLen on the host and does not wait
 * (beyond four calls in flight, for the oldest one's stream table).  A length outside 0..maxBlockLen can therefore be no
 * error code: the stream's wavefront stops there, that block and the rest of that stream's blocks in the call get
 * framedLen = 0 (no valid block has 0: a zero-length array is the header plus one byte), the slot stays as it was after
 * the last good block, and the other streams are unaffected.
 * Switches: block checksums apply; the compression level must be 0; the linked switch and segments are ignored.  The
 * engine's own exact stream (mi355lz4_set_compress_exact) is separate state that this call never touches, on or off.
 * One wavefront walks one stream: throughput comes from the number of streams in the call (the chip runs 2560 at a
 * time), and a stream with many blocks in one call is one serial chain of about 11 ms per 64 KiB block -- a single
 * long stream belongs in mi355lz4_set_compress_exact, which speculates. */
int mi355lz4_compress_streams_device(mi355lz4_ctx *ctx, mi355lz4_cstreams *cs, const uint8_t *src,
                                     const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride,
                                     int maxBlockLen, int nBlocks, const int32_t *streamFirst,
                                     const int32_t *streamSlot, int nStreams, int accel, int headerKind,
                                     uint8_t *slots, size_t slotStride, int32_t *framedLen);
/* Host-buffer form: as mi355lz4_compress_batch (one dense framed stream in block order, blockFramedLen and status per
 * block, synchronous, the same group pipeline; a group seam inside a stream continues its slot).  The lengths are checked
 * on the host: a bad one is MI355LZ4_E_ARG and nothing is enqueued. */
int mi355lz4_compress_streams(mi355lz4_ctx *ctx, mi355lz4_cstreams *cs, const uint8_t *const *src,
                              const int32_t *srcLen, int nBlocks, const int32_t *streamFirst,
                              const int32_t *streamSlot, int nStreams, int accel, int headerKind, uint8_t *framedOut,
                              size_t cap, size_t *outLen, int32_t *blockFramedLen, int32_t *status);

/* ---- shared-dictionary batches: LZ4_loadDict and LZ4_decompress_safe_usingDict ------------------------------------------
 * Small records (rows, log lines, messages, pages of 1-16 KiB) compress poorly on their own, because every block starts with
 * an empty window; the codec's answer is one dictionary shared by all of them.  Here a slot of a mi355lz4_cstreams is loaded
 * once and then serves any number of batches, read-only; the decode side takes the dictionary's bytes directly.
 *
 * _cstreams_load_dict is LZ4_loadDict (cbits/lz4.c:1475-1515) on slot `slot`, on the device: afterwards the slot holds what
 * LZ4_loadDict leaves in an LZ4_stream_t -- the table zeroed, currentOffset 65536 and, for len >= 8 (HASH_UNIT of the
 * reference's 64-bit build), the last min(len, 65536) bytes of dictDevice[0, len) saved with dictSize their count and every
 * third position p <= dictEnd - 8 of those bytes entered with index p - (dictEnd - 65536) under the byU32 hash5, the last
 * writer of a bucket winning.  len < 8: no dictionary and an empty table, but currentOffset is 65536 all the same.  The
 * call only enqueues on the engine's stream and reads nothing on the host; the slot keeps its own copy, so dictDevice may be
 * freed or overwritten once the call has run on the device.  A slot loaded this way continues through
 * mi355lz4_compress_streams_device unchanged: LZ4_loadDict followed by LZ4_compress_fast_continue over separately allocated
 * arrays.
 * MI355LZ4_E_ARG: a null ctx or cs, a slot out of range, len < 0, a null dictDevice with len > 0, `cs` created on another
 * device. */
int mi355lz4_cstreams_load_dict(mi355lz4_ctx *ctx, mi355lz4_cstreams *cs, int slot, const uint8_t *dictDevice, int len);
/* Compress nBlocks independent blocks, every one against the state in slot dictSlot of `cs`.  The block arguments and the
 * outputs are those of mi355lz4_compress_batch_device (slotStride as mi355lz4_slot_stride_ex says).
 * Bytes: block i is what LZ4_compress_fast_continue(&copy, src_i, dst, n_i, LZ4_compressBound(n_i), accel) writes on a COPY
 * of the slot's LZ4_stream_t, for any accel (clamped to 1..65537) and any length 0..maxBlockLen -- after
 * _cstreams_load_dict, the reference's LZ4_loadDict once and a copy of the loaded stream per block.  The state is whatever
 * the slot holds: a slot that streams have continued works the same way (its last array's tail is the dictionary).
 * The slot is never written and blocks do not see each other: the same slot may serve any number of calls, from any
 * engine on its device, also at the same time -- as long as no call that WRITES the slot (_load_dict, _reset,
 * _compress_streams_device naming it) is in flight beside them.
 * Asynchronous: the call only enqueues on the engine's stream; it does not wait and does not read srcLen on the host.  A
 * length outside 0..maxBlockLen can therefore be no error code: that block gets framedLen[i] = 0 and its slot range is left
 * untouched, as in the streams call; the other blocks are unaffected.
 * Switches: block checksums apply; the compression level must be 0 (levels 1..12: mi355lz4_compress_hcdict_device).  Segments, the linked switch and the engine's own exact
 * stream (mi355lz4_set_compress_exact) play no part, on or off.
 * MI355LZ4_E_ARG: a null ctx or cs, `cs` created on another device, a compression level other than 0, dictSlot out of
 * range, nBlocks < 0, a headerKind other than 4 / 8, maxBlockLen outside 0..MI355LZ4_MAX_INPUT_SIZE, with nBlocks > 0 a null
 * src (maxBlockLen > 0), slots or framedLen.  MI355LZ4_E_CAPACITY: slotStride below the bound.  nBlocks == 0 is MI355LZ4_OK.
 * One wavefront per block, the reference's serial parse: 6.9 ms for 16384 text records of 4 KiB against a 64 KiB dictionary
 * (ratio 1.90; mi355lz4_compress_batch_device: 0.39 ms, ratio 1.33), 28.9 ms for 2560 records of 64 KiB (scripts/dict_rate.py,
 * profiles/dict_rate.json). */
int mi355lz4_compress_dict_device(mi355lz4_ctx *ctx, const mi355lz4_cstreams *cs, int dictSlot, const uint8_t *src,
                                  const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride, int maxBlockLen,
                                  int nBlocks, int accel, int headerKind, uint8_t *slots, size_t slotStride,
                                  int32_t *framedLen);
/* Decode nBlocks independent blocks, every one against the dictionary dictDevice[0, dictLen) (device memory, any length).
 * result[i] and out[outOff[i] ..) are those of LZ4_decompress_safe_usingDict(data_i, dst_i, compLen_i, cap_i, dict, dictLen)
 * on its external-dictionary path (LZ4_decompress_safe_forceExtDict, cbits/lz4.c:2404-2417), for well-formed and malformed
 * blocks alike (tests/test_seam_decode_gpu.py holds the call to it on hand-built and corrupted blocks): only the last 64 KiB of the dictionary can be reached, and a dictionary under 64 KiB arms the offset check
 * (:1764).  The prefix mode the reference takes when a destination happens to lie directly behind the dictionary is not
 * restated, here or elsewhere in this engine: wherever the outputs lie, the dictionary is external.  dictLen == 0 is
 * LZ4_decompress_safe: the results of mi355lz4_decompress_batch_device with linked == 0.
 * Block arguments, cap_i, the header rejections, checksum verification and what the call may write are those of
 * mi355lz4_decompress_batch_device with linked == 0.  The dictionary is never written.
 * Enqueue only: every block is decoded once, with the dictionary -- no standalone first pass, no second pass, no host wait;
 * per-block failures are in result[].  mi355lz4_set_decoder is ignored by this call: the workgroup-per-block form has no
 * dictionary, so every block takes the lane-parallel decoder, one wavefront per block.
 * MI355LZ4_E_ARG: null ctx, nBlocks < 0, fixedUncomp < 0, a headerKind other than 4 / 8, dictLen < 0, a null dictDevice with
 * dictLen > 0, a null framed / blockOff / outOff / result with nBlocks > 0, a range begun with
 * mi355lz4_decompress_linked_begin still open.  nBlocks == 0 is MI355LZ4_OK.
 * Rates: 0.22 ms for 16384 blocks of 4 KiB, 0.47 ms for 2560 of 64 KiB, text against a 64 KiB dictionary (the same blocks
 * without one through mi355lz4_decompress_batch_device: 0.18 and 0.40 ms; scripts/dict_rate.py, profiles/dict_rate.json). */
int mi355lz4_decompress_dict_device(mi355lz4_ctx *ctx, const uint8_t *framed, uint64_t framedLen, const uint64_t *blockOff,
                                    int nBlocks, int headerKind, int fixedUncomp, const uint8_t *dictDevice, int dictLen,
                                    uint8_t *out, const uint64_t *outOff, const int32_t *outCap /* may be NULL */,
                                    int32_t *result);
/* Host-buffer forms, synchronous.  _compress_dict: as mi355lz4_compress_batch (one dense framed stream in block order,
 * blockFramedLen and status per block, the same group pipeline), every block against slot dictSlot of `cs`; the lengths are
 * checked on the host, a bad one is MI355LZ4_E_ARG and nothing is enqueued.  _decompress_dict: as mi355lz4_decompress_batch
 * with a host dictionary (dict, dictLen; may be NULL / 0) in place of linked / dict; a single group, as
 * mi355lz4_decompress_partial is: the whole chain and the dictionary's last 64 KiB go to the device, one decode, one copy
 * back -- the group pipeline of the full decode is not used.  The multi-device handle and the legacy LZ4_* face have no
 * dictionary calls. */
int mi355lz4_compress_dict(mi355lz4_ctx *ctx, const mi355lz4_cstreams *cs, int dictSlot, const uint8_t *const *src,
                           const int32_t *srcLen, int nBlocks, int accel, int headerKind, uint8_t *framedOut, size_t cap,
                           size_t *outLen, int32_t *blockFramedLen, int32_t *status);
int mi355lz4_decompress_dict(mi355lz4_ctx *ctx, const uint8_t *framedIn, size_t inLen, int headerKind, int fixedUncomp,
                             const uint8_t *dict, int dictLen, uint8_t *out, size_t cap, size_t *outLen, int32_t *blockLen,
                             int maxBlocks, int *nBlocks);

/* ---- high-compression levels against a shared dictionary: lz4 -9 -D dict ----------------------------------------------------
 * mi355lz4_compress_dict_device is level 0's encoder.  These calls are the hash-chain encoder of levels 1..12
 * (mi355lz4_set_compression_level) with one dictionary in front of every block of a batch: LZ4_loadDictHC once, then
 * LZ4_compress_HC_continue on a copy of the loaded stream per block, in this engine's own parse -- the blocks are plain LZ4
 * (mi355lz4_decompress_dict_device and LZ4_decompress_safe_usingDict read them with the dictionary) but not liblz4's bytes.
 *
 * A mi355lz4_hcdict is an opaque prepared dictionary on the device of the engine it was created with, about 216 KiB: its own
 * copy of the dictionary's last keep = min(len, 65536) bytes and the image of the encoder's tables (the chain ring, 65536 x
 * u16, and the head table) as they are after the inserts of window positions [0, keep - 3) of those bytes alone -- the
 * positions whose four bytes lie inside the dictionary; window position 0 is the first kept byte.  The encoder reloads the
 * image for every block instead of inserting up to 64 KiB of dictionary again.
 * _hcdict_create allocates an object that holds the empty dictionary (no kernel).  _hcdict_load builds the image from
 * dictDevice[0, len) (device memory; len == 0 is legal, under 4 bytes no position is inserted): one workgroup, enqueued on the
 * engine's stream, nothing read on the host; the object keeps its own copy, so dictDevice may be freed or overwritten once the
 * call has run on the device.  Loading again replaces the image.  _hcdict_size: the bytes the last _load kept (0 before the
 * first).  _hcdict_destroy waits for the device first.  Compress calls only read the object: it may serve any number of
 * calls, from any engine on its device, also at the same time -- as long as no _hcdict_load is in flight beside them (the
 * sharing rule of a loaded mi355lz4_cstreams slot).
 * MI355LZ4_E_ARG: _create: a null ctx or out; _load: a null ctx or hd, `hd` created on another device, len < 0, a null
 * dictDevice with len > 0; _size: a null hd. */
typedef struct mi355lz4_hcdict mi355lz4_hcdict;
int mi355lz4_hcdict_create(mi355lz4_ctx *ctx, mi355lz4_hcdict **out);
void mi355lz4_hcdict_destroy(mi355lz4_hcdict *hd);
int mi355lz4_hcdict_load(mi355lz4_ctx *ctx, mi355lz4_hcdict *hd, const uint8_t *dictDevice, int len);
int mi355lz4_hcdict_size(const mi355lz4_hcdict *hd);
/* Compress nBlocks independent blocks at the engine's compression level (1..12; depth 2^(min(level, 9) - 1), as every HC call),
 * every one with the dictionary of `hd` in front of it.  Block arguments, outputs, headers (4 / 8), trailers
 * (mi355lz4_set_block_checksum) and slotStride (mi355lz4_slot_stride_ex) are those of mi355lz4_compress_dict_device; there is
 * no accel (the HC levels ignore it).
 * Bytes: block i is exactly what this engine writes for it when the dictionary's kept bytes lie directly in front of the block
 * in memory -- the second block of the two-block linked call [D[-65536:], B] through mi355lz4_compress_batch_device at the same
 * level; with an empty dictionary, mi355lz4_compress_batch_device's block at that level.  A match may start in the dictionary
 * and run on into the block's own bytes.
 * Asynchronous: the call only enqueues on the engine's stream and does not read srcLen on the host.  A length outside
 * 0..maxBlockLen gives framedLen[i] = 0 and an untouched slot range; the other blocks are unaffected.
 * Switches: the level must be 1..12 -- level 0 against a dictionary is mi355lz4_compress_dict_device.  Segments, the linked
 * switch and the engine's exact stream play no part, on or off.
 * maxBlockLen is at most 4 MiB (the largest block size of the reference's BlockSize): a shared dictionary is for small records,
 * and every workgroup of the launch stages the dictionary and its current block contiguously in engine-owned scratch
 * (65536 + maxBlockLen bytes a workgroup, one workgroup per CU).
 * MI355LZ4_E_ARG: a null ctx or hd, `hd` created on another device, compression level 0, nBlocks < 0, a headerKind other than
 * 4 / 8, maxBlockLen outside 0..4 MiB, with nBlocks > 0 a null src (maxBlockLen > 0), slots or framedLen.
 * MI355LZ4_E_CAPACITY: slotStride below the bound.  nBlocks == 0 is MI355LZ4_OK.
 * One workgroup of 1024 threads per block, as the HC levels without a dictionary: a poor fit for 4 KiB records.  Measured once
 * (scripts/hcdict_rate.py, profiles/hcdict_rate.json; medians of 5 event-timed calls): 16384 text records of 4 KiB against a
 * 64 KiB dictionary at level 9 in 28.3 ms, ratio 2.44 (level 3: 12.4 ms, 2.16; mi355lz4_compress_dict_device: 6.9 ms, 1.90;
 * level 9 without a dictionary: 8.6 ms, 1.37); 2560 records of 64 KiB at level 9 in 69.8 ms, ratio 2.44 (level 0 with the
 * dictionary: 28.8 ms, 1.88; level 9 without: 52.3 ms, 2.12).  _hcdict_load of 64 KiB: 0.8 ms (0.91 ms since it also builds the wave
 * encoder's image, profiles/fastdict_rate.json). */
int mi355lz4_compress_hcdict_device(mi355lz4_ctx *ctx, const mi355lz4_hcdict *hd, const uint8_t *src,
                                    const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride, int maxBlockLen,
                                    int nBlocks, int headerKind, uint8_t *slots, size_t slotStride, int32_t *framedLen);
/* Host-buffer form, synchronous: as mi355lz4_compress_dict (one dense framed stream in block order, blockFramedLen and status per
 * block, the same group pipeline) with the device call above per group.  The lengths are checked on the host: one outside
 * 0..4 MiB is MI355LZ4_E_ARG and nothing is enqueued or written.  The multi-device handle and the legacy LZ4_* face have no
 * such call. */
int mi355lz4_compress_hcdict(mi355lz4_ctx *ctx, const mi355lz4_hcdict *hd, const uint8_t *const *src,
                             const int32_t *srcLen, int nBlocks, int headerKind, uint8_t *framedOut, size_t cap,
                             size_t *outLen, int32_t *blockFramedLen, int32_t *status);

/* ---- level 0 against the same prepared dictionary, fast: the wave encoder -------------------------------------------------------
 * mi355lz4_compress_dict_device gives the reference's bytes and pays for them with the reference's serial parse.  These calls
 * give the engine's own level-0 parse instead -- the encoder of mi355lz4_compress_batch_device, 64 positions a step -- against the
 * dictionary of a mi355lz4_hcdict: one object, loaded once, serves every level.  Beside the image above the object holds the wave
 * encoder's table (4096 16-bit positions and their tags, 10240 bytes, and a 16-byte header) as it is after the dictionary's seed
 * steps; _hcdict_load builds it with a second kernel of one wavefront, and the encoder reloads it for every block instead of
 * seeding up to 64 KiB again.  DESIGN.md 7l.
 *
 * Block arguments, outputs, headers (4 / 8), trailers (mi355lz4_set_block_checksum), the slotStride bound
 * (mi355lz4_slot_stride_ex), framedLen, the error codes and the 4 MiB limit on maxBlockLen are those of
 * mi355lz4_compress_hcdict_device; accel is added, clamped to 1..65537 as in mi355lz4_compress_batch_device.
 * Bytes: with keep = min(len, 65536) the bytes the last _hcdict_load kept, block i is exactly what this engine writes for it as
 * the second block of the two-block linked call [D[-keep:], B_i] -- mi355lz4_compress_batch_device at level 0 with
 * mi355lz4_set_linked_compress(1), the same accel, and max(keep, maxBlockLen) as its maxBlockLen (so the encoder's form for blocks
 * above 64 KiB is taken exactly when this call's maxBlockLen is above 65536).  With keep == 0, block i is the block of the one-block
 * call with the linked switch on.  Blocks under 13 bytes are literals only; an empty block is the single zero token.  The output
 * is a plain LZ4 block: mi355lz4_decompress_dict_device and LZ4_decompress_safe_usingDict read it with the dictionary.  These are
 * not liblz4's bytes.
 * Asynchronous: the call only enqueues on the engine's stream and does not read srcLen on the host.  A length outside
 * 0..maxBlockLen gives framedLen[i] = 0 and an untouched slot range; the other blocks are unaffected.
 * Switches: the level must be 0 (levels 1..12 against a dictionary are mi355lz4_compress_hcdict_device).  Segments, the linked switch
 * and the engine's exact stream play no part, on or off.
 * A persistent grid of single wavefronts, 16 a CU as mi355lz4_compress_batch_device has them; every wave stages the dictionary and
 * its current block contiguously in engine-owned scratch (65536 + maxBlockLen bytes a wave, at most 1 GiB a call: the grid shrinks
 * to fit).  MI355LZ4_FASTDICT_WAVES (read per call; tests and measurements): n > 0 waves per CU, n < 0 a grid of -n waves in all.
 * MI355LZ4_E_ARG: a null ctx or hd, `hd` created on another device, a compression level other than 0, nBlocks < 0, a headerKind
 * other than 4 / 8, maxBlockLen outside 0..4 MiB, with nBlocks > 0 a null src (maxBlockLen > 0), slots or framedLen.
 * MI355LZ4_E_CAPACITY: slotStride below the bound.  nBlocks == 0 is MI355LZ4_OK.
 * Measured once (scripts/fastdict_rate.py, profiles/fastdict_rate.json; one session, medians of 5 event-timed calls): 16384 text
 * records of 4 KiB against a 64 KiB dictionary in 0.60 ms, ratio 1.92 (mi355lz4_compress_dict_device: 6.84 ms, 1.90, its fastest call
 * 6.82 ms; mi355lz4_compress_hcdict_device level 3: 12.18 ms, 2.16; mi355lz4_compress_batch_device without a dictionary: 0.39 ms, 1.33);
 * 2560 records of 64 KiB in 1.47 ms, ratio 1.93 (28.53 ms, 1.88; level 3: 29.58 ms, 2.16; without a dictionary: 1.62 ms, 1.82).  4 / 8 / 16
 * waves a CU: 1.42 / 0.82 / 0.61 ms on the 4 KiB shape, so 16 is the default.  _hcdict_load of 64 KiB, both images: 0.91 ms. */
int mi355lz4_compress_fastdict_device(mi355lz4_ctx *ctx, const mi355lz4_hcdict *hd, const uint8_t *src,
                                      const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride, int maxBlockLen,
                                      int nBlocks, int accel, int headerKind, uint8_t *slots, size_t slotStride,
                                      int32_t *framedLen);
/* Host-buffer form, synchronous: as mi355lz4_compress_hcdict (the same group pipeline) with the device call above per group.  The
 * lengths are checked on the host: one outside 0..4 MiB is MI355LZ4_E_ARG and nothing is enqueued or written.  The multi-device
 * handle and the legacy LZ4_* face have no such call. */
int mi355lz4_compress_fastdict(mi355lz4_ctx *ctx, const mi355lz4_hcdict *hd, const uint8_t *const *src,
                               const int32_t *srcLen, int nBlocks, int accel, int headerKind, uint8_t *framedOut, size_t cap,
                               size_t *outLen, int32_t *blockFramedLen, int32_t *status);

/* ---- dictionary sets: a batch in which every block names its dictionary ---------------------------------------------------------
 * The calls above take one dictionary.  A store of small records has one per table, column, tenant or message type, and under
 * those calls its batch falls apart into one call per dictionary, a few hundred blocks each -- the shape this engine is worst at.
 * These calls take a SET of prepared dictionaries and, per block, an index into it.  Level 0's wave encoder
 * (mi355lz4_compress_fastdict_device) and the dictionary decoder (mi355lz4_decompress_dict_device) have the form; the HC levels,
 * the reference-exact mi355lz4_compress_dict_device, the page calls, the multi-device handle and the legacy LZ4_* face do not.
 * DESIGN.md 7o.
 *
 * A mi355lz4_dictset is an opaque table on the device of the engine it was created with: n entries, 1 <= n <= 65536, one per
 * member, each the member's two images by address.  _dictset_create uploads it (and waits for that copy).  The members are
 * BORROWED: the set neither copies nor owns them, they must outlive it, and destroying a member before the set is the caller's
 * error -- calls through the set would read freed memory.  The same object may stand at several indices.  mi355lz4_hcdict_load on a
 * member rebuilds its images in place, so the set sees the new dictionary without being recreated; the sharing rule is that of a
 * single mi355lz4_hcdict: no _hcdict_load of a member may be in flight beside a call that reads the set.  Calls only read the set
 * (but for two diagnostic words of the compress call), so it may serve any number of calls.  _dictset_destroy waits for the device
 * first, as _hcdict_destroy does, and leaves the members alone.  _dictset_count: n.
 * MI355LZ4_E_ARG: _create: a null ctx, hd or out, n outside 1..65536, a null member, a member created on another device than the
 * engine's; _count: a null set. */
typedef struct mi355lz4_dictset mi355lz4_dictset;
int mi355lz4_dictset_create(mi355lz4_ctx *ctx, const mi355lz4_hcdict *const *hd, int n, mi355lz4_dictset **out);
void mi355lz4_dictset_destroy(mi355lz4_dictset *ds);
int mi355lz4_dictset_count(const mi355lz4_dictset *ds);
/* mi355lz4_compress_fastdict_device with `ds` in place of the dictionary and dictIdx[0, nBlocks) (device memory) beside the blocks.
 * With k = dictIdx[i]: for k in 0..n-1 the slot bytes, header, trailer and framedLen[i] of block i are exactly what
 * mi355lz4_compress_fastdict_device writes for that block alone against member k, with the same accel, maxBlockLen, headerKind and
 * checksum switch; k == -1 is no dictionary: that call's bytes against an object that holds the empty dictionary.  Any other k
 * gives framedLen[i] = 0 and an untouched slot range, like a length outside 0..maxBlockLen; the other blocks are unaffected.
 * The level (0), the switches, the 4 MiB limit, slotStride and the error codes are those of mi355lz4_compress_fastdict_device, with
 * a null ds or dictIdx (nBlocks > 0) and a set created on another device as further MI355LZ4_E_ARG.  Enqueue only: nothing of
 * dictIdx or srcLen is read on the host.
 * How: a grouping pass on the device (a histogram of dictIdx, a scan, a scatter: four small launches, scratch of the engine's) orders
 * the blocks by member; then mi355lz4_compress_fastdict_device's grid of single wavefronts and staging windows, wave w taking the
 * w-th of `grid` equal parts of that order.  A wave stages a dictionary when its next block names another member than its window
 * holds, so a call stages at most grid + G - 1 times for G distinct indices, where one call per dictionary would stage grid times
 * each.  Equal block counts per wave: lengths that go with the dictionary can unbalance the waves (byte-weighted parts are not
 * built).  MI355LZ4_FASTDICT_WAVES applies as it does there.
 * Measured once (scripts/dictset_rate.py, profiles/dictset_rate.json; one session, medians of 5 event-timed calls after a warm-up, the
 * forms alternated): 16384 text records of 4 KiB, 64 members of 64 KiB, 256 records a member.  One call with the members' records
 * shuffled through the batch: 0.74 ms (4096 stagings by 4096 waves); 64 mi355lz4_compress_fastdict_device calls of 256 records back
 * to back: 6.83 ms -- the five values of each lie apart.  Sorted by member: 0.84 ms against 0.62 ms for one single-dictionary call
 * over all records, so the grouping pass and the indirection cost 0.22 ms, a factor 1.35.  Lengths that go with the member (32
 * members with 1 KiB records, 32 with 16 KiB records, the same 64 MiB): 3.04 ms against 0.79 ms for one single-dictionary call on the
 * same lengths, a factor 3.85 -- what equal block counts per wave cost there. */
int mi355lz4_compress_fastdict_multi_device(mi355lz4_ctx *ctx, const mi355lz4_dictset *ds, const int32_t *dictIdx,
                                            const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                            uint64_t blockStride, int maxBlockLen, int nBlocks, int accel, int headerKind,
                                            uint8_t *slots, size_t slotStride, int32_t *framedLen);
/* Host-buffer form, synchronous: mi355lz4_compress_fastdict's group pipeline with the device call above per group; dictIdx is host
 * memory, nBlocks entries, and each group's part of it goes to the device with its lengths.  dictIdx and the lengths are checked on
 * the host before anything is queued: an index outside -1..n-1 or a length outside 0..4 MiB is MI355LZ4_E_ARG, nothing is enqueued
 * or written, and *outLen is 0. */
int mi355lz4_compress_fastdict_multi(mi355lz4_ctx *ctx, const mi355lz4_dictset *ds, const int32_t *dictIdx,
                                     const uint8_t *const *src, const int32_t *srcLen, int nBlocks, int accel, int headerKind,
                                     uint8_t *framedOut, size_t cap, size_t *outLen, int32_t *blockFramedLen, int32_t *status);
/* mi355lz4_decompress_dict_device with (ds, dictIdx) in place of (dictDevice, dictLen); dictIdx[0, nBlocks) is device memory.
 * With k = dictIdx[i]: for k in 0..n-1, result[i] and the bytes written for block i are those of mi355lz4_decompress_dict_device
 * on that block with member k's kept bytes -- the last keep = min(len, 65536) bytes of what was loaded -- as the dictionary, for
 * well-formed and malformed blocks alike.  Only the last 64 KiB of a dictionary can be reached and a dictionary of 65536 bytes
 * leaves the offset check unarmed as a longer one does, so this is also the result against the dictionary that was loaded.
 * k == -1 is dictLen == 0.  Any other k gives result[i] = MI355LZ4_BLK_E_DICT, and nothing is read or written for that block.
 * Header rejections, cap_i, checksum verification, what the call may write, the errors and the enqueue-only rule are those of
 * mi355lz4_decompress_dict_device, with a null ds or dictIdx (nBlocks > 0) and a set created on another device as further
 * MI355LZ4_E_ARG.  One wavefront per block, the member's bytes read in place: nothing is staged and nothing is grouped.
 * Measured once (the same script and shape): one call with shuffled indices 0.27 ms; 64 mi355lz4_decompress_dict_device calls of 256
 * blocks back to back 3.03 ms, the five values of each apart; one such call over all blocks against one dictionary 0.26 ms. */
int mi355lz4_decompress_dict_multi_device(mi355lz4_ctx *ctx, const uint8_t *framed, uint64_t framedLen, const uint64_t *blockOff,
                                          int nBlocks, int headerKind, int fixedUncomp, const mi355lz4_dictset *ds,
                                          const int32_t *dictIdx, uint8_t *out, const uint64_t *outOff,
                                          const int32_t *outCap /* may be NULL */, int32_t *result);
/* Host-buffer form, synchronous: as mi355lz4_decompress_dict (a single group) with dictIdx, host memory of maxBlocks entries, in
 * place of the dictionary.  The first nBlocks entries -- one per block of the chain -- are checked on the host: one outside -1..n-1
 * is MI355LZ4_E_ARG and nothing is enqueued or written. */
int mi355lz4_decompress_dict_multi(mi355lz4_ctx *ctx, const uint8_t *framedIn, size_t inLen, int headerKind, int fixedUncomp,
                                   const mi355lz4_dictset *ds, const int32_t *dictIdx, uint8_t *out, size_t cap, size_t *outLen,
                                   int32_t *blockLen, int maxBlocks, int *nBlocks);

/* ---- fixed-size output pages: LZ4_compress_destSize for batches ---------------------------------------------------------
 * Every other compress call takes a block of a given size and writes what that needs.  This one takes a destination of a given
 * size and puts as much of the input into it as fits: LZ4_compress_destSize (cbits/lz4.h:205-228, cbits/lz4.c:1382-1414), for
 * callers whose storage is made of fixed-size units -- pages of a table store, sectors, fixed-size clusters, network frames --
 * and who would otherwise compress to slots of compressBound bytes and repack, or guess block sizes and retry.  DESIGN.md 7k.
 *
 * Input i is src[srcOff[i], srcOff[i] + srcLen[i]) (device memory, any alignment).  Page k of input i is exactly what
 *     LZ4_compress_destSize(src_i + pos, dst, &remaining, pageSize[i])
 * returns and writes, where pos is the sum of what pages 0..k-1 of the input consumed and remaining = srcLen[i] - pos: the
 * reference's bytes, its return value in pageCompLen[i*maxPages + k], and the count it stores through srcSizePtr in
 * pageSrcLen[i*maxPages + k].  The page lies at pages + (i*maxPages + k) * pageStride (a 64-bit product).  headerKind 0 writes
 * the raw block there; 4 or 8 writes [compLen] or [compLen][uncompLen] in front of it (little-endian, as every framed block of
 * this engine has).  pageSize counts the block's bytes only: it is the reference's targetDstSize.  A headerKind 8 page is an
 * ordinary block for mi355lz4_decompress_batch_device, with its address as blockOff.  maxPages == 1 is LZ4_compress_destSize
 * for a batch.
 * An input's chain stops when the input is consumed (an empty input is one page with the reference's one-byte empty block,
 * cbits/lz4.c:1263-1273); when maxPages pages are written; at a page that returns 0 -- pageSize < 1: that page is not written
 * and not counted --; and behind a page that consumes nothing while input remains -- pageSize == 1: the reference writes a
 * zero token and consumes 0; that page is written and counted.  nPages[i] counts the pages written, consumed[i] the bytes
 * they hold; an unfinished input shows as consumed[i] < srcLen[i].
 * The table type is chosen per page from what remains, as cbits/lz4.c:1390 does (byU16 with the 4-byte hash under 65547 bytes,
 * byU32 with the 5-byte hash from there on), so a long input changes type in the middle of its chain; a page whose pageSize
 * reaches LZ4_compressBound(remaining) is LZ4_compress_fast_extState's at acceleration 1 (cbits/lz4.c:1387) and takes all that
 * remains.  Every page starts from a fresh table.
 * Progress, what a caller sizes maxPages by: a page of pageSize T >= 1 that leaves input behind consumes at least
 * (T - 1) - (T + 240) / 256 bytes (integer division) -- the all-literals page; tests/test_pages_gpu.py holds every page to it.
 * Asynchronous: the call only enqueues on the engine's stream and reads neither srcLen nor pageSize on the host.  An input
 * whose length lies outside 0..MI355LZ4_MAX_INPUT_SIZE, or whose headerKind + pageSize[i] exceeds pageStride, gets
 * nPages[i] = 0 and nothing else written for it; the other inputs are unaffected.
 * Switches: the compression level, accel, the linked switch, segments and the engine's exact stream play no part.  Block
 * checksums must be off: a checksummed page format is out of scope.
 * MI355LZ4_E_ARG: a null ctx, nInputs < 0, maxPages < 1, a headerKind other than 0 / 4 / 8, pageStride < headerKind + 1, block
 * checksums switched on, with nInputs > 0 a null src, srcOff, srcLen, pageSize, pages or result array.  nInputs == 0 is
 * MI355LZ4_OK.  What the call may write: see the top of this header.
 * One wavefront walks one input's chain (k_exact_pages; 16 KiB of LDS for either table, zeroed once per page), and a chain is
 * serial: a call's parallelism is its number of inputs.  Measured once (scripts/pages_rate.py, profiles/pages_rate.json; medians of
 * 5 event-timed calls): 16384 text records of 4 KiB into 1 KiB pages in 6.1 ms (65536 pages, 87 % full, ratio 1.14;
 * mi355lz4_compress_batch_device on the same records: 0.39 ms, ratio 1.33); 2560 records of 64 KiB into 4 KiB pages in 23.9 ms
 * (30720 pages, 93 % full, ratio 1.43; the batch call: 1.60 ms, ratio 1.82).  No rate is part of the contract. */
int mi355lz4_compress_pages_device(mi355lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                   int nInputs, const int32_t *pageSize, int maxPages, int headerKind,
                                   uint8_t *pages, size_t pageStride,
                                   int32_t *pageSrcLen, int32_t *pageCompLen, int32_t *nPages, int32_t *consumed);
/* Host-buffer form, synchronous: input i is src[i][0, srcLen[i]) in host memory, one pageSize for all; pages, pageSrcLen,
 * pageCompLen, nPages and consumed are host arrays laid out as above.  One group, as mi355lz4_decompress_partial is: one upload,
 * the device call, then the four arrays and every written page's bytes [0, headerKind + compLen) copied back.  The lengths and
 * pageSize are checked on the host: a length outside 0..MI355LZ4_MAX_INPUT_SIZE, a null src[i] with srcLen[i] > 0, pageSize < 1
 * or pageStride < headerKind + pageSize is MI355LZ4_E_ARG, besides the device call's, and nothing is enqueued or written.  The
 * multi-device handle and the legacy LZ4_* face have no such call. */
int mi355lz4_compress_pages(mi355lz4_ctx *ctx, const uint8_t *const *src, const int32_t *srcLen, int nInputs, int pageSize,
                            int maxPages, int headerKind, uint8_t *pages, size_t pageStride,
                            int32_t *pageSrcLen, int32_t *pageCompLen, int32_t *nPages, int32_t *consumed);

/* ---- fast fixed-size output pages: the engine's own encoder with an output budget ----------------------------------------
 * The calls above write LZ4_compress_destSize's bytes and pay for them with its serial parse.  A caller who needs valid,
 * independently decodable, full pages and not those exact bytes takes these: the same arguments plus accel (clamped to 1..65537
 * as in mi355lz4_compress_batch_device), the same layout pages + (i*maxPages + k) * pageStride, headerKind 0 / 4 / 8, pageSrcLen,
 * pageCompLen, nPages and consumed, the same chain stops (input consumed; maxPages reached; pageSize < 1: the page is not written
 * and not counted; pageSize == 1: a zero token that consumes 0, counted, the chain ends), the same per-input skips (a length
 * outside 0..MI355LZ4_MAX_INPUT_SIZE or headerKind + pageSize[i] > pageStride: nPages[i] = 0 and nothing else), the same
 * enqueue-only behaviour with srcLen and pageSize unread on the host, and the same argument errors.  The compression level must
 * be 0 (MI355LZ4_E_ARG otherwise) and block checksums off; the linked switch, segments and the exact stream play no part.
 * DESIGN.md 7m.  What differs is what a page holds:
 * Let pos be what pages 0..k-1 consumed, rem = srcLen[i] - pos, n = min(rem, 65536), T = pageSize[i], and E the block that
 * mi355lz4_compress_batch_device writes for src_i[pos, pos + n) at level 0 with this accel, unlinked, maxBlockLen 65536: sequences
 * s_0 .. s_{m-1} and a last literal run.  If E is at most T bytes, the page is E and consumes n.  A page never holds more than
 * 65536 input bytes: highly compressible input gives pages that are NOT full, and maxPages is sized with that in mind
 * (srcLen / 65536 pages at the least).  Otherwise the page is s_0 .. s_j of E, byte for byte, and one literal run of
 * r_j = min(n - inEnd_j, lit(T - outEnd_j)) bytes behind them, where outEnd_j / inEnd_j are the output / input positions behind
 * s_j (0 / 0 for j = -1, no sequence) and lit(s) is the longest run whose token, length bytes and bytes fit in s.  It consumes
 * inEnd_j + r_j.  j is the last sequence with outEnd_j + 1 <= T, r_j >= 5 and matchStart_j + 12 <= inEnd_j + r_j -- the
 * end-of-block rules of cbits/lz4.c:214-221 --, or -1, the all-literals page.  The reference's shortened last match is not
 * taken over.  Every page is a valid LZ4 block on its own, and the decoded pages of an input concatenate to its consumed prefix.
 * A page that leaves input behind and was cut by T (not by the 64 KiB bound) has compLen >= T - 1 and consumes at least the
 * progress bound above, (T - 1) - (T + 240) / 256.
 * One wavefront walks one input's chain (k_pages_fast: the batch encoder's 10 KiB table, zeroed per page; its parse runs up to a
 * queue of sequences past the page's end).  Measured once (scripts/fastpages_rate.py, profiles/fastpages_rate.json; medians of 5
 * event-timed calls, the exact call timed in the same session): 16384 text records of 4 KiB into 1 KiB pages in 0.66 ms against 6.12 ms
 * (fastest call 6.11) for mi355lz4_compress_pages_device, 65536 pages from either call, 88.6 % against 87.4 % full, ratio 1.129 against
 * 1.144; 2560 records of 64 KiB into 4 KiB pages in 1.45 ms against 23.96 ms (fastest 23.86), 30720 pages from either, 95.6 % against
 * 93.4 % full, ratio 1.395 against 1.427; page count ratio 1.000 on both.  No rate is part of the contract. */
int mi355lz4_compress_pages_fast_device(mi355lz4_ctx *ctx, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                        int nInputs, const int32_t *pageSize, int maxPages, int accel, int headerKind,
                                        uint8_t *pages, size_t pageStride,
                                        int32_t *pageSrcLen, int32_t *pageCompLen, int32_t *nPages, int32_t *consumed);
/* Host-buffer form, synchronous: mi355lz4_compress_pages with accel in front of headerKind, the device call above in its one
 * group, and its host-side checks; a compression level other than 0 is MI355LZ4_E_ARG before anything is enqueued. */
int mi355lz4_compress_pages_fast(mi355lz4_ctx *ctx, const uint8_t *const *src, const int32_t *srcLen, int nInputs, int pageSize,
                                 int maxPages, int accel, int headerKind, uint8_t *pages, size_t pageStride,
                                 int32_t *pageSrcLen, int32_t *pageCompLen, int32_t *nPages, int32_t *consumed);

/* ---- fast fixed-size output pages against a prepared dictionary ---------------------------------------------------------
 * Every page of the calls above starts from an empty table, which costs small records most of what a dictionary gives them.
 * These calls put the dictionary of a loaded mi355lz4_hcdict in front of every page.  Everything that
 * mi355lz4_compress_pages_fast_device and mi355lz4_compress_pages_fast define stays: the layout pages + (i*maxPages + k) *
 * pageStride, headerKind 0 / 4 / 8, pageSrcLen, pageCompLen, nPages and consumed, the chain stops (input consumed; maxPages
 * reached; pageSize < 1: no page; pageSize == 1: a zero token that consumes 0, counted, the chain ends), the per-input skips
 * (nPages[i] = 0 and nothing else), accel clamped to 1..65537, the enqueue-only behaviour with srcLen and pageSize unread on the
 * host.  hd is checked as in mi355lz4_compress_fastdict_device: a null hd or one created on another device is MI355LZ4_E_ARG.
 * The compression level must be 0 and block checksums off: both are MI355LZ4_E_ARG before any device work.  The object is only
 * read, and the sharing rule of a loaded mi355lz4_hcdict applies.  A headerKind 8 page is an ordinary block for
 * mi355lz4_decompress_dict_device with the same dictionary, and every page decodes with LZ4_decompress_safe_usingDict.
 * DESIGN.md 7n.  What a page holds:
 * Let keep be the bytes the last mi355lz4_hcdict_load kept, pos what pages 0..k-1 consumed, n = min(srcLen[i] - pos, 65536),
 * T = pageSize[i], and E the block that mi355lz4_compress_fastdict_device writes for src_i[pos, pos + n) with the same hd and the
 * same accel at a maxBlockLen of at most 65536: sequences s_0 .. s_{m-1} and a last literal run.  If E is at most T bytes, the
 * page is E and consumes n.  Otherwise the page is s_0 .. s_j of E, byte for byte, and one literal run of
 * r_j = min(n - inEnd_j, lit(T - outEnd_j)) bytes behind them, with outEnd_j, inEnd_j and lit() as above; it consumes
 * inEnd_j + r_j.  A cut behind s_j is valid when outEnd_j + 1 <= T, r_j >= 5, matchStart_j + 12 <= inEnd_j + r_j and
 * inEnd_j + r_j >= 13.  j + 1 is the number of leading sequences whose cuts are all valid; j = -1 is the all-literals page.
 * Two points differ from the calls above, both because of the dictionary.  The fourth condition: a block against a dictionary
 * may open with a match at its first byte, and a page that consumes fewer than 13 bytes must be literals only (the rule
 * LZ4_compress_fast keeps, cbits/lz4.c:221).  The leading run instead of the last valid cut: with the fourth condition valid cuts
 * no longer form a prefix -- a match of 4 bytes at position 0 and one of 7 directly behind it, T = 12: the cut behind the first
 * is not valid, the one behind the second is -- and the page must not depend on how the encoder batches its sequences.
 * Every page is a valid LZ4 block on its own given the dictionary (keep bytes of window in front of it), and the decoded pages of an
 * input concatenate to its consumed prefix.  A page that leaves input behind and was cut by T (not by the 64 KiB bound) has
 * compLen >= T - 1 and consumes at least (T - 1) - (T + 240) / 256.
 * With keep == 0 the calls are legal: E is then mi355lz4_compress_fastdict_device's block for an empty dictionary.
 * A persistent grid of single waves walks the chains (k_pages_fastdict: mi355lz4_compress_fastdict_device's grid and staging
 * windows, MI355LZ4_FASTDICT_WAVES included; one chain at a time per wave; every page of 13 input bytes and more copies its slice
 * of the input, 64 KiB at the most, behind the dictionary).  Measured once (scripts/dictpages_rate.py, profiles/dictpages_rate.json;
 * medians of 5 event-timed calls, all three calls in one session, a 64 KiB dictionary): 16384 text records of 4 KiB into 1 KiB pages in
 * 0.84 ms, 48816 pages, 70.0 % full, ratio 1.917, where mi355lz4_compress_pages_fast_device takes 0.66 ms for 65536 pages, 88.6 % full,
 * ratio 1.129, and mi355lz4_compress_fastdict_device without pages 0.61 ms at ratio 1.921; 2560 records of 64 KiB into 4 KiB pages in
 * 1.92 ms, 23040 pages, 93.1 % full, ratio 1.909, against 1.46 ms, 30720 pages, 95.6 % full, ratio 1.395, and 1.47 ms at 1.928.
 * No rate is part of the contract. */
int mi355lz4_compress_pages_fastdict_device(mi355lz4_ctx *ctx, const mi355lz4_hcdict *hd,
                                            const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, int nInputs,
                                            const int32_t *pageSize, int maxPages, int accel, int headerKind,
                                            uint8_t *pages, size_t pageStride,
                                            int32_t *pageSrcLen, int32_t *pageCompLen, int32_t *nPages, int32_t *consumed);
/* Host-buffer form, synchronous: mi355lz4_compress_pages_fast with hd in front of src, the device call above in its one group,
 * and its host-side checks; a null hd, a compression level other than 0 or block checksums are MI355LZ4_E_ARG before anything is
 * enqueued. */
int mi355lz4_compress_pages_fastdict(mi355lz4_ctx *ctx, const mi355lz4_hcdict *hd,
                                     const uint8_t *const *src, const int32_t *srcLen, int nInputs, int pageSize, int maxPages,
                                     int accel, int headerKind, uint8_t *pages, size_t pageStride,
                                     int32_t *pageSrcLen, int32_t *pageCompLen, int32_t *nPages, int32_t *consumed);

/* ---- many linked decode streams, continued across calls ---------------------------------------------------------------
 * The decode-side counterpart of mi355lz4_cstreams, and the device-resident form of the reference's one LZ4_streamDecode_t
 * per stream (Internal/LZ4.hs:539-567 -> cbits/lz4.c:2322-2359): a host that runs many pipelines keeps one slot per
 * pipeline and decodes the next blocks of all of them in ONE call, as they arrive -- every stream written by
 * compressChunksD or by mi355lz4_compress_streams_device is such a stream.
 *
 * A mi355lz4_dstreams is an opaque set of nSlots device-resident decode streams, owned by the caller and bound to the
 * device of the engine it was created with (any engine on that device may use it; one call at a time).  One slot holds
 * what LZ4_streamDecode_t amounts to for separately allocated blocks: the last min(r, 65536) bytes of the stream's last
 * block that decoded to r > 0 bytes, and that count -- 65600 bytes, about 64 KiB a slot (2560 slots: about 160 MiB).  No
 * other state, all of it on the device; nothing of a slot lives on the host.
 * _create leaves every slot reset (no dictionary); _reset does that for slots[0..n) (slots == NULL: all of them), enqueued
 * on the engine's stream; _destroy waits for the device.
 * _set_dict is LZ4_setStreamDecode: slot `slot`'s state becomes the last 64 KiB of dictDevice[0, len) (device memory; the
 * slot keeps its own copy); len == 0 equals a reset.  Enqueued; nothing is read after the call has run on the device. */
typedef struct mi355lz4_dstreams mi355lz4_dstreams;
int mi355lz4_dstreams_create(mi355lz4_ctx *ctx, int nSlots, mi355lz4_dstreams **out);
void mi355lz4_dstreams_destroy(mi355lz4_dstreams *ds);
int mi355lz4_dstreams_count(const mi355lz4_dstreams *ds);
int mi355lz4_dstreams_reset(mi355lz4_ctx *ctx, mi355lz4_dstreams *ds, const int32_t *slots, int n);
int mi355lz4_dstreams_set_dict(mi355lz4_ctx *ctx, mi355lz4_dstreams *ds, int slot, const uint8_t *dictDevice, int len);
/* Decode nBlocks blocks that belong to nStreams linked streams.  The block arguments, cap_i, the header rejections and the
 * per-block codes are those of mi355lz4_decompress_streams_device.  Stream s of the call is the blocks
 * [streamFirst[s], streamFirst[s+1]) and continues slot streamSlot[s]; streamFirst (nStreams + 1 entries, streamFirst[0] == 0,
 * streamFirst[nStreams] == nBlocks, ascending) and streamSlot are small HOST arrays with the rules of
 * mi355lz4_compress_streams_device, checked before anything is enqueued and used up before the call returns.
 * Semantics (cbits/lz4.c:2331-2333, 2347-2355): a stream's first block in the call has the slot's bytes as its dictionary;
 * every later block has the output, in `out`, of the last block before it in the stream that decoded to more than 0 bytes,
 * and the slot when there is none.  A block with a result <= 0 or a rejected header leaves that state alone.  After the
 * stream's last block the slot takes the tail of the last block with r > 0 if the call had one, else it stays as it was;
 * an empty stream leaves its slot untouched.  The slot owns its copy: `out` and `framed` may be overwritten or freed once
 * the call has run.  (The reference takes its prefix path when outputs happen to lie back to back; that mode is not
 * restated, here or elsewhere in this engine.)  However a stream is cut into calls, result[] and the bytes are those of ONE
 * mi355lz4_decompress_streams_device call on the whole stream, for well-formed and malformed blocks alike
 * (tests/test_seam_decode_gpu.py holds the call to it on hand-built and corrupted blocks, the dictionary in the slot and in `out`).
 * Enqueue only: no host wait, no read of device memory on the host, no standalone first pass -- every block is decoded
 * once, with its dictionary.  The call returns MI355LZ4_OK once it is enqueued (beyond four calls in flight it waits for
 * the oldest one's stream table); per-block failures are in result[], as with the partial call.  This is the first linked
 * decode form that can sit in a caller's pipeline without a synchronisation.
 * Block checksums, when on, are verified first as in every decode call; a mismatching block is a header-rejected block
 * (MI355LZ4_BLK_E_CHECKSUM) and the stream goes on as after any rejected block.
 * MI355LZ4_E_ARG: a table that is not ascending or does not cover the blocks, a slot out of range, the same slot twice in
 * one call, `ds` created on another device, null pointers with nBlocks > 0, a range begun with
 * mi355lz4_decompress_linked_begin still open.  nBlocks == 0 is MI355LZ4_OK.  What the call may write: see the top.
 * One wavefront walks one stream: throughput comes from the number of streams in the call (the chip runs 2560 at a
 * time), and a stream with many blocks in one call is one serial chain -- a single long stream belongs in
 * mi355lz4_decompress_batch_device(linked != 0).  Rates: unmeasured until scripts/dstreams_rate.py has written
 * profiles/dstreams_rate.json. */
int mi355lz4_decompress_dstreams_device(mi355lz4_ctx *ctx, mi355lz4_dstreams *ds, const uint8_t *framed,
                                        uint64_t framedLen, const uint64_t *blockOff, int nBlocks, int headerKind,
                                        int fixedUncomp, const int32_t *streamFirst, const int32_t *streamSlot,
                                        int nStreams, uint8_t *out, const uint64_t *outOff, const int32_t *outCap,
                                        int32_t *result);
/* Host-buffer form: as mi355lz4_decompress_batch (a dense framed chain in, the decoded blocks back to back out, blockLen per
 * block, synchronous, the same group pipeline with the slots in place of `dict`; a group seam inside a stream continues
 * through its slot).  Stream s is blocks [streamFirst[s], streamFirst[s+1]) of the chain and the table must cover it.  The
 * chain is walked on the host: a length that does not fit it (compLen <= 0, a block cut short, a negative uncompLen) is
 * MI355LZ4_E_ARG and nothing is enqueued.  Every block is written at its header's size (fixedUncomp for headerKind 4)
 * before its result is known: cap below their sum is MI355LZ4_E_CAPACITY, nothing enqueued. */
int mi355lz4_decompress_dstreams(mi355lz4_ctx *ctx, mi355lz4_dstreams *ds, const uint8_t *framedIn, size_t inLen,
                                 int headerKind, int fixedUncomp, const int32_t *streamFirst, const int32_t *streamSlot,
                                 int nStreams, uint8_t *out, size_t cap, size_t *outLen, int32_t *blockLen, int maxBlocks,
                                 int *nBlocks);

/* ---- many fast linked compress streams, continued across calls ------------------------------------------------------------
 * The wave encoder's counterpart of mi355lz4_cstreams and the write side of mi355lz4_dstreams: a host that runs many pipelines
 * (connections, log shards, files) keeps one slot per pipeline and compresses the next separately allocated arrays of all of
 * them in ONE call, as they arrive -- the reference's compressChunksD situation -- at the speed of the other fast forms instead
 * of one serial chain per stream.
 *
 * A mi355lz4_fstreams is an opaque set of nSlots device-resident streams, owned by the caller and bound to the device of the
 * engine it was created with (any engine on that device may use it; one call at a time).  One slot holds the last
 * min(n, 65536) bytes of the stream's last good block and that count -- the mi355lz4_dstreams slot, 65600 bytes (2560 slots:
 * about 160 MiB) -- all of it on the device.  _create leaves every slot reset (no dictionary); _reset does that for
 * slots[0..n) (slots == NULL: all of them), enqueued on the engine's stream; _destroy waits for the device.
 * _set_dict is the write-side twin of mi355lz4_dstreams_set_dict: slot `slot` becomes the last 64 KiB of dictDevice[0, len)
 * (device memory; the slot keeps its own copy); len == 0 equals a reset.  The call only enqueues. */
typedef struct mi355lz4_fstreams mi355lz4_fstreams;
int mi355lz4_fstreams_create(mi355lz4_ctx *ctx, int nSlots, mi355lz4_fstreams **out);
void mi355lz4_fstreams_destroy(mi355lz4_fstreams *fs);
int mi355lz4_fstreams_count(const mi355lz4_fstreams *fs);
int mi355lz4_fstreams_reset(mi355lz4_ctx *ctx, mi355lz4_fstreams *fs, const int32_t *slots, int n);
int mi355lz4_fstreams_set_dict(mi355lz4_ctx *ctx, mi355lz4_fstreams *fs, int slot, const uint8_t *dictDevice, int len);
/* Compress nBlocks blocks that belong to nStreams linked streams.  The argument list, the stream table rules and the error
 * cases are those of mi355lz4_compress_streams_device with `fs` in place of `cs`: streamFirst and streamSlot are HOST arrays,
 * the table ascending over [0, nBlocks], a slot named only once per call, the set bound to its device, only level 0 accepted
 * (MI355LZ4_E_ARG otherwise).  maxBlockLen is bounded as in mi355lz4_compress_fastdict_device (4 MiB).  The linked switch,
 * segments and the exact switch are ignored; block checksums apply.
 * Dictionary of a block: block k of a stream is compressed with D as its dictionary, D being the last min(len, 65536) bytes
 * of the block before it in its stream -- for a stream's first block in a call, what the slot holds.  There is no dictionary
 * when there is no block before it, when that block was empty, or after a reset: a zero-length array resets a stream's
 * dictionary, as it does LZ4_stream_t's and the linked switch's.
 * Bytes: block k is, byte for byte, what mi355lz4_compress_batch_device with the linked switch on writes for the second block
 * of the contiguous two-block call [D, B_k] at level 0 with the same accel and maxBlockLen = max(|D|, maxBlockLen); with an
 * empty D, the block of the one-block linked call.  So a stream's bytes do not depend on how it is cut into calls -- one block
 * per call, one call for all, or any mix -- nor on where its blocks lie: they equal one linked mi355lz4_compress_batch_device
 * call over the stream laid out contiguously.
 * Interop: the output is a linked stream in the reference's sense with separately allocated blocks, read by
 * mi355lz4_decompress_dstreams_device however the stream is cut, by mi355lz4_decompress_streams_device, by
 * mi355lz4_decompress_batch_device(linked != 0) and by LZ4_decompress_safe_continue.
 * Asynchronous: the call only enqueues and reads no device memory on the host (beyond four calls in flight it waits for the
 * oldest one's stream table).  A srcLen outside 0..maxBlockLen can therefore be no error code: that block and the rest of its
 * stream's blocks in the call get framedLen = 0 and their slots in the output are not written, the stream's state slot stays
 * as it was after the last good block, and other streams are unaffected -- the rule of mi355lz4_compress_streams_device.
 * An empty stream leaves its slot untouched.  The slot owns its copy: src may be overwritten once the call has run.
 * What the call may write: see the top.  All blocks of all streams of a call are compressed at once: a stream of many blocks
 * in one call costs no more than as many streams of one.  Rates (profiles/fstreams_rate.json, scripts/fstreams_rate.py): 16 streams
 * of 160 text blocks of 64 KiB in 1.65 ms where mi355lz4_compress_streams_device takes 1850 ms; 2560 streams of one such block in
 * 1.47 ms against 30.2 ms. */
int mi355lz4_compress_streams_fast_device(mi355lz4_ctx *ctx, mi355lz4_fstreams *fs, const uint8_t *src,
                                          const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride,
                                          int maxBlockLen, int nBlocks, const int32_t *streamFirst,
                                          const int32_t *streamSlot, int nStreams, int accel, int headerKind,
                                          uint8_t *slots, size_t slotStride, int32_t *framedLen);
/* Host-buffer form: as mi355lz4_compress_streams (one dense framed stream in block order, blockFramedLen and status per
 * block, synchronous, the same group pipeline; a group seam inside a stream continues through its slot).  The lengths are
 * checked on the host: a bad one is MI355LZ4_E_ARG and nothing is enqueued. */
int mi355lz4_compress_streams_fast(mi355lz4_ctx *ctx, mi355lz4_fstreams *fs, const uint8_t *const *src,
                                   const int32_t *srcLen, int nBlocks, const int32_t *streamFirst,
                                   const int32_t *streamSlot, int nStreams, int accel, int headerKind, uint8_t *framedOut,
                                   size_t cap, size_t *outLen, int32_t *blockFramedLen, int32_t *status);
/* High-compression levels of the two calls above: a property of the set, as LZ4_streamHC_t carries its level.  "Only level 0
 * accepted" above speaks of the ENGINE's level (mi355lz4_set_compression_level), which selects the encoder of the batch calls
 * and stays 0 for the fast stream calls whatever the set's level is; the set's own level selects theirs.  _set_level(fs, L):
 * L in 0..12, 0 (the default after _create) is the wave encoder and everything above holds byte for byte; 1..12 is the
 * hash-chain encoder of mi355lz4_set_compression_level (10..12 search as 9).  A host-side attribute: it needs no device and
 * enqueues nothing, and it applies to the calls made after it -- a call already enqueued keeps the level it was made at.  A
 * NULL set is MI355LZ4_E_ARG; a level outside 0..12 is MI355LZ4_E_ARG and leaves the level as it was.  _get_level returns the
 * level (MI355LZ4_E_ARG for a NULL set).
 * At set level L in 1..12: the dictionary rule, the stream table rules, the bad-length rule, the empty-stream and empty-block
 * rules, the enqueue-only behaviour, what the call may write and block checksums are exactly those of level 0; accel is ignored,
 * as every high-compression call ignores it.  Bytes: block k is, byte for byte, what mi355lz4_compress_batch_device with the
 * linked switch on and the engine at level L writes for the second block of the contiguous two-block call [D, B_k] with
 * maxBlockLen = max(|D|, maxBlockLen); with an empty D, the block of the one-block linked call.  So a stream's bytes depend
 * neither on how it is cut into calls nor on where its blocks lie: they equal one linked mi355lz4_compress_batch_device call at
 * level L over the stream laid out contiguously.  The level may change between calls of one stream: a slot is the last 64 KiB
 * of the stream whatever encoder wrote the block, so the stream stays one valid linked stream, read by the same four readers.
 * mi355lz4_compress_streams_fast follows the set's level the same way, group seams included.  One workgroup per block on a
 * grid of one per CU (MI355LZ4_HSTREAMS_GROUPS, read per call: that many workgroups, clamped to 1..CUs).  Rates (profiles/hstreams_rate.json,
 * scripts/hstreams_rate.py; text): 16 streams of 160 blocks of 64 KiB at level 9 in 78.5 ms and 0.790 of level 0's bytes, where
 * one linked mi355lz4_compress_batch_device call per stream -- the same bytes -- takes 124.4 ms and level 0 1.54 ms; 2560 streams
 * of one such block in 53.2 ms against 13.6 s. */
int mi355lz4_fstreams_set_level(mi355lz4_fstreams *fs, int level);   /* 0..12; 0: the wave encoder (default) */
int mi355lz4_fstreams_get_level(const mi355lz4_fstreams *fs);

/* mi355lz4_slot_stride with room for the trailer when blockChecksum != 0. */
size_t mi355lz4_slot_stride_ex(int blockLen, int headerKind, int blockChecksum);
/* mi355lz4_index_host over a chain whose blocks carry trailers when blockChecksum != 0 (a block spans
 * headerKind + compLen + 4 bytes); a trailer cut short is MI355LZ4_E_STREAM. */
int mi355lz4_index_host_ex(const uint8_t *framedIn, size_t inLen, int headerKind, int fixedUncomp, int blockChecksum,
                           uint64_t *blockOff, int32_t *uncompLen, int maxBlocks, int *nBlocks);
/* out[i] = xxh32(seed) of base[off[i] .. off[i] + len[i]) for i < n: any length (len[i] < 0: out[i] is not written),
 * any alignment.  All pointers are DEVICE pointers; asynchronous on the engine's stream.  The kernel behind the block
 * checksums. */
int mi355lz4_xxh32_device(mi355lz4_ctx *ctx, const uint8_t *base, const uint64_t *off, const int32_t *len, int n,
                          uint32_t seed, uint32_t *out);

/* ---- batches of standard LZ4 frames ------------------------------------
 * The LZ4 frame format (what the `lz4` tool and liblz4's LZ4F_* write) as a batched, device-resident call.  A caller-owned
 * object holds a parsed batch: _frames_load parses many inputs on the device and reports their exact decoded sizes,
 * _frames_decode decodes them all.  An input is what `lz4 -d` accepts: any sequence of LZ4 frames and skippable frames; it may
 * be empty (size 0).  The device-pointer calls carry no _device suffix: they are methods of an object, as mi355lz4_hcdict_load.
 *
 * Format: magic 0x184D2204; skippable frames 0x184D2A50..5F are skipped; version 01; reserved FLG and BD bits and DictID frames
 * are rejected; BD codes 4..7; the optional 8-byte content size; the header checksum byte; in a block word the high bit marks a
 * stored block, n <= the frame's block maximum, 0 is the end mark; a stored block of 0 bytes is skipped; optional block
 * checksums over the block's bytes as stored; the optional content checksum behind the end mark; trailing bytes that begin no
 * frame are MI355LZ4_FRM_E_MAGIC (fewer than four of them: _TRUNCATED).  A linked frame's window is the last 64 KiB of that
 * frame's output, across stored and short blocks.
 * A compressed block's size is read off its token chain by the rule of mi355lz4_decoded_size_device without the last clause of
 * its rule 4 (a long match from the window that ends near the block's end is legitimate in a linked frame), and it is bounded by
 * the frame's block maximum.  Rule 2 stays: a block that breaks the format's end-of-block rules (no match in a block under 13
 * bytes, the last match at least 12 bytes before the end, five literals last) is refused with MI355LZ4_FRM_E_BLOCK where
 * liblz4, given spare capacity, might accept it.  No conforming encoder writes such a block.
 *
 * Codes: sizes[i] / result[i] is the input's decoded size or the MI355LZ4_FRM_E_* code of the error with the smallest byte
 * position in the input: a header error sits at the frame's magic, a block error at the block's size word, content size and
 * content checksum errors at the end mark.  The scan stops at the first structural error (MAGIC, HEADER, HEADER_CHECKSUM,
 * TRUNCATED, BLOCK_SIZE): nothing behind it exists, block errors in front of it win.  MAGIC .. BLOCK_CHECKSUM, CONTENT_SIZE
 * and BLOCK for a chain without a size are known at _load; BLOCK from decoding and CONTENT_CHECKSUM appear in _decode's result.
 * The two flags switch the respective verification off; the fields must still be present and inside the input.
 *
 * _frames_load: buf, inOff, inLen are DEVICE memory; input i is buf[inOff[i], inOff[i] + inLen[i]), full 64-bit quantities, any
 * alignment (an input that leaves [0, bufLen) is _TRUNCATED).  It parses on the engine's stream and WAITS for it, twice: for the
 * frame and block counts that size the tables, and for the sizes.  The tables cost a fixed number of bytes per input, frame
 * and block that is really there; nothing is sized by a declared content size or by blocks x maximum block size.  The object
 * keeps its own copy of inOff and inLen and borrows buf, which must hold the same bytes until the decodes that use it have
 * run.  A second _load on the same object replaces the first.  The frames and the blocks of a call must each number below
 * INT_MAX (MI355LZ4_E_ARG otherwise).
 * _frames_inputs / _blocks / _total (sum of the sizes >= 0) / _sizes (device array, nInputs entries) / _get_sizes (the host
 * copy that _load read back) describe the last _load.
 * _frames_decode: out, outOff, result are DEVICE memory.  Enqueue only, on the engine's stream; mi355lz4_set_block_checksum is
 * ignored (a frame's block checksums are its own).  Input i with sizes[i] >= 0 is written to out[outOff[i], outOff[i] +
 * sizes[i]); result[i] = its size or a code; an input whose size is a code gets that code and nothing of `out` is touched for
 * it; an input that fails at decode time leaves unspecified bytes inside its own range and nowhere else.  The object's decode
 * scratch is written: two decodes of ONE object go on the same stream, or the caller orders them.  Compressed blocks of
 * independent frames take the engine's own decode paths in one internal call; a linked frame is one wavefront's work.
 * MI355LZ4_E_ARG: a null ctx or fr, nInputs < 0, a null array with nInputs > 0, unknown flag bits, an object created on
 * another device's engine, _decode before any _load, a null out with bytes to write.  nInputs == 0 is MI355LZ4_OK.
 * mi355lz4_decompress_frames: host buffers, synchronous: the inputs go to the device, _load, _decode into a dense layout (input
 * i at the scan of the sizes >= 0), outputs and result[] come back: input i lies at the scan of the results >= 0 (an input
 * that failed at decode time is closed up on the host), *outLen = their sum.  cap below the total of the sizes:
 * MI355LZ4_E_CAPACITY with *outLen = that total and nothing written to out, so one failed call sizes the buffer.
 * MI355LZ4_E_BLOCK when some input has a negative result; the others are delivered. */
typedef struct mi355lz4_frames mi355lz4_frames;
#define MI355LZ4_FRAMES_SKIP_CONTENT_CHECKSUM 1u
#define MI355LZ4_FRAMES_SKIP_BLOCK_CHECKSUM   2u
int mi355lz4_frames_create(mi355lz4_ctx *ctx, mi355lz4_frames **out);
void mi355lz4_frames_destroy(mi355lz4_frames *fr);
int mi355lz4_frames_load(mi355lz4_ctx *ctx, mi355lz4_frames *fr, const uint8_t *buf, uint64_t bufLen,
                         const uint64_t *inOff, const uint64_t *inLen, int nInputs, unsigned flags);
int mi355lz4_frames_inputs(const mi355lz4_frames *fr);
int mi355lz4_frames_blocks(const mi355lz4_frames *fr);
uint64_t mi355lz4_frames_total(const mi355lz4_frames *fr);
const int64_t *mi355lz4_frames_sizes(const mi355lz4_frames *fr);
int mi355lz4_frames_get_sizes(const mi355lz4_frames *fr, int64_t *sizesHost);
int mi355lz4_frames_decode(mi355lz4_ctx *ctx, const mi355lz4_frames *fr, uint8_t *out, const uint64_t *outOff,
                           int64_t *result);
int mi355lz4_decompress_frames(mi355lz4_ctx *ctx, const uint8_t *const *in, const size_t *inLen, int nInputs,
                               unsigned flags, uint8_t *out, size_t cap, size_t *outLen, int64_t *result);

/* ---- writing batches of standard LZ4 frames ------------------------------
 * The write side of the frame batches: many device-resident inputs become one standard LZ4 frame each -- what the `lz4` tool,
 * LZ4F_decompress and mi355lz4_frames_load read -- in one call that only enqueues.  A caller-owned object, the frame writer,
 * holds the call's block table and the slots its blocks are compressed into.  The device-pointer calls carry no _device
 * suffix: they are methods of an object, as those of mi355lz4_frames.
 *
 * _cframes_compress: src, inOff, inLen, dst, dstOff, dstCap, frameLen are DEVICE memory.  Input i is src[inOff[i], inOff[i] +
 * inLen[i]), full 64-bit quantities, any alignment; it may be empty.  It becomes exactly one frame at dst + dstOff[i]:
 * frameLen[i] = the frame's length, or MI355LZ4_FRW_E_CAPACITY (the frame does not fit dstCap[i]) or MI355LZ4_FRW_E_INPUT (the
 * input leaves [0, srcBufLen), is longer than maxInputLen, or its blocks end behind the call's block bound), and then nothing
 * is written for the input; the other inputs are unaffected, except that the blocks are counted in input order, so every
 * input with blocks behind one that passes the block bound gets _INPUT too.
 * The frame: magic; FLG (version 01, B.Indep unless MI355LZ4_CFRAMES_LINKED, the three option bits); BD (blockSizeId 4..7: 64 KiB,
 * 256 KiB, 1 MiB, 4 MiB); the 8-byte content size when asked for; the header checksum byte; ceil(len / block size) blocks, of
 * which only the last may be short (an empty input has none); the end mark; the content checksum when asked for.  A block
 * whose compressed size c >= its n bytes is stored (word n | 0x80000000, the input's bytes: lz4FrameCompress's rule); a block
 * checksum covers the payload as stored.
 * The bytes of a compressed block are exactly what one mi355lz4_compress_batch_device call (headerKind 4, maxBlockLen =
 * min(block size, maxInputLen), the engine at its current compression level 0..12, mi355lz4_set_linked_compress = the LINKED
 * flag, the same accel) over the blocks of input i
 * alone, where they lie in src, writes as block k's data -- at level 0 whenever the segment path makes the same choice in both
 * calls (mi355lz4_set_segments(0) fixes that), always at levels 1..12 and with LINKED.  Reference-exact mode and
 * mi355lz4_set_block_checksum do not apply (a frame is its own stream and its block checksums are its own); the engine's linked
 * switch is left as it was.  A linked frame's first block never sees the input in front of it, even where the two lie back
 * to back in src.
 * Host-side bounds: the call cannot read inLen, so the caller states maxInputLen >= every inLen[i] (it gives the largest block,
 * min(block size, maxInputLen), and so the slots' stride) and totalLen >= their sum (the block table holds totalLen / block
 * size + nInputs blocks).  _cframes_reserve sizes the object's scratch for such a shape ahead of time (for LINKED, the larger
 * one); a _compress that finds it too small waits for the engine's stream and grows it.  A warm call only enqueues on the
 * engine's stream (tests/test_cframes_stream_gpu.py).  The scratch is the tables (some 40 bytes per table entry) and one slot of
 * mi355lz4_slot_stride(largest block, 4) bytes per table entry -- with LINKED the table has one more entry per input, which
 * keeps inputs apart.  Two calls on ONE object go on the same stream, or the caller orders them.
 * mi355lz4_cframes_bound (host only): the exact worst case, (7 or 15) + blocks * (4 + 4 with block checksums) + len + 4 + 4 with a
 * content checksum; a dstCap[i] of it never gives _CAPACITY.  0 for a blockSizeId outside 4..7 or unknown flag bits.
 * The content checksum of an input is computed by four lanes (xxh32 is four serial chains): one huge input with
 * MI355LZ4_CFRAMES_CONTENT_CHECKSUM is hashed at well under 1 GB/s, as on the decode side.
 * MI355LZ4_E_ARG: a null ctx or object, an object created on another device's engine, nInputs < 0, a null array with nInputs >
 * 0, blockSizeId outside 4..7, unknown flag bits, totalLen / block size + nInputs (+ nInputs with LINKED) at or above INT_MAX.
 * nInputs == 0 is MI355LZ4_OK.
 * mi355lz4_compress_frames: host buffers, synchronous.  The inputs go to the device in groups under a device-memory budget
 * (MI355LZ4_CFRAMES_BUDGET_MB, default 1024; one input is never split), each group is compressed into a bound-spaced layout, a
 * gather kernel packs its frames densely and one copy brings them back: frame i lies in `out` at the sum of frameLen[0, i),
 * *outLen = their sum.  When they do not fit cap: MI355LZ4_E_CAPACITY with *outLen = that sum, frameLen[] filled and nothing
 * written to out, so one failed call sizes the buffer. */
typedef struct mi355lz4_cframes mi355lz4_cframes;
#define MI355LZ4_CFRAMES_LINKED            1u   /* block-dependent frames (what `lz4` writes by default) */
#define MI355LZ4_CFRAMES_BLOCK_CHECKSUM    2u
#define MI355LZ4_CFRAMES_CONTENT_SIZE      4u
#define MI355LZ4_CFRAMES_CONTENT_CHECKSUM  8u
#define MI355LZ4_FRW_E_CAPACITY (-0x7F000201)   /* the frame does not fit dstCap[i]; nothing written for the input */
#define MI355LZ4_FRW_E_INPUT    (-0x7F000202)   /* the input leaves [0, srcBufLen), exceeds maxInputLen, or its blocks do not fit the call's block bound */
uint64_t mi355lz4_cframes_bound(uint64_t len, int blockSizeId, unsigned flags);
int mi355lz4_cframes_create(mi355lz4_ctx *ctx, mi355lz4_cframes **out);
void mi355lz4_cframes_destroy(mi355lz4_cframes *w);
int mi355lz4_cframes_reserve(mi355lz4_ctx *ctx, mi355lz4_cframes *w, int nInputs, uint64_t maxInputLen, uint64_t totalLen,
                             int blockSizeId);
int mi355lz4_cframes_compress(mi355lz4_ctx *ctx, mi355lz4_cframes *w, const uint8_t *src, uint64_t srcBufLen,
                              const uint64_t *inOff, const uint64_t *inLen, int nInputs, uint64_t maxInputLen, uint64_t totalLen,
                              int blockSizeId, unsigned flags, int accel, uint8_t *dst, const uint64_t *dstOff,
                              const uint64_t *dstCap, int64_t *frameLen);
int mi355lz4_compress_frames(mi355lz4_ctx *ctx, const uint8_t *const *in, const size_t *inLen, int nInputs, int blockSizeId,
                             unsigned flags, int accel, uint8_t *out, size_t cap, size_t *outLen, int64_t *frameLen);

/* ---- timing support: HIP events on the engine's own stream ------------- */
int mi355lz4_event_create(void **ev);
int mi355lz4_event_destroy(void *ev);
int mi355lz4_event_record(mi355lz4_ctx *ctx, void *ev);
/* Blocks until `stop` completed; *ms = elapsed milliseconds start -> stop. */
int mi355lz4_event_elapsed_ms(void *start, void *stop, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* MI355LZ4_H */
