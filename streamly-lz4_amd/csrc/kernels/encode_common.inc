// kernels/encode_common.inc -- what every encoder kernel knows about a call's blocks and slots: the head of kernels/encode.inc, and of
// kernels_hstreams.hip, the one encoder kernel that is a translation unit of its own.  Included, not compiled on its own.
// ---------------------------------------------------------------------------
// What every encoder kernel knows about a call's blocks and slots, once.
// ---------------------------------------------------------------------------
// (The helpers take EncodeArgs by value, and enc_linked_dict has one return: with the kernel's argument handed on by reference,
// or with a second return, k_encode<true, false> and k_encode_seg came out with other scalar spill counts than the written-out
// code they replace -- docs/MEASUREMENT_LOG.md section 17.  Inlined, a copy costs nothing.  k_seg_sizes alone keeps its length
// written out: through the by-value helper it takes 36 scalar registers, not 32.)
// where block blk of a call lies and how long it is (a caller that needs one of the two leaves the other unread)
struct EncBlock { uint64_t off; int n; };
__device__ __forceinline__ EncBlock enc_block(const EncodeArgs a, int blk)
{
    return EncBlock{a.srcOff ? a.srcOff[blk] : (uint64_t)blk * a.blockStride, a.srcLen ? a.srcLen[blk] : a.uniformLen};
}

// linked stream: the block before is the dictionary when it lies directly in front of this one (at off), its last 64 KiB at the most
__device__ __forceinline__ int enc_linked_dict(const EncodeArgs a, int blk, uint64_t off)
{
    int dictLen = 0;
    if (a.linked && (blk > 0 || a.lookBack > 0)) {
        const EncBlock p = enc_block(a, blk - 1);
        if (p.n > 0 && p.off + (uint64_t)p.n == off) dictLen = min(p.n, 65536);
    }
    return dictLen;
}

// cbits/lz4.c:1263-1273: empty input -> single 0 token
__device__ __forceinline__ int enc_empty_block(uint8_t *dst, bool writer)
{
    if (writer) dst[0] = 0;
    return 1;
}

// the end of every block: c compressed bytes of n, the slot's header and the block's framedLen, by the one lane or thread that writes
__device__ __forceinline__ void enc_finish_slot(const EncodeArgs a, int blk, uint8_t *slot, int c, int n, bool writer)
{
    if (!writer) return;
    store_le32(slot, c);                                   // Internal/LZ4.hs:262
    if (a.headerKind == 8) store_le32(slot + 4, n);        // Internal/LZ4.hs:261
    a.framedLen[blk] = (c > 0) ? a.headerKind + c : 0;
}

// n bytes by a workgroup of nWaves waves, this one being `wave`: each wave copies a run of pieces of `piece` bytes
__device__ __forceinline__ void wg_copy_pieces(uint8_t *dst, const uint8_t *src, uint32_t n, uint32_t piece, uint32_t wave, uint32_t nWaves)
{
    for (uint32_t at = wave * piece; at < n; at += nWaves * piece) wave_copy_bytes(dst + at, src + at, min(n - at, piece));
}
