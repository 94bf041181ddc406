// kernels/linked_walk.inc -- linked streams walked in order by one wave: per stream, per stream slot across calls (dstreams), per short run.
// A part of kernels.hip, the one device translation unit: included there, in this order, and not compiled on its own.
// Linked streams (reference semantics of LZ4_decompress_safe_continue with every
// block in its own allocation, cbits/lz4.c:2347-2355): block i may reference the
// output of the last block before it IN ITS STREAM that decoded to > 0 bytes.  A
// block that decodes standalone never consulted a dictionary, so its standalone
// result IS its linked result; only blocks whose standalone decode failed are
// re-decoded here, in stream order, with the dictionary in force.  The chain
// inside one stream is serial (block i needs the bytes of block i-1), so one
// wavefront walks each stream with the lane-parallel decoder; independent
// streams run side by side.  (SURVEY.md 8f N1.)
__global__ PAR_OCC void k_decode_fixup_linked(DecodeArgs a)
{
    if (a.asyncGate && a.linkStat[0] == 0u) return;     // asynchronous linked decode: the first pass found nothing to do
    __shared__ ParLds lds;
    const int sIdx = (int)blockIdx.x;
    if (a.ptr.bad && !a.ptr.bad[sIdx]) return;                        // the data-parallel pass has done this stream
    int b0 = 0, b1 = a.nBlocks;
    const uint8_t *dict = nullptr;
    uint32_t dictLen = 0;
    if (a.streamFirst) {
        b0 = min(max(uni(a.streamFirst[sIdx]), 0), a.nBlocks);
        b1 = min(max(uni(a.streamFirst[sIdx + 1]), b0), a.nBlocks);
    } else if (a.dict0) {
        dict = a.dict0; dictLen = a.dict0Len;
    }
    for (int blk = b0; blk < b1; blk++) {
        int r = uni(a.result[blk]);
        uint8_t *dst = a.out + a.outOff[blk];
        if (r < 0 && r > -0x7F000000 && dictLen > 0) {   // codec error (not a header rejection)
            const uint8_t *data = nullptr;
            int compLen = 0, cap = 0;
            r = read_block_header(a, blk, data, compLen, cap);
            if (r == 0)
                r = decode_block_par<false, true>(data, compLen, dst, cap, dict, dictLen, a.framed,
                                            a.framed + a.framedLen, lds, nullptr);
            r = uni(r);
            if (lane_id() == 0) a.result[blk] = r;
        }
        if (r > 0) { dict = dst; dictLen = (uint32_t)r; }          // :2331-2333, :2353-2355
        wave_fence();       // (the next block reads this one through the pipeline that wrote it: no write-back, see k_runin_decode)
    }
}

// Many linked decode streams continued across calls (mi355lz4_decompress_dstreams_device, DESIGN.md 7h).  Wave w continues the
// stream in slot work[3w + 2] with the blocks [work[3w], work[3w + 1]) of the call.  A slot is what LZ4_streamDecode_t amounts
// to for separately allocated blocks: the last min(r, 65536) bytes of the stream's last block that decoded to r > 0 bytes,
// and that count.  Every block is decoded once, with the dictionary in force (:2347-2355) -- there is no standalone pass
// whose verdict a host would have to read.  A block with a result <= 0 or a rejected header leaves the dictionary alone
// (:2331-2333); after the last block the slot takes the tail of the last block with r > 0, if the call had one.
__global__ PAR_OCC void k_decode_dstreams(DStreamsArgs x)
{
    __shared__ ParLds lds;
    const int32_t *w = x.work + 3 * (size_t)blockIdx.x;
    const int b0 = uni(w[0]), b1 = uni(w[1]);
    uint8_t *slot = x.state + (size_t)uni(w[2]) * DSTREAM_SLOT_BYTES;
    uint32_t *count = (uint32_t *)(slot + DSTREAM_COUNT_OFF);
    const uint8_t *dict = slot;
    uint32_t dictLen = min((uint32_t)uni((int)as_global(count)[0]), (uint32_t)DSTREAM_DICT_BYTES);
    const uint8_t *last = nullptr;                                  // the call's last block with r > 0: the slot's next content
    uint32_t lastN = 0;
    for (int blk = b0; blk < b1; blk++) {
        const uint8_t *data = nullptr;
        int compLen = 0, cap = 0;
        uint8_t *dst = x.d.out + x.d.outOff[blk];
        int r = read_block_header(x.d, blk, data, compLen, cap);
        if (r == 0)
            r = decode_block_par<false, true>(data, compLen, dst, cap, dict, dictLen, x.d.framed,
                                              x.d.framed + x.d.framedLen, lds, nullptr);
        r = uni(r);
        if (lane_id() == 0) x.d.result[blk] = r;
        if (r > 0) { dict = dst; dictLen = (uint32_t)r; last = dst; lastN = (uint32_t)r; }
        wave_fence();       // (the next block reads this one through the pipeline that wrote it, see k_decode_fixup_linked)
    }
    if (!last) return;                                              // no block with output: the slot is as it was
    // (the slot was read by the blocks up to the first one with r > 0, whose loads have returned: wave order)
    const uint32_t keep = lastN < (uint32_t)DSTREAM_DICT_BYTES ? lastN : (uint32_t)DSTREAM_DICT_BYTES;
    wave_copy_bytes(slot, last + (lastN - keep), keep);
    if (lane_id() == 0) as_global(count)[0] = keep;
}

void launch_decode_dstreams(const DStreamsArgs &a, int nWork, hipStream_t s)
{
    if (nWork <= 0) return;
    hipLaunchKernelGGL(k_decode_dstreams, dim3((unsigned)nWork), dim3(64), 0, s, a);
}

// A batch of independent blocks against ONE external dictionary (mi355lz4_decompress_dict_device, DESIGN.md 7i): block
// blockIdx.x is LZ4_decompress_safe_usingDict on its external-dictionary path (LZ4_decompress_safe_forceExtDict,
// cbits/lz4.c:2404-2417) with (a.dict0, a.dict0Len), any length -- only the last 64 KiB can be reached, and a dictionary
// under 64 KiB arms the offset check (:1764).  One wavefront per block, every block decoded once with the dictionary: no
// standalone pass, no second pass, and the dictionary is only read.
__global__ PAR_OCC void k_decode_dict(DecodeArgs a)
{
    __shared__ ParLds lds;
    const int blk = (int)blockIdx.x;
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0;
    int r = read_block_header(a, blk, data, compLen, cap);
    if (r == 0)
        r = decode_block_par<false, true>(data, compLen, a.out + a.outOff[blk], cap, a.dict0, a.dict0Len, a.framed,
                                          a.framed + a.framedLen, lds, nullptr);
    r = uni(r);
    if (lane_id() == 0) a.result[blk] = r;
}

void launch_decode_dict(const DecodeArgs &a, hipStream_t s)
{
    if (a.nBlocks <= 0) return;
    hipLaunchKernelGGL(k_decode_dict, dim3((unsigned)a.nBlocks), dim3(64), 0, s, a);
}

// LZ4_setStreamDecode for `count` slots from `first` on (one wave each): the slot's state becomes the keep <= 65536 bytes at
// src (none: a reset).  dstreams_set_dict and dstreams_reset; nothing of the host is read.
__global__ __launch_bounds__(LZ4_WAVE) void k_dstreams_set(uint8_t *state, int first, const uint8_t *src, uint32_t keep)
{
    uint8_t *slot = state + (size_t)(first + (int)blockIdx.x) * DSTREAM_SLOT_BYTES;
    if (keep) wave_copy_bytes(slot, src, keep);
    if (lane_id() == 0) as_global((uint32_t *)(slot + DSTREAM_COUNT_OFF))[0] = keep;
}

void launch_dstreams_set(uint8_t *state, int first, int count, const uint8_t *src, uint32_t keep, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_dstreams_set, dim3((unsigned)count), dim3(LZ4_WAVE), 0, s, state, first, src,
                       keep > (uint32_t)DSTREAM_DICT_BYTES ? (uint32_t)DSTREAM_DICT_BYTES : keep);
}

// One stream in which FEW blocks need their dictionary (a reference-written stream of data whose matches rarely reach
// back into the block before: 229 of 16 384 blocks of the bench's lzsynth sample): every maximal run of blocks without
// output is walked by a wavefront of its own with the exact lane-parallel decoder and the previous output as external
// dictionary -- the runs are independent of each other because the block in front of a run is final.  The pointer pass
// would write and chase four bytes of pointer per output byte of the whole SPAN between the first and the last dependent
// block for them (2 ms for that sample; this: one block's latency per block of the longest run).  Chosen by the host
// when the longest run is short (linkStat[5]); same dictionary rules as k_decode_fixup_regions (:2331-2333, :2347-2355).
// The runs' first blocks are taken from the FIRST pass's results before any walker has changed them (k_run_starts: a
// list).  Round 4 let every wave decide "am I a run start" from result[blk - 1] inside the walking launch: a wave
// dispatched late could see the block in front of it already fixed by its run's walker, take itself for a run start and
// walk the same blocks a second time, racing the first walker.  (The list also shrinks the grid to one wave per run.)
__global__ __launch_bounds__(256) void k_run_starts(DecodeArgs a)
{
    const int blk = a.segFirst + (int)(blockIdx.x * 256u + threadIdx.x);
    if (blk >= a.segEnd || a.result[blk] > 0) return;
    if (blk != a.segFirst && a.result[blk - 1] <= 0) return;
    const int i = atomicAdd(&a.runs.list[0], 1);
    if (i < a.runs.cap) a.runs.list[1 + i] = blk;
}

__global__ PAR_OCC void k_decode_fixup_runs(DecodeArgs a)
{
    __shared__ ParLds lds;
    int blk = a.segFirst;                                           // (no list: one run, the legacy face's single block)
    if (a.runs.list) {
        if ((int)blockIdx.x >= min(uni(a.runs.list[0]), a.runs.cap)) return;
        blk = uni(a.runs.list[1 + blockIdx.x]);
    } else if (blockIdx.x != 0) return;
    if (blk >= a.segEnd || uni(a.result[blk]) > 0) return;
    const uint8_t *dict = nullptr;
    uint32_t dictLen = 0;
    if (a.dict0) { dict = a.dict0; dictLen = a.dict0Len; }
    for (int j = blk - 1; j >= -a.lookBack; j--) {
        const int rj = uni(a.result[j]);
        if (rj > 0) { dict = a.out + a.outOff[j]; dictLen = (uint32_t)rj; break; }
    }
    // (the blocks behind a run's end decoded in the first pass: no walker writes their results, reading them is safe)
    for (int f = blk; f < a.segEnd; f++) {
        int r = uni(a.result[f]);
        if (r > 0) break;                                           // the run is over
        uint8_t *dst = a.out + a.outOff[f];
        if (is_codec_error(r) && dictLen > 0) {
            const uint8_t *data = nullptr;
            int compLen = 0, cap = 0;
            r = read_block_header(a, f, data, compLen, cap);
            if (r == 0)
                r = decode_block_par<false, true>(data, compLen, dst, cap, dict, dictLen, a.framed,
                                                  a.framed + a.framedLen, lds, nullptr);
            r = uni(r);
            wave_fence();                                           // (one wave per run, nobody else looks before the launch ends)
            if (lane_id() == 0) a.result[f] = r;
        }
        if (r > 0) { dict = dst; dictLen = (uint32_t)r; }
    }
}

void launch_linked_runs(const DecodeArgs &a, hipStream_t s)
{
    const int n = a.segEnd - a.segFirst;
    if (n <= 0) return;
    if (!a.runs.list) { hipLaunchKernelGGL(k_decode_fixup_runs, dim3(1), dim3(64), 0, s, a); return; }
    hipLaunchKernelGGL(k_run_starts, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_decode_fixup_runs, dim3((unsigned)min(n, a.runs.cap)), dim3(64), 0, s, a);
}

// k_decode_dict with a dictionary per block (mi355lz4_decompress_dict_multi_device, DESIGN.md 7o): block blockIdx.x is decoded
// against the kept bytes of member dictIdx[blk] of a mi355lz4_dictset -- the bytes and their count read wave-uniformly from the
// member's image -- or against none (-1).  Any other index: BLK_E_DICT, and nothing of the block is read or written.  The same
// one wavefront per block, the same decoder; the members are only read.
__global__ PAR_OCC void k_decode_dict_multi(DictMultiArgs x)
{
    __shared__ ParLds lds;
    const int blk = (int)blockIdx.x;
    const int k = uni(x.dictIdx[blk]);
    if (k < -1 || k >= x.nDicts) {
        if (lane_id() == 0) x.d.result[blk] = BLK_E_DICT;
        return;
    }
    const uint8_t *dict = nullptr;
    uint32_t dictLen = 0;
    if (k >= 0) {
        const uint8_t *image = (const uint8_t *)(uintptr_t)uni64((int64_t)(uintptr_t)x.set[k].image);
        dictLen = min((uint32_t)uni((int)as_global((const uint32_t *)(image + HCDICT_KEEP_OFF))[0]), 65536u);
        dict = image + HCDICT_DICT_OFF;
    }
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0;
    int r = read_block_header(x.d, blk, data, compLen, cap);
    if (r == 0)
        r = decode_block_par<false, true>(data, compLen, x.d.out + x.d.outOff[blk], cap, dict, dictLen, x.d.framed,
                                          x.d.framed + x.d.framedLen, lds, nullptr);
    r = uni(r);
    if (lane_id() == 0) x.d.result[blk] = r;
}

void launch_decode_dict_multi(const DictMultiArgs &a, hipStream_t s)
{
    if (a.d.nBlocks <= 0) return;
    hipLaunchKernelGGL(k_decode_dict_multi, dim3((unsigned)a.d.nBlocks), dim3(64), 0, s, a);
}
