// kernels/frames.inc -- batches of standard LZ4 frames: the frame layer on the device (mi355lz4_frames, DESIGN.md 7r).
// A part of kernels.hip, the one device translation unit: included there, in this order, and not compiled on its own.
//
// load:   k_frames_scan    one wavefront per input walks frames and block words: counts, the first structural error
//         k_scan_u64       (twice) first frame and first block of every input
//         k_frames_fill    the same walk again, writing the tables
//         k_frames_bsum    block checksums, four lanes per block (checksum.hpp)
//         k_frames_sizes   one wavefront per block: the exact decoded size (size_walk.hpp, WINDOW)
//         k_frames_layout  one wavefront per input: where every block and frame lies in the input's output, the content size
//                          check, the load-time code with the smallest position, and the lists the decode works from
// decode: k_frames_place   the engine call's arrays for the compressed blocks of independent frames (the caller's outOff)
//         (the engine's own decode over that list: frames.cpp)
//         k_frames_stored  stored blocks of independent frames
//         k_decode_frames_linked   one wavefront per linked frame, blocks in order, the frame's last 64 KiB as dictionary
//         k_frames_check, k_frames_finish, k_frames_result   block verdicts, content checksums, result[]
//
// Everything a frame says is checked against the input's own range before it is used, and every block is decoded into exactly the
// size the load found, with [buf, buf + bufLen) as read bounds: whatever buf holds at decode time, nothing is written outside the
// inputs' output ranges.

__device__ __forceinline__ uint32_t frm_rd32(const uint8_t *p) { return (uint32_t)uni((int)xxh_word(p)); }
__device__ __forceinline__ uint32_t frm_rd8(const uint8_t *p) { return (uint32_t)uni((int)as_global(p)[0]); }

// xxh32 (seed 0) of the 2 or 10 bytes of a frame descriptor, in place: under 16 bytes there are no stripes
__device__ __forceinline__ uint32_t frm_xxh_small(const uint8_t *p, int len)
{
    uint32_t h = XXH_P5 + (uint32_t)len;
    int k = 0;
    for (; k + 4 <= len; k += 4) h = xxh_rotl(h + frm_rd32(p + k) * XXH_P3, 17) * XXH_P4;
    for (; k < len; k++) h = xxh_rotl(h + frm_rd8(p + k) * XXH_P5, 11) * XXH_P1;
    h ^= h >> 15; h *= XXH_P2;
    h ^= h >> 13; h *= XXH_P3;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ unsigned long long frm_key(uint64_t pos, int code)
{
    return ((unsigned long long)pos << 4) | (unsigned long long)(uint32_t)(-0x7F000100 - code);
}
__device__ __forceinline__ int frm_key_code(unsigned long long key) { return -0x7F000100 - (int)(key & 15u); }

// The walk over input i: frames, skippable frames, block words.  Every value is the same in all lanes (the chain of block words
// is serial by format: one dependent load per block); lane 0 stores.  FILL: write the tables at the places the scans gave.
template <bool FILL>
__device__ __forceinline__ void frames_walk(const FramesArgs &a, int i)
{
    const int lane = lane_id();
    const uint64_t off = (uint64_t)uni64((int64_t)a.inOff[i]), L = (uint64_t)uni64((int64_t)a.inLen[i]);
    uint64_t nF = 0, nB = 0, errPos = 0;
    int err = 0;
    // FILL: the places the scans gave, and their ends -- the tables were sized by the first walk, and a second walk that finds more
    // (a caller who changed buf in between) stops there instead of writing past them
    uint64_t fBase = 0, bBase = 0, fRoom = ~0ull, bRoom = ~0ull;
    if (FILL) {
        fBase = (uint64_t)uni64((int64_t)a.frameFirst[i]); bBase = (uint64_t)uni64((int64_t)a.blockFirst[i]);
        fRoom = (uint64_t)uni64((int64_t)a.frameFirst[i + 1]) - fBase; bRoom = (uint64_t)uni64((int64_t)a.blockFirst[i + 1]) - bBase;
    }
    if (off > a.bufLen || L > a.bufLen - off) { err = FRM_E_TRUNCATED; errPos = 0; }
    else {
        const uint8_t *in = a.buf + off;
        uint64_t pos = 0;
        while (pos < L) {
            errPos = pos;                                               // header errors sit at the frame's magic
            if (L - pos < 4) { err = FRM_E_TRUNCATED; break; }
            const uint32_t magic = frm_rd32(in + pos);
            if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {                 // skippable frame
                if (L - pos < 8) { err = FRM_E_TRUNCATED; break; }
                const uint32_t len = frm_rd32(in + pos + 4);
                if (L - pos - 8 < (uint64_t)len) { err = FRM_E_TRUNCATED; break; }
                pos += 8 + (uint64_t)len;
                continue;
            }
            if (magic != 0x184D2204u) { err = FRM_E_MAGIC; break; }
            if (nF >= fRoom) { err = FRM_E_TRUNCATED; break; }
            if (L - pos < 6) { err = FRM_E_TRUNCATED; break; }
            const uint32_t flg = frm_rd8(in + pos + 4), bd = frm_rd8(in + pos + 5);
            const uint32_t code = (bd >> 4) & 7u;
            if ((flg >> 6) != 1u || (flg & 3u) || code < 4u || (bd & 0x8Fu)) { err = FRM_E_HEADER; break; }
            const int dlen = 2 + ((flg & 8u) ? 8 : 0);
            if (L - pos < (uint64_t)(4 + dlen + 1)) { err = FRM_E_TRUNCATED; break; }
            if (frm_rd8(in + pos + 4 + dlen) != ((frm_xxh_small(in + pos + 4, dlen) >> 8) & 0xffu)) { err = FRM_E_HEADER_CHECKSUM; break; }
            FrmFrame fr;
            fr.declared = (flg & 8u) ? ((uint64_t)frm_rd32(in + pos + 6) | ((uint64_t)frm_rd32(in + pos + 10) << 32)) : 0;
            fr.blockMax = 1u << (8 + 2 * code);
            fr.flags = flg; fr.checksum = 0; fr.endPos = 0; fr.outRel = 0; fr.size = 0;
            fr.input = i; fr.firstBlock = (int32_t)(bBase + nB); fr.nBlocks = 0;
            const uint32_t trailer = (flg & 0x10u) ? 4u : 0u;
            uint64_t p = pos + 4 + (uint64_t)dlen + 1;
            for (;;) {
                errPos = p;                                             // block errors sit at the block's size word
                if (L - p < 4) { err = FRM_E_TRUNCATED; break; }
                const uint32_t word = frm_rd32(in + p);
                if (word == 0u) {                                       // end mark; content errors sit here
                    fr.endPos = off + p;
                    p += 4;
                    if (flg & 4u) {
                        if (L - p < 4) { err = FRM_E_TRUNCATED; break; }
                        fr.checksum = frm_rd32(in + p);
                        p += 4;
                    }
                    break;
                }
                const uint32_t n = word & 0x7FFFFFFFu;
                if (n > fr.blockMax) { err = FRM_E_BLOCK_SIZE; break; }
                if (L - p - 4 < (uint64_t)n + trailer || nB >= bRoom) { err = FRM_E_TRUNCATED; break; }
                if (FILL && lane == 0) {
                    FrmBlock b;
                    b.payOff = off + p + 4; b.outRel = 0; b.n = word; b.frame = (int32_t)(fBase + nF); b.size = 0; b.kind = FRM_K_NONE;
                    a.blocks[bBase + nB] = b;
                }
                nB++; fr.nBlocks++;
                p += 4 + (uint64_t)n + trailer;
            }
            if (err) { fr.flags |= FRM_F_BROKEN; fr.endPos = off + errPos; }
            if (FILL && lane == 0) a.frames[fBase + nF] = fr;
            nF++;
            if (err) break;
            pos = p;
        }
    }
    if (!FILL && lane == 0) {
        a.nFrames[i] = (int32_t)min(nF, (uint64_t)0x7fffffff);
        a.nBlocks[i] = (int32_t)min(nB, (uint64_t)0x7fffffff);
        a.err[i] = err;
        a.errPos[i] = off + errPos;
    }
}

__global__ __launch_bounds__(LZ4_WAVE) void k_frames_scan(FramesArgs a) { frames_walk<false>(a, (int)blockIdx.x); }
__global__ __launch_bounds__(LZ4_WAVE) void k_frames_fill(FramesArgs a) { frames_walk<true>(a, (int)blockIdx.x); }

// bsumFail[b] = the block's bytes as stored do not match the xxh32 behind them (0 where the frame has none, or the caller skips them)
__global__ __launch_bounds__(256) void k_frames_bsum(FramesArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int b = (int)(t >> 2), q = (int)(t & 3);
    const uint8_t *p = a.buf;
    int64_t L = -1;
    if (b < a.nBlocksAll) {
        const FrmBlock blk = a.blocks[b];
        if (a.frames[blk.frame].flags & 0x10u) { p = a.buf + blk.payOff; L = (int64_t)(blk.n & 0x7FFFFFFFu); }
    }
    const uint32_t h = xxh32_group(p, L, 0u, q);
    if (q == 0 && b < a.nBlocksAll) a.bsumFail[b] = (L >= 0 && h != xxh_word(p + L)) ? 1 : 0;
}

// size of every block: a stored block's is its length, a compressed block's is read off its token chain (a persistent grid, as
// k_decoded_size).  The frame's block maximum bounds it: no conforming writer puts more into a block.
__global__ __launch_bounds__(LZ4_WAVE) void k_frames_sizes(FramesArgs a)
{
    __shared__ SizeLds lds;
    const int lane = lane_id();
    if (lane < 4) ((uint32_t *)&lds.win[SW_WIN])[lane] = 0u;
    if (lane < 2) lds.nz[SW_WIN / 32 + lane] = 0u;
    wave_fence();
    for (int b = (int)blockIdx.x; b < a.nBlocksAll; b += (int)gridDim.x) {
        const uint64_t payOff = (uint64_t)uni64((int64_t)a.blocks[b].payOff);
        const uint32_t word = (uint32_t)uni((int)a.blocks[b].n);
        const int n = (int)(word & 0x7FFFFFFFu);
        int r = n;
        if (!(word & 0x80000000u)) {
            const int bmax = uni((int)a.frames[uni(a.blocks[b].frame)].blockMax);
            // A block of one byte is a token alone: the empty block 0x00 (size 0, size_walk.hpp rule 4), or a field that leaves the
            // block.  It is answered here: in this instantiation the compiler folded the walk's own `s == 0` exit into "no size"
            // whatever the byte, and every frame with such a block was refused at load.
            if (n == 1) r = (frm_rd8(a.buf + payOff) == 0u) ? 0 : SIZE_E_UNKNOWN;
            else r = decoded_size_block<true>(a.buf + payOff, n, bmax, a.buf, a.buf + a.bufLen, lds);
        }
        if (lane == 0) a.blocks[b].size = r;
    }
}

// One wavefront per input: segmented scans of the block sizes (a block's and a frame's place in the input's output), the
// content size check, the load-time code with the smallest position -- and, for an input that stands, what the decode does with
// each block and the two lists it works from.
__global__ __launch_bounds__(LZ4_WAVE) void k_frames_layout(FramesArgs a)
{
    const int i = (int)blockIdx.x, lane = lane_id();
    const int f0 = (int)uni64((int64_t)a.frameFirst[i]), f1 = (int)uni64((int64_t)a.frameFirst[i + 1]);
    int best = uni(a.err[i]);
    uint64_t bestPos = (uint64_t)uni64((int64_t)a.errPos[i]);
    uint64_t total = 0;
    for (int f = f0; f < f1; f++) {
        const uint32_t flags = (uint32_t)uni((int)a.frames[f].flags);
        const int b0 = uni(a.frames[f].firstBlock), b1 = b0 + uni(a.frames[f].nBlocks);
        uint64_t fsz = 0;
        for (int c = b0; c < b1; c += LZ4_WAVE) {
            const int b = c + lane;
            const bool act = b < b1;
            const int sz = act ? a.blocks[b].size : 0;
            const bool ck = act && !(a.flags & FRM_SKIP_BLOCK_CHECKSUM) && a.bsumFail[b] != 0;
            const bool bad = ck || sz < 0;
            const int s = max(sz, 0);
            const int incl = par_scan_incl(s);
            if (act) a.blocks[b].outRel = total + fsz + (uint64_t)(uint32_t)(incl - s);
            fsz += (uint64_t)(uint32_t)__builtin_amdgcn_readlane(incl, LZ4_WAVE - 1);
            const uint64_t m = __ballot(bad);
            if (m) {
                const int l = (int)__builtin_ctzll(m);
                const uint64_t pos = (uint64_t)uni64((int64_t)a.blocks[c + l].payOff) - 4u;
                const int code = __builtin_amdgcn_readlane(ck ? FRM_E_BLOCK_CHECKSUM : FRM_E_BLOCK, l);
                if (!best || pos < bestPos) { best = code; bestPos = pos; }
            }
        }
        if (lane == 0) { a.frames[f].outRel = total; a.frames[f].size = fsz; }
        if (!(flags & FRM_F_BROKEN) && (flags & 8u)) {
            const uint64_t declared = (uint64_t)uni64((int64_t)a.frames[f].declared);
            const uint64_t endPos = (uint64_t)uni64((int64_t)a.frames[f].endPos);
            if (declared != fsz && (!best || endPos < bestPos)) { best = FRM_E_CONTENT_SIZE; bestPos = endPos; }
        }
        total += fsz;
    }
    if (lane == 0) a.sizes[i] = best ? (int64_t)best : (int64_t)total;
    for (int f = f0; f < f1; f++) {
        const uint32_t flags = (uint32_t)uni((int)a.frames[f].flags);
        const int b0 = uni(a.frames[f].firstBlock), b1 = b0 + uni(a.frames[f].nBlocks);
        const bool linked = !(flags & 0x20u);
        if (!best && linked && b1 > b0 && lane == 0) a.linked[atomicAdd(&a.counts[1], 1u)] = f;
        for (int c = b0; c < b1; c += LZ4_WAVE) {
            const int b = c + lane;
            int kind = FRM_K_NONE;
            if (b < b1 && !best) {
                const uint32_t word = a.blocks[b].n;
                if (word & 0x7FFFFFFFu) kind = linked ? FRM_K_LINKED : ((word & 0x80000000u) ? FRM_K_STORED : FRM_K_COMP);
            }
            if (b < b1) a.blocks[b].kind = kind;
            const uint64_t m = __ballot(kind == FRM_K_COMP);
            if (m) {
                uint32_t base = 0;
                if (lane == 0) base = atomicAdd(&a.counts[0], (uint32_t)__builtin_popcountll(m));
                base = (uint32_t)uni((int)base);
                if (kind == FRM_K_COMP) a.indep[base + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = b;
            }
        }
    }
}

static int frames_cus()
{
    static std::atomic<int> cus[64];                                    // CUs per device, asked for once
    int dev = 0;
    (void)hipGetDevice(&dev);
    int nc = cus[dev & 63].load(std::memory_order_relaxed);
    if (nc <= 0) {
        if (hipDeviceGetAttribute(&nc, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || nc <= 0) nc = 256;
        cus[dev & 63].store(nc, std::memory_order_relaxed);
    }
    return nc;
}

void launch_frames_scan(const FramesArgs &a, hipStream_t s)
{
    if (a.nInputs <= 0) return;
    hipLaunchKernelGGL(k_frames_scan, dim3((unsigned)a.nInputs), dim3(LZ4_WAVE), 0, s, a);
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, s, (const int32_t *)a.nFrames, a.nInputs, a.frameFirst);
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, s, (const int32_t *)a.nBlocks, a.nInputs, a.blockFirst);
}

void launch_frames_load(const FramesArgs &a, hipStream_t s)
{
    if (a.nInputs <= 0) return;
    hipLaunchKernelGGL(k_frames_fill, dim3((unsigned)a.nInputs), dim3(LZ4_WAVE), 0, s, a);
    if (a.nBlocksAll > 0) {
        hipLaunchKernelGGL(k_frames_bsum, dim3(xxh_groups(a.nBlocksAll)), dim3(256), 0, s, a);
        const unsigned grid = (unsigned)min(a.nBlocksAll, frames_cus() * 32);
        hipLaunchKernelGGL(k_frames_sizes, dim3(grid), dim3(LZ4_WAVE), 0, s, a);
    }
    hipLaunchKernelGGL(k_frames_layout, dim3((unsigned)a.nInputs), dim3(LZ4_WAVE), 0, s, a);
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_frames_place(FramesArgs a)
{
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t < a.nInputs) a.errKey[t] = ~0ull;
    if (t >= a.nIndep) return;
    const FrmBlock blk = a.blocks[a.indep[t]];
    a.decOff[t] = blk.payOff - 4u;                                      // the size word: the engine's 4-byte header
    a.decOut[t] = a.outOff[a.frames[blk.frame].input] + blk.outRel;
    a.decCap[t] = blk.size;
}

void launch_frames_place(const FramesArgs &a, hipStream_t s)
{
    const int n = max(a.nInputs, a.nIndep);
    if (n > 0) hipLaunchKernelGGL(k_frames_place, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
}

// stored blocks of independent frames: a persistent grid of waves, 16-byte stores where the destination is aligned
__global__ __launch_bounds__(LZ4_WAVE) void k_frames_stored(FramesArgs a)
{
    for (int b = (int)blockIdx.x; b < a.nBlocksAll; b += (int)gridDim.x) {
        if (uni(a.blocks[b].kind) != FRM_K_STORED) continue;
        const uint64_t payOff = (uint64_t)uni64((int64_t)a.blocks[b].payOff);
        const uint32_t n = (uint32_t)uni((int)a.blocks[b].n) & 0x7FFFFFFFu;
        const int input = uni(a.frames[uni(a.blocks[b].frame)].input);
        uint8_t *dst = a.out + (uint64_t)uni64((int64_t)a.outOff[input]) + (uint64_t)uni64((int64_t)a.blocks[b].outRel);
        wave_copy_bytes(dst, a.buf + payOff, n);
    }
}

// One wavefront per linked frame (the pattern of k_decode_dstreams): blocks in order, each with the up to 65536 bytes of this
// frame's output directly in front of it as its dictionary -- across stored and short blocks, which is the frame format's
// window and not the engine's "block before".  A block that does not come out at its size stops the frame.
__global__ PAR_OCC void k_decode_frames_linked(FramesArgs a)
{
    __shared__ ParLds lds;
    const int f = uni(a.linked[blockIdx.x]);
    const int input = uni(a.frames[f].input);
    const int b0 = uni(a.frames[f].firstBlock), b1 = b0 + uni(a.frames[f].nBlocks);
    uint8_t *base = a.out + (uint64_t)uni64((int64_t)a.outOff[input]) + (uint64_t)uni64((int64_t)a.frames[f].outRel);
    uint64_t done = 0;
    for (int b = b0; b < b1; b++) {
        const uint32_t word = (uint32_t)uni((int)a.blocks[b].n);
        const int n = (int)(word & 0x7FFFFFFFu);
        if (n == 0) continue;
        const uint64_t payOff = (uint64_t)uni64((int64_t)a.blocks[b].payOff);
        const int size = uni(a.blocks[b].size);
        uint8_t *dst = base + done;
        int r = n;
        if (word & 0x80000000u) wave_copy_bytes(dst, a.buf + payOff, (uint32_t)n);
        else {
            const uint32_t hist = (uint32_t)min(done, (uint64_t)65536);
            r = uni(decode_block_par<false, true>(a.buf + payOff, n, dst, size, dst - hist, hist, a.buf, a.buf + a.bufLen, lds, nullptr));
        }
        if (r != size) {
            if (lane_id() == 0) atomicMin((unsigned long long *)&a.errKey[input], frm_key(payOff - 4u, FRM_E_BLOCK));
            break;
        }
        done += (uint64_t)(uint32_t)size;
        wave_fence();       // (the next block reads this one through the pipeline that wrote it, see k_decode_fixup_linked)
    }
}

// the engine's verdicts on the compressed blocks of independent frames
__global__ __launch_bounds__(256) void k_frames_check(FramesArgs a)
{
    const int t = (int)(blockIdx.x * 256u + threadIdx.x);
    if (t >= a.nIndep || a.decRes[t] == a.decCap[t]) return;
    const FrmBlock blk = a.blocks[a.indep[t]];
    atomicMin((unsigned long long *)&a.errKey[a.frames[blk.frame].input], frm_key(blk.payOff - 4u, FRM_E_BLOCK));
}

// content checksums, four lanes per frame: xxh32 is four serial chains per range, so one huge frame is checked by four lanes
__global__ __launch_bounds__(256) void k_frames_finish(FramesArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int f = (int)(t >> 2), q = (int)(t & 3);
    const uint8_t *p = a.out;
    int64_t L = -1;
    int input = 0;
    if (f < a.nFramesAll && !(a.flags & FRM_SKIP_CONTENT_CHECKSUM)) {
        const FrmFrame fr = a.frames[f];
        input = fr.input;
        if ((fr.flags & 4u) && !(fr.flags & FRM_F_BROKEN) && a.sizes[input] >= 0) {
            p = a.out + a.outOff[input] + fr.outRel;
            L = (int64_t)fr.size;
        }
    }
    const uint32_t h = xxh32_group(p, L, 0u, q);
    if (q == 0 && L >= 0 && h != a.frames[f].checksum)
        atomicMin((unsigned long long *)&a.errKey[input], frm_key(a.frames[f].endPos, FRM_E_CONTENT_CHECKSUM));
}

__global__ __launch_bounds__(256) void k_frames_result(FramesArgs a)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= a.nInputs) return;
    const int64_t s = a.sizes[i];
    const unsigned long long key = a.errKey[i];
    a.result[i] = (s < 0 || key == ~0ull) ? s : (int64_t)frm_key_code(key);
}

void launch_frames_decode(const FramesArgs &a, hipStream_t s)
{
    if (a.nInputs <= 0) return;
    if (a.nBlocksAll > 0) {
        const unsigned grid = (unsigned)min(a.nBlocksAll, frames_cus() * 32);
        hipLaunchKernelGGL(k_frames_stored, dim3(grid), dim3(LZ4_WAVE), 0, s, a);
    }
    if (a.nLinked > 0) hipLaunchKernelGGL(k_decode_frames_linked, dim3((unsigned)a.nLinked), dim3(64), 0, s, a);
    if (a.nIndep > 0) hipLaunchKernelGGL(k_frames_check, dim3((unsigned)((a.nIndep + 255) / 256)), dim3(256), 0, s, a);
    if (a.nFramesAll > 0) hipLaunchKernelGGL(k_frames_finish, dim3(xxh_groups(a.nFramesAll)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_frames_result, dim3((unsigned)((a.nInputs + 255) / 256)), dim3(256), 0, s, a);
}
