// kernels/decode_seq.inc -- block header checks, the link summary (k_link_stat) and the sequential decoder's kernel (decode_seq.hpp).
// A part of kernels.hip, the one device translation unit: included there, in this order, and not compiled on its own.
// ---------------------------------------------------------------------------
// K1: decode
// ---------------------------------------------------------------------------

// Validate one block header the way decompressChunk does
// (reference src/Streamly/Internal/LZ4.hs:299-318) -- plus the short-array case
// it misses.  Returns 0 or a MI355LZ4_BLK_E_* code; fills compLen / cap.
__device__ __forceinline__ int read_block_header(const DecodeArgs &a, int blk, const uint8_t *&data,
                                                 int &compLen, int &cap)
{
    const uint64_t off = a.blockOff[blk];
    if (off + (uint64_t)a.headerKind > a.framedLen) return BLK_E_TRUNCATED;
    const uint8_t *hdr = a.framed + off;
    compLen = load_le32(hdr);
    int uncomp = (a.headerKind == 8) ? load_le32(hdr + 4) : a.fixedUncomp;
    if (compLen <= 0 || compLen > MAX_COMP_LEN) return BLK_E_COMPLEN;
    if (off + (uint64_t)a.headerKind + (uint64_t)compLen > a.framedLen) return BLK_E_TRUNCATED;
    if (a.ckFail) {                                   // block checksums: the trailer, verified by k_xxh32_verify beforehand
        if (off + (uint64_t)a.headerKind + (uint64_t)compLen + 4u > a.framedLen) return BLK_E_TRUNCATED;
        if (a.ckFail[blk]) return BLK_E_CHECKSUM;
    }
    if (uncomp < 0) return BLK_E_UNCOMPLEN;
    cap = uncomp;
    if (a.outCap) {
        if (a.headerKind == 8 && uncomp > a.outCap[blk]) return BLK_E_UNCOMPLEN;
        if (a.headerKind != 8) cap = a.outCap[blk];
    }
    data = hdr + a.headerKind;
    return 0;
}

// A codec error (not a header rejection) is what a block of a linked stream reports when it is decoded without
// its dictionary: the second pass is launched only when the standalone pass counted some.
__device__ __forceinline__ bool is_codec_error(int r) { return r < 0 && r > -0x7F000000; }

// linkStat = {dependent blocks, first, last, -, largest capacity among them}, from result[] once the standalone pass
// is done.  (Round 3 had every failing block add to these five words itself: four atomics per block on ONE cache line,
// 16 384 of them for a reference-written stream of 4096 blocks, which cost the standalone pass 0.33 of its 0.38 ms --
// the blocks themselves give up at their first sequence.)  One workgroup per 1024 blocks, one set of atomics each.
#define LINK_RUN_CAP 64
__global__ __launch_bounds__(1024) void k_link_stat(DecodeArgs a)
{
    __shared__ uint32_t sh[4];
    const int tid = (int)threadIdx.x;
    if (tid == 0) { sh[0] = 0u; sh[1] = 0xffffffffu; sh[2] = 0u; sh[3] = 0u; }
    __syncthreads();
    const int blk = (int)(blockIdx.x * 1024u) + tid;
    bool bad = false;
    int cap = 0;
    if (blk < a.nBlocks && is_codec_error(a.result[blk])) {
        const uint8_t *data = nullptr;
        int compLen = 0;
        bad = read_block_header(a, blk, data, compLen, cap) == 0;     // (a codec error means the header was accepted)
    }
    const uint64_t m = __ballot(bad);
    if (m) {
        // wave-level first: one lane per wave talks to LDS
        int wcap = bad ? cap : 0;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) wcap = max(wcap, __shfl_xor(wcap, d));
        if ((tid & 63) == 0) {
            const int w0 = blk;                                        // first lane's block
            atomicAdd(&sh[0], (uint32_t)__builtin_popcountll(m));
            atomicMin(&sh[1], (uint32_t)(w0 + (int)__builtin_ctzll(m)));
            atomicMax(&sh[2], (uint32_t)(w0 + 63 - (int)__builtin_clzll(m)));
            atomicMax(&sh[3], (uint32_t)wcap);
        }
    }
    // linkStat[5] = the longest run of consecutive blocks that produced no output (capped at LINK_RUN_CAP + 1): how long
    // the serial part is when every run is walked by a wave of its own (k_decode_fixup_runs).  Only a run's first block
    // counts it.
    if (blk < a.nBlocks && a.result[blk] <= 0 && (blk == 0 || a.result[blk - 1] > 0)) {
        int n = 1;
        while (n <= LINK_RUN_CAP && blk + n < a.nBlocks && a.result[blk + n] <= 0) n++;
        atomicMax(&a.linkStat[5], (uint32_t)n);
        atomicAdd(&a.linkStat[6], 1u);                             // ... and how many runs there are (k_run_starts' list)
    }
    __syncthreads();
    if (tid == 0 && sh[0]) {
        atomicAdd(&a.linkStat[0], sh[0]);
        atomicMin(&a.linkStat[1], sh[1]);
        atomicMax(&a.linkStat[2], sh[2]);
        atomicMax(&a.linkStat[4], sh[3]);          // the largest such block sizes the second pass's scratch
    }
}
void launch_link_stat(const DecodeArgs &a, hipStream_t s)
{
    if (a.linkStat && a.nBlocks > 0)
        hipLaunchKernelGGL(k_link_stat, dim3((unsigned)((a.nBlocks + 1023) / 1024)), dim3(1024), 0, s, a);
}

// One wavefront per block, 4 blocks per 256-thread workgroup.
__global__ __launch_bounds__(256, 6) void k_decode_seq(DecodeArgs a)
{
    const int blk = uni((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    if (blk >= a.nBlocks) return;
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0;
    int r = read_block_header(a, blk, data, compLen, cap);
    if (r == 0)
        r = decode_block_seq(data, compLen, a.out + a.outOff[blk], cap, nullptr, 0, a.framed,
                             a.framed + a.framedLen);
    if (lane_id() == 0) a.result[blk] = r;
}

void launch_decode_seq(const DecodeArgs &a, hipStream_t s)
{
    if (a.nBlocks <= 0) return;
    const unsigned grid = (unsigned)((a.nBlocks + 3) / 4);
    hipLaunchKernelGGL(k_decode_seq, dim3(grid), dim3(256), 0, s, a);
    launch_link_stat(a, s);
}
