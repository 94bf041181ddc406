// kernels_hstreams.hip -- k_encode_hc_fstreams: the fast linked streams of a set whose level is 1..12 (mi355lz4_fstreams_set_level,
// DESIGN.md 7q), and the launch of that one kernel.
//
// A translation unit of its own, for the reason kernels.hip gives for being one: the inliner decides by who else is
// in the module.  This kernel is a second caller of encode_block_hc<false>.  Inside kernels.hip that took the encoder out of line
// in k_encode_hc (116 VGPRs and 8 bytes of scratch against 69 and none); inlined here by name and defined in front of k_encode_hc
// it still moved that kernel's scalar spills (41 against 39).  Compiled apart, no kernel of kernels.hip sees it, and the module's
// device code is the parent's instruction for instruction.  What it shares with kernels/encode.inc is source: the block and slot
// helpers of kernels/encode_common.inc.  k_fstreams_plan and k_fstreams_save, which run in front of and behind it, stay where
// they are; launch_fstreams_hc (kernels/encode.inc) puts the three on the stream.
#include "kernels.h"

#include "encode_hc.hpp"

using namespace lz4dev;

#include "kernels/encode_common.inc"

// encode_block_hc in a linked call inserts the block directly in front, at most its last 64 KiB, and nothing older: block k depends
// on the tail of block k - 1, on itself and on the chain depth, as under the wave encoder.  So the kernel is k_encode_hc -- one
// workgroup of HC_THREADS per block on a persistent grid, all of a CU's LDS -- with k_encode_fstreams' choice of D: the slot's bytes
// for a stream's first block of the call, the tail of the block before it for every other.  A block at or behind its stream's
// good[] gets framedLen 0 and nothing else.  A block under 13 bytes, one with an empty D and one whose D ends exactly where it
// starts are encoded where they lie; every other block is staged, D so that it ends at byte 65536 of the workgroup's window and the
// block behind it, as k_encode_hc_dict stages.  The slots are only read here.  All addresses are 64-bit.
__global__ __launch_bounds__(HC_THREADS) void k_encode_hc_fstreams(FStreamsArgs x, int depth)
{
    __shared__ HcLds L;
    const int t = (int)threadIdx.x, wave = t >> 6;
    const EncodeArgs &a = x.e;
    uint8_t *blockAt = x.stage + (uint64_t)blockIdx.x * (uint64_t)x.stageStride + 65536;
    for (int blk = (int)blockIdx.x; blk < a.nBlocks; blk += (int)gridDim.x) {
        const int w = min(max(uni(x.blockStream[blk]), 0), x.nWork - 1);
        const int32_t *e = x.work + 3 * (size_t)w;
        const int b0 = uni(e[0]);
        if (blk >= uni(x.good[w])) {
            if (t == 0) a.framedLen[blk] = 0;
            continue;
        }
        const EncBlock b = enc_block(a, blk);
        const int n = min(max(uni(b.n), 0), a.uniformLen);              // (inside already: the block is in front of good[w])
        const uint8_t *src = a.src + uni64((int64_t)b.off);
        uint8_t *slot = a.slots + (size_t)blk * a.slotStride;
        int dictLen = 0;
        if (n >= LZ4_MFLIMIT + 1) {
            const uint8_t *dEnd;                                        // D = [dEnd - dictLen, dEnd)
            if (blk <= b0) {                                            // the stream's first block of the call: what the slot holds
                const uint8_t *st = x.state + (size_t)uni(e[2]) * FSTREAM_SLOT_BYTES;
                const uint32_t held = (uint32_t)uni((int32_t)as_global((const uint32_t *)(st + FSTREAM_COUNT_OFF))[0]);
                dictLen = (int)min(held, (uint32_t)FSTREAM_DICT_BYTES);
                dEnd = st + dictLen;
            } else {                                                    // the block before it (a good one: its length is inside)
                const EncBlock p = enc_block(a, blk - 1);
                const int pn = min(max(uni(p.n), 0), a.uniformLen);
                dictLen = min(pn, 65536);
                dEnd = a.src + uni64((int64_t)p.off) + pn;
            }
            if (dictLen > 0 && dEnd != src) {
                __syncthreads();                                        // wave 0 may still be writing the block before's last literals from the window
                wg_copy_pieces(blockAt - dictLen, dEnd - dictLen, (uint32_t)dictLen, 4096u, (uint32_t)wave, HC_WAVES);
                wg_copy_pieces(blockAt, src, (uint32_t)n, 1024u, (uint32_t)wave, HC_WAVES);
                src = blockAt;                                          // (encode_block_hc's first barrier is behind both copies)
            }
        }
        const int c = encode_block_hc<false>(L, src, n, dictLen, slot + a.headerKind, depth);
        enc_finish_slot(a, blk, slot, c, n, t == 0);
    }
}

void launch_encode_hc_fstreams(const FStreamsArgs &a, int grid, int depth, hipStream_t s)
{
    hipLaunchKernelGGL(k_encode_hc_fstreams, dim3((unsigned)grid), dim3(HC_THREADS), 0, s, a, depth);
}
