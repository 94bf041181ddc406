// kernels/decode_par_cu.inc -- first-pass decode: the lane-parallel form (decode_par.hpp), the workgroup form (decode_cu.hpp) and its big linked blocks.
// A part of kernels.hip, the one device translation unit: included there, in this order, and not compiled on its own.
// Lane-parallel decoder (decode_par.hpp): one wavefront (= one workgroup) per block.
#ifdef PAR_WAVES_MAX
#define PAR_OCC __attribute__((amdgpu_flat_work_group_size(64, 64), amdgpu_waves_per_eu(PAR_WAVES, PAR_WAVES_MAX)))
#else
#define PAR_OCC __launch_bounds__(64, PAR_WAVES)
#endif
// The two kernels of this file that decode whole independent blocks run at eight waves per SIMD (PAR_WAVES_MAIN: 64 registers, 32 waves and all of the LDS of a CU); every other user of ParLds keeps PAR_OCC.
#ifdef PAR_WAVES_MAX
#define PAR_OCC_MAIN __attribute__((amdgpu_flat_work_group_size(64, 64), amdgpu_waves_per_eu(PAR_WAVES_MAIN, (PAR_WAVES_MAX > PAR_WAVES_MAIN ? PAR_WAVES_MAX : PAR_WAVES_MAIN))))
#else
#define PAR_OCC_MAIN __launch_bounds__(64, PAR_WAVES_MAIN)
#endif
template <bool STATS>
__global__ PAR_OCC_MAIN void k_decode_par(DecodeArgs a, unsigned long long *stats)
{
    __shared__ ParLds lds;
    const int blk = (int)blockIdx.x;
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0;
    int r = read_block_header(a, blk, data, compLen, cap);
    if (r == 0)
        r = decode_block_par<STATS, false>(data, compLen, a.out + a.outOff[blk], cap, nullptr, 0, a.framed,
                                    a.framed + a.framedLen, lds, stats);
    if (lane_id() == 0) a.result[blk] = r;
}

void launch_decode_par(const DecodeArgs &a, unsigned long long *stats, hipStream_t s)
{
    if (a.nBlocks <= 0) return;
    if (stats)
        hipLaunchKernelGGL(k_decode_par<true>, dim3((unsigned)a.nBlocks), dim3(64), 0, s, a, stats);
    else
        hipLaunchKernelGGL(k_decode_par<false>, dim3((unsigned)a.nBlocks), dim3(64), 0, s, a, stats);
    launch_link_stat(a, s);
}

// The blocks the workgroup-per-block decoder left behind (result CU_REDO), by the lane-parallel decoder.  (A kernel of its
// own, not a template parameter of k_decode_par: that changed the headline kernel's register allocation.)
__global__ PAR_OCC_MAIN void k_decode_par_redo(DecodeArgs a)
{
    __shared__ ParLds lds;
    const int blk = (int)blockIdx.x;
    if (uni(a.result[blk]) != CU_REDO) return;
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0;
    int r = read_block_header(a, blk, data, compLen, cap);
    if (r == 0)
        // (LIST with an empty list: the same decoder as k_decode_par's, but an instantiation of its own -- a second user of
        // k_decode_par's instantiation turns that kernel's inlined decoder into a call)
        r = decode_block_par<false, false, false, true>(data, compLen, a.out + a.outOff[blk], cap, nullptr, 0, a.framed,
                                                        a.framed + a.framedLen, lds, nullptr, nullptr, nullptr, 0);
    if (lane_id() == 0) a.result[blk] = r;
}

// Workgroup-per-block decoder (decode_cu.hpp): sixteen wavefronts per block, for calls that do not fill the GPU.
__global__ __launch_bounds__(CU_THREADS) void k_decode_cu(DecodeArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[CU_LDS_BYTES];
    const int blk = (int)blockIdx.x;
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0;
    int r = uni(read_block_header(a, blk, data, compLen, cap));
    // A block that hardly compresses is literal runs of hundreds of bytes: every one of them ends a segment (the parse follows two
    // extension bytes) and is copied by one wave, which is what the lane-parallel decoder does without the segments' fixed costs
    // (160 blocks of 64 KiB, ms, wavefront / workgroup form: ratio 1.00: 0.045 / 0.070; text at acceleration 64, ratio 1.01: 0.53 / 1.44;
    // lzsynth at 64, 1.03: 0.45 / 0.83; text at 16, ratio 1.14: 0.45 / 0.29 -- from there on the workgroup form is the faster one).
    if (r == 0 && a.cuBail && (int64_t)uni(compLen) * 16 > (int64_t)uni(cap) * 15) r = CU_REDO;
    else if (r == 0)
        r = decode_block_cu<false>(data, uni(compLen), a.out + a.outOff[blk], uni(cap), nullptr, 0, a.framed, a.framed + a.framedLen, lds,
                                   a.cuDbg ? a.cuDbg + 16 * (size_t)blk : nullptr, a.cuBail != 0);
    if (threadIdx.x == 0) a.result[blk] = r;
    // A linked call of big blocks (a.cu.res armed by the caller, launch_cu_linked below): a block that did not decode on its own is,
    // as a rule, one that needs its dictionary -- pass 1 of that path (the block against 64 KiB of zeros) follows at once, while the
    // stream's first block, which decodes on its own, is still at work.  (The redo launch still reports the exact code in result[].)
    // (The call's first block, when blocks lie in front of the call -- a later group of a host call, a.lookBack --, has a dictionary that
    // is FINAL: the last 64 KiB of the block in front of it; it is right after this one decode and is not looked at again.)
    const bool prevFinal = blk == 0 && a.lookBack > 0 && a.cu.res && uni(a.result[-1]) >= 65536;
    if (a.cu.res && (blk > 0 || prevFinal) && r == CU_REDO && !(a.cuBail && (int64_t)uni(compLen) * 16 > (int64_t)uni(cap) * 15)) {
        __syncthreads();
        const uint8_t *dict = prevFinal ? a.out + a.outOff[-1] + (size_t)uni(a.result[-1]) - 65536u : a.run.zeroPage;
        const int r2 = decode_block_cu<true>(data, uni(compLen), a.out + a.outOff[blk], uni(cap), dict, 65536u, a.framed,
                                            a.framed + a.framedLen, lds, nullptr, false, 0);
        if (threadIdx.x == 0) {
            a.cu.res[blk] = r2;
            if (r2 < 0 || (r2 < 65536 && blk + 1 < a.nBlocks)) atomicAdd(&a.cu.flags[1], 1u);   // an error, CU_REDO, or a block too short to be a whole dictionary
        }
    }
}

// ---- big linked blocks (a stream of BlockMax1MB / BlockMax4MB blocks, Config.hs:109-116, written with a dictionary carried from block
// to block, cbits/lz4.c:1608-1636): the workgroup form with a GUESSED dictionary.  A block of 1 MiB forgets a wrong dictionary long
// before its end (text: after 5 to 12 times 64 KiB), so its last 64 KiB -- all its successor can see of it -- come out right even when its
// own dictionary was wrong.  Pass 1 decodes every dependent block against 64 KiB of zeros, every later pass against a snapshot of what its
// predecessor's last 64 KiB were after the pass before, and when a pass changes no snapshot, every block has been decoded against its
// predecessor's final bytes: by induction from the stream's first block, which needs no dictionary, all of them are right.  The caller
// (api.cpp) bounds the passes and falls back to the pointer pass; results go to a.cu.res and are published at the end.
__global__ __launch_bounds__(CU_THREADS) void k_decode_cu_linked(DecodeArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[CU_LDS_BYTES];
    const int blk = (int)blockIdx.x;
    if (uni(a.result[blk]) >= 0) return;                                 // decoded on its own in the first pass: final
    const uint8_t *dict = nullptr;
    if (blk == 0) {
        // a first block that needs a dictionary: the call's own (dict0) is not this path's; the block in front of the call (a later
        // group of a host call) is final, and this block is decoded against its end once -- by the first launch, or here in pass 1
        const bool prevFinal = a.lookBack > 0 && uni(a.result[-1]) >= 65536;
        if (prevFinal && uni(a.cu.res[0]) >= 65536) return;
        if (!prevFinal || a.cu.pass != 1) { if (threadIdx.x == 0) atomicAdd(&a.cu.flags[1], 1u); return; }
        dict = a.out + a.outOff[-1] + (size_t)uni(a.result[-1]) - 65536u;
    } else {
        if (a.cu.pass > 2 && uni(a.cu.flags[2 + blk - 1]) == 0u) return;  // the dictionary it was decoded against last time still stands
        dict = a.cu.pass == 1 ? a.run.zeroPage : a.cu.snap + (size_t)(blk - 1) * 65536u;
    }
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0;
    int r = uni(read_block_header(a, blk, data, compLen, cap));
    if (r == 0)
        r = decode_block_cu<true>(data, uni(compLen), a.out + a.outOff[blk], uni(cap), dict, 65536u, a.framed, a.framed + a.framedLen, lds, nullptr, false,
                                  (blk > 0 && a.cu.pass > 1 && uni(a.cu.res[blk]) >= 65536) ? uni(a.cu.res[blk]) : 0);      // (from the second pass on: stop where the bytes repeat the pass before)
    if (threadIdx.x == 0) {
        a.cu.res[blk] = r;
        if (r < 0 || (r < 65536 && blk + 1 < a.nBlocks)) atomicAdd(&a.cu.flags[1], 1u);      // an error, CU_REDO, or a block too short to be a whole dictionary
    }
}

// the last 64 KiB of every block -> its snapshot; [2 + k] = whether that changed the snapshot, [0] = how many did
__global__ __launch_bounds__(1024) void k_cu_tails(DecodeArgs a)
{
    const int blk = (int)blockIdx.x;
    if (blk + 1 >= a.nBlocks) return;                                    // (nobody looks at the last block's)
    const int32_t r = a.result[blk] >= 0 ? a.result[blk] : a.cu.res[blk];
    __shared__ uint32_t diff;
    if (threadIdx.x == 0) diff = 0u;
    __syncthreads();
    uint32_t d = 0u;
    if (r >= 65536) {
        const uint8_t *tail = a.out + a.outOff[blk] + (size_t)r - 65536u;
        uint8_t *snap = a.cu.snap + (size_t)blk * 65536u;
        for (uint32_t i = threadIdx.x * 16u; i < 65536u; i += 1024u * 16u) {
            const par_v4 v = *(const par_v4u *)(tail + i), o = *(const par_v4 *)(snap + i);
            d |= (v.x ^ o.x) | (v.y ^ o.y) | (v.z ^ o.z) | (v.w ^ o.w);
            *(par_v4 *)(snap + i) = v;
        }
    }
    if (d) atomicOr(&diff, 1u);
    __syncthreads();
    if (threadIdx.x == 0) {
        // (a block that is no whole dictionary -- shorter than 64 KiB, or failed -- in front of a block that needs one: not this path's)
        if (r < 65536 && a.result[blk + 1] < 0) atomicAdd(&a.cu.flags[1], 1u);
        const uint32_t ch = (diff != 0u || a.cu.pass == 1) ? 1u : 0u;
        a.cu.flags[2 + blk] = ch;
        if (ch) atomicAdd(&a.cu.flags[0], 1u);
    }
}

__global__ __launch_bounds__(256) void k_cu_publish(DecodeArgs a)
{
    const int blk = (int)(blockIdx.x * 256u + threadIdx.x);
    if (blk < a.nBlocks && a.result[blk] < 0) a.result[blk] = a.cu.res[blk];
}

void launch_cu_linked(const DecodeArgs &a, bool decode, hipStream_t s)
{
    if (a.nBlocks <= 0) return;
    hipMemsetAsync(a.cu.flags, 0, 4, s);
    if (decode) hipLaunchKernelGGL(k_decode_cu_linked, dim3((unsigned)a.nBlocks), dim3(CU_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_cu_tails, dim3((unsigned)a.nBlocks), dim3(1024), 0, s, a);
}

void launch_cu_publish(const DecodeArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_cu_publish, dim3((unsigned)((a.nBlocks + 255) / 256)), dim3(256), 0, s, a);
}

void launch_decode_cu(const DecodeArgs &a, hipStream_t s)
{
    if (a.nBlocks <= 0) return;
    hipLaunchKernelGGL(k_decode_cu, dim3((unsigned)a.nBlocks), dim3(CU_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_decode_par_redo, dim3((unsigned)a.nBlocks), dim3(64), 0, s, a);
    launch_link_stat(a, s);
}
