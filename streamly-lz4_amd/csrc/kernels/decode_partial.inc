// kernels/decode_partial.inc -- partial decode: the first N bytes of every block, in the three forms.
// A part of kernels.hip, the one device translation unit: included there, in this order, and not compiled on its own.
// ---- partial decode: the first min(target, capacity) bytes of every block (LZ4_decompress_safe_partial, cbits/lz4.c:2179-2185) ----
// Kernel entries of their own over the same device functions with PARTIAL set: the full-decode kernels above keep their code and
// their registers.  `end` is the reference's dstCapacity after :2181; no byte at or behind out + outOff[blk] + end is written.
__device__ __forceinline__ int read_block_header_partial(const DecodeArgs &a, int blk, const uint8_t *&data, int &compLen, int &cap,
                                                         int &end)
{
    const int r = read_block_header(a, blk, data, compLen, cap);
    if (r) return r;
    const int t = a.target[blk];
    if (t < 0) return BLK_E_UNCOMPLEN;
    end = min(t, cap);
    return 0;
}

__global__ __launch_bounds__(256, 6) void k_decode_seq_partial(DecodeArgs a)
{
    const int blk = uni((int)((blockIdx.x * 256u + threadIdx.x) >> 6));
    if (blk >= a.nBlocks) return;
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0, end = 0;
    int r = read_block_header_partial(a, blk, data, compLen, cap, end);
    if (r == 0)
        r = decode_block_seq<false, true>(data, compLen, a.out + a.outOff[blk], end, nullptr, 0, a.framed, a.framed + a.framedLen);
    if (lane_id() == 0) a.result[blk] = r;
}

// REDO: only the blocks k_decode_cu_partial left behind
template <bool REDO>
__global__ PAR_OCC void k_decode_par_partial(DecodeArgs a)
{
    __shared__ ParLds lds;
    const int blk = (int)blockIdx.x;
    if (REDO && uni(a.result[blk]) != CU_REDO) return;
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0, end = 0;
    int r = read_block_header_partial(a, blk, data, compLen, cap, end);
    if (r == 0)
        r = decode_block_par<false, false, false, false, true>(data, compLen, a.out + a.outOff[blk], end, nullptr, 0, a.framed,
                                                               a.framed + a.framedLen, lds, nullptr);
    if (lane_id() == 0) a.result[blk] = r;
}

// The workgroup form takes the blocks whose target does not cut them short (end == capacity): a full decode that succeeds gives what
// the partial mode gives -- with the output end at the capacity no rule of the partial mode clips anything of a block the full mode
// accepts -- and a block it does not finish is CU_REDO as ever.  A block that IS cut short is left to the lane-parallel form at once
// (the route cuBail uses): a prefix is a fraction of a 32 KiB segment, which is all a workgroup could be kept busy with.
__global__ __launch_bounds__(CU_THREADS) void k_decode_cu_partial(DecodeArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[CU_LDS_BYTES];
    const int blk = (int)blockIdx.x;
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0, end = 0;
    int r = uni(read_block_header_partial(a, blk, data, compLen, cap, end));
    if (r == 0 && uni(end) < uni(cap)) r = CU_REDO;
    else if (r == 0)
        r = decode_block_cu<false>(data, uni(compLen), a.out + a.outOff[blk], uni(cap), nullptr, 0, a.framed, a.framed + a.framedLen, lds,
                                   nullptr, false);
    if (threadIdx.x == 0) a.result[blk] = r;
}

void launch_decode_partial(const DecodeArgs &a, int form, hipStream_t s)
{
    if (a.nBlocks <= 0) return;
    if (form == 1) {
        hipLaunchKernelGGL(k_decode_seq_partial, dim3((unsigned)((a.nBlocks + 3) / 4)), dim3(256), 0, s, a);
    } else if (form == 4) {
        hipLaunchKernelGGL(k_decode_cu_partial, dim3((unsigned)a.nBlocks), dim3(CU_THREADS), 0, s, a);
        hipLaunchKernelGGL(k_decode_par_partial<true>, dim3((unsigned)a.nBlocks), dim3(64), 0, s, a);
    } else {
        hipLaunchKernelGGL(k_decode_par_partial<false>, dim3((unsigned)a.nBlocks), dim3(64), 0, s, a);
    }
}
