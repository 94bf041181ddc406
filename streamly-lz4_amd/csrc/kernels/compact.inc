// kernels/compact.inc -- size scan, compaction into the framed stream, interleave, header sizes and decoded sizes (size_walk.hpp).
// A part of kernels.hip, the one device translation unit: included there, in this order, and not compiled on its own.
// ---------------------------------------------------------------------------
// K3: scan + ragged copy
// ---------------------------------------------------------------------------

// Exclusive scan of n int32 sizes into n+1 uint64 offsets; one 1024-thread workgroup.
// (n is the block count of a batch: at most a few million.)
__global__ __launch_bounds__(1024) void k_scan_u64(const int32_t *sizes, int n, uint64_t *offs)
{
    __shared__ uint64_t part[1024];
    const int t = (int)threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    uint64_t sum = 0;
    for (int i = lo; i < hi; i++) sum += (uint64_t)(uint32_t)max(sizes[i], 0);
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        uint64_t v = (t >= d) ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - sum;
    for (int i = lo; i < hi; i++) { offs[i] = run; run += (uint64_t)(uint32_t)max(sizes[i], 0); }
    if (t == 1023) offs[n] = part[1023];
}

// (for the translation units that hold no copy of the kernel: kernels_cframes.hip)
void launch_scan_u64(const int32_t *sizes, int n, uint64_t *offs, hipStream_t s)
{
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, s, sizes, n, offs);
}

// Copy n bytes with a 256-thread workgroup; dst gets 16-byte aligned stores in
// the body, src is read with (possibly unaligned) 16-byte loads.
__device__ __forceinline__ void wg_copy_bytes(uint8_t *dst, const uint8_t *src, uint64_t n)
{
    const uint32_t t = threadIdx.x, T = blockDim.x;
    uint64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
    if (head > n) head = n;
    if (t < head) dst[t] = src[t];
    const uint64_t body = (n - head) >> 4;
    uint4 *d16 = (uint4 *)(dst + head);
    const uint8_t *s16 = src + head;
    for (uint64_t i = t; i < body; i += T) {
        uint4 v;
        __builtin_memcpy(&v, s16 + (i << 4), 16);   // unaligned 16-byte global load
        d16[i] = v;
    }
    const uint64_t done = head + (body << 4);
    if (done + t < n) dst[done + t] = src[done + t];
}

__global__ __launch_bounds__(256) void k_copy_slots(const uint8_t *slots, size_t slotStride,
                                                    const int32_t *framedLen, const uint64_t *denseOff,
                                                    uint8_t *dense, uint64_t denseCap)
{
    const int blk = (int)blockIdx.x;
    const int n = framedLen[blk];
    const uint64_t at = denseOff[blk];
    if (n > 0 && at + (uint64_t)n <= denseCap) wg_copy_bytes(dense + at, slots + (size_t)blk * slotStride, (uint64_t)n);
}

void launch_compact(const uint8_t *slots, size_t slotStride, const int32_t *framedLen, int nBlocks,
                    uint8_t *dense, size_t denseCap, uint64_t *denseOff, hipStream_t s)
{
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, s, framedLen, nBlocks, denseOff);
    if (nBlocks > 0)
        hipLaunchKernelGGL(k_copy_slots, dim3((unsigned)nBlocks), dim3(256), 0, s, slots, slotStride,
                           framedLen, denseOff, dense, (uint64_t)denseCap);
}

__global__ __launch_bounds__(256) void k_interleave(const uint8_t *local, const uint64_t *localOff, int rank,
                                                    int nRanks, uint8_t *global, const uint64_t *globalOff)
{
    const int j = (int)blockIdx.x;
    const uint64_t n = localOff[j + 1] - localOff[j];
    wg_copy_bytes(global + globalOff[(size_t)j * nRanks + rank], local + localOff[j], n);
}

void launch_interleave(const uint8_t *local, const uint64_t *localOff, int nLocal, int rank, int nRanks,
                       uint8_t *global, const uint64_t *globalOff, hipStream_t s)
{
    if (nLocal > 0)
        hipLaunchKernelGGL(k_interleave, dim3((unsigned)nLocal), dim3(256), 0, s, local, localOff, rank,
                           nRanks, global, globalOff);
}

// Header gather for the output index: sizes[i] = uncompressed size of block i (0 if unreadable).
__global__ __launch_bounds__(256) void k_header_sizes(const uint8_t *framed, uint64_t framedLen,
                                                      const uint64_t *blockOff, int nBlocks, int headerKind,
                                                      int fixedUncomp, int32_t *sizes)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= nBlocks) return;
    int u = fixedUncomp;
    if (headerKind == 8) {
        const uint64_t off = blockOff[i];
        u = (off + 8 <= framedLen) ? load_le32(framed + off + 4) : 0;
    }
    sizes[i] = max(u, 0);
}

void launch_index(const uint8_t *framed, uint64_t framedLen, const uint64_t *blockOff, int nBlocks,
                  int headerKind, int fixedUncomp, int32_t *scratchSizes, uint64_t *outOff, hipStream_t s)
{
    if (nBlocks > 0)
        hipLaunchKernelGGL(k_header_sizes, dim3((unsigned)((nBlocks + 255) / 256)), dim3(256), 0, s, framed,
                           framedLen, blockOff, nBlocks, headerKind, fixedUncomp, scratchSizes);
    hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, s, scratchSizes, nBlocks, outOff);
}

// Decoded sizes without decoding (size_walk.hpp): one wavefront per block, a persistent grid.  The header is checked as
// read_block_header checks it; the header's own uncompLen (headerKind 8) is not looked at.
static_assert(SIZE_E_UNKNOWN == BLK_E_SIZE_UNKNOWN, "one code");
__global__ __launch_bounds__(LZ4_WAVE) void k_decoded_size(const uint8_t *framed, uint64_t framedLen, const uint64_t *blockOff,
                                                           int nBlocks, int headerKind, int maxUncomp, int trailer, int32_t *size)
{
    __shared__ SizeLds lds;
    const int lane = lane_id();
    if (lane < 4) ((uint32_t *)&lds.win[SW_WIN])[lane] = 0u;
    if (lane < 2) lds.nz[SW_WIN / 32 + lane] = 0u;
    wave_fence();
    for (int blk = (int)blockIdx.x; blk < nBlocks; blk += (int)gridDim.x) {
        const uint64_t off = blockOff[blk];
        int r;
        if (off + (uint64_t)headerKind > framedLen) r = BLK_E_TRUNCATED;
        else {
            const int compLen = uni(load_le32(framed + off));
            const uint64_t end = off + (uint64_t)headerKind + (uint64_t)(uint32_t)max(compLen, 0);
            if (compLen <= 0 || compLen > MAX_COMP_LEN) r = BLK_E_COMPLEN;
            else if (end > framedLen || (trailer && end + 4u > framedLen)) r = BLK_E_TRUNCATED;
            else r = decoded_size_block(framed + off + headerKind, compLen, maxUncomp, framed, framed + framedLen, lds);
        }
        if (lane == 0) size[blk] = r;
    }
}

void launch_decoded_size(const uint8_t *framed, uint64_t framedLen, const uint64_t *blockOff, int nBlocks, int headerKind,
                         int maxUncomp, int trailer, int32_t *size, uint64_t *outOff, hipStream_t s)
{
    if (nBlocks > 0) {
        static std::atomic<int> cus[64];                                    // CUs per device, asked for once
        int dev = 0;
        (void)hipGetDevice(&dev);
        int nc = cus[dev & 63].load(std::memory_order_relaxed);
        if (nc <= 0) {
            if (hipDeviceGetAttribute(&nc, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || nc <= 0) nc = 256;
            cus[dev & 63].store(nc, std::memory_order_relaxed);
        }
        const unsigned grid = (unsigned)min(nBlocks, max(nc, 1) * 32);      // 8 waves per SIMD
        hipLaunchKernelGGL(k_decoded_size, dim3(grid), dim3(LZ4_WAVE), 0, s, framed, framedLen, blockOff, nBlocks, headerKind,
                           maxUncomp, trailer, size);
    }
    if (outOff) hipLaunchKernelGGL(k_scan_u64, dim3(1), dim3(1024), 0, s, (const int32_t *)size, nBlocks, outOff);
}
