// kernels/checksum.inc -- block checksums: xxh32 of many ranges, the compress side's trailers, the decode side's flags (checksum.hpp).
// A part of kernels.hip, the one device translation unit: included there, in this order, and not compiled on its own.
// ---------------------------------------------------------------------------
// K4: block checksums (checksum.hpp): four lanes per range, 64 ranges per 256-thread workgroup
// ---------------------------------------------------------------------------
static inline unsigned xxh_groups(int n) { return (unsigned)(((int64_t)n * 4 + 255) / 256); }

__global__ __launch_bounds__(256) void k_xxh32_ranges(const uint8_t *base, const uint64_t *off, const int32_t *len, int n,
                                                      uint32_t seed, uint32_t *out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t >> 2), q = (int)(t & 3);
    const uint8_t *p = base;
    int64_t L = -1;
    if (i < n) { p = base + off[i]; L = len[i]; }
    const uint32_t h = xxh32_group(p, L, seed, q);
    if (q == 0 && L >= 0) out[i] = h;
}
void launch_xxh32_ranges(const uint8_t *base, const uint64_t *off, const int32_t *len, int n, uint32_t seed, uint32_t *out,
                         hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(k_xxh32_ranges, dim3(xxh_groups(n)), dim3(256), 0, s, base, off, len, n, seed, out);
}

__global__ __launch_bounds__(256) void k_xxh32_append(uint8_t *slots, size_t slotStride, int headerKind, int32_t *framedLen, int n)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t >> 2), q = (int)(t & 3);
    uint8_t *p = slots;
    int64_t L = -1;
    int f = 0;
    if (i < n) {
        f = framedLen[i];
        p = slots + (size_t)i * slotStride + headerKind;
        if (f > headerKind) L = f - headerKind;                  // (0: the block failed, it gets no trailer)
    }
    const uint32_t h = xxh32_group(p, L, 0u, q);
    if (q == 0 && L >= 0) { store_le32(p + L, (int32_t)h); framedLen[i] = f + 4; }
}
void launch_xxh32_append(uint8_t *slots, size_t slotStride, int headerKind, int32_t *framedLen, int n, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(k_xxh32_append, dim3(xxh_groups(n)), dim3(256), 0, s, slots, slotStride, headerKind, framedLen, n);
}

__global__ __launch_bounds__(256) void k_xxh32_verify(DecodeArgs a, int32_t *fail)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int i = (int)(t >> 2), q = (int)(t & 3);
    const uint8_t *p = a.framed;
    int64_t L = -1;
    if (i < a.nBlocks) {
        const uint64_t off = a.blockOff[i];
        if (off + (uint64_t)a.headerKind <= a.framedLen) {
            const int compLen = load_le32(a.framed + off);
            // (what read_block_header rejects on its own is left to it: no flag)
            if (compLen > 0 && compLen <= MAX_COMP_LEN && off + (uint64_t)a.headerKind + (uint64_t)compLen + 4u <= a.framedLen) {
                p = a.framed + off + a.headerKind;
                L = compLen;
            }
        }
    }
    const uint32_t h = xxh32_group(p, L, 0u, q);
    if (q == 0 && i < a.nBlocks) fail[i] = (L >= 0 && h != (uint32_t)load_le32(p + L)) ? 1 : 0;
}
void launch_xxh32_verify(const DecodeArgs &a, int32_t *fail, hipStream_t s)
{
    if (a.nBlocks > 0) hipLaunchKernelGGL(k_xxh32_verify, dim3(xxh_groups(a.nBlocks)), dim3(256), 0, s, a, fail);
}
