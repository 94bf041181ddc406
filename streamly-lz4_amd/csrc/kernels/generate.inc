// kernels/generate.inc -- synthetic inputs (bench and test support).
// A part of kernels.hip, the one device translation unit: included there, in this order, and not compiled on its own.
// ---------------------------------------------------------------------------
// Synthetic inputs (SURVEY.md 8d): xorshift64* seeded per block by splitmix64.
// One thread per block; setup only, never timed.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t xs64(uint64_t &st)
{
    uint64_t x = st;
    x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
    st = x;
    return x * 0x2545F4914F6CDD1DULL;
}

__global__ __launch_bounds__(64) void k_generate(int kind, uint8_t *dst, int blockLen, int nBlocks,
                                                 uint64_t firstBlock, uint64_t blockStep, uint32_t litMax,
                                                 uint32_t offMax)
{
    const int b = (int)(blockIdx.x * 64u + threadIdx.x);
    if (b >= nBlocks) return;
    uint8_t *out = dst + (size_t)b * (size_t)blockLen;
    const uint64_t index = firstBlock + (uint64_t)b * blockStep;
    const uint32_t n = (uint32_t)blockLen;
    if (kind == 0) {
        uint64_t st = splitmix64(0x9E3779B97F4A7C15ULL ^ index);
        if (!st) st = 1;
        for (uint32_t i = 0; i < n;) {
            uint64_t r = xs64(st);
            for (int k = 0; k < 8 && i < n; k++, i++) out[i] = (uint8_t)(r >> (8 * k));
        }
    } else if (kind == 1) {
        uint64_t st = splitmix64(0x9E3779B97F4A7C15ULL ^ index);
        if (!st) st = 1;
        uint32_t pos = 0;
        while (pos < n) {
            uint32_t L = 1 + (uint32_t)(xs64(st) % litMax);
            for (uint32_t i = 0; i < L && pos < n; i++) out[pos++] = (uint8_t)(32 + xs64(st) % 64);
            if (pos >= n) break;
            uint32_t M = 4 + (uint32_t)(xs64(st) % 61);
            uint32_t lim = (pos < offMax) ? pos : offMax;
            uint32_t o = 1 + (uint32_t)(xs64(st) % lim);
            for (uint32_t i = 0; i < M && pos < n; i++, pos++) out[pos] = out[pos - o];
        }
    } else {
        uint64_t st = splitmix64(0x9E3779B97F4A7C15ULL ^ (index ^ 0x7465787400000000ULL));
        if (!st) st = 1;
        uint32_t pos = 0;
        while (pos < n) {
            uint64_t r = xs64(st);
            uint32_t a = (uint32_t)(r & 4095), bq = (uint32_t)((r >> 12) & 4095);
            uint32_t c = (uint32_t)((r >> 29) & 4095), d = (uint32_t)((r >> 41) & 4095);
            uint32_t w = (((a * bq) >> 12) * ((c * d) >> 12)) >> 12;
            uint64_t h = splitmix64(0x776F7264ULL + w);
            uint32_t len = 2 + (uint32_t)(h & 7);
            uint32_t sep = (uint32_t)((r >> 24) & 31);
            for (uint32_t j = 0; j < len && pos < n; j++)
                out[pos++] = (uint8_t)('a' + ((h >> (3 + 5 * j)) & 31) % 26);
            if (pos < n) out[pos++] = (sep == 0) ? '\n' : (sep == 1) ? ',' : ' ';
            if (sep == 1 && pos < n) out[pos++] = ' ';
        }
    }
}

void launch_generate(int kind, uint8_t *dst, int blockLen, int nBlocks, uint64_t firstBlock,
                     uint64_t blockStep, uint32_t litMax, uint32_t offMax, hipStream_t s)
{
    if (nBlocks > 0)
        hipLaunchKernelGGL(k_generate, dim3((unsigned)((nBlocks + 63) / 64)), dim3(64), 0, s, kind, dst,
                           blockLen, nBlocks, firstBlock, blockStep, litMax, offMax);
}
