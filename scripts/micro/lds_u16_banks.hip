// Microbenchmark (development aid): is ds_read_u16 banked like ds_read_b32?  Both widths are timed on address patterns with a known
// number of distinct dwords per bank among 32 lanes: lanes 2 BYTES apart (two lanes to a dword, what the successor table's gathers
// look like at best), 4 bytes apart (a dword each, none share a bank), 8, 16 and 32 bytes apart (2-, 4- and 8-way conflicts).
// 16 waves per CU, as lds_unaligned.hip; the figure is LDS cycles per wave-instruction per CU.  The loop's own instructions set a
// floor of about 4.8 cycles, so the first three patterns (2 and 4 LDS cycles) are not told apart: what it shows is that both
// widths pay the same for the 4-way and the 8-way pattern (8.3 and 16.2: two groups of 32 lanes times the ways).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
template <int W16>
__global__ __launch_bounds__(64) void k(uint64_t *out, int iters, int strideBytes)
{
    __shared__ __attribute__((aligned(16))) uint8_t buf[4096 + 16];
    const int lane = threadIdx.x;
    for (int i = lane; i < 1028; i += 64) ((uint32_t *)buf)[i] = i * 2654435761u;
    __syncthreads();
    uint64_t acc = 0;
    uint32_t base = 0;
    for (int i = 0; i < iters; i++) {
        const uint32_t a = (base + (uint32_t)(lane * strideBytes)) & 4095u;     // (4096 is a multiple of the 128 bytes of a bank row)
        if (W16) acc += *(const uint16_t *)&buf[a];
        else acc += *(const uint32_t *)&buf[a & ~3u];
        base += 68;
    }
    out[blockIdx.x * 64 + lane] = acc;
}
template <int W16>
static void run(const char *name, int strideBytes)
{
    const int NB = 256 * 16, iters = 20000;
    static uint64_t *out = nullptr;
    if (!out && hipMalloc(&out, (size_t)NB * 64 * 8) != hipSuccess) { printf("hipMalloc failed\n"); exit(1); }
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipLaunchKernelGGL(k<W16>, dim3(NB), dim3(64), 0, 0, out, iters, strideBytes);
    hipEventRecord(e0); hipLaunchKernelGGL(k<W16>, dim3(NB), dim3(64), 0, 0, out, iters, strideBytes); hipEventRecord(e1);
    if (hipEventSynchronize(e1) != hipSuccess) { printf("launch failed\n"); exit(1); }
    float ms; hipEventElapsedTime(&ms, e0, e1);
    printf("%-12s lanes %2d bytes apart : %.2f LDS cycles per wave-instruction per CU (2.4 GHz)\n", name, strideBytes, ms * 1e-3 * 2.4e9 / ((double)iters * 16));
}
int main()
{
    for (int s : {2, 4, 8, 16, 32}) { run<1>("ds_read_u16", s); run<0>("ds_read_b32", s); }
    return 0;
}
