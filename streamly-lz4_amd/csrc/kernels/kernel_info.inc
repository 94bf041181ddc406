// kernels/kernel_info.inc -- what the HIP runtime says about the kernels that decode through decode_block_par (host code only).
// A part of kernels.hip, the one device translation unit: included there last, and not compiled on its own.
// The decoder is bound by the waves a CU holds (DESIGN.md 4), and how many it holds is decided by the LDS GRANULE of the machine,
// which no compile-time figure shows: this asks the runtime.  mi355lz4_debug_kernel_info (api.cpp).
int decode_kernel_info(int which, int *out)
{
    const void *f = nullptr;
    int threads = 64;
    switch (which) {
    case 0: f = (const void *)k_decode_par<false>; break;
    case 1: f = (const void *)k_decode_par_redo; break;
    case 2: f = (const void *)k_decode_dict; break;
    case 3: f = (const void *)k_decode_par_partial<false>; break;
    case 4: f = (const void *)k_decode_par_partial<true>; break;
    case 5: f = (const void *)k_decode_dstreams; break;
    case 6: f = (const void *)k_decode_fixup_linked; break;
    case 7: f = (const void *)k_decode_fixup_runs; break;
    case 8: f = (const void *)k_runin_decode; break;
    case 9: f = (const void *)k_runin_fix; break;
    case 10: f = (const void *)k_decode_tolerant; break;
    default: return -1;
    }
    hipFuncAttributes attr;
    hipError_t e = hipFuncGetAttributes(&attr, f);
    if (e != hipSuccess) return (int)e;
    int resident = 0;
    e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, f, threads, 0);
    if (e != hipSuccess) return (int)e;
    out[0] = resident;
    out[1] = (int)attr.sharedSizeBytes;
    out[2] = attr.numRegs;
    out[3] = (int)sizeof(ParLds);
    return 0;
}
