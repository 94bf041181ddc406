// san_stubs_info.cpp -- the kernel query of kernels.h (defined in kernels/kernel_info.inc), stubbed like the launchers in
// san_stubs.cpp for the CPU-only sanitizer builds of the host library: without device code there is no kernel to ask about.
#include "../../streamly-lz4_amd/csrc/kernels.h"

int decode_kernel_info(int, int *) { return -1; }
