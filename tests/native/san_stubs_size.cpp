// san_stubs_size.cpp -- the decoded-size pass's launcher of kernels.hip (k_decoded_size), stubbed for the CPU-only sanitizer
// build of the host library like those in san_stubs.cpp.  Never reached there.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_decoded_size(const uint8_t *, uint64_t, const uint64_t *, int, int, int, int, int32_t *, uint64_t *, hipStream_t) { abort(); }
