// san_stubs_partial.cpp -- the partial decode's launcher of kernels.hip (k_decode_*_partial), stubbed for the CPU-only sanitizer
// build of the host library like those in san_stubs.cpp.  Never reached there.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_decode_partial(const DecodeArgs &, int, hipStream_t) { abort(); }
