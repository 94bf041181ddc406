// san_stubs_hc.cpp -- the high-compression encoder's launcher of kernels.hip (encode_hc.hpp), stubbed for the CPU-only
// sanitizer build of the host library like those in san_stubs.cpp.  Never reached there.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_encode_hc(const EncodeArgs &, int, hipStream_t) { abort(); }
