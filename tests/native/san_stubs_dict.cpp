// san_stubs_dict.cpp -- the launchers of the shared-dictionary batches (kernels.h; defined in kernels/encode.inc and
// kernels/linked_walk.inc), stubbed like the ones in san_stubs.cpp for the CPU-only sanitizer builds of the host library
// (make asan / make tsan / make asan-dict).  Never reached there: without a gfx950 device no call gets as far as a launch.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_cstreams_load_dict(uint8_t *, const uint8_t *, int, hipStream_t) { abort(); }
void launch_exact_dict(const ExactDictArgs &, hipStream_t) { abort(); }
void launch_decode_dict(const DecodeArgs &, hipStream_t) { abort(); }
