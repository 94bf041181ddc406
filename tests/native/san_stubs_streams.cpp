// san_stubs_streams.cpp -- the many-streams exact encoder's launcher of kernels.hip (k_exact_streams), stubbed for the
// CPU-only sanitizer build of the host library like those in san_stubs.cpp.  Never reached there.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_exact_streams(const ExactStreamsArgs &, int, hipStream_t) { abort(); }
