// san_stubs_fstreams.cpp -- the launcher of the fast linked streams (kernels.h; defined in kernels/encode.inc), stubbed like the
// ones in san_stubs_dictset.cpp for the CPU-only sanitizer builds of the host library (make asan / make tsan and every
// make asan-*).  Never reached there: without a gfx950 device no call gets as far as a launch.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_fstreams(const FStreamsArgs &, int, hipStream_t) { abort(); }
