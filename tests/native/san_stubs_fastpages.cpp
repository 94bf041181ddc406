// san_stubs_fastpages.cpp -- the launcher of the fast fixed-size page batches (kernels.h; defined in kernels/encode.inc), stubbed like
// the ones in san_stubs.cpp for the CPU-only sanitizer builds of the host library (make asan / make tsan / make asan-dict /
// make asan-hcdict / make asan-fastdict / make asan-pages / make asan-fastpages).  Never reached there: without a gfx950 device no
// call gets as far as a launch.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_pages_fast(const PagesFastArgs &, hipStream_t) { abort(); }
