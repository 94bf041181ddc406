// san_stubs_pages.cpp -- the launcher of the fixed-size page batches (kernels.h; defined in kernels/encode.inc), stubbed like the
// ones in san_stubs.cpp for the CPU-only sanitizer builds of the host library (make asan / make tsan / make asan-dict /
// make asan-hcdict / make asan-pages).  Never reached there: without a gfx950 device no call gets as far as a launch.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_exact_pages(const PagesArgs &, hipStream_t) { abort(); }
