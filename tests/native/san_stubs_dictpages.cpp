// san_stubs_dictpages.cpp -- the launcher of the fast fixed-size page batches against a prepared dictionary (kernels.h; defined in
// kernels/encode.inc), stubbed like the ones in san_stubs.cpp for the CPU-only sanitizer builds of the host library (make asan /
// make tsan / make asan-dict / make asan-hcdict / make asan-fastdict / make asan-pages / make asan-fastpages / make asan-dictpages).
// Never reached there: without a gfx950 device no call gets as far as a launch.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_pages_fastdict(const PagesFastDictArgs &, int, hipStream_t) { abort(); }
