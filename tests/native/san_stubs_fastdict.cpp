// san_stubs_fastdict.cpp -- the launchers of the level-0 batches against a prepared dictionary (kernels.h; defined in
// kernels/encode.inc), stubbed like the ones in san_stubs_hcdict.cpp for the CPU-only sanitizer builds of the host library (make
// asan / make tsan / make asan-dict / asan-hcdict / asan-fastdict / asan-pages).  Never reached there: without a gfx950 device no
// call gets as far as a launch.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_hcdict_build_fast(uint8_t *, const uint8_t *, int, hipStream_t) { abort(); }
int encode_fastdict_grid(int, int, size_t) { abort(); }
void launch_encode_fastdict(const FastDictArgs &, int, hipStream_t) { abort(); }
