// san_stubs_hcdict.cpp -- the launchers of the high-compression dictionary batches (kernels.h; defined in kernels/encode.inc),
// stubbed like the ones in san_stubs.cpp for the CPU-only sanitizer builds of the host library (make asan / make tsan /
// make asan-dict / make asan-hcdict).  Never reached there: without a gfx950 device no call gets as far as a launch.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_hcdict_build(uint8_t *, const uint8_t *, int, hipStream_t) { abort(); }
int encode_hc_dict_grid(int) { abort(); }
void launch_encode_hc_dict(const HcDictArgs &, int, hipStream_t) { abort(); }
