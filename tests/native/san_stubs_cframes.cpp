// san_stubs_cframes.cpp -- the launchers of the frame writer (kernels.h; defined in kernels_cframes.hip), stubbed like the ones in
// san_stubs_frames.cpp for the CPU-only sanitizer builds of the host library (make asan / make tsan / make asan-cframes).  Never
// reached there: without a gfx950 device no call gets as far as a launch.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_cframes_plan(const CFramesArgs &, hipStream_t) { abort(); }
void launch_cframes_finish(const CFramesArgs &, hipStream_t) { abort(); }
void launch_cframes_gather(const uint8_t *, const uint64_t *, const int64_t *, int, uint64_t *, uint8_t *, uint64_t, hipStream_t) { abort(); }
