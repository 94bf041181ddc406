// san_stubs_hstreams.cpp -- the launcher of the fast linked streams at a set's level 1..12 and its grid (kernels.h; defined in
// kernels/encode.inc), stubbed for the CPU-only sanitizer builds of the host library (make asan / make tsan and every
// make asan-*).  Unlike the other stubs these two count instead of aborting: tests/native/hstreams_args_main.cpp drives calls at
// set level 9 past every argument check and reads san_hstreams_launches to say how far they came.  Nothing is launched.
#include "../../streamly-lz4_amd/csrc/kernels.h"

int san_hstreams_launches = 0;          // launch_fstreams_hc calls so far
int san_hstreams_last_level = -1;       // the level of the last one

int encode_hc_fstreams_grid(int nBlocks, int knob, size_t) { return nBlocks < 1 ? 1 : (knob > 0 && knob < nBlocks ? knob : nBlocks); }
void launch_fstreams_hc(const FStreamsArgs &, int, int level, hipStream_t)
{
    san_hstreams_launches++;
    san_hstreams_last_level = level;
}
