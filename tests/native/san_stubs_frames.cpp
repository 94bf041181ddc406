// san_stubs_frames.cpp -- the launchers of the frame batches (kernels.h; defined in kernels/frames.inc), stubbed like the ones in
// san_stubs_dictset.cpp for the CPU-only sanitizer builds of the host library (make asan / make tsan / make asan-frames).  Never
// reached there: without a gfx950 device no call gets as far as a launch.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_frames_scan(const FramesArgs &, hipStream_t) { abort(); }
void launch_frames_load(const FramesArgs &, hipStream_t) { abort(); }
void launch_frames_place(const FramesArgs &, hipStream_t) { abort(); }
void launch_frames_decode(const FramesArgs &, hipStream_t) { abort(); }
