// san_stubs_dstreams.cpp -- the decode streams' launchers of kernels.hip (k_decode_dstreams, k_dstreams_set), stubbed for the
// CPU-only sanitizer build of the host library like those in san_stubs.cpp.  Never reached there.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_decode_dstreams(const DStreamsArgs &, int, hipStream_t) { abort(); }
void launch_dstreams_set(uint8_t *, int, int, const uint8_t *, uint32_t, hipStream_t) { abort(); }
