// san_stubs_checksum.cpp -- the block-checksum launchers of kernels.hip (checksum.hpp), stubbed for the CPU-only
// sanitizer build of the host library like those in san_stubs.cpp.  Never reached there.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_xxh32_ranges(const uint8_t *, const uint64_t *, const int32_t *, int, uint32_t, uint32_t *, hipStream_t) { abort(); }
void launch_xxh32_append(uint8_t *, size_t, int, int32_t *, int, hipStream_t) { abort(); }
void launch_xxh32_verify(const DecodeArgs &, int32_t *, hipStream_t) { abort(); }
