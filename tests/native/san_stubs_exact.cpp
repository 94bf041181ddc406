// san_stubs_exact.cpp -- the reference-exact encoder's launchers of kernels.hip (encode_exact.hpp), stubbed for the
// CPU-only sanitizer build of the host library like those in san_stubs.cpp.  Never reached there.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_exact_chain(const ExactArgs &, int, int, int, hipStream_t) { abort(); }
void launch_exact_verify(const ExactArgs &, int, int, hipStream_t) { abort(); }
void launch_exact_finish(const ExactArgs &, hipStream_t) { abort(); }
