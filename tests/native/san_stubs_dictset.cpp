// san_stubs_dictset.cpp -- the launchers of the dictionary-set calls (kernels.h; defined in kernels/encode.inc and
// kernels/linked_walk.inc), stubbed like the ones in san_stubs_fastdict.cpp for the CPU-only sanitizer builds of the host library
// (make asan / make tsan / make asan-dict / asan-hcdict / asan-fastdict / asan-pages / asan-fastpages / asan-dictpages /
// asan-dictset).  Never reached there: without a gfx950 device no call gets as far as a launch.
#include "../../streamly-lz4_amd/csrc/kernels.h"

#include <cstdlib>

void launch_dictset_group(const FastDictMultiArgs &, int, hipStream_t) { abort(); }
void launch_encode_fastdict_multi(const FastDictMultiArgs &, int, hipStream_t) { abort(); }
void launch_decode_dict_multi(const DictMultiArgs &, hipStream_t) { abort(); }
