# Top-level build: the product library (HIP, gfx950 only) and the CPU checker.
#
#   make            -> streamly-lz4_amd/lib/libmi355lz4.so  + oracle/
#   make lib        -> product library only
#   make lib-exp    -> the same with the shelved experiments compiled in (tests only)
#   make oracle     -> oracle/liboracle.so (+ oracle/_ref when /root/reference exists)
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
PKG   := streamly-lz4_amd
CSRC  := $(PKG)/csrc
LIB   := $(PKG)/lib/libmi355lz4.so
HIPFLAGS ?= -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Wall -Wno-unused-function -Wno-unused-value -Wno-unused-result

SRCS := $(CSRC)/kernels.hip $(CSRC)/kernels_hstreams.hip $(CSRC)/kernels_cframes.hip $(CSRC)/api.cpp $(CSRC)/host_batch.cpp $(CSRC)/legacy.cpp $(CSRC)/host_stream.cpp $(CSRC)/lz4_frame.cpp $(CSRC)/multi_device.cpp $(CSRC)/frames.cpp $(CSRC)/cframes.cpp
# kernels/*.inc are the parts of kernels.hip (its one translation unit), not sources of their own; kernels_hstreams.hip is the one
# encoder kernel compiled apart from it and kernels_cframes.hip the frame writer's kernels (the files say why)
HDRS := $(wildcard $(CSRC)/*.hpp $(CSRC)/*.h $(CSRC)/kernels/*.inc include/*.h)
OBJS    := $(patsubst $(CSRC)/%,build/obj/%.o,$(SRCS))
OBJSEXP := $(patsubst $(CSRC)/%,build/obj-exp/%.o,$(SRCS))

all: lib oracle

# One object per source, then the link: `make -j8 lib lib-exp` compiles them side by side (a fixed count: the sources are eleven,
# and a count taken from the machine oversubscribes a shared one).
lib: $(LIB)

build/obj/%.o: $(CSRC)/% $(HDRS)
	@mkdir -p build/obj
	$(HIPCC) $(HIPFLAGS) -c -o $@ -x hip $<

$(LIB): $(OBJS)
	@mkdir -p $(PKG)/lib
	$(HIPCC) $(HIPFLAGS) -shared -Wl,-Bsymbolic -o $@ $(OBJS)

# The library with the measured-and-shelved experiments compiled in (decoder variant 3: the token-list parse of round 4).
# Not what ships: `make lib` leaves them out.  tests/test_experiment_build_gpu.py runs the decoder parity tests on it.
LIBEXP := $(PKG)/lib/libmi355lz4_exp.so
lib-exp: $(LIBEXP)

build/obj-exp/%.o: $(CSRC)/% $(HDRS)
	@mkdir -p build/obj-exp
	$(HIPCC) $(HIPFLAGS) -DMI355LZ4_EXPERIMENTS -c -o $@ -x hip $<

$(LIBEXP): $(OBJSEXP)
	@mkdir -p $(PKG)/lib
	$(HIPCC) $(HIPFLAGS) -DMI355LZ4_EXPERIMENTS -shared -Wl,-Bsymbolic -o $@ $(OBJSEXP)

oracle:
	$(MAKE) -C oracle

# Host-side sanitizer builds (CPU only; GPU ASan is not available on this pool): the host sources (api.cpp, host_batch.cpp,
# legacy.cpp, host_stream.cpp, lz4_frame.cpp, multi_device.cpp, frames.cpp, cframes.cpp) compiled by g++ against the HIP host API, kernel launchers stubbed, driven by tests/native/host_san_test.cpp.
SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp $(CSRC)/legacy.cpp $(CSRC)/host_stream.cpp $(CSRC)/lz4_frame.cpp $(CSRC)/multi_device.cpp $(CSRC)/frames.cpp $(CSRC)/cframes.cpp tests/native/san_stubs_frames.cpp tests/native/san_stubs_cframes.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/host_san_test.cpp
SAN_FLAGS := -std=c++17 -O1 -g -fno-omit-frame-pointer -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Wall -Wno-unused-function -Wno-unused-result
SAN_LIBS := -L/opt/rocm/lib -Wl,-rpath,/opt/rocm/lib -lamdhip64 -lpthread

build/san/host_asan: $(SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(SAN_SRCS) $(SAN_LIBS)

build/san/host_tsan: $(SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=thread -o $@ $(SAN_SRCS) $(SAN_LIBS)

# The shared-dictionary calls' argument checks under ASan+UBSan, a program of its own (tests/native/dict_args_main.cpp): the C ABI's
# two layers and the stubbed launchers are all it needs.
DICT_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/dict_args_main.cpp
build/san/dict_args_asan: $(DICT_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(DICT_SAN_SRCS) $(SAN_LIBS)

asan-dict: build/san/dict_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/dict_args_asan

# The high-compression dictionary calls' argument checks, the same way (tests/native/hcdict_args_main.cpp).
HCDICT_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/hcdict_args_main.cpp
build/san/hcdict_args_asan: $(HCDICT_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(HCDICT_SAN_SRCS) $(SAN_LIBS)

asan-hcdict: build/san/hcdict_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/hcdict_args_asan

# The level-0 calls against a prepared dictionary, the same way (tests/native/fastdict_args_main.cpp).
FASTDICT_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/fastdict_args_main.cpp
build/san/fastdict_args_asan: $(FASTDICT_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(FASTDICT_SAN_SRCS) $(SAN_LIBS)

asan-fastdict: build/san/fastdict_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/fastdict_args_asan

# The fixed-size page calls' argument checks, the same way (tests/native/pages_args_main.cpp).
PAGES_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/pages_args_main.cpp
build/san/pages_args_asan: $(PAGES_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(PAGES_SAN_SRCS) $(SAN_LIBS)

asan-pages: build/san/pages_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/pages_args_asan

# The fast page calls' argument checks, the same way (tests/native/fastpages_args_main.cpp).
FASTPAGES_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/fastpages_args_main.cpp
build/san/fastpages_args_asan: $(FASTPAGES_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(FASTPAGES_SAN_SRCS) $(SAN_LIBS)

asan-fastpages: build/san/fastpages_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/fastpages_args_asan

# The dictionary page calls' argument checks, the same way (tests/native/dictpages_args_main.cpp).
DICTPAGES_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/dictpages_args_main.cpp
build/san/dictpages_args_asan: $(DICTPAGES_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(DICTPAGES_SAN_SRCS) $(SAN_LIBS)

asan-dictpages: build/san/dictpages_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/dictpages_args_asan

# The dictionary-set calls' argument checks, the same way (tests/native/dictset_args_main.cpp).
DICTSET_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/dictset_args_main.cpp
build/san/dictset_args_asan: $(DICTSET_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(DICTSET_SAN_SRCS) $(SAN_LIBS)

asan-dictset: build/san/dictset_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/dictset_args_asan

# The fast linked streams' argument checks, the same way (tests/native/fstreams_args_main.cpp).
FSTREAMS_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/fstreams_args_main.cpp
build/san/fstreams_args_asan: $(FSTREAMS_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(FSTREAMS_SAN_SRCS) $(SAN_LIBS)

asan-fstreams: build/san/fstreams_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/fstreams_args_asan

# The set's level of the fast linked streams, the same way (tests/native/hstreams_args_main.cpp).
HSTREAMS_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/hstreams_args_main.cpp
build/san/hstreams_args_asan: $(HSTREAMS_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(HSTREAMS_SAN_SRCS) $(SAN_LIBS)

asan-hstreams: build/san/hstreams_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/hstreams_args_asan

# The frame batches' argument checks, the same way (tests/native/frames_args_main.cpp; frames.cpp is the layer under test).
FRAMES_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp $(CSRC)/frames.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/san_stubs_frames.cpp tests/native/frames_args_main.cpp
build/san/frames_args_asan: $(FRAMES_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(FRAMES_SAN_SRCS) $(SAN_LIBS)

asan-frames: build/san/frames_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/frames_args_asan

# The frame writer's argument checks, the same way (tests/native/cframes_args_main.cpp; cframes.cpp is the layer under test).
CFRAMES_SAN_SRCS := $(CSRC)/api.cpp $(CSRC)/host_batch.cpp $(CSRC)/cframes.cpp tests/native/san_stubs.cpp tests/native/san_stubs_dict.cpp tests/native/san_stubs_hcdict.cpp tests/native/san_stubs_fastdict.cpp tests/native/san_stubs_dictset.cpp tests/native/san_stubs_fstreams.cpp tests/native/san_stubs_hstreams.cpp tests/native/san_stubs_pages.cpp tests/native/san_stubs_fastpages.cpp tests/native/san_stubs_dictpages.cpp tests/native/san_stubs_info.cpp tests/native/san_stubs_cframes.cpp tests/native/cframes_args_main.cpp
build/san/cframes_args_asan: $(CFRAMES_SAN_SRCS) $(HDRS)
	@mkdir -p build/san
	g++ $(SAN_FLAGS) -fsanitize=address,undefined -fno-sanitize-recover=undefined -o $@ $(CFRAMES_SAN_SRCS) $(SAN_LIBS)

asan-cframes: build/san/cframes_args_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/cframes_args_asan

asan: build/san/host_asan asan-fstreams asan-hstreams asan-cframes
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=0 LSAN_OPTIONS=suppressions=tests/native/lsan.supp ./build/san/host_asan

tsan: build/san/host_tsan
	TSAN_OPTIONS=halt_on_error=1 ./build/san/host_tsan

clean:
	rm -rf build/san build/obj build/obj-exp
	rm -f $(LIB) $(LIBEXP)
	$(MAKE) -C oracle clean

.PHONY: all lib lib-exp oracle clean asan asan-frames asan-cframes asan-dict asan-hcdict asan-fastdict asan-pages asan-fastpages asan-dictpages asan-dictset asan-fstreams asan-hstreams tsan
