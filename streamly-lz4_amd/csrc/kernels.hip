// kernels.hip -- gfx950 kernels of the MI355X LZ4 block engine and their launchers: the one device translation unit.
//
// The kernels live in kernels/*.inc, one file per family, included below.  They stay ONE translation unit on purpose: the
// kernels share out-of-line callees and the inliner decides by who else is in the module, so a family compiled
// on its own is other code.  For the same reason the ORDER of the device definitions is part of the build: add a kernel at the
// end of its family's file, a family at the end of the list.  Launchers are host code and sit with their kernels.
//
//   file (kernels/)        kernels                                                          device functions
//   decode_seq.inc         k_link_stat, k_decode_seq; read_block_header for every decoder   decode_seq.hpp
//   encode.inc             k_encode<MOD, PAIR>: block encode, independent or linked          encode_wave.hpp
//                          k_encode_hc: hash chains + lazy parse                             encode_hc.hpp
//                          k_exact_chain / _verify / _finish, k_exact_streams: the reference's bytes   encode_exact.hpp
//                          k_encode_seg, k_seg_sizes, k_emit_seg: small batches, waves per block       encode_wave.hpp
//                          k_exact_pages: fixed-size output pages, LZ4_compress_destSize      encode_fill.hpp
//                          k_pages_fast: the same pages from the wave encoder with a budget   encode_wave.hpp, BUDGET
//                          k_pages_fastdict: such pages against a prepared dictionary         encode_wave.hpp, DICT + PREP + BUDGET
//                          k_dictset_zero / _hist / _scan / _scatter, k_encode_fastdict_multi<PAIR>: a dictionary per block
//                          k_fstreams_plan, k_encode_fstreams<PAIR>, k_fstreams_save: linked streams continued across calls
//                          (k_encode_hc_fstreams, those streams at a set's level 1..12, is a second caller of encode_block_hc<false>
//                          and for that reason NOT of this unit: kernels_hstreams.hip; its launcher is here)
//   compact.inc            k_scan_u64, k_copy_slots, k_interleave, k_header_sizes, k_decoded_size       size_walk.hpp
//   checksum.inc           k_xxh32_ranges / _append / _verify: four lanes per range          checksum.hpp
//   generate.inc           k_generate: synthetic inputs (bench and test support)
//   decode_par_cu.inc      k_decode_par<STATS>, k_decode_par_redo: one wave per block, 32 to a CU       decode_par.hpp
//                          k_decode_cu: one workgroup per block                              decode_cu.hpp
//                          k_decode_cu_linked, k_cu_tails, k_cu_publish: big linked blocks, guessed dictionaries
//   decode_partial.inc     k_decode_seq_partial, k_decode_par_partial<REDO>, k_decode_cu_partial: the first N bytes
//   decode_tok.inc         k_walk_tokens, k_decode_tok<STATS>: token lists (MI355LZ4_EXPERIMENTS only)   decode_par.hpp, LIST
//   linked_walk.inc        k_decode_fixup_linked: a wave per stream; k_decode_dstreams, k_dstreams_set: streams continued
//                          across calls; k_run_starts, k_decode_fixup_runs: a wave per short run        decode_par.hpp
//                          k_decode_dict, k_decode_dict_multi: independent blocks against one dictionary, or one each
//   runin.inc              k_runin_decode / _verify / _fix / _publish: long streams in pieces (RUNIN_OCC)
//   linked_tolerant.inc    k_decode_tolerant: deferred lists; k_decode_fixup_regions: their replay      linked_replay.hpp
//   linked_ptr.inc         k_ptr_expand / _jump / _fetch<CHASE> / _finish: the pointer passes           linked_ptr.hpp
//                          k_longest_stream, k_dict_share; launch_linked_resolve_a / _b / _fetch_block
//   frames.inc             k_frames_scan / _fill / _bsum / _sizes / _layout: a batch of standard LZ4 frames parsed and sized;
//                          k_frames_place / _stored / _check / _finish / _result, k_decode_frames_linked: its decode     size_walk.hpp, checksum.hpp
//                          (the write side of the frame batches, k_cframes_*, is a unit of its own: kernels_cframes.hip)
//   kernel_info.inc        (no kernel) decode_kernel_info: resident workgroups per CU and static LDS of the decode_par.hpp kernels
//
// Everything is HBM/LDS byte work; there is deliberately no MFMA anywhere.
#include "kernels.h"

#include <algorithm>
#include <atomic>

#include "decode_seq.hpp"
#include "decode_par.hpp"
#include "decode_cu.hpp"
#include "linked_replay.hpp"
#include "linked_ptr.hpp"
#include "encode_wave.hpp"
#include "encode_hc.hpp"
#include "encode_exact.hpp"
#include "checksum.hpp"
#include "size_walk.hpp"
#include "encode_fill.hpp"

using namespace lz4dev;

#include "kernels/decode_seq.inc"
#include "kernels/encode.inc"
#include "kernels/compact.inc"
#include "kernels/checksum.inc"
#include "kernels/generate.inc"
#include "kernels/decode_par_cu.inc"
#include "kernels/decode_partial.inc"
#include "kernels/decode_tok.inc"
#include "kernels/linked_walk.inc"
#include "kernels/runin.inc"
#include "kernels/linked_tolerant.inc"
#include "kernels/linked_ptr.inc"
#include "kernels/frames.inc"
#include "kernels/kernel_info.inc"
