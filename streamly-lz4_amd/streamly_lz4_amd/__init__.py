"""streamly_lz4_amd -- Python binding of the MI355X LZ4 block engine.

Thin ctypes layer over the C ABI in ``include/mi355lz4.h`` (device-resident and
host-buffer batched calls) and over the C++ mirror of the reference's stream
combinators (``include/streamly_lz4.hpp``: compressChunks / decompressChunks /
resizeChunks / decompressChunksWith; reference src/Streamly/LZ4.hs:94-122,
src/Streamly/Internal/LZ4.hs:338-651).

There is no CPU codec in this package: if ``libmi355lz4.so`` is missing, or no
gfx950 device is visible, every codec call raises.  PyTorch is used only by
callers that want device memory / streams / torch.distributed; this module
itself needs only ctypes and numpy.
"""
import ctypes as C
import sys
import os

import numpy as np

__all__ = [
    "lib", "lib_path", "Engine", "CompressStreams", "FastCompressStreams", "DecompressStreams", "LZ4Error", "BlockSize", "BlockConfig", "FrameConfig",
    "defaultBlockConfig", "defaultFrameConfig", "setBlockMaxSize", "setFrameEndMark", "setBlockChecksum",
    "compressChunks", "decompressChunks", "decompressChunksRaw", "resizeChunks",
    "decompressChunksWith", "decompressChunksStream", "simpleFrameParser", "compress_bound", "slot_stride", "slot_stride_ex", "device_count",
    "xxh32", "lz4FrameCompress", "lz4FrameDecompress",
]

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# MI355LZ4_LIB lets a developer A/B another build of the same library (scripts/ab_variants.sh)
lib_path = os.environ.get("MI355LZ4_LIB") or os.path.join(os.path.dirname(_PKG_DIR), "lib", "libmi355lz4.so")

_u8p = C.POINTER(C.c_uint8)
_u64p = C.POINTER(C.c_uint64)
_i32p = C.POINTER(C.c_int32)


class LZ4Error(RuntimeError):
    """Raised where the reference calls `error` / `Parser.die`, with the same message."""


def _preload_torch_hip():
    """PyTorch wheels bundle their own HIP/HSA runtime (same SONAME as /opt/rocm's).  Two HSA
    runtimes in one process do not coexist, so when torch is installed make its copy the one that
    is loaded, whichever of torch / this package is imported first."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=os.RTLD_GLOBAL)
    except Exception:
        pass


def _load():
    _preload_torch_hip()
    if not os.path.exists(lib_path):
        raise ImportError(
            "streamly_lz4_amd: %s is missing -- build it with `make lib` (hipcc, gfx950). "
            "There is no CPU fallback." % lib_path
        )
    L = C.CDLL(lib_path, mode=os.RTLD_LOCAL)

    def sig(name, res, *args):
        f = getattr(L, name)
        f.restype = res
        f.argtypes = list(args)

    vp = C.c_void_p
    sig("mi355lz4_version", C.c_int)
    sig("mi355lz4_last_error", C.c_char_p)
    sig("mi355lz4_device_count", C.c_int)
    sig("mi355lz4_create", C.c_int, C.POINTER(vp), C.c_int)
    sig("mi355lz4_destroy", None, vp)
    sig("mi355lz4_set_stream", C.c_int, vp, vp)
    sig("mi355lz4_get_stream", vp, vp)
    sig("mi355lz4_synchronize", C.c_int, vp)
    sig("mi355lz4_set_decoder", C.c_int, vp, C.c_int)
    sig("mi355lz4_set_segments", C.c_int, vp, C.c_int)
    sig("mi355lz4_set_linked_async", C.c_int, vp, C.c_int)
    sig("mi355lz4_set_linked_compress", C.c_int, vp, C.c_int)
    sig("mi355lz4_compress_bound", C.c_int, C.c_int)
    sig("mi355lz4_slot_stride", C.c_size_t, C.c_int, C.c_int)
    sig("mi355lz4_compress_batch_device", C.c_int, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
        vp, C.c_size_t, vp)
    sig("mi355lz4_compact_device", C.c_int, vp, vp, C.c_size_t, vp, C.c_int, vp, C.c_size_t, vp)
    sig("mi355lz4_decompress_batch_device", C.c_int, vp, vp, C.c_uint64, vp, C.c_int, C.c_int, C.c_int, C.c_int,
        vp, vp, vp, vp)
    sig("mi355lz4_decompress_streams_device", C.c_int, vp, vp, C.c_uint64, vp, C.c_int, C.c_int, C.c_int, vp,
        C.c_int, vp, vp, vp, vp)
    sig("mi355lz4_decompress_linked_begin", C.c_int, vp, vp, C.c_uint64, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp,
        C.c_int)
    sig("mi355lz4_decompress_linked_end", C.c_int, vp)
    sig("mi355lz4_decompress_linked_end_last", C.c_int, vp)
    sig("mi355lz4_index_device", C.c_int, vp, vp, C.c_uint64, vp, C.c_int, C.c_int, C.c_int, vp)
    sig("mi355lz4_decoded_size_device", C.c_int, vp, vp, C.c_uint64, vp, C.c_int, C.c_int, C.c_int, vp, vp)
    sig("mi355lz4_decoded_sizes_host", C.c_int, vp, _u8p, C.c_size_t, _u64p, C.c_int, C.c_int, C.c_int, _i32p)
    # partial decode
    sig("mi355lz4_decompress_partial_device", C.c_int, vp, vp, C.c_uint64, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp)
    sig("mi355lz4_decompress_partial", C.c_int, vp, _u8p, C.c_size_t, C.c_int, C.c_int, _i32p, C.c_int, _u8p, C.c_size_t,
        C.POINTER(C.c_size_t), _i32p, C.c_int, C.POINTER(C.c_int))
    sig("mi355lz4_compress_batch", C.c_int, vp, C.POINTER(_u8p), _i32p, C.c_int, C.c_int, C.c_int, _u8p,
        C.c_size_t, C.POINTER(C.c_size_t), _i32p, _i32p)
    sig("mi355lz4_index_host", C.c_int, _u8p, C.c_size_t, C.c_int, C.c_int, _u64p, _i32p, C.c_int,
        C.POINTER(C.c_int))
    sig("mi355lz4_decompress_batch", C.c_int, vp, _u8p, C.c_size_t, C.c_int, C.c_int, C.c_int, _u8p, C.c_int,
        _u8p, C.c_size_t, C.POINTER(C.c_size_t), _i32p, C.c_int, C.POINTER(C.c_int))
    sig("mi355lz4_decompress_streams", C.c_int, vp, _u8p, C.c_size_t, C.c_int, C.c_int, _i32p, C.c_int,
        _u8p, C.c_size_t, C.POINTER(C.c_size_t), _i32p, C.c_int, C.POINTER(C.c_int))
    sig("mi355lz4_generate_device", C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
        C.c_uint32, C.c_uint32)
    sig("mi355lz4_interleave_device", C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp)
    sig("mi355lz4_event_create", C.c_int, C.POINTER(vp))
    sig("mi355lz4_event_destroy", C.c_int, vp)
    sig("mi355lz4_event_record", C.c_int, vp, vp)
    sig("mi355lz4_event_elapsed_ms", C.c_int, vp, vp, C.POINTER(C.c_float))
    # block checksums
    sig("mi355lz4_set_block_checksum", C.c_int, vp, C.c_int)
    sig("mi355lz4_slot_stride_ex", C.c_size_t, C.c_int, C.c_int, C.c_int)
    sig("mi355lz4_index_host_ex", C.c_int, _u8p, C.c_size_t, C.c_int, C.c_int, C.c_int, _u64p, _i32p, C.c_int,
        C.POINTER(C.c_int))
    sig("mi355lz4_xxh32_device", C.c_int, vp, vp, vp, vp, C.c_int, C.c_uint32, vp)
    # compression levels
    sig("mi355lz4_set_compression_level", C.c_int, vp, C.c_int)
    sig("mi355lz4_get_compression_level", C.c_int, vp)
    sig("mi355lz4_set_compress_exact", C.c_int, vp, C.c_int)
    sig("mi355lz4_get_compress_exact", C.c_int, vp)
    sig("mi355lz4_compress_exact_reset", C.c_int, vp)
    sig("mi355lz4_debug_exact_state", C.c_int, vp, C.POINTER(C.c_int))
    sig("mi355lz4_debug_kernel_info", C.c_int, vp, C.c_int, C.POINTER(C.c_int))
    # many exact streams in one call
    sig("mi355lz4_cstreams_create", C.c_int, vp, C.c_int, C.POINTER(vp))
    sig("mi355lz4_cstreams_destroy", None, vp)
    sig("mi355lz4_cstreams_count", C.c_int, vp)
    sig("mi355lz4_cstreams_reset", C.c_int, vp, vp, _i32p, C.c_int)
    sig("mi355lz4_debug_cstream_state", C.c_int, vp, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))
    sig("mi355lz4_debug_cstream_slot", C.c_int, vp, C.c_int, _u8p)
    sig("mi355lz4_compress_streams_device", C.c_int, vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, _i32p, _i32p,
        C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp)
    sig("mi355lz4_compress_streams", C.c_int, vp, vp, C.POINTER(_u8p), _i32p, C.c_int, _i32p, _i32p, C.c_int, C.c_int,
        C.c_int, _u8p, C.c_size_t, C.POINTER(C.c_size_t), _i32p, _i32p)
    # many fast linked compress streams, continued across calls
    sig("mi355lz4_fstreams_create", C.c_int, vp, C.c_int, C.POINTER(vp))
    sig("mi355lz4_fstreams_destroy", None, vp)
    sig("mi355lz4_fstreams_count", C.c_int, vp)
    sig("mi355lz4_fstreams_reset", C.c_int, vp, vp, _i32p, C.c_int)
    sig("mi355lz4_fstreams_set_dict", C.c_int, vp, vp, C.c_int, vp, C.c_int)
    sig("mi355lz4_fstreams_set_level", C.c_int, vp, C.c_int)
    sig("mi355lz4_fstreams_get_level", C.c_int, vp)
    sig("mi355lz4_debug_fstreams_peek", C.c_int, vp, C.c_int, _u8p, C.POINTER(C.c_int))
    sig("mi355lz4_compress_streams_fast_device", C.c_int, vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, _i32p, _i32p,
        C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp)
    sig("mi355lz4_compress_streams_fast", C.c_int, vp, vp, C.POINTER(_u8p), _i32p, C.c_int, _i32p, _i32p, C.c_int, C.c_int,
        C.c_int, _u8p, C.c_size_t, C.POINTER(C.c_size_t), _i32p, _i32p)
    # many linked decode streams, continued across calls
    sig("mi355lz4_dstreams_create", C.c_int, vp, C.c_int, C.POINTER(vp))
    sig("mi355lz4_dstreams_destroy", None, vp)
    sig("mi355lz4_dstreams_count", C.c_int, vp)
    sig("mi355lz4_dstreams_reset", C.c_int, vp, vp, _i32p, C.c_int)
    sig("mi355lz4_dstreams_set_dict", C.c_int, vp, vp, C.c_int, vp, C.c_int)
    sig("mi355lz4_debug_dstream_state", C.c_int, vp, C.c_int, C.POINTER(C.c_uint32), _u8p, _u8p)
    sig("mi355lz4_decompress_dstreams_device", C.c_int, vp, vp, vp, C.c_uint64, vp, C.c_int, C.c_int, C.c_int, _i32p, _i32p,
        C.c_int, vp, vp, vp, vp)
    sig("mi355lz4_decompress_dstreams", C.c_int, vp, vp, _u8p, C.c_size_t, C.c_int, C.c_int, _i32p, _i32p, C.c_int,
        _u8p, C.c_size_t, C.POINTER(C.c_size_t), _i32p, C.c_int, C.POINTER(C.c_int))
    # shared-dictionary batches
    sig("mi355lz4_cstreams_load_dict", C.c_int, vp, vp, C.c_int, vp, C.c_int)
    sig("mi355lz4_compress_dict_device", C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
        vp, C.c_size_t, vp)
    sig("mi355lz4_decompress_dict_device", C.c_int, vp, vp, C.c_uint64, vp, C.c_int, C.c_int, C.c_int, vp, C.c_int,
        vp, vp, vp, vp)
    sig("mi355lz4_compress_dict", C.c_int, vp, vp, C.c_int, C.POINTER(_u8p), _i32p, C.c_int, C.c_int, C.c_int, _u8p,
        C.c_size_t, C.POINTER(C.c_size_t), _i32p, _i32p)
    sig("mi355lz4_decompress_dict", C.c_int, vp, _u8p, C.c_size_t, C.c_int, C.c_int, _u8p, C.c_int, _u8p, C.c_size_t,
        C.POINTER(C.c_size_t), _i32p, C.c_int, C.POINTER(C.c_int))
    # high-compression levels against a shared dictionary
    sig("mi355lz4_hcdict_create", C.c_int, vp, C.POINTER(vp))
    sig("mi355lz4_hcdict_destroy", None, vp)
    sig("mi355lz4_hcdict_load", C.c_int, vp, vp, vp, C.c_int)
    sig("mi355lz4_hcdict_size", C.c_int, vp)
    sig("mi355lz4_debug_hcdict_image", C.c_int, vp, _u8p)
    sig("mi355lz4_compress_hcdict_device", C.c_int, vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, vp, C.c_size_t,
        vp)
    sig("mi355lz4_compress_hcdict", C.c_int, vp, vp, C.POINTER(_u8p), _i32p, C.c_int, C.c_int, _u8p, C.c_size_t,
        C.POINTER(C.c_size_t), _i32p, _i32p)
    # level 0 against the same prepared dictionary: the wave encoder
    sig("mi355lz4_debug_hcdict_fast_image", C.c_int, vp, _u8p)
    sig("mi355lz4_compress_fastdict_device", C.c_int, vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, vp,
        C.c_size_t, vp)
    sig("mi355lz4_compress_fastdict", C.c_int, vp, vp, C.POINTER(_u8p), _i32p, C.c_int, C.c_int, C.c_int, _u8p, C.c_size_t,
        C.POINTER(C.c_size_t), _i32p, _i32p)
    # dictionary sets: a batch in which every block names its dictionary
    sig("mi355lz4_dictset_create", C.c_int, vp, C.POINTER(vp), C.c_int, C.POINTER(vp))
    sig("mi355lz4_dictset_destroy", None, vp)
    sig("mi355lz4_dictset_count", C.c_int, vp)
    sig("mi355lz4_debug_dictset_last", C.c_int, vp, C.POINTER(C.c_int))
    sig("mi355lz4_compress_fastdict_multi_device", C.c_int, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
        vp, C.c_size_t, vp)
    sig("mi355lz4_compress_fastdict_multi", C.c_int, vp, vp, _i32p, C.POINTER(_u8p), _i32p, C.c_int, C.c_int, C.c_int, _u8p,
        C.c_size_t, C.POINTER(C.c_size_t), _i32p, _i32p)
    sig("mi355lz4_decompress_dict_multi_device", C.c_int, vp, vp, C.c_uint64, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp)
    sig("mi355lz4_decompress_dict_multi", C.c_int, vp, _u8p, C.c_size_t, C.c_int, C.c_int, vp, _i32p, _u8p, C.c_size_t,
        C.POINTER(C.c_size_t), _i32p, C.c_int, C.POINTER(C.c_int))
    # fixed-size output pages
    sig("mi355lz4_compress_pages_device", C.c_int, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, C.c_size_t, vp, vp, vp, vp)
    sig("mi355lz4_compress_pages", C.c_int, vp, C.POINTER(_u8p), _i32p, C.c_int, C.c_int, C.c_int, C.c_int, _u8p, C.c_size_t,
        _i32p, _i32p, _i32p, _i32p)
    sig("mi355lz4_compress_pages_fast_device", C.c_int, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.c_size_t,
        vp, vp, vp, vp)
    sig("mi355lz4_compress_pages_fast", C.c_int, vp, C.POINTER(_u8p), _i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _u8p,
        C.c_size_t, _i32p, _i32p, _i32p, _i32p)
    sig("mi355lz4_compress_pages_fastdict_device", C.c_int, vp, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp,
        C.c_size_t, vp, vp, vp, vp)
    sig("mi355lz4_compress_pages_fastdict", C.c_int, vp, vp, C.POINTER(_u8p), _i32p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
        _u8p, C.c_size_t, _i32p, _i32p, _i32p, _i32p)
    # legacy face (include/lz4.h)
    sig("LZ4_createStream", vp)
    sig("LZ4_freeStream", C.c_int, vp)
    sig("LZ4_createStreamDecode", vp)
    sig("LZ4_freeStreamDecode", C.c_int, vp)
    sig("LZ4_compressBound", C.c_int, C.c_int)
    sig("LZ4_compress_fast_continue", C.c_int, vp, _u8p, _u8p, C.c_int, C.c_int, C.c_int)
    sig("LZ4_decompress_safe_continue", C.c_int, vp, _u8p, _u8p, C.c_int, C.c_int)
    # stream-combinator mirror
    sig("slz4_last_error", C.c_char_p)
    sig("slz4_engine_create", C.c_int, C.POINTER(vp), C.c_int, C.c_size_t)
    sig("slz4_engine_destroy", None, vp)
    sig("slz4_engine_set_batch", None, vp, C.c_size_t)
    sig("slz4_engine_set_linked_compress", None, vp, C.c_int)
    sig("slz4_engine_ctx", vp, vp)
    sig("slz4_arrays_count", C.c_size_t, vp)
    sig("slz4_arrays_flat", C.c_int, vp, C.POINTER(_u8p), C.POINTER(C.POINTER(C.c_size_t)))
    sig("slz4_arrays_len", C.c_size_t, vp, C.c_size_t)
    sig("slz4_arrays_data", _u8p, vp, C.c_size_t)
    sig("slz4_arrays_free", None, vp)
    sig("slz4_trim", None)
    sig("slz4_compress_chunks", C.c_int, vp, C.c_int, C.c_int, _u8p, _u64p, C.c_size_t, C.POINTER(vp))
    sig("slz4_resize_chunks", C.c_int, C.c_int, C.c_int, _u8p, _u64p, C.c_size_t, C.POINTER(vp))
    sig("slz4_decompress_chunks_raw", C.c_int, vp, C.c_int, _u8p, _u64p, C.c_size_t, C.POINTER(vp))
    sig("slz4_decompress_chunks", C.c_int, vp, C.c_int, C.c_int, _u8p, _u64p, C.c_size_t, C.POINTER(vp))
    sig("slz4_decompress_chunks_stream", C.c_int, vp, C.c_int, C.c_int, _u8p, _u64p, C.c_size_t, C.POINTER(vp))
    sig("slz4_decompress_chunks_with", C.c_int, vp, _u8p, _u64p, C.c_size_t, C.POINTER(vp))
    sig("slz4_simple_frame_parser", C.c_int, _u8p, _u64p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(vp))
    # standard LZ4 frames
    sig("slz4_xxh32", C.c_uint32, _u8p, C.c_size_t, C.c_uint32)
    sig("slz4_lz4frame_compress", C.c_int, vp, C.c_int, C.c_int, C.c_int, _u8p, C.c_size_t, C.POINTER(vp))
    sig("slz4_lz4frame_decompress", C.c_int, vp, _u8p, C.c_size_t, C.POINTER(vp))
    # batches of standard LZ4 frames on the device
    sig("mi355lz4_frames_create", C.c_int, vp, C.POINTER(vp))
    sig("mi355lz4_frames_destroy", None, vp)
    sig("mi355lz4_frames_load", C.c_int, vp, vp, vp, C.c_uint64, vp, vp, C.c_int, C.c_uint)
    sig("mi355lz4_frames_inputs", C.c_int, vp)
    sig("mi355lz4_frames_blocks", C.c_int, vp)
    sig("mi355lz4_frames_total", C.c_uint64, vp)
    sig("mi355lz4_frames_sizes", vp, vp)
    sig("mi355lz4_frames_get_sizes", C.c_int, vp, C.POINTER(C.c_int64))
    sig("mi355lz4_frames_decode", C.c_int, vp, vp, vp, vp, vp)
    sig("mi355lz4_decompress_frames", C.c_int, vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.c_int, C.c_uint, _u8p,
        C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int64))
    # writing batches of standard LZ4 frames on the device
    sig("mi355lz4_cframes_bound", C.c_uint64, C.c_uint64, C.c_int, C.c_uint)
    sig("mi355lz4_cframes_create", C.c_int, vp, C.POINTER(vp))
    sig("mi355lz4_cframes_destroy", None, vp)
    sig("mi355lz4_cframes_reserve", C.c_int, vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_int)
    sig("mi355lz4_cframes_compress", C.c_int, vp, vp, vp, C.c_uint64, vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_uint,
        C.c_int, vp, vp, vp, vp)
    sig("mi355lz4_compress_frames", C.c_int, vp, C.POINTER(_u8p), C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_uint, C.c_int, _u8p,
        C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int64))
    return L


lib = _load()

# every symbol include/mi355lz4.h and include/lz4.h declare (checked by tests without a GPU)
DECLARED_SYMBOLS = [
    "mi355lz4_version", "mi355lz4_last_error", "mi355lz4_device_count", "mi355lz4_create", "mi355lz4_destroy",
    "mi355lz4_set_stream", "mi355lz4_get_stream", "mi355lz4_synchronize", "mi355lz4_set_decoder", "mi355lz4_set_segments", "mi355lz4_set_linked_async", "mi355lz4_set_linked_compress",
    "mi355lz4_compress_bound", "mi355lz4_slot_stride", "mi355lz4_compress_batch_device", "mi355lz4_compact_device",
    "mi355lz4_decompress_batch_device", "mi355lz4_decompress_streams_device", "mi355lz4_decompress_linked_begin",
    "mi355lz4_decompress_linked_end", "mi355lz4_decompress_linked_end_last", "mi355lz4_index_device", "mi355lz4_compress_batch", "mi355lz4_index_host",
    "mi355lz4_decompress_batch", "mi355lz4_decompress_streams", "mi355lz4_generate_device", "mi355lz4_interleave_device", "mi355lz4_event_create",
    "mi355lz4_event_destroy", "mi355lz4_event_record", "mi355lz4_event_elapsed_ms",
    "mi355lz4_create_multi", "mi355lz4_destroy_multi", "mi355lz4_multi_device_count", "mi355lz4_multi_engine", "mi355lz4_multi_last_error",
    "mi355lz4_multi_compress_batch", "mi355lz4_multi_decompress_batch",
    "mi355lz4_set_block_checksum", "mi355lz4_slot_stride_ex", "mi355lz4_index_host_ex", "mi355lz4_xxh32_device",
    "mi355lz4_set_compression_level", "mi355lz4_get_compression_level",
    "mi355lz4_set_compress_exact", "mi355lz4_get_compress_exact", "mi355lz4_compress_exact_reset",
    "mi355lz4_cstreams_create", "mi355lz4_cstreams_destroy", "mi355lz4_cstreams_count", "mi355lz4_cstreams_reset",
    "mi355lz4_compress_streams_device", "mi355lz4_compress_streams",
    "mi355lz4_fstreams_create", "mi355lz4_fstreams_destroy", "mi355lz4_fstreams_count", "mi355lz4_fstreams_reset",
    "mi355lz4_fstreams_set_dict", "mi355lz4_compress_streams_fast_device", "mi355lz4_compress_streams_fast",
    "mi355lz4_fstreams_set_level", "mi355lz4_fstreams_get_level",
    "mi355lz4_decoded_size_device", "mi355lz4_decoded_sizes_host",
    "mi355lz4_decompress_partial_device", "mi355lz4_decompress_partial",
    "mi355lz4_dstreams_create", "mi355lz4_dstreams_destroy", "mi355lz4_dstreams_count", "mi355lz4_dstreams_reset",
    "mi355lz4_dstreams_set_dict", "mi355lz4_decompress_dstreams_device", "mi355lz4_decompress_dstreams",
    "mi355lz4_cstreams_load_dict", "mi355lz4_compress_dict_device", "mi355lz4_decompress_dict_device",
    "mi355lz4_compress_dict", "mi355lz4_decompress_dict",
    "mi355lz4_hcdict_create", "mi355lz4_hcdict_destroy", "mi355lz4_hcdict_load", "mi355lz4_hcdict_size",
    "mi355lz4_compress_hcdict_device", "mi355lz4_compress_hcdict",
    "mi355lz4_compress_fastdict_device", "mi355lz4_compress_fastdict",
    "mi355lz4_dictset_create", "mi355lz4_dictset_destroy", "mi355lz4_dictset_count",
    "mi355lz4_compress_fastdict_multi_device", "mi355lz4_compress_fastdict_multi",
    "mi355lz4_decompress_dict_multi_device", "mi355lz4_decompress_dict_multi",
    "mi355lz4_compress_pages_device", "mi355lz4_compress_pages",
    "mi355lz4_compress_pages_fast_device", "mi355lz4_compress_pages_fast",
    "mi355lz4_compress_pages_fastdict_device", "mi355lz4_compress_pages_fastdict",
    "mi355lz4_frames_create", "mi355lz4_frames_destroy", "mi355lz4_frames_load", "mi355lz4_frames_inputs",
    "mi355lz4_frames_blocks", "mi355lz4_frames_total", "mi355lz4_frames_sizes", "mi355lz4_frames_get_sizes",
    "mi355lz4_frames_decode", "mi355lz4_decompress_frames",
    "mi355lz4_cframes_bound", "mi355lz4_cframes_create", "mi355lz4_cframes_destroy", "mi355lz4_cframes_reserve",
    "mi355lz4_cframes_compress", "mi355lz4_compress_frames",
    "LZ4_createStream", "LZ4_freeStream", "LZ4_createStreamDecode", "LZ4_freeStreamDecode", "LZ4_compressBound",
    "LZ4_compress_fast_continue", "LZ4_decompress_safe_continue",
]


def _err():
    return (lib.mi355lz4_last_error() or b"").decode("utf-8", "replace")


def _check(rc, what=""):
    if rc != 0:
        raise LZ4Error("%s failed (%d): %s" % (what or "mi355lz4 call", rc, _err()))


def compress_bound(n):
    return lib.mi355lz4_compress_bound(int(n))


def slot_stride(block_len, header_kind=8):
    return lib.mi355lz4_slot_stride(int(block_len), int(header_kind))


def slot_stride_ex(block_len, header_kind=8, block_checksum=False):
    return lib.mi355lz4_slot_stride_ex(int(block_len), int(header_kind), int(bool(block_checksum)))


def index_host(framed, header_kind=8, fixed_uncomp=0, block_checksum=False, max_blocks=None):
    """Walk a dense framed stream's header chain on the host (mi355lz4_index_host_ex).  Returns (block offsets, uncompressed
    sizes); raises LZ4Error on a malformed chain."""
    src = np.frombuffer(bytes(framed), dtype=np.uint8)
    if max_blocks is None:
        max_blocks = src.size // (header_kind + 1) + 1
    boff = np.zeros(max_blocks + 1, dtype=np.uint64)
    ulen = np.zeros(max_blocks + 1, dtype=np.int32)
    nb = C.c_int()
    _check(lib.mi355lz4_index_host_ex(src.ctypes.data_as(_u8p), src.size, int(header_kind), int(fixed_uncomp),
                                      int(bool(block_checksum)), boff.ctypes.data_as(_u64p), ulen.ctypes.data_as(_i32p),
                                      int(max_blocks), C.byref(nb)), "index_host_ex")
    return boff[: nb.value].tolist(), ulen[: nb.value].tolist()


def device_count():
    return lib.mi355lz4_device_count()


# ---------------------------------------------------------------------------
# Config mirror (reference src/Streamly/Internal/LZ4/Config.hs)
# ---------------------------------------------------------------------------
class BlockSize:
    BlockHasSize = 0
    BlockMax64KB = 1
    BlockMax256KB = 2
    BlockMax1MB = 3
    BlockMax4MB = 4


class BlockConfig:
    def __init__(self, blockSize=BlockSize.BlockHasSize, blockChecksum=False):
        self.blockSize = blockSize
        self.blockChecksum = bool(blockChecksum)   # Config.hs:151: xxh32 of every block's data behind it

    @property
    def _kind(self):  # the C surface's kind: BlockSize, plus SLZ4_BLOCK_CHECKSUM (0x100)
        return int(self.blockSize) | (0x100 if self.blockChecksum else 0)

    @property
    def metaSize(self):  # Internal/LZ4.hs:177-181
        return 8 if self.blockSize == BlockSize.BlockHasSize else 4

    @property
    def fixedUncomp(self):  # Internal/LZ4.hs:189-198
        return {0: 0, 1: 64 << 10, 2: 256 << 10, 3: 1 << 20, 4: 4 << 20}[self.blockSize]


class FrameConfig:
    def __init__(self, hasEndMark=False):
        self.hasEndMark = hasEndMark


defaultBlockConfig = BlockConfig()
defaultFrameConfig = FrameConfig()


def setBlockMaxSize(bs, cfg):
    return BlockConfig(bs, cfg.blockChecksum)


def setBlockChecksum(v, cfg):
    """Config.hs:151 (undefined in the reference): every block carries the xxh32 of its data behind it."""
    return BlockConfig(cfg.blockSize, v)


def setFrameEndMark(v, cfg):
    return FrameConfig(bool(v))


# ---------------------------------------------------------------------------
# Engine
# ---------------------------------------------------------------------------
def _dptr(x):
    """Device pointer of a torch tensor / int / None."""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    return C.c_void_p(x.data_ptr())


class Event:
    def __init__(self):
        self.h = C.c_void_p()
        _check(lib.mi355lz4_event_create(C.byref(self.h)), "event_create")

    def __del__(self):
        try:
            if self.h:
                lib.mi355lz4_event_destroy(self.h)
        except Exception:
            pass


class MultiEngine:
    """Several GPUs behind one handle, one process (include/mi355lz4.h, "several GPUs behind one handle"): the host-buffer
    calls of Engine with the batch cut into one contiguous block range per device.  devices: list of HIP device ordinals
    (the same one may be named more than once: two engines on one GPU)."""

    def __init__(self, devices):
        self._h = C.c_void_p()
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        rc = lib.mi355lz4_create_multi(C.byref(self._h), arr, len(devices))
        if rc != 0:
            lib.mi355lz4_multi_last_error.restype = C.c_char_p
            raise LZ4Error("create_multi failed (%d): %s" % (rc, (lib.mi355lz4_multi_last_error() or b"").decode()))
        self.n = len(devices)

    def close(self):
        if self._h:
            lib.mi355lz4_destroy_multi(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _raise(self, rc, what, allow_block_error):
        if rc != 0 and not (allow_block_error and rc == -5):
            lib.mi355lz4_multi_last_error.restype = C.c_char_p
            raise LZ4Error("%s failed (%d): %s" % (what, rc, (lib.mi355lz4_multi_last_error() or b"").decode()))

    def set_block_checksum(self, on):
        """Block checksums on every engine of the handle (include/mi355lz4.h, mi355lz4_set_block_checksum)."""
        lib.mi355lz4_multi_engine.restype = C.c_void_p
        for i in range(self.n):
            _check(lib.mi355lz4_set_block_checksum(C.c_void_p(lib.mi355lz4_multi_engine(self._h, i)), int(bool(on))),
                   "set_block_checksum")
        self._block_checksum = bool(on)

    def set_compression_level(self, level):
        """Compression level on every engine of the handle (include/mi355lz4.h, mi355lz4_set_compression_level)."""
        lib.mi355lz4_multi_engine.restype = C.c_void_p
        for i in range(self.n):
            _check(lib.mi355lz4_set_compression_level(C.c_void_p(lib.mi355lz4_multi_engine(self._h, i)), int(level)),
                   "set_compression_level")

    def set_decoder(self, variant):
        lib.mi355lz4_multi_engine.restype = C.c_void_p
        for i in range(self.n):
            _check(lib.mi355lz4_set_decoder(C.c_void_p(lib.mi355lz4_multi_engine(self._h, i)), int(variant)), "set_decoder")

    def compress_batch(self, blocks, accel=1, header_kind=8):
        """blocks: list of bytes-like.  Returns (framed bytes, [framed length per block])."""
        n = len(blocks)
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in blocks]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in arrs])
        lens = np.array([a.size for a in arrs], dtype=np.int32)
        cap = int(sum(compress_bound(int(x)) + header_kind + 4 for x in lens)) + 16
        out = np.empty(cap, dtype=np.uint8)
        out_len = C.c_size_t()
        flen = np.zeros(max(n, 1), dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        rc = lib.mi355lz4_multi_compress_batch(self._h, ptrs, lens.ctypes.data_as(_i32p), n, int(accel), int(header_kind),
                                               out.ctypes.data_as(_u8p), C.c_size_t(cap), C.byref(out_len),
                                               flen.ctypes.data_as(_i32p), status.ctypes.data_as(_i32p))
        self._raise(rc, "multi_compress_batch", False)
        return out[: out_len.value].tobytes(), flen[:n].tolist()

    def decompress_batch(self, framed, header_kind=8, fixed_uncomp=0, raise_on_block_error=True):
        """Returns (decoded bytes, [decoded length or negative code per block])."""
        src = np.frombuffer(bytes(framed), dtype=np.uint8)
        max_blocks = src.size // (header_kind + 1) + 1
        boff = np.zeros(max_blocks + 1, dtype=np.uint64)
        ulen = np.zeros(max_blocks + 1, dtype=np.int32)
        nb = C.c_int()
        _check(lib.mi355lz4_index_host_ex(src.ctypes.data_as(_u8p), src.size, header_kind, fixed_uncomp,
                                          int(getattr(self, "_block_checksum", False)), boff.ctypes.data_as(_u64p),
                                          ulen.ctypes.data_as(_i32p), max_blocks, C.byref(nb)), "index_host")
        cap = int(ulen[: nb.value].astype(np.int64).clip(min=0).sum()) + 16
        out = np.empty(cap, dtype=np.uint8)
        out_len = C.c_size_t()
        blen = np.zeros(max(nb.value, 1), dtype=np.int32)
        got = C.c_int()
        rc = lib.mi355lz4_multi_decompress_batch(self._h, src.ctypes.data_as(_u8p), C.c_size_t(src.size), header_kind, fixed_uncomp,
                                                 out.ctypes.data_as(_u8p), C.c_size_t(cap), C.byref(out_len),
                                                 blen.ctypes.data_as(_i32p), max(nb.value, 1), C.byref(got))
        self._raise(rc, "multi_decompress_batch", not raise_on_block_error)
        return out[: out_len.value].tobytes(), blen[: got.value].tolist()


class Engine:
    """One GPU engine (HIP device + stream).  Wraps mi355lz4_ctx and the C++ stream-combinator engine."""

    def __init__(self, device=0, batch_blocks=4096):
        self._h = C.c_void_p()
        if lib.slz4_engine_create(C.byref(self._h), int(device), int(batch_blocks)) != 0:
            raise LZ4Error((lib.slz4_last_error() or b"").decode())
        self.ctx = C.c_void_p(lib.slz4_engine_ctx(self._h))
        self.device = device
        # The engine creates a non-blocking stream of its own.  The tensors this binding is handed are produced
        # and consumed by torch on torch's CURRENT stream, so every device-API call launches there: the stream is
        # re-read on each call (it changes under `with torch.cuda.stream(s):`), and a `torch.zeros(...)` followed
        # by a decode into that tensor is ordered without an explicit synchronisation.  use_stream() pins the
        # engine to one stream instead.
        self._pinned = False
        self._cur_stream = None
        self._block_checksum = False
        self._follow_torch()

    def _follow_torch(self):
        """Launch on torch's current stream for this device (torch may be imported after the engine)."""
        if self._pinned:
            return
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available():
            s = torch.cuda.current_stream(self.device).cuda_stream
            if s != self._cur_stream:
                _check(lib.mi355lz4_set_stream(self.ctx, C.c_void_p(s)), "set_stream")
                self._cur_stream = s

    def close(self):
        if self._h:
            lib.slz4_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_batch_blocks(self, n):
        lib.slz4_engine_set_batch(self._h, int(n))

    @staticmethod
    def has_experiments():
        """True when the loaded library is the experiment build (make lib-exp): decoder variant 3 exists."""
        try:
            f = lib.mi355lz4_debug_has_experiments
        except AttributeError:
            return False
        f.restype = C.c_int
        return bool(f())

    # kernels of the lane-parallel decode family that kernel_info() knows (mi355lz4_debug_kernel_info)
    DECODE_KERNELS = ("k_decode_par", "k_decode_par_redo", "k_decode_dict", "k_decode_par_partial", "k_decode_par_partial_redo",
                      "k_decode_dstreams", "k_decode_fixup_linked", "k_decode_fixup_runs", "k_runin_decode", "k_runin_fix",
                      "k_decode_tolerant")

    def kernel_info(self, kernel="k_decode_par"):
        """What the HIP runtime says about a decode kernel on this device: resident workgroups (= waves) per CU, static LDS
        bytes, registers, and sizeof(ParLds) of the build."""
        out = (C.c_int * 4)()
        _check(lib.mi355lz4_debug_kernel_info(self.ctx, self.DECODE_KERNELS.index(kernel), out), "debug_kernel_info")
        return {"resident_per_cu": int(out[0]), "lds_bytes": int(out[1]), "regs": int(out[2]), "par_lds_bytes": int(out[3])}

    def set_decoder(self, variant):
        _check(lib.mi355lz4_set_decoder(self.ctx, int(variant)), "set_decoder")

    def set_linked_compress(self, on):
        """Compress calls write ONE linked stream (previous block = dictionary), like the reference's compressor."""
        lib.slz4_engine_set_linked_compress(self._h, int(bool(on)))

    def set_block_checksum(self, on):
        """Every block carries its xxh32 behind its data: written by the compress calls, verified on the device by every
        decode call (include/mi355lz4.h, mi355lz4_set_block_checksum; Config.hs setBlockChecksum)."""
        _check(lib.mi355lz4_set_block_checksum(self.ctx, int(bool(on))), "set_block_checksum")
        self._block_checksum = bool(on)

    def set_compression_level(self, level):
        """0 (default): the fast encoder.  1..9: the hash-chain encoder (LZ4HC's levels: chain depth 2^(level-1), lazy
        parse; smaller output, `accel` ignored); 10..12 behave as 9.  Every compress call of the engine -- device and host
        calls, compressChunks, frames -- uses it (include/mi355lz4.h, mi355lz4_set_compression_level)."""
        _check(lib.mi355lz4_set_compression_level(self.ctx, int(level)), "set_compression_level")

    @property
    def compression_level(self):
        """The effective compression level (0..9)."""
        return int(lib.mi355lz4_get_compression_level(self.ctx))

    def set_compress_exact(self, on):
        """Reference-exact compression: every compress call (device and host calls, compressChunks) appends its blocks to
        ONE stream whose bytes are LZ4_compress_fast_continue's over separately allocated arrays -- what the reference's
        compressChunksD writes.  Switching it on starts a new stream (include/mi355lz4.h, mi355lz4_set_compress_exact)."""
        _check(lib.mi355lz4_set_compress_exact(self.ctx, int(bool(on))), "set_compress_exact")

    @property
    def compress_exact(self):
        return bool(lib.mi355lz4_get_compress_exact(self.ctx) == 1)

    def reset_compress_stream(self):
        """Start a new exact stream (LZ4_createStream); compressChunks does it when it starts."""
        _check(lib.mi355lz4_compress_exact_reset(self.ctx), "compress_exact_reset")

    def exact_state(self):
        """Diagnostics of the last exact compress call: (pieces, speculated, kept, redone)."""
        st = (C.c_int * 4)()
        _check(lib.mi355lz4_debug_exact_state(self.ctx, st), "debug_exact_state")
        return tuple(int(v) for v in st)

    def xxh32_device(self, base, off, length, n, seed, out):
        """out[i] = xxh32(seed) of base[off[i] : off[i] + length[i]] for i < n (uint8 / int64 / int32 / int32 device
        tensors); asynchronous on the engine's stream."""
        self._follow_torch()
        _check(lib.mi355lz4_xxh32_device(self.ctx, _dptr(base), _dptr(off), _dptr(length), int(n), int(seed) & 0xFFFFFFFF,
                                         _dptr(out)), "xxh32_device")

    def set_linked_async(self, max_decoded_block_size):
        """Linked device decodes enqueue only, no host wait (include/mi355lz4.h); 0 = default (wait)."""
        _check(lib.mi355lz4_set_linked_async(self.ctx, int(max_decoded_block_size)), "set_linked_async")

    def set_segments(self, segs):
        """Small-batch compression: segments per block (-1 automatic, 0 off, 2..64 forced); include/mi355lz4.h."""
        _check(lib.mi355lz4_set_segments(self.ctx, int(segs)), "set_segments")

    def use_stream(self, hip_stream):
        """Pin the engine to one caller-owned hipStream_t (stops following torch's current stream)."""
        _check(lib.mi355lz4_set_stream(self.ctx, C.c_void_p(hip_stream)), "set_stream")
        self._pinned = True
        self._cur_stream = hip_stream

    def synchronize(self):
        _check(lib.mi355lz4_synchronize(self.ctx), "synchronize")

    # ---- timing on the engine's own stream ---------------------------------
    def record(self, ev):
        self._follow_torch()
        _check(lib.mi355lz4_event_record(self.ctx, ev.h), "event_record")

    @staticmethod
    def elapsed_ms(start, stop):
        ms = C.c_float()
        _check(lib.mi355lz4_event_elapsed_ms(start.h, stop.h, C.byref(ms)), "event_elapsed")
        return ms.value

    # ---- device-resident batched API (torch uint8/int32/int64 CUDA tensors) ----
    def generate(self, kind, dst, block_len, n_blocks, first_block=0, block_step=1, lit_max=16, off_max=2048):
        self._follow_torch()
        k = {"random": 0, "lzsynth": 1, "text": 2}[kind]
        _check(lib.mi355lz4_generate_device(self.ctx, k, _dptr(dst), int(block_len), int(n_blocks), int(first_block),
                                            int(block_step), int(lit_max), int(off_max)), "generate_device")

    def compress_batch_device(self, src, n_blocks, max_block_len, slots, slot_stride_, framed_len, accel=1,
                              header_kind=8, src_off=None, src_len=None, block_stride=None):
        self._follow_torch()
        _check(lib.mi355lz4_compress_batch_device(
            self.ctx, _dptr(src), _dptr(src_off), _dptr(src_len),
            int(max_block_len if block_stride is None else block_stride), int(max_block_len), int(n_blocks),
            int(accel), int(header_kind), _dptr(slots), int(slot_stride_), _dptr(framed_len)), "compress_batch_device")

    def compact_device(self, slots, slot_stride_, framed_len, n_blocks, dense, dense_cap, dense_off):
        self._follow_torch()
        _check(lib.mi355lz4_compact_device(self.ctx, _dptr(slots), int(slot_stride_), _dptr(framed_len), int(n_blocks),
                                           _dptr(dense), int(dense_cap), _dptr(dense_off)), "compact_device")

    def decompress_batch_device(self, framed, framed_len, block_off, n_blocks, out, out_off, result, header_kind=8,
                                fixed_uncomp=0, linked=False, out_cap=None):
        self._follow_torch()
        _check(lib.mi355lz4_decompress_batch_device(
            self.ctx, _dptr(framed), int(framed_len), _dptr(block_off), int(n_blocks), int(header_kind),
            int(fixed_uncomp), int(bool(linked)), _dptr(out), _dptr(out_off), _dptr(out_cap), _dptr(result)),
            "decompress_batch_device")

    def decompress_partial_device(self, framed, framed_len, block_off, n_blocks, out, out_off, target, result, header_kind=8,
                                  fixed_uncomp=0, out_cap=None):
        """The first target[i] bytes of every block (int32 device tensor): result[i] and the bytes are those of
        LZ4_decompress_safe_partial; nothing outside [out_off[i], out_off[i] + min(target[i], cap_i)) is written.
        Enqueues only (include/mi355lz4.h, mi355lz4_decompress_partial_device)."""
        self._follow_torch()
        _check(lib.mi355lz4_decompress_partial_device(
            self.ctx, _dptr(framed), int(framed_len), _dptr(block_off), int(n_blocks), int(header_kind),
            int(fixed_uncomp), _dptr(out), _dptr(out_off), _dptr(out_cap), _dptr(target), _dptr(result)),
            "decompress_partial_device")

    def decompress_streams_device(self, framed, framed_len, block_off, n_blocks, stream_first, n_streams, out,
                                  out_off, result, header_kind=8, fixed_uncomp=0, out_cap=None):
        self._follow_torch()
        """Linked streams: stream s = blocks [stream_first[s], stream_first[s+1]) (int32 device tensor)."""
        _check(lib.mi355lz4_decompress_streams_device(
            self.ctx, _dptr(framed), int(framed_len), _dptr(block_off), int(n_blocks), int(header_kind),
            int(fixed_uncomp), _dptr(stream_first), int(n_streams), _dptr(out), _dptr(out_off), _dptr(out_cap),
            _dptr(result)), "decompress_streams_device")

    def decompress_linked_begin(self, framed, framed_len, block_off, n_blocks, out, out_off, result, look_back,
                                header_kind=8, fixed_uncomp=0):
        """First half of a linked decode of a contiguous RANGE of one stream (include/mi355lz4.h): everything that does
        not read the output of the block in front of the range.  With look_back = 1, out_off (int64, n_blocks + 2) and
        result (int32, n_blocks + 1) carry one leading entry for that block: where its output will be and its size."""
        self._follow_torch()
        lb = 1 if look_back else 0
        _check(lib.mi355lz4_decompress_linked_begin(
            self.ctx, _dptr(framed), int(framed_len), _dptr(block_off), int(n_blocks), int(header_kind), int(fixed_uncomp),
            _dptr(out), C.c_void_p(out_off.data_ptr() + 8 * lb), None, C.c_void_p(result.data_ptr() + 4 * lb), lb),
            "decompress_linked_begin")

    def decompress_linked_end_last(self):
        """Between begin and end: make the range's LAST block final ahead of the rest.  True: its bytes and result are
        final (hand them on, call decompress_linked_end afterwards); False: not available this way, call
        decompress_linked_end first."""
        self._follow_torch()
        r = lib.mi355lz4_decompress_linked_end_last(self.ctx)
        if r < 0:
            _check(r, "decompress_linked_end_last")
        return r == 1

    def decompress_linked_end(self):
        """Second half: fetch from the roots (the first of which lie in the look-back block's output), results."""
        self._follow_torch()
        _check(lib.mi355lz4_decompress_linked_end(self.ctx), "decompress_linked_end")

    def index_device(self, framed, framed_len, block_off, n_blocks, out_off, header_kind=8, fixed_uncomp=0):
        self._follow_torch()
        _check(lib.mi355lz4_index_device(self.ctx, _dptr(framed), int(framed_len), _dptr(block_off), int(n_blocks),
                                         int(header_kind), int(fixed_uncomp), _dptr(out_off)), "index_device")

    def decoded_size_device(self, framed, framed_len, block_off, n_blocks, size, out_off=None, header_kind=4, max_uncomp=0):
        """size[i] (int32, device) = what block i decodes to, read off its token chain, or BLK_E_SIZE_UNKNOWN / a header
        code; out_off (uint64, n_blocks + 1 entries, optional) = exclusive scan of the known sizes.  Enqueues only."""
        self._follow_torch()
        _check(lib.mi355lz4_decoded_size_device(self.ctx, _dptr(framed), int(framed_len), _dptr(block_off), int(n_blocks),
                                                int(header_kind), int(max_uncomp), _dptr(size),
                                                _dptr(out_off) if out_off is not None else None), "decoded_size_device")

    def decoded_sizes(self, framed, header_kind=4, max_uncomp=0):
        """Decoded size of every block of a dense framed stream in host memory, without decoding it: np.int32[], a size or
        a negative per-block code (BLK_E_SIZE_UNKNOWN where the token chain gives none of at most max_uncomp bytes)."""
        import torch
        boff, _ = index_host(framed, header_kind, max_uncomp, self._block_checksum)
        n = len(boff)
        if n == 0:
            return np.zeros(0, dtype=np.int32)
        dev = "cuda:%d" % self.device
        src = torch.from_numpy(np.frombuffer(bytes(framed), dtype=np.uint8).copy()).to(dev)
        off = torch.from_numpy(np.asarray(boff, dtype=np.int64)).to(dev)
        size = torch.empty(n, dtype=torch.int32, device=dev)
        self.decoded_size_device(src, src.numel(), off, n, size, None, header_kind, max_uncomp)
        self.synchronize()
        return size.cpu().numpy()

    def interleave_device(self, local, local_off, n_local, rank, n_ranks, global_buf, global_off):
        self._follow_torch()
        _check(lib.mi355lz4_interleave_device(self.ctx, _dptr(local), _dptr(local_off), int(n_local), int(rank),
                                              int(n_ranks), _dptr(global_buf), _dptr(global_off)), "interleave_device")

    # ---- host-buffer batched API -------------------------------------------
    def compress_batch(self, blocks, accel=1, header_kind=8):
        """blocks: list of bytes-like.  Returns (framed bytes, [framed length per block])."""
        n = len(blocks)
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in blocks]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in arrs])
        lens = np.array([a.size for a in arrs], dtype=np.int32)
        cap = int(sum(compress_bound(int(x)) + header_kind + 4 for x in lens)) + 16
        out = np.empty(cap, dtype=np.uint8)
        out_len = C.c_size_t()
        flen = np.zeros(max(n, 1), dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib.mi355lz4_compress_batch(self.ctx, ptrs, lens.ctypes.data_as(_i32p), n, int(accel), int(header_kind),
                                           out.ctypes.data_as(_u8p), cap, C.byref(out_len),
                                           flen.ctypes.data_as(_i32p), status.ctypes.data_as(_i32p)), "compress_batch")
        return out[: out_len.value].tobytes(), flen[:n].tolist()

    def decompress_batch(self, framed, header_kind=8, fixed_uncomp=0, linked=False, dict_bytes=None, max_blocks=None,
                         raise_on_block_error=True, cap=None):
        """Returns (decoded bytes, [decoded length or negative code per block]).  cap: bytes of output buffer to offer
        (default: every block at its header's size, or at fixed_uncomp)."""
        src = np.frombuffer(bytes(framed), dtype=np.uint8)
        if max_blocks is None:
            max_blocks = src.size // (header_kind + 1) + 1
        boff = np.zeros(max_blocks + 1, dtype=np.uint64)
        ulen = np.zeros(max_blocks + 1, dtype=np.int32)
        nb = C.c_int()
        _check(lib.mi355lz4_index_host_ex(src.ctypes.data_as(_u8p), src.size, header_kind, fixed_uncomp,
                                          int(self._block_checksum), boff.ctypes.data_as(_u64p),
                                          ulen.ctypes.data_as(_i32p), max_blocks, C.byref(nb)), "index_host")
        if cap is None:
            cap = int(ulen[: nb.value].astype(np.int64).clip(min=0).sum()) + 16
        cap = int(cap)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        out_len = C.c_size_t()
        blen = np.zeros(max(nb.value, 1), dtype=np.int32)
        got = C.c_int()
        d = np.frombuffer(bytes(dict_bytes), dtype=np.uint8) if dict_bytes else None
        rc = lib.mi355lz4_decompress_batch(self.ctx, src.ctypes.data_as(_u8p), src.size, header_kind, fixed_uncomp,
                                           int(bool(linked)), d.ctypes.data_as(_u8p) if d is not None else None,
                                           d.size if d is not None else 0, out.ctypes.data_as(_u8p), cap,
                                           C.byref(out_len), blen.ctypes.data_as(_i32p), max(nb.value, 1), C.byref(got))
        if rc != 0 and (raise_on_block_error or rc != -5):
            _check(rc, "decompress_batch")
        return out[: out_len.value].tobytes(), blen[: got.value].tolist()

    def decompress_partial(self, framed, target, header_kind=8, fixed_uncomp=0, max_blocks=None, raise_on_block_error=True,
                           cap=None):
        """The first `target` bytes of every block of a framed chain in host memory (an int for all blocks, or one per
        block).  Returns (the prefixes packed back to back, [result per block]); mi355lz4_decompress_partial.  cap: bytes of
        output buffer to offer (default: what the targets can ask for)."""
        src = np.frombuffer(bytes(framed), dtype=np.uint8)
        if max_blocks is None:
            max_blocks = src.size // (header_kind + 1) + 1
        per_block = not isinstance(target, (int, np.integer))
        tarr = np.ascontiguousarray(target, dtype=np.int32) if per_block else None
        if cap is None:
            boff, ulen = index_host(framed, header_kind, fixed_uncomp, self._block_checksum)
            u = np.asarray(ulen, dtype=np.int64).clip(min=0)
            t = tarr[: len(u)].astype(np.int64) if per_block else np.full(len(u), int(target), dtype=np.int64)
            if per_block and tarr.size < len(u):
                raise ValueError("decompress_partial: %d targets for %d blocks" % (tarr.size, len(u)))
            cap = int(np.minimum(u, t.clip(min=0)).sum()) + 16
        elif per_block:
            boff, _ = index_host(framed, header_kind, fixed_uncomp, self._block_checksum)
            if tarr.size < len(boff):
                raise ValueError("decompress_partial: %d targets for %d blocks" % (tarr.size, len(boff)))
        cap = int(cap)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        out_len = C.c_size_t()
        blen = np.zeros(max(max_blocks, 1), dtype=np.int32)
        got = C.c_int()
        rc = lib.mi355lz4_decompress_partial(self.ctx, src.ctypes.data_as(_u8p), src.size, int(header_kind), int(fixed_uncomp),
                                             tarr.ctypes.data_as(_i32p) if per_block else None, 0 if per_block else int(target),
                                             out.ctypes.data_as(_u8p), cap, C.byref(out_len), blen.ctypes.data_as(_i32p),
                                             int(max_blocks), C.byref(got))
        if rc != 0 and (raise_on_block_error or rc != -5):
            _check(rc, "decompress_partial")
        return out[: out_len.value].tobytes(), blen[: got.value].tolist()

    def compress_streams_device(self, cs, src, n_blocks, max_block_len, stream_first, stream_slot, slots, slot_stride_,
                                framed_len, accel=1, header_kind=8, src_off=None, src_len=None, block_stride=None):
        """Many reference-exact streams in one call (include/mi355lz4.h, mi355lz4_compress_streams_device): stream s is the
        blocks [stream_first[s], stream_first[s+1]) and continues slot stream_slot[s] of cs.  The block arguments are those
        of compress_batch_device (device tensors); stream_first / stream_slot are host sequences.  Only enqueues."""
        self._follow_torch()
        sf = np.ascontiguousarray(stream_first, dtype=np.int32)
        sl = np.ascontiguousarray(stream_slot, dtype=np.int32)
        if sf.size != sl.size + 1:
            raise ValueError("stream_first needs one entry more than stream_slot")
        _check(lib.mi355lz4_compress_streams_device(
            self.ctx, cs._h, _dptr(src), _dptr(src_off), _dptr(src_len),
            int(max_block_len if block_stride is None else block_stride), int(max_block_len), int(n_blocks),
            sf.ctypes.data_as(_i32p), sl.ctypes.data_as(_i32p), int(sl.size), int(accel), int(header_kind), _dptr(slots),
            int(slot_stride_), _dptr(framed_len)), "compress_streams_device")

    def compress_streams(self, streams, cs, slots=None, accel=1, header_kind=8):
        """streams: list of lists of bytes-like, stream s continuing slot slots[s] of cs (default: slot s).  Returns
        (framed bytes of all blocks in order, [framed length per block]); mi355lz4_compress_streams."""
        if slots is None:
            slots = list(range(len(streams)))
        blocks = [b for st in streams for b in st]
        n = len(blocks)
        sf = np.cumsum([0] + [len(st) for st in streams]).astype(np.int32)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        if sl.size != len(streams):
            raise ValueError("one slot per stream")
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in blocks]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in arrs])
        lens = np.array([a.size for a in arrs] + [0], dtype=np.int32)
        cap = int(sum(compress_bound(int(x)) + header_kind + 4 for x in lens[:n])) + 16
        out = np.empty(cap, dtype=np.uint8)
        out_len = C.c_size_t()
        flen = np.zeros(max(n, 1), dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib.mi355lz4_compress_streams(self.ctx, cs._h, ptrs, lens.ctypes.data_as(_i32p), n, sf.ctypes.data_as(_i32p),
                                             sl.ctypes.data_as(_i32p), int(sl.size), int(accel), int(header_kind),
                                             out.ctypes.data_as(_u8p), cap, C.byref(out_len), flen.ctypes.data_as(_i32p),
                                             status.ctypes.data_as(_i32p)), "compress_streams")
        return out[: out_len.value].tobytes(), flen[:n].tolist()

    def compress_streams_fast_device(self, fs, src, n_blocks, max_block_len, stream_first, stream_slot, slots, slot_stride_,
                                     framed_len, accel=1, header_kind=8, src_off=None, src_len=None, block_stride=None):
        """Many fast linked streams in one call (include/mi355lz4.h, mi355lz4_compress_streams_fast_device): the arguments of
        compress_streams_device with a FastCompressStreams in place of the CompressStreams.  Only enqueues."""
        self._follow_torch()
        sf = np.ascontiguousarray(stream_first, dtype=np.int32)
        sl = np.ascontiguousarray(stream_slot, dtype=np.int32)
        if sf.size != sl.size + 1:
            raise ValueError("stream_first needs one entry more than stream_slot")
        _check(lib.mi355lz4_compress_streams_fast_device(
            self.ctx, fs._h, _dptr(src), _dptr(src_off), _dptr(src_len),
            int(max_block_len if block_stride is None else block_stride), int(max_block_len), int(n_blocks),
            sf.ctypes.data_as(_i32p), sl.ctypes.data_as(_i32p), int(sl.size), int(accel), int(header_kind), _dptr(slots),
            int(slot_stride_), _dptr(framed_len)), "compress_streams_fast_device")

    def compress_streams_fast(self, streams, fs, slots=None, accel=1, header_kind=8):
        """streams: list of lists of bytes-like, stream s continuing slot slots[s] of fs (default: slot s).  Returns
        (framed bytes of all blocks in order, [framed length per block], [status per block]);
        mi355lz4_compress_streams_fast."""
        if slots is None:
            slots = list(range(len(streams)))
        blocks = [b for st in streams for b in st]
        n = len(blocks)
        sf = np.cumsum([0] + [len(st) for st in streams]).astype(np.int32)
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        if sl.size != len(streams):
            raise ValueError("one slot per stream")
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in blocks]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in arrs])
        lens = np.array([a.size for a in arrs] + [0], dtype=np.int32)
        cap = int(sum(compress_bound(int(x)) + header_kind + 4 for x in lens[:n])) + 16
        out = np.empty(cap, dtype=np.uint8)
        out_len = C.c_size_t()
        flen = np.zeros(max(n, 1), dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib.mi355lz4_compress_streams_fast(self.ctx, fs._h, ptrs, lens.ctypes.data_as(_i32p), n,
                                                  sf.ctypes.data_as(_i32p), sl.ctypes.data_as(_i32p), int(sl.size), int(accel),
                                                  int(header_kind), out.ctypes.data_as(_u8p), cap, C.byref(out_len),
                                                  flen.ctypes.data_as(_i32p), status.ctypes.data_as(_i32p)),
               "compress_streams_fast")
        return out[: out_len.value].tobytes(), flen[:n].tolist(), status[:n].tolist()

    def decompress_streams(self, framed, stream_first, header_kind=8, fixed_uncomp=0, raise_on_block_error=True):
        """Many linked streams, host buffers: stream s = blocks [stream_first[s], stream_first[s+1]).
        Returns (decoded bytes, [decoded length or negative code per block])."""
        src = np.frombuffer(bytes(framed), dtype=np.uint8)
        max_blocks = src.size // (header_kind + 1) + 1
        boff = np.zeros(max_blocks + 1, dtype=np.uint64)
        ulen = np.zeros(max_blocks + 1, dtype=np.int32)
        nb = C.c_int()
        _check(lib.mi355lz4_index_host_ex(src.ctypes.data_as(_u8p), src.size, header_kind, fixed_uncomp,
                                          int(self._block_checksum), boff.ctypes.data_as(_u64p),
                                          ulen.ctypes.data_as(_i32p), max_blocks, C.byref(nb)), "index_host")
        cap = int(ulen[: nb.value].astype(np.int64).clip(min=0).sum()) + 16
        out = np.empty(cap, dtype=np.uint8)
        out_len = C.c_size_t()
        blen = np.zeros(max(nb.value, 1), dtype=np.int32)
        got = C.c_int()
        sf = np.asarray(stream_first, dtype=np.int32)
        rc = lib.mi355lz4_decompress_streams(self.ctx, src.ctypes.data_as(_u8p), src.size, header_kind, fixed_uncomp,
                                             sf.ctypes.data_as(_i32p), int(sf.size - 1), out.ctypes.data_as(_u8p), cap,
                                             C.byref(out_len), blen.ctypes.data_as(_i32p), max(nb.value, 1), C.byref(got))
        if rc != 0 and (raise_on_block_error or rc != -5):
            _check(rc, "decompress_streams")
        return out[: out_len.value].tobytes(), blen[: got.value].tolist()

    def decompress_dstreams_device(self, ds, framed, framed_len, block_off, n_blocks, stream_first, stream_slot, out, out_off,
                                   result, header_kind=8, fixed_uncomp=0, out_cap=None):
        """Many linked decode streams continued across calls (include/mi355lz4.h, mi355lz4_decompress_dstreams_device):
        stream s is the blocks [stream_first[s], stream_first[s+1]) and continues slot stream_slot[s] of ds.  The block
        arguments are those of decompress_streams_device (device tensors); stream_first / stream_slot are host sequences.
        Only enqueues: per-block codes are in result."""
        self._follow_torch()
        sf = np.ascontiguousarray(stream_first, dtype=np.int32)
        sl = np.ascontiguousarray(stream_slot, dtype=np.int32)
        if sf.size != sl.size + 1:
            raise ValueError("stream_first needs one entry more than stream_slot")
        _check(lib.mi355lz4_decompress_dstreams_device(
            self.ctx, ds._h, _dptr(framed), int(framed_len), _dptr(block_off), int(n_blocks), int(header_kind),
            int(fixed_uncomp), sf.ctypes.data_as(_i32p), sl.ctypes.data_as(_i32p), int(sl.size), _dptr(out), _dptr(out_off),
            _dptr(out_cap), _dptr(result)), "decompress_dstreams_device")

    def decompress_dstreams(self, framed, stream_first, ds, slots=None, header_kind=8, fixed_uncomp=0,
                            raise_on_block_error=True, cap=None):
        """Host buffers: framed holds the next blocks of len(stream_first) - 1 linked streams back to back, stream s =
        blocks [stream_first[s], stream_first[s+1]) continuing slot slots[s] of ds (default: slot s).  Returns (decoded
        bytes, [decoded length or negative code per block]); mi355lz4_decompress_dstreams."""
        src = np.frombuffer(bytes(framed), dtype=np.uint8)
        sf = np.ascontiguousarray(stream_first, dtype=np.int32)
        if slots is None:
            slots = list(range(sf.size - 1))
        sl = np.ascontiguousarray(list(slots) + [0], dtype=np.int32)
        if sl.size != sf.size:
            raise ValueError("one slot per stream")
        max_blocks = src.size // (header_kind + 1) + 1
        if cap is None:
            try:
                _, ulen = index_host(framed, header_kind, fixed_uncomp, self._block_checksum)
            except LZ4Error:
                ulen = []                                   # (the call reports the chain itself)
            cap = int(np.asarray(ulen, dtype=np.int64).clip(min=0).sum()) + 16
        cap = int(cap)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        out_len = C.c_size_t()
        blen = np.zeros(max(max_blocks, 1), dtype=np.int32)
        got = C.c_int()
        rc = lib.mi355lz4_decompress_dstreams(self.ctx, ds._h, src.ctypes.data_as(_u8p) if src.size else None, src.size,
                                              int(header_kind), int(fixed_uncomp), sf.ctypes.data_as(_i32p),
                                              sl.ctypes.data_as(_i32p), int(sf.size - 1), out.ctypes.data_as(_u8p), cap,
                                              C.byref(out_len), blen.ctypes.data_as(_i32p), int(max_blocks), C.byref(got))
        if rc != 0 and (raise_on_block_error or rc != -5):
            _check(rc, "decompress_dstreams")
        return out[: out_len.value].tobytes(), blen[: got.value].tolist()

    def compress_dict_device(self, cs, dict_slot, src, n_blocks, max_block_len, slots, slot_stride_, framed_len, accel=1,
                             header_kind=8, src_off=None, src_len=None, block_stride=None):
        """A batch of independent blocks, every one compressed from a copy of slot dict_slot of cs (a slot that
        CompressStreams.load_dict has loaded): the reference's bytes for LZ4_loadDict + LZ4_compress_fast_continue on a copy
        of the loaded stream.  The block arguments are those of compress_batch_device; the slot is only read.  Only
        enqueues (include/mi355lz4.h, mi355lz4_compress_dict_device)."""
        self._follow_torch()
        _check(lib.mi355lz4_compress_dict_device(
            self.ctx, cs._h if cs is not None else None, int(dict_slot), _dptr(src), _dptr(src_off), _dptr(src_len),
            int(max_block_len if block_stride is None else block_stride), int(max_block_len), int(n_blocks),
            int(accel), int(header_kind), _dptr(slots), int(slot_stride_), _dptr(framed_len)), "compress_dict_device")

    def decompress_dict_device(self, framed, framed_len, block_off, n_blocks, dict_device, dict_len, out, out_off, result,
                               header_kind=8, fixed_uncomp=0, out_cap=None):
        """A batch of independent blocks, every one decoded against dict_device[:dict_len] (a uint8 device tensor, any
        length; 0: none): result[i] and the bytes are those of LZ4_decompress_safe_usingDict on its external-dictionary
        path.  The block arguments are those of decompress_batch_device.  Only enqueues; set_decoder is ignored
        (include/mi355lz4.h, mi355lz4_decompress_dict_device)."""
        self._follow_torch()
        _check(lib.mi355lz4_decompress_dict_device(
            self.ctx, _dptr(framed), int(framed_len), _dptr(block_off), int(n_blocks), int(header_kind), int(fixed_uncomp),
            _dptr(dict_device), int(dict_len), _dptr(out), _dptr(out_off), _dptr(out_cap), _dptr(result)),
            "decompress_dict_device")

    def compress_dict(self, blocks, cs, dict_slot=0, accel=1, header_kind=8):
        """blocks: list of bytes-like, every one compressed against slot dict_slot of cs.  Returns (framed bytes, [framed
        length per block]); mi355lz4_compress_dict."""
        n = len(blocks)
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in blocks]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in arrs])
        lens = np.array([a.size for a in arrs] + [0], dtype=np.int32)
        cap = int(sum(compress_bound(int(x)) + header_kind + 4 for x in lens[:n])) + 16
        out = np.empty(cap, dtype=np.uint8)
        out_len = C.c_size_t()
        flen = np.zeros(max(n, 1), dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib.mi355lz4_compress_dict(self.ctx, cs._h, int(dict_slot), ptrs, lens.ctypes.data_as(_i32p), n, int(accel),
                                          int(header_kind), out.ctypes.data_as(_u8p), cap, C.byref(out_len),
                                          flen.ctypes.data_as(_i32p), status.ctypes.data_as(_i32p)), "compress_dict")
        return out[: out_len.value].tobytes(), flen[:n].tolist()

    def compress_hcdict_device(self, hd, src, n_blocks, max_block_len, slots, slot_stride_, framed_len, header_kind=8,
                               src_off=None, src_len=None, block_stride=None):
        """A batch of independent blocks at the engine's compression level (1..12), every one with the dictionary of the
        HcDict hd in front of it: the bytes of block 1 of the linked call [dictionary, block] at that level.  The block
        arguments are those of compress_batch_device; hd is only read.  Only enqueues (include/mi355lz4.h,
        mi355lz4_compress_hcdict_device)."""
        self._follow_torch()
        _check(lib.mi355lz4_compress_hcdict_device(
            self.ctx, hd._h if hd is not None else None, _dptr(src), _dptr(src_off), _dptr(src_len),
            int(max_block_len if block_stride is None else block_stride), int(max_block_len), int(n_blocks),
            int(header_kind), _dptr(slots), int(slot_stride_), _dptr(framed_len)), "compress_hcdict_device")

    def compress_hcdict(self, blocks, hd, header_kind=8):
        """blocks: list of bytes-like, every one compressed at the engine's level against the HcDict hd.  Returns (framed
        bytes, [framed length per block]); mi355lz4_compress_hcdict."""
        n = len(blocks)
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in blocks]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in arrs])
        lens = np.array([a.size for a in arrs] + [0], dtype=np.int32)
        cap = int(sum(compress_bound(int(x)) + header_kind + 4 for x in lens[:n])) + 16
        out = np.empty(cap, dtype=np.uint8)
        out_len = C.c_size_t()
        flen = np.zeros(max(n, 1), dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib.mi355lz4_compress_hcdict(self.ctx, hd._h if hd is not None else None, ptrs, lens.ctypes.data_as(_i32p), n,
                                            int(header_kind), out.ctypes.data_as(_u8p), cap, C.byref(out_len),
                                            flen.ctypes.data_as(_i32p), status.ctypes.data_as(_i32p)), "compress_hcdict")
        return out[: out_len.value].tobytes(), flen[:n].tolist()

    def compress_fastdict_device(self, hd, src, n_blocks, max_block_len, slots, slot_stride_, framed_len, accel=1, header_kind=8,
                                 src_off=None, src_len=None, block_stride=None):
        """A batch of independent blocks at level 0 by the wave encoder, every one with the dictionary of the HcDict hd in
        front of it: the bytes of block 1 of the linked call [dictionary, block] with the same accel.  The block arguments
        are those of compress_batch_device; hd is only read.  Only enqueues (include/mi355lz4.h,
        mi355lz4_compress_fastdict_device)."""
        self._follow_torch()
        _check(lib.mi355lz4_compress_fastdict_device(
            self.ctx, hd._h if hd is not None else None, _dptr(src), _dptr(src_off), _dptr(src_len),
            int(max_block_len if block_stride is None else block_stride), int(max_block_len), int(n_blocks), int(accel),
            int(header_kind), _dptr(slots), int(slot_stride_), _dptr(framed_len)), "compress_fastdict_device")

    def compress_fastdict(self, blocks, hd, accel=1, header_kind=8):
        """blocks: list of bytes-like, every one compressed at level 0 by the wave encoder against the HcDict hd.  Returns
        (framed bytes, [framed length per block]); mi355lz4_compress_fastdict."""
        n = len(blocks)
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in blocks]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in arrs])
        lens = np.array([a.size for a in arrs] + [0], dtype=np.int32)
        cap = int(sum(compress_bound(max(int(x), 0)) + header_kind + 4 for x in lens[:n])) + 16
        out = np.empty(cap, dtype=np.uint8)
        out_len = C.c_size_t()
        flen = np.zeros(max(n, 1), dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib.mi355lz4_compress_fastdict(self.ctx, hd._h if hd is not None else None, ptrs, lens.ctypes.data_as(_i32p), n,
                                              int(accel), int(header_kind), out.ctypes.data_as(_u8p), cap, C.byref(out_len),
                                              flen.ctypes.data_as(_i32p), status.ctypes.data_as(_i32p)), "compress_fastdict")
        return out[: out_len.value].tobytes(), flen[:n].tolist()

    def compress_pages_device(self, src, src_off, src_len, n_inputs, page_size, max_pages, pages, page_stride, page_src_len,
                              page_comp_len, n_pages, consumed, header_kind=8):
        """Fixed-size output pages: input i (src[src_off[i] : src_off[i] + src_len[i]], device tensors) is cut into a chain of
        at most max_pages pages, page k being what LZ4_compress_destSize makes of the bytes behind pages 0..k-1 with
        page_size[i] as its targetDstSize: the reference's bytes at pages + (i * max_pages + k) * page_stride behind a header of
        header_kind (0, 4, 8) bytes, its return value in page_comp_len and its consumed count in page_src_len; n_pages[i] pages,
        consumed[i] bytes.  Only enqueues (include/mi355lz4.h, mi355lz4_compress_pages_device)."""
        self._follow_torch()
        _check(lib.mi355lz4_compress_pages_device(
            self.ctx, _dptr(src), _dptr(src_off), _dptr(src_len), int(n_inputs), _dptr(page_size), int(max_pages),
            int(header_kind), _dptr(pages), int(page_stride), _dptr(page_src_len), _dptr(page_comp_len), _dptr(n_pages),
            _dptr(consumed)), "compress_pages_device")

    def compress_pages_fast_device(self, src, src_off, src_len, n_inputs, page_size, max_pages, pages, page_stride, page_src_len,
                                   page_comp_len, n_pages, consumed, header_kind=8, accel=1):
        """compress_pages_device at the engine's speed: the same arguments, layout, chains and result arrays, every page made by
        the level-0 wave encoder with page_size[i] as its output budget -- a prefix of the sequences of the block that
        compress_batch_device writes for the next min(remaining, 65536) bytes, closed by the literal run that fills the page.
        Valid, independently decodable pages; not LZ4_compress_destSize's bytes.  Only enqueues (include/mi355lz4.h,
        mi355lz4_compress_pages_fast_device)."""
        self._follow_torch()
        _check(lib.mi355lz4_compress_pages_fast_device(
            self.ctx, _dptr(src), _dptr(src_off), _dptr(src_len), int(n_inputs), _dptr(page_size), int(max_pages), int(accel),
            int(header_kind), _dptr(pages), int(page_stride), _dptr(page_src_len), _dptr(page_comp_len), _dptr(n_pages),
            _dptr(consumed)), "compress_pages_fast_device")

    def compress_pages_fast(self, inputs, page_size, max_pages, header_kind=8, page_stride=None, accel=1):
        """compress_pages with the pages of compress_pages_fast_device; mi355lz4_compress_pages_fast."""
        return self.compress_pages(inputs, page_size, max_pages, header_kind, page_stride, _fast_accel=int(accel))

    def compress_pages_fastdict_device(self, hd, src, src_off, src_len, n_inputs, page_size, max_pages, pages, page_stride,
                                       page_src_len, page_comp_len, n_pages, consumed, header_kind=8, accel=1):
        """compress_pages_fast_device with the dictionary of the HcDict hd in front of every page: the same arguments, layout,
        chains and result arrays; a page holds the leading sequences of the block that compress_fastdict_device writes for the
        next min(remaining, 65536) bytes whose cuts are all valid, closed by the literal run that fills the page.  A page decodes
        with the same dictionary (decompress_dict_device); hd is only read.  Only enqueues (include/mi355lz4.h,
        mi355lz4_compress_pages_fastdict_device)."""
        self._follow_torch()
        _check(lib.mi355lz4_compress_pages_fastdict_device(
            self.ctx, hd._h if hd is not None else None, _dptr(src), _dptr(src_off), _dptr(src_len), int(n_inputs),
            _dptr(page_size), int(max_pages), int(accel), int(header_kind), _dptr(pages), int(page_stride), _dptr(page_src_len),
            _dptr(page_comp_len), _dptr(n_pages), _dptr(consumed)), "compress_pages_fastdict_device")

    def compress_pages_fastdict(self, inputs, hd, page_size, max_pages, header_kind=8, page_stride=None, accel=1):
        """compress_pages with the pages of compress_pages_fastdict_device; mi355lz4_compress_pages_fastdict."""
        return self.compress_pages(inputs, page_size, max_pages, header_kind, page_stride, _fast_accel=int(accel), _hd=(hd,))

    def compress_pages(self, inputs, page_size, max_pages, header_kind=8, page_stride=None, _fast_accel=None, _hd=None):
        """inputs: list of bytes-like, every one cut into pages of page_size compressed bytes.  Returns a list, per input, of
        (pages, consumed): pages a list of (page bytes with its header, bytes of the input it holds); mi355lz4_compress_pages."""
        n = len(inputs)
        if page_stride is None:
            page_stride = int(header_kind) + max(int(page_size), 1)
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in inputs]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in arrs])
        lens = np.array([a.size for a in arrs] + [0], dtype=np.int32)
        np_ = max(n * max(int(max_pages), 0), 1)
        pages = np.zeros(np_ * int(page_stride), dtype=np.uint8)
        psrc = np.zeros(np_, dtype=np.int32)
        pcomp = np.zeros(np_, dtype=np.int32)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        cons = np.zeros(max(n, 1), dtype=np.int32)
        tail = (int(header_kind), pages.ctypes.data_as(_u8p), int(page_stride), psrc.ctypes.data_as(_i32p),
                pcomp.ctypes.data_as(_i32p), cnt.ctypes.data_as(_i32p), cons.ctypes.data_as(_i32p))
        if _hd is not None:
            _check(lib.mi355lz4_compress_pages_fastdict(self.ctx, _hd[0]._h if _hd[0] is not None else None, ptrs,
                                                        lens.ctypes.data_as(_i32p), n, int(page_size), int(max_pages), _fast_accel,
                                                        *tail), "compress_pages_fastdict")
        elif _fast_accel is None:
            _check(lib.mi355lz4_compress_pages(self.ctx, ptrs, lens.ctypes.data_as(_i32p), n, int(page_size), int(max_pages),
                                               *tail), "compress_pages")
        else:
            _check(lib.mi355lz4_compress_pages_fast(self.ctx, ptrs, lens.ctypes.data_as(_i32p), n, int(page_size), int(max_pages),
                                                    _fast_accel, *tail), "compress_pages_fast")
        res = []
        for i in range(n):
            pl = []
            for k in range(int(cnt[i])):
                at = i * int(max_pages) + k
                lo = at * int(page_stride)
                pl.append((pages[lo: lo + int(header_kind) + int(pcomp[at])].tobytes(), int(psrc[at])))
            res.append((pl, int(cons[i])))
        return res

    def decompress_dict(self, framed, dict_bytes, header_kind=8, fixed_uncomp=0, max_blocks=None, raise_on_block_error=True,
                        cap=None):
        """A framed chain in host memory, every block decoded against dict_bytes (may be empty).  Returns (decoded bytes,
        [decoded length or negative code per block]); mi355lz4_decompress_dict."""
        src = np.frombuffer(bytes(framed), dtype=np.uint8)
        if max_blocks is None:
            max_blocks = src.size // (header_kind + 1) + 1
        if cap is None:
            _, ulen = index_host(framed, header_kind, fixed_uncomp, self._block_checksum)
            cap = int(np.asarray(ulen, dtype=np.int64).clip(min=0).sum()) + 16
        cap = int(cap)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        out_len = C.c_size_t()
        blen = np.zeros(max(max_blocks, 1), dtype=np.int32)
        got = C.c_int()
        d = np.frombuffer(bytes(dict_bytes), dtype=np.uint8) if dict_bytes else None
        rc = lib.mi355lz4_decompress_dict(self.ctx, src.ctypes.data_as(_u8p) if src.size else None, src.size, int(header_kind),
                                          int(fixed_uncomp), d.ctypes.data_as(_u8p) if d is not None else None,
                                          d.size if d is not None else 0, out.ctypes.data_as(_u8p), cap, C.byref(out_len),
                                          blen.ctypes.data_as(_i32p), int(max_blocks), C.byref(got))
        if rc != 0 and (raise_on_block_error or rc != -5):
            _check(rc, "decompress_dict")
        return out[: out_len.value].tobytes(), blen[: got.value].tolist()


    def compress_fastdict_multi_device(self, ds, dict_idx, src, n_blocks, max_block_len, slots, slot_stride_, framed_len, accel=1,
                                       header_kind=8, src_off=None, src_len=None, block_stride=None):
        """compress_fastdict_device with a dictionary per block: block i is compressed against member dict_idx[i] (an int32
        device tensor; -1: no dictionary) of the DictSet ds and comes out as compress_fastdict_device writes it against that
        member alone.  Any other index gives framed_len[i] = 0 and an untouched slot.  The set and its members are only read.
        Only enqueues (include/mi355lz4.h, mi355lz4_compress_fastdict_multi_device)."""
        self._follow_torch()
        _check(lib.mi355lz4_compress_fastdict_multi_device(
            self.ctx, ds._h if ds is not None else None, _dptr(dict_idx), _dptr(src), _dptr(src_off), _dptr(src_len),
            int(max_block_len if block_stride is None else block_stride), int(max_block_len), int(n_blocks), int(accel),
            int(header_kind), _dptr(slots), int(slot_stride_), _dptr(framed_len)), "compress_fastdict_multi_device")

    def compress_fastdict_multi(self, blocks, ds, dict_idx, accel=1, header_kind=8):
        """blocks: list of bytes-like, block i compressed at level 0 by the wave encoder against member dict_idx[i] of the
        DictSet ds (-1: none).  Returns (framed bytes, [framed length per block]); mi355lz4_compress_fastdict_multi."""
        n = len(blocks)
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else b for b in blocks]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) for a in arrs])
        lens = np.array([a.size for a in arrs] + [0], dtype=np.int32)
        idx = np.ascontiguousarray(np.asarray(list(dict_idx) + [0], dtype=np.int64).astype(np.int32))
        if idx.size != n + 1:
            raise ValueError("compress_fastdict_multi: one index per block")
        cap = int(sum(compress_bound(max(int(x), 0)) + header_kind + 4 for x in lens[:n])) + 16
        out = np.empty(cap, dtype=np.uint8)
        out_len = C.c_size_t()
        flen = np.zeros(max(n, 1), dtype=np.int32)
        status = np.zeros(max(n, 1), dtype=np.int32)
        _check(lib.mi355lz4_compress_fastdict_multi(self.ctx, ds._h if ds is not None else None, idx.ctypes.data_as(_i32p), ptrs,
                                                    lens.ctypes.data_as(_i32p), n, int(accel), int(header_kind),
                                                    out.ctypes.data_as(_u8p), cap, C.byref(out_len), flen.ctypes.data_as(_i32p),
                                                    status.ctypes.data_as(_i32p)), "compress_fastdict_multi")
        return out[: out_len.value].tobytes(), flen[:n].tolist()

    def decompress_dict_multi_device(self, framed, framed_len, block_off, n_blocks, ds, dict_idx, out, out_off, result,
                                     header_kind=8, fixed_uncomp=0, out_cap=None):
        """decompress_dict_device with a dictionary per block: block i is decoded against the kept bytes of member dict_idx[i]
        (an int32 device tensor; -1: no dictionary) of the DictSet ds.  Any other index gives result[i] = BLK_E_DICT and writes
        nothing.  Only enqueues (include/mi355lz4.h, mi355lz4_decompress_dict_multi_device)."""
        self._follow_torch()
        _check(lib.mi355lz4_decompress_dict_multi_device(
            self.ctx, _dptr(framed), int(framed_len), _dptr(block_off), int(n_blocks), int(header_kind), int(fixed_uncomp),
            ds._h if ds is not None else None, _dptr(dict_idx), _dptr(out), _dptr(out_off), _dptr(out_cap), _dptr(result)),
            "decompress_dict_multi_device")

    def decompress_dict_multi(self, framed, ds, dict_idx, header_kind=8, fixed_uncomp=0, max_blocks=None,
                              raise_on_block_error=True, cap=None):
        """A framed chain in host memory, block i decoded against member dict_idx[i] of the DictSet ds (-1: none).  Returns
        (decoded bytes, [decoded length or negative code per block]); mi355lz4_decompress_dict_multi."""
        src = np.frombuffer(bytes(framed), dtype=np.uint8)
        if max_blocks is None:
            max_blocks = src.size // (header_kind + 1) + 1
        if cap is None:
            _, ulen = index_host(framed, header_kind, fixed_uncomp, self._block_checksum)
            cap = int(np.asarray(ulen, dtype=np.int64).clip(min=0).sum()) + 16
        cap = int(cap)
        out = np.empty(max(cap, 1), dtype=np.uint8)
        out_len = C.c_size_t()
        blen = np.zeros(max(max_blocks, 1), dtype=np.int32)
        got = C.c_int()
        idx = np.zeros(max(max_blocks, 1), dtype=np.int32)
        given = np.asarray(list(dict_idx), dtype=np.int64).astype(np.int32)[: idx.size]
        idx[: given.size] = given
        rc = lib.mi355lz4_decompress_dict_multi(self.ctx, src.ctypes.data_as(_u8p) if src.size else None, src.size,
                                                int(header_kind), int(fixed_uncomp), ds._h if ds is not None else None,
                                                idx.ctypes.data_as(_i32p), out.ctypes.data_as(_u8p), cap, C.byref(out_len),
                                                blen.ctypes.data_as(_i32p), int(max_blocks), C.byref(got))
        if rc != 0 and (raise_on_block_error or rc != -5):
            _check(rc, "decompress_dict_multi")
        return out[: out_len.value].tobytes(), blen[: got.value].tolist()

    def compress_frames(self, inputs, block_size_id=4, flags=0, accel=1, cap=None):
        """Many inputs in host memory, one standard LZ4 frame each, in one call (mi355lz4_compress_frames).  flags:
        CFRAMES_LINKED | CFRAMES_BLOCK_CHECKSUM | CFRAMES_CONTENT_SIZE | CFRAMES_CONTENT_CHECKSUM.  Returns ([frame bytes per
        input], [frame length per input]).  cap: the output capacity; None takes the sum of cframes_bound, which never fails."""
        inputs = [bytes(a) for a in inputs]
        n = len(inputs)
        arrs = [np.frombuffer(a, dtype=np.uint8) for a in inputs]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) if a.size else None for a in arrs])
        lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
        flen = (C.c_int64 * max(n, 1))()
        out_len = C.c_size_t()
        if cap is None:
            cap = sum(cframes_bound(a.size, block_size_id, flags) for a in arrs)
        out = np.empty(max(int(cap), 1), dtype=np.uint8)
        _check(lib.mi355lz4_compress_frames(self.ctx, ptrs, lens, n, int(block_size_id), int(flags), int(accel),
                                            out.ctypes.data_as(_u8p), int(cap), C.byref(out_len), flen), "compress_frames")
        res = [int(flen[i]) for i in range(n)]
        parts, at = [], 0
        for r in res:
            parts.append(out[at: at + r].tobytes())
            at += r
        return parts, res

    def decompress_frames(self, inputs, flags=0, cap=None, raise_on_error=True):
        """Many inputs of standard LZ4 frames in host memory (each what `lz4 -d` accepts), decoded in one call
        (mi355lz4_decompress_frames).  Returns ([decoded bytes per input; b"" for a failed one], [size or MI355LZ4_FRM_E_*
        code per input]).  cap: the output capacity; None sizes it with one failed call, as the C ABI lets a caller do."""
        inputs = [bytes(a) for a in inputs]
        n = len(inputs)
        arrs = [np.frombuffer(a, dtype=np.uint8) for a in inputs]
        ptrs = (_u8p * max(n, 1))(*[a.ctypes.data_as(_u8p) if a.size else None for a in arrs])
        lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
        result = (C.c_int64 * max(n, 1))()
        out_len = C.c_size_t()
        if cap is None:
            rc = lib.mi355lz4_decompress_frames(self.ctx, ptrs, lens, n, int(flags), None, 0, C.byref(out_len), result)
            if rc != -4:
                if rc != 0 and (raise_on_error or rc != -5):
                    _check(rc, "decompress_frames")
                return [b""] * n, [int(result[i]) for i in range(n)]
            cap = int(out_len.value)
        out = np.empty(max(int(cap), 1), dtype=np.uint8)
        rc = lib.mi355lz4_decompress_frames(self.ctx, ptrs, lens, n, int(flags), out.ctypes.data_as(_u8p), int(cap),
                                            C.byref(out_len), result)
        if rc != 0 and (raise_on_error or rc != -5):
            _check(rc, "decompress_frames")
        res = [int(result[i]) for i in range(n)]
        parts, at = [], 0
        for r in res:
            parts.append(out[at: at + r].tobytes() if r >= 0 else b"")
            at += max(r, 0)
        return parts, res


class HcDict:
    """A prepared high-compression dictionary on the engine's device (mi355lz4_hcdict, about 216 KiB): the dictionary's last
    64 KiB and the image of the hash-chain encoder's tables after its inserts, for Engine.compress_hcdict_device /
    compress_hcdict -- and, beside it, the wave encoder's table after the dictionary's seed steps, for level 0
    (Engine.compress_fastdict_device / compress_fastdict).  Holds the empty dictionary until load()."""

    IMAGE_BYTES = 221248        # kernels.h, HCDICT_IMAGE_BYTES: u16 chain[65536], u32 head[6144], 64 bytes of count, 65536 bytes
    FAST_IMAGE_BYTES = 10256    # kernels.h, FASTDICT_IMAGE_BYTES: u16 positions[4096], 2048 bytes of tags, u32 {keep, first seam step, -, -}

    def __init__(self, engine):
        self._h = C.c_void_p()
        self._engine = engine
        engine._follow_torch()
        _check(lib.mi355lz4_hcdict_create(engine.ctx, C.byref(self._h)), "hcdict_create")

    def __len__(self):
        return int(lib.mi355lz4_hcdict_size(self._h))

    def load(self, dict_device, length=None):
        """Build the image from dict_device[:length] (a uint8 device tensor; length defaults to all of it; the last 64 KiB
        count, 0 is legal).  Enqueued; the object keeps its own copy.  Replaces what was loaded before."""
        self._engine._follow_torch()
        n = int(dict_device.numel() if length is None else length) if dict_device is not None else 0
        _check(lib.mi355lz4_hcdict_load(self._engine.ctx, self._h, _dptr(dict_device) if n else None, n), "hcdict_load")

    def image(self):
        """Diagnostics: all IMAGE_BYTES of the device image (chain, head, count, bytes), after the device is idle."""
        buf = np.empty(self.IMAGE_BYTES, dtype=np.uint8)
        _check(lib.mi355lz4_debug_hcdict_image(self._h, buf.ctypes.data_as(_u8p)), "debug_hcdict_image")
        return buf.tobytes()

    def fast_image(self):
        """Diagnostics: all FAST_IMAGE_BYTES of the wave encoder's image (positions, tags, header), after the device is idle."""
        buf = np.empty(self.FAST_IMAGE_BYTES, dtype=np.uint8)
        _check(lib.mi355lz4_debug_hcdict_fast_image(self._h, buf.ctypes.data_as(_u8p)), "debug_hcdict_fast_image")
        return buf.tobytes()

    def close(self):
        if self._h:
            lib.mi355lz4_hcdict_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DictSet:
    """A set of prepared dictionaries on the engine's device (mi355lz4_dictset): a table of the members' images, for
    Engine.compress_fastdict_multi_device / compress_fastdict_multi and Engine.decompress_dict_multi_device /
    decompress_dict_multi, where every block names its member.  The members (HcDict objects; the same one may stand at several
    indices) are borrowed by the C object; this class keeps them alive.  HcDict.load on a member is seen without a new set."""

    BLK_E_DICT = -0x7F000006    # include/mi355lz4.h, MI355LZ4_BLK_E_DICT

    def __init__(self, engine, members):
        self._h = C.c_void_p()
        self._engine = engine
        self._members = list(members)
        engine._follow_torch()
        n = len(self._members)
        arr = (C.c_void_p * max(n, 1))(*[m._h if m is not None else None for m in self._members])
        _check(lib.mi355lz4_dictset_create(engine.ctx, arr, n, C.byref(self._h)), "dictset_create")

    def __len__(self):
        return int(lib.mi355lz4_dictset_count(self._h))

    def members(self):
        return list(self._members)

    def last(self):
        """Diagnostics: (stagings, grid) of the last compress_fastdict_multi_device call that read the set, after the device is idle."""
        out = (C.c_int * 2)()
        _check(lib.mi355lz4_debug_dictset_last(self._h, out), "debug_dictset_last")
        return int(out[0]), int(out[1])

    def close(self):
        if self._h:
            lib.mi355lz4_dictset_destroy(self._h)
            self._h = C.c_void_p()
        self._members = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CompressStreams:
    """A set of n_slots device-resident reference-exact compress streams (mi355lz4_cstreams, about 80 KiB a slot), for
    Engine.compress_streams / compress_streams_device.  Bound to the engine's device; every slot starts reset."""

    def __init__(self, engine, n_slots):
        self._h = C.c_void_p()
        self._engine = engine
        engine._follow_torch()
        _check(lib.mi355lz4_cstreams_create(engine.ctx, int(n_slots), C.byref(self._h)), "cstreams_create")

    def __len__(self):
        return int(lib.mi355lz4_cstreams_count(self._h))

    def reset(self, slots=None):
        """LZ4_resetStream for the listed slots (None: all), enqueued on the engine's stream."""
        self._engine._follow_torch()
        if slots is None:
            _check(lib.mi355lz4_cstreams_reset(self._engine.ctx, self._h, None, 0), "cstreams_reset")
        else:
            a = np.ascontiguousarray(slots, dtype=np.int32)
            _check(lib.mi355lz4_cstreams_reset(self._engine.ctx, self._h, a.ctypes.data_as(_i32p), int(a.size)),
                   "cstreams_reset")

    def load_dict(self, slot, dict_device, length=None):
        """LZ4_loadDict on a slot: table, currentOffset 65536 and the last 64 KiB of dict_device[:length] (a uint8 device
        tensor; length defaults to all of it; under 8 bytes: no dictionary).  Enqueued; the slot keeps its own copy.  The
        slot then serves Engine.compress_dict_device / compress_dict, or continues through compress_streams_device."""
        self._engine._follow_torch()
        n = int(dict_device.numel() if length is None else length) if dict_device is not None else 0
        _check(lib.mi355lz4_cstreams_load_dict(self._engine.ctx, self._h, int(slot), _dptr(dict_device) if n else None, n),
               "cstreams_load_dict")

    def state(self, slot, set_current_offset=None):
        """Diagnostics: (currentOffset, dictSize, saved dictionary bytes) of a slot, after the device is idle; with
        set_current_offset the slot's currentOffset is then overwritten."""
        got = (C.c_uint32 * 3)()
        new = None if set_current_offset is None else C.byref(C.c_uint32(int(set_current_offset)))
        _check(lib.mi355lz4_debug_cstream_state(self._h, int(slot), got, new), "debug_cstream_state")
        return tuple(int(v) for v in got)

    SLOT_BYTES = 81984          # kernels.h, CSTREAM_SLOT_BYTES: uint32 table[4096], 64 bytes of scalars, 65536 saved bytes

    def slot_bytes(self, slot):
        """Diagnostics: all SLOT_BYTES of a slot (table, scalars, saved dictionary bytes), after the device is idle."""
        buf = np.empty(self.SLOT_BYTES, dtype=np.uint8)
        _check(lib.mi355lz4_debug_cstream_slot(self._h, int(slot), buf.ctypes.data_as(_u8p)), "debug_cstream_slot")
        return buf.tobytes()

    def close(self):
        if self._h:
            lib.mi355lz4_cstreams_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FastCompressStreams:
    """A set of n_slots device-resident fast linked compress streams (mi355lz4_fstreams, about 64 KiB a slot: the last
    block's last 64 KiB and their count), for Engine.compress_streams_fast / compress_streams_fast_device.  Bound to the
    engine's device; every slot starts reset."""

    def __init__(self, engine, n_slots):
        self._h = C.c_void_p()
        self._engine = engine
        engine._follow_torch()
        _check(lib.mi355lz4_fstreams_create(engine.ctx, int(n_slots), C.byref(self._h)), "fstreams_create")

    def __len__(self):
        return int(lib.mi355lz4_fstreams_count(self._h))

    def reset(self, slots=None):
        """Forget the listed slots' dictionaries (None: all), enqueued on the engine's stream."""
        self._engine._follow_torch()
        if slots is None:
            _check(lib.mi355lz4_fstreams_reset(self._engine.ctx, self._h, None, 0), "fstreams_reset")
        else:
            a = np.ascontiguousarray(slots, dtype=np.int32)
            _check(lib.mi355lz4_fstreams_reset(self._engine.ctx, self._h, a.ctypes.data_as(_i32p), int(a.size)),
                   "fstreams_reset")

    def set_dict(self, slot, dict_device, length=None):
        """The slot's state becomes the last 64 KiB of dict_device[:length] (a uint8 device tensor; length defaults to all of
        it, 0 equals a reset).  Enqueued; the slot keeps its own copy."""
        self._engine._follow_torch()
        n = int(dict_device.numel() if length is None else length) if dict_device is not None else 0
        _check(lib.mi355lz4_fstreams_set_dict(self._engine.ctx, self._h, int(slot), _dptr(dict_device) if n else None, n),
               "fstreams_set_dict")

    def set_level(self, level):
        """The set's compression level for the calls made after this one (mi355lz4_fstreams_set_level): 0 the wave encoder
        (default), 1..12 the hash-chain encoder.  A host-side attribute: nothing is enqueued."""
        _check(lib.mi355lz4_fstreams_set_level(self._h, int(level)), "fstreams_set_level")

    @property
    def level(self):
        r = int(lib.mi355lz4_fstreams_get_level(self._h))
        _check(min(r, 0), "fstreams_get_level")
        return r

    def peek(self, slot):
        """Diagnostics: (dictionary bytes held, those bytes), after the device is idle."""
        cnt = C.c_int()
        buf = np.empty(65536, dtype=np.uint8)
        _check(lib.mi355lz4_debug_fstreams_peek(self._h, int(slot), buf.ctypes.data_as(_u8p), C.byref(cnt)),
               "debug_fstreams_peek")
        return int(cnt.value), buf[: max(0, min(int(cnt.value), 65536))].tobytes()

    def close(self):
        if self._h:
            lib.mi355lz4_fstreams_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecompressStreams:
    """A set of n_slots device-resident linked decode streams (mi355lz4_dstreams, about 64 KiB a slot), for
    Engine.decompress_dstreams / decompress_dstreams_device.  Bound to the engine's device; every slot starts reset."""

    def __init__(self, engine, n_slots):
        self._h = C.c_void_p()
        self._engine = engine
        engine._follow_torch()
        _check(lib.mi355lz4_dstreams_create(engine.ctx, int(n_slots), C.byref(self._h)), "dstreams_create")

    def __len__(self):
        return int(lib.mi355lz4_dstreams_count(self._h))

    def reset(self, slots=None):
        """Forget the listed slots' dictionaries (None: all), enqueued on the engine's stream."""
        self._engine._follow_torch()
        if slots is None:
            _check(lib.mi355lz4_dstreams_reset(self._engine.ctx, self._h, None, 0), "dstreams_reset")
        else:
            a = np.ascontiguousarray(slots, dtype=np.int32)
            _check(lib.mi355lz4_dstreams_reset(self._engine.ctx, self._h, a.ctypes.data_as(_i32p), int(a.size)),
                   "dstreams_reset")

    def set_dict(self, slot, dict_device, length=None):
        """LZ4_setStreamDecode: the slot's state becomes the last 64 KiB of dict_device[:length] (a uint8 device tensor;
        length defaults to all of it, 0 equals a reset).  Enqueued; the slot keeps its own copy."""
        self._engine._follow_torch()
        n = int(dict_device.numel() if length is None else length) if dict_device is not None else 0
        _check(lib.mi355lz4_dstreams_set_dict(self._engine.ctx, self._h, int(slot), _dptr(dict_device) if n else None, n),
               "dstreams_set_dict")

    def state(self, slot, set_bytes=None):
        """Diagnostics: (dictionary bytes held, the slot's whole 64 KiB area as bytes), after the device is idle; with
        set_bytes (65536 bytes) the area is then overwritten, the count stays."""
        cnt = C.c_uint32()
        buf = np.empty(65536, dtype=np.uint8)
        new = None
        if set_bytes is not None:
            new = np.frombuffer(bytes(set_bytes), dtype=np.uint8)
            if new.size != 65536:
                raise ValueError("set_bytes must be 65536 bytes")
        _check(lib.mi355lz4_debug_dstream_state(self._h, int(slot), C.byref(cnt), buf.ctypes.data_as(_u8p),
                                                new.ctypes.data_as(_u8p) if new is not None else None), "debug_dstream_state")
        return int(cnt.value), buf.tobytes()

    def close(self):
        if self._h:
            lib.mi355lz4_dstreams_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


FRAMES_SKIP_CONTENT_CHECKSUM = 1
FRAMES_SKIP_BLOCK_CHECKSUM = 2
FRM_E_MAGIC, FRM_E_HEADER, FRM_E_HEADER_CHECKSUM, FRM_E_TRUNCATED, FRM_E_BLOCK_SIZE, FRM_E_BLOCK_CHECKSUM, FRM_E_BLOCK, \
    FRM_E_CONTENT_SIZE, FRM_E_CONTENT_CHECKSUM = [-0x7F000100 - k for k in range(1, 10)]


class Frames:
    """A parsed batch of standard LZ4 frames on the engine's device (mi355lz4_frames).  load() parses many inputs and
    reports their exact decoded sizes (it waits for the engine's stream); decode() decodes them all and only enqueues."""

    def __init__(self, engine):
        self._h = C.c_void_p()
        self._engine = engine
        self._buf = None
        _check(lib.mi355lz4_frames_create(engine.ctx, C.byref(self._h)), "frames_create")

    def load(self, buf, in_off, in_len, n_inputs=None, flags=0, buf_len=None):
        """buf: uint8 device tensor (borrowed until the decodes have run); in_off, in_len: uint64-valued int64 device
        tensors; input i is buf[in_off[i] : in_off[i] + in_len[i]].  Returns the sizes (list of ints: size or code)."""
        self._engine._follow_torch()
        n = int(in_off.numel() if n_inputs is None else n_inputs)
        blen = int(buf.numel() if buf_len is None else buf_len) if buf is not None else 0
        _check(lib.mi355lz4_frames_load(self._engine.ctx, self._h, _dptr(buf), blen, _dptr(in_off), _dptr(in_len), n,
                                        int(flags)), "frames_load")
        self._buf = buf
        return self.sizes()

    def sizes(self):
        n = int(lib.mi355lz4_frames_inputs(self._h))
        if n < 0:
            raise LZ4Error("frames_inputs failed: %s" % _err())
        a = (C.c_int64 * max(n, 1))()
        _check(lib.mi355lz4_frames_get_sizes(self._h, a), "frames_get_sizes")
        return [int(a[i]) for i in range(n)]

    def sizes_device_ptr(self):
        return lib.mi355lz4_frames_sizes(self._h)

    def total(self):
        return int(lib.mi355lz4_frames_total(self._h))

    def blocks(self):
        n = int(lib.mi355lz4_frames_blocks(self._h))
        if n < 0:
            raise LZ4Error("frames_blocks failed: %s" % _err())
        return n

    def decode(self, out, out_off, result):
        """out: uint8 device tensor; out_off: int64 device tensor (uint64 values); result: int64 device tensor.  Enqueued."""
        self._engine._follow_torch()
        _check(lib.mi355lz4_frames_decode(self._engine.ctx, self._h, _dptr(out), _dptr(out_off), _dptr(result)),
               "frames_decode")

    def close(self):
        if self._h:
            lib.mi355lz4_frames_destroy(self._h)
            self._h = C.c_void_p()
        self._buf = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


CFRAMES_LINKED, CFRAMES_BLOCK_CHECKSUM, CFRAMES_CONTENT_SIZE, CFRAMES_CONTENT_CHECKSUM = 1, 2, 4, 8
FRW_E_CAPACITY, FRW_E_INPUT = -0x7F000201, -0x7F000202


def cframes_bound(n, block_size_id=4, flags=0):
    """The exact worst case of one frame of n input bytes (mi355lz4_cframes_bound); 0 for a bad block size id or flag."""
    return int(lib.mi355lz4_cframes_bound(int(n), int(block_size_id), int(flags)))


class FrameWriter:
    """A frame writer on the engine's device (mi355lz4_cframes): the block table and the slots of its calls.  compress() turns
    many device-resident inputs into one standard LZ4 frame each and only enqueues once the scratch is there (reserve())."""

    def __init__(self, engine):
        self._h = C.c_void_p()
        self._engine = engine
        _check(lib.mi355lz4_cframes_create(engine.ctx, C.byref(self._h)), "cframes_create")

    def reserve(self, n_inputs, max_input_len, total_len, block_size_id=4):
        """Size the scratch for calls of at most this shape (either linked setting) ahead of time."""
        _check(lib.mi355lz4_cframes_reserve(self._engine.ctx, self._h, int(n_inputs), int(max_input_len), int(total_len),
                                            int(block_size_id)), "cframes_reserve")

    def compress(self, src, in_off, in_len, max_input_len, total_len, dst, dst_off, dst_cap, frame_len, block_size_id=4, flags=0,
                 accel=1, n_inputs=None, src_len=None):
        """src, dst: uint8 device tensors; in_off, in_len, dst_off, dst_cap: uint64-valued int64 device tensors; frame_len:
        int64 device tensor (a length or FRW_E_* per input).  max_input_len, total_len: host-side bounds of in_len and of
        its sum.  Enqueued on the engine's stream."""
        self._engine._follow_torch()
        n = int(in_off.numel() if n_inputs is None else n_inputs)
        slen = int(src.numel() if src_len is None else src_len) if src is not None else 0
        _check(lib.mi355lz4_cframes_compress(self._engine.ctx, self._h, _dptr(src), slen, _dptr(in_off), _dptr(in_len), n,
                                             int(max_input_len), int(total_len), int(block_size_id), int(flags), int(accel),
                                             _dptr(dst), _dptr(dst_off), _dptr(dst_cap), _dptr(frame_len)), "cframes_compress")

    def close(self):
        if self._h:
            lib.mi355lz4_cframes_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------
# Stream-combinator mirror (lists / iterables of bytes in, list of bytes out)
# ---------------------------------------------------------------------------
def _pack(arrays):
    arrays = [bytes(a) for a in arrays]
    data = np.frombuffer(b"".join(arrays), dtype=np.uint8) if arrays else np.zeros(0, dtype=np.uint8)
    if data.size == 0:
        data = np.zeros(1, dtype=np.uint8)
    lens = np.array([len(a) for a in arrays] + [0], dtype=np.uint64)
    return data, lens, len(arrays)


class _ArraysOwner:
    """Keeps a C-side result alive while Python slices of it are in use."""
    def __init__(self, h):
        self.h = h

    def __del__(self):
        if self.h and lib is not None:                 # (module globals are gone at interpreter shutdown)
            lib.slz4_arrays_free(self.h)
            self.h = None


def _unpack_views(h):
    """The result arrays as memoryviews INTO the C-side buffer (no copy): what a Haskell `Array` is -- a slice of a
    shared buffer.  The buffer lives as long as any of the views."""
    owner = _ArraysOwner(h)
    n = lib.slz4_arrays_count(h)
    base, offs = _u8p(), C.POINTER(C.c_size_t)()
    if n and lib.slz4_arrays_flat(h, C.byref(base), C.byref(offs)):
        # one buffer: one ctypes object, the arrays are slices of its memoryview
        total = offs[n]
        if total == 0:
            return [memoryview(b"")] * n
        arr = (C.c_uint8 * total).from_address(C.cast(base, C.c_void_p).value)
        arr._owner = owner
        mv = memoryview(arr).cast("B")
        o = offs[0:n + 1]
        return [mv[o[i]:o[i + 1]] for i in range(n)]
    out = []
    for i in range(n):
        ln = lib.slz4_arrays_len(h, i)
        if ln:
            arr = (C.c_uint8 * ln).from_address(C.cast(lib.slz4_arrays_data(h, i), C.c_void_p).value)
            arr._owner = owner
            out.append(memoryview(arr).cast("B"))
        else:
            out.append(memoryview(b""))
    return out


def _unpack(h):
    try:
        n = lib.slz4_arrays_count(h)
        out = []
        for i in range(n):
            ln = lib.slz4_arrays_len(h, i)
            out.append(C.string_at(lib.slz4_arrays_data(h, i), ln) if ln else b"")
        return out
    finally:
        lib.slz4_arrays_free(h)


def _run(fn, *args, views=False):
    h = C.c_void_p()
    rc = fn(*args, C.byref(h))
    if rc != 0:
        raise LZ4Error((lib.slz4_last_error() or b"").decode("utf-8", "replace"))
    return _unpack_views(h) if views else _unpack(h)


def compressChunks(cfg, speed, arrays, engine):
    """Streamly.LZ4.compressChunks (reference src/Streamly/LZ4.hs:94-100)."""
    data, lens, n = _pack(arrays)
    return _run(lib.slz4_compress_chunks, engine._h, cfg._kind, int(speed), data.ctypes.data_as(_u8p),
                lens.ctypes.data_as(_u64p), n)


def resizeChunks(cfg, conf, arrays):
    """Streamly.Internal.LZ4.resizeChunksD (reference src/Streamly/Internal/LZ4.hs:432-523).  Host only."""
    data, lens, n = _pack(arrays)
    return _run(lib.slz4_resize_chunks, cfg._kind, int(conf.hasEndMark), data.ctypes.data_as(_u8p),
                lens.ctypes.data_as(_u64p), n)


def decompressChunksRaw(cfg, arrays, engine):
    """Streamly.Internal.LZ4.decompressChunksRawD (reference src/Streamly/Internal/LZ4.hs:539-567)."""
    data, lens, n = _pack(arrays)
    return _run(lib.slz4_decompress_chunks_raw, engine._h, cfg._kind, data.ctypes.data_as(_u8p),
                lens.ctypes.data_as(_u64p), n)


def decompressChunks(cfg, arrays, engine, conf=defaultFrameConfig, views=False):
    """Streamly.LZ4.decompressChunks (reference src/Streamly/LZ4.hs:114-122); conf selects the end-mark variant.
    views=True returns the arrays as memoryviews into one result buffer (the reference's arrays are such slices) instead
    of one bytes object -- one copy -- per array."""
    data, lens, n = _pack(arrays)
    return _run(lib.slz4_decompress_chunks, engine._h, cfg._kind, int(conf.hasEndMark), data.ctypes.data_as(_u8p),
                lens.ctypes.data_as(_u64p), n, views=views)


def decompressChunksStream(cfg, arrays, engine, conf=defaultFrameConfig):
    """decompressChunks array at a time, as a consumer of the stream sees it: returns (the arrays delivered, None), or
    (the arrays delivered before the stream raised, the LZ4Error it raised)."""
    data, lens, n = _pack(arrays)
    h = C.c_void_p()
    rc = lib.slz4_decompress_chunks_stream(engine._h, cfg._kind, int(conf.hasEndMark), data.ctypes.data_as(_u8p),
                                           lens.ctypes.data_as(_u64p), n, C.byref(h))
    err = LZ4Error((lib.slz4_last_error() or b"").decode("utf-8", "replace")) if rc != 0 else None
    return _unpack(h), err


def decompressChunksWith(arrays, engine):
    """decompressChunksWithD simpleFrameParserD (reference src/Streamly/Internal/LZ4.hs:569-577)."""
    data, lens, n = _pack(arrays)
    return _run(lib.slz4_decompress_chunks_with, engine._h, data.ctypes.data_as(_u8p), lens.ctypes.data_as(_u64p), n)


def simpleFrameParser(arrays):
    """simpleFrameParserD (reference src/Streamly/Internal/LZ4.hs:590-651).  Returns ((BlockConfig, FrameConfig), rest)."""
    data, lens, n = _pack(arrays)
    h = C.c_void_p()
    em = C.c_int()
    kind = lib.slz4_simple_frame_parser(data.ctypes.data_as(_u8p), lens.ctypes.data_as(_u64p), n, C.byref(em), C.byref(h))
    if kind < 0:
        raise LZ4Error((lib.slz4_last_error() or b"").decode("utf-8", "replace"))
    return (BlockConfig(kind), FrameConfig(bool(em.value))), _unpack(h)


# ---- the standard LZ4 frame format (csrc/lz4_frame.cpp): interop with liblz4's LZ4F_* and the lz4 CLI ----
def _bytes_arg(data):
    a = np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
    if a.size == 0:
        return np.zeros(1, dtype=np.uint8), 0
    return a, int(a.size)


def xxh32(data, seed=0):
    """xxHash32, the checksum of the LZ4 frame format (host code, no GPU)."""
    a, n = _bytes_arg(data)
    return int(lib.slz4_xxh32(a.ctypes.data_as(_u8p), n, int(seed)))


def lz4FrameCompress(data, engine, speed=1, blockMax=BlockSize.BlockMax64KB, blockChecksum=False, contentChecksum=True,
                     contentSize=False, linkedBlocks=False):
    """One standard LZ4 frame (independent blocks, or linked ones: smaller on text) -- readable by LZ4F_decompress / `lz4 -d`.  The reference's
    own frame support stops at parsing a header without these options (src/Streamly/Internal/LZ4.hs:631-638)."""
    a, n = _bytes_arg(data)
    flags = (1 if blockChecksum else 0) | (2 if contentChecksum else 0) | (4 if contentSize else 0) | (8 if linkedBlocks else 0)
    return _run(lib.slz4_lz4frame_compress, engine._h, int(blockMax), flags, int(speed), a.ctypes.data_as(_u8p), n)[0]


def lz4FrameDecompress(frame, engine):
    """Decode any sequence of standard LZ4 frames (linked or independent blocks, stored blocks, checksums verified)."""
    a, n = _bytes_arg(frame)
    return _run(lib.slz4_lz4frame_decompress, engine._h, a.ctypes.data_as(_u8p), n)[0]
