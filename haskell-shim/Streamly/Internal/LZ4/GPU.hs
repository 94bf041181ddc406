{-# LANGUAGE NamedFieldPuns #-}
{-# LANGUAGE ForeignFunctionInterface #-}
-- |
-- Module      : Streamly.Internal.LZ4.GPU
--
-- Batched MI355X replacements for the two per-block primitives of
-- "Streamly.Internal.LZ4" (@compressChunk@ / @decompressChunk@) and for the two
-- combinators that call them once per array (@compressChunksD@,
-- @decompressChunksRawD@).  Everything else of the package (resizeChunksD, the
-- frame parser, Streamly.LZ4) is used unchanged.
--
-- UNTESTED SOURCE: GHC, cabal and streamly-0.8.2 are not available in the build
-- image of this repository, so this module has not been compiled.  The C++ mirror
-- (include/streamly_lz4.hpp, streamly-lz4_amd/csrc/host_stream.cpp) implements the
-- same restructuring and is what the test-suite exercises.  Link with
--
-- >   include-dirs:    <repo>/include
-- >   extra-lib-dirs:  <repo>/streamly-lz4_amd/lib
-- >   extra-libraries: mi355lz4
--
-- Design: the incoming @Array Word8@ stream is grouped into batches of up to
-- 'batchBlocks' arrays; one @ccall safe@ hands a batch to the GPU (a GPU round trip must
-- not block a capability the way the reference's @ccall unsafe@ per-block calls may).
-- Compressed blocks are INDEPENDENT by default, so no previous input has to be kept alive
-- ('setLinkedCompress' makes the blocks of one batch a linked stream like the reference's:
-- a batch is handed over as a whole, so its arrays are alive for the duration of the call);
-- decompression keeps the previous OUTPUT array alive exactly like the reference
-- (it is the dictionary of the next block of a linked stream).
module Streamly.Internal.LZ4.GPU
    ( Engine
    , newEngine
    , freeEngine
    , setLinkedCompress
    , setBlockChecksum
    , setCompressionLevel
    , setCompressExact
    , resetCompressStream
    , c_decodedSizeDevice
    , decodedSizes
    , c_decompressPartialDevice
    , decompressChunksPrefix
    , CompressStreams
    , newCompressStreams
    , freeCompressStreams
    , resetCompressStreams
    , c_compressStreamsDevice
    , compressChunksMany
    , c_cstreamsLoadDict
    , c_compressDictDevice
    , c_decompressDictDevice
    , loadDict
    , compressChunksWithDict
    , decompressChunksWithDict
    , HcDict
    , newHcDict
    , freeHcDict
    , loadHcDict
    , hcDictSize
    , c_compressHcDictDevice
    , compressChunksWithDictHC
    , c_compressFastDictDevice
    , compressChunksWithDictFast
    , DictSet
    , newDictSet
    , freeDictSet
    , dictSetCount
    , c_compressFastDictMultiDevice
    , c_decompressDictMultiDevice
    , compressChunksWithDictsFast
    , decompressChunksWithDicts
    , c_compressPagesDevice
    , compressChunksPaged
    , c_compressPagesFastDevice
    , compressChunksPagedFast
    , c_compressPagesFastDictDevice
    , compressChunksPagedWithDictFast
    , FastStreams
    , newFastStreams
    , freeFastStreams
    , resetFastStreams
    , fastStreamsSetDict
    , setFastStreamsLevel
    , fastStreamsLevel
    , c_compressStreamsFastDevice
    , compressChunksManyFast
    , DecompressStreams
    , newDecompressStreams
    , freeDecompressStreams
    , resetDecompressStreams
    , c_dstreamsSetDict
    , c_decompressDStreamsDevice
    , decompressChunksMany
    , Frames
    , newFrames
    , freeFrames
    , loadFrames
    , decodeFrames
    , decompressFramesMany
    , FrameWriter
    , newFrameWriter
    , freeFrameWriter
    , frameBound
    , reserveFrameWriter
    , compressFramesDevice
    , compressFramesMany
    , MultiEngine
    , newMultiEngine
    , freeMultiEngine
    , c_multiCompressBatch
    , c_multiDecompressBatch
    , compressChunksGPU
    , decompressChunksRawGPU
    )
where

import Control.Monad (forM, forM_, when)
import Control.Monad.IO.Class (MonadIO(..))
import Data.Int (Int32, Int64)
import Data.Word (Word8, Word64)
import Foreign.C (CInt(..), CSize(..), CUInt(..))
import Foreign.Marshal.Alloc (alloca)
import Foreign.Marshal.Array (allocaArray, peekArray, pokeArray, withArrayLen)
import Foreign.Marshal.Utils (copyBytes)
import Foreign.Ptr (Ptr, nullPtr, plusPtr, castPtr)
import Foreign.Storable (peek)

import qualified Streamly.Internal.Data.Array.Foreign as Array
import qualified Streamly.Internal.Data.Array.Foreign.Type as Array
import qualified Streamly.Internal.Data.Array.Foreign.Mut.Type as MArray
import qualified Streamly.Internal.Data.Fold as Fold
import qualified Streamly.Internal.Data.Stream.StreamD as Stream

import Streamly.Internal.LZ4.Config

data C_Engine
newtype Engine = Engine (Ptr C_Engine)

foreign import ccall safe "mi355lz4.h mi355lz4_create"
    c_create :: Ptr (Ptr C_Engine) -> CInt -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_destroy"
    c_destroy :: Ptr C_Engine -> IO ()
foreign import ccall unsafe "mi355lz4.h mi355lz4_compress_bound"
    c_bound :: CInt -> CInt
-- small calls: segments per block (-1 automatic, 0 off, 2..64); include/mi355lz4.h
foreign import ccall unsafe "mi355lz4.h mi355lz4_set_segments"
    c_setSegments :: Ptr C_Engine -> CInt -> IO CInt

-- linked device decodes without a host wait (0 = default: wait); include/mi355lz4.h
foreign import ccall unsafe "mi355lz4.h mi355lz4_set_linked_async"
    c_setLinkedAsync :: Ptr C_Engine -> CInt -> IO CInt

foreign import ccall unsafe "mi355lz4.h mi355lz4_set_linked_compress"
    c_setLinkedCompress :: Ptr C_Engine -> CInt -> IO CInt

-- replaces c_compressFastContinue (Streamly/Internal/LZ4.hs:123-131), N blocks per call
foreign import ccall unsafe "mi355lz4.h mi355lz4_set_block_checksum"
    c_setBlockChecksum :: Ptr C_Engine -> CInt -> IO CInt

foreign import ccall unsafe "mi355lz4.h mi355lz4_set_compression_level"
    c_setCompressionLevel :: Ptr C_Engine -> CInt -> IO CInt

foreign import ccall unsafe "mi355lz4.h mi355lz4_set_compress_exact"
    c_setCompressExact :: Ptr C_Engine -> CInt -> IO CInt

foreign import ccall unsafe "mi355lz4.h mi355lz4_compress_exact_reset"
    c_compressExactReset :: Ptr C_Engine -> IO CInt

foreign import ccall unsafe "mi355lz4.h mi355lz4_get_compress_exact"
    c_getCompressExact :: Ptr C_Engine -> IO CInt

foreign import ccall safe "mi355lz4.h mi355lz4_compress_batch"
    c_compressBatch
        :: Ptr C_Engine -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> Ptr Int32 -> IO CInt

-- Many reference-exact compress streams in ONE call (include/mi355lz4.h, "many reference-exact streams in one call"): a set
-- of device-resident @LZ4_stream_t@s, one slot per pipeline; stream s of a call = blocks [streamFirst[s], streamFirst[s+1]),
-- continuing slot streamSlot[s].  One FFI call for the next arrays of all pipelines instead of one engine per pipeline.
data C_CStreams
newtype CompressStreams = CompressStreams (Ptr C_CStreams)

foreign import ccall safe "mi355lz4.h mi355lz4_cstreams_create"
    c_cstreamsCreate :: Ptr C_Engine -> CInt -> Ptr (Ptr C_CStreams) -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_cstreams_destroy"
    c_cstreamsDestroy :: Ptr C_CStreams -> IO ()
foreign import ccall unsafe "mi355lz4.h mi355lz4_cstreams_count"
    c_cstreamsCount :: Ptr C_CStreams -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_cstreams_reset"
    c_cstreamsReset :: Ptr C_Engine -> Ptr C_CStreams -> Ptr Int32 -> CInt -> IO CInt
-- device pointers in, device pointers out; only enqueues
foreign import ccall safe "mi355lz4.h mi355lz4_compress_streams_device"
    c_compressStreamsDevice
        :: Ptr C_Engine -> Ptr C_CStreams -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> Word64 -> CInt -> CInt
        -> Ptr Int32 -> Ptr Int32 -> CInt -> CInt -> CInt -> Ptr Word8 -> CSize -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_streams"
    c_compressStreams
        :: Ptr C_Engine -> Ptr C_CStreams -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> Ptr Int32 -> Ptr Int32 -> CInt
        -> CInt -> CInt -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> Ptr Int32 -> IO CInt

-- Shared-dictionary batches (include/mi355lz4.h, "shared-dictionary batches"): LZ4_loadDict on one slot of the set, a batch of
-- independent blocks compressed from a copy of that slot each (the slot is only read), and LZ4_decompress_safe_usingDict for a
-- batch against one dictionary.  The _device forms take device pointers and only enqueue.
foreign import ccall safe "mi355lz4.h mi355lz4_cstreams_load_dict"
    c_cstreamsLoadDict :: Ptr C_Engine -> Ptr C_CStreams -> CInt -> Ptr Word8 -> CInt -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_dict_device"
    c_compressDictDevice
        :: Ptr C_Engine -> Ptr C_CStreams -> CInt -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> Word64 -> CInt -> CInt
        -> CInt -> CInt -> Ptr Word8 -> CSize -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_dict_device"
    c_decompressDictDevice
        :: Ptr C_Engine -> Ptr Word8 -> Word64 -> Ptr Word64 -> CInt -> CInt -> CInt -> Ptr Word8 -> CInt
        -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_dict"
    c_compressDict
        :: Ptr C_Engine -> Ptr C_CStreams -> CInt -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_dict"
    c_decompressDict
        :: Ptr C_Engine -> Ptr Word8 -> CSize -> CInt -> CInt -> Ptr Word8 -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> CInt -> Ptr CInt -> IO CInt

-- High-compression levels against a shared dictionary (include/mi355lz4.h, "high-compression levels against a shared
-- dictionary"): a prepared dictionary on the device -- its last 64 KiB and the image of the hash-chain encoder's tables -- and a
-- batch of independent blocks compressed at the engine's level 1..12 with it in front of each (the object is only read).
data C_HcDict
newtype HcDict = HcDict (Ptr C_HcDict)

foreign import ccall safe "mi355lz4.h mi355lz4_hcdict_create"
    c_hcdictCreate :: Ptr C_Engine -> Ptr (Ptr C_HcDict) -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_hcdict_destroy"
    c_hcdictDestroy :: Ptr C_HcDict -> IO ()
foreign import ccall safe "mi355lz4.h mi355lz4_hcdict_load"
    c_hcdictLoad :: Ptr C_Engine -> Ptr C_HcDict -> Ptr Word8 -> CInt -> IO CInt
foreign import ccall unsafe "mi355lz4.h mi355lz4_hcdict_size"
    c_hcdictSize :: Ptr C_HcDict -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_hcdict_device"
    c_compressHcDictDevice
        :: Ptr C_Engine -> Ptr C_HcDict -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> Word64 -> CInt -> CInt
        -> CInt -> Ptr Word8 -> CSize -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_hcdict"
    c_compressHcDict
        :: Ptr C_Engine -> Ptr C_HcDict -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> Ptr Int32 -> IO CInt
-- ... and level 0 against the same object, by the wave encoder (accel in front of headerKind)
foreign import ccall safe "mi355lz4.h mi355lz4_compress_fastdict_device"
    c_compressFastDictDevice
        :: Ptr C_Engine -> Ptr C_HcDict -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> Word64 -> CInt -> CInt
        -> CInt -> CInt -> Ptr Word8 -> CSize -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_fastdict"
    c_compressFastDict
        :: Ptr C_Engine -> Ptr C_HcDict -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> Ptr Int32 -> IO CInt

-- Dictionary sets (include/mi355lz4.h, "dictionary sets"): a table of prepared dictionaries on the device and, per block, an index
-- into it (-1: none).  The members are borrowed: they must outlive the set.  ds and dictIdx stand where the single-dictionary
-- calls have their dictionary.
data C_DictSet
newtype DictSet = DictSet (Ptr C_DictSet)

foreign import ccall safe "mi355lz4.h mi355lz4_dictset_create"
    c_dictsetCreate :: Ptr C_Engine -> Ptr (Ptr C_HcDict) -> CInt -> Ptr (Ptr C_DictSet) -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_dictset_destroy"
    c_dictsetDestroy :: Ptr C_DictSet -> IO ()
foreign import ccall unsafe "mi355lz4.h mi355lz4_dictset_count"
    c_dictsetCount :: Ptr C_DictSet -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_fastdict_multi_device"
    c_compressFastDictMultiDevice
        :: Ptr C_Engine -> Ptr C_DictSet -> Ptr Int32 -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> Word64 -> CInt -> CInt
        -> CInt -> CInt -> Ptr Word8 -> CSize -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_fastdict_multi"
    c_compressFastDictMulti
        :: Ptr C_Engine -> Ptr C_DictSet -> Ptr Int32 -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_dict_multi_device"
    c_decompressDictMultiDevice
        :: Ptr C_Engine -> Ptr Word8 -> Word64 -> Ptr Word64 -> CInt -> CInt -> CInt -> Ptr C_DictSet -> Ptr Int32
        -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_dict_multi"
    c_decompressDictMulti
        :: Ptr C_Engine -> Ptr Word8 -> CSize -> CInt -> CInt -> Ptr C_DictSet -> Ptr Int32
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> CInt -> Ptr CInt -> IO CInt

-- Fixed-size output pages (LZ4_compress_destSize, N inputs per call): input i is cut into at most maxPages pages of
-- pageSize[i] compressed bytes, page (i, k) at pages + (i * maxPages + k) * pageStride behind a header of headerKind (0, 4, 8)
-- bytes.  The device form takes device pointers and only enqueues; the host form is synchronous.
foreign import ccall safe "mi355lz4.h mi355lz4_compress_pages_device"
    c_compressPagesDevice
        :: Ptr C_Engine -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> CInt -> Ptr Int32 -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_pages"
    c_compressPages
        :: Ptr C_Engine -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> IO CInt
-- The same chains by the engine's own level-0 encoder with an output budget: accel in front of headerKind.  Valid, independently
-- decodable pages at the engine's speed, not LZ4_compress_destSize's bytes.
foreign import ccall safe "mi355lz4.h mi355lz4_compress_pages_fast_device"
    c_compressPagesFastDevice
        :: Ptr C_Engine -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> CInt -> Ptr Int32 -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_pages_fast"
    c_compressPagesFast
        :: Ptr C_Engine -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> CInt -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> IO CInt
-- ... and with the dictionary of a loaded 'HcDict' in front of every page: the object in front of the inputs, the rest as above.
foreign import ccall safe "mi355lz4.h mi355lz4_compress_pages_fastdict_device"
    c_compressPagesFastDictDevice
        :: Ptr C_Engine -> Ptr C_HcDict -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> CInt -> Ptr Int32 -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_pages_fastdict"
    c_compressPagesFastDict
        :: Ptr C_Engine -> Ptr C_HcDict -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> CInt -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> IO CInt

-- Decoded sizes without decoding (device pointers in, device pointers out; only enqueues): what every block of a
-- size-less framing (BlockMax64KB .. BlockMax4MB) decodes to, read off its token chain.  size[i] >= 0, or a negative
-- per-block code (MI355LZ4_BLK_E_SIZE_UNKNOWN = -0x7F000005); outOff (may be nullPtr) = their exclusive scan.
foreign import ccall safe "mi355lz4.h mi355lz4_decoded_size_device"
    c_decodedSizeDevice
        :: Ptr C_Engine -> Ptr Word8 -> Word64 -> Ptr Word64 -> CInt -> CInt -> CInt -> Ptr Int32 -> Ptr Word64
        -> IO CInt

-- Partial decode (LZ4_decompress_safe_partial, N blocks per call): the first target[i] bytes of every block.  The device
-- form takes device pointers and only enqueues; the host form walks a framed chain in host memory and brings back the
-- prefixes alone, packed back to back.
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_partial_device"
    c_decompressPartialDevice
        :: Ptr C_Engine -> Ptr Word8 -> Word64 -> Ptr Word64 -> CInt -> CInt -> CInt
        -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> Ptr Int32 -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_partial"
    c_decompressPartial
        :: Ptr C_Engine -> Ptr Word8 -> CSize -> CInt -> CInt -> Ptr Int32 -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> CInt -> Ptr CInt -> IO CInt

-- replaces c_decompressSafeContinue (Streamly/Internal/LZ4.hs:133-140), N blocks per call
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_batch"
    c_decompressBatch
        :: Ptr C_Engine -> Ptr Word8 -> CSize -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CInt -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32
        -> CInt -> Ptr CInt -> IO CInt

-- Many linked streams (each the output of one reference compressChunks pipeline) in one call:
-- stream s = blocks [streamFirst[s], streamFirst[s+1]).  A server that decompresses many files or
-- connections at once gathers their resized blocks and calls this instead of one
-- c_decompressBatch per stream: a single linked stream is walked by one wavefront (slow), many
-- streams run side by side.
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_streams"
    c_decompressStreams
        :: Ptr C_Engine -> Ptr Word8 -> CSize -> CInt -> CInt -> Ptr Int32 -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> CInt -> Ptr CInt -> IO CInt

-- Many linked decode streams continued across calls (include/mi355lz4.h, "many linked decode streams, continued across
-- calls"): a set of device-resident @LZ4_streamDecode_t@s, one slot per pipeline -- the last block's last 64 KiB and their
-- count.  Stream s of a call = blocks [streamFirst[s], streamFirst[s+1]), continuing slot streamSlot[s]: the next blocks of
-- all pipelines in one FFI call, as they arrive, instead of one engine call per stream with a host-side dictionary.
-- Many fast linked compress streams continued across calls (include/mi355lz4.h, "many fast linked compress streams"): the wave
-- encoder's counterpart of the set above.  A slot is the last array's last 64 KiB and their count.
data C_FStreams
newtype FastStreams = FastStreams (Ptr C_FStreams)

foreign import ccall safe "mi355lz4.h mi355lz4_fstreams_create"
    c_fstreamsCreate :: Ptr C_Engine -> CInt -> Ptr (Ptr C_FStreams) -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_fstreams_destroy"
    c_fstreamsDestroy :: Ptr C_FStreams -> IO ()
foreign import ccall unsafe "mi355lz4.h mi355lz4_fstreams_count"
    c_fstreamsCount :: Ptr C_FStreams -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_fstreams_reset"
    c_fstreamsReset :: Ptr C_Engine -> Ptr C_FStreams -> Ptr Int32 -> CInt -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_fstreams_set_dict"
    c_fstreamsSetDict :: Ptr C_Engine -> Ptr C_FStreams -> CInt -> Ptr Word8 -> CInt -> IO CInt
-- the set's compression level: a host-side attribute, no device work
foreign import ccall unsafe "mi355lz4.h mi355lz4_fstreams_set_level"
    c_fstreamsSetLevel :: Ptr C_FStreams -> CInt -> IO CInt
foreign import ccall unsafe "mi355lz4.h mi355lz4_fstreams_get_level"
    c_fstreamsGetLevel :: Ptr C_FStreams -> IO CInt
-- device pointers in, device pointers out; only enqueues
foreign import ccall safe "mi355lz4.h mi355lz4_compress_streams_fast_device"
    c_compressStreamsFastDevice
        :: Ptr C_Engine -> Ptr C_FStreams -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> Word64 -> CInt -> CInt
        -> Ptr Int32 -> Ptr Int32 -> CInt -> CInt -> CInt -> Ptr Word8 -> CSize -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_streams_fast"
    c_compressStreamsFast
        :: Ptr C_Engine -> Ptr C_FStreams -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> Ptr Int32 -> Ptr Int32 -> CInt
        -> CInt -> CInt -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> Ptr Int32 -> IO CInt

data C_DStreams
newtype DecompressStreams = DecompressStreams (Ptr C_DStreams)

foreign import ccall safe "mi355lz4.h mi355lz4_dstreams_create"
    c_dstreamsCreate :: Ptr C_Engine -> CInt -> Ptr (Ptr C_DStreams) -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_dstreams_destroy"
    c_dstreamsDestroy :: Ptr C_DStreams -> IO ()
foreign import ccall unsafe "mi355lz4.h mi355lz4_dstreams_count"
    c_dstreamsCount :: Ptr C_DStreams -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_dstreams_reset"
    c_dstreamsReset :: Ptr C_Engine -> Ptr C_DStreams -> Ptr Int32 -> CInt -> IO CInt
-- LZ4_setStreamDecode: the dictionary is DEVICE memory; enqueued
foreign import ccall safe "mi355lz4.h mi355lz4_dstreams_set_dict"
    c_dstreamsSetDict :: Ptr C_Engine -> Ptr C_DStreams -> CInt -> Ptr Word8 -> CInt -> IO CInt
-- device pointers in, device pointers out; only enqueues (no host wait: per-block codes are in result[])
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_dstreams_device"
    c_decompressDStreamsDevice
        :: Ptr C_Engine -> Ptr C_DStreams -> Ptr Word8 -> Word64 -> Ptr Word64 -> CInt -> CInt -> CInt
        -> Ptr Int32 -> Ptr Int32 -> CInt -> Ptr Word8 -> Ptr Word64 -> Ptr Int32 -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_dstreams"
    c_decompressDStreams
        :: Ptr C_Engine -> Ptr C_DStreams -> Ptr Word8 -> CSize -> CInt -> CInt -> Ptr Int32 -> Ptr Int32 -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> CInt -> Ptr CInt -> IO CInt

-- Several GPUs behind one handle (one process, host buffers: a host caller is bound by PCIe, one link per GPU).  The two
-- batch calls take the arguments of c_compressBatch / c_decompressBatch (independent blocks) and give the same bytes; the
-- batch is cut into one contiguous block range per device and the results lie in order in the caller's buffer
-- (include/mi355lz4.h, "several GPUs behind one handle").
data C_Multi
newtype MultiEngine = MultiEngine (Ptr C_Multi)

foreign import ccall safe "mi355lz4.h mi355lz4_create_multi"
    c_createMulti :: Ptr (Ptr C_Multi) -> Ptr CInt -> CInt -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_destroy_multi"
    c_destroyMulti :: Ptr C_Multi -> IO ()
foreign import ccall safe "mi355lz4.h mi355lz4_multi_compress_batch"
    c_multiCompressBatch
        :: Ptr C_Multi -> Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> Ptr Int32 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_multi_decompress_batch"
    c_multiDecompressBatch
        :: Ptr C_Multi -> Ptr Word8 -> CSize -> CInt -> CInt
        -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int32 -> CInt -> Ptr CInt -> IO CInt

-- | One handle over the given HIP devices (e.g. @[0 .. 7]@ for a node).
newMultiEngine :: [Int] -> IO MultiEngine
newMultiEngine devs = alloca $ \pp -> allocaArray (length devs) $ \pd -> do
    pokeArray pd (map fromIntegral devs)
    rc <- c_createMulti pp pd (fromIntegral (length devs))
    when (rc /= 0) $ error "mi355lz4_create_multi failed (no gfx950 device?)"
    MultiEngine <$> peek pp

freeMultiEngine :: MultiEngine -> IO ()
freeMultiEngine (MultiEngine p) = c_destroyMulti p

newEngine :: Int -> IO Engine
newEngine dev = alloca $ \pp -> do
    rc <- c_create pp (fromIntegral dev)
    when (rc /= 0) $ error "mi355lz4_create failed (no gfx950 device?)"
    Engine <$> peek pp

freeEngine :: Engine -> IO ()
freeEngine (Engine p) = c_destroy p

-- | @decodedSizes eng framed framedLen blockOff nBlocks headerKind maxUncomp size outOff@: enqueues the size pass over
-- @nBlocks@ framed blocks in device memory (include/mi355lz4.h, @mi355lz4_decoded_size_device@).  A block decoded into
-- exactly @size[i]@ bytes gives what it gives decoded into @maxUncomp@, so @size@ / @outOff@ are a dense output layout.
decodedSizes :: Engine -> Ptr Word8 -> Word64 -> Ptr Word64 -> Int -> Int -> Int -> Ptr Int32 -> Ptr Word64 -> IO ()
decodedSizes (Engine p) framed framedLen blockOff nBlocks headerKind maxUncomp size outOff = do
    rc <- c_decodedSizeDevice p framed framedLen blockOff (fromIntegral nBlocks) (fromIntegral headerKind)
                              (fromIntegral maxUncomp) size outOff
    when (rc /= 0) $ error "mi355lz4_decoded_size_device failed"

-- | @decompressChunksPrefix eng framed framedLen headerKind fixedUncomp target out cap blockLen maxBlocks@: the first
-- @target@ bytes of every block of the framed chain @framed@ (host memory), packed back to back into @out@; @blockLen[k]@
-- is block k's result (what @LZ4_decompress_safe_partial@ returns for it).  Returns (bytes written, blocks).  Only the
-- prefixes come back from the device (include/mi355lz4.h, @mi355lz4_decompress_partial@).
decompressChunksPrefix :: Engine -> Ptr Word8 -> Int -> Int -> Int -> Int -> Ptr Word8 -> Int -> Ptr Int32 -> Int -> IO (Int, Int)
decompressChunksPrefix (Engine p) framed framedLen headerKind fixedUncomp target out cap blockLen maxBlocks =
    alloca $ \pLen -> alloca $ \pN -> do
        rc <- c_decompressPartial p framed (fromIntegral framedLen) (fromIntegral headerKind) (fromIntegral fixedUncomp)
                                  nullPtr (fromIntegral target) out (fromIntegral cap) pLen blockLen
                                  (fromIntegral maxBlocks) pN
        when (rc /= 0) $ error "mi355lz4_decompress_partial failed"
        n <- peek pLen
        k <- peek pN
        return (fromIntegral n, fromIntegral k)

-- | 'True': 'compressChunksGPU' writes a linked stream (the block before is a block's
-- dictionary, what @LZ4_compress_fast_continue@ does with the previous chunk,
-- Streamly/Internal/LZ4.hs:376,389); 'decompressChunksRawGPU' reads either kind.
setLinkedCompress :: Engine -> Bool -> IO ()
setLinkedCompress (Engine p) on = do
    rc <- c_setLinkedCompress p (if on then 1 else 0)
    when (rc /= 0) $ error "mi355lz4_set_linked_compress failed"

-- | @setBlockChecksum@ (Streamly/Internal/LZ4/Config.hs:151, @undefined@ in the reference): 'True'
-- makes every block carry the xxh32 of its data behind it,
-- @| compLen | uncompLen (optional) | data | checksum (4 bytes) |@.  'compressChunksGPU' writes the
-- trailer; 'decompressChunksRawGPU' expects it behind every block and checks it on the GPU (a mismatch
-- is an error).  The arrays fed to 'decompressChunksRawGPU' must then be sliced with the trailer
-- (compLen + meta + 4 bytes per block), which the reference's @resizeChunksD@ does not know of.
setBlockChecksum :: Engine -> Bool -> IO ()
setBlockChecksum (Engine p) on = do
    rc <- c_setBlockChecksum p (if on then 1 else 0)
    when (rc /= 0) $ error "mi355lz4_set_block_checksum failed"

-- | The compression level of 'compressChunksGPU' (the @lz4 -1@ .. @-12@ choice, which the reference
-- does not offer): 0, the default, is the fast encoder and the @speed@ argument applies; 1..9 select
-- the GPU hash-chain encoder (LZ4HC's levels, smaller output, @speed@ ignored); 10..12 behave as 9.
-- The blocks are ordinary LZ4 blocks: 'decompressChunksRawGPU' and the reference read them unchanged.
setCompressionLevel :: Engine -> Int -> IO ()
setCompressionLevel (Engine p) level = do
    rc <- c_setCompressionLevel p (fromIntegral level)
    when (rc /= 0) $ error "mi355lz4_set_compression_level: a level is 0..12"

-- | Reference-exact compression: while on, 'compressChunksGPU' writes the bytes the reference's 'compressChunks' writes
-- (one linked stream, @LZ4_compress_fast_continue@'s), for compression level 0.  Like @compressChunksD@, which creates
-- one @LZ4_stream_t@ per stream, 'compressChunksGPU' starts a new stream when its output is first pulled, and its
-- batches continue it.  Switching the mode on starts a new stream too.
setCompressExact :: Engine -> Bool -> IO ()
setCompressExact (Engine p) on = do
    rc <- c_setCompressExact p (if on then 1 else 0)
    when (rc /= 0) $ error "mi355lz4_set_compress_exact failed"

-- | Start a new exact compress stream (@LZ4_createStream@).
resetCompressStream :: Engine -> IO ()
resetCompressStream (Engine p) = do
    rc <- c_compressExactReset p
    when (rc /= 0) $ error "mi355lz4_compress_exact_reset failed"

-- | A set of @n@ device-resident compress streams (about 80 KiB each), every one reset.
newCompressStreams :: Engine -> Int -> IO CompressStreams
newCompressStreams (Engine p) n = alloca $ \pp -> do
    rc <- c_cstreamsCreate p (fromIntegral n) pp
    when (rc /= 0) $ error "mi355lz4_cstreams_create failed"
    CompressStreams <$> peek pp

freeCompressStreams :: CompressStreams -> IO ()
freeCompressStreams (CompressStreams p) = c_cstreamsDestroy p

-- | @LZ4_resetStream@ for the listed slots ('Nothing': all of them).
resetCompressStreams :: Engine -> CompressStreams -> Maybe [Int] -> IO ()
resetCompressStreams (Engine p) (CompressStreams cs) Nothing = do
    rc <- c_cstreamsReset p cs nullPtr 0
    when (rc /= 0) $ error "mi355lz4_cstreams_reset failed"
resetCompressStreams (Engine p) (CompressStreams cs) (Just slots) =
    allocaArray (length slots) $ \ps -> do
        pokeArray ps (map fromIntegral slots)
        rc <- c_cstreamsReset p cs ps (fromIntegral (length slots))
        when (rc /= 0) $ error "mi355lz4_cstreams_reset: a slot is out of range"

-- | A set of @n@ device-resident decode streams (about 64 KiB each), every one reset.
newFastStreams :: Engine -> Int -> IO FastStreams
newFastStreams (Engine p) n = alloca $ \pp -> do
    rc <- c_fstreamsCreate p (fromIntegral n) pp
    when (rc /= 0) $ error "mi355lz4_fstreams_create failed"
    FastStreams <$> peek pp

freeFastStreams :: FastStreams -> IO ()
freeFastStreams (FastStreams p) = c_fstreamsDestroy p

-- | Forget the dictionaries of the listed slots (@Nothing@: all of them); enqueued.
resetFastStreams :: Engine -> FastStreams -> Maybe [Int] -> IO ()
resetFastStreams (Engine p) (FastStreams fs) Nothing = do
    rc <- c_fstreamsReset p fs nullPtr 0
    when (rc /= 0) $ error "mi355lz4_fstreams_reset failed"
resetFastStreams (Engine p) (FastStreams fs) (Just slots) =
    allocaArray (max 1 (length slots)) $ \ps -> do
        pokeArray ps (map fromIntegral slots)
        rc <- c_fstreamsReset p fs ps (fromIntegral (length slots))
        when (rc /= 0) $ error "mi355lz4_fstreams_reset: a slot is out of range"

-- | The slot becomes the last 64 KiB of the @len@ bytes of DEVICE memory at @dict@; enqueued, the slot keeps its own copy.
fastStreamsSetDict :: Engine -> FastStreams -> Int -> Ptr Word8 -> Int -> IO ()
fastStreamsSetDict (Engine p) (FastStreams fs) slot dict len = do
    rc <- c_fstreamsSetDict p fs (fromIntegral slot) dict (fromIntegral len)
    when (rc /= 0) $ error "mi355lz4_fstreams_set_dict failed"

-- | The set's compression level for the calls made after this one: 0 the wave encoder (the default), 1..12 the hash-chain
-- encoder (@LZ4_streamHC_t@'s level: it belongs to the streams, not to a call).  Nothing is enqueued.
setFastStreamsLevel :: FastStreams -> Int -> IO ()
setFastStreamsLevel (FastStreams fs) level = do
    rc <- c_fstreamsSetLevel fs (fromIntegral level)
    when (rc /= 0) $ error "mi355lz4_fstreams_set_level: level outside 0..12"

fastStreamsLevel :: FastStreams -> IO Int
fastStreamsLevel (FastStreams fs) = fromIntegral <$> c_fstreamsGetLevel fs

-- Batches of standard LZ4 frames (include/mi355lz4.h, "batches of standard LZ4 frames"): a parsed batch on the device.
data C_Frames
newtype Frames = Frames (Ptr C_Frames)

foreign import ccall safe "mi355lz4.h mi355lz4_frames_create"
    c_framesCreate :: Ptr C_Engine -> Ptr (Ptr C_Frames) -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_frames_destroy"
    c_framesDestroy :: Ptr C_Frames -> IO ()
foreign import ccall safe "mi355lz4.h mi355lz4_frames_load"
    c_framesLoad
        :: Ptr C_Engine -> Ptr C_Frames -> Ptr Word8 -> Word64 -> Ptr Word64 -> Ptr Word64 -> CInt -> CUInt -> IO CInt
foreign import ccall unsafe "mi355lz4.h mi355lz4_frames_inputs"
    c_framesInputs :: Ptr C_Frames -> IO CInt
foreign import ccall unsafe "mi355lz4.h mi355lz4_frames_blocks"
    c_framesBlocks :: Ptr C_Frames -> IO CInt
foreign import ccall unsafe "mi355lz4.h mi355lz4_frames_total"
    c_framesTotal :: Ptr C_Frames -> IO Word64
foreign import ccall unsafe "mi355lz4.h mi355lz4_frames_sizes"
    c_framesSizes :: Ptr C_Frames -> IO (Ptr Int64)
foreign import ccall unsafe "mi355lz4.h mi355lz4_frames_get_sizes"
    c_framesGetSizes :: Ptr C_Frames -> Ptr Int64 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_frames_decode"
    c_framesDecode :: Ptr C_Engine -> Ptr C_Frames -> Ptr Word8 -> Ptr Word64 -> Ptr Int64 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_decompress_frames"
    c_decompressFrames
        :: Ptr C_Engine -> Ptr (Ptr Word8) -> Ptr CSize -> CInt -> CUInt -> Ptr Word8 -> CSize -> Ptr CSize -> Ptr Int64
        -> IO CInt

newFrames :: Engine -> IO Frames
newFrames (Engine p) = alloca $ \pp -> do
    rc <- c_framesCreate p pp
    when (rc /= 0) $ error "mi355lz4_frames_create failed"
    Frames <$> peek pp

freeFrames :: Frames -> IO ()
freeFrames (Frames p) = c_framesDestroy p

-- | Parse @n@ inputs that lie in DEVICE memory (input i is @buf[inOff[i], inOff[i] + inLen[i])@); the exact decoded size of
-- every input, or its negative @MI355LZ4_FRM_E_*@ code.  Waits for the engine's stream; @buf@ is borrowed until the decodes
-- that use it have run.
loadFrames :: Engine -> Frames -> Ptr Word8 -> Word64 -> Ptr Word64 -> Ptr Word64 -> Int -> Int -> IO [Int64]
loadFrames (Engine p) (Frames fr) buf bufLen inOff inLen n flags = do
    rc <- c_framesLoad p fr buf bufLen inOff inLen (fromIntegral n) (fromIntegral flags)
    when (rc /= 0) $ error "mi355lz4_frames_load failed"
    allocaArray (max n 1) $ \ps -> do
        _ <- c_framesGetSizes fr ps
        peekArray n ps

-- | Decode the loaded inputs into DEVICE memory: input i with a size goes to @out[outOff[i], ..)@, @result[i]@ is its size or
-- a code.  Only enqueues on the engine's stream.
decodeFrames :: Engine -> Frames -> Ptr Word8 -> Ptr Word64 -> Ptr Int64 -> IO ()
decodeFrames (Engine p) (Frames fr) out outOff result = do
    rc <- c_framesDecode p fr out outOff result
    when (rc /= 0) $ error "mi355lz4_frames_decode failed"

-- | Many inputs of standard LZ4 frames (each what @lz4 -d@ accepts) decoded in one GPU call: per input its content, or
-- 'Left' its @MI355LZ4_FRM_E_*@ code.  The first call only sizes the output (the C ABI answers a capacity of 0 with the total).
decompressFramesMany :: Engine -> [Array.Array Word8] -> IO [Either Int64 (Array.Array Word8)]
decompressFramesMany (Engine eng) inputs = do
    let n = length inputs
        lens = map Array.byteLength inputs
        offs = scanl (+) 0 lens
    packed <- concatArrays inputs
    allocaArray (max n 1) $ \pIn -> allocaArray (max n 1) $ \pLen -> allocaArray (max n 1) $ \pRes -> alloca $ \pOutLen ->
      Array.asPtrUnsafe (Array.unsafeCast packed) $ \pBytes -> do
        pokeArray pIn [ (pBytes :: Ptr Word8) `plusPtr` o | o <- take n offs ]
        pokeArray pLen (map fromIntegral lens)
        rc0 <- c_decompressFrames eng pIn pLen (fromIntegral n) 0 nullPtr 0 pOutLen pRes
        total <- if rc0 == (-4) then fromIntegral <$> peek pOutLen else return (0 :: Int)
        (MArray.Array cont _ b _) <- MArray.newArray (max total 1)
        rc <- if rc0 == (-4)
                then c_decompressFrames eng pIn pLen (fromIntegral n) 0 b (fromIntegral total) pOutLen pRes
                else return rc0
        when (rc /= 0 && rc /= (-5)) $ error "decompressFramesMany: mi355lz4_decompress_frames failed"
        res <- peekArray n pRes
        let sizes = map (\r -> if r > 0 then fromIntegral r else 0) res
            starts = scanl (+) 0 sizes
        return [ if r < 0 then Left r else Right (Array.Array cont (b `plusPtr` o) (b `plusPtr` (o + l)))
               | (r, o, l) <- zip3 res starts sizes ]

-- Writing batches of standard LZ4 frames (include/mi355lz4.h, "writing batches of standard LZ4 frames"): a frame writer holds
-- the block table and the slots of its calls on the device.
data C_FrameWriter
newtype FrameWriter = FrameWriter (Ptr C_FrameWriter)

foreign import ccall unsafe "mi355lz4.h mi355lz4_cframes_bound"
    c_cframesBound :: Word64 -> CInt -> CUInt -> IO Word64
foreign import ccall safe "mi355lz4.h mi355lz4_cframes_create"
    c_cframesCreate :: Ptr C_Engine -> Ptr (Ptr C_FrameWriter) -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_cframes_destroy"
    c_cframesDestroy :: Ptr C_FrameWriter -> IO ()
foreign import ccall safe "mi355lz4.h mi355lz4_cframes_reserve"
    c_cframesReserve :: Ptr C_Engine -> Ptr C_FrameWriter -> CInt -> Word64 -> Word64 -> CInt -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_cframes_compress"
    c_cframesCompress
        :: Ptr C_Engine -> Ptr C_FrameWriter -> Ptr Word8 -> Word64 -> Ptr Word64 -> Ptr Word64 -> CInt -> Word64 -> Word64
        -> CInt -> CUInt -> CInt -> Ptr Word8 -> Ptr Word64 -> Ptr Word64 -> Ptr Int64 -> IO CInt
foreign import ccall safe "mi355lz4.h mi355lz4_compress_frames"
    c_compressFrames
        :: Ptr C_Engine -> Ptr (Ptr Word8) -> Ptr CSize -> CInt -> CInt -> CUInt -> CInt -> Ptr Word8 -> CSize -> Ptr CSize
        -> Ptr Int64 -> IO CInt

newFrameWriter :: Engine -> IO FrameWriter
newFrameWriter (Engine p) = alloca $ \pp -> do
    rc <- c_cframesCreate p pp
    when (rc /= 0) $ error "mi355lz4_cframes_create failed"
    FrameWriter <$> peek pp

freeFrameWriter :: FrameWriter -> IO ()
freeFrameWriter (FrameWriter p) = c_cframesDestroy p

-- | The exact worst case of one frame of @len@ bytes at block size id 4..7 with the given @MI355LZ4_CFRAMES_*@ flags.
frameBound :: Word64 -> Int -> Int -> IO Word64
frameBound len bsid flags = c_cframesBound len (fromIntegral bsid) (fromIntegral flags)

-- | Size the writer's scratch for calls of at most @n@ inputs, none longer than @maxLen@, @total@ bytes in all.
reserveFrameWriter :: Engine -> FrameWriter -> Int -> Word64 -> Word64 -> Int -> IO ()
reserveFrameWriter (Engine p) (FrameWriter w) n maxLen total bsid = do
    rc <- c_cframesReserve p w (fromIntegral n) maxLen total (fromIntegral bsid)
    when (rc /= 0) $ error "mi355lz4_cframes_reserve failed"

-- | @n@ inputs in DEVICE memory (input i is @src[inOff[i], inOff[i] + inLen[i])@), one frame each at @dst + dstOff[i]@;
-- @frameLen[i]@ is the frame's length or a negative @MI355LZ4_FRW_E_*@ code.  Only enqueues on the engine's stream.
compressFramesDevice
    :: Engine -> FrameWriter -> Ptr Word8 -> Word64 -> Ptr Word64 -> Ptr Word64 -> Int -> Word64 -> Word64 -> Int -> Int -> Int
    -> Ptr Word8 -> Ptr Word64 -> Ptr Word64 -> Ptr Int64 -> IO ()
compressFramesDevice (Engine p) (FrameWriter w) src srcLen inOff inLen n maxLen total bsid flags accel dst dstOff dstCap frameLen = do
    rc <- c_cframesCompress p w src srcLen inOff inLen (fromIntegral n) maxLen total (fromIntegral bsid) (fromIntegral flags)
                            (fromIntegral accel) dst dstOff dstCap frameLen
    when (rc /= 0) $ error "mi355lz4_cframes_compress failed"

-- | Many inputs, one standard LZ4 frame each, in one GPU call (block size id 4..7, @MI355LZ4_CFRAMES_*@ flags): the frames in
-- input order.  The output is sized by the bound, which never fails.
compressFramesMany :: Engine -> Int -> Int -> Int -> [Array.Array Word8] -> IO [Array.Array Word8]
compressFramesMany (Engine eng) bsid flags accel inputs = do
    let n = length inputs
        lens = map Array.byteLength inputs
        offs = scanl (+) 0 lens
    bounds <- mapM (\l -> fromIntegral <$> frameBound (fromIntegral l) bsid flags) lens
    let cap = sum bounds :: Int
    packed <- concatArrays inputs
    allocaArray (max n 1) $ \pIn -> allocaArray (max n 1) $ \pLen -> allocaArray (max n 1) $ \pRes -> alloca $ \pOutLen ->
      Array.asPtrUnsafe (Array.unsafeCast packed) $ \pBytes -> do
        pokeArray pIn [ (pBytes :: Ptr Word8) `plusPtr` o | o <- take n offs ]
        pokeArray pLen (map fromIntegral lens)
        (MArray.Array cont _ b _) <- MArray.newArray (max cap 1)
        rc <- c_compressFrames eng pIn pLen (fromIntegral n) (fromIntegral bsid) (fromIntegral flags) (fromIntegral accel) b
                               (fromIntegral cap) pOutLen pRes
        when (rc /= 0) $ error "compressFramesMany: mi355lz4_compress_frames failed"
        res <- peekArray n pRes
        let sizes = map fromIntegral res :: [Int]
            starts = scanl (+) 0 sizes
        return [ Array.Array cont (b `plusPtr` o) (b `plusPtr` (o + l)) | (o, l) <- zip starts sizes ]

newDecompressStreams :: Engine -> Int -> IO DecompressStreams
newDecompressStreams (Engine p) n = alloca $ \pp -> do
    rc <- c_dstreamsCreate p (fromIntegral n) pp
    when (rc /= 0) $ error "mi355lz4_dstreams_create failed"
    DecompressStreams <$> peek pp

freeDecompressStreams :: DecompressStreams -> IO ()
freeDecompressStreams (DecompressStreams p) = c_dstreamsDestroy p

-- | Forget the dictionaries of the listed slots ('Nothing': all of them): the next block of such a stream starts one.
resetDecompressStreams :: Engine -> DecompressStreams -> Maybe [Int] -> IO ()
resetDecompressStreams (Engine p) (DecompressStreams ds) Nothing = do
    rc <- c_dstreamsReset p ds nullPtr 0
    when (rc /= 0) $ error "mi355lz4_dstreams_reset failed"
resetDecompressStreams (Engine p) (DecompressStreams ds) (Just slots) =
    allocaArray (length slots) $ \ps -> do
        pokeArray ps (map fromIntegral slots)
        rc <- c_dstreamsReset p ds ps (fromIntegral (length slots))
        when (rc /= 0) $ error "mi355lz4_dstreams_reset: a slot is out of range"

batchBlocks :: Int
batchBlocks = 4096

metaSizeOf :: BlockConfig -> Int
metaSizeOf BlockConfig {blockSize} = case blockSize of
    BlockHasSize -> 8
    _ -> 4

fixedUncompOf :: BlockConfig -> Int
fixedUncompOf BlockConfig {blockSize} = case blockSize of
    BlockHasSize -> 0
    BlockMax64KB -> 64 * 1024
    BlockMax256KB -> 256 * 1024
    BlockMax1MB -> 1024 * 1024
    BlockMax4MB -> 4 * 1024 * 1024

-- | One GPU call for a batch of arrays: the batched form of @compressChunk@.
compressBatch :: Engine -> BlockConfig -> Int -> [Array.Array Word8] -> IO [Array.Array Word8]
compressBatch (Engine eng) cfg speed arrs = do
    let n = length arrs
        meta = metaSizeOf cfg
        lens = map Array.byteLength arrs
        -- (+ 4: room for a block checksum, 'setBlockChecksum')
        cap = sum (map (\l -> fromIntegral (c_bound (fromIntegral l)) + meta + 4) lens)
    (MArray.Array cont dstBegin_ dstBegin dstMax) <- MArray.newArray (max cap 1)
    allocaArray n $ \pSrc -> allocaArray n $ \pLen -> allocaArray n $ \pFlen ->
      allocaArray n $ \pStatus -> alloca $ \pOutLen -> do
        -- pin every source for the duration of the call (Array.asPtrUnsafe nests)
        let withAll [] k = k []
            withAll (a:as) k = Array.asPtrUnsafe (Array.unsafeCast a) $ \p -> withAll as (k . (p :))
        withAll arrs $ \ptrs -> do
            pokeArray pSrc ptrs
            pokeArray pLen (map fromIntegral lens)
            rc <- c_compressBatch eng pSrc pLen (fromIntegral n) (fromIntegral speed)
                      (fromIntegral meta) dstBegin (fromIntegral cap) pOutLen pFlen pStatus
            when (rc /= 0) $ error "compressChunks: mi355lz4_compress_batch failed"
        flens <- map fromIntegral <$> peekArray n pFlen
        -- one Array per block: views into the batch buffer, as resizeChunksD does (:480-484)
        let offs = scanl (+) 0 flens
        return [ Array.unsafeFreeze (MArray.Array cont dstBegin_ (dstBegin `plusPtr` (o + l)) dstMax)
                   `seq` Array.Array cont (dstBegin `plusPtr` o) (dstBegin `plusPtr` (o + l))
               | (o, l) <- zip offs flens ]

-- | The next arrays of many @compressChunks@ pipelines in one GPU call: @(slot, arrays)@ per pipeline, every pipeline
-- continuing its slot of the set.  Each pipeline's result is what the reference's @compressChunksD@ yields for those
-- arrays at this point of its stream (the same bytes, one framed array per input array).
compressChunksMany
    :: Engine -> CompressStreams -> BlockConfig -> Int -> [(Int, [Array.Array Word8])] -> IO [[Array.Array Word8]]
compressChunksMany (Engine eng) (CompressStreams cs) cfg speed pipes = do
    let arrs = concatMap snd pipes
        counts = map (length . snd) pipes
        n = length arrs
        ns = length pipes
        meta = metaSizeOf cfg
        lens = map Array.byteLength arrs
        cap = sum (map (\l -> fromIntegral (c_bound (fromIntegral l)) + meta + 4) lens)
    (MArray.Array cont dstBegin_ dstBegin dstMax) <- MArray.newArray (max cap 1)
    allocaArray n $ \pSrc -> allocaArray n $ \pLen -> allocaArray n $ \pFlen ->
      allocaArray n $ \pStatus -> allocaArray (ns + 1) $ \pFirst -> allocaArray ns $ \pSlot -> alloca $ \pOutLen -> do
        let withAll [] k = k []
            withAll (a:as) k = Array.asPtrUnsafe (Array.unsafeCast a) $ \p -> withAll as (k . (p :))
        withAll arrs $ \ptrs -> do
            pokeArray pSrc ptrs
            pokeArray pLen (map fromIntegral lens)
            pokeArray pFirst (map fromIntegral (scanl (+) 0 counts))
            pokeArray pSlot (map (fromIntegral . fst) pipes)
            rc <- c_compressStreams eng cs pSrc pLen (fromIntegral n) pFirst pSlot (fromIntegral ns)
                      (fromIntegral speed) (fromIntegral meta) dstBegin (fromIntegral cap) pOutLen pFlen pStatus
            when (rc /= 0) $ error "compressChunksMany: mi355lz4_compress_streams failed"
        flens <- map fromIntegral <$> peekArray n pFlen
        let offs = scanl (+) 0 flens
            outs = [ Array.unsafeFreeze (MArray.Array cont dstBegin_ (dstBegin `plusPtr` (o + l)) dstMax)
                       `seq` Array.Array cont (dstBegin `plusPtr` o) (dstBegin `plusPtr` (o + l))
                   | (o, l) <- zip offs flens ]
            split [] _ = []
            split (c : rest) xs = let (h, t) = splitAt c xs in h : split rest t
        return (split counts outs)

-- | 'compressChunksMany' by the wave encoder (level 0): @(slot, arrays)@ per pipeline, every pipeline continuing its slot of
-- the set, every array compressed with the last 64 KiB of the array before it in its pipeline as dictionary.  Each pipeline's
-- result is a linked stream that 'decompressChunksMany' reads however it is cut -- not the reference's bytes -- and all
-- arrays of all pipelines are compressed at once.
compressChunksManyFast
    :: Engine -> FastStreams -> BlockConfig -> Int -> [(Int, [Array.Array Word8])] -> IO [[Array.Array Word8]]
compressChunksManyFast (Engine eng) (FastStreams cs) cfg speed pipes = do
    let arrs = concatMap snd pipes
        counts = map (length . snd) pipes
        n = length arrs
        ns = length pipes
        meta = metaSizeOf cfg
        lens = map Array.byteLength arrs
        cap = sum (map (\l -> fromIntegral (c_bound (fromIntegral l)) + meta + 4) lens)
    (MArray.Array cont dstBegin_ dstBegin dstMax) <- MArray.newArray (max cap 1)
    allocaArray n $ \pSrc -> allocaArray n $ \pLen -> allocaArray n $ \pFlen ->
      allocaArray n $ \pStatus -> allocaArray (ns + 1) $ \pFirst -> allocaArray ns $ \pSlot -> alloca $ \pOutLen -> do
        let withAll [] k = k []
            withAll (a:as) k = Array.asPtrUnsafe (Array.unsafeCast a) $ \p -> withAll as (k . (p :))
        withAll arrs $ \ptrs -> do
            pokeArray pSrc ptrs
            pokeArray pLen (map fromIntegral lens)
            pokeArray pFirst (map fromIntegral (scanl (+) 0 counts))
            pokeArray pSlot (map (fromIntegral . fst) pipes)
            rc <- c_compressStreamsFast eng cs pSrc pLen (fromIntegral n) pFirst pSlot (fromIntegral ns)
                      (fromIntegral speed) (fromIntegral meta) dstBegin (fromIntegral cap) pOutLen pFlen pStatus
            when (rc /= 0) $ error "compressChunksManyFast: mi355lz4_compress_streams_fast failed"
        flens <- map fromIntegral <$> peekArray n pFlen
        let offs = scanl (+) 0 flens
            outs = [ Array.unsafeFreeze (MArray.Array cont dstBegin_ (dstBegin `plusPtr` (o + l)) dstMax)
                       `seq` Array.Array cont (dstBegin `plusPtr` o) (dstBegin `plusPtr` (o + l))
                   | (o, l) <- zip offs flens ]
            split [] _ = []
            split (c : rest) xs = let (h, t) = splitAt c xs in h : split rest t
        return (split counts outs)

-- | @LZ4_loadDict@ on one slot of the set: the dictionary is DEVICE memory (@len@ bytes at @dict@); enqueued, the slot keeps its
-- own copy.  The slot then serves 'compressChunksWithDict', or continues through 'compressChunksMany'.
loadDict :: Engine -> CompressStreams -> Int -> Ptr Word8 -> Int -> IO ()
loadDict (Engine p) (CompressStreams cs) slot dict len = do
    rc <- c_cstreamsLoadDict p cs (fromIntegral slot) dict (fromIntegral len)
    when (rc /= 0) $ error "mi355lz4_cstreams_load_dict failed"

-- | A batch of arrays, every one compressed on its own against the loaded slot @slot@ of the set: one framed array per input
-- array, the bytes @LZ4_loadDict@ + @LZ4_compress_fast_continue@ on a copy of the loaded stream write.  The slot is only read.
compressChunksWithDict
    :: Engine -> CompressStreams -> Int -> BlockConfig -> Int -> [Array.Array Word8] -> IO [Array.Array Word8]
compressChunksWithDict (Engine eng) (CompressStreams cs) slot cfg speed arrs = do
    let n = length arrs
        meta = metaSizeOf cfg
        lens = map Array.byteLength arrs
        cap = sum (map (\l -> fromIntegral (c_bound (fromIntegral l)) + meta + 4) lens)
    (MArray.Array cont dstBegin_ dstBegin dstMax) <- MArray.newArray (max cap 1)
    allocaArray n $ \pSrc -> allocaArray n $ \pLen -> allocaArray n $ \pFlen ->
      allocaArray n $ \pStatus -> alloca $ \pOutLen -> do
        let withAll [] k = k []
            withAll (a:as) k = Array.asPtrUnsafe (Array.unsafeCast a) $ \p -> withAll as (k . (p :))
        withAll arrs $ \ptrs -> do
            pokeArray pSrc ptrs
            pokeArray pLen (map fromIntegral lens)
            rc <- c_compressDict eng cs (fromIntegral slot) pSrc pLen (fromIntegral n) (fromIntegral speed)
                      (fromIntegral meta) dstBegin (fromIntegral cap) pOutLen pFlen pStatus
            when (rc /= 0) $ error "compressChunksWithDict: mi355lz4_compress_dict failed"
        flens <- map fromIntegral <$> peekArray n pFlen
        let offs = scanl (+) 0 flens
        return [ Array.unsafeFreeze (MArray.Array cont dstBegin_ (dstBegin `plusPtr` (o + l)) dstMax)
                   `seq` Array.Array cont (dstBegin `plusPtr` o) (dstBegin `plusPtr` (o + l))
               | (o, l) <- zip offs flens ]

-- | A prepared high-compression dictionary on the engine's device, holding the empty dictionary until 'loadHcDict'.
newHcDict :: Engine -> IO HcDict
newHcDict (Engine p) = alloca $ \pp -> do
    rc <- c_hcdictCreate p pp
    when (rc /= 0) $ error "mi355lz4_hcdict_create failed"
    HcDict <$> peek pp

freeHcDict :: HcDict -> IO ()
freeHcDict (HcDict hd) = c_hcdictDestroy hd

-- | Build the object's image from a dictionary in DEVICE memory (@len@ bytes at @dict@, the last 64 KiB count); enqueued, the
-- object keeps its own copy.  It then serves 'compressChunksWithDictHC'.
loadHcDict :: Engine -> HcDict -> Ptr Word8 -> Int -> IO ()
loadHcDict (Engine p) (HcDict hd) dict len = do
    rc <- c_hcdictLoad p hd dict (fromIntegral len)
    when (rc /= 0) $ error "mi355lz4_hcdict_load failed"

-- | The bytes the last 'loadHcDict' kept.
hcDictSize :: HcDict -> IO Int
hcDictSize (HcDict hd) = fromIntegral <$> c_hcdictSize hd

-- | 'compressChunksWithDict' at the engine's compression level 1..12 ('setCompressionLevel'): one framed array per input array,
-- compressed by the hash-chain encoder with the prepared dictionary in front of it.  'decompressChunksWithDict' reads them with
-- the dictionary's bytes.  The object is only read.
compressChunksWithDictHC
    :: Engine -> HcDict -> BlockConfig -> [Array.Array Word8] -> IO [Array.Array Word8]
compressChunksWithDictHC (Engine eng) (HcDict hd) cfg arrs = do
    let n = length arrs
        meta = metaSizeOf cfg
        lens = map Array.byteLength arrs
        cap = sum (map (\l -> fromIntegral (c_bound (fromIntegral l)) + meta + 4) lens)
    (MArray.Array cont dstBegin_ dstBegin dstMax) <- MArray.newArray (max cap 1)
    allocaArray n $ \pSrc -> allocaArray n $ \pLen -> allocaArray n $ \pFlen ->
      allocaArray n $ \pStatus -> alloca $ \pOutLen -> do
        let withAll [] k = k []
            withAll (a:as) k = Array.asPtrUnsafe (Array.unsafeCast a) $ \p -> withAll as (k . (p :))
        withAll arrs $ \ptrs -> do
            pokeArray pSrc ptrs
            pokeArray pLen (map fromIntegral lens)
            rc <- c_compressHcDict eng hd pSrc pLen (fromIntegral n) (fromIntegral meta) dstBegin (fromIntegral cap)
                      pOutLen pFlen pStatus
            when (rc /= 0) $ error "compressChunksWithDictHC: mi355lz4_compress_hcdict failed"
        flens <- map fromIntegral <$> peekArray n pFlen
        let offs = scanl (+) 0 flens
        return [ Array.unsafeFreeze (MArray.Array cont dstBegin_ (dstBegin `plusPtr` (o + l)) dstMax)
                   `seq` Array.Array cont (dstBegin `plusPtr` o) (dstBegin `plusPtr` (o + l))
               | (o, l) <- zip offs flens ]

-- | The same at level 0 by the wave encoder, with acceleration @accel@: the engine's own fast parse against the prepared
-- dictionary, not the reference's bytes ('compressChunksWithDict' has those).  'decompressChunksWithDict' reads the result.
compressChunksWithDictFast
    :: Engine -> HcDict -> Int -> BlockConfig -> [Array.Array Word8] -> IO [Array.Array Word8]
compressChunksWithDictFast (Engine eng) (HcDict hd) accel cfg arrs = do
    let n = length arrs
        meta = metaSizeOf cfg
        lens = map Array.byteLength arrs
        cap = sum (map (\l -> fromIntegral (c_bound (fromIntegral l)) + meta + 4) lens)
    (MArray.Array cont dstBegin_ dstBegin dstMax) <- MArray.newArray (max cap 1)
    allocaArray n $ \pSrc -> allocaArray n $ \pLen -> allocaArray n $ \pFlen ->
      allocaArray n $ \pStatus -> alloca $ \pOutLen -> do
        let withAll [] k = k []
            withAll (a:as) k = Array.asPtrUnsafe (Array.unsafeCast a) $ \p -> withAll as (k . (p :))
        withAll arrs $ \ptrs -> do
            pokeArray pSrc ptrs
            pokeArray pLen (map fromIntegral lens)
            rc <- c_compressFastDict eng hd pSrc pLen (fromIntegral n) (fromIntegral accel) (fromIntegral meta) dstBegin (fromIntegral cap)
                      pOutLen pFlen pStatus
            when (rc /= 0) $ error "compressChunksWithDictFast: mi355lz4_compress_fastdict failed"
        flens <- map fromIntegral <$> peekArray n pFlen
        let offs = scanl (+) 0 flens
        return [ Array.unsafeFreeze (MArray.Array cont dstBegin_ (dstBegin `plusPtr` (o + l)) dstMax)
                   `seq` Array.Array cont (dstBegin `plusPtr` o) (dstBegin `plusPtr` (o + l))
               | (o, l) <- zip offs flens ]

-- | A set of prepared dictionaries for 'compressChunksWithDictsFast' and 'decompressChunksWithDicts'.  The members are borrowed:
-- free them after the set.  The same 'HcDict' may stand at several indices, and 'loadHcDict' on a member is seen by the set.
newDictSet :: Engine -> [HcDict] -> IO DictSet
newDictSet (Engine p) members = withArrayLen [hd | HcDict hd <- members] $ \n pMembers -> alloca $ \pp -> do
    rc <- c_dictsetCreate p pMembers (fromIntegral n) pp
    when (rc /= 0) $ error "newDictSet: mi355lz4_dictset_create failed"
    DictSet <$> peek pp

freeDictSet :: DictSet -> IO ()
freeDictSet (DictSet ds) = c_dictsetDestroy ds

dictSetCount :: DictSet -> IO Int
dictSetCount (DictSet ds) = fromIntegral <$> c_dictsetCount ds

-- | 'compressChunksWithDictFast' with a dictionary per array: @(index, array)@ pairs, the index naming a member of the set or
-- @-1@ for none.  Every array comes out as 'compressChunksWithDictFast' writes it against that member alone.
compressChunksWithDictsFast
    :: Engine -> DictSet -> Int -> BlockConfig -> [(Int, Array.Array Word8)] -> IO [Array.Array Word8]
compressChunksWithDictsFast (Engine eng) (DictSet ds) accel cfg pairs = do
    let arrs = map snd pairs
        n = length arrs
        meta = metaSizeOf cfg
        lens = map Array.byteLength arrs
        cap = sum (map (\l -> fromIntegral (c_bound (fromIntegral l)) + meta + 4) lens)
    (MArray.Array cont dstBegin_ dstBegin dstMax) <- MArray.newArray (max cap 1)
    allocaArray n $ \pSrc -> allocaArray n $ \pLen -> allocaArray n $ \pIdx -> allocaArray n $ \pFlen ->
      allocaArray n $ \pStatus -> alloca $ \pOutLen -> do
        let withAll [] k = k []
            withAll (a:as) k = Array.asPtrUnsafe (Array.unsafeCast a) $ \p -> withAll as (k . (p :))
        withAll arrs $ \ptrs -> do
            pokeArray pSrc ptrs
            pokeArray pLen (map fromIntegral lens)
            pokeArray pIdx (map (fromIntegral . fst) pairs)
            rc <- c_compressFastDictMulti eng ds pIdx pSrc pLen (fromIntegral n) (fromIntegral accel) (fromIntegral meta) dstBegin
                      (fromIntegral cap) pOutLen pFlen pStatus
            when (rc /= 0) $ error "compressChunksWithDictsFast: mi355lz4_compress_fastdict_multi failed"
        flens <- map fromIntegral <$> peekArray n pFlen
        let offs = scanl (+) 0 flens
        return [ Array.unsafeFreeze (MArray.Array cont dstBegin_ (dstBegin `plusPtr` (o + l)) dstMax)
                   `seq` Array.Array cont (dstBegin `plusPtr` o) (dstBegin `plusPtr` (o + l))
               | (o, l) <- zip offs flens ]

-- | Fixed-size output pages: every array cut into a chain of at most @maxPages@ pages whose blocks are at most @pageSize@
-- bytes; page k is what @LZ4_compress_destSize@ makes of the bytes behind pages 0..k-1.  Per input: its pages in order, each with
-- the configuration's header in front of its block, and the bytes of the input they hold (less than its length when
-- @maxPages@ was too few).  Block checksums must be off.
compressChunksPaged
    :: Engine -> BlockConfig -> Int -> Int -> [Array.Array Word8] -> IO [([Array.Array Word8], Int)]
compressChunksPaged (Engine eng) = pagedWith "compressChunksPaged" (c_compressPages eng)

-- | 'compressChunksPaged' at the engine's speed (@mi355lz4_compress_pages_fast@, acceleration @accel@): every page is a prefix
-- of the sequences the level-0 encoder finds in the next 64 KiB at the most, closed by the literal run that fills the page.  The
-- pages are valid LZ4 blocks that decode on their own, not @LZ4_compress_destSize@'s bytes; highly compressible input gives pages
-- that are not full.  The engine must be at level 0, block checksums off.
compressChunksPagedFast
    :: Engine -> Int -> BlockConfig -> Int -> Int -> [Array.Array Word8] -> IO [([Array.Array Word8], Int)]
compressChunksPagedFast (Engine eng) accel =
    pagedWith "compressChunksPagedFast" (\pSrc pLen n ps mp -> c_compressPagesFast eng pSrc pLen n ps mp (fromIntegral accel))

-- | 'compressChunksPagedFast' with the dictionary of a loaded 'HcDict' in front of every page
-- (@mi355lz4_compress_pages_fastdict@): a page is a prefix of the block 'compressChunksWithDictFast' writes for the next 64 KiB at
-- the most, closed by the literal run that fills the page, and decodes with the same dictionary.  Small records fill about half
-- as many pages as without the dictionary.  The engine must be at level 0, block checksums off; the object is only read.
compressChunksPagedWithDictFast
    :: Engine -> HcDict -> Int -> BlockConfig -> Int -> Int -> [Array.Array Word8] -> IO [([Array.Array Word8], Int)]
compressChunksPagedWithDictFast (Engine eng) (HcDict hd) accel =
    pagedWith "compressChunksPagedWithDictFast"
        (\pSrc pLen n ps mp -> c_compressPagesFastDict eng hd pSrc pLen n ps mp (fromIntegral accel))

pagedWith
    :: String
    -> (Ptr (Ptr Word8) -> Ptr Int32 -> CInt -> CInt -> CInt -> CInt -> Ptr Word8 -> CSize -> Ptr Int32 -> Ptr Int32 -> Ptr Int32
        -> Ptr Int32 -> IO CInt)
    -> BlockConfig -> Int -> Int -> [Array.Array Word8] -> IO [([Array.Array Word8], Int)]
pagedWith who call cfg pageSize maxPages arrs = do
    let n = length arrs
        meta = metaSizeOf cfg
        stride = meta + max pageSize 1
        np = n * max maxPages 1
        lens = map Array.byteLength arrs
    (MArray.Array cont dstBegin_ dstBegin dstMax) <- MArray.newArray (max (np * stride) 1)
    allocaArray (max n 1) $ \pSrc -> allocaArray (max n 1) $ \pLen -> allocaArray (max np 1) $ \pSrcLen ->
      allocaArray (max np 1) $ \pCompLen -> allocaArray (max n 1) $ \pCount -> allocaArray (max n 1) $ \pCons -> do
        let withAll [] k = k []
            withAll (a:as) k = Array.asPtrUnsafe (Array.unsafeCast a) $ \p -> withAll as (k . (p :))
        withAll arrs $ \ptrs -> do
            pokeArray pSrc ptrs
            pokeArray pLen (map fromIntegral lens)
            rc <- call pSrc pLen (fromIntegral n) (fromIntegral pageSize) (fromIntegral maxPages)
                      (fromIntegral meta) dstBegin (fromIntegral stride) pSrcLen pCompLen pCount pCons
            when (rc /= 0) $ error (who ++ ": the call failed")
        counts <- map fromIntegral <$> peekArray n pCount
        cons <- map fromIntegral <$> peekArray n pCons
        comp <- map fromIntegral <$> peekArray np (pCompLen :: Ptr Int32)
        return [ ( [ let o = (i * maxPages + k) * stride
                         l = meta + comp !! (i * maxPages + k)
                     in Array.unsafeFreeze (MArray.Array cont dstBegin_ (dstBegin `plusPtr` (o + l)) dstMax)
                          `seq` Array.Array cont (dstBegin `plusPtr` o) (dstBegin `plusPtr` (o + l))
                   | k <- [0 .. c - 1] ]
                 , used )
               | (i, c, used) <- zip3 [0 ..] counts cons ]

-- | A batch of resized blocks (header + data each), every one decoded against the dictionary (host memory, may be empty) as
-- @LZ4_decompress_safe_usingDict@ does: one decoded array per block.
decompressChunksWithDict
    :: Engine -> BlockConfig -> Array.Array Word8 -> [Array.Array Word8] -> IO [Array.Array Word8]
decompressChunksWithDict (Engine eng) cfg dict blocks = do
    let n = length blocks
        meta = metaSizeOf cfg
    framed <- concatArrays blocks
    cap <- sum <$> forM blocks (\a -> Array.asPtrUnsafe (Array.unsafeCast a) $ \p ->
               if meta == 8 then fromIntegral <$> (peek (castPtr p `plusPtr` 4) :: IO Int32)
                            else return (fixedUncompOf cfg))
    (MArray.Array cont _ b _) <- MArray.newArray (max cap 1)
    allocaArray (max n 1) $ \pBlen -> alloca $ \pOutLen -> alloca $ \pN ->
      Array.asPtrUnsafe (Array.unsafeCast framed) $ \pIn -> Array.asPtrUnsafe (Array.unsafeCast dict) $ \pDict -> do
        rc <- c_decompressDict eng pIn (fromIntegral (Array.byteLength framed)) (fromIntegral meta)
                  (fromIntegral (fixedUncompOf cfg)) pDict (fromIntegral (Array.byteLength dict))
                  b (fromIntegral cap) pOutLen pBlen (fromIntegral n) pN
        when (rc /= 0) $ error "decompressChunksWithDict: mi355lz4_decompress_dict failed"
        lens <- map fromIntegral <$> peekArray n pBlen
        let offs = scanl (+) 0 lens
        return [ Array.Array cont (b `plusPtr` o) (b `plusPtr` (o + l)) | (o, l) <- zip offs lens ]

-- | 'decompressChunksWithDict' with a dictionary per block: @(index, block)@ pairs, every block decoded against the kept bytes of
-- the member it names (@-1@: none).  One decoded array per block.
decompressChunksWithDicts
    :: Engine -> DictSet -> BlockConfig -> [(Int, Array.Array Word8)] -> IO [Array.Array Word8]
decompressChunksWithDicts (Engine eng) (DictSet ds) cfg pairs = do
    let blocks = map snd pairs
        n = length blocks
        meta = metaSizeOf cfg
    framed <- concatArrays blocks
    cap <- sum <$> forM blocks (\a -> Array.asPtrUnsafe (Array.unsafeCast a) $ \p ->
               if meta == 8 then fromIntegral <$> (peek (castPtr p `plusPtr` 4) :: IO Int32)
                            else return (fixedUncompOf cfg))
    (MArray.Array cont _ b _) <- MArray.newArray (max cap 1)
    allocaArray (max n 1) $ \pBlen -> allocaArray (max n 1) $ \pIdx -> alloca $ \pOutLen -> alloca $ \pN ->
      Array.asPtrUnsafe (Array.unsafeCast framed) $ \pIn -> do
        pokeArray pIdx (map (fromIntegral . fst) pairs)
        rc <- c_decompressDictMulti eng pIn (fromIntegral (Array.byteLength framed)) (fromIntegral meta)
                  (fromIntegral (fixedUncompOf cfg)) ds pIdx b (fromIntegral cap) pOutLen pBlen (fromIntegral n) pN
        when (rc /= 0) $ error "decompressChunksWithDicts: mi355lz4_decompress_dict_multi failed"
        lens <- map fromIntegral <$> peekArray n pBlen
        let offs = scanl (+) 0 lens
        return [ Array.Array cont (b `plusPtr` o) (b `plusPtr` (o + l)) | (o, l) <- zip offs lens ]

-- | The next resized blocks of many @decompressChunksRaw@ pipelines in one GPU call, the counterpart of
-- 'compressChunksMany': @(slot, blocks)@ per pipeline, every pipeline continuing its slot of the set -- what the
-- reference's @decompressChunksRawD@ threads through as the previous output array lives in the slot, on the device.
-- Each pipeline's result is one decoded array per block.
decompressChunksMany
    :: Engine -> DecompressStreams -> BlockConfig -> [(Int, [Array.Array Word8])] -> IO [[Array.Array Word8]]
decompressChunksMany (Engine eng) (DecompressStreams ds) cfg pipes = do
    let blocks = concatMap snd pipes
        counts = map (length . snd) pipes
        n = length blocks
        ns = length pipes
        meta = metaSizeOf cfg
    framed <- concatArrays blocks                         -- blocks back to back, pipeline after pipeline
    cap <- sum <$> forM blocks (\a -> Array.asPtrUnsafe (Array.unsafeCast a) $ \p ->
               if meta == 8 then fromIntegral <$> (peek (castPtr p `plusPtr` 4) :: IO Int32)
                            else return (fixedUncompOf cfg))
    (MArray.Array cont _ b _) <- MArray.newArray (max cap 1)
    allocaArray (max n 1) $ \pBlen -> allocaArray (ns + 1) $ \pFirst -> allocaArray (max ns 1) $ \pSlot ->
      alloca $ \pOutLen -> alloca $ \pN ->
        Array.asPtrUnsafe (Array.unsafeCast framed) $ \pIn -> do
            pokeArray pFirst (map fromIntegral (scanl (+) 0 counts))
            pokeArray pSlot (map (fromIntegral . fst) pipes)
            rc <- c_decompressDStreams eng ds pIn (fromIntegral (Array.byteLength framed)) (fromIntegral meta)
                      (fromIntegral (fixedUncompOf cfg)) pFirst pSlot (fromIntegral ns)
                      b (fromIntegral cap) pOutLen pBlen (fromIntegral n) pN
            when (rc /= 0) $ error "decompressChunksMany: mi355lz4_decompress_dstreams failed"
            lens <- map fromIntegral <$> peekArray n pBlen
            let offs = scanl (+) 0 lens
                outs = [ Array.Array cont (b `plusPtr` o) (b `plusPtr` (o + l)) | (o, l) <- zip offs lens ]
                split [] _ = []
                split (c : rest) xs = let (h, t) = splitAt c xs in h : split rest t
            return (split counts outs)

-- | One freshly allocated array holding the given arrays back to back (the reference splices
-- pairwise with @Array.splice@, Streamly/Internal/LZ4.hs:502; a batch is concatenated in one pass).
concatArrays :: [Array.Array Word8] -> IO (Array.Array Word8)
concatArrays arrs = do
    let total = sum (map Array.byteLength arrs)
    (MArray.Array cont b_ b bound) <- MArray.newArray (max total 1)
    let go _ [] = return ()
        go o (a : as) = do
            let l = Array.byteLength a
            Array.asPtrUnsafe (Array.unsafeCast a) $ \p -> copyBytes (b `plusPtr` o) (p :: Ptr Word8) l
            go (o + l) as
    go 0 arrs
    return $ Array.unsafeFreeze (MArray.Array cont b_ (b `plusPtr` total) bound)

-- | Drop-in for @compressChunksD@ (Streamly/Internal/LZ4.hs:353-394).
compressChunksGPU
    :: MonadIO m
    => Engine -> BlockConfig -> Int
    -> Stream.Stream m (Array.Array Word8) -> Stream.Stream m (Array.Array Word8)
compressChunksGPU eng cfg speed0 =
      Stream.concatMap Stream.fromList
    . Stream.mapM (liftIO . compressBatch eng cfg (max speed0 0))
    . Stream.groupsOf batchBlocks Fold.toList
    . startExactStream eng

-- | Before the first array is pulled: a new exact stream when the engine is in the reference-exact mode (one
-- @LZ4_stream_t@ per @compressChunksD@, Streamly/Internal/LZ4.hs:353-394); otherwise nothing.
startExactStream :: MonadIO m => Engine -> Stream.Stream m a -> Stream.Stream m a
startExactStream (Engine p) (Stream.Stream step0 st0) = Stream.Stream step (Left st0)
  where
    step _ (Left st) = do
        liftIO $ do
            on <- c_getCompressExact p
            when (on == 1) $ do
                rc <- c_compressExactReset p
                when (rc /= 0) $ error "mi355lz4_compress_exact_reset failed"
        return $ Stream.Skip (Right st)
    step gst (Right st) = do
        r <- step0 gst st
        return $ case r of
            Stream.Yield a st' -> Stream.Yield a (Right st')
            Stream.Skip st' -> Stream.Skip (Right st')
            Stream.Stop -> Stream.Stop

-- | Drop-in for @decompressChunksRawD@ (Streamly/Internal/LZ4.hs:539-567): the incoming
-- arrays are resized blocks; the previous output array is threaded through as the
-- dictionary of the next batch (linked = 1 gives the reference's stream semantics).
decompressChunksRawGPU
    :: MonadIO m
    => Engine -> BlockConfig
    -> Stream.Stream m (Array.Array Word8) -> Stream.Stream m (Array.Array Word8)
decompressChunksRawGPU (Engine eng) cfg (Stream.Stream step0 st0) =
    Stream.Stream step (st0, Nothing, [], False)
  where
    meta = metaSizeOf cfg
    step _ (st, prev, o : os, done) = return $ Stream.Yield o (st, prev, os, done)
    step _ (_, _, [], True) = return Stream.Stop
    step gst (st, prev, [], False) = do
        (batch, st', done) <- gather gst st batchBlocks []
        if null batch
        then return $ Stream.Skip (st', prev, [], True)
        else do
            outs <- liftIO $ decompressBatch prev batch
            let prev' = case filter ((> 0) . Array.byteLength) outs of
                          [] -> prev
                          xs -> Just (last xs)          -- only a result > 0 moves the dictionary
            return $ Stream.Skip (st', prev', outs, done)
    gather _ st 0 acc = return (reverse acc, st, False)
    gather gst st k acc = do
        r <- step0 gst st
        case r of
            Stream.Yield a st1 -> gather gst st1 (k - 1 :: Int) (a : acc)
            Stream.Skip st1 -> gather gst st1 k acc
            Stream.Stop -> return (reverse acc, st, True)
    decompressBatch prev batch = do
        framed <- concatArrays batch                      -- blocks back to back
        let n = length batch
        -- capacity: sum of the header (or fixed) uncompressed sizes, computed as decompressChunk does
        cap <- sum <$> forM batch (\a -> Array.asPtrUnsafe (Array.unsafeCast a) $ \p ->
                   if meta == 8 then fromIntegral <$> (peek (castPtr p `plusPtr` 4) :: IO Int32)
                                else return (fixedUncompOf cfg))
        (MArray.Array cont b_ b e) <- MArray.newArray (max cap 1)
        allocaArray n $ \pBlen -> alloca $ \pOutLen -> alloca $ \pN ->
          Array.asPtrUnsafe (Array.unsafeCast framed) $ \pIn -> do
            let call dp dl = c_decompressBatch eng pIn (fromIntegral (Array.byteLength framed))
                                 (fromIntegral meta) (fromIntegral (fixedUncompOf cfg)) 1 dp dl
                                 b (fromIntegral cap) pOutLen pBlen (fromIntegral n) pN
            rc <- case prev of
                    Nothing -> call nullPtr 0
                    Just d -> Array.asPtrUnsafe (Array.unsafeCast d) $ \dp ->
                                  call dp (fromIntegral (Array.byteLength d))
            when (rc /= 0) $ error "decompressChunk: c_decompressSafeContinue failed."
            lens <- map fromIntegral <$> peekArray n pBlen
            let offs = scanl (+) 0 lens
            return [ Array.Array cont (b `plusPtr` o) (b `plusPtr` (o + l)) | (o, l) <- zip offs lens ]
