// kernels/encode.inc -- the encoders: k_encode, k_encode_hc, the reference-exact chain and streams, the segment encoder of small batches.
// A part of kernels.hip, the one device translation unit: included there, in this order, and not compiled on its own.
#include "encode_common.inc"

// ---------------------------------------------------------------------------
// K2: encode
// ---------------------------------------------------------------------------
// MOD: table entries are positions modulo 64 Ki (encode_wave.hpp, tab_candidate): needed when positions run beyond
// 64 Ki -- blocks above 64 KiB, or a dictionary in front of the block (linked compression).  The table is the same
// size either way, so every block size runs at the same occupancy (a table of 32-bit positions would halve it).
#ifndef ENC_WAVES_PER_EU
#define ENC_WAVES_PER_EU 4
#endif
// PAIR: two dense windows per step (encode_wave.hpp): blocks of up to 64 KiB, independent or linked (measured: +6 % /
// +5 %); blocks above 64 KiB run one window per step (-9 % with pairs).
template <bool MOD, bool PAIR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ENC_WAVES_PER_EU, ENC_WAVES_PER_EU))) void k_encode(EncodeArgs a)
{
#ifndef ENC_LDS_PAD
#define ENC_LDS_PAD 0
#endif
    // positions + tags (encode_wave.hpp): 10 KiB, 16 waves per CU (the ENC_STAGE experiment's 256 bytes behind them make it 15)
    __shared__ __attribute__((aligned(16))) uint16_t table[ENC_TABLE_ENTRIES + ENC_LDS_PAD + ((PAIR && ENC_STAGE) ? 128 : 0)];
    const int blk = (int)blockIdx.x;
    const EncBlock b = enc_block(a, blk);
    uint8_t *slot = a.slots + (size_t)blk * a.slotStride;
    const int dictLen = MOD ? enc_linked_dict(a, blk, b.off) : 0;
    int c = 0;
    if (b.n >= 0 && (MOD || b.n <= 65536))
        c = encode_block_wave<uint16_t, MOD, false, PAIR>(a.src + b.off, b.n, slot + a.headerKind, a.accel, table, a.stats, dictLen);
    enc_finish_slot(a, blk, slot, c, b.n, lane_id() == 0);
}

void launch_encode(const EncodeArgs &a, bool bigBlocks, hipStream_t s)
{
    if (a.nBlocks <= 0) return;
    const dim3 grid((unsigned)a.nBlocks), wg(64);
    if (bigBlocks) hipLaunchKernelGGL((k_encode<true, false>), grid, wg, 0, s, a);
    else if (a.linked) hipLaunchKernelGGL((k_encode<true, true>), grid, wg, 0, s, a);
#ifdef ENC_EXP_NOPAIR
    else hipLaunchKernelGGL((k_encode<false, false>), grid, wg, 0, s, a);
#else
    else hipLaunchKernelGGL((k_encode<false, true>), grid, wg, 0, s, a);
#endif
}

// ---------------------------------------------------------------------------
// K2, high-compression levels (encode_hc.hpp): one workgroup of HC_THREADS per block, all of a CU's LDS, a persistent grid
// of one workgroup per CU striding over the blocks.  Same slots, headers, framedLen and dictionary as k_encode.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(HC_THREADS) void k_encode_hc(EncodeArgs a, int depth)
{
    __shared__ HcLds L;
    for (int blk = (int)blockIdx.x; blk < a.nBlocks; blk += (int)gridDim.x) {
        const EncBlock b = enc_block(a, blk);
        uint8_t *slot = a.slots + (size_t)blk * a.slotStride;
        const int dictLen = enc_linked_dict(a, blk, b.off);
        int c = 0;
        if (b.n >= 0) c = encode_block_hc(L, a.src + b.off, b.n, dictLen, slot + a.headerKind, depth);
        enc_finish_slot(a, blk, slot, c, b.n, threadIdx.x == 0);
    }
}

// the current device's CU count (the persistent grids' size), asked for once per device
static int hc_cu_count()
{
    static int cus[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    int &nc = cus[dev & 63];
    if (nc <= 0 && hipDeviceGetAttribute(&nc, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) nc = 256;
    return max(nc, 1);
}

void launch_encode_hc(const EncodeArgs &a, int level, hipStream_t s)
{
    if (a.nBlocks <= 0) return;
    const int depth = 1 << (min(level, 9) - 1);
    const unsigned grid = (unsigned)min(a.nBlocks, hc_cu_count());
    hipLaunchKernelGGL(k_encode_hc, dim3(grid), dim3(HC_THREADS), 0, s, a, depth);
}

// ---------------------------------------------------------------------------
// K2, high-compression levels against a shared dictionary (mi355lz4_hcdict, DESIGN.md 7j).  k_hcdict_build runs the dictionary's
// insert rounds once and stores the tables; k_encode_hc_dict reloads them for every block instead of inserting 64 KiB again.
// ---------------------------------------------------------------------------
static_assert(HCDICT_HEAD_ENTRIES == HC_HEAD && HCDICT_TABLE_BYTES == offsetof(HcLds, best) && HCDICT_TABLE_BYTES % 16 == 0,
              "the image is the front of HcLds: chain[], then head[]");

// The image of a dictionary of `len` bytes at `dict` (its last keep = min(len, 65536) count): chain[] and head[] after hc_insert
// over the window positions [0, keep - 3) of the kept bytes alone -- the positions whose four bytes lie inside them -- from
// zeroed chains and empty heads, then keep and the bytes.  One workgroup.  Under 4 bytes no position is inserted.
__global__ __launch_bounds__(HC_THREADS) void k_hcdict_build(uint8_t *image, const uint8_t *dict, int len)
{
    __shared__ HcLds L;
    const int t = (int)threadIdx.x;
    const int keep = min(max(len, 0), 65536);
    const uint8_t *from = dict + (len - keep);                          // (not dereferenced when keep == 0)
    dev_v4 *tab4 = (dev_v4 *)&L;
    for (int i = t; i < (int)(HCDICT_CHAIN_BYTES / 16); i += HC_THREADS) tab4[i] = dev_v4{0u, 0u, 0u, 0u};
    for (int i = t; i < HC_HEAD; i += HC_THREADS) L.head[i] = HC_NONE;
    __syncthreads();
    for (int r = 0; r + 4 <= keep; r += HC_THREADS) hc_insert(L, from, r, min(r + HC_THREADS, keep), keep);
    for (int i = t; i < (int)(HCDICT_TABLE_BYTES / 16); i += HC_THREADS) as_global((dev_v4 *)image)[i] = tab4[i];
    if (t == 0) as_global((uint32_t *)(image + HCDICT_KEEP_OFF))[0] = (uint32_t)keep;
    wg_copy_pieces(image + HCDICT_DICT_OFF, from, (uint32_t)keep, 4096u, (uint32_t)(t / LZ4_WAVE), HC_WAVES);     // the bytes
}

void launch_hcdict_build(uint8_t *image, const uint8_t *dict, int len, hipStream_t s)
{
    hipLaunchKernelGGL(k_hcdict_build, dim3(1), dim3(HC_THREADS), 0, s, image, dict, len);
}

// k_encode_hc with the dictionary of a mi355lz4_hcdict in front of every block: the same persistent grid, one window of x.stage per
// workgroup.  The kept bytes go into the window once; for every block the workgroup copies the block behind them, reloads the
// whole table image (the block before has overwritten heads and ring entries) and runs encode_block_hc<PREPARED>, which inserts
// the three seam positions and then does what it does for the second block of a linked call.  A length outside
// 0..uniformLen gives framedLen 0 and leaves the slot alone.  Nothing of the image is written.
__global__ __launch_bounds__(HC_THREADS) void k_encode_hc_dict(HcDictArgs x, int depth)
{
    __shared__ HcLds L;
    const int t = (int)threadIdx.x, wave = t >> 6;
    const EncodeArgs &a = x.e;
    const int keep = (int)min(ex_uni(as_global((const uint32_t *)(x.image + HCDICT_KEEP_OFF))[0]), 65536u);
    uint8_t *blockAt = x.stage + (size_t)blockIdx.x * x.stageStride + 65536;
    wg_copy_pieces(blockAt - keep, x.image + HCDICT_DICT_OFF, (uint32_t)keep, 4096u, (uint32_t)wave, HC_WAVES);
    for (int blk = (int)blockIdx.x; blk < a.nBlocks; blk += (int)gridDim.x) {
        const EncBlock b = enc_block(a, blk);
        const int n = b.n;
        if (n < 0 || n > a.uniformLen) {
            if (t == 0) a.framedLen[blk] = 0;
            continue;
        }
        uint8_t *slot = a.slots + (size_t)blk * a.slotStride;
        int c;
        if (n < LZ4_MFLIMIT + 1) {                                      // all literals: no window, no table
            c = encode_block_hc<true>(L, a.src + b.off, n, 0, slot + a.headerKind, depth);
        } else {
            __syncthreads();                                            // wave 0 may still be reading the block before from the window
            wg_copy_pieces(blockAt, a.src + b.off, (uint32_t)n, 1024u, (uint32_t)wave, HC_WAVES);
            for (int i = t; i < (int)(HCDICT_TABLE_BYTES / 16); i += HC_THREADS) ((dev_v4 *)&L)[i] = as_global((const dev_v4 *)x.image)[i];
            c = encode_block_hc<true>(L, blockAt, n, keep, slot + a.headerKind, depth);   // (its first barrier is behind both copies)
        }
        enc_finish_slot(a, blk, slot, c, n, t == 0);
    }
}

int encode_hc_dict_grid(int nBlocks) { return min(nBlocks, hc_cu_count()); }

void launch_encode_hc_dict(const HcDictArgs &a, int level, hipStream_t s)
{
    if (a.e.nBlocks <= 0) return;
    const int depth = 1 << (min(level, 9) - 1);
    hipLaunchKernelGGL(k_encode_hc_dict, dim3((unsigned)encode_hc_dict_grid(a.e.nBlocks)), dim3(HC_THREADS), 0, s, a, depth);
}

// ---------------------------------------------------------------------------
// K2, the wave encoder against a shared dictionary (mi355lz4_hcdict at level 0, DESIGN.md 7l).  Block i comes out as the second
// block of the linked call [kept bytes, block i] through k_encode<true, PAIR>.  That kernel zeroes its table and enters every
// ENC_SEED_STEP-th position of the dictionary for every block: 64 KiB of seeding for a record of 4 KiB.  Here the table after the
// seeding is an image made once per load, and a block reloads it.
//
// The seed loop (encode_wave.hpp) is a sequence of STEPS: step s enters the 64 positions s * span + lane * ENC_SEED_STEP
// (span = 64 * ENC_SEED_STEP) with one LDS store and the tag's two atomics.  Lanes of one step that meet in a bucket settle it
// inside those instructions, so a step is replayed whole or not at all.  The last positions (q > keep - 5) hash bytes of the block
// and cannot be in the image: the image is the table after every step in front of the first one that holds such a position
// (header word 1: that step's first position), and every block replays the remaining one or two steps against its staged bytes.
// ---------------------------------------------------------------------------
static_assert(FASTDICT_TABLE_BYTES == ENC_TABLE_ENTRIES * sizeof(uint16_t) && FASTDICT_TABLE_BYTES % 16 == 0,
              "the fast image is the wave encoder's table: positions, then tags");
#define ENC_SEED_SPAN (LZ4_WAVE * ENC_SEED_STEP)

// One step of the seed loop, with its lane-to-position mapping and its instructions: positions q0 + lane * ENC_SEED_STEP below
// dictLen.  EXACT_END (the builder, which has no block behind the kept bytes): a position whose 8-byte load would pass src +
// dictLen reads its five hashed bytes one by one; such a position must have all five inside (it does in every step the builder runs).
template <bool EXACT_END>
__device__ __forceinline__ void enc_seed_step(uint16_t *table, const uint8_t *src, int q0, int dictLen)
{
    ENC_TAG_DECL
    const int q = q0 + lane_id() * ENC_SEED_STEP;
    uint64_t v = 0ull;
    if (q < dictLen) {
        if (!EXACT_END || q + 8 <= dictLen) v = *(const LZ4_GLOBAL u64_unaligned *)as_global(src + q);
        else for (int i = 0; i < 5; i++) v |= (uint64_t)as_global(src)[q + i] << (8 * i);
    }
    if (q < dictLen) { uint32_t h_, t_; ENC_HT(v, h_, t_); table[h_] = (uint16_t)q; ENC_TAG_SET(h_, t_); }
}

// The table image of the last keep = min(len, 65536) bytes of dict: the seed steps without a seam position, from a zeroed table;
// then {keep, first position of the first seam step} as the header.  One wavefront.  Reads nothing behind the kept bytes.
__global__ __launch_bounds__(LZ4_WAVE) void k_hcdict_build_fast(uint8_t *fast, const uint8_t *dict, int len)
{
    __shared__ __attribute__((aligned(16))) uint16_t table[ENC_TABLE_ENTRIES];
    const int lane = lane_id();
    const int keep = min(max(len, 0), 65536);
    const uint8_t *from = dict + (len - keep);                          // (not dereferenced when keep == 0)
    dev_v4 *tab4 = (dev_v4 *)table;
    for (int i = lane; i < (int)(FASTDICT_TABLE_BYTES / 16); i += LZ4_WAVE) tab4[i] = dev_v4{0u, 0u, 0u, 0u};
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // the first seam position: the first entered position above keep - 5; its step and the ones behind it are the blocks' to replay
    const int qSeam = (max(keep - 4, 0) + ENC_SEED_STEP - 1) / ENC_SEED_STEP * ENC_SEED_STEP;
    const int seam0 = qSeam / ENC_SEED_SPAN * ENC_SEED_SPAN;
    for (int q0 = 0; q0 < seam0; q0 += ENC_SEED_SPAN) enc_seed_step<true>(table, from, q0, keep);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int i = lane; i < (int)(FASTDICT_TABLE_BYTES / 16); i += LZ4_WAVE) as_global((dev_v4 *)fast)[i] = tab4[i];
    if (lane == 0) as_global((dev_v4 *)(fast + FASTDICT_KEEP_OFF))[0] = dev_v4{(uint32_t)keep, (uint32_t)seam0, 0u, 0u};
}

void launch_hcdict_build_fast(uint8_t *fast, const uint8_t *dict, int len, hipStream_t s)
{
    hipLaunchKernelGGL(k_hcdict_build_fast, dim3(1), dim3(LZ4_WAVE), 0, s, fast, dict, len);
}

// ---- the window of a wave of the persistent grids (k_encode_fastdict, k_pages_fastdict, k_encode_fastdict_multi, k_encode_fstreams) ----
// Wave blockIdx.x owns stageStride bytes of a call's staging area; a dictionary ends, and the block behind it starts, at byte 65536 of them.
__device__ __forceinline__ uint8_t *enc_window_block_at(uint8_t *stage, size_t stageStride)
{
    return stage + (uint64_t)blockIdx.x * (uint64_t)stageStride + 65536;
}

// The window's head, in two small steps that a kernel calls in the order `keep, seam0, blockAt, dictionary` (one helper for all
// of it -- by value, by reference, or with blockAt in its result -- moved the instructions of k_encode_fastdict, which then ran 1 to
// 1.6 % slower: docs/MEASUREMENT_LOG.md section 24).  Word i of the header of the table image `fast`, {keep, first position of the
// first seam step}: neither above 65536, whatever the image holds ...
__device__ __forceinline__ int enc_window_header(const uint8_t *fast, int i)
{
    return (int)min(ex_uni(as_global((const uint32_t *)(fast + FASTDICT_KEEP_OFF))[i]), 65536u);
}
// ... and the kept bytes of `image`, laid so that they end at blockAt.
__device__ __forceinline__ void enc_window_dict(uint8_t *blockAt, const uint8_t *image, int keep)
{
    if (keep > 0) wave_copy_bytes(blockAt - keep, image + HCDICT_DICT_OFF, (uint32_t)keep);
}

// The prepared window of one block (or of one page's slice) of n >= 13 bytes at src, against a dictionary of keep > 0 bytes: the
// bytes go behind the kept ones, the table is the image again (the block before has written into it), and the seam steps are
// replayed against the staged bytes.  The caller then encodes at blockAt with keep bytes of dictionary.  (The decision stays with
// the caller -- `if (n >= 13 && keep > 0) { prepare; src = blockAt; dictLen = keep; } else if (n >= 13) clear;` -- and the caller's
// tab4 and lane come in: docs/MEASUREMENT_LOG.md section 24 has what the other forms moved.)
__device__ __forceinline__ void enc_window_prepare(uint16_t *table, dev_v4 *tab4, int lane, uint8_t *blockAt, const uint8_t *fast,
                                                   const uint8_t *src, int n, int keep, int seam0)
{
    wave_copy_bytes(blockAt, src, (uint32_t)n);
    for (int i = lane; i < (int)(FASTDICT_TABLE_BYTES / 16); i += LZ4_WAVE) tab4[i] = as_global((const dev_v4 *)fast)[i];
    // the bytes -- and, behind a restaging, the dictionary's -- are read back by other lanes than wrote them, and the steps below
    // enter into the loaded table
    wave_fence();
    for (int q0 = seam0; q0 < keep; q0 += ENC_SEED_SPAN) enc_seed_step<false>(table, blockAt - keep, q0, keep);
}
// ... and without a dictionary: the block of a one-block linked call, from an empty table, where it lies.  (A block under 13 bytes
// is literals and needs neither window nor table.)
__device__ __forceinline__ void enc_window_clear(dev_v4 *tab4, int lane)
{
    for (int i = lane; i < (int)(FASTDICT_TABLE_BYTES / 16); i += LZ4_WAVE) tab4[i] = dev_v4{0u, 0u, 0u, 0u};
}

// A persistent grid of single waves, k_encode's occupancy, one window of x.stage per wave.  The kept bytes go into the window once
// (enc_window_dict).  For every block of 13 bytes and more the wave prepares the window (enc_window_prepare) and runs
// encode_block_wave<.., PREP> on the staged bytes as the linked call would on its own; the output goes straight to the slot.
// Shorter blocks, and every block of an empty dictionary, are encoded where they lie.  A length outside 0..uniformLen gives
// framedLen 0 and leaves the slot alone.  Nothing of the object is written.
template <bool PAIR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ENC_WAVES_PER_EU, ENC_WAVES_PER_EU))) void k_encode_fastdict(FastDictArgs x)
{
    __shared__ __attribute__((aligned(16))) uint16_t table[ENC_TABLE_ENTRIES + ENC_LDS_PAD + ((PAIR && ENC_STAGE) ? 128 : 0)];
    const int lane = lane_id();
    const EncodeArgs a = x.e;
    const int keep = enc_window_header(x.fast, 0), seam0 = enc_window_header(x.fast, 1);
    uint8_t *blockAt = enc_window_block_at(x.stage, x.stageStride);
    enc_window_dict(blockAt, x.image, keep);
    dev_v4 *tab4 = (dev_v4 *)table;
    for (int blk = (int)blockIdx.x; blk < a.nBlocks; blk += (int)gridDim.x) {
        const EncBlock b = enc_block(a, blk);
        const int n = uni(b.n);
        if (n < 0 || n > a.uniformLen) {
            if (lane == 0) a.framedLen[blk] = 0;
            continue;
        }
        const uint8_t *src = a.src + uni64((int64_t)b.off);
        uint8_t *slot = a.slots + (size_t)blk * a.slotStride;
        int dictLen = 0;
        if (n >= LZ4_MFLIMIT + 1 && keep > 0) {
            enc_window_prepare(table, tab4, lane, blockAt, x.fast, src, n, keep, seam0);
            src = blockAt;
            dictLen = keep;
        } else if (n >= LZ4_MFLIMIT + 1) enc_window_clear(tab4, lane);
        // (one call site: the encoder is inlined, and its scalar operands stay scalar)
        const int c = encode_block_wave<uint16_t, true, false, PAIR, true>(src, n, slot + a.headerKind, a.accel, table, a.stats, dictLen);
        enc_finish_slot(a, blk, slot, c, n, lane == 0);
    }
}

// the grid of a call: waves per CU (knob > 0; 0: FASTDICT_WAVES_DEFAULT) or waves in all (knob < 0), no more than blocks, and no
// more windows of stageStride bytes than FASTDICT_SCRATCH_MAX holds
int encode_fastdict_grid(int nBlocks, int knob, size_t stageStride)
{
    long long waves = knob < 0 ? -(long long)knob : (long long)(knob > 0 ? knob : FASTDICT_WAVES_DEFAULT) * hc_cu_count();
    const long long fit = (long long)(FASTDICT_SCRATCH_MAX / (stageStride ? stageStride : 1));
    if (waves > fit) waves = fit;
    if (waves > nBlocks) waves = nBlocks;
    return waves < 1 ? 1 : (int)waves;
}

void launch_encode_fastdict(const FastDictArgs &a, int grid, hipStream_t s)
{
    if (a.e.nBlocks <= 0 || grid <= 0) return;
    if (a.e.uniformLen > 65536) hipLaunchKernelGGL((k_encode_fastdict<false>), dim3((unsigned)grid), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((k_encode_fastdict<true>), dim3((unsigned)grid), dim3(64), 0, s, a);
}

// ---------------------------------------------------------------------------
// K2, reference-exact compression (encode_exact.hpp, DESIGN.md 7d).  One wave per piece of a call, its hash table in LDS.
// ---------------------------------------------------------------------------
// canonical form of table entry v for a block (DESIGN 7d): the block's renorm applied, entries that no position of the
// block can use (below start - 65536) read 0
__device__ __forceinline__ uint32_t exact_canon(uint32_t v, uint32_t start, uint32_t delta)
{
    v = (v < delta) ? 0u : v - delta;
    return (start > 65536u && v < start - 65536u) ? 0u : v;
}

__device__ __forceinline__ dev_v4 exact_canon4(dev_v4 v, uint32_t start, uint32_t delta)
{
    return dev_v4{exact_canon(v.x, start, delta), exact_canon(v.y, start, delta), exact_canon(v.z, start, delta),
                  exact_canon(v.w, start, delta)};
}

// the byte range of block j of a call
__device__ __forceinline__ const uint8_t *exact_src(const EncodeArgs &e, int j)
{
    return e.src + enc_block(e, j).off;
}

// A slot's state (kernels.h, CSTREAM_*) into the wave: the table into LDS -- the caller's barrier comes behind it -- and the
// scalars; returns the end of the saved dictionary bytes.
__device__ __forceinline__ const uint8_t *exact_load_slot(dev_v4 *tab4, const uint8_t *st, uint32_t &cur, uint32_t &dictSize)
{
    const uint32_t *scal = (const uint32_t *)(st + CSTREAM_SCALAR_OFF);
    for (int i = lane_id(); i < EXACT_TABLE / 4; i += LZ4_WAVE) tab4[i] = as_global((const dev_v4 *)st)[i];
    cur = ex_uni(as_global(scal)[0]); dictSize = ex_uni(as_global(scal)[1]);
    return st + CSTREAM_DICT_OFF + ex_uni(as_global(scal)[2]);
}

// piece p = first + blockIdx.x owns blocks [p*P, min(p*P + P, n)).  Speculating (redo = 0), it starts R blocks early
// from a zeroed table, or from the stream's state at block 0 when the run-in reaches it (then it is exact by
// construction), and records assumed[p] at its first block.  Redoing, it starts at its first block from finalT[p-1].
// Either way it leaves finalT[p] and writes the slots, headers and framedLen of the blocks it owns.
__global__ __launch_bounds__(LZ4_WAVE) void k_exact_chain(ExactArgs x, int first, int redo)
{
    __shared__ dev_v4 tab4[EXACT_TABLE / 4];
    uint32_t *tab = (uint32_t *)tab4;
    const int lane = lane_id();
    const int p = first + (int)blockIdx.x;
    const int n = x.e.nBlocks;
    const int own0 = p * x.piece, own1 = min(own0 + x.piece, n);
    int start = own0;
    const uint32_t *init = nullptr;
    if (redo) init = x.finalT + (size_t)(p - 1) * EXACT_TABLE;
    else if (p == 0 || own0 - x.runin <= 0) { start = 0; init = x.state; }
    else start = own0 - x.runin;
    for (int i = lane; i < EXACT_TABLE / 4; i += LZ4_WAVE)
        tab4[i] = init ? as_global((const dev_v4 *)init)[i] : dev_v4{0u, 0u, 0u, 0u};
    __syncthreads();
    for (int j = start; j < own1; j++) {
        const ExactBlock m = x.meta[j];
        // LZ4_renormDictT, cbits/lz4.c:1545-1562.  finalT[p-1] is already block own0's table with its renorm applied
        // (exact_canon4(.., next.delta) below): a redo starts behind that renorm and must not apply it a second time.
        if (m.delta && !(redo && j == own0)) {
            for (int i = lane; i < EXACT_TABLE / 4; i += LZ4_WAVE) tab4[i] = exact_canon4(tab4[i], 0u, m.delta);
            __syncthreads();
        }
        if (!redo && j == own0 && p > 0) {
            dev_v4 *as = (dev_v4 *)(x.assumed + (size_t)p * EXACT_TABLE);
            for (int i = lane; i < EXACT_TABLE / 4; i += LZ4_WAVE) as_global(as)[i] = exact_canon4(tab4[i], m.start, 0u);
        }
        const bool write = j >= own0;
        const uint8_t *src = exact_src(x.e, j);
        const uint8_t *dictEnd = j > 0 ? exact_src(x.e, j - 1) + x.meta[j - 1].n : x.dict0 + x.dict0Len;
        uint8_t *slot = x.e.slots + (size_t)j * x.e.slotStride;
        const int cap = m.n + m.n / 255 + 16;                           // LZ4_compressBound
        int c;
        if (m.n == 0) c = enc_empty_block(slot + x.e.headerKind, write && lane == 0);
        else c = exact_encode_block(tab, src, m.n, dictEnd, m, (uint32_t)x.e.accel, slot + x.e.headerKind, cap, write);
        enc_finish_slot(x.e, j, slot, c, m.n, write && lane == 0);
        __syncthreads();
    }
    const ExactBlock next = x.meta[own1];
    dev_v4 *fin = (dev_v4 *)(x.finalT + (size_t)p * EXACT_TABLE);
    for (int i = lane; i < EXACT_TABLE / 4; i += LZ4_WAVE) as_global(fin)[i] = exact_canon4(tab4[i], next.start, next.delta);
}

// eq[p] = (finalT[p-1] == assumed[p]) for p = first + blockIdx.x (first >= 1)
__global__ __launch_bounds__(LZ4_WAVE) void k_exact_verify(ExactArgs x, int first)
{
    const int p = first + (int)blockIdx.x;
    const dev_v4 *f = (const dev_v4 *)(x.finalT + (size_t)(p - 1) * EXACT_TABLE);
    const dev_v4 *a = (const dev_v4 *)(x.assumed + (size_t)p * EXACT_TABLE);
    bool same = true;
    for (int i = lane_id(); i < EXACT_TABLE / 4; i += LZ4_WAVE) {
        const dev_v4 u = as_global(f)[i], v = as_global(a)[i];
        same = same && u.x == v.x && u.y == v.y && u.z == v.z && u.w == v.w;
    }
    const bool all = __ballot(!same) == 0;
    if (lane_id() == 0) x.eq[p] = all ? 1 : 0;
}

// the stream's state after the call: the last piece's table, and the last array's last bytes (the next call's dictionary)
__global__ __launch_bounds__(256) void k_exact_finish(ExactArgs x)
{
    const dev_v4 *fin = (const dev_v4 *)(x.finalT + (size_t)(x.nPieces - 1) * EXACT_TABLE);
    for (int i = (int)threadIdx.x; i < EXACT_TABLE / 4; i += (int)blockDim.x) as_global((dev_v4 *)x.state)[i] = as_global(fin)[i];
    const int last = x.e.nBlocks - 1;
    const int n = x.meta[last].n;
    const int keep = n < 65536 ? n : 65536;
    const uint8_t *from = exact_src(x.e, last) + (n - keep);
    for (int i = (int)threadIdx.x; i < keep; i += (int)blockDim.x) as_global(x.dictSave)[i] = as_global(from)[i];
}

void launch_exact_chain(const ExactArgs &a, int first, int count, int redo, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_exact_chain, dim3((unsigned)count), dim3(LZ4_WAVE), 0, s, a, first, redo);
}

void launch_exact_verify(const ExactArgs &a, int first, int count, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_exact_verify, dim3((unsigned)count), dim3(LZ4_WAVE), 0, s, a, first);
}

void launch_exact_finish(const ExactArgs &a, hipStream_t s)
{
    if (a.e.nBlocks <= 0) return;
    hipLaunchKernelGGL(k_exact_finish, dim3(1), dim3(256), 0, s, a);
}

// Many reference-exact streams in one call (mi355lz4_compress_streams_device, DESIGN.md 7e).  Wave w continues the stream
// in slot work[3w + 2] with the blocks [work[3w], work[3w + 1]) of the call: every stream starts from its own true state, so
// nothing is speculated.  The wave follows the scalars itself -- LZ4_compress_fast_continue's statements in front of the
// encoder (cbits/lz4.c:1565-1627), the ones exact_encode runs on the host for the single stream: wave-uniform, 32-bit.
// A length outside 0..maxBlockLen ends the stream's part of the call: that block and the ones behind it get framedLen 0,
// and the slot keeps the state after the last good block.
__global__ __launch_bounds__(LZ4_WAVE) void k_exact_streams(ExactStreamsArgs x)
{
    __shared__ dev_v4 tab4[EXACT_TABLE / 4];
    uint32_t *tab = (uint32_t *)tab4;
    const int lane = lane_id();
    const int32_t *w = x.work + 3 * (size_t)blockIdx.x;
    const int b0 = uni(w[0]), b1 = uni(w[1]);
    uint8_t *st = x.state + (size_t)uni(w[2]) * CSTREAM_SLOT_BYTES;
    uint8_t *dictSave = st + CSTREAM_DICT_OFF;
    uint32_t *scal = (uint32_t *)(st + CSTREAM_SCALAR_OFF);
    uint32_t cur, dictSize;
    const uint8_t *dictEnd = exact_load_slot(tab4, st, cur, dictSize);
    const uint8_t *lastSrc = nullptr;                                   // the last good array of the call: the next dictionary
    uint32_t lastN = 0;
    __syncthreads();
    for (int j = b0; j < b1; j++) {
        const int n = uni(enc_block(x.e, j).n);
        if (n < 0 || n > x.e.uniformLen) {
            for (int k = j + lane; k < b1; k += LZ4_WAVE) x.e.framedLen[k] = 0;
            break;
        }
        const ExactBlock m = exact_step(cur, dictSize, (uint32_t)n);
        if (m.delta) {                                                  // LZ4_renormDictT, cbits/lz4.c:1545-1562
            for (int i = lane; i < EXACT_TABLE / 4; i += LZ4_WAVE) tab4[i] = exact_canon4(tab4[i], 0u, m.delta);
            __syncthreads();
        }
        const uint8_t *src = exact_src(x.e, j);
        uint8_t *slot = x.e.slots + (size_t)j * x.e.slotStride;
        const int cap = n + n / 255 + 16;                               // LZ4_compressBound
        int c;
        if (n == 0) c = enc_empty_block(slot + x.e.headerKind, lane == 0);
        else c = exact_encode_block(tab, src, n, dictEnd, m, (uint32_t)x.e.accel, slot + x.e.headerKind, cap, true);
        enc_finish_slot(x.e, j, slot, c, n, lane == 0);
        dictEnd = src + n;
        lastSrc = src; lastN = (uint32_t)n;
        __syncthreads();
    }
    if (!lastSrc) return;                                               // no good block: the slot is as it was
    for (int i = lane; i < EXACT_TABLE / 4; i += LZ4_WAVE) as_global((dev_v4 *)st)[i] = tab4[i];
    const uint32_t keep = lastN < 65536u ? lastN : 65536u;              // (a zero-length last array: no dictionary)
    wave_copy_bytes(dictSave, lastSrc + (lastN - keep), keep);
    if (lane == 0) { as_global(scal)[0] = cur; as_global(scal)[1] = dictSize; as_global(scal)[2] = keep; }
}

void launch_exact_streams(const ExactStreamsArgs &a, int nWork, hipStream_t s)
{
    if (nWork <= 0) return;
    hipLaunchKernelGGL(k_exact_streams, dim3((unsigned)nWork), dim3(LZ4_WAVE), 0, s, a);
}

// LZ4_loadDict (cbits/lz4.c:1475-1515) on one slot of a mi355lz4_cstreams (mi355lz4_cstreams_load_dict, DESIGN.md 7i): one
// workgroup, the table in LDS.  The reference enters every third position p <= dictEnd - 8 of the last 64 KiB in ascending
// order, so a bucket keeps its last writer -- and the index p - (dictEnd - 65536) rises with p, so the last writer is the
// largest index: an LDS atomicMax over the zeroed table gives the same table whatever order the lanes run in.  (Index 0 --
// the first position of a full 64 KiB -- reads as "empty", as it does in the reference.)  Then the table, the scalars
// {currentOffset 65536, dictSize, saved bytes} and the slot's own copy of the bytes go out with vector stores.  Under 8 bytes
// (HASH_UNIT) the reference returns behind the reset and the offset: no dictionary, an empty table, currentOffset 65536.
#define LOAD_DICT_THREADS 256
__global__ __launch_bounds__(LOAD_DICT_THREADS) void k_cstreams_load_dict(uint8_t *st, const uint8_t *dict, int len)
{
    __shared__ dev_v4 tab4[EXACT_TABLE / 4];
    uint32_t *tab = (uint32_t *)tab4;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < EXACT_TABLE / 4; i += LOAD_DICT_THREADS) tab4[i] = dev_v4{0u, 0u, 0u, 0u};
    __syncthreads();
    const uint32_t keep = len < 8 ? 0u : ((uint32_t)len > 65536u ? 65536u : (uint32_t)len);
    const uint8_t *from = dict + ((uint32_t)len - keep);               // (not dereferenced when keep == 0)
    if (keep)                                                           // p + 8 <= keep: the last position is dictEnd - HASH_UNIT
        for (uint32_t p = 3u * tid; p + 8u <= keep; p += 3u * LOAD_DICT_THREADS)
            atomicMax(&tab[ex_hash5(from + p)], p + (65536u - keep));
    __syncthreads();
    for (uint32_t i = tid; i < EXACT_TABLE / 4; i += LOAD_DICT_THREADS) as_global((dev_v4 *)st)[i] = tab4[i];
    if (tid == 0) {
        LZ4_GLOBAL uint32_t *scal = as_global((uint32_t *)(st + CSTREAM_SCALAR_OFF));
        scal[0] = 65536u; scal[1] = keep; scal[2] = keep; scal[3] = 0u;
    }
    wg_copy_pieces(st + CSTREAM_DICT_OFF, from, keep, 16384u, tid / LZ4_WAVE, LOAD_DICT_THREADS / LZ4_WAVE);      // the bytes
}

void launch_cstreams_load_dict(uint8_t *slotState, const uint8_t *dict, int len, hipStream_t s)
{
    hipLaunchKernelGGL(k_cstreams_load_dict, dim3(1), dim3(LOAD_DICT_THREADS), 0, s, slotState, dict, len);
}

// A batch of blocks, each compressed on its own from a COPY of one slot's state (mi355lz4_compress_dict_device, DESIGN.md 7i):
// block blockIdx.x is what LZ4_compress_fast_continue writes on a copy of that LZ4_stream_t.  One wavefront per block; it
// loads the table and the scalars as k_exact_streams does, runs the statements in front of the encoder (cbits/lz4.c:1577-1627,
// the renorm included: the state is whatever the slot holds) and encodes with the slot's saved bytes as the dictionary.
// Nothing goes back to the slot, and no block sees another: the slot is shared, read-only state.
__global__ __launch_bounds__(LZ4_WAVE) void k_exact_dict(ExactDictArgs x)
{
    __shared__ dev_v4 tab4[EXACT_TABLE / 4];
    uint32_t *tab = (uint32_t *)tab4;
    const int lane = lane_id();
    const int j = (int)blockIdx.x;
    const int n = uni(enc_block(x.e, j).n);
    if (n < 0 || n > x.e.uniformLen) {
        if (lane == 0) x.e.framedLen[j] = 0;
        return;
    }
    uint32_t cur, dictSize;                                             // (the copy's: what exact_step advances them to goes nowhere)
    const uint8_t *dictEnd = exact_load_slot(tab4, x.state, cur, dictSize);
    __syncthreads();
    const ExactBlock m = exact_step(cur, dictSize, (uint32_t)n);
    if (m.delta) {                                                      // LZ4_renormDictT, cbits/lz4.c:1545-1562
        for (int i = lane; i < EXACT_TABLE / 4; i += LZ4_WAVE) tab4[i] = exact_canon4(tab4[i], 0u, m.delta);
        __syncthreads();
    }
    uint8_t *slot = x.e.slots + (size_t)j * x.e.slotStride;
    const int cap = n + n / 255 + 16;                                   // LZ4_compressBound
    int c;
    if (n == 0) c = enc_empty_block(slot + x.e.headerKind, lane == 0);
    else c = exact_encode_block(tab, exact_src(x.e, j), n, dictEnd, m, (uint32_t)x.e.accel, slot + x.e.headerKind, cap, true);
    enc_finish_slot(x.e, j, slot, c, n, lane == 0);
}

void launch_exact_dict(const ExactDictArgs &a, hipStream_t s)
{
    if (a.e.nBlocks <= 0) return;
    hipLaunchKernelGGL(k_exact_dict, dim3((unsigned)a.e.nBlocks), dim3(LZ4_WAVE), 0, s, a);
}

// ---------------------------------------------------------------------------
// K2, small batches: several waves per block (encode_wave.hpp, SEG).  One wavefront per block cannot be faster than
// one block (1.5 ms for 64 KiB), however empty the chip is: a call of 160 blocks -- the reference's own benchmark
// protocol, 10 MiB per file -- left 97 % of it idle, and 16 arrays of 640 KiB took 51 ms.  Here a block is cut into
// segments; wave (b, j) seeds its table from the bytes in front of segment j (what linked compression does between
// blocks) and writes sequence records; k_emit_seg then stitches a block's lists into one valid LZ4 block: a segment's
// trailing literals simply become the first literals of the next segment's first sequence.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ENC_WAVES_PER_EU, ENC_WAVES_PER_EU))) void k_encode_seg(EncodeSegArgs a)
{
    __shared__ uint16_t table[ENC_TABLE_ENTRIES + ENC_LDS_PAD];
    const int blk = (int)(blockIdx.x / (unsigned)a.segs), j = (int)(blockIdx.x % (unsigned)a.segs);
    const EncBlock b = enc_block(a.e, blk);
    const int n = b.n;
    uint32_t count = 0;
    if (n > 0) {
        const int s0 = min(n, j * a.segLen), s1 = (j == a.segs - 1) ? n : min(n, (j + 1) * a.segLen);
        if (s1 > s0) {
            SegOut so;
            so.list = a.lists + (size_t)blk * a.listStride + (size_t)(s0 / 4 + j);     // a segment has at most len/4 + 1 records
            so.count = 0;
            const int dictLen = min(s0, 65536);
            so.base = s0 - dictLen;
            so.last = s1 >= n;
            so.tail = n - s1;
            (void)encode_block_wave<uint16_t, true, true>(a.e.src + b.off + s0, s1 - s0, nullptr, a.e.accel, table, a.e.stats, dictLen, &so);
            count = so.count;
        }
    }
    if (lane_id() == 0) a.segCount[(size_t)blk * a.segs + j] = count;
}

// Emission of a segmented block, every segment by a wave of its own, in two steps: k_seg_sizes measures what each
// segment's records come to in bytes (a segment's first sequence takes its literals from where the last sequence
// BEFORE the segment ends), k_emit_seg places every segment behind the ones in front of it.  (One wave per block did
// this in round 3's first version: 8 ms for a 4 MiB block.)
__device__ __forceinline__ int seg_prev_end(const EncodeSegArgs &a, int blk, int j, int n)
{
    // end of the last sequence in front of segment j (0 when there is none)
    for (int i = j - 1; i >= 0; i--) {
        const int cnt = (int)a.segCount[(size_t)blk * a.segs + i];
        if (cnt > 0) {
            const int s0 = min(n, i * a.segLen);
            int start, len, mo;
            seg_unpack(a.lists[(size_t)blk * a.listStride + (size_t)(s0 / 4 + i) + (size_t)(cnt - 1)], start, len, mo);
            return start + len;
        }
    }
    return 0;
}

__global__ __launch_bounds__(64) void k_seg_sizes(EncodeSegArgs a)
{
    const int blk = (int)(blockIdx.x / (unsigned)a.segs), j = (int)(blockIdx.x % (unsigned)a.segs);
    const int lane = lane_id();
    // (the length written out, not enc_block(a.e, blk).n: with the helper this kernel takes 36 scalar registers where the parent's took 32)
    const int n = a.e.srcLen ? a.e.srcLen[blk] : a.e.uniformLen;
    const int cnt = (n > 0) ? (int)a.segCount[(size_t)blk * a.segs + j] : 0;
    const int s0 = min(max(n, 0), j * a.segLen);
    const uint64_t *list = a.lists + (size_t)blk * a.listStride + (size_t)(s0 / 4 + j);
    int prevEnd = (n > 0) ? seg_prev_end(a, blk, j, n) : 0;
    const int prev0 = prevEnd;
    uint32_t bytes = 0;
    for (int i0 = 0; i0 < cnt; i0 += LZ4_WAVE) {
        const int k = min(LZ4_WAVE, cnt - i0);
        int start = 0, len = 0, mo = 0;
        if (lane < k) seg_unpack(list[i0 + lane], start, len, mo);
        const int end = start + len;
        int qPrev = __builtin_amdgcn_update_dpp(prevEnd, end, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        if (lane == 0) qPrev = prevEnd;
        const uint32_t lit = (uint32_t)(start - qPrev), mc = (uint32_t)(len - LZ4_MINMATCH);
        const uint32_t esz = (lane < k) ? 1u + lit + ext_len_bytes(lit) + 2u + ext_len_bytes(mc) : 0u;
        bytes += (uint32_t)__builtin_amdgcn_readlane(enc_scan_incl((int)esz), 63);
        prevEnd = __builtin_amdgcn_readlane(end, k - 1);
    }
    if (lane == 0) {
        a.segBytes[(size_t)blk * a.segs + j] = bytes;
        a.segPrevEnd[(size_t)blk * a.segs + j] = prev0;
    }
}

__global__ __launch_bounds__(64) void k_emit_seg(EncodeSegArgs a)
{
    const int blk = (int)(blockIdx.x / (unsigned)a.segs), j = (int)(blockIdx.x % (unsigned)a.segs);
    const int lane = lane_id();
    const EncBlock b = enc_block(a.e, blk);
    const int n = b.n;
    uint8_t *slot = a.e.slots + (size_t)blk * a.e.slotStride;
    uint8_t *op0 = slot + a.e.headerKind;
    const uint8_t *src = a.e.src + b.off;
    const bool lastSeg = j == a.segs - 1;
    if (n <= 0) {
        const int c = (n == 0) ? enc_empty_block(op0, lastSeg && lane == 0) : 0;
        enc_finish_slot(a.e, blk, slot, c, n, lastSeg && lane == 0);
        return;
    }
    // where this segment's bytes go: behind the segments in front of it (at most 64: one per lane)
    const uint32_t mine = (lane < j) ? a.segBytes[(size_t)blk * a.segs + lane] : 0u;
    const uint32_t before = (uint32_t)__builtin_amdgcn_readlane(enc_scan_incl((int)mine), 63);
    uint8_t *op = op0 + before;
    const int cnt = (int)a.segCount[(size_t)blk * a.segs + j];
    const int s0 = min(n, j * a.segLen);
    const uint64_t *list = a.lists + (size_t)blk * a.listStride + (size_t)(s0 / 4 + j);
    int prevEnd = a.segPrevEnd[(size_t)blk * a.segs + j];
    for (int i0 = 0; i0 < cnt; i0 += LZ4_WAVE) {
        const int k = min(LZ4_WAVE, cnt - i0);
        int start = 0, len = 0, mo = 0;
        if (lane < k) seg_unpack(list[i0 + lane], start, len, mo);
        const int end = start + len;
        // my literals start where the sequence before me ends (lane 0: the one before this batch)
        int qPrev = __builtin_amdgcn_update_dpp(prevEnd, end, 0x138 /* wave_shr:1 */, 0xf, 0xf, false);
        if (lane == 0) qPrev = prevEnd;
        op = emit_sequences(src, op, qPrev, start, len, mo, k);
        prevEnd = __builtin_amdgcn_readlane(end, k - 1);
    }
    if (!lastSeg) return;
    // ---- the block's last segment: last literals (:1204-1231), header ----
    op = emit_last_literals(op, src + prevEnd, (uint32_t)(n - prevEnd));
    enc_finish_slot(a.e, blk, slot, (int)(op - op0), n, lane == 0);
}

void launch_encode_seg(const EncodeSegArgs &a, hipStream_t s)
{
    if (a.e.nBlocks <= 0) return;
    const dim3 grid((unsigned)a.e.nBlocks * (unsigned)a.segs);
    hipLaunchKernelGGL(k_encode_seg, grid, dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_seg_sizes, grid, dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_emit_seg, grid, dim3(64), 0, s, a);
}

// ---------------------------------------------------------------------------
// K2, fixed-size output pages (mi355lz4_compress_pages_device, encode_fill.hpp, DESIGN.md 7k).  One wavefront per input walks the
// input's chain: page k is what LZ4_compress_destSize (cbits/lz4.c:1382-1414) makes of the bytes behind what pages 0..k-1 took.
// Every page starts from a zeroed table, as the reference's LZ4_initStream gives it; the table's type and the mode are chosen per
// page from what remains (:1387-1394), so a long input's chain changes from byU32 to byU16 on its way.  The chain stops when the
// input is consumed, at maxPages pages, at a page that returns 0 (pageSize < 1: it is not written and not counted) and behind a
// page that took nothing (pageSize 1: a zero token).  A chain is serial: a call's parallelism is its number of inputs.
// A length outside 0..LZ4_MAX_INPUT_SIZE or a page that does not fit its stride: nPages[i] = 0 and nothing else.
// ---------------------------------------------------------------------------
// One input's chain (DESIGN.md 7k), for the three page kernels: input i of x checked, its pages made one behind the other by
// make(from, rem, dst, T, used) -> c -- the page of budget T over the rem > 0 bytes at `from`, written at dst; it sets used, the bytes
// the page took -- each recorded by lane 0 in its header words, pageCompLen and pageSrcLen, then nPages[i] and consumed[i].  A page
// that has nothing to take is the zero token and is made here: an empty input, and under ONE_IS_EMPTY (the wave encoder's pages) a
// budget of 1.  A length outside 0..LZ4_MAX_INPUT_SIZE or a page that does not fit its stride: nPages[i] = 0 and nothing else.
template <bool ONE_IS_EMPTY, class MakePage>
__device__ __forceinline__ void pages_walk(const PagesArgs x, int i, int lane, MakePage make)
{
    const int n = uni(x.srcLen[i]);
    const int T = uni(x.pageSize[i]);
    if (n < 0 || n > PAGES_MAX_INPUT || (T > 0 && (uint64_t)x.headerKind + (uint64_t)T > (uint64_t)x.pageStride)) {
        if (lane == 0) x.nPages[i] = 0;
        return;
    }
    const uint8_t *src = x.src + uni64((int64_t)x.srcOff[i]);
    const uint64_t first = (uint64_t)i * (uint64_t)x.maxPages;
    int pos = 0, k = 0;
    while (k < x.maxPages && T >= 1) {                                  // T < 1: the page returns 0, cbits/lz4.c:902, :1264
        const int rem = n - pos;
        uint8_t *page = x.pages + (first + (uint64_t)k) * (uint64_t)x.pageStride;
        uint8_t *dst = page + x.headerKind;
        int c, used = 0;
        if (rem == 0 || (ONE_IS_EMPTY && T == 1)) c = enc_empty_block(dst, lane == 0);     // :1263-1273: takes nothing
        else c = make(src + pos, rem, dst, T, used);
        if (lane == 0) {
            if (x.headerKind >= 4) store_le32(page, c);
            if (x.headerKind == 8) store_le32(page + 4, used);
            x.pageCompLen[first + (uint64_t)k] = c;
            x.pageSrcLen[first + (uint64_t)k] = used;
        }
        k++;
        pos += used;
        if (pos >= n || used == 0) break;
    }
    if (lane == 0) { x.nPages[i] = k; x.consumed[i] = pos; }
}

__global__ __launch_bounds__(LZ4_WAVE) void k_exact_pages(PagesArgs x)
{
    __shared__ dev_v4 tab4[EXACT_TABLE / 4];
    uint32_t *tab = (uint32_t *)tab4;
    const int lane = lane_id();
    pages_walk<false>(x, (int)blockIdx.x, lane, [&](const uint8_t *from, int rem, uint8_t *dst, int T, int &used) -> int {
        for (int j = lane; j < EXACT_TABLE / 4; j += LZ4_WAVE) tab4[j] = dev_v4{0u, 0u, 0u, 0u};
        __syncthreads();
        const bool fill = T < rem + rem / 255 + 16;                     // :1387, LZ4_compressBound
        int c;
        if (rem < FILL_64K_LIMIT) c = fill_encode_page<byU16>(tab, from, rem, dst, T, fill, used);      // :1390
        else c = fill_encode_page<byU32>(tab, from, rem, dst, T, fill, used);
        __syncthreads();
        return c;
    });
}

void launch_exact_pages(const PagesArgs &a, hipStream_t s)
{
    if (a.nInputs <= 0) return;
    hipLaunchKernelGGL(k_exact_pages, dim3((unsigned)a.nInputs), dim3(LZ4_WAVE), 0, s, a);
}

// ---------------------------------------------------------------------------
// K2, fast fixed-size output pages (mi355lz4_compress_pages_fast_device, DESIGN.md 7m).  The same chain, layout and stops (pages_walk);
// a page is made by the wave encoder with an output budget (encode_block_wave<.., BUDGET>): of the block that compress_batch_device
// writes for the next min(rem, 65536) bytes it holds the longest prefix of sequences that leaves room for a valid end, closed by the
// literal run that fills the page.  k_encode's occupancy and table, which the encoder zeroes per page.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ENC_WAVES_PER_EU, ENC_WAVES_PER_EU))) void k_pages_fast(PagesFastArgs y)
{
    __shared__ __attribute__((aligned(16))) uint16_t table[ENC_TABLE_ENTRIES + ENC_LDS_PAD + (ENC_STAGE ? 128 : 0)];
    const int lane = lane_id();
    pages_walk<true>(y.p, (int)blockIdx.x, lane, [&](const uint8_t *from, int rem, uint8_t *dst, int T, int &used) -> int {
        // (one call site: the encoder is inlined, and its scalar operands stay scalar)
        const int c = encode_block_wave<uint16_t, false, false, true, false, true>(from, min(rem, 65536), dst, y.accel, table, nullptr, 0,
                                                                                   nullptr, T, &used);
        wave_fence();                                                   // the next page zeroes the table this one read
        return c;
    });
}

void launch_pages_fast(const PagesFastArgs &a, hipStream_t s)
{
    if (a.p.nInputs <= 0) return;
    hipLaunchKernelGGL(k_pages_fast, dim3((unsigned)a.p.nInputs), dim3(64), 0, s, a);
}

// ---------------------------------------------------------------------------
// K2, fast fixed-size output pages against a prepared dictionary (mi355lz4_compress_pages_fastdict_device, DESIGN.md 7n).
// The persistent grid of single waves and the windows of k_encode_fastdict (enc_window_*), and pages_walk per input.  A page of 13
// input bytes and more has the next min(rem, 65536) bytes prepared in the window and runs encode_block_wave<.., DICT, PREP, BUDGET>:
// of the block that compress_fastdict_device writes for those bytes it holds the leading sequences whose cuts are all valid, closed
// by the literal run that fills the page.  Shorter remainders, and every page of an empty dictionary, are encoded where they lie.
// Nothing of the object is written.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ENC_WAVES_PER_EU, ENC_WAVES_PER_EU))) void k_pages_fastdict(PagesFastDictArgs y)
{
    __shared__ __attribute__((aligned(16))) uint16_t table[ENC_TABLE_ENTRIES + ENC_LDS_PAD + (ENC_STAGE ? 128 : 0)];
    const int lane = lane_id();
    const int keep = enc_window_header(y.fast, 0), seam0 = enc_window_header(y.fast, 1);
    uint8_t *blockAt = enc_window_block_at(y.stage, y.stageStride);
    enc_window_dict(blockAt, y.image, keep);
    dev_v4 *tab4 = (dev_v4 *)table;
    for (int i = (int)blockIdx.x; i < y.p.nInputs; i += (int)gridDim.x) {
        pages_walk<true>(y.p, i, lane, [&](const uint8_t *from, int rem, uint8_t *dst, int T, int &used) -> int {
            const int m = min(rem, 65536);
            int dictLen = 0;
            if (m >= LZ4_MFLIMIT + 1 && keep > 0) {
                enc_window_prepare(table, tab4, lane, blockAt, y.fast, from, m, keep, seam0);
                from = blockAt;
                dictLen = keep;
            } else if (m >= LZ4_MFLIMIT + 1) enc_window_clear(tab4, lane);
            // (one call site: the encoder is inlined, and its scalar operands stay scalar)
            const int c = encode_block_wave<uint16_t, true, false, true, true, true>(from, m, dst, y.accel, table, nullptr, dictLen, nullptr, T, &used);
            wave_fence();                                               // the next page reloads the table and the window this one read
            return c;
        });
    }
}

void launch_pages_fastdict(const PagesFastDictArgs &a, int grid, hipStream_t s)
{
    if (a.p.nInputs <= 0 || grid <= 0) return;
    hipLaunchKernelGGL(k_pages_fastdict, dim3((unsigned)grid), dim3(64), 0, s, a);
}

// ---------------------------------------------------------------------------
// K2, the wave encoder against a SET of prepared dictionaries (mi355lz4_compress_fastdict_multi_device, DESIGN.md 7o): block i
// names member dictIdx[i] of a mi355lz4_dictset, or -1 for none.  A wave that met its blocks in call order would restage up to
// 64 KiB of dictionary for every block, so the blocks are grouped by member first and a wave takes a contiguous range of the
// grouped order: it stages once, and once more per group boundary inside its range.
//
// The grouping pass: bins {-1, 0 .. nDicts - 1, anything else}; a histogram with global atomics, an exclusive scan by one
// workgroup, a scatter through the scanned counts as per-group cursors.  Not stable, and it need not be: a block's bytes do not
// depend on where it runs.  Nothing of it is read on the host.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int dictset_bin(int k, int nDicts) { return (k < -1 || k >= nDicts) ? nDicts + 1 : k + 1; }

// zeroed counts and stagings, and the waves' ranges of order[]: wave w takes [range[w], range[w + 1]) = [w * nBlocks / grid, ..)
__global__ __launch_bounds__(256) void k_dictset_zero(FastDictMultiArgs x, int grid)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i < x.nDicts + 2) x.bins[i] = 0u;
    if (i <= grid) x.range[i] = (int32_t)((int64_t)i * x.e.nBlocks / grid);
    if (i == 0) { x.last[0] = 0u; x.last[1] = (uint32_t)grid; }
}

__global__ __launch_bounds__(256) void k_dictset_hist(FastDictMultiArgs x)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i < x.e.nBlocks) atomicAdd(&x.bins[dictset_bin(x.dictIdx[i], x.nDicts)], 1u);
}

// counts -> first positions, in place: thread t sums a run of bins, the runs' sums are scanned in LDS
#define DICTSET_SCAN_THREADS 1024
__global__ __launch_bounds__(DICTSET_SCAN_THREADS) void k_dictset_scan(FastDictMultiArgs x)
{
    __shared__ uint32_t part[DICTSET_SCAN_THREADS];
    const int t = (int)threadIdx.x, nBins = x.nDicts + 2;
    const int per = (nBins + DICTSET_SCAN_THREADS - 1) / DICTSET_SCAN_THREADS;
    const int lo = min(t * per, nBins), hi = min(lo + per, nBins);
    uint32_t sum = 0;
    for (int i = lo; i < hi; i++) sum += x.bins[i];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < DICTSET_SCAN_THREADS; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t at = part[t] - sum;
    for (int i = lo; i < hi; i++) { const uint32_t c = x.bins[i]; x.bins[i] = at; at += c; }
}

__global__ __launch_bounds__(256) void k_dictset_scatter(FastDictMultiArgs x)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= x.e.nBlocks) return;
    const uint32_t at = atomicAdd(&x.bins[dictset_bin(x.dictIdx[i], x.nDicts)], 1u);
    if (at < (uint32_t)x.e.nBlocks) x.order[at] = i;                   // (always: the counts sum to nBlocks)
}

void launch_dictset_group(const FastDictMultiArgs &a, int grid, hipStream_t s)
{
    if (a.e.nBlocks <= 0) return;
    const unsigned perBlock = (unsigned)((a.e.nBlocks + 255) / 256), perBin = (unsigned)((max(a.nDicts + 2, grid + 1) + 255) / 256);
    hipLaunchKernelGGL(k_dictset_zero, dim3(perBin), dim3(256), 0, s, a, grid);
    hipLaunchKernelGGL(k_dictset_hist, dim3(perBlock), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_dictset_scan, dim3(1), dim3(DICTSET_SCAN_THREADS), 0, s, a);
    hipLaunchKernelGGL(k_dictset_scatter, dim3(perBlock), dim3(256), 0, s, a);
}

// The grid, occupancy and windows of k_encode_fastdict (enc_window_*), and a call site of its own.  Wave w takes order[w * nBlocks / grid, (w + 1) * nBlocks / grid) (x.range) and
// remembers which member its window holds (`held`; -1: none, which needs no window; -2: nothing yet).  When the next block names another member the
// wave reads that member's {keep, seam0} and copies its kept bytes so that they end at byte 65536 of the window -- in front of the
// block copy and of the fence that orders both against the reads.  A shorter dictionary behind a longer one leaves stale bytes in
// front of blockAt - keep: the seam steps read from blockAt - keep on, and the encoder takes src - dictLen as position 0 and never
// forms a candidate below it (tab_candidate).  Every (re)staging counts in x.last[0].  An index outside -1 .. nDicts - 1 or a
// length outside 0..uniformLen gives framedLen 0 and leaves the slot alone.  Nothing of any member is written.
template <bool PAIR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ENC_WAVES_PER_EU, ENC_WAVES_PER_EU))) void k_encode_fastdict_multi(FastDictMultiArgs x)
{
    __shared__ __attribute__((aligned(16))) uint16_t table[ENC_TABLE_ENTRIES + ENC_LDS_PAD + ((PAIR && ENC_STAGE) ? 128 : 0)];
    const int lane = lane_id();
    const EncodeArgs a = x.e;
    const int j0 = min(max(uni(x.range[blockIdx.x]), 0), a.nBlocks), j1 = min(max(uni(x.range[blockIdx.x + 1u]), j0), a.nBlocks);
    uint8_t *blockAt = enc_window_block_at(x.stage, x.stageStride);
    int held = -2, keep = 0, seam0 = 0;                                 // (-2: nothing yet, so the first block counts as a staging)
    const uint8_t *fast = nullptr;
    dev_v4 *tab4 = (dev_v4 *)table;
    for (int j = j0; j < j1; j++) {
        const int blk = uni(x.order[j]);
        if ((unsigned)blk >= (unsigned)a.nBlocks) continue;             // (never: the grouping pass wrote a permutation)
        const int k = uni(x.dictIdx[blk]);
        const EncBlock b = enc_block(a, blk);
        const int n = uni(b.n);
        if (k < -1 || k >= x.nDicts || n < 0 || n > a.uniformLen) {
            if (lane == 0) a.framedLen[blk] = 0;
            continue;
        }
        // (what the wave carries from block to block is wave-uniform, but the lane-0 store above joins the loop's back edge, and a
        // value that lives across such a join counts as divergent: said again here, they stay scalar operands of the encoder)
        held = uni(held); keep = uni(keep); seam0 = uni(seam0);
        fast = (const uint8_t *)(uintptr_t)uni64((int64_t)(uintptr_t)fast);
        if (k != held) {
            keep = 0; seam0 = 0; fast = nullptr;
            if (k >= 0) {
                const DictSetEntry m = x.set[k];
                fast = (const uint8_t *)(uintptr_t)uni64((int64_t)(uintptr_t)m.fast);
                const uint8_t *image = (const uint8_t *)(uintptr_t)uni64((int64_t)(uintptr_t)m.image);
                keep = enc_window_header(fast, 0); seam0 = enc_window_header(fast, 1);
                enc_window_dict(blockAt, image, keep);
            }
            held = k;
            if (lane == 0) atomicAdd(&x.last[0], 1u);
        }
        const uint8_t *src = a.src + uni64((int64_t)b.off);
        uint8_t *slot = a.slots + (size_t)blk * a.slotStride;
        int dictLen = 0;
        if (n >= LZ4_MFLIMIT + 1 && keep > 0) {
            enc_window_prepare(table, tab4, lane, blockAt, fast, src, n, keep, seam0);
            src = blockAt;
            dictLen = keep;
        } else if (n >= LZ4_MFLIMIT + 1) enc_window_clear(tab4, lane);
        // (one call site of an instantiation of its own -- SITE 1, encode_wave.hpp: the encoder is inlined, and its scalar operands
        // stay scalar, here and in k_encode_fastdict)
        const int c = encode_block_wave<uint16_t, true, false, PAIR, true, false, 1>(src, n, slot + a.headerKind, a.accel, table, a.stats, dictLen);
        enc_finish_slot(a, blk, slot, c, n, lane == 0);
    }
}

void launch_encode_fastdict_multi(const FastDictMultiArgs &a, int grid, hipStream_t s)
{
    if (a.e.nBlocks <= 0 || grid <= 0) return;
    if (a.e.uniformLen > 65536) hipLaunchKernelGGL((k_encode_fastdict_multi<false>), dim3((unsigned)grid), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((k_encode_fastdict_multi<true>), dim3((unsigned)grid), dim3(64), 0, s, a);
}

// ---------------------------------------------------------------------------
// K2, many fast linked streams continued across calls (mi355lz4_compress_streams_fast_device, DESIGN.md 7p).  Under DICT the wave
// encoder seeds its table from the dictionary's bytes, so block k of a stream depends on the last 64 KiB of block k - 1, on itself
// and on accel, and on nothing else: every block of every stream of a call is compressed at once, as the second block of the
// linked call [D, block], where D is the tail of the block before it -- the slot's bytes for a stream's first block of the call.
// Three launches, one behind the other: the plan reads the lengths, the encoder reads the slots, k_fstreams_save writes them.
// ---------------------------------------------------------------------------
// Entry w of x.work, one wavefront: good[w] = the stream's first block of the call whose length lies outside 0..uniformLen, or its
// end block -- that block and the ones behind it are not compressed -- and blockStream[b] = w for its blocks.
__global__ __launch_bounds__(LZ4_WAVE) void k_fstreams_plan(FStreamsArgs x)
{
    const int lane = lane_id();
    const int w = (int)blockIdx.x;
    const int32_t *e = x.work + 3 * (size_t)w;
    const int b0 = min(max(uni(e[0]), 0), x.e.nBlocks), b1 = min(max(uni(e[1]), b0), x.e.nBlocks);
    int good = b1;
    for (int j0 = b0; j0 < b1; j0 += LZ4_WAVE) {
        const int j = j0 + lane;
        bool bad = false;
        if (j < b1) {
            const int n = enc_block(x.e, j).n;
            bad = n < 0 || n > x.e.uniformLen;
            x.blockStream[j] = w;
        }
        const uint64_t m = __ballot(bad);
        if (m && good == b1) good = j0 + (int)__builtin_ctzll(m);
    }
    if (lane == 0) x.good[w] = good;
}

// The persistent grid of single waves, occupancy and windows of k_encode_fastdict (enc_window_block_at), over all blocks of the call.  A block at or behind
// its stream's good[] gets framedLen 0 and nothing else.  A block under 13 bytes is literals, and one with an empty D is the block
// of a one-block linked call: both are encoded where they lie.  So is a block whose D ends exactly where it starts -- the block
// before it in the call, when the caller's arrays are contiguous.  Every other block is staged: D so that it ends at byte 65536 of
// the wave's window, the block behind it.  The encoder zeroes and seeds its table itself, as in the linked call (not PREP).
// The slots are only read here.
template <bool PAIR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(ENC_WAVES_PER_EU, ENC_WAVES_PER_EU))) void k_encode_fstreams(FStreamsArgs x)
{
    __shared__ __attribute__((aligned(16))) uint16_t table[ENC_TABLE_ENTRIES + ENC_LDS_PAD + ((PAIR && ENC_STAGE) ? 128 : 0)];
    const int lane = lane_id();
    const EncodeArgs a = x.e;
    uint8_t *blockAt = enc_window_block_at(x.stage, x.stageStride);
    for (int blk = (int)blockIdx.x; blk < a.nBlocks; blk += (int)gridDim.x) {
        const int w = min(max(uni(x.blockStream[blk]), 0), x.nWork - 1);
        const int32_t *e = x.work + 3 * (size_t)w;
        const int b0 = uni(e[0]);
        if (blk >= uni(x.good[w])) {
            if (lane == 0) a.framedLen[blk] = 0;
            continue;
        }
        const EncBlock b = enc_block(a, blk);
        const int n = min(max(uni(b.n), 0), a.uniformLen);              // (inside already: the block is in front of good[w])
        const uint8_t *src = a.src + uni64((int64_t)b.off);
        uint8_t *slot = a.slots + (size_t)blk * a.slotStride;
        int dictLen = 0;
        if (n >= LZ4_MFLIMIT + 1) {
            const uint8_t *dEnd;                                        // D = [dEnd - dictLen, dEnd)
            if (blk <= b0) {                                            // the stream's first block of the call: what the slot holds
                const uint8_t *st = x.state + (size_t)uni(e[2]) * FSTREAM_SLOT_BYTES;
                dictLen = (int)min(ex_uni(as_global((const uint32_t *)(st + FSTREAM_COUNT_OFF))[0]), (uint32_t)FSTREAM_DICT_BYTES);
                dEnd = st + dictLen;
            } else {                                                    // the block before it (a good one: its length is inside)
                const EncBlock p = enc_block(a, blk - 1);
                const int pn = min(max(uni(p.n), 0), a.uniformLen);
                dictLen = min(pn, 65536);
                dEnd = a.src + uni64((int64_t)p.off) + pn;
            }
            if (dictLen > 0 && dEnd != src) {
                wave_copy_bytes(blockAt - dictLen, dEnd - dictLen, (uint32_t)dictLen);
                wave_copy_bytes(blockAt, src, (uint32_t)n);
                wave_fence();                                           // the bytes are read back by other lanes than wrote them
                src = blockAt;
            }
        }
        // (one call site of an instantiation of its own -- SITE 2, encode_wave.hpp: the encoder is inlined, and its scalar operands
        // stay scalar)
        const int c = encode_block_wave<uint16_t, true, false, PAIR, false, false, 2>(src, n, slot + a.headerKind, a.accel, table, a.stats, dictLen);
        enc_finish_slot(a, blk, slot, c, n, lane == 0);
        wave_fence();                                                   // the next block's staging overwrites the window this one read
    }
}

// Entry w of x.work, one workgroup, behind the encoder on the same stream -- a first block's read of the old tail cannot meet the
// write of the new one: the slot takes the last min(n, 65536) bytes of the stream's last good block of the call and their count
// (0 for an empty block: no dictionary).  No good block: the slot is as it was.
#define FSTREAMS_SAVE_THREADS 256
__global__ __launch_bounds__(FSTREAMS_SAVE_THREADS) void k_fstreams_save(FStreamsArgs x)
{
    const int w = (int)blockIdx.x;
    const int32_t *e = x.work + 3 * (size_t)w;
    const int b0 = max(uni(e[0]), 0), good = min(uni(x.good[w]), x.e.nBlocks);
    if (good <= b0) return;
    uint8_t *st = x.state + (size_t)uni(e[2]) * FSTREAM_SLOT_BYTES;
    const EncBlock b = enc_block(x.e, good - 1);
    const int n = min(max(uni(b.n), 0), x.e.uniformLen);
    const uint32_t keep = (uint32_t)min(n, FSTREAM_DICT_BYTES);
    const uint8_t *from = x.e.src + uni64((int64_t)b.off) + ((uint32_t)n - keep);
    wg_copy_pieces(st, from, keep, 4096u, threadIdx.x / LZ4_WAVE, FSTREAMS_SAVE_THREADS / LZ4_WAVE);
    if (threadIdx.x == 0) as_global((uint32_t *)(st + FSTREAM_COUNT_OFF))[0] = keep;
}

void launch_fstreams(const FStreamsArgs &a, int grid, hipStream_t s)
{
    if (a.e.nBlocks <= 0 || a.nWork <= 0 || grid <= 0) return;
    hipLaunchKernelGGL(k_fstreams_plan, dim3((unsigned)a.nWork), dim3(LZ4_WAVE), 0, s, a);
    if (a.e.uniformLen > 65536) hipLaunchKernelGGL((k_encode_fstreams<false>), dim3((unsigned)grid), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((k_encode_fstreams<true>), dim3((unsigned)grid), dim3(64), 0, s, a);
    hipLaunchKernelGGL(k_fstreams_save, dim3((unsigned)a.nWork), dim3(FSTREAMS_SAVE_THREADS), 0, s, a);
}

// ---------------------------------------------------------------------------
// K2, those streams at a set's level 1..12 (mi355lz4_fstreams_set_level, DESIGN.md 7q): the same plan and the same save around
// k_encode_hc_fstreams, the hash-chain encoder with k_encode_fstreams' windows.  That kernel alone is compiled apart
// (kernels_hstreams.hip says why); what is here is host code.
// ---------------------------------------------------------------------------
// the grid of a call: a workgroup per CU, or MI355LZ4_HSTREAMS_GROUPS of them (knob, clamped to 1..CUs; 0: not set), no more than
// blocks, and no more windows of stageStride bytes than FASTDICT_SCRATCH_MAX holds
int encode_hc_fstreams_grid(int nBlocks, int knob, size_t stageStride)
{
    long long groups = hc_cu_count();
    if (knob != 0) groups = min((long long)max(knob, 1), groups);
    const long long fit = (long long)(FASTDICT_SCRATCH_MAX / (stageStride ? stageStride : 1));
    if (groups > fit) groups = fit;
    if (groups > nBlocks) groups = nBlocks;
    return groups < 1 ? 1 : (int)groups;
}

void launch_fstreams_hc(const FStreamsArgs &a, int grid, int level, hipStream_t s)
{
    if (a.e.nBlocks <= 0 || a.nWork <= 0 || grid <= 0) return;
    const int depth = 1 << (min(max(level, 1), 9) - 1);
    hipLaunchKernelGGL(k_fstreams_plan, dim3((unsigned)a.nWork), dim3(LZ4_WAVE), 0, s, a);
    launch_encode_hc_fstreams(a, grid, depth, s);               // (k_encode_hc_fstreams, kernels_hstreams.hip)
    hipLaunchKernelGGL(k_fstreams_save, dim3((unsigned)a.nWork), dim3(FSTREAMS_SAVE_THREADS), 0, s, a);
}
