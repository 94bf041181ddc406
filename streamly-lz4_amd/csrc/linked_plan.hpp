// linked_plan.hpp -- the decisions of a device decode (api.cpp, decode_device_impl): which first pass runs and how a linked call is
// finished.  Pure functions of plain structs, no HIP: tests/native/host_san_test.cpp tabulates call shape -> path on the CPU.
#pragma once

#include <cstdint>
#include <cstdlib>

// How the last linked call was finished (mi355lz4_debug_runin_state, get[4]; the tests assert on the numbers)
enum class LinkedPath : int { None = 0, Runs = 1, RunIn = 2, RunInLong = 3, RunInGivenUp = 4, Pointer = 5, Big = 6 };
constexpr long BIG_KIB_DEFAULT = 512;      // big linked blocks from 512 KiB on: smaller blocks' ends still carry the wrong dictionary, pass after pass
constexpr int BIG_PASSES = 6;              // passes of the big-block form before the call is left to the passes behind it
constexpr int RUNIN_DEFAULT_64K = 11;      // run-in decode of long linked streams: blocks of 64 KiB of run-in ...
constexpr int RUNIN_MIN_SPAN = 9216;       // ... and the span (in 64 KiB) from which it is the default
constexpr int RUNIN_ROUNDS = 8;            // launches of pieces to be redone before the call is left to the pointer pass
constexpr int RUNIN_LONG_64K = 17;         // the long run-in (blocks of 64 KiB): taken after the default one gave a call up for what the data is like
constexpr int RUNIN_LONG_PROBE = 32;       // calls in a row finished with the long run-in before the default is tried again
constexpr int RUNIN_BACKOFF = 16;          // linked calls that skip the run-in decode after the long one gave a call up as well
// How long a stream remembers a missing dictionary is read off the DATA first (RuninState stays the second opinion): over 32 blocks of
// the span, the share of the bytes of a block's first 1024 sequences that matches take directly from the block before it (k_dict_share:
// tokens only, 0.1 ms; whole blocks give 0.065 / 0.077 where the heads give 0.29 / 0.32).  Measured (scripts/runin_share.py): the
// reference's linked text 0.291-0.292 (forgotten after 5 to 12 blocks: the default run-in), the engine's own 0.321-0.325 (9 to 15: the
// long one), Python sources by the reference 0.19, noise with a period just under 64 KiB 0.9 (never: pointer pass).  The two text
// writers are 10 % apart: a calibration on two generators, not a law; a stream on the wrong side costs what it cost before this rule.
constexpr double RUNIN_SHARE_LONG = 0.306;  // sampled share from which the long run-in is taken ...
constexpr double RUNIN_SHARE_NEVER = 0.60;  // ... and from which the stream is taken to never forget its dictionary (pointer pass)
// The MI355LZ4_* overrides (the tests reach every seam with them): read per call, CU_BLOCKS once per process; *Set: present at all
struct DecodeKnobs {
    int cuBlocks = -1;                           // CU_BLOCKS = n: the workgroup form for up to n blocks whatever their size, 0 = never
    long bigKiB = BIG_KIB_DEFAULT;               // LINKED_BIG: big blocks from this many KiB on, 0 = never
    bool asyncSet = false; int asyncCap = 0;     // LINKED_ASYNC = <largest decoded block size>: the asynchronous form
    bool runsSet = false; unsigned runMax = 4;   // LINKED_RUNS: longest run the short-runs walk takes (0 = never; the tests force it)
    bool runinSet = false; int runin = 0;        // LINKED_RUNIN: 0 = never, 1 = whenever it applies (the tests)
    int runinBlocks = 0, runinPiece = 0;         // LINKED_RUNIN_BLOCKS / _PIECE: blocks of run-in / per piece (> 0: forced)
    int runinSpin = 10000;                       // LINKED_RUNIN_SPIN: polls of k_runin_fix
    bool ptrSet = false; int ptr = 1;            // LINKED_PTR = 0: lists without source pointers
    bool poolSet = false; int poolMax = 16384;   // LINKED_POOL_BLOCKS: dependent blocks whose lists share the pool at a time (0: no lists)
    int ptrBlocks = 0;                           // LINKED_PTR_BLOCKS: blocks with source pointers at a time (> 0: forced)
    // what switches automatic choices off: PTR / POOL_BLOCKS the short-runs walk, + RUNS the run-in, + RUNIN / ASYNC the big blocks
    bool runsAuto() const { return !ptrSet && !poolSet; }
    bool runinAuto() const { return runsAuto() && !runsSet; }
    bool bigAuto() const { return runinAuto() && !runinSet && !asyncSet; }
};
inline DecodeKnobs read_decode_knobs()
{
    static const int cuBlocks = [] { const char *e = getenv("MI355LZ4_CU_BLOCKS"); return e ? atoi(e) : -1; }();
    DecodeKnobs k;
    k.cuBlocks = cuBlocks;
    const char *e;
    if ((e = getenv("MI355LZ4_LINKED_BIG"))) k.bigKiB = atol(e);
    if ((e = getenv("MI355LZ4_LINKED_ASYNC"))) { k.asyncSet = true; k.asyncCap = atoi(e); }
    if ((e = getenv("MI355LZ4_LINKED_RUNS"))) { k.runsSet = true; k.runMax = (unsigned)atoi(e); }
    if ((e = getenv("MI355LZ4_LINKED_RUNIN"))) { k.runinSet = true; k.runin = atoi(e); }
    if ((e = getenv("MI355LZ4_LINKED_RUNIN_BLOCKS"))) k.runinBlocks = atoi(e);
    if ((e = getenv("MI355LZ4_LINKED_RUNIN_PIECE"))) k.runinPiece = atoi(e);
    if ((e = getenv("MI355LZ4_LINKED_RUNIN_SPIN"))) k.runinSpin = atoi(e);
    if ((e = getenv("MI355LZ4_LINKED_PTR"))) { k.ptrSet = true; k.ptr = atoi(e); }
    if ((e = getenv("MI355LZ4_LINKED_POOL_BLOCKS"))) { k.poolSet = true; k.poolMax = atoi(e); }
    if ((e = getenv("MI355LZ4_LINKED_PTR_BLOCKS"))) k.ptrBlocks = atoi(e);
    return k;
}
// One device decode (the call shape): the caller's arrays and, for linked streams, what the call is part of
struct DecodeCall {
    const uint8_t *framed; uint64_t framedLen; const uint64_t *blockOff; int nBlocks; int headerKind; int fixedUncomp; int linked;
    uint8_t *out; const uint64_t *outOff; const int32_t *outCap; int32_t *result;
    const uint8_t *dict0 = nullptr; uint32_t dict0Len = 0;     // dictionary in force before block 0
    const int32_t *streamFirst = nullptr; int nStreams = 0;    // stream table (null: one stream)
    int lookBack = 0;                                          // blocks of the same stream in front of block 0
    bool splitOk = false, deferEnd = false;                    // mi355lz4_decompress_linked_begin
    const int32_t *target = nullptr;                           // mi355lz4_decompress_partial_device: bytes wanted per block (device memory)
};
// What the engine is set to: mi355lz4_set_decoder, mi355lz4_debug_stats, LINKED_ASYNC else mi355lz4_set_linked_async
struct EngineMode { int decoder = 0; bool stats = false; int asyncCap = 0; };
// The first pass's summary (linkStat[0..6]; asynchronous form: the whole call and the caller's bound): blocks that need their dictionary,
// the first and the last of them, the longest stream, the largest such block's capacity, the longest run without output, runs
struct LinkStat {
    uint32_t count = 0, first = 0, last = 0, longestStream = 0, maxCap = 0, longestRun = 0, runs = 0;
    static LinkStat from(const uint32_t *w) { return {w[0], w[1], w[2], w[3], w[4], w[5], w[6]}; }
    static LinkStat whole_call(int n, int cap) { return {(uint32_t)n, 0, (uint32_t)(n - 1), (uint32_t)n, (uint32_t)cap, 0, 0}; }
};
// Asynchronous form: one stream only (the streams call keeps the wait: its choice between walk and pointer pass needs the counts)
inline bool async_gate(const DecodeCall &d, const EngineMode &m) { return m.asyncCap > 0 && !d.streamFirst; }
// Whether a call of decoder variant 0 takes the workgroup-per-block decoder (decode_cu.hpp): a CU decodes a 64 KiB block in 0.09-0.11 ms
// where a wavefront takes 0.2-0.3, but 18 wavefronts shared a CU when this was measured (20 now, decode_par.hpp).  Measured (device-resident, ms, workgroup / wavefront form; lzsynth):
// 64 KiB blocks: 256: 0.10 / 0.20, 512: 0.20 / 0.21, 768: 0.29 / 0.21; 16 KiB: 256: 0.045 / 0.074, 512: 0.083 / 0.075; 4 KiB: 160: 0.042 /
// 0.037 (a workgroup's fixed costs are 28 us a block).  So: up to one block per CU when blocks are not tiny, up to two when they are big --
// judged by the compressed bytes per block, which is all the host knows.
inline bool cu_auto(const DecodeKnobs &k, int nBlocks, uint64_t framedLen)
{
    if (k.cuBlocks >= 0) return nBlocks <= k.cuBlocks;
    const uint64_t avg = framedLen / (uint64_t)(nBlocks > 0 ? nBlocks : 1);
    if (avg < 3072) return false;
    return nBlocks <= 256 || (nBlocks <= 512 && avg >= 16384);
}
// The first pass: one workgroup per block for calls that do not fill the GPU (cu_auto; variant 4 forces it: the tests).  A linked call's
// first pass is this same standalone decode (decompressChunks always asks for linked = 1, and this engine's compressor writes
// independent blocks): a block that needs its dictionary fails here as it does there -- 50 us later -- and is counted.
enum class FirstPass { Seq, Tok, Cu, Par };
inline FirstPass first_pass(const DecodeCall &d, const EngineMode &m, const DecodeKnobs &k)
{
    if (m.decoder == 1) return FirstPass::Seq;
    if (m.decoder == 3) return FirstPass::Tok;  // experiment builds only (the lane-parallel form when its scratch cannot be had)
    // A partial call's work is sum(min(target, capacity)), not the blocks' sizes, and the targets are device memory the call does not
    // read: 200 blocks of 64 KiB asked for 100 bytes each are 20 KB of work, a fraction of a segment per workgroup.  Variant 0 takes the
    // lane-parallel form, whose cost follows the prefix; variant 4 (the tests) the workgroup form, which hands every block its target
    // cuts short to the lane-parallel one (kernels/decode_partial.inc, k_decode_cu_partial).  There is no token-list form of it.
    if (d.target && m.decoder != 4) return FirstPass::Par;
    if (!m.stats && (m.decoder == 4 || (m.decoder == 0 && cu_auto(k, d.nBlocks, d.framedLen)))) return FirstPass::Cu;
    return FirstPass::Par;
}
// Big linked blocks (BlockMax1MB / 4MB streams, few enough for a CU each; api.cpp, linked_big): armed before the first launch, which then
// goes on with the path's pass 1, from half the path's block size of compressed bytes per block (a stream of blocks of half that size
// at a ratio of 2 would otherwise pay a pass it has no use for: +0.85 ms for 512 blocks of 256 KiB); else behind the wait (big_takes).
enum class BigArm { No, BeforeFirstPass, AfterWait };
inline BigArm big_arm(const DecodeCall &d, const EngineMode &m, const DecodeKnobs &k)
{
    const bool eligible = d.linked && k.bigKiB > 0 && k.bigAuto() && !d.streamFirst && !d.splitOk && !d.deferEnd && d.lookBack >= 0 &&
                          !d.dict0 && m.decoder == 0 && !m.stats && m.asyncCap <= 0 && d.nBlocks >= 2 && d.nBlocks <= 512 &&
                          cu_auto(k, d.nBlocks, d.framedLen);
    if (!eligible) return BigArm::No;
    return d.framedLen / (uint64_t)d.nBlocks >= (uint64_t)k.bigKiB * 1024u / 2u ? BigArm::BeforeFirstPass : BigArm::AfterWait;
}
inline bool big_takes(const DecodeKnobs &k, const LinkStat &st) { return (uint64_t)st.maxCap >= (uint64_t)k.bigKiB * 1024u; }
// Few dependent blocks, in short runs (api.cpp, linked_runs)
inline bool runs_take(const DecodeCall &d, const EngineMode &m, const DecodeKnobs &k, const LinkStat &st)
{
    return !d.streamFirst && !async_gate(d, m) && !d.splitOk && !d.deferEnd && k.runMax > 0 && st.longestRun >= 1 &&
           st.longestRun <= k.runMax && (k.runsSet || k.runsAuto());
}
// The run-in decode adapts to the engine's streams (the calls that follow one are, as a rule, more of the same)
struct RuninState {
    bool longRun = false;                   // a call was given up with the default run-in (chains of pieces to redo): the long one from here on
    int longOk = 0;                         // ... calls in a row that finished with it (after RUNIN_LONG_PROBE the default is tried again)
    int skip = 0;                           // ... and given up with the long one too: this many linked decodes go straight to the pointer pass
};
struct RuninPlan {
    bool use = false, longRun = false, sample = false;   // sample: the dictionary share is sampled first (runin_after_sample)
    uint64_t per64 = 1, stride = 65536, maxPieces = 0;   // the largest dependent block in 64 KiB (at least 1), a ring slot that size
    int runIn = 0, piece = 0, segBlocks = 0;     // blocks of run-in, per piece, per launch
};
// Step 1, before the share sample.  Every linked call that gets here decays the state (an engine whose later streams are shorter than
// the long run-in's threshold would otherwise never try the default again).  A range of _linked_begin with no seam to wait for
// (lookBack 0) is finished like a plain call.  At least 64 dependent blocks (a few huge ones have the bytes but not the pieces), strides
// of at most 1 GiB (a piece's ring is two).  The engine's own linked text forgets a dictionary after 9 to 15 blocks instead of 5 to 12
// (it takes half of a block from the block before it, the reference a third) and takes the long run-in, which pays from twice the span.
inline RuninPlan runin_plan(RuninState &st, const DecodeCall &d, const EngineMode &m, const DecodeKnobs &k, int span0, uint32_t maxCap)
{
    RuninPlan p;
    p.per64 = ((uint64_t)maxCap + 65535u) / 65536u > 0 ? ((uint64_t)maxCap + 65535u) / 65536u : 1u;
    p.stride = p.per64 * 65536u;
    if (!k.runinSet && st.longRun && ++st.longOk >= RUNIN_LONG_PROBE) { st.longRun = false; st.longOk = 0; }
    p.longRun = st.longRun && !k.runinSet;
    p.use = !d.streamFirst && !async_gate(d, m) && (!(d.splitOk || d.deferEnd) || d.lookBack == 0) &&
            (k.runinSet ? k.runin != 0
                        : (k.runinAuto() && span0 >= 64 && 2u * p.stride <= ((uint64_t)1 << 31) &&
                           (uint64_t)span0 * p.per64 >= (uint64_t)(p.longRun ? 2 * RUNIN_MIN_SPAN : RUNIN_MIN_SPAN)));
    if (p.use && !k.runinSet && st.skip > 0) { st.skip--; p.use = false; }
    p.sample = p.use && !k.runinSet;
    return p;
}
// Step 2: the sampled share (< 0: none), then the sizes.  Run-in length: on text the 5th to 12th block of 64 KiB is the first without a
// byte of the missing dictionary (scripts/runin_sim.py); bigger blocks carry it further in bytes -- 256 KiB: 4 blocks, 1 MiB: 2,
// measured.  Pieces: one wave slot each (256 CUs x 16 waves), and at most 2 GiB of rings.
inline void runin_after_sample(RuninPlan &p, const DecodeKnobs &k, int span0, double share)
{
    if (share >= 0) {
        if (share >= RUNIN_SHARE_NEVER) p.use = false;
        else if (share >= RUNIN_SHARE_LONG) p.longRun = true;
        if (p.longRun && (uint64_t)span0 * p.per64 < 2 * RUNIN_MIN_SPAN) p.use = false;
    }
    if (!p.use) return;
    const uint64_t run64 = p.longRun ? RUNIN_LONG_64K : RUNIN_DEFAULT_64K;
    p.runIn = k.runinBlocks > 0 ? k.runinBlocks : (p.per64 == 1 ? (int)run64 : (int)((run64 + p.per64) / p.per64) + 1);
    if (p.runIn > 64) p.runIn = 64;
    p.maxPieces = ((uint64_t)1 << 31) / (2u * p.stride);
    if (p.maxPieces < 1) p.maxPieces = 1;
    if (p.maxPieces > 4096) p.maxPieces = 4096;
    p.piece = (int)(((uint64_t)span0 + p.maxPieces - 1) / p.maxPieces);
    if (k.runinPiece > 0) p.piece = k.runinPiece;
    if (p.piece < 1) p.piece = 1;
    p.segBlocks = (int)((p.maxPieces * (uint64_t)p.piece < (uint64_t)span0) ? p.maxPieces * (uint64_t)p.piece : (uint64_t)span0);
}
// A segment the run-in did not finish (run.ctl[1]; a kernel that did not launch counts as a broken block).  Given up for what the DATA
// is like (chains of pieces to redo, rounds that do not end), not for a broken block: the engine's next calls take the long run-in,
// or -- that was the long one -- RUNIN_BACKOFF of them do not try.  A forced run-in teaches nothing.
inline void runin_given_up(RuninState &st, const RuninPlan &p, const DecodeKnobs &k, uint32_t why)
{
    if ((why & 1u) || k.runinSet) return;
    if (!p.longRun) st.longRun = true;
    else st.skip = RUNIN_BACKOFF;
    st.longOk = 0;
}
// Lists of deferred matches for up to `pool` dependent blocks at a time (one byte per output byte) and source pointers for up to `seg`
// (four bytes per output byte); without the lists the blocks are walked.  Sized for 64 KiB blocks: a bigger block takes a list region
// and pointers per 64 KiB (beyond 4 MiB it is walked).  Many short streams are walked side by side, one wavefront per stream: a walk
// costs ~0.42 ms per dependent block of the longest stream (up to ~5000 streams at a time), the pointer passes ~0.55 ms + 1.15 us per
// dependent block of the call (MI355X, text-like data).
struct PtrPlan {
    bool walkStreams = false, lists = false, usePtr = false;   // the pool of lists is asked for, and then the source pointers
    int per = 1, poolBlocks = 0, ptrBlocks = 0;  // list regions (64 KiB pieces) per block
    int pool = 0, seg = 0;                       // blocks per tolerant launch, per pointer segment (when the pointers are had; else pool)
    size_t ptrs = 0;                             // pointers of a segment
};
inline PtrPlan ptr_plan(const DecodeCall &d, const DecodeKnobs &k, const LinkStat &st, int span)
{
    PtrPlan p;
    p.walkStreams = d.streamFirst && !k.ptrSet &&
                    0.42 * (double)(st.longestStream > 0 ? st.longestStream - 1 : 0) * (double)(1 + d.nStreams / 5000) <
                        0.55 + 1.15e-3 * (double)st.count;
    p.per = (int)((st.maxCap + 65535u) / 65536u) > 0 ? (int)((st.maxCap + 65535u) / 65536u) : 1;
    p.poolBlocks = k.poolSet ? k.poolMax : (k.poolMax / p.per > 0 ? k.poolMax / p.per : 1);
    p.ptrBlocks = k.ptrBlocks > 0 ? k.ptrBlocks : (4096 / p.per > 0 ? 4096 / p.per : 1);
    p.lists = k.poolMax > 0 && !p.walkStreams;
    p.pool = p.lists ? ((span < p.poolBlocks) ? span : p.poolBlocks) : span;
    p.seg = (p.pool < p.ptrBlocks) ? p.pool : p.ptrBlocks;
    p.ptrs = ((size_t)p.seg + 1) * p.per * 65536 + 65536;
    p.usePtr = k.ptr != 0 && p.ptrs < ((size_t)1 << 31);
    return p;
}
// When one segment covers every dependent block, the half of the second pass that reads no output byte can be issued at once: lists,
// pointers and the first jump pass depend on the tokens only
inline bool linked_split(bool splitOk, bool havePtr, int span, int seg, int pool) { return splitOk && havePtr && span <= seg && span <= pool; }
