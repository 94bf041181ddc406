// kernels/linked_ptr.inc -- one long linked stream: the pointer passes (linked_ptr.hpp), the stream statistics and the second pass's launchers.
// A part of kernels.hip, the one device translation unit: included there, in this order, and not compiled on its own.
// ---- one long linked stream, data-parallel second pass (linked_ptr.hpp) ----
// Where the segment's pointer space starts in the output buffer: at the block before its first block (that
// block's output is the first block's dictionary), or at the first block when there is none.
__device__ __forceinline__ bool ptr_has_prev(const DecodeArgs &a) { return a.segFirst > 0 || a.lookBack > 0; }
__device__ __forceinline__ uint64_t ptr_lo(const DecodeArgs &a)
{
    return ptr_has_prev(a) ? a.outOff[a.segFirst - 1] : a.outOff[a.segFirst];
}
// The stream a block belongs to (index into ptr.bad[]; -1 = none: decoded on its own) and whether the block
// before it is its dictionary.  One stream: every block but the very first has one.
__device__ __forceinline__ int ptr_stream(const DecodeArgs &a, int blk, bool &hasDict)
{
    if (!a.streamFirst) { hasDict = blk > 0 || a.lookBack > 0; return 0; }
    auto first = [&](int s) { return min(max(a.streamFirst[s], 0), a.nBlocks); };
    hasDict = false;
    if (a.nStreams <= 0 || blk < first(0) || blk >= first(a.nStreams)) return -1;
    int lo = 0, hi = a.nStreams;                       // first(lo) <= blk < first(hi)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first(mid) <= blk) lo = mid; else hi = mid;
    }
    hasDict = blk > first(lo);
    return lo;
}
// a block the tolerant pass left a usable list for (stable while the second pass runs: result[] is not)
__device__ __forceinline__ bool ptr_listed(const DecodeArgs &a, int blk)
{
    return blk >= a.segFirst && blk < a.segEnd && a.tol.region[blk] >= 0 && a.tol.size[blk] > 0;
}
// decoded size of block blk as far as the second pass knows it, 0 = no output
__device__ __forceinline__ int ptr_size(const DecodeArgs &a, int blk)
{
    const int r = a.result[blk];
    if (r > 0) return r;
    return (is_codec_error(r) && ptr_listed(a, blk)) ? a.tol.size[blk] : 0;
}

// a dependent block the second pass is resolving: listed, and nothing in its stream was turned down
__device__ __forceinline__ bool ptr_taken(const DecodeArgs &a, int blk)
{
    if (!ptr_listed(a, blk) || !is_codec_error(a.result[blk])) return false;
    bool hd;
    const int sid = ptr_stream(a, blk, hd);
    return sid >= 0 && !a.ptr.bad[sid];
}

// Workgroup i >= 1: block segFirst + i - 1 writes the pointers of its own bytes -- self, then its deferred
// matches.  Workgroup 0: the bytes in front of the segment (caller's dictionary, block before the segment).
__global__ __launch_bounds__(256) void k_ptr_expand(DecodeArgs a)
{
    if (a.asyncGate && a.linkStat[0] == 0u) return;     // asynchronous linked decode: the first pass found nothing to do
    uint32_t *P = a.ptr.buf;
    const int tid = (int)threadIdx.x;
    const uint64_t lo = ptr_lo(a);
    if (blockIdx.x == 0) {
        uint32_t n = PTR_PRE;
        if (ptr_has_prev(a)) {
            const int rp = a.result[a.segFirst - 1];
            if (rp > 0) n += (uint32_t)rp;
        }
        n = (uint32_t)min((uint64_t)n, a.ptr.cap);      // (the first block checks its own range against the capacity)
        for (uint32_t i = (uint32_t)tid; i < n; i += 256u) P[i] = i | PTR_FINAL;
        return;
    }
    const int blk = a.segFirst + (int)blockIdx.x - 1;
    bool hasDict = false;
    const int sid = ptr_stream(a, blk, hasDict);
    auto fail = [&]() { if (tid == 0 && sid >= 0) atomicOr(&a.ptr.bad[sid], 1u); };
    const int r = a.result[blk];
    const bool listed = is_codec_error(r) && ptr_listed(a, blk);
    if (is_codec_error(r) && !listed) { fail(); return; }          // a dependent block without a list
    const int size = listed ? a.tol.size[blk] : r;
    if (size <= 0) return;                                          // no output: nobody points here
    if (a.outOff[blk] < lo) { fail(); return; }
    const uint64_t b64 = a.outOff[blk] - lo + PTR_PRE;
    if (b64 + (uint64_t)size > a.ptr.cap || b64 + (uint64_t)size >= (uint64_t)PTR_FINAL) { fail(); return; }
    const uint32_t bLo = (uint32_t)b64;
    if (!listed) {                                                  // a block that needed nothing: all roots
        for (uint32_t i = (uint32_t)tid; i < (uint32_t)size; i += 256u) P[bLo + i] = (bLo + i) | PTR_FINAL;
        return;
    }

    // the dictionary in force (cbits/lz4.c:2347-2355 with every block in its own allocation): the block before
    uint32_t dictEnd = PTR_PRE;                                     // pointer index one past the dictionary
    int dictLen = 0;
    if (hasDict) {
        const int ps = ptr_size(a, blk - 1);
        if (ps <= 0 || a.outOff[blk - 1] < lo) { fail(); return; } // dictionary further back, or none: serial walk
        dictEnd = (uint32_t)(a.outOff[blk - 1] - lo + PTR_PRE) + (uint32_t)ps;
        dictLen = ps;
    } else if (a.dict0 && !a.streamFirst) {
        dictLen = (int)a.dict0Len;
    }
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0;
    if (read_block_header(a, blk, data, compLen, cap) != 0) { fail(); return; }
    const TolEntry *list = (const TolEntry *)a.tol.pool + (size_t)a.tol.region[blk] * TOL_LIST_CAP;
    const int n = a.tol.count[blk];
    const int lane = tid & 63;
    bool bad = false;
    auto unpack = [](uint64_t w, int &dpos, int &ml, int &spos) { tol_unpack(w, dpos, ml, spos); };
    // The list is in stream order: destinations ascend and do not overlap.  Entry e writes the pointers of ITS range
    // of the block in one go: the clean bytes between the entry before it and itself (roots), then its own bytes.
    for (int e0 = 0; e0 < n; e0 += 256) {
        const int e = e0 + tid;
        int gs = 0, dpos = 0, ml = 0, spos = 0;
        if (e < n) {
            unpack(*(const uint64_t *)(list + e), dpos, ml, spos);
            if (e > 0) {
                int pd, pm, ps;
                unpack(*(const uint64_t *)(list + e - 1), pd, pm, ps);
                gs = pd + pm;
            }
            if (!(ml > 0 && spos < dpos && dpos + ml <= size && spos >= -dictLen && gs <= dpos)) bad = true;
            // a match that starts in the dictionary must end LASTLITERALS before the end of the output (:1884-1889)
            if (spos < 0 && dpos + ml > cap - LZ4_LASTLITERALS) bad = true;
            if (bad) { ml = 0; gs = dpos; }
        }
        // position x of the range: a root in front of dpos; behind it byte x - dpos of the match, which comes from
        // position spos + (x - dpos): in this block, or (negative) in the dictionary
        auto ptrAt = [&](int x, int d, int sp) -> uint32_t {
            if (x < d) return (bLo + (uint32_t)x) | PTR_FINAL;
            const int s1 = sp + (x - d);
            return (s1 >= 0) ? bLo + (uint32_t)s1 : dictEnd - (uint32_t)(-s1);
        };
        const int len = dpos + ml - gs;
        const int head = min(len, 8);
        for (int j = 0; j < head; j++) P[bLo + (uint32_t)(gs + j)] = ptrAt(gs + j, dpos, spos);
        for (uint64_t lm = __ballot(len > 8); lm; lm &= lm - 1) {  // the rest of a long range: by the whole wave
            const int k = (int)__builtin_ctzll(lm);
            const int kg = __builtin_amdgcn_readlane(gs, k), kd = __builtin_amdgcn_readlane(dpos, k);
            const int ks = __builtin_amdgcn_readlane(spos, k), kend = kd + __builtin_amdgcn_readlane(ml, k);
            for (int x = kg + 8 + lane; x < kend; x += LZ4_WAVE) P[bLo + (uint32_t)x] = ptrAt(x, kd, ks);
        }
    }
    {   // the clean bytes behind the last entry
        int tail = 0;
        if (n > 0) {
            int pd, pm, ps;
            unpack(*(const uint64_t *)(list + n - 1), pd, pm, ps);
            tail = min(pd + pm, size);
        }
        for (int x = tail + tid; x < size; x += 256) P[bLo + (uint32_t)x] = (bLo + (uint32_t)x) | PTR_FINAL;
    }
    if (__syncthreads_or(bad ? 1 : 0)) fail();
}

// Workgroup -> (block of the segment, part of the block) for the jump and fetch passes.  Workgroups go to the 8
// XCDs round-robin and each XCD has its own L2: a run of PTR_RUN consecutive blocks, all parts, is given to ONE
// XCD, so that the pointers a chain visits (its own block's and the block's before) are in the L2 it runs on.
#ifndef PTR_RUN
#define PTR_RUN 16
#endif
#ifndef PTR_CHASE
#define PTR_CHASE 32                // pointers the chasing fetch follows before it gives a byte up (12: an engine-written
                                   // linked text stream keeps needing the passes, 44 instead of 59 GB/s; 96: as 32)
#endif
#ifndef PTR_ILP
#define PTR_ILP 1                  // groups per thread advancing in lock step: more requests in flight LOSE (2: -8 %, 4: -15 %),
#endif                             // the passes are bound by the number of scattered requests, not by their latency
__device__ __forceinline__ void ptr_map(unsigned wg, int &blkRel, int &part)
{
#ifdef PTR_FLAT_MAP
    blkRel = (int)(wg / PTR_PARTS); part = (int)(wg % PTR_PARTS);
#else
    const unsigned xcd = wg & 7u, j = wg >> 3;                      // the j-th workgroup this XCD receives
    const unsigned per = PTR_RUN * PTR_PARTS;
    const unsigned run = j / per, within = j % per;
    blkRel = (int)((run * 8u + xcd) * PTR_RUN + within / PTR_PARTS);
    part = (int)(within % PTR_PARTS);
#endif
}
static unsigned ptr_grid(int n) { return (unsigned)((n + 8 * PTR_RUN - 1) / (8 * PTR_RUN)) * (8 * PTR_RUN) * PTR_PARTS; }

// One pass of pointer jumping over the bytes of the listed blocks (PTR_PARTS workgroups per block).  Reads of
// pointers another thread is updating are harmless: every value a pointer ever holds is an ancestor.
__global__ __launch_bounds__(256) void k_ptr_jump(DecodeArgs a, int pass, unsigned items)
{
    if (a.asyncGate && a.linkStat[0] == 0u) return;     // asynchronous linked decode: the first pass found nothing to do
    PtrCtl *ctl = (PtrCtl *)a.ptr.ctl;
    // passes behind the first: only if the chasing fetch left something, and the pass before changed something
    if (pass > 0 && !(ctl->changed[PTR_MAX_PASSES] && ctl->changed[pass - 1])) return;
    uint32_t *P = a.ptr.buf;
    bool open = false;
    int lastBlk = -1;
    // (passes behind the first are launched with a small grid: they usually find nothing to do)
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
    int blkRel, part;
    ptr_map(item, blkRel, part);
    const int blk = a.segFirst + blkRel;
    if (blk >= a.segEnd || !ptr_taken(a, blk)) continue;
    lastBlk = blk;
    const uint32_t bLo = (uint32_t)(a.outOff[blk] - ptr_lo(a) + PTR_PRE);
    const int size = a.tol.size[blk];
    const int per = ((size + PTR_PARTS - 1) / PTR_PARTS + 3) & ~3;
    const int x0 = part * per, x1 = min(size, x0 + per);
    auto chase = [&](uint32_t e) -> uint32_t {
#pragma unroll
        for (int k = 0; k < PTR_JUMPS; k++) {
            e = P[e];
            if (e & PTR_FINAL) break;
        }
        if (!(e & PTR_FINAL)) open = true;
        return e;
    };
    if (((bLo | (uint32_t)x0) & 3u) == 0) {
        // four pointers per thread (16-byte accesses)
        uint4 *P4 = (uint4 *)(P + bLo);
        const int q1 = x1 >> 2;
        // One hop for all four pointers of a group per step.  Neighbouring bytes of a match have neighbouring sources,
        // hop after hop, until a chain leaves its match: while the four pointers are consecutive they are fetched
        // with ONE 16-byte request; otherwise with up to four requests that are in flight together.
        auto hop = [&](uint4 &v) -> bool {                 // false: nothing left to follow
            const bool o0 = !(v.x & PTR_FINAL), o1 = !(v.y & PTR_FINAL), o2 = !(v.z & PTR_FINAL), o3 = !(v.w & PTR_FINAL);
            if (!(o0 || o1 || o2 || o3)) return false;
            if (o0 && o1 && o2 && o3 && v.y == v.x + 1u && v.z == v.x + 2u && v.w == v.x + 3u) {
                uint4 w;
                __builtin_memcpy(&w, P + v.x, 16);
                v = w;
            } else {
                const uint32_t n0 = o0 ? P[v.x] : v.x, n1 = o1 ? P[v.y] : v.y, n2 = o2 ? P[v.z] : v.z, n3 = o3 ? P[v.w] : v.w;
                v.x = n0; v.y = n1; v.z = n2; v.w = n3;
            }
            return true;
        };
        auto unresolved = [](const uint4 &v) { return !((v.x & v.y & v.z & v.w) & PTR_FINAL); };
        for (int qb = (x0 >> 2) + (int)threadIdx.x; qb < q1; qb += 256 * PTR_ILP) {
            uint4 v[PTR_ILP];
            bool live[PTR_ILP];
#pragma unroll
            for (int g = 0; g < PTR_ILP; g++) {
                const int q = qb + 256 * g;
                live[g] = q < q1;
                v[g] = live[g] ? P4[q] : make_uint4(PTR_FINAL, PTR_FINAL, PTR_FINAL, PTR_FINAL);
                live[g] = live[g] && unresolved(v[g]);
            }
            bool dirty[PTR_ILP];
#pragma unroll
            for (int g = 0; g < PTR_ILP; g++) dirty[g] = live[g];
#pragma unroll 1
            for (int k = 0; k < PTR_JUMPS; k++) {
                bool any = false;
#pragma unroll
                for (int g = 0; g < PTR_ILP; g++) {
                    if (live[g]) live[g] = hop(v[g]);
                    any = any || live[g];
                }
                if (!any) break;
            }
#pragma unroll
            for (int g = 0; g < PTR_ILP; g++) {
                if (dirty[g]) {
                    P4[qb + 256 * g] = v[g];
                    if (unresolved(v[g])) open = true;
                }
            }
        }
        for (int x = (q1 << 2) + (int)threadIdx.x; x < x1; x += 256) {
            const uint32_t e = P[bLo + (uint32_t)x];
            if (!(e & PTR_FINAL)) P[bLo + (uint32_t)x] = chase(e);
        }
    } else {
        for (int x = x0 + (int)threadIdx.x; x < x1; x += 256) {
            const uint32_t e = P[bLo + (uint32_t)x];
            if (!(e & PTR_FINAL)) P[bLo + (uint32_t)x] = chase(e);
        }
    }
    }
    if (__syncthreads_or(open ? 1 : 0) && threadIdx.x == 0) {
        ctl->changed[pass] = 1u;
        if (pass == PTR_MAX_PASSES - 1 && lastBlk >= 0) {  // cannot happen (linked_ptr.hpp); never guess
            bool hd;
            atomicOr(&a.ptr.bad[ptr_stream(a, lastBlk, hd)], 1u);
        }
    }
}

// Every deferred byte is fetched from its root.  CHASE: the fetch that runs right behind the FIRST jump pass finishes
// what that pass left open by following those chains itself (up to PTR_CHASE pointers, nothing written back): on
// shallow data -- text is done after one pass and a few hops -- no further pass over the pointers is needed.  A byte it
// cannot resolve raises PtrCtl::changed[PTR_MAX_PASSES]: only then do the remaining jump passes and the plain fetch
// behind them run.
template <bool CHASE>
__global__ __launch_bounds__(256) void k_ptr_fetch(DecodeArgs a, unsigned items)
{
    if (a.asyncGate && a.linkStat[0] == 0u) return;     // asynchronous linked decode: the first pass found nothing to do
    PtrCtl *ctl = (PtrCtl *)a.ptr.ctl;
    if (!CHASE && !ctl->changed[PTR_MAX_PASSES]) return;
    const uint32_t *P = a.ptr.buf;
    const uint64_t lo = ptr_lo(a);
    const uint8_t *outLo = a.out + lo;
    const uint8_t *dictTail = a.dict0 ? a.dict0 + a.dict0Len : nullptr;      // index PTR_PRE - d is dictTail[-d]
    auto root = [&](uint32_t e) -> uint8_t {
        return (e >= PTR_PRE) ? outLo[e - PTR_PRE] : dictTail[(int)e - (int)PTR_PRE];
    };
    bool unresolved = false;
    auto follow = [&](uint32_t e) -> uint32_t {                     // CHASE, one byte: the root, or an open pointer
#pragma unroll 1
        for (int k = 0; k < PTR_CHASE && !(e & PTR_FINAL); k++) e = P[e];
        if (!(e & PTR_FINAL)) unresolved = true;
        return e;
    };
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        int blkRel, part;
        ptr_map(item, blkRel, part);
        const int blk = a.segFirst + blkRel;
        if (blk >= a.segEnd || !ptr_taken(a, blk)) continue;
        if (a.onlyBlk >= 0 && blk != a.onlyBlk) continue;
        const uint32_t bLo = (uint32_t)(a.outOff[blk] - lo + PTR_PRE);
        const int size = a.tol.size[blk];
        const int per = ((size + PTR_PARTS - 1) / PTR_PARTS + 3) & ~3;
        const int x0 = part * per, x1 = min(size, x0 + per);
        uint8_t *dst = a.out + a.outOff[blk];
        if (((bLo | (uint32_t)x0) & 3u) == 0) {
            // four bytes per thread: one 16-byte load of pointers, up to four byte fetches, one 4-byte store
            const uint4 *P4 = (const uint4 *)(P + bLo);
            const int q1 = x1 >> 2;
            for (int q = (x0 >> 2) + (int)threadIdx.x; q < q1; q += 256) {
                uint4 v = P4[q];
                if (CHASE && !((v.x & v.y & v.z & v.w) & PTR_FINAL)) {
#pragma unroll 1
                    for (int k = 0; k < PTR_CHASE; k++) {
                        const bool o0 = !(v.x & PTR_FINAL), o1 = !(v.y & PTR_FINAL), o2 = !(v.z & PTR_FINAL), o3 = !(v.w & PTR_FINAL);
                        if (!(o0 || o1 || o2 || o3)) break;
                        if (o0 && o1 && o2 && o3 && v.y == v.x + 1u && v.z == v.x + 2u && v.w == v.x + 3u) {
                            uint4 w;
                            __builtin_memcpy(&w, P + v.x, 16);            // neighbours: one request for the four
                            v = w;
                        } else {
                            const uint32_t n0 = o0 ? P[v.x] : v.x, n1 = o1 ? P[v.y] : v.y, n2 = o2 ? P[v.z] : v.z, n3 = o3 ? P[v.w] : v.w;
                            v.x = n0; v.y = n1; v.z = n2; v.w = n3;
                        }
                    }
                    if (!((v.x & v.y & v.z & v.w) & PTR_FINAL)) { unresolved = true; continue; }
                }
                v.x &= ~PTR_FINAL; v.y &= ~PTR_FINAL; v.z &= ~PTR_FINAL; v.w &= ~PTR_FINAL;
                const uint32_t self = bLo + 4u * (uint32_t)q;
                const bool m0 = v.x != self, m1 = v.y != self + 1u, m2 = v.z != self + 2u, m3 = v.w != self + 3u;
                if (!(m0 || m1 || m2 || m3)) continue;
                uint32_t w;
                if (m0 && m1 && m2 && m3 && v.x >= PTR_PRE && v.y == v.x + 1u && v.z == v.x + 2u && v.w == v.x + 3u) {
                    __builtin_memcpy(&w, outLo + (v.x - PTR_PRE), 4);          // four neighbouring roots: one request
                } else {
                    __builtin_memcpy(&w, dst + 4 * q, 4);
                    if (m0) w = (w & 0xffffff00u) | (uint32_t)root(v.x);
                    if (m1) w = (w & 0xffff00ffu) | ((uint32_t)root(v.y) << 8);
                    if (m2) w = (w & 0xff00ffffu) | ((uint32_t)root(v.z) << 16);
                    if (m3) w = (w & 0x00ffffffu) | ((uint32_t)root(v.w) << 24);
                }
                __builtin_memcpy(dst + 4 * q, &w, 4);
            }
            for (int x = (q1 << 2) + (int)threadIdx.x; x < x1; x += 256) {
                const uint32_t self = bLo + (uint32_t)x;
                uint32_t e = P[self];
                if (CHASE) { e = follow(e); if (!(e & PTR_FINAL)) continue; }
                e &= ~PTR_FINAL;
                if (e != self) dst[x] = root(e);
            }
        } else {
            for (int x = x0 + (int)threadIdx.x; x < x1; x += 256) {
                const uint32_t self = bLo + (uint32_t)x;
                uint32_t e = P[self];
                if (CHASE) { e = follow(e); if (!(e & PTR_FINAL)) continue; }
                e &= ~PTR_FINAL;
                if (e != self) dst[x] = root(e);
            }
        }
    }
    if (CHASE && __syncthreads_or(unresolved ? 1 : 0) && threadIdx.x == 0) {
        if (a.onlyBlk >= 0) ctl->lastOpen = 1u;          // (the full fetch behind this one decides about the further passes)
        else ctl->changed[PTR_MAX_PASSES] = 1u;
    }
}

// ... and only then do the results change: the passes above tell a dependent block by its standalone result.
__global__ __launch_bounds__(256) void k_ptr_finish(DecodeArgs a)
{
    if (a.asyncGate && a.linkStat[0] == 0u) return;     // asynchronous linked decode: the first pass found nothing to do
    const int blk = a.segFirst + (int)(blockIdx.x * 256u + threadIdx.x);
    if (blk < a.segEnd && ptr_taken(a, blk)) a.result[blk] = a.tol.size[blk];
}

size_t ptr_ctl_bytes() { return sizeof(PtrCtl); }
size_t ptr_ctl_last_open_offset() { return offsetof(PtrCtl, lastOpen); }

// linkStat[3] = blocks of the longest stream (the serial walk of a stream costs its length)
__global__ __launch_bounds__(256) void k_longest_stream(DecodeArgs a)
{
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s >= a.nStreams) return;
    const int b0 = min(max(a.streamFirst[s], 0), a.nBlocks), b1 = min(max(a.streamFirst[s + 1], b0), a.nBlocks);
    atomicMax(&a.linkStat[3], (uint32_t)(b1 - b0));
}

// How much of a linked block's output comes DIRECTLY from the block before it: matches whose source starts in front of
// the block (cbits/lz4.c:1883-1911).  One wavefront per SAMPLED block (blocks a.segFirst, a.segFirst + step, ...: `count` of
// them) walks the block's first sequences -- tokens and lengths only, nothing is copied -- and adds {bytes from the
// dictionary, bytes walked} to linkStat[8], [9].  The run-in decode reads how long a stream remembers a missing dictionary
// off this share before its first call (api.cpp): the reference's text 0.065, the engine's own linked text 0.077, noise
// with a period just under 64 KiB 0.5-0.9 (scripts/dict_share.py).
#define DICT_SHARE_SEQS 1024
__global__ __launch_bounds__(64) void k_dict_share(DecodeArgs a, int step, int count)
{
    const int s = (int)blockIdx.x;
    if (s >= count) return;
    const int blk = a.segFirst + s * step;
    if (blk >= a.nBlocks) return;
    const uint8_t *data = nullptr;
    int compLen = 0, cap = 0;
    if (uni(read_block_header(a, blk, data, compLen, cap)) != 0) return;
    InWindow win;
    win.lo = a.framed; win.hi = a.framed + a.framedLen;
    win.load(data);
    auto rd = [&](int pos) -> uint32_t {
        const uint8_t *p = data + pos;
        if (!win.covers(p, 1)) win.load(p);
        return win.byte_at(p);
    };
    int ip = 0;
    uint32_t op = 0, direct = 0;
    for (int n = 0; n < DICT_SHARE_SEQS && ip + 3 < compLen; n++) {
        const uint32_t t = rd(ip); ip++;
        uint32_t lit = t >> 4;
        if (lit == 15u) { uint32_t x; do { x = (ip < compLen) ? rd(ip) : 0u; ip++; lit += x; } while (x == 255u && ip < compLen); }
        ip += (int)lit; op += lit;
        if (ip + 2 > compLen) break;
        const uint32_t off = rd(ip) | (rd(ip + 1) << 8); ip += 2;
        uint32_t ml = t & 15u;
        if (ml == 15u) { uint32_t x; do { x = (ip < compLen) ? rd(ip) : 0u; ip++; ml += x; } while (x == 255u && ip < compLen); }
        ml += LZ4_MINMATCH;
        if (off > op) direct += min(ml, off - op);
        op += ml;
    }
    if (lane_id() == 0) { atomicAdd(&a.linkStat[8], direct); atomicAdd(&a.linkStat[9], op); }
}

void launch_dict_share(const DecodeArgs &a, int step, int count, hipStream_t s)
{
    if (a.linkStat && count > 0) hipLaunchKernelGGL(k_dict_share, dim3((unsigned)count), dim3(64), 0, s, a, step, count);
}

void launch_longest_stream(const DecodeArgs &a, hipStream_t s)
{
    if (a.streamFirst && a.nStreams > 0 && a.linkStat)
        hipLaunchKernelGGL(k_longest_stream, dim3((unsigned)((a.nStreams + 255) / 256)), dim3(256), 0, s, a);
}

// The pointer pass in two halves.  The first touches pointers only -- where every byte of the segment comes from
// is known from the tokens (lists) alone; the second reads DATA: the roots, the first of which lie in the block in
// front of the segment.  mi355lz4_decompress_linked_begin / _end run them apart so that the output of that block
// (the seam of a stream that is spread over several GPUs) may arrive in between.
void launch_linked_resolve_a(const DecodeArgs &a, hipStream_t s)
{
    const int n = a.segEnd - a.segFirst;
    if (n <= 0) return;
    if (a.tol.pool && a.ptr.buf && a.ptr.ctl && a.ptr.bad) {
        // (the stream flags follow the control block: a stream turned down in one segment gets its chance in the next)
        hipMemsetAsync(a.ptr.ctl, 0, sizeof(PtrCtl) + sizeof(uint32_t) * (size_t)(a.streamFirst ? a.nStreams : 1), s);
        hipLaunchKernelGGL(k_ptr_expand, dim3((unsigned)n + 1u), dim3(256), 0, s, a);
        const unsigned items = ptr_grid(n);
        hipLaunchKernelGGL(k_ptr_jump, dim3(items), dim3(256), 0, s, a, 0, items);
    }
}

void launch_linked_resolve_b(const DecodeArgs &a, hipStream_t s)
{
    const int n = a.segEnd - a.segFirst;
    if (n <= 0) return;
    if (a.tol.pool && a.ptr.buf && a.ptr.ctl && a.ptr.bad) {
        const unsigned items = ptr_grid(n), few = std::min(items, 4096u);
        hipLaunchKernelGGL(k_ptr_fetch<true>, dim3(items), dim3(256), 0, s, a, items);
        // (what follows usually finds nothing to do: small grids that stride over the items)
        for (int pass = 1; pass < PTR_MAX_PASSES; pass++)
            hipLaunchKernelGGL(k_ptr_jump, dim3(few), dim3(256), 0, s, a, pass, items);
        hipLaunchKernelGGL(k_ptr_fetch<false>, dim3(few), dim3(256), 0, s, a, items);
        hipLaunchKernelGGL(k_ptr_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    }
    // whatever the pass above did not take (ptr.bad, or no pool): the walk, block after block
    if (!a.streamFirst)
        hipLaunchKernelGGL(k_decode_fixup_regions, dim3((unsigned)((n + LZ4_WAVE - 1) / LZ4_WAVE)),
                           dim3(RPL_THREADS), 0, s, a);
    else if (a.nStreams > 0)
        hipLaunchKernelGGL(k_decode_fixup_linked, dim3((unsigned)a.nStreams), dim3(64), 0, s, a);
}

// One block of the segment fetched ahead of the others (a.onlyBlk): what a rank hands to its right neighbour when ONE
// linked stream is spread over several GPUs -- the neighbour then waits for one block's fetch, not for a range's.  The
// chasing fetch is complete unless it raises PtrCtl::lastOpen (a chain deeper than the first jump pass plus PTR_CHASE).
void launch_linked_fetch_block(const DecodeArgs &a, hipStream_t s)
{
    const int n = a.segEnd - a.segFirst;
    if (n <= 0 || !(a.tol.pool && a.ptr.buf && a.ptr.ctl && a.ptr.bad)) return;
    const unsigned items = ptr_grid(n);
    hipLaunchKernelGGL(k_ptr_fetch<true>, dim3(std::min(items, 4096u)), dim3(256), 0, s, a, items);
}

void launch_linked_resolve(const DecodeArgs &a, hipStream_t s)
{
    launch_linked_resolve_a(a, s);
    launch_linked_resolve_b(a, s);
}
