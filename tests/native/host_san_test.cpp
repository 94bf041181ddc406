// host_san_test.cpp -- sanitizer driver for the HOST side of libmi355lz4 (api.cpp, host_batch.cpp, legacy.cpp, host_stream.cpp).
//
// Built by `make asan` / `make tsan` (CPU only: the kernel launchers are stubbed by san_stubs.cpp, and
// without a gfx950 device every engine call stops at MI355LZ4_E_NO_DEVICE).  What runs under the sanitizers:
//   * the staging copy pool (api.cpp) hammered from several caller threads at once;
//   * the stream state machines that need no codec: resizeChunks at every split size the reference tests
//     (test/Main.hs:217-224), end mark, the frame-header parser, and their error paths;
//   * the legacy LZ4_* entry points' (legacy.cpp) no-device behaviour (create/free, compressBound, 0 / -1 returns);
//   * the one error message per thread that api.cpp keeps for every layer (host_batch.cpp's argument checks);
//   * the decode planner (linked_plan.hpp): a table of call shape -> path.
#include "../../include/lz4.h"
#include "../../include/mi355lz4.h"
#include "../../include/streamly_lz4.hpp"
#include "../../streamly-lz4_amd/csrc/linked_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

extern "C" int mi355lz4_debug_host_copy(uint8_t *dst, const uint8_t *src, size_t n);

static int failures = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); failures++; } } while (0)

static void pool_stress()
{
    std::vector<std::thread> th;
    for (int t = 0; t < 4; t++)
        th.emplace_back([t] {
            std::mt19937_64 rng(1234 + t);
            for (int it = 0; it < 12; it++) {
                const size_t n = (size_t)(rng() % (6u << 20)) + 1;
                std::vector<uint8_t> a(n), b(n, 0);
                for (size_t i = 0; i < n; i += 997) a[i] = (uint8_t)rng();
                if (mi355lz4_debug_host_copy(b.data(), a.data(), n) != 0 || memcmp(a.data(), b.data(), n) != 0) {
                    fprintf(stderr, "pool copy mismatch (thread %d, n %zu)\n", t, n);
                    __atomic_fetch_add(&failures, 1, __ATOMIC_RELAXED);
                }
            }
        });
    for (auto &x : th) x.join();
}

// a framed stream of fake blocks: resizeChunks only reads headers (Internal/LZ4.hs:459-484)
static std::vector<uint8_t> fake_stream(std::mt19937_64 &rng, int nBlocks, int meta, bool endMark, std::vector<size_t> &cuts)
{
    std::vector<uint8_t> s;
    for (int i = 0; i < nBlocks; i++) {
        const uint32_t c = (uint32_t)(rng() % 3000) + 1, u = (uint32_t)(rng() % 70000);
        cuts.push_back(s.size());
        for (int k = 0; k < 4; k++) s.push_back((uint8_t)(c >> (8 * k)));
        if (meta == 8) for (int k = 0; k < 4; k++) s.push_back((uint8_t)(u >> (8 * k)));
        for (uint32_t k = 0; k < c; k++) s.push_back((uint8_t)rng());
    }
    cuts.push_back(s.size());
    if (endMark) for (int k = 0; k < 4; k++) s.push_back(0);
    return s;
}

static void resize_checks()
{
    using namespace streamly_lz4;
    std::mt19937_64 rng(99);
    for (int meta : {8, 4})
        for (bool endMark : {false, true})
            for (size_t split : {(size_t)1, (size_t)512, (size_t)32768, (size_t)262144}) {
                std::vector<size_t> cuts;
                std::vector<uint8_t> s = fake_stream(rng, 40, meta, endMark, cuts);
                if (endMark) for (int k = 0; k < 7; k++) s.push_back(0xEE);   // trailing bytes after the end mark are ignored (:506-521)
                std::vector<Array> in;
                for (size_t o = 0; o < s.size(); o += split)
                    in.emplace_back(s.begin() + (long)o, s.begin() + (long)std::min(s.size(), o + split));
                BlockConfig cfg;
                cfg.blockSize = meta == 8 ? BlockSize::BlockHasSize : BlockSize::BlockMax64KB;
                FrameConfig fc;
                fc.hasEndMark = endMark;
                StreamPtr r = resizeChunks(cfg, fc, fromList(in));
                std::vector<Array> out = toList(*r);
                CHECK(out.size() + 1 == cuts.size());
                for (size_t i = 0; i < out.size() && i + 1 < cuts.size(); i++)
                    CHECK(out[i].size() == cuts[i + 1] - cuts[i] && memcmp(out[i].data(), s.data() + cuts[i], out[i].size()) == 0);
                // idempotence (test/Main.hs:189-201)
                if (!endMark) {
                    std::vector<Array> again = toList(*resizeChunks(cfg, fc, fromList(out)));
                    CHECK(again.size() == out.size());
                    for (size_t i = 0; i < again.size() && i < out.size(); i++) CHECK(again[i] == out[i]);
                }
            }
    // error paths: a stream cut inside a block, and a missing end mark
    {
        std::vector<size_t> cuts;
        std::vector<uint8_t> s = fake_stream(rng, 3, 8, false, cuts);
        s.resize(s.size() - 5);
        bool threw = false;
        try { toList(*resizeChunks(BlockConfig(), FrameConfig(), fromList({Array(s.begin(), s.end())}))); }
        catch (const Error &) { threw = true; }
        CHECK(threw);
        FrameConfig fc;
        fc.hasEndMark = true;
        std::vector<size_t> c2;
        std::vector<uint8_t> s2 = fake_stream(rng, 3, 8, false, c2);
        threw = false;
        try { toList(*resizeChunks(BlockConfig(), fc, fromList({Array(s2.begin(), s2.end())}))); }
        catch (const Error &) { threw = true; }
        CHECK(threw);
    }
    // frame header parser (Internal/LZ4.hs:590-651)
    {
        const uint8_t hdr[7] = {0x04, 0x22, 0x4D, 0x18, 0x40, 0x40, 0x00};
        auto r = simpleFrameParser(fromList({Array(hdr, hdr + 3), Array(hdr + 3, hdr + 7)}));
        CHECK(r.first.first.blockSize == BlockSize::BlockMax64KB && r.first.second.hasEndMark);
        uint8_t bad[7];
        memcpy(bad, hdr, 7);
        bad[4] = 0x60;                                            // block-independence flag: rejected (:631-632)
        bool threw = false;
        try { simpleFrameParser(fromList({Array(bad, bad + 7)})); } catch (const Error &) { threw = true; }
        CHECK(threw);
    }
}

static void legacy_no_device()
{
    CHECK(LZ4_compressBound(65536) == 65536 + 65536 / 255 + 16);
    CHECK(LZ4_compressBound(0x7E000001) == 0);
    mi355lz4_ctx *c = nullptr;
    const int rc = mi355lz4_create(&c, 0);
    if (rc == MI355LZ4_OK) { mi355lz4_destroy(c); return; }        // a GPU box: nothing more to check here
    CHECK(rc == MI355LZ4_E_NO_DEVICE && c == nullptr && strlen(mi355lz4_last_error()) > 0);
    void *cs = LZ4_createStream();
    void *ds = LZ4_createStreamDecode();
    char src[64] = {0}, dst[128];
    CHECK(LZ4_compress_fast_continue((LZ4_stream_t *)cs, src, dst, 64, 128, 1) == 0);     // no CPU codec: fails like the reference reports failure
    CHECK(LZ4_decompress_safe_continue((LZ4_streamDecode_t *)ds, src, dst, 1, 128) < 0);
    LZ4_freeStream((LZ4_stream_t *)cs);
    LZ4_freeStreamDecode((LZ4_streamDecode_t *)ds);
    LZ4_freeStream(nullptr);
    bool threw = false;
    try { streamly_lz4::Engine e(0); } catch (const streamly_lz4::Error &) { threw = true; }
    CHECK(threw);
}

// mi355lz4_last_error is ONE buffer per thread for the whole library: after a host-buffer call (host_batch.cpp) fails its argument
// check, the message is that call's and no longer the one an engine call (api.cpp) left before it -- on every thread.
static void one_last_error()
{
    auto check = [] {
        CHECK(mi355lz4_create(nullptr, 0) == MI355LZ4_E_ARG && strstr(mi355lz4_last_error(), "mi355lz4_create") != nullptr);
        const uint8_t cut[3] = {9, 0, 0};                          // a chain that ends inside its first header
        int n = -1;
        CHECK(mi355lz4_index_host(cut, sizeof(cut), 4, 65536, nullptr, nullptr, 8, &n) == MI355LZ4_E_STREAM && n == 0);
        CHECK(strstr(mi355lz4_last_error(), "index_host: incomplete block header at offset 0") != nullptr);
        CHECK(mi355lz4_create(nullptr, 0) == MI355LZ4_E_ARG);
        size_t outLen = 0;
        int got = 0;
        CHECK(mi355lz4_decompress_partial(nullptr, cut, sizeof(cut), 4, 65536, nullptr, 16, nullptr, 0, &outLen, nullptr, -1, &got) == MI355LZ4_E_ARG);
        CHECK(strcmp(mi355lz4_last_error(), "null ctx") == 0);
    };
    check();
    std::thread other(check);
    other.join();
}

// the frame reader's host half on valid, damaged and truncated frames: it either parses or throws, nothing else
static void frame_parser_fuzz()
{
    using namespace streamly_lz4;
    std::mt19937_64 rng(99);
    auto put32 = [](Array &a, uint32_t v) { for (int k = 0; k < 4; k++) a.push_back((uint8_t)(v >> (8 * k))); };
    for (int iter = 0; iter < 300; iter++) {
        const bool bsum = rng() & 1, csum = rng() & 1, csize = rng() & 1, indep = rng() & 1;
        const int code = 4 + (int)(rng() % 4);
        Array f, content;
        if (rng() % 4 == 0) { put32(f, 0x184D2A50u + (uint32_t)(rng() % 16)); put32(f, 5); for (int k = 0; k < 5; k++) f.push_back((uint8_t)k); }
        const size_t frameAt = f.size();
        put32(f, 0x184D2204u);
        const size_t descAt = f.size();
        f.push_back((uint8_t)(0x40 | (indep ? 0x20 : 0) | (bsum ? 0x10 : 0) | (csize ? 0x08 : 0) | (csum ? 0x04 : 0)));
        f.push_back((uint8_t)(code << 4));
        const int nb = (int)(rng() % 5);
        std::vector<Array> blocks;
        for (int b = 0; b < nb; b++) {
            Array blk(rng() % 700);
            for (auto &x : blk) x = (uint8_t)rng();
            content.insert(content.end(), blk.begin(), blk.end());
            blocks.push_back(std::move(blk));
        }
        if (csize) for (int k = 0; k < 8; k++) f.push_back((uint8_t)((uint64_t)content.size() >> (8 * k)));
        f.push_back((uint8_t)(xxh32(f.data() + descAt, f.size() - descAt, 0) >> 8));
        for (const Array &blk : blocks) {
            put32(f, (uint32_t)blk.size() | 0x80000000u);
            f.insert(f.end(), blk.begin(), blk.end());
            if (bsum) put32(f, xxh32(blk.data(), blk.size(), 0));
        }
        put32(f, 0);
        if (csum) put32(f, xxh32(content.data(), content.size(), 0));

        // intact: parses, and the re-framed literal blocks carry the content
        {
            size_t at = 0;
            Lz4FrameIndex ix;
            bool isFrame = lz4FrameParse(f, at, ix);
            if (frameAt) { CHECK(!isFrame && at == frameAt); isFrame = lz4FrameParse(f, at, ix); }
            CHECK(isFrame && at == f.size() && ix.independent == indep && ix.blockMax == ((size_t)1 << (8 + 2 * code)));
            CHECK(!csize || ix.contentSize == content.size());
            size_t bytes = 0, live = 0;
            for (const Array &blk : blocks) { bytes += blk.size(); live += !blk.empty(); }
            CHECK(ix.blockAt.size() == live + 1 && ix.framed.size() >= bytes + 5 * live);
        }
        // damaged
        for (int m = 0; m < 20; m++) {
            Array g = f;
            const int kind = (int)(rng() % 3);
            if (kind == 0 && !g.empty()) g.resize(rng() % g.size());
            else if (kind == 1 && !g.empty()) g[rng() % g.size()] ^= (uint8_t)(1u << (rng() % 8));
            else for (int k = 0; k < 4 && !g.empty(); k++) g[rng() % g.size()] = (uint8_t)rng();
            size_t at = 0;
            try {
                Lz4FrameIndex ix;
                while (at < g.size()) lz4FrameParse(g, at, ix);
            } catch (const Error &) {
            }
            CHECK(at <= g.size());
        }
    }
    CHECK(xxh32(nullptr, 0, 0) == 0x02CC5D05u);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Call shape -> path (linked_plan.hpp).  Every row records what decode_device_impl did at 55f3f47, before the decisions moved into
// the planner: the comments quote that code's conditions, and the expected values were read off it, not off the planner.
// ---------------------------------------------------------------------------------------------------------------------------------
static const int32_t kStreamTable[3] = {0, 1, 2};   // (the planner only asks whether there is a stream table / a dictionary)
static const uint8_t kDict[1] = {0};

static DecodeCall linked_call(int nBlocks, uint64_t framedLen)
{
    DecodeCall s{};
    s.linked = 1; s.nBlocks = nBlocks; s.framedLen = framedLen;
    return s;
}

static void plan_first_pass()
{
    // decoder == 1: seq; decoder == 3 (experiments): tok; !stats && (decoder == 4 || (decoder == 0 && cu_auto(nBlocks, framedLen))):
    // cu; else par.  cu_auto: CU_BLOCKS >= 0: nBlocks <= it; avg = framedLen / nBlocks < 3072: no; nBlocks <= 256 || (nBlocks <= 512
    // && avg >= 16384)
    struct Row { int decoder; bool stats; int nBlocks; uint64_t framedLen; int cuBlocks; FirstPass want; } rows[] = {
        {0, false, 256, 256 * 3072ull, -1, FirstPass::Cu},       // avg 3072: not below 3072
        {0, false, 256, 256 * 3072ull - 1, -1, FirstPass::Par},  // avg 3071
        {0, false, 257, 257 * 16384ull, -1, FirstPass::Cu},      // 257..512 blocks from 16384 bytes a block
        {0, false, 257, 257 * 16384ull - 1, -1, FirstPass::Par},
        {0, false, 512, 512 * 16384ull, -1, FirstPass::Cu},
        {0, false, 513, 513 * 65536ull, -1, FirstPass::Par},
        {0, true, 16, 16 * 65536ull, -1, FirstPass::Par},        // stats: never the workgroup form
        {1, false, 16, 16 * 65536ull, -1, FirstPass::Seq},
        {1, true, 16, 16 * 65536ull, -1, FirstPass::Seq},
        {2, false, 16, 16 * 65536ull, -1, FirstPass::Par},
        {3, false, 16, 16 * 65536ull, -1, FirstPass::Tok},
        {4, false, 100000, 100000ull, -1, FirstPass::Cu},        // variant 4: any number of blocks, any size
        {4, true, 16, 16 * 65536ull, -1, FirstPass::Par},
        {0, false, 1000, 1000ull, 1000, FirstPass::Cu},          // CU_BLOCKS = 1000: up to 1000 blocks whatever their size
        {0, false, 1001, 1001 * 65536ull, 1000, FirstPass::Par},
        {0, false, 1, 65536ull, 0, FirstPass::Par},              // CU_BLOCKS = 0: never
    };
    for (const Row &r : rows) {
        DecodeKnobs k;
        k.cuBlocks = r.cuBlocks;
        EngineMode m;
        m.decoder = r.decoder; m.stats = r.stats;
        CHECK(first_pass(linked_call(r.nBlocks, r.framedLen), m, k) == r.want);
    }
}

static void plan_big()
{
    // bigEligible = linked && bigKiB > 0 && plainBig (none of PTR, POOL_BLOCKS, RUNS, RUNIN, ASYNC set) && !streamFirst && !splitOk &&
    // !deferEnd && lookBack >= 0 && !dict0 && decoder == 0 && !stats && linkedAsyncCap <= 0 && 2 <= nBlocks <= 512 && cu_auto;
    // bigPre = bigEligible && framedLen / nBlocks >= bigKiB * 1024 / 2; the passes (and bigLate) need stat[4] >= bigKiB * 1024
    const DecodeCall base = linked_call(64, 64 * 262144ull);
    const DecodeKnobs k0;
    const EngineMode m0;
    CHECK(big_arm(base, m0, k0) == BigArm::BeforeFirstPass);                          // exactly bigKiB * 512 bytes a block
    CHECK(big_arm(linked_call(64, 64 * 262144ull - 1), m0, k0) == BigArm::AfterWait);  // one byte below
    CHECK(big_arm(linked_call(2, 2 * 262144ull), m0, k0) == BigArm::BeforeFirstPass);
    CHECK(big_arm(linked_call(512, 512 * 262144ull), m0, k0) == BigArm::BeforeFirstPass);
    auto no = [&](DecodeCall s, EngineMode m, DecodeKnobs k) { CHECK(big_arm(s, m, k) == BigArm::No); };
    { DecodeCall s = base; s.linked = 0; no(s, m0, k0); }
    { DecodeKnobs k; k.bigKiB = 0; no(base, m0, k); }                                   // LINKED_BIG=0
    { DecodeKnobs k; k.ptrSet = true; no(base, m0, k); }
    { DecodeKnobs k; k.poolSet = true; no(base, m0, k); }
    { DecodeKnobs k; k.runsSet = true; no(base, m0, k); }
    { DecodeKnobs k; k.runinSet = true; no(base, m0, k); }
    { DecodeKnobs k; k.asyncSet = true; no(base, m0, k); }                              // (even LINKED_ASYNC=0)
    { DecodeCall s = base; s.streamFirst = kStreamTable; s.nStreams = 2; no(s, m0, k0); }
    { DecodeCall s = base; s.splitOk = true; no(s, m0, k0); }
    { DecodeCall s = base; s.deferEnd = true; no(s, m0, k0); }
    { DecodeCall s = base; s.lookBack = -1; no(s, m0, k0); }
    { DecodeCall s = base; s.dict0 = kDict; no(s, m0, k0); }
    { EngineMode m; m.decoder = 4; no(base, m, k0); }
    { EngineMode m; m.decoder = 1; no(base, m, k0); }
    { EngineMode m; m.stats = true; no(base, m, k0); }
    { EngineMode m; m.asyncCap = 1; no(base, m, k0); }                                  // mi355lz4_set_linked_async
    no(linked_call(1, 262144ull), m0, k0);
    no(linked_call(513, 513 * 262144ull), m0, k0);
    { DecodeKnobs k; k.cuBlocks = 63; no(base, m0, k); }                                // cu_auto says no
    { DecodeKnobs k; k.bigKiB = 1024; CHECK(big_arm(base, m0, k) == BigArm::AfterWait); }
    LinkStat st;
    st.maxCap = 512 * 1024;
    CHECK(big_takes(k0, st));                                                           // exactly bigKiB * 1024
    st.maxCap = 512 * 1024 - 1;
    CHECK(!big_takes(k0, st));
}

static void plan_runs()
{
    // !streamFirst && !asyncGate && !splitOk && !deferEnd && runMax > 0 && stat[5] >= 1 && stat[5] <= runMax && (RUNS set || plain);
    // runMax = RUNS or 4; plain = neither PTR nor POOL_BLOCKS set
    const DecodeCall s0 = linked_call(100, 100 * 20000ull);
    const EngineMode m0;
    auto take = [&](uint32_t longest, const DecodeKnobs &k, DecodeCall s, EngineMode m) {
        LinkStat st;
        st.count = 3; st.longestRun = longest; st.runs = 3;
        return runs_take(s, m, k, st);
    };
    const DecodeKnobs k0;
    CHECK(!take(0, k0, s0, m0));
    CHECK(take(1, k0, s0, m0));
    CHECK(take(4, k0, s0, m0));
    CHECK(!take(5, k0, s0, m0));
    { DecodeKnobs k; k.runsSet = true; k.runMax = 8; CHECK(take(5, k, s0, m0)); }
    { DecodeKnobs k; k.runsSet = true; k.runMax = 0; CHECK(!take(1, k, s0, m0)); }
    { DecodeKnobs k; k.ptrSet = true; CHECK(!take(1, k, s0, m0)); }
    { DecodeKnobs k; k.poolSet = true; CHECK(!take(1, k, s0, m0)); }
    { DecodeKnobs k; k.ptrSet = true; k.runsSet = true; CHECK(take(1, k, s0, m0)); }    // RUNS set wins over plain
    { DecodeCall s = s0; s.streamFirst = kStreamTable; s.nStreams = 4; CHECK(!take(1, k0, s, m0)); }
    { DecodeCall s = s0; s.splitOk = true; CHECK(!take(1, k0, s, m0)); }
    { DecodeCall s = s0; s.deferEnd = true; CHECK(!take(1, k0, s, m0)); }
    { EngineMode m; m.asyncCap = 65536; CHECK(!take(1, k0, s0, m)); }                   // asyncGate
}

static void plan_runin()
{
    // decay: if (!RUNIN set && runinLong && ++runinLongOk >= 32) { runinLong = false; runinLongOk = 0; }; longRun = runinLong && !RUNIN set
    // use = !streamFirst && !asyncGate && (!(splitOk || deferEnd) || lookBack == 0) && (RUNIN set ? atoi != 0 : (plain && span0 >= 64
    //       && 2 * stride <= 2^31 && span0 * per64 >= (longRun ? 2 * 9216 : 9216))); plain = none of PTR, POOL_BLOCKS, RUNS set;
    //       per64 = max(1, ceil(stat[4] / 64 KiB)), stride = per64 * 64 KiB
    // if (use && !RUNIN set && runinSkip > 0) { runinSkip--; use = false; }; the share is sampled when use && !RUNIN set
    auto plan = [](int span0, uint32_t maxCap, const DecodeKnobs &k = DecodeKnobs(), DecodeCall s = linked_call(100000, 1),
                   RuninState st = RuninState(), EngineMode m = EngineMode()) { return runin_plan(st, s, m, k, span0, maxCap); };
    const uint32_t b64 = 65536;
    CHECK(plan(RUNIN_MIN_SPAN, b64).use && plan(RUNIN_MIN_SPAN, b64).sample);
    CHECK(!plan(RUNIN_MIN_SPAN - 1, b64).use);
    CHECK(plan(RUNIN_MIN_SPAN / 4, 4 * b64).use && plan(RUNIN_MIN_SPAN / 4, 4 * b64).per64 == 4);
    CHECK(!plan(RUNIN_MIN_SPAN / 4 - 1, 4 * b64).use);
    CHECK(plan(RUNIN_MIN_SPAN / 4, 4 * b64 - 1).use);                                  // per64 rounds up
    CHECK(plan(1, 0).per64 == 1);
    CHECK(!plan(63, 200 * b64).use);                                                   // the span from 64 blocks on
    CHECK(plan(64, 144 * b64).use);                                                    // 64 x 144 = 9216
    CHECK(!plan(64, 143 * b64).use);
    CHECK(plan(64, 1u << 30).use);                                                     // strides of 1 GiB: two of them are 2 GiB
    CHECK(!plan(64, (1u << 30) + 1).use);
    {
        RuninState st;
        st.longRun = true;
        DecodeCall s = linked_call(100000, 1);
        for (int span : {2 * RUNIN_MIN_SPAN, 2 * RUNIN_MIN_SPAN - 1}) {
            RuninState t = st;
            const RuninPlan p = runin_plan(t, s, EngineMode(), DecodeKnobs(), span, b64);
            CHECK(p.longRun && p.use == (span == 2 * RUNIN_MIN_SPAN) && t.longOk == 1);
        }
        for (int span : {2 * RUNIN_MIN_SPAN / 4, 2 * RUNIN_MIN_SPAN / 4 - 1}) {
            RuninState t = st;
            CHECK(runin_plan(t, s, EngineMode(), DecodeKnobs(), span, 4 * b64).use == (span == 2 * RUNIN_MIN_SPAN / 4));
        }
    }
    for (int lookBack : {0, 1}) {
        DecodeCall s = linked_call(100000, 1);
        s.lookBack = lookBack; s.splitOk = s.deferEnd = true;
        CHECK(plan(RUNIN_MIN_SPAN, b64, DecodeKnobs(), s).use == (lookBack == 0));
        s.splitOk = false;
        CHECK(plan(RUNIN_MIN_SPAN, b64, DecodeKnobs(), s).use == (lookBack == 0));
        s.lookBack = lookBack; s.splitOk = s.deferEnd = false;
        CHECK(plan(RUNIN_MIN_SPAN, b64, DecodeKnobs(), s).use);                        // a plain call: any lookBack
    }
    { DecodeCall s = linked_call(100000, 1); s.streamFirst = kStreamTable; s.nStreams = 3; CHECK(!plan(RUNIN_MIN_SPAN, b64, DecodeKnobs(), s).use); }
    { EngineMode m; m.asyncCap = 65536; CHECK(!plan(RUNIN_MIN_SPAN, b64, DecodeKnobs(), linked_call(100000, 1), RuninState(), m).use); }
    { DecodeKnobs k; k.runsSet = true; CHECK(!plan(RUNIN_MIN_SPAN, b64, k).use); }
    { DecodeKnobs k; k.ptrSet = true; CHECK(!plan(RUNIN_MIN_SPAN, b64, k).use); }
    { DecodeKnobs k; k.poolSet = true; CHECK(!plan(RUNIN_MIN_SPAN, b64, k).use); }
    { DecodeKnobs k; k.runinSet = true; k.runin = 1; const RuninPlan p = plan(1, b64, k); CHECK(p.use && !p.sample); }
    { DecodeKnobs k; k.runinSet = true; k.runin = 0; CHECK(!plan(RUNIN_MIN_SPAN, b64, k).use); }
    // the skip counter: only when the run-in would be taken, and not when it is forced
    {
        RuninState st;
        st.skip = 3;
        DecodeCall s = linked_call(100000, 1);
        CHECK(!runin_plan(st, s, EngineMode(), DecodeKnobs(), RUNIN_MIN_SPAN, b64).use && st.skip == 2);
        CHECK(!runin_plan(st, s, EngineMode(), DecodeKnobs(), 10, b64).use && st.skip == 2);
        DecodeKnobs k;
        k.runinSet = true; k.runin = 1;
        CHECK(runin_plan(st, s, EngineMode(), k, RUNIN_MIN_SPAN, b64).use && st.skip == 2);
    }
    // the probe: the long run-in for 31 more calls that get here, whatever their size, then the default again; a forced run-in does
    // not count
    {
        RuninState st;
        st.longRun = true;
        DecodeCall s = linked_call(100000, 1);
        s.streamFirst = kStreamTable; s.nStreams = 2;
        for (int call = 1; call <= RUNIN_LONG_PROBE; call++) {
            const RuninPlan p = runin_plan(st, s, EngineMode(), DecodeKnobs(), 10, b64);
            CHECK(!p.use && p.longRun == (call < RUNIN_LONG_PROBE) && st.longRun == (call < RUNIN_LONG_PROBE));
            CHECK(st.longOk == (call < RUNIN_LONG_PROBE ? call : 0));
        }
        st.longRun = true; st.longOk = 5;
        DecodeKnobs k;
        k.runinSet = true; k.runin = 1;
        CHECK(!runin_plan(st, linked_call(100000, 1), EngineMode(), k, 10, b64).longRun && st.longOk == 5 && st.longRun);
    }
    // after the sample: share >= 0.60: no run-in; >= 0.306: the long one, which needs span0 * per64 >= 2 * RUNIN_MIN_SPAN
    auto after = [&](int span0, double share) {
        RuninPlan p = plan(span0, b64);
        runin_after_sample(p, DecodeKnobs(), span0, share);
        return p;
    };
    const int big = 2 * RUNIN_MIN_SPAN;
    CHECK(after(big, 0.3059).use && !after(big, 0.3059).longRun);
    CHECK(after(big, 0.306).use && after(big, 0.306).longRun);
    CHECK(!after(RUNIN_MIN_SPAN, 0.306).use);
    CHECK(after(RUNIN_MIN_SPAN, -1).use && !after(RUNIN_MIN_SPAN, -1).longRun);      // no sample
    CHECK(after(big, 0.5999).use && after(big, 0.5999).longRun);
    CHECK(!after(big, 0.60).use);
    // sizes: runIn = RUNIN_BLOCKS > 0 ? it : (per64 == 1 ? run64 : (run64 + per64) / per64 + 1), run64 = longRun ? 17 : 11, at most
    // 64; maxPieces = 2^31 / (2 * stride) within [1, 4096]; piece = ceil(span0 / maxPieces), or RUNIN_PIECE > 0, at least 1;
    // segBlocks = min(maxPieces * piece, span0)
    struct Size { int span0; uint32_t maxCap; bool longRun; int blocks, pieceKnob; int runIn, piece, segBlocks; uint64_t maxPieces; } sizes[] = {
        {9216, 65536, false, 0, 0, 11, 3, 9216, 4096},
        {18432, 65536, true, 0, 0, 17, 5, 18432, 4096},
        {2304, 4 * 65536, false, 0, 0, 4, 1, 2304, 4096},
        {576, 16 * 65536, false, 0, 0, 2, 1, 576, 1024},
        {1152, 16 * 65536, true, 0, 0, 3, 2, 1152, 1024},
        {64, 1u << 30, false, 0, 0, 2, 64, 64, 1},
        {9216, 65536, false, 5, 7, 5, 7, 9216, 4096},
        {9216, 65536, false, 100, 0, 64, 3, 9216, 4096},                                // runIn capped at 64
        {20000, 65536, false, 0, 2, 11, 2, 8192, 4096},                                  // forced pieces: segments of 4096 x 2 blocks
        {3, 0x7fffffffu, false, 0, 0, 2, 3, 3, 1},                                       // (forced run-in) 2 GiB strides: one piece
    };
    for (const Size &z : sizes) {
        DecodeKnobs k;
        k.runinBlocks = z.blocks; k.runinPiece = z.pieceKnob;
        k.runinSet = true; k.runin = 1;
        RuninState st;
        RuninPlan p = runin_plan(st, linked_call(100000, 1), EngineMode(), k, z.span0, z.maxCap);
        p.longRun = z.longRun;
        runin_after_sample(p, k, z.span0, -1);
        CHECK(p.use && p.runIn == z.runIn && p.piece == z.piece && p.segBlocks == z.segBlocks && p.maxPieces == z.maxPieces);
    }
    // given up: if (!segDone && !(stat[1] & 1u) && !RUNIN set) { if (!longRun) runinLong = true; else runinSkip = 16; runinLongOk = 0; }
    {
        RuninState st;
        st.longOk = 7;
        RuninPlan p;
        runin_given_up(st, p, DecodeKnobs(), 0);                                         // rounds that ran out: default -> long
        CHECK(st.longRun && st.longOk == 0 && st.skip == 0);
        p.longRun = true;
        st.longOk = 3;
        runin_given_up(st, p, DecodeKnobs(), 2);                                         // a chain of dirty pieces: long -> skip 16
        CHECK(st.longRun && st.longOk == 0 && st.skip == RUNIN_BACKOFF && RUNIN_BACKOFF == 16);
        RuninState t;
        runin_given_up(t, RuninPlan(), DecodeKnobs(), 1);                                // a broken block teaches nothing
        DecodeKnobs k;
        k.runinSet = true; k.runin = 1;
        runin_given_up(t, RuninPlan(), k, 0);                                            // nor does a forced run-in
        CHECK(!t.longRun && t.skip == 0);
    }
}

static void plan_pointer()
{
    // poolMax = POOL_BLOCKS or 16384; ptrMax = PTR_BLOCKS > 0 ? it : 4096; usePtr = !PTR || atoi(PTR) != 0; per = max(1, ceil(stat[4] /
    // 64 KiB)); walkStreams = streamFirst && !PTR set && 0.42 * (stat[3] > 0 ? stat[3] - 1 : 0) * (1 + nStreams / 5000) < 0.55 +
    // 1.15e-3 * stat[0]; poolBlocks = POOL_BLOCKS set ? poolMax : max(1, poolMax / per); ptrBlocks = PTR_BLOCKS > 0 ? ptrMax :
    // max(1, ptrMax / per); pool = (poolMax > 0 && !walkStreams) ? min(span, poolBlocks) : span; pointers when usePtr and
    // (min(pool, ptrBlocks) + 1) * per * 64 KiB + 64 KiB < 2^31; split = splitOk && a.ptr.buf && span <= seg && span <= pool
    auto plan = [](int span, uint32_t maxCap, const DecodeKnobs &k = DecodeKnobs(), DecodeCall s = linked_call(100000, 1),
                   uint32_t count = 100, uint32_t longestStream = 0) {
        LinkStat st;
        st.count = count; st.maxCap = maxCap; st.longestStream = longestStream;
        return ptr_plan(s, k, st, span);
    };
    {
        const PtrPlan p = plan(10000, 65536);
        CHECK(p.per == 1 && p.poolBlocks == 16384 && p.ptrBlocks == 4096 && p.lists && p.pool == 10000 && p.seg == 4096 && p.usePtr);
        CHECK(p.ptrs == 4098ull * 65536 && !p.walkStreams);
    }
    {
        const PtrPlan p = plan(10000, 16 * 65536);
        CHECK(p.per == 16 && p.poolBlocks == 1024 && p.ptrBlocks == 256 && p.pool == 1024 && p.seg == 256 && p.usePtr);
    }
    CHECK(plan(10, 0).per == 1);
    { DecodeKnobs k; k.poolSet = true; k.poolMax = 0; const PtrPlan p = plan(10000, 65536, k); CHECK(!p.lists && p.pool == 10000); }
    { DecodeKnobs k; k.poolSet = true; k.poolMax = 3; const PtrPlan p = plan(10000, 16 * 65536, k); CHECK(p.poolBlocks == 3 && p.pool == 3); }
    { DecodeKnobs k; k.ptrSet = true; k.ptr = 0; const PtrPlan p = plan(10000, 65536, k); CHECK(p.lists && !p.usePtr); }
    { DecodeKnobs k; k.ptrSet = true; k.ptr = 1; CHECK(plan(10000, 65536, k).usePtr); }
    { DecodeKnobs k; k.ptrBlocks = 2; const PtrPlan p = plan(10000, 16 * 65536, k); CHECK(p.ptrBlocks == 2 && p.seg == 2); }
    {
        DecodeKnobs k;
        k.poolSet = true; k.poolMax = 10000; k.ptrBlocks = 1000;
        const PtrPlan p = plan(10000, 64 * 65536, k);                                    // 2^31 pointers or more: none
        CHECK(p.pool == 10000 && p.seg == 1000 && !p.usePtr);
    }
    // walk: a longest stream of 3 costs 0.42 * 2 = 0.84 against the pointer passes' 0.55 + 1.15e-3 * count: walked from count 253 on
    DecodeCall s = linked_call(100000, 1);
    s.streamFirst = kStreamTable; s.nStreams = 10;
    CHECK(plan(100, 65536, DecodeKnobs(), s, 1, 2).walkStreams);
    CHECK(plan(100, 65536, DecodeKnobs(), s, 253, 3).walkStreams);
    CHECK(!plan(100, 65536, DecodeKnobs(), s, 252, 3).walkStreams && plan(100, 65536, DecodeKnobs(), s, 252, 3).lists);
    { const PtrPlan p = plan(100, 65536, DecodeKnobs(), s, 1, 2); CHECK(!p.lists && p.pool == 100); }
    { DecodeKnobs k; k.ptrSet = true; CHECK(!plan(100, 65536, k, s, 1, 2).walkStreams); }
    CHECK(!plan(100, 65536, DecodeKnobs(), linked_call(100000, 1), 1, 2).walkStreams);  // one stream: never
    s.nStreams = 5000;
    CHECK(!plan(100, 65536, DecodeKnobs(), s, 1, 2).walkStreams);                        // 0.84 > 0.55115
    CHECK(linked_split(true, true, 10, 10, 10));
    CHECK(!linked_split(false, true, 10, 10, 10));
    CHECK(!linked_split(true, false, 10, 10, 10));
    CHECK(!linked_split(true, true, 11, 10, 20));
    CHECK(!linked_split(true, true, 11, 20, 10));
}

static void plan_knobs()
{
    // the asynchronous form's stand-in summary: stat = {nBlocks, 0, nBlocks - 1, nBlocks, asyncCap}
    const LinkStat a = LinkStat::whole_call(40, 1 << 20);
    CHECK(a.count == 40 && a.first == 0 && a.last == 39 && a.longestStream == 40 && a.maxCap == (1u << 20));
    CHECK(async_gate(linked_call(4, 4), EngineMode{0, false, 1}) && !async_gate(linked_call(4, 4), EngineMode{0, false, 0}));
    const char *names[] = {"MI355LZ4_LINKED_BIG", "MI355LZ4_LINKED_ASYNC", "MI355LZ4_LINKED_RUNS", "MI355LZ4_LINKED_RUNIN",
                           "MI355LZ4_LINKED_RUNIN_BLOCKS", "MI355LZ4_LINKED_RUNIN_PIECE", "MI355LZ4_LINKED_RUNIN_SPIN",
                           "MI355LZ4_LINKED_PTR", "MI355LZ4_LINKED_POOL_BLOCKS", "MI355LZ4_LINKED_PTR_BLOCKS"};
    for (const char *n : names) unsetenv(n);
    DecodeKnobs k = read_decode_knobs();
    CHECK(k.bigKiB == 512 && !k.asyncSet && k.runMax == 4 && !k.runinSet && k.runinSpin == 10000 && k.ptr == 1 && k.poolMax == 16384);
    CHECK(k.runsAuto() && k.runinAuto() && k.bigAuto());
    setenv("MI355LZ4_LINKED_RUNS", "0", 1);
    k = read_decode_knobs();                                 // read per call
    CHECK(k.runsSet && k.runMax == 0 && k.runsAuto() && !k.runinAuto() && !k.bigAuto());
    setenv("MI355LZ4_LINKED_PTR", "0", 1);
    k = read_decode_knobs();
    CHECK(k.ptrSet && k.ptr == 0 && !k.runsAuto());
    for (const char *n : names) unsetenv(n);
    setenv("MI355LZ4_LINKED_ASYNC", "0", 1);                 // set at all: no big blocks
    k = read_decode_knobs();
    CHECK(k.asyncSet && k.asyncCap == 0 && k.runinAuto() && !k.bigAuto());
    unsetenv("MI355LZ4_LINKED_ASYNC");
}

static void linked_plan_table()
{
    plan_first_pass();
    plan_big();
    plan_runs();
    plan_runin();
    plan_pointer();
    plan_knobs();
}

int main()
{
    linked_plan_table();
    frame_parser_fuzz();
    pool_stress();
    resize_checks();
    legacy_no_device();
    one_last_error();
    if (failures) { fprintf(stderr, "host_san_test: %d failure(s)\n", failures); return 1; }
    printf("host_san_test ok\n");
    return 0;
}
