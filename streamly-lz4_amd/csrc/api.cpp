// api.cpp -- C ABI of the MI355X LZ4 block engine (include/mi355lz4.h, include/lz4.h).
//
// Host-side plumbing only: argument checks, device workspaces, copies and
// kernel launches.  All arithmetic of the hot path happens in the kernels (kernels.hip, kernels/*.inc).
// There is no CPU code path: without a gfx950 device every call fails.
#include "engine.hpp"

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>

using namespace mi355lz4_detail;

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local char g_err[512] = "";      // one per thread for the whole library: the other files write it through fail()

int mi355lz4_detail::fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ---------------------------------------------------------------------------
// Host copy pool: the staging copies between pageable caller memory and the
// pinned buffers are what bounds the host-buffer API (one thread moves ~10 GB/s,
// the Gen5 x16 link ~55 GB/s), so they are spread over a few threads.
// MI355LZ4_COPY_THREADS overrides the count (default 8, 1 = no helper threads).
// ---------------------------------------------------------------------------
class CopyPool {
public:
    CopyPool()
    {
        int n = 8;
        if (const char *e = getenv("MI355LZ4_COPY_THREADS")) n = atoi(e);
        const unsigned hw = std::thread::hardware_concurrency();
        if (hw && (unsigned)n > hw) n = (int)hw;
        if (n < 1) n = 1;
        for (int i = 1; i < n; i++) workers_.emplace_back([this] { loop(); });
    }
    ~CopyPool()
    {
        { std::lock_guard<std::mutex> lk(m_); stop_ = true; }
        cvWork_.notify_all();
        for (auto &t : workers_) t.join();
    }
    // run all tasks; the calling thread works too; returns when every byte is copied
    void run(const std::vector<CopyTask> &tasks)
    {
        if (tasks.empty()) return;
        if (workers_.empty() || tasks.size() == 1) {
            for (const CopyTask &t : tasks) if (t.n) memcpy(t.dst, t.src, t.n);
            return;
        }
        std::lock_guard<std::mutex> one(callers_);   // one batch of tasks at a time
        std::unique_lock<std::mutex> lk(m_);
        tasks_ = &tasks; next_ = 0; pending_ = tasks.size();
        grab_ = tasks.size() / ((workers_.size() + 1) * 8) + 1;    // a few grabs per thread: small tasks share a lock trip
        cvWork_.notify_all();
        while (next_ < tasks.size()) {
            const size_t lo = next_, hi = (lo + grab_ < tasks.size()) ? lo + grab_ : tasks.size();
            next_ = hi;
            lk.unlock();
            for (size_t i = lo; i < hi; i++) if (tasks[i].n) memcpy(tasks[i].dst, tasks[i].src, tasks[i].n);
            lk.lock();
            pending_ -= hi - lo;
        }
        cvDone_.wait(lk, [this] { return pending_ == 0; });
        tasks_ = nullptr;
    }
    // one large range, cut into slices
    void copy(uint8_t *dst, const uint8_t *src, size_t n)
    {
        static const size_t kSlice = (size_t)1 << 20;
        std::vector<CopyTask> t;
        for (size_t off = 0; off < n; off += kSlice) t.push_back({dst + off, src + off, (n - off < kSlice) ? n - off : kSlice});
        run(t);
    }

private:
    void loop()
    {
        std::unique_lock<std::mutex> lk(m_);
        for (;;) {
            cvWork_.wait(lk, [this] { return stop_ || (tasks_ && next_ < tasks_->size()); });
            if (stop_) return;
            while (tasks_ && next_ < tasks_->size()) {
                const std::vector<CopyTask> &ts = *tasks_;
                const size_t lo = next_, hi = (lo + grab_ < ts.size()) ? lo + grab_ : ts.size();
                next_ = hi;
                lk.unlock();
                for (size_t i = lo; i < hi; i++) if (ts[i].n) memcpy(ts[i].dst, ts[i].src, ts[i].n);
                lk.lock();
                pending_ -= hi - lo;
                if (pending_ == 0) cvDone_.notify_all();
            }
        }
    }
    std::vector<std::thread> workers_;
    std::mutex m_, callers_;
    std::condition_variable cvWork_, cvDone_;
    const std::vector<CopyTask> *tasks_ = nullptr;
    size_t next_ = 0, pending_ = 0, grab_ = 1;
    bool stop_ = false;
};

static CopyPool &copy_pool()
{
    static CopyPool *pool = new CopyPool();     // leaked on purpose: no thread joins during process teardown
    return *pool;
}
void mi355lz4_detail::pool_run(const std::vector<CopyTask> &tasks) { copy_pool().run(tasks); }
void mi355lz4_detail::pool_copy(uint8_t *dst, const uint8_t *src, size_t n) { copy_pool().copy(dst, src, n); }

// ---------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------
int mi355lz4_detail::dev_reserve(DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return 0;
    if (b.p) { hipFree(b.p); b.p = nullptr; b.cap = 0; }
    size_t want = bytes + bytes / 4 + 256;
    HIP_TRY(hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}
int mi355lz4_detail::pin_reserve(DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return 0;
    if (b.p) { hipHostFree(b.p); b.p = nullptr; b.cap = 0; }
    size_t want = bytes + bytes / 4 + 256;
    HIP_TRY(hipHostMalloc(&b.p, want, hipHostMallocDefault));
    b.cap = want;
    return 0;
}
void mi355lz4_detail::dev_release(DevBuf &b) { if (b.p) hipFree(b.p); b.p = nullptr; b.cap = 0; }
void mi355lz4_detail::pin_release(DevBuf &b) { if (b.p) hipHostFree(b.p); b.p = nullptr; b.cap = 0; }

// ---------------------------------------------------------------------------
// Host <-> device transfers of pageable memory, pipelined through pinned staging:
// the CPU memcpy of chunk i+1 overlaps the DMA of chunk i.
// A plain hipMemcpy of pageable memory runs at a few GB/s; this keeps the link busy.
// ---------------------------------------------------------------------------
static size_t stage_chunk()
{
    static const size_t v = [] {
        const char *e = getenv("MI355LZ4_STAGE_CHUNK_MB");
        const long mb = e ? atol(e) : 16;
        return (size_t)((mb < 1) ? 1 : (mb > 256 ? 256 : mb)) << 20;
    }();
    return v;
}
#define kStageChunk (stage_chunk())

int mi355lz4_detail::h2d_staged(mi355lz4_ctx *c, void *dstDev, const uint8_t *srcHost, size_t bytes)
{
    if (!bytes) return 0;
    int r = pin_reserve(c->pinIn, bytes);
    if (r) return r;
    uint8_t *stage = (uint8_t *)c->pinIn.p;
    for (size_t off = 0; off < bytes; off += kStageChunk) {
        const size_t n = (bytes - off < kStageChunk) ? bytes - off : kStageChunk;
        copy_pool().copy(stage + off, srcHost + off, n);
        HIP_TRY(hipMemcpyAsync((uint8_t *)dstDev + off, stage + off, n, hipMemcpyHostToDevice, c->stream));
    }
    return 0;
}

int mi355lz4_detail::d2h_staged(mi355lz4_ctx *c, uint8_t *dstHost, const void *srcDev, size_t bytes)
{
    if (!bytes) return 0;
    int r = pin_reserve(c->pinOut, bytes);
    if (r) return r;
    uint8_t *stage = (uint8_t *)c->pinOut.p;
    const size_t nChunks = (bytes + kStageChunk - 1) / kStageChunk;
    std::vector<hipEvent_t> ev(nChunks, nullptr);
    int rc = 0;
    size_t issued = 0;
    for (size_t k = 0; k < nChunks && !rc; k++) {
        const size_t off = k * kStageChunk;
        const size_t n = (bytes - off < kStageChunk) ? bytes - off : kStageChunk;
        if (hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess ||
            hipMemcpyAsync(stage + off, (const uint8_t *)srcDev + off, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipEventRecord(ev[k], c->stream) != hipSuccess)
            rc = fail(MI355LZ4_E_HIP, "d2h_staged: copy of chunk %zu could not be queued", k);
        else
            issued = k + 1;
    }
    for (size_t k = 0; k < nChunks; k++) {
        const size_t off = k * kStageChunk;
        const size_t n = (bytes - off < kStageChunk) ? bytes - off : kStageChunk;
        if (!rc && k < issued && hipEventSynchronize(ev[k]) != hipSuccess) rc = fail(MI355LZ4_E_HIP, "hipEventSynchronize failed");
        if (!rc && k < issued) copy_pool().copy(dstHost + off, stage + off, n);
        if (ev[k]) hipEventDestroy(ev[k]);
    }
    return rc;
}

static bool device_is_gfx950(int dev)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
    return strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

// Diagnostic hook (not part of the public header): one copy through the staging copy pool, so that the
// sanitizer driver (tests/native/host_san_test.cpp) can exercise the pool without a device.
extern "C" int mi355lz4_debug_host_copy(uint8_t *dst, const uint8_t *src, size_t n)
{
    if (n && (!dst || !src)) return fail(MI355LZ4_E_ARG, "debug_host_copy: null pointer");
    copy_pool().copy(dst, src, n);
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_version(void) { return MI355LZ4_VERSION; }
extern "C" const char *mi355lz4_last_error(void) { return g_err; }

extern "C" int mi355lz4_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int d = 0; d < n; d++) ok += device_is_gfx950(d) ? 1 : 0;
    return ok;
}

extern "C" int mi355lz4_create(mi355lz4_ctx **out, int device)
{
    if (!out) return fail(MI355LZ4_E_ARG, "mi355lz4_create: null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(MI355LZ4_E_NO_DEVICE, "mi355lz4: no HIP device visible (this engine has no CPU path)");
    if (device < 0 || device >= n) return fail(MI355LZ4_E_ARG, "mi355lz4_create: device %d out of range", device);
    if (!device_is_gfx950(device))
        return fail(MI355LZ4_E_NO_DEVICE, "mi355lz4: device %d is not gfx950 (MI355X); kernels are gfx950-only", device);
    mi355lz4_ctx *c = new (std::nothrow) mi355lz4_ctx();
    if (!c) return fail(MI355LZ4_E_ARG, "out of host memory");
    c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) { delete c; return fail(MI355LZ4_E_HIP, "hipSetDevice: %s", hipGetErrorString(e)); }
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(MI355LZ4_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    c->ownStream = true;
    *out = c;
    return MI355LZ4_OK;
}

extern "C" void mi355lz4_destroy(mi355lz4_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (DevBuf *b : {&c->in, &c->slots, &c->dense, &c->out, &c->offA, &c->offB, &c->lenA, &c->lenB, &c->res, &c->scratch,
                      &c->tolPool, &c->tolMeta, &c->linkBuf, &c->ptrBuf, &c->seg[0].b, &c->seg[1].b, &c->seg[2].b, &c->seg[3].b, &c->tokBuf,
                      &c->hcStage[0].b, &c->hcStage[1].b, &c->hcStage[2].b, &c->hcStage[3].b,
                      &c->ckBuf, &c->exState, &c->exMeta, &c->exTabs, &c->exFlags})
        dev_release(*b);
    if (c->linkEvent) hipEventDestroy(c->linkEvent);
    if (c->ckEvent) hipEventDestroy(c->ckEvent);
    pin_release(c->pinStat);
    pin_release(c->pinIn);
    pin_release(c->pinOut);
    pin_release(c->pinMeta);
    if (c->sIn) hipStreamDestroy(c->sIn);
    if (c->sOut) hipStreamDestroy(c->sOut);
    for (hipStream_t &k : c->sK) if (k) hipStreamDestroy(k);
    if (c->ownStream && c->stream) hipStreamDestroy(c->stream);
    delete c;
}

extern "C" int mi355lz4_set_stream(mi355lz4_ctx *c, void *s)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (c->ownStream && c->stream) { hipStreamSynchronize(c->stream); hipStreamDestroy(c->stream); }
    c->stream = (hipStream_t)s;
    c->ownStream = false;
    return MI355LZ4_OK;
}
extern "C" void *mi355lz4_get_stream(mi355lz4_ctx *c) { return c ? (void *)c->stream : nullptr; }

extern "C" int mi355lz4_set_linked_async(mi355lz4_ctx *c, int maxDecodedBlockSize)
{
    if (!c || maxDecodedBlockSize < 0) return fail(MI355LZ4_E_ARG, "mi355lz4_set_linked_async: bad arguments");
    c->linkedAsyncCap = maxDecodedBlockSize;
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_set_segments(mi355lz4_ctx *c, int segs)
{
    if (!c || segs < -1 || segs > 64) return fail(MI355LZ4_E_ARG, "mi355lz4_set_segments: -1 (auto), 0 (off) or 2..64");
    c->segMode = segs;
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_synchronize(mi355lz4_ctx *c)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MI355LZ4_OK;
}

// 1 when the library was built with the shelved experiments (make lib-exp): the tests ask before they use variant 3.
// Not in the public header.
extern "C" int mi355lz4_debug_has_experiments(void)
{
#ifdef MI355LZ4_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}

extern "C" int mi355lz4_set_decoder(mi355lz4_ctx *c, int variant)
{
    // 0 = chosen per call, 1 = sequence at a time, 2 = lane-parallel (one wavefront per block), 4 = one workgroup per block
    // (decode_cu.hpp); 3 = the parse as a pass of its own (token lists), experiment builds only (make lib-exp)
    bool ok = c && (variant == 0 || variant == 1 || variant == 2 || variant == 4);
#ifdef MI355LZ4_EXPERIMENTS
    ok = ok || (c && variant == 3);
#endif
    if (!ok) return fail(MI355LZ4_E_ARG, "bad decoder variant");
    c->decoder = variant;
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_set_block_checksum(mi355lz4_ctx *c, int on)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    c->blockChecksum = on ? 1 : 0;
    return MI355LZ4_OK;
}

// the switch as the multi handle sees it (multi_device.cpp): its engines must agree
int mi355lz4_detail::engine_block_checksum(const mi355lz4_ctx *c) { return c ? c->blockChecksum : 0; }

extern "C" int mi355lz4_set_compression_level(mi355lz4_ctx *c, int level)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (level < 0 || level > 12) return fail(MI355LZ4_E_ARG, "compression level %d: 0..12", level);
    c->compLevel = level > 9 ? 9 : level;      // 10..12 (LZ4HC's optimal parser) search as 9
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_get_compression_level(const mi355lz4_ctx *c)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    return c->compLevel;
}

int mi355lz4_detail::engine_compression_level(const mi355lz4_ctx *c) { return c ? c->compLevel : 0; }

extern "C" int mi355lz4_set_compress_exact(mi355lz4_ctx *c, int on)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    c->compExact = on ? 1 : 0;
    if (on) c->ex = mi355lz4_ctx::ExactStream();     // switching it on starts a new stream
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_get_compress_exact(const mi355lz4_ctx *c)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    return c->compExact;
}

extern "C" int mi355lz4_compress_exact_reset(mi355lz4_ctx *c)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    c->ex = mi355lz4_ctx::ExactStream();              // LZ4_createStream: the table is zeroed by the next call
    return MI355LZ4_OK;
}

int mi355lz4_detail::engine_compress_exact(const mi355lz4_ctx *c) { return c ? c->compExact : 0; }
int mi355lz4_detail::engine_swap_compress_exact(mi355lz4_ctx *c, int on)
{
    if (!c) return 0;
    const int was = c->compExact;
    c->compExact = on;
    return was;
}

// Diagnostic hook (not part of the public header): the last exact compress call's pieces.  get (4 ints): pieces in all,
// pieces speculated (started from a zeroed table), speculated pieces whose assumption held, pieces redone.
extern "C" int mi355lz4_debug_exact_state(mi355lz4_ctx *c, int *get)
{
    if (!c || !get) return fail(MI355LZ4_E_ARG, "debug_exact_state: null argument");
    for (int i = 0; i < 4; i++) get[i] = c->ex.last[i];
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_set_linked_compress(mi355lz4_ctx *c, int on)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    c->linkedCompress = on ? 1 : 0;
    return MI355LZ4_OK;
}

// Diagnostic hook (not part of the public header): enable/read the lane-parallel decoder's
// phase counters.  enable != 0 switches the STATS kernel on (slower); out receives and resets
// PAR_STATS_COUNT counters.
extern "C" int mi355lz4_debug_stats(mi355lz4_ctx *c, int enable, unsigned long long *out)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->stats && out) HIP_TRY(hipMemcpy(out, c->stats, PAR_STATS_COUNT * 8, hipMemcpyDeviceToHost));
    if (enable && !c->stats) HIP_TRY(hipMalloc((void **)&c->stats, PAR_STATS_COUNT * 8));
    if (c->stats) HIP_TRY(hipMemset(c->stats, 0, PAR_STATS_COUNT * 8));
    if (!enable && c->stats) { hipFree(c->stats); c->stats = nullptr; }
    return MI355LZ4_OK;
}

// Diagnostic hook (not part of the public header): the run-in decode's adaptive state {longRun, longOk, skip} (RuninState) and, in
// get[3], the dictionary share the last linked call sampled (millionths; -1: none) and, in get[4], how the last linked call was
// finished (LinkedPath): 0 None, 1 Runs, 2 RunIn, 3 RunInLong, 4 RunInGivenUp, 5 Pointer, 6 Big.  get (may be null, 5 ints) receives
// it; set (may be null, 3 ints) replaces the state.  Lets a test drive default -> long -> skip -> probe.
extern "C" int mi355lz4_debug_runin_state(mi355lz4_ctx *c, int *get, const int *set)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (get) { get[0] = c->runin.longRun ? 1 : 0; get[1] = c->runin.longOk; get[2] = c->runin.skip; get[3] = c->runinShareE6; get[4] = c->linkedPath; }
    if (set) { c->runin.longRun = set[0] != 0; c->runin.longOk = set[1]; c->runin.skip = set[2]; }
    return MI355LZ4_OK;
}

// Diagnostic hook (not part of the public header): what the HIP runtime says about a kernel of the lane-parallel decode family on
// this context's device.  which: 0 k_decode_par<false>, 1 k_decode_par_redo, 2 k_decode_dict, 3 k_decode_par_partial<false>,
// 4 k_decode_par_partial<true>, 5 k_decode_dstreams, 6 k_decode_fixup_linked, 7 k_decode_fixup_runs, 8 k_runin_decode, 9 k_runin_fix,
// 10 k_decode_tolerant.  out (4 ints) = {resident workgroups per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor; a workgroup is
// one wave), static LDS bytes and registers (hipFuncGetAttributes), sizeof(ParLds)}.
extern "C" int mi355lz4_debug_kernel_info(mi355lz4_ctx *c, int which, int *out)
{
    if (!c || !out) return fail(MI355LZ4_E_ARG, "debug_kernel_info: null argument");
    HIP_TRY(hipSetDevice(c->device));
    const int r = decode_kernel_info(which, out);
    if (r == -1) return fail(MI355LZ4_E_ARG, "debug_kernel_info: unknown kernel");
    if (r != 0) HIP_TRY((hipError_t)r);
    return MI355LZ4_OK;
}

// Diagnostic hook (not part of the public header): the workgroup-per-block decoder writes 16 words per block of the
// next calls to devBuf (caller-owned device memory, 64 bytes per block; null switches it off): decode_cu.hpp, `dbg`.
extern "C" int mi355lz4_debug_cu(mi355lz4_ctx *c, uint32_t *devBuf)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    c->cuDbg = devBuf;
    return MI355LZ4_OK;
}

// Diagnostic hook (not part of the public header): what the tolerant pass of the last linked single-stream call
// left behind.  out[0] = dependent blocks that got a list, out[1] = entries in all lists, out[2] = longest
// list, out[3] = blocks whose list overflowed, out[4] = dependent blocks without a list.
extern "C" int mi355lz4_debug_tol_stats(mi355lz4_ctx *c, int nBlocks, long long *out)
{
    if (!c || !out || nBlocks <= 0 || !c->tolMeta.p) return fail(MI355LZ4_E_ARG, "debug_tol_stats: nothing to report");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<int32_t> m((size_t)nBlocks * 3 + 4);
    HIP_TRY(hipMemcpy(m.data(), c->tolMeta.p, m.size() * 4, hipMemcpyDeviceToHost));
    const int regionsUsed = m[0];
    for (int i = 0; i < 8; i++) out[i] = 0;
    // only blocks the tolerant kernel visited have meaningful entries: it hands out regions 0..regionsUsed-1
    std::vector<char> seen((size_t)(regionsUsed > 0 ? regionsUsed : 0), 0);
    for (int b = 0; b < nBlocks; b++) {
        const int reg = m[4 + (size_t)b], cnt = m[4 + (size_t)nBlocks + b];
        if (reg >= 0 && reg < regionsUsed && !seen[(size_t)reg]) {
            seen[(size_t)reg] = 1;
            out[0]++; out[1] += cnt;
            if (cnt > out[2]) out[2] = cnt;
            if (cnt > 8192) out[3]++;
        }
    }
    out[4] = regionsUsed - out[0];
    // RPL_STATS builds: rounds, super-batches, replay cycles / 16
    out[5] = (unsigned)m[1]; out[6] = (unsigned)m[2]; out[7] = (unsigned)m[3];
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_compress_bound(int n)
{
    if ((unsigned)n > (unsigned)MI355LZ4_MAX_INPUT_SIZE) return 0;
    return n + n / 255 + 16;
}

extern "C" size_t mi355lz4_slot_stride(int blockLen, int headerKind)
{
    size_t b = (size_t)mi355lz4_compress_bound(blockLen) + (size_t)headerKind;
    return (b + 15) & ~(size_t)15;
}

extern "C" size_t mi355lz4_slot_stride_ex(int blockLen, int headerKind, int blockChecksum)
{
    size_t b = (size_t)mi355lz4_compress_bound(blockLen) + (size_t)headerKind + (blockChecksum ? 4u : 0u);
    return (b + 15) & ~(size_t)15;
}

int mi355lz4_detail::check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MI355LZ4_E_HIP, "%s: %s", what, hipGetErrorString(e));
    return MI355LZ4_OK;
}

// ---------------------------------------------------------------------------
// device-resident batched API
//
// Reference-exact compression (mi355lz4_set_compress_exact; encode_exact.hpp).  The host follows the
// stream's scalar state (currentOffset, dictSize, renorms) from the lengths alone; the device holds the table and the
// dictionary bytes.  Pieces of P blocks are speculated from a zeroed table R blocks early and verified in parallel; the
// ones whose assumption failed are redone from their predecessor's true table, serially and in order.
// ---------------------------------------------------------------------------
int mi355lz4_detail::env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
}

static int exact_encode(mi355lz4_ctx *c, EncodeArgs a, const int32_t *hostLen)
{
    const int n = a.nBlocks;
    std::vector<int32_t> lens((size_t)n, a.uniformLen);
    if (hostLen) {
        std::copy(hostLen, hostLen + n, lens.begin());
    } else if (a.srcLen) {                      // the device call: the plan needs the lengths (a wait on the engine's stream)
        HIP_TRY(hipMemcpyAsync(lens.data(), a.srcLen, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    for (int j = 0; j < n; j++)
        if (lens[(size_t)j] < 0 || lens[(size_t)j] > a.uniformLen)
            return fail(MI355LZ4_E_ARG, "compress_exact: block %d length %d outside 0..maxBlockLen", j, lens[(size_t)j]);
    // cbits/lz4.c:1565-1637 with the lengths alone (kernels.h, exact_step)
    std::vector<ExactBlock> meta((size_t)n + 1);
    uint32_t cur = c->ex.cur, dictSize = c->ex.dictSize;
    for (int j = 0; j < n; j++) meta[(size_t)j] = exact_step(cur, dictSize, (uint32_t)lens[(size_t)j]);
    meta[(size_t)n] = ExactBlock{cur, dictSize, 0u, 0, 0, 0};

    // R = 0: no speculation, one serial chain
    const int R = std::max(0, env_int("MI355LZ4_EXACT_RUNIN", 12));
    int P = env_int("MI355LZ4_EXACT_PIECE", 0);
    if (P <= 0) P = std::max(4, (n + 2047) / 2048);
    if (R == 0) P = n;
    const int np = (n + P - 1) / P;
    const size_t tabBytes = (size_t)EXACT_TABLE * 4;
    int r;
    if (!c->exState.p) {                         // never grown: it holds the stream
        HIP_TRY(hipMalloc(&c->exState.p, tabBytes + 65536));
        c->exState.cap = tabBytes + 65536;
    }
    if ((r = dev_reserve(c->exMeta, ((size_t)n + 1) * sizeof(ExactBlock)))) return r;
    if ((r = dev_reserve(c->exTabs, 2 * (size_t)np * tabBytes))) return r;
    if ((r = dev_reserve(c->exFlags, (size_t)np * 4 + 64))) return r;     // eq[np]
    if (c->ex.fresh) {
        HIP_TRY(hipMemsetAsync(c->exState.p, 0, tabBytes, c->stream));
        c->ex.fresh = false;
    }
    ExactArgs x;
    x.e = a;
    x.meta = (const ExactBlock *)c->exMeta.p;
    x.dict0 = (const uint8_t *)c->exState.p + tabBytes;
    x.dict0Len = c->ex.dictBytes;
    x.state = (uint32_t *)c->exState.p;
    x.dictSave = (uint8_t *)c->exState.p + tabBytes;
    x.assumed = (uint32_t *)c->exTabs.p;
    x.finalT = (uint32_t *)c->exTabs.p + (size_t)np * EXACT_TABLE;
    x.eq = (int32_t *)c->exFlags.p;
    x.piece = P; x.runin = R; x.nPieces = np;
    HIP_TRY(hipMemcpyAsync(c->exMeta.p, meta.data(), meta.size() * sizeof(ExactBlock), hipMemcpyHostToDevice, c->stream));
    launch_exact_chain(x, 0, np, 0, c->stream);
    if ((r = check_launch("exact chain launch"))) return r;

    // which pieces started from the stream's true state (exact by construction), which were speculated
    std::vector<char> exactStart((size_t)np);
    int speculated = 0, redone = 0;
    for (int p = 0; p < np; p++) {
        exactStart[(size_t)p] = (p == 0 || p * P - R <= 0) ? 1 : 0;
        if (!exactStart[(size_t)p]) speculated++;
    }
    std::vector<int32_t> eq((size_t)np, 0);
    if (speculated) {
        launch_exact_verify(x, 1, np - 1, c->stream);
        if ((r = check_launch("exact verify launch"))) return r;
        HIP_TRY(hipMemcpyAsync(eq.data(), x.eq, (size_t)np * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    // In order: piece p is exact when it started from the true state, or piece p-1 is exact and p's assumed table is
    // p-1's final one (eq[p]).  The first piece that is neither is redone from p-1's final table, which makes it exact,
    // and the comparison of its successor is repeated against the new final table.  One piece per round, one wait.
    for (int p = 1; p < np; p++) {
        if (exactStart[(size_t)p] || eq[(size_t)p]) continue;
        launch_exact_chain(x, p, 1, 1, c->stream);
        const bool check = p + 1 < np && !exactStart[(size_t)p + 1];
        if (check) launch_exact_verify(x, p + 1, 1, c->stream);
        if ((r = check_launch("exact redo launch"))) return r;
        if (check) {
            HIP_TRY(hipMemcpyAsync(&eq[(size_t)p + 1], x.eq + p + 1, 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        redone++;
    }
    launch_exact_finish(x, c->stream);
    if ((r = check_launch("exact finish launch"))) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));     // meta is a host vector of this frame
    c->ex.cur = cur;
    c->ex.dictSize = dictSize;
    c->ex.dictBytes = (int)std::min<uint32_t>((uint32_t)lens[(size_t)n - 1], 65536u);
    c->ex.last[0] = np; c->ex.last[1] = speculated; c->ex.last[2] = speculated - redone; c->ex.last[3] = redone;
    return MI355LZ4_OK;
}

// LZ4_compress_fast_continue's clamp (cbits/lz4.c:1577-1578), for every call that takes accel
static int accel_clamped(int accel) { return accel < 1 ? 1 : (accel > 65537 ? 65537 : accel); }

EncodeArgs mi355lz4_detail::make_encode_args(const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride,
                                             int maxBlockLen, int nBlocks, int accel, int headerKind, uint8_t *slots,
                                             size_t slotStride, int32_t *framedLen)
{
    return EncodeArgs{src, srcOff, srcLen, blockStride, maxBlockLen, nBlocks, accel_clamped(accel), headerKind, slots, slotStride,
                      framedLen, nullptr, 0, 0};
}

// The argument contract of a device batch, written once for the four entry points; `who` names the caller in the messages.  In two
// halves, because the empty call returns between them (and the HC dictionary call's own limit comes in front of that):
// batch_shape_check the counts, the header kind and the block length against the call's limit, batch_buffers_check the pointers
// and the slot stride against bound + header + trailer.
static int batch_shape_check(const char *who, int nBlocks, int headerKind, int maxBlockLen, int limit)
{
    if (nBlocks < 0 || (headerKind != 4 && headerKind != 8) || maxBlockLen < 0 || (unsigned)maxBlockLen > (unsigned)limit)
        return fail(MI355LZ4_E_ARG, "%s: bad arguments", who);
    return MI355LZ4_OK;
}
// The shape check of the calls that stage every block behind a dictionary (the HC and the fast dictionary batch, the dictionary
// set, the fast streams; device and host-buffer forms): no block length is "bad" here but a negative one, and the limit of
// HCDICT_MAX_BLOCK has its own message, in front of the empty call.  `what` names what takes the bytes.
int mi355lz4_detail::dict_batch_shape_check(const char *who, const char *what, int nBlocks, int headerKind, int maxBlockLen)
{
    if (int r = batch_shape_check(who, nBlocks, headerKind, maxBlockLen, INT_MAX)) return r;
    if (maxBlockLen > HCDICT_MAX_BLOCK)
        return fail(MI355LZ4_E_ARG, "%s: maxBlockLen %d above the %d bytes %s takes", who, maxBlockLen, HCDICT_MAX_BLOCK, what);
    return MI355LZ4_OK;
}
static int batch_buffers_check(const mi355lz4_ctx *c, const char *who, const uint8_t *src, int maxBlockLen, int headerKind,
                               const uint8_t *slots, size_t slotStride, const int32_t *framedLen)
{
    if (!src && maxBlockLen > 0) return fail(MI355LZ4_E_ARG, "%s: null src", who);
    if (!slots || !framedLen) return fail(MI355LZ4_E_ARG, "%s: null output", who);
    if (slotStride < (size_t)mi355lz4_compress_bound(maxBlockLen) + (size_t)headerKind + (c->blockChecksum ? 4u : 0u))
        return fail(MI355LZ4_E_CAPACITY, "%s: slotStride %zu < bound", who, slotStride);
    return MI355LZ4_OK;
}

// Behind an encoder's launch.  encode_trailers: with block checksums on, the trailers go behind the encoder's output, on the same
// stream, before anything reads framedLen.  encode_launched: the launch checked first (`what` names it for check_launch).
static int encode_trailers(mi355lz4_ctx *c, const EncodeArgs &a)
{
    if (!c->blockChecksum) return MI355LZ4_OK;
    launch_xxh32_append(a.slots, a.slotStride, a.headerKind, a.framedLen, a.nBlocks, c->stream);
    return check_launch("checksum launch");
}
static int encode_launched(mi355lz4_ctx *c, const EncodeArgs &a, const char *what)
{
    if (int r = check_launch(what)) return r;
    return encode_trailers(c, a);
}

// One scratch per stream the engine has been used on, `count` of the four slots so far: the slot of the engine's current stream,
// else a free one, else the one used longest ago -- *takeOver then says that it is still another stream's, and the caller waits
// for slot->s by its own rule before the slot changes hands.
static mi355lz4_ctx::SegScratch *scratch_slot(mi355lz4_ctx *c, mi355lz4_ctx::SegScratch *slots, int &count, bool *takeOver)
{
    *takeOver = false;
    for (int i = 0; i < count; i++) if (slots[i].s == c->stream) return &slots[i];
    if (count < 4) return &slots[count++];
    mi355lz4_ctx::SegScratch *slot = &slots[0];
    for (int i = 1; i < count; i++) if (slots[i].tick < slot->tick) slot = &slots[i];
    *takeOver = true;
    return slot;
}

int mi355lz4_detail::encode_device(mi355lz4_ctx *c, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                   uint64_t blockStride, int maxBlockLen, int nBlocks, int accel, int headerKind, uint8_t *slots,
                                   size_t slotStride, int32_t *framedLen, int lookBack, const int32_t *hostLen)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (int r = batch_shape_check("compress_batch_device", nBlocks, headerKind, maxBlockLen, MI355LZ4_MAX_INPUT_SIZE)) return r;
    if (nBlocks == 0) return MI355LZ4_OK;
    if (int r = batch_buffers_check(c, "compress_batch_device", src, maxBlockLen, headerKind, slots, slotStride, framedLen)) return r;
    HIP_TRY(hipSetDevice(c->device));
    EncodeArgs a = make_encode_args(src, srcOff, srcLen, blockStride, maxBlockLen, nBlocks, accel, headerKind, slots, slotStride, framedLen);
    a.stats = c->stats; a.linked = c->linkedCompress; a.lookBack = lookBack;
    auto finish = [&]() -> int { return encode_launched(c, a, "encode launch"); };
    // the reference-exact stream: its own chain of kernels, whatever the linked switch says
    if (c->compExact) {
        if (c->compLevel != 0)
            return fail(MI355LZ4_E_ARG, "compress_exact: compression level %d; the exact mode is level 0's encoder", c->compLevel);
        if (c->segMode > 0)
            return fail(MI355LZ4_E_ARG, "compress_exact: forced segments (mi355lz4_set_segments %d) cannot give the reference's bytes", c->segMode);
        const int r = exact_encode(c, a, hostLen);
        return r ? r : finish();
    }
    // compression levels 1..12: the hash-chain encoder, every block size, linked or not; accel does not apply (as in LZ4HC)
    if (c->compLevel > 0) {
        launch_encode_hc(a, c->compLevel, c->stream);
        return finish();
    }
    // Small batches: with fewer blocks than the chip has wave slots (256 CUs x 16), a block is cut into segments that
    // several waves compress at once (kernels/encode.inc, "K2, small batches").  Segments of >= 4 KiB, at most 64 per block,
    // about two waves per slot in all; blocks of up to 4 MiB (24-bit positions in the records); independent blocks only.
    // MI355LZ4_SEG=0 turns it off, MI355LZ4_SEG=k forces k segments (tests).
    {
        static const int segEnv0 = [] { const char *e = getenv("MI355LZ4_SEG"); return e ? atoi(e) : -1; }();
        const int segEnv = c->segMode >= 0 ? c->segMode : segEnv0;
        int segs = 0;
        if (!a.linked && maxBlockLen >= 8192 && maxBlockLen <= (4 << 20) && segEnv != 0) {
            const long slots_ = 2L * 256 * 16;
            long want = segEnv > 0 ? segEnv : slots_ / (long)nBlocks;
            if (want > maxBlockLen / 4096) want = maxBlockLen / 4096;
            if (want > 64) want = 64;
            if (want >= 2) segs = (int)want;
        }
        if (segs >= 2) {
            EncodeSegArgs sa;
            sa.e = a;
            sa.segs = segs;
            sa.segLen = ((maxBlockLen + segs - 1) / segs + 63) & ~63;
            sa.listStride = (size_t)maxBlockLen / 4 + (size_t)segs + 2;
            const size_t listBytes = (size_t)nBlocks * sa.listStride * sizeof(uint64_t);
            const size_t cntBytes = (size_t)nBlocks * (size_t)segs * sizeof(uint32_t);
            // The record lists are twice the input.  Automatic mode only takes the segment path while they stay under
            // SEG_SCRATCH_MAX (a call of 2048 x 4 MiB would otherwise pin 20 GiB per stream until mi355lz4_destroy:
            // round-3 advisor finding); a forced count (tests, mi355lz4_set_segments(k)) is the caller's decision.
            const size_t SEG_SCRATCH_MAX = (size_t)1 << 30;
            const bool fits = segEnv > 0 || listBytes + 3 * cntBytes <= SEG_SCRATCH_MAX;
            // One scratch per stream the engine has been used on, four at the most: a fifth stream takes over the slot
            // that was used longest ago, once the work queued on that slot's stream is done with it.
            mi355lz4_ctx::SegScratch *slot = nullptr;
            if (fits) {
                bool takeOver;
                slot = scratch_slot(c, c->seg, c->nSeg, &takeOver);
                if (takeOver) (void)hipStreamSynchronize(slot->s);
                slot->s = c->stream;
                slot->tick = ++c->segTick;
                // a scratch that a big forced call left behind is given back when a call needs less than a quarter of it
                if (slot->b.cap > SEG_SCRATCH_MAX && (listBytes + 3 * cntBytes + 256) * 4 < slot->b.cap) {
                    (void)hipStreamSynchronize(slot->s);
                    dev_release(slot->b);
                }
            }
            DevBuf *sb = slot ? &slot->b : nullptr;
            if (sb && dev_reserve(*sb, listBytes + 3 * cntBytes + 256) == 0) {
                sa.lists = (uint64_t *)sb->p;
                sa.segCount = (uint32_t *)((uint8_t *)sb->p + ((listBytes + 63) & ~(size_t)63));
                sa.segBytes = sa.segCount + (size_t)nBlocks * (size_t)segs;
                sa.segPrevEnd = (int32_t *)(sa.segBytes + (size_t)nBlocks * (size_t)segs);
                launch_encode_seg(sa, c->stream);
                return finish();
            }
            (void)hipGetLastError();          // no scratch: the one-wave-per-block path needs none
        }
    }
    launch_encode(a, maxBlockLen > 65536, c->stream);
    return finish();
}

extern "C" int mi355lz4_compress_batch_device(mi355lz4_ctx *c, const uint8_t *src, const uint64_t *srcOff,
                                              const int32_t *srcLen, uint64_t blockStride, int maxBlockLen,
                                              int nBlocks, int accel, int headerKind, uint8_t *slots,
                                              size_t slotStride, int32_t *framedLen)
{
    return encode_device(c, src, srcOff, srcLen, blockStride, maxBlockLen, nBlocks, accel, headerKind, slots, slotStride,
                         framedLen, 0);
}

// ---------------------------------------------------------------------------
// Many reference-exact streams in one call (mi355lz4_cstreams, mi355lz4_compress_streams_device).  A slot of
// the set is a whole LZ4_stream_t on the device -- table, scalars, the previous array's last 64 KiB (kernels.h,
// CSTREAM_*) -- and k_exact_streams follows the scalars itself, so the host never reads a length and never waits.
// The small per-call table {first block, end block, slot} per stream goes through a ring of pinned buffers: an entry is
// reused once the launch that read it is done (four calls may be in flight before a call waits for the oldest).
// ---------------------------------------------------------------------------
// (StreamTableRing, SlotSet and the three sets built on it: engine.hpp)

template <class Set>
static int slots_create(mi355lz4_ctx *c, int nSlots, size_t slotBytes, Set **out, const char *who)
{
    if (out) *out = nullptr;
    if (!c || !out || nSlots < 1) return fail(MI355LZ4_E_ARG, "%s: bad arguments", who);
    HIP_TRY(hipSetDevice(c->device));
    Set *s = new (std::nothrow) Set();
    if (!s) return fail(MI355LZ4_E_ARG, "out of host memory");
    s->device = c->device;
    s->nSlots = nSlots;
    const size_t bytes = (size_t)nSlots * slotBytes;
    hipError_t e = hipMalloc((void **)&s->state, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(s->state, 0, bytes, c->stream);      // every slot reset (LZ4_resetStream; no dictionary)
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);                    // (whatever stream the engine is on later)
    if (e != hipSuccess) {
        if (s->state) hipFree(s->state);
        delete s;
        return fail(MI355LZ4_E_HIP, "%s: %d slots (%zu bytes): %s", who, nSlots, bytes, hipGetErrorString(e));
    }
    *out = s;
    return MI355LZ4_OK;
}
template <class Set>
static void slots_destroy(Set *s)
{
    if (!s) return;
    hipSetDevice(s->device);
    hipDeviceSynchronize();                 // calls that still use the slots
    s->table.release();
    if (s->state) hipFree(s->state);
    delete s;
}
static int slots_count(const SlotSet *s, const char *who) { return s ? s->nSlots : fail(MI355LZ4_E_ARG, "%s: null set", who); }
// an object of the engine's device (a set of slots, a prepared dictionary, a dictionary set): `what` names it in the message
template <class Obj>
static int same_device(const mi355lz4_ctx *c, const Obj *o, const char *who, const char *what = "set")
{
    if (!c || !o) return fail(MI355LZ4_E_ARG, "%s: null argument", who);
    if (o->device != c->device) return fail(MI355LZ4_E_ARG, "%s: the %s lives on device %d, the engine on %d", who, what, o->device, c->device);
    return MI355LZ4_OK;
}
static int slot_range_check(const SlotSet *s, int slot, const char *who)
{
    if (slot < 0 || slot >= s->nSlots) return fail(MI355LZ4_E_ARG, "%s: slot %d of %d", who, slot, s->nSlots);
    return MI355LZ4_OK;
}
// the arguments of a _reset: the set on the engine's device and, with a list, every slot of it in range
static int slots_reset_check(const mi355lz4_ctx *c, const SlotSet *s, const int32_t *slots, int n, const char *who)
{
    if (int r = same_device(c, s, who)) return r;
    HIP_TRY(hipSetDevice(c->device));
    if (!slots) return MI355LZ4_OK;
    if (n < 0) return fail(MI355LZ4_E_ARG, "%s: bad count", who);
    for (int i = 0; i < n; i++)
        if (slots[i] < 0 || slots[i] >= s->nSlots) return fail(MI355LZ4_E_ARG, "%s: slot %d out of range", who, slots[i]);
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_cstreams_create(mi355lz4_ctx *c, int nSlots, mi355lz4_cstreams **out)
{
    return slots_create(c, nSlots, CSTREAM_SLOT_BYTES, out, "cstreams_create");
}
extern "C" void mi355lz4_cstreams_destroy(mi355lz4_cstreams *cs) { slots_destroy(cs); }
extern "C" int mi355lz4_cstreams_count(const mi355lz4_cstreams *cs) { return slots_count(cs, "cstreams_count"); }

extern "C" int mi355lz4_cstreams_reset(mi355lz4_ctx *c, mi355lz4_cstreams *cs, const int32_t *slots, int n)
{
    if (int r = slots_reset_check(c, cs, slots, n, "cstreams_reset")) return r;
    if (!slots) {
        HIP_TRY(hipMemsetAsync(cs->state, 0, (size_t)cs->nSlots * CSTREAM_SLOT_BYTES, c->stream));
        return MI355LZ4_OK;
    }
    for (int i = 0; i < n; i++)             // the table and the scalars: a dictionary of 0 bytes needs no bytes cleared
        HIP_TRY(hipMemsetAsync(cs->state + (size_t)slots[i] * CSTREAM_SLOT_BYTES, 0, CSTREAM_DICT_OFF, c->stream));
    return MI355LZ4_OK;
}

// Diagnostic hook (not part of the public header): slot `slot`'s scalars.  get (3 words, may be null): currentOffset, dictSize,
// saved dictionary bytes, after everything queued on the device has run.  A non-null setCurrentOffset then overwrites
// currentOffset (the tests reach the 2 GiB renorm with it).
extern "C" int mi355lz4_debug_cstream_state(mi355lz4_cstreams *cs, int slot, uint32_t *get, const uint32_t *setCurrentOffset)
{
    if (!cs || slot < 0 || slot >= cs->nSlots) return fail(MI355LZ4_E_ARG, "debug_cstream_state: bad arguments");
    HIP_TRY(hipSetDevice(cs->device));
    HIP_TRY(hipDeviceSynchronize());
    uint8_t *scal = cs->state + (size_t)slot * CSTREAM_SLOT_BYTES + CSTREAM_SCALAR_OFF;
    if (get) HIP_TRY(hipMemcpy(get, scal, 12, hipMemcpyDeviceToHost));
    if (setCurrentOffset) HIP_TRY(hipMemcpy(scal, setCurrentOffset, 4, hipMemcpyHostToDevice));
    return MI355LZ4_OK;
}

// Diagnostic hook (not part of the public header): slot `slot` as it is after everything queued on the device has run, all
// CSTREAM_SLOT_BYTES of it (table, scalars, saved bytes) into bytes (host memory).  The tests compare a loaded slot with
// LZ4_loadDict's state and show that a shared slot is never written.
extern "C" int mi355lz4_debug_cstream_slot(mi355lz4_cstreams *cs, int slot, uint8_t *bytes)
{
    if (!cs || !bytes || slot < 0 || slot >= cs->nSlots) return fail(MI355LZ4_E_ARG, "debug_cstream_slot: bad arguments");
    HIP_TRY(hipSetDevice(cs->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(bytes, cs->state + (size_t)slot * CSTREAM_SLOT_BYTES, CSTREAM_SLOT_BYTES, hipMemcpyDeviceToHost));
    return MI355LZ4_OK;
}

// the stream table of a call, checked: ascending over [0, nBlocks], every slot in range and named once
static int stream_table_check(int nSlots, int nBlocks, const int32_t *streamFirst, const int32_t *streamSlot, int nStreams,
                              const char *who)
{
    if (nBlocks < 0 || nStreams < 0 || !streamFirst || (nStreams > 0 && !streamSlot)) return fail(MI355LZ4_E_ARG, "%s: bad stream table", who);
    if (streamFirst[0] != 0 || streamFirst[nStreams] != nBlocks)
        return fail(MI355LZ4_E_ARG, "%s: the streams do not cover blocks 0..%d", who, nBlocks);
    std::vector<char> seen((size_t)nSlots, 0);
    for (int s = 0; s < nStreams; s++) {
        if (streamFirst[s + 1] < streamFirst[s]) return fail(MI355LZ4_E_ARG, "%s: stream table is not ascending at %d", who, s);
        const int k = streamSlot[s];
        if (k < 0 || k >= nSlots) return fail(MI355LZ4_E_ARG, "%s: stream %d names slot %d of %d", who, s, k, nSlots);
        if (seen[(size_t)k]) return fail(MI355LZ4_E_ARG, "%s: slot %d is named twice", who, k);
        seen[(size_t)k] = 1;
    }
    return MI355LZ4_OK;
}

// the checks both compress-side sets share (mi355lz4_cstreams, mi355lz4_fstreams): the set on the engine's device, level 0, the table
// over the set's nSlots slots.  `what` names the form in the level's message.
static int compress_streams_check(const mi355lz4_ctx *c, const SlotSet *s, int nSlots, int nBlocks, const int32_t *streamFirst,
                                  const int32_t *streamSlot, int nStreams, const char *who, const char *what)
{
    if (int r = same_device(c, s, who)) return r;
    if (c->compLevel != 0)
        return fail(MI355LZ4_E_ARG, "%s: compression level %d; %s streams are level 0's encoder", who, c->compLevel, what);
    return stream_table_check(nSlots, nBlocks, streamFirst, streamSlot, nStreams, who);
}

int mi355lz4_detail::streams_check(const mi355lz4_ctx *c, const mi355lz4_cstreams *cs, int nBlocks, const int32_t *streamFirst,
                                   const int32_t *streamSlot, int nStreams, const char *who)
{
    return compress_streams_check(c, cs, cs ? cs->nSlots : 0, nBlocks, streamFirst, streamSlot, nStreams, who, "exact");
}

int mi355lz4_detail::fstreams_check(const mi355lz4_ctx *c, const mi355lz4_fstreams *fs, int nBlocks, const int32_t *streamFirst,
                                    const int32_t *streamSlot, int nStreams, const char *who)
{
    return compress_streams_check(c, fs, fs ? fs->nSlots : 0, nBlocks, streamFirst, streamSlot, nStreams, who, "fast");
}

// The upload: {first block, end block, slot} per stream with blocks in [b0, b1), relative to b0, longer parts first, through
// the next entry of the set's ring.
// *nWork = 0: nothing to launch.  The caller launches the kernel that reads *workDev, then calls stream_table_launched.
static int stream_table_upload(mi355lz4_ctx *c, StreamTableRing &t, int b0, int b1, const int32_t *streamFirst,
                               const int32_t *streamSlot, int nStreams, const int32_t **workDev, int *nWorkOut,
                               StreamTableRing::Ring **used)
{
    *nWorkOut = 0;
    std::vector<int32_t> work;
    {
        std::vector<std::pair<int, int>> order;         // (-blocks, stream)
        for (int s = 0; s < nStreams; s++) {
            const int lo = std::max(streamFirst[s], b0), hi = std::min(streamFirst[s + 1], b1);
            if (hi > lo) order.push_back({lo - hi, s});
        }
        std::stable_sort(order.begin(), order.end(), [](const std::pair<int, int> &x, const std::pair<int, int> &y) { return x.first < y.first; });
        work.reserve(order.size() * 3);
        for (const auto &o : order) {
            const int s = o.second;
            work.push_back(std::max(streamFirst[s], b0) - b0);
            work.push_back(std::min(streamFirst[s + 1], b1) - b0);
            work.push_back(streamSlot[s]);
        }
    }
    const int nWork = (int)(work.size() / 3);
    if (nWork == 0) return MI355LZ4_OK;
    StreamTableRing::Ring &r = t.ring[t.next];
    t.next = (t.next + 1) & 3;
    if (r.busy) HIP_TRY(hipEventSynchronize(r.ev));      // the launch that last read this entry (four calls back)
    r.busy = false;
    if (!r.ev) HIP_TRY(hipEventCreateWithFlags(&r.ev, hipEventDisableTiming));
    int rc;
    if ((rc = pin_reserve(r.pin, work.size() * 4)) || (rc = dev_reserve(r.dev, work.size() * 4))) return rc;
    memcpy(r.pin.p, work.data(), work.size() * 4);
    HIP_TRY(hipMemcpyAsync(r.dev.p, r.pin.p, work.size() * 4, hipMemcpyHostToDevice, c->stream));
    *workDev = (const int32_t *)r.dev.p;
    *nWorkOut = nWork;
    *used = &r;
    return MI355LZ4_OK;
}
static int stream_table_launched(mi355lz4_ctx *c, StreamTableRing::Ring *r)
{
    HIP_TRY(hipEventRecord(r->ev, c->stream));
    r->busy = true;
    return MI355LZ4_OK;
}

// Enqueue the streams' parts that fall into blocks [b0, b1) of the table (a.* describes exactly those blocks): a stream cut
// by b0 or b1 simply continues its slot in the next launch.  Longer parts go first: the launch ends with its longest chain.
int mi355lz4_detail::streams_enqueue(mi355lz4_ctx *c, mi355lz4_cstreams *cs, const EncodeArgs &a, int b0, int b1,
                                     const int32_t *streamFirst, const int32_t *streamSlot, int nStreams)
{
    ExactStreamsArgs x;
    int nWork = 0, rc;
    StreamTableRing::Ring *used = nullptr;
    if ((rc = stream_table_upload(c, cs->table, b0, b1, streamFirst, streamSlot, nStreams, &x.work, &nWork, &used))) return rc;
    if (nWork == 0) return MI355LZ4_OK;
    x.e = a;
    x.state = cs->state;
    launch_exact_streams(x, nWork, c->stream);
    if ((rc = check_launch("exact streams launch"))) return rc;
    if ((rc = stream_table_launched(c, used))) return rc;       // (the ring entry is busy from here on, whatever the trailers do)
    return encode_trailers(c, a);
}

extern "C" int mi355lz4_compress_streams_device(mi355lz4_ctx *c, mi355lz4_cstreams *cs, const uint8_t *src,
                                                const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride,
                                                int maxBlockLen, int nBlocks, const int32_t *streamFirst,
                                                const int32_t *streamSlot, int nStreams, int accel, int headerKind,
                                                uint8_t *slots, size_t slotStride, int32_t *framedLen)
{
    int r = streams_check(c, cs, nBlocks, streamFirst, streamSlot, nStreams, "compress_streams_device");
    if (r) return r;
    // (nBlocks < 0 has gone to the stream-table check above)
    if ((r = batch_shape_check("compress_streams_device", nBlocks, headerKind, maxBlockLen, MI355LZ4_MAX_INPUT_SIZE))) return r;
    if (nBlocks == 0) return MI355LZ4_OK;
    if ((r = batch_buffers_check(c, "compress_streams_device", src, maxBlockLen, headerKind, slots, slotStride, framedLen))) return r;
    HIP_TRY(hipSetDevice(c->device));
    const EncodeArgs a = make_encode_args(src, srcOff, srcLen, blockStride, maxBlockLen, nBlocks, accel, headerKind, slots, slotStride, framedLen);
    return streams_enqueue(c, cs, a, 0, nBlocks, streamFirst, streamSlot, nStreams);
}

// ---------------------------------------------------------------------------
// Shared-dictionary batches.  mi355lz4_cstreams_load_dict is LZ4_loadDict on one slot of a set, on the device;
// mi355lz4_compress_dict_device compresses every block of a batch from a copy of that slot (k_exact_dict: one wave per block,
// the slot read-only), so the same loaded slot serves any number of calls.  Both only enqueue.
// ---------------------------------------------------------------------------
extern "C" int mi355lz4_cstreams_load_dict(mi355lz4_ctx *c, mi355lz4_cstreams *cs, int slot, const uint8_t *dictDevice, int len)
{
    if (int r = same_device(c, cs, "cstreams_load_dict")) return r;
    if (int r = slot_range_check(cs, slot, "cstreams_load_dict")) return r;
    if (len < 0 || (len > 0 && !dictDevice)) return fail(MI355LZ4_E_ARG, "cstreams_load_dict: bad dictionary");
    HIP_TRY(hipSetDevice(c->device));
    launch_cstreams_load_dict(cs->state + (size_t)slot * CSTREAM_SLOT_BYTES, dictDevice, len, c->stream);
    return check_launch("cstreams load_dict launch");
}

extern "C" int mi355lz4_compress_dict_device(mi355lz4_ctx *c, const mi355lz4_cstreams *cs, int dictSlot, const uint8_t *src,
                                             const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride,
                                             int maxBlockLen, int nBlocks, int accel, int headerKind, uint8_t *slots,
                                             size_t slotStride, int32_t *framedLen)
{
    if (int r = same_device(c, cs, "compress_dict_device")) return r;
    if (c->compLevel != 0)
        return fail(MI355LZ4_E_ARG, "compress_dict_device: compression level %d; the dictionary batch is level 0's encoder", c->compLevel);
    if (int r = slot_range_check(cs, dictSlot, "compress_dict_device")) return r;
    if (int r = batch_shape_check("compress_dict_device", nBlocks, headerKind, maxBlockLen, MI355LZ4_MAX_INPUT_SIZE)) return r;
    if (nBlocks == 0) return MI355LZ4_OK;
    if (int r = batch_buffers_check(c, "compress_dict_device", src, maxBlockLen, headerKind, slots, slotStride, framedLen)) return r;
    HIP_TRY(hipSetDevice(c->device));
    ExactDictArgs x;
    x.e = make_encode_args(src, srcOff, srcLen, blockStride, maxBlockLen, nBlocks, accel, headerKind, slots, slotStride, framedLen);
    x.state = cs->state + (size_t)dictSlot * CSTREAM_SLOT_BYTES;
    launch_exact_dict(x, c->stream);
    return encode_launched(c, x.e, "exact dict launch");
}

// ---------------------------------------------------------------------------
// Fixed-size output pages: LZ4_compress_destSize for a batch, and chains of such pages per input (k_exact_pages:
// one wave per input, every page from a zeroed table).  Enqueues only; srcLen and pageSize stay unread on the host.
// ---------------------------------------------------------------------------
// (the three page calls' arguments in one place: pages_args makes the kernels' struct of them, pages_check holds it to the calls'
// contract, `who` naming the caller in the messages -- the counts, the header kind and the stride; no block checksums; level 0 for
// the wave encoder's forms, `fastKind` naming theirs ("fast", "dictionary"; null: the exact form, any level); then, behind the empty
// call, which the caller returns from as well, the nine pointers)
static PagesArgs pages_args(const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen, int nInputs, const int32_t *pageSize,
                            int maxPages, int headerKind, uint8_t *pages, size_t pageStride, int32_t *pageSrcLen,
                            int32_t *pageCompLen, int32_t *nPages, int32_t *consumed)
{
    return PagesArgs{src, srcOff, srcLen, nInputs, pageSize, maxPages, headerKind, pages, pageStride, pageSrcLen, pageCompLen, nPages, consumed};
}
static int pages_check(const mi355lz4_ctx *c, const char *who, const char *fastKind, const PagesArgs &x)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (x.nInputs < 0 || x.maxPages < 1 || (x.headerKind != 0 && x.headerKind != 4 && x.headerKind != 8) || x.pageStride < (size_t)x.headerKind + 1)
        return fail(MI355LZ4_E_ARG, "%s: bad arguments", who);
    if (c->blockChecksum) return fail(MI355LZ4_E_ARG, "%s: block checksums are on; pages carry no trailer", who);
    if (fastKind && c->compLevel != 0)
        return fail(MI355LZ4_E_ARG, "%s: compression level %d; %s pages are level 0's encoder", who, c->compLevel, fastKind);
    if (x.nInputs == 0) return MI355LZ4_OK;
    if (!x.src || !x.srcOff || !x.srcLen || !x.pageSize || !x.pages || !x.pageSrcLen || !x.pageCompLen || !x.nPages || !x.consumed)
        return fail(MI355LZ4_E_ARG, "%s: null pointer", who);
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_compress_pages_device(mi355lz4_ctx *c, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                              int nInputs, const int32_t *pageSize, int maxPages, int headerKind,
                                              uint8_t *pages, size_t pageStride, int32_t *pageSrcLen, int32_t *pageCompLen,
                                              int32_t *nPages, int32_t *consumed)
{
    const PagesArgs x = pages_args(src, srcOff, srcLen, nInputs, pageSize, maxPages, headerKind, pages, pageStride, pageSrcLen, pageCompLen, nPages, consumed);
    if (int r = pages_check(c, "compress_pages_device", nullptr, x)) return r;
    if (nInputs == 0) return MI355LZ4_OK;
    HIP_TRY(hipSetDevice(c->device));
    launch_exact_pages(x, c->stream);
    return check_launch("exact pages launch");
}

// The same chains at the engine's speed: every page by the wave encoder with an output budget (k_pages_fast), this
// engine's bytes and not LZ4_compress_destSize's.  Level 0 only; accel is added.
extern "C" int mi355lz4_compress_pages_fast_device(mi355lz4_ctx *c, const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                                   int nInputs, const int32_t *pageSize, int maxPages, int accel, int headerKind,
                                                   uint8_t *pages, size_t pageStride, int32_t *pageSrcLen, int32_t *pageCompLen,
                                                   int32_t *nPages, int32_t *consumed)
{
    const PagesFastArgs x{pages_args(src, srcOff, srcLen, nInputs, pageSize, maxPages, headerKind, pages, pageStride, pageSrcLen, pageCompLen, nPages, consumed),
                          accel_clamped(accel)};
    if (int r = pages_check(c, "compress_pages_fast_device", "fast", x.p)) return r;
    if (nInputs == 0) return MI355LZ4_OK;
    HIP_TRY(hipSetDevice(c->device));
    launch_pages_fast(x, c->stream);
    return check_launch("fast pages launch");
}

// ---------------------------------------------------------------------------
// High-compression levels against a shared dictionary.  A mi355lz4_hcdict is the device image of encode_hc.hpp's
// tables after the dictionary's inserts (k_hcdict_build, once per load); mi355lz4_compress_hcdict_device reloads it for every
// block (k_encode_hc_dict) and only reads it, so one object serves any number of calls.  Both only enqueue.
// ---------------------------------------------------------------------------
extern "C" int mi355lz4_hcdict_create(mi355lz4_ctx *c, mi355lz4_hcdict **out)
{
    if (out) *out = nullptr;
    if (!c || !out) return fail(MI355LZ4_E_ARG, "hcdict_create: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    mi355lz4_hcdict *hd = new (std::nothrow) mi355lz4_hcdict();
    if (!hd) return fail(MI355LZ4_E_ARG, "out of host memory");
    hd->device = c->device;
    hipError_t e = hipMalloc((void **)&hd->image, HCDICT_IMAGE_BYTES);
    if (e == hipSuccess) e = hipMalloc((void **)&hd->fastImage, FASTDICT_IMAGE_BYTES);
    // an empty dictionary until the first load: empty heads, keep 0 (no kernel: two memsets, and the wait slots_create has);
    // the wave encoder's image of it is an empty table, keep 0
    if (e == hipSuccess) e = hipMemsetAsync(hd->image, 0, HCDICT_IMAGE_BYTES, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(hd->image + HCDICT_CHAIN_BYTES, 0xFF, (size_t)HCDICT_HEAD_ENTRIES * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(hd->fastImage, 0, FASTDICT_IMAGE_BYTES, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        if (hd->image) hipFree(hd->image);
        if (hd->fastImage) hipFree(hd->fastImage);
        delete hd;
        return fail(MI355LZ4_E_HIP, "hcdict_create: %zu bytes: %s", (size_t)HCDICT_IMAGE_BYTES, hipGetErrorString(e));
    }
    *out = hd;
    return MI355LZ4_OK;
}

extern "C" void mi355lz4_hcdict_destroy(mi355lz4_hcdict *hd)
{
    if (!hd) return;
    hipSetDevice(hd->device);
    hipDeviceSynchronize();                 // calls that still read the image
    if (hd->image) hipFree(hd->image);
    if (hd->fastImage) hipFree(hd->fastImage);
    delete hd;
}

extern "C" int mi355lz4_hcdict_size(const mi355lz4_hcdict *hd) { return hd ? hd->keep : fail(MI355LZ4_E_ARG, "hcdict_size: null object"); }

extern "C" int mi355lz4_hcdict_load(mi355lz4_ctx *c, mi355lz4_hcdict *hd, const uint8_t *dictDevice, int len)
{
    if (int r = same_device(c, hd, "hcdict_load", "dictionary")) return r;
    if (len < 0 || (len > 0 && !dictDevice)) return fail(MI355LZ4_E_ARG, "hcdict_load: bad dictionary");
    HIP_TRY(hipSetDevice(c->device));
    launch_hcdict_build(hd->image, dictDevice, len, c->stream);
    if (int r = check_launch("hcdict build launch")) return r;
    launch_hcdict_build_fast(hd->fastImage, dictDevice, len, c->stream);
    if (int r = check_launch("hcdict fast build launch")) return r;
    hd->keep = len < 65536 ? len : 65536;
    return MI355LZ4_OK;
}

// Diagnostic hook (not part of the public header): the object's whole device image (HCDICT_IMAGE_BYTES: chain, head, count,
// bytes) into bytes (host memory), after everything queued on the device has run.  The tests show with it that compress calls
// never write the image.
extern "C" int mi355lz4_debug_hcdict_image(mi355lz4_hcdict *hd, uint8_t *bytes)
{
    if (!hd || !bytes) return fail(MI355LZ4_E_ARG, "debug_hcdict_image: bad arguments");
    HIP_TRY(hipSetDevice(hd->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(bytes, hd->image, HCDICT_IMAGE_BYTES, hipMemcpyDeviceToHost));
    return MI355LZ4_OK;
}

// ... and the wave encoder's image (FASTDICT_IMAGE_BYTES: the table, then keep and the first seam step) the same way
extern "C" int mi355lz4_debug_hcdict_fast_image(mi355lz4_hcdict *hd, uint8_t *bytes)
{
    if (!hd || !bytes) return fail(MI355LZ4_E_ARG, "debug_hcdict_fast_image: bad arguments");
    HIP_TRY(hipSetDevice(hd->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(bytes, hd->fastImage, FASTDICT_IMAGE_BYTES, hipMemcpyDeviceToHost));
    return MI355LZ4_OK;
}

// the staging windows of a call on the engine's current stream: one scratch per stream the engine has been used on, four at the
// most, the one used longest ago taken over once its stream is done with it (the rule of the segment scratch, encode_device)
static int hcdict_stage(mi355lz4_ctx *c, size_t bytes, uint8_t **out)
{
    bool takeOver;
    mi355lz4_ctx::SegScratch *slot = scratch_slot(c, c->hcStage, c->nHcStage, &takeOver);
    if (takeOver) HIP_TRY(hipStreamSynchronize(slot->s));
    slot->s = c->stream;
    slot->tick = ++c->segTick;
    if (bytes > slot->b.cap) HIP_TRY(hipStreamSynchronize(slot->s));   // (dev_reserve frees what queued work may still use)
    if (int r = dev_reserve(slot->b, bytes)) return r;
    *out = (uint8_t *)slot->b.p;
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_compress_hcdict_device(mi355lz4_ctx *c, const mi355lz4_hcdict *hd, const uint8_t *src,
                                               const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride,
                                               int maxBlockLen, int nBlocks, int headerKind, uint8_t *slots,
                                               size_t slotStride, int32_t *framedLen)
{
    if (int r = same_device(c, hd, "compress_hcdict_device", "dictionary")) return r;
    if (c->compLevel < 1)
        return fail(MI355LZ4_E_ARG, "compress_hcdict_device: compression level %d; level 0 against a dictionary is mi355lz4_compress_dict_device",
                    c->compLevel);
    if (int r = dict_batch_shape_check("compress_hcdict_device", "a dictionary batch", nBlocks, headerKind, maxBlockLen)) return r;
    if (nBlocks == 0) return MI355LZ4_OK;
    if (int r = batch_buffers_check(c, "compress_hcdict_device", src, maxBlockLen, headerKind, slots, slotStride, framedLen)) return r;
    HIP_TRY(hipSetDevice(c->device));
    HcDictArgs x;
    x.e = make_encode_args(src, srcOff, srcLen, blockStride, maxBlockLen, nBlocks, 1, headerKind, slots, slotStride, framedLen);
    x.image = hd->image;
    x.stageStride = 65536 + (((size_t)maxBlockLen + 255) & ~(size_t)255) + 256;
    if (int r = hcdict_stage(c, (size_t)encode_hc_dict_grid(nBlocks) * x.stageStride, &x.stage)) return r;
    launch_encode_hc_dict(x, c->compLevel, c->stream);
    return encode_launched(c, x.e, "hc dict launch");
}

// Level 0 against the same object: the wave encoder, block i as the second block of the linked call [kept bytes,
// block i].  k_encode_fastdict reloads the table image per block and stages the block behind its own copy of the dictionary; the
// windows come from the pool above (a call's windows are its stream's).  Enqueues only.  MI355LZ4_FASTDICT_WAVES is read per call.
extern "C" int mi355lz4_compress_fastdict_device(mi355lz4_ctx *c, const mi355lz4_hcdict *hd, const uint8_t *src,
                                                 const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride,
                                                 int maxBlockLen, int nBlocks, int accel, int headerKind, uint8_t *slots,
                                                 size_t slotStride, int32_t *framedLen)
{
    if (int r = same_device(c, hd, "compress_fastdict_device", "dictionary")) return r;
    if (c->compLevel != 0)
        return fail(MI355LZ4_E_ARG, "compress_fastdict_device: compression level %d; levels 1..12 against a dictionary are mi355lz4_compress_hcdict_device",
                    c->compLevel);
    if (int r = dict_batch_shape_check("compress_fastdict_device", "a dictionary batch", nBlocks, headerKind, maxBlockLen)) return r;
    if (nBlocks == 0) return MI355LZ4_OK;
    if (int r = batch_buffers_check(c, "compress_fastdict_device", src, maxBlockLen, headerKind, slots, slotStride, framedLen)) return r;
    HIP_TRY(hipSetDevice(c->device));
    FastDictArgs x;
    x.e = make_encode_args(src, srcOff, srcLen, blockStride, maxBlockLen, nBlocks, accel, headerKind, slots, slotStride, framedLen);
    x.e.stats = c->stats;
    x.image = hd->image;
    x.fast = hd->fastImage;
    x.stageStride = fastdict_window_stride(maxBlockLen);
    const int grid = encode_fastdict_grid(nBlocks, env_int("MI355LZ4_FASTDICT_WAVES", 0), x.stageStride);
    if (int r = hcdict_stage(c, (size_t)grid * x.stageStride, &x.stage)) return r;
    launch_encode_fastdict(x, grid, c->stream);
    return encode_launched(c, x.e, "fast dict launch");
}

// Fast pages against the same object: mi355lz4_compress_pages_fast_device's chains, every page made by the wave
// encoder with the dictionary in front of it and an output budget (k_pages_fastdict: compress_fastdict_device's grid and windows,
// sized for a block of 65536 bytes, which is the most a page holds).  Enqueues only; srcLen and pageSize stay unread on the host.
extern "C" int mi355lz4_compress_pages_fastdict_device(mi355lz4_ctx *c, const mi355lz4_hcdict *hd, const uint8_t *src,
                                                       const uint64_t *srcOff, const int32_t *srcLen, int nInputs,
                                                       const int32_t *pageSize, int maxPages, int accel, int headerKind,
                                                       uint8_t *pages, size_t pageStride, int32_t *pageSrcLen, int32_t *pageCompLen,
                                                       int32_t *nPages, int32_t *consumed)
{
    if (int r = same_device(c, hd, "compress_pages_fastdict_device", "dictionary")) return r;
    PagesFastDictArgs x;
    x.p = pages_args(src, srcOff, srcLen, nInputs, pageSize, maxPages, headerKind, pages, pageStride, pageSrcLen, pageCompLen, nPages, consumed);
    if (int r = pages_check(c, "compress_pages_fastdict_device", "dictionary", x.p)) return r;
    if (nInputs == 0) return MI355LZ4_OK;
    HIP_TRY(hipSetDevice(c->device));
    x.accel = accel_clamped(accel);
    x.image = hd->image;
    x.fast = hd->fastImage;
    x.stageStride = fastdict_window_stride(65536);                      // (the most a page holds)
    const int grid = encode_fastdict_grid(nInputs, env_int("MI355LZ4_FASTDICT_WAVES", 0), x.stageStride);
    if (int r = hcdict_stage(c, (size_t)grid * x.stageStride, &x.stage)) return r;
    launch_pages_fastdict(x, grid, c->stream);
    return check_launch("fast dict pages launch");
}

// ---------------------------------------------------------------------------
// Dictionary sets: a batch in which every block names its dictionary.  A mi355lz4_dictset is a table on the device
// of the members' image pointers; the members are borrowed (mi355lz4_hcdict_load rebuilds their images in place, so the set follows
// a reload without being recreated).  Level 0's wave encoder and the dictionary decoder take it; both only enqueue.
// ---------------------------------------------------------------------------
extern "C" int mi355lz4_dictset_create(mi355lz4_ctx *c, const mi355lz4_hcdict *const *hd, int n, mi355lz4_dictset **out)
{
    if (out) *out = nullptr;
    if (!c || !hd || !out) return fail(MI355LZ4_E_ARG, "dictset_create: null argument");
    if (n < 1 || n > DICTSET_MAX) return fail(MI355LZ4_E_ARG, "dictset_create: %d members outside 1..%d", n, DICTSET_MAX);
    for (int i = 0; i < n; i++) {
        if (!hd[i]) return fail(MI355LZ4_E_ARG, "dictset_create: member %d is null", i);
        if (hd[i]->device != c->device)
            return fail(MI355LZ4_E_ARG, "dictset_create: member %d lives on device %d, the engine on %d", i, hd[i]->device, c->device);
    }
    HIP_TRY(hipSetDevice(c->device));
    mi355lz4_dictset *ds = new (std::nothrow) mi355lz4_dictset();
    if (!ds) return fail(MI355LZ4_E_ARG, "out of host memory");
    ds->device = c->device;
    ds->n = n;
    std::vector<DictSetEntry> host((size_t)n + 1);                    // (the last entry's bytes: the two diagnostic words, zero)
    for (int i = 0; i < n; i++) host[(size_t)i] = DictSetEntry{hd[i]->image, hd[i]->fastImage};
    host[(size_t)n] = DictSetEntry{nullptr, nullptr};
    const size_t bytes = ((size_t)n + 1) * sizeof(DictSetEntry);
    hipError_t e = hipMalloc((void **)&ds->table, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(ds->table, host.data(), bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);           // (host is pageable memory, and gone at the return)
    if (e != hipSuccess) {
        if (ds->table) hipFree(ds->table);
        delete ds;
        return fail(MI355LZ4_E_HIP, "dictset_create: %zu bytes: %s", bytes, hipGetErrorString(e));
    }
    *out = ds;
    return MI355LZ4_OK;
}

extern "C" void mi355lz4_dictset_destroy(mi355lz4_dictset *ds)
{
    if (!ds) return;
    hipSetDevice(ds->device);
    hipDeviceSynchronize();                 // calls that still read the table
    if (ds->table) hipFree(ds->table);
    delete ds;
}

extern "C" int mi355lz4_dictset_count(const mi355lz4_dictset *ds) { return ds ? ds->n : fail(MI355LZ4_E_ARG, "dictset_count: null set"); }

// Diagnostic hook (not part of the public header): out = {stagings, grid} of the last mi355lz4_compress_fastdict_multi_device call
// that read the set -- how often its waves staged a dictionary (or dropped to none), and how many waves there were -- after
// everything queued on the device has run.  The tests hold the call to stagings <= grid + distinct indices - 1 with it.
extern "C" int mi355lz4_debug_dictset_last(mi355lz4_dictset *ds, int out[2])
{
    if (!ds || !out) return fail(MI355LZ4_E_ARG, "debug_dictset_last: bad arguments");
    HIP_TRY(hipSetDevice(ds->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, ds->last(), 8, hipMemcpyDeviceToHost));
    return MI355LZ4_OK;
}

// mi355lz4_compress_fastdict_device with a dictionary per block: the same checks, grid and windows; behind the windows the scratch
// holds the grouping pass's order[], bins[] and range[].  Enqueues only; nothing of dictIdx or srcLen is read on the host.
extern "C" int mi355lz4_compress_fastdict_multi_device(mi355lz4_ctx *c, const mi355lz4_dictset *ds, const int32_t *dictIdx,
                                                       const uint8_t *src, const uint64_t *srcOff, const int32_t *srcLen,
                                                       uint64_t blockStride, int maxBlockLen, int nBlocks, int accel, int headerKind,
                                                       uint8_t *slots, size_t slotStride, int32_t *framedLen)
{
    if (int r = same_device(c, ds, "compress_fastdict_multi_device")) return r;
    if (c->compLevel != 0)
        return fail(MI355LZ4_E_ARG, "compress_fastdict_multi_device: compression level %d; a dictionary set is level 0's encoder", c->compLevel);
    if (int r = dict_batch_shape_check("compress_fastdict_multi_device", "a dictionary batch", nBlocks, headerKind, maxBlockLen)) return r;
    if (nBlocks == 0) return MI355LZ4_OK;
    if (!dictIdx) return fail(MI355LZ4_E_ARG, "compress_fastdict_multi_device: null dictIdx");
    if (int r = batch_buffers_check(c, "compress_fastdict_multi_device", src, maxBlockLen, headerKind, slots, slotStride, framedLen)) return r;
    HIP_TRY(hipSetDevice(c->device));
    FastDictMultiArgs x;
    x.e = make_encode_args(src, srcOff, srcLen, blockStride, maxBlockLen, nBlocks, accel, headerKind, slots, slotStride, framedLen);
    x.e.stats = c->stats;
    x.set = ds->table;
    x.nDicts = ds->n;
    x.dictIdx = dictIdx;
    x.last = ds->last();
    x.stageStride = fastdict_window_stride(maxBlockLen);
    const int grid = encode_fastdict_grid(nBlocks, env_int("MI355LZ4_FASTDICT_WAVES", 0), x.stageStride);
    const size_t windows = (size_t)grid * x.stageStride, orderBytes = ((size_t)nBlocks * 4 + 255) & ~(size_t)255;
    if (int r = hcdict_stage(c, windows + orderBytes + ((size_t)ds->n + 2 + (size_t)grid + 1) * 4, &x.stage)) return r;
    x.order = (int32_t *)(x.stage + windows);
    x.bins = (uint32_t *)(x.stage + windows + orderBytes);
    x.range = (int32_t *)(x.bins + ds->n + 2);
    launch_dictset_group(x, grid, c->stream);
    if (int r = check_launch("dictionary set grouping launch")) return r;
    launch_encode_fastdict_multi(x, grid, c->stream);
    return encode_launched(c, x.e, "fast dict multi launch");
}

// ---------------------------------------------------------------------------
// Many fast linked streams continued across calls (mi355lz4_fstreams, mi355lz4_compress_streams_fast_device): the
// wave encoder's counterpart of mi355lz4_cstreams, and the write side of mi355lz4_dstreams -- a slot is that set's slot, the last
// good block's last 64 KiB and their count.  A block's bytes depend on the tail of the block before it, on itself and on accel, so
// all blocks of all streams of a call are compressed at once (k_encode_fstreams); the slots are read by that launch and written by
// the one behind it.  The per-call table goes through the same ring as the other two sets' (stream_table_upload); the windows and
// the plan's scratch come from the dictionary calls' pool.  Everything only enqueues.  MI355LZ4_FSTREAMS_WAVES is read per call.
// ---------------------------------------------------------------------------
extern "C" int mi355lz4_fstreams_create(mi355lz4_ctx *c, int nSlots, mi355lz4_fstreams **out)
{
    return slots_create(c, nSlots, FSTREAM_SLOT_BYTES, out, "fstreams_create");
}
extern "C" void mi355lz4_fstreams_destroy(mi355lz4_fstreams *fs) { slots_destroy(fs); }
extern "C" int mi355lz4_fstreams_count(const mi355lz4_fstreams *fs) { return slots_count(fs, "fstreams_count"); }

// The set's level: LZ4's level belongs to the stream, here to the set.  0: the wave encoder; 1..12: the hash-chain
// encoder over the same plan, windows and slots (k_encode_hc_fstreams; 10..12 search as 9).  A host-side attribute: no device,
// nothing enqueued; a call reads it when it enqueues, so a call already made keeps its level.
extern "C" int mi355lz4_fstreams_set_level(mi355lz4_fstreams *fs, int level)
{
    if (!fs) return fail(MI355LZ4_E_ARG, "fstreams_set_level: null set");
    if (level < 0 || level > 12) return fail(MI355LZ4_E_ARG, "fstreams_set_level: level %d outside 0..12", level);
    fs->level = level;
    return MI355LZ4_OK;
}
extern "C" int mi355lz4_fstreams_get_level(const mi355lz4_fstreams *fs)
{
    if (!fs) return fail(MI355LZ4_E_ARG, "fstreams_get_level: null set");
    return fs->level;
}

extern "C" int mi355lz4_fstreams_reset(mi355lz4_ctx *c, mi355lz4_fstreams *fs, const int32_t *slots, int n)
{
    if (int r = slots_reset_check(c, fs, slots, n, "fstreams_reset")) return r;
    if (!slots) {
        launch_dstreams_set(fs->state, 0, fs->nSlots, nullptr, 0, c->stream);
        return check_launch("fstreams reset launch");
    }
    for (int i = 0; i < n; i++)             // the count: a dictionary of 0 bytes needs no bytes cleared
        HIP_TRY(hipMemsetAsync(fs->state + (size_t)slots[i] * FSTREAM_SLOT_BYTES + FSTREAM_COUNT_OFF, 0, 4, c->stream));
    return MI355LZ4_OK;
}

// the write-side twin of mi355lz4_dstreams_set_dict: the slot becomes the last 64 KiB of dictDevice[0, len)
extern "C" int mi355lz4_fstreams_set_dict(mi355lz4_ctx *c, mi355lz4_fstreams *fs, int slot, const uint8_t *dictDevice, int len)
{
    if (int r = same_device(c, fs, "fstreams_set_dict")) return r;
    if (int r = slot_range_check(fs, slot, "fstreams_set_dict")) return r;
    if (len < 0 || (len > 0 && !dictDevice)) return fail(MI355LZ4_E_ARG, "fstreams_set_dict: bad dictionary");
    HIP_TRY(hipSetDevice(c->device));
    const int keep = len > FSTREAM_DICT_BYTES ? FSTREAM_DICT_BYTES : len;
    launch_dstreams_set(fs->state, slot, 1, keep ? dictDevice + (len - keep) : nullptr, (uint32_t)keep, c->stream);
    return check_launch("fstreams set_dict launch");
}

// Diagnostic hook (not part of the public header): slot `slot` as it is after everything queued on the device has run -- *count =
// its dictionary bytes, hostBytes65536 (may be null) = the slot's whole dictionary area, of which the first *count bytes are kept.
extern "C" int mi355lz4_debug_fstreams_peek(mi355lz4_fstreams *fs, int slot, uint8_t *hostBytes65536, int *count)
{
    if (!fs || slot < 0 || slot >= fs->nSlots) return fail(MI355LZ4_E_ARG, "debug_fstreams_peek: bad arguments");
    HIP_TRY(hipSetDevice(fs->device));
    HIP_TRY(hipDeviceSynchronize());
    const uint8_t *st = fs->state + (size_t)slot * FSTREAM_SLOT_BYTES;
    if (count) HIP_TRY(hipMemcpy(count, st + FSTREAM_COUNT_OFF, 4, hipMemcpyDeviceToHost));
    if (hostBytes65536) HIP_TRY(hipMemcpy(hostBytes65536, st, FSTREAM_DICT_BYTES, hipMemcpyDeviceToHost));
    return MI355LZ4_OK;
}

// Enqueue the streams' parts that fall into blocks [b0, b1) of the table (a.* describes exactly those blocks), as streams_enqueue
// does: a stream cut by b0 or b1 continues through its slot in the next launch, which runs behind this one's k_fstreams_save.
int mi355lz4_detail::fstreams_enqueue(mi355lz4_ctx *c, mi355lz4_fstreams *fs, const EncodeArgs &a, int b0, int b1,
                                      const int32_t *streamFirst, const int32_t *streamSlot, int nStreams)
{
    if (a.nBlocks <= 0) return MI355LZ4_OK;
    FStreamsArgs x;
    int rc;
    StreamTableRing::Ring *used = nullptr;
    if ((rc = stream_table_upload(c, fs->table, b0, b1, streamFirst, streamSlot, nStreams, &x.work, &x.nWork, &used))) return rc;
    if (x.nWork == 0) return MI355LZ4_OK;
    x.e = a;
    x.e.stats = c->stats;
    x.e.linked = 0; x.e.lookBack = 0;
    x.state = fs->state;
    x.stageStride = fastdict_window_stride(a.uniformLen);
    const int level = fs->level;                                // (the set's, as it is now: the chain depth is a launch argument)
    const int grid = level > 0 ? encode_hc_fstreams_grid(a.nBlocks, env_int("MI355LZ4_HSTREAMS_GROUPS", 0), x.stageStride)
                               : encode_fastdict_grid(a.nBlocks, env_int("MI355LZ4_FSTREAMS_WAVES", 0), x.stageStride);
    const size_t windows = (size_t)grid * x.stageStride;
    if ((rc = hcdict_stage(c, windows + ((size_t)x.nWork + (size_t)a.nBlocks) * 4, &x.stage))) return rc;
    x.good = (int32_t *)(x.stage + windows);
    x.blockStream = x.good + x.nWork;
    if (level > 0) launch_fstreams_hc(x, grid, level, c->stream);
    else launch_fstreams(x, grid, c->stream);
    if ((rc = check_launch("fast streams launch"))) return rc;
    if ((rc = stream_table_launched(c, used))) return rc;       // (the ring entry is busy from here on, whatever the trailers do)
    return encode_trailers(c, x.e);
}

extern "C" int mi355lz4_compress_streams_fast_device(mi355lz4_ctx *c, mi355lz4_fstreams *fs, const uint8_t *src,
                                                     const uint64_t *srcOff, const int32_t *srcLen, uint64_t blockStride,
                                                     int maxBlockLen, int nBlocks, const int32_t *streamFirst,
                                                     const int32_t *streamSlot, int nStreams, int accel, int headerKind,
                                                     uint8_t *slots, size_t slotStride, int32_t *framedLen)
{
    int r = fstreams_check(c, fs, nBlocks, streamFirst, streamSlot, nStreams, "compress_streams_fast_device");
    if (r) return r;
    // (nBlocks < 0 has gone to the stream-table check above)
    if ((r = dict_batch_shape_check("compress_streams_fast_device", "a fast stream's block", nBlocks, headerKind, maxBlockLen))) return r;
    if (nBlocks == 0) return MI355LZ4_OK;
    if ((r = batch_buffers_check(c, "compress_streams_fast_device", src, maxBlockLen, headerKind, slots, slotStride, framedLen))) return r;
    HIP_TRY(hipSetDevice(c->device));
    const EncodeArgs a = make_encode_args(src, srcOff, srcLen, blockStride, maxBlockLen, nBlocks, accel, headerKind, slots, slotStride, framedLen);
    return fstreams_enqueue(c, fs, a, 0, nBlocks, streamFirst, streamSlot, nStreams);
}

extern "C" int mi355lz4_compact_device(mi355lz4_ctx *c, const uint8_t *slots, size_t slotStride,
                                       const int32_t *framedLen, int nBlocks, uint8_t *dense, size_t denseCap,
                                       uint64_t *denseOff)
{
    if (!c || nBlocks < 0 || !denseOff) return fail(MI355LZ4_E_ARG, "compact_device: bad arguments");
    if (nBlocks > 0 && (!slots || !framedLen || !dense)) return fail(MI355LZ4_E_ARG, "compact_device: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    // The total is only known on the device: the copy kernel never writes at or past denseCap (blocks that
    // do not fit are skipped), and denseOff[nBlocks] still reports the bytes the full stream needs, so a
    // caller that sized `dense` below the worst case compares denseOff[nBlocks] with denseCap.
    launch_compact(slots, slotStride, framedLen, nBlocks, dense, denseCap, denseOff, c->stream);
    return check_launch("compact launch");
}

// The scratch of a linked decode (linkBuf, tolPool, tolMeta, ptrBuf) belongs to the engine and its second pass is
// left in flight on the stream the call was made on.  When the next linked decode comes on ANOTHER stream (the
// Python binding re-targets the engine to torch's current stream on every call), that stream first waits for the
// previous use; on the same stream the order is already there.
static void link_scratch_acquire(mi355lz4_ctx *c)
{
    if (c->linkBusy && c->linkEvent && c->linkStream != c->stream) (void)hipStreamWaitEvent(c->stream, c->linkEvent, 0);
}
static void link_scratch_release(mi355lz4_ctx *c)
{
    if (!c->linkEvent && hipEventCreateWithFlags(&c->linkEvent, hipEventDisableTiming) != hipSuccess) { c->linkEvent = nullptr; return; }
    if (hipEventRecord(c->linkEvent, c->stream) == hipSuccess) { c->linkStream = c->stream; c->linkBusy = true; }
}

// The data half of a linked decode (see LinkedPlan): everything that reads output bytes.
static int linked_finish(mi355lz4_ctx *c)
{
    if (!c->plan.active) return MI355LZ4_OK;
    c->plan.active = false;
    DecodeArgs a = c->plan.a;
    const int first = c->plan.first, last = c->plan.last, pool = c->plan.pool, seg = c->plan.seg;
    if (c->plan.split) {
        launch_linked_resolve_b(a, c->stream);
    } else {
        for (int p0 = first; p0 <= last; p0 += pool) {
            const int p1 = (last + 1 - p0 < pool) ? last + 1 : p0 + pool;
            a.segFirst = p0; a.segEnd = p1;
            launch_linked_tolerant(a, c->stream);
            for (int b = p0; b < p1; b += seg) {
                a.segFirst = b;
                a.segEnd = (p1 - b < seg) ? p1 : b + seg;
                launch_linked_resolve(a, c->stream);
            }
        }
    }
    link_scratch_release(c);
    return check_launch("decode launch");
}

// The steps of a linked decode return STEP_NEXT or what the call returns; ending, they order the link scratch behind what they queued.
// pinStat words: 0-7 the summary, 8-9 the share sample, 10-11 big-pass flags, 12-13 run.ctl; _linked_end_last: 8-11 its own (below).
constexpr int STEP_NEXT = 1;
static int link_done(mi355lz4_ctx *c) { link_scratch_release(c); return check_launch("decode launch"); }
static int link_fail(mi355lz4_ctx *c, int rc) { link_scratch_release(c); return rc; }
#define LINK_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return link_fail(c, fail(MI355LZ4_E_HIP, "%s: %s", #x, hipGetErrorString(e_))); } while (0)
static int link_summary(mi355lz4_ctx *c, const LinkStat &st, int nBlocks)
{
    if (st.count == 0) return link_done(c);
    const int first = (int)st.first, last = (int)st.last;
    if (first < 0 || last >= nBlocks || first > last)
        return link_fail(c, fail(MI355LZ4_E_HIP, "decompress: bad failure range %d..%d", first, last));
    return STEP_NEXT;
}
// The big-block path's scratch: a 64 KiB snapshot per block (ptrBuf) and, in tolMeta, 64 KiB of zeros, the flags and the results;
// pass 1: the first launch makes the path's first pass.  Scratch that cannot be had is no error: the call takes the other paths.
static bool big_scratch(mi355lz4_ctx *c, DecodeArgs &a, int pass)
{
    const size_t metaBytes = 65536 + ((size_t)a.nBlocks * 2 + 4) * sizeof(uint32_t);
    const bool ok = dev_reserve(c->ptrBuf, (size_t)a.nBlocks * 65536u) == 0 && dev_reserve(c->tolMeta, metaBytes) == 0 &&
                    hipMemsetAsync(c->tolMeta.p, 0, metaBytes, c->stream) == hipSuccess;
    (void)hipGetLastError();
    if (!ok) return false;
    uint8_t *meta = (uint8_t *)c->tolMeta.p;
    a.run.zeroPage = meta;
    a.cu = {(uint8_t *)c->ptrBuf.p, (uint32_t *)(meta + 65536), (int32_t *)(meta + 65536 + ((size_t)a.nBlocks + 4) * sizeof(uint32_t)), pass};   // snap, flags, res, pass
    return true;
}
// Big blocks (big_arm): every dependent block by the workgroup form against a GUESS of its dictionary -- zeros, then its predecessor's
// last 64 KiB a pass ago -- until a pass changes none (k_decode_cu_linked).  A block of 1 MiB forgets a wrong dictionary long before its
// end: two passes do as a rule, the first maybe made by the first launch (pre).  Anything the form cannot take (a failing block,
// CU_REDO, snapshots that do not settle in BIG_PASSES) leaves the call to the next steps: the results so far live in scratch.
static int linked_big(mi355lz4_ctx *c, DecodeArgs &a, const DecodeKnobs &k, const LinkStat &st, BigArm arm, bool pre)
{
    bool late = false;
    if (arm != BigArm::No && !pre) {           // (also when the scratch could not be had before the first launch)
        late = big_takes(k, st) && big_scratch(c, a, 0);
        (void)hipGetLastError();
    }
    if (!pre && !late) return STEP_NEXT;
    if (big_takes(k, st)) {
        uint32_t *flags = (uint32_t *)c->pinStat.p + 10;
        bool settled = false; int passes = 0;
        for (int pass = 1; pass <= BIG_PASSES && !settled; pass++) {
            a.cu.pass = pass; passes = pass;
            launch_cu_linked(a, pass > 1 || late, c->stream);
            if (hipGetLastError() != hipSuccess) break;
            if (pass == 1) continue;                                  // (every snapshot is new after the first pass)
            LINK_TRY(hipMemcpyAsync(flags, a.cu.flags, 8, hipMemcpyDeviceToHost, c->stream));
            LINK_TRY(hipStreamSynchronize(c->stream));
            if (flags[1] != 0) break;                                 // a block this form cannot take
            settled = flags[0] == 0;
        }
        if (settled) {
            launch_cu_publish(a, c->stream);
            c->linkedPath = (int)LinkedPath::Big; c->runinShareE6 = passes;   // (diagnostics: Big reports its passes where the others report the sampled share)
            return link_done(c);
        }
        (void)hipGetLastError();
    }
    a.cu = {}; a.run.zeroPage = nullptr;
    return STEP_NEXT;
}
// Short runs (runs_take): every run walked by a wave of its own with the exact decoder and its dictionary, from a list of their starts
static int linked_runs(mi355lz4_ctx *c, DecodeArgs &a, const DecodeCall &d, const EngineMode &m, const DecodeKnobs &k, const LinkStat &st)
{
    if (!runs_take(d, m, k, st)) return STEP_NEXT;
    const int runs = (int)st.runs > 0 ? (int)st.runs : 1;
    if (int r = dev_reserve(c->tolMeta, ((size_t)runs + 1) * sizeof(int32_t))) return link_fail(c, r);
    a.runs.list = (int32_t *)c->tolMeta.p; a.runs.cap = runs;
    if (hipMemsetAsync(a.runs.list, 0, sizeof(int32_t), c->stream) != hipSuccess)
        return link_fail(c, fail(MI355LZ4_E_HIP, "decompress: the run list could not be cleared"));
    a.segFirst = (int)st.first; a.segEnd = (int)st.last + 1;
    launch_linked_runs(a, c->stream);
    c->linkedPath = (int)LinkedPath::Runs;
    return link_done(c);
}
// Long runs of dependent blocks (a reference-written stream is ONE) in pieces, every piece decoded from a few blocks in front of it
// ("run-in": by then the dictionary is the true one; checked against what the piece in front wrote, redone where not:
// kernels/runin.inc, "RUN-IN DECODE").  Serial chain: run-in + piece blocks (0.53 ms per 64 KiB of text); one wave and a ring of two blocks per piece.
// Not finished (a broken block, rounds that run out, no scratch): finished segments are final, st is taken again for the rest.
static int linked_runin(mi355lz4_ctx *c, DecodeArgs &a, const DecodeCall &d, const EngineMode &m, const DecodeKnobs &k, LinkStat &st)
{
    const int first = (int)st.first, last = (int)st.last, span0 = last - first + 1;
    uint32_t *pin = (uint32_t *)c->pinStat.p;
    RuninPlan p = runin_plan(c->runin, d, m, k, span0, st.maxCap);
    double share = -1;
    if (p.sample) {
        const int nS = span0 < 32 ? span0 : 32, step = span0 / nS;
        a.segFirst = first;
        bool sampled = hipMemsetAsync(a.linkStat + 8, 0, 8, c->stream) == hipSuccess;
        if (sampled) launch_dict_share(a, step, nS, c->stream);
        sampled = sampled && hipMemcpyAsync(pin + 8, a.linkStat + 8, 8, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
                  hipStreamSynchronize(c->stream) == hipSuccess;
        (void)hipGetLastError();
        if (sampled && pin[9] > 0) { share = (double)pin[8] / (double)pin[9]; c->runinShareE6 = (int)(share * 1e6); }
    }
    if (p.use) runin_after_sample(p, k, span0, share);
    if (!p.use) return STEP_NEXT;
    a.run.spin = k.runinSpin;
    const size_t nPiecesMax = ((size_t)p.segBlocks + p.piece - 1) / p.piece, metaBytes = 65536 + (size_t)p.segBlocks * 4 + nPiecesMax * 20 + 64;
    bool done = false;
    if (dev_reserve(c->ptrBuf, nPiecesMax * 2u * p.stride) == 0 && dev_reserve(c->tolMeta, metaBytes) == 0) {
        uint8_t *meta = (uint8_t *)c->tolMeta.p, *tail = meta + 65536 + (size_t)p.segBlocks * 4;
        a.run.zeroPage = meta; a.run.ring = (uint8_t *)c->ptrBuf.p; a.run.stride = p.stride; a.run.piece = p.piece; a.run.in = p.runIn;
        a.run.res = (int32_t *)(meta + 65536); a.run.info = (int32_t *)tail;
        a.run.dirty = (uint32_t *)(tail + nPiecesMax * 16); a.run.ctl = (uint32_t *)(tail + nPiecesMax * 20);
        // (a kernel that did not launch must not read as "nothing left to do": run.ctl was zeroed by the host)
        uint32_t *ctl = pin + 12;
        LINK_TRY(hipMemsetAsync(meta, 0x00, 65536, c->stream));
        done = true;
        for (int s0 = first; s0 <= last && done; s0 += p.segBlocks) {
            a.segFirst = s0; a.segEnd = (s0 + p.segBlocks < last + 1) ? s0 + p.segBlocks : last + 1;
            LINK_TRY(hipMemsetAsync(a.run.ctl, 0, 8, c->stream));
            launch_runin_decode(a, c->stream);
            bool segDone = false, launched = hipGetLastError() == hipSuccess;
            for (int round = 0; round < RUNIN_ROUNDS && !segDone && launched; round++) {
                a.run.round = round;
                if (round) LINK_TRY(hipMemsetAsync(a.run.ctl, 0, 4, c->stream));
                launch_runin_fix(a, c->stream);
                if (hipGetLastError() != hipSuccess) { launched = false; break; }
                LINK_TRY(hipMemcpyAsync(ctl, a.run.ctl, 8, hipMemcpyDeviceToHost, c->stream));
                LINK_TRY(hipStreamSynchronize(c->stream));
                if (ctl[1] != 0) break;                 // a block failed with the dictionary it got, or a chain of dirty pieces
                segDone = ctl[0] == 0;
            }
            done = segDone;
            if (segDone) launch_runin_publish(a, c->stream);
            else runin_given_up(c->runin, p, k, launched ? ctl[1] : 1u);
        }
    }
    (void)hipGetLastError();                             // (only a failed reservation is left to swallow here)
    a.run = {};
    c->linkedPath = (int)(done ? (p.longRun ? LinkedPath::RunInLong : LinkedPath::RunIn) : LinkedPath::RunInGivenUp);
    if (done) return link_done(c);
    a.segFirst = 0; a.segEnd = a.nBlocks;
    LINK_TRY(hipMemsetAsync(a.linkStat, 0, 32, c->stream));
    LINK_TRY(hipMemsetAsync(a.linkStat + 1, 0xff, 4, c->stream));
    launch_link_stat(a, c->stream);
    LINK_TRY(hipMemcpyAsync(pin, a.linkStat, 32, hipMemcpyDeviceToHost, c->stream));
    LINK_TRY(hipStreamSynchronize(c->stream));
    st = LinkStat::from(pin);
    return link_summary(c, st, a.nBlocks);
}
// The lists / pointer passes (ptr_plan), or the serial walk without their scratch; the data half in linked_finish (now, or at _end)
static int linked_pointer(mi355lz4_ctx *c, DecodeArgs &a, const DecodeCall &d, const DecodeKnobs &k, const LinkStat &st)
{
    const int first = (int)st.first, last = (int)st.last, span = last - first + 1;
    if (c->linkedPath != (int)LinkedPath::RunInGivenUp) c->linkedPath = (int)LinkedPath::Pointer;
    const PtrPlan p = ptr_plan(d, k, st, span);
    int seg = p.pool;
    if (p.lists && dev_reserve(c->tolPool, (size_t)p.pool * p.per * tol_region_bytes()) == 0 &&
        dev_reserve(c->tolMeta, ((size_t)a.nBlocks * 3 + 4) * sizeof(int32_t)) == 0) {
        a.tol.pool = c->tolPool.p; a.tol.regions = p.pool * p.per; a.tol.per = p.per;
        a.tol.counter = (uint32_t *)c->tolMeta.p; a.tol.region = (int32_t *)c->tolMeta.p + 4;
        a.tol.count = a.tol.region + a.nBlocks; a.tol.size = a.tol.count + a.nBlocks;
        if (p.usePtr && dev_reserve(c->ptrBuf, p.ptrs * sizeof(uint32_t)) == 0) {
            a.ptr.buf = (uint32_t *)c->ptrBuf.p; a.ptr.cap = p.ptrs;
            a.ptr.ctl = (uint8_t *)c->linkBuf.p + 64;
            a.ptr.bad = (uint32_t *)((uint8_t *)c->linkBuf.p + 64 + ptr_ctl_bytes());
            seg = p.seg;
        }
    }
    (void)hipGetLastError();          // scratch that could not be had is not an error: the serial walk needs none
    c->plan.active = true;
    c->plan.a = a; c->plan.first = first; c->plan.last = last; c->plan.pool = p.pool; c->plan.seg = seg;
    c->plan.split = linked_split(d.splitOk, a.ptr.buf != nullptr, span, seg, p.pool);
    if (c->plan.split) {
        a.segFirst = first; a.segEnd = last + 1;
        launch_linked_tolerant(a, c->stream);
        launch_linked_resolve_a(a, c->stream);
        c->plan.a = a;
    }
    return d.deferEnd ? check_launch("decode launch") : linked_finish(c);
}

static int decode_device_impl(mi355lz4_ctx *c, const DecodeCall &d, const int32_t *ckFail)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (c->plan.active) return fail(MI355LZ4_E_ARG, "a linked decode begun with mi355lz4_decompress_linked_begin is still open");
    if (d.nBlocks < 0 || (d.headerKind != 4 && d.headerKind != 8) || d.fixedUncomp < 0)
        return fail(MI355LZ4_E_ARG, "decompress_batch_device: bad arguments");
    if (d.nBlocks == 0) return MI355LZ4_OK;
    if (!d.framed || !d.blockOff || !d.outOff || !d.result) return fail(MI355LZ4_E_ARG, "decompress_batch_device: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    const DecodeKnobs k = read_decode_knobs();
    const EngineMode m{c->decoder, c->stats != nullptr, k.asyncSet ? k.asyncCap : c->linkedAsyncCap};
    DecodeArgs a{};
    a.framed = d.framed; a.framedLen = d.framedLen; a.blockOff = d.blockOff; a.nBlocks = d.nBlocks; a.segEnd = d.nBlocks;
    a.headerKind = d.headerKind; a.fixedUncomp = d.fixedUncomp; a.linked = d.linked ? 1 : 0;
    a.out = d.out; a.outOff = d.outOff; a.outCap = d.outCap; a.result = d.result; a.dict0 = d.dict0; a.dict0Len = d.dict0Len;
    a.streamFirst = d.streamFirst; a.nStreams = d.nStreams; a.lookBack = d.lookBack;
    a.onlyBlk = -1; a.cuDbg = c->cuDbg; a.cuBail = c->decoder == 0; a.ckFail = ckFail;
    int r;
    if (d.linked) {
        link_scratch_acquire(c);
        const size_t nFlags = d.streamFirst ? (size_t)(d.nStreams > 0 ? d.nStreams : 1) : 1;
        if ((r = dev_reserve(c->linkBuf, 64 + ptr_ctl_bytes() + 4 * nFlags)) || (r = pin_reserve(c->pinStat, 64))) return r;
        a.linkStat = (uint32_t *)c->linkBuf.p;
        HIP_TRY(hipMemsetAsync(a.linkStat, 0, 32, c->stream));
        HIP_TRY(hipMemsetAsync(a.linkStat + 1, 0xff, 4, c->stream));
    }
    if (d.target) {                                  // partial decode: no dictionary, so nothing follows the one pass
        a.target = d.target;
        const FirstPass fp = first_pass(d, m, k);
        launch_decode_partial(a, fp == FirstPass::Seq ? 1 : (fp == FirstPass::Cu ? 4 : 2), c->stream);
        return check_launch("decode launch");
    }
    const BigArm big = big_arm(d, m, k);
    const bool bigPre = big == BigArm::BeforeFirstPass && big_scratch(c, a, 1);
    switch (first_pass(d, m, k)) {
    case FirstPass::Seq: launch_decode_seq(a, c->stream); break;
    case FirstPass::Cu: launch_decode_cu(a, c->stream); break;
#ifdef MI355LZ4_EXPERIMENTS
    case FirstPass::Tok:   // experiment: the parse as a pass of its own (token lists), then the list-driven decoder
        if (dev_reserve(c->tokBuf, (size_t)(d.framedLen >> 1) + 192 + ((size_t)d.nBlocks + 1) * sizeof(int32_t)) == 0) {
            a.tok.cnt = (int32_t *)c->tokBuf.p;
            a.tok.list = (uint8_t *)c->tokBuf.p + ((((size_t)d.nBlocks + 1) * sizeof(int32_t) + 63) & ~(size_t)63);
            launch_decode_tok(a, c->stream);
            break;
        }
        [[fallthrough]];
#endif
    default: launch_decode_par(a, c->stats, c->stream);
    }
    if (!d.linked) return check_launch("decode launch");
    // Linked: the call waits for the standalone pass (independent blocks pay this wait and nothing else).  Asynchronous form: no wait;
    // the second pass is enqueued over ALL blocks, its kernels return at once when the first pass counted no dependent block.
    LinkStat st;
    if (async_gate(d, m)) { a.asyncGate = 1; st = LinkStat::whole_call(d.nBlocks, m.asyncCap); } else {
        launch_longest_stream(a, c->stream);
        HIP_TRY(hipMemcpyAsync(c->pinStat.p, a.linkStat, 32, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        st = LinkStat::from((const uint32_t *)c->pinStat.p);
    }
    c->runinShareE6 = -1; c->linkedPath = (int)LinkedPath::None;
    if ((r = link_summary(c, st, d.nBlocks)) != STEP_NEXT) return r;
    if ((r = linked_big(c, a, k, st, big, bigPre)) != STEP_NEXT) return r;
    if ((r = linked_runs(c, a, d, m, k, st)) != STEP_NEXT) return r;
    if ((r = linked_runin(c, a, d, m, k, st)) != STEP_NEXT) return r;
    return linked_pointer(c, a, d, k, st);
}
#undef LINK_TRY

// Every decode of the engine.  With block checksums on, the blocks' data is hashed first (k_xxh32_verify, one flag per
// block in ckBuf) and read_block_header turns a mismatch into MI355LZ4_BLK_E_CHECKSUM: to every decode path a block
// that fails its checksum is a header-rejected block, so linked streams treat it as they treat any other.
int mi355lz4_detail::decode_device(mi355lz4_ctx *c, const DecodeCall &d)
{
    if (!c || !c->blockChecksum || d.nBlocks <= 0 || c->plan.active || !d.framed || !d.blockOff ||
        (d.headerKind != 4 && d.headerKind != 8))
        return decode_device_impl(c, d, nullptr);
    HIP_TRY(hipSetDevice(c->device));
    // the flags belong to the engine: a decode on another stream first waits for the last one that read them
    if (c->ckEvent && c->ckStream != c->stream) HIP_TRY(hipStreamWaitEvent(c->stream, c->ckEvent, 0));
    int r;
    if ((r = dev_reserve(c->ckBuf, (size_t)d.nBlocks * 4))) return r;
    DecodeArgs v = DecodeArgs();
    v.framed = d.framed; v.framedLen = d.framedLen; v.blockOff = d.blockOff; v.nBlocks = d.nBlocks; v.headerKind = d.headerKind;
    launch_xxh32_verify(v, (int32_t *)c->ckBuf.p, c->stream);
    if ((r = check_launch("checksum launch"))) return r;
    r = decode_device_impl(c, d, (const int32_t *)c->ckBuf.p);
    if (!c->ckEvent && hipEventCreateWithFlags(&c->ckEvent, hipEventDisableTiming) != hipSuccess) c->ckEvent = nullptr;
    if (c->ckEvent && hipEventRecord(c->ckEvent, c->stream) == hipSuccess) c->ckStream = c->stream;
    return r;
}

extern "C" int mi355lz4_decompress_batch_device(mi355lz4_ctx *c, const uint8_t *framed, uint64_t framedLen,
                                                const uint64_t *blockOff, int nBlocks, int headerKind,
                                                int fixedUncomp, int linked, uint8_t *out, const uint64_t *outOff,
                                                const int32_t *outCap, int32_t *result)
{
    return decode_device(c, {framed, framedLen, blockOff, nBlocks, headerKind, fixedUncomp, linked, out, outOff, outCap, result});
}

extern "C" int mi355lz4_decompress_partial_device(mi355lz4_ctx *c, const uint8_t *framed, uint64_t framedLen,
                                                  const uint64_t *blockOff, int nBlocks, int headerKind, int fixedUncomp,
                                                  uint8_t *out, const uint64_t *outOff, const int32_t *outCap,
                                                  const int32_t *target, int32_t *result)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (nBlocks < 0 || (headerKind != 4 && headerKind != 8) || fixedUncomp < 0)
        return fail(MI355LZ4_E_ARG, "decompress_partial_device: bad arguments");
    if (nBlocks > 0 && (!target || !framed || !blockOff || !outOff || !result))
        return fail(MI355LZ4_E_ARG, "decompress_partial_device: null pointer");
    DecodeCall d{framed, framedLen, blockOff, nBlocks, headerKind, fixedUncomp, 0, out, outOff, outCap, result};
    d.target = target;
    return decode_device(c, d);
}

extern "C" int mi355lz4_decompress_linked_begin(mi355lz4_ctx *c, const uint8_t *framed, uint64_t framedLen,
                                               const uint64_t *blockOff, int nBlocks, int headerKind, int fixedUncomp,
                                               uint8_t *out, const uint64_t *outOff, const int32_t *outCap,
                                               int32_t *result, int lookBack)
{
    if (lookBack < 0 || lookBack > 1) return fail(MI355LZ4_E_ARG, "decompress_linked_begin: lookBack must be 0 or 1");
    DecodeCall d{framed, framedLen, blockOff, nBlocks, headerKind, fixedUncomp, 1, out, outOff, outCap, result};
    d.lookBack = lookBack; d.splitOk = d.deferEnd = true;
    return decode_device(c, d);
}

extern "C" int mi355lz4_decompress_linked_end(mi355lz4_ctx *c)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    return linked_finish(c);
}

// The LAST block of a range begun with mi355lz4_decompress_linked_begin, ahead of _end: 1 = its bytes are final (the
// caller may pass them on and call _end at leisure), 0 = not available this way (call _end first).
extern "C" int mi355lz4_decompress_linked_end_last(mi355lz4_ctx *c)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->plan.active) return 1;                           // no block of the range needed its dictionary: all final
    if (!c->plan.split || !c->plan.a.ptr.ctl || c->plan.a.streamFirst) return 0;
    DecodeArgs a = c->plan.a;
    const int last = a.nBlocks - 1;
    int r;
    if ((r = pin_reserve(c->pinStat, 48))) return r;
    // {lastOpen, the stream's flag, the last block's standalone result, whether it has a list}
    uint32_t *stat = (uint32_t *)c->pinStat.p + 8;
    uint8_t *ctl = (uint8_t *)a.ptr.ctl;
    stat[0] = stat[1] = 0; stat[3] = 0;
    if (last >= a.segFirst && last < a.segEnd) {
        HIP_TRY(hipMemsetAsync(ctl + ptr_ctl_last_open_offset(), 0, sizeof(uint32_t), c->stream));
        a.onlyBlk = last;
        launch_linked_fetch_block(a, c->stream);
        HIP_TRY(hipMemcpyAsync(&stat[0], ctl + ptr_ctl_last_open_offset(), 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&stat[1], a.ptr.bad, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(&stat[3], a.tol.region + last, 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(&stat[2], a.result + last, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((r = check_launch("decode launch"))) return r;
    const int32_t res = (int32_t)stat[2];
    if (res > 0) return 1;                                   // decoded on its own: final since the first pass
    // a dependent block: final only if the pointer pass took it and its chasing fetch left nothing open
    return (stat[0] == 0 && stat[1] == 0 && (int32_t)stat[3] >= 0) ? 1 : 0;
}

extern "C" int mi355lz4_decompress_streams_device(mi355lz4_ctx *c, const uint8_t *framed, uint64_t framedLen,
                                                  const uint64_t *blockOff, int nBlocks, int headerKind,
                                                  int fixedUncomp, const int32_t *streamFirst, int nStreams,
                                                  uint8_t *out, const uint64_t *outOff, const int32_t *outCap,
                                                  int32_t *result)
{
    if (nStreams < 0 || (nStreams > 0 && !streamFirst))
        return fail(MI355LZ4_E_ARG, "decompress_streams_device: bad stream table");
    DecodeCall d{framed, framedLen, blockOff, nBlocks, headerKind, fixedUncomp, nStreams > 0, out, outOff, outCap, result};
    if (nStreams > 0) { d.streamFirst = streamFirst; d.nStreams = nStreams; }   // (no streams: every block is decoded on its own)
    return decode_device(c, d);
}

// ---------------------------------------------------------------------------
// Many linked decode streams continued across calls (mi355lz4_dstreams, mi355lz4_decompress_dstreams_device):
// the decode side's counterpart of mi355lz4_cstreams.  A slot is LZ4_streamDecode_t for separately allocated blocks, on the
// device -- the last block's last 64 KiB and their count (kernels.h, DSTREAM_*) -- and k_decode_dstreams decodes every block
// once, with its dictionary, so there is no first pass whose verdict the host would wait for: the call only enqueues.  The
// per-call table goes through the same ring as the compress side's (stream_table_upload).
// ---------------------------------------------------------------------------
extern "C" int mi355lz4_dstreams_create(mi355lz4_ctx *c, int nSlots, mi355lz4_dstreams **out)
{
    return slots_create(c, nSlots, DSTREAM_SLOT_BYTES, out, "dstreams_create");
}
extern "C" void mi355lz4_dstreams_destroy(mi355lz4_dstreams *ds) { slots_destroy(ds); }
extern "C" int mi355lz4_dstreams_count(const mi355lz4_dstreams *ds) { return slots_count(ds, "dstreams_count"); }

extern "C" int mi355lz4_dstreams_reset(mi355lz4_ctx *c, mi355lz4_dstreams *ds, const int32_t *slots, int n)
{
    if (int r = slots_reset_check(c, ds, slots, n, "dstreams_reset")) return r;
    if (!slots) {
        launch_dstreams_set(ds->state, 0, ds->nSlots, nullptr, 0, c->stream);
        return check_launch("dstreams reset launch");
    }
    for (int i = 0; i < n; i++)             // the count: a dictionary of 0 bytes needs no bytes cleared
        HIP_TRY(hipMemsetAsync(ds->state + (size_t)slots[i] * DSTREAM_SLOT_BYTES + DSTREAM_COUNT_OFF, 0, 4, c->stream));
    return MI355LZ4_OK;
}

// LZ4_setStreamDecode (cbits/lz4.c:2292-2300) for one slot: only the last 64 KiB of a dictionary can be referenced
extern "C" int mi355lz4_dstreams_set_dict(mi355lz4_ctx *c, mi355lz4_dstreams *ds, int slot, const uint8_t *dictDevice, int len)
{
    if (int r = same_device(c, ds, "dstreams_set_dict")) return r;
    if (int r = slot_range_check(ds, slot, "dstreams_set_dict")) return r;
    if (len < 0 || (len > 0 && !dictDevice)) return fail(MI355LZ4_E_ARG, "dstreams_set_dict: bad dictionary");
    HIP_TRY(hipSetDevice(c->device));
    const int keep = len > DSTREAM_DICT_BYTES ? DSTREAM_DICT_BYTES : len;
    launch_dstreams_set(ds->state, slot, 1, keep ? dictDevice + (len - keep) : nullptr, (uint32_t)keep, c->stream);
    return check_launch("dstreams set_dict launch");
}

// Diagnostic hook (not part of the public header): slot `slot` as it is after everything queued on the device has run --
// *count = its dictionary bytes, bytes (may be null, 65536 bytes of host memory) = the slot's whole dictionary area.  A
// non-null setBytes (65536 bytes) then overwrites that area, the count stays (the tests put guard patterns into unused slots).
extern "C" int mi355lz4_debug_dstream_state(mi355lz4_dstreams *ds, int slot, uint32_t *count, uint8_t *bytes, const uint8_t *setBytes)
{
    if (!ds || slot < 0 || slot >= ds->nSlots) return fail(MI355LZ4_E_ARG, "debug_dstream_state: bad arguments");
    HIP_TRY(hipSetDevice(ds->device));
    HIP_TRY(hipDeviceSynchronize());
    uint8_t *st = ds->state + (size_t)slot * DSTREAM_SLOT_BYTES;
    if (count) HIP_TRY(hipMemcpy(count, st + DSTREAM_COUNT_OFF, 4, hipMemcpyDeviceToHost));
    if (bytes) HIP_TRY(hipMemcpy(bytes, st, DSTREAM_DICT_BYTES, hipMemcpyDeviceToHost));
    if (setBytes) HIP_TRY(hipMemcpy(st, setBytes, DSTREAM_DICT_BYTES, hipMemcpyHostToDevice));
    return MI355LZ4_OK;
}

int mi355lz4_detail::dstreams_check(const mi355lz4_ctx *c, const mi355lz4_dstreams *ds, int nBlocks, const int32_t *streamFirst,
                                    const int32_t *streamSlot, int nStreams, const char *who)
{
    if (int r = same_device(c, ds, who)) return r;
    if (c->plan.active) return fail(MI355LZ4_E_ARG, "%s: a linked decode begun with mi355lz4_decompress_linked_begin is still open", who);
    return stream_table_check(ds->nSlots, nBlocks, streamFirst, streamSlot, nStreams, who);
}

// Block checksums for the calls that decode every block once (dstreams, dictionary batches), as decode_device has them: ck_flags
// enqueues k_xxh32_verify over a's blocks into the engine's ckBuf and arms a.ckFail (nothing when checksums are off); ck_done,
// behind the launches that read the flags, marks where the next decode on another stream has to wait.
static int ck_flags(mi355lz4_ctx *c, DecodeArgs &a)
{
    if (!c->blockChecksum) return MI355LZ4_OK;
    int rc;
    if (c->ckEvent && c->ckStream != c->stream) HIP_TRY(hipStreamWaitEvent(c->stream, c->ckEvent, 0));
    if ((rc = dev_reserve(c->ckBuf, (size_t)a.nBlocks * 4))) return rc;
    launch_xxh32_verify(a, (int32_t *)c->ckBuf.p, c->stream);
    if ((rc = check_launch("checksum launch"))) return rc;
    a.ckFail = (const int32_t *)c->ckBuf.p;
    return MI355LZ4_OK;
}
static void ck_done(mi355lz4_ctx *c)
{
    if (!c->blockChecksum) return;
    if (!c->ckEvent && hipEventCreateWithFlags(&c->ckEvent, hipEventDisableTiming) != hipSuccess) c->ckEvent = nullptr;
    if (c->ckEvent && hipEventRecord(c->ckEvent, c->stream) == hipSuccess) c->ckStream = c->stream;
}

// Enqueue the streams' parts that fall into blocks [b0, b1) of the table (d.* describes exactly those blocks, as a.* does in
// streams_enqueue): the checksum flags first, as in decode_device, then one wave per stream with blocks.
int mi355lz4_detail::dstreams_enqueue(mi355lz4_ctx *c, mi355lz4_dstreams *ds, const DecodeCall &d, int b0, int b1,
                                      const int32_t *streamFirst, const int32_t *streamSlot, int nStreams)
{
    if (d.nBlocks <= 0) return MI355LZ4_OK;
    DStreamsArgs x{};
    x.d.framed = d.framed; x.d.framedLen = d.framedLen; x.d.blockOff = d.blockOff; x.d.nBlocks = d.nBlocks; x.d.segEnd = d.nBlocks;
    x.d.headerKind = d.headerKind; x.d.fixedUncomp = d.fixedUncomp; x.d.linked = 1;
    x.d.out = d.out; x.d.outOff = d.outOff; x.d.outCap = d.outCap; x.d.result = d.result; x.d.onlyBlk = -1;
    int rc;
    if ((rc = ck_flags(c, x.d))) return rc;
    int nWork = 0;
    StreamTableRing::Ring *used = nullptr;
    if ((rc = stream_table_upload(c, ds->table, b0, b1, streamFirst, streamSlot, nStreams, &x.work, &nWork, &used))) return rc;
    if (nWork > 0) {
        x.state = ds->state;
        launch_decode_dstreams(x, nWork, c->stream);
        if ((rc = check_launch("decode streams launch"))) return rc;
        if ((rc = stream_table_launched(c, used))) return rc;
    }
    ck_done(c);
    return MI355LZ4_OK;
}

extern "C" int mi355lz4_decompress_dstreams_device(mi355lz4_ctx *c, mi355lz4_dstreams *ds, const uint8_t *framed,
                                                   uint64_t framedLen, const uint64_t *blockOff, int nBlocks, int headerKind,
                                                   int fixedUncomp, const int32_t *streamFirst, const int32_t *streamSlot,
                                                   int nStreams, uint8_t *out, const uint64_t *outOff, const int32_t *outCap,
                                                   int32_t *result)
{
    int r = dstreams_check(c, ds, nBlocks, streamFirst, streamSlot, nStreams, "decompress_dstreams_device");
    if (r) return r;
    if ((headerKind != 4 && headerKind != 8) || fixedUncomp < 0) return fail(MI355LZ4_E_ARG, "decompress_dstreams_device: bad arguments");
    if (nBlocks == 0) return MI355LZ4_OK;
    if (!framed || !blockOff || !outOff || !result) return fail(MI355LZ4_E_ARG, "decompress_dstreams_device: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    const DecodeCall d{framed, framedLen, blockOff, nBlocks, headerKind, fixedUncomp, 1, out, outOff, outCap, result};
    return dstreams_enqueue(c, ds, d, 0, nBlocks, streamFirst, streamSlot, nStreams);
}

// Independent blocks against one external dictionary: LZ4_decompress_safe_usingDict's external-dictionary path
// for every block, k_decode_dict.  Every block is decoded once, with the dictionary, so the call only enqueues; the checksum
// flags go first (ck_flags).  The decoder-variant knob has no say: the workgroup form has no dictionary.
extern "C" int mi355lz4_decompress_dict_device(mi355lz4_ctx *c, const uint8_t *framed, uint64_t framedLen,
                                               const uint64_t *blockOff, int nBlocks, int headerKind, int fixedUncomp,
                                               const uint8_t *dictDevice, int dictLen, uint8_t *out, const uint64_t *outOff,
                                               const int32_t *outCap, int32_t *result)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (c->plan.active) return fail(MI355LZ4_E_ARG, "decompress_dict_device: a linked decode begun with mi355lz4_decompress_linked_begin is still open");
    if (nBlocks < 0 || (headerKind != 4 && headerKind != 8) || fixedUncomp < 0)
        return fail(MI355LZ4_E_ARG, "decompress_dict_device: bad arguments");
    if (dictLen < 0 || (dictLen > 0 && !dictDevice)) return fail(MI355LZ4_E_ARG, "decompress_dict_device: bad dictionary");
    if (nBlocks == 0) return MI355LZ4_OK;
    if (!framed || !blockOff || !outOff || !result) return fail(MI355LZ4_E_ARG, "decompress_dict_device: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    DecodeArgs a{};
    a.framed = framed; a.framedLen = framedLen; a.blockOff = blockOff; a.nBlocks = nBlocks; a.segEnd = nBlocks;
    a.headerKind = headerKind; a.fixedUncomp = fixedUncomp;
    a.out = out; a.outOff = outOff; a.outCap = outCap; a.result = result; a.onlyBlk = -1;
    a.dict0 = dictDevice; a.dict0Len = (uint32_t)dictLen;
    if (int rc = ck_flags(c, a)) return rc;
    launch_decode_dict(a, c->stream);
    const int rc = check_launch("decode dict launch");
    ck_done(c);
    return rc;
}

// ... and every block against the member of a dictionary set that it names: the call above with (ds, dictIdx) in
// place of (dict, dictLen), k_decode_dict_multi.  Enqueues only; nothing of dictIdx is read on the host.
extern "C" int mi355lz4_decompress_dict_multi_device(mi355lz4_ctx *c, const uint8_t *framed, uint64_t framedLen,
                                                     const uint64_t *blockOff, int nBlocks, int headerKind, int fixedUncomp,
                                                     const mi355lz4_dictset *ds, const int32_t *dictIdx, uint8_t *out,
                                                     const uint64_t *outOff, const int32_t *outCap, int32_t *result)
{
    if (int r = same_device(c, ds, "decompress_dict_multi_device")) return r;
    if (c->plan.active)
        return fail(MI355LZ4_E_ARG, "decompress_dict_multi_device: a linked decode begun with mi355lz4_decompress_linked_begin is still open");
    if (nBlocks < 0 || (headerKind != 4 && headerKind != 8) || fixedUncomp < 0)
        return fail(MI355LZ4_E_ARG, "decompress_dict_multi_device: bad arguments");
    if (nBlocks == 0) return MI355LZ4_OK;
    if (!framed || !blockOff || !outOff || !result || !dictIdx) return fail(MI355LZ4_E_ARG, "decompress_dict_multi_device: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    DictMultiArgs x{};
    DecodeArgs &a = x.d;
    a.framed = framed; a.framedLen = framedLen; a.blockOff = blockOff; a.nBlocks = nBlocks; a.segEnd = nBlocks;
    a.headerKind = headerKind; a.fixedUncomp = fixedUncomp;
    a.out = out; a.outOff = outOff; a.outCap = outCap; a.result = result; a.onlyBlk = -1;
    x.set = ds->table; x.nDicts = ds->n; x.dictIdx = dictIdx;
    if (int rc = ck_flags(c, a)) return rc;
    launch_decode_dict_multi(x, c->stream);
    const int rc = check_launch("decode dict multi launch");
    ck_done(c);
    return rc;
}

extern "C" int mi355lz4_xxh32_device(mi355lz4_ctx *c, const uint8_t *base, const uint64_t *off, const int32_t *len, int n,
                                     uint32_t seed, uint32_t *out)
{
    if (!c) return fail(MI355LZ4_E_ARG, "null ctx");
    if (n < 0) return fail(MI355LZ4_E_ARG, "xxh32_device: bad arguments");
    if (n == 0) return MI355LZ4_OK;
    if (!base || !off || !len || !out) return fail(MI355LZ4_E_ARG, "xxh32_device: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    launch_xxh32_ranges(base, off, len, n, seed, out, c->stream);
    return check_launch("checksum launch");
}

extern "C" int mi355lz4_index_device(mi355lz4_ctx *c, const uint8_t *framed, uint64_t framedLen,
                                     const uint64_t *blockOff, int nBlocks, int headerKind, int fixedUncomp,
                                     uint64_t *outOff)
{
    if (!c || nBlocks < 0 || !outOff || (headerKind != 4 && headerKind != 8))
        return fail(MI355LZ4_E_ARG, "index_device: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    int r = dev_reserve(c->scratch, (size_t)(nBlocks + 1) * sizeof(int32_t));
    if (r) return r;
    launch_index(framed, framedLen, blockOff, nBlocks, headerKind, fixedUncomp, (int32_t *)c->scratch.p, outOff,
                 c->stream);
    return check_launch("index launch");
}

extern "C" int mi355lz4_decoded_size_device(mi355lz4_ctx *c, const uint8_t *framed, uint64_t framedLen,
                                            const uint64_t *blockOff, int nBlocks, int headerKind, int maxUncomp,
                                            int32_t *size, uint64_t *outOff)
{
    if (!c || nBlocks < 0 || maxUncomp < 0 || (headerKind != 4 && headerKind != 8) ||
        (nBlocks > 0 && (!framed || !blockOff || !size)))
        return fail(MI355LZ4_E_ARG, "decoded_size_device: bad arguments");
    HIP_TRY(hipSetDevice(c->device));
    launch_decoded_size(framed, framedLen, blockOff, nBlocks, headerKind, maxUncomp, c->blockChecksum, size, outOff, c->stream);
    return check_launch("size launch");
}

extern "C" int mi355lz4_generate_device(mi355lz4_ctx *c, int kind, uint8_t *dst, int blockLen, int nBlocks,
                                        uint64_t firstBlock, uint64_t blockStep, uint32_t litMax, uint32_t offMax)
{
    if (!c || kind < 0 || kind > 2 || blockLen < 0 || nBlocks < 0 || (nBlocks > 0 && blockLen > 0 && !dst))
        return fail(MI355LZ4_E_ARG, "generate_device: bad arguments");
    if (kind == 1 && (litMax == 0 || offMax == 0)) return fail(MI355LZ4_E_ARG, "generate_device: litMax/offMax must be > 0");
    if (nBlocks == 0 || blockLen == 0) return MI355LZ4_OK;
    HIP_TRY(hipSetDevice(c->device));
    launch_generate(kind, dst, blockLen, nBlocks, firstBlock, blockStep, litMax, offMax, c->stream);
    return check_launch("generate launch");
}

extern "C" int mi355lz4_interleave_device(mi355lz4_ctx *c, const uint8_t *local, const uint64_t *localOff,
                                          int nLocalBlocks, int rank, int nRanks, uint8_t *global,
                                          const uint64_t *globalOff)
{
    if (!c || nLocalBlocks < 0 || nRanks <= 0 || rank < 0 || rank >= nRanks)
        return fail(MI355LZ4_E_ARG, "interleave_device: bad arguments");
    if (nLocalBlocks == 0) return MI355LZ4_OK;
    if (!local || !localOff || !global || !globalOff) return fail(MI355LZ4_E_ARG, "interleave_device: null pointer");
    HIP_TRY(hipSetDevice(c->device));
    launch_interleave(local, localOff, nLocalBlocks, rank, nRanks, global, globalOff, c->stream);
    return check_launch("interleave launch");
}

// ---------------------------------------------------------------------------
// events (bench.py times kernels on the engine's own stream)
// ---------------------------------------------------------------------------
extern "C" int mi355lz4_event_create(void **ev)
{
    if (!ev) return fail(MI355LZ4_E_ARG, "null");
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    *ev = (void *)e;
    return MI355LZ4_OK;
}
extern "C" int mi355lz4_event_destroy(void *ev)
{
    if (ev) HIP_TRY(hipEventDestroy((hipEvent_t)ev));
    return MI355LZ4_OK;
}
extern "C" int mi355lz4_event_record(mi355lz4_ctx *c, void *ev)
{
    if (!c || !ev) return fail(MI355LZ4_E_ARG, "null");
    HIP_TRY(hipEventRecord((hipEvent_t)ev, c->stream));
    return MI355LZ4_OK;
}
extern "C" int mi355lz4_event_elapsed_ms(void *start, void *stop, float *ms)
{
    if (!start || !stop || !ms) return fail(MI355LZ4_E_ARG, "null");
    HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return MI355LZ4_OK;
}

