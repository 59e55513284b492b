/*
 * lzf_api.cpp -- the device side of liblzf_hip.so's C-ABI.
 *
 * The kernel routing (which generation compresses a batch, which decoder
 * decodes it), the per-device compress scratch and the LDS lane-order
 * self-check, and the device-pointer calls of include/lzf_gpu.h.  The
 * host-memory calls -- the drop-in pair of include/lzf.h (src/lzf.h:76-78,
 * 95-97) and the lzf_host_* batches -- are in lzf_host.cpp and launch
 * through lzf_route_compress / lzf_route_decompress below.  There is no CPU
 * codec in this library: every call runs the HIP kernels.  Failures never
 * abort (a server must survive a transient HIP error): the batch calls
 * return a negative LZF_GPU_E* code (LZF_GPU_ENODEV without a device).
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "lzf_internal.h"
#include "lzf_request.h"
#include "lzf_order.h"
#include "../../include/lzf.h"
#include "../../include/lzf_gpu.h"

#ifdef LZF_DIAG
hipError_t lzf_launch_compress_serial(const LzfBatch &b, hipStream_t s);
hipError_t lzf_launch_decompress_serial(const LzfBatch &b, hipStream_t s);
#endif

int lzf_lds_order_check(int dev);   /* lzf_selfcheck.hip */

namespace {

enum KernelGen { GEN_TABLE = 0, GEN_LANE = 1, GEN_WINDOW = 2, GEN_SERIAL = 3, GEN_WTAB = 4, GEN_TABLE_ONLY = 5 };

/* values of at most this many bytes take the lane generation by default
 * (stream cand + lane parse), larger ones the table generation: json4k
 * 1 M x 4 KiB 45.9 vs 48.7 ms (small class), text8k 1 M x 8 KiB 88.8 vs
 * 111.0 ms (table), mixed16k 256 K x 16 KiB 65.1 vs 71.4 ms (table), but
 * text64k 128 K x 64 KiB 127.4 vs 121.6 ms (the table's two-link records
 * save the parse more hops than its cand costs) */
constexpr uint32_t LANE_DEFAULT_MAX = 16384u;

/* LZF_GPU_KERNEL picks the kernel generation, read per launch so one process
 * can A/B them.  Unset: the measured routing of launch_compress (the lane
 * generation -- the stream cand kernel, lzf_stream.hip, and the lane parse,
 * lzf_lane.hip -- up to 16 KiB; the table generation, lzf_cand.hip, for values
 * of 16-64 KiB; window64 past 64 KiB and for small batches).
 * "lane": the lane generation wherever it applies; "table": the table
 * generation at any size it takes; "window": one wave per value (window64 /
 * tokpar64).  Diagnostic build only: "serial" (the single-lane first
 * generation) and "wtab" (the window-parse generation, lzf_wparse.hip, a
 * measured prototype that is not routed).  All are bit-exact; the GPU tests
 * cross-check them. */
KernelGen kernel_gen()
{
    const char *e = getenv("LZF_GPU_KERNEL");
#ifdef LZF_DIAG
    if (e && !strcmp(e, "serial")) return GEN_SERIAL;
    if (e && !strcmp(e, "wtab")) return GEN_WTAB;
#endif
    if (e && !strcmp(e, "window")) return GEN_WINDOW;
    if (e && !strcmp(e, "lane")) return GEN_LANE;
    if (e && !strcmp(e, "table")) return GEN_TABLE_ONLY;
    return GEN_TABLE;
}

bool device_ok(int dev)
{
    static std::mutex mu;
    static int checked[64];      /* 0 unknown, 1 ok, -1 bad */
    if (dev < 0 || dev >= 64) return false;
    std::lock_guard<std::mutex> lk(mu);
    if (!checked[dev]) {
        hipDeviceProp_t prop;
        checked[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess &&
                        strstr(prop.gcnArchName, "gfx950") != nullptr) ? 1 : -1;
    }
    return checked[dev] == 1;
}

/* The table, lane and window generations need the LDS to run a wave's
 * same-address ds_mskor_rtn_b32 in lane order (lzf_selfcheck.hip).  Checked
 * per device before their first launch (on the probe's own stream, so the
 * caller's stream and the rest of the device are not synchronised); where it
 * does not hold, compress batches go to window64.  Only a definite answer is
 * kept: a probe that could not run (an allocation or launch failure under
 * load) routes this batch to window64 and is tried again on the next one.
 * LZF_GPU_FORCE_ORDER_FAIL=1 makes the check report a violation (tests of
 * the fallback).  A caller that captures compress launches in a HIP graph
 * runs lzf_gpu_selfcheck() first, outside the capture. */
int g_order[64];                     /* 0 unchecked, 1 held, -1 violated */
int g_order_last[64];                /* the last probe's outcome, -2: it could not run */
/* a probe that could not run is retried no sooner than this (a backoff
 * doubling from 100 ms to 10 s, so a lasting failure -- memory pressure, a
 * caller capturing a graph -- does not cost every compress call a probe
 * under the mutex) */
std::chrono::steady_clock::time_point g_order_retry[64];
std::chrono::milliseconds g_order_backoff[64];
std::mutex g_order_mu;

int lds_order_state(bool run)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -2;
    std::lock_guard<std::mutex> lk(g_order_mu);
    const auto now = std::chrono::steady_clock::now();
    if (!g_order[dev] && run && (g_order_last[dev] != -2 || now >= g_order_retry[dev])) {
        const char *f = getenv("LZF_GPU_FORCE_ORDER_FAIL");
        const int bad = (f && *f == '1') ? 1 : lzf_lds_order_check(dev);
        g_order_last[dev] = bad == 0 ? 1 : bad > 0 ? -1 : -2;
        if (bad >= 0) {
            g_order[dev] = g_order_last[dev];
        } else {
            auto &b = g_order_backoff[dev];
            b = b.count() ? std::min(b * 2, std::chrono::milliseconds(10000)) : std::chrono::milliseconds(100);
            g_order_retry[dev] = now + b;
        }
        return g_order_last[dev];
    }
    return g_order[dev] ? g_order[dev] : g_order_last[dev];
}

bool lds_order_ok() { return lds_order_state(true) == 1; }

int current_device_ok()
{
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) return LZF_GPU_ENODEV;
    return device_ok(dev) ? LZF_GPU_OK : LZF_GPU_ENODEV;
}

/* Compress scratch (records/cand words + inserted bitmap), ONE per device,
 * shared by every host thread under a mutex and grown on demand (cap:
 * scratch_limit).  The mutex is held while a batch is enqueued; a batch on
 * another stream than the previous user first waits for that user's
 * kernels (an event), so concurrent callers stay correct.  lzf_gpu_release()
 * frees it. */
struct Scratch {
    std::mutex mu;
    void *p = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;
    bool used = false;
    /* this scratch's share of the cap: 1 for the device's, NSLOT for each
     * chunk slot of the registered host pipeline, whose launches run side by
     * side and keep their buffers between calls -- together they stay within
     * one cap instead of taking half of what each one finds free */
    unsigned share = 1;
#ifdef LZF_DIAG
    hipStream_t aux = nullptr;      /* kernel-2 stream of the chunk pipeline */
    hipEvent_t pev[4] = {nullptr, nullptr, nullptr, nullptr};
#endif
};

Scratch g_scratch[64];

/* Scratch cap: LZF_GPU_SCRATCH_MB if set, else half of the device memory
 * free when the scratch grows (at least 1 GiB): a whole BASELINE batch
 * (256 K x 64 KiB: 67 GiB of records) then runs as one chunk, and a caller
 * that holds most of the device still gets chunked, not refused. */
size_t scratch_limit(size_t held, unsigned share = 1)
{
    if (share < 1) share = 1;
    const char *e = getenv("LZF_GPU_SCRATCH_MB");
    if (e) {
        unsigned long long mb = strtoull(e, nullptr, 10);
        if (mb < 1) mb = 1;
        return ((size_t)mb << 20) / share;
    }
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) return ((size_t)40 << 30) / share;
    /* held: this scratch's own buffer, which a regrow gives back first; the
     * slot scratches' shares are of the device's total, so buffers the other
     * slots already hold do not shrink the next one's share */
    size_t lim = share == 1 ? (fr + held) / 2 : tot / (2 * (size_t)share);
    if (share > 1 && lim > fr + held) lim = fr + held;
    return lim > ((size_t)1 << 30) ? lim : ((size_t)1 << 30);
}

void scratch_free(Scratch &S)
{
    if (S.p) {
        if (S.used && S.ev) (void)hipEventSynchronize(S.ev);
        (void)hipFree(S.p);
    }
    S.p = nullptr;
    S.cap = 0;
    S.used = false;
}

enum ScratchUser { SU_LANE = 0, SU_TABLE = 1, SU_WTAB = 2 };
/* chunks of this thread's last scratch-bound compress launch (kernel_info) */
thread_local uint32_t g_last_chunks = 0;
/* the route of this thread's last launch_compress (lzf_gpu_mixed_last_plan) */
enum Route { ROUTE_NONE = 0, ROUTE_LANE = 1, ROUTE_TABLE = 2, ROUTE_WINDOW = 3, ROUTE_DIAG = 4 };
thread_local int g_last_route = ROUTE_NONE;

hipError_t window_compress(const LzfBatch &b, hipStream_t s)
{
    g_last_route = ROUTE_WINDOW;
    return lzf_launch_compress(b, s);
}

/* own: a caller's private scratch (the host pipelines' slots, so their
 * chunks' compress launches can run side by side), else the device's */
hipError_t lane_compress(const LzfBatch &b, hipStream_t s, ScratchUser who, Scratch *own = nullptr,
                         const LzfParts *parts = nullptr)
{
    const bool table = who == SU_TABLE;
    g_last_route = table ? ROUTE_TABLE : who == SU_LANE ? ROUTE_LANE : ROUTE_DIAG;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    Scratch &S = own ? *own : g_scratch[dev & 63];
    std::lock_guard<std::mutex> lk(S.mu);
#ifdef LZF_DIAG
    const size_t per = who == SU_WTAB ? lzf_wtab_scratch_per_value(b.max_len)
                       : table        ? lzf_table_scratch_per_value(b.max_len)
                                      : lzf_lane_scratch_per_value(b.max_len);
#else
    const size_t per = table ? lzf_table_scratch_per_value(b.max_len) : lzf_lane_scratch_per_value(b.max_len);
#endif
    size_t want = per * (size_t)b.count + 512;
    const size_t lim = scratch_limit(S.cap, S.share);
    if (want > lim) want = lim;
    if (want < 2 * per + 1024) want = 2 * per + 1024;     /* two pipeline halves */
    /* an explicit cap binds even when an earlier batch grew the scratch past
     * it: the buffer is given back and re-made at the cap */
    const bool capped = getenv("LZF_GPU_SCRATCH_MB") != nullptr;
    if (capped && S.cap > want && S.cap > lim) scratch_free(S);
    if (S.cap < want) {
        scratch_free(S);
        /* short of device memory: a smaller scratch only means more chunks */
        const size_t least = 2 * per + 1024;
        while ((e = hipMalloc(&S.p, want)) != hipSuccess && want > least) {
            (void)hipGetLastError();
            want = want / 2 > least ? want / 2 : least;
        }
        if (e != hipSuccess) {
            S.p = nullptr;
            return e;
        }
        S.cap = want;
    }
    if (!S.ev && (e = hipEventCreateWithFlags(&S.ev, hipEventDisableTiming)) != hipSuccess) return e;
    if (S.used && S.last != s && (e = hipStreamWaitEvent(s, S.ev, 0)) != hipSuccess) return e;
    /* the chunk size comes from the usable scratch: the buffer, or the cap
     * when one is set below it */
    const size_t use = capped && lim < S.cap ? (lim > 2 * per + 1024 ? lim : 2 * per + 1024) : S.cap;
    if (table) {
        e = lzf_launch_compress_table(b, s, S.p, use, &g_last_chunks, parts);
    }
#ifdef LZF_DIAG
    else if (who == SU_WTAB) {
        e = lzf_launch_compress_wtab(b, s, S.p, use, &g_last_chunks);
    }
#endif
    else {
        /* the lane generation takes the batch whole: every part in first */
        for (uint32_t p = 0; parts && p < parts->n; p++)
            if ((e = hipStreamWaitEvent(s, parts->ev[p], 0)) != hipSuccess) return e;
#ifdef LZF_DIAG
        const char *ff = getenv("LZF_GPU_LANE_FORCE_FIX");
        /* LZF_GPU_LANE_PIPE=1 overlaps the two kernels of consecutive chunks
         * on two streams (both kernels hold LDS and do not co-reside well) */
        const char *pp = getenv("LZF_GPU_LANE_PIPE");
        const bool pipe = pp && *pp == '1';
        if (pipe && !S.aux) {
            if ((e = hipStreamCreateWithFlags(&S.aux, hipStreamNonBlocking)) != hipSuccess) return e;
            for (int k = 0; k < 4; k++)
                if ((e = hipEventCreateWithFlags(&S.pev[k], hipEventDisableTiming)) != hipSuccess) return e;
        }
        e = lzf_launch_compress_lane(b, s, S.p, use, (ff && *ff == '1') ? 1u : 0u, pipe ? S.aux : nullptr,
                                     pipe ? S.pev : nullptr, &g_last_chunks);
#else
        e = lzf_launch_compress_lane(b, s, S.p, use, 0u, nullptr, nullptr, &g_last_chunks);
#endif
    }
    if (e != hipSuccess) return e;
    e = hipEventRecord(S.ev, s);
    S.last = s;
    S.used = true;
    return e;
}

/* smallest batch the lane / table generations take (LZF_GPU_LANE_MIN
 * overrides): below it window64's one wave per value finishes first, since
 * the parse's time has a floor of one whole value's parse per lane.
 * tools/crossover.py, round 4, the routed generations (stream cand + lane
 * parse up to 16 KiB, table above) vs window64, compress ms
 * (profiles/r04/xo_*.txt): json 4 KiB 7.02 vs 6.61 at 96 K values, 7.71 vs
 * 8.78 at 128 K; text 8 KiB 11.21 vs 11.31 at 32 K; mixed 16 KiB 24.80 vs
 * 20.07 at 32 K, 26.37 vs 29.86 at 48 K; text 64 KiB 77.22 vs 69.47 at 24 K,
 * 80.45 vs 92.62 at 32 K. */
uint32_t lane_min_count(uint32_t max_len)
{
    const char *e = getenv("LZF_GPU_LANE_MIN");
    if (e) return (uint32_t)strtoul(e, nullptr, 10);
    if (max_len <= 4096u) return 114688u;
    if (max_len <= 8192u) return 32768u;
    if (max_len <= 16384u) return 45056u;
    return 28672u;
}

/* bulk: the caller runs several launches side by side (the host-memory
 * pipeline), so the per-launch floor of the parse overlaps and the batch
 * threshold below which window64 wins alone does not apply */
hipError_t launch_compress(const LzfBatch &b, hipStream_t s, Scratch *own = nullptr, bool bulk = false,
                           const LzfParts *parts = nullptr)
{
    const KernelGen g = kernel_gen();
    /* inputs in parts: a route that takes the batch whole waits for all */
    const bool routed_default = g == GEN_TABLE && lds_order_ok() && lzf_table_compress_supported(b.max_len);
    if (parts && !routed_default)
        for (uint32_t p = 0; p < parts->n; p++) {
            const hipError_t e = hipStreamWaitEvent(s, parts->ev[p], 0);
            if (e != hipSuccess) return e;
        }
    if (!routed_default) parts = nullptr;
    if (g != GEN_WINDOW && g != GEN_SERIAL && !lds_order_ok()) return window_compress(b, s);
    switch (g) {
#ifdef LZF_DIAG
    case GEN_SERIAL: g_last_route = ROUTE_DIAG; return lzf_launch_compress_serial(b, s);
#endif
    case GEN_WINDOW: return window_compress(b, s);
    case GEN_LANE:
        return (lzf_lane_compress_supported(b.max_len) && b.count >= lane_min_count(b.max_len))
                   ? lane_compress(b, s, SU_LANE)
                   : window_compress(b, s);
#ifdef LZF_DIAG
    case GEN_WTAB:
        return lzf_wtab_compress_supported(b.max_len) ? lane_compress(b, s, SU_WTAB) : window_compress(b, s);
#endif
    case GEN_TABLE_ONLY:
        return (lzf_table_compress_supported(b.max_len) && b.count >= lane_min_count(b.max_len))
                   ? lane_compress(b, s, SU_TABLE)
                   : window_compress(b, s);
    default:
        /* batches with values past 64 KiB, and small batches, go to the window
         * generation: the parse runs one value per lane, so its time has a
         * floor of one whole value's parse (~5 ms); below the crossover one
         * wave per value finishes first (tools/crossover.py).  Values of at
         * most LANE_DEFAULT_MAX bytes take the lane generation (the stream
         * cand kernel, lzf_stream.hip, and the lane parse), larger ones the
         * table generation (two-link records, lzf_cand.hip) */
        if ((!bulk && b.count < lane_min_count(b.max_len)) || !lzf_table_compress_supported(b.max_len)) {
            for (uint32_t p = 0; parts && p < parts->n; p++) {
                const hipError_t e = hipStreamWaitEvent(s, parts->ev[p], 0);
                if (e != hipSuccess) return e;
            }
            return window_compress(b, s);
        }
        /* the lane generation where its kernel 1 takes the batch (a
         * diagnostic LZF_GPU_CAND=small stops at 4 KiB), else the table one --
         * unless the scratch cap splits the table generation into more chunks
         * than the lane generation (half the scratch per value): every chunk
         * pays the parse's per-launch floor, so the chunk count decides
         * (configs[2] under a 16 GiB cap: table 5 chunks 441 ms, lane 3 chunks
         * 335 ms; 8 GiB: 712 / 488; uncapped table 190 vs lane 214,
         * profiles/r05/cap/) */
        {
            bool lane = b.max_len <= LANE_DEFAULT_MAX && lzf_lane_compress_supported(b.max_len);
            if (!lane && lzf_lane_compress_supported(b.max_len)) {
                int dev = 0;
                if (hipGetDevice(&dev) == hipSuccess) {
                    Scratch &S = own ? *own : g_scratch[dev & 63];
                    size_t held;
                    unsigned share;
                    {
                        /* another thread's lane_compress may be regrowing it */
                        std::lock_guard<std::mutex> lk(S.mu);
                        held = S.cap;
                        share = S.share;
                    }
                    const size_t lim = scratch_limit(held, share);
                    const uint64_t need_t = (uint64_t)b.count * lzf_table_scratch_per_value(b.max_len);
                    const uint64_t need_l = (uint64_t)b.count * lzf_lane_scratch_per_value(b.max_len);
                    lane = (need_t + lim - 1) / lim > (need_l + lim - 1) / lim;
                }
            }
            return lane_compress(b, s, lane ? SU_LANE : SU_TABLE, own, parts);
        }
    }
}

/* The lane decoder (one lane per stream, diagnostic build) is bit-exact but,
 * streaming 64 values per wave through L2, slower than pipe / tokpar64 on
 * the BASELINE shapes; it runs only when
 * LZF_GPU_DECOMPRESS=lane asks for it. */
bool lane_decoder()
{
#ifdef LZF_DIAG
    const char *e = getenv("LZF_GPU_DECOMPRESS");
    return e && !strcmp(e, "lane");
#else
    return false;                    /* the lane decoder is in the diagnostic build only */
#endif
}

hipError_t launch_decompress(const LzfBatch &b, hipStream_t s)
{
    switch (kernel_gen()) {
#ifdef LZF_DIAG
    case GEN_SERIAL: return lzf_launch_decompress_serial(b, s);
    default: return lane_decoder() ? lzf_launch_decompress_lane(b, s) : lzf_launch_decompress(b, s);
#else
    default: return lzf_launch_decompress(b, s);
#endif
    }
}

/* the compress step of the device SET path (lzf_launch_store): the uniform
 * routed launch over the whole batch; per-class routing would go in here */
hipError_t store_compress(const LzfBatch &b, hipStream_t s) { return launch_compress(b, s); }

int code_of(hipError_t e)
{
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return LZF_GPU_ENOMEM;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return LZF_GPU_ENODEV;
    return LZF_GPU_ELAUNCH;
}

/* what an entry point returns for its launcher's result */
int rc_of(hipError_t e) { return e == hipSuccess ? LZF_GPU_OK : code_of(e); }

/* the store's item arrays as the one view the launchers take (LzfItems).  Its
 * members are not const; a call site whose operator only reads an array casts
 * there and says so */
LzfItems items_of(uint8_t *enc, uint32_t count, int64_t *item_time, int32_t *item_ttl, int64_t *item_lock,
                  int64_t *last_access, int64_t now)
{
    return LzfItems{enc, count, item_time, item_ttl, item_lock, last_access, now};
}

/* ---- mixed-size batches: one class batch per size class -------------------- */

constexpr uint32_t MIXED_NC = LZF_GPU_NCLASS + 1;

/* whether launch_compress sends this batch to window64 -- its conditions,
 * read-only.  It only chooses the stream of a class batch (window64 holds no
 * scratch, so it may run beside the others); were it ever wrong, the scratch's
 * own event still orders its users across streams. */
bool compress_goes_window(const LzfBatch &b)
{
    const KernelGen g = kernel_gen();
    if (g == GEN_SERIAL) return false;
    if (g == GEN_WINDOW || !lds_order_ok()) return true;
    switch (g) {
    case GEN_LANE: return !(lzf_lane_compress_supported(b.max_len) && b.count >= lane_min_count(b.max_len));
#ifdef LZF_DIAG
    case GEN_WTAB: return !lzf_wtab_compress_supported(b.max_len);
#endif
    case GEN_TABLE_ONLY: return !(lzf_table_compress_supported(b.max_len) && b.count >= lane_min_count(b.max_len));
    default: return b.count < lane_min_count(b.max_len) || !lzf_table_compress_supported(b.max_len);
    }
}

/* the decoder lzf_launch_decompress picks for a bound (lzf_decompress.hip:
 * tokpar64 up to 4 KiB, tokpar64-far up to CD_FAR_MAX = 16 KiB, the pipe past) */
int decompress_route(uint32_t max_len)
{
#ifdef LZF_DIAG
    if (kernel_gen() == GEN_SERIAL || lane_decoder()) return ROUTE_DIAG;
#endif
    return max_len <= 4096u ? 1 : max_len <= 16384u ? 2 : 3;
}

/* per device: the side stream of the window64 classes with its fork / join
 * events, and the pinned landing place of the 48-byte plan.  The mutex is
 * held while a mixed call enqueues (its one wait included), so concurrent
 * mixed calls on one device take turns. */
struct Side {
    std::mutex mu;
    hipStream_t st = nullptr;
    hipEvent_t fork = nullptr, join = nullptr, got = nullptr;
    uint32_t *pin = nullptr;
};
Side g_side[64];

void side_free(Side &S)
{
    if (S.st) {
        (void)hipStreamSynchronize(S.st);
        (void)hipStreamDestroy(S.st);
    }
    if (S.fork) (void)hipEventDestroy(S.fork);
    if (S.join) (void)hipEventDestroy(S.join);
    if (S.got) (void)hipEventDestroy(S.got);
    if (S.pin) (void)hipHostFree(S.pin);
    S.st = nullptr;
    S.fork = S.join = S.got = nullptr;
    S.pin = nullptr;
}

/* this thread's last mixed device call (lzf_gpu_mixed_last_plan) */
thread_local uint32_t g_plan_count[MIXED_NC], g_plan_max[MIXED_NC];
thread_local int g_plan_route[MIXED_NC];
thread_local uint32_t g_last_mixed = 0;

size_t mixed_work_bytes(uint32_t count)
{
    /* perm, four descriptor copies, out_len and err copies; the plan; the
     * partition's tables; room to align the caller's pointer */
    return (size_t)count * (2u * sizeof(uint64_t) + 5u * sizeof(uint32_t)) + 64u + lzf_partition_work_bytes(count) +
           16u;
}

int mixed_call(int kind, const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len, uint8_t *out,
               const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, int32_t *err, uint32_t count,
               uint32_t bound, void *work, hipStream_t s)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return LZF_GPU_ENODEV;
    uint8_t *w = (uint8_t *)(((uintptr_t)work + 15u) & ~(uintptr_t)15u);
    uint64_t *c_in_off = (uint64_t *)w;
    uint64_t *c_out_off = c_in_off + count;
    uint32_t *perm = (uint32_t *)(c_out_off + count);
    uint32_t *c_in_len = perm + count, *c_out_cap = c_in_len + count, *c_out_len = c_out_cap + count;
    int32_t *c_err = (int32_t *)(c_out_len + count);
    uint32_t *plan = (uint32_t *)(c_err + count);           /* class_count, class_max */
    void *pwork = plan + 16;
    const bool comp = kind == LZF_GPU_KIND_COMPRESS;

    Side &S = g_side[dev];
    std::lock_guard<std::mutex> lk(S.mu);
    hipError_t e;
    if (!S.pin && (e = hipHostMalloc((void **)&S.pin, 2u * MIXED_NC * sizeof(uint32_t), hipHostMallocDefault)) !=
                      hipSuccess) {
        S.pin = nullptr;
        return code_of(e);
    }
    if (!S.got && (e = hipEventCreateWithFlags(&S.got, hipEventDisableTiming)) != hipSuccess) return code_of(e);

    /* partition by the length that picks the plan, compact the descriptors,
     * and fetch the plan: the call's one wait */
    if ((e = lzf_launch_size_partition(comp ? in_len : out_cap, count, bound, kind, perm, plan, plan + MIXED_NC,
                                       pwork, s)) != hipSuccess ||
        (e = lzf_launch_mixed_gather(perm, count, in_off, in_len, out_off, out_cap, c_in_off, c_in_len, c_out_off,
                                     c_out_cap, s)) != hipSuccess ||
        (e = hipMemcpyAsync(S.pin, plan, 2u * MIXED_NC * sizeof(uint32_t), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipEventRecord(S.got, s)) != hipSuccess || (e = hipEventSynchronize(S.got)) != hipSuccess)
        return code_of(e);
    uint32_t start[MIXED_NC], at = 0;
    for (uint32_t c = 0; c < MIXED_NC; c++) {
        g_plan_count[c] = S.pin[c];
        g_plan_max[c] = S.pin[MIXED_NC + c];
        g_plan_route[c] = ROUTE_NONE;
        start[c] = at;
        at += g_plan_count[c];
    }
    if (at != count) return LZF_GPU_ELAUNCH;               /* the partition did not account for every value */

    /* the class batches, largest class first; the window64 ones (compress)
     * aside, unless nothing else would run on the caller's stream */
    LzfBatch cb[LZF_GPU_NCLASS];
    int cls_of[LZF_GPU_NCLASS], main_i[LZF_GPU_NCLASS], side_i[LZF_GPU_NCLASS];
    uint32_t nb = 0, nmain = 0, nside = 0;
    for (int c = LZF_GPU_NCLASS - 1; c >= 0; c--) {
        if (!g_plan_count[c]) continue;
        const uint32_t o = start[c];
        cb[nb] = LzfBatch{in,           c_in_off + o,  c_in_len + o,
                          out,          c_out_off + o, c_out_cap + o,
                          c_out_len + o, err ? c_err + o : nullptr,
                          g_plan_count[c], g_plan_max[c] ? g_plan_max[c] : 1u};
        cls_of[nb] = c;
        if (comp && g_plan_max[c] && compress_goes_window(cb[nb]))
            side_i[nside++] = (int)nb;
        else
            main_i[nmain++] = (int)nb;
        nb++;
    }
    if (!nmain && nside) {
        main_i[nmain++] = side_i[0];
        for (uint32_t k = 1; k < nside; k++) side_i[k - 1] = side_i[k];
        nside--;
    }
    g_last_mixed = nb;

    auto run = [&](int k, hipStream_t st) -> hipError_t {
        const LzfBatch &b = cb[k];
        const int c = cls_of[k];
        if (!comp) {
            g_plan_route[c] = decompress_route(b.max_len);
            return launch_decompress(b, st);
        }
        if (!g_plan_max[c])              /* a class of empty values: out_len 0 each, as max_in_len 0 does */
            return hipMemsetAsync(b.out_len, 0, (size_t)b.count * sizeof(uint32_t), st);
        const hipError_t r = launch_compress(b, st);
        g_plan_route[c] = g_last_route;
        return r;
    };

    hipError_t first = hipSuccess;
    bool forked = false;
    if (nside) {
        if (!S.st) e = hipStreamCreateWithFlags(&S.st, hipStreamNonBlocking);
        else e = hipSuccess;
        if (e == hipSuccess && !S.fork) e = hipEventCreateWithFlags(&S.fork, hipEventDisableTiming);
        if (e == hipSuccess && !S.join) e = hipEventCreateWithFlags(&S.join, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(S.fork, s);
        if (e == hipSuccess) e = hipStreamWaitEvent(S.st, S.fork, 0);
        if (e != hipSuccess) return code_of(e);
        forked = true;
        for (uint32_t k = 0; k < nside && first == hipSuccess; k++) first = run(side_i[k], S.st);
    }
    for (uint32_t k = 0; k < nmain && first == hipSuccess; k++) first = run(main_i[k], s);
    if (forked) {                        /* joined even after a failure: the side work must not outlive the call's order */
        e = hipEventRecord(S.join, S.st);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, S.join, 0);
        if (first == hipSuccess) first = e;
    }
    if (first != hipSuccess) return code_of(first);
    e = lzf_launch_mixed_scatter(perm, count, plan, c_out_len, err ? c_err : nullptr, out_len, err, s);
    return e == hipSuccess ? LZF_GPU_OK : code_of(e);
}

}  // namespace

/* the routed launches and the scratch, for the host-memory paths (lzf_host.cpp) */
hipError_t lzf_route_compress(const LzfBatch &b, hipStream_t s) { return launch_compress(b, s); }
hipError_t lzf_route_decompress(const LzfBatch &b, hipStream_t s) { return launch_decompress(b, s); }
uint32_t lzf_route_min_count(uint32_t max_len) { return lane_min_count(max_len); }
bool lzf_device_ok(int dev) { return device_ok(dev); }
hipError_t lzf_route_compress_window(const LzfBatch &b, hipStream_t s) { return lzf_launch_compress(b, s); }
bool lzf_route_default(void) { return kernel_gen() == GEN_TABLE && lds_order_ok(); }
hipError_t lzf_route_compress_bulk(const LzfBatch &b, hipStream_t s, void *scratch, const LzfParts *parts)
{
    return launch_compress(b, s, (Scratch *)scratch, true, parts);
}
void *lzf_scratch_create(unsigned share)
{
    Scratch *S = new Scratch();
    S->share = share ? share : 1u;
    return S;
}
void lzf_scratch_destroy(void *scratch)
{
    Scratch *S = (Scratch *)scratch;
    if (!S) return;
    {
        std::lock_guard<std::mutex> lk(S->mu);
        scratch_free(*S);
        if (S->ev) (void)hipEventDestroy(S->ev);
    }
    delete S;
}
void lzf_scratch_release(void *scratch)
{
    Scratch *S = (Scratch *)scratch;
    if (!S) return;
    std::lock_guard<std::mutex> lk(S->mu);
    scratch_free(*S);
}
void lzf_scratch_release_all(void)
{
    for (Scratch &S : g_scratch) {
        std::lock_guard<std::mutex> lk(S.mu);
        scratch_free(S);
    }
    /* the mixed calls' side stream, events and pinned plan */
    for (Side &S : g_side) {
        std::lock_guard<std::mutex> lk(S.mu);
        side_free(S);
    }
}

extern "C" {

uint64_t lzf_gpu_mixed_work_size(uint32_t count)
{
    return mixed_work_bytes(count);
}

int lzf_gpu_compress_mixed(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                           uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                           uint32_t *out_len, uint32_t count, uint32_t max_in_len, void *work, void *stream)
{
    if (!count || !in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !work)
        return LZF_GPU_EARG;
    if (max_in_len > LZF_GPU_MAX_VALUE) return LZF_GPU_EARG;
    int rc = current_device_ok();
    if (rc) return rc;
    return mixed_call(LZF_GPU_KIND_COMPRESS, in, in_off, in_len, out, out_off, out_cap, out_len, nullptr, count,
                      max_in_len, work, (hipStream_t)stream);
}

int lzf_gpu_decompress_mixed(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                             uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                             uint32_t *out_len, int32_t *err, uint32_t count,
                             uint32_t max_out_cap, void *work, void *stream)
{
    if (!count || !in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !err || !work)
        return LZF_GPU_EARG;
    int rc = current_device_ok();
    if (rc) return rc;
    return mixed_call(LZF_GPU_KIND_DECOMPRESS, in, in_off, in_len, out, out_off, out_cap, out_len, err, count,
                      max_out_cap, work, (hipStream_t)stream);
}

int lzf_gpu_mixed_last_plan(uint32_t *class_count, uint32_t *class_max, int *route, int max)
{
    for (int c = 0; c < max && c < (int)MIXED_NC; c++) {
        if (class_count) class_count[c] = g_plan_count[c];
        if (class_max) class_max[c] = g_plan_max[c];
        if (route) route[c] = g_plan_route[c];
    }
    return (int)g_last_mixed;
}

int lzf_gpu_compress_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                           uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                           uint32_t *out_len, uint32_t count, uint32_t max_in_len, void *stream)
{
    if (!count || !in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len) return LZF_GPU_EARG;
    if (max_in_len > LZF_GPU_MAX_VALUE) return LZF_GPU_EARG;
    int rc = current_device_ok();
    if (rc) return rc;
    if (!max_in_len)                  /* every value empty: out_len 0 each (src/lzf_c.c:131) */
        return hipMemsetAsync(out_len, 0, (size_t)count * sizeof(uint32_t), (hipStream_t)stream) == hipSuccess
                   ? LZF_GPU_OK
                   : LZF_GPU_ELAUNCH;
    LzfBatch b{in, in_off, in_len, out, out_off, out_cap, out_len, nullptr, count, max_in_len};
    const hipError_t e = launch_compress(b, (hipStream_t)stream);
    return e == hipSuccess ? LZF_GPU_OK : code_of(e);
}

int lzf_gpu_decompress_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                             uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                             uint32_t *out_len, int32_t *err, uint32_t count,
                             uint32_t max_out_cap, void *stream)
{
    if (!count || !in || !in_off || !in_len || !out || !out_off || !out_cap || !out_len || !err)
        return LZF_GPU_EARG;
    int rc = current_device_ok();
    if (rc) return rc;
    LzfBatch b{in, in_off, in_len, out, out_off, out_cap, out_len, err, count, max_out_cap};
    const hipError_t e = launch_decompress(b, (hipStream_t)stream);
    return e == hipSuccess ? LZF_GPU_OK : code_of(e);
}

int lzf_gpu_synth_fill(int kind, uint64_t seed, uint64_t first, uint64_t stride, uint32_t count,
                       uint32_t n, uint8_t *out, void *stream)
{
    if (!count || !n || !out || kind < 0) return LZF_GPU_EARG;
    int rc = current_device_ok();
    if (rc) return rc;
    return lzf_launch_synth(kind, seed, first, stride, count, n, out, (hipStream_t)stream) ==
                   hipSuccess
               ? LZF_GPU_OK
               : LZF_GPU_ELAUNCH;
}

int lzf_gpu_decoded_size_batch(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                               uint32_t *out_size, int32_t *err, uint32_t count, uint32_t out_limit, void *stream)
{
    if (!count || !in || !in_off || !in_len || !out_size || !err) return LZF_GPU_EARG;
    int rc = current_device_ok();
    if (rc) return rc;
    return lzf_launch_dsize(in, in_off, in_len, out_size, err, count, out_limit, (hipStream_t)stream) == hipSuccess
               ? LZF_GPU_OK
               : LZF_GPU_ELAUNCH;
}

uint64_t lzf_gpu_kv_frame_work_size(uint32_t count)
{
    return lzf_frame_work_bytes(count);
}

int lzf_gpu_kv_frame(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                     const uint8_t *vals, const uint64_t *val_off, const uint32_t *val_size,
                     const uint8_t *enc, const uint32_t *val_len, uint32_t count,
                     uint32_t elements, uint32_t max_val_len, int reply_header,
                     uint8_t *frame, uint64_t max_response, uint64_t *frame_len, void *work,
                     void *stream)
{
    if (!count || !keys || !key_off || !key_len || !vals || !val_off || !val_size || !enc ||
        !val_len || !frame || !frame_len || !work)
        return LZF_GPU_EARG;
    if (max_val_len > LZF_GPU_MAX_VALUE) return LZF_GPU_EARG;
    int rc = current_device_ok();
    if (rc) return rc;
    LzfFrameArgs a{};
    a.keys = keys; a.key_off = key_off; a.key_len = key_len;
    a.vals = vals; a.val_off = val_off; a.val_size = val_size;
    a.enc = enc; a.val_len = val_len;
    a.count = count; a.elements = elements; a.max_val_len = max_val_len ? max_val_len : 1u;
    a.reply_header = reply_header;
    a.max_response = max_response;
    a.frame = frame; a.frame_len = frame_len;
    lzf_frame_carve(a, work);
    return lzf_launch_frame(a, (hipStream_t)stream, launch_decompress) == hipSuccess ? LZF_GPU_OK
                                                                                    : LZF_GPU_ELAUNCH;
}

uint64_t lzf_gpu_set_store_work_size(uint32_t count, uint64_t in_bytes)
{
    return lzf_store_work_bytes(count, in_bytes);
}

int lzf_gpu_set_store(const uint8_t *in, const uint64_t *in_off, const uint32_t *in_len,
                      uint32_t count, uint32_t max_in_len, uint64_t in_bytes, uint32_t compression,
                      uint8_t *store, uint64_t store_cap, uint64_t *store_used,
                      uint64_t *val_off, uint32_t *val_size, uint8_t *enc, uint32_t *status,
                      void *work, void *stream)
{
    if (!count || !in || !in_off || !in_len || !store || !store_used || !val_off || !val_size || !enc ||
        !status || !work)
        return LZF_GPU_EARG;
    if (max_in_len > LZF_GPU_MAX_VALUE || !store_cap) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfStoreArgs a{};
    a.in = in; a.in_off = in_off; a.in_len = in_len;
    a.count = count; a.max_in_len = max_in_len; a.compression = compression;
    a.in_bytes = in_bytes;
    a.store = store; a.store_cap = store_cap; a.store_used = store_used;
    a.val_off = val_off; a.val_size = val_size; a.enc = enc; a.status = status;
    lzf_store_carve(a, work);
    return rc_of(lzf_launch_store(a, (hipStream_t)stream, store_compress));
}

int lzf_gpu_store_delete(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count, void *stream)
{
    if (!idx || !enc || !count) return LZF_GPU_EARG;
    if (!n) return LZF_GPU_OK;
    if (const int rc = current_device_ok()) return rc;
    return rc_of(lzf_launch_store_delete(idx, n, enc, count, (hipStream_t)stream));
}

int lzf_gpu_store_expire(const int64_t *item_time, const int32_t *ttl, int64_t now,
                         uint8_t *enc, uint32_t count, uint32_t *expired, void *stream)
{
    if (!item_time || !ttl || !enc || !expired || !count) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    /* the sweep reads the time arrays only */
    const LzfItems it = items_of(enc, count, const_cast<int64_t *>(item_time), const_cast<int32_t *>(ttl), nullptr,
                                 nullptr, now);
    return rc_of(lzf_launch_store_expire(it, expired, (hipStream_t)stream));
}

uint64_t lzf_gpu_store_compact_work_size(uint32_t count)
{
    return lzf_compact_work_bytes(count);
}

int lzf_gpu_store_usage(const uint32_t *val_size, const uint8_t *enc, uint32_t count,
                        uint64_t *report, void *work, void *stream)
{
    if (!val_size || !enc || !count || !report || !work) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfCompactArgs a{};
    a.val_size = const_cast<uint32_t *>(val_size);         /* usage only reads */
    a.enc = enc; a.count = count; a.report = report;
    lzf_compact_carve(a, work);
    return rc_of(lzf_launch_store_usage(a, (hipStream_t)stream));
}

int lzf_gpu_store_compact(const uint8_t *src, uint64_t src_cap,
                          uint64_t *val_off, uint32_t *val_size, const uint8_t *enc, uint32_t count,
                          uint8_t *dst, uint64_t dst_cap, uint64_t *dst_used,
                          uint64_t *report, uint32_t *status, void *work, void *stream)
{
    if (!src || !val_off || !val_size || !enc || !dst || !dst_used || !report || !status || !work)
        return LZF_GPU_EARG;
    if (!count || !src_cap || !dst_cap) return LZF_GPU_EARG;
    /* a semispace copy: the arenas must not share a byte.  The ends saturate */
    const uint64_t s0 = (uint64_t)(uintptr_t)src, d0 = (uint64_t)(uintptr_t)dst;
    const uint64_t s1 = s0 + src_cap < s0 ? ~0ull : s0 + src_cap, d1 = d0 + dst_cap < d0 ? ~0ull : d0 + dst_cap;
    if (d0 < s1 && s0 < d1) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfCompactArgs a{};
    a.src = src; a.src_cap = src_cap;
    a.val_off = val_off; a.val_size = val_size; a.enc = enc; a.count = count;
    a.dst = dst; a.dst_cap = dst_cap; a.dst_used = dst_used;
    a.report = report; a.status = status;
    lzf_compact_carve(a, work);
    return rc_of(lzf_launch_store_compact(a, (hipStream_t)stream));
}

uint64_t lzf_gpu_store_renumber_work_size(uint32_t count)
{
    return lzf_renumber_work_bytes(count);
}

/* the public struct's members, one for one */
static LzfItemArrays arrays_of(const lzf_store_items *p)
{
    return LzfItemArrays{p->val_off, p->val_size, p->enc, p->val_len, p->key_off, p->key_len,
                         p->item_time, p->item_ttl, p->item_lock, p->last_access};
}

int lzf_gpu_store_renumber(const lzf_store_items *src, uint32_t count,
                           const uint8_t *src_keys, uint64_t src_keys_cap,
                           const lzf_store_items *dst, uint32_t dst_cap,
                           uint8_t *dst_keys, uint64_t dst_keys_cap, uint64_t *dst_keys_used,
                           uint32_t *remap, uint64_t *report, uint32_t *status,
                           void *work, void *stream)
{
    if (!src || !dst || !src_keys || !dst_keys || !dst_keys_used || !report || !status || !work) return LZF_GPU_EARG;
    if (!count || !dst_cap || !src_keys_cap || !dst_keys_cap) return LZF_GPU_EARG;
    const LzfItemArrays s = arrays_of(src), d = arrays_of(dst);
    const void *sp[10] = {s.val_off, s.val_size, s.enc, s.val_len, s.key_off, s.key_len,
                          s.item_time, s.item_ttl, s.item_lock, s.last_access};
    const void *dp[10] = {d.val_off, d.val_size, d.enc, d.val_len, d.key_off, d.key_len,
                          d.item_time, d.item_ttl, d.item_lock, d.last_access};
    for (int k = 0; k < 10; k++) {
        if (k < 6 && (!sp[k] || !dp[k])) return LZF_GPU_EARG;         /* the six required members */
        if (!sp[k] != !dp[k]) return LZF_GPU_EARG;                    /* an optional member: in both or in neither */
        if (sp[k] && sp[k] == dp[k]) return LZF_GPU_EARG;             /* a semispace copy: never in place */
    }
    if (!s.item_time != !s.item_ttl) return LZF_GPU_EARG;
    /* the key arenas must not share a byte.  The ends saturate */
    const uint64_t s0 = (uint64_t)(uintptr_t)src_keys, d0 = (uint64_t)(uintptr_t)dst_keys;
    const uint64_t s1 = s0 + src_keys_cap < s0 ? ~0ull : s0 + src_keys_cap;
    const uint64_t d1 = d0 + dst_keys_cap < d0 ? ~0ull : d0 + dst_keys_cap;
    if (d0 < s1 && s0 < d1) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfRenumberArgs a{};
    a.src = s; a.dst = d; a.count = count; a.dst_cap = dst_cap;
    a.src_keys = src_keys; a.src_keys_cap = src_keys_cap;
    a.dst_keys = dst_keys; a.dst_keys_cap = dst_keys_cap; a.dst_keys_used = dst_keys_used;
    a.remap = remap; a.report = report; a.status = status;
    lzf_renumber_carve(a, work);
    return rc_of(lzf_launch_store_renumber(a, (hipStream_t)stream));
}

int lzf_gpu_store_remap(uint32_t *idx, uint32_t n, const uint32_t *remap, uint32_t count, void *stream)
{
    if (!idx || !remap || !n || !count) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    return rc_of(lzf_launch_store_remap(idx, n, remap, count, (hipStream_t)stream));
}

uint64_t lzf_gpu_store_select_work_size(uint32_t count)
{
    return lzf_select_work_bytes(count);
}

int lzf_gpu_store_select_prefix(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                                const uint8_t *enc, uint32_t count,
                                const uint8_t *prefix, uint32_t prefix_len,
                                uint32_t *sel, uint32_t cap, uint32_t *result, void *work, void *stream)
{
    if (!keys || !key_off || !key_len || !enc || !prefix || !sel || !result || !work) return LZF_GPU_EARG;
    if (!count || !prefix_len || !cap) return LZF_GPU_EARG;   /* the reference asserts len > 0 */
    if (const int rc = current_device_ok()) return rc;
    LzfSelectArgs a{};
    a.keys = keys; a.key_off = key_off; a.key_len = key_len; a.enc = enc; a.count = count;
    a.prefix = prefix; a.prefix_len = prefix_len;
    a.sel = sel; a.cap = cap; a.result = result;
    lzf_select_carve(a, work);
    return rc_of(lzf_launch_store_select(a, (hipStream_t)stream));
}

uint64_t lzf_gpu_store_select_ordered_work_size(uint32_t count, uint32_t cand_cap, uint64_t node_cap, uint32_t cap)
{
    return lzf_order_work_bytes(count, cand_cap, node_cap, cap);
}

int lzf_gpu_store_select_ordered(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                                 const uint8_t *enc, uint32_t count,
                                 const uint8_t *prefix, uint32_t prefix_len, int64_t limit,
                                 uint32_t cand_cap, uint64_t node_cap,
                                 uint32_t *sel, uint32_t cap, uint64_t *result, void *work, void *stream)
{
    if (!keys || !key_off || !key_len || !enc || !prefix || !sel || !result || !work) return LZF_GPU_EARG;
    if (!count || !prefix_len || !cap || !cand_cap || !node_cap) return LZF_GPU_EARG;
    if (lzf_order_work_bytes(count, cand_cap, node_cap, cap) == ~0ull) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfOrderArgs a{};
    a.keys = keys; a.key_off = key_off; a.key_len = key_len; a.enc = enc; a.count = count;
    a.prefix = prefix; a.prefix_len = prefix_len; a.limit = limit;
    a.cand_cap = cand_cap; a.node_cap = node_cap;
    a.sel = sel; a.cap = cap; a.result = result;
    lzf_order_carve(a, work);
    return rc_of(lzf_launch_store_select_ordered(a, (hipStream_t)stream));
}

int lzf_host_store_select_ordered(const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                                  const uint8_t *enc, uint32_t count,
                                  const uint8_t *prefix, uint32_t prefix_len, int64_t limit,
                                  uint32_t cand_cap, uint64_t node_cap,
                                  uint32_t *sel, uint32_t cap, uint64_t *result)
{
    if (!keys || !key_off || !key_len || !enc || !prefix || !sel || !result) return LZF_GPU_EARG;
    if (!count || !prefix_len || !cap || !cand_cap || !node_cap) return LZF_GPU_EARG;
    return lzf_order_host(keys, key_off, key_len, enc, count, prefix, prefix_len, limit, cand_cap, node_cap, sel,
                          cap, result);
}

uint64_t lzf_gpu_store_mget_work_size(uint32_t n)
{
    return lzf_mget_work_bytes(n);
}

int lzf_gpu_store_mget(const uint32_t *idx, uint32_t n,
                       const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                       const uint8_t *store, const uint64_t *val_off, const uint32_t *val_size,
                       uint8_t *enc, const uint32_t *val_len, uint32_t count,
                       const int64_t *item_time, const int32_t *item_ttl, int64_t now,
                       int64_t *last_access, uint32_t max_val_len, int reply_header,
                       uint8_t *frame, uint64_t max_response, uint64_t *frame_len,
                       uint64_t *result, void *work, void *stream)
{
    if (!idx || !keys || !key_off || !key_len || !store || !val_off || !val_size || !enc || !val_len ||
        !frame || !frame_len || !result || !work)
        return LZF_GPU_EARG;
    if (!n || !count || !item_time != !item_ttl) return LZF_GPU_EARG;
    if (max_val_len > LZF_GPU_MAX_VALUE) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfMgetArgs a{};
    a.idx = idx; a.n = n;
    a.keys = keys; a.key_off = key_off; a.key_len = key_len;
    a.store = store; a.val_off = val_off; a.val_size = val_size; a.val_len = val_len;
    /* MGET reads the time arrays only */
    a.it = items_of(enc, count, const_cast<int64_t *>(item_time), const_cast<int32_t *>(item_ttl), nullptr, last_access,
                    now);
    a.max_val_len = max_val_len ? max_val_len : 1u;
    a.reply_header = reply_header;
    a.frame = frame; a.max_response = max_response; a.frame_len = frame_len; a.result = result;
    lzf_mget_carve(a, work);
    return rc_of(lzf_launch_store_mget(a, (hipStream_t)stream, launch_decompress));
}

uint64_t lzf_gpu_store_replies_work_size(uint32_t n)
{
    return lzf_reply_work_bytes(n);
}

int lzf_gpu_store_replies(const uint32_t *idx, uint32_t n, int mode, const uint8_t *op_status,
                          const uint8_t *store, const uint64_t *val_off, const uint32_t *val_size,
                          uint8_t *enc, const uint32_t *val_len, uint32_t count,
                          const int64_t *item_time, const int32_t *item_ttl, int64_t now,
                          int64_t *last_access, uint32_t max_val_len,
                          uint8_t *replies, uint64_t rep_cap, uint64_t *rep_used,
                          uint64_t *rep_off, uint32_t *rep_len, uint8_t *entry_status,
                          uint64_t *result, void *work, void *stream)
{
    if (!idx || !store || !val_off || !val_size || !enc || !val_len || !replies || !rep_used || !rep_off ||
        !rep_len || !entry_status || !result || !work)
        return LZF_GPU_EARG;
    if (!n || !count || !item_time != !item_ttl) return LZF_GPU_EARG;
    if (mode != LZF_REPLY_GET && mode != LZF_REPLY_VALUE) return LZF_GPU_EARG;
    if ((mode == LZF_REPLY_VALUE) != (op_status != nullptr)) return LZF_GPU_EARG;
    if (max_val_len > LZF_GPU_MAX_VALUE) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    /* one decode launch bounded by max_val_len, as MGET's, is the measured
     * default; LZF_GPU_REPLY_ONE_ROUTE=0 runs one launch per
     * decode size class.  Read per call, so one process can time both in turn */
    const char *route = getenv("LZF_GPU_REPLY_ONE_ROUTE");
    const bool one_route = !(route && !strcmp(route, "0"));
    LzfReplyArgs a{};
    a.idx = idx; a.n = n; a.mode = mode; a.op_status = op_status;
    a.store = store; a.val_off = val_off; a.val_size = val_size; a.val_len = val_len;
    /* the replies read the time arrays only */
    a.it = items_of(enc, count, const_cast<int64_t *>(item_time), const_cast<int32_t *>(item_ttl), nullptr, last_access,
                    now);
    a.max_val_len = max_val_len ? max_val_len : 1u;
    a.replies = replies; a.rep_cap = rep_cap; a.rep_used = rep_used;
    a.rep_off = rep_off; a.rep_len = rep_len; a.entry_status = entry_status; a.result = result;
    lzf_reply_carve(a, work);
    return rc_of(lzf_launch_store_replies(a, (hipStream_t)stream, launch_decompress, one_route));
}

int lzf_host_reply_code(int ent_status)
{
    return lzf_reply_code(ent_status);
}

/* the arguments of both request parses; false: LZF_GPU_EARG */
static bool request_args(LzfRequestArgs &a, const uint8_t *req, uint64_t req_bytes, const uint64_t *req_off,
                         const uint32_t *req_len, uint32_t n, uint32_t max_key, uint32_t max_value, uint32_t expect_op,
                         uint8_t *op, uint8_t *status, uint64_t *key_off, uint32_t *key_len, uint64_t *val_off,
                         uint32_t *val_len, int64_t *num, uint64_t *result)
{
    if (!req || !req_off || !req_len || !op || !status || !key_off || !key_len || !val_off || !val_len || !num ||
        !result)
        return false;
    if (!n || !max_key || !max_value) return false;
    a = LzfRequestArgs{req, req_bytes, req_off, req_len, n, max_key, max_value, expect_op,
                       op, status, key_off, val_off, key_len, val_len, num, result};
    return true;
}

int lzf_gpu_request_parse(const uint8_t *req, uint64_t req_bytes, const uint64_t *req_off, const uint32_t *req_len,
                          uint32_t n, uint32_t max_key, uint32_t max_value, uint32_t expect_op,
                          uint8_t *op, uint8_t *status, uint64_t *key_off, uint32_t *key_len,
                          uint64_t *val_off, uint32_t *val_len, int64_t *num, uint64_t *result, void *stream)
{
    LzfRequestArgs a{};
    if (!request_args(a, req, req_bytes, req_off, req_len, n, max_key, max_value, expect_op, op, status, key_off,
                      key_len, val_off, val_len, num, result))
        return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    return rc_of(lzf_launch_request_parse(a, (hipStream_t)stream));
}

int lzf_host_request_parse(const uint8_t *req, uint64_t req_bytes, const uint64_t *req_off, const uint32_t *req_len,
                           uint32_t n, uint32_t max_key, uint32_t max_value, uint32_t expect_op,
                           uint8_t *op, uint8_t *status, uint64_t *key_off, uint32_t *key_len,
                           uint64_t *val_off, uint32_t *val_len, int64_t *num, uint64_t *result)
{
    LzfRequestArgs a{};
    if (!request_args(a, req, req_bytes, req_off, req_len, n, max_key, max_value, expect_op, op, status, key_off,
                      key_len, val_off, val_len, num, result))
        return LZF_GPU_EARG;
    for (uint32_t c = 0; c < LZF_REQ_NSTATUS; c++) result[c] = 0ull;
    for (uint32_t k = 0; k < n; k++) result[lzf_request_entry(a, k)]++;
    return LZF_GPU_OK;
}

int lzf_host_request_reply_code(int status)
{
    return lzf_request_reply_code_of(status);
}

uint64_t lzf_gpu_store_append_keys_work_size(uint32_t n)
{
    return lzf_append_work_bytes(n);
}

int lzf_gpu_store_append_keys(const uint8_t *req, uint64_t req_bytes, const uint8_t *op, const uint8_t *status,
                              const uint64_t *rq_key_off, const uint32_t *rq_key_len, const uint32_t *rq_val_len,
                              const int64_t *num, uint32_t n, uint8_t *keys, uint64_t keys_cap, uint64_t *keys_used,
                              uint64_t *key_off, uint32_t *key_len, int64_t *item_time, int32_t *item_ttl,
                              int64_t *item_lock, int64_t *last_access, uint32_t first, uint32_t count, int64_t now,
                              int32_t max_item_ttl, uint32_t *set_len, uint32_t *void_idx, uint64_t *result,
                              void *work, void *stream)
{
    if (!req || !op || !status || !rq_key_off || !rq_key_len || !rq_val_len || !num || !keys || !keys_used ||
        !key_off || !key_len || !set_len || !void_idx || !result || !work)
        return LZF_GPU_EARG;
    if (!n || !count || !keys_cap || (uint64_t)first + n > count || !item_time != !item_ttl) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfAppendArgs a{};
    a.req = req; a.req_bytes = req_bytes; a.op = op; a.status = status;
    a.rq_key_off = rq_key_off; a.rq_key_len = rq_key_len; a.rq_val_len = rq_val_len; a.num = num;
    a.n = n; a.first = first;
    a.keys = keys; a.keys_cap = keys_cap; a.keys_used = keys_used;
    a.key_off = key_off; a.key_len = key_len;
    a.item_time = item_time; a.item_ttl = item_ttl; a.item_lock = item_lock; a.last_access = last_access;
    a.now = now; a.max_item_ttl = max_item_ttl;
    a.set_len = set_len; a.void_idx = void_idx; a.result = result;
    lzf_append_carve(a, work);
    return rc_of(lzf_launch_store_append_keys(a, (hipStream_t)stream));
}

int lzf_host_request_class(int op, int status)
{
    return (int)lzf_request_class_of((uint32_t)op, (uint32_t)status);
}

uint64_t lzf_gpu_request_bucket_work_size(uint32_t n)
{
    return lzf_bucket_work_bytes(n);
}

/* the arguments of both buckets; false: LZF_GPU_EARG */
static bool bucket_args(LzfBucketArgs &a, const uint8_t *op, const uint8_t *status, const uint64_t *key_off,
                        const uint32_t *key_len, const uint64_t *val_off, const uint32_t *val_len, const int64_t *num,
                        uint32_t n, uint32_t *perm, uint32_t *slot, uint32_t *class_first, uint8_t *b_op,
                        uint8_t *b_status, uint64_t *b_key_off, uint32_t *b_key_len, uint64_t *b_val_off,
                        uint32_t *b_val_len, int64_t *b_num)
{
    if (!op || !status || !key_off || !key_len || !val_off || !val_len || !num || !perm || !slot || !class_first ||
        !b_op || !b_status || !b_key_off || !b_key_len || !b_val_off || !b_val_len || !b_num || !n)
        return false;
    a.op = op; a.status = status; a.key_off = key_off; a.key_len = key_len;
    a.val_off = val_off; a.val_len = val_len; a.num = num; a.n = n;
    a.perm = perm; a.slot = slot; a.class_first = class_first;
    a.b_op = b_op; a.b_status = b_status; a.b_key_off = b_key_off; a.b_key_len = b_key_len;
    a.b_val_off = b_val_off; a.b_val_len = b_val_len; a.b_num = b_num;
    return true;
}

int lzf_gpu_request_bucket(const uint8_t *op, const uint8_t *status, const uint64_t *key_off, const uint32_t *key_len,
                           const uint64_t *val_off, const uint32_t *val_len, const int64_t *num, uint32_t n,
                           uint32_t *perm, uint32_t *slot, uint32_t *class_first, uint8_t *b_op, uint8_t *b_status,
                           uint64_t *b_key_off, uint32_t *b_key_len, uint64_t *b_val_off, uint32_t *b_val_len,
                           int64_t *b_num, void *work, void *stream)
{
    LzfBucketArgs a{};
    if (!bucket_args(a, op, status, key_off, key_len, val_off, val_len, num, n, perm, slot, class_first, b_op,
                     b_status, b_key_off, b_key_len, b_val_off, b_val_len, b_num) ||
        !work)
        return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    lzf_bucket_carve(a, work);
    return rc_of(lzf_launch_request_bucket(a, (hipStream_t)stream));
}

int lzf_host_request_bucket(const uint8_t *op, const uint8_t *status, const uint64_t *key_off, const uint32_t *key_len,
                            const uint64_t *val_off, const uint32_t *val_len, const int64_t *num, uint32_t n,
                            uint32_t *perm, uint32_t *slot, uint32_t *class_first, uint8_t *b_op, uint8_t *b_status,
                            uint64_t *b_key_off, uint32_t *b_key_len, uint64_t *b_val_off, uint32_t *b_val_len,
                            int64_t *b_num)
{
    LzfBucketArgs a{};
    if (!bucket_args(a, op, status, key_off, key_len, val_off, val_len, num, n, perm, slot, class_first, b_op,
                     b_status, b_key_off, b_key_len, b_val_off, b_val_len, b_num))
        return LZF_GPU_EARG;
    lzf_request_bucket_host(op, status, key_off, key_len, val_off, val_len, num, n, perm, slot, class_first, b_op,
                            b_status, b_key_off, b_key_len, b_val_off, b_val_len, b_num);
    return LZF_GPU_OK;
}

/* the arguments of both stitches; false: LZF_GPU_EARG */
static bool stitch_args(LzfStitchArgs &a, const uint8_t *op, const uint8_t *status, const uint32_t *slot,
                            uint32_t n, const uint32_t *class_first, const uint8_t *class_mode,
                            const uint64_t *class_base, const uint64_t *b_rep_off, const uint32_t *b_rep_len,
                            const uint8_t *b_ent, const uint8_t *b_refused, uint8_t *replies, uint64_t rep_cap,
                            uint64_t code_base, uint64_t *out_off, uint32_t *out_len, uint8_t *out_kind,
                            uint64_t *result)
{
    if (!op || !status || !slot || !class_first || !class_mode || !class_base || !replies || !out_off || !out_len ||
        !out_kind || !result || !n)
        return false;
    if (rep_cap < LZF_STITCH_CODES || code_base > rep_cap - LZF_STITCH_CODES) return false;
    a.op = op; a.status = status; a.slot = slot; a.class_first = class_first; a.n = n;
    for (uint32_t c = 0; c < (uint32_t)LZF_RQ_NCLASS; c++) {
        if (class_mode[c] > (uint8_t)LZF_STITCH_CODE) return false;
        if (class_mode[c] == (uint8_t)LZF_STITCH_ARENA && (!b_rep_off || !b_rep_len)) return false;
        if (class_mode[c] == (uint8_t)LZF_STITCH_CODE && !b_ent) return false;
        a.class_mode[c] = class_mode[c];
        a.class_base[c] = class_base[c];
    }
    a.b_rep_off = b_rep_off; a.b_rep_len = b_rep_len; a.b_ent = b_ent; a.b_refused = b_refused;
    a.replies = replies; a.rep_cap = rep_cap; a.code_base = code_base;
    a.out_off = out_off; a.out_len = out_len; a.out_kind = out_kind; a.result = result;
    return true;
}

int lzf_gpu_request_stitch(const uint8_t *op, const uint8_t *status, const uint32_t *slot, uint32_t n,
                           const uint32_t *class_first, const uint8_t *class_mode, const uint64_t *class_base,
                           const uint64_t *b_rep_off, const uint32_t *b_rep_len, const uint8_t *b_ent,
                           const uint8_t *b_refused, uint8_t *replies, uint64_t rep_cap, uint64_t code_base,
                           uint64_t *out_off, uint32_t *out_len, uint8_t *out_kind, uint64_t *result, void *stream)
{
    LzfStitchArgs a{};
    if (!stitch_args(a, op, status, slot, n, class_first, class_mode, class_base, b_rep_off, b_rep_len, b_ent,
                         b_refused, replies, rep_cap, code_base, out_off, out_len, out_kind, result))
        return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    return rc_of(lzf_launch_request_stitch(a, (hipStream_t)stream));
}

int lzf_host_request_stitch(const uint8_t *op, const uint8_t *status, const uint32_t *slot, uint32_t n,
                            const uint32_t *class_first, const uint8_t *class_mode, const uint64_t *class_base,
                            const uint64_t *b_rep_off, const uint32_t *b_rep_len, const uint8_t *b_ent,
                            const uint8_t *b_refused, uint8_t *replies, uint64_t rep_cap, uint64_t code_base,
                            uint64_t *out_off, uint32_t *out_len, uint8_t *out_kind, uint64_t *result)
{
    LzfStitchArgs a{};
    if (!stitch_args(a, op, status, slot, n, class_first, class_mode, class_base, b_rep_off, b_rep_len, b_ent,
                         b_refused, replies, rep_cap, code_base, out_off, out_len, out_kind, result))
        return LZF_GPU_EARG;
    lzf_request_stitch_host(a);
    return LZF_GPU_OK;
}

int lzf_gpu_store_count(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count,
                        const int64_t *item_time, const int32_t *item_ttl, int64_t now,
                        int64_t *last_access, uint64_t *result, void *stream)
{
    if (!idx || !enc || !result || !n || !count || !item_time != !item_ttl) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    /* COUNT reads the time arrays only */
    const LzfItems it = items_of(enc, count, const_cast<int64_t *>(item_time), const_cast<int32_t *>(item_ttl), nullptr,
                                 last_access, now);
    return rc_of(lzf_launch_store_count(idx, n, it, result, (hipStream_t)stream));
}

int lzf_gpu_store_mttl(const uint32_t *idx, uint32_t n, int32_t ttl, uint8_t *enc, uint32_t count,
                       int64_t *item_time, int32_t *item_ttl, int64_t now,
                       int64_t *last_access, uint64_t *result, void *stream)
{
    if (!idx || !enc || !item_time || !item_ttl || !result || !n || !count) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    const LzfItems it = items_of(enc, count, item_time, item_ttl, nullptr, last_access, now);
    return rc_of(lzf_launch_store_mttl(idx, n, ttl, it, result, (hipStream_t)stream));
}

int lzf_gpu_store_mlock(const uint32_t *idx, uint32_t n, int64_t lock_time, uint8_t *enc, uint32_t count,
                        int64_t *item_time, const int32_t *item_ttl, int64_t *item_lock, int64_t now,
                        int64_t *last_access, uint8_t *entry_status, uint64_t *result, void *stream)
{
    if (!idx || !enc || !item_time || !item_ttl || !item_lock || !result || !n || !count) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfLockArgs a{};
    a.idx = idx; a.n = n; a.lock_time = lock_time;
    /* MLOCK only reads the ttl */
    a.it = items_of(enc, count, item_time, const_cast<int32_t *>(item_ttl), item_lock, last_access, now);
    a.entry_status = entry_status; a.result = result;
    return rc_of(lzf_launch_store_mlock(a, (hipStream_t)stream));
}

int lzf_gpu_store_munlock(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count,
                          const int64_t *item_time, const int32_t *item_ttl, int64_t *item_lock, int64_t now,
                          int64_t *last_access, uint8_t *entry_status, uint64_t *result, void *stream)
{
    if (!idx || !enc || !item_time || !item_ttl || !item_lock || !result || !n || !count) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfLockArgs a{};
    a.idx = idx; a.n = n;
    /* MUNLOCK only reads the time arrays */
    a.it = items_of(enc, count, const_cast<int64_t *>(item_time), const_cast<int32_t *>(item_ttl), item_lock,
                    last_access, now);
    a.entry_status = entry_status; a.result = result;
    return rc_of(lzf_launch_store_munlock(a, (hipStream_t)stream));
}

int lzf_gpu_store_mdel(const uint32_t *idx, uint32_t n, uint8_t *enc, uint32_t count,
                       const int64_t *item_time, const int32_t *item_ttl, const int64_t *item_lock,
                       int64_t now, uint8_t *entry_status, uint64_t *result, void *stream)
{
    if (!idx || !enc || !result || !n || !count) return LZF_GPU_EARG;
    if (!item_time != !item_ttl || (item_lock && !item_time)) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfLockArgs a{};
    a.idx = idx; a.n = n;
    /* MDEL reads the time arrays and the locks only */
    a.it = items_of(enc, count, const_cast<int64_t *>(item_time), const_cast<int32_t *>(item_ttl),
                    const_cast<int64_t *>(item_lock), nullptr, now);
    a.entry_status = entry_status; a.result = result;
    return rc_of(lzf_launch_store_mdel(a, (hipStream_t)stream));
}

uint64_t lzf_gpu_store_minc_work_size(uint32_t n)
{
    return lzf_minc_work_bytes(n);
}

int lzf_gpu_store_minc(const uint32_t *idx, uint32_t n, int64_t delta, int single,
                       uint8_t *store, uint64_t store_cap, uint64_t *store_used,
                       uint64_t *val_off, uint32_t *val_size, uint8_t *enc, uint32_t count,
                       const int64_t *item_time, const int32_t *item_ttl, const int64_t *item_lock, int64_t now,
                       int64_t *last_access, uint8_t *entry_status, int64_t *entry_value,
                       uint64_t *result, uint32_t *status, void *work, void *stream)
{
    if (!idx || !store || !store_used || !val_off || !val_size || !enc || !result || !status || !work)
        return LZF_GPU_EARG;
    if (!n || !count || !item_time != !item_ttl || (item_lock && !item_time)) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfMincArgs a{};
    a.idx = idx; a.n = n; a.delta = delta; a.single = single ? 1 : 0;
    a.store = store; a.store_cap = store_cap; a.store_used = store_used;
    a.val_off = val_off; a.val_size = val_size;
    /* INC / DEC read the time arrays and the locks only */
    a.it = items_of(enc, count, const_cast<int64_t *>(item_time), const_cast<int32_t *>(item_ttl),
                    const_cast<int64_t *>(item_lock), last_access, now);
    a.entry_status = entry_status; a.entry_value = entry_value;
    a.result = result; a.status = status;
    lzf_minc_carve(a, work);
    return rc_of(lzf_launch_store_minc(a, (hipStream_t)stream));
}

int lzf_host_parse_long(const uint8_t *v, uint32_t len, int64_t *out)
{
    if (!v || !out) return 0;
    return lzf_ops_parse_long(v, len, out);
}

int lzf_gpu_store_set_guard(const uint32_t *occ, uint32_t first, uint32_t n, uint8_t *enc, uint32_t count,
                            const int64_t *item_time, const int64_t *item_lock, int64_t now,
                            uint8_t *refused, uint64_t *result, void *stream)
{
    if (!occ || !enc || !item_time || !item_lock || !result) return LZF_GPU_EARG;
    if (!count || !n || (uint64_t)first + n > count) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    /* the guard reads the times and the locks only */
    const LzfItems it = items_of(enc, count, const_cast<int64_t *>(item_time), nullptr, const_cast<int64_t *>(item_lock),
                                 nullptr, now);
    return rc_of(lzf_launch_store_set_guard(occ, first, n, it, refused, result, (hipStream_t)stream));
}

uint64_t lzf_gpu_store_mset_work_size(uint32_t n, uint32_t vlen)
{
    return lzf_mset_work_bytes(n, vlen);
}

int lzf_gpu_store_mset(const uint32_t *idx, uint32_t n, const uint8_t *value, uint32_t vlen, uint32_t compression,
                       uint8_t *store, uint64_t store_cap, uint64_t *store_used,
                       uint64_t *val_off, uint32_t *val_size, uint8_t *enc, uint32_t *val_len, uint32_t count,
                       int64_t *item_time, int32_t *item_ttl, int64_t *item_lock, int64_t now,
                       int64_t *last_access, uint8_t *entry_status, uint64_t *result, uint32_t *status,
                       void *work, void *stream)
{
    if (!idx || !value || !store || !store_used || !val_off || !val_size || !enc || !val_len || !item_time ||
        !item_ttl || !result || !status || !work)
        return LZF_GPU_EARG;
    if (!n || !count || !store_cap) return LZF_GPU_EARG;
    if (!vlen || vlen > LZF_GPU_MAX_VALUE) return LZF_GPU_EARG;   /* the reference asserts vlen > 0 */
    if (const int rc = current_device_ok()) return rc;
    LzfMsetArgs a{};
    a.idx = idx; a.n = n; a.value = value; a.vlen = vlen; a.compression = compression;
    a.store = store; a.store_cap = store_cap; a.store_used = store_used;
    a.val_off = val_off; a.val_size = val_size; a.val_len = val_len;
    a.it = items_of(enc, count, item_time, item_ttl, item_lock, last_access, now);
    a.entry_status = entry_status; a.result = result; a.status = status;
    lzf_mset_carve(a, work);
    return rc_of(lzf_launch_store_mset(a, (hipStream_t)stream, store_compress));
}

int lzf_gpu_store_gc(const int64_t *last_access, int64_t now, int64_t gc_ratio,
                     uint8_t *enc, const uint32_t *val_size, uint32_t count,
                     const uint64_t *gate, uint64_t max_bytes, uint64_t *result, void *stream)
{
    if (!last_access || !enc || !val_size || !result || !count) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    /* the sweep only reads last_access */
    const LzfItems it = items_of(enc, count, nullptr, nullptr, nullptr, const_cast<int64_t *>(last_access), now);
    return rc_of(lzf_launch_store_gc(it, gc_ratio, val_size, gate, max_bytes, result, (hipStream_t)stream));
}

int lzf_host_meta_field(const uint8_t *m, uint32_t mlen)
{
    return lzf_meta_field(m, mlen);
}

int lzf_gpu_store_meta(const uint32_t *idx, uint32_t n, int field, uint8_t *enc, const uint32_t *val_size,
                       uint32_t count, const int64_t *item_time, const int32_t *item_ttl,
                       const int64_t *item_lock, int64_t now, int64_t *last_access,
                       uint8_t *entry_status, int64_t *entry_value, uint64_t *result, void *stream)
{
    if (!idx || !enc || !val_size || !item_time || !item_ttl || !entry_value || !result) return LZF_GPU_EARG;
    if (!n || !count || field < LZF_META_SIZE || field > LZF_META_LOCK) return LZF_GPU_EARG;
    if (field == LZF_META_ACCESS && !last_access) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfMetaArgs a{};
    a.idx = idx; a.n = n; a.field = field; a.val_size = val_size;
    /* META reads the time arrays and the locks only */
    a.it = items_of(enc, count, const_cast<int64_t *>(item_time), const_cast<int32_t *>(item_ttl),
                    const_cast<int64_t *>(item_lock), last_access, now);
    a.entry_status = entry_status; a.entry_value = entry_value; a.result = result;
    return rc_of(lzf_launch_store_meta(a, (hipStream_t)stream));
}

uint64_t lzf_gpu_store_keys_work_size(uint32_t n)
{
    return lzf_keys_work_bytes(n);
}

int lzf_gpu_store_keys(const uint32_t *idx, uint32_t n,
                       const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                       const uint8_t *enc, uint32_t count, int reply_header,
                       uint8_t *frame, uint64_t max_response, uint64_t *frame_len,
                       uint64_t *result, void *work, void *stream)
{
    if (!idx || !keys || !key_off || !key_len || !enc || !frame || !frame_len || !result || !work)
        return LZF_GPU_EARG;
    if (!n || !count) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfKeysArgs a{};
    a.idx = idx; a.n = n; a.keys = keys; a.key_off = key_off; a.key_len = key_len; a.enc = enc; a.count = count;
    a.reply_header = reply_header;
    a.frame = frame; a.max_response = max_response; a.frame_len = frame_len; a.result = result;
    lzf_keys_carve(a, work);
    return rc_of(lzf_launch_store_keys(a, (hipStream_t)stream));
}

uint64_t lzf_gpu_key_index_bytes(uint32_t slots)
{
    return lzf_kidx_slots_ok(slots) ? lzf_kidx_table_bytes(slots) : 0ull;
}

uint32_t lzf_host_key_home(const uint8_t *key, uint32_t len, uint32_t slots)
{
    if (!lzf_kidx_slots_ok(slots) || (!key && len)) return 0xFFFFFFFFu;
    return lzf_kidx_home(key, len, slots);
}

int lzf_gpu_key_index_insert(void *table, uint32_t slots, uint32_t *used,
                             const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                             uint8_t *enc, uint32_t count, uint32_t first, uint32_t n,
                             uint64_t *result, uint32_t *status, void *stream)
{
    if (!table || !used || !keys || !key_off || !key_len || !enc || !result || !status) return LZF_GPU_EARG;
    if (!count || !n || (uint64_t)first + n > count) return LZF_GPU_EARG;
    if (!lzf_kidx_slots_ok(slots) || ((uintptr_t)table & 7u)) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfKidxArgs a{};
    a.table = table; a.slots = slots; a.used = used;
    a.keys = keys; a.key_off = key_off; a.key_len = key_len;
    a.enc = enc; a.count = count; a.first = first; a.n = n;
    a.result = result; a.status = status;
    return rc_of(lzf_launch_kidx_insert(a, (hipStream_t)stream));
}

int lzf_gpu_key_index_rebuild(void *table, uint32_t slots, uint32_t *used,
                              const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                              uint8_t *enc, uint32_t count,
                              uint64_t *result, uint32_t *status, void *stream)
{
    if (!table || !used || !keys || !key_off || !key_len || !enc || !result || !status) return LZF_GPU_EARG;
    if (!count) return LZF_GPU_EARG;
    if (!lzf_kidx_slots_ok(slots) || ((uintptr_t)table & 7u)) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfKidxArgs a{};
    a.table = table; a.slots = slots; a.used = used;
    a.keys = keys; a.key_off = key_off; a.key_len = key_len;
    a.enc = enc; a.count = count; a.first = 0u; a.n = count;
    a.result = result; a.status = status;
    return rc_of(lzf_launch_kidx_rebuild(a, (hipStream_t)stream));
}

int lzf_gpu_key_index_lookup(const void *table, uint32_t slots,
                             const uint8_t *keys, const uint64_t *key_off, const uint32_t *key_len,
                             const uint8_t *enc, uint32_t count,
                             const uint8_t *qkeys, const uint64_t *q_off, const uint32_t *q_len, uint32_t nq,
                             uint32_t *idx, uint64_t *result, void *stream)
{
    if (!table || !keys || !key_off || !key_len || !enc || !qkeys || !q_off || !q_len || !idx || !result)
        return LZF_GPU_EARG;
    if (!count || !nq) return LZF_GPU_EARG;
    if (!lzf_kidx_slots_ok(slots) || ((uintptr_t)table & 7u)) return LZF_GPU_EARG;
    if (const int rc = current_device_ok()) return rc;
    LzfKidxArgs a{};
    a.table = const_cast<void *>(table); a.slots = slots;  /* the lookup only reads */
    a.keys = keys; a.key_off = key_off; a.key_len = key_len;
    a.enc = const_cast<uint8_t *>(enc); a.count = count;
    a.result = result;
    return rc_of(lzf_launch_kidx_lookup(a, qkeys, q_off, q_len, nq, idx, (hipStream_t)stream));
}

int lzf_gpu_selfcheck(void)
{
    int rc = current_device_ok();
    if (rc) return rc;
    const int st = lds_order_state(true);
    return st == 1 ? 1 : st == -1 ? 0 : LZF_GPU_ELAUNCH;
}

int lzf_gpu_lds_order_probe(void)
{
    int rc = current_device_ok();
    if (rc) return rc;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return LZF_GPU_ENODEV;
    return lzf_lds_order_check(dev);
}

const char *lzf_gpu_kernel_info(void)
{
    static thread_local std::string s;
    switch (kernel_gen()) {
#ifdef LZF_DIAG
    case GEN_SERIAL: s = "compress=serial decompress=serial"; break;
#endif
    case GEN_WINDOW:
        s = std::string("compress=") + lzf_compress_kernel_name() + " decompress=" +
            lzf_decompress_kernel_name();
        break;
#ifdef LZF_DIAG
    case GEN_WTAB:
        s = std::string("compress=wtab(cand_q1+wparse; window64 past 64 KiB) decompress=") +
            lzf_decompress_kernel_name();
        break;
#endif
    case GEN_TABLE_ONLY:
        s = std::string("compress=table(cand_table+parse_rec; window64 past 64 KiB or below ") +
            std::to_string(lane_min_count(4096u)) + " values of <= 4 KiB / " +
            std::to_string(lane_min_count(8192u)) + " of <= 8 KiB / " +
            std::to_string(lane_min_count(16384u)) + " of <= 16 KiB / " +
            std::to_string(lane_min_count(65536u)) + " of <= 64 KiB) decompress=" +
            (lane_decoder() ? "lane" : lzf_decompress_kernel_name());
        break;
    case GEN_LANE:
        s = std::string("compress=lane(") + lzf_lane_cand_name() + "+parse_lane; window64 past 64 KiB or below " +
            std::to_string(lane_min_count(4096u)) + " values of <= 4 KiB / " +
            std::to_string(lane_min_count(8192u)) + " of <= 8 KiB / " +
            std::to_string(lane_min_count(16384u)) + " of <= 16 KiB / " +
            std::to_string(lane_min_count(65536u)) + " of <= 64 KiB) decompress=" +
            (lane_decoder() ? "lane" : lzf_decompress_kernel_name());
        break;
    default:
        s = std::string("compress=lane(") + lzf_lane_cand_name() + "+parse_lane) up to " +
            std::to_string(LANE_DEFAULT_MAX / 1024u) + " KiB, table(cand_table+parse_rec) up to 64 KiB; window64 past 64 KiB or below " +
            std::to_string(lane_min_count(4096u)) + " values of <= 4 KiB / " +
            std::to_string(lane_min_count(8192u)) + " of <= 8 KiB / " +
            std::to_string(lane_min_count(16384u)) + " of <= 16 KiB / " +
            std::to_string(lane_min_count(65536u)) + " of <= 64 KiB) decompress=" +
            (lane_decoder() ? "lane" : lzf_decompress_kernel_name());
        break;
    }
    {
        const int st = lds_order_state(false);
        s += std::string(" lds_order=") + (st == 1 ? "held" : st == -1 ? "violated(compress->window64)"
                                           : st == -2 ? "probe-failed(retried)" : "unchecked");
        if (g_last_chunks) s += " scratch_chunks=" + std::to_string(g_last_chunks);
        /* class batches of the thread's last mixed call */
        if (g_last_mixed) s += " mixed=" + std::to_string(g_last_mixed);
    }
    return s.c_str();
}

}  // extern "C"
