// transfer.hip -- staged copies between pageable host memory and the device, and the threaded host-side array helpers of the
// drop-in class (nnd_host_*).  Nothing here knows the API: the entry points of capi.hip call the two copy functions.  No kernel.
#include <string.h>

#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

#include "common.h"
#include "state.h"

// Pageable host memory -> device.  The runtime stages such a copy through its own pinned buffers; how fast depends on the box
// (one staging thread, the NUMA node of the caller's pages): the same 488 MB took 9.7 ms on one MI355X host and visibly more on
// another (round-5 review: 32.9 vs 42.2 ms for the whole nnd_build call).  Here: eight pinned 8 MB buffers per device (allocated
// once per process), eight host threads -- thread t copies chunks t, t + 8, ... into ITS buffer and queues the DMA of each on the
// handle's stream itself (the chunks are independent; what follows on the stream is ordered behind all of them).  A pinned
// source is copied directly.  Each thread waits for its last DMA before the call returns: the staging events are shared by
// every handle of the device, and a later call (another handle, another stream) must never wait on an event last recorded
// on a stream that may have been destroyed since (such a wait has failed with hipErrorCapturedEvent, although no stream is
// ever captured in the process).
static std::mutex g_up_mu[64];  // per device: the ranks of nnd_build_multi upload side by side
static char *g_up_stage[64][16] = {};
static hipEvent_t g_up_ev[64][16] = {};
int nnd_h2d_parallel(nnd_ctx *ctx, void *dst_dev, const void *src, size_t bytes) {
    constexpr size_t STAGE = (size_t)8 << 20;
    int P = 8;  // staging threads (= buffers); 4 .. 16 measured the same 10.8 ms for 488 MB: the link, not the host copies, sets the rate
    if (const char *e = nnd_knob("NND_H2D_THREADS")) { const int v = atoi(e); if (v >= 1 && v <= 16) P = v; }
    bool direct = bytes < (size_t)(16u << 20) || ctx->p.device < 0 || ctx->p.device >= 64;
    if (!direct) {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, src) == hipSuccess && at.type == hipMemoryTypeHost) direct = true;
        else (void)hipGetLastError();
    }
    if (direct) {
        NND_HIP_CHECK(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
    const int dev = ctx->p.device;
    std::lock_guard<std::mutex> lk(g_up_mu[dev]);
    NND_HIP_CHECK(hipSetDevice(dev));
    for (int b = 0; b < P; b++) {
        if (!g_up_stage[dev][b] && hipHostMalloc((void **)&g_up_stage[dev][b], STAGE, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();  // no pinned memory for the staging buffers: the runtime's own pageable path
            g_up_stage[dev][b] = nullptr;
            NND_HIP_CHECK(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, ctx->stream));
            return 0;
        }
        if (!g_up_ev[dev][b]) NND_HIP_CHECK(hipEventCreateWithFlags(&g_up_ev[dev][b], hipEventDisableTiming));
    }
    const size_t nchunks = (bytes + STAGE - 1) / STAGE;
    std::atomic<int> failed{0};
    hipStream_t st = ctx->stream;
    auto work = [&](int t) {
        if (hipSetDevice(dev) != hipSuccess) { failed = 1; return; }
        bool first = true;
        for (size_t c = (size_t)t; c < nchunks && !failed; c += P) {
            const size_t o = c * STAGE, len = bytes - o < STAGE ? bytes - o : STAGE;
            if (!first && hipEventSynchronize(g_up_ev[dev][t]) != hipSuccess) { failed = 1; return; }
            first = false;
            memcpy(g_up_stage[dev][t], (const char *)src + o, len);
            if (hipMemcpyAsync((char *)dst_dev + o, g_up_stage[dev][t], len, hipMemcpyHostToDevice, st) != hipSuccess ||
                hipEventRecord(g_up_ev[dev][t], st) != hipSuccess) { failed = 1; return; }
        }
        if (!first && hipEventSynchronize(g_up_ev[dev][t]) != hipSuccess) failed = 1;  // this call's last DMA out of buffer t
    };
    std::vector<std::thread> th;
    for (int t = 1; t < P; t++) th.emplace_back(work, t);
    work(0);
    for (auto &t : th) t.join();
    if (failed) {  // (no DMA out of a staging buffer may outlive the call: the next one writes into them)
        (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
        ctx->set_error("nnd_set_data_host: staged host-to-device copy failed");
        return 1;
    }
    return 0;
}

// Device -> pageable host memory.  The runtime stages such a copy through pinned buffers with a single-threaded memcpy
// (~9 GB/s: 13 ms for the 114 MB graph of a 1 M-point index).  Here: two pinned 32 MB buffers (allocated once per
// process), the DMA of chunk c + 1 in flight while chunk c is copied out of its buffer by four host threads.
static std::mutex g_stage_mu;
// per DEVICE: an event can only be recorded on a stream of the device it was created on (a build on device 1 after one on
// device 0 in the same process), and the pinned buffers are registered with the device that was current at allocation
static char *g_stage_dev[64][2] = {{nullptr, nullptr}};
static hipEvent_t g_stage_ev_dev[64][2] = {{nullptr, nullptr}};
int nnd_d2h_parallel(nnd_ctx *ctx, void *dst, const void *src, size_t bytes, int parts) {
    constexpr size_t STAGE = (size_t)32 << 20;
    if (bytes < (size_t)(4u << 20) || ctx->p.device < 0 || ctx->p.device >= 64) {
        NND_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return 0;
    }
    {   // a pinned destination (nnd_host_alloc: the result arrays of the drop-in class) takes the DMA directly
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, dst) == hipSuccess && at.type == hipMemoryTypeHost) {
            NND_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
            NND_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            return 0;
        }
        (void)hipGetLastError();  // (an ordinary host pointer is "invalid value" to the query)
    }
    std::lock_guard<std::mutex> lk(g_stage_mu);
    char **g_stage = g_stage_dev[ctx->p.device];
    hipEvent_t *g_stage_ev = g_stage_ev_dev[ctx->p.device];
    NND_HIP_CHECK(hipSetDevice(ctx->p.device));
    for (int b = 0; b < 2; b++) {
        if (!g_stage[b]) NND_HIP_CHECK(hipHostMalloc((void **)&g_stage[b], STAGE, hipHostMallocDefault));
        if (!g_stage_ev[b]) NND_HIP_CHECK(hipEventCreateWithFlags(&g_stage_ev[b], hipEventDisableTiming));
    }
    const size_t nchunks = (bytes + STAGE - 1) / STAGE;
    for (size_t c = 0; c <= nchunks; c++) {
        if (c < nchunks) {
            const size_t o = c * STAGE, len = bytes - o < STAGE ? bytes - o : STAGE;
            NND_HIP_CHECK(hipMemcpyAsync(g_stage[c & 1], (const char *)src + o, len, hipMemcpyDeviceToHost, ctx->stream));
            NND_HIP_CHECK(hipEventRecord(g_stage_ev[c & 1], ctx->stream));
        }
        if (c >= 1) {
            const size_t o = (c - 1) * STAGE, len = bytes - o < STAGE ? bytes - o : STAGE;
            NND_HIP_CHECK(hipEventSynchronize(g_stage_ev[(c - 1) & 1]));
            const char *from = g_stage[(c - 1) & 1];
            char *to = (char *)dst + o;
            std::vector<std::thread> th;
            const size_t piece = ((len + parts - 1) / parts + 4095) & ~(size_t)4095;
            for (int t = 1; t < parts; t++) {
                const size_t po = (size_t)t * piece;
                if (po >= len) break;
                const size_t pl = len - po < piece ? len - po : piece;
                th.emplace_back([=] { memcpy(to + po, from + po, pl); });
            }
            memcpy(to, from, len < piece ? len : piece);
            for (auto &t : th) t.join();
        }
    }
    return 0;
}

// ---- host-side helpers of the drop-in class (include/pynnd_amd.h): first-touch-bound array operations over a few threads
template <typename F>
static void host_parallel(size_t bytes, size_t unit, F fn) {  // fn(offset_units, count_units); pieces are multiples of a page
    const size_t total = bytes / unit;
    int parts = bytes >= ((size_t)32 << 20) ? 16 : (bytes >= ((size_t)4 << 20) ? 8 : 1);
    const unsigned hc = std::thread::hardware_concurrency();
    if (hc && (unsigned)parts > hc) parts = (int)hc;
    const size_t per = ((total + parts - 1) / parts + (4096 / unit) - 1) / (4096 / unit) * (4096 / unit);
    std::vector<std::thread> th;
    for (int t = 1; t < parts; t++) {
        const size_t o = (size_t)t * per;
        if (o >= total) break;
        const size_t c = total - o < per ? total - o : per;
        th.emplace_back([=] { fn(o, c); });
    }
    fn(0, total < per ? total : per);
    for (auto &t : th) t.join();
}
// Pinned (page-locked, resident) host memory for result arrays: no first-touch page faults when the graph lands in it, and the
// device-to-host copy is one DMA at the link rate instead of a staged copy.  NULL when there is no device or no memory: the
// caller then uses ordinary memory.
extern "C" void *nnd_host_alloc(int64_t bytes) {
    void *p = nullptr;
    if (bytes <= 0) return nullptr;
    if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
extern "C" int32_t nnd_host_free(void *p) {
    if (p && hipHostFree(p) != hipSuccess) { (void)hipGetLastError(); nnd_set_global_error("nnd_host_free: not a pointer of nnd_host_alloc"); return 1; }
    return 0;
}
extern "C" int32_t nnd_host_copy(void *dst, const void *src, int64_t bytes) {
    if (bytes < 0 || (bytes > 0 && (!dst || !src))) { nnd_set_global_error("nnd_host_copy: bad arguments"); return 1; }
    host_parallel((size_t)bytes, 1, [=](size_t o, size_t c) { memcpy((char *)dst + o, (const char *)src + o, c); });
    return 0;
}
// IEEE square roots, eight per instruction where the host has AVX2 (vsqrtps is correctly rounded: the same bits as sqrtf / numpy.sqrt;
// the scalar loop does not vectorise under the default -fmath-errno)
#if !defined(__HIP_DEVICE_COMPILE__) && (defined(__x86_64__) || defined(_M_X64))
#include <immintrin.h>
__attribute__((target("avx2"))) static void host_sqrt_avx2(float *dst, const float *src, size_t n) {
    size_t i = 0;
    for (; i + 8 <= n; i += 8) _mm256_storeu_ps(dst + i, _mm256_sqrt_ps(_mm256_loadu_ps(src + i)));
    for (; i < n; i++) dst[i] = sqrtf(src[i]);
}
static bool host_has_avx2() { return __builtin_cpu_supports("avx2"); }
#else
static void host_sqrt_avx2(float *dst, const float *src, size_t n) { for (size_t i = 0; i < n; i++) dst[i] = sqrtf(src[i]); }
static bool host_has_avx2() { return false; }
#endif
extern "C" int32_t nnd_host_sqrt_f32(float *dst, const float *src, int64_t count) {
    if (count < 0 || (count > 0 && (!dst || !src))) { nnd_set_global_error("nnd_host_sqrt_f32: bad arguments"); return 1; }
    const bool avx2 = host_has_avx2();
    host_parallel((size_t)count * sizeof(float), sizeof(float), [=](size_t o, size_t c) {
        if (avx2) host_sqrt_avx2(dst + o, src + o, c);
        else
            for (size_t i = o; i < o + c; i++) dst[i] = sqrtf(src[i]);
    });
    return 0;
}
