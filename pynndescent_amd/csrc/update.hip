// update.hip -- what NNDescent.update() and NNDescent.recall() of a device-built index need besides the build itself: the old
// graph invalidated and padded for the warm start (pynndescent_.py:2461-2493), and the hit count of recall().  The rows of the
// grown point set are assembled by devarray.hip (nnd_device_update_rows), next to the conversions they share.  The entries take
// a device ordinal and a stream instead of a handle, like those of devarray.hip, and wait for nothing.
#include <math.h>
#include <stdio.h>

#include "common.h"
#include "state.h"

// ---- the "is updated" lookup: one byte per old point, plain stores (two pairs that name one id store the same byte) ----
__global__ __launch_bounds__(256) void k_mark_updated(const int32_t *__restrict__ ids, int64_t n_upd, int64_t n_old, uint8_t *__restrict__ map) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_upd) return;
    const int64_t id = ids[i];
    if (id >= 0 && id < n_old) map[id] = 1;
}

// ---- the (n_new, k) id / distance pair the warm start reads ----
// An entry survives when its row is an old row that was not updated and it does not point at an updated point; everything else
// -- rows of updated points, stale entries (cleared in place: the host path does not compact either), the fresh rows -- is
// (-1, +inf).  A thread takes four consecutive entries of the flat arrays: one 16-byte load per input where all four lie in the
// old graph, one 16-byte store per output (both arrays start 16-byte aligned; the last, partial group goes element by element).
__global__ __launch_bounds__(256) void k_update_graph(const int32_t *__restrict__ idx, const float *__restrict__ dist, const uint8_t *__restrict__ map,
                                                      int64_t n_old, int64_t n_new, int k, int vec, int32_t *__restrict__ out_idx, float *__restrict__ out_dist) {
    const int64_t old_count = n_old * k, count = n_new * k, groups = (count + 3) / 4;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e0 = g * 4;
        int32_t id[4];
        float ds[4];
        if (vec && e0 + 4 <= old_count) {
            const int4 vi = *(const int4 *)(idx + e0);
            const float4 vd = *(const float4 *)(dist + e0);
            id[0] = vi.x; id[1] = vi.y; id[2] = vi.z; id[3] = vi.w;
            ds[0] = vd.x; ds[1] = vd.y; ds[2] = vd.z; ds[3] = vd.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const bool in = e0 + c < old_count;
                id[c] = in ? idx[e0 + c] : -1;
                ds[c] = in ? dist[e0 + c] : INFINITY;
            }
        }
        int64_t row = e0 / k;  // (one division per group: the row advances where the column wraps)
        int col = (int)(e0 - row * k);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            bool clear = true;
            // two unconditional byte loads and selects instead of nested branches: an entry that points nowhere looks its own row up twice
            if (row < n_old) {
                const bool points = id[c] >= 0 && (int64_t)id[c] < n_old;
                clear = ((unsigned)map[row] | (unsigned)map[points ? (int64_t)id[c] : row]) != 0u;
            }
            id[c] = clear ? -1 : id[c];
            ds[c] = clear ? INFINITY : ds[c];
            if (++col == k) { col = 0; row++; }
        }
        if (vec && e0 + 4 <= count) {
            *(int4 *)(out_idx + e0) = make_int4(id[0], id[1], id[2], id[3]);
            *(float4 *)(out_dist + e0) = make_float4(ds[0], ds[1], ds[2], ds[3]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (e0 + c < count) { out_idx[e0 + c] = id[c]; out_dist[e0 + c] = ds[c]; }
        }
    }
}

// ---- recall(): how many of the true neighbours appear in the graph's rows ----
// One wave per sampled row: the lanes hold the graph's row (width <= 256: up to four entries each), the k <= 256 true ids are
// read one after the other by the whole wave and looked for.  sum(isin(true[i], graph[rows[i]])) of the host path, entry for
// entry; one add per wave.
__global__ __launch_bounds__(256) void k_recall_hits(const int32_t *__restrict__ true_idx, int64_t m, int k, const int32_t *__restrict__ gidx, int64_t n,
                                                     int width, const int32_t *__restrict__ rows, unsigned long long *__restrict__ hits) {
    const int lane = nnd_lane();
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= m) return;
    const int64_t r = rows[i];
    if (r < 0 || r >= n) return;
    int32_t g[4];
#pragma unroll
    for (int c = 0; c < 4; c++) g[c] = lane + 64 * c < width ? gidx[r * width + lane + 64 * c] : INT32_MIN;
    int cnt = 0;
    for (int j = 0; j < k; j++) {
        const int32_t t = true_idx[i * k + j];
        const bool hit = t != INT32_MIN && (g[0] == t || g[1] == t || g[2] == t || g[3] == t);
        cnt += __ballot(hit) != 0 ? 1 : 0;
    }
    if (lane == 0 && cnt) atomicAdd(hits, (unsigned long long)cnt);
}

static thread_local char g_uperr[256] = {0};
static int up_fail(const char *msg) {
    snprintf(g_uperr, sizeof(g_uperr), "%s", msg);
    nnd_set_global_error(g_uperr);
    return 1;
}

extern "C" int32_t nnd_device_update_graph(int32_t device, void *hip_stream, const int32_t *idx_dev, const float *dist_dev, int64_t n_old, int32_t k,
                                           const int32_t *upd_ids_dev, int64_t n_upd, int64_t n_new, uint8_t *map_dev, int32_t *out_idx_dev,
                                           float *out_dist_dev) {
    if (n_old < 0 || n_new < n_old || k < 1 || n_upd < 0) return up_fail("nnd_device_update_graph: bad shape");
    if (n_new == 0) return 0;
    if (!out_idx_dev || !out_dist_dev || (n_old > 0 && (!idx_dev || !dist_dev || !map_dev)) || (n_upd > 0 && !upd_ids_dev))
        return up_fail("nnd_device_update_graph: null pointer");
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return up_fail("nnd_device_update_graph: no such device"); }
    hipStream_t st = (hipStream_t)hip_stream;
    if (n_old > 0 && hipMemsetAsync(map_dev, 0, (size_t)n_old, st) != hipSuccess) { (void)hipGetLastError(); return up_fail("nnd_device_update_graph: memset failed"); }
    if (n_upd > 0 && n_old > 0) hipLaunchKernelGGL(k_mark_updated, dim3((unsigned)((n_upd + 255) / 256)), dim3(256), 0, st, upd_ids_dev, n_upd, n_old, map_dev);
    const int vec = ((((uintptr_t)idx_dev | (uintptr_t)dist_dev | (uintptr_t)out_idx_dev | (uintptr_t)out_dist_dev) & 15) == 0) ? 1 : 0;
    int64_t blocks = ((n_new * k + 3) / 4 + 255) / 256;
    if (blocks > 65536) blocks = 65536;  // (the kernel strides over the rest)
    hipLaunchKernelGGL(k_update_graph, dim3((unsigned)blocks), dim3(256), 0, st, idx_dev, dist_dev, map_dev, n_old, n_new, (int)k, vec, out_idx_dev, out_dist_dev);
    if (hipGetLastError() != hipSuccess) return up_fail("nnd_device_update_graph: kernel launch failed");
    return 0;
}

extern "C" int32_t nnd_device_recall_hits(int32_t device, void *hip_stream, const int32_t *true_idx_dev, int64_t m, int32_t k, const int32_t *graph_idx_dev,
                                          int64_t n, int32_t width, const int32_t *rows_dev, int64_t *hits_dev) {
    if (m < 0 || n < 0 || k < 1 || k > NND_WIDE_K || width < 1 || width > NND_WIDE_K) return up_fail("nnd_device_recall_hits: k and the graph's width must be in 1..256");
    if (!hits_dev || (m > 0 && (!true_idx_dev || !graph_idx_dev || !rows_dev))) return up_fail("nnd_device_recall_hits: null pointer");
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return up_fail("nnd_device_recall_hits: no such device"); }
    hipStream_t st = (hipStream_t)hip_stream;
    if (hipMemsetAsync(hits_dev, 0, sizeof(int64_t), st) != hipSuccess) { (void)hipGetLastError(); return up_fail("nnd_device_recall_hits: memset failed"); }
    if (m == 0) return 0;
    hipLaunchKernelGGL(k_recall_hits, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, st, true_idx_dev, m, (int)k, graph_idx_dev, n, (int)width, rows_dev,
                       (unsigned long long *)hits_dev);
    if (hipGetLastError() != hipSuccess) return up_fail("nnd_device_recall_hits: kernel launch failed");
    return 0;
}
