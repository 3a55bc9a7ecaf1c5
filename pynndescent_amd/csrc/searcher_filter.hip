// searcher_filter.hip -- what restricts a searcher's answers (include/pynnd_amd.h): the allow set of nnd_searcher_set_filter* and
// the rows' tag words of nnd_searcher_set_tags*, with the counts per mask.  The walk reads both in query.hip (k_query's FILT).
#include "searcher.h"

// ---- the filter's allow set (nnd_searcher_set_filter*) ----
// an id list (original numbering) marked into a byte mask; an id outside 0 .. n - 1 raises the flag and is never written
__global__ void k_filter_mark_ids(const int64_t *__restrict__ ids, int64_t m, int64_t n, uint8_t *__restrict__ mask,
                                  unsigned long long *__restrict__ fstat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t id = ids[i];
    if (id < 0 || id >= n) {
        atomicOr(&fstat[1], 1ull);
        return;
    }
    mask[id] = 1;
}
// the bitset over the searcher's numbering: bit i = mask[order[i]] != 0 (order nullptr: the identity), 64 rows of a wave packed by
// one ballot into two words; fstat[0] counts the allowed rows.  A wave's first row is a multiple of 64, so no two waves share a word.
__global__ __launch_bounds__(256) void k_filter_bitset(const uint8_t *__restrict__ mask, const int32_t *__restrict__ order, int64_t n,
                                                       uint32_t *__restrict__ bits, unsigned long long *__restrict__ fstat) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    if (i < n) {
        const int64_t r = order ? (int64_t)order[i] : i;
        on = r >= 0 && r < n && mask[r] != 0;
    }
    const unsigned long long m = __ballot(on);
    if (nnd_lane() == 0 && i < n) {
        bits[i >> 5] = (uint32_t)m;
        if (i + 32 < n) bits[(i >> 5) + 1] = (uint32_t)(m >> 32);
        if (m) atomicAdd(&fstat[0], (unsigned long long)__popcll(m));
    }
}

// ---- per-query filters: the rows' tag words (nnd_searcher_set_tags*) ----
// the tag words in the searcher's numbering: out[i] = tags[order[i]] (order nullptr: the identity); the sibling of k_filter_bitset
__global__ __launch_bounds__(256) void k_tags_gather(const uint64_t *__restrict__ tags, const int32_t *__restrict__ order, int64_t n,
                                                     uint64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t r = order ? (int64_t)order[i] : i;
    out[i] = r >= 0 && r < n ? tags[r] : 0ull;
}
// counts[u] += rows whose tag word meets masks[u], u < n_masks: one pass over the tag words.  A workgroup keeps Q_COUNT_ROWS rows
// per thread in registers and takes the masks (wave-uniform loads) in groups of Q_COUNT_MASKS: a wave reduction per mask, the four
// waves' sums meet in LDS, and one global atomic per workgroup and mask adds what is not zero.
#define Q_COUNT_ROWS 8
#define Q_COUNT_MASKS 1024
__global__ __launch_bounds__(256) void k_tags_count(const uint64_t *__restrict__ tags, int64_t n, const uint64_t *__restrict__ masks, int n_masks,
                                                    unsigned long long *__restrict__ counts) {
    __shared__ int part[Q_COUNT_MASKS];
    const int lane = nnd_lane();
    uint64_t t[Q_COUNT_ROWS];
    const int64_t base = (int64_t)blockIdx.x * (256 * Q_COUNT_ROWS) + threadIdx.x;
#pragma unroll
    for (int j = 0; j < Q_COUNT_ROWS; j++) {
        const int64_t i = base + 256 * j;
        t[j] = i < n ? tags[i] : 0ull;
    }
    for (int u0 = 0; u0 < n_masks; u0 += Q_COUNT_MASKS) {
        const int nu = n_masks - u0 < Q_COUNT_MASKS ? n_masks - u0 : Q_COUNT_MASKS;
        for (int u = threadIdx.x; u < nu; u += 256) part[u] = 0;
        __syncthreads();
        for (int u = 0; u < nu; u++) {
            const uint64_t m = masks[u0 + u];
            int c = 0;
#pragma unroll
            for (int j = 0; j < Q_COUNT_ROWS; j++) c += (t[j] & m) != 0ull ? 1 : 0;
            c = nnd_wave_sum_i32(c);
            if (lane == 0 && c) atomicAdd(&part[u], c);
        }
        __syncthreads();
        for (int u = threadIdx.x; u < nu; u += 256)
            if (part[u]) atomicAdd(&counts[u0 + u], (unsigned long long)part[u]);
        __syncthreads();
    }
}

// ---- the filter (include/pynnd_amd.h): the allow bitset, built on `st` from a mask or an id list in device memory ----
static int searcher_build_filter(nnd_searcher_s *s, const char *who, const void *filter_dev, int64_t count, int32_t kind, const int32_t *order_dev,
                                 hipStream_t st, nnd_scratch &tmp, int64_t *n_allowed) {
    s->filter_on = false;  // a failed call leaves the searcher unfiltered
    if (!s->allow) S_ALLOC(&s->allow, (size_t)((s->n + 31) / 32));
    if (!s->fstat) S_ALLOC(&s->fstat, 2);
    S_HIP(hipMemsetAsync(s->fstat, 0, 2 * sizeof(unsigned long long), st));
    const uint8_t *mask = (const uint8_t *)filter_dev;
    if (kind == NND_FILTER_IDS) {
        uint8_t *marked = tmp.get<uint8_t>(s, (size_t)s->n);
        if (!marked) return 1;
        S_HIP(hipMemsetAsync(marked, 0, (size_t)s->n, st));
        if (count > 0)
            hipLaunchKernelGGL(k_filter_mark_ids, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const int64_t *)filter_dev, count, s->n, marked,
                               s->fstat);
        mask = marked;
    }
    hipLaunchKernelGGL(k_filter_bitset, dim3((unsigned)((s->n + 255) / 256)), dim3(256), 0, st, mask, order_dev, s->n, s->allow, s->fstat);
    S_HIP(hipGetLastError());
    unsigned long long stat[2] = {0, 0};
    S_HIP(hipMemcpyAsync(stat, s->fstat, sizeof(stat), hipMemcpyDeviceToHost, st));
    S_HIP(hipStreamSynchronize(st));
    if (stat[1]) {
        s->set_error("%s: an id of the filter is outside 0 .. %lld", who, (long long)(s->n - 1));
        return 2;
    }
    if (n_allowed) *n_allowed = (int64_t)stat[0];
    s->filter_on = true;
    return 0;
}
static int filter_args(nnd_searcher_s *s, const char *who, const void *filter, int64_t count, int32_t kind) {
    if (kind != NND_FILTER_MASK && kind != NND_FILTER_IDS) { s->set_error("%s: kind must be NND_FILTER_MASK or NND_FILTER_IDS (got %d)", who, kind); return 1; }
    if (count < 0 || (count > 0 && !filter)) { s->set_error("%s: filter missing", who); return 1; }
    if (kind == NND_FILTER_MASK && count != s->n) { s->set_error("%s: a mask has one byte per row (%lld), got %lld", who, (long long)s->n, (long long)count); return 1; }
    if (count >= ((int64_t)1 << 40)) { s->set_error("%s: too many ids", who); return 1; }
    return 0;
}
extern "C" int32_t nnd_searcher_set_filter(nnd_searcher_t s, const void *filter, int64_t count, int32_t kind, const int32_t *order, int64_t *n_allowed) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_set_filter: null searcher"); return 1; }
    if (filter_args(s, "nnd_searcher_set_filter", filter, count, kind)) return 1;
    S_HIP(hipSetDevice(s->device));
    nnd_scratch tmp;  // released on return, behind the synchronise of searcher_build_filter
    const size_t bytes = (size_t)count * (kind == NND_FILTER_IDS ? sizeof(int64_t) : 1);
    unsigned char *dfilter = tmp.get<unsigned char>(s, bytes);
    int32_t *dorder = order ? tmp.get<int32_t>(s, (size_t)s->n) : nullptr;
    if (!dfilter || (order && !dorder)) return 1;
    if (bytes) S_HIP(hipMemcpyAsync(dfilter, filter, bytes, hipMemcpyHostToDevice, s->stream));
    if (order) S_HIP(hipMemcpyAsync(dorder, order, sizeof(int32_t) * (size_t)s->n, hipMemcpyHostToDevice, s->stream));
    const int rc = searcher_build_filter(s, "nnd_searcher_set_filter", dfilter, count, kind, dorder, s->stream, tmp, n_allowed);
    if (rc) (void)hipStreamSynchronize(s->stream);  // nothing queued still reads tmp
    return rc;
}
extern "C" int32_t nnd_searcher_set_filter_device(nnd_searcher_t s, const void *filter_dev, int64_t count, int32_t kind, const int32_t *order_dev,
                                                  int64_t *n_allowed, void *hip_stream) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_set_filter_device: null searcher"); return 1; }
    if (filter_args(s, "nnd_searcher_set_filter_device", filter_dev, count, kind)) return 1;
    S_HIP(hipSetDevice(s->device));
    nnd_scratch tmp;
    const int rc = searcher_build_filter(s, "nnd_searcher_set_filter_device", filter_dev, count, kind, order_dev, (hipStream_t)hip_stream, tmp, n_allowed);
    if (rc) (void)hipStreamSynchronize((hipStream_t)hip_stream);
    return rc;
}
extern "C" int32_t nnd_searcher_clear_filter(nnd_searcher_t s) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_clear_filter: null searcher"); return 1; }
    s->filter_on = false;  // the bitset stays allocated for the next filter
    return 0;
}

// ---- per-query filters (include/pynnd_amd.h): the tag words, the counts per mask, the tagged query ----
static int searcher_gather_tags(nnd_searcher_s *s, const uint64_t *tags_dev, const int32_t *order_dev, hipStream_t st) {
    if (!s->tags) S_ALLOC(&s->tags, (size_t)s->n);
    hipLaunchKernelGGL(k_tags_gather, dim3((unsigned)((s->n + 255) / 256)), dim3(256), 0, st, tags_dev, order_dev, s->n, s->tags);
    S_HIP(hipGetLastError());
    S_HIP(hipStreamSynchronize(st));
    return 0;
}
extern "C" int32_t nnd_searcher_clear_tags(nnd_searcher_t s) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_clear_tags: null searcher"); return 1; }
    S_HIP(hipSetDevice(s->device));
    S_HIP(hipStreamSynchronize(s->stream));
    s->mem.free(&s->tags);
    return 0;
}
extern "C" int32_t nnd_searcher_set_tags(nnd_searcher_t s, const uint64_t *tags, const int32_t *order) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_set_tags: null searcher"); return 1; }
    if (!tags) { s->set_error("nnd_searcher_set_tags: tags missing"); return 1; }
    S_HIP(hipSetDevice(s->device));
    nnd_scratch tmp;  // released on return, behind the synchronise of searcher_gather_tags
    uint64_t *dtags = tmp.get<uint64_t>(s, (size_t)s->n);
    int32_t *dorder = order ? tmp.get<int32_t>(s, (size_t)s->n) : nullptr;
    if (!dtags || (order && !dorder)) return 1;
    S_HIP(hipMemcpyAsync(dtags, tags, sizeof(uint64_t) * (size_t)s->n, hipMemcpyHostToDevice, s->stream));
    if (order) S_HIP(hipMemcpyAsync(dorder, order, sizeof(int32_t) * (size_t)s->n, hipMemcpyHostToDevice, s->stream));
    const int rc = searcher_gather_tags(s, dtags, dorder, s->stream);
    if (rc) (void)hipStreamSynchronize(s->stream);
    return rc;
}
extern "C" int32_t nnd_searcher_set_tags_device(nnd_searcher_t s, const uint64_t *tags_dev, const int32_t *order_dev, void *hip_stream) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_set_tags_device: null searcher"); return 1; }
    if (!tags_dev) { s->set_error("nnd_searcher_set_tags_device: tags missing"); return 1; }
    S_HIP(hipSetDevice(s->device));
    return searcher_gather_tags(s, tags_dev, order_dev, (hipStream_t)hip_stream);
}
static int searcher_count_tags(nnd_searcher_s *s, const uint64_t *masks_dev, int32_t n_masks, unsigned long long *counts_dev, hipStream_t st) {
    S_HIP(hipMemsetAsync(counts_dev, 0, sizeof(unsigned long long) * (size_t)n_masks, st));
    const int64_t per_block = 256 * Q_COUNT_ROWS;
    hipLaunchKernelGGL(k_tags_count, dim3((unsigned)((s->n + per_block - 1) / per_block)), dim3(256), 0, st, (const uint64_t *)s->tags, s->n, masks_dev, (int)n_masks,
                       counts_dev);
    S_HIP(hipGetLastError());
    return 0;
}
static int count_args(nnd_searcher_s *s, const char *who, const void *masks, int32_t n_masks, const void *counts) {
    if (!s->tags) { s->set_error("%s: the searcher has no tags (nnd_searcher_set_tags first)", who); return 1; }
    if (n_masks < 0 || (n_masks > 0 && (!masks || !counts))) { s->set_error("%s: masks or counts missing", who); return 1; }
    return 0;
}
extern "C" int32_t nnd_searcher_count_tags(nnd_searcher_t s, const uint64_t *masks, int32_t n_masks, int64_t *counts) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_count_tags: null searcher"); return 1; }
    if (count_args(s, "nnd_searcher_count_tags", masks, n_masks, counts)) return 1;
    if (n_masks == 0) return 0;
    S_HIP(hipSetDevice(s->device));
    nnd_scratch tmp;
    uint64_t *dm = tmp.get<uint64_t>(s, (size_t)n_masks);
    unsigned long long *dc = tmp.get<unsigned long long>(s, (size_t)n_masks);
    if (!dm || !dc) return 1;
    int rc = 0;
    if (hipMemcpyAsync(dm, masks, sizeof(uint64_t) * (size_t)n_masks, hipMemcpyHostToDevice, s->stream) != hipSuccess) { s->set_error("nnd_searcher_count_tags: H2D of the masks failed"); rc = 1; }
    if (!rc) rc = searcher_count_tags(s, dm, n_masks, dc, s->stream);
    if (!rc && hipMemcpyAsync(counts, dc, sizeof(int64_t) * (size_t)n_masks, hipMemcpyDeviceToHost, s->stream) != hipSuccess) { s->set_error("nnd_searcher_count_tags: D2H of the counts failed"); rc = 1; }
    if (hipStreamSynchronize(s->stream) != hipSuccess && !rc) { s->set_error("nnd_searcher_count_tags: kernel failed: %s", hipGetErrorString(hipGetLastError())); rc = 1; }
    return rc;
}
extern "C" int32_t nnd_searcher_count_tags_device(nnd_searcher_t s, const uint64_t *masks_dev, int32_t n_masks, int64_t *counts_dev, void *hip_stream) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_count_tags_device: null searcher"); return 1; }
    if (count_args(s, "nnd_searcher_count_tags_device", masks_dev, n_masks, counts_dev)) return 1;
    if (n_masks == 0) return 0;
    S_HIP(hipSetDevice(s->device));
    if (searcher_count_tags(s, masks_dev, n_masks, (unsigned long long *)counts_dev, (hipStream_t)hip_stream)) return 1;
    S_HIP(hipStreamSynchronize((hipStream_t)hip_stream));
    return 0;
}
