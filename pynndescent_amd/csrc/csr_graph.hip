// csr_graph.hip -- k-lists to canonical CSR on the device: what scipy's coo.tocsr() + sum_duplicates() (and, for the symmetric
// form, an explicit min-union of A and A^T) make of an (m, k) pair of neighbour ids and values.  Columns strictly ascending in
// every row, no -1; indptr int64 (m + 1), indices int32, data float32.  DESIGN.md section 4 "Graph export".
//
//   directed    k_csr_count_rows  -> rocprim::exclusive_scan -> k_csr_write_rows<KU, W, IdT>  (two launches: count, then write)
//   symmetric   k_csr_sym_count   -> scan -> k_csr_sym_scatter -> k_csr_sym_merge (+ k_csr_sym_merge_long) -> scan -> k_csr_copy_rows
//
// A row is sorted as 64-bit keys (column << 32 | value bits) by one wave: a bitonic network over 64, 128 or 256 keys, one,
// two or four per lane (the KU of query.hip's k_query; the symmetric merge also eight, 512 keys), partners at distance < 64 through a
// lane exchange, the others inside the lane.
// An empty place is the all-ones key and sorts to the end.  A row of at most 16 or 32 places needs the network's first stages
// only (W = 16 or 32 lanes: 10 or 15 exchanges where 64 lanes take 21), and the directed form then gives every W lanes of the
// wave a row of their own.  The staging stretch of a row of the symmetric form holds its k places (no atomic, no count: an
// empty place is staged as the empty key) followed by its reverse edges; a stretch of more than 512 keys (a hub) is sorted
// by one workgroup where it lies (k_csr_sym_merge_long), and the call reports how many rows went that way.
//
// Determinism: the reverse edges reach a row's stretch in the order the atomic cursors hand out, which differs between runs;
// the sort by (column, value bits) that follows does not see that order, and where a column appears twice (the edge and its
// reverse) the entry keeps the smaller of the two floats.  Counts come from integer additions, which commute.
// No atomic here is anything but an integer add, nothing spins, and every store is a vector store.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "../../include/pynnd_amd.h"
#include "common.h"
#include "devmem.h"
#include "state.h"

#define CSR_REG_CAP 256    // the widest k-list
#define CSR_UNION_CAP 512  // staged keys of a row (its k places and its reverse edges) one wave sorts in registers; more: k_csr_sym_merge_long
#define CSR_EMPTY 0xFFFFFFFFFFFFFFFFull

// the column of a place: its id when that names a column (and is not the dropped diagonal), else -1
template <typename IdT>
__device__ __forceinline__ int32_t csr_col(const IdT *__restrict__ ids, int64_t at, int64_t n, int64_t row, int drop_self) {
    const int64_t j = (int64_t)ids[at];
    return (j >= 0 && j < n && !(drop_self && j == row)) ? (int32_t)j : -1;
}
__device__ __forceinline__ uint64_t csr_key(int32_t col, float v) { return ((uint64_t)(uint32_t)col << 32) | (uint64_t)__float_as_uint(v); }
__device__ __forceinline__ uint32_t csr_key_col(uint64_t key) { return (uint32_t)(key >> 32); }
__device__ __forceinline__ float csr_key_val(uint64_t key) { return __uint_as_float((uint32_t)key); }
__device__ __forceinline__ uint64_t csr_shfl64(uint64_t v, int src) {
    return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64) << 32) | (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, src, 64);
}

// Ascending bitonic sort of the 64 * KU keys of a wave; key[u] of lane l is element u * 64 + l.  Every lane takes part.
// W < 64 (KU == 1): every aligned group of W lanes sorts its own W keys.
template <int KU, int W>
__device__ __forceinline__ void csr_wave_sort(uint64_t (&key)[KU]) {
    static_assert(W == 64 || KU == 1, "several keys per lane: the whole wave is one row");
    const int lane = nnd_lane() & (W - 1);
#pragma unroll
    for (int size = 2; size <= W * KU; size <<= 1) {
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride >= 64) {  // both elements in this lane
                const int du = stride >> 6;
#pragma unroll
                for (int u = 0; u < KU; u++) {
                    if (u & du) continue;
                    const bool asc = (((u * 64) & size) == 0);  // (size >= 128 here: the bit is one of u's)
                    const uint64_t a = key[u], b = key[u | du];
                    const bool swap = (a > b) == asc;
                    key[u] = swap ? b : a;
                    key[u | du] = swap ? a : b;
                }
            } else {
#pragma unroll
                for (int u = 0; u < KU; u++) {
                    const uint64_t other = csr_shfl64(key[u], nnd_lane() ^ stride);  // (stride < W: a lane of the same group)
                    const bool asc = (((u * 64 + lane) & size) == 0);
                    const bool lower = (lane & stride) == 0;
                    const uint64_t lo = key[u] < other ? key[u] : other, hi = key[u] < other ? other : key[u];
                    key[u] = (lower == asc) ? lo : hi;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- directed form
// cnt[row] = places of the row that hold a column.  One thread per row: the pass reads the ids alone, and a thread's k ids are
// one or a few cache lines that its neighbours' rows continue.
template <typename IdT>
__global__ __launch_bounds__(256) void k_csr_count_rows(const IdT *__restrict__ ids, int64_t m, int32_t k, int64_t ld, int64_t n, int drop_self,
                                                        unsigned long long *__restrict__ cnt) {
    for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < m; row += (int64_t)gridDim.x * blockDim.x) {
        int c = 0;
        for (int e = 0; e < k; e++) c += csr_col(ids, row * ld + e, n, row, drop_self) >= 0 ? 1 : 0;
        cnt[row] = (unsigned long long)c;
    }
}
// one wave per row -- W < 64: one row per W lanes -- : load, drop the empty places, sort by column, write at indptr[row]
template <int KU, int W, typename IdT>
__global__ __launch_bounds__(256) void k_csr_write_rows(const IdT *__restrict__ ids, const float *__restrict__ vals, int64_t m, int32_t k, int64_t ld,
                                                        int64_t n, int drop_self, int connectivity, const int64_t *__restrict__ indptr,
                                                        int32_t *__restrict__ indices, float *__restrict__ data) {
    constexpr int R = 64 / W;  // rows of a wave
    const int sub = nnd_lane() & (W - 1), group = nnd_lane() / W;
    for (int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R; first < m; first += (int64_t)gridDim.x * 4 * R) {  // wave-uniform
        const int64_t row = first + group;
        const bool live = row < m;
        uint64_t key[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int e = u * 64 + sub;
            key[u] = CSR_EMPTY;
            if (live && e < k) {
                const int32_t col = csr_col(ids, row * ld + e, n, row, drop_self);
                if (col >= 0) key[u] = csr_key(col, vals[row * ld + e]);
            }
        }
        csr_wave_sort<KU, W>(key);
        const int64_t at = live ? indptr[row] : 0;
#pragma unroll
        for (int u = 0; u < KU; u++) {
            if (key[u] != CSR_EMPTY) {  // the filled keys are the first ones: element e lands at place e
                indices[at + u * 64 + sub] = (int32_t)csr_key_col(key[u]);
                data[at + u * 64 + sub] = connectivity ? 1.0f : csr_key_val(key[u]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- symmetric form (m == n)
// The staging stretch of row i: its k places, then its reverse edges.  roff = the exclusive sums of the reverse counts.
__device__ __forceinline__ int64_t csr_stretch(const int64_t *__restrict__ roff, int64_t row, int32_t k, int64_t *len) {
    const int64_t a = roff[row];
    *len = (int64_t)k + (roff[row + 1] - a);
    return a + row * (int64_t)k;
}
// cnt[j] += 1 for the reverse of every edge (i, j), i != j (the diagonal is its own reverse)
template <typename IdT>
__global__ __launch_bounds__(256) void k_csr_sym_count(const IdT *__restrict__ ids, int64_t n, int32_t k, int64_t ld, int drop_self,
                                                       unsigned long long *__restrict__ cnt) {
    const int64_t total = n * (int64_t)k;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / k;
        const int32_t col = csr_col(ids, row * ld + (t - row * k), n, row, drop_self);
        if (col >= 0 && (int64_t)col != row) atomicAdd(&cnt[col], 1ull);
    }
}
// every place into its own slot of its row's stretch (an empty place as the empty key), and the reverse of every edge behind the
// k places of the other row, at the place that row's cursor hands out (any order: the merge sorts)
template <typename IdT>
__global__ __launch_bounds__(256) void k_csr_sym_scatter(const IdT *__restrict__ ids, const float *__restrict__ vals, int64_t n, int32_t k, int64_t ld,
                                                         int drop_self, const int64_t *__restrict__ roff, unsigned int *__restrict__ cursor,
                                                         uint64_t *__restrict__ stage) {
    const int64_t total = n * (int64_t)k;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / k, e = t - row * k, at = row * ld + e;
        const int32_t col = csr_col(ids, at, n, row, drop_self);
        const float v = col >= 0 ? vals[at] : 0.0f;
        stage[roff[row] + t] = col >= 0 ? csr_key(col, v) : CSR_EMPTY;  // (roff[row] + row * k + e)
        if (col >= 0 && (int64_t)col != row) {
            int64_t len;
            const int64_t a = csr_stretch(roff, col, k, &len);
            const int64_t q = (int64_t)k + (int64_t)atomicAdd(&cursor[col], 1u);
            if (q < len) stage[a + q] = csr_key((int32_t)row, v);  // (always: the counts were made by the same rule)
        }
    }
}
// the smaller float of an entry and its twin (the same column once more, right behind it after the sort)
__device__ __forceinline__ uint64_t csr_min_with_twin(uint64_t key, uint64_t next) {
    if (next != CSR_EMPTY && csr_key_col(next) == csr_key_col(key)) {
        const float a = csr_key_val(key), b = csr_key_val(next);
        return csr_key((int32_t)csr_key_col(key), b < a ? b : a);
    }
    return key;
}
// one stretch of at most W * KU staged keys: sort, collapse equal columns with min, write back packed; returns the entries left
template <int KU, int W>
__device__ __forceinline__ int csr_union_row(uint64_t *seg, int len) {
    const int lane = nnd_lane();
    uint64_t key[KU];
#pragma unroll
    for (int u = 0; u < KU; u++) key[u] = (u * 64 + lane < len) ? seg[u * 64 + lane] : CSR_EMPTY;
    csr_wave_sort<KU, W>(key);  // (W < 64: the lanes from W on hold empty keys, and stay so)
    int base = 0;
#pragma unroll
    for (int u = 0; u < KU; u++) {
        const uint64_t before_in = csr_shfl64(key[u], (lane + 63) & 63), after_in = csr_shfl64(key[u], (lane + 1) & 63);
        const uint64_t before_out = u > 0 ? csr_shfl64(key[u - 1], 63) : CSR_EMPTY;
        const uint64_t after_out = u < KU - 1 ? csr_shfl64(key[u + 1], 0) : CSR_EMPTY;
        const uint64_t before = lane == 0 ? before_out : before_in, after = lane == 63 ? after_out : after_in;
        const bool first = (u == 0 && lane == 0);
        const bool keep = key[u] != CSR_EMPTY && (first || csr_key_col(before) != csr_key_col(key[u]));
        const unsigned long long mask = __ballot(keep);
        if (keep) seg[base + nnd_prefix_popc(mask)] = csr_min_with_twin(key[u], after);  // (every key is in registers by now)
        base += __popcll(mask);
    }
    return base;
}
// one wave per row; a stretch of more than CSR_UNION_CAP staged keys is put on the list of k_csr_sym_merge_long
__global__ __launch_bounds__(256) void k_csr_sym_merge(int64_t n, int32_t k, const int64_t *__restrict__ roff, uint64_t *stage,
                                                       unsigned long long *__restrict__ ucnt, int32_t *__restrict__ long_rows,
                                                       unsigned int *__restrict__ n_long) {
    const int lane = nnd_lane();
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (int64_t)gridDim.x * 4) {  // wave-uniform
        int64_t len;
        const int64_t a = csr_stretch(roff, row, k, &len);
        if (len > CSR_UNION_CAP) {
            if (lane == 0) long_rows[atomicAdd(n_long, 1u)] = (int32_t)row;
            continue;
        }
        int left;
        if (len <= 16) left = csr_union_row<1, 16>(stage + a, (int)len);
        else if (len <= 32) left = csr_union_row<1, 32>(stage + a, (int)len);
        else if (len <= 64) left = csr_union_row<1, 64>(stage + a, (int)len);
        else if (len <= 128) left = csr_union_row<2, 64>(stage + a, (int)len);
        else if (len <= 256) left = csr_union_row<4, 64>(stage + a, (int)len);
        else left = csr_union_row<8, 64>(stage + a, (int)len);
        if (lane == 0) ucnt[row] = (unsigned long long)left;
    }
}
// A long row, one workgroup at a time, where it lies: a bitonic network whose every comparison puts the smaller key at the
// lower index (the first step of a merge mirrors the upper half), so the places past the row's end, which would hold +inf,
// never take part; then the collapse of equal columns, 256 keys at a time from the front (what a piece writes lies at or in
// front of what it read, and the column of the key in front of a piece is carried over in LDS).
__global__ __launch_bounds__(256) void k_csr_sym_merge_long(int32_t k, const int64_t *__restrict__ roff, uint64_t *stage,
                                                            unsigned long long *__restrict__ ucnt, const int32_t *__restrict__ long_rows,
                                                            const unsigned int *__restrict__ n_long) {
    __shared__ int s_wave[4];
    __shared__ uint32_t s_last_col;
    const int tid = threadIdx.x, lane = nnd_lane(), w = tid >> 6;
    const unsigned int rows = *n_long;
    for (unsigned int r = blockIdx.x; r < rows; r += gridDim.x) {  // block-uniform
        const int64_t row = long_rows[r];
        int64_t len;
        uint64_t *seg = stage + csr_stretch(roff, row, k, &len);
        int64_t pow2 = 1;
        while (pow2 < len) pow2 <<= 1;
        const int64_t pairs = pow2 >> 1;
        for (int64_t size = 2; size <= pow2; size <<= 1) {
            const int64_t half = size >> 1;
            for (int64_t p = tid; p < pairs; p += 256) {  // mirror step
                const int64_t lo = (p / half) * size + (p % half), hi = (p / half) * size + size - 1 - (p % half);
                if (hi < len) {
                    const uint64_t x = seg[lo], y = seg[hi];
                    if (x > y) { seg[lo] = y; seg[hi] = x; }
                }
            }
            __syncthreads();
            for (int64_t stride = half >> 1; stride > 0; stride >>= 1) {
                for (int64_t p = tid; p < pairs; p += 256) {
                    const int64_t lo = (p / stride) * 2 * stride + (p % stride), hi = lo + stride;
                    if (hi < len) {
                        const uint64_t x = seg[lo], y = seg[hi];
                        if (x > y) { seg[lo] = y; seg[hi] = x; }
                    }
                }
                __syncthreads();
            }
        }
        int64_t written = 0;
        for (int64_t c0 = 0; c0 < len; c0 += 256) {
            const int64_t e = c0 + tid;
            const uint64_t key = e < len ? seg[e] : CSR_EMPTY;
            const uint64_t after = e + 1 < len ? seg[e + 1] : CSR_EMPTY;
            const uint32_t before_col = tid > 0 ? csr_key_col(e - 1 < len ? seg[e - 1] : CSR_EMPTY) : (c0 > 0 ? s_last_col : 0xFFFFFFFFu);
            __syncthreads();  // every read of the piece is done (and s_last_col read) before anything is written
            const bool keep = key != CSR_EMPTY && csr_key_col(key) != before_col;
            const unsigned long long mask = __ballot(keep);
            if (lane == 0) s_wave[w] = __popcll(mask);
            if (tid == 255) s_last_col = csr_key_col(key);  // (only read when another piece follows: then e < len)
            __syncthreads();
            int pos = nnd_prefix_popc(mask), all = 0;
            for (int i = 0; i < 4; i++) { pos += i < w ? s_wave[i] : 0; all += s_wave[i]; }
            if (keep) seg[written + pos] = csr_min_with_twin(key, after);
            written += all;
            __syncthreads();
        }
        if (tid == 0) ucnt[row] = (unsigned long long)written;
        __syncthreads();
    }
}
// the packed rows out of the staging buffer: G lanes per row (a power of two, at most 64)
__global__ __launch_bounds__(256) void k_csr_copy_rows(int64_t n, int32_t k, int G, const int64_t *__restrict__ roff, const uint64_t *__restrict__ stage,
                                                       int connectivity, const int64_t *__restrict__ indptr, int32_t *__restrict__ indices,
                                                       float *__restrict__ data) {
    const int sub = threadIdx.x & (G - 1);
    const int64_t per_pass = (int64_t)gridDim.x * (256 / G);
    for (int64_t row = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; row < n; row += per_pass) {
        const int64_t from = roff[row] + row * (int64_t)k, to = indptr[row], len = indptr[row + 1] - to;
        for (int64_t e = sub; e < len; e += G) {
            const uint64_t key = stage[from + e];
            indices[to + e] = (int32_t)csr_key_col(key);
            data[to + e] = connectivity ? 1.0f : csr_key_val(key);
        }
    }
}

// ---------------------------------------------------------------------------------------------- host side
struct nnd_csr_s {
    nnd_devmem mem;  // one block: the three arrays below are pieces of it
    int device = 0;
    int64_t m = 0, nnz = 0, long_rows = 0;
    int64_t *indptr = nullptr;
    int32_t *indices = nullptr;
    float *data = nullptr;
};

namespace {
struct csr_err {  // the error sink of an entry without a handle: what nnd_last_global_error returns
    char msg[256];
    void set_error(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        nnd_set_global_error(msg);
    }
};
unsigned csr_grid(int64_t items, int per_block, int64_t cap) {
    const int64_t b = (items + per_block - 1) / per_block;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}
#define CSR_HIP(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) {                                                                             \
            (void)hipGetLastError();                                                                        \
            err.set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);       \
            return 1;                                                                                       \
        }                                                                                                   \
    } while (0)

// Device allocations are the expensive part of a call at this size (a hipMalloc or hipFree costs about what the directed
// form's kernels cost together), so a call makes few: one block for all its small scratch arrays, one for the staging buffer
// of the symmetric form, one for the result.  A block is carved into 256-byte aligned pieces.
size_t csr_room(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
struct csr_carve {
    unsigned char *base = nullptr;
    size_t at = 0;
    template <typename T>
    T *take(size_t count) {
        T *p = (T *)(base + at);
        at += csr_room(sizeof(T) * (count ? count : 1));
        return p;
    }
};
size_t csr_scan_bytes(int64_t rows) {  // rocprim's temporary storage for the scan of rows + 1 counts (0: the query failed)
    size_t bytes = 0;
    if (rocprim::exclusive_scan(nullptr, bytes, (const int64_t *)nullptr, (int64_t *)nullptr, (int64_t)0, (size_t)(rows + 1), rocprim::plus<int64_t>(),
                                (hipStream_t) nullptr) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return bytes + 256;
}
// counts (rows + 1, the last one 0) -> their exclusive sums, and the total on the host (the stream is drained for it)
int csr_scan(csr_err &err, void *scan_tmp, size_t scan_bytes, hipStream_t st, const unsigned long long *cnt, int64_t *sums, int64_t rows,
             int64_t *total) {
    CSR_HIP(rocprim::exclusive_scan(scan_tmp, scan_bytes, (const int64_t *)cnt, sums, (int64_t)0, (size_t)(rows + 1), rocprim::plus<int64_t>(), st));
    CSR_HIP(hipMemcpyAsync(total, sums + rows, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    CSR_HIP(hipStreamSynchronize(st));
    return 0;
}
// the result's one block: indptr (a copy of the scan's sums), indices, data
int csr_result(csr_err &err, hipStream_t st, nnd_csr_s *g, const int64_t *sums, int64_t m) {
    unsigned char *block = nullptr;
    const size_t bytes = csr_room(sizeof(int64_t) * (size_t)(m + 1)) + csr_room(sizeof(int32_t) * (size_t)(g->nnz ? g->nnz : 1)) +
                         csr_room(sizeof(float) * (size_t)(g->nnz ? g->nnz : 1));
    if (!g->mem.alloc(&block, bytes)) { err.set_error("nnd_graph_csr: no device memory for %lld entries (%zu bytes)", (long long)g->nnz, bytes); return 1; }
    csr_carve c{block};
    g->indptr = c.take<int64_t>((size_t)m + 1);
    g->indices = c.take<int32_t>((size_t)g->nnz);
    g->data = c.take<float>((size_t)g->nnz);
    CSR_HIP(hipMemcpyAsync(g->indptr, sums, sizeof(int64_t) * (size_t)(m + 1), hipMemcpyDeviceToDevice, st));
    return 0;
}

template <typename IdT>
void launch_write_rows(hipStream_t st, const IdT *ids, const float *vals, int64_t m, int32_t k, int64_t ld, int64_t n, int drop_self, int conn,
                       const int64_t *indptr, int32_t *indices, float *data) {
    const int rows_per_block = k <= 16 ? 16 : (k <= 32 ? 8 : 4);
    const dim3 grid(csr_grid(m, rows_per_block, 1 << 20)), block(256);
    if (k <= 16) hipLaunchKernelGGL((k_csr_write_rows<1, 16, IdT>), grid, block, 0, st, ids, vals, m, k, ld, n, drop_self, conn, indptr, indices, data);
    else if (k <= 32) hipLaunchKernelGGL((k_csr_write_rows<1, 32, IdT>), grid, block, 0, st, ids, vals, m, k, ld, n, drop_self, conn, indptr, indices, data);
    else if (k <= 64) hipLaunchKernelGGL((k_csr_write_rows<1, 64, IdT>), grid, block, 0, st, ids, vals, m, k, ld, n, drop_self, conn, indptr, indices, data);
    else if (k <= 128) hipLaunchKernelGGL((k_csr_write_rows<2, 64, IdT>), grid, block, 0, st, ids, vals, m, k, ld, n, drop_self, conn, indptr, indices, data);
    else hipLaunchKernelGGL((k_csr_write_rows<4, 64, IdT>), grid, block, 0, st, ids, vals, m, k, ld, n, drop_self, conn, indptr, indices, data);
}

// the kernels of one export on `st`; the result's arrays are allocated in g->mem, the scratch in tmp.  The stream is drained
// at the two places where a total has to reach the host; the caller drains it once more before the scratch goes.
template <typename IdT>
int csr_build(csr_err &err, nnd_scratch &tmp, hipStream_t st, nnd_csr_s *g, const IdT *ids, const float *vals, int64_t m, int32_t k, int64_t ld,
              int64_t n, int conn, int symmetric, int drop_self) {
    const size_t scan_bytes = csr_scan_bytes(m);
    if (!scan_bytes) { err.set_error("nnd_graph_csr: the scan's storage query failed"); return 1; }
    const size_t rows1 = (size_t)m + 1;
    const size_t small_bytes = 2 * csr_room(8 * rows1) + csr_room(scan_bytes) +
                               (symmetric ? csr_room(8 * rows1) + 2 * csr_room(4 * rows1) : 0);
    csr_carve small{tmp.get<unsigned char>(&err, small_bytes)};
    if (!small.base) return 1;
    unsigned long long *cnt = small.take<unsigned long long>(rows1);
    int64_t *sums = small.take<int64_t>(rows1);  // the scan that becomes indptr
    unsigned char *scan_tmp = small.take<unsigned char>(scan_bytes);
    CSR_HIP(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * rows1, st));
    if (!symmetric) {
        if (m > 0) hipLaunchKernelGGL((k_csr_count_rows<IdT>), dim3(csr_grid(m, 256, 4096)), dim3(256), 0, st, ids, m, k, ld, n, drop_self, cnt);
        if (csr_scan(err, scan_tmp, scan_bytes, st, cnt, sums, m, &g->nnz)) return 1;
        if (csr_result(err, st, g, sums, m)) return 1;
        if (g->nnz > 0) launch_write_rows<IdT>(st, ids, vals, m, k, ld, n, drop_self, conn, g->indptr, g->indices, g->data);
        CSR_HIP(hipGetLastError());
        return 0;
    }
    // symmetric: every row's places and reverse edges staged in one stretch, merged per row, packed
    int64_t *roff = small.take<int64_t>(rows1);
    unsigned int *cursor = small.take<unsigned int>(rows1);  // [n]: the number of long rows
    int32_t *long_rows = small.take<int32_t>(rows1);
    CSR_HIP(hipMemsetAsync(cursor, 0, sizeof(unsigned int) * rows1, st));
    const int64_t places = n * (int64_t)k;
    if (places > 0) hipLaunchKernelGGL((k_csr_sym_count<IdT>), dim3(csr_grid(places, 256, 8192)), dim3(256), 0, st, ids, n, k, ld, drop_self, cnt);
    int64_t reversed = 0;
    if (csr_scan(err, scan_tmp, scan_bytes, st, cnt, roff, n, &reversed)) return 1;
    const int64_t staged = places + reversed;
    uint64_t *stage = tmp.get<uint64_t>(&err, (size_t)staged);
    if (!stage) return 1;
    if (staged > 0) {
        hipLaunchKernelGGL((k_csr_sym_scatter<IdT>), dim3(csr_grid(places, 256, 8192)), dim3(256), 0, st, ids, vals, n, k, ld, drop_self,
                           (const int64_t *)roff, cursor, stage);
        CSR_HIP(hipMemsetAsync(cnt, 0, sizeof(unsigned long long) * rows1, st));  // from here on: the rows' final lengths
        hipLaunchKernelGGL(k_csr_sym_merge, dim3(csr_grid(n, 4, 1 << 20)), dim3(256), 0, st, n, k, (const int64_t *)roff, stage, cnt, long_rows,
                           cursor + n);
        hipLaunchKernelGGL(k_csr_sym_merge_long, dim3(256), dim3(256), 0, st, k, (const int64_t *)roff, stage, cnt, (const int32_t *)long_rows,
                           (const unsigned int *)(cursor + n));
    }
    unsigned int n_long = 0;
    CSR_HIP(hipMemcpyAsync(&n_long, cursor + n, sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    if (csr_scan(err, scan_tmp, scan_bytes, st, cnt, sums, n, &g->nnz)) return 1;
    g->long_rows = (int64_t)n_long;
    if (csr_result(err, st, g, sums, n)) return 1;
    if (g->nnz > 0) {
        int G = 1;
        while (G < 64 && (int64_t)G * n < g->nnz) G <<= 1;  // about one lane per entry of an average row
        hipLaunchKernelGGL(k_csr_copy_rows, dim3(csr_grid(n, 256 / G, 1 << 20)), dim3(256), 0, st, n, k, G, (const int64_t *)roff,
                           (const uint64_t *)stage, conn, (const int64_t *)g->indptr, g->indices, g->data);
    }
    CSR_HIP(hipGetLastError());
    return 0;
}

int csr_check(csr_err &err, const char *who, const void *ids, int32_t id_bytes, const float *vals, int64_t m, int32_t k, int64_t ld, int64_t n,
              int32_t mode, int32_t symmetric) {
    if (m < 0 || n < 1 || k < 1 || k > CSR_REG_CAP || ld < k || m >= (int64_t)0x7FFFFFF0 || n >= (int64_t)0x7FFFFFF0) {
        err.set_error("%s: bad shape (m = %lld, k = %d, ld = %lld, n = %lld; k <= %d)", who, (long long)m, (int)k, (long long)ld, (long long)n, CSR_REG_CAP);
        return 1;
    }
    if (id_bytes != 4 && id_bytes != 8) { err.set_error("%s: ids are int32 or int64 (id_bytes = %d)", who, (int)id_bytes); return 1; }
    if (mode < 0 || mode > (NND_CSR_CONNECTIVITY | NND_CSR_DROP_SELF)) { err.set_error("%s: unknown mode %d", who, (int)mode); return 1; }
    if (symmetric && m != n) { err.set_error("%s: the symmetric form needs m == n (m = %lld, n = %lld)", who, (long long)m, (long long)n); return 1; }
    if (m > 0 && (!ids || !vals)) { err.set_error("%s: null pointer", who); return 1; }
    return 0;
}

int csr_run(csr_err &err, hipStream_t st, nnd_csr_s *g, const void *ids, int32_t id_bytes, const float *vals, int64_t m, int32_t k, int64_t ld,
            int64_t n, int32_t mode, int32_t symmetric) {
    nnd_scratch tmp;  // released on return, behind the synchronise below
    const int conn = (mode & NND_CSR_CONNECTIVITY) ? 1 : 0, drop_self = (mode & NND_CSR_DROP_SELF) ? 1 : 0;
    g->m = m;
    const int rc = id_bytes == 4 ? csr_build<int32_t>(err, tmp, st, g, (const int32_t *)ids, vals, m, k, ld, n, conn, symmetric ? 1 : 0, drop_self)
                                 : csr_build<int64_t>(err, tmp, st, g, (const int64_t *)ids, vals, m, k, ld, n, conn, symmetric ? 1 : 0, drop_self);
    const hipError_t e = hipStreamSynchronize(st);  // (on every path: the scratch goes when this returns)
    if (rc) return 1;
    if (e != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_graph_csr: a kernel failed: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
}  // namespace

extern "C" int32_t nnd_graph_csr_device(int32_t device, void *hip_stream, const void *ids_dev, int32_t id_bytes, const float *vals_dev, int64_t m,
                                        int32_t k, int64_t ld, int64_t n, int32_t mode, int32_t symmetric, nnd_csr_t *out) {
    csr_err err;
    if (!out) { err.set_error("nnd_graph_csr_device: null pointer"); return 1; }
    *out = nullptr;
    if (csr_check(err, "nnd_graph_csr_device", ids_dev, id_bytes, vals_dev, m, k, ld, n, mode, symmetric)) return 1;
    CSR_HIP(hipSetDevice(device));
    nnd_csr_s *g = new nnd_csr_s();
    g->device = device;
    if (csr_run(err, (hipStream_t)hip_stream, g, ids_dev, id_bytes, vals_dev, m, k, ld, n, mode, symmetric)) { delete g; return 1; }
    *out = g;
    return 0;
}

extern "C" int32_t nnd_csr_arrays(nnd_csr_t g, const int64_t **indptr_dev, const int32_t **indices_dev, const float **data_dev, int64_t *nnz,
                                  int64_t *long_rows) {
    if (!g) { nnd_set_global_error("nnd_csr_arrays: null handle"); return 1; }
    if (indptr_dev) *indptr_dev = g->indptr;
    if (indices_dev) *indices_dev = g->indices;
    if (data_dev) *data_dev = g->data;
    if (nnz) *nnz = g->nnz;
    if (long_rows) *long_rows = g->long_rows;
    return 0;
}

extern "C" int32_t nnd_csr_destroy(nnd_csr_t g) {
    if (!g) return 0;
    if (hipSetDevice(g->device) != hipSuccess) (void)hipGetLastError();
    delete g;
    return 0;
}

extern "C" int32_t nnd_graph_csr(int32_t device, const void *ids, int32_t id_bytes, const float *vals, int64_t m, int32_t k, int64_t n, int32_t mode,
                                 int32_t symmetric, int64_t *indptr, int32_t *indices, float *data, int64_t capacity, int64_t *nnz,
                                 int64_t *long_rows) {
    csr_err err;
    if (csr_check(err, "nnd_graph_csr", ids, id_bytes, vals, m, k, k, n, mode, symmetric)) return 1;
    if (!indptr || !nnz || capacity < 0 || (capacity > 0 && (!indices || !data))) { err.set_error("nnd_graph_csr: null pointer"); return 1; }
    CSR_HIP(hipSetDevice(device));
    nnd_csr_s g;
    g.device = device;
    nnd_scratch up;
    const size_t places = (size_t)m * (size_t)k;
    unsigned char *ids_dev = up.get<unsigned char>(&err, places * (size_t)id_bytes);
    float *vals_dev = up.get<float>(&err, places);
    if (!ids_dev || !vals_dev) return 1;
    hipStream_t st = nullptr;
    if (places > 0) {
        CSR_HIP(hipMemcpyAsync(ids_dev, ids, places * (size_t)id_bytes, hipMemcpyHostToDevice, st));
        CSR_HIP(hipMemcpyAsync(vals_dev, vals, places * sizeof(float), hipMemcpyHostToDevice, st));
    }
    if (csr_run(err, st, &g, ids_dev, id_bytes, vals_dev, m, k, k, n, mode, symmetric)) return 1;
    *nnz = g.nnz;
    if (long_rows) *long_rows = g.long_rows;
    if (g.nnz > capacity) { err.set_error("nnd_graph_csr: %lld entries, room for %lld", (long long)g.nnz, (long long)capacity); return 1; }
    CSR_HIP(hipMemcpy(indptr, g.indptr, sizeof(int64_t) * (size_t)(m + 1), hipMemcpyDeviceToHost));
    if (g.nnz > 0) {
        CSR_HIP(hipMemcpy(indices, g.indices, sizeof(int32_t) * (size_t)g.nnz, hipMemcpyDeviceToHost));
        CSR_HIP(hipMemcpy(data, g.data, sizeof(float) * (size_t)g.nnz, hipMemcpyDeviceToHost));
    }
    return 0;
}
