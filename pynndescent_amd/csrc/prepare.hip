// prepare.hip -- the device glue of NNDescent.prepare() for an index whose rows and graph live on the device (built from a
// torch tensor): what search_tree.py / nndescent.py do with numpy and scipy on the host path, between kernels that were on the
// device already (hubtree.hip, prune.hip / searchgraph.hip, searcher.hip / query.hip):
//   nnd_rank_order_device    compute_global_degrees (rp_trees.py:714-744) + the (-degree, id) order of make_hub_tree:
//                            k_prep_degrees -> k_prep_rank_keys -> rocprim::radix_sort_keys -> k_prep_rank_ids
//   nnd_reorder_csr_device   the search graph in the hub tree's leaf order (pynndescent_.py:1629-1651; scipy's
//                            g[order, :].tocsc()[:, order].tocsr() + sort_indices()):
//                            k_prep_inverse -> rocprim::exclusive_scan -> k_prep_relabel_rows (one wave per row)
//   nnd_reorder_host         the same and the rows' gather (devarray.hip nnd_launch_gather_rows) on host arrays: the test entry
// Bytes moved at n points, k neighbours, nnz edges: the rank reads the graph once (4 n k) and sorts n 8-byte keys; the reorder
// reads and writes the CSR once (8 nnz + 8 n) plus one 4-byte gather per edge through the inverse permutation; the rows' gather
// (searcher.hip nnd_searcher_create_device) reads and writes the point set once.  None of the entries has a handle: they take a
// device ordinal and a stream, like those of devarray.hip, and return when the stream has drained.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "state.h"

#define PREP_ROW_CAP 384  // CSR row entries a wave sorts through LDS: round(1.5 * 256), the degree bound at k = 256; longer rows: global memory

// ---------------------------------------------------------------------------------------------- in-degrees and hub rank
// how often every id appears as somebody's neighbour; ids outside [0, n) are skipped (unfilled slots are -1)
__global__ __launch_bounds__(256) void k_prep_degrees(const int32_t *__restrict__ idx, int64_t total, int64_t n, uint32_t *__restrict__ deg) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int32_t u = idx[e];
        if (u >= 0 && (int64_t)u < n) atomicAdd(&deg[u], 1u);
    }
}
// ascending keys = descending degree, ties by ascending id: numpy.argsort(-degree, kind="stable")
__global__ __launch_bounds__(256) void k_prep_rank_keys(const uint32_t *__restrict__ deg, int64_t n, uint64_t *__restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        keys[i] = ((uint64_t)(0xFFFFFFFFu - deg[i]) << 32) | (uint64_t)(uint32_t)i;
}
__global__ __launch_bounds__(256) void k_prep_rank_ids(const uint64_t *__restrict__ keys, int64_t n, int32_t *__restrict__ rank) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        rank[i] = (int32_t)(uint32_t)keys[i];
}

// ---------------------------------------------------------------------------------------------- reorder of the CSR graph
// inv[order[i]] = i; len[i] = length of old row order[i]; len[n] = 0 (the scan's last position is the total).  An entry of
// `order` outside [0, n) (a caller's error) is left out: nothing is read or written out of bounds.
__global__ __launch_bounds__(256) void k_prep_inverse(const int32_t *__restrict__ order, int64_t n, const int32_t *__restrict__ indptr,
                                                      int32_t *__restrict__ inv, int32_t *__restrict__ len) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
        if (i == n) { len[n] = 0; continue; }
        const int32_t o = order[i];
        const bool ok = o >= 0 && (int64_t)o < n;
        if (ok) inv[o] = (int32_t)i;
        len[i] = ok ? indptr[o + 1] - indptr[o] : 0;
    }
}
// One wave per new row i (= old row order[i]): every column j becomes inv[j], and the row is written in ascending order.  The
// relabelled row is staged in LDS (PREP_ROW_CAP words per wave) and rank-sorted: entry e goes to the position "entries smaller
// than it, or equal and in front of it" -- L broadcast reads per entry, ceil(L / 64) entries per lane; columns of a CSR row are
// distinct, the tie rule only keeps the positions a permutation whatever the input.  A row longer than PREP_ROW_CAP takes the same
// steps with the staged values re-read through global memory.
__global__ __launch_bounds__(256) void k_prep_relabel_rows(const int32_t *__restrict__ order, int64_t n, const int32_t *__restrict__ indptr,
                                                           const int32_t *__restrict__ indices, const int32_t *__restrict__ inv,
                                                           const int32_t *__restrict__ indptr_out, int32_t *__restrict__ indices_out) {
    __shared__ int32_t stage[4][PREP_ROW_CAP];
    const int lane = nnd_lane(), w = threadIdx.x >> 6;
    int32_t *row = stage[w];
    for (int64_t i = (int64_t)blockIdx.x * 4 + w; i < n; i += (int64_t)gridDim.x * 4) {  // wave-uniform
        const int32_t o = order[i];
        if (o < 0 || (int64_t)o >= n) continue;
        const int32_t a = indptr[o], L = indptr[o + 1] - a, at = indptr_out[i];
        const int32_t *src = indices + a;
        const bool staged = L <= PREP_ROW_CAP;
        if (staged)
            for (int e = lane; e < L; e += 64) row[e] = inv[src[e]];
        __builtin_amdgcn_wave_barrier();  // (one wave: its LDS accesses are served in program order)
        for (int e = lane; e < L; e += 64) {
            const int32_t mine = staged ? row[e] : inv[src[e]];
            int pos = 0;
            for (int j = 0; j < L; j++) {
                const int32_t v = staged ? row[j] : inv[src[j]];
                pos += (v < mine || (v == mine && j < e)) ? 1 : 0;
            }
            indices_out[at + pos] = mine;
        }
        __builtin_amdgcn_wave_barrier();  // the next row's staging stays behind this row's reads
    }
}

// ---------------------------------------------------------------------------------------------- host side
namespace {
struct prep_err {  // the error sink of an entry without a handle: what nnd_last_global_error returns
    char msg[256];
    void set_error(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        nnd_set_global_error(msg);
    }
};
unsigned prep_grid(int64_t items) {  // 256 threads per block, at most 4096 blocks: the kernels stride over the rest
    const int64_t b = (items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}
#define PREP_HIP(expr)                                                                                      \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) {                                                                             \
            (void)hipGetLastError();                                                                        \
            err.set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);       \
            return 1;                                                                                       \
        }                                                                                                   \
    } while (0)

// the kernels of the CSR reorder on `st`; the scratch lives in `tmp` (the caller drains the stream before it lets go of it)
int reorder_csr(prep_err &err, nnd_scratch &tmp, hipStream_t st, const int32_t *order, int64_t n, const int32_t *indptr, const int32_t *indices,
                int64_t nnz, int32_t *indptr_out, int32_t *indices_out) {
    if (!order) {  // identity: the graph as it is
        PREP_HIP(hipMemcpyAsync(indptr_out, indptr, sizeof(int32_t) * (size_t)(n + 1), hipMemcpyDeviceToDevice, st));
        if (nnz > 0) PREP_HIP(hipMemcpyAsync(indices_out, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    int32_t *inv = tmp.get<int32_t>(&err, (size_t)n), *len = tmp.get<int32_t>(&err, (size_t)n + 1);
    if (!inv || !len) return 1;
    size_t scan_bytes = 0;
    PREP_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, len, indptr_out, 0, (size_t)(n + 1), rocprim::plus<int32_t>(), st));
    unsigned char *scan_tmp = tmp.get<unsigned char>(&err, scan_bytes + 256);
    if (!scan_tmp) return 1;
    hipLaunchKernelGGL(k_prep_inverse, dim3(prep_grid(n + 1)), dim3(256), 0, st, order, n, indptr, inv, len);
    PREP_HIP(rocprim::exclusive_scan(scan_tmp, scan_bytes, len, indptr_out, 0, (size_t)(n + 1), rocprim::plus<int32_t>(), st));
    if (nnz > 0) {
        const int64_t blocks = (n + 3) / 4;
        hipLaunchKernelGGL(k_prep_relabel_rows, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, st, order, n, indptr, indices,
                           (const int32_t *)inv, (const int32_t *)indptr_out, indices_out);
    }
    PREP_HIP(hipGetLastError());
    return 0;
}
}  // namespace

extern "C" int32_t nnd_rank_order_device(int32_t device, void *hip_stream, const int32_t *idx_dev, int64_t n, int32_t k, int32_t *rank_order_dev) {
    prep_err err;
    if (n < 0 || k < 0 || n >= (int64_t)0x7FFFFFF0) { err.set_error("nnd_rank_order_device: bad shape (n = %lld, k = %d)", (long long)n, (int)k); return 1; }
    if (n == 0) return 0;
    if (!rank_order_dev || (k > 0 && !idx_dev)) { err.set_error("nnd_rank_order_device: null pointer"); return 1; }
    PREP_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    nnd_scratch tmp;  // released on return, behind the synchronise below
    uint32_t *deg = tmp.get<uint32_t>(&err, (size_t)n);
    uint64_t *keys = tmp.get<uint64_t>(&err, (size_t)n), *keys2 = tmp.get<uint64_t>(&err, (size_t)n);
    if (!deg || !keys || !keys2) return 1;
    size_t sort_bytes = 0;
    PREP_HIP(rocprim::radix_sort_keys(nullptr, sort_bytes, keys, keys2, (size_t)n, 0u, 64u, st));
    unsigned char *sort_tmp = tmp.get<unsigned char>(&err, sort_bytes + 256);
    if (!sort_tmp) return 1;
    int rc = 0;
    do {
        if (hipMemsetAsync(deg, 0, sizeof(uint32_t) * (size_t)n, st) != hipSuccess) { rc = 1; break; }
        const int64_t total = n * (int64_t)k;
        if (total > 0) hipLaunchKernelGGL(k_prep_degrees, dim3(prep_grid(total)), dim3(256), 0, st, idx_dev, total, n, deg);
        hipLaunchKernelGGL(k_prep_rank_keys, dim3(prep_grid(n)), dim3(256), 0, st, (const uint32_t *)deg, n, keys);
        // the key bits that matter: the 32 of the id and those of 0xFFFFFFFF - degree, all 32 (a small degree is a large word)
        if (rocprim::radix_sort_keys(sort_tmp, sort_bytes, keys, keys2, (size_t)n, 0u, 64u, st) != hipSuccess) { rc = 1; break; }
        hipLaunchKernelGGL(k_prep_rank_ids, dim3(prep_grid(n)), dim3(256), 0, st, (const uint64_t *)keys2, n, rank_order_dev);
        if (hipGetLastError() != hipSuccess) rc = 1;
    } while (0);
    const hipError_t e = hipStreamSynchronize(st);  // (on every path: the scratch goes when the call returns)
    if (rc || e != hipSuccess) {
        (void)hipGetLastError();
        err.set_error("nnd_rank_order_device: a kernel, the sort or the synchronise failed (%s)", hipGetErrorString(e));
        return 1;
    }
    return 0;
}

extern "C" int32_t nnd_reorder_csr_device(int32_t device, void *hip_stream, const int32_t *order_dev, int64_t n, const int32_t *indptr_dev,
                                          const int32_t *indices_dev, int64_t nnz, int32_t *indptr_out_dev, int32_t *indices_out_dev) {
    prep_err err;
    if (n < 1 || nnz < 0 || n >= (int64_t)0x7FFFFFF0 || nnz >= (int64_t)0x7FFFFFF0) { err.set_error("nnd_reorder_csr_device: bad shape (n = %lld, nnz = %lld)", (long long)n, (long long)nnz); return 1; }
    if (!indptr_dev || !indptr_out_dev || (nnz > 0 && (!indices_dev || !indices_out_dev))) { err.set_error("nnd_reorder_csr_device: null pointer"); return 1; }
    PREP_HIP(hipSetDevice(device));
    hipStream_t st = (hipStream_t)hip_stream;
    nnd_scratch tmp;
    const int rc = reorder_csr(err, tmp, st, order_dev, n, indptr_dev, indices_dev, nnz, indptr_out_dev, indices_out_dev);
    const hipError_t e = hipStreamSynchronize(st);
    if (rc) return 1;
    if (e != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_reorder_csr_device: kernel failed: %s", hipGetErrorString(e)); return 1; }
    return 0;
}

extern "C" int32_t nnd_reorder_host(int32_t device, int64_t n, int32_t dim, const int32_t *order, const int32_t *indptr, const int32_t *indices,
                                    int64_t nnz, const float *x, int32_t *indptr_out, int32_t *indices_out, float *x_out) {
    prep_err err;
    if (n < 1 || dim < 1 || nnz < 0 || n >= (int64_t)0x7FFFFFF0 || nnz >= (int64_t)0x7FFFFFF0) { err.set_error("nnd_reorder_host: bad shape"); return 1; }
    if (!indptr || !indptr_out || !x || !x_out || (nnz > 0 && (!indices || !indices_out))) { err.set_error("nnd_reorder_host: null pointer"); return 1; }
    // the arrays are a caller's: everything a kernel would index with is checked here
    if (indptr[0] != 0 || (int64_t)indptr[n] != nnz) { err.set_error("nnd_reorder_host: indptr does not span 0 .. nnz"); return 1; }
    for (int64_t i = 0; i < n; i++)
        if (indptr[i + 1] < indptr[i]) { err.set_error("nnd_reorder_host: indptr decreases at row %lld", (long long)i); return 1; }
    for (int64_t e = 0; e < nnz; e++)
        if (indices[e] < 0 || (int64_t)indices[e] >= n) { err.set_error("nnd_reorder_host: column %d at entry %lld is outside [0, n)", (int)indices[e], (long long)e); return 1; }
    if (order) {
        std::vector<char> seen((size_t)n, 0);
        for (int64_t i = 0; i < n; i++) {
            const int32_t o = order[i];
            if (o < 0 || (int64_t)o >= n || seen[(size_t)o]) { err.set_error("nnd_reorder_host: order is not a permutation of [0, n)"); return 1; }
            seen[(size_t)o] = 1;
        }
    }
    PREP_HIP(hipSetDevice(device));
    const int dp = (dim + 3) & ~3;
    hipStream_t st = nullptr;
    PREP_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    int rc = 1;
    {
        nnd_scratch tmp;
        do {
            int32_t *d_order = order ? tmp.get<int32_t>(&err, (size_t)n) : nullptr;
            int32_t *d_ptr = tmp.get<int32_t>(&err, (size_t)n + 1), *d_ind = tmp.get<int32_t>(&err, (size_t)nnz);
            int32_t *d_ptr2 = tmp.get<int32_t>(&err, (size_t)n + 1), *d_ind2 = tmp.get<int32_t>(&err, (size_t)nnz);
            float *d_x = tmp.get<float>(&err, (size_t)n * dim), *d_x2 = tmp.get<float>(&err, (size_t)n * dp);
            if ((order && !d_order) || !d_ptr || !d_ind || !d_ptr2 || !d_ind2 || !d_x || !d_x2) break;
            bool ok = true;
            if (order) ok = ok && hipMemcpyAsync(d_order, order, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(d_ptr, indptr, sizeof(int32_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st) == hipSuccess;
            if (nnz > 0) ok = ok && hipMemcpyAsync(d_ind, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(d_x, x, sizeof(float) * (size_t)n * dim, hipMemcpyHostToDevice, st) == hipSuccess;
            if (!ok) { (void)hipGetLastError(); err.set_error("nnd_reorder_host: host-to-device copy failed"); break; }
            if (reorder_csr(err, tmp, st, d_order, n, d_ptr, d_ind, nnz, d_ptr2, d_ind2)) break;
            if (nnd_launch_gather_rows(st, d_x, NND_DTYPE_FLOAT32, d_order, n, dim, dp, d_x2)) { (void)hipGetLastError(); err.set_error("nnd_reorder_host: gather launch failed"); break; }
            ok = hipMemcpyAsync(indptr_out, d_ptr2, sizeof(int32_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, st) == hipSuccess;
            if (nnz > 0) ok = ok && hipMemcpyAsync(indices_out, d_ind2, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(x_out, d_x2, sizeof(float) * (size_t)n * dp, hipMemcpyDeviceToHost, st) == hipSuccess;
            if (!ok) { (void)hipGetLastError(); err.set_error("nnd_reorder_host: device-to-host copy failed"); break; }
            rc = 0;
        } while (0);
        const hipError_t e = hipStreamSynchronize(st);  // before the scratch goes
        if (!rc && e != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_reorder_host: kernel or copy failed: %s", hipGetErrorString(e)); rc = 1; }
    }
    (void)hipStreamDestroy(st);
    return rc;
}
