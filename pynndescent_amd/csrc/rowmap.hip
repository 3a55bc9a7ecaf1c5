// rowmap.hip -- the per-row maps of the derived metrics (row_map.py; DESIGN.md "Row maps"): a name that means "this map of every
// row, then a metric the kernels already have".
//     k_rank_rows / k_rank_rows_sort:  Y[i, :] = average ranks of X[i, :]        (spearmanr = correlation of the rank rows)
//     k_sphere_rows:                   Y[i, :] = P(lat, lon) - c, three floats   (haversine = a function of the chord |P(x) - P(y)|)
// float32 rows with an element stride in, contiguous float32 rows out.  Everything behind these kernels runs the metric code of
// the base metric on Y unchanged (metric.h is not touched).
//
// The contract of both, as linear.hip states its own: a row's result depends on that row alone -- not on n, on the row's place in
// a workgroup, on its neighbours in the launch, or on the run.  Columns at or beyond d (the padding of a stride) are never read.
// Duplicate rows stay duplicates, so their distance is exactly 0.
//
// Ranks.  r_j = #{i : x_i < x_j} + (#{i : x_i == x_j} + 1) / 2: the average rank, ties sharing the mean of their places
// (scipy's rankdata(method="average"), the reference's distances.py rankdata).  Both counts are integers below 2^23, so r_j is
// an exact half-integer in float32 and the output equals the numpy model bit for bit: there is no rounding anywhere.  -0.0 and
// 0.0 compare equal and tie.  NaN never reaches a build (the input checks reject it); the kernels are still defined on it: in
// the counting form every comparison with a NaN is false (it is below nobody and nobody is below it, so it ties with the row's
// smallest values), in the sorting form a NaN is ordered by its bit pattern beyond the infinities of its sign; no loop's trip
// count depends on a value, and no index does beyond the counts' own range.
//   d <= RM_RANK_WAVE_MAX: the counting form.  One wave per row, four rows per workgroup, no workgroup barrier.  The wave stages
//   its row once in a wave-private LDS slice; lane l owns the elements l, l + 64, ... (NI of them, in registers) and walks the
//   row as 16-byte LDS reads whose address is the same in every lane (a broadcast: no bank conflict), counting the values below
//   each of its elements: one compare and one add-with-carry per pair, 2 d^2 / 64 wave-instructions per row.  The slice is padded
//   to NI * 64 elements with NaN, which is below nobody.  The ties need no second compare: equal values share their count and
//   distinct values do not, so one LDS tally indexed by the count (d atomic adds per row) holds every element's number of ties.
//   d <= RM_RANK_MAX: the sorting form.  One workgroup per row: (ordered value bits, index) keys of 64 bits, padded to a power
//   of two P with keys above every real one, bitonic-sorted in LDS (log2 P (log2 P + 1) / 2 passes); then every element finds
//   the two ends of its tie run by two binary searches of log2 P + 1 steps each.  The keys are distinct, so the sorted order is unique.
//
// Sphere.  P(lat, lon) = (cos lat cos lon, cos lat sin lon, sin lat) in float64, minus the float64 value of the float32 shift c,
// rounded to float32 once.  c is a point near the data (the mean of P over a sample of the training rows, fixed when the index
// is built): euclidean distance does not see it, and the rounding error of a component then scales with the extent of the data
// instead of with 1.  One thread per row; the kernel is bound by its memory traffic (8 bytes in, 12 out).
#include <stdarg.h>
#include <stdio.h>

#include "common.h"
#include "devmem.h"
#include "state.h"

#define RM_RANK_WAVE_MAX 1024  // largest d of the counting form: 16 elements per lane
#define RM_RANK_MAX 16384      // largest d of the sorting form: 128 KiB of keys
#define RM_SORT_THREADS 512

template <int NI>
__global__ __launch_bounds__(256) void k_rank_rows(const float *__restrict__ x, int64_t ld, int64_t n, int d, float *__restrict__ y) {
    __shared__ __attribute__((aligned(16))) float slices[4][NI * 64];
    __shared__ int tallies[4][NI * 64];
    const int lane = nnd_lane(), wave = (int)threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= n) return;  // (wave-uniform; the kernel has no workgroup barrier)
    float *s = slices[wave];
    int *tally = tallies[wave];
    const float *xr = x + row * ld;
    float e[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int j = lane + 64 * i;
        e[i] = j < d ? xr[j] : __builtin_nanf("");
        s[j] = e[i];
        tally[j] = 0;
    }
    nnd_wave_lds_sync();
    int lt[NI];
#pragma unroll
    for (int i = 0; i < NI; i++) lt[i] = 0;
    const int d4 = (d + 3) >> 2;  // 4 * d4 <= NI * 64: the last chunk ends inside the slice, in its NaN padding
    for (int j4 = 0; j4 < d4; j4++) {
        const float4 v = *(const float4 *)&s[4 * j4];
#pragma unroll
        for (int i = 0; i < NI; i++) lt[i] += (int)(v.x < e[i]) + (int)(v.y < e[i]) + (int)(v.z < e[i]) + (int)(v.w < e[i]);
    }
    // lt < d (an element is not below itself), equal values share their lt and distinct values do not: tally[lt] counts the ties
#pragma unroll
    for (int i = 0; i < NI; i++)
        if (lane + 64 * i < d) atomicAdd(&tally[lt[i]], 1);
    nnd_wave_lds_sync();
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int j = lane + 64 * i;
        if (j < d) y[row * (int64_t)d + j] = (float)(2 * lt[i] + tally[lt[i]] + 1) * 0.5f;
    }
}

// the number of keys[0 .. d) that are < target (or <= target), 0 .. d: keys ascending, P a power of two >= d; log2 P + 1 steps
// (the first, of P itself, is taken only when d == P and every key counts)
__device__ __forceinline__ int rm_count_below(const unsigned long long *keys, int d, int P, unsigned long long target, bool inclusive) {
    int pos = 0;
    for (int step = P; step >= 1; step >>= 1) {
        const int at = pos + step;
        if (at <= d) {
            const unsigned long long k = keys[at - 1];
            if (inclusive ? k <= target : k < target) pos = at;
        }
    }
    return pos;
}

template <int P_MAX>
__global__ __launch_bounds__(RM_SORT_THREADS) void k_rank_rows_sort(const float *__restrict__ x, int64_t ld, int64_t n, int d, int P,
                                                                    float *__restrict__ y) {
    __shared__ unsigned long long keys[P_MAX];  // d <= P <= P_MAX
    const int tid = (int)threadIdx.x;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {  // (block-uniform trip count)
        const float *xr = x + row * ld;
        for (int j = tid; j < P; j += RM_SORT_THREADS) {
            unsigned long long key = ~0ull;  // padding: above every real key (a real key's index is below d)
            if (j < d) {
                float v = xr[j];
                if (v == 0.0f) v = 0.0f;  // -0.0 ties with 0.0
                uint32_t u = __float_as_uint(v);
                u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // unsigned order = float order
                key = ((unsigned long long)u << 32) | (unsigned)j;
            }
            keys[j] = key;
        }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < (P >> 1); t += RM_SORT_THREADS) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;  // lo < hi < P
                    const unsigned long long a = keys[lo], b = keys[hi];
                    if ((a > b) == ((lo & k) == 0)) { keys[lo] = b; keys[hi] = a; }
                }
                __syncthreads();
            }
        }
        for (int p = tid; p < d; p += RM_SORT_THREADS) {  // places 0 .. d - 1 hold the real keys
            const unsigned long long key = keys[p], base = key & 0xFFFFFFFF00000000ull;
            const int lt = rm_count_below(keys, d, P, base, false), le = rm_count_below(keys, d, P, base | 0xFFFFFFFFull, true);
            y[row * (int64_t)d + (int)(uint32_t)key] = (float)(lt + le + 1) * 0.5f;  // lt + (eq + 1) / 2, eq = le - lt
        }
        __syncthreads();  // the next row's keys stay behind this row's searches
    }
}

__global__ __launch_bounds__(256) void k_sphere_rows(const float *__restrict__ x, int64_t ld, const float *__restrict__ shift, int64_t n,
                                                     float *__restrict__ y) {
#pragma clang fp contract(off)
    const double c0 = (double)shift[0], c1 = (double)shift[1], c2 = (double)shift[2];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double lat = (double)x[i * ld], lon = (double)x[i * ld + 1];
        const double cl = cos(lat), sl = sin(lat), co = cos(lon), so = sin(lon);
        const double p0 = cl * co, p1 = cl * so;
        y[3 * i + 0] = (float)(p0 - c0);
        y[3 * i + 1] = (float)(p1 - c1);
        y[3 * i + 2] = (float)(sl - c2);
    }
}

// The output width of a map: dim for the ranks, 3 for the sphere (whose input width is 2); 0: a kind or a width the map refuses.
static int rm_out_dim(int kind, int dim) {
    if (kind == NND_ROWMAP_RANK) return dim >= 1 && dim <= RM_RANK_MAX ? dim : 0;
    if (kind == NND_ROWMAP_SPHERE) return dim == 2 ? 3 : 0;
    return 0;
}

// (n, d) float32 rows of stride ld at x -> contiguous rows at y, all on the current device, queued on `st`.
int nnd_launch_map_rows(hipStream_t st, int kind, const float *shift, const float *x, int64_t ld, int64_t n, int d, float *y) {
    if (n <= 0) return 0;
    if (!rm_out_dim(kind, d) || ld < d) return 1;
    if (kind == NND_ROWMAP_SPHERE) {
        int64_t blocks = (n + 255) / 256;
        if (blocks > 65536) blocks = 65536;  // (the kernel strides over the rest)
        hipLaunchKernelGGL(k_sphere_rows, dim3((unsigned)blocks), dim3(256), 0, st, x, ld, shift, n, y);
    } else if (d <= RM_RANK_WAVE_MAX) {
        const int64_t blocks = (n + 3) / 4;
        if (blocks > (int64_t)0x7FFFFFFF) return 1;
        const dim3 g((unsigned)blocks), b(256);
        if (d <= 64) hipLaunchKernelGGL(k_rank_rows<1>, g, b, 0, st, x, ld, n, d, y);
        else if (d <= 128) hipLaunchKernelGGL(k_rank_rows<2>, g, b, 0, st, x, ld, n, d, y);
        else if (d <= 256) hipLaunchKernelGGL(k_rank_rows<4>, g, b, 0, st, x, ld, n, d, y);
        else if (d <= 512) hipLaunchKernelGGL(k_rank_rows<8>, g, b, 0, st, x, ld, n, d, y);
        else hipLaunchKernelGGL(k_rank_rows<16>, g, b, 0, st, x, ld, n, d, y);
    } else {
        int P = 2048;
        while (P < d) P <<= 1;  // d <= RM_RANK_MAX: P <= 16384
        const dim3 g((unsigned)(n < 65536 ? n : 65536)), b(RM_SORT_THREADS);  // (the kernel strides over the rest)
        if (P <= 4096) hipLaunchKernelGGL(k_rank_rows_sort<4096>, g, b, 0, st, x, ld, n, d, P, y);
        else hipLaunchKernelGGL(k_rank_rows_sort<RM_RANK_MAX>, g, b, 0, st, x, ld, n, d, P, y);
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

namespace {
struct rm_err {  // the error sink of an entry without a handle: what nnd_last_global_error returns
    char msg[256];
    void set_error(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        nnd_set_global_error(msg);
    }
};
bool rm_args_ok(rm_err &err, const char *who, int32_t kind, int32_t dim, int64_t x_stride, int64_t n, const void *shift, const void *x, const void *y) {
    if (!rm_out_dim(kind, dim) || n < 0 || x_stride < dim) { err.set_error("%s: bad kind, width or stride (ranks take 1 .. %d columns, the sphere 2)", who, RM_RANK_MAX); return false; }
    if ((kind == NND_ROWMAP_SPHERE && !shift) || (n > 0 && (!x || !y))) { err.set_error("%s: null pointer", who); return false; }
    return true;
}
}  // namespace

extern "C" int32_t nnd_device_map_rows(int32_t device, void *hip_stream, int32_t kind, int32_t dim, int64_t x_stride, const float *shift_dev,
                                       const float *x_dev, int64_t n, float *y_dev) {
    rm_err err;
    if (!rm_args_ok(err, "nnd_device_map_rows", kind, dim, x_stride, n, shift_dev, x_dev, y_dev)) return 1;
    if (n == 0) return 0;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_device_map_rows: no such device"); return 1; }
    if (nnd_launch_map_rows((hipStream_t)hip_stream, kind, shift_dev, x_dev, x_stride, n, dim, y_dev)) {
        (void)hipGetLastError();
        err.set_error("nnd_device_map_rows: kernel launch failed");
        return 1;
    }
    return 0;
}

extern "C" int32_t nnd_map_rows_host(int32_t device, int32_t kind, int32_t dim, int64_t x_stride, const float *shift, const float *x, int64_t n,
                                     float *y) {
    rm_err err;
    if (!rm_args_ok(err, "nnd_map_rows_host", kind, dim, x_stride, n, shift, x, y)) return 1;
    if (n == 0) return 0;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_map_rows_host: no HIP device %d", (int)device); return 1; }
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_map_rows_host: no stream"); return 1; }
    const size_t in_count = (size_t)(n - 1) * (size_t)x_stride + (size_t)dim, out_count = (size_t)n * (size_t)rm_out_dim(kind, dim);
    int rc = 1;
    {
        nnd_scratch tmp;
        do {
            float *d_shift = kind == NND_ROWMAP_SPHERE ? tmp.get<float>(&err, 3) : nullptr;
            float *d_x = tmp.get<float>(&err, in_count), *d_y = tmp.get<float>(&err, out_count);
            if ((kind == NND_ROWMAP_SPHERE && !d_shift) || !d_x || !d_y) break;
            bool ok = !d_shift || hipMemcpyAsync(d_shift, shift, sizeof(float) * 3, hipMemcpyHostToDevice, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(d_x, x, sizeof(float) * in_count, hipMemcpyHostToDevice, st) == hipSuccess;
            if (!ok) { (void)hipGetLastError(); err.set_error("nnd_map_rows_host: host-to-device copy failed"); break; }
            if (nnd_launch_map_rows(st, kind, d_shift, d_x, x_stride, n, dim, d_y)) { (void)hipGetLastError(); err.set_error("nnd_map_rows_host: kernel launch failed"); break; }
            if (hipMemcpyAsync(y, d_y, sizeof(float) * out_count, hipMemcpyDeviceToHost, st) != hipSuccess) {
                (void)hipGetLastError();
                err.set_error("nnd_map_rows_host: device-to-host copy failed");
                break;
            }
            rc = 0;
        } while (0);
        const hipError_t e = hipStreamSynchronize(st);  // before the scratch goes
        if (!rc && e != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_map_rows_host: kernel or copy failed: %s", hipGetErrorString(e)); rc = 1; }
    }
    (void)hipStreamDestroy(st);
    return rc;
}
