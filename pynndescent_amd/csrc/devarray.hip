// devarray.hip -- what a caller whose arrays live on the device needs around the build and the search: typed rows (float16 /
// bfloat16 / float64 / float32) -> the float32 rows every kernel reads (in place of the rows, or gathered by a permutation into
// the searcher's padded layout: prepare() of a device-built index), dot's row normalisation, and the corrections
// NNDescent.neighbor_graph / query apply to the kernels' distances (pynndescent_.py:1271-1298), all without a host round trip.
// The two exported entries take a device ordinal and a stream instead of a handle: a graph is corrected long after its builder
// is gone, and a query batch is converted before any searcher sees it.
#include <float.h>
#include <stdio.h>

#include "common.h"
#include "convert_index.h"
#include "state.h"

// ---- typed rows -> float32 ----
template <typename T>
struct conv_traits;
template <>
struct conv_traits<float> {  // (dot on float32 rows: the copy that is normalised afterwards)
    static constexpr int VEC = 4;
    typedef float4 vec_t;
    __device__ static __forceinline__ float one(float v) { return v; }
    __device__ static __forceinline__ void many(const vec_t &v, float *o) { o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w; }
};
struct conv_f16 { uint16_t bits; };
struct conv_bf16 { uint16_t bits; };
__device__ static __forceinline__ float conv_half_bits(uint32_t b) {
    union { uint16_t u; _Float16 h; } c;
    c.u = (uint16_t)b;
    return (float)c.h;  // exact: every binary16 value (subnormals, inf, NaN) is a binary32 value
}
template <>
struct conv_traits<conv_f16> {
    static constexpr int VEC = 8;
    typedef uint4 vec_t;
    __device__ static __forceinline__ float one(conv_f16 v) { return conv_half_bits(v.bits); }
    __device__ static __forceinline__ void many(const vec_t &v, float *o) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            o[2 * i] = conv_half_bits(w[i] & 0xFFFFu);
            o[2 * i + 1] = conv_half_bits(w[i] >> 16);
        }
    }
};
template <>
struct conv_traits<conv_bf16> {  // bfloat16 is the upper half of a binary32: exact
    static constexpr int VEC = 8;
    typedef uint4 vec_t;
    __device__ static __forceinline__ float one(conv_bf16 v) { return __uint_as_float((uint32_t)v.bits << 16); }
    __device__ static __forceinline__ void many(const vec_t &v, float *o) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; i++) {
            o[2 * i] = __uint_as_float(w[i] << 16);
            o[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u);
        }
    }
};
struct conv_d4 { double2 a, b; };  // four doubles: two 16-byte loads of one 32-byte aligned group
template <>
struct conv_traits<double> {  // round to nearest even, what numpy's astype(float32) does
    static constexpr int VEC = 4;
    typedef conv_d4 vec_t;
    __device__ static __forceinline__ float one(double v) { return __double2float_rn(v); }
    __device__ static __forceinline__ void many(const vec_t &v, float *o) {
        o[0] = __double2float_rn(v.a.x); o[1] = __double2float_rn(v.a.y);
        o[2] = __double2float_rn(v.b.x); o[3] = __double2float_rn(v.b.y);
    }
};

// one work item per thread (convert_index.h): a whole aligned vector of the source, or one element of the head / tail.  The
// destination's vectors are stored whole when they are 16-byte aligned as well (dst_vec), element by element otherwise.
template <typename T>
__global__ __launch_bounds__(256) void k_rows_to_f32(const T *__restrict__ src, float *__restrict__ dst, nnd_conv_plan plan, int dst_vec) {
    typedef conv_traits<T> tr;
    const int64_t items = nnd_conv_items(plan);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t first;
        const int len = nnd_conv_item(plan, i, &first);
        if (len == 1) {
            dst[first] = tr::one(src[first]);
            continue;
        }
        float o[tr::VEC];
        tr::many(*(const typename tr::vec_t *)(src + first), o);
        if (dst_vec) {
#pragma unroll
            for (int c = 0; c < tr::VEC; c += 4) *(float4 *)(dst + first + c) = make_float4(o[c], o[c + 1], o[c + 2], o[c + 3]);
        } else {
#pragma unroll
            for (int c = 0; c < tr::VEC; c++) dst[first + c] = o[c];
        }
    }
}

// Correctly rounded float32 square root and quotient, whatever the compiler's float32 defaults are (__fsqrt_rn is the native,
// approximate instruction here): the float64 operation is correctly rounded, and rounding a 53-bit square root or quotient of
// 24-bit operands once more to 24 bits cannot differ from rounding the exact value (53 >= 2 * 24 + 2).
__device__ __forceinline__ float sqrt_rn_f32(float v) { return (float)__dsqrt_rn((double)v); }
__device__ __forceinline__ float div_rn_f32(float a, float b) { return (float)__ddiv_rn((double)a, (double)b); }

// ---- dot: x / sqrt(sum x^2) in place, one wave per row (pynndescent_.py:1101-1102, sklearn.preprocessing.normalize) ----
// float32 arithmetic like sklearn's row_norms, a correctly rounded square root and division like numpy's; a zero row stays zero.
// The order of a plain float32 sum is the wave's here and the host's SIMD width there, and each order carries its own rounding
// (up to about log2(d) / 2 ulp): two such sums put the rows up to 3 ulp apart (measured at d = 24).  So this side's sum carries
// its rounding errors along -- every product with its exact error (fma), every addition with its exact error (two_sum), in float32
// pairs -- and rounds once at the end: what is left between the two is the host's own rounding.
__device__ __forceinline__ void two_sum(float a, float b, float *s, float *e) {
#pragma clang fp contract(off)
    const float t = a + b, bb = t - a;
    *s = t;
    *e = (a - (t - bb)) + (b - bb);
}
__global__ __launch_bounds__(256) void k_normalize_rows(float *__restrict__ x, int64_t n, int d) {
    const int lane = nnd_lane();
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n) return;
    float *r = x + row * d;
    float hi = 0.0f, lo = 0.0f;
    for (int j = lane; j < d; j += 64) {
#pragma clang fp contract(off)  // (p must be the rounded product: the fma below measures exactly that rounding)
        const float v = r[j], p = v * v, pe = fmaf(v, v, -p);
        float e;
        two_sum(hi, p, &hi, &e);
        lo += e + pe;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float oh = __shfl_xor(hi, o, 64), ol = __shfl_xor(lo, o, 64);
        float e;
        two_sum(hi, oh, &hi, &e);
        lo = (lo + ol) + e;
    }
    const float s = hi + lo;
    if (!(s > 0.0f) && !(s != s)) return;  // zero row (a NaN goes on: the prep kernel flags it)
    const float nrm = sqrt_rn_f32(s);
    for (int j = lane; j < d; j += 64) r[j] = div_rn_f32(r[j], nrm);
}

template <typename T>
static int rows_launch(hipStream_t st, const void *src, int64_t count, float *dst) {
    typedef conv_traits<T> tr;
    const nnd_conv_plan plan = nnd_conv_make_plan((uint64_t)(uintptr_t)src, (int)sizeof(T), tr::VEC, count);
    const int64_t items = nnd_conv_items(plan);
    if (items <= 0) return 0;
    const int dst_vec = (((uintptr_t)dst + sizeof(float) * (size_t)plan.head) & 15) == 0 ? 1 : 0;
    int64_t blocks = (items + 255) / 256;
    if (blocks > 262144) blocks = 262144;  // (the kernel strides over the rest)
    hipLaunchKernelGGL(k_rows_to_f32<T>, dim3((unsigned)blocks), dim3(256), 0, st, (const T *)src, dst, plan, dst_vec);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

// (n, d) rows of `dtype` at src -> float32 at dst (both on the current device), then dot's normalisation when asked for
int nnd_launch_rows_f32(hipStream_t st, const void *src, int dtype, int64_t n, int d, bool normalize, float *dst) {
    const int64_t count = n * (int64_t)d;
    int rc = 1;
    switch (dtype) {
        case NND_DTYPE_FLOAT32:
            if ((const void *)dst == src) rc = 0;
            else rc = rows_launch<float>(st, src, count, dst);
            break;
        case NND_DTYPE_FLOAT16: rc = rows_launch<conv_f16>(st, src, count, dst); break;
        case NND_DTYPE_BFLOAT16: rc = rows_launch<conv_bf16>(st, src, count, dst); break;
        case NND_DTYPE_FLOAT64: rc = rows_launch<double>(st, src, count, dst); break;
        default: return 1;
    }
    if (rc) return 1;
    if (normalize && n > 0 && d > 0) {
        hipLaunchKernelGGL(k_normalize_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, dst, n, d);
        if (hipGetLastError() != hipSuccess) return 1;
    }
    return 0;
}

// ---- gather: dst row i = float32 of src row order[i], in rows of dp >= d floats with zero fill (the searcher's layout) ----
// 2^lpr_log2 lanes share a row (a whole wave for 256 floats and more, part of one below: 32 lanes at d = 128); a lane takes
// every 2^lpr_log2-th chunk of the row.  VECSRC (d a multiple of the type's vector, base aligned): one aligned vector load of the
// source per chunk, 16 bytes for float32 / binary16 / bfloat16; otherwise up to four element loads, the columns past d read as
// zero.  The destination's 16-byte chunks are always aligned (dp is a multiple of 4 floats) and stored whole.  An entry of
// `order` outside [0, n) (a caller's error) leaves its row unwritten: nothing is read out of bounds.
template <typename T, bool VECSRC>
__global__ __launch_bounds__(256) void k_gather_rows(const T *__restrict__ src, const int32_t *__restrict__ order, int64_t n, int d, int dp,
                                                     int lpr_log2, float *__restrict__ dst) {
    typedef conv_traits<T> tr;
    constexpr int CH = VECSRC ? tr::VEC : 4;
    const int lpr = 1 << lpr_log2, sub = (int)threadIdx.x & (lpr - 1);
    const int64_t step = (int64_t)gridDim.x * (256 >> lpr_log2);
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lpr_log2; i < n; i += step) {
        const int64_t r = order ? (int64_t)order[i] : i;
        if (r < 0 || r >= n) continue;
        const T *s = src + r * d;
        float *o = dst + i * dp;
        for (int c = sub; c * CH < dp; c += lpr) {
            float v[CH];
            if constexpr (VECSRC) {
                tr::many(*(const typename tr::vec_t *)(s + c * CH), v);
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) v[q] = c * 4 + q < d ? tr::one(s[c * 4 + q]) : 0.0f;
            }
#pragma unroll
            for (int q = 0; q < CH; q += 4) *(float4 *)(o + c * CH + q) = make_float4(v[q], v[q + 1], v[q + 2], v[q + 3]);
        }
    }
}
template <typename T>
static int gather_launch(hipStream_t st, const void *src, const int32_t *order, int64_t n, int d, int dp, float *dst) {
    typedef conv_traits<T> tr;
    const bool vec = d % tr::VEC == 0 && ((uintptr_t)src & 15) == 0;  // (then dp == d: every vector is 4 or 8 floats)
    const int chunks = vec ? d / tr::VEC : dp / 4;
    int lpr_log2 = 0;
    while (lpr_log2 < 6 && (1 << lpr_log2) < chunks) lpr_log2++;
    const int64_t rows_per_block = 256 >> lpr_log2;
    int64_t blocks = (n + rows_per_block - 1) / rows_per_block;
    if (blocks > 8192) blocks = 8192;  // (the kernel strides over the rest)
    if (vec) hipLaunchKernelGGL((k_gather_rows<T, true>), dim3((unsigned)blocks), dim3(256), 0, st, (const T *)src, order, n, d, dp, lpr_log2, dst);
    else hipLaunchKernelGGL((k_gather_rows<T, false>), dim3((unsigned)blocks), dim3(256), 0, st, (const T *)src, order, n, d, dp, lpr_log2, dst);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
int nnd_launch_gather_rows(hipStream_t st, const void *src, int dtype, const int32_t *order, int64_t n, int d, int dp, float *dst) {
    if (n <= 0 || d <= 0) return 0;
    if (dp < d || (dp & 3) || ((uintptr_t)dst & 15)) return 1;
    switch (dtype) {
        case NND_DTYPE_FLOAT32: return gather_launch<float>(st, src, order, n, d, dp, dst);
        case NND_DTYPE_FLOAT16: return gather_launch<conv_f16>(st, src, order, n, d, dp, dst);
        case NND_DTYPE_BFLOAT16: return gather_launch<conv_bf16>(st, src, order, n, d, dp, dst);
        case NND_DTYPE_FLOAT64: return gather_launch<double>(st, src, order, n, d, dp, dst);
        default: return 1;
    }
}

// ---- update(): the grown point set assembled on the device (NNDescent.update of a device-built index) ----
// The new (n_old + n_fresh, d) tensor takes the old rows, the fresh rows behind them and the updated rows at their ids.  When
// every array has the tensor's own type nothing is converted: the elements move as words of their size (k_rows_copy, with the
// work split of k_rows_to_f32: aligned 16-byte loads of the source, 16-byte stores when the destination is aligned as well).
// Otherwise the tensor is float32 and the rows go through k_rows_to_f32.
template <typename U>
__global__ __launch_bounds__(256) void k_rows_copy(const U *__restrict__ src, U *__restrict__ dst, nnd_conv_plan plan, int dst_vec) {
    constexpr int VEC = 16 / (int)sizeof(U);
    const int64_t items = nnd_conv_items(plan);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t first;
        const int len = nnd_conv_item(plan, i, &first);
        if (len == 1) {
            dst[first] = src[first];
            continue;
        }
        union { uint4 v; U e[VEC]; } w;
        w.v = *(const uint4 *)(src + first);
        if (dst_vec) {
            *(uint4 *)(dst + first) = w.v;
        } else {
#pragma unroll
            for (int c = 0; c < VEC; c++) dst[first + c] = w.e[c];
        }
    }
}
template <typename U>
static int copy_launch(hipStream_t st, const void *src, int64_t count, void *dst) {
    const nnd_conv_plan plan = nnd_conv_make_plan((uint64_t)(uintptr_t)src, (int)sizeof(U), 16 / (int)sizeof(U), count);
    const int64_t items = nnd_conv_items(plan);
    if (items <= 0) return 0;
    const int dst_vec = (((uintptr_t)dst + sizeof(U) * (size_t)plan.head) & 15) == 0 ? 1 : 0;
    int64_t blocks = (items + 255) / 256;
    if (blocks > 262144) blocks = 262144;  // (the kernel strides over the rest)
    hipLaunchKernelGGL(k_rows_copy<U>, dim3((unsigned)blocks), dim3(256), 0, st, (const U *)src, (U *)dst, plan, dst_vec);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
static size_t dtype_size(int dtype) { return dtype == NND_DTYPE_FLOAT64 ? 8 : dtype == NND_DTYPE_FLOAT32 ? 4 : 2; }
// `count` elements of `dtype` at src -> dst: as they are when out_dtype is the same type, as float32 otherwise
static int rows_into(hipStream_t st, const void *src, int dtype, int64_t count, void *dst, int out_dtype) {
    if (count <= 0) return 0;
    if (dtype != out_dtype) return nnd_launch_rows_f32(st, src, dtype, count, 1, false, (float *)dst);
    switch (dtype_size(dtype)) {
        case 2: return copy_launch<uint16_t>(st, src, count, dst);
        case 4: return copy_launch<uint32_t>(st, src, count, dst);
        default: return copy_launch<uint64_t>(st, src, count, dst);
    }
}

// The typed row scatter: row ids[i] of dst = row rows[i] of src, 2^lpr_log2 lanes per pair, a lane every 2^lpr_log2-th element.
// The pairs' ids are distinct (the host resolves duplicates: the last one wins there), so no two groups write one row; a pair
// that names a row outside either array (a caller's error) is skipped: nothing is read or written out of bounds.
// RAW: both arrays hold the same type, moved as words of its size (T == OUT: uint16_t / uint32_t / uint64_t)
template <typename T, typename OUT, bool RAW>
__global__ __launch_bounds__(256) void k_scatter_rows(const T *__restrict__ src, int64_t n_src, const int32_t *__restrict__ rows, const int32_t *__restrict__ ids,
                                                      int64_t n_pairs, int d, int lpr_log2, OUT *__restrict__ dst, int64_t n_dst) {
    const int lpr = 1 << lpr_log2, sub = (int)threadIdx.x & (lpr - 1);
    const int64_t step = (int64_t)gridDim.x * (256 >> lpr_log2);
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lpr_log2; i < n_pairs; i += step) {
        const int64_t s = rows[i], r = ids[i];
        if (s < 0 || s >= n_src || r < 0 || r >= n_dst) continue;
        const T *from = src + s * d;
        OUT *to = dst + r * d;
        for (int c = sub; c < d; c += lpr) {
            if constexpr (RAW) to[c] = from[c];
            else to[c] = conv_traits<T>::one(from[c]);
        }
    }
}
template <typename T, typename OUT, bool RAW>
static int scatter_launch(hipStream_t st, const void *src, int64_t n_src, const int32_t *rows, const int32_t *ids, int64_t n_pairs, int d, void *dst,
                          int64_t n_dst) {
    int lpr_log2 = 0;
    while (lpr_log2 < 6 && (1 << lpr_log2) < d) lpr_log2++;
    const int64_t per_block = 256 >> lpr_log2;
    int64_t blocks = (n_pairs + per_block - 1) / per_block;
    if (blocks > 8192) blocks = 8192;  // (the kernel strides over the rest)
    hipLaunchKernelGGL((k_scatter_rows<T, OUT, RAW>), dim3((unsigned)blocks), dim3(256), 0, st, (const T *)src, n_src, rows, ids, n_pairs, d, lpr_log2, (OUT *)dst,
                       n_dst);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}
static int scatter_into(hipStream_t st, const void *src, int dtype, int64_t n_src, const int32_t *rows, const int32_t *ids, int64_t n_pairs, int d, void *dst,
                        int out_dtype, int64_t n_dst) {
    if (n_pairs <= 0) return 0;
    if (dtype == out_dtype) {
        switch (dtype_size(dtype)) {
            case 2: return scatter_launch<uint16_t, uint16_t, true>(st, src, n_src, rows, ids, n_pairs, d, dst, n_dst);
            case 4: return scatter_launch<uint32_t, uint32_t, true>(st, src, n_src, rows, ids, n_pairs, d, dst, n_dst);
            default: return scatter_launch<uint64_t, uint64_t, true>(st, src, n_src, rows, ids, n_pairs, d, dst, n_dst);
        }
    }
    switch (dtype) {
        case NND_DTYPE_FLOAT32: return scatter_launch<float, float, false>(st, src, n_src, rows, ids, n_pairs, d, dst, n_dst);
        case NND_DTYPE_FLOAT16: return scatter_launch<conv_f16, float, false>(st, src, n_src, rows, ids, n_pairs, d, dst, n_dst);
        case NND_DTYPE_BFLOAT16: return scatter_launch<conv_bf16, float, false>(st, src, n_src, rows, ids, n_pairs, d, dst, n_dst);
        default: return scatter_launch<double, float, false>(st, src, n_src, rows, ids, n_pairs, d, dst, n_dst);
    }
}

// ---- corrections ----
template <int KIND, typename OUT>
__global__ __launch_bounds__(256) void k_correct(const float *__restrict__ in, OUT *__restrict__ out, int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = in[i];
        if (KIND == NND_CORRECT_SQRT) out[i] = (OUT)sqrt_rn_f32(d);
        else if (KIND == NND_CORRECT_ALT_COSINE) out[i] = (OUT)(1.0 - exp2(-(double)d));
        else if (KIND == NND_CORRECT_ALT_INNER_PRODUCT) out[i] = (OUT)(d >= FLT_MAX ? 0.0 : __ddiv_rn(-1.0, (double)d));
        else if (KIND == NND_CORRECT_HAVERSINE) out[i] = (OUT)(2.0 * asin(fmin(1.0, __dsqrt_rn((double)d) * 0.5)));
        else out[i] = (OUT)__dsqrt_rn(1.0 - exp2(-(double)d));
    }
}
// the copy moves words, not floats: every bit pattern (the ids of a graph as well) arrives as it left
__global__ __launch_bounds__(256) void k_copy_words(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, int64_t count) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) out[i] = in[i];
}

static thread_local char g_daerr[256] = {0};
void nnd_set_global_error(const char *msg);  // handle.hip: what nnd_last_global_error returns

static int da_fail(const char *msg) {
    snprintf(g_daerr, sizeof(g_daerr), "%s", msg);
    nnd_set_global_error(g_daerr);
    return 1;
}

extern "C" int32_t nnd_device_rows_f32(int32_t device, void *hip_stream, const void *src_dev, int32_t dtype, int64_t n, int32_t dim,
                                       int32_t normalize, float *dst_dev) {
    if (n < 0 || dim < 0 || dtype < NND_DTYPE_FLOAT32 || dtype > NND_DTYPE_FLOAT64) return da_fail("nnd_device_rows_f32: bad shape or dtype");
    if (n == 0 || dim == 0) return 0;
    if (!src_dev || !dst_dev) return da_fail("nnd_device_rows_f32: null pointer");
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return da_fail("nnd_device_rows_f32: no such device"); }
    if (nnd_launch_rows_f32((hipStream_t)hip_stream, src_dev, dtype, n, dim, normalize != 0, dst_dev)) {
        (void)hipGetLastError();
        return da_fail("nnd_device_rows_f32: kernel launch failed");
    }
    return 0;
}

extern "C" int32_t nnd_device_correct(int32_t device, void *hip_stream, int32_t kind, const float *in_dev, void *out_dev, int64_t count) {
    if (count < 0 || kind < NND_CORRECT_COPY || kind > NND_CORRECT_HAVERSINE) return da_fail("nnd_device_correct: bad kind or count");
    if (count == 0) return 0;
    if (!in_dev || !out_dev) return da_fail("nnd_device_correct: null pointer");
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return da_fail("nnd_device_correct: no such device"); }
    hipStream_t st = (hipStream_t)hip_stream;
    int64_t blocks = (count + 255) / 256;
    if (blocks > 262144) blocks = 262144;
    const dim3 g((unsigned)blocks), b(256);
    switch (kind) {
        case NND_CORRECT_COPY: hipLaunchKernelGGL(k_copy_words, g, b, 0, st, (const uint32_t *)in_dev, (uint32_t *)out_dev, count); break;
        case NND_CORRECT_SQRT: hipLaunchKernelGGL((k_correct<NND_CORRECT_SQRT, float>), g, b, 0, st, in_dev, (float *)out_dev, count); break;
        case NND_CORRECT_ALT_COSINE: hipLaunchKernelGGL((k_correct<NND_CORRECT_ALT_COSINE, double>), g, b, 0, st, in_dev, (double *)out_dev, count); break;
        case NND_CORRECT_ALT_INNER_PRODUCT: hipLaunchKernelGGL((k_correct<NND_CORRECT_ALT_INNER_PRODUCT, double>), g, b, 0, st, in_dev, (double *)out_dev, count); break;
        case NND_CORRECT_HAVERSINE: hipLaunchKernelGGL((k_correct<NND_CORRECT_HAVERSINE, double>), g, b, 0, st, in_dev, (double *)out_dev, count); break;
        default: hipLaunchKernelGGL((k_correct<NND_CORRECT_ALT_HELLINGER, double>), g, b, 0, st, in_dev, (double *)out_dev, count); break;
    }
    if (hipGetLastError() != hipSuccess) return da_fail("nnd_device_correct: kernel launch failed");
    return 0;
}

static bool dtype_ok(int32_t t) { return t >= NND_DTYPE_FLOAT32 && t <= NND_DTYPE_FLOAT64; }

extern "C" int32_t nnd_device_update_rows(int32_t device, void *hip_stream, int32_t dim, const void *old_dev, int32_t old_dtype, int64_t n_old,
                                          const void *fresh_dev, int32_t fresh_dtype, int64_t n_fresh, const void *upd_dev, int32_t upd_dtype,
                                          int64_t n_upd, const int32_t *upd_rows_dev, const int32_t *upd_ids_dev, int64_t n_pairs, void *out_dev,
                                          int32_t out_dtype) {
    if (dim < 1 || n_old < 0 || n_fresh < 0 || n_upd < 0 || n_pairs < 0 || !dtype_ok(out_dtype)) return da_fail("nnd_device_update_rows: bad shape or dtype");
    const bool has_old = n_old > 0, has_fresh = n_fresh > 0, has_upd = n_pairs > 0;
    if ((has_old && !dtype_ok(old_dtype)) || (has_fresh && !dtype_ok(fresh_dtype)) || (has_upd && !dtype_ok(upd_dtype)))
        return da_fail("nnd_device_update_rows: bad shape or dtype");
    // the dtype rule: one shared type is kept, anything else meets in float32
    if (out_dtype != NND_DTYPE_FLOAT32 && ((has_old && old_dtype != out_dtype) || (has_fresh && fresh_dtype != out_dtype) || (has_upd && upd_dtype != out_dtype)))
        return da_fail("nnd_device_update_rows: arrays of different types are assembled as float32");
    if ((has_old && !old_dev) || (has_fresh && !fresh_dev) || (has_upd && (!upd_dev || !upd_rows_dev || !upd_ids_dev)) || ((has_old || has_fresh) && !out_dev))
        return da_fail("nnd_device_update_rows: null pointer");
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return da_fail("nnd_device_update_rows: no such device"); }
    hipStream_t st = (hipStream_t)hip_stream;
    char *out = (char *)out_dev;
    const size_t esz = dtype_size(out_dtype);
    if (rows_into(st, old_dev, old_dtype, n_old * (int64_t)dim, out, out_dtype) ||
        rows_into(st, fresh_dev, fresh_dtype, n_fresh * (int64_t)dim, out + esz * (size_t)n_old * dim, out_dtype) ||
        scatter_into(st, upd_dev, upd_dtype, n_upd, upd_rows_dev, upd_ids_dev, n_pairs, dim, out, out_dtype, n_old)) {
        (void)hipGetLastError();
        return da_fail("nnd_device_update_rows: kernel launch failed");
    }
    return 0;
}
