// linear.hip -- the fixed linear map of the metrics that are squared euclidean distance after one: seuclidean
// (D = diag(V^-1/2)), wminkowski with p = 2 (D = diag(sqrt w)) and mahalanobis (any A with A^T A = sym(VI)).
//     k_linear_rows:  Y[i, :] = A (X[i, :] - c)
// float32 rows of stride d in, float32 rows of stride d out; c is a shift near the data (the column mean of a sample of the
// training rows, fixed when the index is built), so that A never sees the data's offset -- the reason k_prep_rows centres the
// rows of metric code 0.  Everything behind this kernel runs code 0 on Y unchanged (metric.h, DESIGN.md "Metrics").
//
// The contract: a row's result depends on that row alone -- not on n, on the row's place in a tile, on its neighbours in the
// launch, or on the run.  Dense form: every output element is one chain of v_mfma_f32_16x16x4_f32 steps (an fmaf chain, one
// rounding per product) over the K blocks in ascending order, the k's of a block in the fixed order of the operand map
// below, padded k's contributing fma(0, 0, acc) = acc; the lane a row lands on changes which register holds the chain, not
// the chain.  Diagonal form: one subtraction and one multiplication per element.  So duplicate rows stay duplicates (their
// distance is exactly 0), and a row transformed alone equals the row transformed inside any batch.
//
// Error of the dense form against exact arithmetic on the float32 operands, componentwise:
//     |Y~_j - Y_j| <= (d + 2) u sum_k |A_jk| |x_k - c_k| + O(u^2),   u = 2^-24
// (one rounding of x_k - c_k, one per product-and-add of a chain of at most d + 1 steps).
//
// Dense layout: a workgroup of four waves takes 64 rows (16 per wave) and walks the output columns in chunks of 128 (eight
// 16 x 16 accumulator tiles per wave); per chunk it walks K in blocks of 32: the 64 x 32 block of X - c and the 128 x 32 block
// of A are staged in LDS (27 KB together, padding included -- A is never required to fit whole, d is unbounded), and every
// wave runs 8 x 8 MFMA steps on them.  Columns at or beyond d are never read: of X, of c, or of A (d need not be a multiple of anything).  Bytes
// moved: X once per column chunk (once for d <= 128), Y once, A once per workgroup from L2.
#include <stdarg.h>
#include <stdio.h>

#include "common.h"
#include "devmem.h"
#include "state.h"

#define LIN_ROWS 64    // rows of a workgroup
#define LIN_JC 128     // output columns of a chunk: 8 accumulator tiles per wave
#define LIN_KB 32      // K block
#define LIN_LD 36      // LDS row stride in floats: the block and one 16-byte chunk of padding

// Stage `rows` x LIN_KB floats of a row-major (n_rows, d) matrix, rows r0.., columns k0.., into dst (stride LIN_LD), minus
// shift[k] when `shift` is given.  Rows at or beyond n_rows and columns at or beyond d are zeros and are not read.
template <bool VEC>
__device__ __forceinline__ void lin_stage(const float *__restrict__ src, int64_t n_rows, int d, int64_t r0, int k0, int rows,
                                          const float *__restrict__ shift, float *dst, int tid) {
    const int total = rows * (LIN_KB / 4);
    for (int idx = tid; idx < total; idx += 256) {
        const int r = idx >> 3, ch = idx & 7;
        const int64_t row = r0 + r;
        const int k = k0 + 4 * ch;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (row < n_rows) {
            const float *p = src + row * (int64_t)d + k;
            if (VEC) {  // d % 4 == 0 and a 16-byte aligned base: a chunk is inside the row or outside it, whole
                if (k < d) {
                    const float4 x = *(const float4 *)p;
                    v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
                    if (shift) {
                        const float4 s = *(const float4 *)(shift + k);
                        v[0] -= s.x; v[1] -= s.y; v[2] -= s.z; v[3] -= s.w;
                    }
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    if (k + q < d) v[q] = shift ? p[q] - shift[k + q] : p[q];
            }
        }
        *(float4 *)&dst[r * LIN_LD + 4 * ch] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// Operand map of a K block (gram.h's): lane l holds row (or column) l & 15 and the 16-byte chunk 4 t + (l >> 4) of it; the
// chunk's four floats feed four consecutive MFMA steps, so step s of group t sums k = 16 t + 4 g + s over g = 0..3.
template <bool VEC>
__global__ __launch_bounds__(256) void k_linear_rows(const float *__restrict__ x, const float *__restrict__ a, const float *__restrict__ shift,
                                                     int64_t n, int d, float *__restrict__ y) {
    __shared__ __attribute__((aligned(16))) float Xs[LIN_ROWS * LIN_LD];
    __shared__ __attribute__((aligned(16))) float As[LIN_JC * LIN_LD];
    const int tid = (int)threadIdx.x, lane = nnd_lane(), wave = tid >> 6;
    const int r16 = lane & 15, g = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * LIN_ROWS;
    for (int jc = 0; jc < d; jc += LIN_JC) {
        const int ntiles = min(LIN_JC, d - jc + 15) >> 4;  // tiles of this chunk that hold a column below d (block-uniform)
        f32x4 acc[LIN_JC / 16];
#pragma unroll
        for (int J = 0; J < LIN_JC / 16; J++) acc[J] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < d; k0 += LIN_KB) {
            lin_stage<VEC>(x, n, d, r0, k0, LIN_ROWS, shift, Xs, tid);
            lin_stage<VEC>(a, (int64_t)d, d, (int64_t)jc, k0, ntiles * 16, nullptr, As, tid);
            __syncthreads();
#pragma unroll
            for (int t = 0; t < LIN_KB / 16; t++) {
                const float4 xa = *(const float4 *)&Xs[(wave * 16 + r16) * LIN_LD + 16 * t + 4 * g];
#pragma unroll
                for (int J = 0; J < LIN_JC / 16; J++) {
                    if (J < ntiles) {
                        const float4 b = *(const float4 *)&As[(J * 16 + r16) * LIN_LD + 16 * t + 4 * g];
                        acc[J] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.x, b.x, acc[J], 0, 0, 0);
                        acc[J] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.y, b.y, acc[J], 0, 0, 0);
                        acc[J] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.z, b.z, acc[J], 0, 0, 0);
                        acc[J] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.w, b.w, acc[J], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
        // D[row = 4 (l >> 4) + r][col = l & 15] in register r
#pragma unroll
        for (int J = 0; J < LIN_JC / 16; J++) {
            const int col = jc + J * 16 + r16;
            if (J < ntiles && col < d) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int64_t row = r0 + wave * 16 + 4 * g + r;
                    if (row < n) y[row * (int64_t)d + col] = acc[J][r];
                }
            }
        }
    }
}

// Diagonal form: y = (x - c) * s per element; no matrix code in this instance.  VEC: d % 4 == 0 and 16-byte aligned bases.
template <bool VEC>
__global__ __launch_bounds__(256) void k_linear_rows_diag(const float *__restrict__ x, const float *__restrict__ s, const float *__restrict__ shift,
                                                          int64_t n, int d, float *__restrict__ y) {
#pragma clang fp contract(off)
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    if (VEC) {
        const int dv = d >> 2;
        const int64_t items = n * (int64_t)dv;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += step) {
            const int j = (int)(i % dv) * 4;
            const float4 v = *(const float4 *)(x + 4 * i), c = *(const float4 *)(shift + j), w = *(const float4 *)(s + j);
            *(float4 *)(y + 4 * i) = make_float4((v.x - c.x) * w.x, (v.y - c.y) * w.y, (v.z - c.z) * w.z, (v.w - c.w) * w.w);
        }
    } else {
        const int64_t items = n * (int64_t)d;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < items; i += step) {
            const int j = (int)(i % d);
            y[i] = (x[i] - shift[j]) * s[j];
        }
    }
}

// (n, d) float32 rows at x -> y, all on the current device, queued on `st`.  kind: NND_LINEAR_DIAGONAL (map: d floats) or
// NND_LINEAR_DENSE (map: (d, d) row-major, y_j = sum_k map[j, k] (x_k - shift_k)).
int nnd_launch_linear_rows(hipStream_t st, int kind, const float *map, const float *shift, const float *x, int64_t n, int d, float *y) {
    if (n <= 0 || d <= 0) return 0;
    const bool vec = (d & 3) == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)map | (uintptr_t)shift) & 15) == 0;
    if (kind == NND_LINEAR_DIAGONAL) {
        int64_t blocks = (n * (int64_t)d / (vec ? 4 : 1) + 255) / 256;
        if (blocks > 65536) blocks = 65536;  // (the kernel strides over the rest)
        if (vec) hipLaunchKernelGGL(k_linear_rows_diag<true>, dim3((unsigned)blocks), dim3(256), 0, st, x, map, shift, n, d, y);
        else hipLaunchKernelGGL(k_linear_rows_diag<false>, dim3((unsigned)blocks), dim3(256), 0, st, x, map, shift, n, d, y);
    } else if (kind == NND_LINEAR_DENSE) {
        const int64_t blocks = (n + LIN_ROWS - 1) / LIN_ROWS;
        if (blocks > (int64_t)0x7FFFFFFF) return 1;
        if (vec) hipLaunchKernelGGL(k_linear_rows<true>, dim3((unsigned)blocks), dim3(256), 0, st, x, map, shift, n, d, y);
        else hipLaunchKernelGGL(k_linear_rows<false>, dim3((unsigned)blocks), dim3(256), 0, st, x, map, shift, n, d, y);
    } else {
        return 1;
    }
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

namespace {
struct lin_err {  // the error sink of an entry without a handle: what nnd_last_global_error returns
    char msg[256];
    void set_error(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg, sizeof(msg), fmt, ap);
        va_end(ap);
        nnd_set_global_error(msg);
    }
};
bool lin_args_ok(lin_err &err, const char *who, int32_t kind, int32_t dim, int64_t n, const void *map, const void *shift, const void *x, const void *y) {
    if ((kind != NND_LINEAR_DIAGONAL && kind != NND_LINEAR_DENSE) || dim < 1 || n < 0 || dim > 46340) { err.set_error("%s: bad kind or shape", who); return false; }
    if (!map || !shift || (n > 0 && (!x || !y))) { err.set_error("%s: null pointer", who); return false; }
    return true;
}
}  // namespace

extern "C" int32_t nnd_device_linear_rows(int32_t device, void *hip_stream, int32_t kind, int32_t dim, const float *map_dev, const float *shift_dev,
                                          const float *x_dev, int64_t n, float *y_dev) {
    lin_err err;
    if (!lin_args_ok(err, "nnd_device_linear_rows", kind, dim, n, map_dev, shift_dev, x_dev, y_dev)) return 1;
    if (n == 0) return 0;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_device_linear_rows: no such device"); return 1; }
    if (nnd_launch_linear_rows((hipStream_t)hip_stream, kind, map_dev, shift_dev, x_dev, n, dim, y_dev)) {
        (void)hipGetLastError();
        err.set_error("nnd_device_linear_rows: kernel launch failed");
        return 1;
    }
    return 0;
}

extern "C" int32_t nnd_linear_rows_host(int32_t device, int32_t kind, int32_t dim, const float *map, const float *shift, const float *x, int64_t n,
                                        float *y) {
    lin_err err;
    if (!lin_args_ok(err, "nnd_linear_rows_host", kind, dim, n, map, shift, x, y)) return 1;
    if (n == 0) return 0;
    if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_linear_rows_host: no HIP device %d", (int)device); return 1; }
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_linear_rows_host: no stream"); return 1; }
    const size_t map_count = kind == NND_LINEAR_DENSE ? (size_t)dim * dim : (size_t)dim, count = (size_t)n * dim;
    int rc = 1;
    {
        nnd_scratch tmp;
        do {
            float *d_map = tmp.get<float>(&err, map_count), *d_shift = tmp.get<float>(&err, (size_t)dim);
            float *d_x = tmp.get<float>(&err, count), *d_y = tmp.get<float>(&err, count);
            if (!d_map || !d_shift || !d_x || !d_y) break;
            bool ok = hipMemcpyAsync(d_map, map, sizeof(float) * map_count, hipMemcpyHostToDevice, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(d_shift, shift, sizeof(float) * (size_t)dim, hipMemcpyHostToDevice, st) == hipSuccess;
            ok = ok && hipMemcpyAsync(d_x, x, sizeof(float) * count, hipMemcpyHostToDevice, st) == hipSuccess;
            if (!ok) { (void)hipGetLastError(); err.set_error("nnd_linear_rows_host: host-to-device copy failed"); break; }
            if (nnd_launch_linear_rows(st, kind, d_map, d_shift, d_x, n, dim, d_y)) { (void)hipGetLastError(); err.set_error("nnd_linear_rows_host: kernel launch failed"); break; }
            if (hipMemcpyAsync(y, d_y, sizeof(float) * count, hipMemcpyDeviceToHost, st) != hipSuccess) {
                (void)hipGetLastError();
                err.set_error("nnd_linear_rows_host: device-to-host copy failed");
                break;
            }
            rc = 0;
        } while (0);
        const hipError_t e = hipStreamSynchronize(st);  // before the scratch goes
        if (!rc && e != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_linear_rows_host: kernel or copy failed: %s", hipGetErrorString(e)); rc = 1; }
    }
    (void)hipStreamDestroy(st);
    return rc;
}
