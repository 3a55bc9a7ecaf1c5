// fuzzy.hip -- UMAP's fuzzy simplicial set from k-lists on the device: smooth_knn_dist (a bisection per row for sigma, a
// selection for rho), compute_membership_strengths, and the fuzzy union with the transpose.  DESIGN.md section 4 "Fuzzy
// simplicial set".
//
//   k_fuzzy_mean -> k_fuzzy_mean_sum      the mean of all non-empty distances (the floor of a row whose rho is 0), float64
//   k_smooth_knn<KU, W, IdT>              rho, sigma and the weight of every place; a place that is not stored gets id -1
//   csr_build_i32 (csr_graph.hip)         the two (m, k) buffers to canonical CSR: directed as they are, or the fuzzy union
//
// A row is its k places (id, d); a place whose id is outside [0, n) is empty and adds nothing to a sum, a mean or the matrix.
// Place 0 is left out of the bisection's sums (UMAP's loops start at 1); rho and the means see every place.
//
// k_smooth_knn has csr_wave_sort's split: a row of at most 16, 32 or 64 places is held by W = 16, 32 or 64 lanes, one place a
// lane, so a wave solves 64 / W rows at once; 65..256 places take the wave with KU = 2 or 4 places per lane.  The distances
// are read once and stay in registers for the 64 rounds.  A round is one v_exp_f32 per place, one reciprocal, a sum over the
// group and the compare: x = (d - rho) * log2(e) is formed once per row (0 where d - rho <= 0: 2^-0 is the 1 such a place
// adds; +inf where the place does not count: 2^-inf is 0), so there is no select in the loop.
//
// Determinism: the group sum is four DPP row rotations by 8, 4, 2, 1 -- after a rotation by half the period both partners
// have added the same two floats, so all 16 lanes of a row hold the same bits -- and, for W > 16, the row sums fetched with
// v_readlane and added in one fixed order.  lo, mid and hi are therefore the same in every lane of a group with no broadcast,
// and a row's result does not depend on which rows share its wave.  No LDS, no barrier, no atomic; k_fuzzy_mean adds float64
// partials in a fixed order and uses no floating-point atomic either.  Every store is a vector store.
#include <math.h>
#include <string.h>

#include "../../include/pynnd_amd.h"
#include "common.h"
#include "csr_graph.h"

#define FZ_ROUNDS 64
#define FZ_TOLERANCE 1e-5f  // SMOOTH_K_TOLERANCE
#define FZ_MIN_SCALE 1e-3   // MIN_K_DIST_SCALE
#define FZ_LOG2E 1.4426950408889634f
#define FZ_MEAN_BLOCKS 512  // the most partials k_fuzzy_mean leaves

// the id of a place when it names a column, else -1
template <typename IdT>
__device__ __forceinline__ int32_t fz_col(const IdT *__restrict__ ids, int64_t at, int64_t n) {
    const int64_t j = (int64_t)ids[at];
    return (j >= 0 && j < n) ? (int32_t)j : -1;
}

// ---------------------------------------------------------------------------------------------- the mean of all distances
// One (sum, count) per workgroup: a thread adds its places in index order, a wave its lanes by a fixed tree, thread 0 the
// four waves in order.  The grid depends on the shape alone, so the partials are the same bits on every run.
template <typename IdT>
__global__ __launch_bounds__(256) void k_fuzzy_mean(const IdT *__restrict__ ids, const float *__restrict__ dists, int64_t m, int32_t k, int64_t ld,
                                                    int64_t n, double *__restrict__ part_sum, unsigned long long *__restrict__ part_cnt) {
    __shared__ double s_sum[4];
    __shared__ unsigned long long s_cnt[4];
    const int64_t total = m * (int64_t)k;
    double s = 0.0;
    unsigned long long c = 0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t row = t / k, at = row * ld + (t - row * k);
        if (fz_col(ids, at, n) >= 0) { s += (double)dists[at]; c++; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o, 64); c += __shfl_down(c, o, 64); }
    if (nnd_lane() == 0) { s_sum[threadIdx.x >> 6] = s; s_cnt[threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_sum[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        part_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    }
}
// one wave adds the partials: a lane its own in index order, then the same tree
__global__ __launch_bounds__(64) void k_fuzzy_mean_sum(const double *__restrict__ part_sum, const unsigned long long *__restrict__ part_cnt, int parts,
                                                       double *__restrict__ mean) {
    double s = 0.0;
    unsigned long long c = 0;
    for (int i = nnd_lane(); i < parts; i += 64) { s += part_sum[i]; c += part_cnt[i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o, 64); c += __shfl_down(c, o, 64); }
    if (nnd_lane() == 0) *mean = c ? s / (double)c : 0.0;
}

// ---------------------------------------------------------------------------------------------- sigma, rho and the weights
// The sum of v over the W lanes of this lane's group, the same bits in each of them (every lane of the wave is active).
template <int W>
__device__ __forceinline__ float fz_group_sum(float v) {
    v += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(8)>(__float_as_int(v)));
    v += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(4)>(__float_as_int(v)));
    v += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(2)>(__float_as_int(v)));
    v += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(1)>(__float_as_int(v)));
    if constexpr (W == 16) return v;
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    if constexpr (W == 32) return nnd_lane() < 32 ? r0 + r1 : r2 + r3;
    return (r0 + r1) + (r2 + r3);
}
// the bits of a ballot that belong to this lane's group, moved down to bit 0
template <int W>
__device__ __forceinline__ unsigned long long fz_group_bits(unsigned long long mask) {
    if constexpr (W == 64) return mask;
    return (mask >> (nnd_lane() & ~(W - 1))) & ((1ull << W) - 1ull);
}
// nz[idx - 1] + t * (nz[idx] - nz[idx - 1]) as UMAP writes it, one float32 operation after the other
__device__ __forceinline__ float fz_interpolate(float a, float b, float t) {
#pragma clang fp contract(off)
    return a + t * (b - a);
}

template <int KU, int W, typename IdT>
__global__ __launch_bounds__(256) void k_smooth_knn(const IdT *__restrict__ ids, const float *__restrict__ dists, int64_t m, int32_t k, int64_t ld,
                                                    int64_t n, float local_connectivity, float target, const double *__restrict__ mean_all,
                                                    float *__restrict__ sigmas, float *__restrict__ rhos, int32_t *__restrict__ cols,
                                                    float *__restrict__ weights) {
    static_assert(W == 64 || KU == 1, "several places per lane: the whole wave is one row");
    constexpr int R = 64 / W;  // rows of a wave
    const int lane = nnd_lane(), sub = lane & (W - 1), group = lane / W;
    const int lc_idx = (int)floorf(local_connectivity);
    const float lc_t = local_connectivity - (float)lc_idx;
    const unsigned long long below = (1ull << sub) - 1ull;  // the lanes of the group in front of this one
    for (int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R; first < m; first += (int64_t)gridDim.x * 4 * R) {  // wave-uniform
        const int64_t row = first + group;
        const bool live = row < m;
        float d[KU];
        int32_t col[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int e = u * 64 + sub;
            col[u] = -1;
            d[u] = 0.0f;
            if (live && e < k) {
                col[u] = fz_col(ids, row * ld + e, n);
                if (col[u] >= 0) d[u] = dists[row * ld + e];
            }
        }
        // ---- rho: the positive distances in row order are ranked by ballot and popcount, the two that count fetched by a shuffle
        bool pos[KU];
        int rank[KU], npos = 0, filled = 0;
        float top = 0.0f;
        double row_sum = 0.0;
#pragma unroll
        for (int u = 0; u < KU; u++) {
            pos[u] = col[u] >= 0 && d[u] > 0.0f;
            const unsigned long long g = fz_group_bits<W>(__ballot(pos[u]));
            rank[u] = npos + __popcll(g & below);
            npos += __popcll(g);
            filled += __popcll(fz_group_bits<W>(__ballot(col[u] >= 0)));
            top = fmaxf(top, pos[u] ? d[u] : 0.0f);
            row_sum += (double)d[u];  // (an empty place holds 0)
        }
        float nz_lo = 0.0f, nz_hi = 0.0f;  // nz[lc_idx - 1], nz[lc_idx]; 0 where the row has no such distance
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const unsigned long long g_lo = fz_group_bits<W>(__ballot(pos[u] && rank[u] == lc_idx - 1));
            const unsigned long long g_hi = fz_group_bits<W>(__ballot(pos[u] && rank[u] == lc_idx));
            const float v_lo = __shfl(d[u], group * W + (g_lo ? (int)__builtin_ctzll(g_lo) : 0), 64);
            const float v_hi = __shfl(d[u], group * W + (g_hi ? (int)__builtin_ctzll(g_hi) : 0), 64);
            if (g_lo) nz_lo = v_lo;
            if (g_hi) nz_hi = v_hi;
        }
#pragma unroll
        for (int o = W >> 1; o > 0; o >>= 1) {  // (xor partners: every lane of the group ends with the same bits)
            top = fmaxf(top, __shfl_xor(top, o, 64));
            row_sum += __shfl_xor(row_sum, o, 64);
        }
        float rho;
        if ((float)npos >= local_connectivity) {
            if (lc_idx > 0) rho = lc_t > FZ_TOLERANCE ? fz_interpolate(nz_lo, nz_hi, lc_t) : nz_lo;
            else rho = lc_t * nz_hi;
        } else {
            rho = top;  // (0 for a row without a positive distance)
        }
        // ---- sigma: x = (d - rho) * log2(e); a place adds 2^(-x / mid)
        float x[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const float t = d[u] - rho;
            x[u] = (col[u] >= 0 && u * 64 + sub >= 1) ? (t > 0.0f ? t * FZ_LOG2E : 0.0f) : INFINITY;
        }
        float lo = 0.0f, hi = INFINITY, mid = 1.0f;
        bool done = !live;
        for (int round = 0; round < FZ_ROUNDS; round++) {
            const float inv = -1.0f / mid;
            float s = 0.0f;
#pragma unroll
            for (int u = 0; u < KU; u++) s += __builtin_amdgcn_exp2f(x[u] * inv);
            s = fz_group_sum<W>(s);
            if (!done) {
                if (fabsf(s - target) < FZ_TOLERANCE) {
                    done = true;  // mid is frozen
                } else if (s > target) {
                    hi = mid;
                    mid = (lo + hi) * 0.5f;
                } else {
                    lo = mid;
                    mid = hi == INFINITY ? mid * 2.0f : (lo + hi) * 0.5f;
                }
            }
            if (__ballot(!done) == 0ull) break;  // every group of the wave has stopped
        }
        const double mean = rho > 0.0f ? (filled ? row_sum / (double)filled : 0.0) : *mean_all;
        const float sigma = (float)fmax((double)mid, FZ_MIN_SCALE * mean);
        // ---- the weights; a place that is not stored (empty, the row itself, weight 0) is handed on as an empty place
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int e = u * 64 + sub;
            if (live && e < k) {
                const float t = d[u] - rho;
                float w = 0.0f;
                if (col[u] >= 0 && (int64_t)col[u] != row) w = (t <= 0.0f || sigma == 0.0f) ? 1.0f : __builtin_amdgcn_exp2f(-(t * FZ_LOG2E) / sigma);
                weights[row * k + e] = w;
                cols[row * k + e] = w != 0.0f ? col[u] : -1;
            }
        }
        if (live && sub == 0) { sigmas[row] = sigma; rhos[row] = rho; }
    }
}

// ---------------------------------------------------------------------------------------------- host side
namespace {
size_t fz_room(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

struct fz_args {
    float local_connectivity, bandwidth, mix;
    int apply_set_ops;
};

int fz_check(csr_err &err, const char *who, const void *ids, int32_t id_bytes, const float *dists, int64_t m, int32_t k, int64_t ld, int64_t n,
             const fz_args &a, const float *sigmas, const float *rhos) {
    if (m < 0 || n < 1 || k < 2 || k > CSR_REG_CAP || ld < k || m >= (int64_t)0x7FFFFFF0 || n >= (int64_t)0x7FFFFFF0) {
        err.set_error("%s: bad shape (m = %lld, k = %d, ld = %lld, n = %lld; 2 <= k <= %d)", who, (long long)m, (int)k, (long long)ld, (long long)n,
                      CSR_REG_CAP);
        return 1;
    }
    if (id_bytes != 4 && id_bytes != 8) { err.set_error("%s: ids are int32 or int64 (id_bytes = %d)", who, (int)id_bytes); return 1; }
    if (!(a.local_connectivity > 0.0f) || a.local_connectivity > (float)(k - 1) || !(a.bandwidth > 0.0f) || !(a.mix >= 0.0f && a.mix <= 1.0f)) {
        err.set_error("%s: 0 < local_connectivity <= k - 1, bandwidth > 0, 0 <= set_op_mix_ratio <= 1 (got %g, %g, %g; k = %d)", who,
                      (double)a.local_connectivity, (double)a.bandwidth, (double)a.mix, (int)k);
        return 1;
    }
    if (a.apply_set_ops && m != n) { err.set_error("%s: the set operations need m == n (m = %lld, n = %lld)", who, (long long)m, (long long)n); return 1; }
    if (m > 0 && (!ids || !dists || !sigmas || !rhos)) { err.set_error("%s: null pointer", who); return 1; }
    return 0;
}

template <typename IdT>
void fz_launch_smooth(hipStream_t st, const IdT *ids, const float *dists, int64_t m, int32_t k, int64_t ld, int64_t n, float lc, float target,
                      const double *mean, float *sigmas, float *rhos, int32_t *cols, float *weights) {
    const int rows_per_block = k <= 16 ? 16 : (k <= 32 ? 8 : 4);
    const int64_t blocks = (m + rows_per_block - 1) / rows_per_block;
    const dim3 grid((unsigned)(blocks > (1 << 20) ? (1 << 20) : blocks)), block(256);
    if (k <= 16) hipLaunchKernelGGL((k_smooth_knn<1, 16, IdT>), grid, block, 0, st, ids, dists, m, k, ld, n, lc, target, mean, sigmas, rhos, cols, weights);
    else if (k <= 32) hipLaunchKernelGGL((k_smooth_knn<1, 32, IdT>), grid, block, 0, st, ids, dists, m, k, ld, n, lc, target, mean, sigmas, rhos, cols, weights);
    else if (k <= 64) hipLaunchKernelGGL((k_smooth_knn<1, 64, IdT>), grid, block, 0, st, ids, dists, m, k, ld, n, lc, target, mean, sigmas, rhos, cols, weights);
    else if (k <= 128) hipLaunchKernelGGL((k_smooth_knn<2, 64, IdT>), grid, block, 0, st, ids, dists, m, k, ld, n, lc, target, mean, sigmas, rhos, cols, weights);
    else hipLaunchKernelGGL((k_smooth_knn<4, 64, IdT>), grid, block, 0, st, ids, dists, m, k, ld, n, lc, target, mean, sigmas, rhos, cols, weights);
}

// mean, sigma / rho / weights, then the CSR stage on the two (m, k) scratch buffers
template <typename IdT>
int fz_build(csr_err &err, nnd_scratch &tmp, hipStream_t st, nnd_csr_s *g, const IdT *ids, const float *dists, int64_t m, int32_t k, int64_t ld,
             int64_t n, const fz_args &a, float *sigmas, float *rhos) {
    const size_t places = (size_t)m * (size_t)k;
    const int64_t want = ((int64_t)places + 4095) / 4096;  // 16 places a thread
    const int parts = (int)(want < 1 ? 1 : (want > FZ_MEAN_BLOCKS ? FZ_MEAN_BLOCKS : want));
    const size_t bytes = 2 * fz_room(8 * (size_t)FZ_MEAN_BLOCKS) + fz_room(8) + 2 * fz_room(4 * (places ? places : 1));
    unsigned char *base = tmp.get<unsigned char>(&err, bytes);
    if (!base) return 1;
    double *part_sum = (double *)base;
    unsigned long long *part_cnt = (unsigned long long *)(base + fz_room(8 * (size_t)FZ_MEAN_BLOCKS));
    double *mean = (double *)(base + 2 * fz_room(8 * (size_t)FZ_MEAN_BLOCKS));
    int32_t *cols = (int32_t *)(base + 2 * fz_room(8 * (size_t)FZ_MEAN_BLOCKS) + fz_room(8));
    float *weights = (float *)((unsigned char *)cols + fz_room(4 * (places ? places : 1)));
    if (m > 0) {
        const float target = (float)(log2((double)k) * (double)a.bandwidth);
        hipLaunchKernelGGL((k_fuzzy_mean<IdT>), dim3(parts), dim3(256), 0, st, ids, dists, m, k, ld, n, part_sum, part_cnt);
        hipLaunchKernelGGL(k_fuzzy_mean_sum, dim3(1), dim3(64), 0, st, (const double *)part_sum, (const unsigned long long *)part_cnt, parts, mean);
        fz_launch_smooth<IdT>(st, ids, dists, m, k, ld, n, a.local_connectivity, target, (const double *)mean, sigmas, rhos, cols, weights);
        CSR_HIP(hipGetLastError());
    }
    csr_combine combine;
    combine.fuzzy = 1;
    combine.mix = a.mix;
    return csr_build_i32(err, tmp, st, g, cols, weights, m, k, k, n, a.apply_set_ops ? 1 : 0, combine);
}

int fz_run(csr_err &err, hipStream_t st, nnd_csr_s *g, const void *ids, int32_t id_bytes, const float *dists, int64_t m, int32_t k, int64_t ld,
           int64_t n, const fz_args &a, float *sigmas, float *rhos) {
    nnd_scratch tmp;  // released on return, behind the synchronise below
    const int rc = id_bytes == 4 ? fz_build<int32_t>(err, tmp, st, g, (const int32_t *)ids, dists, m, k, ld, n, a, sigmas, rhos)
                                 : fz_build<int64_t>(err, tmp, st, g, (const int64_t *)ids, dists, m, k, ld, n, a, sigmas, rhos);
    const hipError_t e = hipStreamSynchronize(st);  // (on every path: the scratch goes when this returns)
    if (rc) return 1;
    if (e != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_fuzzy_set: a kernel failed: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
}  // namespace

extern "C" int32_t nnd_fuzzy_set_device(int32_t device, void *hip_stream, const void *ids_dev, int32_t id_bytes, const float *dists_dev, int64_t m,
                                        int32_t k, int64_t ld, int64_t n, float local_connectivity, float bandwidth, float set_op_mix_ratio,
                                        int32_t apply_set_ops, float *sigmas_dev, float *rhos_dev, nnd_csr_t *out) {
    csr_err err;
    if (!out) { err.set_error("nnd_fuzzy_set_device: null pointer"); return 1; }
    *out = nullptr;
    const fz_args a{local_connectivity, bandwidth, set_op_mix_ratio, apply_set_ops ? 1 : 0};
    if (fz_check(err, "nnd_fuzzy_set_device", ids_dev, id_bytes, dists_dev, m, k, ld, n, a, sigmas_dev, rhos_dev)) return 1;
    CSR_HIP(hipSetDevice(device));
    nnd_csr_s *g = new nnd_csr_s();
    g->device = device;
    if (fz_run(err, (hipStream_t)hip_stream, g, ids_dev, id_bytes, dists_dev, m, k, ld, n, a, sigmas_dev, rhos_dev)) { delete g; return 1; }
    *out = g;
    return 0;
}

extern "C" int32_t nnd_fuzzy_set(int32_t device, const void *ids, int32_t id_bytes, const float *dists, int64_t m, int32_t k, int64_t n,
                                 float local_connectivity, float bandwidth, float set_op_mix_ratio, int32_t apply_set_ops, float *sigmas,
                                 float *rhos, int64_t *indptr, int32_t *indices, float *data, int64_t capacity, int64_t *nnz, int64_t *long_rows) {
    csr_err err;
    const fz_args a{local_connectivity, bandwidth, set_op_mix_ratio, apply_set_ops ? 1 : 0};
    if (fz_check(err, "nnd_fuzzy_set", ids, id_bytes, dists, m, k, k, n, a, sigmas, rhos)) return 1;
    if (!indptr || !nnz || capacity < 0 || (capacity > 0 && (!indices || !data))) { err.set_error("nnd_fuzzy_set: null pointer"); return 1; }
    CSR_HIP(hipSetDevice(device));
    nnd_csr_s g;
    g.device = device;
    nnd_scratch up;
    const size_t places = (size_t)m * (size_t)k;
    unsigned char *ids_dev = up.get<unsigned char>(&err, places * (size_t)id_bytes);
    float *dists_dev = up.get<float>(&err, places);
    float *row_dev = up.get<float>(&err, 2 * (size_t)m);  // sigmas, then rhos
    if (!ids_dev || !dists_dev || !row_dev) return 1;
    hipStream_t st = nullptr;
    if (places > 0) {
        CSR_HIP(hipMemcpyAsync(ids_dev, ids, places * (size_t)id_bytes, hipMemcpyHostToDevice, st));
        CSR_HIP(hipMemcpyAsync(dists_dev, dists, places * sizeof(float), hipMemcpyHostToDevice, st));
    }
    if (fz_run(err, st, &g, ids_dev, id_bytes, dists_dev, m, k, k, n, a, row_dev, row_dev + m)) return 1;
    *nnz = g.nnz;
    if (long_rows) *long_rows = g.long_rows;
    if (g.nnz > capacity) { err.set_error("nnd_fuzzy_set: %lld entries, room for %lld", (long long)g.nnz, (long long)capacity); return 1; }
    if (m > 0) {
        CSR_HIP(hipMemcpy(sigmas, row_dev, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
        CSR_HIP(hipMemcpy(rhos, row_dev + m, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
    }
    CSR_HIP(hipMemcpy(indptr, g.indptr, sizeof(int64_t) * (size_t)(m + 1), hipMemcpyDeviceToHost));
    if (g.nnz > 0) {
        CSR_HIP(hipMemcpy(indices, g.indices, sizeof(int32_t) * (size_t)g.nnz, hipMemcpyDeviceToHost));
        CSR_HIP(hipMemcpy(data, g.data, sizeof(float) * (size_t)g.nnz, hipMemcpyDeviceToHost));
    }
    return 0;
}
