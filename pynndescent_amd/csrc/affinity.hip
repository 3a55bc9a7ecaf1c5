// affinity.hip -- t-SNE's perplexity affinities from k-lists on the device: per row the search for the Gaussian precision beta
// whose conditional distribution has the requested perplexity (sklearn's _binary_search_perplexity), for up to four
// perplexities at once (the multiscale form), then the symmetrisation P + P^T and the division by the total.  DESIGN.md
// section 4 "Perplexity affinities".
//
//   k_perplexity_search<KU, W, S>          beta of every row and scale, the conditional entry of every place; a place that is not
//                                          stored gets id -1 and value 0
//   k_affinity_total -> k_affinity_total_sum   the total of the conditional matrix, float64 (normalize)
//   k_affinity_scale                       the directed, normalised form: every entry times 1 / total
//   csr_build_i32 (csr_graph.hip)          the two (m, k) buffers to canonical CSR: directed as they are, or (a + b) * scale
//
// A row is its k places (id, d).  A place counts when its id lies in [0, n), is not the row itself (m == n) and its energy
// e = d * d (or d) is finite; any other place adds nothing to a sum and gets no entry.  The search works on x = (e - min e) *
// log2(e): the nearest place stays at p = 2^0 = 1 however large the distances are, so sum p >= 1 and the floor of 1e-8 is met
// by a row without a counting place alone.
//
// k_perplexity_search has csr_wave_sort's split: a row of at most 16, 32 or 64 places is held by W = 16, 32 or 64 lanes, one
// place a lane, so a wave solves 64 / W rows at once; 65..256 places take the wave with KU = 2 or 4 places per lane.  The ids
// and distances are read once; x stays in registers for all steps and all S scales, whose searches share the loop.  A step of
// a scale is per place one multiply, one v_exp_f32, one add and one fma (x held twice: +inf for the exponent of a place that
// does not count, 0 as its factor in sum x p, so the loop has no select), the two group sums carried through the DPP rotations
// together, one v_log_f32 and one v_rcp_f32.  No LDS, no barrier, no atomic.
//
// Determinism: the group sums are fuzzy.hip's -- four DPP row rotations by 8, 4, 2, 1, after which the 16 lanes of a row hold
// the same bits, and for W > 16 the row sums fetched with v_readlane and added in one fixed order.  lo, beta and hi are
// therefore the same in every lane of a group with no broadcast, and a row's result does not depend on which rows share its
// wave.  A scale that has stopped keeps its beta; the wave leaves the loop when a ballot says every scale of every group has
// stopped.  The total is a float64 sum of partials in a fixed order on a grid that depends on the shape alone.  Every store
// is a vector store.
#include <float.h>
#include <math.h>
#include <string.h>

#include "../../include/pynnd_amd.h"
#include "common.h"
#include "csr_graph.h"

#define AF_STEPS 100
#define AF_LOG2E 1.4426950408889634f
#define AF_TOLERANCE (1e-5f * AF_LOG2E)  // |H - log(perplexity)| <= 1e-5, in bits
#define AF_MIN_SUM 1e-8f                 // sklearn's EPSILON_DBL
#define AF_MAX_SCALES 4
#define AF_TOTAL_BLOCKS 512  // the most partials k_affinity_total leaves

struct af_scales {
    float target[AF_MAX_SCALES];  // log2(perplexity)
};

// ---------------------------------------------------------------------------------------------- the search
// The sums of a and of b over the W lanes of this lane's group, the same bits in each of them (every lane of the wave is
// active).  The two chains are independent and interleave.
template <int W>
__device__ __forceinline__ void af_group_sum2(float &a, float &b) {
    a += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(8)>(__float_as_int(a)));
    b += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(8)>(__float_as_int(b)));
    a += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(4)>(__float_as_int(a)));
    b += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(4)>(__float_as_int(b)));
    a += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(2)>(__float_as_int(a)));
    b += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(2)>(__float_as_int(b)));
    a += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(1)>(__float_as_int(a)));
    b += __int_as_float(nnd_dpp_i32<NND_DPP_ROW_ROR(1)>(__float_as_int(b)));
    if constexpr (W > 16) {
        const float a0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 0)), a1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 16));
        const float a2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 32)), a3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), 48));
        const float b0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), 0)), b1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), 16));
        const float b2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), 32)), b3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), 48));
        if constexpr (W == 32) {
            const bool low = nnd_lane() < 32;
            a = low ? a0 + a1 : a2 + a3;
            b = low ? b0 + b1 : b2 + b3;
        } else {
            a = (a0 + a1) + (a2 + a3);
            b = (b0 + b1) + (b2 + b3);
        }
    }
}

template <int KU, int W, int S>
__global__ __launch_bounds__(256) void k_perplexity_search(const void *__restrict__ ids, int id_bytes, const float *__restrict__ dists, int64_t m,
                                                           int32_t k, int64_t ld, int64_t n, int drop_self, int squared, af_scales scales,
                                                           float *__restrict__ betas, int32_t *__restrict__ cols, float *__restrict__ weights) {
    static_assert(W == 64 || KU == 1, "several places per lane: the whole wave is one row");
    constexpr int R = 64 / W;  // rows of a wave
    const int lane = nnd_lane(), sub = lane & (W - 1), group = lane / W;
    for (int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R; first < m; first += (int64_t)gridDim.x * 4 * R) {  // wave-uniform
        const int64_t row = first + group;
        const bool live = row < m;
        // ---- the row: x is the exponent's operand (+inf where the place does not count), w the factor in sum x p (0 there)
        float x[KU], w[KU];
        int32_t col[KU];
        int64_t id[KU];
        float e_min = INFINITY;
#pragma unroll
        for (int u = 0; u < KU; u++) {  // (every load of the row is issued before the first one is waited for)
            const int e = u * 64 + sub;
            id[u] = -1;
            x[u] = 0.0f;
            if (live && e < k) {
                const int64_t at = row * ld + e;
                id[u] = id_bytes == 8 ? ((const int64_t *)ids)[at] : (int64_t)((const int32_t *)ids)[at];
                x[u] = dists[at];
            }
        }
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int u = 0; u < KU; u++) {
                const float energy = squared ? x[u] * x[u] : x[u];
                const bool counts = id[u] >= 0 && id[u] < n && !(drop_self && id[u] == row) && fabsf(energy) < INFINITY;  // (false for NaN)
                col[u] = counts ? (int32_t)id[u] : -1;
                x[u] = counts ? energy : INFINITY;
                e_min = fminf(e_min, x[u]);
            }
#pragma unroll
            for (int o = W >> 1; o > 0; o >>= 1) e_min = fminf(e_min, __shfl_xor(e_min, o, 64));
#pragma unroll
            for (int u = 0; u < KU; u++) {
                x[u] = col[u] >= 0 ? fminf((x[u] - e_min) * AF_LOG2E, FLT_MAX) : INFINITY;
                w[u] = col[u] >= 0 ? x[u] : 0.0f;
            }
        }
        // ---- the S searches, one step of each per turn of the loop
        float beta[S], lo[S], hi[S], total[S];
        bool done[S];
#pragma unroll
        for (int s = 0; s < S; s++) {
            beta[s] = 1.0f;
            lo[s] = -INFINITY;
            hi[s] = INFINITY;
            total[s] = 1.0f;
            done[s] = !live;
        }
        for (int step = 0; step < AF_STEPS; step++) {
            bool open = false;
#pragma unroll
            for (int s = 0; s < S; s++) {
                const float nb = -beta[s];
                float sp = 0.0f, sxp = 0.0f;
#pragma unroll
                for (int u = 0; u < KU; u++) {
                    const float p = __builtin_amdgcn_exp2f(x[u] * nb);
                    sp += p;
                    sxp = fmaf(w[u], p, sxp);
                }
                af_group_sum2<W>(sp, sxp);
                sp = fmaxf(sp, AF_MIN_SUM);
                const float diff = (__builtin_amdgcn_logf(sp) + beta[s] * sxp * __builtin_amdgcn_rcpf(sp)) - scales.target[s];
                total[s] = sp;  // (a stopped scale keeps its beta: the same bits again)
                if (!done[s]) {
                    if (fabsf(diff) <= AF_TOLERANCE || step == AF_STEPS - 1) {
                        done[s] = true;  // beta is frozen; no update follows the last evaluation
                    } else if (diff > 0.0f) {
                        lo[s] = beta[s];
                        beta[s] = hi[s] == INFINITY ? beta[s] * 2.0f : (beta[s] + hi[s]) * 0.5f;
                    } else {
                        hi[s] = beta[s];
                        beta[s] = lo[s] == -INFINITY ? beta[s] * 0.5f : (beta[s] + lo[s]) * 0.5f;
                    }
                }
                open = open || !done[s];
            }
            if (__ballot(open) == 0ull) break;  // every scale of every group of the wave has stopped
        }
        // ---- the conditional entries: the mean over the scales of p / sum p; a place that is not stored is handed on as empty
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int e = u * 64 + sub;
            if (live && e < k) {
                float c = 0.0f;
#pragma unroll
                for (int s = 0; s < S; s++) c += __builtin_amdgcn_exp2f(x[u] * -beta[s]) / total[s];
                if constexpr (S > 1) c = c / (float)S;
                const bool stored = col[u] >= 0 && c > 0.0f;
                weights[row * k + e] = stored ? c : 0.0f;
                cols[row * k + e] = stored ? col[u] : -1;
            }
        }
        if (live && sub == 0) {
#pragma unroll
            for (int s = 0; s < S; s++) betas[row * S + s] = beta[s];
        }
    }
}

// ---------------------------------------------------------------------------------------------- the total of the matrix
// One partial per workgroup: a thread adds its places in index order (a place that is not stored holds 0), a wave its lanes
// by a fixed tree, thread 0 the four waves in order.  The grid depends on the shape alone, so the partials are the same bits
// on every run.
__global__ __launch_bounds__(256) void k_affinity_total(const float *__restrict__ weights, int64_t places, double *__restrict__ part) {
    __shared__ double s_sum[4];
    double s = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < places; t += (int64_t)gridDim.x * 256) s += (double)weights[t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (nnd_lane() == 0) s_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
}
// one wave adds the partials: a lane its own in index order, then the same tree
__global__ __launch_bounds__(64) void k_affinity_total_sum(const double *__restrict__ part, int parts, double *__restrict__ total) {
    double s = 0.0;
    for (int i = nnd_lane(); i < parts; i += 64) s += part[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (nnd_lane() == 0) *total = s;
}
// the directed form's division by the total; an entry that becomes 0 is handed on as an empty place
__global__ __launch_bounds__(256) void k_affinity_scale(int32_t *__restrict__ cols, float *__restrict__ weights, int64_t places, float scale) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < places; t += (int64_t)gridDim.x * 256) {
        const float v = weights[t] * scale;
        weights[t] = v;
        if (v == 0.0f) cols[t] = -1;
    }
}

// ---------------------------------------------------------------------------------------------- host side
namespace {
size_t af_room(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

struct af_args {
    af_scales scales;
    int n_scales, squared, symmetrize, normalize;
};

int af_check(csr_err &err, const char *who, const void *ids, int32_t id_bytes, const float *dists, int64_t m, int32_t k, int64_t ld, int64_t n,
             const float *perplexities, int32_t n_scales, int32_t symmetrize, const float *betas, af_args *a) {
    if (m < 0 || n < 1 || k < 1 || k > CSR_REG_CAP || ld < k || m >= (int64_t)0x7FFFFFF0 || n >= (int64_t)0x7FFFFFF0) {
        err.set_error("%s: bad shape (m = %lld, k = %d, ld = %lld, n = %lld; 1 <= k <= %d)", who, (long long)m, (int)k, (long long)ld, (long long)n,
                      CSR_REG_CAP);
        return 1;
    }
    if (id_bytes != 4 && id_bytes != 8) { err.set_error("%s: ids are int32 or int64 (id_bytes = %d)", who, (int)id_bytes); return 1; }
    if (n_scales < 1 || n_scales > AF_MAX_SCALES || !perplexities) {
        err.set_error("%s: between 1 and %d perplexities (got %d)", who, AF_MAX_SCALES, (int)n_scales);
        return 1;
    }
    for (int s = 0; s < AF_MAX_SCALES; s++) {
        const float p = perplexities[s < n_scales ? s : 0];
        if (!(p > 0.0f) || !(p < INFINITY)) { err.set_error("%s: a perplexity is above 0 and finite (got %g)", who, (double)p); return 1; }
        a->scales.target[s] = (float)log2((double)p);
    }
    if (symmetrize && m != n) { err.set_error("%s: symmetrize needs m == n (m = %lld, n = %lld)", who, (long long)m, (long long)n); return 1; }
    if (m > 0 && (!ids || !dists || !betas)) { err.set_error("%s: null pointer", who); return 1; }
    return 0;
}

template <int KU, int W>
void af_launch_scales(hipStream_t st, dim3 grid, int S, const void *ids, int id_bytes, const float *dists, int64_t m, int32_t k, int64_t ld, int64_t n,
                      int drop_self, int squared, const af_scales &sc, float *betas, int32_t *cols, float *weights) {
    const dim3 block(256);
    if (S == 1) hipLaunchKernelGGL((k_perplexity_search<KU, W, 1>), grid, block, 0, st, ids, id_bytes, dists, m, k, ld, n, drop_self, squared, sc, betas, cols, weights);
    else if (S == 2) hipLaunchKernelGGL((k_perplexity_search<KU, W, 2>), grid, block, 0, st, ids, id_bytes, dists, m, k, ld, n, drop_self, squared, sc, betas, cols, weights);
    else if (S == 3) hipLaunchKernelGGL((k_perplexity_search<KU, W, 3>), grid, block, 0, st, ids, id_bytes, dists, m, k, ld, n, drop_self, squared, sc, betas, cols, weights);
    else hipLaunchKernelGGL((k_perplexity_search<KU, W, 4>), grid, block, 0, st, ids, id_bytes, dists, m, k, ld, n, drop_self, squared, sc, betas, cols, weights);
}

void af_launch_search(hipStream_t st, const void *ids, int id_bytes, const float *dists, int64_t m, int32_t k, int64_t ld, int64_t n, const af_args &a,
                      float *betas, int32_t *cols, float *weights) {
    const int rows_per_block = k <= 16 ? 16 : (k <= 32 ? 8 : 4);
    const int64_t blocks = (m + rows_per_block - 1) / rows_per_block;
    const dim3 grid((unsigned)(blocks > (1 << 20) ? (1 << 20) : blocks));
    const int drop_self = m == n ? 1 : 0;
    if (k <= 16) af_launch_scales<1, 16>(st, grid, a.n_scales, ids, id_bytes, dists, m, k, ld, n, drop_self, a.squared, a.scales, betas, cols, weights);
    else if (k <= 32) af_launch_scales<1, 32>(st, grid, a.n_scales, ids, id_bytes, dists, m, k, ld, n, drop_self, a.squared, a.scales, betas, cols, weights);
    else if (k <= 64) af_launch_scales<1, 64>(st, grid, a.n_scales, ids, id_bytes, dists, m, k, ld, n, drop_self, a.squared, a.scales, betas, cols, weights);
    else if (k <= 128) af_launch_scales<2, 64>(st, grid, a.n_scales, ids, id_bytes, dists, m, k, ld, n, drop_self, a.squared, a.scales, betas, cols, weights);
    else af_launch_scales<4, 64>(st, grid, a.n_scales, ids, id_bytes, dists, m, k, ld, n, drop_self, a.squared, a.scales, betas, cols, weights);
}

// the search, the total where it is asked for, then the CSR stage on the two (m, k) scratch buffers
int af_build(csr_err &err, nnd_scratch &tmp, hipStream_t st, nnd_csr_s *g, const void *ids, int id_bytes, const float *dists, int64_t m, int32_t k,
             int64_t ld, int64_t n, const af_args &a, float *betas) {
    const size_t places = (size_t)m * (size_t)k;
    const int64_t want = ((int64_t)places + 4095) / 4096;  // 16 places a thread
    const int parts = (int)(want < 1 ? 1 : (want > AF_TOTAL_BLOCKS ? AF_TOTAL_BLOCKS : want));
    const size_t head = af_room(8 * (size_t)AF_TOTAL_BLOCKS) + af_room(8);
    unsigned char *base = tmp.get<unsigned char>(&err, head + 2 * af_room(4 * (places ? places : 1)));
    if (!base) return 1;
    double *part = (double *)base, *total = (double *)(base + af_room(8 * (size_t)AF_TOTAL_BLOCKS));
    int32_t *cols = (int32_t *)(base + head);
    float *weights = (float *)(base + head + af_room(4 * (places ? places : 1)));
    float scale = 1.0f;
    if (m > 0) {
        af_launch_search(st, ids, id_bytes, dists, m, k, ld, n, a, betas, cols, weights);
        if (a.normalize) {
            double sum = 0.0;
            hipLaunchKernelGGL(k_affinity_total, dim3(parts), dim3(256), 0, st, (const float *)weights, (int64_t)places, part);
            hipLaunchKernelGGL(k_affinity_total_sum, dim3(1), dim3(64), 0, st, (const double *)part, parts, total);
            CSR_HIP(hipMemcpyAsync(&sum, total, sizeof(double), hipMemcpyDeviceToHost, st));
            CSR_HIP(hipStreamSynchronize(st));
            scale = sum > 0.0 ? (float)(1.0 / (a.symmetrize ? 2.0 * sum : sum)) : 0.0f;
            if (!a.symmetrize) hipLaunchKernelGGL(k_affinity_scale, dim3(parts), dim3(256), 0, st, cols, weights, (int64_t)places, scale);
        }
        CSR_HIP(hipGetLastError());
    }
    csr_combine combine;
    combine.sum = 1;
    combine.scale = scale;
    return csr_build_i32(err, tmp, st, g, cols, weights, m, k, k, n, a.symmetrize, combine);
}

int af_run(csr_err &err, hipStream_t st, nnd_csr_s *g, const void *ids, int32_t id_bytes, const float *dists, int64_t m, int32_t k, int64_t ld,
           int64_t n, const af_args &a, float *betas) {
    nnd_scratch tmp;  // released on return, behind the synchronise below
    const int rc = af_build(err, tmp, st, g, ids, id_bytes, dists, m, k, ld, n, a, betas);
    const hipError_t e = hipStreamSynchronize(st);  // (on every path: the scratch goes when this returns)
    if (rc) return 1;
    if (e != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_perplexity_affinities: a kernel failed: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
}  // namespace

extern "C" int32_t nnd_perplexity_affinities_device(int32_t device, void *hip_stream, const void *ids_dev, int32_t id_bytes, const float *dists_dev,
                                                    int64_t m, int32_t k, int64_t ld, int64_t n, const float *perplexities, int32_t n_scales,
                                                    int32_t squared, int32_t symmetrize, int32_t normalize, float *betas_dev, nnd_csr_t *out) {
    csr_err err;
    if (!out) { err.set_error("nnd_perplexity_affinities_device: null pointer"); return 1; }
    *out = nullptr;
    af_args a{{}, (int)n_scales, squared ? 1 : 0, symmetrize ? 1 : 0, normalize ? 1 : 0};
    if (af_check(err, "nnd_perplexity_affinities_device", ids_dev, id_bytes, dists_dev, m, k, ld, n, perplexities, n_scales, symmetrize, betas_dev, &a))
        return 1;
    CSR_HIP(hipSetDevice(device));
    nnd_csr_s *g = new nnd_csr_s();
    g->device = device;
    if (af_run(err, (hipStream_t)hip_stream, g, ids_dev, id_bytes, dists_dev, m, k, ld, n, a, betas_dev)) { delete g; return 1; }
    *out = g;
    return 0;
}

extern "C" int32_t nnd_perplexity_affinities(int32_t device, const void *ids, int32_t id_bytes, const float *dists, int64_t m, int32_t k, int64_t n,
                                             const float *perplexities, int32_t n_scales, int32_t squared, int32_t symmetrize, int32_t normalize,
                                             float *betas, int64_t *indptr, int32_t *indices, float *data, int64_t capacity, int64_t *nnz,
                                             int64_t *long_rows) {
    csr_err err;
    af_args a{{}, (int)n_scales, squared ? 1 : 0, symmetrize ? 1 : 0, normalize ? 1 : 0};
    if (af_check(err, "nnd_perplexity_affinities", ids, id_bytes, dists, m, k, k, n, perplexities, n_scales, symmetrize, betas, &a)) return 1;
    if (!indptr || !nnz || capacity < 0 || (capacity > 0 && (!indices || !data))) { err.set_error("nnd_perplexity_affinities: null pointer"); return 1; }
    CSR_HIP(hipSetDevice(device));
    nnd_csr_s g;
    g.device = device;
    nnd_scratch up;
    const size_t places = (size_t)m * (size_t)k;
    unsigned char *ids_dev = up.get<unsigned char>(&err, places * (size_t)id_bytes);
    float *dists_dev = up.get<float>(&err, places);
    float *betas_dev = up.get<float>(&err, (size_t)m * (size_t)n_scales);
    if (!ids_dev || !dists_dev || !betas_dev) return 1;
    hipStream_t st = nullptr;
    if (places > 0) {
        CSR_HIP(hipMemcpyAsync(ids_dev, ids, places * (size_t)id_bytes, hipMemcpyHostToDevice, st));
        CSR_HIP(hipMemcpyAsync(dists_dev, dists, places * sizeof(float), hipMemcpyHostToDevice, st));
    }
    if (af_run(err, st, &g, ids_dev, id_bytes, dists_dev, m, k, k, n, a, betas_dev)) return 1;
    *nnz = g.nnz;
    if (long_rows) *long_rows = g.long_rows;
    if (g.nnz > capacity) { err.set_error("nnd_perplexity_affinities: %lld entries, room for %lld", (long long)g.nnz, (long long)capacity); return 1; }
    if (m > 0) CSR_HIP(hipMemcpy(betas, betas_dev, sizeof(float) * (size_t)m * (size_t)n_scales, hipMemcpyDeviceToHost));
    CSR_HIP(hipMemcpy(indptr, g.indptr, sizeof(int64_t) * (size_t)(m + 1), hipMemcpyDeviceToHost));
    if (g.nnz > 0) {
        CSR_HIP(hipMemcpy(indices, g.indices, sizeof(int32_t) * (size_t)g.nnz, hipMemcpyDeviceToHost));
        CSR_HIP(hipMemcpy(data, g.data, sizeof(float) * (size_t)g.nnz, hipMemcpyDeviceToHost));
    }
    return 0;
}
