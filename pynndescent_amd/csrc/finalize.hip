// finalize.hip -- final row ordering and exact distances; debug Gram tile.
//
// k_finalize replaces deheap_sort (reference utils.py:189-218): rows ascending by distance, empty
// slots (-1, +inf) last.  The k-lists carry Gram-form f32 distances of centred / normalised rows
// (good enough to RANK); the distances handed back are recomputed from the ORIGINAL rows in the
// reference's own formulas with float64 accumulation (metric.h nnd_ref_acc / nnd_ref_dist, hellinger's
// terms in float32 as the reference's), then rows are re-sorted by that value.
//
// The float64 arithmetic of the codes 0 / 1 on rows of whole 16-byte chunks (d % 4 == 0, k <= 64) is spelled operation by
// operation, so that the bits handed back are a property of this text and not of the compiler's choice of what to fuse:
//   * the 16 lanes of a group split a row by chunks: lane l takes the chunks t = 4 l + 64 i, i = 0, 1, ..;
//   * a chunk's four terms p0..p3 (code 0: p = (a - b)^2 on the float64 difference; code 1: a b, a a and b b, three sums)
//     join as s = p1, s = fma(., ., s) for p0, p2, p3 in that order, then the lane's sum takes s by one addition;
//   * the 16 lanes' sums join by the xor butterfly 8, 4, 2, 1 (v += partner's v; every lane ends on the same bits);
//   * the value is (float) of that sum (code 1: of nnd_ref_dist on the three sums).
// fin_* below are the only float64 operations of that path, compiled with contraction off; tests/finalize_reference.py restates
// them and tests/test_gpu_finalize_exact.py holds the kernels to it bit for bit.  The codes 2..6, rows with d % 4 != 0 and
// k_finalize_wide sum as nnd_ref_acc does.
#include "common.h"
#include "merge.h"
#include "metric.h"
#include "state.h"

__device__ __forceinline__ double fin_sub(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double fin_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
// one chunk of <a, b>: p1 first, then p0, p2, p3 by fused multiply-add
__device__ __forceinline__ double fin_chunk(double a0, double a1, double a2, double a3, double b0, double b1, double b2, double b3) {
#pragma clang fp contract(off)
    double s = a1 * b1;
    s = __builtin_fma(a0, b0, s);
    s = __builtin_fma(a2, b2, s);
    return __builtin_fma(a3, b3, s);
}
// code 0: the chunk's squared differences
__device__ __forceinline__ double fin_chunk_sq(const float4 a, const float4 b) {
    const double d0 = fin_sub((double)a.x, (double)b.x), d1 = fin_sub((double)a.y, (double)b.y);
    const double d2 = fin_sub((double)a.z, (double)b.z), d3 = fin_sub((double)a.w, (double)b.w);
    return fin_chunk(d0, d1, d2, d3, d0, d1, d2, d3);
}
__device__ __forceinline__ double fin_chunk_dot(const float4 a, const float4 b) {
    return fin_chunk((double)a.x, (double)a.y, (double)a.z, (double)a.w, (double)b.x, (double)b.y, (double)b.z, (double)b.w);
}

// one coordinate pair into the float64 sums, hellinger's terms as the reference takes them (metric.h)
template <int FAM>
__device__ __forceinline__ void fin_acc(int metric, double a, double b, double &dot, double &nx, double &ny) {
    nnd_ref_acc<FAM, NND_HELLINGER_F32>(metric, a, b, dot, nx, ny);
}
// the 16 lanes' partial sums of one pair -> the distance handed back
template <int FAM>
__device__ __forceinline__ float fin_value(int metric, double dot, double nx, double ny, int d) {
    const double dt = nnd_group_sum_f64<16>(dot);
    if (metric == 0) return (float)dt;
    if constexpr (FAM == NND_CODES_BOOL)  // the three counts and the column count (the only family that reads d)
        return (float)nnd_ref_dist<FAM>(metric, dt, nnd_group_sum_f64<16>(nx), nnd_group_sum_f64<16>(ny), (double)d);
    return (float)nnd_ref_dist<FAM>(metric, dt, nnd_group_sum_f64<16>(nx), nnd_group_sum_f64<16>(ny));
}

// One wave per row.  The 64 lanes work as 4 groups of 16: group g takes neighbours g, 4+g, 8+g, ... so four distances
// are accumulated side by side and up to 16 neighbour rows are in flight per wave (the gather is latency bound when
// the rows are fetched one after another).
// METRIC is a template parameter: the euclidean instance does not carry the cosine accumulators (146 -> far fewer
// registers, i.e. more waves per SIMD for what is a gather-latency-bound kernel).  METRIC 2..6: the other metrics, one
// instance each; METRIC 8..16: the boolean family, one instance each (the counts of the rows as given, then the float64 twin).
template <int METRIC>
__global__ __launch_bounds__(256, METRIC == 0 ? 6 : 4) void k_finalize(const float *__restrict__ x, int d, int64_t lo, int64_t n, int k, int ks,
                                                  const uint32_t *__restrict__ knn_e, const int32_t *__restrict__ order,
                                                  int32_t *__restrict__ out_idx, float *__restrict__ out_dist) {
    const int lane = nnd_lane(), w = threadIdx.x >> 6;
    // rows are visited in `order` (spatially coherent, see nnd_vertex_order), one contiguous eighth per XCD, so the
    // neighbour rows of concurrently running waves overlap in L2
    int64_t b = blockIdx.x;
    if ((gridDim.x & 7) == 0) b = (b & 7) * (gridDim.x >> 3) + (b >> 3);
    const int64_t g = lo + b * 4 + w;  // owned rows [lo, n); output row index is v - lo
    if (g >= n) return;
    const int64_t v = order ? (int64_t)order[g] : g;
    uint32_t e = lane < k ? knn_e[v * ks + lane] : NND_EMPTY_E;
    const float *xv = x + v * d;
    const int grp = lane >> 4, l16 = lane & 15;
    const bool vec = (d & 3) == 0;  // rows 16-byte aligned
    constexpr int metric = METRIC, FAM = METRIC < 2 ? NND_CODES_01 : (METRIC >= NND_BOOL_FIRST ? NND_CODES_BOOL : NND_CODES_ANY);
    float mine = INFINITY;
    const int nsteps = (k + 3) >> 2;
    for (int s0 = 0; s0 < nsteps; s0 += 4) {
        const float *xu[4];
        bool on[4];
        double dot[4], nx[4], ny[4];  // (sqeuclidean: the squared differences in dot)
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = 4 * (s0 + u) + grp;
            const uint32_t ej = __shfl(e, j & 63, 64);
            on[u] = j < k && ej != NND_EMPTY_E;
            xu[u] = x + (int64_t)(on[u] ? (ej & NND_IDX_MASK) : 0) * d;
            dot[u] = nx[u] = ny[u] = 0.0;
        }
        double mua = 0.0, mub[4] = {0.0, 0.0, 0.0, 0.0};  // correlation: the row means
        if (metric == 4) {
            mua = nnd_row_mean_f64<16>(xv, d, l16);
#pragma unroll
            for (int u = 0; u < 4; u++) mub[u] = nnd_row_mean_f64<16>(xu[u], d, l16);
        }
        if (vec) {
            for (int t = 4 * l16; t < d; t += 64) {
                const float4 a = *(const float4 *)(xv + t);
                float4 q[4];
#pragma unroll
                for (int u = 0; u < 4; u++) q[u] = *(const float4 *)(xu[u] + t);
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (metric == 0) {  // codes 0 / 1: a chunk's four terms are summed before they join the accumulator (file header)
                        dot[u] = fin_add(dot[u], fin_chunk_sq(a, q[u]));
                    } else if (metric == 1) {
                        dot[u] = fin_add(dot[u], fin_chunk_dot(a, q[u]));
                        nx[u] = fin_add(nx[u], fin_chunk_dot(a, a));
                        ny[u] = fin_add(ny[u], fin_chunk_dot(q[u], q[u]));
                    } else {
                        const double a0 = a.x, a1 = a.y, a2 = a.z, a3 = a.w;
                        const double b0 = q[u].x, b1 = q[u].y, b2 = q[u].z, b3 = q[u].w;
                        fin_acc<FAM>(metric, a0 - mua, b0 - mub[u], dot[u], nx[u], ny[u]);
                        fin_acc<FAM>(metric, a1 - mua, b1 - mub[u], dot[u], nx[u], ny[u]);
                        fin_acc<FAM>(metric, a2 - mua, b2 - mub[u], dot[u], nx[u], ny[u]);
                        fin_acc<FAM>(metric, a3 - mua, b3 - mub[u], dot[u], nx[u], ny[u]);
                    }
                }
            }
        } else {
            for (int t = l16; t < d; t += 16) {
                const double a0 = xv[t];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    fin_acc<FAM>(metric, a0 - mua, (double)xu[u][t] - mub[u], dot[u], nx[u], ny[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            float val = fin_value<FAM>(metric, dot[u], nx[u], ny[u], d);
            if (!on[u]) val = INFINITY;
            // neighbour j = 4 * (s0 + u) + group: lane j takes it from (any lane of) group j & 3
            const float got = __shfl(val, 16 * (lane & 3), 64);
            if ((lane >> 2) == s0 + u) mine = got;
        }
    }
    // rank by (distance, index); empty entries are (+inf, 0x7FFFFFFF) and land at the tail
    const uint32_t myidx = e == NND_EMPTY_E ? NND_IDX_MASK : (e & NND_IDX_MASK);
    const uint64_t mykey = ((uint64_t)__float_as_uint(mine) << 32) | myidx;
    int r = 0;
    for (int j = 0; j < k; j++) {
        uint64_t kj = ((uint64_t)__float_as_uint(__shfl(mine, j, 64)) << 32) | __shfl(myidx, j, 64);
        r += (kj < mykey || (kj == mykey && j < lane)) ? 1 : 0;
    }
    if (lane < k) {
        out_idx[(v - lo) * k + r] = e == NND_EMPTY_E ? -1 : (int32_t)(e & NND_IDX_MASK);
        out_dist[(v - lo) * k + r] = mine;
    }
}

// k <= 16, codes 0 / 1, d % 4 == 0: one row per 16-lane group, four rows per wave.  Everything a row needs stays inside its
// DPP row, so nothing goes through the LDS pipe and the per-wave bookkeeping is shared by four rows:
//   * every lane of a group reads the row's 16 entries itself (four 16-byte loads of one address per group);
//   * the group takes its neighbours four at a time (16 neighbour rows in flight per wave, as in k_finalize);
//   * the butterfly's partners come by DPP moves.  No single pattern reaches lane l ^ 4, so lane p of the group plays chunk
//     lane c = p ^ 3 for p & 4, p otherwise: then c ^ 8, c ^ 4, c ^ 2, c ^ 1 sit at p ror 8, the half-row mirror 7 - (p & 7),
//     p ^ 2, p ^ 1 -- the pairs and their order are the file header's, only the lane that holds a chunk differs;
//   * the four sums of a round join in one butterfly: at the first step a lane keeps two of the four sums and hands the other
//     two to its partner, at the second it keeps one of two, so a lane's four additions per step become 2, 1, 1, 1 -- each still
//     v[c] + v[c ^ o] of the same two lanes.  Quad q of the row ends on the sum of the round's neighbour q;
//   * lane p therefore keeps neighbour 4 (p & 3) + (p >> 2); the rank is a count over the 15 row rotations of the (distance,
//     index) keys.
template <int CTRL>
__device__ __forceinline__ double fin_dpp_f64(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xF, 0xF, true);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, true);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}
__device__ __forceinline__ double fin_row_sum_f64(double v) {  // all 16 lanes of the row active
    v = fin_add(v, fin_dpp_f64<NND_DPP_ROW_ROR(8)>(v));
    v = fin_add(v, fin_dpp_f64<NND_DPP_ROW_HALF_MIRROR>(v));
    v = fin_add(v, fin_dpp_f64<NND_DPP_QUAD_XOR2>(v));
    return fin_add(v, fin_dpp_f64<NND_DPP_QUAD_XOR1>(v));
}
// four sums per lane -> quad q of the row holds the 16-lane sum of v[q] (on every one of its lanes)
__device__ __forceinline__ double fin_row_sum4_f64(const double (&v)[4], int p16) {
    const bool lo8 = (p16 & 8) == 0, lo4 = (p16 & 4) == 0;
    const double a = fin_add(lo8 ? v[0] : v[2], fin_dpp_f64<NND_DPP_ROW_ROR(8)>(lo8 ? v[2] : v[0]));
    const double b = fin_add(lo8 ? v[1] : v[3], fin_dpp_f64<NND_DPP_ROW_ROR(8)>(lo8 ? v[3] : v[1]));
    double s = fin_add(lo4 ? a : b, fin_dpp_f64<NND_DPP_ROW_HALF_MIRROR>(lo4 ? b : a));
    s = fin_add(s, fin_dpp_f64<NND_DPP_QUAD_XOR2>(s));
    return fin_add(s, fin_dpp_f64<NND_DPP_QUAD_XOR1>(s));
}
// keys of the row that sort before mine: rotation T brings lane p the key of lane (p - T) & 15, which wins a tie iff p >= T
template <int T>
__device__ __forceinline__ int fin_row_rank(uint32_t klo, uint32_t khi, int p16) {
    if constexpr (T == 0) return 0;
    else {
        const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)klo, NND_DPP_ROW_ROR(T), 0xF, 0xF, true);
        const uint32_t ohi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)khi, NND_DPP_ROW_ROR(T), 0xF, 0xF, true);
        const uint64_t other = ((uint64_t)ohi << 32) | olo, mine = ((uint64_t)khi << 32) | klo;
        return (((other < mine) | ((other == mine) & (p16 >= T))) ? 1 : 0) + fin_row_rank<T - 1>(klo, khi, p16);
    }
}

template <int METRIC>
__global__ __launch_bounds__(256, METRIC == 0 ? 6 : 4) void k_finalize16(const float *__restrict__ x, int d, int64_t lo, int64_t n, int k, int ks,
                                                    const uint32_t *__restrict__ knn_e, const int32_t *__restrict__ order,
                                                    int32_t *__restrict__ out_idx, float *__restrict__ out_dist) {
    static_assert(METRIC == 0 || METRIC == 1, "the other codes go through k_finalize");
    const int lane = nnd_lane(), w = threadIdx.x >> 6, grp = lane >> 4, p16 = lane & 15;
    const int c16 = (p16 & 4) ? (p16 ^ 3) : p16;  // the chunk lane this lane plays
    // rows in `order`, one contiguous eighth per XCD (see k_finalize)
    int64_t b = blockIdx.x;
    if ((gridDim.x & 7) == 0) b = (b & 7) * (gridDim.x >> 3) + (b >> 3);
    const int64_t g0 = lo + (b * 4 + w) * 4;
    if (g0 >= n) return;
    // a group past the end works on the last row again and stores nothing: every lane of the wave stays active for the DPP moves
    const bool row_on = g0 + grp < n;
    const int64_t g = row_on ? g0 + grp : n - 1;
    const int64_t v = order ? (int64_t)order[g] : g;
    const uint32_t *er = knn_e + v * ks;  // (ks = 16: a 64-byte row)
    const int j16 = 4 * (p16 & 3) + (p16 >> 2);  // the neighbour whose value ends on this lane
    const uint32_t e = j16 < k ? er[j16] : NND_EMPTY_E;
    u32x4 eb[4];
#pragma unroll
    for (int bt = 0; bt < 4; bt++) eb[bt] = *(const u32x4 *)(er + 4 * bt);
    const uint32_t row_bytes = (uint32_t)d * 4u;  // (one 64-bit multiply-add per row address)
    const char *xc = (const char *)(x + 4 * c16);
    const float *xv = (const float *)(xc + (uint64_t)v * row_bytes);
    float mine = INFINITY;
#pragma unroll
    for (int bt = 0; bt < 4; bt++) {
        if (4 * bt >= k) break;
        const float *xu[4];
        double dot[4], ny[4], nx = 0.0;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t ej = eb[bt][u];
            const bool on = 4 * bt + u < k && ej != NND_EMPTY_E;  // (an empty slot reads row 0; its lane hands back +inf)
            xu[u] = (const float *)(xc + (uint64_t)(on ? (ej & NND_IDX_MASK) : 0u) * row_bytes);
            dot[u] = ny[u] = 0.0;
        }
        for (int t = 4 * c16; t < d; t += 64) {
            const int o = t - 4 * c16;
            const float4 a = *(const float4 *)(xv + o);
            float4 q[4];
#pragma unroll
            for (int u = 0; u < 4; u++) q[u] = *(const float4 *)(xu[u] + o);
            if (METRIC == 1) nx = fin_add(nx, fin_chunk_dot(a, a));
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (METRIC == 0) {
                    dot[u] = fin_add(dot[u], fin_chunk_sq(a, q[u]));
                } else {
                    dot[u] = fin_add(dot[u], fin_chunk_dot(a, q[u]));
                    ny[u] = fin_add(ny[u], fin_chunk_dot(q[u], q[u]));
                }
            }
        }
        const double dt = fin_row_sum4_f64(dot, p16);  // neighbour 4 bt + (p16 >> 2)
        float val;
        if (METRIC == 0) val = (float)dt;
        else val = (float)nnd_ref_dist<NND_CODES_01>(1, dt, fin_row_sum_f64(nx), fin_row_sum4_f64(ny, p16));
        if ((p16 & 3) == bt) mine = val;
    }
    if (e == NND_EMPTY_E) mine = INFINITY;
    // rank by (distance, index); empty entries are (+inf, 0x7FFFFFFF) and land at the tail, lanes past k behind every key
    const uint32_t myidx = e == NND_EMPTY_E ? NND_IDX_MASK : (e & NND_IDX_MASK);
    const uint32_t klo = j16 < k ? myidx : 0xFFFFFFFFu, khi = j16 < k ? __float_as_uint(mine) : 0xFFFFFFFFu;
    const int r = fin_row_rank<15>(klo, khi, p16);
    if (row_on && j16 < k) {
        out_idx[(v - lo) * k + r] = e == NND_EMPTY_E ? -1 : (int32_t)(e & NND_IDX_MASK);
        out_dist[(v - lo) * k + r] = mine;
    }
}

// 64 < k <= NND_WIDE_K: one wave per row, ids / exact distances through LDS, four neighbours at a time (16 lanes each), ranks by
// counting over the LDS copy.  Same arithmetic as k_finalize.  FAM: NND_CODES_01, NND_CODES_ANY for the metrics of codes 2..6 (the
// sqeuclidean / cosine instance does not carry their registers) or NND_CODES_BOOL (metric.h nnd_metric_family).
template <int FAM>
__device__ __forceinline__ void fin_wide_body(const float *__restrict__ x, int d, int64_t lo, int64_t n, int k, int ks, int metric,
                                              const uint32_t *__restrict__ knn_e, int32_t *__restrict__ out_idx,
                                              float *__restrict__ out_dist) {
    __shared__ uint32_t sid[4][NND_WIDE_K];
    __shared__ float sdist[4][NND_WIDE_K];
    constexpr bool XM = FAM != NND_CODES_01;
    const int lane = nnd_lane(), w = threadIdx.x >> 6, grp = lane >> 4, l16 = lane & 15;
    const int64_t v = lo + (int64_t)blockIdx.x * 4 + w;
    if (v >= n) return;
    for (int j = lane; j < k; j += 64) sid[w][j] = knn_e[v * ks + j];
    nnd_wave_lds_sync();
    const float *xv = x + v * d;
    for (int j0 = 0; j0 < k; j0 += 4) {
        const int j = j0 + grp;
        const uint32_t ej = j < k ? sid[w][j] : NND_EMPTY_E;
        const bool on = ej != NND_EMPTY_E;
        const float *xu = x + (int64_t)(on ? (ej & NND_IDX_MASK) : 0) * d;
        double dot = 0.0, nx = 0.0, ny = 0.0;
        const bool corr = XM && FAM != NND_CODES_BOOL && metric == 4;
        const double mua = corr ? nnd_row_mean_f64<16>(xv, d, l16) : 0.0, mub = corr ? nnd_row_mean_f64<16>(xu, d, l16) : 0.0;
        for (int t = l16; t < d; t += 16) fin_acc<FAM>(metric, (double)xv[t] - mua, (double)xu[t] - mub, dot, nx, ny);
        float val = fin_value<FAM>(metric, dot, nx, ny, d);
        if (!on) val = INFINITY;
        if (l16 == 0 && j < k) sdist[w][j] = val;
    }
    nnd_wave_lds_sync();
    for (int j = lane; j < k; j += 64) {
        const uint32_t e = sid[w][j];
        const uint32_t myidx = e == NND_EMPTY_E ? NND_IDX_MASK : (e & NND_IDX_MASK);
        const uint64_t mykey = ((uint64_t)__float_as_uint(sdist[w][j]) << 32) | myidx;
        int r = 0;
        for (int q = 0; q < k; q++) {
            const uint32_t eq = sid[w][q];
            const uint64_t kq = ((uint64_t)__float_as_uint(sdist[w][q]) << 32) | (eq == NND_EMPTY_E ? NND_IDX_MASK : (eq & NND_IDX_MASK));
            r += (kq < mykey || (kq == mykey && q < j)) ? 1 : 0;
        }
        out_idx[(v - lo) * k + r] = e == NND_EMPTY_E ? -1 : (int32_t)(e & NND_IDX_MASK);
        out_dist[(v - lo) * k + r] = sdist[w][j];
    }
}
template <int FAM>
__global__ __launch_bounds__(256) void k_finalize_wide(const float *__restrict__ x, int d, int64_t lo, int64_t n, int k, int ks, int metric,
                                                       const uint32_t *__restrict__ knn_e, int32_t *__restrict__ out_idx,
                                                       float *__restrict__ out_dist) {
    fin_wide_body<FAM>(x, d, lo, n, k, ks, metric, knn_e, out_idx, out_dist);
}

int nnd_launch_finalize(nnd_ctx *ctx, int32_t *out_idx_dev, float *out_dist_dev) {
    unsigned grid = (unsigned)((ctx->own_hi - ctx->own_lo + 3) / 4);
    if (ctx->k > 64) {
        hipLaunchKernelGGL(nnd_metric_bool(ctx->p.metric) ? k_finalize_wide<NND_CODES_BOOL> : (ctx->p.metric >= 2 ? k_finalize_wide<NND_CODES_ANY> : k_finalize_wide<NND_CODES_01>), dim3(grid), dim3(256), 0, ctx->stream, ctx->x_orig, ctx->d, ctx->own_lo, ctx->own_hi, ctx->k, ctx->ks,
                           ctx->p.metric, ctx->knn_e, out_idx_dev, out_dist_dev);
        NND_HIP_CHECK(hipGetLastError());
        return 0;
    }
    if (ctx->k <= 16 && ctx->p.metric <= 1 && (ctx->d & 3) == 0) {  // four rows per wave
        grid = ((unsigned)((ctx->own_hi - ctx->own_lo + 15) / 16) + 7u) & ~7u;
        hipLaunchKernelGGL(ctx->p.metric == 0 ? k_finalize16<0> : k_finalize16<1>, dim3(grid), dim3(256), 0, ctx->stream, ctx->x_orig, ctx->d,
                           ctx->own_lo, ctx->own_hi, ctx->k, ctx->ks, ctx->knn_e, nnd_vertex_order(ctx), out_idx_dev, out_dist_dev);
        NND_HIP_CHECK(hipGetLastError());
        return 0;
    }
    grid = (grid + 7u) & ~7u;  // whole multiples of the XCD count
    auto kern = k_finalize<0>;
    switch (ctx->p.metric) {
        case 1: kern = k_finalize<1>; break;
        case 2: kern = k_finalize<2>; break;
        case 3: kern = k_finalize<3>; break;
        case 4: kern = k_finalize<4>; break;
        case 5: kern = k_finalize<5>; break;
        case 6: kern = k_finalize<6>; break;
        case 8: kern = k_finalize<8>; break;
        case 9: kern = k_finalize<9>; break;
        case 10: kern = k_finalize<10>; break;
        case 11: kern = k_finalize<11>; break;
        case 12: kern = k_finalize<12>; break;
        case 13: kern = k_finalize<13>; break;
        case 14: kern = k_finalize<14>; break;
        case 15: kern = k_finalize<15>; break;
        case 16: kern = k_finalize<16>; break;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, ctx->stream, ctx->x_orig, ctx->d, ctx->own_lo, ctx->own_hi,
                       ctx->k, ctx->ks, ctx->knn_e, nnd_vertex_order(ctx), out_idx_dev, out_dist_dev);
    NND_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- debug / parity: the MFMA Gram tile on arbitrary row lists (tests/test_gpu_kernels.py) ----
// one wave per 16x16 output tile; operands come straight from global memory with the same K mapping
// as gram.h (chunk c of a row feeds lane group c & 3).
// (the body of k_pairwise; FAM: NND_CODES_ANY, or NND_CODES_BOOL for the boolean family: metric.h nnd_metric_family)
template <int FAM>
__device__ __forceinline__ void fin_pairwise_body(const float *__restrict__ xp, int dp, const float *__restrict__ nrm,
                                                 int metric, const int32_t *__restrict__ rows_a, int na,
                                                 const int32_t *__restrict__ rows_b, int nb, float *__restrict__ out) {
    const int lane = nnd_lane(), r16 = lane & 15, g = lane >> 4;
    const int ta = blockIdx.y, tb = blockIdx.x;
    int ia = ta * 16 + r16, ib = tb * 16 + r16;
    int ida = ia < na ? rows_a[ia] : -1, idb = ib < nb ? rows_b[ib] : -1;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < (dp >> 4); t++) {
        int c = 4 * t + g;
        float4 a = ida >= 0 ? *(const float4 *)(xp + (int64_t)ida * dp + 4 * c) : make_float4(0, 0, 0, 0);
        float4 b = idb >= 0 ? *(const float4 *)(xp + (int64_t)idb * dp + 4 * c) : make_float4(0, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    }
    int col = tb * 16 + r16;
    float nbv = idb >= 0 ? nrm[idb] : 0.0f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int row = ta * 16 + 4 * g + r;
        int idr = row < na ? rows_a[row] : -1;
        if (row < na && col < nb) out[(int64_t)row * nb + col] = nnd_gram_to_dist<FAM>(metric, acc[r], idr >= 0 ? nrm[idr] : 0.0f, nbv);
    }
}
template <int FAM>
__global__ __launch_bounds__(64) void k_pairwise(const float *__restrict__ xp, int dp, const float *__restrict__ nrm,
                                                 int metric, const int32_t *__restrict__ rows_a, int na,
                                                 const int32_t *__restrict__ rows_b, int nb, float *__restrict__ out) {
    fin_pairwise_body<FAM>(xp, dp, nrm, metric, rows_a, na, rows_b, nb, out);
}

int nnd_launch_pairwise(nnd_ctx *ctx, const int32_t *rows_a_dev, int na, const int32_t *rows_b_dev, int nb, float *out_dev) {
    dim3 grid((nb + 15) / 16, (na + 15) / 16);
    hipLaunchKernelGGL(nnd_metric_bool(ctx->p.metric) ? k_pairwise<NND_CODES_BOOL> : k_pairwise<NND_CODES_ANY>, grid, dim3(64), 0, ctx->stream, ctx->xp, ctx->dp, ctx->nrm, nnd_kmetric(ctx), rows_a_dev, na,
                       rows_b_dev, nb, out_dev);
    NND_HIP_CHECK(hipGetLastError());
    return 0;
}
