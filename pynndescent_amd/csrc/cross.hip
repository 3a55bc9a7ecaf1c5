// cross.hip -- the spanning tree: the components of the spanning forest (mst.hip) joined by their lightest cross-component
// edges under mutual reachability, searched over ALL rows of the other components on the matrix pipe.  What HDBSCAN, robust
// single linkage and every dendrogram need where the k-NN graph is not connected.  DESIGN.md section 4 "Spanning tree".
//
// Definitions (tests/spanning_tree_util.py restates them in numpy):
//   F, labels, core   exactly what the spanning forest gives for the k-lists (mst.hip)
//   d(i, j)      the float32 rounding of the float64 distance of the rows as given, in the metric's own space (the space of
//                neighbor_graph's distances): nnd_ref_acc / nnd_ref_dist of metric.h in float64, then the metric's correction
//                in float64 (none / sqrt / 1 - 2^-v), then one rounding
//   w(i, j)      for i, j in different components of F: max(core(i), core(j), d(i, j)) in float32; a pair whose d is not finite
//                is no edge
//   key          (bits of w, min(i, j), max(i, j)), the forest's rule; the weight between two components is the smallest key over
//                all their cross pairs
//   C            the unique minimum spanning tree of the complete graph of the components under the key order
//   tree         F + C, an exactly symmetric CSR matrix, zero weights stored.  NOT the minimum spanning tree of the complete
//                mutual-reachability graph: a cross edge may make a forest edge redundant.
//
// Boruvka rounds on the components, after the forest's own.  In a round every component but the largest (ties: the one with
// the smaller smallest member) asks for its smallest outgoing key -- legal by the cut property under a strict order, and the
// number of the asking components still at least halves -- so the query rows are the points outside the giant component only:
//   k_cross_sizes / _giant / _flag / _list   the sizes, the giant, the compacted query rows (a prefix sum), the counters
//   k_cross_scan<DC, TS>   tier 1.  64 query rows x a slice of the prepared rows per workgroup, f32 MFMA Gram tiles (gram.h).
//                The epilogue stays in registers: per accumulator value a LOWER BOUND lb of the pair's exact weight (the
//                kernel distance minus the rounding band of exact_band.h, carried through the metric's correction; the cores are
//                exact), the screen key (lb bits, j), and per lane and accumulator row the two smallest screen keys seen.  For a
//                fixed i the order of (w, min(i, j), max(i, j)) is the order of (w, j), so a key is one 64-bit word.  At the
//                end of the slice the 16 lanes of a row rank their smallest keys by shuffles: the row's CX_R smallest are its
//                candidates, and T is the smallest screen key left out.  No LDS queue, no list merge, no barrier beyond staging.
//   k_cross_refine<TS>     one wave per query row: the float64 distances of the slices' candidates from the ORIGINAL rows, the
//                exact keys, and the certificate: every pair left out has an exact key >= its screen key >= T (a larger exact
//                weight gives a larger key, an equal one leaves the ids to decide), so the row is final iff its smallest exact
//                candidate key lies below T.  Core-dominated ties -- the rule under mutual reachability -- keep the smallest ids
//                and certify.  A final row writes its record for k_mst_pick; the others are listed for tier 2.
//   k_cross_f64<TS>        tier 2, the definition: one workgroup per listed row over all rows of other components in float64.
//   mst_launch_join        k_mst_pick, k_mst_hook, k_mst_jump, k_mst_flatten of mst.hip: the records do not care who wrote them
// Every device loop is bounded by a number derived from the shapes; the rounds by ceil(log2 components) + 1.  The only atomics
// are integer minima, maxima and counts; every store is a vector store; the result is the same bytes on every run.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "../../include/pynnd_amd.h"
#include "common.h"
#include "metric.h"
#include "state.h"
#include "gram.h"
#include "exact_band.h"
#include "csr_graph.h"
#include "mst.h"

#define CX_QB 64  // query rows per workgroup: 16 per wave
#define CX_TB 64  // data rows per tile: four 16x16 accumulator tiles per wave
#define CX_R 4    // candidates a slice keeps per query row
#define CX_MAX_SLICES 64  // CX_R * CX_MAX_SLICES candidates per row at most: what k_cross_refine walks

// the metric's own space (TS): the kernel distance as it is (sqeuclidean), its square root (euclidean, l2), 1 - 2^-v (cosine)
enum { CX_SPACE_SQ = 0, CX_SPACE_SQRT = 1, CX_SPACE_COSINE = 2 };

struct cx_counters {  // one per round, written by the device
    unsigned long long giant;  // (size << 32 | ~smallest member) of the largest component
    int32_t n_components, n_query, n_uncertified, pad;
};

__device__ __forceinline__ uint64_t cx_shfl_xor64(uint64_t v, int o) {
    return ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64) << 32) | (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
}
__device__ __forceinline__ uint64_t cx_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t cx_key(float w, uint32_t j) { return ((uint64_t)__float_as_uint(w > 0.0f ? w : 0.0f) << 32) | j; }

// ---------------------------------------------------------------------------------------------- the query rows of a round
__global__ __launch_bounds__(256) void k_cross_clear(mst_state s, int32_t *__restrict__ size) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.m; i += (int64_t)gridDim.x * 256) {
        size[i] = 0;
        s.smallest[i] = INT_MAX;
    }
}
__global__ __launch_bounds__(256) void k_cross_sizes(mst_state s, int32_t *__restrict__ size) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.m; i += (int64_t)gridDim.x * 256) {
        const int32_t c = s.comp[i];
        atomicAdd(&size[c], 1);
        if ((int32_t)i < __hip_atomic_load(&s.smallest[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&s.smallest[c], (int32_t)i);
    }
}
__global__ __launch_bounds__(256) void k_cross_giant(mst_state s, const int32_t *__restrict__ size, cx_counters *__restrict__ ctr) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < s.m; c += (int64_t)gridDim.x * 256) {
        if (s.comp[c] != (int32_t)c) continue;
        atomicMax(&ctr->giant, ((unsigned long long)(uint32_t)size[c] << 32) | (0xFFFFFFFFu - (uint32_t)s.smallest[c]));
        atomicAdd(&ctr->n_components, 1);
    }
}
// every row is dead until k_cross_refine / k_cross_f64 give it a record
__global__ __launch_bounds__(256) void k_cross_flag(mst_state s, const cx_counters *__restrict__ ctr) {
    const int32_t giant = s.comp[0xFFFFFFFFu - (uint32_t)ctr->giant];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.m; i += (int64_t)gridDim.x * 256) {
        s.flag[i] = s.comp[i] != giant ? 1 : 0;
        s.dead[i] = 1;
    }
}
__global__ __launch_bounds__(256) void k_cross_list(mst_state s, int32_t *__restrict__ qlist, cx_counters *__restrict__ ctr) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.m; i += (int64_t)gridDim.x * 256) {
        if (s.flag[i]) qlist[s.pos[i]] = (int32_t)i;
        if (i == s.m - 1) ctr->n_query = s.pos[i] + s.flag[i];
    }
}
__global__ __launch_bounds__(256) void k_cross_fill(int32_t *__restrict__ ids, float *__restrict__ w, unsigned int *__restrict__ hooks, int64_t total, int n_hooks) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        ids[t] = -1;
        w[t] = 0.0f;
        if (t < n_hooks) hooks[t] = 0u;
    }
}
// the forest's columns and the joining rounds' side by side: what csr_build_i32 makes the tree of
__global__ __launch_bounds__(256) void k_cross_columns(int64_t m, int r1, int r2, const int32_t *__restrict__ e1, const float *__restrict__ w1, int cols1,
                                                       const int32_t *__restrict__ e2, const float *__restrict__ w2, int cols2,
                                                       int32_t *__restrict__ out_e, float *__restrict__ out_w) {
    const int cols = r1 + r2;
    const int64_t total = m * (int64_t)cols;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t i = t / cols;
        const int c = (int)(t - i * cols);
        out_e[t] = c < r1 ? e1[i * cols1 + c] : e2[i * cols2 + (c - r1)];
        out_w[t] = c < r1 ? w1[i * cols1 + c] : w2[i * cols2 + (c - r1)];
    }
}

// ---------------------------------------------------------------------------------------------- tier 1: the scan
// A float32 value that is not above the exact float32 distance d(i, j) of the pair, from the Gram value g of the prepared rows.
// band: the relative band of exact_band.h with room for the roundings made here (cx_band).  Every step rounds towards the safe
// side or is followed by a shave of 2^-22 of the value; the conversions are monotone, so a bound below the float64 distance
// stays below its float32 rounding.
template <int TS>
__device__ __forceinline__ float cx_lower_dist(float g, float na, float nb, float band) {
    if constexpr (TS == CX_SPACE_COSINE) {
        if (na == 0.0f && nb == 0.0f) return 0.0f;              // two zero rows: distance 0
        float v = (1.0f - g) - band;                            // 1 - cosine; a zero row or a cosine <= 0 is distance 1 exactly
        v = v < 1.0f ? v : 1.0f;
        return v > 0.0f ? v : 0.0f;
    } else {
        float v = nnd_clamp_dist(na + nb - 2.0f * g) - band * (na + nb);
        v -= fabsf(v) * 2.384185791015625e-07f;
        if (!(v > 0.0f)) return 0.0f;
        if constexpr (TS == CX_SPACE_SQ) return v;
        v = __fsqrt_rn(v);
        return v - v * 2.384185791015625e-07f;
    }
}

// Workgroup (bx, by): query rows qlist[64 bx ..] against data rows [c_lo, c_hi) of slice by.  Wave w owns query rows 16 w ..
// 16 w + 15; lane l holds, per accumulator tile J, rows 4 (l >> 4) + r and column 16 J + (l & 15) (gram.h).  dp <= DC: the
// query rows are staged once; above, K chunk by K chunk.  Each tile row's component and core distance are staged beside its norm.
template <int DC, int TS>
__global__ __launch_bounds__(256) void k_cross_scan(const float *__restrict__ xp, const float *__restrict__ nrm, int64_t n, int dp, float band,
                                                    const float *__restrict__ core, const int32_t *__restrict__ comp,
                                                    const int32_t *__restrict__ qlist, int nq, int nq_pad, int64_t rows_per_slice,
                                                    unsigned long long *__restrict__ out_keys, unsigned long long *__restrict__ out_t) {
    extern __shared__ __align__(16) unsigned char cx_smem[];
    float *Xs = (float *)cx_smem;                 // (CX_QB + CX_TB) rows of DC floats, swizzled: queries, then the data tile
    float *snrm = Xs + (CX_QB + CX_TB) * DC;      // (CX_TB) norm words of the tile
    float *score = snrm + CX_TB;                  // (CX_TB) core distances
    int32_t *scomp = (int32_t *)(score + CX_TB);  // (CX_TB) components, -1 past the slice
    int32_t *sq = scomp + CX_TB;                  // (CX_QB) ids of the query rows, -1 = none
    const int tid = threadIdx.x, lane = nnd_lane(), w = tid >> 6, g = lane >> 4, c16 = lane & 15;
    const int q0 = blockIdx.x * CX_QB;
    const int64_t c_lo = (int64_t)blockIdx.y * rows_per_slice;
    const int64_t c_hi = c_lo + rows_per_slice < n ? c_lo + rows_per_slice : n;
    if (tid < CX_QB) sq[tid] = q0 + tid < nq ? qlist[q0 + tid] : -1;
    __syncthreads();
    const bool multi = dp > DC;
    if (!multi) nnd_stage_rows<DC>(xp, dp, sq, CX_QB, 0, dp, Xs, tid, 256);
    float na[4], ci_core[4];
    int32_t ci[4];
    uint64_t best[4], second[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int id = sq[16 * w + 4 * g + r];
        na[r] = id >= 0 ? nrm[id] : 0.0f;
        ci_core[r] = id >= 0 ? core[id] : 0.0f;
        ci[r] = id >= 0 ? comp[id] : -1;  // (-1: no row; a tile row past the slice has -1 too, so the pair never counts)
        best[r] = second[r] = MST_EMPTY;
    }
    for (int64_t t0 = c_lo; t0 < c_hi; t0 += CX_TB) {  // (rows_per_slice / CX_TB tiles at most)
        f32x4 acc[4];
#pragma unroll
        for (int J = 0; J < 4; J++) acc[J] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < dp; c0 += DC) {
            const int cw = dp - c0 < DC ? dp - c0 : DC;
            __syncthreads();  // the operand reads of the previous chunk / tile are done
            if (multi) nnd_stage_rows<DC>(xp, dp, sq, CX_QB, c0, cw, Xs, tid, 256);
            const int nch = cw >> 2, total = CX_TB * nch;
#pragma unroll 4
            for (int idx = tid; idx < total; idx += 256) {
                const int r = idx / nch, ch = idx - r * nch;
                const int64_t row = t0 + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < c_hi) v = *(const float4 *)(xp + row * dp + c0 + 4 * ch);
                *(float4 *)&Xs[nnd_swz<DC>(CX_QB + r, ch)] = v;
            }
            if (c0 == 0 && tid < CX_TB) {
                const bool in = t0 + tid < c_hi;
                snrm[tid] = in ? nrm[t0 + tid] : 0.0f;
                score[tid] = in ? core[t0 + tid] : 0.0f;
                scomp[tid] = in ? comp[t0 + tid] : -1;
            }
            __syncthreads();
            nnd_gram_chunk<DC, 4>(Xs, 16 * w, CX_QB, cw, acc, [](int) { return true; });
        }
#pragma unroll
        for (int J = 0; J < 4; J++) {
            const int col = 16 * J + c16;
            const uint32_t cid = (uint32_t)(t0 + col);
            const float nb = snrm[col], cj_core = score[col];
            const int32_t cj = scomp[col];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const float lb = fmaxf(fmaxf(ci_core[r], cj_core), cx_lower_dist<TS>(acc[J][r], na[r], nb, band));
                const uint64_t key = (cj != ci[r] && cj >= 0 && ci[r] >= 0) ? cx_key(lb, cid) : MST_EMPTY;
                const uint64_t lo = cx_min64(key, best[r]), hi = key < best[r] ? best[r] : key;
                best[r] = lo;
                second[r] = cx_min64(second[r], hi);
            }
        }
    }
    // the 16 lanes of a row rank their smallest keys (empty keys tie: the lane decides), the row's CX_R smallest are its
    // candidates, T the smallest of everything else
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint64_t b = best[r];
        int rank = 0;
#pragma unroll
        for (int t = 1; t < 16; t++) {
            const uint64_t o = cx_shfl_xor64(b, t);
            rank += (o < b || (o == b && (c16 ^ t) < c16)) ? 1 : 0;
        }
        const size_t row = (size_t)blockIdx.y * nq_pad + q0 + 16 * w + 4 * g + r;
        if (rank < CX_R) out_keys[row * CX_R + rank] = b;
        uint64_t t = rank < CX_R ? second[r] : cx_min64(b, second[r]);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) t = cx_min64(t, cx_shfl_xor64(t, o));
        if (c16 == 0) out_t[row] = t;
    }
}

// ---------------------------------------------------------------------------------------------- exact weights
// d(i, j) by the 16 lanes of a group: the float64 sums of k_exact_refine (lane l takes coordinates l, l + 16, ..), the metric's
// correction in float64, one rounding
template <int TS>
__device__ __forceinline__ float cx_true_dist(const float *__restrict__ xa, const float *__restrict__ xb, int d, int l16) {
    constexpr int code = TS == CX_SPACE_COSINE ? 1 : 0;
    double dot = 0.0, nx = 0.0, ny = 0.0;
    for (int t = l16; t < d; t += 16) nnd_ref_acc<NND_CODES_01, NND_HELLINGER_F64>(code, (double)xa[t], (double)xb[t], dot, nx, ny);
    const double dt = nnd_group_sum_f64<16>(dot);
    const double ax = code == 0 ? 0.0 : nnd_group_sum_f64<16>(nx), ay = code == 0 ? 0.0 : nnd_group_sum_f64<16>(ny);
    const double r = nnd_ref_dist<NND_CODES_01>(code, dt, ax, ay);
    if constexpr (TS == CX_SPACE_SQ) return (float)r;
    if constexpr (TS == CX_SPACE_SQRT) return (float)sqrt(r);
    return (float)(1.0 - exp2(-r));
}
// the exact key of the pair for row i: (bits of max(core(i), core(j), d), j); no key where d is not finite
__device__ __forceinline__ uint64_t cx_exact_key(float dist, float core_i, float core_j, uint32_t j) {
    if (!(dist < INFINITY)) return MST_EMPTY;  // (a NaN too)
    return cx_key(fmaxf(fmaxf(core_i, core_j), dist), j);
}
// row i's record for k_mst_pick and its component's offer; key: (w bits, j) of its smallest outgoing pair, or none
__device__ __forceinline__ void cx_write_record(const mst_state &s, uint32_t i, int32_t ci, uint64_t key) {
    if (key == MST_EMPTY) return;  // (the row stays dead: nothing finite leaves its component)
    const uint32_t j = (uint32_t)key, lo = i < j ? i : j, hi = i < j ? j : i;
    const unsigned long long k1 = (key & 0xFFFFFFFF00000000ull) | lo;
    s.rec1[i] = k1;
    s.rec2[i] = hi;
    s.dead[i] = 0;
    atomicMin(&s.best1[ci], k1);
}

// one wave per query row: the slices' candidates in float64, the certificate, the record or the tier-2 list
template <int TS>
__global__ __launch_bounds__(256) void k_cross_refine(const float *__restrict__ x, int d, const float *__restrict__ core, const int32_t *__restrict__ qlist, int nq,
                                                      int nq_pad, int n_slices, const unsigned long long *__restrict__ keys,
                                                      const unsigned long long *__restrict__ ts, mst_state s, int force,
                                                      int32_t *__restrict__ uncert, cx_counters *__restrict__ ctr) {
    const int lane = nnd_lane(), grp = lane >> 4, l16 = lane & 15;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;  // wave-uniform
    const uint32_t i = (uint32_t)qlist[q];
    const float *xa = x + (int64_t)i * d;
    const float core_i = core[i];
    const int total = n_slices * CX_R;  // <= CX_MAX_SLICES * CX_R
    uint64_t bestk = MST_EMPTY;
    for (int c0 = 0; c0 < total; c0 += 4) {
        const int c = c0 + grp;
        const uint64_t key = c < total ? keys[((size_t)(c / CX_R) * nq_pad + q) * CX_R + (c % CX_R)] : MST_EMPTY;
        const bool on = key != MST_EMPTY;
        const uint32_t j = on ? (uint32_t)key : 0u;
        const float dist = cx_true_dist<TS>(xa, x + (int64_t)j * d, d, l16);
        if (on) bestk = cx_min64(bestk, cx_exact_key(dist, core_i, core[j], j));
    }
    uint64_t t = MST_EMPTY;
    for (int sl = lane; sl < n_slices; sl += 64) t = cx_min64(t, ts[(size_t)sl * nq_pad + q]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bestk = cx_min64(bestk, cx_shfl_xor64(bestk, o));
        t = cx_min64(t, cx_shfl_xor64(t, o));
    }
    if (lane != 0) return;
    if (force || !(bestk < t || t == MST_EMPTY)) uncert[atomicAdd(&ctr->n_uncertified, 1)] = q;
    else cx_write_record(s, i, s.comp[i], bestk);
}

// ---------------------------------------------------------------------------------------------- tier 2: the definition
// one workgroup per listed row; group gg of 16 lanes takes rows gg, gg + 16, .. of the whole set, in float64
template <int TS>
__global__ __launch_bounds__(256) void k_cross_f64(const float *__restrict__ x, int64_t n, int d, const float *__restrict__ core,
                                                   const int32_t *__restrict__ qlist, const int32_t *__restrict__ uncert,
                                                   const cx_counters *__restrict__ ctr, mst_state s) {
    __shared__ unsigned long long sbest[4];
    if ((int)blockIdx.x >= ctr->n_uncertified) return;  // block-uniform
    const int lane = nnd_lane(), gg = threadIdx.x >> 4, l16 = lane & 15;
    const uint32_t i = (uint32_t)qlist[uncert[blockIdx.x]];
    const float *xa = x + (int64_t)i * d;
    const float core_i = core[i];
    const int32_t ci = s.comp[i];
    uint64_t bestk = MST_EMPTY;
    for (int64_t j0 = 0; j0 < n; j0 += 16) {
        const int64_t j = j0 + gg;
        const bool on = j < n && s.comp[j < n ? j : 0] != ci;
        const float dist = cx_true_dist<TS>(xa, x + (on ? j : 0) * d, d, l16);
        if (on) bestk = cx_min64(bestk, cx_exact_key(dist, core_i, core[j], (uint32_t)j));
    }
#pragma unroll
    for (int o = 32; o >= 16; o >>= 1) bestk = cx_min64(bestk, cx_shfl_xor64(bestk, o));
    if (lane == 0) sbest[threadIdx.x >> 6] = bestk;
    __syncthreads();
    if (threadIdx.x == 0) cx_write_record(s, i, ci, cx_min64(cx_min64(sbest[0], sbest[1]), cx_min64(sbest[2], sbest[3])));
}

// ---------------------------------------------------------------------------------------------- host side
namespace {
// data slices of the scan: about 1024 workgroups where the query blocks alone do not fill the chip, whole tiles, at most
// CX_MAX_SLICES (the rule of nnd_exact_slices_for, without its batches)
int cx_slices_for(int64_t n, int64_t nq) {
    const int64_t nqb = (nq + CX_QB - 1) / CX_QB, ntiles = (n + CX_TB - 1) / CX_TB;
    int64_t sl = nqb > 0 ? (1024 + nqb - 1) / nqb : 1;
    if (sl > CX_MAX_SLICES) sl = CX_MAX_SLICES;
    if (sl > ntiles) sl = ntiles;
    if (sl < 1) sl = 1;
    const int64_t tps = (ntiles + sl - 1) / sl;
    return (int)((ntiles + tps - 1) / tps);
}
// the band as cx_lower_dist takes it: exact_band.h's, widened for the float32 arithmetic that applies it
float cx_band(int space, int d, int dp) {
    if (dp > NND_EXACT_DP_MAX) return INFINITY;
    if (space == CX_SPACE_COSINE) return (float)(nnd_exact_band_unit(d, dp) * 1.01 + 8.0 * NND_EXACT_U);
    return (float)(nnd_exact_band_sqeuclid(dp, 0.5, 0.5) * 1.001);  // per unit of na + nb
}

template <int DC, int TS>
int cx_launch_scan_dc(csr_err &err, hipStream_t st, dim3 grid, const nnd_ctx *ctx, float band, const float *core, const int32_t *comp, const int32_t *qlist, int nq,
                      int nq_pad, int64_t rows_per_slice, unsigned long long *keys, unsigned long long *ts) {
    const size_t lds = sizeof(float) * ((CX_QB + CX_TB) * DC + 2 * CX_TB) + sizeof(int32_t) * (CX_TB + CX_QB);
    auto kern = k_cross_scan<DC, TS>;
    if (lds > 48 * 1024) CSR_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, (const float *)ctx->xp, (const float *)ctx->nrm, ctx->n, ctx->dp, band, core, comp, qlist, nq, nq_pad,
                       rows_per_slice, keys, ts);
    CSR_HIP(hipGetLastError());
    return 0;
}
template <int TS>
int cx_launch_scan(csr_err &err, hipStream_t st, dim3 grid, const nnd_ctx *ctx, float band, const float *core, const int32_t *comp, const int32_t *qlist, int nq,
                   int nq_pad, int64_t rows_per_slice, unsigned long long *keys, unsigned long long *ts) {
    if (ctx->dp <= 32) return cx_launch_scan_dc<32, TS>(err, st, grid, ctx, band, core, comp, qlist, nq, nq_pad, rows_per_slice, keys, ts);
    if (ctx->dp <= 64) return cx_launch_scan_dc<64, TS>(err, st, grid, ctx, band, core, comp, qlist, nq, nq_pad, rows_per_slice, keys, ts);
    return cx_launch_scan_dc<128, TS>(err, st, grid, ctx, band, core, comp, qlist, nq, nq_pad, rows_per_slice, keys, ts);
}

// the sizes, the giant and the query rows of the components as s.comp has them, into *ctr and qlist
int cx_query_rows(csr_err &err, hipStream_t st, mst_work &w, int32_t *size, int32_t *qlist, cx_counters *ctr) {
    mst_state &s = w.s;
    const dim3 grid(mst_grid(s.m, 256)), block(256);
    hipLaunchKernelGGL(k_cross_clear, grid, block, 0, st, s, size);
    hipLaunchKernelGGL(k_cross_sizes, grid, block, 0, st, s, size);
    hipLaunchKernelGGL(k_cross_giant, grid, block, 0, st, s, (const int32_t *)size, ctr);
    hipLaunchKernelGGL(k_cross_flag, grid, block, 0, st, s, (const cx_counters *)ctr);
    CSR_HIP(rocprim::exclusive_scan(w.scan_tmp, w.scan_bytes, (const int32_t *)s.flag, s.pos, (int32_t)0, (size_t)s.m, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(k_cross_list, grid, block, 0, st, s, qlist, ctr);
    CSR_HIP(hipGetLastError());
    return 0;
}

template <int TS>
int cx_round(csr_err &err, nnd_scratch &tmp, hipStream_t st, const nnd_ctx *ctx, const float *core, mst_state &s, const int32_t *qlist, int nq, int force,
             cx_counters *ctr, nnd_tree_stats *stats) {
    const int64_t n = ctx->n;
    const int nq_pad = (nq + CX_QB - 1) / CX_QB * CX_QB, S = cx_slices_for(n, nq);
    const int64_t ntiles = (n + CX_TB - 1) / CX_TB, rows_per_slice = (ntiles + S - 1) / S * CX_TB;
    unsigned long long *keys = tmp.get<unsigned long long>(&err, (size_t)S * nq_pad * CX_R), *ts = tmp.get<unsigned long long>(&err, (size_t)S * nq_pad);
    int32_t *uncert = tmp.get<int32_t>(&err, (size_t)nq_pad);
    if (!keys || !ts || !uncert) return 1;
    const dim3 grid((unsigned)(nq_pad / CX_QB), (unsigned)S);
    if (cx_launch_scan<TS>(err, st, grid, ctx, cx_band(TS, ctx->d, ctx->dp), core, s.comp, qlist, nq, nq_pad, rows_per_slice, keys, ts)) return 1;
    hipLaunchKernelGGL(k_cross_refine<TS>, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, ctx->x_orig, ctx->d, core, qlist, nq, nq_pad, S,
                       (const unsigned long long *)keys, (const unsigned long long *)ts, s, force, uncert, ctr);
    hipLaunchKernelGGL(k_cross_f64<TS>, dim3((unsigned)nq), dim3(256), 0, st, ctx->x_orig, n, ctx->d, core, qlist, (const int32_t *)uncert,
                       (const cx_counters *)ctr, s);
    CSR_HIP(hipGetLastError());
    if (S > stats->slices) stats->slices = S;
    stats->mfma += (int64_t)grid.x * (rows_per_slice / CX_TB) * S * 16 * (ctx->dp / 4);
    return 0;
}

int cx_build(csr_err &err, nnd_scratch &tmp, nnd_csr_s &sym, nnd_ctx *ctx, nnd_csr_s *g, const void *ids, int32_t id_bytes, const float *dists, int32_t k,
             int64_t ld_ids, int64_t ld_dists, int32_t min_samples, int space, float *core, nnd_tree_stats *stats) {
    hipStream_t st = ctx->stream;
    const int64_t m = ctx->n;
    const int force = (ctx->p.flags & NND_FLAG_TEST_TREE_F64) ? 1 : 0;
    mst_work w;
    int r1 = 0;
    if (mst_forest_rounds(err, tmp, sym, st, ids, id_bytes, dists, m, k, ld_ids, ld_dists, min_samples, core, w, &r1)) return 1;
    stats->forest_rounds = r1;
    const int max_rounds = mst_ceil_log2(m) + 1;
    int32_t *size = tmp.get<int32_t>(&err, (size_t)m), *qlist = tmp.get<int32_t>(&err, (size_t)m);
    cx_counters *ctr = tmp.get<cx_counters>(&err, (size_t)max_rounds + 2);
    if (!size || !qlist || !ctr) return 1;
    CSR_HIP(hipMemsetAsync(ctr, 0, sizeof(cx_counters) * ((size_t)max_rounds + 2), st));
    if (cx_query_rows(err, st, w, size, qlist, ctr)) return 1;
    cx_counters now[2];
    CSR_HIP(hipMemcpyAsync(&now[1], ctr, sizeof(cx_counters), hipMemcpyDeviceToHost, st));
    CSR_HIP(hipStreamSynchronize(st));
    stats->n_components = now[1].n_components;
    stats->query_rows = now[1].n_query;
    int nq = now[1].n_query, r2 = 0;
    mst_state s2 = w.s;  // the joining rounds: the forest's state with edge columns and counters of their own
    s2.cols = now[1].n_components > 1 ? mst_ceil_log2(now[1].n_components) + 1 : 1;
    const size_t slots = (size_t)m * (size_t)s2.cols;
    s2.edge_ids = tmp.get<int32_t>(&err, slots);
    s2.edge_w = tmp.get<float>(&err, slots);
    s2.hooks = tmp.get<unsigned int>(&err, (size_t)s2.cols + 1);
    if (!s2.edge_ids || !s2.edge_w || !s2.hooks) return 1;
    if (nq > 0) hipLaunchKernelGGL(k_cross_fill, dim3(mst_grid((int64_t)slots, 256)), dim3(256), 0, st, s2.edge_ids, s2.edge_w, s2.hooks, (int64_t)slots, s2.cols + 1);
    while (nq > 0) {  // (s2.cols rounds at most)
        if (r2 >= s2.cols) { err.set_error("nnd_spanning_tree: more than %d rounds (%d components)", (int)s2.cols, (int)stats->n_components); return 1; }
        stats->query_rows_all += nq;
        int rc;
        if (space == CX_SPACE_SQ) rc = cx_round<CX_SPACE_SQ>(err, tmp, st, ctx, core, s2, qlist, nq, force, ctr + r2, stats);
        else if (space == CX_SPACE_SQRT) rc = cx_round<CX_SPACE_SQRT>(err, tmp, st, ctx, core, s2, qlist, nq, force, ctr + r2, stats);
        else rc = cx_round<CX_SPACE_COSINE>(err, tmp, st, ctx, core, s2, qlist, nq, force, ctr + r2, stats);
        if (rc) return 1;
        mst_launch_join(st, s2, r2);
        w.s.comp = s2.comp;  // (the query rows are counted on the new components)
        w.s.comp_next = s2.comp_next;
        if (cx_query_rows(err, st, w, size, qlist, ctr + r2 + 1)) return 1;
        unsigned int hooks[2] = {0u, 0u};  // this round's count, and the word the pointer jumping reports a cycle in
        CSR_HIP(hipMemcpyAsync(now, ctr + r2, 2 * sizeof(cx_counters), hipMemcpyDeviceToHost, st));
        CSR_HIP(hipMemcpyAsync(hooks, s2.hooks + r2, sizeof(hooks), hipMemcpyDeviceToHost, st));
        CSR_HIP(hipStreamSynchronize(st));
        const unsigned int hooked = hooks[0];
        if ((hooks[0] | hooks[1]) & MST_FAULT) { err.set_error("nnd_spanning_tree: round %d met a loop bound (m = %lld)", r2, (long long)m); return 1; }
        stats->tier2_rows += now[0].n_uncertified;
        if (hooked == 0) break;  // components without a finite weight between them stay apart
        r2++;
        nq = now[1].n_query;
    }
    stats->rounds = r2;
    if (r2 == 0) return csr_build_i32(err, tmp, st, g, w.s.edge_ids, w.s.edge_w, m, r1 > 0 ? r1 : 1, w.s.cols, m, 1, csr_combine());
    const size_t all = (size_t)m * (size_t)(r1 + r2);
    int32_t *all_e = tmp.get<int32_t>(&err, all);
    float *all_w = tmp.get<float>(&err, all);
    if (!all_e || !all_w) return 1;
    hipLaunchKernelGGL(k_cross_columns, dim3(mst_grid((int64_t)all, 256)), dim3(256), 0, st, m, r1, r2, (const int32_t *)w.s.edge_ids, (const float *)w.s.edge_w,
                       (int)w.s.cols, (const int32_t *)s2.edge_ids, (const float *)s2.edge_w, (int)s2.cols, all_e, all_w);
    CSR_HIP(hipGetLastError());
    return csr_build_i32(err, tmp, st, g, all_e, all_w, m, r1 + r2, r1 + r2, m, 1, csr_combine());
}

// the checks of both entries; *space: the metric's own space
int cx_check(nnd_ctx *ctx, const char *who, const void *ids, int32_t id_bytes, const float *dists, int32_t k, int64_t ld_ids, int64_t ld_dists, int32_t min_samples,
             int32_t euclidean, const float *core, int *space) {
    csr_err err;
    if (ctx->p.metric != NND_METRIC_SQEUCLIDEAN && ctx->p.metric != NND_METRIC_ALT_COSINE) {
        ctx->set_error("%s: the spanning tree covers the metric codes 0 (sqeuclidean, euclidean) and 1 (cosine), not %d", who, (int)ctx->p.metric);
        return 1;
    }
    if (!ctx->x_orig || !ctx->x_valid) { ctx->set_error("%s: no data set (call nnd_set_data_host/device first)", who); return 1; }
    if (ctx->n_ranks > 0) { ctx->set_error("%s: the handle is a shard of a multi-GPU build", who); return 1; }
    if (mst_check(err, who, ids, id_bytes, dists, ctx->n, k, ld_ids, ld_dists, min_samples, (const int32_t *)core, core)) { ctx->set_error("%s", err.msg); return 1; }
    *space = ctx->p.metric == NND_METRIC_ALT_COSINE ? CX_SPACE_COSINE : (euclidean ? CX_SPACE_SQRT : CX_SPACE_SQ);
    return 0;
}

int cx_run(nnd_ctx *ctx, nnd_csr_s *g, const void *ids, int32_t id_bytes, const float *dists, int32_t k, int64_t ld_ids, int64_t ld_dists, int32_t min_samples,
           int space, float *core, nnd_tree_stats *stats) {
    csr_err err;
    err.msg[0] = 0;
    nnd_scratch tmp;  // released on return, behind the synchronise below
    nnd_csr_s sym;    // the symmetric mutual-reachability matrix: likewise
    nnd_tree_stats st{};
    int rc;
    if (ctx->n == 0) rc = csr_build_i32(err, tmp, ctx->stream, g, nullptr, nullptr, 0, 1, 1, 1, 0, csr_combine());
    else rc = cx_build(err, tmp, sym, ctx, g, ids, id_bytes, dists, k, ld_ids, ld_dists, min_samples, space, core, &st);
    const hipError_t e = hipStreamSynchronize(ctx->stream);  // (on every path: the scratch goes when this returns)
    if (rc) { ctx->set_error("%s", err.msg); return 1; }
    if (e != hipSuccess) { (void)hipGetLastError(); ctx->set_error("nnd_spanning_tree: a kernel failed: %s", hipGetErrorString(e)); return 1; }
    if (stats) *stats = st;
    return 0;
}
}  // namespace

extern "C" int32_t nnd_spanning_tree_device(nnd_handle_t ctx, const void *ids_dev, int32_t id_bytes, const float *dists_dev, int32_t k, int64_t ld_ids,
                                            int64_t ld_dists, int32_t min_samples, int32_t euclidean, float *core_dev, nnd_tree_stats *stats,
                                            nnd_csr_t *out) {
    if (!ctx) { nnd_set_global_error("null handle"); return 1; }
    if (!out) { ctx->set_error("nnd_spanning_tree_device: null pointer"); return 1; }
    *out = nullptr;
    if (ctx->p.flags & NND_FLAG_NO_PREP) { ctx->set_error("nnd_spanning_tree_device: this handle holds no prepared rows (NND_FLAG_NO_PREP)"); return 1; }
    int space = 0;
    if (cx_check(ctx, "nnd_spanning_tree_device", ids_dev, id_bytes, dists_dev, k, ld_ids, ld_dists, min_samples, euclidean, core_dev, &space)) return 1;
    NND_HIP_CHECK(hipSetDevice(ctx->p.device));
    nnd_csr_s *g = new nnd_csr_s();
    g->device = ctx->p.device;
    if (cx_run(ctx, g, ids_dev, id_bytes, dists_dev, k, ld_ids, ld_dists, min_samples, space, core_dev, stats)) {
        delete g;
        return 1;
    }
    *out = g;
    return 0;
}

extern "C" int32_t nnd_spanning_tree(nnd_handle_t ctx, const void *ids, int32_t id_bytes, const float *dists, int32_t k, int32_t min_samples, int32_t euclidean,
                                     float *core, nnd_tree_stats *stats, int64_t *indptr, int32_t *indices, float *data, int64_t capacity, int64_t *nnz) {
    if (!ctx) { nnd_set_global_error("null handle"); return 1; }
    if (ctx->p.flags & NND_FLAG_NO_PREP) { ctx->set_error("nnd_spanning_tree: this handle holds no prepared rows (NND_FLAG_NO_PREP)"); return 1; }
    int space = 0;
    if (cx_check(ctx, "nnd_spanning_tree", ids, id_bytes, dists, k, k, k, min_samples, euclidean, core, &space)) return 1;
    if (!indptr || !nnz || capacity < 0 || (capacity > 0 && (!indices || !data))) { ctx->set_error("nnd_spanning_tree: null pointer"); return 1; }
    NND_HIP_CHECK(hipSetDevice(ctx->p.device));
    const int64_t m = ctx->n;
    nnd_csr_s g;
    g.device = ctx->p.device;
    nnd_scratch up;
    const size_t places = (size_t)m * (size_t)k;
    unsigned char *ids_dev = up.get<unsigned char>(ctx, places * (size_t)id_bytes);
    float *dists_dev = up.get<float>(ctx, places), *core_dev = up.get<float>(ctx, (size_t)m);
    if (!ids_dev || !dists_dev || !core_dev) return 1;
    if (places > 0) {
        NND_HIP_CHECK(hipMemcpyAsync(ids_dev, ids, places * (size_t)id_bytes, hipMemcpyHostToDevice, ctx->stream));
        NND_HIP_CHECK(hipMemcpyAsync(dists_dev, dists, places * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    }
    if (cx_run(ctx, &g, ids_dev, id_bytes, dists_dev, k, k, k, min_samples, space, core_dev, stats)) return 1;
    *nnz = g.nnz;
    if (g.nnz > capacity) { ctx->set_error("nnd_spanning_tree: %lld entries, room for %lld", (long long)g.nnz, (long long)capacity); return 1; }
    if (m > 0) NND_HIP_CHECK(hipMemcpy(core, core_dev, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
    NND_HIP_CHECK(hipMemcpy(indptr, g.indptr, sizeof(int64_t) * (size_t)(m + 1), hipMemcpyDeviceToHost));
    if (g.nnz > 0) {
        NND_HIP_CHECK(hipMemcpy(indices, g.indices, sizeof(int32_t) * (size_t)g.nnz, hipMemcpyDeviceToHost));
        NND_HIP_CHECK(hipMemcpy(data, g.data, sizeof(float) * (size_t)g.nnz, hipMemcpyDeviceToHost));
    }
    return 0;
}
