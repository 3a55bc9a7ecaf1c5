// query.hip -- batched k-NN queries against a prepared index: tree descent + best-first graph search.
//
// Replaces the search closure of NNDescent._init_search_function (reference pynndescent_.py:1793-1883), the tree
// descent select_side / search_flat_tree (rp_trees.py:2662-2741) and the final deheap_sort (utils.py:189-218) for
// dense float32 data with the euclidean / cosine / dot / inner-product / correlation / hellinger metrics.  The reference walks one query at a time (optionally one
// numba thread per query); here ONE WAVE owns one query:
//   * result list: the k best (distance, vertex) pairs, sorted ascending, one entry per lane (k <= 64; two per lane up to k = 128) -- the
//     reference's max-heap of size k (simple_heap_push, utils.py:352-406): a candidate enters iff it beats the worst
//     entry, the worst leaves; insertion = one ballot (rank) + one lane shift;
//   * frontier (`seed_set`, a heapq in the reference): (distance, vertex) pairs in LDS, pop-min by a wave reduction.
//     Entries at or beyond the current distance bound can never be expanded (the bound only shrinks), so they are
//     dropped when the array fills up;
//   * visited set (a bitset over all n points in the reference, utils.py:323-349): a hash set in LDS (open addressing);
//   * distances: a quad (4 lanes) per candidate, 16 candidates of an adjacency row per step, rows gathered from HBM,
//     the query vector in LDS; float32 in the reference's formulas (distances.py:63-91, 583-630) on the RAW rows --
//     cosine queries are normalised first (pynndescent_.py:1808-1815), data rows are not.  The other metrics (codes 2..5)
//     work on prepared rows, as the build does (metric.h nnd_gram_to_dist): the searcher's copy of the data gets the
//     metric's transform once (k_searcher_prep_rows), each query gets it in the kernel (dot: normalised, a zero query is
//     skipped as for cosine; correlation: centred, then normalised; hellinger: sqrt, then normalised; inner product: raw);
//   * stop rule: the nearest unexpanded frontier vertex is farther than
//         bound = worst + epsilon * (worst - min_distance)                         (pynndescent_.py:1850-1853).
//   * quantization="uint8" (Q8 instances, euclidean / cosine / dot): the walk runs on the searcher's uint8 code rows with
//     the reference's proxy distances (q_quad_proxy) and keeps search_k = proxy_beam_size * k results; its epilogue is
//     the reference's rerank (pynndescent_.py:776-789): exact distances of the RAW query to the float rows of those
//     candidates, pushed in ascending proxy order into a list of k (DESIGN.md "Quantized search").
//   * metric="proxy_inner_product" (RR instances without Q8, code 6): the walk runs on the float rows with the proxy
//     -log2(cos) + 1 / sqrt<q,x> and keeps search_k results; the same epilogue reranks them by -<q,x> (DESIGN.md "Proxy
//     distances").
// Random choices (ties in the tree descent, random start vertices when the tree leaf holds fewer than
// min(k, n_neighbors) points) come from the counter hash, keyed by the query's number.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "common.h"
#include "metric.h"
#include "devmem.h"
#include "../../include/pynnd_amd.h"

// devarray.hip: rows of NND_DTYPE_* `dtype` gathered by `order` (nullptr: identity) into float32 rows of dp floats, zero padded
int nnd_launch_gather_rows(hipStream_t st, const void *src, int dtype, const int32_t *order, int64_t n, int d, int dp, float *dst);

#define Q_FRONTIER 512   // frontier entries per query (LDS tier)
#define Q_VISITED 4096   // visited-set slots per query (power of two; LDS tier)
#define Q_VISITED_MAX 3400  // entries after which the LDS set counts as full
#define Q_BIG_FRONTIER 65536  // frontier entries per query of the global-memory tier
#define Q_BIG_BATCH 256       // queries per launch of the global-memory tier (scratch = batch * (n / 8 + 512 KB))
// Two tiers.  The LDS tier (visited = hash set of Q_VISITED_MAX vertices, frontier of Q_FRONTIER entries) covers what a
// search with the usual k / epsilon touches.  A query that would overflow either structure is NOT answered from a
// truncated search: the wave raises the query's flag and stops, and the host re-runs exactly those queries on the
// global-memory tier -- visited = a bitset over all n points (the reference's own structure, utils.py:323-349), frontier
// of Q_BIG_FRONTIER entries in HBM -- so no result ever comes from a search the reference would have continued.
#define Q_CHUNK 64       // candidates handled per step
#define Q_EMPTY 0xFFFFFFFFu

struct nnd_searcher_s {
    int device = 0;
    int64_t n = 0, nnz = 0, n_nodes = 0;
    int d = 0, dp = 0, metric = 0, n_neighbors = 0;
    float min_distance = 0.0f;
    uint32_t seed = 0;
    float *x = nullptr;        // (n, dp) rows padded to a multiple of 4 floats
    float *xn2 = nullptr;      // (n) squared norms (cosine; the prepared rows' for the codes 2..5)
    uint8_t *codes = nullptr;  // quantization="uint8": (n, dcs) codes, rows padded to 16 bytes with code 0
    float *cn2 = nullptr;      // (n) sum of LUT[c]^2 over a code row (cosine / dot)
    float *lut = nullptr;      // 512: the walk's codebook (256, padded with the last value), then the search table (+inf padded)
    int dcs = 0;               // code row stride: d rounded up to 16
    float tab_host[512];       // the host side of `lut` (the source of its stream-ordered upload)
    int32_t *indptr = nullptr, *indices = nullptr;
    float *hyper = nullptr, *offsets = nullptr;  // (n_nodes, dp), (n_nodes)
    int32_t *children = nullptr, *tree_idx = nullptr;
    hipStream_t stream = nullptr;
    int64_t last_spilled = 0;  // queries of the last call that ran on the global-memory tier
    bool force_big = false;    // nnd_searcher_set_tier(1): every query on the global-memory tier (tests)
    uint32_t *allow = nullptr;            // the filter's bitset over the searcher's numbering, (n + 31) / 32 words (allocated on first use)
    unsigned long long *fstat = nullptr;  // 2: allowed rows of the last filter, its out-of-range flag
    bool filter_on = false;               // nnd_searcher_set_filter*: the query entries run the filtered instances
    uint64_t *tags = nullptr;             // nnd_searcher_set_tags*: (n) tag words in the searcher's numbering (the tagged query entries)
    nnd_devmem mem;            // owner of the device buffers above (devmem.h)
    char err[512] = {0};
    void set_error(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, sizeof(err), fmt, ap);
        va_end(ap);
    }
};

static thread_local char g_serr[512] = {0};

// sum over the four lanes of a quad, in every one of them (two DPP quad permutes)
__device__ __forceinline__ float q_quad_sum(float acc) {
    acc += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0xB1, 0xF, 0xF, false));
    acc += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(acc), 0x4E, 0xF, 0xF, false));
    return acc;
}
// quad-cooperative <q, x_v> of the query (LDS, dp floats) and the float row `v`, lane `sub` of the quad taking every fourth
// 16-byte chunk; SQDIFF: its sibling |q - x_v|^2 (code 0).  Every float distance below starts from it; the rerank instances of
// code 6 take both of theirs from the plain product -- the walk's proxy nnd_gram_to_dist<NND_CODE_6>(<q,x>, |q|^2, |x|^2) and
// the rerank's true distance -<q,x> (inner_product, the reference's _true_distance_func), neither clamped nor corrected
template <bool SQDIFF = false>
__device__ __forceinline__ float q_quad_dot(const float *__restrict__ x, int dp, const float *qs, int64_t v, int sub) {
    const float4 *row = (const float4 *)(x + v * dp);
    const float4 *q4 = (const float4 *)qs;
    float acc = 0.0f;
    for (int c = sub; c < (dp >> 2); c += 4) {
        const float4 a = row[c], b = q4[c];
        if constexpr (SQDIFF) {
            const float d0 = b.x - a.x, d1 = b.y - a.y, d2 = b.z - a.z, d3 = b.w - a.w;
            acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        } else {
            acc += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
        }
    }
    return q_quad_sum(acc);
}

// quad-cooperative alt-space distance between the query (LDS, dp floats, |q|^2 = qn2) and row `v`
__device__ __forceinline__ float q_quad_dist(const float *__restrict__ x, const float *__restrict__ xn2, int dp, int metric,
                                             const float *qs, float qn2, int64_t v, int sub) {
    if (metric == 0) return q_quad_dot<true>(x, dp, qs, v, sub);
    const float acc = q_quad_dot(x, dp, qs, v, sub);
    if (metric != 1) return nnd_gram_to_dist<NND_CODES_0_5>(metric, acc, qn2, xn2[v]);  // prepared rows and query (codes 2..5)
    // alternative_cosine (distances.py:600-630) on the raw rows
    const float nx = xn2[v];
    if (qn2 == 0.0f && nx == 0.0f) return 0.0f;
    if (qn2 == 0.0f || nx == 0.0f || acc <= 0.0f) return NND_FLT_MAX;
    const float r = sqrtf(qn2 * nx) / acc;
    return r > 1.0f ? log2f(r) : 0.0f;
}

// quad-cooperative proxy distance between the float query (LDS, |q|^2 = qn2) and the uint8 code row `v`, each code looked
// up in the codebook `lut` (LDS): quantized_uint8_sq_euclidean / _alternative_cosine / _alternative_dot (distances.py:1869,
// 1905, 1948).  A lane takes 16 codes per 16-byte load; the query's padding columns are 0 (no term under cosine / dot), the
// euclidean tail chunk of a row whose d is no multiple of 16 masks them.
__device__ __forceinline__ float q_quad_proxy(const uint8_t *__restrict__ codes, const float *__restrict__ cn2, int dcs, int d,
                                              int metric, const float *lut, const float *qs, float qn2, int64_t v, int sub) {
    const uint4 *row = (const uint4 *)(codes + v * dcs);
    float acc = 0.0f;
    auto chunk = [&](int c, int lim) {  // codes 16 c .. 16 c + 15, the first `lim` of them live
        const uint4 w = row[c];
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        const float4 *q4 = (const float4 *)(qs + 16 * c);
#pragma unroll
        for (int h = 0; h < 4; h++) {
            const float4 q = q4[h];
            const float qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const float y = lut[(ws[h] >> (8 * b)) & 0xFFu];
                if (metric == 0) {
                    const float df = qv[b] - y;
                    if (4 * h + b < lim) acc += df * df;
                } else {
                    acc += qv[b] * y;
                }
            }
        }
    };
    const int full = d >> 4;
    for (int c = sub; c < full; c += 4) chunk(c, 16);
    if ((d & 15) && sub == (full & 3)) chunk(full, d & 15);
    acc = q_quad_sum(acc);
    if (metric == 0) return acc;
    const float ny = cn2[v];
    if (metric == 2) return acc > 0.0f ? -log2f(acc / sqrtf(ny)) : NND_FLT_MAX;  // distances.py:1948-1966
    if (qn2 == 0.0f && ny == 0.0f) return 0.0f;                                  // distances.py:1905-1930
    if (qn2 == 0.0f || ny == 0.0f || acc <= 0.0f) return NND_FLT_MAX;
    return -log2f((acc / sqrtf(qn2 * ny) + 1.0f) / 2.0f);
}

// the rerank's exact distance (the reference's _distance_func on the raw query and the float row): q_quad_dist, except
// that dot is alternative_dot on the un-normalised query (distances.py:680-701), so it is not clamped at 0
__device__ __forceinline__ float q_rerank_dist(const float *__restrict__ x, const float *__restrict__ xn2, int dp, int metric,
                                               const float *qs, float qn2, int64_t v, int sub) {
    if (metric != 2) return q_quad_dist(x, xn2, dp, metric, qs, qn2, v, sub);
    const float acc = q_quad_dot(x, dp, qs, v, sub);
    return acc > 0.0f ? -log2f(acc) : NND_FLT_MAX;
}

// KU: result entries per lane -- entry u of lane j is position 64 u + j of the list (k <= 64 KU: 1, 2 or 4)
// Q8: quantization="uint8" -- the walk on the code rows (k = search_k), the rerank to k_out in the epilogue; the codebook
// (256 floats) sits in front of the waves' LDS.  The float instances (Q8 = false) never touch the codes, the codebook and cn2.
// RR: the rerank epilogue (k = search_k, the k_out best by the true distance leave).  Three forms: the float walk without it,
// the uint8 walk with it, and the float walk with it (Q8 = false, RR = true: metric code 6 and nothing else -- the walk on the
// float rows by the proxy inner product, the rerank by -<q,x>; the query stays as given, a zero query is searched).
// BM: the boolean family (codes 8..16, the instances of k_query_bool): the tree is descended with the query as given, then the
// query becomes its indicator row and the walk's distances are metric.h nnd_bool_dist on exact counts.
// FL: filtered (the instances of k_query_filtered / k_query_bool_filtered): a vertex enters the walk's result list only if its
// bit in `allow` (a bitset over the searcher's numbering) is set.  It is still visited, pushed to the frontier and expanded, so
// the bound, the stop rule and the hand-over to the big tier are those of the unfiltered walk relative to the allowed rows; the
// rerank's candidates are the walk's results and so all allowed.  The other instances never read `allow`.
// TG: tagged (the instances of k_query_tagged / k_query_bool_tagged): the same rule with a predicate per query -- the vertex's tag
// word (`tags`, the searcher's numbering) must meet the query's mask word (`qmasks`, one per query of the call, read once into
// scalar registers: one wave serves one query).  A query whose mask is 0 has no allowed row and does not walk.
// The body is shared by the kernels k_query (BM = false) and k_query_bool below.
template <bool BIG, int KU, bool Q8, bool RR, bool BM, bool FL = false, bool TG = false>
__device__ __forceinline__ void q_body(const float *__restrict__ x, const float *__restrict__ xn2, int dp, int d, int metric,
                                               int64_t n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                               const float *__restrict__ hyper, const float *__restrict__ offsets,
                                               const int32_t *__restrict__ children, const int32_t *__restrict__ tree_idx,
                                               int64_t n_nodes, const float *__restrict__ queries, int64_t nq, int k, float epsilon,
                                               float min_distance, int n_neighbors, uint32_t seed, int32_t *__restrict__ out_idx,
                                               float *__restrict__ out_dist, uint8_t *__restrict__ overflow /* (nq) LDS tier: set when the query needs the big tier */,
                                               const int32_t *__restrict__ qlist /* BIG: the queries of this batch */,
                                               int n_list, unsigned char *__restrict__ scratch, size_t scratch_stride,
                                               const uint8_t *__restrict__ codes, int dcs, const float *__restrict__ lut,
                                               const float *__restrict__ cn2, int k_out,
                                               const uint32_t *__restrict__ allow = nullptr,
                                               const uint64_t *__restrict__ tags = nullptr, const uint64_t *__restrict__ qmasks = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qsm[];
    const int lane = nnd_lane(), w = threadIdx.x >> 6;
    if constexpr (Q8) {  // the codebook, once per workgroup (256 threads: one entry each)
        ((float *)qsm)[threadIdx.x] = lut[threadIdx.x];
        __syncthreads();
    }
    const int64_t slot = (int64_t)blockIdx.x * 4 + w;
    if (BIG ? slot >= n_list : slot >= nq) return;  // whole wave; no workgroup barrier below
    const int64_t qi = BIG ? (int64_t)qlist[slot] : slot;
    constexpr int FCAP = BIG ? Q_BIG_FRONTIER : Q_FRONTIER;
    const int qp = Q8 ? dcs : dp;  // query floats in LDS (Q8: as many as a code row has columns)
    const size_t per_wave = BIG ? (size_t)qp * 4 + Q_CHUNK * 8 : (size_t)qp * 4 + Q_FRONTIER * 8 + Q_VISITED * 4 + Q_CHUNK * 8;
    unsigned char *mine = qsm + (Q8 ? 1024 : 0) + (size_t)w * ((per_wave + 15) & ~(size_t)15);
    float *qs = (float *)mine;                       // qp
    float *fd;                                       // FCAP distances
    int32_t *fv;                                     // FCAP vertices
    uint32_t *vis;                                   // LDS tier: Q_VISITED hash slots; big tier: (n + 31) / 32 bit words
    int32_t *cl;                                     // Q_CHUNK candidate ids
    if (BIG) {
        unsigned char *gs = scratch + (size_t)slot * scratch_stride;
        fd = (float *)gs;
        fv = (int32_t *)(fd + FCAP);
        vis = (uint32_t *)(fv + FCAP);
        cl = (int32_t *)(qs + qp);
    } else {
        fd = qs + qp;
        fv = (int32_t *)(fd + FCAP);
        vis = (uint32_t *)(fv + FCAP);
        cl = (int32_t *)(vis + Q_VISITED);
    }
    float *cd = (float *)(cl + Q_CHUNK);             // Q_CHUNK candidate distances
    const int sub = lane & 3, grp = lane >> 2;
    const int64_t vis_words = BIG ? (n + 31) / 32 : Q_VISITED;
    bool spilled = false;  // LDS tier: a structure overflowed -- the query is handed to the big tier (wave-uniform)

    // ---- the query: cosine queries are normalised (pynndescent_.py:1808-1815); a zero cosine query returns nothing ----
    float part = 0.0f;
    for (int j = lane; j < qp; j += 64) {
        const float v = j < d ? queries[qi * d + j] : 0.0f;
        qs[j] = v;
        part += v * v;
    }
    float qn2 = nnd_wave_sum_f32(part);
    for (int64_t s = lane; s < vis_words; s += 64) vis[s] = BIG ? 0u : Q_EMPTY;
    bool dead = false;
    uint64_t qmask = 0;  // TG: this query's mask word, wave-uniform
    if constexpr (TG) {
        const uint64_t m = qmasks[qi];
        qmask = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(m >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m);
        dead = qmask == 0ull;
    }
    if (metric == 1 || metric == 2) {  // cosine / dot (the reference's normalize_query, pynndescent_.py:1764-1768)
        const float nrm = sqrtf(qn2);
        if (nrm > 0.0f) {
            nnd_wave_lds_sync();
            for (int j = lane; j < dp; j += 64) qs[j] = qs[j] / nrm;
            nnd_wave_lds_sync();
            float p2 = 0.0f;
            for (int j = lane; j < dp; j += 64) p2 += qs[j] * qs[j];
            qn2 = nnd_wave_sum_f32(p2);
        } else {
            dead = true;
        }
    }
    nnd_wave_lds_sync();

    float rd[KU];    // result list, ascending: entry u of lane j holds the (64 u + j)-th best
    int32_t rv[KU];
#pragma unroll
    for (int u = 0; u < KU; u++) {
        rd[u] = INFINITY;
        rv[u] = -1;
    }
    int fn = 0;            // frontier size (wave-uniform)
    float bound = INFINITY;
    auto worst = [&]() -> float {
        float w = rd[0];
#pragma unroll
        for (int u = 1; u < KU; u++) w = ((k - 1) >> 6) == u ? rd[u] : w;  // (wave-uniform)
        return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), (k - 1) & 63));
    };
    auto update_bound = [&]() {
        const float wd = worst();
        // inf while the list is not full (not through the formula: with epsilon = 0 it gives 0 * inf = NaN there, and a NaN
        // bound ends the search at the seeds)
        bound = wd < INFINITY ? wd + epsilon * (wd - min_distance) : INFINITY;
    };
    // simple_heap_push (utils.py:352-406) on the sorted list: enters iff it beats the worst entry
    auto result_push = [&](float dc, int32_t vc) {
        if (!(dc < worst())) return;
        int pos = 0;  // entries that stay in front of the new one
        float cd[KU];  // what falls from the end of every 64-entry segment when the entries behind `pos` move up by one
        int32_t cv[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            pos += __popcll(__ballot(64 * u + lane < k && rd[u] <= dc));
            cd[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(rd[u]), 63));
            cv[u] = __builtin_amdgcn_readlane(rv[u], 63);
        }
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int p = pos - 64 * u;  // where the new entry lands, seen from this segment (wave-uniform)
            if (p >= 64) continue;       // behind this segment: nothing moves here
            const float dn = __shfl_up(rd[u], 1, 64);
            const int32_t vn = __shfl_up(rv[u], 1, 64);
            if (p < 0) {  // in an earlier segment: the whole segment moves up, its first lane takes what fell from the one before
                if (64 * u + lane < k) {
                    rd[u] = lane == 0 ? cd[u > 0 ? u - 1 : 0] : dn;
                    rv[u] = lane == 0 ? cv[u > 0 ? u - 1 : 0] : vn;
                }
            } else {
                if (lane > p && 64 * u + lane < k) { rd[u] = dn; rv[u] = vn; }
                if (lane == p) { rd[u] = dc; rv[u] = vc; }
            }
        }
    };
    // FL: may `vc` (wave-uniform) enter the result list -- one word of the allow bitset; TG: its tag word against the query's mask
    auto allowed = [&](int32_t vc) -> bool {
        if constexpr (TG) return (tags[(uint32_t)__builtin_amdgcn_readfirstlane(vc)] & qmask) != 0ull;
        if constexpr (!FL) return true;
        const uint32_t u = (uint32_t)__builtin_amdgcn_readfirstlane(vc);
        return ((allow[u >> 5] >> (u & 31u)) & 1u) != 0u;
    };
    auto frontier_push = [&](float dc, int32_t vc) {
        if (fn == FCAP) {  // drop what can never be expanded any more (the bound only shrinks)
            int kept = 0;
            for (int s0 = 0; s0 < FCAP; s0 += 64) {
                const float e = fd[s0 + lane];
                const int32_t ev = fv[s0 + lane];
                const bool keep = e < bound;
                const unsigned long long m = __ballot(keep);
                nnd_wave_lds_sync();
                if (keep) {
                    fd[kept + nnd_prefix_popc(m)] = e;
                    fv[kept + nnd_prefix_popc(m)] = ev;
                }
                kept += __popcll(m);
                nnd_wave_lds_sync();
            }
            fn = kept;
            if (fn == FCAP) {  // still full: the reference's heap would have grown -- LDS tier: hand the query over
                if (!BIG) spilled = true;  // (big tier, 65536 live entries: the candidate stays in the result list only)
                return;
            }
        }
        if (lane == 0) {
            fd[fn] = dc;
            fv[fn] = vc;
        }
        fn++;
    };
    // check_and_mark_visited (utils.py:335-349): true if `u` had not been seen.  Big tier: the reference's bitset over
    // all n points.  LDS tier: a hash set; once it holds Q_VISITED_MAX vertices the query is handed to the big tier
    // (the callers test nvis after every batch).
    int nvis = 0;  // wave-uniform (updated with ballots by the callers)
    auto mark_fresh = [&](uint32_t u) -> bool {
        if (BIG) {
            const uint32_t bit = 1u << (u & 31u);
            return (atomicOr(&vis[u >> 5], bit) & bit) == 0u;
        }
        if (nvis >= Q_VISITED_MAX) return false;
        uint32_t h = nnd_mix32(u) & (Q_VISITED - 1);
        for (int probe = 0; probe < Q_VISITED; probe++) {
            const uint32_t old = atomicCAS(&vis[h], Q_EMPTY, u);
            if (old == Q_EMPTY) return true;
            if (old == u) return false;
            h = (h + 1) & (Q_VISITED - 1);
        }
        return false;
    };
    // distances of cl[0..nc) -> cd, a quad per candidate
    auto chunk_dists = [&](int nc) {
        for (int c0 = 0; c0 < nc; c0 += 16) {
            const int c = c0 + grp;
            const int64_t v = cl[c < nc ? c : 0];
            float dv;
            if constexpr (Q8) dv = q_quad_proxy(codes, cn2, dcs, d, metric, (const float *)qsm, qs, qn2, v, sub);
            else if constexpr (RR) dv = nnd_gram_to_dist<NND_CODE_6>(metric, q_quad_dot(x, dp, qs, v, sub), qn2, xn2[v]);
            else if constexpr (BM) dv = nnd_gram_to_dist<NND_CODES_BOOL>(nnd_kernel_metric(metric, d), q_quad_dot(x, dp, qs, v, sub), qn2, xn2[v]);
            else dv = q_quad_dist(x, xn2, dp, metric, qs, qn2, v, sub);
            if (sub == 0 && c < nc) cd[c] = dv;
        }
        nnd_wave_lds_sync();
    };
    auto in_result = [&](int32_t vc) -> bool {
        bool hit = false;
#pragma unroll
        for (int u = 0; u < KU; u++) hit = hit || (64 * u + lane < k && rv[u] == vc);
        return __ballot(hit) != 0ull;
    };

    if (!dead) {
        // ---- init from the tree (rp_trees.py:2732-2741): descend to a leaf ----
        int ls = 0, le = 0;
        if (n_nodes > 0) {
            int node = 0;
            int depth = 0;
            while (children[2 * node] > 0) {
                float m = 0.0f;
                const float *h = hyper + (int64_t)node * dp;
                for (int j = lane; j < dp; j += 64) m += h[j] * qs[j];
                m = nnd_wave_sum_f32(m) + offsets[node];
                int side;
                if (fabsf(m) < 1e-8f) side = (int)(nnd_hash3(seed, (uint32_t)qi, (uint32_t)depth) & 1u);  // rp_trees.py:2668-2673
                else side = m > 0.0f ? 0 : 1;
                node = children[2 * node + side];
                depth++;
            }
            ls = -children[2 * node];
            le = -children[2 * node + 1];
        }
        if constexpr (BM) {  // the tree splits the rows as given, the distances take the indicator rows: qn2 = nnz(q)
            float p2 = 0.0f;
            for (int j = lane; j < d; j += 64) {
                const float v = qs[j] != 0.0f ? 1.0f : 0.0f;
                qs[j] = v;
                p2 += v;
            }
            qn2 = nnd_wave_sum_f32(p2);
            nnd_wave_lds_sync();
        }
        if (metric == 4 || metric == 5) {  // correlation / hellinger: the tree splits the raw rows (angular), the distances the prepared ones
            const double mu = metric == 4 ? nnd_row_mean_f64<64>(qs, d, lane) : 0.0;
            nnd_wave_lds_sync();
            float p2 = 0.0f;
            for (int j = lane; j < d; j += 64) {
                const float v = nnd_unit_transform(metric == 4 ? 4 : 5, qs[j], mu);  // (this block: the codes 4 / 5 only)
                qs[j] = v;
                p2 += v * v;
            }
            p2 = nnd_wave_sum_f32(p2);
            const float inv = p2 > 0.0f ? 1.0f / sqrtf(p2) : 0.0f;
            nnd_wave_lds_sync();
            for (int j = lane; j < d; j += 64) qs[j] *= inv;
            nnd_wave_lds_sync();
            qn2 = p2 > 0.0f ? 1.0f : 0.0f;
        }
        const int n_initial = le - ls;
        for (int c0 = 0; c0 < n_initial; c0 += Q_CHUNK) {
            const int nc = n_initial - c0 < Q_CHUNK ? n_initial - c0 : Q_CHUNK;
            bool fr = false;
            if (lane < nc) {
                const int32_t u = tree_idx[ls + c0 + lane];
                cl[lane] = u;
                fr = mark_fresh((uint32_t)u);
            }
            nvis += __popcll(__ballot(fr));
            if (!BIG && nvis >= Q_VISITED_MAX) spilled = true;
            nnd_wave_lds_sync();
            chunk_dists(nc);
            for (int j = 0; j < nc; j++) {  // pynndescent_.py:1826-1832
                if (allowed(cl[j])) result_push(cd[j], cl[j]);
                frontier_push(cd[j], cl[j]);
            }
            nnd_wave_lds_sync();
            if (spilled) break;
        }
        // ---- random start vertices if the leaf was small (pynndescent_.py:1834-1848) ----
        const int n_random = (k < n_neighbors ? k : n_neighbors) - n_initial;
        for (int j = 0; j < n_random && !spilled; j++) {
            const uint32_t u = nnd_hash3(seed ^ 0x3C6EF372u, (uint32_t)qi, (uint32_t)j) % (uint32_t)n;
            bool fresh = false;
            if (lane == 0) fresh = mark_fresh(u);
            fresh = __shfl((int)fresh, 0, 64);
            if (!fresh) continue;
            nvis++;
            if (lane == 0) cl[0] = (int32_t)u;
            nnd_wave_lds_sync();
            chunk_dists(1);
            if (allowed(cl[0])) result_push(cd[0], cl[0]);
            frontier_push(cd[0], cl[0]);
            nnd_wave_lds_sync();
        }
        update_bound();

        // ---- best-first search (pynndescent_.py:1850-1881) ----
        while (fn > 0 && !spilled) {
            nnd_wave_lds_sync();
            // pop the nearest frontier vertex
            float bd = INFINITY;
            int bp = -1;
            for (int s = lane; s < fn; s += 64) {
                const float e = fd[s];
                if (e < bd) { bd = e; bp = s; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float od = __shfl_xor(bd, o, 64);
                const int op = __shfl_xor(bp, o, 64);
                if (od < bd || (od == bd && op >= 0 && (bp < 0 || op < bp))) { bd = od; bp = op; }
            }
            if (bp < 0 || !(bd < bound)) break;  // pynndescent_.py:1857
            const int32_t vertex = fv[bp];
            nnd_wave_lds_sync();
            if (lane == 0) {
                fd[bp] = fd[fn - 1];
                fv[bp] = fv[fn - 1];
            }
            fn--;
            const int a = indptr[vertex], b = indptr[vertex + 1];
            for (int e0 = a; e0 < b; e0 += Q_CHUNK) {
                const int e = e0 + lane;
                bool fresh = false;
                int32_t u = -1;
                if (e < b) {
                    u = indices[e];
                    fresh = mark_fresh((uint32_t)u);
                }
                const unsigned long long m = __ballot(fresh);
                const int nc = __popcll(m);
                nvis += nc;
                if (!BIG && nvis >= Q_VISITED_MAX) spilled = true;  // this batch is still exact (the set has room for it)
                if (nc == 0) continue;
                nnd_wave_lds_sync();
                if (fresh) cl[nnd_prefix_popc(m)] = u;
                nnd_wave_lds_sync();
                chunk_dists(nc);
                for (int j = 0; j < nc; j++) {
                    const float dc = cd[j];
                    const int32_t vc = cl[j];
                    if (dc < bound && !in_result(vc)) {  // pynndescent_.py:1866-1874
                        if (allowed(vc)) result_push(dc, vc);
                        frontier_push(dc, vc);
                        update_bound();
                    }
                }
                nnd_wave_lds_sync();
                if (spilled) break;
            }
        }
    }
    if constexpr (RR) {  // rerank (pynndescent_.py:776-789, 2364): the walk's search_k results -> the k_out best by exact distance
        const int ks = k;
        k = k_out;  // from here on the result list (worst(), result_push) and the output hold k_out entries
        if (!spilled && !dead) {
            nnd_wave_lds_sync();
#pragma unroll
            for (int u = 0; u < KU; u++)
                if (64 * u + lane < ks) fv[64 * u + lane] = rv[u];  // candidates in ascending proxy order (the frontier is spent)
            if constexpr (Q8) {  // the RAW query: the rerank takes query_data, not the normalised query
                float p = 0.0f;
                for (int j = lane; j < dp; j += 64) {
                    const float v = j < d ? queries[qi * d + j] : 0.0f;
                    qs[j] = v;
                    p += v * v;
                }
                qn2 = nnd_wave_sum_f32(p);
            }  // (the float walk of code 6 ran on the raw query: it is in place)
            nnd_wave_lds_sync();
            for (int c0 = 0; c0 < ks; c0 += 16) {
                const int c = c0 + grp;
                const int32_t vc = fv[c < ks ? c : 0];
                float dv;
                if constexpr (Q8) dv = q_rerank_dist(x, xn2, dp, metric, qs, qn2, vc < 0 ? 0 : vc, sub);
                else dv = -q_quad_dot(x, dp, qs, vc < 0 ? 0 : vc, sub);
                if (sub == 0 && c < ks) fd[c] = dv;
            }
            nnd_wave_lds_sync();
#pragma unroll
            for (int u = 0; u < KU; u++) {
                rd[u] = INFINITY;
                rv[u] = -1;
            }
            for (int j = 0; j < ks; j++) {  // simple_heap_push in the walk's order; idx < 0 is skipped (pynndescent_.py:783-784)
                const int32_t vc = fv[j];
                if (vc >= 0) result_push(fd[j], vc);
            }
        }
    }
    if (!BIG && lane == 0) overflow[qi] = spilled ? 1 : 0;  // the host re-runs flagged queries on the big tier
#pragma unroll
    for (int u = 0; u < KU; u++)
        if (64 * u + lane < k) {  // ascending, like deheap_sort; unfilled slots (-1, inf)
            out_idx[qi * k + 64 * u + lane] = rv[u];
            out_dist[qi * k + 64 * u + lane] = rd[u];
        }
}
template <bool BIG, int KU, bool Q8 = false, bool RR = Q8>
__global__ __launch_bounds__(256) void k_query(const float *__restrict__ x, const float *__restrict__ xn2, int dp, int d, int metric,
                                               int64_t n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                               const float *__restrict__ hyper, const float *__restrict__ offsets,
                                               const int32_t *__restrict__ children, const int32_t *__restrict__ tree_idx,
                                               int64_t n_nodes, const float *__restrict__ queries, int64_t nq, int k, float epsilon,
                                               float min_distance, int n_neighbors, uint32_t seed, int32_t *__restrict__ out_idx,
                                               float *__restrict__ out_dist, uint8_t *__restrict__ overflow /* (nq) LDS tier: set when the query needs the big tier */,
                                               const int32_t *__restrict__ qlist /* BIG: the queries of this batch */,
                                               int n_list, unsigned char *__restrict__ scratch, size_t scratch_stride,
                                               const uint8_t *__restrict__ codes, int dcs, const float *__restrict__ lut,
                                               const float *__restrict__ cn2, int k_out) {
    q_body<BIG, KU, Q8, RR, false>(x, xn2, dp, d, metric, n, indptr, indices, hyper, offsets, children, tree_idx, n_nodes, queries, nq, k, epsilon, min_distance,
                               n_neighbors, seed, out_idx, out_dist, overflow, qlist, n_list, scratch, scratch_stride, codes, dcs, lut, cn2, k_out);
}
template <bool BIG, int KU>
__global__ __launch_bounds__(256) void k_query_bool(const float *__restrict__ x, const float *__restrict__ xn2, int dp, int d, int metric,
                                               int64_t n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                               const float *__restrict__ hyper, const float *__restrict__ offsets,
                                               const int32_t *__restrict__ children, const int32_t *__restrict__ tree_idx,
                                               int64_t n_nodes, const float *__restrict__ queries, int64_t nq, int k, float epsilon,
                                               float min_distance, int n_neighbors, uint32_t seed, int32_t *__restrict__ out_idx,
                                               float *__restrict__ out_dist, uint8_t *__restrict__ overflow /* (nq) LDS tier: set when the query needs the big tier */,
                                               const int32_t *__restrict__ qlist /* BIG: the queries of this batch */,
                                               int n_list, unsigned char *__restrict__ scratch, size_t scratch_stride,
                                               const uint8_t *__restrict__ codes, int dcs, const float *__restrict__ lut,
                                               const float *__restrict__ cn2, int k_out) {
    q_body<BIG, KU, false, false, true>(x, xn2, dp, d, metric, n, indptr, indices, hyper, offsets, children, tree_idx, n_nodes, queries, nq, k, epsilon, min_distance,
                               n_neighbors, seed, out_idx, out_dist, overflow, qlist, n_list, scratch, scratch_stride, codes, dcs, lut, cn2, k_out);
}
// the filtered siblings (FL): the same arguments and `allow`
template <bool BIG, int KU, bool Q8 = false, bool RR = Q8>
__global__ __launch_bounds__(256) void k_query_filtered(const float *__restrict__ x, const float *__restrict__ xn2, int dp, int d, int metric,
                                               int64_t n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                               const float *__restrict__ hyper, const float *__restrict__ offsets,
                                               const int32_t *__restrict__ children, const int32_t *__restrict__ tree_idx,
                                               int64_t n_nodes, const float *__restrict__ queries, int64_t nq, int k, float epsilon,
                                               float min_distance, int n_neighbors, uint32_t seed, int32_t *__restrict__ out_idx,
                                               float *__restrict__ out_dist, uint8_t *__restrict__ overflow /* (nq) LDS tier: set when the query needs the big tier */,
                                               const int32_t *__restrict__ qlist /* BIG: the queries of this batch */,
                                               int n_list, unsigned char *__restrict__ scratch, size_t scratch_stride,
                                               const uint8_t *__restrict__ codes, int dcs, const float *__restrict__ lut,
                                               const float *__restrict__ cn2, int k_out,
                                               const uint32_t *__restrict__ allow /* (n + 31) / 32 words */) {
    q_body<BIG, KU, Q8, RR, false, true>(x, xn2, dp, d, metric, n, indptr, indices, hyper, offsets, children, tree_idx, n_nodes, queries, nq, k, epsilon, min_distance,
                               n_neighbors, seed, out_idx, out_dist, overflow, qlist, n_list, scratch, scratch_stride, codes, dcs, lut, cn2, k_out, allow);
}
template <bool BIG, int KU>
__global__ __launch_bounds__(256) void k_query_bool_filtered(const float *__restrict__ x, const float *__restrict__ xn2, int dp, int d, int metric,
                                               int64_t n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                               const float *__restrict__ hyper, const float *__restrict__ offsets,
                                               const int32_t *__restrict__ children, const int32_t *__restrict__ tree_idx,
                                               int64_t n_nodes, const float *__restrict__ queries, int64_t nq, int k, float epsilon,
                                               float min_distance, int n_neighbors, uint32_t seed, int32_t *__restrict__ out_idx,
                                               float *__restrict__ out_dist, uint8_t *__restrict__ overflow /* (nq) LDS tier: set when the query needs the big tier */,
                                               const int32_t *__restrict__ qlist /* BIG: the queries of this batch */,
                                               int n_list, unsigned char *__restrict__ scratch, size_t scratch_stride,
                                               const uint8_t *__restrict__ codes, int dcs, const float *__restrict__ lut,
                                               const float *__restrict__ cn2, int k_out,
                                               const uint32_t *__restrict__ allow /* (n + 31) / 32 words */) {
    q_body<BIG, KU, false, false, true, true>(x, xn2, dp, d, metric, n, indptr, indices, hyper, offsets, children, tree_idx, n_nodes, queries, nq, k, epsilon, min_distance,
                               n_neighbors, seed, out_idx, out_dist, overflow, qlist, n_list, scratch, scratch_stride, codes, dcs, lut, cn2, k_out, allow);
}

// the tagged siblings (TG): the same arguments, the tag words and the queries' mask words
template <bool BIG, int KU, bool Q8 = false, bool RR = Q8>
__global__ __launch_bounds__(256) void k_query_tagged(const float *__restrict__ x, const float *__restrict__ xn2, int dp, int d, int metric,
                                               int64_t n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                               const float *__restrict__ hyper, const float *__restrict__ offsets,
                                               const int32_t *__restrict__ children, const int32_t *__restrict__ tree_idx,
                                               int64_t n_nodes, const float *__restrict__ queries, int64_t nq, int k, float epsilon,
                                               float min_distance, int n_neighbors, uint32_t seed, int32_t *__restrict__ out_idx,
                                               float *__restrict__ out_dist, uint8_t *__restrict__ overflow /* (nq) LDS tier: set when the query needs the big tier */,
                                               const int32_t *__restrict__ qlist /* BIG: the queries of this batch */,
                                               int n_list, unsigned char *__restrict__ scratch, size_t scratch_stride,
                                               const uint8_t *__restrict__ codes, int dcs, const float *__restrict__ lut,
                                               const float *__restrict__ cn2, int k_out,
                                               const uint64_t *__restrict__ tags /* (n) */, const uint64_t *__restrict__ qmasks /* (nq) */) {
    q_body<BIG, KU, Q8, RR, false, false, true>(x, xn2, dp, d, metric, n, indptr, indices, hyper, offsets, children, tree_idx, n_nodes, queries, nq, k, epsilon, min_distance,
                               n_neighbors, seed, out_idx, out_dist, overflow, qlist, n_list, scratch, scratch_stride, codes, dcs, lut, cn2, k_out, nullptr, tags, qmasks);
}
template <bool BIG, int KU>
__global__ __launch_bounds__(256) void k_query_bool_tagged(const float *__restrict__ x, const float *__restrict__ xn2, int dp, int d, int metric,
                                               int64_t n, const int32_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                               const float *__restrict__ hyper, const float *__restrict__ offsets,
                                               const int32_t *__restrict__ children, const int32_t *__restrict__ tree_idx,
                                               int64_t n_nodes, const float *__restrict__ queries, int64_t nq, int k, float epsilon,
                                               float min_distance, int n_neighbors, uint32_t seed, int32_t *__restrict__ out_idx,
                                               float *__restrict__ out_dist, uint8_t *__restrict__ overflow /* (nq) LDS tier: set when the query needs the big tier */,
                                               const int32_t *__restrict__ qlist /* BIG: the queries of this batch */,
                                               int n_list, unsigned char *__restrict__ scratch, size_t scratch_stride,
                                               const uint8_t *__restrict__ codes, int dcs, const float *__restrict__ lut,
                                               const float *__restrict__ cn2, int k_out,
                                               const uint64_t *__restrict__ tags /* (n) */, const uint64_t *__restrict__ qmasks /* (nq) */) {
    q_body<BIG, KU, false, false, true, false, true>(x, xn2, dp, d, metric, n, indptr, indices, hyper, offsets, children, tree_idx, n_nodes, queries, nq, k, epsilon, min_distance,
                               n_neighbors, seed, out_idx, out_dist, overflow, qlist, n_list, scratch, scratch_stride, codes, dcs, lut, cn2, k_out, nullptr, tags, qmasks);
}


// the searcher's copy of the rows for the codes 2..5: the build's row transform (metric.h), one wave per row, in place --
// dot: L2-normalised; correlation: minus the row mean (float64), then normalised; hellinger: sqrt, then normalised
__global__ void k_searcher_prep_rows(float *__restrict__ x, int64_t n, int d, int dp, int metric) {
    const int lane = nnd_lane();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    float *row = x + r * dp;
    const double mu = metric == 4 ? nnd_row_mean_f64<64>(row, d, lane) : 0.0;
    float s = 0.0f;
    for (int j = lane; j < d; j += 64) {
        const float v = nnd_unit_transform(metric, row[j], mu);
        row[j] = v;
        s += v * v;
    }
    s = nnd_wave_sum_f32(s);
    const float inv = s > 0.0f ? 1.0f / sqrtf(s) : 0.0f;
    for (int j = lane; j < d; j += 64) row[j] *= inv;
}

// the boolean family: the searcher's rows become indicator rows in place (x != 0 -> 1, else 0; the padding stays 0), so that
// k_row_norm2 gives nnz(x) and every product of the walk is a count
__global__ void k_searcher_indicator_rows(float *__restrict__ x, int64_t n, int dp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n * dp) x[i] = x[i] != 0.0f ? 1.0f : 0.0f;
}
static void searcher_indicator_rows(nnd_searcher_s *s, hipStream_t st) {
    const int64_t total = s->n * s->dp;
    hipLaunchKernelGGL(k_searcher_indicator_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, s->x, s->n, s->dp);
}

// squared norms of the padded rows (alternative_cosine recomputes them per call, distances.py:617-620)
__global__ void k_row_norm2(const float *__restrict__ x, int64_t n, int dp, float *__restrict__ out) {
    const int lane = nnd_lane();
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    float s = 0.0f;
    for (int j = lane; j < dp; j += 64) {
        const float v = x[r * dp + j];
        s += v * v;
    }
    s = nnd_wave_sum_f32(s);
    if (lane == 0) out[r] = s;
}

// uint8 codes of the searcher's rows (pynndescent_.py:2207-2209: np.searchsorted(values, raw).astype(np.uint8)): one wave
// per row, one element per lane.  The search is a branchless searchsorted-left over the 256-entry table `tab` (the codebook,
// +inf past its n_values entries): a value above the last entry gets n_values, and 256 wraps to code 0 through the uint8
// cast, bit for bit as the reference.  Code rows have stride dcs, padding bytes 0.  cn2 (cosine / dot; may be null): the
// row's sum of lut[c]^2 with the walk's table.  x == nullptr: the codes are already in place, only cn2 is computed.
__global__ __launch_bounds__(256) void k_quantize_u8(const float *__restrict__ x, int64_t xstride, int64_t n, int d, int dcs,
                                                     const float *__restrict__ lut, const float *__restrict__ tab,
                                                     uint8_t *__restrict__ codes, float *__restrict__ cn2) {
    __shared__ float st[256], lt[256];
    st[threadIdx.x] = tab[threadIdx.x];
    lt[threadIdx.x] = lut[threadIdx.x];
    __syncthreads();
    const int lane = nnd_lane();
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {  // wave-uniform
        float s = 0.0f;
        for (int j = lane; j < dcs; j += 64) {
            uint32_t c = 0;
            if (x) {
                if (j < d) {
                    const float v = x[r * xstride + j];
                    int lo = 0;
#pragma unroll
                    for (int h = 128; h > 0; h >>= 1) lo += st[lo + h - 1] < v ? h : 0;
                    lo += st[lo] < v ? 1 : 0;  // 0 .. 256
                    c = (uint32_t)lo & 0xFFu;
                }
                codes[r * dcs + j] = (uint8_t)c;
            } else {
                c = codes[r * dcs + j];
            }
            if (j < d) s += lt[c] * lt[c];
        }
        if (cn2) {
            s = nnd_wave_sum_f32(s);
            if (lane == 0) cn2[r] = s;
        }
    }
}

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

#define S_HIP(expr)                                                                                 \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            s->set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);  \
            return 1;                                                                               \
        }                                                                                           \
    } while (0)
#define S_ALLOC(p, count)                                                                      \
    do {                                                                                       \
        if (!s->mem.alloc(p, count)) {                                                         \
            s->set_error("out of device memory: %s, %zu elements (%s:%d)", #p, (size_t)(count), __FILE__, __LINE__); \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

static int upload_padded(nnd_searcher_s *s, float **dst, const float *src, int64_t rows, int d, int dp) {
    S_ALLOC(dst, (size_t)(rows ? rows : 1) * dp);
    if (rows == 0) return 0;
    if (d == dp) {
        S_HIP(hipMemcpy(*dst, src, sizeof(float) * (size_t)rows * d, hipMemcpyHostToDevice));
    } else {
        S_HIP(hipMemset(*dst, 0, sizeof(float) * (size_t)rows * dp));
        S_HIP(hipMemcpy2D(*dst, sizeof(float) * dp, src, sizeof(float) * d, sizeof(float) * d, (size_t)rows, hipMemcpyHostToDevice));
    }
    return 0;
}

extern "C" const char *nnd_searcher_last_error(nnd_searcher_t s) { return s ? s->err : g_serr; }

extern "C" int32_t nnd_searcher_destroy(nnd_searcher_t s) {
    if (!s) return 0;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    s->mem.release_all();
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return 0;
}

static int searcher_fill(nnd_searcher_s *s, const float *data, const int32_t *indptr, const int32_t *indices, const float *hyperplanes,
                         const float *offsets, const int32_t *children, const int32_t *tree_indices) {
    S_HIP(hipSetDevice(s->device));
    S_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    if (upload_padded(s, &s->x, data, s->n, s->d, s->dp)) return 1;
    S_ALLOC(&s->xn2, (size_t)s->n);
    if (s->metric == NND_METRIC_ALT_DOT || s->metric == NND_METRIC_CORRELATION || s->metric == NND_METRIC_ALT_HELLINGER)
        hipLaunchKernelGGL(k_searcher_prep_rows, dim3((unsigned)((s->n + 3) / 4)), dim3(256), 0, s->stream, s->x, s->n, s->d, s->dp, s->metric);
    if (nnd_metric_bool(s->metric)) searcher_indicator_rows(s, s->stream);
    hipLaunchKernelGGL(k_row_norm2, dim3((unsigned)((s->n + 3) / 4)), dim3(256), 0, s->stream, s->x, s->n, s->dp, s->xn2);
    S_ALLOC(&s->indptr, (size_t)(s->n + 1));
    S_HIP(hipMemcpy(s->indptr, indptr, sizeof(int32_t) * (size_t)(s->n + 1), hipMemcpyHostToDevice));
    S_ALLOC(&s->indices, (size_t)s->nnz);
    S_HIP(hipMemcpy(s->indices, indices, sizeof(int32_t) * (size_t)s->nnz, hipMemcpyHostToDevice));
    if (s->n_nodes > 0) {
        if (upload_padded(s, &s->hyper, hyperplanes, s->n_nodes, s->d, s->dp)) return 1;
        S_ALLOC(&s->offsets, (size_t)s->n_nodes);
        S_HIP(hipMemcpy(s->offsets, offsets, sizeof(float) * (size_t)s->n_nodes, hipMemcpyHostToDevice));
        S_ALLOC(&s->children, 2 * (size_t)s->n_nodes);
        S_HIP(hipMemcpy(s->children, children, sizeof(int32_t) * 2 * (size_t)s->n_nodes, hipMemcpyHostToDevice));
        S_ALLOC(&s->tree_idx, (size_t)s->n);
        S_HIP(hipMemcpy(s->tree_idx, tree_indices, sizeof(int32_t) * (size_t)s->n, hipMemcpyHostToDevice));
    }
    S_HIP(hipStreamSynchronize(s->stream));
    return 0;
}

// the same state from device memory, on the caller's stream: rows gathered by `order` straight into the padded layout
// (devarray.hip), the CSR copied device to device; the tree tables come from the host as above
static int searcher_fill_device(nnd_searcher_s *s, const void *rows, int dtype, const int32_t *order, const int32_t *indptr, const int32_t *indices,
                                const float *hyperplanes, const float *offsets, const int32_t *children, const int32_t *tree_indices, hipStream_t st) {
    S_HIP(hipSetDevice(s->device));
    S_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    S_ALLOC(&s->x, (size_t)s->n * s->dp);
    S_ALLOC(&s->xn2, (size_t)s->n);
    S_ALLOC(&s->indptr, (size_t)(s->n + 1));
    S_ALLOC(&s->indices, (size_t)s->nnz);
    if (nnd_launch_gather_rows(st, rows, dtype, order, s->n, s->d, s->dp, s->x)) {
        (void)hipGetLastError();
        s->set_error("the rows' gather could not be launched (dtype %d)", dtype);
        return 1;
    }
    if (s->metric == NND_METRIC_ALT_DOT || s->metric == NND_METRIC_CORRELATION || s->metric == NND_METRIC_ALT_HELLINGER)
        hipLaunchKernelGGL(k_searcher_prep_rows, dim3((unsigned)((s->n + 3) / 4)), dim3(256), 0, st, s->x, s->n, s->d, s->dp, s->metric);
    if (nnd_metric_bool(s->metric)) searcher_indicator_rows(s, st);
    hipLaunchKernelGGL(k_row_norm2, dim3((unsigned)((s->n + 3) / 4)), dim3(256), 0, st, s->x, s->n, s->dp, s->xn2);
    S_HIP(hipGetLastError());
    S_HIP(hipMemcpyAsync(s->indptr, indptr, sizeof(int32_t) * (size_t)(s->n + 1), hipMemcpyDeviceToDevice, st));
    if (s->nnz > 0) S_HIP(hipMemcpyAsync(s->indices, indices, sizeof(int32_t) * (size_t)s->nnz, hipMemcpyDeviceToDevice, st));
    if (s->n_nodes > 0) {
        if (upload_padded(s, &s->hyper, hyperplanes, s->n_nodes, s->d, s->dp)) return 1;
        S_ALLOC(&s->offsets, (size_t)s->n_nodes);
        S_HIP(hipMemcpy(s->offsets, offsets, sizeof(float) * (size_t)s->n_nodes, hipMemcpyHostToDevice));
        S_ALLOC(&s->children, 2 * (size_t)s->n_nodes);
        S_HIP(hipMemcpy(s->children, children, sizeof(int32_t) * 2 * (size_t)s->n_nodes, hipMemcpyHostToDevice));
        S_ALLOC(&s->tree_idx, (size_t)s->n);
        S_HIP(hipMemcpy(s->tree_idx, tree_indices, sizeof(int32_t) * (size_t)s->n, hipMemcpyHostToDevice));
    }
    S_HIP(hipStreamSynchronize(st));  // the caller's buffers are free again, and the searcher's own stream may read what was written
    return 0;
}

// what the two create entries share: the argument and device checks, and the searcher with its scalars set (nullptr: g_serr says why)
static nnd_searcher_s *searcher_new(const char *who, bool args_ok, int32_t device, int64_t n, int32_t dim, int32_t metric, int64_t nnz,
                                    bool tree_ok, int64_t n_nodes, float min_distance, int32_t n_neighbors, const int64_t *rng_state) {
    auto fail = [&](const char *msg) -> nnd_searcher_s * {
        snprintf(g_serr, sizeof(g_serr), "%s: %s", who, msg);
        return nullptr;
    };
    if (!args_ok || n < 1 || dim < 1 || nnz < 0) return fail("bad arguments");
    if (metric < NND_METRIC_SQEUCLIDEAN || metric > NND_METRIC_YULE || metric == NND_METRIC_PROXY_INNER_PRODUCT + 1) return fail("unknown metric");
    if (nnd_metric_bool(metric) && dim >= (1 << 23)) return fail("the boolean metrics need dim < 2^23");
    if (n_nodes > 0 && !tree_ok) return fail("tree arrays missing");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail("no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail("device out of range");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("this build targets gfx950 (MI355X) only");
    nnd_searcher_s *s = new nnd_searcher_s();
    s->device = device;
    s->n = n;
    s->nnz = nnz;
    s->n_nodes = n_nodes;
    s->d = dim;
    s->dp = (dim + 3) & ~3;
    s->metric = metric;
    s->n_neighbors = n_neighbors;
    s->min_distance = min_distance;
    s->seed = rng_state ? nnd_mix32((uint32_t)rng_state[0] ^ nnd_mix32((uint32_t)rng_state[1] + 0x9E3779B9u) ^ nnd_mix32((uint32_t)rng_state[2] + 0x7F4A7C15u)) : 1u;
    return s;
}
static int searcher_filled(const char *who, nnd_searcher_s *s, int rc, nnd_searcher_t *out) {
    if (rc) {
        snprintf(g_serr, sizeof(g_serr), "%s: %s", who, s->err);
        nnd_searcher_destroy(s);
        return 1;
    }
    *out = s;
    return 0;
}

extern "C" int32_t nnd_searcher_create(nnd_searcher_t *out, int32_t device, int64_t n, int32_t dim, int32_t metric, const float *data,
                                       const int32_t *indptr, const int32_t *indices, int64_t nnz, const float *hyperplanes,
                                       const float *offsets, const int32_t *children, const int32_t *tree_indices, int64_t n_nodes,
                                       float min_distance, int32_t n_neighbors, const int64_t *rng_state) {
    nnd_searcher_s *s = searcher_new("nnd_searcher_create", out && data && indptr && indices, device, n, dim, metric, nnz,
                                     hyperplanes && offsets && children && tree_indices, n_nodes, min_distance, n_neighbors, rng_state);
    if (!s) return 1;
    return searcher_filled("nnd_searcher_create", s, searcher_fill(s, data, indptr, indices, hyperplanes, offsets, children, tree_indices), out);
}

extern "C" int32_t nnd_searcher_create_device(nnd_searcher_t *out, int32_t device, int64_t n, int32_t dim, int32_t metric, const void *rows_dev,
                                              int32_t dtype, const int32_t *order_dev, const int32_t *indptr_dev, const int32_t *indices_dev,
                                              int64_t nnz, const float *hyperplanes, const float *offsets, const int32_t *children,
                                              const int32_t *tree_indices, int64_t n_nodes, float min_distance, int32_t n_neighbors,
                                              const int64_t *rng_state, void *hip_stream) {
    const bool args_ok = out && rows_dev && indptr_dev && (indices_dev || nnz == 0) && dtype >= NND_DTYPE_FLOAT32 && dtype <= NND_DTYPE_FLOAT64;
    nnd_searcher_s *s = searcher_new("nnd_searcher_create_device", args_ok, device, n, dim, metric, nnz,
                                     hyperplanes && offsets && children && tree_indices, n_nodes, min_distance, n_neighbors, rng_state);
    if (!s) return 1;
    return searcher_filled("nnd_searcher_create_device", s,
                           searcher_fill_device(s, rows_dev, dtype, order_dev, indptr_dev, indices_dev, hyperplanes, offsets, children, tree_indices,
                                                (hipStream_t)hip_stream), out);
}

extern "C" int64_t nnd_searcher_last_spilled(nnd_searcher_t s) { return s ? s->last_spilled : -1; }
extern "C" int32_t nnd_searcher_set_tier(nnd_searcher_t s, int32_t tier) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_set_tier: null searcher"); return 1; }
    if (tier != 0 && tier != 1) { s->set_error("nnd_searcher_set_tier: tier must be 0 (automatic) or 1 (global-memory tier for every query)"); return 1; }
    s->force_big = tier == 1;
    return 0;
}

// the three forms of k_query (its Q8 / RR switches)
enum q_form { Q_FORM_FLOAT, Q_FORM_U8, Q_FORM_RERANK, Q_FORM_BOOL /* the float form of the boolean family: k_query_bool */ };
template <bool BIG>
static auto query_kernel(q_form form, int k) -> decltype(&k_query<BIG, 1>) {
    // (k > 64, round 5: the result list as two or four entries per lane; the reference takes any k, pynndescent_.py:2275-2379)
    switch (form) {
        case Q_FORM_U8: return k > 128 ? k_query<BIG, 4, true> : (k > 64 ? k_query<BIG, 2, true> : k_query<BIG, 1, true>);
        case Q_FORM_BOOL: return k > 128 ? k_query_bool<BIG, 4> : (k > 64 ? k_query_bool<BIG, 2> : k_query_bool<BIG, 1>);
        case Q_FORM_RERANK: return k > 128 ? k_query<BIG, 4, false, true> : (k > 64 ? k_query<BIG, 2, false, true> : k_query<BIG, 1, false, true>);
        default: return k > 128 ? k_query<BIG, 4> : (k > 64 ? k_query<BIG, 2> : k_query<BIG, 1>);
    }
}
template <bool BIG>
static auto query_kernel_filtered(q_form form, int k) -> decltype(&k_query_filtered<BIG, 1>) {
    switch (form) {
        case Q_FORM_U8: return k > 128 ? k_query_filtered<BIG, 4, true> : (k > 64 ? k_query_filtered<BIG, 2, true> : k_query_filtered<BIG, 1, true>);
        case Q_FORM_BOOL: return k > 128 ? k_query_bool_filtered<BIG, 4> : (k > 64 ? k_query_bool_filtered<BIG, 2> : k_query_bool_filtered<BIG, 1>);
        case Q_FORM_RERANK:
            return k > 128 ? k_query_filtered<BIG, 4, false, true> : (k > 64 ? k_query_filtered<BIG, 2, false, true> : k_query_filtered<BIG, 1, false, true>);
        default: return k > 128 ? k_query_filtered<BIG, 4> : (k > 64 ? k_query_filtered<BIG, 2> : k_query_filtered<BIG, 1>);
    }
}
template <bool BIG>
static auto query_kernel_tagged(q_form form, int k) -> decltype(&k_query_tagged<BIG, 1>) {
    switch (form) {
        case Q_FORM_U8: return k > 128 ? k_query_tagged<BIG, 4, true> : (k > 64 ? k_query_tagged<BIG, 2, true> : k_query_tagged<BIG, 1, true>);
        case Q_FORM_BOOL: return k > 128 ? k_query_bool_tagged<BIG, 4> : (k > 64 ? k_query_bool_tagged<BIG, 2> : k_query_bool_tagged<BIG, 1>);
        case Q_FORM_RERANK:
            return k > 128 ? k_query_tagged<BIG, 4, false, true> : (k > 64 ? k_query_tagged<BIG, 2, false, true> : k_query_tagged<BIG, 1, false, true>);
        default: return k > 128 ? k_query_tagged<BIG, 4> : (k > 64 ? k_query_tagged<BIG, 2> : k_query_tagged<BIG, 1>);
    }
}

// every query entry point: the walk keeps k results (the float rows) or k = search_k results and reranks them to k_out
// (Q_FORM_U8: the walk on the code rows; Q_FORM_RERANK: on the float rows); out_idx / out_dist are (nq, k_out)
static int searcher_run(nnd_searcher_s *s, const float *queries, int64_t nq, int32_t k, int32_t k_out, float epsilon, q_form form,
                        int32_t *out_idx, float *out_dist, bool on_device = false, hipStream_t user_stream = nullptr,
                        const uint64_t *qmasks = nullptr /* the tagged entries: (nq) mask words, where the queries are */) {
    const bool q8 = form == Q_FORM_U8;
    if (form == Q_FORM_FLOAT && nnd_metric_bool(s->metric)) form = Q_FORM_BOOL;
    auto kq_lds = query_kernel<false>(form, k);
    auto kq_big = query_kernel<true>(form, k);
    auto fq_lds = query_kernel_filtered<false>(form, k);  // launched instead while a filter is set (nnd_searcher_set_filter*)
    auto fq_big = query_kernel_filtered<true>(form, k);
    const uint32_t *allow = s->filter_on ? s->allow : nullptr;
    auto tq_lds = query_kernel_tagged<false>(form, k);  // launched instead by the tagged entries (nnd_searcher_query_tagged*)
    auto tq_big = query_kernel_tagged<true>(form, k);
    const uint64_t *dmasks = nullptr;
    if (nq <= 0) return 0;
    if (nq >= (int64_t)0x7FFFFFF0) { s->set_error("nnd_searcher_query: too many queries in one call"); return 1; }
    S_HIP(hipSetDevice(s->device));
    hipStream_t st = on_device ? user_stream : s->stream;
    nnd_scratch tmp;  // the buffers of this call
    int32_t *dlist = nullptr;
    unsigned char *scratch = nullptr;
    int rc = 0;
    const size_t qp = q8 ? (size_t)s->dcs : (size_t)s->dp;  // query floats per wave in LDS (k_query's qp)
    const size_t lut_bytes = q8 ? 1024 : 0;                  // the codebook in front of the waves
    const size_t per_wave = (qp * 4 + Q_FRONTIER * 8 + Q_VISITED * 4 + Q_CHUNK * 8 + 15) & ~(size_t)15;
    const size_t smem = 4 * per_wave + lut_bytes;
    const size_t per_wave_big = (qp * 4 + Q_CHUNK * 8 + 15) & ~(size_t)15;
    s->last_spilled = 0;
    std::vector<uint8_t> hov((size_t)nq, 1);
    do {
        float *dq = on_device ? const_cast<float *>(queries) : tmp.get<float>(s, (size_t)nq * s->d);
        float *dd = on_device ? out_dist : tmp.get<float>(s, (size_t)nq * k_out);
        int32_t *di = on_device ? out_idx : tmp.get<int32_t>(s, (size_t)nq * k_out);
        uint8_t *dov = tmp.get<uint8_t>(s, (size_t)nq);
        if (!dq || !dd || !di || !dov) { s->set_error("nnd_searcher_query: out of device memory"); rc = 1; break; }
        if (!on_device && hipMemcpyAsync(dq, queries, sizeof(float) * (size_t)nq * s->d, hipMemcpyHostToDevice, st) != hipSuccess) { s->set_error("H2D of the queries failed"); rc = 1; break; }
        if (qmasks) {
            dmasks = qmasks;
            if (!on_device) {
                uint64_t *dm = tmp.get<uint64_t>(s, (size_t)nq);
                if (!dm) { rc = 1; break; }
                if (hipMemcpyAsync(dm, qmasks, sizeof(uint64_t) * (size_t)nq, hipMemcpyHostToDevice, st) != hipSuccess) { s->set_error("H2D of the query masks failed"); rc = 1; break; }
                dmasks = dm;
            }
        }
        if (!s->force_big) {
            if (smem > 64 * 1024 && hipFuncSetAttribute(dmasks ? (const void *)tq_lds : allow ? (const void *)fq_lds : (const void *)kq_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) {
                s->set_error("nnd_searcher_query: rows of %d floats need %zu bytes of LDS per workgroup", s->d, smem); rc = 1; break;
            }
            if (dmasks)
                hipLaunchKernelGGL(tq_lds, dim3((unsigned)((nq + 3) / 4)), dim3(256), smem, st, s->x, s->xn2, s->dp, s->d, s->metric, s->n,
                                   s->indptr, s->indices, s->hyper, s->offsets, s->children, s->tree_idx, s->n_nodes, dq, nq, k, epsilon,
                                   s->min_distance, s->n_neighbors, s->seed, di, dd, dov, (const int32_t *)nullptr, 0, (unsigned char *)nullptr, (size_t)0,
                                   (const uint8_t *)s->codes, s->dcs, (const float *)s->lut, (const float *)s->cn2, k_out, (const uint64_t *)s->tags, dmasks);
            else if (allow)
                hipLaunchKernelGGL(fq_lds, dim3((unsigned)((nq + 3) / 4)), dim3(256), smem, st, s->x, s->xn2, s->dp, s->d, s->metric, s->n,
                                   s->indptr, s->indices, s->hyper, s->offsets, s->children, s->tree_idx, s->n_nodes, dq, nq, k, epsilon,
                                   s->min_distance, s->n_neighbors, s->seed, di, dd, dov, (const int32_t *)nullptr, 0, (unsigned char *)nullptr, (size_t)0,
                                   (const uint8_t *)s->codes, s->dcs, (const float *)s->lut, (const float *)s->cn2, k_out, allow);
            else
                hipLaunchKernelGGL(kq_lds, dim3((unsigned)((nq + 3) / 4)), dim3(256), smem, st, s->x, s->xn2, s->dp, s->d, s->metric, s->n,
                                   s->indptr, s->indices, s->hyper, s->offsets, s->children, s->tree_idx, s->n_nodes, dq, nq, k, epsilon,
                                   s->min_distance, s->n_neighbors, s->seed, di, dd, dov, (const int32_t *)nullptr, 0, (unsigned char *)nullptr, (size_t)0,
                                   (const uint8_t *)s->codes, s->dcs, (const float *)s->lut, (const float *)s->cn2, k_out);
            if (hipGetLastError() != hipSuccess) { s->set_error("k_query launch failed"); rc = 1; break; }
            if (hipMemcpyAsync(hov.data(), dov, (size_t)nq, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
                s->set_error("nnd_searcher_query: kernel or D2H failed: %s", hipGetErrorString(hipGetLastError())); rc = 1; break;
            }
        }
        // queries whose search outgrew the LDS structures (or all of them, nnd_searcher_set_tier(1)): global-memory tier
        std::vector<int32_t> again;
        for (int64_t i = 0; i < nq; i++)
            if (hov[(size_t)i]) again.push_back((int32_t)i);
        s->last_spilled = (int64_t)again.size();
        if (!again.empty()) {
            const size_t stride = ((size_t)Q_BIG_FRONTIER * 8 + (size_t)((s->n + 31) / 32) * 4 + 255) & ~(size_t)255;
            const size_t batch = again.size() < Q_BIG_BATCH ? again.size() : (size_t)Q_BIG_BATCH;
            scratch = tmp.get<unsigned char>(s, stride * batch);
            dlist = tmp.get<int32_t>(s, again.size());
            if (!scratch || !dlist) {
                s->set_error("nnd_searcher_query: out of device memory for the global-memory tier (%zu bytes)", stride * batch); rc = 1; break;
            }
            if (hipMemcpyAsync(dlist, again.data(), sizeof(int32_t) * again.size(), hipMemcpyHostToDevice, st) != hipSuccess) { s->set_error("H2D of the query list failed"); rc = 1; break; }
            for (size_t b0 = 0; b0 < again.size() && !rc; b0 += batch) {
                const int nb = (int)(again.size() - b0 < batch ? again.size() - b0 : batch);
                if (dmasks)
                    hipLaunchKernelGGL(tq_big, dim3((unsigned)((nb + 3) / 4)), dim3(256), 4 * per_wave_big + lut_bytes, st, s->x, s->xn2, s->dp, s->d,
                                       s->metric, s->n, s->indptr, s->indices, s->hyper, s->offsets, s->children, s->tree_idx, s->n_nodes, dq, nq, k, epsilon,
                                       s->min_distance, s->n_neighbors, s->seed, di, dd, (uint8_t *)nullptr, (const int32_t *)(dlist + b0), nb, scratch, stride,
                                       (const uint8_t *)s->codes, s->dcs, (const float *)s->lut, (const float *)s->cn2, k_out, (const uint64_t *)s->tags, dmasks);
                else if (allow)
                    hipLaunchKernelGGL(fq_big, dim3((unsigned)((nb + 3) / 4)), dim3(256), 4 * per_wave_big + lut_bytes, st, s->x, s->xn2, s->dp, s->d,
                                       s->metric, s->n, s->indptr, s->indices, s->hyper, s->offsets, s->children, s->tree_idx, s->n_nodes, dq, nq, k, epsilon,
                                       s->min_distance, s->n_neighbors, s->seed, di, dd, (uint8_t *)nullptr, (const int32_t *)(dlist + b0), nb, scratch, stride,
                                       (const uint8_t *)s->codes, s->dcs, (const float *)s->lut, (const float *)s->cn2, k_out, allow);
                else
                    hipLaunchKernelGGL(kq_big, dim3((unsigned)((nb + 3) / 4)), dim3(256), 4 * per_wave_big + lut_bytes, st, s->x, s->xn2, s->dp, s->d,
                                       s->metric, s->n, s->indptr, s->indices, s->hyper, s->offsets, s->children, s->tree_idx, s->n_nodes, dq, nq, k, epsilon,
                                       s->min_distance, s->n_neighbors, s->seed, di, dd, (uint8_t *)nullptr, (const int32_t *)(dlist + b0), nb, scratch, stride,
                                       (const uint8_t *)s->codes, s->dcs, (const float *)s->lut, (const float *)s->cn2, k_out);
                if (hipGetLastError() != hipSuccess) { s->set_error("k_query (global-memory tier) launch failed"); rc = 1; }
            }
            if (rc) break;
        }
        if ((!on_device && (hipMemcpyAsync(out_idx, di, sizeof(int32_t) * (size_t)nq * k_out, hipMemcpyDeviceToHost, st) != hipSuccess ||
                            hipMemcpyAsync(out_dist, dd, sizeof(float) * (size_t)nq * k_out, hipMemcpyDeviceToHost, st) != hipSuccess)) ||
            hipStreamSynchronize(st) != hipSuccess) { s->set_error("nnd_searcher_query: kernel or D2H failed: %s", hipGetErrorString(hipGetLastError())); rc = 1; break; }
    } while (0);
    return rc;
}

extern "C" int32_t nnd_searcher_query(nnd_searcher_t s, const float *queries, int64_t nq, int32_t k, float epsilon, int32_t *out_idx,
                                      float *out_dist) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_query: null searcher"); return 1; }
    if (k < 1 || k > 256) { s->set_error("nnd_searcher_query: k must be in 1..256 (got %d)", k); return 1; }
    if (s->metric == NND_METRIC_PROXY_INNER_PRODUCT) {
        s->set_error("nnd_searcher_query: metric %d is a proxy distance: its queries go through nnd_searcher_query_rerank", s->metric);
        return 1;
    }
    return searcher_run(s, queries, nq, k, k, epsilon, Q_FORM_FLOAT, out_idx, out_dist);
}

// ---- quantization="uint8" (pynndescent_.py:2191-2225, 2309-2364) ----
// the two 256-entry tables: the walk's codebook (entries past n_values = the last value; the reference reads past its
// array there, DESIGN.md "Quantized search") and the search table (+inf past n_values)
static int quant_tables(nnd_searcher_s *s, const char *who, const float *values, int32_t n_values) {
    if (s->metric != NND_METRIC_SQEUCLIDEAN && s->metric != NND_METRIC_ALT_COSINE && s->metric != NND_METRIC_ALT_DOT) {
        s->set_error("%s: uint8 quantization supports the sqeuclidean, alternative cosine and alternative dot metrics (metric %d)", who, s->metric);
        return 1;
    }
    if (!values || n_values < 1 || n_values > 256) { s->set_error("%s: the codebook must have 1..256 values (got %d)", who, n_values); return 1; }
    S_HIP(hipSetDevice(s->device));
    S_HIP(hipStreamSynchronize(s->stream));  // no kernel or copy of an earlier call still uses the tables
    float *tab = s->tab_host;
    for (int i = 0; i < 256; i++) {
        tab[i] = values[i < n_values ? i : n_values - 1];
        tab[256 + i] = i < n_values ? values[i] : INFINITY;
    }
    s->dcs = (s->d + 15) & ~15;
    if (!s->lut) S_ALLOC(&s->lut, 512);
    if (!s->codes) S_ALLOC(&s->codes, (size_t)s->n * s->dcs);
    if (!s->cn2 && s->metric != NND_METRIC_SQEUCLIDEAN) S_ALLOC(&s->cn2, (size_t)s->n);
    // queued on the searcher's stream, so the kernels that read the tables are ordered after it (the stream is
    // non-blocking: it does not wait for copies on the null stream); tab_host outlives the copy (next call syncs first)
    S_HIP(hipMemcpyAsync(s->lut, tab, sizeof(float) * 512, hipMemcpyHostToDevice, s->stream));
    return 0;
}

static int quant_launch(nnd_searcher_s *s, const float *x, int64_t xstride) {
    const int64_t blocks = (s->n + 3) / 4 < 4096 ? (s->n + 3) / 4 : 4096;
    hipLaunchKernelGGL(k_quantize_u8, dim3((unsigned)blocks), dim3(256), 0, s->stream, x, xstride, s->n, s->d, s->dcs, (const float *)s->lut,
                       (const float *)(s->lut + 256), s->codes, s->cn2);
    S_HIP(hipGetLastError());
    return 0;
}

extern "C" int32_t nnd_searcher_quantize_u8(nnd_searcher_t s, const float *rows, const float *values, int32_t n_values, uint8_t *codes_out) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_quantize_u8: null searcher"); return 1; }
    if (quant_tables(s, "nnd_searcher_quantize_u8", values, n_values)) return 1;
    nnd_scratch tmp;  // released on return, behind the synchronise below
    float *drows = nullptr;
    if (rows) {
        if (!(drows = tmp.get<float>(s, (size_t)s->n * s->d))) return 1;
        if (hipMemcpyAsync(drows, rows, sizeof(float) * (size_t)s->n * s->d, hipMemcpyHostToDevice, s->stream) != hipSuccess) {
            s->set_error("nnd_searcher_quantize_u8: H2D of the rows failed");
            return 1;
        }
    }
    int rc = rows ? quant_launch(s, drows, s->d) : quant_launch(s, s->x, s->dp);
    if (!rc && codes_out &&
        hipMemcpy2DAsync(codes_out, (size_t)s->d, s->codes, (size_t)s->dcs, (size_t)s->d, (size_t)s->n, hipMemcpyDeviceToHost, s->stream) != hipSuccess) {
        s->set_error("nnd_searcher_quantize_u8: D2H of the codes failed");
        rc = 1;
    }
    if (hipStreamSynchronize(s->stream) != hipSuccess && !rc) {
        s->set_error("nnd_searcher_quantize_u8: kernel failed: %s", hipGetErrorString(hipGetLastError()));
        rc = 1;
    }
    return rc;
}

extern "C" int32_t nnd_searcher_set_codes_u8(nnd_searcher_t s, const float *values, int32_t n_values, const uint8_t *codes) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_set_codes_u8: null searcher"); return 1; }
    if (!codes) { s->set_error("nnd_searcher_set_codes_u8: codes missing"); return 1; }
    if (quant_tables(s, "nnd_searcher_set_codes_u8", values, n_values)) return 1;
    S_HIP(hipMemsetAsync(s->codes, 0, (size_t)s->n * s->dcs, s->stream));
    S_HIP(hipMemcpy2DAsync(s->codes, (size_t)s->dcs, codes, (size_t)s->d, (size_t)s->d, (size_t)s->n, hipMemcpyHostToDevice, s->stream));
    if (s->cn2 && quant_launch(s, nullptr, 0)) return 1;
    S_HIP(hipStreamSynchronize(s->stream));
    return 0;
}

extern "C" int32_t nnd_searcher_query_proxy(nnd_searcher_t s, const float *queries, int64_t nq, int32_t k, int32_t search_k, float epsilon,
                                            int32_t *out_idx, float *out_dist) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_query_proxy: null searcher"); return 1; }
    if (!s->codes) { s->set_error("nnd_searcher_query_proxy: the searcher has no codes (nnd_searcher_quantize_u8 first)"); return 1; }
    if (search_k < 1 || search_k > 256 || k < 1 || k > search_k) {
        s->set_error("nnd_searcher_query_proxy: need 1 <= k <= search_k <= 256 (got k %d, search_k %d)", k, search_k);
        return 1;
    }
    return searcher_run(s, queries, nq, search_k, k, epsilon, Q_FORM_U8, out_idx, out_dist);
}

// ---- metric="proxy_inner_product" (pynndescent_.py:2309-2312, 2363-2371): the float walk with the rerank epilogue ----
extern "C" int32_t nnd_searcher_query_rerank(nnd_searcher_t s, const float *queries, int64_t nq, int32_t k, int32_t search_k, float epsilon,
                                             int32_t *out_idx, float *out_dist) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_query_rerank: null searcher"); return 1; }
    if (s->metric != NND_METRIC_PROXY_INNER_PRODUCT) {
        s->set_error("nnd_searcher_query_rerank: metric %d has no true distance to rerank by (the proxy inner product, %d, has)", s->metric,
                     NND_METRIC_PROXY_INNER_PRODUCT);
        return 1;
    }
    if (search_k < 1 || search_k > 256 || k < 1 || k > search_k) {
        s->set_error("nnd_searcher_query_rerank: need 1 <= k <= search_k <= 256 (got k %d, search_k %d)", k, search_k);
        return 1;
    }
    return searcher_run(s, queries, nq, search_k, k, epsilon, Q_FORM_RERANK, out_idx, out_dist);
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

// ---- the same three entries for queries and results that live on the device (include/pynnd_amd.h) ----
static int device_args(nnd_searcher_s *s, const char *who, const void *q, int64_t nq, const void *oi, const void *od) {
    if (nq > 0 && (!q || !oi || !od)) { s->set_error("%s: null device pointer", who); return 1; }
    return 0;
}
extern "C" int32_t nnd_searcher_query_device(nnd_searcher_t s, const float *queries_dev, int64_t nq, int32_t k, float epsilon,
                                             int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_query_device: null searcher"); return 1; }
    if (k < 1 || k > 256) { s->set_error("nnd_searcher_query_device: k must be in 1..256 (got %d)", k); return 1; }
    if (s->metric == NND_METRIC_PROXY_INNER_PRODUCT) {
        s->set_error("nnd_searcher_query_device: metric %d is a proxy distance: its queries go through nnd_searcher_query_rerank_device", s->metric);
        return 1;
    }
    if (device_args(s, "nnd_searcher_query_device", queries_dev, nq, out_idx_dev, out_dist_dev)) return 1;
    return searcher_run(s, queries_dev, nq, k, k, epsilon, Q_FORM_FLOAT, out_idx_dev, out_dist_dev, true, (hipStream_t)hip_stream);
}
extern "C" int32_t nnd_searcher_query_proxy_device(nnd_searcher_t s, const float *queries_dev, int64_t nq, int32_t k, int32_t search_k,
                                                   float epsilon, int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_query_proxy_device: null searcher"); return 1; }
    if (!s->codes) { s->set_error("nnd_searcher_query_proxy_device: the searcher has no codes (nnd_searcher_quantize_u8 first)"); return 1; }
    if (search_k < 1 || search_k > 256 || k < 1 || k > search_k) {
        s->set_error("nnd_searcher_query_proxy_device: need 1 <= k <= search_k <= 256 (got k %d, search_k %d)", k, search_k);
        return 1;
    }
    if (device_args(s, "nnd_searcher_query_proxy_device", queries_dev, nq, out_idx_dev, out_dist_dev)) return 1;
    return searcher_run(s, queries_dev, nq, search_k, k, epsilon, Q_FORM_U8, out_idx_dev, out_dist_dev, true, (hipStream_t)hip_stream);
}
extern "C" int32_t nnd_searcher_query_rerank_device(nnd_searcher_t s, const float *queries_dev, int64_t nq, int32_t k, int32_t search_k,
                                                    float epsilon, int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_query_rerank_device: null searcher"); return 1; }
    if (s->metric != NND_METRIC_PROXY_INNER_PRODUCT) {
        s->set_error("nnd_searcher_query_rerank_device: metric %d has no true distance to rerank by (the proxy inner product, %d, has)", s->metric,
                     NND_METRIC_PROXY_INNER_PRODUCT);
        return 1;
    }
    if (search_k < 1 || search_k > 256 || k < 1 || k > search_k) {
        s->set_error("nnd_searcher_query_rerank_device: need 1 <= k <= search_k <= 256 (got k %d, search_k %d)", k, search_k);
        return 1;
    }
    if (device_args(s, "nnd_searcher_query_rerank_device", queries_dev, nq, out_idx_dev, out_dist_dev)) return 1;
    return searcher_run(s, queries_dev, nq, search_k, k, epsilon, Q_FORM_RERANK, out_idx_dev, out_dist_dev, true, (hipStream_t)hip_stream);
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
// the tagged query: `form` NND_QUERY_FLOAT (search_k is ignored), NND_QUERY_PROXY or NND_QUERY_RERANK -- the checks of the three entries
static int tagged_args(nnd_searcher_s *s, const char *who, int32_t form, int32_t k, int32_t *search_k, const void *masks, int64_t nq, q_form *qf) {
    if (!s->tags) { s->set_error("%s: the searcher has no tags (nnd_searcher_set_tags first)", who); return 1; }
    if (s->filter_on) { s->set_error("%s: the searcher has a filter set; an allow set and query masks do not combine", who); return 1; }
    if (nq > 0 && !masks) { s->set_error("%s: masks missing", who); return 1; }
    if (form == NND_QUERY_FLOAT) {
        if (k < 1 || k > 256) { s->set_error("%s: k must be in 1..256 (got %d)", who, k); return 1; }
        if (s->metric == NND_METRIC_PROXY_INNER_PRODUCT) { s->set_error("%s: metric %d is a proxy distance: its queries take NND_QUERY_RERANK", who, s->metric); return 1; }
        *search_k = k;
        *qf = Q_FORM_FLOAT;
        return 0;
    }
    if (form == NND_QUERY_PROXY) {
        if (!s->codes) { s->set_error("%s: the searcher has no codes (nnd_searcher_quantize_u8 first)", who); return 1; }
        *qf = Q_FORM_U8;
    } else if (form == NND_QUERY_RERANK) {
        if (s->metric != NND_METRIC_PROXY_INNER_PRODUCT) { s->set_error("%s: metric %d has no true distance to rerank by", who, s->metric); return 1; }
        *qf = Q_FORM_RERANK;
    } else {
        s->set_error("%s: form must be NND_QUERY_FLOAT, NND_QUERY_PROXY or NND_QUERY_RERANK (got %d)", who, form);
        return 1;
    }
    if (*search_k < 1 || *search_k > 256 || k < 1 || k > *search_k) { s->set_error("%s: need 1 <= k <= search_k <= 256 (got k %d, search_k %d)", who, k, *search_k); return 1; }
    return 0;
}
extern "C" int32_t nnd_searcher_query_tagged(nnd_searcher_t s, int32_t form, const float *queries, int64_t nq, int32_t k, int32_t search_k, float epsilon,
                                             const uint64_t *masks, int32_t *out_idx, float *out_dist) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_query_tagged: null searcher"); return 1; }
    q_form qf;
    if (tagged_args(s, "nnd_searcher_query_tagged", form, k, &search_k, masks, nq, &qf)) return 1;
    return searcher_run(s, queries, nq, search_k, k, epsilon, qf, out_idx, out_dist, false, nullptr, masks);
}
extern "C" int32_t nnd_searcher_query_tagged_device(nnd_searcher_t s, int32_t form, const float *queries_dev, int64_t nq, int32_t k, int32_t search_k,
                                                    float epsilon, const uint64_t *masks_dev, int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_query_tagged_device: null searcher"); return 1; }
    q_form qf;
    if (tagged_args(s, "nnd_searcher_query_tagged_device", form, k, &search_k, masks_dev, nq, &qf)) return 1;
    if (device_args(s, "nnd_searcher_query_tagged_device", queries_dev, nq, out_idx_dev, out_dist_dev)) return 1;
    return searcher_run(s, queries_dev, nq, search_k, k, epsilon, qf, out_idx_dev, out_dist_dev, true, (hipStream_t)hip_stream, masks_dev);
}
