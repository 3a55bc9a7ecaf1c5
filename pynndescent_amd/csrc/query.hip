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
//   * quantization="uint8" (the Q_FORM_U8 instances, euclidean / cosine / dot): the walk runs on the searcher's uint8 code rows with
//     the reference's proxy distances (q_quad_proxy) and keeps search_k = proxy_beam_size * k results; its epilogue is
//     the reference's rerank (pynndescent_.py:776-789): exact distances of the RAW query to the float rows of those
//     candidates, pushed in ascending proxy order into a list of k (DESIGN.md "Quantized search").
//   * metric="proxy_inner_product" (the Q_FORM_RERANK instances, code 6): the walk runs on the float rows with the proxy
//     -log2(cos) + 1 / sqrt<q,x> and keeps search_k results; the same epilogue reranks them by -<q,x> (DESIGN.md "Proxy
//     distances").
// Random choices (ties in the tree descent, random start vertices when the tree leaf holds fewer than
// min(k, n_neighbors) points) come from the counter hash, keyed by the query's number.
// The searcher itself (searcher.h) is created, filled and quantized in searcher.hip; its allow set and tag words are made in
// searcher_filter.hip.  Here: the walk (k_query), its table and launch (searcher_run) and the query entries.
#include <vector>

#include "searcher.h"

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

// the forms of the walk, and what may enter its result list
enum q_form { Q_FORM_FLOAT, Q_FORM_U8, Q_FORM_RERANK, Q_FORM_BOOL };
enum q_filt { Q_FILT_NONE, Q_FILT_ALLOW, Q_FILT_TAGS };

// KU: result entries per lane -- entry u of lane j is position 64 u + j of the list (k <= 64 KU: 1, 2 or 4)
// FORM, a q_form:
//   Q_FORM_FLOAT   the walk on the float rows, k results.  Never touches the codes, the codebook and cn2.
//   Q_FORM_U8      quantization="uint8" (Q8, RR below) -- the walk on the code rows (k = search_k), then the rerank epilogue: the
//                  k_out best by the true distance leave.  The codebook (256 floats) sits in front of the waves' LDS.
//   Q_FORM_RERANK  the float walk with the rerank epilogue (RR without Q8: metric code 6 and nothing else) -- the walk on the float
//                  rows by the proxy inner product, the rerank by -<q,x>; the query stays as given, a zero query is searched.
//   Q_FORM_BOOL    the boolean family (BM, codes 8..16): the tree is descended with the query as given, then the query becomes its
//                  indicator row and the walk's distances are metric.h nnd_bool_dist on exact counts.
// FILT, a q_filt:
//   Q_FILT_NONE    every vertex may enter the result list; `allow`, `tags` and `qmasks` are never read.
//   Q_FILT_ALLOW   filtered (FL): a vertex enters the walk's result list only if its bit in `allow` (a bitset over the searcher's
//                  numbering, (n + 31) / 32 words) is set.  It is still visited, pushed to the frontier and expanded, so the bound,
//                  the stop rule and the hand-over to the big tier are those of the unfiltered walk relative to the allowed rows;
//                  the rerank's candidates are the walk's results and so all allowed.
//   Q_FILT_TAGS    tagged (TG): the same rule with a predicate per query -- the vertex's tag word (`tags`, (n), the searcher's
//                  numbering) must meet the query's mask word (`qmasks`, one per query of the call, read once into scalar
//                  registers: one wave serves one query).  A query whose mask is 0 has no allowed row and does not walk.
// The body of k_query below; it stays an inlined function of its own because every instance compiles to other code when the
// body stands in the kernel itself (KU 1: mostly the same instructions in another order; KU 2 and 4: up to 17 instructions more
// or fewer; profiles/search_fold_isa.txt).
template <bool BIG, int KU, int FORM, int FILT>
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
                                               const uint32_t *__restrict__ allow, const uint64_t *__restrict__ tags, const uint64_t *__restrict__ qmasks) {
    constexpr bool Q8 = FORM == Q_FORM_U8, RR = FORM == Q_FORM_U8 || FORM == Q_FORM_RERANK, BM = FORM == Q_FORM_BOOL;
    constexpr bool FL = FILT == Q_FILT_ALLOW, TG = FILT == Q_FILT_TAGS;
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
// every instance of the walk: 2 tiers x 3 KU x 4 forms x 3 filters, one signature
template <bool BIG, int KU, int FORM, int FILT>
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
                                               const float *__restrict__ cn2, int k_out,
                                               const uint32_t *__restrict__ allow /* Q_FILT_ALLOW */, const uint64_t *__restrict__ tags /* Q_FILT_TAGS */,
                                               const uint64_t *__restrict__ qmasks /* Q_FILT_TAGS: (nq) */) {
    q_body<BIG, KU, FORM, FILT>(x, xn2, dp, d, metric, n, indptr, indices, hyper, offsets, children, tree_idx, n_nodes, queries, nq, k, epsilon, min_distance,
                                n_neighbors, seed, out_idx, out_dist, overflow, qlist, n_list, scratch, scratch_stride, codes, dcs, lut, cn2, k_out, allow, tags, qmasks);
}
using q_kernel = decltype(&k_query<false, 1, Q_FORM_FLOAT, Q_FILT_NONE>);
// (k > 64: the result list as two or four entries per lane; the reference takes any k, pynndescent_.py:2275-2379)
static q_kernel query_kernel(bool big, q_form form, q_filt filt, int k) {
#define Q_KU(BIG, FORM, FILT) {k_query<BIG, 1, FORM, FILT>, k_query<BIG, 2, FORM, FILT>, k_query<BIG, 4, FORM, FILT>}
#define Q_FILTS(BIG, FORM) {Q_KU(BIG, FORM, Q_FILT_NONE), Q_KU(BIG, FORM, Q_FILT_ALLOW), Q_KU(BIG, FORM, Q_FILT_TAGS)}
#define Q_FORMS(BIG) {Q_FILTS(BIG, Q_FORM_FLOAT), Q_FILTS(BIG, Q_FORM_U8), Q_FILTS(BIG, Q_FORM_RERANK), Q_FILTS(BIG, Q_FORM_BOOL)}
    static const q_kernel table[2][4][3][3] = {Q_FORMS(false), Q_FORMS(true)};
#undef Q_FORMS
#undef Q_FILTS
#undef Q_KU
    return table[big][form][filt][k > 128 ? 2 : k > 64 ? 1 : 0];
}

// what one launch of the walk takes beside the searcher's own state (host side only: the kernel takes plain arguments)
struct q_call {
    const float *dq;
    int64_t nq;
    int k, k_out;
    float epsilon;
    int32_t *di;
    float *dd;
    uint8_t *dov;          // LDS tier: the queries' overflow flags
    const int32_t *qlist;  // big tier: the queries of this batch, n_list of them
    int n_list;
    unsigned char *scratch;
    size_t stride;
    const uint32_t *allow;
    const uint64_t *dmasks;
};
static void query_launch(q_kernel kern, unsigned grid, size_t lds, hipStream_t st, const nnd_searcher_s *s, const q_call &c) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st, s->x, s->xn2, s->dp, s->d, s->metric, s->n, s->indptr, s->indices, s->hyper, s->offsets,
                       s->children, s->tree_idx, s->n_nodes, c.dq, c.nq, c.k, c.epsilon, s->min_distance, s->n_neighbors, s->seed, c.di, c.dd, c.dov,
                       c.qlist, c.n_list, c.scratch, c.stride, (const uint8_t *)s->codes, s->dcs, (const float *)s->lut, (const float *)s->cn2, c.k_out,
                       c.allow, (const uint64_t *)s->tags, c.dmasks);
}

// every query entry point: the walk keeps k results (the float rows) or k = search_k results and reranks them to k_out
// (Q_FORM_U8: the walk on the code rows; Q_FORM_RERANK: on the float rows); out_idx / out_dist are (nq, k_out)
static int searcher_run(nnd_searcher_s *s, const float *queries, int64_t nq, int32_t k, int32_t k_out, float epsilon, q_form form,
                        int32_t *out_idx, float *out_dist, bool on_device = false, hipStream_t user_stream = nullptr,
                        const uint64_t *qmasks = nullptr /* the tagged entries: (nq) mask words, where the queries are */) {
    const bool q8 = form == Q_FORM_U8;
    const uint32_t *allow = s->filter_on ? s->allow : nullptr;  // set by nnd_searcher_set_filter*
    const q_filt filt = qmasks ? Q_FILT_TAGS : allow ? Q_FILT_ALLOW : Q_FILT_NONE;
    const q_kernel kq_lds = query_kernel(false, form, filt, k), kq_big = query_kernel(true, form, filt, k);
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
        q_call call = {dq, nq, k, k_out, epsilon, di, dd, dov, nullptr, 0, nullptr, 0, allow, dmasks};
        if (!s->force_big) {
            if (smem > 64 * 1024 && hipFuncSetAttribute((const void *)kq_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess) {
                s->set_error("nnd_searcher_query: rows of %d floats need %zu bytes of LDS per workgroup", s->d, smem); rc = 1; break;
            }
            query_launch(kq_lds, (unsigned)((nq + 3) / 4), smem, st, s, call);
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
            call.dov = nullptr;
            call.scratch = scratch;
            call.stride = stride;
            for (size_t b0 = 0; b0 < again.size() && !rc; b0 += batch) {
                call.qlist = dlist + b0;
                call.n_list = (int)(again.size() - b0 < batch ? again.size() - b0 : batch);
                query_launch(kq_big, (unsigned)((call.n_list + 3) / 4), 4 * per_wave_big + lut_bytes, st, s, call);
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

// ---- the query entries (include/pynnd_amd.h) ----
// The checks of all eight.  `form`: NND_QUERY_FLOAT (search_k is ignored: the walk keeps k), NND_QUERY_PROXY (quantization="uint8",
// pynndescent_.py:2191-2225, 2309-2364) or NND_QUERY_RERANK (metric="proxy_inner_product", pynndescent_.py:2309-2312, 2363-2371);
// `rerank_via`: how this entry's caller reaches the rerank form; `masks`: the tagged entries' mask words (tagged = true), which
// need the searcher's tags and no allow set.  On 0, *search_k is the walk's list length and *qf its form.
static int query_args(nnd_searcher_s *s, const char *who, int32_t form, int32_t k, int32_t *search_k, const char *rerank_via, bool tagged,
                      const void *masks, int64_t nq, q_form *qf) {
    if (tagged) {
        if (!s->tags) { s->set_error("%s: the searcher has no tags (nnd_searcher_set_tags first)", who); return 1; }
        if (s->filter_on) { s->set_error("%s: the searcher has a filter set; an allow set and query masks do not combine", who); return 1; }
        if (nq > 0 && !masks) { s->set_error("%s: masks missing", who); return 1; }
    }
    if (form == NND_QUERY_FLOAT) {
        if (k < 1 || k > 256) { s->set_error("%s: k must be in 1..256 (got %d)", who, k); return 1; }
        if (s->metric == NND_METRIC_PROXY_INNER_PRODUCT) { s->set_error("%s: metric %d is a proxy distance: its queries %s", who, s->metric, rerank_via); return 1; }
        *search_k = k;
        *qf = nnd_metric_bool(s->metric) ? Q_FORM_BOOL : Q_FORM_FLOAT;
        return 0;
    }
    if (form == NND_QUERY_PROXY) {
        if (!s->codes) { s->set_error("%s: the searcher has no codes (nnd_searcher_quantize_u8 first)", who); return 1; }
        *qf = Q_FORM_U8;
    } else if (form == NND_QUERY_RERANK) {
        if (s->metric != NND_METRIC_PROXY_INNER_PRODUCT) {
            if (tagged) s->set_error("%s: metric %d has no true distance to rerank by", who, s->metric);
            else s->set_error("%s: metric %d has no true distance to rerank by (the proxy inner product, %d, has)", who, s->metric, NND_METRIC_PROXY_INNER_PRODUCT);
            return 1;
        }
        *qf = Q_FORM_RERANK;
    } else {
        s->set_error("%s: form must be NND_QUERY_FLOAT, NND_QUERY_PROXY or NND_QUERY_RERANK (got %d)", who, form);
        return 1;
    }
    if (*search_k < 1 || *search_k > 256 || k < 1 || k > *search_k) { s->set_error("%s: need 1 <= k <= search_k <= 256 (got k %d, search_k %d)", who, k, *search_k); return 1; }
    return 0;
}
// queries and results that live on the device
static int device_args(nnd_searcher_s *s, const char *who, const void *q, int64_t nq, const void *oi, const void *od) {
    if (nq > 0 && (!q || !oi || !od)) { s->set_error("%s: null device pointer", who); return 1; }
    return 0;
}
static int no_searcher(const char *who) {
    snprintf(g_serr, sizeof(g_serr), "%s: null searcher", who);
    return 1;
}

extern "C" int32_t nnd_searcher_query(nnd_searcher_t s, const float *queries, int64_t nq, int32_t k, float epsilon, int32_t *out_idx,
                                      float *out_dist) {
    if (!s) return no_searcher("nnd_searcher_query");
    q_form qf;
    int32_t search_k = k;
    if (query_args(s, "nnd_searcher_query", NND_QUERY_FLOAT, k, &search_k, "go through nnd_searcher_query_rerank", false, nullptr, nq, &qf)) return 1;
    return searcher_run(s, queries, nq, search_k, k, epsilon, qf, out_idx, out_dist);
}
extern "C" int32_t nnd_searcher_query_proxy(nnd_searcher_t s, const float *queries, int64_t nq, int32_t k, int32_t search_k, float epsilon,
                                            int32_t *out_idx, float *out_dist) {
    if (!s) return no_searcher("nnd_searcher_query_proxy");
    q_form qf;
    if (query_args(s, "nnd_searcher_query_proxy", NND_QUERY_PROXY, k, &search_k, nullptr, false, nullptr, nq, &qf)) return 1;
    return searcher_run(s, queries, nq, search_k, k, epsilon, qf, out_idx, out_dist);
}
extern "C" int32_t nnd_searcher_query_rerank(nnd_searcher_t s, const float *queries, int64_t nq, int32_t k, int32_t search_k, float epsilon,
                                             int32_t *out_idx, float *out_dist) {
    if (!s) return no_searcher("nnd_searcher_query_rerank");
    q_form qf;
    if (query_args(s, "nnd_searcher_query_rerank", NND_QUERY_RERANK, k, &search_k, nullptr, false, nullptr, nq, &qf)) return 1;
    return searcher_run(s, queries, nq, search_k, k, epsilon, qf, out_idx, out_dist);
}
extern "C" int32_t nnd_searcher_query_tagged(nnd_searcher_t s, int32_t form, const float *queries, int64_t nq, int32_t k, int32_t search_k, float epsilon,
                                             const uint64_t *masks, int32_t *out_idx, float *out_dist) {
    if (!s) return no_searcher("nnd_searcher_query_tagged");
    q_form qf;
    if (query_args(s, "nnd_searcher_query_tagged", form, k, &search_k, "take NND_QUERY_RERANK", true, masks, nq, &qf)) return 1;
    return searcher_run(s, queries, nq, search_k, k, epsilon, qf, out_idx, out_dist, false, nullptr, masks);
}

extern "C" int32_t nnd_searcher_query_device(nnd_searcher_t s, const float *queries_dev, int64_t nq, int32_t k, float epsilon,
                                             int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream) {
    if (!s) return no_searcher("nnd_searcher_query_device");
    q_form qf;
    int32_t search_k = k;
    if (query_args(s, "nnd_searcher_query_device", NND_QUERY_FLOAT, k, &search_k, "go through nnd_searcher_query_rerank_device", false, nullptr, nq, &qf)) return 1;
    if (device_args(s, "nnd_searcher_query_device", queries_dev, nq, out_idx_dev, out_dist_dev)) return 1;
    return searcher_run(s, queries_dev, nq, search_k, k, epsilon, qf, out_idx_dev, out_dist_dev, true, (hipStream_t)hip_stream);
}
extern "C" int32_t nnd_searcher_query_proxy_device(nnd_searcher_t s, const float *queries_dev, int64_t nq, int32_t k, int32_t search_k,
                                                   float epsilon, int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream) {
    if (!s) return no_searcher("nnd_searcher_query_proxy_device");
    q_form qf;
    if (query_args(s, "nnd_searcher_query_proxy_device", NND_QUERY_PROXY, k, &search_k, nullptr, false, nullptr, nq, &qf)) return 1;
    if (device_args(s, "nnd_searcher_query_proxy_device", queries_dev, nq, out_idx_dev, out_dist_dev)) return 1;
    return searcher_run(s, queries_dev, nq, search_k, k, epsilon, qf, out_idx_dev, out_dist_dev, true, (hipStream_t)hip_stream);
}
extern "C" int32_t nnd_searcher_query_rerank_device(nnd_searcher_t s, const float *queries_dev, int64_t nq, int32_t k, int32_t search_k,
                                                    float epsilon, int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream) {
    if (!s) return no_searcher("nnd_searcher_query_rerank_device");
    q_form qf;
    if (query_args(s, "nnd_searcher_query_rerank_device", NND_QUERY_RERANK, k, &search_k, nullptr, false, nullptr, nq, &qf)) return 1;
    if (device_args(s, "nnd_searcher_query_rerank_device", queries_dev, nq, out_idx_dev, out_dist_dev)) return 1;
    return searcher_run(s, queries_dev, nq, search_k, k, epsilon, qf, out_idx_dev, out_dist_dev, true, (hipStream_t)hip_stream);
}
extern "C" int32_t nnd_searcher_query_tagged_device(nnd_searcher_t s, int32_t form, const float *queries_dev, int64_t nq, int32_t k, int32_t search_k,
                                                    float epsilon, const uint64_t *masks_dev, int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream) {
    if (!s) return no_searcher("nnd_searcher_query_tagged_device");
    q_form qf;
    if (query_args(s, "nnd_searcher_query_tagged_device", form, k, &search_k, "take NND_QUERY_RERANK", true, masks_dev, nq, &qf)) return 1;
    if (device_args(s, "nnd_searcher_query_tagged_device", queries_dev, nq, out_idx_dev, out_dist_dev)) return 1;
    return searcher_run(s, queries_dev, nq, search_k, k, epsilon, qf, out_idx_dev, out_dist_dev, true, (hipStream_t)hip_stream, masks_dev);
}

extern "C" int64_t nnd_searcher_last_spilled(nnd_searcher_t s) { return s ? s->last_spilled : -1; }
extern "C" int32_t nnd_searcher_set_tier(nnd_searcher_t s, int32_t tier) {
    if (!s) { snprintf(g_serr, sizeof(g_serr), "nnd_searcher_set_tier: null searcher"); return 1; }
    if (tier != 0 && tier != 1) { s->set_error("nnd_searcher_set_tier: tier must be 0 (automatic) or 1 (global-memory tier for every query)"); return 1; }
    s->force_big = tier == 1;
    return 0;
}
