// mst.hip -- the minimum spanning forest of the mutual-reachability graph of square k-lists, and the connected components of
// that graph, on the device: what HDBSCAN, robust single linkage and every "is my k-NN graph connected?" question start
// from.  Boruvka rounds on the symmetric CSR form of the graph.  DESIGN.md section 4 "Spanning forest".
//
// Definitions (tests/spanning_util.py restates them in numpy):
//   live place   (i, s) with 0 <= id < m, id != i and a distance that is finite and >= 0 (-0.0 counts as +0.0)
//   core(i)      0 when min_samples == 0; else (1 <= min_samples <= k) the min_samples-th smallest distance among row i's places
//                with a valid id and a valid distance -- the row's own place counts when it is listed, as sklearn's HDBSCAN
//                counts the point itself; with fewer such places the largest of them, with none 0.  Rows need not be sorted.
//   weight       of a live place: w = max(core(i), core(j), d) in float32
//   key          of an undirected edge: (bits of w as uint32, lo = min(i, j), hi = max(i, j)); a strict total order on distinct
//                pairs; copies of one pair (both directions, a repeated id) differ at most in w, and the smallest copy counts
//   forest       the unique minimum spanning forest under that order: what Kruskal over the sorted keys gives.  A function of
//                the input, the same bits on every run.  Zero weights are stored.
//   labels       the connected component of every point, numbered by ascending smallest member
//
// An edge (i, j) is an outgoing edge of j's component too, also where row j does not list i; a round that lets a component
// choose among its own rows' places only picks edges that are not minima of their cut (and closes cycles of three).  So the
// rounds run on the symmetric min-union of the weighted lists, the CSR matrix csr_build_i32 makes: every row sees all its
// edges, a pair once, with its smallest weight.
//
//   k_mst_core<KU, W, IdT>  core(i) by rank counting (csr_wave_sort's split: W lanes a row, KU places a lane from 65 places on),
//                           and the clean int32 ids, -1 in every place that is not live
//   k_mst_weights           w of every live place: one gather of core(j)
//   csr_build_i32           the min-union G of the (m, k) pair
//   per round  k_mst_scan<G>   a row's smallest key that leaves its component -> its record, and (w, lo) to the component by a
//                              64-bit atomicMin; a row with no such key is dead from then on (components only grow)
//              k_mst_pick      the rows whose (w, lo) is their component's offer hi by a 32-bit atomicMin
//              k_mst_hook      per root with a key: parent = the other end's component -- but of two roots that chose the same
//                              pair the smaller keeps itself (under a strict order the only cycles) -- the edge into column
//                              `round` of the row of its inner end, and the round's hook count
//              k_mst_jump      every old root's parent becomes its tree's root (pointer jumping, bounded by m)
//              k_mst_flatten   comp'[i] = parent[comp[i]]: reads one array, writes another
//   k_mst_labels_min / _flag / _rank   the smallest member per root, a prefix sum over the flags of those members, the ranks
//   csr_build_i32           the (m, rounds) edge columns to the symmetric forest
//
// Every device loop is bounded by a number derived from m: the rounds by ceil(log2 m) + 1, the pointer jumping by m; a bound
// that is met raises MST_FAULT in the round's counter and the call returns an error.  Nothing spins.  The only atomics are
// integer minima and one integer count, every store is a vector store: the same bytes on every run.
#include <limits.h>
#include <math.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "../../include/pynnd_amd.h"
#include "common.h"
#include "csr_graph.h"
#include "mst.h"

// the bits of a ballot that belong to this lane's group, moved down to bit 0
template <int W>
__device__ __forceinline__ unsigned long long mst_group_bits(unsigned long long mask) {
    if constexpr (W == 64) return mask;
    return (mask >> (nnd_lane() & ~(W - 1))) & ((1ull << W) - 1ull);
}
__device__ __forceinline__ uint64_t mst_shfl_xor64(uint64_t v, int o) {
    return ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64) << 32) | (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
}

// ---------------------------------------------------------------------------------------------- core distances, clean ids
template <int KU, int W, typename IdT>
__global__ __launch_bounds__(256) void k_mst_core(const IdT *__restrict__ ids, const float *__restrict__ dists, int64_t m, int32_t k, int64_t ld_ids,
                                                  int64_t ld_dists, int32_t min_samples, int32_t *__restrict__ clean, float *__restrict__ core) {
    static_assert(W == 64 || KU == 1, "several places per lane: the whole wave is one row");
    constexpr int R = 64 / W;  // rows of a wave
    __shared__ uint32_t s_key[KU > 1 ? 4 : 1][KU > 1 ? KU * 64 : 1];
    uint32_t *row_keys = s_key[KU > 1 ? (threadIdx.x >> 6) : 0];  // (KU > 1: this wave's copy of its row)
    const int lane = nnd_lane(), sub = lane & (W - 1), group = lane / W;
    for (int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R; first < m; first += (int64_t)gridDim.x * 4 * R) {  // wave-uniform
        const int64_t row = first + group;
        const bool live = row < m;
        uint32_t key[KU];  // the distance bits of a place that counts towards core(i)
        int count = 0;
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int e = u * 64 + sub;
            key[u] = MST_NO_KEY;
            if (live && e < k) {
                const int64_t j = (int64_t)ids[row * ld_ids + e];
                const float d = dists[row * ld_dists + e];
                int32_t id = -1;
                if (j >= 0 && j < m && d >= 0.0f && d < INFINITY) {  // (a NaN fails the first compare)
                    key[u] = __float_as_uint(d) & 0x7FFFFFFFu;       // (-0.0 is +0.0)
                    if (j != row) id = (int32_t)j;
                }
                clean[row * k + e] = id;
            }
            count += __popcll(mst_group_bits<W>(__ballot(key[u] != MST_NO_KEY)));
        }
        if constexpr (KU > 1) {
#pragma unroll
            for (int u = 0; u < KU; u++) row_keys[u * 64 + lane] = key[u];
            nnd_wave_lds_sync();
        }
        // ---- the rank of a place: the places of its row with smaller bits, or the same bits in front of it
        int rank[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) rank[u] = 0;
        for (int t = 0; t < k; t++) {  // wave-uniform; t < W * KU
            uint32_t s;
            if constexpr (KU == 1) s = (uint32_t)__shfl((int)key[0], group * W + t, 64);
            else s = row_keys[t];
#pragma unroll
            for (int u = 0; u < KU; u++) rank[u] += (s < key[u] || (s == key[u] && t < u * 64 + sub)) ? 1 : 0;
        }
        const int target = (min_samples < count ? min_samples : count) - 1;  // -1: min_samples == 0, or nothing counts
#pragma unroll
        for (int u = 0; u < KU; u++)
            if (live && key[u] != MST_NO_KEY && rank[u] == target) core[row] = __uint_as_float(key[u]);  // (one place of the row)
        if (live && sub == 0 && target < 0) core[row] = 0.0f;
        if constexpr (KU > 1) nnd_wave_lds_sync();  // the next row's keys are written over these
    }
}

// w = max(core(i), core(j), d) of every live place; 0 where the place is not live (its id is -1)
__global__ __launch_bounds__(256) void k_mst_weights(const int32_t *__restrict__ clean, const float *__restrict__ dists, int64_t m, int32_t k, int64_t ld_dists,
                                                     const float *__restrict__ core, float *__restrict__ weights) {
    const int64_t total = m * (int64_t)k;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t row = t / k;
        const int32_t j = clean[t];
        float w = 0.0f;
        if (j >= 0) {
            const float d = dists[row * ld_dists + (t - row * k)];
            w = fmaxf(fmaxf(core[row], core[j]), d == 0.0f ? 0.0f : d);
        }
        weights[t] = w;
    }
}

// ---------------------------------------------------------------------------------------------- the rounds' state
__global__ __launch_bounds__(256) void k_mst_init(mst_state s) {
    const int64_t total = s.m * (int64_t)s.cols;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        s.edge_ids[t] = -1;
        s.edge_w[t] = 0.0f;
        if (t < s.m) {
            s.comp[t] = s.parent[t] = (int32_t)t;
            s.smallest[t] = INT_MAX;
        }
    }
}

// G lanes per row of the symmetric matrix, 64 / G rows a wave.  FIRST: every point is its own component, so the row's best
// is the component's best: no gather, no atomic.
template <int G, bool FIRST>
__global__ __launch_bounds__(256) void k_mst_scan(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, const float *__restrict__ data,
                                                  mst_state s) {
    constexpr int R = 64 / G;
    const int lane = nnd_lane(), sub = lane & (G - 1), group = lane / G;
    for (int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R; first < s.m; first += (int64_t)gridDim.x * 4 * R) {  // wave-uniform
        const int64_t row = first + group;
        const bool live = row < s.m && (FIRST || !s.dead[row]);
        const int32_t ci = live ? (FIRST ? (int32_t)row : s.comp[row]) : -1;
        unsigned long long k1 = MST_EMPTY;
        uint32_t k2 = MST_NO_KEY;
        if (live) {
            const int64_t end = indptr[row + 1];
            for (int64_t e = indptr[row] + sub; e < end; e += G) {
                const int32_t j = indices[e];
                const int32_t cj = FIRST ? j : s.comp[j];
                if (cj != ci) {
                    const uint32_t lo = (uint32_t)(j < row ? j : row), hi = (uint32_t)(j < row ? row : j);
                    const unsigned long long c1 = ((unsigned long long)__float_as_uint(data[e]) << 32) | lo;
                    if (c1 < k1 || (c1 == k1 && hi < k2)) { k1 = c1; k2 = hi; }
                }
            }
        }
#pragma unroll
        for (int o = G >> 1; o > 0; o >>= 1) {  // (xor partners inside the group; every lane of the wave takes part)
            const unsigned long long o1 = mst_shfl_xor64(k1, o);
            const uint32_t o2 = (uint32_t)__shfl_xor((int)k2, o, 64);
            if (o1 < k1 || (o1 == k1 && o2 < k2)) { k1 = o1; k2 = o2; }
        }
        if (live && sub == 0) {
            if (FIRST) {
                s.dead[row] = k1 == MST_EMPTY ? 1 : 0;
                s.best1[row] = k1;
                s.best2[row] = k2;
            } else if (k1 == MST_EMPTY) {
                s.dead[row] = 1;
            } else if (k1 <= __hip_atomic_load(&s.best1[ci], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {  // (it only falls: a stale read costs an atomic)
                atomicMin(&s.best1[ci], k1);
            }
            s.rec1[row] = k1;
            s.rec2[row] = k2;
        }
    }
}

// the key has 96 bits, the atomics 64: the rows that hold their component's (w, lo) offer hi
__global__ __launch_bounds__(256) void k_mst_pick(mst_state s) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.m; i += (int64_t)gridDim.x * 256) {
        if (s.dead[i]) continue;
        const int32_t c = s.comp[i];
        if (s.rec1[i] == s.best1[c]) atomicMin(&s.best2[c], s.rec2[i]);
    }
}

__global__ __launch_bounds__(256) void k_mst_hook(mst_state s, int32_t round) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < s.m; c += (int64_t)gridDim.x * 256) {
        const unsigned long long k1 = s.best1[c];
        if (s.comp[c] != (int32_t)c || k1 == MST_EMPTY) continue;  // not a root, or a component nothing leaves
        const uint32_t lo = (uint32_t)k1, hi = s.best2[c];
        if ((int64_t)lo >= s.m || (int64_t)hi >= s.m || round >= s.cols) { atomicOr(&s.hooks[round < s.cols ? round : s.cols], MST_FAULT); continue; }
        const uint32_t inner = s.comp[lo] == (int32_t)c ? lo : hi, other = lo ^ hi ^ inner;  // exactly one end lies inside
        const int32_t c2 = s.comp[other];
        if (s.best1[c2] == k1 && s.best2[c2] == hi && (int32_t)c < c2) continue;  // both chose this pair: the smaller root stays
        s.parent[c] = c2;
        s.edge_ids[(int64_t)inner * s.cols + round] = (int32_t)other;  // (one component, one winner a round: the place is this root's)
        s.edge_w[(int64_t)inner * s.cols + round] = __uint_as_float((uint32_t)(k1 >> 32));
        atomicAdd(&s.hooks[round], 1u);
    }
}

// Every old root's parent becomes the root of its tree.  A thread writes its own parent only, with an ancestor that is
// nearer the root, so what another thread reads meanwhile is an ancestor too; a chain is at most m long.
__global__ __launch_bounds__(256) void k_mst_jump(mst_state s, int32_t round) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < s.m; c += (int64_t)gridDim.x * 256) {
        if (s.comp[c] != (int32_t)c) continue;
        int32_t p = __hip_atomic_load(&s.parent[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int64_t steps = 0;
        for (; steps <= s.m; steps++) {
            const int32_t g = __hip_atomic_load(&s.parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (g == p) break;
            __hip_atomic_store(&s.parent[c], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            p = g;
        }
        if (steps > s.m) atomicOr(&s.hooks[round + 1], MST_FAULT);  // a cycle: the next round's read reports it
    }
}

__global__ __launch_bounds__(256) void k_mst_flatten(mst_state s) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.m; i += (int64_t)gridDim.x * 256) {
        s.comp_next[i] = s.parent[s.comp[i]];
        s.best1[i] = MST_EMPTY;
        s.best2[i] = MST_NO_KEY;
    }
}

// ---------------------------------------------------------------------------------------------- labels
__global__ __launch_bounds__(256) void k_mst_labels_min(mst_state s) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.m; i += (int64_t)gridDim.x * 256) {
        int32_t *at = &s.smallest[s.comp[i]];  // (one address for a whole component: the read keeps all but the first few off it)
        if ((int32_t)i < __hip_atomic_load(at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(at, (int32_t)i);
    }
}
__global__ __launch_bounds__(256) void k_mst_labels_flag(mst_state s) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.m; i += (int64_t)gridDim.x * 256) s.flag[i] = s.smallest[s.comp[i]] == (int32_t)i ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_mst_labels_rank(mst_state s, int32_t *__restrict__ labels) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.m; i += (int64_t)gridDim.x * 256) labels[i] = s.pos[s.smallest[s.comp[i]]];
}

// ---------------------------------------------------------------------------------------------- host side
int mst_check(csr_err &err, const char *who, const void *ids, int32_t id_bytes, const float *dists, int64_t m, int32_t k, int64_t ld_ids,
              int64_t ld_dists, int32_t min_samples, const int32_t *labels, const float *core) {
    if (m < 0 || k < 1 || k > CSR_REG_CAP || ld_ids < k || ld_dists < k || m >= (int64_t)0x7FFFFFF0) {
        err.set_error("%s: bad shape (m = %lld, k = %d, ld = %lld / %lld; 1 <= k <= %d)", who, (long long)m, (int)k, (long long)ld_ids,
                      (long long)ld_dists, CSR_REG_CAP);
        return 1;
    }
    if (id_bytes != 4 && id_bytes != 8) { err.set_error("%s: ids are int32 or int64 (id_bytes = %d)", who, (int)id_bytes); return 1; }
    if (min_samples < 0 || min_samples > k) { err.set_error("%s: 0 <= min_samples <= k (got %d; k = %d)", who, (int)min_samples, (int)k); return 1; }
    if (m > 0 && (!ids || !dists || !labels || !core)) { err.set_error("%s: null pointer", who); return 1; }
    return 0;
}

namespace {
template <typename IdT>
void mst_launch_core(hipStream_t st, const IdT *ids, const float *dists, int64_t m, int32_t k, int64_t ld_ids, int64_t ld_dists, int32_t min_samples,
                     int32_t *clean, float *core) {
    const dim3 grid(mst_grid(m, k <= 16 ? 16 : (k <= 32 ? 8 : 4))), block(256);
    if (k <= 16) hipLaunchKernelGGL((k_mst_core<1, 16, IdT>), grid, block, 0, st, ids, dists, m, k, ld_ids, ld_dists, min_samples, clean, core);
    else if (k <= 32) hipLaunchKernelGGL((k_mst_core<1, 32, IdT>), grid, block, 0, st, ids, dists, m, k, ld_ids, ld_dists, min_samples, clean, core);
    else if (k <= 64) hipLaunchKernelGGL((k_mst_core<1, 64, IdT>), grid, block, 0, st, ids, dists, m, k, ld_ids, ld_dists, min_samples, clean, core);
    else if (k <= 128) hipLaunchKernelGGL((k_mst_core<2, 64, IdT>), grid, block, 0, st, ids, dists, m, k, ld_ids, ld_dists, min_samples, clean, core);
    else hipLaunchKernelGGL((k_mst_core<4, 64, IdT>), grid, block, 0, st, ids, dists, m, k, ld_ids, ld_dists, min_samples, clean, core);
}

template <bool FIRST>
void mst_launch_scan(hipStream_t st, const nnd_csr_s &sym, const mst_state &s) {
    const int64_t mean = sym.nnz / s.m;  // entries of an average row: about a lane each
    const int G = mean <= 8 ? 8 : (mean <= 16 ? 16 : (mean <= 32 ? 32 : 64));
    const dim3 grid(mst_grid(s.m, 4 * (64 / G))), block(256);
    const int64_t *indptr = sym.indptr;
    const int32_t *indices = sym.indices;
    const float *data = sym.data;
    if (G == 8) hipLaunchKernelGGL((k_mst_scan<8, FIRST>), grid, block, 0, st, indptr, indices, data, s);
    else if (G == 16) hipLaunchKernelGGL((k_mst_scan<16, FIRST>), grid, block, 0, st, indptr, indices, data, s);
    else if (G == 32) hipLaunchKernelGGL((k_mst_scan<32, FIRST>), grid, block, 0, st, indptr, indices, data, s);
    else hipLaunchKernelGGL((k_mst_scan<64, FIRST>), grid, block, 0, st, indptr, indices, data, s);
}

// the rounds on the symmetric matrix; *rounds: the rounds that hooked (the filled columns of edge_ids)
int mst_rounds(csr_err &err, hipStream_t st, const nnd_csr_s &sym, mst_state &s, int *rounds) {
    const dim3 rows(mst_grid(s.m, 256)), block(256);
    for (int round = 0; round < s.cols; round++) {  // (the last one allowed must hook nothing)
        if (round == 0) mst_launch_scan<true>(st, sym, s);
        else {
            mst_launch_scan<false>(st, sym, s);
            hipLaunchKernelGGL(k_mst_pick, rows, block, 0, st, s);
        }
        hipLaunchKernelGGL(k_mst_hook, rows, block, 0, st, s, (int32_t)round);
        unsigned int hooked = 0;
        CSR_HIP(hipMemcpyAsync(&hooked, s.hooks + round, sizeof(hooked), hipMemcpyDeviceToHost, st));
        CSR_HIP(hipStreamSynchronize(st));
        if (hooked & MST_FAULT) { err.set_error("nnd_spanning_forest: round %d met a loop bound (m = %lld)", round, (long long)s.m); return 1; }
        if (hooked == 0) { *rounds = round; return 0; }
        hipLaunchKernelGGL(k_mst_jump, rows, block, 0, st, s, (int32_t)round);
        hipLaunchKernelGGL(k_mst_flatten, rows, block, 0, st, s);
        int32_t *t = s.comp;
        s.comp = s.comp_next;
        s.comp_next = t;
    }
    err.set_error("nnd_spanning_forest: more than %d rounds (m = %lld)", (int)s.cols, (long long)s.m);
    return 1;
}

}  // namespace

int mst_forest_rounds(csr_err &err, nnd_scratch &tmp, nnd_csr_s &sym, hipStream_t st, const void *ids, int32_t id_bytes, const float *dists, int64_t m,
                      int32_t k, int64_t ld_ids, int64_t ld_dists, int32_t min_samples, float *core, mst_work &w, int *rounds) {
    mst_state &s = w.s;
    s.m = m;
    s.cols = mst_ceil_log2(m) + 1;
    const size_t rows = (size_t)m, places = rows * (size_t)k, slots = rows * (size_t)s.cols;
    size_t scan_bytes = 0;
    CSR_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, rows, rocprim::plus<int32_t>(), st));
    mst_carve c;
    c.take<int32_t>(places); c.take<float>(places); c.take<int32_t>(slots); c.take<float>(slots);
    for (int i = 0; i < 7; i++) c.take<int32_t>(rows);
    c.take<unsigned long long>(rows); c.take<unsigned long long>(rows); c.take<uint32_t>(rows); c.take<unsigned char>(rows);
    c.take<unsigned int>((size_t)s.cols + 1); c.take<unsigned char>(scan_bytes + 256);
    const size_t bytes = c.at;
    c = mst_carve{tmp.get<unsigned char>(&err, bytes)};
    if (!c.base) return 1;
    int32_t *clean = c.take<int32_t>(places);
    float *weights = c.take<float>(places);
    s.edge_ids = c.take<int32_t>(slots);
    s.edge_w = c.take<float>(slots);
    s.comp = c.take<int32_t>(rows); s.comp_next = c.take<int32_t>(rows); s.parent = c.take<int32_t>(rows); s.smallest = c.take<int32_t>(rows);
    s.flag = c.take<int32_t>(rows); s.pos = c.take<int32_t>(rows); s.rec2 = (uint32_t *)c.take<int32_t>(rows);
    s.best1 = c.take<unsigned long long>(rows); s.rec1 = c.take<unsigned long long>(rows);
    s.best2 = c.take<uint32_t>(rows); s.dead = c.take<unsigned char>(rows);
    s.hooks = c.take<unsigned int>((size_t)s.cols + 1);
    w.scan_tmp = c.take<unsigned char>(scan_bytes + 256);
    w.scan_bytes = scan_bytes;

    CSR_HIP(hipMemsetAsync(s.hooks, 0, sizeof(unsigned int) * ((size_t)s.cols + 1), st));
    if (id_bytes == 4) mst_launch_core<int32_t>(st, (const int32_t *)ids, dists, m, k, ld_ids, ld_dists, min_samples, clean, core);
    else mst_launch_core<int64_t>(st, (const int64_t *)ids, dists, m, k, ld_ids, ld_dists, min_samples, clean, core);
    hipLaunchKernelGGL(k_mst_weights, dim3(mst_grid((int64_t)places, 256)), dim3(256), 0, st, (const int32_t *)clean, dists, m, k, ld_dists,
                       (const float *)core, weights);
    hipLaunchKernelGGL(k_mst_init, dim3(mst_grid((int64_t)slots, 256)), dim3(256), 0, st, s);
    CSR_HIP(hipGetLastError());
    if (csr_build_i32(err, tmp, st, &sym, clean, weights, m, k, k, m, 1, csr_combine())) return 1;  // the min-union
    return mst_rounds(err, st, sym, s, rounds);
}

void mst_launch_join(hipStream_t st, mst_state &s, int32_t round) {
    const dim3 rows(mst_grid(s.m, 256)), block(256);
    hipLaunchKernelGGL(k_mst_pick, rows, block, 0, st, s);
    hipLaunchKernelGGL(k_mst_hook, rows, block, 0, st, s, round);
    hipLaunchKernelGGL(k_mst_jump, rows, block, 0, st, s, round);  // (nothing hooked: every root stays its own parent)
    hipLaunchKernelGGL(k_mst_flatten, rows, block, 0, st, s);
    int32_t *t = s.comp;
    s.comp = s.comp_next;
    s.comp_next = t;
}

namespace {
int mst_build(csr_err &err, nnd_scratch &tmp, nnd_csr_s &sym, hipStream_t st, nnd_csr_s *g, const void *ids, int32_t id_bytes, const float *dists, int64_t m,
              int32_t k, int64_t ld_ids, int64_t ld_dists, int32_t min_samples, int32_t *labels, float *core, int32_t *rounds_out) {
    if (rounds_out) *rounds_out = 0;
    if (m == 0) return csr_build_i32(err, tmp, st, g, nullptr, nullptr, 0, 1, 1, 1, 0, csr_combine());
    mst_work w;
    int rounds = 0;
    if (mst_forest_rounds(err, tmp, sym, st, ids, id_bytes, dists, m, k, ld_ids, ld_dists, min_samples, core, w, &rounds)) return 1;
    mst_state &s = w.s;
    if (rounds_out) *rounds_out = rounds;
    const dim3 grid(mst_grid(m, 256)), block(256);
    hipLaunchKernelGGL(k_mst_labels_min, grid, block, 0, st, s);
    hipLaunchKernelGGL(k_mst_labels_flag, grid, block, 0, st, s);
    CSR_HIP(rocprim::exclusive_scan(w.scan_tmp, w.scan_bytes, (const int32_t *)s.flag, s.pos, (int32_t)0, (size_t)m, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(k_mst_labels_rank, grid, block, 0, st, s, labels);
    CSR_HIP(hipGetLastError());
    return csr_build_i32(err, tmp, st, g, s.edge_ids, s.edge_w, m, rounds > 0 ? rounds : 1, s.cols, m, 1, csr_combine());
}

int mst_run(csr_err &err, hipStream_t st, nnd_csr_s *g, const void *ids, int32_t id_bytes, const float *dists, int64_t m, int32_t k, int64_t ld_ids,
            int64_t ld_dists, int32_t min_samples, int32_t *labels, float *core, int32_t *rounds) {
    nnd_scratch tmp;  // released on return, behind the synchronise below
    nnd_csr_s sym;    // the symmetric mutual-reachability matrix: likewise
    const int rc = mst_build(err, tmp, sym, st, g, ids, id_bytes, dists, m, k, ld_ids, ld_dists, min_samples, labels, core, rounds);
    const hipError_t e = hipStreamSynchronize(st);  // (on every path: the scratch goes when this returns)
    if (rc) return 1;
    if (e != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_spanning_forest: a kernel failed: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
}  // namespace

extern "C" int32_t nnd_spanning_forest_device(int32_t device, void *hip_stream, const void *ids_dev, int32_t id_bytes, const float *dists_dev, int64_t m,
                                              int32_t k, int64_t ld_ids, int64_t ld_dists, int32_t min_samples, int32_t *labels_dev,
                                              float *core_dev, int32_t *rounds, nnd_csr_t *out) {
    csr_err err;
    if (!out) { err.set_error("nnd_spanning_forest_device: null pointer"); return 1; }
    *out = nullptr;
    if (mst_check(err, "nnd_spanning_forest_device", ids_dev, id_bytes, dists_dev, m, k, ld_ids, ld_dists, min_samples, labels_dev, core_dev)) return 1;
    CSR_HIP(hipSetDevice(device));
    nnd_csr_s *g = new nnd_csr_s();
    g->device = device;
    if (mst_run(err, (hipStream_t)hip_stream, g, ids_dev, id_bytes, dists_dev, m, k, ld_ids, ld_dists, min_samples, labels_dev, core_dev, rounds)) {
        delete g;
        return 1;
    }
    *out = g;
    return 0;
}

extern "C" int32_t nnd_spanning_forest(int32_t device, const void *ids, int32_t id_bytes, const float *dists, int64_t m, int32_t k, int32_t min_samples,
                                       int32_t *labels, float *core, int32_t *rounds, int64_t *indptr, int32_t *indices, float *data,
                                       int64_t capacity, int64_t *nnz) {
    csr_err err;
    if (mst_check(err, "nnd_spanning_forest", ids, id_bytes, dists, m, k, k, k, min_samples, labels, core)) return 1;
    if (!indptr || !nnz || capacity < 0 || (capacity > 0 && (!indices || !data))) { err.set_error("nnd_spanning_forest: null pointer"); return 1; }
    CSR_HIP(hipSetDevice(device));
    nnd_csr_s g;
    g.device = device;
    nnd_scratch up;
    const size_t places = (size_t)m * (size_t)k;
    unsigned char *ids_dev = up.get<unsigned char>(&err, places * (size_t)id_bytes);
    float *dists_dev = up.get<float>(&err, places);
    float *core_dev = up.get<float>(&err, (size_t)m);
    int32_t *labels_dev = up.get<int32_t>(&err, (size_t)m);
    if (!ids_dev || !dists_dev || !core_dev || !labels_dev) return 1;
    hipStream_t st = nullptr;
    if (places > 0) {
        CSR_HIP(hipMemcpyAsync(ids_dev, ids, places * (size_t)id_bytes, hipMemcpyHostToDevice, st));
        CSR_HIP(hipMemcpyAsync(dists_dev, dists, places * sizeof(float), hipMemcpyHostToDevice, st));
    }
    if (mst_run(err, st, &g, ids_dev, id_bytes, dists_dev, m, k, k, k, min_samples, labels_dev, core_dev, rounds)) return 1;
    *nnz = g.nnz;
    if (g.nnz > capacity) { err.set_error("nnd_spanning_forest: %lld entries, room for %lld", (long long)g.nnz, (long long)capacity); return 1; }
    if (m > 0) {
        CSR_HIP(hipMemcpy(labels, labels_dev, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
        CSR_HIP(hipMemcpy(core, core_dev, sizeof(float) * (size_t)m, hipMemcpyDeviceToHost));
    }
    CSR_HIP(hipMemcpy(indptr, g.indptr, sizeof(int64_t) * (size_t)(m + 1), hipMemcpyDeviceToHost));
    if (g.nnz > 0) {
        CSR_HIP(hipMemcpy(indices, g.indices, sizeof(int32_t) * (size_t)g.nnz, hipMemcpyDeviceToHost));
        CSR_HIP(hipMemcpy(data, g.data, sizeof(float) * (size_t)g.nnz, hipMemcpyDeviceToHost));
    }
    return 0;
}
