// snn.hip -- the shared-nearest-neighbour graph of square k-lists on the device: every k-NN edge (i, j) weighted by how many
// neighbours its two ends share, as a count or as the Jaccard index of the two neighbour sets (PhenoGraph, Seurat's
// FindNeighbors, scran's buildSNNGraph "number" / "jaccard", the Jarvis-Patrick criterion).  DESIGN.md section 4
// "Shared-neighbour graph".
//
//   k_snn_sets<KU, W, IdT>        each row's clean set O(i) once: (m, k) int32, -1 where the place is empty, out of range, the
//                                 row itself or a repeat of an earlier place; 65..256 places: ascending, the -1 last
//   k_snn_weights<W> / _wide<KU>  one wave per row i: a gather of the clean rows O(j) of its neighbours and a set intersection
//                                 per edge; (col, w) per place, col = -1 for a place that is not stored
//   csr_build_i32 (csr_graph.hip) the two (m, k) buffers to canonical CSR: directed as they are, or the min-union
//
// N(i) = O(i) + {i} (include_self) or O(i).  For an edge, j in O(i), i not in O(i), j not in O(j), so
// |N(i) & N(j)| = |O(i) & O(j)| + include_self * ([i in O(j)] + 1), and |N(j)| is read off the gathered row: no second gather.
//
// k_snn_sets has csr_wave_sort's split: a row of at most 16, 32 or 64 places is held by W = 16, 32 or 64 lanes, a place a lane;
// 65..256 places take the wave with KU = 2 or 4 places per lane.  A repeat is found on lane data: place t's id is read out of
// the wave (v_readlane) and compared by every lane at once; the ballot is cut to the later lanes of t's group, a constant of
// the unrolled loop, and or-ed on the scalar unit.  No LDS.
//
// k_snn_weights (k <= 64): O(i) is read out of the wave into scalar registers once per row.  Every W lanes take one neighbour
// j per pass and each lane one place of O(j); the membership test is one v_cmp_eq_i32 against a scalar per element of O(i),
// the masks or-ed on the scalar unit; the counts of place e are popcounts of its group's stretch of three masks (member of
// O(i), filled, equal to i), taken by lane e, which holds j, keeps the weight and stores it: the stores of a row are one
// coalesced pair.  The next pass's places are loaded before the current pass's compares.
// k_snn_weights_wide (65..256): O(i) is sorted, so it is copied into a wave-private LDS stretch of 128 or 256 ints padded
// with INT_MAX, and a lane looks each of its KU places of O(j) up by a branch-free lower bound (7 or 8 reads, the first ones
// broadcasts).  Only the wave that wrote the stretch reads it: a wave fence, no barrier.
//
// Integer counts, one correctly rounded division, no atomic, every store a vector store: the same bytes on every run.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "../../include/pynnd_amd.h"
#include "common.h"
#include "csr_graph.h"

#define SNN_PAD INT_MAX  // behind the last element of a sorted set
#define SNN_NONE (-2)    // a gathered place that holds nothing: equal to no element of O(i), the -1 included

// the lanes of lane t's group of W behind t
template <int W>
__device__ __forceinline__ constexpr unsigned long long snn_later_in_group(int t) {
    const int end = (t / W + 1) * W;  // one past the group's last lane
    const unsigned long long upto_end = end == 64 ? ~0ull : ((1ull << end) - 1ull);
    return upto_end & ~((2ull << t) - 1ull);
}
// bit `lane` of a wave-uniform mask
__device__ __forceinline__ bool snn_my_bit(unsigned long long mask) { return (mask >> nnd_lane()) & 1ull; }

// ---------------------------------------------------------------------------------------------- the clean sets
template <int KU, int W, typename IdT>
__global__ __launch_bounds__(256) void k_snn_sets(const IdT *__restrict__ ids, int64_t m, int32_t k, int64_t ld, int32_t *__restrict__ clean) {
    static_assert(W == 64 || KU == 1, "several places per lane: the whole wave is one row");
    constexpr int R = 64 / W;  // rows of a wave
    const int lane = nnd_lane(), sub = lane & (W - 1), group = lane / W;
    for (int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * R; first < m; first += (int64_t)gridDim.x * 4 * R) {  // wave-uniform
        const int64_t row = first + group;
        const bool live = row < m;
        int32_t v[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int e = u * 64 + sub;
            v[u] = -1;
            if (live && e < k) {
                const int64_t j = (int64_t)ids[row * ld + e];
                if (j >= 0 && j < m && j != row) v[u] = (int32_t)j;
            }
        }
        // ---- repeats: place (ut, t) against every later place of its row
        unsigned long long dup[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) dup[u] = 0ull;
#pragma unroll
        for (int ut = 0; ut < KU; ut++) {
#pragma unroll
            for (int t = 0; t < 64; t++) {
                const int32_t s = __builtin_amdgcn_readlane(v[ut], t);
#pragma unroll
                for (int u = ut; u < KU; u++) dup[u] |= __ballot(v[u] == s) & (u == ut ? snn_later_in_group<W>(t) : ~0ull);
            }
        }
#pragma unroll
        for (int u = 0; u < KU; u++)
            if (snn_my_bit(dup[u])) v[u] = -1;  // (two empty places "repeat" each other: -1 stays -1)
        if constexpr (KU == 1) {
            if (live && sub < k) clean[row * k + sub] = v[0];
        } else {
            // ---- ascending: an element's place is the number of smaller ones (they are distinct), the -1 follow in lane order
            int32_t key[KU];
            int rank[KU];
#pragma unroll
            for (int u = 0; u < KU; u++) { key[u] = v[u] >= 0 ? v[u] : SNN_PAD; rank[u] = 0; }
#pragma unroll
            for (int ut = 0; ut < KU; ut++) {
#pragma unroll
                for (int t = 0; t < 64; t++) {
                    const int32_t s = __builtin_amdgcn_readlane(key[ut], t);
#pragma unroll
                    for (int u = 0; u < KU; u++) rank[u] += s < key[u] ? 1 : 0;
                }
            }
            int filled = 0, holes = 0;  // holes: the -1 of places u' < u
#pragma unroll
            for (int u = 0; u < KU; u++) filled += __popcll(__ballot(v[u] >= 0));
#pragma unroll
            for (int u = 0; u < KU; u++) {
                const unsigned long long hole = __ballot(v[u] < 0);
                const int at = v[u] >= 0 ? rank[u] : filled + holes + nnd_prefix_popc(hole);
                if (live && at < k) clean[row * k + at] = v[u];  // (the places u * 64 + lane >= k are holes behind every place of the row)
                holes += __popcll(hole);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- the weights
struct snn_args {
    int count;  // the weight is c, not c / u
    int include_self;
    float prune;
};
// the weight of an edge whose ends have a and b elements in O and share c of them; here: whether i is in O(j)
__device__ __forceinline__ float snn_weight(const snn_args &a, int oi, int oj, int shared, int here) {
    const int c = shared + (a.include_self ? here + 1 : 0);
    const int u = oi + oj + (a.include_self ? 2 : 0) - c;  // >= 1: j is in O(i)
    return a.count ? (float)c : __fdiv_rn((float)c, (float)u);
}
__device__ __forceinline__ bool snn_stored(const snn_args &a, float w) { return w > 0.0f && w >= a.prune; }

// k <= W places a row (W = 16, 32, 64); one wave per row, R = 64 / W neighbours a pass
template <int W>
__global__ __launch_bounds__(256) void k_snn_weights(const int32_t *__restrict__ clean, int64_t m, int32_t k, snn_args a, int32_t *__restrict__ cols,
                                                     float *__restrict__ weights) {
    constexpr int R = 64 / W;
    constexpr unsigned long long GROUP = W == 64 ? ~0ull : ((1ull << W) - 1ull);
    const int lane = nnd_lane(), sub = lane & (W - 1), group = lane / W;
    const int passes = (k + R - 1) / R;
    const int my_pass = lane / R, my_shift = (lane % R) * W;  // place `lane` is taken in pass my_pass by group lane % R
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < m; row += (int64_t)gridDim.x * 4) {  // wave-uniform
        const int32_t mine = lane < k ? clean[row * k + lane] : -1;  // O(i), place `lane`
        int32_t set[W];  // ... in scalar registers
#pragma unroll
        for (int t = 0; t < W; t++) set[t] = __builtin_amdgcn_readlane(mine, t);
        const int n_i = __popcll(__ballot(mine >= 0));
        // the place of O(j) this lane takes in pass p: j is place p * R + group of O(i)
        auto gather = [&](int p) -> int32_t {
            const int32_t j = __shfl(mine, p * R + group, 64);  // (p * R + group <= 63; a place >= k holds -1)
            int32_t x = SNN_NONE;
            if (j >= 0 && sub < k) {
                x = clean[(int64_t)j * k + sub];
                if (x < 0) x = SNN_NONE;
            }
            return x;
        };
        int shared = 0, n_j = 0, here = 0;
        int32_t x = gather(0);
        for (int p = 0; p < passes; p++) {
            const int32_t next = p + 1 < passes ? gather(p + 1) : SNN_NONE;  // in flight during the compares below
            unsigned long long member = 0ull;
#pragma unroll
            for (int t = 0; t < W; t++) member |= __ballot(x == set[t]);
            const unsigned long long filled = __ballot(x >= 0), self = __ballot(x == (int32_t)row);
            if (p == my_pass) {
                shared = __popcll((member >> my_shift) & GROUP);
                n_j = __popcll((filled >> my_shift) & GROUP);
                here = ((self >> my_shift) & GROUP) != 0ull ? 1 : 0;
            }
            x = next;
        }
        if (lane < k) {
            const float w = mine >= 0 ? snn_weight(a, n_i, n_j, shared, here) : 0.0f;
            const bool keep = mine >= 0 && snn_stored(a, w);
            cols[row * k + lane] = keep ? mine : -1;
            weights[row * k + lane] = w;
        }
    }
}

// 65..256 places a row: O(i) sorted in LDS, one neighbour a pass, KU places of O(j) per lane
template <int KU>
__global__ __launch_bounds__(256) void k_snn_weights_wide(const int32_t *__restrict__ clean, int64_t m, int32_t k, snn_args a,
                                                          int32_t *__restrict__ cols, float *__restrict__ weights) {
    constexpr int CAP = KU * 64;
    __shared__ int32_t s_set[4][CAP];
    const int lane = nnd_lane();
    int32_t *set = s_set[threadIdx.x >> 6];
    for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < m; row += (int64_t)gridDim.x * 4) {  // wave-uniform
        int32_t mine[KU];
        int n_i = 0;
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int e = u * 64 + lane;
            mine[u] = e < k ? clean[row * k + e] : -1;
            set[e] = mine[u] >= 0 ? mine[u] : SNN_PAD;
            n_i += __popcll(__ballot(mine[u] >= 0));
        }
        nnd_wave_lds_sync();
        auto gather = [&](int p, int32_t (&x)[KU]) {  // O(j), j = place p of O(i); p < n_i
            const int64_t j = (int64_t)set[p];
#pragma unroll
            for (int u = 0; u < KU; u++) {
                const int e = u * 64 + lane;
                x[u] = (e < k && j < m) ? clean[j * k + e] : -1;  // (j < m: always, by the order k_snn_sets leaves)
            }
        };
        float w_mine[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) w_mine[u] = 0.0f;
        int32_t x[KU], next[KU];
#pragma unroll
        for (int u = 0; u < KU; u++) x[u] = next[u] = -1;
        if (n_i > 0) gather(0, x);
#pragma unroll
        for (int up = 0; up < KU; up++) {
            for (int t = 0; t < 64; t++) {
                const int p = up * 64 + t;
                if (p >= n_i) break;  // (sorted: the filled places are the first n_i)
                if (p + 1 < n_i) gather(p + 1, next);  // in flight during the look-ups below
                int shared = 0, n_j = 0, here = 0;
#pragma unroll
                for (int u = 0; u < KU; u++) {
                    const int32_t q = x[u] >= 0 ? x[u] : SNN_NONE;
                    int at = 0;
#pragma unroll
                    for (int step = CAP >> 1; step > 0; step >>= 1) at += set[at + step - 1] < q ? step : 0;  // elements below q; <= CAP - 1
                    shared += __popcll(__ballot(set[at] == q));
                    n_j += __popcll(__ballot(x[u] >= 0));
                    here |= __ballot(x[u] == (int32_t)row) != 0ull ? 1 : 0;
                }
                const float w = snn_weight(a, n_i, n_j, shared, here);
                if (lane == t) w_mine[up] = w;
#pragma unroll
                for (int u = 0; u < KU; u++) x[u] = next[u];
            }
        }
#pragma unroll
        for (int u = 0; u < KU; u++) {
            const int e = u * 64 + lane;
            if (e < k) {
                const bool keep = mine[u] >= 0 && snn_stored(a, w_mine[u]);
                cols[row * k + e] = keep ? mine[u] : -1;
                weights[row * k + e] = w_mine[u];
            }
        }
        nnd_wave_lds_sync();  // the next row's set is written over this one
    }
}

// ---------------------------------------------------------------------------------------------- host side
namespace {
size_t snn_room(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

int snn_check(csr_err &err, const char *who, const void *ids, int32_t id_bytes, int64_t m, int32_t k, int64_t ld, int32_t weight, float prune) {
    if (m < 0 || k < 2 || k > CSR_REG_CAP || ld < k || m >= (int64_t)0x7FFFFFF0) {
        err.set_error("%s: bad shape (m = %lld, k = %d, ld = %lld; 2 <= k <= %d)", who, (long long)m, (int)k, (long long)ld, CSR_REG_CAP);
        return 1;
    }
    if (id_bytes != 4 && id_bytes != 8) { err.set_error("%s: ids are int32 or int64 (id_bytes = %d)", who, (int)id_bytes); return 1; }
    if (weight != NND_SNN_JACCARD && weight != NND_SNN_COUNT) { err.set_error("%s: unknown weight %d", who, (int)weight); return 1; }
    if (!(prune >= 0.0f)) { err.set_error("%s: prune must be 0 or above (got %g)", who, (double)prune); return 1; }
    if (m > 0 && !ids) { err.set_error("%s: null pointer", who); return 1; }
    return 0;
}

template <typename IdT>
void snn_launch(hipStream_t st, const IdT *ids, int64_t m, int32_t k, int64_t ld, const snn_args &a, int32_t *clean, int32_t *cols, float *weights) {
    const int rows_per_block = k <= 16 ? 16 : (k <= 32 ? 8 : 4);
    const int64_t blocks = (m + rows_per_block - 1) / rows_per_block, waves = (m + 3) / 4;
    const dim3 sets((unsigned)(blocks > (1 << 20) ? (1 << 20) : blocks)), grid((unsigned)(waves > (1 << 20) ? (1 << 20) : waves)), block(256);
    if (k <= 16) {
        hipLaunchKernelGGL((k_snn_sets<1, 16, IdT>), sets, block, 0, st, ids, m, k, ld, clean);
        hipLaunchKernelGGL((k_snn_weights<16>), grid, block, 0, st, (const int32_t *)clean, m, k, a, cols, weights);
    } else if (k <= 32) {
        hipLaunchKernelGGL((k_snn_sets<1, 32, IdT>), sets, block, 0, st, ids, m, k, ld, clean);
        hipLaunchKernelGGL((k_snn_weights<32>), grid, block, 0, st, (const int32_t *)clean, m, k, a, cols, weights);
    } else if (k <= 64) {
        hipLaunchKernelGGL((k_snn_sets<1, 64, IdT>), sets, block, 0, st, ids, m, k, ld, clean);
        hipLaunchKernelGGL((k_snn_weights<64>), grid, block, 0, st, (const int32_t *)clean, m, k, a, cols, weights);
    } else if (k <= 128) {
        hipLaunchKernelGGL((k_snn_sets<2, 64, IdT>), sets, block, 0, st, ids, m, k, ld, clean);
        hipLaunchKernelGGL((k_snn_weights_wide<2>), grid, block, 0, st, (const int32_t *)clean, m, k, a, cols, weights);
    } else {
        hipLaunchKernelGGL((k_snn_sets<4, 64, IdT>), sets, block, 0, st, ids, m, k, ld, clean);
        hipLaunchKernelGGL((k_snn_weights_wide<4>), grid, block, 0, st, (const int32_t *)clean, m, k, a, cols, weights);
    }
}

// the clean sets, the weights, then the CSR stage on the two (m, k) scratch buffers
int snn_run(csr_err &err, hipStream_t st, nnd_csr_s *g, const void *ids, int32_t id_bytes, int64_t m, int32_t k, int64_t ld, const snn_args &a,
            int symmetric) {
    nnd_scratch tmp;  // released on return, behind the synchronise below
    const size_t places = (size_t)m * (size_t)k, room = snn_room(4 * (places ? places : 1));
    unsigned char *base = tmp.get<unsigned char>(&err, 3 * room);
    int rc = base ? 0 : 1;
    if (!rc) {
        int32_t *clean = (int32_t *)base, *cols = (int32_t *)(base + room);
        float *weights = (float *)(base + 2 * room);
        if (m > 0) {
            if (id_bytes == 4) snn_launch<int32_t>(st, (const int32_t *)ids, m, k, ld, a, clean, cols, weights);
            else snn_launch<int64_t>(st, (const int64_t *)ids, m, k, ld, a, clean, cols, weights);
        }
        const hipError_t launched = hipGetLastError();
        if (launched != hipSuccess) { err.set_error("nnd_snn_graph: a launch failed: %s", hipGetErrorString(launched)); rc = 1; }
        else rc = csr_build_i32(err, tmp, st, g, cols, weights, m, k, k, m > 0 ? m : 1, m > 0 ? symmetric : 0, csr_combine());  // (min-union)
    }
    const hipError_t e = hipStreamSynchronize(st);  // (on every path: the scratch goes when this returns)
    if (rc) return 1;
    if (e != hipSuccess) { (void)hipGetLastError(); err.set_error("nnd_snn_graph: a kernel failed: %s", hipGetErrorString(e)); return 1; }
    return 0;
}
}  // namespace

extern "C" int32_t nnd_snn_graph_device(int32_t device, void *hip_stream, const void *ids_dev, int32_t id_bytes, int64_t m, int32_t k, int64_t ld,
                                        int32_t weight, int32_t include_self, float prune, int32_t symmetric, nnd_csr_t *out) {
    csr_err err;
    if (!out) { err.set_error("nnd_snn_graph_device: null pointer"); return 1; }
    *out = nullptr;
    if (snn_check(err, "nnd_snn_graph_device", ids_dev, id_bytes, m, k, ld, weight, prune)) return 1;
    CSR_HIP(hipSetDevice(device));
    nnd_csr_s *g = new nnd_csr_s();
    g->device = device;
    const snn_args a{weight == NND_SNN_COUNT ? 1 : 0, include_self ? 1 : 0, prune};
    if (snn_run(err, (hipStream_t)hip_stream, g, ids_dev, id_bytes, m, k, ld, a, symmetric ? 1 : 0)) { delete g; return 1; }
    *out = g;
    return 0;
}

extern "C" int32_t nnd_snn_graph(int32_t device, const void *ids, int32_t id_bytes, int64_t m, int32_t k, int32_t weight, int32_t include_self,
                                 float prune, int32_t symmetric, int64_t *indptr, int32_t *indices, float *data, int64_t capacity, int64_t *nnz,
                                 int64_t *long_rows) {
    csr_err err;
    if (snn_check(err, "nnd_snn_graph", ids, id_bytes, m, k, k, weight, prune)) return 1;
    if (!indptr || !nnz || capacity < 0 || (capacity > 0 && (!indices || !data))) { err.set_error("nnd_snn_graph: null pointer"); return 1; }
    CSR_HIP(hipSetDevice(device));
    nnd_csr_s g;
    g.device = device;
    nnd_scratch up;
    const size_t places = (size_t)m * (size_t)k;
    unsigned char *ids_dev = up.get<unsigned char>(&err, places * (size_t)id_bytes);
    if (!ids_dev) return 1;
    hipStream_t st = nullptr;
    if (places > 0) CSR_HIP(hipMemcpyAsync(ids_dev, ids, places * (size_t)id_bytes, hipMemcpyHostToDevice, st));
    const snn_args a{weight == NND_SNN_COUNT ? 1 : 0, include_self ? 1 : 0, prune};
    if (snn_run(err, st, &g, ids_dev, id_bytes, m, k, k, a, symmetric ? 1 : 0)) return 1;
    *nnz = g.nnz;
    if (long_rows) *long_rows = g.long_rows;
    if (g.nnz > capacity) { err.set_error("nnd_snn_graph: %lld entries, room for %lld", (long long)g.nnz, (long long)capacity); return 1; }
    CSR_HIP(hipMemcpy(indptr, g.indptr, sizeof(int64_t) * (size_t)(m + 1), hipMemcpyDeviceToHost));
    if (g.nnz > 0) {
        CSR_HIP(hipMemcpy(indices, g.indices, sizeof(int32_t) * (size_t)g.nnz, hipMemcpyDeviceToHost));
        CSR_HIP(hipMemcpy(data, g.data, sizeof(float) * (size_t)g.nnz, hipMemcpyDeviceToHost));
    }
    return 0;
}
