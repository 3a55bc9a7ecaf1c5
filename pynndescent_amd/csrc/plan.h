// plan.h -- the plan of a handle: the parameter checks of nnd_create and every scalar it derives from the parameters (padded
// widths, table capacities, the routing forest's geometry).  Host code without HIP headers: handle.hip copies a plan into the
// nnd_ctx and allocates by it, shard.hip asks the routing predicate, tests/plan_cpu.cpp pins the figures without a device.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/pynnd_amd.h"
#include "knob.h"

constexpr int NND_PLAN_MAX_K = 256;  // = NND_WIDE_K (common.h; handle.hip asserts it)

static inline int nnd_check_params(const nnd_params *p, char *err, size_t errlen) {
    if (p->n < 1 || p->dim < 1) { snprintf(err, errlen, "nnd_create: need n >= 1 and dim >= 1 (got n=%lld dim=%d)", (long long)p->n, p->dim); return 1; }
    if (p->metric < NND_METRIC_SQEUCLIDEAN || p->metric > NND_METRIC_YULE || p->metric == NND_METRIC_PROXY_INNER_PRODUCT + 1 /* 7 is no code */) { snprintf(err, errlen, "nnd_create: unknown metric %d", p->metric); return 1; }
    if (p->metric >= NND_METRIC_JACCARD && p->dim >= (1 << 23)) { snprintf(err, errlen, "nnd_create: the boolean metrics need dim < 2^23 (got %d)", p->dim); return 1; }
    if (p->n_neighbors < 1 || p->n_neighbors > NND_PLAN_MAX_K) { snprintf(err, errlen, "nnd_create: n_neighbors must be in 1..%d (got %d)", NND_PLAN_MAX_K, p->n_neighbors); return 1; }
    if (p->max_candidates < 1 || p->max_candidates > 128) { snprintf(err, errlen, "nnd_create: max_candidates must be in 1..128 (got %d)", p->max_candidates); return 1; }
    if (p->n_trees < 0 || p->n_trees > 4096 || p->leaf_size < 1) { snprintf(err, errlen, "nnd_create: bad n_trees (0..4096) / leaf_size"); return 1; }
    if (p->n >= (int64_t)0x7FFFFFF0) { snprintf(err, errlen, "nnd_create: n too large for int32 ids"); return 1; }
    if (p->n_trees > 0 && (int64_t)p->n_trees * p->n >= (int64_t)0x7FFFFFF0) {
        snprintf(err, errlen, "nnd_create: n_trees * n = %lld exceeds the forest's int32 position space (2^31)", (long long)((int64_t)p->n_trees * p->n));
        return 1;
    }
    return 0;
}

// one shard of a row-sharded build: bounds[r] is the first row of rank r, bounds[n_ranks] = n
static inline int nnd_check_shard_bounds(int64_t n, const int64_t *bounds, int n_ranks, int rank, char *err, size_t errlen) {
    if (n_ranks < 1 || n_ranks > 64 || rank < 0 || rank >= n_ranks || bounds[0] != 0 || bounds[n_ranks] != n) {
        snprintf(err, errlen, "nnd_create: bad shard bounds (need 1 <= n_ranks <= 64, bounds from 0 to n)");
        return 1;
    }
    for (int r = 0; r < n_ranks; r++)
        if (bounds[r] > bounds[r + 1]) { snprintf(err, errlen, "nnd_create: shard bounds must not decrease"); return 1; }
    return 0;
}

// Routing pass (rpforest.hip): the top of the trees is built from every 16th point when the set is large
// enough for that sample to resolve cells of a few hundred points, and rows fit the route kernel's registers.
// (Round 4: stride 8 / cells of <= 48 sample members -> 16 / 24: the same cells on average, half the sample
// passes -- 4.66 -> 4.28 ms per forest at 1 M x 8 trees, 14.5 -> 12.2 ms at 10 M x 2; in a sharded build the
// sample tops are the part of the forest that is not divided by the number of ranks.)
// NND_FOREST_WHOLE=1 forces the whole-set level-synchronous build (A/B measurements).
static inline bool nnd_plan_routes(int64_t n, int dim, int flags) {
    const char *whole = nnd_knob("NND_FOREST_WHOLE");
    return !(flags & NND_FLAG_NO_GRAPH) && n >= 131072 && ((dim + 31) & ~31) <= 256 && !(whole && whole[0] == '1');
}

// join_blocks = 0: chosen here.  A row takes at most 64 updates per merge (its proposal slots); rows of more than 64 neighbours
// change by more than that per iteration while the graph is poor (the reference's heaps have no such bound, utils.py:459-500), so
// their iterations are cut into sub-steps (join a part of the vertices, merge, ...: pynndescent_.py:239-261 does the same in
// blocks of 16384 vertices) until the slots of an iteration add up to 2 k.
// More than 64 candidates per class run as five passes of the 64-slot join (join.hip launch_join_blocked) that all deposit into
// the same 64 proposal slots of a row: twice the sub-steps, so that a merge empties the slots between them (round-5 advisor item).
static inline int nnd_auto_join_blocks(int k, int mc) { return (k <= 64 ? 1 : (k + 31) / 32) * (mc > 64 ? 2 : 1); }

static inline int nnd_knob_int(const char *name, int unset, int at_least) {
    const char *e = nnd_knob(name);
    const int v = e ? atoi(e) : unset;
    return v < at_least ? at_least : v;
}

// What a build takes from the plan apart from the handle's geometry (handle.hip arm_for_build: a parked handle is re-armed by it).
struct nnd_join_plan {
    int join_blocks = 0;                    // effective sub-steps per iteration
    bool jb_auto = false;
    int jb_max = 8, jb_div = 2, jb_first = 8;  // the schedule of nnd_join_substeps (capi.hip)
};
static inline nnd_join_plan nnd_plan_join(const nnd_params &p) {
    nnd_join_plan j;
    j.jb_auto = p.join_blocks < 1;
    j.join_blocks = j.jb_auto ? nnd_auto_join_blocks(p.n_neighbors, p.max_candidates) : p.join_blocks;
    j.jb_max = nnd_knob_int("NND_JB_MAX", j.jb_max, 1);  // experiments: the schedule of nnd_join_substeps
    j.jb_div = nnd_knob_int("NND_JB_DIV", j.jb_div, 1);
    j.jb_first = nnd_knob_int("NND_JB_FIRST", j.jb_first, 0);
    return j;
}

struct nnd_plan : nnd_join_plan {
    int64_t n = 0, own_lo = 0, own_hi = 0;  // rows, and the rows this handle owns
    int n_ranks = 0;                        // > 0: one shard of a row-sharded build
    bool slim = false;                      // ... of several: the per-owned-row tables hold the owned rows only
    int d = 0, dp = 0, k = 0, ks = 0, mc = 0, mcp = 0, rcap = 0, pcap = 0;
    int64_t P = 0, max_segs = 0;            // the forest's position space and segment tables (0: no forest)
    int64_t s_stride = 0, s_m = 0;          // routing forest: sampling stride, sample size per tree (0: no routing)
    int early_stop = 8, cell_leaf = 0;      // (early_stop is read by the routing forest only, which sets it below)
    int64_t node_cap = 0, cell_cap = 0;
};

// parameters that passed nnd_check_params (and bounds that passed nnd_check_shard_bounds, or nullptr: a plain handle)
static inline nnd_plan nnd_make_plan(const nnd_params &p, const int64_t *bounds, int n_ranks, int rank) {
    nnd_plan pl;
    static_cast<nnd_join_plan &>(pl) = nnd_plan_join(p);
    pl.n = p.n;
    pl.own_hi = p.n;
    if (bounds) {
        pl.n_ranks = n_ranks;
        pl.own_lo = bounds[rank];
        pl.own_hi = bounds[rank + 1];
        pl.slim = n_ranks > 1;
    }
    pl.d = p.dim;
    pl.dp = (p.dim + 31) & ~31;
    pl.k = p.n_neighbors;
    pl.ks = (p.n_neighbors + 15) & ~15;
    pl.mc = p.max_candidates;
    pl.mcp = p.max_candidates <= 16 ? 16 : (p.max_candidates <= 32 ? 32 : (p.max_candidates <= 64 ? 64 : 128));  // (128: the blocked passes of join.hip)
    if (pl.ks > 64 && pl.mcp < 32) pl.mcp = 32;  // wide rows: the join that reads neighbour lists from global memory (join.hip k_local_join_w)
    // reverse-offer slots per (vertex, class): at least max_candidates rounded up to a power of two, so that a vertex
    // can fill its list from reverse offers alone, as the reference's max_candidates-deep heaps can (utils.py:277-306)
    pl.rcap = p.max_candidates <= 32 ? 32 : (p.max_candidates <= 64 ? 64 : 128);  // (128: hashed slots, the bucketed pass stops at 64)
    pl.pcap = 64;  // one candidate per lane in k_merge (merge.h NCHUNK = 1)
    // experiments: reverse-offer slots per (vertex, class) / proposal slots per vertex, a power of two <= 64
    if (const int r = nnd_knob_int("NND_RCAP", 0, 0); r == 16 || r == 32 || r == 64) pl.rcap = r;
    if (const int r = nnd_knob_int("NND_PCAP", 0, 0); r == 16 || r == 32 || r == 64) pl.pcap = r;
    if (p.n_trees > 0) {
        pl.P = (int64_t)p.n_trees * p.n;
        pl.max_segs = pl.P / (p.leaf_size + 1) + p.n_trees + 8;
        if (nnd_plan_routes(p.n, p.dim, p.flags)) {
            pl.s_stride = nnd_knob_int("NND_SAMPLE_STRIDE", 16, 2);
            pl.s_m = p.n / pl.s_stride;
            pl.early_stop = nnd_knob_int("NND_EARLY_STOP", 0, INT32_MIN);
            pl.cell_leaf = nnd_knob_int("NND_CELL_LEAF", 24, 8);  // x stride: cells of <= ~450 points, ~215 on average (one wave per cell)
            const int64_t Ps = (int64_t)p.n_trees * pl.s_m;
            pl.node_cap = Ps / (pl.cell_leaf / 4) + 4 * p.n_trees + 64;
            pl.cell_cap = pl.node_cap + p.n_trees;
            pl.max_segs += pl.cell_cap;
        }
    }
    return pl;
}
