// plan_cpu.cpp -- the handle's plan (pynndescent_amd/csrc/plan.h) on a CPU, driven by test_plan_cpu.py: `plan_cpu <case>` prints
// every field of the plan nnd_make_plan derives for the case's parameters, one "name value" per line; a bad_* case prints the
// return value and the text of nnd_check_params / nnd_check_shard_bounds.  Host compiler only: the header needs no HIP.
#include <string.h>

#include <string>

#include "plan.h"

static nnd_params base(int64_t n, int dim, int k, int mc, int trees, int leaf) {
    nnd_params p;
    memset(&p, 0, sizeof(p));
    p.n = n;
    p.dim = dim;
    p.metric = NND_METRIC_SQEUCLIDEAN;
    p.n_neighbors = k;
    p.max_candidates = mc;
    p.n_trees = trees;
    p.leaf_size = leaf;
    return p;
}

static int show(const nnd_params &p, const int64_t *bounds = nullptr, int n_ranks = 0, int rank = 0) {
    char err[512] = {0};
    if (nnd_check_params(&p, err, sizeof(err)) || (bounds && nnd_check_shard_bounds(p.n, bounds, n_ranks, rank, err, sizeof(err)))) {
        printf("refused 1\n%s\n", err);
        return 0;
    }
    const nnd_plan pl = nnd_make_plan(p, bounds, n_ranks, rank);
    printf("n %lld\nown_lo %lld\nown_hi %lld\nn_ranks %d\nslim %d\n", (long long)pl.n, (long long)pl.own_lo, (long long)pl.own_hi, pl.n_ranks, (int)pl.slim);
    printf("d %d\ndp %d\nk %d\nks %d\nmc %d\nmcp %d\nrcap %d\npcap %d\njoin_blocks %d\njb_auto %d\n", pl.d, pl.dp, pl.k, pl.ks, pl.mc, pl.mcp, pl.rcap, pl.pcap,
           pl.join_blocks, (int)pl.jb_auto);
    printf("P %lld\nmax_segs %lld\ns_stride %lld\ns_m %lld\nearly_stop %d\ncell_leaf %d\nnode_cap %lld\ncell_cap %lld\n", (long long)pl.P, (long long)pl.max_segs,
           (long long)pl.s_stride, (long long)pl.s_m, pl.early_stop, pl.cell_leaf, (long long)pl.node_cap, (long long)pl.cell_cap);
    printf("routes %d\n", (int)nnd_plan_routes(p.n, p.dim, p.flags));
    return 0;
}

int main(int argc, char **argv) {
    const std::string c = argc > 1 ? argv[1] : "";
    const nnd_params bench = base(1000000, 128, 15, 15, 8, 60), edge = base(131072, 8, 10, 10, 2, 30), small = base(1000, 8, 10, 10, 2, 30);
    nnd_params p = bench;
    if (c == "bench") return show(bench);
    if (c == "route_edge") return show(edge);
    if (c == "route_below") { p = edge; p.n = 131071; return show(p); }
    if (c == "route_wide_rows") { p = bench; p.n = 200000; p.dim = 257; return show(p); }
    if (c == "route_no_graph") { p.flags = NND_FLAG_NO_GRAPH; return show(p); }
    if (c == "wide_k") { p.n_neighbors = 70; p.max_candidates = 10; return show(p); }
    if (c == "wide_k_mc") { p.n_neighbors = 70; p.max_candidates = 65; return show(p); }
    if (c.rfind("mc_", 0) == 0) { p.max_candidates = atoi(c.c_str() + 3); return show(p); }  // mc_16, mc_17, ...
    if (c == "explicit_jb") { p.join_blocks = 5; return show(p); }
    const int64_t two[3] = {0, 400, 1000}, one[2] = {0, 1000};
    if (c == "shard") return show(small, two, 2, 1);
    if (c == "shard_one_rank") return show(small, one, 1, 0);
    // ---- refusals
    p = small;
    if (c == "bad_n") { p.n = 0; return show(p); }
    if (c == "bad_dim") { p.dim = 0; return show(p); }
    if (c == "bad_metric") { p.metric = 7; return show(p); }
    if (c == "bad_k_low") { p.n_neighbors = 0; return show(p); }
    if (c == "bad_k_high") { p.n_neighbors = NND_PLAN_MAX_K + 1; return show(p); }
    if (c == "bad_mc_low") { p.max_candidates = 0; return show(p); }
    if (c == "bad_mc_high") { p.max_candidates = 129; return show(p); }
    if (c == "bad_trees") { p.n_trees = 4097; return show(p); }
    if (c == "bad_leaf") { p.leaf_size = 0; return show(p); }
    if (c == "bad_n_int32") { p.n = 0x7FFFFFF0; return show(p); }
    if (c == "bad_positions") { p.n = 0x7FFFFFF0 / 16; p.n_trees = 16; return show(p); }
    const int64_t from_one[3] = {1, 400, 1000}, falling[4] = {0, 600, 400, 1000}, short_end[3] = {0, 400, 999};
    if (c == "bad_bounds_start") return show(small, from_one, 2, 1);
    if (c == "bad_bounds_falling") return show(small, falling, 3, 1);
    if (c == "bad_bounds_end") return show(small, short_end, 2, 1);
    if (c == "bad_ranks") return show(small, two, 65, 1);  // (refused before any bound is read)
    fprintf(stderr, "unknown case %s\n", c.c_str());
    return 2;
}
