// state.h -- host-side state of one builder handle (one GPU, one HIP stream) and the
// launch entry points implemented by the kernel translation units.
#pragma once
#include <mutex>
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/pynnd_amd.h"
#include "devmem.h"
#include "knob.h"

// device-side counters (one int64 each), reset per phase
enum {
    CNT_ACCEPT = 0,   // k-list insertions (c of pynndescent_.py:317)
    CNT_PAIRS,        // pair distances evaluated
    CNT_ROWS,         // point rows gathered
    CNT_PROPOSALS,    // proposals emitted by the join
    CNT_ACTIVE,       // vertices with >=1 new candidate
    CNT_DEGENERATE,   // rp-forest: segments whose split left one side empty
    CNT_ACTIVE_SEGS,  // rp-forest: splittable segments for the next level
    CNT_LEAVES,
    CNT_SCRATCH,      // first of the forest's four scratch words: use the names below
    CNT_MFMA = 12,    // v_mfma_f32_16x16x4_f32 instructions issued (2048 flop each) by the join / leaf kernels
    CNT_COUNT = 16
};
// The rp-forest's scratch words in stripe 0 of the counter block (rpforest.hip), one name per meaning.  Names that share a
// word are never live together: the forest runs level loop -> [recording finisher] -> [cell lists] -> finishers -> leaf tables.
enum {
    CNT_ACTIVE_POS = CNT_LEAVES,       // level loop: positions still in the level passes (k_children; CNT_LEAVES is not used by the forest otherwise)
    CNT_SCAN_TOTAL = CNT_SCRATCH,      // int32: grand total of the scan that ran last (run_scan, scan_i32_inplace, nnd_forest_stable_partition)
    CNT_FIN_COUNT = CNT_SCRATCH + 1,   // entries of the finisher work list: grows across the levels (k_children), through k_cell_lists and the big finisher
    CNT_BIG_COUNT = CNT_SCRATCH + 2,   // k_cell_lists: cells for the global-memory finisher ...
    CNT_SMALL_COUNT = CNT_SCRATCH + 3, // ... and cells finished one wave each (k_cell_lists counts [fin, big, small] in three adjacent words)
    CNT_REC_FLAGS = CNT_SCRATCH + 2,   // recording finisher (after the level loop, before any cell list): two ints, [0] node-id counter, [1] overflow flag
    CNT_MAX_LEAF = CNT_SCRATCH + 2,    // leaf tables (after the finishers): int32, longest leaf
    CNT_MAX_STAY = CNT_SCRATCH + 3,    // level loop: longest segment that stays in the level passes (k_children)
    CNT_PREP_FLAG = CNT_SCRATCH        // in counters_SUM, not in the stripes: bit 0 non-finite / bit 1 negative input (prep.hip; read by shard.hip, capi.hip data_flag)
};
static_assert(CNT_SMALL_COUNT < CNT_MFMA && CNT_MAX_STAY < CNT_MFMA, "the forest's scratch words end below CNT_MFMA");
static_assert(CNT_BIG_COUNT == CNT_FIN_COUNT + 1 && CNT_SMALL_COUNT == CNT_FIN_COUNT + 2, "k_cell_lists counts its three classes in adjacent words");
// What the host learns after every level of the forest's level loop: the six adjacent counter words from CNT_ACTIVE_SEGS on
// (copied, or written to pinned memory by k_children itself).
constexpr int NND_LEVEL_WORDS = 6;
struct nnd_level_words {
    long long segs;        // CNT_ACTIVE_SEGS: segments of the next level
    long long active_pos;  // CNT_ACTIVE_POS
    long long scan_total, fin_count, rec_flags;  // (travel along; the host reads them elsewhere)
    long long max_stay;    // CNT_MAX_STAY
};
static_assert(sizeof(nnd_level_words) == NND_LEVEL_WORDS * sizeof(long long), "hand-over layout");
static_assert(CNT_ACTIVE_POS == CNT_ACTIVE_SEGS + 1 && CNT_SCAN_TOTAL == CNT_ACTIVE_SEGS + 2 && CNT_FIN_COUNT == CNT_ACTIVE_SEGS + 3 &&
                  CNT_REC_FLAGS == CNT_ACTIVE_SEGS + 4 && CNT_MAX_STAY == CNT_ACTIVE_SEGS + NND_LEVEL_WORDS - 1,
              "nnd_level_words mirrors the counter layout");
// The words k_children writes to pinned memory itself: the level's words, then the sequence number the host spins on.
struct nnd_level_flag {
    nnd_level_words w;
    long long seq;
};
static_assert(offsetof(nnd_level_flag, seq) == NND_LEVEL_WORDS * sizeof(long long), "k_children writes seq right behind the words");

// The pinned host words of a handle (nnd_ctx::h_pin): every small latency-critical read-back has a field of its own, so no
// two of them can collide whatever order the stages run in.
struct nnd_sg_tail { uint32_t min_dist_bits, hi0; int32_t max_degree_out, hi1; };  // searchgraph.hip misc[2..3]: low halves of two 64-bit words
struct nnd_pin_words {
    long long counters[CNT_COUNT];   // mirror of counters_sum (prep.hip nnd_read_counters, shard.hip)
    nnd_level_words level;           // rpforest.hip: a level's hand-over, copy form
    long long fin_count;             // rpforest.hip: entries of the finisher work list
    long long n_big, n_small;        // rpforest.hip: k_cell_lists' other two counts (adjacent: one copy)
    int32_t rec_flags[2];            // rpforest.hip: recording finisher, [0] node ids taken, [1] node tables exhausted
    int32_t max_leaf[2];             // rpforest.hip: [0] longest leaf (the copy brings the whole 64-bit device word)
    int32_t scan_total;              // rpforest.hip: number of leaves / cells (total of a leaf-mark scan)
    int32_t sg_forward_nnz, sg_union_nnz, sg_final_nnz;  // searchgraph.hip: totals of its scans
    long long sg_misc[5];            // searchgraph.hip: [0] live keys, [1] reverse nnz, [4] rows longer than the pass handles
    nnd_sg_tail sg_tail;             // searchgraph.hip: statistics read at the end of the pass
    long long data_flags;            // CNT_PREP_FLAG of the last prep: bit 0 non-finite, bit 1 negative (prep.hip, shard.hip -> capi.hip)
    alignas(64) nnd_level_flag flag; // rpforest.hip: a level's hand-over, written by k_children through h_pin_dev (a cache line of its own)
    long long spare[17];
};
constexpr size_t NND_PIN_WORDS = 64;
static_assert(sizeof(nnd_pin_words) == NND_PIN_WORDS * sizeof(long long), "the pinned block is 64 words");
static_assert(offsetof(nnd_pin_words, n_small) == offsetof(nnd_pin_words, n_big) + sizeof(long long), "one copy brings both counts");

// Work lists of the forest's finishers: (start, len, depth) per entry, carved out of buffers that are free at that time.
struct nnd_work_list { int32_t *start, *len, *depth; };
constexpr int NND_SEG_CHILD_WORDS = 2;  // seg_child: two child ids per segment, then the finisher work list (three rows of max_segs)
constexpr int NND_WORK_LIST_ROWS = 3;
// route_roots: the root of every routed tree on one GPU; a by-cell sharded build (its roots live in shard.hip's maps) keeps
// two small per-tree tables in the upper half instead.  shard.hip enables the by-cell forest within these limits only.
constexpr int NND_ROUTE_TREES_MAX = 4096;    // trees the routing passes take
constexpr int NND_BY_CELL_TREES_MAX = 1024;  // trees of a by-cell sharded build
constexpr int NND_BY_CELL_RANK_TREES_MAX = 64;  // ... and of one rank's share of the tops
constexpr int NND_ROUTE_ROOTS_WORDS = 4096;
constexpr int NND_RR_TREE_CELLS = 2048;                                       // (trees of this rank) first cell of every local tree
constexpr int NND_RR_TREE_POS = NND_RR_TREE_CELLS + NND_BY_CELL_RANK_TREES_MAX;  // (all trees + 1) position of every tree's first own cell
static_assert(NND_ROUTE_TREES_MAX <= NND_ROUTE_ROOTS_WORDS && NND_RR_TREE_POS + NND_BY_CELL_TREES_MAX + 1 <= NND_ROUTE_ROOTS_WORDS,
              "the sub-tables of route_roots fit its allocation");
// Hot kernels add to one of NND_CNT_STRIPES copies of the counter block (stripe = workgroup id), one
// atomic per workgroup per counter: a single shared word saturates at ~12 ns per atomic on MI355X and
// would serialise a million-wave launch.  nnd_read_counters sums the stripes.
#define NND_CNT_STRIPES 512

struct nnd_tlog { int ev; float *dst; bool add; };
struct nnd_hub_result;  // hubtree.hip: the last hub search tree built on this handle (FlatTree arrays, host side)  // a pending stage timer: events ev, ev+1 -> *dst

struct nnd_handle_s {
    nnd_params p{};
    nnd_stats stats{};
    char err[512] = {0};
    nnd_devmem mem;                // owner of every device buffer below, whichever translation unit allocates it (devmem.h)
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> tev;   // event pool of the deferred stage timers (t_begin / t_end / t_flush below)
    int tev_used = 0;
    std::vector<nnd_tlog> tlog;
    hipEvent_t ev_spin = nullptr;  // nnd_sync_spin: busy-polled completion of small read-backs (lower wake-up latency)
    // a shard's host waits go through its communicator (comm.h comm_wait: abort flag of the other ranks, timeout) -- a
    // collective whose peer died would otherwise keep every later wait on the stream blocked for ever
    int (*wait_hook)(void *user, hipStream_t stream) = nullptr;
    void *wait_user = nullptr;

    // geometry
    int64_t n = 0;
    int d = 0, dp = 0;      // dp = d rounded up to 32 floats (128-byte rows)
    int k = 0, ks = 0;      // ks = k rounded up to 16 (64-byte k-list rows)
    int mc = 0, mcp = 0;    // mcp = max_candidates rounded up to 16/32/64
    int rcap = 0, pcap = 0; // reverse-offer slots per (vertex,class); proposal slots per vertex
    int iter = 0;
    int64_t own_lo = 0, own_hi = 0; // rows this handle owns (row-sharded multi-GPU build); default [0, n)
    int n_ranks = 0;                // > 0 once nnd_set_shard_bounds was called: this handle is one shard of n_ranks
    int64_t *shard_bounds = nullptr;      // device (n_ranks + 1): first row of every rank, then n
    long long *shard_cursors = nullptr;   // device (66): per-destination record cursors, [64] dropped, [65] deferred
    bool stream_owned = true;             // false after nnd_set_stream: the caller's stream is borrowed
    // A shard created by nnd_create_impl with bounds allocates the per-OWNED-row tables (cand, rbuf, active, pbuf) for its own
    // rows only; those working pointers are biased by -own_lo rows so that kernels keep indexing by global vertex id (`mem` holds the bases).
    bool lists_replicated = false;        // shard: the neighbour ids of ALL rows are refreshed before every join (shard.hip): remote targets are tested too
    const int32_t *own_order = nullptr;   // shard: the owned vertices in a spatially coherent order (shard.hip), or nullptr
    bool slim = false;
    int64_t slim_rows() const { return slim ? own_hi - own_lo : n; }  // rows those three tables hold
    int64_t slim_row0() const { return slim ? own_lo : 0; }            // first of them
    uint32_t seed = 0, tree_seed = 0;

    // data
    const float *x_orig = nullptr; // (n,d) original rows (device); owned iff x_owned
    bool x_owned = false;
    bool x_valid = false;          // x_orig holds the rows of a nnd_set_data_* call made on THIS use of the handle
    float *xp = nullptr;   // (n,dp) prepared rows: centred (euclid) or L2-normalised (cosine), zero padded
    float *nrm = nullptr;  // (n) |x-mu|^2 (euclid) or 1/0 non-zero flag (cosine)
    float2 *nr2 = nullptr;                    // (n) (nrm, |x - bf16(x)|) per row: what the forest's margin kernels read (rpforest.hip rp_band)
    uint16_t *xh = nullptr; // (n,dp) bf16 copy of xp: screening pass of the rp-forest margins (half the bytes)
    float *mean = nullptr; // (dp + 4): column means | [dp] scale of the half-precision screening copies (prep.hip k_screen_scale) | [dp + 1] 1 / scale^2 | [dp + 2] sampled max |x|

    // k-lists, rows ascending by (dist, idx)
    uint32_t *knn_e = nullptr; // (n,ks) neighbour | NEW_BIT ; 0xFFFFFFFF = empty
    float *knn_d = nullptr;    // (n,ks) alt-space distance ; +inf = empty
    float *th = nullptr;       // (n) worst distance of every row (= knn_d[v][k-1]); compact so that threshold gathers stay in L2

    // candidates / proposals
    int32_t *cand = nullptr;  // (n, 2*mcp): [new | old], -1 padded
    uint32_t *rbuf = nullptr; // (n, 2, rcap) reverse offers, hashed slots: 32-bit invertible priority of the source (sample.hip)
    uint64_t *pbuf = nullptr; // (n, pcap) proposals (dist_bits<<32 | source), hashed slots; a shard holds its OWNED rows only (biased)
    uint64_t *pbuf_r = nullptr; // shard: (n, pcap_r) proposals for vertices owned elsewhere, exported every iteration (merge.hip)
    int pcap_r = 32;
    uint8_t *pdirty = nullptr; // (n) 1 when the row has pending proposals
    uint8_t *active = nullptr; // (n) 1 when the vertex will hold >= 1 new candidate this iteration

    // rp forest (all trees in one position space P = n_trees*n)
    int64_t P = 0;
    int32_t *perm[2] = {nullptr, nullptr};    // point id per position (ping-pong)
    int32_t *pos_seg[2] = {nullptr, nullptr}; // active segment index per position or -1
    int32_t *inv = nullptr;                   // (P) seg_pt: segment of point i in tree t, point-major [tree][point], -1 once final (top levels)
    uint8_t *side = nullptr;                  // (P) 0 left / 1 right
    uint8_t *side_pt = nullptr;               // (P) the same, point-major [tree][point] (written by the fused margin pass)
    uint8_t *leaf_flag = nullptr;             // (P) 1 at the first position of every final leaf
    int32_t *scan_out = nullptr;              // (P) exclusive scan scratch
    int32_t *scan_blk = nullptr;              // block sums
    int32_t *seg_start[2] = {nullptr, nullptr}, *seg_len[2] = {nullptr, nullptr};
    int32_t *seg_nleft = nullptr, *seg_child = nullptr; // per active segment scratch
    float *hyper = nullptr;                   // (max_segs, dp+?) hyperplane + offset
    uint16_t *hyper_h = nullptr;              // (max_segs, dp) bf16 copy of the normals (screening pass)
    int64_t max_segs = 0;
    int cur = 0; // which ping-pong half holds the finished permutation
    // routing pass (rpforest.hip forest_by_routing): sample, recorded top of the trees, cells
    int64_t s_m = 0, s_stride = 0;            // sample size per tree (0: routing disabled), sampling stride
    int cell_leaf = 0;                        // recorded trees stop at nodes of <= cell_leaf sample members
    int early_stop = 8;                       // ... or when fewer than 1 / early_stop of the sample positions are still splittable
    float *xs = nullptr;                      // (s_m, dp) compact copy of the sample rows
    uint16_t *xsh = nullptr;                  // (s_m, dp) bf16
    float2 *nr2s = nullptr;                   // (s_m) the sample's copy of nr2
    int64_t node_cap = 0, cell_cap = 0;
    float *node_hf = nullptr;                 // (node_cap, dp + 4) f32 hyperplane + offset + |h|
    uint16_t *node_hh = nullptr;              // (node_cap, dp) bf16 hyperplane
    int32_t *node_child = nullptr;            // (node_cap, 2) child node id, or -2 - first sample position of a cell
    unsigned char *node_pack = nullptr;       // (node_cap, 2 * dp + 16) packed records read by the routing passes (compacted ids)
    float *node_hfc = nullptr;                // (node_cap, dp + 4) node_hf compacted like node_pack (exact rechecks of the routing passes)
    int32_t *route_roots = nullptr;           // (NND_ROUTE_ROOTS_WORDS) root node of every routed tree | sub-tables of the by-cell build (nnd_route_tree_cells / _pos)
    unsigned char *route_ws = nullptr;        // workspace of the coherent routing passes (rpforest.hip route_geometry), grow-only
    size_t route_ws_cap = 0;
    int32_t *s_leaf_depth = nullptr;          // (n_trees * s_m) depth of the cell that starts at a sample position
    int32_t *cell_count = nullptr, *cell_start = nullptr, *cell_depth = nullptr;  // (cell_cap)
    int32_t *small_list = nullptr;            // (NND_WORK_LIST_ROWS, cell_cap) work list of the cells finished one wave per cell (nnd_small_list)
    int32_t *leaf_start = nullptr, *leaf_len = nullptr; // (n_leaves) after the forest is done; grow-only buffers
    double *colsum_partial = nullptr;         // prep scratch (column sums per row block), grow-only
    size_t colsum_cap = 0;
    int64_t leaf_cap = 0;                     // allocated entries of leaf_start / leaf_len
    std::vector<int32_t> h_leaf_start, h_leaf_len;  // host copies, fetched lazily (nnd_fetch_leaf_tables)
    bool h_leaf_valid = false;
    long long *tree_begin_dev = nullptr;      // (n_trees) first leaf index of every tree
    long long *h_tree_begin = nullptr;        // pinned host copy
    int32_t *wl_start = nullptr, *wl_len = nullptr; // leaf-seeding work list when leaves had to be cut (grow-only)
    int64_t wl_cap = 0;
    int64_t n_leaves = 0;
    int32_t max_leaf = 0;
    std::vector<int64_t> tree_leaf_begin; // per tree: first leaf index (host)
    bool forest_built = false;
    bool all_new = false;  // every edge of the graph still carries the "new" flag (true from reset until the first sampling pass)
    // candidate sampling by transposition (sample.hip): the reverse offers of an iteration are placed by the target's BUCKET (a run
    // of consecutive positions of the visiting order) and appended to the targets' slot banks in LDS
    int32_t *rv_pos = nullptr;                // (n) position of every vertex in the visiting order, grow-only
    int rv_pos_gen = -1;                      // forest_gen the table was built for
    int forest_gen = 0;                       // bumped whenever a forest (a visiting order) is finished
    uint32_t *rv_in_cursor = nullptr;         // (n_buckets, 8) cursors of the record sub-regions (+ the overflow count behind them)
    uint2 *rv_in_rec = nullptr;               // (n_buckets, 8, cap) records: (slot word = invertible priority of the source, target's index in its bucket | class << 15)
    uint2 *rv_ov = nullptr;                   // overflow list (hubs): (word, bucket << 9 | class << 8 | index)
    int64_t rv_cap_in = 0, rv_cap_ov = 0, rv_cap_pos = 0;
    int rv_in_cap = 0;
    const int32_t *rv_pos_of = nullptr;       // the order rv_pos inverts
    bool rv_off = false;                      // the record regions could not be allocated: this handle samples through the hashed atomicMin slots (rbuf) from now on
    bool jb_auto = false;                     // join_blocks was left to the library: sub-steps per iteration follow the update volume (capi.hip descent_iter)
    int jb_max = 8, jb_div = 2, jb_first = 8; // the schedule: sub-steps = pow2ceil(expected insertions per row / jb_div), at most jb_max; first iteration: as if jb_first per row
    int64_t last_updates = -1;                // k-list insertions of the previous iteration (-1: unknown): picks the late-iteration form of the pass
    bool pbuf_clean = false, rbuf_clean = false;  // every proposal / reverse-offer slot is EMPTY (their consumers re-arm what they read): nnd_launch_reset_graph then skips the 2 x 512 MB memsets

    int32_t *out_idx = nullptr;           // finished graph of the host-buffer entry points (grow-only; capi.hip out_buffers)
    float *out_dist = nullptr;
    size_t out_cap = 0;
    nnd_hub_result *hub = nullptr;
    struct nnd_sg_state *sg = nullptr;    // searchgraph.hip: workspace and result of the device pruning pass
    unsigned char *exact_ws = nullptr;    // exact.hip: workspace of the exact search (query rows, partial lists, results), grow-only
    size_t exact_ws_cap = 0;

    long long *counters = nullptr;      // device NND_CNT_STRIPES x CNT_COUNT (stripe 0 doubles as scratch for single-block kernels)
    long long h_counters[CNT_COUNT] = {0};
    long long *counters_sum = nullptr;        // (CNT_COUNT) device: stripes summed by k_counters_reduce
    nnd_pin_words *h_pin = nullptr;           // pinned host words for the small latency-critical read-backs
    nnd_pin_words *h_pin_dev = nullptr;       // the same words as the device sees them: a kernel can hand the host a few values itself
    long long flag_seq = 0;                   // sequence number of the last such hand-over (rpforest.hip level_handover)

    void set_error(const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(err, sizeof(err), fmt, ap);
        va_end(ap);
    }
};
typedef nnd_handle_s nnd_ctx;

static inline int32_t *nnd_scan_total(const nnd_ctx *ctx) { return (int32_t *)(ctx->counters + CNT_SCAN_TOTAL); }
// The three work lists of the forest's finishers.  Finisher list: behind the child ids in seg_child.  One-wave list: small_list
// (its rows also serve as the owner's placement cursors until k_cell_lists fills them).  Big list: the level passes' segment
// tables of half 0 and seg_nleft, free once the level loop is over.
static inline nnd_work_list nnd_fin_list(const nnd_ctx *ctx) {
    int32_t *s = ctx->seg_child + NND_SEG_CHILD_WORDS * ctx->max_segs;
    return {s, s + ctx->max_segs, s + 2 * ctx->max_segs};
}
static inline nnd_work_list nnd_small_list(const nnd_ctx *ctx) {
    return {ctx->small_list, ctx->small_list + ctx->cell_cap, ctx->small_list + 2 * ctx->cell_cap};
}
static inline nnd_work_list nnd_big_list(const nnd_ctx *ctx) { return {ctx->seg_start[0], ctx->seg_len[0], ctx->seg_nleft}; }
static inline int32_t *nnd_route_tree_cells(const nnd_ctx *ctx) { return &ctx->route_roots[NND_RR_TREE_CELLS]; }
static inline int32_t *nnd_route_tree_pos(const nnd_ctx *ctx) { return &ctx->route_roots[NND_RR_TREE_POS]; }

// handle.hip: nnd_create with the shard geometry known up front (bounds == nullptr: a plain handle)
int nnd_create_impl(nnd_handle_t *out, const nnd_params *p, const int64_t *bounds_host, int n_ranks, int rank);
void nnd_set_global_error(const char *msg);  // handle.hip: what nnd_last_global_error returns (the entries that have no handle)
// transfer.hip: pageable host memory <-> device through pinned staging buffers (small or pinned: one plain copy); d2h returns drained
int nnd_h2d_parallel(nnd_ctx *ctx, void *dst_dev, const void *src, size_t bytes);
int nnd_d2h_parallel(nnd_ctx *ctx, void *dst, const void *src, size_t bytes, int parts);
// ---- implemented in the kernel translation units; each returns 0 / sets ctx->err ----
int nnd_launch_prep(nnd_ctx *ctx);
// the pieces of nnd_launch_prep (prep.hip), for the sharded build: a rank preps its own rows first, the others once they arrive
bool nnd_prep_column_pass(int metric);
// the `metric` argument of a ranking kernel: the code, and for the boolean family the true column count in the bits above it
// (metric.h nnd_kernel_metric: six of its formulas need d, the kernels receive dp, and no argument block grows)
static inline int nnd_kmetric(const nnd_ctx *ctx) { return ctx->p.metric >= NND_METRIC_JACCARD ? ctx->p.metric | (ctx->d << 8) : ctx->p.metric; }
void nnd_prep_mean_geometry(int64_t n, int64_t *n_s, int64_t *stride);
int nnd_prep_partial_blocks(int64_t members);
double *nnd_prep_partial_buffer(nnd_ctx *ctx, size_t doubles);
int nnd_prep_mean_partial(nnd_ctx *ctx, const float *x_rows, int64_t row0, int64_t r_lo, int64_t r_hi, int64_t stride, double *partial);
int nnd_prep_mean_finish(nnd_ctx *ctx, const double *partial, int nblocks, int64_t n_s);
int nnd_prep_rows(nnd_ctx *ctx, const float *x_all, int64_t row_lo, int64_t row_hi, bool first);
int nnd_launch_reset_graph(nnd_ctx *ctx);
int nnd_launch_forest(nnd_ctx *ctx);
// the forest of the row-sharded build, sharded by cell (rpforest.hip; driven by shard.hip)
struct nnd_tops_info {
    int64_t n_packed = 0;        // packed node records of this rank's trees
    int64_t n_low = 0, high_lo = 0;
    int32_t n_cells = 0;         // cells of this rank's trees, numbered tree-major
    int32_t tree_cells[NND_BY_CELL_RANK_TREES_MAX] = {0};  // ... per local tree
    int levels = 0;
};
int nnd_forest_sample_gather(nnd_ctx *ctx, int64_t j_lo, int64_t j_hi);
int nnd_forest_tops(nnd_ctx *ctx, int T_loc, int tree_bias, nnd_tops_info *out);
int nnd_forest_tops_pack(nnd_ctx *ctx, const nnd_tops_info *ti, int64_t node_base, const int32_t *cell_gid_dev, unsigned char *pack_dst, float *hf_dst);
int nnd_forest_route_rows(nnd_ctx *ctx, const unsigned char *pack_all, const float *hf_all, const int32_t *roots_dev, int T_all, int64_t row_lo,
                          int64_t nrows, int64_t n_cells_all, int32_t *cell_count_all);
int nnd_forest_route_records(nnd_ctx *ctx, int T_all, int64_t row_lo, int64_t nrows, int32_t n_cells_all, int32_t *cell_count_all, int32_t *count_copy,
                             const int32_t *dest_cell_dev, int G, int32_t *rec_cell, int32_t *rec_row, long long *dest_off_dev);
int nnd_forest_finish_owned(nnd_ctx *ctx, const int32_t *rec_cell, const int32_t *rec_row, int64_t n_rec, int32_t cell_base, int32_t n_cells_own,
                            const int32_t *cnt_src, int G, const int32_t *cell_depth_all, const int32_t *depth_map_dev,
                            const int32_t *tree_first_cell_dev, int T_all);
int nnd_launch_leaf_array(nnd_ctx *ctx, int32_t *out_dev /* (n_leaves,max_leaf) */);
int nnd_fetch_leaf_tables(nnd_ctx *ctx);
int nnd_launch_leaf_init(nnd_ctx *ctx);
int nnd_launch_leaf_init_array(nnd_ctx *ctx, const int32_t *leaf_host, int64_t n_leaves, int32_t max_leaf_size);
int nnd_launch_random_init(nnd_ctx *ctx);
int nnd_launch_init_from_graph(nnd_ctx *ctx, const int32_t *idx_dev, const float *dist_dev, int width);
int nnd_launch_sample(nnd_ctx *ctx);
// One process-wide lock around the creation and the tear-down of handles (hipMalloc / hipFree storms, stream and event
// creation / destruction): ranks that live as threads of one process (LOCAL transport, nnd_build_multi) create and destroy
// their state at the same moment; none of it is on a timed path, so it is simply serialised.  (handle.hip)
std::recursive_mutex &nnd_lifecycle_mutex();

int nnd_launch_sample_begin(nnd_ctx *ctx, int64_t cap, int32_t *targets_dev, uint32_t *sources_dev, long long *counts_dev);
int nnd_launch_sample_finish(nnd_ctx *ctx, const int32_t *targets_dev, const uint32_t *sources_dev, int64_t count);
int nnd_launch_proposal_export_regions(nnd_ctx *ctx, int64_t cap, int32_t *targets_dev, uint64_t *keys_dev, long long *counts_dev);
int nnd_launch_join(nnd_ctx *ctx, int64_t v_begin, int64_t v_end);
int nnd_launch_merge(nnd_ctx *ctx);
int nnd_launch_finalize(nnd_ctx *ctx, int32_t *out_idx_dev, float *out_dist_dev);
// devarray.hip: (n, d) rows of NND_DTYPE_* `dtype` -> float32 at dst (current device, stream st), dot's normalisation on request
int nnd_launch_rows_f32(hipStream_t st, const void *src, int dtype, int64_t n, int d, bool normalize, float *dst);
int nnd_launch_pairwise(nnd_ctx *ctx, const int32_t *rows_a_dev, int na, const int32_t *rows_b_dev, int nb,
                        float *out_dev);
int nnd_launch_import_proposals(nnd_ctx *ctx, const uint64_t *keys, const int32_t *targets, int64_t count);
int nnd_launch_merge_graph_rows(nnd_ctx *ctx, int64_t lo, int64_t hi, const uint32_t *e_src, const float *d_src, int n_src, int64_t stride);
int nnd_launch_clear_new_flags(nnd_ctx *ctx);
int nnd_launch_diversify_rows(nnd_ctx *ctx, int32_t *idx_dev, float *dist_dev, const nnd_prune_opts *opts,
                              const int32_t *degree_dev);
int nnd_launch_diversify_csr(nnd_ctx *ctx, const int32_t *indptr_dev, const int32_t *indices_dev, float *data_dev,
                             int *too_long_dev, const nnd_prune_opts *opts, const int32_t *degree_dev);
int nnd_launch_degree_prune(nnd_ctx *ctx, const int32_t *indptr_dev, float *data_dev, int max_degree);
void nnd_forest_stable_partition(nnd_ctx *ctx, int64_t n, const int32_t *ord, const int32_t *pos, uint8_t *side, const int32_t *seg_start,
                                 const int32_t *seg_len, int n_segs, int32_t *nleft, const int32_t *seg_child, int32_t *ord_out,
                                 int32_t *pos_out);
int nnd_hub_tree_build_impl(nnd_ctx *ctx, const int32_t *rank_order, bool rank_on_device, int leaf_size, int max_depth, int angular);
int nnd_hub_tree_fetch_impl(nnd_ctx *ctx, float *hyperplanes, float *offsets, int32_t *children, int32_t *indices, int32_t *max_leaf);
int64_t nnd_hub_tree_nodes(const nnd_ctx *ctx);
void nnd_hub_tree_free(nnd_ctx *ctx);
void nnd_search_graph_free(nnd_ctx *ctx);
int nnd_search_graph_impl(nnd_ctx *ctx, const int32_t *idx_src, const float *dist_src, bool src_on_device, int n_neighbors, float multiplier,
                          float diversify_prob, bool aware, float aggressiveness, uint32_t seed, int32_t *fwd_rows_host, float *fwd_dist_host,
                          nnd_search_graph_stats *st);
int nnd_search_graph_fetch_impl(nnd_ctx *ctx, int32_t *indptr_host, int32_t *indices_host);
int nnd_search_graph_device_impl(nnd_ctx *ctx, const int32_t **indptr_dev, const int32_t **indices_dev, int64_t *nnz);
// prepare.hip: rows of NND_DTYPE_* `dtype` gathered by `order` (nullptr: identity) into float32 rows of dp >= d floats, zero
// padded (current device, stream st): dst row i = src row order[i]
int nnd_launch_gather_rows(hipStream_t st, const void *src, int dtype, const int32_t *order, int64_t n, int d, int dp, float *dst);
// exact.hip: exact k nearest neighbours of `rows` of the point set (q == nullptr; rows == nullptr: all of them) or of the
// external queries q (host (nq, d)); host outputs (nq, k).  With `dev` the caller's arrays are on the handle's device instead:
// int32 row ids (nullptr: all rows) or (nq, d) queries of an NND_DTYPE_* type (nullptr: rows of the point set), device outputs
struct nnd_exact_dev {
    const int32_t *rows_dev;
    const void *q_dev;
    int q_dtype;
};
// `tg`: the masked search -- data row c belongs to query row i's point set iff tags_dev[c] & masks_dev[i] != 0 (device pointers: n
// tag words, nq mask words in the order of the query rows); the answer is exact among those rows, short rows end in (-1, inf)
struct nnd_exact_tags {
    const uint64_t *tags_dev;
    const uint64_t *masks_dev;
};
int nnd_exact_knn_impl(nnd_ctx *ctx, const int64_t *rows, const float *q, int64_t nq, int k, int32_t *out_idx, float *out_dist, nnd_exact_stats *st,
                       const nnd_exact_dev *dev = nullptr, const nnd_exact_tags *tg = nullptr);
int nnd_exact_slices_for(int64_t n, int64_t nq);  // data slices (gridDim.y) of the scan for nq query rows
int nnd_read_counters(nnd_ctx *ctx);  // device -> ctx->h_counters (synchronises the stream)
int nnd_zero_counters(nnd_ctx *ctx);

// Visiting order for the vertex-parallel kernels (join, finalize): the first tree's leaf order -- a permutation of
// [0, n) in which consecutive entries are close in space -- or nullptr (identity) when there is no forest or the
// handle owns only a slice of the rows.
static inline const int32_t *nnd_vertex_order(const nnd_ctx *ctx) {
    if (!ctx->forest_built || ctx->p.n_trees <= 0 || ctx->own_lo != 0 || ctx->own_hi != ctx->n) return nullptr;
    return ctx->perm[ctx->cur];
}

// Rows whose CURRENT neighbour lists this handle holds (the join's membership test reads them): every row on a plain
// handle and on a shard whose builder all-gathers the neighbour ids before every join (lists_replicated); only the owned
// slice otherwise (the owners then dedup at import / in the merge, utils.py:489-492).
static inline int64_t nnd_list_lo(const nnd_ctx *ctx) { return (ctx->n_ranks > 1 && !ctx->lists_replicated) ? ctx->own_lo : 0; }
static inline int64_t nnd_list_hi(const nnd_ctx *ctx) { return (ctx->n_ranks > 1 && !ctx->lists_replicated) ? ctx->own_hi : ctx->n; }

// Wait for everything queued on the handle's stream by polling an event: the per-level read-backs of the forest build
// are latency critical (the GPU idles until the host has the segment count), and a blocking wait wakes up late.
static inline hipError_t nnd_sync_spin(nnd_ctx *ctx) {
    if (ctx->wait_hook) return ctx->wait_hook(ctx->wait_user, ctx->stream) ? hipErrorUnknown : hipSuccess;
    if (!ctx->ev_spin) return hipStreamSynchronize(ctx->stream);
    hipError_t e = hipEventRecord(ctx->ev_spin, ctx->stream);
    if (e != hipSuccess) return e;
    while ((e = hipEventQuery(ctx->ev_spin)) == hipErrorNotReady) {
    }
    return e;
}

// Stage timers are DEFERRED: begin/end events are recorded on the stream and read back in one go (t_flush) where the
// host waits anyway, so timing a stage never drains the GPU pipeline between stages.
static inline int t_begin(nnd_ctx *ctx) {
    const int idx = ctx->tev_used;
    while ((int)ctx->tev.size() < idx + 2) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return -1;  // callers skip the timer
        ctx->tev.push_back(e);
    }
    (void)hipEventRecord(ctx->tev[idx], ctx->stream);
    ctx->tev_used += 2;
    return idx;
}
static inline void t_end(nnd_ctx *ctx, int idx, float *dst, bool add) {
    if (idx < 0) return;
    (void)hipEventRecord(ctx->tev[idx + 1], ctx->stream);
    ctx->tlog.push_back({idx, dst, add});
}
static inline void t_flush(nnd_ctx *ctx) {
    if (ctx->tlog.empty()) { ctx->tev_used = 0; return; }
    (void)nnd_sync_spin(ctx);
    for (const nnd_tlog &t : ctx->tlog) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ctx->tev[t.ev], ctx->tev[t.ev + 1]);
        if (t.add) *t.dst += ms; else *t.dst = ms;
    }
    ctx->tlog.clear();
    ctx->tev_used = 0;
}

