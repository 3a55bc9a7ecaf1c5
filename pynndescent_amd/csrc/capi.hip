// capi.hip -- the extern "C" entry points of include/pynnd_amd.h that work on a live handle: argument checks, and the
// orchestration that mirrors nn_descent / nn_descent_internal (reference pynndescent_.py:266-366).  Handle lifetime is
// handle.hip, the staged copies are transfer.hip, the sizing rules are plan.h.  No kernel here.
#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "metric.h"
#include "state.h"

extern "C" int32_t nnd_abi_version(void) { return NND_ABI_VERSION; }

// What an entry point needs of its handle; checked in this order.
enum { NEED_GRAPH = 1, NEED_PREP = 2, NEED_DATA = 4 };
static int need(nnd_ctx *ctx, int mask, const char *who) {
    // build entry points: the handle must hold the graph state (not an auxiliary NND_FLAG_NO_GRAPH handle)
    if ((mask & NEED_GRAPH) && (ctx->p.flags & NND_FLAG_NO_GRAPH)) { ctx->set_error("this handle was created with NND_FLAG_NO_GRAPH: it has no k-lists / candidate tables (pruning pass and hub tree only)"); return 1; }
    if ((mask & NEED_PREP) && (ctx->p.flags & NND_FLAG_NO_PREP)) { ctx->set_error("%s: this handle holds no prepared rows (NND_FLAG_NO_PREP)", who); return 1; }
    if ((mask & NEED_DATA) && (!ctx->x_orig || !ctx->x_valid)) { ctx->set_error("no data set (call nnd_set_data_host/device first)"); return 1; }
    return 0;
}
static int enter(nnd_ctx *ctx, int mask, const char *who) {
    if (!ctx) { nnd_set_global_error("null handle"); return 1; }
    NND_HIP_CHECK(hipSetDevice(ctx->p.device));
    return need(ctx, mask, who);
}
#define ENTER(ctx, mask) \
    if (enter(ctx, mask, __func__)) return 1

// One timed stage: fn() launches it between two deferred timer events (state.h t_begin / t_end).  The caller flushes.
template <typename F>
static int timed(nnd_ctx *ctx, float *dst, bool add, F fn) {
    const int t_ = t_begin(ctx);
    if (fn()) return 1;
    t_end(ctx, t_, dst, add);
    return 0;
}
static float *iter_slot(nnd_ctx *ctx, float *per_iter) {  // the stats block records 64 iterations
    static float sink;
    return ctx->iter < 64 ? &per_iter[ctx->iter] : &sink;
}
static int stage_prep(nnd_ctx *ctx) {
    return timed(ctx, &ctx->stats.ms_prep, false, [&] { return nnd_launch_prep(ctx) || (!(ctx->p.flags & NND_FLAG_NO_GRAPH) && nnd_launch_reset_graph(ctx)); });
}
static int stage_forest(nnd_ctx *ctx) { return timed(ctx, &ctx->stats.ms_forest, false, [&] { return nnd_launch_forest(ctx); }); }
static int stage_leaf_init(nnd_ctx *ctx) { return timed(ctx, &ctx->stats.ms_leaf_init, false, [&] { return nnd_launch_leaf_init(ctx); }); }
static int stage_random_init(nnd_ctx *ctx) { return timed(ctx, &ctx->stats.ms_random_init, false, [&] { return nnd_launch_random_init(ctx); }); }
static int stage_sample(nnd_ctx *ctx) { return timed(ctx, iter_slot(ctx, ctx->stats.ms_sample), false, [&] { return nnd_launch_sample(ctx); }); }
static int stage_join(nnd_ctx *ctx, int64_t v0, int64_t v1, bool add) {
    return timed(ctx, iter_slot(ctx, ctx->stats.ms_join), add, [&] { return nnd_launch_join(ctx, v0, v1); });
}
static int stage_merge(nnd_ctx *ctx) { return timed(ctx, iter_slot(ctx, ctx->stats.ms_merge), true, [&] { return nnd_launch_merge(ctx); }); }
static int stage_finalize(nnd_ctx *ctx, int32_t *out_idx_dev, float *out_dist_dev) {
    return timed(ctx, &ctx->stats.ms_finalize, false, [&] { return nnd_launch_finalize(ctx, out_idx_dev, out_dist_dev); });
}
static int flushed(nnd_ctx *ctx, int rc) {  // a granular entry: its stage, then the timers (no flush after a failure)
    if (rc) return 1;
    t_flush(ctx);
    return 0;
}

static int after_data(nnd_ctx *ctx) {
    if (ctx->p.flags & NND_FLAG_NO_PREP) return 0;  // hub-tree handle: the original rows are all it reads
    return flushed(ctx, stage_prep(ctx));
}

extern "C" int32_t nnd_set_data_host(nnd_handle_t ctx, const float *x) {
    ENTER(ctx, 0);
    if (!x) { ctx->set_error("nnd_set_data_host: null data"); return 1; }
    if (!(ctx->x_owned && ctx->x_orig)) {  // the handle's own copy of the rows: allocated once, reused by later calls
        if (!ctx->mem.alloc(&ctx->x_orig, (size_t)ctx->n * ctx->d)) { ctx->set_error("nnd_set_data_host: out of device memory for the handle's copy of the rows"); return 1; }
        ctx->x_owned = true;
    }
    if (nnd_h2d_parallel(ctx, (void *)ctx->x_orig, x, sizeof(float) * (size_t)ctx->n * ctx->d)) return 1;
    ctx->x_valid = true;
    return after_data(ctx);
}

extern "C" int32_t nnd_set_data_device(nnd_handle_t ctx, const float *x_dev) {
    ENTER(ctx, 0);
    if (!x_dev) { ctx->set_error("nnd_set_data_device: null data"); return 1; }
    if (ctx->x_owned) ctx->mem.free(&ctx->x_orig);
    ctx->x_orig = x_dev;
    ctx->x_owned = false;
    ctx->x_valid = true;
    return after_data(ctx);
}

// Rows of another type than float32 (and dot's rows of any type, which the reference normalises before anything else sees
// them, pynndescent_.py:1101-1102): converted on the device into the handle's own float32 copy -- finalize.hip, exact.hip and
// hubtree.hip read x_orig raw, so it stays float32 -- then prepared like any other point set.  float32 rows of the other
// metrics are borrowed as nnd_set_data_device borrows them.
extern "C" int32_t nnd_set_data_device_typed(nnd_handle_t ctx, const void *x_dev, int32_t dtype) {
    ENTER(ctx, 0);
    if (!x_dev) { ctx->set_error("nnd_set_data_device_typed: null data"); return 1; }
    if (dtype < NND_DTYPE_FLOAT32 || dtype > NND_DTYPE_FLOAT64) { ctx->set_error("nnd_set_data_device_typed: dtype %d is none of NND_DTYPE_*", (int)dtype); return 1; }
    const bool normalize = ctx->p.metric == NND_METRIC_ALT_DOT;
    if (dtype == NND_DTYPE_FLOAT32 && !normalize) return nnd_set_data_device(ctx, (const float *)x_dev);
    if (!(ctx->x_owned && ctx->x_orig)) {
        if (!ctx->mem.alloc(&ctx->x_orig, (size_t)ctx->n * ctx->d)) { ctx->set_error("nnd_set_data_device_typed: out of device memory for the handle's copy of the rows"); return 1; }
        ctx->x_owned = true;
    }
    if (nnd_launch_rows_f32(ctx->stream, x_dev, dtype, ctx->n, ctx->d, normalize, (float *)ctx->x_orig)) {
        (void)hipGetLastError();
        ctx->set_error("nnd_set_data_device_typed: conversion kernel launch failed");
        return 1;
    }
    ctx->x_valid = true;
    return after_data(ctx);
}

// Bit 0 / bit 1 of the prep kernel's flag word.  Bit 0: the point set handed to nnd_set_data_* held a NaN or an infinity; the
// reference rejects such input in check_array (pynndescent_.py:1054), and the host mirror raises the same error from this
// flag.  Bit 1: a hellinger point set held a negative entry.
static int data_flag(nnd_ctx *ctx, int bit, int32_t *out) {
    if (ctx->p.flags & NND_FLAG_NO_PREP) { *out = 0; return 0; }
    NND_HIP_CHECK(nnd_sync_spin(ctx));
    *out = (ctx->h_pin->data_flags & bit) != 0 ? 1 : 0;
    return 0;
}
extern "C" int32_t nnd_data_nonfinite(nnd_handle_t ctx, int32_t *out) {
    ENTER(ctx, NEED_DATA);
    return data_flag(ctx, 1, out);
}
extern "C" int32_t nnd_data_negative(nnd_handle_t ctx, int32_t *out) {
    ENTER(ctx, NEED_DATA);
    return data_flag(ctx, 2, out);
}

extern "C" int32_t nnd_make_forest(nnd_handle_t ctx) {
    ENTER(ctx, NEED_PREP | NEED_DATA);
    return flushed(ctx, stage_forest(ctx));
}

extern "C" int32_t nnd_leaf_array_shape(nnd_handle_t ctx, int64_t *n_leaves, int32_t *max_leaf_size) {
    ENTER(ctx, 0);
    if (!ctx->forest_built) {  // rp_trees.py:2921-2922: np.array([[-1]])
        *n_leaves = 1;
        *max_leaf_size = 1;
        return 0;
    }
    *n_leaves = ctx->n_leaves;
    *max_leaf_size = ctx->max_leaf;
    return 0;
}

extern "C" int32_t nnd_get_leaf_array(nnd_handle_t ctx, int32_t *out_host) {
    ENTER(ctx, 0);
    if (!ctx->forest_built) {
        out_host[0] = -1;
        return 0;
    }
    size_t total = (size_t)ctx->n_leaves * ctx->max_leaf;
    nnd_scratch tmp;
    int32_t *d = tmp.get<int32_t>(ctx, total);
    if (!d) return 1;
    if (nnd_launch_leaf_array(ctx, d)) return 1;
    NND_HIP_CHECK(hipMemcpyAsync(out_host, d, sizeof(int32_t) * total, hipMemcpyDeviceToHost, ctx->stream));
    NND_HIP_CHECK(nnd_sync_spin(ctx));
    return 0;
}

extern "C" int32_t nnd_reset_graph(nnd_handle_t ctx) {
    ENTER(ctx, NEED_GRAPH);
    return nnd_launch_reset_graph(ctx);
}

extern "C" int32_t nnd_init_from_leaves(nnd_handle_t ctx) {
    ENTER(ctx, NEED_GRAPH | NEED_DATA);
    return flushed(ctx, stage_leaf_init(ctx));
}

// init_rp_tree with the caller's leaf_array (the `leaf_array` argument of nn_descent, pynndescent_.py:324-337)
extern "C" int32_t nnd_init_from_leaf_array(nnd_handle_t ctx, const int32_t *leaf_array, int64_t n_leaves, int32_t max_leaf_size) {
    ENTER(ctx, NEED_GRAPH | NEED_DATA);
    if (!leaf_array || n_leaves < 0 || max_leaf_size < 1) { ctx->set_error("nnd_init_from_leaf_array: bad arguments"); return 1; }
    return flushed(ctx, timed(ctx, &ctx->stats.ms_leaf_init, false, [&] { return nnd_launch_leaf_init_array(ctx, leaf_array, n_leaves, max_leaf_size); }));
}

extern "C" int32_t nnd_init_random(nnd_handle_t ctx) {
    ENTER(ctx, NEED_GRAPH | NEED_DATA);
    return flushed(ctx, stage_random_init(ctx));
}

extern "C" int32_t nnd_init_from_graph(nnd_handle_t ctx, const int32_t *init_idx, const float *init_dist, int32_t width) {
    ENTER(ctx, NEED_GRAPH | NEED_DATA);
    if (!init_idx || width < 1 || width > NND_WIDE_K) { ctx->set_error("nnd_init_from_graph: width must be in 1..%d", NND_WIDE_K); return 1; }
    // the caller's arrays are the FULL (n, width) graph; the launcher takes the rows this handle OWNS (all of them, or a
    // shard's slice -- nnd_shard_handle exposes such handles): upload exactly those
    const int64_t rows = ctx->own_hi - ctx->own_lo;
    if (rows <= 0) return 0;
    const size_t cnt = (size_t)rows * width, off = (size_t)ctx->own_lo * width;
    nnd_scratch tmp;
    int32_t *di = tmp.get<int32_t>(ctx, cnt);
    float *dd = init_dist ? tmp.get<float>(ctx, cnt) : nullptr;
    if (!di || (init_dist && !dd)) return 1;
    NND_HIP_CHECK(hipMemcpyAsync(di, init_idx + off, sizeof(int32_t) * cnt, hipMemcpyHostToDevice, ctx->stream));
    if (init_dist) NND_HIP_CHECK(hipMemcpyAsync(dd, init_dist + off, sizeof(float) * cnt, hipMemcpyHostToDevice, ctx->stream));
    int rc = nnd_launch_init_from_graph(ctx, di, dd, width);
    (void)hipStreamSynchronize(ctx->stream);  // the scratch buffers are released on return
    return rc;
}

// init_from_neighbor_graph (pynndescent_.py:206-214), the warm start of NNDescent.update: the entries of an existing
// graph (alt-space distances given) are inserted with flag 0 ("old").  Call on a freshly reset graph.
extern "C" int32_t nnd_init_from_neighbor_graph(nnd_handle_t ctx, const int32_t *init_idx, const float *init_dist, int32_t width) {
    if (!ctx) return 1;
    if (!init_dist) { ENTER(ctx, 0); ctx->set_error("nnd_init_from_neighbor_graph: distances are required"); return 1; }
    if (nnd_init_from_graph(ctx, init_idx, init_dist, width)) return 1;
    if (nnd_launch_clear_new_flags(ctx)) return 1;
    ctx->all_new = false;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->set_error("nnd_init_from_neighbor_graph: synchronize failed"); return 1; }
    return 0;
}

// The two entries above for a graph that lives on the handle's device: the full (n, width) arrays are read in place on the
// handle's stream (a shard's handle reads its own rows of them).  Nothing is staged, so nothing has to be waited for before
// the return: the arrays must stay valid until the stream has passed the call.
extern "C" int32_t nnd_init_from_graph_device(nnd_handle_t ctx, const int32_t *init_idx_dev, const float *init_dist_dev, int32_t width) {
    ENTER(ctx, NEED_GRAPH | NEED_DATA);
    if (!init_idx_dev || width < 1 || width > NND_WIDE_K) { ctx->set_error("nnd_init_from_graph_device: width must be in 1..%d", NND_WIDE_K); return 1; }
    const size_t off = (size_t)ctx->own_lo * width;
    return nnd_launch_init_from_graph(ctx, init_idx_dev + off, init_dist_dev ? init_dist_dev + off : nullptr, width);
}
extern "C" int32_t nnd_init_from_neighbor_graph_device(nnd_handle_t ctx, const int32_t *init_idx_dev, const float *init_dist_dev, int32_t width) {
    if (!ctx) return 1;
    if (!init_dist_dev) { ENTER(ctx, 0); ctx->set_error("nnd_init_from_neighbor_graph_device: distances are required"); return 1; }
    if (nnd_init_from_graph_device(ctx, init_idx_dev, init_dist_dev, width)) return 1;
    if (nnd_launch_clear_new_flags(ctx)) return 1;
    ctx->all_new = false;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->set_error("nnd_init_from_neighbor_graph_device: synchronize failed"); return 1; }
    return 0;
}

extern "C" int32_t nnd_sample_candidates(nnd_handle_t ctx) {
    ENTER(ctx, NEED_GRAPH);
    return nnd_launch_sample(ctx);
}

// Sub-steps of an iteration (join a part of the vertices, merge, ...).  The reference applies the updates of every block of 16384
// vertices before it generates the next block's (pynndescent_.py:239-261): thresholds tighten INSIDE an iteration, and a row
// never has more than a block's worth of pushes pending.  One launch per iteration (rounds 1-5) leaves a row's 64 hashed
// proposal slots to take a whole iteration's proposals -- 23 per row in the first iteration of the 1 M bench set, more where
// convergence is slow -- and what collides is lost: measured on 200 000 iid Gaussian points x 32 (the reference algorithm
// reaches recall@10 0.613 there, tools/mid_regime_study.py): 0.6094 with one launch, 0.6108 / 0.6112 / 0.6125 with 2 / 4 / 12
// sub-steps (12 = the reference's blocking at that size).  When join_blocks is left to the library the sub-steps of an iteration
// follow the insertions per row the previous iteration made (halving is the slowest decay seen), so that late iterations --
// few updates, nothing to collide -- stay single launches.  An explicit join_blocks is taken as given.
int nnd_join_substeps(const nnd_ctx *ctx) {
    int nb = ctx->p.join_blocks;
    if (!ctx->jb_auto || ctx->k > 64) return nb;  // (wide rows: nnd_auto_join_blocks has cut their iterations already)
    const double rows = (double)(ctx->own_hi - ctx->own_lo);
    const double per_row = (ctx->iter == 0 || ctx->last_updates < 0 || rows <= 0) ? (double)ctx->jb_first : (double)ctx->last_updates / rows;
    int m = 1;
    while (m < ctx->jb_max && (double)(m * ctx->jb_div) < per_row) m <<= 1;
    return nb * m;
}

// what the join counted, into the stats of the current iteration (after nnd_read_counters)
static void record_join_counters(nnd_ctx *ctx) {
    const int it = ctx->iter;
    if (it >= 64) return;
    ctx->stats.join_pairs[it] = ctx->h_counters[CNT_PAIRS];
    ctx->stats.join_rows[it] = ctx->h_counters[CNT_ROWS];
    ctx->stats.join_active[it] = ctx->h_counters[CNT_ACTIVE];
    ctx->stats.proposals[it] = ctx->h_counters[CNT_PROPOSALS];
}

// one iteration of nn_descent_internal (pynndescent_.py:296-320)
static int descent_iter(nnd_ctx *ctx, int64_t *c_out) {
    const int it = ctx->iter;
    if (stage_sample(ctx)) return 1;
    if (nnd_zero_counters(ctx)) return 1;
    // The reference joins vertices in blocks of 16384 and applies updates between blocks
    // (pynndescent_.py:239-261) so thresholds tighten inside an iteration; join_blocks sub-steps do the same.
    const int nb = nnd_join_substeps(ctx);
    if (it < 64) {
        ctx->stats.ms_join[it] = ctx->stats.ms_merge[it] = 0.f;
        ctx->stats.join_substeps[it] = nb;
    }
    for (int b = 0; b < nb; b++) {
        const int64_t span = ctx->own_hi - ctx->own_lo;
        if (stage_join(ctx, ctx->own_lo + span * b / nb, ctx->own_lo + span * (b + 1) / nb, true)) return 1;
        if (stage_merge(ctx)) return 1;
    }
    if (nnd_read_counters(ctx)) return 1;  // the host needs c here anyway: the timers are read at no extra wait
    t_flush(ctx);
    record_join_counters(ctx);
    if (it < 64) {
        ctx->stats.updates[it] = ctx->h_counters[CNT_ACCEPT];
        ctx->stats.join_mfma[it] = ctx->h_counters[CNT_MFMA];
    }
    *c_out = ctx->h_counters[CNT_ACCEPT];
    ctx->last_updates = ctx->h_counters[CNT_ACCEPT];
    ctx->iter++;
    ctx->stats.n_iters_run = ctx->iter;
    return 0;
}

extern "C" int32_t nnd_descent_iter(nnd_handle_t ctx, int64_t *c_out) {
    ENTER(ctx, NEED_GRAPH | NEED_DATA);
    int64_t c = 0;
    if (descent_iter(ctx, &c)) return 1;
    if (c_out) *c_out = c;
    return 0;
}

// (ev0 / ev1 are the handle's: nothing else has them in flight during a descent -- the pruning pass and the sharded build
// record and read them inside one call of their own)
static int descent_loop(nnd_ctx *ctx) {
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    int rc = 0;
    for (int it = 0; it < ctx->p.n_iters; it++) {
        int64_t c = 0;
        if ((rc = descent_iter(ctx, &c))) break;
        if ((double)c <= (double)ctx->p.delta * ctx->k * (double)ctx->n) break;  // pynndescent_.py:317
    }
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    (void)hipEventSynchronize(ctx->ev1);
    (void)hipEventElapsedTime(&ctx->stats.ms_descent, ctx->ev0, ctx->ev1);
    return rc;
}

extern "C" int32_t nnd_descent(nnd_handle_t ctx) {
    ENTER(ctx, NEED_GRAPH | NEED_DATA);
    return descent_loop(ctx);
}

extern "C" int32_t nnd_finalize_device(nnd_handle_t ctx, int32_t *out_idx_dev, float *out_dist_dev) {
    ENTER(ctx, NEED_GRAPH | NEED_DATA);
    return flushed(ctx, stage_finalize(ctx, out_idx_dev, out_dist_dev));
}

// grow-only device buffers for the finished graph of the host-buffer entry points (no hipMalloc / hipFree per call)
static int out_buffers(nnd_ctx *ctx, size_t cnt) {
    if (!ctx->mem.grow2(&ctx->out_idx, &ctx->out_dist, &ctx->out_cap, cnt, cnt)) { ctx->set_error("out of device memory for the finished graph (%zu entries)", cnt); return 1; }
    return 0;
}

extern "C" int32_t nnd_finalize_host(nnd_handle_t ctx, int32_t *out_idx, float *out_dist) {
    ENTER(ctx, NEED_GRAPH | NEED_DATA);
    size_t cnt = (size_t)(ctx->own_hi - ctx->own_lo) * ctx->k;  // owned rows only
    if (out_buffers(ctx, cnt)) return 1;
    if (nnd_finalize_device(ctx, ctx->out_idx, ctx->out_dist)) return 1;  // (ends with a flush: the stream has drained)
    if (nnd_d2h_parallel(ctx, out_idx, ctx->out_idx, sizeof(int32_t) * cnt, 4)) return 1;
    if (nnd_d2h_parallel(ctx, out_dist, ctx->out_dist, sizeof(float) * cnt, 4)) return 1;
    return 0;
}

// nn_descent (pynndescent_.py:323-366) on a resident point set: EMPTY_GRAPH branch
extern "C" int32_t nnd_build_device(nnd_handle_t ctx, int32_t *out_idx_dev, float *out_dist_dev) {
    ENTER(ctx, NEED_GRAPH | NEED_DATA);
    if (nnd_launch_reset_graph(ctx)) return 1;
    if (ctx->p.n_trees > 0 && (stage_forest(ctx) || stage_leaf_init(ctx))) return 1;
    if (stage_random_init(ctx)) return 1;
    if (descent_loop(ctx)) return 1;
    return flushed(ctx, stage_finalize(ctx, out_idx_dev, out_dist_dev));
}

extern "C" int32_t nnd_build(const nnd_params *params, const float *x, const int32_t *init_idx, const float *init_dist,
                             int32_t init_width, int32_t *out_idx, float *out_dist, nnd_stats *stats, char *err,
                             int32_t errlen) {
    auto fail = [&](const char *msg) {
        if (err && errlen > 0) { strncpy(err, msg, (size_t)errlen - 1); err[errlen - 1] = 0; }
        return 1;
    };
    nnd_handle_t h = nullptr;
    nnd_params p = *params;
    if (init_idx) p.n_trees = 0;  // pynndescent_.py:1059-1062: an init graph disables the forest
    if (nnd_create(&h, &p)) return fail(nnd_last_global_error());
    int rc = nnd_set_data_host(h, x);
    if (!rc) {
        if (init_idx) {
            rc = nnd_init_from_graph(h, init_idx, init_dist, init_width);
            if (!rc) rc = nnd_descent(h);
            if (!rc) rc = nnd_finalize_host(h, out_idx, out_dist);
        } else {
            if (!rc) rc = out_buffers(h, (size_t)h->n * h->k);
            if (!rc) rc = nnd_build_device(h, h->out_idx, h->out_dist);
            if (!rc) rc = nnd_d2h_parallel(h, out_idx, h->out_idx, sizeof(int32_t) * (size_t)h->n * h->k, 4);
            if (!rc) rc = nnd_d2h_parallel(h, out_dist, h->out_dist, sizeof(float) * (size_t)h->n * h->k, 4);
        }
    }
    if (stats) *stats = h->stats;
    std::string msg = h->err;
    nnd_destroy(h);
    if (rc) return fail(msg.c_str());
    return 0;
}

extern "C" int32_t nnd_get_stats(nnd_handle_t ctx, nnd_stats *out) {
    if (!ctx || !out) { nnd_set_global_error("null argument"); return 1; }
    *out = ctx->stats;
    return 0;
}

extern "C" int32_t nnd_synchronize(nnd_handle_t ctx) {
    ENTER(ctx, 0);
    NND_HIP_CHECK(nnd_sync_spin(ctx));
    return 0;
}

// ---- introspection for the parity tests ----
extern "C" int32_t nnd_get_graph(nnd_handle_t ctx, int32_t *idx, float *dist, uint8_t *flags) {
    ENTER(ctx, NEED_GRAPH);
    size_t cnt = (size_t)ctx->n * ctx->ks;
    std::vector<uint32_t> he(cnt);
    std::vector<float> hd(cnt);
    NND_HIP_CHECK(hipMemcpyAsync(he.data(), ctx->knn_e, sizeof(uint32_t) * cnt, hipMemcpyDeviceToHost, ctx->stream));
    NND_HIP_CHECK(hipMemcpyAsync(hd.data(), ctx->knn_d, sizeof(float) * cnt, hipMemcpyDeviceToHost, ctx->stream));
    NND_HIP_CHECK(nnd_sync_spin(ctx));
    for (int64_t v = 0; v < ctx->n; v++)
        for (int j = 0; j < ctx->k; j++) {
            uint32_t e = he[v * ctx->ks + j];
            size_t o = (size_t)v * ctx->k + j;
            if (idx) idx[o] = e == NND_EMPTY_E ? -1 : (int32_t)(e & NND_IDX_MASK);
            if (dist) dist[o] = hd[v * ctx->ks + j];
            if (flags) flags[o] = e == NND_EMPTY_E ? 0 : (uint8_t)(e >> 31);
        }
    return 0;
}

extern "C" int32_t nnd_get_candidates(nnd_handle_t ctx, int32_t *new_idx, int32_t *old_idx) {
    ENTER(ctx, NEED_GRAPH);
    size_t cnt = (size_t)ctx->n * 2 * ctx->mcp;
    std::vector<int32_t> hc(cnt);
    NND_HIP_CHECK(hipMemcpyAsync(hc.data(), ctx->cand, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, ctx->stream));
    NND_HIP_CHECK(nnd_sync_spin(ctx));
    for (int64_t v = 0; v < ctx->n; v++)
        for (int j = 0; j < ctx->mc; j++) {
            if (new_idx) new_idx[v * ctx->mc + j] = hc[v * 2 * ctx->mcp + j];
            if (old_idx) old_idx[v * ctx->mc + j] = hc[v * 2 * ctx->mcp + ctx->mcp + j];
        }
    return 0;
}

extern "C" int32_t nnd_pairwise_gram(nnd_handle_t ctx, const int32_t *rows_a, int32_t na, const int32_t *rows_b,
                                     int32_t nb, float *out) {
    ENTER(ctx, NEED_PREP | NEED_DATA);
    nnd_scratch tmp;
    int32_t *da = tmp.get<int32_t>(ctx, (size_t)na), *db = tmp.get<int32_t>(ctx, (size_t)nb);
    float *dout = tmp.get<float>(ctx, (size_t)na * nb);
    if (!da || !db || !dout) return 1;
    NND_HIP_CHECK(hipMemcpyAsync(da, rows_a, sizeof(int32_t) * na, hipMemcpyHostToDevice, ctx->stream));
    NND_HIP_CHECK(hipMemcpyAsync(db, rows_b, sizeof(int32_t) * nb, hipMemcpyHostToDevice, ctx->stream));
    if (nnd_launch_pairwise(ctx, da, na, db, nb, dout)) return 1;
    NND_HIP_CHECK(hipMemcpyAsync(out, dout, sizeof(float) * (size_t)na * nb, hipMemcpyDeviceToHost, ctx->stream));
    NND_HIP_CHECK(nnd_sync_spin(ctx));
    return 0;
}

// exact k nearest neighbours (exact.hip): rows of the point set / external queries
// (after the entry's NEED_PREP)
static int exact_checks(nnd_ctx *ctx, const char *who, int64_t nq, int32_t k, const void *out_idx, const void *out_dist) {
    if (ctx->p.metric == NND_METRIC_PROXY_INNER_PRODUCT) { ctx->set_error("%s: the exact search has no certificate for the proxy inner product (metric 6)", who); return 1; }
    if (need(ctx, NEED_DATA, who)) return 1;
    if (k < 1 || k > NND_WIDE_K || (int64_t)k > ctx->n) { ctx->set_error("%s: k = %d is outside 1 .. min(n, %d) (n = %lld)", who, (int)k, NND_WIDE_K, (long long)ctx->n); return 1; }
    if (nq < 0 || (nq > 0 && (!out_idx || !out_dist))) { ctx->set_error("%s: null output or negative row count", who); return 1; }
    return 0;
}
extern "C" int32_t nnd_exact_knn_rows(nnd_handle_t ctx, const int64_t *rows, int64_t n_rows, int32_t k, int32_t *out_idx, float *out_dist, nnd_exact_stats *st) {
    ENTER(ctx, NEED_PREP);
    if (!rows) n_rows = ctx->n;
    if (exact_checks(ctx, "nnd_exact_knn_rows", n_rows, k, out_idx, out_dist)) return 1;
    return nnd_exact_knn_impl(ctx, rows, nullptr, n_rows, k, out_idx, out_dist, st);
}
extern "C" int32_t nnd_exact_knn_queries(nnd_handle_t ctx, const float *q, int64_t n_q, int32_t k, int32_t *out_idx, float *out_dist, nnd_exact_stats *st) {
    ENTER(ctx, NEED_PREP);
    if (exact_checks(ctx, "nnd_exact_knn_queries", n_q, k, out_idx, out_dist)) return 1;
    if (!q && n_q > 0) { ctx->set_error("nnd_exact_knn_queries: null queries"); return 1; }
    if (!q) { if (st) *st = nnd_exact_stats{}; return 0; }
    return nnd_exact_knn_impl(ctx, nullptr, q, n_q, k, out_idx, out_dist, st);
}
// ... with the caller's arrays on the handle's device (exact.hip: the batch copies become device to device)
extern "C" int32_t nnd_exact_knn_rows_device(nnd_handle_t ctx, const int32_t *rows_dev, int64_t n_rows, int32_t k, int32_t *out_idx_dev, float *out_dist_dev,
                                             nnd_exact_stats *st) {
    ENTER(ctx, NEED_PREP);
    if (!rows_dev) n_rows = ctx->n;
    if (exact_checks(ctx, "nnd_exact_knn_rows_device", n_rows, k, out_idx_dev, out_dist_dev)) return 1;
    const nnd_exact_dev dev{rows_dev, nullptr, NND_DTYPE_FLOAT32};
    return nnd_exact_knn_impl(ctx, nullptr, nullptr, n_rows, k, out_idx_dev, out_dist_dev, st, &dev);
}
extern "C" int32_t nnd_exact_knn_queries_device(nnd_handle_t ctx, const void *q_dev, int32_t dtype, int64_t n_q, int32_t k, int32_t *out_idx_dev,
                                                float *out_dist_dev, nnd_exact_stats *st) {
    ENTER(ctx, NEED_PREP);
    if (exact_checks(ctx, "nnd_exact_knn_queries_device", n_q, k, out_idx_dev, out_dist_dev)) return 1;
    if (dtype < NND_DTYPE_FLOAT32 || dtype > NND_DTYPE_FLOAT64) { ctx->set_error("nnd_exact_knn_queries_device: dtype %d is none of NND_DTYPE_*", (int)dtype); return 1; }
    if (!q_dev && n_q > 0) { ctx->set_error("nnd_exact_knn_queries_device: null queries"); return 1; }
    if (!q_dev) { if (st) *st = nnd_exact_stats{}; return 0; }
    const nnd_exact_dev dev{nullptr, q_dev, dtype};
    return nnd_exact_knn_impl(ctx, nullptr, nullptr, n_q, k, out_idx_dev, out_dist_dev, st, &dev);
}
// ... among the rows a predicate allows (exact.hip, the masked instances): n tag words, one mask word per query row
static int exact_tag_checks(nnd_ctx *ctx, const char *who, const void *tags, const void *masks, int64_t nq) {
    if (!tags || (nq > 0 && !masks)) { ctx->set_error("%s: tags or masks missing", who); return 1; }
    return 0;
}
// the host forms' words go up into buffers of the call (released behind the search's last synchronise)
static int exact_upload_tags(nnd_ctx *ctx, nnd_scratch &tmp, const uint64_t *tags, const uint64_t *masks, int64_t nq, nnd_exact_tags *tg) {
    uint64_t *dt = tmp.get<uint64_t>(ctx, (size_t)ctx->n), *dm = tmp.get<uint64_t>(ctx, (size_t)nq);
    if (!dt || !dm) return 1;
    NND_HIP_CHECK(hipMemcpyAsync(dt, tags, sizeof(uint64_t) * (size_t)ctx->n, hipMemcpyHostToDevice, ctx->stream));
    if (nq > 0) NND_HIP_CHECK(hipMemcpyAsync(dm, masks, sizeof(uint64_t) * (size_t)nq, hipMemcpyHostToDevice, ctx->stream));
    *tg = nnd_exact_tags{dt, dm};
    return 0;
}
extern "C" int32_t nnd_exact_knn_rows_tagged(nnd_handle_t ctx, const int64_t *rows, int64_t n_rows, int32_t k, const uint64_t *tags, const uint64_t *masks,
                                             int32_t *out_idx, float *out_dist, nnd_exact_stats *st) {
    ENTER(ctx, NEED_PREP);
    if (!rows) n_rows = ctx->n;
    if (exact_checks(ctx, "nnd_exact_knn_rows_tagged", n_rows, k, out_idx, out_dist)) return 1;
    if (exact_tag_checks(ctx, "nnd_exact_knn_rows_tagged", tags, masks, n_rows)) return 1;
    nnd_scratch tmp;
    nnd_exact_tags tg;
    int rc = exact_upload_tags(ctx, tmp, tags, masks, n_rows, &tg);
    if (!rc) rc = nnd_exact_knn_impl(ctx, rows, nullptr, n_rows, k, out_idx, out_dist, st, nullptr, &tg);
    if (rc) (void)nnd_sync_spin(ctx);  // nothing queued still reads tmp
    return rc;
}
extern "C" int32_t nnd_exact_knn_queries_tagged(nnd_handle_t ctx, const float *q, int64_t n_q, int32_t k, const uint64_t *tags, const uint64_t *masks,
                                                int32_t *out_idx, float *out_dist, nnd_exact_stats *st) {
    ENTER(ctx, NEED_PREP);
    if (exact_checks(ctx, "nnd_exact_knn_queries_tagged", n_q, k, out_idx, out_dist)) return 1;
    if (!q && n_q > 0) { ctx->set_error("nnd_exact_knn_queries_tagged: null queries"); return 1; }
    if (!q) { if (st) *st = nnd_exact_stats{}; return 0; }
    if (exact_tag_checks(ctx, "nnd_exact_knn_queries_tagged", tags, masks, n_q)) return 1;
    nnd_scratch tmp;
    nnd_exact_tags tg;
    int rc = exact_upload_tags(ctx, tmp, tags, masks, n_q, &tg);
    if (!rc) rc = nnd_exact_knn_impl(ctx, nullptr, q, n_q, k, out_idx, out_dist, st, nullptr, &tg);
    if (rc) (void)nnd_sync_spin(ctx);
    return rc;
}
extern "C" int32_t nnd_exact_knn_rows_tagged_device(nnd_handle_t ctx, const int32_t *rows_dev, int64_t n_rows, int32_t k, const uint64_t *tags_dev,
                                                    const uint64_t *masks_dev, int32_t *out_idx_dev, float *out_dist_dev, nnd_exact_stats *st) {
    ENTER(ctx, NEED_PREP);
    if (!rows_dev) n_rows = ctx->n;
    if (exact_checks(ctx, "nnd_exact_knn_rows_tagged_device", n_rows, k, out_idx_dev, out_dist_dev)) return 1;
    if (exact_tag_checks(ctx, "nnd_exact_knn_rows_tagged_device", tags_dev, masks_dev, n_rows)) return 1;
    const nnd_exact_dev dev{rows_dev, nullptr, NND_DTYPE_FLOAT32};
    const nnd_exact_tags tg{tags_dev, masks_dev};
    return nnd_exact_knn_impl(ctx, nullptr, nullptr, n_rows, k, out_idx_dev, out_dist_dev, st, &dev, &tg);
}
extern "C" int32_t nnd_exact_knn_queries_tagged_device(nnd_handle_t ctx, const void *q_dev, int32_t dtype, int64_t n_q, int32_t k, const uint64_t *tags_dev,
                                                       const uint64_t *masks_dev, int32_t *out_idx_dev, float *out_dist_dev, nnd_exact_stats *st) {
    ENTER(ctx, NEED_PREP);
    if (exact_checks(ctx, "nnd_exact_knn_queries_tagged_device", n_q, k, out_idx_dev, out_dist_dev)) return 1;
    if (dtype < NND_DTYPE_FLOAT32 || dtype > NND_DTYPE_FLOAT64) { ctx->set_error("nnd_exact_knn_queries_tagged_device: dtype %d is none of NND_DTYPE_*", (int)dtype); return 1; }
    if (!q_dev && n_q > 0) { ctx->set_error("nnd_exact_knn_queries_tagged_device: null queries"); return 1; }
    if (!q_dev) { if (st) *st = nnd_exact_stats{}; return 0; }
    if (exact_tag_checks(ctx, "nnd_exact_knn_queries_tagged_device", tags_dev, masks_dev, n_q)) return 1;
    const nnd_exact_dev dev{nullptr, q_dev, dtype};
    const nnd_exact_tags tg{tags_dev, masks_dev};
    return nnd_exact_knn_impl(ctx, nullptr, nullptr, n_q, k, out_idx_dev, out_dist_dev, st, &dev, &tg);
}
extern "C" int32_t nnd_exact_slice_count(nnd_handle_t ctx, int64_t n_rows) {
    if (!ctx) return 0;
    return nnd_exact_slices_for(ctx->n, n_rows);  // (of the first batch: exact.hip takes at most EX_BATCH query rows per pass)
}

extern "C" int32_t nnd_descent_sample(nnd_handle_t ctx) {
    ENTER(ctx, NEED_GRAPH);
    return stage_sample(ctx);
}
extern "C" int32_t nnd_descent_join(nnd_handle_t ctx) {
    ENTER(ctx, NEED_GRAPH);
    if (nnd_zero_counters(ctx)) return 1;
    if (stage_join(ctx, ctx->own_lo, ctx->own_hi, false)) return 1;
    if (nnd_read_counters(ctx)) return 1;  // (a test / profiling entry point: the join's counters are in the stats when it returns)
    t_flush(ctx);
    record_join_counters(ctx);
    return 0;
}

// ---- search-graph pruning pass (BASELINE config 5); host glue: pynndescent_amd/search_graph.py ----
// Host-buffer entry points: the graph of this stage is handed over and taken back as numpy arrays by the
// reference as well (its glue between the numba kernels is scipy on the host, pynndescent_.py:1509-1611).
static nnd_prune_opts prune_defaults(const nnd_prune_opts *o) {
    nnd_prune_opts d{};
    d.prune_probability = 1.0f;
    d.alpha = 1.0f;
    d.max_degree = 1;
    return o ? *o : d;
}

extern "C" int32_t nnd_diversify_host(nnd_handle_t ctx, int32_t *idx /* (n,k) in/out */, float *dist /* (n,k) in/out */,
                                      const nnd_prune_opts *opts, const int32_t *degree /* (n), degree-aware only */) {
    ENTER(ctx, NEED_PREP | NEED_DATA);
    const nnd_prune_opts o = prune_defaults(opts);
    if (o.degree_aware && (!degree || o.max_degree < 1)) { ctx->set_error("nnd_diversify_host: the degree-aware method needs degrees and max_degree >= 1"); return 1; }
    size_t cnt = (size_t)ctx->n * ctx->k;
    nnd_scratch tmp;
    int32_t *di = tmp.get<int32_t>(ctx, cnt);
    float *dd = tmp.get<float>(ctx, cnt);
    int32_t *dg = o.degree_aware ? tmp.get<int32_t>(ctx, (size_t)ctx->n) : nullptr;
    if (!di || !dd || (o.degree_aware && !dg)) return 1;
    NND_HIP_CHECK(hipMemcpyAsync(di, idx, sizeof(int32_t) * cnt, hipMemcpyHostToDevice, ctx->stream));
    NND_HIP_CHECK(hipMemcpyAsync(dd, dist, sizeof(float) * cnt, hipMemcpyHostToDevice, ctx->stream));
    if (dg) NND_HIP_CHECK(hipMemcpyAsync(dg, degree, sizeof(int32_t) * (size_t)ctx->n, hipMemcpyHostToDevice, ctx->stream));
    if (nnd_launch_diversify_rows(ctx, di, dd, &o, dg)) return 1;
    NND_HIP_CHECK(hipMemcpyAsync(idx, di, sizeof(int32_t) * cnt, hipMemcpyDeviceToHost, ctx->stream));
    NND_HIP_CHECK(hipMemcpyAsync(dist, dd, sizeof(float) * cnt, hipMemcpyDeviceToHost, ctx->stream));
    NND_HIP_CHECK(nnd_sync_spin(ctx));
    return 0;
}

extern "C" int32_t nnd_diversify_csr_host(nnd_handle_t ctx, const int32_t *indptr /* n+1 */, const int32_t *indices,
                                          float *data /* nnz in/out */, int64_t nnz, const nnd_prune_opts *opts,
                                          const int32_t *degree /* (n), degree-aware only */) {
    ENTER(ctx, NEED_PREP | NEED_DATA);
    const nnd_prune_opts o = prune_defaults(opts);
    if (o.degree_aware && !degree) { ctx->set_error("nnd_diversify_csr_host: the degree-aware method needs degrees"); return 1; }
    nnd_scratch tmp;
    int32_t *dp = tmp.get<int32_t>(ctx, (size_t)(ctx->n + 1)), *di = tmp.get<int32_t>(ctx, (size_t)nnz);
    float *dd = tmp.get<float>(ctx, (size_t)nnz);
    int *flag = tmp.get<int>(ctx, 1);
    int32_t *dg = o.degree_aware ? tmp.get<int32_t>(ctx, (size_t)ctx->n) : nullptr;
    if (!dp || !di || !dd || !flag || (o.degree_aware && !dg)) return 1;
    NND_HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int), ctx->stream));
    NND_HIP_CHECK(hipMemcpyAsync(dp, indptr, sizeof(int32_t) * (size_t)(ctx->n + 1), hipMemcpyHostToDevice, ctx->stream));
    NND_HIP_CHECK(hipMemcpyAsync(di, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
    NND_HIP_CHECK(hipMemcpyAsync(dd, data, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
    if (dg) NND_HIP_CHECK(hipMemcpyAsync(dg, degree, sizeof(int32_t) * (size_t)ctx->n, hipMemcpyHostToDevice, ctx->stream));
    if (nnd_launch_diversify_csr(ctx, dp, di, dd, flag, &o, dg)) return 1;
    int too_long = 0;
    NND_HIP_CHECK(hipMemcpyAsync(data, dd, sizeof(float) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
    NND_HIP_CHECK(hipMemcpyAsync(&too_long, flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    NND_HIP_CHECK(nnd_sync_spin(ctx));
    if (too_long) {
        ctx->set_error("nnd_diversify_csr_host: %d rows are longer than 64 entries (rows of a diversified k-NN graph have <= k <= 64)", too_long);
        return 1;
    }
    return 0;
}

extern "C" int32_t nnd_degree_prune_host(nnd_handle_t ctx, const int32_t *indptr /* n+1 */, float *data /* nnz in/out */,
                                         int64_t nnz, int32_t max_degree) {
    ENTER(ctx, 0);
    nnd_scratch tmp;
    int32_t *dp = tmp.get<int32_t>(ctx, (size_t)(ctx->n + 1));
    float *dd = tmp.get<float>(ctx, (size_t)nnz);
    if (!dp || !dd) return 1;
    NND_HIP_CHECK(hipMemcpyAsync(dp, indptr, sizeof(int32_t) * (size_t)(ctx->n + 1), hipMemcpyHostToDevice, ctx->stream));
    NND_HIP_CHECK(hipMemcpyAsync(dd, data, sizeof(float) * (size_t)nnz, hipMemcpyHostToDevice, ctx->stream));
    if (nnd_launch_degree_prune(ctx, dp, dd, max_degree)) return 1;
    NND_HIP_CHECK(hipMemcpyAsync(data, dd, sizeof(float) * (size_t)nnz, hipMemcpyDeviceToHost, ctx->stream));
    NND_HIP_CHECK(nnd_sync_spin(ctx));
    return 0;
}

// the whole pass on the device (searchgraph.hip)
extern "C" int32_t nnd_search_graph(nnd_handle_t ctx, const int32_t *idx, const float *dist, int32_t on_device, int32_t n_neighbors,
                                    float pruning_degree_multiplier, float diversify_prob, int32_t degree_aware, float degree_prune_aggressiveness,
                                    uint32_t seed, int32_t *fwd_rows_host, float *fwd_dist_host, nnd_search_graph_stats *stats) {
    ENTER(ctx, NEED_PREP | NEED_DATA);
    if (!idx || !dist || n_neighbors < 1) { ctx->set_error("nnd_search_graph: bad arguments"); return 1; }
    return nnd_search_graph_impl(ctx, idx, dist, on_device != 0, n_neighbors, pruning_degree_multiplier, diversify_prob, degree_aware != 0,
                                 degree_prune_aggressiveness, seed, fwd_rows_host, fwd_dist_host, stats);
}
extern "C" int32_t nnd_search_graph_fetch(nnd_handle_t ctx, int32_t *indptr_host, int32_t *indices_host) {
    ENTER(ctx, 0);
    if (!indptr_host) { ctx->set_error("nnd_search_graph_fetch: null argument"); return 1; }
    return nnd_search_graph_fetch_impl(ctx, indptr_host, indices_host);
}
extern "C" int32_t nnd_search_graph_device(nnd_handle_t ctx, const int32_t **indptr_dev, const int32_t **indices_dev, int64_t *nnz) {
    ENTER(ctx, 0);
    if (!indptr_dev || !indices_dev || !nnz) { ctx->set_error("nnd_search_graph_device: null argument"); return 1; }
    return nnd_search_graph_device_impl(ctx, indptr_dev, indices_dev, nnz);
}

// the hub tree splits the rows AS GIVEN, angularly where the reference's search tree is angular (pynndescent_.py:1075-1086): the
// unit-row metrics, and jaccard / dice of the boolean family
static bool hub_tree_angular(int metric) { return nnd_metric_unit(metric) || metric == NND_METRIC_JACCARD || metric == NND_METRIC_DICE; }
// ---- hub search tree of NNDescent.prepare() (reference rp_trees.py:714-1312, 2926-3049; host glue: search_tree.py) ----
extern "C" int32_t nnd_hub_tree_build(nnd_handle_t ctx, const int32_t *rank_order /* host (n): ids by (-in-degree, id) */,
                                      int32_t leaf_size, int32_t max_depth, int64_t *n_nodes_out) {
    ENTER(ctx, NEED_DATA);
    if (!rank_order) { ctx->set_error("nnd_hub_tree_build: null rank order"); return 1; }
    if (nnd_hub_tree_build_impl(ctx, rank_order, false, leaf_size, max_depth, hub_tree_angular(ctx->p.metric))) return 1;
    if (n_nodes_out) *n_nodes_out = nnd_hub_tree_nodes(ctx);
    return 0;
}
extern "C" int32_t nnd_hub_tree_build_device(nnd_handle_t ctx, const int32_t *rank_order_dev /* device (n) */, int32_t leaf_size, int32_t max_depth,
                                             int64_t *n_nodes_out) {
    ENTER(ctx, NEED_DATA);
    if (!rank_order_dev) { ctx->set_error("nnd_hub_tree_build_device: null rank order"); return 1; }
    if (nnd_hub_tree_build_impl(ctx, rank_order_dev, true, leaf_size, max_depth, hub_tree_angular(ctx->p.metric))) return 1;
    if (n_nodes_out) *n_nodes_out = nnd_hub_tree_nodes(ctx);
    return 0;
}
extern "C" int32_t nnd_hub_tree_fetch(nnd_handle_t ctx, float *hyperplanes, float *offsets, int32_t *children, int32_t *indices,
                                      int32_t *max_leaf_size) {
    ENTER(ctx, 0);
    return nnd_hub_tree_fetch_impl(ctx, hyperplanes, offsets, children, indices, max_leaf_size);
}
