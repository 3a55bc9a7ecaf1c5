// handle.hip -- lifetime of a builder handle: creation by its plan (plan.h), the allocation of its tables, parking and
// tear-down, the lifecycle lock, the handle's stream, and the error text of the calls that have no handle.  No kernel here.
#include <string.h>

#include <mutex>

#include "common.h"
#include "plan.h"
#include "state.h"

static_assert(NND_PLAN_MAX_K == NND_WIDE_K, "plan.h checks n_neighbors against the kernels' widest row");

static thread_local char g_err[512] = {0};

static void gerr(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

void nnd_set_global_error(const char *msg) { gerr("%s", msg); }  // the entries that have no handle (capi.hip, transfer.hip, devarray.hip)
extern "C" const char *nnd_last_global_error(void) { return g_err; }
extern "C" const char *nnd_last_error(nnd_handle_t h) { return h ? h->err : g_err; }

static void nnd_release_parked();
template <typename T>
static int dalloc(nnd_ctx *ctx, T **p, size_t count) {
    if (!ctx->mem.alloc(p, count)) {
        nnd_release_parked();  // a parked handle (nnd_destroy) may hold what is missing
        if (!ctx->mem.alloc(p, count)) { ctx->set_error("out of device memory: allocation of %zu bytes failed", sizeof(T) * (count ? count : 1)); return 1; }
    }
    // debugging aid: fresh hipMalloc pages are usually zero, recycled ones are not -- NND_POISON=<byte> fills every buffer with
    // that byte (try 165: negative ints / tiny floats, and 1 or 127: positive ints) before the build initialises it
    static const int poison = [] { const char *e = nnd_knob("NND_POISON"); return e ? atoi(e) : 0; }();  // the fill byte
    // (on the handle's own stream, like the memsets of allocate_tables below: a hipMemset on the NULL stream queues behind
    // whatever the caller's framework still has in flight there and would land in the middle of the build)
    if (poison) {
        NND_HIP_CHECK(hipMemsetAsync(*p, poison & 0xFF, sizeof(T) * (count ? count : 1), ctx->stream));
        NND_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

std::recursive_mutex &nnd_lifecycle_mutex() {
#ifdef NND_TEST_NO_LIFECYCLE_LOCK  // heap-check builds only (tools/gpu_asan.sh nolock): every thread gets its own mutex
    static thread_local std::recursive_mutex m;
#else
    static std::recursive_mutex m;
#endif
    return m;
}

// Everything the handle holds.  Device memory has one owner (ctx->mem, devmem.h): whichever translation unit allocated a table,
// it goes here; what is listed below is what is not device memory.
static void free_all(nnd_ctx *ctx) {
    ctx->mem.release_all();
    if (ctx->h_pin) { (void)hipHostFree(ctx->h_pin); ctx->h_pin = nullptr; }
    if (ctx->h_tree_begin) { (void)hipHostFree(ctx->h_tree_begin); ctx->h_tree_begin = nullptr; }
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev_spin) (void)hipEventDestroy(ctx->ev_spin);
    for (hipEvent_t e : ctx->tev) if (e) (void)hipEventDestroy(e);
    ctx->tev.clear();
    nnd_hub_tree_free(ctx);
    nnd_search_graph_free(ctx);
    if (ctx->stream && ctx->stream_owned) (void)hipStreamDestroy(ctx->stream);
}

// Arm a handle for one build -- a new one (nnd_create_impl) or a parked one (take_parked): everything that is per build is
// derived from the parameters or reset HERE, and nowhere else.  What is not touched survives parking on purpose: the grow-only
// buffers and their capacities, rv_off, pbuf_clean / rbuf_clean, rv_pos_gen, forest_gen, cur, flag_seq.
static void arm_for_build(nnd_ctx *ctx, const nnd_params *p, const nnd_join_plan &pl) {
    ctx->p = *p;
    ctx->p.join_blocks = pl.join_blocks;  // (the effective count: nnd_join_substeps, shard.hip)
    ctx->jb_auto = pl.jb_auto, ctx->jb_max = pl.jb_max, ctx->jb_div = pl.jb_div, ctx->jb_first = pl.jb_first;
    ctx->seed = nnd_seed_of(p->rng_state);
    ctx->tree_seed = nnd_seed_of(p->tree_rng);
    ctx->iter = 0;
    ctx->stats = nnd_stats{};
    ctx->err[0] = 0;
    ctx->forest_built = false;
    ctx->h_leaf_valid = false;
    ctx->n_leaves = 0;
    ctx->max_leaf = 0;
    ctx->own_order = nullptr;
    ctx->lists_replicated = false;
    ctx->x_valid = false;
    ctx->tlog.clear();
    ctx->tev_used = 0;
    nnd_hub_tree_free(ctx);
}

// the geometry of a new handle: fixed for its life, parked or not
static void copy_plan(nnd_ctx *ctx, const nnd_plan &pl) {
    ctx->n = pl.n, ctx->own_lo = pl.own_lo, ctx->own_hi = pl.own_hi, ctx->n_ranks = pl.n_ranks, ctx->slim = pl.slim;
    ctx->d = pl.d, ctx->dp = pl.dp, ctx->k = pl.k, ctx->ks = pl.ks, ctx->mc = pl.mc, ctx->mcp = pl.mcp, ctx->rcap = pl.rcap, ctx->pcap = pl.pcap;
    ctx->P = pl.P, ctx->max_segs = pl.max_segs;
    ctx->s_stride = pl.s_stride, ctx->s_m = pl.s_m, ctx->early_stop = pl.early_stop, ctx->cell_leaf = pl.cell_leaf;
    ctx->node_cap = pl.node_cap, ctx->cell_cap = pl.cell_cap;
}

// Stream, events and every create-time table of a handle whose plan is in place.  The order and the element counts of the
// allocations are part of the build's behaviour (addresses, alignment); after the first failure the later steps do nothing.
static int allocate_tables(nnd_ctx *ctx, const int64_t *bounds_host) {
    int rc = 0;
    auto A = [&](auto **p, size_t count) { if (!rc) rc = dalloc(ctx, p, count); };
    auto need = [&](bool ok, const char *what) { if (!rc && !ok) { ctx->set_error("%s", what); rc = 1; } };
    const nnd_params *p = &ctx->p;
    need(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess, "hipStreamCreate failed");
    need(rc || (hipEventCreate(&ctx->ev0) == hipSuccess && hipEventCreate(&ctx->ev1) == hipSuccess &&
                hipEventCreateWithFlags(&ctx->ev_spin, hipEventDisableTiming) == hipSuccess), "hipEventCreate failed");
    const size_t n = (size_t)ctx->n;
    const bool graph = !(p->flags & NND_FLAG_NO_GRAPH), prepared = !(p->flags & NND_FLAG_NO_PREP);
    need(prepared || !graph, "NND_FLAG_NO_PREP needs NND_FLAG_NO_GRAPH (the build reads the prepared rows)");
    if (prepared) {
        A(&ctx->xp, n * ctx->dp);
        A(&ctx->nrm, n);
        if (p->n_trees > 0) A(&ctx->xh, n * ctx->dp);
        if (p->n_trees > 0) A(&ctx->nr2, n);
        A(&ctx->mean, (size_t)ctx->dp + 4);  // + scale of the screening copies, 1 / scale^2, sampled max
    }
    if (graph) {
        A(&ctx->knn_e, n * ctx->ks);
        A(&ctx->knn_d, n * ctx->ks);
        A(&ctx->th, n);
        const size_t rows = (size_t)ctx->slim_rows(), row0 = (size_t)ctx->slim_row0();  // per-OWNED-row tables
        int32_t *a_cand = nullptr;
        uint32_t *a_rbuf = nullptr;
        uint8_t *a_active = nullptr;
        uint64_t *a_pbuf = nullptr;
        A(&a_cand, rows * 2 * ctx->mcp);
        A(&a_rbuf, rows * 2 * ctx->rcap);
        A(&a_active, rows);
        A(&a_pbuf, rows * ctx->pcap);
        if (!rc) {  // the working pointers are biased by -own_lo rows (0 on a plain handle): kernels index by global vertex id
            ctx->cand = a_cand - row0 * 2 * ctx->mcp;
            ctx->rbuf = a_rbuf - row0 * 2 * ctx->rcap;
            ctx->active = a_active - row0;
            ctx->pbuf = a_pbuf - row0 * ctx->pcap;
        }
        if (ctx->slim) A(&ctx->pbuf_r, n * ctx->pcap_r);
        A(&ctx->pdirty, n);
        // on the handle's stream: the NULL-stream form is ordered behind the caller's pending NULL-stream work (torch's
        // default stream) and not with this handle's non-blocking stream -- it could clear the flags of a build in progress
        need(rc || hipMemsetAsync(ctx->pdirty, 0, n, ctx->stream) == hipSuccess, "hipMemset failed");
        if (ctx->n_ranks > 0)
            need(rc || (ctx->mem.alloc(&ctx->shard_bounds, 65) && ctx->mem.alloc(&ctx->shard_cursors, 66) &&
                        hipMemcpy(ctx->shard_bounds, bounds_host, sizeof(int64_t) * (size_t)(ctx->n_ranks + 1), hipMemcpyHostToDevice) == hipSuccess),
                 "allocation of the shard tables failed");
    }
    A(&ctx->counters, (size_t)CNT_COUNT * NND_CNT_STRIPES);
    A(&ctx->counters_sum, (size_t)CNT_COUNT);
    need(rc || hipHostMalloc((void **)&ctx->h_pin, sizeof(nnd_pin_words), hipHostMallocDefault) == hipSuccess, "hipHostMalloc failed");
    if (rc) return rc;
    memset(ctx->h_pin, 0, sizeof(nnd_pin_words));
    if (hipHostGetDevicePointer((void **)&ctx->h_pin_dev, ctx->h_pin, 0) != hipSuccess) { (void)hipGetLastError(); ctx->h_pin_dev = nullptr; }
    if (p->n_trees > 0) {
        const size_t P = (size_t)ctx->P, S = (size_t)ctx->max_segs;
        if (ctx->s_m > 0) {  // the routing forest (plan.h nnd_plan_routes)
            A(&ctx->xs, (size_t)ctx->s_m * ctx->dp);
            A(&ctx->xsh, (size_t)ctx->s_m * ctx->dp);
            A(&ctx->nr2s, (size_t)ctx->s_m);
            A(&ctx->node_hf, (size_t)ctx->node_cap * (ctx->dp + 4));
            A(&ctx->node_hh, (size_t)ctx->node_cap * ctx->dp);
            A(&ctx->node_child, (size_t)ctx->node_cap * 2);
            A(&ctx->node_pack, (size_t)ctx->node_cap * (2 * ctx->dp + 16));
            A(&ctx->node_hfc, (size_t)ctx->node_cap * (ctx->dp + 4));
            A(&ctx->route_roots, (size_t)NND_ROUTE_ROOTS_WORDS);
            A(&ctx->s_leaf_depth, (size_t)p->n_trees * (size_t)ctx->s_m);
            A(&ctx->cell_count, (size_t)ctx->cell_cap);
            A(&ctx->cell_start, (size_t)ctx->cell_cap);
            A(&ctx->cell_depth, (size_t)ctx->cell_cap);
            A(&ctx->small_list, (size_t)ctx->cell_cap * NND_WORK_LIST_ROWS);
        }
        for (int i = 0; i < 2; i++) {
            A(&ctx->perm[i], P);
            A(&ctx->pos_seg[i], P);
            A(&ctx->seg_start[i], S);
            A(&ctx->seg_len[i], S);
        }
        A(&ctx->inv, P);
        A(&ctx->side, P);
        A(&ctx->side_pt, P);
        A(&ctx->leaf_flag, P);
        A(&ctx->scan_out, P + 1);
        A(&ctx->scan_blk, P / 2048 + 2);
        A(&ctx->seg_nleft, S);
        A(&ctx->seg_child, (NND_SEG_CHILD_WORDS + NND_WORK_LIST_ROWS) * S);  // child ids + finisher work list (nnd_fin_list)
        A(&ctx->hyper, S * (size_t)(ctx->dp + 4));
        A(&ctx->hyper_h, S * (size_t)ctx->dp);
        // (sized for any tree count: a shard finishes cells of ALL the build's trees, whatever its own allocation)
        A(&ctx->tree_begin_dev, (size_t)4097);
        need(rc || hipHostMalloc((void **)&ctx->h_tree_begin, sizeof(long long) * (size_t)4097, hipHostMallocDefault) == hipSuccess, "hipHostMalloc failed");
    }
    return rc;
}

static nnd_ctx *take_parked(const nnd_params *p);
extern "C" int32_t nnd_create(nnd_handle_t *out, const nnd_params *p) { return nnd_create_impl(out, p, nullptr, 0, 0); }

// check, plan, copy the plan, allocate
int nnd_create_impl(nnd_handle_t *out, const nnd_params *p, const int64_t *bounds_host, int n_ranks, int rank) {
    if (!out || !p) { gerr("nnd_create: null argument"); return 1; }
    *out = nullptr;
    if (nnd_check_params(p, g_err, sizeof(g_err))) return 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { gerr("nnd_create: no HIP device visible (this library has no CPU path)"); return 1; }
    if (p->device < 0 || p->device >= ndev) { gerr("nnd_create: device %d out of range (%d visible)", p->device, ndev); return 1; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p->device) != hipSuccess) { gerr("nnd_create: hipGetDeviceProperties failed"); return 1; }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) { gerr("nnd_create: device %d is %s; this build targets gfx950 (MI355X) only", p->device, prop.gcnArchName); return 1; }
    if (hipSetDevice(p->device) != hipSuccess) { gerr("nnd_create: hipSetDevice failed"); return 1; }
    if (!bounds_host) {
        if (nnd_ctx *parked = take_parked(p)) {
            *out = parked;
            return 0;
        }
        nnd_release_parked();  // a parked handle of another geometry: its memory is wanted now
    }
    // one shard of a row-sharded build: the geometry is known before anything is allocated
    if (bounds_host && nnd_check_shard_bounds(p->n, bounds_host, n_ranks, rank, g_err, sizeof(g_err))) return 1;

    std::lock_guard<std::recursive_mutex> lifecycle(nnd_lifecycle_mutex());
    const nnd_plan pl = nnd_make_plan(*p, bounds_host, n_ranks, rank);
    nnd_ctx *ctx = new nnd_ctx();
    arm_for_build(ctx, p, pl);
    copy_plan(ctx, pl);
    if (allocate_tables(ctx, bounds_host)) {
        gerr("nnd_create: %s", ctx->err);
        free_all(ctx);
        delete ctx;
        return 1;
    }
    *out = ctx;
    return 0;
}

// Creating and releasing a handle's HBM costs ~10 ms at 1 M points (every hipFree synchronises the device and unmaps;
// doing it on a background thread only moved the cost into the next call's hipMalloc).  nnd_destroy therefore PARKS one
// plain handle instead of freeing it, and nnd_create re-arms the parked handle when the geometry matches (same device,
// n, dim, metric, k, trees, leaf size, candidates, flags): repeated builds -- NNDescent(...) in a loop, nnd_build -- pay
// neither.  The parked handle holds its memory until a different geometry arrives, nnd_release_pending() is called, or
// the process ends; an allocation that fails while a handle is parked releases it and tries once more.
static std::mutex g_park_mu;
static nnd_ctx *g_parked = nullptr;

static void destroy_now(nnd_ctx *ctx) {
    std::lock_guard<std::recursive_mutex> lifecycle(nnd_lifecycle_mutex());
    (void)hipSetDevice(ctx->p.device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    free_all(ctx);
    delete ctx;
}
static void nnd_release_parked() {
    nnd_ctx *old = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_park_mu);
        old = g_parked;
        g_parked = nullptr;
    }
    if (old) destroy_now(old);
}
static bool same_geometry(const nnd_params &a, const nnd_params &b) {
    return a.n == b.n && a.dim == b.dim && a.metric == b.metric && a.n_neighbors == b.n_neighbors && a.n_trees == b.n_trees &&
           a.leaf_size == b.leaf_size && a.max_candidates == b.max_candidates && a.device == b.device && a.flags == b.flags;
}
// a parked handle of this geometry, re-armed for a new build (seeds, counters, per-build flags), or nullptr
static nnd_ctx *take_parked(const nnd_params *p) {
    nnd_ctx *ctx = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_park_mu);
        if (g_parked && same_geometry(g_parked->p, *p)) {
            ctx = g_parked;
            g_parked = nullptr;
        }
    }
    if (!ctx) return nullptr;
    (void)hipSetDevice(p->device);
    arm_for_build(ctx, p, nnd_plan_join(*p));
    if (!ctx->stream_owned) {  // a borrowed stream must not outlive its lender
        ctx->stream = nullptr;
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { destroy_now(ctx); return nullptr; }
        ctx->stream_owned = true;
    }
    if (!ctx->x_owned) ctx->x_orig = nullptr;  // a borrowed point set is gone; an owned copy's buffer is reused by nnd_set_data_host
    return ctx;
}

extern "C" int32_t nnd_destroy(nnd_handle_t ctx) {
    if (!ctx) return 0;
    (void)hipSetDevice(ctx->p.device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    nnd_ctx *old = nullptr;
    if (ctx->n_ranks == 0) {  // plain handles only: a shard's tables are sized by its slice
        std::lock_guard<std::mutex> lk(g_park_mu);
        old = g_parked;
        g_parked = ctx;
    } else {
        old = ctx;
    }
    if (old) destroy_now(old);
    return 0;
}
// release the parked handle's device memory now
extern "C" int32_t nnd_release_pending(void) {
    nnd_release_parked();
    return 0;
}

// Run on the caller's HIP stream (e.g. torch's current stream) instead of the handle's own: the library's kernels and the
// caller's work are then ordered by the stream itself, no host synchronisation between them.  NULL: back to own.
extern "C" int32_t nnd_set_stream(nnd_handle_t ctx, void *hip_stream) {
    if (!ctx) { gerr("null handle"); return 1; }
    NND_HIP_CHECK(hipSetDevice(ctx->p.device));
    NND_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (hip_stream) {
        if (ctx->stream_owned && ctx->stream) { NND_HIP_CHECK(hipStreamDestroy(ctx->stream)); }
        ctx->stream = (hipStream_t)hip_stream;
        ctx->stream_owned = false;
    } else if (!ctx->stream_owned) {
        NND_HIP_CHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
        ctx->stream_owned = true;
    }
    return 0;
}
