/*
 * pynnd_amd.h -- C ABI of the MI355X (gfx950) NN-Descent index builder.
 *
 * This is the drop-in boundary for the BUILD path of lmcinnes/pynndescent 0.6.0.
 * The reference has no FFI of its own (it is Python + numba); the boundary is the
 * two call sites inside NNDescent.__init__ (reference pynndescent/pynndescent_.py):
 *
 *     make_forest(...) + rptree_leaf_array(...)      pynndescent_.py:1118-1130
 *     nn_descent(data, n_neighbors, rng_state, max_candidates, dist, n_iters,
 *                delta, init_graph, rp_tree_init, leaf_array, ...)
 *                                                    pynndescent_.py:1247-1260
 *
 * Each entry point below names the reference function(s) it replaces.  All
 * pointers are plain host or device pointers, all sizes are explicit, no C++ or
 * torch types cross the boundary.  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - Every function returns 0 on success, non-zero on failure; the message is
 *     available from nnd_last_error(handle) (or nnd_last_global_error() when no
 *     handle exists yet).  There is NO CPU fallback: without a gfx950 device
 *     nnd_create fails.
 *   - "alt space": distances are squared-euclidean (metric 0),
 *     log2(|x||y|/<x,y>) (metric 1), -log2<x,y> of L2-normalised rows (2),
 *     1/<x,y> (3), 1 - Pearson correlation (4), log2(sqrt(|x|_1|y|_1) /
 *     sum sqrt(x_i y_i)) (5) or log2(|x||y|/<x,y>) + 1/sqrt<x,y> (6, a proxy: handed out as it is), exactly what the reference keeps in
 *     NNDescent._neighbor_graph (distances.py:63-91, 583-630, 680, 759, 1284, 1387);
 *     the caller applies sqrt / 1-2^-d / -1/d / sqrt(1-2^-d) itself
 *     (distances.py:2170-2173), as NNDescent.neighbor_graph does.
 *   - Output rows are ascending in distance; missing entries are (-1, +inf) at
 *     the row tail (utils.py:130-158, 189-218).
 *   - One handle = one GPU = one HIP stream.  Calls on one handle must be
 *     serialised by the caller; distinct handles are independent.
 */
#ifndef PYNND_AMD_H
#define PYNND_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NND_METRIC_SQEUCLIDEAN 0 /* reference distances.py:63  squared_euclidean  */
#define NND_METRIC_ALT_COSINE 1  /* reference distances.py:583 alternative_cosine */
#define NND_METRIC_ALT_DOT 2     /* reference distances.py:680 alternative_dot (rows L2-normalised by the kernels) */
#define NND_METRIC_ALT_INNER_PRODUCT 3 /* reference distances.py:759 alternative_inner_product (rows as given) */
#define NND_METRIC_CORRELATION 4 /* reference distances.py:1284 correlation (a true distance: no correction) */
#define NND_METRIC_ALT_HELLINGER 5 /* reference distances.py:1387 alternative_hellinger (input must be >= 0) */
/* Proxy metrics: a distance to build and walk on, with a true distance to rerank by (reference distances.py:2190 proxy_distances).
 * They continue the numbering of the codes above; the six #define lines above stay the list of the alt-space metrics
 * (tests/test_metrics_cpu.py holds that list), so this family is an enumeration of its own.
 * NND_METRIC_PROXY_INNER_PRODUCT: reference distances.py:810 proxy_inner_product (rows as given), the build's and the walk's
 * distance of metric="proxy_inner_product"; its true distance, the negative inner product, is what nnd_searcher_query_rerank
 * returns.  <x,y> = 0 is FLT_MAX here, +inf in the reference. */
enum { NND_METRIC_PROXY_INNER_PRODUCT = 6 };
/* Boolean metrics (reference distances.py:259-552): functions of the counts of the indicator rows b_x = (x != 0) --
 * c = <b_x, b_y> = n_TT, a = nnz(x), b = nnz(y), ne = a + b - 2c, and the column count d.  The kernels build and walk on
 * indicator rows (x != 0 -> 1, else 0); the distances handed back are the float64 formulas on the counts of the rows as given.
 * NND_METRIC_JACCARD is alternative_jaccard, -log2(c / (c + ne)) (the caller applies 1 - 2^-v; c = 0 on a non-empty union is
 * FLT_MAX here, +inf in the reference); the other eight are the reference's distances as they are.  dim must be below 2^23.  7 is no code
 * (nnd_create has always refused it, and a test pins that refusal).
 * An enumeration of its own, like the proxy family: the six #define lines above stay the list of the alt-space metrics. */
enum {
    NND_METRIC_JACCARD = 8,         /* alternative_jaccard :303 */
    NND_METRIC_DICE = 9,            /* ne / (2c + ne) :360 */
    NND_METRIC_SOKALSNEATH = 10,     /* ne / (0.5c + ne) :479 */
    NND_METRIC_MATCHING = 11,       /* ne / d :340 */
    NND_METRIC_ROGERSTANIMOTO = 12, /* 2ne / (d + ne) :414 */
    NND_METRIC_SOKALMICHENER = 13,  /* the same :458 */
    NND_METRIC_KULSINSKI = 14,      /* (ne - c + d) / (ne + d) :386 */
    NND_METRIC_RUSSELLRAO = 15,     /* (d - c) / d :435 */
    NND_METRIC_YULE = 16            /* 2 n_TF n_FT / (c n_FF + n_TF n_FT) :525 */
};

#define NND_ABI_VERSION 6 /* 6 (round 6): nnd_stats grew join_substeps[] and nnd_shard_info grew gather_bytes[] / gather_section[] at their ends; nnd_host_alloc / nnd_host_free; 5: nnd_search_graph / nnd_search_graph_fetch */

typedef struct nnd_handle_s *nnd_handle_t;

/* Build parameters; mirrors the NNDescent ctor kwargs that reach the build path
 * (pynndescent_.py:976-1007) after the ctor's defaulting (pynndescent_.py:1009-1012,
 * 1135-1138; rp_trees.py:2845-2846).  The host code does the defaulting. */
typedef struct nnd_params {
    int64_t n;              /* points */
    int32_t dim;            /* features */
    int32_t metric;         /* NND_METRIC_* */
    int32_t n_neighbors;    /* k, 1..256 (rows above 64 entries are merged through LDS: correct, not tuned) */
    int32_t n_trees;        /* 0 = no RP-forest initialisation */
    int32_t leaf_size;      /* > 0 */
    int32_t max_depth;      /* max_rptree_depth (pynndescent_.py:1000) */
    int32_t max_candidates; /* 1..128 (above 64: five passes of the 64-slot join over blocks of the candidate lists) */
    int32_t n_iters;
    float delta;            /* stop when c <= delta*k*n (pynndescent_.py:317) */
    int64_t rng_state[3];   /* NNDescent.rng_state (pynndescent_.py:1105-1107) */
    int64_t tree_rng[3];    /* first row of make_forest's per-tree draw (rp_trees.py:2850) */
    int32_t device;         /* HIP device ordinal */
    int32_t join_blocks;    /* descent sub-steps per iteration; reference blocks by 16384 vertices (pynndescent_.py:279).  0 = chosen by the
                             * library: 1 up to 64 neighbours, ceil(k / 32) above (a row takes at most 64 updates per sub-step) */
    int32_t flags;          /* NND_FLAG_*; 0 for a build handle */
    int32_t reserved[5];
} nnd_params;

/* Auxiliary handles (the pruning pass and the hub search tree of NNDescent.prepare() run on a handle of their own):
 * NND_FLAG_NO_GRAPH skips the k-lists, candidate / proposal / reverse-offer tables and the routing-forest tables -- a
 * handle for nnd_diversify_*_host / nnd_degree_prune_host / nnd_hub_tree_*; every build entry point fails on it.
 * NND_FLAG_NO_PREP additionally skips the prepared (padded, centred / normalised) copy of the rows: hub tree only. */
#define NND_FLAG_NO_GRAPH 1
#define NND_FLAG_NO_PREP 2
/* test hook: candidate selection by the one-wave-per-vertex kernel where the two-vertices-per-wave kernel would run
 * (tests/test_gpu_kernels.py proves the two produce identical lists) */
#define NND_FLAG_TEST_SELECT_WAVE 4
/* test hook (row-sharded build): proposal regions of ONE record per destination row instead of 32, so that the deferral
 * path (records that do not fit stay in the sender's table and travel with the next iteration's) is exercised at test
 * sizes (tests/test_gpu_sharded.py) */
#define NND_FLAG_TEST_SMALL_REGIONS 8
/* test hook: the rp forest's routing pass as ONE walk per (tree, point) through global memory (the round-2 kernel)
 * instead of the two coherent passes; the two assign every point to the same cell (tests/test_gpu_kernels.py) */
#define NND_FLAG_TEST_ROUTE_PLAIN 16
/* test hooks of the row-sharded build (tests/test_gpu_sharded.py): the forest split by tree (the round-3 scheme) where it
 * would be sharded by cell; a rank that FAILS at the start of its second iteration (error return: the other ranks must
 * return an error too, promptly); a rank that VANISHES there (returns without telling anybody, as a killed process
 * would: the other ranks must give up after the communicator's timeout) */
#define NND_FLAG_TEST_FOREST_BY_TREE 32
#define NND_FLAG_TEST_FAIL 64
#define NND_FLAG_TEST_VANISH 128
/* test hook: the reverse offers of the candidate sampling through the round-1..4 kernel (one device-scope atomicMin per
 * edge into 32 hashed slots per bank) instead of the bucketed transposition (sample.hip): comparison / timing */
#define NND_FLAG_TEST_SAMPLE_ATOMIC 256
/* test hook (row-sharded build): a rank pretends that the forest sharded by cell cannot be built on this data -- at the
 * tree tops (512), at the owners' shares (1024) or at the over-long cells (512 | 1024); the ranks must agree and build
 * the forest split by tree instead (tests/test_gpu_sharded.py) */
#define NND_FLAG_TEST_FOREST_FALLBACK_TOPS 512
#define NND_FLAG_TEST_FOREST_FALLBACK_SHARE 1024
#define NND_TEST_FALLBACK_AT(flags) ((((flags) & 512) ? 1 : 0) + (((flags) & 1024) ? 2 : 0))
/* test hook: the candidate sampling behaves as if the record regions of the bucketed transposition could not be allocated
 * (wide rows on a full device): the handle must switch to the hashed slots and build, not fail (tests/test_gpu_kernels.py) */
#define NND_FLAG_TEST_SAMPLE_NOMEM 2048
/* test hook: the fused candidate selection with 32 lanes per vertex where rows and candidate lists of at most 16 entries would
 * take 16 (four vertices per wave): the two forms must write identical lists (tests/test_gpu_kernels.py) */
#define NND_FLAG_TEST_SELECT_HALF 4096
/* test hook (row-sharded build): the per-iteration threshold / neighbour-id all-gather on the BUILD's channel, in front of the offer
 * exchange (rounds 3-5), where it would run on the second channel beside the sampling: same graph either way (tests/test_gpu_sharded.py) */
#define NND_FLAG_TEST_GATHER_INLINE 8192
/* test hook: the local join of 17..32 candidates per class (k_local_join_w) reads the neighbour lists of its membership tests from
 * global memory (rounds 3-5) where it would stage them in LDS (round 6, rows of <= 32 neighbours on one GPU): the two forms must
 * build the same graph, entry for entry (tests/test_gpu_kernels.py) */
#define NND_FLAG_TEST_JOIN_UNSTAGED 16384

/* test hook: nnd_exact_knn_* answers every row through the float64 tier (tests/test_gpu_exact.py compares the two tiers) */
#define NND_FLAG_TEST_EXACT_F64 32768
/* test hook: nnd_init_random launches one wave per row (the earlier form) where it would let one wave screen 64 rows and work on
 * those that are not full: the two forms must leave identical k-lists (tests/test_gpu_random_init.py) */
#define NND_FLAG_TEST_RANDOM_INIT_ROWWISE 65536

/* Run-time statistics for measurement (bench.py roofline). */
typedef struct nnd_stats {
    int64_t n_iters_run;
    int64_t n_leaves;
    int64_t tree_levels;
    int64_t leaf_pairs;          /* pair distances evaluated during leaf seeding */
    int64_t leaf_rows;           /* point rows loaded by the leaf kernel */
    int64_t join_pairs[64];      /* P_i: pair distances evaluated, per iteration */
    int64_t join_rows[64];       /* C_i: candidate rows gathered, per iteration */
    int64_t join_active[64];     /* vertices with >=1 new candidate, per iteration */
    int64_t proposals[64];       /* proposals emitted by the join, per iteration */
    int64_t updates[64];         /* c: accepted k-list insertions, per iteration */
    float ms_prep, ms_forest, ms_leaf_init, ms_random_init, ms_descent, ms_finalize;
    float ms_sample[64], ms_join[64], ms_merge[64];
    int64_t join_mfma[64];       /* v_mfma_f32_16x16x4_f32 instructions issued by the join (2048 flop each), per iteration */
    int64_t leaf_mfma;           /* the same for the leaf-seeding kernel, whole stage */
    int64_t n_cells;             /* rp forest: cells of the routing pass (0 = whole-set level-synchronous build) */
    int64_t join_substeps[64];   /* ABI 6: join + merge sub-steps of every iteration (join_blocks, or the library's schedule when join_blocks = 0) */
} nnd_stats;

int32_t nnd_abi_version(void);
const char *nnd_last_global_error(void);
const char *nnd_last_error(nnd_handle_t h);

/* Create a builder on params->device and allocate its HBM state (k-lists,
 * candidate lists, proposal buffers).  Fails if the device is not gfx950. */
int32_t nnd_create(nnd_handle_t *out, const nnd_params *params);
/* nnd_destroy PARKS one plain handle instead of releasing it (every hipFree synchronises the device: ~9 ms for the state
 * of a 1 M-point build, and as much again for the next hipMalloc): an nnd_create of the same geometry re-arms it.  A
 * create of another geometry, an allocation that fails, or nnd_release_pending() releases the parked handle's HBM. */
int32_t nnd_destroy(nnd_handle_t h);
int32_t nnd_release_pending(void);

/* Host-side helpers for the result arrays (NNDescent.neighbor_graph returns a COPY of the ids and the corrected
 * distances, pynndescent_.py:2145-2158): a fresh 60 MB destination costs ~15 k first-touch page faults, which a
 * single-threaded numpy copy / sqrt pays one after the other (18 + 14 ms at 1 M x 15).  These split the range over a few
 * host threads.  nnd_host_sqrt_f32 is IEEE sqrtf per element: bit-identical to numpy.sqrt on float32. */
int32_t nnd_host_copy(void *dst, const void *src, int64_t bytes);
int32_t nnd_host_sqrt_f32(float *dst, const float *src, int64_t count);
/* Pinned host memory for result arrays (round 6).  The reference returns freshly allocated numpy arrays
 * (pynndescent_.py:2145-2158, 1247-1260); at 1 M x 15 their first touch cost more than the device-to-host copy itself.  The host
 * side of the drop-in class keeps a small pool of these buffers (pynndescent_amd/_capi.py HostPool): a buffer goes back to the
 * pool when the last numpy view of it dies.  nnd_host_alloc returns NULL without a device or without memory (callers fall back
 * to ordinary allocations); the finalize / build entry points recognise a pinned destination and copy into it with one DMA. */
void *nnd_host_alloc(int64_t bytes);
int32_t nnd_host_free(void *p);

/* Point set, float32 C-contiguous (n, dim) -- NNDescent._raw_data (pynndescent_.py:1054-1057).
 * Host variant copies H2D; device variant BORROWS the pointer (it must outlive the handle's
 * build calls).  Both then run the prep kernel (pad to 32 floats, centre / L2-normalise, norms)
 * on the handle's stream, immediately: the device buffer must be COMPLETE when the call is made --
 * synchronise the stream that produced it first, or make the handle run on that stream
 * (nnd_set_stream).  The prepared copy is made once per call, not once per build. */
int32_t nnd_set_data_host(nnd_handle_t h, const float *x);
int32_t nnd_set_data_device(nnd_handle_t h, const float *x_dev);
/* Device arrays of other types (a caller whose embeddings live on the GPU, often in half precision).  dtype: */
#define NND_DTYPE_FLOAT32 0
#define NND_DTYPE_FLOAT16 1  /* IEEE binary16 */
#define NND_DTYPE_BFLOAT16 2
#define NND_DTYPE_FLOAT64 3
/* nnd_set_data_device_typed: the point set as (n, dim) C-contiguous rows of `dtype` on the handle's device.  float32 is BORROWED
 * exactly as nnd_set_data_device borrows it; the other types are converted on the handle's stream into the handle's OWN float32
 * copy (binary16 / bfloat16 exactly, float64 rounded to nearest even, what numpy's astype(float32) does), and the caller's
 * buffer is free again once the stream has passed the call.  NND_METRIC_ALT_DOT: rows of every type, float32 included, go into
 * the own copy L2-normalised (x / sqrt(sum x^2), float32 accumulation, zero rows stay zero), which the host entry leaves to its
 * caller (pynndescent_.py:1101-1102).  Then the prep kernel runs as for the other two entries; the stream rule is theirs. */
int32_t nnd_set_data_device_typed(nnd_handle_t h, const void *x_dev, int32_t dtype);
/* The same conversion without a handle, on `device` and `hip_stream` (NULL: the device's default stream): (n, dim) rows of
 * `dtype` at src_dev -> float32 at dst_dev, L2-normalised when `normalize` is non-zero.  A query batch before a searcher sees
 * it; dot's rows where the caller keeps the normalised copy itself.  Asynchronous: nothing is waited for. */
int32_t nnd_device_rows_f32(int32_t device, void *hip_stream, const void *src_dev, int32_t dtype, int64_t n, int32_t dim,
                            int32_t normalize, float *dst_dev);
/* Sparse input: the CSR matrix at indptr_dev (n + 1 entries) / indices_dev / values_dev (float32), all on `device`, written
 * dense into the (n, dim) float32 buffer dst_dev (row stride dim, any dim >= 1; aligned to a float).  indptr_width and
 * indices_width are the byte widths of the two index arrays, 4 (int32) or 8 (int64) each, as scipy hands them out.  The matrix
 * is CANONICAL (column indices ascending within a row, no duplicates; the caller sees to it): every element of dst is then
 * written exactly once -- an explicitly stored zero like any other value -- and dst is never read.  indices_dev / values_dev may be
 * NULL for a matrix without a stored entry.  Queued on `hip_stream` (NULL: the device's default stream): nothing is waited for. */
int32_t nnd_device_csr_rows(int32_t device, void *hip_stream, const void *indptr_dev, int32_t indptr_width, const void *indices_dev,
                            int32_t indices_width, const float *values_dev, int64_t n, int32_t dim, float *dst_dev);
/* Corrections of the kernels' distances (the reference's distance_correction, pynndescent_.py:1271-1298) on the device, without
 * a handle: a graph is corrected when NNDescent.neighbor_graph is read, long after its builder is gone.  `count` float32 values
 * at in_dev -> out_dev, asynchronous on `hip_stream` of `device`.  Unfilled entries (+inf) come out as the host functions map
 * them: sqrt +inf, cosine 1, inner product 0, hellinger 1, haversine pi. */
#define NND_CORRECT_COPY 0              /* 32-bit words out, bit for bit (sqeuclidean, correlation, the proxies; the ids of a graph) */
#define NND_CORRECT_SQRT 1              /* float32 out, correctly rounded: the bits of numpy.sqrt */
#define NND_CORRECT_ALT_COSINE 2        /* float64 out: 1 - 2^-d */
#define NND_CORRECT_ALT_INNER_PRODUCT 3 /* float64 out: d >= FLT_MAX ? 0 : -1 / d (an IEEE division: the host's bits) */
#define NND_CORRECT_ALT_HELLINGER 4     /* float64 out: sqrt(1 - 2^-d) */
#define NND_CORRECT_HAVERSINE 5         /* float64 out: 2 asin(min(1, sqrt(d) / 2)), the angle of the squared chord d (+inf: pi) */
int32_t nnd_device_correct(int32_t device, void *hip_stream, int32_t kind, const float *in_dev, void *out_dev, int64_t count);
/* ---- metrics with a fixed linear map (csrc/linear.hip; DESIGN.md "Metrics"): seuclidean, wminkowski with p = 2, mahalanobis ----
 * They are NND_METRIC_SQEUCLIDEAN after y = A (x - c): the caller transforms every row that enters the library (training
 * rows, update() rows, queries) with one of the two entries below and hands the float32 result to the entry points of metric
 * code 0, unchanged.  kind: */
#define NND_LINEAR_DIAGONAL 0 /* map: dim floats, y_j = map[j] (x_j - shift_j): V^-1/2 of seuclidean, sqrt(w) of wminkowski */
#define NND_LINEAR_DENSE 1    /* map: (dim, dim) row-major, y_j = sum_k map[j, k] (x_k - shift_k): a factor of mahalanobis' VI */
/* (n, dim) float32 rows at x -> (n, dim) float32 rows at y (x == y is not allowed for the dense kind).  A row's result
 * depends on that row alone, bit for bit: not on n, on its position, on the other rows of the call, or on the run.
 * nnd_device_linear_rows: every pointer is a device pointer on `device`; queued on `hip_stream` (NULL: the default stream),
 * nothing is waited for, nothing is allocated.  nnd_linear_rows_host: every pointer is a host pointer; the rows go up, the
 * result comes down, and the call returns when it is there (its device buffers are one nnd_scratch, released on return). */
int32_t nnd_device_linear_rows(int32_t device, void *hip_stream, int32_t kind, int32_t dim, const float *map_dev, const float *shift_dev,
                               const float *x_dev, int64_t n, float *y_dev);
int32_t nnd_linear_rows_host(int32_t device, int32_t kind, int32_t dim, const float *map, const float *shift, const float *x, int64_t n,
                             float *y);
/* ---- derived metrics: a per-row map, then a metric above (csrc/rowmap.hip; DESIGN.md "Row maps") ----
 * As with the linear maps, the caller maps every row that enters the library and hands the float32 result to the entry points
 * of the base metric's code, unchanged.  kind: */
#define NND_ROWMAP_RANK 0   /* dim in, dim out: the average ranks of the row's values (ties share the mean of their places); exact.
                             * spearmanr = NND_METRIC_CORRELATION of the rank rows.  1 <= dim <= 16384; shift is not read */
#define NND_ROWMAP_SPHERE 1 /* 2 in (lat, lon; radians), 3 out: (cos lat cos lon, cos lat sin lon, sin lat) - shift, in float64,
                             * rounded once.  haversine = NND_CORRECT_HAVERSINE of NND_METRIC_SQEUCLIDEAN of these rows; shift: 3 floats */
/* (n, dim) float32 rows at x, row i at x + i * x_stride (x_stride >= dim, in elements; the elements between the rows are never
 * read) -> contiguous float32 rows at y, of the kind's output width.  A row's result depends on that row alone, bit for bit.
 * A kind, width or stride outside the above is refused (nonzero, nnd_last_global_error), never clamped.  The two entries relate
 * as nnd_device_linear_rows and nnd_linear_rows_host do: device pointers, queued on `hip_stream`, nothing waited for or
 * allocated; or host pointers (x: (n - 1) * x_stride + dim floats), and the call returns when the result is there. */
int32_t nnd_device_map_rows(int32_t device, void *hip_stream, int32_t kind, int32_t dim, int64_t x_stride, const float *shift_dev,
                            const float *x_dev, int64_t n, float *y_dev);
int32_t nnd_map_rows_host(int32_t device, int32_t kind, int32_t dim, int64_t x_stride, const float *shift, const float *x, int64_t n,
                          float *y);
/* ---- NNDescent.update() / recall() of an index whose rows and graph live on the device (csrc/devarray.hip, csrc/update.hip;
 * DESIGN.md "Device arrays") ----  Like the two entries above: a device ordinal and a HIP stream (NULL: the device's default
 * stream) instead of a handle, everything is queued there and nothing is waited for; every array is the caller's and must stay
 * valid until the stream has passed the call.
 *
 * nnd_device_update_rows: the grown point set (pynndescent_.py:2461-2476).  out_dev: (n_old + n_fresh, dim) rows of out_dtype,
 * 16-byte aligned.  Rows [0, n_old) = old_dev, rows [n_old, ..) = fresh_dev, then row upd_ids_dev[i] = row upd_rows_dev[i] of
 * upd_dev ((n_upd, dim)) for the n_pairs pairs; the ids of the pairs must be distinct and in [0, n_old) (the host resolves
 * duplicates and negative ids first; a pair out of range is skipped).  Each of the three inputs has an NND_DTYPE_* of its own
 * (ignored where its count is 0).  out_dtype is either the one type all inputs share -- then no value is converted -- or
 * NND_DTYPE_FLOAT32: binary16 / bfloat16 widen exactly, float64 rounds to nearest even (nnd_set_data_device_typed's conversion).
 * Nothing is normalised. */
int32_t nnd_device_update_rows(int32_t device, void *hip_stream, int32_t dim, const void *old_dev, int32_t old_dtype, int64_t n_old,
                               const void *fresh_dev, int32_t fresh_dtype, int64_t n_fresh, const void *upd_dev, int32_t upd_dtype,
                               int64_t n_upd, const int32_t *upd_rows_dev, const int32_t *upd_ids_dev, int64_t n_pairs, void *out_dev,
                               int32_t out_dtype);
/* nnd_device_update_graph: the invalidated, padded graph of the warm start (pynndescent_.py:2478-2493).  idx_dev / dist_dev: the
 * old (n_old, k) graph; upd_ids_dev: the n_upd ids of the updated points (in [0, n_old); repeats allowed); map_dev: n_old bytes
 * of scratch (the "is updated" lookup, written here).  out_idx_dev / out_dist_dev, (n_new, k) with n_new >= n_old: the rows of
 * updated points, every entry that points at one (cleared in place) and the rows from n_old on are (-1, +inf); every other entry
 * is copied. */
int32_t nnd_device_update_graph(int32_t device, void *hip_stream, const int32_t *idx_dev, const float *dist_dev, int64_t n_old, int32_t k,
                                const int32_t *upd_ids_dev, int64_t n_upd, int64_t n_new, uint8_t *map_dev, int32_t *out_idx_dev,
                                float *out_dist_dev);
/* nnd_device_recall_hits: *hits_dev (one int64 on the device, zeroed here) = the number of entries of true_idx_dev ((m, k),
 * k <= 256) that appear in row rows_dev[i] of graph_idx_dev ((n, width), width <= 256) -- sum(isin(true[i], graph[rows[i]])).
 * One wave per sampled row. */
int32_t nnd_device_recall_hits(int32_t device, void *hip_stream, const int32_t *true_idx_dev, int64_t m, int32_t k, const int32_t *graph_idx_dev,
                               int64_t n, int32_t width, const int32_t *rows_dev, int64_t *hits_dev);
/* *out = 1 when the point set held a NaN or an infinity (seen by the prep kernel while it read the rows).  The reference
 * rejects such input in check_array (pynndescent_.py:1054) with a scan of its own; the host mirror raises the same
 * error from this flag instead of scanning 488 MB on one core (24 ms at 1 M x 128). */
int32_t nnd_data_nonfinite(nnd_handle_t h, int32_t *out);
/* *out = 1 when the metric is NND_METRIC_ALT_HELLINGER and the point set held a negative entry (raised by the prep kernel
 * in the same pass).  The reference computes NaN distances from such input without a word; the host mirror raises
 * ValueError instead.  0 for every other metric. */
int32_t nnd_data_negative(nnd_handle_t h, int32_t *out);

/* make_forest (rp_trees.py:2815-2888): builds all n_trees trees level-synchronously on device. */
int32_t nnd_make_forest(nnd_handle_t h);
/* rptree_leaf_array (rp_trees.py:2891-2922): shape query then copy, int32 (n_leaves, max_leaf_size), -1 padded. */
int32_t nnd_leaf_array_shape(nnd_handle_t h, int64_t *n_leaves, int32_t *max_leaf_size);
int32_t nnd_get_leaf_array(nnd_handle_t h, int32_t *out_host);

/* make_heap (utils.py:130-158): reset the k-lists to (-1, +inf, 0). */
int32_t nnd_reset_graph(nnd_handle_t h);
/* init_rp_tree + generate_leaf_updates (pynndescent_.py:73-185): all-pairs inside every leaf. */
int32_t nnd_init_from_leaves(nnd_handle_t h);
/* The same on a CALLER-PROVIDED leaf array: the `leaf_array` argument of the reference's nn_descent
 * (pynndescent_.py:324-337) -- host int32 (n_leaves, max_leaf_size), -1 padded, as rptree_leaf_array returns it
 * (rp_trees.py:2891-2922); a row ends at its first negative entry (pynndescent_.py:88-92).  A caller that keeps the
 * reference's make_forest hands its leaves in here; the handle needs no forest of its own (n_trees may be 0). */
int32_t nnd_init_from_leaf_array(nnd_handle_t h, const int32_t *leaf_array, int64_t n_leaves, int32_t max_leaf_size);
/* init_random (pynndescent_.py:188-203): top up rows that are not full with random points. */
int32_t nnd_init_random(nnd_handle_t h);
/* initalize_heap_from_graph_indices[_and_distances] (utils.py:836-860), used for init_graph /
 * init_dist (pynndescent_.py:1225-1242).  init_dist may be NULL. Host pointers, (n, width), width <= 256. */
int32_t nnd_init_from_graph(nnd_handle_t h, const int32_t *init_idx, const float *init_dist, int32_t width);
/* init_from_neighbor_graph (pynndescent_.py:206-214), the warm start of NNDescent.update
 * (pynndescent_.py:2512-2517): the entries of an existing graph -- host (n, width) indices (-1 = none) and
 * alt-space distances (required) -- are inserted with flag 0 ("old").  Call after nnd_reset_graph. */
int32_t nnd_init_from_neighbor_graph(nnd_handle_t h, const int32_t *init_idx, const float *init_dist, int32_t width);
/* The two entries above for a graph on the handle's device: DEVICE pointers to the full (n, width) int32 ids and float32
 * distances (init_dist_dev nullable for nnd_init_from_graph_device, required for the neighbour-graph form), read in place on the
 * handle's stream (nnd_set_stream: the caller's), nothing is staged.  The arrays stay the caller's and must remain valid until
 * the stream has passed the call; nnd_init_from_graph_device returns without waiting, nnd_init_from_neighbor_graph_device
 * returns with the stream drained, as its host form does. */
int32_t nnd_init_from_graph_device(nnd_handle_t h, const int32_t *init_idx_dev, const float *init_dist_dev, int32_t width);
int32_t nnd_init_from_neighbor_graph_device(nnd_handle_t h, const int32_t *init_idx_dev, const float *init_dist_dev, int32_t width);

/* One iteration of nn_descent_internal (pynndescent_.py:296-320):
 * new_build_candidates (utils.py:221-320) + generate_graph_update_array (utils.py:536-658)
 * + apply_graph_update_array (utils.py:661-733).  *c_out = number of k-list insertions. */
int32_t nnd_descent_iter(nnd_handle_t h, int64_t *c_out);
/* The whole loop with the reference's stop rule (pynndescent_.py:317). */
int32_t nnd_descent(nnd_handle_t h);

/* deheap_sort (utils.py:189-218) + exact (f64-accumulated) recomputation of the n*k distances.
 * Writes int32 (n,k) indices and float32 (n,k) alt-space distances. */
int32_t nnd_finalize_host(nnd_handle_t h, int32_t *out_idx, float *out_dist);
int32_t nnd_finalize_device(nnd_handle_t h, int32_t *out_idx_dev, float *out_dist_dev);

/* Everything between "data is resident" and "graph is resident":
 * forest -> leaf init -> random init -> descent -> finalize (device outputs). */
int32_t nnd_build_device(nnd_handle_t h, int32_t *out_idx_dev, float *out_dist_dev);

/* One-shot host-buffer build == make_forest + rptree_leaf_array + nn_descent of the reference
 * (pynndescent_.py:1118-1130, 1247-1260).  init_idx/init_dist nullable (init_graph path). */
int32_t nnd_build(const nnd_params *params, const float *x, const int32_t *init_idx, const float *init_dist,
                  int32_t init_width, int32_t *out_idx, float *out_dist, nnd_stats *stats, char *err,
                  int32_t errlen);

int32_t nnd_get_stats(nnd_handle_t h, nnd_stats *out);
int32_t nnd_synchronize(nnd_handle_t h);

/* ---- introspection used by the parity tests (device state -> host) ---- */
/* Current k-lists, unsorted-by-contract but kept ascending: int32 idx (-1 empty), f32 dist, u8 new-flag. */
int32_t nnd_get_graph(nnd_handle_t h, int32_t *idx, float *dist, uint8_t *flags);
/* Candidate lists of the last nnd_descent_iter: int32 (n, max_candidates) each, -1 padded. */
int32_t nnd_get_candidates(nnd_handle_t h, int32_t *new_idx, int32_t *old_idx);
/* Sampling only (no join): fills the candidate lists and clears sampled new-flags. */
int32_t nnd_sample_candidates(nnd_handle_t h);
/* Pairwise alt-space distances between listed rows, computed by the same MFMA Gram tile code
 * the join uses: out (na, nb) float32 host. */
int32_t nnd_pairwise_gram(nnd_handle_t h, const int32_t *rows_a, int32_t na, const int32_t *rows_b, int32_t nb,
                          float *out);

/* ---- row-sharded multi-GPU build ----
 * The reference is single-process; its sharding idea is the owner-computes rule of apply_graph_update_array /
 * new_build_candidates / init_rp_tree (utils.py:709-731, 259-306; pynndescent_.py:154-185: each thread owns a contiguous
 * vertex range) and its knob is n_jobs (pynndescent_.py:1141-1143).  Here the same rule crosses GPUs: rank r owns rows
 * [lo_r, hi_r) of the k-lists; the point set is replicated once (all-gather over xGMI, on a second channel behind the
 * forest's first steps: candidate vectors never travel again); the forest is sharded BY CELL -- rank r builds the top of
 * its share of the trees on the global sample, the packed tops are all-gathered, every rank routes ITS rows through ALL
 * trees, the (cell, row) pairs go to the rank that owns the cell (1 / G of every tree's cells), which finishes the cells
 * and seeds the k-lists from their leaves; partial k-list rows go to their owners and are merged there (small point sets:
 * split by tree).  The forest is the single-GPU forest whatever the number of ranks.  Per NN-descent iteration
 *   (1) all-gather of the thresholds, 4 bytes per row, and -- while the lists still change much -- of the neighbour ids;
 *   (2) reverse-offer all-to-all-v of 8-byte records (the cross-process form of the ownership test utils.py:266-273);
 *   (3) local sampling + join of the owned vertices; (4) proposal all-to-all-v of 12-byte records, owner-side merge
 *   (utils.py:721-731); the update counts of all ranks (stop rule, pynndescent_.py:317) ride on the record-count exchange.
 * The whole per-rank build runs inside the library (csrc/shard.hip) on one HIP stream; the exchanges are issued from
 * the C side on that stream -- ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd (RCCL) -- so kernels and collectives
 * need no host synchronisation between them; the host waits twice per iteration, for the record counts.
 *
 * Communicators.  One per rank.  RCCL: rank 0 calls nnd_comm_unique_id, the launcher hands the 128 bytes to the other
 * ranks (any side channel), every rank calls nnd_comm_create_rccl.  LOCAL: world ranks as threads of ONE process that
 * may share a GPU (tests, nnd_build_multi with repeated device ids).  HOST: device buffers staged through pinned host
 * memory and exchanged by a caller-supplied callback (debugging transport; gloo in the tests). */
typedef struct nnd_comm_s *nnd_comm_t;
#define NND_COMM_ID_BYTES 128
int32_t nnd_comm_unique_id(void *id_out /* NND_COMM_ID_BYTES */);
int32_t nnd_comm_create_rccl(nnd_comm_t *out, const void *id, int32_t world, int32_t rank, int32_t device);
int32_t nnd_comm_create_local(nnd_comm_t *out /* [world] */, int32_t world, const int32_t *devices /* [world], NULL: all 0 */);
/* all-to-all-v on HOST memory: byte segment [send_off[d], + send_bytes[d]) of `send` goes to rank d; what rank s sends
 * arrives at recv + recv_off[s] (recv_bytes[s] bytes, known to the receiver).  Returns 0 on success. */
typedef int32_t (*nnd_host_exchange_fn)(void *user, const void *send, const int64_t *send_off, const int64_t *send_bytes,
                                        void *recv, const int64_t *recv_off, const int64_t *recv_bytes);
int32_t nnd_comm_create_host(nnd_comm_t *out, int32_t world, int32_t rank, int32_t device, nnd_host_exchange_fn fn, void *user);
/* Second channel of an RCCL communicator (its own ncclComm_t from a second unique id, its own stream): the point-set
 * all-gather runs on it while the build's stream works.  Collective: every rank calls it (or none).  LOCAL communicators
 * are created with theirs; HOST has none (the transfer then runs on the build's channel). */
int32_t nnd_comm_add_channel_rccl(nnd_comm_t c, const void *id /* a second id from nnd_comm_unique_id */);
/* Failure handling.  Every host wait of a build polls the communicator: a rank whose peer failed (ranks of one process
 * share a flag: LOCAL, nnd_build_multi) or that has waited longer than the timeout (default 120 s; the only signal
 * between processes) gives up -- ncclCommAbort on its communicators, error return -- instead of blocking in a collective
 * for ever.  nnd_comm_abort makes THIS rank give up (and tells the ranks of its process). */
int32_t nnd_comm_set_timeout(nnd_comm_t c, int64_t timeout_ms);
int32_t nnd_comm_destroy(nnd_comm_t c);
int32_t nnd_comm_abort(nnd_comm_t c);
/* out[0] transport (1 RCCL, 2 LOCAL, 3 HOST), out[1] ranks, out[2] ncclGetVersion() (0 unless RCCL), out[3] second channel present */
int32_t nnd_comm_info(nnd_comm_t c, int32_t *out /* [4] */);
/* Collective (every rank of the world calls it): each rank sends its rank number to every other rank through the transport's
 * ordinary exchange and checks what arrived -- the exchange nnd_comm_create_rccl / nnd_comm_add_channel_rccl end with.
 * RCCL and LOCAL transports; 0 = every pair of ranks moved its bytes (both channels). */
int32_t nnd_comm_self_test(nnd_comm_t c);
/* LOCAL only: compute sections of the ranks run one at a time (per-rank timings on a shared GPU; tools/rank_critical_path.py) */
int32_t nnd_comm_local_set_serial(nnd_comm_t c, int32_t on);
const char *nnd_comm_last_error(nnd_comm_t c /* NULL: the error of a failed create */);

/* One rank of a sharded build.  params: n = the GLOBAL point count, n_trees = the GLOBAL tree count, device = this
 * rank's GPU, everything else as for nnd_create (the reference's derived defaults are taken on the global n by the
 * host).  shard_sizes[world]: rows per rank, in rank order (rank r owns the rows after those of ranks < r). */
typedef struct nnd_shard_s *nnd_shard_t;
typedef struct nnd_shard_info {
    int64_t n_total, own_lo, own_hi;
    int32_t world, rank, local_trees, iters;
    int64_t c[64];                /* GLOBAL update count per iteration (the stop rule's c, pynndescent_.py:317) */
    int64_t offer_records[64];    /* reverse-offer records this rank sent to other ranks, per iteration */
    int64_t proposal_records[64]; /* proposal records this rank sent to other ranks, per iteration */
    int64_t deferred[64];         /* proposal records that did not fit their destination's region and were kept for the next iteration */
    int64_t dropped_offers;       /* must stay 0: the offer regions are sized for every owned edge */
    int64_t bytes_sent;           /* payload bytes this rank sent to other ranks during the build */
    float ms_total;               /* this rank's wall time of the last build, exchanges included */
    float ms_allgather, ms_klist_exchange; /* stream time of the two bulk exchanges */
    int32_t n_sections;           /* compute sections of the last build (timeline below) */
    float section_ms[256];        /* LOCAL serial mode: GPU time of each compute section of this rank, in program order */
    int64_t section_bytes[256];   /* payload bytes this rank sent in the exchange that FOLLOWS the section */
    int32_t forest_by_cell;       /* 1: forest sharded by cell, 0: split by tree */
    int32_t n_sections_overlap;   /* the first sections of the build that need only this rank's rows: the point-set all-gather runs beside them */
    int64_t forest_positions;     /* point-trees this rank finished and seeded (forest by cell: ~ n_trees * n / ranks) */
    /* ABI 6: the threshold / neighbour-id all-gather of every iteration runs on the SECOND channel beside the offer exchange and the
     * second half of the sampling (only the join needs what it brings).  gather_bytes[i]: payload this rank sent in it;
     * gather_section[i]: index of the compute section it runs beside (LOCAL serial mode times that section apart; -1: the gather ran on
     * the build's channel, in front of the offer exchange, as it did through round 5) */
    int64_t gather_bytes[64];
    int32_t gather_section[64];
} nnd_shard_info;
int32_t nnd_shard_create(nnd_shard_t *out, const nnd_params *params, nnd_comm_t comm, const int64_t *shard_sizes);
/* x_local_dev: this rank's rows, float32 (n_local, dim) on its GPU, complete when the call is made (or produced on
 * x_stream, which the build then waits for).  Outputs: device buffers (n_local, k): GLOBAL neighbour ids, alt-space
 * distances, rows ascending.  Blocks until this rank's rows are final. */
int32_t nnd_shard_build(nnd_shard_t s, const float *x_local_dev, void *x_stream, int32_t *out_idx_dev, float *out_dist_dev);
/* ... from the rank's OWN rows of an init graph (device (n_own, init_width), global ids; init_dist_dev nullable); the shard must have been
 * created with n_trees = 0 */
int32_t nnd_shard_build_from_graph(nnd_shard_t s, const float *x_local_dev, void *x_stream, const int32_t *init_idx_dev,
                                   const float *init_dist_dev, int32_t init_width, int32_t *out_idx_dev, float *out_dist_dev);
/* ... NNDescent.update() (pynndescent_.py:2498-2535): the rank's rows of the previous graph enter as OLD entries (alt-space distances
 * required) before the fresh forest's leaves are joined; no random fill */
int32_t nnd_shard_build_update(nnd_shard_t s, const float *x_local_dev, void *x_stream, const int32_t *old_idx_dev, const float *old_dist_dev,
                               int32_t width, int32_t *out_idx_dev, float *out_dist_dev);
int32_t nnd_shard_get_info(nnd_shard_t s, nnd_shard_info *out);
int32_t nnd_shard_get_stats(nnd_shard_t s, nnd_stats *out); /* this rank's kernels */
/* the rank's builder handle (tests: nnd_leaf_array_shape / nnd_get_leaf_array give the leaves this rank seeded from) */
nnd_handle_t nnd_shard_handle(nnd_shard_t s);
int32_t nnd_shard_destroy(nnd_shard_t s);
const char *nnd_shard_last_error(nnd_shard_t s /* NULL: the error of a failed create */);

/* nnd_build over n_devices GPUs of this node: host buffers in, host buffers out, one host thread per GPU inside the
 * library (the reference's analogue is n_jobs, pynndescent_.py:1141-1143).  devices: HIP ordinals, NULL = 0..n_devices-1.
 * Distinct ordinals talk over RCCL; a list that repeats an ordinal (several ranks on one GPU: tests on a one-GPU box)
 * uses the LOCAL transport.  Results depend on n_devices as the reference's depend on its thread count.  stats: rank 0's. */
int32_t nnd_build_multi(const nnd_params *params, const float *x, int32_t n_devices, const int32_t *devices, int32_t *out_idx,
                        float *out_dist, nnd_stats *stats, nnd_shard_info *info_rank0 /* nullable */, char *err, int32_t errlen);
/* ... from an init graph (ABI 5): the warm start of NNDescent(init_graph=, init_dist=), pynndescent_.py:1225-1242 /
 * initalize_heap_from_graph_indices[_and_distances], utils.py:836-860 -- init_idx host (n, init_width) GLOBAL ids (-1: empty),
 * init_dist nullable (alt-space distances; computed when NULL).  No forest (an init graph disables it, pynndescent_.py:1059-1062:
 * params->n_trees is taken as 0), no random fill.  Every rank seeds ITS rows from its rows of the init graph. */
int32_t nnd_build_multi_from_graph(const nnd_params *params, const float *x, int32_t n_devices, const int32_t *devices,
                                   const int32_t *init_idx, const float *init_dist, int32_t init_width, int32_t *out_idx, float *out_dist,
                                   nnd_stats *stats, nnd_shard_info *info_rank0 /* nullable */, char *err, int32_t errlen);
/* NNDescent.update() (pynndescent_.py:2381-2553, the rebuild at 2498-2535) over n_devices GPUs: a fresh forest of params->n_trees trees
 * (n_trees_after_update) over the changed point set, the previous graph's surviving entries as OLD entries (init_from_neighbor_graph,
 * pynndescent_.py:206-214; old_idx host (n, width) global ids, -1 where invalidated, old_dist their alt-space distances), no random fill */
int32_t nnd_build_multi_update(const nnd_params *params, const float *x, int32_t n_devices, const int32_t *devices, const int32_t *old_idx,
                               const float *old_dist, int32_t width, int32_t *out_idx, float *out_dist, nnd_stats *stats,
                               nnd_shard_info *info_rank0 /* nullable */, char *err, int32_t errlen);

/* ---- exact k nearest neighbours by brute force (csrc/exact.hip; DESIGN.md "Exact search") ----
 * The companion of the approximate index: ground truth, recall on the caller's own data, small point sets.  Works on any
 * handle whose point set is resident and prepared (nnd_set_data_*): an NND_FLAG_NO_GRAPH handle (the natural one: no k-lists
 * are allocated) or a build handle; fails on NND_FLAG_NO_PREP, for k < 1 and for k > min(n, 256).  Two tiers: an f32 MFMA
 * Gram scan keeps the W >= k best candidates per row, their distances are recomputed from the original rows with float64
 * accumulation (the formulas of nnd_finalize_*), and a row is answered from them only if a rounding-error bound proves that
 * nothing the scan left out can belong to the top k; every other row is scanned again in float64.  The result is the exact
 * top k by (float64 distance, id): rows ascending, ties to the smaller id, float32 alt-space distances. */
typedef struct nnd_exact_stats {
    int64_t n_rows, n_fallback;   /* rows answered / rows that were not certified and went through the float64 scan */
    int64_t pairs, mfma;          /* pair distances and v_mfma_f32_16x16x4_f32 instructions of the scan */
    float ms_scan, ms_refine, ms_fallback;
} nnd_exact_stats;
/* rows of the handle's own point set (host int64 ids, NULL = all n), self included */
int32_t nnd_exact_knn_rows(nnd_handle_t h, const int64_t *rows, int64_t n_rows, int32_t k,
                           int32_t *out_idx, float *out_dist, nnd_exact_stats *st /* may be NULL */);
/* external queries, host float32 (n_q, dim): prepared with the point set's transform (code 0: the SET's column means) */
int32_t nnd_exact_knn_queries(nnd_handle_t h, const float *q, int64_t n_q, int32_t k,
                              int32_t *out_idx, float *out_dist, nnd_exact_stats *st);
/* The two entries above for a caller on the handle's device, on the handle's stream (nnd_set_stream: the caller's).  rows_dev:
 * int32 ids on the device (NULL = all n; an id outside [0, n) is an error, found on the device as the ids enter their batch and reported with that batch).  q_dev: (n_q, dim)
 * queries of `dtype` (NND_DTYPE_*), converted into each batch's own float32 copy (NND_METRIC_ALT_DOT: and L2-normalised, as
 * nnd_set_data_device_typed normalises the rows).  out_idx_dev / out_dist_dev: DEVICE (m, k) arrays, written device to device.
 * All arrays stay the caller's; the call returns with the stream drained (one scalar per batch, the count of uncertified rows,
 * crosses the bus in any case). */
int32_t nnd_exact_knn_rows_device(nnd_handle_t h, const int32_t *rows_dev, int64_t n_rows, int32_t k,
                                  int32_t *out_idx_dev, float *out_dist_dev, nnd_exact_stats *st /* may be NULL */);
int32_t nnd_exact_knn_queries_device(nnd_handle_t h, const void *q_dev, int32_t dtype, int64_t n_q, int32_t k,
                                     int32_t *out_idx_dev, float *out_dist_dev, nnd_exact_stats *st);
/* The four entries above under a predicate per query row (the masked instances of the scan and of the float64 tier): `tags` holds
 * one 64-bit tag word per row of the point set, `masks` one mask word per query row (in the order of rows / q), and data row c
 * belongs to query row i's point set iff tags[c] & masks[i] != 0.  The answer is the exact top k by (float64 distance, id) AMONG
 * THOSE ROWS; a pair that does not meet is neither a candidate nor counted into the certificate's bound.  Fewer than k such rows
 * (a mask of 0: none) leave (-1, +inf) in the last places.  Host forms take host words, device forms words on the handle's device. */
int32_t nnd_exact_knn_rows_tagged(nnd_handle_t h, const int64_t *rows, int64_t n_rows, int32_t k, const uint64_t *tags,
                                  const uint64_t *masks, int32_t *out_idx, float *out_dist, nnd_exact_stats *st /* may be NULL */);
int32_t nnd_exact_knn_queries_tagged(nnd_handle_t h, const float *q, int64_t n_q, int32_t k, const uint64_t *tags,
                                     const uint64_t *masks, int32_t *out_idx, float *out_dist, nnd_exact_stats *st);
int32_t nnd_exact_knn_rows_tagged_device(nnd_handle_t h, const int32_t *rows_dev, int64_t n_rows, int32_t k, const uint64_t *tags_dev,
                                         const uint64_t *masks_dev, int32_t *out_idx_dev, float *out_dist_dev, nnd_exact_stats *st);
int32_t nnd_exact_knn_queries_tagged_device(nnd_handle_t h, const void *q_dev, int32_t dtype, int64_t n_q, int32_t k,
                                            const uint64_t *tags_dev, const uint64_t *masks_dev, int32_t *out_idx_dev,
                                            float *out_dist_dev, nnd_exact_stats *st);
/* data slices the scan splits the point set into when n_rows query rows are asked for (a function of the shapes alone: few
 * query blocks -> many slices, so that the chip is filled); tests */
int32_t nnd_exact_slice_count(nnd_handle_t h, int64_t n_rows);

/* Stream the handle runs on: the caller's HIP stream (e.g. the one that produces the point set) instead of the handle's
 * own, so the device-pointer entry points need no synchronisation with it.  NULL: the handle's own stream again. */
int32_t nnd_set_stream(nnd_handle_t h, void *hip_stream);
/* one descent iteration in two steps (the state between them is what nnd_reset_graph has to clear: tests) */
int32_t nnd_descent_sample(nnd_handle_t h);
int32_t nnd_descent_join(nnd_handle_t h);

/* ---- search-graph pruning pass (BASELINE config 5; reference NNDescent._init_search_graph, pynndescent_.py:1451-1611) ----
 * Host arrays in / out: like the reference, the conversions between these kernels (COO->CSR, transpose, maximum,
 * binarise) are scipy calls on the host. */
typedef struct nnd_prune_opts {
    float prune_probability; /* diversify_prob: an eligible edge is pruned with this probability (pynndescent_.py:388, 582) */
    int32_t degree_aware;    /* 0: diversify / diversify_csr; 1: diversify_degree_aware / diversify_csr_degree_aware */
    int32_t max_degree;      /* degree-aware: the degree above which the threshold is relaxed (pynndescent_.py:1478, 1567) */
    float aggressiveness;    /* degree-aware: degree_prune_aggressiveness */
    float alpha;             /* degree-aware forward pass only (pynndescent_.py:435, 528) */
    uint32_t seed;           /* coin hash seed (the reference draws from NNDescent.rng_state) */
    int32_t reserved[2];
} nnd_prune_opts;
/* diversify (pynndescent_.py:369-403) / diversify_degree_aware (433-546): (n,k) rows ascending in alt space; pruned
 * slots -> (-1, +inf).  opts NULL = the reference defaults (standard method, probability 1).  degree: host int32 (n)
 * undirected degrees (compute_degrees, pynndescent_.py:406-418), required when opts->degree_aware. */
int32_t nnd_diversify_host(nnd_handle_t h, int32_t *idx, float *dist, const nnd_prune_opts *opts, const int32_t *degree);
/* diversify_csr (pynndescent_.py:549-588) / diversify_csr_degree_aware (625-726) on CSR rows of <= 64 entries; pruned
 * entries get weight 0.  degree: host int32 (n) (compute_degrees_csr, pynndescent_.py:591-622) when degree_aware. */
int32_t nnd_diversify_csr_host(nnd_handle_t h, const int32_t *indptr, const int32_t *indices, float *data, int64_t nnz,
                               const nnd_prune_opts *opts, const int32_t *degree);
/* degree_prune_internal (pynndescent_.py:728-738): rows longer than max_degree keep entries <= sorted(row)[max_degree] */
int32_t nnd_degree_prune_host(nnd_handle_t h, const int32_t *indptr, float *data, int64_t nnz, int32_t max_degree);

/* The whole pruning pass of NNDescent._init_search_graph (pynndescent_.py:1451-1611) on the device (csrc/searchgraph.hip):
 * forward diversify -> COO -> CSR -> "reverse" diversify_csr on the shared arrays -> union max(F', F'^T) -> diagonal and zeros
 * dropped -> degree_prune to round(pruning_degree_multiplier * n_neighbors) -> binarise; ONE device-to-host copy at the end.
 * Replaces, besides the three numba kernels above, the scipy glue between them (coo_matrix / tocsr 1527-1537, transpose 1549,
 * maximum 1599, setdiag / eliminate_zeros 1602-1604, `!= 0` 1611).
 * idx / dist: the (n, k) neighbour graph (k = the handle's n_neighbors; rows ascending in alt space, -1 / +inf padded), on the
 * host (on_device = 0) or on the handle's device (1); not modified.  The handle must hold the point set (nnd_set_data_*): an
 * NND_FLAG_NO_GRAPH handle, or the handle that built the graph (no second upload of the rows).  fwd_rows / fwd_dist: optional
 * host (n, k) arrays that receive the graph after the forward pass (the `stages` view of the tests), or NULL. */
typedef struct nnd_search_graph_stats {
    int64_t forward_nnz;   /* edges after the forward pass */
    int64_t reverse_nnz;   /* ... after the second pass (the reference's reverse_graph.nnz; = the forward matrix's, shared arrays) */
    int64_t union_nnz;     /* entries of max(F', F'^T) without the diagonal */
    int64_t final_nnz;     /* entries of the search graph */
    float min_distance;    /* NNDescent._min_distance (pynndescent_.py:1539) */
    int32_t max_degree_out;
    float ms_device;       /* stream time of the pass, copies of the graph in included */
    int32_t reserved[3];
} nnd_search_graph_stats;
int32_t nnd_search_graph(nnd_handle_t h, const int32_t *idx, const float *dist, int32_t on_device, int32_t n_neighbors,
                         float pruning_degree_multiplier, float diversify_prob, int32_t degree_aware, float degree_prune_aggressiveness,
                         uint32_t seed, int32_t *fwd_rows_host, float *fwd_dist_host, nnd_search_graph_stats *stats);
/* the finished search graph of the last nnd_search_graph call: CSR pattern, indptr (n + 1), indices (final_nnz) sorted by column */
int32_t nnd_search_graph_fetch(nnd_handle_t h, int32_t *indptr_host, int32_t *indices_host);

/* ---- hub search tree of NNDescent.prepare() (reference rp_trees.py:714-1312 make_hub_tree and its splits,
 * rp_trees.py:2926-3049 convert_tree_format) ----
 * Built level-synchronously on the device from the ORIGINAL rows (nnd_set_data_*; the handle must have been created
 * with n_trees >= 1: the builder borrows the forest's scan / scatter buffers) and the finished graph's in-degrees:
 * rank_order = the point ids sorted by (-in-degree, id) (compute_global_degrees, rp_trees.py:714-744, is a bincount of
 * the neighbour array; the order is host glue).  Angular splits when the handle's metric is one of the angular codes (1, 2, 4, 5).
 * Result: the reference's FlatTree in pre-order numbering: hyperplanes (n_nodes, dim), offsets (n_nodes),
 * children (n_nodes, 2) [internal: child node ids; leaf: (-leaf_start, -leaf_end) into indices], indices (n). */
int32_t nnd_hub_tree_build(nnd_handle_t h, const int32_t *rank_order_host, int32_t leaf_size, int32_t max_depth,
                           int64_t *n_nodes_out);
int32_t nnd_hub_tree_fetch(nnd_handle_t h, float *hyperplanes, float *offsets, int32_t *children, int32_t *indices,
                           int32_t *max_leaf_size);

/* ---- prepare() of an index whose rows and graph live on the device (csrc/prepare.hip; DESIGN.md "Device arrays") ----
 * The glue between the hub tree, the pruning pass and the searcher, so that neither the rows nor the graph visit the host.
 * The entries without a handle take a device ordinal and a HIP stream (NULL: the device's default stream), queue their kernels
 * there and return when the stream has drained (their scratch buffers are released on return).
 *
 * nnd_rank_order_device: the hub tree's rank order from a device graph.  idx_dev: int32 (n, k) neighbour ids; ids < 0 and
 * ids >= n are skipped (compute_global_degrees, rp_trees.py:714-744).  rank_order_dev (n): the point ids sorted by
 * (-in-degree, id) -- numpy.argsort(-degree, kind="stable") entry for entry: one radix sort of the packed keys
 * (0xFFFFFFFF - degree) << 32 | id. */
int32_t nnd_rank_order_device(int32_t device, void *hip_stream, const int32_t *idx_dev, int64_t n, int32_t k, int32_t *rank_order_dev);
/* nnd_hub_tree_build with the rank order on the handle's device (read on the handle's stream); everything else as there */
int32_t nnd_hub_tree_build_device(nnd_handle_t h, const int32_t *rank_order_dev, int32_t leaf_size, int32_t max_depth,
                                  int64_t *n_nodes_out);
/* The finished search graph of the last nnd_search_graph call where it lies: device addresses of indptr (n + 1) and indices
 * (final_nnz) in the handle's workspace, valid until the next pass on the handle or its nnd_destroy.  No copy is made. */
int32_t nnd_search_graph_device(nnd_handle_t h, const int32_t **indptr_dev, const int32_t **indices_dev, int64_t *nnz);
/* The tail of _init_search_graph (pynndescent_.py:1629-1651) for the graph: rows and columns of a CSR pattern (indptr (n + 1),
 * indices (nnz), rows of at most 384 entries, columns in [0, n)) in the order `order_dev` (n, a permutation of [0, n): new row i
 * is old row order[i], column j becomes the position of j in `order`), columns ascending within a row -- scipy's
 * g[order, :].tocsc()[:, order].tocsr() with sort_indices().  order_dev NULL: the identity, the graph is copied as it is.
 * Outputs: indptr_out_dev (n + 1), indices_out_dev (nnz).  One wave per row. */
int32_t nnd_reorder_csr_device(int32_t device, void *hip_stream, const int32_t *order_dev, int64_t n, const int32_t *indptr_dev,
                               const int32_t *indices_dev, int64_t nnz, int32_t *indptr_out_dev, int32_t *indices_out_dev);
/* The same, and the rows' gather, on host arrays staged through the device (tests: row shapes no small index produces).
 * x: float32 (n, dim); x_out: (n, dp) with dp = (dim + 3) & ~3, row i = x[order[i]] followed by dp - dim zeros -- the
 * searcher's padded layout.  order NULL: the identity. */
int32_t nnd_reorder_host(int32_t device, int64_t n, int32_t dim, const int32_t *order, const int32_t *indptr, const int32_t *indices,
                         int64_t nnz, const float *x, int32_t *indptr_out, int32_t *indices_out, float *x_out);

/* ---- batched queries against a prepared index (reference NNDescent.query, pynndescent_.py:2275-2379: the search
 * closure of _init_search_function 1793-1883, select_side / search_flat_tree rp_trees.py:2662-2741, deheap_sort) ----
 * The searcher owns device copies of what the reference's closure captures: the (reordered) raw data, the CSR search
 * graph, the FlatTree of the search forest's first tree (n_nodes = 0: no tree, random starts only), min_distance and
 * n_neighbors.  All pointers are HOST pointers.  One wave per query; k <= 256 (the query's k, not the index's; above 64 the result list is two or four entries per lane).  Output rows ascending in the
 * alternative distance space, vertex numbers in the searcher's (reordered) numbering; unfilled slots (-1, +inf). */
typedef struct nnd_searcher_s *nnd_searcher_t;
int32_t nnd_searcher_create(nnd_searcher_t *out, int32_t device, int64_t n, int32_t dim, int32_t metric, const float *data,
                            const int32_t *indptr, const int32_t *indices, int64_t nnz, const float *hyperplanes,
                            const float *offsets, const int32_t *children, const int32_t *tree_indices, int64_t n_nodes,
                            float min_distance, int32_t n_neighbors, const int64_t *search_rng_state /* 3 */);
/* The same searcher filled from device memory, on `hip_stream` (NULL: the device's default stream) of `device`.  rows_dev: the
 * point set, (n, dim) rows of `dtype` (NND_DTYPE_*) in their ORIGINAL order; order_dev (n, device; NULL: the identity): row i of
 * the searcher is row order[i] of rows_dev, converted to float32 and written straight into the padded layout (dp floats, zero
 * fill).  indptr_dev / indices_dev: the CSR graph in the searcher's numbering (nnd_reorder_csr_device), copied device to
 * device.  The tree tables are HOST pointers as above (tree_indices in the searcher's numbering).  The caller's buffers are
 * free again when the call returns (the stream has drained). */
int32_t nnd_searcher_create_device(nnd_searcher_t *out, int32_t device, int64_t n, int32_t dim, int32_t metric, const void *rows_dev,
                                   int32_t dtype, const int32_t *order_dev, const int32_t *indptr_dev, const int32_t *indices_dev,
                                   int64_t nnz, const float *hyperplanes, const float *offsets, const int32_t *children,
                                   const int32_t *tree_indices, int64_t n_nodes, float min_distance, int32_t n_neighbors,
                                   const int64_t *search_rng_state /* 3 */, void *hip_stream);
int32_t nnd_searcher_query(nnd_searcher_t s, const float *queries /* (nq, dim) */, int64_t nq, int32_t k, float epsilon,
                           int32_t *out_idx /* (nq, k) */, float *out_dist /* (nq, k) */);
/* The search runs in two tiers: per-query LDS structures (3400 visited vertices, 512 frontier entries) and, for exactly
 * the queries that would overflow them (large k / epsilon, oversized tree leaves), a global-memory tier with the
 * reference's own structures (visited bitset over all n points, utils.py:323-349; frontier of 65536 entries).  No answer
 * comes from a truncated search.  nnd_searcher_last_spilled: queries of the last call that ran on the second tier;
 * nnd_searcher_set_tier(s, 1) sends every query there (tests), 0 = automatic. */
int64_t nnd_searcher_last_spilled(nnd_searcher_t s);
int32_t nnd_searcher_set_tier(nnd_searcher_t s, int32_t tier);
/* quantization="uint8" (reference prepare() / query(), pynndescent_.py:2191-2225, 2309-2364; metrics sqeuclidean, alt
 * cosine, alt dot).  nnd_searcher_quantize_u8: codes = np.searchsorted(values, rows).astype(np.uint8) on the device (a value
 * above the last entry gets n_values; 256 wraps to 0), values ascending, 1 <= n_values <= 256.  rows: (n, dim) host rows in
 * the searcher's order, or NULL to quantize the searcher's own copy (dot: that copy is normalised again on the device, so
 * hand in the rows whose codes are wanted).  codes_out (n, dim) may be NULL.  nnd_searcher_set_codes_u8: the same state from
 * codes computed before (an unpickled index).  nnd_searcher_query_proxy: the walk on the codes with the proxy distances keeps
 * search_k results (1 <= k <= search_k <= 256), then reranks them by the exact distance of the raw query to the float rows
 * and returns the k best, (nq, k), ascending, as nnd_searcher_query. */
int32_t nnd_searcher_quantize_u8(nnd_searcher_t s, const float *rows /* may be NULL */, const float *values, int32_t n_values,
                                 uint8_t *codes_out /* may be NULL */);
int32_t nnd_searcher_set_codes_u8(nnd_searcher_t s, const float *values, int32_t n_values, const uint8_t *codes /* (n, dim) */);
int32_t nnd_searcher_query_proxy(nnd_searcher_t s, const float *queries /* (nq, dim) */, int64_t nq, int32_t k, int32_t search_k,
                                 float epsilon, int32_t *out_idx /* (nq, k) */, float *out_dist /* (nq, k) */);
/* metric="proxy_inner_product" (reference query(), pynndescent_.py:2309-2312, 2363-2371; rerank 776-789).  Valid on a searcher
 * whose metric has a true distance besides the one it walks on (NND_METRIC_PROXY_INNER_PRODUCT), an error on every other.  The
 * walk on the float rows with the proxy distance keeps search_k results (1 <= k <= search_k <= 256); they are pushed in ascending
 * proxy order, by the true distance -<q,x> of the raw query, into a list of k.  Output (nq, k): rows ascending in -<q,x> (float32
 * accumulation, neither clamped nor corrected), unfilled slots (-1, +inf).  A zero query is searched like any other. */
int32_t nnd_searcher_query_rerank(nnd_searcher_t s, const float *queries /* (nq, dim) */, int64_t nq, int32_t k, int32_t search_k,
                                  float epsilon, int32_t *out_idx /* (nq, k) */, float *out_dist /* (nq, k) */);
/* The three query entries for a caller on the device: queries (float32, C-contiguous), out_idx and out_dist are DEVICE pointers
 * on the searcher's device, neither copy is made, and the kernels run on `hip_stream` (NULL: the device's default stream) -- the
 * stream that produced the queries, so that nothing has to be synchronised first.  The call returns when the stream has
 * drained (the walk's overflow flags are read back in any case).  Everything else is as in the host forms. */
int32_t nnd_searcher_query_device(nnd_searcher_t s, const float *queries_dev, int64_t nq, int32_t k, float epsilon,
                                  int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream);
int32_t nnd_searcher_query_proxy_device(nnd_searcher_t s, const float *queries_dev, int64_t nq, int32_t k, int32_t search_k,
                                        float epsilon, int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream);
int32_t nnd_searcher_query_rerank_device(nnd_searcher_t s, const float *queries_dev, int64_t nq, int32_t k, int32_t search_k,
                                         float epsilon, int32_t *out_idx_dev, float *out_dist_dev, void *hip_stream);
/* Filtered queries (beyond the reference): an allow set, one for all queries of a call.  The filter is STATE of the searcher: once
 * set, every query entry above (host and device forms, float / proxy / rerank) runs its filtered kernel instance until
 * nnd_searcher_clear_filter or the next nnd_searcher_set_filter*; a searcher without a filter launches exactly the kernels it
 * launched before.  The rule of the filtered walk: a vertex enters the walk's result list only if it is allowed.  It is still
 * visited, pushed to the frontier and expanded, so the bound (taken from the allowed-only list, +inf while that is short), the
 * stop rule and the hand-over to the global-memory tier are unchanged; the proxy / rerank entries rerank search_k allowed
 * candidates.  Unfilled slots (-1, +inf).
 *   kind NND_FILTER_MASK: `filter` is one byte per row (count == n), non-zero = allowed;
 *   kind NND_FILTER_IDS:  `filter` is `count` int64 row ids (duplicates are fine); an id outside 0 .. n - 1 is reported by the
 *                         return value 2, nothing is written for it and the searcher is left without a filter.
 * Mask and ids are in the ORIGINAL row numbering; `order` (n, int32; NULL: the identity) is the searcher's row order, row i of
 * the searcher being original row order[i] -- the bitset the kernels read (32 rows per word) is in the searcher's numbering.
 * n_allowed (may be NULL): the number of allowed rows.  The host form copies filter and order to the device and runs on the
 * searcher's stream; the device form reads device pointers on `hip_stream` (NULL: the default stream).  Both return when the
 * stream has drained, so the caller's buffers are free again.  Returns 0, 1 (error) or 2 (id out of range). */
#define NND_FILTER_MASK 0
#define NND_FILTER_IDS 1
int32_t nnd_searcher_set_filter(nnd_searcher_t s, const void *filter, int64_t count, int32_t kind, const int32_t *order /* may be NULL */,
                                int64_t *n_allowed /* may be NULL */);
int32_t nnd_searcher_set_filter_device(nnd_searcher_t s, const void *filter_dev, int64_t count, int32_t kind,
                                       const int32_t *order_dev /* may be NULL */, int64_t *n_allowed /* may be NULL */, void *hip_stream);
int32_t nnd_searcher_clear_filter(nnd_searcher_t s);
/* Per-query filters (beyond the reference): every row may carry a tag word (64 bits, one per tag), every query of a call a mask
 * word; row r may be returned to query i iff tags[r] & masks[i] != 0.  A row with tag word 0 is never returned, a query with
 * mask 0 gets (-1, +inf) in every place.  The tag words are STATE of the searcher (its own copy, n x 8 bytes, in the searcher's
 * numbering: `tags` is in the ORIGINAL numbering and gathered through `order` as for the filter above); the masks come with the
 * call.  nnd_searcher_query_tagged* is the walk of the query entries above with the filter's rule per query -- a vertex enters the
 * result list only if its tag word meets the query's mask; it is still visited and expanded -- for the three forms: NND_QUERY_FLOAT
 * (nnd_searcher_query; search_k is ignored), NND_QUERY_PROXY (nnd_searcher_query_proxy) and NND_QUERY_RERANK
 * (nnd_searcher_query_rerank).  It fails without tags and while a filter is set (the two do not combine).
 * nnd_searcher_count_tags*: counts[u] = rows whose tag word meets masks[u], one pass over the tag words for all n_masks masks.
 * Host forms copy their arrays and run on the searcher's stream, device forms read and write device memory on `hip_stream`; all
 * return with the stream drained.  nnd_searcher_clear_tags releases the searcher's copy. */
#define NND_QUERY_FLOAT 0
#define NND_QUERY_PROXY 1
#define NND_QUERY_RERANK 2
int32_t nnd_searcher_set_tags(nnd_searcher_t s, const uint64_t *tags /* (n) */, const int32_t *order /* may be NULL */);
int32_t nnd_searcher_set_tags_device(nnd_searcher_t s, const uint64_t *tags_dev, const int32_t *order_dev /* may be NULL */, void *hip_stream);
int32_t nnd_searcher_clear_tags(nnd_searcher_t s);
int32_t nnd_searcher_count_tags(nnd_searcher_t s, const uint64_t *masks, int32_t n_masks, int64_t *counts);
int32_t nnd_searcher_count_tags_device(nnd_searcher_t s, const uint64_t *masks_dev, int32_t n_masks, int64_t *counts_dev, void *hip_stream);
int32_t nnd_searcher_query_tagged(nnd_searcher_t s, int32_t form, const float *queries, int64_t nq, int32_t k, int32_t search_k,
                                  float epsilon, const uint64_t *masks /* (nq) */, int32_t *out_idx, float *out_dist);
int32_t nnd_searcher_query_tagged_device(nnd_searcher_t s, int32_t form, const float *queries_dev, int64_t nq, int32_t k, int32_t search_k,
                                         float epsilon, const uint64_t *masks_dev, int32_t *out_idx_dev, float *out_dist_dev,
                                         void *hip_stream);
int32_t nnd_searcher_destroy(nnd_searcher_t s);
const char *nnd_searcher_last_error(nnd_searcher_t s /* NULL: the error of a failed create */);

/* ---- graph export: k-lists to canonical CSR on the device (csrc/csr_graph.hip; DESIGN.md "Graph export") ----
 * ids: (m, k) int32 or int64 (id_bytes 4 or 8), vals: float32 (m, k), k <= 256; a place whose id is -1 -- or anything else
 * outside [0, n) -- is empty.  A row must not hold one id twice.  Result: the (m, n) matrix in CSR form -- indptr int64
 * (m + 1), indices int32 (nnz), data float32 (nnz), columns strictly ascending in every row: scipy's coo.tocsr() +
 * sum_duplicates().  mode: NND_CSR_DISTANCE keeps the values, NND_CSR_CONNECTIVITY stores 1.0f; | NND_CSR_DROP_SELF drops
 * the places (i, i).  symmetric (m == n only): the union of the matrix and its transpose; an entry present on both sides
 * holds the smaller of the two floats, so the result does not depend on the order the device found the edges in.
 * A row whose k places and reverse edges together are more than 512 (a hub) is merged by a workgroup in global memory, the
 * others by one wave in registers; long_rows counts the former.
 *
 * nnd_graph_csr_device: device pointers, row stride ld >= k elements, on `hip_stream` (NULL: the device's default stream) of
 * `device`; returns with the stream drained.  The arrays belong to the nnd_csr_t: nnd_csr_arrays hands out their device
 * addresses and nnz (any out pointer may be NULL), nnd_csr_destroy frees them.
 * nnd_graph_csr: the same on host arrays (contiguous rows); indices / data have room for `capacity` entries -- m * k always
 * suffices for the directed form, 2 * m * k for the symmetric one; *nnz is set even when the room does not suffice. */
#define NND_CSR_DISTANCE 0
#define NND_CSR_CONNECTIVITY 1
#define NND_CSR_DROP_SELF 2
typedef struct nnd_csr_s *nnd_csr_t;
int32_t nnd_graph_csr_device(int32_t device, void *hip_stream, const void *ids_dev, int32_t id_bytes, const float *vals_dev, int64_t m,
                             int32_t k, int64_t ld, int64_t n, int32_t mode, int32_t symmetric, nnd_csr_t *out);
int32_t nnd_csr_arrays(nnd_csr_t g, const int64_t **indptr_dev, const int32_t **indices_dev, const float **data_dev, int64_t *nnz,
                       int64_t *long_rows);
int32_t nnd_csr_destroy(nnd_csr_t g);
int32_t nnd_graph_csr(int32_t device, const void *ids, int32_t id_bytes, const float *vals, int64_t m, int32_t k, int64_t n, int32_t mode,
                      int32_t symmetric, int64_t *indptr, int32_t *indices, float *data, int64_t capacity, int64_t *nnz, int64_t *long_rows);

#ifdef __cplusplus
}
#endif
#endif /* PYNND_AMD_H */
