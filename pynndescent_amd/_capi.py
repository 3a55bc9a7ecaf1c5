"""ctypes binding of libpynnd_amd.so (include/pynnd_amd.h).

This is the whole FFI: plain pointers and sizes, no torch types.  The library is built in-tree by
``__graft_entry__.build()`` / ``make -C pynndescent_amd/csrc``; if it is missing or no gfx950 device
is present the build path fails loudly -- there is no CPU fallback."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PYNND_AMD_LIB", os.path.join(_HERE, "libpynnd_amd.so"))  # override: A/B experiments only

NND_METRIC_SQEUCLIDEAN = 0
NND_METRIC_ALT_COSINE = 1
NND_METRIC_ALT_DOT = 2
NND_METRIC_ALT_INNER_PRODUCT = 3
NND_METRIC_CORRELATION = 4
NND_METRIC_ALT_HELLINGER = 5
NND_METRIC_PROXY_INNER_PRODUCT = 6
# the reference's metric names on this path -> the space the kernels work in ("sqeuclidean" and "correlation" are that space
# itself: no correction, distances.py named_distances / fast_distance_alternatives)
METRIC_CODES = {"euclidean": NND_METRIC_SQEUCLIDEAN, "l2": NND_METRIC_SQEUCLIDEAN, "sqeuclidean": NND_METRIC_SQEUCLIDEAN,
                "cosine": NND_METRIC_ALT_COSINE, "dot": NND_METRIC_ALT_DOT, "inner_product": NND_METRIC_ALT_INNER_PRODUCT,
                "correlation": NND_METRIC_CORRELATION, "hellinger": NND_METRIC_ALT_HELLINGER,
                "proxy_inner_product": NND_METRIC_PROXY_INNER_PRODUCT}
# the boolean family (include/pynnd_amd.h: an enumeration of its own): name -> code, in the header's order
(NND_METRIC_JACCARD, NND_METRIC_DICE, NND_METRIC_SOKALSNEATH, NND_METRIC_MATCHING, NND_METRIC_ROGERSTANIMOTO,
 NND_METRIC_SOKALMICHENER, NND_METRIC_KULSINSKI, NND_METRIC_RUSSELLRAO, NND_METRIC_YULE) = range(8, 17)
BOOLEAN_METRIC_CODES = {"jaccard": NND_METRIC_JACCARD, "dice": NND_METRIC_DICE, "sokalsneath": NND_METRIC_SOKALSNEATH,
                        "matching": NND_METRIC_MATCHING, "rogerstanimoto": NND_METRIC_ROGERSTANIMOTO,
                        "sokalmichener": NND_METRIC_SOKALMICHENER, "kulsinski": NND_METRIC_KULSINSKI,
                        "russellrao": NND_METRIC_RUSSELLRAO, "yule": NND_METRIC_YULE}


def metric_code(name):
    """The kernels' code of a metric name of either table."""
    return METRIC_CODES[name] if name in METRIC_CODES else BOOLEAN_METRIC_CODES[name]
# element types of a device array (include/pynnd_amd.h NND_DTYPE_*) and the corrections of nnd_device_correct (NND_CORRECT_*)
NND_DTYPE_FLOAT32, NND_DTYPE_FLOAT16, NND_DTYPE_BFLOAT16, NND_DTYPE_FLOAT64 = 0, 1, 2, 3
NND_FILTER_MASK, NND_FILTER_IDS = 0, 1  # nnd_searcher_set_filter's `kind`
NND_QUERY_FORMS = {"float": 0, "proxy": 1, "rerank": 2}  # nnd_searcher_query_tagged's `form` (NND_QUERY_*)
NND_CORRECT_COPY, NND_CORRECT_SQRT, NND_CORRECT_ALT_COSINE, NND_CORRECT_ALT_INNER_PRODUCT, NND_CORRECT_ALT_HELLINGER = 0, 1, 2, 3, 4
NND_CORRECT_HAVERSINE = 5
NND_LINEAR_DIAGONAL, NND_LINEAR_DENSE = 0, 1  # the kinds of a metric's linear map (include/pynnd_amd.h NND_LINEAR_*, csrc/linear.hip)
NND_CSR_DISTANCE, NND_CSR_CONNECTIVITY, NND_CSR_DROP_SELF = 0, 1, 2  # nnd_graph_csr's `mode` (csrc/csr_graph.hip); DROP_SELF is or-ed in
CSR_MAX_K = 256  # the widest k-list nnd_graph_csr takes (csrc/csr_graph.hip CSR_REG_CAP)
NND_ROWMAP_RANK, NND_ROWMAP_SPHERE = 0, 1  # the kinds of a derived metric's row map (include/pynnd_amd.h NND_ROWMAP_*, csrc/rowmap.hip)
ROWMAP_RANK_MAX_DIM = 16384  # the widest row nnd_device_map_rows ranks (csrc/rowmap.hip RM_RANK_MAX)
NND_FLAG_NO_GRAPH = 1  # auxiliary handle: no k-lists / candidate / proposal tables (pruning pass, hub tree)
NND_FLAG_NO_PREP = 2   # ... and no prepared copy of the rows (hub tree only)
NND_FLAG_TEST_SELECT_WAVE = 4  # test hook: the one-wave-per-vertex selection kernel
NND_FLAG_TEST_SMALL_REGIONS = 8  # test hook (sharded build): tiny proposal regions, so that records are deferred
NND_FLAG_TEST_ROUTE_PLAIN = 16  # test hook: the forest's routing pass as one walk per (tree, point) through global memory
NND_FLAG_TEST_FOREST_BY_TREE = 32  # test hook (sharded build): forest split by tree where it would be sharded by cell
NND_FLAG_TEST_FAIL = 64  # test hook (sharded build): this rank returns an error at the start of its second iteration
NND_FLAG_TEST_VANISH = 128  # ... or returns there without telling anybody (a killed process)
NND_FLAG_TEST_FOREST_FALLBACK_TOPS = 512  # test hook (sharded build): a rank reports that the by-cell forest cannot be built (at the tops)
NND_FLAG_TEST_FOREST_FALLBACK_SHARE = 1024  # ... at the owners' shares; both flags: at the over-long cells
NND_FLAG_TEST_GATHER_INLINE = 8192  # test hook (sharded build): the id / threshold gather on the build's channel instead of the second one
NND_FLAG_TEST_JOIN_UNSTAGED = 16384  # test hook: k_local_join_w with the membership lists read from global memory instead of staged in LDS
NND_FLAG_TEST_SELECT_HALF = 4096  # test hook: the fused selection with 32 lanes per vertex where 16 would do (k <= 16, max_candidates <= 16)
NND_FLAG_TEST_SAMPLE_NOMEM = 2048  # test hook: the sampler's record regions "cannot be allocated": the handle must fall back to the hashed slots
NND_FLAG_TEST_EXACT_F64 = 32768  # test hook: the exact search answers every row through its float64 tier
NND_FLAG_TEST_RANDOM_INIT_ROWWISE = 65536  # test hook: init_random with one wave per row instead of one screening wave per 64 rows
NND_FLAG_TEST_SAMPLE_ATOMIC = 256  # test hook: reverse offers by one global atomicMin per edge (rounds 1-4) instead of the bucketed transposition


class NNDParams(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("dim", C.c_int32),
        ("metric", C.c_int32),
        ("n_neighbors", C.c_int32),
        ("n_trees", C.c_int32),
        ("leaf_size", C.c_int32),
        ("max_depth", C.c_int32),
        ("max_candidates", C.c_int32),
        ("n_iters", C.c_int32),
        ("delta", C.c_float),
        ("rng_state", C.c_int64 * 3),
        ("tree_rng", C.c_int64 * 3),
        ("device", C.c_int32),
        ("join_blocks", C.c_int32),
        ("flags", C.c_int32),
        ("reserved", C.c_int32 * 5),
    ]


class NNDSearchGraphStats(C.Structure):
    _fields_ = [("forward_nnz", C.c_int64), ("reverse_nnz", C.c_int64), ("union_nnz", C.c_int64), ("final_nnz", C.c_int64),
                ("min_distance", C.c_float), ("max_degree_out", C.c_int32), ("ms_device", C.c_float), ("reserved", C.c_int32 * 3)]


class NNDStats(C.Structure):
    _fields_ = [
        ("n_iters_run", C.c_int64),
        ("n_leaves", C.c_int64),
        ("tree_levels", C.c_int64),
        ("leaf_pairs", C.c_int64),
        ("leaf_rows", C.c_int64),
        ("join_pairs", C.c_int64 * 64),
        ("join_rows", C.c_int64 * 64),
        ("join_active", C.c_int64 * 64),
        ("proposals", C.c_int64 * 64),
        ("updates", C.c_int64 * 64),
        ("ms_prep", C.c_float),
        ("ms_forest", C.c_float),
        ("ms_leaf_init", C.c_float),
        ("ms_random_init", C.c_float),
        ("ms_descent", C.c_float),
        ("ms_finalize", C.c_float),
        ("ms_sample", C.c_float * 64),
        ("ms_join", C.c_float * 64),
        ("ms_merge", C.c_float * 64),
        ("join_mfma", C.c_int64 * 64),
        ("leaf_mfma", C.c_int64),
        ("n_cells", C.c_int64),
        ("join_substeps", C.c_int64 * 64),
    ]

    def as_dict(self):
        it = int(self.n_iters_run)
        m = min(it, 64)
        out = {
            "n_iters_run": it, "n_leaves": int(self.n_leaves), "tree_levels": int(self.tree_levels),
            "leaf_pairs": int(self.leaf_pairs), "leaf_rows": int(self.leaf_rows), "leaf_mfma": int(self.leaf_mfma), "n_cells": int(self.n_cells),
        }
        for name in ("join_pairs", "join_rows", "join_active", "proposals", "updates", "join_mfma", "join_substeps"):
            out[name] = [int(v) for v in getattr(self, name)[:m]]
        for name in ("ms_prep", "ms_forest", "ms_leaf_init", "ms_random_init", "ms_descent", "ms_finalize"):
            out[name] = float(getattr(self, name))
        for name in ("ms_sample", "ms_join", "ms_merge"):
            out[name] = [float(v) for v in getattr(self, name)[:m]]
        return out


class NNDShardInfo(C.Structure):
    _fields_ = [
        ("n_total", C.c_int64), ("own_lo", C.c_int64), ("own_hi", C.c_int64),
        ("world", C.c_int32), ("rank", C.c_int32), ("local_trees", C.c_int32), ("iters", C.c_int32),
        ("c", C.c_int64 * 64),
        ("offer_records", C.c_int64 * 64),
        ("proposal_records", C.c_int64 * 64),
        ("deferred", C.c_int64 * 64),
        ("dropped_offers", C.c_int64),
        ("bytes_sent", C.c_int64),
        ("ms_total", C.c_float), ("ms_allgather", C.c_float), ("ms_klist_exchange", C.c_float),
        ("n_sections", C.c_int32),
        ("section_ms", C.c_float * 256),
        ("section_bytes", C.c_int64 * 256),
        ("forest_by_cell", C.c_int32),
        ("n_sections_overlap", C.c_int32),
        ("forest_positions", C.c_int64),
        ("gather_bytes", C.c_int64 * 64),
        ("gather_section", C.c_int32 * 64),
    ]

    def as_dict(self):
        it = min(int(self.iters), 64)
        ns = int(self.n_sections)
        return {"n_total": int(self.n_total), "range": (int(self.own_lo), int(self.own_hi)), "world": int(self.world),
                "rank": int(self.rank), "local_trees": int(self.local_trees), "iters": int(self.iters),
                "c": [int(v) for v in self.c[:it]], "offer_records": [int(v) for v in self.offer_records[:it]],
                "proposal_records": [int(v) for v in self.proposal_records[:it]],
                "exchanged_records": [int(a) + int(b) for a, b in zip(self.offer_records[:it], self.proposal_records[:it])],
                "deferred": [int(v) for v in self.deferred[:it]], "dropped_offers": int(self.dropped_offers),
                "bytes_sent": int(self.bytes_sent), "ms_total": float(self.ms_total),
                "ms_allgather": float(self.ms_allgather), "ms_klist_exchange": float(self.ms_klist_exchange),
                "section_ms": [float(v) for v in self.section_ms[:ns]],
                "section_bytes": [int(v) for v in self.section_bytes[:ns]],
                "forest_by_cell": bool(self.forest_by_cell), "n_sections_overlap": int(self.n_sections_overlap),
                "forest_positions": int(self.forest_positions),
                "gather_bytes": [int(v) for v in self.gather_bytes[:it]], "gather_section": [int(v) for v in self.gather_section[:it]]}


HOST_EXCHANGE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p,
                               C.POINTER(C.c_int64), C.POINTER(C.c_int64))


class NNDExactStats(C.Structure):
    _fields_ = [
        ("n_rows", C.c_int64),
        ("n_fallback", C.c_int64),
        ("pairs", C.c_int64),
        ("mfma", C.c_int64),
        ("ms_scan", C.c_float),
        ("ms_refine", C.c_float),
        ("ms_fallback", C.c_float),
    ]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class NNDPruneOpts(C.Structure):
    _fields_ = [
        ("prune_probability", C.c_float),
        ("degree_aware", C.c_int32),
        ("max_degree", C.c_int32),
        ("aggressiveness", C.c_float),
        ("alpha", C.c_float),
        ("seed", C.c_uint32),
        ("reserved", C.c_int32 * 2),
    ]


# every symbol include/pynnd_amd.h declares: (name, restype, argtypes)
_H = C.c_void_p
_SIGNATURES = [
    ("nnd_abi_version", C.c_int32, []),
    ("nnd_last_global_error", C.c_char_p, []),
    ("nnd_last_error", C.c_char_p, [_H]),
    ("nnd_create", C.c_int32, [C.POINTER(_H), C.POINTER(NNDParams)]),
    ("nnd_destroy", C.c_int32, [_H]),
    ("nnd_set_data_host", C.c_int32, [_H, C.c_void_p]),
    ("nnd_set_data_device", C.c_int32, [_H, C.c_void_p]),
    ("nnd_set_data_device_typed", C.c_int32, [_H, C.c_void_p, C.c_int32]),
    ("nnd_device_rows_f32", C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    ("nnd_device_csr_rows", C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32,
                                        C.c_void_p]),
    ("nnd_device_correct", C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64]),
    ("nnd_device_linear_rows", C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("nnd_linear_rows_host", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("nnd_device_map_rows", C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("nnd_map_rows_host", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("nnd_device_update_rows", C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int32, C.c_int64,
                                           C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32]),
    ("nnd_device_update_graph", C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nnd_device_recall_hits", C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                           C.c_void_p]),
    ("nnd_data_nonfinite", C.c_int32, [_H, C.POINTER(C.c_int32)]),
    ("nnd_data_negative", C.c_int32, [_H, C.POINTER(C.c_int32)]),
    ("nnd_release_pending", C.c_int32, []),
    ("nnd_host_copy", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("nnd_host_sqrt_f32", C.c_int32, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("nnd_host_alloc", C.c_void_p, [C.c_int64]),
    ("nnd_host_free", C.c_int32, [C.c_void_p]),
    ("nnd_make_forest", C.c_int32, [_H]),
    ("nnd_leaf_array_shape", C.c_int32, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    ("nnd_get_leaf_array", C.c_int32, [_H, C.c_void_p]),
    ("nnd_reset_graph", C.c_int32, [_H]),
    ("nnd_init_from_leaves", C.c_int32, [_H]),
    ("nnd_init_from_leaf_array", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32]),
    ("nnd_init_random", C.c_int32, [_H]),
    ("nnd_init_from_graph", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_int32]),
    ("nnd_init_from_neighbor_graph", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_int32]),
    ("nnd_init_from_graph_device", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_int32]),
    ("nnd_init_from_neighbor_graph_device", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_int32]),
    ("nnd_descent_iter", C.c_int32, [_H, C.POINTER(C.c_int64)]),
    ("nnd_descent", C.c_int32, [_H]),
    ("nnd_finalize_host", C.c_int32, [_H, C.c_void_p, C.c_void_p]),
    ("nnd_finalize_device", C.c_int32, [_H, C.c_void_p, C.c_void_p]),
    ("nnd_build_device", C.c_int32, [_H, C.c_void_p, C.c_void_p]),
    ("nnd_build", C.c_int32, [C.POINTER(NNDParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                              C.c_void_p, C.POINTER(NNDStats), C.c_char_p, C.c_int32]),
    ("nnd_get_stats", C.c_int32, [_H, C.POINTER(NNDStats)]),
    ("nnd_synchronize", C.c_int32, [_H]),
    ("nnd_get_graph", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nnd_get_candidates", C.c_int32, [_H, C.c_void_p, C.c_void_p]),
    ("nnd_sample_candidates", C.c_int32, [_H]),
    ("nnd_pairwise_gram", C.c_int32, [_H, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    ("nnd_exact_knn_rows", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(NNDExactStats)]),
    ("nnd_exact_knn_queries", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(NNDExactStats)]),
    ("nnd_exact_knn_rows_device", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(NNDExactStats)]),
    ("nnd_exact_knn_queries_device", C.c_int32, [_H, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                                 C.POINTER(NNDExactStats)]),
    ("nnd_exact_slice_count", C.c_int32, [_H, C.c_int64]),
    ("nnd_descent_sample", C.c_int32, [_H]),
    ("nnd_descent_join", C.c_int32, [_H]),
    ("nnd_set_stream", C.c_int32, [_H, C.c_void_p]),
    ("nnd_comm_unique_id", C.c_int32, [C.c_void_p]),
    ("nnd_comm_create_rccl", C.c_int32, [C.POINTER(_H), C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    ("nnd_comm_create_local", C.c_int32, [C.POINTER(_H), C.c_int32, C.c_void_p]),
    ("nnd_comm_create_host", C.c_int32, [C.POINTER(_H), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    ("nnd_comm_add_channel_rccl", C.c_int32, [_H, C.c_void_p]),
    ("nnd_comm_set_timeout", C.c_int32, [_H, C.c_int64]),
    ("nnd_comm_info", C.c_int32, [_H, C.POINTER(C.c_int32)]),
    ("nnd_comm_self_test", C.c_int32, [_H]),
    ("nnd_comm_destroy", C.c_int32, [_H]),
    ("nnd_comm_abort", C.c_int32, [_H]),
    ("nnd_comm_local_set_serial", C.c_int32, [_H, C.c_int32]),
    ("nnd_comm_last_error", C.c_char_p, [_H]),
    ("nnd_shard_create", C.c_int32, [C.POINTER(_H), C.POINTER(NNDParams), _H, C.c_void_p]),
    ("nnd_shard_build", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nnd_shard_get_info", C.c_int32, [_H, C.POINTER(NNDShardInfo)]),
    ("nnd_shard_get_stats", C.c_int32, [_H, C.POINTER(NNDStats)]),
    ("nnd_shard_handle", _H, [_H]),
    ("nnd_shard_destroy", C.c_int32, [_H]),
    ("nnd_shard_last_error", C.c_char_p, [_H]),
    ("nnd_build_multi", C.c_int32, [C.POINTER(NNDParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(NNDStats), C.POINTER(NNDShardInfo), C.c_char_p, C.c_int32]),
    ("nnd_build_multi_from_graph", C.c_int32, [C.POINTER(NNDParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.POINTER(NNDStats), C.POINTER(NNDShardInfo), C.c_char_p, C.c_int32]),
    ("nnd_shard_build_from_graph", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ("nnd_shard_build_update", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ("nnd_build_multi_update", C.c_int32, [C.POINTER(NNDParams), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p, C.c_void_p, C.POINTER(NNDStats), C.POINTER(NNDShardInfo), C.c_char_p, C.c_int32]),
    ("nnd_diversify_host", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.POINTER(NNDPruneOpts), C.c_void_p]),
    ("nnd_diversify_csr_host", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(NNDPruneOpts),
                                           C.c_void_p]),
    ("nnd_degree_prune_host", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    ("nnd_search_graph", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_uint32,
                                     C.c_void_p, C.c_void_p, C.POINTER(NNDSearchGraphStats)]),
    ("nnd_search_graph_fetch", C.c_int32, [_H, C.c_void_p, C.c_void_p]),
    ("nnd_hub_tree_build", C.c_int32, [_H, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("nnd_hub_tree_fetch", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]),
    ("nnd_searcher_create", C.c_int32, [C.POINTER(_H), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_int32,
                                        C.c_void_p]),
    ("nnd_rank_order_device", C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]),
    ("nnd_hub_tree_build_device", C.c_int32, [_H, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    ("nnd_search_graph_device", C.c_int32, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    ("nnd_reorder_csr_device", C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_void_p]),
    ("nnd_reorder_host", C.c_int32, [C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    ("nnd_searcher_create_device", C.c_int32, [C.POINTER(_H), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                               C.c_float, C.c_int32, C.c_void_p, C.c_void_p]),
    ("nnd_searcher_query", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    ("nnd_searcher_last_spilled", C.c_int64, [_H]),
    ("nnd_searcher_set_tier", C.c_int32, [_H, C.c_int32]),
    ("nnd_searcher_quantize_u8", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    ("nnd_searcher_set_codes_u8", C.c_int32, [_H, C.c_void_p, C.c_int32, C.c_void_p]),
    ("nnd_searcher_query_proxy", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    ("nnd_searcher_query_rerank", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p]),
    ("nnd_searcher_query_device", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nnd_searcher_query_proxy_device", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                                    C.c_void_p]),
    ("nnd_searcher_query_rerank_device", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                                     C.c_void_p]),
    ("nnd_searcher_set_filter", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int64)]),
    ("nnd_searcher_set_filter_device", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]),
    ("nnd_searcher_clear_filter", C.c_int32, [_H]),
    ("nnd_searcher_set_tags", C.c_int32, [_H, C.c_void_p, C.c_void_p]),
    ("nnd_searcher_set_tags_device", C.c_int32, [_H, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nnd_searcher_clear_tags", C.c_int32, [_H]),
    ("nnd_searcher_count_tags", C.c_int32, [_H, C.c_void_p, C.c_int32, C.c_void_p]),
    ("nnd_searcher_count_tags_device", C.c_int32, [_H, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ("nnd_searcher_query_tagged", C.c_int32, [_H, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p,
                                              C.c_void_p]),
    ("nnd_searcher_query_tagged_device", C.c_int32, [_H, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p]),
    ("nnd_exact_knn_rows_tagged", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(NNDExactStats)]),
    ("nnd_exact_knn_queries_tagged", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.POINTER(NNDExactStats)]),
    ("nnd_exact_knn_rows_tagged_device", C.c_int32, [_H, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.POINTER(NNDExactStats)]),
    ("nnd_exact_knn_queries_tagged_device", C.c_int32, [_H, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.POINTER(NNDExactStats)]),
    ("nnd_searcher_destroy", C.c_int32, [_H]),
    ("nnd_searcher_last_error", C.c_char_p, [_H]),
    ("nnd_graph_csr_device", C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int64,
                                         C.c_int32, C.c_int32, C.POINTER(_H)]),
    ("nnd_csr_arrays", C.c_int32, [_H, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                   C.POINTER(C.c_int64)]),
    ("nnd_csr_destroy", C.c_int32, [_H]),
    ("nnd_graph_csr", C.c_int32, [C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
]
EXPORTED_SYMBOLS = [s[0] for s in _SIGNATURES]

_lib = None


def load_library():
    """dlopen libpynnd_amd.so and bind every entry point.  Raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C pynndescent_amd/csrc`. pynndescent_amd has no CPU fallback." % LIB_PATH
        )
    lib = C.CDLL(LIB_PATH)
    for name, restype, argtypes in _SIGNATURES:
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class NNDError(RuntimeError):
    pass


class Builder:
    """Thin object wrapper over an ``nnd_handle_t`` (one GPU, one stream)."""

    def __init__(self, n, dim, metric, n_neighbors, n_trees, leaf_size, max_depth, max_candidates, n_iters, delta,
                 rng_state, tree_rng, device=0, join_blocks=0, flags=0):
        self.lib = load_library()
        p = NNDParams()
        p.n, p.dim, p.metric = int(n), int(dim), int(metric)
        p.n_neighbors, p.n_trees, p.leaf_size = int(n_neighbors), int(n_trees), int(leaf_size)
        p.max_depth, p.max_candidates, p.n_iters = int(max_depth), int(max_candidates), int(n_iters)
        p.delta = float(delta)
        for i in range(3):
            p.rng_state[i] = int(rng_state[i])
            p.tree_rng[i] = int(tree_rng[i])
        p.device, p.join_blocks, p.flags = int(device), int(join_blocks), int(flags)
        self.params = p
        self.n, self.dim, self.k, self.mc = int(n), int(dim), int(n_neighbors), int(max_candidates)
        self._h = _H()
        if self.lib.nnd_create(C.byref(self._h), C.byref(p)) != 0:
            raise NNDError(self.lib.nnd_last_global_error().decode())
        self._keepalive = None

    def _check(self, rc):
        if rc != 0:
            raise NNDError(self.lib.nnd_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.nnd_destroy(self._h)
            self._h = _H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data -----------------------------------------------------------------------------------
    def set_data_host(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.shape == (self.n, self.dim)
        self._check(self.lib.nnd_set_data_host(self._h, _ptr(x)))

    def data_nonfinite(self):
        """True when the point set handed in held a NaN or an infinity (flag raised by the prep kernel)."""
        out = C.c_int32()
        self._check(self.lib.nnd_data_nonfinite(self._h, C.byref(out)))
        return bool(out.value)

    def data_negative(self):
        """True when the metric is hellinger and the point set held a negative entry (flag raised by the prep kernel)."""
        out = C.c_int32()
        self._check(self.lib.nnd_data_negative(self._h, C.byref(out)))
        return bool(out.value)

    def set_data_device(self, dev_ptr, keepalive=None):
        """dev_ptr: integer address of a float32 (n, dim) C-contiguous device buffer (e.g. tensor.data_ptr()).

        The prep kernel reads the buffer right away on the handle's stream: the producer must be done
        (``torch.cuda.synchronize()`` / stream sync) unless the handle runs on the producing stream (``set_stream``)."""
        self._keepalive = keepalive
        self._check(self.lib.nnd_set_data_device(self._h, C.c_void_p(int(dev_ptr))))

    def set_data_device_typed(self, dev_ptr, dtype, keepalive=None):
        """dev_ptr: integer address of an (n, dim) C-contiguous device buffer of ``dtype`` (NND_DTYPE_*).  float32 is borrowed
        like ``set_data_device``; the other types -- and every type under dot, whose rows are L2-normalised -- are converted
        into the handle's own float32 copy.  The stream rule is ``set_data_device``'s."""
        self._keepalive = keepalive
        self._check(self.lib.nnd_set_data_device_typed(self._h, C.c_void_p(int(dev_ptr)), int(dtype)))

    # -- stages ---------------------------------------------------------------------------------
    def make_forest(self):
        self._check(self.lib.nnd_make_forest(self._h))

    def leaf_array(self):
        nl, ms = C.c_int64(), C.c_int32()
        self._check(self.lib.nnd_leaf_array_shape(self._h, C.byref(nl), C.byref(ms)))
        out = np.empty((max(nl.value, 1), max(ms.value, 1)), np.int32)
        self._check(self.lib.nnd_get_leaf_array(self._h, _ptr(out)))
        return out[: nl.value]

    def reset_graph(self):
        self._check(self.lib.nnd_reset_graph(self._h))

    def init_from_leaves(self):
        self._check(self.lib.nnd_init_from_leaves(self._h))

    def init_from_leaf_array(self, leaf_array):
        """init_rp_tree on the caller's leaves: int32 (n_leaves, max_leaf_size), -1 padded (rptree_leaf_array's table)."""
        la = np.ascontiguousarray(leaf_array, dtype=np.int32)
        assert la.ndim == 2
        self._check(self.lib.nnd_init_from_leaf_array(self._h, _ptr(la), la.shape[0], la.shape[1]))

    def init_random(self):
        self._check(self.lib.nnd_init_random(self._h))

    def init_from_graph(self, idx, dist=None):
        idx = np.ascontiguousarray(idx, np.int32)
        dist = None if dist is None else np.ascontiguousarray(dist, np.float32)
        self._check(self.lib.nnd_init_from_graph(self._h, _ptr(idx), _ptr(dist), idx.shape[1]))

    def init_from_neighbor_graph(self, idx, dist):
        idx = np.ascontiguousarray(idx, np.int32)
        dist = np.ascontiguousarray(dist, np.float32)
        self._check(self.lib.nnd_init_from_neighbor_graph(self._h, _ptr(idx), _ptr(dist), idx.shape[1]))

    def init_from_graph_device(self, idx_ptr, dist_ptr, width):
        """``init_from_graph`` on the device addresses of an int32 / float32 (n, width) graph (``dist_ptr`` 0: distances are
        computed), read in place on the handle's stream; nothing is waited for."""
        self._check(self.lib.nnd_init_from_graph_device(self._h, C.c_void_p(int(idx_ptr)), C.c_void_p(int(dist_ptr)) if dist_ptr else None,
                                                        int(width)))

    def init_from_neighbor_graph_device(self, idx_ptr, dist_ptr, width):
        """``init_from_neighbor_graph`` on device addresses; returns with the handle's stream drained."""
        self._check(self.lib.nnd_init_from_neighbor_graph_device(self._h, C.c_void_p(int(idx_ptr)), C.c_void_p(int(dist_ptr)), int(width)))

    def descent_iter(self):
        c = C.c_int64()
        self._check(self.lib.nnd_descent_iter(self._h, C.byref(c)))
        return c.value

    def descent(self):
        self._check(self.lib.nnd_descent(self._h))

    def sample_candidates(self):
        self._check(self.lib.nnd_sample_candidates(self._h))

    def finalize(self):
        idx = host_pool.empty((self.n, self.k), np.int32)
        dist = host_pool.empty((self.n, self.k), np.float32)
        self._check(self.lib.nnd_finalize_host(self._h, _ptr(idx), _ptr(dist)))
        return idx, dist

    def finalize_device(self, idx_ptr, dist_ptr):
        self._check(self.lib.nnd_finalize_device(self._h, C.c_void_p(int(idx_ptr)), C.c_void_p(int(dist_ptr))))

    def build_device(self, idx_ptr, dist_ptr):
        self._check(self.lib.nnd_build_device(self._h, C.c_void_p(int(idx_ptr)), C.c_void_p(int(dist_ptr))))

    def synchronize(self):
        self._check(self.lib.nnd_synchronize(self._h))

    # -- introspection --------------------------------------------------------------------------
    def stats(self, raw=False):
        """The handle's statistics block; ``raw``: the ctypes structure itself (per-iteration arrays beyond ``n_iters_run`` too:
        ``descent_join`` leaves the counters of a join that no finished iteration owns yet at index ``n_iters_run``)."""
        s = NNDStats()
        self._check(self.lib.nnd_get_stats(self._h, C.byref(s)))
        return s if raw else s.as_dict()

    def graph(self):
        idx = np.empty((self.n, self.k), np.int32)
        dist = np.empty((self.n, self.k), np.float32)
        flags = np.empty((self.n, self.k), np.uint8)
        self._check(self.lib.nnd_get_graph(self._h, _ptr(idx), _ptr(dist), _ptr(flags)))
        return idx, dist, flags

    def candidates(self):
        new = np.empty((self.n, self.mc), np.int32)
        old = np.empty((self.n, self.mc), np.int32)
        self._check(self.lib.nnd_get_candidates(self._h, _ptr(new), _ptr(old)))
        return new, old

    def set_stream(self, stream_ptr):
        """Run the handle on the caller's HIP stream (integer address; 0 / None: the handle's own stream again)."""
        self._check(self.lib.nnd_set_stream(self._h, C.c_void_p(int(stream_ptr)) if stream_ptr else None))

    def descent_sample(self):
        self._check(self.lib.nnd_descent_sample(self._h))

    def descent_join(self):
        self._check(self.lib.nnd_descent_join(self._h))

    @staticmethod
    def _prune_opts(prune_probability=1.0, degree_aware=False, max_degree=1, aggressiveness=1.0, alpha=1.0, seed=0):
        o = NNDPruneOpts()
        o.prune_probability, o.degree_aware, o.max_degree = float(prune_probability), int(bool(degree_aware)), int(max_degree)
        o.aggressiveness, o.alpha, o.seed = float(aggressiveness), float(alpha), int(seed) & 0xFFFFFFFF
        return o

    def diversify(self, idx, dist, degree=None, **opts):
        """diversify / diversify_degree_aware; opts: prune_probability, degree_aware, max_degree, aggressiveness, alpha, seed."""
        idx = np.ascontiguousarray(idx, np.int32).copy()
        dist = np.ascontiguousarray(dist, np.float32).copy()
        assert idx.shape == (self.n, self.k) and dist.shape == idx.shape
        o = self._prune_opts(**opts)
        degree = None if degree is None else np.ascontiguousarray(degree, np.int32)
        self._check(self.lib.nnd_diversify_host(self._h, _ptr(idx), _ptr(dist), C.byref(o), _ptr(degree)))
        return idx, dist

    def diversify_csr(self, indptr, indices, data, degree=None, **opts):
        indptr = np.ascontiguousarray(indptr, np.int32)
        indices = np.ascontiguousarray(indices, np.int32)
        data = np.ascontiguousarray(data, np.float32).copy()
        assert indptr.shape[0] == self.n + 1
        o = self._prune_opts(**opts)
        degree = None if degree is None else np.ascontiguousarray(degree, np.int32)
        self._check(self.lib.nnd_diversify_csr_host(self._h, _ptr(indptr), _ptr(indices), _ptr(data), data.shape[0],
                                                    C.byref(o), _ptr(degree)))
        return data

    def search_graph(self, idx, dist, n_neighbors, pruning_degree_multiplier=1.5, diversify_prob=1.0, degree_aware=False,
                     degree_prune_aggressiveness=1.0, seed=0, on_device=False, want_forward=False):
        """The whole pruning pass on the device (csrc/searchgraph.hip).  idx / dist: numpy (n, k) arrays, or device addresses
        (ints) when ``on_device``.  Returns (indptr, indices, stats dict[, forward rows, forward distances])."""
        st = NNDSearchGraphStats()
        fr = fd = None
        if want_forward:
            fr = np.empty((self.n, self.k), np.int32)
            fd = np.empty((self.n, self.k), np.float32)
        if on_device:
            pi, pd = C.c_void_p(int(idx)), C.c_void_p(int(dist))
        else:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            dist = np.ascontiguousarray(dist, dtype=np.float32)
            assert idx.shape == (self.n, self.k) and dist.shape == (self.n, self.k)
            pi, pd = _ptr(idx), _ptr(dist)
        self._check(self.lib.nnd_search_graph(self._h, pi, pd, 1 if on_device else 0, int(n_neighbors), float(pruning_degree_multiplier),
                                              float(diversify_prob), 1 if degree_aware else 0, float(degree_prune_aggressiveness),
                                              int(seed) & 0xFFFFFFFF, _ptr(fr) if want_forward else None, _ptr(fd) if want_forward else None,
                                              C.byref(st)))
        indptr = np.empty(self.n + 1, np.int32)
        indices = np.empty(max(int(st.final_nnz), 1), np.int32)
        self._check(self.lib.nnd_search_graph_fetch(self._h, _ptr(indptr), _ptr(indices)))
        stats = {f: getattr(st, f) for f, _ in NNDSearchGraphStats._fields_ if f != "reserved"}
        out = (indptr, indices[: int(st.final_nnz)], stats)
        return out + (fr, fd) if want_forward else out

    def search_graph_device(self, idx_ptr, dist_ptr, n_neighbors, pruning_degree_multiplier=1.5, diversify_prob=1.0, degree_aware=False,
                            degree_prune_aggressiveness=1.0, seed=0):
        """The pass on a graph at the device addresses ``idx_ptr`` / ``dist_ptr``, its result left where it lies: returns (device
        address of indptr (n + 1), of indices (nnz), nnz, stats dict).  The addresses are the handle's: valid until its next pass
        or ``close()``; the reorder of ``reorder_csr_device`` reads them in place."""
        st = NNDSearchGraphStats()
        self._check(self.lib.nnd_search_graph(self._h, C.c_void_p(int(idx_ptr)), C.c_void_p(int(dist_ptr)), 1, int(n_neighbors),
                                              float(pruning_degree_multiplier), float(diversify_prob), 1 if degree_aware else 0,
                                              float(degree_prune_aggressiveness), int(seed) & 0xFFFFFFFF, None, None, C.byref(st)))
        indptr, indices, nnz = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self.lib.nnd_search_graph_device(self._h, C.byref(indptr), C.byref(indices), C.byref(nnz)))
        stats = {f: getattr(st, f) for f, _ in NNDSearchGraphStats._fields_ if f != "reserved"}
        return int(indptr.value or 0), int(indices.value or 0), int(nnz.value), stats

    def degree_prune(self, indptr, data, max_degree):
        indptr = np.ascontiguousarray(indptr, np.int32)
        data = np.ascontiguousarray(data, np.float32).copy()
        self._check(self.lib.nnd_degree_prune_host(self._h, _ptr(indptr), _ptr(data), data.shape[0], int(max_degree)))
        return data

    def hub_tree(self, rank_order, leaf_size, max_depth):
        """make_hub_tree + convert_tree_format on the device; returns (hyperplanes, offsets, children, indices, leaf_size)."""
        ro = np.ascontiguousarray(rank_order, np.int32)
        assert ro.shape == (self.n,)
        nn = C.c_int64()
        self._check(self.lib.nnd_hub_tree_build(self._h, _ptr(ro), int(leaf_size), int(max_depth), C.byref(nn)))
        return self._hub_tree_fetch(nn.value)

    def _hub_tree_fetch(self, n_nodes):
        hyper = np.empty((n_nodes, self.dim), np.float32)
        offs = np.empty((n_nodes,), np.float32)
        children = np.empty((n_nodes, 2), np.int32)
        indices = np.empty((self.n,), np.int32)
        ml = C.c_int32()
        self._check(self.lib.nnd_hub_tree_fetch(self._h, _ptr(hyper), _ptr(offs), _ptr(children), _ptr(indices), C.byref(ml)))
        return hyper, offs, children, indices, int(ml.value)

    def hub_tree_device(self, rank_order_ptr, leaf_size, max_depth):
        """``hub_tree`` with the rank order at a device address (int32 (n), e.g. what ``rank_order_device`` wrote)."""
        nn = C.c_int64()
        self._check(self.lib.nnd_hub_tree_build_device(self._h, C.c_void_p(int(rank_order_ptr)), int(leaf_size), int(max_depth), C.byref(nn)))
        return self._hub_tree_fetch(nn.value)

    def pairwise_gram(self, rows_a, rows_b):
        a = np.ascontiguousarray(rows_a, np.int32)
        b = np.ascontiguousarray(rows_b, np.int32)
        out = np.empty((a.shape[0], b.shape[0]), np.float32)
        self._check(self.lib.nnd_pairwise_gram(self._h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], _ptr(out)))
        return out


    # -- exact search (csrc/exact.hip) --------------------------------------------------------------
    def _exact(self, call, arg, m, k, tags=None, masks=None):
        idx = np.empty((m, int(k)), np.int32)
        dist = np.empty((m, int(k)), np.float32)
        st = NNDExactStats()
        if tags is not None:  # the masked search (the *_tagged entry given as ``call``): uint64 words, n tags and m masks
            tags, masks = np.ascontiguousarray(tags, np.uint64), np.ascontiguousarray(masks, np.uint64)
            assert tags.shape == (self.n,) and masks.shape == (m,)
            self._check(call(self._h, _ptr(arg), m, int(k), _ptr(tags), _ptr(masks), _ptr(idx), _ptr(dist), C.byref(st)))
        else:
            self._check(call(self._h, _ptr(arg), m, int(k), _ptr(idx), _ptr(dist), C.byref(st)))
        stats = st.as_dict()
        stats["slices"] = int(self.lib.nnd_exact_slice_count(self._h, m))
        return idx, dist, stats

    def exact_knn(self, rows=None, k=10, tags=None, masks=None):
        """Exact k nearest neighbours (self included) of ``rows`` of the handle's point set (None: all of them): int32 ids and
        float32 alt-space distances (m, k), rows ascending by (float64 distance, id), and the call's statistics.  ``tags`` (n
        uint64 words) and ``masks`` (one per query row): the masked search among the rows whose tag word meets the row's mask."""
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        call = self.lib.nnd_exact_knn_rows if tags is None else self.lib.nnd_exact_knn_rows_tagged
        return self._exact(call, rows, self.n if rows is None else rows.shape[0], k, tags, masks)

    def exact_knn_queries(self, q, k, tags=None, masks=None):
        """The same for external queries, float32 (m, dim), prepared with the point set's own transform."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        assert q.ndim == 2 and q.shape[1] == self.dim
        call = self.lib.nnd_exact_knn_queries if tags is None else self.lib.nnd_exact_knn_queries_tagged
        return self._exact(call, q, q.shape[0], k, tags, masks)


    def exact_knn_device(self, k, idx_ptr, dist_ptr, rows_ptr=0, n_rows=None, q_ptr=0, q_dtype=NND_DTYPE_FLOAT32, n_q=0, tags_ptr=0,
                         masks_ptr=0):
        """The exact search with every array on the handle's device, on the handle's stream: of the int32 row ids at ``rows_ptr``
        (0: all rows), or of the (n_q, dim) queries of ``q_dtype`` at ``q_ptr``; int32 / float32 (m, k) answers written at
        ``idx_ptr`` / ``dist_ptr``.  ``tags_ptr`` / ``masks_ptr``: the masked search (n tag words, m mask words on the device).
        Returns the call's statistics."""
        st = NNDExactStats()
        dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
        if q_ptr:
            m = int(n_q)
            if tags_ptr:
                self._check(self.lib.nnd_exact_knn_queries_tagged_device(self._h, dev(q_ptr), int(q_dtype), m, int(k), dev(tags_ptr),
                                                                         dev(masks_ptr), dev(idx_ptr), dev(dist_ptr), C.byref(st)))
            else:
                self._check(self.lib.nnd_exact_knn_queries_device(self._h, dev(q_ptr), int(q_dtype), m, int(k), dev(idx_ptr), dev(dist_ptr),
                                                                  C.byref(st)))
        else:
            m = self.n if not rows_ptr else int(n_rows)
            if tags_ptr:
                self._check(self.lib.nnd_exact_knn_rows_tagged_device(self._h, dev(rows_ptr), m, int(k), dev(tags_ptr), dev(masks_ptr),
                                                                      dev(idx_ptr), dev(dist_ptr), C.byref(st)))
            else:
                self._check(self.lib.nnd_exact_knn_rows_device(self._h, dev(rows_ptr), m, int(k), dev(idx_ptr), dev(dist_ptr), C.byref(st)))
        stats = st.as_dict()
        stats["slices"] = int(self.lib.nnd_exact_slice_count(self._h, m))
        return stats


class Searcher:
    """Thin wrapper over an ``nnd_searcher_t``: device copies of a prepared index, batched queries (one wave per query)."""

    def __init__(self, data, search_graph, tree, metric, min_distance, n_neighbors, search_rng_state, device=0):
        self.lib = load_library()
        data = np.ascontiguousarray(data, np.float32)
        self.n, self.dim = data.shape
        indptr = np.ascontiguousarray(search_graph.indptr, np.int32)
        indices = np.ascontiguousarray(search_graph.indices, np.int32)
        if tree is not None:
            hyper = np.ascontiguousarray(tree.hyperplanes, np.float32)
            offs = np.ascontiguousarray(tree.offsets, np.float32)
            children = np.ascontiguousarray(tree.children, np.int32)
            tidx = np.ascontiguousarray(tree.indices, np.int32)
            n_nodes = hyper.shape[0]
        else:
            hyper = offs = children = tidx = None
            n_nodes = 0
        rng = np.ascontiguousarray(search_rng_state, np.int64)
        self.has_codes = False  # quantize_u8 / set_codes_u8 ran
        self._h = _H()
        rc = self.lib.nnd_searcher_create(C.byref(self._h), int(device), self.n, self.dim, int(metric), _ptr(data), _ptr(indptr),
                                          _ptr(indices), int(indices.shape[0]), _ptr(hyper), _ptr(offs), _ptr(children), _ptr(tidx),
                                          int(n_nodes), float(min_distance), int(n_neighbors), _ptr(rng))
        if rc != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(None).decode())

    @classmethod
    def from_device(cls, rows_ptr, dtype, n, dim, order_ptr, indptr_ptr, indices_ptr, nnz, tree, metric, min_distance, n_neighbors,
                    search_rng_state, device=0, stream_ptr=0):
        """The searcher filled from device memory (``nnd_searcher_create_device``): (n, dim) rows of ``dtype`` (NND_DTYPE_*) at
        ``rows_ptr`` in their original order, gathered by the int32 permutation at ``order_ptr`` (0: identity); the CSR graph in the
        searcher's numbering at ``indptr_ptr`` / ``indices_ptr``; ``tree``: host FlatTree or None; on the HIP stream ``stream_ptr``."""
        self = object.__new__(cls)
        self.lib = load_library()
        self.n, self.dim = int(n), int(dim)
        if tree is not None:
            hyper = np.ascontiguousarray(tree.hyperplanes, np.float32)
            offs = np.ascontiguousarray(tree.offsets, np.float32)
            children = np.ascontiguousarray(tree.children, np.int32)
            tidx = np.ascontiguousarray(tree.indices, np.int32)
            n_nodes = hyper.shape[0]
        else:
            hyper = offs = children = tidx = None
            n_nodes = 0
        rng = np.ascontiguousarray(search_rng_state, np.int64)
        self.has_codes = False
        self._h = _H()
        dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
        rc = self.lib.nnd_searcher_create_device(C.byref(self._h), int(device), self.n, self.dim, int(metric), dev(rows_ptr), int(dtype),
                                                 dev(order_ptr), dev(indptr_ptr), dev(indices_ptr), int(nnz), _ptr(hyper), _ptr(offs),
                                                 _ptr(children), _ptr(tidx), int(n_nodes), float(min_distance), int(n_neighbors), _ptr(rng),
                                                 dev(stream_ptr))
        if rc != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(None).decode())
        return self

    def query(self, queries, k, epsilon):
        q = np.ascontiguousarray(queries, np.float32)
        assert q.ndim == 2 and q.shape[1] == self.dim
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.float32)
        if self.lib.nnd_searcher_query(self._h, _ptr(q), q.shape[0], int(k), float(epsilon), _ptr(idx), _ptr(dist)) != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(self._h).decode())
        return idx, dist

    def quantize_u8(self, values, rows=None, fetch=True):
        """Device codes of the rows (``np.searchsorted(values, rows).astype(np.uint8)``) for ``query_proxy``; ``rows``
        (n, dim) in the searcher's order, or None for the searcher's own copy.  Returns the (n, dim) uint8 codes, or None
        when ``fetch`` is false."""
        values = np.ascontiguousarray(values, np.float32)
        if rows is not None:
            rows = np.ascontiguousarray(rows, np.float32)
            assert rows.shape == (self.n, self.dim)
        codes = np.empty((self.n, self.dim), np.uint8) if fetch else None
        if self.lib.nnd_searcher_quantize_u8(self._h, _ptr(rows), _ptr(values), int(values.shape[0]), _ptr(codes)) != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(self._h).decode())
        self.has_codes = True
        return codes

    def set_codes_u8(self, values, codes):
        """The state of ``quantize_u8`` from codes computed before."""
        values = np.ascontiguousarray(values, np.float32)
        codes = np.ascontiguousarray(codes, np.uint8)
        assert codes.shape == (self.n, self.dim)
        if self.lib.nnd_searcher_set_codes_u8(self._h, _ptr(values), int(values.shape[0]), _ptr(codes)) != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(self._h).decode())
        self.has_codes = True

    def query_proxy(self, queries, k, search_k, epsilon):
        """The walk on the codes keeps ``search_k`` results, the exact rerank returns the best ``k`` (alt space)."""
        q = np.ascontiguousarray(queries, np.float32)
        assert q.ndim == 2 and q.shape[1] == self.dim
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.float32)
        if self.lib.nnd_searcher_query_proxy(self._h, _ptr(q), q.shape[0], int(k), int(search_k), float(epsilon), _ptr(idx),
                                             _ptr(dist)) != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(self._h).decode())
        return idx, dist

    def query_rerank(self, queries, k, search_k, epsilon):
        """A metric with a true distance besides the one it walks on (proxy_inner_product): the walk on the float rows keeps
        ``search_k`` results by the proxy distance, the rerank returns the best ``k`` by the true one (-<q,x>)."""
        q = np.ascontiguousarray(queries, np.float32)
        assert q.ndim == 2 and q.shape[1] == self.dim
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.float32)
        if self.lib.nnd_searcher_query_rerank(self._h, _ptr(q), q.shape[0], int(k), int(search_k), float(epsilon), _ptr(idx),
                                              _ptr(dist)) != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(self._h).decode())
        return idx, dist

    def query_device(self, form, q_ptr, nq, k, search_k, epsilon, idx_ptr, dist_ptr, stream_ptr):
        """The three query forms (``form``: "float", "proxy", "rerank") on device buffers: float32 (nq, dim) queries at
        ``q_ptr``, int32 / float32 (nq, k) results at ``idx_ptr`` / ``dist_ptr``, on the HIP stream ``stream_ptr`` (0: the
        device's default stream).  Returns when the stream has drained."""
        q, oi, od = C.c_void_p(int(q_ptr)), C.c_void_p(int(idx_ptr)), C.c_void_p(int(dist_ptr))
        st = C.c_void_p(int(stream_ptr)) if stream_ptr else None
        if form == "float":
            rc = self.lib.nnd_searcher_query_device(self._h, q, int(nq), int(k), float(epsilon), oi, od, st)
        elif form == "proxy":
            rc = self.lib.nnd_searcher_query_proxy_device(self._h, q, int(nq), int(k), int(search_k), float(epsilon), oi, od, st)
        else:
            rc = self.lib.nnd_searcher_query_rerank_device(self._h, q, int(nq), int(k), int(search_k), float(epsilon), oi, od, st)
        if rc != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(self._h).decode())

    def set_filter(self, filter, order=None):
        """The allow set of the next queries (``nnd_searcher_set_filter``), from host arrays: a bool / uint8 mask of n rows or an
        integer array of row ids, in the ORIGINAL numbering; ``order`` (int32, n; None: the identity) is the searcher's row order.
        Returns the number of allowed rows; ``ValueError`` for an id outside 0 .. n - 1."""
        f = np.asarray(filter)
        if f.dtype == np.bool_ or f.dtype == np.uint8:
            f, kind = np.ascontiguousarray(f).view(np.uint8), NND_FILTER_MASK
        else:
            f, kind = np.ascontiguousarray(f, np.int64), NND_FILTER_IDS
        assert f.ndim == 1 and (kind == NND_FILTER_IDS or f.shape[0] == self.n)
        if order is not None:
            order = np.ascontiguousarray(order, np.int32)
            assert order.shape == (self.n,)
        count = C.c_int64(0)
        return self._filter_rc(self.lib.nnd_searcher_set_filter(self._h, _ptr(f), int(f.shape[0]), kind, _ptr(order), C.byref(count)), count)

    def set_filter_device(self, filter_ptr, count, kind, order_ptr, stream_ptr):
        """``set_filter`` from device memory (``nnd_searcher_set_filter_device``): ``count`` mask bytes (``NND_FILTER_MASK``) or int64
        ids (``NND_FILTER_IDS``) at ``filter_ptr``, the int32 row order at ``order_ptr`` (0: the identity), on the HIP stream
        ``stream_ptr`` (0: the default stream)."""
        dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
        n_allowed = C.c_int64(0)
        return self._filter_rc(self.lib.nnd_searcher_set_filter_device(self._h, dev(filter_ptr), int(count), int(kind), dev(order_ptr),
                                                                       C.byref(n_allowed), dev(stream_ptr)), n_allowed)

    def _filter_rc(self, rc, count):
        if rc == 2:
            raise ValueError(self.lib.nnd_searcher_last_error(self._h).decode())
        if rc != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(self._h).decode())
        return int(count.value)

    def clear_filter(self):
        """Back to unfiltered queries."""
        if self.lib.nnd_searcher_clear_filter(self._h) != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(self._h).decode())

    # -- per-query filters: the rows' tag words, the counts per mask, the tagged walk --------------------
    def _rc(self, rc):
        if rc != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(self._h).decode())

    def set_tags(self, tags, order=None):
        """The rows' tag words (``nnd_searcher_set_tags``) from a host array of n 64-bit words in the ORIGINAL numbering; ``order``
        (int32, n; None: the identity) is the searcher's row order."""
        t = np.ascontiguousarray(tags).view(np.uint64)
        assert t.shape == (self.n,)
        if order is not None:
            order = np.ascontiguousarray(order, np.int32)
            assert order.shape == (self.n,)
        self._rc(self.lib.nnd_searcher_set_tags(self._h, _ptr(t), _ptr(order)))

    def set_tags_device(self, tags_ptr, order_ptr, stream_ptr):
        """``set_tags`` from device memory: n 64-bit words at ``tags_ptr``, the int32 row order at ``order_ptr`` (0: the identity)."""
        dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
        self._rc(self.lib.nnd_searcher_set_tags_device(self._h, dev(tags_ptr), dev(order_ptr), dev(stream_ptr)))

    def clear_tags(self):
        """Releases the searcher's copy of the tag words."""
        self._rc(self.lib.nnd_searcher_clear_tags(self._h))

    def count_tags(self, masks):
        """For every 64-bit mask word of the host array ``masks``: the rows whose tag word meets it (int64)."""
        m = np.ascontiguousarray(masks).view(np.uint64).reshape(-1)
        counts = np.zeros(m.shape[0], np.int64)
        self._rc(self.lib.nnd_searcher_count_tags(self._h, _ptr(m), int(m.shape[0]), _ptr(counts)))
        return counts

    def count_tags_device(self, masks_ptr, n_masks, counts_ptr, stream_ptr):
        """``count_tags`` on device memory: ``n_masks`` words at ``masks_ptr``, int64 counts written at ``counts_ptr``."""
        dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
        self._rc(self.lib.nnd_searcher_count_tags_device(self._h, dev(masks_ptr), int(n_masks), dev(counts_ptr), dev(stream_ptr)))

    def query_tagged(self, form, queries, masks, k, search_k, epsilon):
        """The walk of ``query`` / ``query_proxy`` / ``query_rerank`` (``form``: "float", "proxy", "rerank") in which a vertex
        enters query i's result list only if its tag word meets ``masks[i]`` (host arrays)."""
        q = np.ascontiguousarray(queries, np.float32)
        m = np.ascontiguousarray(masks).view(np.uint64)
        assert q.ndim == 2 and q.shape[1] == self.dim and m.shape == (q.shape[0],)
        idx = np.empty((q.shape[0], k), np.int32)
        dist = np.empty((q.shape[0], k), np.float32)
        self._rc(self.lib.nnd_searcher_query_tagged(self._h, NND_QUERY_FORMS[form], _ptr(q), q.shape[0], int(k), int(search_k), float(epsilon),
                                                    _ptr(m), _ptr(idx), _ptr(dist)))
        return idx, dist

    def query_tagged_device(self, form, q_ptr, masks_ptr, nq, k, search_k, epsilon, idx_ptr, dist_ptr, stream_ptr):
        """``query_tagged`` on device buffers (see ``query_device``); ``masks_ptr``: nq 64-bit words."""
        dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
        self._rc(self.lib.nnd_searcher_query_tagged_device(self._h, NND_QUERY_FORMS[form], dev(q_ptr), int(nq), int(k), int(search_k),
                                                           float(epsilon), dev(masks_ptr), dev(idx_ptr), dev(dist_ptr), dev(stream_ptr)))

    def last_spilled(self):
        """Queries of the last call whose search outgrew the LDS structures and ran on the global-memory tier."""
        return int(self.lib.nnd_searcher_last_spilled(self._h))

    def set_tier(self, tier):
        """0: automatic (LDS tier, overflowing queries re-run on the global-memory tier); 1: every query on the latter."""
        if self.lib.nnd_searcher_set_tier(self._h, int(tier)) != 0:
            raise NNDError(self.lib.nnd_searcher_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.nnd_searcher_destroy(self._h)
            self._h = _H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostPool:
    """Result arrays in pinned host memory, recycled (round 6; include/pynnd_amd.h nnd_host_alloc).

    ``empty(shape, dtype)`` is ``numpy.empty`` for arrays of 4 MB and more, backed by a pinned buffer: the pages are resident (a
    fresh 60 MB numpy array costs ~15 k page faults on first touch: 12 of the 57 ms of ``NNDescent(x).neighbor_graph`` at
    1 M x 15) and the library copies a finished graph into it with one DMA.  A buffer returns to the pool when the last numpy
    view of it is garbage-collected and serves the next request of the same size: a process that builds index after index
    allocates its result arrays once.  Without a device, or beyond ``max_bytes`` of pinned memory, ``numpy.empty``."""

    def __init__(self, min_bytes=4 << 20, max_bytes=4 << 30, keep_per_size=6):
        import threading

        self.min_bytes, self.max_bytes, self.keep = min_bytes, max_bytes, keep_per_size
        self._free, self._held, self._lock = {}, 0, threading.Lock()

    def _release(self, ptr, nbytes):
        with self._lock:
            lst = self._free.setdefault(nbytes, [])
            if len(lst) < self.keep:
                lst.append(ptr)
                return
            self._held -= nbytes
        try:
            load_library().nnd_host_free(C.c_void_p(ptr))
        except Exception:  # (interpreter shutdown)
            pass

    def empty(self, shape, dtype):
        import weakref

        dtype = np.dtype(dtype)
        shape = tuple(int(v) for v in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        if nbytes < self.min_bytes:
            return np.empty(shape, dtype)
        ptr = None
        with self._lock:
            lst = self._free.get(nbytes)
            if lst:
                ptr = lst.pop()
            elif self._held + nbytes <= self.max_bytes:
                self._held += nbytes
                ptr = 0
        if ptr == 0:
            ptr = load_library().nnd_host_alloc(nbytes)
            if not ptr:
                with self._lock:
                    self._held -= nbytes
                ptr = None
        if ptr is None:
            return np.empty(shape, dtype)
        buf = (C.c_char * nbytes).from_address(ptr)
        fin = weakref.finalize(buf, self._release, ptr, nbytes)
        fin.atexit = False  # (process exit releases the memory)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    def trim(self):
        """Give the idle buffers back."""
        with self._lock:
            items = [(p, nb) for nb, lst in self._free.items() for p in lst]
            self._free.clear()
            self._held -= sum(nb for _, nb in items)
        for p, _ in items:
            load_library().nnd_host_free(C.c_void_p(p))


host_pool = HostPool()


def host_copy(a):
    """``a.copy()`` for a C-contiguous array, the pages of the fresh destination touched by several host threads."""
    if not a.flags.c_contiguous or a.nbytes < (4 << 20):
        return a.copy()
    out = host_pool.empty(a.shape, a.dtype)
    if load_library().nnd_host_copy(_ptr(out), _ptr(a), a.nbytes) != 0:
        raise NNDError(load_library().nnd_last_global_error().decode())
    return out


def host_sqrt(a):
    """``numpy.sqrt(a)`` for a C-contiguous float32 array (IEEE sqrtf per element: the same bits), several host threads."""
    if a.dtype != np.float32 or not a.flags.c_contiguous or a.nbytes < (4 << 20):
        return np.sqrt(a)
    out = host_pool.empty(a.shape, a.dtype)
    if load_library().nnd_host_sqrt_f32(_ptr(out), _ptr(a), a.size) != 0:
        raise NNDError(load_library().nnd_last_global_error().decode())
    return out


def device_rows_f32(device, stream_ptr, src_ptr, dtype, n, dim, normalize, dst_ptr):
    """(n, dim) rows of ``dtype`` (NND_DTYPE_*) at the device address ``src_ptr`` -> float32 at ``dst_ptr``, L2-normalised when
    ``normalize``; queued on the HIP stream ``stream_ptr`` (0: the default stream) of ``device``, nothing is waited for."""
    lib = load_library()
    if lib.nnd_device_rows_f32(int(device), C.c_void_p(int(stream_ptr)) if stream_ptr else None, C.c_void_p(int(src_ptr)), int(dtype),
                               int(n), int(dim), 1 if normalize else 0, C.c_void_p(int(dst_ptr))) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())


def device_csr_rows(device, stream_ptr, indptr_ptr, indptr_width, indices_ptr, indices_width, values_ptr, n, dim, dst_ptr):
    """The canonical CSR matrix at the device addresses ``indptr_ptr`` (n + 1 entries of ``indptr_width`` bytes, 4 or 8) /
    ``indices_ptr`` (``indices_width`` bytes each) / ``values_ptr`` (float32) -> its dense (n, dim) float32 rows at ``dst_ptr``
    (csrc/sparse.hip); queued on ``stream_ptr`` of ``device``, nothing is waited for."""
    lib = load_library()
    dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
    if lib.nnd_device_csr_rows(int(device), dev(stream_ptr), dev(indptr_ptr), int(indptr_width), dev(indices_ptr), int(indices_width),
                               dev(values_ptr), int(n), int(dim), dev(dst_ptr)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())


def device_linear_rows(device, stream_ptr, kind, dim, map_ptr, shift_ptr, x_ptr, n, y_ptr):
    """``y = A (x - c)`` for the (n, dim) float32 rows at the device address ``x_ptr`` into ``y_ptr`` (``kind``: NND_LINEAR_*;
    ``map_ptr``: dim floats or (dim, dim); ``shift_ptr``: dim floats); queued on ``stream_ptr`` of ``device``."""
    lib = load_library()
    dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
    if lib.nnd_device_linear_rows(int(device), dev(stream_ptr), int(kind), int(dim), dev(map_ptr), dev(shift_ptr), dev(x_ptr), int(n),
                                  dev(y_ptr)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())


def linear_rows_host(kind, a, shift, x, device=0):
    """``y = A (x - c)`` of the float32 host rows ``x`` by the device kernel (``nnd_linear_rows_host``): a new float32 array."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    a, shift = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(shift, np.float32)
    n, dim = x.shape
    assert shift.shape == (dim,) and a.shape == ((dim, dim) if kind == NND_LINEAR_DENSE else (dim,))
    y = np.empty((n, dim), np.float32)
    if lib.nnd_linear_rows_host(int(device), int(kind), dim, _ptr(a), _ptr(shift), _ptr(x), n, _ptr(y)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())
    return y


def rowmap_out_dim(kind, dim):
    """The output width of a row map (``NND_ROWMAP_*``) for rows of ``dim`` columns."""
    return 3 if int(kind) == NND_ROWMAP_SPHERE else int(dim)


def device_map_rows(device, stream_ptr, kind, dim, x_stride, shift_ptr, x_ptr, n, y_ptr):
    """The row map ``kind`` (NND_ROWMAP_*) of the (n, dim) float32 rows at the device address ``x_ptr`` (row stride ``x_stride``
    elements) into the contiguous rows at ``y_ptr`` (``rowmap_out_dim`` columns; ``shift_ptr``: 3 floats for the sphere, else 0);
    queued on ``stream_ptr`` of ``device``."""
    lib = load_library()
    dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
    if lib.nnd_device_map_rows(int(device), dev(stream_ptr), int(kind), int(dim), int(x_stride), dev(shift_ptr), dev(x_ptr), int(n),
                               dev(y_ptr)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())


def map_rows_host(kind, shift, x, device=0, dim=None):
    """The row map ``kind`` of the float32 host rows ``x`` by the device kernel (``nnd_map_rows_host``): a new float32 array.
    ``dim``: the live columns of ``x`` when it has more (the rest is a stride's padding, never read)."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    n, stride = x.shape
    dim = stride if dim is None else int(dim)
    if shift is not None:
        shift = np.ascontiguousarray(shift, np.float32)
        assert shift.shape == (3,)
    y = np.empty((n, rowmap_out_dim(kind, dim)), np.float32)
    if lib.nnd_map_rows_host(int(device), int(kind), dim, stride, None if shift is None else _ptr(shift), _ptr(x), n, _ptr(y)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())
    return y


def device_correct(device, stream_ptr, kind, in_ptr, out_ptr, count):
    """``count`` float32 kernel distances at ``in_ptr`` -> the metric's own at ``out_ptr`` (``kind``: NND_CORRECT_*; float32 out
    for COPY and SQRT, float64 for the others), queued on ``stream_ptr`` of ``device``."""
    lib = load_library()
    if lib.nnd_device_correct(int(device), C.c_void_p(int(stream_ptr)) if stream_ptr else None, int(kind), C.c_void_p(int(in_ptr)),
                              C.c_void_p(int(out_ptr)), int(count)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())


def device_update_rows(device, stream_ptr, dim, old, fresh, updated, pairs, out_ptr, out_dtype):
    """The grown point set of ``update()`` at ``out_ptr`` (``nnd_device_update_rows``).  ``old`` / ``fresh`` / ``updated``:
    ``(device address, NND_DTYPE_*, rows)`` each (rows 0: absent); ``pairs``: ``(address of the int32 source rows, address of the
    int32 destination ids, count)``; queued on ``stream_ptr`` of ``device``."""
    lib = load_library()
    dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
    if lib.nnd_device_update_rows(int(device), dev(stream_ptr), int(dim), dev(old[0]), int(old[1]), int(old[2]), dev(fresh[0]), int(fresh[1]),
                                  int(fresh[2]), dev(updated[0]), int(updated[1]), int(updated[2]), dev(pairs[0]), dev(pairs[1]), int(pairs[2]),
                                  dev(out_ptr), int(out_dtype)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())


def device_update_graph(device, stream_ptr, idx_ptr, dist_ptr, n_old, k, ids_ptr, n_upd, n_new, map_ptr, out_idx_ptr, out_dist_ptr):
    """The old (n_old, k) graph at ``idx_ptr`` / ``dist_ptr`` invalidated for the ``n_upd`` updated ids at ``ids_ptr`` and padded
    to ``n_new`` rows, into ``out_idx_ptr`` / ``out_dist_ptr``; ``map_ptr``: n_old bytes of scratch."""
    lib = load_library()
    dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
    if lib.nnd_device_update_graph(int(device), dev(stream_ptr), dev(idx_ptr), dev(dist_ptr), int(n_old), int(k), dev(ids_ptr), int(n_upd),
                                   int(n_new), dev(map_ptr), dev(out_idx_ptr), dev(out_dist_ptr)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())


def device_recall_hits(device, stream_ptr, true_ptr, m, k, graph_ptr, n, width, rows_ptr, hits_ptr):
    """The int64 at ``hits_ptr`` = how many of the (m, k) true ids at ``true_ptr`` appear in the rows ``rows_ptr`` (int32 (m)) of the
    int32 (n, width) graph at ``graph_ptr``; queued on ``stream_ptr`` of ``device``."""
    lib = load_library()
    dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
    if lib.nnd_device_recall_hits(int(device), dev(stream_ptr), dev(true_ptr), int(m), int(k), dev(graph_ptr), int(n), int(width), dev(rows_ptr),
                                  dev(hits_ptr)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())


def rank_order_device(device, stream_ptr, idx_ptr, n, k, out_ptr):
    """The hub tree's rank order of the int32 (n, k) graph at the device address ``idx_ptr``: the ids by (-in-degree, id), int32
    (n) at ``out_ptr`` -- ``numpy.argsort(-bincount, kind="stable")``; on ``stream_ptr`` of ``device``, drained on return."""
    lib = load_library()
    if lib.nnd_rank_order_device(int(device), C.c_void_p(int(stream_ptr)) if stream_ptr else None, C.c_void_p(int(idx_ptr)), int(n), int(k),
                                 C.c_void_p(int(out_ptr))) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())


def reorder_csr_device(device, stream_ptr, order_ptr, n, indptr_ptr, indices_ptr, nnz, indptr_out_ptr, indices_out_ptr):
    """Rows and columns of the CSR pattern at the device addresses ``indptr_ptr`` / ``indices_ptr`` in the order of the int32
    permutation at ``order_ptr`` (0: the identity, a copy), columns ascending, into ``indptr_out_ptr`` / ``indices_out_ptr``."""
    lib = load_library()
    dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
    if lib.nnd_reorder_csr_device(int(device), dev(stream_ptr), dev(order_ptr), int(n), dev(indptr_ptr), dev(indices_ptr), int(nnz),
                                  dev(indptr_out_ptr), dev(indices_out_ptr)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())


def reorder_host(order, indptr, indices, x, device=0):
    """``search_tree.reorder_by_tree`` by the device kernels on host arrays (the test entry): returns (indptr, indices, rows) --
    the CSR pattern and the float32 rows ``x`` in the order ``order`` (None: identity), the rows in the searcher's layout, (n, dp)
    with dp = (dim + 3) & ~3 and zeros past dim."""
    lib = load_library()
    x = np.ascontiguousarray(x, np.float32)
    n, dim = x.shape
    indptr = np.ascontiguousarray(indptr, np.int32)
    indices = np.ascontiguousarray(indices, np.int32)
    order = None if order is None else np.ascontiguousarray(order, np.int32)
    assert indptr.shape == (n + 1,) and (order is None or order.shape == (n,))
    nnz = int(indices.shape[0])
    out_ptr = np.empty(n + 1, np.int32)
    out_ind = np.empty(max(nnz, 1), np.int32)
    out_x = np.empty((n, (dim + 3) & ~3), np.float32)
    if lib.nnd_reorder_host(int(device), n, dim, _ptr(order), _ptr(indptr), _ptr(indices), nnz, _ptr(x), _ptr(out_ptr), _ptr(out_ind),
                            _ptr(out_x)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())
    return out_ptr, out_ind[:nnz], out_x


def _csr_mode(mode, drop_self=False):
    """``"distance"`` / ``"connectivity"`` (or an NND_CSR_* code) as nnd_graph_csr's ``mode``, NND_CSR_DROP_SELF or-ed in."""
    code = {"distance": NND_CSR_DISTANCE, "connectivity": NND_CSR_CONNECTIVITY}.get(mode, mode)
    if code not in (NND_CSR_DISTANCE, NND_CSR_CONNECTIVITY):
        raise ValueError("mode must be 'distance' or 'connectivity' (got %r)" % (mode,))
    return code | (NND_CSR_DROP_SELF if drop_self else 0)


def graph_csr(ids, vals, n, mode="distance", symmetric=False, drop_self=False, device=0, want_long_rows=False):
    """Host k-lists -> canonical CSR by the device kernels (``nnd_graph_csr``, csrc/csr_graph.hip): ``ids`` (m, k) int32 or int64
    with -1 for an empty place, ``vals`` (m, k) float32, ``n`` columns.  Returns (indptr int64 (m + 1), indices int32, data
    float32)[, rows of the symmetric union that took the long-row kernel]."""
    lib = load_library()
    ids = np.asarray(ids)
    ids = np.ascontiguousarray(ids, dtype=np.int64 if ids.dtype == np.int64 else np.int32)
    vals = np.ascontiguousarray(vals, dtype=np.float32)
    assert ids.ndim == 2 and vals.shape == ids.shape
    m, k = ids.shape
    cap = max(1, m * k * (2 if symmetric else 1))
    indptr, indices, data = np.empty(m + 1, np.int64), np.empty(cap, np.int32), np.empty(cap, np.float32)
    nnz, long_rows = C.c_int64(), C.c_int64()
    if lib.nnd_graph_csr(int(device), _ptr(ids), ids.dtype.itemsize, _ptr(vals), m, k, int(n), _csr_mode(mode, drop_self), 1 if symmetric else 0,
                         _ptr(indptr), _ptr(indices), _ptr(data), cap, C.byref(nnz), C.byref(long_rows)) != 0:
        raise NNDError(lib.nnd_last_global_error().decode())
    out = (indptr, indices[: nnz.value].copy(), data[: nnz.value].copy())
    return out + (int(long_rows.value),) if want_long_rows else out


class _DeviceBuffer:
    """A stretch of a ``DeviceCsr``'s memory as an object with ``__cuda_array_interface__``: ``torch.as_tensor`` wraps it without
    a copy and keeps this object -- and through it the owner -- alive as long as the tensor lives."""

    def __init__(self, owner, address, count, typestr):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(address), False), "strides": None,
                                         "version": 2}


class DeviceCsr:
    """Device k-lists -> canonical CSR where they lie (``nnd_graph_csr_device``): ``ids_ptr`` / ``vals_ptr`` are device addresses
    of an (m, k) int32 / int64 (``id_bytes``) and float32 array with row stride ``ld`` elements; queued on ``stream_ptr`` of
    ``device``, drained on return.  The object owns the three result arrays (freed with it): ``indptr`` (int64, m + 1),
    ``indices`` (int32, nnz), ``data`` (float32, nnz) are ``__cuda_array_interface__`` views of them; ``nnz``, ``long_rows``."""

    def __init__(self, device, stream_ptr, ids_ptr, id_bytes, vals_ptr, m, k, ld, n, mode="distance", symmetric=False, drop_self=False):
        self.lib = load_library()
        self._h = _H()
        dev = lambda p: C.c_void_p(int(p)) if p else None  # noqa: E731
        if self.lib.nnd_graph_csr_device(int(device), dev(stream_ptr), dev(ids_ptr), int(id_bytes), dev(vals_ptr), int(m), int(k), int(ld), int(n),
                                         _csr_mode(mode, drop_self), 1 if symmetric else 0, C.byref(self._h)) != 0:
            raise NNDError(self.lib.nnd_last_global_error().decode())
        indptr, indices, data, nnz, long_rows = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
        self.lib.nnd_csr_arrays(self._h, C.byref(indptr), C.byref(indices), C.byref(data), C.byref(nnz), C.byref(long_rows))
        self.m, self.n, self.nnz, self.long_rows = int(m), int(n), int(nnz.value), int(long_rows.value)
        self._addresses = (indptr.value, indices.value, data.value)

    # (made per read: a view kept on the object would be a reference cycle, and the arrays would wait for the collector)
    indptr = property(lambda self: _DeviceBuffer(self, self._addresses[0], self.m + 1, "<i8"))
    indices = property(lambda self: _DeviceBuffer(self, self._addresses[1], self.nnz, "<i4"))
    data = property(lambda self: _DeviceBuffer(self, self._addresses[2], self.nnz, "<f4"))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.lib.nnd_csr_destroy(self._h)
            self._h = _H()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
