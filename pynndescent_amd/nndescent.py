"""``NNDescent`` -- drop-in for the BUILD path of ``pynndescent.NNDescent`` on an MI355X.

Mirrors the reference constructor (pynndescent/pynndescent_.py:976-1269): same keyword arguments in
the same positional order, same derived defaults, same RandomState draw order, same attributes after
construction, same errors and warnings.  The dense euclidean / cosine branch
(pynndescent_.py:1221-1260) -- ``make_forest`` + ``rptree_leaf_array`` + ``nn_descent`` -- runs on
the GPU through the C ABI of ``include/pynnd_amd.h``.  Nothing here computes neighbours on the CPU:
if the HIP library or a gfx950 device is missing, construction raises.

Also on the GPU: ``update`` (warm start, pynndescent_.py:2381-2553), ``build_search_graph`` (the pruning
pass of ``_init_search_graph``, all diversify methods), ``prepare`` (hub search tree + reordering) and
``query``.  Metrics: euclidean / l2 / sqeuclidean / cosine / dot / inner_product / correlation / hellinger (hellinger input
must be non-negative: a negative entry raises ``ValueError``, where the reference computes NaN distances without a word) and
proxy_inner_product (graph and walk on the reference's proxy distance, queries reranked by the true inner product); and the
metrics that are euclidean after a fixed linear map of the rows, with ``metric_kwds`` read positionally as the reference reads
it: seuclidean / standardised_euclidean ``(V,)``, wminkowski / weighted_minkowski ``(w,)`` or ``(w, 2)``, mahalanobis ``(VI,)``
and minkowski ``()`` or ``(2,)`` (linear_map.py; the device transforms every row once, csrc/linear.hip); and the derived metrics
spearmanr (correlation of the rows' average ranks) and haversine (2-D rows ``(lat, lon)`` in radians: euclidean on their points of
the unit sphere, handed out as the angle), whose rows the device maps once as well (row_map.py, csrc/rowmap.hip).
Sparse input (any ``scipy.sparse`` matrix, for the metrics the reference's sparse path has too) is uploaded as CSR and made dense
on the device (sparse_input.py, csrc/sparse.hip); from there it is a device-resident index whose ``_raw_data`` is the CSR matrix.
Out of scope: sparse input whose dense rows do not fit the device or with ``n_devices`` > 1, torch sparse tensors, every other
metric, ``n_neighbors`` above 256 or
``max_candidates`` above 128 (``query``: more than 256 results per query).  Those raise ``NotImplementedError`` naming the reference entry point to use
instead; ``pynndescent_amd.make_index`` hands such inputs to ``pynndescent.NNDescent`` when it is importable.

This file holds the class and the helpers that read an index's ``__dict__``; the metric table is metrics.py, the tensor plumbing
device_arrays.py, the single-GPU build driver and ``nn_descent`` build.py, ``exact_knn`` exact.py.
"""
import inspect
from warnings import warn

import numpy as np
from sklearn.utils import check_array, check_random_state

from . import _capi, build, device_arrays, filtered, graph_export, linear_map, row_map, sparse_input, tags as tagwords
# Every name below was defined here once and is read here still (tests, tools/, and pickles, which name
# pynndescent_amd.nndescent.correct_alternative_*): the same objects as in their home modules.  Two are replaced by tests and
# are therefore CALLED through their home module alone -- ``build.ts()``, ``device_arrays._torch()``.
from .build import (EMPTY_GRAPH, _build_graph, _check_array_no_scan, _check_supported_sizes, _descend,  # noqa: F401
                    _raise_if_nonfinite, _reference_defaults, nn_descent, ts)
from .device_arrays import (_DEVICE_DTYPES, _check_device_array, _device_corrected, _DeviceInput, _DeviceLinear,  # noqa: F401
                            _DeviceRowsView, _dtype_name, _ids_to_host, _is_device_array, _OnTorchStream, _resolve_updated_indices,
                            _rows_to_host, _shape_of, _stream_ms, _torch, _update_dtype)
from .exact import _exact_knn_device, _exact_linear_rows, exact_knn  # noqa: F401
from .metrics import (_ANGULAR_METRICS, _BOOLEAN_METRICS, _DISTANCE_CORRECTIONS, _KNOWN_REFERENCE_METRICS,  # noqa: F401
                      _LINEAR_METRICS, _METRIC_TABLE, _METRICS, _ND_ALIASES, _ND_DISTS, _NEGATIVE_HELLINGER, _check_quantization,
                      _linear_map_of, _Metric, _metric_of, _metric_record, _no_exact_for_proxy, _raise_if_negative_host,
                      _refuse_uint8_and_sharding, correct_alternative_cosine, correct_alternative_hellinger,
                      correct_alternative_inner_product)

_refuse_with_linear = _refuse_uint8_and_sharding  # (its name before it said what it refuses)

INT32_MIN = np.iinfo(np.int32).min + 1  # pynndescent_.py:62
INT32_MAX = np.iinfo(np.int32).max - 1  # pynndescent_.py:63


def tau_rand_int(state):
    """Reference utils.py:17-40 on an int64[3] numpy state (used only to warm up search_rng_state)."""
    s = [int(v) for v in state]
    s[0] = (((s[0] & 4294967294) << 12) & 0xFFFFFFFF) ^ ((((s[0] << 13) & 0xFFFFFFFF) ^ s[0]) >> 19)
    s[1] = (((s[1] & 4294967288) << 4) & 0xFFFFFFFF) ^ ((((s[1] << 2) & 0xFFFFFFFF) ^ s[1]) >> 25)
    s[2] = (((s[2] & 4294967280) << 17) & 0xFFFFFFFF) ^ ((((s[2] << 3) & 0xFFFFFFFF) ^ s[2]) >> 11)
    state[0], state[1], state[2] = s
    r = (s[0] ^ s[1] ^ s[2]) & 0xFFFFFFFF
    return r - (1 << 32) if r >= (1 << 31) else r


def _proxy_search_k(k, proxy_beam_size):
    """``search_k`` of a query that is reranked (pynndescent_.py:2309-2312), within what the query kernel keeps."""
    search_k = proxy_beam_size * k
    if search_k < k:
        raise ValueError("proxy_beam_size must be at least 1 (got %r)" % (proxy_beam_size,))
    if search_k > 256:
        raise NotImplementedError("pynndescent_amd keeps proxy_beam_size * k <= 256 candidates per quantized query "
                                  "(got %d); use index.to_reference()" % search_k)
    return search_k


def uint8_codebook(raw, random_state):
    """The reference's uint8 codebook (pynndescent_.py:2193-2206) of the rows ``raw`` in their ORIGINAL order: a sample of
    min(10000, n) rows drawn by ``check_random_state(random_state)``; its distinct values when there are at most 256,
    else its quantiles at ``linspace(0, 1, 256)``; float32."""
    rs = check_random_state(random_state)
    sample = raw[rs.choice(raw.shape[0], min(10000, raw.shape[0]), replace=False)].ravel()
    unique = np.unique(sample)
    if len(unique) <= 256:
        return unique.astype(np.float32)
    return np.quantile(sample, np.linspace(0, 1, 256)).astype(np.float32)


def _updates_on_device(index, xs_fresh, xs_updated):
    """Whether ``update()`` of ``index`` stays on the device (``NNDescent._update_device``): the index holds its rows and its graph
    on one GPU, and at least one of the incoming arrays is a device array or a ``scipy.sparse`` matrix (made dense on the device),
    or the index was built from sparse input.  Reads ``__dict__`` only."""
    d = index.__dict__
    if "_device_data" not in d or "_device_graph" not in d or int(d.get("n_devices", 1)) != 1:
        return False
    if d.get("_is_sparse"):  # (a sparse index has no host rows to fall back on: every update is assembled on the device)
        return True
    return any(_is_device_array(a) or sparse_input.is_sparse(a) for a in (xs_fresh, xs_updated))


def _prepares_on_device(index):
    """Whether ``prepare()`` of ``index`` runs from its device tensors (``NNDescent._init_search_graph_device``): an index built
    from a device array on one GPU that still holds its rows and its graph there, a graph within the device pass's edge
    positions, and no reason to go through the host -- the ``_host_prepare`` switch, or dot with uint8 codes (they are the codes
    of rows other than the searcher's own copy).  Reads ``__dict__`` only: no host mirror is fetched by asking."""
    from .search_graph import DEVICE_PASS_MAX_EDGES

    d = index.__dict__
    if d.get("_host_prepare", getattr(type(index), "_host_prepare", False)):
        return False
    if "_device_data" not in d or "_device_graph" not in d or int(d.get("n_devices", 1)) != 1:
        return False
    if d.get("quantization") == "uint8" and _metric_of(d["metric"]).normalize:
        return False
    n, k = (int(v) for v in d["_device_graph"][0].shape)
    return 2 * n * k < DEVICE_PASS_MAX_EDGES


class _DeviceForestSentinel:
    """Stands in for ``_rp_forest``: downstream reference code only null-checks it
    (pynndescent_.py:1353) -- the build consumes nothing but the leaf array."""

    def __init__(self, n_trees, n_leaves, max_leaf_size):
        self.n_trees, self.n_leaves, self.max_leaf_size = n_trees, n_leaves, max_leaf_size

    def __len__(self):
        return self.n_trees


class NNDescent:
    """See ``pynndescent.NNDescent``; constructor signature identical (pynndescent_.py:976-1007)."""

    # the host-path switch of prepare(): set ``index._host_prepare = True`` on an index built from a device array and its
    # prepare() takes the path of a host-built index (mirrors fetched, scipy reorder, three uploads) -- tests and
    # tools/ab/device_prepare_timing.py compare the two paths on one and the same graph with it
    _host_prepare = False

    def __init__(
        self,
        data,
        metric="euclidean",
        metric_kwds=None,
        bit_metric=False,
        n_neighbors=30,
        n_trees=None,
        angular_trees=False,
        leaf_size=None,
        pruning_degree_multiplier=1.5,
        diversify_prob=1.0,
        diversify_method="standard",
        degree_prune_aggressiveness=1.0,
        n_search_trees=1,
        search_tree_leaf_size=None,
        max_search_tree_depth=None,
        quantization=None,
        tree_init=True,
        init_graph=None,
        init_dist=None,
        random_state=None,
        low_memory=True,
        max_candidates=None,
        max_rptree_depth=200,
        n_iters=None,
        delta=0.001,
        n_jobs=None,
        compressed=False,
        parallel_batch_queries=False,
        verbose=False,
        device=0,
        n_devices=1,
        devices=None,
    ):
        """``device``: HIP ordinal of the GPU that builds the index.  ``n_devices`` > 1: the build is row-sharded over that
        many GPUs of this node (``nnd_build_multi``: one host thread per GPU inside the library, RCCL over xGMI; the
        reference's analogue is ``n_jobs``, pynndescent_.py:1141-1143); ``devices`` lists their ordinals (default
        0..n_devices-1; a list that repeats an ordinal puts several ranks on one GPU).  Everything after the build
        (``prepare``, ``query``, ``update``) runs on ``device``.

        ``data`` may be a device array -- a 2-D ``torch.Tensor`` on a HIP device, float32 / float16 / bfloat16 / float64 (half
        precision and float64 are converted to float32 on the device; a float32 tensor is kept by reference, not copied).
        The index then runs on the tensor's device and on torch's current stream: data queued on that stream needs no
        synchronisation, and ``neighbor_graph`` / ``query(device array)`` return tensors there, corrected on the device.
        ``prepare()`` -- and so the first ``query()`` -- runs from those tensors too (hub rank, tree, pruning pass, reorder and
        the searcher's fill on the device: only the tree's tables, ``_vertex_order`` and scalars cross the bus; dot with
        ``quantization="uint8"`` takes the host path).  ``_raw_data``, ``_neighbor_graph``, ``_search_graph`` and
        ``_quantized_data`` are host mirrors fetched on first use; ``build_search_graph``, pickling and ``to_reference`` work
        through them.  ``update()`` with a tensor and ``recall()`` stay on the device (``_update_device``, ``_recall_device``);
        ``update()`` with host arrays alone makes the index a host index.  ``init_graph`` / ``init_dist`` may be tensors as well:
        with device ``data`` on one GPU they are cast to int32 / float32 on the device and seed the build where they are
        (``nnd_init_from_graph_device``); in every other combination they are brought to the host.  Out of scope: the hub
        tree's FlatTree assembly on the device; producers other than torch (``__cuda_array_interface__``, DLPack); and a sharded
        build from device memory -- with ``n_devices`` > 1 the rows are brought to the host first and the index is a host index,
        as for host input.

        ``data`` may be a ``scipy.sparse`` matrix or array (sparse_input.py): made canonical float32 CSR on the host, uploaded as
        CSR and written dense on ``device`` by one kernel, after which it is the float32 tensor of the paragraph above in every
        respect but two -- ``_raw_data`` is the CSR matrix (``_is_sparse`` is True; no dense host mirror is ever made), and the
        answers are numpy arrays.  ``NotImplementedError`` when the dense rows and their prepared copy do not fit the free device
        memory, or with ``n_devices`` > 1; the reference's ``ValueError`` for a metric its sparse path lacks."""
        dev_checked = None
        if _is_device_array(data):  # dtype, shape and device first: before any device work, and before the shape is read
            dev_checked = _check_device_array(data, device)
            data, device = dev_checked[0], dev_checked[2]
        # init_graph / init_dist tensors seed a device build where they are (cast on torch's stream here, before the builder's
        # stream is taken from it); every other combination meets on the host
        if dev_checked is not None and int(n_devices) == 1 and _is_device_array(init_graph) and (init_dist is None or _is_device_array(init_dist)):
            torch = device_arrays._torch()
            init_graph = init_graph.detach().to(device=data.device, dtype=torch.int32).contiguous()
            if init_dist is not None:
                init_dist = init_dist.detach().to(device=data.device, dtype=torch.float32).contiguous()
        else:
            init_graph, init_dist = _ids_to_host(init_graph), _ids_to_host(init_dist)
        n_trees, n_iters, eff_leaf_size, eff_max_candidates = _reference_defaults(
            data.shape[0], n_neighbors, n_trees, n_iters, leaf_size, max_candidates)

        self.n_trees = n_trees
        self.angular_trees = angular_trees
        self.n_trees_after_update = max(2, int(np.round(self.n_trees / 3)))
        self.n_neighbors = n_neighbors
        self.metric = metric
        self.metric_kwds = metric_kwds
        self.bit_metric = bit_metric
        self.leaf_size = leaf_size
        self.prune_degree_multiplier = pruning_degree_multiplier
        self.diversify_prob = diversify_prob
        self.diversify_method = diversify_method
        self.degree_prune_aggressiveness = degree_prune_aggressiveness
        self.n_search_trees = n_search_trees
        self.search_tree_leaf_size = search_tree_leaf_size
        self.max_search_tree_depth = max_search_tree_depth
        self.max_rptree_depth = max_rptree_depth
        self.max_candidates = max_candidates
        self.quantization = quantization
        self.low_memory = low_memory
        self.n_iters = n_iters
        self.delta = delta
        self.dim = data.shape[1]
        self.n_jobs = n_jobs
        self.compressed = compressed
        self.parallel_batch_queries = parallel_batch_queries
        self.verbose = verbose
        self.device = device
        self.n_devices = int(n_devices)
        self.devices = None if devices is None else [int(v) for v in devices]
        if self.n_devices < 1 or (self.devices is not None and len(self.devices) != self.n_devices):
            raise ValueError("n_devices must be >= 1 and match len(devices)")

        m = _metric_record(metric)
        lin = _linear_map_of(metric, m, metric_kwds, data.shape[1])  # (host only: every error of metric_kwds comes first)
        _refuse_uint8_and_sharding(metric, m, quantization, self.n_devices)
        sparse = sparse_input.is_sparse(data)
        if sparse:  # the metric rule of sparse input, decided before any device work
            sparse_input.check_sparse_metric(metric, self.n_devices)

        _check_supported_sizes(n_neighbors, max_candidates, init_graph)
        csr = None
        if sparse:  # the CSR arrays go up and are made dense there: from here on the input is a float32 device array
            csr = sparse_input.canonical_csr(data)
            data = sparse_input.dense_rows_on_device(csr, device, check_fit=True)
            dev_checked = _check_device_array(data, device)
        # pynndescent_.py:1054 check_array(data, dtype=np.float32, order="C") -- minus its single-core scan for NaN / inf
        # (24 ms at 1 M x 128): the prep kernel looks at every value anyway and raises a flag; _raise_if_nonfinite then
        # lets sklearn produce the reference's own error
        # pynndescent_.py:1041-1046: a float32 C-contiguous input is the caller's own array after check_array -- normalised
        # into a copy; any other input has been copied by check_array already and is normalised in place
        dev_in = None
        if dev_checked is not None:
            _, dtype_code, ordinal = dev_checked
            if self.n_devices > 1:  # the sharded build takes its rows from the host, as for host input
                data = np.ascontiguousarray(data.detach().float().cpu().numpy())
            else:
                dev_in = _DeviceInput(data, dtype_code, ordinal, n_neighbors)
        copy_on_normalize = getattr(data, "dtype", None) == np.float32 and bool(getattr(getattr(data, "flags", None), "c_contiguous", False))
        if dev_in is None:
            data = _check_array_no_scan(data)
        self.tree_init = not (not tree_init or n_trees == 0 or init_graph is not None)  # pynndescent_.py:1059-1062
        self._dist_args = tuple((metric_kwds or {}).values())
        current_random_state = self._set_up(None if dev_in is not None else data, m, random_state, copy_on_normalize)
        if csr is not None:  # pynndescent_.py:1114-1116: the index holds the CSR matrix, never dense rows
            self._is_sparse, self._raw_data = True, csr
        if dev_in is None:
            data = self._raw_data
        self._linear_map = None
        if m.row_map is not None:  # (the mapped rows are finite whatever the input holds: the prep kernel's flag cannot tell)
            device_arrays._assert_all_finite(data)
        if lin is not None:  # the shift is fixed here, once; the device builds on the transformed copy, _raw_data stays the caller's
            # (_linear_map: the index's LinearMap, or the RowMap of a derived metric -- one attribute, one set of code paths)
            self._linear_map = lin = row_map.with_shift(lin, data if dev_in is None else _DeviceRowsView(data))
            if dev_in is None:
                data = self._lin_data = row_map.rows_host(lin, data, device=device)
            else:
                dev_in.linear = self._linear_on_device(data.device)

        n = data.shape[0]
        if self.tree_init:
            if verbose:
                print(build.ts(), "Building RP forest with", str(n_trees), "trees")
            tree_states = current_random_state.randint(INT32_MIN, INT32_MAX, size=(n_trees, 3)).astype(np.int64)
            eff_trees = n_trees
        else:
            tree_states = np.zeros((1, 3), np.int64)
            eff_trees = 0

        if init_graph is not None:
            if not _is_device_array(init_graph):
                init_graph = np.asarray(init_graph)
            if init_graph.shape[0] != n:
                raise ValueError("Init graph size does not match dataset size!")  # pynndescent_.py:1229
            if init_dist is not None and tuple(init_graph.shape) != _shape_of(init_dist):
                raise ValueError("The shapes of init graph and init distances do not match!")  # pynndescent_.py:1236

        if self.n_devices > 1:  # (a build that starts from init_graph is sharded too -- nnd_build_multi_from_graph)
            n_leaves = self._build_multi(data, eff_trees, eff_leaf_size, eff_max_candidates, tree_states[0], verbose,
                                         init_graph=init_graph, init_dist=init_dist)
        else:
            graph, self._build_stats, n_leaves = _build_graph(
                data, m, n_neighbors, eff_trees, eff_leaf_size, max_rptree_depth, eff_max_candidates, n_iters, delta,
                self.rng_state, tree_states[0], device, forest=self.tree_init, init_graph=init_graph, init_dist=init_dist,
                random_fill=init_graph is None, check_finite=True, verbose=verbose, announce=verbose, dev_in=dev_in)
            if dev_in is None:
                self._neighbor_graph = graph
            else:  # the graph and the rows stay on the device; _neighbor_graph / _raw_data are fetched when first read
                self._device_graph, self._device_data = graph, dev_in.rows
                if dev_in.linear is not None:  # _device_data: the transformed rows the device works on; the caller's tensor stays
                    self._device_raw = dev_in.tensor
        self._rp_forest = _DeviceForestSentinel(n_trees, n_leaves, eff_leaf_size) if self.tree_init else None

        # pynndescent_.py:1262-1267 `np.any(indices < 0)`: rows are ascending with the unfilled entries (-1, +inf) at the
        # tail, so the last column tells (1 M strided reads instead of a 15 M-element temporary; on the device: one scalar back)
        if dev_in is not None:
            unfilled = bool((self._device_graph[0][:, -1].min() < 0).item())
        else:
            unfilled = self._neighbor_graph[0][:, -1].min() < 0
        if unfilled:
            warn(
                "Failed to correctly find n_neighbors for some samples."
                " Results may be less than ideal. Try re-running with"
                " different parameters."
            )

    def _set_up(self, data, m, random_state, copy):
        """What the constructor and ``from_graph`` share (pynndescent_.py:1064-1113): the data the index holds (dot: rows
        L2-normalised, into a new array when ``copy``; ``data`` None: the rows are on the device), the metric's correction and tree flags, and ``rng_state`` /
        ``search_rng_state`` drawn in the reference's order.  Returns the RandomState, whose next draws are the trees'."""
        if data is not None and m.normalize:  # pynndescent_.py:1101-1102
            from sklearn.preprocessing import normalize

            data = normalize(data, norm="l2", copy=copy)
        self._input_dtype = np.float32
        if data is not None:  # (None: a device array -- _raw_data is its host mirror, fetched by __getattr__)
            self._raw_data = data
        self.random_state = random_state
        current_random_state = check_random_state(random_state)
        self._distance_correction = m.correction
        self._distance_func = None  # device kernels; see include/pynnd_amd.h NND_METRIC_*
        self._is_proxy_distance = m.proxy  # pynndescent_.py:1272-1280 (the true distance: the rerank of csrc/query.hip)
        self._angular_trees = m.angular
        self._bit_trees = False
        self._is_sparse = False
        # RandomState draw order of the reference: rng_state, search_rng_state, then the per-tree
        # states inside make_forest (pynndescent_.py:1105-1113, rp_trees.py:2850)
        self.rng_state = current_random_state.randint(INT32_MIN, INT32_MAX, 3).astype(np.int64)
        self.search_rng_state = current_random_state.randint(INT32_MIN, INT32_MAX, 3).astype(np.int64)
        for _ in range(10):
            tau_rand_int(self.search_rng_state)
        return current_random_state

    def _build_multi(self, data, n_trees, leaf_size, max_candidates, tree_state, verbose, init_graph=None, init_dist=None,
                     old_graph=None):
        """Row-sharded build over several GPUs, one call into the library (include/pynnd_amd.h nnd_build_multi): from a
        forest, from ``init_graph`` / ``init_dist``, or from a forest and ``old_graph`` (``update()``).  Sets the graph
        and the stats; returns the forest's leaf count."""
        from sklearn.utils import assert_all_finite

        from . import sharded

        assert_all_finite(data)  # check_array's scan (pynndescent_.py:1054): the one-call multi-GPU build has no flag to read
        _raise_if_negative_host(data, _metric_of(self.metric))
        if verbose:
            print(build.ts(), "NN descent for", str(self.n_iters), "iterations on", self.n_devices, "GPUs")
        idx, dst, st, info = sharded.build_multi(
            data, self.n_devices, self.devices, self.metric, self.n_neighbors, n_trees, leaf_size, max_candidates,
            self.n_iters, self.delta, max_rptree_depth=self.max_rptree_depth, rng_state=self.rng_state,
            tree_state=tree_state, init_graph=init_graph, init_dist=init_dist, old_graph=old_graph)
        self._neighbor_graph = (idx, dst)
        self._build_stats = st
        self._shard_info = info
        if verbose:
            for it, c in enumerate(info["c"]):
                print("\t", it + 1, " / ", self.n_iters, " c =", c)
        return st["n_leaves"]

    @property
    def neighbor_graph(self):
        """pynndescent_.py:2145-2158: copies, with the distance correction applied."""
        if self.compressed and not hasattr(self, "_neighbor_graph"):
            warn("Compressed indexes do not have neighbor graph information.")
            return None
        # built from a device array: fresh tensors there, corrected by the library (scipy input gets numpy answers: the mirror's)
        if "_device_graph" in self.__dict__ and not self.__dict__.get("_is_sparse"):
            torch = device_arrays._torch()
            idx, dist = self._device_graph
            with torch.cuda.device(self.device):
                return idx.clone(), _device_corrected(torch, dist, _metric_of(self.metric), self.device)
        return (_capi.host_copy(self._neighbor_graph[0]), self._distance_correction(self._neighbor_graph[1]))

    def __getattr__(self, name):
        """The host mirrors of an index built from a device array, fetched on first access and cached: ``_raw_data`` (float32
        numpy rows; dot: the normalised rows the device computed; after a device prepare: in the search tree's leaf order, as
        the host path leaves them) and ``_neighbor_graph`` (numpy int32 / float32); after a device prepare also ``_search_graph``
        (scipy CSR uint8, sorted indices) and ``_quantized_data`` (the searcher's uint8 codes).  Every line that reads the names
        finds them as on a host-built index, and ``hasattr`` keeps its meaning."""
        d = self.__dict__
        if name == "_raw_data" and d.get("_is_sparse"):  # (a sparse index holds its CSR matrix itself: there is no dense mirror)
            raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))
        if name in ("_raw_data", "_lin_data") and "_device_data" in d and (name == "_raw_data" or d.get("_linear_map") is not None):
            # (a metric with a linear map: _device_data holds the transformed rows, _device_raw the caller's)
            rows = d["_device_raw" if name == "_raw_data" and "_device_raw" in d else "_device_data"].detach()
            if "_device_order" in d:  # x_new[i] = x[order[i]]: the gather the searcher's fill makes
                rows = rows[d["_device_order"].long()]
            value = np.ascontiguousarray(rows.float().cpu().numpy())
        elif name == "_lin_data" and d.get("_linear_map") is not None:
            # the transformed rows of a host index that has none at hand (unpickled, from_graph): a row's transform depends on
            # the row alone, so transforming _raw_data again gives the bits the index was built on, in _raw_data's order
            lin = d["_linear_map"]
            value = row_map.rows_host(lin, self._raw_data, device=self.device)
        elif name == "_neighbor_graph" and "_device_graph" in d:
            value = tuple(np.ascontiguousarray(t.cpu().numpy()) for t in d["_device_graph"])
        elif name == "_search_graph" and "_device_search_graph" in d:
            import scipy.sparse as sp

            indptr, indices = (np.ascontiguousarray(t.cpu().numpy()) for t in d["_device_search_graph"])
            n = indptr.shape[0] - 1
            value = sp.csr_array((np.ones(indices.shape[0], np.uint8), indices, indptr), shape=(n, n))
            value.has_sorted_indices = True
        elif (name == "_quantized_data" and "_device_search_graph" in d and d.get("_searcher") is not None
              and d["_searcher"].has_codes):  # the codes the searcher derived from its own rows, deterministic: derived again
            value = d["_searcher"].quantize_u8(d["_quantized_values"], rows=None)
        else:
            raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))
        d[name] = value
        return value

    # The names of an index's device-resident and derived state, by group; the sites that drop state are unions of these.
    # the device tensors: what a build from a device array leaves, and what a device prepare adds to it
    _DEVICE_PREPARED = ("_device_order", "_device_search_graph", "_device_prepare_stats")
    _DEVICE_TENSORS = ("_device_graph", "_device_data", "_device_raw") + _DEVICE_PREPARED
    # the copies made of ``_linear_map``: the map as tensors (``_linear_on_device``) and the transformed rows
    _LINEAR_COPIES = ("_device_linear", "_lin_data")
    # what ``prepare()`` derives from the rows and the graph
    _SEARCH_STRUCTURES = ("_search_graph", "_search_forest", "_vertex_order", "_searcher")
    # what ``__getattr__`` fetches from the device tensors on first read
    _HOST_MIRRORS = ("_raw_data", "_lin_data", "_neighbor_graph", "_search_graph", "_quantized_data")

    def _drop_device_copies(self):
        """After the host mirrors have become the truth (``update()``), or for a pickle: the device tensors go.  ``_device_linear``
        stays: the map does not change with the rows, and a device query of the host index uses it again."""
        for name in self._DEVICE_TENSORS:
            self.__dict__.pop(name, None)

    def _kernel_metric(self):
        """The metric name the kernels run: the index's own, euclidean on the transformed rows of a linear map, or the base
        metric of a derived one on its mapped rows."""
        return _metric_of(self.metric).kernel_metric or self.metric

    def _mapped_record(self):
        """For ``exact_knn`` on rows a row map has made already: the derived metric's record (the base metric's kernels, its own
        correction); None for every other metric, whose ``_kernel_metric()`` says it all."""
        m = _metric_of(self.metric)
        return m if m.row_map is not None else None

    def _work_rows(self):
        """The host rows the device works on: ``_raw_data``, its transformed copy ``_lin_data`` for a metric with a linear map, or
        the dense form of a sparse index's CSR matrix (a row's dense form depends on the row alone: the bits the device made)."""
        if self.__dict__.get("_is_sparse"):  # (the host path of a sparse index, e.g. an unpickled one: dense for this call, not kept)
            return np.ascontiguousarray(self._raw_data.toarray(), dtype=np.float32)
        return self._lin_data if self.__dict__.get("_linear_map") is not None else self._raw_data

    def _linear_on_device(self, device):
        """The index's linear map as tensors on ``device`` (a ``_DeviceLinear``; a derived metric: its ``_DeviceRowMap``), uploaded
        once."""
        d = self.__dict__
        if d.get("_device_linear") is None:
            ordinal = getattr(device, "index", None)
            d["_device_linear"] = device_arrays._device_map(d["_linear_map"], device, int(self.device) if ordinal is None else ordinal)
        return d["_device_linear"]

    @property
    def _prepared(self):
        """Whether ``_init_search_graph`` has run (``_vertex_order`` is set eagerly on both paths).  Looks at ``__dict__``: asking
        fetches no host mirror."""
        return "_vertex_order" in self.__dict__

    @staticmethod
    def _recall_rows(n, n_rows, random_state):
        """The rows ``recall`` samples: ``RandomState(random_state).choice(n, min(n_rows, n), replace=False)``."""
        return np.random.RandomState(random_state).choice(int(n), size=min(int(n_rows), int(n)), replace=False).astype(np.int64)

    def recall(self, k=None, n_rows=1000, random_state=None):
        """How good the graph is: the share of the true ``k`` nearest neighbours (self included; ``k`` defaults to
        ``min(10, n_neighbors)``) that appear anywhere in the graph's row, averaged over ``min(n_rows, n)`` distinct rows
        drawn by ``_recall_rows`` -- the convention of the reference's tests (tests/test_pynndescent_.py:27-31).  The truth
        is the exact brute-force search of ``exact_knn`` over the index's data; only the data and the graph are read, so
        every way of making the index (one or several devices, ``from_graph``, after ``update()``) is covered.  An index built
        from a device array on one GPU is measured where it is: the exact search and the count run on its tensors, the sampled
        row ids go up and one integer comes back (the same value, and no host mirror is fetched).  dot: the truth is searched
        on rows normalised once more -- by the device there, by sklearn on the host path -- which agree within rounding only,
        so the two paths may differ where two true neighbours are that close; every other metric gives the same value."""
        _no_exact_for_proxy(self.metric, _metric_of(self.metric), "NNDescent.recall")
        d = self.__dict__
        if d.get("_is_sparse"):  # (an unpickled one: its rows and its graph go up again first)
            self._sparse_to_device()
        if "_device_data" in d and "_device_graph" in d and int(d.get("n_devices", 1)) == 1:
            return self._recall_device(k, n_rows, random_state)
        graph_idx = self._neighbor_graph[0]
        n = graph_idx.shape[0]
        k = min(10, int(self.n_neighbors)) if k is None else int(k)
        rows = self._recall_rows(n, n_rows, random_state)
        data = self._work_rows()  # (a metric with a linear map: the truth is euclidean on the transformed rows)
        if hasattr(self, "_vertex_order"):  # prepare() keeps the rows in the search tree's leaf order; the graph keeps its numbering
            data = data[np.argsort(self._vertex_order), :]
        true_idx = exact_knn(data, k=k, metric=self._kernel_metric(), rows=rows, device=getattr(self, "device", 0))[0]
        hits = sum(int(np.isin(t, a).sum()) for t, a in zip(true_idx, graph_idx[rows]))
        return hits / float(true_idx.shape[0] * k)

    def _recall_device(self, k, n_rows, random_state):
        """``recall`` of an index that holds its rows and its graph on the device: the sampled ids go up, the exact search runs on
        the tensors (``_device_data`` keeps the original order through ``prepare()``), one wave per sampled row counts the true ids
        found in the graph's row, and one integer comes back.  No host mirror is read or made."""
        torch, d = device_arrays._torch(), self.__dict__
        data, gidx = d["_device_data"], d["_device_graph"][0]
        n, ordinal = int(gidx.shape[0]), int(self.device)
        k = min(10, int(self.n_neighbors)) if k is None else int(k)
        rows = self._recall_rows(n, n_rows, random_state)
        with torch.cuda.device(ordinal):
            rows_dev = torch.from_numpy(rows.astype(np.int32)).to(data.device)
            true_idx = _exact_knn_device(data, None, k, self.metric, _metric_of(self.metric), rows_dev, ordinal, False)[0]
            hits = torch.empty((1,), dtype=torch.int64, device=data.device)
            _capi.device_recall_hits(ordinal, torch.cuda.current_stream(ordinal).cuda_stream, true_idx.data_ptr(), true_idx.shape[0], k,
                                     gidx.data_ptr(), n, gidx.shape[1], rows_dev.data_ptr(), hits.data_ptr())
            return int(hits.item()) / float(true_idx.shape[0] * k)

    def build_search_graph(self):
        """The pruning pass of ``_init_search_graph`` (pynndescent_.py:1451-1611: diversify, reverse diversify,
        degree prune) on the GPU alone; returns the CSR uint8 graph in the ORIGINAL vertex numbering (``prepare()``
        runs the same pass and then re-indexes everything by the hub search tree's leaf order)."""
        from .search_graph import build_search_graph

        if self._prepared:
            raise RuntimeError("the index is prepared already: its search graph is index._search_graph (in leaf order)")
        self._pruned_graph = build_search_graph(
            self._work_rows(), self._neighbor_graph[0], self._neighbor_graph[1], self._kernel_metric(), self.n_neighbors,
            self.prune_degree_multiplier, self.diversify_prob, self.diversify_method,
            degree_prune_aggressiveness=self.degree_prune_aggressiveness,
            seed=int(self.rng_state[0]) & 0xFFFFFFFF, device=self.device)
        return self._pruned_graph

    # attributes of the reference class that prepare() / query() / update() read (pynndescent_.py:1014-1113)
    _HANDOVER = (
        "n_trees", "angular_trees", "n_trees_after_update", "n_neighbors", "metric", "metric_kwds", "bit_metric",
        "leaf_size", "prune_degree_multiplier", "diversify_prob", "diversify_method", "degree_prune_aggressiveness",
        "n_search_trees", "search_tree_leaf_size", "max_search_tree_depth", "max_rptree_depth", "max_candidates",
        "quantization", "low_memory", "n_iters", "delta", "dim", "n_jobs", "compressed", "parallel_batch_queries",
        "verbose", "_input_dtype", "_raw_data", "tree_init", "_dist_args", "random_state", "_angular_trees",
        "_bit_trees", "_is_sparse", "rng_state", "search_rng_state", "_rp_forest",
    )

    def to_reference(self):
        """Hand the GPU-built index to ``pynndescent.NNDescent`` (must be importable) WITHOUT rebuilding: the returned
        object carries this index's data, graph and parameters, so the reference's own ``prepare()`` (hub search tree,
        pruned + reordered search graph) and ``query()`` run on it unchanged.  The reference only null-checks
        ``_rp_forest`` before building its hub tree from the graph (pynndescent_.py:1353-1437).

        seuclidean / wminkowski / mahalanobis / minkowski: the reference keeps no squared space for them, so the graph handed
        over holds true distances, and the search structures of a prepared index are LEFT OUT of the hand-over (its tree's
        hyperplanes split the transformed space, the reference's tree descent takes raw queries): the rows go back to their
        original order and the reference's own ``prepare()`` rebuilds tree and search graph from the graph.  spearmanr /
        haversine: the same, for the same reason (the graph's distances go over as the metric's own, float32)."""
        if self.__dict__.get("_is_sparse"):
            raise NotImplementedError("to_reference() of an index built from sparse input: the reference's sparse search "
                                      "structures (sparse hub tree, sparse distances) are not produced; build with pynndescent.NNDescent")
        import pynndescent

        m = _metric_of(self.metric)
        linear = m.mapped
        ref = object.__new__(pynndescent.NNDescent)
        for name in self._HANDOVER:
            if hasattr(self, name):
                setattr(ref, name, getattr(self, name))
        if linear and self._prepared:
            ref._raw_data = np.ascontiguousarray(self._raw_data[np.argsort(self._vertex_order), :])
        if hasattr(self, "_neighbor_graph"):
            dist = self._neighbor_graph[1]
            if linear:  # true distances: sqrt of the code-0 value, or the derived metric's own correction
                dist = np.sqrt(dist) if m.linear else m.correction(dist).astype(np.float32)
            ref._neighbor_graph = (self._neighbor_graph[0].copy(), dist.copy() if not linear else dist)
        ref._distance_correction = None
        ref._set_distance_func()  # pynndescent_.py:1271-1298: numba distance, correction, proxy flags
        if hasattr(self, "_search_graph") and not linear:  # prepared on the GPU: the reference's prepare() has nothing left to build
            from pynndescent.rp_trees import FlatTree as RefFlatTree

            ref._search_graph = self._search_graph.copy()
            ref._search_forest = [RefFlatTree(*t) for t in self._search_forest]
            ref._vertex_order = np.asarray(self._vertex_order).copy()
            ref._min_distance = self._min_distance
            ref._visited = np.zeros_like(self._visited)
            if hasattr(ref, "_rp_forest"):
                del ref._rp_forest
        return ref

    @classmethod
    def from_graph(cls, data, indices, distances, metric="euclidean", random_state=None, **kwargs):
        """An index object around an existing k-NN graph (``distances`` in the alternative space, rows ascending), no
        build: the starting point for ``update()`` / ``build_search_graph()`` / ``to_reference()``."""
        self = object.__new__(cls)
        data = check_array(data, dtype=np.float32, order="C")
        n = data.shape[0]
        if "pruning_degree_multiplier" in kwargs:  # the constructor's name for prune_degree_multiplier
            kwargs["prune_degree_multiplier"] = kwargs.pop("pruning_degree_multiplier")
        unknown = set(kwargs) - set(_FROM_GRAPH_DEFAULTS)
        if unknown:
            raise TypeError("unexpected arguments: %s" % sorted(unknown))
        for name, value in dict(_FROM_GRAPH_DEFAULTS, **kwargs).items():
            setattr(self, name, value)
        m = _metric_record(metric, reference_fallback=False)
        indices = np.ascontiguousarray(indices, np.int32)
        distances = np.ascontiguousarray(distances, np.float32)
        if indices.shape != distances.shape or indices.shape[0] != n:
            raise ValueError("Init graph size does not match dataset size!")
        _check_supported_sizes(indices.shape[1], self.max_candidates, None)
        _raise_if_negative_host(data, m)
        self.metric, self.n_neighbors = metric, indices.shape[1]
        self.n_trees, self.n_iters, _, _ = _reference_defaults(n, self.n_neighbors, self.n_trees, self.n_iters)
        self.n_trees_after_update = max(2, int(np.round(self.n_trees / 3)))
        self.dim = data.shape[1]
        self.tree_init = True
        self._dist_args = tuple((self.metric_kwds or {}).values())
        lin = _linear_map_of(metric, m, self.metric_kwds, data.shape[1])
        _refuse_uint8_and_sharding(metric, m, self.quantization, 1)
        self._set_up(data, m, random_state, copy=True)  # (dot: the data NNDescent would hold, in a new array)
        # (``distances`` of a metric with a linear map: squared, of the rows transformed with this shift -- what the build keeps)
        self._linear_map = None if lin is None else row_map.with_shift(lin, self._raw_data)
        self._rp_forest = _DeviceForestSentinel(self.n_trees, 0, 0)
        self._neighbor_graph = (indices, distances)
        return self

    # ------------------------------------------------------------------------------------------------ prepare / query
    def _init_search_graph(self):
        """``NNDescent._init_search_graph`` (pynndescent_.py:1333-1662) on the GPU: the hub search tree built from the
        data and the finished graph (csrc/hubtree.hip), the pruning pass (csrc/prune.hip), then data, graph and tree
        re-indexed by the tree's leaf order (pynndescent_.py:1629-1651)."""
        from .search_graph import build_search_graph
        from .search_tree import make_hub_tree, reorder_by_tree

        search_leaf_size = (self.search_tree_leaf_size if self.search_tree_leaf_size is not None
                            else (self.leaf_size if self.leaf_size is not None else 30))  # pynndescent_.py:1341-1345
        search_tree_depth = (self.max_search_tree_depth if self.max_search_tree_depth is not None
                             else self.max_rptree_depth)                                   # pynndescent_.py:1346-1350
        if _prepares_on_device(self):
            try:
                return self._init_search_graph_device(search_leaf_size, search_tree_depth)
            except _capi.NNDError as e:
                if "memory" not in str(e).lower():
                    raise
                warn("the search-graph pass does not fit the device (%s): preparing through the host" % e)
        if not hasattr(self, "_search_forest"):
            if getattr(self, "_rp_forest", None) is None and not self.tree_init:
                self._search_forest = []  # pynndescent_.py:1377-1378: no tree, queries start from random vertices
            else:
                if self.verbose:
                    print(build.ts(), "Building hub-based search tree")
                self._search_forest = [make_hub_tree(self._work_rows(), self._neighbor_graph[0], self._kernel_metric(), search_leaf_size,
                                                     search_tree_depth, device=self.device,
                                                     seed=int(self.rng_state[0]) & 0x7FFFFFFF)]
                self._rp_forest = None  # the reference deletes it here (pynndescent_.py:1444)
        if self.verbose:
            print(build.ts(), "Diversifying and pruning the search graph")
        graph, stages = build_search_graph(
            self._work_rows(), self._neighbor_graph[0], self._neighbor_graph[1], self._kernel_metric(), self.n_neighbors,
            self.prune_degree_multiplier, self.diversify_prob, self.diversify_method,
            degree_prune_aggressiveness=self.degree_prune_aggressiveness, seed=int(self.rng_state[0]) & 0xFFFFFFFF,
            device=self.device, return_stages=True)
        self._min_distance = np.float32(stages["min_distance"])                     # pynndescent_.py:1539
        self._visited = np.zeros((self._raw_data.shape[0] // 8) + 1, dtype=np.uint8, order="C")  # pynndescent_.py:1624-1626
        if self.verbose:
            print(build.ts(), "Resorting data and graph based on tree order")
        if self._search_forest:
            graph, data, self._vertex_order, tree = reorder_by_tree(graph, self._work_rows(), self._search_forest[0])
            if self.__dict__.get("_linear_map") is not None:  # both copies in the leaf order
                self._lin_data, self._raw_data = data, np.ascontiguousarray(self._raw_data[self._vertex_order, :])
            elif self.__dict__.get("_is_sparse"):  # pynndescent_.py:1630: the CSR rows in the leaf order
                self._raw_data = self._raw_data[self._vertex_order, :]
            else:
                self._raw_data = data
            self._search_forest = [tree] + list(self._search_forest[1: self.n_search_trees])
        else:
            self._vertex_order = np.arange(self._raw_data.shape[0])
        self._search_graph = graph
        self._searcher = None
        if self.compressed:  # pynndescent_.py:1653-1658
            if hasattr(self, "_rp_forest"):
                del self._rp_forest
            del self._neighbor_graph
            self.__dict__.pop("_device_graph", None)

    def _init_search_graph_device(self, search_leaf_size, search_tree_depth):
        """``_init_search_graph`` from the device tensors of an index built from a device array, on torch's current stream
        (``_OnTorchStream``): the in-degrees and the hub rank (csrc/prepare.hip), the hub tree and the pruning pass on handles
        bound to the tensor, the graph re-indexed by the tree's leaf order where the pass left it.  The rows and the graphs
        never visit the host and no host mirror is made; what crosses the bus: the FlatTree tables, ``_vertex_order`` (4 bytes
        per point, down and up again) and scalars.  The rows are gathered when the searcher is filled (``prepare``);
        ``_device_data`` stays the caller's tensor in its original order."""
        from .search_tree import FlatTree

        if self.diversify_method not in ("standard", "degree_aware"):
            raise ValueError("diversify_method must be 'standard' or 'degree_aware'")
        torch, d, m = device_arrays._torch(), self.__dict__, _metric_of(self.metric)
        data, (gidx, gdist) = d["_device_data"], d["_device_graph"]
        n, dim, k = int(data.shape[0]), int(data.shape[1]), int(gidx.shape[1])
        dtype, ordinal = _DEVICE_DTYPES[str(data.dtype).rsplit(".", 1)[-1]], int(self.device)
        seed = int(self.rng_state[0])
        ms = {}  # stream time of every stage (tools/ab/device_prepare_timing.py reads them)

        def bound(builder, stream):  # dot: _device_data is the normalised float32 copy already, borrowed as it is
            builder.set_stream(stream.ptr)
            if m.normalize:
                builder.set_data_device(data.data_ptr(), keepalive=data)
            else:
                builder.set_data_device_typed(data.data_ptr(), dtype, keepalive=data)
            return builder

        with torch.cuda.device(ordinal):
            if "_search_forest" not in d:
                if getattr(self, "_rp_forest", None) is None and not self.tree_init:
                    self._search_forest = []  # pynndescent_.py:1377-1378: no tree, queries start from random vertices
                else:
                    if self.verbose:
                        print(build.ts(), "Building hub-based search tree")
                    stream = _OnTorchStream(torch, ordinal)
                    b = None
                    try:
                        rank = torch.empty((n,), dtype=torch.int32, device=data.device)
                        _, ms["ms_rank"] = _stream_ms(torch, stream, lambda: _capi.rank_order_device(
                            ordinal, stream.ptr, gidx.data_ptr(), n, k, rank.data_ptr()))
                        b = _capi.Builder(n, dim, m.code, 1, 1, max(int(search_leaf_size), 1), search_tree_depth, 1, 1, 0.001,
                                          [seed & 0x7FFFFFFF, 2, 3], [4, 5, 6], device=ordinal,
                                          flags=_capi.NND_FLAG_NO_GRAPH | _capi.NND_FLAG_NO_PREP)
                        tables, ms["ms_hub_tree"] = _stream_ms(torch, stream, lambda: bound(b, stream).hub_tree_device(
                            rank.data_ptr(), search_leaf_size, search_tree_depth))
                        self._search_forest = [FlatTree(*tables)]
                    finally:
                        if b is not None:
                            b.close()
                        stream.done()
                    self._rp_forest = None  # the reference deletes it here (pynndescent_.py:1444)
            order = None
            if self._search_forest:  # the leaf order goes up once; the queries' id mapping reads the same tensor
                tree = self._search_forest[0]
                vertex_order = np.asarray(tree.indices)
                order = torch.from_numpy(np.ascontiguousarray(vertex_order, dtype=np.int32)).to(data.device)
            if self.verbose:
                print(build.ts(), "Diversifying and pruning the search graph")
            stream = _OnTorchStream(torch, ordinal)  # (made after the upload: a side stream waits for it)
            b = None
            try:
                b = bound(_capi.Builder(n, dim, m.code, k, 0, 60, 200, min(60, k), 1, 0.001, [1, 2, 3], [4, 5, 6], device=ordinal,
                                        flags=_capi.NND_FLAG_NO_GRAPH), stream)
                indptr_at, indices_at, nnz, st = b.search_graph_device(
                    gidx.data_ptr(), gdist.data_ptr(), self.n_neighbors, self.prune_degree_multiplier, self.diversify_prob,
                    self.diversify_method == "degree_aware", self.degree_prune_aggressiveness, seed & 0xFFFFFFFF)
                if self.verbose:
                    print(build.ts(), "Resorting data and graph based on tree order")
                indptr = torch.empty((n + 1,), dtype=torch.int32, device=data.device)
                indices = torch.empty((nnz,), dtype=torch.int32, device=data.device)
                _, ms["ms_reorder"] = _stream_ms(torch, stream, lambda: _capi.reorder_csr_device(
                    ordinal, stream.ptr, 0 if order is None else order.data_ptr(), n, indptr_at, indices_at, nnz, indptr.data_ptr(),
                    indices.data_ptr() if nnz else 0))
            finally:
                if b is not None:
                    b.close()
                stream.done()
        self._min_distance = np.float32(float(st["min_distance"]))                  # pynndescent_.py:1539
        self._visited = np.zeros((n // 8) + 1, dtype=np.uint8, order="C")           # pynndescent_.py:1624-1626
        if order is not None:
            self._vertex_order = vertex_order
            self._device_order = order
            new_tree = FlatTree(tree.hyperplanes, tree.offsets, tree.children, np.arange(n, dtype=np.int32), tree.leaf_size)
            self._search_forest = [new_tree] + list(self._search_forest[1: self.n_search_trees])
        else:
            self._vertex_order = np.arange(n)
        if d.get("_is_sparse"):  # the CSR matrix follows the leaf order on the host (pynndescent_.py:1630); _device_data stays as it is
            if order is not None:
                d["_raw_data"] = d["_raw_data"][vertex_order, :]
        else:
            d.pop("_raw_data", None)  # (a mirror fetched before: the rows in their original order; the next read gathers them)
        d.pop("_lin_data", None)
        self._device_search_graph = (indptr, indices)
        self._device_prepare_stats = dict(ms, ms_search_graph=float(st["ms_device"]), final_nnz=int(nnz))
        self._searcher = None
        if self.compressed:  # pynndescent_.py:1653-1658
            d.pop("_rp_forest", None)
            d.pop("_neighbor_graph", None)
            d.pop("_device_graph", None)

    def prepare(self):
        """``NNDescent.prepare`` (pynndescent_.py:2174-2273): build everything a query needs.  quantization="uint8": the
        codebook is drawn on the host from the rows in their original order, the device quantizes the searcher's rows, and
        ``_quantized_data`` is kept on the host in the searcher's (tree) order, as the reference keeps it.  An index that
        already has them (unpickled) reuses ``_quantized_values`` / ``_quantized_data``."""
        _check_quantization(self.quantization, self.metric)
        quantized = self.quantization == "uint8"
        self._is_proxy_distance = quantized or _metric_of(self.metric).proxy
        d = self.__dict__
        fresh = not self._prepared
        if quantized and (fresh or d.get("_quantized_values") is None):
            if "_device_search_graph" in d or (fresh and _prepares_on_device(self)):  # the sample is gathered on the device
                raw = _DeviceRowsView(d["_device_data"])
            else:
                raw = self._raw_data if fresh else self._raw_data[np.argsort(self._vertex_order)]
                if d.get("_is_sparse"):
                    raw = sparse_input.CsrRowsView(raw)
            self._quantized_values = uint8_codebook(raw, self.random_state)
            self._quantized_data = None  # derived by the device below, in the searcher's order
        if fresh:
            self._init_search_graph()
        on_device = "_device_search_graph" in d and "_device_data" in d
        if d.get("_searcher") is None:
            tree = self._search_forest[0] if self._search_forest else None
            if on_device:
                self._searcher = self._searcher_from_device(tree)
            else:
                self._searcher = _capi.Searcher(self._work_rows(), self._search_graph, tree, _metric_of(self.metric).code,
                                                self._min_distance, self.n_neighbors, self.search_rng_state, device=self.device)
        if quantized and not self._searcher.has_codes:
            if d.get("_quantized_data") is None:
                # dot: the searcher's own copy is normalised once more on the device; the codes are those of _raw_data
                rows = self._raw_data if _metric_of(self.metric).normalize else None
                if on_device and rows is None:  # the codes stay with the searcher; _quantized_data is their mirror, fetched when read
                    self._searcher.quantize_u8(self._quantized_values, rows=None, fetch=False)
                    d.pop("_quantized_data", None)
                else:
                    self._quantized_data = self._searcher.quantize_u8(self._quantized_values, rows=rows)
            else:
                self._searcher.set_codes_u8(self._quantized_values, self._quantized_data)

    def _searcher_from_device(self, tree):
        """The searcher of a device-prepared index, filled on torch's current stream from the caller's tensor (its rows gathered by
        the leaf order straight into the searcher's layout), the reordered device graph and the host tree tables."""
        torch, d = device_arrays._torch(), self.__dict__
        data, (indptr, indices), order = d["_device_data"], d["_device_search_graph"], d.get("_device_order")
        ordinal = int(self.device)
        with torch.cuda.device(ordinal):
            stream = _OnTorchStream(torch, ordinal)
            try:
                searcher, ms = _stream_ms(torch, stream, lambda: _capi.Searcher.from_device(
                    data.data_ptr(), _DEVICE_DTYPES[str(data.dtype).rsplit(".", 1)[-1]], data.shape[0], data.shape[1],
                    0 if order is None else order.data_ptr(), indptr.data_ptr(), indices.data_ptr() if indices.numel() else 0,
                    indices.numel(), tree, _metric_of(self.metric).code, self._min_distance, self.n_neighbors, self.search_rng_state,
                    device=ordinal, stream_ptr=stream.ptr))
                d.setdefault("_device_prepare_stats", {})["ms_searcher_fill"] = ms
            finally:
                stream.done()
        if order is not None:
            searcher.vertex_order_device = order  # what _query_device maps the answers' ids through
        return searcher

    def set_row_tags(self, tags):
        """The rows' tag words for per-query filters (``query(..., query_tags=...)``; beyond the reference): 1-D, one entry per row
        in the ORIGINAL numbering, 64 tag bits each -- a numpy ``uint64`` or ``int64`` array (the bit pattern counts: bit 63 is a
        tag like any other) or an ``int64`` tensor on the index's device; anything else raises ``ValueError``.  ``None`` removes
        the tags.  The index keeps what it is given: a tensor stays where it is, a host array goes to the device once, when a
        query first needs it, not once per call; a pickle carries a host copy.  ``update()`` clears the tags."""
        d = self.__dict__
        if tags is None:
            d.pop("_row_tags", None)
        else:
            d["_row_tags"] = tagwords.check_words(tags, int(self._raw_data_n()), self.device, "tags", "row")[0]
        d.pop("_row_tags_cleared", None)
        searcher = d.get("_searcher")
        if searcher is not None and getattr(searcher, "tags_set", False):  # the searcher's copy is of the old tags
            searcher.clear_tags()
            searcher.tags_set = False

    def query(self, query_data, k=10, epsilon=0.1, proxy_beam_size=4, filter=None, filter_mode="auto", query_tags=None):
        """``NNDescent.query`` (pynndescent_.py:2275-2379) on the GPU: one wave per query (csrc/query.hip).
        Returns (indices (n_queries, k) in the ORIGINAL numbering, true distances (n_queries, k)).  A device array
        ``query_data`` (float32 / float16 / bfloat16 / float64, on the index's device) is answered with device tensors: the
        queries are converted, the ids mapped back and the distances corrected on the device, on torch's current stream;
        the index may have been built from host or device data alike, and a host ``query_data`` returns numpy on both.

        ``filter`` (beyond the reference; filtered.py): the rows that may be returned, one set for all queries of the call, in
        the ORIGINAL numbering -- a 1-D boolean mask of n rows (True: allowed) or a 1-D integer array of row ids, numpy or a
        tensor on the index's device, whichever side the queries are on.  Places that no allowed row fills hold (-1, inf).
        ``filter_mode``: "walk" -- the graph walk in which a vertex enters the result list only if it is allowed (it is still
        traversed, so bound and stop rule are those of the walk relative to the allowed rows); "exact" -- brute force over a
        compact copy of the allowed rows, by (float64 distance, id) as ``exact_knn`` (not for proxy_inner_product); "auto" --
        "exact" for at most ``filtered.FILTER_EXACT_MAX_ROWS`` allowed rows when the metric has an exact search, else "walk".
        After a filtered call ``self.last_filter`` says what ran: ``{"mode": "walk" | "exact" | "empty", "n_allowed": rows}``
        ("empty": no row allowed, answered without a launch).  Soft deletion: keep a mask of the live rows and pass it.

        ``query_tags`` (per-query filters; needs ``set_row_tags``, does not combine with ``filter``): a mask word per query, 1-D,
        the dtypes of ``set_row_tags``, on the host or on the index's device whichever side the queries are on.  Row r may be
        returned to query i iff ``tags[r] & query_tags[i] != 0``; a query with mask 0 gets (-1, inf) in every place.
        ``filter_mode``: "walk" -- the walk with that rule per query; "exact" -- the masked brute-force scan over all rows (not for
        proxy_inner_product); "auto" -- per query: the device counts the rows each distinct mask of the call allows, a query whose
        mask allows at most ``filtered.TAG_EXACT_MAX_ROWS`` rows goes to the exact path, one whose mask allows none is answered
        without a search, the others walk; with more than ``filtered.TAG_COUNT_MAX_MASKS`` distinct masks nothing is counted and
        every query walks.  ``self.last_filter`` is then ``{"mode": "tags", "n_walk", "n_exact", "n_empty", "n_masks"}``."""
        if k > 256:
            raise NotImplementedError("pynndescent_amd answers queries with k <= 256; use index.to_reference() for k = %d" % k)
        _check_quantization(self.quantization, self.metric)
        m = _metric_of(self.metric)
        if filter_mode not in filtered.FILTER_MODES:
            raise ValueError("filter_mode must be one of %s (got %r)" % (", ".join(filtered.FILTER_MODES), filter_mode))
        if query_tags is not None:
            return self._query_tagged(query_data, m, k, epsilon, proxy_beam_size, filter, filter_mode, query_tags)
        if sparse_input.is_sparse(query_data):
            return self._query_sparse(query_data, m, k, epsilon, proxy_beam_size, filter, filter_mode)
        if filter is not None:
            return self._query_filtered(query_data, m, k, epsilon, proxy_beam_size, filter, filter_mode)
        return self._query_walk(query_data, m, k, epsilon, proxy_beam_size)

    def kneighbors_graph(self, X=None, k=None, mode="distance", symmetric=False, include_self=True, epsilon=0.1, **query_kwds):
        """The index's answers as a sparse neighbour matrix in canonical CSR form (graph_export.py, csrc/csr_graph.hip): columns
        ascending in every row, float32 data, int32 column ids, assembled on the GPU.

        ``X`` None: the built graph, (n, n), with the distances ``neighbor_graph`` hands out; ``k`` (default ``n_neighbors``)
        takes the first k columns.  ``X`` given: the answers of ``query(X, k, epsilon, **query_kwds)`` as an (n_queries, n)
        matrix -- ``filter``, ``filter_mode``, ``query_tags`` and ``proxy_beam_size`` pass through, and the (-1, inf) places a
        filter leaves are dropped, so such a row holds fewer than k entries.
        ``mode``: "distance" stores the distances, "connectivity" 1.0.  ``symmetric`` (built graph only): the union of the matrix
        and its transpose; where the two sides of a pair differ in the last bits the entry holds the smaller value.
        ``include_self=False`` (built graph only) drops every entry (i, i), wherever in the row it stands.
        Returns ``scipy.sparse.csr_array`` for an index of host (or scipy.sparse) data or one built with ``n_devices`` > 1, and a
        ``torch.sparse_csr_tensor`` on the index's device, on torch's current stream, for a device-resident index; that tensor
        is built on the kernels' own buffers, nothing is copied."""
        return graph_export.kneighbors_graph(self, X, k, mode, symmetric, include_self, epsilon, **query_kwds)

    def _query_sparse(self, query_data, m, k, epsilon, proxy_beam_size, filter, filter_mode):
        """``query`` for a ``scipy.sparse`` batch, on an index built from sparse or dense data alike: the batch is made canonical,
        uploaded as CSR and made dense on the device (sparse_input.py), and answered by the device-array forms of every query
        path.  Scipy in, numpy out: the ids and the kernels' distances come down and the host applies the metric's correction,
        so the answers are those of ``query(query_data.toarray())``, bit for bit."""
        if tuple(_shape_of(query_data))[1:] != (self.dim,):
            raise ValueError("query_data must have shape (n_queries, %d)" % self.dim)
        if filter is not None:  # (validated on the host, before the upload; a host filter goes where the queries will be)
            f = filtered.check_filter(filter, int(self._raw_data_n()), self.device)
            if f.n_allowed == 0:
                self.last_filter = {"mode": "empty", "n_allowed": 0}
                return filtered.empty_answer(query_data, k)
        q = sparse_input.query_rows(query_data, self.dim, self.device)
        if filter is not None:
            if not f.on_device:
                filter = device_arrays._torch().from_numpy(f.values).to(q.device)
            indices, dists = self._query_filtered(q, m, k, epsilon, proxy_beam_size, filter, filter_mode, host_answers=True)
            if not _is_device_array(indices):  # (the exact path has brought them down and corrected them)
                return indices, dists
        else:
            indices, dists = self._query_walk(q, m, k, epsilon, proxy_beam_size, host_answers=True)
        indices, dists = np.ascontiguousarray(indices.cpu().numpy()), np.ascontiguousarray(dists.cpu().numpy())
        if self._distance_correction is not None:  # pynndescent_.py:2375-2376
            dists = self._distance_correction(dists)
        return indices, dists

    def _query_filtered(self, query_data, m, k, epsilon, proxy_beam_size, filter, filter_mode, host_answers=False):
        """``query`` with a filter: everything is validated before any device work, then the path ``filtered.choose_mode`` names.
        ``host_answers`` (device queries made from a sparse batch): see ``_query_device``."""
        if self.quantization is not None or m.proxy:
            _proxy_search_k(k, proxy_beam_size)
        f = filtered.check_filter(filter, int(self._raw_data_n()), self.device)
        if tuple(_shape_of(query_data))[1:] != (self.dim,):
            raise ValueError("query_data must have shape (n_queries, %d)" % self.dim)
        mode = filtered.choose_mode(filter_mode, f.n_allowed, self.metric)
        self.last_filter = {"mode": mode, "n_allowed": f.n_allowed}
        if mode == "exact":
            _no_exact_for_proxy(self.metric, m, 'NNDescent.query(filter_mode="exact")')
        if mode == "empty":
            return filtered.empty_answer(query_data, k)
        if not self._prepared:
            self.prepare()
        if mode == "exact":
            if host_answers:
                return filtered.query_exact(self, query_data, k, f, host_answers=True)
            return filtered.query_exact(self, query_data, k, f)
        if getattr(self, "_searcher", None) is None or (self.quantization is not None and not self._searcher.has_codes):
            self.prepare()
        filtered.set_walk_filter(self, f)
        try:
            return self._query_walk(query_data, m, k, epsilon, proxy_beam_size, host_answers=host_answers)
        finally:
            self._searcher.clear_filter()

    def _query_tagged(self, query_data, m, k, epsilon, proxy_beam_size, filter, filter_mode, query_tags):
        """``query`` with ``query_tags``: everything is validated before any device work; then the walk on the whole batch (a
        query's seed depends on its place in the batch, so the queries another path answers stay in it with mask 0, which ends
        their wave at once), the masked exact scan on the queries ``auto`` or "exact" gives it, and the two scattered into one
        answer where ``query_data`` lives."""
        d = self.__dict__
        if filter is not None:
            raise ValueError("query takes filter or query_tags, not both: an allow set and per-query masks do not combine")
        if "_row_tags" not in d:
            if d.get("_row_tags_cleared"):
                raise ValueError("update() cleared the row tags, the row set has changed: set the row tags again (set_row_tags)")
            raise ValueError("query_tags needs the rows' tags: call set_row_tags first")
        if getattr(self, "n_devices", 1) > 1:
            raise NotImplementedError("query_tags is not available on an index built with n_devices > 1")
        if self.quantization is not None or m.proxy:
            _proxy_search_k(k, proxy_beam_size)
        if tuple(_shape_of(query_data))[1:] != (self.dim,):
            raise ValueError("query_data must have shape (n_queries, %d)" % self.dim)
        nq = int(_shape_of(query_data)[0])
        masks, masks_on_device = tagwords.check_words(query_tags, nq, self.device, "query_tags", "query")
        if filter_mode == "exact":
            _no_exact_for_proxy(self.metric, m, 'NNDescent.query(filter_mode="exact")')
        sparse = sparse_input.is_sparse(query_data)
        if sparse:  # uploaded as CSR and made dense on the device; the answers come down again (``_query_sparse``)
            query_data = sparse_input.query_rows(query_data, self.dim, self.device)
        on_device = _is_device_array(query_data)
        if (not self._prepared or getattr(self, "_searcher", None) is None
                or (self.quantization is not None and not self._searcher.has_codes)):
            self.prepare()
        # the path of every query, on the host: the masks of a call are 8 bytes per query
        host_masks = tagwords.to_host(masks, masks_on_device)
        distinct, inverse = np.unique(host_masks, return_inverse=True)
        if filter_mode == "auto":
            counts = filtered.tag_counts(self, distinct) if filtered.tag_counts_taken(len(distinct)) and len(distinct) else None
            walk, exact, empty = filtered.tag_auto_paths(inverse, distinct, counts, exact_ok=not m.proxy)
        else:
            empty = np.flatnonzero(host_masks == 0)
            rest = np.flatnonzero(host_masks != 0)
            walk, exact = (rest, rest[:0]) if filter_mode == "walk" else (rest[:0], rest)
        self.last_filter = {"mode": "tags", "n_walk": len(walk), "n_exact": len(exact), "n_empty": len(empty), "n_masks": len(distinct)}
        indices, dists = filtered.empty_answer(query_data, k)
        if len(walk):
            walk_masks = host_masks
            if len(walk) != nq:
                walk_masks = np.zeros(nq, np.uint64)
                walk_masks[walk] = host_masks[walk]
            elif masks_on_device and on_device:
                walk_masks = masks  # (the caller's tensor as it is)
            indices, dists = self._query_walk(query_data, m, k, epsilon, proxy_beam_size, host_answers=sparse, query_masks=walk_masks)
            if sparse:
                indices, dists = np.ascontiguousarray(indices.cpu().numpy()), np.ascontiguousarray(dists.cpu().numpy())
                if self._distance_correction is not None:
                    dists = self._distance_correction(dists)
        if len(exact):
            whole = len(exact) == nq
            if on_device:
                torch = device_arrays._torch()
                where = torch.from_numpy(exact).to(query_data.device)
                sub_q = query_data if whole else query_data[where]
            else:
                sub_q = query_data if whole else np.asarray(query_data)[exact]
            sub_i, sub_d = filtered.query_tagged_exact(self, sub_q, k, host_masks[exact], False, host_answers=sparse)
            if _is_device_array(indices) and not _is_device_array(sub_i):  # (a sparse batch whose queries all went exact)
                indices, dists = indices.cpu().numpy(), dists.cpu().numpy()
            if _is_device_array(indices):
                indices[where] = sub_i.to(indices.dtype)
                dists = dists.to(sub_d.dtype) if dists.dtype != sub_d.dtype else dists
                dists[where] = sub_d
            else:
                dists = dists.astype(sub_d.dtype, copy=False)
                indices[exact], dists[exact] = sub_i, sub_d
        if sparse and _is_device_array(indices):  # (nothing ran: the empty answer was made where the dense queries are)
            indices, dists = indices.cpu().numpy(), dists.cpu().numpy()
        # the places no allowed row fills hold (-1, inf), whatever the metric's correction makes of inf
        if _is_device_array(dists):
            dists = dists.masked_fill(indices < 0, float("inf"))
        else:
            dists = np.array(dists, copy=True)
            dists[indices < 0] = np.inf
        return indices, dists

    def _raw_data_n(self):
        """The number of rows, without fetching a host mirror."""
        d = self.__dict__
        return d["_device_data"].shape[0] if "_device_data" in d else self._raw_data.shape[0]

    def _query_walk(self, query_data, m, k, epsilon, proxy_beam_size, host_answers=False, query_masks=None):
        """The graph walk of ``query`` (with the searcher's filter, when ``_query_filtered`` has set one; ``query_masks``: the
        tagged walk, a mask word per query -- numpy uint64, or an int64 tensor beside device queries)."""
        search_k = k
        if self.quantization is not None or m.proxy:  # pynndescent_.py:2309-2312
            search_k = _proxy_search_k(k, proxy_beam_size)
        if (not self._prepared or getattr(self, "_searcher", None) is None
                or (self.quantization is not None and not self._searcher.has_codes)):
            self.prepare()
        if query_masks is not None:
            filtered.ensure_searcher_tags(self)
        if _is_device_array(query_data):
            return self._query_device(query_data, m, k, search_k, epsilon, corrected=not host_answers, query_masks=query_masks)
        query_data = np.asarray(query_data).astype(np.float32, order="C")  # pynndescent_.py:2316
        if query_data.ndim != 2 or query_data.shape[1] != self.dim:
            raise ValueError("query_data must have shape (n_queries, %d)" % self.dim)
        _raise_if_negative_host(query_data, m)
        lin = self.__dict__.get("_linear_map")
        if lin is not None:  # the queries through the index's own (A, c), by the kernel that transformed its rows
            query_data = row_map.rows_host(lin, query_data, device=self.device)
        if query_masks is not None:  # the same three forms, eps as below
            form = "proxy" if self.quantization is not None else ("rerank" if m.proxy else "float")
            indices, dists = self._searcher.query_tagged(form, query_data, query_masks, k, search_k, epsilon + (1e-32 if form == "proxy" else 0.0))
        elif self.quantization is not None:  # the walk on the codes, the rerank in its epilogue (pynndescent_.py:2321-2322, 2363-2371)
            indices, dists = self._searcher.query_proxy(query_data, k, search_k, epsilon + 1e-32)
        elif m.proxy:  # the walk on the proxy distance, the rerank by the true one; epsilon as given (pynndescent_.py:2321-2322)
            indices, dists = self._searcher.query_rerank(query_data, k, search_k, epsilon)
        else:
            indices, dists = self._searcher.query(query_data, k, epsilon)
        found = indices >= 0
        indices = np.where(found, self._vertex_order[np.where(found, indices, 0)], -1).astype(np.int32)  # pynndescent_.py:2373
        if self._distance_correction is not None:  # pynndescent_.py:2375-2376
            dists = self._distance_correction(dists)
        return indices, dists

    def _query_device(self, q, m, k, search_k, epsilon, corrected=True, query_masks=None):
        """``query`` for a device array: the three forms on the device-pointer entries of the searcher.  ``corrected`` False: the
        kernels' own distances are returned -- the caller brings them to the host and applies the host's correction there, for
        answers that equal a host query's bit for bit (the device's 1 - 2^-d agrees with numpy's within rounding only)."""
        torch = device_arrays._torch()
        q, dtype, ordinal = _check_device_array(q, what="query_data")
        if ordinal != int(self.device):
            raise ValueError("query_data is on device %d, the index on device %d" % (ordinal, int(self.device)))
        nq, dim = int(q.shape[0]), int(self.dim)
        if q.shape[1] != dim:
            raise ValueError("query_data must have shape (n_queries, %d)" % dim)
        with torch.cuda.device(ordinal):
            stream = torch.cuda.current_stream(ordinal).cuda_stream
            if self.__dict__.get("_linear_map") is not None:  # converted, then through the index's own (A, c)
                q = self._linear_on_device(q.device).rows(q, dtype, stream)
            elif dtype != _capi.NND_DTYPE_FLOAT32:  # pynndescent_.py:2316
                q32 = torch.empty((nq, dim), dtype=torch.float32, device=q.device)
                _capi.device_rows_f32(ordinal, stream, q.data_ptr(), dtype, nq, dim, False, q32.data_ptr())
                q = q32
            if m.nonnegative and nq and bool((q.min() < 0).item()):
                raise ValueError(_NEGATIVE_HELLINGER)
            indices = torch.empty((nq, k), dtype=torch.int32, device=q.device)
            dists = torch.empty((nq, k), dtype=torch.float32, device=q.device)
            if self.quantization is not None:
                form, eps = "proxy", epsilon + 1e-32
            elif m.proxy:
                form, eps = "rerank", epsilon
            else:
                form, eps = "float", epsilon
            if nq and query_masks is not None:
                masks = tagwords.to_device(query_masks, _is_device_array(query_masks), q.device)
                self._searcher.query_tagged_device(form, q.data_ptr(), masks.data_ptr(), nq, k, search_k, eps, indices.data_ptr(),
                                                   dists.data_ptr(), stream)
            elif nq:
                self._searcher.query_device(form, q.data_ptr(), nq, k, search_k, eps, indices.data_ptr(), dists.data_ptr(), stream)
            order = getattr(self._searcher, "vertex_order_device", None)  # lives and dies with the searcher
            if order is None:
                order = torch.from_numpy(np.ascontiguousarray(self._vertex_order, dtype=np.int32)).to(q.device)
                self._searcher.vertex_order_device = order
            found = indices >= 0
            indices = torch.where(found, order[indices.clamp(min=0).long()], torch.full_like(indices, -1))  # pynndescent_.py:2373
            if corrected and self._distance_correction is not None and m.device_kind != _capi.NND_CORRECT_COPY:  # pynndescent_.py:2375-2376
                dists = _device_corrected(torch, dists, m, ordinal)
        return indices, dists

    # ------------------------------------------------------------------------------------------------ pickling
    def __getstate__(self):
        """pynndescent_.py:1306-1320: a pickled index is a PREPARED index; device handles and the build forest stay behind."""
        if not self._prepared:
            self._init_search_graph()
        if "_device_data" in self.__dict__ or "_device_graph" in self.__dict__:  # the host mirrors travel, the tensors stay
            self._raw_data
            for name in ("_neighbor_graph", "_search_graph", "_quantized_data"):
                hasattr(self, name)
        state = self.__dict__.copy()
        if _is_device_array(state.get("_row_tags")):  # the tag words travel as a host copy
            state["_row_tags"] = tagwords.to_host(state["_row_tags"], True)
        # a linear map travels as _linear_map (kind, A, c: float32); the transformed rows are derived again from _raw_data
        for name in self._DEVICE_TENSORS + self._LINEAR_COPIES + ("_rp_forest", "_searcher"):
            state.pop(name, None)
        state["_search_forest"] = tuple(tuple(t) for t in self._search_forest)  # rp_trees.py:3060-3069 denumbaify_tree
        return state

    def __setstate__(self, d):
        """pynndescent_.py:1322-1331: rebuild what cannot be pickled (here: the device copy, lazily on the first query)."""
        from .search_tree import FlatTree

        self.__dict__ = d
        self._distance_correction = _metric_of(self.metric).correction
        self._search_forest = [FlatTree(*t) for t in d["_search_forest"]]  # rp_trees.py:3072-3081 renumbaify_tree
        self._searcher = None

    def update(self, xs_fresh=None, xs_updated=None, updated_indices=None):
        """``pynndescent.NNDescent.update`` (pynndescent_.py:2381-2553) on the GPU: fresh rows are appended, updated
        rows replaced (their graph rows and every edge pointing at them are dropped), then the graph is rebuilt from
        a warm start -- the old graph inserted as "old" edges (init_from_neighbor_graph, flag 0), a forest of
        ``n_trees_after_update`` trees seeding "new" edges, no random fill -- and NN-descent runs to the stop rule.

        An index built from a device array on one GPU stays there when ``xs_fresh`` or ``xs_updated`` is a device array (a host
        array given alongside is uploaded): the new rows and the invalidated graph are assembled on the device
        (``_update_device``), ``neighbor_graph`` keeps returning tensors and a prepared index is prepared again on the device.
        With host arrays alone such an index becomes a host index, as before; a device array given to a host index, or to one
        built on several GPUs, is brought to the host.  ``updated_indices`` may be a tensor; the ids are read on the host."""
        sparse_index = bool(self.__dict__.get("_is_sparse"))
        if sparse_index:  # (an unpickled one: its rows and its graph go up again first)
            self._sparse_to_device()
        on_device = _updates_on_device(self, xs_fresh, xs_updated)
        if not on_device:  # a tensor or a sparse matrix on an index that cannot stay on the device: its values, through the host path
            xs_fresh, xs_updated = (sparse_input.canonical_csr(a).toarray() if sparse_input.is_sparse(a) else _rows_to_host(a)
                                    for a in (xs_fresh, xs_updated))
        updated_indices = _ids_to_host(updated_indices)  # (a tensor of ids: they are few, and they stay a host list)
        csr_rows = {}  # a sparse index: the incoming rows as CSR as well, for its _raw_data

        def checked(rows, what):  # check_array; a device array of the device path: its validator, nothing is read
            if sparse_input.is_sparse(rows):  # (the device path: made canonical, checked, then dense on the device)
                rows = sparse_input.canonical_csr(rows)
                if rows.shape[1] != self.dim:
                    raise ValueError("%s must have shape (n_rows, %d), got %s" % (what, self.dim, tuple(rows.shape)))
                csr_rows[what] = rows
                return sparse_input.dense_rows_on_device(rows, self.device)
            if not _is_device_array(rows):
                rows = check_array(rows, dtype=self._input_dtype, order="C")
                if sparse_index:
                    csr_rows[what] = sparse_input.as_csr(rows)
                return rows
            rows, _, ordinal = _check_device_array(rows, what=what)
            if ordinal != int(self.device):
                raise ValueError("%s is on device %d, the index on device %d" % (what, ordinal, int(self.device)))
            if rows.shape[1] != self.dim:
                raise ValueError("%s must have shape (n_rows, %d), got %s" % (what, self.dim, tuple(rows.shape)))
            return rows

        current_random_state = check_random_state(self.random_state)
        # drawn and handed to make_forest by the reference (pynndescent_.py:2408-2411); kept for the stream position
        current_random_state.randint(INT32_MIN, INT32_MAX, 3)
        if xs_updated is not None:
            xs_updated = checked(xs_updated, "xs_updated")
            if updated_indices is None:
                raise ValueError("If xs_updated are provided, updated_indices must also be provided!")
            try:
                updated_indices = list(map(int, updated_indices))
            except (TypeError, ValueError):
                raise ValueError("Could not convert updated indices to list of int(s).")
            n1, n2 = len(updated_indices), xs_updated.shape[0]
            if n1 != n2:
                raise ValueError(
                    f"Number of updated indices ({n1}) must match " f"number of rows of xs_updated ({n2})."
                )
        else:
            if updated_indices is not None:
                warn("xs_updated not provided, while update_indices provided. " "They will be ignored.")
            updated_indices = None
        if self.__dict__.pop("_row_tags", None) is not None:  # the row set changes: the tags are the caller's to set again
            self._row_tags_cleared = True
        if on_device:
            return self._update_device(None if xs_fresh is None else checked(xs_fresh, "xs_fresh"), xs_updated, updated_indices or [],
                                       current_random_state, csr_rows=csr_rows)
        if updated_indices is None:
            xs_updated = np.zeros((0, self._raw_data.shape[1]), self._input_dtype)
            updated_indices = []
        if xs_fresh is None:
            xs_fresh = np.zeros((0, self._raw_data.shape[1]), dtype=self._input_dtype)
        else:
            xs_fresh = check_array(xs_fresh, dtype=self._input_dtype, order="C")

        # data and graph invalidation (pynndescent_.py:2461-2493), vectorised; a prepared index keeps its rows in the
        # search tree's leaf order: back to the original order first (pynndescent_.py:2462-2465, 2476)
        raw = np.array(self._raw_data, copy=True)
        if hasattr(self, "_vertex_order"):
            raw = raw[np.argsort(self._vertex_order), :]
        for x_updated, i_fresh in zip(xs_updated, updated_indices):
            raw[i_fresh] = x_updated
        n_old = raw.shape[0]
        raw = np.ascontiguousarray(np.vstack([raw, xs_fresh]))
        ns, ds = (np.array(a, copy=True) for a in self._neighbor_graph)
        self._drop_device_copies()  # (an index built from a device array: from here on its host arrays are the index)
        if updated_indices:
            hit = np.zeros(n_old, bool)
            hit[updated_indices] = True
            ns[hit] = -1
            ds[hit] = np.inf
            stale = (ns >= 0) & hit[np.clip(ns, 0, None)]
            ns[stale] = -1
            ds[stale] = np.inf
        n = raw.shape[0]
        pad_i = np.full((n, ns.shape[1]), -1, np.int32)
        pad_d = np.full((n, ns.shape[1]), np.inf, np.float32)
        pad_i[:n_old] = ns
        pad_d[:n_old] = ds

        self.n_trees = self.n_trees_after_update  # pynndescent_.py:2498
        _, _, eff_leaf_size, eff_max_candidates = _reference_defaults(n, self.n_neighbors, self.n_trees, self.n_iters,
                                                                      self.leaf_size, self.max_candidates)
        tree_states = current_random_state.randint(INT32_MIN, INT32_MAX, size=(self.n_trees, 3)).astype(np.int64)
        if getattr(self, "n_devices", 1) > 1:  # the rebuild is sharded like the build was (nnd_build_multi_update)
            n_leaves = self._build_multi(raw, self.n_trees, eff_leaf_size, eff_max_candidates, tree_states[0], False,
                                         old_graph=(pad_i, pad_d))
        else:  # pynndescent_.py:2512-2517: the old graph's entries as "old" edges, then the forest's; no random fill
            lin, work = self.__dict__.get("_linear_map"), raw
            self.__dict__.pop("_lin_data", None)
            if _metric_of(self.metric).row_map is not None:
                device_arrays._assert_all_finite(raw)
            if lin is not None:  # old, updated and fresh rows through the index's own (A, c): old rows come out as they were
                work = self._lin_data = row_map.rows_host(lin, raw, device=self.device)
            self._neighbor_graph, self._build_stats, n_leaves = _build_graph(
                work, _metric_of(self.metric), self.n_neighbors, self.n_trees, eff_leaf_size, self.max_rptree_depth,
                eff_max_candidates, self.n_iters, self.delta, self.rng_state, tree_states[0], self.device, forest=True,
                old_graph=(pad_i, pad_d), verbose=self.verbose)
        self._rp_forest = _DeviceForestSentinel(self.n_trees, n_leaves, eff_leaf_size)
        self._raw_data = raw
        if self._prepared:  # pynndescent_.py:2538-2553: the derived structures are rebuilt
            # (``_quantized_data`` stays where ``_update_device`` pops it: the fresh prepare() below resets it with the codebook)
            for name in self._SEARCH_STRUCTURES:
                self.__dict__.pop(name, None)
            self.prepare()


    def _sparse_to_device(self):
        """A sparse index that has lost its device tensors (unpickled) gets them again: the CSR rows, back in their original order,
        are made dense on the device -- a row's dense form depends on the row alone, so the bits are those of the build -- and the
        graph's host mirror goes up.  ``update()`` and ``recall()`` then run where they run for a freshly built index."""
        d = self.__dict__
        if "_device_data" not in d:
            raw = d["_raw_data"]
            if "_vertex_order" in d:
                raw = raw[np.argsort(d["_vertex_order"]), :]
            d["_device_data"] = sparse_input.dense_rows_on_device(raw, self.device)
        if "_device_graph" not in d and "_neighbor_graph" in d:
            torch = device_arrays._torch()
            d["_device_graph"] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(d["_device_data"].device) for a in d["_neighbor_graph"])

    def _update_device(self, xs_fresh, xs_updated, updated_indices, current_random_state, csr_rows=None):
        """``update`` of an index that holds its rows and its graph on the device, entry for entry what the host path computes
        from the mirrors -- on torch's current stream (``_OnTorchStream``), with no host leg: the new ``(n_old + n_fresh, d)``
        tensor (old rows, fresh rows, updated rows scattered to their ids; the dtype all arrays share, else float32) and the
        invalidated, padded graph are written by the library (``nnd_device_update_rows`` / ``nnd_device_update_graph``), the
        rebuild binds the new rows as they are (dot: not normalised again, as on the host path) and reads the old graph in place.
        What crosses the bus: the resolved ``(row id, source row)`` pairs, host arrays given alongside, and the build's scalars."""
        d, m = self.__dict__, _metric_of(self.metric)
        # (a metric with a linear map: the new tensor is assembled from the caller's rows, and transformed as a whole below)
        data, (gidx, gdist) = d.get("_device_raw", d["_device_data"]), d["_device_graph"]
        linear = self._linear_on_device(data.device) if d.get("_linear_map") is not None else None
        n_old, dim, k, ordinal = int(data.shape[0]), int(data.shape[1]), int(gidx.shape[1]), int(self.device)
        ids, sources = _resolve_updated_indices(updated_indices, n_old)  # (IndexError: before any device work)
        torch = device_arrays._torch()
        n_fresh = 0 if xs_fresh is None else int(xs_fresh.shape[0])
        n = n_old + n_fresh
        n_trees = self.n_trees_after_update  # pynndescent_.py:2498 (assigned with the new tensors: a rebuild that raises changes nothing)
        _, _, eff_leaf_size, eff_max_candidates = _reference_defaults(n, self.n_neighbors, n_trees, self.n_iters,
                                                                      self.leaf_size, self.max_candidates)
        tree_states = current_random_state.randint(INT32_MIN, INT32_MAX, size=(n_trees, 3)).astype(np.int64)
        with torch.cuda.device(ordinal):
            def on_device(rows):  # a host array given alongside goes up (float32: what check_array made of it)
                return rows if rows is None or _is_device_array(rows) else torch.from_numpy(rows).to(data.device)

            def described(rows):  # (address, NND_DTYPE_*, rows) of an array that may be absent
                return (0, 0, 0) if rows is None or rows.shape[0] == 0 else (rows.data_ptr(), _DEVICE_DTYPES[_dtype_name(rows)], rows.shape[0])

            xs_fresh, xs_updated = on_device(xs_fresh), on_device(xs_updated)
            out_name = _update_dtype([_dtype_name(data)] + [_dtype_name(a) for a in (xs_fresh, xs_updated) if a is not None])
            new_data = torch.empty((n, dim), dtype=getattr(torch, out_name), device=data.device)
            pad_i = torch.empty((n, k), dtype=torch.int32, device=data.device)
            pad_d = torch.empty((n, k), dtype=torch.float32, device=data.device)
            updated_map = torch.empty((n_old,), dtype=torch.uint8, device=data.device)
            pairs = torch.from_numpy(np.stack([ids, sources])).to(data.device) if ids.shape[0] else None
            stream = _OnTorchStream(torch, ordinal)  # (made after the uploads: a side stream waits for them)
            try:
                ids_ptr, sources_ptr = (pairs[0].data_ptr(), pairs[1].data_ptr()) if pairs is not None else (0, 0)
                _capi.device_update_rows(ordinal, stream.ptr, dim, described(data), described(xs_fresh), described(xs_updated),
                                         (sources_ptr, ids_ptr, ids.shape[0]), new_data.data_ptr(), _DEVICE_DTYPES[out_name])
                _capi.device_update_graph(ordinal, stream.ptr, gidx.data_ptr(), gdist.data_ptr(), n_old, k, ids_ptr, ids.shape[0], n,
                                          updated_map.data_ptr(), pad_i.data_ptr(), pad_d.data_ptr())
            finally:
                stream.done()
            if m.row_map is not None:
                device_arrays._assert_all_finite(new_data)
            # pynndescent_.py:2512-2517: the old graph's entries as "old" edges, then the forest's; no random fill
            dev_in = _DeviceInput(new_data, _DEVICE_DTYPES[out_name], ordinal, self.n_neighbors, as_given=True, linear=linear)
            graph, build_stats, n_leaves = _build_graph(
                new_data, m, self.n_neighbors, n_trees, eff_leaf_size, self.max_rptree_depth, eff_max_candidates, self.n_iters,
                self.delta, self.rng_state, tree_states[0], ordinal, forest=True, old_graph=(pad_i, pad_d), check_finite=True,
                verbose=self.verbose, dev_in=dev_in)
        self.n_trees, self._build_stats = n_trees, build_stats
        self._rp_forest = _DeviceForestSentinel(n_trees, n_leaves, eff_leaf_size)
        was_prepared = self._prepared
        new_csr = None
        if d.get("_is_sparse"):  # _raw_data is updated as CSR, in the original order (pynndescent_.py:2461-2476)
            raw = d["_raw_data"][np.argsort(d["_vertex_order"]), :] if "_vertex_order" in d else d["_raw_data"]
            new_csr = sparse_input.updated_csr(raw, (csr_rows or {}).get("xs_updated"), ids, sources, (csr_rows or {}).get("xs_fresh"))
        # (the rows and the graph are replaced below; every mirror of the old ones is stale, ``_device_linear`` is the same map)
        for name in self._DEVICE_PREPARED + self._HOST_MIRRORS + self._SEARCH_STRUCTURES:
            d.pop(name, None)
        self._device_data, self._device_graph = dev_in.rows, graph  # (the caller's original tensor is released)
        if new_csr is not None:
            d["_raw_data"] = new_csr
        if linear is not None:
            self._device_raw = new_data
        if was_prepared:  # pynndescent_.py:2538-2553: the derived structures are rebuilt, from the tensors when _prepares_on_device
            self.prepare()


# from_graph's keywords and their defaults: the constructor's, minus what the graph fixes (the data, n_neighbors, the metric
# and random_state are arguments of their own; the build's seeding and its devices do not apply)
_FROM_GRAPH_DEFAULTS = {
    ("prune_degree_multiplier" if name == "pruning_degree_multiplier" else name): p.default
    for name, p in inspect.signature(NNDescent.__init__).parameters.items()
    if name not in ("self", "data", "metric", "n_neighbors", "random_state", "tree_init", "init_graph", "init_dist",
                    "n_devices", "devices")
}

def make_index(data, *args, **kwargs):
    """``NNDescent(data, ...)`` on the GPU when the input is in scope (dense data, or sparse data whose dense rows fit the device
    and a metric the reference's sparse path has too; euclidean / l2 / sqeuclidean / cosine / dot /
    inner_product / correlation / hellinger / proxy_inner_product / seuclidean / mahalanobis / minkowski and wminkowski with p = 2 /
    spearmanr / haversine / the boolean metrics jaccard, dice, sokalsneath, matching, rogerstanimoto, sokalmichener, kulsinski, russellrao and yule,
    k <= 256);
    otherwise -- and only then -- the reference ``pynndescent.NNDescent`` on the CPU when that package is importable
    (SURVEY.md section 8b), with a warning.  A missing HIP library or GPU is never papered over: that still raises."""
    device = kwargs.pop("device", 0)
    try:
        return NNDescent(data, *args, device=device, **kwargs)
    except NotImplementedError as exc:
        try:
            import pynndescent
        except ImportError:
            raise exc
        warn("pynndescent_amd: %s -- building with pynndescent.NNDescent on the CPU instead" % exc)
        return pynndescent.NNDescent(data, *args, **kwargs)
