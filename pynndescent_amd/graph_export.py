"""Graph export: an index's answers as a sparse neighbour matrix, the form UMAP, t-SNE, Isomap, spectral methods and
scanpy-style pipelines consume -- ``NNDescent.kneighbors_graph`` and ``PyNNDescentTransformer`` (pynndescent_.py:2640-2868).

The k-lists become canonical CSR on the device (csrc/csr_graph.hip): one wave sorts a row by column, the symmetric form is the
min-union of the matrix and its transpose.  A device-resident index gets a ``torch.sparse_csr_tensor`` built on the kernels' own
buffers; a host index gets a ``scipy.sparse.csr_array``.  Nothing here computes on the host: it checks arguments, picks the
side and wraps the arrays.
"""
import warnings

import numpy as np

from . import _capi, device_arrays
from .metrics import _metric_of

GRAPH_MODES = ("distance", "connectivity")


def _index_on_device(index):
    """Whether the index's rows live on the device (built from a tensor): its graphs are handed out as tensors there.  An index
    built from ``scipy.sparse`` input answers with host arrays although its dense rows are on the device."""
    d = index.__dict__
    return "_device_data" in d and not d.get("_is_sparse")


def _check_arguments(index, X, k, mode, symmetric, include_self, query_kwds):
    """The argument errors of ``kneighbors_graph``, before anything runs.  Returns k."""
    if mode not in GRAPH_MODES:
        raise ValueError("mode must be one of %s (got %r)" % (", ".join(GRAPH_MODES), mode))
    if k is None:
        k = int(index.n_neighbors)
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1 (got %d)" % k)
    if X is not None:
        if symmetric:
            raise ValueError("symmetric=True needs the built graph (X=None): the answers of queries are not a square matrix")
        if not include_self:
            raise ValueError("include_self=False needs the built graph (X=None): a query row is not a row of the index")
        return k
    if query_kwds:
        raise TypeError("kneighbors_graph() takes %s only with X: the built graph is not queried" % ", ".join(sorted(query_kwds)))
    if k > int(index.n_neighbors):
        raise ValueError("k = %d, but the built graph has n_neighbors = %d columns; query for more with kneighbors_graph(X, k)"
                         % (k, int(index.n_neighbors)))
    return k


def _scipy_csr(indptr, indices, data, shape):
    import scipy.sparse as sp

    if indices.shape[0] < 2 ** 31:  # scipy keeps one integer type for both index arrays: the m + 1 offsets are narrowed
        indptr = indptr.astype(np.int32)
    out = sp.csr_array((data, indices, indptr), shape=shape)
    out.has_sorted_indices = True  # the kernels' order: columns strictly ascending, no duplicates
    out.has_canonical_format = True
    return out


def _torch_csr(torch, ids, vals, n, k, mode, symmetric, drop_self, ordinal):
    """The kernels on the (m, >= k) tensors ``ids`` (int32 / int64) and ``vals`` (float32), first ``k`` columns, on torch's
    current stream; a ``sparse_csr`` tensor that wraps the result's own buffers (they live as long as its parts)."""
    m, ld = int(ids.shape[0]), int(ids.shape[1])
    with torch.cuda.device(ordinal):
        on = device_arrays._OnTorchStream(torch, ordinal)
        csr = _capi.DeviceCsr(ordinal, on.ptr, ids.data_ptr(), ids.element_size(), vals.data_ptr(), m, k, ld, n, mode=mode,
                              symmetric=symmetric, drop_self=drop_self)
        on.done()
        device = ids.device
        indptr = torch.as_tensor(csr.indptr, device=device)
        if csr.nnz:
            indices, data = torch.as_tensor(csr.indices, device=device), torch.as_tensor(csr.data, device=device)
        else:
            indices, data = torch.empty(0, dtype=torch.int32, device=device), torch.empty(0, dtype=torch.float32, device=device)
        # torch wants one integer type for both index arrays: the m + 1 offsets are narrowed (the entries are not touched)
        narrow = csr.nnz < 2 ** 31
        with warnings.catch_warnings():  # (torch announces once per process that its CSR layout is in beta)
            warnings.filterwarnings("ignore", message="Sparse CSR tensor support is in beta state")
            out = torch.sparse_csr_tensor(indptr.to(torch.int32) if narrow else indptr, indices if narrow else indices.long(), data,
                                          size=(m, int(n)))
    return out


def _as_device_lists(torch, ids, vals, device):
    """Query answers of either side as contiguous device tensors: int32 / int64 ids, float32 values."""
    if not device_arrays._is_device_array(ids):
        ids, vals = torch.from_numpy(np.ascontiguousarray(ids)).to(device), torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32)).to(device)
    if ids.dtype not in (torch.int32, torch.int64):
        ids = ids.to(torch.int32)
    return ids.contiguous(), vals.to(torch.float32).contiguous()


def _as_host_lists(ids, vals):
    if device_arrays._is_device_array(ids):
        ids, vals = ids.detach().cpu().numpy(), vals.detach().cpu().numpy()
    return ids, np.ascontiguousarray(vals, dtype=np.float32)


def kneighbors_graph(index, X=None, k=None, mode="distance", symmetric=False, include_self=True, epsilon=0.1, **query_kwds):
    """``NNDescent.kneighbors_graph``: see there."""
    k = _check_arguments(index, X, k, mode, symmetric, include_self, query_kwds)
    n = int(index._raw_data_n())
    on_device = _index_on_device(index)
    drop_self = not include_self
    if X is not None:
        ids, vals = index.query(X, k=k, epsilon=epsilon, **query_kwds)
        if on_device:
            torch = device_arrays._torch()
            ids, vals = _as_device_lists(torch, ids, vals, index.__dict__["_device_data"].device)
            return _torch_csr(torch, ids, vals, n, k, mode, False, False, int(index.device))
        ids, vals = _as_host_lists(ids, vals)
        return _scipy_csr(*_capi.graph_csr(ids, vals, n, mode=mode, device=int(index.device)), shape=(ids.shape[0], n))
    if on_device and "_device_graph" in index.__dict__:  # the graph where it lies; its first k columns through the row stride
        torch = device_arrays._torch()
        ids, dist = index.__dict__["_device_graph"]
        m = _metric_of(index.metric)
        with torch.cuda.device(int(index.device)):
            vals = dist if m.device_kind == _capi.NND_CORRECT_COPY else device_arrays._device_corrected(torch, dist, m, int(index.device))
        return _torch_csr(torch, ids.contiguous(), vals.to(torch.float32).contiguous(), n, k, mode, symmetric, drop_self, int(index.device))
    graph = index.neighbor_graph  # host arrays, corrected (n_devices > 1, scipy input, from_graph, an updated index: the mirror)
    if graph is None:
        raise ValueError("this index was compressed: it has no neighbor graph to export")
    ids, vals = _as_host_lists(*graph)
    ids, vals = np.ascontiguousarray(ids[:, :k]), np.ascontiguousarray(vals[:, :k])
    return _scipy_csr(*_capi.graph_csr(ids, vals, n, mode=mode, symmetric=symmetric, drop_self=drop_self, device=int(index.device)),
                      shape=(ids.shape[0], n))


try:
    from sklearn.base import BaseEstimator, TransformerMixin

    _TRANSFORMER_BASES = (TransformerMixin, BaseEstimator)
except ImportError:  # without sklearn the class keeps the estimator protocol over its constructor arguments

    class _Params:
        @classmethod
        def _param_names(cls):
            import inspect

            return [p for p in inspect.signature(cls.__init__).parameters if p != "self"]

        def get_params(self, deep=True):
            return {name: getattr(self, name) for name in self._param_names()}

        def set_params(self, **params):
            names = self._param_names()
            for name, value in params.items():
                if name not in names:
                    raise ValueError("Invalid parameter %r for estimator %s" % (name, type(self).__name__))
                setattr(self, name, value)
            return self

    _TRANSFORMER_BASES = (_Params,)


class PyNNDescentTransformer(*_TRANSFORMER_BASES):
    """``pynndescent.PyNNDescentTransformer`` (pynndescent_.py:2640-2868) on the GPU: fits an ``NNDescent`` index with
    ``n_neighbors + 1`` neighbours (sklearn does not count a point as its own neighbour) and hands out sparse neighbour graphs
    -- ``scipy.sparse.csr_array`` for host data, ``torch.sparse_csr_tensor`` for a device tensor.  Constructor arguments and
    attributes are the reference's; unsupported metrics or parameters raise what ``NNDescent`` raises.  Beyond the reference the
    columns of every row are sorted, and ``fit_transform`` leaves the index uncompressed, so ``transform(None)`` works after it."""

    def __init__(
        self,
        n_neighbors=30,
        metric="euclidean",
        metric_kwds=None,
        n_trees=None,
        leaf_size=None,
        search_epsilon=0.1,
        pruning_degree_multiplier=1.5,
        diversify_prob=1.0,
        n_search_trees=1,
        tree_init=True,
        random_state=None,
        n_jobs=None,
        low_memory=True,
        max_candidates=None,
        n_iters=None,
        early_termination_value=0.001,
        parallel_batch_queries=False,
        verbose=False,
    ):
        self.n_neighbors = n_neighbors
        self.metric = metric
        self.metric_kwds = metric_kwds
        self.n_trees = n_trees
        self.leaf_size = leaf_size
        self.search_epsilon = search_epsilon
        self.pruning_degree_multiplier = pruning_degree_multiplier
        self.diversify_prob = diversify_prob
        self.n_search_trees = n_search_trees
        self.tree_init = tree_init
        self.random_state = random_state
        self.low_memory = low_memory
        self.max_candidates = max_candidates
        self.n_iters = n_iters
        self.early_termination_value = early_termination_value
        self.n_jobs = n_jobs
        self.parallel_batch_queries = parallel_batch_queries
        self.verbose = verbose

    def fit(self, X, compress_index=True):
        """Build the index on ``X`` (pynndescent_.py:2750-2800)."""
        from .nndescent import NNDescent

        self.n_samples_fit = X.shape[0]
        self.index_ = NNDescent(
            X,
            metric=self.metric,
            metric_kwds={} if self.metric_kwds is None else self.metric_kwds,
            n_neighbors=self.n_neighbors + 1,
            n_trees=self.n_trees,
            leaf_size=self.leaf_size,
            pruning_degree_multiplier=self.pruning_degree_multiplier,
            diversify_prob=self.diversify_prob,
            n_search_trees=self.n_search_trees,
            tree_init=self.tree_init,
            random_state=self.random_state,
            low_memory=self.low_memory,
            max_candidates=self.max_candidates,
            n_iters=self.n_iters,
            delta=self.early_termination_value,
            n_jobs=self.n_jobs,
            compressed=compress_index,
            parallel_batch_queries=self.parallel_batch_queries,
            verbose=self.verbose,
        )
        return self

    def transform(self, X, y=None):
        """The (n_samples_transform, n_samples_fit) graph of the ``n_neighbors`` nearest indexed rows of every row of ``X``;
        ``X`` None: the built graph, ``n_neighbors + 1`` entries per row with the diagonal explicit (pynndescent_.py:2802-2838)."""
        if X is None:
            return self.index_.kneighbors_graph()
        return self.index_.kneighbors_graph(X, k=self.n_neighbors, epsilon=self.search_epsilon)

    def fit_transform(self, X, y=None, **fit_params):
        """``fit`` and the built graph (pynndescent_.py:2840-2867); the diagonal is explicit."""
        self.fit(X, compress_index=False)
        return self.transform(X=None)


__all__ = ["GRAPH_MODES", "PyNNDescentTransformer", "kneighbors_graph"]
