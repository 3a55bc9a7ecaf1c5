"""The minimum spanning forest of a k-NN graph's mutual-reachability weights, and the graph's connected components, on the GPU:
what HDBSCAN and robust single linkage start from (core distances, mutual reachability, the spanning forest) and what UMAP's
spectral initialisation, scanpy and Isomap ask of a graph (its components) -- csrc/mst.hip, and the merge of
csrc/csr_graph.hip.  ``NNDescent.spanning_forest`` runs on the built graph, ``spanning_forest`` on k-lists the caller already
has.  Device k-lists give a ``torch.sparse_csr_tensor`` and two tensors, host k-lists a ``scipy.sparse.csr_array`` and two
arrays.  ``spanning_tree`` / ``NNDescent.spanning_tree`` join the forest's components by cross-component searches over the
rows themselves (csrc/cross.hip) and return one tree.  Nothing here computes on the host: it checks arguments, picks the side and
wraps the arrays.
"""
import numpy as np

from . import _capi, device_arrays
from .graph_export import _index_on_device, _scipy_csr, _wrap_device_csr
from .metrics import _metric_of, _metric_record

TREE_METRICS = ("euclidean", "l2", "sqeuclidean", "cosine")  # the spaces csrc/cross.hip carries its rounding band through


def _check_arguments(n_neighbors, min_samples):
    k, s = int(n_neighbors), int(min_samples)
    if k < 1 or k > _capi.CSR_MAX_K:
        raise ValueError("n_neighbors must be between 1 and %d (got %d)" % (_capi.CSR_MAX_K, k))
    if s < 0 or s > k:
        raise ValueError("min_samples must be between 0 and n_neighbors = %d (got %d)" % (k, s))
    return k, s


def _rows_apart(t, k):
    """``t`` when its first ``k`` columns can be read where they lie, through the row stride; else a contiguous copy."""
    return t if t.stride(1) == 1 and t.stride(0) >= k else t.contiguous()


def _on_device(torch, ids, dists, k, min_samples, ordinal):
    """The kernels on the (m, >= k) device tensors, first ``k`` columns through each one's row stride, on torch's current stream."""
    m = int(ids.shape[0])
    with torch.cuda.device(ordinal):
        labels = torch.empty(m, dtype=torch.int32, device=ids.device)
        core = torch.empty(m, dtype=torch.float32, device=ids.device)
        on = device_arrays._OnTorchStream(torch, ordinal)
        csr = _capi.DeviceSpanningForest(ordinal, on.ptr, ids.data_ptr(), ids.element_size(), dists.data_ptr(), m, k, int(ids.stride(0)),
                                         int(dists.stride(0)), min_samples, labels.data_ptr(), core.data_ptr())
        on.done()
        return _wrap_device_csr(torch, csr, ids.device), labels, core


def _on_host(ids, dists, min_samples, device):
    indptr, indices, data, labels, core = _capi.spanning_forest(ids, dists, min_samples, device=device)
    return _scipy_csr(indptr, indices, data, shape=(ids.shape[0], ids.shape[0])), labels, core


def spanning_forest(knn_indices, knn_dists, min_samples=5, device=0):
    """The minimum spanning forest of the square k-lists ``knn_indices`` (m, k) int32 / int64 and ``knn_dists`` (m, k)
    float32 under mutual reachability: row i is point i; a place counts when its id lies in [0, m), is not i, and its distance
    is finite and not negative.  ``core(i)`` is the ``min_samples``-th smallest distance of row i (the row's own place counts
    when it is listed; 0 with ``min_samples=0``: plain single linkage), an edge weighs ``max(core(i), core(j), d)``, and ties are
    broken by (weight, min(i, j), max(i, j)), so the forest is a function of the input.  Returns ``(forest, labels,
    core_distances)``: the exactly symmetric (m, m) forest with zero weights stored, the int32 connected component of every
    point numbered as ``scipy.sparse.csgraph.connected_components`` numbers them, and the float32 core distances -- for tensors
    on a HIP device a ``torch.sparse_csr_tensor`` and two tensors there, on torch's current stream; for numpy arrays a canonical
    ``scipy.sparse.csr_array`` and two arrays, computed on ``device``."""
    if len(knn_indices.shape) != 2 or tuple(knn_dists.shape) != tuple(knn_indices.shape):
        raise ValueError("knn_indices and knn_dists must be two (m, k) arrays of one shape")
    k, min_samples = _check_arguments(knn_indices.shape[1], min_samples)
    if device_arrays._is_device_array(knn_indices):
        torch = device_arrays._torch()
        if knn_indices.dtype not in (torch.int32, torch.int64) or knn_dists.dtype != torch.float32:
            raise ValueError("knn_indices must be int32 or int64 and knn_dists float32 (got %s, %s)" % (knn_indices.dtype, knn_dists.dtype))
        if not device_arrays._is_device_array(knn_dists) or knn_dists.device != knn_indices.device:
            raise ValueError("knn_indices and knn_dists must lie on one device")
        return _on_device(torch, _rows_apart(knn_indices, k), _rows_apart(knn_dists, k), k, min_samples, int(knn_indices.device.index or 0))
    ids, dists = np.asarray(knn_indices), np.asarray(knn_dists)
    if ids.dtype not in (np.int32, np.int64) or dists.dtype != np.float32:
        raise ValueError("knn_indices must be int32 or int64 and knn_dists float32 (got %s, %s)" % (ids.dtype, dists.dtype))
    return _on_host(ids, dists, min_samples, int(device))


def index_spanning_forest(index, min_samples=5, n_neighbors=None):
    """``NNDescent.spanning_forest``: see there.  The k-lists are taken as ``kneighbors_graph(X=None)`` takes them."""
    k, min_samples = _check_arguments(index.n_neighbors if n_neighbors is None else n_neighbors, min_samples)
    if k > int(index.n_neighbors):
        raise ValueError("n_neighbors = %d, but the built graph has n_neighbors = %d columns" % (k, int(index.n_neighbors)))
    if _index_on_device(index) and "_device_graph" in index.__dict__:  # the graph where it lies; its first k columns through the row stride
        torch = device_arrays._torch()
        ids, dist = index.__dict__["_device_graph"]
        m = _metric_of(index.metric)
        with torch.cuda.device(int(index.device)):
            dists = dist if m.device_kind == _capi.NND_CORRECT_COPY else device_arrays._device_corrected(torch, dist, m, int(index.device))
        return _on_device(torch, ids.contiguous(), dists.to(torch.float32).contiguous(), k, min_samples, int(index.device))
    graph = index.neighbor_graph  # host arrays, corrected (n_devices > 1, scipy input, from_graph, an updated index: the mirror)
    if graph is None:
        raise ValueError("this index was compressed: it has no neighbor graph to export")
    ids = graph[0].detach().cpu().numpy() if device_arrays._is_device_array(graph[0]) else np.asarray(graph[0])
    dists = graph[1].detach().cpu().numpy() if device_arrays._is_device_array(graph[1]) else np.asarray(graph[1])
    return _on_host(np.ascontiguousarray(ids[:, :k]), np.ascontiguousarray(dists[:, :k], dtype=np.float32), min_samples, int(index.device))


def _check_tree_metric(metric, n_neighbors):
    """What the spanning tree refuses, before any device work; returns the metric's record."""
    if callable(metric) or metric not in TREE_METRICS:
        _metric_record(metric)  # (a name nobody knows: the reference's ValueError)
        raise NotImplementedError("pynndescent_amd.spanning_tree covers the metrics %s (got %r)" % (", ".join(TREE_METRICS), metric))
    if int(n_neighbors) > 256:
        raise NotImplementedError("pynndescent_amd.spanning_tree takes k-lists of at most 256 columns (got %d)" % int(n_neighbors))
    return _metric_record(metric)


def spanning_tree(data, knn_indices, knn_dists, metric="euclidean", min_samples=5, device=0, return_stats=False, _flags=0):
    """One spanning tree of the points ``data`` (m, d) under mutual reachability: the spanning forest of their square k-lists
    ``knn_indices`` / ``knn_dists`` (the argument rules of ``spanning_forest``; distances in ``metric``'s own space), and its
    components joined on the GPU by their lightest cross-component edges (csrc/cross.hip).  For i and j in different components
    an edge weighs ``max(core(i), core(j), d(i, j))`` with ``d`` the float32 rounding of the float64 distance of the two rows; ties
    are broken by (weight, min(i, j), max(i, j)); the components are joined by the minimum spanning tree of those weights.
    Returns ``(tree, core_distances, n_components)``: the exactly symmetric (m, m) matrix with zero weights stored and m - 1
    edges, the float32 core distances, and the number of components the forest had -- for tensors on a HIP device a
    ``torch.sparse_csr_tensor`` and a tensor there, on torch's current stream; for numpy arrays a canonical
    ``scipy.sparse.csr_array`` and an array, computed on ``device``.  ``tree`` is the forest plus the joining edges, not the minimum
    spanning tree of the complete mutual-reachability graph: a cross edge may make a forest edge redundant.  ``return_stats``
    adds the call's statistics (rounds, query rows, rows that took the float64 tier).  Metrics: euclidean, l2, sqeuclidean, cosine."""
    if len(knn_indices.shape) != 2 or tuple(knn_dists.shape) != tuple(knn_indices.shape):
        raise ValueError("knn_indices and knn_dists must be two (m, k) arrays of one shape")
    m = _check_tree_metric(metric, knn_indices.shape[1])
    k, min_samples = _check_arguments(knn_indices.shape[1], min_samples)
    if len(data.shape) != 2 or int(data.shape[0]) != int(knn_indices.shape[0]):
        raise ValueError("data must have shape (m, d) with one row per row of the k-lists (got %s; m = %d)" % (tuple(data.shape), knn_indices.shape[0]))
    n, euclidean = int(data.shape[0]), metric in ("euclidean", "l2")
    aux = dict(rng_state=[1, 2, 3], tree_rng=[4, 5, 6], flags=_capi.NND_FLAG_NO_GRAPH | int(_flags))
    if device_arrays._is_device_array(data):
        torch = device_arrays._torch()
        data, dtype, ordinal = device_arrays._check_device_array(data, device)
        ids, dists = knn_indices, knn_dists
        if not (device_arrays._is_device_array(ids) and device_arrays._is_device_array(dists) and ids.device == data.device and dists.device == data.device):
            raise ValueError("data, knn_indices and knn_dists must lie on one device")
        if ids.dtype not in (torch.int32, torch.int64) or dists.dtype != torch.float32:
            raise ValueError("knn_indices must be int32 or int64 and knn_dists float32 (got %s, %s)" % (ids.dtype, dists.dtype))
        ids, dists = _rows_apart(ids, k), _rows_apart(dists, k)
        with torch.cuda.device(ordinal):
            core = torch.empty(n, dtype=torch.float32, device=data.device)
            on = device_arrays._OnTorchStream(torch, ordinal)
            builder = _capi.Builder(n, int(data.shape[1]), m.code, max(1, min(k, n)), 0, 60, 200, max(1, min(60, k, n)), 1, 0.001, device=ordinal, **aux)
            try:
                builder.set_stream(on.ptr)
                builder.set_data_device_typed(data.data_ptr(), dtype, keepalive=data)
                csr = _capi.DeviceSpanningTree(builder, ids.data_ptr(), ids.element_size(), dists.data_ptr(), k, int(ids.stride(0)), int(dists.stride(0)),
                                               min_samples, euclidean, core.data_ptr())
            finally:
                builder.close()
                on.done()
            out = (_wrap_device_csr(torch, csr, data.device), core, csr.stats["n_components"])
            return out + (csr.stats,) if return_stats else out
    data, ids, dists = np.ascontiguousarray(data, dtype=np.float32), np.asarray(knn_indices), np.asarray(knn_dists)
    if ids.dtype not in (np.int32, np.int64) or dists.dtype != np.float32:
        raise ValueError("knn_indices must be int32 or int64 and knn_dists float32 (got %s, %s)" % (ids.dtype, dists.dtype))
    builder = _capi.Builder(n, data.shape[1], m.code, max(1, min(k, n)), 0, 60, 200, max(1, min(60, k, n)), 1, 0.001, device=int(device), **aux)
    try:
        builder.set_data_host(data)
        indptr, indices, values, core, stats = _capi.spanning_tree(builder, ids, dists, min_samples, euclidean)
    finally:
        builder.close()
    out = (_scipy_csr(indptr, indices, values, shape=(n, n)), core, stats["n_components"])
    return out + (stats,) if return_stats else out


def index_spanning_tree(index, min_samples=5, n_neighbors=None):
    """``NNDescent.spanning_tree``: see there.  The k-lists are taken as ``spanning_forest`` takes them, the rows where the index
    holds them: on the device for a device-resident index, else the host rows (the mirror of an index built with ``n_devices`` > 1)."""
    _check_tree_metric(index.metric, index.n_neighbors if n_neighbors is None else n_neighbors)
    k, min_samples = _check_arguments(index.n_neighbors if n_neighbors is None else n_neighbors, min_samples)
    if k > int(index.n_neighbors):
        raise ValueError("n_neighbors = %d, but the built graph has n_neighbors = %d columns" % (k, int(index.n_neighbors)))
    d = index.__dict__
    if _index_on_device(index) and "_device_graph" in d and "_device_data" in d:
        torch = device_arrays._torch()
        ids, dist = d["_device_graph"]
        m = _metric_of(index.metric)
        with torch.cuda.device(int(index.device)):
            dists = dist if m.device_kind == _capi.NND_CORRECT_COPY else device_arrays._device_corrected(torch, dist, m, int(index.device))
        return spanning_tree(d["_device_data"], ids.contiguous()[:, :k], dists.to(torch.float32).contiguous()[:, :k], index.metric, min_samples, int(index.device))
    graph = index.neighbor_graph
    if graph is None or d.get("_is_sparse") or getattr(index, "_raw_data", None) is None:
        raise ValueError("this index does not hold its rows and its neighbor graph (compressed, or made by from_graph): "
                         "spanning_tree searches the rows themselves")
    rows = index._raw_data
    if hasattr(index, "_vertex_order"):  # prepare() keeps the rows in the search tree's leaf order; the graph keeps its numbering
        rows = rows[np.argsort(index._vertex_order), :]
    ids = graph[0].detach().cpu().numpy() if device_arrays._is_device_array(graph[0]) else np.asarray(graph[0])
    dists = graph[1].detach().cpu().numpy() if device_arrays._is_device_array(graph[1]) else np.asarray(graph[1])
    return spanning_tree(rows, np.ascontiguousarray(ids[:, :k]), np.ascontiguousarray(dists[:, :k], dtype=np.float32), index.metric, min_samples,
                         int(index.device))


__all__ = ["spanning_forest", "index_spanning_forest", "spanning_tree", "index_spanning_tree"]
