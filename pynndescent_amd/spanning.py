"""The minimum spanning forest of a k-NN graph's mutual-reachability weights, and the graph's connected components, on the GPU:
what HDBSCAN and robust single linkage start from (core distances, mutual reachability, the spanning forest) and what UMAP's
spectral initialisation, scanpy and Isomap ask of a graph (its components) -- csrc/mst.hip, and the merge of
csrc/csr_graph.hip.  ``NNDescent.spanning_forest`` runs on the built graph, ``spanning_forest`` on k-lists the caller already
has.  Device k-lists give a ``torch.sparse_csr_tensor`` and two tensors, host k-lists a ``scipy.sparse.csr_array`` and two
arrays.  Nothing here computes on the host: it checks arguments, picks the side and wraps the arrays.
"""
import numpy as np

from . import _capi, device_arrays
from .graph_export import _index_on_device, _scipy_csr, _wrap_device_csr
from .metrics import _metric_of


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


__all__ = ["spanning_forest", "index_spanning_forest"]
