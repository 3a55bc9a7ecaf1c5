"""The shared-nearest-neighbour graph of a k-NN graph on the GPU: every k-NN edge weighted by the neighbours its two ends share,
as a count or as the Jaccard index of the two neighbour sets (PhenoGraph, Seurat's ``FindNeighbors``, scran's ``buildSNNGraph``
``"jaccard"`` / ``"number"``), the matrix graph clustering runs on (csrc/snn.hip, and the merge of csrc/csr_graph.hip).
``NNDescent.shared_neighbor_graph`` runs on the built graph, ``shared_neighbor_graph`` on k-lists the caller already has.  Device
k-lists give a ``torch.sparse_csr_tensor``, host k-lists a ``scipy.sparse.csr_array``.  Nothing here computes on the host: it
checks arguments, picks the side and wraps the arrays.
"""
import numpy as np

from . import _capi, device_arrays
from .graph_export import _index_on_device, _scipy_csr, _wrap_device_csr


def _check_arguments(n_neighbors, weight, prune):
    k = int(n_neighbors)
    if k < 2 or k > _capi.CSR_MAX_K:
        raise ValueError("n_neighbors must be between 2 and %d (got %d)" % (_capi.CSR_MAX_K, k))
    _capi._snn_weight(weight)
    if not float(prune) >= 0.0:
        raise ValueError("prune must be 0 or above (got %r)" % (prune,))
    return k


def _on_device(torch, ids, k, params, ordinal):
    """The kernels on the (m, >= k) device tensor whose rows are ``ids.stride(0)`` apart, first ``k`` columns, on torch's
    current stream."""
    m, ld = int(ids.shape[0]), int(ids.stride(0))
    with torch.cuda.device(ordinal):
        on = device_arrays._OnTorchStream(torch, ordinal)
        csr = _capi.DeviceSnnGraph(ordinal, on.ptr, ids.data_ptr(), ids.element_size(), m, k, ld, *params)
        on.done()
        return _wrap_device_csr(torch, csr, ids.device)


def _on_host(ids, params, device):
    indptr, indices, data = _capi.snn_graph(ids, *params, device=device)
    return _scipy_csr(indptr, indices, data, shape=(ids.shape[0], ids.shape[0]))


def shared_neighbor_graph(knn_indices, weight="jaccard", include_self=True, prune=0.0, symmetric=True, device=0):
    """The shared-neighbour graph of the square k-lists ``knn_indices`` (m, k) int32 / int64: row i is point i, a place whose
    id is outside [0, m) is empty.  With O(i) the distinct ids of row i other than i and N(i) = O(i) + {i} (``include_self``)
    or O(i), every i and j in O(i) is an edge of c = |N(i) & N(j)| shared neighbours; its weight is c (``weight="count"``) or
    c / (|N(i)| + |N(j)| - c) (``"jaccard"``), stored when it is above 0 and at least ``prune`` (Seurat's ``prune.SNN``).
    ``symmetric`` joins the matrix with its transpose.  Returns the (m, m) matrix: for a tensor on a HIP device a
    ``torch.sparse_csr_tensor`` there, on torch's current stream; for a numpy array a canonical ``scipy.sparse.csr_array``,
    computed on ``device``."""
    if len(knn_indices.shape) != 2:
        raise ValueError("knn_indices must be one (m, k) array")
    k = _check_arguments(knn_indices.shape[1], weight, prune)
    params = (weight, bool(include_self), float(prune), bool(symmetric))
    if device_arrays._is_device_array(knn_indices):
        torch = device_arrays._torch()
        if knn_indices.dtype not in (torch.int32, torch.int64):
            raise ValueError("knn_indices must be int32 or int64 (got %s)" % (knn_indices.dtype,))
        rows_apart = knn_indices.stride(1) == 1 and knn_indices.stride(0) >= k  # the first columns of a wider tensor: read where they lie
        ids = knn_indices if rows_apart else knn_indices.contiguous()
        return _on_device(torch, ids, k, params, int(ids.device.index or 0))
    ids = np.asarray(knn_indices)
    if ids.dtype.kind not in "iu":
        raise ValueError("knn_indices must be int32 or int64 (got %s)" % (ids.dtype,))
    return _on_host(ids, params, int(device))


def index_shared_neighbor_graph(index, n_neighbors=None, weight="jaccard", include_self=True, prune=0.0, symmetric=True):
    """``NNDescent.shared_neighbor_graph``: see there.  The k-lists are taken as ``kneighbors_graph(X=None)`` takes them."""
    k = _check_arguments(index.n_neighbors if n_neighbors is None else n_neighbors, weight, prune)
    if k > int(index.n_neighbors):
        raise ValueError("n_neighbors = %d, but the built graph has n_neighbors = %d columns" % (k, int(index.n_neighbors)))
    params = (weight, bool(include_self), float(prune), bool(symmetric))
    if _index_on_device(index) and "_device_graph" in index.__dict__:  # the graph where it lies; its first k columns through the row stride
        torch = device_arrays._torch()
        ids = index.__dict__["_device_graph"][0]
        return _on_device(torch, ids.contiguous(), k, params, int(index.device))
    graph = index.neighbor_graph  # host arrays (n_devices > 1, scipy input, from_graph, an updated index: the mirror)
    if graph is None:
        raise ValueError("this index was compressed: it has no neighbor graph to export")
    ids = graph[0].detach().cpu().numpy() if device_arrays._is_device_array(graph[0]) else np.asarray(graph[0])
    return _on_host(np.ascontiguousarray(ids[:, :k]), params, int(index.device))


__all__ = ["shared_neighbor_graph", "index_shared_neighbor_graph"]
