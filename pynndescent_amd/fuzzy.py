"""UMAP's fuzzy simplicial set (``umap.umap_.fuzzy_simplicial_set`` with a precomputed k-NN graph) on the GPU: the per-row
bisection for sigma and rho, the membership strengths and the fuzzy union with the transpose (csrc/fuzzy.hip, and the merge
of csrc/csr_graph.hip).  ``NNDescent.fuzzy_simplicial_set`` runs on the built graph, ``fuzzy_simplicial_set`` on k-lists the
caller already has.  Device k-lists give a ``torch.sparse_csr_tensor`` and two tensors, host k-lists a
``scipy.sparse.csr_array`` and two arrays.  Nothing here computes on the host: it checks arguments, picks the side and wraps
the arrays.
"""
import numpy as np

from . import _capi, device_arrays
from .graph_export import _as_device_lists, _as_host_lists, _index_on_device, _scipy_csr, _wrap_device_csr
from .metrics import _metric_of


def _check_arguments(n_neighbors, set_op_mix_ratio, local_connectivity, bandwidth):
    k = int(n_neighbors)
    if k < 2 or k > _capi.CSR_MAX_K:
        raise ValueError("n_neighbors must be between 2 and %d (got %d)" % (_capi.CSR_MAX_K, k))
    if not 0.0 < float(local_connectivity) <= k - 1:
        raise ValueError("local_connectivity must be above 0 and at most n_neighbors - 1 = %d (got %r)" % (k - 1, local_connectivity))
    if not float(bandwidth) > 0.0:
        raise ValueError("bandwidth must be above 0 (got %r)" % (bandwidth,))
    if not 0.0 <= float(set_op_mix_ratio) <= 1.0:
        raise ValueError("set_op_mix_ratio must lie in [0, 1] (got %r)" % (set_op_mix_ratio,))
    return k


def _on_device(torch, ids, dists, n, k, params, ordinal):
    """The kernels on the (m, >= k) device tensors, first ``k`` columns, on torch's current stream."""
    m, ld = int(ids.shape[0]), int(ids.shape[1])
    with torch.cuda.device(ordinal):
        sigmas, rhos = torch.empty(m, dtype=torch.float32, device=ids.device), torch.empty(m, dtype=torch.float32, device=ids.device)
        on = device_arrays._OnTorchStream(torch, ordinal)
        csr = _capi.DeviceFuzzySet(ordinal, on.ptr, ids.data_ptr(), ids.element_size(), dists.data_ptr(), m, k, ld, n, *params,
                                   sigmas.data_ptr(), rhos.data_ptr())
        on.done()
        return _wrap_device_csr(torch, csr, ids.device), sigmas, rhos


def _on_host(ids, dists, n, params, device):
    indptr, indices, data, sigmas, rhos = _capi.fuzzy_set(ids, dists, n, *params, device=device)
    return _scipy_csr(indptr, indices, data, shape=(ids.shape[0], n)), sigmas, rhos


def fuzzy_simplicial_set(knn_indices, knn_dists, n_points=None, set_op_mix_ratio=1.0, local_connectivity=1.0, bandwidth=1.0,
                         apply_set_operations=True, device=0):
    """The fuzzy simplicial set of the k-lists ``knn_indices`` (m, k) int32 / int64 and ``knn_dists`` (m, k), UMAP's
    ``precomputed_knn`` form; ``n_points`` (default m) is the number of columns.  A place whose id is negative or not below
    ``n_points`` is empty.  Returns ``(graph, sigmas, rhos)``: for tensors on a HIP device a ``torch.sparse_csr_tensor`` and two
    float32 tensors there, on torch's current stream; for numpy arrays a canonical ``scipy.sparse.csr_array`` and two float32
    arrays, computed on ``device``."""
    if len(knn_indices.shape) != 2 or tuple(knn_dists.shape) != tuple(knn_indices.shape):
        raise ValueError("knn_indices and knn_dists must be two (m, k) arrays of one shape")
    m = int(knn_indices.shape[0])
    k = _check_arguments(knn_indices.shape[1], set_op_mix_ratio, local_connectivity, bandwidth)
    n = m if n_points is None else int(n_points)
    if apply_set_operations and m != n:
        raise ValueError("apply_set_operations=True needs square k-lists: %d rows, n_points = %d" % (m, n))
    params = (float(local_connectivity), float(bandwidth), float(set_op_mix_ratio), bool(apply_set_operations))
    if device_arrays._is_device_array(knn_indices):
        torch = device_arrays._torch()
        ids, dists = _as_device_lists(torch, knn_indices, knn_dists, knn_indices.device)
        return _on_device(torch, ids, dists, n, k, params, int(ids.device.index or 0))
    ids, dists = _as_host_lists(knn_indices, knn_dists)
    return _on_host(np.ascontiguousarray(ids), dists, n, params, int(device))


def index_fuzzy_simplicial_set(index, n_neighbors=None, set_op_mix_ratio=1.0, local_connectivity=1.0, bandwidth=1.0, apply_set_operations=True):
    """``NNDescent.fuzzy_simplicial_set``: see there.  The k-lists are taken as ``kneighbors_graph(X=None)`` takes them."""
    k = _check_arguments(index.n_neighbors if n_neighbors is None else n_neighbors, set_op_mix_ratio, local_connectivity, bandwidth)
    if k > int(index.n_neighbors):
        raise ValueError("n_neighbors = %d, but the built graph has n_neighbors = %d columns" % (k, int(index.n_neighbors)))
    n = int(index._raw_data_n())
    params = (float(local_connectivity), float(bandwidth), float(set_op_mix_ratio), bool(apply_set_operations))
    if _index_on_device(index) and "_device_graph" in index.__dict__:  # the graph where it lies; its first k columns through the row stride
        torch = device_arrays._torch()
        ids, dist = index.__dict__["_device_graph"]
        m = _metric_of(index.metric)
        with torch.cuda.device(int(index.device)):
            dists = dist if m.device_kind == _capi.NND_CORRECT_COPY else device_arrays._device_corrected(torch, dist, m, int(index.device))
        return _on_device(torch, ids.contiguous(), dists.to(torch.float32).contiguous(), n, k, params, int(index.device))
    graph = index.neighbor_graph  # host arrays, corrected (n_devices > 1, scipy input, from_graph, an updated index: the mirror)
    if graph is None:
        raise ValueError("this index was compressed: it has no neighbor graph to export")
    ids, dists = _as_host_lists(*graph)
    return _on_host(np.ascontiguousarray(ids[:, :k]), np.ascontiguousarray(dists[:, :k]), n, params, int(index.device))


__all__ = ["fuzzy_simplicial_set", "index_fuzzy_simplicial_set"]
