"""t-SNE's perplexity affinities (sklearn's ``_binary_search_perplexity`` and ``P + P.T``, openTSNE's multiscale form) of a k-NN
graph on the GPU: the per-row search for the Gaussian precision beta, the conditional matrix, its symmetrisation and the
division by its total (csrc/affinity.hip, and the merge of csrc/csr_graph.hip).  ``NNDescent.perplexity_affinities`` runs on
the built graph, ``perplexity_affinities`` on k-lists the caller already has.  Device k-lists give a
``torch.sparse_csr_tensor`` and a tensor, host k-lists a ``scipy.sparse.csr_array`` and an array.  Nothing here computes on
the host: it checks arguments, picks the side and wraps the arrays.
"""
import numpy as np

from . import _capi, device_arrays
from .graph_export import _as_device_lists, _as_host_lists, _index_on_device, _scipy_csr, _wrap_device_csr
from .metrics import _metric_of


def _check_arguments(n_neighbors, perplexity):
    """(k, the perplexities as a list, whether one scalar was given)."""
    k = int(n_neighbors)
    if k < 1 or k > _capi.CSR_MAX_K:
        raise ValueError("n_neighbors must be between 1 and %d (got %d)" % (_capi.CSR_MAX_K, k))
    scalar = np.ndim(perplexity) == 0
    scales = [float(p) for p in np.atleast_1d(np.asarray(perplexity, dtype=np.float64))]
    if not 1 <= len(scales) <= _capi.AFFINITY_MAX_SCALES:
        raise ValueError("perplexity must be one value or a sequence of at most %d (got %d)" % (_capi.AFFINITY_MAX_SCALES, len(scales)))
    if not all(0.0 < p < np.inf for p in scales):
        raise ValueError("perplexity must be above 0 and finite (got %r)" % (perplexity,))
    return k, scales, scalar


def _on_device(torch, ids, dists, n, k, scales, scalar, flags, ordinal):
    """The kernels on the (m, >= k) device tensors, first ``k`` columns, on torch's current stream."""
    m, ld = int(ids.shape[0]), int(ids.shape[1])
    with torch.cuda.device(ordinal):
        betas = torch.empty((m, len(scales)), dtype=torch.float32, device=ids.device)
        on = device_arrays._OnTorchStream(torch, ordinal)
        csr = _capi.DeviceAffinities(ordinal, on.ptr, ids.data_ptr(), ids.element_size(), dists.data_ptr(), m, k, ld, n, scales, *flags,
                                     betas.data_ptr())
        on.done()
        return _wrap_device_csr(torch, csr, ids.device), betas[:, 0] if scalar else betas


def _on_host(ids, dists, n, scales, scalar, flags, device):
    indptr, indices, data, betas = _capi.perplexity_affinities(ids, dists, n, scales, *flags, device=device)
    return _scipy_csr(indptr, indices, data, shape=(ids.shape[0], n)), betas[:, 0] if scalar else betas


def perplexity_affinities(knn_indices, knn_dists, n_points=None, perplexity=30.0, squared=True, symmetrize=True, normalize=True, device=0):
    """The perplexity affinities of the k-lists ``knn_indices`` (m, k) int32 / int64 and ``knn_dists`` (m, k); ``n_points``
    (default m) is the number of columns.  A place whose id is negative or, with the default ``n_points``, not below m is
    empty; with ``n_points == m`` a row's own id is left out.  ``symmetrize=False`` gives the row-normalised conditional
    matrix, the form an embedding of new points takes from ``query()`` answers.  Returns ``(P, betas)``: for tensors on a HIP
    device a ``torch.sparse_csr_tensor`` and a float32 tensor there, on torch's current stream; for numpy arrays a canonical
    ``scipy.sparse.csr_array`` and a float32 array, computed on ``device``.  ``betas`` is (m,), or (m, S) for S perplexities."""
    if len(knn_indices.shape) != 2 or tuple(knn_dists.shape) != tuple(knn_indices.shape):
        raise ValueError("knn_indices and knn_dists must be two (m, k) arrays of one shape")
    m = int(knn_indices.shape[0])
    k, scales, scalar = _check_arguments(knn_indices.shape[1], perplexity)
    n = m if n_points is None else int(n_points)
    if n < 1:
        raise ValueError("n_points must be at least 1 (got %d)" % n)
    if symmetrize and m != n:
        raise ValueError("symmetrize=True needs square k-lists: %d rows, n_points = %d" % (m, n))
    if n_points is not None and m > 0 and int(knn_indices.max()) >= n:
        raise ValueError("n_points = %d, but knn_indices holds the id %d" % (n, int(knn_indices.max())))
    flags = (bool(squared), bool(symmetrize), bool(normalize))
    if device_arrays._is_device_array(knn_indices):
        torch = device_arrays._torch()
        ids, dists = _as_device_lists(torch, knn_indices, knn_dists, knn_indices.device)
        return _on_device(torch, ids, dists, n, k, scales, scalar, flags, int(ids.device.index or 0))
    ids, dists = _as_host_lists(knn_indices, knn_dists)
    return _on_host(np.ascontiguousarray(ids), dists, n, scales, scalar, flags, int(device))


def index_perplexity_affinities(index, perplexity=30.0, n_neighbors=None, squared=True, symmetrize=True, normalize=True):
    """``NNDescent.perplexity_affinities``: see there.  The k-lists are taken as ``kneighbors_graph(X=None)`` takes them."""
    k, scales, scalar = _check_arguments(min(int(index.n_neighbors), _capi.CSR_MAX_K) if n_neighbors is None else n_neighbors, perplexity)
    if k > int(index.n_neighbors):
        raise ValueError("n_neighbors = %d, but the built graph has n_neighbors = %d columns" % (k, int(index.n_neighbors)))
    n = int(index._raw_data_n())
    flags = (bool(squared), bool(symmetrize), bool(normalize))
    if _index_on_device(index) and "_device_graph" in index.__dict__:  # the graph where it lies; its first k columns through the row stride
        torch = device_arrays._torch()
        ids, dist = index.__dict__["_device_graph"]
        metric = _metric_of(index.metric)
        with torch.cuda.device(int(index.device)):
            dists = dist if metric.device_kind == _capi.NND_CORRECT_COPY else device_arrays._device_corrected(torch, dist, metric, int(index.device))
        return _on_device(torch, ids.contiguous(), dists.to(torch.float32).contiguous(), n, k, scales, scalar, flags, int(index.device))
    graph = index.neighbor_graph  # host arrays, corrected (n_devices > 1, scipy input, from_graph, an updated index: the mirror)
    if graph is None:
        raise ValueError("this index was compressed: it has no neighbor graph to export")
    ids, dists = _as_host_lists(*graph)
    return _on_host(np.ascontiguousarray(ids[:, :k]), np.ascontiguousarray(dists[:, :k]), n, scales, scalar, flags, int(index.device))


__all__ = ["perplexity_affinities", "index_perplexity_affinities"]
