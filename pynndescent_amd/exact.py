"""The exact brute-force search (csrc/exact.hip): ``exact_knn`` on host arrays and on device arrays.
"""
import numpy as np

from . import _capi, device_arrays, row_map, sparse_input, tags as tagwords
from .build import _check_array_no_scan, _raise_if_nonfinite
from .device_arrays import (_check_device_array, _device_corrected, _DeviceRowsView, _dtype_name, _ids_to_host,
                            _is_device_array, _OnTorchStream, _rows_to_host, _shape_of)
from .metrics import (_METRICS, _NEGATIVE_HELLINGER, _linear_map_of, _metric_record, _no_exact_for_proxy,
                      _raise_if_negative_host)


def _exact_linear_rows(metric, m, metric_kwds, data, queries, device):
    """``exact_knn`` of a metric with a linear map or a row map: ``(data, queries)`` transformed by the device (float32; tensors
    stay tensors), on which the search is the base metric's (euclidean; spearmanr: correlation).  The shift is the one an index of
    ``data`` would fix; distances do not depend on it."""
    if _is_device_array(data):
        data, dtype, ordinal = _check_device_array(data, device)
        lin = _linear_map_of(metric, m, metric_kwds, data.shape[1])
        if lin is None:
            return data, queries
        torch = device_arrays._torch()
        with torch.cuda.device(ordinal):
            if m.row_map is not None:
                device_arrays._assert_all_finite(data)
            dl = device_arrays._device_map(row_map.with_shift(lin, _DeviceRowsView(data)), data.device, ordinal)
            stream = torch.cuda.current_stream(ordinal).cuda_stream
            if queries is not None:
                if _is_device_array(queries):
                    queries, q_dtype, _ = _check_device_array(queries, what="queries")
                    queries = queries.to(data.device)
                else:
                    queries, q_dtype = torch.from_numpy(_check_array_no_scan(queries)).to(data.device), _capi.NND_DTYPE_FLOAT32
                if queries.shape[1] != data.shape[1]:
                    raise ValueError("queries must have shape (n_queries, %d)" % data.shape[1])
                if m.row_map is not None:
                    device_arrays._assert_all_finite(queries)
                queries = dl.rows(queries, q_dtype, stream)
            return dl.rows(data, dtype, stream), queries
    data = _check_array_no_scan(data)
    lin = _linear_map_of(metric, m, metric_kwds, data.shape[1])
    if lin is None:
        return data, queries
    if m.row_map is not None:  # (mapped rows are finite whatever the input holds: the scan comes first)
        device_arrays._assert_all_finite(data)
    lin = row_map.with_shift(lin, data)
    if queries is not None:
        queries = _check_array_no_scan(_rows_to_host(queries))
        if queries.shape[1] != data.shape[1]:
            raise ValueError("queries must have shape (n_queries, %d)" % data.shape[1])
        if m.row_map is not None:
            device_arrays._assert_all_finite(queries)
        queries = row_map.rows_host(lin, queries, device=device)
    return row_map.rows_host(lin, data, device=device), queries


def _exact_knn_sparse(data, queries, k, metric, m, rows, device, return_stats, metric_kwds, words=None):
    """``exact_knn`` with a ``scipy.sparse`` ``data`` and / or ``queries``: the metric rule of sparse input, then whatever is
    sparse is uploaded as CSR and made dense on the device (sparse_input.py), host ``data`` given with sparse queries is
    uploaded, and the device route searches.  Scipy or numpy ``data`` gets numpy answers with the host's correction (the bits of
    the host route); a tensor ``data`` gets tensors."""
    sparse_input.check_sparse_metric(metric)
    if m.linear:  # minkowski: metric_kwds under the dense rule (p = 2 alone), then the euclidean path itself
        _linear_map_of(metric, m, metric_kwds, data.shape[1])
        metric, m = "euclidean", _METRICS["euclidean"]
    host_answers = not _is_device_array(data)
    if queries is not None and tuple(_shape_of(queries))[1:] != (data.shape[1],):
        raise ValueError("queries must have shape (n_queries, %d)" % data.shape[1])
    if sparse_input.is_sparse(data):
        data = sparse_input.dense_rows_on_device(sparse_input.canonical_csr(data), device, check_fit=True)
    elif host_answers:
        torch = device_arrays._torch()
        data = torch.from_numpy(_check_array_no_scan(data)).to(torch.device("cuda", int(device)))
    ordinal = getattr(data.device, "index", None) or 0
    if sparse_input.is_sparse(queries):
        queries = sparse_input.query_rows(queries, data.shape[1], ordinal, what="queries")
    return _exact_knn_device(data, queries, k, metric, m, rows, ordinal, return_stats, host_answers=host_answers, words=words)


def _check_tag_arguments(data, queries, rows, row_tags, query_tags, device):
    """``(tags, masks)`` of a masked ``exact_knn`` call, each as ``tags.check_words`` returns it, or None without them."""
    if row_tags is None and query_tags is None:
        return None
    if row_tags is None or query_tags is None:
        raise ValueError("exact_knn takes row_tags and query_tags together: a predicate needs both sides")
    n = int(_shape_of(data)[0])
    if _is_device_array(data):
        device = getattr(data.device, "index", None) or 0
    m = int(_shape_of(queries)[0]) if queries is not None else (n if rows is None else int(_shape_of(rows)[0]))
    return (tagwords.check_words(row_tags, n, device, "row_tags", "row"),
            tagwords.check_words(query_tags, m, device, "query_tags", "query"))


def _unfilled_to_inf(idx, dist):
    """The places no allowed row fills hold (-1, inf) whatever the metric's correction made of inf."""
    if _is_device_array(dist):
        return dist.masked_fill(idx < 0, float("inf"))
    dist = np.array(dist, copy=True)
    dist[idx < 0] = np.inf
    return dist


def exact_knn(data, queries=None, k=10, metric="euclidean", rows=None, device=0, return_stats=False, metric_kwds=None,
              _host_answers=False, row_tags=None, query_tags=None, _record=None):
    """Exact ``k`` nearest neighbours by brute force on the GPU (csrc/exact.hip): of every row of ``data`` (self included), of the
    rows ``rows`` of it, or of the external ``queries``.  Returns ``(indices int32 (m, k), distances float32-precision (m, k))``
    in the metric's own space (the correction ``NNDescent.neighbor_graph`` applies), rows ascending, ties to the smaller id;
    with ``return_stats`` also the call's statistics (rows that needed the float64 tier, kernel times).  The metrics and the
    input rules are the class's: dot rows and queries are L2-normalised, hellinger takes no negative entry, NaN / inf raise
    the reference's error.  ``k`` is at most 256 and at most the number of rows.

    ``data`` may be a device array (a 2-D ``torch.Tensor`` on a HIP device, float32 / float16 / bfloat16 / float64): the search
    then runs on the tensor where it is, on torch's current stream, and the answers are tensors on that device -- int32 ids, and
    the distances corrected on the device (float32 or float64, as ``NNDescent.neighbor_graph`` returns them for the metric; dot
    normalises on the device, within rounding of the host's rows).  ``queries`` on the other side are moved to where ``data`` is;
    ``rows`` may be a host array or a tensor (the ids are range-checked on the host).

    ``metric_kwds``: the arguments of seuclidean / wminkowski (p = 2) / mahalanobis / minkowski (p = 2), read positionally as by
    ``NNDescent``; every other metric ignores it.  For these metrics the answers are exact in this sense: (float64 distance, id)
    on the float32 transformed rows -- the rows ``A (x - c)`` the device computes once (csrc/linear.hip), on which the search is
    the euclidean one.  spearmanr and haversine (2-D ``(lat, lon)`` rows, radians) likewise: exact on the float32 rows their row
    map makes (csrc/rowmap.hip) -- rank rows, which are exact themselves, and the points of the unit sphere.  ``_record``
    (``NNDescent``'s filtered paths): a derived metric's record for rows and queries that are mapped already; ``metric`` then
    names the base metric.

    ``data`` and / or ``queries`` may be ``scipy.sparse`` matrices, for the metrics ``NNDescent`` takes with sparse input: they
    are made dense on the device (sparse_input.py) and the device route searches; the answers are numpy arrays, those of the dense
    call bit for bit, unless ``data`` is a tensor.

    ``row_tags`` and ``query_tags`` (both or neither; DESIGN.md "Per-query filters"): 64 tag bits per row of ``data`` and a mask
    word per query -- with ``queries=None`` per row searched, the masks belonging to the rows themselves -- each a 1-D numpy
    ``uint64`` / ``int64`` array or an ``int64`` tensor on the device.  Row r is a candidate of query i iff
    ``row_tags[r] & query_tags[i] != 0``, and the answer is exact by (float64 distance, id) among those rows: the ground truth for
    recall under a predicate.  Places that fewer than ``k`` such rows leave open hold (-1, inf)."""
    if queries is not None and rows is not None:
        raise ValueError("exact_knn takes `queries` (external points) or `rows` (ids of data rows), not both")
    words = _check_tag_arguments(data, queries, rows, row_tags, query_tags, device)
    k = int(k)
    if k > 256:
        raise NotImplementedError("pynndescent_amd.exact_knn keeps at most k <= 256 neighbours per row (got k = %d)" % k)
    m = _metric_record(metric) if _record is None else _record
    _no_exact_for_proxy(metric, m, "exact_knn")
    if sparse_input.is_sparse(data) or sparse_input.is_sparse(queries):
        return _exact_knn_sparse(data, queries, k, metric, m, rows, device, return_stats, metric_kwds, words)
    if m.linear:  # (metric_kwds is validated in there, before any device work)
        data, queries = _exact_linear_rows(metric, m, metric_kwds, data, queries, device)
        metric, m = "euclidean", _METRICS["euclidean"]
    elif m.row_map is not None and _record is None:  # the base metric's kernels, the derived metric's own correction
        data, queries = _exact_linear_rows(metric, m, metric_kwds, data, queries, device)
        metric = m.row_map.base
    if _is_device_array(data):
        return _exact_knn_device(data, queries, k, metric, m, rows, device, return_stats, host_answers=_host_answers, words=words)
    queries, rows = _rows_to_host(queries), _ids_to_host(rows)  # (the results live where the data lives)
    data = _check_array_no_scan(data)
    n = data.shape[0]
    if k < 1 or k > n:
        raise ValueError("k must be in 1 .. n = %d (got %d)" % (n, k))
    _raise_if_negative_host(data, m)
    if queries is not None:
        from sklearn.utils import assert_all_finite

        queries = _check_array_no_scan(queries)
        if queries.shape[1] != data.shape[1]:
            raise ValueError("queries must have shape (n_queries, %d)" % data.shape[1])
        assert_all_finite(queries)
        _raise_if_negative_host(queries, m)
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        if rows.size and (rows.min() < 0 or rows.max() >= n):
            raise ValueError("rows must be ids in [0, %d)" % n)
    if m.normalize:  # pynndescent_.py:1101-1102, 2316-2318
        from sklearn.preprocessing import normalize

        data = normalize(data, norm="l2", copy=True)
        if queries is not None:
            queries = normalize(queries, norm="l2", copy=True)
    # an auxiliary handle: the rows and their prepared copy, no k-lists
    builder = _capi.Builder(n, data.shape[1], m.code, k, 0, 60, 200, min(60, k), 1, 0.001, [1, 2, 3], [4, 5, 6], device=device,
                            flags=_capi.NND_FLAG_NO_GRAPH)
    try:
        builder.set_data_host(data)
        _raise_if_nonfinite(builder, data)
        tm = {} if words is None else {"tags": tagwords.to_host(*words[0]), "masks": tagwords.to_host(*words[1])}
        if queries is not None:
            idx, dist, stats = builder.exact_knn_queries(queries, k, **tm)
        else:
            idx, dist, stats = builder.exact_knn(rows, k, **tm)
    finally:
        builder.close()
    dist = m.correction(dist)
    if words is not None:
        dist = _unfilled_to_inf(idx, dist)
    return (idx, dist, stats) if return_stats else (idx, dist)


def _exact_knn_device(data, queries, k, metric, m, rows, device, return_stats, host_answers=False, words=None):
    """``exact_knn`` for a device array ``data`` (``k``, the metric and queries-or-rows are checked already): an auxiliary handle
    bound to the tensor on torch's current stream, the device entries of csrc/exact.hip, the answers corrected on the device.
    ``rows``: a host array or a tensor of ids (range-checked on the host), or an int32 tensor on the data's device that the
    caller has checked (``NNDescent._recall_device``).  What crosses the bus: the row ids, host queries, and scalars.
    ``host_answers``: the ids and the kernels' distances are brought to the host and corrected there, as the host route does (the
    same bits; the device's correction agrees with numpy's within rounding only) -- for callers whose input came from the host."""
    data, dtype, ordinal = _check_device_array(data, device)
    n, dim = int(data.shape[0]), int(data.shape[1])
    if k < 1 or k > n:
        raise ValueError("k must be in 1 .. n = %d (got %d)" % (n, k))
    torch = device_arrays._torch()
    with torch.cuda.device(ordinal):
        q = q_dtype = None
        if queries is not None:
            if _is_device_array(queries):
                q, q_dtype, q_ordinal = _check_device_array(queries, what="queries")
                if q_ordinal != ordinal:
                    q = q.to(data.device)
            else:
                q, q_dtype = torch.from_numpy(_check_array_no_scan(queries)).to(data.device), _capi.NND_DTYPE_FLOAT32
            if q.shape[1] != dim:
                raise ValueError("queries must have shape (n_queries, %d)" % dim)
            if q.shape[0] and not bool(torch.isfinite(q).all().item()):  # one scalar; only the error path brings the queries down
                from sklearn.utils import assert_all_finite

                assert_all_finite(_rows_to_host(q))
            if m.nonnegative and q.shape[0] and bool((q.min() < 0).item()):
                raise ValueError(_NEGATIVE_HELLINGER)
        rows_dev = None
        if rows is not None:
            if _is_device_array(rows) and _dtype_name(rows) == "int32" and len(rows.shape) == 1 and rows.device == data.device:
                rows_dev = rows
            else:
                rows = np.ascontiguousarray(_ids_to_host(rows), dtype=np.int64).reshape(-1)
                if rows.size and (rows.min() < 0 or rows.max() >= n):
                    raise ValueError("rows must be ids in [0, %d)" % n)
                rows_dev = torch.from_numpy(rows.astype(np.int32)).to(data.device)
        n_out = int(q.shape[0]) if q is not None else (n if rows_dev is None else int(rows_dev.shape[0]))
        tm = {}
        if words is not None:  # (host words go up here, before the side stream is made)
            tags_dev, masks_dev = tagwords.to_device(*words[0], data.device), tagwords.to_device(*words[1], data.device)
            tm = {"tags_ptr": tags_dev.data_ptr(), "masks_ptr": masks_dev.data_ptr() if n_out else 0}
        idx = torch.empty((n_out, k), dtype=torch.int32, device=data.device)
        dist = torch.empty((n_out, k), dtype=torch.float32, device=data.device)
        stream = _OnTorchStream(torch, ordinal)  # (made after the uploads: a side stream waits for them)
        # an auxiliary handle: the rows and their prepared copy, no k-lists
        builder = _capi.Builder(n, dim, m.code, k, 0, 60, 200, min(60, k), 1, 0.001, [1, 2, 3], [4, 5, 6], device=ordinal,
                                flags=_capi.NND_FLAG_NO_GRAPH)
        try:
            builder.set_stream(stream.ptr)
            builder.set_data_device_typed(data.data_ptr(), dtype, keepalive=data)  # (dot: normalised there, as the class does)
            _raise_if_nonfinite(builder, lambda: _rows_to_host(data))
            if m.nonnegative and builder.data_negative():
                raise ValueError(_NEGATIVE_HELLINGER)
            if n_out == 0:  # (nothing asked for: an empty tensor has no address to hand over)
                stats = dict(_capi.NNDExactStats().as_dict(), slices=0)
            elif q is not None:
                stats = builder.exact_knn_device(k, idx.data_ptr(), dist.data_ptr(), q_ptr=q.data_ptr(), q_dtype=q_dtype, n_q=n_out, **tm)
            else:
                stats = builder.exact_knn_device(k, idx.data_ptr(), dist.data_ptr(), rows_ptr=0 if rows_dev is None else rows_dev.data_ptr(),
                                                 n_rows=n_out, **tm)
        finally:
            builder.close()
            stream.done()
        if host_answers:
            idx, dist = np.ascontiguousarray(idx.cpu().numpy()), m.correction(np.ascontiguousarray(dist.cpu().numpy()))
        else:
            dist = _device_corrected(torch, dist, m, ordinal)
        if words is not None:
            dist = _unfilled_to_inf(idx, dist)
    return (idx, dist, stats) if return_stats else (idx, dist)
