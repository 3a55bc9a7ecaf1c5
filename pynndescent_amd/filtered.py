"""Filtered queries: ``NNDescent.query(..., filter=..., filter_mode=...)`` (DESIGN.md "Filtered queries").

One allow set for all queries of a call, in the ORIGINAL row numbering: a 1-D boolean mask of n rows or a 1-D integer array of
row ids, numpy or a tensor on the index's device.  Two paths: ``walk`` -- the graph walk with the rule "a vertex enters the
result list only if it is allowed" (csrc/query.hip, k_query's Q_FILT_ALLOW instances; the allow bitset is built on the device by
``nnd_searcher_set_filter*``), and ``exact`` -- the allowed rows gathered into a compact copy that ``exact_knn`` searches.
``auto`` takes the exact path for at most ``FILTER_EXACT_MAX_ROWS`` allowed rows.

Per-query filters (DESIGN.md "Per-query filters"): ``index.set_row_tags(tags)`` and ``query(..., query_tags=masks)`` -- 64 tag bits
per row, a mask word per query, row r allowed for query i iff ``tags[r] & masks[i] != 0``.  ``walk``: k_query's Q_FILT_TAGS instances
(csrc/query.hip) on the searcher's own copy of the tag words; ``exact``: the masked scan of csrc/exact.hip over all rows;
``auto``: per query, by the number of rows its mask allows (``tag_auto_paths``).
"""
from collections import namedtuple

import numpy as np

from . import _capi, device_arrays, row_map
from .device_arrays import _dtype_name, _is_device_array, _shape_of
from .exact import exact_knn
from .metrics import _metric_of

FILTER_MODES = ("auto", "walk", "exact")
# ``auto``: the exact path answers a call with at most this many allowed rows.  The brute-force search costs (allowed rows x
# queries) distances and gets cheaper with every row filtered out, the walk does 1 / selectivity times the unfiltered work, so
# they cross: at 1 M x 128, k = 10, 10 000 queries between 49 690 allowed rows (walk 23.35 ms, exact 10.77 ms) and 99 546
# (12.32 / 15.60 ms), by interpolation at about 85 000 (profiles/filtered_query_1m.txt, tools/ab/filtered_query_timing.py).
FILTER_EXACT_MAX_ROWS = 85000

# Per-query filters, ``auto``: a query whose mask allows at most this many rows is answered by the masked exact scan.  That scan
# streams ALL rows past every query block whatever the mask allows (66 .. 75 ms at 1 M x 128, k = 10, 10 000 queries), so its
# crossing with the walk lies lower than the compact copy's: between 99 921 allowed rows (walk 13.06 ms, exact 75.15 ms) and 9 957
# (506.43 / 71.13 ms); the walk's time over that decade goes as rows^-1.59, which puts the crossing at about 34 000
# (profiles/tag_filter_1m.txt, tools/ab/tag_filter_timing.py).
TAG_EXACT_MAX_ROWS = 34000
# ``auto`` counts the allowed rows of at most this many distinct masks per call (one pass over the tag words for all of them);
# a call with more distinct masks walks every query.  A bound on the counting work: a condition, not a measurement.
TAG_COUNT_MAX_MASKS = 1024

# kind "mask" (bool, n) or "ids" (int64); ``values`` numpy or tensor; ``n_allowed`` distinct allowed rows
_Filter = namedtuple("_Filter", ["kind", "values", "on_device", "n_allowed"])


def check_filter(filter, n, device):
    """``filter`` as a ``_Filter``, or ``ValueError``: not 1-D, a float dtype, a mask of the wrong length, an id outside
    0 .. n - 1, a tensor on another device than the index."""
    if _is_device_array(filter):
        if (getattr(filter.device, "index", None) or 0) != int(device):
            raise ValueError("filter is on device %d, the index on device %d" % (filter.device.index or 0, int(device)))
        torch = device_arrays._torch()
        name = _dtype_name(filter)
        if filter.dim() != 1:
            raise ValueError("filter must be 1-D (got %d dimensions)" % filter.dim())
        if name == "bool":
            if filter.shape[0] != n:
                raise ValueError("a boolean filter has one entry per row (%d), got %d" % (n, filter.shape[0]))
            return _Filter("mask", filter.contiguous(), True, int(torch.count_nonzero(filter).item()))
        if name not in ("int8", "int16", "int32", "int64", "uint8"):
            raise ValueError("filter must be a boolean mask or an integer array of row ids (got dtype %s)" % name)
        ids = filter.to(torch.int64).contiguous()
        if ids.numel() and bool(((ids < 0) | (ids >= n)).any().item()):
            raise ValueError("filter holds a row id outside 0 .. %d" % (n - 1))
        return _Filter("ids", ids, True, int(torch.unique(ids).numel()))
    a = np.asarray(filter)
    if a.ndim != 1:
        raise ValueError("filter must be 1-D (got %d dimensions)" % a.ndim)
    if a.dtype == np.bool_:
        if a.shape[0] != n:
            raise ValueError("a boolean filter has one entry per row (%d), got %d" % (n, a.shape[0]))
        return _Filter("mask", np.ascontiguousarray(a), False, int(np.count_nonzero(a)))
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("filter must be a boolean mask or an integer array of row ids (got dtype %s)" % a.dtype)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= n):
        raise ValueError("filter holds a row id outside 0 .. %d" % (n - 1))
    ids = np.ascontiguousarray(a, np.int64)
    return _Filter("ids", ids, False, int(np.unique(ids).size))


def choose_mode(filter_mode, n_allowed, metric):
    """The path a call takes: "empty" (no allowed row), "exact" or "walk"."""
    if n_allowed == 0:
        return "empty"
    if filter_mode == "auto":
        return "exact" if n_allowed <= FILTER_EXACT_MAX_ROWS and not _metric_of(metric).proxy else "walk"
    return filter_mode


def empty_answer(query_data, k, dist_dtype=np.float32):
    """(-1, inf) for every query, where the queries live."""
    nq = int(_shape_of(query_data)[0])
    if _is_device_array(query_data):
        torch = device_arrays._torch()
        return (torch.full((nq, k), -1, dtype=torch.int32, device=query_data.device),
                torch.full((nq, k), float("inf"), dtype=torch.float32, device=query_data.device))
    return np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, dist_dtype)


def set_walk_filter(index, f):
    """The searcher's allow bitset from ``f`` (the filter stays where it is: a host filter goes up through the host entry, a
    tensor is read on torch's current stream), gathered through the searcher's row order.  Returns the allowed-row count."""
    searcher = index._searcher
    if not f.on_device:
        return searcher.set_filter(f.values, index._vertex_order)
    torch = device_arrays._torch()
    ordinal = int(index.device)
    with torch.cuda.device(ordinal):
        order = getattr(searcher, "vertex_order_device", None)
        if order is None:
            order = torch.from_numpy(np.ascontiguousarray(index._vertex_order, dtype=np.int32)).to(f.values.device)
            searcher.vertex_order_device = order
        kind = _capi.NND_FILTER_MASK if f.kind == "mask" else _capi.NND_FILTER_IDS
        return searcher.set_filter_device(f.values.data_ptr() if f.values.numel() else 0, f.values.numel(), kind, order.data_ptr(),
                                          torch.cuda.current_stream(ordinal).cuda_stream)


def _allowed_ids(f):
    """The allowed rows' ids, ascending and distinct, where the filter lives."""
    if f.on_device:
        torch = device_arrays._torch()
        return torch.nonzero(f.values).reshape(-1) if f.kind == "mask" else torch.unique(f.values)
    return np.flatnonzero(f.values).astype(np.int64) if f.kind == "mask" else np.unique(f.values)


def query_exact(index, query_data, k, f, host_answers=False):
    """``filter_mode="exact"``: the allowed rows of the rows the index works on, gathered in ascending id order into a compact
    copy; ``exact_knn`` answers the queries on it -- by (float64 distance, id), the compact id order being the original one --
    and the ids are mapped back.  Fewer allowed rows than ``k`` leave (-1, inf).  Results live where ``query_data`` lives;
    ``host_answers``: the queries are a tensor made from a host batch (a sparse one), and the answers are numpy arrays corrected
    on the host, the bits of the host route."""
    d = index.__dict__
    on_device = _is_device_array(query_data)
    ids = _allowed_ids(f)

    def ids_host():
        return ids.cpu().numpy() if f.on_device else ids

    def ids_on(where):
        return ids.to(where) if f.on_device else device_arrays._torch().from_numpy(ids).to(where)

    lin = d.get("_linear_map")
    if "_device_data" in d:  # the caller's tensor (a linear map: its transformed rows), in the original order
        compact = d["_device_data"][ids_on(d["_device_data"].device)]
    else:  # the host rows are in the searcher's order since prepare(): original row r is row position[r]
        order = np.asarray(index._vertex_order)
        position = np.empty(order.shape[0], np.int64)
        position[order] = np.arange(order.shape[0])
        if d.get("_is_sparse"):  # (a sparse index without its tensor, e.g. unpickled: the allowed rows alone are made dense)
            compact = np.ascontiguousarray(index._raw_data[position[ids_host()]].toarray(), dtype=np.float32)
        else:
            compact = np.ascontiguousarray(index._work_rows()[position[ids_host()]])
        if on_device:
            compact = device_arrays._torch().from_numpy(compact).to(query_data.device)
    if lin is not None:  # the queries through the index's own (A, c); the search on the transformed rows is euclidean
        if on_device:
            torch = device_arrays._torch()
            q, dtype, ordinal = device_arrays._check_device_array(query_data, what="query_data")
            with torch.cuda.device(ordinal):
                query_data = index._linear_on_device(q.device).rows(q, dtype, torch.cuda.current_stream(ordinal).cuda_stream)
        else:
            query_data = row_map.rows_host(lin, np.asarray(query_data).astype(np.float32, order="C"),
                                                device=index.device)
    kk = min(int(k), int(f.n_allowed))
    idx, dist = exact_knn(compact, queries=query_data, k=kk, metric=index._kernel_metric(), device=index.device,
                          _host_answers=host_answers, _record=index._mapped_record())
    if _is_device_array(idx):
        torch = device_arrays._torch()
        idx = ids_on(idx.device)[idx.long()].to(torch.int32)
        if kk < k:
            pad_i = torch.full((idx.shape[0], k - kk), -1, dtype=idx.dtype, device=idx.device)
            pad_d = torch.full((idx.shape[0], k - kk), float("inf"), dtype=dist.dtype, device=dist.device)
            idx, dist = torch.cat([idx, pad_i], 1), torch.cat([dist, pad_d], 1)
        if not on_device:
            idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        return idx, dist
    idx = ids_host()[idx].astype(np.int32)
    if kk < k:
        idx = np.concatenate([idx, np.full((idx.shape[0], k - kk), -1, np.int32)], 1)
        dist = np.concatenate([dist, np.full((dist.shape[0], k - kk), np.inf, dist.dtype)], 1)
    return idx, dist


# ------------------------------------------------------------------------------------------------ per-query filters
def tag_mask_paths(distinct, counts, exact_ok=True):
    """The ``auto`` rule per DISTINCT mask: "empty" (the mask is 0, or it allows no row), "exact" (it allows at most
    ``TAG_EXACT_MAX_ROWS`` rows and the metric has an exact search) or "walk".  ``counts`` (allowed rows per distinct mask) is None
    when the call has more than ``TAG_COUNT_MAX_MASKS`` distinct masks: then nothing was counted and every non-zero mask walks."""
    distinct = np.asarray(distinct).view(np.uint64)
    paths = np.full(distinct.shape[0], "walk", dtype=object)
    paths[distinct == 0] = "empty"
    if counts is not None:
        counts = np.asarray(counts, np.int64)
        paths[counts == 0] = "empty"
        if exact_ok:
            paths[(counts > 0) & (counts <= TAG_EXACT_MAX_ROWS) & (distinct != 0)] = "exact"
    return paths


def tag_counts_taken(n_distinct):
    """Does ``auto`` count the allowed rows of a call with ``n_distinct`` distinct masks?"""
    return int(n_distinct) <= TAG_COUNT_MAX_MASKS


def tag_auto_paths(inverse, distinct, counts, exact_ok=True):
    """The ``auto`` rule per QUERY: ``(walk, exact, empty)``, the positions in the batch of the queries each path answers.
    ``distinct``: the distinct masks of the call; ``inverse``: for every query the position of its mask in ``distinct``;
    ``counts``: the allowed rows per distinct mask, or None if they were not taken (``tag_counts_taken``)."""
    if counts is not None and not tag_counts_taken(len(distinct)):
        counts = None
    per_query = tag_mask_paths(distinct, counts, exact_ok)[np.asarray(inverse, np.int64)]
    return tuple(np.flatnonzero(per_query == name) for name in ("walk", "exact", "empty"))


def ensure_searcher_tags(index):
    """The searcher's copy of the index's tag words (its own numbering), built when tags are first used: a host array goes up
    through the host entry, a tensor is gathered where it is.  The copy lives until the tags change or the searcher is rebuilt."""
    searcher = index._searcher
    if getattr(searcher, "tags_set", False):
        return
    values = index._row_tags
    if not _is_device_array(values):
        searcher.set_tags(values, index._vertex_order)
    else:
        torch = device_arrays._torch()
        ordinal = int(index.device)
        with torch.cuda.device(ordinal):
            searcher.set_tags_device(values.data_ptr(), _searcher_order(index, values.device).data_ptr(),
                                     torch.cuda.current_stream(ordinal).cuda_stream)
    searcher.tags_set = True


def _searcher_order(index, where):
    """The searcher's row order as an int32 tensor (lives and dies with the searcher)."""
    order = getattr(index._searcher, "vertex_order_device", None)
    if order is None:
        order = device_arrays._torch().from_numpy(np.ascontiguousarray(index._vertex_order, dtype=np.int32)).to(where)
        index._searcher.vertex_order_device = order
    return order


def tag_counts(index, distinct):
    """Allowed rows per distinct mask (numpy uint64 ``distinct``), counted by the device in one pass over the searcher's tag words."""
    ensure_searcher_tags(index)
    return index._searcher.count_tags(distinct)


def rows_in_original_order(index, where=None):
    """Every row the index works on, in the ORIGINAL numbering, for the masked exact scan: the caller's tensor (a linear map: its
    transformed rows) where there is one, else a host copy un-permuted from the searcher's order (a sparse index without its
    tensor: made dense).  ``where``: a torch device the host copy is moved to."""
    d = index.__dict__
    if "_device_data" in d:
        return d["_device_data"]
    order = np.asarray(index._vertex_order)
    position = np.empty(order.shape[0], np.int64)
    position[order] = np.arange(order.shape[0])
    if d.get("_is_sparse"):
        rows = np.ascontiguousarray(index._raw_data[position].toarray(), dtype=np.float32)
    else:
        rows = np.ascontiguousarray(index._work_rows()[position])
    if where is not None:
        rows = device_arrays._torch().from_numpy(rows).to(where)
    return rows


def query_tagged_exact(index, query_data, k, masks, masks_on_device, host_answers=False):
    """``filter_mode="exact"`` of a tagged call: ``exact_knn`` with ``row_tags`` / ``query_tags`` over all rows in the original
    numbering -- exact by (float64 distance, id) among each query's allowed rows, (-1, inf) where they run out.  Results live where
    ``query_data`` lives (``host_answers``: see ``query_exact``)."""
    d = index.__dict__
    on_device = _is_device_array(query_data)
    rows = rows_in_original_order(index, query_data.device if on_device else None)
    lin = d.get("_linear_map")
    if lin is not None:  # the queries through the index's own (A, c); the search on the transformed rows is euclidean
        if on_device:
            torch = device_arrays._torch()
            q, dtype, ordinal = device_arrays._check_device_array(query_data, what="query_data")
            with torch.cuda.device(ordinal):
                query_data = index._linear_on_device(q.device).rows(q, dtype, torch.cuda.current_stream(ordinal).cuda_stream)
        else:
            query_data = row_map.rows_host(lin, np.asarray(query_data).astype(np.float32, order="C"),
                                                device=index.device)
    kk = min(int(k), int(_shape_of(rows)[0]))
    idx, dist = exact_knn(rows, queries=query_data, k=kk, metric=index._kernel_metric(), device=index.device, _host_answers=host_answers,
                          row_tags=index._row_tags, query_tags=masks, _record=index._mapped_record())
    if _is_device_array(idx):
        torch = device_arrays._torch()
        if kk < k:
            idx = torch.cat([idx, torch.full((idx.shape[0], k - kk), -1, dtype=idx.dtype, device=idx.device)], 1)
            dist = torch.cat([dist, torch.full((dist.shape[0], k - kk), float("inf"), dtype=dist.dtype, device=dist.device)], 1)
        if not on_device:
            idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        return idx, dist
    if kk < k:
        idx = np.concatenate([idx, np.full((idx.shape[0], k - kk), -1, np.int32)], 1)
        dist = np.concatenate([dist, np.full((dist.shape[0], k - kk), np.inf, dist.dtype)], 1)
    return idx, dist
