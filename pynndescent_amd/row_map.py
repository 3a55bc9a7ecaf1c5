"""The derived metrics: a name that means "this map of every row, then that metric of the table" -- ``spearmanr`` and
``haversine``.

    spearmanr(x, y) = correlation(rank(x), rank(y))           rank: average ranks, ties share the mean of their places
    haversine(x, y) = 2 arcsin(min(1, |P(x) - P(y)| / 2))      P(lat, lon) = (cos lat cos lon, cos lat sin lon, sin lat)

(reference distances.py:1430-1480 and 503-521; ``sin^2(dlat / 2) + cos lat1 cos lat2 sin^2(dlon / 2) = |P(x) - P(y)|^2 / 4``.)
A row's map depends on that row alone, so the device maps every row once (csrc/rowmap.hip) and everything behind it runs the
base metric's path unchanged: correlation on rank rows, euclidean on the 3-D rows ``P(x) - c``.  The ranks are exact; the
sphere rows carry a shift ``c`` near the data, as the linear maps do, which euclidean distance does not see.

The names live in a registry of their own, ``ROW_MAP_METRICS``, outside ``metrics._METRIC_TABLE``: the table is the list of
metrics with a distance formula in the kernels (or a linear map in front of one), and ``nn_descent(dist=...)``, the uint8 proxy
and the sharded build are defined over it; a derived name takes part in none of those.  ``metrics._metric_record`` consults the
table first, then this registry, and builds the record from the base metric's.

Host only, numpy only (the constants of ``_capi``; the library is loaded by the calls that map rows).
"""
from typing import Callable, NamedTuple, Optional

import numpy as np

from . import _capi, linear_map


def correct_haversine(s):
    """The angle of the squared chord ``s`` of two points of the unit sphere: ``2 arcsin(min(1, sqrt(s) / 2))``, float64 (the
    reference's haversine returns float64 as well); an unfilled entry (+inf) gives pi."""
    s = np.asarray(s, dtype=np.float64)
    return 2.0 * np.arcsin(np.minimum(1.0, np.sqrt(s) / 2.0))


class RowMapMetric(NamedTuple):
    """One derived metric."""
    name: str
    kind: int  # the map (include/pynnd_amd.h NND_ROWMAP_*)
    base: str  # the metric of the table whose kernels run on the mapped rows
    correction: Callable  # kernel distance of the base metric -> this metric's own, always a new array
    device_kind: int  # the same correction on a device tensor (NND_CORRECT_*)
    in_dim: Optional[int]  # the only input width the metric is defined for (None: any)
    out_dim: Optional[int]  # the width of the mapped rows (None: the input's)


ROW_MAP_METRICS = {
    "spearmanr": RowMapMetric("spearmanr", _capi.NND_ROWMAP_RANK, "correlation", _capi.host_copy, _capi.NND_CORRECT_COPY, None, None),
    "haversine": RowMapMetric("haversine", _capi.NND_ROWMAP_SPHERE, "euclidean", correct_haversine, _capi.NND_CORRECT_HAVERSINE, 2, 3),
}

RANK_MAX_DIM = _capi.ROWMAP_RANK_MAX_DIM  # the widest row the device ranks; 2^23 and beyond could not be exact in float32


class RowMap(NamedTuple):
    """What an index keeps (and pickles) of its metric's row map, where a linear metric keeps its ``LinearMap``."""
    kind: int  # NND_ROWMAP_*
    shift: Optional[np.ndarray]  # the sphere: (3,) float32, fixed when the index is first built; the ranks: None


def row_map_of(spec, dim):
    """The ``RowMap`` (without its shift) of the derived metric ``spec`` for rows of ``dim`` columns.  ValueError: a width the
    metric is not defined for (the reference's wording).  NotImplementedError: more columns than the device ranks."""
    dim = int(dim)
    if spec.in_dim is not None and dim != spec.in_dim:
        raise ValueError("%s is only defined for %d dimensional graph_data" % (spec.name, spec.in_dim))
    if spec.kind == _capi.NND_ROWMAP_RANK and dim > RANK_MAX_DIM:
        raise NotImplementedError("pynndescent_amd ranks rows of at most %d columns for metric %r (got %d); use pynndescent.NNDescent"
                                  % (RANK_MAX_DIM, spec.name, dim))
    return RowMap(spec.kind, None)


def sphere_points(rows):
    """``P(lat, lon)`` of (n, 2) rows, float64: the host model of the sphere map before its shift and its rounding."""
    rows = np.asarray(rows, dtype=np.float64)
    cl = np.cos(rows[:, 0])
    return np.stack([cl * np.cos(rows[:, 1]), cl * np.sin(rows[:, 1]), np.sin(rows[:, 0])], axis=1)


def with_shift(m, rows_view):
    """``m`` (a ``LinearMap`` or a ``RowMap``) with the shift an index of the rows ``rows_view`` fixes: a linear map's column
    mean (``linear_map.shift_of``); the sphere's float32 of the float64 mean of ``P`` over the same strided sample; none for the
    ranks.  ``rows_view[ids]`` gives the sampled rows as float32 -- a host array, or a gathering view of a device tensor."""
    if isinstance(m, linear_map.LinearMap):
        return m._replace(shift=linear_map.shift_of(rows_view))
    if m.kind != _capi.NND_ROWMAP_SPHERE:
        return m
    sample = np.asarray(rows_view[linear_map.shift_rows(rows_view.shape[0])], dtype=np.float32)
    return m._replace(shift=sphere_points(sample).mean(axis=0).astype(np.float32))


def rows_host(m, x, device=0):
    """The host rows ``x`` through ``m`` (a ``LinearMap`` or a ``RowMap`` with its shift) by the device kernel: a new float32 array."""
    if isinstance(m, linear_map.LinearMap):
        return _capi.linear_rows_host(m.kind, m.a, m.shift, x, device=device)
    return _capi.map_rows_host(m.kind, m.shift, x, device=device)
