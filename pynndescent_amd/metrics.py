"""The metrics of the device path: one table of records, the corrections, and what each metric refuses.

Host only: numpy, the constants and host helpers of ``_capi`` (the library is not loaded here), ``linear_map`` and ``row_map``
(the derived metrics: a registry of their own, consulted after the table).
"""
from typing import Callable, NamedTuple

import numpy as np

from . import _capi, linear_map, row_map
from .row_map import correct_haversine  # noqa: F401


def correct_alternative_cosine(d):
    """1 - 2^-d (reference distances.py:704-711); float64 like the reference's ufunc."""
    return 1.0 - np.power(2.0, -np.asarray(d, dtype=np.float64))


def correct_alternative_inner_product(d):
    """-1/d, and 0 for FLT_MAX (reference distances.py:842-853); float64 like the reference's ufunc."""
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(d >= np.finfo(np.float32).max, 0.0, -1.0 / d)


def correct_alternative_hellinger(d):
    """sqrt(1 - 2^-d) (reference distances.py:1420-1426); float64 like the reference's ufunc."""
    return np.sqrt(1.0 - np.power(2.0, -np.asarray(d, dtype=np.float64)))


class _Metric(NamedTuple):
    """What the host needs to know about one metric of the device path."""
    code: int  # the kernels' metric (include/pynnd_amd.h NND_METRIC_*)
    correction: Callable  # kernel distance -> the metric's own, always a new array (pynndescent_.py:1271-1298)
    angular: bool = False  # angular trees in the reference (pynndescent_.py:1075-1086)
    uint8: bool = False  # has a uint8 proxy distance (distances.py:2250-2255 quantized_distances["uint8"])
    normalize: bool = False  # rows L2-normalised before anything else (pynndescent_.py:1101-1102)
    nonnegative: bool = False  # hellinger takes sqrt(x): a negative entry is an error here, NaN distances in the reference
    # a proxy with a true distance (distances.py:2190 proxy_distances): the graph is built and walked on the kernel distance, which
    # neighbor_graph hands out as it is; query() keeps proxy_beam_size * k candidates and the device reranks them by the true one
    proxy: bool = False
    device_kind: int = _capi.NND_CORRECT_COPY  # the same correction on a device tensor (include/pynnd_amd.h NND_CORRECT_*)
    # carries a fixed linear map from metric_kwds (linear_map.py): the device works on y = A (x - c), a transformed float32 copy
    # of the rows, with the kernels of ``code`` unchanged; _raw_data stays the caller's rows
    linear: bool = False
    # a function of the counts of indicator rows (x != 0): the device turns the rows into indicators itself (csrc/prep.hip), so
    # the host hands over the caller's rows as they are; one GPU, no uint8 proxy
    boolean: bool = False
    # a derived metric (row_map.py): its ``RowMapMetric`` -- the device works on a mapped float32 copy of the rows with the kernels
    # of the base metric's ``code``; _raw_data stays the caller's rows.  None for every record of the table
    row_map: object = None

    @property
    def mapped(self):
        """The device works on a transformed copy of the rows (a linear map or a row map), which the index keeps next to them."""
        return self.linear or self.row_map is not None

    @property
    def kernel_metric(self):
        """The name of the table whose kernels run on the mapped rows; None for a metric that is its own."""
        return "euclidean" if self.linear else (self.row_map.base if self.row_map is not None else None)


# every accepted name.  Corrections: numpy.sqrt, large float32 arrays through the library's threaded sqrtf (the same bits, the
# fresh pages touched in parallel); "sqeuclidean" and "correlation" are the kernels' own space, with no correction
# (pynndescent_.py:1271-1298) -- neighbor_graph still hands out a copy
_METRIC_TABLE = {
    "euclidean": _Metric(_capi.METRIC_CODES["euclidean"], _capi.host_sqrt, uint8=True, device_kind=_capi.NND_CORRECT_SQRT),
    "l2": _Metric(_capi.METRIC_CODES["l2"], _capi.host_sqrt, uint8=True, device_kind=_capi.NND_CORRECT_SQRT),
    "sqeuclidean": _Metric(_capi.METRIC_CODES["sqeuclidean"], _capi.host_copy),
    "cosine": _Metric(_capi.METRIC_CODES["cosine"], correct_alternative_cosine, angular=True, uint8=True,
                      device_kind=_capi.NND_CORRECT_ALT_COSINE),
    "dot": _Metric(_capi.METRIC_CODES["dot"], correct_alternative_cosine, angular=True, uint8=True, normalize=True,
                   device_kind=_capi.NND_CORRECT_ALT_COSINE),
    "inner_product": _Metric(_capi.METRIC_CODES["inner_product"], correct_alternative_inner_product,
                             device_kind=_capi.NND_CORRECT_ALT_INNER_PRODUCT),
    "correlation": _Metric(_capi.METRIC_CODES["correlation"], _capi.host_copy, angular=True),
    "hellinger": _Metric(_capi.METRIC_CODES["hellinger"], correct_alternative_hellinger, angular=True, nonnegative=True,
                         device_kind=_capi.NND_CORRECT_ALT_HELLINGER),
    "proxy_inner_product": _Metric(_capi.METRIC_CODES["proxy_inner_product"], _capi.host_copy, proxy=True),
    # euclidean distance after a fixed linear map of the rows (seuclidean, wminkowski with p = 2, mahalanobis; minkowski with
    # p = 2 has no map and is the euclidean path itself): code 0 and euclidean's correction on the transformed rows.  These names
    # take metric_kwds, the nine above ignore it
    **{name: _Metric(_capi.METRIC_CODES["euclidean"], _capi.host_sqrt, device_kind=_capi.NND_CORRECT_SQRT, linear=True)
       for name in linear_map.LINEAR_METRICS},
    # the boolean family (distances.py:259-552): functions of the Gram counts of indicator rows (DESIGN.md "Boolean metrics").
    # jaccard is built on alternative_jaccard and corrected by 1 - 2^-v (correct_alternative_jaccard, the same function as
    # cosine's correction); the other eight are handed out as they are.  ``angular`` is what the reference reports
    # (pynndescent_.py:1075-1086); the device splits indicator rows with euclidean trees.
    **{name: _Metric(code, correct_alternative_cosine if name == "jaccard" else _capi.host_copy,
                     angular=name in ("jaccard", "dice"), boolean=True,
                     device_kind=_capi.NND_CORRECT_ALT_COSINE if name == "jaccard" else _capi.NND_CORRECT_COPY)
       for name, code in _capi.BOOLEAN_METRIC_CODES.items()},
}
# views of the table by family (neither flag, ``linear``, ``boolean``), and of the plain records by one field
_METRICS = {name: m for name, m in _METRIC_TABLE.items() if not (m.linear or m.boolean)}
_LINEAR_METRICS = {name: m for name, m in _METRIC_TABLE.items() if m.linear}
_BOOLEAN_METRICS = {name: m for name, m in _METRIC_TABLE.items() if m.boolean}
_DISTANCE_CORRECTIONS = {name: m.correction for name, m in _METRICS.items()}
_ANGULAR_METRICS = frozenset(name for name, m in _METRICS.items() if m.angular)


def _derived_record(spec):
    """The record of a derived metric: the base record's kernels, the derived metric's own corrections, and no flag of the base
    metric's but its code -- ``angular`` is what the reference reports for these names (False, pynndescent_.py:1075-1086; the
    device splits the mapped rows as the base metric does)."""
    return _Metric(_METRIC_TABLE[spec.base].code, spec.correction, device_kind=spec.device_kind, row_map=spec)


_DERIVED_METRICS = {name: _derived_record(spec) for name, spec in row_map.ROW_MAP_METRICS.items()}


def _metric_of(name):
    """The record of a metric an index already has (its name was accepted by ``_metric_record``)."""
    return _METRIC_TABLE[name] if name in _METRIC_TABLE else _DERIVED_METRICS[name]


def _metric_record(metric, reference_fallback=True):
    """The row of ``_METRIC_TABLE``, or the record of a derived metric (``row_map.ROW_MAP_METRICS``).  A metric off the device path raises the reference's ValueError (pynndescent_.py:1292), or
    with ``reference_fallback`` NotImplementedError when the reference runs it (a callable, a name it knows): what
    ``make_index`` hands to ``pynndescent.NNDescent``."""
    if not callable(metric) and metric in _METRIC_TABLE:
        return _METRIC_TABLE[metric]
    if not callable(metric) and metric in _DERIVED_METRICS:
        return _DERIVED_METRICS[metric]
    if reference_fallback and (callable(metric) or metric in _KNOWN_REFERENCE_METRICS):
        raise NotImplementedError(
            "pynndescent_amd accelerates the dense euclidean / l2 / sqeuclidean / cosine / dot / inner_product / "
            "correlation / hellinger / proxy_inner_product / seuclidean / standardised_euclidean / mahalanobis build and the "
            "p = 2 form of minkowski / wminkowski / weighted_minkowski, and the boolean metrics jaccard / dice / sokalsneath / "
            "matching / rogerstanimoto / sokalmichener / kulsinski / russellrao / yule, and spearmanr / haversine only; "
            "use pynndescent.NNDescent for metric %r" % (metric,)
        )
    raise ValueError("Metric is neither callable, " + "nor a recognised string")


def _no_exact_for_proxy(metric, m, what):
    """The exact search certifies its answers with a float64 bound per formula; it has none for a proxy distance."""
    if m.proxy:
        raise NotImplementedError("pynndescent_amd.%s does not cover metric %r (a proxy distance: the float64 certificate of the "
                                  "exact search has no bound for it)" % (what, metric))


def _check_quantization(quantization, metric):
    """The quantization checks of the reference's ``prepare()`` (pynndescent_.py:2175-2263), host only."""
    if quantization is None:
        return
    if quantization == "uint8":
        if not _metric_record(metric, reference_fallback=False).uint8:
            raise ValueError(f"Not uint8 quantization version of {metric}")
        return
    if quantization in ("uint4", "binary"):
        raise NotImplementedError("quantized search with quantization=%r is out of scope for pynndescent_amd (\"uint8\" is "
                                  "supported); use index.to_reference()" % (quantization,))
    raise ValueError(f"Unrecognized quantization type {quantization}")


def _linear_map_of(metric, m, metric_kwds, dim):
    """The ``LinearMap`` (without its shift) of a metric that carries one, the ``RowMap`` of a derived metric; None for every other
    metric -- ``metric_kwds`` stays unread for those -- and for minkowski with p = 2.  Raises what
    ``linear_map.parse_metric_kwds`` / ``row_map.row_map_of`` raise."""
    if m.row_map is not None:
        return row_map.row_map_of(m.row_map, dim)
    return linear_map.parse_metric_kwds(metric, metric_kwds, dim) if m.linear else None


def _refuse_uint8_and_sharding(metric, m, quantization, n_devices):
    """What the metrics with a linear map or a row map, and the boolean metrics, do not combine with, reported before any device
    work."""
    if not (m.mapped or m.boolean):
        return
    if quantization == "uint8":
        _check_quantization(quantization, metric)  # the reference's ValueError("Not uint8 quantization version of ...")
    if int(n_devices) > 1:
        raise NotImplementedError("pynndescent_amd builds metric %r on one GPU (n_devices = %d): the row-sharded build has no "
                                  "%s; use n_devices=1" % (metric, int(n_devices), "linear map" if m.linear else ("row map" if m.row_map is not None else "boolean metrics")))


# the reference's functions of the kernels' own spaces (pynndescent_.py:1247-1260) -> the metric whose kernels they name;
# "alternative_jaccard": the kernel distance of the boolean family's jaccard
_ND_ALIASES = {"squared_euclidean": "sqeuclidean", "alternative_cosine": "cosine", "alternative_dot": "dot",
               "alternative_inner_product": "inner_product", "alternative_hellinger": "hellinger", "alternative_jaccard": "jaccard"}
# distance arguments nn_descent understands: name (or __name__ of the reference's function) -> (kernel metric, correction);
# the plain and the boolean metrics give true distances (the same kernels, corrected on return), the aliases none (a copy is no
# correction: nn_descent returns the finished arrays themselves); the names with a linear map are not nn_descent's
_ND_DISTS = {
    **{name: (m.code, None if m.correction is _capi.host_copy else m.correction)
       for name, m in _METRIC_TABLE.items() if not m.linear},
    **{alt: (_METRIC_TABLE[name].code, None) for alt, name in _ND_ALIASES.items()},
}

# hellinger takes sqrt(x): the reference computes NaN distances from a negative entry without a word; here it is an error
_NEGATIVE_HELLINGER = "the hellinger metric needs non-negative input: the data holds a negative entry"


def _raise_if_negative_host(data, m):
    if m.nonnegative and data.size and data.min() < 0:
        raise ValueError(_NEGATIVE_HELLINGER)


# string metrics the reference recognises (distances.py:2103-2168 named_distances keys, 2190-2239 proxy_distances keys) -- used only to
# decide between NotImplementedError (valid in the reference, not accelerated) and the reference's ValueError.
_KNOWN_REFERENCE_METRICS = frozenset(
    """euclidean l2 sqeuclidean manhattan taxicab l1 chebyshev linfinity linfty linf minkowski seuclidean
    standardised_euclidean wminkowski weighted_minkowski mahalanobis canberra cosine dot inner_product correlation
    haversine braycurtis spearmanr tsss true_angular hellinger kantorovich wasserstein wasserstein_1d
    wasserstein-1d kantorovich-1d kantorovich_1d circular_kantorovich circular_wasserstein sinkhorn jensen-shannon
    jensen_shannon symmetric-kl symmetric_kl symmetric_kullback_liebler hamming jaccard dice matching kulsinski
    rogerstanimoto russellrao sokalsneath sokalmichener yule bit_hamming bit_jaccard
    proxy_inner_product proxy_wasserstein_1d proxy_wasserstein-1d proxy_kantorovich proxy_wasserstein
    proxy_circular_kantorovich proxy_circular_wasserstein proxy_jensen_shannon proxy_jensen-shannon proxy_symmetric_kl
    proxy_symmetric-kl proxy_sinkhorn""".split()
)
