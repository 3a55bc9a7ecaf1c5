"""``NNDescent`` -- drop-in for the BUILD path of ``pynndescent.NNDescent`` on an MI355X.

Mirrors the reference constructor (pynndescent/pynndescent_.py:976-1269): same keyword arguments in
the same positional order, same derived defaults, same RandomState draw order, same attributes after
construction, same errors and warnings.  The dense euclidean / cosine branch
(pynndescent_.py:1221-1260) -- ``make_forest`` + ``rptree_leaf_array`` + ``nn_descent`` -- runs on
the GPU through the C ABI of ``include/pynnd_amd.h``.  Nothing here computes neighbours on the CPU:
if the HIP library or a gfx950 device is missing, construction raises.

Also on the GPU: ``update`` (warm start, pynndescent_.py:2381-2553), ``build_search_graph`` (the pruning
pass of ``_init_search_graph``, all diversify methods), ``prepare`` (hub search tree + reordering) and
``query``.  Metrics: euclidean / l2 / sqeuclidean / cosine / dot / inner_product / correlation / hellinger (hellinger input
must be non-negative: a negative entry raises ``ValueError``, where the reference computes NaN distances without a word) and
proxy_inner_product (graph and walk on the reference's proxy distance, queries reranked by the true inner product); and the
metrics that are euclidean after a fixed linear map of the rows, with ``metric_kwds`` read positionally as the reference reads
it: seuclidean / standardised_euclidean ``(V,)``, wminkowski / weighted_minkowski ``(w,)`` or ``(w, 2)``, mahalanobis ``(VI,)``
and minkowski ``()`` or ``(2,)`` (linear_map.py; the device transforms every row once, csrc/linear.hip).
Out of scope: sparse input, every other metric, ``n_neighbors`` above 256 or
``max_candidates`` above 128 (``query``: more than 256 results per query).  Those raise ``NotImplementedError`` naming the reference entry point to use
instead; ``pynndescent_amd.make_index`` hands such inputs to ``pynndescent.NNDescent`` when it is importable.
"""
import inspect
import time
from typing import Callable, NamedTuple
from warnings import warn

import numpy as np
from sklearn.utils import check_array, check_random_state

from . import _capi, linear_map

INT32_MIN = np.iinfo(np.int32).min + 1  # pynndescent_.py:62
INT32_MAX = np.iinfo(np.int32).max - 1  # pynndescent_.py:63


def ts():
    """Timestamp used in verbose output (reference utils.py:881-883)."""
    return time.ctime(time.time())


def tau_rand_int(state):
    """Reference utils.py:17-40 on an int64[3] numpy state (used only to warm up search_rng_state)."""
    s = [int(v) for v in state]
    s[0] = (((s[0] & 4294967294) << 12) & 0xFFFFFFFF) ^ ((((s[0] << 13) & 0xFFFFFFFF) ^ s[0]) >> 19)
    s[1] = (((s[1] & 4294967288) << 4) & 0xFFFFFFFF) ^ ((((s[1] << 2) & 0xFFFFFFFF) ^ s[1]) >> 25)
    s[2] = (((s[2] & 4294967280) << 17) & 0xFFFFFFFF) ^ ((((s[2] << 3) & 0xFFFFFFFF) ^ s[2]) >> 11)
    state[0], state[1], state[2] = s
    r = (s[0] ^ s[1] ^ s[2]) & 0xFFFFFFFF
    return r - (1 << 32) if r >= (1 << 31) else r


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


# corrections: numpy.sqrt, large float32 arrays through the library's threaded sqrtf (the same bits, the fresh pages touched in
# parallel); "sqeuclidean" and "correlation" are the kernels' own space, with no correction (pynndescent_.py:1271-1298) --
# neighbor_graph still hands out a copy
_METRICS = {
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
}
# euclidean distance after a fixed linear map of the rows (seuclidean, wminkowski with p = 2, mahalanobis; minkowski with p = 2
# has no map and is the euclidean path itself): code 0 and euclidean's correction on the transformed rows.  A table of its own:
# these names take metric_kwds, the nine above ignore it
_LINEAR_METRICS = {name: _Metric(_capi.METRIC_CODES["euclidean"], _capi.host_sqrt, device_kind=_capi.NND_CORRECT_SQRT, linear=True)
                   for name in linear_map.LINEAR_METRICS}
# the boolean family (distances.py:259-552): functions of the Gram counts of indicator rows (DESIGN.md "Boolean metrics").  A
# table of its own, like the linear one: tests enumerate ``_METRICS``.  jaccard is built on alternative_jaccard and corrected by
# 1 - 2^-v (correct_alternative_jaccard, the same function as cosine's correction); the other eight are handed out as they are.
# ``angular`` is what the reference reports (pynndescent_.py:1075-1086); the device splits indicator rows with euclidean trees.
_BOOLEAN_METRICS = {name: _Metric(code, correct_alternative_cosine if name == "jaccard" else _capi.host_copy,
                                  angular=name in ("jaccard", "dice"), boolean=True,
                                  device_kind=_capi.NND_CORRECT_ALT_COSINE if name == "jaccard" else _capi.NND_CORRECT_COPY)
                    for name, code in _capi.BOOLEAN_METRIC_CODES.items()}
# views of the table by one field
_DISTANCE_CORRECTIONS = {name: m.correction for name, m in _METRICS.items()}
_ANGULAR_METRICS = frozenset(name for name, m in _METRICS.items() if m.angular)


def _metric_of(name):
    """The record of a metric an index already has (its name was accepted by ``_metric_record``)."""
    if name in _METRICS:
        return _METRICS[name]
    return _LINEAR_METRICS[name] if name in _LINEAR_METRICS else _BOOLEAN_METRICS[name]


def _metric_record(metric, reference_fallback=True):
    """The row of ``_METRICS``.  A metric off the device path raises the reference's ValueError (pynndescent_.py:1292), or
    with ``reference_fallback`` NotImplementedError when the reference runs it (a callable, a name it knows): what
    ``make_index`` hands to ``pynndescent.NNDescent``."""
    if not callable(metric) and metric in _METRICS:
        return _METRICS[metric]
    if not callable(metric) and metric in _LINEAR_METRICS:
        return _LINEAR_METRICS[metric]
    if not callable(metric) and metric in _BOOLEAN_METRICS:
        return _BOOLEAN_METRICS[metric]
    if reference_fallback and (callable(metric) or metric in _KNOWN_REFERENCE_METRICS):
        raise NotImplementedError(
            "pynndescent_amd accelerates the dense euclidean / l2 / sqeuclidean / cosine / dot / inner_product / "
            "correlation / hellinger / proxy_inner_product / seuclidean / standardised_euclidean / mahalanobis build and the "
            "p = 2 form of minkowski / wminkowski / weighted_minkowski, and the boolean metrics jaccard / dice / sokalsneath / "
            "matching / rogerstanimoto / sokalmichener / kulsinski / russellrao / yule only; "
            "use pynndescent.NNDescent for metric %r" % (metric,)
        )
    raise ValueError("Metric is neither callable, " + "nor a recognised string")


def _reference_defaults(n, n_neighbors, n_trees=None, n_iters=None, leaf_size=None, max_candidates=None):
    """The reference's derived defaults for what is None: (n_trees, n_iters, leaf_size, max_candidates) for ``n`` rows
    (pynndescent_.py:1009-1012, 1135-1138; rp_trees.py:2845-2846)."""
    if n_trees is None:
        n_trees = max(3, min(12, int(round(2.0 * np.log10(n)))))
    if n_iters is None:
        n_iters = max(5, int(round(np.log2(n))))
    if leaf_size is None:
        leaf_size = max(60, min(256, 5 * int(n_neighbors)))
    if max_candidates is None:
        max_candidates = min(60, n_neighbors)
    return n_trees, n_iters, leaf_size, max_candidates


def _proxy_search_k(k, proxy_beam_size):
    """``search_k`` of a query that is reranked (pynndescent_.py:2309-2312), within what the query kernel keeps."""
    search_k = proxy_beam_size * k
    if search_k < k:
        raise ValueError("proxy_beam_size must be at least 1 (got %r)" % (proxy_beam_size,))
    if search_k > 256:
        raise NotImplementedError("pynndescent_amd keeps proxy_beam_size * k <= 256 candidates per quantized query "
                                  "(got %d); use index.to_reference()" % search_k)
    return search_k


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


def uint8_codebook(raw, random_state):
    """The reference's uint8 codebook (pynndescent_.py:2193-2206) of the rows ``raw`` in their ORIGINAL order: a sample of
    min(10000, n) rows drawn by ``check_random_state(random_state)``; its distinct values when there are at most 256,
    else its quantiles at ``linspace(0, 1, 256)``; float32."""
    rs = check_random_state(random_state)
    sample = raw[rs.choice(raw.shape[0], min(10000, raw.shape[0]), replace=False)].ravel()
    unique = np.unique(sample)
    if len(unique) <= 256:
        return unique.astype(np.float32)
    return np.quantile(sample, np.linspace(0, 1, 256)).astype(np.float32)


# ---- device arrays: input that lives on the GPU (in practice a torch.Tensor on a HIP device; torch is imported on this path only)
_DEVICE_DTYPES = {"float32": _capi.NND_DTYPE_FLOAT32, "float16": _capi.NND_DTYPE_FLOAT16, "bfloat16": _capi.NND_DTYPE_BFLOAT16,
                  "float64": _capi.NND_DTYPE_FLOAT64}


def _is_device_array(a):
    """A device array: ``is_cuda`` is true and there is a ``data_ptr()`` (with ``dtype``, ``shape``, ``device``, ``is_contiguous()``)."""
    return getattr(a, "is_cuda", False) is True and callable(getattr(a, "data_ptr", None))


def _check_device_array(a, device=0, what="data"):
    """check_array for a device array: 2-D, float32 / float16 / bfloat16 / float64, on the GPU ``device`` names when that is not
    0 (the default means "where the array is").  Returns ``(the array, contiguous -- a device copy when it was not --, its
    NND_DTYPE_* code, its device ordinal)``; no device work besides that copy, no torch."""
    name = str(a.dtype).rsplit(".", 1)[-1]
    if name not in _DEVICE_DTYPES:
        raise TypeError("pynndescent_amd takes device arrays of dtype float32, float16, bfloat16 or float64 (%s has dtype %s)"
                        % (what, a.dtype))
    if len(a.shape) != 2:
        raise ValueError("Expected 2D array, got %dD array instead: %s has shape %s" % (len(a.shape), what, tuple(a.shape)))
    ordinal = getattr(a.device, "index", None)
    ordinal = 0 if ordinal is None else int(ordinal)
    if device and int(device) != ordinal:
        raise ValueError("device=%d, but %s is on device %d: the index runs where its data is" % (int(device), what, ordinal))
    if not a.is_contiguous():
        a = a.contiguous()
    return a, _DEVICE_DTYPES[name], ordinal


def _torch():
    import torch  # (lazily: a host-only install never needs it)

    return torch


def _dtype_name(a):
    """``float32`` of ``torch.float32``: the key of ``_DEVICE_DTYPES`` and the attribute of torch."""
    return str(a.dtype).rsplit(".", 1)[-1]


def _shape_of(a):
    """The shape of a host array-like or a device array, without bringing either anywhere."""
    return tuple(a.shape) if hasattr(a, "shape") else np.shape(a)


def _rows_to_host(a):
    """A device array as the float32 host rows ``check_array`` would make of its values (a host array: as it is)."""
    return np.ascontiguousarray(a.detach().float().cpu().numpy()) if _is_device_array(a) else a


def _ids_to_host(a):
    """Row ids given as a device array, on the host (they are few); everything else as it is."""
    return a.detach().cpu().numpy() if _is_device_array(a) else a


def _updates_on_device(index, xs_fresh, xs_updated):
    """Whether ``update()`` of ``index`` stays on the device (``NNDescent._update_device``): the index holds its rows and its graph
    on one GPU, and at least one of the incoming arrays is a device array.  Reads ``__dict__`` only."""
    d = index.__dict__
    if "_device_data" not in d or "_device_graph" not in d or int(d.get("n_devices", 1)) != 1:
        return False
    return _is_device_array(xs_fresh) or _is_device_array(xs_updated)


def _resolve_updated_indices(updated_indices, n_old):
    """``updated_indices`` as the host loop ``raw[i] = x`` reads them (pynndescent_.py:2467-2469), resolved to distinct pairs:
    ``(row ids, source rows)``, int32, ids ascending -- a negative id wraps, of several entries that name one row the last one
    wins, an id outside ``[-n_old, n_old)`` raises numpy's ``IndexError``.  No two pairs write one row."""
    ids = np.asarray(updated_indices, dtype=np.int64).reshape(-1)
    outside = (ids < -n_old) | (ids >= n_old)
    if outside.any():
        raise IndexError("index %d is out of bounds for axis 0 with size %d" % (int(ids[outside][0]), n_old))
    ids = np.where(ids < 0, ids + n_old, ids)
    unique, first_from_the_end = np.unique(ids[::-1], return_index=True)
    return unique.astype(np.int32), (ids.shape[0] - 1 - first_from_the_end).astype(np.int32)


def _update_dtype(names):
    """The dtype rule of the device ``update()``: ``names`` -- the dtype names of the index's tensor and of every incoming array
    (a host array counts as float32, what ``check_array`` makes of it) -- share one dtype: it is kept; otherwise float32."""
    names = list(names)
    return names[0] if all(name == names[0] for name in names) else "float32"


class _OnTorchStream:
    """The HIP stream a library call runs on so that it is ordered with torch's work on ``ordinal``: torch's current stream.  The
    default stream has no handle a builder could adopt (NULL means the builder's own, which does not wait for it), so there
    the call runs on a side stream that waits for the default stream first and that the default stream waits for afterwards
    -- on the device; the host waits for nothing."""

    def __init__(self, torch, ordinal):
        self.current = torch.cuda.current_stream(ordinal)
        self.side = None
        if not self.current.cuda_stream:
            self.side = torch.cuda.Stream(device=ordinal)
            self.side.wait_stream(self.current)
        self.ptr = (self.side or self.current).cuda_stream

    def done(self):
        if self.side is not None:
            self.current.wait_stream(self.side)


def _stream_ms(torch, stream, fn):
    """``fn()`` between two events on the stream of an ``_OnTorchStream``: (its result, the stream time in ms).  For calls that
    return with the stream drained (the entries of csrc/prepare.hip, the searcher's fill): reading the time waits for nothing."""
    on = stream.side or stream.current
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(on)
    out = fn()
    e1.record(on)
    e1.synchronize()
    return out, float(e0.elapsed_time(e1))


class _DeviceInput:
    """The device side of one single-GPU build (``_build_graph``): the caller's tensor in, the finished graph out as tensors."""

    def __init__(self, tensor, dtype, ordinal, k, as_given=False, linear=None):
        self.torch = _torch()
        self.tensor, self.dtype, self.ordinal, self.k = tensor, dtype, ordinal, int(k)
        # what the device works on: the caller's own tensor, dot's normalised float32 rows, or the rows a linear map transformed
        self.rows = tensor
        self.as_given = as_given  # update(): dot's rows enter as they are (float32, pynndescent_.py:2461-2476 normalises nothing)
        self.linear = linear  # a _DeviceLinear: the metric's map on this device (None: the metric has none)

    def host_rows(self):
        """The caller's rows on the host, float32: for sklearn's wording of the NaN / inf error, the one place that needs them."""
        return np.ascontiguousarray(self.tensor.detach().float().cpu().numpy())

    def set_data(self, builder, m):
        torch, t = self.torch, self.tensor
        self.stream = _OnTorchStream(torch, self.ordinal)
        builder.set_stream(self.stream.ptr)
        if self.linear is not None:  # the builder borrows the transformed copy, and the index keeps it next to the caller's rows
            self.rows = self.linear.rows(t, self.dtype, self.stream.ptr)
            builder.set_data_device(self.rows.data_ptr(), keepalive=self.rows)
        elif m.normalize and self.as_given:  # (the typed entry would normalise every dot input)
            builder.set_data_device(t.data_ptr(), keepalive=t)
        elif m.normalize:  # pynndescent_.py:1101-1102: the index holds the normalised rows; the builder borrows them
            self.rows = torch.empty(tuple(t.shape), dtype=torch.float32, device=t.device)
            _capi.device_rows_f32(self.ordinal, self.stream.ptr, t.data_ptr(), self.dtype, t.shape[0], t.shape[1], True,
                                  self.rows.data_ptr())
            builder.set_data_device(self.rows.data_ptr(), keepalive=self.rows)
        else:
            builder.set_data_device_typed(t.data_ptr(), self.dtype, keepalive=t)

    def finalize(self, builder):
        torch, n = self.torch, self.tensor.shape[0]
        idx = torch.empty((n, self.k), dtype=torch.int32, device=self.tensor.device)
        dist = torch.empty((n, self.k), dtype=torch.float32, device=self.tensor.device)
        builder.finalize_device(idx.data_ptr(), dist.data_ptr())
        return idx, dist

    def close(self):
        if getattr(self, "stream", None) is not None:
            self.stream.done()
            self.stream = None


class _DeviceLinear:
    """A metric's linear map (``linear_map.LinearMap``) on one device: ``a`` and ``shift`` as float32 tensors there (uploaded
    here, on torch's current stream: make it before the ``_OnTorchStream`` of the call that uses it)."""

    def __init__(self, lin, device, ordinal):
        torch = _torch()
        self.kind, self.ordinal = int(lin.kind), int(ordinal)
        self.a = torch.from_numpy(np.ascontiguousarray(lin.a, dtype=np.float32)).to(device)
        self.shift = torch.from_numpy(np.ascontiguousarray(lin.shift, dtype=np.float32)).to(device)

    def rows(self, t, dtype, stream_ptr):
        """``A (x - shift)`` of the contiguous (n, d) tensor ``t`` (``dtype``: its NND_DTYPE_*): a new float32 tensor, queued on
        ``stream_ptr``.  The existing conversion to float32 runs first (csrc/devarray.hip), then csrc/linear.hip."""
        torch = _torch()
        n, dim = int(t.shape[0]), int(t.shape[1])
        out = torch.empty((n, dim), dtype=torch.float32, device=t.device)
        if n == 0:
            return out
        if dtype != _capi.NND_DTYPE_FLOAT32:
            x32 = torch.empty((n, dim), dtype=torch.float32, device=t.device)
            _capi.device_rows_f32(self.ordinal, stream_ptr, t.data_ptr(), dtype, n, dim, False, x32.data_ptr())
            t = x32
        _capi.device_linear_rows(self.ordinal, stream_ptr, self.kind, dim, self.a.data_ptr(), self.shift.data_ptr(), t.data_ptr(), n,
                                 out.data_ptr())
        return out


def _linear_map_of(metric, m, metric_kwds, dim):
    """The ``LinearMap`` (without its shift) of a metric that carries one; None for every other metric -- ``metric_kwds`` stays
    unread for those -- and for minkowski with p = 2.  Raises what ``linear_map.parse_metric_kwds`` raises."""
    return linear_map.parse_metric_kwds(metric, metric_kwds, dim) if m.linear else None


def _refuse_with_linear(metric, m, quantization, n_devices):
    """What the metrics with a linear map, and the boolean metrics, do not combine with, reported before any device work."""
    if not (m.linear or m.boolean):
        return
    if quantization == "uint8":
        _check_quantization(quantization, metric)  # the reference's ValueError("Not uint8 quantization version of ...")
    if int(n_devices) > 1:
        raise NotImplementedError("pynndescent_amd builds metric %r on one GPU (n_devices = %d): the row-sharded build has no "
                                  "%s; use n_devices=1" % (metric, int(n_devices), "linear map" if m.linear else "boolean metrics"))


def _device_corrected(torch, dist, m, ordinal):
    """``m.correction`` of the float32 tensor ``dist``, on the device by the library (a new tensor; float64 where the host's is)."""
    kind = m.device_kind
    out = torch.empty_like(dist, dtype=torch.float32 if kind in (_capi.NND_CORRECT_COPY, _capi.NND_CORRECT_SQRT) else torch.float64)
    _capi.device_correct(ordinal, torch.cuda.current_stream(ordinal).cuda_stream, kind, dist.data_ptr(), out.data_ptr(), dist.numel())
    return out


class _DeviceRowsView:
    """The rows of a device tensor for ``uint8_codebook``: its shape, and ``view[rows]`` -- the sample, gathered on the device with
    torch indexing and brought to the host as float32 (at most 10 000 rows cross the bus, in the order asked for)."""

    def __init__(self, tensor):
        self.tensor, self.shape = tensor, tuple(tensor.shape)

    def __getitem__(self, rows):
        torch = _torch()
        at = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)).to(self.tensor.device)
        return np.ascontiguousarray(self.tensor.detach()[at].float().cpu().numpy())


def _prepares_on_device(index):
    """Whether ``prepare()`` of ``index`` runs from its device tensors (``NNDescent._init_search_graph_device``): an index built
    from a device array on one GPU that still holds its rows and its graph there, a graph within the device pass's edge
    positions, and no reason to go through the host -- the ``_host_prepare`` switch, or dot with uint8 codes (they are the codes
    of rows other than the searcher's own copy).  Reads ``__dict__`` only: no host mirror is fetched by asking."""
    from .search_graph import DEVICE_PASS_MAX_EDGES

    d = index.__dict__
    if d.get("_host_prepare", getattr(type(index), "_host_prepare", False)):
        return False
    if "_device_data" not in d or "_device_graph" not in d or int(d.get("n_devices", 1)) != 1:
        return False
    if d.get("quantization") == "uint8" and _metric_of(d["metric"]).normalize:
        return False
    n, k = (int(v) for v in d["_device_graph"][0].shape)
    return 2 * n * k < DEVICE_PASS_MAX_EDGES


class _DeviceForestSentinel:
    """Stands in for ``_rp_forest``: downstream reference code only null-checks it
    (pynndescent_.py:1353) -- the build consumes nothing but the leaf array."""

    def __init__(self, n_trees, n_leaves, max_leaf_size):
        self.n_trees, self.n_leaves, self.max_leaf_size = n_trees, n_leaves, max_leaf_size

    def __len__(self):
        return self.n_trees


class NNDescent:
    """See ``pynndescent.NNDescent``; constructor signature identical (pynndescent_.py:976-1007)."""

    # the host-path switch of prepare(): set ``index._host_prepare = True`` on an index built from a device array and its
    # prepare() takes the path of a host-built index (mirrors fetched, scipy reorder, three uploads) -- tests and
    # tools/ab/device_prepare_timing.py compare the two paths on one and the same graph with it
    _host_prepare = False

    def __init__(
        self,
        data,
        metric="euclidean",
        metric_kwds=None,
        bit_metric=False,
        n_neighbors=30,
        n_trees=None,
        angular_trees=False,
        leaf_size=None,
        pruning_degree_multiplier=1.5,
        diversify_prob=1.0,
        diversify_method="standard",
        degree_prune_aggressiveness=1.0,
        n_search_trees=1,
        search_tree_leaf_size=None,
        max_search_tree_depth=None,
        quantization=None,
        tree_init=True,
        init_graph=None,
        init_dist=None,
        random_state=None,
        low_memory=True,
        max_candidates=None,
        max_rptree_depth=200,
        n_iters=None,
        delta=0.001,
        n_jobs=None,
        compressed=False,
        parallel_batch_queries=False,
        verbose=False,
        device=0,
        n_devices=1,
        devices=None,
    ):
        """``device``: HIP ordinal of the GPU that builds the index.  ``n_devices`` > 1: the build is row-sharded over that
        many GPUs of this node (``nnd_build_multi``: one host thread per GPU inside the library, RCCL over xGMI; the
        reference's analogue is ``n_jobs``, pynndescent_.py:1141-1143); ``devices`` lists their ordinals (default
        0..n_devices-1; a list that repeats an ordinal puts several ranks on one GPU).  Everything after the build
        (``prepare``, ``query``, ``update``) runs on ``device``.

        ``data`` may be a device array -- a 2-D ``torch.Tensor`` on a HIP device, float32 / float16 / bfloat16 / float64 (half
        precision and float64 are converted to float32 on the device; a float32 tensor is kept by reference, not copied).
        The index then runs on the tensor's device and on torch's current stream: data queued on that stream needs no
        synchronisation, and ``neighbor_graph`` / ``query(device array)`` return tensors there, corrected on the device.
        ``prepare()`` -- and so the first ``query()`` -- runs from those tensors too (hub rank, tree, pruning pass, reorder and
        the searcher's fill on the device: only the tree's tables, ``_vertex_order`` and scalars cross the bus; dot with
        ``quantization="uint8"`` takes the host path).  ``_raw_data``, ``_neighbor_graph``, ``_search_graph`` and
        ``_quantized_data`` are host mirrors fetched on first use; ``build_search_graph``, pickling and ``to_reference`` work
        through them.  ``update()`` with a tensor and ``recall()`` stay on the device (``_update_device``, ``_recall_device``);
        ``update()`` with host arrays alone makes the index a host index.  ``init_graph`` / ``init_dist`` may be tensors as well:
        with device ``data`` on one GPU they are cast to int32 / float32 on the device and seed the build where they are
        (``nnd_init_from_graph_device``); in every other combination they are brought to the host.  Out of scope: the hub
        tree's FlatTree assembly on the device; producers other than torch (``__cuda_array_interface__``, DLPack); and a sharded
        build from device memory -- with ``n_devices`` > 1 the rows are brought to the host first and the index is a host index,
        as for host input."""
        dev_checked = None
        if _is_device_array(data):  # dtype, shape and device first: before any device work, and before the shape is read
            dev_checked = _check_device_array(data, device)
            data, device = dev_checked[0], dev_checked[2]
        # init_graph / init_dist tensors seed a device build where they are (cast on torch's stream here, before the builder's
        # stream is taken from it); every other combination meets on the host
        if dev_checked is not None and int(n_devices) == 1 and _is_device_array(init_graph) and (init_dist is None or _is_device_array(init_dist)):
            torch = _torch()
            init_graph = init_graph.detach().to(device=data.device, dtype=torch.int32).contiguous()
            if init_dist is not None:
                init_dist = init_dist.detach().to(device=data.device, dtype=torch.float32).contiguous()
        else:
            init_graph, init_dist = _ids_to_host(init_graph), _ids_to_host(init_dist)
        n_trees, n_iters, eff_leaf_size, eff_max_candidates = _reference_defaults(
            data.shape[0], n_neighbors, n_trees, n_iters, leaf_size, max_candidates)

        self.n_trees = n_trees
        self.angular_trees = angular_trees
        self.n_trees_after_update = max(2, int(np.round(self.n_trees / 3)))
        self.n_neighbors = n_neighbors
        self.metric = metric
        self.metric_kwds = metric_kwds
        self.bit_metric = bit_metric
        self.leaf_size = leaf_size
        self.prune_degree_multiplier = pruning_degree_multiplier
        self.diversify_prob = diversify_prob
        self.diversify_method = diversify_method
        self.degree_prune_aggressiveness = degree_prune_aggressiveness
        self.n_search_trees = n_search_trees
        self.search_tree_leaf_size = search_tree_leaf_size
        self.max_search_tree_depth = max_search_tree_depth
        self.max_rptree_depth = max_rptree_depth
        self.max_candidates = max_candidates
        self.quantization = quantization
        self.low_memory = low_memory
        self.n_iters = n_iters
        self.delta = delta
        self.dim = data.shape[1]
        self.n_jobs = n_jobs
        self.compressed = compressed
        self.parallel_batch_queries = parallel_batch_queries
        self.verbose = verbose
        self.device = device
        self.n_devices = int(n_devices)
        self.devices = None if devices is None else [int(v) for v in devices]
        if self.n_devices < 1 or (self.devices is not None and len(self.devices) != self.n_devices):
            raise ValueError("n_devices must be >= 1 and match len(devices)")

        m = _metric_record(metric)
        lin = _linear_map_of(metric, m, metric_kwds, data.shape[1])  # (host only: every error of metric_kwds comes first)
        _refuse_with_linear(metric, m, quantization, self.n_devices)
        try:
            import scipy.sparse

            if scipy.sparse.issparse(data):
                raise NotImplementedError(
                    "sparse input is out of scope for pynndescent_amd; use pynndescent.NNDescent (sparse_nndescent)"
                )
        except ImportError:  # pragma: no cover
            pass

        _check_supported_sizes(n_neighbors, max_candidates, init_graph)
        # pynndescent_.py:1054 check_array(data, dtype=np.float32, order="C") -- minus its single-core scan for NaN / inf
        # (24 ms at 1 M x 128): the prep kernel looks at every value anyway and raises a flag; _raise_if_nonfinite then
        # lets sklearn produce the reference's own error
        # pynndescent_.py:1041-1046: a float32 C-contiguous input is the caller's own array after check_array -- normalised
        # into a copy; any other input has been copied by check_array already and is normalised in place
        dev_in = None
        if dev_checked is not None:
            _, dtype_code, ordinal = dev_checked
            if self.n_devices > 1:  # the sharded build takes its rows from the host, as for host input
                data = np.ascontiguousarray(data.detach().float().cpu().numpy())
            else:
                dev_in = _DeviceInput(data, dtype_code, ordinal, n_neighbors)
        copy_on_normalize = getattr(data, "dtype", None) == np.float32 and bool(getattr(getattr(data, "flags", None), "c_contiguous", False))
        if dev_in is None:
            data = _check_array_no_scan(data)
        self.tree_init = not (not tree_init or n_trees == 0 or init_graph is not None)  # pynndescent_.py:1059-1062
        self._dist_args = tuple((metric_kwds or {}).values())
        current_random_state = self._set_up(None if dev_in is not None else data, m, random_state, copy_on_normalize)
        if dev_in is None:
            data = self._raw_data
        self._linear_map = None
        if lin is not None:  # the shift is fixed here, once; the device builds on the transformed copy, _raw_data stays the caller's
            self._linear_map = lin = lin._replace(shift=linear_map.shift_of(data if dev_in is None else _DeviceRowsView(data)))
            if dev_in is None:
                data = self._lin_data = _capi.linear_rows_host(lin.kind, lin.a, lin.shift, data, device=device)
            else:
                dev_in.linear = self._linear_on_device(data.device)

        n = data.shape[0]
        if self.tree_init:
            if verbose:
                print(ts(), "Building RP forest with", str(n_trees), "trees")
            tree_states = current_random_state.randint(INT32_MIN, INT32_MAX, size=(n_trees, 3)).astype(np.int64)
            eff_trees = n_trees
        else:
            tree_states = np.zeros((1, 3), np.int64)
            eff_trees = 0

        if init_graph is not None:
            if not _is_device_array(init_graph):
                init_graph = np.asarray(init_graph)
            if init_graph.shape[0] != n:
                raise ValueError("Init graph size does not match dataset size!")  # pynndescent_.py:1229
            if init_dist is not None and tuple(init_graph.shape) != _shape_of(init_dist):
                raise ValueError("The shapes of init graph and init distances do not match!")  # pynndescent_.py:1236

        if self.n_devices > 1:  # (a build that starts from init_graph is sharded too -- nnd_build_multi_from_graph)
            n_leaves = self._build_multi(data, eff_trees, eff_leaf_size, eff_max_candidates, tree_states[0], verbose,
                                         init_graph=init_graph, init_dist=init_dist)
        else:
            graph, self._build_stats, n_leaves = _build_graph(
                data, m, n_neighbors, eff_trees, eff_leaf_size, max_rptree_depth, eff_max_candidates, n_iters, delta,
                self.rng_state, tree_states[0], device, forest=self.tree_init, init_graph=init_graph, init_dist=init_dist,
                random_fill=init_graph is None, check_finite=True, verbose=verbose, announce=verbose, dev_in=dev_in)
            if dev_in is None:
                self._neighbor_graph = graph
            else:  # the graph and the rows stay on the device; _neighbor_graph / _raw_data are fetched when first read
                self._device_graph, self._device_data = graph, dev_in.rows
                if dev_in.linear is not None:  # _device_data: the transformed rows the device works on; the caller's tensor stays
                    self._device_raw = dev_in.tensor
        self._rp_forest = _DeviceForestSentinel(n_trees, n_leaves, eff_leaf_size) if self.tree_init else None

        # pynndescent_.py:1262-1267 `np.any(indices < 0)`: rows are ascending with the unfilled entries (-1, +inf) at the
        # tail, so the last column tells (1 M strided reads instead of a 15 M-element temporary; on the device: one scalar back)
        if dev_in is not None:
            unfilled = bool((self._device_graph[0][:, -1].min() < 0).item())
        else:
            unfilled = self._neighbor_graph[0][:, -1].min() < 0
        if unfilled:
            warn(
                "Failed to correctly find n_neighbors for some samples."
                " Results may be less than ideal. Try re-running with"
                " different parameters."
            )

    def _set_up(self, data, m, random_state, copy):
        """What the constructor and ``from_graph`` share (pynndescent_.py:1064-1113): the data the index holds (dot: rows
        L2-normalised, into a new array when ``copy``; ``data`` None: the rows are on the device), the metric's correction and tree flags, and ``rng_state`` /
        ``search_rng_state`` drawn in the reference's order.  Returns the RandomState, whose next draws are the trees'."""
        if data is not None and m.normalize:  # pynndescent_.py:1101-1102
            from sklearn.preprocessing import normalize

            data = normalize(data, norm="l2", copy=copy)
        self._input_dtype = np.float32
        if data is not None:  # (None: a device array -- _raw_data is its host mirror, fetched by __getattr__)
            self._raw_data = data
        self.random_state = random_state
        current_random_state = check_random_state(random_state)
        self._distance_correction = m.correction
        self._distance_func = None  # device kernels; see include/pynnd_amd.h NND_METRIC_*
        self._is_proxy_distance = m.proxy  # pynndescent_.py:1272-1280 (the true distance: the rerank of csrc/query.hip)
        self._angular_trees = m.angular
        self._bit_trees = False
        self._is_sparse = False
        # RandomState draw order of the reference: rng_state, search_rng_state, then the per-tree
        # states inside make_forest (pynndescent_.py:1105-1113, rp_trees.py:2850)
        self.rng_state = current_random_state.randint(INT32_MIN, INT32_MAX, 3).astype(np.int64)
        self.search_rng_state = current_random_state.randint(INT32_MIN, INT32_MAX, 3).astype(np.int64)
        for _ in range(10):
            tau_rand_int(self.search_rng_state)
        return current_random_state

    def _build_multi(self, data, n_trees, leaf_size, max_candidates, tree_state, verbose, init_graph=None, init_dist=None,
                     old_graph=None):
        """Row-sharded build over several GPUs, one call into the library (include/pynnd_amd.h nnd_build_multi): from a
        forest, from ``init_graph`` / ``init_dist``, or from a forest and ``old_graph`` (``update()``).  Sets the graph
        and the stats; returns the forest's leaf count."""
        from sklearn.utils import assert_all_finite

        from . import sharded

        assert_all_finite(data)  # check_array's scan (pynndescent_.py:1054): the one-call multi-GPU build has no flag to read
        _raise_if_negative_host(data, _metric_of(self.metric))
        if verbose:
            print(ts(), "NN descent for", str(self.n_iters), "iterations on", self.n_devices, "GPUs")
        idx, dst, st, info = sharded.build_multi(
            data, self.n_devices, self.devices, self.metric, self.n_neighbors, n_trees, leaf_size, max_candidates,
            self.n_iters, self.delta, max_rptree_depth=self.max_rptree_depth, rng_state=self.rng_state,
            tree_state=tree_state, init_graph=init_graph, init_dist=init_dist, old_graph=old_graph)
        self._neighbor_graph = (idx, dst)
        self._build_stats = st
        self._shard_info = info
        if verbose:
            for it, c in enumerate(info["c"]):
                print("\t", it + 1, " / ", self.n_iters, " c =", c)
        return st["n_leaves"]

    @property
    def neighbor_graph(self):
        """pynndescent_.py:2145-2158: copies, with the distance correction applied."""
        if self.compressed and not hasattr(self, "_neighbor_graph"):
            warn("Compressed indexes do not have neighbor graph information.")
            return None
        if "_device_graph" in self.__dict__:  # built from a device array: fresh tensors there, corrected by the library
            torch = _torch()
            idx, dist = self._device_graph
            with torch.cuda.device(self.device):
                return idx.clone(), _device_corrected(torch, dist, _metric_of(self.metric), self.device)
        return (_capi.host_copy(self._neighbor_graph[0]), self._distance_correction(self._neighbor_graph[1]))

    def __getattr__(self, name):
        """The host mirrors of an index built from a device array, fetched on first access and cached: ``_raw_data`` (float32
        numpy rows; dot: the normalised rows the device computed; after a device prepare: in the search tree's leaf order, as
        the host path leaves them) and ``_neighbor_graph`` (numpy int32 / float32); after a device prepare also ``_search_graph``
        (scipy CSR uint8, sorted indices) and ``_quantized_data`` (the searcher's uint8 codes).  Every line that reads the names
        finds them as on a host-built index, and ``hasattr`` keeps its meaning."""
        d = self.__dict__
        if name in ("_raw_data", "_lin_data") and "_device_data" in d and (name == "_raw_data" or d.get("_linear_map") is not None):
            # (a metric with a linear map: _device_data holds the transformed rows, _device_raw the caller's)
            rows = d["_device_raw" if name == "_raw_data" and "_device_raw" in d else "_device_data"].detach()
            if "_device_order" in d:  # x_new[i] = x[order[i]]: the gather the searcher's fill makes
                rows = rows[d["_device_order"].long()]
            value = np.ascontiguousarray(rows.float().cpu().numpy())
        elif name == "_lin_data" and d.get("_linear_map") is not None:
            # the transformed rows of a host index that has none at hand (unpickled, from_graph): a row's transform depends on
            # the row alone, so transforming _raw_data again gives the bits the index was built on, in _raw_data's order
            lin = d["_linear_map"]
            value = _capi.linear_rows_host(lin.kind, lin.a, lin.shift, self._raw_data, device=self.device)
        elif name == "_neighbor_graph" and "_device_graph" in d:
            value = tuple(np.ascontiguousarray(t.cpu().numpy()) for t in d["_device_graph"])
        elif name == "_search_graph" and "_device_search_graph" in d:
            import scipy.sparse as sp

            indptr, indices = (np.ascontiguousarray(t.cpu().numpy()) for t in d["_device_search_graph"])
            n = indptr.shape[0] - 1
            value = sp.csr_array((np.ones(indices.shape[0], np.uint8), indices, indptr), shape=(n, n))
            value.has_sorted_indices = True
        elif (name == "_quantized_data" and "_device_search_graph" in d and d.get("_searcher") is not None
              and d["_searcher"].has_codes):  # the codes the searcher derived from its own rows, deterministic: derived again
            value = d["_searcher"].quantize_u8(d["_quantized_values"], rows=None)
        else:
            raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))
        d[name] = value
        return value

    def _drop_device_copies(self):
        """After the host mirrors have become the truth (``update()``), or for a pickle: the device tensors go."""
        for name in ("_device_graph", "_device_data", "_device_raw", "_device_order", "_device_search_graph", "_device_prepare_stats"):
            self.__dict__.pop(name, None)

    def _kernel_metric(self):
        """The metric name the kernels run: the index's own, or euclidean on the transformed rows of a linear map."""
        return "euclidean" if _metric_of(self.metric).linear else self.metric

    def _work_rows(self):
        """The host rows the device works on: ``_raw_data``, or its transformed copy ``_lin_data`` for a metric with a linear map."""
        return self._lin_data if self.__dict__.get("_linear_map") is not None else self._raw_data

    def _linear_on_device(self, device):
        """The index's linear map as tensors on ``device`` (a ``_DeviceLinear``), uploaded once."""
        d = self.__dict__
        if d.get("_device_linear") is None:
            ordinal = getattr(device, "index", None)
            d["_device_linear"] = _DeviceLinear(d["_linear_map"], device, int(self.device) if ordinal is None else ordinal)
        return d["_device_linear"]

    @property
    def _prepared(self):
        """Whether ``_init_search_graph`` has run (``_vertex_order`` is set eagerly on both paths).  Looks at ``__dict__``: asking
        fetches no host mirror."""
        return "_vertex_order" in self.__dict__

    @staticmethod
    def _recall_rows(n, n_rows, random_state):
        """The rows ``recall`` samples: ``RandomState(random_state).choice(n, min(n_rows, n), replace=False)``."""
        return np.random.RandomState(random_state).choice(int(n), size=min(int(n_rows), int(n)), replace=False).astype(np.int64)

    def recall(self, k=None, n_rows=1000, random_state=None):
        """How good the graph is: the share of the true ``k`` nearest neighbours (self included; ``k`` defaults to
        ``min(10, n_neighbors)``) that appear anywhere in the graph's row, averaged over ``min(n_rows, n)`` distinct rows
        drawn by ``_recall_rows`` -- the convention of the reference's tests (tests/test_pynndescent_.py:27-31).  The truth
        is the exact brute-force search of ``exact_knn`` over the index's data; only the data and the graph are read, so
        every way of making the index (one or several devices, ``from_graph``, after ``update()``) is covered.  An index built
        from a device array on one GPU is measured where it is: the exact search and the count run on its tensors, the sampled
        row ids go up and one integer comes back (the same value, and no host mirror is fetched).  dot: the truth is searched
        on rows normalised once more -- by the device there, by sklearn on the host path -- which agree within rounding only,
        so the two paths may differ where two true neighbours are that close; every other metric gives the same value."""
        _no_exact_for_proxy(self.metric, _metric_of(self.metric), "NNDescent.recall")
        d = self.__dict__
        if "_device_data" in d and "_device_graph" in d and int(d.get("n_devices", 1)) == 1:
            return self._recall_device(k, n_rows, random_state)
        graph_idx = self._neighbor_graph[0]
        n = graph_idx.shape[0]
        k = min(10, int(self.n_neighbors)) if k is None else int(k)
        rows = self._recall_rows(n, n_rows, random_state)
        data = self._work_rows()  # (a metric with a linear map: the truth is euclidean on the transformed rows)
        if hasattr(self, "_vertex_order"):  # prepare() keeps the rows in the search tree's leaf order; the graph keeps its numbering
            data = data[np.argsort(self._vertex_order), :]
        true_idx = exact_knn(data, k=k, metric=self._kernel_metric(), rows=rows, device=getattr(self, "device", 0))[0]
        hits = sum(int(np.isin(t, a).sum()) for t, a in zip(true_idx, graph_idx[rows]))
        return hits / float(true_idx.shape[0] * k)

    def _recall_device(self, k, n_rows, random_state):
        """``recall`` of an index that holds its rows and its graph on the device: the sampled ids go up, the exact search runs on
        the tensors (``_device_data`` keeps the original order through ``prepare()``), one wave per sampled row counts the true ids
        found in the graph's row, and one integer comes back.  No host mirror is read or made."""
        torch, d = _torch(), self.__dict__
        data, gidx = d["_device_data"], d["_device_graph"][0]
        n, ordinal = int(gidx.shape[0]), int(self.device)
        k = min(10, int(self.n_neighbors)) if k is None else int(k)
        rows = self._recall_rows(n, n_rows, random_state)
        with torch.cuda.device(ordinal):
            rows_dev = torch.from_numpy(rows.astype(np.int32)).to(data.device)
            true_idx = _exact_knn_device(data, None, k, self.metric, _metric_of(self.metric), rows_dev, ordinal, False)[0]
            hits = torch.empty((1,), dtype=torch.int64, device=data.device)
            _capi.device_recall_hits(ordinal, torch.cuda.current_stream(ordinal).cuda_stream, true_idx.data_ptr(), true_idx.shape[0], k,
                                     gidx.data_ptr(), n, gidx.shape[1], rows_dev.data_ptr(), hits.data_ptr())
            return int(hits.item()) / float(true_idx.shape[0] * k)

    def build_search_graph(self):
        """The pruning pass of ``_init_search_graph`` (pynndescent_.py:1451-1611: diversify, reverse diversify,
        degree prune) on the GPU alone; returns the CSR uint8 graph in the ORIGINAL vertex numbering (``prepare()``
        runs the same pass and then re-indexes everything by the hub search tree's leaf order)."""
        from .search_graph import build_search_graph

        if self._prepared:
            raise RuntimeError("the index is prepared already: its search graph is index._search_graph (in leaf order)")
        self._pruned_graph = build_search_graph(
            self._work_rows(), self._neighbor_graph[0], self._neighbor_graph[1], self._kernel_metric(), self.n_neighbors,
            self.prune_degree_multiplier, self.diversify_prob, self.diversify_method,
            degree_prune_aggressiveness=self.degree_prune_aggressiveness,
            seed=int(self.rng_state[0]) & 0xFFFFFFFF, device=self.device)
        return self._pruned_graph

    # attributes of the reference class that prepare() / query() / update() read (pynndescent_.py:1014-1113)
    _HANDOVER = (
        "n_trees", "angular_trees", "n_trees_after_update", "n_neighbors", "metric", "metric_kwds", "bit_metric",
        "leaf_size", "prune_degree_multiplier", "diversify_prob", "diversify_method", "degree_prune_aggressiveness",
        "n_search_trees", "search_tree_leaf_size", "max_search_tree_depth", "max_rptree_depth", "max_candidates",
        "quantization", "low_memory", "n_iters", "delta", "dim", "n_jobs", "compressed", "parallel_batch_queries",
        "verbose", "_input_dtype", "_raw_data", "tree_init", "_dist_args", "random_state", "_angular_trees",
        "_bit_trees", "_is_sparse", "rng_state", "search_rng_state", "_rp_forest",
    )

    def to_reference(self):
        """Hand the GPU-built index to ``pynndescent.NNDescent`` (must be importable) WITHOUT rebuilding: the returned
        object carries this index's data, graph and parameters, so the reference's own ``prepare()`` (hub search tree,
        pruned + reordered search graph) and ``query()`` run on it unchanged.  The reference only null-checks
        ``_rp_forest`` before building its hub tree from the graph (pynndescent_.py:1353-1437).

        seuclidean / wminkowski / mahalanobis / minkowski: the reference keeps no squared space for them, so the graph handed
        over holds true distances, and the search structures of a prepared index are LEFT OUT of the hand-over (its tree's
        hyperplanes split the transformed space, the reference's tree descent takes raw queries): the rows go back to their
        original order and the reference's own ``prepare()`` rebuilds tree and search graph from the graph."""
        import pynndescent

        linear = _metric_of(self.metric).linear
        ref = object.__new__(pynndescent.NNDescent)
        for name in self._HANDOVER:
            if hasattr(self, name):
                setattr(ref, name, getattr(self, name))
        if linear and self._prepared:
            ref._raw_data = np.ascontiguousarray(self._raw_data[np.argsort(self._vertex_order), :])
        if hasattr(self, "_neighbor_graph"):
            dist = self._neighbor_graph[1]
            ref._neighbor_graph = (self._neighbor_graph[0].copy(), np.sqrt(dist) if linear else dist.copy())
        ref._distance_correction = None
        ref._set_distance_func()  # pynndescent_.py:1271-1298: numba distance, correction, proxy flags
        if hasattr(self, "_search_graph") and not linear:  # prepared on the GPU: the reference's prepare() has nothing left to build
            from pynndescent.rp_trees import FlatTree as RefFlatTree

            ref._search_graph = self._search_graph.copy()
            ref._search_forest = [RefFlatTree(*t) for t in self._search_forest]
            ref._vertex_order = np.asarray(self._vertex_order).copy()
            ref._min_distance = self._min_distance
            ref._visited = np.zeros_like(self._visited)
            if hasattr(ref, "_rp_forest"):
                del ref._rp_forest
        return ref

    @classmethod
    def from_graph(cls, data, indices, distances, metric="euclidean", random_state=None, **kwargs):
        """An index object around an existing k-NN graph (``distances`` in the alternative space, rows ascending), no
        build: the starting point for ``update()`` / ``build_search_graph()`` / ``to_reference()``."""
        self = object.__new__(cls)
        data = check_array(data, dtype=np.float32, order="C")
        n = data.shape[0]
        if "pruning_degree_multiplier" in kwargs:  # the constructor's name for prune_degree_multiplier
            kwargs["prune_degree_multiplier"] = kwargs.pop("pruning_degree_multiplier")
        unknown = set(kwargs) - set(_FROM_GRAPH_DEFAULTS)
        if unknown:
            raise TypeError("unexpected arguments: %s" % sorted(unknown))
        for name, value in dict(_FROM_GRAPH_DEFAULTS, **kwargs).items():
            setattr(self, name, value)
        m = _metric_record(metric, reference_fallback=False)
        indices = np.ascontiguousarray(indices, np.int32)
        distances = np.ascontiguousarray(distances, np.float32)
        if indices.shape != distances.shape or indices.shape[0] != n:
            raise ValueError("Init graph size does not match dataset size!")
        _check_supported_sizes(indices.shape[1], self.max_candidates, None)
        _raise_if_negative_host(data, m)
        self.metric, self.n_neighbors = metric, indices.shape[1]
        self.n_trees, self.n_iters, _, _ = _reference_defaults(n, self.n_neighbors, self.n_trees, self.n_iters)
        self.n_trees_after_update = max(2, int(np.round(self.n_trees / 3)))
        self.dim = data.shape[1]
        self.tree_init = True
        self._dist_args = tuple((self.metric_kwds or {}).values())
        lin = _linear_map_of(metric, m, self.metric_kwds, data.shape[1])
        _refuse_with_linear(metric, m, self.quantization, 1)
        self._set_up(data, m, random_state, copy=True)  # (dot: the data NNDescent would hold, in a new array)
        # (``distances`` of a metric with a linear map: squared, of the rows transformed with this shift -- what the build keeps)
        self._linear_map = None if lin is None else lin._replace(shift=linear_map.shift_of(self._raw_data))
        self._rp_forest = _DeviceForestSentinel(self.n_trees, 0, 0)
        self._neighbor_graph = (indices, distances)
        return self

    # ------------------------------------------------------------------------------------------------ prepare / query
    def _init_search_graph(self):
        """``NNDescent._init_search_graph`` (pynndescent_.py:1333-1662) on the GPU: the hub search tree built from the
        data and the finished graph (csrc/hubtree.hip), the pruning pass (csrc/prune.hip), then data, graph and tree
        re-indexed by the tree's leaf order (pynndescent_.py:1629-1651)."""
        from .search_graph import build_search_graph
        from .search_tree import make_hub_tree, reorder_by_tree

        search_leaf_size = (self.search_tree_leaf_size if self.search_tree_leaf_size is not None
                            else (self.leaf_size if self.leaf_size is not None else 30))  # pynndescent_.py:1341-1345
        search_tree_depth = (self.max_search_tree_depth if self.max_search_tree_depth is not None
                             else self.max_rptree_depth)                                   # pynndescent_.py:1346-1350
        if _prepares_on_device(self):
            try:
                return self._init_search_graph_device(search_leaf_size, search_tree_depth)
            except _capi.NNDError as e:
                if "memory" not in str(e).lower():
                    raise
                warn("the search-graph pass does not fit the device (%s): preparing through the host" % e)
        if not hasattr(self, "_search_forest"):
            if getattr(self, "_rp_forest", None) is None and not self.tree_init:
                self._search_forest = []  # pynndescent_.py:1377-1378: no tree, queries start from random vertices
            else:
                if self.verbose:
                    print(ts(), "Building hub-based search tree")
                self._search_forest = [make_hub_tree(self._work_rows(), self._neighbor_graph[0], self._kernel_metric(), search_leaf_size,
                                                     search_tree_depth, device=self.device,
                                                     seed=int(self.rng_state[0]) & 0x7FFFFFFF)]
                self._rp_forest = None  # the reference deletes it here (pynndescent_.py:1444)
        if self.verbose:
            print(ts(), "Diversifying and pruning the search graph")
        graph, stages = build_search_graph(
            self._work_rows(), self._neighbor_graph[0], self._neighbor_graph[1], self._kernel_metric(), self.n_neighbors,
            self.prune_degree_multiplier, self.diversify_prob, self.diversify_method,
            degree_prune_aggressiveness=self.degree_prune_aggressiveness, seed=int(self.rng_state[0]) & 0xFFFFFFFF,
            device=self.device, return_stages=True)
        self._min_distance = np.float32(stages["min_distance"])                     # pynndescent_.py:1539
        self._visited = np.zeros((self._raw_data.shape[0] // 8) + 1, dtype=np.uint8, order="C")  # pynndescent_.py:1624-1626
        if self.verbose:
            print(ts(), "Resorting data and graph based on tree order")
        if self._search_forest:
            graph, data, self._vertex_order, tree = reorder_by_tree(graph, self._work_rows(), self._search_forest[0])
            if self.__dict__.get("_linear_map") is not None:  # both copies in the leaf order
                self._lin_data, self._raw_data = data, np.ascontiguousarray(self._raw_data[self._vertex_order, :])
            else:
                self._raw_data = data
            self._search_forest = [tree] + list(self._search_forest[1: self.n_search_trees])
        else:
            self._vertex_order = np.arange(self._raw_data.shape[0])
        self._search_graph = graph
        self._searcher = None
        if self.compressed:  # pynndescent_.py:1653-1658
            if hasattr(self, "_rp_forest"):
                del self._rp_forest
            del self._neighbor_graph
            self.__dict__.pop("_device_graph", None)

    def _init_search_graph_device(self, search_leaf_size, search_tree_depth):
        """``_init_search_graph`` from the device tensors of an index built from a device array, on torch's current stream
        (``_OnTorchStream``): the in-degrees and the hub rank (csrc/prepare.hip), the hub tree and the pruning pass on handles
        bound to the tensor, the graph re-indexed by the tree's leaf order where the pass left it.  The rows and the graphs
        never visit the host and no host mirror is made; what crosses the bus: the FlatTree tables, ``_vertex_order`` (4 bytes
        per point, down and up again) and scalars.  The rows are gathered when the searcher is filled (``prepare``);
        ``_device_data`` stays the caller's tensor in its original order."""
        from .search_tree import FlatTree

        if self.diversify_method not in ("standard", "degree_aware"):
            raise ValueError("diversify_method must be 'standard' or 'degree_aware'")
        torch, d, m = _torch(), self.__dict__, _metric_of(self.metric)
        data, (gidx, gdist) = d["_device_data"], d["_device_graph"]
        n, dim, k = int(data.shape[0]), int(data.shape[1]), int(gidx.shape[1])
        dtype, ordinal = _DEVICE_DTYPES[str(data.dtype).rsplit(".", 1)[-1]], int(self.device)
        seed = int(self.rng_state[0])
        ms = {}  # stream time of every stage (tools/ab/device_prepare_timing.py reads them)

        def bound(builder, stream):  # dot: _device_data is the normalised float32 copy already, borrowed as it is
            builder.set_stream(stream.ptr)
            if m.normalize:
                builder.set_data_device(data.data_ptr(), keepalive=data)
            else:
                builder.set_data_device_typed(data.data_ptr(), dtype, keepalive=data)
            return builder

        with torch.cuda.device(ordinal):
            if "_search_forest" not in d:
                if getattr(self, "_rp_forest", None) is None and not self.tree_init:
                    self._search_forest = []  # pynndescent_.py:1377-1378: no tree, queries start from random vertices
                else:
                    if self.verbose:
                        print(ts(), "Building hub-based search tree")
                    stream = _OnTorchStream(torch, ordinal)
                    b = None
                    try:
                        rank = torch.empty((n,), dtype=torch.int32, device=data.device)
                        _, ms["ms_rank"] = _stream_ms(torch, stream, lambda: _capi.rank_order_device(
                            ordinal, stream.ptr, gidx.data_ptr(), n, k, rank.data_ptr()))
                        b = _capi.Builder(n, dim, m.code, 1, 1, max(int(search_leaf_size), 1), search_tree_depth, 1, 1, 0.001,
                                          [seed & 0x7FFFFFFF, 2, 3], [4, 5, 6], device=ordinal,
                                          flags=_capi.NND_FLAG_NO_GRAPH | _capi.NND_FLAG_NO_PREP)
                        tables, ms["ms_hub_tree"] = _stream_ms(torch, stream, lambda: bound(b, stream).hub_tree_device(
                            rank.data_ptr(), search_leaf_size, search_tree_depth))
                        self._search_forest = [FlatTree(*tables)]
                    finally:
                        if b is not None:
                            b.close()
                        stream.done()
                    self._rp_forest = None  # the reference deletes it here (pynndescent_.py:1444)
            order = None
            if self._search_forest:  # the leaf order goes up once; the queries' id mapping reads the same tensor
                tree = self._search_forest[0]
                vertex_order = np.asarray(tree.indices)
                order = torch.from_numpy(np.ascontiguousarray(vertex_order, dtype=np.int32)).to(data.device)
            if self.verbose:
                print(ts(), "Diversifying and pruning the search graph")
            stream = _OnTorchStream(torch, ordinal)  # (made after the upload: a side stream waits for it)
            b = None
            try:
                b = bound(_capi.Builder(n, dim, m.code, k, 0, 60, 200, min(60, k), 1, 0.001, [1, 2, 3], [4, 5, 6], device=ordinal,
                                        flags=_capi.NND_FLAG_NO_GRAPH), stream)
                indptr_at, indices_at, nnz, st = b.search_graph_device(
                    gidx.data_ptr(), gdist.data_ptr(), self.n_neighbors, self.prune_degree_multiplier, self.diversify_prob,
                    self.diversify_method == "degree_aware", self.degree_prune_aggressiveness, seed & 0xFFFFFFFF)
                if self.verbose:
                    print(ts(), "Resorting data and graph based on tree order")
                indptr = torch.empty((n + 1,), dtype=torch.int32, device=data.device)
                indices = torch.empty((nnz,), dtype=torch.int32, device=data.device)
                _, ms["ms_reorder"] = _stream_ms(torch, stream, lambda: _capi.reorder_csr_device(
                    ordinal, stream.ptr, 0 if order is None else order.data_ptr(), n, indptr_at, indices_at, nnz, indptr.data_ptr(),
                    indices.data_ptr() if nnz else 0))
            finally:
                if b is not None:
                    b.close()
                stream.done()
        self._min_distance = np.float32(float(st["min_distance"]))                  # pynndescent_.py:1539
        self._visited = np.zeros((n // 8) + 1, dtype=np.uint8, order="C")           # pynndescent_.py:1624-1626
        if order is not None:
            self._vertex_order = vertex_order
            self._device_order = order
            new_tree = FlatTree(tree.hyperplanes, tree.offsets, tree.children, np.arange(n, dtype=np.int32), tree.leaf_size)
            self._search_forest = [new_tree] + list(self._search_forest[1: self.n_search_trees])
        else:
            self._vertex_order = np.arange(n)
        d.pop("_raw_data", None)  # (a mirror fetched before: the rows in their original order; the next read gathers them)
        d.pop("_lin_data", None)
        self._device_search_graph = (indptr, indices)
        self._device_prepare_stats = dict(ms, ms_search_graph=float(st["ms_device"]), final_nnz=int(nnz))
        self._searcher = None
        if self.compressed:  # pynndescent_.py:1653-1658
            d.pop("_rp_forest", None)
            d.pop("_neighbor_graph", None)
            d.pop("_device_graph", None)

    def prepare(self):
        """``NNDescent.prepare`` (pynndescent_.py:2174-2273): build everything a query needs.  quantization="uint8": the
        codebook is drawn on the host from the rows in their original order, the device quantizes the searcher's rows, and
        ``_quantized_data`` is kept on the host in the searcher's (tree) order, as the reference keeps it.  An index that
        already has them (unpickled) reuses ``_quantized_values`` / ``_quantized_data``."""
        _check_quantization(self.quantization, self.metric)
        quantized = self.quantization == "uint8"
        self._is_proxy_distance = quantized or _metric_of(self.metric).proxy
        d = self.__dict__
        fresh = not self._prepared
        if quantized and (fresh or d.get("_quantized_values") is None):
            if "_device_search_graph" in d or (fresh and _prepares_on_device(self)):  # the sample is gathered on the device
                raw = _DeviceRowsView(d["_device_data"])
            else:
                raw = self._raw_data if fresh else self._raw_data[np.argsort(self._vertex_order)]
            self._quantized_values = uint8_codebook(raw, self.random_state)
            self._quantized_data = None  # derived by the device below, in the searcher's order
        if fresh:
            self._init_search_graph()
        on_device = "_device_search_graph" in d and "_device_data" in d
        if d.get("_searcher") is None:
            tree = self._search_forest[0] if self._search_forest else None
            if on_device:
                self._searcher = self._searcher_from_device(tree)
            else:
                self._searcher = _capi.Searcher(self._work_rows(), self._search_graph, tree, _metric_of(self.metric).code,
                                                self._min_distance, self.n_neighbors, self.search_rng_state, device=self.device)
        if quantized and not self._searcher.has_codes:
            if d.get("_quantized_data") is None:
                # dot: the searcher's own copy is normalised once more on the device; the codes are those of _raw_data
                rows = self._raw_data if _metric_of(self.metric).normalize else None
                if on_device and rows is None:  # the codes stay with the searcher; _quantized_data is their mirror, fetched when read
                    self._searcher.quantize_u8(self._quantized_values, rows=None, fetch=False)
                    d.pop("_quantized_data", None)
                else:
                    self._quantized_data = self._searcher.quantize_u8(self._quantized_values, rows=rows)
            else:
                self._searcher.set_codes_u8(self._quantized_values, self._quantized_data)

    def _searcher_from_device(self, tree):
        """The searcher of a device-prepared index, filled on torch's current stream from the caller's tensor (its rows gathered by
        the leaf order straight into the searcher's layout), the reordered device graph and the host tree tables."""
        torch, d = _torch(), self.__dict__
        data, (indptr, indices), order = d["_device_data"], d["_device_search_graph"], d.get("_device_order")
        ordinal = int(self.device)
        with torch.cuda.device(ordinal):
            stream = _OnTorchStream(torch, ordinal)
            try:
                searcher, ms = _stream_ms(torch, stream, lambda: _capi.Searcher.from_device(
                    data.data_ptr(), _DEVICE_DTYPES[str(data.dtype).rsplit(".", 1)[-1]], data.shape[0], data.shape[1],
                    0 if order is None else order.data_ptr(), indptr.data_ptr(), indices.data_ptr() if indices.numel() else 0,
                    indices.numel(), tree, _metric_of(self.metric).code, self._min_distance, self.n_neighbors, self.search_rng_state,
                    device=ordinal, stream_ptr=stream.ptr))
                d.setdefault("_device_prepare_stats", {})["ms_searcher_fill"] = ms
            finally:
                stream.done()
        if order is not None:
            searcher.vertex_order_device = order  # what _query_device maps the answers' ids through
        return searcher

    def query(self, query_data, k=10, epsilon=0.1, proxy_beam_size=4):
        """``NNDescent.query`` (pynndescent_.py:2275-2379) on the GPU: one wave per query (csrc/query.hip).
        Returns (indices (n_queries, k) in the ORIGINAL numbering, true distances (n_queries, k)).  A device array
        ``query_data`` (float32 / float16 / bfloat16 / float64, on the index's device) is answered with device tensors: the
        queries are converted, the ids mapped back and the distances corrected on the device, on torch's current stream;
        the index may have been built from host or device data alike, and a host ``query_data`` returns numpy on both."""
        if k > 256:
            raise NotImplementedError("pynndescent_amd answers queries with k <= 256; use index.to_reference() for k = %d" % k)
        _check_quantization(self.quantization, self.metric)
        m = _metric_of(self.metric)
        search_k = k
        if self.quantization is not None or m.proxy:  # pynndescent_.py:2309-2312
            search_k = _proxy_search_k(k, proxy_beam_size)
        if (not self._prepared or getattr(self, "_searcher", None) is None
                or (self.quantization is not None and not self._searcher.has_codes)):
            self.prepare()
        if _is_device_array(query_data):
            return self._query_device(query_data, m, k, search_k, epsilon)
        query_data = np.asarray(query_data).astype(np.float32, order="C")  # pynndescent_.py:2316
        if query_data.ndim != 2 or query_data.shape[1] != self.dim:
            raise ValueError("query_data must have shape (n_queries, %d)" % self.dim)
        _raise_if_negative_host(query_data, m)
        lin = self.__dict__.get("_linear_map")
        if lin is not None:  # the queries through the index's own (A, c), by the kernel that transformed its rows
            query_data = _capi.linear_rows_host(lin.kind, lin.a, lin.shift, query_data, device=self.device)
        if self.quantization is not None:  # the walk on the codes, the rerank in its epilogue (pynndescent_.py:2321-2322, 2363-2371)
            indices, dists = self._searcher.query_proxy(query_data, k, search_k, epsilon + 1e-32)
        elif m.proxy:  # the walk on the proxy distance, the rerank by the true one; epsilon as given (pynndescent_.py:2321-2322)
            indices, dists = self._searcher.query_rerank(query_data, k, search_k, epsilon)
        else:
            indices, dists = self._searcher.query(query_data, k, epsilon)
        found = indices >= 0
        indices = np.where(found, self._vertex_order[np.where(found, indices, 0)], -1).astype(np.int32)  # pynndescent_.py:2373
        if self._distance_correction is not None:  # pynndescent_.py:2375-2376
            dists = self._distance_correction(dists)
        return indices, dists

    def _query_device(self, q, m, k, search_k, epsilon):
        """``query`` for a device array: the three forms on the device-pointer entries of the searcher."""
        torch = _torch()
        q, dtype, ordinal = _check_device_array(q, what="query_data")
        if ordinal != int(self.device):
            raise ValueError("query_data is on device %d, the index on device %d" % (ordinal, int(self.device)))
        nq, dim = int(q.shape[0]), int(self.dim)
        if q.shape[1] != dim:
            raise ValueError("query_data must have shape (n_queries, %d)" % dim)
        with torch.cuda.device(ordinal):
            stream = torch.cuda.current_stream(ordinal).cuda_stream
            if self.__dict__.get("_linear_map") is not None:  # converted, then through the index's own (A, c)
                q = self._linear_on_device(q.device).rows(q, dtype, stream)
            elif dtype != _capi.NND_DTYPE_FLOAT32:  # pynndescent_.py:2316
                q32 = torch.empty((nq, dim), dtype=torch.float32, device=q.device)
                _capi.device_rows_f32(ordinal, stream, q.data_ptr(), dtype, nq, dim, False, q32.data_ptr())
                q = q32
            if m.nonnegative and nq and bool((q.min() < 0).item()):
                raise ValueError(_NEGATIVE_HELLINGER)
            indices = torch.empty((nq, k), dtype=torch.int32, device=q.device)
            dists = torch.empty((nq, k), dtype=torch.float32, device=q.device)
            if self.quantization is not None:
                form, eps = "proxy", epsilon + 1e-32
            elif m.proxy:
                form, eps = "rerank", epsilon
            else:
                form, eps = "float", epsilon
            if nq:
                self._searcher.query_device(form, q.data_ptr(), nq, k, search_k, eps, indices.data_ptr(), dists.data_ptr(), stream)
            order = getattr(self._searcher, "vertex_order_device", None)  # lives and dies with the searcher
            if order is None:
                order = torch.from_numpy(np.ascontiguousarray(self._vertex_order, dtype=np.int32)).to(q.device)
                self._searcher.vertex_order_device = order
            found = indices >= 0
            indices = torch.where(found, order[indices.clamp(min=0).long()], torch.full_like(indices, -1))  # pynndescent_.py:2373
            if self._distance_correction is not None and m.device_kind != _capi.NND_CORRECT_COPY:  # pynndescent_.py:2375-2376
                dists = _device_corrected(torch, dists, m, ordinal)
        return indices, dists

    # ------------------------------------------------------------------------------------------------ pickling
    def __getstate__(self):
        """pynndescent_.py:1306-1320: a pickled index is a PREPARED index; device handles and the build forest stay behind."""
        if not self._prepared:
            self._init_search_graph()
        if "_device_data" in self.__dict__ or "_device_graph" in self.__dict__:  # the host mirrors travel, the tensors stay
            self._raw_data
            for name in ("_neighbor_graph", "_search_graph", "_quantized_data"):
                hasattr(self, name)
        state = self.__dict__.copy()
        for name in ("_device_graph", "_device_data", "_device_order", "_device_search_graph", "_device_prepare_stats"):
            state.pop(name, None)
        # a linear map travels as _linear_map (kind, A, c: float32); the transformed rows are derived again from _raw_data
        for name in ("_device_raw", "_device_linear", "_lin_data"):
            state.pop(name, None)
        state.pop("_rp_forest", None)
        state.pop("_searcher", None)
        state["_search_forest"] = tuple(tuple(t) for t in self._search_forest)  # rp_trees.py:3060-3069 denumbaify_tree
        return state

    def __setstate__(self, d):
        """pynndescent_.py:1322-1331: rebuild what cannot be pickled (here: the device copy, lazily on the first query)."""
        from .search_tree import FlatTree

        self.__dict__ = d
        self._distance_correction = _metric_of(self.metric).correction
        self._search_forest = [FlatTree(*t) for t in d["_search_forest"]]  # rp_trees.py:3072-3081 renumbaify_tree
        self._searcher = None

    def update(self, xs_fresh=None, xs_updated=None, updated_indices=None):
        """``pynndescent.NNDescent.update`` (pynndescent_.py:2381-2553) on the GPU: fresh rows are appended, updated
        rows replaced (their graph rows and every edge pointing at them are dropped), then the graph is rebuilt from
        a warm start -- the old graph inserted as "old" edges (init_from_neighbor_graph, flag 0), a forest of
        ``n_trees_after_update`` trees seeding "new" edges, no random fill -- and NN-descent runs to the stop rule.

        An index built from a device array on one GPU stays there when ``xs_fresh`` or ``xs_updated`` is a device array (a host
        array given alongside is uploaded): the new rows and the invalidated graph are assembled on the device
        (``_update_device``), ``neighbor_graph`` keeps returning tensors and a prepared index is prepared again on the device.
        With host arrays alone such an index becomes a host index, as before; a device array given to a host index, or to one
        built on several GPUs, is brought to the host.  ``updated_indices`` may be a tensor; the ids are read on the host."""
        on_device = _updates_on_device(self, xs_fresh, xs_updated)
        if not on_device:  # a tensor on an index that cannot stay on the device: its values, through the host path
            xs_fresh, xs_updated = _rows_to_host(xs_fresh), _rows_to_host(xs_updated)
        updated_indices = _ids_to_host(updated_indices)  # (a tensor of ids: they are few, and they stay a host list)

        def checked(rows, what):  # check_array; a device array of the device path: its validator, nothing is read
            if not _is_device_array(rows):
                return check_array(rows, dtype=self._input_dtype, order="C")
            rows, _, ordinal = _check_device_array(rows, what=what)
            if ordinal != int(self.device):
                raise ValueError("%s is on device %d, the index on device %d" % (what, ordinal, int(self.device)))
            if rows.shape[1] != self.dim:
                raise ValueError("%s must have shape (n_rows, %d), got %s" % (what, self.dim, tuple(rows.shape)))
            return rows

        current_random_state = check_random_state(self.random_state)
        # drawn and handed to make_forest by the reference (pynndescent_.py:2408-2411); kept for the stream position
        current_random_state.randint(INT32_MIN, INT32_MAX, 3)
        if xs_updated is not None:
            xs_updated = checked(xs_updated, "xs_updated")
            if updated_indices is None:
                raise ValueError("If xs_updated are provided, updated_indices must also be provided!")
            try:
                updated_indices = list(map(int, updated_indices))
            except (TypeError, ValueError):
                raise ValueError("Could not convert updated indices to list of int(s).")
            n1, n2 = len(updated_indices), xs_updated.shape[0]
            if n1 != n2:
                raise ValueError(
                    f"Number of updated indices ({n1}) must match " f"number of rows of xs_updated ({n2})."
                )
        else:
            if updated_indices is not None:
                warn("xs_updated not provided, while update_indices provided. " "They will be ignored.")
            updated_indices = None
        if on_device:
            return self._update_device(None if xs_fresh is None else checked(xs_fresh, "xs_fresh"), xs_updated, updated_indices or [],
                                       current_random_state)
        if updated_indices is None:
            xs_updated = np.zeros((0, self._raw_data.shape[1]), self._input_dtype)
            updated_indices = []
        if xs_fresh is None:
            xs_fresh = np.zeros((0, self._raw_data.shape[1]), dtype=self._input_dtype)
        else:
            xs_fresh = check_array(xs_fresh, dtype=self._input_dtype, order="C")

        # data and graph invalidation (pynndescent_.py:2461-2493), vectorised; a prepared index keeps its rows in the
        # search tree's leaf order: back to the original order first (pynndescent_.py:2462-2465, 2476)
        raw = np.array(self._raw_data, copy=True)
        if hasattr(self, "_vertex_order"):
            raw = raw[np.argsort(self._vertex_order), :]
        for x_updated, i_fresh in zip(xs_updated, updated_indices):
            raw[i_fresh] = x_updated
        n_old = raw.shape[0]
        raw = np.ascontiguousarray(np.vstack([raw, xs_fresh]))
        ns, ds = (np.array(a, copy=True) for a in self._neighbor_graph)
        self._drop_device_copies()  # (an index built from a device array: from here on its host arrays are the index)
        if updated_indices:
            hit = np.zeros(n_old, bool)
            hit[updated_indices] = True
            ns[hit] = -1
            ds[hit] = np.inf
            stale = (ns >= 0) & hit[np.clip(ns, 0, None)]
            ns[stale] = -1
            ds[stale] = np.inf
        n = raw.shape[0]
        pad_i = np.full((n, ns.shape[1]), -1, np.int32)
        pad_d = np.full((n, ns.shape[1]), np.inf, np.float32)
        pad_i[:n_old] = ns
        pad_d[:n_old] = ds

        self.n_trees = self.n_trees_after_update  # pynndescent_.py:2498
        _, _, eff_leaf_size, eff_max_candidates = _reference_defaults(n, self.n_neighbors, self.n_trees, self.n_iters,
                                                                      self.leaf_size, self.max_candidates)
        tree_states = current_random_state.randint(INT32_MIN, INT32_MAX, size=(self.n_trees, 3)).astype(np.int64)
        if getattr(self, "n_devices", 1) > 1:  # the rebuild is sharded like the build was (nnd_build_multi_update)
            n_leaves = self._build_multi(raw, self.n_trees, eff_leaf_size, eff_max_candidates, tree_states[0], False,
                                         old_graph=(pad_i, pad_d))
        else:  # pynndescent_.py:2512-2517: the old graph's entries as "old" edges, then the forest's; no random fill
            lin, work = self.__dict__.get("_linear_map"), raw
            self.__dict__.pop("_lin_data", None)
            if lin is not None:  # old, updated and fresh rows through the index's own (A, c): old rows come out as they were
                work = self._lin_data = _capi.linear_rows_host(lin.kind, lin.a, lin.shift, raw, device=self.device)
            self._neighbor_graph, self._build_stats, n_leaves = _build_graph(
                work, _metric_of(self.metric), self.n_neighbors, self.n_trees, eff_leaf_size, self.max_rptree_depth,
                eff_max_candidates, self.n_iters, self.delta, self.rng_state, tree_states[0], self.device, forest=True,
                old_graph=(pad_i, pad_d), verbose=self.verbose)
        self._rp_forest = _DeviceForestSentinel(self.n_trees, n_leaves, eff_leaf_size)
        self._raw_data = raw
        if self._prepared:  # pynndescent_.py:2538-2553: the derived structures are rebuilt
            for name in ("_search_graph", "_search_forest", "_vertex_order", "_searcher"):
                self.__dict__.pop(name, None)
            self.prepare()


    def _update_device(self, xs_fresh, xs_updated, updated_indices, current_random_state):
        """``update`` of an index that holds its rows and its graph on the device, entry for entry what the host path computes
        from the mirrors -- on torch's current stream (``_OnTorchStream``), with no host leg: the new ``(n_old + n_fresh, d)``
        tensor (old rows, fresh rows, updated rows scattered to their ids; the dtype all arrays share, else float32) and the
        invalidated, padded graph are written by the library (``nnd_device_update_rows`` / ``nnd_device_update_graph``), the
        rebuild binds the new rows as they are (dot: not normalised again, as on the host path) and reads the old graph in place.
        What crosses the bus: the resolved ``(row id, source row)`` pairs, host arrays given alongside, and the build's scalars."""
        d, m = self.__dict__, _metric_of(self.metric)
        # (a metric with a linear map: the new tensor is assembled from the caller's rows, and transformed as a whole below)
        data, (gidx, gdist) = d.get("_device_raw", d["_device_data"]), d["_device_graph"]
        linear = self._linear_on_device(data.device) if d.get("_linear_map") is not None else None
        n_old, dim, k, ordinal = int(data.shape[0]), int(data.shape[1]), int(gidx.shape[1]), int(self.device)
        ids, sources = _resolve_updated_indices(updated_indices, n_old)  # (IndexError: before any device work)
        torch = _torch()
        n_fresh = 0 if xs_fresh is None else int(xs_fresh.shape[0])
        n = n_old + n_fresh
        n_trees = self.n_trees_after_update  # pynndescent_.py:2498 (assigned with the new tensors: a rebuild that raises changes nothing)
        _, _, eff_leaf_size, eff_max_candidates = _reference_defaults(n, self.n_neighbors, n_trees, self.n_iters,
                                                                      self.leaf_size, self.max_candidates)
        tree_states = current_random_state.randint(INT32_MIN, INT32_MAX, size=(n_trees, 3)).astype(np.int64)
        with torch.cuda.device(ordinal):
            def on_device(rows):  # a host array given alongside goes up (float32: what check_array made of it)
                return rows if rows is None or _is_device_array(rows) else torch.from_numpy(rows).to(data.device)

            def described(rows):  # (address, NND_DTYPE_*, rows) of an array that may be absent
                return (0, 0, 0) if rows is None or rows.shape[0] == 0 else (rows.data_ptr(), _DEVICE_DTYPES[_dtype_name(rows)], rows.shape[0])

            xs_fresh, xs_updated = on_device(xs_fresh), on_device(xs_updated)
            out_name = _update_dtype([_dtype_name(data)] + [_dtype_name(a) for a in (xs_fresh, xs_updated) if a is not None])
            new_data = torch.empty((n, dim), dtype=getattr(torch, out_name), device=data.device)
            pad_i = torch.empty((n, k), dtype=torch.int32, device=data.device)
            pad_d = torch.empty((n, k), dtype=torch.float32, device=data.device)
            updated_map = torch.empty((n_old,), dtype=torch.uint8, device=data.device)
            pairs = torch.from_numpy(np.stack([ids, sources])).to(data.device) if ids.shape[0] else None
            stream = _OnTorchStream(torch, ordinal)  # (made after the uploads: a side stream waits for them)
            try:
                ids_ptr, sources_ptr = (pairs[0].data_ptr(), pairs[1].data_ptr()) if pairs is not None else (0, 0)
                _capi.device_update_rows(ordinal, stream.ptr, dim, described(data), described(xs_fresh), described(xs_updated),
                                         (sources_ptr, ids_ptr, ids.shape[0]), new_data.data_ptr(), _DEVICE_DTYPES[out_name])
                _capi.device_update_graph(ordinal, stream.ptr, gidx.data_ptr(), gdist.data_ptr(), n_old, k, ids_ptr, ids.shape[0], n,
                                          updated_map.data_ptr(), pad_i.data_ptr(), pad_d.data_ptr())
            finally:
                stream.done()
            # pynndescent_.py:2512-2517: the old graph's entries as "old" edges, then the forest's; no random fill
            dev_in = _DeviceInput(new_data, _DEVICE_DTYPES[out_name], ordinal, self.n_neighbors, as_given=True, linear=linear)
            graph, build_stats, n_leaves = _build_graph(
                new_data, m, self.n_neighbors, n_trees, eff_leaf_size, self.max_rptree_depth, eff_max_candidates, self.n_iters,
                self.delta, self.rng_state, tree_states[0], ordinal, forest=True, old_graph=(pad_i, pad_d), check_finite=True,
                verbose=self.verbose, dev_in=dev_in)
        self.n_trees, self._build_stats = n_trees, build_stats
        self._rp_forest = _DeviceForestSentinel(n_trees, n_leaves, eff_leaf_size)
        was_prepared = self._prepared
        for name in ("_device_order", "_device_search_graph", "_device_prepare_stats", "_raw_data", "_lin_data", "_neighbor_graph",
                     "_search_graph", "_quantized_data", "_searcher", "_search_forest", "_vertex_order"):
            d.pop(name, None)
        self._device_data, self._device_graph = dev_in.rows, graph  # (the caller's original tensor is released)
        if linear is not None:
            self._device_raw = new_data
        if was_prepared:  # pynndescent_.py:2538-2553: the derived structures are rebuilt, from the tensors when _prepares_on_device
            self.prepare()


# from_graph's keywords and their defaults: the constructor's, minus what the graph fixes (the data, n_neighbors, the metric
# and random_state are arguments of their own; the build's seeding and its devices do not apply)
_FROM_GRAPH_DEFAULTS = {
    ("prune_degree_multiplier" if name == "pruning_degree_multiplier" else name): p.default
    for name, p in inspect.signature(NNDescent.__init__).parameters.items()
    if name not in ("self", "data", "metric", "n_neighbors", "random_state", "tree_init", "init_graph", "init_dist",
                    "n_devices", "devices")
}

EMPTY_GRAPH = (np.array([[-1]], dtype=np.int32), np.array([[np.inf]], dtype=np.float32),
               np.array([[0]], dtype=np.uint8))  # pynndescent_.py:64-68

# the reference's functions of the kernels' own spaces (pynndescent_.py:1247-1260) -> the metric whose kernels they name
_ND_ALIASES = {"squared_euclidean": "sqeuclidean", "alternative_cosine": "cosine", "alternative_dot": "dot",
               "alternative_inner_product": "inner_product", "alternative_hellinger": "hellinger"}
# distance arguments nn_descent understands: name (or __name__ of the reference's function) -> (kernel metric, correction);
# the eight metrics give true distances (the same kernels, corrected on return), the aliases none (a copy is no correction:
# nn_descent returns the finished arrays themselves)
_ND_DISTS = {name: (m.code, None if m.correction is _capi.host_copy else m.correction) for name, m in _METRICS.items()}
_ND_DISTS.update((alt, (_METRICS[name].code, None)) for alt, name in _ND_ALIASES.items())
# the boolean family: the nine names (jaccard: corrected on return), and "alternative_jaccard" for its kernel distance
_ND_ALIASES["alternative_jaccard"] = "jaccard"
_ND_DISTS.update((name, (m.code, None if m.correction is _capi.host_copy else m.correction)) for name, m in _BOOLEAN_METRICS.items())
_ND_DISTS["alternative_jaccard"] = (_BOOLEAN_METRICS["jaccard"].code, None)


def nn_descent(data, n_neighbors, rng_state, max_candidates=50, dist="squared_euclidean", n_iters=10, delta=0.001,
               init_graph=EMPTY_GRAPH, rp_tree_init=True, leaf_array=None, low_memory=True, verbose=False, device=0):
    """The reference's ``nn_descent`` (pynndescent_.py:323-366) with the same arguments, on the GPU: the seam a caller
    uses who keeps the reference's ``make_forest`` / ``rptree_leaf_array`` and hands the leaves in.

    data float32 (n, d); rng_state int64[3]; ``dist``: "squared_euclidean" / "alternative_cosine" / "alternative_dot" /
    "alternative_inner_product" / "correlation" / "alternative_hellinger" (what NNDescent passes, pynndescent_.py:1247-1260),
    "euclidean" / "cosine" / "dot" / "inner_product" / "hellinger" (true distances: the same kernels, corrected on return),
    "proxy_inner_product" (the proxy distances themselves: it has no correction), the boolean metrics "jaccard" (corrected
    on return; "alternative_jaccard": its kernel distance) / "dice" / "sokalsneath" / "matching" / "rogerstanimoto" /
    "sokalmichener" / "kulsinski" / "russellrao" / "yule",
    or the reference function of one of those names (dot: the kernels rank by the L2-normalised rows, as NNDescent's
    normalised data gives; hand in normalised rows for the reference's ranking); ``init_graph``: EMPTY_GRAPH, or the heap triple ``(indices (n, k),
    distances (n, k), flags (n, k))`` the reference accepts (entries with index -1 are empty); ``leaf_array`` int32
    (n_leaves, max_leaf_size), -1 padded, used when ``rp_tree_init``.  ``low_memory`` is accepted and unused, as in the
    reference (pynndescent_.py:335).  Returns ``(indices int32 (n, k), distances float32 (n, k))``, rows ascending."""
    name = dist if isinstance(dist, str) else getattr(dist, "__name__", None)
    if name not in _ND_DISTS:
        raise NotImplementedError("pynndescent_amd.nn_descent: dist must be one of %s (got %r)" % (sorted(_ND_DISTS), dist))
    m, correction = _metric_of(_ND_ALIASES.get(name, name)), _ND_DISTS[name][1]
    data = np.ascontiguousarray(data, dtype=np.float32)
    n = data.shape[0]
    _check_supported_sizes(n_neighbors, max_candidates, None)
    empty = init_graph[0].shape[0] == 1  # EMPTY_GRAPH
    if not empty and not (init_graph[0].shape[0] == n and init_graph[0].shape[1] == n_neighbors):
        raise ValueError("Invalid initial graph specified!")  # pynndescent_.py:352
    if empty and rp_tree_init and leaf_array is None:
        raise ValueError("rp_tree_init=True needs a leaf_array (rptree_leaf_array of a forest)")
    leaf_size = _reference_defaults(n, n_neighbors, 0, n_iters, None, max_candidates)[2]
    # (a heap handed over: its entries, with their distances; flags restart as "new": they were never sampled here)
    (idx, dst), _, _ = _build_graph(
        data, m, n_neighbors, 0, leaf_size, 200, max_candidates, n_iters, delta, np.asarray(rng_state, np.int64),
        np.zeros(3, np.int64), device, leaf_array=leaf_array if empty and rp_tree_init else None,
        init_graph=None if empty else np.asarray(init_graph[0], np.int32),
        init_dist=None if empty else np.asarray(init_graph[1], np.float32), random_fill=empty, stats=False, verbose=verbose)
    if correction is not None:
        dst = correction(dst).astype(np.float32)
    return idx, dst


def _exact_linear_rows(metric, m, metric_kwds, data, queries, device):
    """``exact_knn`` of a metric with a linear map: ``(data, queries)`` transformed by the device (float32; tensors stay tensors),
    on which the search is euclidean.  The shift is the one an index of ``data`` would fix; distances do not depend on it."""
    if _is_device_array(data):
        data, dtype, ordinal = _check_device_array(data, device)
        lin = _linear_map_of(metric, m, metric_kwds, data.shape[1])
        if lin is None:
            return data, queries
        torch = _torch()
        with torch.cuda.device(ordinal):
            dl = _DeviceLinear(lin._replace(shift=linear_map.shift_of(_DeviceRowsView(data))), data.device, ordinal)
            stream = torch.cuda.current_stream(ordinal).cuda_stream
            if queries is not None:
                if _is_device_array(queries):
                    queries, q_dtype, _ = _check_device_array(queries, what="queries")
                    queries = queries.to(data.device)
                else:
                    queries, q_dtype = torch.from_numpy(_check_array_no_scan(queries)).to(data.device), _capi.NND_DTYPE_FLOAT32
                if queries.shape[1] != data.shape[1]:
                    raise ValueError("queries must have shape (n_queries, %d)" % data.shape[1])
                queries = dl.rows(queries, q_dtype, stream)
            return dl.rows(data, dtype, stream), queries
    data = _check_array_no_scan(data)
    lin = _linear_map_of(metric, m, metric_kwds, data.shape[1])
    if lin is None:
        return data, queries
    lin = lin._replace(shift=linear_map.shift_of(data))
    if queries is not None:
        queries = _check_array_no_scan(_rows_to_host(queries))
        if queries.shape[1] != data.shape[1]:
            raise ValueError("queries must have shape (n_queries, %d)" % data.shape[1])
        queries = _capi.linear_rows_host(lin.kind, lin.a, lin.shift, queries, device=device)
    return _capi.linear_rows_host(lin.kind, lin.a, lin.shift, data, device=device), queries


def exact_knn(data, queries=None, k=10, metric="euclidean", rows=None, device=0, return_stats=False, metric_kwds=None):
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
    the euclidean one."""
    if queries is not None and rows is not None:
        raise ValueError("exact_knn takes `queries` (external points) or `rows` (ids of data rows), not both")
    k = int(k)
    if k > 256:
        raise NotImplementedError("pynndescent_amd.exact_knn keeps at most k <= 256 neighbours per row (got k = %d)" % k)
    m = _metric_record(metric)
    _no_exact_for_proxy(metric, m, "exact_knn")
    if m.linear:  # (metric_kwds is validated in there, before any device work)
        data, queries = _exact_linear_rows(metric, m, metric_kwds, data, queries, device)
        metric, m = "euclidean", _METRICS["euclidean"]
    if _is_device_array(data):
        return _exact_knn_device(data, queries, k, metric, m, rows, device, return_stats)
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
        if queries is not None:
            idx, dist, stats = builder.exact_knn_queries(queries, k)
        else:
            idx, dist, stats = builder.exact_knn(rows, k)
    finally:
        builder.close()
    dist = m.correction(dist)
    return (idx, dist, stats) if return_stats else (idx, dist)


def _exact_knn_device(data, queries, k, metric, m, rows, device, return_stats):
    """``exact_knn`` for a device array ``data`` (``k``, the metric and queries-or-rows are checked already): an auxiliary handle
    bound to the tensor on torch's current stream, the device entries of csrc/exact.hip, the answers corrected on the device.
    ``rows``: a host array or a tensor of ids (range-checked on the host), or an int32 tensor on the data's device that the
    caller has checked (``NNDescent._recall_device``).  What crosses the bus: the row ids, host queries, and scalars."""
    data, dtype, ordinal = _check_device_array(data, device)
    n, dim = int(data.shape[0]), int(data.shape[1])
    if k < 1 or k > n:
        raise ValueError("k must be in 1 .. n = %d (got %d)" % (n, k))
    torch = _torch()
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
                stats = builder.exact_knn_device(k, idx.data_ptr(), dist.data_ptr(), q_ptr=q.data_ptr(), q_dtype=q_dtype, n_q=n_out)
            else:
                stats = builder.exact_knn_device(k, idx.data_ptr(), dist.data_ptr(), rows_ptr=0 if rows_dev is None else rows_dev.data_ptr(),
                                                 n_rows=n_out)
        finally:
            builder.close()
            stream.done()
        dist = _device_corrected(torch, dist, m, ordinal)
    return (idx, dist, stats) if return_stats else (idx, dist)


def _build_graph(data, m, n_neighbors, n_trees, leaf_size, max_depth, max_candidates, n_iters, delta, rng_state, tree_rng,
                 device, forest=False, leaf_array=None, init_graph=None, init_dist=None, old_graph=None, random_fill=False,
                 check_finite=False, stats=True, verbose=False, announce=False, dev_in=None):
    """Every single-GPU build (``_capi.Builder``): the data in, its flags read (the NaN / inf one only when
    ``check_finite``), ``forest`` built on the device, the graph seeded -- ``old_graph`` (ids, distances) as "old" edges,
    then ``init_graph`` / ``init_dist``, the caller's ``leaf_array`` or the forest's leaves, then the random fill when
    ``random_fill`` -- NN-descent to the stop rule, the graph out.  ``announce``: the constructor's verbose line.  ``dev_in``
    (a ``_DeviceInput``): the rows are a device array, read in place on torch's stream, and the graph comes out as tensors;
    ``old_graph`` and ``init_graph`` / ``init_dist`` may then be tensors as well (int32 / float32, read in place).  Returns
    ``((indices, distances), the stats (when ``stats``), the forest's leaf count)``."""
    n = data.shape[0]
    builder = _capi.Builder(n, data.shape[1], m.code, n_neighbors, n_trees, leaf_size, max_depth, max_candidates, n_iters,
                            delta, rng_state, tree_rng, device=device)
    try:
        if dev_in is None:
            builder.set_data_host(data)
        else:
            dev_in.set_data(builder, m)
        if check_finite:
            _raise_if_nonfinite(builder, data if dev_in is None else dev_in.host_rows)
        if m.nonnegative and builder.data_negative():
            raise ValueError(_NEGATIVE_HELLINGER)
        n_leaves = None
        if forest:
            builder.make_forest()
            n_leaves = builder.stats()["n_leaves"]
        if announce:
            print(ts(), "NN descent for", str(n_iters), "iterations")
        if old_graph is not None:
            builder.reset_graph()
            if _is_device_array(old_graph[0]):  # (update() of a device-built index: the invalidated graph is a pair of tensors)
                builder.init_from_neighbor_graph_device(old_graph[0].data_ptr(), old_graph[1].data_ptr(), old_graph[0].shape[1])
            else:
                builder.init_from_neighbor_graph(*old_graph)
        if init_graph is not None and _is_device_array(init_graph):  # int32 / float32, contiguous, on the data's device
            builder.init_from_graph_device(init_graph.data_ptr(), 0 if init_dist is None else init_dist.data_ptr(), init_graph.shape[1])
        elif init_graph is not None:
            builder.init_from_graph(init_graph, init_dist)
        elif leaf_array is not None:
            builder.init_from_leaf_array(leaf_array)
        elif forest:
            builder.init_from_leaves()
        if random_fill:
            builder.init_random()
        _descend(builder, n, n_neighbors, n_iters, delta, verbose)
        graph = builder.finalize() if dev_in is None else dev_in.finalize(builder)
        return graph, builder.stats() if stats else None, n_leaves
    finally:
        builder.close()
        if dev_in is not None:
            dev_in.close()


def _descend(builder, n, n_neighbors, n_iters, delta, verbose):
    """nn_descent_internal (pynndescent_.py:296-320): the library's loop (nnd_descent, no host round trip per iteration),
    or with ``verbose`` the same iterations and stop rule driven from here, so that the output matches the reference's."""
    if not verbose:
        builder.descent()
        return
    for it in range(n_iters):
        print("\t", it + 1, " / ", n_iters)
        c = builder.descent_iter()
        if c <= delta * n_neighbors * n:
            print("\tStopping threshold met -- exiting after", it + 1, "iterations")
            break


def _check_array_no_scan(data):
    try:
        return check_array(data, dtype=np.float32, order="C", ensure_all_finite=False)
    except TypeError:  # scikit-learn < 1.6
        return check_array(data, dtype=np.float32, order="C", force_all_finite=False)


def _raise_if_nonfinite(builder, data):
    """The ValueError check_array raises in the reference for NaN / inf input (pynndescent_.py:1054), from the device flag."""
    if builder.data_nonfinite():
        from sklearn.utils import assert_all_finite

        if callable(data):  # a device array: only this error path brings the rows to the host, for sklearn's wording
            data = data()
        assert_all_finite(data)  # raises "Input contains NaN." / "... infinity or a value too large ..."
        raise ValueError("Input contains NaN or infinity.")  # (unreachable unless the two scans disagree)


# hellinger takes sqrt(x): the reference computes NaN distances from a negative entry without a word; here it is an error
_NEGATIVE_HELLINGER = "the hellinger metric needs non-negative input: the data holds a negative entry"


def _raise_if_negative_host(data, m):
    if m.nonnegative and data.size and data.min() < 0:
        raise ValueError(_NEGATIVE_HELLINGER)


def _check_supported_sizes(n_neighbors, max_candidates, init_graph):
    """The GPU k-lists hold at most 256 entries (four per lane of a wave; rows above 64 take the LDS-merge kernels) and the
    candidate lists at most 128 (above 64: five passes of the 64-slot join over blocks of the lists); the reference has no such bounds (pynndescent_.py:976-982), so the limits are reported up
    front and by name."""
    if int(n_neighbors) > 256 or (max_candidates is not None and int(max_candidates) > 128):
        raise NotImplementedError(
            "pynndescent_amd supports n_neighbors <= 256 and max_candidates <= 128 (got n_neighbors=%s, max_candidates=%s); "
            "use pynndescent.NNDescent (or pynndescent_amd.make_index) for wider graphs" % (n_neighbors, max_candidates))
    if init_graph is not None and len(_shape_of(init_graph)) == 2 and _shape_of(init_graph)[1] > 256:
        raise NotImplementedError("pynndescent_amd supports init_graph with at most 256 columns (got %d); use "
                                  "pynndescent.NNDescent" % _shape_of(init_graph)[1])


def make_index(data, *args, **kwargs):
    """``NNDescent(data, ...)`` on the GPU when the input is in scope (dense data, euclidean / l2 / sqeuclidean / cosine / dot /
    inner_product / correlation / hellinger / proxy_inner_product / seuclidean / mahalanobis / minkowski and wminkowski with p = 2 /
    the boolean metrics jaccard, dice, sokalsneath, matching, rogerstanimoto, sokalmichener, kulsinski, russellrao and yule,
    k <= 256);
    otherwise -- and only then -- the reference ``pynndescent.NNDescent`` on the CPU when that package is importable
    (SURVEY.md section 8b), with a warning.  A missing HIP library or GPU is never papered over: that still raises."""
    device = kwargs.pop("device", 0)
    try:
        return NNDescent(data, *args, device=device, **kwargs)
    except NotImplementedError as exc:
        try:
            import pynndescent
        except ImportError:
            raise exc
        warn("pynndescent_amd: %s -- building with pynndescent.NNDescent on the CPU instead" % exc)
        return pynndescent.NNDescent(data, *args, **kwargs)


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
