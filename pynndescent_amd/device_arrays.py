"""Device arrays: input that lives on the GPU (in practice a torch.Tensor on a HIP device), and the plumbing between torch's
tensors and streams and the library's device-pointer entries.

torch is imported by ``_torch()`` alone, on the paths that meet a tensor: importing this module does not import it.
"""
import numpy as np

from . import _capi, row_map

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


def _assert_all_finite(a):
    """sklearn's ``assert_all_finite`` (the reference's ``check_array`` scan) for host rows or a device array; of a device array
    one scalar comes back, and only the error path brings the rows down, for sklearn's wording."""
    from sklearn.utils import assert_all_finite

    if not _is_device_array(a):
        assert_all_finite(a)
    elif a.shape[0] and not bool(_torch().isfinite(a).all().item()):
        assert_all_finite(_rows_to_host(a))


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
        self.linear = linear  # a _DeviceLinear or a _DeviceRowMap: the metric's map on this device (None: the metric has none)

    def work_dim(self):
        """The width of the rows the device works on: the tensor's, or what the metric's map makes of it."""
        dim = int(self.tensor.shape[1])
        return dim if self.linear is None else self.linear.out_dim(dim)

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

    def out_dim(self, dim):
        return int(dim)

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


class _DeviceRowMap:
    """A derived metric's row map (``row_map.RowMap``) on one device, with the interface of ``_DeviceLinear``: the sphere's shift
    as a float32 tensor there (uploaded here, on torch's current stream); the ranks have nothing to upload."""

    def __init__(self, m, device, ordinal):
        self.kind, self.ordinal = int(m.kind), int(ordinal)
        self.shift = None if m.shift is None else _torch().from_numpy(np.ascontiguousarray(m.shift, dtype=np.float32)).to(device)

    def out_dim(self, dim):
        return _capi.rowmap_out_dim(self.kind, dim)

    def rows(self, t, dtype, stream_ptr):
        """The map of the contiguous (n, d) tensor ``t`` (``dtype``: its NND_DTYPE_*): a new float32 tensor of the map's output
        width, queued on ``stream_ptr``.  The existing conversion to float32 runs first (csrc/devarray.hip), then csrc/rowmap.hip."""
        torch = _torch()
        n, dim = int(t.shape[0]), int(t.shape[1])
        out = torch.empty((n, _capi.rowmap_out_dim(self.kind, dim)), dtype=torch.float32, device=t.device)
        if n == 0:
            return out
        if dtype != _capi.NND_DTYPE_FLOAT32:
            x32 = torch.empty((n, dim), dtype=torch.float32, device=t.device)
            _capi.device_rows_f32(self.ordinal, stream_ptr, t.data_ptr(), dtype, n, dim, False, x32.data_ptr())
            t = x32
        _capi.device_map_rows(self.ordinal, stream_ptr, self.kind, dim, dim, 0 if self.shift is None else self.shift.data_ptr(),
                              t.data_ptr(), n, out.data_ptr())
        return out


def _device_map(m, device, ordinal):
    """``m`` -- an index's ``LinearMap`` or ``RowMap`` -- on ``device``: the object whose ``rows()`` maps a tensor there."""
    return (_DeviceRowMap if isinstance(m, row_map.RowMap) else _DeviceLinear)(m, device, ordinal)


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
