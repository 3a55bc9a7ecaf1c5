"""Sparse input: ``scipy.sparse`` matrices as data, queries and update rows ("Sparse input").

A sparse matrix goes up the bus as its three CSR arrays -- 8 bytes per stored entry instead of 4 bytes per element -- and one
kernel (csrc/sparse.hip, ``nnd_device_csr_rows``) writes its dense float32 rows where the device-array path expects a tensor.
From there the index is a device-resident index: build, ``update()``, ``prepare()``, ``query()``, ``recall()`` and ``exact_knn``
run on the tensor as they do for a caller's own, unchanged.  What the host keeps is the canonical CSR matrix (``_raw_data``, as
the reference keeps it), never a dense mirror.

A stored entry is a VALUE, as in ``toarray()``: an explicitly stored zero is a zero.  (The reference's sparse boolean distances
count the stored entries of a row, so there a stored zero is "present".)

Host only up to ``dense_rows_on_device``: importing this module imports neither torch nor the library.
"""
import numpy as np

from . import _capi, device_arrays

# names of the project's metric table, and its derived metrics, that the reference's sparse path does not have (sparse.py
# sparse_named_distances): the reference refuses them for sparse data with a ValueError, and so does this path, with the same
# words (pynndescent_.py:1122)
SPARSE_REFUSED_METRICS = frozenset(("dot", "inner_product", "proxy_inner_product", "yule", "seuclidean", "standardised_euclidean",
                                    "wminkowski", "weighted_minkowski", "mahalanobis", "spearmanr", "haversine"))


def is_sparse(a):
    """Whether ``a`` is a ``scipy.sparse`` matrix or array (False when scipy is not there: nothing can be one then)."""
    if a is None or isinstance(a, np.ndarray):
        return False
    try:
        import scipy.sparse
    except ImportError:  # pragma: no cover
        return False
    return scipy.sparse.issparse(a)


def check_sparse_metric(metric, n_devices=1):
    """The metric rule of sparse input, for a name ``_metric_record`` has accepted: the reference's ValueError for a name its sparse
    path lacks, and one GPU only (the row-sharded build reads host rows)."""
    if metric in SPARSE_REFUSED_METRICS:
        raise ValueError("Metric {} not supported for sparse data".format(metric))
    if int(n_devices) > 1:
        raise NotImplementedError("pynndescent_amd builds sparse input on one GPU (n_devices = %d): the row-sharded build reads "
                                  "host rows; use n_devices=1, or pynndescent.NNDescent" % int(n_devices))


def canonical_csr(a):
    """``a`` as a canonical float32 CSR matrix: ``check_array(accept_sparse="csr", dtype=np.float32)`` (pynndescent_.py:1054)
    without its scan for NaN / inf (the device's prep kernel flags them), then column indices ascending within a row and no
    duplicates.  A copy is made only where something changes, and the caller's object is never modified; explicitly stored
    zeros stay stored.  The index arrays keep the width scipy gave them (int32 or int64): the kernel reads both."""
    from sklearn.utils import check_array

    try:
        out = check_array(a, accept_sparse="csr", dtype=np.float32, ensure_all_finite=False)
    except TypeError:  # (scikit-learn before 1.6 spells it force_all_finite)
        out = check_array(a, accept_sparse="csr", dtype=np.float32, force_all_finite=False)
    if not out.has_canonical_format:
        shared = out is a or any(np.shares_memory(getattr(out, name), getattr(a, name))
                                 for name in ("indptr", "indices", "data") if isinstance(getattr(a, name, None), np.ndarray))
        if shared:  # (check_array converts without a copy where it can)
            out = out.copy()
        out.sum_duplicates()  # (sorts the indices first)
    return out


def dense_bytes(n, dim):
    """``(tensor, prepared)``: the bytes of the dense float32 rows and of the handle's prepared copy of them (rows padded to a
    multiple of 32 floats, csrc/plan.h) -- what a build needs for the rows alone."""
    n, dim = int(n), int(dim)
    return 4 * n * dim, 4 * n * ((dim + 31) & ~31)


def check_dense_fits(n, dim, free_bytes):
    """The size rule: ``NotImplementedError`` when the dense rows alone -- the float32 tensor plus the handle's prepared copy --
    need more than ``free_bytes`` of device memory.  The message names the reference's entry point, so that ``make_index`` hands
    the build to it.  Returns the two byte counts."""
    tensor, prepared = dense_bytes(n, dim)
    if tensor + prepared > int(free_bytes):
        raise NotImplementedError(
            "sparse input is made dense on the device: the %d x %d float32 rows (%d bytes) and the build's prepared copy of them "
            "(%d bytes) do not fit the %d bytes of free device memory; use pynndescent.NNDescent (sparse_nndescent)"
            % (int(n), int(dim), tensor, prepared, int(free_bytes)))
    return tensor, prepared


def dense_rows_on_device(csr, device, check_fit=False):
    """The canonical CSR matrix ``csr`` as a dense float32 tensor on the GPU ``device``: the three arrays are uploaded as they are
    and ``nnd_device_csr_rows`` writes the rows, on torch's current stream; nothing is waited for.  ``check_fit``: the size rule
    first, against the free device memory at this call; a missing torch raises the same error."""
    n, dim = (int(v) for v in csr.shape)
    ordinal = int(device)
    try:
        torch = device_arrays._torch()
    except ImportError:
        raise NotImplementedError(
            "sparse input is made dense on the device through torch, which cannot be imported: the %d x %d float32 rows "
            "(%d bytes) and the build's prepared copy (%d bytes) have nowhere to go; use pynndescent.NNDescent (sparse_nndescent)"
            % ((n, dim) + dense_bytes(n, dim)))
    with torch.cuda.device(ordinal):
        where = torch.device("cuda", ordinal)
        if check_fit:
            check_dense_fits(n, dim, torch.cuda.mem_get_info(ordinal)[0])
        out = torch.empty((n, dim), dtype=torch.float32, device=where)
        if n == 0 or dim == 0:
            return out
        indptr = torch.from_numpy(np.ascontiguousarray(csr.indptr)).to(where)
        indices = torch.from_numpy(np.ascontiguousarray(csr.indices)).to(where)
        values = torch.from_numpy(np.ascontiguousarray(csr.data, dtype=np.float32)).to(where)
        _capi.device_csr_rows(ordinal, torch.cuda.current_stream(ordinal).cuda_stream, indptr.data_ptr(), csr.indptr.dtype.itemsize,
                              indices.data_ptr() if indices.numel() else 0, csr.indices.dtype.itemsize,
                              values.data_ptr() if values.numel() else 0, n, dim, out.data_ptr())
        # (the three arrays are freed when this returns: torch's allocator keeps their blocks for the stream that used them)
    return out


def query_rows(query_data, dim, device, what="query_data"):
    """A sparse query batch, checked against the index's ``dim`` before any device work, as a float32 tensor on ``device``."""
    if len(query_data.shape) != 2 or query_data.shape[1] != dim:
        raise ValueError("%s must have shape (n_queries, %d)" % (what, dim))
    return dense_rows_on_device(canonical_csr(query_data), device)


def updated_csr(raw, xs_updated, ids, sources, xs_fresh):
    """``update()`` on the CSR matrix: ``raw`` (in the original row order) with the rows ``ids`` replaced by the rows ``sources`` of
    ``xs_updated`` (the resolved pairs of ``_resolve_updated_indices``) and ``xs_fresh`` appended (pynndescent_.py:2461-2476).
    One row selection of the stacked blocks: work proportional to the stored entries."""
    import scipy.sparse as sp

    n_old = raw.shape[0]
    blocks, select = [raw], np.arange(n_old, dtype=np.int64)
    if xs_updated is not None and len(ids):
        blocks.append(xs_updated)
        select[np.asarray(ids, dtype=np.int64)] = n_old + np.asarray(sources, dtype=np.int64)
    if xs_fresh is not None and xs_fresh.shape[0]:
        first = sum(b.shape[0] for b in blocks)
        blocks.append(xs_fresh)
        select = np.concatenate([select, first + np.arange(xs_fresh.shape[0], dtype=np.int64)])
    stacked = sp.vstack(blocks, format="csr", dtype=np.float32) if len(blocks) > 1 else raw
    out = stacked[select] if len(blocks) > 1 else raw.copy()
    out.sort_indices()
    return out


def as_csr(rows):
    """Host rows given to ``update()`` of a sparse index alongside sparse ones, as the canonical CSR matrix of their values."""
    import scipy.sparse as sp

    return canonical_csr(rows) if is_sparse(rows) else sp.csr_matrix(np.asarray(rows, dtype=np.float32))


class CsrRowsView:
    """The rows of a CSR matrix for ``uint8_codebook``: its shape, and ``view[rows]`` -- the sampled rows, dense."""

    def __init__(self, csr):
        self.csr, self.shape = csr, tuple(csr.shape)

    def __getitem__(self, rows):
        return np.ascontiguousarray(self.csr[np.asarray(rows)].toarray(), dtype=np.float32)
