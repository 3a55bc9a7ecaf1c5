"""Sparse input, the host side alone: canonical CSR, the metric rule, the size rule and the query shape check.  Everything here is
decided before any device work, so it runs without a GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from pynndescent_amd import NNDescent, sparse_input
from tests import sparse_util as SU


def _dense():
    rs = np.random.RandomState(3)
    x = np.where(rs.random_sample((40, 9)) < 0.3, rs.uniform(0.5, 2.0, (40, 9)), 0.0).astype(np.float64)
    x[5] = 0.0
    return x


def _snapshot(m):
    return tuple(np.array(getattr(m, name), copy=True) for name in (("row", "col", "data") if m.format == "coo" else ("indptr", "indices", "data")))


def _assert_canonical(c, dense):
    assert sp.issparse(c) and c.format == "csr" and c.dtype == np.float32 and c.shape == dense.shape
    assert c.has_canonical_format
    for r in range(c.shape[0]):
        cols = c.indices[c.indptr[r]:c.indptr[r + 1]]
        assert (np.diff(cols) > 0).all()
    assert np.array_equal(c.toarray(), dense.astype(np.float32))


@pytest.mark.parametrize("form", ["coo", "csc", "csr_unsorted", "csr_duplicates", "csr_array", "csr_float32"])
def test_canonical_csr(form):
    dense = _dense()
    if form == "coo":
        given = sp.coo_matrix(dense)
    elif form == "csc":
        given = sp.csc_matrix(dense)
    elif form == "csr_array":
        given = sp.csr_array(dense)
    elif form == "csr_float32":  # nothing to change: no copy is needed
        given = sp.csr_matrix(dense.astype(np.float32))
    elif form == "csr_unsorted":
        c = sp.csr_matrix(dense.astype(np.float32))
        indices, data = c.indices.copy(), c.data.copy()
        for r in range(c.shape[0]):  # every row's entries in descending column order
            s, e = c.indptr[r], c.indptr[r + 1]
            indices[s:e], data[s:e] = indices[s:e][::-1], data[s:e][::-1]
        given = sp.csr_matrix((data, indices, c.indptr.copy()), shape=c.shape)
        assert not given.has_sorted_indices or (np.diff(c.indptr) < 2).all()
        given.has_sorted_indices = False
    else:  # every entry stored as two halves
        c = sp.coo_matrix(dense.astype(np.float32))
        row, col, data = np.concatenate([c.row, c.row]), np.concatenate([c.col, c.col]), np.concatenate([c.data, c.data]) / 2
        order = np.lexsort((col, row))
        indptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=dense.shape[0]))])
        given = sp.csr_matrix((data[order].astype(np.float32), col[order], indptr), shape=dense.shape)
        assert given.nnz == 2 * c.nnz
    before = _snapshot(given)
    c = sparse_input.canonical_csr(given)
    _assert_canonical(c, dense)
    for was, now in zip(before, _snapshot(given)):  # the caller's object is as it was
        assert np.array_equal(was, now)
    if form == "csr_float32":
        assert c is given


def test_explicit_zero_stays_stored():
    dense = _dense()
    c = sp.csr_matrix(dense.astype(np.float32))
    c.data[3] = 0.0
    dense32 = c.toarray()
    out = sparse_input.canonical_csr(c)
    assert out.nnz == c.nnz and (out.data == 0).sum() == 1
    assert np.array_equal(out.toarray(), dense32)


def _csr(n=50, d=8):
    return SU.random_csr(n, d, 0.3, 1)[0]


@pytest.mark.parametrize("metric,kwds", [("dot", None), ("inner_product", None), ("yule", None), ("mahalanobis", {"VI": np.eye(8)})])
def test_metric_without_a_sparse_form_raises_the_references_error(metric, kwds):
    with pytest.raises(ValueError, match="Metric %s not supported for sparse data" % metric):
        NNDescent(_csr(), metric=metric, metric_kwds=kwds, n_neighbors=5)


def test_refused_metric_stays_refused_and_sharding_is_refused():
    with pytest.raises(NotImplementedError, match="manhattan"):
        NNDescent(_csr(), metric="manhattan", n_neighbors=5)
    with pytest.raises(NotImplementedError, match="one GPU"):
        NNDescent(_csr(), metric="euclidean", n_neighbors=5, n_devices=2)
    with pytest.raises(NotImplementedError):  # minkowski under the dense rule: p = 2 alone
        NNDescent(_csr(), metric="minkowski", metric_kwds={"p": 3}, n_neighbors=5)


def test_size_rule_around_the_threshold():
    n, d = 1000, 70  # the tensor: 4 n d; the handle's prepared copy: rows padded to 96 floats
    tensor, prepared = sparse_input.dense_bytes(n, d)
    assert (tensor, prepared) == (4 * n * d, 4 * n * 96)
    assert sparse_input.check_dense_fits(n, d, tensor + prepared) == (tensor, prepared)
    with pytest.raises(NotImplementedError) as e:
        sparse_input.check_dense_fits(n, d, tensor + prepared - 1)
    msg = str(e.value)
    assert "sparse input" in msg and "pynndescent.NNDescent" in msg and str(tensor) in msg and str(prepared) in msg
    assert sparse_input.check_dense_fits(0, d, 0) == (0, 0)


def test_sparse_query_of_the_wrong_width_raises():
    x = SU.random_csr(30, 8, 0.5, 2)[1]
    idx = np.tile(np.arange(5, dtype=np.int32), (30, 1))
    index = NNDescent.from_graph(x, idx, np.zeros((30, 5), np.float32))
    with pytest.raises(ValueError, match=r"query_data must have shape \(n_queries, 8\)"):
        index.query(SU.random_csr(4, 7, 0.5, 3)[0], k=3)
    with pytest.raises(ValueError, match=r"query_data must have shape \(n_queries, 8\)"):
        index.query(SU.random_csr(4, 7, 0.5, 3)[0], k=3, filter=np.ones(30, bool))


def test_make_index_hands_rows_that_do_not_fit_to_the_reference(monkeypatch):
    """The size rule's error is what ``make_index`` turns into a build by ``pynndescent.NNDescent`` (a stand-in here)."""
    import sys
    import types

    import pynndescent_amd

    def no_room(csr, device, check_fit=False):
        assert check_fit
        sparse_input.check_dense_fits(csr.shape[0], csr.shape[1], 1000)

    seen = {}
    stand_in = types.ModuleType("pynndescent")
    stand_in.NNDescent = lambda data, *a, **kw: seen.update(data=data, kw=kw) or "reference index"
    monkeypatch.setattr(sparse_input, "dense_rows_on_device", no_room)
    monkeypatch.setitem(sys.modules, "pynndescent", stand_in)
    m = _csr()
    with pytest.warns(UserWarning, match="sparse input"):
        assert pynndescent_amd.make_index(m, metric="cosine", n_neighbors=5) == "reference index"
    assert seen["data"] is m and seen["kw"] == {"metric": "cosine", "n_neighbors": 5}
    with pytest.raises(ValueError, match="not supported for sparse data"):  # the reference's own error is not handed over
        pynndescent_amd.make_index(m, metric="dot", n_neighbors=5)
