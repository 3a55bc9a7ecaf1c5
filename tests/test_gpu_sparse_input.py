"""Sparse input on a real MI355X: the CSR -> dense kernel against ``toarray()`` bit for bit, an index built from a scipy.sparse
matrix against the index built from its dense form (graph, queries, filtered queries, update, exact search, recall, pickling --
all by ``array_equal``), and builds and queries against the reference's own sparse path (tests/golden/sparse_input.npz,
tests/golden/make_golden_sparse.py)."""
import functools
import itertools
import os
import pickle

import numpy as np
import pytest
import scipy.sparse as sp

from pynndescent_amd import NNDescent, _capi, exact_knn, sparse_input
from tests import sparse_util as SU

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_input.npz")
WIDTHS = list(itertools.product((np.int32, np.int64), repeat=2))  # (indptr, indices)
K = 10
SEED = 5


def _torch():
    import torch

    return torch


def _dense_by_kernel(csr, offset=0):
    """``csr`` through ``nnd_device_csr_rows`` into a buffer pre-filled with NaN, ``offset`` floats behind a 16-byte boundary; the
    (n, d) result and the NaN guard floats around it, as numpy."""
    torch = _torch()
    dev = torch.device("cuda", 0)
    n, d = csr.shape
    guard = 8
    buf = torch.full((guard + offset + n * d + guard,), float("nan"), dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    dst = buf[guard + offset: guard + offset + n * d]
    indptr, indices, values = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (csr.indptr, csr.indices, csr.data))
    _capi.device_csr_rows(0, torch.cuda.current_stream(0).cuda_stream, indptr.data_ptr(), csr.indptr.dtype.itemsize,
                          indices.data_ptr() if csr.nnz else 0, csr.indices.dtype.itemsize, values.data_ptr() if csr.nnz else 0, n, d,
                          dst.data_ptr())
    out = buf.cpu().numpy()
    return out[guard + offset: guard + offset + n * d].reshape(n, d), np.concatenate([out[:guard + offset], out[guard + offset + n * d:]])


def _assert_dense(csr, dense, offset=0):
    got, around = _dense_by_kernel(csr, offset)
    assert np.isnan(around).all(), "a write outside the buffer"
    assert not np.isnan(got).any(), "%d elements were not written" % int(np.isnan(got).sum())
    assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(dense, np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("d", [1, 3, 4, 5, 63, 64, 65, 130, 4099, 20011])
def test_kernel_equals_toarray(d):
    """Single floats, both sides of the 16-byte boundary, rows that straddle tiles and rows much longer than a tile; every
    density; both widths of both index arrays; the buffer on and off a 16-byte boundary."""
    combos = itertools.cycle(WIDTHS)
    for n in (1, 2, 257):
        for density in (0.0, 0.02, 0.3, 1.0):
            csr, dense = SU.random_csr(n, d, density, seed=n + d, index_dtypes=next(combos))
            assert np.array_equal(csr.toarray(), dense)
            _assert_dense(csr, dense, offset=(n + d) % 4)
    csr, dense = SU.random_csr(257, d, 0.3, seed=d)
    for widths in WIDTHS:
        _assert_dense(SU.with_index_dtypes(csr, widths), dense)
    for offset in (1, 2, 3):
        _assert_dense(csr, dense, offset=offset)


@pytest.mark.parametrize("d", [1, 5, 64, 130, 4099])
def test_kernel_edge_rows(d):
    n = 257
    for empty, full in (((0,), ()), ((128,), ()), ((256,), ()), ((0, 128, 256), ()), ((100,), (101,)), ((101,), (100,)),
                        ((0, 2), (1,)), ((), (0, 256))):
        csr, dense = SU.random_csr(n, d, 0.3, seed=d + len(empty), empty_rows=empty, full_rows=full)
        _assert_dense(csr, dense)
    for widths in WIDTHS:  # no stored entry at all
        _assert_dense(SU.with_index_dtypes(sp.csr_matrix((n, d), dtype=np.float32), widths), np.zeros((n, d), np.float32))
    # the flat neighbours: column d - 1 of a row and column 0 of the next, and nothing else
    dense = np.zeros((n, d), np.float32)
    dense[10, d - 1], dense[11, 0], dense[255, d - 1], dense[256, 0], dense[0, 0], dense[256, d - 1] = 1.5, -2.5, 3.5, 4.5, 5.5, 6.5
    _assert_dense(sp.csr_matrix(dense), dense)
    # an explicitly stored zero is a value like any other
    csr, dense = SU.random_csr(n, d, 0.3, seed=99)
    csr.data[::3] = 0.0
    _assert_dense(csr, csr.toarray())


def test_kernel_entry_refuses_bad_arguments():
    torch = _torch()
    t = torch.zeros((8,), dtype=torch.float32, device="cuda:0")
    with pytest.raises(_capi.NNDError, match="index width"):
        _capi.device_csr_rows(0, 0, t.data_ptr(), 2, t.data_ptr(), 4, t.data_ptr(), 1, 4, t.data_ptr())
    with pytest.raises(_capi.NNDError, match="null pointer"):
        _capi.device_csr_rows(0, 0, 0, 4, t.data_ptr(), 4, t.data_ptr(), 1, 4, t.data_ptr())
    _capi.device_csr_rows(0, 0, 0, 4, 0, 4, 0, 0, 4, 0)  # nothing to do


# ------------------------------------------------------------------------------------- equality with the dense build
METRICS = ["euclidean", "cosine", "correlation", "hellinger", "jaccard", "russellrao"]
BOOLEAN = ("jaccard", "russellrao")


@functools.lru_cache(maxsize=None)
def _data(boolean):
    x, q, fresh, upd = SU.equality_data(boolean)
    return x, q, fresh, upd


@functools.lru_cache(maxsize=None)
def _pair(metric):
    """(the index of the CSR matrix, the index of its dense form), same ``random_state``; neither is modified by a test."""
    x = _data(metric in BOOLEAN)[0]
    csr = sp.csr_matrix(x)
    assert np.array_equal(csr.toarray(), x)
    return (NNDescent(csr, metric=metric, n_neighbors=K, random_state=SEED),
            NNDescent(x, metric=metric, n_neighbors=K, random_state=SEED))


def _same(got, want):
    assert isinstance(got[0], np.ndarray) and isinstance(got[1], np.ndarray)
    assert got[0].dtype == want[0].dtype and got[1].dtype == want[1].dtype
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])


@pytest.mark.parametrize("metric", METRICS)
def test_sparse_build_equals_dense_build(metric):
    s, h = _pair(metric)
    assert s._is_sparse and sp.issparse(s._raw_data) and s._raw_data.format == "csr"
    assert np.array_equal(s._raw_data.toarray(), h._raw_data)
    _same(s.neighbor_graph, h.neighbor_graph)
    assert np.array_equal(s.rng_state, h.rng_state) and np.array_equal(s.search_rng_state, h.search_rng_state)


@pytest.mark.parametrize("metric", METRICS)
def test_sparse_queries_equal_dense_queries(metric):
    s, h = _pair(metric)
    q = _data(metric in BOOLEAN)[1]
    csr_q = sp.csr_matrix(q)
    assert sp.issparse(s._raw_data)
    want = h.query(q, k=7)
    _same(s.query(csr_q, k=7), want)
    assert sp.issparse(s._raw_data) and np.array_equal(s._raw_data.toarray(), h._raw_data)  # both in the leaf order now
    _same(h.query(csr_q, k=7), want)  # a sparse batch on an index built from dense data
    _same(s.query(q, k=7), want)  # a dense batch on the sparse index: the host-query route
    _same(s.query(sp.coo_matrix(q), k=7), want)
    allowed = np.random.RandomState(1).random_sample(h._raw_data.shape[0]) < 0.3
    for mode in ("walk", "exact"):
        want = h.query(q, k=7, filter=allowed, filter_mode=mode)
        _same(s.query(csr_q, k=7, filter=allowed, filter_mode=mode), want)
        assert s.last_filter == h.last_filter
        _same(s.query(csr_q, k=7, filter=np.flatnonzero(allowed), filter_mode=mode), want)
    few = np.array([3, 100, 900])  # fewer allowed rows than k: (-1, inf) behind them
    _same(s.query(csr_q, k=7, filter=few), h.query(q, k=7, filter=few))
    _same(s.query(csr_q, k=7, filter=np.zeros(allowed.shape[0], bool)), h.query(q, k=7, filter=np.zeros(allowed.shape[0], bool)))


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_sparse_uint8_queries_equal_dense_uint8_queries(metric):
    """The uint8 proxy walk with its rerank: the codebook is drawn from the same rows, whichever side they are on."""
    x, q = _data(False)[:2]
    s = NNDescent(sp.csr_matrix(x), metric=metric, n_neighbors=K, random_state=SEED, quantization="uint8")
    h = NNDescent(x, metric=metric, n_neighbors=K, random_state=SEED, quantization="uint8")
    want = h.query(q, k=5)
    _same(s.query(sp.csr_matrix(q), k=5), want)
    _same(s.query(q, k=5), want)
    assert np.array_equal(s._quantized_values, h._quantized_values) and sp.issparse(s._raw_data)
    again = pickle.loads(pickle.dumps(s))
    _same(again.query(sp.csr_matrix(q), k=5), want)


@pytest.mark.parametrize("metric", METRICS)
def test_sparse_update_equals_dense_update(metric):
    x, _, fresh, upd = _data(metric in BOOLEAN)
    ids = [int(v) for v in np.random.RandomState(2).choice(x.shape[0], upd.shape[0], replace=False)]
    ids[3] = 7  # an empty row gets entries
    upd = upd.copy()
    upd[5] = 0.0  # and a row loses all of its
    s = NNDescent(sp.csr_matrix(x), metric=metric, n_neighbors=K, random_state=SEED)
    h = NNDescent(x, metric=metric, n_neighbors=K, random_state=SEED)
    s.prepare()
    h.prepare()
    s.update(xs_fresh=sp.csr_matrix(fresh), xs_updated=sp.csr_matrix(upd), updated_indices=ids)
    h.update(xs_fresh=fresh, xs_updated=upd, updated_indices=ids)
    _same(s.neighbor_graph, h.neighbor_graph)
    assert sp.issparse(s._raw_data) and s._raw_data.shape == (x.shape[0] + fresh.shape[0], x.shape[1])
    assert np.array_equal(s._raw_data.toarray(), h._raw_data)  # prepared again: both in the new leaf order
    assert np.array_equal(s._vertex_order, h._vertex_order)
    q = _data(metric in BOOLEAN)[1]
    _same(s.query(sp.csr_matrix(q), k=5), h.query(q, k=5))
    s.update(xs_fresh=fresh[:4])  # host rows alongside a sparse index: uploaded, and _raw_data stays CSR
    h.update(xs_fresh=fresh[:4])
    _same(s.neighbor_graph, h.neighbor_graph)
    assert sp.issparse(s._raw_data) and np.array_equal(s._raw_data.toarray(), h._raw_data)


@pytest.mark.parametrize("metric", METRICS)
def test_sparse_exact_knn_and_recall_equal_dense(metric):
    s, h = _pair(metric)
    x, q = _data(metric in BOOLEAN)[:2]
    csr, csr_q = sp.csr_matrix(x), sp.csr_matrix(q)
    want = exact_knn(x, queries=q, k=6, metric=metric)
    _same(exact_knn(csr, queries=csr_q, k=6, metric=metric), want)
    _same(exact_knn(csr, queries=q, k=6, metric=metric), want)
    _same(exact_knn(x, queries=csr_q, k=6, metric=metric), want)
    rows = np.array([0, 7, 100, 900, 1499])
    _same(exact_knn(csr, k=6, metric=metric, rows=rows), exact_knn(x, k=6, metric=metric, rows=rows))
    assert s.recall(n_rows=300, random_state=1) == h.recall(n_rows=300, random_state=1)
    assert sp.issparse(s._raw_data)


@pytest.mark.parametrize("metric", ["euclidean", "cosine", "jaccard"])
def test_sparse_index_pickles_as_csr(metric):
    s, h = _pair(metric)
    q = _data(metric in BOOLEAN)[1]
    csr_q = sp.csr_matrix(q)
    want = h.query(q, k=7)
    blob = pickle.dumps(s)
    again = pickle.loads(blob)
    assert again._is_sparse and sp.issparse(again._raw_data) and "_device_data" not in again.__dict__
    _same(again.query(csr_q, k=7), want)
    _same(again.query(q, k=7), want)
    allowed = np.random.RandomState(1).random_sample(h._raw_data.shape[0]) < 0.3
    _same(again.query(csr_q, k=7, filter=allowed, filter_mode="exact"), h.query(q, k=7, filter=allowed, filter_mode="exact"))
    assert sp.issparse(again._raw_data)
    assert again.recall(n_rows=300, random_state=1) == h.recall(n_rows=300, random_state=1)
    _same(again.neighbor_graph, h.neighbor_graph)
    with pytest.raises(NotImplementedError, match="sparse"):
        s.to_reference()


def test_pickle_carries_no_dense_rows():
    n, d = 1500, 400
    csr = SU.random_csr(n, d, 0.05, seed=8)[0]
    csr.data = np.abs(csr.data)
    index = NNDescent(csr, metric="cosine", n_neighbors=K, random_state=SEED)
    assert sp.issparse(index._raw_data)
    index.prepare()
    assert sp.issparse(index._raw_data)
    blob = pickle.dumps(index)
    print("pickle of a %d x %d index at density 0.05: %d bytes, dense rows %d bytes" % (n, d, len(blob), n * d * 4))
    assert len(blob) < n * d * 4 / 2
    again = pickle.loads(blob)
    _same(again.query(csr[:20], k=5), index.query(csr[:20], k=5))


def test_errors_come_from_the_device_flags():
    x = SU.equality_data()[0]
    bad = x.copy()
    bad[1234, 5] = -1e-3
    with pytest.raises(ValueError, match="non-negative"):
        NNDescent(sp.csr_matrix(bad), metric="hellinger", n_neighbors=K, random_state=1)
    bad[1234, 5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        NNDescent(sp.csr_matrix(bad), metric="euclidean", n_neighbors=K, random_state=1)
    with pytest.raises(NotImplementedError, match="sparse input") as e:  # the size rule, against the free memory at the call
        NNDescent(sp.csr_matrix((4_000_000, 40_000), dtype=np.float32), metric="euclidean", n_neighbors=K)
    assert "pynndescent.NNDescent" in str(e.value)


# ------------------------------------------------------------------------------- against the reference's own sparse path
def _returned_distances(metric, q, x, ids):
    out = np.empty(ids.shape, np.float64)
    for r in range(ids.shape[0]):
        rows = x[np.maximum(ids[r], 0)]
        out[r] = SU.exact_euclidean(q[r:r + 1], rows)[0] if metric == "euclidean" else SU.true_distances(metric, q[r:r + 1], rows)[0]
    return out


@functools.lru_cache(maxsize=None)
def _fixture():
    x, q = SU.fixture_data()
    return np.load(GOLDEN), x, q, sp.csr_matrix(x), sp.csr_matrix(q)


@pytest.mark.parametrize("metric", ["euclidean", "cosine", "hellinger", "jaccard"])
def test_build_against_reference_sparse_fixture(metric):
    f, x, _, csr, _ = _fixture()
    kth = SU.kth_distance(metric, x, x, 10)
    rec_gpu, rec_ref = [], []
    for s in f["seeds"]:
        idx, dist = NNDescent(csr, metric=metric, n_neighbors=10, random_state=int(s)).neighbor_graph
        assert idx.shape == (x.shape[0], 10) and (idx >= 0).all()
        rec_gpu.append(SU.recall_by_distance(metric, x, x, idx, kth))
        rec_ref.append(float(f["%s_recall_%d" % (metric, s)]))
        np.testing.assert_allclose(dist, _returned_distances(metric, x, x, idx), rtol=2e-4, atol=1e-6)
    print("%s: recall@10 gpu %.4f reference %.4f" % (metric, np.mean(rec_gpu), np.mean(rec_ref)))
    assert np.mean(rec_ref) >= 0.9
    assert abs(np.mean(rec_gpu) - np.mean(rec_ref)) <= 0.01


@pytest.mark.parametrize("metric", ["euclidean", "cosine", "hellinger", "jaccard"])
def test_query_against_reference_sparse_fixture(metric):
    f, x, q, csr, csr_q = _fixture()
    index = NNDescent(csr, metric=metric, n_neighbors=10, random_state=int(f["seeds"][0]))
    qi, qd = index.query(csr_q, k=10)
    assert (qi >= 0).all()
    kth = SU.kth_distance(metric, q, x, 10)
    r_gpu, r_ref = SU.recall_by_distance(metric, q, x, qi, kth), SU.recall_by_distance(metric, q, x, f[metric + "_q_idx"], kth)
    print("%s queries: recall@10 gpu %.4f reference %.4f" % (metric, r_gpu, r_ref))
    assert r_ref == pytest.approx(float(f[metric + "_q_recall"]))
    assert r_gpu >= r_ref - 0.02
    # hellinger: the bound of tests/test_gpu_metrics.py, for its reason (float32 Gram values near 1)
    np.testing.assert_allclose(qd, _returned_distances(metric, q, x, qi), rtol=1e-3 if metric == "hellinger" else 2e-4, atol=1e-6)
