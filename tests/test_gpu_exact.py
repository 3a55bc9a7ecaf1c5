"""Exact k-nearest-neighbour search on the GPU (csrc/exact.hip): the f32 MFMA scan + float64 refinement with its certificate,
and the float64 tier, against brute-force truth under the comparison rule of tests/exact_util.py."""
import functools

import numpy as np
import pytest

import pynndescent_amd
from oracle import oracle as O
from pynndescent_amd import NNDescent, _capi
from tests import exact_util as XU
from tests import metric_util as MU
from tests.util_data import clustered

pytestmark = pytest.mark.gpu

NAMES = ("euclidean", "l2", "sqeuclidean", "cosine", "dot", "inner_product", "correlation", "hellinger")


def _unit(x):
    """dot: the rows as NNDescent hands them to the library (L2-normalised on the host)"""
    from sklearn.preprocessing import normalize

    return normalize(x, norm="l2", copy=True)


def _builder(x, metric, flags=0, k=10):
    b = _capi.Builder(x.shape[0], x.shape[1], _capi.METRIC_CODES[metric], k, 0, 60, 200, min(60, k), 1, 0.001, [1, 2, 3], [4, 5, 6],
                      flags=_capi.NND_FLAG_NO_GRAPH | flags)
    b.set_data_host(x)
    return b


# ---- 1. rows mode, every tile edge --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_set(d, metric):
    x = clustered(3000, d, 6, 24, 100 + d)
    return x, _builder(x, metric), _builder(x, metric, _capi.NND_FLAG_TEST_EXACT_F64)


@functools.lru_cache(maxsize=None)
def _edge_truth(d, metric, k):
    return XU.oracle_truth(_edge_set(d, metric)[0], k, metric)


SAMPLE_257 = np.sort(np.random.RandomState(5).choice(3000, 257, replace=False)).astype(np.int64)


@pytest.mark.parametrize("sample", [False, True], ids=["all", "257rows"])
@pytest.mark.parametrize("k", [1, 10, 33, 64, 65, 100, 256])
@pytest.mark.parametrize("metric", ["euclidean", "cosine", "correlation"])
@pytest.mark.parametrize("d", [7, 24, 40, 130])
def test_rows_mode_tile_edges(d, metric, k, sample):
    x, b_def, b_f64 = _edge_set(d, metric)
    rows = SAMPLE_257 if sample else None
    truth = _edge_truth(d, metric, k)
    xq = x
    if sample:
        truth, xq = truth[rows], x[rows]
    name = "d=%d %s k=%d %s" % (d, metric, k, "sample" if sample else "all")
    i1, d1, s1 = b_def.exact_knn(rows, k)
    i2, d2, s2 = b_f64.exact_knn(rows, k)
    print(name, "default:", s1, "f64 tier:", s2)
    XU.check_exact(name + " default", metric, x, xq, i1, d1, truth, k)
    XU.check_exact(name + " f64 tier", metric, x, xq, i2, d2, truth, k)
    XU.agree(name + " default vs f64 tier", metric, x, xq, (i1, d1), (i2, d2), k)
    m = xq.shape[0]
    assert s1["n_rows"] == m and s2["n_rows"] == m and s2["n_fallback"] == m
    assert s1["n_fallback"] <= m / 2, "the certificate's band must not be vacuous: %d of %d rows fell back" % (s1["n_fallback"], m)
    assert s1["pairs"] == m * 3000 and s1["mfma"] > 0


# ---- 2. all eight names ------------------------------------------------------------------------------------------------
def _named_data(metric):
    if metric in MU.NEW_METRICS:
        x = MU.metric_data(metric)[0]
        return _unit(x) if metric == "dot" else x
    x = clustered(2000, 16, 6, 24, 11)
    if metric == "cosine":
        x[[7, 500]] = 0.0
    return x


@pytest.mark.parametrize("k", [10, 33, 65])
@pytest.mark.parametrize("metric", NAMES)
def test_all_eight_names(metric, k):
    x = _named_data(metric)
    truth = XU.oracle_truth(x, k, metric)
    b = _builder(x, metric)
    idx, dist, st = b.exact_knn(None, k)
    b.close()
    print(metric, k, st)
    XU.check_exact("%s k=%d C ABI" % (metric, k), metric, x, x, idx, dist, truth, k)
    # the public function: the metric's own distances against the oracle's
    pi, pd = pynndescent_amd.exact_knn(x, k=k, metric=metric)
    oi, od = O.brute_force_knn(x, k, "euclidean" if metric in XU.EUCLID else metric)
    if metric == "sqeuclidean":
        od = od ** 2
    XU.check_exact("%s k=%d exact_knn ids" % (metric, k), metric, x, x, pi, dist, truth, k)
    pd = np.asarray(pd, np.float64)
    fin = np.isfinite(od) & (np.abs(od) < 1e30)
    # float32 alt-space values through the correction (its slope is at most ~1 on these sets, sqrt at a distance of 0 apart)
    assert np.allclose(pd[fin], od[fin], rtol=1e-5, atol=1e-5), np.abs(pd[fin] - od[fin]).max()


# ---- 3. the data slices ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows", [48, 3000])
def test_data_slices(n_rows):
    x = clustered(20000, 16, 6, 40, 2)
    rows = np.sort(np.random.RandomState(3).choice(20000, n_rows, replace=False)).astype(np.int64)
    b = _builder(x, "euclidean")
    idx, dist, st = b.exact_knn(rows, 15)
    b.close()
    print(n_rows, st)
    truth = XU.oracle_truth(x, 15, "euclidean", rows=rows)
    XU.check_exact("slices %d rows" % n_rows, "euclidean", x, x[rows], idx, dist, truth, 15)
    if n_rows == 48:
        assert st["slices"] > 1, "48 query rows are one query block: the point set must be split over slices"
    assert st["n_fallback"] <= n_rows / 2


# ---- 4. the bimodal set, where an f32 Gram ranking is blind ------------------------------------------------------------
def test_bimodal_set_needs_the_float64_tier():
    rs = np.random.RandomState(7)
    x = 0.01 * rs.standard_normal((3000, 24))
    x = (x + np.where(rs.rand(3000, 1) < 0.5, 1000.0, -1000.0)).astype(np.float32)
    rows = np.sort(np.random.RandomState(1).choice(3000, 300, replace=False)).astype(np.int64)
    b = _builder(x, "euclidean")
    idx, dist, st = b.exact_knn(rows, 10)
    b.close()
    print(st)
    truth = XU.oracle_truth(x, 10, "euclidean", rows=rows)
    XU.check_exact("bimodal", "euclidean", x, x[rows], idx, dist, truth, 10)
    assert st["n_fallback"] >= 1


# ---- 5. exact ties -----------------------------------------------------------------------------------------------------
def test_exact_ties_go_to_the_smaller_id():
    x = clustered(3000, 24, 6, 24, 3)
    x[100:140] = x[100]
    b = _builder(x, "euclidean")
    idx, dist, st = b.exact_knn(None, 10)
    b.close()
    assert np.array_equal(idx[100:140], np.tile(np.arange(100, 110, dtype=np.int32), (40, 1)))
    assert np.all(dist[100:140] == 0.0)
    truth = XU.oracle_truth(x, 10, "euclidean")
    assert np.array_equal(truth[100:140, :10], np.tile(np.arange(100, 110), (40, 1)))
    rest = np.r_[0:100, 140:3000]
    XU.check_exact("ties, other rows", "euclidean", x, x[rest], idx[rest], dist[rest], truth[rest], 10)


# ---- 6. queries mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", NAMES)
def test_queries_mode(metric):
    nonneg = metric == "hellinger"
    allx = clustered(3000 + 257, 24, 6, 24, 21, nonneg=nonneg)
    if metric == "inner_product":
        allx = allx + np.float32(0.5)
    x, q = np.ascontiguousarray(allx[:3000]), np.ascontiguousarray(allx[3000:])
    q[5] = x[1234]
    if metric in ("cosine", "dot", "correlation"):
        q[9] = 0.0
    if metric in XU.EUCLID:
        q = q + np.float32(50.0)  # the SET's column means centre the queries, not their own
    if metric == "dot":
        x, q = _unit(x), _unit(q)
    k = 10
    truth = XU.matrix_truth(metric, x, q, k)
    b = _builder(x, metric)
    idx, dist, st = b.exact_knn_queries(q, k)
    b.close()
    print(metric, st)
    XU.check_exact("queries " + metric, metric, x, q, idx, dist, truth, k)  # (a zero query's row is one tie from end to end)
    pi, pd = pynndescent_amd.exact_knn(x, queries=q, k=k, metric=metric)
    assert np.array_equal(pi, idx)


# ---- 7. NNDescent.recall -----------------------------------------------------------------------------------------------
def test_recall_matches_the_oracle_formula():
    x = clustered(5000, 20, 6, 25, 12)
    index = NNDescent(x, n_neighbors=12, random_state=3)
    got = index.recall(n_rows=500, random_state=1)
    rows = np.random.RandomState(1).choice(5000, size=500, replace=False).astype(np.int64)
    assert np.array_equal(rows, NNDescent._recall_rows(5000, 500, 1))
    want = O.recall(O.brute_force_knn(x, 10, "euclidean", rows=rows)[0], index._neighbor_graph[0][rows])
    assert abs(got - want) <= 1e-12 and 0.9 < got <= 1.0, (got, want)
    k = 12
    bad = NNDescent.from_graph(x, np.tile(np.arange(k, dtype=np.int32), (5000, 1)), np.zeros((5000, k), np.float32))
    got_bad = bad.recall(n_rows=500, random_state=1)
    want_bad = O.recall(O.brute_force_knn(x, 10, "euclidean", rows=rows)[0], bad._neighbor_graph[0][rows])
    assert abs(got_bad - want_bad) <= 1e-12 and got_bad < 0.05, (got_bad, want_bad)


# ---- 8. handles --------------------------------------------------------------------------------------------------------
def test_build_handle_answers_and_keeps_its_graph():
    import torch

    from tests.gpu_util import make_builder

    x = clustered(3000, 24, 6, 24, 8)
    b = make_builder(x, "euclidean", k=15)
    oi = torch.empty((3000, 15), dtype=torch.int32, device="cuda")
    od = torch.empty((3000, 15), dtype=torch.float32, device="cuda")
    b.build_device(oi.data_ptr(), od.data_ptr())
    b.synchronize()
    g0 = b.graph()
    rows = np.arange(0, 3000, 7, dtype=np.int64)
    idx, dist, st = b.exact_knn(rows, 10)
    q = x[:100] + np.float32(0.01)
    qi, qd, _ = b.exact_knn_queries(q, 10)
    g1 = b.graph()
    for a, c in zip(g0, g1):
        assert a.tobytes() == c.tobytes()
    b.close()
    XU.check_exact("build handle rows", "euclidean", x, x[rows], idx, dist, XU.oracle_truth(x, 10, "euclidean", rows=rows), 10)
    XU.check_exact("build handle queries", "euclidean", x, q, qi, qd, XU.matrix_truth("euclidean", x, q, 10), 10)


def test_no_prep_handle_refuses_by_name():
    x = clustered(500, 8, 4, 6, 2)
    b = _capi.Builder(500, 8, 0, 10, 1, 60, 200, 10, 1, 0.001, [1, 2, 3], [4, 5, 6], flags=_capi.NND_FLAG_NO_GRAPH | _capi.NND_FLAG_NO_PREP)
    b.set_data_host(x)
    with pytest.raises(_capi.NNDError, match="NND_FLAG_NO_PREP"):
        b.exact_knn(None, 5)
    with pytest.raises(_capi.NNDError, match="NND_FLAG_NO_PREP"):
        b.exact_knn_queries(x[:4], 5)
    b.close()
    b = _builder(x, "euclidean")
    for k in (0, 257, 501):
        with pytest.raises(_capi.NNDError, match="outside 1"):
            b.exact_knn(None, k)
    b.close()
