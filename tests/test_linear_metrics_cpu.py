"""seuclidean / wminkowski (p = 2) / mahalanobis / minkowski (p = 2) without a device: the positional reading of metric_kwds and
every error it can raise (before any library call), the factor of VI, the combinations refused up front, and the pickle
round trip of the map an index keeps."""
import pickle

import numpy as np
import pytest

import pynndescent_amd
from pynndescent_amd import NNDescent, _capi, linear_map, nndescent

D = 6
RS = np.random.RandomState(0)
X = (5.0 + RS.standard_normal((60, D))).astype(np.float32)
B = RS.standard_normal((D, D))
VI = B @ B.T + 0.5 * np.eye(D)
V = X.astype(np.float64).var(axis=0)
W = np.array([0.5, 2.0, 0.0, 1.0, 3.0, 0.25])


@pytest.fixture
def no_library(monkeypatch):
    """any call into the library (a handle, a searcher, a transform, a device) fails the test"""
    def boom(*a, **k):
        raise AssertionError("the library was called before the arguments were checked")

    monkeypatch.setattr(_capi, "Builder", boom)
    monkeypatch.setattr(_capi, "Searcher", boom)
    monkeypatch.setattr(_capi, "load_library", boom)


def test_the_names_are_on_the_device_path():
    for name in ("seuclidean", "standardised_euclidean", "wminkowski", "weighted_minkowski", "mahalanobis", "minkowski"):
        m = nndescent._metric_record(name)
        assert m.linear and m.code == _capi.NND_METRIC_SQEUCLIDEAN and m.device_kind == _capi.NND_CORRECT_SQRT
        assert m.correction is _capi.host_sqrt and not m.uint8 and not m.angular and not m.proxy
        assert name in nndescent._KNOWN_REFERENCE_METRICS
        assert name not in nndescent._ND_DISTS  # nn_descent(dist=...) is not extended
    assert not any(m.linear for m in nndescent._METRICS.values())
    with pytest.raises(NotImplementedError, match="mahalanobis"):  # the text make_index shows lists the new names
        nndescent._metric_record("manhattan")


def test_metric_kwds_are_read_by_position_not_by_name():
    a = linear_map.parse_metric_kwds("seuclidean", {"anything": V}, D)
    assert a.kind == linear_map.NND_LINEAR_DIAGONAL and a.a.dtype == np.float32 and a.shift is None
    np.testing.assert_array_equal(a.a, (1.0 / np.sqrt(V)).astype(np.float32))
    np.testing.assert_array_equal(linear_map.parse_metric_kwds("standardised_euclidean", {"sigma": V}, D).a, a.a)
    # (w, p): the first value is w whatever it is called, the second is p
    w = linear_map.parse_metric_kwds("wminkowski", {"p": W, "w": 2}, D)
    assert w.kind == linear_map.NND_LINEAR_DIAGONAL
    np.testing.assert_array_equal(w.a, np.sqrt(W).astype(np.float32))
    np.testing.assert_array_equal(linear_map.parse_metric_kwds("weighted_minkowski", {"w": W}, D).a, w.a)
    m = linear_map.parse_metric_kwds("mahalanobis", {"vinv": VI}, D)
    assert m.kind == linear_map.NND_LINEAR_DENSE and m.a.shape == (D, D) and m.a.dtype == np.float32
    assert linear_map.parse_metric_kwds("minkowski", None, D) is None
    assert linear_map.parse_metric_kwds("minkowski", {}, D) is None
    assert linear_map.parse_metric_kwds("minkowski", {"p": 2}, D) is None
    assert linear_map.parse_metric_kwds("minkowski", {"p": 2.0}, D) is None


def test_the_diagonal_factors_are_exact_square_roots():
    v = np.array([4.0, 0.25, 16.0, 1.0, 64.0, 0.0625])
    np.testing.assert_array_equal(linear_map.parse_metric_kwds("seuclidean", {"V": v}, D).a,
                                  np.array([0.5, 2.0, 0.25, 1.0, 0.125, 4.0], np.float32))
    w = np.array([4.0, 0.25, 0.0, 1.0, 9.0, 2.25])
    np.testing.assert_array_equal(linear_map.parse_metric_kwds("wminkowski", {"w": w}, D).a,
                                  np.array([2.0, 0.5, 0.0, 1.0, 3.0, 1.5], np.float32))


@pytest.mark.parametrize("case", ["spd", "asymmetric", "rank_deficient", "zero"])
def test_the_factor_reproduces_the_symmetric_part(case):
    rs = np.random.RandomState(1)
    d = 9
    if case == "spd":
        b = rs.standard_normal((d, d))
        vi = b @ b.T + np.eye(d)
    elif case == "asymmetric":  # only the symmetric part enters x^T VI x
        b = rs.standard_normal((d, d))
        skew = rs.standard_normal((d, d))
        vi = b @ b.T + np.eye(d) + (skew - skew.T)
    elif case == "rank_deficient":  # PSD of rank 4: Cholesky fails, eigh takes over
        b = rs.standard_normal((d, 4))
        vi = b @ b.T
    else:
        vi = np.zeros((d, d))
    a = linear_map.mahalanobis_factor(vi)
    sym = (vi + vi.T) / 2.0
    scale = max(np.abs(sym).max(), 1.0)
    assert a.dtype == np.float64 and a.shape == (d, d)
    np.testing.assert_allclose(a.T @ a, sym, rtol=0, atol=64 * d * np.finfo(np.float64).eps * scale)
    x = rs.standard_normal((20, d))
    np.testing.assert_allclose(((x @ a.T) ** 2).sum(1), np.einsum("ni,ij,nj->n", x, sym, x), rtol=1e-10, atol=1e-10 * scale)


def _bad_kwds():
    nan_v, nan_vi = V.copy(), VI.copy()
    nan_v[2], nan_vi[1, 3] = np.nan, np.inf
    return [
        ("seuclidean", None, "seuclidean"), ("seuclidean", {}, "seuclidean"),
        ("standardised_euclidean", None, "standardised_euclidean"),
        ("seuclidean", {"V": V[:-1]}, "shape"), ("seuclidean", {"V": nan_v}, "NaN"),
        ("seuclidean", {"V": np.where(np.arange(D) == 1, 0.0, V)}, "> 0"),
        ("seuclidean", {"V": np.where(np.arange(D) == 1, -1.0, V)}, "> 0"),
        ("seuclidean", {"V": V, "extra": 1}, "seuclidean"),
        ("wminkowski", None, "wminkowski"), ("weighted_minkowski", {}, "weighted_minkowski"),
        ("wminkowski", {"w": W[:-1]}, "shape"), ("wminkowski", {"w": np.where(np.arange(D) == 0, np.inf, W)}, "infinity"),
        ("wminkowski", {"w": np.where(np.arange(D) == 4, -0.5, W)}, ">= 0"),
        ("mahalanobis", None, "mahalanobis"), ("mahalanobis", {}, "mahalanobis"),
        ("mahalanobis", {"VI": VI[:-1]}, "shape"), ("mahalanobis", {"VI": VI[:-1, :-1]}, "shape"),
        ("mahalanobis", {"VI": nan_vi}, "infinity"),
        ("mahalanobis", {"VI": -VI}, "positive semi-definite"),
        ("mahalanobis", {"VI": np.diag([1.0, 1.0, -1e-3, 1.0, 1.0, 1.0])}, "positive semi-definite"),
        ("minkowski", {"p": 2, "q": 2}, "at most one"),
    ]


@pytest.mark.parametrize("metric, kwds, match", _bad_kwds())
def test_bad_metric_kwds_are_value_errors_before_any_device_work(no_library, metric, kwds, match):
    with pytest.raises(ValueError, match=match):
        NNDescent(X, metric=metric, metric_kwds=kwds, n_neighbors=5)
    with pytest.raises(ValueError, match=match):
        pynndescent_amd.exact_knn(X, k=3, metric=metric, metric_kwds=kwds)
    idx = np.tile(np.arange(5, dtype=np.int32), (X.shape[0], 1))
    with pytest.raises(ValueError, match=match):
        NNDescent.from_graph(X, idx, np.zeros(idx.shape, np.float32), metric=metric, metric_kwds=kwds)


@pytest.mark.parametrize("metric, kwds", [("minkowski", {"p": 3}), ("minkowski", {"p": 1.0}), ("wminkowski", {"w": W, "p": 1}),
                                          ("weighted_minkowski", {"w": W, "p": 2.5})])
def test_other_p_goes_to_the_reference(no_library, metric, kwds):
    """NotImplementedError is what make_index hands to pynndescent.NNDescent."""
    with pytest.raises(NotImplementedError, match="p = 2"):
        NNDescent(X, metric=metric, metric_kwds=kwds, n_neighbors=5)
    with pytest.raises(NotImplementedError, match="p = 2"):
        pynndescent_amd.exact_knn(X, k=3, metric=metric, metric_kwds=kwds)


@pytest.mark.parametrize("metric, kwds", [("seuclidean", {"V": V}), ("wminkowski", {"w": W}), ("mahalanobis", {"VI": VI}),
                                          ("minkowski", {"p": 2})])
def test_refused_combinations_come_first(no_library, metric, kwds):
    with pytest.raises(ValueError, match="Not uint8 quantization version of " + metric):
        NNDescent(X, metric=metric, metric_kwds=kwds, n_neighbors=5, quantization="uint8")
    with pytest.raises(NotImplementedError, match="one GPU"):
        NNDescent(X, metric=metric, metric_kwds=kwds, n_neighbors=5, n_devices=2)
    with pytest.raises(NotImplementedError, match="dist must be one of"):
        pynndescent_amd.nn_descent(X, 5, np.array([1, 2, 3], np.int64), dist=metric)


def test_metric_kwds_stays_unread_for_the_other_metrics(no_library):
    """The nine metrics without arguments ignore metric_kwds as before: nothing in it can raise."""
    idx = np.tile(np.arange(5, dtype=np.int32), (X.shape[0], 1))
    for metric in ("euclidean", "cosine", "sqeuclidean"):
        index = NNDescent.from_graph(X, idx, np.zeros(idx.shape, np.float32), metric=metric, metric_kwds={"V": "nonsense"})
        assert index._linear_map is None


def test_the_shift_comes_from_one_place():
    rows = linear_map.shift_rows(100000)
    assert rows[0] == 0 and rows[1] == 100000 // 4096 and rows[-1] < 100000
    np.testing.assert_array_equal(linear_map.shift_rows(10), np.arange(10))

    class View:  # what a device tensor's gathering view looks like to shift_of
        shape = X.shape

        def __getitem__(self, ids):
            return X[ids].copy()

    c = linear_map.shift_of(X)
    assert c.dtype == np.float32 and c.shape == (D,)
    np.testing.assert_array_equal(c, linear_map.shift_of(View()))
    np.testing.assert_array_equal(c, X.astype(np.float64).mean(0).astype(np.float32))


@pytest.mark.parametrize("metric, kwds", [("seuclidean", {"V": V}), ("wminkowski", {"w": W, "p": 2}), ("mahalanobis", {"VI": VI})])
def test_pickle_round_trip_of_the_map(no_library, metric, kwds):
    n = X.shape[0]
    idx = np.stack([(np.arange(n) + j) % n for j in range(5)], 1).astype(np.int32)
    index = NNDescent.from_graph(X, idx, np.zeros(idx.shape, np.float32), metric=metric, metric_kwds=kwds, random_state=1)
    lin = index._linear_map
    assert lin.a.dtype == np.float32 and lin.shift.dtype == np.float32 and lin.shift.shape == (D,)
    np.testing.assert_array_equal(lin.shift, linear_map.shift_of(X))
    # a prepared index by hand (prepare() is the device's): what __getstate__ needs
    index._vertex_order = np.arange(n)
    index._search_forest = []
    index.__dict__["_lin_data"] = np.zeros((n, D), np.float32)  # derived data: must not travel
    clone = pickle.loads(pickle.dumps(index))
    assert "_lin_data" not in clone.__dict__ and "_device_linear" not in clone.__dict__
    assert clone._linear_map.kind == lin.kind
    for got, want in ((clone._linear_map.a, lin.a), (clone._linear_map.shift, lin.shift)):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(clone._raw_data, X)
    assert clone._distance_correction is _capi.host_sqrt and clone.metric == metric
