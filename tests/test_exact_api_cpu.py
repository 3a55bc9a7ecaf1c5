"""pynndescent_amd.exact_knn / NNDescent.recall without a GPU: the argument errors are raised before any library call, and
the row sampling of recall() is a documented, deterministic rule."""
import numpy as np
import pytest

import pynndescent_amd
from pynndescent_amd import NNDescent, _capi


@pytest.fixture
def no_library(monkeypatch):
    """any call into the library (a handle, a device) fails the test"""
    def boom(*a, **k):
        raise AssertionError("the library was called before the arguments were checked")

    monkeypatch.setattr(_capi, "Builder", boom)


X = np.random.RandomState(0).standard_normal((40, 5)).astype(np.float32)


def test_exact_knn_is_exported():
    assert pynndescent_amd.exact_knn is pynndescent_amd.nndescent.exact_knn
    assert callable(NNDescent.recall)


def test_argument_errors_come_before_any_device_work(no_library):
    with pytest.raises(ValueError, match="not both"):
        pynndescent_amd.exact_knn(X, queries=X[:3], rows=[0, 1], k=3)
    with pytest.raises(NotImplementedError, match="256"):
        pynndescent_amd.exact_knn(np.zeros((300, 4), np.float32), k=257)
    with pytest.raises(ValueError, match="k must be in 1"):
        pynndescent_amd.exact_knn(X, k=41)
    with pytest.raises(ValueError, match="k must be in 1"):
        pynndescent_amd.exact_knn(X, k=0)
    with pytest.raises(ValueError, match="Metric is neither callable"):
        pynndescent_amd.exact_knn(X, k=3, metric="no-such-metric")
    with pytest.raises(NotImplementedError, match="use pynndescent.NNDescent"):
        pynndescent_amd.exact_knn(X, k=3, metric="manhattan")
    with pytest.raises(ValueError, match="non-negative"):
        pynndescent_amd.exact_knn(-np.abs(X), k=3, metric="hellinger")
    with pytest.raises(ValueError, match="non-negative"):
        pynndescent_amd.exact_knn(np.abs(X), queries=-np.abs(X[:2]), k=3, metric="hellinger")
    with pytest.raises(ValueError, match="shape"):
        pynndescent_amd.exact_knn(X, queries=np.zeros((2, 4), np.float32), k=3)
    with pytest.raises(ValueError, match="rows must be ids"):
        pynndescent_amd.exact_knn(X, rows=[0, 40], k=3)
    q = X[:3].copy()
    q[1, 2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        pynndescent_amd.exact_knn(X, queries=q, k=3)


def test_recall_exists_on_from_graph_and_samples_deterministically(no_library):
    idx = np.tile(np.arange(5, dtype=np.int32), (40, 1))
    index = NNDescent.from_graph(X, idx, np.zeros((40, 5), np.float32))
    assert callable(index.recall)
    a = NNDescent._recall_rows(1000, 100, 7)
    b = index._recall_rows(1000, 100, 7)
    assert np.array_equal(a, b) and a.dtype == np.int64
    assert np.array_equal(a, np.random.RandomState(7).choice(1000, size=100, replace=False))
    assert len(np.unique(a)) == 100 and a.min() >= 0 and a.max() < 1000
    assert not np.array_equal(a, NNDescent._recall_rows(1000, 100, 8))
    assert np.array_equal(np.sort(NNDescent._recall_rows(30, 1000, 0)), np.arange(30))  # min(n_rows, n) distinct rows
    with pytest.raises(AssertionError, match="library was called"):  # ... and the method goes on to the exact search
        index.recall(n_rows=10, random_state=0)
