"""to_reference() for the metrics with a linear map: true distances are handed over and a prepared index's search structures
are left out, so the reference's own prepare() and query() run on raw rows.  Runs only where the reference is importable (the
build container, through the T0 stub); no GPU -- the index is made around a brute-force graph with NNDescent.from_graph."""
import numpy as np
import pytest

from tests import linear_util as LU


def _reference():
    try:
        from oracle import ref_t0

        return ref_t0.load_reference()
    except Exception as e:  # pragma: no cover
        pytest.skip("reference not importable here: %s" % e)


@pytest.mark.parametrize("metric", LU.METRICS)
def test_handover_of_a_prepared_index(metric):
    ref = _reference()
    from pynndescent_amd import NNDescent

    x, q = LU.fixture_data()
    x, q = np.ascontiguousarray(x[:300, :6]), np.ascontiguousarray(q[:12, :6])
    full = LU.fixture_kwds(LU.fixture_data()[0])[metric]
    kwds = {name: (np.asarray(v)[:6, :6] if np.ndim(v) == 2 else np.asarray(v)[:6] if np.ndim(v) == 1 else v) for name, v in full.items()}
    idx = LU.brute_knn(metric, kwds, x, k=10).astype(np.int32)
    true = LU.true_dist_pairs(metric, kwds, x[:, None, :], x[idx])
    index = NNDescent.from_graph(x, idx, (true ** 2).astype(np.float32), metric=metric, metric_kwds=kwds, random_state=7)
    # prepared by hand (prepare() is the device's): rows in a leaf order, structures of the transformed space
    order = np.random.RandomState(1).permutation(x.shape[0])
    index._vertex_order = order
    index._raw_data = np.ascontiguousarray(x[order])
    index._search_graph, index._search_forest = object(), [object()]
    handed = index.to_reference()
    assert type(handed) is ref.NNDescent
    assert not hasattr(handed, "_search_graph") and not hasattr(handed, "_search_forest") and not hasattr(handed, "_vertex_order")
    np.testing.assert_array_equal(handed._raw_data, x)  # back in the original order
    np.testing.assert_allclose(handed._neighbor_graph[1], true, rtol=1e-6, atol=1e-7)  # true distances, no squared space
    assert handed._distance_correction is None
    np.testing.assert_allclose(handed._distance_func(x[0], x[1]), LU.true_dist_pairs(metric, kwds, x[0], x[1]), rtol=1e-5)
    qi, qd = handed.query(q, k=5, epsilon=0.2)  # the reference's own prepare() and search, on raw rows
    truth = LU.brute_knn(metric, kwds, x, q, k=5)
    rec = np.mean([len(np.intersect1d(t, a)) / 5.0 for t, a in zip(truth, qi)])
    assert rec >= 0.9, rec
    np.testing.assert_allclose(qd, LU.true_dist_pairs(metric, kwds, q[:, None, :], x[qi]), rtol=1e-4, atol=1e-6)
