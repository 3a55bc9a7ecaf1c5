"""The spanning forest without a GPU: the host model of tests/spanning_util.py against scipy.sparse.csgraph on inputs whose
weights are all positive (scipy's spanning tree drops stored zeros), and the argument errors of both entry points."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components, minimum_spanning_tree

from tests.spanning_util import blob_lists, live_edges, model_forest

CASES = [(301, 5, 7, 5, 0), (301, 5, 7, 0, 0), (301, 15, 3, 5, 20), (600, 65, 2, 10, 0), (301, 2, 7, 2, 0)]  # m, k, blobs, min_samples, duplicated


@pytest.mark.parametrize("m,k,blobs,min_samples,duplicated", CASES)
def test_model_equals_scipy(m, k, blobs, min_samples, duplicated):
    ids, dists = blob_lists(m, k, blobs, duplicated)
    forest, labels, core = model_forest(ids, dists, min_samples)
    i, j, w, _ = live_edges(ids, dists, min_samples)
    dense = np.full((m, m), np.inf, dtype=np.float32)
    np.minimum.at(dense, (i, j), w)
    dense = np.minimum(dense, dense.T)  # the min-combined symmetric matrix
    assert (w > 0).all() and (min_samples == 0) == (not core.any())
    graph = sp.csr_array(np.where(np.isfinite(dense), dense, 0))
    n, want = connected_components(graph, directed=False)
    assert n >= blobs and np.array_equal(labels, want)
    tree = np.sort(minimum_spanning_tree(graph.astype(np.float64)).data.astype(np.float32))
    assert forest.nnz == 2 * (m - n) and np.array_equal(np.sort(sp.triu(forest).data), tree)  # the weight multiset is unique
    if min_samples >= 5:
        assert len(np.unique(tree)) < len(tree)  # mutual reachability ties
    assert (forest != forest.T).nnz == 0


def _host_index(n=50, k=5):
    """An index that needs no GPU: NNDescent.from_graph wraps an existing graph."""
    from pynndescent_amd import NNDescent

    x = np.random.RandomState(0).standard_normal((n, 4)).astype(np.float32)
    idx = (np.arange(n, dtype=np.int32)[:, None] + np.arange(k, dtype=np.int32)[None, :]) % n
    dist = np.tile(np.arange(k, dtype=np.float32), (n, 1))
    return NNDescent.from_graph(x, idx, dist, random_state=1), idx, dist


def test_argument_errors_come_before_any_device_work():
    from pynndescent_amd import spanning_forest

    index, idx, dist = _host_index()
    for bad in ({"min_samples": 6}, {"min_samples": -1}, {"n_neighbors": 0}, {"n_neighbors": 6}):
        with pytest.raises(ValueError, match="min_samples|n_neighbors"):
            index.spanning_forest(**bad)
    with pytest.raises(ValueError, match="min_samples"):
        spanning_forest(idx, dist, min_samples=6)
    with pytest.raises(ValueError, match="n_neighbors"):
        spanning_forest(np.zeros((3, 257), np.int32), np.zeros((3, 257), np.float32))
    with pytest.raises(ValueError, match="n_neighbors"):
        spanning_forest(idx[:, :0], dist[:, :0], min_samples=0)
    with pytest.raises(ValueError, match="one shape"):  # mismatched shapes, and not (m, k)
        spanning_forest(idx, dist[:, :4])
    with pytest.raises(ValueError, match="one shape"):
        spanning_forest(idx[0], dist[0])
    with pytest.raises(ValueError, match="int32 or int64"):
        spanning_forest(idx.astype(np.float32), dist)
    with pytest.raises(ValueError, match="float32"):
        spanning_forest(idx, dist.astype(np.float64))
