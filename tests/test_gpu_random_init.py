"""init_random on a real MI355X: the kernel that lets one wave screen 64 rows must leave the k-lists that one wave per row
(NND_FLAG_TEST_RANDOM_INIT_ROWWISE, the earlier form) leaves -- same picks, same distances, same flags."""
import numpy as np
import pytest

from pynndescent_amd import _capi
from tests.gpu_util import make_builder
from tests.util_data import clustered

pytestmark = pytest.mark.gpu

N = 130  # two full groups of 64 rows and two rows of a third


def _partial_graph(k):
    """rows that are full, rows with holes anywhere in the row, empty rows: ids unique within a row"""
    rs = np.random.RandomState(k)
    g = np.stack([rs.permutation(N)[:k] for _ in range(N)]).astype(np.int32)
    g[rs.rand(N, k) < 0.3] = -1
    g[::7] = -1                                                 # empty rows
    full = np.arange(3, N, 5)
    g[full] = np.stack([rs.permutation(N)[:k] for _ in full])   # full rows, the last row (129) not among them
    g[64:128:2] = np.stack([rs.permutation(N)[:k] for _ in range(32)])  # and a group of 64 with every other row full
    return g


def _lists(x, metric, k, graph, flags):
    b = make_builder(x, metric, k=k, n_trees=0, flags=flags)
    if graph is not None:
        b.init_from_graph(graph)
    before = b.graph()[0].copy()
    b.init_random()
    out = tuple(np.array(a, copy=True) for a in b.graph())
    b.close()
    return before, out


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
@pytest.mark.parametrize("start", ["empty", "partial"])
@pytest.mark.parametrize("k", [3, 15, 40])
def test_screening_wave_leaves_the_rowwise_lists(k, start, metric):
    x = clustered(N, 12, 3, 8, seed=k)
    graph = _partial_graph(k) if start == "partial" else None
    before, (idx, dist, fl) = _lists(x, metric, k, graph, 0)
    _, (idx_r, dist_r, fl_r) = _lists(x, metric, k, graph, _capi.NND_FLAG_TEST_RANDOM_INIT_ROWWISE)
    np.testing.assert_array_equal(idx, idx_r)
    np.testing.assert_array_equal(dist.view(np.uint32), dist_r.view(np.uint32))
    np.testing.assert_array_equal(fl, fl_r)
    # rows that were full keep their lists, rows that were not drew: nothing is skipped, nothing is drawn for nothing
    was_full = (before >= 0).all(1)
    if start == "partial":
        assert was_full.any() and not was_full.all()
        assert np.array_equal(np.sort(idx[was_full], 1), np.sort(before[was_full], 1))
    grew = (idx >= 0).sum(1) > (before >= 0).sum(1)
    assert grew[~was_full].mean() > 0.9  # (a row short of one entry can draw an id it already holds)
