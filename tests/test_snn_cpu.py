"""The shared-neighbour graph without a GPU: the set model on an example counted by hand, and the argument errors of both entry
points."""
import numpy as np
import pytest

from tests.snn_util import model_snn

# O: {1, 2}, {0, 2}, {3} (lists itself), {4} (listed twice), {} (an id past the end, an empty place)
IDS = np.array([[1, 2], [0, 2], [3, 2], [4, 4], [7, -1]], dtype=np.int32)
# with the rows themselves: {0, 1, 2}, {0, 1, 2}, {2, 3}, {3, 4}, {4}
WITH_SELF = {(0, 1): (3, 3), (0, 2): (1, 4), (1, 0): (3, 3), (1, 2): (1, 4), (2, 3): (1, 3), (3, 4): (1, 2)}  # edge: (c, u)
WITHOUT = {(0, 1): (1, 3), (1, 0): (1, 3)}  # every other edge shares nothing and vanishes


def entries(a):
    return {(i, int(a.indices[p])): a.data[p] for i in range(a.shape[0]) for p in range(a.indptr[i], a.indptr[i + 1])}


def test_model_on_a_hand_counted_example():
    assert entries(model_snn(IDS, "count", True, 0.0, False)) == {e: np.float32(c) for e, (c, u) in WITH_SELF.items()}
    assert entries(model_snn(IDS, "jaccard", True, 0.0, False)) == {e: np.float32(c / u) for e, (c, u) in WITH_SELF.items()}
    assert entries(model_snn(IDS, "jaccard", False, 0.0, False)) == {e: np.float32(1 / 3) for e in WITHOUT}
    both = {**WITH_SELF, **{(j, i): cu for (i, j), cu in WITH_SELF.items()}}
    got = model_snn(IDS, "jaccard", True, 0.0, True)
    assert entries(got) == {e: np.float32(c / u) for e, (c, u) in both.items()} and len(both) == 10
    assert got.has_canonical_format and got.data.dtype == np.float32 and got.indices.dtype == np.int32 and (got.diagonal() == 0).all()
    kept = {e: np.float32(c / u) for e, (c, u) in WITH_SELF.items() if c / u >= 0.3}  # 1/4 goes, 1/3 stays
    assert entries(model_snn(IDS, "jaccard", True, 0.3, False)) == kept and len(kept) == 4


def _host_index(n=50, k=5):
    """An index that needs no GPU: NNDescent.from_graph wraps an existing graph."""
    from pynndescent_amd import NNDescent

    x = np.random.RandomState(0).standard_normal((n, 4)).astype(np.float32)
    idx = (np.arange(n, dtype=np.int32)[:, None] + np.arange(k, dtype=np.int32)[None, :]) % n
    return NNDescent.from_graph(x, idx, np.tile(np.arange(k, dtype=np.float32), (n, 1)), random_state=1), idx


@pytest.mark.parametrize("kwargs,match", [({"weight": "rank"}, "weight"), ({"prune": -0.5}, "prune"), ({"prune": float("nan")}, "prune")])
def test_argument_errors_come_before_any_device_work(kwargs, match):
    from pynndescent_amd import shared_neighbor_graph

    index, idx = _host_index()
    with pytest.raises(ValueError, match=match):
        index.shared_neighbor_graph(**kwargs)
    with pytest.raises(ValueError, match=match):
        shared_neighbor_graph(idx, **kwargs)


def test_shape_and_type_errors():
    from pynndescent_amd import shared_neighbor_graph

    index, idx = _host_index()
    for k in (1, 6):  # below 2, and more columns than the graph has
        with pytest.raises(ValueError, match="n_neighbors"):
            index.shared_neighbor_graph(n_neighbors=k)
    for bad in (idx[:, :1], np.zeros((3, 257), np.int32)):
        with pytest.raises(ValueError, match="n_neighbors"):
            shared_neighbor_graph(bad)
    with pytest.raises(ValueError, match="(m, k)"):
        shared_neighbor_graph(idx[0])
    with pytest.raises(ValueError, match="int32 or int64"):
        shared_neighbor_graph(idx.astype(np.float32))
