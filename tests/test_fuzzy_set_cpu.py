"""The fuzzy simplicial set without a GPU: the argument errors of both entry points and the C ABI's new names."""
import os
import re
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENTS = [
    ({"local_connectivity": 0.0}, "local_connectivity"), ({"local_connectivity": 4.5}, "local_connectivity"),
    ({"bandwidth": 0.0}, "bandwidth"), ({"set_op_mix_ratio": -0.1}, "set_op_mix_ratio"), ({"set_op_mix_ratio": 1.5}, "set_op_mix_ratio"),
]


def _host_index(n=50, k=5):
    """An index that needs no GPU: NNDescent.from_graph wraps an existing graph."""
    from pynndescent_amd import NNDescent

    x = np.random.RandomState(0).standard_normal((n, 4)).astype(np.float32)
    idx = (np.arange(n, dtype=np.int32)[:, None] + np.arange(k, dtype=np.int32)[None, :]) % n
    dist = np.tile(np.arange(k, dtype=np.float32), (n, 1))
    return NNDescent.from_graph(x, idx, dist, random_state=1), idx, dist


@pytest.mark.parametrize("kwargs,match", BAD_ARGUMENTS)
def test_argument_errors_come_before_any_device_work(kwargs, match):
    from pynndescent_amd import fuzzy_simplicial_set

    index, idx, dist = _host_index()
    with pytest.raises(ValueError, match=match):
        index.fuzzy_simplicial_set(**kwargs)
    with pytest.raises(ValueError, match=match):
        fuzzy_simplicial_set(idx, dist, **kwargs)


def test_shape_errors():
    from pynndescent_amd import fuzzy_simplicial_set

    index, idx, dist = _host_index()
    for k in (1, 6):  # below 2, and more columns than the graph has
        with pytest.raises(ValueError, match="n_neighbors"):
            index.fuzzy_simplicial_set(n_neighbors=k)
    with pytest.raises(ValueError, match="n_neighbors"):
        fuzzy_simplicial_set(idx[:, :1], dist[:, :1])
    with pytest.raises(ValueError, match="n_neighbors"):
        fuzzy_simplicial_set(np.zeros((3, 257), np.int32), np.zeros((3, 257), np.float32))
    with pytest.raises(ValueError, match="square"):
        fuzzy_simplicial_set(idx[:20], dist[:20], n_points=50)
    index.compressed = True
    del index._neighbor_graph
    with warnings.catch_warnings(), pytest.raises(ValueError, match="compressed"):
        warnings.simplefilter("ignore")
        index.fuzzy_simplicial_set()


def test_new_symbols_are_declared_and_bound():
    from pynndescent_amd import _capi

    header = open(os.path.join(ROOT, "include", "pynnd_amd.h")).read()
    lib = _capi.load_library()
    for name in ("nnd_fuzzy_set", "nnd_fuzzy_set_device"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
