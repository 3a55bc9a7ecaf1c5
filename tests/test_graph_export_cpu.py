"""Graph export without a GPU: the transformer's signature, the argument errors of kneighbors_graph, the C ABI's new names,
and the host model every GPU test of the export compares against (tests/graph_export_util.py) on hand-written cases."""
import inspect
import os
import re

import numpy as np
import pytest

from tests.graph_export_util import model_csr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# pynndescent_.py:2709-2729: names, order and defaults of PyNNDescentTransformer.__init__
REFERENCE_ARGUMENTS = [
    ("n_neighbors", 30), ("metric", "euclidean"), ("metric_kwds", None), ("n_trees", None), ("leaf_size", None),
    ("search_epsilon", 0.1), ("pruning_degree_multiplier", 1.5), ("diversify_prob", 1.0), ("n_search_trees", 1),
    ("tree_init", True), ("random_state", None), ("n_jobs", None), ("low_memory", True), ("max_candidates", None),
    ("n_iters", None), ("early_termination_value", 0.001), ("parallel_batch_queries", False), ("verbose", False),
]


def test_transformer_signature_and_attributes_match_the_reference():
    from pynndescent_amd import PyNNDescentTransformer

    params = list(inspect.signature(PyNNDescentTransformer.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == REFERENCE_ARGUMENTS
    t = PyNNDescentTransformer()
    for name, default in REFERENCE_ARGUMENTS:
        assert getattr(t, name) == default, name
    given = {name: i + 2 for i, (name, _) in enumerate(REFERENCE_ARGUMENTS)}
    t = PyNNDescentTransformer(**given)
    for name, value in given.items():
        assert getattr(t, name) == value, name
    assert list(inspect.signature(PyNNDescentTransformer.fit).parameters)[1:] == ["X", "compress_index"]
    assert inspect.signature(PyNNDescentTransformer.fit).parameters["compress_index"].default is True
    for method in ("fit", "transform", "fit_transform", "get_params", "set_params"):
        assert callable(getattr(t, method))


def test_transformer_parameters_round_trip():
    from pynndescent_amd import PyNNDescentTransformer

    t = PyNNDescentTransformer(n_neighbors=7, metric="cosine", random_state=3)
    params = t.get_params()
    assert sorted(params) == sorted(name for name, _ in REFERENCE_ARGUMENTS)
    assert params["n_neighbors"] == 7 and params["metric"] == "cosine" and params["random_state"] == 3
    assert t.set_params(n_neighbors=9) is t and t.n_neighbors == 9
    with pytest.raises(ValueError):
        t.set_params(no_such_parameter=1)
    try:
        from sklearn.base import clone
    except ImportError:
        return
    assert clone(t).get_params() == t.get_params()


def _host_index(n=50, k=5):
    """An index that needs no GPU: NNDescent.from_graph wraps an existing graph."""
    from pynndescent_amd import NNDescent

    x = np.random.RandomState(0).standard_normal((n, 4)).astype(np.float32)
    idx = (np.arange(n, dtype=np.int32)[:, None] + np.arange(k, dtype=np.int32)[None, :]) % n
    dist = np.tile(np.arange(k, dtype=np.float32), (n, 1))
    return NNDescent.from_graph(x, idx, dist, random_state=1), x


def test_kneighbors_graph_argument_errors_come_before_any_device_work():
    index, x = _host_index()
    with pytest.raises(ValueError, match="symmetric"):
        index.kneighbors_graph(x[:3], k=2, symmetric=True)
    with pytest.raises(ValueError, match="include_self"):
        index.kneighbors_graph(x[:3], k=2, include_self=False)
    with pytest.raises(ValueError, match="mode"):
        index.kneighbors_graph(mode="similarity")
    with pytest.raises(ValueError, match="mode"):
        index.kneighbors_graph(x[:3], k=2, mode="similarity")
    with pytest.raises(ValueError, match="n_neighbors"):
        index.kneighbors_graph(k=index.n_neighbors + 1)
    with pytest.raises(ValueError, match="at least 1"):
        index.kneighbors_graph(k=0)
    with pytest.raises(TypeError, match="filter"):
        index.kneighbors_graph(filter=np.arange(3))


def test_new_symbols_are_declared_and_bound():
    from pynndescent_amd import _capi

    header = open(os.path.join(ROOT, "include", "pynnd_amd.h")).read()
    lib = _capi.load_library()
    for name in ("nnd_graph_csr", "nnd_graph_csr_device", "nnd_csr_arrays", "nnd_csr_destroy"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.nnd_abi_version() == 6
    assert (_capi.NND_CSR_DISTANCE, _capi.NND_CSR_CONNECTIVITY, _capi.NND_CSR_DROP_SELF) == tuple(
        int(re.search(r"#define %s (\d+)" % n, header).group(1)) for n in ("NND_CSR_DISTANCE", "NND_CSR_CONNECTIVITY", "NND_CSR_DROP_SELF"))


# ---- the model, on 4 x 3 k-lists written out by hand (n = 4 columns)
IDS = np.array([[2, 0, 1],
                [-1, 3, -1],
                [-1, -1, -1],
                [0, -1, 3]], np.int32)
VALS = np.array([[0.5, 0.0, 0.25],
                 [9.0, 0.75, 9.0],
                 [9.0, 9.0, 9.0],
                 [0.125, 9.0, 0.0]], np.float32)


def test_model_directed_by_hand():
    indptr, indices, data = model_csr(IDS, VALS, 4)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and data.dtype == np.float32
    assert indptr.tolist() == [0, 3, 4, 4, 6]
    assert indices.tolist() == [0, 1, 2, 3, 0, 3]
    assert data.tolist() == [0.0, 0.25, 0.5, 0.75, 0.125, 0.0]
    indptr, indices, data = model_csr(IDS, VALS, 4, mode="connectivity")
    assert indptr.tolist() == [0, 3, 4, 4, 6] and indices.tolist() == [0, 1, 2, 3, 0, 3] and data.tolist() == [1.0] * 6
    indptr, indices, data = model_csr(IDS, VALS, 4, drop_self=True)
    assert indptr.tolist() == [0, 2, 3, 3, 4] and indices.tolist() == [1, 2, 3, 0] and data.tolist() == [0.25, 0.5, 0.75, 0.125]


def test_model_symmetric_by_hand():
    # edges: 0-2 (.5), 0-0 (0), 0-1 (.25), 1-3 (.75), 3-0 (.125), 3-3 (0); row 2 lists nobody and is reached through 0 alone
    indptr, indices, data = model_csr(IDS, VALS, 4, symmetric=True)
    assert indptr.tolist() == [0, 4, 6, 7, 10]
    assert indices.tolist() == [0, 1, 2, 3, 0, 3, 0, 0, 1, 3]
    assert data.tolist() == [0.0, 0.25, 0.5, 0.125, 0.25, 0.75, 0.5, 0.125, 0.75, 0.0]


def test_model_symmetric_takes_the_min_of_a_mutual_pair():
    ids = np.array([[1, -1, -1], [0, 2, -1], [-1, -1, -1], [-1, -1, -1]], np.int32)
    lo = np.float32(0.3)
    hi = np.nextafter(lo, np.float32(1.0))
    vals = np.array([[hi, 9, 9], [lo, 0.5, 9], [9, 9, 9], [9, 9, 9]], np.float32)
    indptr, indices, data = model_csr(ids, vals, 4, symmetric=True)
    assert indptr.tolist() == [0, 1, 3, 4, 4] and indices.tolist() == [1, 0, 2, 1]
    assert data[0] == lo and data[1] == lo and data[0] != hi and data.tolist()[2:] == [0.5, 0.5]
    assert model_csr(ids, vals, 4, mode="connectivity", symmetric=True)[2].tolist() == [1.0] * 4
