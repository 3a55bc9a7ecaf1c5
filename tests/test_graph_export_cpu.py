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


def test_model_takes_an_id_outside_the_columns_as_an_empty_place():
    ids = np.array([[2, 4, 1], [7, -7, 2 ** 31 - 1], [0, 1, 2]], np.int64)
    ids[2, 1] = 2 ** 32 + 1  # (a narrowing cast would make it column 1)
    vals = np.arange(9, dtype=np.float32).reshape(3, 3)
    cleaned = np.where((ids >= 0) & (ids < 4), ids, -1)
    for kwargs in ({}, {"drop_self": True}):
        got, want = model_csr(ids, vals, 4, **kwargs), model_csr(cleaned, vals, 4, **kwargs)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert model_csr(ids, vals, 4)[0].tolist() == [0, 2, 2, 4] and model_csr(ids, vals, 4)[1].tolist() == [1, 2, 0, 2]
    sq = np.where((ids >= 0) & (ids < 3), ids, -1)
    assert all(np.array_equal(g, w) for g, w in zip(model_csr(ids, vals, 3, symmetric=True), model_csr(sq, vals, 3, symmetric=True)))


def test_model_keeps_the_smaller_bits_of_two_equal_floats():
    ids = np.array([[1, 2], [0, -1], [0, -1]], np.int32)
    for first, second in ((0.0, -0.0), (-0.0, 0.0)):
        vals = np.array([[first, -2.0], [second, 9], [2.0, 9]], np.float32)
        indptr, indices, data = model_csr(ids, vals, 3, symmetric=True)
        assert indptr.tolist() == [0, 2, 3, 4] and indices.tolist() == [1, 2, 0, 0]
        assert data.view(np.uint32).tolist() == [0, np.float32(-2.0).view(np.uint32), 0, np.float32(-2.0).view(np.uint32)]  # +0.0; -2 < 2


# ---- the cases of the width tests reach what they are written for (tests/graph_export_cases.py)
from tests import graph_export_cases as GC  # noqa: E402


@pytest.mark.parametrize("name", sorted(GC.SYMMETRIC))
def test_symmetric_cases_have_their_designated_lengths_and_twins(name):
    case, ids = GC.SYMMETRIC[name], GC.sym_lists(name)
    lengths = GC.stretch_lengths(ids, case.n, case.k)
    assert np.array_equal(lengths, GC.stretch_lengths(ids, case.n, case.k, drop_self=True))
    print("%s: rows per merge instance %s = %s" % (name, list(GC.MERGE_INSTANCES), GC.instance_counts(ids, case.n, case.k)))
    for row, length in (case.lengths or {}).items():
        assert lengths[row] == length, (row, length, lengths[row])
    # no row holds an id twice
    filled = np.sort(np.where(ids >= 0, ids.astype(np.int64), -1 - np.arange(case.k, dtype=np.int64)[None, :]), axis=1)
    assert (filled[:, 1:] != filled[:, :-1]).all()
    for which in GC.VALUE_SETS:
        vals = GC.sym_values(name, which)
        assert vals.dtype == np.float32 and vals.shape == ids.shape and not np.isnan(vals).any()
        for row, position in case.mutual:
            found = GC.twin_positions(ids, vals, case.n, row)
            if position < 0:
                position += len(GC.sorted_stretch(ids, vals, case.n, row)[0])
            print("%s / %s: row %d (length %d, %s) has twins at %s" % (name, which, row, lengths[row], GC.merge_instance(lengths[row]), found))
            assert position in found, (row, position, found)
    if case.lengths:  # a designated row keeps empty places
        assert all((ids[row] < 0).any() for row in case.lengths)


def test_symmetric_cases_reach_every_merge_instance_and_boundary():
    reached, lengths = {}, set()
    for name, case in GC.SYMMETRIC.items():
        here = GC.stretch_lengths(GC.sym_lists(name), case.n, case.k)
        lengths |= set(here.tolist())
        for inst, rows in zip(GC.MERGE_INSTANCES, GC.instance_counts(GC.sym_lists(name), case.n, case.k)):
            reached[inst] = reached.get(inst, 0) + rows
    print("rows per merge instance over all cases: %s" % reached)
    print("boundary lengths reached: %s" % sorted(set(GC.BOUNDARY_LENGTHS) & lengths))
    assert all(reached[inst] > 0 for inst in GC.MERGE_INSTANCES)
    assert set(GC.BOUNDARY_LENGTHS) <= lengths
    assert [GC.merge_instance(v) for v in GC.BOUNDARY_LENGTHS] == [16, 32, 32, 64, 64, 128, 128, 256, 256, 512, 512, "long"]
    many = GC.SYMMETRIC["many_long_k256"]
    assert GC.instance_counts(GC.sym_lists("many_long_k256"), many.n, many.k)[-1] > GC.LONG_GRID
    tiny = GC.stretch_lengths(GC.sym_lists("tiny_k1"), 40, 1)
    assert tiny.tolist() == [40] + [1] * 39


def test_designed_twins_of_the_signed_values_need_the_second_key():
    """On every designed pair the two directions differ, and the smaller float is the one the sort puts second."""
    for name, case in GC.SYMMETRIC.items():
        ids, vals = GC.sym_lists(name), GC.sym_values(name, "signed")
        pairs = GC.designed_pairs(name)
        assert len(pairs) == len(case.mutual)
        for row, _ in pairs:
            cols, bits = GC.sorted_stretch(ids, vals, case.n, row)
            for p in GC.twin_positions(ids, vals, case.n, row):
                a, b = bits[p : p + 2].astype(np.uint32).view(np.float32)
                assert bits[p] < bits[p + 1] and b < a, (name, row, p, a, b)


def test_signed_values_are_what_they_claim():
    ids = GC.sym_lists("many_long_k256")
    vals = GC.signed_values(ids, seed=3)
    i = np.arange(800)[:, None]
    assert (vals[ids == i] == 0).all() and not np.isnan(vals).any()
    off = vals[ids != i]
    assert (off < 0).any() and (off > 0).any() and (off == 0).any() and (off == np.float32(3e38)).any()
    assert ((off.view(np.uint32) & 0x7FFFFFFF) == GC.SUBNORMAL_BITS).any() and 0 < GC.SUBNORMAL_BITS < 0x00800000  # below the normals
    # the two directions of a mutual pair: equal bits on most, on about a tenth one ulp, the sign, or the sign of zero
    back = np.full((800, 800), -1, np.int64)
    back[i, ids] = np.arange(256)[None, :]
    there = back[ids, i]  # the place of row ids[i, e] that names i
    mutual = (there >= 0) & (ids != i)
    a, b = vals[mutual], vals[ids[mutual], there[mutual]]
    same = a.view(np.uint32) == b.view(np.uint32)
    share = 1.0 - same.mean()
    print("mutual places %d, differing share %.3f" % (mutual.sum(), share))
    assert 0.05 < share < 0.15
    ulp = ~same & (np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) == 1)
    magnitude_a, magnitude_b = a.view(np.uint32) & 0x7FFFFFFF, b.view(np.uint32) & 0x7FFFFFFF
    zeros = ~same & (magnitude_a == 0) & (magnitude_b == 0)
    sign = ~same & (magnitude_a == magnitude_b) & (magnitude_a != 0)
    assert ulp.any() and zeros.any() and sign.any() and (same | ulp | zeros | sign).all()


def test_directed_cases_reach_every_write_instance_with_both_id_types():
    reached = sorted({GC.write_instance(k) + (np.dtype(t).name,) for _, k, _, t, _ in GC.DIRECTED})
    print("k_csr_write_rows instances (KU, W, IdT): %s" % reached)
    assert reached == sorted(inst + (t,) for inst in GC.WRITE_INSTANCES for t in ("int32", "int64"))
    assert [GC.write_instance(k) for k in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256)] == [
        (1, 16), (1, 16), (1, 32), (1, 32), (1, 64), (1, 64), (2, 64), (2, 64), (4, 64), (4, 64)]
    for m, k, n, t, empty in GC.DIRECTED:
        ids, vals = GC.directed_lists(m, k, n, t, empty)
        assert ids.shape == (m, k) and ids.dtype == t and (vals < 0).any()
        assert ((ids < 0).any()) == (empty > 0) and (ids >= 0).any()
    assert any(m % (64 // GC.write_instance(k)[1]) for m, k, _, _, _ in GC.DIRECTED if GC.write_instance(k)[1] == 32)


def _dense_union(ids, vals, n):
    """The symmetric form the long way: an n x n array of nothing, the elementwise minimum over both directions (of two equal
    floats the smaller bits), read out by column.  A float is compared as its sign and magnitude, read from its bits (finite
    floats order like those integers, and both zeros are 0), which no floating-point mode of the process changes."""
    dense = np.zeros((n, n), np.uint32)
    there = np.zeros((n, n), bool)
    number = lambda b: -(b & 0x7FFFFFFF) if b >> 31 else b  # noqa: E731
    for i in range(n):
        for j, b in zip(ids[i].tolist(), vals[i].view(np.uint32).tolist()):
            if 0 <= j < n:
                for r, c in ((i, j), (j, i)):
                    cur = int(dense[r, c])
                    if not there[r, c] or number(b) < number(cur) or (number(b) == number(cur) and b < cur):
                        dense[r, c], there[r, c] = b, True
    indptr, indices, data = [0], [], []
    for i in range(n):
        cols = np.nonzero(there[i])[0]
        indices += cols.tolist()
        data.append(dense[i, cols])
        indptr.append(len(indices))
    return np.asarray(indptr, np.int64), np.asarray(indices, np.int32), np.concatenate(data).view(np.float32)


def test_model_equals_a_dense_construction_on_signed_values():
    n, k = 60, 12
    ids = GC.designed_klists(n, k, {5: 40, 17: 12, 33: 13}, [(5, 20)], seed=2)
    ids = ids.copy()
    ids[7, 3], ids[44, 0] = n + 5, -7  # ids that name no column
    pairs = [(i, int(j)) for i in range(n) for j in ids[i] if 0 <= j < n and j > i and (ids[j] == i).any()]
    assert len(pairs) > 20
    vals = GC.signed_values(ids, seed=5, differ=pairs[::2])
    want = _dense_union(ids, vals, n)
    got = model_csr(ids, vals, n, symmetric=True)
    for g, w, name in zip(got, want, ("indptr", "indices", "data")):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32) if name == "data" else g, w.view(np.uint32) if name == "data" else w), name
    assert (got[2] < 0).any() and (got[2] == 0).any()
