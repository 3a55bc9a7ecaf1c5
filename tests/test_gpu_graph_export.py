"""Graph export on the GPU (csrc/csr_graph.hip, pynndescent_amd/graph_export.py): the kernels against the host model of
tests/graph_export_util.py bit for bit, then kneighbors_graph and PyNNDescentTransformer on small indexes."""
import numpy as np
import pytest

from pynndescent_amd import _capi
from tests.graph_export_cases import merge_instance, stretch_lengths
from tests.graph_export_util import assert_same_csr, model_csr, random_klists, symmetric_values

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. directed form, kernel level
# (m, k, n): the lane-packing boundaries 64 / 65 and 128 / 129, and the cap
DIRECTED_SHAPES = [(1, 1, 1), (3, 5, 7), (130, 64, 200), (130, 65, 200), (70, 128, 300), (40, 129, 300), (33, 256, 400)]


@pytest.mark.parametrize("m,k,n", DIRECTED_SHAPES)
@pytest.mark.parametrize("mode", ["distance", "connectivity"])
def test_directed_form_equals_the_model(m, k, n, mode):
    ids, vals = random_klists(m, k, n, seed=m * 1000 + k)
    if m == 1:
        ids[:] = 0  # (the one place of the 1 x 1 case is filled)
    assert_same_csr(_capi.graph_csr(ids, vals, n, mode=mode), model_csr(ids, vals, n, mode=mode))


def test_directed_form_of_empty_lists_has_no_entries():
    ids = np.full((37, 20), -1, np.int32)
    vals = np.full((37, 20), np.inf, np.float32)
    indptr, indices, data = _capi.graph_csr(ids, vals, 50)
    assert indptr.dtype == np.int64 and indptr.tolist() == [0] * 38 and indices.shape == (0,) and data.shape == (0,)


def test_directed_form_takes_int64_ids_and_drops_the_diagonal():
    ids, vals = random_klists(90, 70, 150, seed=11, id_dtype=np.int64)
    ids[np.arange(90), np.arange(90) % 70] = np.arange(90)  # a diagonal entry per row, at different places
    for i in range(90):  # (the row must not hold its own id twice)
        dup = np.nonzero(ids[i] == i)[0]
        ids[i, dup[dup != i % 70]] = -1
    assert ids.dtype == np.int64
    assert_same_csr(_capi.graph_csr(ids, vals, 150), model_csr(ids, vals, 150))
    got = _capi.graph_csr(ids, vals, 150, drop_self=True)
    assert_same_csr(got, model_csr(ids, vals, 150, drop_self=True))
    assert got[0][-1] == model_csr(ids, vals, 150)[0][-1] - 90


# ------------------------------------------------------------------------------------------------ 2. symmetric form, kernel level
@pytest.mark.parametrize("n", [1, 2, 50, 600])
@pytest.mark.parametrize("k", [1, 15, 64])
def test_symmetric_form_equals_the_model(n, k):
    if k > n:
        k_eff, pad = n, k - n  # fewer ids than places exist: the remaining places are empty
    else:
        k_eff, pad = k, 0
    ids, _ = random_klists(n, k_eff, n, seed=n * 100 + k)
    ids = np.concatenate([ids, np.full((n, pad), -1, np.int32)], axis=1)
    vals = symmetric_values(ids)
    for mode in ("distance", "connectivity"):
        got = _capi.graph_csr(ids, vals, n, mode=mode, symmetric=True, want_long_rows=True)
        assert_same_csr(got[:3], model_csr(ids, vals, n, mode=mode, symmetric=True))
    assert_same_csr(_capi.graph_csr(ids, vals, n, symmetric=True, drop_self=True), model_csr(ids, vals, n, symmetric=True, drop_self=True))


def _hub_lists(n=600, k=15):
    rs = np.random.RandomState(5)
    ids = np.stack([1 + rs.permutation(n - 1)[:k] for _ in range(n)]).astype(np.int32)
    ids[:, 3] = 0  # every row lists vertex 0 (row 0 too: its diagonal)
    return ids, symmetric_values(ids)


def test_symmetric_hub_row_takes_the_long_path_and_is_deterministic():
    ids, vals = _hub_lists()
    want = model_csr(ids, vals, 600, symmetric=True)
    assert want[0][1] - want[0][0] > 256  # row 0 of the union: everybody
    first = _capi.graph_csr(ids, vals, 600, symmetric=True, want_long_rows=True)
    assert first[3] == sum(merge_instance(int(v)) == "long" for v in stretch_lengths(ids, 600, 15)) == 1
    assert_same_csr(first[:3], want)
    second = _capi.graph_csr(ids, vals, 600, symmetric=True, want_long_rows=True)  # (the scatter order may differ between runs)
    for a, b in zip(first[:3], second[:3]):
        assert a.tobytes() == b.tobytes()
    assert second[3] == first[3]


def test_symmetric_mutual_pair_holds_the_min_on_both_sides():
    ids, _ = random_klists(50, 8, 50, seed=3, empty=0.0, empty_rows=0.0)
    vals = symmetric_values(ids)
    ids[4, 0], ids[9, 0] = 9, 4  # a mutual pair whose two values differ in the last bit
    for r, other in ((4, 9), (9, 4)):
        ids[r, 1:][ids[r, 1:] == other] = -1
    lo = np.float32(0.37)
    hi = np.nextafter(lo, np.float32(1.0))
    vals[4, 0], vals[9, 0] = hi, lo
    indptr, indices, data = got = _capi.graph_csr(ids, vals, 50, symmetric=True)
    assert_same_csr(got, model_csr(ids, vals, 50, symmetric=True))
    for r, c in ((4, 9), (9, 4)):
        row = slice(indptr[r], indptr[r + 1])
        at = np.nonzero(indices[row] == c)[0]
        assert at.shape == (1,) and data[row][at[0]] == lo and data[row][at[0]] != hi


# ------------------------------------------------------------------------------------------------ 3.-5. class level
N, DIM, NQ = 2000, 16, 300


@pytest.fixture(scope="module")
def rows():
    rs = np.random.RandomState(42)
    return rs.standard_normal((N, DIM)).astype(np.float32), rs.standard_normal((NQ, DIM)).astype(np.float32)


@pytest.fixture(scope="module", params=["euclidean", "cosine"])
def indexes(request, rows):
    """(metric, host index, device index) on the same rows, built once per metric."""
    import torch

    from pynndescent_amd import NNDescent

    x = rows[0]
    host = NNDescent(x, metric=request.param, n_neighbors=10, random_state=0)
    device = NNDescent(torch.from_numpy(x).cuda(), metric=request.param, n_neighbors=10, random_state=0)
    return request.param, host, device


def _parts(t):
    """The three arrays of a torch sparse_csr tensor, on the host."""
    return t.crow_indices().cpu().numpy(), t.col_indices().cpu().numpy(), t.values().cpu().numpy()


def _scipy_parts(a):
    return a.indptr, a.indices, a.data


def _host_lists(graph):
    ids, vals = graph
    if hasattr(ids, "cpu"):
        ids, vals = ids.cpu().numpy(), vals.cpu().numpy()
    return ids, vals.astype(np.float32)


def test_kneighbors_graph_of_a_host_index(indexes):
    import scipy.sparse as sp

    _, index, _ = indexes
    ids, vals = _host_lists(index.neighbor_graph)
    g = index.kneighbors_graph()
    assert isinstance(g, sp.csr_array) and g.shape == (N, N) and g.data.dtype == np.float32 and g.indices.dtype == np.int32
    assert g.has_sorted_indices and g.has_canonical_format
    assert_same_csr(_scipy_parts(g), model_csr(ids, vals, N))
    assert_same_csr(_scipy_parts(index.kneighbors_graph(mode="connectivity")), model_csr(ids, vals, N, mode="connectivity"))
    assert_same_csr(_scipy_parts(index.kneighbors_graph(symmetric=True)), model_csr(ids, vals, N, symmetric=True))
    assert_same_csr(_scipy_parts(index.kneighbors_graph(k=4)), model_csr(ids[:, :4], vals[:, :4], N))
    no_self = index.kneighbors_graph(include_self=False)
    assert_same_csr(_scipy_parts(no_self), model_csr(ids, vals, N, drop_self=True))
    assert (no_self.diagonal() == 0).all() and no_self.nnz == g.nnz - int((ids == np.arange(N)[:, None]).sum())
    full, kept = g.tocoo(), no_self.tocoo()
    dropped = set(zip(full.row.tolist(), full.col.tolist())) - set(zip(kept.row.tolist(), kept.col.tolist()))
    assert dropped and all(i == j for i, j in dropped)


def test_kneighbors_graph_of_a_device_index(indexes):
    import torch

    _, _, index = indexes
    ids, vals = _host_lists(index.neighbor_graph)
    g = index.kneighbors_graph()
    assert g.layout == torch.sparse_csr and g.device == index._device_data.device and tuple(g.shape) == (N, N)
    assert g.values().dtype == torch.float32 and g.col_indices().dtype == torch.int32
    assert_same_csr(_parts(g), model_csr(ids, vals, N))
    assert_same_csr(_parts(index.kneighbors_graph(symmetric=True)), model_csr(ids, vals, N, symmetric=True))
    assert_same_csr(_parts(index.kneighbors_graph(k=4)), model_csr(ids[:, :4], vals[:, :4], N))
    assert_same_csr(_parts(index.kneighbors_graph(k=4, mode="connectivity", symmetric=True)),
                    model_csr(ids[:, :4], vals[:, :4], N, mode="connectivity", symmetric=True))
    assert_same_csr(_parts(index.kneighbors_graph(include_self=False)), model_csr(ids, vals, N, drop_self=True))
    # the tensor's parts outlive the call that made them (they are the kernels' own buffers)
    values = index.kneighbors_graph().values()
    torch.cuda.synchronize()
    assert np.array_equal(values.cpu().numpy(), model_csr(ids, vals, N)[2])


def test_device_and_host_results_agree_on_one_graph(indexes):
    """The tensor's three parts equal the host result: the device index's graph through its host mirror (from_graph) gives
    the scipy matrix of the same k-lists."""
    from pynndescent_amd import NNDescent

    metric, _, device = indexes
    ids, vals = _host_lists(device.neighbor_graph)
    mirror = NNDescent.from_graph(device._raw_data, ids, vals, metric="sqeuclidean", random_state=0)  # (no correction: values as they are)
    for kwargs in ({}, {"symmetric": True}, {"k": 4}):
        assert_same_csr(_parts(device.kneighbors_graph(**kwargs)), _scipy_parts(mirror.kneighbors_graph(**kwargs)))


def test_kneighbors_graph_of_queries(indexes, rows):
    import torch

    _, host, device = indexes
    xq = rows[1]
    ids, vals = host.query(xq, k=7)
    g = host.kneighbors_graph(xq, k=7)
    assert g.shape == (NQ, N)
    assert_same_csr(_scipy_parts(g), model_csr(ids, vals.astype(np.float32), N))
    tq = torch.from_numpy(xq).cuda()
    ids_d, vals_d = _host_lists(device.query(tq, k=7))
    gd = device.kneighbors_graph(tq, k=7)
    assert gd.layout == torch.sparse_csr and tuple(gd.shape) == (NQ, N)
    assert_same_csr(_parts(gd), model_csr(ids_d, vals_d, N))
    # a filter that allows 5 rows: every query gets 5 answers and two (-1, inf) fills, which the export drops
    allowed = np.array([3, 77, 500, 1234, 1999])
    ids_f, vals_f = host.query(xq, k=7, filter=allowed)
    assert (ids_f < 0).any()
    gf = host.kneighbors_graph(xq, k=7, filter=allowed)
    assert_same_csr(_scipy_parts(gf), model_csr(ids_f, vals_f.astype(np.float32), N))
    per_row = np.diff(gf.indptr)
    assert (per_row[(ids_f < 0).any(axis=1)] < 7).all() and gf.nnz == int((ids_f >= 0).sum())
    assert set(gf.indices.tolist()) <= set(allowed.tolist())


def test_transformer(rows):
    from pynndescent_amd import PyNNDescentTransformer

    x, xq = rows
    t = PyNNDescentTransformer(n_neighbors=8, random_state=0)
    g = t.fit_transform(x)
    assert g.shape == (N, N) and t.n_samples_fit == N and t.index_.n_neighbors == 9
    assert (np.diff(g.indptr) == 9).all()
    assert int((g.indices == np.repeat(np.arange(N), 9)).sum()) == N  # the diagonal is explicit: every row stores (i, i)
    again = t.transform(None)
    assert_same_csr(_scipy_parts(again), _scipy_parts(g))
    gq = t.transform(xq)
    assert gq.shape == (NQ, N) and (np.diff(gq.indptr) == 8).all()


def test_transformer_in_a_sklearn_pipeline(rows):
    try:
        from sklearn.base import clone
        from sklearn.neighbors import KNeighborsClassifier
        from sklearn.pipeline import make_pipeline
    except ImportError:
        pytest.skip("sklearn does not import")
    from pynndescent_amd import PyNNDescentTransformer

    x, xq = rows
    t = PyNNDescentTransformer(n_neighbors=8, metric="euclidean", random_state=0, n_trees=5)
    assert clone(t).get_params() == t.get_params() and clone(t) is not t
    y = (x[:, 0] > 0).astype(np.int64)
    pipe = make_pipeline(clone(t), KNeighborsClassifier(n_neighbors=5, metric="precomputed"))
    pipe.fit(x, y)
    predicted = pipe.predict(xq)
    assert predicted.shape == (NQ,)
    # the neighbours carry the label's half-space: chance is 0.5 with a standard deviation of 0.03 over 300 queries
    assert (predicted == (xq[:, 0] > 0)).mean() > 0.6
