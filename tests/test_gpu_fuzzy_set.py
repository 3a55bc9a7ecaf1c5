"""The fuzzy simplicial set on the GPU (csrc/fuzzy.hip, the fuzzy merge of csrc/csr_graph.hip, pynndescent_amd/fuzzy.py) against
the float64 model of tests/fuzzy_set_util.py: pattern, symmetry, rhos and run-to-run bytes exactly; sigmas and data within 4x the
noise floor of the formulation, which is the deviation of the same model run in float32.

Measured on an MI355X over the 22 model comparisons below: the floor of the sigmas (relative) lay between 1.4e-6 and 1.4e-5 and
the kernels' largest deviation between 0.01x and 1.34x of it; for the data (absolute) the floor lay between 4.6e-7 and 4.8e-6
and the kernels' deviation between 0.14x and 1.20x of it."""
import functools

import numpy as np
import pytest

from pynndescent_amd import _capi, fuzzy_simplicial_set
from tests.fuzzy_set_util import deviation, model_fuzzy_set

pytestmark = pytest.mark.gpu
M = 301


@functools.lru_cache(maxsize=None)
def gaussian_lists(k):
    """exact_knn of 301 x 8 Gaussian rows whose rows 0..19 are one point: those rows hold 20 zero distances (k < 20: nothing else)."""
    from pynndescent_amd import exact_knn

    x = np.random.RandomState(7).standard_normal((M, 8)).astype(np.float32)
    x[:20] = x[0]
    ids, dists = exact_knn(x, k=k)
    ids, dists = np.ascontiguousarray(ids, dtype=np.int32), np.ascontiguousarray(dists, dtype=np.float32)
    ids.setflags(write=False)
    dists.setflags(write=False)
    return ids, dists


def check(ids, dists, n, lc=1.0, bandwidth=1.0, mix=1.0, set_ops=True):
    want, sigmas64, rhos, weights = model_fuzzy_set(ids, dists, n, lc, bandwidth, mix, set_ops)
    floor, sigmas32, _, _ = model_fuzzy_set(ids, dists, n, lc, bandwidth, mix, set_ops, f=np.float32)
    # the condition of pattern equality: no stored value of the model is near float32's underflow
    assert weights[weights != 0].min() > 1e-30 and (want.nnz == 0 or want.data.min() > 1e-30)
    assert np.array_equal(floor.indptr, want.indptr) and np.array_equal(floor.indices, want.indices)
    got = _capi.fuzzy_set(ids, dists, n, lc, bandwidth, mix, set_ops, want_long_rows=True)
    again = _capi.fuzzy_set(ids, dists, n, lc, bandwidth, mix, set_ops, want_long_rows=True)
    indptr, indices, data, sigmas, rhos_got, long_rows = got
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[:5], again[:5]))
    assert np.array_equal(indptr, want.indptr) and np.array_equal(indices, want.indices)
    assert rhos_got.tobytes() == rhos.tobytes()
    if set_ops:
        import scipy.sparse as sp

        t = sp.csr_array((data.view(np.uint32), indices, indptr), shape=(n, n)).T.tocsr()
        t.sort_indices()
        assert np.array_equal(t.indptr, indptr) and np.array_equal(t.indices, indices) and np.array_equal(t.data, data.view(np.uint32))
    for name, g, w, f32, relative in (("sigmas", sigmas, sigmas64, sigmas32, True), ("data", data, want.data, floor.data, False)):
        noise, dev = deviation(f32, w, relative), deviation(g, w, relative)
        print("%s: float32 floor %.3g, kernel deviation %.3g (%.2f x)" % (name, noise, dev, dev / noise if noise else np.inf))
        assert dev <= 4 * noise, (name, dev, noise)
    return long_rows


@pytest.mark.parametrize("k", [5, 15, 16, 17, 33, 65, 200])
def test_every_lane_split_equals_the_model(k):
    ids, dists = gaussian_lists(k)
    assert (dists[:20, : min(k, 20)] == 0).all() and ((dists[:20] > 0).any() == (k > 20))
    assert check(ids, dists, M) == 0


@pytest.mark.parametrize("bandwidth", [1.0, 2.0])
@pytest.mark.parametrize("lc", [0.5, 1.0, 1.5, 2.0])
def test_local_connectivity_and_bandwidth(lc, bandwidth):
    check(*gaussian_lists(15), M, lc=lc, bandwidth=bandwidth)


@pytest.mark.parametrize("mix,set_ops", [(1.0, True), (0.5, True), (0.0, True), (1.0, False)])
def test_set_operations(mix, set_ops):
    check(*gaussian_lists(15), M, mix=mix, set_ops=set_ops)


def test_hub_row_takes_the_long_merge():
    rs = np.random.RandomState(5)
    ids = np.stack([1 + rs.permutation(699)[:15] for _ in range(700)]).astype(np.int32)
    ids[:, 3] = 0  # every row lists row 0: its union holds more than 512 keys
    dists = np.sort(rs.uniform(0.1, 2.0, (700, 15)).astype(np.float32), axis=1)
    assert check(ids, dists, 700) == 1


def test_rows_with_empty_places():
    ids, dists = (a.copy() for a in gaussian_lists(15))
    for row, kept in ((30, 9), (31, 2), (32, 1), (33, 0), (300, 5)):  # trailing (-1, inf), as a filtered query leaves them
        ids[row, kept:], dists[row, kept:] = -1, np.inf
    check(ids, dists, M)
    check(ids, dists, M, lc=2.0, set_ops=False)


def _device_parts(result):
    graph, sigmas, rhos = result
    return [t.cpu().numpy() for t in (graph.crow_indices(), graph.col_indices(), graph.values(), sigmas, rhos)]


def test_host_arrays_and_device_tensors_give_the_same_bytes():
    import torch

    ids, dists = gaussian_lists(33)
    graph, sigmas, rhos = fuzzy_simplicial_set(ids, dists)
    assert graph.has_canonical_format and graph.shape == (M, M) and sigmas.dtype == rhos.dtype == graph.data.dtype == np.float32
    device = fuzzy_simplicial_set(torch.from_numpy(ids.astype(np.int64)).cuda(), torch.from_numpy(dists.copy()).cuda())
    assert device[0].layout == torch.sparse_csr and device[1].is_cuda
    for a, b in zip((graph.indptr, graph.indices, graph.data, sigmas, rhos), _device_parts(device)):
        assert a.tobytes() == b.astype(a.dtype).tobytes()


def test_through_nndescent():
    import scipy.sparse as sp
    import torch

    from pynndescent_amd import NNDescent

    x = np.random.RandomState(3).standard_normal((500, 8)).astype(np.float32)
    index = NNDescent(torch.from_numpy(x).cuda(), n_neighbors=10, random_state=0)
    got, want = _device_parts(index.fuzzy_simplicial_set()), _device_parts(fuzzy_simplicial_set(*index.neighbor_graph))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and got[2].shape[0] > 500
    narrow = index.fuzzy_simplicial_set(n_neighbors=6, set_op_mix_ratio=0.5)
    ids, dists = index.neighbor_graph
    want = _device_parts(fuzzy_simplicial_set(ids[:, :6].contiguous(), dists[:, :6].contiguous(), set_op_mix_ratio=0.5))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_device_parts(narrow), want))
    graph, sigmas, rhos = NNDescent(x, n_neighbors=10, random_state=0).fuzzy_simplicial_set()
    assert isinstance(graph, sp.csr_array) and graph.has_canonical_format and graph.shape == (500, 500)
    assert isinstance(sigmas, np.ndarray) and sigmas.dtype == rhos.dtype == np.float32 and (abs(graph - graph.T)).nnz == 0
