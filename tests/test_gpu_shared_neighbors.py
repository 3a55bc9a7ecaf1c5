"""The shared-neighbour graph on the GPU (csrc/snn.hip, the min merge of csrc/csr_graph.hip) against the set model of
tests/snn_util.py.  Every comparison is exact -- offsets, columns and the data's bytes -- and every call is made twice.

The input is overlapping windows, ids[i] = (i + 1 + a random k of the next min(3k, m - 1) offsets) % m, so the intersections
vary from edge to edge; m = 301, or 600 for k >= 129.  The k cover every lane split of the two kernels, both sides of each
boundary and both LDS tiers."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from pynndescent_amd import _capi, shared_neighbor_graph
from tests.snn_util import model_snn, same_bytes

pytestmark = pytest.mark.gpu
KS = [2, 5, 15, 16, 17, 33, 64, 65, 129, 256]
VARIANTS = [("jaccard", False, 0.0, True), ("jaccard", True, 1 / 15, True), ("count", True, 0.0, False), ("count", False, 3.0, True)]


@functools.lru_cache(maxsize=None)
def lists(k, m=None):
    m = m or (600 if k >= 129 else 301)
    rs, w = np.random.RandomState(11), min(3 * k, m - 1)
    ids = np.stack([(i + 1 + rs.permutation(w)[:k]) % m for i in range(m)]).astype(np.int32)
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def dirty(k, m=700):
    """lists(k, 700) with rows that end in -1, ids past the end, repeats, rows that list themselves, one id (9) that every
    row lists -- a symmetric row of more than 512 keys -- and, set last, a row of nothing but -1."""
    ids = lists(k, m).astype(np.int64)
    ids[:, k - 2] = 9
    ids[3:6, k // 2:] = -1
    ids[7, :3] = (m, m + 5, 2 ** 40)
    ids[8, 1] = ids[8, k - 1] = ids[8, 0]
    ids[10:20, 0] = np.arange(10, 20)
    ids[6] = -1
    ids.setflags(write=False)
    return ids


@functools.lru_cache(maxsize=None)
def model(ids_of, k, *form):
    return model_snn(ids_of(k), *form)


def scipy_of(t):
    """A device result as the scipy matrix the host call returns."""
    out = sp.csr_array((t.values().cpu().numpy(), t.col_indices().cpu().numpy().astype(np.int32), t.crow_indices().cpu().numpy()), shape=tuple(t.shape))
    return out


def twice(ids, *form):
    got, again = shared_neighbor_graph(ids, *form), shared_neighbor_graph(ids, *form)
    if not isinstance(got, sp.csr_array):
        got, again = scipy_of(got), scipy_of(again)
    assert same_bytes(got, again) and got.shape == (ids.shape[0], ids.shape[0])
    return got


def weights_met(ids_of, k, include_self):
    return np.unique(model(ids_of, k, "count", include_self, 0.0, False).data)


@pytest.mark.parametrize("k", KS)
def test_every_lane_split_equals_the_model(k):
    got = twice(lists(k))
    assert isinstance(got, sp.csr_array) and got.has_canonical_format and got.data.dtype == np.float32 and got.indices.dtype == np.int32
    assert len(weights_met(lists, k, True)) >= (2 if k == 2 else 5 if k == 5 else 10)  # the edges do not all share the same number
    assert same_bytes(got, model(lists, k, "jaccard", True, 0.0, True))
    t = got.T.tocsr()
    t.sort_indices()
    assert same_bytes(got, t)


@pytest.mark.parametrize("form", VARIANTS, ids=lambda f: "-".join(str(v) for v in f))
@pytest.mark.parametrize("k", [15, 65])
def test_weights_self_prune_and_direction(k, form):
    want, whole = model(lists, k, *form), model(lists, k, form[0], True, 0.0, form[3])
    dropped = 1.0 - want.nnz / whole.nnz  # the edges that share nothing, or less than the bound
    assert 0.0 <= dropped < 1.0 and not same_bytes(want, model(lists, k, "jaccard", True, 0.0, True))
    if form[2] > 0 or (k == 15 and not form[1]):  # (at k = 65 every two ends share a neighbour)
        assert dropped > 0.0
    assert same_bytes(twice(lists(k), *form), want)


@pytest.mark.parametrize("k", [15, 65])
def test_dirty_lists_int64_and_a_row_stride(k):
    import torch

    ids = dirty(k)
    want = model(dirty, k, "jaccard", True, 0.0, True)
    assert np.diff(want.indptr).max() > 512 and _capi.snn_graph(ids, want_long_rows=True)[3] >= 1  # the hub's row takes the long merge
    assert same_bytes(twice(ids), want)
    wide = torch.full((ids.shape[0], k + 3), 5, dtype=torch.int64).cuda()
    wide[:, :k] = torch.from_numpy(ids.copy()).cuda()
    assert same_bytes(twice(wide[:, :k]), want)
    assert same_bytes(twice(np.where(ids >= 2 ** 31, 2 ** 31 - 1, ids).astype(np.int32), "count", False, 0.0, False), model(dirty, k, "count", False, 0.0, False))


def test_host_arrays_and_device_tensors_give_the_same_bytes():
    import torch

    ids = lists(33)
    host, device = twice(ids), shared_neighbor_graph(torch.from_numpy(ids.copy()).cuda())
    assert device.layout == torch.sparse_csr and device.is_cuda and same_bytes(host, scipy_of(device))


def test_through_nndescent():
    import torch

    from pynndescent_amd import NNDescent

    x = np.random.RandomState(5).standard_normal((500, 8)).astype(np.float32)
    index = NNDescent(torch.from_numpy(x).cuda(), n_neighbors=10, random_state=0)
    ids = index.neighbor_graph[0]
    got = index.shared_neighbor_graph()
    assert got.layout == torch.sparse_csr and got.is_cuda and same_bytes(scipy_of(got), scipy_of(shared_neighbor_graph(ids)))
    assert same_bytes(scipy_of(got), model_snn(ids.cpu().numpy()))
    assert same_bytes(scipy_of(index.shared_neighbor_graph(n_neighbors=6, weight="count")), scipy_of(shared_neighbor_graph(ids[:, :6], weight="count")))
    host_index = NNDescent(x, n_neighbors=10, random_state=0)
    host = host_index.shared_neighbor_graph()
    assert isinstance(host, sp.csr_array) and host.has_canonical_format and host.shape == (500, 500)
    assert same_bytes(host, shared_neighbor_graph(host_index.neighbor_graph[0])) and same_bytes(host, model_snn(host_index.neighbor_graph[0]))
