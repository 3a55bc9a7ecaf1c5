"""The spanning forest on the GPU (csrc/mst.hip, the min merge of csrc/csr_graph.hip) against the Kruskal model of
tests/spanning_util.py.  Every comparison is exact -- the forest's offsets, columns and data bytes, the labels, the core
distances -- and every call is made twice.

The inputs are exact k-lists of Gaussian blobs (several components, tied mutual-reachability weights); m = 301, or 600 for
k >= 129.  The k cover every lane split of k_mst_core, both sides of each boundary and both LDS tiers; the symmetric rows they
give cover the four widths of k_mst_scan (8 lanes a row at k = 1..5, 16 at the index test's 6 and 10, 32 at 15..17, 64 above)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from pynndescent_amd import _capi, spanning_forest
from tests.spanning_util import blob_lists, model_forest, same_bytes

pytestmark = pytest.mark.gpu
KS = [1, 2, 5, 15, 16, 17, 32, 33, 64, 65, 128, 129, 256]


@functools.lru_cache(maxsize=None)
def lists(k, duplicated=0):
    ids, dists = blob_lists(600 if k >= 129 else 301, k, 2 if k >= 33 else 7, duplicated)
    ids.setflags(write=False), dists.setflags(write=False)
    return ids, dists


@functools.lru_cache(maxsize=None)
def ruler(m=300):
    """A path: row i lists i - 1 and i + 1; edge (i, i + 1) is 1 + the trailing zero bits of i + 1 long."""
    at = np.arange(m)
    ids = np.stack([at - 1, np.where(at + 1 < m, at + 1, -1)], axis=1).astype(np.int32)
    step = np.array([1 + ((i + 1) & -(i + 1)).bit_length() - 1 for i in range(m)], dtype=np.float32)
    return ids, np.stack([np.roll(step, 1), step], axis=1)


@functools.lru_cache(maxsize=None)
def dirty(k, m=700):
    """The dirty() recipe of the shared-neighbour test on int64 ids with distances: rows that end in -1, ids past the end,
    a repeated id, rows that list themselves, an inf and a NaN distance, unsorted rows (the hub column), one id (9) that every
    row lists -- a symmetric row of more than 512 keys -- and, set last, a row of nothing but -1."""
    ids, dists = blob_lists(m, k, 5)
    ids, dists = ids.astype(np.int64), dists.copy()
    ids[:, k - 2], dists[:, k - 2] = 9, np.float32(60) + np.arange(m, dtype=np.float32) % 7
    ids[3:6, k // 2:] = -1
    ids[7, :3] = (m, m + 5, 2 ** 40)
    ids[8, 1] = ids[8, k - 1] = ids[8, 2]
    ids[10:20, 1] = np.arange(10, 20)
    dists[21, 1], dists[22, 2], dists[23, 1] = np.inf, np.nan, -0.0
    ids[6] = -1
    return ids, dists


@functools.lru_cache(maxsize=None)
def model(lists_of, min_samples, *args):
    return model_forest(*lists_of(*args), min_samples)


def scipy_of(t):
    """A device result as the scipy matrix the host call returns."""
    return sp.csr_array((t.values().cpu().numpy(), t.col_indices().cpu().numpy().astype(np.int32), t.crow_indices().cpu().numpy()), shape=tuple(t.shape))


def twice(ids, dists, min_samples):
    got, again = spanning_forest(ids, dists, min_samples), spanning_forest(ids, dists, min_samples)
    if not isinstance(got[0], sp.csr_array):
        got, again = [(scipy_of(f), l.cpu().numpy(), c.cpu().numpy()) for f, l, c in (got, again)]
    assert all(same(got, again)) and got[0].shape == (ids.shape[0], ids.shape[0])
    return got


def same(got, want):
    """forest bytes, labels, core distances"""
    return (same_bytes(got[0], want[0]), got[1].dtype == np.int32 and np.array_equal(got[1], want[1]),
            got[2].dtype == np.float32 and got[2].tobytes() == want[2].tobytes())


@pytest.mark.parametrize("k", KS)
def test_every_lane_split_equals_the_model(k):
    got, want = twice(*lists(k), min(5, k)), model(lists, min(5, k), k)
    assert isinstance(got[0], sp.csr_array) and got[0].has_canonical_format and got[0].indices.dtype == np.int32
    assert want[1].max() >= 1 and (k < 5 or len(np.unique(want[0].data)) < want[0].nnz // 2)  # components, tied weights
    assert same(got, want) == (True, True, True)


@pytest.mark.parametrize("min_samples", [0, 1, 15])
def test_min_samples_forms(min_samples):
    want = model(lists, min_samples, 15, 20)  # 20 duplicated rows
    assert (min_samples > 1) or (want[0].data == 0).sum() >= 20  # zero weights are stored, and met
    assert same(twice(*lists(15, 20), min_samples), want) == (True, True, True)


def test_ruler_path_doubles_its_components_every_round():
    """Blocks of 2^r points after r rounds, many equal weights: the case for a tie rule that is not a function of the edge and
    for a hook step that closes a cycle.  Eight rounds: the short last block [256, 300) joins its left neighbour in round 7
    already (its only edge out), so two components are left for the eighth."""
    ids, dists = ruler()
    want = model(ruler, 0)
    assert want[1].max() == 0 and want[0].nnz == 2 * 299
    assert same(twice(ids, dists, 0), want) == (True, True, True)
    assert _capi.spanning_forest(ids, dists, 0, want_rounds=True)[5] == 8


@pytest.mark.parametrize("k", [15, 65])
def test_dirty_lists_int64_and_a_row_stride(k):
    import torch

    ids, dists = dirty(k)
    want = model(dirty, 5, k)
    assert same(twice(ids, dists, 5), want) == (True, True, True)
    wide_ids, wide_dists = torch.full((ids.shape[0], k + 3), 5, dtype=torch.int64).cuda(), torch.full((ids.shape[0], k + 6), 0.5).cuda()
    wide_ids[:, :k], wide_dists[:, :k] = torch.from_numpy(ids).cuda(), torch.from_numpy(dists).cuda()
    assert same(twice(wide_ids[:, :k], wide_dists[:, :k], 5), want) == (True, True, True)


def test_host_arrays_and_device_tensors_give_the_same_bytes():
    import torch

    ids, dists = lists(33)
    device = spanning_forest(torch.from_numpy(ids.copy()).cuda(), torch.from_numpy(dists.copy()).cuda())
    assert device[0].layout == torch.sparse_csr and device[0].is_cuda and device[1].is_cuda and device[2].is_cuda
    assert same(twice(ids, dists, 5), (scipy_of(device[0]), device[1].cpu().numpy(), device[2].cpu().numpy())) == (True, True, True)


@pytest.mark.parametrize("on_device", [True, False])
def test_through_nndescent(on_device):
    import torch

    from pynndescent_amd import NNDescent

    x = np.random.RandomState(5).standard_normal((500, 8)).astype(np.float32)
    index = NNDescent(torch.from_numpy(x).cuda() if on_device else x, n_neighbors=10, random_state=0)
    ids, dists = index.neighbor_graph
    for kwargs, k in (({}, 10), ({"n_neighbors": 6, "min_samples": 3}, 6)):
        got, want = index.spanning_forest(**kwargs), spanning_forest(ids[:, :k], dists[:, :k], kwargs.get("min_samples", 5))
        if on_device:
            assert got[0].layout == torch.sparse_csr and got[0].is_cuda
            got, want = [(scipy_of(f), l.cpu().numpy(), c.cpu().numpy()) for f, l, c in (got, want)]
            ids_h, dists_h = ids.cpu().numpy(), dists.cpu().numpy()
        else:
            assert isinstance(got[0], sp.csr_array) and got[0].has_canonical_format and got[0].shape == (500, 500)
            ids_h, dists_h = ids, dists
        assert same(got, want) == (True, True, True)
        assert same(got, model_forest(ids_h[:, :k], dists_h[:, :k], kwargs.get("min_samples", 5))) == (True, True, True)
