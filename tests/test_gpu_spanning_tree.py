"""The spanning tree on the GPU (csrc/cross.hip on top of csrc/mst.hip) against the model of tests/spanning_tree_util.py: the
tree's offsets and columns, its weights (bit for bit where distances are exact in both precisions, within one float32 ulp of the
numpy float64 sums elsewhere), the core distances and the component count; every call is made twice and must give the same
bytes.  On the Gaussian sets at most 1 % of the query rows may take the float64 tier: a screen that certifies nothing would
pass every other check."""
import functools

import numpy as np
import pytest

from pynndescent_amd import _capi, spanning_forest, spanning_tree
from tests.spanning_tree_util import brute_lists, model_tree
from tests.spanning_util import blob_lists, same_bytes

pytestmark = pytest.mark.gpu


def blobs(sizes, d, spread, seed, metric="euclidean"):
    """Gaussian blobs of the given sizes around far centres; k-lists inside each blob (k = 6), so a blob is a component."""
    rs = np.random.RandomState(seed)
    groups = np.repeat(np.arange(len(sizes)), sizes)
    x = (spread * rs.standard_normal((len(sizes), d))[groups] + rs.standard_normal((len(groups), d))).astype(np.float32)
    return (x,) + brute_lists(x, 6, metric, groups)


def lattice(min_samples):
    """Integer rows, 40 of them twice: every distance and every tie is exact in float64 and float32 alike."""
    x = np.random.RandomState(1).randint(0, 4, (700, 6)).astype(np.float32)
    x[660:] = x[:40]
    return (x,) + brute_lists(x, max(2, min_samples))


def chain(_):
    """16 blobs on a line at the gaps of a ruler (10, 20, 10, 30, ..): pairs, then fours, then eights join."""
    at = np.cumsum([0] + [10 * ((i & -i).bit_length()) for i in range(1, 16)])
    rs = np.random.RandomState(2)
    x = rs.standard_normal((16 * 12, 5)).astype(np.float32) * 0.5
    x[:, 0] += np.repeat(at, 12)
    return (x,) + brute_lists(x, 4, groups=np.repeat(np.arange(16), 12))


CASES = {
    # name: (maker, argument, metric, min_samples, exact bits, rounds at least)
    "lattice-single-linkage": (lattice, 0, "euclidean", 0, True, 1),
    "lattice-core-3": (lattice, 3, "euclidean", 3, True, 1),
    "sizes-d5": (lambda d: blobs([1100, 1, 2, 63, 64, 65, 205], d, 30, 4), 5, "euclidean", 4, False, 1),
    "sizes-d128-cosine": (lambda d: blobs([1100, 1, 2, 63, 64, 65, 205], d, 2, 5, "cosine"), 128, "cosine", 4, False, 1),
    "sizes-d130-sq": (lambda d: blobs([700, 1, 2, 63, 64, 65], d, 6, 6, "sqeuclidean"), 130, "sqeuclidean", 4, False, 1),
    "one-query-row": (lambda q: blobs([200, q], 5, 30, 7), 1, "euclidean", 3, False, 1),
    "one-block-of-query-rows": (lambda q: blobs([200, q], 5, 30, 7), 64, "euclidean", 3, False, 1),
    "two-blocks-of-query-rows": (lambda q: blobs([200, q], 5, 30, 7), 65, "euclidean", 3, False, 1),
    "ruler-chain": (chain, None, "euclidean", 2, False, 3),
}


@functools.lru_cache(maxsize=None)
def case(name):
    maker, arg, metric, min_samples = CASES[name][:4]
    x, ids, dists = maker(arg)
    for a in (x, ids, dists):
        a.setflags(write=False)
    return x, ids, dists, model_tree(x, ids, dists, min_samples, metric)


def within_an_ulp(got, want):
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32)).max(initial=0) <= 1


def run(name, flags=0):
    x, ids, dists, _ = case(name)
    metric, min_samples = CASES[name][2:4]
    first = spanning_tree(x, ids, dists, metric, min_samples, return_stats=True, _flags=flags)
    again = spanning_tree(x, ids, dists, metric, min_samples, _flags=flags)
    assert same_bytes(first[0], again[0]) and first[1].tobytes() == again[1].tobytes() and first[2] == again[2]
    return first


@pytest.mark.parametrize("name", list(CASES))
def test_tree_equals_the_model(name):
    (tree, core, n_components, stats), (want, want_core, want_n) = run(name), case(name)[3]
    exact, rounds = CASES[name][4:]
    print(name, stats)
    assert n_components == want_n > 1 and stats["rounds"] >= rounds and core.tobytes() == want_core.tobytes()
    assert tree.has_canonical_format and tree.nnz == 2 * (len(core) - 1) and (abs(tree - tree.T)).nnz == 0
    assert np.array_equal(tree.indptr, want.indptr) and np.array_equal(tree.indices, want.indices)
    assert tree.data.tobytes() == want.data.tobytes() if exact else within_an_ulp(tree.data, want.data)
    if name.startswith("sizes"):
        sizes = np.bincount(spanning_forest(*case(name)[1:3], CASES[name][3])[1])
        assert {1, 2, 63, 64, 65} <= set(sizes.tolist()) and stats["slices"] >= 2
        assert stats["query_rows"] == len(core) - sizes.max() and stats["tier2_rows"] <= 0.01 * stats["query_rows_all"]
    if name.endswith("query-rows") or name == "one-query-row":
        assert stats["query_rows"] == CASES[name][1]


@pytest.mark.parametrize("name", ["lattice-core-3", "sizes-d128-cosine", "sizes-d130-sq"])
def test_float64_tier_gives_the_same_tree(name):
    (tree, core, n, _), (forced, forced_core, forced_n, stats) = run(name), run(name, _capi.NND_FLAG_TEST_TREE_F64)
    assert stats["tier2_rows"] == stats["query_rows_all"] > 0
    assert same_bytes(tree, forced) and core.tobytes() == forced_core.tobytes() and n == forced_n


def test_connected_graph_is_its_forest():
    ids, dists = blob_lists(301, 15, 1)
    x = np.random.RandomState(0).standard_normal((301, 4)).astype(np.float32)  # (never read: nothing is left to join)
    forest, labels, core = spanning_forest(ids, dists, 5)
    tree, tree_core, n, stats = spanning_tree(x, ids, dists, "euclidean", 5, return_stats=True)
    assert labels.max() == 0 and n == 1 and stats["rounds"] == 0 and stats["query_rows"] == 0
    assert same_bytes(tree, forest) and tree_core.tobytes() == core.tobytes()


def test_device_tensors_and_the_index_method():
    import torch

    from pynndescent_amd import NNDescent
    from tests.test_gpu_spanning_forest import scipy_of

    x, ids, dists, (want, want_core, want_n) = case("sizes-d5")
    tree, core, n = spanning_tree(torch.from_numpy(x.copy()).cuda(), torch.from_numpy(ids.copy()).cuda(), torch.from_numpy(dists.copy()).cuda(), "euclidean", 4)
    assert tree.layout == torch.sparse_csr and tree.is_cuda and core.is_cuda and n == want_n
    assert same_bytes(scipy_of(tree), run("sizes-d5")[0]) and core.cpu().numpy().tobytes() == want_core.tobytes()
    index = NNDescent(x[:600], n_neighbors=4, random_state=0)
    g_ids, g_dists = index.neighbor_graph
    got, want = index.spanning_tree(min_samples=3), spanning_tree(x[:600], g_ids, g_dists, "euclidean", 3)
    assert same_bytes(got[0], want[0]) and got[0].nnz == 2 * 599 and got[2] == want[2]
