"""The perplexity affinities on the GPU (csrc/affinity.hip, the sum merge of csrc/csr_graph.hip) against the float64 model of
tests/affinity_util.py: pattern, symmetry, run-to-run bytes and the total exactly; betas and data within 4x the deviation of the
same model run in float32; a returned row's entropy within 1e-5 plus that model's entropy deviation of log(perplexity).  The
pattern may lack model entries below the smallest float32 normal times the row's largest (v_exp_f32 flushes them).

An input is 1000 rows (301: multiscale), searched by the model once; a case of m < 1000 rows hands the device the first m and
takes the floor of all 1000.  beta moves in dyadic steps, so the two models differ only on the 3 to 17 rows of 1000 where a
rounding of H crosses the stop rule: on 67 rows the floor is often exactly 0, and 4 x 0 would ask the device for float64's
decisions bit for bit.  Rows do not see each other: the m < 1000 cases' bytes are those of the same rows in the 1000-row call.

Measured on an MI355X over the 69 comparisons: floor of the betas 1.8e-5 .. 8.8e-4 relative (0 where no row can reach its
perplexity; the kernel's deviation was 0 too), the kernels' deviation at most 1.55x of it; floor of the data 2.4e-12 .. 9.8e-6
absolute, the kernels' at most 1.68x.  No model entry was missing.  Entropies within 1.05e-5 (1e-5 + 1.6e-5 .. 2.0e-5 allowed)."""
import functools

import numpy as np
import pytest

from pynndescent_amd import perplexity_affinities
from tests.affinity_util import model_matrix, model_search, row_entropies
from tests.fuzzy_set_util import deviation

pytestmark = pytest.mark.gpu
KS = [2, 15, 16, 17, 32, 33, 64, 65, 90, 128, 129, 256]  # every group width and places-per-lane edge
MS = [1, 5, 67, 1000]  # partial last waves for every rows-per-wave
N = 1000


@functools.lru_cache(maxsize=None)
def lists(k, near=0.0, seed=0, rows=N):
    """k distinct ids per row, never the row itself, sorted random distances above ``near``; rows 1..5: trailing (-1, inf) places,
    an empty row, equal distances, a row that starts with zeros, a row whose last place is so far that its entry rounds to 0."""
    rs = np.random.RandomState(seed + k)
    order = rs.random_sample((rows, N))
    order[np.arange(rows), np.arange(rows)] = 2.0
    ids = np.argsort(order, axis=1)[:, :k].astype(np.int32)
    dists = (near + np.sort(rs.uniform(1.0, 2.0, (rows, k)) * (100.0 if near else 1.0), axis=1)).astype(np.float32)
    ids[1, k // 2:], dists[1, k // 2:], ids[2], dists[2] = -1, np.inf, -1, np.inf
    dists[3], dists[4, : min(k, 3)], dists[5, -1] = near + 1.5, 0.0, near + 1e3
    ids.setflags(write=False)
    dists.setflags(write=False)
    return ids, dists


@functools.lru_cache(maxsize=None)
def searched(k, perplexity, squared=True, near=0.0, seed=0, rows=N):
    """The model's (betas, conditional entries) of lists(k, near, seed, rows) in float64 and in float32, computed once."""
    ids, dists = lists(k, near, seed, rows)
    return model_search(ids, dists, N, perplexity, squared) + model_search(ids, dists, N, perplexity, squared, f=np.float32)


def left_out(want):
    """The model's entries that the device may lack: below the smallest float32 normal times the row's largest entry."""
    rows = np.repeat(np.arange(want.shape[0]), np.diff(want.indptr))
    largest = np.zeros(want.shape[0])
    np.maximum.at(largest, rows, want.data)
    return want.data < float(np.finfo(np.float32).tiny) * largest[rows]


def check(k, perplexity, m=N, squared=True, symmetrize=True, normalize=True, near=0.0, seed=0, rows=N, ids_type=np.int32):
    ids, dists = lists(k, near, seed, rows)
    betas64, cond64, betas32, cond32 = searched(k, perplexity, squared, near, seed, rows)
    form = (N, symmetrize, normalize)
    want_all, floor_all = model_matrix(ids, cond64, *form), model_matrix(ids, cond32, *form)
    want = want_all if m == rows else model_matrix(ids[:m], cond64[:m], *form)
    scalar = not isinstance(perplexity, tuple)
    kwargs = dict(n_points=N, perplexity=perplexity if scalar else list(perplexity), squared=squared, symmetrize=symmetrize, normalize=normalize)
    got, betas = perplexity_affinities(ids[:m].astype(ids_type), dists[:m], **kwargs)
    again, betas_again = perplexity_affinities(ids[:m].astype(ids_type), dists[:m], **kwargs)
    parts = (got.indptr, got.indices, got.data, betas)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(parts, (again.indptr, again.indices, again.data, betas_again)))
    assert got.has_canonical_format and got.has_sorted_indices and got.shape == (m, N) and betas.shape == ((m,) if scalar else (m, len(perplexity)))
    assert got.data.dtype == betas.dtype == np.float32 and got.indices.dtype == np.int32
    assert np.isfinite(got.data).all() and np.isfinite(betas).all() and (got.data > 0).all()
    # the pattern: every entry is one of the model's, and only model entries that may be left out are missing
    may_lack, keys = left_out(want), lambda a: np.repeat(np.arange(a.shape[0], dtype=np.int64), np.diff(a.indptr)) * N + a.indices
    print("pattern: %d entries, %d of the model's %d left out (%d may be)" % (got.nnz, want.nnz - got.nnz, want.nnz, may_lack.sum()))
    assert may_lack.sum() <= 0.01 * max(want.nnz, 1)
    assert np.isin(keys(got), keys(want)).all() and np.isin(keys(want)[~may_lack], keys(got)).all()
    if symmetrize:
        t = got.T.tocsr()
        t.sort_indices()
        assert np.array_equal(t.indptr, got.indptr) and np.array_equal(t.indices, got.indices) and t.data.tobytes() == got.data.tobytes()
    if normalize and got.nnz:
        assert abs(got.data.sum(dtype=np.float64) - 1.0) <= got.nnz * 2.0 ** -24
    for name, g, w, noise, relative in (("betas", betas.reshape(m, -1), betas64[:m], deviation(betas32, betas64, True), True),
                                        ("data", got.toarray(), want.toarray(), deviation(floor_all.toarray(), want_all.toarray(), False), False)):
        dev = deviation(g, w, relative)
        print("%s: float32 floor %.3g, kernel deviation %.3g (%.2f x)" % (name, noise, dev, dev / noise if noise else np.inf))
        assert dev <= 4 * noise, (name, dev, noise)
    if scalar and not symmetrize and not normalize:  # independent of the model's entries: the entropy of the rows handed out
        h64, h32, h = row_entropies(want_all), row_entropies(floor_all), np.abs(row_entropies(got) - np.log(perplexity))
        reached = np.abs(h64 - np.log(perplexity)) <= 1e-5  # the rows whose target the model meets
        noise = float(np.abs(h32 - h64)[reached].max())
        print("entropy: %d of %d rows reach the target, float32 floor %.3g, kernel %.3g" % (reached[:m].sum(), m, noise, h[reached[:m]].max(initial=0)))
        assert reached.sum() >= rows - 4 and (h[reached[:m]] <= 1e-5 + noise).all()
    return got, betas


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("k", KS)
def test_every_lane_split_equals_the_model(k, m):
    if m == N:
        check(k, max(1.5, k / 3.0))
        return
    got, betas = check(k, max(1.5, k / 3.0), m, symmetrize=False, normalize=False)
    full, full_betas = perplexity_affinities(*lists(k), n_points=N, perplexity=max(1.5, k / 3.0), symmetrize=False, normalize=False)
    assert betas.tobytes() == full_betas[:m].tobytes() and np.array_equal(got.indptr, full.indptr[: m + 1])
    assert got.indices.tobytes() == full.indices[: got.nnz].tobytes() and got.data.tobytes() == full.data[: got.nnz].tobytes()


@pytest.mark.parametrize("perplexities", [(3.0, 8.0), (3.0, 5.0, 8.0), (2.0, 4.0, 6.0, 8.0)])
@pytest.mark.parametrize("k", [15, 32, 64, 90, 256])
def test_multiscale(k, perplexities):
    check(k, tuple(p * k / 24.0 for p in perplexities), 301, symmetrize=False, seed=1, rows=301)


@pytest.mark.parametrize("case", ["above_the_place_count", "near_1e4", "plain_distances", "int64", "directed", "unnormalized"])
def test_input_classes(case):
    kwargs = {"above_the_place_count": {}, "near_1e4": {"near": 1e4}, "plain_distances": {"squared": False, "symmetrize": False, "normalize": False},
              "int64": {"ids_type": np.int64}, "directed": {"symmetrize": False}, "unnormalized": {"normalize": False}}[case]
    k, perplexity = (15, 40.0) if case == "above_the_place_count" else (90, 30.0)
    check(k, perplexity, seed=2, **kwargs)


def _device_parts(result):
    return [t.cpu().numpy() for t in (result[0].crow_indices(), result[0].col_indices(), result[0].values(), result[1])]


def test_device_tensors_and_the_class_method():
    import scipy.sparse as sp
    import torch

    from pynndescent_amd import NNDescent

    ids, dists = lists(33, seed=3)
    host, betas = perplexity_affinities(ids.astype(np.int64), dists, perplexity=[5.0, 11.0])
    device = perplexity_affinities(torch.from_numpy(ids.astype(np.int64)).cuda(), torch.from_numpy(dists.copy()).cuda(), perplexity=[5.0, 11.0])
    assert device[0].layout == torch.sparse_csr and device[1].is_cuda and device[1].shape == (N, 2)
    for a, b in zip((host.indptr, host.indices, host.data, betas), _device_parts(device)):
        assert a.tobytes() == b.astype(a.dtype).tobytes()
    x = np.random.RandomState(3).standard_normal((2000, 16)).astype(np.float32)
    index = NNDescent(torch.from_numpy(x).cuda(), n_neighbors=31, random_state=0)
    got, want = _device_parts(index.perplexity_affinities(10.0)), _device_parts(perplexity_affinities(*index.neighbor_graph, perplexity=10.0))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)) and got[2].shape[0] > 2000 * 30
    host_index = NNDescent(x, n_neighbors=31, random_state=0)
    p, betas = host_index.perplexity_affinities(10.0)
    assert isinstance(p, sp.csr_array) and p.has_canonical_format and p.shape == (2000, 2000) and (abs(p - p.T)).nnz == 0 and isinstance(betas, np.ndarray) and betas.dtype == np.float32 and betas.shape == (2000,)
    want, want_betas = perplexity_affinities(*host_index.neighbor_graph, perplexity=10.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((p.indptr, p.indices, p.data, betas), (want.indptr, want.indices, want.data, want_betas)))
