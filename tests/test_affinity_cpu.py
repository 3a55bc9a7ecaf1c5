"""The perplexity affinities without a GPU: the argument errors of both entry points (before the library is loaded), the host
model on cases solvable by hand, and the share of the GPU tests' model entries that the device may leave out of the pattern."""
import numpy as np
import pytest

from tests.affinity_util import model_matrix, model_search, row_entropies


def test_argument_errors_come_before_the_library_is_loaded(monkeypatch):
    from pynndescent_amd import NNDescent, _capi, perplexity_affinities

    x = np.random.RandomState(0).standard_normal((50, 4)).astype(np.float32)
    idx = (np.arange(50, dtype=np.int32)[:, None] + 1 + np.arange(5, dtype=np.int32)[None, :]) % 50
    dist = np.tile(np.arange(1, 6, dtype=np.float32), (50, 1))
    index = NNDescent.from_graph(x, idx, dist, random_state=1)  # an index that needs no GPU
    monkeypatch.setattr(_capi, "load_library", lambda: pytest.fail("the library was loaded"))
    for perplexity in (0.0, -3.0, np.inf, [5.0, 0.0], [1.0, 2.0, 3.0, 4.0, 5.0], []):
        for call in (index.perplexity_affinities, lambda p: perplexity_affinities(idx, dist, perplexity=p)):
            with pytest.raises(ValueError, match="perplexity"):
                call(perplexity)
    for call, match in ((lambda: index.perplexity_affinities(2.0, n_neighbors=6), "n_neighbors"),  # more columns than the graph has
                        (lambda: index.perplexity_affinities(2.0, n_neighbors=0), "n_neighbors"),
                        (lambda: perplexity_affinities(np.zeros((3, 257), np.int32), np.zeros((3, 257), np.float32)), "n_neighbors"),
                        (lambda: perplexity_affinities(idx, dist[:, :4]), "one shape"),
                        (lambda: perplexity_affinities(idx[:20], dist[:20], n_points=50), "square"),
                        (lambda: perplexity_affinities(idx, dist, n_points=49, symmetrize=False), "holds the id 49")):
        with pytest.raises(ValueError, match=match):
            call()


@pytest.mark.parametrize("perplexity,beta", [(7.0, 1.0), (14.0, 2.0 ** -99), (3.0, 2.0 ** 99)])
def test_equidistant_places_give_a_uniform_row(perplexity, beta):
    """7 places at one distance, entropy log(7) at every beta: perplexity 7 is met at once, any other runs out the 100 steps."""
    ids, dists = np.arange(1, 8, dtype=np.int32)[None, :], np.full((1, 7), 2.5, np.float32)
    betas, cond = model_search(ids, dists, 10, perplexity)
    assert betas[0, 0] == beta and np.array_equal(cond[0], np.full(7, 1.0 / 7.0))


def test_two_places_follow_the_closed_form():
    """Energies 0 and e: with q = exp(-beta e) the row is (1, q) / (1 + q) and H = log(1 + q) + beta e q / (1 + q)."""
    ids, dists, e = np.array([[3, 4]], np.int32), np.array([[0.5, 2.0]], np.float32), 2.0 - 0.5
    betas, cond = model_search(ids, dists, 10, 1.5, squared=False)
    q = np.exp(-betas[0, 0] * e)
    assert abs(np.log1p(q) + betas[0, 0] * e * q / (1 + q) - np.log(1.5)) <= 1e-5
    np.testing.assert_allclose(cond[0], [1 / (1 + q), q / (1 + q)], rtol=1e-14)


def test_model_rows_and_the_entries_the_device_may_leave_out():
    """The GPU shape cases' inputs: reachable rows have entropy log(perplexity) to 1e-5; under 1 % of a case may be left out."""
    from tests.test_gpu_affinity import KS, MS, N, left_out, lists, searched

    for k in KS:
        ids, perplexity = lists(k)[0], max(1.5, k / 3.0)
        betas, cond = searched(k, perplexity)[:2]
        searching = (betas[:, 0] > 2.0 ** -99) & (betas[:, 0] < 2.0 ** 99)  # the rows that did not run out their steps
        assert searching.sum() >= N - 4
        for m in MS:
            p = model_matrix(ids[:m], cond[:m], N, symmetrize=m == N, normalize=m == N)
            assert left_out(p).sum() <= 0.01 * max(p.nnz, 1), (k, m)
            if m < N:
                assert (np.abs(row_entropies(p)[searching[:m]] - np.log(perplexity)) <= 1e-5).all()
