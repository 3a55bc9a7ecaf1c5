"""The CPU oracle's dot / inner_product / correlation / hellinger (codes 2..5) pinned to the reference's own results
(tests/golden/metric_*.npz and metric_search_graph.npz, written by tests/golden/make_golden_metrics.py).

The GPU tests of these metrics (tests/test_gpu_metric_kernels.py) use the oracle as the reference algorithm, so these
pins are what makes their parity bands mean "the reference"."""
import os

import numpy as np
import pytest
from sklearn.preprocessing import normalize

from oracle import oracle as O
from pynndescent_amd import _capi
from tests import metric_util as MU

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALT_FN = {"dot": "orc_alternative_dot", "inner_product": "orc_alternative_inner_product",
          "correlation": "orc_correlation", "hellinger": "orc_alternative_hellinger"}


def _golden(metric):
    return np.load(os.path.join(GOLDEN, "metric_%s.npz" % metric))


def _space(metric, x):
    """The rows the reference's build reads: NNDescent normalises dot data (pynndescent_.py:1101-1103)."""
    return np.ascontiguousarray(normalize(x, norm="l2"), np.float32) if metric == "dot" else x


def _oracle_edges(metric, xs, idx, rows=None):
    """the oracle's float32 alt distance of every edge (rows[r], idx[r, j])."""
    fn = getattr(O.load("strict"), ALT_FN[metric])
    rows = np.arange(idx.shape[0]) if rows is None else rows
    out = np.full(idx.shape, np.inf, np.float32)
    for r, i in enumerate(rows):
        for j, p in enumerate(idx[r]):
            if p >= 0:
                out[r, j] = fn(xs[i], xs[p], xs.shape[1])
    return out


def test_metric_codes_match_the_library():
    for name, code in O.METRICS.items():
        assert _capi.METRIC_CODES[name] == code, name
    assert set(MU.NEW_METRICS) <= set(O.METRICS)


def test_angular_trees_follow_the_class():
    """one table: angular trees for every unit-row metric, euclidean trees for inner product (as nndescent._METRICS)."""
    from pynndescent_amd import nndescent

    for name in O.ANGULAR:
        assert O.ANGULAR[name] == nndescent._METRICS[name].angular, name


# measured maximum gaps between the oracle's float32 alt distances and the reference's stored ones on the fixture edges:
# dot 2 ulp, inner product 0, hellinger 1 ulp.  The float32 sums are bitwise the same; the fixture ran un-jitted, so its
# logarithms are numpy's float32 log2, which differs from libm's log2f (the oracle's, and what numba links) by 1-2 ulp on a
# quarter of the dot edges.  Correlation differs by up to
# 3.6e-7 absolute: its numba locals are float64, but the fixture ran un-jitted, where NumPy 2 keeps the float64 literals
# at the rows' float32, so the fixture carries float32 rounding of a value near 1 that the oracle's float64 does not.
ULP_GAP = {"dot": 2, "inner_product": 0, "hellinger": 1}


@pytest.mark.parametrize("metric", MU.NEW_METRICS)
def test_alt_distances_match_reference(metric):
    f = _golden(metric)
    xs = _space(metric, f["x"])
    idx, dist = f["idx_3"], f["dist_3"]
    got = _oracle_edges(metric, xs, idx)
    ok = idx >= 0
    assert ok.mean() > 0.99
    assert np.array_equal(got[ok] >= MU.FLT_MAX, dist[ok] >= MU.FLT_MAX)
    if metric == "correlation":
        np.testing.assert_allclose(got[ok], dist[ok], rtol=0, atol=4e-7)
    else:
        ulp = np.abs(got[ok].view(np.int32).astype(np.int64) - dist[ok].view(np.int32).astype(np.int64))
        assert ulp.max() <= ULP_GAP[metric], ulp.max()


@pytest.mark.parametrize("metric", MU.NEW_METRICS)
def test_alt_distances_match_float64(metric):
    """against metric_util.alt_dist in float64, with the conditioning rule of the GPU pairwise-Gram test: tight where the
    (transformed) rows are not near-orthogonal, looser where the similarity cancels."""
    f = _golden(metric)
    xs = _space(metric, f["x"])
    rows = np.arange(0, xs.shape[0], 7)
    idx = f["idx_3"][rows]
    got = _oracle_edges(metric, xs, idx, rows)
    for r, (i, ids) in enumerate(zip(rows, idx)):
        want = MU.alt_dist(metric, xs[i:i + 1], xs[ids])[0]
        g = got[r].astype(np.float64)
        big = want >= MU.FLT_MAX
        assert np.array_equal(g >= MU.FLT_MAX, big), (i, g, want)
        cos = MU.abs_cos(metric, xs[i:i + 1], xs[ids])[0]
        good = ~big & ~(cos < 0.05)
        np.testing.assert_allclose(g[good], want[good], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(g[~big], want[~big], rtol=2e-4, atol=1e-5)


@pytest.mark.parametrize("metric", MU.NEW_METRICS)
def test_corrections_match_reference(metric):
    f = _golden(metric)
    for s in f["seeds"]:
        np.testing.assert_allclose(O.correct_distances(f["dist_%d" % s], metric), f["corrected_%d" % s], rtol=1e-12, atol=0)
    edge = np.array([0.0, 0.5, 2.0, MU.FLT_MAX], np.float32)
    np.testing.assert_allclose(O.correct_distances(edge, metric), MU.correct(metric, edge), rtol=1e-12, atol=0)


@pytest.mark.parametrize("metric", MU.NEW_METRICS)
def test_brute_force_ranks_by_each_metric(metric):
    f = _golden(metric)
    xs = _space(metric, f["x"])
    rows = np.arange(0, xs.shape[0], 11)
    oi, od = O.brute_force_knn(xs, 10, metric, rows=rows)
    want = MU.alt_dist(metric, xs[rows], xs)
    # (float64 sums in another order: 4.4e-16 apart; hellinger's sqrt(1 - 2^-d) turns that into 1.5e-8 next to 0)
    np.testing.assert_allclose(od, MU.correct(metric, np.take_along_axis(want, oi.astype(np.int64), 1)), rtol=1e-9, atol=1e-7)
    # the distances of every row are the true k smallest (ids may differ on ties)
    np.testing.assert_allclose(np.take_along_axis(want, oi.astype(np.int64), 1), np.sort(want, 1)[:, :10], rtol=1e-9,
                               atol=1e-12)


@pytest.mark.parametrize("metric", MU.NEW_METRICS)
def test_builds_match_reference_recall(metric):
    """three seeds: recall@10 within 0.005 of the reference's recorded recall (the bar of the cosine pins); inner product
    also keeps the reference's share of rows that list themselves first (d(x, x) = 1 / |x|^2)."""
    f = _golden(metric)
    xs = _space(metric, f["x"])
    truth = MU.brute_knn(metric, xs, k=10)
    for s in f["seeds"]:
        oi, od = O.build_index(xs, metric, n_neighbors=10, random_state=int(s), n_threads=1)
        r = MU.recall(truth, oi)
        assert abs(r - float(f["recall_%d" % s])) <= 0.005, (int(s), r, float(f["recall_%d" % s]))
        if metric == "inner_product":
            assert abs(MU.self_first_share(oi) - float(f["self_first_%d" % s])) <= 0.05


@pytest.mark.parametrize("metric", MU.NEW_METRICS)
def test_search_graph_matches_reference(metric):
    """the pruning pass of prepare() on the reference's own seed-3 graph against the reference's search graph, at the 1 %
    bar of the cosine pins (measured: identical for all four metrics).  The row's own vertex as a comparison point takes
    the stored d(i, j) (nnd_oracle.c orc_cmp_dist): recomputed with libm's log2f instead of the fixture's numpy log2, the
    dot self distances above EPS flipped 184 of 8320 edges."""
    f = _golden(metric)
    sg = np.load(os.path.join(GOLDEN, "metric_search_graph.npz"))
    xs = _space(metric, f["x"])
    g = O.search_graph(xs, f["idx_3"], f["dist_3"], metric, 10)
    coo = g.tocoo()
    got = set(zip(coo.row.tolist(), coo.col.tolist()))
    want = set(zip(sg[metric + "_rows"].tolist(), sg[metric + "_cols"].tolist()))
    assert len(got ^ want) <= 0.01 * len(want), (len(got ^ want), len(want))
