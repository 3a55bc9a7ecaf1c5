"""metric="proxy_inner_product": the host side -- the float64 formula against the reference's recorded graph
(tests/golden/proxy_inner_product.npz, tests/golden/make_golden_proxy.py), the metric record, the errors raised before any
device work, and the share of queries the search model (tests/proxy_reference.py) leaves to the weak checks.  No GPU needed."""
import numpy as np
import pytest

import pynndescent_amd
from pynndescent_amd import NNDescent, _capi, nndescent
from tests import proxy_reference as PR
from tests import proxy_util as PU
from tests.search_cases import FLOAT_CAP

OTHER_PROXIES = ("proxy_wasserstein_1d", "proxy_wasserstein-1d", "proxy_kantorovich", "proxy_wasserstein", "proxy_circular_kantorovich",
                 "proxy_circular_wasserstein", "proxy_jensen_shannon", "proxy_jensen-shannon", "proxy_symmetric_kl", "proxy_symmetric-kl",
                 "proxy_sinkhorn")


@pytest.fixture
def no_library(monkeypatch):
    """any call into the library (a handle, a searcher, a device) fails the test"""
    def boom(*a, **k):
        raise AssertionError("the library was called before the arguments were checked")

    monkeypatch.setattr(_capi, "Builder", boom)
    monkeypatch.setattr(_capi, "Searcher", boom)
    monkeypatch.setattr(_capi, "load_library", boom)


def _index(quantization=None, n=300, d=8):
    """An un-prepared index around a small random graph (no device work until prepare())."""
    rs = np.random.RandomState(0)
    x = np.abs(rs.standard_normal((n, d))).astype(np.float32)
    idx = np.stack([(np.arange(n) + j) % n for j in range(10)], 1).astype(np.int32)
    dist = np.sort(rs.uniform(0.1, 1.0, idx.shape), axis=1).astype(np.float32)
    return NNDescent.from_graph(x, idx, dist, metric=PU.METRIC, random_state=3, quantization=quantization)


def test_metric_record():
    m = nndescent._METRICS[PU.METRIC]
    assert m.code == _capi.METRIC_CODES[PU.METRIC] == _capi.NND_METRIC_PROXY_INNER_PRODUCT == PU.CODE == 6
    assert m.proxy and not m.angular and not m.uint8 and not m.normalize and not m.nonnegative
    assert m.correction is _capi.host_copy
    assert [name for name, r in nndescent._METRICS.items() if r.proxy] == [PU.METRIC]
    assert nndescent._ND_DISTS[PU.METRIC] == (6, None)  # nn_descent hands the proxy distances out uncorrected
    assert "nnd_searcher_query_rerank" in _capi.EXPORTED_SYMBOLS
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pynnd_amd.h")).read()
    assert re.findall(r"enum \{ NND_METRIC_PROXY_INNER_PRODUCT = (\d+) \};", header) == ["6"]  # the header's constant is _capi's


def test_constructor_accepts_the_name(no_library):
    """The metric is known: construction gets as far as the device (here: the patched-out library), where it used to stop at
    ValueError("Metric is neither callable, nor a recognised string")."""
    x = np.abs(np.random.RandomState(1).standard_normal((64, 4))).astype(np.float32)
    with pytest.raises(AssertionError, match="library was called"):
        NNDescent(x, metric=PU.METRIC, n_neighbors=5)


def test_from_graph_mirrors_the_reference_flags(no_library):
    index = _index()
    assert index._is_proxy_distance is True and index._angular_trees is False
    d = np.float32([[0.5, 1.5]])
    out = index._distance_correction(d)
    assert np.array_equal(out, d) and out is not d  # no correction: a copy
    plain = NNDescent.from_graph(index._raw_data, *index._neighbor_graph, metric="inner_product")
    assert plain._is_proxy_distance is False


def test_host_errors_come_before_any_device_work(no_library):
    with pytest.raises(ValueError, match="Not uint8 quantization version of proxy_inner_product"):
        _index("uint8").prepare()
    with pytest.raises(ValueError, match="Not uint8 quantization version of proxy_inner_product"):
        _index("uint8").query(np.zeros((2, 8), np.float32), k=5)
    index = _index()
    with pytest.raises(NotImplementedError, match="260"):
        index.query(np.zeros((2, 8), np.float32), k=65, proxy_beam_size=4)
    with pytest.raises(ValueError, match="proxy_beam_size"):
        index.query(np.zeros((2, 8), np.float32), k=10, proxy_beam_size=0)
    assert not hasattr(index, "_search_graph")
    with pytest.raises(NotImplementedError, match="proxy_inner_product"):
        pynndescent_amd.exact_knn(index._raw_data, k=3, metric=PU.METRIC)
    with pytest.raises(NotImplementedError, match="proxy_inner_product"):
        index.recall(n_rows=10, random_state=0)


@pytest.mark.parametrize("name", OTHER_PROXIES)
def test_other_proxy_names_are_the_references(name, no_library):
    """Names the reference accepts (distances.py proxy_distances) and this package does not run: NotImplementedError, which
    make_index turns into the reference's own build, not the ValueError of an unknown string."""
    assert name in nndescent._KNOWN_REFERENCE_METRICS
    x = np.zeros((20, 4), np.float32)
    with pytest.raises(NotImplementedError, match="use pynndescent.NNDescent"):
        NNDescent(x, metric=name, n_neighbors=5)
    with pytest.raises(ValueError, match="Metric is neither callable"):
        NNDescent(x, metric="proxy_no_such_thing", n_neighbors=5)


def test_formula_agrees_with_the_fixture_graph():
    """The reference evaluates proxy_inner_product with float32 accumulators: a float32 sum of d products, one log2 and one
    sqrt around it.  Every distance it stored lies in the a-priori interval of tests/proxy_util.py around the float64 formula
    for the ids it stored; FLT_MAX and +inf both mean "infinitely far" (the reference gives +inf at <x,y> = 0)."""
    g = np.load(PU.GOLDEN)
    x = g["x"]
    worst = 0.0
    for seed in PU.SEEDS:
        idx, dist = g["graph_idx_%d" % seed], g["graph_dist_%d" % seed]
        assert idx.shape == dist.shape == (2000, PU.K) and (idx >= 0).all()
        mid, lo, hi = PU.proxy_pairs_f32(x[:, None, :], x[idx])
        assert PU.within(dist, lo, hi).all()
        fin = mid < PU.FLT_MAX
        worst = max(worst, float(np.max(np.abs(dist[fin] - mid[fin]) / np.maximum(hi - mid, mid - lo)[fin])))
        assert np.all(np.diff(dist.astype(np.float64), axis=1) >= 0.0)
        assert abs(float(g["min_distance_%d" % seed]) - 0.0412) < 5e-4
    print("largest |reference - float64| in units of the radius: %.3f" % worst)


def test_fixture_recalls_are_the_recorded_ones():
    """The stored recalls are those of the stored answers against float64 truth recomputed here."""
    g = np.load(PU.GOLDEN)
    x, q = g["x"], g["queries"]
    fx, fq = PU.fixture_data()
    assert np.array_equal(x, fx) and np.array_equal(q, fq)
    mips, proxy_nn = PU.mips_truth(x, q), PU.proxy_truth(x)
    for seed in PU.SEEDS:
        assert PU.recall(proxy_nn, g["graph_idx_%d" % seed]) == pytest.approx(float(g["graph_recall_%d" % seed]), abs=1e-12)
        for beam in (4, 1):
            qi, qd = g["q_idx_b%d_%d" % (beam, seed)], g["q_dist_b%d_%d" % (beam, seed)]
            assert PU.recall(mips, qi) == pytest.approx(float(g["q_recall_b%d_%d" % (beam, seed)]), abs=1e-12)
            ip = -np.einsum("qd,qkd->qk", q.astype(np.float64), x[qi].astype(np.float64))
            np.testing.assert_allclose(qd, ip, rtol=0, atol=16 * PU.gamma(16) * float(np.abs(ip).max()))
    assert float(g["q_recall_b4_3"]) == pytest.approx(0.5285, abs=1e-4) and float(g["q_recall_b1_3"]) == pytest.approx(0.196, abs=1e-4)


def test_interval_contains_the_float32_evaluation():
    """proxy_interval is a bound on ANY float32 evaluation of the formula from float32 sums: the straightforward numpy float32
    one lies inside it, on rows of every length from 1e-15 to 1 and at the FLT_MAX places."""
    rs = np.random.RandomState(5)
    a = (np.abs(rs.standard_normal((400, 17))) * 10.0 ** rs.uniform(-15, 0, (400, 1))).astype(np.float32)
    b = (np.abs(rs.standard_normal((400, 17))) * 10.0 ** rs.uniform(-3, 0, (400, 1))).astype(np.float32)
    a[3] = 0.0
    b[5] = -b[5]
    g32 = np.einsum("nd,nd->n", a, b, dtype=np.float32)
    na, nb = np.einsum("nd,nd->n", a, a, dtype=np.float32), np.einsum("nd,nd->n", b, b, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.maximum(-np.log2(g32 / np.sqrt(na * nb)), np.float32(0)) + np.float32(1) / np.sqrt(g32)
    v = np.where((na == 0) | (nb == 0) | ~(g32 > 0), np.float32(PU.FLT_MAX), v)
    mid, lo, hi = PU.proxy_pairs_f32(a, b)
    assert mid[3] == PU.FLT_MAX and mid[5] == PU.FLT_MAX and lo[3] == hi[3] == PU.FLT_MAX
    assert PU.within(v, lo, hi).all()
    assert np.all(hi[mid < PU.FLT_MAX] - lo[mid < PU.FLT_MAX] < 1e-4 * mid[mid < PU.FLT_MAX] + 4 * PU.LOG_TERM_ABS)


@pytest.mark.parametrize("d,k,search_k", PR.SEARCH_CASES)
def test_search_cases_stay_under_the_ambiguity_cap(d, k, search_k):
    """The GPU comparison is entry for entry on the queries the model does not flag; at most a tenth may be flagged (the cap of
    the float cases of tests/search_cases.py).  Every list must fill, and no case may be answered by FLT_MAX ties."""
    case, res = PR.search_case(d, k, search_k)
    amb = float(np.mean([r.ambiguous for r in res]))
    print("%s: %.1f %% of %d queries flagged (%s); visited %d .. %d" % (
        case.name, 100.0 * amb, len(res), sorted({w for r in res for w in r.reason.split("; ") if w}), min(r.V for r in res), max(r.V for r in res)))
    assert amb <= FLOAT_CAP
    assert all((r.ids >= 0).all() and len(set(r.ids.tolist())) == k for r in res)
    assert all(np.all(np.diff(r.dists) >= 0.0) and np.all(r.dists < 0.0) for r in res)


def test_lattice_case_is_a_lattice():
    case, res = PR.lattice_case()
    assert np.all(case.data == np.rint(case.data)) and np.all(case.queries == np.rint(case.queries))
    assert case.data.shape[1] * float(max(np.abs(case.data).max(), np.abs(case.queries).max())) ** 2 < 2.0 ** 24
    amb = float(np.mean([r.ambiguous for r in res]))
    print("%s: %.1f %% of %d queries flagged" % (case.name, 100.0 * amb, len(res)))
    assert amb <= FLOAT_CAP
    assert all(np.all(r.radius[r.ids >= 0] == 0.0) and np.all(r.dists[r.ids >= 0] == np.rint(r.dists[r.ids >= 0])) for r in res)
