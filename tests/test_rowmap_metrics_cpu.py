"""spearmanr and haversine on the host side: the derived-metric registry next to the metric table, every refusal before any
device work, the numpy models of the two row maps against the reference's own values (tests/golden/metric_rowmap.npz), and the
derived haversine error bound re-checked on the CPU model.  No GPU."""
import os
import pickle

import numpy as np
import pytest

from pynndescent_amd import NNDescent, _capi, exact_knn, linear_map, metrics, row_map
from tests import metric_util as MU
from tests import rowmap_util as RU
from tests.test_host_layout_cpu import BOOLEAN, LINEAR, PLAIN

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "metric_rowmap.npz"))


def test_the_table_is_what_it_was_and_the_registry_stands_beside_it():
    assert list(metrics._METRIC_TABLE) == PLAIN + LINEAR + BOOLEAN
    assert [list(v) for v in (metrics._METRICS, metrics._LINEAR_METRICS, metrics._BOOLEAN_METRICS)] == [PLAIN, LINEAR, BOOLEAN]
    assert metrics._ANGULAR_METRICS == frozenset(["cosine", "dot", "correlation", "hellinger"])
    assert not {"spearmanr", "haversine"} & set(metrics._ND_DISTS)
    assert all(m.row_map is None and m.mapped == m.linear for m in metrics._METRIC_TABLE.values())
    assert list(row_map.ROW_MAP_METRICS) == ["spearmanr", "haversine"]
    assert {"spearmanr", "haversine"} <= metrics._KNOWN_REFERENCE_METRICS

    s = metrics._metric_record("spearmanr")
    assert s is metrics._metric_of("spearmanr") is metrics._metric_record("spearmanr", reference_fallback=False)
    assert s.code == _capi.METRIC_CODES["correlation"] == 4 and s.row_map.kind == _capi.NND_ROWMAP_RANK == 0
    assert s.correction is _capi.host_copy and s.device_kind == _capi.NND_CORRECT_COPY
    assert s.kernel_metric == "correlation" and s.mapped and not s.linear

    h = metrics._metric_record("haversine")
    assert h is metrics._metric_of("haversine")
    assert h.code == _capi.METRIC_CODES["euclidean"] == 0 and h.row_map.kind == _capi.NND_ROWMAP_SPHERE == 1
    assert h.correction is row_map.correct_haversine and h.device_kind == _capi.NND_CORRECT_HAVERSINE == 5
    assert h.kernel_metric == "euclidean" and h.row_map.in_dim == 2 and h.row_map.out_dim == 3
    for m in (s, h):  # what the reference reports for these names, and nothing of the base metric's but its code
        assert not (m.angular or m.uint8 or m.normalize or m.nonnegative or m.proxy or m.boolean)
    assert metrics._metric_of("euclidean").kernel_metric is None and metrics._metric_of("mahalanobis").kernel_metric == "euclidean"


def test_the_refusal_of_other_names_names_the_new_ones():
    with pytest.raises(NotImplementedError, match="use pynndescent.NNDescent for metric 'manhattan'") as e:
        metrics._metric_record("manhattan")
    assert "spearmanr" in str(e.value) and "haversine" in str(e.value) and "mahalanobis" in str(e.value)
    with pytest.raises(NotImplementedError):
        metrics._metric_record("true_angular")


def test_every_refusal_comes_before_any_device_work():
    sp = pytest.importorskip("scipy.sparse")
    x8 = RU.decimal_rows(60, 8, seed=1)
    x2 = RU.latlon_rows(60, seed=1)
    for metric, x in (("spearmanr", x8), ("haversine", x2)):
        with pytest.raises(ValueError, match="Metric %s not supported for sparse data" % metric):
            NNDescent(sp.csr_matrix(x), metric=metric, n_neighbors=5)
        with pytest.raises(ValueError, match="Metric %s not supported for sparse data" % metric):
            exact_knn(sp.csr_matrix(x), k=5, metric=metric)
        with pytest.raises(ValueError, match="Not uint8 quantization version of %s" % metric):
            NNDescent(x, metric=metric, n_neighbors=5, quantization="uint8")
        with pytest.raises(NotImplementedError, match="n_devices"):
            NNDescent(x, metric=metric, n_neighbors=5, n_devices=2)
    for bad in (x8, x2[:, :1]):
        with pytest.raises(ValueError, match="haversine is only defined for 2 dimensional graph_data"):
            NNDescent(bad, metric="haversine", n_neighbors=5)
        with pytest.raises(ValueError, match="haversine is only defined for 2 dimensional graph_data"):
            exact_knn(bad, k=5, metric="haversine")
    wide = np.zeros((4, row_map.RANK_MAX_DIM + 1), np.float32)
    with pytest.raises(NotImplementedError, match="at most %d columns" % row_map.RANK_MAX_DIM):
        NNDescent(wide, metric="spearmanr", n_neighbors=2)
    assert row_map.RANK_MAX_DIM == 16384 < 2 ** 23
    assert row_map.row_map_of(row_map.ROW_MAP_METRICS["spearmanr"], 16384) == row_map.RowMap(_capi.NND_ROWMAP_RANK, None)
    for metric, x in (("spearmanr", x8), ("haversine", x2)):  # NaN / inf: the mapped rows would hide them, so they are scanned for
        bad = x.copy()
        bad[3, 1] = np.nan
        with pytest.raises(ValueError, match="NaN"):
            NNDescent(bad, metric=metric, n_neighbors=5)


def test_from_graph_keeps_the_callers_rows_and_fixes_the_shift():
    x2 = RU.latlon_rows(5000, seed=2)
    idx, dist = np.tile(np.arange(5, dtype=np.int32), (5000, 1)), np.zeros((5000, 5), np.float32)
    index = NNDescent.from_graph(x2, idx, dist, metric="haversine", random_state=1)
    assert index.dim == 2 and index._raw_data.shape == (5000, 2) and not index._angular_trees
    assert index._distance_correction is row_map.correct_haversine and index._kernel_metric() == "euclidean"
    m = index._linear_map
    assert isinstance(m, row_map.RowMap) and m.kind == _capi.NND_ROWMAP_SPHERE and m.shift.dtype == np.float32
    assert np.array_equal(m.shift, RU.sphere_shift(x2))
    assert np.array_equal(m.shift, RU.sphere_points(x2[linear_map.shift_rows(5000)]).mean(0).astype(np.float32))
    assert pickle.loads(pickle.dumps(m)).kind == m.kind and pickle.loads(pickle.dumps(index._distance_correction)) is row_map.correct_haversine
    s = NNDescent.from_graph(RU.decimal_rows(50, 8, seed=3), idx[:50], dist[:50], metric="spearmanr")
    assert s._linear_map == row_map.RowMap(_capi.NND_ROWMAP_RANK, None) and s._kernel_metric() == "correlation" and s.dim == 8


def test_the_haversine_correction():
    s = np.array([0.0, 1.0, 2.0, 4.0, 4.0000005, np.inf], np.float32)
    got = row_map.correct_haversine(s)
    assert got.dtype == np.float64 and got is not s
    np.testing.assert_allclose(got, [0.0, np.pi / 3, np.pi / 2, np.pi, np.pi, np.pi], rtol=1e-15)
    assert np.array_equal(got, RU.haversine_of_chord2(s))


def test_rank_models_agree_and_match_the_reference(golden):
    x = golden["rank_x"]
    r = RU.model_ranks(x)
    assert r.dtype == np.float32 and np.array_equal(r, RU.model_ranks_counting(x))
    assert np.array_equal(r[1], np.full(8, 4.5, np.float32))  # the constant row
    assert set(r[2]) == {4.0, 8.0}  # seven signed zeros tie, the one above them
    wide = RU.tied_rows(3, 1500, seed=4)
    assert np.array_equal(RU.model_ranks(wide), RU.model_ranks_counting(wide))
    stats = pytest.importorskip("scipy.stats")
    assert np.array_equal(r, stats.rankdata(x, method="average", axis=1).astype(np.float32))
    pairs = golden["pairs"]
    got = RU.spearmanr64(x[pairs[:, 0]], x[pairs[:, 1]])
    np.testing.assert_allclose(got, golden["spearmanr_pairs"], rtol=1e-5, atol=1e-6)
    assert (got[:300] == 0.0).all()
    # the reference's ten nearest neighbours, by the model: the same distances row by row (ids may differ on ties)
    dm = MU.alt_dist("correlation", r, r)
    np.testing.assert_allclose(np.sort(dm, 1)[:, :10], golden["spearmanr_knn_dist"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(np.take_along_axis(dm, golden["spearmanr_knn_idx"].astype(np.int64), 1), golden["spearmanr_knn_dist"],
                               rtol=1e-5, atol=1e-6)


def _model_haversine(x, ia, ib, shift):
    """What the device hands out for the pairs, modelled: the float32 sphere rows, the float64 sum of their squared differences
    rounded to float32 (csrc/metric.h, the distances handed back), the correction."""
    rows = RU.model_sphere(x, shift).astype(np.float64)
    s = ((rows[ia] - rows[ib]) ** 2).sum(-1).astype(np.float32)
    return row_map.correct_haversine(s), float(np.abs(rows).max())


def test_sphere_model_matches_the_reference_within_the_derived_bound(golden):
    x, pairs = golden["sphere_x"], golden["pairs"]
    got, m_abs = _model_haversine(x, pairs[:, 0], pairs[:, 1], RU.sphere_shift(x))
    want = golden["haversine_pairs"]
    assert (got[:300] == 0.0).all() and got[np.flatnonzero((pairs == [4, 5]).all(1))].sum() == 0.0
    near = want <= 3.0
    assert near.sum() > 1900
    # the fixture's values are the reference's formula in float64 on the float32 inputs: its own error, a few float64 roundings
    # amplified by 1 / cos(theta / 2) <= 15, is far below 1e-12
    ref_err = 1e-12
    assert (np.abs(got[near] - want[near]) <= RU.haversine_bound(want[near], m_abs) + ref_err).all()
    np.testing.assert_allclose(RU.haversine64(x[pairs[:, 0]], x[pairs[:, 1]])[near], want[near], rtol=0, atol=ref_err)
    np.testing.assert_allclose(RU.haversine64(x[pairs[:, 0]], x[pairs[:, 1]])[~near], want[~near], rtol=0, atol=1e-9)
    dm = RU.haversine64(x[:, None, :], x[None, :, :])
    np.testing.assert_allclose(np.sort(dm, 1)[:, :10], golden["haversine_knn_dist"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("region", [None, (0.7, 2.1, 0.05), (0.7, 2.1, 0.002), (-1.2, -3.0, 0.3)])
def test_the_haversine_bound_holds_on_the_cpu_model(region):
    """|err| <= 4e-7 * M / cos(theta / 2) against the float64 formula on the float32 inputs, theta <= 3.0 (DESIGN.md "Row maps"
    quotes the worst ratio printed here)."""
    x = RU.latlon_rows(20000, seed=12, region=region)
    rs = np.random.RandomState(13)
    ia, ib = rs.randint(0, 20000, 200000), rs.randint(0, 20000, 200000)
    got, m_abs = _model_haversine(x, ia, ib, RU.sphere_shift(x))
    want = RU.haversine64(x[ia], x[ib])
    keep = want <= 3.0
    ratio = np.abs(got[keep] - want[keep]) / RU.haversine_bound(want[keep], m_abs)
    print("region %r: M = %.3g, worst |err| %.3g rad, worst ratio to the bound %.3f" % (region, m_abs, np.abs(got[keep] - want[keep]).max(),
                                                                                         ratio.max()))
    assert ratio.max() <= 1.0
    if region is not None:  # the point of the shift: the error scales with the extent of the data
        assert m_abs < 3.0 * region[2] + 1e-3
