"""quantization="uint8" on a real MI355X: the device codes against np.searchsorted, an index against the reference's own
(tests/golden/quantized_uint8.npz, tests/golden/make_golden_quantized.py), both search tiers, pickling, and the rerank's
exact distances."""
import os
import pickle
import types

import numpy as np
import pytest

from pynndescent_amd import NNDescent, _capi
from tests import metric_util as MU
from tests import quantized_util as QU

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantized_uint8.npz")
METRICS = ("euclidean", "cosine", "dot")
_BUILT = {}


def _golden():
    return np.load(GOLDEN)


def _built(metric):
    """The fixture's index on the GPU, prepared, and its answers to the fixture's queries (built once per metric)."""
    if metric not in _BUILT:
        x, q = QU.fixture_data(metric)
        index = NNDescent(x, metric=metric, n_neighbors=QU.K, random_state=3, quantization="uint8")
        index.prepare()
        qi, qd = index.query(q, k=QU.K)
        _BUILT[metric] = (index, q, qi, qd)
    return _BUILT[metric]


def _searcher(x, metric=_capi.NND_METRIC_SQEUCLIDEAN):
    """A searcher over x with a ring graph and no tree: enough to quantize through the ABI."""
    n = x.shape[0]
    graph = types.SimpleNamespace(indptr=np.arange(n + 1, dtype=np.int32), indices=((np.arange(n) + 1) % n).astype(np.int32))
    return _capi.Searcher(x, graph, None, metric, 0.0, 10, np.array([1, 2, 3], np.int64))


def _edge_rows(values, n=50_000, d=24, seed=0):
    """Rows of values below, equal to, just around and above the codebook entries (above the last one: code n_values,
    and for 256 entries the wrap to 0)."""
    rs = np.random.RandomState(seed)
    v = values.astype(np.float32)
    pool = np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf)),
                           v - np.float32(1e-3), v + np.float32(1e-3), [v[0] - np.float32(1.0), v[-1] + np.float32(1.0)]])
    pool = pool.astype(np.float32)
    # no subnormals: a -ffast-math library loaded earlier in the process (the oracle's timing build) sets the CPU's
    # denormals-are-zero flag, and the host's np.searchsorted would then compare them as 0 while the device does not
    bits = pool.view(np.uint32) & np.uint32(0x7FFFFFFF)  # (told apart by their bits: DAZ makes them compare equal to 0)
    pool = pool[(bits == 0) | (bits >= np.uint32(0x00800000))]
    x = rs.choice(pool, size=(n, d))
    mixed = rs.uniform(v[0] - 0.5, v[-1] + 0.5, size=(n // 4, d)).astype(np.float32)
    x[: n // 4] = mixed
    return np.ascontiguousarray(x, np.float32)


@pytest.mark.parametrize("codebook", ["quantiles_256", "unique_short"])
def test_device_codes_equal_searchsorted(codebook):
    rs = np.random.RandomState(4)
    if codebook == "quantiles_256":
        values = np.quantile(rs.standard_normal(100_000), np.linspace(0, 1, 256)).astype(np.float32)
    else:
        values = np.unique(rs.randint(-20, 20, 200).astype(np.float32) * np.float32(0.125))
    x = _edge_rows(values)
    want = np.searchsorted(values, x).astype(np.uint8)
    assert (want == 0).sum() > (x <= values[0]).sum() or len(values) < 256  # the wrap is exercised (256 entries)
    s = _searcher(x)
    try:
        got = s.quantize_u8(values)
        np.testing.assert_array_equal(got, want)
        got_rows = s.quantize_u8(values, rows=x[::-1].copy())  # rows handed in by the host
        np.testing.assert_array_equal(got_rows, want[::-1])
    finally:
        s.close()


@pytest.mark.parametrize("metric", METRICS)
def test_fixture_codes_recall_and_exact_distances(metric):
    g = _golden()
    index, q, qi, qd = _built(metric)
    np.testing.assert_array_equal(index._quantized_values, g["values_%s" % metric])
    ours = index._quantized_data[np.argsort(index._vertex_order)]
    ref = g["codes_%s" % metric][np.argsort(g["vertex_order_%s" % metric])]
    assert ours.dtype == np.uint8 and ours.tobytes() == ref.tobytes()

    x = index._raw_data[np.argsort(index._vertex_order)]  # dot: the normalised rows NNDescent holds
    rec = MU.recall(QU.truth(metric, x, q), qi)
    assert abs(rec - float(g["recall_uint8_%s" % metric])) <= 0.01, (rec, float(g["recall_uint8_%s" % metric]))

    live = qi >= 0
    if metric == "dot":  # the zero query is skipped: nothing found (the convention of unquantized queries)
        assert not live[5].any()
        live[5] = False
    assert live[np.arange(len(q)) != (5 if metric == "dot" else -1)].all()
    want = QU.exact_corrected(metric, x, q, qi)
    np.testing.assert_allclose(qd[live], want[live], rtol=2e-4, atol=2e-6)
    assert (np.diff(qd[live.all(1)], axis=1) >= 0).all()
    if metric == "dot":
        assert (qd[live] < 0).any()  # 1 - q.x with the raw query: below 0 where |q| > 1


@pytest.mark.parametrize("metric", METRICS)
def test_global_tier_gives_the_same_answers(metric):
    index, q, qi, qd = _built(metric)
    index._searcher.set_tier(1)
    try:
        qi1, qd1 = index.query(q, k=QU.K)
        assert index._searcher.last_spilled() == q.shape[0]
    finally:
        index._searcher.set_tier(0)
    np.testing.assert_array_equal(qi1, qi)
    np.testing.assert_array_equal(qd1, qd)


def test_pickled_index_answers_identically():
    index, q, qi, qd = _built("cosine")
    loaded = pickle.loads(pickle.dumps(index))
    assert loaded._searcher is None
    np.testing.assert_array_equal(loaded._quantized_data, index._quantized_data)
    loaded.random_state = 12345  # a re-derived codebook would differ: the loaded one is reused
    qi2, qd2 = loaded.query(q, k=QU.K)
    np.testing.assert_array_equal(loaded._quantized_values, index._quantized_values)
    np.testing.assert_array_equal(qi2, qi)
    np.testing.assert_array_equal(qd2, qd)
    assert loaded._quantized_data is not None and loaded._searcher.has_codes


def test_beam_and_wide_lists():
    """proxy_beam_size 1 (the walk keeps k) and search_k = 256 (four list entries per lane) on a d that is no multiple of
    16 (the code rows' padding): sorted exact distances; at beam 4 recall no worse than the unquantized search's minus 0.02
    (beam 1 reranks only the k proxy results: lower, here about 0.9 against 0.97)."""
    x, q = QU.fixture_data("euclidean")
    x, q = np.ascontiguousarray(x[:, :13]), np.ascontiguousarray(q[:, :13])
    index = NNDescent(x, metric="euclidean", n_neighbors=QU.K, random_state=5, quantization="uint8")
    plain = NNDescent(x, metric="euclidean", n_neighbors=QU.K, random_state=5)
    t = QU.truth("euclidean", x, q)
    rec_plain = MU.recall(t, plain.query(q, k=QU.K)[0])
    for k, beam in ((10, 1), (10, 4), (64, 4)):
        qi, qd = index.query(q, k=k, proxy_beam_size=beam)
        assert qi.shape == (q.shape[0], k) and (qi >= 0).all()
        np.testing.assert_allclose(qd, QU.exact_corrected("euclidean", x, q, qi), rtol=2e-4, atol=2e-6)
        assert (np.diff(qd, axis=1) >= 0).all()
        assert all(len(set(r)) == k for r in qi)
        if k == 10:
            floor = rec_plain - 0.02 if beam == 4 else 0.8
            assert MU.recall(t, qi) >= floor, (beam, MU.recall(t, qi), rec_plain)
