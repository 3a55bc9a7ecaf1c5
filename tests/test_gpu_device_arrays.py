"""NNDescent on device arrays (torch tensors on the GPU) on a real MI355X: the device-resident build against the host build of
the same values, half precision and float64 input, dot's device normalisation, neighbor_graph and query as tensors with the
corrections done on the device, the errors and the warning of the host path, the lazily fetched host mirrors through the life
cycle of an index, and the stream rule."""
import functools
import pickle
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from sklearn.preprocessing import normalize  # noqa: E402

from pynndescent_amd import NNDescent, _capi  # noqa: E402
from pynndescent_amd import nndescent as N  # noqa: E402
from tests import metric_util as MU  # noqa: E402
from tests.util_data import clustered  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 10
SEED = 5
BUILD_METRICS = ("euclidean", "cosine", "correlation", "hellinger", "inner_product", "proxy_inner_product")
FLOAT32_OUT = ("euclidean", "l2", "sqeuclidean", "correlation", "proxy_inner_product")


def _data(metric, n, d):
    x = clustered(n, d, 6, 24, 40 + d, nonneg=metric == "hellinger")
    if metric in ("inner_product", "proxy_inner_product"):
        x = x + np.float32(0.5)
    return x


@functools.lru_cache(maxsize=None)
def _host_index(metric, n, d):
    return NNDescent(_data(metric, n, d), metric=metric, n_neighbors=K, random_state=SEED)


@functools.lru_cache(maxsize=None)
def _device_index(metric, n, d):
    return NNDescent(torch.from_numpy(_data(metric, n, d)).to(DEV), metric=metric, n_neighbors=K, random_state=SEED)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _assert_same_graph(got, want):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32
    assert np.array_equal(got[0], want[0])
    assert _same_bits(got[1], want[1])


def _assert_distances(metric, got, host):
    """``got`` (the device's corrected distances, as numpy) against the host's correction of the same kernel distances: the same
    bits where the correction is a copy, a float32 square root or an IEEE division; 1 - 2^-d within 2^-50 (2^-d in (0, 1] to one
    ulp on each side, <= 2^-52, one rounding of the subtraction on each side, <= 2^-53 each, a factor of two in hand);
    hellinger on the squares with that bound doubled (the square root is unbounded in relative terms at 0)."""
    assert got.dtype == host.dtype == (np.float32 if metric in FLOAT32_OUT else np.float64)
    assert got.shape == host.shape
    if metric in FLOAT32_OUT or metric == "inner_product":
        assert _same_bits(got, host)
    elif metric in ("cosine", "dot"):
        assert np.all(np.abs(got - host) <= 2.0 ** -50), np.abs(got - host).max()
    else:
        assert metric == "hellinger"
        assert np.all(np.abs(got * got - host * host) <= 2.0 ** -49), np.abs(got * got - host * host).max()


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("d", [23, 128])
@pytest.mark.parametrize("metric", BUILD_METRICS)
def test_float32_device_build_equals_host_build(metric, d):
    host, dev = _host_index(metric, 3000, d), _device_index(metric, 3000, d)
    _assert_same_graph(dev._neighbor_graph, host._neighbor_graph)
    assert np.array_equal(dev.rng_state, host.rng_state) and np.array_equal(dev.search_rng_state, host.search_rng_state)
    assert dev._build_stats["n_iters_run"] == host._build_stats["n_iters_run"]


def test_float32_tensor_is_kept_by_reference():
    x = torch.from_numpy(_data("euclidean", 500, 16)).to(DEV)
    index = NNDescent(x, n_neighbors=K, random_state=SEED)
    assert index._device_data is x and index.device == 0
    assert "_neighbor_graph" not in index.__dict__ and "_raw_data" not in index.__dict__  # nothing came to the host
    xt = torch.from_numpy(_data("euclidean", 16, 500)).to(DEV).t()  # not contiguous: made contiguous on the device
    assert not xt.is_contiguous()
    twin = NNDescent(xt, n_neighbors=K, random_state=SEED)
    assert twin._device_data.is_contiguous() and twin._device_data.is_cuda
    want = NNDescent(np.ascontiguousarray(xt.cpu().numpy()), n_neighbors=K, random_state=SEED)
    _assert_same_graph(twin._neighbor_graph, want._neighbor_graph)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("d", [23, 128])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16", "float64"])
def test_half_precision_and_float64_input(dtype, d):
    n = 2001  # the last conversion block is partial
    x = _data("euclidean", n, d)
    if dtype == "float64":
        x64 = x.astype(np.float64) * (1.0 + 1e-9 * np.random.RandomState(3).standard_normal(x.shape))
        x64[0, 0], x64[0, 1], x64[0, 2] = 1.0 + 2.0 ** -24, 1.0 + 3.0 * 2.0 ** -24, -(1.0 + 2.0 ** -24)  # ties: to even
        xt = torch.from_numpy(x64).to(DEV)
        up = x64.astype(np.float32)
        assert up[0, 0] == 1.0 and up[0, 1] == np.float32(1.0 + 2.0 ** -22)
    else:
        xt = torch.from_numpy(x).to(DEV).to(getattr(torch, dtype))
        up = xt.float().cpu().numpy()
        assert not np.array_equal(up, x)  # the rounding to 16 bits is part of the input
    dev = NNDescent(xt, n_neighbors=K, random_state=SEED)
    host = NNDescent(up, n_neighbors=K, random_state=SEED)
    _assert_same_graph(dev._neighbor_graph, host._neighbor_graph)
    assert _same_bits(dev._raw_data, up)


@pytest.mark.parametrize("dtype", ["float16", "float64"])
def test_conversion_of_a_view_that_starts_off_the_vector_grid(dtype):
    """Rows 1.. of an odd-d tensor start 2 * 23 (8 * 23) bytes into the allocation: the scalar head of the conversion."""
    base = torch.from_numpy(_data("euclidean", 1001, 23)).to(DEV).to(getattr(torch, dtype))
    view = base[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    out = torch.full((1000, 23), float("nan"), dtype=torch.float32, device=DEV)
    _capi.device_rows_f32(0, torch.cuda.current_stream().cuda_stream, view.data_ptr(), N._DEVICE_DTYPES[dtype], 1000, 23, False,
                          out.data_ptr())
    assert _same_bits(out.cpu().numpy(), view.float().cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- 3
@functools.lru_cache(maxsize=None)
def _dot_case():
    x = clustered(3000, 24, 6, 24, 11)
    x[[7, 500, 1500]] = 0.0
    host = NNDescent(x, metric="dot", n_neighbors=K, random_state=SEED)
    dev = NNDescent(torch.from_numpy(x).to(DEV), metric="dot", n_neighbors=K, random_state=SEED)
    return x, host, dev


def _true_corrected(metric, xs, ids):
    out = np.empty(ids.shape, np.float64)
    for i in range(ids.shape[0]):
        out[i] = MU.alt_dist(metric, xs[i:i + 1], xs[ids[i]])[0]
    return MU.correct(metric, out)


def test_dot_device_build():
    x, host, dev = _dot_case()
    xs = normalize(x, norm="l2")
    truth = MU.brute_knn("dot", xs, k=10)
    recalls = {}
    for name, index in (("host", host), ("device", dev)):
        idx, dist = index.neighbor_graph
        if name == "device":
            assert idx.is_cuda and dist.is_cuda and dist.dtype == torch.float64
            idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        assert (idx >= 0).all()
        np.testing.assert_allclose(dist, _true_corrected("dot", xs, idx), rtol=2e-4, atol=1e-6)
        recalls[name] = MU.recall(truth, idx)
    print("dot 3000 x 24: recall@10 host %.4f device %.4f" % (recalls["host"], recalls["device"]))
    assert abs(recalls["host"] - recalls["device"]) <= 0.01


def test_dot_mirror_is_the_normalised_rows():
    """Within 2 float32 ulp of sklearn's: one rounding from the order of the norm's sum, one from the division.
    Measured on an MI355X: 3 ulp at most with a plain float32 wave sum in k_normalize_rows (two float32 sums in different orders
    are further apart than one rounding), 2 ulp at most with the compensated float32 sum the kernel uses (11645 of 72000 elements
    differ from sklearn's)."""
    x, host, dev = _dot_case()
    want = normalize(x, norm="l2")
    got = dev._raw_data
    assert got.dtype == np.float32 and got.shape == want.shape
    assert _same_bits(host._raw_data, want)
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print("dot mirror: largest distance to sklearn's rows %d ulp, %d of %d elements differ" % (ulps.max(), (ulps > 0).sum(), ulps.size))
    assert ulps.max() <= 2
    assert not got[[7, 500, 1500]].any()  # zero rows stay zero


def test_typed_entry_normalises_dot_like_the_handle_free_conversion():
    """nnd_set_data_device_typed under NND_METRIC_ALT_DOT (float16 rows into the handle's own normalised copy) against
    nnd_device_rows_f32 + nnd_set_data_device (the rows the class keeps): the same graph, bit for bit."""
    x16 = torch.from_numpy(clustered(2001, 23, 6, 24, 12)).to(DEV).half()
    n, d = x16.shape
    graphs = []
    for typed in (True, False):
        b = _capi.Builder(n, d, _capi.METRIC_CODES["dot"], K, 3, 60, 200, K, 8, 0.001, [1, 2, 3], [4, 5, 6])
        try:
            oi = torch.empty((n, K), dtype=torch.int32, device=DEV)
            od = torch.empty((n, K), dtype=torch.float32, device=DEV)
            torch.cuda.synchronize()
            if typed:
                b.set_data_device_typed(x16.data_ptr(), _capi.NND_DTYPE_FLOAT16, keepalive=x16)
            else:
                xn = torch.empty((n, d), dtype=torch.float32, device=DEV)
                _capi.device_rows_f32(0, 0, x16.data_ptr(), _capi.NND_DTYPE_FLOAT16, n, d, True, xn.data_ptr())
                torch.cuda.synchronize()
                b.set_data_device(xn.data_ptr(), keepalive=xn)
            assert not b.data_nonfinite()
            b.build_device(oi.data_ptr(), od.data_ptr())
            b.synchronize()
            graphs.append((oi.cpu().numpy(), od.cpu().numpy()))
        finally:
            b.close()
    _assert_same_graph(graphs[0], graphs[1])
    assert (graphs[0][0] >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "correlation", "proxy_inner_product", "inner_product", "cosine",
                                    "dot", "hellinger"])
def test_neighbor_graph_on_the_device(metric):
    if metric == "dot":
        dev = _dot_case()[2]
    elif metric == "sqeuclidean":
        dev = NNDescent(torch.from_numpy(_data(metric, 3000, 23)).to(DEV), metric=metric, n_neighbors=K, random_state=SEED)
    else:
        dev = _device_index(metric, 3000, 23)
    idx, dist = dev.neighbor_graph
    assert isinstance(idx, torch.Tensor) and isinstance(dist, torch.Tensor)
    assert idx.device == dev._device_graph[0].device == torch.device(DEV) and dist.device == idx.device
    assert idx.dtype == torch.int32 and tuple(idx.shape) == tuple(dist.shape) == (3000, K)
    raw_idx, raw_dist = dev._neighbor_graph
    assert np.array_equal(idx.cpu().numpy(), raw_idx)
    _assert_distances(metric, dist.cpu().numpy(), N._METRICS[metric].correction(raw_dist))
    # a copy, as in the reference: writing into it leaves the index alone
    keep_i, keep_d = idx.clone(), dist.clone()
    idx.fill_(-7)
    dist.zero_()
    again_i, again_d = dev.neighbor_graph
    assert torch.equal(again_i, keep_i) and torch.equal(again_d, keep_d)
    assert np.array_equal(dev._device_graph[0].cpu().numpy(), raw_idx)


@pytest.mark.parametrize("metric", ["euclidean", "sqeuclidean", "inner_product", "cosine", "hellinger"])
def test_corrections_of_special_values(metric):
    """nnd_device_correct on the values a graph can hold: +inf (an unfilled entry), FLT_MAX (no similarity), 0, subnormals."""
    rs = np.random.RandomState(2)
    d = np.concatenate([np.array([0.0, np.inf, MU.FLT_MAX, 1e-45, 1e-38, 3.0e38, 1.0, 2.0, 1e-7, 24.0, 60.0, 1100.0], np.float32),
                        np.abs(rs.standard_normal(100_003)).astype(np.float32) * np.float32(3.0),
                        (rs.uniform(0, 1, 5000) ** 8).astype(np.float32)])
    m = N._METRICS[metric]
    got = N._device_corrected(torch, torch.from_numpy(d).to(DEV), m, 0).cpu().numpy()
    with np.errstate(divide="ignore"):
        host = np.asarray(m.correction(d))
    _assert_distances(metric, got, host)
    assert got[1] == host[1] and got[2] == host[2]


@pytest.mark.parametrize("metric", ["euclidean", "cosine", "inner_product", "hellinger"])
def test_unfilled_entries_map_as_on_the_host(metric):
    x = _data(metric, 8, 5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dev = NNDescent(torch.from_numpy(x).to(DEV), metric=metric, n_neighbors=K, random_state=1)
    idx, dist = dev.neighbor_graph
    raw_idx, raw_dist = dev._neighbor_graph
    assert (raw_idx < 0).any() and np.isinf(raw_dist[raw_idx < 0]).all()
    assert np.array_equal(idx.cpu().numpy(), raw_idx)
    _assert_distances(metric, dist.cpu().numpy(), N._METRICS[metric].correction(raw_dist))


# ---------------------------------------------------------------------------------------------------------------- 5
def test_errors_match_the_host_path():
    x = _data("euclidean", 600, 12)
    bad = x.copy()
    bad[5, 3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        NNDescent(torch.from_numpy(bad).to(DEV), n_neighbors=K)
    bad = x.copy()
    bad[599, 11] = np.inf
    with pytest.raises(ValueError, match="infinity"):
        NNDescent(torch.from_numpy(bad).to(DEV).half(), n_neighbors=K)
    neg = _data("hellinger", 600, 12)
    neg[17, 2] = -0.25
    with pytest.raises(ValueError, match="non-negative"):
        NNDescent(torch.from_numpy(neg).to(DEV), metric="hellinger", n_neighbors=K)
    with pytest.raises(TypeError, match="int32"):
        NNDescent(torch.zeros((600, 12), dtype=torch.int32, device=DEV), n_neighbors=K)
    with pytest.raises(ValueError, match="2D"):
        NNDescent(torch.zeros(600, device=DEV), n_neighbors=K)
    with pytest.raises(ValueError, match="device=1"):  # found before any device work: no second GPU needed
        NNDescent(torch.from_numpy(x).to(DEV), n_neighbors=K, device=1)


def test_warning_when_rows_stay_short():
    x = torch.from_numpy(clustered(8, 5, 3, 2, 1)).to(DEV)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        index = NNDescent(x, n_neighbors=10, random_state=1)
    assert any("Failed to correctly find n_neighbors" in str(m.message) for m in w)
    assert "_neighbor_graph" not in index.__dict__  # decided on the device
    idx, dist = index.neighbor_graph
    assert torch.all((idx >= 0).sum(1) == 8) and torch.isinf(dist[idx < 0]).all()


# ---------------------------------------------------------------------------------------------------------------- 6
@functools.lru_cache(maxsize=None)
def _query_case(metric, quantization):
    x = _data(metric, 2200, 16)
    index = NNDescent(torch.from_numpy(x[:2000]).to(DEV), metric=metric, n_neighbors=K, random_state=SEED, quantization=quantization)
    index.prepare()
    return index, np.ascontiguousarray(x[2000:])


QUERY_CASES = [("euclidean", None), ("cosine", None), ("euclidean", "uint8"), ("proxy_inner_product", None)]


@pytest.mark.parametrize("metric, quantization", QUERY_CASES)
def test_query_with_device_queries(metric, quantization):
    index, q = _query_case(metric, quantization)
    hi, hd = index.query(q, k=K)
    assert isinstance(hi, np.ndarray) and isinstance(hd, np.ndarray)  # a host query on a device-built index: numpy, as ever
    qt = torch.from_numpy(q).to(DEV)
    di, dd = index.query(qt, k=K)
    assert di.is_cuda and dd.is_cuda and di.dtype == torch.int32 and tuple(di.shape) == tuple(dd.shape) == (200, K)
    assert np.array_equal(di.cpu().numpy(), hi) and (hi >= 0).all()
    _assert_distances(metric, dd.cpu().numpy(), hd)
    # float16 queries: converted on the device, the answers of their upcast values
    q16 = qt.half()
    fi, fd = index.query(q16, k=K)
    ui, ud = index.query(q16.float().cpu().numpy(), k=K)
    assert np.array_equal(fi.cpu().numpy(), ui)
    _assert_distances(metric, fd.cpu().numpy(), ud)


def test_zero_query_under_cosine():
    index, q = _query_case("cosine", None)
    q0 = np.zeros((3, 16), np.float32)
    q0[1] = q[0]
    hi, hd = index.query(q0, k=K)
    di, dd = index.query(torch.from_numpy(q0).to(DEV), k=K)
    assert (hi[0] == -1).all() and (hi[2] == -1).all() and (hi[1] >= 0).all()
    assert np.array_equal(di.cpu().numpy(), hi)
    _assert_distances("cosine", dd.cpu().numpy(), hd)


def test_device_queries_on_a_host_built_index():
    x = _data("euclidean", 2200, 16)
    index = NNDescent(x[:2000], n_neighbors=K, random_state=SEED)
    hi, hd = index.query(x[2000:], k=K)
    di, dd = index.query(torch.from_numpy(x[2000:]).to(DEV).double(), k=K)
    assert np.array_equal(di.cpu().numpy(), hi)
    _assert_distances("euclidean", dd.cpu().numpy(), hd)
    with pytest.raises(ValueError, match="shape"):
        index.query(torch.zeros((4, 15), device=DEV), k=K)
    with pytest.raises(TypeError, match="int64"):
        index.query(torch.zeros((4, 16), dtype=torch.int64, device=DEV), k=K)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_mirrors_and_life_cycle():
    x = _data("euclidean", 2200, 16)
    x16 = torch.from_numpy(x[:2000]).to(DEV).half()
    up = x16.float().cpu().numpy()
    q = np.ascontiguousarray(x[2000:2100])
    index = NNDescent(x16, n_neighbors=K, random_state=SEED)
    twin = NNDescent(up, n_neighbors=K, random_state=SEED)
    assert "_raw_data" not in index.__dict__ and hasattr(index, "_raw_data") and "_raw_data" in index.__dict__
    assert index._raw_data.dtype == np.float32 and index._raw_data.flags.c_contiguous and _same_bits(index._raw_data, up)
    assert not hasattr(index, "_no_such_attribute")
    _assert_same_graph(index._neighbor_graph, twin._neighbor_graph)
    assert index.recall(random_state=0) == twin.recall(random_state=0)
    index.prepare()
    twin.prepare()
    qi, qd = index.query(q, k=K)
    ti, td = twin.query(q, k=K)
    assert np.array_equal(qi, ti) and _same_bits(qd, td)
    state = index.__getstate__()
    assert "_device_graph" not in state and "_device_data" not in state and "_searcher" not in state
    assert not any(isinstance(v, torch.Tensor) for v in state.values())
    clone = pickle.loads(pickle.dumps(index))
    ci, cd = clone.query(q, k=K)
    assert np.array_equal(ci, qi) and _same_bits(cd, qd)
    assert isinstance(index.neighbor_graph[0], torch.Tensor)  # pickling left the index itself on the device
    fresh = np.ascontiguousarray(x[2100:2200])
    index.update(xs_fresh=fresh)
    twin.update(xs_fresh=fresh)
    assert index._raw_data.shape == (2100, 16) and "_device_graph" not in index.__dict__ and "_device_data" not in index.__dict__
    gi, gd = index.neighbor_graph  # the host arrays are the index now
    assert isinstance(gi, np.ndarray) and gi.shape == gd.shape == (2100, K) and (gi >= 0).all()
    _assert_same_graph(index._neighbor_graph, twin._neighbor_graph)


def test_compressed_index_keeps_no_graph():
    x = torch.from_numpy(_data("euclidean", 1000, 16)).to(DEV)
    index = NNDescent(x, n_neighbors=K, random_state=SEED, compressed=True)
    assert isinstance(index.neighbor_graph[0], torch.Tensor)
    index.prepare()
    assert not hasattr(index, "_neighbor_graph") and "_device_graph" not in index.__dict__
    with pytest.warns(UserWarning, match="Compressed indexes"):
        assert index.neighbor_graph is None
    qi, _ = index.query(x[:5], k=3)
    assert qi.is_cuda and np.array_equal(qi.cpu().numpy(), index.query(x[:5].cpu().numpy(), k=3)[0])


# ---------------------------------------------------------------------------------------------------------------- 8
def test_input_produced_on_another_stream_needs_no_synchronisation():
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(4)
        heavy = torch.randn((2048, 2048), device=DEV, generator=gen) * 0.02
        for _ in range(30):  # work in front of the rows on the same stream: they are not ready when the constructor is called
            heavy = torch.tanh(heavy @ heavy)
        a = torch.randn((3000, 8), device=DEV, generator=gen)
        b = torch.randn((8, 23), device=DEV, generator=gen)
        x = a @ b + heavy[0, 0] * 0.0
        index = NNDescent(x, n_neighbors=K, random_state=SEED)
        idx, dist = index.neighbor_graph  # stream-ordered for torch consumers: used on the same stream, unsynchronised
        total = (idx >= 0).sum()
    torch.cuda.synchronize()
    assert int(total) == 3000 * K
    host = NNDescent(x.cpu().numpy(), n_neighbors=K, random_state=SEED)
    _assert_same_graph(index._neighbor_graph, host._neighbor_graph)
    assert _same_bits(dist.cpu().numpy(), host.neighbor_graph[1])
