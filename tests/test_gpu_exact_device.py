"""exact_knn on device arrays (torch tensors on the GPU) on a real MI355X: the search runs on the tensor and answers with tensors
-- over all rows, over ``rows``, and for ``queries`` given as a tensor or as a host array -- and computes what the host call
computes from the tensor's float32 values.  dot normalises on the device: within rounding of the host's rows, so it is checked
against float64 instead."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from pynndescent_amd import exact_knn  # noqa: E402
from tests import metric_util as MU  # noqa: E402
from tests.util_data import clustered  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ROWS, N_Q, D = 3000, 257, 23  # 257 queries: one partial query block
FLOAT32_OUT = ("euclidean", "l2", "sqeuclidean", "correlation", "proxy_inner_product")
BIT_METRICS = ("euclidean", "sqeuclidean", "cosine", "correlation", "hellinger", "inner_product")
ROWS = np.sort(np.random.RandomState(5).choice(N_ROWS, N_Q, replace=False)).astype(np.int64)
CASES = [(k, "float32") for k in (1, 10, 64)] + [(10, "float16"), (10, "float64")]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


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


@functools.lru_cache(maxsize=None)
def _tensors(metric, dtype):
    """(data tensor, query tensor) of ``dtype`` on the device, and their float32 values on the host."""
    x = clustered(N_ROWS + N_Q, D, 6, 24, 77, nonneg=metric == "hellinger")
    if metric == "inner_product":
        x = x + np.float32(0.5)
    t = torch.from_numpy(x).to(DEV)
    if dtype == "float64":  # values float32 cannot hold: the rounding to float32 is part of the conversion
        t = t.double() * (1.0 + 1e-9 * torch.from_numpy(np.random.RandomState(3).standard_normal(x.shape)).to(DEV))
    else:
        t = t.to(getattr(torch, dtype))
    data, q = t[:N_ROWS].contiguous(), t[N_ROWS:].contiguous()
    return data, q, np.ascontiguousarray(data.float().cpu().numpy()), np.ascontiguousarray(q.float().cpu().numpy())


def _check_result(idx, dist, metric, shape):
    assert isinstance(idx, torch.Tensor) and isinstance(dist, torch.Tensor)
    assert idx.device == dist.device == torch.device(DEV)
    assert idx.dtype == torch.int32 and dist.dtype == (torch.float32 if metric in FLOAT32_OUT else torch.float64)
    assert tuple(idx.shape) == tuple(dist.shape) == shape
    return idx.cpu().numpy(), dist.cpu().numpy()


@pytest.mark.parametrize("k, dtype", CASES)
@pytest.mark.parametrize("metric", BIT_METRICS)
def test_equals_the_host_search_of_the_float32_values(metric, k, dtype):
    data, q, data_host, q_host = _tensors(metric, dtype)
    runs = [(dict(), dict(), N_ROWS),
            (dict(rows=ROWS), dict(rows=ROWS), N_Q),
            (dict(rows=torch.from_numpy(ROWS).to(DEV)), dict(rows=ROWS), N_Q),
            (dict(queries=q), dict(queries=q_host), N_Q),
            (dict(queries=q_host), dict(queries=q_host), N_Q)]
    for dev_args, host_args, m in runs:
        gi, gd = _check_result(*exact_knn(data, k=k, metric=metric, **dev_args), metric, (m, k))
        hi, hd = exact_knn(data_host, k=k, metric=metric, **host_args)
        assert np.array_equal(gi, hi), sorted(dev_args)
        _assert_distances(metric, gd, hd)


def test_host_data_with_device_queries_answers_on_the_host():
    data, q, data_host, q_host = _tensors("euclidean", "float32")
    gi, gd = exact_knn(data_host, queries=q, k=10)
    hi, hd = exact_knn(data_host, queries=q_host, k=10)
    assert isinstance(gi, np.ndarray) and np.array_equal(gi, hi) and _same_bits(gd, hd)


def test_return_stats():
    data, q, _, _ = _tensors("cosine", "float32")
    idx, dist, stats = exact_knn(data, queries=q, k=10, metric="cosine", return_stats=True)
    assert stats["n_rows"] == N_Q and stats["slices"] >= 1 and 0 <= stats["n_fallback"] <= N_Q and idx.is_cuda and dist.is_cuda


@pytest.mark.parametrize("k, dtype", CASES)
def test_dot_within_rounding_of_float64(k, dtype):
    """dot: the rows and the queries are normalised on the device.  Each returned distance matches the float64 value of the
    returned id, and no returned id is farther than the true k-th neighbour, within the tolerances of the device-array and
    quantized tests (rtol 2e-4, atol 2e-6)."""
    data, q, data_host, q_host = _tensors("dot", dtype)
    unit = lambda a: a.astype(np.float64) / np.linalg.norm(a.astype(np.float64), axis=1, keepdims=True)  # noqa: E731
    xs, qs = unit(data_host), unit(q_host)
    for dev_args, who, m in ((dict(), xs, N_ROWS), (dict(rows=ROWS), xs[ROWS], N_Q), (dict(queries=q), qs, N_Q), (dict(queries=q_host), qs, N_Q)):
        gi, gd = _check_result(*exact_knn(data, k=k, metric="dot", **dev_args), "dot", (m, k))
        truth = MU.correct("dot", MU.alt_dist("dot", who, xs))
        of_returned = np.take_along_axis(truth, gi.astype(np.int64), axis=1)
        np.testing.assert_allclose(gd, of_returned, rtol=2e-4, atol=2e-6)
        kth = np.partition(truth, k - 1, axis=1)[:, k - 1]
        assert (gi >= 0).all() and np.all(of_returned <= kth[:, None] + 2e-6), (of_returned - kth[:, None]).max()
        assert np.all(np.diff(gd, axis=1) >= 0)


def test_errors_are_the_host_path():
    data, q, _, _ = _tensors("euclidean", "float32")
    bad = data.clone()
    bad[5, 3] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        exact_knn(bad, k=5)
    bad_q = q.clone()
    bad_q[256, 22] = float("inf")
    with pytest.raises(ValueError, match="infinity"):
        exact_knn(data, queries=bad_q, k=5)
    pos, pos_q, _, _ = _tensors("hellinger", "float32")
    neg = pos.clone()
    neg[17, 2] = -0.25
    with pytest.raises(ValueError, match="non-negative"):
        exact_knn(neg, k=5, metric="hellinger")
    neg_q = pos_q.clone()
    neg_q[0, 0] = -1.0
    with pytest.raises(ValueError, match="non-negative"):
        exact_knn(pos, queries=neg_q, k=5, metric="hellinger")
    with pytest.raises(NotImplementedError, match="proxy"):
        exact_knn(data, k=5, metric="proxy_inner_product")
    with pytest.raises(NotImplementedError, match="k <= 256"):
        exact_knn(data, k=257)
    with pytest.raises(ValueError, match="k must be in 1"):
        exact_knn(data[:4], k=5)
    with pytest.raises(ValueError, match="not both"):
        exact_knn(data, queries=q, rows=ROWS, k=5)
    with pytest.raises(ValueError, match="rows must be ids"):
        exact_knn(data, rows=[0, N_ROWS], k=5)
    with pytest.raises(ValueError, match="queries must have shape"):
        exact_knn(data, queries=torch.zeros((3, D + 1), device=DEV), k=5)
    with pytest.raises(TypeError, match="int64"):
        exact_knn(data.long(), k=5)
    from pynndescent_amd import _capi

    with pytest.raises(_capi.NNDError, match=r"1 row ids are outside \[0, 3000\)"):  # int32 ids on the device: checked there
        exact_knn(data, rows=torch.tensor([5, N_ROWS, 7], dtype=torch.int32, device=DEV), k=5)
    idx, dist = exact_knn(data, rows=np.zeros(0, np.int64), k=5)  # nothing asked for: empty tensors, no search
    assert tuple(idx.shape) == tuple(dist.shape) == (0, 5) and idx.is_cuda
