"""The host side of update() / exact_knn / recall on device arrays that needs neither a GPU nor torch: how updated_indices are
resolved, the dtype rule, which path an update takes, and that every argument error and the warning come before any library call.
Device arrays are stubs with the attributes the package looks at; ``_capi.Builder`` and ``sharded.build_multi`` are recording
fakes, as in tests/test_host_orchestration_cpu.py."""
import warnings

import numpy as np
import pytest

from pynndescent_amd import _capi, nndescent, sharded
from pynndescent_amd import nndescent as N
from pynndescent_amd.nndescent import NNDescent

N_ROWS, D, K = 120, 6, 5


class _Device:
    def __init__(self, index):
        self.type, self.index = "cuda", index


class StubTensor:
    """A device array as the package sees one, with host values behind it for the calls that bring it down."""

    def __init__(self, array, device=0, dtype=None):
        self.a = np.asarray(array)
        self.shape, self.dtype, self.device, self.is_cuda = self.a.shape, dtype or "torch.%s" % self.a.dtype, _Device(device), True
        self.fetched = 0

    def data_ptr(self):
        return 0x1000

    def is_contiguous(self):
        return True

    def detach(self):
        return self

    def float(self):
        out = StubTensor(self.a.astype(np.float32))
        out.origin = self
        return out

    def cpu(self):
        origin = getattr(self, "origin", self)
        origin.fetched += 1
        return self

    def numpy(self):
        return self.a


def _graph(n, k):
    idx = ((np.arange(n)[:, None] + np.arange(1, k + 1)[None, :]) % n).astype(np.int32)
    return idx, np.tile(np.arange(1, k + 1, dtype=np.float32), (n, 1))


def _x(n=N_ROWS, seed=0):
    return np.random.RandomState(seed).standard_normal((n, D)).astype(np.float32)


def _host_index(**attrs):
    index = NNDescent.from_graph(_x(), *_graph(N_ROWS, K), random_state=3)
    for name, value in attrs.items():
        setattr(index, name, value)
    return index


def _device_index(**attrs):
    """A host-made index dressed as one built from a device array: the tensors in place of the host arrays."""
    index = _host_index(**attrs)
    d = index.__dict__
    d["_device_data"] = StubTensor(d.pop("_raw_data"))
    d["_device_graph"] = tuple(StubTensor(a) for a in d.pop("_neighbor_graph"))
    return index


# ------------------------------------------------------------------------------------------------ the id resolution
@pytest.mark.parametrize("as_array", [False, True], ids=["list", "numpy"])
def test_updated_indices_resolve_like_the_host_loop(as_array):
    n = 10
    given = [3, 5, 3, -1, 5, 0, -10]
    ids, sources = N._resolve_updated_indices(np.array(given) if as_array else given, n)
    assert ids.dtype == sources.dtype == np.int32
    raw = np.full(n, -1)
    for position, i in enumerate(given):  # the host loop (pynndescent_.py:2467-2469): the last write to a row stays
        raw[i] = position
    want = np.flatnonzero(raw >= 0)
    assert np.array_equal(ids, want) and np.array_equal(sources, raw[want])
    assert len(set(ids.tolist())) == len(ids)  # distinct: no two threads write one row
    hit = np.zeros(n, bool)
    hit[given] = True
    assert np.array_equal(np.flatnonzero(hit), ids)


def test_updated_indices_edge_cases():
    ids, sources = N._resolve_updated_indices([], 10)
    assert ids.shape == sources.shape == (0,) and ids.dtype == np.int32
    ids, sources = N._resolve_updated_indices([-10, 9], 10)
    assert ids.tolist() == [0, 9] and sources.tolist() == [0, 1]
    for bad in ([10], [-11], [0, 3, 25]):
        with pytest.raises(IndexError, match=r"index -?\d+ is out of bounds for axis 0 with size 10"):
            N._resolve_updated_indices(bad, 10)
        with pytest.raises(IndexError, match="out of bounds for axis 0 with size 10"):
            np.zeros((10, 2))[bad[-1]] = 1.0  # numpy's own wording


# ------------------------------------------------------------------------------------------------ the dtype rule
def test_dtype_rule():
    assert N._update_dtype(["float16", "float16"]) == "float16"
    assert N._update_dtype(["bfloat16", "bfloat16", "bfloat16"]) == "bfloat16"
    assert N._update_dtype(["float16", "float32"]) == "float32"
    assert N._update_dtype(["float64", "float32"]) == "float32"
    assert N._update_dtype(["float16", "bfloat16"]) == "float32"
    assert N._update_dtype(["float64", "float64"]) == "float64"
    assert N._update_dtype(["float64"]) == "float64"
    assert N._update_dtype(["float32", "float32", "float16"]) == "float32"


# ------------------------------------------------------------------------------------------------ path selection
def test_which_updates_stay_on_the_device():
    fresh_dev, fresh_host = StubTensor(_x(4, 1)), _x(4, 1)
    assert N._updates_on_device(_device_index(), fresh_dev, None)
    assert N._updates_on_device(_device_index(), None, fresh_dev)
    assert N._updates_on_device(_device_index(), fresh_host, fresh_dev)  # a host array beside a tensor is uploaded
    assert not N._updates_on_device(_device_index(), fresh_host, None)  # host arrays take the host path
    assert not N._updates_on_device(_device_index(), None, None)
    assert not N._updates_on_device(_host_index(), fresh_dev, None)  # a host-built index takes the host path
    assert not N._updates_on_device(_device_index(n_devices=2), fresh_dev, None)  # several GPUs: the host path
    half = _device_index()
    del half.__dict__["_device_graph"]  # (a compressed index after prepare(): no graph to start from)
    assert not N._updates_on_device(half, fresh_dev, None)


@pytest.fixture
def rec(monkeypatch):
    """Recording fakes of the two build entries; the device path's first step towards the library (torch) stops the test."""
    calls = []

    class FakeBuilder:
        def __init__(self, n, dim, *args, **kwargs):
            self.n, self.k = int(n), int(args[1])
            calls.append("new")

        def __getattr__(self, name):
            def call(*args):
                calls.append(name)
                if name == "set_data_host":
                    self.x = np.array(args[0], copy=True)
                    FakeBuilder.rows = self.x
                if name == "stats":
                    return {"n_leaves": 7, "n_iters_run": 2}
                if name == "finalize":
                    return _graph(self.n, self.k)
                return False
            return call

    def fake_build_multi(x, *args, **kwargs):
        calls.append("build_multi")
        FakeBuilder.rows = np.array(x, copy=True)
        idx, dist = _graph(x.shape[0], K)
        return idx, dist, {"n_leaves": 9}, {"c": [5]}

    class Stop(Exception):
        pass

    def no_torch():
        calls.append("torch")
        raise Stop()

    monkeypatch.setattr(_capi, "Builder", FakeBuilder)
    monkeypatch.setattr(sharded, "build_multi", fake_build_multi)
    monkeypatch.setattr(nndescent.device_arrays, "_torch", no_torch)
    calls_and_stop = type("Rec", (), {})()
    calls_and_stop.calls, calls_and_stop.Stop, calls_and_stop.builder = calls, Stop, FakeBuilder
    return calls_and_stop


HOST_UPDATE = ["new", "set_data_host", "make_forest", "stats", "reset_graph", "init_from_neighbor_graph", "init_from_leaves",
               "descent", "finalize", "stats", "close"]


def test_host_arrays_on_a_device_built_index_take_the_host_path(rec):
    index = _device_index()
    data = index.__dict__["_device_data"]
    fresh = _x(4, 1)
    index.update(xs_fresh=fresh)
    assert rec.calls == HOST_UPDATE  # ... and torch was never asked for
    assert "_device_data" not in index.__dict__ and "_device_graph" not in index.__dict__ and data.fetched == 1
    assert index._raw_data.shape == (N_ROWS + 4, D) and np.array_equal(index._raw_data[N_ROWS:], fresh)
    assert np.array_equal(rec.builder.rows, index._raw_data)


def test_tensors_on_a_host_built_index_are_brought_to_the_host(rec):
    index = _host_index()
    fresh, updated = StubTensor(_x(4, 1).astype(np.float64)), StubTensor(_x(2, 2).astype(np.float16), dtype="torch.float16")
    index.update(xs_fresh=fresh, xs_updated=updated, updated_indices=StubTensor(np.array([7, -1])))
    assert rec.calls == HOST_UPDATE and fresh.fetched == 1 and updated.fetched == 1
    assert index._raw_data.dtype == np.float32 and index._raw_data.shape == (N_ROWS + 4, D)
    assert np.array_equal(index._raw_data[N_ROWS:], fresh.a.astype(np.float32))
    assert np.array_equal(index._raw_data[7], updated.a[0].astype(np.float32)) and np.array_equal(index._raw_data[-5], updated.a[1].astype(np.float32))


def test_several_gpus_take_the_host_path(rec):
    index = _device_index(n_devices=2, devices=None)
    fresh = StubTensor(_x(4, 1))
    index.update(xs_fresh=fresh)
    assert rec.calls == ["build_multi"] and fresh.fetched == 1
    assert "_device_data" not in index.__dict__ and rec.builder.rows.shape == (N_ROWS + 4, D)


def test_a_tensor_on_a_device_built_index_takes_the_device_path(rec):
    index = _device_index()
    with pytest.raises(rec.Stop):
        index.update(xs_fresh=StubTensor(_x(4, 1)), xs_updated=_x(2, 2), updated_indices=[3, -1])
    assert rec.calls == ["torch"]  # the ids were resolved, then the device work began
    assert "_device_data" in index.__dict__ and index.__dict__["_device_data"].fetched == 0


# ------------------------------------------------------------------------------------------------ errors first
def test_argument_errors_and_the_warning_come_before_any_library_call(rec):
    index = _device_index()
    n_trees = index.n_trees
    rows = StubTensor(_x(2, 2))
    with pytest.raises(ValueError, match="If xs_updated are provided, updated_indices must also be provided!"):
        index.update(xs_updated=rows)
    with pytest.raises(ValueError, match=r"Could not convert updated indices to list of int\(s\)\."):
        index.update(xs_updated=rows, updated_indices=["a", "b"])
    with pytest.raises(ValueError, match=r"Number of updated indices \(3\) must match number of rows of xs_updated \(2\)\."):
        index.update(xs_updated=rows, updated_indices=[1, 2, 3])
    with pytest.raises(IndexError, match="index 120 is out of bounds for axis 0 with size 120"):
        index.update(xs_updated=rows, updated_indices=[1, N_ROWS])
    with pytest.raises(IndexError, match="index -121 is out of bounds"):
        index.update(xs_updated=rows, updated_indices=StubTensor(np.array([-N_ROWS - 1, 0])))
    with pytest.raises(TypeError, match=r"xs_fresh has dtype torch\.int32"):
        index.update(xs_fresh=StubTensor(np.zeros((2, D), np.int32)))
    with pytest.raises(ValueError, match="Expected 2D array, got 1D"):
        index.update(xs_fresh=StubTensor(np.zeros(D, np.float32)))
    with pytest.raises(ValueError, match=r"xs_updated must have shape \(n_rows, 6\)"):
        index.update(xs_updated=StubTensor(_x(2, 2)[:, :5]), updated_indices=[1, 2])
    with pytest.raises(ValueError, match="xs_fresh is on device 1, the index on device 0"):
        index.update(xs_fresh=StubTensor(_x(2, 2), device=1))
    assert rec.calls == [] and index.n_trees == n_trees and index.__dict__["_device_data"].fetched == 0
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with pytest.raises(rec.Stop):
            index.update(xs_fresh=rows, updated_indices=[1, 2])
    assert [str(w.message) for w in caught] == ["xs_updated not provided, while update_indices provided. They will be ignored."]
    assert rec.calls == ["torch"]


def test_exact_knn_checks_come_before_any_library_call(rec):
    data = StubTensor(_x())
    with pytest.raises(ValueError, match="not both"):
        N.exact_knn(data, queries=data, rows=[0], k=3)
    with pytest.raises(NotImplementedError, match="k <= 256"):
        N.exact_knn(data, k=257)
    with pytest.raises(NotImplementedError, match="proxy distance"):
        N.exact_knn(data, k=3, metric="proxy_inner_product")
    with pytest.raises(ValueError, match="Metric is neither callable"):
        N.exact_knn(data, k=3, metric="no-such-metric")
    with pytest.raises(TypeError, match=r"data has dtype torch\.int64"):
        N.exact_knn(StubTensor(np.zeros((9, 3), np.int64)), k=3)
    with pytest.raises(ValueError, match=r"k must be in 1 \.\. n = 120 \(got 121\)"):
        N.exact_knn(data, k=121)
    with pytest.raises(ValueError, match="device=1, but data is on device 0"):
        N.exact_knn(data, k=3, device=1)
    assert rec.calls == []


def test_recall_of_a_device_built_index_goes_to_the_device(rec):
    index = _device_index()
    with pytest.raises(rec.Stop):
        index.recall(k=3)
    assert rec.calls == ["torch"] and index.__dict__["_device_data"].fetched == 0 and "_raw_data" not in index.__dict__
    with pytest.raises(NotImplementedError, match="proxy distance"):
        _device_index(metric="proxy_inner_product").recall()
