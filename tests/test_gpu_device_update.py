"""update(), recall() and init_graph / init_dist on device arrays (torch tensors on the GPU) on a real MI355X: an index built
from a tensor stays on the device through update() and recall(), and computes what its host twin computes.  The twin of every
parity test is ``pickle.loads(pickle.dumps(index))`` taken before the operation: a host index with the same rows, graph and rng
state (pickling prepares the index, on the device; the twin is prepared too).  The builds are deterministic: ids equal,
distances bit-equal."""
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from pynndescent_amd import NNDescent, _capi  # noqa: E402
from tests.util_data import clustered  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 10
SEED = 5
FLOAT32_OUT = ("euclidean", "l2", "sqeuclidean", "correlation", "proxy_inner_product")
MIRRORS = ("_raw_data", "_neighbor_graph", "_search_graph", "_quantized_data")


def _data(metric, n, d, seed=0):
    return clustered(n, d, 6, 24, 40 + d + seed, nonneg=metric == "hellinger")


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


def _device_index(metric, n, d, dtype="float32", **kwargs):
    x = torch.from_numpy(_data(metric, n, d)).to(DEV).to(getattr(torch, dtype))
    return NNDescent(x, metric=metric, n_neighbors=K, random_state=SEED, **kwargs)


def _twin(index):
    return pickle.loads(pickle.dumps(index))


def _device_graph(index):
    return tuple(np.ascontiguousarray(t.cpu().numpy()) for t in index.__dict__["_device_graph"])


def _rows_in_original_order(host_index):
    raw = host_index._raw_data
    return raw[np.argsort(host_index._vertex_order)] if hasattr(host_index, "_vertex_order") else raw


def _assert_on_device_and_equal(index, twin, n_rows, d):
    """The index after a device update: still on the device, no host mirror made, its graph and its rows the twin's."""
    dd = index.__dict__
    assert "_raw_data" not in dd and "_neighbor_graph" not in dd
    assert tuple(dd["_device_data"].shape) == (n_rows, d) and dd["_device_data"].is_cuda
    gi, gd = index.neighbor_graph
    assert isinstance(gi, torch.Tensor) and isinstance(gd, torch.Tensor) and tuple(gi.shape) == (n_rows, K)
    assert "_raw_data" not in dd and "_neighbor_graph" not in dd
    _assert_same_graph(_device_graph(index), twin._neighbor_graph)
    assert _same_bits(dd["_device_data"].float().cpu().numpy(), _rows_in_original_order(twin))
    assert index.n_trees == twin.n_trees
    assert index._build_stats["n_iters_run"] == twin._build_stats["n_iters_run"]


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("d", [16, 23])
@pytest.mark.parametrize("f", [1, 100])
@pytest.mark.parametrize("metric", ["euclidean", "cosine", "correlation", "hellinger", "dot"])
def test_update_with_fresh_tensor_stays_on_the_device(metric, f, d):
    n = 2000
    assert (n + f) % 256 != 0
    index = _device_index(metric, n, d)
    twin = _twin(index)
    fresh = _data(metric, f, d, seed=7)
    index.update(xs_fresh=torch.from_numpy(fresh).to(DEV))
    twin.update(xs_fresh=fresh)
    _assert_on_device_and_equal(index, twin, n + f, d)
    _assert_distances(metric, index.neighbor_graph[1].cpu().numpy(), twin.neighbor_graph[1])


# ---------------------------------------------------------------------------------------------------------------- 2
def _hub_ids(graph_idx, count):
    """The vertices with the highest in-degree: their stale edges sit in many rows."""
    degree = np.bincount(graph_idx[graph_idx >= 0].ravel(), minlength=graph_idx.shape[0])
    return np.argsort(-degree, kind="stable")[:count]


@pytest.mark.parametrize("ids_as_tensor", [False, True], ids=["list", "tensor"])
def test_update_with_updated_rows_and_fresh_rows(ids_as_tensor):
    n, d, f = 2000, 23, 37
    index = _device_index("euclidean", n, d)
    twin = _twin(index)
    old_idx = _device_graph(index)[0]
    hubs = _hub_ids(old_idx, 12)
    ids = [int(v) for v in hubs] + [int(hubs[0]), int(hubs[3]) - n]  # a duplicate (the last wins) and a negative id
    updated = _data("euclidean", len(ids), d, seed=3) + np.float32(0.25)
    fresh = _data("euclidean", f, d, seed=7)
    hit = np.zeros(n, bool)
    hit[ids] = True
    assert hit.sum() == 12
    assert (np.isin(old_idx, np.flatnonzero(hit)).any(1) & ~hit).any()  # stale edges in rows that are not updated themselves
    given = torch.tensor(ids, device=DEV) if ids_as_tensor else ids
    index.update(xs_fresh=torch.from_numpy(fresh).to(DEV), xs_updated=torch.from_numpy(updated).to(DEV), updated_indices=given)
    twin.update(xs_fresh=fresh, xs_updated=updated, updated_indices=ids)
    _assert_on_device_and_equal(index, twin, n + f, d)
    rows = index._device_data.cpu().numpy()
    assert _same_bits(rows[hubs[0]], updated[12]) and _same_bits(rows[hubs[3]], updated[13]) and _same_bits(rows[hubs[1]], updated[1])


def test_updated_host_rows_beside_a_fresh_tensor_are_uploaded():
    n, d = 2000, 16
    index = _device_index("cosine", n, d)
    twin = _twin(index)
    updated, fresh = _data("cosine", 3, d, seed=3), _data("cosine", 5, d, seed=7)
    index.update(xs_fresh=torch.from_numpy(fresh).to(DEV), xs_updated=updated, updated_indices=np.array([4, 1999, -2000]))
    twin.update(xs_fresh=fresh, xs_updated=updated, updated_indices=[4, 1999, -2000])
    _assert_on_device_and_equal(index, twin, n + 5, d)


def test_invalidated_graph_kernel_against_numpy():
    """nnd_device_update_graph on its own: rows of updated ids and every entry that points at one are cleared in place, fresh rows
    are empty; a row that is not updated loses an entry."""
    n, k, n_new = 2001, K, 2001 + 77
    index = _device_index("euclidean", n, 16)
    gi, gd = index._device_graph
    old_i, old_d = _device_graph(index)
    upd = np.unique(np.concatenate([_hub_ids(old_i, 9), [0, n - 1]])).astype(np.int32)
    upd_twice = np.concatenate([upd, upd[:3]])  # (repeats are allowed here: the byte map takes the same store twice)
    ids = torch.from_numpy(upd_twice).to(DEV)
    out_i = torch.full((n_new, k), 12345, dtype=torch.int32, device=DEV)
    out_d = torch.full((n_new, k), 7.0, dtype=torch.float32, device=DEV)
    scratch = torch.empty((n,), dtype=torch.uint8, device=DEV)
    _capi.device_update_graph(0, torch.cuda.current_stream().cuda_stream, gi.data_ptr(), gd.data_ptr(), n, k, ids.data_ptr(), ids.shape[0], n_new,
                              scratch.data_ptr(), out_i.data_ptr(), out_d.data_ptr())
    hit = np.zeros(n, bool)
    hit[upd] = True
    want_i = np.full((n_new, k), -1, np.int32)
    want_d = np.full((n_new, k), np.inf, np.float32)
    want_i[:n], want_d[:n] = old_i, old_d
    want_i[:n][hit], want_d[:n][hit] = -1, np.inf
    stale = np.zeros((n_new, k), bool)
    stale[:n] = (old_i >= 0) & hit[np.clip(old_i, 0, None)]
    want_i[stale], want_d[stale] = -1, np.inf
    _assert_same_graph((out_i.cpu().numpy(), out_d.cpu().numpy()), (want_i, want_d))
    lost = (stale[:n] & ~hit[:, None]).any(1)
    assert lost.any() and np.array_equal(scratch.cpu().numpy().astype(bool), hit)
    assert np.array_equal(_device_graph(index)[0], old_i)  # the old graph is read, not written


def test_out_of_range_id_raises_and_leaves_the_index_alone():
    n, d = 2000, 16
    index = _device_index("euclidean", n, d)
    data, graph, n_trees = index._device_data, index._device_graph, index.n_trees
    rows = torch.from_numpy(_data("euclidean", 2, d, seed=3)).to(DEV)
    for bad in ([5, n], [-n - 1, 5]):
        with pytest.raises(IndexError, match="out of bounds"):
            index.update(xs_updated=rows, updated_indices=bad)
        assert index._device_data is data and index._device_graph is graph and index.n_trees == n_trees
    with pytest.raises(ValueError, match="must match"):
        index.update(xs_updated=rows, updated_indices=[1])
    with pytest.raises(ValueError, match="updated_indices must also be provided"):
        index.update(xs_updated=rows)
    with pytest.raises(ValueError, match="shape"):
        index.update(xs_fresh=torch.zeros((3, d + 1), device=DEV))
    assert index._device_data is data and index._device_graph is graph and index.n_trees == n_trees


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("index_dtype, fresh_dtype, kept", [("float16", "float16", "float16"), ("float16", "float32", "float32"),
                                                           ("float64", "float32", "float32"), ("bfloat16", "bfloat16", "bfloat16")])
def test_dtype_rule(index_dtype, fresh_dtype, kept):
    n, d, f = 2000, 23, 45
    index = _device_index("euclidean", n, d, dtype=index_dtype)
    twin = _twin(index)
    fresh = torch.from_numpy(_data("euclidean", f + 2, d, seed=7)).to(DEV).to(getattr(torch, fresh_dtype))
    index.update(xs_fresh=fresh[:f], xs_updated=fresh[f:], updated_indices=[17, 1999])
    up = fresh.float().cpu().numpy()  # what a host twin holds: float32(everything)
    twin.update(xs_fresh=up[:f], xs_updated=up[f:], updated_indices=[17, 1999])
    assert index._device_data.dtype == getattr(torch, kept)
    _assert_on_device_and_equal(index, twin, n + f, d)


@pytest.mark.parametrize("index_dtype, fresh_dtype", [("float32", "float32"), ("float16", "float16"), ("float32", "float16")])
def test_rows_off_the_vector_grid(index_dtype, fresh_dtype):
    """n_old * d * element size is no multiple of 16, so the fresh rows land on a destination that is not 16-byte aligned (element
    stores), and the fresh rows are a view that starts in the middle of an allocation (the scalar head of the source)."""
    n, d, f = 2001, 23, 45
    index = _device_index("euclidean", n, d, dtype=index_dtype)
    twin = _twin(index)
    base = torch.from_numpy(_data("euclidean", f + 3, d, seed=7)).to(DEV).to(getattr(torch, fresh_dtype))
    fresh, updated = base[1:f + 1], base[f + 1:]
    out_size = 2 if index_dtype == fresh_dtype == "float16" else 4
    assert fresh.is_contiguous() and fresh.data_ptr() % 16 != 0 and (n * d * out_size) % 16 != 0
    index.update(xs_fresh=fresh, xs_updated=updated, updated_indices=[2000, 0])
    up = base.float().cpu().numpy()
    twin.update(xs_fresh=up[1:f + 1], xs_updated=up[f + 1:], updated_indices=[2000, 0])
    assert index._device_data.dtype == getattr(torch, "float16" if out_size == 2 else "float32")
    _assert_on_device_and_equal(index, twin, n + f, d)


def test_rebuild_that_raises_changes_nothing():
    n, d = 2000, 16
    index = _device_index("euclidean", n, d)
    data, graph, n_trees = index._device_data, index._device_graph, index.n_trees
    bad = torch.from_numpy(_data("euclidean", 3, d, seed=7)).to(DEV)
    bad[1, 2] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        index.update(xs_fresh=bad)
    assert index._device_data is data and index._device_graph is graph and index.n_trees == n_trees
    assert n_trees != index.n_trees_after_update  # (the assertion above tells something)


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("metric, quantization", [("euclidean", None), ("cosine", None), ("euclidean", "uint8")])
def test_prepared_index_is_prepared_again_on_the_device(metric, quantization):
    n, d, f = 2000, 16, 100
    x = _data(metric, n + f + 150, d)
    index = NNDescent(torch.from_numpy(x[:n]).to(DEV), metric=metric, n_neighbors=K, random_state=SEED, quantization=quantization)
    index.prepare()
    twin = _twin(index)
    index.update(xs_fresh=torch.from_numpy(x[n:n + f]).to(DEV))
    twin.update(xs_fresh=np.ascontiguousarray(x[n:n + f]))
    assert "_device_search_graph" in index.__dict__ and "_device_order" in index.__dict__
    _assert_on_device_and_equal(index, twin, n + f, d)
    q = np.ascontiguousarray(x[n + f:])
    qi, qd = index.query(q, k=K)
    ti, td = twin.query(q, k=K)
    assert np.array_equal(qi, ti) and _same_bits(qd, td) and (qi >= 0).all()
    assert "_raw_data" not in index.__dict__ and "_neighbor_graph" not in index.__dict__


# ---------------------------------------------------------------------------------------------------------------- 5
def test_two_updates_in_a_row():
    n, d = 2000, 16
    x = _data("euclidean", n + 120, d)
    index = NNDescent(torch.from_numpy(x[:n]).to(DEV), n_neighbors=K, random_state=SEED)
    twin = _twin(index)
    index.update(xs_fresh=torch.from_numpy(x[n:n + 50]).to(DEV))
    index.update(xs_fresh=torch.from_numpy(x[n + 50:]).to(DEV), xs_updated=torch.from_numpy(x[:2] + np.float32(1)).to(DEV),
                 updated_indices=[n + 10, 3])  # (a row of the first update is updated by the second)
    twin.update(xs_fresh=np.ascontiguousarray(x[n:n + 50]))
    twin.update(xs_fresh=np.ascontiguousarray(x[n + 50:]), xs_updated=x[:2] + np.float32(1), updated_indices=[n + 10, 3])
    _assert_on_device_and_equal(index, twin, n + 120, d)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_host_arrays_still_make_a_host_index():
    n, d, f = 2000, 16, 100
    index = _device_index("euclidean", n, d)
    twin = _twin(index)
    fresh = _data("euclidean", f, d, seed=7)
    index.update(xs_fresh=fresh)
    twin.update(xs_fresh=fresh)
    assert "_device_data" not in index.__dict__ and "_device_graph" not in index.__dict__
    gi, gd = index.neighbor_graph
    assert isinstance(gi, np.ndarray) and gi.shape == (n + f, K)
    _assert_same_graph(index._neighbor_graph, twin._neighbor_graph)
    # ... and a tensor given to a host index is brought to the host, where it was an error
    more = _data("euclidean", 7, d, seed=9)
    index.update(xs_fresh=torch.from_numpy(more).to(DEV))
    twin.update(xs_fresh=more)
    assert "_device_data" not in index.__dict__
    _assert_same_graph(index._neighbor_graph, twin._neighbor_graph)


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_recall_on_the_device(metric):
    n, d = 2000, 16
    x = _data(metric, n + 100, d)
    index = NNDescent(torch.from_numpy(x[:n]).to(DEV).half(), metric=metric, n_neighbors=K, random_state=SEED)

    def recalls(ix):
        return [ix.recall(k=1, n_rows=300, random_state=0), ix.recall(k=10, n_rows=5000, random_state=1), ix.recall(random_state=2)]

    def no_mirror(ix):
        return not any(name in ix.__dict__ for name in MIRRORS)

    before = recalls(index)
    assert no_mirror(index) and not index._prepared
    twin = _twin(index)  # (prepares the index, on the device, and fetches the mirrors for the pickle)
    for name in MIRRORS:
        index.__dict__.pop(name, None)
    assert index._prepared and "_device_search_graph" in index.__dict__
    after = recalls(index)
    assert no_mirror(index)
    want = recalls(twin)
    print("recall %s: %s" % (metric, want))
    assert before == want and after == want and 0.5 < want[1] <= 1.0
    fresh = np.ascontiguousarray(x[n:])
    index.update(xs_fresh=torch.from_numpy(fresh).to(DEV))
    twin.update(xs_fresh=fresh)
    assert recalls(index) == recalls(twin) and no_mirror(index)


def test_recall_hits_kernel_against_numpy():
    """nnd_device_recall_hits on its own: rows wider than a wave, ids that repeat in a graph row, empty entries, k = 1 and 256."""
    rs = np.random.RandomState(3)
    n, width, m = 700, 256, 333
    graph = rs.randint(-1, n, size=(n, width)).astype(np.int32)
    rows = rs.choice(n, m, replace=False).astype(np.int32)
    for k in (1, 10, 256):
        true = np.stack([rs.choice(n, k, replace=False) for _ in range(m)]).astype(np.int32)
        want = sum(int(np.isin(t, a).sum()) for t, a in zip(true, graph[rows]))
        hits = torch.full((1,), -5, dtype=torch.int64, device=DEV)
        t_dev, g_dev, r_dev = (torch.from_numpy(a).to(DEV) for a in (true, graph, rows))
        _capi.device_recall_hits(0, torch.cuda.current_stream().cuda_stream, t_dev.data_ptr(), m, k, g_dev.data_ptr(), n, width, r_dev.data_ptr(),
                                 hits.data_ptr())
        assert int(hits.item()) == want and want > 0


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize("with_dist", [False, True], ids=["ids", "ids+dist"])
def test_init_graph_tensors_seed_the_build_on_the_device(with_dist, monkeypatch):
    n, d = 2001, 23
    x = _data("euclidean", n, d)
    rs = np.random.RandomState(1)
    g = rs.randint(0, n, size=(n, K)).astype(np.int64)
    g[5, 3] = -1
    gd = ((x[:, None, :] - x[np.clip(g, 0, None)]) ** 2).sum(-1).astype(np.float32) if with_dist else None
    calls = []
    real = _capi.Builder.init_from_graph_device
    monkeypatch.setattr(_capi.Builder, "init_from_graph_device", lambda self, *a: (calls.append(a), real(self, *a))[1])
    monkeypatch.setattr(_capi.Builder, "init_from_graph", lambda self, *a: pytest.fail("the init graph went through the host"))
    dev = NNDescent(torch.from_numpy(x).to(DEV), n_neighbors=K, random_state=SEED, init_graph=torch.from_numpy(g).to(DEV),
                    init_dist=None if gd is None else torch.from_numpy(gd).to(DEV).double())
    monkeypatch.undo()
    assert len(calls) == 1 and calls[0][2] == K and bool(calls[0][1]) == with_dist
    host = NNDescent(x, n_neighbors=K, random_state=SEED, init_graph=g, init_dist=gd)
    _assert_same_graph(_device_graph(dev), host._neighbor_graph)
    assert not dev.tree_init and dev._rp_forest is None
    with pytest.raises(ValueError, match="Init graph size does not match"):
        NNDescent(torch.from_numpy(x).to(DEV), n_neighbors=K, init_graph=torch.from_numpy(g[:-1]).to(DEV))
    with pytest.raises(ValueError, match="shapes of init graph and init distances"):
        NNDescent(torch.from_numpy(x).to(DEV), n_neighbors=K, init_graph=torch.from_numpy(g).to(DEV),
                  init_dist=torch.zeros((n, K + 1), device=DEV))
