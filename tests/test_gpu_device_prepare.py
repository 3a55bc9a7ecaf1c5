"""prepare() of an index built from a device array, on a real MI355X: it runs from the device tensors (no host mirror appears),
it leaves the index the host path leaves bit for bit (the ``_host_prepare`` switch sends a twin through that path on one and the
same graph), the reorder kernels and the hub rank alone against scipy / numpy on shapes no small index produces, the life cycle
after a device prepare, and the stream rule."""
import functools
import pickle

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import scipy.sparse as sp  # noqa: E402

from pynndescent_amd import NNDescent, _capi  # noqa: E402
from pynndescent_amd.search_tree import FlatTree, reorder_by_tree  # noqa: E402
from tests.util_data import clustered  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 10
SEED = 5
NQ = 100


def _data(metric, n, d):
    x = clustered(n, d, 6, 24, 40 + d, nonneg=metric == "hellinger")
    if metric in ("inner_product", "proxy_inner_product"):
        x = x + np.float32(0.5)
    return x


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same_answers(got, want):
    """Query answers of one kernel on one and the same index state: ids equal, distances by bits."""
    gi, gd = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got)
    wi, wd = (t.cpu().numpy() if isinstance(t, torch.Tensor) else t for t in want)
    return np.array_equal(gi, wi) and _same_bits(gd, wd)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_nothing_comes_to_the_host(dtype):
    x = _data("euclidean", 2000 + NQ, 16)
    t = torch.from_numpy(x).to(DEV).to(dtype)
    index = NNDescent(t[:2000].contiguous(), n_neighbors=K, random_state=SEED)
    index.prepare()
    idx, dist = index.query(t[2000:].contiguous(), k=K)
    for name in ("_raw_data", "_neighbor_graph", "_search_graph"):
        assert name not in index.__dict__, name
    assert isinstance(idx, torch.Tensor) and isinstance(dist, torch.Tensor) and idx.is_cuda and dist.is_cuda
    assert tuple(idx.shape) == tuple(dist.shape) == (NQ, K) and bool((idx >= 0).all())
    assert index._device_data.data_ptr() == t.data_ptr()  # the caller's tensor, by reference, in its original order
    assert index._vertex_order.shape == (2000,) and index._min_distance.dtype == np.float32 and index._visited.shape == (251,)


# ---------------------------------------------------------------------------------------------------------------- 2
CASES = {
    "euclidean": dict(metric="euclidean"),
    "cosine": dict(metric="cosine"),
    "dot": dict(metric="dot"),
    "correlation": dict(metric="correlation"),
    "hellinger": dict(metric="hellinger"),
    "proxy_inner_product": dict(metric="proxy_inner_product"),
    "float16": dict(metric="euclidean", half=True),
    "d23": dict(metric="euclidean", d=23),  # padding columns, rows that start off a 16-byte boundary
    "d3": dict(metric="euclidean", d=3),
    "degree_aware": dict(metric="euclidean", diversify_method="degree_aware"),
    "n65": dict(metric="euclidean", n=65),  # the default search leaf size (30): a tree of a few leaves
    "n40_one_leaf": dict(metric="euclidean", n=40, search_tree_leaf_size=64),  # one leaf: the identity order
    "no_tree": dict(metric="euclidean", tree_init=False),
    "compressed": dict(metric="euclidean", compressed=True),
    # CSR rows beyond 128 entries, up to round(1.5 * 200) = 300: no edge is diversified away (with the default probability the
    # pruned rows of this set stay below 20 entries), so the union of a row's 200 neighbours and its reverse edges meets the degree cut
    "k200": dict(metric="euclidean", n=3000, d=8, n_neighbors=200, diversify_prob=0.0),
    "uint8_euclidean": dict(metric="euclidean", quantization="uint8"),
    "uint8_cosine": dict(metric="cosine", quantization="uint8"),
}


@functools.lru_cache(maxsize=None)
def _prepared_pair(case):
    """Two indexes from one tensor and seed, one prepared on the device and its twin through the host-path switch, and queries."""
    kw = dict(CASES[case])
    n, d, half = kw.pop("n", 2000), kw.pop("d", 16), kw.pop("half", False)
    kw.setdefault("n_neighbors", K)
    x = _data(kw["metric"], n + NQ, d)
    t = torch.from_numpy(x).to(DEV)
    if half:
        t = t.half()
    rows, q = t[:n].contiguous(), t[n:].contiguous()
    dev = NNDescent(rows, random_state=SEED, **kw)
    twin = NNDescent(rows, random_state=SEED, **kw)
    twin._host_prepare = True
    assert torch.equal(dev._device_graph[0], twin._device_graph[0])
    assert _same_bits(dev._device_graph[1].cpu().numpy(), twin._device_graph[1].cpu().numpy())
    dev.prepare()
    twin.prepare()
    return dev, twin, q


@pytest.mark.parametrize("case", sorted(CASES))
def test_same_index_as_the_host_path(case):
    dev, twin, q = _prepared_pair(case)
    n = dev._device_data.shape[0]
    assert "_device_search_graph" in dev.__dict__ and "_device_search_graph" not in twin.__dict__  # each took its path
    assert np.array_equal(dev._vertex_order, twin._vertex_order)
    if case == "n40_one_leaf":
        assert np.array_equal(dev._vertex_order, np.arange(n))
    g, h = dev._search_graph, twin._search_graph
    assert g.shape == h.shape == (n, n) and g.data.dtype == np.uint8 and (g.data == 1).all() and g.has_sorted_indices
    assert np.array_equal(g.indptr, h.indptr) and np.array_equal(g.indices, h.indices)
    if case == "k200":
        # (degree_prune keeps the entries <= sorted(row)[300], pynndescent_.py:728-738: 301 of them, more with ties; 384 is what a
        # wave of the reorder kernel stages in LDS)
        assert 128 < np.diff(g.indptr).max() <= 384
    assert len(dev._search_forest) == len(twin._search_forest) == (0 if case == "no_tree" else 1)
    for a, b in zip(dev._search_forest, twin._search_forest):
        for name in ("hyperplanes", "offsets", "children", "indices"):
            assert _same_bits(getattr(a, name), getattr(b, name)), name
        assert a.leaf_size == b.leaf_size
    assert _same_bits(np.float32(dev._min_distance), np.float32(twin._min_distance))
    assert dev._visited.shape == twin._visited.shape
    assert _same_bits(dev._raw_data, twin._raw_data)  # the mirror: the rows in tree order, float32
    if case != "dot":  # still the caller's tensor (dot: each index's own normalised copy, in the original order)
        assert dev._device_data.data_ptr() == twin._device_data.data_ptr()
    if case.startswith("uint8"):
        assert _same_bits(dev._quantized_values, twin._quantized_values)
        assert "_quantized_data" not in dev.__dict__
        assert _same_bits(dev._quantized_data, twin._quantized_data)
    qh = np.ascontiguousarray(q.float().cpu().numpy())
    assert _same_answers(dev.query(qh, k=K), twin.query(qh, k=K))
    di, dd = dev.query(q, k=K)
    assert isinstance(di, torch.Tensor) and _same_answers((di, dd), twin.query(q, k=K))
    assert bool((di >= 0).all())


# ---------------------------------------------------------------------------------------------------------------- 3
ROW_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 383, 384)


@functools.lru_cache(maxsize=None)
def _synthetic_csr(n=1000):
    rs = np.random.RandomState(11)
    lens = rs.choice(ROW_LENGTHS, size=n)
    lens[:7] = 0  # runs of empty rows at both ends
    lens[-5:] = 0
    lens[7:7 + len(ROW_LENGTHS)] = ROW_LENGTHS  # every length at least once
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([rs.choice(n, size=L, replace=False) for L in lens]).astype(np.int32)  # columns without repetition, unsorted
    return indptr, indices


@pytest.mark.parametrize("order_kind", ["random", "identity", "reversal"])
@pytest.mark.parametrize("d", [1, 3, 4, 100, 129])
def test_reorder_entry_against_scipy(order_kind, d):
    n = 1000
    indptr, indices = _synthetic_csr(n)
    rs = np.random.RandomState(100 + d)
    order = {"random": rs.permutation(n), "identity": np.arange(n), "reversal": np.arange(n)[::-1]}[order_kind].astype(np.int32)
    # rows of distinct bit patterns (finite floats, so that the bytes are what is compared and nothing else can be meant)
    x = (np.arange(n * d, dtype=np.uint32) * np.uint32(2654435761) % np.uint32(0x7F000000)).reshape(n, d).view(np.float32)
    x = np.ascontiguousarray(x)
    graph = sp.csr_array((np.ones(indices.shape[0], np.uint8), indices, indptr), shape=(n, n))
    want_g, want_x, want_order, _ = reorder_by_tree(graph, x, FlatTree(None, None, None, order, 0))
    got_ptr, got_ind, got_x = _capi.reorder_host(order, indptr, indices, x)
    assert np.array_equal(got_ptr, want_g.indptr) and np.array_equal(got_ind, want_g.indices)
    dp = (d + 3) & ~3
    assert got_x.shape == (n, dp) and _same_bits(got_x[:, :d], want_x)
    assert not got_x[:, d:].view(np.uint32).any()  # zeroed padding columns
    if order_kind == "identity":  # and the entry's own identity (no permutation handed in): the graph as it is, rows padded
        ptr2, ind2, x2 = _capi.reorder_host(None, indptr, indices, x)
        assert np.array_equal(ptr2, indptr) and np.array_equal(ind2, indices) and _same_bits(x2, got_x)


def test_reorder_entry_rejects_what_it_would_index_with():
    indptr, indices = _synthetic_csr(1000)
    x = np.zeros((1000, 4), np.float32)
    bad = np.arange(1000, dtype=np.int32)
    bad[3] = 4
    with pytest.raises(_capi.NNDError, match="permutation"):
        _capi.reorder_host(bad, indptr, indices, x)
    cols = indices.copy()
    cols[10] = 1000
    with pytest.raises(_capi.NNDError, match="outside"):
        _capi.reorder_host(None, indptr, cols, x)


# ---------------------------------------------------------------------------------------------------------------- 4
def _rank_cases():
    rs = np.random.RandomState(3)
    ties = rs.randint(0, 50, size=(500, 10)).astype(np.int32)  # ids 0..49 only: every other id ties at degree 0
    holes = rs.randint(0, 300, size=(300, 15)).astype(np.int32)
    holes[rs.uniform(size=holes.shape) < 0.3] = -1
    holes[5, 2] = 300  # an id past the end is skipped like a negative one
    hub = rs.randint(0, 2000, size=(2000, 10)).astype(np.int32)
    hub[::3, 0] = 1234  # one id of degree far above k
    return {"ties": ties, "holes": holes, "hub": hub, "n65": rs.randint(0, 65, size=(65, 5)).astype(np.int32),
            "n4097": rs.randint(0, 4097, size=(4097, 7)).astype(np.int32)}


@pytest.mark.parametrize("case", ["ties", "holes", "hub", "n65", "n4097"])
def test_degrees_and_rank(case):
    idx = _rank_cases()[case]
    n, k = idx.shape
    t = torch.from_numpy(idx).to(DEV)
    out = torch.empty((n,), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    _capi.rank_order_device(0, 0, t.data_ptr(), n, k, out.data_ptr())
    valid = idx[(idx >= 0) & (idx < n)]
    want = np.argsort(-np.bincount(valid.ravel(), minlength=n)[:n], kind="stable")
    assert np.array_equal(out.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_life_cycle_after_a_device_prepare():
    x = _data("euclidean", 2200, 16)
    t = torch.from_numpy(x[:2000]).to(DEV)
    q = np.ascontiguousarray(x[2000:2100])
    index = NNDescent(t, n_neighbors=K, random_state=SEED)
    twin = NNDescent(t, n_neighbors=K, random_state=SEED)
    twin._host_prepare = True
    index.prepare()
    twin.prepare()
    with pytest.raises(RuntimeError, match="prepared already"):
        index.build_search_graph()
    # a host query on the device-prepared index: numpy, equal to the tensor answers
    hi, hd = index.query(q, k=K)
    di, dd = index.query(torch.from_numpy(q).to(DEV), k=K)
    assert isinstance(hi, np.ndarray) and isinstance(hd, np.ndarray) and di.is_cuda
    assert np.array_equal(di.cpu().numpy(), hi) and _same_bits(dd.cpu().numpy(), hd)
    assert "_raw_data" not in index.__dict__ and "_search_graph" not in index.__dict__
    # pickle: the mirrors travel, the tensors stay
    state = index.__getstate__()
    assert not any(isinstance(v, torch.Tensor) or (isinstance(v, tuple) and any(isinstance(e, torch.Tensor) for e in v)) for v in state.values())
    clone = pickle.loads(pickle.dumps(index))
    assert _same_answers(clone.query(q, k=K), (hi, hd))
    assert isinstance(index.neighbor_graph[0], torch.Tensor) and "_device_search_graph" in index.__dict__
    assert _same_answers(index.query(q, k=K), (hi, hd))
    assert index.recall(random_state=0) == twin.recall(random_state=0)
    # update(): the host arrays become the index, on both
    fresh = np.ascontiguousarray(x[2100:2200])
    index.update(xs_fresh=fresh)
    twin.update(xs_fresh=fresh)
    for name in ("_device_graph", "_device_data", "_device_order", "_device_search_graph"):
        assert name not in index.__dict__, name
    assert index._raw_data.shape == (2100, 16)
    assert np.array_equal(index._neighbor_graph[0], twin._neighbor_graph[0]) and _same_bits(index._neighbor_graph[1], twin._neighbor_graph[1])
    assert _same_answers(index.query(q, k=K), twin.query(q, k=K))


# ---------------------------------------------------------------------------------------------------------------- 6
def test_prepare_and_query_on_another_stream_need_no_synchronisation():
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gen = torch.Generator(device=DEV)
        gen.manual_seed(4)
        heavy = torch.randn((2048, 2048), device=DEV, generator=gen) * 0.02
        for _ in range(30):  # work in front of the rows on the same stream: they are not ready when the constructor is called
            heavy = torch.tanh(heavy @ heavy)
        a = torch.randn((3000 + NQ, 8), device=DEV, generator=gen)
        b = torch.randn((8, 23), device=DEV, generator=gen)
        xq = a @ b + heavy[0, 0] * 0.0
        x, q = xq[:3000].contiguous(), xq[3000:].contiguous()
        index = NNDescent(x, n_neighbors=K, random_state=SEED)
        index.prepare()
        idx, dist = index.query(q, k=K)  # stream-ordered for torch consumers: used on the same stream, unsynchronised
        found = (idx >= 0).sum()
    torch.cuda.synchronize()
    assert int(found) == NQ * K and "_raw_data" not in index.__dict__
    ref = NNDescent(x, n_neighbors=K, random_state=SEED)  # everything complete, on the default stream
    ref.prepare()
    assert np.array_equal(ref._vertex_order, index._vertex_order)
    assert _same_answers((idx, dist), ref.query(q, k=K))
